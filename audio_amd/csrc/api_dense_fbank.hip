// Dense filterbank projection of the C ABI (csrc/dense_fbank.h): exported tile constants and the one launch.
#include "api_common.h"
#include "dense_fbank.h"

using namespace aamd;

extern "C" {

int32_t aamd_dense_fbank_tiles(int32_t which) {
  return which == 0 ? dfb::kFrames : (which == 1 ? dfb::kTileK : (which == 2 ? dfb::kMaxN : (which == 3 ? dfb::kMaxK : 0)));
}

int aamd_dense_fbank(int32_t dtype, const void* x, const float* w, void* out, int64_t rows, int64_t frames,
                     int64_t stride_row, int64_t stride_freq, int64_t stride_frame, int32_t n_freqs, int32_t n_out,
                     void* stream) {
  DeviceScope dev_scope_(x);
  static_assert(dfb::kMaxN == AAMD_DENSE_FBANK_MAX_OUT && dfb::kMaxK == AAMD_DENSE_FBANK_MAX_FREQS,
                "the header's limits are the kernel's");
  AAMD_CHECK_ARG(dtype == AAMD_SA_F32 || dtype == AAMD_SA_F16 || dtype == AAMD_SA_BF16,
                 "dense_fbank: float32, float16 or bfloat16 elements");
  AAMD_CHECK_ARG(rows >= 0 && frames >= 0 && n_freqs >= 1 && n_out >= 1, "dense_fbank: bad sizes");
  if (n_out > AAMD_DENSE_FBANK_MAX_OUT)
    return fail(AAMD_EUNSUPPORTED, "audio_amd: dense_fbank: the kernel serves up to 128 outputs");
  if (n_freqs > AAMD_DENSE_FBANK_MAX_FREQS)
    return fail(AAMD_EUNSUPPORTED, "audio_amd: dense_fbank: the kernel serves up to 4097 frequency bins");
  AAMD_CHECK_ARG(stride_row >= 0 && stride_freq >= 1 && stride_frame >= 1, "dense_fbank: strides must be positive");
  AAMD_CHECK_ARG(stride_freq == 1 || stride_frame == 1 || n_freqs == 1 || frames <= 1,
                 "dense_fbank: the input needs unit stride along freq or along time");
  if (rows == 0 || frames == 0) return AAMD_OK;
  const int64_t tiles = dfb::tiles_per_row(frames);
  AAMD_CHECK_ARG(rows < (1ll << 31) && frames < (1ll << 40) && rows * tiles < (1ll << 31), "dense_fbank: too many rows or frames");
  AAMD_CHECK_ARG(x && w && out, "null buffer");
  const int es = dtype == AAMD_SA_F32 ? 4 : 2;
  AAMD_CHECK_ARG(((uintptr_t)x & (uintptr_t)(es - 1)) == 0, "dense_fbank: the input is not aligned to its element");
  // (a lane stores 4 consecutive outputs in one access where n_out % 4 == 0)
  AAMD_CHECK_ARG(((uintptr_t)out & (uintptr_t)((n_out % 4 == 0 ? 4 : 1) * es - 1)) == 0, "dense_fbank: the output is not aligned");
  AAMD_CHECK_ARG(((uintptr_t)w & 15) == 0, "dense_fbank: the filterbank's image must be 16-byte aligned");
  dfb::Args a{};
  a.x = x; a.W = w; a.out = out;
  a.rows = rows; a.T = frames; a.sr = rows > 1 ? stride_row : 0; a.sk = stride_freq; a.st = stride_frame;
  a.K = n_freqs; a.N = n_out;
  a.time_major = (stride_freq == 1 || n_freqs == 1) ? 0 : 1;
  const size_t lds = (size_t)dfb::lds_floats(n_out) * sizeof(float);     // 20 .. 48 KB
  hipStream_t s = (hipStream_t)stream;
  const bool small = dfb::n_tiles(n_out) <= dfb::kSmallNT;
#define AAMD_DFB_LAUNCH(DT)                                                                                    \
  return small ? launch(dfb::dense_fbank_kernel<DT, true>, rows * tiles, dfb::kThreads, lds, s, a, tiles)       \
               : launch(dfb::dense_fbank_kernel<DT, false>, rows * tiles, dfb::kThreads, lds, s, a, tiles)
  switch (dtype) {
    case AAMD_SA_F32: AAMD_DFB_LAUNCH(wa::kF32);
    case AAMD_SA_F16: AAMD_DFB_LAUNCH(wa::kF16);
    default: AAMD_DFB_LAUNCH(wa::kBF16);
  }
#undef AAMD_DFB_LAUNCH
}

}  // extern "C"
