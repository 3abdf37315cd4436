// InverseMelScale of the C ABI (csrc/inverse_mel.h): exported tile constants and the one launch.
#include "api_common.h"
#include "inverse_mel.h"

using namespace aamd;

extern "C" {

int32_t aamd_inverse_mel_tiles(int32_t which) {
  return which == 0 ? iml::kFrames : (which == 1 ? iml::kBins : (which == 2 ? iml::kMaxMels : 0));
}

int aamd_inverse_mel(int32_t dtype, const void* x, const float* pinv, void* out, int64_t rows, int64_t frames,
                     int64_t stride_row, int64_t stride_mel, int64_t stride_frame, int32_t n_stft, int32_t n_mels,
                     int32_t log_input, void* stream) {
  DeviceScope dev_scope_(x);
  static_assert(iml::kMaxMels == AAMD_INVERSE_MEL_MAX_MELS, "the header's limit is the kernel's");
  AAMD_CHECK_ARG(dtype == AAMD_SA_F32 || dtype == AAMD_SA_F16 || dtype == AAMD_SA_BF16,
                 "inverse_mel: float32, float16 or bfloat16 elements");
  AAMD_CHECK_ARG(rows >= 0 && frames >= 0 && n_stft >= 1 && n_mels >= 1, "inverse_mel: bad sizes");
  if (n_mels > AAMD_INVERSE_MEL_MAX_MELS)
    return fail(AAMD_EUNSUPPORTED, "audio_amd: inverse_mel: the kernel serves up to 256 mel bins");
  AAMD_CHECK_ARG(stride_row >= 0 && stride_mel >= 1 && stride_frame >= 1, "inverse_mel: strides must be positive");
  AAMD_CHECK_ARG(stride_mel == 1 || stride_frame == 1 || n_mels == 1 || frames <= 1,
                 "inverse_mel: the input needs unit stride along mel or along time");
  if (rows == 0 || frames == 0) return AAMD_OK;
  const int64_t tiles = iml::tiles_per_row(frames);
  AAMD_CHECK_ARG(rows < (1ll << 31) && frames < (1ll << 40) && rows * tiles < (1ll << 31), "inverse_mel: too many rows or frames");
  AAMD_CHECK_ARG(x && pinv && out, "null buffer");
  const int es = dtype == AAMD_SA_F32 ? 4 : 2;
  AAMD_CHECK_ARG((((uintptr_t)x | (uintptr_t)out) & (uintptr_t)(es - 1)) == 0, "inverse_mel: a buffer is not aligned to its element");
  AAMD_CHECK_ARG(((uintptr_t)pinv & 15) == 0, "inverse_mel: the pseudo-inverse's tiles must be 16-byte aligned");
  iml::Args a{};
  a.x = x; a.P = pinv; a.out = out;
  a.rows = rows; a.T = frames; a.sr = rows > 1 ? stride_row : 0; a.sm = stride_mel; a.st = stride_frame;
  a.F = n_stft; a.K = n_mels;
  a.time_major = (stride_mel == 1 || n_mels == 1) ? 0 : 1;
  a.log_input = log_input ? 1 : 0;
  const size_t lds = (size_t)iml::lds_floats(n_mels) * sizeof(float);
  if (lds > 48 * 1024 && lds > dev_props().lds_per_block_optin)
    return fail(AAMD_EUNSUPPORTED, "audio_amd: inverse_mel: this device has less LDS than the tiles were planned for");
  hipStream_t s = (hipStream_t)stream;
  switch (dtype) {
    case AAMD_SA_F32: return launch(iml::inverse_mel_kernel<wa::kF32>, rows * tiles, iml::kThreads, lds, s, a, tiles);
    case AAMD_SA_F16: return launch(iml::inverse_mel_kernel<wa::kF16>, rows * tiles, iml::kThreads, lds, s, a, tiles);
    default: return launch(iml::inverse_mel_kernel<wa::kBF16>, rows * tiles, iml::kThreads, lds, s, a, tiles);
  }
}

}  // extern "C"
