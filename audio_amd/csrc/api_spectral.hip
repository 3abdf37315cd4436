// Spectral features of the C ABI (csrc/spectral_feat.h): exported constants and the centroid reduction.
#include "api_common.h"
#include "spectral_feat.h"

using namespace aamd;

namespace {

template <int DT>
int centroid_launch(const sf::CentArgs& a, bool lines, hipStream_t s) {
  const int64_t items = a.rows * a.frames;
  if (lines) {
    const int64_t per_block = sf::kThreads / a.lanes;
    return launch(sf::centroid_kernel<DT, true>, (items + per_block - 1) / per_block, sf::kThreads, 0, s, a);
  }
  return launch(sf::centroid_kernel<DT, false>, (items + sf::kThreads - 1) / sf::kThreads, sf::kThreads, 0, s, a);
}

}  // namespace

extern "C" {

int32_t aamd_spectral_tiles(int32_t which) {
  return which == 0 ? sf::kThreads : (which == 1 ? sf::kVec : (which == 2 ? sf::kMaxLanes : 0));
}

int32_t aamd_spectral_lanes(int64_t n_freq) { return n_freq < 1 ? 0 : sf::lanes_for(n_freq); }

int aamd_spectral_centroid(int32_t out_dtype, const float* mag, const float* freqs, void* out, int64_t rows, int64_t frames,
                           int64_t n_freq, int64_t stride_row, int64_t stride_frame, int64_t stride_freq, void* stream) {
  DeviceScope dev_scope_(mag);
  AAMD_CHECK_ARG(out_dtype == AAMD_SA_F32 || out_dtype == AAMD_SA_F16 || out_dtype == AAMD_SA_BF16,
                 "spectral_centroid: the result is float32, float16 or bfloat16");
  AAMD_CHECK_ARG(rows >= 0 && frames >= 0 && n_freq >= 1, "spectral_centroid: bad sizes");
  AAMD_CHECK_ARG(stride_row >= 0 && stride_frame >= 0 && stride_freq >= 0, "spectral_centroid: negative stride");
  AAMD_CHECK_ARG(rows < (1ll << 31) && frames < (1ll << 31) && n_freq < (1ll << 31), "spectral_centroid: too many rows, frames or bins");
  if (rows == 0 || frames == 0) return AAMD_OK;
  AAMD_CHECK_ARG(mag && freqs && out, "null buffer");
  AAMD_CHECK_ARG(((uintptr_t)mag & 3) == 0 && ((uintptr_t)freqs & 15) == 0, "spectral_centroid: a float buffer is misaligned");
  AAMD_CHECK_ARG(((uintptr_t)out & (uintptr_t)(out_dtype == AAMD_SA_F32 ? 3 : 1)) == 0, "spectral_centroid: the result is misaligned");
  sf::CentArgs a{};
  a.m = mag; a.freqs = freqs; a.out = out; a.rows = rows; a.frames = frames; a.n_freq = n_freq;
  a.sr = stride_row; a.st = stride_frame; a.sk = stride_freq;
  const bool lines = stride_freq == 1 || n_freq == 1;
  a.lanes = lines ? sf::lanes_for(n_freq) : 1;
  AAMD_CHECK_ARG(rows * frames / (sf::kThreads / a.lanes) < (1ll << 31) - 1, "spectral_centroid: too many workgroups");
  hipStream_t s = (hipStream_t)stream;
  switch (out_dtype) {
    case AAMD_SA_F32: return centroid_launch<wa::kF32>(a, lines, s);
    case AAMD_SA_F16: return centroid_launch<wa::kF16>(a, lines, s);
    default: return centroid_launch<wa::kBF16>(a, lines, s);
  }
}

}  // extern "C"
