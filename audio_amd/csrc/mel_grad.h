// Element-wise kernels beside the forward STFT: the RNN-T log / normalisation of a mel buffer and the backward of the
// (mel) spectrogram's power stage.  Reference: the autograd of transforms/_transforms.py:101-123, :612-622.
#pragma once
#include "hd.h"
#include "stft_generic.h"

#if defined(__HIPCC__)
namespace aamd {

// RNN-T feature post-processing on a frame-major mel buffer (the unfused form of EPI400_MEL_NORM)
__global__ void __launch_bounds__(256)
lognorm_kernel(float* __restrict__ x, int64_t n, int n_mels, float gain, const float* __restrict__ mean,
               const float* __restrict__ invstd) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int m = (int)(i % n_mels);
    const float y = x[i] * gain;
    const float t = y > 2.718281828459045f ? __log2f(y) * 0.69314718055994531f : y;   // see epi_plog (melspec400.h):
    const float l = t <= 2.718281828459045f ? t / 2.718281828459045f : t;             // the reference's second mask
    x[i] = (l - mean[m]) * invstd[m];
  }
}

// Backward of |X|^p: G = dP * p * |X|^(p-2) * X per bin (0 where X = 0 and p < 2) -- the spectrum-domain cotangent the
// STFT adjoint (aamd_istft_f32, adjoint = 1) consumes; X and G interleaved complex, dP real, all frame-major
__global__ void __launch_bounds__(256)
spec_grad_kernel(const float2* X, const float* __restrict__ dP, float2* G, int64_t n, float power) {   // G may alias X (in-place backward)
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const float2 x = X[i];
    float f = power * dP[i];
    if (power != 2.0f) {
      const float m2 = x.x * x.x + x.y * x.y;
      f = m2 > 0.0f ? f * powf(m2, 0.5f * power - 1.0f) : 0.0f;
    }
    G[i] = make_float2(f * x.x, f * x.y);
  }
}

// Backward of MelSpectrogram's two element-wise stages in one pass: dP[k] = sum_m fb[k][m] dY[m] (band table of fb^T)
// and G = dP p |X|^(p-2) X, written over X (`XG`)
__global__ void __launch_bounds__(256)
mel_grad_kernel(float2* __restrict__ XG, const float* __restrict__ dY, MelBandsDev bt /* bands of fb^T: one per bin */,
                int64_t n_vec, int n_mels, float power) {
  const int n_freq = bt.n_mels;                          // "mels" of the transposed table are the bins
  const int64_t total = n_vec * n_freq;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += stride) {
    const int64_t v = o / n_freq;
    const int k = (int)(o - v * n_freq);
    const int lo = bt.lo[k], w = bt.width[k];
    const float* wt = bt.weights + (int64_t)k * bt.max_width;
    const float* row = dY + v * n_mels + lo;
    float dp = 0.0f;
    for (int i = 0; i < w; ++i) dp += wt[i] * row[i];
    const float2 x = XG[o];
    float f = power * dp;
    if (power != 2.0f) {
      const float m2 = x.x * x.x + x.y * x.y;
      f = m2 > 0.0f ? f * powf(m2, 0.5f * power - 1.0f) : 0.0f;
    }
    XG[o] = make_float2(f * x.x, f * x.y);
  }
}

}  // namespace aamd
#endif
