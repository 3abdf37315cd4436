// The two table-building kernels of the n_fft = 400 path (once per filterbank / DCT matrix, not per launch), apart from
// melspec400.h so that the sources that include it for the transform kernels do not each emit them.
#pragma once
#include "f16_bits.h"
#include "melspec400.h"

#if defined(__HIPCC__)
namespace aamd {
namespace m400 {

// The DCT matrix as MFMA A fragments, split into binary16 hi / lo planes (once per DCT matrix; aamd_mfcc_frag_build).
__global__ void __launch_bounds__(256) mfcc_frag_build_kernel(const float* __restrict__ dct, int n_mels, int n_mfcc,
                                                              float* __restrict__ frag) {
  uint16_t* fh = reinterpret_cast<uint16_t*>(frag);
  const int n = kMfccMT * kMfccSteps * 64 * 8;                        // (t, s, lane, j)
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int j = i & 7, lane = (i >> 3) & 63, g = i >> 9, s = g % kMfccSteps, t = g / kMfccSteps;
    const float v = mfcc_frag_value(dct, n_mels, n_mfcc, t, s, lane, j);
    const uint16_t hi = rsm::f16_bits(v);
    const uint16_t lo = rsm::f16_bits(v - rsm::f16_value(hi));
    fh[mfcc_frag_piece(t, s, 0, lane) * 8 + j] = hi;
    fh[mfcc_frag_piece(t, s, 1, lane) * 8 + j] = lo;
  }
}

// One workgroup lays out the band table image in global memory (once per filterbank; aamd_mel400_table_build).
__global__ void __launch_bounds__(256) mel_tab_build_kernel(MelBandsDev mb, float* __restrict__ out) {
  MelTab mt{};
  mel_tab_rounds(threadIdx.x, blockDim.x, mb, out, mt);
  __syncthreads();   // the chunk counts written above are read below by other threads of this workgroup
  mel_tab_fill(threadIdx.x, blockDim.x, mb, out, mt);
}

}  // namespace m400
}  // namespace aamd
#endif
