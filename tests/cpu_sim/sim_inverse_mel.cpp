// CPU replay of the InverseMelScale kernel (audio_amd/csrc/inverse_mel.h compiled with g++, no GPU): the driver mirrors
// inverse_mel_kernel, "all threads run phase X, then __syncthreads()" replaced by a loop over thread ids, with the launch
// geometry and the LDS carve-up of the C ABI; the MFMA chain is the header's fmaf restatement.  TEST INFRASTRUCTURE ONLY.
#include <cstdint>
#include <vector>

#include "../../audio_amd/csrc/inverse_mel.h"

using namespace aamd;

template <int DT>
static int run(const iml::Args& a) {
  const int KP = iml::k_pad(a.K);
  // canaries around the three LDS regions: a phase that writes outside its region is caught here, not on a GPU
  const int64_t n = iml::lds_floats(a.K);
  const float canary = -12345.5f;
  std::vector<float> store((size_t)n + 12, canary);
  float* smem = store.data();
  while (((uintptr_t)smem & 15) != 0) ++smem;              // the regions are 16-byte aligned, as the kernel's are
  float* yfrag = smem + 4;
  float* pfrag = yfrag + iml::kFrames * KP;
  float* otile = pfrag + iml::kBins * KP;
  const int64_t tiles = iml::tiles_per_row(a.T);
  for (int64_t blk = 0; blk < a.rows * tiles; ++blk) {
    const int64_t row = blk / tiles, t0 = (blk - row * tiles) * iml::kFrames;
    for (int tid = 0; tid < iml::kThreads; ++tid) iml::stage_y<DT>(tid, a, row, t0, yfrag);
    for (int f0 = 0; f0 < a.F; f0 += iml::kBins) {
      for (int tid = 0; tid < iml::kThreads; ++tid) iml::stage_p(tid, a, f0, pfrag);
      for (int tid = 0; tid < iml::kThreads; ++tid) iml::mma_thread(tid, a, f0, yfrag, pfrag, otile);
      for (int tid = 0; tid < iml::kThreads; ++tid) iml::store_tile<DT>(tid, a, row, t0, f0, otile);
    }
    if (yfrag[-1] != canary || yfrag[n] != canary) return -2;
  }
  return 0;
}

extern "C" {

int sim_iml_tiles(int which) { return which == 0 ? iml::kFrames : (which == 1 ? iml::kBins : iml::kMaxMels); }
int64_t sim_iml_lds_bytes(int n_mels) { return iml::lds_floats(n_mels) * (int64_t)sizeof(float); }

// The arguments of aamd_inverse_mel; < 0 on an unknown dtype or a write outside the LDS regions.
int sim_iml(int dtype, const void* x, const float* pinv, void* out, int64_t rows, int64_t frames, int64_t sr, int64_t sm,
            int64_t st, int n_stft, int n_mels, int log_input) {
  iml::Args a{};
  a.x = x; a.P = pinv; a.out = out;
  a.rows = rows; a.T = frames; a.sr = rows > 1 ? sr : 0; a.sm = sm; a.st = st;
  a.F = n_stft; a.K = n_mels;
  a.time_major = (sm == 1 || n_mels == 1) ? 0 : 1;
  a.log_input = log_input ? 1 : 0;
  switch (dtype) {
    case wa::kF32: return run<wa::kF32>(a);
    case wa::kF16: return run<wa::kF16>(a);
    case wa::kBF16: return run<wa::kBF16>(a);
    default: return -1;
  }
}

}  // extern "C"
