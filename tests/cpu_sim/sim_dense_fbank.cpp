// CPU replay of the dense filterbank kernel (audio_amd/csrc/dense_fbank.h compiled with g++, no GPU): the driver mirrors
// dense_fbank_kernel, "all threads run phase X, then __syncthreads()" replaced by a loop over thread ids that keeps every
// thread's registers (its fetched tile, its accumulators) between phases, with the launch geometry and the LDS carve-up of
// the C ABI; the MFMA chain is the header's fmaf restatement.  TEST INFRASTRUCTURE ONLY.
#include <cstdint>
#include <vector>

#include "../../audio_amd/csrc/dense_fbank.h"

using namespace aamd;

template <int DT, int NT>
static int run_nt(const dfb::Args& a) {
  using S = typename dfb::Elem<DT>::S;
  // canaries around the two LDS regions: a phase that writes outside its region is caught here, not on a GPU
  const int64_t n = dfb::lds_floats(a.N);
  const float canary = -12345.5f;
  std::vector<float> store((size_t)n + 12, canary);
  float* smem = store.data();
  while (((uintptr_t)smem & 15) != 0) ++smem;              // the regions are 16-byte aligned, as the kernel's are
  float* xfrag = smem + 4;
  float* wfrag = xfrag + dfb::kFrames * dfb::kTileK;
  std::vector<dfb::Fetched<S, NT>> f(dfb::kThreads);
  std::vector<dfb::Acc> acc(dfb::kThreads);
  const int64_t tiles = dfb::tiles_per_row(a.T);
  for (int64_t blk = 0; blk < a.rows * tiles; ++blk) {
    const int64_t row = blk / tiles, t0 = (blk - row * tiles) * dfb::kFrames;
    for (int tid = 0; tid < dfb::kThreads; ++tid) {
      dfb::clear<NT>(acc[tid]);
      dfb::fetch<DT, NT>(tid, a, row, t0, 0, f[tid]);
    }
    for (int k0 = 0; k0 < a.K; k0 += dfb::kTileK) {
      for (int tid = 0; tid < dfb::kThreads; ++tid) dfb::commit<DT, NT>(tid, a, t0, k0, f[tid], xfrag, wfrag);
      for (int tid = 0; tid < dfb::kThreads; ++tid) {
        if (k0 + dfb::kTileK < a.K) dfb::fetch<DT, NT>(tid, a, row, t0, k0 + dfb::kTileK, f[tid]);
        dfb::mma_lane<NT>(tid >> 6, tid & 63, dfb::tile_steps(a.K, k0), xfrag, wfrag, acc[tid]);
      }
    }
    for (int tid = 0; tid < dfb::kThreads; ++tid) dfb::store_lane<DT, NT>(tid >> 6, tid & 63, a, row, t0, acc[tid]);
    if (xfrag[-1] != canary || xfrag[n] != canary) return -2;
  }
  return 0;
}

template <int DT>
static int run(const dfb::Args& a) {
  switch (dfb::n_tiles(a.N)) {
    case 1: return run_nt<DT, 1>(a);
    case 2: return run_nt<DT, 2>(a);
    case 3: return run_nt<DT, 3>(a);
    case 4: return run_nt<DT, 4>(a);
    case 5: return run_nt<DT, 5>(a);
    case 6: return run_nt<DT, 6>(a);
    case 7: return run_nt<DT, 7>(a);
    default: return run_nt<DT, 8>(a);
  }
}

extern "C" {

int sim_dfb_tiles(int which) {
  return which == 0 ? dfb::kFrames : (which == 1 ? dfb::kTileK : (which == 2 ? dfb::kMaxN : dfb::kMaxK));
}
int64_t sim_dfb_lds_bytes(int n_out) { return dfb::lds_floats(n_out) * (int64_t)sizeof(float); }

// The arguments of aamd_dense_fbank; < 0 on an unknown dtype, a size beyond the limits or a write outside the LDS regions.
int sim_dfb(int dtype, const void* x, const float* w, void* out, int64_t rows, int64_t frames, int64_t sr, int64_t sk,
            int64_t st, int n_freqs, int n_out) {
  if (n_out < 1 || n_out > dfb::kMaxN || n_freqs < 1 || n_freqs > dfb::kMaxK) return -3;
  dfb::Args a{};
  a.x = x; a.W = w; a.out = out;
  a.rows = rows; a.T = frames; a.sr = rows > 1 ? sr : 0; a.sk = sk; a.st = st;
  a.K = n_freqs; a.N = n_out;
  a.time_major = (sk == 1 || n_freqs == 1) ? 0 : 1;
  switch (dtype) {
    case wa::kF32: return run<wa::kF32>(a);
    case wa::kF16: return run<wa::kF16>(a);
    case wa::kBF16: return run<wa::kBF16>(a);
    default: return -1;
  }
}

}  // extern "C"
