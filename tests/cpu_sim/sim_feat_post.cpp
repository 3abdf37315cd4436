// CPU replay of the feature post-processing kernels (audio_amd/csrc/feat_post.h compiled with g++, no GPU): each driver
// mirrors its __global__ kernel, "all threads run phase X, then __syncthreads()" replaced by a loop over thread ids, with
// the launch geometry of the C ABI (delta_plan / cmn_plan).  TEST INFRASTRUCTURE ONLY.
#include <cstdint>
#include <vector>

#include "../../audio_amd/csrc/feat_post.h"

using namespace aamd;

template <typename T>
static int sim_deltas(const T* x, T* out, int64_t C, int64_t F, int64_t Tn, int64_t sc, int64_t sf, int64_t st,
                      int win_length, int mode, int adjoint) {
  fp::DeltaGeom g;
  if (!fp::delta_plan(g, C, F, Tn, sc, sf, st, (win_length - 1) / 2, mode, adjoint, (int64_t)sizeof(T))) return -2;
  std::vector<T> lds((size_t)g.tf * g.w);
  const int64_t blocks = C * g.n_ftiles * g.n_ttiles;
  for (int64_t b0 = 0; b0 < blocks; ++b0) {
    int64_t b = b0;
    const int64_t tt = b % g.n_ttiles;
    b /= g.n_ttiles;
    const int64_t ft = b % g.n_ftiles;
    const int64_t c = b / g.n_ftiles;
    for (int tid = 0; tid < fp::kDtThreads; ++tid) fp::delta_fill<T>(tid, fp::kDtThreads, g, c, ft * g.tf, tt * fp::kDtT, x, lds.data());
    for (int tid = 0; tid < fp::kDtThreads; ++tid)
      fp::delta_out<T>(tid, fp::kDtThreads, g, c, ft * g.tf, tt * fp::kDtT, x, lds.data(), out);
  }
  return 0;
}

template <typename T>
static int sim_cmn(const T* x, T* out, int64_t C, int64_t Tn, int64_t F, int64_t sc, int64_t st, int64_t sf, int64_t win,
                   int64_t min_win, int center, int norm_vars, int adjoint) {
  fp::CmnGeom g;
  fp::cmn_plan(g, C, Tn, F, sc, st, sf, win, min_win, center, norm_vars, adjoint);
  std::vector<double> ws((size_t)(C * g.n_chunks * F * (norm_vars ? 2 : 1)) + 1);
  const int64_t blocks = C * g.n_chunks * g.n_ftiles;
  for (int pass = 0; pass < 2; ++pass)
    for (int64_t b0 = 0; b0 < blocks; ++b0) {
      int64_t b = b0;
      const int64_t ft = b % g.n_ftiles;
      b /= g.n_ftiles;
      const int64_t k = b % g.n_chunks;
      const int64_t c = b / g.n_chunks;
      for (int tid = 0; tid < g.threads; ++tid) {
        const int64_t f = ft * g.threads + tid;
        if (f >= F) continue;
        if (pass == 0) fp::cmn_chunk_sum<T>(g, x, ws.data(), c, k, f);
        else fp::cmn_walk<T>(g, x, ws.data(), out, c, k, f);
      }
    }
  return 0;
}

extern "C" {

int sim_deltas_f32(const float* x, float* out, int64_t C, int64_t F, int64_t Tn, int64_t sc, int64_t sf, int64_t st,
                   int win_length, int mode, int adjoint) {
  return sim_deltas<float>(x, out, C, F, Tn, sc, sf, st, win_length, mode, adjoint);
}

int sim_deltas_f64(const double* x, double* out, int64_t C, int64_t F, int64_t Tn, int64_t sc, int64_t sf, int64_t st,
                   int win_length, int mode, int adjoint) {
  return sim_deltas<double>(x, out, C, F, Tn, sc, sf, st, win_length, mode, adjoint);
}

int sim_cmn_f32(const float* x, float* out, int64_t C, int64_t Tn, int64_t F, int64_t sc, int64_t st, int64_t sf,
                int64_t win, int64_t min_win, int center, int norm_vars, int adjoint) {
  return sim_cmn<float>(x, out, C, Tn, F, sc, st, sf, win, min_win, center, norm_vars, adjoint);
}

int sim_cmn_f64(const double* x, double* out, int64_t C, int64_t Tn, int64_t F, int64_t sc, int64_t st, int64_t sf,
                int64_t win, int64_t min_win, int center, int norm_vars, int adjoint) {
  return sim_cmn<double>(x, out, C, Tn, F, sc, st, sf, win, min_win, center, norm_vars, adjoint);
}

}  // extern "C"
