// CPU replay of the NCCF pitch kernels (audio_amd/csrc/pitch.h compiled with g++, no GPU): each driver mirrors its
// __global__ kernel, "all threads run phase X, then __syncthreads()" replaced by a loop over thread ids, with the launch
// geometry of the C ABI (pitch_plan).  TEST INFRASTRUCTURE ONLY.
#include <cstdint>
#include <vector>

#include "../../audio_amd/csrc/pitch.h"

using namespace aamd;

// mode 0: out = float32 (rows, n_out) and lag_out = int32 (rows, F); mode 1: out = T (rows, F, lags)
template <typename T>
static int sim_pitch(const T* x, void* out, int32_t* lag_out, int64_t rows, int64_t L, int64_t rs, int sr, int fs, int lags,
                     int lag_min, int win, int mode, int64_t* geom) {
  pt::PitchGeom g;
  if (!pt::pitch_plan(g, rows, L, rs, fs, lags, lag_min, mode == 1 ? 3 : win, (float)sr, mode, (int64_t)sizeof(T))) return -2;
  if (geom) {   // T, J, n_chunks, LDS bytes
    geom[0] = g.T; geom[1] = g.J; geom[2] = g.n_chunks; geom[3] = pt::pitch_lds_bytes(g, (int64_t)sizeof(T));
  }
  std::vector<T> lds((size_t)g.lds_elems);
  std::vector<pt::PickState> st((size_t)g.T);
  const int nth = pt::kThreads;
  for (int64_t blk = 0; blk < rows * g.n_ftiles; ++blk) {
    const int64_t row = blk / g.n_ftiles, k0 = (blk - row * g.n_ftiles) * g.T;
    const T* xr = x + row * rs;
    for (int tid = 0; tid < nth; ++tid) pt::pitch_stage_s1<T>(tid, nth, g, xr, k0, lds.data());
    for (int t = 0; t < g.T; ++t) st[t] = pt::pitch_pick_init();
    for (int c = 0; c < g.n_chunks; ++c) {
      const int j0 = 1 + c * g.J;
      for (int tid = 0; tid < nth; ++tid) pt::pitch_stage_seg2<T>(tid, nth, g, xr, k0, j0, lds.data());
      for (int tid = 0; tid < nth; ++tid) pt::pitch_block_sums<T>(tid, nth, g, lds.data());
      for (int tid = 0; tid < nth; ++tid) pt::pitch_energies<T>(tid, nth, g, c == 0, lds.data());
      for (int tid = 0; tid < nth; ++tid) pt::pitch_nccf<T>(tid, nth, g, lds.data());
      if (mode == 1) {
        for (int tid = 0; tid < nth; ++tid) pt::pitch_write_nccf<T>(tid, nth, g, row, k0, j0, lds.data(), static_cast<T*>(out));
        continue;
      }
      const int J = (g.lags - (j0 - 1)) < g.J ? (g.lags - (j0 - 1)) : g.J;
      for (int t = 0; t < g.T; ++t) {
        // the wave's 64 lanes, then the butterfly: the merge order differs from the device, the comparator is a total order
        pt::PickState s = pt::pitch_pick_init();
        for (int lane = 0; lane < 64; ++lane) {
          pt::PickState l = pt::pitch_pick_init();
          for (int j = lane; j < J; j += 64) pt::pitch_pick_fold<T>(l, lds[g.o_nccf + t * (g.G * pt::kR) + j], j0 + j, g);
          pt::pitch_pick_merge<T>(s, l);
        }
        pt::pitch_pick_merge<T>(st[t], s);
        if (c == g.n_chunks - 1 && k0 + t < g.F) lag_out[row * g.F + k0 + t] = pt::pitch_combine<T>(st[t]);
      }
    }
  }
  if (mode == 1 || g.n_out < 1) return 0;
  const int64_t per_row = (g.n_out + pt::kMedT - 1) / pt::kMedT;
  std::vector<int> tile(pt::kMedT + g.win - 1);
  const bool tiled = pt::pitch_median_tiled(g);
  for (int64_t blk = 0; blk < rows * per_row; ++blk) {
    const int64_t row = blk / per_row, t0 = (blk - row * per_row) * pt::kMedT;
    if (tiled)
      for (int tid = 0; tid < nth; ++tid) pt::pitch_median_fill(tid, nth, g, lag_out, row, t0, tile.data());
    for (int tid = 0; tid < nth; ++tid)
      pt::pitch_median_out(tid, g, lag_out, tiled ? tile.data() : nullptr, row, t0, static_cast<float*>(out));
  }
  return 0;
}

extern "C" {

int sim_pitch_f32(const float* x, void* out, int32_t* lag_out, int64_t rows, int64_t L, int64_t rs, int sr, int fs, int lags,
                  int lag_min, int win, int mode, int64_t* geom) {
  return sim_pitch<float>(x, out, lag_out, rows, L, rs, sr, fs, lags, lag_min, win, mode, geom);
}

int sim_pitch_f64(const double* x, void* out, int32_t* lag_out, int64_t rows, int64_t L, int64_t rs, int sr, int fs, int lags,
                  int lag_min, int win, int mode, int64_t* geom) {
  return sim_pitch<double>(x, out, lag_out, rows, L, rs, sr, fs, lags, lag_min, win, mode, geom);
}

}  // extern "C"
