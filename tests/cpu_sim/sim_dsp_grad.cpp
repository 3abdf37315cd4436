// CPU replay of the synthesis ops' backward kernels (audio_amd/csrc/dsp_synth_grad.h compiled with g++, no GPU): each driver
// mirrors its kernel, "all threads run phase X, then __syncthreads()" replaced by a loop over thread ids, with the launch
// geometry, the LDS layout and the workspaces of the C ABI.  TEST INFRASTRUCTURE ONLY.
#include <cstdint>
#include <vector>

#include "../../audio_amd/csrc/dsp_synth_grad.h"

using namespace aamd;

template <int DT>
static void run_fw_grad(const dsp::FwGradArgs& a) {     // fw_gx_kernel; fw_gh_kernel, then fw_gh_fold_kernel
  using C = typename wa::Elem<DT>::C;
  if (a.gx) {
    std::vector<C> gs(dsp::fw_lds_values(a.L));
    for (int64_t blk = 0; blk < a.rows * a.tiles; ++blk) {
      const int64_t row = blk / a.tiles, tile = blk - row * a.tiles;
      for (int tid = 0; tid < dsp::kThreads; ++tid) dsp::fwg_stage<DT>(tid, a, row, tile, gs.data());
      for (int tid = 0; tid < dsp::kThreads; ++tid) dsp::fwg_outputs<DT>(tid, a, row, tile, gs.data());
    }
  }
  if (a.gh) {
    std::vector<C> xs(dsp::kGhPiece), gs(dsp::kGhPiece + dsp::kGhLags - 1);
    for (int64_t blk = 0; blk < a.rows * a.units * a.lag_tiles; ++blk) {
      const int64_t lag_tile = blk % a.lag_tiles, ru = blk / a.lag_tiles;
      const int64_t row = ru / a.units, unit = ru - row * a.units;
      for (int tid = 0; tid < dsp::kThreads; ++tid) dsp::fwg_gh_stage<DT>(tid, a, row, unit, lag_tile, xs.data(), gs.data());
      for (int tid = 0; tid < dsp::kThreads; ++tid) dsp::fwg_gh_lags<DT>(tid, a, row, unit, lag_tile, xs.data(), gs.data());
    }
    if (!a.direct) {
      const int64_t count = (a.batched ? a.rows : 1) * a.F * a.L;
      for (int64_t i = 0; i < (count + dsp::kThreads - 1) / dsp::kThreads * dsp::kThreads; ++i) dsp::fwg_gh_fold<DT>(a, i);
    }
  }
}

template <int DT>
static void run_osc_grad(const dsp::OscGradArgs& a) {  // osc_sums_kernel, osc_grad_totals_kernel, osc_grad_apply_kernel
  const dsp::OscArgs& o = a.o;
  const dsp::OscGeom g = dsp::osc_geom(o.N);
  std::vector<double> sub(dsp::kThreads), start(dsp::kThreads), qsub(dsp::kThreads), tail(dsp::kThreads), base(dsp::kThreads),
      above(dsp::kThreads);
  for (int64_t blk = 0; o.chunks > 1 && blk < o.rows * (o.chunks - 1); ++blk) {
    const int64_t row = blk / (o.chunks - 1), chunk = blk - row * (o.chunks - 1);
    for (int tid = 0; tid < dsp::kThreads; ++tid) sub[tid] = dsp::osc_slice_sum<DT>(tid, o, g, row, chunk);
    for (int tid = 0; tid < dsp::kThreads; ++tid) dsp::osc_chunk_sum(tid, o, g, row, chunk, sub.data());
  }
  for (int64_t blk = 0; a.gf && o.chunks > 1 && blk < o.rows * (o.chunks - 1); ++blk) {
    const int64_t row = blk / (o.chunks - 1), chunk = 1 + blk - row * (o.chunks - 1);
    for (int tid = 0; tid < dsp::kThreads; ++tid) {
      sub[tid] = dsp::osc_slice_sum<DT>(tid, o, g, row, chunk);
      dsp::osc_start(tid, o, row, chunk, start.data());
    }
    for (int tid = 0; tid < dsp::kThreads; ++tid)
      qsub[tid] = dsp::osc_grad_slice<DT>(tid, a, g, row, chunk, dsp::osc_base(tid, o, g, start.data(), sub.data()), false, 0.0);
    for (int tid = 0; tid < dsp::kThreads; ++tid) dsp::osc_grad_chunk_total(tid, a, g, row, chunk, qsub.data());
  }
  for (int64_t blk = 0; blk < o.rows * o.chunks; ++blk) {
    const int64_t row = blk / o.chunks, chunk = blk - row * o.chunks;
    for (int tid = 0; tid < dsp::kThreads; ++tid) {
      sub[tid] = dsp::osc_slice_sum<DT>(tid, o, g, row, chunk);
      dsp::osc_start(tid, o, row, chunk, start.data());
    }
    for (int tid = 0; tid < dsp::kThreads; ++tid) {
      base[tid] = dsp::osc_base(tid, o, g, start.data(), sub.data());
      above[tid] = 0.0;
      if (a.gf) {
        qsub[tid] = dsp::osc_grad_slice<DT>(tid, a, g, row, chunk, base[tid], false, 0.0);
        dsp::osc_grad_tail(tid, a, row, chunk, tail.data());
      }
    }
    for (int tid = 0; tid < dsp::kThreads; ++tid) {
      if (a.gf) above[tid] = dsp::osc_grad_above(tid, a, g, tail.data(), qsub.data());
      dsp::osc_grad_slice<DT>(tid, a, g, row, chunk, base[tid], true, above[tid]);
    }
  }
}

#define SIM_DISPATCH(dtype, F, a)                 \
  switch (dtype) {                                \
    case wa::kF32: F<wa::kF32>(a); break;         \
    case wa::kF64: F<wa::kF64>(a); break;         \
    case wa::kF16: F<wa::kF16>(a); break;         \
    case wa::kBF16: F<wa::kBF16>(a); break;       \
    default: return -1;                           \
  }

extern "C" {

int sim_dsp_grad_tiles(int which) {
  const int v[2] = {dsp::kGhPiece, dsp::kGhLags};
  return which >= 0 && which < 2 ? v[which] : 0;
}

// the buffers of the C ABI on the host (a null gradient is not computed); -1 on an argument it refuses, -2 beyond a limit
int sim_filter_waveform_grad(int dtype, const void* x, const void* h, const void* g, void* gx, void* gh, int64_t rows, int64_t T,
                             int64_t sx, int64_t F, int L, int batched) {
  if (rows < 0 || T < 0 || F < 1 || L < 1 || T % F) return -1;
  if (L > dsp::kMaxTaps) return -2;
  if (rows == 0 || T == 0) return 0;
  dsp::FwGradArgs a{};
  a.x = x; a.h = h; a.g = g; a.gx = gx; a.gh = gh; a.rows = rows; a.T = T; a.sx = sx; a.F = F; a.C = T / F;
  a.tiles = (T + dsp::kFwTile - 1) / dsp::kFwTile; a.L = L; a.batched = batched;
  dsp::fw_grad_geom(a);
  std::vector<double> ws(a.direct ? 1 : (size_t)(rows * F * a.P * L), -7.0);
  a.ws = ws.data();
  SIM_DISPATCH(dtype, run_fw_grad, a)
  return 0;
}

int sim_oscillator_bank_grad(int dtype, const void* freq, const void* amp, const void* g, void* gf, void* ga, int64_t rows,
                             int64_t T, int64_t N, int64_t sf, int64_t sa, double sample_rate, int reduction) {
  if (rows < 0 || T < 0 || N < 0 || reduction < 0 || reduction > 2) return -1;
  if (N > dsp::kMaxOsc) return -2;
  if (rows == 0 || T == 0 || N == 0) return 0;
  dsp::OscGradArgs a{};
  dsp::OscArgs& o = a.o;
  o.chunks = (T + dsp::kOscChunk - 1) / dsp::kOscChunk;
  std::vector<double> sums((size_t)(rows * o.chunks * N), -7.0), tots((size_t)(rows * o.chunks * N), -7.0);
  o.freq = freq; o.amp = amp; o.sums = sums.data();
  o.rows = rows; o.T = T; o.sf = sf; o.sa = sa; o.sample_rate = sample_rate; o.N = (int32_t)N; o.reduction = reduction;
  a.g = g; a.ga = ga; a.gf = gf; a.tots = tots.data();
  SIM_DISPATCH(dtype, run_osc_grad, a)
  return 0;
}

}  // extern "C"
