// First-order adjoints of the two hot synthesis ops of csrc/dsp_synth.h (oscillator_bank, filter_waveform).  The definition is
// tests/dsp_grad_oracle.py.  dsp_synth.h is included as it is: the phase of the oscillator's gradients is formed by the
// forward's own functions (osc_w, osc_slice_sum, osc_chunk_sum, osc_start, osc_base, reduce_2pi), so it has the forward's bits.
//
// filter_waveform, y[n] = sum_j x[m] h[m / C][j], m = n + d - j, with the cotangent g (rows, T) dense:
//   fw_gx     gx[m] = sum_j h[m / C][j] g[m - d + j].  One launch with the forward's tile: a workgroup owns kFwTile outputs of
//             one row and stages g[tile_start - d .. tile_end - d + L - 1] in LDS; a lane owns kFwPer consecutive outputs,
//             one accumulator each in ascending j (fused multiply-adds in C).  The values of g are a register window that
//             slides by one LDS read per tap; the tap is one load for the lane where its outputs share a chunk (they do
//             except across a chunk boundary, and at C < kFwPer).  A tap whose g lies outside the row is skipped by a select.
//   fw_gh     gh[set][c][j] = sum_m x[r][m] g[r][m - d + j] over the m of chunk c (and over the rows r where the filters are
//             shared).  A workgroup owns (row, unit of time, tile of kGhLags lags): a unit is a piece of at most kGhPiece
//             samples of one chunk where C >= kGhPiece, and floor(kGhPiece / C) whole chunks otherwise, so F = 1 with a long
//             row is cut into T / kGhPiece pieces and C = 1 into runs of kGhPiece chunks.  x and g of the unit sit in LDS;
//             lane j walks m in ascending order with one float64 fused multiply-add per product (a float32 product is exact
//             in float64) and closes its sum where the chunk or the piece ends.  With one piece per chunk and one row per
//             set the sum is the result and is stored rounded once; otherwise it goes to the float64 workspace
//             (rows, F, pieces, L) and fw_gh_fold adds the pieces in ascending time, then the rows in ascending order, and
//             rounds once.  No atomics: two calls give the same bits.
//
// oscillator_bank, y[t] = sum_n a'[t, n] sin phi[t, n], with g (rows, T) -- (rows, T, N) for "none"; divided by N in C for
// "mean" -- and q = g a' cos phi:
//   ga[t, n] = g sin phi where the oscillator is live, (g sin phi) * 0 where it is dead (0, or NaN under a poisoned phase);
//   gf[t, n] = (2 pi / sample_rate) sum_{s >= t} q[s, n].
// The lanes are the forward's (slice, n).  osc_sums_kernel gives the chunk sums of w.  osc_grad_totals (chunks 1 ..) walks
// every slice once and stores the chunk's total of q -- float64, each slice in time order, the slices in ascending order.
// osc_grad_apply walks its slice twice: once for the slice's total of q, then, with `above` = (the totals of the later
// chunks, added from the last one down) + (the later slices of this chunk, from the last one down) + the slice's own total,
// it stores gf[t] = scale (above - the running sum before t), rounded once to C, and ga as it goes.  q is formed as
// fma(double(g) double(a'), double(cos phi), sum): for float32 the product g a' is exact.
//
// The phase functions are AAMD_HD: tests/cpu_sim/sim_dsp_grad.cpp replays them with g++.
#pragma once
#include "dsp_synth.h"

namespace aamd {
namespace dsp {

constexpr int kGhPiece = 1024;      // samples of one unit of fw_gh
constexpr int kGhLags = kThreads;   // lags of one workgroup of fw_gh: one per lane

AAMD_HD float d_cos(float v) { return cosf(v); }
AAMD_HD double d_cos(double v) { return cos(v); }

// ---- filter_waveform -------------------------------------------------------------------------------------------------------
struct FwGradArgs {
  const void *x, *h, *g;      // x (rows, T) through sx; h (F, L) or (rows, F, L) dense; g (rows, T) dense
  void *gx, *gh;              // (rows, T) dense; the shape of h, dense
  double* ws;                 // (rows, F, P, L) where the sums are folded
  int64_t rows, T, sx, F, C, tiles;
  int64_t P, G, units, lag_tiles;   // pieces per chunk, chunks per unit, units per row, tiles of lags
  int32_t L, batched, direct;
};

AAMD_HD void fw_grad_geom(FwGradArgs& a) {
  a.P = (a.C + kGhPiece - 1) / kGhPiece;
  a.G = a.C >= kGhPiece ? 1 : kGhPiece / a.C;
  a.units = a.G == 1 ? a.F * a.P : (a.F + a.G - 1) / a.G;
  a.lag_tiles = (a.L + kGhLags - 1) / kGhLags;
  a.direct = (a.P == 1 && (a.batched || a.rows == 1)) ? 1 : 0;
}

template <int DT>
AAMD_HD void fwg_stage(int tid, const FwGradArgs& a, int64_t row, int64_t tile, typename wa::Elem<DT>::C* gs) {
  using E = wa::Elem<DT>;
  const typename E::S* g = static_cast<const typename E::S*>(a.g) + row * a.T;
  const int64_t span0 = tile * kFwTile - (a.L - 1) / 2;
  const int count = kFwTile + a.L - 1;
  for (int i = tid; i < count; i += kThreads) {
    const int64_t n = span0 + i;
    gs[i] = (n >= 0 && n < a.T) ? E::load(g[n]) : typename E::C(0);
  }
}

template <int DT>
AAMD_HD void fwg_outputs(int tid, const FwGradArgs& a, int64_t row, int64_t tile, const typename wa::Elem<DT>::C* gs) {
  using E = wa::Elem<DT>;
  using C = typename E::C;
  using S = typename E::S;
  const int d = (a.L - 1) / 2;
  const int64_t m0 = tile * kFwTile + (int64_t)tid * kFwPer;
  if (m0 >= a.T) return;
  const S* h = static_cast<const S*>(a.h) + (a.batched ? row * a.F * a.L : 0);
  const S* hr[kFwPer];
  for (int r = 0; r < kFwPer; ++r) {
    const int64_t m = m0 + r < a.T ? m0 + r : a.T - 1;
    hr[r] = h + (m / a.C) * a.L;
  }
  const bool same = hr[0] == hr[kFwPer - 1];
  const int base = tid * kFwPer;                      // gs[base + r + j] is g[m0 + r - d + j]
  const int64_t n0 = m0 - d;
  C acc[kFwPer], gw[kFwPer];
  for (int r = 0; r < kFwPer; ++r) acc[r] = C(0), gw[r] = gs[base + r];
  for (int j = 0; j < a.L; ++j) {
    C hv[kFwPer];
    if (same) {
      const C v = E::load(hr[0][j]);
#if defined(__HIPCC__)
#pragma unroll
#endif
      for (int r = 0; r < kFwPer; ++r) hv[r] = v;
    } else {
#if defined(__HIPCC__)
#pragma unroll
#endif
      for (int r = 0; r < kFwPer; ++r) hv[r] = E::load(hr[r][j]);
    }
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int r = 0; r < kFwPer; ++r) {
      const C nv = d_fma(hv[r], gw[r], acc[r]);
      acc[r] = (uint64_t)(n0 + r + j) < (uint64_t)a.T ? nv : acc[r];
    }
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int r = 0; r < kFwPer - 1; ++r) gw[r] = gw[r + 1];
    if (j + 1 < a.L) gw[kFwPer - 1] = gs[base + kFwPer + j];
  }
  S* o = static_cast<S*>(a.gx) + row * a.T;
  for (int r = 0; r < kFwPer; ++r)
    if (m0 + r < a.T) o[m0 + r] = E::store(acc[r]);
}

// the samples [ma, mb) of unit `unit` of a row and its piece of the chunk
AAMD_HD void fwg_unit(const FwGradArgs& a, int64_t unit, int64_t& ma, int64_t& mb, int64_t& piece) {
  if (a.G == 1) {
    const int64_t c = unit / a.P;
    piece = unit - c * a.P;
    ma = c * a.C + piece * kGhPiece;
    mb = ma + kGhPiece < (c + 1) * a.C ? ma + kGhPiece : (c + 1) * a.C;
  } else {
    piece = 0;
    ma = unit * a.G * a.C;
    mb = ma + a.G * a.C < a.T ? ma + a.G * a.C : a.T;
  }
}

// xs: kGhPiece values, gs: kGhPiece + kGhLags - 1 values; gs[i] is g[ma - d + j0 + i]
template <int DT>
AAMD_HD void fwg_gh_stage(int tid, const FwGradArgs& a, int64_t row, int64_t unit, int64_t lag_tile, typename wa::Elem<DT>::C* xs,
                          typename wa::Elem<DT>::C* gs) {
  using E = wa::Elem<DT>;
  using S = typename E::S;
  int64_t ma, mb, piece;
  fwg_unit(a, unit, ma, mb, piece);
  const S* x = static_cast<const S*>(a.x) + row * a.sx;
  const S* g = static_cast<const S*>(a.g) + row * a.T;
  const int len = (int)(mb - ma);
  for (int i = tid; i < len; i += kThreads) xs[i] = E::load(x[ma + i]);
  const int64_t span0 = ma - (a.L - 1) / 2 + lag_tile * kGhLags;
  for (int i = tid; i < len + kGhLags - 1; i += kThreads) {
    const int64_t n = span0 + i;
    gs[i] = (n >= 0 && n < a.T) ? E::load(g[n]) : typename E::C(0);
  }
}

template <int DT>
AAMD_HD void fwg_gh_lags(int tid, const FwGradArgs& a, int64_t row, int64_t unit, int64_t lag_tile,
                         const typename wa::Elem<DT>::C* xs, const typename wa::Elem<DT>::C* gs) {
  using E = wa::Elem<DT>;
  using C = typename E::C;
  using S = typename E::S;
  const int64_t j = lag_tile * kGhLags + tid;
  if (j >= a.L) return;
  int64_t ma, mb, piece;
  fwg_unit(a, unit, ma, mb, piece);
  const int len = (int)(mb - ma);
  const int64_t n0 = ma - (a.L - 1) / 2 + j;          // the index into g at m = ma
  int64_t c = ma / a.C, cnt = ma - c * a.C;
  double acc = 0.0;
  for (int i = 0; i < len; ++i) {
    const double nv = fma((double)xs[i], (double)gs[i + tid], acc);
    acc = (uint64_t)(n0 + i) < (uint64_t)a.T ? nv : acc;
    if (++cnt == a.C || i == len - 1) {
      if (a.direct) static_cast<S*>(a.gh)[((a.batched ? row * a.F : 0) + c) * a.L + j] = E::store((C)acc);
      else a.ws[(((row * a.F + c) * a.P) + piece) * a.L + j] = acc;
      acc = 0.0;
      cnt = 0;
      ++c;
    }
  }
}

// element i of gh: the pieces in ascending time, then the rows in ascending order
template <int DT>
AAMD_HD void fwg_gh_fold(const FwGradArgs& a, int64_t i) {
  using E = wa::Elem<DT>;
  using C = typename E::C;
  const int64_t sets = a.batched ? a.rows : 1;
  if (i >= sets * a.F * a.L) return;
  const int64_t j = i % a.L, c = (i / a.L) % a.F, set = i / (a.L * a.F);
  const int64_t r0 = a.batched ? set : 0, r1 = a.batched ? set + 1 : a.rows;
  double total = 0.0;
  for (int64_t r = r0; r < r1; ++r) {
    double s = 0.0;
    for (int64_t p = 0; p < a.P; ++p) s += a.ws[(((r * a.F + c) * a.P) + p) * a.L + j];
    total += s;
  }
  static_cast<typename E::S*>(a.gh)[i] = E::store((C)total);
}

// ---- oscillator_bank -------------------------------------------------------------------------------------------------------
struct OscGradArgs {
  OscArgs o;                  // freq, amp, sums, rows, T, sf, sa, chunks, sample_rate, N, reduction: the forward's (out unused)
  const void* g;              // (rows, T), or (rows, T, N) for "none", dense
  void *ga, *gf;              // (rows, T, N) dense; null: not wanted
  double* tots;               // (rows, chunks, N): the chunk totals of q (chunk 0 is not used)
};

// lane `tid`'s slice in time order.  write = false: returns the slice's total of q.  write = true: stores ga and
// gf[t] = scale (above - the sum of q before t), and returns the same total.
template <int DT>
AAMD_HD double osc_grad_slice(int tid, const OscGradArgs& a, const OscGeom& g, int64_t row, int64_t chunk, double run, bool write,
                              double above) {
  using E = wa::Elem<DT>;
  using C = typename E::C;
  using S = typename E::S;
  const OscArgs& o = a.o;
  const int ts = tid / o.N, n = tid - ts * o.N;
  if (ts >= g.TS) return 0.0;
  const S* f = static_cast<const S*>(o.freq) + row * o.sf;
  const S* am = static_cast<const S*>(o.amp) + row * o.sa;
  const S* gp = static_cast<const S*>(a.g);
  const C two_pi = (C)(2.0 * kPi), sr = (C)o.sample_rate, nyq = (C)(o.sample_rate / 2.0);
  const double scale = 2.0 * kPi / o.sample_rate;
  const int64_t t0 = chunk * kOscChunk + (int64_t)ts * g.S;
  double pre = 0.0;
  for (int s = 0; s < g.S; ++s) {
    const int64_t t = t0 + s;
    if (!(ts * g.S + s < kOscChunk && t < o.T)) break;
    const C fv = E::load(f[t * o.N + n]);
    run += (double)osc_w<C>(fv, two_pi, sr);
    const C ph = (C)reduce_2pi(run);
    const bool dead = d_abs(fv) >= nyq;
    C gv = E::load(o.reduction == kNone ? gp[(row * o.T + t) * o.N + n] : gp[row * o.T + t]);
    if (o.reduction == kMean) gv = gv / (C)o.N;
    if (write && a.ga) {
      const C v = gv * d_sin(ph);
      static_cast<S*>(a.ga)[(row * o.T + t) * o.N + n] = E::store(dead ? v * C(0) : v);
    }
    if (a.gf) {
      const C ap = dead ? C(0) : E::load(am[t * o.N + n]);
      if (write) static_cast<S*>(a.gf)[(row * o.T + t) * o.N + n] = E::store((C)(scale * (above - pre)));
      pre = fma((double)gv * (double)ap, (double)d_cos(ph), pre);
    }
  }
  return pre;
}

// osc_grad_totals: lane n < N adds the slices in ascending order
AAMD_HD void osc_grad_chunk_total(int tid, const OscGradArgs& a, const OscGeom& g, int64_t row, int64_t chunk, const double* qsub) {
  if (tid >= a.o.N) return;
  double sum = 0.0;
  for (int ts = 0; ts < g.TS; ++ts) sum += qsub[ts * a.o.N + tid];
  a.tots[(row * a.o.chunks + chunk) * a.o.N + tid] = sum;
}

// osc_grad_apply: lane n < N adds the totals of the later chunks, from the last one down
AAMD_HD void osc_grad_tail(int tid, const OscGradArgs& a, int64_t row, int64_t chunk, double* tail) {
  if (tid >= a.o.N) return;
  double sum = 0.0;
  for (int64_t c = a.o.chunks - 1; c > chunk; --c) sum += a.tots[(row * a.o.chunks + c) * a.o.N + tid];
  tail[tid] = sum;
}

// the tail, the later slices of this chunk from the last one down, and the lane's own slice
AAMD_HD double osc_grad_above(int tid, const OscGradArgs& a, const OscGeom& g, const double* tail, const double* qsub) {
  const int ts = tid / a.o.N, n = tid - ts * a.o.N;
  if (ts >= g.TS) return 0.0;
  double above = tail[n];
  for (int q = g.TS - 1; q >= ts; --q) above += qsub[q * a.o.N + n];
  return above;
}

#if defined(__HIPCC__)
template <int DT>
__global__ __launch_bounds__(kThreads) void fw_gx_kernel(FwGradArgs a) {
  using C = typename wa::Elem<DT>::C;
  extern __shared__ __align__(16) unsigned char fwg_smem[];
  C* gs = reinterpret_cast<C*>(fwg_smem);
  const int64_t row = (int64_t)blockIdx.x / a.tiles, tile = (int64_t)blockIdx.x - row * a.tiles;
  fwg_stage<DT>(threadIdx.x, a, row, tile, gs);
  __syncthreads();
  fwg_outputs<DT>(threadIdx.x, a, row, tile, gs);
}

template <int DT>
__global__ __launch_bounds__(kThreads) void fw_gh_kernel(FwGradArgs a) {
  using C = typename wa::Elem<DT>::C;
  __shared__ C xs[kGhPiece], gs[kGhPiece + kGhLags - 1];
  const int64_t lag_tile = (int64_t)blockIdx.x % a.lag_tiles, ru = (int64_t)blockIdx.x / a.lag_tiles;
  const int64_t row = ru / a.units, unit = ru - row * a.units;
  fwg_gh_stage<DT>(threadIdx.x, a, row, unit, lag_tile, xs, gs);
  __syncthreads();
  fwg_gh_lags<DT>(threadIdx.x, a, row, unit, lag_tile, xs, gs);
}

template <int DT>
__global__ __launch_bounds__(kThreads) void fw_gh_fold_kernel(FwGradArgs a) {
  fwg_gh_fold<DT>(a, (int64_t)blockIdx.x * kThreads + threadIdx.x);
}

template <int DT>
__global__ __launch_bounds__(kThreads) void osc_grad_totals_kernel(OscGradArgs a) {
  __shared__ double sub[kThreads], start[kThreads], qsub[kThreads];
  const OscGeom g = osc_geom(a.o.N);
  const int tid = threadIdx.x;
  const int64_t row = (int64_t)blockIdx.x / (a.o.chunks - 1), chunk = 1 + (int64_t)blockIdx.x - row * (a.o.chunks - 1);
  sub[tid] = osc_slice_sum<DT>(tid, a.o, g, row, chunk);
  osc_start(tid, a.o, row, chunk, start);
  __syncthreads();
  qsub[tid] = osc_grad_slice<DT>(tid, a, g, row, chunk, osc_base(tid, a.o, g, start, sub), false, 0.0);
  __syncthreads();
  osc_grad_chunk_total(tid, a, g, row, chunk, qsub);
}

template <int DT>
__global__ __launch_bounds__(kThreads) void osc_grad_apply_kernel(OscGradArgs a) {
  __shared__ double sub[kThreads], start[kThreads], qsub[kThreads], tail[kThreads];
  const OscGeom g = osc_geom(a.o.N);
  const int tid = threadIdx.x;
  const int64_t row = (int64_t)blockIdx.x / a.o.chunks, chunk = (int64_t)blockIdx.x - row * a.o.chunks;
  sub[tid] = osc_slice_sum<DT>(tid, a.o, g, row, chunk);
  osc_start(tid, a.o, row, chunk, start);
  __syncthreads();
  const double base = osc_base(tid, a.o, g, start, sub);
  double above = 0.0;
  if (a.gf) {
    qsub[tid] = osc_grad_slice<DT>(tid, a, g, row, chunk, base, false, 0.0);
    osc_grad_tail(tid, a, row, chunk, tail);
    __syncthreads();
    above = osc_grad_above(tid, a, g, tail, qsub);
  }
  osc_grad_slice<DT>(tid, a, g, row, chunk, base, true, above);
}
#endif

}  // namespace dsp
}  // namespace aamd
