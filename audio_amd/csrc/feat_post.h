// Feature post-processing after the front-ends: delta coefficients (F.compute_deltas / T.ComputeDeltas) and Kaldi's
// sliding-window cepstral mean / variance normalisation (F.sliding_window_cmn / T.SlidingWindowCmn).
//
// Both are memory-bound streaming stencils along time over the (..., freq, time) tensors MelSpectrogram / fbank_batch
// produce.  The per-thread phase functions below are AAMD_HD so that tests/cpu_sim/sim_feat_post.cpp replays them with
// g++ (one loop over thread ids per phase); the __global__ kernels at the bottom only decode the workgroup index.
//
// Deltas (reference semantics: pad the time axis by n = (win_length - 1) / 2 frames with `mode`, correlate with
// [-n .. n], divide by denom = n (n + 1) (2n + 1) / 3):
//   one workgroup per tile of kDtT frames x tf features of one channel.  Phase 1 fills an LDS tile with the tile's frames
//   plus an n-frame halo on each side; the pad mode lives entirely in the halo's index map (pad_source_index: clamp /
//   mirror / wrap / zero).  The input is read IN PLACE through its element strides: lanes walk time when the rows are
//   time-contiguous, features when the storage is frame-major (feature stride 1: every MelSpectrogram / Spectrogram
//   output, fbank_batch(...).transpose(-1, -2)); the LDS tile is the transpose.  Phase 2 runs the stencil out of LDS
//   with lanes along time and writes the contiguous (C, F, T) result.
//   adjoint = 1 evaluates the transpose of that linear map (autograd): inside, the negated stencil over the zero-extended
//   gradient; every padded position i then folds its value back onto its source frame pad_source_index(i) (the edge frame
//   for replicate, the mirrored frame for reflect, the wrapped frame for circular, nothing for constant).
//
// Sliding-window CMN (window [s(t), e(t)) of cmn_window(); the reference keeps a float32 running sum, here every window
// sum is accumulated in float64):
//   pass 1: float64 sums (and sums of squares with norm_vars) of every chunk of kCmnL frames, per (channel, feature),
//           into a caller-allocated workspace;
//   pass 2: one lane per (channel, chunk, feature): the window sum at the chunk's first frame from the chunk sums plus at
//           most two partial chunks (each at most kCmnL / 2 frames: the shorter side of the chunk boundary), then a walk
//           over the chunk that adds the frame entering and drops the frame leaving the window (s and e move by at most
//           one frame per step).  The walk's loads are issued kCmnB steps ahead of the float64 chain.
//   Each input element is read from memory a bounded number of times (its own chunk in pass 1, its own frame, once as
//   the frame entering and once as the frame leaving a window, partial chunks at chunk starts) whatever cmn_window is.
//   adjoint = 1 (norm_vars = false only): gx[u] = g[u] - sum_{t : s(t) <= u < e(t)} g[t] / n(t); the set of such t is the
//   interval [a(u), b(u)) (s and e are monotone), walked by the same passes over the values g[t] / n(t).
#pragma once
#include "hd.h"

namespace aamd {
namespace fp {

constexpr int kDtT = 64;               // frames per delta tile
constexpr int kDtThreads = 256;
constexpr int kDtLdsBytes = 32 * 1024; // LDS budget of a delta tile
constexpr int kDtFill = 8;             // tile elements per thread whose loads are issued together
constexpr int kCmnL = 64;              // frames per CMN chunk
constexpr int kCmnB = 8;               // walk steps whose loads are issued together

struct DeltaGeom {
  int64_t C, F, T;       // channels, features, frames
  int64_t sc, sf, st;    // input element strides
  int64_t n_ftiles, n_ttiles;
  int32_t n;             // half window
  int32_t mode;          // AAMD_PAD_*
  int32_t adjoint;
  int32_t tf;            // features per tile
  int32_t w;             // LDS row stride (odd, >= kDtT + 2n)
  int32_t feat_fast;     // 1: fill the tile with lanes along features
  double denom;
};

// Launch geometry (shared by the C ABI and the CPU replay).  false: the window's LDS tile does not fit the budget.
inline bool delta_plan(DeltaGeom& g, int64_t C, int64_t F, int64_t T, int64_t sc, int64_t sf, int64_t st, int n, int mode,
                       int adjoint, int64_t elem_bytes) {
  g.C = C; g.F = F; g.T = T;
  g.sc = sc; g.sf = sf; g.st = st;
  g.n = n; g.mode = mode; g.adjoint = adjoint ? 1 : 0;
  g.denom = (double)n * (n + 1) * (2 * n + 1) / 3.0;
  g.w = (kDtT + 2 * n) | 1;                                       // odd row stride: frame-major fills are conflict-free
  const int64_t max_tf = kDtLdsBytes / ((int64_t)g.w * elem_bytes);
  if (max_tf < 1) return false;
  g.feat_fast = (F > 1 && sf == 1 && st != 1) ? 1 : 0;
  const int64_t cap = g.feat_fast ? (max_tf < 128 ? max_tf : 128) : (max_tf < 16 ? max_tf : 16);
  const int64_t nft = (F + cap - 1) / cap;
  g.tf = (int32_t)((F + nft - 1) / nft);
  g.n_ftiles = (F + g.tf - 1) / g.tf;
  g.n_ttiles = (T + kDtT - 1) / kDtT;
  return true;
}

// padded frame i (in [-n, T + n)) -> source frame or -1 (zero).  The adjoint reads its gradient zero-extended.
AAMD_HD int64_t delta_src(int64_t i, const DeltaGeom& g) {
  if (i >= 0 && i < g.T) return i;
  return g.adjoint ? -1 : pad_source_index(i, g.T, g.mode);
}

// Phase 1: the tile [t0 - n, t0 + kDtT + n) x [f0, f0 + tf) of channel c into lds[f * w + p].
template <typename T>
AAMD_HD void delta_fill(int tid, int nthreads, const DeltaGeom& g, int64_t c, int64_t f0, int64_t t0, const T* x, T* lds) {
  const int wt = kDtT + 2 * g.n;
  const int total = g.tf * wt;
  const T* xc = x + c * g.sc;
  // kDtFill elements per thread and round: their loads are issued back to back, then stored to LDS
  for (int base = tid; base < total; base += kDtFill * nthreads) {
    T v[kDtFill];
    int at[kDtFill];
    for (int k = 0; k < kDtFill; ++k) {
      const int idx = base + k * nthreads;
      int f, p;
      if (g.feat_fast) { p = idx / g.tf; f = idx - p * g.tf; }
      else { f = idx / wt; p = idx - f * wt; }
      const int64_t src = delta_src(t0 - g.n + p, g);
      const bool ok = idx < total && f0 + f < g.F && src >= 0;
      v[k] = ok ? xc[(f0 + f) * g.sf + src * g.st] : T(0);
      at[k] = idx < total ? f * g.w + p : -1;
    }
    for (int k = 0; k < kDtFill; ++k)
      if (at[k] >= 0) lds[at[k]] = v[k];
  }
}

// adjoint only: the value of padded position i, -sum_j j g0[i + j] (g0 = the gradient zero-extended), read from memory
template <typename T>
AAMD_HD T delta_pad_value(const DeltaGeom& g, const T* row, int64_t i) {
  T acc = T(0);
  for (int j = 1; j <= g.n; ++j) {
    const int64_t a = i + j, b = i - j;
    const T va = (a >= 0 && a < g.T) ? row[a * g.st] : T(0);
    const T vb = (b >= 0 && b < g.T) ? row[b * g.st] : T(0);
    acc += T(j) * (va - vb);
  }
  return -acc;
}

// Phase 2: the stencil out of LDS, lanes along time; out is contiguous (C, F, T).
template <typename T>
AAMD_HD void delta_out(int tid, int nthreads, const DeltaGeom& g, int64_t c, int64_t f0, int64_t t0, const T* x,
                       const T* lds, T* out) {
  const int total = g.tf * kDtT;
  for (int idx = tid; idx < total; idx += nthreads) {
    const int f = idx / kDtT, tt = idx - f * kDtT;
    const int64_t t = t0 + tt;
    if (f0 + f >= g.F || t >= g.T) continue;
    const T* r = lds + f * g.w + tt + g.n;
    T acc = T(0);
    for (int j = 1; j <= g.n; ++j) acc += T(j) * (r[j] - r[-j]);
    if (g.adjoint) {
      acc = -acc;
      // padded positions whose source is frame t (only frames within n + 1 of either end have any)
      if (g.mode != 1 && (t <= g.n || t >= g.T - 1 - g.n)) {
        const T* row = x + c * g.sc + (f0 + f) * g.sf;
        for (int64_t q = 0; q < 2 * (int64_t)g.n; ++q) {
          const int64_t i = q < g.n ? q - g.n : g.T + (q - g.n);
          if (pad_source_index(i, g.T, g.mode) == t) acc += delta_pad_value(g, row, i);
        }
      }
    }
    out[(c * g.F + f0 + f) * g.T + t] = acc / T(g.denom);
  }
}

// ---------------------------------------------------------------------------------------------------------------------

struct CmnGeom {
  int64_t C, T, F;       // channels, frames, features
  int64_t sc, st, sf;    // input element strides
  int64_t win, min_win;
  int64_t n_chunks, n_ftiles;
  int32_t center, norm_vars, adjoint;
  int32_t threads;       // lanes per workgroup (features of one tile)
};

inline void cmn_plan(CmnGeom& g, int64_t C, int64_t T, int64_t F, int64_t sc, int64_t st, int64_t sf, int64_t win,
                     int64_t min_win, int center, int norm_vars, int adjoint) {
  g.C = C; g.T = T; g.F = F;
  g.sc = sc; g.st = st; g.sf = sf;
  g.win = win; g.min_win = min_win;
  g.center = center ? 1 : 0; g.norm_vars = norm_vars ? 1 : 0; g.adjoint = adjoint ? 1 : 0;
  g.n_chunks = (T + kCmnL - 1) / kCmnL;
  g.threads = (int32_t)(F >= 256 ? 256 : (F + 63) / 64 * 64);
  g.n_ftiles = (F + g.threads - 1) / g.threads;
}

// the reference's window of frame t (its per-frame loop, verbatim)
AAMD_HD void cmn_window(int64_t t, const CmnGeom& g, int64_t& s, int64_t& e) {
  if (g.center) {
    s = t - g.win / 2;
    e = s + g.win;
  } else {
    s = t - g.win;
    e = t + 1;
  }
  if (s < 0) {
    e -= s;
    s = 0;
  }
  if (!g.center && e > t) e = (t + 1 > g.min_win) ? t + 1 : g.min_win;
  if (e > g.T) {
    s -= e - g.T;
    e = g.T;
    if (s < 0) s = 0;
  }
}

AAMD_HD int64_t cmn_count(int64_t t, const CmnGeom& g) {
  int64_t s, e;
  cmn_window(t, g, s, e);
  return e - s;
}

// adjoint window of frame u: [a(u), b(u)) = {t : s(t) <= u < e(t)}.  a = first t with e(t) > u, b = first t with s(t) > u.
AAMD_HD void cmn_adjoint_window(int64_t u, const CmnGeom& g, int64_t& a, int64_t& b) {
  int64_t lo = 0, hi = g.T;                // first t in [lo, hi) with e(t) > u (hi if none)
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    int64_t s, e;
    cmn_window(mid, g, s, e);
    if (e > u) hi = mid; else lo = mid + 1;
  }
  a = lo;
  lo = 0;
  hi = g.T;
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    int64_t s, e;
    cmn_window(mid, g, s, e);
    if (s > u) hi = mid; else lo = mid + 1;
  }
  b = lo;
}

// the summed value of frame t: x itself, or (adjoint) g[t] / n(t)
template <typename T>
AAMD_HD double cmn_value(const CmnGeom& g, const T* xc, int64_t t, int64_t f) {
  const double v = (double)xc[t * g.st + f * g.sf];
  return g.adjoint ? v / (double)cmn_count(t, g) : v;
}

// Pass 1: float64 sum (and sum of squares) of chunk k for feature f of channel c.  ws = [C][n_chunks][F] sums, then the
// same of squares with norm_vars.
template <typename T>
AAMD_HD void cmn_chunk_sum(const CmnGeom& g, const T* x, double* ws, int64_t c, int64_t k, int64_t f) {
  const T* xc = x + c * g.sc;
  const int64_t t0 = k * kCmnL;
  const int64_t t1 = t0 + kCmnL < g.T ? t0 + kCmnL : g.T;
  double s = 0.0, q = 0.0;
  if (!g.adjoint && t1 - t0 == kCmnL) {
#if defined(__HIPCC__)
#pragma unroll 16
#endif
    for (int j = 0; j < kCmnL; ++j) {
      const double v = (double)xc[(t0 + j) * g.st + f * g.sf];
      s += v;
      q += v * v;
    }
  } else {
    for (int64_t t = t0; t < t1; ++t) {
      const double v = cmn_value(g, xc, t, f);
      s += v;
      q += v * v;
    }
  }
  const int64_t o = (c * g.n_chunks + k) * g.F + f;
  ws[o] = s;
  if (g.norm_vars) ws[g.C * g.n_chunks * g.F + o] = q;
}

struct CmnAcc {
  double s, q;
};

template <typename T>
AAMD_HD void cmn_direct(const CmnGeom& g, const T* xc, int64_t f, int64_t a, int64_t b, double sign, CmnAcc& acc) {
  for (int64_t t0 = a; t0 < b; t0 += kCmnB) {          // kCmnB loads in flight, then the float64 sums
    double v[kCmnB];
    for (int j = 0; j < kCmnB; ++j) v[j] = t0 + j < b ? cmn_value(g, xc, t0 + j, f) : 0.0;
    for (int j = 0; j < kCmnB; ++j) {
      acc.s += sign * v[j];
      acc.q += sign * v[j] * v[j];
    }
  }
}

// sum over frames [lo, hi): the whole chunks inside from the workspace, the rest frame by frame (per chunk boundary the
// shorter side: a partial chunk, or a whole chunk's sum minus its complement)
template <typename T>
AAMD_HD CmnAcc cmn_window_sum(const CmnGeom& g, const T* xc, const double* ws, int64_t c, int64_t f, int64_t lo, int64_t hi) {
  CmnAcc acc{0.0, 0.0};
  if (hi - lo <= 2 * kCmnL) {
    cmn_direct(g, xc, f, lo, hi, 1.0, acc);
    return acc;
  }
  const double* cs = ws + c * g.n_chunks * g.F + f;
  const double* cq = cs + g.C * g.n_chunks * g.F;
  const int64_t kl = (lo + kCmnL - 1) / kCmnL, kh = hi / kCmnL;     // whole chunks [kl, kh); kl < kh here
  for (int64_t k = kl; k < kh; ++k) {
    acc.s += cs[k * g.F];
    if (g.norm_vars) acc.q += cq[k * g.F];
  }
  const int64_t r = kl * kCmnL - lo;                                  // frames [lo, kl L)
  if (r <= kCmnL / 2) {
    cmn_direct(g, xc, f, lo, kl * kCmnL, 1.0, acc);
  } else {                                                            // chunk kl - 1 minus [(kl - 1) L, lo)
    acc.s += cs[(kl - 1) * g.F];
    if (g.norm_vars) acc.q += cq[(kl - 1) * g.F];
    cmn_direct(g, xc, f, (kl - 1) * kCmnL, lo, -1.0, acc);
  }
  const int64_t q = hi - kh * kCmnL;                                  // frames [kh L, hi)
  if (q <= kCmnL / 2 || kh >= g.n_chunks) {
    cmn_direct(g, xc, f, kh * kCmnL, hi, 1.0, acc);
  } else {                                                            // chunk kh minus [hi, end of chunk kh)
    const int64_t end = (kh + 1) * kCmnL < g.T ? (kh + 1) * kCmnL : g.T;
    acc.s += cs[kh * g.F];
    if (g.norm_vars) acc.q += cq[kh * g.F];
    cmn_direct(g, xc, f, hi, end, -1.0, acc);
  }
  if (!g.norm_vars) acc.q = 0.0;
  return acc;
}

template <typename T>
AAMD_HD T cmn_result(const CmnGeom& g, double xt, const CmnAcc& acc, int64_t n) {
  const double nd = (double)n;
  double y = xt - acc.s / nd;
  if (g.norm_vars) {
    if (n == 1) {
      y = 0.0;
    } else {
      const double var = acc.q / nd - (acc.s * acc.s) / (nd * nd);
      y *= 1.0 / sqrt(var);
    }
  }
  return (T)y;
}

// Pass 2: the outputs of chunk k for feature f of channel c; out is contiguous (C, T, F).
template <typename T>
AAMD_HD void cmn_walk(const CmnGeom& g, const T* x, const double* ws, T* out, int64_t c, int64_t k, int64_t f) {
  const T* xc = x + c * g.sc;
  T* oc = out + c * g.T * g.F + f;
  const int64_t t0 = k * kCmnL;
  const int64_t t1 = t0 + kCmnL < g.T ? t0 + kCmnL : g.T;
  int64_t lo, hi;
  if (g.adjoint) {
    cmn_adjoint_window(t0, g, lo, hi);
    CmnAcc acc = cmn_window_sum(g, xc, ws, c, f, lo, hi);
    for (int64_t t = t0; t < t1; ++t) {
      if (t > t0) {            // the adjoint window can jump by more than one frame (e.g. past the min_cmn_window plateau)
        int64_t s, e;
        while (lo < g.T && (cmn_window(lo, g, s, e), e <= t)) acc.s -= cmn_value(g, xc, lo++, f);
        while (hi < g.T && (cmn_window(hi, g, s, e), s <= t)) acc.s += cmn_value(g, xc, hi++, f);
      }
      oc[t * g.F] = (T)((double)xc[t * g.st + f * g.sf] - acc.s);
    }
    return;
  }
  cmn_window(t0, g, lo, hi);
  CmnAcc acc = cmn_window_sum(g, xc, ws, c, f, lo, hi);
  for (int64_t tb = t0; tb < t1; tb += kCmnB) {
    // loads of kCmnB steps first (s and e move by at most one frame per step), then the float64 chain
    double xt[kCmnB], xa[kCmnB], xd[kCmnB];
    int64_t nn[kCmnB];
    int64_t l = lo, h = hi;
    for (int j = 0; j < kCmnB; ++j) {
      const int64_t t = tb + j < t1 ? tb + j : t1 - 1;
      int64_t s, e;
      cmn_window(t, g, s, e);
      const bool drop = s > l, add = e > h;
      xt[j] = (double)xc[t * g.st + f * g.sf];
      xd[j] = drop ? (double)xc[l * g.st + f * g.sf] : 0.0;
      xa[j] = add ? (double)xc[h * g.st + f * g.sf] : 0.0;
      nn[j] = e - s;
      l = s;
      h = e;
    }
    for (int j = 0; j < kCmnB; ++j) {
      if (tb + j >= t1) break;
      acc.s += xa[j] - xd[j];
      if (g.norm_vars) acc.q += xa[j] * xa[j] - xd[j] * xd[j];
      oc[(tb + j) * g.F] = cmn_result<T>(g, xt[j], acc, nn[j]);
    }
    lo = l;
    hi = h;
  }
}

#if defined(__HIPCC__)
template <typename T>
__global__ void __launch_bounds__(kDtThreads) deltas_kernel(const T* __restrict__ x, T* __restrict__ out, DeltaGeom g) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_dt[];
  T* lds = reinterpret_cast<T*>(smem_dt);
  int64_t b = blockIdx.x;
  const int64_t tt = b % g.n_ttiles;
  b /= g.n_ttiles;
  const int64_t ft = b % g.n_ftiles;
  const int64_t c = b / g.n_ftiles;
  delta_fill<T>(threadIdx.x, kDtThreads, g, c, ft * g.tf, tt * kDtT, x, lds);
  __syncthreads();
  delta_out<T>(threadIdx.x, kDtThreads, g, c, ft * g.tf, tt * kDtT, x, lds, out);
}

template <typename T>
__global__ void __launch_bounds__(256) cmn_chunk_kernel(const T* __restrict__ x, double* __restrict__ ws, CmnGeom g) {
  int64_t b = blockIdx.x;
  const int64_t ft = b % g.n_ftiles;
  b /= g.n_ftiles;
  const int64_t k = b % g.n_chunks;
  const int64_t c = b / g.n_chunks;
  const int64_t f = ft * g.threads + threadIdx.x;
  if (f < g.F) cmn_chunk_sum<T>(g, x, ws, c, k, f);
}

template <typename T>
__global__ void __launch_bounds__(256) cmn_walk_kernel(const T* __restrict__ x, const double* __restrict__ ws,
                                                       T* __restrict__ out, CmnGeom g) {
  int64_t b = blockIdx.x;
  const int64_t ft = b % g.n_ftiles;
  b /= g.n_ftiles;
  const int64_t k = b % g.n_chunks;
  const int64_t c = b / g.n_chunks;
  const int64_t f = ft * g.threads + threadIdx.x;
  if (f < g.F) cmn_walk<T>(g, x, ws, out, c, k, f);
}
#endif

}  // namespace fp
}  // namespace aamd
