// NCCF pitch tracker, F.detect_pitch_frequency (torchaudio functional.py: _compute_nccf, _find_max_per_frame,
// _combine_max, _median_smoothing).
//
// Reference semantics for one row x of length L (zero-padded on the right to lags + F fs):
//   nccf[k][lag - 1] = sum_i x[k fs + i] x[k fs + lag + i] / (EPS + |s1|)^2 / (EPS + |s2|)^2,  lag = 1 .. lags, i < fs
//   best = first argmax over lag in [lag_min + 1, lags], half = first argmax over [lag_min + 1, lags / 2]
//   lag(k) = half.v > 0.99 best.v ? half : best;  out[t] = sample_rate / lower_median(lag(k) windowed, left-replicated)
//
// pitch_nccf_pick_kernel: one workgroup per (row, tile of T frames); lags are processed in chunks of J (one chunk
// unless fs and lags are large).  Per chunk:
//   stage   s1 rows (frame t: x[(k0 + t) fs + i], i < fs, zero to fsR) once per tile, and seg2 = x[k0 fs + j0 + m]
//           (zeros past the row end: the reference's right pad);
//   energy  the denominator (EPS + sqrt(e))^2 of every s2 window start in seg2, from block sums of kEb samples plus a
//           direct head and tail (all terms non-negative: no cancellation);
//   nccf    register blocking: a lane owns kR consecutive lags of one frame and slides a kR-sample register window over
//           seg2, so one LDS read of s1 (4 samples) feeds 4 kR FMAs and one read of seg2 feeds kR;
//   then    mode 0: one wave per frame runs both first-index max reductions and the 0.99 combine and writes one int32
//           lag per frame; mode 1: the chunk's NCCF rows are written out (rows, F, lags).  Both modes run the same
//           arithmetic into the same LDS rows, so the fused pick sees exactly the NCCF that mode 1 returns.
// pitch_median_kernel: the lower median of win_length bounded lags per output frame (counting select out of an LDS
//   tile), then float32 reciprocal(EPS + lag) * sample_rate.
//
// The per-thread phase functions are AAMD_HD so that tests/cpu_sim/sim_pitch.cpp replays them with g++.
#pragma once
#include "hd.h"

namespace aamd {
namespace pt {

constexpr int kR = 12;              // lags per lane (register window)
constexpr int kEb = 17;             // energy block (odd: lanes striding by it read distinct LDS banks)
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxT = 64;           // frames per tile
constexpr int kMedT = 256;          // median outputs per workgroup
constexpr int64_t kMedLds = 32 * 1024;  // median tile budget (larger windows read the lags from memory)
constexpr int64_t kLdsSmall = 64 * 1024;
constexpr int64_t kLdsMax = 160 * 1024;
constexpr int kMaxFrameSize = 8192;
constexpr int kMaxLags = 16384;

struct PitchGeom {
  int64_t rows, L, rs;   // rows, samples per row, row stride (elements)
  int64_t F;             // frames
  int64_t n_ftiles;
  int64_t n_out;         // output frames (F + p - win + 1)
  int32_t fs, fsR;       // frame size, padded to a multiple of kR (and of 4)
  int32_t lags, lag_min; // lag_min = ceil(sr / freq_high)
  int32_t half_end;      // lags // 2: the half slice holds lags lag_min + 1 .. half_end
  int32_t T;             // frames per tile
  int32_t J, G;          // lags per chunk (G kR), lane groups per chunk
  int32_t n_chunks;
  int32_t len2, nd2, nb2;  // seg2 samples, energy windows, energy blocks
  int32_t win, p;        // median window, its left pad
  int32_t mode;          // 0: pick, 1: write the NCCF
  float sample_rate;
  // LDS offsets, in elements
  int32_t o_s1, o_seg2, o_d2, o_nccf, o_d1, o_bs;
  int64_t lds_elems;     // elements of T; the per-frame pick state follows (pitch_lds_bytes)
};

inline int64_t round_up(int64_t a, int64_t b) { return (a + b - 1) / b * b; }

inline void pitch_layout(PitchGeom& g) {
  g.G = (g.J + kR - 1) / kR;
  g.len2 = (g.T - 1) * g.fs + g.G * kR + g.fsR;
  g.nd2 = (g.T - 1) * g.fs + g.G * kR;
  g.nb2 = (g.len2 + kEb - 1) / kEb;
  int64_t o = 0;
  g.o_s1 = 0;
  o += (int64_t)g.T * g.fsR;
  g.o_seg2 = (int32_t)o;
  o += round_up(g.len2, 4);
  g.o_d2 = (int32_t)o;
  o += round_up(g.nd2, 4);
  g.o_nccf = (int32_t)o;
  o += (int64_t)g.T * g.G * kR;
  g.o_d1 = (int32_t)o;
  o += round_up(g.T, 4);
  g.o_bs = (int32_t)o;
  o += round_up(g.nb2, 4);
  g.lds_elems = o;
}

// Pick state per frame (best value/lag, half value/lag), after the element arrays, in bytes.
inline int64_t pitch_lds_bytes(const PitchGeom& g, int64_t elem) { return g.lds_elems * elem + (int64_t)g.T * 4 * 8; }

// Launch geometry (shared by the C ABI and the CPU replay).  false: fs or lags beyond the supported range, or no tile fits.
inline bool pitch_plan(PitchGeom& g, int64_t rows, int64_t L, int64_t rs, int fs, int lags, int lag_min, int win, float sr,
                       int mode, int64_t elem) {
  g.rows = rows; g.L = L; g.rs = rs;
  g.fs = fs; g.lags = lags; g.lag_min = lag_min; g.half_end = lags / 2;
  g.win = win; g.p = (win - 1) / 2; g.mode = mode; g.sample_rate = sr;
  if (fs < 1 || fs > kMaxFrameSize || lags < 1 || lags > kMaxLags) return false;
  g.fsR = (int32_t)round_up(fs, kR % 4 == 0 ? kR : kR * 4);
  g.F = (L + fs - 1) / fs;
  g.n_out = g.F + g.p - win + 1;
  // all lags in one chunk: as many frames as fill the workgroup's lanes once, within the small LDS budget
  g.J = lags;
  const int G = (lags + kR - 1) / kR;
  int T = kThreads / G;
  if (T < 1) T = 1;
  if (T > kMaxT) T = kMaxT;
  for (; T >= 1; --T) {
    g.T = T;
    pitch_layout(g);
    if (pitch_lds_bytes(g, elem) <= kLdsSmall) break;
  }
  if (T < 1) {
    // one frame per tile and lags in chunks: the largest chunk (a multiple of 64 kR lags, or of kR) within the LDS
    g.T = 1;
    for (int64_t budget : {kLdsSmall, kLdsMax}) {
      for (int J = (int)round_up(lags, kR); J >= kR; J -= (J > 64 * kR ? 64 * kR : kR)) {
        g.J = J;
        pitch_layout(g);
        if (pitch_lds_bytes(g, elem) <= budget) break;
      }
      if (pitch_lds_bytes(g, elem) <= budget) break;
    }
    if (pitch_lds_bytes(g, elem) > kLdsMax) return false;
    if (g.J > lags) g.J = lags;
    pitch_layout(g);
  }
  g.n_chunks = (lags + g.J - 1) / g.J;
  g.n_ftiles = (g.F + g.T - 1) / g.T;
  return true;
}

// ---- phase functions ----------------------------------------------------------------------------------------------------

// s1 rows of the tile: frame t at s1[t fsR + i] = x[(k0 + t) fs + i] for i < fs, zero up to fsR.
template <typename T>
AAMD_HD void pitch_stage_s1(int tid, int nthreads, const PitchGeom& g, const T* xr, int64_t k0, T* lds) {
  T* s1 = lds + g.o_s1;
  const int total = g.T * g.fsR;
  for (int idx = tid; idx < total; idx += nthreads) {
    const int t = idx / g.fsR, i = idx - t * g.fsR;
    const int64_t pos = (k0 + t) * g.fs + i;
    s1[idx] = (i < g.fs && pos < g.L) ? xr[pos] : T(0);
  }
}

// seg2 of chunk c: seg2[m] = x[k0 fs + j0 + m] (zero past the row end), j0 = 1 + c J.
template <typename T>
AAMD_HD void pitch_stage_seg2(int tid, int nthreads, const PitchGeom& g, const T* xr, int64_t k0, int j0, T* lds) {
  T* seg2 = lds + g.o_seg2;
  const int64_t base = k0 * g.fs + j0;
  for (int m = tid; m < g.len2; m += nthreads) {
    const int64_t pos = base + m;
    seg2[m] = pos < g.L ? xr[pos] : T(0);
  }
}

// Block sums of squares of seg2 (block b = samples [b kEb, b kEb + kEb) within len2).
template <typename T>
AAMD_HD void pitch_block_sums(int tid, int nthreads, const PitchGeom& g, T* lds) {
  const T* seg2 = lds + g.o_seg2;
  T* bs = lds + g.o_bs;
  for (int b = tid; b < g.nb2; b += nthreads) {
    T s = T(0);
    const int e = (b + 1) * kEb < g.len2 ? (b + 1) * kEb : g.len2;
    for (int i = b * kEb; i < e; ++i) s = fma(seg2[i], seg2[i], s);
    bs[b] = s;
  }
}

template <typename T>
AAMD_HD T pitch_denom(T e) {
  const T eps = T(1e-9);
  const T n = eps + sqrt(e);
  return n * n;
}

// Denominators of the s2 windows d2[rel] (window seg2[rel, rel + fs)), and of the s1 rows d1[t] (first chunk only).
// Window rel = q kEb + r is item r nq + q: a wave's lanes share r, hence the head and tail lengths.
template <typename T>
AAMD_HD void pitch_energies(int tid, int nthreads, const PitchGeom& g, bool first, T* lds) {
  const T* seg2 = lds + g.o_seg2;
  const T* bs = lds + g.o_bs;
  T* d2 = lds + g.o_d2;
  const int nq = (g.nd2 + kEb - 1) / kEb;
  const int n_items = nq * kEb + (first ? g.T : 0);
  for (int idx = tid; idx < n_items; idx += nthreads) {
    if (idx >= nq * kEb) {
      const int t = idx - nq * kEb;
      const T* s1 = lds + g.o_s1 + t * g.fsR;
      T s = T(0);
      for (int i = 0; i < g.fs; ++i) s = fma(s1[i], s1[i], s);
      lds[g.o_d1 + t] = pitch_denom(s);
      continue;
    }
    const int r = idx / nq, q = idx - r * nq;
    const int rel = q * kEb + r;
    if (rel >= g.nd2) continue;
    const int e = rel + g.fs;
    const int b0 = (rel + kEb - 1) / kEb, b1 = e / kEb;
    T s = T(0);
    if (b0 >= b1) {
      for (int i = rel; i < e; ++i) s = fma(seg2[i], seg2[i], s);
    } else {
      for (int i = rel; i < b0 * kEb; ++i) s = fma(seg2[i], seg2[i], s);
      for (int b = b0; b < b1; ++b) s += bs[b];
      for (int i = b1 * kEb; i < e; ++i) s = fma(seg2[i], seg2[i], s);
    }
    d2[rel] = pitch_denom(s);
  }
}

// NCCF of the chunk: item (t, gi) -> nccf[t][gi kR + r] for the lags j0 + gi kR + r, r < kR.
template <typename T>
AAMD_HD void pitch_nccf(int tid, int nthreads, const PitchGeom& g, T* lds) {
  const int n_items = g.T * g.G;
  for (int idx = tid; idx < n_items; idx += nthreads) {
    const int t = idx / g.G, gi = idx - t * g.G;
    const T* a = lds + g.o_s1 + t * g.fsR;
    const T* w = lds + g.o_seg2 + t * g.fs + gi * kR;
    T acc[kR], win[kR];
#pragma unroll
    for (int r = 0; r < kR; ++r) { acc[r] = T(0); win[r] = w[r]; }
    // kR steps per iteration: slot (s + r) % kR holds w[i0 + s + r] at step s, so the window never moves in registers
    for (int i0 = 0; i0 < g.fsR; i0 += kR) {
#pragma unroll
      for (int s4 = 0; s4 < kR; s4 += 4) {
        T av[4];
#if defined(__HIPCC__)
        if constexpr (sizeof(T) == 4) {
          const float4 v = *reinterpret_cast<const float4*>(a + i0 + s4);
          av[0] = v.x; av[1] = v.y; av[2] = v.z; av[3] = v.w;
        } else
#endif
        {
#pragma unroll
          for (int u = 0; u < 4; ++u) av[u] = a[i0 + s4 + u];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int s = s4 + u;
#pragma unroll
          for (int r = 0; r < kR; ++r) acc[r] = fma(av[u], win[(s + r) % kR], acc[r]);
          win[s % kR] = w[i0 + s + kR];
        }
      }
    }
    const T d1 = lds[g.o_d1 + t];
    const T* d2 = lds + g.o_d2 + t * g.fs + gi * kR;
    T* out = lds + g.o_nccf + t * (g.G * kR) + gi * kR;
#pragma unroll
    for (int r = 0; r < kR; ++r) out[r] = acc[r] / d1 / d2[r];
  }
}

// (v1, i1) before (v2, i2) in torch.max's order: NaN first, then larger, ties to the smaller lag.
template <typename T>
AAMD_HD bool pitch_better(T v1, int i1, T v2, int i2) {
  const bool n1 = v1 != v1, n2 = v2 != v2;
  if (n1 || n2) return n1 && (!n2 || i1 < i2);
  return v1 > v2 || (v1 == v2 && i1 < i2);
}

struct PickState {
  double bv, hv;   // (values of T, held in double: exact for float and double)
  int bi, hi;
};

AAMD_HD PickState pitch_pick_init() {
  PickState s;
  s.bv = s.hv = -__builtin_huge_val();
  s.bi = s.hi = 0x7fffffff;
  return s;
}

template <typename T>
AAMD_HD void pitch_pick_fold(PickState& s, T v, int lag, const PitchGeom& g) {
  if (lag > g.lag_min && lag <= g.lags && pitch_better(v, lag, (T)s.bv, s.bi)) { s.bv = (double)v; s.bi = lag; }
  if (lag > g.lag_min && lag <= g.half_end && pitch_better(v, lag, (T)s.hv, s.hi)) { s.hv = (double)v; s.hi = lag; }
}

template <typename T>
AAMD_HD void pitch_pick_merge(PickState& s, const PickState& o) {
  if (pitch_better((T)o.bv, o.bi, (T)s.bv, s.bi)) { s.bv = o.bv; s.bi = o.bi; }
  if (pitch_better((T)o.hv, o.hi, (T)s.hv, s.hi)) { s.hv = o.hv; s.hi = o.hi; }
}

// 0.99 rounded to the compute type, as the reference's `thresh * b[0]`
template <typename T>
AAMD_HD int pitch_combine(const PickState& s) {
  const T thresh = T(0.99);
  return ((T)s.hv > thresh * (T)s.bv) ? s.hi : s.bi;
}

// Mode 1: the chunk's NCCF rows to out (rows, F, lags), lags fastest.
template <typename T>
AAMD_HD void pitch_write_nccf(int tid, int nthreads, const PitchGeom& g, int64_t row, int64_t k0, int j0, const T* lds,
                              T* out) {
  const int J = (g.lags - (j0 - 1)) < g.J ? (g.lags - (j0 - 1)) : g.J;
  const int total = g.T * J;
  for (int idx = tid; idx < total; idx += nthreads) {
    const int t = idx / J, j = idx - t * J;
    if (k0 + t >= g.F) continue;
    out[(row * g.F + k0 + t) * g.lags + (j0 - 1) + j] = lds[g.o_nccf + t * (g.G * kR) + j];
  }
}

// Median phase: the lower median of v(0 .. win) by counting select (the values are bounded lags; win is small).
template <typename Get>
AAMD_HD int pitch_lower_median(const Get& v, int win) {
  const int k = (win - 1) / 2;
  for (int a = 0; a < win; ++a) {
    const int x = v(a);
    int less = 0, leq = 0;
    for (int b = 0; b < win; ++b) {
      const int u = v(b);
      less += u < x;
      leq += u <= x;
    }
    if (less <= k && k < leq) return x;
  }
  return v(0);   // unreachable
}

AAMD_HD float pitch_freq(int lag, float sample_rate) {
  const float eps = 1e-9f;
  const float r = 1.0f / (eps + (float)lag);
  return r * sample_rate;
}

// padded[j] = lag[max(j - p, 0)] of one row (clamped at the end too: only read beyond the last output's window)
AAMD_HD int pitch_padded(const PitchGeom& g, const int* lag_row, int64_t j) {
  int64_t src = j - g.p;
  if (src < 0) src = 0;
  if (src >= g.F) src = g.F - 1;
  return lag_row[src];
}

// Median tile of workgroup (row, t0): padded[t0 + j] for j < kMedT + win - 1 (when it fits kMedLds).
AAMD_HD bool pitch_median_tiled(const PitchGeom& g) { return (int64_t)(kMedT + g.win - 1) * 4 <= kMedLds; }

AAMD_HD void pitch_median_fill(int tid, int nthreads, const PitchGeom& g, const int* lag, int64_t row, int64_t t0,
                               int* tile) {
  const int n = kMedT + g.win - 1;
  for (int j = tid; j < n; j += nthreads) tile[j] = pitch_padded(g, lag + row * g.F, t0 + j);
}

struct MedTile {
  const int* p;
  AAMD_HD int operator()(int a) const { return p[a]; }
};

struct MedRow {
  const PitchGeom* g;
  const int* lag_row;
  int64_t t;
  AAMD_HD int operator()(int a) const { return pitch_padded(*g, lag_row, t + a); }
};

// out[row][t0 + tid]; tile == nullptr: the window is read from lag directly
AAMD_HD void pitch_median_out(int tid, const PitchGeom& g, const int* lag, const int* tile, int64_t row, int64_t t0,
                              float* out) {
  const int64_t t = t0 + tid;
  if (t >= g.n_out) return;
  int m;
  if (tile) m = pitch_lower_median(MedTile{tile + tid}, g.win);
  else m = pitch_lower_median(MedRow{&g, lag + row * g.F, t}, g.win);
  out[row * g.n_out + t] = pitch_freq(m, g.sample_rate);
}

#if defined(__HIPCC__)

template <typename T>
__global__ __launch_bounds__(kThreads) void pitch_nccf_pick_kernel(const T* __restrict__ x, PitchGeom g,
                                                                  int32_t* __restrict__ lag_out, T* __restrict__ nccf_out) {
  extern __shared__ __align__(16) unsigned char smem[];
  T* lds = reinterpret_cast<T*>(smem);
  PickState* st = reinterpret_cast<PickState*>(smem + g.lds_elems * (int64_t)sizeof(T));
  const int64_t row = blockIdx.x / g.n_ftiles;
  const int64_t k0 = (blockIdx.x - row * g.n_ftiles) * (int64_t)g.T;
  const T* xr = x + row * g.rs;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  pitch_stage_s1<T>(tid, kThreads, g, xr, k0, lds);
  for (int t = tid; t < g.T; t += kThreads) st[t] = pitch_pick_init();
  for (int c = 0; c < g.n_chunks; ++c) {
    const int j0 = 1 + c * g.J;
    if (c > 0) __syncthreads();                      // the previous chunk's reads of seg2 / nccf are done
    pitch_stage_seg2<T>(tid, kThreads, g, xr, k0, j0, lds);
    __syncthreads();
    pitch_block_sums<T>(tid, kThreads, g, lds);
    __syncthreads();
    pitch_energies<T>(tid, kThreads, g, c == 0, lds);
    __syncthreads();
    pitch_nccf<T>(tid, kThreads, g, lds);
    __syncthreads();
    if (g.mode == 1) {
      pitch_write_nccf<T>(tid, kThreads, g, row, k0, j0, lds, nccf_out);
      continue;
    }
    const int J = (g.lags - (j0 - 1)) < g.J ? (g.lags - (j0 - 1)) : g.J;
    for (int t = wave; t < g.T; t += kWaves) {
      PickState s = pitch_pick_init();
      const T* row_n = lds + g.o_nccf + t * (g.G * kR);
      for (int j = lane; j < J; j += 64) pitch_pick_fold<T>(s, row_n[j], j0 + j, g);
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) {
        PickState o;
        o.bv = __shfl_xor(s.bv, off);
        o.bi = __shfl_xor(s.bi, off);
        o.hv = __shfl_xor(s.hv, off);
        o.hi = __shfl_xor(s.hi, off);
        pitch_pick_merge<T>(s, o);
      }
      if (lane == 0) {
        PickState m = st[t];
        pitch_pick_merge<T>(m, s);
        st[t] = m;
        if (c == g.n_chunks - 1 && k0 + t < g.F) lag_out[row * g.F + k0 + t] = pitch_combine<T>(m);
      }
    }
  }
}

__global__ __launch_bounds__(kThreads) void pitch_median_kernel(const int32_t* __restrict__ lag, float* __restrict__ out,
                                                                PitchGeom g) {
  extern __shared__ __align__(16) unsigned char smem[];
  int* tile = reinterpret_cast<int*>(smem);
  const int64_t per_row = (g.n_out + kMedT - 1) / kMedT;
  const int64_t row = blockIdx.x / per_row;
  const int64_t t0 = (blockIdx.x - row * per_row) * kMedT;
  const bool tiled = pitch_median_tiled(g);
  if (tiled) {
    pitch_median_fill(threadIdx.x, kThreads, g, lag, row, t0, tile);
    __syncthreads();
  }
  pitch_median_out(threadIdx.x, g, lag, tiled ? tile : nullptr, row, t0, out);
}

#endif

}  // namespace pt
}  // namespace aamd
