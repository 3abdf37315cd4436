// Separation metrics (F.signal_distortion_ratio, F.scale_invariant_signal_distortion_ratio, F.scale_invariant_signal_noise_ratio,
// F.signal_noise_ratio): every row of a batch scored on the device, without atomics and without a host read-back.  The
// definitions are restated in tests/sdr_oracle.py.  All sums are float64 for every input dtype; samples are read as stored
// through the row stride and widened on load; nothing at or beyond a row's length is read.
//   moments_kernel   one workgroup per (row, 4096 samples): the float64 sums of p, t, pp, tt, pt and a non-finite flag, 16-byte
//                    loads, a fixed tree over the 256 lanes.  With zero_mean the sums are of (x - x[0]): the centred moments
//                    then lose nothing to a large DC.  Every later kernel folds a row's partials in ascending order itself
//                    (one lane per moment), which gives the means, the 1 / max(norm, 1e-6) scales and alpha.
//   corr_kernel      SDR's hot kernel: r[k] = sum_n t~[n] t~[n + k] and b[k] = sum_n t~[n] p~[n + k] for k < filter_length as a
//                    Gram product on the float64 matrix cores.  With n = 16 q + i, r[k] = sum_i M[i][i + k] where
//                    M[i][j] = sum_q t~[16 q + i] x~[16 q + j] is 16 x (L + 15): a matrix product over q.  One workgroup per
//                    (row, 8192 samples) walks four staged pieces of 2048 samples: t~ and p~ of the piece, extended by the
//                    column range, go to LDS as float64, already centred and scaled, zero past the row's end (the A operand is
//                    the head of the staged t~).  K-step s of v_mfma_f64_16x16x4_f64 reads A = t~[64 s + lane] and, for column
//                    tile c, B = x~[64 s + 16 c + lane]: contiguous 64-double LDS reads.  Waves 0 / 2 own the even / odd column
//                    tiles of r, waves 1 / 3 those of b: at most 17 tiles = 136 accumulator registers a wave, kept across the
//                    four pieces.  Epilogue: a tile goes to LDS, 31 lanes sum its diagonals in ascending row order, then one lane
//                    per lag adds the two tiles that hold its 16 entries and writes the workgroup's partial.
//   solve_kernel     one wave per row: folds the partials in ascending order, adds load_diag, runs the Levinson recursion for a
//                    general right-hand side in float64 with the forward vector and the solution 8 elements per lane (the
//                    reversal goes through LDS), wave-synchronous; coh = b . h + h . (b - T h) and the score.  A step whose prediction error
//                    is not finite and positive makes the row NaN.  Nothing is indexed with a data value.
//   residual_kernel  SI-SDR / SNR: sum of (alpha t - p)^2 per (row, 4096 samples), summed directly (the algebraic form cancels
//                    at high SDR), 16-byte loads.
//   finish_kernel    one wave per row: the score, and the row's eight statistics for the backward.
//   grad_kernel      grad_preds and / or grad_target = c1 p + c2 t + c3 with per-row float64 coefficients; half types are
//                    rounded once; exactly zero at or beyond the row's length.
// Chunks, pieces and spans are anchored at a row's first sample and depend on nothing but the index, so row b of a batch equals
// the call on row b and a row with lengths[b] equals the call on row[:lengths[b]], bit for bit.
#pragma once
#include <math.h>

#include "wave_augment.h"

namespace aamd {
namespace sdr {

using wa::Elem;
using wa::Vec;

constexpr int kThreads = 256;
constexpr int kChunk = 4096;             // samples per workgroup of the streaming kernels
constexpr int kStage = 2048;             // samples of a staged piece of corr_kernel: 32 K-steps of 64
constexpr int kWalk = 4;                 // pieces a workgroup walks with its accumulators in registers
constexpr int kSpan = kStage * kWalk;    // samples per workgroup of corr_kernel
constexpr int kLagsSmall = 64, kLagsMax = 512;
constexpr int kTilesSmall = (kLagsSmall + 15 + 15) / 16, kTilesMax = (kLagsMax + 15 + 15) / 16;   // column tiles: 5 and 33
constexpr int kSolveThreads = 64;
constexpr int kMom = 6;                  // p, t, pp, tt, pt, non-finite
constexpr int kStat = 8;                 // N, centre of p, centre of t, tt, pt, alpha, residual, bad
constexpr int kTilePitch = 17;
enum { kModeSdr = 0, kModeSi = 1, kModeSnr = 2 };

struct Args {
  const void *p, *t;            // preds, target: (rows, T), unit sample stride, row strides sp / st
  const void* lengths;          // [rows] int32 / int64, or null
  int64_t rows, T, sp, st;
  int64_t chunks, spans;        // workgroups per row of the streaming kernels and of corr_kernel
  int32_t len64, zero_mean, mode, flen, lpad, has_diag, want_p, want_t;
  double load_diag, eps;
  double* mom;                  // (rows, chunks, 6)
  double* res;                  // (rows, chunks), SI-SDR / SNR
  double* corr;                 // (rows, spans, 2, lpad), SDR
  double* stat;                 // (rows, 8), SI-SDR / SNR
  const double* cot;            // (rows), backward
  void *gp, *gt;                // dense (rows, T), backward
  void* out;                    // (rows) float32, or float64 for float64 input
};

struct Stats {
  double N, cp, ct, Spp, Stt, Spt;      // samples, what is subtracted from p and t, the moments of what remains
  bool bad;
};

AAMD_HD int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// the row's length, or -1 where it lies outside [0, T]
AAMD_HD int64_t row_length(const Args& a, int64_t row) {
  int64_t L = a.T;
  if (a.lengths) L = a.len64 ? static_cast<const int64_t*>(a.lengths)[row] : (int64_t) static_cast<const int32_t*>(a.lengths)[row];
  return (L < 0 || L > a.T) ? -1 : L;
}

AAMD_HD bool finite(double v) { return (v - v) == 0.0; }

// the folded sums sh[0 .. 5] of (x - shift) -> the row's statistics
AAMD_HD Stats stats_of(const Args& a, int64_t L, const double* sh, double shp, double sht) {
  Stats s{};
  s.bad = L < 0 || sh[5] != 0.0;
  s.N = L > 0 ? (double)L : 0.0;
  if (a.zero_mean && L > 0) {
    s.cp = shp + sh[0] / s.N;
    s.ct = sht + sh[1] / s.N;
    s.Spp = sh[2] - sh[0] * sh[0] / s.N;
    s.Stt = sh[3] - sh[1] * sh[1] / s.N;
    s.Spt = sh[4] - sh[0] * sh[1] / s.N;
    if (s.Spp < 0.0) s.Spp = 0.0;
    if (s.Stt < 0.0) s.Stt = 0.0;
  } else {
    s.Spp = sh[2]; s.Stt = sh[3]; s.Spt = sh[4];
  }
  return s;
}

AAMD_HD double alpha_of(const Args& a, const Stats& s) { return a.mode == kModeSi ? (s.Spt + a.eps) / (s.Stt + a.eps) : 1.0; }

// the per-row coefficients of grad_preds = g (c[0] p + c[1] t + c[2]) and grad_target = g (c[3] p + c[4] t + c[5]) from stat
AAMD_HD void grad_coef(const Args& a, const double* st, double g, double c[6]) {
  const double cp = st[1], ct = st[2], Stt = st[3], Spt = st[4], al = st[5], Nn = st[6] + a.eps;
  const double k = g * 4.342944819032518;           // 10 / ln 10
  if (a.mode == kModeSi) {
    const double b = Stt + a.eps, S = al * al * Stt + a.eps;
    const double q = a.eps * (Stt - Spt) / b;       // sum (alpha t - p) t = alpha Stt - Spt, without the cancellation
    const double X = 2.0 * al * Stt / (S * b) - 2.0 * q / (Nn * b) + 2.0 * al / Nn;
    c[0] = -2.0 / Nn; c[1] = X; c[3] = X;
    c[4] = (2.0 * al * al - 4.0 * al * al * Stt / b) / S - (2.0 * al * al - 4.0 * al * q / b) / Nn;
  } else {
    c[0] = -2.0 / Nn; c[1] = 2.0 / Nn; c[3] = 2.0 / Nn;
    c[4] = 2.0 / (Stt + a.eps) - 2.0 / Nn;
  }
  c[0] *= k; c[1] *= k; c[3] *= k; c[4] *= k;
  c[2] = -(c[0] * cp + c[1] * ct);
  c[5] = -(c[3] * cp + c[4] * ct);
  if (st[7] != 0.0) c[0] = c[1] = c[2] = c[3] = c[4] = c[5] = NAN;
}

// v rounded ONCE to the storage type: float64 -> float32 to odd, so that the second rounding to a half type is the only one
template <int DT>
AAMD_HD typename Elem<DT>::S store_once(double v) {
  using E = Elem<DT>;
  if (DT == wa::kF64 || DT == wa::kF32) return E::store((typename E::C)v);
  float f = (float)v;
  const double d = (double)f;
  if (d != v && (f - f) == 0.0f) {
    uint32_t bits;
    __builtin_memcpy(&bits, &f, 4);
    if (fabs(d) > fabs(v)) bits -= 1;               // back to the truncated value
    bits |= 1u;
    __builtin_memcpy(&f, &bits, 4);
  }
  return E::store((typename E::C)f);
}

#if defined(__HIPCC__)
typedef double d4 __attribute__((ext_vector_type(4)));

// the lanes of one wave see each other's LDS writes after this; no workgroup barrier
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// lanes 0 .. 5 fold the row's moment partials, lane 6 the residual partials, in ascending chunk order -> sh[0 .. 6]; the
// caller synchronises
__device__ __forceinline__ void fold_row(const Args& a, int64_t row, int64_t L, int tid, double* sh) {
  if (tid > 6) return;
  const int64_t nch = L > 0 ? ceil_div(L, kChunk) : 0;
  double s = 0.0;
  if (tid < kMom) {
    for (int64_t c = 0; c < nch && c < a.chunks; ++c) s += a.mom[(row * a.chunks + c) * kMom + tid];
  } else if (a.res) {
    for (int64_t c = 0; c < nch && c < a.chunks; ++c) s += a.res[row * a.chunks + c];
  }
  sh[tid] = s;
}

// what zero_mean's sums are taken about: the row's first samples
template <int DT>
__device__ __forceinline__ void shift_of(const Args& a, int64_t row, int64_t L, double& shp, double& sht) {
  using E = Elem<DT>;
  shp = sht = 0.0;
  if (a.zero_mean && L > 0) {
    shp = (double)E::load(static_cast<const typename E::S*>(a.p)[row * a.sp]);
    sht = (double)E::load(static_cast<const typename E::S*>(a.t)[row * a.st]);
  }
}

__device__ __forceinline__ void tree_sum(int tid, double* red) {      // red[kThreads], fixed order
  __syncthreads();
  for (int stride = kThreads >> 1; stride > 0; stride >>= 1) {
    if (tid < stride) red[tid] += red[tid + stride];
    __syncthreads();
  }
}

// One thread's share of a chunk: groups g kThreads + tid of 16 bytes, elements in index order; f(p, t) for every sample
// below `end`.
template <int DT, class F>
__device__ __forceinline__ void for_chunk(const Args& a, int64_t row, int64_t chunk, int64_t end, int tid, F f) {
  using E = Elem<DT>;
  using S = typename E::S;
  constexpr int V = 16 / sizeof(S);
  const S* p = static_cast<const S*>(a.p) + row * a.sp;
  const S* t = static_cast<const S*>(a.t) + row * a.st;
  const bool vp = wa::aligned16(p), vt = wa::aligned16(t);
#pragma unroll
  for (int g = 0; g < kChunk / (kThreads * V); ++g) {
    const int64_t i0 = chunk * kChunk + (int64_t)(g * kThreads + tid) * V;
    if (i0 >= end) continue;
    Vec<S> xp, xt;
    wa::load_group(p, vp, i0, end, xp);
    wa::load_group(t, vt, i0, end, xt);
#pragma unroll
    for (int k = 0; k < V; ++k)
      if (i0 + k < end) f(i0 + k, (double)E::load(xp.e[k]), (double)E::load(xt.e[k]));
  }
}

template <int DT>
__global__ __launch_bounds__(kThreads) void moments_kernel(Args a) {
  __shared__ double red[kThreads];
  __shared__ int any_bad;
  const int tid = threadIdx.x;
  const int64_t row = (int64_t)blockIdx.x / a.chunks, chunk = (int64_t)blockIdx.x - row * a.chunks;
  const int64_t L = row_length(a, row);
  if (L <= 0 || chunk * kChunk >= L) return;                           // uniform; such a partial is never folded
  const int64_t end = (chunk + 1) * kChunk < L ? (chunk + 1) * kChunk : L;
  double shp, sht;
  shift_of<DT>(a, row, L, shp, sht);
  double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  int bad = 0;
  for_chunk<DT>(a, row, chunk, end, tid, [&](int64_t, double p, double t) {
    bad |= (!finite(p)) | (!finite(t));
    p -= shp; t -= sht;
    acc[0] += p; acc[1] += t; acc[2] += p * p; acc[3] += t * t; acc[4] += p * t;
  });
  if (tid == 0) any_bad = 0;
  __syncthreads();
  if (bad) any_bad = 1;                                                // every writer stores the same value
  double* out = a.mom + (row * a.chunks + chunk) * kMom;
  for (int m = 0; m < 5; ++m) {
    red[tid] = acc[m];
    tree_sum(tid, red);
    if (tid == 0) out[m] = red[0];
    __syncthreads();
  }
  if (tid == 0) out[5] = any_bad ? 1.0 : 0.0;
}

template <int DT>
__global__ __launch_bounds__(kThreads) void residual_kernel(Args a) {
  __shared__ double red[kThreads];
  __shared__ double sh[8];
  const int tid = threadIdx.x;
  const int64_t row = (int64_t)blockIdx.x / a.chunks, chunk = (int64_t)blockIdx.x - row * a.chunks;
  const int64_t L = row_length(a, row);
  if (L <= 0 || chunk * kChunk >= L) return;
  const int64_t end = (chunk + 1) * kChunk < L ? (chunk + 1) * kChunk : L;
  double shp, sht;
  shift_of<DT>(a, row, L, shp, sht);
  fold_row(a, row, L, tid, sh);
  __syncthreads();
  const Stats s = stats_of(a, L, sh, shp, sht);
  const double al = alpha_of(a, s);
  double acc = 0.0;
  for_chunk<DT>(a, row, chunk, end, tid, [&](int64_t, double p, double t) {
    const double e = al * (t - s.ct) - (p - s.cp);
    acc += e * e;
  });
  red[tid] = acc;
  tree_sum(tid, red);
  if (tid == 0) a.res[row * a.chunks + chunk] = red[0];
}

template <int DT>
__global__ __launch_bounds__(kSolveThreads) void finish_kernel(Args a) {
  using C = typename Elem<DT>::C;
  __shared__ double sh[8];
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;
  const int64_t L = row_length(a, row);
  double shp, sht;
  shift_of<DT>(a, row, L, shp, sht);
  fold_row(a, row, L, tid, sh);
  __syncthreads();
  if (tid != 0) return;
  const Stats s = stats_of(a, L, sh, shp, sht);
  const double al = alpha_of(a, s);
  const double S = al * al * s.Stt + a.eps, Nn = sh[6] + a.eps;
  static_cast<C*>(a.out)[row] = (C)(s.bad ? NAN : 10.0 * log10(S / Nn));
  double* st = a.stat + row * kStat;
  st[0] = s.N; st[1] = s.cp; st[2] = s.ct; st[3] = s.Stt; st[4] = s.Spt; st[5] = al; st[6] = sh[6]; st[7] = s.bad ? 1.0 : 0.0;
}

template <int DT>
__global__ __launch_bounds__(kThreads) void grad_kernel(Args a) {
  using E = Elem<DT>;
  using S = typename E::S;
  constexpr int V = 16 / sizeof(S);
  const int tid = threadIdx.x;
  const int64_t row = (int64_t)blockIdx.x / a.chunks, chunk = (int64_t)blockIdx.x - row * a.chunks;
  int64_t L = row_length(a, row);
  if (L < 0) L = 0;
  double c[6];
  grad_coef(a, a.stat + row * kStat, a.cot[row], c);
  const int64_t cend = (chunk + 1) * kChunk < a.T ? (chunk + 1) * kChunk : a.T;
  const int64_t end = cend < L ? cend : L;                              // samples below it are read
  const S* p = static_cast<const S*>(a.p) + row * a.sp;
  const S* t = static_cast<const S*>(a.t) + row * a.st;
  S* gp = a.want_p ? static_cast<S*>(a.gp) + row * a.T : nullptr;
  S* gt = a.want_t ? static_cast<S*>(a.gt) + row * a.T : nullptr;
  const bool vp = wa::aligned16(p), vt = wa::aligned16(t), vgp = wa::aligned16(gp), vgt = wa::aligned16(gt);
#pragma unroll
  for (int g = 0; g < kChunk / (kThreads * V); ++g) {
    const int64_t i0 = chunk * kChunk + (int64_t)(g * kThreads + tid) * V;
    if (i0 >= cend) continue;
    Vec<S> xp, xt, op, ot;
    wa::load_group(p, vp, i0, end, xp);                                // nothing at or beyond `end` is read
    wa::load_group(t, vt, i0, end, xt);
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const bool in = i0 + k < end;
      const double pv = (double)E::load(xp.e[k]), tv = (double)E::load(xt.e[k]);
      op.e[k] = in ? store_once<DT>(c[0] * pv + c[1] * tv + c[2]) : S(0);
      ot.e[k] = in ? store_once<DT>(c[3] * pv + c[4] * tv + c[5]) : S(0);
    }
    if (gp) wa::store_group(gp, vgp, i0, cend, op);
    if (gt) wa::store_group(gt, vgt, i0, cend, ot);
  }
}

// ---- SDR: the correlations ---------------------------------------------------------------------------------------------------------
template <int NT>
struct CorrGeom {
  static constexpr int kExt = kStage + 16 * (NT - 1);     // staged samples of a signal: the last B read ends at kExt - 1
  static constexpr int kTpw = (NT + 1) / 2;                // column tiles a wave may own
  static constexpr int kDiag = 4 * 16 * kTilePitch;        // epilogue: the four waves' tiles, then [2][NT][32] diagonal sums
  static_assert(kDiag + 2 * NT * 32 <= 2 * kExt, "the epilogue reuses the staging area");
};

template <int DT, int NT>
__global__ __launch_bounds__(kThreads) void corr_kernel(Args a) {
  using E = Elem<DT>;
  using S = typename E::S;
  using G = CorrGeom<NT>;
  __shared__ __align__(16) double lds[2 * G::kExt];
  __shared__ double sh[8];
  double* xt = lds;
  double* xp = lds + G::kExt;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t row = (int64_t)blockIdx.x / a.spans, span = (int64_t)blockIdx.x - row * a.spans;
  const int64_t L = row_length(a, row);
  const int64_t n_begin = span * kSpan;
  if (L <= 0 || n_begin >= L) return;                                  // uniform; such a partial is never folded
  double shp, sht;
  shift_of<DT>(a, row, L, shp, sht);
  fold_row(a, row, L, tid, sh);
  __syncthreads();
  const Stats s = stats_of(a, L, sh, shp, sht);
  const double np = sqrt(s.Spp), nt = sqrt(s.Stt);
  const double scp = 1.0 / (np > 1e-6 ? np : 1e-6), sct = 1.0 / (nt > 1e-6 ? nt : 1e-6);
  const S* p = static_cast<const S*>(a.p) + row * a.sp;
  const S* t = static_cast<const S*>(a.t) + row * a.st;
  const int ntile = (a.flen + 15 + 15) >> 4;                            // column tiles the lags need: at most NT
  const int sig = wave & 1, c_first = wave >> 1;                        // this wave's tiles: c_first, c_first + 2, ...
  const double* xb = sig ? xp : xt;

  d4 acc[G::kTpw];
#pragma unroll
  for (int k = 0; k < G::kTpw; ++k) acc[k] = d4{0.0, 0.0, 0.0, 0.0};

  for (int w = 0; w < kWalk; ++w) {
    const int64_t n0 = n_begin + (int64_t)w * kStage;
    if (n0 >= L) break;                                                 // uniform
    if (w > 0) __syncthreads();
    for (int j = tid; j < G::kExt; j += kThreads) {
      const int64_t n = n0 + j;
      const bool in = n < L;
      xt[j] = in ? ((double)E::load(t[in ? n : 0]) - s.ct) * sct : 0.0;
      xp[j] = in ? ((double)E::load(p[in ? n : 0]) - s.cp) * scp : 0.0;
    }
    __syncthreads();
    const int64_t live = L - n0 < kStage ? L - n0 : kStage;             // K-steps past it multiply zeros
    const int steps = (int)((live + 63) >> 6);
#pragma unroll 1
    for (int st = 0; st < steps; ++st) {
      const double av = xt[64 * st + lane];
#pragma unroll
      for (int k = 0; k < G::kTpw; ++k) {
        const int c = c_first + 2 * k;
        if (c < ntile && c < NT) {                                      // uniform over the wave
          const double bv = xb[64 * st + 16 * c + lane];
          acc[k] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc[k], 0, 0, 0);
        }
      }
    }
  }

  // epilogue: D[i][j] of a tile sits in lane 16 (i & 3) + j, register i >> 2
  __syncthreads();
  double* tile = lds + wave * 16 * kTilePitch;
  double* diag = lds + G::kDiag;
#pragma unroll
  for (int k = 0; k < G::kTpw; ++k) {
    const int c = c_first + 2 * k;
    if (c < ntile && c < NT) {
#pragma unroll
      for (int v = 0; v < 4; ++v) tile[(4 * v + (lane >> 4)) * kTilePitch + (lane & 15)] = acc[k][v];
      wave_sync();
      if (lane < 31) {
        const int d = lane - 15;
        double sum = 0.0;
        for (int i = 0; i < 16; ++i) {
          const int j = i + d;
          if (j >= 0 && j < 16) sum += tile[i * kTilePitch + j];
        }
        diag[(sig * NT + c) * 32 + lane] = sum;
      }
      wave_sync();
    }
  }
  __syncthreads();
  double* out = a.corr + (row * a.spans + span) * 2 * a.lpad;
  for (int idx = tid; idx < 2 * a.flen; idx += kThreads) {
    const int sg = idx >= a.flen ? 1 : 0, kk = idx - sg * a.flen;
    const int c0 = kk >> 4, lo = kk & 15;
    double sum = diag[(sg * NT + c0) * 32 + 15 + lo];                   // rows i with i + lo < 16
    if (lo != 0 && c0 + 1 < NT) sum += diag[(sg * NT + c0 + 1) * 32 + lo - 1];
    out[sg * a.lpad + kk] = sum;
  }
}

// ---- SDR: fold, Levinson, score ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ double wave_sum(double v) {                  // every lane gets the same bits
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// U elements per lane: element e lives in lane e & 63, register e >> 6
template <int DT, int U>
__global__ __launch_bounds__(kSolveThreads) void solve_kernel(Args a) {
  using C = typename Elem<DT>::C;
  __shared__ double r[64 * U], bv[64 * U], fl[64 * U];
  __shared__ double sh[8];
  const int lane = threadIdx.x;
  const int64_t row = blockIdx.x;
  const int64_t L = row_length(a, row);
  const int flen = a.flen < 64 * U ? a.flen : 64 * U;
  double shp, sht;
  shift_of<DT>(a, row, L, shp, sht);
  fold_row(a, row, L, lane, sh);
  const int64_t nsp = L > 0 ? ceil_div(L, kSpan) : 0;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int e = lane + 64 * u;
    double sr = 0.0, sb = 0.0;
    if (e < flen)
      for (int64_t sp = 0; sp < nsp && sp < a.spans; ++sp) {
        const double* c = a.corr + (row * a.spans + sp) * 2 * a.lpad;
        sr += c[e];
        sb += c[a.lpad + e];
      }
    r[e] = sr; bv[e] = sb; fl[e] = 0.0;
  }
  wave_sync();
  const Stats s = stats_of(a, L, sh, shp, sht);
  const double r0 = r[0] + (a.has_diag ? a.load_diag : 0.0);
  bool ok = !s.bad && r0 > 0.0 && finite(r0);
  double f[U], x[U];
#pragma unroll
  for (int u = 0; u < U; ++u) f[u] = x[u] = 0.0;
  if (lane == 0) {
    f[0] = 1.0 / r0;
    x[0] = bv[0] / r0;
    fl[0] = f[0];
    r[0] = r0;
  }
  wave_sync();
  for (int m = 1; m < flen; ++m) {
    double pe = 0.0, px = 0.0;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = lane + 64 * u;
      if (64 * u < m && i < m) {
        const double rv = r[m - i];
        pe += rv * f[u];
        px += rv * x[u];
      }
    }
    const double ef = wave_sum(pe), ex = wave_sum(px);
    const double d = 1.0 - ef * ef;                                     // the step's prediction error over the last one
    ok = ok && d > 0.0 && finite(d);
    const double inv = 1.0 / d;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int j = lane + 64 * u;
      if (64 * u <= m && j <= m) f[u] = (f[u] - ef * fl[m - j]) * inv;  // fl[m] is still zero
    }
    wave_sync();
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int j = lane + 64 * u;
      if (64 * u <= m && j <= m) fl[j] = f[u];
    }
    wave_sync();
    const double cx = bv[m] - ex;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int j = lane + 64 * u;
      if (64 * u <= m && j <= m) x[u] += cx * fl[m - j];
    }
  }
  // coh = b . h + h . (b - T h): the recursion's error in h then enters coh only to second order
  wave_sync();
#pragma unroll
  for (int u = 0; u < U; ++u) fl[lane + 64 * u] = x[u];
  wave_sync();
  double pc = 0.0;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int j = lane + 64 * u;
    if (64 * u < flen) {
      double th = 0.0;
      for (int i = 0; i < flen; ++i) th += r[j >= i ? j - i : i - j] * fl[i];      // j - i stays below 64 U
      if (j < flen) pc += x[u] * (bv[j] + (bv[j] - th));
    }
  }
  const double coh = wave_sum(pc);
  if (lane == 0) static_cast<C*>(a.out)[row] = (C)(ok ? 10.0 * log10(coh / (1.0 - coh)) : NAN);
}
#endif

}  // namespace sdr
}  // namespace aamd
