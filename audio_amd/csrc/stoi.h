// Short-time objective intelligibility (F.stoi): STOI and ESTOI of every row of a batch at 10 kHz, on the device, without a
// host read-back.  The definition (README, tests/stoi_oracle.py): 256-sample Hann frames at hop 128; the frames of the clean
// signal within 40 dB of its loudest one are kept and both signals rebuilt from them by overlap-add; 512-point spectra of the
// rebuilt signals' frames, 15 third-octave band magnitudes per frame; a correlation statistic over every run of 30 frames.
// Five launches:
//   energy_kernel    one workgroup per (row, 8 frames): 32 lanes per frame, the float64 sum of (w x)^2 as 8 terms per lane
//                    and a fixed tree over the 32 lanes, stored in dB; the workgroup also scans its 1024 samples of both
//                    signals (the row's last workgroup: up to the row's length) for a non-finite value, one flag each.
//   select_kernel    one workgroup per row: the largest energy (tree), the keep flags, an exclusive scan of the per-thread
//                    counts and the ascending list kept[row][j]; n_kept[row], or -1 for a row that scores NaN (a length outside
//                    [0, T], a non-finite sample below the length).
//   tob_kernel       one workgroup per (row, 8 output frames): the 9 hops of both rebuilt signals are gathered into LDS (at
//                    most two kept source frames per sample); each of the 4 waves transforms two frames, x + i y as ONE complex
//                    512-point radix-2 transform in LDS (the zero-padded upper half makes the first stage a copy, done by the
//                    load), separates the two spectra by conjugate symmetry over the bins 7 ... 218 only, sums the 15 bands in
//                    ascending bin order and writes their square roots.  Neither the rebuilt signals nor a spectrum reach memory.
//   segment_kernel   one workgroup per (row, 16 segments), one lane per (segment, band): 45 frames of both band matrices in
//                    LDS as float64, the statistic in float64; ESTOI's column step goes across the 15 band lanes of a segment
//                    through LDS.  A fixed tree folds the workgroup's 240 values into one partial.
//   finish_kernel    one wave per row: folds the row's partials in a fixed order and writes the score, 1e-5 or NaN.
// No atomics: two calls give the same bits; a row's arithmetic depends on the row alone (its own length and kept list), so a row
// of a batch equals the call on that row.  The window and the twiddles are computed in the kernels (float64 cos / sin, rounded
// once to the compute type): no table is cached, so a first call can be captured in a graph.  Sample loads are scalar and
// coalesced (a row of a batch need not be 16-byte aligned).  No data value is used as an index: kept indices come from the scan
// over flags and are compared with the row's frame count before use.
//
// The phase functions are AAMD_HD: tests/cpu_sim/sim_stoi.cpp replays them with g++.
#pragma once
#include <math.h>

#include "wave_augment.h"

namespace aamd {
namespace stoi {

using wa::Elem;
using wa::rounded;

constexpr int kThreads = 256;            // per workgroup of the first four kernels
constexpr int kFinishThreads = 64;
constexpr int kFrame = 256, kHop = 128, kFft = 512, kLogFft = 9, kBands = 15, kSeg = 30;
constexpr int kEnergyFrames = 8;         // frames per workgroup of energy_kernel: 32 lanes each
constexpr int kEnergySpan = kEnergyFrames * kHop;
constexpr int kTobFrames = 8;            // output frames per workgroup of tob_kernel: 4 waves x 2 rounds
constexpr int kTobSpan = (kTobFrames + 1) * kHop;
constexpr int kSegTile = 16;             // segments per workgroup of segment_kernel: 16 x 15 = 240 lanes
constexpr int kSegRows = kSegTile + kSeg - 1;
constexpr int kBin0 = 7, kBins = 212;    // the bins the bands cover: 7 ... 218
constexpr double kEps = 2.220446049250313e-16;     // 2^-52
constexpr double kRange = 40.0;
constexpr double kClip = 6.623413251903491;        // 1 + 10^0.75
constexpr double kShort = 1e-5;

struct Args {
  const void* x;                // target (clean): (rows, T), unit sample stride, row stride sx
  const void* y;                // preds (processed), row stride sy
  const void* lengths;          // [rows] int32 / int64, or null
  int64_t rows, T, sx, sy;
  int64_t K_max, M_max;         // frames of a row of T samples; K_max - 1 (at least 0)
  int64_t nb_e, nt_seg;         // workgroups per row of energy_kernel and of segment_kernel
  int32_t len64, extended;
  double* e;                    // (rows, K_max) frame energies in dB
  int32_t* bad;                 // (rows, nb_e)
  int32_t* kept;                // (rows, K_max)
  int32_t* n_kept;              // (rows)
  void* tob;                    // (rows, 2, M_max, 15) of the compute type
  double* part;                 // (rows, nt_seg)
  void* out;                    // (rows) of the compute type
};

AAMD_HD int band_edge(int b) {            // lo_b = edge b, hi_b = edge b + 1
  constexpr int edges[kBands + 1] = {7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219};
  return edges[b];
}

AAMD_HD int64_t frames_of(int64_t L) { return L >= kFrame ? (L - kFrame) / kHop + 1 : 0; }
AAMD_HD int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// the row's length, or -1 where it lies outside [0, T]
AAMD_HD int64_t row_length(const Args& a, int64_t row) {
  int64_t L = a.T;
  if (a.lengths) L = a.len64 ? static_cast<const int64_t*>(a.lengths)[row] : (int64_t) static_cast<const int32_t*>(a.lengths)[row];
  return (L < 0 || L > a.T) ? -1 : L;
}

// the row's kept frames and output frames from n_kept, compared with their static bounds; false: nothing to transform
AAMD_HD bool row_frames(const Args& a, int64_t row, int64_t& K, int64_t& M) {
  const int64_t k = a.n_kept[row];
  K = (k < 0 || k > a.K_max) ? 0 : k;
  M = K > 0 ? K - 1 : 0;
  return k >= 0 && M >= kSeg && M <= a.M_max;
}

AAMD_HD double window64(int n) { return 0.5 - 0.5 * cos(2.0 * 3.141592653589793 * (double)(n + 1) / 257.0); }

template <typename C>
AAMD_HD bool finite(C v) { return (v - v) == (C)0; }

// ---- frame energies ------------------------------------------------------------------------------------------------------------
// lanes 32 fi ... 32 fi + 31 share frame fi of the block: 8 terms each, in float64 from the samples as stored
template <int DT>
AAMD_HD double energy_partial(int tid, const Args& a, int64_t row, int64_t L, int64_t blk, const double* w) {
  using E = Elem<DT>;
  const int fi = tid >> 5, l = tid & 31;
  const int64_t f = blk * kEnergyFrames + fi;
  if (L < 0 || f >= frames_of(L)) return 0.0;
  const typename E::S* x = static_cast<const typename E::S*>(a.x) + row * a.sx + f * kHop;
  double acc = 0.0;
  for (int k = 0; k < kFrame / 32; ++k) {
    const int n = l + 32 * k;
    const double v = w[n] * (double)E::load(x[n]);
    acc += v * v;
  }
  return acc;
}

AAMD_HD void energy_tree_step(int tid, int stride, double* red) {
  if ((tid & 31) < stride) red[tid] += red[tid + stride];
}

AAMD_HD void energy_write(int tid, const Args& a, int64_t row, int64_t L, int64_t blk, const double* red) {
  const int64_t f = blk * kEnergyFrames + (tid >> 5);
  if ((tid & 31) == 0 && L >= 0 && f < frames_of(L) && f < a.K_max) a.e[row * a.K_max + f] = 20.0 * log10(sqrt(red[tid]) + kEps);
}

// 1 where one of this thread's samples of the block, of either signal, is not finite (or the row's length is bad)
template <int DT>
AAMD_HD int nonfinite_thread(int tid, const Args& a, int64_t row, int64_t L, int64_t blk) {
  using E = Elem<DT>;
  if (L < 0) return 1;
  const int64_t nb = ceil_div(frames_of(L), kEnergyFrames);
  const int64_t start = blk * kEnergySpan;
  int64_t end = blk + 1 >= nb ? L : start + kEnergySpan;      // the row's last block takes the tail no frame covers
  if (end > L) end = L;
  const typename E::S* x = static_cast<const typename E::S*>(a.x) + row * a.sx;
  const typename E::S* y = static_cast<const typename E::S*>(a.y) + row * a.sy;
  int bad = 0;
  for (int64_t i = start + tid; i < end; i += kThreads) bad |= (!finite(E::load(x[i]))) | (!finite(E::load(y[i])));
  return bad;
}

// ---- the kept list -------------------------------------------------------------------------------------------------------------
AAMD_HD int select_bad(int tid, const Args& a, int64_t row) {
  int bad = 0;
  for (int64_t j = tid; j < a.nb_e; j += kThreads) bad |= a.bad[row * a.nb_e + j];
  return bad;
}

AAMD_HD double select_max(int tid, const Args& a, int64_t row, int64_t K_all) {
  double m = -INFINITY;
  for (int64_t i = tid; i < K_all; i += kThreads) {
    const double v = a.e[row * a.K_max + i];
    if (v > m) m = v;
  }
  return m;
}

AAMD_HD void max_step(int tid, int stride, double* s) {
  if (tid < stride && s[tid + stride] > s[tid]) s[tid] = s[tid + stride];
}

// thread tid owns the frames [tid c, (tid + 1) c) with c = ceil(K_all / 256)
AAMD_HD int select_count(int tid, const Args& a, int64_t row, int64_t K_all, double mx) {
  const int64_t c = ceil_div(K_all, kThreads);
  const int64_t i1 = (tid + 1) * c < K_all ? (tid + 1) * c : K_all;
  int n = 0;
  for (int64_t i = tid * c; i < i1; ++i) n += a.e[row * a.K_max + i] > mx - kRange ? 1 : 0;
  return n;
}

AAMD_HD void scan_step(int tid, int stride, const int* src, int* dst) {       // inclusive, Hillis-Steele
  dst[tid] = tid >= stride ? src[tid] + src[tid - stride] : src[tid];
}

AAMD_HD void select_write(int tid, const Args& a, int64_t row, int64_t K_all, double mx, int before) {
  const int64_t c = ceil_div(K_all, kThreads);
  const int64_t i1 = (tid + 1) * c < K_all ? (tid + 1) * c : K_all;
  int64_t j = before;
  for (int64_t i = tid * c; i < i1; ++i)
    if (a.e[row * a.K_max + i] > mx - kRange && j < a.K_max) a.kept[row * a.K_max + j++] = (int32_t)i;
}

// ---- band magnitudes -----------------------------------------------------------------------------------------------------------
AAMD_HD int pidx(int p) { return p + (p >> 5); }
constexpr int kPlane = kFft - 1 + ((kFft - 1) >> 5) + 1;     // words of one plane of the transform: 527

AAMD_HD uint32_t bitrev9(uint32_t v) {
  v = ((v >> 1) & 0x55555555u) | ((v & 0x55555555u) << 1);
  v = ((v >> 2) & 0x33333333u) | ((v & 0x33333333u) << 2);
  v = ((v >> 4) & 0x0f0f0f0fu) | ((v & 0x0f0f0f0fu) << 4);
  v = ((v >> 8) & 0x00ff00ffu) | ((v & 0x00ff00ffu) << 8);
  v = (v >> 16) | (v << 16);
  return v >> (32 - kLogFft);
}

// the LDS of one tob workgroup, in words of the compute type
constexpr int kTobW = 0, kTobTwr = kTobW + kFrame, kTobTwi = kTobTwr + kFft / 2, kTobXs = kTobTwi + kFft / 2,
              kTobYs = kTobXs + kTobSpan, kTobPlanes = kTobYs + kTobSpan, kTobPw = kTobPlanes + 4 * 2 * kPlane,
              kTobWords = kTobPw + 4 * 2 * kBins;
template <typename C>
AAMD_HD size_t tob_lds_bytes() { return (size_t)kTobWords * sizeof(C); }

template <typename C>
AAMD_HD void tob_tables(int tid, C* w, C* twr, C* twi) {
  w[tid] = (C)window64(tid);
  const double ang = -2.0 * 3.141592653589793 * (double)tid / (double)kFft;
  twr[tid] = (C)cos(ang);
  twi[tid] = (C)sin(ang);
}

// one sample of a rebuilt signal: hop h of the kept list (h <= K - 1), offset r < 128
template <int DT>
AAMD_HD typename Elem<DT>::C rebuilt_sample(const void* sig, int64_t row_off, const int32_t* kept, int64_t K, int64_t K_all, int64_t h,
                                            int r, const typename Elem<DT>::C* w) {
  using E = Elem<DT>;
  using C = typename E::C;
  const typename E::S* x = static_cast<const typename E::S*>(sig) + row_off;
  C v = (C)0;
  if (h < K) {
    const int64_t i1 = kept[h];
    if (i1 >= 0 && i1 < K_all) v = rounded(w[r] * E::load(x[i1 * kHop + r]));
  }
  if (h >= 1 && h - 1 < K) {
    const int64_t i0 = kept[h - 1];
    if (i0 >= 0 && i0 < K_all) v += rounded(w[r + kHop] * E::load(x[i0 * kHop + r + kHop]));
  }
  return v;
}

template <int DT>
AAMD_HD void tob_gather(int tid, const Args& a, int64_t row, int64_t K, int64_t K_all, int64_t blk, const typename Elem<DT>::C* w,
                        typename Elem<DT>::C* xs, typename Elem<DT>::C* ys) {
  const int32_t* kept = a.kept + row * a.K_max;
  for (int i = tid; i < kTobSpan; i += kThreads) {
    const int64_t h = blk * kTobFrames + (i >> 7);
    const int r = i & (kHop - 1);
    xs[i] = rebuilt_sample<DT>(a.x, row * a.sx, kept, K, K_all, h, r, w);
    ys[i] = rebuilt_sample<DT>(a.y, row * a.sy, kept, K, K_all, h, r, w);
  }
}

// frame fl (0 ... 7) of the block, windowed again, as x + i y in bit-reversed order; the upper half of the 512 points is zero,
// so the first stage copies every even position to the odd one after it
template <typename C>
AAMD_HD void tob_frame_load(int lane, int fl, const C* w, const C* xs, const C* ys, C* re, C* im) {
  for (int k = 0; k < kFrame / 64; ++k) {
    const int n = lane + 64 * k;
    const C zr = w[n] * xs[fl * kHop + n], zi = w[n] * ys[fl * kHop + n];
    const int j = (int)bitrev9((uint32_t)n);
    re[pidx(j)] = zr; im[pidx(j)] = zi;
    re[pidx(j + 1)] = zr; im[pidx(j + 1)] = zi;
  }
}

// stage s (1 ... 8) of the decimation-in-time transform, 4 butterflies per lane of the wave
template <typename C>
AAMD_HD void tob_fft_stage(int lane, int s, const C* twr, const C* twi, C* re, C* im) {
  const int half = 1 << s;
  for (int k = 0; k < kFft / 2 / 64; ++k) {
    const int j = lane + 64 * k;
    const int pos = j & (half - 1);
    const int i0 = pidx(((j >> s) << (s + 1)) + pos), i1 = pidx(((j >> s) << (s + 1)) + pos + half);
    const int t = pos << (kLogFft - 1 - s);
    const C wr = twr[t], wi = twi[t];
    const C xr = re[i1], xi = im[i1], ur = re[i0], ui = im[i0];
    const C tr = xr * wr - xi * wi, ti = xr * wi + xi * wr;
    re[i0] = ur + tr; im[i0] = ui + ti;
    re[i1] = ur - tr; im[i1] = ui - ti;
  }
}

// |X[f]|^2 and |Y[f]|^2 of the bins 7 ... 218 from Z = FFT(x + i y): X = (Z[f] + conj Z[512 - f]) / 2, Y = (Z[f] - conj Z[512 - f]) / 2i
template <typename C>
AAMD_HD void tob_power(int lane, const C* re, const C* im, C* pw) {
  for (int q = lane; q < kBins; q += 64) {
    const int f = kBin0 + q, g = kFft - f;
    const C ar = re[pidx(f)], ai = im[pidx(f)], br = re[pidx(g)], bi = im[pidx(g)];
    const C xr = (C)0.5 * (ar + br), xi = (C)0.5 * (ai - bi), yr = (C)0.5 * (ai + bi), yi = (C)0.5 * (br - ar);
    pw[q] = xr * xr + xi * xi;
    pw[kBins + q] = yr * yr + yi * yi;
  }
}

// lanes 0 ... 29: band lane % 15 of signal lane / 15, summed in ascending bin order
template <typename C>
AAMD_HD void tob_bands(int lane, const Args& a, int64_t row, int64_t m, const C* pw) {
  if (lane >= 2 * kBands) return;
  const int sig = lane / kBands, b = lane - sig * kBands;
  C acc = (C)0;
  for (int f = band_edge(b); f < band_edge(b + 1); ++f) acc += pw[sig * kBins + f - kBin0];
  static_cast<C*>(a.tob)[((row * 2 + sig) * a.M_max + m) * kBands + b] = sqrt(acc);
}

// ---- the segment statistic -----------------------------------------------------------------------------------------------------
// frames s0 ... s0 + 44 of both band matrices as float64; zero beyond the row's M
template <typename C>
AAMD_HD void seg_stage(int tid, const Args& a, int64_t row, int64_t M, int64_t s0, double* tx, double* ty) {
  const C* t = static_cast<const C*>(a.tob);
  for (int i = tid; i < kSegRows * kBands; i += kThreads) {
    const int64_t m = s0 + i / kBands;
    const int b = i % kBands;
    const bool in = m < M;
    tx[i] = in ? (double)t[((row * 2 + 0) * a.M_max + m) * kBands + b] : 0.0;
    ty[i] = in ? (double)t[((row * 2 + 1) * a.M_max + m) * kBands + b] : 0.0;
  }
}

// STOI of (segment sl of the tile, band b): the clipped, normalised correlation over the 30 frames
AAMD_HD double seg_stoi_lane(int sl, int b, const double* tx, const double* ty) {
  const double* pa = tx + sl * kBands + b;
  const double* pc = ty + sl * kBands + b;
  double sa = 0.0, saa = 0.0, scc = 0.0;
#pragma unroll 2
  for (int t = 0; t < kSeg; ++t) {
    const double av = pa[t * kBands], cv = pc[t * kBands];
    sa += av; saa += av * av; scc += cv * cv;
  }
  const double alpha = sqrt(saa) / (sqrt(scc) + kEps);
  double sc = 0.0;
#pragma unroll 2
  for (int t = 0; t < kSeg; ++t) sc += fmin(alpha * pc[t * kBands], kClip * pa[t * kBands]);
  const double ma = sa / kSeg, mc = sc / kSeg;
  double daa = 0.0, dcc = 0.0, dac = 0.0;
#pragma unroll 2
  for (int t = 0; t < kSeg; ++t) {
    const double av = pa[t * kBands] - ma, cv = fmin(alpha * pc[t * kBands], kClip * pa[t * kBands]) - mc;
    daa += av * av; dcc += cv * cv; dac += av * cv;
  }
  return dac / ((sqrt(daa) + kEps) * (sqrt(dcc) + kEps));
}

// ESTOI, rows: the mean and 1 / (norm + EPS) over time of band b of both matrices -> st[4]
AAMD_HD void seg_estoi_rows(int sl, int b, const double* tx, const double* ty, double* st) {
  const double* p[2] = {tx + sl * kBands + b, ty + sl * kBands + b};
  for (int q = 0; q < 2; ++q) {
    double s = 0.0, d = 0.0;
#pragma unroll 2
    for (int t = 0; t < kSeg; ++t) s += p[q][t * kBands];
    const double m = s / kSeg;
#pragma unroll 2
    for (int t = 0; t < kSeg; ++t) {
      const double v = p[q][t * kBands] - m;
      d += v * v;
    }
    st[2 * q] = m;
    st[2 * q + 1] = sqrt(d) + kEps;
  }
}

// ESTOI, columns: frame t of segment sl across the 15 row-normalised bands; `stat` = the segment's [15][4]
AAMD_HD double seg_estoi_col(int sl, int t, const double* tx, const double* ty, const double* stat) {
  const double* pa = tx + (sl + t) * kBands;
  const double* pc = ty + (sl + t) * kBands;
  double sa = 0.0, sc = 0.0;
#pragma unroll 1
  for (int b = 0; b < kBands; ++b) {
    sa += (pa[b] - stat[4 * b]) / stat[4 * b + 1];
    sc += (pc[b] - stat[4 * b + 2]) / stat[4 * b + 3];
  }
  const double ma = sa / kBands, mc = sc / kBands;
  double daa = 0.0, dcc = 0.0, dac = 0.0;
#pragma unroll 1
  for (int b = 0; b < kBands; ++b) {
    const double av = (pa[b] - stat[4 * b]) / stat[4 * b + 1] - ma, cv = (pc[b] - stat[4 * b + 2]) / stat[4 * b + 3] - mc;
    daa += av * av; dcc += cv * cv; dac += av * cv;
  }
  return dac / ((sqrt(daa) + kEps) * (sqrt(dcc) + kEps));
}

AAMD_HD void sum_step(int tid, int stride, double* s) {
  if (tid < stride) s[tid] += s[tid + stride];
}

// ---- the score -------------------------------------------------------------------------------------------------------------------
AAMD_HD double finish_partial(int tid, const Args& a, int64_t row, int64_t tiles) {
  double acc = 0.0;
  for (int64_t t = tid; t < tiles; t += kFinishThreads) acc += a.part[row * a.nt_seg + t];
  return acc;
}

// what the row scores without a statistic: NaN, 1e-5, or 0 with `tiles` set
AAMD_HD double finish_fixed(const Args& a, int64_t row, int64_t& J, int64_t& tiles) {
  int64_t K, M;
  J = tiles = 0;
  if (a.n_kept[row] < 0) return NAN;
  if (!row_frames(a, row, K, M)) return kShort;
  J = M - kSeg + 1;
  tiles = ceil_div(J, kSegTile);
  if (tiles > a.nt_seg) tiles = a.nt_seg;
  return 0.0;
}

AAMD_HD double score_of(const Args& a, double total, int64_t J) { return total / ((double)(a.extended ? kSeg : kBands) * (double)J); }

#if defined(__HIPCC__)
template <int DT>
__global__ __launch_bounds__(kThreads) void energy_kernel(Args a) {
  __shared__ double w[kFrame];
  __shared__ double red[kThreads];
  __shared__ int any_bad;
  const int tid = threadIdx.x;
  const int64_t row = (int64_t)blockIdx.x / a.nb_e, blk = (int64_t)blockIdx.x - row * a.nb_e;
  const int64_t L = row_length(a, row);
  w[tid] = window64(tid);
  if (tid == 0) any_bad = 0;
  __syncthreads();
  red[tid] = energy_partial<DT>(tid, a, row, L, blk, w);
  if (nonfinite_thread<DT>(tid, a, row, L, blk)) any_bad = 1;       // every writer stores the same value
  __syncthreads();
  for (int stride = 16; stride > 0; stride >>= 1) {
    energy_tree_step(tid, stride, red);
    __syncthreads();
  }
  energy_write(tid, a, row, L, blk, red);
  if (tid == 0) a.bad[row * a.nb_e + blk] = any_bad;
}

__global__ __launch_bounds__(kThreads) void select_kernel(Args a) {
  __shared__ double smax[kThreads];
  __shared__ int cnt[2][kThreads];
  __shared__ int any_bad;
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;
  const int64_t L = row_length(a, row);
  int64_t K_all = L < 0 ? 0 : frames_of(L);
  if (K_all > a.K_max) K_all = a.K_max;
  if (tid == 0) any_bad = L < 0 ? 1 : 0;
  __syncthreads();
  if (select_bad(tid, a, row)) any_bad = 1;
  smax[tid] = select_max(tid, a, row, K_all);
  __syncthreads();
  for (int stride = kThreads >> 1; stride > 0; stride >>= 1) {
    max_step(tid, stride, smax);
    __syncthreads();
  }
  const double mx = smax[0];
  const int mine = select_count(tid, a, row, K_all, mx);
  cnt[0][tid] = mine;
  __syncthreads();
  int cur = 0;
  for (int stride = 1; stride < kThreads; stride <<= 1) {
    scan_step(tid, stride, cnt[cur], cnt[cur ^ 1]);
    cur ^= 1;
    __syncthreads();
  }
  select_write(tid, a, row, K_all, mx, cnt[cur][tid] - mine);
  if (tid == 0) a.n_kept[row] = any_bad ? -1 : cnt[cur][kThreads - 1];
}

template <int DT>
__global__ __launch_bounds__(kThreads) void tob_kernel(Args a) {
  using C = typename Elem<DT>::C;
  extern __shared__ __align__(16) unsigned char stoi_smem[];
  C* lds = reinterpret_cast<C*>(stoi_smem);
  C *w = lds + kTobW, *twr = lds + kTobTwr, *twi = lds + kTobTwi, *xs = lds + kTobXs, *ys = lds + kTobYs;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  C* re = lds + kTobPlanes + wave * 2 * kPlane;
  C* im = re + kPlane;
  C* pw = lds + kTobPw + wave * 2 * kBins;
  const int64_t nblk = ceil_div(a.M_max, kTobFrames);
  const int64_t row = (int64_t)blockIdx.x / nblk, blk = (int64_t)blockIdx.x - row * nblk;
  int64_t K, M;
  if (!row_frames(a, row, K, M) || blk * kTobFrames >= M) return;      // uniform over the workgroup
  const int64_t L = row_length(a, row);
  const int64_t K_all = L < 0 ? 0 : frames_of(L);
  tob_tables(tid, w, twr, twi);
  __syncthreads();
  tob_gather<DT>(tid, a, row, K, K_all, blk, w, xs, ys);
  __syncthreads();
  for (int rnd = 0; rnd < kTobFrames / 4; ++rnd) {
    const int fl = rnd * 4 + wave;
    const int64_t m = blk * kTobFrames + fl;
    const bool live = m < M;                                           // uniform over the wave
    if (live) tob_frame_load(lane, fl, w, xs, ys, re, im);
    __syncthreads();
    for (int s = 1; s < kLogFft; ++s) {
      if (live) tob_fft_stage(lane, s, twr, twi, re, im);
      __syncthreads();
    }
    if (live) tob_power(lane, re, im, pw);
    __syncthreads();
    if (live) tob_bands(lane, a, row, m, pw);
    __syncthreads();
  }
}

template <typename C>
__global__ __launch_bounds__(kThreads) void segment_kernel(Args a) {
  __shared__ double tx[kSegRows * kBands], ty[kSegRows * kBands];
  __shared__ double stat[kSegTile * kBands * 4];
  __shared__ double red[kThreads];
  const int tid = threadIdx.x;
  const int64_t row = (int64_t)blockIdx.x / a.nt_seg, tile = (int64_t)blockIdx.x - row * a.nt_seg;
  int64_t K, M;
  if (!row_frames(a, row, K, M)) return;
  const int64_t J = M - kSeg + 1, s0 = tile * kSegTile;
  if (s0 >= J) return;                                                 // uniform over the workgroup
  seg_stage<C>(tid, a, row, M, s0, tx, ty);
  __syncthreads();
  const int sl = tid / kBands, b = tid - sl * kBands;
  const bool live = sl < kSegTile && s0 + sl < J;
  double v = 0.0;
  if (a.extended) {
    if (live) seg_estoi_rows(sl, b, tx, ty, stat + (sl * kBands + b) * 4);
    __syncthreads();
    if (live) v = seg_estoi_col(sl, b, tx, ty, stat + sl * kBands * 4) + seg_estoi_col(sl, b + kBands, tx, ty, stat + sl * kBands * 4);
  } else if (live) {
    v = seg_stoi_lane(sl, b, tx, ty);
  }
  red[tid] = v;
  __syncthreads();
  for (int stride = kThreads >> 1; stride > 0; stride >>= 1) {
    sum_step(tid, stride, red);
    __syncthreads();
  }
  if (tid == 0) a.part[row * a.nt_seg + tile] = red[0];
}

template <typename C>
__global__ __launch_bounds__(kFinishThreads) void finish_kernel(Args a) {
  __shared__ double red[kFinishThreads];
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;
  int64_t J, tiles;
  const double fixed = finish_fixed(a, row, J, tiles);
  red[tid] = finish_partial(tid, a, row, tiles);
  __syncthreads();
  for (int stride = kFinishThreads >> 1; stride > 0; stride >>= 1) {
    sum_step(tid, stride, red);
    __syncthreads();
  }
  if (tid == 0) static_cast<C*>(a.out)[row] = (C)(J > 0 ? score_of(a, red[0], J) : fixed);
}
#endif

}  // namespace stoi
}  // namespace aamd
