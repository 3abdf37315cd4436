// Differentiable-DSP synthesis ops (prototype.functional: oscillator_bank, filter_waveform, sinc_impulse_response,
// frequency_impulse_response, extend_pitch).  The definition is tests/dsp_oracle.py; the kernels here are its forward path.
//
// oscillator_bank.  frequencies and amplitudes are (rows, T, N), N innermost.  Per element, in the compute type C (float32
// for float32 and the half types, double for float64): v = (f * 2 pi) / sample_rate with each operation rounded once,
// w = remainder(v, 2 pi) in [0, 2 pi); the phase is the inclusive prefix sum of w over time in float64, reduced to
// [-pi, pi] with a two-term 2 pi, rounded once to C, then sin() and a' = (|f| >= sample_rate / 2 ? 0 : a).  Time is cut
// into chunks of kOscChunk steps from t = 0, so a sample's bits depend on neither the batch nor the call's length.  A
// workgroup of kThreads owns one (row, chunk) and lays its lanes out as (slice, n): TS = kThreads / N time slices of
// S = ceil(kOscChunk / TS) consecutive steps each, so N = 1 keeps 256 lanes busy and N = 64 four slices of 64.  Two launches:
//   osc_sums    per (row, chunk, n): the sum of w over the chunk -- each slice summed in time order, the slices added in
//               ascending order -- reduced mod 2 pi, to the workspace.  The last chunk of a row has no successor and is
//               not summed.
//   osc_apply   the chunk's starting phase is the fold start = reduce(start + sum) over the chunks before it; a lane's
//               base adds the slices before its own in ascending order; it then re-reads its slice and scans it in time
//               order.  "none" stores a' sin(phi) as it goes.  "sum" / "mean" pass kOscSteps steps of every slice through
//               LDS (rows padded to an odd stride) and one lane per output sample runs the fused multiply-add chain
//               acc = fma(a', sin(phi), acc) over ascending n; "mean" divides once.
// Nothing is indexed with a data value; a NaN or infinite frequency makes w NaN, which poisons that oscillator's phase
// from that step on (and every later chunk through the sums).
//
// filter_waveform.  y[n] = sum_j x[m] h[m / C][j], m = n + d - j, d = (L - 1) / 2, C = T / F: every input sample is
// filtered by the filter of its own chunk.  One accumulator per output in ascending m (fused multiply-adds in C).  A
// workgroup owns kFwTile outputs of one row and stages x[tile_start + d - L + 1 .. tile_end + d] in LDS (zeros outside the
// row).  A lane owns kFwPer consecutive outputs; a wave walks m over the span its 64 kFwPer outputs need, with x[m] an LDS
// broadcast, the chunk index a wave-uniform counter and the taps h[c][j0 .. j0 + kFwPer) a register window that slides by
// one tap per step (one load per kFwPer multiply-adds) and is reloaded where m enters another chunk -- at C = 1 every step,
// the diagonal read of `kernels` that case is bound by.  A tap outside [0, L) is skipped by a select, never multiplied by
// zero, so a non-finite sample reaches only the outputs under its filter.
//
// sinc_impulse_response: one workgroup per cutoff, float64 throughout, sum in a fixed order (lane-strided partial sums,
// then the 256 partials in ascending order), every addition with its rounding error kept.  frequency_impulse_response: one
// workgroup per filter; the magnitudes and the host-built cos(2 pi q / N) table live in LDS in C, ir[k] is one fused
// multiply-add chain over ascending j of (c_j m_j) tab[j k mod N].  extend_pitch: one product per element.
//
// The phase functions are AAMD_HD: tests/cpu_sim/sim_dsp.cpp replays them with g++.
#pragma once
#include <math.h>

#include "hd.h"
#include "wave_augment.h"   // wa::Elem, wa::rounded

#if !defined(__HIPCC__)
using std::sin;
using std::cos;
using std::fmod;
using std::fabs;
using std::rint;
#endif

namespace aamd {
namespace dsp {

constexpr int kThreads = 256;
constexpr int kOscChunk = 512;      // time steps per chunk of the scan
constexpr int kOscSteps = 8;        // steps of every slice that pass through LDS together
constexpr int kMaxOsc = 256;        // oscillators: one lane each
constexpr int kFwPer = 4;           // consecutive outputs of a lane
constexpr int kFwTile = kThreads * kFwPer;
constexpr int kMaxTaps = 2049;
constexpr int kMaxMags = 4097;      // (4097 + 8192) doubles of LDS
constexpr double kPi = 3.14159265358979323846;
constexpr double k2PiHi = 6.283185307179586;          // double(2 pi)
constexpr double k2PiLo = 2.4492935982947064e-16;     // 2 pi - double(2 pi)
constexpr double kInv2Pi = 0.15915494309189535;
enum { kSum = 0, kMean = 1, kNone = 2 };

AAMD_HD float d_sin(float v) { return sinf(v); }
AAMD_HD double d_sin(double v) { return sin(v); }
AAMD_HD float d_fmod(float a, float b) { return fmodf(a, b); }
AAMD_HD double d_fmod(double a, double b) { return fmod(a, b); }
AAMD_HD float d_abs(float v) { return fabsf(v); }
AAMD_HD double d_abs(double v) { return fabs(v); }
AAMD_HD float d_fma(float a, float b, float c) { return fmaf(a, b, c); }
AAMD_HD double d_fma(double a, double b, double c) { return fma(a, b, c); }

// x - rint(x / 2 pi) (hi + lo): the first step is exact for |x| < 2^20, the second rounds once
AAMD_HD double reduce_2pi(double x) {
  const double k = rint(x * kInv2Pi);
  return fma(-k, k2PiLo, fma(-k, k2PiHi, x));
}

// ---- oscillator_bank -------------------------------------------------------------------------------------------------------
struct OscArgs {
  const void *freq, *amp;     // (rows, T, N) dense per row, row strides sf / sa in elements
  void* out;                  // (rows, T) or (rows, T, N) dense
  double* sums;               // (rows, chunks, N)
  int64_t rows, T, sf, sa, chunks;
  double sample_rate;
  int32_t N, reduction;
};

struct OscGeom {
  int TS, S, SB, Np;          // slices, steps per slice, steps per LDS pass, padded LDS row
};

AAMD_HD OscGeom osc_geom(int N) {
  OscGeom g;
  g.TS = kThreads / N;
  g.S = (kOscChunk + g.TS - 1) / g.TS;
  g.TS = (kOscChunk + g.S - 1) / g.S;            // the slices that hold a step
  g.SB = g.S < kOscSteps ? g.S : kOscSteps;
  g.Np = N | 1;
  return g;
}
AAMD_HD int osc_lds_values(int N) {
  const OscGeom g = osc_geom(N);
  return g.TS * g.SB * g.Np;
}
// TS SB (N | 1) <= SB (TS N + TS): 8 (256 + 64) where a slice has 8 steps or more (TS <= 64); otherwise SB = S, TS S <= 512 + TS
// and N <= 3, so at most 768 * 3.  tests/test_dsp_synth.py checks every N.
constexpr int kOscLdsValues = kOscSteps * (kThreads + 64);

template <typename C>
AAMD_HD C osc_w(C f, C two_pi, C sr) {
  const C v = wa::rounded(f * two_pi) / sr;
  C w = d_fmod(v, two_pi);
  if (w != C(0) && w < C(0)) w = w + two_pi;
  return w;
}

// the sum of w over the steps of lane `tid`'s slice that lie in the row, in time order
template <int DT>
AAMD_HD double osc_slice_sum(int tid, const OscArgs& a, const OscGeom& g, int64_t row, int64_t chunk) {
  using E = wa::Elem<DT>;
  using C = typename E::C;
  const int ts = tid / a.N, n = tid - ts * a.N;
  if (ts >= g.TS) return 0.0;
  const typename E::S* f = static_cast<const typename E::S*>(a.freq) + row * a.sf;
  const C two_pi = (C)(2.0 * kPi), sr = (C)a.sample_rate;
  const int64_t t0 = chunk * kOscChunk + (int64_t)ts * g.S;
  double sum = 0.0;
  for (int s = 0; s < g.S; ++s) {
    const int64_t t = t0 + s;
    if (ts * g.S + s < kOscChunk && t < a.T) sum += (double)osc_w<C>(E::load(f[t * a.N + n]), two_pi, sr);
  }
  return sum;
}

// osc_sums: lane n < N adds the slices in ascending order
AAMD_HD void osc_chunk_sum(int tid, const OscArgs& a, const OscGeom& g, int64_t row, int64_t chunk, const double* sub) {
  if (tid >= a.N) return;
  double sum = 0.0;
  for (int ts = 0; ts < g.TS; ++ts) sum += sub[ts * a.N + tid];
  a.sums[(row * a.chunks + chunk) * a.N + tid] = reduce_2pi(sum);
}

// osc_apply: lane n < N folds the sums of the chunks before this one
AAMD_HD void osc_start(int tid, const OscArgs& a, int64_t row, int64_t chunk, double* start) {
  if (tid >= a.N) return;
  double st = 0.0;
  for (int64_t c = 0; c < chunk; ++c) st = reduce_2pi(st + a.sums[(row * a.chunks + c) * a.N + tid]);
  start[tid] = st;
}

AAMD_HD double osc_base(int tid, const OscArgs& a, const OscGeom& g, const double* start, const double* sub) {
  const int ts = tid / a.N, n = tid - ts * a.N;
  if (ts >= g.TS) return 0.0;
  double base = start[n];
  for (int q = 0; q < ts; ++q) base += sub[q * a.N + n];
  return base;
}

// steps s0 .. s0 + SB of lane `tid`'s slice: `run` is the phase before step s0 and after the call the phase behind the
// last step taken; a' sin(phi) goes to `vals` (sum / mean) or to the result (none)
template <int DT>
AAMD_HD void osc_steps(int tid, const OscArgs& a, const OscGeom& g, int64_t row, int64_t chunk, int s0, double& run,
                       typename wa::Elem<DT>::C* vals) {
  using E = wa::Elem<DT>;
  using C = typename E::C;
  using S = typename E::S;
  const int ts = tid / a.N, n = tid - ts * a.N;
  if (ts >= g.TS) return;
  const S* f = static_cast<const S*>(a.freq) + row * a.sf;
  const S* am = static_cast<const S*>(a.amp) + row * a.sa;
  const C two_pi = (C)(2.0 * kPi), sr = (C)a.sample_rate, nyq = (C)(a.sample_rate / 2.0);
  const int64_t t0 = chunk * kOscChunk + (int64_t)ts * g.S;
  for (int sb = 0; sb < g.SB; ++sb) {
    const int s = s0 + sb;
    const int64_t t = t0 + s;
    if (!(s < g.S && ts * g.S + s < kOscChunk && t < a.T)) break;
    const C fv = E::load(f[t * a.N + n]);
    run += (double)osc_w<C>(fv, two_pi, sr);
    const C ph = (C)reduce_2pi(run);
    const C ap = d_abs(fv) >= nyq ? C(0) : E::load(am[t * a.N + n]);
    const C sn = d_sin(ph);
    if (a.reduction == kNone) static_cast<S*>(a.out)[(row * a.T + t) * a.N + n] = E::store(ap * sn);
    else {
      // the chain multiplies and adds in one operation: it gets the factors, not the product
      vals[(ts * g.SB + sb) * g.Np + n] = sn;
      vals[kOscLdsValues + (ts * g.SB + sb) * g.Np + n] = ap;
    }
  }
}

// sum / mean: lane `tid` reduces the output samples o = tid, tid + kThreads, ... of this pass
template <int DT>
AAMD_HD void osc_reduce(int tid, const OscArgs& a, const OscGeom& g, int64_t row, int64_t chunk, int s0,
                        const typename wa::Elem<DT>::C* vals) {
  using E = wa::Elem<DT>;
  using C = typename E::C;
  for (int o = tid; o < g.TS * g.SB; o += kThreads) {
    const int ts = o / g.SB, sb = o - ts * g.SB, s = s0 + sb;
    const int64_t t = chunk * kOscChunk + (int64_t)ts * g.S + s;
    if (!(s < g.S && ts * g.S + s < kOscChunk && t < a.T)) continue;
    C acc = C(0);
    for (int n = 0; n < a.N; ++n) acc = d_fma(vals[kOscLdsValues + o * g.Np + n], vals[o * g.Np + n], acc);
    if (a.reduction == kMean) acc = acc / (C)a.N;
    static_cast<typename E::S*>(a.out)[row * a.T + t] = E::store(acc);
  }
}

// ---- filter_waveform -------------------------------------------------------------------------------------------------------
struct FwArgs {
  const void *x, *h;          // x (rows, T) through sx; h (F, L) or (rows, F, L) dense
  void* out;                  // (rows, T) dense
  int64_t rows, T, sx, F, C, tiles;
  int32_t L, batched;
};

AAMD_HD size_t fw_lds_values(int L) { return (size_t)kFwTile + (size_t)L - 1; }

template <int DT>
AAMD_HD void fw_stage(int tid, const FwArgs& a, int64_t row, int64_t tile, typename wa::Elem<DT>::C* xs) {
  using E = wa::Elem<DT>;
  const typename E::S* x = static_cast<const typename E::S*>(a.x) + row * a.sx;
  const int64_t span0 = tile * kFwTile + (a.L - 1) / 2 - a.L + 1;
  const int count = kFwTile + a.L - 1;
  for (int i = tid; i < count; i += kThreads) {
    const int64_t g = span0 + i;
    xs[i] = (g >= 0 && g < a.T) ? E::load(x[g]) : typename E::C(0);
  }
}

template <int DT>
AAMD_HD void fw_outputs(int tid, const FwArgs& a, int64_t row, int64_t tile, const typename wa::Elem<DT>::C* xs) {
  using E = wa::Elem<DT>;
  using C = typename E::C;
  using S = typename E::S;
  const int d = (a.L - 1) / 2;
  const int64_t t0 = tile * kFwTile, span0 = t0 + d - a.L + 1;
  const int64_t wn0 = t0 + (int64_t)(tid & ~63) * kFwPer;             // the wave's first output
  if (wn0 >= a.T) return;
  int64_t wn1 = wn0 + 64 * kFwPer - 1;
  if (wn1 > a.T - 1) wn1 = a.T - 1;
  int64_t mlo = wn0 + d - a.L + 1, mhi = wn1 + d;
  if (mlo < 0) mlo = 0;
  if (mhi > a.T - 1) mhi = a.T - 1;
  const int64_t n0 = t0 + (int64_t)tid * kFwPer;
  const S* h = static_cast<const S*>(a.h) + (a.batched ? row * a.F * a.L : 0);
  int64_t c = mlo / a.C, cnt = mlo - c * a.C;
  C acc[kFwPer], hw[kFwPer];
  for (int r = 0; r < kFwPer; ++r) acc[r] = C(0), hw[r] = C(0);
  bool fresh = true;
  for (int64_t m = mlo; m <= mhi; ++m) {
    const int j0 = (int)(n0 + d - m);
    const S* hc = h + c * a.L;
    if (fresh) {
#if defined(__HIPCC__)
#pragma unroll
#endif
      for (int r = 0; r < kFwPer; ++r) hw[r] = (unsigned)(j0 + r) < (unsigned)a.L ? E::load(hc[j0 + r]) : C(0);
      fresh = false;
    } else {
#if defined(__HIPCC__)
#pragma unroll
#endif
      for (int r = kFwPer - 1; r > 0; --r) hw[r] = hw[r - 1];
      hw[0] = (unsigned)j0 < (unsigned)a.L ? E::load(hc[j0]) : C(0);
    }
    const C xv = xs[m - span0];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int r = 0; r < kFwPer; ++r) {
      const C nv = d_fma(xv, hw[r], acc[r]);
      acc[r] = (unsigned)(j0 + r) < (unsigned)a.L ? nv : acc[r];
    }
    if (++cnt == a.C) {
      cnt = 0;
      ++c;
      fresh = true;
    }
  }
  S* o = static_cast<S*>(a.out) + row * a.T;
  for (int r = 0; r < kFwPer; ++r)
    if (n0 + r < a.T) o[n0 + r] = E::store(acc[r]);
}

// ---- sinc_impulse_response -------------------------------------------------------------------------------------------------
struct SincArgs {
  const void* cutoff;         // (rows,)
  void* out;                  // (rows, W)
  int64_t rows;
  int32_t W, high_pass;
};

AAMD_HD double sinc_g(double cut, int i, int half, int W) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double x = cut * (double)i;
  const double px = kPi * x;
  const double s = px == 0.0 ? 1.0 : sin(px) / px;
  const double win = W == 1 ? 1.0 : 0.54 - 0.46 * cos(2.0 * kPi * (double)(i + half) / (double)(W - 1));
  return s * win;
}

template <int DT>
AAMD_HD double sinc_cut(const SincArgs& a, int64_t row) {
  return DT == wa::kF64 ? static_cast<const double*>(a.cutoff)[row] : (double)static_cast<const float*>(a.cutoff)[row];
}

// s + c += v with the rounding error of the addition kept in c (Neumaier): the taps of a filter at the Nyquist cutoff are
// rounding noise beside the centre tap, and the high-pass centre 1 - g / |sum g| shows whatever the sum loses
AAMD_HD void add_kept(double& s, double& c, double v) {
  const double t = s + v;
  c += fabs(s) >= fabs(v) ? (s - t) + v : (v - t) + s;
  s = t;
}

// lane `tid`'s taps k = tid, tid + kThreads, ...: part[tid] and part[kThreads + tid] are their sum and what it lost
template <int DT>
AAMD_HD void sinc_partial(int tid, const SincArgs& a, int64_t row, double* part) {
  const int half = a.W / 2;
  const double cut = sinc_cut<DT>(a, row);
  double p = 0.0, c = 0.0;
  for (int k = tid; k < a.W; k += kThreads) add_kept(p, c, sinc_g(cut, k - half, half, a.W));
  part[tid] = p;
  part[kThreads + tid] = c;
}

template <int DT>
AAMD_HD void sinc_write(int tid, const SincArgs& a, int64_t row, const double* part) {
  const int half = a.W / 2;
  const double cut = sinc_cut<DT>(a, row);
  double sum = 0.0, lost = 0.0;
  for (int q = 0; q < kThreads; ++q) {
    add_kept(sum, lost, part[q]);
    lost += part[kThreads + q];
  }
  sum = fabs(sum + lost);
  for (int k = tid; k < a.W; k += kThreads) {
    double v = sinc_g(cut, k - half, half, a.W) / sum;
    if (a.high_pass) {
      v = -v;
      if (k == half) v = v + 1.0;
    }
    if (DT == wa::kF64) static_cast<double*>(a.out)[row * a.W + k] = v;
    else static_cast<float*>(a.out)[row * a.W + k] = (float)v;
  }
}

// ---- frequency_impulse_response --------------------------------------------------------------------------------------------
struct FirArgs {
  const void *mags, *table;   // (rows, n) dense; cos(2 pi q / N), q < N, in the element type
  void* out;                  // (rows, N)
  int64_t rows;
  int32_t n;
};

template <int DT>
AAMD_HD void fir_stage(int tid, const FirArgs& a, int64_t row, typename wa::Elem<DT>::C* lds) {
  using C = typename wa::Elem<DT>::C;
  const int N = 2 * (a.n - 1);
  const C* m = static_cast<const C*>(a.mags) + row * a.n;
  const C* tab = static_cast<const C*>(a.table);
  for (int j = tid; j < a.n; j += kThreads) lds[j] = (j == 0 || j == a.n - 1) ? m[j] : C(2) * m[j];
  for (int q = tid; q < N; q += kThreads) lds[a.n + q] = tab[q];
}

template <int DT>
AAMD_HD void fir_write(int tid, const FirArgs& a, int64_t row, const typename wa::Elem<DT>::C* lds) {
  using C = typename wa::Elem<DT>::C;
  const int N = 2 * (a.n - 1);
  const C* tab = lds + a.n;
  for (int i = tid; i < N; i += kThreads) {
    const int k = (i + N / 2) % N;
    C acc = C(0);
    int idx = 0;
    for (int j = 0; j < a.n; ++j) {
      acc = d_fma(lds[j], tab[idx], acc);
      idx += k;
      if (idx >= N) idx -= N;
    }
    const C ir = acc / (C)N;
    const C win = (C)(0.5 * (1.0 - cos(2.0 * kPi * (double)i / (double)(N - 1))));
    static_cast<C*>(a.out)[row * N + i] = ir * win;
  }
}

// ---- extend_pitch ----------------------------------------------------------------------------------------------------------
struct PitchArgs {
  const void *base, *pattern; // (M,), (N,)
  void* out;                  // (M, N)
  int64_t M, N;
};

template <int DT>
AAMD_HD void pitch_one(const PitchArgs& a, int64_t i) {
  using E = wa::Elem<DT>;
  if (i >= a.M * a.N) return;
  const int64_t m = i / a.N, n = i - m * a.N;
  const typename E::C v = E::load(static_cast<const typename E::S*>(a.base)[m]) * E::load(static_cast<const typename E::S*>(a.pattern)[n]);
  static_cast<typename E::S*>(a.out)[i] = E::store(v);
}

#if defined(__HIPCC__)
template <int DT>
__global__ __launch_bounds__(kThreads) void osc_sums_kernel(OscArgs a) {
  __shared__ double sub[kThreads];
  const OscGeom g = osc_geom(a.N);
  const int64_t row = (int64_t)blockIdx.x / (a.chunks - 1), chunk = (int64_t)blockIdx.x - row * (a.chunks - 1);
  sub[threadIdx.x] = osc_slice_sum<DT>(threadIdx.x, a, g, row, chunk);
  __syncthreads();
  osc_chunk_sum(threadIdx.x, a, g, row, chunk, sub);
}

template <int DT>
__global__ __launch_bounds__(kThreads) void osc_apply_kernel(OscArgs a) {
  using C = typename wa::Elem<DT>::C;
  __shared__ double sub[kThreads], start[kThreads];
  __shared__ C vals[2 * kOscLdsValues];
  const OscGeom g = osc_geom(a.N);
  const int tid = threadIdx.x;
  const int64_t row = (int64_t)blockIdx.x / a.chunks, chunk = (int64_t)blockIdx.x - row * a.chunks;
  sub[tid] = osc_slice_sum<DT>(tid, a, g, row, chunk);
  osc_start(tid, a, row, chunk, start);
  __syncthreads();
  double run = osc_base(tid, a, g, start, sub);
  for (int s0 = 0; s0 < g.S; s0 += g.SB) {
    osc_steps<DT>(tid, a, g, row, chunk, s0, run, vals);
    if (a.reduction != kNone) {
      __syncthreads();
      osc_reduce<DT>(tid, a, g, row, chunk, s0, vals);
      __syncthreads();
    }
  }
}

template <int DT>
__global__ __launch_bounds__(kThreads) void fw_kernel(FwArgs a) {
  using C = typename wa::Elem<DT>::C;
  extern __shared__ __align__(16) unsigned char fw_smem[];
  C* xs = reinterpret_cast<C*>(fw_smem);
  const int64_t row = (int64_t)blockIdx.x / a.tiles, tile = (int64_t)blockIdx.x - row * a.tiles;
  fw_stage<DT>(threadIdx.x, a, row, tile, xs);
  __syncthreads();
  fw_outputs<DT>(threadIdx.x, a, row, tile, xs);
}

template <int DT>
__global__ __launch_bounds__(kThreads) void sinc_kernel(SincArgs a) {
  __shared__ double part[2 * kThreads];
  sinc_partial<DT>(threadIdx.x, a, blockIdx.x, part);
  __syncthreads();
  sinc_write<DT>(threadIdx.x, a, blockIdx.x, part);
}

template <int DT>
__global__ __launch_bounds__(kThreads) void fir_kernel(FirArgs a) {
  using C = typename wa::Elem<DT>::C;
  extern __shared__ __align__(16) unsigned char fir_smem[];
  C* lds = reinterpret_cast<C*>(fir_smem);
  fir_stage<DT>(threadIdx.x, a, blockIdx.x, lds);
  __syncthreads();
  fir_write<DT>(threadIdx.x, a, blockIdx.x, lds);
}

template <int DT>
__global__ __launch_bounds__(kThreads) void pitch_kernel(PitchArgs a) {
  pitch_one<DT>(a, (int64_t)blockIdx.x * kThreads + threadIdx.x);
}
#endif

}  // namespace dsp
}  // namespace aamd
