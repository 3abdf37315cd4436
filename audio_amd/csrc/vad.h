// Voice-activity trimming (F.vad, F.vad_start, T.Vad): SoX's vad effect, whose reference walks the signal in a Python loop
// with two FFTs, a read-back and a ring scan per measurement and channel.
//
// A measurement every P samples of every row: the magnitude spectrum of the last L samples (Hann window, N-point FFT, bins
// [s0, s1)), smoothed over frames and reduced by a tracked noise floor (two first-order recurrences per bin), then the
// power of the cepstrum (an N/2-point FFT of the windowed, noise-reduced spectrum) in [c0, c1) on a log scale.  The trigger
// is a float64 first-order mean of the measurements and, at the frame where it crosses the level, a scan back over the last
// M measurements.  Four launches (five with the joint start of F.vad):
//   spec_kernel      one workgroup per (row, frame): window the L samples into LDS in bit-reversed order, radix-2 in LDS,
//                    |X[k]| of the bins [s0, s1) to the workspace d[row][frame][bin].  Frame-parallel.
//   smooth_kernel    one thread per (row, bin), consecutive threads consecutive bins: walks the frames in order with the
//                    smoothed spectrum and the noise floor in registers and overwrites d with e * cw.  Every product that
//                    the reference rounds on its own is rounded on its own here (wa::rounded).
//   ceps_kernel      one workgroup per (row, frame): the N/2-point FFT of that row of d in LDS, the band sum as a strided
//                    partial per thread and a tree over the threads (no atomics: two calls give the same bits), the log
//                    in float64 by thread 0.
//   trigger_kernel   one lane per row: the float64 mean until it crosses, then the ring scan (offsets come from the frame
//                    and ring counters only, never from a data value).
//   joint_kernel     one workgroup: the least (first frame, row) over the rows, then the largest flush of the rows from
//                    that row on: the common start of F.vad.
// Both FFTs are complex radix-2 with the imaginary part zero, on split re / im planes whose index is skewed by one word
// per 32 and per 1024 (pidx): the bit-reversed stores of consecutive samples, N / 32 words apart, then fall on 32 different
// banks for every N from 1024 to 8192, and the butterflies keep unit stride.  Twiddles come from a host-built table of
// exp(-2 pi i k / N), k < N / 2 (float64 rounded once); the half-size transform reads every second entry.
//
// The phase functions are AAMD_HD: tests/cpu_sim/sim_vad.cpp replays them with g++.
#pragma once
#include <math.h>

#include "wave_augment.h"

namespace aamd {
namespace vad {

using wa::Elem;
using wa::rounded;

constexpr int kThreads = 256;             // per workgroup of spec_kernel, smooth_kernel, ceps_kernel and joint_kernel
constexpr int kTrigThreads = 64;          // rows (= lanes) per workgroup of trigger_kernel
constexpr int kMinN = 16;
constexpr int kMaxN = 8192;               // the defaults up to 81.9 kHz; both planes of it take 66 KiB of LDS

struct MeasArgs {
  const void* x;                // (rows, T) through sx
  const float* w;               // [L]  the measurement window
  const float* cw;              // [s1 - s0]  the cepstrum window
  const float* tw;              // [N / 2][2]  (cos, -sin)(2 pi k / N)
  float* d;                     // workspace (rows, frames, s1 - s0)
  float* meas;                  // (rows, frames)
  int64_t rows, T, sx, frames;
  double smooth;                // measure_smooth_time's multiplier
  float up, down, nra;          // the noise floor's two multipliers, noise_reduction_amount
  int32_t L, N, logN, P, s0, s1, c0, c1, boot_max;
};

struct TrigArgs {
  const float* meas;            // (rows, frames)
  int64_t rows, frames, M, gap, P, fixed;
  double level, trig;
  int64_t *first, *start, *joint;
};

// frames f = 0, 1, ... while L + f P < T
AAMD_HD int64_t n_frames(int64_t T, int64_t L, int64_t P) { return T <= L ? 0 : (T - L - 1) / P + 1; }

AAMD_HD int pidx(int p) { return p + (p >> 5) + (p >> 10); }
AAMD_HD int plane(int n) { return pidx(n - 1) + 1; }           // words of one plane of an n-point transform
AAMD_HD size_t lds_bytes(int n) { return (size_t)2 * plane(n) * sizeof(float); }

AAMD_HD uint32_t bitrev(uint32_t v, int bits) {
  v = ((v >> 1) & 0x55555555u) | ((v & 0x55555555u) << 1);
  v = ((v >> 2) & 0x33333333u) | ((v & 0x33333333u) << 2);
  v = ((v >> 4) & 0x0f0f0f0fu) | ((v & 0x0f0f0f0fu) << 4);
  v = ((v >> 8) & 0x00ff00ffu) | ((v & 0x00ff00ffu) << 8);
  v = (v >> 16) | (v << 16);
  return v >> (32 - bits);
}

template <int DT>
AAMD_HD float sample(const void* x, int64_t i) {       // float64 is rounded, the half types are widened
  using E = Elem<DT>;
  return (float)E::load(static_cast<const typename E::S*>(x)[i]);
}

// ---- the transforms ---------------------------------------------------------------------------------------------------------
// Stage s (0-based) of an n-point decimation-in-time transform over bit-reversed input; `log_table` is log2 of the size the
// twiddle table was built for (n or 2 n).
AAMD_HD void fft_stage(int tid, int n, int s, const float* tw, int log_table, float* re, float* im) {
  const int half = 1 << s;
  for (int j = tid; j < (n >> 1); j += kThreads) {
    const int pos = j & (half - 1);
    const int i0 = pidx(((j >> s) << (s + 1)) + pos), i1 = pidx(((j >> s) << (s + 1)) + pos + half);
    const int t = pos << (log_table - 1 - s);
    const float wr = tw[2 * t], wi = tw[2 * t + 1];
    const float xr = re[i1], xi = im[i1], ur = re[i0], ui = im[i0];
    const float tr = xr * wr - xi * wi, ti = xr * wi + xi * wr;
    re[i0] = ur + tr; im[i0] = ui + ti;
    re[i1] = ur - tr; im[i1] = ui - ti;
  }
}

// the L samples that end at L + f P, windowed and zero-padded to N, in bit-reversed order
template <int DT>
AAMD_HD void frame_load(int tid, const MeasArgs& a, int64_t row, int64_t f, float* re, float* im) {
  const int64_t base = row * a.sx + f * a.P;
  for (int i = tid; i < a.N; i += kThreads) {
    const float v = i < a.L ? sample<DT>(a.x, base + i) * a.w[i] : 0.0f;
    const int j = pidx((int)bitrev((uint32_t)i, a.logN));
    re[j] = v;
    im[j] = 0.0f;
  }
}

AAMD_HD void spec_write(int tid, const MeasArgs& a, int64_t row, int64_t f, const float* re, const float* im) {
  const int nb = a.s1 - a.s0;
  float* d = a.d + (row * a.frames + f) * nb;
  for (int k = tid; k < nb; k += kThreads) {
    const float r = re[pidx(a.s0 + k)], i = im[pidx(a.s0 + k)];
    d[k] = sqrt(r * r + i * i);
  }
}

// ---- the two recurrences over frames of one (row, bin) ------------------------------------------------------------------------
AAMD_HD void smooth_thread(const MeasArgs& a, int64_t row, int k) {
  const int nb = a.s1 - a.s0;
  float* d = a.d + row * a.frames * nb + k;
  const float cw = a.cw[k];
  float spec = 0.0f, noise = 0.0f;
  for (int64_t f = 0; f < a.frames; ++f) {
    const bool boot = f <= a.boot_max;
    const double md = boot ? (double)f / (1.0 + (double)f) : a.smooth;
    const float mult = (float)md, om = (float)(1.0 - md);
    const float dd = d[f * nb];
    spec = rounded(spec * mult) + rounded(dd * om);
    const float d2 = rounded(spec * spec);
    const float m = boot ? 0.0f : (d2 > noise ? a.up : a.down);
    noise = rounded(noise * m) + rounded(d2 * rounded(1.0f - m));
    const float v = d2 - rounded(a.nra * noise);
    d[f * nb] = sqrt(v < 0.0f ? 0.0f : v) * cw;          // a NaN stays a NaN
  }
}

// ---- the cepstral power ---------------------------------------------------------------------------------------------------
AAMD_HD void ceps_load(int tid, const MeasArgs& a, int64_t row, int64_t f, float* re, float* im) {
  const int nb = a.s1 - a.s0, n2 = a.N >> 1;
  const float* d = a.d + (row * a.frames + f) * nb;
  for (int i = tid; i < n2; i += kThreads) {
    const float v = (i >= a.s0 && i < a.s1) ? d[i - a.s0] : 0.0f;
    const int j = pidx((int)bitrev((uint32_t)i, a.logN - 1));
    re[j] = v;
    im[j] = 0.0f;
  }
}

AAMD_HD float ceps_partial(int tid, const MeasArgs& a, const float* re, const float* im) {
  float acc = 0.0f;
  for (int k = a.c0 + tid; k < a.c1; k += kThreads) {
    const float r = re[pidx(k)], i = im[pidx(k)];
    acc += r * r + i * i;
  }
  return acc;
}

AAMD_HD void sum_step(int tid, int stride, float* s) {
  if (tid < stride) s[tid] += s[tid + stride];
}

// max(0, 21 + log(pw / n)) in float64 from the float32 power, rounded once; 0 unless pw > 0 (a NaN measures 0)
AAMD_HD float measure_of(float pw, int n) {
  if (!(pw > 0.0f)) return 0.0f;
  const double v = 21.0 + log((double)pw / (double)n);
  return (float)(v > 0.0 ? v : 0.0);
}

// ---- the trigger ------------------------------------------------------------------------------------------------------------
AAMD_HD int64_t first_of(const TrigArgs& a, int64_t row) {
  const float* m = a.meas + row * a.frames;
  const double omt = 1.0 - a.trig;
  double mean = 0.0;
  for (int64_t f = 0; f < a.frames; ++f) {
    mean = rounded(mean * a.trig) + rounded((double)m[f] * omt);
    if (mean >= a.level) return f;
  }
  return -1;
}

// how many measurements before frame f the kept part starts: the scan back over the ring of the last M measurements
AAMD_HD int64_t flush_at(const TrigArgs& a, int64_t row, int64_t f) {
  const float* m = a.meas + row * a.frames;
  int64_t jT = a.M, jZ = a.M;
  for (int64_t j = 0; j < a.M; ++j) {
    const double v = f - j >= 0 ? (double)m[f - j] : 0.0;
    if (v >= a.level && j <= jT + a.gap) jZ = jT = j;
    else if (v == 0.0 && jT >= jZ) jZ = j;
  }
  return jZ < a.M - 1 ? jZ : a.M - 1;
}

AAMD_HD int64_t start_of(const TrigArgs& a, int64_t f, int64_t flush) {
  const int64_t s = (f - flush) * a.P - a.fixed;
  return s > 0 ? s : 0;
}

AAMD_HD void trigger_row(const TrigArgs& a, int64_t row) {
  const int64_t f = first_of(a, row);
  a.first[row] = f;
  a.start[row] = f < 0 ? -1 : start_of(a, f, flush_at(a, row, f));
}

constexpr int64_t kNone = INT64_MAX;

// the least (first, row) of the rows tid, tid + kThreads, ...
AAMD_HD void joint_scan(int tid, const TrigArgs& a, int64_t& bf, int64_t& br) {
  bf = br = kNone;
  for (int64_t r = tid; r < a.rows; r += kThreads) {
    const int64_t f = a.first[r];
    if (f >= 0 && f < bf) { bf = f; br = r; }
  }
}
AAMD_HD void joint_min_step(int tid, int stride, int64_t* sf, int64_t* sr) {
  if (tid < stride) {
    const int64_t f = sf[tid + stride], r = sr[tid + stride];
    if (f < sf[tid] || (f == sf[tid] && r < sr[tid])) { sf[tid] = f; sr[tid] = r; }
  }
}
AAMD_HD int64_t joint_flush(int tid, const TrigArgs& a, int64_t f, int64_t r0) {
  int64_t mx = 0;
  for (int64_t r = r0 + tid; r < a.rows; r += kThreads) {
    const int64_t v = flush_at(a, r, f);
    mx = v > mx ? v : mx;
  }
  return mx;
}
AAMD_HD void joint_max_step(int tid, int stride, int64_t* s) {
  if (tid < stride && s[tid + stride] > s[tid]) s[tid] = s[tid + stride];
}

#if defined(__HIPCC__)
template <int DT>
__global__ __launch_bounds__(kThreads) void spec_kernel(MeasArgs a) {
  extern __shared__ __align__(16) float vad_smem[];
  float* re = vad_smem;
  float* im = vad_smem + plane(a.N);
  const int64_t row = (int64_t)blockIdx.x / a.frames, f = (int64_t)blockIdx.x - row * a.frames;
  const int tid = threadIdx.x;
  frame_load<DT>(tid, a, row, f, re, im);
  __syncthreads();
  for (int s = 0; s < a.logN; ++s) {
    fft_stage(tid, a.N, s, a.tw, a.logN, re, im);
    __syncthreads();
  }
  spec_write(tid, a, row, f, re, im);
}

__global__ __launch_bounds__(kThreads) void smooth_kernel(MeasArgs a) {
  const int nb = a.s1 - a.s0;
  const int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (q >= a.rows * nb) return;
  const int64_t row = q / nb;
  smooth_thread(a, row, (int)(q - row * nb));
}

__global__ __launch_bounds__(kThreads) void ceps_kernel(MeasArgs a) {
  extern __shared__ __align__(16) float vad_smem[];
  __shared__ float red[kThreads];
  const int n2 = a.N >> 1;
  float* re = vad_smem;
  float* im = vad_smem + plane(n2);
  const int64_t row = (int64_t)blockIdx.x / a.frames, f = (int64_t)blockIdx.x - row * a.frames;
  const int tid = threadIdx.x;
  ceps_load(tid, a, row, f, re, im);
  __syncthreads();
  for (int s = 0; s < a.logN - 1; ++s) {
    fft_stage(tid, n2, s, a.tw, a.logN, re, im);
    __syncthreads();
  }
  red[tid] = ceps_partial(tid, a, re, im);
  __syncthreads();
  for (int stride = kThreads >> 1; stride > 0; stride >>= 1) {
    sum_step(tid, stride, red);
    __syncthreads();
  }
  if (tid == 0) a.meas[row * a.frames + f] = measure_of(red[0], a.c1 - a.c0);
}

__global__ __launch_bounds__(kTrigThreads) void trigger_kernel(TrigArgs a) {
  const int64_t row = (int64_t)blockIdx.x * kTrigThreads + threadIdx.x;
  if (row < a.rows) trigger_row(a, row);
}

__global__ __launch_bounds__(kThreads) void joint_kernel(TrigArgs a) {
  __shared__ int64_t sf[kThreads], sr[kThreads];
  const int tid = threadIdx.x;
  joint_scan(tid, a, sf[tid], sr[tid]);
  __syncthreads();
  for (int stride = kThreads >> 1; stride > 0; stride >>= 1) {
    joint_min_step(tid, stride, sf, sr);
    __syncthreads();
  }
  const int64_t f = sf[0], r0 = sr[0];
  __syncthreads();
  if (f == kNone) {
    if (tid == 0) a.joint[0] = -1;
    return;
  }
  sf[tid] = joint_flush(tid, a, f, r0);
  __syncthreads();
  for (int stride = kThreads >> 1; stride > 0; stride >>= 1) {
    joint_max_step(tid, stride, sf);
    __syncthreads();
  }
  if (tid == 0) a.joint[0] = start_of(a, f, sf[0]);
}
#endif

}  // namespace vad
}  // namespace aamd
