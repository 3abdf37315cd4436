// Spectral centroid (F.spectral_centroid / T.SpectralCentroid): the reduction over frequency that follows the magnitude
// spectrogram,  out[r][t] = sum_k freqs[k] m[r][t][k] / sum_k m[r][t][k].
//
// The reference multiplies the spectrogram by a broadcast frequency column, sums twice and divides: four passes over the
// spectrogram and two temporaries of its size.  Here it is one read of the float32 magnitudes and one write per frame.
//
// Frame-major memory (unit stride along frequency -- what every STFT kernel of this library writes): a frame's line is cut
// into 16-byte vectors at multiples of 16 bytes of the ADDRESS, P lanes share the line (P = the power of two that leaves a
// lane about four vectors, at most 64: n_freq = 33 puts sixteen frames on a wave, 201 four, n_freq > 512 one), lane l takes
// the vectors l, l + P, ...  A whole vector is one 16-byte load; the partial vectors at the two ends of a line that does not start or
// end on a 16-byte boundary are read element by element, so nothing outside the line is touched.  Any other strides (the
// time-contiguous layout among them): one lane per frame walks the bins through the strides, neighbouring lanes read
// neighbouring frames.
//
// Numerator and denominator are float64: a product of two float32 values is exact there, each lane adds its bins in
// ascending order, the lanes of a frame combine in one fixed tree (lane l += lane l + s for s = P / 2 .. 1), then one
// float64 division and one rounding to the output type.  No atomics: two calls give the same bits.  (The order of the
// additions depends on the line's address modulo 16 bytes, and on nothing else.)  A frame of zeros gives 0 / 0 = NaN, as
// the reference does; a NaN stays in its frame.
//
// The phase functions are AAMD_HD: tests/cpu_sim/sim_spectral_point.cpp replays them with g++.
#pragma once
#include "hd.h"
#include "wave_augment.h"   // wa::Elem

namespace aamd {
namespace sf {

constexpr int kThreads = 256;
constexpr int kVec = 4;         // float32 values per 16-byte vector
constexpr int kMaxLanes = 64;   // lanes that share a frame line: at most one wave
constexpr int kUnroll = 4;      // vectors per lane whose loads are issued together

struct CentArgs {
  const float* m;               // magnitudes, (rows, frames, n_freq) through sr / st / sk
  const float* freqs;           // [n_freq], 16-byte aligned
  void* out;                    // dense (rows, frames) of the output type
  int64_t rows, frames, n_freq;
  int64_t sr, st, sk;           // element strides
  int32_t lanes;                // P: lanes per frame; 1 on the strided path
};

// lanes that share a frame line of n_freq bins: about kUnroll vectors per lane
AAMD_HD int32_t lanes_for(int64_t n_freq) {
  const int64_t vecs = (n_freq + kVec - 1) / kVec, want = (vecs + kUnroll - 1) / kUnroll;
  int32_t p = 1;
  while (p < kMaxLanes && p < want) p <<= 1;
  return p;
}

// Vector j of a line that starts `mis` elements past a 16-byte boundary: bins [4 j - mis, 4 j - mis + 4) and their
// frequencies; what lies outside the line comes back as +0, which changes neither sum.
AAMD_HD void load_vector(const CentArgs& a, const float* line, int64_t mis, int64_t j, float m[kVec], float f[kVec]) {
  const int64_t k0 = j * kVec - mis;
  if (k0 >= 0 && k0 + kVec <= a.n_freq) {
    const F4 v = *reinterpret_cast<const F4*>(line + k0);
    m[0] = v.x; m[1] = v.y; m[2] = v.z; m[3] = v.w;
    if (mis == 0) {
      const F4 g = *reinterpret_cast<const F4*>(a.freqs + k0);
      f[0] = g.x; f[1] = g.y; f[2] = g.z; f[3] = g.w;
    } else {
#pragma unroll
      for (int e = 0; e < kVec; ++e) f[e] = a.freqs[k0 + e];
    }
    return;
  }
#pragma unroll
  for (int e = 0; e < kVec; ++e) {
    const bool in = j >= 0 && k0 + e >= 0 && k0 + e < a.n_freq;
    m[e] = in ? line[k0 + e] : 0.0f;
    f[e] = in ? a.freqs[k0 + e] : 0.0f;
  }
}

// Frame-major: lane `lane` of the P that share frame q (= row * frames + t).  The loads of kUnroll vectors are issued
// together; the additions run in ascending order of the bins.
AAMD_HD void lane_partial(const CentArgs& a, int64_t q, int lane, double& num, double& den) {
  num = 0.0;
  den = 0.0;
  if (q >= a.rows * a.frames) return;
  const int64_t row = q / a.frames, t = q - row * a.frames;
  const float* line = a.m + row * a.sr + t * a.st;
  const int64_t mis = (int64_t)(((uintptr_t)line >> 2) & 3);     // elements between the 16-byte boundary below and the line
  const int64_t n_vec = (a.n_freq + mis + kVec - 1) / kVec;
  for (int64_t j0 = lane; j0 < n_vec; j0 += (int64_t)kUnroll * a.lanes) {
    float m[kUnroll][kVec], f[kUnroll][kVec];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int64_t j = j0 + (int64_t)u * a.lanes;
      load_vector(a, line, mis, j < n_vec ? j : -1, m[u], f[u]);
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u)
#pragma unroll
      for (int e = 0; e < kVec; ++e) {
        num += (double)f[u][e] * (double)m[u][e];
        den += (double)m[u][e];
      }
  }
}

// Any strides: the one lane of frame q.
AAMD_HD void frame_strided(const CentArgs& a, int64_t q, double& num, double& den) {
  num = 0.0;
  den = 0.0;
  if (q >= a.rows * a.frames) return;
  const int64_t row = q / a.frames, t = q - row * a.frames;
  const float* p = a.m + row * a.sr + t * a.st;
  for (int64_t k = 0; k < a.n_freq; ++k) {
    const float m = p[k * a.sk];
    num += (double)a.freqs[k] * (double)m;
    den += (double)m;
  }
}

// One step of the tree over the P lanes of a frame (s: the lanes' sums, `lane` the index within the frame).
AAMD_HD void tree_step(double* num, double* den, int lane, int stride) {
  if (lane < stride) {
    num[lane] += num[lane + stride];
    den[lane] += den[lane + stride];
  }
}

template <int DT>
AAMD_HD void store_result(const CentArgs& a, int64_t q, double num, double den) {
  using E = wa::Elem<DT>;
  static_cast<typename E::S*>(a.out)[q] = E::store((typename E::C)(num / den));
}

#if defined(__HIPCC__)
template <int DT, bool LINES>
__global__ __launch_bounds__(kThreads) void centroid_kernel(CentArgs a) {
  const int tid = threadIdx.x;
  if (!LINES) {
    const int64_t q = (int64_t)blockIdx.x * kThreads + tid;
    double num, den;
    frame_strided(a, q, num, den);
    if (q < a.rows * a.frames) store_result<DT>(a, q, num, den);
    return;
  }
  const int P = a.lanes, per_block = kThreads / P;
  const int lane = tid & (P - 1);
  const int64_t q = (int64_t)blockIdx.x * per_block + tid / P;
  double num, den;
  lane_partial(a, q, lane, num, den);
  for (int s = P >> 1; s > 0; s >>= 1) {                          // every lane takes part; lane < s holds the tree's value
    num += __shfl_down(num, s, kMaxLanes);
    den += __shfl_down(den, s, kMaxLanes);
  }
  if (lane == 0 && q < a.rows * a.frames) store_result<DT>(a, q, num, den);
}
#endif

}  // namespace sf
}  // namespace aamd
