// Energy histograms of shoebox rooms by ray tracing (F.ray_tracing, F.ray_tracing_batch), whose reference is a CPU-only loop
// over the rays of one room.  The definition is the docstring of F.ray_tracing (tests/ray_oracle.py restates it): ray i of N
// leaves the source in direction i of a Fibonacci sphere (a regular fan in 2-D) with E0 = 2 / N in every band, and per bounce
//   1. finds the next wall,  2. adds tr / (r2 p_hit) to hist[m][band][floor(d / w_bin)] for every microphone whose sphere of
//   radius R the segment crosses,  3. moves to the wall and loses the absorbed part,  4. adds the scattered share a
//   microphone sees from the wall point,  5. loses the scattered part and ends past S_max or below energy_thres,  6. reflects.
// Two launches:
//   trace_kernel    one ray per lane; a workgroup of kThreads takes consecutive rays of one room (block = room * blocks per
//                   room + run of rays).  The room, the source, the microphones and the coefficients sit in LDS (struct Room);
//                   the lanes check them item by item (room_bad_part, one barrier-wide OR) and a bad room is left untouched.
//                   The bounce loop runs at most K = sum_d (floor(S_max / room_d) + 2) <= kMaxBounces times whatever the
//                   data: along axis d a path of length S meets the walls at most floor(S / room_d) + 1 times and the loop
//                   ends at the first step past S_max.  A room whose K exceeds the cap is bad.  Position, direction and the
//                   per-band energies stay in registers: every loop over axes and bands has a compile-time count (D and the
//                   band class NBC of 1, 4 or 8 are template arguments) and the hit axis selects by comparison, never by
//                   index.  A bin is compared with [0, bins) as a double before it becomes an integer.
//                   Sums are fixed point: a contribution e becomes q = rint(e 2^k) and is added to an int64 accumulator of
//                   the result's shape with a 64-bit integer atomic.  Integer addition commutes, so no arrival order can
//                   change a bit.  k = 62 - ceil(log2(8 kHeadroom / R^2)) comes from the host: e <= 4 E0 / R^2, so a
//                   (microphone, bin) that takes up to kHeadroom contributions of EVERY ray stays below 2^62.
//   convert_kernel  out = acc 2^-k in the element type, NaN for a negative (wrapped) accumulator and for every element of a
//                   bad room, whose validity it forms again from the same inputs.
// The phase functions are AAMD_HD: tests/cpu_sim/sim_ray.cpp replays them with g++.
#pragma once
#include <math.h>

#include "hd.h"

namespace aamd {
namespace ray {

constexpr int kThreads = 256;                  // rays per workgroup
constexpr int kMaxBands = 8;
constexpr int kMaxMics = 16;
constexpr int kMaxRays = 1 << 24;
constexpr int kMaxBins = 65536;
constexpr int kMaxBounces = 4096;              // the defaults in a 6 x 5 x 3 m room need 2406
constexpr int kHeadroom = 64;                  // contributions of every ray one (microphone, bin) may take: see the scale
constexpr int kF32 = 0, kF64 = 1;              // AAMD_SA_F32 / AAMD_SA_F64
constexpr double kPi = 3.14159265358979323846;
constexpr double kGolden = kPi * (3.0 - 2.23606797749979);     // pi (3 - sqrt 5), folded in float64
constexpr long long kSaturated = -0x7fffffffffffffffll - 1;     // what a contribution beyond int64 becomes: a negative sum

struct Args {
  const void *room, *source, *mic;             // (B, D), (B, D), (B, M, D) dense, of the element type
  const void *absorption, *scattering;         // (B, NB, 2 D) dense each
  long long* acc;                              // (B, M, NB, bins) dense, zero on entry
  void* out;                                   // (B, M, NB, bins) dense
  int64_t B, N, bins, blocks_per_room;
  double e0, s_max, r2, w_bin, energy_thres, scale;   // 2 / N, time_thres sound_speed, R^2, sound_speed hist_bin_size, -, 2^k
  int32_t D, M, NB, k;
};

struct Room {                                  // LDS of a workgroup; every entry beyond D, M, NB is unused
  double room[3], source[3];
  double mic[kMaxMics * 3];
  double ab[kMaxBands * 6], sc[kMaxBands * 6]; // [band][wall], wall = 2 axis + (upper wall)
};

template <int DT>
AAMD_HD double ld(const void* p, int64_t i) {
  return DT == kF64 ? static_cast<const double*>(p)[i] : (double)static_cast<const float*>(p)[i];
}

AAMD_HD bool finite_(double v) { return fabs(v) <= 1.7976931348623157e308; }      // false for NaN

AAMD_HD int band_class(int nb) { return nb == 1 ? 1 : (nb <= 4 ? 4 : 8); }

// lane `tid` copies its items of room b (strided, so any thread count fills the struct)
template <int DT>
AAMD_HD void load_room(int tid, int threads, const Args& a, int64_t b, Room& rm) {
  const int D = a.D, nm = a.M * D, nc = a.NB * 2 * D;
  for (int i = tid; i < D; i += threads) {
    rm.room[i] = ld<DT>(a.room, b * D + i);
    rm.source[i] = ld<DT>(a.source, b * D + i);
  }
  for (int i = tid; i < nm; i += threads) rm.mic[i] = ld<DT>(a.mic, b * nm + i);
  for (int i = tid; i < nc; i += threads) {
    rm.ab[i] = ld<DT>(a.absorption, b * nc + i);
    rm.sc[i] = ld<DT>(a.scattering, b * nc + i);
  }
}

// K = sum_d (floor(S_max / room_d) + 2) as a double (it may be huge, infinite or NaN: compare before converting)
AAMD_HD double bounce_bound(const Args& a, const Room& rm) {
  double k = 0.0;
  for (int d = 0; d < a.D; ++d) k += floor(a.s_max / rm.room[d]) + 2.0;
  return k;
}

// lane `tid`'s share of the room's checks; the room is bad if any lane says so
AAMD_HD bool room_bad_part(int tid, int threads, const Args& a, const Room& rm) {
  const int D = a.D, nm = a.M * D, nc = a.NB * 2 * D;
  bool bad = false;
  for (int i = tid; i < D; i += threads) {
    const double r = rm.room[i], s = rm.source[i];
    bad = bad || !(finite_(r) && r > 0.0) || !(s > 0.0 && s < r);
  }
  for (int i = tid; i < nm; i += threads) {
    const double r = rm.room[i % D], p = rm.mic[i];
    bad = bad || !(p > 0.0 && p < r);
  }
  for (int i = tid; i < nc; i += threads)
    bad = bad || !(rm.ab[i] >= 0.0 && rm.ab[i] <= 1.0) || !(rm.sc[i] >= 0.0 && rm.sc[i] <= 1.0);
  if (tid == 0) bad = bad || !(bounce_bound(a, rm) <= (double)kMaxBounces);
  return bad;
}

// ---- the phases of a ray -----------------------------------------------------------------------------------------------------
// every product and sum below is rounded on its own (no contraction): the float64 value of the definition read left to right

template <int D>
AAMD_HD void direction(int64_t i, int64_t n, double* dir) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (D == 3) {
    const double z = 1.0 - (double)(2 * i + 1) / (double)n;
    const double rho = sqrt(1.0 - z * z);
    const double phi = (double)i * kGolden;
    dir[0] = rho * cos(phi);
    dir[1] = rho * sin(phi);
    dir[D - 1] = z;
  } else {
    const double phi = (2.0 * kPi) * ((double)i + 0.5) / (double)n;
    dir[0] = cos(phi);
    dir[1] = sin(phi);
  }
}

// the distance t to the next wall and its axis: the first axis that attains the minimum
template <int D>
AAMD_HD void next_wall(const double* p, const double* dir, const Room& rm, double& t, int& axis) {
  t = INFINITY;
  axis = 0;
#pragma unroll
  for (int d = 0; d < D; ++d) {
    double td = INFINITY;
    if (dir[d] > 0.0) td = (rm.room[d] - p[d]) / dir[d];
    else if (dir[d] < 0.0) td = p[d] / (-dir[d]);
    if (td < t) {
      t = td;
      axis = d;
    }
  }
}

AAMD_HD long long quantise(double e, double scale) {
  const double v = rint(e * scale);
  return v < 9.2233720368547758e18 ? (long long)v : kSaturated;     // NaN saturates too
}

// e[band] = num[band] / (r2 p_hit) at distance d, into bin floor(d / w_bin) of microphone m if that is a bin
template <int NBC, class Sink>
AAMD_HD void deposit(const Args& a, int64_t b, int m, double d, const double* num, Sink& sink) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double x = floor(d / a.w_bin);
  if (!(x >= 0.0 && x < (double)a.bins)) return;
  const int64_t bin = (int64_t)x;
  const double r2 = fmax(d * d, a.r2);
  const double p_hit = 1.0 - sqrt(1.0 - a.r2 / r2);
  const double den = r2 * p_hit;
#pragma unroll
  for (int band = 0; band < NBC; ++band)
    if (band < a.NB) {
      const long long q = quantise(num[band] / den, a.scale);
      if (q != 0) sink.add(((b * a.M + m) * a.NB + band) * a.bins + bin, q);
    }
}

// step 2: the segment p + s dir, 0 <= s <= t, against the sphere of microphone m
template <int D, int NBC, class Sink>
AAMD_HD void direct_hit(const Args& a, const Room& rm, int64_t b, int m, const double* p, const double* dir, double t,
                        double travel, const double* tr, Sink& sink) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double u = 0.0, vv = 0.0;
#pragma unroll
  for (int d = 0; d < D; ++d) {
    const double v = rm.mic[m * D + d] - p[d];
    u += v * dir[d];
    vv += v * v;
  }
  const double q = vv - u * u;
  if (!(u >= 0.0 && u <= t && q < a.r2)) return;
  deposit<NBC>(a, b, m, travel + u, tr, sink);
}

// step 4: what microphone m sees of the energy scattered at the wall point p of wall w (axis `axis`)
template <int D, int NBC, class Sink>
AAMD_HD void scattered(const Args& a, const Room& rm, int64_t b, int m, const double* p, int axis, int w, double travel,
                       const double* tr, Sink& sink) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double h2 = 0.0, va = 0.0;
#pragma unroll
  for (int d = 0; d < D; ++d) {
    const double v = rm.mic[m * D + d] - p[d];
    h2 += v * v;
    va = d == axis ? fabs(v) : va;
  }
  const double h = sqrt(h2);
  const double cos_theta = va / h;
  const double h2c = fmax(h2, a.r2);
  const double p_eq = 1.0 - sqrt(1.0 - a.r2 / h2c);
  double st[NBC], top = 0.0;
#pragma unroll
  for (int band = 0; band < NBC; ++band) {
    st[band] = band < a.NB ? 2.0 * cos_theta * p_eq * tr[band] * rm.sc[band * 2 * D + w] : 0.0;
    top = fmax(top, st[band]);
  }
  const double d = travel + h;
  if (!(d < a.s_max && top > a.energy_thres)) return;
  deposit<NBC>(a, b, m, d, st, sink);
}

// ray i of room b, at most `bounces` steps
template <int D, int NBC, class Sink>
AAMD_HD void trace_ray(const Args& a, const Room& rm, int64_t b, int64_t i, int bounces, Sink& sink) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double p[D], dir[D], tr[NBC];
  direction<D>(i, a.N, dir);
#pragma unroll
  for (int d = 0; d < D; ++d) p[d] = rm.source[d];
#pragma unroll
  for (int band = 0; band < NBC; ++band) tr[band] = band < a.NB ? a.e0 : 0.0;
  double travel = 0.0;
  for (int k = 0; k < bounces; ++k) {
    double t;
    int axis;
    next_wall<D>(p, dir, rm, t, axis);
    bool up = false;
#pragma unroll
    for (int d = 0; d < D; ++d) up = d == axis ? dir[d] > 0.0 : up;
    const int w = 2 * axis + (up ? 1 : 0);                        // in [0, 2 D): axis is a loop index, not a data value
    for (int m = 0; m < a.M; ++m) direct_hit<D, NBC>(a, rm, b, m, p, dir, t, travel, tr, sink);
    travel += t;
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const double moved = p[d] + t * dir[d];
      p[d] = d == axis ? (up ? rm.room[d] : 0.0) : moved;
    }
    bool any = false;
#pragma unroll
    for (int band = 0; band < NBC; ++band)
      if (band < a.NB) {
        tr[band] *= 1.0 - rm.ab[band * 2 * D + w];
        any = any || rm.sc[band * 2 * D + w] > 0.0;
      }
    if (any)
      for (int m = 0; m < a.M; ++m) scattered<D, NBC>(a, rm, b, m, p, axis, w, travel, tr, sink);
    double top = 0.0;
#pragma unroll
    for (int band = 0; band < NBC; ++band)
      if (band < a.NB) {
        tr[band] *= 1.0 - rm.sc[band * 2 * D + w];
        top = fmax(top, tr[band]);
      }
    if (!(travel <= a.s_max) || top < a.energy_thres) break;
#pragma unroll
    for (int d = 0; d < D; ++d) dir[d] = d == axis ? -dir[d] : dir[d];
  }
}

// element j of room b's block of the result
template <int DT>
AAMD_HD void convert(const Args& a, int64_t b, int64_t per_room, int64_t j, bool bad) {
  if (j >= per_room) return;
  const long long q = a.acc[b * per_room + j];
  const bool nan = bad || q < 0;
  if (DT == kF64) static_cast<double*>(a.out)[b * per_room + j] = nan ? (double)NAN : ldexp((double)q, -a.k);
  else static_cast<float*>(a.out)[b * per_room + j] = nan ? (float)NAN : ldexpf((float)q, -a.k);
}

#if defined(__HIPCC__)
struct AtomicSink {
  long long* acc;
  __device__ __forceinline__ void add(int64_t idx, long long q) {
    atomicAdd(reinterpret_cast<unsigned long long*>(acc) + idx, (unsigned long long)q);
  }
};

template <int DT, int D, int NBC>
__global__ __launch_bounds__(kThreads) void trace_kernel(Args a) {
  __shared__ Room rm;
  const int tid = threadIdx.x;
  const int64_t b = (int64_t)blockIdx.x / a.blocks_per_room, run = (int64_t)blockIdx.x - b * a.blocks_per_room;
  load_room<DT>(tid, kThreads, a, b, rm);
  __syncthreads();
  if (__syncthreads_or(room_bad_part(tid, kThreads, a, rm))) return;
  const int64_t i = run * kThreads + tid;
  if (i >= a.N) return;
  AtomicSink sink{a.acc};
  trace_ray<D, NBC>(a, rm, b, i, (int)bounce_bound(a, rm), sink);     // the bound is <= kMaxBounces here
}

template <int DT>
__global__ __launch_bounds__(kThreads) void convert_kernel(Args a) {
  __shared__ Room rm;
  const int tid = threadIdx.x;
  const int64_t b = (int64_t)blockIdx.x / a.blocks_per_room, part = (int64_t)blockIdx.x - b * a.blocks_per_room;
  load_room<DT>(tid, kThreads, a, b, rm);
  __syncthreads();
  const bool bad = __syncthreads_or(room_bad_part(tid, kThreads, a, rm)) != 0;
  convert<DT>(a, b, (int64_t)a.M * a.NB * a.bins, part * kThreads + tid, bad);
}
#endif

}  // namespace ray
}  // namespace aamd
