// Room impulse responses of shoebox rooms by the image-source method (F.simulate_rir_ism, F.simulate_rir_ism_batch), whose
// reference builds the images in Python and lays the delay filters down in a CPU-only operator, one room at a time.
//
//   rir[c][n] = sum_i a_ic g(n - pad - tau_ic),   g(x) = sinc(x) (1 + cos(pi x / pad)) / 2 for |x| <= pad, else 0
//
// over the images i of the lattice table (ascending), with a = att / dist and tau = dist sample_rate / sound_speed: the
// gather form of the reference's scatter (every output sample collects the filters that cover it), so no atomics, and a
// sample's sum does not depend on the batch, on the tile it falls in or on the output length.  One launch:
//   rir_kernel   a workgroup of kThreads owns kTile consecutive samples of one (room, microphone).  It first builds in LDS
//                the powers of the six wall transmissions and (cos, sin)(pi k / pad) for -pad <= k < pad.  Then it walks the
//                lattice in chunks of kChunk images: every lane forms one image's geometry in float64 (image_term), a
//                ballot per wave and a prefix popcount (list_slot) compact the images whose taps meet the tile into an LDS
//                list in index order.  Each wave then culls the list against the 64-sample stretches it owns (lane_hit, one
//                listed image per lane, a ballot) and adds the images that remain, two at a time (add_hits).  Every
//                tile visits every image, so a non-finite tau or a anywhere poisons every tile of the row: the whole row
//                comes back NaN.  Nothing is indexed with a data value: the list holds ceil(tau) only for images that meet
//                the tile, and the table index n - ceil(tau) is used only inside [0, 2 pad).  The list is double-buffered,
//                so a chunk costs two barriers and the waves with no tap of it go on to the next chunk's geometry.
// With tc = ceil(tau), delta = tc - tau in [0, 1) and m = n - tc: x = (m - pad) + delta, the taps are m = 0 .. 2 pad - 1 (for
// delta = 0 the definition also has m = 2 pad, where g(pad) is exactly 0), sin(pi x) = (-1)^(m - pad) sin(pi delta) and
// cos(pi x / pad) = cos(pi (m - pad) / pad) cos(pi delta / pad) - sin(pi (m - pad) / pad) sin(pi delta / pad).  So a tap
// costs one float64 division and a few multiply-adds, and the three transcendentals are per image, not per tap.  sin(pi
// delta) is taken of min(delta, 1 - delta) (exact), so the tap next to the peak keeps its relative accuracy when delta is
// close to 1.  An 81-tap filter covers two or three of the eight 64-sample stretches of a tile, and the tap loop is bound by
// latency (LDS reads, then the division chain), not by issue: testing every listed image in every lane cost as much as the
// taps, and the wave-level cull alone did not help until the taps lost their branch and went two at a time.
//
// The phase functions are AAMD_HD: tests/cpu_sim/sim_rir.cpp replays them with g++.
#pragma once
#include <math.h>

#include "hd.h"

namespace aamd {
namespace rir {

constexpr int kThreads = 256;
constexpr int kPerLane = 2;                    // samples of a lane: n = tile start + j kThreads + tid
constexpr int kTile = kThreads * kPerLane;     // samples per workgroup
constexpr int kChunk = kThreads;               // images per chunk: one per lane
constexpr int kWaves = kThreads / 64;
constexpr int kMaxFl = 1025;                   // the (cos, sin) table of it takes 16 KiB of LDS
constexpr int kMaxOrder = 64;                  // 357 889 images in 3-D; the lattice table is int16
constexpr int kF32 = 0, kF64 = 1;              // AAMD_SA_F32 / AAMD_SA_F64
constexpr double kPi = 3.14159265358979323846;
constexpr int32_t kNever = 0x7fffffff;         // a ceil(tau) no sample reaches: what a lane behind the list's end tests

struct Args {
  const void *room, *source, *mic, *absorption;   // (B, D), (B, D), (B, M, D), (B, 2 D) dense, of the element type
  const int16_t* lattice;                          // (n_img, D)
  void* out;                                       // (B, M, L) dense
  int64_t B, M, L, n_img, tiles;                   // tiles per row = ceil(L / kTile)
  double sample_rate, sound_speed;
  int32_t D, order, pad;
};

struct alignas(16) Listed {  // an image whose taps meet the tile
  double delta;              // ceil(tau) - tau
  double s;                  // a sin(pi delta) / pi
  double hc, hs;             // cos(pi delta / pad) / 2, -sin(pi delta / pad) / 2
};

struct Term {
  Listed e;
  double a;                  // att / dist
  int32_t tc;                // ceil(tau)
  bool bad;                  // tau or a is not finite
  bool meets;                // a tap falls in [t0, t0 + kTile)
};

struct Lists {               // LDS of a chunk
  int32_t tc[kChunk];
  Listed e[kChunk];
  double a[kChunk];
};

AAMD_HD int pow_rows(int order) { return order / 2 + 2; }               // exponents 0 .. order / 2 + 1
AAMD_HD size_t lds_doubles(int order, int pad) { return (size_t)6 * pow_rows(order) + 2 * (size_t)(2 * pad); }
AAMD_HD size_t lds_bytes(int order, int pad) { return lds_doubles(order, pad) * sizeof(double); }

template <int DT>
AAMD_HD double ld(const void* p, int64_t i) {
  return DT == kF64 ? static_cast<const double*>(p)[i] : (double)static_cast<const float*>(p)[i];
}

AAMD_HD bool finite_(double v) { return fabs(v) <= 1.7976931348623157e308; }      // false for NaN

// ---- the tables of a workgroup -------------------------------------------------------------------------------------------
// pw[w][e] = sqrt(1 - absorption_w)^e by repeated multiplication, w = 2 d + (upper wall), e < pow_rows: lanes 0 .. 2 D - 1
template <int DT>
AAMD_HD void build_powers(int tid, const Args& a, int64_t b, double* pw) {
  if (tid >= 2 * a.D) return;
  const int rows = pow_rows(a.order);
  const double tr = sqrt(1.0 - ld<DT>(a.absorption, b * 2 * a.D + tid));
  double p = 1.0;
  for (int e = 0; e < rows; ++e) {
    pw[tid * rows + e] = p;
    p *= tr;
  }
}

// cs[m] = (cos, sin)(pi (m - pad) / pad), 0 <= m < 2 pad
AAMD_HD void build_hann(int tid, const Args& a, double* cs) {
  for (int i = tid; i < 2 * a.pad; i += kThreads) {
    const double t = kPi * (double)(i - a.pad) / (double)a.pad;
    cs[2 * i] = cos(t);
    cs[2 * i + 1] = sin(t);
  }
}

// ---- one image and one microphone -------------------------------------------------------------------------------------------
template <int DT>
AAMD_HD Term image_term(const Args& a, int64_t b, int64_t c, int64_t img, int64_t t0, const double* pw) {
  // every product below is rounded on its own, so tau is the float64 value of the definition read left to right (a fused
  // multiply-add in the sum of squares would move it by an ulp, which is the whole float64 error budget of a single image)
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const int rows = pow_rows(a.order);
  double d2 = 0.0, att = 1.0;
  for (int d = 0; d < a.D; ++d) {
    const int v = a.lattice[img * a.D + d];
    const double room = ld<DT>(a.room, b * a.D + d), src = ld<DT>(a.source, b * a.D + d);
    const double loc = (v & 1) ? room * (double)(v + 1) - src : room * (double)v + src;
    const double diff = loc - ld<DT>(a.mic, (b * a.M + c) * a.D + d);
    d2 += diff * diff;
    const int lo = v >> 1, hi = (v + 1) >> 1;                        // floor(v / 2), floor((v + 1) / 2)
    const int elo = lo < 0 ? -lo : lo, ehi = hi < 0 ? -hi : hi;       // <= order / 2 + 1 for |v| <= order; clamped for any table
    att *= pw[(2 * d) * rows + (elo < rows ? elo : rows - 1)] * pw[(2 * d + 1) * rows + (ehi < rows ? ehi : rows - 1)];
  }
  const double dist = sqrt(d2);
  const double amp = att / dist;
  const double tau = dist * a.sample_rate / a.sound_speed;
  const double up = ceil(tau);
  Term t{};
  t.bad = !(finite_(tau) && finite_(amp));
  // the taps n = ceil(tau) .. ceil(tau) + 2 pad - 1 meet [t0, t0 + kTile); a ceil(tau) that passes lies in (-2 pad, 2^31)
  t.meets = !t.bad && up < (double)(t0 + kTile) && up + (double)(2 * a.pad) > (double)t0;
  if (!t.meets) return t;
  const double delta = up - tau;
  const double r = delta <= 0.5 ? delta : 1.0 - delta;
  const double w = kPi * delta / (double)a.pad;
  t.a = amp;
  t.tc = (int32_t)up;
  t.e.delta = delta;
  t.e.s = amp * sin(kPi * r) / kPi;
  t.e.hc = 0.5 * cos(w);
  t.e.hs = -0.5 * sin(w);
  return t;
}

AAMD_HD int popc64(unsigned long long m) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __popcll(m);
#else
  return __builtin_popcountll(m);
#endif
}

// where lane `tid` writes its image in the list, given the ballots of the waves; the list's length with tid = kThreads
AAMD_HD int list_slot(int tid, const unsigned long long* masks) {
  const int w = tid >> 6, lane = tid & 63;
  int n = 0;
  for (int i = 0; i < w && i < kWaves; ++i) n += popc64(masks[i]);
  if (w < kWaves && lane) n += popc64(masks[w] & (~0ull >> (64 - lane)));
  return n;
}

// lane `tid` puts its image at its slot
AAMD_HD void list_write(int tid, const Term& t, const unsigned long long* masks, Lists& l) {
  if (!t.meets) return;
  const int s = list_slot(tid, masks);
  l.tc[s] = t.tc;
  l.e[s] = t.e;
  l.a[s] = t.a;
}

// does an image with this ceil(tau) have a tap among the 64 samples from n_lo on?  m = n - tc in [0, taps) for some n
AAMD_HD bool wave_hit(int32_t tc, int32_t n_lo, uint32_t taps) { return (uint32_t)(n_lo + 63 - tc) < taps + 63u; }

// lane `lane` of the wave whose 64 samples start at n_lo tests listed image r0 + lane
AAMD_HD bool lane_hit(int lane, int32_t n_lo, const Args& a, const Lists& l, int r0, int count) {
  const int32_t tc = r0 + lane < count ? l.tc[r0 + lane] : kNever;
  return wave_hit(tc, n_lo, 2u * (uint32_t)a.pad);
}

AAMD_HD int ctz64(unsigned long long m) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __ffsll((long long)m) - 1;
#else
  return __builtin_ctzll(m);
#endif
}

// the tap of listed image j at sample n, 0.0 where n is not under its filter: no branch, so that two images' LDS reads
// and division chains overlap (a wave that gets here has lanes under the filter; the others ride along)
AAMD_HD double tap_or_zero(const Args& a, const Lists& l, int j, int32_t n, const double* cs) {
  const int32_t m = n - l.tc[j];
  const bool inside = (uint32_t)m < 2u * (uint32_t)a.pad;
  const int mc = inside ? m : 0;
  const Listed e = l.e[j];
  const int k = mc - a.pad;
  const double x = (double)k + e.delta;
  const double hann = 0.5 + (cs[2 * mc] * e.hc + cs[2 * mc + 1] * e.hs);
  const double v = x == 0.0 ? l.a[j] : ((k & 1) ? -e.s : e.s) / x * hann;
  return inside ? v : 0.0;
}

// acc += the taps at sample n of the listed images r0 + q, q a set bit of `hits` (the ballot of lane_hit: the same word for
// every lane of a wave, so the loop is the wave's, not the lane's), two at a time, added in ascending (= image) order.
// Adding the 0.0 of a lane outside a filter changes no bit: acc starts at +0.0 and a sum is -0.0 only if both terms are.
AAMD_HD void add_hits(const Args& a, int32_t n, const Lists& l, int r0, unsigned long long hits, const double* cs, double& acc) {
  while (hits) {
    const int j1 = r0 + ctz64(hits);
    hits &= hits - 1;
    const bool two = hits != 0;
    const int j2 = two ? r0 + ctz64(hits) : j1;
    hits &= hits - 1;
    const double v1 = tap_or_zero(a, l, j1, n, cs), v2 = tap_or_zero(a, l, j2, n, cs);
    acc += v1;
    acc += two ? v2 : 0.0;
  }
}

template <int DT>
AAMD_HD void store(const Args& a, int64_t row, int64_t n, double v, bool bad) {
  if (n >= a.L) return;
  if (bad) v = NAN;
  if (DT == kF64) static_cast<double*>(a.out)[row * a.L + n] = v;
  else static_cast<float*>(a.out)[row * a.L + n] = (float)v;
}

#if defined(__HIPCC__)
template <int DT>
__global__ __launch_bounds__(kThreads) void rir_kernel(Args a) {
  extern __shared__ __align__(16) double rir_smem[];
  __shared__ Lists lists[2];
  __shared__ unsigned long long masks[2][kWaves], bad_masks[2][kWaves];
  double* pw = rir_smem;
  double* cs = rir_smem + 6 * pow_rows(a.order);
  const int tid = threadIdx.x;
  const int64_t row = (int64_t)blockIdx.x / a.tiles, tile = (int64_t)blockIdx.x - row * a.tiles;
  const int64_t b = row / a.M, c = row - b * a.M, t0 = tile * kTile;
  build_powers<DT>(tid, a, b, pw);
  build_hann(tid, a, cs);
  __syncthreads();
  double acc[kPerLane];
  for (int j = 0; j < kPerLane; ++j) acc[j] = 0.0;
  bool bad = false;
  // two barriers a chunk: the ballots and the list of chunk i live in buffer i & 1, which is written again in chunk i + 2,
  // behind the first barrier of chunk i + 1, which no wave passes before every wave has added chunk i
  int buf = 0;
  for (int64_t i0 = 0; i0 < a.n_img; i0 += kChunk, buf ^= 1) {
    Term t{};
    if (i0 + tid < a.n_img) t = image_term<DT>(a, b, c, i0 + tid, t0, pw);
    const unsigned long long m = __ballot(t.meets), mb = __ballot(t.bad);
    if ((tid & 63) == 0) {
      masks[buf][tid >> 6] = m;
      bad_masks[buf][tid >> 6] = mb;
    }
    __syncthreads();
    list_write(tid, t, masks[buf], lists[buf]);
    const int count = list_slot(kThreads, masks[buf]);
    for (int w = 0; w < kWaves; ++w) bad = bad || bad_masks[buf][w] != 0;
    __syncthreads();
    for (int r0 = 0; r0 < count; r0 += 64)
      for (int p = 0; p < kPerLane; ++p) {
        const int32_t n_lo = (int32_t)t0 + p * kThreads + (tid & ~63);
        const unsigned long long hits = __ballot(lane_hit(tid & 63, n_lo, a, lists[buf], r0, count));
        add_hits(a, n_lo + (tid & 63), lists[buf], r0, hits, cs, acc[p]);
      }
  }
  for (int j = 0; j < kPerLane; ++j) store<DT>(a, row, t0 + j * kThreads + tid, acc[j], bad);
}
#endif

}  // namespace rir
}  // namespace aamd
