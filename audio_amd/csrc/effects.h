// SoX-style effects (F.overdrive, F.phaser, F.flanger): the three functions whose reference is a Python loop over samples.
//
// phaser / flanger.  Every output sample is one fixed expression tree over earlier samples, so any schedule that keeps the
// dependencies gives the reference's bits.  Two routes:
//   delay_kernel   the general route (phaser; flanger with regen != 0).  Rows are independent, time is serial within a row:
//                  one row per lane, kRows rows per workgroup.  Input and output move through LDS in tiles of kTile samples:
//                  the workgroup moves a tile with 16-byte accesses that are coalesced along time (rows that do not start on a
//                  16-byte boundary sample by sample, as in wave_augment.h) and the lanes read it transposed (pitch kTile + 1:
//                  no bank conflict).  The delay ring is laid out [position][lane], conflict-free whatever position a lane
//                  reads -- the flanger's channels sit at different phases of the modulation table.  It lives in LDS where
//                  kRows x L elements fit beside the tile (ring_in_lds), else in the caller's workspace, kRows x L elements per
//                  workgroup, which stay in L2.  The modulation table is read from global memory, the tile's entries once per
//                  tile into LDS beside the samples (table_load), so that no global load sits in the serial loop: the phaser's
//                  entry is the same for every lane, the flanger's differs per channel by cph[c].
//   stream_kernel  flanger with regen == 0: the ring holds x itself, so out[i] = x[i] ig + interp(x[i - k], x[i - k - 1]
//                  (, x[i - k - 2])) dg is a streaming gather: one thread per 16 / sizeof samples, rows of any stride read in
//                  place.  Indices below 0 read zero; a lag of L aliases to 0 (the quadratic tap k + 2 = L reads the sample
//                  just written).  Equal to the general route bit for bit on finite input, except that the general route
//                  stores x + last * 0 in the ring, which turns a stored -0.0 into +0.0 where last * 0 is +0.0; here x is read
//                  as stored.  A non-finite sample reaches only the outputs whose taps read it.
// Products that the reference rounds on their own go through wa::rounded() (the library is built with -ffp-contract=fast).
// float16 / bfloat16 are widened in the tile load, computed in float32 and rounded once in the tile store.
//
// overdrive.  t = soft clip of x g + c (element-wise), y[i] = (t[i] - t[i-1]) + 0.995 y[i-1], out = clamp(0.5 x + 0.75 y).
// A first-order linear recurrence: two launches in the style of add_noise, no floating-point atomics, two calls give the
// same bits.  The state is float64 for every dtype.  A workgroup owns a chunk of kOdChunk samples of one row, a thread
// kOdSeg consecutive ones:
//   reduce  every thread scans its samples from a zero state; a Hillis-Steele scan over the threads (the partner's value
//           times 0.995 ^ (kOdSeg * offset)) leaves the chunk's end state from a zero incoming state in the last thread,
//           which writes it to the workspace.
//   apply   the chunk's incoming state is the Horner sum of the earlier chunks' end states, in order (so a NaN lives on, as
//           in the reference's loop); thread 0 starts from it, the same scan gives every thread its incoming state, and
//           each thread scans its samples again and writes them.
//
// The phase functions are AAMD_HD: tests/cpu_sim/sim_effects.cpp replays them with g++.
#pragma once
#include <math.h>

#include "wave_augment.h"

namespace aamd {
namespace fx {

using wa::Elem;
using wa::Vec;
using wa::aligned16;
using wa::load_group;
using wa::rounded;
using wa::store_group;

constexpr int kRows = 64;                 // rows (= lanes) per workgroup of the delay-line kernel
constexpr int kTile = 64;                 // samples of every row that pass through LDS at a time
constexpr int kPitch = kTile + 1;         // elements between two rows of the LDS tile
constexpr int kBlock = 8;                 // samples whose inputs a lane fetches from LDS ahead of their serial steps
constexpr int64_t kLdsBytes = 160 * 1024;
constexpr int kPhaserMaxRing = 512;
constexpr int kFlangerMaxRing = 4096;
constexpr int64_t kMaxTable = 1 << 24;
constexpr int kMaxChannels = 4;

constexpr int kOdThreads = 256;
constexpr int kOdSeg = 16;                // consecutive samples per thread
constexpr int kOdChunk = kOdThreads * kOdSeg;
constexpr int kOdLevels = 8;              // log2(kOdThreads)

template <typename C>
AAMD_HD C clamp1(C v) {                   // a NaN stays a NaN
  return v < C(-1) ? C(-1) : (v > C(1) ? C(1) : v);
}

// ---- phaser / flanger -------------------------------------------------------------------------------------------------------
struct DelayArgs {
  const void* x;                // (rows, T) through sx
  void* out;                    // dense (rows, T)
  void* ws;                     // the rings of the workspace route: [workgroup][position][lane] compute elements
  const void* table;            // phaser: int32[M] in [1, L]; flanger: float[M] in [0, L - 2]
  int64_t rows, T, sx, M;
  int64_t cph[kMaxChannels];    // flanger: the channel's offset into the table
  double g0, g1, g2;            // phaser: gain_in, decay, gain_out; flanger: feedback gain, in gain, delay gain
  int32_t L, channels, quadratic;
};

// LDS ahead of the ring: the tile of samples, then the tile's table entries [channel][sample] as 32-bit words
template <typename C>
AAMD_HD int64_t tile_bytes() { return (int64_t)kRows * kPitch * (int64_t)sizeof(C) + (int64_t)kMaxChannels * kTile * 4; }
template <typename C>
AAMD_HD int64_t ring_bytes(int64_t L) { return (int64_t)kRows * L * (int64_t)sizeof(C); }
template <typename C>
AAMD_HD bool ring_in_lds(int64_t L) { return tile_bytes<C>() + ring_bytes<C>(L) <= kLdsBytes; }
AAMD_HD int64_t n_groups(int64_t rows) { return (rows + kRows - 1) / kRows; }

// The workgroup's share of moving tile [t0, t0 + kTile) of its rows from memory to LDS (widened) and back (rounded once).
// The load is in two halves, so that the kernel can have the next tile's loads in flight while it works on this one:
// tile_fetch brings the thread's kTile / V vectors into registers (all loads issued together), tile_put writes them to LDS.
template <int DT>
AAMD_HD void tile_fetch(int tid, const DelayArgs& a, int64_t grp, int64_t t0, Vec<typename Elem<DT>::S>* g) {
  using S = typename Elem<DT>::S;
  constexpr int V = 16 / sizeof(S), PR = kTile / V;
#pragma unroll
  for (int j = 0; j < PR; ++j) {
    const int q = j * kRows + tid;
    const int r = q / PR, v = q - r * PR;
    const int64_t row = grp * kRows + r, i0 = t0 + (int64_t)v * V;
    if (row >= a.rows || i0 >= a.T) continue;
    const S* x = static_cast<const S*>(a.x) + row * a.sx;
    load_group(x, aligned16(x), i0, a.T, g[j]);
  }
}
template <int DT>
AAMD_HD void tile_put(int tid, const DelayArgs& a, int64_t grp, int64_t t0, const Vec<typename Elem<DT>::S>* g,
                      typename Elem<DT>::C* tile) {
  using E = Elem<DT>;
  using S = typename E::S;
  constexpr int V = 16 / sizeof(S), PR = kTile / V;
#pragma unroll
  for (int j = 0; j < PR; ++j) {
    const int q = j * kRows + tid;
    const int r = q / PR, v = q - r * PR;
    if (grp * kRows + r >= a.rows || t0 + (int64_t)v * V >= a.T) continue;
#pragma unroll
    for (int k = 0; k < V; ++k) tile[r * kPitch + v * V + k] = E::load(g[j].e[k]);
  }
}
template <int DT>
AAMD_HD void tile_store(int tid, const DelayArgs& a, int64_t grp, int64_t t0, const typename Elem<DT>::C* tile) {
  using E = Elem<DT>;
  using S = typename E::S;
  constexpr int V = 16 / sizeof(S), PR = kTile / V;
  for (int q = tid; q < kRows * PR; q += kRows) {
    const int r = q / PR, v = q - r * PR;
    const int64_t row = grp * kRows + r, i0 = t0 + (int64_t)v * V;
    if (row >= a.rows || i0 >= a.T) continue;
    S* o = static_cast<S*>(a.out) + row * a.T;
    Vec<S> g;
#pragma unroll
    for (int k = 0; k < V; ++k) g.e[k] = E::store(tile[r * kPitch + v * V + k]);
    store_group(o, aligned16(o), i0, a.T, g);
  }
}

// The workgroup's share of fetching the table entries of tile [t0, t0 + kTile) for every channel (cph[0] = 0 for the phaser).
AAMD_HD void table_load(int tid, const DelayArgs& a, int64_t t0, uint32_t* tab) {
  const uint32_t* table = static_cast<const uint32_t*>(a.table);
  for (int q = tid; q < a.channels * kTile; q += kRows) {
    const int c = q / kTile, s = q - c * kTile;
    if (t0 + s < a.T) tab[q] = table[(t0 + s + a.cph[c]) % a.M];
  }
}

// What a lane carries from one tile to the next.
template <typename C>
struct Lane {
  int32_t pos;                  // ring position
  C last;                       // flanger: the delayed sample fed back
};

template <typename C>
AAMD_HD void lane_init(Lane<C>& st) {
  st.pos = 0;
  st.last = C(0);
}
// ring: the lane's column, elements kRows apart
template <typename C>
AAMD_HD void ring_clear(const DelayArgs& a, C* ring) {
  for (int p = 0; p < a.L; ++p) ring[(int64_t)p * kRows] = C(0);
}

// n samples of one row, in place in the lane's row of the tile; tab: the tile's table entries of the lane's channel.  The
// reference's ring, step for step: the feedback tap is read at (pos + m) mod L before pos moves on, the new sample is
// written at the new pos.
template <typename C>
AAMD_HD void phaser_lane(const DelayArgs& a, Lane<C>& st, C* t, C* ring, const uint32_t* tab, int n) {
  const C gin = (C)a.g0, decay = (C)a.g1, gout = (C)a.g2;
  const int32_t L = a.L;
  int32_t pos = st.pos;
  for (int s0 = 0; s0 < n; s0 += kBlock) {
    C p[kBlock];
    int32_t m[kBlock];
#pragma unroll
    for (int j = 0; j < kBlock; ++j) {                // what does not depend on the ring, fetched ahead of the serial part
      const int s = s0 + j < n ? s0 + j : n - 1;
      p[j] = rounded(t[s] * gin);
      m[j] = (int32_t)tab[s];
      m[j] = m[j] < 1 ? 1 : (m[j] > L ? L : m[j]);
    }
#pragma unroll
    for (int j = 0; j < kBlock; ++j) {
      if (s0 + j < n) {
        int32_t idx = pos + m[j];
        if (idx >= L) idx -= L;
        pos = pos + 1 == L ? 0 : pos + 1;
        const C f = rounded(ring[(int64_t)idx * kRows] * decay);
        const C v = p[j] + f;
        ring[(int64_t)pos * kRows] = v;
        p[j] = clamp1(v * gout);
      }
    }
#pragma unroll
    for (int j = 0; j < kBlock; ++j)
      if (s0 + j < n) t[s0 + j] = p[j];
  }
  st.pos = pos;
}

// One modulation-table entry as the integer and the fractional delay.
AAMD_HD void split_delay(float dt, int32_t L, int32_t& k, float& fr) {
  const float fl = floorf(dt);
  fr = dt - fl;
  k = fl >= 0.0f ? (fl <= (float)(L - 2) ? (int32_t)fl : L - 2) : 0;      // a table outside [0, L - 2] indexes nothing else
}

template <typename C>
AAMD_HD C interp(C d0, C d1, C d2, C fr, int quadratic) {
  if (!quadratic) return d0 + rounded((d1 - d0) * fr);
  d2 = d2 - d0;
  d1 = d1 - d0;
  const C h = rounded(d2 * C(0.5));
  const C qa = h - d1, qb = rounded(d1 * C(2)) - h;
  const C inner = rounded(qa * fr) + qb;
  return d0 + rounded(inner * fr);
}

template <typename C>
AAMD_HD void flanger_lane(const DelayArgs& a, Lane<C>& st, C* t, C* ring, const uint32_t* tab, int n) {
  const C fg = (C)a.g0, ig = (C)a.g1, dg = (C)a.g2;
  const int32_t L = a.L;
  int32_t pos = st.pos;
  C last = st.last;
  for (int s0 = 0; s0 < n; s0 += kBlock) {
    C x[kBlock], fr[kBlock];
    int32_t k[kBlock];
#pragma unroll
    for (int j = 0; j < kBlock; ++j) {                // what does not depend on the ring, fetched ahead of the serial part
      const int s = s0 + j < n ? s0 + j : n - 1;
      float frf;
      x[j] = t[s];
      split_delay(sa::bits_f32(tab[s]), L, k[j], frf);
      fr[j] = (C)frf;
    }
#pragma unroll
    for (int j = 0; j < kBlock; ++j) {
      if (s0 + j < n) {
        pos = pos == 0 ? L - 1 : pos - 1;
        ring[(int64_t)pos * kRows] = x[j] + rounded(last * fg);   // written before the reads
        int32_t i0 = pos + k[j];
        if (i0 >= L) i0 -= L;
        const int32_t i1 = i0 + 1 == L ? 0 : i0 + 1;
        const int32_t i2 = i1 + 1 == L ? 0 : i1 + 1;
        const C d0 = ring[(int64_t)i0 * kRows], d1 = ring[(int64_t)i1 * kRows];
        const C d2 = a.quadratic ? ring[(int64_t)i2 * kRows] : C(0);
        const C d = interp(d0, d1, d2, fr[j], a.quadratic);
        last = d;
        const C p = rounded(x[j] * ig), q = rounded(d * dg);
        x[j] = clamp1(p + q);
      }
    }
#pragma unroll
    for (int j = 0; j < kBlock; ++j)
      if (s0 + j < n) t[s0 + j] = x[j];
  }
  st.pos = pos; st.last = last;
}

// flanger without feedback: one thread's groups of a chunk of wa::kChunk samples
template <int DT>
AAMD_HD void stream_thread(int tid, const DelayArgs& a, int64_t row, int64_t chunk) {
  using E = Elem<DT>;
  using S = typename E::S;
  using C = typename E::C;
  constexpr int V = 16 / sizeof(S);
  const S* x = static_cast<const S*>(a.x) + row * a.sx;
  S* o = static_cast<S*>(a.out) + row * a.T;
  const float* table = static_cast<const float*>(a.table);
  const bool vx = aligned16(x), vo = aligned16(o);
  const C ig = (C)a.g1, dg = (C)a.g2;
  const int32_t L = a.L;
  const int64_t cph = a.cph[row % a.channels];
  const int64_t c0 = chunk * wa::kChunk;
  const int64_t c1 = c0 + wa::kChunk < a.T ? c0 + wa::kChunk : a.T;
  for (int64_t i0 = c0 + (int64_t)tid * V; i0 < c1; i0 += (int64_t)wa::kThreads * V) {
    Vec<S> xv, r;
    load_group(x, vx, i0, c1, xv);
    int64_t tp = (i0 + cph) % a.M;
#pragma unroll
    for (int e = 0; e < V; ++e) {
      const int64_t i = i0 + e;
      if (i < c1) {
        int32_t k;
        float frf;
        split_delay(table[tp], L, k, frf);
        const int64_t j0 = i - k, j1 = j0 - 1, j2 = k + 2 == L ? i : j0 - 2;
        const C d0 = j0 >= 0 ? E::load(x[j0]) : C(0), d1 = j1 >= 0 ? E::load(x[j1]) : C(0);
        const C d2 = a.quadratic && j2 >= 0 ? E::load(x[j2]) : C(0);
        const C d = interp(d0, d1, d2, (C)frf, a.quadratic);
        const C xi = E::load(xv.e[e]);
        const C p = rounded(xi * ig), q = rounded(d * dg);
        r.e[e] = E::store(clamp1(p + q));
      } else {
        r.e[e] = S(0);
      }
      tp = tp + 1 == a.M ? 0 : tp + 1;
    }
    store_group(o, vo, i0, c1, r);
  }
}

// ---- overdrive --------------------------------------------------------------------------------------------------------------
struct OdArgs {
  const void* x;                // (rows, T) through sx
  void* out;                    // dense (rows, T)
  double* ws;                   // [rows][chunks]: the chunk's end state from a zero incoming state
  int64_t rows, T, sx, chunks;
  double gain, colour;          // 10 ^ (gain dB / 20) and colour / 200
};

AAMD_HD int64_t od_chunks(int64_t T) { return (T + kOdChunk - 1) / kOdChunk; }

template <typename C>
AAMD_HD C od_coef() { return C(0.995); }

// pw[l] = 0.995 ^ (kOdSeg << l) in float64 by squaring; pw[kOdLevels] is the power of a whole chunk
template <typename C>
AAMD_HD void od_powers(double pw[kOdLevels + 1]) {
  double p = (double)od_coef<C>();
  for (int k = 1; k < kOdSeg; k <<= 1) p = p * p;
  for (int l = 0; l <= kOdLevels; ++l) {
    pw[l] = p;
    p = p * p;
  }
}

template <typename C>
AAMD_HD C od_shape(C x, C g, C c) {
  const C p = rounded(x * g);
  const C t = p + c;
  if (t < C(-1)) return C(-2.0 / 3.0);
  if (t > C(1)) return C(2.0 / 3.0);
  const C t2 = rounded(t * t);
  const C t3 = rounded(t2 * t);
  return t - rounded(t3 * C(1.0 / 3.0));
}

// The thread's kOdSeg samples (zero bits beyond the row) and their shaped values; tprev: the shaped sample before them.
template <int DT>
AAMD_HD void od_fetch(int tid, const OdArgs& a, int64_t row, int64_t chunk, Vec<typename Elem<DT>::S>* xv,
                      typename Elem<DT>::C* t, typename Elem<DT>::C& tprev) {
  using E = Elem<DT>;
  using S = typename E::S;
  using C = typename E::C;
  constexpr int V = 16 / sizeof(S);
  const S* x = static_cast<const S*>(a.x) + row * a.sx;
  const bool vx = aligned16(x);
  const C g = (C)a.gain, c = (C)a.colour;
  const int64_t i0 = chunk * kOdChunk + (int64_t)tid * kOdSeg;
#pragma unroll
  for (int j = 0; j < kOdSeg / V; ++j) {
    if (i0 + j * V < a.T) {
      load_group(x, vx, i0 + j * V, a.T, xv[j]);
    } else {
#pragma unroll
      for (int k = 0; k < V; ++k) xv[j].e[k] = S(0);
    }
  }
  tprev = (i0 > 0 && i0 - 1 < a.T) ? od_shape(E::load(x[i0 - 1]), g, c) : C(0);
#pragma unroll
  for (int j = 0; j < kOdSeg / V; ++j)
#pragma unroll
    for (int k = 0; k < V; ++k) t[j * V + k] = od_shape(E::load(xv[j].e[k]), g, c);
}

// the state after the thread's samples, from state y
template <typename C>
AAMD_HD double od_segment_end(const C* t, C tprev, double y) {
  const double c = (double)od_coef<C>();
  double prev = (double)tprev;
#pragma unroll
  for (int j = 0; j < kOdSeg; ++j) {
    const double tj = (double)t[j];
    y = (tj - prev) + c * y;
    prev = tj;
  }
  return y;
}

// one step of the scan over the threads' end states; the kernel separates the steps by barriers
AAMD_HD void od_scan_step(int tid, int level, const double* pw, const double* in, double* out) {
  const int off = 1 << level;
  out[tid] = tid >= off ? in[tid] + pw[level] * in[tid - off] : in[tid];
}

// Horner step over a batch of earlier chunks' end states (sp[0 .. n))
AAMD_HD double od_horner(double y, double pchunk, const double* sp, int n) {
  for (int j = 0; j < n; ++j) y = pchunk * y + sp[j];
  return y;
}

template <int DT>
AAMD_HD void od_write(int tid, const OdArgs& a, int64_t row, int64_t chunk, const Vec<typename Elem<DT>::S>* xv,
                      const typename Elem<DT>::C* t, typename Elem<DT>::C tprev, double y) {
  using E = Elem<DT>;
  using S = typename E::S;
  using C = typename E::C;
  constexpr int V = 16 / sizeof(S);
  S* o = static_cast<S*>(a.out) + row * a.T;
  const bool vo = aligned16(o);
  const double c = (double)od_coef<C>();
  const int64_t i0 = chunk * kOdChunk + (int64_t)tid * kOdSeg;
  double prev = (double)tprev;
#pragma unroll
  for (int j = 0; j < kOdSeg / V; ++j) {
    Vec<S> r;
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const double tj = (double)t[j * V + k];
      y = (tj - prev) + c * y;
      prev = tj;
      const C p = rounded(E::load(xv[j].e[k]) * C(0.5)), q = rounded((C)y * C(0.75));
      r.e[k] = E::store(clamp1(p + q));
    }
    if (i0 + j * V < a.T) store_group(o, vo, i0 + j * V, a.T, r);
  }
}

#if defined(__HIPCC__)
template <int DT, bool FLANGER, bool LDSRING>
__global__ __launch_bounds__(kRows) void delay_kernel(DelayArgs a) {
  using C = typename Elem<DT>::C;
  extern __shared__ __align__(16) unsigned char fx_smem[];
  C* tile = reinterpret_cast<C*>(fx_smem);
  uint32_t* tab = reinterpret_cast<uint32_t*>(tile + kRows * kPitch);
  const int lane = threadIdx.x;
  const int64_t grp = blockIdx.x, row = grp * kRows + lane;
  C* ring = (LDSRING ? reinterpret_cast<C*>(fx_smem + tile_bytes<C>()) : static_cast<C*>(a.ws) + grp * kRows * (int64_t)a.L) + lane;
  const bool active = row < a.rows;
  const uint32_t* mytab = tab + (active ? (int)(row % a.channels) : 0) * kTile;
  Lane<C> st;
  lane_init(st);
  Vec<typename Elem<DT>::S> next[kTile * sizeof(typename Elem<DT>::S) / 16];
  tile_fetch<DT>(lane, a, grp, 0, next);
  if (active) ring_clear(a, ring);
  for (int64_t t0 = 0; t0 < a.T; t0 += kTile) {
    tile_put<DT>(lane, a, grp, t0, next, tile);
    table_load(lane, a, t0, tab);
    __syncthreads();
    if (t0 + kTile < a.T) tile_fetch<DT>(lane, a, grp, t0 + kTile, next);     // in flight during the serial part
    const int n = a.T - t0 < kTile ? (int)(a.T - t0) : kTile;
    if (active) {
      if (FLANGER) flanger_lane(a, st, tile + lane * kPitch, ring, mytab, n);
      else phaser_lane(a, st, tile + lane * kPitch, ring, mytab, n);
    }
    __syncthreads();
    tile_store<DT>(lane, a, grp, t0, tile);
    __syncthreads();
  }
}

template <int DT>
__global__ __launch_bounds__(wa::kThreads) void stream_kernel(DelayArgs a, int64_t chunks) {
  const int64_t row = (int64_t)blockIdx.x / chunks, chunk = (int64_t)blockIdx.x - row * chunks;
  stream_thread<DT>(threadIdx.x, a, row, chunk);
}

// the scan over the threads' end states; the result is in s[kOdLevels & 1]
AAMD_D const double* od_scan(int tid, const double* pw, double (*s)[kOdThreads]) {
  __syncthreads();
#pragma unroll
  for (int l = 0; l < kOdLevels; ++l) {
    od_scan_step(tid, l, pw, s[l & 1], s[(l + 1) & 1]);
    __syncthreads();
  }
  return s[kOdLevels & 1];
}

template <int DT>
__global__ __launch_bounds__(kOdThreads) void overdrive_reduce_kernel(OdArgs a) {
  using E = Elem<DT>;
  using S = typename E::S;
  using C = typename E::C;
  __shared__ double s[2][kOdThreads];
  const int tid = threadIdx.x;
  const int64_t row = (int64_t)blockIdx.x / a.chunks, chunk = (int64_t)blockIdx.x - row * a.chunks;
  double pw[kOdLevels + 1];
  od_powers<C>(pw);
  Vec<S> xv[kOdSeg * sizeof(S) / 16];
  C t[kOdSeg], tprev;
  od_fetch<DT>(tid, a, row, chunk, xv, t, tprev);
  s[0][tid] = od_segment_end(t, tprev, 0.0);
  const double* r = od_scan(tid, pw, s);
  if (tid == kOdThreads - 1) a.ws[row * a.chunks + chunk] = r[tid];
}

template <int DT>
__global__ __launch_bounds__(kOdThreads) void overdrive_apply_kernel(OdArgs a) {
  using E = Elem<DT>;
  using S = typename E::S;
  using C = typename E::C;
  __shared__ double s[2][kOdThreads];
  const int tid = threadIdx.x;
  const int64_t row = (int64_t)blockIdx.x / a.chunks, chunk = (int64_t)blockIdx.x - row * a.chunks;
  double pw[kOdLevels + 1];
  od_powers<C>(pw);
  Vec<S> xv[kOdSeg * sizeof(S) / 16];
  C t[kOdSeg], tprev;
  od_fetch<DT>(tid, a, row, chunk, xv, t, tprev);
  double y0 = 0.0;                                     // thread 0: the chunk's incoming state
  for (int64_t base = 0; base < chunk; base += kOdThreads) {
    const int n = chunk - base < kOdThreads ? (int)(chunk - base) : kOdThreads;
    if (tid < n) s[0][tid] = a.ws[row * a.chunks + base + tid];
    __syncthreads();
    if (tid == 0) y0 = od_horner(y0, pw[kOdLevels], s[0], n);
    __syncthreads();
  }
  s[0][tid] = od_segment_end(t, tprev, y0);
  const double* r = od_scan(tid, pw, s);
  od_write<DT>(tid, a, row, chunk, xv, t, tprev, tid == 0 ? y0 : r[tid - 1]);
}
#endif

}  // namespace fx
}  // namespace aamd
