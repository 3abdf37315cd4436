// Batched Levenshtein distance with error counts (F.edit_distance_batch / F.edit_distance).
// hyps (pairs, N) and refs (pairs / per_ref, M) int32 / int64, optional lengths int32 / int64, all read on the device.  Pair p
// scores hypothesis p against reference p / per_ref.  Cell (i, j), 0 <= i <= M_p, 0 <= j <= N_p, holds (cost, S, D, I):
//     (0, j) = (j, 0, 0, j)      (i, 0) = (i, 0, i, 0)
//     (i, j) = the first of   (i-1, j-1) + (sub, sub, 0, 0)   [sub = r[i-1] != h[j-1]]
//                             (i-1, j)   + (1, 0, 1, 0)       [deletion]
//                             (i, j-1)   + (1, 0, 0, 1)       [insertion]
//              whose cost is smallest; the result is cell (M_p, N_p).
//
// One workgroup per pair, one launch, no workspace.  The reference lies across lanes x registers: lane l owns the rows
// l * KS + 1 .. l * KS + KS (reference positions l * KS .. l * KS + KS - 1, loaded once).  The hypothesis streams through as a
// skewed wavefront: at step s lane l works on column j = s - l.  Its KS cells run in sequence in registers (the deletion
// dependency), over its own previous column (the insertion dependency); from lane l - 1 it takes that lane's last cell of
// column j -- a one-lane shift inside a wave, a double-buffered LDS line with one barrier per step for the first lane of a
// wave -- and keeps the one it took a step earlier for the diagonal.  The hypothesis tokens come from an LDS ring of 2 NT
// tokens that all lanes refill every NT steps, each from a register it loaded NT steps before: lane l reads token j - 1 there.
// (KS, threads) follow from the tensor width M (config()), never from device data.
//
// A cell is one 64-bit word, cost << 48 | S << 32 | D << 16 | I; a candidate is one 64-bit add and the choice compares
// word >> 48 only.  With M <= kMaxRef and N <= kMaxHyp < 32768 no field carries: every field of a cell is at most
// max(M, N) <= 32767, and a candidate adds at most one to it.  Lanes beyond a pair's last row compute the rows of a reference
// padded with zeros (cells of a real problem no larger than NT * KS x N, so the bound holds) that nobody reads.
// A pair with a length outside [0, N] / [0, M] gets -1 in every field and no token of it is read.
//
// The phase functions are AAMD_HD: tests/cpu_sim/sim_edit_distance.cpp replays them with g++.
#pragma once
#include "hd.h"

#if !defined(AAMD_UNROLL)
#if defined(__HIPCC__)
#define AAMD_UNROLL _Pragma("unroll")
#else
#define AAMD_UNROLL
#endif
#endif

namespace aamd {
namespace ed {

constexpr int kMaxRef = 4096;        // 256 lanes x 16 rows
constexpr int kMaxHyp = 32767;       // fields of 16 bits: a candidate of a cell of cost 32767 is 32768
constexpr uint64_t kSub = (1ull << 48) | (1ull << 32);
constexpr uint64_t kDel = (1ull << 48) | (1ull << 16);
constexpr uint64_t kIns = (1ull << 48) | 1ull;

// rows per lane and lanes per workgroup for references of width M
AAMD_HD void config(int64_t M, int& ks, int& nt) {
  if (M <= 64 * 4) { ks = 4; nt = 64; }
  else if (M <= 256 * 4) { ks = 4; nt = 256; }
  else { ks = 16; nt = 256; }
}

struct Args {
  const void* hyps;                  // (pairs, N)
  const void* refs;                  // (pairs / per_ref, M)
  const void* hyp_len;               // (pairs,) or null: N
  const void* ref_len;               // (pairs / per_ref,) or null: M
  int64_t pairs, per_ref, N, M;
  int32_t hyp64, ref64, hlen64, rlen64, ops;
  int32_t* out;                      // (pairs,) or (pairs, 4)
};

AAMD_HD int64_t read_int(const void* p, int64_t i, int is64) {
  return is64 ? static_cast<const int64_t*>(p)[i] : (int64_t) static_cast<const int32_t*>(p)[i];
}

struct Geom {
  int64_t pair, ref;
  int Nb, Mb;
};

AAMD_HD bool lens_ok(const Args& a, int64_t pair, Geom& g) {
  g.pair = pair;
  g.ref = pair / a.per_ref;
  const int64_t nb = a.hyp_len ? read_int(a.hyp_len, g.pair, a.hlen64) : a.N;
  const int64_t mb = a.ref_len ? read_int(a.ref_len, g.ref, a.rlen64) : a.M;
  const bool ok = nb >= 0 && nb <= a.N && mb >= 0 && mb <= a.M;
  g.Nb = ok ? (int)nb : 0;
  g.Mb = ok ? (int)mb : 0;
  return ok;
}

AAMD_HD uint64_t pack(uint64_t cost, uint64_t s, uint64_t d, uint64_t i) { return cost << 48 | s << 32 | d << 16 | i; }
AAMD_HD uint64_t row0_cell(int j) { return pack((uint64_t)j, 0, 0, (uint64_t)j); }     // cell (0, j)
AAMD_HD uint64_t col0_cell(int i) { return pack((uint64_t)i, 0, (uint64_t)i, 0); }     // cell (i, 0)

AAMD_HD void write_result(const Args& a, int64_t pair, uint64_t cell) {
  if (a.ops) {
    AAMD_UNROLL
    for (int f = 0; f < 4; ++f) a.out[pair * 4 + f] = (int32_t)((cell >> (48 - 16 * f)) & 0xffffu);
  } else {
    a.out[pair] = (int32_t)(cell >> 48);
  }
}
AAMD_HD void write_bad(const Args& a, int64_t pair) {
  if (a.ops) {
    AAMD_UNROLL
    for (int f = 0; f < 4; ++f) a.out[pair * 4 + f] = -1;
  } else {
    a.out[pair] = -1;
  }
}

// hypothesis token t of the pair; 0 beyond its length (no lane works on such a column)
AAMD_HD int64_t hyp_token(const Args& a, const Geom& g, int64_t t) {
  return t < g.Nb ? read_int(a.hyps, g.pair * a.N + t, a.hyp64) : 0;
}

template <int KS>
struct Lane {
  int64_t ref[KS];                   // reference positions tid * KS + k
  uint64_t col[KS];                  // cells (tid * KS + 1 + k, j - 1): the lane's previous column
  uint64_t diag;                     // cell (tid * KS, j - 1): what the lane took from above a step earlier
};

template <int KS>
AAMD_HD void lane_setup(const Args& a, const Geom& g, int tid, Lane<KS>& s) {
  AAMD_UNROLL
  for (int k = 0; k < KS; ++k) {
    const int i = tid * KS + k;
    s.ref[k] = i < g.Mb ? read_int(a.refs, g.ref * a.M + i, a.ref64) : 0;
    s.col[k] = col0_cell(i + 1);
  }
  s.diag = col0_cell(tid * KS);
}

// the lane whose rows hold the pair's last one, and the steps the wavefront takes to finish there
AAMD_HD int last_lane(const Geom& g, int ks) { return (g.Mb - 1) / ks; }
AAMD_HD int total_steps(const Geom& g, int ks) { return g.Nb + last_lane(g, ks); }
AAMD_HD bool active(const Geom& g, int ks, int tid, int j) { return j >= 1 && j <= g.Nb && tid <= last_lane(g, ks); }

// column j of the lane's rows, in place; top = cell (tid * KS, j), tok = h[j - 1]
template <int KS>
AAMD_HD void step(Lane<KS>& s, uint64_t top, int64_t tok) {
  uint64_t dg = s.diag, up = top;
  AAMD_UNROLL
  for (int k = 0; k < KS; ++k) {
    const uint64_t left = s.col[k];
    uint64_t best = dg + (s.ref[k] != tok ? kSub : 0ull);
    const uint64_t del = up + kDel, ins = left + kIns;
    if ((del >> 48) < (best >> 48)) best = del;
    if ((ins >> 48) < (best >> 48)) best = ins;
    s.col[k] = best;
    dg = left;
    up = best;
  }
  s.diag = top;
}

// after the last step: the lane that owns row M_p writes cell (M_p, N_p)
template <int KS>
AAMD_HD void finish(const Args& a, const Geom& g, int tid, const Lane<KS>& s) {
  AAMD_UNROLL
  for (int k = 0; k < KS; ++k)
    if (tid * KS + k + 1 == g.Mb) write_result(a, g.pair, s.col[k]);
}

#if defined(__HIPCC__)
template <int KS, int NT>
__global__ __launch_bounds__(NT) void edit_kernel(Args a) {
  constexpr int WAVES = NT / 64, RING = 2 * NT;
  __shared__ uint64_t line[2][WAVES];                       // the last cell of every wave, by the parity of the step
  __shared__ int64_t ring[RING];                            // hypothesis tokens, token t at t % RING
  const int tid = threadIdx.x;
  Geom g;
  if (!lens_ok(a, blockIdx.x, g)) {                         // the same in every lane
    if (tid == 0) write_bad(a, g.pair);
    return;
  }
  if (g.Mb == 0 || g.Nb == 0) {
    if (tid == 0) write_result(a, g.pair, g.Mb == 0 ? row0_cell(g.Nb) : col0_cell(g.Mb));
    return;
  }
  Lane<KS> s;
  lane_setup<KS>(a, g, tid, s);
  const int total = total_steps(g, KS);
  int64_t next = hyp_token(a, g, tid);
  for (int s0 = 0; s0 < total; s0 += NT) {                  // tokens s0 .. s0 + NT - 1 serve lane 0 in the steps s0 + 1 .. s0 + NT
    ring[(s0 + tid) & (RING - 1)] = next;
    next = hyp_token(a, g, (int64_t)s0 + NT + tid);
    __syncthreads();
    const int s1 = s0 + NT < total ? s0 + NT : total;
    for (int st = s0 + 1; st <= s1; ++st) {
      uint64_t top = __shfl_up(s.col[KS - 1], 1);           // every lane shifts; a lane that is not active ignores it
      if (WAVES > 1 && (tid & 63) == 0 && tid) top = line[(st & 1) ^ 1][(tid >> 6) - 1];
      const int j = st - tid;
      if (tid == 0) top = row0_cell(j);
      if (active(g, KS, tid, j)) step<KS>(s, top, ring[(j - 1) & (RING - 1)]);
      if (WAVES > 1) {                                      // every lane meets every barrier
        if ((tid & 63) == 63) line[st & 1][tid >> 6] = s.col[KS - 1];
        __syncthreads();
      }
    }
  }
  finish<KS>(a, g, tid, s);
}
#endif

}  // namespace ed
}  // namespace aamd
