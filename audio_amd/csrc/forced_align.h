// CTC forced alignment (F.forced_align): the Viterbi path of a transcript through a matrix of log-probabilities.
// log_probs (B, T, C) dense, targets (B, L) int32 / int64, input_lengths / target_lengths (B,) int32 / int64; lengths and labels
// are read on the device.  Example b has the states i = 0 .. 2 L_b (even: blank, odd: targets[b][i / 2]) and
//     alpha_t[i] = max(alpha_{t-1}[i], alpha_{t-1}[i-1], alpha_{t-1}[i-2] if the two labels differ) + lp[t][label(i)]
// with strict comparisons taken in that order (a tie keeps the smaller move), accumulated in float64 for every input type.
//
// forward    One workgroup per example for all T_b steps; nothing waits on another workgroup.  A lane owns the KS consecutive
//            states from tid * KS on: alpha of the previous step lives in its registers, and its columns of log_probs are fixed
//            for the whole call (the blank column once, one column per odd state), so the gathers of step t + kPF are issued
//            while step t is computed -- a register ring whose indices are compile-time constants.  A run starts on an even
//            state, which takes no move 2, so a step needs ONE value from the left neighbour: alpha_{t-1}[tid * KS - 1].  It
//            comes by a one-lane shift inside a wave and, for the first lane of a wave, from a double-buffered LDS line with
//            one barrier per step.  (KS, threads) follow from 2 L + 1 (config()): up to 256 states run on one wave with no
//            barrier at all, up to 1024 as 4 per lane on four waves, up to 4096 as 16 per lane.  The move of every state, 2 bits, is packed into one word per lane and step and stored to the
//            workspace; the final state goes to info[b].  Every lane runs every step, a run without a live state on -inf.
//            An example with T_b outside [1, T], L_b outside [0, L], T_b < L_b + (adjacent equal labels), or a live label
//            outside [0, C) or equal to blank is flagged (info[b] = -1) and nothing is indexed with those values.
// backtrack  Second launch, one workgroup per example.  The state falls by at most 2 per frame, so the moves that kBT frames
//            below state s can need lie in a triangle of words: all lanes fetch it with independent loads into LDS, one lane
//            walks kBT frames out of LDS, then all lanes write paths and copy the scores element for element (bit for bit).
//            A move is clamped to min(2, state), so no value of the workspace takes the walk below state 0.  Padding frames
//            get blank / 0, a flagged example -1 / NaN over its whole row.
//
// The phase functions are AAMD_HD: tests/cpu_sim/sim_forced_align.cpp replays them with g++.
#pragma once
#include "hd.h"
#include "wave_augment.h"   // wa::Elem (storage / compute types of the four dtypes)

#if !defined(AAMD_UNROLL)
#if defined(__HIPCC__)
#define AAMD_UNROLL _Pragma("unroll")
#else
#define AAMD_UNROLL
#endif
#endif

namespace aamd {
namespace fa {

constexpr int kPF = 4;               // steps the forward's gathers run ahead
constexpr int kBT = 64;              // frames per backtrack block
constexpr int kBtThreads = 256;      // backtrack workgroup
constexpr int kMaxL = 2047;          // 2 L + 1 <= 256 lanes x 16 states
constexpr int kMinKS = 4;
constexpr int kTriPitch = 64;            // row pitch of the triangle in LDS: a power of two >= 2 * kBT / kMinKS + 2 words

AAMD_HD double neg_inf() { return -__builtin_inf(); }

// states per lane and lanes per workgroup for transcripts of up to L labels
AAMD_HD void config(int64_t L, int& ks, int& nt) {
  const int64_t states = 2 * L + 1;
  if (states <= 64 * 4) { ks = 4; nt = 64; }
  else if (states <= 256 * 4) { ks = 4; nt = 256; }
  else { ks = 16; nt = 256; }
}

struct Args {
  const void* lp;                    // (B, T, C)
  const void* targets;               // (B, L) int32 or int64
  const void* in_len;                // (B,) int32 or int64
  const void* tg_len;
  int64_t B, T, C, L;
  int32_t blank, tgt64, len64, dtype;
  int32_t ks, nt, ks_shift;          // config(L); ks = 1 << ks_shift
  // workspace
  int32_t* info;                     // (B,): the final state, -1 for a flagged example
  uint8_t* moves;                    // (B, T, nt) words of ks / 4 bytes; row 0 of an example is not used
  void* paths;                       // (B, T) as targets
  void* scores;                      // (B, T) as lp
};

AAMD_HD int64_t info_bytes(int64_t B) { return (B * 4 + 15) / 16 * 16; }
AAMD_HD int64_t ws_bytes(int64_t B, int64_t T, int64_t L) {
  int ks, nt;
  config(L, ks, nt);
  return info_bytes(B) + B * T * nt * (ks / 4);
}
AAMD_HD void ws_bind(Args& a, void* ws) {
  config(a.L, a.ks, a.nt);
  a.ks_shift = a.ks == 4 ? 2 : 4;
  a.info = static_cast<int32_t*>(ws);
  a.moves = static_cast<uint8_t*>(ws) + info_bytes(a.B);
}

AAMD_HD int64_t read_int(const void* p, int64_t i, int is64) {
  return is64 ? static_cast<const int64_t*>(p)[i] : (int64_t) static_cast<const int32_t*>(p)[i];
}

struct Geom {
  int64_t b;
  int Tb, Lb;
};

AAMD_HD bool lens_ok(const Args& a, int64_t b, Geom& g) {
  const int64_t tb = read_int(a.in_len, b, a.len64), lb = read_int(a.tg_len, b, a.len64);
  g.b = b;
  g.Tb = (int)tb;
  g.Lb = (int)lb;
  return tb >= 1 && tb <= a.T && lb >= 0 && lb <= a.L;
}

// lanes share the scan of the live labels: one outside [0, C) or equal to blank, and the number of adjacent equal pairs
AAMD_HD void scan_labels(const Args& a, const Geom& g, int tid, int nt, int& bad, int& rep) {
  bad = rep = 0;
  for (int u = tid; u < g.Lb; u += nt) {
    const int64_t v = read_int(a.targets, g.b * a.L + u, a.tgt64);
    if (v < 0 || v >= a.C || v == a.blank) bad = 1;
    if (u >= 1 && v == read_int(a.targets, g.b * a.L + u - 1, a.tgt64)) ++rep;
  }
}

template <int DT, int KS>
struct Lane {
  double alpha[KS];
  typename wa::Elem<DT>::S ring[kPF][KS / 2 + 1];   // [.][0]: the blank column, [.][1 + m]: the column of state 2 m + 1 of the run
  int32_t col[KS / 2];
  uint32_t skip;                     // bit k: state tid * KS + k may take move 2
};

template <int DT, int KS>
AAMD_HD void lane_setup(const Args& a, const Geom& g, int tid, Lane<DT, KS>& s) {
  const int j0 = tid * (KS / 2);                             // the label of the run's first odd state
  s.skip = 0;
  AAMD_UNROLL
  for (int k = 0; k < KS; ++k) s.alpha[k] = neg_inf();
  AAMD_UNROLL
  for (int m = 0; m < KS / 2; ++m) {
    const int j = j0 + m;
    s.col[m] = a.blank;                                      // a dead state gathers the blank column; nothing reads its alpha
    if (j < g.Lb) {
      const int64_t v = read_int(a.targets, g.b * a.L + j, a.tgt64);
      s.col[m] = (int32_t)v;
      if (j >= 1 && v != read_int(a.targets, g.b * a.L + j - 1, a.tgt64)) s.skip |= 1u << (2 * m + 1);
    }
  }
}

// the gathers of step t into slot j of the ring.  No branch stands round a load -- a step past the last frame gathers the last
// frame again and a run without a live state the blank column -- so the waits on the ring are counted, not drained.
template <int DT, int KS>
AAMD_HD void fetch(const Args& a, const Geom& g, int64_t t, int j, Lane<DT, KS>& s) {
  const int64_t tc = t < g.Tb ? t : g.Tb - 1;
  const typename wa::Elem<DT>::S* row = static_cast<const typename wa::Elem<DT>::S*>(a.lp) + (g.b * a.T + tc) * a.C;
  s.ring[j][0] = row[a.blank];
  AAMD_UNROLL
  for (int m = 0; m < KS / 2; ++m) s.ring[j][1 + m] = row[s.col[m]];
}

template <int DT, int KS>
AAMD_HD double ring_value(const Lane<DT, KS>& s, int j, int k) {
  return (double)wa::Elem<DT>::load(s.ring[j][(k & 1) ? 1 + k / 2 : 0]);
}

// alpha of state k of the run; k = -1: the left neighbour's last state
template <int DT, int KS>
AAMD_HD double alpha_at(const Lane<DT, KS>& s, int k, double left) {
  return k >= 0 ? s.alpha[k >= 0 ? k : 0] : left;
}

// t = 0 (slot 0 of the ring): states 0 and 1 are live
template <int DT, int KS>
AAMD_HD void first_step(const Args& a, const Geom& g, int tid, Lane<DT, KS>& s) {
  if (tid == 0) {
    s.alpha[0] = ring_value(s, 0, 0);
    if (g.Lb > 0) s.alpha[1] = ring_value(s, 0, 1);
  }
  fetch<DT, KS>(a, g, kPF, 0, s);
}

// t >= 1, in place from the run's last state down; left = alpha_{t-1}[tid * KS - 1].  Returns the run's moves, 2 bits each.
template <int DT, int KS>
AAMD_HD uint32_t step(int j, double left, Lane<DT, KS>& s) {
  uint32_t word = 0;
  AAMD_UNROLL
  for (int k = KS - 1; k >= 0; --k) {
    const double x1 = alpha_at(s, k - 1, left);
    double best = s.alpha[k];
    uint32_t mv = 0;
    if (x1 > best) { best = x1; mv = 1; }
    if (k & 1) {
      const double x2 = alpha_at(s, k - 2, left);
      if (((s.skip >> k) & 1u) && x2 > best) { best = x2; mv = 2; }
    }
    s.alpha[k] = best + ring_value(s, j, k);
    word |= mv << (2 * k);
  }
  return word;
}

template <int KS>
AAMD_HD void store_moves(const Args& a, const Geom& g, int64_t t, int tid, uint32_t word) {
  const int64_t at = (g.b * a.T + t) * a.nt + tid;
  if (KS == 4) a.moves[at] = (uint8_t)word;
  else reinterpret_cast<uint32_t*>(a.moves)[at] = word;
}

// frame t >= 1 out of slot j: the step, its word of moves, and the gathers of frame t + kPF into the slot it has emptied
template <int DT, int KS>
AAMD_HD void advance(const Args& a, const Geom& g, int64_t t, int j, int tid, double left, Lane<DT, KS>& s) {
  store_moves<KS>(a, g, t, tid, step<DT, KS>(j, left, s));
  fetch<DT, KS>(a, g, t + kPF, j, s);
}

// after the last step: the lane that owns state 2 L_b decides the final state
template <int DT, int KS>
AAMD_HD void finish(const Args& a, const Geom& g, int tid, double left, const Lane<DT, KS>& s) {
  AAMD_UNROLL
  for (int k = 0; k < KS; k += 2) {
    if (tid * KS + k != 2 * g.Lb) continue;
    const double prev = alpha_at(s, k - 1, left);
    a.info[g.b] = (g.Lb > 0 && !(s.alpha[k] > prev)) ? 2 * g.Lb - 1 : 2 * g.Lb;
  }
}

#if defined(__HIPCC__)
template <int DT, int KS, int NT>
__global__ __launch_bounds__(NT) void forward_kernel(Args a) {
  constexpr int WAVES = NT / 64;
  __shared__ double line[2][WAVES];                         // alpha of the last state of every wave, by the parity of the step
  __shared__ int s_bad, s_rep;
  const int tid = threadIdx.x;
  Geom g;
  const bool ok = lens_ok(a, blockIdx.x, g);
  if (tid == 0) s_bad = s_rep = 0;
  __syncthreads();
  if (ok) {
    int bad, rep;
    scan_labels(a, g, tid, NT, bad, rep);
    if (bad) atomicOr(&s_bad, 1);
    if (rep) atomicAdd(&s_rep, rep);
  }
  __syncthreads();
  if (!ok || s_bad || g.Tb < g.Lb + s_rep) {                // the same in every lane
    if (tid == 0) a.info[g.b] = -1;
    return;
  }
  Lane<DT, KS> s;
  lane_setup<DT, KS>(a, g, tid, s);
  AAMD_UNROLL
  for (int j = 0; j < kPF; ++j) fetch<DT, KS>(a, g, j, j, s);
  auto left_of = [&](int64_t t) {                           // alpha_{t-1}[tid * KS - 1]; every lane calls it
    double l = __shfl_up(s.alpha[KS - 1], 1);
    if (WAVES > 1 && (tid & 63) == 0 && tid) l = line[(t & 1) ^ 1][(tid >> 6) - 1];
    return tid ? l : neg_inf();
  };
  auto publish = [&](int64_t t) {                           // every lane meets every barrier
    if (WAVES > 1) {
      if ((tid & 63) == 63) line[t & 1][tid >> 6] = s.alpha[KS - 1];
      __syncthreads();
    }
  };
  first_step<DT, KS>(a, g, tid, s);
  publish(0);
  int64_t t0 = 1;
  for (; t0 + kPF <= g.Tb; t0 += kPF) {                     // whole groups: straight-line code, frame t in slot t % kPF
    AAMD_UNROLL
    for (int j = 0; j < kPF; ++j) {
      const int64_t t = t0 + j;
      advance<DT, KS>(a, g, t, (1 + j) % kPF, tid, left_of(t), s);
      publish(t);
    }
  }
  AAMD_UNROLL
  for (int j = 0; j < kPF - 1; ++j) {                       // the last kPF - 1 frames at most; T_b is the same in every lane
    const int64_t t = t0 + j;
    if (t < g.Tb) {
      advance<DT, KS>(a, g, t, (1 + j) % kPF, tid, left_of(t), s);
      publish(t);
    }
  }
  finish<DT, KS>(a, g, tid, left_of(g.Tb), s);
}
#endif

// ---- backtrack ------------------------------------------------------------------------------------------------------------------
AAMD_HD uint32_t load_word(const Args& a, int64_t b, int64_t t, int w) {
  const int64_t at = (b * a.T + t) * a.nt + w;
  return a.ks == 4 ? (uint32_t)a.moves[at] : reinterpret_cast<const uint32_t*>(a.moves)[at];
}
AAMD_HD int tri_width(const Args& a) { return ((2 * kBT) >> a.ks_shift) + 2; }

AAMD_HD void put_path(const Args& a, int64_t at, int64_t v) {
  if (a.tgt64) static_cast<int64_t*>(a.paths)[at] = v;
  else static_cast<int32_t*>(a.paths)[at] = (int32_t)v;
}
// kind 0: zero, 1: NaN, 2: the element at src, copied as bits
AAMD_HD void put_score(const Args& a, int64_t at, int kind, int64_t src) {
  if (a.dtype == wa::kF64) {
    uint64_t* o = static_cast<uint64_t*>(a.scores);
    o[at] = kind == 2 ? static_cast<const uint64_t*>(a.lp)[src] : (kind ? 0x7ff8000000000000ull : 0ull);
  } else if (a.dtype == wa::kF32) {
    uint32_t* o = static_cast<uint32_t*>(a.scores);
    o[at] = kind == 2 ? static_cast<const uint32_t*>(a.lp)[src] : (kind ? 0x7fc00000u : 0u);
  } else {
    uint16_t* o = static_cast<uint16_t*>(a.scores);
    o[at] = kind == 2 ? static_cast<const uint16_t*>(a.lp)[src] : (uint16_t)(kind ? (a.dtype == wa::kF16 ? 0x7e00 : 0x7fc0) : 0);
  }
}

// a flagged example: -1 / NaN over the whole row; otherwise the frames from T_b on: blank / 0
AAMD_HD void bt_fill(const Args& a, int64_t b, int64_t from, bool bad, int tid) {
  for (int64_t t = from + tid; t < a.T; t += kBtThreads) {
    put_path(a, b * a.T + t, bad ? -1 : a.blank);
    put_score(a, b * a.T + t, bad ? 1 : 0, 0);
  }
}

// the words that the frames t_hi - d, d < kBT, can need below state s: row d holds the words whi, whi - 1, ... down to the
// one of state max(0, s - 2 d), at tri[d * kTriPitch + (whi - w)].  Frame 0 has no move.  (Shifts and masks throughout: the walk
// below is one lane's dependent chain, and a division by a run-time ks would be most of it.)
AAMD_HD void bt_fetch(const Args& a, int64_t b, int64_t t_hi, int s, int tid, uint32_t* tri) {
  const int tw = tri_width(a), whi = s >> a.ks_shift;
  for (int e = tid; e < kBT * kTriPitch; e += kBtThreads) {
    const int d = e / kTriPitch, c = e % kTriPitch;
    const int64_t t = t_hi - d;
    const int lo = s - 2 * d > 0 ? s - 2 * d : 0;
    const int w = whi - c;
    if (c < tw && t >= 1 && w >= (lo >> a.ks_shift)) tri[e] = load_word(a, b, t, w);
  }
}

// one lane: the states of the frames t_hi, t_hi - 1, ... into states[]; returns how many, and s becomes the state of the frame
// below them
AAMD_HD int bt_walk(const Args& a, int64_t t_hi, int& s, const uint32_t* tri, int* states) {
  const int whi = s >> a.ks_shift;
  int d = 0;
  for (; d < kBT && t_hi - d >= 0; ++d) {
    states[d] = s;
    if (t_hi - d == 0) { ++d; break; }
    const uint32_t word = tri[d * kTriPitch + (whi - (s >> a.ks_shift))];
    const int mv = (int)((word >> (2 * (s & (a.ks - 1)))) & 3u);
    const int cap = s < 2 ? s : 2;
    s -= mv < cap ? mv : cap;
  }
  return d;
}

AAMD_HD void bt_write(const Args& a, int64_t b, int64_t t_hi, int n, const int* states, int tid) {
  for (int d = tid; d < n; d += kBtThreads) {
    const int64_t t = t_hi - d;
    const int st = states[d];
    const int64_t label = (st & 1) ? read_int(a.targets, b * a.L + st / 2, a.tgt64) : (int64_t)a.blank;
    put_path(a, b * a.T + t, label);
    put_score(a, b * a.T + t, 2, (b * a.T + t) * a.C + label);
  }
}

#if defined(__HIPCC__)
__global__ __launch_bounds__(kBtThreads) void backtrack_kernel(Args a) {
  __shared__ uint32_t tri[kBT * kTriPitch];
  __shared__ int states[kBT];
  __shared__ int s_state, s_count;
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  const int fin = a.info[b];
  if (fin < 0) {                                            // the same in every lane
    bt_fill(a, b, 0, true, tid);
    return;
  }
  Geom g;
  lens_ok(a, b, g);
  bt_fill(a, b, g.Tb, false, tid);
  int s = fin;
  for (int64_t t_hi = g.Tb - 1; t_hi >= 0; t_hi -= kBT) {
    bt_fetch(a, b, t_hi, s, tid, tri);
    __syncthreads();
    if (tid == 0) {
      int st = s;
      s_count = bt_walk(a, t_hi, st, tri, states);
      s_state = st;
    }
    __syncthreads();
    s = s_state;
    bt_write(a, b, t_hi, s_count, states, tid);
    __syncthreads();                                        // states[] and tri[] are rewritten by the next block
  }
}
#endif

}  // namespace fa
}  // namespace aamd
