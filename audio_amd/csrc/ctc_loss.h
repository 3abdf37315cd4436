// CTC loss (F.ctc_loss, T.CTCLoss).  x (T, N, V) raw logits (fused log-softmax) or log-probabilities, read in place through
// its time and batch strides (unit class stride); targets (N, S) padded or 1-D concatenated, int32 / int64; input_lengths /
// target_lengths (N,) int32 / int64.  Lengths and labels are read on the device.  Example b has the states s = 0 .. 2 S_b
// (even: blank, odd: targets[b][s / 2]) and, in float64 log space for every input type,
//     alpha_t[s] = lp_t[label(s)] + log(e^alpha_{t-1}[s] + e^alpha_{t-1}[s-1] + e^alpha_{t-1}[s-2] if label(s) != label(s-2)),
// lp_t[c] = x[t][b][c] - denom[t][b].  The gradient of both forms is (e^lp - occupancy) * g, as the reference's own backward
// forms it, with denom = 0 when the input holds log-probabilities already.
//
// row      Fused only: ONE streaming read of x.  A team of W lanes (rnnt::team_width) owns one (t, b) row: scalar head and
//          tail, 16-byte body, online (max, sum of exp) per lane, a fixed xor butterfly; lane 0 writes denom[t][b] as float64.
//          Rows with t >= T_b are not read.
// lattice  One workgroup per example and direction; a lane owns the KS consecutive states from tid * KS on (config(): 4
//          states on one wave, 4 on four waves, 16 on four waves), alpha of the previous step in registers.  A run starts on
//          a blank state, so a step needs ONE value from the left neighbour: a one-lane shift inside a wave, a double-buffered
//          LDS line with one barrier per step across waves.  The lane's columns of x are fixed for the call: the gathers of step
//          t + kPF (and the row's denominator) are issued while step t is computed, into a register ring that moves down one
//          slot a step.  DIR 0 (forward): stores alpha_t[s] to the workspace, -log Z is the cost.  DIR 1 (backward): the same
//          recurrence over the lattice reversed in both axes is beta; every step loads alpha_t[s] ahead of its arithmetic and overwrites it
//          with the occupancy gamma_t[s] = exp(alpha + beta - lp - log Z).  It also builds the example's chain of equal labels
//          (first occurrence / next occurrence) once.  A lattice belongs to one workgroup: nothing waits on another one.
//          An example whose T_b is outside [0, T], whose S_b is outside its target row, or with a live label outside [0, V) or
//          equal to blank is flagged (NaN cost, NaN gradient block, nothing indexed with those values); T_b < S_b + (adjacent
//          equal labels) is infeasible (cost inf); T_b = S_b = 0 costs 0.
// reduce   One workgroup: "none" / "sum" / "mean" of the costs in a fixed order, zero_infinity, the result in x's type.
// grad     One streaming read of x and one streaming write of the gradient, rows and vectors as in `row`: exp(x - denom) * g_b
//          with the reduction's factor folded into g_b.  Behind a workgroup barrier the team rewrites the classes that occur
//          in the target: blank from the even states (strided over the team, xor butterfly), each label from its chain in a
//          fixed order -- no atomics.  Padding rows are zeros and a flagged example NaN without reading x.
//
// The phase functions are AAMD_HD.
#pragma once
#include "rnnt_loss.h"      // rnnt::split / ms_add / ms_vecs / ms_combine / team_width / fill_row / row_blocks

namespace aamd {
namespace ctc {

constexpr int kThreads = 256;        // row, gradient and reduction workgroups
constexpr int kPF = 4;               // steps the lattice's gathers run ahead
constexpr int kMaxS = 2047;          // 2 S + 1 <= 256 lanes x 16 states
enum { kOk = 0, kFlagged = 1, kInfeasible = 2, kEmpty = 3 };
enum { kNone = 0, kMean = 1, kSum = 2 };

// states per lane and lanes per workgroup for targets of up to S labels: the configurations of forced_align.h (its header
// defines a kernel that is no template, so it is not included a second time)
AAMD_HD void config(int64_t S, int& ks, int& nt) {
  const int64_t states = 2 * S + 1;
  if (states <= 64 * 4) { ks = 4; nt = 64; }
  else if (states <= 256 * 4) { ks = 4; nt = 256; }
  else { ks = 16; nt = 256; }
}

AAMD_HD int64_t read_int(const void* p, int64_t i, int is64) {
  return is64 ? static_cast<const int64_t*>(p)[i] : (int64_t) static_cast<const int32_t*>(p)[i];
}

struct Args {
  const void* x;                     // (T, N, V)
  int64_t st, sb;                    // strides of x in elements
  const void* targets;               // (N, pitch) or (total,)
  const void* in_len;
  const void* tg_len;
  int64_t N, T, V;
  int64_t S;                         // bound on the target lengths: picks the lattice's configuration
  int64_t pitch;                     // row pitch of padded targets; -1: concatenated
  int64_t total;                     // entries of targets
  int32_t blank, fused, tgt64, len64, reduction, zero_inf;
  // workspace
  double *denom, *logz, *cost, *alpha;   // (T, N); (N,); (N,); T * (2 * total + N): example b's (T, 2 S_b + 1) block at abase
  int64_t* toff;                     // (N,): where example b's labels start
  int32_t *state, *chain;            // (N,); (total,): (next occurrence + 1) * 2 + (first occurrence)
  void* out;                         // forward: (N,) or one element, as x
  // backward
  const double* go;                  // cotangent of out, element b * go_stride
  int64_t go_stride;
  void* grad;                        // (T, N, V) as x, strides gst / gsb
  int64_t gst, gsb;
};

AAMD_HD int64_t ws_doubles(int64_t N, int64_t T, int64_t total) {
  return T * N + 3 * N + (N + 1) / 2 + (total + 1) / 2 + T * (2 * total + N);
}
AAMD_HD void ws_bind(Args& a, void* ws) {
  double* w = static_cast<double*>(ws);
  a.denom = w; w += a.T * a.N;
  a.logz = w; w += a.N;
  a.cost = w; w += a.N;
  a.toff = reinterpret_cast<int64_t*>(w); w += a.N;
  a.state = reinterpret_cast<int32_t*>(w); w += (a.N + 1) / 2;
  a.chain = reinterpret_cast<int32_t*>(w); w += (a.total + 1) / 2;
  a.alpha = w;
}

struct Geom {
  int64_t b, toff, abase;            // abase: start of the example's alpha block
  int Tb, Sb, pitch;                 // pitch = 2 S_b + 1
};

AAMD_HD int64_t clamped_len(const Args& a, int64_t i) {
  const int64_t v = read_int(a.tg_len, i, a.len64);
  return v < 0 ? 0 : (v > a.total ? a.total : v);
}
// true when both lengths can be used as they are
AAMD_HD bool geom(const Args& a, int64_t b, int64_t toff, Geom& g) {
  const int64_t tb = read_int(a.in_len, b, a.len64), sb = read_int(a.tg_len, b, a.len64);
  g.b = b; g.toff = toff; g.abase = a.T * (2 * toff + b);
  g.Tb = (int)tb; g.Sb = (int)sb; g.pitch = 2 * (int)sb + 1;
  return tb >= 0 && tb <= a.T && sb >= 0 && toff >= 0 && (a.pitch >= 0 ? sb <= a.pitch : toff + sb <= a.total);
}
AAMD_HD int64_t label(const Args& a, const Geom& g, int j) { return read_int(a.targets, g.toff + j, a.tgt64); }

// ---- row pass ------------------------------------------------------------------------------------------------------------------------
// a row of T * N is live when its example's T_b is usable and t < T_b
AAMD_HD bool row_live(const Args& a, int64_t row, int64_t& t, int64_t& b) {
  t = row / a.N;
  b = row % a.N;
  const int64_t tb = read_int(a.in_len, b, a.len64);
  return tb <= a.T && t < tb;
}

template <int DT>
AAMD_HD void row_partial(const typename wa::Elem<DT>::S* p, int64_t V, int lane, int W, typename wa::Elem<DT>::C& m,
                         typename wa::Elem<DT>::C& s) {
  using E = wa::Elem<DT>;
  using S = typename E::S;
  using C = typename E::C;
  constexpr int VEC = 16 / (int)sizeof(S);
  const rnnt::Split sp = rnnt::split(p, V, (int)sizeof(S));
  if (lane < sp.h) {
    const C x = E::load(p[lane]);
    rnnt::ms_add<C, 1>(m, s, &x);
  }
  const wa::Vec<S>* q = reinterpret_cast<const wa::Vec<S>*>(p + sp.h);
  int64_t i = lane;
  for (; i + 3 * W < sp.nvec; i += 4 * W) {
    const wa::Vec<S> v[4] = {q[i], q[i + W], q[i + 2 * W], q[i + 3 * W]};
    rnnt::ms_vecs<DT, 4>(m, s, v);
  }
  for (; i < sp.nvec; i += W) {
    const wa::Vec<S> v = q[i];
    rnnt::ms_vecs<DT, 1>(m, s, &v);
  }
  if (lane < sp.tail) {
    const C x = E::load(p[sp.h + sp.nvec * VEC + lane]);
    rnnt::ms_add<C, 1>(m, s, &x);
  }
}

#if defined(__HIPCC__)
template <int DT, int W>
__global__ __launch_bounds__(kThreads) void row_kernel(Args a) {
  using S = typename wa::Elem<DT>::S;
  using C = typename wa::Elem<DT>::C;
  constexpr int RPB = kThreads / W;
  const int lane = threadIdx.x % W, team = threadIdx.x / W;
  const int64_t rows = a.T * a.N;
  for (int64_t r0 = (int64_t)blockIdx.x * RPB; r0 < rows; r0 += (int64_t)gridDim.x * RPB) {
    const int64_t row = r0 + team;
    int64_t t = 0, b = 0;
    const bool live = row < rows && row_live(a, row, t, b);               // the same for every lane of a team
    C m = rnnt::neg_inf<C>(), s = C(0);
    if (live) row_partial<DT>(static_cast<const S*>(a.x) + t * a.st + b * a.sb, a.V, lane, W, m, s);
    AAMD_UNROLL
    for (int o = 1; o < W; o *= 2) {
      const C m2 = __shfl_xor(m, o, W), s2 = __shfl_xor(s, o, W);
      rnnt::ms_combine<C>(m, s, m2, s2);
    }
    if (live && lane == 0) a.denom[row] = (double)(m + rnnt::xlog(s));
  }
}
#endif

// ---- lattice -------------------------------------------------------------------------------------------------------------------------
AAMD_HD double ninf() { return -__builtin_inf(); }
// log(e^x0 + e^x1 + e^x2); all -inf: -inf, and a NaN stays one
AAMD_HD double lse3(double x0, double x1, double x2) {
  double m = x1 > x0 ? x1 : x0;
  m = x2 > m ? x2 : m;
  if (m == ninf()) return x0 + x1 + x2;
  return m + log(exp(x0 - m) + exp(x1 - m) + exp(x2 - m));
}
AAMD_HD double lse2(double x0, double x1) {
  const double m = x1 > x0 ? x1 : x0;
  if (m == ninf()) return x0 + x1;
  return m + log(exp(x0 - m) + exp(x1 - m));
}

template <int DT, int KS>
struct Lane {
  double alpha[KS];
  typename wa::Elem<DT>::S ring[kPF][KS / 2 + 1];   // [.][0]: the blank column, [.][1 + m]: the column of state 2 m + 1 of the run
  double den[kPF];
  int32_t col[KS / 2];
  uint32_t skip;                     // bit k: state tid * KS + k may be entered from two states below
};

// the label of odd state 2 j + 1 in the direction's own coordinates
template <int DIR>
AAMD_HD int64_t dir_label(const Args& a, const Geom& g, int j) { return label(a, g, DIR ? g.Sb - 1 - j : j); }

// lanes share the scan of the live labels: one outside [0, V) or equal to blank, and the number of adjacent equal pairs
AAMD_HD void scan_labels(const Args& a, const Geom& g, int tid, int nt, int& bad, int& rep) {
  bad = rep = 0;
  for (int j = tid; j < g.Sb; j += nt) {
    const int64_t v = label(a, g, j);
    if (v < 0 || v >= a.V || v == a.blank) bad = 1;
    if (j >= 1 && v == label(a, g, j - 1)) ++rep;
  }
}

// the step before the first frame: all mass on state 0, which frame 0 moves to the states 0 and 1
template <int DT, int KS, int DIR>
AAMD_HD void lane_setup(const Args& a, const Geom& g, int tid, Lane<DT, KS>& s) {
  s.skip = 0;
  AAMD_UNROLL
  for (int k = 0; k < KS; ++k) s.alpha[k] = ninf();
  if (tid == 0) s.alpha[0] = 0.0;
  AAMD_UNROLL
  for (int m = 0; m < KS / 2; ++m) {
    const int j = tid * (KS / 2) + m;
    s.col[m] = a.blank;                                      // a dead state gathers the blank column; nothing stores its alpha
    if (j < g.Sb) {
      const int64_t v = dir_label<DIR>(a, g, j);
      s.col[m] = (int32_t)v;
      if (j >= 1 && v != dir_label<DIR>(a, g, j - 1)) s.skip |= 1u << (2 * m + 1);
    }
  }
}

// the frame of x that step t of the direction reads; steps past the last one read the last frame again
template <int DIR>
AAMD_HD int64_t frame_of(const Geom& g, int64_t t) {
  const int64_t tc = t < g.Tb ? t : g.Tb - 1;
  return DIR ? g.Tb - 1 - tc : tc;
}

// the gathers of step t into slot j of the ring; no branch stands round a load
template <int DT, int KS, int DIR>
AAMD_HD void fetch(const Args& a, const Geom& g, int64_t t, int j, Lane<DT, KS>& s) {
  const int64_t tr = frame_of<DIR>(g, t);
  const typename wa::Elem<DT>::S* row = static_cast<const typename wa::Elem<DT>::S*>(a.x) + tr * a.st + g.b * a.sb;
  s.ring[j][0] = row[a.blank];
  AAMD_UNROLL
  for (int m = 0; m < KS / 2; ++m) s.ring[j][1 + m] = row[s.col[m]];
  s.den[j] = a.fused ? a.denom[tr * a.N + g.b] : 0.0;
}

template <int DT, int KS>
AAMD_HD double lp_of(const Lane<DT, KS>& s, int j, int k) {
  return (double)wa::Elem<DT>::load(s.ring[j][(k & 1) ? 1 + k / 2 : 0]) - s.den[j];
}

// one frame out of slot j, in place from the run's last state down; left = the previous step's alpha of state tid * KS - 1
template <int DT, int KS>
AAMD_HD void step(int j, double left, Lane<DT, KS>& s) {
  AAMD_UNROLL
  for (int k = KS - 1; k >= 0; --k) {
    const double x1 = k >= 1 ? s.alpha[k >= 1 ? k - 1 : 0] : left;
    double v;
    if (k & 1) {
      const double x2 = k >= 2 ? s.alpha[k >= 2 ? k - 2 : 0] : left;
      v = lse3(s.alpha[k], x1, ((s.skip >> k) & 1u) ? x2 : ninf());
    } else {
      v = lse2(s.alpha[k], x1);
    }
    s.alpha[k] = v + lp_of(s, j, k);
  }
}

// step t of the direction out of slot 0: DIR 0 keeps alpha_t, DIR 1 turns the stored alpha_t into the occupancy.  Then the ring
// moves down one slot and the gathers of step t + kPF go into the last one.  (The ring is rotated, not indexed by t % kPF in
// an unrolled group of steps as in forced_align.h: a step is 2 .. 3 float64 exponentials and a logarithm per state, and kPF
// copies of that body would not fit the instruction cache; the moves are noise beside it.)
template <int DT, int KS, int DIR>
AAMD_HD void advance(const Args& a, const Geom& g, int64_t t, int tid, double left, double logz, Lane<DT, KS>& s) {
  double* at = a.alpha + g.abase + frame_of<DIR>(g, t) * g.pitch;
  const int s0 = tid * KS, last = 2 * g.Sb;
  double al[DIR ? KS : 1];
  if (DIR) {                                                 // issued ahead of the step's arithmetic
    AAMD_UNROLL
    for (int k = 0; k < KS; ++k) al[k] = s0 + k <= last ? at[last - s0 - k] : 0.0;
  }
  step<DT, KS>(0, left, s);
  AAMD_UNROLL
  for (int k = 0; k < KS; ++k) {
    if (s0 + k > last) continue;
    if (DIR) at[last - s0 - k] = exp(al[k] + s.alpha[k] - lp_of(s, 0, k) - logz);
    else at[s0 + k] = s.alpha[k];
  }
  AAMD_UNROLL
  for (int j = 0; j + 1 < kPF; ++j) {
    AAMD_UNROLL
    for (int m = 0; m < KS / 2 + 1; ++m) s.ring[j][m] = s.ring[j + 1][m];
    s.den[j] = s.den[j + 1];
  }
  fetch<DT, KS, DIR>(a, g, t + kPF, kPF - 1, s);
}

// after the last step: the lane that owns state 2 S_b holds log Z with its left neighbour's state
template <int DT, int KS>
AAMD_HD void finish(const Args& a, const Geom& g, int tid, double left, const Lane<DT, KS>& s) {
  AAMD_UNROLL
  for (int k = 0; k < KS; k += 2) {
    if (tid * KS + k != 2 * g.Sb) continue;
    const double prev = k >= 1 ? s.alpha[k >= 1 ? k - 1 : 0] : left;
    const double z = g.Sb > 0 ? lse2(s.alpha[k], prev) : s.alpha[k];
    a.logz[g.b] = z;
    a.cost[g.b] = -z;
  }
}

// label j's entry of the chain: the next occurrence of the same label and whether j is the first one
AAMD_HD int32_t chain_entry(const Args& a, const Geom& g, int j) {
  const int64_t v = label(a, g, j);
  int next = -1, first = 1;
  for (int i = j + 1; i < g.Sb && next < 0; ++i)
    if (label(a, g, i) == v) next = i;
  for (int i = j - 1; i >= 0 && first; --i)
    if (label(a, g, i) == v) first = 0;
  return (next + 1) * 2 + first;
}

#if defined(__HIPCC__)
template <int DT, int KS, int NT, int DIR>
__global__ __launch_bounds__(NT) void lattice_kernel(Args a) {
  constexpr int WAVES = NT / 64;
  __shared__ double line[2][WAVES];                         // alpha of the last state of every wave, by the parity of the step
  __shared__ int s_bad, s_rep;
  __shared__ unsigned long long s_off;
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  Geom g;
  if (DIR == 0) {
    if (tid == 0) {
      s_bad = s_rep = 0;
      s_off = 0;
    }
    __syncthreads();
    if (a.pitch < 0) {                                       // concatenated targets start at the sum of the lengths before
      unsigned long long part = 0;
      for (int64_t i = tid; i < b; i += NT) part += (unsigned long long)clamped_len(a, i);
      if (part) atomicAdd(&s_off, part);
    }
    __syncthreads();
    const bool ok = geom(a, b, a.pitch < 0 ? (int64_t)s_off : b * a.pitch, g);
    if (ok) {
      int bad, rep;
      scan_labels(a, g, tid, NT, bad, rep);
      if (bad) atomicOr(&s_bad, 1);
      if (rep) atomicAdd(&s_rep, rep);
    }
    __syncthreads();
    int state = kOk;                                         // the same in every lane
    if (!ok || s_bad) state = kFlagged;
    else if (g.Tb < g.Sb + s_rep || g.Sb > a.S) state = kInfeasible;
    else if (g.Tb == 0) state = kEmpty;
    if (tid == 0) {
      a.state[b] = state;
      a.toff[b] = g.toff;
      if (state != kOk) {
        a.cost[b] = state == kFlagged ? rnnt::nan64() : (state == kEmpty ? 0.0 : -ninf());
        a.logz[b] = -a.cost[b];
      }
    }
    if (state != kOk) return;
  } else {
    if (a.state[b] != kOk) return;
    geom(a, b, a.toff[b], g);
    for (int j = tid; j < g.Sb; j += NT) a.chain[g.toff + j] = chain_entry(a, g, j);
  }
  const double logz = DIR ? a.logz[b] : 0.0;
  Lane<DT, KS> s;
  lane_setup<DT, KS, DIR>(a, g, tid, s);
  AAMD_UNROLL
  for (int j = 0; j < kPF; ++j) fetch<DT, KS, DIR>(a, g, j, j, s);
  auto left_of = [&](int64_t t) {                           // the previous step's alpha of state tid * KS - 1; every lane calls it
    double l = __shfl_up(s.alpha[KS - 1], 1);
    if (WAVES > 1 && (tid & 63) == 0 && tid) l = line[(t & 1) ^ 1][(tid >> 6) - 1];
    return tid ? l : ninf();
  };
  auto publish = [&](int64_t t) {                           // every lane meets every barrier
    if (WAVES > 1) {
      if ((tid & 63) == 63) line[t & 1][tid >> 6] = s.alpha[KS - 1];
      __syncthreads();
    }
  };
  publish(1);                                               // what step 0 reads
#pragma unroll 1
  for (int64_t t = 0; t < g.Tb; ++t) {                      // T_b is the same in every lane
    advance<DT, KS, DIR>(a, g, t, tid, left_of(t), logz, s);
    publish(t);
  }
  if (DIR == 0) finish<DT, KS>(a, g, tid, left_of(g.Tb), s);
}
#endif

// ---- reduction -----------------------------------------------------------------------------------------------------------------------
// example b's term of the reduction
AAMD_HD double reduce_term(const Args& a, int64_t b) {
  double c = a.cost[b];
  if (a.zero_inf && c == -ninf()) c = 0.0;
  if (a.reduction == kMean) {
    const int64_t sb = read_int(a.tg_len, b, a.len64);
    c /= (double)(sb > 1 ? sb : 1);
  }
  return c;
}

#if defined(__HIPCC__)
template <int DT>
__global__ __launch_bounds__(kThreads) void reduce_kernel(Args a) {
  using E = wa::Elem<DT>;
  using C = typename E::C;
  __shared__ double part[kThreads];
  typename E::S* out = static_cast<typename E::S*>(a.out);
  const int tid = threadIdx.x;
  double acc = 0.0;
  for (int64_t b = tid; b < a.N; b += kThreads) {
    const double c = reduce_term(a, b);
    if (a.reduction == kNone) out[b] = E::store((C)c);
    acc += c;
  }
  part[tid] = acc;
  __syncthreads();
  for (int o = kThreads / 2; o > 0; o /= 2) {
    if (tid < o) part[tid] += part[tid + o];
    __syncthreads();
  }
  if (tid == 0 && a.reduction != kNone) out[0] = E::store((C)(a.reduction == kMean ? part[0] / (double)a.N : part[0]));
}
#endif

// ---- gradient ------------------------------------------------------------------------------------------------------------------------
template <int DT>
AAMD_HD typename wa::Elem<DT>::S grad_elem(typename wa::Elem<DT>::S raw, typename wa::Elem<DT>::C den, typename wa::Elem<DT>::C occ,
                                           typename wa::Elem<DT>::C go) {
  using E = wa::Elem<DT>;
  return E::store((rnnt::xexp(E::load(raw) - den) - occ) * go);
}

// exp(x - den) * go over the row, the team's lanes sharing it
template <int DT>
AAMD_HD void grad_dense(const typename wa::Elem<DT>::S* p, typename wa::Elem<DT>::S* out, int64_t V, int lane, int W,
                        typename wa::Elem<DT>::C den, typename wa::Elem<DT>::C go) {
  using S = typename wa::Elem<DT>::S;
  using C = typename wa::Elem<DT>::C;
  constexpr int VEC = 16 / (int)sizeof(S);
  const rnnt::Split sp = rnnt::split(p, V, (int)sizeof(S));
  const bool vec_store = (((uintptr_t)p ^ (uintptr_t)out) & 15) == 0;
  if (lane < sp.h) out[lane] = grad_elem<DT>(p[lane], den, C(0), go);
  const wa::Vec<S>* q = reinterpret_cast<const wa::Vec<S>*>(p + sp.h);
  for (int64_t i = lane; i < sp.nvec; i += W) {
    const wa::Vec<S> v = q[i];
    wa::Vec<S> o;
    AAMD_UNROLL
    for (int k = 0; k < VEC; ++k) o.e[k] = grad_elem<DT>(v.e[k], den, C(0), go);
    S* dst = out + sp.h + i * VEC;
    if (vec_store) {
      *reinterpret_cast<wa::Vec<S>*>(dst) = o;
    } else {
      AAMD_UNROLL
      for (int k = 0; k < VEC; ++k) dst[k] = o.e[k];
    }
  }
  if (lane < sp.tail) {
    const int64_t idx = sp.h + sp.nvec * VEC + lane;
    out[idx] = grad_elem<DT>(p[idx], den, C(0), go);
  }
}

// the factor of example b: its cotangent times the reduction's weight
AAMD_HD double grad_factor(const Args& a, const Geom& g) {
  double go = a.go[g.b * a.go_stride];
  if (a.reduction == kMean) go /= (double)a.N * (double)(g.Sb > 1 ? g.Sb : 1);
  return go;
}

// this lane's share of the blank occupancy of a row: the even states, strided over the team
AAMD_HD double blank_partial(const double* gam, const Geom& g, int lane, int W) {
  double acc = 0.0;
  for (int i = lane; i <= g.Sb; i += W) acc += gam[2 * i];
  return acc;
}

// the labels of the row this lane owns (first occurrences j = lane, lane + W, ...): the occupancy summed along the chain
template <int DT>
AAMD_HD void grad_labels(const Args& a, const Geom& g, const double* gam, const typename wa::Elem<DT>::S* p,
                         typename wa::Elem<DT>::S* out, int lane, int W, typename wa::Elem<DT>::C den, typename wa::Elem<DT>::C go) {
  using C = typename wa::Elem<DT>::C;
  for (int j = lane; j < g.Sb; j += W) {
    int32_t e = a.chain[g.toff + j];
    if (!(e & 1)) continue;
    double acc = 0.0;
    for (int i = j;;) {
      acc += gam[2 * i + 1];
      i = (e >> 1) - 1;
      if (i < 0) break;
      e = a.chain[g.toff + i];
    }
    const int64_t c = label(a, g, j);
    out[c] = grad_elem<DT>(p[c], den, (C)acc, go);
  }
}

#if defined(__HIPCC__)
template <int DT, int W>
__global__ __launch_bounds__(kThreads) void grad_kernel(Args a) {
  using E = wa::Elem<DT>;
  using S = typename E::S;
  using C = typename E::C;
  constexpr int RPB = kThreads / W;
  const int lane = threadIdx.x % W, team = threadIdx.x / W;
  const int64_t rows = a.T * a.N;
  for (int64_t r0 = (int64_t)blockIdx.x * RPB; r0 < rows; r0 += (int64_t)gridDim.x * RPB) {   // every lane meets the barrier
    const int64_t row = r0 + team;
    bool sparse = false;                                     // the same for every lane of a team
    Geom g{};
    const S* p = nullptr;
    S* out = nullptr;
    C den = C(0), go = C(0);
    if (row < rows) {
      const int64_t t = row / a.N, b = row % a.N;
      p = static_cast<const S*>(a.x) + t * a.st + b * a.sb;
      out = static_cast<S*>(a.grad) + t * a.gst + b * a.gsb;
      const int state = a.state[b];
      if (state == kFlagged) {
        rnnt::fill_row<DT>(out, a.V, lane, W, E::store((C)rnnt::nan64()));
      } else {
        geom(a, b, a.toff[b], g);
        if (t >= g.Tb || (state == kInfeasible && a.zero_inf)) {
          rnnt::fill_row<DT>(out, a.V, lane, W, E::store(C(0)));
        } else if (state == kInfeasible) {
          rnnt::fill_row<DT>(out, a.V, lane, W, E::store((C)rnnt::nan64()));
        } else {
          sparse = true;
          den = a.fused ? (C)a.denom[row] : C(0);
          go = (C)grad_factor(a, g);
          grad_dense<DT>(p, out, a.V, lane, W, den, go);
        }
      }
    }
    __syncthreads();                                         // the row is written: the target's classes are rewritten behind it
    const double* gam = a.alpha + g.abase + (row < rows ? row / a.N : 0) * g.pitch;
    double occ = sparse ? blank_partial(gam, g, lane, W) : 0.0;
    AAMD_UNROLL
    for (int o = W / 2; o > 0; o /= 2) occ += __shfl_xor(occ, o, W);
    if (sparse) {
      if (lane == 0) out[a.blank] = grad_elem<DT>(p[a.blank], den, (C)occ, go);
      grad_labels<DT>(a, g, gam, p, out, lane, W, den, go);
    }
  }
}
#endif

}  // namespace ctc
}  // namespace aamd
