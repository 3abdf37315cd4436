// RNN transducer loss (F.rnnt_loss, T.RNNTLoss).  logits (B, T, U1, V) dense with U1 = U + 1, targets (B, U) int32,
// logit_lengths / target_lengths (B,) int32; everything the kernels need of them is read on the device.
//
// row      Forward, fused log-softmax: ONE streaming read of logits.  A team of W lanes (W from V: team_width()) owns one
//          (b, t, u) row of V: each lane keeps an online (max, sum of exp) over its 16-byte vectors -- a row starts at element
//          row * V, so a scalar head and tail are peeled per row and the body is 16 bytes per lane and access whatever the
//          row's residue -- and the lanes are folded by an xor butterfly (a fixed order: two calls give the same bits).  Lane 0
//          writes the denominator and the two log-probabilities the lattice needs (blank, targets[b][u]) as float64.  Rows
//          with t >= T_b or u > U_b are not read.  Not fused: gather_kernel, two loads per live cell and no pass over V.
// lattice  One workgroup per (b, direction), alpha and beta side by side: kLatThreads lanes across u (lat_ku() columns per
//          lane), one anti-diagonal per step, the previous diagonal in LDS (two buffers, one barrier per diagonal), float64
//          throughout.  The log-probabilities of a step do not depend on the recurrence: they are loaded kPF diagonals ahead
//          into a register ring whose indices are compile-time constants.  beta runs as alpha over the reversed lattice.  The
//          cost is -beta[0][0].  A lattice belongs to one workgroup: nothing waits on another workgroup.
//          An example with T_b outside [1, T], U_b outside [0, U] or a live target outside [0, V) is flagged (bad[b]), its cost
//          is NaN and nothing is indexed with those values.
// grad     Backward: one streaming read of logits and one streaming write of the gradient, rows and vectors as in `row`.
//          Per row three float64 scalars (alpha + beta - logZ - denom, and that plus beta[t+1][u] - beta[t][u] /
//          beta[t][u+1] - beta[t][u]), then exp(logit + c) per element in the compute type, the transition terms at blank and
//          at the target, the clamp, and the factor grad_costs[b].  Padding rows are written as zeros and a flagged example as
//          NaN without reading logits.
//
// The phase functions are AAMD_HD: tests/cpu_sim/sim_rnnt_loss.cpp replays them with g++.
#pragma once
#include "hd.h"
#include "wave_augment.h"   // wa::Elem (storage / compute types of the four dtypes), wa::Vec

#if !defined(__HIPCC__)
#include <limits>
using std::exp;
using std::log1p;
using std::fabs;
#endif

#if !defined(AAMD_UNROLL)
#if defined(__HIPCC__)
#define AAMD_UNROLL _Pragma("unroll")
#else
#define AAMD_UNROLL
#endif
#endif

namespace aamd {
namespace rnnt {

constexpr int kThreads = 256;        // row and gradient passes
constexpr int kLatThreads = 256;     // lattice workgroup
constexpr int kMaxKU = 4;            // columns of the lattice per lane
constexpr int kMaxU1 = kLatThreads * kMaxKU;
constexpr int kPF = 4;               // diagonals the lattice's loads run ahead
constexpr int kMinTeam = 8, kMaxTeam = 64;

AAMD_HD float xexp(float x) { return expf(x); }
AAMD_HD double xexp(double x) { return exp(x); }
AAMD_HD float xlog(float x) { return logf(x); }
AAMD_HD double xlog(double x) { return log(x); }

template <typename C> AAMD_HD C neg_inf();
template <> AAMD_HD float neg_inf<float>() { return -__builtin_inff(); }
template <> AAMD_HD double neg_inf<double>() { return -__builtin_inf(); }
AAMD_HD double nan64() { return __builtin_nan(""); }

struct Args {
  const void* logits;
  const int32_t* targets;            // (B, U1 - 1)
  const int32_t* logit_lengths;
  const int32_t* target_lengths;
  int64_t B, T, U1, V;
  int32_t blank, fused;
  // workspace, (B, T, U1) float64 each and one flag per example
  double *denom, *lpb, *lpt, *alpha, *beta;
  int32_t* bad;
  double* costs;                     // (B,), forward
  // backward
  double clamp;
  const double* grad_costs;          // (B,)
  void* grad;                        // as logits
};

AAMD_HD int64_t cells(int64_t B, int64_t T, int64_t U1) { return B * T * U1; }
AAMD_HD int64_t ws_bytes(int64_t B, int64_t T, int64_t U1) { return (5 * cells(B, T, U1) + (B + 1) / 2) * 8; }
AAMD_HD void ws_bind(Args& a, void* ws) {
  const int64_t n = cells(a.B, a.T, a.U1);
  double* w = static_cast<double*>(ws);
  a.denom = w; a.lpb = w + n; a.lpt = w + 2 * n; a.alpha = w + 3 * n; a.beta = w + 4 * n;
  a.bad = reinterpret_cast<int32_t*>(w + 5 * n);
}

// lanes per row: the narrowest team whose one access per lane covers the row, a whole wave for long rows
AAMD_HD int team_width(int elem_bytes, int64_t V) {
  const int vec = 16 / elem_bytes;
  int w = kMinTeam;
  while (w < kMaxTeam && (int64_t)w * vec < V) w *= 2;
  return w;
}
AAMD_HD int lat_ku(int64_t U1) { return U1 <= kLatThreads ? 1 : (U1 <= 2 * kLatThreads ? 2 : kMaxKU); }

AAMD_HD bool lens_ok(const Args& a, int64_t b, int& Tb, int& Ub) {
  Tb = a.logit_lengths[b];
  Ub = a.target_lengths[b];
  return Tb >= 1 && Tb <= a.T && Ub >= 0 && Ub <= a.U1 - 1;
}

// row = (b * T + t) * U1 + u; live: inside the example's own lattice
AAMD_HD bool row_live(const Args& a, int64_t row, int64_t& b, int& t, int& u, int& Tb, int& Ub) {
  u = (int)(row % a.U1);
  const int64_t bt = row / a.U1;
  t = (int)(bt % a.T);
  b = bt / a.T;
  return lens_ok(a, b, Tb, Ub) && t < Tb && u <= Ub;
}
// the label of a live cell with u < U_b, or -1 when it lies outside [0, V)
AAMD_HD int target_at(const Args& a, int64_t b, int u) {
  const int32_t k = a.targets[b * (a.U1 - 1) + u];
  return k >= 0 && k < a.V ? k : -1;
}

// ---- a row of V elements at p as scalar head, 16-byte body, scalar tail ----------------------------------------------------------
struct Split {
  int h, tail;
  int64_t nvec;
};
AAMD_HD Split split(const void* p, int64_t V, int es) {
  const int vec = 16 / es;
  Split s;
  const int64_t h = (int64_t)(((16 - ((uintptr_t)p & 15)) & 15) / es);
  s.h = (int)(h < V ? h : V);
  s.nvec = (V - s.h) / vec;
  s.tail = (int)(V - s.h - s.nvec * vec);
  return s;
}

// ---- online (max, sum of exp) ------------------------------------------------------------------------------------------------------
template <typename C, int N>
AAMD_HD void ms_add(C& m, C& s, const C* x) {
  C mx = m;
  AAMD_UNROLL
  for (int k = 0; k < N; ++k) mx = x[k] > mx ? x[k] : mx;
  if (mx == neg_inf<C>()) {                                 // nothing finite yet: only a NaN changes the sum
    AAMD_UNROLL
    for (int k = 0; k < N; ++k)
      if (x[k] != x[k]) s = x[k];
    return;
  }
  C acc = s * xexp(m - mx);
  AAMD_UNROLL
  for (int k = 0; k < N; ++k) acc += xexp(x[k] - mx);
  s = acc;
  m = mx;
}
template <typename C>
AAMD_HD void ms_combine(C& m, C& s, C m2, C s2) {
  const C mx = m2 > m ? m2 : m;
  if (mx == neg_inf<C>()) {
    s = s + s2;
    return;
  }
  s = s * xexp(m - mx) + s2 * xexp(m2 - mx);
  m = mx;
}

template <int DT, int NV>
AAMD_HD void ms_vecs(typename wa::Elem<DT>::C& m, typename wa::Elem<DT>::C& s, const wa::Vec<typename wa::Elem<DT>::S>* v) {
  using E = wa::Elem<DT>;
  constexpr int VEC = 16 / (int)sizeof(typename E::S);
  typename E::C x[NV * VEC];
  AAMD_UNROLL
  for (int j = 0; j < NV; ++j) {
    AAMD_UNROLL
    for (int k = 0; k < VEC; ++k) x[j * VEC + k] = E::load(v[j].e[k]);
  }
  ms_add<typename E::C, NV * VEC>(m, s, x);
}

// lane `lane` of a team of W: its share of the row
template <int DT>
AAMD_HD void row_partial(const Args& a, int64_t row, int lane, int W, typename wa::Elem<DT>::C& m, typename wa::Elem<DT>::C& s) {
  using E = wa::Elem<DT>;
  using S = typename E::S;
  using C = typename E::C;
  constexpr int VEC = 16 / (int)sizeof(S);
  const S* p = static_cast<const S*>(a.logits) + row * a.V;
  const Split sp = split(p, a.V, (int)sizeof(S));
  m = neg_inf<C>();
  s = C(0);
  if (lane < sp.h) {
    const C x = E::load(p[lane]);
    ms_add<C, 1>(m, s, &x);
  }
  const wa::Vec<S>* q = reinterpret_cast<const wa::Vec<S>*>(p + sp.h);
  int64_t i = lane;
  for (; i + 3 * W < sp.nvec; i += 4 * W) {
    const wa::Vec<S> v[4] = {q[i], q[i + W], q[i + 2 * W], q[i + 3 * W]};
    ms_vecs<DT, 4>(m, s, v);
  }
  for (; i < sp.nvec; i += W) {
    const wa::Vec<S> v = q[i];
    ms_vecs<DT, 1>(m, s, &v);
  }
  if (lane < sp.tail) {
    const C x = E::load(p[sp.h + sp.nvec * VEC + lane]);
    ms_add<C, 1>(m, s, &x);
  }
}

// lane 0 of the team, after the fold
template <int DT>
AAMD_HD void row_finish(const Args& a, int64_t row, int64_t b, int u, int Ub, typename wa::Elem<DT>::C m, typename wa::Elem<DT>::C s) {
  using E = wa::Elem<DT>;
  const typename E::S* p = static_cast<const typename E::S*>(a.logits) + row * a.V;
  const double den = (double)(m + xlog(s));
  a.denom[row] = den;
  a.lpb[row] = (double)E::load(p[a.blank]) - den;
  if (u < Ub) {
    const int k = target_at(a, b, u);
    a.lpt[row] = k >= 0 ? (double)E::load(p[k]) - den : nan64();
  }
}

// fused_log_softmax = False: the input holds log-probabilities already
template <int DT>
AAMD_HD void gather_cell(const Args& a, int64_t row) {
  using E = wa::Elem<DT>;
  int64_t b;
  int t, u, Tb, Ub;
  if (!row_live(a, row, b, t, u, Tb, Ub)) return;
  const typename E::S* p = static_cast<const typename E::S*>(a.logits) + row * a.V;
  a.denom[row] = 0.0;
  a.lpb[row] = (double)E::load(p[a.blank]);
  if (u < Ub) {
    const int k = target_at(a, b, u);
    a.lpt[row] = k >= 0 ? (double)E::load(p[k]) : nan64();
  }
}

AAMD_HD int64_t row_blocks(int64_t rows, int W) {
  const int rpb = kThreads / W;
  const int64_t n = (rows + rpb - 1) / rpb;
  return n < (1 << 22) ? n : (1 << 22);
}

#if defined(__HIPCC__)
template <int DT, int W>
__global__ __launch_bounds__(kThreads) void row_kernel(Args a) {
  using C = typename wa::Elem<DT>::C;
  constexpr int RPB = kThreads / W;
  const int lane = threadIdx.x % W, team = threadIdx.x / W;
  const int64_t rows = cells(a.B, a.T, a.U1);
  for (int64_t r0 = (int64_t)blockIdx.x * RPB; r0 < rows; r0 += (int64_t)gridDim.x * RPB) {
    const int64_t row = r0 + team;
    int64_t b = 0;
    int t, u = 0, Tb, Ub = 0;
    const bool live = row < rows && row_live(a, row, b, t, u, Tb, Ub);    // the same for every lane of a team
    C m = neg_inf<C>(), s = C(0);
    if (live) row_partial<DT>(a, row, lane, W, m, s);
    AAMD_UNROLL
    for (int o = 1; o < W; o *= 2) {
      const C m2 = __shfl_xor(m, o, W), s2 = __shfl_xor(s, o, W);
      ms_combine<C>(m, s, m2, s2);
    }
    if (live && lane == 0) row_finish<DT>(a, row, b, u, Ub, m, s);
  }
}

template <int DT>
__global__ __launch_bounds__(kThreads) void gather_kernel(Args a) {
  const int64_t rows = cells(a.B, a.T, a.U1);
  for (int64_t row = (int64_t)blockIdx.x * kThreads + threadIdx.x; row < rows; row += (int64_t)gridDim.x * kThreads)
    gather_cell<DT>(a, row);
}
#endif

// ---- lattice -------------------------------------------------------------------------------------------------------------------------
AAMD_HD double logaddexp(double x, double y) {
  const double mx = y > x ? y : x;
  if (mx == neg_inf<double>()) return x != x ? x : (y != y ? y : mx);
  return mx + log1p(exp(-fabs(x - y)));
}

struct LatGeom {
  int64_t base;                      // b * T * U1
  int Tb, Ub, dir;                   // dir 0: alpha; 1: beta = alpha over the lattice reversed in both axes
};
template <int KU>
struct LatState {
  double pb[KU][kPF], pt[KU][kPF];
};

// lanes share the scan of the live labels
AAMD_HD bool lat_bad_targets(const Args& a, int64_t b, int Ub, int tid) {
  bool bad = false;
  for (int u = tid; u < Ub; u += kLatThreads) bad = bad || target_at(a, b, u) < 0;
  return bad;
}

// the two log-probabilities that cell (d - uu, uu) of the direction's own coordinates adds: -inf where there is no such term
AAMD_HD void lat_fetch(const Args& a, const LatGeom& g, int64_t d, int uu, double& pb, double& pt) {
  pb = pt = neg_inf<double>();
  const int64_t tt = d - uu;
  if (uu > g.Ub || tt < 0 || tt >= g.Tb) return;
  if (g.dir == 0) {
    if (tt >= 1) pb = a.lpb[g.base + (tt - 1) * a.U1 + uu];
    if (uu >= 1) pt = a.lpt[g.base + tt * a.U1 + uu - 1];
  } else {
    const int64_t at = g.base + (g.Tb - 1 - tt) * a.U1 + (g.Ub - uu);
    pb = a.lpb[at];
    if (uu >= 1) pt = a.lpt[at];
  }
}

AAMD_HD void lat_cell(const Args& a, const LatGeom& g, int64_t b, int64_t d, int uu, double pb, double pt, const double* prev,
                      double* cur) {
  const int64_t tt = d - uu;
  if (uu > g.Ub || tt < 0 || tt >= g.Tb) return;
  double v;
  if (tt == 0 && uu == 0) {
    v = g.dir ? pb : 0.0;
  } else {
    v = neg_inf<double>();
    if (tt >= 1) v = prev[uu] + pb;
    if (uu >= 1) v = logaddexp(v, prev[uu - 1] + pt);
  }
  cur[uu] = v;
  if (g.dir == 0) {
    a.alpha[g.base + tt * a.U1 + uu] = v;
  } else {
    a.beta[g.base + (g.Tb - 1 - tt) * a.U1 + (g.Ub - uu)] = v;
    if (tt == g.Tb - 1 && uu == g.Ub) a.costs[b] = -v;
  }
}

template <int KU>
AAMD_HD void lat_prime(const Args& a, const LatGeom& g, int tid, LatState<KU>& s) {
  AAMD_UNROLL
  for (int k = 0; k < KU; ++k) {
    AAMD_UNROLL
    for (int j = 0; j < kPF; ++j) lat_fetch(a, g, j, tid + k * kLatThreads, s.pb[k][j], s.pt[k][j]);
  }
}
// diagonal d = d0 + j (j a compile-time constant where this is inlined into the unrolled loop)
template <int KU>
AAMD_HD void lat_step(const Args& a, const LatGeom& g, int64_t b, int tid, int64_t d, int j, LatState<KU>& s, const double* prev,
                      double* cur) {
  AAMD_UNROLL
  for (int k = 0; k < KU; ++k) {
    const int uu = tid + k * kLatThreads;
    lat_cell(a, g, b, d, uu, s.pb[k][j], s.pt[k][j], prev, cur);
    lat_fetch(a, g, d + kPF, uu, s.pb[k][j], s.pt[k][j]);
  }
}

#if defined(__HIPCC__)
template <int KU>
__global__ __launch_bounds__(kLatThreads) void lattice_kernel(Args a) {
  __shared__ double buf[2][kLatThreads * KU];
  __shared__ int s_bad;
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x >> 1;
  LatGeom g;
  g.dir = blockIdx.x & 1;
  g.base = b * a.T * a.U1;
  const bool ok = lens_ok(a, b, g.Tb, g.Ub);
  if (tid == 0) s_bad = 0;
  __syncthreads();
  if (ok && lat_bad_targets(a, b, g.Ub, tid)) s_bad = 1;
  __syncthreads();
  if (!ok || s_bad) {                                       // the same in every lane
    if (g.dir && tid == 0) {
      a.costs[b] = nan64();
      a.bad[b] = 1;
    }
    return;
  }
  if (g.dir && tid == 0) a.bad[b] = 0;
  LatState<KU> s;
  lat_prime<KU>(a, g, tid, s);
  const int64_t D = (int64_t)g.Tb + g.Ub;
  for (int64_t d0 = 0; d0 < D; d0 += kPF) {
    AAMD_UNROLL
    for (int j = 0; j < kPF; ++j) {                         // past the last diagonal no cell is live: every lane meets every barrier
      const int64_t d = d0 + j;
      lat_step<KU>(a, g, b, tid, d, j, s, buf[(d & 1) ^ 1], buf[d & 1]);
      __syncthreads();
    }
  }
}
#endif

// ---- gradient ------------------------------------------------------------------------------------------------------------------------
template <int DT>
AAMD_HD void fill_row(typename wa::Elem<DT>::S* g, int64_t V, int lane, int W, typename wa::Elem<DT>::S value) {
  using S = typename wa::Elem<DT>::S;
  constexpr int VEC = 16 / (int)sizeof(S);
  const Split sp = split(g, V, (int)sizeof(S));
  if (lane < sp.h) g[lane] = value;
  wa::Vec<S> v;
  AAMD_UNROLL
  for (int k = 0; k < VEC; ++k) v.e[k] = value;
  wa::Vec<S>* q = reinterpret_cast<wa::Vec<S>*>(g + sp.h);
  for (int64_t i = lane; i < sp.nvec; i += W) q[i] = v;
  if (lane < sp.tail) g[sp.h + sp.nvec * VEC + lane] = value;
}

template <typename C>
struct GradRow {
  C c, cb, ct, go, clamp;            // exponent offsets of the occupancy and of the two transitions, grad_costs[b], the clamp
  int64_t blank, tgt;
  int fused;
};

template <int DT>
AAMD_HD typename wa::Elem<DT>::S grad_elem(const GradRow<typename wa::Elem<DT>::C>& r, int64_t idx, typename wa::Elem<DT>::S raw) {
  using E = wa::Elem<DT>;
  using C = typename E::C;
  const C l = E::load(raw);
  C g = r.fused ? xexp(l + r.c) : C(0);
  if (idx == r.blank) g -= xexp(l + r.cb);
  if (idx == r.tgt) g -= xexp(l + r.ct);
  if (r.clamp > C(0)) g = g < -r.clamp ? -r.clamp : (g > r.clamp ? r.clamp : g);
  return E::store(g * r.go);
}

template <int DT, int NV>
AAMD_HD void grad_vecs(const GradRow<typename wa::Elem<DT>::C>& r, int64_t first, int64_t stride,
                       const wa::Vec<typename wa::Elem<DT>::S>* in, typename wa::Elem<DT>::S* out, bool vec_store) {
  using S = typename wa::Elem<DT>::S;
  constexpr int VEC = 16 / (int)sizeof(S);
  AAMD_UNROLL
  for (int j = 0; j < NV; ++j) {
    wa::Vec<S> o;
    AAMD_UNROLL
    for (int k = 0; k < VEC; ++k) o.e[k] = grad_elem<DT>(r, first + j * stride + k, in[j].e[k]);
    S* dst = out + first + j * stride;
    if (vec_store) {
      *reinterpret_cast<wa::Vec<S>*>(dst) = o;
    } else {
      AAMD_UNROLL
      for (int k = 0; k < VEC; ++k) dst[k] = o.e[k];
    }
  }
}

template <int DT>
AAMD_HD void grad_row(const Args& a, int64_t row, int lane, int W) {
  using E = wa::Elem<DT>;
  using S = typename E::S;
  using C = typename E::C;
  constexpr int VEC = 16 / (int)sizeof(S);
  S* out = static_cast<S*>(a.grad) + row * a.V;
  int64_t b;
  int t, u, Tb, Ub;
  const bool live = row_live(a, row, b, t, u, Tb, Ub);
  if (a.bad[b]) {
    fill_row<DT>(out, a.V, lane, W, E::store((C)nan64()));
    return;
  }
  if (!live) {
    fill_row<DT>(out, a.V, lane, W, E::store(C(0)));
    return;
  }
  const double be = a.beta[row], logz = a.beta[b * a.T * a.U1];
  const double c = a.alpha[row] + be - logz - a.denom[row];
  const double db = t + 1 < Tb ? a.beta[row + a.U1] - be : (u == Ub ? -be : neg_inf<double>());
  const double dt = u < Ub ? a.beta[row + 1] - be : neg_inf<double>();
  GradRow<C> r;
  r.c = (C)c; r.cb = (C)(c + db); r.ct = (C)(c + dt);
  r.go = (C)a.grad_costs[b];
  r.clamp = (C)a.clamp;
  r.blank = a.blank;
  r.tgt = u < Ub ? target_at(a, b, u) : -1;
  r.fused = a.fused;
  const S* p = static_cast<const S*>(a.logits) + row * a.V;
  if (!a.fused) {                                           // two entries differ from zero: no pass over the row's values
    fill_row<DT>(out, a.V, lane, W, E::store(C(0)));
    return;
  }
  const Split sp = split(p, a.V, (int)sizeof(S));
  const bool vec_store = (((uintptr_t)p ^ (uintptr_t)out) & 15) == 0;
  if (lane < sp.h) out[lane] = grad_elem<DT>(r, lane, p[lane]);
  const wa::Vec<S>* q = reinterpret_cast<const wa::Vec<S>*>(p + sp.h);
  int64_t i = lane;
  for (; i + 3 * W < sp.nvec; i += 4 * W) {
    const wa::Vec<S> v[4] = {q[i], q[i + W], q[i + 2 * W], q[i + 3 * W]};
    grad_vecs<DT, 4>(r, sp.h + i * VEC, (int64_t)W * VEC, v, out, vec_store);
  }
  for (; i < sp.nvec; i += W) {
    const wa::Vec<S> v = q[i];
    grad_vecs<DT, 1>(r, sp.h + i * VEC, 0, &v, out, vec_store);
  }
  if (lane < sp.tail) {
    const int64_t idx = sp.h + sp.nvec * VEC + lane;
    out[idx] = grad_elem<DT>(r, idx, p[idx]);
  }
}

// not fused, after the zeros of the row are written by the whole team: lane 0 writes the two entries
template <int DT>
AAMD_HD void grad_row_sparse(const Args& a, int64_t row) {
  using E = wa::Elem<DT>;
  using S = typename E::S;
  using C = typename E::C;
  int64_t b;
  int t, u, Tb, Ub;
  if (a.fused || !row_live(a, row, b, t, u, Tb, Ub) || a.bad[b]) return;
  const S* p = static_cast<const S*>(a.logits) + row * a.V;
  S* out = static_cast<S*>(a.grad) + row * a.V;
  const double be = a.beta[row], logz = a.beta[b * a.T * a.U1];
  const double c = a.alpha[row] + be - logz;
  GradRow<C> r;
  r.c = (C)c;
  r.cb = (C)(c + (t + 1 < Tb ? a.beta[row + a.U1] - be : (u == Ub ? -be : neg_inf<double>())));
  r.ct = (C)(c + (u < Ub ? a.beta[row + 1] - be : neg_inf<double>()));
  r.go = (C)a.grad_costs[b];
  r.clamp = (C)a.clamp;
  r.blank = a.blank;
  r.tgt = u < Ub ? target_at(a, b, u) : -1;
  r.fused = 0;
  out[r.blank] = grad_elem<DT>(r, r.blank, p[r.blank]);
  if (r.tgt >= 0 && r.tgt != r.blank) out[r.tgt] = grad_elem<DT>(r, r.tgt, p[r.tgt]);
}

#if defined(__HIPCC__)
template <int DT, int W>
__global__ __launch_bounds__(kThreads) void grad_kernel(Args a) {
  constexpr int RPB = kThreads / W;
  const int lane = threadIdx.x % W, team = threadIdx.x / W;
  const int64_t rows = cells(a.B, a.T, a.U1);
  for (int64_t r0 = (int64_t)blockIdx.x * RPB; r0 < rows; r0 += (int64_t)gridDim.x * RPB) {
    const int64_t row = r0 + team;
    if (row < rows) grad_row<DT>(a, row, lane, W);
  }
}

// not fused: the two entries per live cell, launched behind grad_kernel on the same stream
template <int DT>
__global__ __launch_bounds__(kThreads) void grad_sparse_kernel(Args a) {
  const int64_t rows = cells(a.B, a.T, a.U1);
  for (int64_t row = (int64_t)blockIdx.x * kThreads + threadIdx.x; row < rows; row += (int64_t)gridDim.x * kThreads)
    grad_row_sparse<DT>(a, row);
}
#endif

}  // namespace rnnt
}  // namespace aamd
