// CPU replay of the transducer-loss kernels (audio_amd/csrc/rnnt_loss.h compiled with g++, no GPU): each driver mirrors its
// __global__ kernel with the launch geometry of the C ABI -- "all threads run a phase, then __syncthreads()" is a loop over
// thread ids, the xor butterfly of a team is run over an array of its lanes' values.  TEST INFRASTRUCTURE ONLY.
#include <cstdint>
#include <vector>

#include "../../audio_amd/csrc/rnnt_loss.h"

using namespace aamd;

template <int DT>
static void row_run(const rnnt::Args& a) {
  using C = typename wa::Elem<DT>::C;
  const int W = rnnt::team_width((int)sizeof(typename wa::Elem<DT>::S), a.V);
  const int64_t rows = rnnt::cells(a.B, a.T, a.U1);
  std::vector<C> m(W), s(W), m2(W), s2(W);
  for (int64_t row = 0; row < rows; ++row) {
    int64_t b;
    int t, u, Tb, Ub;
    if (!rnnt::row_live(a, row, b, t, u, Tb, Ub)) continue;
    for (int l = 0; l < W; ++l) rnnt::row_partial<DT>(a, row, l, W, m[l], s[l]);
    for (int o = 1; o < W; o *= 2) {
      for (int l = 0; l < W; ++l) { m2[l] = m[l ^ o]; s2[l] = s[l ^ o]; }
      for (int l = 0; l < W; ++l) rnnt::ms_combine<C>(m[l], s[l], m2[l], s2[l]);
    }
    rnnt::row_finish<DT>(a, row, b, u, Ub, m[0], s[0]);
  }
}

template <int DT>
static void gather_run(const rnnt::Args& a) {
  for (int64_t row = 0; row < rnnt::cells(a.B, a.T, a.U1); ++row) rnnt::gather_cell<DT>(a, row);
}

template <int KU>
static void lattice_run(const rnnt::Args& a) {
  const int NT = rnnt::kLatThreads;
  std::vector<double> buf0(NT * KU), buf1(NT * KU);
  std::vector<rnnt::LatState<KU>> st(NT);
  for (int64_t blk = 0; blk < 2 * a.B; ++blk) {
    const int64_t b = blk >> 1;
    rnnt::LatGeom g;
    g.dir = (int)(blk & 1);
    g.base = b * a.T * a.U1;
    const bool ok = rnnt::lens_ok(a, b, g.Tb, g.Ub);
    bool bad = !ok;
    for (int tid = 0; ok && tid < NT; ++tid) bad = bad || rnnt::lat_bad_targets(a, b, g.Ub, tid);
    if (bad) {
      if (g.dir) { a.costs[b] = rnnt::nan64(); a.bad[b] = 1; }
      continue;
    }
    if (g.dir) a.bad[b] = 0;
    for (int tid = 0; tid < NT; ++tid) rnnt::lat_prime<KU>(a, g, tid, st[tid]);
    const int64_t D = (int64_t)g.Tb + g.Ub;
    for (int64_t d0 = 0; d0 < D; d0 += rnnt::kPF)
      for (int j = 0; j < rnnt::kPF; ++j) {
        const int64_t d = d0 + j;
        double* cur = (d & 1) ? buf1.data() : buf0.data();
        const double* prev = (d & 1) ? buf0.data() : buf1.data();
        for (int tid = 0; tid < NT; ++tid) rnnt::lat_step<KU>(a, g, b, tid, d, j, st[tid], prev, cur);
      }
  }
}

template <int DT>
static void grad_run(const rnnt::Args& a) {
  const int W = rnnt::team_width((int)sizeof(typename wa::Elem<DT>::S), a.V);
  const int64_t rows = rnnt::cells(a.B, a.T, a.U1);
  for (int64_t row = 0; row < rows; ++row)
    for (int l = 0; l < W; ++l) rnnt::grad_row<DT>(a, row, l, W);
  for (int64_t row = 0; row < rows; ++row) rnnt::grad_row_sparse<DT>(a, row);
}

static void bind(rnnt::Args& a, const void* logits, const int32_t* targets, const int32_t* ll, const int32_t* tl,
                 const int64_t* dims, int blank, int fused, void* ws) {
  a.logits = logits; a.targets = targets; a.logit_lengths = ll; a.target_lengths = tl;
  a.B = dims[0]; a.T = dims[1]; a.U1 = dims[2]; a.V = dims[3]; a.blank = blank; a.fused = fused;
  rnnt::ws_bind(a, ws);
}

extern "C" {

int sim_rnnt_team_width(int dtype, int64_t V) { return rnnt::team_width(dtype == wa::kF64 ? 8 : (dtype == wa::kF32 ? 4 : 2), V); }
int sim_rnnt_lattice_threads() { return rnnt::kLatThreads; }
int sim_rnnt_max_u1() { return rnnt::kMaxU1; }
int64_t sim_rnnt_workspace(int64_t B, int64_t T, int64_t U1) { return rnnt::ws_bytes(B, T, U1); }

// dims: B, T, U1, V
int sim_rnnt_forward(int dtype, const void* logits, const int32_t* targets, const int32_t* ll, const int32_t* tl,
                     const int64_t* dims, int blank, int fused, void* ws, double* costs) {
  rnnt::Args a{};
  bind(a, logits, targets, ll, tl, dims, blank, fused, ws);
  if (a.U1 > rnnt::kMaxU1) return -2;
  a.costs = costs;
  if (fused) {
    switch (dtype) {
      case wa::kF32: row_run<wa::kF32>(a); break;
      case wa::kF64: row_run<wa::kF64>(a); break;
      case wa::kF16: row_run<wa::kF16>(a); break;
      default: row_run<wa::kBF16>(a); break;
    }
  } else {
    switch (dtype) {
      case wa::kF32: gather_run<wa::kF32>(a); break;
      case wa::kF64: gather_run<wa::kF64>(a); break;
      case wa::kF16: gather_run<wa::kF16>(a); break;
      default: gather_run<wa::kBF16>(a); break;
    }
  }
  switch (rnnt::lat_ku(a.U1)) {
    case 1: lattice_run<1>(a); break;
    case 2: lattice_run<2>(a); break;
    default: lattice_run<rnnt::kMaxKU>(a); break;
  }
  return 0;
}

int sim_rnnt_backward(int dtype, const void* logits, const int32_t* targets, const int32_t* ll, const int32_t* tl,
                      const int64_t* dims, int blank, int fused, double clamp, void* ws, const double* grad_costs, void* grad) {
  rnnt::Args a{};
  bind(a, logits, targets, ll, tl, dims, blank, fused, ws);
  a.clamp = clamp; a.grad_costs = grad_costs; a.grad = grad;
  switch (dtype) {
    case wa::kF32: grad_run<wa::kF32>(a); break;
    case wa::kF64: grad_run<wa::kF64>(a); break;
    case wa::kF16: grad_run<wa::kF16>(a); break;
    default: grad_run<wa::kBF16>(a); break;
  }
  return 0;
}

}  // extern "C"
