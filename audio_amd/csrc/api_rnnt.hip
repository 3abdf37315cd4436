// The RNN transducer loss of the C ABI (csrc/rnnt_loss.h): workspace query, forward (row pass + lattice), backward.
#include "api_common.h"
#include "rnnt_loss.h"

using namespace aamd;

namespace {

int elem_bytes(int32_t dtype) { return dtype == AAMD_SA_F64 ? 8 : (dtype == AAMD_SA_F32 ? 4 : 2); }

int rnnt_args(rnnt::Args& a, int32_t dtype, const void* logits, const int32_t* targets, const int32_t* logit_lengths,
              const int32_t* target_lengths, int64_t batch, int64_t max_t, int64_t max_u1, int64_t vocab, int32_t blank,
              int32_t fused, const void* workspace) {
  AAMD_CHECK_ARG(dtype >= AAMD_SA_F32 && dtype <= AAMD_SA_BF16, "rnnt_loss: unknown element type");
  AAMD_CHECK_ARG(batch >= 0 && max_t >= 1 && max_u1 >= 1 && vocab >= 1, "rnnt_loss: bad sizes");
  AAMD_CHECK_ARG(max_t < (1ll << 31) && vocab < (1ll << 31), "rnnt_loss: max_t and vocab must fit 32 bits");
  if (max_u1 > AAMD_RNNT_MAX_U1)
    return fail(AAMD_EUNSUPPORTED, "audio_amd: rnnt_loss: the lattice kernel serves U + 1 <= 1024");
  AAMD_CHECK_ARG(blank >= 0 && blank < vocab, "rnnt_loss: blank must lie in [0, vocab)");
  if (batch == 0) return AAMD_OK;
  AAMD_CHECK_ARG(logits && logit_lengths && target_lengths && workspace && (targets || max_u1 == 1), "null buffer");
  AAMD_CHECK_ARG(((uintptr_t)workspace & 7) == 0, "rnnt_loss: workspace must be 8-byte aligned");
  AAMD_CHECK_ARG(((uintptr_t)logits & (uintptr_t)(elem_bytes(dtype) - 1)) == 0, "rnnt_loss: logits is not aligned to its element");
  a.logits = logits; a.targets = targets; a.logit_lengths = logit_lengths; a.target_lengths = target_lengths;
  a.B = batch; a.T = max_t; a.U1 = max_u1; a.V = vocab; a.blank = blank; a.fused = fused ? 1 : 0;
  rnnt::ws_bind(a, const_cast<void*>(workspace));
  return AAMD_OK;
}

// KIND 0: the row pass, 1: the gradient pass; one instantiation per element type and team width
template <int KIND, int DT, int W>
int team_launch(const rnnt::Args& a, hipStream_t s) {
  const int64_t blocks = rnnt::row_blocks(rnnt::cells(a.B, a.T, a.U1), W);
  if (KIND == 0) return launch(rnnt::row_kernel<DT, W>, blocks, rnnt::kThreads, 0, s, a);
  return launch(rnnt::grad_kernel<DT, W>, blocks, rnnt::kThreads, 0, s, a);
}
template <int KIND, int DT>
int team_launch_w(const rnnt::Args& a, hipStream_t s) {
  switch (rnnt::team_width((int)sizeof(typename wa::Elem<DT>::S), a.V)) {
    case 8: return team_launch<KIND, DT, 8>(a, s);
    case 16: return team_launch<KIND, DT, 16>(a, s);
    case 32: return team_launch<KIND, DT, 32>(a, s);
    default: return team_launch<KIND, DT, 64>(a, s);
  }
}
template <int KIND>
int team_launch_dt(int32_t dtype, const rnnt::Args& a, hipStream_t s) {
  switch (dtype) {
    case AAMD_SA_F32: return team_launch_w<KIND, wa::kF32>(a, s);
    case AAMD_SA_F64: return team_launch_w<KIND, wa::kF64>(a, s);
    case AAMD_SA_F16: return team_launch_w<KIND, wa::kF16>(a, s);
    default: return team_launch_w<KIND, wa::kBF16>(a, s);
  }
}

// KIND 0: gather_kernel (forward, not fused), 1: grad_sparse_kernel (backward, not fused): one thread per cell
template <int KIND>
int cell_launch(int32_t dtype, const rnnt::Args& a, hipStream_t s) {
  const int64_t n = rnnt::cells(a.B, a.T, a.U1);
  int64_t blocks = (n + rnnt::kThreads - 1) / rnnt::kThreads;
  if (blocks > (1 << 22)) blocks = 1 << 22;
#define AAMD_RNNT_CELL(DT) \
  return KIND == 0 ? launch(rnnt::gather_kernel<DT>, blocks, rnnt::kThreads, 0, s, a) \
                   : launch(rnnt::grad_sparse_kernel<DT>, blocks, rnnt::kThreads, 0, s, a)
  switch (dtype) {
    case AAMD_SA_F32: AAMD_RNNT_CELL(wa::kF32);
    case AAMD_SA_F64: AAMD_RNNT_CELL(wa::kF64);
    case AAMD_SA_F16: AAMD_RNNT_CELL(wa::kF16);
    default: AAMD_RNNT_CELL(wa::kBF16);
  }
#undef AAMD_RNNT_CELL
}

}  // namespace

extern "C" {

int32_t aamd_rnnt_team_width(int32_t dtype, int64_t vocab) { return rnnt::team_width(elem_bytes(dtype), vocab); }
int32_t aamd_rnnt_lattice_threads(void) { return rnnt::kLatThreads; }

int64_t aamd_rnnt_loss_workspace(int64_t batch, int64_t max_t, int64_t max_u1) {
  if (batch < 0 || max_t < 0 || max_u1 < 0) return 0;
  return rnnt::ws_bytes(batch, max_t, max_u1);
}

int aamd_rnnt_loss_forward(int32_t dtype, const void* logits, const int32_t* targets, const int32_t* logit_lengths,
                           const int32_t* target_lengths, int64_t batch, int64_t max_t, int64_t max_u1, int64_t vocab,
                           int32_t blank, int32_t fused_log_softmax, void* workspace, double* costs, void* stream) {
  DeviceScope dev_scope_(logits);
  static_assert(rnnt::kMaxU1 == AAMD_RNNT_MAX_U1, "the header's limit is the lattice kernel's");
  rnnt::Args a{};
  int rc = rnnt_args(a, dtype, logits, targets, logit_lengths, target_lengths, batch, max_t, max_u1, vocab, blank,
                     fused_log_softmax, workspace);
  if (rc != AAMD_OK || batch == 0) return rc;
  AAMD_CHECK_ARG(costs, "null buffer");
  AAMD_CHECK_ARG(2 * batch < (1ll << 31), "rnnt_loss: too many examples for one launch");
  a.costs = costs;
  hipStream_t s = (hipStream_t)stream;
  rc = a.fused ? team_launch_dt<0>(dtype, a, s) : cell_launch<0>(dtype, a, s);
  if (rc != AAMD_OK) return rc;
  switch (rnnt::lat_ku(max_u1)) {
    case 1: return launch(rnnt::lattice_kernel<1>, 2 * batch, rnnt::kLatThreads, 0, s, a);
    case 2: return launch(rnnt::lattice_kernel<2>, 2 * batch, rnnt::kLatThreads, 0, s, a);
    default: return launch(rnnt::lattice_kernel<rnnt::kMaxKU>, 2 * batch, rnnt::kLatThreads, 0, s, a);
  }
}

int aamd_rnnt_loss_backward(int32_t dtype, const void* logits, const int32_t* targets, const int32_t* logit_lengths,
                            const int32_t* target_lengths, int64_t batch, int64_t max_t, int64_t max_u1, int64_t vocab,
                            int32_t blank, int32_t fused_log_softmax, double clamp, const void* workspace,
                            const double* grad_costs, void* grad, void* stream) {
  DeviceScope dev_scope_(logits);
  rnnt::Args a{};
  int rc = rnnt_args(a, dtype, logits, targets, logit_lengths, target_lengths, batch, max_t, max_u1, vocab, blank,
                     fused_log_softmax, workspace);
  if (rc != AAMD_OK || batch == 0) return rc;
  AAMD_CHECK_ARG(grad_costs && grad, "null buffer");
  AAMD_CHECK_ARG(((uintptr_t)grad & (uintptr_t)(elem_bytes(dtype) - 1)) == 0, "rnnt_loss: grad is not aligned to its element");
  a.grad_costs = grad_costs; a.grad = grad; a.clamp = clamp;
  hipStream_t s = (hipStream_t)stream;
  rc = team_launch_dt<1>(dtype, a, s);
  if (rc != AAMD_OK || a.fused) return rc;
  return cell_launch<1>(dtype, a, s);
}

}  // extern "C"
