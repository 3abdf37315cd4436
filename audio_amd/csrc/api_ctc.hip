// The CTC loss of the C ABI (csrc/ctc_loss.h): configuration and workspace queries, forward (row pass, alpha lattice,
// reduction), backward (beta lattice folded into the occupancy, gradient pass).
#include "api_common.h"
#include "ctc_loss.h"

using namespace aamd;

namespace {

int ctc_args(ctc::Args& a, int32_t dtype, const void* logits, int64_t stride_t, int64_t stride_n, const void* targets,
             int32_t targets_int64, int64_t target_pitch, int64_t target_entries, const void* input_lengths,
             const void* target_lengths, int32_t lengths_int64, int64_t batch, int64_t max_t, int64_t vocab, int64_t max_s,
             int32_t blank, int32_t fused, int32_t reduction, int32_t zero_infinity, const void* workspace) {
  AAMD_CHECK_ARG(dtype >= AAMD_SA_F32 && dtype <= AAMD_SA_BF16, "ctc_loss: unknown element type");
  AAMD_CHECK_ARG(batch >= 0 && max_t >= 1 && vocab >= 1 && max_s >= 0 && target_entries >= 0, "ctc_loss: bad sizes");
  AAMD_CHECK_ARG(max_t < (1ll << 31) && vocab < (1ll << 31) && batch < (1ll << 31) && target_entries < (1ll << 31),
                 "ctc_loss: batch, max_t, vocab and the target entries must fit 32 bits");
  AAMD_CHECK_ARG(target_pitch < 0 || target_pitch * batch == target_entries, "ctc_loss: padded targets hold batch * pitch entries");
  AAMD_CHECK_ARG(target_pitch <= max_s, "ctc_loss: max_s is below the pitch of the padded targets");
  if (max_s > AAMD_CTC_MAX_TARGET)
    return fail(AAMD_EUNSUPPORTED, "audio_amd: ctc_loss: the lattice kernel serves targets up to 2047 labels");
  AAMD_CHECK_ARG(blank >= 0 && blank < vocab, "ctc_loss: blank must lie in [0, vocab)");
  AAMD_CHECK_ARG(reduction >= ctc::kNone && reduction <= ctc::kSum, "ctc_loss: unknown reduction");
  AAMD_CHECK_ARG(workspace, "null buffer");
  AAMD_CHECK_ARG(((uintptr_t)workspace & 7) == 0, "ctc_loss: workspace must be 8-byte aligned");
  if (batch) {
    AAMD_CHECK_ARG(logits && input_lengths && target_lengths && (targets || target_entries == 0), "null buffer");
    AAMD_CHECK_ARG(((uintptr_t)logits & (uintptr_t)(elem_size(dtype) - 1)) == 0, "ctc_loss: logits is not aligned to its element");
  }
  a.x = logits; a.st = stride_t; a.sb = stride_n;
  a.targets = targets; a.in_len = input_lengths; a.tg_len = target_lengths;
  a.N = batch; a.T = max_t; a.V = vocab; a.S = max_s; a.pitch = target_pitch < 0 ? -1 : target_pitch; a.total = target_entries;
  a.blank = blank; a.fused = fused ? 1 : 0; a.tgt64 = targets_int64 ? 1 : 0; a.len64 = lengths_int64 ? 1 : 0;
  a.reduction = reduction; a.zero_inf = zero_infinity ? 1 : 0;
  ctc::ws_bind(a, const_cast<void*>(workspace));
  return AAMD_OK;
}

// KIND 0: the row pass, 1: the gradient pass; one instantiation per element type and team width
template <int KIND, int DT, int W>
int team_launch(const ctc::Args& a, hipStream_t s) {
  const int64_t blocks = rnnt::row_blocks(a.T * a.N, W);
  if (KIND == 0) return launch(ctc::row_kernel<DT, W>, blocks, ctc::kThreads, 0, s, a);
  return launch(ctc::grad_kernel<DT, W>, blocks, ctc::kThreads, 0, s, a);
}
template <int KIND>
int team_launch_dt(int32_t dtype, const ctc::Args& a, hipStream_t s) {
  return for_dtype(dtype, [&](auto dt) {
    switch (rnnt::team_width(elem_size(dt.value), a.V)) {
      case 8: return team_launch<KIND, dt.value, 8>(a, s);
      case 16: return team_launch<KIND, dt.value, 16>(a, s);
      case 32: return team_launch<KIND, dt.value, 32>(a, s);
      default: return team_launch<KIND, dt.value, 64>(a, s);
    }
  });
}

// one workgroup per example, the configuration by the bound on the target lengths
template <int DIR>
int lattice_launch(int32_t dtype, const ctc::Args& a, hipStream_t s) {
  int ks, nt;
  ctc::config(a.S, ks, nt);
  return for_dtype(dtype, [&](auto dt) {
    if (nt == 64) return launch(ctc::lattice_kernel<dt.value, 4, 64, DIR>, a.N, 64, 0, s, a);
    if (ks == 4) return launch(ctc::lattice_kernel<dt.value, 4, 256, DIR>, a.N, 256, 0, s, a);
    return launch(ctc::lattice_kernel<dt.value, 16, 256, DIR>, a.N, 256, 0, s, a);
  });
}

}  // namespace

extern "C" {

int32_t aamd_ctc_loss_config(int32_t which, int64_t max_s) {
  int ks, nt;
  ctc::config(max_s, ks, nt);
  switch (which) {
    case 0: return ks;
    case 1: return nt;
    case 2: return ctc::kPF;
    case 3: return ctc::kMaxS;
    default: return 0;
  }
}

int64_t aamd_ctc_loss_workspace(int64_t batch, int64_t max_t, int64_t target_entries) {
  if (batch < 0 || max_t < 0 || target_entries < 0) return 0;
  return ctc::ws_doubles(batch, max_t, target_entries) * 8;
}

int aamd_ctc_loss_forward(int32_t dtype, const void* logits, int64_t stride_t, int64_t stride_n, const void* targets,
                          int32_t targets_int64, int64_t target_pitch, int64_t target_entries, const void* input_lengths,
                          const void* target_lengths, int32_t lengths_int64, int64_t batch, int64_t max_t, int64_t vocab,
                          int64_t max_s, int32_t blank, int32_t fused_log_softmax, int32_t reduction, int32_t zero_infinity,
                          void* workspace, void* out, void* stream) {
  DeviceScope dev_scope_(workspace);
  static_assert(ctc::kMaxS == AAMD_CTC_MAX_TARGET, "the header's limit is the lattice kernel's");
  ctc::Args a{};
  AAMD_TRY(ctc_args(a, dtype, logits, stride_t, stride_n, targets, targets_int64, target_pitch, target_entries, input_lengths,
                    target_lengths, lengths_int64, batch, max_t, vocab, max_s, blank, fused_log_softmax, reduction,
                    zero_infinity, workspace));
  AAMD_CHECK_ARG(out, "null buffer");
  AAMD_CHECK_ARG(((uintptr_t)out & (uintptr_t)(elem_size(dtype) - 1)) == 0, "ctc_loss: out is not aligned to its element");
  a.out = out;
  hipStream_t s = (hipStream_t)stream;
  if (batch) {
    if (a.fused) AAMD_TRY(team_launch_dt<0>(dtype, a, s));
    AAMD_TRY(lattice_launch<0>(dtype, a, s));
  }
  return for_dtype(dtype, [&](auto dt) { return launch(ctc::reduce_kernel<dt.value>, 1, ctc::kThreads, 0, s, a); });
}

int aamd_ctc_loss_backward(int32_t dtype, const void* logits, int64_t stride_t, int64_t stride_n, const void* targets,
                           int32_t targets_int64, int64_t target_pitch, int64_t target_entries, const void* input_lengths,
                           const void* target_lengths, int32_t lengths_int64, int64_t batch, int64_t max_t, int64_t vocab,
                           int64_t max_s, int32_t blank, int32_t fused_log_softmax, int32_t reduction, int32_t zero_infinity,
                           void* workspace, const double* grad_out, int64_t grad_out_stride, void* grad, int64_t grad_stride_t,
                           int64_t grad_stride_n, void* stream) {
  DeviceScope dev_scope_(workspace);
  ctc::Args a{};
  AAMD_TRY(ctc_args(a, dtype, logits, stride_t, stride_n, targets, targets_int64, target_pitch, target_entries, input_lengths,
                    target_lengths, lengths_int64, batch, max_t, vocab, max_s, blank, fused_log_softmax, reduction,
                    zero_infinity, workspace));
  if (batch == 0) return AAMD_OK;
  AAMD_CHECK_ARG(grad_out && grad, "null buffer");
  AAMD_CHECK_ARG(grad_out_stride == 0 || grad_out_stride == 1, "ctc_loss: grad_out is one element or one per example");
  AAMD_CHECK_ARG(((uintptr_t)grad & (uintptr_t)(elem_size(dtype) - 1)) == 0, "ctc_loss: grad is not aligned to its element");
  a.go = grad_out; a.go_stride = grad_out_stride; a.grad = grad; a.gst = grad_stride_t; a.gsb = grad_stride_n;
  hipStream_t s = (hipStream_t)stream;
  AAMD_TRY(lattice_launch<1>(dtype, a, s));
  return team_launch_dt<1>(dtype, a, s);
}

}  // extern "C"
