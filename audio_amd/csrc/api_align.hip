// CTC forced alignment of the C ABI (csrc/forced_align.h): exported constants, workspace query, forward + backtrack.
#include "api_common.h"
#include "forced_align.h"

using namespace aamd;

namespace {

template <int DT>
int forward_launch(const fa::Args& a, hipStream_t s) {
  if (a.nt == 64) return launch(fa::forward_kernel<DT, 4, 64>, a.B, 64, 0, s, a);
  if (a.ks == 4) return launch(fa::forward_kernel<DT, 4, 256>, a.B, 256, 0, s, a);
  return launch(fa::forward_kernel<DT, 16, 256>, a.B, 256, 0, s, a);
}

}  // namespace

extern "C" {

int32_t aamd_forced_align_states_per_lane(int64_t max_l) {
  int ks, nt;
  fa::config(max_l, ks, nt);
  return ks;
}
int32_t aamd_forced_align_threads(int64_t max_l) {
  int ks, nt;
  fa::config(max_l, ks, nt);
  return nt;
}
int32_t aamd_forced_align_prefetch(void) { return fa::kPF; }
int32_t aamd_forced_align_backtrack_block(void) { return fa::kBT; }

int64_t aamd_forced_align_workspace(int64_t batch, int64_t max_t, int64_t max_l) {
  if (batch < 0 || max_t < 0 || max_l < 0 || max_l > fa::kMaxL) return 0;
  return fa::ws_bytes(batch, max_t, max_l);
}

int aamd_forced_align(int32_t dtype, const void* log_probs, const void* targets, int32_t targets_int64,
                      const void* input_lengths, const void* target_lengths, int32_t lengths_int64, int64_t batch,
                      int64_t max_t, int64_t classes, int64_t max_l, int32_t blank, void* workspace, void* paths, void* scores,
                      void* stream) {
  DeviceScope dev_scope_(log_probs);
  static_assert(fa::kMaxL == AAMD_FORCED_ALIGN_MAX_L, "the header's limit is the forward kernel's");
  AAMD_CHECK_ARG(dtype >= AAMD_SA_F32 && dtype <= AAMD_SA_BF16, "forced_align: unknown element type");
  AAMD_CHECK_ARG(batch >= 0 && max_t >= 1 && classes >= 1 && max_l >= 0, "forced_align: bad sizes");
  AAMD_CHECK_ARG(max_t < (1ll << 31) && classes < (1ll << 31) && batch < (1ll << 31),
                 "forced_align: batch, max_t and classes must fit 32 bits");
  if (max_l > AAMD_FORCED_ALIGN_MAX_L)
    return fail(AAMD_EUNSUPPORTED, "audio_amd: forced_align: the forward kernel serves L <= 2047");
  AAMD_CHECK_ARG(blank >= 0 && blank < classes, "forced_align: blank must lie in [0, classes)");
  if (batch == 0) return AAMD_OK;
  AAMD_CHECK_ARG(log_probs && input_lengths && target_lengths && workspace && paths && scores && (targets || max_l == 0),
                 "null buffer");
  const int es = dtype == AAMD_SA_F64 ? 8 : (dtype == AAMD_SA_F32 ? 4 : 2);
  AAMD_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "forced_align: workspace must be 16-byte aligned");
  AAMD_CHECK_ARG((((uintptr_t)log_probs | (uintptr_t)scores) & (uintptr_t)(es - 1)) == 0,
                 "forced_align: log_probs or scores is not aligned to its element");
  fa::Args a{};
  a.lp = log_probs; a.targets = targets; a.in_len = input_lengths; a.tg_len = target_lengths;
  a.B = batch; a.T = max_t; a.C = classes; a.L = max_l;
  a.blank = blank; a.tgt64 = targets_int64 ? 1 : 0; a.len64 = lengths_int64 ? 1 : 0; a.dtype = dtype;
  a.paths = paths; a.scores = scores;
  fa::ws_bind(a, workspace);
  hipStream_t s = (hipStream_t)stream;
  int rc;
  switch (dtype) {
    case AAMD_SA_F32: rc = forward_launch<wa::kF32>(a, s); break;
    case AAMD_SA_F64: rc = forward_launch<wa::kF64>(a, s); break;
    case AAMD_SA_F16: rc = forward_launch<wa::kF16>(a, s); break;
    default: rc = forward_launch<wa::kBF16>(a, s); break;
  }
  if (rc != AAMD_OK) return rc;
  return launch(fa::backtrack_kernel, batch, fa::kBtThreads, 0, s, a);
}

}  // extern "C"
