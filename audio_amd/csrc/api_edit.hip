// Batched edit distance of the C ABI (csrc/edit_distance.h): exported configurations and limits, the one launch.
#include "api_common.h"
#include "edit_distance.h"

using namespace aamd;

extern "C" {

int32_t aamd_edit_distance_states_per_lane(int64_t max_m) {
  int ks, nt;
  ed::config(max_m, ks, nt);
  return ks;
}
int32_t aamd_edit_distance_threads(int64_t max_m) {
  int ks, nt;
  ed::config(max_m, ks, nt);
  return nt;
}
int32_t aamd_edit_distance_max_ref(void) { return ed::kMaxRef; }
int32_t aamd_edit_distance_max_hyp(void) { return ed::kMaxHyp; }

int aamd_edit_distance(const void* hyps, int32_t hyps_int64, const void* refs, int32_t refs_int64, const void* hyp_lengths,
                       int32_t hyp_lengths_int64, const void* ref_lengths, int32_t ref_lengths_int64, int64_t pairs,
                       int64_t pairs_per_ref, int64_t max_n, int64_t max_m, int32_t return_ops, int32_t* out, void* stream) {
  DeviceScope dev_scope_(out);
  static_assert(ed::kMaxRef == AAMD_EDIT_DISTANCE_MAX_REF && ed::kMaxHyp == AAMD_EDIT_DISTANCE_MAX_HYP,
                "the header's limits are the kernel's");
  AAMD_CHECK_ARG(pairs >= 0 && pairs_per_ref >= 1 && max_n >= 0 && max_m >= 0, "edit_distance: bad sizes");
  AAMD_CHECK_ARG(pairs % pairs_per_ref == 0, "edit_distance: pairs must be a multiple of pairs_per_ref");
  AAMD_CHECK_ARG(pairs < (1ll << 31), "edit_distance: pairs must fit 32 bits");
  if (max_m > AAMD_EDIT_DISTANCE_MAX_REF)
    return fail(AAMD_EUNSUPPORTED, "audio_amd: edit_distance: the kernel serves references of width M <= 4096");
  if (max_n > AAMD_EDIT_DISTANCE_MAX_HYP)
    return fail(AAMD_EUNSUPPORTED, "audio_amd: edit_distance: the kernel serves hypotheses of width N <= 32767");
  if (pairs == 0) return AAMD_OK;
  AAMD_CHECK_ARG(out && (hyps || max_n == 0) && (refs || max_m == 0), "null buffer");
  AAMD_CHECK_ARG(((uintptr_t)out & 3) == 0 && ((uintptr_t)hyps & (hyps_int64 ? 7 : 3)) == 0 &&
                     ((uintptr_t)refs & (refs_int64 ? 7 : 3)) == 0 && ((uintptr_t)hyp_lengths & (hyp_lengths_int64 ? 7 : 3)) == 0 &&
                     ((uintptr_t)ref_lengths & (ref_lengths_int64 ? 7 : 3)) == 0,
                 "edit_distance: a buffer is not aligned to its element");
  ed::Args a{};
  a.hyps = hyps; a.refs = refs; a.hyp_len = hyp_lengths; a.ref_len = ref_lengths;
  a.pairs = pairs; a.per_ref = pairs_per_ref; a.N = max_n; a.M = max_m;
  a.hyp64 = hyps_int64 ? 1 : 0; a.ref64 = refs_int64 ? 1 : 0;
  a.hlen64 = hyp_lengths_int64 ? 1 : 0; a.rlen64 = ref_lengths_int64 ? 1 : 0;
  a.ops = return_ops ? 1 : 0;
  a.out = out;
  hipStream_t s = (hipStream_t)stream;
  int ks, nt;
  ed::config(max_m, ks, nt);
  if (nt == 64) return launch(ed::edit_kernel<4, 64>, pairs, 64, 0, s, a);
  if (ks == 4) return launch(ed::edit_kernel<4, 256>, pairs, 256, 0, s, a);
  return launch(ed::edit_kernel<16, 256>, pairs, 256, 0, s, a);
}

}  // extern "C"
