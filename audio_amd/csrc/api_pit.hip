// Permutation-invariant training of the C ABI (csrc/pit.h): exported constants, the workspace query, the fused forward
// (pairwise scores + assignment, four launches), the assignment alone, the permuted backward and the row gather.
//
// Device pass only: the compiler may form no packed fp32 arithmetic (v_pk_*_f32) in this translation unit, whatever the
// vectoriser's settings.  The kernels' arithmetic is float64; the attribute keeps the half-type conversions and the float32
// stores that way.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif
#include "api_common.h"
#include "pit.h"

using namespace aamd;

namespace {

struct Layout {
  int64_t gspans, rparts, chunks;
  int64_t gram, pstat, res, total;         // byte offsets
};

Layout layout_of(int64_t B, int64_t S, int64_t T) {
  Layout l{};
  l.gspans = T > 0 ? sdr::ceil_div(T, pit::kGramSpan) : 1;
  l.rparts = T > 0 ? sdr::ceil_div(T, pit::res_sub((int)S)) : 1;
  l.chunks = T > 0 ? sdr::ceil_div(T, pit::kResChunk) : 1;
  l.gram = 0;
  l.pstat = l.gram + B * l.gspans * pit::kPart * 8;
  l.res = l.pstat + B * S * S * sdr::kStat * 8;
  l.total = l.res + B * l.rparts * 64 * 8;
  return l;
}

// the checks the waveform entry points share; fills what the kernels read of the inputs
int common(const char* who, pit::Args& a, int32_t dtype, int32_t mode, const void* preds, const void* target, int64_t batch,
           int64_t sources, int64_t length, int64_t pb, int64_t ps, int64_t tb, int64_t ts, const void* lengths,
           int32_t lengths_int64, int32_t zero_mean) {
  const std::string w(who);
  AAMD_CHECK_ARG(dtype >= AAMD_SA_F32 && dtype <= AAMD_SA_BF16, w + ": unknown element type");
  AAMD_CHECK_ARG(mode == sdr::kModeSi || mode == sdr::kModeSnr, w + ": mode must be 1 (SI-SDR) or 2 (SNR)");
  AAMD_CHECK_ARG(batch >= 0 && length >= 0 && pb >= 0 && ps >= 0 && tb >= 0 && ts >= 0, w + ": bad sizes");
  AAMD_CHECK_ARG(sources >= 1, w + ": at least one source is needed");
  if (sources > pit::kMaxS)
    return fail(AAMD_EUNSUPPORTED, "audio_amd: " + w + ": more than " + std::to_string(pit::kMaxS) + " sources are not implemented");
  AAMD_CHECK_ARG(batch < (1ll << 31) && length < (1ll << 40), w + ": too many examples or samples");
  AAMD_CHECK_ARG((preds && target) || length == 0 || batch == 0, w + ": null buffer");
  AAMD_CHECK_ARG((((uintptr_t)preds | (uintptr_t)target) & (uintptr_t)(elem_size(dtype) - 1)) == 0, w + ": a waveform is not aligned to its element");
  AAMD_CHECK_ARG(((uintptr_t)lengths & (lengths_int64 ? 7 : 3)) == 0, w + ": lengths is misaligned");
  a.p = preds; a.t = target; a.lengths = lengths;
  a.B = batch; a.S = (int32_t)sources; a.T = length;
  a.pb = batch > 1 ? pb : 0; a.ps = sources > 1 ? ps : 0; a.tb = batch > 1 ? tb : 0; a.ts = sources > 1 ? ts : 0;
  a.len64 = lengths_int64 ? 1 : 0; a.zero_mean = zero_mean ? 1 : 0; a.mode = mode;
  a.eps = comp_eps(dtype);
  const Layout l = layout_of(batch, sources, length);
  a.gspans = l.gspans; a.rparts = l.rparts; a.chunks = l.chunks;
  a.gchunks = length > 0 ? sdr::ceil_div(length, sdr::kChunk) : 1;
  AAMD_CHECK_ARG(batch * sources * a.gchunks < (1ll << 31), w + ": too many workgroups");
  return AAMD_OK;
}

template <int DT>
int run_forward(const pit::Args& a, hipStream_t s) {
  using C = typename wa::Elem<DT>::C;
  AAMD_TRY(launch(pit::gram_kernel<DT>, a.B * a.gspans, pit::kThreads, 0, s, a));
  AAMD_TRY(launch(pit::pair_stats_kernel<DT>, a.B, sdr::kSolveThreads, 0, s, a));
  switch (pit::res_bucket(a.S)) {
    case 1: AAMD_TRY(launch(pit::pair_residual_kernel<DT, 1>, a.B * a.chunks, pit::kThreads, 0, s, a)); break;
    case 2: AAMD_TRY(launch(pit::pair_residual_kernel<DT, 2>, a.B * a.chunks, pit::kThreads, 0, s, a)); break;
    case 4: AAMD_TRY(launch(pit::pair_residual_kernel<DT, 4>, a.B * a.chunks, pit::kThreads, 0, s, a)); break;
    default: AAMD_TRY(launch(pit::pair_residual_kernel<DT, 8>, a.B * a.chunks, pit::kThreads, 0, s, a)); break;
  }
  return launch(pit::assign_kernel<C>, a.B, pit::kThreads, 0, s, a);
}

template <int DT>
int run_grad(const pit::Args& a, hipStream_t s) {
  return launch(pit::pit_grad_kernel<DT>, a.B * a.S * a.gchunks, pit::kThreads, 0, s, a);
}

}  // namespace

extern "C" {

int32_t aamd_pit_tiles(int32_t which) {
  switch (which) {
    case 0: return pit::kThreads;
    case 1: return pit::kGramSpan;
    case 2: return pit::kResChunk;
    case 3: return pit::kMaxS;
    default: return 0;
  }
}

int64_t aamd_pit_workspace(int64_t batch, int64_t sources, int64_t length) {
  if (batch <= 0 || sources < 1 || sources > pit::kMaxS || length < 0 || length >= (1ll << 40)) return 0;
  return layout_of(batch, sources, length).total;
}

int aamd_pit_forward(int32_t dtype, int32_t mode, const void* preds, const void* target, int64_t batch, int64_t sources,
                     int64_t length, int64_t preds_batch_stride, int64_t preds_source_stride, int64_t target_batch_stride,
                     int64_t target_source_stride, const void* lengths, int32_t lengths_int64, int32_t zero_mean,
                     int32_t minimize, void* workspace, void* matrix, void* best_metric, int64_t* best_perm, double* stat,
                     void* stream) {
  DeviceScope dev_scope_(workspace);
  pit::Args a{};
  AAMD_TRY(common("pit_forward", a, dtype, mode, preds, target, batch, sources, length, preds_batch_stride, preds_source_stride,
                  target_batch_stride, target_source_stride, lengths, lengths_int64, zero_mean));
  if (batch == 0) return AAMD_OK;
  AAMD_CHECK_ARG(workspace, "pit_forward: null buffer");
  const uintptr_t omask = (uintptr_t)(comp_size(dtype) - 1);
  AAMD_CHECK_ARG((((uintptr_t)workspace | (uintptr_t)stat | (uintptr_t)best_perm) & 7) == 0 &&
                     (((uintptr_t)matrix | (uintptr_t)best_metric) & omask) == 0, "pit_forward: a buffer is misaligned");
  const Layout l = layout_of(batch, sources, length);
  AAMD_CHECK_ARG(batch * l.gspans < (1ll << 31) && batch * l.chunks < (1ll << 31), "pit_forward: too many workgroups");
  char* ws = static_cast<char*>(workspace);
  a.gram = reinterpret_cast<double*>(ws + l.gram);
  a.pstat = reinterpret_cast<double*>(ws + l.pstat);
  a.res = reinterpret_cast<double*>(ws + l.res);
  a.minimize = minimize ? 1 : 0;
  a.mout = matrix; a.best = best_metric; a.perm = best_perm; a.stat = stat;
  return for_dtype(dtype, [&](auto dt) { return run_forward<dt.value>(a, (hipStream_t)stream); });
}

int aamd_pit_assign(int32_t dtype, const void* matrix, int64_t batch, int64_t sources, int32_t minimize, void* best_metric,
                    int64_t* best_perm, void* stream) {
  DeviceScope dev_scope_(matrix);
  AAMD_CHECK_ARG(dtype == AAMD_SA_F32 || dtype == AAMD_SA_F64, "pit_assign: the matrix must be float32 or float64");
  AAMD_CHECK_ARG(batch >= 0 && batch < (1ll << 31), "pit_assign: bad sizes");
  AAMD_CHECK_ARG(sources >= 1, "pit_assign: at least one source is needed");
  if (sources > pit::kMaxS)
    return fail(AAMD_EUNSUPPORTED, "audio_amd: pit_assign: more than " + std::to_string(pit::kMaxS) + " sources are not implemented");
  if (batch == 0) return AAMD_OK;
  AAMD_CHECK_ARG(matrix && best_metric && best_perm, "pit_assign: null buffer");
  const uintptr_t omask = (uintptr_t)(comp_size(dtype) - 1);
  AAMD_CHECK_ARG((((uintptr_t)matrix | (uintptr_t)best_metric) & omask) == 0 && ((uintptr_t)best_perm & 7) == 0,
                 "pit_assign: a buffer is misaligned");
  pit::Args a{};
  a.B = batch; a.S = (int32_t)sources; a.minimize = minimize ? 1 : 0;
  a.min = matrix; a.best = best_metric; a.perm = best_perm;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == AAMD_SA_F64) return launch(pit::assign_kernel<double>, batch, pit::kThreads, 0, s, a);
  return launch(pit::assign_kernel<float>, batch, pit::kThreads, 0, s, a);
}

int aamd_pit_grad(int32_t dtype, int32_t mode, const void* preds, const void* target, int64_t batch, int64_t sources,
                  int64_t length, int64_t preds_batch_stride, int64_t preds_source_stride, int64_t target_batch_stride,
                  int64_t target_source_stride, const void* lengths, int32_t lengths_int64, const double* stat,
                  const int64_t* perm, const double* cotangent, void* grad_preds, void* grad_target, void* stream) {
  DeviceScope dev_scope_(stat);
  pit::Args a{};
  AAMD_TRY(common("pit_grad", a, dtype, mode, preds, target, batch, sources, length, preds_batch_stride, preds_source_stride,
                  target_batch_stride, target_source_stride, lengths, lengths_int64, 0));
  if (batch == 0 || length == 0 || (!grad_preds && !grad_target)) return AAMD_OK;
  AAMD_CHECK_ARG(stat && perm && cotangent, "pit_grad: null buffer");
  AAMD_CHECK_ARG((((uintptr_t)stat | (uintptr_t)perm | (uintptr_t)cotangent) & 7) == 0 &&
                     (((uintptr_t)grad_preds | (uintptr_t)grad_target) & (uintptr_t)(elem_size(dtype) - 1)) == 0, "pit_grad: a buffer is misaligned");
  a.stat = const_cast<double*>(stat);
  a.perm_in = perm; a.cot = cotangent;
  a.gp = grad_preds; a.gt = grad_target;
  return for_dtype(dtype, [&](auto dt) { return run_grad<dt.value>(a, (hipStream_t)stream); });
}

int aamd_pit_permutate(int32_t elem_bytes, const void* src, const int64_t* perm, int64_t batch, int64_t sources,
                       int64_t row_elems, int64_t src_batch_stride, int64_t src_source_stride, uint64_t fill, void* out,
                       void* stream) {
  DeviceScope dev_scope_(out);
  AAMD_CHECK_ARG(elem_bytes == 1 || elem_bytes == 2 || elem_bytes == 4 || elem_bytes == 8, "pit_permutate: elements of 1, 2, 4 or 8 bytes");
  AAMD_CHECK_ARG(batch >= 0 && sources >= 0 && row_elems >= 0 && src_batch_stride >= 0 && src_source_stride >= 0, "pit_permutate: bad sizes");
  if (batch == 0 || sources == 0 || row_elems == 0) return AAMD_OK;
  AAMD_CHECK_ARG(src && perm && out, "pit_permutate: null buffer");
  AAMD_CHECK_ARG((((uintptr_t)src | (uintptr_t)out) & (uintptr_t)(elem_bytes - 1)) == 0 && ((uintptr_t)perm & 7) == 0,
                 "pit_permutate: a buffer is misaligned");
  pit::GatherArgs g{};
  g.src = src; g.perm = perm; g.out = out;
  g.B = batch; g.S = sources; g.R = row_elems; g.sb = src_batch_stride; g.ss = src_source_stride; g.fill = fill;
  g.chunks = sdr::ceil_div(row_elems, (int64_t)pit::kGatherVecs * pit::kThreads * (16 / elem_bytes));
  AAMD_CHECK_ARG(batch * sources < (1ll << 31) && batch * sources * g.chunks < (1ll << 31), "pit_permutate: too many workgroups");
  hipStream_t s = (hipStream_t)stream;
  const int64_t blocks = batch * sources * g.chunks;
  switch (elem_bytes) {
    case 1: return launch(pit::gather_kernel<uint8_t>, blocks, pit::kThreads, 0, s, g);
    case 2: return launch(pit::gather_kernel<uint16_t>, blocks, pit::kThreads, 0, s, g);
    case 4: return launch(pit::gather_kernel<uint32_t>, blocks, pit::kThreads, 0, s, g);
    default: return launch(pit::gather_kernel<uint64_t>, blocks, pit::kThreads, 0, s, g);
  }
}

}  // extern "C"

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
