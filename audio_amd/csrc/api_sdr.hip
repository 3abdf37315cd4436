// SDR, SI-SDR / SI-SNR and SNR of the C ABI (csrc/sdr.h): exported constants, the workspace query, the forward launches and
// the SI-SDR / SNR backward.
//
// Device pass only: the compiler may form no packed fp32 arithmetic (v_pk_*_f32) in this translation unit, whatever the
// vectoriser's settings.  The kernels' arithmetic is float64 and today's compile holds none either way; the attribute keeps the
// half-type conversions and the float32 stores that way.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif
#include "api_common.h"
#include "sdr.h"

using namespace aamd;

namespace {

struct Layout {
  int64_t chunks, spans, lpad;
  int64_t mom, tail, total;                // byte offsets; tail: the correlation partials (SDR) or the residual partials
};

Layout layout_of(int32_t mode, int64_t rows, int64_t T, int64_t flen) {
  Layout l{};
  l.chunks = T > 0 ? sdr::ceil_div(T, sdr::kChunk) : 1;
  l.spans = T > 0 ? sdr::ceil_div(T, sdr::kSpan) : 1;
  l.lpad = 16 * (flen <= sdr::kLagsSmall ? sdr::kTilesSmall : sdr::kTilesMax);
  l.mom = 0;
  l.tail = rows * l.chunks * sdr::kMom * 8;
  l.total = l.tail + (mode == sdr::kModeSdr ? rows * l.spans * 2 * l.lpad : rows * l.chunks) * 8;
  return l;
}

// the checks every entry point shares; fills what the kernels read of the inputs
int common(const char* who, sdr::Args& a, int32_t dtype, int32_t mode, const void* preds, const void* target, int64_t rows,
           int64_t length, int64_t preds_stride, int64_t target_stride, const void* lengths, int32_t lengths_int64,
           int32_t zero_mean) {
  const std::string w(who);
  AAMD_CHECK_ARG(dtype >= AAMD_SA_F32 && dtype <= AAMD_SA_BF16, w + ": unknown element type");
  AAMD_CHECK_ARG(mode >= sdr::kModeSdr && mode <= sdr::kModeSnr, w + ": unknown mode");
  AAMD_CHECK_ARG(rows >= 0 && length >= 0 && preds_stride >= 0 && target_stride >= 0, w + ": bad sizes");
  AAMD_CHECK_ARG(rows < (1ll << 31) && length < (1ll << 40), w + ": too many rows or samples");
  AAMD_CHECK_ARG(rows <= 1 || (preds_stride >= length && target_stride >= length), w + ": rows overlap");
  AAMD_CHECK_ARG((preds && target) || length == 0 || rows == 0, w + ": null buffer");
  AAMD_CHECK_ARG((((uintptr_t)preds | (uintptr_t)target) & (uintptr_t)(elem_size(dtype) - 1)) == 0,
                 w + ": a waveform is not aligned to its element");
  AAMD_CHECK_ARG(((uintptr_t)lengths & (lengths_int64 ? 7 : 3)) == 0, w + ": lengths is misaligned");
  a.p = preds; a.t = target; a.lengths = lengths;
  a.rows = rows; a.T = length; a.sp = rows > 1 ? preds_stride : 0; a.st = rows > 1 ? target_stride : 0;
  a.len64 = lengths_int64 ? 1 : 0; a.zero_mean = zero_mean ? 1 : 0; a.mode = mode;
  a.eps = comp_eps(dtype);
  a.chunks = length > 0 ? sdr::ceil_div(length, sdr::kChunk) : 1;
  a.spans = length > 0 ? sdr::ceil_div(length, sdr::kSpan) : 1;
  AAMD_CHECK_ARG(rows * a.chunks < (1ll << 31), w + ": too many workgroups");
  return AAMD_OK;
}

template <int DT>
int run_sdr(const sdr::Args& a, hipStream_t s) {
  AAMD_TRY(launch(sdr::moments_kernel<DT>, a.rows * a.chunks, sdr::kThreads, 0, s, a));
  if (a.flen <= sdr::kLagsSmall) {
    AAMD_TRY(launch(sdr::corr_kernel<DT, sdr::kTilesSmall>, a.rows * a.spans, sdr::kThreads, 0, s, a));
    return launch(sdr::solve_kernel<DT, 1>, a.rows, sdr::kSolveThreads, 0, s, a);
  }
  AAMD_TRY(launch(sdr::corr_kernel<DT, sdr::kTilesMax>, a.rows * a.spans, sdr::kThreads, 0, s, a));
  return launch(sdr::solve_kernel<DT, sdr::kLagsMax / 64>, a.rows, sdr::kSolveThreads, 0, s, a);
}

template <int DT>
int run_si(const sdr::Args& a, hipStream_t s) {
  AAMD_TRY(launch(sdr::moments_kernel<DT>, a.rows * a.chunks, sdr::kThreads, 0, s, a));
  AAMD_TRY(launch(sdr::residual_kernel<DT>, a.rows * a.chunks, sdr::kThreads, 0, s, a));
  return launch(sdr::finish_kernel<DT>, a.rows, sdr::kSolveThreads, 0, s, a);
}

template <int DT>
int run_grad(const sdr::Args& a, hipStream_t s) {
  return launch(sdr::grad_kernel<DT>, a.rows * a.chunks, sdr::kThreads, 0, s, a);
}

}  // namespace

extern "C" {

int32_t aamd_sdr_tiles(int32_t which) {
  switch (which) {
    case 0: return sdr::kThreads;
    case 1: return sdr::kChunk;
    case 2: return sdr::kStage;
    case 3: return sdr::kSpan;
    case 4: return sdr::kLagsSmall;
    case 5: return sdr::kLagsMax;
    default: return 0;
  }
}

int64_t aamd_sdr_workspace(int32_t mode, int64_t rows, int64_t length, int64_t filter_length) {
  if (rows <= 0 || length < 0 || length >= (1ll << 40) || filter_length < 1 || filter_length > sdr::kLagsMax) return 0;
  return layout_of(mode, rows, length, filter_length).total;
}

int aamd_sdr(int32_t dtype, const void* preds, const void* target, int64_t rows, int64_t length, int64_t preds_stride,
             int64_t target_stride, const void* lengths, int32_t lengths_int64, int64_t filter_length, int32_t zero_mean,
             int32_t has_load_diag, double load_diag, void* workspace, void* out, void* stream) {
  DeviceScope dev_scope_(out);
  sdr::Args a{};
  AAMD_TRY(common("sdr", a, dtype, sdr::kModeSdr, preds, target, rows, length, preds_stride, target_stride, lengths,
                  lengths_int64, zero_mean));
  AAMD_CHECK_ARG(filter_length >= 1, "sdr: filter_length must be at least 1");
  if (filter_length > sdr::kLagsMax)
    return fail(AAMD_EUNSUPPORTED, "audio_amd: sdr: filter_length above " + std::to_string(sdr::kLagsMax) + " is not implemented");
  if (rows == 0) return AAMD_OK;
  AAMD_CHECK_ARG(workspace && out, "sdr: null buffer");
  AAMD_CHECK_ARG(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)out & (uintptr_t)(comp_size(dtype) - 1)) == 0, "sdr: a buffer is misaligned");
  const Layout l = layout_of(sdr::kModeSdr, rows, length, filter_length);
  AAMD_CHECK_ARG(rows * l.spans < (1ll << 31), "sdr: too many workgroups");
  char* ws = static_cast<char*>(workspace);
  a.flen = (int32_t)filter_length; a.lpad = (int32_t)l.lpad;
  a.has_diag = has_load_diag ? 1 : 0; a.load_diag = load_diag;
  a.mom = reinterpret_cast<double*>(ws + l.mom);
  a.corr = reinterpret_cast<double*>(ws + l.tail);
  a.out = out;
  return for_dtype(dtype, [&](auto dt) { return run_sdr<dt.value>(a, (hipStream_t)stream); });
}

int aamd_si_sdr(int32_t dtype, int32_t mode, const void* preds, const void* target, int64_t rows, int64_t length,
                int64_t preds_stride, int64_t target_stride, const void* lengths, int32_t lengths_int64, int32_t zero_mean,
                void* workspace, double* stat, void* out, void* stream) {
  DeviceScope dev_scope_(out);
  sdr::Args a{};
  AAMD_TRY(common("si_sdr", a, dtype, mode, preds, target, rows, length, preds_stride, target_stride, lengths, lengths_int64,
                  zero_mean));
  AAMD_CHECK_ARG(mode != sdr::kModeSdr, "si_sdr: mode must be 1 (SI-SDR) or 2 (SNR)");
  if (rows == 0) return AAMD_OK;
  AAMD_CHECK_ARG(workspace && out && stat, "si_sdr: null buffer");
  AAMD_CHECK_ARG((((uintptr_t)workspace | (uintptr_t)stat) & 7) == 0 && ((uintptr_t)out & (uintptr_t)(comp_size(dtype) - 1)) == 0,
                 "si_sdr: a buffer is misaligned");
  const Layout l = layout_of(mode, rows, length, 1);
  char* ws = static_cast<char*>(workspace);
  a.mom = reinterpret_cast<double*>(ws + l.mom);
  a.res = reinterpret_cast<double*>(ws + l.tail);
  a.stat = stat;
  a.out = out;
  return for_dtype(dtype, [&](auto dt) { return run_si<dt.value>(a, (hipStream_t)stream); });
}

int aamd_si_sdr_grad(int32_t dtype, int32_t mode, const void* preds, const void* target, int64_t rows, int64_t length,
                     int64_t preds_stride, int64_t target_stride, const void* lengths, int32_t lengths_int64,
                     const double* stat, const double* cotangent, void* grad_preds, void* grad_target, void* stream) {
  DeviceScope dev_scope_(stat);
  sdr::Args a{};
  AAMD_TRY(common("si_sdr_grad", a, dtype, mode, preds, target, rows, length, preds_stride, target_stride, lengths,
                  lengths_int64, 0));
  AAMD_CHECK_ARG(mode != sdr::kModeSdr, "si_sdr_grad: mode must be 1 (SI-SDR) or 2 (SNR)");
  if (rows == 0 || length == 0 || (!grad_preds && !grad_target)) return AAMD_OK;
  AAMD_CHECK_ARG(stat && cotangent, "si_sdr_grad: null buffer");
  AAMD_CHECK_ARG((((uintptr_t)stat | (uintptr_t)cotangent) & 7) == 0 &&
                     (((uintptr_t)grad_preds | (uintptr_t)grad_target) & (uintptr_t)(elem_size(dtype) - 1)) == 0,
                 "si_sdr_grad: a buffer is misaligned");
  a.stat = const_cast<double*>(stat);
  a.cot = cotangent;
  a.gp = grad_preds; a.gt = grad_target;
  a.want_p = grad_preds ? 1 : 0; a.want_t = grad_target ? 1 : 0;
  return for_dtype(dtype, [&](auto dt) { return run_grad<dt.value>(a, (hipStream_t)stream); });
}

}  // extern "C"

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
