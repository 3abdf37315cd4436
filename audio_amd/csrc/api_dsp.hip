// Synthesis ops of the C ABI (csrc/dsp_synth.h): oscillator bank, time-varying FIR, the two filter designers, extend_pitch;
// the first-order adjoints of the first two (csrc/dsp_synth_grad.h).
#include "api_common.h"
#include "dsp_synth_grad.h"

using namespace aamd;

namespace {

bool aligned(const void* p, int32_t dtype) {
  const uintptr_t el = dtype == AAMD_SA_F64 ? 7 : (dtype == AAMD_SA_F32 ? 3 : 1);
  return ((uintptr_t)p & el) == 0;
}

#define AAMD_DSP_DISPATCH(dtype, KERNEL, ...)                                        \
  switch (dtype) {                                                                   \
    case AAMD_SA_F32: return launch(KERNEL<wa::kF32>, __VA_ARGS__);                  \
    case AAMD_SA_F64: return launch(KERNEL<wa::kF64>, __VA_ARGS__);                  \
    case AAMD_SA_F16: return launch(KERNEL<wa::kF16>, __VA_ARGS__);                  \
    default: return launch(KERNEL<wa::kBF16>, __VA_ARGS__);                          \
  }

int osc_sums(int32_t dtype, const dsp::OscArgs& a, hipStream_t s) {
  AAMD_DSP_DISPATCH(dtype, dsp::osc_sums_kernel, a.rows * (a.chunks - 1), dsp::kThreads, 0, s, a)
}
int osc_apply(int32_t dtype, const dsp::OscArgs& a, hipStream_t s) {
  AAMD_DSP_DISPATCH(dtype, dsp::osc_apply_kernel, a.rows * a.chunks, dsp::kThreads, 0, s, a)
}
int fw(int32_t dtype, const dsp::FwArgs& a, size_t lds, hipStream_t s) {
  AAMD_DSP_DISPATCH(dtype, dsp::fw_kernel, a.rows * a.tiles, dsp::kThreads, lds, s, a)
}
int pitch(int32_t dtype, const dsp::PitchArgs& a, int64_t blocks, hipStream_t s) {
  AAMD_DSP_DISPATCH(dtype, dsp::pitch_kernel, blocks, dsp::kThreads, 0, s, a)
}

int fw_gx(int32_t dtype, const dsp::FwGradArgs& a, size_t lds, hipStream_t s) {
  AAMD_DSP_DISPATCH(dtype, dsp::fw_gx_kernel, a.rows * a.tiles, dsp::kThreads, lds, s, a)
}
int fw_gh(int32_t dtype, const dsp::FwGradArgs& a, hipStream_t s) {
  AAMD_DSP_DISPATCH(dtype, dsp::fw_gh_kernel, a.rows * a.units * a.lag_tiles, dsp::kThreads, 0, s, a)
}
int fw_gh_fold(int32_t dtype, const dsp::FwGradArgs& a, int64_t blocks, hipStream_t s) {
  AAMD_DSP_DISPATCH(dtype, dsp::fw_gh_fold_kernel, blocks, dsp::kThreads, 0, s, a)
}
int osc_grad_totals(int32_t dtype, const dsp::OscGradArgs& a, hipStream_t s) {
  AAMD_DSP_DISPATCH(dtype, dsp::osc_grad_totals_kernel, a.o.rows * (a.o.chunks - 1), dsp::kThreads, 0, s, a)
}
int osc_grad_apply(int32_t dtype, const dsp::OscGradArgs& a, hipStream_t s) {
  AAMD_DSP_DISPATCH(dtype, dsp::osc_grad_apply_kernel, a.o.rows * a.o.chunks, dsp::kThreads, 0, s, a)
}

bool any_float(int32_t dtype) { return dtype == AAMD_SA_F32 || dtype == AAMD_SA_F64 || dtype == AAMD_SA_F16 || dtype == AAMD_SA_BF16; }

}  // namespace

extern "C" {

int32_t aamd_dsp_tiles(int32_t which) {
  static_assert(dsp::kMaxTaps == AAMD_DSP_MAX_TAPS && dsp::kMaxOsc == AAMD_DSP_MAX_OSCILLATORS &&
                dsp::kMaxMags == AAMD_DSP_MAX_MAGNITUDES, "the header's limits are the kernels'");
  static_assert(wa::kF32 == AAMD_SA_F32 && wa::kF64 == AAMD_SA_F64 && wa::kF16 == AAMD_SA_F16 && wa::kBF16 == AAMD_SA_BF16,
                "the element codes are the header's");
  static_assert(dsp::kSum == AAMD_DSP_SUM && dsp::kMean == AAMD_DSP_MEAN && dsp::kNone == AAMD_DSP_NONE, "the reduction codes");
  switch (which) {
    case 0: return dsp::kOscChunk;
    case 1: return dsp::kFwTile;
    case 2: return dsp::kMaxTaps;
    case 3: return dsp::kMaxOsc;
    case 4: return dsp::kMaxMags;
    default: return 0;
  }
}

int64_t aamd_oscillator_workspace(int64_t rows, int64_t time, int64_t n) {
  if (rows < 0 || time < 0 || n < 0) return -1;
  const int64_t chunks = (time + dsp::kOscChunk - 1) / dsp::kOscChunk;
  return rows * chunks * n * (int64_t)sizeof(double);
}

int aamd_oscillator_bank(int32_t dtype, const void* freq, const void* amp, void* out, void* workspace, int64_t rows, int64_t time,
                         int64_t n, int64_t freq_row_stride, int64_t amp_row_stride, double sample_rate, int32_t reduction,
                         void* stream) {
  DeviceScope dev_scope_(out);
  AAMD_CHECK_ARG(any_float(dtype), "oscillator_bank: the element type must be float32, float64, float16 or bfloat16");
  AAMD_CHECK_ARG(reduction == AAMD_DSP_SUM || reduction == AAMD_DSP_MEAN || reduction == AAMD_DSP_NONE, "oscillator_bank: bad reduction");
  AAMD_CHECK_ARG(rows >= 0 && time >= 0 && n >= 0 && freq_row_stride >= 0 && amp_row_stride >= 0, "oscillator_bank: bad sizes");
  if (n > AAMD_DSP_MAX_OSCILLATORS) return fail(AAMD_EUNSUPPORTED, "audio_amd: oscillator_bank: the kernel serves up to 256 oscillators");
  if (rows == 0 || time == 0 || n == 0) return AAMD_OK;       // an empty sum is the caller's fill
  const int64_t chunks = (time + dsp::kOscChunk - 1) / dsp::kOscChunk;
  AAMD_CHECK_ARG(rows < (1ll << 31) && chunks < (1ll << 31) && rows * chunks < (1ll << 31), "oscillator_bank: too many workgroups");
  AAMD_CHECK_ARG(freq && amp && out && (workspace || chunks == 1), "null buffer");
  AAMD_CHECK_ARG(aligned(freq, dtype) && aligned(amp, dtype) && aligned(out, dtype) && ((uintptr_t)workspace & 7) == 0,
                 "oscillator_bank: a buffer is misaligned");
  dsp::OscArgs a{};
  a.freq = freq; a.amp = amp; a.out = out; a.sums = static_cast<double*>(workspace);
  a.rows = rows; a.T = time; a.sf = freq_row_stride; a.sa = amp_row_stride; a.chunks = chunks;
  a.sample_rate = sample_rate; a.N = (int32_t)n; a.reduction = reduction;
  hipStream_t s = (hipStream_t)stream;
  if (chunks > 1) {
    const int rc = osc_sums(dtype, a, s);
    if (rc != AAMD_OK) return rc;
  }
  return osc_apply(dtype, a, s);
}

int aamd_filter_waveform(int32_t dtype, const void* x, const void* kernels, void* out, int64_t rows, int64_t time,
                         int64_t row_stride, int64_t num_filters, int32_t taps, int32_t batched, void* stream) {
  DeviceScope dev_scope_(out);
  AAMD_CHECK_ARG(any_float(dtype), "filter_waveform: the element type must be float32, float64, float16 or bfloat16");
  AAMD_CHECK_ARG(rows >= 0 && time >= 0 && row_stride >= 0 && num_filters >= 1 && taps >= 1, "filter_waveform: bad sizes");
  AAMD_CHECK_ARG(time % num_filters == 0, "filter_waveform: the length is not a multiple of the number of filters");
  if (taps > AAMD_DSP_MAX_TAPS) return fail(AAMD_EUNSUPPORTED, "audio_amd: filter_waveform: the kernel serves filters up to 2049 taps");
  if (rows == 0 || time == 0) return AAMD_OK;
  const int64_t tiles = (time + dsp::kFwTile - 1) / dsp::kFwTile;
  AAMD_CHECK_ARG(rows < (1ll << 31) && time < (1ll << 40) && rows * tiles < (1ll << 31), "filter_waveform: too many workgroups");
  AAMD_CHECK_ARG(x && kernels && out, "null buffer");
  AAMD_CHECK_ARG(aligned(x, dtype) && aligned(kernels, dtype) && aligned(out, dtype), "filter_waveform: a buffer is misaligned");
  dsp::FwArgs a{};
  a.x = x; a.h = kernels; a.out = out;
  a.rows = rows; a.T = time; a.sx = row_stride; a.F = num_filters; a.C = time / num_filters; a.tiles = tiles;
  a.L = taps; a.batched = batched ? 1 : 0;
  const size_t lds = dsp::fw_lds_values(taps) * (dtype == AAMD_SA_F64 ? 8 : 4);
  return fw(dtype, a, lds, (hipStream_t)stream);
}

int32_t aamd_dsp_grad_tiles(int32_t which) {
  switch (which) {
    case 0: return dsp::kGhPiece;
    case 1: return dsp::kGhLags;
    default: return 0;
  }
}

int64_t aamd_oscillator_grad_workspace(int64_t rows, int64_t time, int64_t n) {
  if (rows < 0 || time < 0 || n < 0) return -1;
  const int64_t chunks = (time + dsp::kOscChunk - 1) / dsp::kOscChunk;
  return 2 * rows * chunks * n * (int64_t)sizeof(double);          // the chunk sums of w, the chunk totals of q
}

int aamd_oscillator_bank_grad(int32_t dtype, const void* freq, const void* amp, const void* grad_out, void* grad_freq, void* grad_amp,
                              void* workspace, int64_t rows, int64_t time, int64_t n, int64_t freq_row_stride, int64_t amp_row_stride,
                              double sample_rate, int32_t reduction, void* stream) {
  DeviceScope dev_scope_(grad_out);
  AAMD_CHECK_ARG(any_float(dtype), "oscillator_bank_grad: the element type must be float32, float64, float16 or bfloat16");
  AAMD_CHECK_ARG(reduction == AAMD_DSP_SUM || reduction == AAMD_DSP_MEAN || reduction == AAMD_DSP_NONE, "oscillator_bank_grad: bad reduction");
  AAMD_CHECK_ARG(rows >= 0 && time >= 0 && n >= 0 && freq_row_stride >= 0 && amp_row_stride >= 0, "oscillator_bank_grad: bad sizes");
  if (n > AAMD_DSP_MAX_OSCILLATORS) return fail(AAMD_EUNSUPPORTED, "audio_amd: oscillator_bank_grad: the kernel serves up to 256 oscillators");
  if (rows == 0 || time == 0 || n == 0 || (!grad_freq && !grad_amp)) return AAMD_OK;
  const int64_t chunks = (time + dsp::kOscChunk - 1) / dsp::kOscChunk;
  AAMD_CHECK_ARG(rows < (1ll << 31) && chunks < (1ll << 31) && rows * chunks < (1ll << 31), "oscillator_bank_grad: too many workgroups");
  AAMD_CHECK_ARG(freq && amp && grad_out && (workspace || chunks == 1), "null buffer");
  AAMD_CHECK_ARG(aligned(freq, dtype) && aligned(amp, dtype) && aligned(grad_out, dtype) && aligned(grad_freq, dtype) &&
                     aligned(grad_amp, dtype) && ((uintptr_t)workspace & 7) == 0,
                 "oscillator_bank_grad: a buffer is misaligned");
  dsp::OscGradArgs a{};
  a.o.freq = freq; a.o.amp = amp; a.o.sums = static_cast<double*>(workspace);
  a.o.rows = rows; a.o.T = time; a.o.sf = freq_row_stride; a.o.sa = amp_row_stride; a.o.chunks = chunks;
  a.o.sample_rate = sample_rate; a.o.N = (int32_t)n; a.o.reduction = reduction;
  a.g = grad_out; a.gf = grad_freq; a.ga = grad_amp;
  a.tots = chunks > 1 ? static_cast<double*>(workspace) + rows * chunks * n : nullptr;
  hipStream_t s = (hipStream_t)stream;
  if (chunks > 1) {
    dsp::OscArgs o = a.o;
    int rc = osc_sums(dtype, o, s);
    if (rc == AAMD_OK && grad_freq) rc = osc_grad_totals(dtype, a, s);
    if (rc != AAMD_OK) return rc;
  }
  return osc_grad_apply(dtype, a, s);
}

int64_t aamd_filter_waveform_grad_workspace(int64_t rows, int64_t time, int64_t num_filters, int32_t taps, int32_t batched) {
  if (rows < 0 || time < 0 || num_filters < 1 || taps < 1 || time % num_filters != 0) return -1;
  if (rows == 0 || time == 0) return 0;
  dsp::FwGradArgs a{};
  a.rows = rows; a.T = time; a.F = num_filters; a.C = time / num_filters; a.L = taps; a.batched = batched ? 1 : 0;
  dsp::fw_grad_geom(a);
  return a.direct ? 0 : rows * num_filters * a.P * taps * (int64_t)sizeof(double);
}

int aamd_filter_waveform_grad(int32_t dtype, const void* x, const void* kernels, const void* grad_out, void* grad_x, void* grad_kernels,
                              void* workspace, int64_t rows, int64_t time, int64_t row_stride, int64_t num_filters, int32_t taps,
                              int32_t batched, void* stream) {
  DeviceScope dev_scope_(grad_out);
  AAMD_CHECK_ARG(any_float(dtype), "filter_waveform_grad: the element type must be float32, float64, float16 or bfloat16");
  AAMD_CHECK_ARG(rows >= 0 && time >= 0 && row_stride >= 0 && num_filters >= 1 && taps >= 1, "filter_waveform_grad: bad sizes");
  AAMD_CHECK_ARG(time % num_filters == 0, "filter_waveform_grad: the length is not a multiple of the number of filters");
  if (taps > AAMD_DSP_MAX_TAPS) return fail(AAMD_EUNSUPPORTED, "audio_amd: filter_waveform_grad: the kernel serves filters up to 2049 taps");
  if (rows == 0 || time == 0 || (!grad_x && !grad_kernels)) return AAMD_OK;      // no samples: grad_kernels is the caller's fill
  const int64_t tiles = (time + dsp::kFwTile - 1) / dsp::kFwTile;
  dsp::FwGradArgs a{};
  a.x = x; a.h = kernels; a.g = grad_out; a.gx = grad_x; a.gh = grad_kernels; a.ws = static_cast<double*>(workspace);
  a.rows = rows; a.T = time; a.sx = row_stride; a.F = num_filters; a.C = time / num_filters; a.tiles = tiles;
  a.L = taps; a.batched = batched ? 1 : 0;
  dsp::fw_grad_geom(a);
  AAMD_CHECK_ARG(rows < (1ll << 31) && time < (1ll << 40) && rows * tiles < (1ll << 31) &&
                     rows * a.units < (1ll << 31) / a.lag_tiles,
                 "filter_waveform_grad: too many workgroups");
  AAMD_CHECK_ARG(grad_out && (!grad_x || kernels) && (!grad_kernels || x) && (!grad_kernels || a.direct || workspace), "null buffer");
  AAMD_CHECK_ARG(aligned(x, dtype) && aligned(kernels, dtype) && aligned(grad_out, dtype) && aligned(grad_x, dtype) &&
                     aligned(grad_kernels, dtype) && ((uintptr_t)workspace & 7) == 0,
                 "filter_waveform_grad: a buffer is misaligned");
  hipStream_t s = (hipStream_t)stream;
  if (grad_x) {
    const int rc = fw_gx(dtype, a, dsp::fw_lds_values(taps) * (dtype == AAMD_SA_F64 ? 8 : 4), s);
    if (rc != AAMD_OK) return rc;
  }
  if (!grad_kernels) return AAMD_OK;
  const int rc = fw_gh(dtype, a, s);
  if (rc != AAMD_OK || a.direct) return rc;
  const int64_t count = (a.batched ? rows : 1) * num_filters * taps;
  return fw_gh_fold(dtype, a, (count + dsp::kThreads - 1) / dsp::kThreads, s);
}

int aamd_sinc_impulse_response(int32_t dtype, const void* cutoff, void* out, int64_t rows, int32_t window_size, int32_t high_pass,
                               void* stream) {
  DeviceScope dev_scope_(out);
  AAMD_CHECK_ARG(dtype == AAMD_SA_F32 || dtype == AAMD_SA_F64, "sinc_impulse_response: the element type must be float32 or float64");
  AAMD_CHECK_ARG(window_size >= 1 && (window_size & 1), "sinc_impulse_response: window_size must be odd and positive");
  AAMD_CHECK_ARG(rows >= 0 && rows < (1ll << 31), "sinc_impulse_response: bad sizes");
  if (rows == 0) return AAMD_OK;
  AAMD_CHECK_ARG(cutoff && out, "null buffer");
  AAMD_CHECK_ARG(aligned(cutoff, dtype) && aligned(out, dtype), "sinc_impulse_response: a buffer is misaligned");
  dsp::SincArgs a{};
  a.cutoff = cutoff; a.out = out; a.rows = rows; a.W = window_size; a.high_pass = high_pass ? 1 : 0;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == AAMD_SA_F64) return launch(dsp::sinc_kernel<wa::kF64>, rows, dsp::kThreads, 0, s, a);
  return launch(dsp::sinc_kernel<wa::kF32>, rows, dsp::kThreads, 0, s, a);
}

int aamd_frequency_impulse_response(int32_t dtype, const void* magnitudes, const void* table, void* out, int64_t rows, int32_t n,
                                    void* stream) {
  DeviceScope dev_scope_(out);
  AAMD_CHECK_ARG(dtype == AAMD_SA_F32 || dtype == AAMD_SA_F64, "frequency_impulse_response: the element type must be float32 or float64");
  AAMD_CHECK_ARG(n >= 2, "frequency_impulse_response: at least two magnitudes");
  if (n > AAMD_DSP_MAX_MAGNITUDES)
    return fail(AAMD_EUNSUPPORTED, "audio_amd: frequency_impulse_response: the kernel serves up to 4097 magnitudes");
  AAMD_CHECK_ARG(rows >= 0 && rows < (1ll << 31), "frequency_impulse_response: bad sizes");
  if (rows == 0) return AAMD_OK;
  AAMD_CHECK_ARG(magnitudes && table && out, "null buffer");
  AAMD_CHECK_ARG(aligned(magnitudes, dtype) && aligned(table, dtype) && aligned(out, dtype), "frequency_impulse_response: a buffer is misaligned");
  dsp::FirArgs a{};
  a.mags = magnitudes; a.table = table; a.out = out; a.rows = rows; a.n = n;
  const size_t lds = ((size_t)n + 2 * ((size_t)n - 1)) * (dtype == AAMD_SA_F64 ? 8 : 4);
  if (lds > 48 * 1024 && dev_props().ok && lds > dev_props().lds_per_block_optin)
    return fail(AAMD_EUNSUPPORTED, "audio_amd: frequency_impulse_response: the tables do not fit the device's LDS");
  hipStream_t s = (hipStream_t)stream;
  if (dtype == AAMD_SA_F64) return launch(dsp::fir_kernel<wa::kF64>, rows, dsp::kThreads, lds, s, a);
  return launch(dsp::fir_kernel<wa::kF32>, rows, dsp::kThreads, lds, s, a);
}

int aamd_extend_pitch(int32_t dtype, const void* base, const void* pattern, void* out, int64_t count, int64_t n, void* stream) {
  DeviceScope dev_scope_(out);
  AAMD_CHECK_ARG(any_float(dtype), "extend_pitch: the element type must be float32, float64, float16 or bfloat16");
  AAMD_CHECK_ARG(count >= 0 && n >= 0, "extend_pitch: bad sizes");
  if (count == 0 || n == 0) return AAMD_OK;
  AAMD_CHECK_ARG(count < (1ll << 38) / n, "extend_pitch: too many workgroups");
  AAMD_CHECK_ARG(base && pattern && out, "null buffer");
  AAMD_CHECK_ARG(aligned(base, dtype) && aligned(pattern, dtype) && aligned(out, dtype), "extend_pitch: a buffer is misaligned");
  dsp::PitchArgs a{};
  a.base = base; a.pattern = pattern; a.out = out; a.M = count; a.N = n;
  return pitch(dtype, a, (count * n + dsp::kThreads - 1) / dsp::kThreads, (hipStream_t)stream);
}

}  // extern "C"
