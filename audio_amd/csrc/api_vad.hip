// Voice-activity trimming of the C ABI (csrc/vad.h): exported constants, workspace query, the measurement pass (three
// launches) and the trigger pass (one launch, two with the joint start).
#include "api_common.h"
#include "vad.h"

using namespace aamd;

namespace {

int elem_size(int32_t dtype) { return dtype == AAMD_SA_F64 ? 8 : (dtype == AAMD_SA_F32 ? 4 : 2); }

template <int DT>
int measure_launch(const vad::MeasArgs& a, hipStream_t s) {
  const int64_t items = a.rows * a.frames;
  int rc = launch(vad::spec_kernel<DT>, items, vad::kThreads, vad::lds_bytes(a.N), s, a);
  if (rc != AAMD_OK) return rc;
  const int64_t lanes = a.rows * (a.s1 - a.s0);
  rc = launch(vad::smooth_kernel, (lanes + vad::kThreads - 1) / vad::kThreads, vad::kThreads, 0, s, a);
  if (rc != AAMD_OK) return rc;
  return launch(vad::ceps_kernel, items, vad::kThreads, vad::lds_bytes(a.N >> 1), s, a);
}

}  // namespace

extern "C" {

int32_t aamd_vad_tiles(int32_t which) {
  static_assert(vad::kMaxN == AAMD_VAD_MAX_FFT, "the header's limit is the kernels'");
  return which == 0 ? vad::kThreads : (which == 1 ? vad::kMaxN : (which == 2 ? vad::kMinN : (which == 3 ? vad::kTrigThreads : 0)));
}

int64_t aamd_vad_workspace(int64_t rows, int64_t frames, int64_t bins) {
  if (rows <= 0 || frames <= 0 || bins <= 0) return 0;
  return rows * frames * bins * 4;
}

int aamd_vad_measure(int32_t dtype, const void* x, int64_t rows, int64_t length, int64_t row_stride, int32_t win, int32_t n_fft,
                     int32_t period, int32_t s0, int32_t s1, int32_t c0, int32_t c1, int32_t boot_max, double smooth, double up,
                     double down, double noise_reduction, const float* tables, void* workspace, float* meas, int64_t frames,
                     void* stream) {
  DeviceScope dev_scope_(x);
  AAMD_CHECK_ARG(dtype >= AAMD_SA_F32 && dtype <= AAMD_SA_BF16, "vad: unknown element type");
  AAMD_CHECK_ARG(rows >= 0 && length >= 0 && row_stride >= 0, "vad: bad sizes");
  AAMD_CHECK_ARG(n_fft >= vad::kMinN && (n_fft & (n_fft - 1)) == 0, "vad: the transform size must be a power of two, at least 16");
  if (n_fft > AAMD_VAD_MAX_FFT) return fail(AAMD_EUNSUPPORTED, "audio_amd: vad: the kernels serve transforms up to 8192 points");
  AAMD_CHECK_ARG(win >= 1 && win <= n_fft && period >= 1, "vad: the measurement needs 1 <= samples <= transform size and a period >= 1");
  AAMD_CHECK_ARG(s0 >= 1 && s0 < s1 && s1 <= n_fft / 2, "vad: the spectrum range must satisfy 1 <= s0 < s1 <= n_fft / 2");
  AAMD_CHECK_ARG(c0 >= 0 && c0 < c1 && c1 <= n_fft / 4, "vad: the cepstrum range must satisfy 0 <= c0 < c1 <= n_fft / 4");
  AAMD_CHECK_ARG(boot_max >= 0, "vad: negative boot count");
  AAMD_CHECK_ARG(frames == vad::n_frames(length, win, period), "vad: frames does not match length, samples and period");
  AAMD_CHECK_ARG(rows < (1ll << 31) && length < (1ll << 40), "vad: too many rows or samples");
  if (rows == 0 || frames == 0) return AAMD_OK;
  AAMD_CHECK_ARG(rows * frames < (1ll << 31) && rows * (int64_t)(s1 - s0) < (1ll << 38), "vad: too many workgroups");
  AAMD_CHECK_ARG(x && tables && workspace && meas, "null buffer");
  AAMD_CHECK_ARG(((uintptr_t)x & (uintptr_t)(elem_size(dtype) - 1)) == 0, "vad: the waveform is not aligned to its element");
  AAMD_CHECK_ARG((((uintptr_t)tables | (uintptr_t)workspace | (uintptr_t)meas) & 3) == 0, "vad: a float buffer is misaligned");
  vad::MeasArgs a{};
  a.x = x; a.w = tables; a.cw = tables + win; a.tw = tables + win + (s1 - s0);
  a.d = static_cast<float*>(workspace); a.meas = meas;
  a.rows = rows; a.T = length; a.sx = rows > 1 ? row_stride : 0; a.frames = frames;
  a.smooth = smooth; a.up = (float)up; a.down = (float)down; a.nra = (float)noise_reduction;
  a.L = win; a.N = n_fft; a.logN = 0;
  while ((1 << a.logN) < n_fft) ++a.logN;
  a.P = period; a.s0 = s0; a.s1 = s1; a.c0 = c0; a.c1 = c1; a.boot_max = boot_max;
  if (vad::lds_bytes(n_fft) > 48 * 1024 && vad::lds_bytes(n_fft) > dev_props().lds_per_block_optin)
    return fail(AAMD_EUNSUPPORTED, "audio_amd: vad: this device has less LDS than the transform was planned for");
  hipStream_t s = (hipStream_t)stream;
  switch (dtype) {
    case AAMD_SA_F32: return measure_launch<wa::kF32>(a, s);
    case AAMD_SA_F64: return measure_launch<wa::kF64>(a, s);
    case AAMD_SA_F16: return measure_launch<wa::kF16>(a, s);
    default: return measure_launch<wa::kBF16>(a, s);
  }
}

int aamd_vad_trigger(const float* meas, int64_t rows, int64_t frames, int64_t ring, int64_t gap, int64_t period, int64_t fixed,
                     double trigger_level, double trigger_mult, int64_t* first, int64_t* start, int64_t* joint, void* stream) {
  DeviceScope dev_scope_(first);
  AAMD_CHECK_ARG(rows >= 0 && frames >= 0 && rows < (1ll << 31) && frames < (1ll << 31), "vad: bad sizes");
  AAMD_CHECK_ARG(ring >= 1 && ring < (1ll << 31) && gap >= 0 && gap < (1ll << 31), "vad: the ring needs 1 <= length and a gap >= 0");
  AAMD_CHECK_ARG(period >= 1 && period < (1ll << 31) && fixed >= 0 && fixed < (1ll << 40), "vad: bad period or pre-trigger samples");
  AAMD_CHECK_ARG(rows == 0 || (first && start), "null buffer");
  AAMD_CHECK_ARG(rows == 0 || frames == 0 || meas, "null buffer");
  AAMD_CHECK_ARG((((uintptr_t)first | (uintptr_t)start | (uintptr_t)joint) & 7) == 0 && ((uintptr_t)meas & 3) == 0,
                 "vad: a buffer is misaligned");
  vad::TrigArgs a{};
  a.meas = meas; a.rows = rows; a.frames = frames; a.M = ring; a.gap = gap; a.P = period; a.fixed = fixed;
  a.level = trigger_level; a.trig = trigger_mult; a.first = first; a.start = start; a.joint = joint;
  hipStream_t s = (hipStream_t)stream;
  if (rows > 0) {
    const int rc = launch(vad::trigger_kernel, (rows + vad::kTrigThreads - 1) / vad::kTrigThreads, vad::kTrigThreads, 0, s, a);
    if (rc != AAMD_OK) return rc;
  }
  return joint ? launch(vad::joint_kernel, 1, vad::kThreads, 0, s, a) : AAMD_OK;
}

}  // extern "C"
