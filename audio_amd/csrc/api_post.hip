// Feature post-processing and augmentation of the C ABI: deltas, sliding-window CMN, pitch, SpecAugment, add_noise,
// preemphasis, MVDR beamforming.
#include "api_common.h"
#include "feat_post.h"
#include "pitch.h"
#include "spec_augment.h"
#include "wave_augment.h"
#include "beamform.h"

using namespace aamd;

namespace {

// ---- feature post-processing: deltas and sliding-window CMN (csrc/feat_post.h) -----------------------------------------
template <typename T>
int compute_deltas(const T* x, T* out, int64_t channels, int64_t n_feat, int64_t n_frames, int64_t sc, int64_t sf,
                          int64_t st, int32_t win_length, int32_t pad_mode, int32_t adjoint, void* stream) {
  DeviceScope dev_scope_(x);
  AAMD_CHECK_ARG(channels >= 0 && n_feat >= 0 && n_frames >= 0, "bad sizes");
  AAMD_CHECK_ARG(win_length >= 3, "win_length must be >= 3");
  AAMD_CHECK_ARG(pad_mode >= AAMD_PAD_REFLECT && pad_mode <= AAMD_PAD_CIRCULAR, "unknown pad mode");
  const int n = (win_length - 1) / 2;
  AAMD_CHECK_ARG(pad_mode != AAMD_PAD_REFLECT || n < n_frames, "reflect padding needs (win_length - 1) / 2 < frames");
  AAMD_CHECK_ARG(pad_mode != AAMD_PAD_CIRCULAR || n <= n_frames, "circular padding needs (win_length - 1) / 2 <= frames");
  if (channels * n_feat * n_frames == 0) return AAMD_OK;
  AAMD_CHECK_ARG(x && out, "null buffer");
  fp::DeltaGeom g;
  if (!fp::delta_plan(g, channels, n_feat, n_frames, sc, sf, st, n, pad_mode, adjoint, (int64_t)sizeof(T)))
    return fail(AAMD_EUNSUPPORTED, "audio_amd: compute_deltas: win_length too large for one LDS tile");
  const int64_t blocks = channels * g.n_ftiles * g.n_ttiles;
  AAMD_CHECK_ARG(blocks < (1ll << 31), "too many tiles for one launch");
  const size_t lds = (size_t)g.tf * g.w * sizeof(T);
  return launch(fp::deltas_kernel<T>, blocks, fp::kDtThreads, lds, (hipStream_t)stream, x, out, g);
}

template <typename T>
int sliding_window_cmn(const T* x, T* out, void* workspace, int64_t channels, int64_t n_frames, int64_t n_feat,
                              int64_t sc, int64_t sf, int64_t st, int64_t cmn_window, int64_t min_cmn_window,
                              int32_t center, int32_t norm_vars, int32_t adjoint, void* stream) {
  DeviceScope dev_scope_(x);
  AAMD_CHECK_ARG(channels >= 0 && n_frames >= 0 && n_feat >= 0, "bad sizes");
  AAMD_CHECK_ARG(cmn_window >= 0, "cmn_window must be >= 0");
  AAMD_CHECK_ARG(!(adjoint && norm_vars), "the adjoint is served for norm_vars = false only");
  if (channels * n_frames * n_feat == 0) return AAMD_OK;
  AAMD_CHECK_ARG(x && out && workspace, "null buffer");
  AAMD_CHECK_ARG(((uintptr_t)workspace & 7) == 0, "workspace must be 8-byte aligned");
  fp::CmnGeom g;
  fp::cmn_plan(g, channels, n_frames, n_feat, sc, st, sf, cmn_window, min_cmn_window, center, norm_vars, adjoint);
  const int64_t blocks = channels * g.n_chunks * g.n_ftiles;
  AAMD_CHECK_ARG(blocks < (1ll << 31), "too many chunks for one launch");
  hipStream_t s = (hipStream_t)stream;
  double* ws = static_cast<double*>(workspace);
  int rc = launch(fp::cmn_chunk_kernel<T>, blocks, g.threads, 0, s, x, ws, g);
  if (rc != AAMD_OK) return rc;
  return launch(fp::cmn_walk_kernel<T>, blocks, g.threads, 0, s, x, ws, out, g);
}

// ---- NCCF pitch tracker (csrc/pitch.h) ------------------------------------------------------------------------------------
template <typename T>
int detect_pitch(const T* x, void* out, void* workspace, int64_t rows, int64_t length, int64_t row_stride,
                        int32_t sample_rate, int32_t frame_size, int32_t lags, int32_t lag_min, int32_t win_length,
                        int32_t mode, void* stream) {
  DeviceScope dev_scope_(x);
  AAMD_CHECK_ARG(rows >= 0 && length >= 0, "bad sizes");
  AAMD_CHECK_ARG(mode == 0 || mode == 1, "mode must be 0 (pitch) or 1 (nccf)");
  AAMD_CHECK_ARG(frame_size >= 1 && lags >= 1, "frame_size and lags must be >= 1");
  AAMD_CHECK_ARG(mode == 1 || (lag_min >= 0 && lag_min < lags / 2), "need 0 <= lag_min < lags / 2");
  AAMD_CHECK_ARG(mode == 1 || win_length >= 3, "win_length must be >= 3");
  if (frame_size > pt::kMaxFrameSize || lags > pt::kMaxLags)
    return fail(AAMD_EUNSUPPORTED, "audio_amd: detect_pitch_frequency: frame size > 8192 or lags > 16384 is not supported");
  pt::PitchGeom g;
  if (!pt::pitch_plan(g, rows, length, row_stride, frame_size, lags, lag_min, mode == 1 ? 3 : win_length,
                      (float)sample_rate, mode, (int64_t)sizeof(T)))
    return fail(AAMD_EUNSUPPORTED, "audio_amd: detect_pitch_frequency: no LDS tile fits these sizes");
  AAMD_CHECK_ARG(mode == 1 || g.n_out >= 1, "fewer than one output frame");
  if (rows == 0 || g.F == 0) return AAMD_OK;
  AAMD_CHECK_ARG(x && out && (mode == 1 || workspace), "null buffer");
  AAMD_CHECK_ARG(rows == 1 || row_stride >= length, "rows must not overlap");
  const int64_t blocks = rows * g.n_ftiles;
  AAMD_CHECK_ARG(blocks < (1ll << 31), "too many frame tiles for one launch");
  hipStream_t s = (hipStream_t)stream;
  const size_t lds = (size_t)pt::pitch_lds_bytes(g, (int64_t)sizeof(T));
  if (lds > 48 * 1024 && lds > dev_props().lds_per_block_optin)
    return fail(AAMD_EUNSUPPORTED, "audio_amd: detect_pitch_frequency: the LDS tile exceeds this device's");
  int32_t* lag = static_cast<int32_t*>(workspace);
  int rc = launch(pt::pitch_nccf_pick_kernel<T>, blocks, pt::kThreads, lds, s, x, g, lag, static_cast<T*>(out));
  if (rc != AAMD_OK || mode == 1) return rc;
  const int64_t mblocks = rows * ((g.n_out + pt::kMedT - 1) / pt::kMedT);
  AAMD_CHECK_ARG(mblocks < (1ll << 31), "too many output tiles for one launch");
  const size_t mlds = pt::pitch_median_tiled(g) ? (size_t)(pt::kMedT + g.win - 1) * sizeof(int) : 0;
  return launch(pt::pitch_median_kernel, mblocks, pt::kThreads, mlds, s, lag, static_cast<float*>(out), g);
}

// ---- SpecAugment masking: a whole policy in one launch (csrc/spec_augment.h) --------------------------------------------
// draws != nullptr: bounds from the raw draws (params); else the shared bounds (starts / ends).
int spec_augment(const void* x, void* out, int64_t examples, int64_t n_outer, int64_t n_inner, int64_t se, int64_t so,
                        int64_t si, int32_t dtype, int32_t time_inner, int32_t n_masks, const int32_t* axes,
                        const int64_t* params, const void* draws, const int64_t* starts, const int64_t* ends,
                        uint64_t value_bits, const void* value_ptr, void* stream) {
  DeviceScope dev_scope_(x);
  AAMD_CHECK_ARG(examples >= 0 && n_outer >= 0 && n_inner >= 0, "bad sizes");
  AAMD_CHECK_ARG(n_outer < (1ll << 31) && n_inner < (1ll << 31), "spec_augment: an axis of 2^31 or more elements");
  AAMD_CHECK_ARG(dtype >= AAMD_SA_F32 && dtype <= AAMD_SA_BF16, "spec_augment: unknown element type");
  AAMD_CHECK_ARG(n_masks >= 0 && n_masks <= sa::kMaxMasks, "spec_augment: at most 32 masks per launch");
  AAMD_CHECK_ARG(n_masks == 0 || axes, "null mask table");
  AAMD_CHECK_ARG(n_masks == 0 || (draws ? params != nullptr : (starts && ends)), "null mask table");
  for (int m = 0; m < n_masks; ++m)
    AAMD_CHECK_ARG(axes[m] == AAMD_SA_FREQ || axes[m] == AAMD_SA_TIME, "spec_augment: a mask axis is AAMD_SA_FREQ or AAMD_SA_TIME");
  if (examples * n_outer * n_inner == 0) return AAMD_OK;
  AAMD_CHECK_ARG(x && out, "null buffer");
  sa::Plan p{};
  p.E = examples; p.O = n_outer; p.I = n_inner;
  p.xe = se; p.xo = so; p.xi = si;
  p.draws = draws; p.value_ptr = value_ptr; p.value_bits = value_bits;
  p.dtype = dtype;
  sa::plan_masks(p, time_inner, n_masks, axes, draws ? params : nullptr, starts, ends);
  const int es = sa::elem_size(dtype);
  const bool dense = sa::plan_is_dense(p, x, out);
  sa::plan_chunks(p, dense, es);
  const int64_t blocks = examples * p.chunks;
  AAMD_CHECK_ARG(blocks < (1ll << 31), "too many examples for one launch");
  hipStream_t s = (hipStream_t)stream;
  auto kern = dense ? (es == 2 ? sa::spec_augment_kernel<2, 1> : es == 4 ? sa::spec_augment_kernel<4, 1> : sa::spec_augment_kernel<8, 1>)
                    : (es == 2 ? sa::spec_augment_kernel<2, 0> : es == 4 ? sa::spec_augment_kernel<4, 0> : sa::spec_augment_kernel<8, 0>);
  return launch(kern, blocks, sa::kThreads, 0, s, x, out, p);
}

// ---- waveform augmentation: add_noise and preemphasis (csrc/wave_augment.h) ----------------------------------------------
template <int DT>
int add_noise_launch(const wa::NoiseArgs& a, int64_t blocks, hipStream_t s) {
  int rc = launch(wa::add_noise_reduce_kernel<DT>, blocks, wa::kThreads, 0, s, a);
  if (rc != AAMD_OK) return rc;
  return launch(wa::add_noise_apply_kernel<DT>, blocks, wa::kThreads, 0, s, a);
}

int add_noise(int32_t dtype, const void* w, const void* n, const void* g, void* out, void* out2, void* workspace,
                     int64_t rows, int64_t length, int64_t sw, int64_t sn, int64_t sg, const double* snr, int64_t ssnr,
                     const int64_t* lengths, int64_t slen, int32_t mode, void* stream) {
  DeviceScope dev_scope_(w);
  AAMD_CHECK_ARG(rows >= 0 && length >= 0, "bad sizes");
  AAMD_CHECK_ARG(mode == AAMD_ADD_NOISE_FORWARD || mode == AAMD_ADD_NOISE_GRADIENT, "add_noise: unknown mode");
  AAMD_CHECK_ARG(sw >= 0 && sn >= 0 && sg >= 0 && ssnr >= 0 && slen >= 0, "add_noise: negative stride");
  if (rows * length == 0) return AAMD_OK;
  AAMD_CHECK_ARG(w && n && out && snr && workspace, "null buffer");
  AAMD_CHECK_ARG(mode == AAMD_ADD_NOISE_FORWARD || (g && out2), "add_noise: the gradient needs a cotangent and two outputs");
  AAMD_CHECK_ARG(((uintptr_t)workspace & 7) == 0, "workspace must be 8-byte aligned");
  wa::NoiseArgs a{};
  a.w = w; a.n = n; a.g = g; a.out = out; a.out2 = out2;
  a.ws = static_cast<double*>(workspace);
  a.snr = snr; a.lengths = lengths;
  a.rows = rows; a.L = length; a.sw = sw; a.sn = sn; a.sg = sg; a.ssnr = ssnr; a.slen = slen;
  a.chunks = wa::n_chunks(length);
  a.grad = mode == AAMD_ADD_NOISE_GRADIENT;
  const int64_t blocks = rows * a.chunks;
  AAMD_CHECK_ARG(blocks < (1ll << 31), "too many chunks for one launch");
  hipStream_t s = (hipStream_t)stream;
  switch (dtype) {
    case AAMD_SA_F32: return add_noise_launch<wa::kF32>(a, blocks, s);
    case AAMD_SA_F64: return add_noise_launch<wa::kF64>(a, blocks, s);
    case AAMD_SA_F16: return add_noise_launch<wa::kF16>(a, blocks, s);
    case AAMD_SA_BF16: return add_noise_launch<wa::kBF16>(a, blocks, s);
    default: return fail(AAMD_EINVAL, "audio_amd: add_noise: unknown element type");
  }
}

int preemphasis(int32_t dtype, const void* x, void* out, int64_t rows, int64_t length, int64_t stride_row, double coeff,
                       int32_t transposed, void* stream) {
  DeviceScope dev_scope_(x);
  AAMD_CHECK_ARG(rows >= 0 && length >= 0 && stride_row >= 0, "bad sizes");
  if (rows * length == 0) return AAMD_OK;
  AAMD_CHECK_ARG(x && out, "null buffer");
  wa::PreArgs a{};
  a.x = x; a.out = out; a.rows = rows; a.L = length; a.sx = stride_row; a.chunks = wa::n_chunks(length);
  a.coeff = coeff; a.transposed = transposed ? 1 : 0;
  const int64_t blocks = rows * a.chunks;
  AAMD_CHECK_ARG(blocks < (1ll << 31), "too many chunks for one launch");
  hipStream_t s = (hipStream_t)stream;
  switch (dtype) {
    case AAMD_SA_F32: return launch(wa::preemphasis_kernel<wa::kF32>, blocks, wa::kThreads, 0, s, a);
    case AAMD_SA_F64: return launch(wa::preemphasis_kernel<wa::kF64>, blocks, wa::kThreads, 0, s, a);
    case AAMD_SA_F16: return launch(wa::preemphasis_kernel<wa::kF16>, blocks, wa::kThreads, 0, s, a);
    case AAMD_SA_BF16: return launch(wa::preemphasis_kernel<wa::kBF16>, blocks, wa::kThreads, 0, s, a);
    default: return fail(AAMD_EINVAL, "audio_amd: preemphasis: unknown element type");
  }
}

// ---- MVDR beamforming: psd, the per-bin solve, apply (csrc/beamform.h) ---------------------------------------------------
int bf_view(bf::SpecView& v, const void* x, int64_t B, int64_t C, int64_t F, int64_t T, int64_t sb, int64_t sc,
                   int64_t sf, int64_t st, int32_t& fmajor) {
  AAMD_CHECK_ARG(B >= 0 && F >= 0 && T >= 0, "beamform: bad sizes");
  if (C > AAMD_BF_MAX_CHANNELS) return fail(AAMD_EINVAL, "audio_amd: beamform: more than 16 channels are not implemented");
  AAMD_CHECK_ARG(C >= 1, "beamform: bad sizes");
  AAMD_CHECK_ARG(sb >= 0 && sc >= 0 && sf >= 0 && st >= 0, "beamform: negative stride");
  AAMD_CHECK_ARG(sf == 1 || st == 1 || F <= 1 || T <= 1, "beamform: the spectrogram needs unit stride along freq or time");
  fmajor = st == 1 ? 0 : (sf == 1 ? 1 : (T <= 1 ? 0 : 1));      // the unit-stride axis; an axis of one element serves as well
  v.p = x; v.sb = sb; v.sc = sc; v.sf = sf; v.st = st;
  return AAMD_OK;
}

template <typename T>
int psd_launch(const bf::PsdArgs& a, int64_t blocks, hipStream_t s) {
  const int no = bf::outputs_per_thread(a.C);
  return launch(no <= 1 ? bf::psd_kernel<T, 1> : no <= 3 ? bf::psd_kernel<T, 3> : bf::psd_kernel<T, 9>, blocks, bf::kThreads, 0, s, a);
}

}  // namespace

extern "C" {

int aamd_compute_deltas_f32(const float* x, float* out, int64_t channels, int64_t n_feat, int64_t n_frames,
                            int64_t stride_channel, int64_t stride_feat, int64_t stride_frame, int32_t win_length,
                            int32_t pad_mode, int32_t adjoint, void* stream) {
  return compute_deltas<float>(x, out, channels, n_feat, n_frames, stride_channel, stride_feat, stride_frame, win_length,
                               pad_mode, adjoint, stream);
}

int aamd_compute_deltas_f64(const double* x, double* out, int64_t channels, int64_t n_feat, int64_t n_frames,
                            int64_t stride_channel, int64_t stride_feat, int64_t stride_frame, int32_t win_length,
                            int32_t pad_mode, int32_t adjoint, void* stream) {
  return compute_deltas<double>(x, out, channels, n_feat, n_frames, stride_channel, stride_feat, stride_frame, win_length,
                                pad_mode, adjoint, stream);
}

int64_t aamd_sliding_window_cmn_workspace(int64_t channels, int64_t n_frames, int64_t n_feat, int32_t norm_vars) {
  if (channels < 0 || n_frames < 0 || n_feat < 0) return 0;
  const int64_t n_chunks = (n_frames + fp::kCmnL - 1) / fp::kCmnL;
  return channels * n_chunks * n_feat * (norm_vars ? 2 : 1) * (int64_t)sizeof(double);
}

int aamd_sliding_window_cmn_f32(const float* x, float* out, void* workspace, int64_t channels, int64_t n_frames,
                                int64_t n_feat, int64_t stride_channel, int64_t stride_feat, int64_t stride_frame,
                                int64_t cmn_window, int64_t min_cmn_window, int32_t center, int32_t norm_vars,
                                int32_t adjoint, void* stream) {
  return sliding_window_cmn<float>(x, out, workspace, channels, n_frames, n_feat, stride_channel, stride_feat, stride_frame,
                                   cmn_window, min_cmn_window, center, norm_vars, adjoint, stream);
}

int aamd_sliding_window_cmn_f64(const double* x, double* out, void* workspace, int64_t channels, int64_t n_frames,
                                int64_t n_feat, int64_t stride_channel, int64_t stride_feat, int64_t stride_frame,
                                int64_t cmn_window, int64_t min_cmn_window, int32_t center, int32_t norm_vars,
                                int32_t adjoint, void* stream) {
  return sliding_window_cmn<double>(x, out, workspace, channels, n_frames, n_feat, stride_channel, stride_feat, stride_frame,
                                    cmn_window, min_cmn_window, center, norm_vars, adjoint, stream);
}

int64_t aamd_detect_pitch_workspace(int64_t rows, int64_t length, int32_t frame_size) {
  if (rows < 0 || length < 0 || frame_size < 1) return 0;
  return rows * ((length + frame_size - 1) / frame_size) * (int64_t)sizeof(int32_t);
}

int aamd_detect_pitch_f32(const float* x, void* out, void* workspace, int64_t rows, int64_t length, int64_t row_stride,
                          int32_t sample_rate, int32_t frame_size, int32_t lags, int32_t lag_min, int32_t win_length,
                          int32_t mode, void* stream) {
  return detect_pitch<float>(x, out, workspace, rows, length, row_stride, sample_rate, frame_size, lags, lag_min, win_length,
                             mode, stream);
}

int aamd_detect_pitch_f64(const double* x, void* out, void* workspace, int64_t rows, int64_t length, int64_t row_stride,
                          int32_t sample_rate, int32_t frame_size, int32_t lags, int32_t lag_min, int32_t win_length,
                          int32_t mode, void* stream) {
  return detect_pitch<double>(x, out, workspace, rows, length, row_stride, sample_rate, frame_size, lags, lag_min,
                              win_length, mode, stream);
}

int aamd_spec_augment_iid(const void* x, void* out, int64_t examples, int64_t n_outer, int64_t n_inner,
                          int64_t stride_example, int64_t stride_outer, int64_t stride_inner, int32_t dtype,
                          int32_t time_inner, int32_t n_masks, const int32_t* axes, const int64_t* mask_params,
                          const void* draws, uint64_t value_bits, const void* value_ptr, void* stream) {
  AAMD_CHECK_ARG(n_masks <= 0 || draws, "spec_augment: null draws");
  return spec_augment(x, out, examples, n_outer, n_inner, stride_example, stride_outer, stride_inner, dtype, time_inner,
                      n_masks, axes, mask_params, draws, nullptr, nullptr, value_bits, value_ptr, stream);
}

int aamd_spec_augment_shared(const void* x, void* out, int64_t examples, int64_t n_outer, int64_t n_inner,
                             int64_t stride_example, int64_t stride_outer, int64_t stride_inner, int32_t dtype,
                             int32_t time_inner, int32_t n_masks, const int32_t* axes, const int64_t* starts,
                             const int64_t* ends, uint64_t value_bits, const void* value_ptr, void* stream) {
  return spec_augment(x, out, examples, n_outer, n_inner, stride_example, stride_outer, stride_inner, dtype, time_inner,
                      n_masks, axes, nullptr, nullptr, starts, ends, value_bits, value_ptr, stream);
}

int64_t aamd_add_noise_workspace(int64_t rows, int64_t length) {
  if (rows < 0 || length < 0) return 0;
  return (rows + rows * wa::n_chunks(length) * 3) * (int64_t)sizeof(double);
}

int aamd_add_noise_f32(const float* waveform, const float* noise, const float* cotangent, float* out, float* out2,
                       void* workspace, int64_t rows, int64_t length, int64_t stride_waveform, int64_t stride_noise,
                       int64_t stride_cotangent, const double* snr, int64_t stride_snr, const int64_t* lengths,
                       int64_t stride_lengths, int32_t mode, void* stream) {
  return add_noise(AAMD_SA_F32, waveform, noise, cotangent, out, out2, workspace, rows, length, stride_waveform, stride_noise,
                   stride_cotangent, snr, stride_snr, lengths, stride_lengths, mode, stream);
}

int aamd_add_noise_f64(const double* waveform, const double* noise, const double* cotangent, double* out, double* out2,
                       void* workspace, int64_t rows, int64_t length, int64_t stride_waveform, int64_t stride_noise,
                       int64_t stride_cotangent, const double* snr, int64_t stride_snr, const int64_t* lengths,
                       int64_t stride_lengths, int32_t mode, void* stream) {
  return add_noise(AAMD_SA_F64, waveform, noise, cotangent, out, out2, workspace, rows, length, stride_waveform, stride_noise,
                   stride_cotangent, snr, stride_snr, lengths, stride_lengths, mode, stream);
}

int aamd_add_noise_lp(const void* waveform, const void* noise, const void* cotangent, void* out, void* out2, void* workspace,
                      int64_t rows, int64_t length, int64_t stride_waveform, int64_t stride_noise, int64_t stride_cotangent,
                      const double* snr, int64_t stride_snr, const int64_t* lengths, int64_t stride_lengths, int32_t dtype,
                      int32_t mode, void* stream) {
  AAMD_CHECK_ARG(dtype == AAMD_SA_F16 || dtype == AAMD_SA_BF16, "add_noise: the low-precision entry takes AAMD_SA_F16 or AAMD_SA_BF16");
  return add_noise(dtype, waveform, noise, cotangent, out, out2, workspace, rows, length, stride_waveform, stride_noise,
                   stride_cotangent, snr, stride_snr, lengths, stride_lengths, mode, stream);
}

int aamd_preemphasis_f32(const float* x, float* out, int64_t rows, int64_t length, int64_t stride_row, double coeff,
                         int32_t transposed, void* stream) {
  return preemphasis(AAMD_SA_F32, x, out, rows, length, stride_row, coeff, transposed, stream);
}

int aamd_preemphasis_f64(const double* x, double* out, int64_t rows, int64_t length, int64_t stride_row, double coeff,
                         int32_t transposed, void* stream) {
  return preemphasis(AAMD_SA_F64, x, out, rows, length, stride_row, coeff, transposed, stream);
}

int aamd_preemphasis_lp(const void* x, void* out, int64_t rows, int64_t length, int64_t stride_row, double coeff, int32_t dtype,
                        int32_t transposed, void* stream) {
  AAMD_CHECK_ARG(dtype == AAMD_SA_F16 || dtype == AAMD_SA_BF16, "preemphasis: the low-precision entry takes AAMD_SA_F16 or AAMD_SA_BF16");
  return preemphasis(dtype, x, out, rows, length, stride_row, coeff, transposed, stream);
}

int32_t aamd_beamform_freq_tile(void) { return bf::kFT; }
int32_t aamd_beamform_time_chunk(void) { return bf::kTCMax; }

int aamd_beamform_psd(int32_t dtype, const void* x, int64_t batch, int64_t channels, int64_t freq, int64_t time,
                      int64_t stride_b, int64_t stride_c, int64_t stride_f, int64_t stride_t, const void* mask1,
                      const int64_t* mask1_strides, const void* mask2, const int64_t* mask2_strides, int32_t normalize,
                      double eps, void* out, void* stream) {
  DeviceScope dev_scope_(x);
  AAMD_CHECK_ARG(dtype == AAMD_BF_C64 || dtype == AAMD_BF_C128, "beamform: unknown element type");
  bf::PsdArgs a{};
  int rc = bf_view(a.x, x, batch, channels, freq, time, stride_b, stride_c, stride_f, stride_t, a.fmajor);
  if (rc != AAMD_OK) return rc;
  AAMD_CHECK_ARG(mask1 || !mask2, "psd: a second mask needs a first one");
  AAMD_CHECK_ARG((!mask1 || mask1_strides) && (!mask2 || mask2_strides), "psd: a mask needs its strides");
  if (batch * freq == 0) return AAMD_OK;
  AAMD_CHECK_ARG(out && (x || time == 0), "null buffer");
  a.mask[0] = mask1; a.mask[1] = mask2;
  const int64_t* ms[2] = {mask1_strides, mask2_strides};
  for (int n = 0; n < 2; ++n)
    if (a.mask[n]) {
      AAMD_CHECK_ARG(ms[n][0] >= 0 && ms[n][1] >= 0 && ms[n][2] >= 0, "psd: negative mask stride");
      a.mb[n] = ms[n][0]; a.mf[n] = ms[n][1]; a.mt[n] = ms[n][2];
    }
  a.out = out; a.B = batch; a.F = freq; a.T = time; a.C = (int32_t)channels;
  a.n_out = mask2 ? 2 : 1; a.normalize = normalize ? 1 : 0; a.eps = eps;
  const int64_t blocks = batch * bf::freq_tiles(freq);
  AAMD_CHECK_ARG(blocks < (1ll << 31), "too many tiles for one launch");
  return dtype == AAMD_BF_C64 ? psd_launch<float>(a, blocks, (hipStream_t)stream) : psd_launch<double>(a, blocks, (hipStream_t)stream);
}

int aamd_beamform_weights(int32_t dtype, int32_t mode, const void* a_, const void* b, const void* reference_vector, void* out,
                          int64_t batch, int64_t freq, int32_t channels, int32_t rhs, int32_t reference, int32_t loading,
                          double diag_eps, double eps, int32_t n_iter, int32_t adjoint, void* stream) {
  DeviceScope dev_scope_(a_);
  AAMD_CHECK_ARG(dtype == AAMD_BF_C64 || dtype == AAMD_BF_C128, "beamform: unknown element type");
  AAMD_CHECK_ARG(mode >= AAMD_BF_SOLVE && mode <= AAMD_BF_RTF_POWER, "beamform: unknown mode");
  AAMD_CHECK_ARG(batch >= 0 && freq >= 0, "beamform: bad sizes");
  if (channels > AAMD_BF_MAX_CHANNELS) return fail(AAMD_EINVAL, "audio_amd: beamform: more than 16 channels are not implemented");
  AAMD_CHECK_ARG(channels >= 1, "beamform: bad sizes");
  if (mode == AAMD_BF_SOUDEN || mode == AAMD_BF_RTF_POWER) rhs = channels;
  if (mode == AAMD_BF_RTF) rhs = 1;
  AAMD_CHECK_ARG(rhs >= 1 && rhs <= channels, "beamform: between 1 and `channels` right-hand sides");
  AAMD_CHECK_ARG(reference < channels, "beamform: the reference channel is out of range");
  AAMD_CHECK_ARG(mode == AAMD_BF_SOLVE || mode == AAMD_BF_RTF || reference >= 0 || reference_vector,
                 "beamform: this mode needs a reference channel or vector");
  AAMD_CHECK_ARG(mode != AAMD_BF_RTF_POWER || n_iter >= 1, "rtf_power: n_iter must be positive");
  AAMD_CHECK_ARG(mode == AAMD_BF_SOLVE || !adjoint, "beamform: adjoint belongs to AAMD_BF_SOLVE");
  const int64_t bins = batch * freq;
  if (bins == 0) return AAMD_OK;
  AAMD_CHECK_ARG(a_ && b && out, "null buffer");
  bf::WArgs a{};
  a.a = a_; a.b = b; a.u = reference >= 0 ? nullptr : reference_vector; a.out = out;
  a.bins = bins; a.F = freq; a.C = channels; a.K = rhs; a.mode = mode; a.ref = reference >= 0 ? reference : -1;
  a.loading = loading ? 1 : 0; a.n_iter = n_iter; a.adjoint = adjoint ? 1 : 0; a.diag_eps = diag_eps; a.eps = eps;
  const int64_t blocks = (bins + bf::kTeams - 1) / bf::kTeams;
  AAMD_CHECK_ARG(blocks < (1ll << 31), "too many bins for one launch");
  return launch(dtype == AAMD_BF_C64 ? bf::weights_kernel<float> : bf::weights_kernel<double>, blocks, bf::kTeam * bf::kTeams, 0,
                (hipStream_t)stream, a);
}

int aamd_beamform_apply(int32_t dtype, const void* w, const void* x, int64_t batch, int64_t channels, int64_t freq,
                        int64_t time, int64_t stride_b, int64_t stride_c, int64_t stride_f, int64_t stride_t, void* out,
                        const int64_t* out_strides, void* stream) {
  DeviceScope dev_scope_(x);
  AAMD_CHECK_ARG(dtype == AAMD_BF_C64 || dtype == AAMD_BF_C128, "beamform: unknown element type");
  bf::ApplyArgs a{};
  int rc = bf_view(a.x, x, batch, channels, freq, time, stride_b, stride_c, stride_f, stride_t, a.fmajor);
  if (rc != AAMD_OK) return rc;
  if (batch * freq * time == 0) return AAMD_OK;
  AAMD_CHECK_ARG(w && x && out && out_strides, "null buffer");
  AAMD_CHECK_ARG(out_strides[0] >= 0 && out_strides[1] >= 1 && out_strides[2] >= 1, "apply_beamforming: bad output strides");
  AAMD_CHECK_ARG((a.fmajor ? out_strides[1] : out_strides[2]) == 1 || (a.fmajor ? freq : time) <= 1,
                 "apply_beamforming: the output needs unit stride along the input's unit-stride axis");
  a.w = w; a.out = out; a.ob = out_strides[0]; a.of = out_strides[1]; a.ot = out_strides[2];
  a.B = batch; a.F = freq; a.T = time; a.C = (int32_t)channels;
  const int U = dtype == AAMD_BF_C64 ? bf::unit_tile<float>() : bf::unit_tile<double>();
  const int64_t blocks = batch * bf::apply_unit_tiles(a.fmajor ? freq : time, U) * bf::apply_line_tiles(a.fmajor ? time : freq);
  AAMD_CHECK_ARG(blocks < (1ll << 31), "too many tiles for one launch");
  return launch(dtype == AAMD_BF_C64 ? bf::apply_kernel<float> : bf::apply_kernel<double>, blocks, bf::kThreads, 0,
                (hipStream_t)stream, a);
}

}  // extern "C"
