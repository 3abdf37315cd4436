// Spectrogram-domain ops of the C ABI: phase vocoder, Griffin-Lim update, MelScale, dB conversions, the MFCC DCT.
#include "api_common.h"
#include "vocoder.h"
#include "db_mfcc.h"

using namespace aamd;

namespace {

// launch geometry of db_group_kernel: one workgroup per kDbChunk elements of one group
int db_grid(int64_t n, int64_t group_size, int64_t* chunks_per_group, int64_t* blocks) {
  const int64_t n_groups = (n + group_size - 1) / group_size;
  *chunks_per_group = (group_size + kDbChunk - 1) / kDbChunk;
  *blocks = n_groups * *chunks_per_group;
  return *blocks < (1ll << 31) ? AAMD_OK : AAMD_EINVAL;
}

}  // namespace

extern "C" {

int aamd_phase_vocoder_f32(const float* spec, const float* phase_advance, float* out, const aamd_vocoder_desc* d,
                           void* stream) {
  DeviceScope dev_scope_(spec);
  AAMD_CHECK_ARG(d != nullptr && spec && phase_advance && out, "null buffer");
  AAMD_CHECK_ARG(d->rows >= 0 && d->n_freq >= 1 && d->n_frames_in >= 0 && d->n_frames_out >= 0, "bad sizes");
  AAMD_CHECK_ARG(d->rate > 0.0, "rate must be positive");
  if (d->rows == 0 || d->n_frames_out == 0) return AAMD_OK;
  VocoderGeom g{d->rows, d->n_freq, d->n_frames_in, d->n_frames_out, d->in_stride_row, d->in_stride_freq,
                d->in_stride_frame, d->out_stride_row, d->out_stride_freq, d->out_stride_frame, d->rate};
  const int64_t chains = d->rows * d->n_freq;
  AAMD_CHECK_ARG((chains + 255) / 256 < (1ll << 31), "too many chains for one launch");
  return launch(phase_vocoder_kernel, (chains + 255) / 256, 256, 0, (hipStream_t)stream, g,
                reinterpret_cast<const cplx<float>*>(spec), phase_advance, reinterpret_cast<cplx<float>*>(out));
}

int aamd_griffinlim_update_f32(const float* rebuilt, float* tprev, const float* magnitude, float* next, int64_t n,
                               float momentum, void* stream) {
  DeviceScope dev_scope_(rebuilt);
  AAMD_CHECK_ARG(rebuilt && tprev && magnitude && next, "null buffer");
  AAMD_CHECK_ARG(n >= 0, "bad size");
  if (n == 0) return AAMD_OK;
  const int blocks = grid_for(n, 256, dev_props().cu_count * 16);
  return launch(griffinlim_update_kernel, blocks, 256, 0, (hipStream_t)stream, reinterpret_cast<const cplx<float>*>(rebuilt),
                reinterpret_cast<cplx<float>*>(tprev), magnitude, reinterpret_cast<cplx<float>*>(next), n, momentum);
}

int aamd_mel_scale_f32(const float* spec, const aamd_mel_bands* bands, float* out, int64_t rows,
                       int32_t n_frames, int32_t n_freq, void* stream) {
  DeviceScope dev_scope_(spec);
  AAMD_CHECK_ARG(spec && out, "null buffer");
  AAMD_CHECK_ARG(rows >= 0 && n_frames >= 0 && n_freq >= 1, "bad sizes");
  MelBandsDev mb;
  int rc = validate_bands(bands, n_freq, mb);
  if (rc != AAMD_OK) return rc;
  const int64_t n_vec = rows * n_frames;
  if (n_vec == 0) return AAMD_OK;
  const size_t lds = ms_lds_floats(mb.n_mels, mb.max_width, n_freq) * sizeof(float);
  if (lds <= 96 * 1024) {                                  // band table + 16 spectrum rows in LDS, persistent workgroups
    const int blocks = grid_for(n_vec, kMsVec, dev_props().cu_count * 8);
    return launch(mel_scale_lds_kernel, blocks, 256, lds, (hipStream_t)stream, spec, mb, out, n_vec, n_freq);
  }
  const int blocks = grid_for(n_vec * mb.n_mels, 256, dev_props().cu_count * 16);
  return launch(mel_scale_kernel, blocks, 256, 0, (hipStream_t)stream, spec, mb, out, n_vec, n_freq);
}

int aamd_amplitude_to_db_f32(const float* x, float* out, int64_t n, float multiplier, float amin,
                             float db_multiplier, float* group_max, int64_t group_size, void* stream) {
  DeviceScope dev_scope_(x);
  AAMD_CHECK_ARG(x && (out || group_max), "null buffer");
  AAMD_CHECK_ARG(n >= 0, "negative size");
  AAMD_CHECK_ARG(group_max == nullptr || group_size >= 1, "group_size must be >= 1");
  if (n == 0) return AAMD_OK;
  const int64_t gs = group_max ? group_size : n;
  int64_t cpg, blocks;
  AAMD_CHECK_ARG(db_grid(n, gs, &cpg, &blocks) == AAMD_OK, "too many chunks for one launch");
  hipStream_t s = (hipStream_t)stream;
  if (group_max == nullptr)
    hipLaunchKernelGGL((db_group_kernel<true, false, false>), dim3((unsigned)blocks), dim3(256), 0, s, x, out, n, multiplier,
                       amin, db_multiplier, group_max, gs, cpg, 0.0f);
  else if (out != nullptr)
    hipLaunchKernelGGL((db_group_kernel<true, true, false>), dim3((unsigned)blocks), dim3(256), 0, s, x, out, n, multiplier,
                       amin, db_multiplier, group_max, gs, cpg, 0.0f);
  else                                                     // maximum only: first pass of a top_db conversion
    hipLaunchKernelGGL((db_group_kernel<false, true, false>), dim3((unsigned)blocks), dim3(256), 0, s, x, out, n, multiplier,
                       amin, db_multiplier, group_max, gs, cpg, 0.0f);
  return launch_check();
}

int aamd_amplitude_to_db_clamped_f32(const float* x, float* out, int64_t n, float multiplier, float amin,
                                     float db_multiplier, const float* group_max, int64_t group_size, float top_db,
                                     void* stream) {
  DeviceScope dev_scope_(x);
  AAMD_CHECK_ARG(x && out && group_max, "null buffer");
  AAMD_CHECK_ARG(n >= 0 && group_size >= 1, "bad sizes");
  if (n == 0) return AAMD_OK;
  int64_t cpg, blocks;
  AAMD_CHECK_ARG(db_grid(n, group_size, &cpg, &blocks) == AAMD_OK, "too many chunks for one launch");
  return launch(db_group_kernel<true, false, true>, blocks, 256, 0, (hipStream_t)stream, x, out, n, multiplier, amin,
                db_multiplier, const_cast<float*>(group_max), group_size, cpg, top_db);
}

int aamd_db_clamp_f32(const float* x, float* out, int64_t n, const float* group_max,
                      int64_t group_size, float top_db, void* stream) {
  DeviceScope dev_scope_(x);
  AAMD_CHECK_ARG(x && out && group_max, "null buffer");
  AAMD_CHECK_ARG(n >= 0 && group_size >= 1, "bad sizes");
  if (n == 0) return AAMD_OK;
  const int blocks = grid_for(n, 256, dev_props().cu_count * 16);
  return launch(db_clamp_kernel, blocks, 256, 0, (hipStream_t)stream, x, out, n, group_max, group_size, top_db);
}

int aamd_mfcc_dct_f32(const float* mel, const float* dct, float* out, int64_t n_vec, int32_t n_mels,
                      int32_t n_mfcc, int32_t log_mode, const float* group_max,
                      int64_t vec_per_group, float top_db, void* stream) {
  DeviceScope dev_scope_(mel);
  AAMD_CHECK_ARG(mel && dct && out, "null buffer");
  AAMD_CHECK_ARG(n_vec >= 0 && n_mels >= 1 && n_mfcc >= 1, "bad sizes");
  AAMD_CHECK_ARG(log_mode >= 0 && log_mode <= 2, "bad log_mode");
  AAMD_CHECK_ARG(vec_per_group >= 1 || group_max == nullptr, "vec_per_group must be >= 1");
  if (n_vec == 0) return AAMD_OK;
  const int nt = (n_mfcc + 15) / 16;
  if (n_mels % 4 == 0 && n_mels <= 16 * kDctMaxChunks && nt <= 4 && reinterpret_cast<uintptr_t>(mel) % 16 == 0 &&
      reinterpret_cast<uintptr_t>(out) % 16 == 0 && !force_generic()) {
    const size_t flds = (size_t)dct_frag_floats(n_mels, n_mfcc) * sizeof(float);
    if (flds <= 64 * 1024) {
      const int64_t tiles = (n_vec + kDctFramesPerTile - 1) / kDctFramesPerTile;
      const int blocks = grid_for(tiles, 4, dev_props().cu_count * 8);
      const int64_t vpg = vec_per_group < 1 ? 1 : vec_per_group;
#define AAMD_DCT(NT)                                                                                      \
  return launch(mfcc_dct_mfma_kernel<NT>, blocks, 256, flds, (hipStream_t)stream, mel, dct, out, n_vec, n_mels, \
                n_mfcc, log_mode, group_max, vpg, top_db)
      switch (nt) {
        case 1: AAMD_DCT(1);
        case 2: AAMD_DCT(2);
        case 3: AAMD_DCT(3);
        default: AAMD_DCT(4);
      }
#undef AAMD_DCT
    }
  }
  const size_t lds = ((size_t)n_mels * n_mfcc + (size_t)kMfccVecPerBlock * n_mels) * sizeof(float);
  if (lds > 160 * 1024) return fail(AAMD_EUNSUPPORTED, "audio_amd: dct matrix too large for LDS");
  const int blocks = grid_for(n_vec, kMfccVecPerBlock, dev_props().cu_count * 8);
  return launch(mfcc_dct_kernel, blocks, 256, lds, (hipStream_t)stream, mel, dct, out, n_vec, n_mels, n_mfcc, log_mode,
                group_max, vec_per_group < 1 ? 1 : vec_per_group, top_db);
}

}  // extern "C"
