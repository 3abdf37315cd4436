// Kaldi-compatible front-end (fbank / spectrogram / mfcc rows) of the C ABI.
#include <cmath>

#include "api_common.h"
#include "kaldi_generic.h"
#include "stft_pow2.h"

using namespace aamd;

extern "C" {

int aamd_kaldi_features_f32(const float* wav, const float* window, const float* twiddle, const aamd_mel_bands* bands,
                            float* out, const aamd_kaldi_desc* d, void* stream) {
  DeviceScope dev_scope_(wav);
  AAMD_CHECK_ARG(d != nullptr && wav && window && twiddle && out, "null buffer");
  AAMD_CHECK_ARG(d->n_samples >= 0 && d->n_frames >= 0, "negative sizes");
  AAMD_CHECK_ARG(d->shift >= 1 && d->win >= 2 && d->win <= d->n_fft, "need shift >= 1 and 2 <= win <= n_fft");
  AAMD_CHECK_ARG(d->preemphasis >= 0.0f && d->preemphasis <= 1.0f, "preemphasis must be in [0, 1]");
  AAMD_CHECK_ARG(d->n_fft % 2 == 0, "the padded window must be even (compliance/kaldi.py:139-141)");
  AAMD_CHECK_ARG(d->dither == 0.0f || d->noise != nullptr, "dither needs the noise buffer");
  if (d->n_frames == 0) return AAMD_OK;
  MelBandsDev mb{};
  if (bands != nullptr) {
    int rc = validate_bands(bands, d->n_fft / 2 + 1, mb);
    if (rc != AAMD_OK) return rc;
    AAMD_CHECK_ARG(d->n_cols >= mb.n_mels && d->first_col >= 0 && d->first_col + mb.n_mels <= d->n_cols &&
                   d->energy_col < d->n_cols, "bad output columns");
  }
  p2::KaldiGeom kg{};
  kg.n_samples = d->n_samples; kg.n_frames = d->n_frames; kg.shift = d->shift; kg.win = d->win;
  kg.snip_edges = d->snip_edges; kg.pad_left = d->win / 2 - d->shift / 2;
  kg.preemph = d->preemphasis; kg.remove_dc = d->remove_dc_offset; kg.raw_energy = d->raw_energy;
  kg.log_energy_floor = d->energy_floor > 0.0f ? std::log(d->energy_floor) : -INFINITY;
  kg.eps = 1.1920928955078125e-07f;
  kg.use_power = d->use_power; kg.use_log = d->use_log;
  kg.energy_col = d->energy_col; kg.first_col = d->first_col; kg.n_cols = d->n_cols;
  kg.noise = d->dither != 0.0f ? d->noise : nullptr; kg.dither = d->dither;
  kg.n_utt = d->n_utt > 1 ? d->n_utt : 1;
  kg.utt_stride = d->n_utt > 1 ? d->utt_stride : d->n_samples;
  AAMD_CHECK_ARG(kg.utt_stride >= d->n_samples, "utt_stride < n_samples");
  const bool pow2 = d->n_fft == 256 || d->n_fft == 512 || d->n_fft == 1024 || d->n_fft == 2048;
  if (!pow2 || force_generic()) {
    // any even padded window: mixed-radix Stockham stages in LDS (csrc/kaldi_generic.h)
    kgen::Plan plan{};
    plan.n_fft = d->n_fft;
    plan.n_stages = plan_radices(d->n_fft, plan.radix);
    if (plan.n_stages < 0 || d->n_fft > 8192)
      return fail(AAMD_EUNSUPPORTED, "audio_amd: padded window too long / too many prime factors for the Kaldi front-end");
    const int pb = kgen::pairs_per_block(d->n_fft);
    size_t lds = kgen::lds_floats(d->n_fft, pb) * sizeof(float);
    const bool long_win = lds > dev_props().lds_per_block_optin;     // ~5 750 .. 8 192: the layout without the LDS twiddle table
    if (long_win) lds = kgen::lds_floats_long(d->n_fft, pb) * sizeof(float);
    if (lds > dev_props().lds_per_block_optin)
      return fail(AAMD_EUNSUPPORTED, "audio_amd: padded window too long for the LDS");
    const int64_t bpu = (d->n_frames + 2 * pb - 1) / (2 * pb);
    const int64_t nblk = bpu * kg.n_utt;
    AAMD_CHECK_ARG(nblk < (1ll << 31), "too many frames for one launch");
    const auto* twg = reinterpret_cast<const cplx<float>*>(twiddle);
    auto kk = bands == nullptr ? (long_win ? kgen::kaldi_generic_kernel<0, 1> : kgen::kaldi_generic_kernel<0>)
                               : (long_win ? kgen::kaldi_generic_kernel<1, 1> : kgen::kaldi_generic_kernel<1>);
    return launch(kk, nblk, kgen::kThreads, lds, (hipStream_t)stream, kg, plan, pb, (int)bpu, wav, window, twg, mb, out);
  }
  const int64_t n_pairs = (d->n_frames + 1) / 2 * kg.n_utt;
  const int64_t blocks = p2::kaldi_blocks(dev_props().cu_count, n_pairs);
  const auto* twc = reinterpret_cast<const p2::C32*>(twiddle);
#define AAMD_KALDI(EE, MODE)                                                                                  \
  return launch(p2::kaldi_pow2_kernel<EE, MODE>, blocks, 64 * p2::kWaves,                                     \
                (size_t)p2::kWaves * p2::Cfg<EE>::lds_complex * sizeof(p2::C32), (hipStream_t)stream, kg, wav, window, twc, mb, out)
  if (bands == nullptr) {
    if (d->n_fft == 256) AAMD_KALDI(4, 0); else if (d->n_fft == 512) AAMD_KALDI(8, 0); else if (d->n_fft == 1024) AAMD_KALDI(16, 0); else AAMD_KALDI(32, 0);
  } else {
    if (d->n_fft == 256) AAMD_KALDI(4, 1); else if (d->n_fft == 512) AAMD_KALDI(8, 1); else if (d->n_fft == 1024) AAMD_KALDI(16, 1); else AAMD_KALDI(32, 1);
  }
#undef AAMD_KALDI
}

}  // extern "C"
