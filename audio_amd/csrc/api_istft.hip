// Inverse STFT (and the STFT adjoint) of the C ABI.
#include "api_common.h"
#include "istft400.h"
#include "istft.h"
#include "stft_pow2.h"

using namespace aamd;

extern "C" {

int aamd_istft_f32(const float* spec, const float* window, const float* twiddle, const float* inv_envelope,
                   float* out, const aamd_stft_desc* desc, int32_t adjoint, void* stream) {
  DeviceScope dev_scope_(spec);
  AAMD_CHECK_ARG(desc != nullptr && spec && window && twiddle && out, "null buffer");
  AAMD_CHECK_ARG(desc->rows >= 0 && desc->length >= 0 && desc->n_frames >= 0, "negative sizes");
  AAMD_CHECK_ARG(desc->n_fft >= 2 && desc->hop >= 1 && desc->pad >= 0, "n_fft must be >= 2, hop >= 1, pad >= 0");
  AAMD_CHECK_ARG(desc->pad_mode >= 0 && desc->pad_mode <= 3, "bad pad_mode");
  if (!desc->onesided) return fail(AAMD_EUNSUPPORTED, "audio_amd: inverse STFT needs a onesided spectrum");
  if (desc->rows == 0 || desc->length == 0 || desc->n_frames == 0) return AAMD_OK;
  OlaGeom og{};
  StftGeom& g = og.g;
  g.rows = desc->rows; g.length = desc->length; g.row_stride = desc->length;
  g.n_fft = desc->n_fft; g.hop = desc->hop; g.pad = desc->pad; g.center = desc->center;
  g.pad_mode = desc->pad_mode; g.onesided = 1; g.n_frames = desc->n_frames;
  g.n_freq = desc->n_fft / 2 + 1;
  g.scale = 1.0f; g.power = 0.0f;
  g.n_stages = plan_radices(desc->n_fft, g.radix);
  if (g.n_stages < 0) return fail(AAMD_EUNSUPPORTED, "audio_amd: n_fft has too many prime factors");
  og.interior = adjoint ? 0.5f : 1.0f;
  og.scale = desc->scale * (adjoint ? 1.0f : 1.0f / (float)desc->n_fft);
  og.scale_d = (double)desc->scale * (adjoint ? 1.0 : 1.0 / (double)desc->n_fft);
  if (g.n_fft == 400 && (g.hop == 100 || g.hop == 160 || g.hop == 200) && g.center && g.pad == 0 &&
      !force_generic()) {
    // radix-20x20 register FFT run backwards (istft400.h)
    m400::Inv400Geom ig{g, og.interior};
    const int tiles_per_row = (g.n_frames + m400::kFramesPerWave - 1) / m400::kFramesPerWave;
    const int64_t n_tiles = g.rows * tiles_per_row;
    const int64_t blocks = m400::inv_blocks(dev_props().cu_count, n_tiles);
    const auto* sp = reinterpret_cast<const cplx<float>*>(spec);
#define AAMD_I400(HH)                                                                                             \
    return launch(m400::istft400_kernel<HH>, blocks, 64 * m400::kInvWaves,                                        \
                  ((size_t)m400::kInvWaves * m400::Hop<HH>::lds_dwords + m400::kConstDwords) * sizeof(float),     \
                  (hipStream_t)stream, ig, sp, window, twiddle, inv_envelope, out, og.scale, tiles_per_row, n_tiles)
    if (g.hop == 100) AAMD_I400(5); else if (g.hop == 200) AAMD_I400(10); else AAMD_I400(8);
#undef AAMD_I400
  }
  if ((g.n_fft == 256 || g.n_fft == 512 || g.n_fft == 1024 || g.n_fft == 2048) && !force_generic()) {
    // register-resident wave FFT run as the inverse (stft_pow2.h)
    p2::InvGeom ig{g, og.interior};
    const auto* sp = reinterpret_cast<const p2::C32*>(spec);
    const auto* twc = reinterpret_cast<const p2::C32*>(twiddle);
    // runs of consecutive pairs per wave, or pair-at-a-time atomics (hop > n_fft, or by policy): p2::inv_plan
    const p2::InvPlan pl = p2::inv_plan(g.n_fft, g.hop, dev_props().cu_count, g.rows, g.n_frames,
                                        (policy() & AAMD_POLICY_ISTFT_ATOMIC) != 0);
    const bool use_runs = pl.use_runs;
    const int run_len = pl.run_len;
    const int64_t ppr = pl.pairs_per_row, n_pairs = pl.n_pairs, rpr = pl.runs_per_row, n_runs = pl.n_runs, blocks = pl.blocks;
#define AAMD_IP2(EE)                                                                                              \
    return use_runs                                                                                               \
        ? launch(p2::istft_pow2_run_kernel<EE>, blocks, 64 * p2::kWaves,                                          \
                 (size_t)p2::kWaves * (2 * p2::Cfg<EE>::lds_complex + 2 * p2::Cfg<EE>::N) * sizeof(float),        \
                 (hipStream_t)stream, ig, sp, window, twc, inv_envelope, out, og.scale, ppr, rpr, n_runs, run_len) \
        : launch(p2::istft_pow2_kernel<EE>, blocks, 64 * p2::kWaves,                                              \
                 (size_t)p2::kWaves * p2::Cfg<EE>::lds_complex * sizeof(p2::C32), (hipStream_t)stream, ig, sp,    \
                 window, twc, inv_envelope, out, og.scale, ppr, n_pairs)
    if (g.n_fft == 256) AAMD_IP2(4); else if (g.n_fft == 512) AAMD_IP2(8); else if (g.n_fft == 1024) AAMD_IP2(16); else AAMD_IP2(32);
#undef AAMD_IP2
  }
  int pb = gen_pairs_per_block(g.n_fft);
  const int pairs_per_row = (g.n_frames + 1) / 2;
  if (pb > pairs_per_row) pb = pairs_per_row;
  const int bpr = (pairs_per_row + pb - 1) / pb;
  const int64_t blocks = g.rows * bpr;
  AAMD_CHECK_ARG(blocks < (1ll << 31), "too many frames for one launch");
  size_t lds = ((size_t)2 * g.n_fft + (size_t)4 * pb * gen_seq_len(g.n_fft)) * sizeof(float);
  auto kern = ola_kernel<float>;
  if (lds > dev_props().lds_per_block_optin) {     // long windows: twiddles from memory (stft_generic.h, gen_lds_floats_long)
    lds = gen_lds_floats_long(g.n_fft, pb) * sizeof(float);
    kern = ola_kernel<float, 1>;
    if (lds > dev_props().lds_per_block_optin) return fail(AAMD_EUNSUPPORTED, "audio_amd: n_fft too large for the LDS");
  }
  return launch(kern, blocks, kGenThreads, lds, (hipStream_t)stream, og, spec, window,
                reinterpret_cast<const cplx<float>*>(twiddle), inv_envelope, out, pb, bpr);
}

}  // extern "C"
