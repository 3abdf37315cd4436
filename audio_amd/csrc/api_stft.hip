// Forward STFT family of the C ABI: spectrogram, mel spectrogram (float input) with its dB / log-norm epilogues, the fused
// MFCC, the n_fft = 400 tables and the two spectrogram gradients.  Owns every float-input melspec400_kernel instantiation.
#include <cstdlib>
#include <map>
#include <mutex>
#include <utility>

#include "api_common.h"
#include "mel400_launch.h"
#include "mel400_tables.h"
#include "mel_grad.h"
#include "stft_pow2.h"

using namespace aamd;

// (Only in builds with -DAAMD_M400_POOLS=1: the product is built without the pools, DESIGN 4.1 "Round 5".)
// Ticket counters of the n_fft = 400 kernel's tail pools (csrc/melspec400.h, pool_tile): one zeroed 64 KB block per (device,
// stream), allocated on the stream's first eligible launch and never freed (at most 256 of them, 16 MB).  The kernel leaves
// every counter at zero, and launches on one stream run one after the other, so the block needs no memset between launches.
// Under stream capture nothing is handed out (no allocation inside a capture, and a captured launch may be replayed on
// another stream beside eager launches of this one): such launches run their static tile runs, as every launch of the
// product does.  In such a build this is the library's only mutable state besides the thread-local error string.
#if AAMD_M400_POOLS
unsigned* aamd::mel400_pool_block(hipStream_t s) {
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &st) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
  if (st != hipStreamCaptureStatusNone) return nullptr;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
  static std::mutex mu;
  static std::map<std::pair<int, hipStream_t>, unsigned*> blocks;
  std::lock_guard<std::mutex> lock(mu);
  auto it = blocks.find({dev, s});
  if (it != blocks.end()) return it->second;
  if (blocks.size() >= 256) return nullptr;
  constexpr size_t kBytes = 64 * 1024;
  void* p = nullptr;
  if (hipMalloc(&p, kBytes) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
  if (hipMemsetAsync(p, 0, kBytes, s) != hipSuccess) { (void)hipGetLastError(); (void)hipFree(p); return nullptr; }   // ordered in front of the launch
  blocks[{dev, s}] = static_cast<unsigned*>(p);
  return static_cast<unsigned*>(p);
}
#endif

namespace {

// n_fft = 256 / 512 / 1024 / 2048, onesided: the register-resident wave FFT of stft_pow2.h
template <int EPI, int E>
int launch_pow2(const StftGeom& g, const MelBandsDev& mb, const float* wav, const float* window,
                const float* twiddle, float* out, hipStream_t s) {
  const int64_t pairs_per_row = (g.n_frames + 1) / 2;
  const int64_t n_pairs = g.rows * pairs_per_row;
  if (n_pairs == 0) return AAMD_OK;
  size_t lds = (size_t)p2::kWaves * p2::Cfg<E>::lds_complex * sizeof(p2::C32);
  if (EPI == EPI_MEL && p2::mel_in_lds(mb.n_mels, mb.max_width))
    lds += (size_t)p2::mel_lds_floats(mb.n_mels, mb.max_width) * sizeof(float);
  auto kern = p2::stft_pow2_kernel<E, EPI>;
  const int64_t blocks = p2::fwd_blocks(E, dev_props().cu_count, n_pairs);     // persistent waves striding over the pairs
  return launch(kern, blocks, 64 * p2::kWaves, lds, s, g, wav, window, reinterpret_cast<const p2::C32*>(twiddle), mb, out,
                pairs_per_row, n_pairs);
}

template <int EPI>
int launch_generic(const StftGeom& g, const MelBandsDev& mb, const float* wav, const float* window,
                   const float* twiddle, float* out, hipStream_t s) {
  if (g.rows == 0) return AAMD_OK;
  if (g.onesided && !force_generic()) {
    if (g.n_fft == 256) return launch_pow2<EPI, 4>(g, mb, wav, window, twiddle, out, s);
    if (g.n_fft == 512) return launch_pow2<EPI, 8>(g, mb, wav, window, twiddle, out, s);
    if (g.n_fft == 1024) return launch_pow2<EPI, 16>(g, mb, wav, window, twiddle, out, s);
    if (g.n_fft == 2048) return launch_pow2<EPI, 32>(g, mb, wav, window, twiddle, out, s);
  }
  int pb = gen_pairs_per_block(g.n_fft);
  const int pairs_per_row = (g.n_frames + 1) / 2;
  if (pb > pairs_per_row) pb = pairs_per_row;
  const int bpr = (pairs_per_row + pb - 1) / pb;
  const int64_t blocks = g.rows * bpr;
  AAMD_CHECK_ARG(blocks < (1ll << 31), "too many frames for one launch");
  size_t lds = gen_lds_floats(g.n_fft, g.n_freq, pb) * sizeof(float);
  auto kern = stft_generic_kernel<float, EPI>;
  if (lds > dev_props().lds_per_block_optin) {
    // long windows (n_fft ~5 750 .. 8 192): the layout without the LDS twiddle table (stft_generic.h, gen_lds_floats_long)
    lds = gen_lds_floats_long(g.n_fft, pb) * sizeof(float);
    kern = stft_generic_kernel<float, EPI, 1>;
    if (lds > dev_props().lds_per_block_optin) return fail(AAMD_EUNSUPPORTED, "audio_amd: n_fft too large for the LDS");
  }
  return launch(kern, blocks, kGenThreads, lds, s, g, wav, window, reinterpret_cast<const cplx<float>*>(twiddle), mb, out, pb,
                bpr);
}

// ---- MFCC in one kernel (+ a fix-up launch for clamped tiles) --------------------------------------------------------
bool mfcc_fused_ok(const StftGeom& g, const MelBandsDev& mb, int n_mfcc) {
  if (!(mel400_eligible(g, mb) && mb.n_mels == m400::kMfccMels && n_mfcc >= 4 && n_mfcc <= 16 * m400::kMfccMT && n_mfcc % 4 == 0))
    return false;
  // hop 100 / 160 keep the DCT fragments in LDS: a band table too wide to leave them room takes the two-kernel path
  const int wdw = g.hop == 100 ? m400::Hop<5>::lds_dwords : g.hop == 200 ? m400::Hop<10>::lds_dwords : m400::Hop<8>::lds_dwords;
  return g.hop == 200 || m400::lds_bytes(mb.n_mels, mb.max_width, wdw, true) <= dev_props().lds_per_block_optin;
}

}  // namespace

extern "C" {

int64_t aamd_mel400_table_dwords(int32_t n_mels, int32_t max_width) {
  if (n_mels < 1 || max_width < 1) return 0;
  if (m400::mel_ws(max_width) > m400::kMelMaxTaps + 4 || m400::mel_rounds(n_mels) > m400::kMelMaxRounds) return 0;
  return m400::mel_tab_dwords(n_mels, max_width);
}

int aamd_mel400_table_build(const aamd_mel_bands* bands, float* table_out, void* stream) {
  DeviceScope dev_scope_(table_out);
  MelBandsDev mb{};
  int rc = validate_bands(bands, 201, mb);
  if (rc != AAMD_OK) return rc;
  AAMD_CHECK_ARG(table_out != nullptr, "null table buffer");
  if (aamd_mel400_table_dwords(mb.n_mels, mb.max_width) == 0)
    return fail(AAMD_EUNSUPPORTED, "audio_amd: filterbank outside the radix-20x20 kernel (n_mels > 160 or band > 62 bins)");
  mb.table400 = nullptr;
  return launch(m400::mel_tab_build_kernel, 1, 256, 0, (hipStream_t)stream, mb, table_out);
}

int aamd_spectrogram_f32(const float* wav, const float* window, const float* twiddle, float* out,
                         const aamd_stft_desc* desc, void* stream) {
  DeviceScope dev_scope_(wav);
  StftGeom g;
  int rc = validate_desc(desc, g);
  if (rc != AAMD_OK) return rc;
  AAMD_CHECK_ARG(wav && window && twiddle && out, "null buffer");
  MelBandsDev mb{};
  if (fft400_eligible(g) && reinterpret_cast<uintptr_t>(out) % 16 == 0) {   // power <= 0: complex rows
    m400::Epi400 epi{};
    epi.power = g.power;
    return launch_fft400<m400::EPI400_SPEC>(g, mb, wav, window, twiddle, out, epi, (hipStream_t)stream);
  }
  return launch_generic<EPI_SPEC>(g, mb, wav, window, twiddle, out, (hipStream_t)stream);
}

int aamd_melspectrogram_f32(const float* wav, const float* window, const float* twiddle,
                            const aamd_mel_bands* bands, float* out, const aamd_stft_desc* desc,
                            void* stream) {
  DeviceScope dev_scope_(wav);
  StftGeom g;
  MelBandsDev mb;
  int rc = mel_prologue(desc, bands, wav && window && twiddle && out, false, g, mb);
  if (rc != AAMD_OK) return rc;
  if (mel400_eligible(g, mb))
    return launch_fft400<m400::EPI400_MEL>(g, mb, wav, window, twiddle, out, m400::Epi400{}, (hipStream_t)stream);
  return launch_generic<EPI_MEL>(g, mb, wav, window, twiddle, out, (hipStream_t)stream);
}

int32_t aamd_mfcc_frag_floats(void) { return m400::kMfccFragFloats; }

int64_t aamd_mfcc_fused_tiles(const aamd_stft_desc* desc) {
  StftGeom g;
  if (validate_desc(desc, g) != AAMD_OK) return -1;
  return g.rows * ((g.n_frames + m400::kFramesPerWave - 1) / m400::kFramesPerWave);
}

int aamd_mfcc_fused_supported(const aamd_stft_desc* desc, const aamd_mel_bands* bands, int32_t n_mfcc) {
  StftGeom g;
  if (validate_desc(desc, g) != AAMD_OK) return 0;
  MelBandsDev mb;
  if (validate_bands(bands, g.n_freq, mb) != AAMD_OK) return 0;
  return mfcc_fused_ok(g, mb, n_mfcc) ? 1 : 0;
}

int aamd_mfcc_frag_build(const float* dct, int32_t n_mels, int32_t n_mfcc, float* frag, void* stream) {
  DeviceScope dev_scope_(dct);
  AAMD_CHECK_ARG(dct && frag, "null buffer");
  AAMD_CHECK_ARG(n_mels >= 1 && n_mels <= m400::kMfccMels && n_mfcc >= 1 && n_mfcc <= 16 * m400::kMfccMT, "bad sizes");
  return launch(m400::mfcc_frag_build_kernel, 15, 256, 0, (hipStream_t)stream, dct, n_mels, n_mfcc, frag);
}

int aamd_mfcc_fused_f32(const float* wav, const float* window, const float* twiddle, const aamd_mel_bands* bands,
                        float* out, const aamd_stft_desc* desc, const aamd_mfcc_fused* f, void* stream) {
  DeviceScope dev_scope_(wav);
  StftGeom g;
  int rc = validate_desc(desc, g);
  if (rc != AAMD_OK) return rc;
  AAMD_CHECK_ARG(wav && window && twiddle && out && f, "null buffer");
  AAMD_CHECK_ARG(f->dct_frag && f->group_max && f->tile_min, "the fused MFCC needs dct_frag, group_max and tile_min");
  AAMD_CHECK_ARG(f->rows_per_group >= 1 && (f->pass == 0 || f->pass == 1), "bad rows_per_group / pass");
  AAMD_CHECK_ARG(f->fix_count != nullptr, "the fused MFCC needs fix_count in both passes (pass 0 resets it)");
  AAMD_CHECK_ARG(reinterpret_cast<uintptr_t>(out) % 16 == 0 && reinterpret_cast<uintptr_t>(f->dct_frag) % 16 == 0,
                 "out and dct_frag must be 16-byte aligned");
  MelBandsDev mb;
  rc = validate_bands(bands, g.n_freq, mb);
  if (rc != AAMD_OK) return rc;
  if (!mfcc_fused_ok(g, mb, f->n_mfcc))
    return fail(AAMD_EUNSUPPORTED, "audio_amd: the fused MFCC serves n_fft 400 / hop 100, 160, 200 / 80 mels / n_mfcc <= 48 "
                                   "(multiple of 4); use aamd_melspectrogram_db_f32 + aamd_mfcc_dct_f32");
  m400::Epi400 epi{};
  epi.multiplier = f->multiplier; epi.amin = f->amin; epi.db_sub = f->multiplier * f->db_multiplier;
  epi.group_max = f->group_max; epi.rows_per_group = f->rows_per_group;
  epi.dct_frag = f->dct_frag; epi.n_mfcc = f->n_mfcc; epi.top_db = f->top_db; epi.tile_min = f->tile_min;
  epi.fix_count = f->fix_count; epi.fixup = f->pass; epi.fix_list = f->tile_list;
  // (pass 1: every workgroup of the fix-up launch finds the flagged tiles among its own strided share of the tile minima --
  // no list kernel between the passes; fix_count was reset by pass 0 of this call and collects what the workgroups redo)
  if (f->pass == 1) AAMD_CHECK_ARG(f->fix_count && f->tile_list, "pass 1 of the fused MFCC needs fix_count and tile_list");
#ifdef AAMD_LAB
  static const int mfcc_lab = [] { const char* e = std::getenv("AAMD_MFCC_LAB"); return e ? std::atoi(e) : 0; }();   // tools only
  epi.lab = mfcc_lab;
#endif
  hipStream_t s = (hipStream_t)stream;
  switch (g.hop) {
    case 100: return launch_fft400_nr<m400::EPI400_MFCC, 5, float, 4>(g, mb, wav, window, twiddle, out, epi, s);
    case 200: return launch_fft400_nr<m400::EPI400_MFCC, 10, float, 4>(g, mb, wav, window, twiddle, out, epi, s);
    default: return launch_fft400_nr<m400::EPI400_MFCC, 8, float, 4>(g, mb, wav, window, twiddle, out, epi, s);
  }
}

int aamd_melspectrogram_db_f32(const float* wav, const float* window, const float* twiddle,
                               const aamd_mel_bands* bands, float* out, const aamd_stft_desc* desc,
                               float multiplier, float amin, float db_multiplier, float* group_max,
                               int64_t rows_per_group, void* stream) {
  DeviceScope dev_scope_(wav);
  StftGeom g;
  MelBandsDev mb;
  int rc = mel_prologue(desc, bands, wav && window && twiddle && out, false, g, mb, {},
                        [&] { return group_max == nullptr || rows_per_group >= 1 ? nullptr : "rows_per_group must be >= 1"; });
  if (rc != AAMD_OK) return rc;
  if (mel400_eligible(g, mb)) {
    m400::Epi400 epi{};
    epi.multiplier = multiplier; epi.amin = amin; epi.db_sub = multiplier * db_multiplier;
    epi.group_max = group_max; epi.rows_per_group = rows_per_group < 1 ? 1 : rows_per_group;
    return launch_fft400<m400::EPI400_MEL_DB>(g, mb, wav, window, twiddle, out, epi, (hipStream_t)stream);
  }
  rc = launch_generic<EPI_MEL>(g, mb, wav, window, twiddle, out, (hipStream_t)stream);
  if (rc != AAMD_OK) return rc;
  return aamd_amplitude_to_db_f32(out, out, g.rows * g.n_frames * (int64_t)mb.n_mels, multiplier, amin,
                                  db_multiplier, group_max,
                                  (rows_per_group < 1 ? 1 : rows_per_group) * g.n_frames * (int64_t)mb.n_mels,
                                  stream);
}

int aamd_melspectrogram_lognorm_f32(const float* wav, const float* window, const float* twiddle,
                                    const aamd_mel_bands* bands, float* out, const aamd_stft_desc* desc, float gain,
                                    const float* mean, const float* invstddev, int64_t out_frames, void* stream) {
  DeviceScope dev_scope_(wav);
  StftGeom g;
  MelBandsDev mb;
  int rc = mel_prologue(desc, bands, wav && window && twiddle && out && mean && invstddev, false, g, mb, {},
                        [&] { return out_frames >= desc->n_frames ? nullptr : "out_frames must be >= n_frames"; });
  if (rc != AAMD_OK) return rc;
  if (mel400_eligible(g, mb)) {
    m400::Epi400 epi{};
    epi.gain = gain; epi.mean = mean; epi.invstd = invstddev; epi.out_frames = out_frames;
    return launch_fft400<m400::EPI400_MEL_NORM>(g, mb, wav, window, twiddle, out, epi, (hipStream_t)stream);
  }
  if (out_frames != g.n_frames)
    return fail(AAMD_EUNSUPPORTED, "audio_amd: padded feature rows need the n_fft = 400 fast path");
  rc = launch_generic<EPI_MEL>(g, mb, wav, window, twiddle, out, (hipStream_t)stream);
  if (rc != AAMD_OK) return rc;
  const int64_t n = g.rows * g.n_frames * (int64_t)mb.n_mels;
  if (n == 0) return AAMD_OK;
  return launch(lognorm_kernel, grid_for(n, 256, dev_props().cu_count * 16), 256, 0, (hipStream_t)stream, out, n, mb.n_mels,
                gain, mean, invstddev);
}

int aamd_spectrogram_grad_f32(const float* spec, const float* dpower, float* out, int64_t n, float power, void* stream) {
  DeviceScope dev_scope_(spec);
  AAMD_CHECK_ARG(spec && dpower && out, "null buffer");
  AAMD_CHECK_ARG(n >= 0 && power > 0.0f, "bad sizes / power");
  if (n == 0) return AAMD_OK;
  return launch(spec_grad_kernel, grid_for(n, 256, dev_props().cu_count * 16), 256, 0, (hipStream_t)stream,
                reinterpret_cast<const float2*>(spec), dpower, reinterpret_cast<float2*>(out), n, power);
}

int aamd_melspectrogram_grad_f32(float* spec_inout, const float* dmel, const aamd_mel_bands* bands_t, int64_t n_vec,
                                 int32_t n_freq, int32_t n_mels, float power, void* stream) {
  DeviceScope dev_scope_(spec_inout);
  AAMD_CHECK_ARG(spec_inout && dmel, "null buffer");
  AAMD_CHECK_ARG(n_vec >= 0 && n_freq >= 1 && n_mels >= 1 && power > 0.0f, "bad sizes / power");
  MelBandsDev bt;
  int rc = validate_bands(bands_t, n_mels, bt);          // table of fb^T: one band of mels per bin
  if (rc != AAMD_OK) return rc;
  AAMD_CHECK_ARG(bt.n_mels == n_freq, "the transposed band table must have one band per bin");
  const int64_t n = n_vec * n_freq;
  if (n == 0) return AAMD_OK;
  return launch(mel_grad_kernel, grid_for(n, 256, dev_props().cu_count * 16), 256, 0, (hipStream_t)stream,
                reinterpret_cast<float2*>(spec_inout), dmel, bt, n_vec, n_mels, power);
}

}  // extern "C"
