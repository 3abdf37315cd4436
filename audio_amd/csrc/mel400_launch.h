// Launch side of the n_fft = 400 kernel (melspec400.h), shared by api_stft.hip (float input) and api_mel400_lowp.hip (int16 /
// half / bfloat16 input): eligibility, the prologue of the mel entry points, and the (EPI, TIn) -> instantiation dispatch.
// Every (EPI, hop, TIn, NR, SIG) instantiation is reached from one entry point, hence emitted by one of the two sources.
#pragma once
#include <cstdint>
#include <cstdlib>
#include <type_traits>

#include "api_common.h"
#include "melspec400.h"

#pragma GCC visibility push(hidden)
namespace aamd {

inline bool fft400_eligible(const StftGeom& g) {
  return g.n_fft == 400 && (g.hop == 160 || g.hop == 200 || g.hop == 100) && g.center && g.pad_mode == AAMD_PAD_REFLECT &&
         g.onesided && g.pad == 0 && g.length > 400 && !force_generic();
}

inline bool mel400_eligible(const StftGeom& g, const MelBandsDev& mb) {
  return fft400_eligible(g) && g.power == 2.0f &&
         m400::mel_ws(mb.max_width) <= m400::kMelMaxTaps + 4 &&
         m400::mel_rounds(mb.n_mels) <= m400::kMelMaxRounds;
}

struct NoCheck { const char* operator()() const { return nullptr; } };

// What the mel entry points open with, in the order they always checked: the descriptor, the buffers, the entry's own
// checks `before`, power and onesided (`one_message`: the wording of the PCM / low-precision entries), the entry's own
// checks `after`, the band table.  An entry's check returns the message of its first failed condition, or null.
template <class Before = NoCheck, class After = NoCheck>
int mel_prologue(const aamd_stft_desc* desc, const aamd_mel_bands* bands, bool buffers, bool one_message, StftGeom& g,
                 MelBandsDev& mb, Before before = {}, After after = {}) {
  int rc = validate_desc(desc, g);
  if (rc != AAMD_OK) return rc;
  AAMD_CHECK_ARG(buffers, "null buffer");
  if (const char* m = before()) return fail(AAMD_EINVAL, std::string("audio_amd: ") + m);
  if (one_message) {
    AAMD_CHECK_ARG(desc->power > 0.0f && desc->onesided, "mel spectrogram needs power > 0 and a onesided spectrum");
  } else {
    AAMD_CHECK_ARG(desc->power > 0.0f, "mel spectrogram needs power > 0");
    AAMD_CHECK_ARG(desc->onesided, "mel spectrogram needs a onesided spectrum");
  }
  if (const char* m = after()) return fail(AAMD_EINVAL, std::string("audio_amd: ") + m);
  return validate_bands(bands, g.n_freq, mb);
}

// the ticket counters of the tail pools (builds with -DAAMD_M400_POOLS=1 only): defined in api_stft.hip, one table for both sources
#if AAMD_M400_POOLS
unsigned* mel400_pool_block(hipStream_t s);
#endif

template <int EPI, int H, typename TIn, int NR, int SIG = 0, int AR = m400::AR_LEGACY>
int launch_fft400_nr(const StftGeom& g, const MelBandsDev& mb, const TIn* wav, const float* window,
                     const float* twiddle, float* out, const m400::Epi400& epi_in, hipStream_t s) {
  if (g.rows == 0) return AAMD_OK;
  const int tiles_per_row = (g.n_frames + m400::kFramesPerWave - 1) / m400::kFramesPerWave;
  const int64_t n_tiles = g.rows * tiles_per_row;
  AAMD_CHECK_ARG(n_tiles < (1ll << 31), "too many frames for one launch");
  const int wpb = m400::kWavesPerBlock;
  const int wdw = m400::Hop<H>::lds_dwords;
  size_t lds = (EPI == m400::EPI400_SPEC) ? m400::lds_bytes(0, 1, wdw) : m400::lds_bytes(mb.n_mels, mb.max_width, wdw);
  m400::Epi400 epi = epi_in;
  if (EPI == m400::EPI400_MFCC && H != 10) {
    // hop 100 / 160: the DCT fragments sit next to the band table in LDS (the kernel's choice per instantiation, melspec400.h
    // kFragLds; mfcc_fused_ok has checked that they fit); hop 200: read from the cache-resident table
    lds = m400::lds_bytes(mb.n_mels, mb.max_width, wdw, true);
    epi.frag_in_lds = 1;
  }
  if (lds > dev_props().lds_per_block_optin)
    return fail(AAMD_EUNSUPPORTED, "audio_amd: mel filterbank too large for the LDS of this device");
  auto kern = m400::melspec400_kernel<0, EPI, H, TIn, NR, SIG, AR>;
#ifdef AAMD_LAB    // tools-only instantiations are compiled into the lab library only (python -m audio_amd._build --lab)
  if (EPI == m400::EPI400_MFCC && epi.lab != 0) kern = m400::melspec400_kernel<(EPI == m400::EPI400_MFCC ? 524288 : 0), EPI, H, TIn, NR, SIG>;
#endif
  // persistent grid: ONE 12-wave workgroup per CU; each owns a contiguous run of tiles (6 frames
  // each) that its waves claim dynamically
  int64_t blocks = dev_props().cu_count;
  const int64_t need = (n_tiles + wpb - 1) / wpb;
  if (blocks > need) blocks = need;
  if (blocks >= 8) blocks -= blocks % 8;  // XCD remap wants a multiple of 8
  if (blocks < 1) blocks = 1;
  const int tiles_per_block = (int)((n_tiles + blocks - 1) / blocks);
  // tail pools: the last P tiles of every workgroup's run are shared with the workgroups of the other XCDs (melspec400.h, pool_tile)
  epi.pool = nullptr;
  epi.pool_p = 0;
#if AAMD_M400_POOLS
  {
#ifdef AAMD_LAB
    static const int lab_p = [] { const char* e = std::getenv("AAMD_MEL400_POOL_P"); return e ? std::atoi(e) : -1; }();   // tools only
#else
    constexpr int lab_p = -1;
#endif
    int P = lab_p >= 0 ? lab_p : m400::pool_share(tiles_per_block);
    if (P > tiles_per_block) P = tiles_per_block;
    const bool fixup_pass = (EPI == m400::EPI400_MFCC) && epi.fixup != 0;
    if (P > 0 && !fixup_pass && epi.lab == 0 && (policy() & AAMD_POLICY_MEL400_NO_POOL) == 0 &&
        (size_t)m400::pool_count((int)blocks) * m400::kPoolStride * sizeof(unsigned) <= 64 * 1024) {
      epi.pool = mel400_pool_block(s);
      epi.pool_p = epi.pool ? P : 0;
    }
  }
#endif
  // 16-B paths: LDS-DMA staging of the waveform, dwordx4 stores of the output rows
  const int in_aligned = (reinterpret_cast<uintptr_t>(wav) % 16 == 0) && (g.row_stride % (16 / (int)sizeof(TIn)) == 0);
  // mel rows leave as 4-byte stores straight from the accumulators: the LDS pipe is this kernel's
  // bottleneck and the LDS-staged dwordx4 path measured 3-4 us slower (AAMD_MEL400_WIDE=1 selects it)
  const bool want_wide = (EPI == m400::EPI400_SPEC) || (policy() & AAMD_POLICY_MEL400_WIDE) != 0;
  const int out_wide = want_wide && (reinterpret_cast<uintptr_t>(out) % 16 == 0) &&
                       (EPI == m400::EPI400_SPEC || mb.n_mels % 4 == 0);
  if (EPI == m400::EPI400_SPEC && !out_wide)
    return fail(AAMD_EINVAL, "audio_amd: spectrogram output buffer must be 16-byte aligned");
  return launch(kern, blocks, 64 * wpb, lds, s, wav, window, twiddle, mb, out, g.rows, g.length, g.row_stride, g.n_frames,
                g.scale, tiles_per_row, n_tiles, tiles_per_block, in_aligned, out_wide, epi);
}

// NR = 4 (n_mels <= 80: band-table control words in registers) or 8 (up to 160 mels); the spectrogram epilogue has
// no mel phase and uses one instantiation
template <int EPI, int H, typename TIn = float>
int launch_fft400_h(const StftGeom& g, const MelBandsDev& mb, const TIn* wav, const float* window,
                    const float* twiddle, float* out, const m400::Epi400& epi, hipStream_t s) {
  if (EPI != m400::EPI400_SPEC && m400::mel_rounds(mb.n_mels) <= 4) {
    // the 80-mel HTK / Slaney banks of the 16 kHz front-ends (headline hop, float input): band reduction compiled for them
    if constexpr (H == 8 && sizeof(TIn) == 4 && std::is_same<TIn, float>::value &&
                  (EPI == m400::EPI400_MEL || EPI == m400::EPI400_MFCC)) {   // (MEL_DB: the straight-line form spills 4 registers)
      if (mb.table_sig == m400::kSigHtk80 && mb.n_mels == 80) {
        // the headline shape: roundings pinned in the source, paired operations as packed fp32 -- or, by policy, the same
        // arithmetic one scalar instruction per operation (bit-identical; tests and A/B runs)
        if constexpr (EPI == m400::EPI400_MEL) {
          if (policy() & AAMD_POLICY_MEL400_SCALAR)
            return launch_fft400_nr<EPI, H, TIn, 4, m400::kSigHtk80, m400::kArScalar>(g, mb, wav, window, twiddle, out, epi, s);
          return launch_fft400_nr<EPI, H, TIn, 4, m400::kSigHtk80, m400::kArPacked>(g, mb, wav, window, twiddle, out, epi, s);
        }
        return launch_fft400_nr<EPI, H, TIn, 4, m400::kSigHtk80>(g, mb, wav, window, twiddle, out, epi, s);
      }
      if (mb.table_sig == m400::kSigSlaney80 && mb.n_mels == 80)
        return launch_fft400_nr<EPI, H, TIn, 4, m400::kSigSlaney80>(g, mb, wav, window, twiddle, out, epi, s);
    }
    return launch_fft400_nr<EPI, H, TIn, 4>(g, mb, wav, window, twiddle, out, epi, s);
  }
  return launch_fft400_nr<EPI, H, TIn, m400::kMelMaxRounds>(g, mb, wav, window, twiddle, out, epi, s);
}

// hop = 20 H.  Inputs other than float are served at hop 160 / 200 only (their entry points have checked).
template <int EPI, typename TIn>
int launch_fft400(const StftGeom& g, const MelBandsDev& mb, const TIn* wav, const float* window,
                  const float* twiddle, float* out, const m400::Epi400& epi, hipStream_t s) {
  if constexpr (std::is_same<TIn, float>::value)
    if (g.hop == 100) return launch_fft400_h<EPI, 5, TIn>(g, mb, wav, window, twiddle, out, epi, s);
  if (g.hop == 200) return launch_fft400_h<EPI, 10, TIn>(g, mb, wav, window, twiddle, out, epi, s);
  return launch_fft400_h<EPI, 8, TIn>(g, mb, wav, window, twiddle, out, epi, s);
}

}  // namespace aamd
#pragma GCC visibility pop
