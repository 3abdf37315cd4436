/*
 * audio_amd.h -- C ABI of libaudio_amd.so: MI355X (gfx950) native kernels for the
 * torchaudio DSP hot path (Spectrogram / MelSpectrogram / MFCC / Resample / lfilter /
 * fftconvolve).
 *
 * Boundary contract
 *   - plain C, no torch types: device pointers + sizes + a HIP stream handle (void* =
 *     hipStream_t; NULL = the legacy default stream).  The caller owns every buffer; the
 *     library allocates nothing, keeps no global mutable state and is re-entrant per
 *     (device, stream).  Kernels are enqueued asynchronously on `stream`.
 *   - every entry point returns AAMD_OK (0) or a negative AAMD_E* code;
 *     aamd_last_error() returns a thread-local message for the last failure.
 *   - all tensors are dense row-major fp32 unless stated; "rows" = the flattened leading
 *     dims of the reference's (..., time) tensors.
 *
 * What each entry point replaces in the reference (pytorch/audio, paths relative to
 * src/torchaudio/):
 *   aamd_spectrogram_f32      functional/functional.py:54-145 (F.spectrogram = pad +
 *                             torch.stft + normalisation + abs/pow), called by
 *                             transforms/_transforms.py:101-123 (Spectrogram.forward)
 *   aamd_melspectrogram_f32   transforms/_transforms.py:612-622 (MelSpectrogram.forward =
 *                             Spectrogram.forward + MelScale.forward :403-415)
 *   aamd_melspectrogram_db_f32  ... + F.amplitude_to_DB and its top_db group maximum fused
 *                             (first half of MFCC.forward, _transforms.py:692-706)
 *   aamd_melspectrogram_lognorm_f32  pipelines/rnnt_pipeline.py:16-47, 319-326 (RNN-T feature extractor: the
 *                             MelSpectrogram + transpose + gain/log + global-stats normalisation chain)
 *   aamd_kaldi_features_f32   compliance/kaldi.py:229-315 (spectrogram), :514-645 (fbank; mfcc = fbank + aamd_mfcc_dct_f32)
 *   aamd_phase_vocoder_f32    functional/functional.py:732-803 (F.phase_vocoder; T.TimeStretch, F.pitch_shift)
 *   aamd_griffinlim_update_f32  functional/functional.py:336-343 (phase update of F.griffinlim)
 *   aamd_istft_f32            functional/functional.py:148-225 (F.inverse_spectrogram -> torch.istft) and the
 *                             adjoint of the STFT for autograd of the STFT family
 *   aamd_mel_scale_f32        transforms/_transforms.py:403-415 (MelScale.forward on a
 *                             caller-supplied spectrogram)
 *   aamd_amplitude_to_db_f32  functional/functional.py:356-404 (F.amplitude_to_DB)
 *   aamd_mfcc_dct_f32         transforms/_transforms.py:692-709 (MFCC.forward after the
 *                             mel step: dB/log + top_db clamp + DCT-II matmul)
 *   aamd_resample_f32         functional/functional.py:1405-1432 (_apply_sinc_resample_kernel:
 *                             pad + strided conv1d + phase interleave + crop)
 *   aamd_resample_banded_f32  the same, banded evaluation on the matrix cores
 *   aamd_lfilter_f32          functional/filtering.py:1027-1099 (_lfilter + clamp), i.e.
 *                             DifferentiableFIR.forward :943-951 and the native IIR loop
 *                             libtorchaudio/lfilter.cpp:17-48 / iir_cuda.cu:10-35
 *                             (op torchaudio::_lfilter_core_loop, lfilter.cpp:118-124)
 *   aamd_fftconvolve_f32      functional/functional.py:2222-2258 (F.fftconvolve)
 *   aamd_compute_deltas_f32   F.compute_deltas / T.ComputeDeltas (pad + grouped conv1d in the reference)
 *   aamd_sliding_window_cmn_f32  F.sliding_window_cmn / T.SlidingWindowCmn (a per-frame loop in the reference)
 *                             -- these two (and their _f64 forms) are additions to ABI 7, which stays 7
 *   aamd_spec_augment_iid     F.mask_along_axis_iid / T.SpecAugment (a dozen element-wise launches and one masked_fill
 *   aamd_spec_augment_shared  per mask in the reference); F.mask_along_axis / T.FrequencyMasking / T.TimeMasking
 *                             -- additions to ABI 7 as well
 *   aamd_add_noise_f32        F.add_noise / T.AddNoise (two masks, two norms, logs, a power, a multiply and an add in the
 *   aamd_preemphasis_f32      reference); F.preemphasis / T.Preemphasis -- additions to ABI 7 as well
 *   aamd_beamform_psd         F.psd / T.PSD, the weight solves and F.apply_beamforming / T.MVDR (einsum + linalg.solve
 *   aamd_beamform_weights     compositions over a (..., freq, time, ch, ch) temporary in the reference) -- additions to
 *   aamd_beamform_apply       ABI 7 as well
 *   aamd_rnnt_loss_forward    F.rnnt_loss / T.RNNTLoss (the reference's compiled transducer loss, libtorchaudio/rnnt):
 *   aamd_rnnt_loss_backward   one read of the logits forward, one read and one write backward -- additions to ABI 7 as well
 *   aamd_forced_align         F.forced_align (the reference's libtorchaudio/forced_align: one launch per frame and a host
 *                             backtrack there; two launches here) -- an addition to ABI 7 as well
 *   aamd_overdrive            F.overdrive / F.phaser / F.flanger (the reference's Python loops over samples: a chunked
 *   aamd_phaser               float64 scan in two launches; one launch with the delay ring in LDS, bit for bit; a streaming
 *   aamd_flanger              gather where nothing is fed back) -- additions to ABI 7 as well
 *   aamd_ctc_beam_search      models.decoder.cuda_ctc_decoder (the reference's CUDA-only libctc_prefix_decoder); a row pass and
 *                             a beam pass, float64 scores -- an addition to ABI 7 as well
 *   aamd_vad_measure          F.vad / F.vad_start / T.Vad (the reference's Python loop over measurements: three launches
 *   aamd_vad_trigger          for all measurements of all rows, one or two for the trigger) -- additions to ABI 7 as well
 *   aamd_simulate_rir         prototype.functional.simulate_rir_ism (the reference's Python image lattice around the CPU-only
 *                             torchaudio::_simulate_rir) and a batch of rooms per call; one launch -- an addition to ABI 7
 *   aamd_ray_trace            prototype.functional.ray_tracing (the reference's CPU-only loop over the rays of one room) and a
 *                             batch of rooms per call; fixed-point sums, two launches -- an addition to ABI 7
 *   aamd_oscillator_bank, aamd_filter_waveform, aamd_sinc_impulse_response, aamd_frequency_impulse_response,
 *   aamd_extend_pitch         the synthesis ops of prototype.functional -- additions to ABI 7 as well
 *   aamd_oscillator_bank_grad, aamd_filter_waveform_grad: their first-order gradients (autograd composes a dozen launches over
 *                             (rows, time, taps) gathers in the reference) -- additions to ABI 7 as well
 *   aamd_dense_fbank          F.dense_fbank_scale / prototype.transforms.ChromaScale (a matmul with a dense (n_freqs, n_chroma)
 *                             filterbank in the reference); one launch -- an addition to ABI 7 as well
 *   aamd_edit_distance        F.edit_distance / F.edit_distance_batch (the reference's Python loop over the cells of one pair on
 *                             the host); every pair of a batch in one launch, with the error counts -- an addition to ABI 7
 *   aamd_stoi                 F.stoi: STOI / ESTOI of every row of a batch (pystoi's float64 numpy loop over one utterance on
 *                             the host, through torchmetrics); five launches, no read-back -- an addition to ABI 7
 *   aamd_detect_pitch_f32     F.detect_pitch_frequency (_compute_nccf + _find_max_per_frame + _median_smoothing in the
 *                             reference; an addition to ABI 7 as well)
 *
 * The reference-side binding a maintainer would add is shown in INTEGRATION.md.
 */
#ifndef AUDIO_AMD_H
#define AUDIO_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AAMD_ABI_VERSION 7

enum {
  AAMD_OK = 0,
  AAMD_EINVAL = -1,      /* bad argument (message in aamd_last_error) */
  AAMD_EUNSUPPORTED = -2,/* valid request this build cannot serve (e.g. n_fft too large) */
  AAMD_EHIP = -3         /* a HIP runtime call / kernel launch failed */
};

/* pad modes of torch.stft(center=True) (torch/functional.py:675-680) */
enum { AAMD_PAD_REFLECT = 0, AAMD_PAD_CONSTANT = 1, AAMD_PAD_REPLICATE = 2, AAMD_PAD_CIRCULAR = 3 };

/* Framing + FFT description shared by the STFT-family entry points. */
typedef struct aamd_stft_desc {
  int64_t rows;        /* number of waveforms (flattened leading dims) */
  int64_t length;      /* samples per waveform BEFORE `pad` */
  int64_t row_stride;  /* elements between consecutive waveforms (>= length) */
  int32_t n_fft;
  int32_t hop;
  int32_t pad;         /* F.spectrogram's two-sided constant zero padding (functional.py:112-114) */
  int32_t center;      /* 0/1 */
  int32_t pad_mode;    /* AAMD_PAD_* (used when center) */
  int32_t onesided;    /* 0/1 */
  int32_t n_frames;    /* must equal 1 + (L' - n_fft)/hop, L' = length + 2*pad (+ 2*(n_fft/2) if center) */
  float   scale;       /* multiplies the complex spectrum: 1, n_fft^-1/2 ("frame_length") or 1/||w||_2 ("window") */
  float   power;       /* <= 0: complex output;  1: |X|;  2: |X|^2;  else |X|^power */
} aamd_stft_desc;

/* Banded view of a mel filterbank fb[n_freq][n_mels] (built by the host from the SAME fb
 * tensor the reference multiplies with): column m is non-zero only on rows
 * [lo[m], lo[m]+width[m]); weights[m*max_width + i] = fb[lo[m]+i][m], zero padded. */
typedef struct aamd_mel_bands {
  int32_t n_mels;
  int32_t max_width;
  const int32_t* lo;       /* device, n_mels */
  const int32_t* width;    /* device, n_mels */
  const float*   weights;  /* device, n_mels * max_width */
  /* Optional (may be NULL = identity): lane assignment for the radix-20x20 kernel, device
   * int32[ceil(n_mels/20)*20]; entry 20 r + i = the mel evaluated at lane position i in round r
   * (every mel exactly once, -1 = unused).  Results do not depend on it; it only decides which
   * LDS banks the band reads of a wavefront hit (audio_amd/_host.py: mel_lane_order). */
  const int32_t* lane_order;
  /* Optional (may be NULL): the radix-20x20 kernel's band table laid out once per filterbank by
   * aamd_mel400_table_build (device float[aamd_mel400_table_dwords(n_mels, max_width)]).  With it every workgroup of a
   * launch copies the table into LDS with one round of loads; without it each workgroup derives it from lo / width /
   * weights / lane_order (three dependent rounds, ~3 us per launch).  Results are identical. */
  const float* table400;
  /* Optional (0 = unknown): the shape of the table400 image -- 4-tap chunks of round r in nibble r, given ONLY when the
   * filterbank has exactly 4 rounds of 20 mels and every table row holds a mel.  For the signatures the library was built
   * for (HTK / Slaney 80 mels at 16 kHz: 0x4221 / 0x4211) the radix-20x20 kernel runs an instantiation whose band
   * reduction is straight-line code (- 3 %).  A signature that does not describe table400 is a caller bug: the kernel
   * checks it against the table and traps.  audio_amd/_host.py: mel400_table_signature. */
  int32_t table_sig;
} aamd_mel_bands;

/* Size (in 4-byte words) of the prebuilt band table for a filterbank, 0 if the filterbank is outside what the
 * radix-20x20 kernel serves (more than 160 mels or a band wider than 62 bins). */
int64_t aamd_mel400_table_dwords(int32_t n_mels, int32_t max_width);
/* Lay the table out (one small launch; once per filterbank and lane order, not per call).  bands->table400 is ignored. */
int aamd_mel400_table_build(const aamd_mel_bands* bands, float* table_out, void* stream);

/* Kernel-selection switches for tests and A/B measurements (never needed in production): a process-wide bit mask,
 * initialised once from the environment variables AAMD_FORCE_GENERIC / AAMD_MEL400_WIDE / AAMD_ISTFT_ATOMIC /
 * AAMD_RESAMPLE_FP32 / AAMD_FFTCONV_NO_FDL / AAMD_FFTCONV_FDL / AAMD_RESAMPLE_B32 / AAMD_MEL400_NO_POOL / AAMD_MEL400_SCALAR.
 * aamd_set_kernel_policy returns the previous mask; a negative argument only queries.  Results do not depend on the mask, only which kernel computes them. */
enum {
  AAMD_POLICY_FORCE_GENERIC = 1,  /* skip the shape-specialised kernels (radix-20x20, wave FFT, MFMA paths) */
  AAMD_POLICY_MEL400_WIDE   = 2,  /* n_fft = 400 mel epilogue: 16-byte stores through an LDS stage */
  AAMD_POLICY_ISTFT_ATOMIC  = 4,  /* inverse STFT: one atomic per contribution instead of run-based overlap-add */
  AAMD_POLICY_RESAMPLE_FP32 = 8,  /* banded resampling on v_mfma_f32_16x16x4_f32 instead of the f16 hi/lo-split MFMAs (16 x slower pipe) */
  AAMD_POLICY_FFTCONV_NO_FDL = 16, /* overlap-save: never the frequency-domain delay-line plan */
  AAMD_POLICY_FFTCONV_FDL   = 32, /* overlap-save: the COMPLEX-block delay-line plan (2) whenever the tap count allows it (cost model ignored) */
  AAMD_POLICY_FFTCONV_COMPLEX = 64, /* overlap-save: only the complex-block kernels of rounds 1-3 (plans 1 / 2), never the
                                      real-block kernel of round 4 (plan 3).  NOTE: ANY of the three FFTCONV bits selects the
                                      complex-block kernels for ALL tap counts -- also for <= 8192 taps, where plan 3 is plain
                                      overlap-save on real blocks and no delay line is involved */
  AAMD_POLICY_RESAMPLE_B32 = 128, /* f16 resampler: 4-byte LDS operand reads also where the 8-byte layout of round 5 applies
                                      (odd reduced `orig`, bands of 257 .. 448 taps: kaiser_best 44.1k -> 16k) */
  AAMD_POLICY_MEL400_NO_POOL = 256, /* n_fft = 400 kernels, builds with -DAAMD_M400_POOLS=1 only (round 5 experiment: the last tiles of
                                      every workgroup's run shared between the XCDs; bit-identical results, - 0.8 %, compiled out
                                      of the product): static tile runs per workgroup, as the product always does */
  AAMD_POLICY_MEL400_SCALAR = 512  /* n_fft = 400 mel, headline shape (hop 160, 80-mel HTK bank): the scalar-arithmetic twin of the
                                      packed-fp32 kernel (same roundings, bit-identical output; tests and A/B runs) */
};
int         aamd_set_kernel_policy(int flags);

int         aamd_abi_version(void);
const char* aamd_last_error(void);
/* "gfx950" when the current device is an MI355X-class part; fills name (<=63 chars). */
int         aamd_device_info(char* name, int32_t name_len, int32_t* cu_count, int64_t* hbm_bytes);
/* Measurement aid (bench.py `box_calibration`; no reference counterpart): n_blocks workgroups of 256 threads each run
 * `iters` x 64 dependent fp32 FMAs per lane and record into rec[4 b .. 4 b + 3] = {shader cycles, 100 MHz wall ticks,
 * XCD id, start tick}: the shader clock the box sustains under vector-ALU load and the skew between its XCDs. */
int         aamd_box_probe(int64_t* rec, int32_t n_blocks, int32_t iters, void* stream);

/* ---- STFT family --------------------------------------------------------------------- */

/* window: device float[n_fft] (already centre zero-padded from win_length, as aten::stft does).
 * twiddle: device float[2*n_fft], twiddle[2t],[2t+1] = cos, -sin(2*pi*t/n_fft), fp64-computed.
 * out: frame-major.  power > 0: float[rows][n_frames][n_freq];  power <= 0: interleaved complex
 *      float[rows][n_frames][n_freq][2].  n_freq = onesided ? n_fft/2+1 : n_fft.
 * The reference's logical (..., freq, time) tensor is the transposed VIEW of this buffer, with
 * exactly the strides torch.stft returns. */
int aamd_spectrogram_f32(const float* wav, const float* window, const float* twiddle,
                         float* out, const aamd_stft_desc* desc, void* stream);

/* Fused STFT -> |X|^power -> banded mel.  out: float[rows][n_frames][n_mels].
 * Uses the register/LDS radix-20x20 kernel when n_fft = 400 and hop = 100, 160 or 200, center/reflect,
 * onesided, power 2; every other shape takes the generic LDS Stockham kernel -- same results.
 * (aamd_spectrogram_f32 takes the same fast kernel for that shape when power > 0.) */
int aamd_melspectrogram_f32(const float* wav, const float* window, const float* twiddle,
                            const aamd_mel_bands* bands, float* out,
                            const aamd_stft_desc* desc, void* stream);

/* The same with F.amplitude_to_DB (functional.py:390-391) fused into the epilogue:
 *   out = multiplier*log10(max(mel, amin)) - multiplier*db_multiplier,
 * and, if group_max != NULL, the running maximum of `out` over each cut-off group of
 * rows_per_group consecutive waveforms max-reduced into group_max[row / rows_per_group]
 * (float; caller pre-fills with -inf) -- the reduction top_db needs (functional.py:393-402).
 * This is the first half of MFCC.forward (transforms/_transforms.py:692-706); aamd_mfcc_dct_f32
 * with log_mode 2 is the second half. */
int aamd_melspectrogram_db_f32(const float* wav, const float* window, const float* twiddle,
                               const aamd_mel_bands* bands, float* out, const aamd_stft_desc* desc,
                               float multiplier, float amin, float db_multiplier, float* group_max,
                               int64_t rows_per_group, void* stream);

/* MFCC.forward (transforms/_transforms.py:692-709: MelSpectrogram -> amplitude_to_DB(top_db) -> DCT matmul) in ONE kernel
 * for the headline front-end (n_fft 400, hop 100 / 160 / 200, 80 mels, n_mfcc <= 48 and a multiple of 4), plus a fix-up launch:
 *   pass 0  writes out[rows][n_frames][n_mfcc] WITHOUT the top_db cut-off, max-reduces the dB values of each cut-off group
 *           into group_max (caller pre-fills with -inf) and records the smallest dB value of every 6-frame tile in tile_min;
 *   (multi-GPU: all-reduce group_max with MAX here)
 *   pass 1  redoes, clamped at group_max[g] - top_db, exactly the tiles whose minimum lies under that cut-off and counts
 *           them in fix_count (required in both passes: pass 0 resets it); every workgroup of this launch checks a strided
 *           share of the tile minima itself (its flagged tiles go to a private run of tile_list) and leaves when none is
 *           flagged -- no separate compaction kernel between the passes.  Batches in which nothing reaches the cut-off pay ~2 us for it; batches in which
 *           most tiles do should take aamd_melspectrogram_db_f32 + aamd_mfcc_dct_f32 (the caller's choice).
 * Results equal the two-kernel path's up to the rounding of the fp32 contraction order. */
typedef struct aamd_mfcc_fused {
  const float* dct_frag;   /* device float[aamd_mfcc_frag_floats()], from aamd_mfcc_frag_build */
  int32_t n_mfcc;
  int32_t pass;            /* 0 or 1 */
  float multiplier, amin, db_multiplier, top_db;   /* F.amplitude_to_DB's (functional.py:356-404) */
  float* group_max;        /* device float[ceil(rows / rows_per_group)] */
  int64_t rows_per_group;
  float* tile_min;         /* device float[aamd_mfcc_fused_tiles(desc)] */
  int32_t* fix_count;      /* device int32: pass 0 resets it, pass 1 leaves the number of tiles it redoes here */
  int32_t* tile_list;      /* device int32[aamd_mfcc_fused_tiles(desc)]: scratch of pass 1 -- each workgroup's flagged tiles (its
                              candidates are every n-th tile, so clamped tiles spread evenly however they cluster by clip) */
} aamd_mfcc_fused;
int32_t aamd_mfcc_frag_floats(void);
int64_t aamd_mfcc_fused_tiles(const aamd_stft_desc* desc);
int aamd_mfcc_fused_supported(const aamd_stft_desc* desc, const aamd_mel_bands* bands, int32_t n_mfcc);   /* 1 / 0 */
/* dct: device float[n_mels][n_mfcc] (F.create_dct, functional.py:636-667) -> the MFMA operand layout of the fused kernel */
int aamd_mfcc_frag_build(const float* dct, int32_t n_mels, int32_t n_mfcc, float* frag, void* stream);
int aamd_mfcc_fused_f32(const float* wav, const float* window, const float* twiddle, const aamd_mel_bands* bands,
                        float* out, const aamd_stft_desc* desc, const aamd_mfcc_fused* f, void* stream);

/* MelSpectrogram with the RNN-T front-end's feature post-processing fused into the epilogue
 * (pipelines/rnnt_pipeline.py:16-47, 319-326: x * gain -> _piecewise_linear_log -> (x - mean) * invstddev):
 *   out[row][t][m] = (plog(mel[row][t][m] * gain) - mean[m]) * invstddev[m]
 *   plog = the reference's two in-place masked assignments as evaluated: y <= e: y / e; e < y <= e^e: ln(y) / e;
 *   y > e^e: ln(y)   (the second mask sees the values the first one wrote)
 * out is frame-major float[rows][out_frames][n_mels] with out_frames >= n_frames; frames n_frames .. out_frames-1
 * (the pipeline's right padding) are NOT written: the caller zero-fills them.  mean / invstddev: float[n_mels].
 * Shapes outside the n_fft = 400 fast path need out_frames == n_frames. */
int aamd_melspectrogram_lognorm_f32(const float* wav, const float* window, const float* twiddle,
                                    const aamd_mel_bands* bands, float* out, const aamd_stft_desc* desc, float gain,
                                    const float* mean, const float* invstddev, int64_t out_frames, void* stream);

/* The same two kernels reading 16-bit PCM directly (what the decoder upstream of the transform produces,
 * torchaudio/_torchcodec.py -> float = int16 / 32768): the int16 -> float pass and half of the input bytes disappear.
 * wav: int16[rows][row_stride]; fold the 1 / 32768 into desc->scale.  mean == invstddev == NULL: plain mel spectrogram
 * (out_frames ignored); otherwise the RNN-T feature epilogue of aamd_melspectrogram_lognorm_f32.
 * Served for n_fft = 400, hop 160 / 200 (centre, reflect, power 2); other shapes: AAMD_EUNSUPPORTED (convert first). */
int aamd_melspectrogram_pcm16_f32(const int16_t* wav, const float* window, const float* twiddle,
                                  const aamd_mel_bands* bands, float* out, const aamd_stft_desc* desc, float gain,
                                  const float* mean, const float* invstddev, int64_t out_frames, void* stream);

/* The same, reading INTERLEAVED 16-bit PCM: pcm = int16[clips][row_stride][channels] (time-major, channels adjacent: the
 * decoder's native order, which the reference transposes to (channel, time) before any transform,
 * torchaudio/_torchcodec.py:150-152).  desc->rows = clips * channels (row r = clip r / channels, channel r % channels:
 * the output is laid out (clip, channel, frames, n_mels)); desc->length and desc->row_stride count SAMPLE TIMES per
 * channel.  channels = 1 is aamd_melspectrogram_pcm16_f32; channels = 2 is served by the same kernel (both rows of a clip
 * stage the same 32-bit (L, R) words and the gather takes the row's half-word: de-interleave, conversion and 1 / 32768 in
 * the load); any other count: AAMD_EUNSUPPORTED (transpose first). */
int aamd_melspectrogram_pcm16_interleaved_f32(const int16_t* pcm, int32_t channels, const float* window, const float* twiddle,
                                              const aamd_mel_bands* bands, float* out, const aamd_stft_desc* desc,
                                              float gain, const float* mean, const float* invstddev, int64_t out_frames,
                                              void* stream);

/* Half / bfloat16 WAVEFORMS (ABI 6; the reference accepts any floating dtype -- functional/functional.py:1413-1414, the
 * `forward` of every transform -- and returns it): wav is read as binary16 / bfloat16 and converted in the load of the
 * radix-20x20 kernel (n_fft = 400, hop 160 / 200, power 2: AAMD_EUNSUPPORTED otherwise -- the host then casts and calls the
 * float entry).  Arithmetic and `out` are float32; the caller casts the result to the input dtype.  row_stride and length in
 * SAMPLES. */
enum { AAMD_DTYPE_F16 = 1, AAMD_DTYPE_BF16 = 2 };
int aamd_melspectrogram_lowp_f32(const void* wav, int32_t wav_dtype, const float* window, const float* twiddle,
                                 const aamd_mel_bands* bands, float* out, const aamd_stft_desc* desc, void* stream);

/* Backward of the |X|^p stage of F.spectrogram (functional.py:141-145), element-wise over n bins:
 *   out = dpower * p * |X|^(p-2) * X   (interleaved complex; 0 where X = 0 and p < 2)
 * -- the spectrum-domain cotangent aamd_istft_f32(adjoint = 1) turns into d loss / d waveform.  The filterbank's backward
 * (dpower = dmel * fb^T) is aamd_mel_scale_f32 with the band table of fb^T. */
int aamd_spectrogram_grad_f32(const float* spec, const float* dpower, float* out, int64_t n, float power, void* stream);

/* Both of the above in one pass for MelSpectrogram's backward: spec_inout holds the complex STFT X
 * (float[n_vec][n_freq][2]) and receives G = (sum_m fb[k][m] dmel[v][m]) * p |X|^(p-2) X.  bands_t: band table of
 * fb^T (one band of mels per bin).  dmel: float[n_vec][n_mels]. */
int aamd_melspectrogram_grad_f32(float* spec_inout, const float* dmel, const aamd_mel_bands* bands_t, int64_t n_vec,
                                 int32_t n_freq, int32_t n_mels, float power, void* stream);

/* Kaldi-compatible front-end (compliance/kaldi.py: spectrogram :229-315, fbank :514-645; the framing and per-frame
 * conditioning of _get_window :154-217): frames of `win` samples every `shift` samples of ONE waveform, DC removal, raw
 * or windowed log-energy, pre-emphasis, window, zero padding to n_fft, power spectrum, then
 *   bands == NULL: rows float[n_frames][n_fft/2 + 1] = log(max(|X|^2, eps)), column 0 = log energy   (kaldi.spectrogram)
 *   bands != NULL: rows float[n_frames][n_cols]: column first_col + m = mel-bank energy m (log(max(., eps)) if use_log),
 *                  column energy_col (if >= 0) = log energy                                        (kaldi.fbank)
 * window: float[n_fft], the window function in the first `win` entries, zero after.  n_fft = 256 / 512 / 1024 / 2048 run on
 * the register FFT; any other EVEN n_fft (round_to_power_of_two = False: 400 at 16 kHz, 200 at 8 kHz, 1102 at 44.1 kHz ...)
 * on the mixed-radix LDS kernel of csrc/kaldi_generic.h.  Dither: the caller draws the Gaussian noise (as the reference
 * does with torch.randn) and passes it in desc->noise. */
typedef struct aamd_kaldi_desc {
  int64_t n_samples, n_frames;
  int32_t n_fft, shift, win;
  int32_t snip_edges;
  float preemphasis;
  int32_t remove_dc_offset, raw_energy;
  float energy_floor;                  /* 0: no floor */
  int32_t use_power, use_log;
  int32_t energy_col, first_col, n_cols;
  float dither;                        /* 0: off; else frames += dither * noise (kaldi.py:180-183) */
  const float* noise;                  /* device float[n_utt][n_frames][win] unit Gaussian draws (the caller's RNG), NULL if dither == 0 */
  int64_t n_utt;                       /* 0 or 1: one waveform (the reference's API); > 1: a batch of equal-length utterances */
  int64_t utt_stride;                  /* samples between utterances (>= n_samples); out is float[n_utt][n_frames][row] */
} aamd_kaldi_desc;
int aamd_kaldi_features_f32(const float* wav, const float* window, const float* twiddle, const aamd_mel_bands* bands,
                            float* out, const aamd_kaldi_desc* desc, void* stream);

/* Frames -> waveform (overlap-add).  spec: interleaved complex float[rows][n_frames][n_fft/2+1][2] (frame-major,
 * onesided); window / twiddle as for aamd_spectrogram_f32; out: float[rows][length], MUST be zero-filled by the
 * caller (contributions are accumulated with atomic adds).  desc->length = output samples per row; frame t
 * covers padded-axis samples t*hop .. t*hop+n_fft-1, which map to output samples exactly as the forward's
 * padding does (centre offset n_fft/2, pad_mode, desc->pad); samples that map nowhere are dropped.
 *   adjoint == 0: torch.istft's numerator (functional/functional.py:205-216): out += scale/n_fft * w[n] * irfft-sum;
 *                 pass pad_mode = AAMD_PAD_CONSTANT (centre trimming) and inv_envelope[length] = 1 / sum_t w^2
 *                 to get the least-squares inverse, or NULL for the bare overlap-add.
 *   adjoint != 0: the adjoint of the onesided STFT (autograd of Spectrogram & co.):
 *                 out[i] += scale * w[n] * Re sum_{k=0}^{n_fft/2} spec[t][k] e^{+2 pi i n k / n_fft}
 *                 with the forward's pad_mode, so reflected / replicated edges fold back onto the samples they copied. */
int aamd_istft_f32(const float* spec, const float* window, const float* twiddle, const float* inv_envelope,
                   float* out, const aamd_stft_desc* desc, int32_t adjoint, void* stream);

/* Phase vocoder (functional/functional.py:732-803; T.TimeStretch, F.pitch_shift): stretch a complex
 * spectrogram in time by `rate`.  Strides are in COMPLEX elements, so the reference's (rows, freq, frames)
 * tensors and this library's frame-major (rows, frames, freq) buffers are both addressable.
 * n_frames_out = ceil(n_frames_in / rate); phase_advance: float[n_freq]. */
typedef struct aamd_vocoder_desc {
  int64_t rows;
  int32_t n_freq, n_frames_in, n_frames_out;
  int64_t in_stride_row, in_stride_freq, in_stride_frame;
  int64_t out_stride_row, out_stride_freq, out_stride_frame;
  double rate;
} aamd_vocoder_desc;
int aamd_phase_vocoder_f32(const float* spec, const float* phase_advance, float* out, const aamd_vocoder_desc* desc,
                           void* stream);

/* One phase update of Griffin-Lim (functional/functional.py:336-343), element-wise over n complex values:
 *   a = rebuilt - momentum * tprev;  a /= |a| + 1e-16;  tprev = rebuilt;  next = magnitude * a
 * (`momentum` is already momentum / (1 + momentum), :302). */
int aamd_griffinlim_update_f32(const float* rebuilt, float* tprev, const float* magnitude, float* next, int64_t n,
                               float momentum, void* stream);

/* MelScale.forward on an existing spectrogram given frame-major: spec float[rows][n_frames][n_freq]
 * -> out float[rows][n_frames][n_mels]. */
int aamd_mel_scale_f32(const float* spec, const aamd_mel_bands* bands, float* out,
                       int64_t rows, int32_t n_frames, int32_t n_freq, void* stream);

/* ---- dB / MFCC ------------------------------------------------------------------------- */

/* x_db = multiplier*log10(max(x, amin)) - multiplier*db_multiplier (functional.py:390-391).
 * If group_max != NULL, also atomically max-reduces x_db of group g = i / group_size into
 * group_max[g] (float bit pattern; caller pre-fills with -inf).  out may alias x. */
int aamd_amplitude_to_db_f32(const float* x, float* out, int64_t n, float multiplier, float amin,
                             float db_multiplier, float* group_max, int64_t group_size, void* stream);

/* dB conversion and top_db clamp in one sweep, given the group maxima of a previous aamd_amplitude_to_db_f32(x, NULL, ...)
 * call (out == NULL there = maximum only): out[i] = max(dB(x[i]), group_max[i / group_size] - top_db). */
int aamd_amplitude_to_db_clamped_f32(const float* x, float* out, int64_t n, float multiplier, float amin,
                                     float db_multiplier, const float* group_max, int64_t group_size, float top_db,
                                     void* stream);

/* out[i] = max(x[i], group_max[i / group_size] - top_db)  (functional.py:393-402). */
int aamd_db_clamp_f32(const float* x, float* out, int64_t n, const float* group_max,
                      int64_t group_size, float top_db, void* stream);

/* MFCC tail on frame-major mel features mel float[n_vec][n_mels]:
 *   log_mode 0: y = 10*log10(max(mel,1e-10)) clamped at group_max[g]-top_db (top_db<0: no clamp)
 *   log_mode 1: y = log(mel + 1e-6)
 *   log_mode 2: mel already holds y (dB), only clamp
 * then out[v][k] = sum_m y[v][m] * dct[m][k]   (dct: device float[n_mels][n_mfcc]).
 * g = v / vec_per_group. */
int aamd_mfcc_dct_f32(const float* mel, const float* dct, float* out, int64_t n_vec,
                      int32_t n_mels, int32_t n_mfcc, int32_t log_mode, const float* group_max,
                      int64_t vec_per_group, float top_db, void* stream);

/* ---- Resample --------------------------------------------------------------------------- */

/* y[row][q*new + p] = sum_k kernel[p][k] * xpad[row][q*orig + k],  xpad = [0]*width ++ x ++ [0]*(width+orig),
 * for the first out_len = ceil(new*length/orig) outputs.  kernel: device float[new][taps],
 * taps = 2*width + orig.  out: float[rows][out_len]. */
int aamd_resample_f32(const float* wav, const float* kernel, float* out, int64_t rows,
                      int64_t length, int64_t row_stride, int32_t orig, int32_t new_, int32_t width,
                      int64_t out_len, void* stream);

/* Band description of the tap table per tile of 16 consecutive phases (HOST memory): every
 * non-negligible tap of phases [16t, 16t+16) lies in [tap_lo[t], tap_lo[t] + tap_span).
 * Taps outside the band are treated as zero (the caller decides what is negligible; the Python
 * host drops |h| <= 2^-40 max|h|, < 1e-9 of a full-scale output). */
typedef struct aamd_resample_bands {
  int32_t n_tiles;         /* ceil(new / 16) */
  int32_t tap_span;
  const int32_t* tap_lo;   /* host, n_tiles */
} aamd_resample_bands;

/* Same result as aamd_resample_f32, evaluated on the matrix cores over the banded tap table
 * (v_mfma_f32_16x16x4_f32, exact fp32 FMA chains).  bands == NULL, a band wider than 448 taps
 * or an `orig` whose double-buffered chunk exceeds the LDS fall back to aamd_resample_f32. */
int aamd_resample_banded_f32(const float* wav, const float* kernel, float* out, int64_t rows,
                             int64_t length, int64_t row_stride, int32_t orig, int32_t new_,
                             int32_t width, int64_t out_len, const aamd_resample_bands* bands,
                             void* stream);

/* Prepared tap fragments (ABI 7, round 5).  The binary16-split matrix-core kernels multiply with the filter's taps as packed
 * (hi, lo) binary16 fragments; formed by every workgroup in its prologue they cost 13 % of a BASELINE config-3 launch.  A filter
 * that is applied many times (T.Resample holds its `kernel` buffer, transforms/_transforms.py:966-980) prepares them once:
 *   aamd_resample_frag_bytes      size of the table for this band table (0: no matrix-core kernel serves it)
 *   aamd_resample_frag_build_f32  fills `frag` (device, 16-byte aligned, that many bytes) from the tap table, on `stream`
 *   aamd_resample_prepared_f32    = aamd_resample_banded_f32 reading `frag` (NULL: forms the fragments itself; bit-identical results)
 * `frag` must come from a build with the same kernel values, orig, new, width and band table, stream-ordered before the call
 * (or synchronised); it is read-only while calls run and independent of the kernel policy (the fp32-MFMA and scalar kernels
 * ignore it). */
int64_t aamd_resample_frag_bytes(int32_t orig, int32_t new_, const aamd_resample_bands* bands);
int     aamd_resample_frag_build_f32(const float* kernel, int32_t orig, int32_t new_, int32_t width,
                                     const aamd_resample_bands* bands, void* frag, void* stream);
int     aamd_resample_prepared_f32(const float* wav, const float* kernel, float* out, int64_t rows,
                                   int64_t length, int64_t row_stride, int32_t orig, int32_t new_,
                                   int32_t width, int64_t out_len, const aamd_resample_bands* bands,
                                   const void* frag, void* stream);

/* Sparse evaluation for ratios whose REDUCED rates are huge (F.pitch_shift / T.PitchShift: 20158 -> 16000 Hz is
 * 10079 : 8000, a tap table of 8000 x 10095 with ~36 non-negligible taps per phase; functional/functional.py:1790-1840):
 * taps_compact: device float[new][span] = kernel[p][tap_lo[p] .. tap_lo[p] + span), tap_lo: device int32[new], compacted
 * once by the host.  Same result as aamd_resample_f32 up to the taps the caller dropped. */
int aamd_resample_sparse_f32(const float* wav, const float* taps_compact, const int32_t* tap_lo, float* out, int64_t rows,
                             int64_t length, int64_t row_stride, int32_t orig, int32_t new_, int32_t width, int32_t span,
                             int64_t out_len, void* stream);

/* ---- lfilter ---------------------------------------------------------------------------- */

/* x, y: float[batch][channels][length]; a, b: device float[n_coeff_rows][n_order] with
 * n_coeff_rows = 1 (shared) or channels (per channel), lower delays first, NOT yet normalised
 * by a0 (the kernel divides, like filtering.py:1028-1029).  clamp: 0/1 -> clamp(y,-1,1) after
 * the recursion.  n_stages > 1 applies a cascade: a, b are float[n_stages][n_coeff_rows][n_order]
 * and each stage's (clamped) output feeds the next -- equal to n_stages sequential F.lfilter calls.
 * clamp = 2 clamps after the LAST stage only: one higher-order filter given as second-order sections
 * (the host layer factors orders 3 .. 8 that way when the sections reproduce the filter, see
 * audio_amd/_host.py lfilter_sos; the biquad-class kernels run ~6 x faster than the general-order scan). */
int aamd_lfilter_f32(const float* x, const float* a, const float* b, float* y, int64_t batch,
                     int32_t channels, int64_t length, int32_t n_order, int32_t n_coeff_rows,
                     int32_t n_stages, int32_t clamp, void* stream);
/* aamd_lfilter_plan reports what aamd_lfilter_f32 launches for these buffers and sizes on the current device under the current
 * kernel policy (no launch; x and y are only looked at for their 16-byte alignment):
 * out = {kernel, W, workgroups, dynamic LDS bytes}.  kernel: 0 the general-order kernel (csrc/lfilter.h; W and LDS 0),
 * 1 lfw::lfilter_wave_kernel<0, 8, true>, 2 <0, 8, false>, 3 <0, 16, true>, 4 <0, 16, false>, 5 lfw::lfilter_wave_pipe_kernel,
 * 6 lfw::lfilter_wave_mover_kernel (csrc/lfilter_wave.h, lfw::pick).  W: waves per sequence; workgroup g filters the sequences
 * g, g + workgroups, ... */
int aamd_lfilter_plan(const void* x, const void* y, int64_t batch, int32_t channels, int64_t length, int32_t n_order,
                      int32_t n_stages, int32_t out[4]);

/* ---- fftconvolve ------------------------------------------------------------------------ */

/* Linear convolution along the last dim: out[row][n] = sum_m x[rx][m] * y[ry][n-m], full length
 * nx+ny-1, then the slice [start, start+out_len) is stored (mode crop, functional.py:2207-2219).
 * x: float[n_x_rows][nx], y: float[n_y_rows][ny]; x_row_of / y_row_of are device int64[rows] maps
 * from output row to input row (broadcasting); NULL means identity.
 * The shorter operand is treated as the taps.  <= 192 taps: tiled time-domain evaluation.  More:
 * overlap-save on a 16384-point complex FFT held in LDS (two real blocks per complex FFT, taps
 * in partitions of <= 8192; tap spectra, the twiddle table and -- for 8193 .. 32768 taps -- the
 * frequency-domain delay lines of the workgroups live in `workspace`, which must hold
 * aamd_fftconvolve_workspace() bytes, 8-byte aligned; it may be NULL when that is 0).
 * aamd_fftconvolve_plan reports what a call of that shape runs on the current device: 0 time domain, 1 overlap-save
 * with the input spectrum recomputed per tap partition, 2 overlap-save with a frequency-domain delay line (uniform
 * 8192-tap partitions, one forward + one inverse FFT per block; chosen by a cost model over rows, blocks and CUs),
 * 3 (193 .. 32768 taps, the default; 24576 until ABI 5) REAL blocks as 8192-point complex FFTs, one row per workgroup of
 * 1024 threads (csrc/fftconv_fdr.h): plain overlap-save up to 8192 taps (hop = 16385 - taps), beyond that the delay line over
 * 8192-tap partitions with up to three delayed spectra in registers. */
int64_t aamd_fftconvolve_workspace(int64_t rows, int64_t n_x_rows, int64_t n_y_rows, int64_t nx, int64_t ny);
int aamd_fftconvolve_plan(int64_t rows, int64_t nx, int64_t ny, int64_t out_len);
int aamd_fftconvolve_f32(const float* x, const float* y, float* out, int64_t rows, int64_t n_x_rows,
                         int64_t n_y_rows, int64_t nx, int64_t ny, const int64_t* x_row_of,
                         const int64_t* y_row_of, int64_t start, int64_t out_len, void* workspace,
                         void* stream);
/* The same call in two stages (ABI 6), for the case the reference's users have in practice -- many batches convolved with
 * ONE room impulse response (`T.FFTConvolve` inside an augmentation loop, functional.py:2222-2258 recomputes rfft(y) every
 * call): AAMD_FFTCONV_PREPARE writes the twiddle table and the tap spectra of the call's plan into `workspace` (two small
 * launches, ~16 us on the BASELINE config-5 shard), AAMD_FFTCONV_RUN walks the rows using a workspace prepared before.
 * Both bits = aamd_fftconvolve_f32.  A RUN-only call must see the workspace of a PREPARE call with the same taps, tap rows,
 * kernel policy and plan (aamd_fftconvolve_plan; plan 3 and plan 1 keep the workspace read-only while they run, plan 2
 * holds its delay-line ring there: one call at a time), stream-ordered after it.  PREPARE alone accepts x = out = NULL;
 * with <= 192 taps (time-domain kernel) it does nothing. */
enum { AAMD_FFTCONV_PREPARE = 1, AAMD_FFTCONV_RUN = 2 };
int aamd_fftconvolve_staged_f32(const float* x, const float* y, float* out, int64_t rows, int64_t n_x_rows,
                                int64_t n_y_rows, int64_t nx, int64_t ny, const int64_t* x_row_of,
                                const int64_t* y_row_of, int64_t start, int64_t out_len, void* workspace,
                                int32_t stages, void* stream);

/* ---- float64 ------------------------------------------------------------------------------ */

/* The reference guarantees first- AND second-order gradients of this path and checks them in float64
 * (test/torchaudio_unittest/functional/autograd_impl.py:21-35, transforms/autograd_test_impl.py:30-45); its native IIR
 * loop dispatches on double too (libtorchaudio/lfilter.cpp:62-68).  These entries have the semantics of their _f32
 * namesakes on double buffers.  They are the generic kernels (no shape-specialised fast paths): precision, not
 * throughput.  aamd_spectrogram_f64: twiddle is double[2 * n_fft]; desc->power <= 0 (complex) or > 0.
 * aamd_lfilter_f64: n_stages must be 1.  aamd_fftconvolve_f64: direct evaluation, no workspace. */
int aamd_spectrogram_f64(const double* wav, const double* window, const double* twiddle, double* out,
                         const aamd_stft_desc* desc, void* stream);
int aamd_istft_f64(const double* spec, const double* window, const double* twiddle, const double* inv_envelope,
                   double* out, const aamd_stft_desc* desc, int32_t adjoint, void* stream);
int aamd_lfilter_f64(const double* x, const double* a, const double* b, double* y, int64_t batch, int32_t channels,
                     int64_t length, int32_t n_order, int32_t n_coeff_rows, int32_t n_stages, int32_t clamp, void* stream);
int aamd_resample_f64(const double* wav, const double* kernel, double* out, int64_t rows, int64_t length,
                      int64_t row_stride, int32_t orig, int32_t new_, int32_t width, int64_t out_len, void* stream);
int aamd_fftconvolve_f64(const double* x, const double* y, double* out, int64_t rows, int64_t n_x_rows, int64_t n_y_rows,
                         int64_t nx, int64_t ny, const int64_t* x_row_of, const int64_t* y_row_of, int64_t start,
                         int64_t out_len, void* stream);

/* ---- feature post-processing (additions to ABI 7; csrc/feat_post.h) --------------------------------------------- */

/* Delta coefficients, F.compute_deltas (functional/functional.py, compute_deltas): every (channel, feature) row of
 * n_frames frames is padded by n = (win_length - 1) / 2 frames with pad_mode (AAMD_PAD_*) and correlated with
 * [-n .. n]; the result is divided by n (n + 1) (2n + 1) / 3.  x is read in place through its element strides
 * (stride_channel, stride_feat, stride_frame): time-contiguous rows and frame-major storage (stride_feat == 1, what
 * MelSpectrogram returns) are both read without a copy.  out is dense (channels, n_feat, n_frames).
 * adjoint = 1 applies the transpose of the same linear map (its gradient; the adjoint of the adjoint is the forward).
 * win_length >= 3; AAMD_PAD_REFLECT needs n < n_frames and AAMD_PAD_CIRCULAR n <= n_frames (AAMD_EINVAL otherwise);
 * a window whose LDS tile does not fit (n in the thousands) is AAMD_EUNSUPPORTED. */
int aamd_compute_deltas_f32(const float* x, float* out, int64_t channels, int64_t n_feat, int64_t n_frames,
                            int64_t stride_channel, int64_t stride_feat, int64_t stride_frame, int32_t win_length,
                            int32_t pad_mode, int32_t adjoint, void* stream);
int aamd_compute_deltas_f64(const double* x, double* out, int64_t channels, int64_t n_feat, int64_t n_frames,
                            int64_t stride_channel, int64_t stride_feat, int64_t stride_frame, int32_t win_length,
                            int32_t pad_mode, int32_t adjoint, void* stream);
/* Sliding-window cepstral mean (and variance) normalisation, F.sliding_window_cmn (functional/functional.py,
 * sliding_window_cmn; Kaldi's apply-cmvn-sliding): x is (channels, n_frames, n_feat) through its element strides (given,
 * like the deltas', in (channel, feature, frame) order); out is dense (channels, n_frames, n_feat).  Every window sum is
 * accumulated in float64 (chunk sums in `workspace`, which must hold aamd_sliding_window_cmn_workspace() bytes, 8-byte
 * aligned).  adjoint = 1 (norm_vars = 0 only) applies the transpose of the linear map x -> out.  cmn_window >= 0. */
int64_t aamd_sliding_window_cmn_workspace(int64_t channels, int64_t n_frames, int64_t n_feat, int32_t norm_vars);
int aamd_sliding_window_cmn_f32(const float* x, float* out, void* workspace, int64_t channels, int64_t n_frames,
                                int64_t n_feat, int64_t stride_channel, int64_t stride_feat, int64_t stride_frame,
                                int64_t cmn_window, int64_t min_cmn_window, int32_t center, int32_t norm_vars,
                                int32_t adjoint, void* stream);
int aamd_sliding_window_cmn_f64(const double* x, double* out, void* workspace, int64_t channels, int64_t n_frames,
                                int64_t n_feat, int64_t stride_channel, int64_t stride_feat, int64_t stride_frame,
                                int64_t cmn_window, int64_t min_cmn_window, int32_t center, int32_t norm_vars,
                                int32_t adjoint, void* stream);

/* ---- NCCF pitch tracker (additions to ABI 7; csrc/pitch.h) ----------------------------------------------------------- */

/* F.detect_pitch_frequency (functional/functional.py, detect_pitch_frequency): x is `rows` rows of `length` samples,
 * row r at x + r * row_stride (time stride 1).  The caller computes the sizes with the reference's expressions:
 * frame_size = ceil(sample_rate * frame_time), lags = ceil(sample_rate / freq_low), lag_min = ceil(sample_rate / freq_high).
 * mode 0: out is float32 (rows, n_out), n_out = F + p - win_length + 1 with F = ceil(length / frame_size) and
 *         p = (win_length - 1) / 2: the median-smoothed pitch in Hz, float32 whatever the input type.  `workspace` holds
 *         aamd_detect_pitch_workspace() bytes (one int32 lag per frame), 4-byte aligned.  Needs win_length >= 3,
 *         0 <= lag_min < lags / 2 and n_out >= 1 (AAMD_EINVAL otherwise).
 * mode 1: out is (rows, F, lags) of the input's type: the NCCF the pick of mode 0 reads, bit for bit; no workspace.
 * frame_size > 8192 or lags > 16384 is AAMD_EUNSUPPORTED.  No gradient. */
int64_t aamd_detect_pitch_workspace(int64_t rows, int64_t length, int32_t frame_size);
int aamd_detect_pitch_f32(const float* x, void* out, void* workspace, int64_t rows, int64_t length, int64_t row_stride,
                          int32_t sample_rate, int32_t frame_size, int32_t lags, int32_t lag_min, int32_t win_length,
                          int32_t mode, void* stream);
int aamd_detect_pitch_f64(const double* x, void* out, void* workspace, int64_t rows, int64_t length, int64_t row_stride,
                          int32_t sample_rate, int32_t frame_size, int32_t lags, int32_t lag_min, int32_t win_length,
                          int32_t mode, void* stream);

/* ---- SpecAugment masking (additions to ABI 7; csrc/spec_augment.h) --------------------------------------------------- */

/* element types of aamd_spec_augment_*: they decide the arithmetic of the mask bounds; elements move as 2 / 4 / 8 bytes */
enum { AAMD_SA_F32 = 0, AAMD_SA_F64 = 1, AAMD_SA_F16 = 2, AAMD_SA_BF16 = 3 };
/* axis tag of one mask */
enum { AAMD_SA_FREQ = 0, AAMD_SA_TIME = 1 };

/* A whole masking policy in one launch (functional/functional.py, mask_along_axis_iid / mask_along_axis; transforms,
 * SpecAugment): out[e, o, i] = mask_value where one of the n_masks masks covers (e, o, i), else a bit copy of x[e, o, i].
 * x is (examples, n_outer, n_inner) through its element strides; out is dense in that order.  The caller names as `inner`
 * the axis its storage is contiguous along and says with time_inner whether that axis is time (a time-contiguous
 * (..., freq, time) tensor) or frequency (time_inner = 0: the frame-major storage MelSpectrogram returns); mask m covers
 * axis axes[m] (AAMD_SA_FREQ / AAMD_SA_TIME).  When x is one dense block and x and out are 16-byte aligned the tensor is
 * streamed with 16-byte accesses and vectors that are wholly masked are not read; any other strides are gathered.
 * mask_value: one device element of the tensor's type at value_ptr (no host synchronisation; e.g. specgram.mean()), or,
 * with value_ptr = NULL, the element's bits in value_bits.
 * _iid:    draws holds the raw uniform draws, [n_masks][2][examples] of the tensor's type; example e's mask m is
 *          value = draws[m][0][e] * mask_params[m], min_value = draws[m][1][e] * (size - value), start = (long) min_value,
 *          end = start + (long) value, evaluated in the tensor's type as aten does (size = the length of the mask's axis).
 * _shared: every example takes [starts[m], ends[m]) (cut to the axis).
 * More than 32 masks, an unknown axis tag or element type: AAMD_EINVAL (chain launches beyond 32 masks). */
int aamd_spec_augment_iid(const void* x, void* out, int64_t examples, int64_t n_outer, int64_t n_inner,
                          int64_t stride_example, int64_t stride_outer, int64_t stride_inner, int32_t dtype,
                          int32_t time_inner, int32_t n_masks, const int32_t* axes, const int64_t* mask_params,
                          const void* draws, uint64_t value_bits, const void* value_ptr, void* stream);
int aamd_spec_augment_shared(const void* x, void* out, int64_t examples, int64_t n_outer, int64_t n_inner,
                             int64_t stride_example, int64_t stride_outer, int64_t stride_inner, int32_t dtype,
                             int32_t time_inner, int32_t n_masks, const int32_t* axes, const int64_t* starts,
                             const int64_t* ends, uint64_t value_bits, const void* value_ptr, void* stream);

/* ---- waveform augmentation (additions to ABI 7; csrc/wave_augment.h) ------------------------------------------------ */

enum { AAMD_ADD_NOISE_FORWARD = 0, AAMD_ADD_NOISE_GRADIENT = 1 };

/* F.add_noise (functional/functional.py, add_noise): out = waveform + scale * noise per row, with
 *   scale = 10 ** ((10 (log10 Es - log10 En) - snr) / 20),   Es / En = the sums of waveform^2 / noise^2 over the samples
 * below the row's length.  Two launches: float64 partial sums per (row, chunk) into `workspace`
 * (aamd_add_noise_workspace() bytes, 8-byte aligned; no floating-point atomics, so two calls give the same bits), then the
 * mix over the whole row.  The scale is formed in float64 and rounded once; the product and the sum are rounded separately.
 * Zero energies give what IEEE arithmetic gives (scale 0, +inf or NaN).
 * Operands are (rows, length) with unit stride along time and a row stride in elements each: 0 reads one row for every
 * output row (a broadcast noise), length + k reads rows of a wider tensor; rows that start on a 16-byte boundary move with
 * 16-byte accesses, others sample by sample, nothing is copied.  out (and out2) are dense.  snr[row * stride_snr] (dB) and
 * lengths[row * stride_lengths] (NULL: nothing masked; clamped to [0, length]) are device arrays read by the kernels.
 * mode AAMD_ADD_NOISE_FORWARD:  cotangent and out2 are unused (NULL).
 * mode AAMD_ADD_NOISE_GRADIENT: with d = sum over the row of cotangent * noise and m the length mask,
 *   out = cotangent + d (s / Es) m waveform, out2 = s cotangent - d (s / En) m noise, and the first `rows` doubles of
 *   workspace receive the gradient to snr, -(ln 10 / 20) s d.
 * _lp: float16 / bfloat16 storage (dtype AAMD_SA_F16 / AAMD_SA_BF16), float32 arithmetic, results rounded once. */
int64_t aamd_add_noise_workspace(int64_t rows, int64_t length);
int aamd_add_noise_f32(const float* waveform, const float* noise, const float* cotangent, float* out, float* out2,
                       void* workspace, int64_t rows, int64_t length, int64_t stride_waveform, int64_t stride_noise,
                       int64_t stride_cotangent, const double* snr, int64_t stride_snr, const int64_t* lengths,
                       int64_t stride_lengths, int32_t mode, void* stream);
int aamd_add_noise_f64(const double* waveform, const double* noise, const double* cotangent, double* out, double* out2,
                       void* workspace, int64_t rows, int64_t length, int64_t stride_waveform, int64_t stride_noise,
                       int64_t stride_cotangent, const double* snr, int64_t stride_snr, const int64_t* lengths,
                       int64_t stride_lengths, int32_t mode, void* stream);
int aamd_add_noise_lp(const void* waveform, const void* noise, const void* cotangent, void* out, void* out2, void* workspace,
                      int64_t rows, int64_t length, int64_t stride_waveform, int64_t stride_noise, int64_t stride_cotangent,
                      const double* snr, int64_t stride_snr, const int64_t* lengths, int64_t stride_lengths, int32_t dtype,
                      int32_t mode, void* stream);

/* F.preemphasis (functional/functional.py, preemphasis): out[i] = x[i] - coeff * x[i - 1], out[0] = x[0]; transposed = 1
 * applies the transpose of that map (its gradient), out[i] = x[i] - coeff * x[i + 1], out[length - 1] = x[length - 1].
 * coeff is rounded to the compute type first; the product and the difference are rounded separately, so float32 and
 * float64 results equal the reference's expression bit for bit.  x is (rows, length) with unit stride along time and
 * stride_row elements between rows (any alignment, not copied); out is dense. */
int aamd_preemphasis_f32(const float* x, float* out, int64_t rows, int64_t length, int64_t stride_row, double coeff,
                         int32_t transposed, void* stream);
int aamd_preemphasis_f64(const double* x, double* out, int64_t rows, int64_t length, int64_t stride_row, double coeff,
                         int32_t transposed, void* stream);
int aamd_preemphasis_lp(const void* x, void* out, int64_t rows, int64_t length, int64_t stride_row, double coeff, int32_t dtype,
                        int32_t transposed, void* stream);

/* ---- MVDR beamforming (additions to ABI 7; csrc/beamform.h) ------------------------------------------------------------ */

enum { AAMD_BF_C64 = 0, AAMD_BF_C128 = 1 };
enum { AAMD_BF_SOLVE = 0, AAMD_BF_SOUDEN = 1, AAMD_BF_RTF = 2, AAMD_BF_RTF_POWER = 3 };
#define AAMD_BF_MAX_CHANNELS 16

/* Frequencies per workgroup of the PSD kernel, and its largest time chunk (frames staged at a time; complex128 uses half). */
int32_t aamd_beamform_freq_tile(void);
int32_t aamd_beamform_time_chunk(void);

/* F.psd / T.PSD: out[n][b][f] = sum_t m'_n[b][f][t] x[b][:, f, t] x[b][:, f, t]^H for n < n_masks (or one unweighted sum when
 * mask1 is NULL), m' = m / (sum_t m + eps) when `normalize`.  x is (batch, channels, freq, time) complex (interleaved re, im)
 * read through strides counted in complex elements; stride_f == 1 (frame-major) or stride_t == 1 is read coalesced, anything
 * else is the caller's to gather first (AAMD_EINVAL).  Masks are real (batch, freq, time) of the matching precision, any
 * non-negative strides (in elements), two of them give both matrices from one pass.  out is dense
 * (n, batch, freq, channels, channels), exactly Hermitian.  One launch, float64 sums in a fixed order, no atomics. */
int aamd_beamform_psd(int32_t dtype, const void* x, int64_t batch, int64_t channels, int64_t freq, int64_t time,
                      int64_t stride_b, int64_t stride_c, int64_t stride_f, int64_t stride_t, const void* mask1,
                      const int64_t* mask1_strides, const void* mask2, const int64_t* mask2_strides, int32_t normalize,
                      double eps, void* out, void* stream);

/* The per-bin small solve behind F.mvdr_weights_souden, F.mvdr_weights_rtf and F.rtf_power: one launch, LU with partial
 * pivoting in float64, bins = batch * freq.  a is (bins, C, C) dense; with `loading`, a + (Re tr a * diag_eps + 1e-8) I is
 * used wherever a is.  `reference` >= 0 selects a channel; otherwise reference_vector (batch, C) complex is used (both absent:
 * AAMD_BF_RTF without a reference).
 *   AAMD_BF_SOLVE      b (bins, C, K), K <= C: out (bins, C, K) = a^-1 b; adjoint = 1 inverts a^H instead
 *   AAMD_BF_SOUDEN     b (bins, C, C): N = a^-1 b, out (bins, C) = N[:, ref] / (tr N + eps)   (or N u / ...)
 *   AAMD_BF_RTF        b (bins, C) = r: n = a^-1 r, out = n / (Re(r^H n) + eps) [* conj(r[ref]) or sum_c conj(r_c) u_c]
 *   AAMD_BF_RTF_POWER  b (bins, C, C): phi = a^-1 b, r = phi[:, ref] (or phi u), n_iter - 2 times r <- phi r, then
 *                      r <- b r (n_iter >= 2) or r <- a r (n_iter == 1); out (bins, C) = r */
int aamd_beamform_weights(int32_t dtype, int32_t mode, const void* a, const void* b, const void* reference_vector, void* out,
                          int64_t batch, int64_t freq, int32_t channels, int32_t rhs, int32_t reference, int32_t loading,
                          double diag_eps, double eps, int32_t n_iter, int32_t adjoint, void* stream);

/* F.apply_beamforming: out[b][f][t] = sum_c conj(w[b][f][c]) x[b][c][f][t].  w dense (batch, freq, channels); x as for
 * aamd_beamform_psd; out (batch, freq, time) through out_strides (complex elements), unit stride along the same axis as x. */
int aamd_beamform_apply(int32_t dtype, const void* w, const void* x, int64_t batch, int64_t channels, int64_t freq,
                        int64_t time, int64_t stride_b, int64_t stride_c, int64_t stride_f, int64_t stride_t, void* out,
                        const int64_t* out_strides, void* stream);

/* ---- RNN transducer loss (additions to ABI 7; csrc/rnnt_loss.h) -------------------------------------------------------- */

#define AAMD_RNNT_MAX_U1 1024        /* the longest target axis (U + 1) the lattice kernel serves */

/* Lanes per (b, t, u) row that the row and gradient passes use for a vocabulary of `vocab` entries of element type `dtype`
 * (AAMD_SA_F32 / F64 / F16 / BF16): 8, 16, 32 or 64.  The lattice workgroup's thread count. */
int32_t aamd_rnnt_team_width(int32_t dtype, int64_t vocab);
int32_t aamd_rnnt_lattice_threads(void);

/* Bytes of device workspace a forward call needs and a backward call reads again (8-byte aligned): denominators, the two
 * log-probabilities per cell, alpha and beta as float64 (batch, max_t, max_u1) each, and one flag per example. */
int64_t aamd_rnnt_loss_workspace(int64_t batch, int64_t max_t, int64_t max_u1);

/* Forward.  logits dense (batch, max_t, max_u1, vocab) of `dtype` (AAMD_SA_*), targets dense (batch, max_u1 - 1) int32,
 * logit_lengths / target_lengths (batch,) int32, all on the device and read there: no synchronisation.  blank in [0, vocab).
 * fused_log_softmax != 0: the log-softmax over vocab is part of the loss (one streaming read of logits); 0: logits holds
 * log-probabilities.  costs (batch,) float64 = -log P(targets | logits) per example.  An example with a logit length outside
 * [1, max_t], a target length outside [0, max_u1 - 1] or a live target outside [0, vocab) gets a NaN cost, and nothing is
 * indexed with those values.  max_u1 > AAMD_RNNT_MAX_U1: AAMD_EUNSUPPORTED.  Two launches (row pass, lattice). */
int aamd_rnnt_loss_forward(int32_t dtype, const void* logits, const int32_t* targets, const int32_t* logit_lengths,
                           const int32_t* target_lengths, int64_t batch, int64_t max_t, int64_t max_u1, int64_t vocab,
                           int32_t blank, int32_t fused_log_softmax, void* workspace, double* costs, void* stream);

/* Backward, from the workspace a forward call with the same arguments left: grad (as logits) = d costs[b] / d logits,
 * clamped to [-clamp, clamp] when clamp > 0, times grad_costs[b] (float64, read on the device).  Exactly zero where
 * t >= logit_lengths[b] or u > target_lengths[b]; NaN over the whole block of an example whose cost is NaN.  One launch when
 * fused (one read of logits, one write of grad), two otherwise. */
int aamd_rnnt_loss_backward(int32_t dtype, const void* logits, const int32_t* targets, const int32_t* logit_lengths,
                            const int32_t* target_lengths, int64_t batch, int64_t max_t, int64_t max_u1, int64_t vocab,
                            int32_t blank, int32_t fused_log_softmax, double clamp, const void* workspace,
                            const double* grad_costs, void* grad, void* stream);

/* ---- CTC forced alignment (additions to ABI 7; csrc/forced_align.h) -------------------------------------------------- */

#define AAMD_FORCED_ALIGN_MAX_L 2047 /* the longest transcript axis the forward kernel serves (2 L + 1 states) */

/* What the launcher picks for a transcript axis of max_l labels: consecutive states per lane (4 or 16) and lanes per
 * workgroup (64 or 256); the steps the forward's gathers run ahead; the frames per block of the backtrack. */
int32_t aamd_forced_align_states_per_lane(int64_t max_l);
int32_t aamd_forced_align_threads(int64_t max_l);
int32_t aamd_forced_align_prefetch(void);
int32_t aamd_forced_align_backtrack_block(void);

/* Bytes of device workspace a call needs (16-byte aligned; written and read on the device only): one int32 per example and
 * 2 bits per (example, frame, state).  0 for max_l > AAMD_FORCED_ALIGN_MAX_L. */
int64_t aamd_forced_align_workspace(int64_t batch, int64_t max_t, int64_t max_l);

/* F.forced_align.  log_probs dense (batch, max_t, classes) of `dtype` (AAMD_SA_*), targets dense (batch, max_l) int32 or
 * int64 (targets_int64), input_lengths / target_lengths (batch,) int32 or int64 (lengths_int64), all on the device and read
 * there: no synchronisation.  blank in [0, classes).  paths (batch, max_t) of the targets' type: the label of the Viterbi
 * state of every frame (float64 accumulation; ties keep the smaller move); scores (batch, max_t) of `dtype`:
 * log_probs[b][t][paths[b][t]] copied bit for bit.  Frames from input_lengths[b] on: blank / 0.  An example with an input
 * length outside [1, max_t], a target length outside [0, max_l], fewer frames than labels plus adjacent equal labels, or a
 * live label outside [0, classes) or equal to blank gets -1 / NaN over its whole row, and nothing is indexed with those
 * values.  max_l > AAMD_FORCED_ALIGN_MAX_L: AAMD_EUNSUPPORTED.  Two launches (forward, backtrack). */
int aamd_forced_align(int32_t dtype, const void* log_probs, const void* targets, int32_t targets_int64,
                      const void* input_lengths, const void* target_lengths, int32_t lengths_int64, int64_t batch,
                      int64_t max_t, int64_t classes, int64_t max_l, int32_t blank, void* workspace, void* paths, void* scores,
                      void* stream);

/* ---- SoX-style effects (additions to ABI 7; csrc/effects.h) ----------------------------------------------------------- */

enum { AAMD_FX_OVERDRIVE = 0, AAMD_FX_PHASER = 1, AAMD_FX_FLANGER = 2 };
#define AAMD_PHASER_MAX_RING 512      /* the longest delay ring (samples) the phaser kernel serves */
#define AAMD_FLANGER_MAX_RING 4096    /* ... and the flanger kernels: 40 ms at 96 kHz */
#define AAMD_EFFECTS_MAX_TABLE (1 << 24) /* the longest modulation table */

/* which = 0: rows per workgroup of the delay-line kernel; 1: samples per LDS tile; 2: samples per overdrive chunk. */
int32_t aamd_effects_tiles(int32_t which);

/* Bytes of device workspace a call needs (written and read on the device only).  AAMD_FX_OVERDRIVE: one double per (row,
 * chunk); `ring` is ignored.  AAMD_FX_PHASER / AAMD_FX_FLANGER: 0 where the delay ring of `ring` samples per row fits the
 * LDS for `dtype` (AAMD_SA_*), else one ring per row of every workgroup (16-byte aligned). */
int64_t aamd_effects_workspace(int32_t effect, int32_t dtype, int64_t rows, int64_t length, int64_t ring);

/* Every effect: x is (rows, length) of `dtype` (AAMD_SA_*) with unit stride along time and row_stride elements between
 * rows, out is dense (rows, length) of the same type; float16 / bfloat16 compute in float32 and are rounded once.  Results
 * are clamped to [-1, 1]; a NaN stays a NaN.
 *
 * F.overdrive: gain = 10 ^ (dB / 20) and colour = colour / 200 are rounded to the compute type; the recurrence state is
 * float64 for every type.  Two launches (one for rows of one chunk), no atomics: two calls give the same bits. */
int aamd_overdrive(int32_t dtype, const void* x, void* out, void* workspace, int64_t rows, int64_t length,
                   int64_t row_stride, double gain, double colour, void* stream);

/* F.phaser: table is int32[table_len] on the device with entries in [1, ring] (the reference's modulation buffer); the
 * result equals the reference's loop bit for bit.  ring > AAMD_PHASER_MAX_RING or table_len > AAMD_EFFECTS_MAX_TABLE:
 * AAMD_EUNSUPPORTED. */
int aamd_phaser(int32_t dtype, const void* x, void* out, void* workspace, int64_t rows, int64_t length, int64_t row_stride,
                const int32_t* table, int64_t table_len, int64_t ring, double gain_in, double gain_out, double decay,
                void* stream);

/* F.flanger: row r is channel r % channels (channels <= 4); table is float[table_len] on the device with entries in
 * [0, ring - 2] (the reference's lfo); channel_phase is a HOST array of `channels` offsets into the table.  The result equals
 * the reference's loop bit for bit.  feedback_gain == 0 and general == 0: the streaming gather, which reads x as stored
 * (a -0.0 is not turned into +0.0, a non-finite sample reaches only the outputs whose taps read it) and needs no workspace.
 * ring > AAMD_FLANGER_MAX_RING or table_len > AAMD_EFFECTS_MAX_TABLE: AAMD_EUNSUPPORTED. */
int aamd_flanger(int32_t dtype, const void* x, void* out, void* workspace, int64_t rows, int64_t length, int64_t row_stride,
                 int32_t channels, const float* table, int64_t table_len, const int64_t* channel_phase, int64_t ring,
                 double feedback_gain, double in_gain, double delay_gain, int32_t quadratic, int32_t general, void* stream);

/* ---- CTC prefix beam search (additions to ABI 7; csrc/ctc_decoder.h) ------------------------------------------------- */

#define AAMD_CTC_DECODER_MAX_BEAM 32 /* the widest beam the beam kernel serves */

/* The widest beam; threads per workgroup of the row pass (one wave per frame) and of the beam pass (one workgroup of four
 * waves per example); for a beam of `beam`, the (value, token) slots of a frame's record (beam + 1) and the candidates of a
 * frame (per entry: the stay, one extension per record slot, the extension by its own last token: beam * (beam + 3)); the
 * two size limits beyond the 32-bit ones: the most frames of a call (batch * max_t) and the most trie nodes of an example
 * (1 + beam * max_t). */
int32_t aamd_ctc_decoder_max_beam(void);
int32_t aamd_ctc_decoder_row_threads(void);
int32_t aamd_ctc_decoder_beam_threads(void);
int32_t aamd_ctc_decoder_record_slots(int32_t beam);
int32_t aamd_ctc_decoder_candidates(int32_t beam);
int64_t aamd_ctc_decoder_max_frames(void);
int64_t aamd_ctc_decoder_max_nodes(void);

/* Bytes of device workspace a call needs (16-byte aligned; written and read on the device only): a record of beam + 1
 * (value, token) pairs per frame and 1 + beam * max_t trie nodes per example.  0 for sizes the search does not serve. */
int64_t aamd_ctc_decoder_workspace(int64_t batch, int64_t max_t, int64_t vocab, int64_t beam);

/* audio_amd.models.decoder.ctc_beam_search: CTC prefix beam search without a language model.  log_probs dense (batch,
 * max_t, vocab) of `dtype` (AAMD_SA_*), lengths (batch,) int32 or int64 (lengths_int64), on the device and read there: no
 * synchronisation.  A frame with log_probs[b][t][blank] > threshold is skipped entirely; float64 accumulation for every
 * dtype; a candidate whose score is -inf or NaN is never kept.  tokens (batch, nbest, max_t) int32, zero beyond each
 * length; token_lengths (batch, nbest) int32, -1 where the beam held fewer hypotheses; scores (batch, nbest) float64 in
 * descending order, -inf for a missing hypothesis.  An example with a length outside [0, max_t] gets lengths -1 and scores
 * NaN, and nothing is indexed with that length.  beam > AAMD_CTC_DECODER_MAX_BEAM, batch / max_t / vocab >= 2^31,
 * batch * max_t > aamd_ctc_decoder_max_frames() (2^36) or 1 + beam * max_t > aamd_ctc_decoder_max_nodes() (2^31 - 1):
 * AAMD_EUNSUPPORTED.  Two launches (row pass, beam pass). */
int aamd_ctc_beam_search(int32_t dtype, const void* log_probs, const void* lengths, int32_t lengths_int64, int64_t batch,
                         int64_t max_t, int64_t vocab, int32_t blank, int32_t beam, int32_t nbest, double threshold,
                         void* workspace, int32_t* tokens, int32_t* token_lengths, double* scores, void* stream);

/* ---- InverseMelScale (additions to ABI 7; csrc/inverse_mel.h) -------------------------------------------------------- */

#define AAMD_INVERSE_MEL_MAX_MELS 256 /* the most mel bins the kernel serves (both operands of a tile live in LDS) */

/* which = 0: frames of one row per workgroup; 1: bins of n_stft per LDS tile; 2: the most mel bins (the define above). */
int32_t aamd_inverse_mel_tiles(int32_t which);

/* F.inverse_mel_scale: out[r][t][f] = relu(sum_m pinv[f][m] * y[r][m][t]), y = x or, with log_input, expf(x).  x is
 * (rows, n_mels, frames) of `dtype` (AAMD_SA_F32 / F16 / BF16) read in place through its strides in elements: unit stride
 * along mel (stride_mel == 1: frame-major) or along time (stride_frame == 1); anything else is AAMD_EINVAL (gather first).
 * pinv is the (n_stft, n_mels) float32 matrix on the device, 16-byte aligned, laid out tile by tile as the kernel reads it:
 * ceil(n_stft / 64) tiles of 64 * K4 floats (K4 = n_mels rounded up to 4), element (m, j) of a tile -- j the row within
 * the tile -- at ((m / 4) * 4 + j / 16) * 64 + (m % 4) * 16 + j % 16, zeros beyond n_stft and n_mels
 * (_host.inverse_mel_fragments).  out is dense (rows, frames, n_stft) of `dtype`.  float32 FMA chains
 * in ascending m on the matrix cores, one accumulator per output, rounded once to `dtype`: the result does not depend on
 * the layout, the alignment or the number of rows.  n_mels > AAMD_INVERSE_MEL_MAX_MELS: AAMD_EUNSUPPORTED.  One launch. */
int aamd_inverse_mel(int32_t dtype, const void* x, const float* pinv, void* out, int64_t rows, int64_t frames,
                     int64_t stride_row, int64_t stride_mel, int64_t stride_frame, int32_t n_stft, int32_t n_mels,
                     int32_t log_input, void* stream);

/* ---- Voice-activity trimming (additions to ABI 7; csrc/vad.h) --------------------------------------------------------- */

#define AAMD_VAD_MAX_FFT 8192 /* the largest measurement transform the kernels serve (the defaults up to 81.9 kHz) */

/* which = 0: threads per workgroup of the measurement kernels; 1: the largest transform (the define above); 2: the
 * smallest (16); 3: rows per workgroup of the trigger kernel. */
int32_t aamd_vad_tiles(int32_t which);

/* Bytes of device workspace of aamd_vad_measure: one float per (row, frame, spectrum bin), bins = s1 - s0. */
int64_t aamd_vad_workspace(int64_t rows, int64_t frames, int64_t bins);

/* The measurements of F.vad: x is (rows, length) of `dtype` (AAMD_SA_*) with unit stride along time and row_stride elements
 * between rows, every row a recording of its own; arithmetic is float32 for every type.  Frame f = 0 .. frames - 1 ends at
 * sample win + f * period (frames = the count of f with win + f * period < length, checked): the magnitude spectrum of the
 * last `win` samples (n_fft points, a power of two in [16, AAMD_VAD_MAX_FFT]; larger: AAMD_EUNSUPPORTED) over the bins
 * [s0, s1), smoothed (f / (1 + f) while f <= boot_max, then `smooth`), reduced by noise_reduction times the tracked noise
 * floor (`up` where the smoothed power exceeds it, else `down`), and the power of the n_fft / 2-point transform of the
 * result over [c0, c1): meas[row][f] = max(0, 21 + log(power / (c1 - c0))), 0 unless power > 0.  tables is float[win +
 * (s1 - s0) + n_fft] on the device: the measurement window, the cepstrum window and (cos, -sin)(2 pi k / n_fft) for
 * k < n_fft / 2 (_host.vad_tables).  meas is dense (rows, frames).  Three launches, no atomics: two calls give the same
 * bits. */
int aamd_vad_measure(int32_t dtype, const void* x, int64_t rows, int64_t length, int64_t row_stride, int32_t win, int32_t n_fft,
                     int32_t period, int32_t s0, int32_t s1, int32_t c0, int32_t c1, int32_t boot_max, double smooth, double up,
                     double down, double noise_reduction, const float* tables, void* workspace, float* meas, int64_t frames,
                     void* stream);

/* The trigger of F.vad over dense (rows, frames) measurements (any float32 values, a NaN never triggers): first[row] = the
 * first frame at which the float64 mean, mean = mean * trigger_mult + meas * (1 - trigger_mult), reaches trigger_level, or
 * -1; start[row] = max(0, (first - flush) * period - fixed) with flush from the scan back over the last `ring` measurements
 * (zeros before frame 0; `gap` measurements below the level are bridged), or -1.  joint, where not null, receives one
 * value: the same with the least first of all rows and the largest flush, at that frame, of the rows from the least row
 * that has it on; -1 where no row triggers.  One launch, two with joint; exact, in integers and float64. */
int aamd_vad_trigger(const float* meas, int64_t rows, int64_t frames, int64_t ring, int64_t gap, int64_t period, int64_t fixed,
                     double trigger_level, double trigger_mult, int64_t* first, int64_t* start, int64_t* joint, void* stream);

/* ---- Spectral centroid (additions to ABI 7; csrc/spectral_feat.h) ---------------------------------------------------- */

/* which = 0: threads per workgroup; 1: float32 values per 16-byte vector; 2: the most lanes that share a frame line. */
int32_t aamd_spectral_tiles(int32_t which);

/* Lanes that share a frame line of n_freq bins with unit stride along frequency: the power of two that leaves a lane about
 * four 16-byte vectors (it covers ceil(ceil(n_freq / 4) / 4)), at most 64; 0 for n_freq < 1. */
int32_t aamd_spectral_lanes(int64_t n_freq);

/* The reduction of F.spectral_centroid: out[r][t] = sum_k freqs[k] mag[r][t][k] / sum_k mag[r][t][k].  mag is float32
 * (rows, frames, n_freq) read in place through its strides in elements (any non-negative strides; unit stride along
 * frequency takes 16-byte loads, several lanes per frame line); freqs is float32[n_freq] on the device, 16-byte aligned;
 * out is dense (rows, frames) of out_dtype (AAMD_SA_F32 / F16 / BF16).  Both sums are float64, each lane adds its bins in
 * ascending order and the lanes of a frame combine in one fixed tree, then one float64 division and one rounding.  A frame
 * of zeros gives NaN.  One launch, no atomics: two calls give the same bits. */
int aamd_spectral_centroid(int32_t out_dtype, const float* mag, const float* freqs, void* out, int64_t rows, int64_t frames,
                           int64_t n_freq, int64_t stride_row, int64_t stride_frame, int64_t stride_freq, void* stream);

/* ---- Pointwise waveform ops (additions to ABI 7; csrc/wave_pointwise.h) ---------------------------------------------- */

enum { AAMD_PW_SCALE = 0, AAMD_PW_CONTRAST = 1, AAMD_PW_DB_TO_AMPLITUDE = 2, AAMD_PW_MU_ENCODE = 3, AAMD_PW_MU_DECODE = 4,
       AAMD_PW_FADE = 5 };
/* element types beyond AAMD_SA_*: the integer codes AAMD_PW_MU_DECODE reads */
enum { AAMD_PW_I64 = 4, AAMD_PW_I32 = 5, AAMD_PW_I16 = 6, AAMD_PW_I8 = 7, AAMD_PW_U8 = 8 };

/* which = 0: threads per workgroup; 1: samples per workgroup; 2: 16-byte groups a thread keeps in flight. */
int32_t aamd_pointwise_tiles(int32_t which);

/* One streaming pass over x, (rows, length) of `dtype` with unit stride along time and row_stride elements between rows,
 * into dense out.  float32 and float64 compute in their own precision; float16 and bfloat16 in float32, rounded once.
 *   AAMD_PW_SCALE            out = x * p0, clamped to [-1, 1] where flag != 0                  (F.gain, T.Vol)
 *   AAMD_PW_CONTRAST         t = x * p0; out = sin(t + p1 * sin(t * 4))                        (F.contrast: p0 = pi / 2)
 *   AAMD_PW_DB_TO_AMPLITUDE  out = p0 * pow(pow(10, 0.1 * x), p1)                              (p0 = ref, p1 = power)
 *   AAMD_PW_MU_ENCODE        v = sign(x) log1p(p0 |x|) / log1p(p0); out = int64((v + 1) / 2 * p0 + 0.5), toward zero;
 *                            out is int64 for every dtype (p0 = quantization_channels - 1 >= 1)
 *   AAMD_PW_MU_DECODE        y = x / p0 * 2 - 1; out = sign(y) (exp(|y| log1p(p0)) - 1) / p0; dtype may be AAMD_PW_I64 ..
 *                            AAMD_PW_U8: the codes are read as they are and out is float32
 *   AAMD_PW_FADE             out = (fade_in * fade_out) * x: table holds the fade-in ramp (n_in values) and the fade-out
 *                            ramp (n_out values, the last n_out samples of a row) in `dtype`, n_in, n_out <= length;
 *                            a sample outside both ramps is copied bit for bit
 * table, n_in and n_out are read by AAMD_PW_FADE only.  One launch. */
int aamd_pointwise(int32_t op, int32_t dtype, const void* x, void* out, int64_t rows, int64_t length, int64_t row_stride,
                   double p0, double p1, int32_t flag, const void* table, int64_t n_in, int64_t n_out, void* stream);

/* ---- Image-source room impulse responses (additions to ABI 7; csrc/rir.h) --------------------------------------------- */

#define AAMD_RIR_MAX_FILTER 1025 /* the longest fractional-delay filter (taps, odd) the kernel serves */
#define AAMD_RIR_MAX_ORDER 64    /* the largest reflection order: 357 889 images in 3-D */

/* which = 0: samples per workgroup; 1: images per chunk; 2: AAMD_RIR_MAX_FILTER; 3: AAMD_RIR_MAX_ORDER. */
int32_t aamd_rir_tiles(int32_t which);

/* F.simulate_rir_ism_batch: out[b][c][n] = sum_i a g(n - pad - tau), 0 <= n < out_len, over the images i of `lattice` in
 * ascending order, with pad = filter_len / 2, g(x) = sinc(x) (1 + cos(pi x / pad)) / 2 for |x| <= pad and 0 elsewhere.
 * room and source are dense (batch, dims), mic dense (batch, mics, dims), absorption dense (batch, 2 dims) in the order lower
 * wall, upper wall of each axis, out dense (batch, mics, out_len): all of `dtype` (AAMD_SA_F32 or AAMD_SA_F64), on the
 * device.  lattice is int16 (n_img, dims) on the device: every integer vector v with sum |v_d| <= max_order, last axis
 * fastest (n_img must be that count).  Per image and axis loc = room (v + 1) - source for odd v, room v + source for even v;
 * att = prod_d sqrt(1 - absorption_lower)^|floor(v / 2)| sqrt(1 - absorption_upper)^|floor((v + 1) / 2)|; dist = |loc - mic|,
 * a = att / dist, tau = dist sample_rate / sound_speed.  Geometry, filter argument and sums are float64 for both element
 * types and a float32 result is rounded once.  A (room, microphone) row with a non-finite a or tau is NaN throughout.  No
 * atomics, sums in image order: the bits of a sample do not depend on batch, mics or out_len.  dims outside {2, 3}, an even
 * or short filter: AAMD_EINVAL; filter_len > AAMD_RIR_MAX_FILTER or max_order > AAMD_RIR_MAX_ORDER: AAMD_EUNSUPPORTED.  One
 * launch. */
int aamd_simulate_rir(int32_t dtype, const void* room, const void* source, const void* mic, const void* absorption,
                      const int16_t* lattice, int64_t n_img, void* out, int64_t batch, int64_t mics, int32_t dims,
                      int32_t max_order, int32_t filter_len, int64_t out_len, double sample_rate, double sound_speed,
                      void* stream);

/* ---- Ray-traced energy histograms of shoebox rooms (additions to ABI 7; csrc/ray_trace.h) ----------------------------- */

#define AAMD_RAY_MAX_BANDS 8         /* frequency bands of the coefficients */
#define AAMD_RAY_MAX_MICS 16         /* microphones of a room */
#define AAMD_RAY_MAX_RAYS 16777216   /* 2^24 rays */
#define AAMD_RAY_MAX_BINS 65536      /* histogram bins */
#define AAMD_RAY_MAX_BOUNCES 4096    /* the cap on a room's bounce bound sum_d (floor(S_max / room_d) + 2) */
#define AAMD_RAY_HEADROOM 64         /* contributions of EVERY ray one (microphone, bin) may take before its sum can wrap */

/* which = 0: rays per workgroup; 1: AAMD_RAY_MAX_BANDS; 2: AAMD_RAY_MAX_MICS; 3: AAMD_RAY_MAX_RAYS; 4: AAMD_RAY_MAX_BINS;
 * 5: AAMD_RAY_MAX_BOUNCES; 6: AAMD_RAY_HEADROOM. */
int32_t aamd_ray_tiles(int32_t which);

/* F.ray_tracing_batch: out[b][m][band][bin] = the energy that the num_rays rays of room b leave at microphone m (the
 * definition: the docstring of F.ray_tracing, restated by tests/ray_oracle.py).  room and source are dense (batch, dims), mic
 * dense (batch, mics, dims), absorption and scattering dense (batch, bands, 2 dims) in the order lower wall, upper wall of
 * each axis, out dense (batch, mics, bands, num_bins): all of `dtype` (AAMD_SA_F32 or AAMD_SA_F64), on the device.  acc is
 * an int64 buffer of out's shape that is ZERO on entry: every contribution e is added to it as rint(e 2^scale_log2) with
 * 64-bit integer atomics, so the sums do not depend on the order of arrival, and out = acc 2^-scale_log2 rounded to the
 * element type.  The caller forms scale_log2 = 62 - ceil(log2(8 AAMD_RAY_HEADROOM / mic_radius^2)) from mic_radius alone;
 * an accumulator that wrapped (negative) gives NaN.  Geometry and energies are float64 for both element types.  A bad room
 * -- a dimension that is not finite and positive, a source or microphone not strictly inside, a coefficient outside [0, 1]
 * or NaN, a bounce bound above AAMD_RAY_MAX_BOUNCES with S_max = time_thres sound_speed -- is NaN throughout and no ray of
 * it is traced; the other rooms keep their bits.  The bounce loop of a ray is bounded by the room's bounce bound whatever
 * the data.  dims outside {2, 3}, a non-positive or non-finite scalar: AAMD_EINVAL; bands, mics, num_rays or num_bins
 * above the limits: AAMD_EUNSUPPORTED.  Two launches (trace, convert), no synchronisation. */
int aamd_ray_trace(int32_t dtype, const void* room, const void* source, const void* mic, const void* absorption,
                   const void* scattering, int64_t* acc, void* out, int64_t batch, int64_t mics, int32_t dims, int32_t bands,
                   int64_t num_rays, int64_t num_bins, int32_t scale_log2, double mic_radius, double sound_speed,
                   double energy_thres, double time_thres, double hist_bin_size, void* stream);

/* ---- Synthesis ops (additions to ABI 7; csrc/dsp_synth.h)------------------------------------------------------------- */

#define AAMD_DSP_MAX_TAPS 2049        /* the longest filter of aamd_filter_waveform */
#define AAMD_DSP_MAX_OSCILLATORS 256  /* the most oscillators of aamd_oscillator_bank */
#define AAMD_DSP_MAX_MAGNITUDES 4097  /* the most magnitudes of aamd_frequency_impulse_response */
enum { AAMD_DSP_SUM = 0, AAMD_DSP_MEAN = 1, AAMD_DSP_NONE = 2 };

/* which = 0: time steps per chunk of the oscillator scan; 1: outputs per workgroup of the filter; 2: AAMD_DSP_MAX_TAPS;
 * 3: AAMD_DSP_MAX_OSCILLATORS; 4: AAMD_DSP_MAX_MAGNITUDES. */
int32_t aamd_dsp_tiles(int32_t which);

/* Bytes of workspace aamd_oscillator_bank needs (float64 chunk sums); -1 on a negative size. */
int64_t aamd_oscillator_workspace(int64_t rows, int64_t time, int64_t n);

/* prototype.functional.oscillator_bank: freq and amp are (rows, time, n) of `dtype` (AAMD_SA_*), dense within a row, rows
 * `*_row_stride` elements apart.  In the compute type (float32; double for AAMD_SA_F64): w = remainder((f * 2 pi) /
 * sample_rate, 2 pi), each operation rounded once; phi = the inclusive prefix sum of w over time in float64, reduced to
 * [-pi, pi] with a two-term 2 pi and rounded once; a' = 0 where |f| >= sample_rate / 2.  AAMD_DSP_NONE writes a' sin(phi) to
 * out (rows, time, n); AAMD_DSP_SUM / _MEAN write one fused multiply-add chain over ascending n to out (rows, time), the
 * mean divided once.  Two launches (one where time fits one chunk), no atomics: bits depend on neither rows nor time.
 * n > AAMD_DSP_MAX_OSCILLATORS: AAMD_EUNSUPPORTED.  With n == 0 nothing is written. */
int aamd_oscillator_bank(int32_t dtype, const void* freq, const void* amp, void* out, void* workspace, int64_t rows, int64_t time,
                         int64_t n, int64_t freq_row_stride, int64_t amp_row_stride, double sample_rate, int32_t reduction,
                         void* stream);

/* prototype.functional.filter_waveform: out[r][i] = sum_j x[r][m] h[m / C][j], m = i + (taps - 1) / 2 - j in [0, time),
 * C = time / num_filters, one accumulator per output in ascending m (fused multiply-adds in the compute type).  x is
 * (rows, time) with unit stride along time and rows `row_stride` elements apart, kernels dense (num_filters, taps), or
 * (rows, num_filters, taps) where `batched`; out dense (rows, time).  taps > AAMD_DSP_MAX_TAPS: AAMD_EUNSUPPORTED. */
int aamd_filter_waveform(int32_t dtype, const void* x, const void* kernels, void* out, int64_t rows, int64_t time,
                         int64_t row_stride, int64_t num_filters, int32_t taps, int32_t batched, void* stream);

/* First-order adjoints of the two ops above (csrc/dsp_synth_grad.h); additions to ABI 7 as well.
 * which = 0: samples per unit of time of the filter-gradient reduction; 1: lags per workgroup of it. */
int32_t aamd_dsp_grad_tiles(int32_t which);

/* Bytes of workspace aamd_oscillator_bank_grad needs (float64 chunk sums of w and chunk totals); -1 on a negative size. */
int64_t aamd_oscillator_grad_workspace(int64_t rows, int64_t time, int64_t n);

/* The gradient of aamd_oscillator_bank: grad_out is dense (rows, time), or (rows, time, n) for AAMD_DSP_NONE (AAMD_DSP_MEAN
 * divides it by n in the compute type); grad_freq and grad_amp are dense (rows, time, n), and a null one is not computed.
 * The phase is the forward's, bit for bit.  grad_amp = g sin(phi) where the oscillator is live, (g sin(phi)) * 0 where
 * |f| >= sample_rate / 2; grad_freq = (2 pi / sample_rate) sum_{s >= t} g a' cos(phi): a float64 suffix sum in a fixed order
 * (slices of a chunk, then chunks through the workspace), rounded once.  Two or three launches, no atomics. */
int aamd_oscillator_bank_grad(int32_t dtype, const void* freq, const void* amp, const void* grad_out, void* grad_freq, void* grad_amp,
                              void* workspace, int64_t rows, int64_t time, int64_t n, int64_t freq_row_stride, int64_t amp_row_stride,
                              double sample_rate, int32_t reduction, void* stream);

/* Bytes of workspace aamd_filter_waveform_grad needs for grad_kernels (float64 partial sums; 0 where every sum is formed by
 * one workgroup); -1 on sizes the op refuses. */
int64_t aamd_filter_waveform_grad_workspace(int64_t rows, int64_t time, int64_t num_filters, int32_t taps, int32_t batched);

/* The gradient of aamd_filter_waveform: grad_out dense (rows, time); grad_x dense (rows, time), grad_kernels dense in the
 * shape of kernels; a null one is not computed (kernels may then be null for grad_kernels alone, x for grad_x alone).
 * grad_x[m] = sum_j h[m / C][j] g[m - d + j], one fused multiply-add chain in ascending j in the compute type;
 * grad_kernels[c][j] = sum over the m of chunk c (and over the rows where the filters are shared) of x[m] g[m - d + j],
 * accumulated in float64 in a fixed order (time, then rows) and rounded once.  No atomics. */
int aamd_filter_waveform_grad(int32_t dtype, const void* x, const void* kernels, const void* grad_out, void* grad_x, void* grad_kernels,
                              void* workspace, int64_t rows, int64_t time, int64_t row_stride, int64_t num_filters, int32_t taps,
                              int32_t batched, void* stream);

/* prototype.functional.sinc_impulse_response: cutoff (rows,) -> out (rows, window_size), float32 or float64, evaluated in
 * float64 and rounded once: g[i] = sinc(cutoff i) hamming(window_size)[i + half], h = g / |sum g|; high_pass negates h and
 * adds 1 to the centre tap.  One launch. */
int aamd_sinc_impulse_response(int32_t dtype, const void* cutoff, void* out, int64_t rows, int32_t window_size, int32_t high_pass,
                               void* stream);

/* prototype.functional.frequency_impulse_response: magnitudes (rows, n) -> out (rows, N), N = 2 (n - 1), float32 or float64:
 * the inverse real FFT as one fused multiply-add chain over ascending j per tap, shifted by N / 2 and multiplied by the
 * symmetric Hann window.  table is cos(2 pi q / N), q < N, of `dtype` on the device.  n > AAMD_DSP_MAX_MAGNITUDES:
 * AAMD_EUNSUPPORTED.  One launch. */
int aamd_frequency_impulse_response(int32_t dtype, const void* magnitudes, const void* table, void* out, int64_t rows, int32_t n,
                                    void* stream);

/* prototype.functional.extend_pitch: out[i][k] = base[i] * pattern[k], i < count, k < n, of `dtype`; the half types
 * multiply in float32 and round once.  One launch. */
int aamd_extend_pitch(int32_t dtype, const void* base, const void* pattern, void* out, int64_t count, int64_t n, void* stream);

/* ---- Dense filterbank projection (additions to ABI 7; csrc/dense_fbank.h) -------------------------------------------- */

#define AAMD_DENSE_FBANK_MAX_OUT 128    /* the most outputs (filters) the kernel serves: 8 accumulators per wave */
#define AAMD_DENSE_FBANK_MAX_FREQS 4097 /* the most frequency bins: n_fft = 8192 */

/* which = 0: frames of one row per workgroup; 1: bins of n_freqs per LDS tile; 2: the most outputs; 3: the most bins (the
 * defines above). */
int32_t aamd_dense_fbank_tiles(int32_t which);

/* F.dense_fbank_scale / T.ChromaScale: out[r][t][n] = sum_k x[r][k][t] * w[k][n].  x is (rows, n_freqs, frames) of `dtype`
 * (AAMD_SA_F32 / F16 / BF16) read in place through its strides in elements: unit stride along freq (stride_freq == 1:
 * frame-major) or along time (stride_frame == 1); anything else is AAMD_EINVAL (gather first).  w is the (n_freqs, n_out)
 * float32 filterbank on the device, 16-byte aligned, in the order the kernel reads it: K4 / 4 * NT * 64 floats (K4 = n_freqs
 * rounded up to 4, NT = ceil(n_out / 16)), element (k, n) at ((k / 4) * NT + n / 16) * 64 + (k % 4) * 16 + n % 16, zeros
 * beyond n_freqs and n_out (_host.dense_fbank_fragments).  out is dense (rows, frames, n_out) of `dtype`.  float32 FMA
 * chains in ascending k on the matrix cores, one accumulator per output, rounded once to `dtype`: the result does not
 * depend on the layout, the alignment, the number of rows or the tiling of k.  n_out > AAMD_DENSE_FBANK_MAX_OUT or
 * n_freqs > AAMD_DENSE_FBANK_MAX_FREQS: AAMD_EUNSUPPORTED.  One launch. */
int aamd_dense_fbank(int32_t dtype, const void* x, const float* w, void* out, int64_t rows, int64_t frames,
                     int64_t stride_row, int64_t stride_freq, int64_t stride_frame, int32_t n_freqs, int32_t n_out,
                     void* stream);

/* ---- Batched edit distance (additions to ABI 7; csrc/edit_distance.h) ------------------------------------------------ */

#define AAMD_EDIT_DISTANCE_MAX_REF 4096  /* the widest reference axis: 256 lanes x 16 rows of one workgroup */
#define AAMD_EDIT_DISTANCE_MAX_HYP 32767 /* the widest hypothesis axis: the fields of a cell are 16 bits */

/* What the launcher picks for a reference axis of max_m tokens: consecutive rows per lane (4 or 16) and lanes per workgroup
 * (64 or 256); the two limits (the defines above). */
int32_t aamd_edit_distance_states_per_lane(int64_t max_m);
int32_t aamd_edit_distance_threads(int64_t max_m);
int32_t aamd_edit_distance_max_ref(void);
int32_t aamd_edit_distance_max_hyp(void);

/* F.edit_distance_batch.  hyps dense (pairs, max_n) and refs dense (pairs / pairs_per_ref, max_m), int32 or int64 each
 * (hyps_int64, refs_int64; compared as integers); pair p scores hypothesis p against reference p / pairs_per_ref.
 * hyp_lengths (pairs,) and ref_lengths (pairs / pairs_per_ref,), int32 or int64 each, or null for the full width.  All on
 * the device and read there: no synchronisation, no workspace.  out is int32 (pairs,): the Levenshtein distance; with
 * return_ops (pairs, 4): (distance, substitutions, deletions, insertions) of the alignment that takes, cell by cell, the
 * first of diagonal, deletion (a reference token without a partner), insertion whose cost is smallest.  A pair with a
 * hypothesis length outside [0, max_n] or a reference length outside [0, max_m] gets -1 in every field, and nothing is
 * indexed with those values.  max_m > AAMD_EDIT_DISTANCE_MAX_REF or max_n > AAMD_EDIT_DISTANCE_MAX_HYP:
 * AAMD_EUNSUPPORTED.  One launch, integers only. */
int aamd_edit_distance(const void* hyps, int32_t hyps_int64, const void* refs, int32_t refs_int64, const void* hyp_lengths,
                       int32_t hyp_lengths_int64, const void* ref_lengths, int32_t ref_lengths_int64, int64_t pairs,
                       int64_t pairs_per_ref, int64_t max_n, int64_t max_m, int32_t return_ops, int32_t* out, void* stream);

/* ---- STOI / ESTOI speech intelligibility (additions to ABI 7; csrc/stoi.h) ------------------------------------------- */

/* which: 0 threads per workgroup, 1 frames per workgroup of the energy kernel, 2 output frames per workgroup of the band
 * kernel, 3 segments per workgroup of the segment kernel, 4 threads per row of the finishing kernel. */
int32_t aamd_stoi_tiles(int32_t which);

/* Bytes of workspace for `rows` rows of `length` samples of `dtype` (AAMD_SA_*); 0 for no rows. */
int64_t aamd_stoi_workspace(int32_t dtype, int64_t rows, int64_t length);

/* F.stoi at 10 kHz.  preds (processed) and target (clean): (rows, length) of `dtype` (AAMD_SA_F32 / F64 / F16 / BF16), unit
 * sample stride, row strides in elements.  lengths: (rows,) int32 or int64 (lengths_int64) or null for the full width; row b
 * ends at lengths[b] and nothing at or beyond it is read; a length outside [0, length] scores NaN, as does a row with a
 * non-finite sample below its length.  extended: ESTOI.  workspace: aamd_stoi_workspace bytes, 8-byte aligned.  out: (rows,)
 * float32, or float64 for AAMD_SA_F64.  Rows with fewer than 30 output frames score 1e-5.  All on the device and read
 * there: five launches, no synchronisation, no atomics, no cached table. */
int aamd_stoi(int32_t dtype, const void* preds, const void* target, int64_t rows, int64_t length, int64_t preds_stride,
              int64_t target_stride, const void* lengths, int32_t lengths_int64, int32_t extended, void* workspace, void* out,
              void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AUDIO_AMD_H */
