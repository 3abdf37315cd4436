"""ctypes binding of libaudio_amd.so (the C ABI declared in include/audio_amd.h).

The shared library is built in-tree by ``python -m audio_amd._build`` (or
``__graft_entry__.build()``) with ``hipcc --offload-arch=gfx950``.  There is NO
fallback: if the library is missing or a call fails, a RuntimeError is raised.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libaudio_amd.so")
if os.environ.get("AAMD_USE_LAB_LIB"):
    # tools/ only: the library with the tools-only kernel instantiations and their environment switches
    # (python -m audio_amd._build --lab; see audio_amd/_build.py).  The product never sets this.
    LIB_PATH = os.path.join(_HERE, "lib", "libaudio_amd_lab.so")

AAMD_OK = 0
PAD_MODES = {"reflect": 0, "constant": 1, "replicate": 2, "circular": 3}


class StftDesc(C.Structure):
    _fields_ = [
        ("rows", C.c_int64), ("length", C.c_int64), ("row_stride", C.c_int64),
        ("n_fft", C.c_int32), ("hop", C.c_int32), ("pad", C.c_int32), ("center", C.c_int32),
        ("pad_mode", C.c_int32), ("onesided", C.c_int32), ("n_frames", C.c_int32),
        ("scale", C.c_float), ("power", C.c_float),
    ]


class MelBands(C.Structure):
    _fields_ = [
        ("n_mels", C.c_int32), ("max_width", C.c_int32),
        ("lo", C.c_void_p), ("width", C.c_void_p), ("weights", C.c_void_p), ("lane_order", C.c_void_p),
        ("table400", C.c_void_p), ("table_sig", C.c_int32),
    ]


class MfccFused(C.Structure):
    """aamd_mfcc_fused (include/audio_amd.h)."""
    _fields_ = [("dct_frag", C.c_void_p), ("n_mfcc", C.c_int32), ("pass_", C.c_int32), ("multiplier", C.c_float),
                ("amin", C.c_float), ("db_multiplier", C.c_float), ("top_db", C.c_float), ("group_max", C.c_void_p),
                ("rows_per_group", C.c_int64), ("tile_min", C.c_void_p), ("fix_count", C.c_void_p),
                ("tile_list", C.c_void_p)]


class ResampleBands(C.Structure):
    _fields_ = [("n_tiles", C.c_int32), ("tap_span", C.c_int32), ("tap_lo", C.POINTER(C.c_int32))]


_lib = None
_lock = threading.Lock()

_P = C.c_void_p
class VocoderDesc(C.Structure):
    """aamd_vocoder_desc (include/audio_amd.h)."""
    _fields_ = [("rows", C.c_int64), ("n_freq", C.c_int32), ("n_frames_in", C.c_int32), ("n_frames_out", C.c_int32),
                ("in_stride_row", C.c_int64), ("in_stride_freq", C.c_int64), ("in_stride_frame", C.c_int64),
                ("out_stride_row", C.c_int64), ("out_stride_freq", C.c_int64), ("out_stride_frame", C.c_int64),
                ("rate", C.c_double)]


class KaldiDesc(C.Structure):
    """aamd_kaldi_desc (include/audio_amd.h)."""
    _fields_ = [("n_samples", C.c_int64), ("n_frames", C.c_int64), ("n_fft", C.c_int32), ("shift", C.c_int32),
                ("win", C.c_int32), ("snip_edges", C.c_int32), ("preemphasis", C.c_float),
                ("remove_dc_offset", C.c_int32), ("raw_energy", C.c_int32), ("energy_floor", C.c_float),
                ("use_power", C.c_int32), ("use_log", C.c_int32), ("energy_col", C.c_int32), ("first_col", C.c_int32),
                ("n_cols", C.c_int32), ("dither", C.c_float), ("noise", C.c_void_p), ("n_utt", C.c_int64),
                ("utt_stride", C.c_int64)]


_SIGS = {
    "aamd_abi_version": (C.c_int, []),
    "aamd_last_error": (C.c_char_p, []),
    "aamd_set_kernel_policy": (C.c_int, [C.c_int]),
    "aamd_mel400_table_dwords": (C.c_int64, [C.c_int32, C.c_int32]),
    "aamd_mel400_table_build": (C.c_int, [C.POINTER(MelBands), _P, _P]),
    "aamd_device_info": (C.c_int, [C.c_char_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    "aamd_box_probe": (C.c_int, [_P, C.c_int32, C.c_int32, _P]),
    "aamd_spectrogram_f32": (C.c_int, [_P, _P, _P, _P, C.POINTER(StftDesc), _P]),
    "aamd_melspectrogram_f32": (C.c_int, [_P, _P, _P, C.POINTER(MelBands), _P, C.POINTER(StftDesc), _P]),
    "aamd_melspectrogram_db_f32": (C.c_int, [_P, _P, _P, C.POINTER(MelBands), _P, C.POINTER(StftDesc), C.c_float,
                                             C.c_float, C.c_float, _P, C.c_int64, _P]),
    "aamd_melspectrogram_lognorm_f32": (C.c_int, [_P, _P, _P, C.POINTER(MelBands), _P, C.POINTER(StftDesc), C.c_float,
                                                  _P, _P, C.c_int64, _P]),
    "aamd_melspectrogram_pcm16_f32": (C.c_int, [_P, _P, _P, C.POINTER(MelBands), _P, C.POINTER(StftDesc), C.c_float,
                                                _P, _P, C.c_int64, _P]),
    "aamd_melspectrogram_pcm16_interleaved_f32": (C.c_int, [_P, C.c_int32, _P, _P, C.POINTER(MelBands), _P,
                                                            C.POINTER(StftDesc), C.c_float, _P, _P, C.c_int64, _P]),
    "aamd_melspectrogram_lowp_f32": (C.c_int, [_P, C.c_int32, _P, _P, C.POINTER(MelBands), _P, C.POINTER(StftDesc), _P]),
    "aamd_spectrogram_grad_f32": (C.c_int, [_P, _P, _P, C.c_int64, C.c_float, _P]),
    "aamd_melspectrogram_grad_f32": (C.c_int, [_P, _P, C.POINTER(MelBands), C.c_int64, C.c_int32, C.c_int32, C.c_float, _P]),
    "aamd_kaldi_features_f32": (C.c_int, [_P, _P, _P, C.POINTER(MelBands), _P, C.POINTER(KaldiDesc), _P]),
    "aamd_istft_f32": (C.c_int, [_P, _P, _P, _P, _P, C.POINTER(StftDesc), C.c_int32, _P]),
    "aamd_phase_vocoder_f32": (C.c_int, [_P, _P, _P, C.POINTER(VocoderDesc), _P]),
    "aamd_griffinlim_update_f32": (C.c_int, [_P, _P, _P, _P, C.c_int64, C.c_float, _P]),
    "aamd_mel_scale_f32": (C.c_int, [_P, C.POINTER(MelBands), _P, C.c_int64, C.c_int32, C.c_int32, _P]),
    "aamd_amplitude_to_db_f32": (C.c_int, [_P, _P, C.c_int64, C.c_float, C.c_float, C.c_float, _P, C.c_int64, _P]),
    "aamd_amplitude_to_db_clamped_f32": (C.c_int, [_P, _P, C.c_int64, C.c_float, C.c_float, C.c_float, _P, C.c_int64,
                                                   C.c_float, _P]),
    "aamd_db_clamp_f32": (C.c_int, [_P, _P, C.c_int64, _P, C.c_int64, C.c_float, _P]),
    "aamd_mfcc_dct_f32": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int64,
                                    C.c_float, _P]),
    "aamd_mfcc_frag_floats": (C.c_int32, []),
    "aamd_mfcc_fused_tiles": (C.c_int64, [C.POINTER(StftDesc)]),
    "aamd_mfcc_fused_supported": (C.c_int, [C.POINTER(StftDesc), C.POINTER(MelBands), C.c_int32]),
    "aamd_mfcc_frag_build": (C.c_int, [_P, C.c_int32, C.c_int32, _P, _P]),
    "aamd_mfcc_fused_f32": (C.c_int, [_P, _P, _P, C.POINTER(MelBands), _P, C.POINTER(StftDesc), C.POINTER(MfccFused), _P]),
    "aamd_resample_f32": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_int32,
                                    C.c_int32, C.c_int64, _P]),
    "aamd_resample_banded_f32": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_int32,
                                           C.c_int32, C.c_int64, C.POINTER(ResampleBands), _P]),
    "aamd_resample_frag_bytes": (C.c_int64, [C.c_int32, C.c_int32, C.POINTER(ResampleBands)]),
    "aamd_resample_frag_build_f32": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, C.POINTER(ResampleBands), _P, _P]),
    "aamd_resample_prepared_f32": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_int32,
                                             C.c_int32, C.c_int64, C.POINTER(ResampleBands), _P, _P]),
    "aamd_resample_sparse_f32": (C.c_int, [_P, _P, _P, _P, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int32,
                                           C.c_int32, C.c_int64, _P]),
    "aamd_lfilter_f32": (C.c_int, [_P, _P, _P, _P, C.c_int64, C.c_int32, C.c_int64, C.c_int32, C.c_int32,
                                   C.c_int32, C.c_int32, _P]),
    "aamd_lfilter_plan": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_int32)]),
    "aamd_spectrogram_f64": (C.c_int, [_P, _P, _P, _P, C.POINTER(StftDesc), _P]),
    "aamd_istft_f64": (C.c_int, [_P, _P, _P, _P, _P, C.POINTER(StftDesc), C.c_int32, _P]),
    "aamd_lfilter_f64": (C.c_int, [_P, _P, _P, _P, C.c_int64, C.c_int32, C.c_int64, C.c_int32, C.c_int32,
                                   C.c_int32, C.c_int32, _P]),
    "aamd_resample_f64": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_int32,
                                    C.c_int32, C.c_int64, _P]),
    "aamd_fftconvolve_f64": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, _P, _P,
                                       C.c_int64, C.c_int64, _P]),
    "aamd_fftconvolve_workspace": (C.c_int64, [C.c_int64] * 5),
    "aamd_fftconvolve_plan": (C.c_int, [C.c_int64] * 4),
    "aamd_fftconvolve_f32": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, _P, _P,
                                       C.c_int64, C.c_int64, _P, _P]),
    "aamd_fftconvolve_staged_f32": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, _P, _P,
                                              C.c_int64, C.c_int64, _P, C.c_int32, _P]),
    # feature post-processing (additions to ABI 7)
    "aamd_compute_deltas_f32": (C.c_int, [_P, _P] + [C.c_int64] * 6 + [C.c_int32] * 3 + [_P]),
    "aamd_compute_deltas_f64": (C.c_int, [_P, _P] + [C.c_int64] * 6 + [C.c_int32] * 3 + [_P]),
    "aamd_sliding_window_cmn_workspace": (C.c_int64, [C.c_int64] * 3 + [C.c_int32]),
    "aamd_sliding_window_cmn_f32": (C.c_int, [_P, _P, _P] + [C.c_int64] * 8 + [C.c_int32] * 3 + [_P]),
    "aamd_sliding_window_cmn_f64": (C.c_int, [_P, _P, _P] + [C.c_int64] * 8 + [C.c_int32] * 3 + [_P]),
    "aamd_detect_pitch_workspace": (C.c_int64, [C.c_int64, C.c_int64, C.c_int32]),
    "aamd_detect_pitch_f32": (C.c_int, [_P, _P, _P] + [C.c_int64] * 3 + [C.c_int32] * 6 + [_P]),
    "aamd_detect_pitch_f64": (C.c_int, [_P, _P, _P] + [C.c_int64] * 3 + [C.c_int32] * 6 + [_P]),
    # SpecAugment masking (additions to ABI 7)
    "aamd_spec_augment_iid": (C.c_int, [_P, _P] + [C.c_int64] * 6 + [C.c_int32] * 3 + [_P, _P, _P, C.c_uint64, _P, _P]),
    "aamd_spec_augment_shared": (C.c_int, [_P, _P] + [C.c_int64] * 6 + [C.c_int32] * 3 + [_P, _P, _P, C.c_uint64, _P, _P]),
    # waveform augmentation (additions to ABI 7)
    "aamd_add_noise_workspace": (C.c_int64, [C.c_int64] * 2),
    "aamd_add_noise_f32": (C.c_int, [_P] * 6 + [C.c_int64] * 5 + [_P, C.c_int64, _P, C.c_int64, C.c_int32, _P]),
    "aamd_add_noise_f64": (C.c_int, [_P] * 6 + [C.c_int64] * 5 + [_P, C.c_int64, _P, C.c_int64, C.c_int32, _P]),
    "aamd_add_noise_lp": (C.c_int, [_P] * 6 + [C.c_int64] * 5 + [_P, C.c_int64, _P, C.c_int64, C.c_int32, C.c_int32, _P]),
    "aamd_preemphasis_f32": (C.c_int, [_P, _P] + [C.c_int64] * 3 + [C.c_double, C.c_int32, _P]),
    "aamd_preemphasis_f64": (C.c_int, [_P, _P] + [C.c_int64] * 3 + [C.c_double, C.c_int32, _P]),
    "aamd_preemphasis_lp": (C.c_int, [_P, _P] + [C.c_int64] * 3 + [C.c_double, C.c_int32, C.c_int32, _P]),
    # MVDR beamforming (additions to ABI 7)
    "aamd_beamform_freq_tile": (C.c_int32, []),
    "aamd_beamform_time_chunk": (C.c_int32, []),
    "aamd_beamform_psd": (C.c_int, [C.c_int32, _P] + [C.c_int64] * 8 + [_P, _P, _P, _P, C.c_int32, C.c_double, _P, _P]),
    "aamd_beamform_weights": (C.c_int, [C.c_int32, C.c_int32, _P, _P, _P, _P, C.c_int64, C.c_int64] + [C.c_int32] * 4 +
                              [C.c_double, C.c_double, C.c_int32, C.c_int32, _P]),
    "aamd_beamform_apply": (C.c_int, [C.c_int32, _P, _P] + [C.c_int64] * 8 + [_P, _P, _P]),
    # RNN transducer loss (additions to ABI 7)
    "aamd_rnnt_team_width": (C.c_int32, [C.c_int32, C.c_int64]),
    "aamd_rnnt_lattice_threads": (C.c_int32, []),
    "aamd_rnnt_loss_workspace": (C.c_int64, [C.c_int64] * 3),
    "aamd_rnnt_loss_forward": (C.c_int, [C.c_int32, _P, _P, _P, _P] + [C.c_int64] * 4 + [C.c_int32, C.c_int32, _P, _P, _P]),
    "aamd_rnnt_loss_backward": (C.c_int, [C.c_int32, _P, _P, _P, _P] + [C.c_int64] * 4 + [C.c_int32, C.c_int32, C.c_double,
                                          _P, _P, _P, _P]),
    # CTC forced alignment (additions to ABI 7)
    "aamd_forced_align_states_per_lane": (C.c_int32, [C.c_int64]),
    "aamd_forced_align_threads": (C.c_int32, [C.c_int64]),
    "aamd_forced_align_prefetch": (C.c_int32, []),
    "aamd_forced_align_backtrack_block": (C.c_int32, []),
    "aamd_forced_align_workspace": (C.c_int64, [C.c_int64] * 3),
    "aamd_forced_align": (C.c_int, [C.c_int32, _P, _P, C.c_int32, _P, _P, C.c_int32] + [C.c_int64] * 4 + [C.c_int32, _P, _P, _P,
                                    _P]),
    # CTC prefix beam search (additions to ABI 7)
    "aamd_ctc_decoder_max_beam": (C.c_int32, []),
    "aamd_ctc_decoder_row_threads": (C.c_int32, []),
    "aamd_ctc_decoder_beam_threads": (C.c_int32, []),
    "aamd_ctc_decoder_record_slots": (C.c_int32, [C.c_int32]),
    "aamd_ctc_decoder_candidates": (C.c_int32, [C.c_int32]),
    "aamd_ctc_decoder_max_frames": (C.c_int64, []),
    "aamd_ctc_decoder_max_nodes": (C.c_int64, []),
    "aamd_ctc_decoder_workspace": (C.c_int64, [C.c_int64] * 4),
    "aamd_ctc_beam_search": (C.c_int, [C.c_int32, _P, _P, C.c_int32] + [C.c_int64] * 3 + [C.c_int32] * 3 + [C.c_double] +
                             [_P] * 5),
    # SoX-style effects (additions to ABI 7)
    "aamd_effects_tiles": (C.c_int32, [C.c_int32]),
    "aamd_effects_workspace": (C.c_int64, [C.c_int32, C.c_int32] + [C.c_int64] * 3),
    "aamd_overdrive": (C.c_int, [C.c_int32, _P, _P, _P] + [C.c_int64] * 3 + [C.c_double, C.c_double, _P]),
    "aamd_phaser": (C.c_int, [C.c_int32, _P, _P, _P] + [C.c_int64] * 3 + [_P, C.c_int64, C.c_int64] + [C.c_double] * 3 + [_P]),
    "aamd_flanger": (C.c_int, [C.c_int32, _P, _P, _P] + [C.c_int64] * 3 + [C.c_int32, _P, C.c_int64, C.POINTER(C.c_int64),
                               C.c_int64] + [C.c_double] * 3 + [C.c_int32, C.c_int32, _P]),
    # InverseMelScale (additions to ABI 7)
    "aamd_inverse_mel_tiles": (C.c_int32, [C.c_int32]),
    "aamd_inverse_mel": (C.c_int, [C.c_int32, _P, _P, _P] + [C.c_int64] * 5 + [C.c_int32] * 3 + [_P]),
    # voice-activity trimming (additions to ABI 7)
    "aamd_vad_tiles": (C.c_int32, [C.c_int32]),
    "aamd_vad_workspace": (C.c_int64, [C.c_int64] * 3),
    "aamd_vad_measure": (C.c_int, [C.c_int32, _P] + [C.c_int64] * 3 + [C.c_int32] * 8 + [C.c_double] * 4 + [_P, _P, _P, C.c_int64,
                                   _P]),
    "aamd_vad_trigger": (C.c_int, [_P] + [C.c_int64] * 6 + [C.c_double] * 2 + [_P] * 4),
    # spectral centroid (additions to ABI 7)
    "aamd_spectral_tiles": (C.c_int32, [C.c_int32]),
    "aamd_spectral_lanes": (C.c_int32, [C.c_int64]),
    "aamd_spectral_centroid": (C.c_int, [C.c_int32, _P, _P, _P] + [C.c_int64] * 6 + [_P]),
    # pointwise waveform ops (additions to ABI 7)
    "aamd_pointwise_tiles": (C.c_int32, [C.c_int32]),
    "aamd_pointwise": (C.c_int, [C.c_int32, C.c_int32, _P, _P] + [C.c_int64] * 3 + [C.c_double, C.c_double, C.c_int32, _P,
                                 C.c_int64, C.c_int64, _P]),
    # image-source room impulse responses (additions to ABI 7)
    "aamd_rir_tiles": (C.c_int32, [C.c_int32]),
    "aamd_simulate_rir": (C.c_int, [C.c_int32] + [_P] * 5 + [C.c_int64, _P, C.c_int64, C.c_int64] + [C.c_int32] * 3 +
                          [C.c_int64, C.c_double, C.c_double, _P]),
    # ray-traced energy histograms (additions to ABI 7)
    "aamd_ray_tiles": (C.c_int32, [C.c_int32]),
    "aamd_ray_trace": (C.c_int, [C.c_int32] + [_P] * 7 + [C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int64, C.c_int64,
                                 C.c_int32] + [C.c_double] * 5 + [_P]),
    # synthesis ops (additions to ABI 7)
    "aamd_dsp_tiles": (C.c_int32, [C.c_int32]),
    "aamd_oscillator_workspace": (C.c_int64, [C.c_int64] * 3),
    "aamd_oscillator_bank": (C.c_int, [C.c_int32] + [_P] * 4 + [C.c_int64] * 5 + [C.c_double, C.c_int32, _P]),
    "aamd_filter_waveform": (C.c_int, [C.c_int32] + [_P] * 3 + [C.c_int64] * 4 + [C.c_int32, C.c_int32, _P]),
    "aamd_dsp_grad_tiles": (C.c_int32, [C.c_int32]),
    "aamd_oscillator_grad_workspace": (C.c_int64, [C.c_int64] * 3),
    "aamd_oscillator_bank_grad": (C.c_int, [C.c_int32] + [_P] * 6 + [C.c_int64] * 5 + [C.c_double, C.c_int32, _P]),
    "aamd_filter_waveform_grad_workspace": (C.c_int64, [C.c_int64] * 3 + [C.c_int32, C.c_int32]),
    "aamd_filter_waveform_grad": (C.c_int, [C.c_int32] + [_P] * 6 + [C.c_int64] * 4 + [C.c_int32, C.c_int32, _P]),
    "aamd_sinc_impulse_response": (C.c_int, [C.c_int32, _P, _P, C.c_int64, C.c_int32, C.c_int32, _P]),
    "aamd_frequency_impulse_response": (C.c_int, [C.c_int32, _P, _P, _P, C.c_int64, C.c_int32, _P]),
    "aamd_extend_pitch": (C.c_int, [C.c_int32, _P, _P, _P, C.c_int64, C.c_int64, _P]),
    # dense filterbank projection (additions to ABI 7)
    "aamd_dense_fbank_tiles": (C.c_int32, [C.c_int32]),
    "aamd_dense_fbank": (C.c_int, [C.c_int32, _P, _P, _P] + [C.c_int64] * 5 + [C.c_int32] * 2 + [_P]),
    # batched edit distance (additions to ABI 7)
    "aamd_edit_distance_states_per_lane": (C.c_int32, [C.c_int64]),
    "aamd_edit_distance_threads": (C.c_int32, [C.c_int64]),
    "aamd_edit_distance_max_ref": (C.c_int32, []),
    "aamd_edit_distance_max_hyp": (C.c_int32, []),
    "aamd_edit_distance": (C.c_int, [_P, C.c_int32] * 4 + [C.c_int64] * 4 + [C.c_int32, _P, _P]),
    # STOI / ESTOI (additions to ABI 7)
    "aamd_stoi_tiles": (C.c_int32, [C.c_int32]),
    "aamd_stoi_workspace": (C.c_int64, [C.c_int32, C.c_int64, C.c_int64]),
    "aamd_stoi": (C.c_int, [C.c_int32, _P, _P] + [C.c_int64] * 4 + [_P, C.c_int32, C.c_int32, _P, _P, _P]),
}

EXPORTED_SYMBOLS = tuple(_SIGS)


def lib():
    """Load (once) and return the ctypes handle; raise loudly if the HIP library is absent."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise RuntimeError(
                    f"audio_amd: {LIB_PATH} not found. Build the HIP extension first "
                    "(python -m audio_amd._build). There is no CPU fallback.")
            h = C.CDLL(LIB_PATH)
            for name, (res, args) in _SIGS.items():
                fn = getattr(h, name)   # AttributeError if the ABI symbol is missing
                fn.restype = res
                fn.argtypes = args
            if h.aamd_abi_version() != 7:
                raise RuntimeError("audio_amd: ABI version mismatch between _lib.py and libaudio_amd.so")
            _lib = h
    return _lib


POLICY_FORCE_GENERIC, POLICY_MEL400_WIDE, POLICY_ISTFT_ATOMIC, POLICY_RESAMPLE_FP32 = 1, 2, 4, 8
POLICY_FFTCONV_NO_FDL, POLICY_FFTCONV_FDL, POLICY_FFTCONV_COMPLEX = 16, 32, 64
POLICY_RESAMPLE_B32, POLICY_MEL400_NO_POOL, POLICY_MEL400_SCALAR = 128, 256, 512


class kernel_policy:
    """``with _lib.kernel_policy(_lib.POLICY_FORCE_GENERIC): ...`` -- tests / A-B runs pick the kernel family."""

    def __init__(self, flags: int):
        self.flags = flags

    def __enter__(self):
        self.prev = lib().aamd_set_kernel_policy(self.flags)
        return self

    def __exit__(self, *exc):
        lib().aamd_set_kernel_policy(self.prev)
        return False


EUNSUPPORTED = -2          # AAMD_EUNSUPPORTED: valid request this build cannot serve


def check(rc: int) -> None:
    if rc != AAMD_OK:
        msg = lib().aamd_last_error()
        raise RuntimeError((msg or b"audio_amd: unknown error").decode())


def ptr(t) -> int:
    """Device pointer of a torch tensor (0-size tensors give a dummy non-null pointer)."""
    return t.data_ptr() if t.numel() else 0


def current_stream(device) -> int:
    import torch
    return torch.cuda.current_stream(device).cuda_stream
