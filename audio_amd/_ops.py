"""``torch.ops.audio_amd.*`` -- the hot path registered as PyTorch custom ops.

The reference reaches native code through operator registration: ``torch.ops.load_library`` runs
``STABLE_TORCH_LIBRARY_FRAGMENT(torchaudio, m){ m.def(schema) }`` / ``..._IMPL(torchaudio, CUDA, m)``
(src/libtorchaudio/lfilter.cpp:118-138, src/torchaudio/_extension/utils.py:50-56).  This module is the
same mechanism from the Python side (``torch.library``): schemas in a new namespace, implementations
under the CUDA dispatch key (ROCm tensors dispatch there) that call libaudio_amd.so's C ABI, and
Meta ("fake") implementations so the ops trace / export.  There is deliberately NO CPU-key
implementation: a CPU tensor fails in the dispatcher ("no kernel for CPU"), loudly.

Each op is declared once, by one ``_register(schema, kernel, meta)`` call below its kernel and Meta function; ``OPS`` records the
triples (tests/test_ops_registration.py checks them against the dispatcher and against each other's arity).

Schemas follow SURVEY.md 8(b).  ``norm_mode``: 0 none, 1 "frame_length", 2 "window".
"""
from __future__ import annotations

import math

import torch
from torch import Tensor

from . import _host
from . import functional as F

_NORM = {0: False, 1: "frame_length", 2: "window"}

_DEF = torch.library.Library("audio_amd", "DEF")
_CUDA = torch.library.Library("audio_amd", "IMPL", "CUDA")
_META = torch.library.Library("audio_amd", "IMPL", "Meta")
_AUTOGRAD = torch.library.Library("audio_amd", "IMPL", "AutogradCUDA")

OPS = {}                                   # name -> (schema, CUDA-key kernel, Meta kernel)


def _plain_tensor_wants_grad(a) -> bool:
    # (`type(a) is Tensor`: fake / functional tensors of a tracer never take the Python implementation -- they go on to the
    # Meta kernel exactly as before the autograd route existed)
    return type(a) is Tensor and a.requires_grad


def _register(schema: str, fn, meta) -> None:
    """One op: its schema, its CUDA-key kernel (= the eager implementation) and its Meta kernel (shapes / strides only).
    The AutogradCUDA kernel makes a SCRIPTED call differentiable the way the eager call is (the reference's scripted modules
    are: they are aten compositions): when autograd is recording and an argument asks for a gradient the implementation runs
    right there, at the autograd level, and its own autograd Functions (F._SpectrogramFunction, _LFilterFunction, ...) record
    the graph; every other call goes below autograd to the CUDA / Meta kernel."""
    name = schema[:schema.index("(")]
    _DEF.define(schema)
    _CUDA.impl(name, fn)
    op = getattr(torch.ops.audio_amd, name).default

    def at_autograd_level(*args):
        if torch.is_grad_enabled() and any(_plain_tensor_wants_grad(a) for a in args):
            return fn(*args)
        with torch._C._AutoDispatchBelowAutograd():
            return op(*args)

    _AUTOGRAD.impl(name, at_autograd_level)
    _META.impl(name, meta)
    OPS[name] = (schema, fn, meta)


# ---- Meta helpers shared by several ops ------------------------------------------------------

def _stft_frames(length, pad, n_fft, hop, center):
    return _host.frame_count(length, n_fft, hop, center, pad)


def _frame_major_view(waveform, n_out, T, dtype=None):
    lead = tuple(waveform.shape[:-1])
    rows = 1
    for d in lead:
        rows *= d
    out = waveform.new_empty((rows, T, n_out), dtype=dtype or waveform.dtype)
    return out.view(lead + (T, n_out)).transpose(-1, -2)


_same_as_waveform = lambda waveform, *rest: torch.empty_like(waveform)        # noqa: E731
_dense_like = lambda x, *rest: torch.empty_like(x, memory_format=torch.contiguous_format)        # noqa: E731


# ---- the spectrogram family ------------------------------------------------------------------

def _spectrogram(waveform, window, pad, n_fft, hop_length, win_length, power, norm_mode, center, pad_mode, onesided):
    return F.spectrogram(waveform, pad, window, n_fft, hop_length, win_length, power, _NORM[norm_mode], center,
                         pad_mode, onesided)


def _spectrogram_meta(waveform, window, pad, n_fft, hop_length, win_length, power, norm_mode, center, pad_mode, onesided):
    T = _stft_frames(waveform.shape[-1], pad, n_fft, hop_length, center)
    n_freq = n_fft // 2 + 1 if onesided else n_fft
    return _frame_major_view(waveform, n_freq, T, torch.complex64 if power is None else None)


_register("spectrogram(Tensor waveform, Tensor window, int pad, int n_fft, int hop_length, int win_length, "
          "float? power, int norm_mode, bool center, str pad_mode, bool onesided) -> Tensor", _spectrogram, _spectrogram_meta)


def _mel_spectrogram_module(waveform, window, fb, pad, n_fft, hop_length, win_length, power, norm_mode, center, pad_mode):
    return F._melspectrogram_module(waveform, window, fb, pad, n_fft, hop_length, win_length, power, _NORM[norm_mode], center,
                                    pad_mode)


def _mel_meta(waveform, window, fb, pad, n_fft, hop_length, win_length, power, norm_mode, center, pad_mode):
    return _frame_major_view(waveform, fb.shape[1], _stft_frames(waveform.shape[-1], pad, n_fft, hop_length, center))


_register("mel_spectrogram(Tensor waveform, Tensor window, Tensor fb, int pad, int n_fft, int hop_length, "
          "int win_length, float power, int norm_mode, bool center, str pad_mode) -> Tensor", _mel_spectrogram_module, _mel_meta)


def _mfcc(waveform, window, fb, dct_mat, pad, n_fft, hop_length, win_length, power, norm_mode, center, pad_mode,
          log_mels, top_db):
    return F._mfcc(waveform, pad, window, fb, dct_mat, n_fft, hop_length, win_length, power, _NORM[norm_mode], center,
                   pad_mode, log_mels, top_db)


def _mfcc_meta(waveform, window, fb, dct_mat, pad, n_fft, hop_length, win_length, power, norm_mode, center, pad_mode,
               *rest):
    # (serves mfcc and mfcc_module: the arguments after pad_mode do not change the shape)
    return _frame_major_view(waveform, dct_mat.shape[1], _stft_frames(waveform.shape[-1], pad, n_fft, hop_length, center))


_register("mfcc(Tensor waveform, Tensor window, Tensor fb, Tensor dct_mat, int pad, int n_fft, int hop_length, "
          "int win_length, float power, int norm_mode, bool center, str pad_mode, bool log_mels, float top_db) -> Tensor",
          _mfcc, _mfcc_meta)


def _inverse_spectrogram(spectrogram, length, window, pad, n_fft, hop_length, win_length, norm_mode, center, pad_mode,
                         onesided):
    return F.inverse_spectrogram(spectrogram, length, pad, window, n_fft, hop_length, win_length, _NORM[norm_mode],
                                 center, pad_mode, onesided)


def _inverse_spectrogram_meta(spectrogram, length, window, pad, n_fft, hop_length, win_length, norm_mode, center, pad_mode,
                              onesided):
    T = spectrogram.shape[-1]
    n = length if length is not None else n_fft + hop_length * (T - 1) - (2 * (n_fft // 2) if center else 0)
    return spectrogram.new_empty(tuple(spectrogram.shape[:-2]) + (n,), dtype=torch.float32)


_register("inverse_spectrogram(Tensor spectrogram, int? length, Tensor window, int pad, int n_fft, int hop_length, "
          "int win_length, int norm_mode, bool center, str pad_mode, bool onesided) -> Tensor",
          _inverse_spectrogram, _inverse_spectrogram_meta)
_register("amplitude_to_DB(Tensor x, float multiplier, float amin, float db_multiplier, float? top_db) -> Tensor",
          F.amplitude_to_DB, _same_as_waveform)


# ---- resampling, filtering, convolution ------------------------------------------------------

def _resample_apply(waveform, kernel, orig_freq, new_freq, gcd, width):
    # (the schema puts the tap table second; until round 6 the function itself was registered and received the arguments in the
    # wrong order -- found by the first scripted Resample that ran on a device, tests/test_torchscript.py)
    return F._apply_sinc_resample_kernel(waveform, orig_freq, new_freq, gcd, kernel, width)


def _resample_meta(waveform, kernel, orig_freq, new_freq, gcd, width):
    orig, new = int(orig_freq) // gcd, int(new_freq) // gcd
    return waveform.new_empty(tuple(waveform.shape[:-1]) + (int(math.ceil(new * waveform.shape[-1] / orig)),))


def _lfilter_meta(waveform, a_coeffs, b_coeffs, clamp, batching):
    if a_coeffs.ndim > 1 and not batching:
        return waveform.new_empty(tuple(waveform.shape[:-1]) + (a_coeffs.shape[0], waveform.shape[-1]))
    return torch.empty_like(waveform)


def _fftconvolve_meta(x, y, mode):
    F._check_shape_compatible(x, y)
    F._check_convolve_mode(mode)
    nx, ny = x.shape[-1], y.shape[-1]
    n = {"full": nx + ny - 1, "same": nx, "valid": max(nx, ny) - min(nx, ny) + 1}[mode]
    lead = tuple(max(a, b) for a, b in zip(x.shape[:-1], y.shape[:-1]))
    return x.new_empty(lead + (n,))


_register("resample_apply(Tensor waveform, Tensor kernel, int orig_freq, int new_freq, int gcd, int width) -> Tensor",
          _resample_apply, _resample_meta)
_register("lfilter(Tensor waveform, Tensor a_coeffs, Tensor b_coeffs, bool clamp, bool batching) -> Tensor",
          F.lfilter, _lfilter_meta)
_register("lfilter_cascade(Tensor waveform, Tensor a_coeffs, Tensor b_coeffs, bool clamp) -> Tensor",
          F.biquad_cascade, _same_as_waveform)
_register("fftconvolve(Tensor x, Tensor y, str mode) -> Tensor", F.fftconvolve, _fftconvolve_meta)


# ---- phase vocoder, Griffin-Lim --------------------------------------------------------------

def _phase_vocoder_meta(complex_specgrams, rate, phase_advance):
    if rate == 1.0:
        return complex_specgrams
    T = int(math.ceil(complex_specgrams.shape[-1] / rate))
    return complex_specgrams.new_empty(tuple(complex_specgrams.shape[:-1]) + (T,), dtype=torch.complex64)


def _griffinlim_meta(specgram, window, n_fft, hop_length, win_length, power, n_iter, momentum, length, rand_init):
    n = length if length is not None else hop_length * (specgram.shape[-1] - 1)
    return specgram.new_empty(tuple(specgram.shape[:-2]) + (n,), dtype=torch.float32)


_register("phase_vocoder(Tensor complex_specgrams, float rate, Tensor phase_advance) -> Tensor",
          F.phase_vocoder, _phase_vocoder_meta)
_register("griffinlim(Tensor specgram, Tensor window, int n_fft, int hop_length, int win_length, float power, int n_iter, "
          "float momentum, int? length, bool rand_init) -> Tensor", F.griffinlim, _griffinlim_meta)


# ---- round 6: the rest of the public surface, so that every scripted front of functional.py / transforms.py is one operator

def _mel_scale_meta(specgram, fb):
    lead, T = tuple(specgram.shape[:-2]), specgram.shape[-1]
    return specgram.new_empty(lead + (T, fb.shape[1])).transpose(-1, -2)


def _resample_full_meta(waveform, orig_freq, new_freq, lowpass_filter_width, rolloff, resampling_method, beta):
    if orig_freq == new_freq:
        return waveform
    g = math.gcd(int(orig_freq), int(new_freq))
    return _resample_meta(waveform, None, orig_freq, new_freq, g, 0)


def _mfcc_module(waveform, window, fb, dct_mat, pad, n_fft, hop_length, win_length, power, norm_mode, center, pad_mode,
                 log_mels, top_db, multiplier, amin, db_multiplier, fused, state):
    return F._mfcc_module(waveform, window, fb, dct_mat, pad, n_fft, hop_length, win_length, power, _NORM[norm_mode], center,
                          pad_mode, log_mels, top_db, (multiplier, amin, db_multiplier), fused,
                          F._mfcc_state_of(state) if fused else None)


_register("mel_scale(Tensor specgram, Tensor fb) -> Tensor", F.mel_scale, _mel_scale_meta)
_register("resample(Tensor waveform, int orig_freq, int new_freq, int lowpass_filter_width, float rolloff, "
          "str resampling_method, float? beta) -> Tensor", F.resample, _resample_full_meta)
_register("pitch_shift(Tensor waveform, int sample_rate, int n_steps, int bins_per_octave, int n_fft, int? win_length, "
          "int? hop_length, Tensor? window) -> Tensor", F.pitch_shift, _same_as_waveform)
_register("biquad(Tensor waveform, float b0, float b1, float b2, float a0, float a1, float a2) -> Tensor",
          F.biquad, _same_as_waveform)
_register("filtfilt(Tensor waveform, Tensor a_coeffs, Tensor b_coeffs, bool clamp) -> Tensor", F.filtfilt, _same_as_waveform)
_register("designed_biquad(Tensor waveform, str kind, int sample_rate, float[] params, bool flag) -> Tensor",
          F._designed_biquad, _same_as_waveform)
_register("mfcc_module(Tensor waveform, Tensor window, Tensor fb, Tensor dct_mat, int pad, int n_fft, int hop_length, "
          "int win_length, float power, int norm_mode, bool center, str pad_mode, bool log_mels, float top_db, "
          "float multiplier, float amin, float db_multiplier, int fused, int state) -> Tensor", _mfcc_module, _mfcc_meta)


# ---- feature post-processing, pitch ----------------------------------------------------------

def _sliding_window_cmn_meta(specgram, cmn_window, min_cmn_window, center, norm_vars):
    out = torch.empty_like(specgram, memory_format=torch.contiguous_format)
    return out.squeeze(0) if specgram.dim() == 2 else out


def _detect_pitch_frequency_meta(waveform, sample_rate, frame_time, win_length, freq_low, freq_high):
    if waveform.dim() == 0:
        raise ValueError("audio_amd: detect_pitch_frequency expects a (..., time) waveform, got a 0-d tensor")
    n_out = F._pitch_plan(waveform.shape[-1], sample_rate, frame_time, win_length, freq_low, freq_high)[4]
    return waveform.new_empty(tuple(waveform.shape[:-1]) + (n_out,), dtype=torch.float32)


_register("compute_deltas(Tensor specgram, int win_length, str mode) -> Tensor", F.compute_deltas, _dense_like)
_register("sliding_window_cmn(Tensor specgram, int cmn_window, int min_cmn_window, bool center, bool norm_vars) -> Tensor",
          F.sliding_window_cmn, _sliding_window_cmn_meta)
_register("detect_pitch_frequency(Tensor waveform, int sample_rate, float frame_time, int win_length, int freq_low, "
          "int freq_high) -> Tensor", F.detect_pitch_frequency, _detect_pitch_frequency_meta)


# ---- SpecAugment masking ---------------------------------------------------------------------

def _masking_meta(specgram, *rest):
    # a dense input keeps its strides in either order of the last two axes (masked_fill does); others come back contiguous
    if specgram.dim() >= 2 and not specgram.is_contiguous() and specgram.transpose(-1, -2).is_contiguous():
        return torch.empty_like(specgram.transpose(-1, -2), memory_format=torch.contiguous_format).transpose(-1, -2)
    return torch.empty_like(specgram, memory_format=torch.contiguous_format)


_register("mask_along_axis(Tensor specgram, int mask_param, float mask_value, int axis, float p) -> Tensor",
          F._mask_along_axis_eager, _masking_meta)
_register("mask_along_axis_iid(Tensor specgrams, int mask_param, float mask_value, int axis, float p) -> Tensor",
          F._mask_along_axis_iid_eager, _masking_meta)
_register("spec_augment(Tensor specgram, int n_time_masks, int time_mask_param, int n_freq_masks, int freq_mask_param, "
          "bool iid_masks, float p, bool zero_masking) -> Tensor", F._spec_augment_eager, _masking_meta)


# ---- waveform augmentation -------------------------------------------------------------------

def _add_noise_meta(waveform, noise, snr, lengths):
    lead = torch.broadcast_shapes(tuple(waveform.shape[:-1]), tuple(noise.shape[:-1]), tuple(snr.shape),
                                  tuple(lengths.shape) if lengths is not None else ())
    return waveform.new_empty(tuple(lead) + (waveform.shape[-1],))


_register("add_noise(Tensor waveform, Tensor noise, Tensor snr, Tensor? lengths) -> Tensor", F._add_noise_eager, _add_noise_meta)
_register("preemphasis(Tensor waveform, float coeff) -> Tensor", F._preemphasis_eager, _dense_like)
_register("deemphasis(Tensor waveform, float coeff) -> Tensor", F._deemphasis_eager, _dense_like)
_register("convolve(Tensor x, Tensor y, str mode) -> Tensor", F._convolve_eager, _fftconvolve_meta)


# ---- MVDR beamforming ------------------------------------------------------------------------

def _ref_of(reference_channel, reference_vector):
    return reference_vector if reference_vector is not None else reference_channel


def _psd_meta(specgram, mask, normalize, eps):
    c, f = specgram.shape[-3], specgram.shape[-2]
    return specgram.new_empty(tuple(specgram.shape[:-3]) + (f, c, c))


def _psd_pair_meta(specgram, mask_s, mask_n, normalize, eps):
    c, f = specgram.shape[-3], specgram.shape[-2]
    return specgram.new_empty((2,) + tuple(specgram.shape[:-3]) + (f, c, c))


def _apply_beamforming_meta(beamform_weights, specgram):
    """(..., freq, time) in the input's (freq, time) stride order: frame-major in, frame-major out."""
    lead, f, t = tuple(specgram.shape[:-3]), specgram.shape[-2], specgram.shape[-1]
    if t > 1 and specgram.stride(-1) != 1 and (f <= 1 or specgram.stride(-2) == 1):
        return specgram.new_empty(lead + (t, f)).transpose(-1, -2)
    return specgram.new_empty(lead + (f, t))


_register("psd(Tensor specgram, Tensor? mask, bool normalize, float eps) -> Tensor", F._psd_eager, _psd_meta)
_register("psd_pair(Tensor specgram, Tensor mask_s, Tensor mask_n, bool normalize, float eps) -> Tensor",
          F._psd_pair_eager, _psd_pair_meta)
_register("mvdr_weights_souden(Tensor psd_s, Tensor psd_n, int reference_channel, Tensor? reference_vector, "
          "bool diagonal_loading, float diag_eps, float eps) -> Tensor",
          lambda psd_s, psd_n, ref, vec, loading, diag_eps, eps:
          F._mvdr_weights_souden_eager(psd_s, psd_n, _ref_of(ref, vec), loading, diag_eps, eps),
          lambda psd_s, psd_n, *rest: psd_n.new_empty(tuple(psd_n.shape[:-1])))
_register("mvdr_weights_rtf(Tensor rtf, Tensor psd_n, int? reference_channel, Tensor? reference_vector, "
          "bool diagonal_loading, float diag_eps, float eps) -> Tensor",
          lambda rtf, psd_n, ref, vec, loading, diag_eps, eps:
          F._mvdr_weights_rtf_eager(rtf, psd_n, _ref_of(ref, vec), loading, diag_eps, eps),
          lambda rtf, psd_n, *rest: rtf.new_empty(tuple(rtf.shape)))
_register("rtf_power(Tensor psd_s, Tensor psd_n, int reference_channel, Tensor? reference_vector, int n_iter, "
          "bool diagonal_loading, float diag_eps) -> Tensor",
          lambda psd_s, psd_n, ref, vec, n_iter, loading, diag_eps:
          F._rtf_power_eager(psd_s, psd_n, _ref_of(ref, vec), n_iter, loading, diag_eps),
          lambda psd_s, psd_n, *rest: psd_n.new_empty(tuple(psd_n.shape[:-1])))
_register("apply_beamforming(Tensor beamform_weights, Tensor specgram) -> Tensor",
          F._apply_beamforming_eager, _apply_beamforming_meta)


# ---- the RNN transducer: loss, and the feature front of the pipeline -------------------------

def _rnnt_loss_meta(logits, targets, logit_lengths, target_lengths, blank, clamp, reduction, fused_log_softmax):
    if reduction not in ("none", "mean", "sum"):
        raise ValueError("reduction should be one of 'none', 'mean', or 'sum'")
    if logits.dim() != 4 or targets.dim() != 2 or targets.shape[0] != logits.shape[0] or targets.shape[1] + 1 != logits.shape[2]:
        raise ValueError(f"logits must be (batch, time, target + 1, class) and targets (batch, target): got {tuple(logits.shape)} "
                         f"and {tuple(targets.shape)}")
    return logits.new_empty((logits.shape[0],) if reduction == "none" else ())


def _rnnt_features(waveform, window, fb, n_fft, hop_length, gain, mean, invstddev, right_padding):
    out = F._mel_lognorm(waveform, window, fb, n_fft, hop_length, gain, mean, invstddev, right_padding)
    return out.view(tuple(waveform.shape[:-1]) + out.shape[-2:])


def _rnnt_features_meta(waveform, window, fb, n_fft, hop_length, gain, mean, invstddev, right_padding):
    T = _stft_frames(waveform.shape[-1], 0, n_fft, hop_length, True)
    return waveform.new_empty(tuple(waveform.shape[:-1]) + (T + right_padding, fb.shape[1]), dtype=torch.float32)


_register("rnnt_loss(Tensor logits, Tensor targets, Tensor logit_lengths, Tensor target_lengths, int blank, float clamp, "
          "str reduction, bool fused_log_softmax) -> Tensor", F._rnnt_loss_eager, _rnnt_loss_meta)
_register("rnnt_features(Tensor waveform, Tensor window, Tensor fb, int n_fft, int hop_length, float gain, Tensor mean, "
          "Tensor invstddev, int right_padding) -> Tensor", _rnnt_features, _rnnt_features_meta)
