"""Drop-in replacements for the hot-path modules of ``torchaudio.transforms``:
Spectrogram, MelScale, MelSpectrogram, AmplitudeToDB, MFCC, Resample, FFTConvolve, ComputeDeltas, SlidingWindowCmn,
FrequencyMasking, TimeMasking, SpecAugment, AddNoise, Preemphasis, Deemphasis, Convolve, PSD, MVDR, SoudenMVDR, RTFMVDR,
RNNTLoss, Vad, LFCC, SpectralCentroid, MuLawEncoding, MuLawDecoding, Fade, Vol, and of ``torchaudio.prototype.transforms``:
BarkScale, InverseBarkScale, BarkSpectrogram, ChromaScale, ChromaSpectrogram.

Constructor / forward signatures, registered buffer names (``window``, ``fb``, ``dct_mat``,
``kernel``), shapes, strides, warnings and error messages follow
src/torchaudio/transforms/_transforms.py; ``forward`` calls the HIP kernels through
``audio_amd.functional``.
"""
from __future__ import annotations

import ctypes as C
import math
import secrets
import warnings
from typing import Callable, Optional, Tuple, Union

import torch
from torch import Tensor

from . import _host, _lib
from . import functional as F
from . import _ops  # noqa: F401  (registers torch.ops.audio_amd.* -- the opaque module-level ops torch.compile sees)


_norm_mode = F._norm_mode      # `normalized` as the op schemas' integer: 0 none, 1 "frame_length", 2 "window" / True

# TorchScript (reference: test/torchaudio_unittest/transforms/torchscript_consistency_impl.py:13-76 scripts every module of this
# file).  Each ``forward`` below has two bodies: called from Python it runs ``_forward_eager`` (plan caches, autograd Functions,
# ctypes -- not compiled, the call sits behind ``torch.jit.is_scripting()``); inside a scripted program it is ONE operator of
# the ``audio_amd`` namespace (audio_amd/_ops.py) whose kernel runs the same launches, so scripted == eager bit for bit and the
# scripted module keeps ``state_dict`` keys, buffers and attributes.

__all__ = ["Spectrogram", "InverseSpectrogram", "GriffinLim", "TimeStretch", "PitchShift", "Speed", "SpeedPerturbation",
           "MelScale", "InverseMelScale", "MelSpectrogram", "AmplitudeToDB", "MFCC", "Resample", "FFTConvolve", "ComputeDeltas",
           "SlidingWindowCmn", "FrequencyMasking", "TimeMasking", "SpecAugment", "AddNoise", "Preemphasis", "Deemphasis",
           "Convolve", "PSD", "MVDR", "SoudenMVDR", "RTFMVDR", "RNNTLoss", "Vad", "LFCC", "SpectralCentroid", "MuLawEncoding",
           "MuLawDecoding", "Fade", "Vol", "BarkScale", "InverseBarkScale", "BarkSpectrogram", "ChromaScale", "ChromaSpectrogram"]


class Spectrogram(torch.nn.Module):
    r"""Spectrogram of ``(..., time)`` audio (reference: _transforms.py:25-123)."""
    __constants__ = ["n_fft", "win_length", "hop_length", "pad", "power", "normalized"]

    def __init__(
        self,
        n_fft: int = 400,
        win_length: Optional[int] = None,
        hop_length: Optional[int] = None,
        pad: int = 0,
        window_fn: Callable[..., Tensor] = torch.hann_window,
        power: Optional[float] = 2.0,
        normalized: Union[bool, str] = False,
        wkwargs: Optional[dict] = None,
        center: bool = True,
        pad_mode: str = "reflect",
        onesided: bool = True,
        return_complex: Optional[bool] = None,
    ) -> None:
        super().__init__()
        torch._C._log_api_usage_once("torchaudio.transforms.Spectrogram")
        self.n_fft = n_fft
        self.win_length = win_length if win_length is not None else n_fft
        self.hop_length = hop_length if hop_length is not None else self.win_length // 2
        window = window_fn(self.win_length) if wkwargs is None else window_fn(self.win_length, **wkwargs)
        self.register_buffer("window", window)
        self.pad = pad
        self.power = power
        self.normalized = normalized
        self.center = center
        self.pad_mode = pad_mode
        self.onesided = onesided
        if return_complex is not None:
            warnings.warn(
                "`return_complex` argument is now deprecated and is not effective."
                "`torchaudio.transforms.Spectrogram(power=None)` always returns a tensor with "
                "complex dtype. Please remove the argument in the function call."
            )

    def forward(self, waveform: Tensor) -> Tensor:
        if not torch.jit.is_scripting():
            return self._forward_eager(waveform)
        return torch.ops.audio_amd.spectrogram(waveform, self.window, self.pad, self.n_fft, self.hop_length, self.win_length,
                                               self.power, _norm_mode(self.normalized), self.center, self.pad_mode,
                                               self.onesided)

    def _forward_eager(self, waveform: Tensor) -> Tensor:
        if torch.compiler.is_compiling():          # one opaque op with a fake kernel (see MelSpectrogram.forward)
            return torch.ops.audio_amd.spectrogram(waveform, self.window, self.pad, self.n_fft, self.hop_length,
                                                   self.win_length, self.power, _norm_mode(self.normalized), self.center,
                                                   self.pad_mode, self.onesided)
        return F.spectrogram(waveform, self.pad, self.window, self.n_fft, self.hop_length, self.win_length,
                             self.power, self.normalized, self.center, self.pad_mode, self.onesided)


class InverseSpectrogram(torch.nn.Module):
    r"""Least-squares inverse of a complex spectrogram (reference: _transforms.py:126-208)."""
    __constants__ = ["n_fft", "win_length", "hop_length", "pad", "power", "normalized"]

    def __init__(
        self,
        n_fft: int = 400,
        win_length: Optional[int] = None,
        hop_length: Optional[int] = None,
        pad: int = 0,
        window_fn: Callable[..., Tensor] = torch.hann_window,
        normalized: Union[bool, str] = False,
        wkwargs: Optional[dict] = None,
        center: bool = True,
        pad_mode: str = "reflect",
        onesided: bool = True,
    ) -> None:
        super().__init__()
        self.n_fft = n_fft
        self.win_length = win_length if win_length is not None else n_fft
        self.hop_length = hop_length if hop_length is not None else self.win_length // 2
        window = window_fn(self.win_length) if wkwargs is None else window_fn(self.win_length, **wkwargs)
        self.register_buffer("window", window)
        self.pad = pad
        self.normalized = normalized
        self.center = center
        self.pad_mode = pad_mode
        self.onesided = onesided

    def forward(self, spectrogram: Tensor, length: Optional[int] = None) -> Tensor:
        return F.inverse_spectrogram(spectrogram, length, self.pad, self.window, self.n_fft, self.hop_length,
                                     self.win_length, self.normalized, self.center, self.pad_mode, self.onesided)


class GriffinLim(torch.nn.Module):
    r"""Waveform from a magnitude spectrogram by Griffin-Lim (reference: _transforms.py:212-297)."""
    __constants__ = ["n_fft", "n_iter", "win_length", "hop_length", "power", "length", "momentum", "rand_init"]

    def __init__(
        self,
        n_fft: int = 400,
        n_iter: int = 32,
        win_length: Optional[int] = None,
        hop_length: Optional[int] = None,
        window_fn: Callable[..., Tensor] = torch.hann_window,
        power: float = 2.0,
        wkwargs: Optional[dict] = None,
        momentum: float = 0.99,
        length: Optional[int] = None,
        rand_init: bool = True,
    ) -> None:
        super().__init__()
        if not (0 <= momentum < 1):
            raise ValueError("momentum must be in the range [0, 1). Found: {}".format(momentum))
        self.n_fft = n_fft
        self.n_iter = n_iter
        self.win_length = win_length if win_length is not None else n_fft
        self.hop_length = hop_length if hop_length is not None else self.win_length // 2
        window = window_fn(self.win_length) if wkwargs is None else window_fn(self.win_length, **wkwargs)
        self.register_buffer("window", window)
        self.length = length
        self.power = power
        self.momentum = momentum
        self.rand_init = rand_init

    def forward(self, specgram: Tensor) -> Tensor:
        return F.griffinlim(specgram, self.window, self.n_fft, self.hop_length, self.win_length, self.power,
                            self.n_iter, self.momentum, self.length, self.rand_init)


class TimeStretch(torch.nn.Module):
    r"""Stretch a complex STFT in time without modifying pitch (reference: _transforms.py:1014-1083)."""
    __constants__ = ["fixed_rate"]

    def __init__(self, hop_length: Optional[int] = None, n_freq: int = 201, fixed_rate: Optional[float] = None) -> None:
        super().__init__()
        self.fixed_rate = fixed_rate
        n_fft = (n_freq - 1) * 2
        hop_length = hop_length if hop_length is not None else n_fft // 2
        self.register_buffer("phase_advance", torch.linspace(0, math.pi * hop_length, n_freq)[..., None])

    def forward(self, complex_specgrams: Tensor, overriding_rate: Optional[float] = None) -> Tensor:
        if not torch.is_complex(complex_specgrams):
            raise ValueError("audio_amd: the input to TimeStretch must be a complex tensor")
        if overriding_rate is None:
            if self.fixed_rate is None:
                raise ValueError("If no fixed_rate is specified, must pass a valid rate to the forward method.")
            rate = self.fixed_rate
        else:
            rate = overriding_rate
        return F.phase_vocoder(complex_specgrams, rate, self.phase_advance)


class PitchShift(torch.nn.Module):
    r"""Shift the pitch of a waveform by ``n_steps`` steps (reference: _transforms.py:1674-1780)."""
    __constants__ = ["sample_rate", "n_steps", "bins_per_octave", "n_fft", "win_length", "hop_length"]

    def __init__(
        self,
        sample_rate: int,
        n_steps: int,
        bins_per_octave: int = 12,
        n_fft: int = 512,
        win_length: Optional[int] = None,
        hop_length: Optional[int] = None,
        window_fn: Callable[..., Tensor] = torch.hann_window,
        wkwargs: Optional[dict] = None,
    ) -> None:
        super().__init__()
        self.n_steps = n_steps
        self.bins_per_octave = bins_per_octave
        self.sample_rate = sample_rate
        self.n_fft = n_fft
        self.win_length = win_length if win_length is not None else n_fft
        self.hop_length = hop_length if hop_length is not None else self.win_length // 4
        window = window_fn(self.win_length) if wkwargs is None else window_fn(self.win_length, **wkwargs)
        self.register_buffer("window", window)
        rate = 2.0 ** (-float(n_steps) / bins_per_octave)
        self.orig_freq = int(sample_rate / rate)
        self.gcd = math.gcd(int(self.orig_freq), int(sample_rate))
        self.width = -1
        self.kernel = None          # built on the first call (the reference uses a lazy UninitializedParameter)

    def forward(self, waveform: Tensor) -> Tensor:
        if not torch.jit.is_scripting():
            return self._forward_eager(waveform)
        # (the scripted program rebuilds nothing either: F.pitch_shift keeps the tap table per parameter set)
        return torch.ops.audio_amd.pitch_shift(waveform, self.sample_rate, self.n_steps, self.bins_per_octave, self.n_fft,
                                               self.win_length, self.hop_length, self.window)

    def _forward_eager(self, waveform: Tensor) -> Tensor:
        if waveform.dtype in F.LOW_PRECISION:         # float16 / bfloat16: float32 arithmetic, the input dtype back (F._reduced_precision_io)
            return self._forward_eager(waveform.float()).to(waveform.dtype)
        F._require_device(waveform, "waveform")
        shape = waveform.size()
        stretch = F._stretch_waveform(waveform, self.n_steps, self.bins_per_octave, self.n_fft, self.win_length,
                                      self.hop_length, self.window)
        if self.orig_freq != self.sample_rate:
            if self.kernel is None or self.kernel.device != waveform.device:
                kernel, self.width = _host.sinc_resample_kernel(self.orig_freq, self.sample_rate, self.gcd,
                                                                dtype=waveform.dtype)
                self.kernel = kernel.to(waveform.device)
            shift = F._apply_sinc_resample_kernel(stretch, self.orig_freq, self.sample_rate, self.gcd, self.kernel,
                                                  self.width)
        else:
            shift = stretch
        return F._fix_waveform_shape(shift, shape)


class Speed(torch.nn.Module):
    r"""Adjust waveform speed (reference: _transforms.py:1958-2001)."""

    def __init__(self, orig_freq, factor) -> None:
        super().__init__()
        self.orig_freq = orig_freq
        self.factor = factor
        source = int(factor * orig_freq)
        target = int(orig_freq)
        gcd = math.gcd(source, target)
        self.source_sample_rate, self.target_sample_rate = source // gcd, target // gcd
        self.resampler = Resample(orig_freq=self.source_sample_rate, new_freq=self.target_sample_rate)

    def forward(self, waveform: Tensor, lengths: Optional[Tensor] = None) -> Tuple[Tensor, Optional[Tensor]]:
        if lengths is None:
            out_lengths = None
        else:
            out_lengths = torch.ceil(lengths * self.target_sample_rate / self.source_sample_rate).to(lengths.dtype)
        return self.resampler(waveform), out_lengths


class SpeedPerturbation(torch.nn.Module):
    r"""Pick one of ``factors`` uniformly at random and adjust the speed by it (reference: _transforms.py:2004-2055)."""

    def __init__(self, orig_freq: int, factors) -> None:
        super().__init__()
        self.speeders = torch.nn.ModuleList([Speed(orig_freq=orig_freq, factor=factor) for factor in factors])

    def forward(self, waveform: Tensor, lengths: Optional[Tensor] = None) -> Tuple[Tensor, Optional[Tensor]]:
        pick = int(torch.randint(len(self.speeders), ()))
        # (a walk instead of `self.speeders[pick]`: TorchScript indexes a ModuleList with constants only)
        for i, speeder in enumerate(self.speeders):
            if i == pick:
                return speeder(waveform, lengths)
        raise RuntimeError("SpeedPerturbation: no speeder was picked")


class AmplitudeToDB(torch.nn.Module):
    r"""Power/amplitude -> dB (reference: _transforms.py:300-346)."""
    __constants__ = ["multiplier", "amin", "ref_value", "db_multiplier"]

    def __init__(self, stype: str = "power", top_db: Optional[float] = None) -> None:
        super().__init__()
        self.stype = stype
        if top_db is not None and top_db < 0:
            raise ValueError("top_db must be positive value")
        self.top_db = top_db
        self.multiplier = 10.0 if stype == "power" else 20.0
        self.amin = 1e-10
        self.ref_value = 1.0
        self.db_multiplier = math.log10(max(self.amin, self.ref_value))

    def forward(self, x: Tensor) -> Tensor:
        if not torch.jit.is_scripting():
            if torch.compiler.is_compiling():
                return torch.ops.audio_amd.amplitude_to_DB(x, self.multiplier, self.amin, self.db_multiplier, self.top_db)
        return F.amplitude_to_DB(x, self.multiplier, self.amin, self.db_multiplier, self.top_db)


class ComputeDeltas(torch.nn.Module):
    r"""Delta coefficients of a ``(..., freq, time)`` tensor (reference: T.ComputeDeltas); no buffers."""
    __constants__ = ["win_length"]

    def __init__(self, win_length: int = 5, mode: str = "replicate") -> None:
        super().__init__()
        self.win_length = win_length
        self.mode = mode

    def forward(self, specgram: Tensor) -> Tensor:
        if not torch.jit.is_scripting():
            if torch.compiler.is_compiling():
                return torch.ops.audio_amd.compute_deltas(specgram, self.win_length, self.mode)
        return F.compute_deltas(specgram, win_length=self.win_length, mode=self.mode)


class SlidingWindowCmn(torch.nn.Module):
    r"""Sliding-window cepstral mean (and variance) normalisation of a ``(..., time, freq)`` tensor (reference:
    T.SlidingWindowCmn); no buffers."""

    def __init__(self, cmn_window: int = 600, min_cmn_window: int = 100, center: bool = False,
                 norm_vars: bool = False) -> None:
        super().__init__()
        self.cmn_window = cmn_window
        self.min_cmn_window = min_cmn_window
        self.center = center
        self.norm_vars = norm_vars

    def forward(self, specgram: Tensor) -> Tensor:
        if not torch.jit.is_scripting():
            if torch.compiler.is_compiling():
                return torch.ops.audio_amd.sliding_window_cmn(specgram, self.cmn_window, self.min_cmn_window, self.center,
                                                              self.norm_vars)
        return F.sliding_window_cmn(specgram, self.cmn_window, self.min_cmn_window, self.center, self.norm_vars)


class _AxisMasking(torch.nn.Module):
    r"""One mask along frequency or time (reference: _transforms.py, _AxisMasking); no buffers."""
    __constants__ = ["mask_param", "axis", "iid_masks", "p"]

    def __init__(self, mask_param: int, axis: int, iid_masks: bool, p: float = 1.0) -> None:
        super().__init__()
        self.mask_param = mask_param
        self.axis = axis
        self.iid_masks = iid_masks
        self.p = p

    def forward(self, specgram: Tensor, mask_value: float = 0.0) -> Tensor:
        if self.iid_masks:
            return F.mask_along_axis_iid(specgram, self.mask_param, mask_value, self.axis + specgram.dim() - 3, p=self.p)
        else:
            return F.mask_along_axis(specgram, self.mask_param, mask_value, self.axis + specgram.dim() - 3, p=self.p)


class FrequencyMasking(_AxisMasking):
    r"""A mask of up to ``freq_mask_param`` bins along frequency of a ``(..., freq, time)`` tensor (reference:
    T.FrequencyMasking): shared by every example, or one per example with ``iid_masks`` (three dimensions or more)."""

    def __init__(self, freq_mask_param: int, iid_masks: bool = False) -> None:
        super(FrequencyMasking, self).__init__(freq_mask_param, 1, iid_masks)


class TimeMasking(_AxisMasking):
    r"""A mask of up to ``time_mask_param`` frames (and at most ``p`` of the axis) along time (reference: T.TimeMasking)."""

    def __init__(self, time_mask_param: int, iid_masks: bool = False, p: float = 1.0) -> None:
        if not 0.0 <= p <= 1.0:
            raise ValueError(f"The value of p must be between 0.0 and 1.0 ({p} given).")
        super(TimeMasking, self).__init__(time_mask_param, 2, iid_masks, p=p)


class SpecAugment(torch.nn.Module):
    r"""Time masks, then frequency masks, filled with zero or the tensor's mean (reference: T.SpecAugment).  The whole
    policy is one kernel launch whatever the number of masks (csrc/spec_augment.h); no buffers."""
    __constants__ = ["n_time_masks", "time_mask_param", "n_freq_masks", "freq_mask_param", "iid_masks", "p", "zero_masking"]

    def __init__(self, n_time_masks: int, time_mask_param: int, n_freq_masks: int, freq_mask_param: int,
                 iid_masks: bool = True, p: float = 1.0, zero_masking: bool = False) -> None:
        super(SpecAugment, self).__init__()
        self.n_time_masks = n_time_masks
        self.time_mask_param = time_mask_param
        self.n_freq_masks = n_freq_masks
        self.freq_mask_param = freq_mask_param
        self.iid_masks = iid_masks
        self.p = p
        self.zero_masking = zero_masking

    def forward(self, specgram: Tensor) -> Tensor:
        if not torch.jit.is_scripting():
            if not torch.compiler.is_compiling():
                return F._spec_augment_eager(specgram, self.n_time_masks, self.time_mask_param, self.n_freq_masks,
                                             self.freq_mask_param, self.iid_masks, self.p, self.zero_masking)
        if specgram.dim() >= 2 and self.p >= 0.0 and self.p <= 1.0:
            # no mask at all: the input itself, decided before the op
            no_time = self.n_time_masks < 1 or F._get_mask_param(self.time_mask_param, self.p, specgram.size(-1)) < 1
            no_freq = self.n_freq_masks < 1 or F._get_mask_param(self.freq_mask_param, self.p, specgram.size(-2)) < 1
            if no_time and no_freq:
                return specgram
        return torch.ops.audio_amd.spec_augment(specgram, self.n_time_masks, self.time_mask_param, self.n_freq_masks,
                                                self.freq_mask_param, self.iid_masks, self.p, self.zero_masking)


class MelScale(torch.nn.Module):
    r"""STFT bins -> mel bins with triangular filters (reference: _transforms.py:349-415)."""
    __constants__ = ["n_mels", "sample_rate", "f_min", "f_max"]

    def __init__(
        self,
        n_mels: int = 128,
        sample_rate: int = 16000,
        f_min: float = 0.0,
        f_max: Optional[float] = None,
        n_stft: int = 201,
        norm: Optional[str] = None,
        mel_scale: str = "htk",
    ) -> None:
        super().__init__()
        self.n_mels = n_mels
        self.sample_rate = sample_rate
        self.f_max = f_max if f_max is not None else float(sample_rate // 2)
        self.f_min = f_min
        self.norm = norm
        self.mel_scale = mel_scale
        if f_min > self.f_max:
            raise ValueError("Require f_min: {} <= f_max: {}".format(f_min, self.f_max))
        fb = F.melscale_fbanks(n_stft, self.f_min, self.f_max, self.n_mels, self.sample_rate, self.norm, self.mel_scale)
        self.register_buffer("fb", fb)

    def forward(self, specgram: Tensor) -> Tensor:
        return F.mel_scale(specgram, self.fb)


class InverseMelScale(torch.nn.Module):
    r"""Mel bins -> STFT bins (reference: T.InverseMelScale, the ``lstsq`` form): ``(..., n_mels, time) -> (..., n_stft, time)``.

    The reference solves ``fb^T x = melspec`` with ``torch.linalg.lstsq(driver=...)`` and applies ``relu``; ``gels`` assumes
    a full-rank filterbank, which the default filterbanks are not (``melscale_fbanks(201, 0, 8000, 80, 16000)`` has rank 75 in
    float32).  Here the result is DEFINED as ``relu(P @ melspec)`` with ``P`` the pseudo-inverse of ``fb^T`` built in float64
    and cut at ``sigma_i > 2^-23 max(n_stft, n_mels) sigma_max``: the minimum-norm least-squares solution -- what all four
    drivers return for a full-rank ``fb`` and ``gelsd`` (default float32 ``rcond``) for a rank-deficient one.  ``driver`` is
    checked and stored and does not change the result.  One launch (``F.inverse_mel_scale``, csrc/inverse_mel.h); the module
    calls a plain Python entry point, so it is not scriptable as one op."""
    __constants__ = ["n_stft", "n_mels", "sample_rate", "f_min", "f_max"]

    def __init__(
        self,
        n_stft: int,
        n_mels: int = 128,
        sample_rate: int = 16000,
        f_min: float = 0.0,
        f_max: Optional[float] = None,
        norm: Optional[str] = None,
        mel_scale: str = "htk",
        driver: str = "gels",
    ) -> None:
        super().__init__()
        self.n_mels = n_mels
        self.sample_rate = sample_rate
        self.f_max = f_max if f_max is not None else float(sample_rate // 2)
        self.f_min = f_min
        self.n_stft = n_stft
        self.norm = norm
        self.mel_scale = mel_scale
        self.driver = driver
        if f_min > self.f_max:
            raise ValueError("Require f_min: {} <= f_max: {}".format(f_min, self.f_max))
        if driver not in ["gels", "gelsy", "gelsd", "gelss"]:
            raise ValueError(f'driver must be one of ["gels", "gelsy", "gelsd", "gelss"]. Found {driver}.')
        fb = F.melscale_fbanks(n_stft, self.f_min, self.f_max, self.n_mels, self.sample_rate, self.norm, self.mel_scale)
        self.register_buffer("fb", fb)

    def forward(self, melspec: Tensor) -> Tensor:
        return F.inverse_mel_scale(melspec, self.fb)


class MelSpectrogram(torch.nn.Module):
    r"""MelSpectrogram (reference: _transforms.py:506-622).  ``forward`` is ONE fused kernel:
    framing -> window -> FFT -> |X|^power -> banded mel; the (rows, T, freq) spectrogram the
    reference materialises between its two sub-modules never touches HBM."""
    __constants__ = ["sample_rate", "n_fft", "win_length", "hop_length", "pad", "n_mels", "f_min"]

    def __init__(
        self,
        sample_rate: int = 16000,
        n_fft: int = 400,
        win_length: Optional[int] = None,
        hop_length: Optional[int] = None,
        f_min: float = 0.0,
        f_max: Optional[float] = None,
        pad: int = 0,
        n_mels: int = 128,
        window_fn: Callable[..., Tensor] = torch.hann_window,
        power: float = 2.0,
        normalized: bool = False,
        wkwargs: Optional[dict] = None,
        center: bool = True,
        pad_mode: str = "reflect",
        onesided: Optional[bool] = None,
        norm: Optional[str] = None,
        mel_scale: str = "htk",
    ) -> None:
        super().__init__()
        torch._C._log_api_usage_once("torchaudio.transforms.MelSpectrogram")
        if onesided is not None:
            warnings.warn(
                "Argument 'onesided' has been deprecated and has no influence on the behavior of this module."
            )
        self.sample_rate = sample_rate
        self.n_fft = n_fft
        self.win_length = win_length if win_length is not None else n_fft
        self.hop_length = hop_length if hop_length is not None else self.win_length // 2
        self.pad = pad
        self.power = power
        self.normalized = normalized
        self.n_mels = n_mels
        self.f_max = f_max
        self.f_min = f_min
        self.spectrogram = Spectrogram(
            n_fft=self.n_fft, win_length=self.win_length, hop_length=self.hop_length, pad=self.pad,
            window_fn=window_fn, power=self.power, normalized=self.normalized, wkwargs=wkwargs,
            center=center, pad_mode=pad_mode, onesided=True,
        )
        self.mel_scale = MelScale(self.n_mels, self.sample_rate, self.f_min, self.f_max, self.n_fft // 2 + 1,
                                  norm, mel_scale)
        self._plans: dict = {}      # per-(shape, device, buffer version) launch plans of the inference path

    def __getstate__(self):
        state = self.__dict__.copy()
        state["_plans"] = {}            # launch plans hold op handles and device tensors: rebuilt on first use
        return state

    def _frame_major(self, waveform: Tensor, db=None) -> Tensor:
        sp = self.spectrogram
        return F._melspectrogram(waveform, sp.pad, sp.window, self.mel_scale.fb, sp.n_fft, sp.hop_length,
                                 sp.win_length, sp.power, sp.normalized, sp.center, sp.pad_mode, db=db)

    def forward(self, waveform: Tensor) -> Tensor:
        if not torch.jit.is_scripting():
            return self._forward_eager(waveform)
        return torch.ops.audio_amd.mel_spectrogram(waveform, self.spectrogram.window, self.mel_scale.fb, self.spectrogram.pad,
                                                   self.spectrogram.n_fft, self.spectrogram.hop_length,
                                                   self.spectrogram.win_length, float(self.power),
                                                   _norm_mode(self.spectrogram.normalized), self.spectrogram.center,
                                                   self.spectrogram.pad_mode)

    def _forward_eager(self, waveform: Tensor) -> Tensor:
        sp = self.spectrogram
        if torch.compiler.is_compiling():
            # torch.compile / torch.export: the module is ONE opaque op with a fake kernel (audio_amd/_ops.py); the host-side
            # plan caches (tensor identities, data pointers, ctypes) are not something a tracer should look into
            return torch.ops.audio_amd.mel_spectrogram(waveform, sp.window, self.mel_scale.fb, sp.pad, sp.n_fft,
                                                       sp.hop_length, sp.win_length, float(sp.power),
                                                       _norm_mode(sp.normalized), sp.center, sp.pad_mode)
        # low-precision / float64 / learnable / training / steady-state serving: F._melspectrogram_module (the kernel of the
        # operator above is the same function), with this module's own launch plans
        return F._melspectrogram_module(waveform, sp.window, self.mel_scale.fb, sp.pad, sp.n_fft, sp.hop_length, sp.win_length,
                                        sp.power, sp.normalized, sp.center, sp.pad_mode, self._plans)


class BarkScale(torch.nn.Module):
    r"""STFT bins -> Bark bins with triangular filters (reference: prototype.transforms.BarkScale):
    ``(..., n_stft, time) -> (..., n_barks, time)``.  The filterbank is banded, so ``forward`` is ``F.mel_scale`` on it: the
    banded kernel ``MelScale`` runs."""
    __constants__ = ["n_barks", "sample_rate", "f_min", "f_max"]

    def __init__(
        self,
        n_barks: int = 128,
        sample_rate: int = 16000,
        f_min: float = 0.0,
        f_max: Optional[float] = None,
        n_stft: int = 201,
        bark_scale: str = "traunmuller",
    ) -> None:
        super().__init__()
        self.n_barks = n_barks
        self.sample_rate = sample_rate
        self.f_max = f_max if f_max is not None else float(sample_rate // 2)
        self.f_min = f_min
        self.bark_scale = bark_scale
        if f_min > self.f_max:
            raise ValueError("Require f_min: {} <= f_max: {}".format(f_min, self.f_max))
        fb = F.barkscale_fbanks(n_stft, self.f_min, self.f_max, self.n_barks, self.sample_rate, self.bark_scale)
        self.register_buffer("fb", fb)

    def forward(self, specgram: Tensor) -> Tensor:
        return F.mel_scale(specgram, self.fb)


class InverseBarkScale(torch.nn.Module):
    r"""Bark bins -> STFT bins (reference: prototype.transforms.InverseBarkScale):
    ``(..., n_barks, time) -> (..., n_stft, time)``.

    STATED DIFFERENCE: the reference minimises ``|barkspec - fb^T x|`` by SGD from a random start.  Here the result is the
    ``InverseMelScale`` definition on the Bark filterbank -- ``relu(P @ barkspec)`` with ``P`` the float64 pseudo-inverse of
    ``fb^T`` cut at float32's rank, the minimum-norm least-squares solution, one launch (``F.inverse_mel_scale``) --
    deterministic and what the iteration converges towards.  ``max_iter``, ``tolerance_loss``, ``tolerance_change`` and
    ``sgdargs`` are stored and unused."""
    __constants__ = ["n_stft", "n_barks", "sample_rate", "f_min", "f_max", "max_iter", "tolerance_loss", "tolerance_change"]

    def __init__(
        self,
        n_stft: int,
        n_barks: int = 128,
        sample_rate: int = 16000,
        f_min: float = 0.0,
        f_max: Optional[float] = None,
        max_iter: int = 100000,
        tolerance_loss: float = 1e-5,
        tolerance_change: float = 1e-8,
        sgdargs: Optional[dict] = None,
        bark_scale: str = "traunmuller",
    ) -> None:
        super().__init__()
        self.n_barks = n_barks
        self.sample_rate = sample_rate
        self.f_max = f_max if f_max is not None else float(sample_rate // 2)
        self.f_min = f_min
        self.n_stft = n_stft
        self.max_iter = max_iter
        self.tolerance_loss = tolerance_loss
        self.tolerance_change = tolerance_change
        self.sgdargs = sgdargs or {"lr": 0.1, "momentum": 0.9}
        self.bark_scale = bark_scale
        if f_min > self.f_max:
            raise ValueError("Require f_min: {} <= f_max: {}".format(f_min, self.f_max))
        fb = F.barkscale_fbanks(n_stft, self.f_min, self.f_max, self.n_barks, self.sample_rate, self.bark_scale)
        self.register_buffer("fb", fb)

    def forward(self, barkspec: Tensor) -> Tensor:
        return F.inverse_mel_scale(barkspec, self.fb)


class BarkSpectrogram(torch.nn.Module):
    r"""Bark spectrogram of ``(..., time)`` audio (reference: prototype.transforms.BarkSpectrogram).  ``forward`` is
    ``MelSpectrogram``'s eager route with the Bark filterbank: the same ONE fused launch, dtypes and gradient routes."""
    __constants__ = ["sample_rate", "n_fft", "win_length", "hop_length", "pad", "n_barks", "f_min"]

    def __init__(
        self,
        sample_rate: int = 16000,
        n_fft: int = 400,
        win_length: Optional[int] = None,
        hop_length: Optional[int] = None,
        f_min: float = 0.0,
        f_max: Optional[float] = None,
        pad: int = 0,
        n_barks: int = 128,
        window_fn: Callable[..., Tensor] = torch.hann_window,
        power: float = 2.0,
        normalized: bool = False,
        wkwargs: Optional[dict] = None,
        center: bool = True,
        pad_mode: str = "reflect",
        bark_scale: str = "traunmuller",
    ) -> None:
        super().__init__()
        self.sample_rate = sample_rate
        self.n_fft = n_fft
        self.win_length = win_length if win_length is not None else n_fft
        self.hop_length = hop_length if hop_length is not None else self.win_length // 2
        self.pad = pad
        self.power = power
        self.normalized = normalized
        self.n_barks = n_barks
        self.f_max = f_max
        self.f_min = f_min
        self.spectrogram = Spectrogram(
            n_fft=self.n_fft, win_length=self.win_length, hop_length=self.hop_length, pad=self.pad,
            window_fn=window_fn, power=self.power, normalized=self.normalized, wkwargs=wkwargs,
            center=center, pad_mode=pad_mode, onesided=True,
        )
        self.bark_scale = BarkScale(self.n_barks, self.sample_rate, self.f_min, self.f_max, self.n_fft // 2 + 1, bark_scale)
        self._plans: dict = {}      # per-(shape, device, buffer version) launch plans of the inference path

    def __getstate__(self):
        state = self.__dict__.copy()
        state["_plans"] = {}            # launch plans hold op handles and device tensors: rebuilt on first use
        return state

    def forward(self, waveform: Tensor) -> Tensor:
        sp = self.spectrogram
        return F._melspectrogram_module(waveform, sp.window, self.bark_scale.fb, sp.pad, sp.n_fft, sp.hop_length, sp.win_length,
                                        sp.power, sp.normalized, sp.center, sp.pad_mode, self._plans)


class ChromaScale(torch.nn.Module):
    r"""STFT bins -> chroma (pitch class) bins (reference: prototype.transforms.ChromaScale):
    ``(..., n_freqs, time) -> (..., n_chroma, time)``.  The chroma filterbank is dense, so ``forward`` is
    ``F.dense_fbank_scale``: one launch of the dense projection kernel (csrc/dense_fbank.h); a plain Python entry point, so
    the module is not scriptable as one op."""
    __constants__ = ["sample_rate", "n_freqs", "n_chroma"]

    def __init__(
        self,
        sample_rate: int,
        n_freqs: int,
        *,
        n_chroma: int = 12,
        tuning: float = 0.0,
        ctroct: float = 5.0,
        octwidth: Optional[float] = 2.0,
        norm: int = 2,
        base_c: bool = True,
    ) -> None:
        super().__init__()
        self.sample_rate = sample_rate
        self.n_freqs = n_freqs
        self.n_chroma = n_chroma
        fb = F.chroma_filterbank(sample_rate, n_freqs, n_chroma, tuning=tuning, ctroct=ctroct, octwidth=octwidth, norm=norm,
                                 base_c=base_c)
        self.register_buffer("fb", fb)

    def forward(self, specgram: Tensor) -> Tensor:
        return F.dense_fbank_scale(specgram, self.fb)


class ChromaSpectrogram(torch.nn.Module):
    r"""Chromagram of ``(..., time)`` audio (reference: prototype.transforms.ChromaSpectrogram): ``(..., n_chroma, time)``.
    Two launches and no layout copy: the spectrogram of whichever STFT family serves ``n_fft``, then the dense projection
    over its frame-major memory.  ``power=None`` (a complex spectrogram) raises ``ValueError`` here, at construction; the
    reference fails later, inside ``matmul``."""
    __constants__ = ["sample_rate", "n_fft", "win_length", "hop_length", "pad", "n_chroma"]

    def __init__(
        self,
        sample_rate: int,
        n_fft: int,
        *,
        win_length: Optional[int] = None,
        hop_length: Optional[int] = None,
        pad: int = 0,
        window_fn: Callable[..., Tensor] = torch.hann_window,
        power: float = 2.0,
        normalized: bool = False,
        wkwargs: Optional[dict] = None,
        center: bool = True,
        pad_mode: str = "reflect",
        n_chroma: int = 12,
        tuning: float = 0.0,
        ctroct: float = 5.0,
        octwidth: Optional[float] = 2.0,
        norm: int = 2,
        base_c: bool = True,
    ) -> None:
        super().__init__()
        if power is None:
            raise ValueError("audio_amd: ChromaSpectrogram needs a real power (got None): the chroma filterbank is applied "
                             "to a power or magnitude spectrogram")
        self.sample_rate = sample_rate
        self.n_fft = n_fft
        self.win_length = win_length if win_length is not None else n_fft
        self.hop_length = hop_length if hop_length is not None else self.win_length // 2
        self.pad = pad
        self.n_chroma = n_chroma
        self.spectrogram = Spectrogram(
            n_fft=self.n_fft, win_length=self.win_length, hop_length=self.hop_length, pad=self.pad,
            window_fn=window_fn, power=power, normalized=normalized, wkwargs=wkwargs,
            center=center, pad_mode=pad_mode, onesided=True,
        )
        self.chroma_scale = ChromaScale(sample_rate, n_fft // 2 + 1, n_chroma=n_chroma, tuning=tuning, ctroct=ctroct,
                                        octwidth=octwidth, norm=norm, base_c=base_c)

    def forward(self, waveform: Tensor) -> Tensor:
        return self.chroma_scale(self.spectrogram(waveform))


class MFCC(torch.nn.Module):
    r"""MFCC (reference: _transforms.py:625-709): fused mel kernel, then dB (+ top_db = 80 with the
    reference's grouping of the cut-off) or log, then the DCT-II as one kernel."""
    __constants__ = ["sample_rate", "n_mfcc", "dct_type", "top_db", "log_mels"]

    def __init__(
        self,
        sample_rate: int = 16000,
        n_mfcc: int = 40,
        dct_type: int = 2,
        norm: str = "ortho",
        log_mels: bool = False,
        melkwargs: Optional[dict] = None,
    ) -> None:
        super().__init__()
        supported_dct_types = [2]
        if dct_type not in supported_dct_types:
            raise ValueError("DCT type not supported: {}".format(dct_type))
        self.sample_rate = sample_rate
        self.n_mfcc = n_mfcc
        self.dct_type = dct_type
        self.norm = norm
        self.top_db = 80.0
        self.amplitude_to_DB = AmplitudeToDB("power", self.top_db)
        melkwargs = melkwargs or {}
        self.MelSpectrogram = MelSpectrogram(sample_rate=self.sample_rate, **melkwargs)
        if self.n_mfcc > self.MelSpectrogram.n_mels:
            raise ValueError("Cannot select more MFCC coefficients than # mel bins")
        dct_mat = F.create_dct(self.n_mfcc, self.MelSpectrogram.n_mels, self.norm)
        self.register_buffer("dct_mat", dct_mat)
        self.log_mels = log_mels
        #: optional hook ``fn(group_max: Tensor) -> None`` run between the dB pass and the clamp;
        #: audio_amd.distributed installs an all-reduce(MAX) here when a batch is sharded.
        self.group_max_hook: Optional[Callable[[Tensor], None]] = None
        #: EXTENSION: which MFCC path runs.  True = the one-kernel MFCC (DCT on the f16 matrix pipe in the mel kernel's epilogue,
        #: operands split into two binary16 numbers, + a fix-up launch over the compacted list of tiles the top_db cut-off
        #: reaches); False = the exact two-kernel path; both are bit-reproducible call to call.  "auto" (default) decides ONCE
        #: per module, at its first eligible call, from the share of tiles that call had to redo (> 15 %: two kernels are
        #: cheaper) and keeps that arithmetic for every later call (F.MfccFusedState; round 3 re-decided from a polled event,
        #: so equal inputs could return different bits).  A group_max_hook (sharded batches) or a HIP-graph capture in
        #: progress run the one-kernel path without deciding.  Same results within 3e-5 dB.  Measured on the cfg4 batch
        #: (profiles/r03_d_mfcc_paths.txt): 211 us against 229 us for two kernels on noise, 220 against 234 with 5 % clamped
        #: tiles, 297 against 220 with 50 %.
        self.fused = "auto"
        #: the handle of this module's "auto" decision (F._mfcc_state_of): an integer, so that a scripted copy carries it and
        #: shares the decision -- and therefore the bits -- of the module it was scripted from
        self._fused_handle = secrets.randbits(62)

    __jit_unused_properties__ = ["_fused_state"]

    @property
    def _fused_state(self) -> "F.MfccFusedState":
        return F._mfcc_state_of(self._fused_handle)

    def fused_report(self) -> dict:
        """EXTENSION: which MFCC path ran last, the module's "auto" decision, and what the last one-kernel call's fix-up pass
        had to redo (this read synchronises with the device)."""
        st = F._mfcc_state_of(self._fused_handle)
        share = None
        if st.last_count is not None:
            share = float(st.last_count.item()) / max(st.last_tiles, 1)
        return {"path": st.path, "redone_share": share, "decided": st.decided, "decided_share": st.decided_share,
                "calls_fused": st.calls_fused, "calls_two_kernel": st.calls_two_kernel}

    def reset_fused_decision(self) -> None:
        """EXTENSION: forget the "auto" decision (the next eligible call takes it again, e.g. after the kind of batch changed)."""
        F._mfcc_state_of(self._fused_handle).reset()

    def __getstate__(self):
        d = dict(self.__dict__)
        d["_fused_handle"] = secrets.randbits(62)     # a copy / an unpickled module decides for itself
        return d

    def forward(self, waveform: Tensor) -> Tensor:
        if not torch.jit.is_scripting():
            return self._forward_eager(waveform)
        return torch.ops.audio_amd.mfcc_module(
            waveform, self.MelSpectrogram.spectrogram.window, self.MelSpectrogram.mel_scale.fb, self.dct_mat,
            self.MelSpectrogram.spectrogram.pad, self.MelSpectrogram.spectrogram.n_fft,
            self.MelSpectrogram.spectrogram.hop_length, self.MelSpectrogram.spectrogram.win_length,
            float(self.MelSpectrogram.power), _norm_mode(self.MelSpectrogram.spectrogram.normalized),
            self.MelSpectrogram.spectrogram.center, self.MelSpectrogram.spectrogram.pad_mode, self.log_mels, self.top_db,
            self.amplitude_to_DB.multiplier, self.amplitude_to_DB.amin, self.amplitude_to_DB.db_multiplier,
            _fused_mode(self.fused), self._fused_handle)

    def _forward_eager(self, waveform: Tensor) -> Tensor:
        sp = self.MelSpectrogram.spectrogram
        if torch.compiler.is_compiling():          # one opaque op with a fake kernel (see MelSpectrogram.forward)
            return torch.ops.audio_amd.mfcc(waveform, sp.window, self.MelSpectrogram.mel_scale.fb, self.dct_mat, sp.pad,
                                            sp.n_fft, sp.hop_length, sp.win_length, float(sp.power),
                                            _norm_mode(sp.normalized), sp.center, sp.pad_mode, self.log_mels, self.top_db)
        a2db = self.amplitude_to_DB
        fused = _fused_mode(getattr(self, "fused", "auto"))
        return F._mfcc_module(waveform, sp.window, self.MelSpectrogram.mel_scale.fb, self.dct_mat, sp.pad, sp.n_fft,
                              sp.hop_length, sp.win_length, sp.power, sp.normalized, sp.center, sp.pad_mode, self.log_mels,
                              self.top_db, (a2db.multiplier, a2db.amin, a2db.db_multiplier), fused,
                              F._mfcc_state_of(self._fused_handle) if fused else None, self.group_max_hook,
                              self.MelSpectrogram._plans)


def _fused_mode(fused: Union[str, bool]) -> int:
    """``MFCC.fused`` as the op schema's integer: 0 = False (two kernels), 1 = True (one kernel), 2 = "auto"."""
    if isinstance(fused, str):
        return 2
    return 1 if fused else 0


class Resample(torch.nn.Module):
    r"""Resample (reference: _transforms.py:899-980): the tap table is computed once in float64
    and cached as the float32 buffer ``kernel``; forward is the polyphase HIP kernel."""

    def __init__(
        self,
        orig_freq: int = 16000,
        new_freq: int = 16000,
        resampling_method: str = "sinc_interp_hann",
        lowpass_filter_width: int = 6,
        rolloff: float = 0.99,
        beta: Optional[float] = None,
        *,
        dtype: Optional[torch.dtype] = None,
    ) -> None:
        super().__init__()
        self.orig_freq = orig_freq
        self.new_freq = new_freq
        self.gcd = math.gcd(int(self.orig_freq), int(self.new_freq))
        self.resampling_method = resampling_method
        self.lowpass_filter_width = lowpass_filter_width
        self.rolloff = rolloff
        self.beta = beta
        if self.orig_freq != self.new_freq:
            kernel, self.width = _host.sinc_resample_kernel(
                self.orig_freq, self.new_freq, self.gcd, self.lowpass_filter_width, self.rolloff,
                self.resampling_method, beta, dtype=dtype)
            self.register_buffer("kernel", kernel)

    def forward(self, waveform: Tensor) -> Tensor:
        if self.orig_freq == self.new_freq:
            return waveform
        if not torch.jit.is_scripting():
            if torch.compiler.is_compiling():          # one opaque op with a fake kernel (see MelSpectrogram.forward)
                return torch.ops.audio_amd.resample_apply(waveform, self.kernel, self.orig_freq, self.new_freq, self.gcd,
                                                          self.width)
        return F._apply_sinc_resample_kernel(waveform, self.orig_freq, self.new_freq, self.gcd, self.kernel,
                                             self.width)


class FFTConvolve(torch.nn.Module):
    r"""Convolution along the last dim (reference: _transforms.py:1906-1948)."""

    def __init__(self, mode: str = "full") -> None:
        super().__init__()
        F._check_convolve_mode(mode)
        self.mode = mode

    def forward(self, x: Tensor, y: Tensor) -> Tensor:
        if not torch.jit.is_scripting():
            if torch.compiler.is_compiling():
                return torch.ops.audio_amd.fftconvolve(x, y, self.mode)
        return F.fftconvolve(x, y, mode=self.mode)


class Convolve(torch.nn.Module):
    r"""Convolution along the last dim, evaluated directly in the reference (reference: T.Convolve); here short kernels are a
    direct sum and long ones go through the FFT plans (``F.convolve``)."""

    def __init__(self, mode: str = "full") -> None:
        super().__init__()
        F._check_convolve_mode(mode)
        self.mode = mode

    def forward(self, x: Tensor, y: Tensor) -> Tensor:
        return F.convolve(x, y, mode=self.mode)


class AddNoise(torch.nn.Module):
    r"""Scale noise to a signal-to-noise ratio per row and add it (reference: T.AddNoise); no buffers."""

    def forward(self, waveform: Tensor, noise: Tensor, snr: Tensor, lengths: Optional[Tensor] = None) -> Tensor:
        return F.add_noise(waveform, noise, snr, lengths)


class Vad(torch.nn.Module):
    r"""Voice-activity detector: trims the silence in front of the first speech (reference: T.Vad, SoX's effect); the
    parameters, semantics and limits of :func:`audio_amd.functional.vad`.  No buffers, an empty ``state_dict``; one 8-byte
    device-to-host copy per call (the slice bound), so not capturable in a graph; not scriptable."""

    def __init__(self, sample_rate: int, trigger_level: float = 7.0, trigger_time: float = 0.25, search_time: float = 1.0,
                 allowed_gap: float = 0.25, pre_trigger_time: float = 0.0, boot_time: float = 0.35, noise_up_time: float = 0.1,
                 noise_down_time: float = 0.01, noise_reduction_amount: float = 1.35, measure_freq: float = 20.0,
                 measure_duration: Optional[float] = None, measure_smooth_time: float = 0.4, hp_filter_freq: float = 50.0,
                 lp_filter_freq: float = 6000.0, hp_lifter_freq: float = 150.0, lp_lifter_freq: float = 2000.0) -> None:
        super().__init__()
        self.sample_rate = sample_rate
        self.trigger_level = trigger_level
        self.trigger_time = trigger_time
        self.search_time = search_time
        self.allowed_gap = allowed_gap
        self.pre_trigger_time = pre_trigger_time
        self.boot_time = boot_time
        self.noise_up_time = noise_up_time
        self.noise_down_time = noise_down_time
        self.noise_reduction_amount = noise_reduction_amount
        self.measure_freq = measure_freq
        self.measure_duration = measure_duration
        self.measure_smooth_time = measure_smooth_time
        self.hp_filter_freq = hp_filter_freq
        self.lp_filter_freq = lp_filter_freq
        self.hp_lifter_freq = hp_lifter_freq
        self.lp_lifter_freq = lp_lifter_freq

    def forward(self, waveform: Tensor) -> Tensor:
        return F.vad(waveform, self.sample_rate, self.trigger_level, self.trigger_time, self.search_time, self.allowed_gap,
                     self.pre_trigger_time, self.boot_time, self.noise_up_time, self.noise_down_time, self.noise_reduction_amount,
                     self.measure_freq, self.measure_duration, self.measure_smooth_time, self.hp_filter_freq, self.lp_filter_freq,
                     self.hp_lifter_freq, self.lp_lifter_freq)


class LFCC(torch.nn.Module):
    r"""Linear-frequency cepstral coefficients (reference: T.LFCC): the spectrogram through a filterbank that is triangular
    on a LINEAR frequency scale (buffer ``filter_mat``), then dB (+ top_db = 80 with the reference's grouping of the
    cut-off) or ``log(x + 1e-6)``, then the DCT-II (buffer ``dct_mat``).  The exact two-kernel path of :class:`MFCC` with
    ``filter_mat`` in place of the mel filterbank: float64, gradients, half precision and learnable buffers as there.  Not
    registered as a dispatcher op (not scriptable as one op)."""
    __constants__ = ["sample_rate", "n_filter", "n_lfcc", "dct_type", "top_db", "log_lf"]

    def __init__(
        self,
        sample_rate: int = 16000,
        n_filter: int = 128,
        f_min: float = 0.0,
        f_max: Optional[float] = None,
        n_lfcc: int = 40,
        dct_type: int = 2,
        norm: str = "ortho",
        log_lf: bool = False,
        speckwargs: Optional[dict] = None,
    ) -> None:
        super().__init__()
        supported_dct_types = [2]
        if dct_type not in supported_dct_types:
            raise ValueError("DCT type not supported: {}".format(dct_type))
        self.sample_rate = sample_rate
        self.f_min = f_min
        self.f_max = f_max if f_max is not None else float(sample_rate // 2)
        self.n_filter = n_filter
        self.n_lfcc = n_lfcc
        self.dct_type = dct_type
        self.norm = norm
        self.top_db = 80.0
        self.amplitude_to_DB = AmplitudeToDB("power", self.top_db)
        speckwargs = speckwargs or {}
        self.Spectrogram = Spectrogram(**speckwargs)
        if self.n_lfcc > self.Spectrogram.n_fft:
            raise ValueError("Cannot select more LFCC coefficients than # fft bins")
        filter_mat = F.linear_fbanks(n_freqs=self.Spectrogram.n_fft // 2 + 1, f_min=self.f_min, f_max=self.f_max,
                                     n_filter=self.n_filter, sample_rate=self.sample_rate)
        self.register_buffer("filter_mat", filter_mat)
        dct_mat = F.create_dct(self.n_lfcc, self.n_filter, self.norm)
        self.register_buffer("dct_mat", dct_mat)
        self.log_lf = log_lf
        self._plans: dict = {}      # launch plans of the filterbank kernel (see MelSpectrogram)

    def __getstate__(self):
        state = dict(self.__dict__)
        state["_plans"] = {}
        return state

    def forward(self, waveform: Tensor) -> Tensor:
        sp, a2db = self.Spectrogram, self.amplitude_to_DB
        return F._mfcc_module(waveform, sp.window, self.filter_mat, self.dct_mat, sp.pad, sp.n_fft, sp.hop_length,
                              sp.win_length, sp.power, sp.normalized, sp.center, sp.pad_mode, self.log_lf, self.top_db,
                              (a2db.multiplier, a2db.amin, a2db.db_multiplier), 0, None, None, self._plans)


class SpectralCentroid(torch.nn.Module):
    r"""Spectral centroid per frame, ``(..., time) -> (..., frames)`` (reference: T.SpectralCentroid); one buffer,
    ``window``; the launches and limits of :func:`audio_amd.functional.spectral_centroid`."""
    __constants__ = ["sample_rate", "n_fft", "win_length", "hop_length", "pad"]

    def __init__(
        self,
        sample_rate: int,
        n_fft: int = 400,
        win_length: Optional[int] = None,
        hop_length: Optional[int] = None,
        pad: int = 0,
        window_fn: Callable[..., Tensor] = torch.hann_window,
        wkwargs: Optional[dict] = None,
    ) -> None:
        super().__init__()
        self.sample_rate = sample_rate
        self.n_fft = n_fft
        self.win_length = win_length if win_length is not None else n_fft
        self.hop_length = hop_length if hop_length is not None else self.win_length // 2
        window = window_fn(self.win_length) if wkwargs is None else window_fn(self.win_length, **wkwargs)
        self.register_buffer("window", window)
        self.pad = pad

    def forward(self, waveform: Tensor) -> Tensor:
        return F.spectral_centroid(waveform, self.sample_rate, self.pad, self.window, self.n_fft, self.hop_length,
                                   self.win_length)


class MuLawEncoding(torch.nn.Module):
    r"""Mu-law companding of a signal in [-1, 1] into int64 codes (reference: T.MuLawEncoding); no buffers."""
    __constants__ = ["quantization_channels"]

    def __init__(self, quantization_channels: int = 256) -> None:
        super().__init__()
        self.quantization_channels = quantization_channels

    def forward(self, x: Tensor) -> Tensor:
        return F.mu_law_encoding(x, self.quantization_channels)


class MuLawDecoding(torch.nn.Module):
    r"""Mu-law codes back to a signal in [-1, 1] (reference: T.MuLawDecoding); no buffers."""
    __constants__ = ["quantization_channels"]

    def __init__(self, quantization_channels: int = 256) -> None:
        super().__init__()
        self.quantization_channels = quantization_channels

    def forward(self, x_mu: Tensor) -> Tensor:
        return F.mu_law_decoding(x_mu, self.quantization_channels)


class Fade(torch.nn.Module):
    r"""Fade in and / or out along the last axis (reference: T.Fade): ``(fade_in * fade_out) * waveform`` with ramps of shape
    "linear", "exponential", "logarithmic", "quarter_sine" or "half_sine".  The ramps are host tables (float64, rounded once
    to the waveform's dtype, cached per parameters, dtype and device: run the call once eagerly before capturing it in a
    graph); one launch that multiplies inside the ramps and copies bits elsewhere.  A fade longer than the signal raises
    ``ValueError`` (the reference fails in ``torch.ones`` with a negative size).  No buffers."""

    def __init__(self, fade_in_len: int = 0, fade_out_len: int = 0, fade_shape: str = "linear") -> None:
        super().__init__()
        if fade_shape not in _host.FADE_SHAPES:
            raise ValueError(f"fade_shape must be one of {', '.join(_host.FADE_SHAPES)} (got {fade_shape!r})")
        self.fade_in_len = fade_in_len
        self.fade_out_len = fade_out_len
        self.fade_shape = fade_shape

    def forward(self, waveform: Tensor) -> Tensor:
        return F._fade(waveform, self.fade_in_len, self.fade_out_len, self.fade_shape)


class Vol(torch.nn.Module):
    r"""Adjust the volume and clamp to [-1, 1] (reference: T.Vol): ``gain_type`` "amplitude" multiplies by ``gain``, "db" is
    ``F.gain(x, gain)``, "power" is ``F.gain(x, 10 * log10(gain))``; the product and the clamp share one launch."""

    def __init__(self, gain: float, gain_type: str = "amplitude") -> None:
        super().__init__()
        self.gain = gain
        self.gain_type = gain_type
        if gain_type in ["amplitude", "power"] and gain < 0:
            raise ValueError("If gain_type = amplitude or power, gain must be positive.")

    def forward(self, waveform: Tensor) -> Tensor:
        return F._vol(waveform, self.gain, self.gain_type)


class Preemphasis(torch.nn.Module):
    r"""``y[i] = x[i] - coeff * x[i - 1]`` along the last dim (reference: T.Preemphasis); no buffers."""

    def __init__(self, coeff: float = 0.97) -> None:
        super().__init__()
        self.coeff = coeff

    def forward(self, waveform: Tensor) -> Tensor:
        return F.preemphasis(waveform, coeff=self.coeff)


class Deemphasis(torch.nn.Module):
    r"""The inverse of ``Preemphasis``, through ``lfilter`` (reference: T.Deemphasis); no buffers."""

    def __init__(self, coeff: float = 0.97) -> None:
        super().__init__()
        self.coeff = coeff

    def forward(self, waveform: Tensor) -> Tensor:
        return F.deemphasis(waveform, coeff=self.coeff)


class PSD(torch.nn.Module):
    r"""Cross-channel power spectral density matrix ``(..., freq, ch, ch)`` of a complex ``(..., ch, freq, time)``
    spectrogram (reference: T.PSD); one launch (``F.psd``).  A multi-channel mask ``(..., ch, freq, time)`` is averaged over
    its channels first."""

    def __init__(self, multi_mask: bool = False, normalize: bool = True, eps: float = 1e-15) -> None:
        super().__init__()
        self.multi_mask = multi_mask
        self.normalize = normalize
        self.eps = eps

    def forward(self, specgram: Tensor, mask: Optional[Tensor] = None) -> Tensor:
        if mask is not None:
            if self.multi_mask:
                mask = mask.mean(dim=-3)
        return F.psd(specgram, mask, self.normalize, self.eps)


class SoudenMVDR(torch.nn.Module):
    r"""MVDR beamforming by Souden's method from given PSD matrices (reference: T.SoudenMVDR): two launches, the weights
    (``F.mvdr_weights_souden``) and their application (``F.apply_beamforming``); no buffers."""

    def forward(self, specgram: Tensor, psd_s: Tensor, psd_n: Tensor, reference_channel: Union[int, Tensor],
                diagonal_loading: bool = True, diag_eps: float = 1e-7, eps: float = 1e-8) -> Tensor:
        w_mvdr = F.mvdr_weights_souden(psd_s, psd_n, reference_channel, diagonal_loading, diag_eps, eps)
        return F.apply_beamforming(w_mvdr, specgram)


class RTFMVDR(torch.nn.Module):
    r"""MVDR beamforming from a relative transfer function and the noise PSD (reference: T.RTFMVDR): two launches; no
    buffers."""

    def forward(self, specgram: Tensor, rtf: Tensor, psd_n: Tensor, reference_channel: Union[int, Tensor],
                diagonal_loading: bool = True, diag_eps: float = 1e-7, eps: float = 1e-8) -> Tensor:
        w_mvdr = F.mvdr_weights_rtf(rtf, psd_n, reference_channel, diagonal_loading, diag_eps, eps)
        return F.apply_beamforming(w_mvdr, specgram)


class MVDR(torch.nn.Module):
    r"""Mask-based MVDR beamformer (reference: T.MVDR): both PSD matrices from one pass over the spectrogram, the weights,
    the application -- three launches for ``solution="ref_channel"`` (Souden), four for ``"stv_power"`` (``F.rtf_power`` then
    ``F.mvdr_weights_rtf``).  Computed in complex128, returned in the input's dtype and (freq, time) stride order.
    ``solution="stv_evd"`` needs a Hermitian eigen-solver and ``online=True`` running state: neither is implemented."""

    def __init__(self, ref_channel: int = 0, solution: str = "ref_channel", multi_mask: bool = False, diag_loading: bool = True,
                 diag_eps: float = 1e-7, online: bool = False) -> None:
        super().__init__()
        if solution not in ["ref_channel", "stv_evd", "stv_power"]:
            raise ValueError('`solution` must be one of ["ref_channel", "stv_evd", "stv_power"]. Given {}'.format(solution))
        if solution == "stv_evd":
            raise NotImplementedError('audio_amd: MVDR(solution="stv_evd") is not implemented: it needs a Hermitian '
                                      'eigen-solver kernel; use "stv_power" or "ref_channel"')
        if online:
            raise NotImplementedError("audio_amd: MVDR(online=True) is not implemented: the recursive update of the PSD "
                                      "matrices needs running state this package does not keep")
        self.ref_channel = ref_channel
        self.solution = solution
        self.multi_mask = multi_mask
        self.diag_loading = diag_loading
        self.diag_eps = diag_eps
        self.online = online

    def forward(self, specgram: Tensor, mask_s: Tensor, mask_n: Optional[Tensor] = None) -> Tensor:
        dtype = specgram.dtype
        if specgram.ndim < 3:
            raise ValueError(f"Expected at least 3D tensor (..., channel, freq, time). Found: {specgram.shape}")
        if not specgram.is_complex():
            raise ValueError(f"The type of ``specgram`` tensor must be ``torch.cfloat`` or ``torch.cdouble``. Found: {specgram.dtype}")
        if specgram.dtype == torch.cfloat:
            specgram = specgram.cdouble()          # Convert specgram to ``torch.cdouble``.
        if mask_n is None:
            warnings.warn("``mask_n`` is not provided, use ``1 - mask_s`` as ``mask_n``.")
            mask_n = 1 - mask_s
        if self.multi_mask:
            mask_s = mask_s.mean(dim=-3)
            mask_n = mask_n.mean(dim=-3)
        both = F._psd_pair(specgram, mask_s.to(torch.float64), mask_n.to(torch.float64), True, 1e-15)
        psd_s, psd_n = both[0], both[1]
        if self.solution == "ref_channel":
            w_mvdr = F.mvdr_weights_souden(psd_s, psd_n, self.ref_channel, self.diag_loading, self.diag_eps, 1e-8)
        else:
            stv = F.rtf_power(psd_s, psd_n, self.ref_channel, 3, self.diag_loading, self.diag_eps)
            w_mvdr = F.mvdr_weights_rtf(stv, psd_n, self.ref_channel, self.diag_loading, self.diag_eps, 1e-8)
        return F.apply_beamforming(w_mvdr, specgram).to(dtype)



class RNNTLoss(torch.nn.Module):
    r"""RNN transducer loss of ``(batch, time, target + 1, class)`` joiner outputs (reference: T.RNNTLoss): ``F.rnnt_loss``
    with the module's ``blank``, ``clamp``, ``reduction`` and ``fused_log_softmax``; no buffers."""
    __constants__ = ["blank", "clamp", "reduction", "fused_log_softmax"]

    def __init__(self, blank: int = -1, clamp: float = -1.0, reduction: str = "mean", fused_log_softmax: bool = True) -> None:
        super().__init__()
        self.blank = blank
        self.clamp = clamp
        self.reduction = reduction
        self.fused_log_softmax = fused_log_softmax

    def forward(self, logits: Tensor, targets: Tensor, logit_lengths: Tensor, target_lengths: Tensor) -> Tensor:
        return F.rnnt_loss(logits, targets, logit_lengths, target_lengths, self.blank, self.clamp, self.reduction,
                           self.fused_log_softmax)
