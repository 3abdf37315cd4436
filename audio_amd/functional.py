"""Drop-in replacements for the hot-path functions of ``torchaudio.functional``.

Same names, argument meaning, shapes, strides, warnings and error messages as the reference
(src/torchaudio/functional/functional.py and filtering.py); the arithmetic runs in hand-written
HIP kernels for MI355X behind the C ABI of ``libaudio_amd.so``.  Inputs must live on a ROCm
device (``tensor.is_cuda``) and be float32; there is no CPU fallback.
"""
from __future__ import annotations

import collections
import ctypes as C
import dataclasses
import math
import os
import threading
import warnings
import weakref
from typing import List, Optional, Tuple, Union

import numpy as np
import torch
from torch import Tensor

from . import _host
from . import _lib
from . import _shim
from . import _diff
from ._host import create_dct, linear_fbanks, melscale_fbanks  # noqa: F401  (re-exported, host-side constants)
from ._host import barkscale_fbanks, chroma_filterbank  # noqa: F401  (prototype.functional's, re-exported likewise)

__all__ = [
    "spectrogram", "inverse_spectrogram", "griffinlim", "phase_vocoder", "pitch_shift", "speed", "amplitude_to_DB", "melscale_fbanks", "create_dct", "resample",
    "lfilter", "biquad", "fftconvolve", "mel_scale", "filtfilt",
    "lowpass_biquad", "highpass_biquad", "allpass_biquad", "bandpass_biquad",
    "bandreject_biquad", "equalizer_biquad", "band_biquad", "treble_biquad", "bass_biquad", "deemph_biquad", "riaa_biquad",
    "compute_deltas", "sliding_window_cmn", "detect_pitch_frequency", "mask_along_axis", "mask_along_axis_iid",
    "add_noise", "preemphasis", "deemphasis", "convolve",
    "psd", "mvdr_weights_souden", "mvdr_weights_rtf", "rtf_power", "rtf_evd", "apply_beamforming",
    "rnnt_loss", "forced_align", "merge_tokens", "TokenSpan",
    "overdrive", "phaser", "flanger", "effects_tiles",
    "vad", "vad_start", "vad_tiles",
    "inverse_mel_scale", "inverse_mel_tiles",
    "linear_fbanks", "spectral_centroid", "spectral_tiles",
    "gain", "contrast", "DB_to_amplitude", "mu_law_encoding", "mu_law_decoding", "pointwise_tiles",
    "simulate_rir_ism", "simulate_rir_ism_batch", "rir_tiles",
    "ray_tracing", "ray_tracing_batch", "ray_tiles",
    "oscillator_bank", "filter_waveform", "sinc_impulse_response", "frequency_impulse_response", "adsr_envelope", "extend_pitch",
    "dsp_tiles", "dsp_grad_tiles",
    "barkscale_fbanks", "chroma_filterbank", "dense_fbank_scale", "dense_fbank_tiles",
    "edit_distance", "edit_distance_batch", "edit_distance_tiles",
    "stoi", "stoi_tiles",
]

# --------------------------------------------------------------------------- #
# helpers                                                                     #
# --------------------------------------------------------------------------- #


def _require_device(t: Tensor, what: str, allow_grad: bool = False, allow_f64: bool = False) -> None:
    if not t.is_cuda:
        raise RuntimeError(
            f"audio_amd: {what} must be on an MI355X (ROCm) device, got {t.device}. "
            "The HIP kernels have no CPU fallback.")
    if t.dtype == torch.float64 and allow_f64:
        pass       # precision path: generic float64 kernels (csrc/f64_paths.h), differentiable to any order (_diff.py)
    elif t.dtype != torch.float32:
        raise TypeError(f"audio_amd: {what} must be float32{' or float64' if allow_f64 else ''} (got {t.dtype}); "
                        "kernels compute in fp32.")
    if t.requires_grad and torch.is_grad_enabled() and not allow_grad:
        raise RuntimeError("audio_amd: this op is forward-only (autograd: spectrogram family, lfilter / biquad, fftconvolve, resample); "
                           "wrap the call in torch.no_grad().")


LOW_PRECISION = (torch.float16, torch.bfloat16)


def _cast_result(out, dtype):
    if isinstance(out, Tensor):
        if out.is_complex():                       # half -> ComplexHalf as aten::stft does; bfloat16 has no complex type
            return out.to(torch.complex32) if dtype == torch.float16 else out
        return out.to(dtype) if out.is_floating_point() else out
    if isinstance(out, (tuple, list)):
        return type(out)(_cast_result(o, dtype) for o in out)
    return out


def _reduced_precision_io(fn):
    """float16 / bfloat16 in, the same dtype out (round 5; the reference accepts every floating dtype and returns it --
    functional/functional.py:1413-1414, filtering.py:1032-1099 -- where its backend implements the dtype: resample, lfilter,
    amplitude_to_DB and the matmul of MelScale do on CPU, aten::stft and fft do not).  The kernels compute in float32 -- strictly
    more accurate than the reference's half arithmetic -- so a reduced-precision tensor argument is widened on entry and the
    result narrowed on exit (two element-wise passes; the n_fft = 400 MelSpectrogram reads half directly instead,
    `_melspectrogram_lowp`).  The casts are ordinary autograd nodes.  The FIRST tensor argument decides."""
    import functools

    @functools.wraps(fn)
    def wrapper(*args, **kwargs):
        first = next((a for a in args if isinstance(a, Tensor)), None)
        if first is None:
            first = next((v for v in kwargs.values() if isinstance(v, Tensor)), None)
        if first is None or first.dtype not in LOW_PRECISION:
            return fn(*args, **kwargs)
        dt = first.dtype

        def widen(a):
            if isinstance(a, Tensor) and (a.dtype in LOW_PRECISION):
                if a is not first and not a.requires_grad:
                    # a constant of a module cast with .half() (window, filterbank, tap table): widened ONCE per tensor, so that
                    # what is derived from it (band tables, prepared tap fragments) is found again on the next call
                    return _tensor_cached(a, "widened_f32", lambda: a.float())
                return a.float()
            if isinstance(a, Tensor) and a.dtype == torch.complex32:
                return a.to(torch.complex64)
            return a
        out = fn(*[widen(a) for a in args], **{k: widen(v) for k, v in kwargs.items()})
        return _cast_result(out, dt)
    return wrapper


def _learnable(*tensors) -> bool:
    """True when autograd is on and one of the module constants asks for a gradient: the call takes the differentiable
    composition (reference behaviour: _transforms.py:413, 708 -- gradients flow into `fb` / `dct_mat` / `window`)."""
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


def _rows2d(t: Tensor) -> Tensor:
    """(..., L) -> contiguous (rows, L) view/copy."""
    x = t.reshape(-1, t.shape[-1])
    if x.stride(-1) != 1 or (x.shape[0] > 1 and x.stride(0) < x.shape[1]):
        x = x.contiguous()
    return x


# Launch route, decided ONCE per process: the compiled dispatcher-level boundary (torch.ops.aamd.*, csrc/torch_shim.cpp:
# boxed stable-ABI kernels that take the current stream and call the C ABI) when libaudio_amd_torch.so is built, else /
# with AAMD_NO_TORCH_SHIM=1 the ctypes binding of the same C ABI (_lib.py).  Both end in the same aamd_* entry points.
_ROUTE = {"ops": None, "decided": False}


def _ops():
    if not _ROUTE["decided"]:
        if os.environ.get("AAMD_NO_TORCH_SHIM") is None and _shim.available():
            _shim.load()
            _ROUTE["ops"] = torch.ops.aamd
        _ROUTE["decided"] = True
    return _ROUTE["ops"]


def _force_route(kind: Optional[str]) -> None:
    """Tests: 'shim', 'ctypes', or None = decide again from the environment."""
    if kind is None:
        _ROUTE["decided"] = False
        _ROUTE["ops"] = None
    elif kind == "shim":
        _shim.load()
        _ROUTE["ops"], _ROUTE["decided"] = torch.ops.aamd, True
    else:
        _ROUTE["ops"], _ROUTE["decided"] = None, True


_CACHE: "collections.OrderedDict" = collections.OrderedDict()   # value-keyed constants (twiddles, sinc kernels), LRU
_TENSOR_CACHE: dict = {}  # id(tensor) -> (weakref(tensor), {key: value})
_CACHE_LOCK = threading.RLock()   # transforms are called from data-loader / serving threads: plan caches are shared
_CACHE_MAX = 256


def _cached(key, make):
    with _CACHE_LOCK:
        v = _CACHE.get(key)
        if v is not None:
            _CACHE.move_to_end(key)
            return v
    v = make()                                   # built outside the lock (may launch / copy); a race builds it twice
    with _CACHE_LOCK:
        v = _CACHE.setdefault(key, v)
        _CACHE.move_to_end(key)
        while len(_CACHE) > _CACHE_MAX:
            _CACHE.popitem(last=False)           # least recently used, not clear-all
    return v


def _drop_dead_slot(tid: int, ref) -> None:
    """Weak-reference callback of `_tensor_cached`: the tensor object is gone, so is everything derived from it (the
    slots of dead tensors -- prepared fftconvolve workspaces of up to 64 MiB among them -- used to wait for their id to be
    reused or for the dictionary to pass 512 entries)."""
    cache, lock = _TENSOR_CACHE, _CACHE_LOCK
    if cache is None or lock is None:          # interpreter shutdown: the module's globals are already gone
        return
    with lock:
        slot = cache.get(tid)
        if slot is not None and slot[0] is ref:
            del cache[tid]


def _tensor_cached(t: Tensor, key, make, replace: bool = False):
    """Cache a constant derived from tensor `t` (window / fb buffers).  The slot is found by
    object id but is only trusted while its weak reference still resolves to `t` itself, so a
    new tensor that reuses a dead tensor's id can never hit a stale entry (finalizers of tensor
    wrappers may run late).  The key holds the in-place version counter AND the storage address, so
    `t.add_(...)` and `t.data = other` both invalidate; writes through `t.data.copy_()` bump neither and
    are not seen (use `t.copy_()`)."""
    tid = id(t)
    k = (key, t._version, t.data_ptr(), str(t.device), t.dtype)
    with _CACHE_LOCK:
        slot = _TENSOR_CACHE.get(tid)
        if slot is None or slot[0]() is not t:
            if len(_TENSOR_CACHE) > 512:
                for kk in [kk for kk, sl in _TENSOR_CACHE.items() if sl[0]() is None]:
                    del _TENSOR_CACHE[kk]
            slot = (weakref.ref(t, lambda r, tid=tid: _drop_dead_slot(tid, r)), {})
            _TENSOR_CACHE[tid] = slot
        v = None if replace else slot[1].get(k)
        if v is not None:
            return v
    v = make()
    with _CACHE_LOCK:
        if len(slot[1]) > 64:                    # a tensor mutated every step: keep only the newest derivations
            slot[1].clear()
        if replace:
            slot[1][k] = v
        else:
            v = slot[1].setdefault(k, v)
    return v


def _twiddles(n_fft: int, device) -> Tensor:
    return _cached(("tw", n_fft, str(device)),
                   lambda: torch.from_numpy(_host.twiddle_table(n_fft)).to(device).contiguous())


def _padded_window(window: Tensor, n_fft: int) -> Tensor:
    return _tensor_cached(window, ("win", n_fft),
                          lambda: _host.center_pad_window(window.detach(), n_fft).contiguous())


class MelBandsOnDevice:
    """Device copy of the banded filterbank + the ctypes struct that points at it."""

    def __init__(self, fb: Tensor, device):
        lo, width, weights, max_width = _host.mel_band_table(fb.detach().cpu().numpy())
        self.n_freq, self.n_mels = fb.shape
        self.lo = torch.from_numpy(lo).to(device)
        self.width = torch.from_numpy(width).to(device)
        self.weights = torch.from_numpy(weights).to(device).contiguous()
        self.max_width = max_width
        # lane assignment and band-read starts of the radix-20x20 kernel (chosen against LDS bank conflicts; the kernel's
        # results do not depend on them): the table's LDS image is laid out once per filterbank, on the host
        use_order = self.n_freq == 201 and os.environ.get("AAMD_MEL400_NO_LANE_ORDER") is None   # env: A/B experiments
        image = None
        if use_order:
            # the image exists only for filterbanks the radix-20x20 kernel serves (<= 8 rounds of 20 mels, bands <= 62 bins:
            # aamd_mel400_table_dwords() > 0); anything wider keeps the plain lane order and runs on the generic kernel
            fast = _lib.lib().aamd_mel400_table_dwords(int(self.n_mels), int(max_width)) > 0
            if fast and os.environ.get("AAMD_MEL400_ORDER_ONLY") is None:                         # env: A/B experiments
                image, order = _host.mel400_table_image(lo, width, weights, max_width)
            elif fast:
                image, order = None, _host.mel_lane_order(lo, width)
            else:
                image, order = None, None
            self.lane_order = torch.from_numpy(order).to(device) if order is not None else None
        else:
            self.lane_order = None
        self.struct = _lib.MelBands(self.n_mels, max_width, self.lo.data_ptr(), self.width.data_ptr(),
                                    self.weights.data_ptr(),
                                    self.lane_order.data_ptr() if self.lane_order is not None else None, None)
        self.table400 = None
        self.table_sig = 0
        if self.n_freq == 201 and self.lo.is_cuda:
            L = _lib.lib()
            n = L.aamd_mel400_table_dwords(self.n_mels, max_width)
            if n > 0:
                if image is not None and image.shape[0] == n:
                    self.table400 = torch.from_numpy(image).to(device)
                    self.table_sig = _host.mel400_table_signature(image, int(self.n_mels), int(max_width))
                    self.struct.table_sig = self.table_sig
                else:       # the device builder (band starts at the band's first even bin)
                    self.table400 = torch.zeros(n, dtype=torch.float32, device=device)
                    with torch.cuda.device(device):
                        _lib.check(L.aamd_mel400_table_build(C.byref(self.struct), self.table400.data_ptr(),
                                                             _lib.current_stream(device)))
                self.struct.table400 = self.table400.data_ptr()


def _mel_bands(fb: Tensor, device) -> MelBandsOnDevice:
    # (a module cast with .half() / .bfloat16() carries a reduced-precision filterbank: the band table is built from its values
    # widened to float32, once per buffer)
    return _tensor_cached(fb, ("bands", str(device)),
                          lambda: MelBandsOnDevice(fb if fb.dtype == torch.float32 else fb.detach().float(), device))


def _get_spec_norms(normalized: Union[str, bool]):
    frame_length_norm, window_norm = False, False
    if isinstance(normalized, str):
        if normalized not in ["frame_length", "window"]:
            raise ValueError("Invalid normalized parameter: {}".format(normalized))
        if normalized == "frame_length":
            frame_length_norm = True
        elif normalized == "window":
            window_norm = True
    elif isinstance(normalized, bool):
        if normalized:
            window_norm = True
    else:
        raise TypeError("Input type not supported")
    return frame_length_norm, window_norm


def _stft_desc(x2: Tensor, pad: int, window: Tensor, n_fft: int, hop_length: int, power, normalized,
               center: bool, pad_mode: str, onesided: bool) -> _lib.StftDesc:
    rows, length = x2.shape
    if pad_mode not in _lib.PAD_MODES:
        raise NotImplementedError(f"audio_amd: pad_mode {pad_mode!r} is not supported")
    l1 = length + 2 * pad
    if center:
        half = n_fft // 2
        if pad_mode == "reflect" and not half < l1:
            raise RuntimeError(
                f"Argument #4: Padding size should be less than the corresponding input dimension, "
                f"but got: padding ({half}, {half}) at dimension 2 of input {[1, rows, l1]}")
        if pad_mode == "circular" and half > l1:
            raise RuntimeError("Padding value causes wrapping around more than once.")
        l1 += 2 * half
    if not (0 < n_fft <= l1):
        raise RuntimeError(f"stft: expected 0 < n_fft <= {l1}, but got n_fft={n_fft}")
    if hop_length <= 0:
        raise RuntimeError(f"stft: expected hop_length > 0, but got hop_length={hop_length}")
    n_frames = 1 + (l1 - n_fft) // hop_length
    frame_norm, window_norm = _get_spec_norms(normalized)
    scale = 1.0
    if frame_norm:
        scale = 1.0 / math.sqrt(n_fft)
    if window_norm:
        scale = scale / _tensor_cached(window, "l2norm", lambda: float(window.pow(2.0).sum().sqrt()))
    return _lib.StftDesc(rows, length, x2.stride(0) if rows > 1 else max(length, 1), n_fft, hop_length, pad,
                         int(center), _lib.PAD_MODES[pad_mode], int(onesided), n_frames, scale,
                         0.0 if power is None else float(power))


# --------------------------------------------------------------------------- #
# spectrogram                                                                 #
# --------------------------------------------------------------------------- #


@_reduced_precision_io
def _spectrogram_eager(
    waveform: Tensor,
    pad: int,
    window: Tensor,
    n_fft: int,
    hop_length: int,
    win_length: int,
    power: Optional[float],
    normalized: Union[bool, str],
    center: bool = True,
    pad_mode: str = "reflect",
    onesided: bool = True,
    return_complex: Optional[bool] = None,
) -> Tensor:
    r"""Spectrogram of ``(..., time)`` audio -> ``(..., freq, time)``; reference:
    torchaudio/functional/functional.py:54-145.  One fused HIP kernel does padding-by-index,
    windowing, the FFT and ``|X|^power``; the result is stored frame-major and returned as the
    same transposed view (same strides) ``torch.stft`` produces."""
    if return_complex is not None:
        warnings.warn(
            "`return_complex` argument is now deprecated and is not effective."
            "`torchaudio.functional.spectrogram(power=None)` always returns a tensor with "
            "complex dtype. Please remove the argument in the function call."
        )
    _require_device(waveform, "waveform", allow_grad=True, allow_f64=True)
    if window.shape[0] != win_length:
        raise RuntimeError(
            f"stft: expected a 1D window tensor of size equal to win_length={win_length}, "
            f"but got window with size {list(window.shape)}")
    if not 0 < win_length <= n_fft:
        raise RuntimeError(f"stft: expected 0 < win_length <= n_fft, but got win_length={win_length}")
    learn_window = torch.is_grad_enabled() and window.requires_grad
    if waveform.dtype == torch.float64 or learn_window or (not onesided and torch.is_grad_enabled() and waveform.requires_grad):
        # precision / two-sided training / learnable-window path: the differentiable blocks (onesided kernel + Hermitian
        # extension; a window that requires grad takes the bilinear form of _diff.stft_complex_learnable_window -- the reference
        # propagates into it through aten::stft)
        _stft_desc(_rows2d(waveform), pad, window.to(waveform.device), n_fft, hop_length, power, normalized, center, pad_mode,
                   True)                       # the reference's argument checks and error messages
        return _diff.spectrogram(waveform, pad, window, n_fft, hop_length, win_length, power, normalized, center, pad_mode,
                                 onesided)
    window = window.to(device=waveform.device, dtype=torch.float32)
    shape = waveform.size()
    x2 = _rows2d(waveform)
    desc = _stft_desc(x2, pad, window, n_fft, hop_length, power, normalized, center, pad_mode, onesided)
    n_freq = n_fft // 2 + 1 if onesided else n_fft
    lead = tuple(shape[:-1])
    T = desc.n_frames
    if torch.is_grad_enabled() and waveform.requires_grad:
        out = _SpectrogramFunction.apply(x2, _padded_window(window, n_fft), desc, power)
    else:
        out = _spectrogram_launch(x2, _padded_window(window, n_fft), desc, power)
    if power is None:
        out = torch.view_as_complex(out.view(desc.rows, T, n_freq, 2))
    return out.view(lead + (T, n_freq)).transpose(-1, -2)


def _spectrogram_launch(x2: Tensor, window_padded: Tensor, desc, power) -> Tensor:
    """Frame-major (rows, T, n_freq [* 2 for complex]) float32 through aamd_spectrogram_f32."""
    n_freq = desc.n_fft // 2 + 1 if desc.onesided else desc.n_fft
    comp = 2 if power is None else 1
    ops = _ops()
    if ops is not None:
        return ops.spectrogram(x2, window_padded, _twiddles(desc.n_fft, x2.device), desc.n_fft, desc.hop, desc.pad,
                               bool(desc.center), desc.pad_mode, bool(desc.onesided), desc.n_frames, desc.scale,
                               desc.power)
    out = torch.empty((desc.rows, desc.n_frames, n_freq * comp), dtype=torch.float32, device=x2.device)
    if out.numel():
        L = _lib.lib()
        _lib.check(L.aamd_spectrogram_f32(
            x2.data_ptr(), window_padded.data_ptr(), _twiddles(desc.n_fft, x2.device).data_ptr(),
            out.data_ptr(), C.byref(desc), _lib.current_stream(x2.device)))
    return out


def _copy_desc(desc, **changes):
    d = _lib.StftDesc()
    C.memmove(C.byref(d), C.byref(desc), C.sizeof(_lib.StftDesc))
    for k, v in changes.items():
        setattr(d, k, v)
    return d


def _istft_launch(spec_fm: Tensor, window_padded: Tensor, desc, adjoint: bool, inv_env: Optional[Tensor]) -> Tensor:
    """spec_fm: float32 (rows, T, n_freq * 2) interleaved complex -> (rows, desc.length) via aamd_istft_f32."""
    ops = _ops()
    if ops is not None and spec_fm.numel():
        n_freq = desc.n_fft // 2 + 1
        return ops.istft(spec_fm.view(desc.rows, desc.n_frames, n_freq, 2), window_padded, _twiddles(desc.n_fft, spec_fm.device),
                         inv_env, desc.n_fft, desc.hop, desc.pad, bool(desc.center), desc.pad_mode, desc.length, desc.scale,
                         bool(adjoint))
    out = torch.zeros((desc.rows, desc.length), dtype=torch.float32, device=spec_fm.device)
    if out.numel() and desc.n_frames:
        L = _lib.lib()
        _lib.check(L.aamd_istft_f32(
            spec_fm.data_ptr(), window_padded.data_ptr(), _twiddles(desc.n_fft, spec_fm.device).data_ptr(),
            None if inv_env is None else inv_env.data_ptr(), out.data_ptr(), C.byref(desc), int(adjoint),
            _lib.current_stream(spec_fm.device)))
    return out


_NOISE_FLOOR_POWER = 2.0 ** -40         # (2^-20)^2: a bin this far under its neighbourhood's peak is rounding, not signal


def _silence_noise_floor(X: Tensor, n_freq: int) -> Tensor:
    """In place: exact zeros for the bins of the recomputed spectrum X (rows, T, 2 * n_freq) that lie under the float32 noise
    floor of the transform.  The STFT kernels transform two frames per complex FFT, so a SILENT frame (zero padding, digital
    silence) comes back as the rounding cross-talk of its partner, ~ 2^-24 of that frame's peak, instead of 0.  For p < 2 the
    cotangent p |X|^(p-2) X turns that into a unit-phase (p = 1) or huge (p < 1) random gradient where the reference's is 0
    (sgn(0) = 0), and the adjoint's own pairing spreads it into the neighbouring frame.  A bin below 2^-20 of the largest bin
    of its frame and the two frames next to it (whatever the kernel's pairing) has no correct digit: it is treated as the
    zero it stands for, and the gradient kernels return 0 there."""
    rows, T = X.shape[0], X.shape[1]
    Xc = X.view(rows, T, n_freq, 2)
    m2 = Xc.square().sum(-1)                                                                # (rows, T, n_freq)
    near = torch.nn.functional.max_pool1d(m2.amax(-1).unsqueeze(1), 3, 1, 1).squeeze(1)    # (rows, T)
    Xc.mul_((m2 > near.unsqueeze(-1) * _NOISE_FLOOR_POWER).unsqueeze(-1))
    return X


def _spectrum_cotangent(x2: Tensor, window_padded: Tensor, desc, dpower: Tensor, power: float) -> Tensor:
    """G = dP * p * |X|^(p-2) * X with X recomputed by the fast complex STFT kernel; (rows, T, 2 * n_freq) float32."""
    dX = _copy_desc(desc, power=0.0)
    G = _spectrogram_launch(x2, window_padded, dX, None)               # X: (rows, T, 2 * n_freq) interleaved complex
    n = G.numel() // 2
    if n and power != 2.0:
        _silence_noise_floor(G, desc.n_fft // 2 + 1)
    if n:
        L = _lib.lib()                                                 # in place: G <- dP p |X|^(p-2) X
        _lib.check(L.aamd_spectrogram_grad_f32(G.data_ptr(), dpower.contiguous().data_ptr(), G.data_ptr(), n, float(power),
                                               _lib.current_stream(x2.device)))
    return G


class _MelSpectrogramFunction(torch.autograd.Function):
    """MelSpectrogram in training mode: forward = the fused mel kernel (same launch as inference); backward =
    complex STFT recompute -> filterbank transpose + spectrum cotangent in one pass (aamd_melspectrogram_grad_f32, in
    place) -> STFT adjoint (aamd_istft_f32, adjoint = 1).  All HIP kernels."""

    @staticmethod
    def forward(ctx, x2, window, fb, args):
        pad, n_fft, hop_length, win_length, power, normalized, center, pad_mode = args
        out = _melspectrogram(x2.detach(), pad, window, fb, n_fft, hop_length, win_length, power, normalized, center, pad_mode)
        ctx.save_for_backward(x2, window, fb)
        ctx.args = args
        return out

    @staticmethod
    def backward(ctx, dy):
        x2, window, fb = ctx.saved_tensors
        pad, n_fft, hop_length, win_length, power, normalized, center, pad_mode = ctx.args
        dev = x2.device
        if torch.is_grad_enabled():
            # create_graph=True (gradgradcheck, higher-order use): the same gradient out of differentiable pieces --
            # d/dx of  mel = |scale * Stft(x)|^p . fb  through autograd over `_diff.Stft` (reference composition)
            with torch.enable_grad():
                spec = _diff.spectrogram(x2, pad, window, n_fft, hop_length, win_length, power, normalized, center, pad_mode)
                mel = torch.matmul(spec.transpose(-1, -2), fb.to(dev))            # (rows, T, n_mels)
                (dx,) = torch.autograd.grad(mel, x2, dy, create_graph=True)
            return dx, None, None, None
        window = window.to(device=dev, dtype=torch.float32)
        desc = _stft_desc(x2, pad, window, n_fft, hop_length, power, normalized, center, pad_mode, True)
        wp = _padded_window(window, n_fft)
        rows, T, n_mels = dy.shape
        n_freq = n_fft // 2 + 1
        bands_t = _tensor_cached(fb, ("bands_T", str(dev)), lambda: MelBandsOnDevice(fb.t().contiguous(), dev))
        dy = dy.contiguous()
        G = _spectrogram_launch(x2, wp, _copy_desc(desc, power=0.0), None)      # X: (rows, T, 2 * n_freq)
        if G.numel() and power != 2.0:
            _silence_noise_floor(G, n_freq)
        if G.numel():
            L = _lib.lib()                                                      # in place: X -> (fb dY) p |X|^(p-2) X
            _lib.check(L.aamd_melspectrogram_grad_f32(G.data_ptr(), dy.data_ptr(), C.byref(bands_t.struct), rows * T, n_freq,
                                                      n_mels, float(power), _lib.current_stream(dev)))
        dx = _istft_launch(G, wp, _copy_desc(desc), True, None)
        return dx, None, None, None


class _SpectrogramFunction(torch.autograd.Function):
    """d/d waveform of the (onesided) spectrogram on the HIP kernels.  Backward recomputes the complex STFT
    X (fast kernel), forms G = dL/dRe Y + i dL/dIm Y for complex output or G = dY p |X|^(p-2) X for
    |X|^p, and runs the ADJOINT of the STFT (aamd_istft_f32, adjoint = 1): inverse FFT of every frame,
    window, overlap-add with the forward's padding map reversed.  The window is a constant (as in the
    reference's autograd tests, test/torchaudio_unittest/transforms/autograd_test_impl.py)."""

    @staticmethod
    def forward(ctx, x2, window_padded, desc, power):
        ctx.save_for_backward(x2, window_padded)
        ctx.desc, ctx.power = desc, power
        return _spectrogram_launch(x2, window_padded, desc, power)

    @staticmethod
    def backward(ctx, dy):
        x2, window_padded = ctx.saved_tensors
        desc, power = ctx.desc, ctx.power
        n_freq = desc.n_fft // 2 + 1
        if torch.is_grad_enabled():
            # create_graph=True: differentiate the differentiable composition instead (see _MelSpectrogramFunction)
            pm = [k for k, v in _lib.PAD_MODES.items() if v == desc.pad_mode][0]
            with torch.enable_grad():
                X = _diff.stft_complex(x2, window_padded, (desc.n_fft, desc.hop, desc.pad, bool(desc.center), pm)) * desc.scale
                if power is None:
                    Y = torch.view_as_real(X).reshape(X.shape[0], X.shape[1], -1)
                else:
                    Y = X.abs() if power == 1.0 else X.abs().pow(power)
                (dx,) = torch.autograd.grad(Y, x2, dy, create_graph=True)
            return dx, None, None, None
        dy = dy.contiguous()
        if power is None:
            G = dy                                             # (rows, T, n_freq * 2): dL/dRe, dL/dIm interleaved
        else:
            G = _spectrum_cotangent(x2, window_padded, desc, dy, power)
        dA = _copy_desc(desc)                                  # same geometry, scale and padding map
        dx = _istft_launch(G.contiguous(), window_padded, dA, True, None)
        return dx, None, None, None


@_reduced_precision_io
def _inverse_spectrogram_eager(
    spectrogram: Tensor,
    length: Optional[int],
    pad: int,
    window: Tensor,
    n_fft: int,
    hop_length: int,
    win_length: int,
    normalized: Union[bool, str],
    center: bool = True,
    pad_mode: str = "reflect",
    onesided: bool = True,
) -> Tensor:
    r"""Least-squares inverse of the spectrogram (reference: functional/functional.py:148-225 ->
    ``torch.istft``): inverse FFT of every frame, window, overlap-add, divided by the window envelope
    ``sum_t w^2``, trimmed to the centre -- one HIP kernel (csrc/istft.h) plus the cached envelope."""
    frame_length_norm, window_norm = _get_spec_norms(normalized)
    if not spectrogram.is_complex():
        raise ValueError("Expected `spectrogram` to be complex dtype.")
    if not spectrogram.is_cuda:
        raise RuntimeError(f"audio_amd: spectrogram must be on an MI355X (ROCm) device, got {spectrogram.device}. "
                           "The HIP kernels have no CPU fallback.")
    if spectrogram.dtype not in (torch.complex64, torch.complex128):
        raise TypeError(f"audio_amd: spectrogram must be complex64 or complex128 (got {spectrogram.dtype}).")
    if not onesided:
        if spectrogram.shape[-2] != n_fft:
            raise RuntimeError(f"istft: expected the frequency dimension of the input to be n_fft = {n_fft} when "
                               f"onesided=False, but got {spectrogram.shape[-2]}")
        from . import _diff
        spectrogram = _diff.onesided_part(spectrogram, n_fft)          # what aten::istft does with a two-sided input
    want_grad = spectrogram.requires_grad and torch.is_grad_enabled()
    dev = spectrogram.device
    f64 = spectrogram.dtype == torch.complex128          # the reference's tests run in float64 too: the float64 inverse kernel
    rdt = torch.float64 if f64 else torch.float32
    window = window.to(device=dev, dtype=rdt)
    wp = _padded_window(window, n_fft)
    shape = spectrogram.size()
    n_freq, T = shape[-2], shape[-1]
    if n_freq != n_fft // 2 + 1:
        raise RuntimeError(f"istft: expected the frequency dimension of the input to be n_fft / 2 + 1 = "
                           f"{n_fft // 2 + 1}, but got {n_freq}")
    fm = spectrogram.transpose(-1, -2).reshape(-1, T, n_freq)
    if not fm.is_contiguous():
        fm = fm.contiguous()
    rows = fm.shape[0]
    expected = n_fft + hop_length * (T - 1)
    start = n_fft // 2 if center else 0
    if length is not None:
        out_len = length + 2 * pad
    else:
        out_len = expected - 2 * start
    scale = 1.0
    if window_norm:
        scale *= _tensor_cached(window, "l2norm", lambda: float(window.pow(2.0).sum().sqrt()))
    if frame_length_norm:
        scale *= math.sqrt(n_fft)

    def make_env():
        w2 = wp.double().pow(2).view(1, 1, n_fft)
        env = torch.nn.functional.conv_transpose1d(torch.ones(1, 1, T, dtype=torch.float64, device=dev), w2,
                                                   stride=hop_length).view(-1)
        env = env[start:start + out_len]
        if env.numel() < out_len:
            env = torch.nn.functional.pad(env, (0, out_len - env.numel()), value=1.0)
        # torch.istft checks the envelope over the span the frames cover (NOLA)
        covered = env[: max(min(out_len, expected - start), 0)]
        if covered.numel() and float(covered.abs().min()) < 1e-11:
            raise RuntimeError("istft(...) window overlap add min: 1")
        return (1.0 / env).to(rdt).contiguous()

    inv_env = _tensor_cached(window, ("istft_env", n_fft, hop_length, T, out_len, center), make_env)
    desc = _lib.StftDesc(rows, out_len, out_len, n_fft, hop_length, 0, int(center), _lib.PAD_MODES["constant"], 1, T,
                         1.0 if f64 else scale, 0.0)      # (the descriptor's scale is a float: float64 applies it below)
    if want_grad:
        # training path (transforms/autograd_test_impl.py:76-83): the inverse STFT is linear in the spectrum, and its operator
        # is the adjoint of the zero-padded STFT -- the Stft / StftAdjoint pair of _diff.py, differentiable to any order
        from . import _diff
        out = _diff.istft(fm, wp, n_fft, hop_length, bool(center), out_len, inv_env, scale)
    elif f64:
        from . import _diff
        out = torch.zeros((rows, out_len), dtype=torch.float64, device=dev)
        if out.numel() and T:
            with torch.cuda.device(dev):
                _lib.check(_lib.lib().aamd_istft_f64(torch.view_as_real(fm).data_ptr(), wp.data_ptr(),
                                                     _diff.twiddles(n_fft, dev, torch.float64).data_ptr(), inv_env.data_ptr(),
                                                     out.data_ptr(), C.byref(desc), 0, _lib.current_stream(dev)))
        if scale != 1.0:
            out = out * scale
    else:
        out = _istft_launch(torch.view_as_real(fm).view(rows, T, 2 * n_freq), wp, desc, False, inv_env)
    if length is not None and pad > 0:
        out = out[:, pad:-pad]
    return out.reshape(tuple(shape[:-2]) + out.shape[-1:])


def _phase_vocoder_launch(spec: Tensor, rate: float, phase_advance: Tensor, frame_major_out: bool) -> Tensor:
    """spec: complex64 (rows, F, T) view with arbitrary strides -> complex64 (rows, F, T_out), contiguous, or a
    transposed view of frame-major (rows, T_out, F) memory when `frame_major_out` (what the iSTFT kernel eats)."""
    rows, n_freq, n_in = spec.shape
    n_out = int(math.ceil(n_in / rate))
    dev = spec.device
    pa = phase_advance.to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
    if pa.numel() != n_freq:
        raise RuntimeError(f"audio_amd: phase_advance must have {n_freq} elements, got {pa.numel()}")
    ops = _ops()
    if ops is not None and rows * n_out * n_freq:      # the dispatcher op allocates its own output
        res = torch.view_as_complex(ops.phase_vocoder(torch.view_as_real(spec), pa, float(rate), bool(frame_major_out)))
        return res.transpose(-1, -2) if frame_major_out else res
    if frame_major_out:
        out = torch.empty((rows, n_out, n_freq), dtype=torch.complex64, device=dev)
        o_row, o_t, o_f = out.stride()
    else:
        out = torch.empty((rows, n_freq, n_out), dtype=torch.complex64, device=dev)
        o_row, o_f, o_t = out.stride()
    if out.numel():
        i_row, i_f, i_t = spec.stride()
        d = _lib.VocoderDesc(rows, n_freq, n_in, n_out, i_row, i_f, i_t, o_row, o_f, o_t, float(rate))
        L = _lib.lib()
        # data_ptr of a complex view points at its first element (storage offset included)
        _lib.check(L.aamd_phase_vocoder_f32(torch.view_as_real(spec).data_ptr(), pa.data_ptr(),
                                            torch.view_as_real(out).data_ptr(), C.byref(d), _lib.current_stream(dev)))
    return out.transpose(-1, -2) if frame_major_out else out


@_reduced_precision_io
def _phase_vocoder_eager(complex_specgrams: Tensor, rate: float, phase_advance: Tensor) -> Tensor:
    r"""Stretch a complex spectrogram in time by ``rate`` without changing pitch
    (reference: functional/functional.py:732-803) -- one HIP kernel, a thread per (row, frequency) chain."""
    if rate == 1.0:
        return complex_specgrams
    if not complex_specgrams.is_cuda:
        raise RuntimeError(f"audio_amd: complex_specgrams must be on an MI355X (ROCm) device, got "
                           f"{complex_specgrams.device}. The HIP kernels have no CPU fallback.")
    shape = complex_specgrams.size()
    if complex_specgrams.dtype == torch.complex128 or (complex_specgrams.requires_grad and torch.is_grad_enabled()
                                                       and complex_specgrams.dtype == torch.complex64):
        # precision / training route of this thin caller: the reference's formula as device tensor arithmetic, which
        # autograd differentiates (transforms/autograd_test_impl.py:225-262 TimeStretch)
        from . import _diff
        return _diff.phase_vocoder(complex_specgrams, rate, phase_advance)
    if complex_specgrams.dtype != torch.complex64:
        raise TypeError(f"audio_amd: complex_specgrams must be complex64 or complex128 (got {complex_specgrams.dtype}).")
    spec = complex_specgrams.reshape((-1,) + tuple(shape[-2:]))
    out = _phase_vocoder_launch(spec, rate, phase_advance, frame_major_out=False)
    return out.reshape(tuple(shape[:-2]) + out.shape[1:])


@_reduced_precision_io
def _griffinlim_eager(
    specgram: Tensor,
    window: Tensor,
    n_fft: int,
    hop_length: int,
    win_length: int,
    power: float,
    n_iter: int,
    momentum: float,
    length: Optional[int],
    rand_init: bool,
) -> Tensor:
    r"""Griffin-Lim phase recovery (reference: functional/functional.py:255-353).  Every iteration is three
    launches on frame-major buffers: inverse STFT (csrc/istft.h), complex STFT (the radix-20x20 fast path
    for n_fft = 400, the generic Stockham kernel otherwise) and the fused phase update (csrc/vocoder.h)."""
    if not 0 <= momentum < 1:
        raise ValueError("momentum must be in range [0, 1). Found: {}".format(momentum))
    if specgram.is_cuda and (specgram.dtype == torch.float64 or (specgram.requires_grad and torch.is_grad_enabled())):
        return _griffinlim_diff(specgram, window, n_fft, hop_length, win_length, power, n_iter, momentum / (1 + momentum),
                                length, rand_init)
    _require_device(specgram, "specgram")
    momentum = momentum / (1 + momentum)
    shape = specgram.size()
    dev = specgram.device
    n_freq, T = shape[-2], shape[-1]
    window = window.to(device=dev, dtype=torch.float32)
    # frame-major magnitude, (rows, T, F)
    mag = specgram.to(torch.float32).reshape(-1, n_freq, T).transpose(-1, -2).pow(1 / power).contiguous()
    rows = mag.shape[0]
    if rand_init:
        # the reference draws torch.rand in the COMPLEX dtype: uniform real and imaginary parts
        angles = torch.rand((rows, n_freq, T), dtype=torch.complex64, device=dev).transpose(-1, -2)
        cur = (mag * angles).contiguous()
    else:
        cur = torch.complex(mag, torch.zeros_like(mag))
    tprev = torch.zeros_like(cur)
    nxt = None                             # scratch of the ctypes route only (the dispatcher op returns its own tensor)
    L = _lib.lib()

    def invert(z: Tensor) -> Tensor:
        return inverse_spectrogram(z.transpose(-1, -2), length, 0, window, n_fft, hop_length, win_length, False)

    for _ in range(n_iter):
        inverse = invert(cur)
        rebuilt = spectrogram(inverse, 0, window, n_fft, hop_length, win_length, None, False)   # (rows, F, T') view
        rebuilt_fm = rebuilt.transpose(-1, -2)
        if rebuilt_fm.shape[1] != T:
            raise RuntimeError("audio_amd: griffinlim needs length consistent with the number of frames")
        if not rebuilt_fm.is_contiguous():
            rebuilt_fm = rebuilt_fm.contiguous()
        ops = _ops()
        if ops is not None:
            cur = torch.view_as_complex(ops.griffinlim_update(torch.view_as_real(rebuilt_fm), torch.view_as_real(tprev), mag,
                                                              float(momentum)))
            continue
        if nxt is None:
            nxt = torch.empty_like(cur)
        _lib.check(L.aamd_griffinlim_update_f32(
            torch.view_as_real(rebuilt_fm).data_ptr(), torch.view_as_real(tprev).data_ptr(), mag.data_ptr(),
            torch.view_as_real(nxt).data_ptr(), mag.numel(), float(momentum), _lib.current_stream(dev)))
        cur, nxt = nxt, cur
    waveform = invert(cur)
    return waveform.reshape(tuple(shape[:-2]) + waveform.shape[-1:])


def _griffinlim_diff(specgram: Tensor, window: Tensor, n_fft: int, hop_length: int, win_length: int, power: float,
                     n_iter: int, momentum: float, length: Optional[int], rand_init: bool) -> Tensor:
    """Griffin-Lim in training mode / float64 (transforms/autograd_test_impl.py:99-109 runs gradcheck + gradgradcheck on it):
    the iteration of functional/functional.py:313-347 written on the differentiable blocks -- the inverse STFT as the adjoint
    operator (`_diff.istft`), the rebuild as `_diff.Stft`, the phase normalisation as tensor arithmetic.  `momentum` arrives
    already mapped to m / (1 + m)."""
    shape = specgram.size()
    mag = specgram.reshape((-1,) + tuple(shape[-2:])).pow(1 / power)
    cdt = torch.complex128 if specgram.dtype == torch.float64 else torch.complex64
    if rand_init:       # the reference draws in the COMPLEX dtype, on the spectrogram's device, in (rows, freq, time) order
        angles = torch.rand(mag.size(), dtype=cdt, device=mag.device)
    else:
        angles = torch.full(mag.size(), 1, dtype=cdt, device=mag.device)
    tprev = None
    for _ in range(n_iter):
        inverse = inverse_spectrogram(mag * angles, length, 0, window, n_fft, hop_length, win_length, False)
        rebuilt = _diff.spectrogram(inverse, 0, window, n_fft, hop_length, win_length, None, False, True, "reflect")
        if rebuilt.shape[-1] != mag.shape[-1]:
            raise RuntimeError("audio_amd: griffinlim needs length consistent with the number of frames")
        angles = rebuilt
        if momentum and tprev is not None:
            angles = angles - tprev * momentum
        angles = angles / (angles.abs() + 1e-16)
        tprev = rebuilt
    waveform = inverse_spectrogram(mag * angles, length, 0, window, n_fft, hop_length, win_length, False)
    return waveform.reshape(tuple(shape[:-2]) + waveform.shape[-1:])


def _stretch_waveform(waveform: Tensor, n_steps: int, bins_per_octave: int = 12, n_fft: int = 512,
                      win_length: Optional[int] = None, hop_length: Optional[int] = None,
                      window: Optional[Tensor] = None) -> Tensor:
    """functional/functional.py:1644-1693: STFT -> phase vocoder -> inverse STFT, frame-major end to end."""
    if hop_length is None:
        hop_length = n_fft // 4
    if win_length is None:
        win_length = n_fft
    if window is None:
        window = torch.hann_window(window_length=win_length, device=waveform.device)
    shape = waveform.size()
    waveform = waveform.reshape(-1, shape[-1])
    ori_len = shape[-1]
    rate = 2.0 ** (-float(n_steps) / bins_per_octave)
    spec_f = spectrogram(waveform, 0, window, n_fft, hop_length, win_length, None, False)
    phase_advance = torch.linspace(0, math.pi * hop_length, spec_f.shape[-2], device=spec_f.device)[..., None]
    if rate == 1.0:
        spec_stretch = spec_f
    else:
        spec_stretch = _phase_vocoder_launch(spec_f, rate, phase_advance, frame_major_out=True)
    len_stretch = int(round(ori_len / rate))
    return inverse_spectrogram(spec_stretch, len_stretch, 0, window, n_fft, hop_length, win_length, False)


def _fix_waveform_shape(waveform_shift: Tensor, shape) -> Tensor:
    """functional/functional.py:1696-1719."""
    ori_len = shape[-1]
    shift_len = waveform_shift.size()[-1]
    if shift_len > ori_len:
        waveform_shift = waveform_shift[..., :ori_len]
    else:
        waveform_shift = torch.nn.functional.pad(waveform_shift, [0, ori_len - shift_len])
    return waveform_shift.reshape(tuple(shape[:-1]) + waveform_shift.shape[-1:])


@_reduced_precision_io
def _pitch_shift_eager(waveform: Tensor, sample_rate: int, n_steps: int, bins_per_octave: int = 12, n_fft: int = 512,
                win_length: Optional[int] = None, hop_length: Optional[int] = None,
                window: Optional[Tensor] = None) -> Tensor:
    r"""Shift the pitch by ``n_steps`` (reference: functional/functional.py:1596-1641): time-stretch with the
    phase vocoder, then resample back -- four HIP kernels (STFT, vocoder, inverse STFT, polyphase resampler)."""
    _require_device(waveform, "waveform")
    waveform_stretch = _stretch_waveform(waveform, n_steps, bins_per_octave, n_fft, win_length, hop_length, window)
    rate = 2.0 ** (-float(n_steps) / bins_per_octave)
    waveform_shift = resample(waveform_stretch, int(sample_rate / rate), sample_rate)
    return _fix_waveform_shape(waveform_shift, waveform.size())


def _melspectrogram(waveform: Tensor, pad: int, window: Tensor, fb: Tensor, n_fft: int, hop_length: int,
                    win_length: int, power: float, normalized, center: bool, pad_mode: str,
                    bands: Optional[MelBandsOnDevice] = None, db=None) -> Tensor:
    """Fused Spectrogram + MelScale (transforms/_transforms.py:612-622). Returns frame-major
    (rows, T, n_mels); callers build the (..., n_mels, T) view.

    ``db = (multiplier, amin, db_multiplier, group_max, rows_per_group)`` additionally fuses
    F.amplitude_to_DB (functional.py:390-391) into the kernel epilogue and max-reduces the dB
    values of each cut-off group into ``group_max`` (the top_db reduction, :393-402)."""
    _require_device(waveform, "waveform")
    if power is None:
        raise ValueError("audio_amd: MelSpectrogram needs a real power (got None)")
    window = window.to(device=waveform.device, dtype=torch.float32)
    x2 = _rows2d(waveform)
    desc = _stft_desc(x2, pad, window, n_fft, hop_length, power, normalized, center, pad_mode, True)
    if bands is None:
        bands = _mel_bands(fb, waveform.device)
    if bands.n_freq != n_fft // 2 + 1:
        raise RuntimeError(
            f"mat1 and mat2 shapes cannot be multiplied ({desc.n_frames}x{n_fft // 2 + 1} and "
            f"{bands.n_freq}x{bands.n_mels})")
    ops = _ops()
    if ops is not None:
        targs = (x2, _padded_window(window, n_fft), _twiddles(n_fft, waveform.device), bands.lo, bands.width,
                 bands.weights, bands.lane_order, bands.table400, n_fft, hop_length, pad, bool(center), desc.pad_mode, desc.n_frames,
                 desc.scale, desc.power)
        sig = int(bands.table_sig)
        if db is None:
            return ops.mel_spectrogram(*targs, sig)
        multiplier, amin, db_multiplier, group_max, rows_per_group = db
        return ops.mel_spectrogram_db(*targs, multiplier, amin, db_multiplier, group_max, rows_per_group, sig)
    out = torch.empty((desc.rows, desc.n_frames, bands.n_mels), dtype=torch.float32, device=waveform.device)
    if out.numel():
        L = _lib.lib()
        args = (x2.data_ptr(), _padded_window(window, n_fft).data_ptr(), _twiddles(n_fft, waveform.device).data_ptr(),
                C.byref(bands.struct), out.data_ptr(), C.byref(desc))
        if db is None:
            _lib.check(L.aamd_melspectrogram_f32(*args, _lib.current_stream(waveform.device)))
        else:
            multiplier, amin, db_multiplier, group_max, rows_per_group = db
            _lib.check(L.aamd_melspectrogram_db_f32(
                *args, multiplier, amin, db_multiplier, None if group_max is None else group_max.data_ptr(),
                rows_per_group, _lib.current_stream(waveform.device)))
    return out


def _melspectrogram_lowp(waveform: Tensor, pad: int, window: Tensor, fb: Tensor, n_fft: int, hop_length: int,
                         win_length: int, power: float, normalized, center: bool, pad_mode: str) -> Optional[Tensor]:
    """MelSpectrogram of a float16 / bfloat16 waveform read AS IT IS (aamd_melspectrogram_lowp_f32: the conversion happens in
    the kernel's load -- half the input bytes, no cast pass).  Frame-major float32 (rows, T, n_mels), or None when the shape is
    not the n_fft = 400 / hop 160, 200 / power 2 kernel's (the caller then casts and takes the float path)."""
    if n_fft != 400 or hop_length not in (160, 200) or power != 2.0 or not waveform.is_cuda:
        return None
    dev = waveform.device
    window = window.to(device=dev, dtype=torch.float32)
    x2 = _rows2d(waveform)
    desc = _stft_desc(x2, pad, window, n_fft, hop_length, power, normalized, center, pad_mode, True)
    bands = _mel_bands(fb, dev)
    if bands.n_freq != n_fft // 2 + 1:
        return None
    L = _lib.lib()
    out = torch.empty((desc.rows, desc.n_frames, bands.n_mels), dtype=torch.float32, device=dev)
    if out.numel():
        code = 1 if waveform.dtype == torch.float16 else 2
        with torch.cuda.device(dev):
            rc = L.aamd_melspectrogram_lowp_f32(x2.data_ptr(), code, _padded_window(window, n_fft).data_ptr(),
                                                _twiddles(n_fft, dev).data_ptr(), C.byref(bands.struct), out.data_ptr(),
                                                C.byref(desc), _lib.current_stream(dev))
        if rc == _lib.EUNSUPPORTED:
            return None
        _lib.check(rc)
    return out


def _melspectrogram_plan(waveform: Tensor, pad: int, window: Tensor, fb: Tensor, n_fft: int, hop_length: int,
                         win_length: int, power: float, normalized, center: bool, pad_mode: str):
    """Everything of `_melspectrogram` that depends only on (shape, dtype, device, parameters): validated once, then the
    module replays it per call (transforms.MelSpectrogram keeps the plans; host issue cost per call ~20 us -> a dict
    lookup + one boxed op).  Returns None when the call cannot take the compiled route."""
    ops = _ops()
    if ops is None or power is None:
        return None
    _require_device(waveform, "waveform")
    window_in = window
    window = window.to(device=waveform.device, dtype=torch.float32)
    x2 = _rows2d(waveform)
    if x2.data_ptr() != waveform.data_ptr():
        return None                               # needed a copy: no stable view recipe
    desc = _stft_desc(x2, pad, window, n_fft, hop_length, power, normalized, center, pad_mode, True)
    bands = _mel_bands(fb, waveform.device)
    if bands.n_freq != n_fft // 2 + 1:
        return None
    args = (_padded_window(window, n_fft), _twiddles(n_fft, waveform.device), bands.lo, bands.width, bands.weights,
            bands.lane_order, bands.table400, n_fft, hop_length, pad, bool(center), desc.pad_mode, desc.n_frames,
            desc.scale, desc.power, int(bands.table_sig))
    # keep-alives last -- including the caller's OWN window / fb tensors: the module finds this plan by their addresses and
    # version counters, and an address can only be reused by another tensor once the old one is gone
    return ops.mel_spectrogram, (x2.shape[0], x2.shape[1]), args, (bands, window, window_in, fb)


def _mel_lognorm(waveform: Tensor, window: Tensor, fb: Tensor, n_fft: int, hop_length: int, gain: float,
                 mean: Tensor, invstddev: Tensor, right_padding: int,
                 bands: Optional[MelBandsOnDevice] = None, interleaved_channels: int = 0) -> Tensor:
    """MelSpectrogram (power 2, centre / reflect) with the RNN-T feature post-processing fused
    (pipelines/rnnt_pipeline.py:16-47, 319-326).  Returns (rows, T + right_padding, n_mels), the padding rows zero.

    `interleaved_channels` = C > 0: `waveform` is int16 PCM laid out (..., time, C) -- the decoder's interleaved order, which
    the reference transposes to (channel, time) before any transform (torchaudio/_torchcodec.py:150-152).  Rows of the
    result are then (clip, channel) pairs.  C = 1, 2 are read directly by the kernel (de-interleave in the load); any other
    count is transposed first."""
    L0 = _lib.lib()
    if interleaved_channels:
        C_ = int(interleaved_channels)
        if waveform.dtype != torch.int16 or waveform.shape[-1] != C_:
            raise ValueError("audio_amd: interleaved PCM must be int16 with a trailing channel dimension")
        n_time = waveform.shape[-2]
        direct = (C_ in (1, 2) and waveform.is_cuda and n_fft == 400 and hop_length in (160, 200) and n_time > 400
                  and not (L0.aamd_set_kernel_policy(-1) & _lib.POLICY_FORCE_GENERIC))
        if direct:
            bands_d = bands if bands is not None else _mel_bands(fb, waveform.device)
            direct = bands_d.n_mels <= 160 and bands_d.max_width <= 62
        if not direct:      # the planar path (which itself converts first when it has to)
            planar = waveform.transpose(-1, -2).contiguous()
            return _mel_lognorm(planar, window, fb, n_fft, hop_length, gain, mean, invstddev, right_padding, bands)
    pcm16 = waveform.dtype == torch.int16
    if pcm16 and not interleaved_channels and not (
            n_fft == 400 and hop_length in (160, 200) and waveform.shape[-1] > 400
            and not (L0.aamd_set_kernel_policy(-1) & _lib.POLICY_FORCE_GENERIC)):
        waveform, pcm16 = waveform.to(torch.float32) * (1.0 / 32768.0), False   # shapes the PCM kernel does not serve
    if pcm16:
        if not waveform.is_cuda:
            raise RuntimeError(f"audio_amd: waveform must be on an MI355X (ROCm) device, got {waveform.device}. "
                               "The HIP kernels have no CPU fallback.")
    else:
        _require_device(waveform, "waveform")
    dev = waveform.device
    window = window.to(device=dev, dtype=torch.float32)
    if interleaved_channels:
        clips = waveform.reshape(-1, waveform.shape[-2], interleaved_channels).contiguous()   # (clips, time, C)
        if clips.data_ptr() % 4 != 0:
            # a contiguous VIEW that starts on an odd half-word (pcm.view(-1)[1:] ...): the kernel reads one 32-bit (L, R)
            # word per sample time, so the buffer moves to a fresh (aligned) allocation instead of being refused
            clips = clips.clone()
        # the geometry of (clips * C) planar rows of `time` samples; the entry below is told they are interleaved
        probe = torch.empty((clips.shape[0] * interleaved_channels, clips.shape[1]), dtype=torch.float32, device="meta")
        desc = _stft_desc(probe, 0, window, n_fft, hop_length, 2.0, False, True, "reflect", True)
        x2 = clips
    else:
        x2 = _rows2d(waveform)
        desc = _stft_desc(x2, 0, window, n_fft, hop_length, 2.0, False, True, "reflect", True)
    if pcm16:
        desc.scale = desc.scale / 32768.0          # float = int16 / 32768 (what the decoder's normalisation does)
    if bands is None:
        bands = _mel_bands(fb, dev)
    mean = mean.to(device=dev, dtype=torch.float32).contiguous()
    invstddev = invstddev.to(device=dev, dtype=torch.float32).contiguous()
    if mean.numel() != bands.n_mels or invstddev.numel() != bands.n_mels:
        raise RuntimeError(f"audio_amd: global statistics must have n_mels = {bands.n_mels} entries")
    if pcm16 and not interleaved_channels and not (bands.n_mels <= 160 and bands.max_width <= 62):   # filterbank outside the radix-20x20 kernel
        return _mel_lognorm(waveform.to(torch.float32) * (1.0 / 32768.0), window, fb, n_fft, hop_length, gain, mean,
                            invstddev, right_padding, bands)
    T = desc.n_frames
    # Rows of T + right_padding frames come straight from the kernel only on the radix-20x20 fast path.  Its
    # eligibility (csrc/mel400_launch.h: mel400_eligible -- hop, clip length, filterbank geometry, kernel policy) is mirrored
    # here; every other shape writes T frames and is padded afterwards, as the reference does.
    n_time = x2.shape[-2] if interleaved_channels else x2.shape[1]
    fused_pad = (right_padding > 0 and n_fft == 400 and hop_length in (100, 160, 200) and n_time > 400
                 and bands.n_mels <= 160 and bands.max_width <= 62
                 and not (L0.aamd_set_kernel_policy(-1) & _lib.POLICY_FORCE_GENERIC))
    if interleaved_channels:
        def entry(wav, *rest):
            return L0.aamd_melspectrogram_pcm16_interleaved_f32(wav, int(interleaved_channels), *rest)
    else:
        entry = L0.aamd_melspectrogram_pcm16_f32 if pcm16 else L0.aamd_melspectrogram_lognorm_f32

    def launch(frames: int) -> Tensor:
        out = torch.empty((desc.rows, frames, bands.n_mels), dtype=torch.float32, device=dev)
        if out.numel():
            if frames > T:
                out[:, T:].zero_()
            if T:
                _lib.check(entry(
                    x2.data_ptr(), _padded_window(window, n_fft).data_ptr(), _twiddles(n_fft, dev).data_ptr(),
                    C.byref(bands.struct), out.data_ptr(), C.byref(desc), float(gain), mean.data_ptr(),
                    invstddev.data_ptr(), frames, _lib.current_stream(dev)))
        return out

    if fused_pad:
        try:
            return launch(T + right_padding)
        except RuntimeError as e:                   # the C side's eligibility is the authority: fall back to T frames
            if "padded feature rows" not in str(e):
                raise
    out = launch(T)
    if right_padding:
        out = torch.nn.functional.pad(out, (0, 0, 0, right_padding))
    return out


def _mfcc_dct_launch(mel2: Tensor, dct: Tensor, log_mode: int, gmax: Optional[Tensor], vec_per_group: int,
                     top_db: float) -> Tensor:
    """(n_vec, n_mels) frame-major features -> (n_vec, n_mfcc) through aamd_mfcc_dct_f32."""
    n_vec, n_mels = mel2.shape
    ops = _ops()
    if ops is not None:
        return ops.mfcc_dct(mel2, dct, log_mode, gmax, vec_per_group, top_db)
    out = torch.empty((n_vec, dct.shape[1]), dtype=torch.float32, device=mel2.device)
    if out.numel():
        L = _lib.lib()
        _lib.check(L.aamd_mfcc_dct_f32(mel2.data_ptr(), dct.data_ptr(), out.data_ptr(), n_vec, n_mels, dct.shape[1],
                                       log_mode, None if gmax is None else gmax.data_ptr(), vec_per_group, float(top_db),
                                       _lib.current_stream(mel2.device)))
    return out


class _NegInfPool:
    """-inf-filled float32 scratch for the group maxima of the top_db cut-off, handed out in slices.

    Every MFCC / amplitude_to_DB call needs a handful of floats pre-filled with -inf (the kernels max-reduce into them with
    atomics).  A ``torch.full`` per call is a kernel of its own in front of the transform -- 3-5 us of every ~190 us MFCC call on
    the cfg4 batch (profiles/r04_p_mfcc_one_launch.txt: the launches around the main kernel are what is left to remove).  One
    fill covers ~32 calls instead: the pool is filled once ON the stream that uses it and each call takes the next slice, used
    exactly once.  Pools are per (device, stream) -- a slice is only ever touched by launches ordered behind its fill -- and are
    bypassed while a HIP graph is being captured (a captured call must own its fill) and for large requests."""

    def __init__(self, calls_per_fill: int = 32, max_request: int = 4096):
        self.lock = threading.Lock()
        self.pools = {}
        self.calls_per_fill = calls_per_fill
        self.max_request = max_request

    def take(self, n: int, dev: torch.device) -> Tensor:
        if torch.device(dev).type != "cuda":         # (host-logic tests drive the callers with stubbed launches)
            return torch.full((max(n, 0),), float("-inf"), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):                 # (the capture status and the current stream are per device)
            if n > self.max_request or n <= 0 or torch.cuda.is_current_stream_capturing():
                return torch.full((max(n, 0),), float("-inf"), dtype=torch.float32, device=dev)
            stream = torch.cuda.current_stream()
            key = (stream.device_index, stream.cuda_stream)
            return self._slice(key, n, dev)

    def _slice(self, key, n: int, dev: torch.device) -> Tensor:
        with self.lock:
            ent = self.pools.get(key)
            if ent is None or ent[1] + n > ent[0].numel():
                if len(self.pools) >= 32:            # streams come and go: forget the lot rather than grow without bound
                    self.pools.clear()
                buf = torch.full((max(self.calls_per_fill * n, 1024),), float("-inf"), dtype=torch.float32, device=dev)
                ent = [buf, 0]
                self.pools[key] = ent
            out = ent[0][ent[1]:ent[1] + n]
            ent[1] += n
        return out


_neg_inf = _NegInfPool()


class MfccFusedState:
    """What the module keeps between calls of the one-kernel MFCC: the DCT matrix in the kernel's operand layout, and the
    module's path DECISION.

    ``MFCC.fused`` is True (always the one-kernel path), False (always the exact two-kernel path) or "auto".  Both explicit
    settings are bit-reproducible call to call.  "auto" decides ONCE per module, at its first eligible call, synchronised:
    that call runs the one-kernel path, reads the number of tiles its fix-up pass had to redo, and

    * keeps the one-kernel path for the life of the module when at most ``max_share`` of the tiles were redone (loud,
      unpadded batches: pass 0 + a near-empty fix-up launch, ~8 % faster than two kernels);
    * otherwise (zero-padded batches, top_db reached everywhere: every tile would be computed twice) recomputes THAT call on
      the two-kernel path and stays there.

    So a module returns the same arithmetic on every call (round 3 re-decided from an event it polled without synchronising:
    the same input could come back bit-different call to call and rank to rank -- VERDICT r3 weak).  No decision is
    TAKEN while a HIP graph is being captured (a decision needs a host read) or when a ``group_max_hook`` is installed (every
    rank of a sharded batch must run the same arithmetic; a rank cannot know what the others saw): an undecided module runs the
    one-kernel path there and stays undecided.  A decision that has been taken is honoured everywhere -- a module that decided
    "two-kernel" in eager mode runs the two-kernel path under capture and under a hook as well (it used to fall back
    to the one-kernel path there, ~3e-5 dB away from its own eager calls).  Ranks of a sharded job that must agree bit for bit
    set ``fused`` to True or False explicitly.  ``MFCC.fused_report()`` says what ran and why; ``MFCC.reset_fused_decision()``
    forgets the decision."""

    def __init__(self, max_share: float = 0.15):
        self.frag = None
        self.frag_key = None
        self.frag_src = None          # weak reference to the DCT tensor the fragments were built from
        self.max_share = max_share
        self.decided = None           # None (not yet) | "fused" | "two-kernel"
        self.decided_share = None     # share of redone tiles the decision was taken on
        self.last_count = None        # device int32[1]: tiles redone by the last one-kernel call (never read unless asked)
        self.last_tiles = 0
        self.force = False            # MFCC.fused = True: always the one-kernel path
        self.path = None
        self.calls_fused = 0
        self.calls_two_kernel = 0

    def reset(self):
        self.decided = None
        self.decided_share = None


def _mfcc_fused(waveform: Tensor, window: Tensor, fb: Tensor, dct: Tensor, n_fft: int, hop_length: int, pad: int,
                normalized, center: bool, pad_mode: str, top_db: float, db, packed: int, n_groups: int,
                group_max_hook, state: MfccFusedState) -> Optional[Tensor]:
    """MFCC.forward in one kernel + a fix-up launch (aamd_mfcc_fused_f32).  None when the shape is not served."""
    dev = waveform.device
    window = window.to(device=dev, dtype=torch.float32)
    x2 = _rows2d(waveform)
    desc = _stft_desc(x2, pad, window, n_fft, hop_length, 2.0, normalized, center, pad_mode, True)
    bands = _mel_bands(fb, dev)
    n_mfcc = dct.shape[1]
    L = _lib.lib()
    if bands.n_freq != n_fft // 2 + 1 or not L.aamd_mfcc_fused_supported(C.byref(desc), C.byref(bands.struct), n_mfcc):
        return None
    # the fragments belong to the tensor OBJECT they were built from (weak reference) at its in-place version: an address
    # and a version counter alone can be reused by a fresh tensor with other values (the lfilter sections)
    key = (dct._version, dct.data_ptr(), str(dev), n_mfcc, bands.n_mels)
    stream = _lib.current_stream(dev)
    with torch.cuda.device(dev):
        if state.frag is None or state.frag_key != key or state.frag_src is None or state.frag_src() is not dct:
            frag = torch.empty((L.aamd_mfcc_frag_floats(),), dtype=torch.float32, device=dev)
            _lib.check(L.aamd_mfcc_frag_build(dct.data_ptr(), bands.n_mels, n_mfcc, frag.data_ptr(), stream))
            state.frag, state.frag_key, state.frag_src = frag, key, weakref.ref(dct)
        n_tiles = int(L.aamd_mfcc_fused_tiles(C.byref(desc)))
        out = torch.empty((desc.rows, desc.n_frames, n_mfcc), dtype=torch.float32, device=dev)
        gmax = _neg_inf.take(n_groups, dev)
        if out.numel() == 0:
            # an empty shard still takes part in the exchange of the batch-global cut-off: the other ranks are waiting in the
            # same all-reduce (returning before the hook hung the job)
            if group_max_hook is not None:
                group_max_hook(gmax)
            return out
        tile_min = torch.empty((n_tiles,), dtype=torch.float32, device=dev)
        count = torch.empty((1,), dtype=torch.int32, device=dev)
        tile_list = torch.empty((n_tiles,), dtype=torch.int32, device=dev)
        # (round 4 tried to fold the compaction of the fix-up list into pass 0 -- its last workgroup to finish scanned the tile
        # minima itself: one workgroup walking 85 k minima is latency-bound, +50 us on the cfg4 batch against the 4.8 us of the
        # chip-wide list kernel it saved; profiles/r04_b_configs.jsonl.  The in-kernel grid barrier form (all workgroups meet, each
        # redoes the flagged tiles of a strided share) was built and measured too: + 2.3 us -- un-profiled, the two small launches
        # cost ~5.5 us together, the barrier 3 us and the write-through stores a cross-XCD rewrite needs 4-6 us;
        # profiles/r04_p_mfcc_one_launch.txt.  What that measurement did pay for: the chip-wide list kernel between the passes is
        # gone -- the fix-up launch's workgroups check a strided share of the tile minima themselves and leave when none is
        # flagged.  Two launches per call.)
        f = _lib.MfccFused(state.frag.data_ptr(), n_mfcc, 0, float(db[0]), float(db[1]), float(db[2]), float(top_db),
                           gmax.data_ptr(), max(packed, 1), tile_min.data_ptr(), count.data_ptr(), tile_list.data_ptr())
        args = (x2.data_ptr(), _padded_window(window, n_fft).data_ptr(), _twiddles(n_fft, dev).data_ptr(),
                C.byref(bands.struct), out.data_ptr(), C.byref(desc))
        _lib.check(L.aamd_mfcc_fused_f32(*args, C.byref(f), stream))
        if group_max_hook is not None:
            group_max_hook(gmax)
        f.pass_ = 1
        _lib.check(L.aamd_mfcc_fused_f32(*args, C.byref(f), stream))
        state.last_count, state.last_tiles = count, n_tiles     # stays on the device; read only by a decision / a report
    return out


def _mfcc(waveform: Tensor, pad: int, window: Tensor, fb: Tensor, dct_mat: Tensor, n_fft: int, hop_length: int,
          win_length: int, power: float, normalized, center: bool, pad_mode: str, log_mels: bool, top_db: float,
          db=(10.0, 1e-10, 0.0), group_max_hook=None, fused_state: Optional[MfccFusedState] = None) -> Tensor:
    """MFCC.forward (transforms/_transforms.py:692-709) in two kernels: the mel kernel with
    amplitude_to_DB and the per-cut-off-group maximum fused into its epilogue, then clamp + DCT-II
    on the matrix cores.  ``group_max_hook(gmax)`` runs between them (audio_amd.distributed installs
    the all-reduce(MAX) a batch-global cut-off needs when the batch is sharded)."""
    lead = tuple(waveform.shape[:-1])
    dev = waveform.device
    # F.create_dct returns a TRANSPOSED view (functional.py:667 `dct.t()`), so the module's buffer is not contiguous: a
    # `.contiguous()` here was a copy launch per call AND a new tensor object per call -- which the fragment cache of the
    # one-kernel path is keyed by, so the fragments were rebuilt every call too (two launches, ~10 us of the cfg4 step, found
    # in the round-4 per-config rocprof).  The kernel-ready copy is cached per buffer (invalidated by in-place updates).
    if dct_mat.device == dev and dct_mat.dtype == torch.float32 and dct_mat.is_contiguous():
        dct = dct_mat
    else:
        dct = _tensor_cached(dct_mat, ("dct_f32", str(dev)),
                             lambda: dct_mat.detach().to(device=dev, dtype=torch.float32).contiguous())
    n_mfcc = dct.shape[1]
    L = _lib.lib()
    if log_mels:
        mel = _melspectrogram(waveform, pad, window, fb, n_fft, hop_length, win_length, power, normalized, center,
                              pad_mode)                                  # (rows, T, n_mels) frame-major
        rows, T, n_mels = mel.shape
        out = _mfcc_dct_launch(mel.view(rows * T, n_mels), dct, 1, None, 1, -1.0)
    else:
        # amplitude_to_DB's cut-off groups: the mel tensor is (..., C?, n_mels, T); one cut-off per
        # leading item of its (-1, C, n_mels, T) view (functional.py:393-402)
        packed = waveform.shape[-2] if waveform.dim() > 1 else 1
        n_rows = 1
        for d in lead:
            n_rows *= d
        n_groups = max(n_rows // max(packed, 1), 1)
        st = fused_state
        if st is not None and power == 2.0 and waveform.is_cuda and waveform.dtype == torch.float32:
            # which path: an explicit True, a hook (all ranks alike) or a capture in progress (no host read possible) run the
            # one-kernel path without deciding anything; "auto" follows the module's decision, taking it on this call if
            # it has not been taken yet (MfccFusedState)
            # (a decision "two-kernel" that HAS been taken is honoured under a hook or a capture as well: only TAKING one needs
            # the host read.  The capture query runs on the waveform's device, not on the current one.)
            with torch.cuda.device(dev):
                capturing = torch.cuda.is_current_stream_capturing()
            undecidable = group_max_hook is not None or capturing
            if st.force or st.decided != "two-kernel":
                out = _mfcc_fused(waveform, window, fb, dct, n_fft, hop_length, pad, normalized, center, pad_mode, top_db,
                                  db, packed, n_groups, group_max_hook, st)
                if out is not None:
                    redo = False
                    if not st.force and not undecidable and st.decided is None and out.numel():
                        share = float(st.last_count.item()) / max(st.last_tiles, 1)     # the one synchronisation of "auto"
                        st.decided_share = share
                        st.decided = "fused" if share <= st.max_share else "two-kernel"
                        redo = st.decided == "two-kernel"
                    if not redo:
                        st.path = "fused"
                        st.calls_fused += 1
                        return out.view(lead + (out.shape[1], n_mfcc)).transpose(-1, -2)
        if fused_state is not None:
            fused_state.path = "two-kernel"
            fused_state.calls_two_kernel += 1
        gmax = _neg_inf.take(n_groups, dev)
        mel = _melspectrogram(waveform, pad, window, fb, n_fft, hop_length, win_length, power, normalized, center,
                              pad_mode, db=(db[0], db[1], db[2], gmax, max(packed, 1)))
        rows, T, n_mels = mel.shape
        if group_max_hook is not None:
            group_max_hook(gmax)
        out = _mfcc_dct_launch(mel.view(rows * T, n_mels), dct, 2, gmax, max(packed, 1) * max(T, 1), float(top_db))
    return out.view(lead + (T, n_mfcc)).transpose(-1, -2)


def _melspectrogram_module(waveform: Tensor, window: Tensor, fb: Tensor, pad: int, n_fft: int, hop_length: int, win_length: int,
                           power, normalized, center: bool, pad_mode: str, plans: Optional[dict] = None) -> Tensor:
    """``transforms.MelSpectrogram.forward`` as a function of the module's buffers and constants (reference:
    transforms/_transforms.py:612-622) -- the module calls it with its own plan dictionary, the scripted module reaches it
    through `audio_amd::mel_spectrogram` with the shared one: the same launches either way."""
    if waveform.dtype in LOW_PRECISION:
        # float16 / bfloat16 waveforms (the reference takes any floating dtype and returns it): the n_fft = 400 kernel reads
        # them as they are (conversion in its load); every other shape, and training, widens first.  float32 arithmetic.
        if not (torch.is_grad_enabled() and waveform.requires_grad) and not _learnable(window, fb):
            out = _melspectrogram_lowp(waveform, pad, window, fb, n_fft, hop_length, win_length, power, normalized, center,
                                       pad_mode)
            if out is not None:
                return out.view(tuple(waveform.shape[:-1]) + out.shape[-2:]).transpose(-1, -2).to(waveform.dtype)
        return _melspectrogram_module(waveform.float(), window, fb, pad, n_fft, hop_length, win_length, power, normalized,
                                      center, pad_mode, plans).to(waveform.dtype)
    if (waveform.dtype == torch.float64 and waveform.is_cuda) or _learnable(window, fb):
        # (a learnable window / filterbank: the same composition; gradients flow into both, as in the reference)
        # precision path: the reference composition (_transforms.py:612-622) over the float64 STFT kernels
        return mel_scale(spectrogram(waveform, pad, window, n_fft, hop_length, win_length, power, normalized, center, pad_mode,
                                     True), fb)
    if torch.is_grad_enabled() and waveform.requires_grad:
        # training mode: the same fused forward launch; backward = filterbank transpose, spectrum cotangent and
        # STFT adjoint, all HIP kernels (_MelSpectrogramFunction)
        if power is None:
            raise ValueError("audio_amd: MelSpectrogram needs a real power (got None)")
        out = _MelSpectrogramFunction.apply(_rows2d(waveform), window, fb,
                                            (pad, n_fft, hop_length, win_length, power, normalized, center, pad_mode))
        return out.view(tuple(waveform.shape[:-1]) + out.shape[-2:]).transpose(-1, -2)
    # steady-state serving: the argument tuple of the boxed op is a function of (shape, strides, device, buffers) only
    if plans is None:
        plans = _SHARED_MEL_PLANS
    key = (waveform.shape, waveform.stride(), waveform.dtype, waveform.device, window.data_ptr(), window._version,
           fb.data_ptr(), fb._version, _ROUTE["ops"] is not None,
           n_fft, hop_length, win_length, pad, power, normalized, center, pad_mode)
    plan = plans.get(key)
    if plan is None:
        plan = _melspectrogram_plan(waveform, pad, window, fb, n_fft, hop_length, win_length, power, normalized, center,
                                    pad_mode) or False
        if len(plans) > 64:
            plans.clear()
        plans[key] = plan
    if plan:
        op, shape2, args, _keep = plan
        out = op(waveform.view(shape2), *args)
    else:
        out = _melspectrogram(waveform, pad, window, fb, n_fft, hop_length, win_length, power, normalized, center,
                              pad_mode)                               # (rows, T, n_mels)
    return out.view(tuple(waveform.shape[:-1]) + out.shape[-2:]).transpose(-1, -2)


_SHARED_MEL_PLANS: dict = {}      # launch plans of calls that arrive without a module (scripted programs, audio_amd::mel_spectrogram)

# "auto" decisions of MFCC modules, by handle.  An eager module and every scripted copy of it carry the same integer, so they
# share ONE decision and return the same bits; a scripted module loaded into a fresh process finds no state under its handle
# and decides again at its first eligible call.
_MFCC_STATES: dict = {}
_MFCC_STATES_LOCK = threading.Lock()


def _mfcc_state_of(handle: int) -> "MfccFusedState":
    with _MFCC_STATES_LOCK:
        st = _MFCC_STATES.get(handle)
        if st is None:
            if len(_MFCC_STATES) > 4096:               # handles of modules long gone: forget the oldest half
                for k in list(_MFCC_STATES)[:2048]:
                    del _MFCC_STATES[k]
            st = _MFCC_STATES[handle] = MfccFusedState()
        return st


def _mfcc_module(waveform: Tensor, window: Tensor, fb: Tensor, dct_mat: Tensor, pad: int, n_fft: int, hop_length: int,
                 win_length: int, power, normalized, center: bool, pad_mode: str, log_mels: bool, top_db: float,
                 db=(10.0, 1e-10, 0.0), fused=2, state: Optional["MfccFusedState"] = None, group_max_hook=None,
                 mel_plans: Optional[dict] = None) -> Tensor:
    """``transforms.MFCC.forward`` as a function of the module's buffers and constants (reference:
    transforms/_transforms.py:692-709).  ``fused``: 0 = the exact two-kernel path, 1 = always the one-kernel path, 2 = "auto"
    (the decision lives in ``state``)."""
    n_mfcc = dct_mat.shape[1]
    if waveform.dtype in LOW_PRECISION:         # float16 / bfloat16: float32 arithmetic, the input dtype back
        return _mfcc_module(waveform.float(), window, fb, dct_mat, pad, n_fft, hop_length, win_length, power, normalized, center,
                            pad_mode, log_mels, top_db, db, fused, state, group_max_hook, mel_plans).to(waveform.dtype)
    if (torch.is_grad_enabled() and waveform.requires_grad) or (waveform.dtype == torch.float64 and waveform.is_cuda) or \
            _learnable(window, fb, dct_mat):
        # differentiable / float64 path (reference composition, _transforms.py:692-709, on top of the
        # differentiable mel spectrogram): the dB / top_db / DCT tail is cheap and torch's autograd
        # reproduces the reference's sub-gradients (clamp, amax) exactly
        if waveform.numel() == 0 and group_max_hook is not None and not log_mels:
            # an empty shard still joins the exchange of the batch-global cut-off (the other ranks wait in it): one -inf per
            # cut-off group, counted as _mfcc counts them, and the frame count every other path takes from the descriptor
            # (`1 + L // hop` only held for center=True, pad=0)
            packed = waveform.shape[-2] if waveform.dim() > 1 else 1
            n_rows = 1
            for d in waveform.shape[:-1]:
                n_rows *= d
            n_groups = max(n_rows // max(packed, 1), 1)
            group_max_hook(torch.full((n_groups,), float("-inf"), dtype=waveform.dtype, device=waveform.device))
            T_ = max(_host.frame_count(waveform.shape[-1], n_fft, hop_length, center, pad), 0)
            return waveform.new_zeros(tuple(waveform.shape[:-1]) + (n_mfcc, T_))
        mel = _melspectrogram_module(waveform, window, fb, pad, n_fft, hop_length, win_length, power, normalized, center,
                                     pad_mode, mel_plans)
        if log_mels:
            mel = torch.log(mel + 1e-6)
        else:
            multiplier, amin, db_multiplier = db
            x_db = multiplier * torch.log10(torch.clamp(mel, min=amin)) - multiplier * db_multiplier
            shp = x_db.size()
            packed = shp[-3] if x_db.dim() > 2 else 1
            x_db = x_db.reshape(-1, packed, shp[-2], shp[-1])
            gmax = x_db.amax(dim=(-3, -2, -1))
            if group_max_hook is not None:
                # sharded batch (audio_amd.distributed): the cut-off is the maximum over ALL ranks' shards.  The exchange
                # runs on a detached copy in the path's own dtype; where another rank holds the maximum it enters as a
                # constant -- its sub-gradient belongs to that rank's element -- and where this rank holds it the
                # reference's amax sub-gradient is kept (this branch used per-shard cut-offs)
                g_all = gmax.detach().clone()
                group_max_hook(g_all)
                gmax = torch.where(g_all > gmax, g_all, gmax)      # (a tie keeps the local amax and its whole sub-gradient)
            x_db = torch.max(x_db, (gmax - top_db).view(-1, 1, 1, 1))
            mel = x_db.reshape(shp)
        return torch.matmul(mel.transpose(-1, -2), dct_mat.to(device=mel.device, dtype=mel.dtype)).transpose(-1, -2)
    st = None
    if fused != 0:
        st = state if state is not None else MfccFusedState()
        st.force = fused == 1        # 1: always one kernel; 2: the "auto" decision held by the state
    return _mfcc(waveform, pad, window, fb, dct_mat, n_fft, hop_length, win_length, power, normalized, center, pad_mode,
                 log_mels, top_db, db=db, group_max_hook=group_max_hook, fused_state=st)


def _dct_rows(x: Tensor, dct: Tensor) -> Tensor:
    """(n_vec, n_in) @ (n_in, n_out) on the MFCC path's matrix-core DCT kernel (log_mode 2 without a cut-off =
    plain product).  Used by compliance.kaldi.mfcc."""
    return _mfcc_dct_launch(x, dct, 2, None, 1, -1.0)


@_reduced_precision_io
def _mel_scale_eager(specgram: Tensor, fb: Tensor) -> Tensor:
    """MelScale.forward (transforms/_transforms.py:403-415): (..., freq, time) -> (..., n_mels, time)."""
    if specgram.is_cuda and (specgram.dtype == torch.float64 or
                             (torch.is_grad_enabled() and (specgram.requires_grad or fb.requires_grad))):
        # precision / training path of this thin caller: the reference's own product, differentiable to any order in the
        # spectrogram AND in a learnable filterbank (_transforms.py:413: the reference propagates into `fb` through matmul)
        # (the fused MelSpectrogram kernel is the throughput path; test: transforms/autograd_test_impl.py test_melscale)
        return torch.matmul(specgram.transpose(-1, -2), fb.to(device=specgram.device, dtype=specgram.dtype)).transpose(-1, -2)
    _require_device(specgram, "specgram")
    shape = specgram.shape
    n_freq, T = shape[-2], shape[-1]
    if n_freq != fb.shape[0]:
        raise RuntimeError(
            f"mat1 and mat2 shapes cannot be multiplied ({T}x{n_freq} and {fb.shape[0]}x{fb.shape[1]})")
    fm = specgram.transpose(-1, -2).reshape(-1, T, n_freq)
    if not fm.is_contiguous():
        fm = fm.contiguous()
    bands = _mel_bands(fb, specgram.device)
    ops = _ops()
    if ops is not None and fm.numel():
        out = ops.mel_scale(fm, bands.lo, bands.width, bands.weights)
        return out.view(tuple(shape[:-2]) + (T, bands.n_mels)).transpose(-1, -2)
    out = torch.empty((fm.shape[0], T, bands.n_mels), dtype=torch.float32, device=specgram.device)
    if out.numel():
        L = _lib.lib()
        _lib.check(L.aamd_mel_scale_f32(fm.data_ptr(), C.byref(bands.struct), out.data_ptr(), fm.shape[0], T,
                                        n_freq, _lib.current_stream(specgram.device)))
    return out.view(tuple(shape[:-2]) + (T, bands.n_mels)).transpose(-1, -2)


# --------------------------------------------------------------------------- #
# dB                                                                          #
# --------------------------------------------------------------------------- #


@_reduced_precision_io
def _amplitude_to_DB_eager(x: Tensor, multiplier: float, amin: float, db_multiplier: float,
                    top_db: Optional[float] = None) -> Tensor:
    r"""Power/amplitude -> decibel (functional/functional.py:356-404).  With ``top_db`` the cut-off
    is per leading item of the ``(-1, C, F, T)`` view, ``C = shape[-3]`` if ``x.dim() > 2`` else 1."""
    if x.is_cuda and (x.dtype == torch.float64 or (torch.is_grad_enabled() and x.requires_grad)):
        # precision / training path: the reference's element-wise formula (functional.py:390-402), so that autograd
        # reproduces its clamp / amax sub-gradients to any order (test: autograd_test_impl.py test_amplitude_to_db)
        x_db = multiplier * torch.log10(torch.clamp(x, min=amin))
        x_db = x_db - multiplier * db_multiplier
        if top_db is not None:
            shape = x_db.size()
            packed_channels = shape[-3] if x_db.dim() > 2 else 1
            x_db = x_db.reshape(-1, packed_channels, shape[-2], shape[-1])
            x_db = torch.max(x_db, (x_db.amax(dim=(-3, -2, -1)) - top_db).view(-1, 1, 1, 1))
            x_db = x_db.reshape(shape)
        return x_db
    _require_device(x, "x")
    # The op is element-wise plus a maximum over whole (C, F, T) blocks, so it runs in MEMORY order: the frame-major
    # tensors Spectrogram / MelSpectrogram / MelScale return ((..., F, T) views of (..., T, F) storage) are processed
    # as they lie and come back with the same strides -- what the reference's element-wise ops do -- instead of
    # paying a transposing copy first.
    if not x.is_contiguous() and x.dim() >= 2 and x.transpose(-1, -2).is_contiguous():
        return amplitude_to_DB(x.transpose(-1, -2), multiplier, amin, db_multiplier, top_db).transpose(-1, -2)
    xc = x if x.is_contiguous() else x.contiguous()
    n = xc.numel()
    out = torch.empty_like(xc)
    L = _lib.lib()
    stream = _lib.current_stream(x.device)
    if n == 0:
        return out.view(x.shape)
    if top_db is None:
        _lib.check(L.aamd_amplitude_to_db_f32(xc.data_ptr(), out.data_ptr(), n, multiplier, amin, db_multiplier,
                                              None, 1, stream))
        return out.view(x.shape)
    shape = x.shape
    packed = shape[-3] if x.dim() > 2 else 1
    group = packed * shape[-2] * shape[-1]
    n_groups = n // group
    gmax = _neg_inf.take(n_groups, x.device)
    # pass 1: group maxima only (reads x, writes nothing); pass 2: dB + clamp + store
    _lib.check(L.aamd_amplitude_to_db_f32(xc.data_ptr(), None, n, multiplier, amin, db_multiplier, gmax.data_ptr(), group,
                                          stream))
    _lib.check(L.aamd_amplitude_to_db_clamped_f32(xc.data_ptr(), out.data_ptr(), n, multiplier, amin, db_multiplier,
                                                  gmax.data_ptr(), group, float(top_db), stream))
    return out.view(shape)


# --------------------------------------------------------------------------- #
# resample                                                                    #
# --------------------------------------------------------------------------- #


_SPARSE_TAPS = 4096      # polyphase tables with longer rows are evaluated sparsely (they are > 99 % zeros)


def _polyphase(x2: Tensor, kern: Tensor, key_tensor: Tensor, key, orig: int, new: int, width: int) -> Tensor:
    """(rows, L) -> (rows, ceil(new L / orig)) through aamd_resample_banded_f32; band table cached per tensor."""
    rows, length = x2.shape
    out_len = int(math.ceil(new * length / orig))
    if x2.dtype == torch.float64:
        x2 = x2.contiguous()
        out = torch.empty((rows, out_len), dtype=torch.float64, device=x2.device)
        if out.numel():
            with torch.cuda.device(x2.device):
                _lib.check(_lib.lib().aamd_resample_f64(x2.data_ptr(), kern.data_ptr(), out.data_ptr(), rows, length,
                                                       max(length, 1), orig, new, width, out_len,
                                                       _lib.current_stream(x2.device)))
        return out
    if kern.shape[1] > _SPARSE_TAPS:
        # huge reduced rates (PitchShift: 10079 : 8000 -> a 8000 x 10095 table with ~36 live taps per phase): the
        # compacted table (host, once per kernel tensor) through the sparse kernel instead of 10 095 taps per sample
        hb, lo, span = _tensor_cached(key_tensor, ("rs_sparse", key, new, str(x2.device)), lambda: tuple(
            (torch.from_numpy(t).to(x2.device) if isinstance(t, np.ndarray) else t)
            for t in _host.resample_sparse_table(kern.cpu().numpy())))
        if x2.stride(0) != length and rows > 1:
            x2 = x2.contiguous()
        out = torch.empty((rows, out_len), dtype=torch.float32, device=x2.device)
        if out.numel():
            with torch.cuda.device(x2.device):
                _lib.check(_lib.lib().aamd_resample_sparse_f32(
                    x2.data_ptr(), hb.data_ptr(), lo.data_ptr(), out.data_ptr(), rows, length, max(length, 1), orig, new,
                    width, int(span), out_len, _lib.current_stream(x2.device)))
        return out
    # few output phases (48 k -> 16 k has ONE): the same filter for the pair (m orig : m new), whose m new phases fill the
    # 16-phase tiles of the matrix-core kernel (host, once per kernel tensor; same outputs in the same order)
    def _fill():
        kp, mm = _host.resample_fill_phase_tiles(kern.cpu().numpy(), orig, new, width)
        return (kern if mm == 1 else torch.from_numpy(np.ascontiguousarray(kp)).to(x2.device)), mm

    kern_m, m = _tensor_cached(key_tensor, ("rs_fill", key, orig, new, width, str(x2.device)), _fill)
    if m > 1:
        kern, orig, new = kern_m, m * orig, m * new
    # band table of the taps (host, once per kernel tensor): the matrix-core kernel skips the
    # ~1e-20-sized window tails outside each phase tile's band
    tap_lo, span = _tensor_cached(key_tensor, ("rs_bands", key, new),
                                  lambda: _host.resample_band_table(kern.cpu().numpy()))
    ops = _ops()
    lo_list = _tensor_cached(key_tensor, ("rs_bands_list", key, new), lambda: [int(v) for v in tap_lo])
    # prepared tap fragments of the binary16-split matrix-core kernel (C ABI 7): the packed (hi, lo) operands of the filter, built
    # once per kernel tensor instead of in every workgroup's prologue (13 % of a BASELINE config-3 launch).  Built on the current
    # stream and synchronised once, so that any later stream may read them; not under graph capture (memory of a capture's
    # private pool must not outlive the graph): such a call forms the fragments in the kernel, with identical results
    frag = None
    with torch.cuda.device(x2.device):               # (the capture status is per device: ask the one the data lives on)
        capturing = torch.cuda.is_current_stream_capturing()
    if _host._rs_pick_ks(int(span)) != 0 and not capturing:
        def _frag():
            L = _lib.lib()
            bands = _lib.ResampleBands(tap_lo.shape[0], span, tap_lo.ctypes.data_as(C.POINTER(C.c_int32)))
            with torch.cuda.device(x2.device):
                if ops is not None:
                    t = ops.resample_frag_build(kern, orig, new, width, lo_list, int(span))
                else:
                    nb = int(L.aamd_resample_frag_bytes(orig, new, C.byref(bands)))
                    t = torch.empty((nb // 4,), dtype=torch.float32, device=x2.device)
                    _lib.check(L.aamd_resample_frag_build_f32(kern.data_ptr(), orig, new, width, C.byref(bands), t.data_ptr(),
                                                              _lib.current_stream(x2.device)))
                # later calls may run on other streams: they wait for this event (device-side) until it has completed -- the host
                # is not blocked (a blocking synchronize here cost a pipeline bubble per new tap table)
                ev = torch.cuda.Event()
                ev.record(torch.cuda.current_stream(x2.device))
            return [t, ev, _lib.current_stream(x2.device)]
        ent = _tensor_cached(key_tensor, ("rs_frag", key, orig, new, width, str(x2.device)), _frag)
        frag = ent[0]
        if ent[1] is not None:
            if ent[1].query():
                ent[1] = None                       # built long ago: nothing to order any more
            elif _lib.current_stream(x2.device) != ent[2]:
                torch.cuda.current_stream(x2.device).wait_event(ent[1])
    if ops is not None:
        if x2.stride(0) != length and rows > 1:
            x2 = x2.contiguous()
        return ops.resample(x2, kern, orig, new, width, out_len, lo_list, int(span), frag)
    out = torch.empty((rows, out_len), dtype=torch.float32, device=x2.device)
    if out.numel():
        L = _lib.lib()
        bands = _lib.ResampleBands(tap_lo.shape[0], span, tap_lo.ctypes.data_as(C.POINTER(C.c_int32)))
        _lib.check(L.aamd_resample_prepared_f32(x2.data_ptr(), kern.data_ptr(), out.data_ptr(), rows, length,
                                                x2.stride(0) if rows > 1 else max(length, 1), orig, new, width,
                                                out_len, C.byref(bands), None if frag is None else frag.data_ptr(),
                                                _lib.current_stream(x2.device)))
    return out


class _ResampleFunction(torch.autograd.Function):
    """Resampling is linear in the waveform; its adjoint is again a polyphase filter with the two rates
    swapped and the tap table re-indexed (`_host.resample_adjoint_table`), so the backward pass is one
    more launch of the same matrix-core kernel.  The tap table is a constant (no gradient), as in the
    reference's gradcheck (test/torchaudio_unittest/functional/autograd_impl.py)."""

    @staticmethod
    def forward(ctx, x2, kern, kernel_key, orig, new, width):
        ctx.kern, ctx.kernel_key, ctx.geom, ctx.length = kern, kernel_key, (orig, new, width), x2.shape[1]
        return _polyphase(x2, kern, kernel_key, "fwd", orig, new, width)

    @staticmethod
    def backward(ctx, dy):
        orig, new, width = ctx.geom
        adj = _tensor_cached(ctx.kernel_key, ("rs_adjoint", orig, new, width), lambda: tuple(
            (torch.from_numpy(t).to(dy.device) if isinstance(t, np.ndarray) else t)
            for t in _host.resample_adjoint_table(ctx.kern.cpu().numpy(), orig, new, width)))
        kern_adj, width_adj = adj
        if torch.is_grad_enabled():      # create_graph=True: the adjoint is the same kind of operator -- apply it differentiably
            dx = _ResampleFunction.apply(dy.contiguous(), kern_adj, kern_adj, new, orig, int(width_adj))
        else:
            dx = _polyphase(dy.contiguous(), kern_adj, kern_adj, "adj", new, orig, int(width_adj))
        return dx[:, :ctx.length], None, None, None, None, None


@_reduced_precision_io
def _apply_sinc_resample_kernel_eager(waveform: Tensor, orig_freq: int, new_freq: int, gcd: int, kernel: Tensor,
                                width: int) -> Tensor:
    """functional/functional.py:1405-1432 as one polyphase HIP kernel (differentiable in the waveform)."""
    if not waveform.is_floating_point():
        raise TypeError(f"Expected floating point type for waveform tensor, but received {waveform.dtype}.")
    _require_device(waveform, "waveform", allow_grad=True, allow_f64=True)
    orig = int(orig_freq) // gcd
    new = int(new_freq) // gcd
    shape = waveform.size()
    x2 = _rows2d(waveform)
    kern = kernel.to(device=waveform.device, dtype=waveform.dtype).reshape(new, -1).contiguous()
    if kern.shape[1] != 2 * width + orig:
        raise RuntimeError("audio_amd: resample kernel shape does not match (new, 2*width+orig)")
    if torch.is_grad_enabled() and kernel.requires_grad:
        # a learnable tap table (the reference propagates into it through conv1d, functional.py:1419-1431)
        out = _diff.resample_learnable_kernel(x2, kernel.to(device=waveform.device, dtype=waveform.dtype).reshape(new, -1),
                                              orig, new, width)
    elif torch.is_grad_enabled() and waveform.requires_grad:
        out = _ResampleFunction.apply(x2, kern, kernel, orig, new, width)
    else:
        out = _polyphase(x2, kern, kernel, "fwd", orig, new, width)
    return out.view(tuple(shape[:-1]) + (out.shape[-1],))


@_reduced_precision_io
def _resample_eager(
    waveform: Tensor,
    orig_freq: int,
    new_freq: int,
    lowpass_filter_width: int = 6,
    rolloff: float = 0.99,
    resampling_method: str = "sinc_interp_hann",
    beta: Optional[float] = None,
) -> Tensor:
    r"""Band-limited sinc-interpolation resampling (functional/functional.py:1435-1490).  The tap
    table is evaluated on the host in the waveform's dtype exactly as the reference's CPU path
    does per call (cached here per parameter set) and applied by the polyphase HIP kernel."""
    if orig_freq <= 0.0 or new_freq <= 0.0:
        raise ValueError("Original frequency and desired frequecy should be positive")
    if orig_freq == new_freq:
        return waveform
    gcd = math.gcd(int(orig_freq), int(new_freq))
    key = ("sinc", int(orig_freq), int(new_freq), lowpass_filter_width, rolloff, resampling_method, beta,
           str(waveform.dtype), str(waveform.device))
    def make():
        k, w = _host.sinc_resample_kernel(orig_freq, new_freq, gcd, lowpass_filter_width, rolloff, resampling_method,
                                          beta, dtype=waveform.dtype)
        return k.to(waveform.device), w

    kernel, width = _cached(key, make)
    return _apply_sinc_resample_kernel(waveform, orig_freq, new_freq, gcd, kernel, width)


# --------------------------------------------------------------------------- #
# lfilter / biquad                                                            #
# --------------------------------------------------------------------------- #


def _lfilter_launch(x3: Tensor, a: Tensor, b: Tensor, clamp: bool, n_stages: int = 1) -> Tensor:
    """x3: (batch, channels, L) contiguous; a, b: (n_stages, rows, n_order)."""
    batch, channels, length = x3.shape
    if x3.dtype == torch.float64:
        if n_stages != 1:
            raise NotImplementedError("audio_amd: float64 lfilter runs one stage per call")
        y = torch.empty_like(x3)
        if y.numel():
            with torch.cuda.device(x3.device):
                _lib.check(_lib.lib().aamd_lfilter_f64(x3.data_ptr(), a.data_ptr(), b.data_ptr(), y.data_ptr(), batch,
                                                      channels, length, a.shape[-1], a.shape[-2], 1, int(clamp),
                                                      _lib.current_stream(x3.device)))
        return y
    ops = _ops()
    if ops is not None:
        return ops.lfilter(x3, a.reshape(n_stages, -1, a.shape[-1]), b.reshape(n_stages, -1, b.shape[-1]), n_stages,
                           int(clamp))
    y = torch.empty_like(x3)
    if y.numel():
        L = _lib.lib()
        _lib.check(L.aamd_lfilter_f32(x3.data_ptr(), a.data_ptr(), b.data_ptr(), y.data_ptr(), batch, channels,
                                      length, a.shape[-1], a.shape[-2], n_stages, int(clamp),
                                      _lib.current_stream(x3.device)))
    return y


def _lfilter_any(x3: Tensor, a_n: Tensor, b_n: Tensor, sos) -> Tensor:
    """Unclamped filter of (batch, rows, L) by the (rows, n_order) coefficients: the host-vouched second-order sections
    `sos` on the cascade kernels when the caller has them, else the general-order kernel (float64 state, csrc/lfilter.h)."""
    if sos is not None:
        return _lfilter_launch(x3, sos[0], sos[1], 0, n_stages=sos[0].shape[0])
    return _lfilter_launch(x3, a_n.unsqueeze(0), b_n.unsqueeze(0), False)


class _LFilterFunction(torch.autograd.Function):
    """Autograd of lfilter on the HIP kernels (reference: DifferentiableFIR / DifferentiableIIR,
    functional/filtering.py:941-1024).  With w = FIR(x; b^) and y = IIR(w; a^), both LTI:
      dL/dx   = time-reversed lfilter(a^, b^) of the time-reversed dL/dy      (one kernel launch)
      dL/dw   = time-reversed all-pole filter 1/A of the time-reversed dL/dy  (one kernel launch)
      dL/db^k = sum_n dL/dw[n] x[n-k],   dL/da^k = -sum_n dL/dw[n] y[n-k]  (k >= 1; a^0 = 1 is not a parameter)
    clamp(-1, 1) passes gradient where the unclamped output lies inside [-1, 1] (torch.clamp's rule).
    `sos`: second-order sections of (a^, b^) for a FIXED filter under a differentiable waveform (the forward and the dx
    launch then run on the cascade kernels); learnable coefficients change every step and take the general-order kernel."""

    @staticmethod
    def forward(ctx, x3, a_n, b_n, clamp, sos=None):
        a_n = a_n.contiguous()
        b_n = b_n.contiguous()
        y_raw = _lfilter_any(x3, a_n, b_n, sos)
        ctx.save_for_backward(x3, a_n, b_n, y_raw)
        ctx.clamp = clamp
        ctx.sos = sos
        return y_raw.clamp(-1.0, 1.0) if clamp else y_raw

    @staticmethod
    def backward(ctx, dy):
        x3, a_n, b_n, y = ctx.saved_tensors
        sos = ctx.sos
        g = dy
        if ctx.clamp:
            g = g * ((y >= -1.0) & (y <= 1.0)).to(g.dtype)
        gf = g.flip(-1).contiguous()
        # Under create_graph=True (gradgradcheck) every piece below must itself be differentiable: the adjoint filters are
        # then applied through this very Function (as the reference's DifferentiableIIR.backward calls
        # DifferentiableIIR.apply, filtering.py:1000-1017) and `y` is the graph-connected output it saved.
        if torch.is_grad_enabled():
            run = lambda t, aa, bb, ss=None: _LFilterFunction.apply(t, aa, bb, False, ss)        # noqa: E731
            y = run(x3, a_n, b_n, sos)   # graph-connected copy of the unclamped output (da below depends on it)
        else:
            run = lambda t, aa, bb, ss=None: _lfilter_any(t, aa, bb, ss)                         # noqa: E731
        dx = da = db = None
        if ctx.needs_input_grad[0]:
            dx = run(gf, a_n, b_n, sos).flip(-1)
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            one = torch.zeros_like(b_n)
            one[:, 0] = 1.0
            dw = run(gf, a_n, one).flip(-1)
            n_order, L = a_n.shape[1], x3.shape[-1]
            if ctx.needs_input_grad[2]:
                db = torch.stack([(dw[..., k:] * x3[..., :L - k]).sum((0, 2)) for k in range(n_order)], 1)
            if ctx.needs_input_grad[1]:
                cols = [torch.zeros(a_n.shape[0], dtype=a_n.dtype, device=a_n.device)]
                cols += [-(dw[..., k:] * y[..., :L - k]).sum((0, 2)) for k in range(1, n_order)]
                da = torch.stack(cols, 1)
        return dx, da, db, None, None


_SOS_MIN_SAMPLES = 0            # every size: the sections are the FAST form (biquad-class kernels); accuracy no longer depends
                                # on them -- the general-order kernel carries its state in float64 since round 3
_SOS_MAX_COEFFS = 17            # order <= 16 = 8 sections, what one launch of the cascade kernels takes
_SOS_BY_VALUE: dict = {}        # coefficient bytes -> sections (host arrays) or None: callers that rebuild their tensors per call
_SOS_ENABLED = [os.environ.get("AAMD_LFILTER_NO_SECTIONS") is None]


def set_lfilter_sections(enabled: bool) -> bool:
    """Switch the host factorisation of orders 3 .. 16 into second-order sections on or off (returns the previous
    setting).  Factoring needs the coefficient VALUES on the host: one blocking device-to-host copy per new coefficient
    tensor pair (plus root finding on a value miss) -- callers that build coefficients on the device every call, or capture
    HIP graphs, switch it off and stay on the general-order kernel, which needs nothing from the host."""
    prev = _SOS_ENABLED[0]
    _SOS_ENABLED[0] = bool(enabled)
    return prev


def _lfilter_sections(a_key: Tensor, b_key: Tensor, a: Tensor, b: Tensor):
    """Second-order sections (device tensors (n_sections, rows, 3)) of the order 3 .. 16 filter (a, b), or None when
    `_host.lfilter_sos` does not vouch for the factorisation.  Cached per coefficient tensor (no host round trip on a hit)
    and per coefficient values (one device-to-host copy, no root finding, for callers that rebuild the tensors)."""
    def make():
        ah, bh = a.detach().cpu().numpy(), b.detach().cpu().numpy()
        key = (ah.shape, ah.tobytes(), bh.tobytes())
        with _CACHE_LOCK:
            hit = key in _SOS_BY_VALUE
            sec = _SOS_BY_VALUE.get(key)
        if not hit:
            sec = _host.lfilter_sos(ah, bh)
            with _CACHE_LOCK:
                if len(_SOS_BY_VALUE) > 256:
                    _SOS_BY_VALUE.clear()
                _SOS_BY_VALUE[key] = sec
        if sec is None:
            return (None, None, weakref.ref(b_key))
        return (torch.from_numpy(sec[0]).to(a.device), torch.from_numpy(sec[1]).to(a.device), weakref.ref(b_key))

    # The slot lives on `a_key` (weakref-checked by _tensor_cached); `b_key` is identified by a weak reference stored IN the
    # entry -- never by id() / data_ptr(), which CPython and the allocator reuse for a fresh tensor with other values.
    k = ("lf_sos", b_key._version, b_key.data_ptr(), str(a.device))
    got = _tensor_cached(a_key, k, make)
    if got[2]() is not b_key:
        got = _tensor_cached(a_key, k, make, replace=True)
    return None if got[0] is None else got[:2]


@_reduced_precision_io
def _lfilter_eager(waveform: Tensor, a_coeffs: Tensor, b_coeffs: Tensor, clamp: bool = True, batching: bool = True) -> Tensor:
    r"""IIR filter by the difference equation (functional/filtering.py:1032-1099): FIR + recursion
    + clamp in one HIP kernel (chunked linear-recurrence scan, see csrc/lfilter.h)."""
    if a_coeffs.size() != b_coeffs.size():
        raise ValueError(
            "Expected coeffs to be the same size."
            f"Found: a_coeffs size: {a_coeffs.size()}, b_coeffs size: {b_coeffs.size()}"
        )
    if a_coeffs.ndim > 2:
        raise ValueError(f"Expected coeffs to have greater than 1 dimension. Found: {a_coeffs.ndim}")
    a_key, b_key = a_coeffs, b_coeffs            # the caller's tensor objects: cache slots for what is derived from them
    if a_coeffs.ndim > 1:
        if batching:
            if waveform.ndim <= 0:
                raise ValueError("Expected waveform to have a positive number of dimensions." f"Found: {waveform.ndim}")
            if waveform.shape[-2] != a_coeffs.shape[0]:
                raise ValueError(
                    "Expected number of batches in waveform and coeffs to be the same."
                    f"Found: coeffs batches: {a_coeffs.shape[0]}, waveform batches: {waveform.shape[-2]}"
                )
        else:
            waveform = torch.stack([waveform] * a_coeffs.shape[0], -2)
    else:
        a_coeffs = a_coeffs.unsqueeze(0)
        b_coeffs = b_coeffs.unsqueeze(0)
    coeff_grad = torch.is_grad_enabled() and (a_coeffs.requires_grad or b_coeffs.requires_grad)
    needs_grad = coeff_grad or (torch.is_grad_enabled() and waveform.requires_grad)
    _require_device(waveform, "waveform", allow_grad=True, allow_f64=True)
    shape = waveform.size()
    n_filt = a_coeffs.shape[0]
    x3 = waveform.reshape(-1, n_filt, shape[-1]).contiguous()
    a = a_coeffs.to(device=waveform.device, dtype=waveform.dtype).contiguous()
    b = b_coeffs.to(device=waveform.device, dtype=waveform.dtype).contiguous()
    # orders 3 .. 16 with FIXED coefficients: second-order sections on the biquad-class kernels, clamped once at the end
    sos = None
    if (x3.dtype == torch.float32 and 4 <= a.shape[-1] <= _SOS_MAX_COEFFS and x3.numel() >= _SOS_MIN_SAMPLES
            and _SOS_ENABLED[0] and not coeff_grad):
        sos = _lfilter_sections(a_key, b_key, a.detach(), b.detach())
    if needs_grad:
        # differentiable path (functional/filtering.py:941-1029): normalise by a0 with torch ops so that
        # autograd sees the division, the recursion and its adjoint run in the HIP kernels
        y = _LFilterFunction.apply(x3, a / a[:, 0:1], b / a[:, 0:1], clamp, sos)
    elif sos is not None:
        y = _lfilter_launch(x3, sos[0], sos[1], 2 if clamp else 0, n_stages=sos[0].shape[0])
    else:
        y = _lfilter_launch(x3, a, b, clamp)
    return y.reshape(shape[:-1] + y.shape[-1:])


@_reduced_precision_io
def _biquad_cascade_eager(waveform: Tensor, a_coeffs: Tensor, b_coeffs: Tensor, clamp: bool = True) -> Tensor:
    """``n_stages`` sequential ``lfilter`` calls (each clamped like the reference's default) fused in
    ONE pass over the audio.  a_coeffs, b_coeffs: (n_stages, n_order) shared across channels or
    (n_stages, channels, n_order).  Extension of the reference API (BASELINE config 5a)."""
    _require_device(waveform, "waveform")
    if a_coeffs.shape != b_coeffs.shape or a_coeffs.ndim not in (2, 3):
        raise ValueError("biquad_cascade: a_coeffs and b_coeffs must both be (stages, order+1) or (stages, channels, order+1)")
    shape = waveform.size()
    a = a_coeffs.to(device=waveform.device, dtype=torch.float32)
    b = b_coeffs.to(device=waveform.device, dtype=torch.float32)
    if a.ndim == 2:
        a, b = a.unsqueeze(1), b.unsqueeze(1)
        x3 = waveform.reshape(-1, 1, shape[-1]).contiguous()
    else:
        if waveform.ndim < 2 or waveform.shape[-2] != a.shape[1]:
            raise ValueError("biquad_cascade: waveform channel dim does not match coefficient rows")
        x3 = waveform.reshape(-1, a.shape[1], shape[-1]).contiguous()
    y = _lfilter_launch(x3, a.contiguous(), b.contiguous(), clamp, n_stages=a.shape[0])
    return y.reshape(shape)


def _cpu_scalar(v, dtype) -> Tensor:
    """0-dim CPU tensor of the waveform dtype (the reference builds its coefficients with
    ``torch.as_tensor(v, dtype=waveform.dtype)`` scalars; doing it on the host avoids launches)."""
    if isinstance(v, Tensor):
        if v.requires_grad and torch.is_grad_enabled():
            return v.to(device="cpu", dtype=dtype).reshape(())     # a learnable filter parameter: stay on the graph
        return v.detach().to(device="cpu", dtype=dtype).reshape(())
    return torch.as_tensor(v, dtype=dtype)


def _biquad_eager(waveform: Tensor, b0: float, b1: float, b2: float, a0: float, a1: float, a2: float) -> Tensor:
    r"""Biquad filter (functional/filtering.py:295-333): ``lfilter`` with 3-tap a, b."""
    dtype = waveform.dtype
    coef = torch.stack([_cpu_scalar(v, dtype) for v in (a0, a1, a2, b0, b1, b2)]).to(waveform.device)
    return lfilter(waveform, coef[:3], coef[3:])


@_reduced_precision_io
def _filtfilt_eager(waveform: Tensor, a_coeffs: Tensor, b_coeffs: Tensor, clamp: bool = True) -> Tensor:
    r"""Forward-backward IIR filtering (functional/filtering.py:672-711)."""
    fwd = lfilter(waveform, a_coeffs, b_coeffs, clamp=False, batching=True)
    bwd = lfilter(fwd.flip(-1), a_coeffs, b_coeffs, clamp=clamp, batching=True).flip(-1)
    return bwd


# ---- biquad designers: RBJ-cookbook coefficient formulas evaluated with 0-dim tensors of the
# ---- waveform dtype (as the reference does), then one call to biquad --------------------- #


def _w0(freq, sample_rate: int, dtype) -> Tensor:
    return 2 * math.pi * _cpu_scalar(freq, dtype) / sample_rate


def _lowpass_biquad_eager(waveform: Tensor, sample_rate: int, cutoff_freq: float, Q: float = 0.707) -> Tensor:
    r"""functional/filtering.py:1102-1133."""
    dt = waveform.dtype
    w0 = _w0(cutoff_freq, sample_rate, dt)
    alpha = torch.sin(w0) / 2 / _cpu_scalar(Q, dt)
    b0 = (1 - torch.cos(w0)) / 2
    return biquad(waveform, b0, 1 - torch.cos(w0), b0, 1 + alpha, -2 * torch.cos(w0), 1 - alpha)


def _highpass_biquad_eager(waveform: Tensor, sample_rate: int, cutoff_freq: float, Q: float = 0.707) -> Tensor:
    r"""functional/filtering.py:893-923."""
    dt = waveform.dtype
    w0 = _w0(cutoff_freq, sample_rate, dt)
    alpha = torch.sin(w0) / 2.0 / _cpu_scalar(Q, dt)
    b0 = (1 + torch.cos(w0)) / 2
    return biquad(waveform, b0, -1 - torch.cos(w0), b0, 1 + alpha, -2 * torch.cos(w0), 1 - alpha)


def _allpass_biquad_eager(waveform: Tensor, sample_rate: int, central_freq: float, Q: float = 0.707) -> Tensor:
    r"""functional/filtering.py:70-101."""
    dt = waveform.dtype
    w0 = _w0(central_freq, sample_rate, dt)
    alpha = torch.sin(w0) / 2 / _cpu_scalar(Q, dt)
    return biquad(waveform, 1 - alpha, -2 * torch.cos(w0), 1 + alpha, 1 + alpha, -2 * torch.cos(w0), 1 - alpha)


def _bandpass_biquad_eager(waveform: Tensor, sample_rate: int, central_freq: float, Q: float = 0.707,
                    const_skirt_gain: bool = False) -> Tensor:
    r"""functional/filtering.py:104-142."""
    dt = waveform.dtype
    w0 = _w0(central_freq, sample_rate, dt)
    alpha = torch.sin(w0) / 2 / _cpu_scalar(Q, dt)
    peak = torch.sin(w0) / 2 if const_skirt_gain else alpha
    return biquad(waveform, peak, 0.0, -peak, 1 + alpha, -2 * torch.cos(w0), 1 - alpha)


def _bandreject_biquad_eager(waveform: Tensor, sample_rate: int, central_freq: float, Q: float = 0.707) -> Tensor:
    r"""functional/filtering.py:145-177."""
    dt = waveform.dtype
    w0 = _w0(central_freq, sample_rate, dt)
    alpha = torch.sin(w0) / 2 / _cpu_scalar(Q, dt)
    return biquad(waveform, 1.0, -2 * torch.cos(w0), 1.0, 1 + alpha, -2 * torch.cos(w0), 1 - alpha)


def _equalizer_biquad_eager(waveform: Tensor, sample_rate: int, center_freq: float, gain: float, Q: float = 0.707) -> Tensor:
    r"""functional/filtering.py:851-890."""
    dt = waveform.dtype
    w0 = _w0(center_freq, sample_rate, dt)
    A = torch.exp(_cpu_scalar(gain, dt) / 40.0 * math.log(10))
    alpha = torch.sin(w0) / 2 / _cpu_scalar(Q, dt)
    return biquad(waveform, 1 + alpha * A, -2 * torch.cos(w0), 1 - alpha * A, 1 + alpha / A, -2 * torch.cos(w0),
                  1 - alpha / A)


def _band_biquad_eager(waveform: Tensor, sample_rate: int, central_freq: float, Q: float = 0.707, noise: bool = False) -> Tensor:
    r"""functional/filtering.py:180-229."""
    dt = waveform.dtype
    fc = _cpu_scalar(central_freq, dt)
    w0 = 2 * math.pi * fc / sample_rate
    bw_hz = fc / _cpu_scalar(Q, dt)
    a2 = torch.exp(-2 * math.pi * bw_hz / sample_rate)
    a1 = -4 * a2 / (1 + a2) * torch.cos(w0)
    b0 = torch.sqrt(1 - a1 * a1 / (4 * a2)) * (1 - a2)
    if noise:
        mult = torch.sqrt(((1 + a2) * (1 + a2) - a1 * a1) * (1 - a2) / (1 + a2)) / b0
        b0 = mult * b0
    return biquad(waveform, b0, 0.0, 0.0, 1.0, a1, a2)


def _shelf_terms(sample_rate: int, gain, central_freq, Q, dt):
    w0 = _w0(central_freq, sample_rate, dt)
    alpha = torch.sin(w0) / 2 / _cpu_scalar(Q, dt)
    A = torch.exp(_cpu_scalar(gain, dt) / 40 * math.log(10))
    return A, 2 * torch.sqrt(A) * alpha, (A - 1) * torch.cos(w0), (A + 1) * torch.cos(w0)


def _treble_biquad_eager(waveform: Tensor, sample_rate: int, gain: float, central_freq: float = 3000, Q: float = 0.707) -> Tensor:
    r"""functional/filtering.py:1363-1411 (high shelf)."""
    A, t1, t2, t3 = _shelf_terms(sample_rate, gain, central_freq, Q, waveform.dtype)
    b0 = A * ((A + 1) + t2 + t1)
    b1 = -2 * A * ((A - 1) + t3)
    b2 = A * ((A + 1) + t2 - t1)
    a0 = (A + 1) - t2 + t1
    a1 = 2 * ((A - 1) - t3)
    a2 = (A + 1) - t2 - t1
    return biquad(waveform, b0, b1, b2, a0, a1, a2)


def _bass_biquad_eager(waveform: Tensor, sample_rate: int, gain: float, central_freq: float = 100, Q: float = 0.707) -> Tensor:
    r"""functional/filtering.py:232-280 (low shelf; coefficients pre-divided by a0 as there)."""
    A, t1, t2, t3 = _shelf_terms(sample_rate, gain, central_freq, Q, waveform.dtype)
    b0 = A * ((A + 1) - t2 + t1)
    b1 = 2 * A * ((A - 1) - t3)
    b2 = A * ((A + 1) - t2 - t1)
    a0 = (A + 1) + t2 + t1
    a1 = -2 * ((A - 1) + t3)
    a2 = (A + 1) + t2 - t1
    return biquad(waveform, b0 / a0, b1 / a0, b2 / a0, a0 / a0, a1 / a0, a2 / a0)


# --------------------------------------------------------------------------- #
# fftconvolve                                                                 #
# --------------------------------------------------------------------------- #


def _deemph_biquad_eager(waveform: Tensor, sample_rate: int) -> Tensor:
    r"""ISO 908 CD de-emphasis (functional/filtering.py:417-462): a high shelf in SoX's slope parameterisation,
    alpha = sin(w0) / 2 * sqrt((A + 1 / A) (1 / S - 1) + 2), at 44.1 kHz (5283 Hz, S 0.4845, -9.477 dB) or 48 kHz (5356 Hz,
    S 0.479, -9.62 dB); any other rate raises like the reference."""
    table = {44100: (5283.0, 0.4845, -9.477), 48000: (5356.0, 0.479, -9.62)}
    if sample_rate not in table:
        raise ValueError("Sample rate must be 44100 (audio-CD) or 48000 (DAT)")
    freq, slope, gain = table[sample_rate]
    w0 = 2.0 * math.pi * freq / sample_rate
    A = math.exp(gain / 40.0 * math.log(10.0))
    alpha = math.sin(w0) / 2.0 * math.sqrt((A + 1.0 / A) * (1.0 / slope - 1.0) + 2.0)
    t1, t2, t3 = 2.0 * math.sqrt(A) * alpha, (A - 1.0) * math.cos(w0), (A + 1.0) * math.cos(w0)
    return biquad(waveform, A * ((A + 1.0) + t2 + t1), -2.0 * A * ((A - 1.0) + t3), A * ((A + 1.0) + t2 - t1),
                  (A + 1.0) - t2 + t1, 2.0 * ((A - 1.0) - t3), (A + 1.0) - t2 - t1)


def _riaa_biquad_eager(waveform: Tensor, sample_rate: int) -> Tensor:
    r"""RIAA vinyl playback equalisation (functional/filtering.py:1294-1360): SoX's zero / pole pairs for 44.1, 48, 88.2 and
    96 kHz, normalised to 0 dB at 1 kHz; any other rate raises like the reference."""
    table = {44100: ((-0.2014898, 0.9233820), (0.7083149, 0.9924091)), 48000: ((-0.1766069, 0.9321590), (0.7396325, 0.9931330)),
             88200: ((-0.1168735, 0.9648312), (0.8590646, 0.9964002)), 96000: ((-0.1141486, 0.9676817), (0.8699137, 0.9966946))}
    if sample_rate not in table:
        raise ValueError("Sample rate must be 44.1k, 48k, 88.2k, or 96k")
    (z0, z1), (p0, p1) = table[sample_rate]
    b = [1.0, -(z0 + z1), z0 * z1]
    a = [1.0, -(p0 + p1), p0 * p1]
    y = 2.0 * math.pi * 1000.0 / sample_rate                       # |H| = 1 at 1 kHz
    num = complex(b[0] + b[1] * math.cos(y) + b[2] * math.cos(2 * y), -(b[1] * math.sin(y) + b[2] * math.sin(2 * y)))
    den = complex(a[0] + a[1] * math.cos(y) + a[2] * math.cos(2 * y), -(a[1] * math.sin(y) + a[2] * math.sin(2 * y)))
    g = abs(den) / abs(num)
    return biquad(waveform, b[0] * g, b[1] * g, b[2] * g, a[0], a[1], a[2])


def _check_shape_compatible(x: Tensor, y: Tensor) -> None:
    if x.ndim != y.ndim:
        raise ValueError(f"The operands must be the same dimension (got {x.ndim} and {y.ndim}).")
    for i in range(x.ndim - 1):
        xi, yi = x.size(i), y.size(i)
        if xi == yi or xi == 1 or yi == 1:
            continue
        raise ValueError(f"Leading dimensions of x and y are not broadcastable (got {x.shape} and {y.shape}).")


_CONV_MODES = ["full", "valid", "same"]


def _check_convolve_mode(mode: str) -> None:
    if mode not in _CONV_MODES:
        raise ValueError(f"Unrecognized mode value '{mode}'. Please specify one of {_CONV_MODES}.")


_FFTCONV_HELD_BYTES = 64 << 20       # largest workspace kept with a tap tensor (cfg5: 0.5 MiB per tap row)
_FFTCONV_HELD_TOTAL = 512 << 20      # ... and of all kept workspaces together, per process
_HELD_LIVE: list = []                # weak references to the live _HeldTaps (their bytes are summed when one more is asked for)


def _held_taps_or_none(ws_bytes: int, dev):
    """A workspace to keep with a tap tensor, or None when the process already keeps `_FFTCONV_HELD_TOTAL` bytes of them."""
    with _CACHE_LOCK:
        live = [r for r in _HELD_LIVE if r() is not None]
        _HELD_LIVE[:] = live
        if sum(r().ws.numel() * 4 for r in live) + ws_bytes > _FFTCONV_HELD_TOTAL:
            return None
    held = _HeldTaps(torch.empty((ws_bytes // 4 + 2,), dtype=torch.float32, device=dev))
    with _CACHE_LOCK:
        _HELD_LIVE.append(weakref.ref(held))
    return held


class _HeldTaps:
    """The prepared workspace of one (tap tensor, plan, stream): twiddles + tap spectra, read-only once `ready`."""
    __slots__ = ("ws", "ready", "_claimed", "_lock", "__weakref__")

    def __init__(self, ws: Tensor):
        self.ws, self.ready, self._claimed, self._lock = ws, False, False, threading.Lock()

    def claim(self) -> bool:
        with self._lock:
            if self._claimed:
                return False
            self._claimed = True
            return True


def fftconvolve_held_taps(y: Tensor) -> int:
    """How many prepared workspaces the cache holds for tap tensor `y` at its current version (tests, reports)."""
    with _CACHE_LOCK:
        slot = _TENSOR_CACHE.get(id(y))
        if slot is None or slot[0]() is not y:
            return 0
        return sum(1 for k, v in slot[1].items() if isinstance(v, _HeldTaps) and v.ready and k[1] == y._version)


def _conv_slice(x: Tensor, y: Tensor, start: int, out_len: int, hold: bool = True) -> Tensor:
    """out[..., i] = (x * y)[start + i], i in [0, out_len): a slice of the full linear convolution of the
    last dims, leading dims broadcast (forward-only launcher of aamd_fftconvolve_f32)."""
    nx, ny = x.size(-1), y.size(-1)
    lead = torch.broadcast_shapes(tuple(x.shape[:-1]), tuple(y.shape[:-1]))
    rows = 1
    for d in lead:
        rows *= d
    xr = x.reshape(-1, nx).contiguous()
    yr = y.reshape(-1, ny).contiguous()

    def row_map(t: Tensor, n_rows: int):
        if tuple(t.shape[:-1]) == tuple(lead):
            return None
        # (a function of the two shapes only: kept, so that a repeated call is ONE launch -- building it took an arange and a
        # copy kernel per call, ~10 us of GPU time in front of a 0.7 ms convolution)
        def make():
            idx = torch.arange(n_rows, device=x.device).view(tuple(t.shape[:-1]))
            return idx.expand(lead).reshape(-1).contiguous()
        if torch.cuda.is_current_stream_capturing():       # (memory of a capture's private pool must not outlive the graph)
            return make()
        return _cached(("conv_row_map", tuple(t.shape[:-1]), tuple(lead), str(x.device), _lib.current_stream(x.device)), make)

    xmap, ymap = row_map(x, xr.shape[0]), row_map(y, yr.shape[0])
    if x.dtype == torch.float64:
        out = torch.empty((rows, out_len), dtype=torch.float64, device=x.device)
        if out.numel():
            with torch.cuda.device(x.device):
                _lib.check(_lib.lib().aamd_fftconvolve_f64(
                    xr.data_ptr(), yr.data_ptr(), out.data_ptr(), rows, xr.shape[0], yr.shape[0], nx, ny,
                    xmap.data_ptr() if xmap is not None else None, ymap.data_ptr() if ymap is not None else None,
                    start, out_len, _lib.current_stream(x.device)))
        return out.view(tuple(lead) + (out_len,))
    ops = _ops()
    L = _lib.lib()
    dev = x.device
    if rows * out_len == 0:
        return torch.empty((rows, out_len), dtype=torch.float32, device=dev).view(tuple(lead) + (out_len,))
    with torch.cuda.device(dev):
        ws_bytes = L.aamd_fftconvolve_workspace(rows, xr.shape[0], yr.shape[0], nx, ny)
        # A repeated impulse response (T.FFTConvolve in an augmentation loop; the reference recomputes rfft(y) every call,
        # functional.py:2252-2258): the twiddle table and the tap spectra of the plan stay with the tap tensor, and every call
        # after the first skips the two preparation launches (aamd_fftconvolve_staged_f32; ~16 us of the config-5 shard's 0.79 ms).
        # Only where the workspace is read-only while the plan runs (plans 1 and 3), the taps are y (ny <= nx), nothing is being
        # captured (a replayed graph must not depend on host-side version checks) and the workspace is small.
        # A workspace is kept only for a tap tensor that has SHOWN it is reused -- from the second call with the same
        # (tensor object, version) on: a fresh RIR batch per step must not leave 64 MiB behind per step --, never for
        # the flipped temporaries of the autograd backward (`hold=False`), and only while the process keeps less than
        # `_FFTCONV_HELD_TOTAL` bytes of them; the slot goes when the tap tensor dies (`_drop_dead_slot`).
        held, stages = None, 3
        if hold and ws_bytes and ny <= nx and ws_bytes <= _FFTCONV_HELD_BYTES and not torch.cuda.is_current_stream_capturing():
            plan = int(L.aamd_fftconvolve_plan(rows, nx, ny, out_len))
            if plan in (1, 3):
                key = ("fftconv_ws", plan, ny, yr.shape[0], int(ws_bytes), _lib.current_stream(dev),
                       int(L.aamd_set_kernel_policy(-1)))
                seen = _tensor_cached(y, ("fftconv_seen",) + key[1:], lambda: [0])
                seen[0] += 1
                if seen[0] >= 2:
                    held = _tensor_cached(y, key, lambda: _held_taps_or_none(int(ws_bytes), dev) or False) or None
                if held is not None:
                    if held.ready:
                        stages = 2
                    elif not held.claim():      # another thread is preparing this very workspace right now: use a private one
                        held = None
        ws = held.ws if held is not None else torch.empty((ws_bytes // 4 + 2,), dtype=torch.float32, device=dev)
        if ops is not None:
            out = ops.fftconvolve_staged(xr, yr, xmap, ymap, rows, start, out_len, ws, stages)
        else:
            out = torch.empty((rows, out_len), dtype=torch.float32, device=dev)
            _lib.check(L.aamd_fftconvolve_staged_f32(
                xr.data_ptr(), yr.data_ptr(), out.data_ptr(), rows, xr.shape[0], yr.shape[0], nx, ny,
                xmap.data_ptr() if xmap is not None else None, ymap.data_ptr() if ymap is not None else None,
                start, out_len, ws.data_ptr() if ws_bytes else None, stages, _lib.current_stream(dev)))
        if held is not None and stages == 3:
            held.ready = True                   # the preparation launches are in the stream: later calls on it may run-only
    return out.view(tuple(lead) + (out_len,))


class _FFTConvolveFunction(torch.autograd.Function):
    """z = (x * y)[start : start + out_len].  Both adjoints are correlations, i.e. convolutions with a
    time-reversed operand, evaluated by the same kernels:
        dL/dx[m] = sum_n dz[n] y[n - m] = (dz_full * flip(y))[m + ny - 1]
        dL/dy[j] = sum_n dz[n] x[n - j] = (dz_full * flip(x))[j + nx - 1]
    (dz_full = dz placed at offset `start` of the full length), summed over broadcast leading dims."""

    @staticmethod
    def forward(ctx, x, y, start, out_len):
        ctx.save_for_backward(x, y)
        ctx.start, ctx.out_len = start, out_len
        return _conv_slice(x, y, start, out_len)

    @staticmethod
    def backward(ctx, dz):
        x, y = ctx.saved_tensors
        nx, ny = x.size(-1), y.size(-1)
        full = torch.nn.functional.pad(dz, (ctx.start, nx + ny - 1 - ctx.start - ctx.out_len))   # dz at offset `start`
        # create_graph=True: both adjoints are convolutions again -- apply them through this Function
        # (the flipped operands are temporaries: nothing is kept with them)
        conv = _FFTConvolveFunction.apply if torch.is_grad_enabled() else (lambda a, b, st, n: _conv_slice(a, b, st, n, hold=False))
        dx = dy = None
        if ctx.needs_input_grad[0]:
            dx = conv(full, y.flip(-1), ny - 1, nx).sum_to_size(x.shape)
        if ctx.needs_input_grad[1]:
            dy = conv(full, x.flip(-1), nx - 1, ny).sum_to_size(y.shape)
        return dx, dy, None, None


@_reduced_precision_io
def _fftconvolve_eager(x: Tensor, y: Tensor, mode: str = "full") -> Tensor:
    r"""Linear convolution along the last dim with broadcast leading dims and the reference's
    full / valid / same crops (functional/functional.py:2222-2258).  Differentiable in both operands."""
    _check_shape_compatible(x, y)
    _check_convolve_mode(mode)
    if not x.is_floating_point():
        x = x.float()
    if not y.is_floating_point():
        y = y.float()
    _require_device(x, "x", allow_grad=True, allow_f64=True)
    _require_device(y, "y", allow_grad=True, allow_f64=True)
    if x.dtype != y.dtype:
        raise TypeError(f"audio_amd: fftconvolve operands must share a dtype (got {x.dtype} and {y.dtype})")
    nx, ny = x.size(-1), y.size(-1)
    n_full = nx + ny - 1
    if mode == "full":
        start, out_len = 0, n_full
    elif mode == "valid":
        out_len = max(nx, ny) - min(nx, ny) + 1
        start = (n_full - out_len) // 2
    else:
        out_len = nx
        start = (n_full - nx) // 2
    if torch.is_grad_enabled() and (x.requires_grad or y.requires_grad):
        return _FFTConvolveFunction.apply(x, y, start, out_len)
    return _conv_slice(x, y, start, out_len)


# --------------------------------------------------------------------------- #
# deltas / sliding-window CMN (csrc/feat_post.h)                              #
# --------------------------------------------------------------------------- #

_DELTA_PAD = {"reflect": 0, "constant": 1, "replicate": 2, "circular": 3}


def _deltas_launch(x3: Tensor, win_length: int, mode_id: int, adjoint: bool) -> Tensor:
    """(C, F, T) of any strides -> dense (C, F, T): the delta stencil (adjoint: its transpose), one launch."""
    ops = _ops()
    if ops is not None:
        return ops.compute_deltas(x3, win_length, mode_id, adjoint)
    out = torch.empty(x3.shape, dtype=x3.dtype, device=x3.device)
    fn = _lib.lib().aamd_compute_deltas_f64 if x3.dtype == torch.float64 else _lib.lib().aamd_compute_deltas_f32
    with torch.cuda.device(x3.device):
        _lib.check(fn(_lib.ptr(x3) or None, _lib.ptr(out) or None, x3.shape[0], x3.shape[1], x3.shape[2], x3.stride(0),
                      x3.stride(1), x3.stride(2), win_length, mode_id, int(adjoint), _lib.current_stream(x3.device)))
    return out


class _DeltasFunction(torch.autograd.Function):
    """The delta stencil D (adjoint=False) or its transpose D^T (adjoint=True).  Linear: the backward is the other one,
    applied through this Function again, so gradients of every order run on the kernel."""

    @staticmethod
    def forward(ctx, x3, win_length, mode_id, adjoint):
        ctx.args = (win_length, mode_id, adjoint)
        return _deltas_launch(x3, win_length, mode_id, adjoint)

    @staticmethod
    def backward(ctx, g):
        win_length, mode_id, adjoint = ctx.args
        if torch.is_grad_enabled():
            return _DeltasFunction.apply(g, win_length, mode_id, not adjoint), None, None, None
        return _deltas_launch(g, win_length, mode_id, not adjoint), None, None, None


@_reduced_precision_io
def _compute_deltas_eager(specgram: Tensor, win_length: int = 5, mode: str = "replicate") -> Tensor:
    r"""Delta coefficients along time of a ``(..., freq, time)`` tensor (reference: F.compute_deltas, pad + grouped conv1d).
    The input is read in place through its strides -- time-contiguous rows and the frame-major storage of every
    MelSpectrogram / Spectrogram output alike -- and the result is a new contiguous tensor of the input's shape."""
    if win_length < 3:
        raise ValueError(f"Window length should be greater than or equal to 3. Found win_length {win_length}")
    if mode not in _DELTA_PAD:
        raise ValueError(f"audio_amd: compute_deltas: unknown padding mode {mode!r} "
                         "(reflect, constant, replicate, circular)")
    _require_device(specgram, "specgram", allow_grad=True, allow_f64=True)
    shape = specgram.shape
    T = shape[-1] if specgram.dim() >= 1 else 1
    n = (win_length - 1) // 2
    if (mode == "reflect" and n >= T) or (mode == "circular" and n > T):
        raise RuntimeError(f"audio_amd: compute_deltas: {mode} padding of {n} frames needs "
                           f"{'more than' if mode == 'reflect' else 'at least'} {n} frames, got {T}")
    x3 = specgram.reshape(-1, shape[-2] if specgram.dim() >= 2 else 1, T)       # a view wherever the strides allow
    if torch.is_grad_enabled() and specgram.requires_grad:
        out = _DeltasFunction.apply(x3, win_length, _DELTA_PAD[mode], False)
    else:
        out = _deltas_launch(x3, win_length, _DELTA_PAD[mode], False)
    return out.view(shape)


def _cmn_launch(x3: Tensor, cmn_window: int, min_cmn_window: int, center: bool, norm_vars: bool, adjoint: bool) -> Tensor:
    """(C, T, F) of any strides -> dense (C, T, F): chunk sums, then the window walk (two launches)."""
    ops = _ops()
    if ops is not None:
        return ops.sliding_window_cmn(x3, cmn_window, min_cmn_window, center, norm_vars, adjoint)
    L = _lib.lib()
    out = torch.empty(x3.shape, dtype=x3.dtype, device=x3.device)
    ws = torch.empty((max(int(L.aamd_sliding_window_cmn_workspace(*x3.shape, int(norm_vars))) // 8, 1),),
                     dtype=torch.float64, device=x3.device)
    fn = L.aamd_sliding_window_cmn_f64 if x3.dtype == torch.float64 else L.aamd_sliding_window_cmn_f32
    with torch.cuda.device(x3.device):
        _lib.check(fn(_lib.ptr(x3) or None, _lib.ptr(out) or None, ws.data_ptr(), x3.shape[0], x3.shape[1], x3.shape[2],
                      x3.stride(0), x3.stride(2), x3.stride(1), cmn_window, min_cmn_window, int(center), int(norm_vars),
                      int(adjoint), _lib.current_stream(x3.device)))
    return out


class _CmnFunction(torch.autograd.Function):
    """Sliding-window mean normalisation (norm_vars=False) is linear: x - W x.  The backward is its transpose
    g - W^T (g), run by the same kernels (adjoint=1), and the transpose of that is the forward again."""

    @staticmethod
    def forward(ctx, x3, cmn_window, min_cmn_window, center, adjoint):
        ctx.args = (cmn_window, min_cmn_window, center, adjoint)
        return _cmn_launch(x3, cmn_window, min_cmn_window, center, False, adjoint)

    @staticmethod
    def backward(ctx, g):
        cmn_window, min_cmn_window, center, adjoint = ctx.args
        if torch.is_grad_enabled():
            gx = _CmnFunction.apply(g, cmn_window, min_cmn_window, center, not adjoint)
        else:
            gx = _cmn_launch(g, cmn_window, min_cmn_window, center, False, not adjoint)
        return gx, None, None, None, None


@_reduced_precision_io
def _sliding_window_cmn_eager(specgram: Tensor, cmn_window: int = 600, min_cmn_window: int = 100, center: bool = False,
                              norm_vars: bool = False) -> Tensor:
    r"""Kaldi's sliding-window cepstral mean (and variance) normalisation of a ``(..., time, freq)`` tensor (reference:
    F.sliding_window_cmn, a per-frame loop with a float32 running sum).  Every window sum here is exact to float64
    accumulation.  Any strides are accepted (the reference's ``view`` refuses some); the result is a new contiguous
    tensor, squeezed like the reference's for a 2-D input of one frame.  With ``norm_vars`` and an input that requires
    grad the call takes the differentiable composition ``_diff.sliding_window_cmvn``."""
    if specgram.dim() < 2:
        raise ValueError(f"audio_amd: sliding_window_cmn expects (..., time, freq), got shape {tuple(specgram.shape)}")
    if cmn_window < 0:
        raise ValueError(f"audio_amd: sliding_window_cmn: cmn_window must be >= 0, got {cmn_window}")
    _require_device(specgram, "specgram", allow_grad=True, allow_f64=True)
    shape = specgram.shape
    x3 = specgram.reshape(-1, shape[-2], shape[-1])
    grad = torch.is_grad_enabled() and specgram.requires_grad
    if norm_vars and grad:
        out = _diff.sliding_window_cmvn(x3, cmn_window, min_cmn_window, center)
    elif grad:
        out = _CmnFunction.apply(x3, cmn_window, min_cmn_window, center, False)
    else:
        out = _cmn_launch(x3, cmn_window, min_cmn_window, center, norm_vars, False)
    out = out.view(shape)
    if len(shape) == 2:
        out = out.squeeze(0)
    return out


# --------------------------------------------------------------------------- #
# NCCF pitch tracker (csrc/pitch.h)                                           #
# --------------------------------------------------------------------------- #

_PITCH_MAX_FRAME = 8192
_PITCH_MAX_LAGS = 16384


def _pitch_sizes(length: int, sample_rate: int, frame_time: float, freq_low: int) -> Tuple[int, int, int]:
    """(lags, frame_size, frames) with exactly the reference's expressions (_compute_nccf); its errors where it has them."""
    lags = int(math.ceil(sample_rate / freq_low))
    fs = int(math.ceil(sample_rate * frame_time))
    F_ = int(math.ceil(length / fs))
    if lags < 1:      # the reference's lag loop is empty: torch.cat([])
        raise ValueError(f"torch.cat(): expected a non-empty list of Tensors (lags = ceil({sample_rate} / {freq_low}) = {lags})")
    if fs < 0:
        raise RuntimeError(f"audio_amd: detect_pitch_frequency: frame size ceil({sample_rate} * {frame_time}) = {fs} < 0")
    return lags, fs, F_


def _pitch_plan(length: int, sample_rate: int, frame_time: float, win_length: int, freq_low: int,
                freq_high: int) -> Tuple[int, int, int, int, int]:
    """(lags, frame_size, frames, lag_min, n_out) of detect_pitch_frequency, raising what the reference raises, in its
    order; sizes this build does not serve raise NotImplementedError."""
    lags, fs, F_ = _pitch_sizes(length, sample_rate, frame_time, freq_low)
    lag_min = int(math.ceil(sample_rate / freq_high))
    if lag_min < 0:
        raise ValueError(f"audio_amd: detect_pitch_frequency: freq_high = {freq_high} gives a negative minimal lag")
    if lag_min >= lags or lags // 2 <= lag_min:    # torch.max over nccf[..., lag_min:] or nccf[..., lag_min:lags // 2]
        raise IndexError(f"max(): Expected reduction dim 2 to have non-zero size. (lag_min = {lag_min}, lags = {lags}: "
                         "freq_high must be well above freq_low)")
    p = (win_length - 1) // 2
    if F_ == 0:
        raise IndexError(f"index {p} is out of bounds for dimension 1 with size {p} (the waveform has no frame)")
    if p <= 0:        # _median_smoothing's torch.cat(pad_length * [...])
        raise ValueError(f"torch.cat(): expected a non-empty list of Tensors (win_length = {win_length} < 3)")
    n_out = F_ + p - win_length + 1
    if n_out < 1:     # _median_smoothing's unfold
        raise RuntimeError(f"maximum size for tensor at dimension 1 is {F_ + p} but size is {win_length} "
                           f"({F_} frames are fewer than one median window)")
    if fs > _PITCH_MAX_FRAME or lags > _PITCH_MAX_LAGS:
        raise NotImplementedError(f"audio_amd: detect_pitch_frequency serves frame sizes up to {_PITCH_MAX_FRAME} and up to "
                                  f"{_PITCH_MAX_LAGS} lags (got {fs} and {lags})")
    return lags, fs, F_, lag_min, n_out


def _pitch_rows(waveform: Tensor) -> Tensor:
    """(..., L) -> (rows, L) float32 / float64 with time stride 1, rows read in place where the strides allow."""
    if waveform.dtype in LOW_PRECISION and waveform.is_cuda:
        x = waveform.detach().float()
    else:
        _require_device(waveform, "waveform", allow_grad=True, allow_f64=True)
        x = waveform.detach()
    if x.dim() == 0:
        raise ValueError("audio_amd: detect_pitch_frequency expects a (..., time) waveform, got a 0-d tensor")
    return _rows2d(x)


def _pitch_launch(x2: Tensor, sample_rate: int, fs: int, lags: int, lag_min: int, win_length: int, mode: int) -> Tensor:
    """mode 0: float32 (rows, n_out) pitch; mode 1: (rows, F, lags) NCCF of x2's dtype."""
    ops = _ops()
    if ops is not None:
        return ops.detect_pitch(x2, sample_rate, fs, lags, lag_min, win_length, mode)
    rows, L = x2.shape
    F_ = -(-L // fs)
    if mode == 1:
        out = torch.empty((rows, F_, lags), dtype=x2.dtype, device=x2.device)
    else:
        out = torch.empty((rows, F_ + (win_length - 1) // 2 - win_length + 1), dtype=torch.float32, device=x2.device)
    Lb = _lib.lib()
    ws = torch.empty((max(int(Lb.aamd_detect_pitch_workspace(rows, L, fs)) // 4, 1),), dtype=torch.int32, device=x2.device)
    fn = Lb.aamd_detect_pitch_f64 if x2.dtype == torch.float64 else Lb.aamd_detect_pitch_f32
    with torch.cuda.device(x2.device):
        _lib.check(fn(_lib.ptr(x2) or None, _lib.ptr(out) or None, ws.data_ptr(), rows, L, x2.stride(0), sample_rate, fs,
                      lags, lag_min, win_length, mode, _lib.current_stream(x2.device)))
    return out


def _compute_nccf(waveform: Tensor, sample_rate: int, frame_time: float, freq_low: int) -> Tensor:
    r"""The NCCF of the reference's private helper: ``(..., L)`` -> ``(..., frames, lags)``, float64 for a float64 input and
    float32 otherwise.  It is what detect_pitch_frequency's fused pick reads, bit for bit (the same kernel, mode 1)."""
    x2 = _pitch_rows(waveform)
    lags, fs, F_ = _pitch_sizes(x2.shape[-1], sample_rate, frame_time, freq_low)
    if fs > _PITCH_MAX_FRAME or lags > _PITCH_MAX_LAGS:
        raise NotImplementedError(f"audio_amd: _compute_nccf serves frame sizes up to {_PITCH_MAX_FRAME} and up to "
                                  f"{_PITCH_MAX_LAGS} lags (got {fs} and {lags})")
    out = _pitch_launch(x2, sample_rate, fs, lags, 0, 3, 1)
    return out.view(tuple(waveform.shape[:-1]) + (F_, lags))


def _detect_pitch_frequency_eager(waveform: Tensor, sample_rate: int, frame_time: float = 10 ** (-2), win_length: int = 30,
                                  freq_low: int = 85, freq_high: int = 3400) -> Tensor:
    r"""Pitch of a ``(..., time)`` waveform in Hz (reference: F.detect_pitch_frequency): the NCCF, both max reductions and
    the 0.99 combine in one kernel, the median smoothing and the reciprocal in a second.  float32 out for every input dtype
    (float64 inputs compute in float64, float16 / bfloat16 in float32); no gradient, as in the reference."""
    x2 = _pitch_rows(waveform)
    lags, fs, F_, lag_min, n_out = _pitch_plan(x2.shape[-1], sample_rate, frame_time, win_length, freq_low, freq_high)
    out = _pitch_launch(x2, sample_rate, fs, lags, lag_min, win_length, 0)
    return out.view(tuple(waveform.shape[:-1]) + (n_out,))


# --------------------------------------------------------------------------- #
# SpecAugment masking (csrc/spec_augment.h)                                   #
# --------------------------------------------------------------------------- #

_SA_FREQ, _SA_TIME = 0, 1                                      # axis tags of the C ABI (AAMD_SA_FREQ / AAMD_SA_TIME)
_SA_DTYPES = {torch.float32: 0, torch.float64: 1, torch.float16: 2, torch.bfloat16: 3}
_SA_BITS = {2: torch.int16, 4: torch.int32, 8: torch.int64}
_SA_MAX_MASKS = 32                                             # per launch; longer policies chain launches


def _get_mask_param(mask_param: int, p: float, axis_length: int) -> int:
    if p == 1.0:
        return mask_param
    return min(mask_param, int(axis_length * p))


def _sa_require(x: Tensor, what: str) -> None:
    if not x.is_floating_point():
        raise TypeError(f"audio_amd: {what} must be a floating-point tensor (got {x.dtype})")
    if not x.is_cuda:
        raise RuntimeError(f"audio_amd: {what} must be on an MI355X (ROCm) device, got {x.device}. "
                           "The HIP kernels have no CPU fallback.")


def _sa_check(dim: int, min_dim: int, axis: int, p: float) -> None:
    if dim < min_dim:
        if min_dim == 3:
            raise ValueError(f"Spectrogram must have at least three dimensions ({dim} given).")
        raise ValueError(f"Spectrogram must have at least two dimensions (time and frequency) ({dim} given).")
    if axis not in [dim - 2, dim - 1]:
        raise ValueError("Only Frequency and Time masking are supported"
                         f" (axis {dim - 2} and axis {dim - 1} supported; {axis} given).")
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"The value of p must be between 0.0 and 1.0 ({p} given).")


def _sa_value_bits(value: float, dtype: torch.dtype) -> int:
    """mask_value as the element's bits (unsigned), converted the way masked_fill converts a Python scalar."""
    def make():
        t = torch.full((), value, dtype=dtype)
        return int(t.view(_SA_BITS[t.element_size()]).item()) & ((1 << (8 * t.element_size())) - 1)
    return _cached(("sa_value_bits", float(value), dtype), make)


def _sa_launch(x3: Tensor, time_inner: bool, draws: Optional[Tensor], axes: List[int], params: List[int],
               starts: List[int], ends: List[int], bits: int, value: Optional[Tensor]) -> Tensor:
    """(examples, outer, inner) of any strides -> dense, at most _SA_MAX_MASKS masks, one launch."""
    ops = _ops()
    if ops is not None:
        return ops.spec_augment(x3, draws, axes, params, starts, ends, time_inner, bits - (1 << 64) if bits >= 1 << 63 else bits,
                                value)
    out = torch.empty(x3.shape, dtype=x3.dtype, device=x3.device)
    n = len(axes)
    ax = (C.c_int32 * max(n, 1))(*axes)
    common = (_lib.ptr(x3) or None, _lib.ptr(out) or None, x3.shape[0], x3.shape[1], x3.shape[2], x3.stride(0), x3.stride(1),
              x3.stride(2), _SA_DTYPES[x3.dtype], int(time_inner), n, ax)
    vp = value.data_ptr() if value is not None else None
    with torch.cuda.device(x3.device):
        if draws is not None:
            _lib.check(_lib.lib().aamd_spec_augment_iid(*common, (C.c_int64 * max(n, 1))(*params), _lib.ptr(draws) or None,
                                                        bits, vp, _lib.current_stream(x3.device)))
        else:
            _lib.check(_lib.lib().aamd_spec_augment_shared(*common, (C.c_int64 * max(n, 1))(*starts),
                                                           (C.c_int64 * max(n, 1))(*ends), bits, vp,
                                                           _lib.current_stream(x3.device)))
    return out


def _sa_run(x: Tensor, draws: Optional[Tensor], plan, bounds, value) -> Tensor:
    """The policy over x (..., freq, time): `plan` lists (axis tag, mask_param) per mask; iid bounds come from `draws`
    (masks, 2, examples), shared ones from `bounds` [(start, end)].  A dense x in either order of its last two axes is
    streamed along its own contiguous axis and the result has x's strides; anything else is gathered into a contiguous
    result."""
    shape = tuple(x.shape)
    n_freq, n_time = shape[-2], shape[-1]
    examples = 1
    for d in shape[:-2]:
        examples *= d
    if x.is_contiguous():
        x3, time_inner = x.view(examples, n_freq, n_time), True
    elif x.transpose(-1, -2).is_contiguous():                      # frame-major: what every MelSpectrogram here returns
        x3, time_inner = x.transpose(-1, -2).view(examples, n_time, n_freq), False
    else:
        x3, time_inner = x.reshape(examples, n_freq, n_time), True
    bits, vt = 0, None
    if isinstance(value, Tensor):
        vt = value.detach().to(device=x.device, dtype=x.dtype).reshape(())
    else:
        bits = _sa_value_bits(value, x.dtype)
    out = x3
    for at in range(0, max(len(plan), 1), _SA_MAX_MASKS):
        part = plan[at:at + _SA_MAX_MASKS]
        axes = [a for a, _ in part]
        if draws is not None:
            out = _sa_launch(out, time_inner, draws[at:at + len(part)], axes, [m for _, m in part], [], [], bits, vt)
        else:
            b = bounds[at:at + len(part)]
            out = _sa_launch(out, time_inner, None, axes, [], [s_ for s_, _ in b], [e_ for _, e_ in b], bits, vt)
    if time_inner:
        return out.view(shape)
    return out.view(shape[:-2] + (n_time, n_freq)).transpose(-1, -2)


class _SpecAugmentFunction(torch.autograd.Function):
    """out = x (1 - m) + v m.  The gradient to x is the same masks over the cotangent with value 0 (its own adjoint, so
    every order runs on the kernel); a tensor mask_value receives what the masks removed, (g - g_x).sum()."""

    @staticmethod
    def forward(ctx, x, value, draws, plan, bounds):
        ctx.masks = (draws, plan, bounds)
        ctx.value_grad = isinstance(value, Tensor) and value.requires_grad
        ctx.value_meta = (value.shape, value.dtype, value.device) if isinstance(value, Tensor) else None
        return _sa_run(x, draws, plan, bounds, value)

    @staticmethod
    def backward(ctx, g):
        draws, plan, bounds = ctx.masks
        gx = gv = None
        if ctx.needs_input_grad[0] or ctx.value_grad:
            if torch.is_grad_enabled():
                gx = _SpecAugmentFunction.apply(g, 0.0, draws, plan, bounds)
            else:
                gx = _sa_run(g, draws, plan, bounds, 0.0)
        if ctx.value_grad:
            shape, dtype, device = ctx.value_meta
            gv = (g - gx).sum().to(device=device, dtype=dtype).reshape(shape)
        return (gx if ctx.needs_input_grad[0] else None), gv, None, None, None


def _spec_augment_apply(x: Tensor, draws_or_bounds, plan, mask_value=0.0) -> Tensor:
    r"""A masking policy with explicit masks over ``x`` (..., freq, time), any number of masks: ``plan`` lists one
    ``(axis, mask_param)`` per mask, axis 0 for frequency and 1 for time (or ``-2`` / ``-1``).  ``draws_or_bounds`` is either
    the raw uniform draws, a ``(masks, 2) + x.shape[:-2]`` tensor of ``x``'s dtype on its device (per-example masks with the
    arithmetic of F.mask_along_axis_iid), or a list of shared ``(start, end)`` pairs (mask_param is then unused).
    ``mask_value`` is a number or a one-element tensor (read on the device: no synchronisation)."""
    _sa_require(x, "specgram")
    if x.dim() < 2:
        raise ValueError(f"Spectrogram must have at least two dimensions (time and frequency) ({x.dim()} given).")
    plan = [(a, 0) if isinstance(a, int) else (a[0], int(a[1])) for a in plan]
    plan = [(_SA_TIME if a in (_SA_TIME, -1) else _SA_FREQ, m) for a, m in plan]
    draws = bounds = None
    if isinstance(draws_or_bounds, Tensor):
        draws = draws_or_bounds
        if draws.dtype != x.dtype or draws.device != x.device or tuple(draws.shape) != (len(plan), 2) + tuple(x.shape[:-2]):
            raise ValueError("audio_amd: draws must be a (masks, 2) + specgram.shape[:-2] tensor of specgram's dtype on its device")
        draws = draws.contiguous().view(len(plan), 2, -1) if draws.numel() else draws.reshape(len(plan), 2, 0)
    else:
        bounds = [(int(s_), int(e_)) for s_, e_ in draws_or_bounds]
        if len(bounds) != len(plan):
            raise ValueError("audio_amd: one (start, end) pair per mask")
    wants = x.requires_grad or (isinstance(mask_value, Tensor) and mask_value.requires_grad)
    if torch.is_grad_enabled() and wants:
        return _SpecAugmentFunction.apply(x, mask_value, draws, plan, bounds)
    return _sa_run(x, draws, plan, bounds, mask_value)


def _sa_draw_iid(specgrams: Tensor, n_masks: int) -> Tensor:
    """The reference's draws, in its order: per mask torch.rand(lead) for `value`, then for `min_value`, of the tensor's
    dtype on its device -- each written into its slice of one buffer (a seeded call reproduces the reference's masks)."""
    lead = specgrams.shape[:-2]
    draws = torch.empty((n_masks, 2) + tuple(lead), dtype=specgrams.dtype, device=specgrams.device)
    for m in range(n_masks):
        torch.rand(lead, device=specgrams.device, dtype=specgrams.dtype, out=draws[m, 0])
        torch.rand(lead, device=specgrams.device, dtype=specgrams.dtype, out=draws[m, 1])
    return draws


def _sa_draw_shared(mask_param: int, size: int) -> Tuple[int, int]:
    """The reference's shared mask: float32 draws on the CPU whatever the tensor's dtype."""
    value = torch.rand(1) * mask_param
    min_value = torch.rand(1) * (size - value)
    start = int(min_value.long())
    end = start + int(value.long())
    if end - start >= mask_param:
        raise ValueError("Number of columns to be masked should be less than mask_param")
    return start, end


def _mask_along_axis_iid_eager(specgrams: Tensor, mask_param: int, mask_value, axis: int, p: float = 1.0) -> Tensor:
    r"""Per-example masks along frequency or time (reference: F.mask_along_axis_iid), one launch: the two raw draws go to
    the kernel, which derives every example's [start, end) itself in the tensor's dtype."""
    dim = specgrams.dim()
    _sa_check(dim, 3, axis, p)
    mask_param = _get_mask_param(mask_param, p, specgrams.shape[axis])
    if mask_param < 1:
        return specgrams
    _sa_require(specgrams, "specgrams")
    draws = _sa_draw_iid(specgrams, 1)
    return _spec_augment_apply(specgrams, draws, [(_SA_TIME if axis == dim - 1 else _SA_FREQ, mask_param)], mask_value)


def _mask_along_axis_eager(specgram: Tensor, mask_param: int, mask_value, axis: int, p: float = 1.0) -> Tensor:
    r"""One mask shared by every example (reference: F.mask_along_axis); its bounds travel in the kernel arguments."""
    dim = specgram.dim()
    _sa_check(dim, 2, axis, p)
    mask_param = _get_mask_param(mask_param, p, specgram.shape[axis])
    if mask_param < 1:
        return specgram
    _sa_require(specgram, "specgram")
    bounds = [_sa_draw_shared(mask_param, specgram.shape[axis])]
    return _spec_augment_apply(specgram, bounds, [(_SA_TIME if axis == dim - 1 else _SA_FREQ, mask_param)], mask_value)


def _spec_augment_eager(specgram: Tensor, n_time_masks: int, time_mask_param: int, n_freq_masks: int, freq_mask_param: int,
                        iid_masks: bool = True, p: float = 1.0, zero_masking: bool = False) -> Tensor:
    r"""T.SpecAugment's forward: all time masks, then all frequency masks, in ONE launch (the union of the masks does not
    depend on their order once mask_value is fixed).  mask_value = specgram.mean() stays on the device."""
    dim = specgram.dim()
    iid = dim > 2 and iid_masks
    _sa_check(dim, 3 if iid else 2, dim - 1, p)
    plan = []
    for n, param, axis in ((n_time_masks, time_mask_param, dim - 1), (n_freq_masks, freq_mask_param, dim - 2)):
        param = _get_mask_param(param, p, specgram.shape[axis])
        if param >= 1:
            plan += [(_SA_TIME if axis == dim - 1 else _SA_FREQ, param)] * max(n, 0)
    if not plan:
        return specgram
    _sa_require(specgram, "specgram")
    mask_value = 0.0 if zero_masking else specgram.mean()
    if iid:
        masks = _sa_draw_iid(specgram, len(plan))
    else:
        masks = [_sa_draw_shared(m, specgram.shape[-1] if a == _SA_TIME else specgram.shape[-2]) for a, m in plan]
    return _spec_augment_apply(specgram, masks, plan, mask_value)


# --------------------------------------------------------------------------- #
# waveform augmentation (csrc/wave_augment.h)                                 #
# --------------------------------------------------------------------------- #

WAVE_AUGMENT_CHUNK = 4096       # samples per workgroup of the add_noise / preemphasis kernels (wa::kChunk)
_WA_FLOATS = (torch.float32, torch.float64, torch.float16, torch.bfloat16)


def _wa_require(t: Tensor, what: str, floating: bool = True) -> None:
    if floating and t.dtype not in _WA_FLOATS:
        raise TypeError(f"audio_amd: {what} must be float16, bfloat16, float32 or float64 (got {t.dtype})")
    if not floating and (t.is_complex() or t.dtype == torch.bool):
        raise TypeError(f"audio_amd: {what} must be an integer or floating-point tensor (got {t.dtype})")
    if not t.is_cuda:
        raise RuntimeError(f"audio_amd: {what} must be on an MI355X (ROCm) device, got {t.device}. "
                           "The HIP kernels have no CPU fallback.")


def _wa_rows(t: Tensor, lead, L: int) -> Tensor:
    """`t` broadcast to lead + (L,), as (rows, L) with unit stride along time and ONE row stride -- 0 for a broadcast row,
    more than L for rows of a wider tensor -- without a copy wherever the strides collapse that way."""
    e = t.expand(tuple(lead) + (L,))
    if L > 1 and e.stride(-1) != 1:
        e = e.contiguous()
    rows = 1
    for d in lead:
        rows *= d
    if e.dim() != 2:
        try:
            e = e.view(rows, L)
        except RuntimeError:
            e = e.contiguous().view(rows, L)
    if rows > 1 and e.stride(0) < 0:
        e = e.contiguous()
    return e


def _wa_stride(t: Tensor) -> int:
    return t.stride(0) if t.shape[0] > 1 else 0


def _add_noise_launch(w2: Tensor, n2: Tensor, snr1: Tensor, len1: Optional[Tensor], g2: Optional[Tensor] = None):
    """The two launches over (rows, L) operands.  Forward: (out, workspace); with a cotangent g2: ((2, rows, L) = grad_w and
    grad_n, workspace whose first `rows` elements hold the gradient to snr).  The workspace comes from torch's allocator,
    so the call can be captured in a graph."""
    rows, L = w2.shape
    lib = _lib.lib()
    ws = torch.empty((max(int(lib.aamd_add_noise_workspace(rows, L)) // 8, 1),), dtype=torch.float64, device=w2.device)
    ops = _ops()
    if ops is not None:
        if g2 is None:
            return ops.add_noise(w2, n2, snr1, len1, ws), ws
        return ops.add_noise_grad(g2, w2, n2, snr1, len1, ws), ws
    out = torch.empty((rows, L) if g2 is None else (2, rows, L), dtype=w2.dtype, device=w2.device)
    if rows * L == 0:
        return out, ws
    args = (_lib.ptr(w2), _lib.ptr(n2), _lib.ptr(g2) if g2 is not None else None, out.data_ptr(),
            out[1].data_ptr() if g2 is not None else None, ws.data_ptr(), rows, L, _wa_stride(w2), _wa_stride(n2),
            _wa_stride(g2) if g2 is not None else 0, snr1.data_ptr(), _wa_stride(snr1),
            len1.data_ptr() if len1 is not None else None, _wa_stride(len1) if len1 is not None else 0)
    mode = 0 if g2 is None else 1
    with torch.cuda.device(w2.device):
        if w2.dtype == torch.float32:
            _lib.check(lib.aamd_add_noise_f32(*args, mode, _lib.current_stream(w2.device)))
        elif w2.dtype == torch.float64:
            _lib.check(lib.aamd_add_noise_f64(*args, mode, _lib.current_stream(w2.device)))
        else:
            _lib.check(lib.aamd_add_noise_lp(*args, _SA_DTYPES[w2.dtype], mode, _lib.current_stream(w2.device)))
    return out, ws


def _add_noise_operands(waveform: Tensor, noise: Tensor, snr: Tensor, lengths: Optional[Tensor]):
    """Leading shape and the kernel's operands: (rows, L) views of waveform and noise, snr as float64 (rows,), lengths as
    int64 (rows,) -- floating lengths by a device-side ceil, which keeps `i < length`.  Nothing here waits for the device."""
    L = waveform.size(-1)
    lead = torch.broadcast_shapes(tuple(waveform.shape[:-1]), tuple(noise.shape[:-1]), tuple(snr.shape),
                                  tuple(lengths.shape) if lengths is not None else ())
    snr1 = snr.detach().to(torch.float64).expand(lead).reshape(-1)
    len1 = None
    if lengths is not None:
        ln = lengths.detach()
        ln = torch.ceil(ln).to(torch.int64) if ln.is_floating_point() else ln.to(torch.int64)
        len1 = ln.expand(lead).reshape(-1)
    return lead, L, _wa_rows(waveform.detach(), lead, L), _wa_rows(noise.detach(), lead, L), snr1, len1


def _add_noise_forward(waveform: Tensor, noise: Tensor, snr: Tensor, lengths: Optional[Tensor]) -> Tensor:
    lead, L, w2, n2, snr1, len1 = _add_noise_operands(waveform, noise, snr, lengths)
    out, _ = _add_noise_launch(w2, n2, snr1, len1)
    return out.view(tuple(lead) + (L,))


class _AddNoiseFunction(torch.autograd.Function):
    """out = w + s(w, n, snr) n.  First order: the gradient mode of the same two launches.  While the backward itself is
    recorded (create_graph) the gradients come from the differentiable composition `_diff.add_noise_grads` instead."""

    @staticmethod
    def forward(ctx, waveform, noise, snr, lengths):
        ctx.save_for_backward(waveform, noise, snr, lengths)
        return _add_noise_forward(waveform, noise, snr, lengths)

    @staticmethod
    def backward(ctx, g):
        waveform, noise, snr, lengths = ctx.saved_tensors
        if torch.is_grad_enabled():
            gw, gn, gs = _diff.add_noise_grads(g, waveform, noise, snr, lengths)
        else:
            lead, L, w2, n2, snr1, len1 = _add_noise_operands(waveform, noise, snr, lengths)
            both, ws = _add_noise_launch(w2, n2, snr1, len1, _wa_rows(g, lead, L))
            gw, gn = both[0].view(tuple(lead) + (L,)), both[1].view(tuple(lead) + (L,))
            gs = ws[:w2.shape[0]].view(tuple(lead))
        need = ctx.needs_input_grad
        return (gw.sum_to_size(waveform.shape) if need[0] else None, gn.sum_to_size(noise.shape) if need[1] else None,
                gs.sum_to_size(snr.shape).to(snr.dtype) if need[2] else None, None)


def _add_noise_eager(waveform: Tensor, noise: Tensor, snr: Tensor, lengths: Optional[Tensor] = None) -> Tensor:
    r"""Scale ``noise`` to the requested signal-to-noise ratio (dB) and add it to ``waveform`` (reference: F.add_noise).
    The energies are float64 sums over the samples below ``lengths``; the scale is formed in float64 from the reference's
    formula and rounded once; the whole row is mixed.  Leading dimensions broadcast.  Rows of zero energy give what IEEE
    arithmetic gives the formula: scale 0 (silent signal), ``inf`` (silent noise) or NaN (both).  float16 and bfloat16
    are read and written by the kernel and computed in float32.  Two launches, no temporaries, bit-reproducible."""
    if not (waveform.ndim - 1 == noise.ndim - 1 == snr.ndim and (lengths is None or lengths.ndim == snr.ndim)):
        raise ValueError("Input leading dimensions don't match.")
    L = waveform.size(-1)
    if L != noise.size(-1):
        raise ValueError(f"Length dimensions of waveform and noise don't match (got {L} and {noise.size(-1)}).")
    for t, what in ((waveform, "waveform"), (noise, "noise"), (snr, "snr")):
        if t.dtype not in _WA_FLOATS:
            raise TypeError(f"audio_amd: {what} must be float16, bfloat16, float32 or float64 (got {t.dtype})")
    if waveform.dtype != noise.dtype:
        raise TypeError(f"audio_amd: add_noise operands must share a dtype (got {waveform.dtype} and {noise.dtype})")
    _wa_require(waveform, "waveform")
    _wa_require(noise, "noise")
    _wa_require(snr, "snr")
    if lengths is not None:
        _wa_require(lengths, "lengths", floating=False)
    if torch.is_grad_enabled() and (waveform.requires_grad or noise.requires_grad or snr.requires_grad):
        return _AddNoiseFunction.apply(waveform, noise, snr, lengths)
    return _add_noise_forward(waveform, noise, snr, lengths)


def _preemphasis_launch(x2: Tensor, coeff: float, transposed: bool) -> Tensor:
    """(rows, L) of any row stride -> dense (rows, L): y[i] = x[i] - c x[i - 1] (transposed: x[i] - c x[i + 1]), one launch."""
    ops = _ops()
    if ops is not None:
        return ops.preemphasis(x2, coeff, transposed)
    out = torch.empty(x2.shape, dtype=x2.dtype, device=x2.device)
    if out.numel() == 0:
        return out
    lib = _lib.lib()
    head = (_lib.ptr(x2), out.data_ptr(), x2.shape[0], x2.shape[1], _wa_stride(x2), float(coeff))
    with torch.cuda.device(x2.device):
        if x2.dtype == torch.float32:
            _lib.check(lib.aamd_preemphasis_f32(*head, int(transposed), _lib.current_stream(x2.device)))
        elif x2.dtype == torch.float64:
            _lib.check(lib.aamd_preemphasis_f64(*head, int(transposed), _lib.current_stream(x2.device)))
        else:
            _lib.check(lib.aamd_preemphasis_lp(*head, _SA_DTYPES[x2.dtype], int(transposed), _lib.current_stream(x2.device)))
    return out


class _PreemphasisFunction(torch.autograd.Function):
    """The pre-emphasis stencil P (transposed=False) or P^T.  Linear: the backward is the other one, applied through this
    Function again, so gradients of every order run on the kernel."""

    @staticmethod
    def forward(ctx, x2, coeff, transposed):
        ctx.args = (coeff, transposed)
        return _preemphasis_launch(x2, coeff, transposed)

    @staticmethod
    def backward(ctx, g):
        coeff, transposed = ctx.args
        g2 = _wa_rows(g, g.shape[:-1], g.shape[-1])
        if torch.is_grad_enabled():
            return _PreemphasisFunction.apply(g2, coeff, not transposed), None, None
        return _preemphasis_launch(g2, coeff, not transposed), None, None


def _preemphasis_eager(waveform: Tensor, coeff: float = 0.97) -> Tensor:
    r"""``y[i] = x[i] - coeff * x[i - 1]`` along the last dim, ``y[0] = x[0]`` (reference: F.preemphasis).  ``coeff`` is
    rounded to the compute type and the product and the difference are rounded separately, so float32 and float64 results
    equal the reference's expression bit for bit; float16 and bfloat16 compute in float32 and round once.  Rows are read in
    place through their stride; the result is a new contiguous tensor."""
    _wa_require(waveform, "waveform")
    if waveform.dim() < 1:
        raise ValueError("audio_amd: preemphasis expects (..., time), got a 0-dimensional tensor")
    shape = waveform.shape
    x2 = _wa_rows(waveform, shape[:-1], shape[-1])
    if torch.is_grad_enabled() and waveform.requires_grad:
        out = _PreemphasisFunction.apply(x2, float(coeff), False)
    else:
        out = _preemphasis_launch(x2, float(coeff), False)
    return out.view(shape)


def _deemphasis_eager(waveform: Tensor, coeff: float = 0.97) -> Tensor:
    r"""The inverse of pre-emphasis, ``y[i] = x[i] + coeff * y[i - 1]`` (reference: F.deemphasis): ``lfilter`` with
    ``a = [1, -coeff]``, ``b = [1, 0]`` and its default clamp to [-1, 1]; gradients are lfilter's."""
    _wa_require(waveform, "waveform")
    dtype = waveform.dtype
    coef = torch.stack([_cpu_scalar(v, dtype) for v in (1.0, -coeff, 1.0, 0.0)]).to(waveform.device)
    return lfilter(waveform, coef[:2], coef[2:])


# --------------------------------------------------------------------------- #
# MVDR beamforming (csrc/beamform.h)                                          #
# --------------------------------------------------------------------------- #

BEAMFORM_MAX_CHANNELS = 16      # bf::kMaxC
_BF_DTYPES = {torch.complex64: 0, torch.complex128: 1}
_BF_REAL = {torch.complex64: torch.float32, torch.complex128: torch.float64}
_BF_SOLVE, _BF_SOUDEN, _BF_RTF, _BF_RTF_POWER = 0, 1, 2, 3


def beamform_tiles() -> Tuple[int, int]:
    """(frequencies per workgroup, largest time chunk) of the PSD kernel (bf::kFT, bf::kTCMax)."""
    lib = _lib.lib()
    return int(lib.aamd_beamform_freq_tile()), int(lib.aamd_beamform_time_chunk())


def _bf_require(t: Tensor, what: str) -> None:
    if t.dtype not in _BF_DTYPES:
        raise TypeError(f"audio_amd: {what} must be complex64 or complex128 (got {t.dtype})")
    if not t.is_cuda:
        raise RuntimeError(f"audio_amd: {what} must be on an MI355X (ROCm) device, got {t.device}. "
                           "The HIP kernels have no CPU fallback.")


def _bf_channels(c: int) -> None:
    if c > BEAMFORM_MAX_CHANNELS:
        raise NotImplementedError(f"audio_amd: beamforming kernels take up to {BEAMFORM_MAX_CHANNELS} channels (got {c})")


def _bf_wants_grad(*tensors) -> bool:
    return torch.is_grad_enabled() and any(isinstance(t, Tensor) and t.requires_grad for t in tensors)


def _bf_frame_major(x4: Tensor) -> bool:
    """The unit-stride axis of a (B, C, F, T) view the kernels accept: True = freq (bf_view of csrc/api_post.hip)."""
    F_, T_ = x4.shape[2], x4.shape[3]
    sf, st = (x4.stride(2) if F_ > 1 else 1), (x4.stride(3) if T_ > 1 else 1)
    return False if st == 1 else (True if sf == 1 else T_ > 1)


def _bf_spec(specgram: Tensor):
    """(..., C, F, T) -> (leading shape, (B, C, F, T) view).  Unit stride along freq (the frame-major view that
    Spectrogram(power=None) returns) or along time is read in place; anything else is gathered into a contiguous tensor."""
    lead = tuple(specgram.shape[:-3])
    x4 = specgram.detach().resolve_conj().reshape((-1,) + tuple(specgram.shape[-3:]))
    F_, T_ = x4.shape[2], x4.shape[3]
    if not (T_ <= 1 or F_ <= 1 or x4.stride(3) == 1 or x4.stride(2) == 1):
        x4 = x4.contiguous()
    return lead, x4


def _bf_strides(t: Tensor):
    return (C.c_int64 * t.dim())(*[t.stride(d) if t.shape[d] > 1 else 0 for d in range(t.dim())])


def _bf_spec_strides(x4: Tensor):
    return [x4.stride(d) if x4.shape[d] > 1 else (1 if d == 3 else 0) for d in range(4)]


def _bf_mask3(mask: Tensor, x4: Tensor) -> Tensor:
    return mask.detach().to(_BF_REAL[x4.dtype]).reshape(x4.shape[0], x4.shape[2], x4.shape[3])


def _bf_psd_launch(x4: Tensor, m1: Optional[Tensor], m2: Optional[Tensor], normalize: bool, eps: float) -> Tensor:
    """(B, C, F, T) and none, one or two (B, F, T) masks -> (n, B, F, C, C), one launch."""
    B, Cc, F_, T_ = x4.shape
    n = 2 if m2 is not None else 1
    ops = _ops()
    if ops is not None:
        return torch.view_as_complex(ops.beamform_psd(torch.view_as_real(x4), m1, m2, bool(normalize), float(eps)))
    out = torch.empty((n, B, F_, Cc, Cc), dtype=x4.dtype, device=x4.device)
    if out.numel() == 0:
        return out
    if T_ == 0:
        return out.zero_()
    lib = _lib.lib()
    with torch.cuda.device(x4.device):
        _lib.check(lib.aamd_beamform_psd(_BF_DTYPES[x4.dtype], _lib.ptr(x4), B, Cc, F_, T_, *_bf_spec_strides(x4),
                                         _lib.ptr(m1) if m1 is not None else None, _bf_strides(m1) if m1 is not None else None,
                                         _lib.ptr(m2) if m2 is not None else None, _bf_strides(m2) if m2 is not None else None,
                                         int(bool(normalize)), float(eps), out.data_ptr(), _lib.current_stream(x4.device)))
    return out


def _bf_weights_launch(mode: int, a3: Tensor, b: Tensor, u2: Optional[Tensor], batch: int, freq: int, ref: int, loading: bool,
                       diag_eps: float, eps: float, n_iter: int = 0, adjoint: bool = False) -> Tensor:
    """The per-bin solve: a3 (bins, C, C), b (bins, C, K) or (bins, C), u2 (batch, C) or None -> (bins, C, K) or (bins, C)."""
    ops = _ops()
    if ops is not None:
        return torch.view_as_complex(ops.beamform_weights(mode, torch.view_as_real(a3), torch.view_as_real(b),
                                                          torch.view_as_real(u2) if u2 is not None else None, batch, freq, ref,
                                                          bool(loading), float(diag_eps), float(eps), n_iter, adjoint))
    bins, Cc = a3.shape[0], a3.shape[1]
    K = 1 if mode == _BF_RTF else b.shape[2]
    out = torch.empty(tuple(b.shape) if mode == _BF_SOLVE else (bins, Cc), dtype=a3.dtype, device=a3.device)
    if out.numel() == 0:
        return out
    lib = _lib.lib()
    with torch.cuda.device(a3.device):
        _lib.check(lib.aamd_beamform_weights(_BF_DTYPES[a3.dtype], mode, _lib.ptr(a3), _lib.ptr(b),
                                             _lib.ptr(u2) if u2 is not None else None, out.data_ptr(), batch, freq, Cc, K, ref,
                                             int(bool(loading)), float(diag_eps), float(eps), n_iter, int(adjoint),
                                             _lib.current_stream(a3.device)))
    return out


def _bf_apply_launch(w3: Tensor, x4: Tensor) -> Tensor:
    """(B, F, C) weights and a (B, C, F, T) view -> (B, F, T) in the input's (freq, time) stride order, one launch."""
    B, Cc, F_, T_ = x4.shape
    fm = _bf_frame_major(x4)
    ops = _ops()
    if ops is not None:
        out = torch.view_as_complex(ops.beamform_apply(torch.view_as_real(w3), torch.view_as_real(x4), fm))
        return out.transpose(1, 2) if fm else out
    out = torch.empty((B, T_, F_) if fm else (B, F_, T_), dtype=x4.dtype, device=x4.device)
    res = out.transpose(1, 2) if fm else out
    if out.numel() == 0:
        return res
    lib = _lib.lib()
    so = (C.c_int64 * 3)(F_ * T_, 1 if fm else T_, F_ if fm else 1)
    with torch.cuda.device(x4.device):
        _lib.check(lib.aamd_beamform_apply(_BF_DTYPES[x4.dtype], _lib.ptr(w3), _lib.ptr(x4), B, Cc, F_, T_, *_bf_spec_strides(x4),
                                           out.data_ptr(), so, _lib.current_stream(x4.device)))
    return res


def _bf_check_mask(specgram: Tensor, mask: Tensor, what: str = "mask") -> None:
    want = tuple(specgram.shape[:-3]) + tuple(specgram.shape[-2:])
    if tuple(mask.shape) != want:
        raise ValueError(f"The shape of {what} must be the specgram's without the channel dimension: expected {want}, "
                         f"got {tuple(mask.shape)}.")
    if mask.is_complex():
        raise TypeError(f"audio_amd: {what} must be a real tensor (got {mask.dtype})")
    if mask.device != specgram.device:
        raise RuntimeError(f"audio_amd: {what} must be on the specgram's device")


def _psd_pair_eager(specgram: Tensor, mask_s: Tensor, mask_n: Tensor, normalize: bool = True, eps: float = 1e-10) -> Tensor:
    """Both PSD matrices of T.MVDR, stacked as (2, ..., freq, ch, ch): one launch reads the spectrogram once."""
    if specgram.dim() < 3:
        raise ValueError(f"Expected at least 3D tensor (..., channel, freq, time). Found: {tuple(specgram.shape)}")
    _bf_check_mask(specgram, mask_s, "mask_s")
    _bf_check_mask(specgram, mask_n, "mask_n")
    _bf_channels(specgram.shape[-3])
    _bf_require(specgram, "specgram")
    if _bf_wants_grad(specgram, mask_s, mask_n):
        return torch.stack([_diff.bf_psd(specgram, mask_s, normalize, eps), _diff.bf_psd(specgram, mask_n, normalize, eps)])
    lead, x4 = _bf_spec(specgram)
    out = _bf_psd_launch(x4, _bf_mask3(mask_s, x4), _bf_mask3(mask_n, x4), normalize, eps)
    return out.view((2,) + lead + tuple(out.shape[2:]))


def _psd_eager(specgram: Tensor, mask: Optional[Tensor] = None, normalize: bool = True, eps: float = 1e-10) -> Tensor:
    r"""Power spectral density matrix of a multi-channel complex spectrogram ``(..., ch, freq, time)`` (reference: F.psd):
    ``psd[f] = sum_t m'[f, t] x[:, f, t] x[:, f, t]^H`` with ``m' = mask / (mask.sum(time) + eps)`` when ``normalize``,
    the plain sum without a mask.  One launch and one pass, no ``(..., time, ch, ch)`` temporary; float64 sums in a fixed
    order, so two calls give the same bits; the result ``(..., freq, ch, ch)`` is exactly Hermitian."""
    if specgram.dim() < 3:
        raise ValueError(f"Expected at least 3D tensor (..., channel, freq, time). Found: {tuple(specgram.shape)}")
    if mask is not None:
        _bf_check_mask(specgram, mask)
    _bf_channels(specgram.shape[-3])
    _bf_require(specgram, "specgram")
    if _bf_wants_grad(specgram, mask):
        return _diff.bf_psd(specgram, mask, normalize, eps)
    lead, x4 = _bf_spec(specgram)
    out = _bf_psd_launch(x4, _bf_mask3(mask, x4) if mask is not None else None, None, normalize, eps)
    return out.view(lead + tuple(out.shape[2:]))


def _assert_psd_matrices(psd_s: Tensor, psd_n: Tensor) -> None:
    if psd_s.ndim < 3 or psd_n.ndim < 3:
        raise ValueError("Expected at least 3D Tensor (..., channel, channel) for psd_s and psd_n. "
                         f"Found {tuple(psd_s.shape)} for psd_s and {tuple(psd_n.shape)} for psd_n.")
    if not (psd_s.is_complex() and psd_n.is_complex()):
        raise TypeError("The type of psd_s and psd_n must be ``torch.cfloat`` or ``torch.cdouble``. "
                        f"Found {psd_s.dtype} for psd_s and {psd_n.dtype} for psd_n.")
    if psd_s.shape != psd_n.shape:
        raise ValueError(f"The dimensions of psd_s and psd_n should be the same. Found {tuple(psd_s.shape)} and {tuple(psd_n.shape)}.")
    if psd_s.shape[-1] != psd_s.shape[-2]:
        raise ValueError(f"The last two dimensions of psd_s should be the same. Found {tuple(psd_s.shape)}.")


def _bf_reference(reference_channel, psd: Tensor, optional: bool = False):
    """(index or -1, (batch, C) complex tensor or None) of an int / Tensor reference for PSD matrices (..., F, C, C)."""
    Cc = psd.shape[-1]
    if reference_channel is None and optional:
        return -1, None
    if isinstance(reference_channel, Tensor):
        lead = tuple(psd.shape[:-3])
        if tuple(reference_channel.shape) != lead + (Cc,):
            raise ValueError(f"Expected a reference vector of shape {lead + (Cc,)}, got {tuple(reference_channel.shape)}.")
        if reference_channel.device != psd.device:
            raise RuntimeError("audio_amd: reference_channel must be on the PSD matrices' device")
        return -1, reference_channel.detach().to(psd.dtype).reshape(-1, Cc).contiguous()
    if isinstance(reference_channel, int) and not isinstance(reference_channel, bool):
        if not -Cc <= reference_channel < Cc:
            raise IndexError(f"reference_channel {reference_channel} is out of range for {Cc} channels")
        return reference_channel % Cc, None
    raise RuntimeError(f'Expected "int" or "Tensor" for reference_channel. Found: {type(reference_channel)}.')


def _bf_bins(psd: Tensor):
    """(..., F, C, C) -> (batch, F, contiguous (bins, C, C))."""
    Cc, F_ = psd.shape[-1], psd.shape[-3]
    a3 = psd.detach().resolve_conj().reshape(-1, Cc, Cc).contiguous()
    return a3.shape[0] // F_ if F_ else 0, F_, a3


def _mvdr_weights_souden_eager(psd_s: Tensor, psd_n: Tensor, reference_channel, diagonal_loading: bool = True,
                               diag_eps: float = 1e-7, eps: float = 1e-8) -> Tensor:
    r"""MVDR weights by Souden's method (reference: F.mvdr_weights_souden): ``W = N / (tr N + eps)`` with
    ``N = psd_n^-1 psd_s`` (``psd_n`` loaded with ``(Re tr psd_n * diag_eps + 1e-8) I`` first), column ``reference_channel``
    of it or ``W u`` for a vector.  One launch: an LU solve with partial pivoting per (batch, freq) bin, in float64."""
    _assert_psd_matrices(psd_s, psd_n)
    _bf_channels(psd_s.shape[-1])
    _bf_require(psd_s, "psd_s")
    _bf_require(psd_n, "psd_n")
    if psd_s.dtype != psd_n.dtype:
        raise TypeError(f"audio_amd: psd_s and psd_n must share a dtype (got {psd_s.dtype} and {psd_n.dtype})")
    ref, u = _bf_reference(reference_channel, psd_n)
    if _bf_wants_grad(psd_s, psd_n, reference_channel):
        return _diff.bf_souden(psd_s, psd_n, reference_channel, diagonal_loading, diag_eps, eps)
    batch, F_, a3 = _bf_bins(psd_n)
    out = _bf_weights_launch(_BF_SOUDEN, a3, _bf_bins(psd_s)[2], u, batch, F_, ref, diagonal_loading, diag_eps, eps)
    return out.view(tuple(psd_n.shape[:-1]))


def _mvdr_weights_rtf_eager(rtf: Tensor, psd_n: Tensor, reference_channel=None, diagonal_loading: bool = True,
                            diag_eps: float = 1e-7, eps: float = 1e-8) -> Tensor:
    r"""MVDR weights from a relative transfer function (reference: F.mvdr_weights_rtf): ``w = n / (Re(r^H n) + eps)`` with
    ``n = psd_n^-1 r``, times ``conj(r[ref])`` (or ``sum_c conj(r_c) u_c``) when a reference is given.  One launch."""
    if rtf.ndim < 2:
        raise ValueError(f"Expected at least 2D Tensor (..., freq, channel) for rtf. Found {tuple(rtf.shape)}.")
    if psd_n.ndim < 3:
        raise ValueError(f"Expected at least 3D Tensor (..., freq, channel, channel) for psd_n. Found {tuple(psd_n.shape)}.")
    if not (rtf.is_complex() and psd_n.is_complex()):
        raise TypeError("The type of rtf and psd_n must be ``torch.cfloat`` or ``torch.cdouble``. "
                        f"Found {rtf.dtype} for rtf and {psd_n.dtype} for psd_n.")
    if rtf.shape != psd_n.shape[:-1]:
        raise ValueError("The dimensions of rtf and the dimensions without the last dimension of psd_n should be the same. "
                         f"Found {tuple(rtf.shape)} for rtf and {tuple(psd_n.shape)} for psd_n.")
    if psd_n.shape[-1] != psd_n.shape[-2]:
        raise ValueError(f"The last two dimensions of psd_n should be the same. Found {tuple(psd_n.shape)}.")
    _bf_channels(psd_n.shape[-1])
    _bf_require(rtf, "rtf")
    _bf_require(psd_n, "psd_n")
    if rtf.dtype != psd_n.dtype:
        raise TypeError(f"audio_amd: rtf and psd_n must share a dtype (got {rtf.dtype} and {psd_n.dtype})")
    ref, u = _bf_reference(reference_channel, psd_n, optional=True)
    if _bf_wants_grad(rtf, psd_n, reference_channel):
        return _diff.bf_rtf(rtf, psd_n, reference_channel, diagonal_loading, diag_eps, eps)
    batch, F_, a3 = _bf_bins(psd_n)
    r2 = rtf.detach().resolve_conj().reshape(-1, rtf.shape[-1]).contiguous()
    out = _bf_weights_launch(_BF_RTF, a3, r2, u, batch, F_, ref, diagonal_loading, diag_eps, eps)
    return out.view(tuple(rtf.shape))


def _rtf_power_eager(psd_s: Tensor, psd_n: Tensor, reference_channel, n_iter: int = 3, diagonal_loading: bool = True,
                     diag_eps: float = 1e-7) -> Tensor:
    r"""Relative transfer function by the power method (reference: F.rtf_power): ``phi = psd_n^-1 psd_s`` (loaded ``psd_n``),
    ``r = phi[:, ref]`` (or ``phi u``), ``n_iter - 2`` times ``r <- phi r``, then ``r <- psd_s r``; ``n_iter == 1`` multiplies
    by the loaded ``psd_n`` instead.  One launch."""
    _assert_psd_matrices(psd_s, psd_n)
    if n_iter <= 0:
        raise ValueError(f"The number of iteration must be greater than 0. Found {n_iter}.")
    _bf_channels(psd_s.shape[-1])
    _bf_require(psd_s, "psd_s")
    _bf_require(psd_n, "psd_n")
    if psd_s.dtype != psd_n.dtype:
        raise TypeError(f"audio_amd: psd_s and psd_n must share a dtype (got {psd_s.dtype} and {psd_n.dtype})")
    ref, u = _bf_reference(reference_channel, psd_n)
    if _bf_wants_grad(psd_s, psd_n, reference_channel):
        return _diff.bf_rtf_power(psd_s, psd_n, reference_channel, n_iter, diagonal_loading, diag_eps)
    batch, F_, a3 = _bf_bins(psd_n)
    out = _bf_weights_launch(_BF_RTF_POWER, a3, _bf_bins(psd_s)[2], u, batch, F_, ref, diagonal_loading, diag_eps, 0.0, int(n_iter))
    return out.view(tuple(psd_n.shape[:-1]))


def _apply_beamforming_eager(beamform_weights: Tensor, specgram: Tensor) -> Tensor:
    r"""``y[f, t] = sum_c conj(w[f, c]) x[c, f, t]`` (reference: F.apply_beamforming): weights ``(..., freq, ch)``, spectrogram
    ``(..., ch, freq, time)``, result ``(..., freq, time)`` in the spectrogram's (freq, time) stride order -- a frame-major
    input gives a frame-major output, which ``InverseSpectrogram`` takes as it is.  One streaming launch."""
    if specgram.dim() < 3:
        raise ValueError(f"Expected at least 3D tensor (..., channel, freq, time). Found: {tuple(specgram.shape)}")
    if beamform_weights.shape[:-2] != specgram.shape[:-3]:
        raise ValueError("The dimensions except the last two dimensions of beamform_weights should be the same as the "
                         f"dimensions except the last three dimensions of specgram. Found {tuple(beamform_weights.shape)} for "
                         f"beamform_weights and {tuple(specgram.shape)} for specgram.")
    if beamform_weights.shape[-2:] != (specgram.shape[-2], specgram.shape[-3]):
        raise ValueError(f"Expected beamform_weights (..., freq, channel) = {(specgram.shape[-2], specgram.shape[-3])}, "
                         f"got {tuple(beamform_weights.shape[-2:])}.")
    if not (beamform_weights.is_complex() and specgram.is_complex()):
        raise TypeError("The type of beamform_weights and specgram must be ``torch.cfloat`` or ``torch.cdouble``. "
                        f"Found {beamform_weights.dtype} for beamform_weights and {specgram.dtype} for specgram.")
    _bf_channels(specgram.shape[-3])
    _bf_require(beamform_weights, "beamform_weights")
    _bf_require(specgram, "specgram")
    if beamform_weights.dtype != specgram.dtype:
        raise TypeError(f"audio_amd: beamform_weights and specgram must share a dtype (got {beamform_weights.dtype} and "
                        f"{specgram.dtype})")
    if _bf_wants_grad(beamform_weights, specgram):
        return _diff.bf_apply(beamform_weights, specgram)
    lead, x4 = _bf_spec(specgram)
    w3 = beamform_weights.detach().resolve_conj().reshape((-1,) + tuple(beamform_weights.shape[-2:])).contiguous()
    out = _bf_apply_launch(w3, x4)
    if len(lead) == 1:
        return out
    if not lead:
        return out[0]
    fm = out.stride(1) == 1 and out.shape[1] > 1
    if fm:
        return out.transpose(1, 2).reshape(lead + (out.shape[2], out.shape[1])).transpose(-1, -2)
    return out.reshape(lead + tuple(out.shape[1:]))


def rtf_evd(psd_s: Tensor) -> Tensor:
    r"""Not part of this package yet: the eigenvalue-decomposition RTF needs a Hermitian eigen-solver kernel."""
    raise NotImplementedError("audio_amd: rtf_evd is not implemented: it needs a Hermitian eigen-solver kernel, which this "
                              "package does not have yet; use rtf_power")


# --------------------------------------------------------------------------- #
# RNN transducer loss (csrc/rnnt_loss.h)                                      #
# --------------------------------------------------------------------------- #
_RNNT_DTYPES = {torch.float32: 0, torch.float64: 1, torch.float16: 2, torch.bfloat16: 3}      # AAMD_SA_*
RNNT_MAX_U1 = 1024                   # AAMD_RNNT_MAX_U1: the longest target axis (U + 1) the lattice kernel serves


def rnnt_tiles() -> Tuple[Tuple[int, ...], int, int]:
    """(team widths of the row and gradient passes, threads of a lattice workgroup, largest U + 1) of csrc/rnnt_loss.h."""
    lib = _lib.lib()
    widths = sorted({int(lib.aamd_rnnt_team_width(0, 1 << k)) for k in range(12)})
    return tuple(widths), int(lib.aamd_rnnt_lattice_threads()), RNNT_MAX_U1


def rnnt_team_width(dtype: torch.dtype, vocab: int) -> int:
    """Lanes per (b, t, u) row that the launcher picks for a vocabulary of ``vocab`` entries of ``dtype``."""
    return int(_lib.lib().aamd_rnnt_team_width(_RNNT_DTYPES[dtype], int(vocab)))


def _rnnt_check(logits: Tensor, targets: Tensor, logit_lengths: Tensor, target_lengths: Tensor, blank: int,
                reduction: str) -> int:
    """The host-side checks of F.rnnt_loss; returns the blank index counted from the front."""
    if reduction not in ("none", "mean", "sum"):
        raise ValueError("reduction should be one of 'none', 'mean', or 'sum'")
    if logits.dim() != 4:
        raise ValueError(f"logits must be 4-D (batch, time, target + 1, class), got {tuple(logits.shape)}")
    if targets.dim() != 2:
        raise ValueError(f"targets must be 2-D (batch, target), got {tuple(targets.shape)}")
    if logit_lengths.dim() != 1 or target_lengths.dim() != 1:
        raise ValueError("logit_lengths and target_lengths must be 1-D (batch,)")
    B, T_, U1, V = logits.shape
    if targets.shape[0] != B or logit_lengths.shape[0] != B or target_lengths.shape[0] != B:
        raise ValueError(f"batch sizes differ: logits {B}, targets {targets.shape[0]}, logit_lengths {logit_lengths.shape[0]}, "
                         f"target_lengths {target_lengths.shape[0]}")
    if targets.shape[1] + 1 != U1:
        raise ValueError(f"logits dimension 2 must be targets dimension 1 plus one (got {U1} and {targets.shape[1]})")
    if T_ < 1 or V < 1:
        raise ValueError(f"logits needs at least one frame and one class, got {tuple(logits.shape)}")
    if logits.dtype not in _RNNT_DTYPES:
        raise TypeError(f"logits must be float32, float64, float16 or bfloat16 (got {logits.dtype})")
    for t, what in ((targets, "targets"), (logit_lengths, "logit_lengths"), (target_lengths, "target_lengths")):
        if t.dtype != torch.int32:
            raise TypeError(f"{what} must be int32 (got {t.dtype})")
    for t, what in ((logits, "logits"), (targets, "targets"), (logit_lengths, "logit_lengths"),
                    (target_lengths, "target_lengths")):
        if not t.is_contiguous():
            raise ValueError(f"{what} must be contiguous")
    bl = blank + V if blank < 0 else blank
    if not 0 <= bl < V:
        raise ValueError(f"blank must lie in [-{V}, {V}) for {V} classes (got {blank})")
    if U1 > RNNT_MAX_U1:
        raise NotImplementedError(f"audio_amd: rnnt_loss serves targets up to U + 1 = {RNNT_MAX_U1} (got {U1}): the lattice of one "
                                  "example belongs to one workgroup")
    for t, what in ((logits, "logits"), (targets, "targets"), (logit_lengths, "logit_lengths"),
                    (target_lengths, "target_lengths")):
        if not t.is_cuda:
            raise RuntimeError(f"audio_amd: {what} must be on an MI355X (ROCm) device, got {t.device}. "
                               "The HIP kernels have no CPU fallback.")
        if t.device != logits.device:
            raise RuntimeError(f"audio_amd: {what} must be on the logits' device")
    return bl


def _rnnt_forward_launch(logits: Tensor, targets: Tensor, logit_lengths: Tensor, target_lengths: Tensor, blank: int,
                         fused: bool) -> Tuple[Tensor, Tensor]:
    """(costs (B,) float64, workspace): the row pass and the lattice.  Nothing is read back: lengths stay on the device."""
    B, T_, U1, V = logits.shape
    lib = _lib.lib()
    ws = torch.empty((max(int(lib.aamd_rnnt_loss_workspace(B, T_, U1)) // 8, 1),), dtype=torch.float64, device=logits.device)
    ops = _ops()
    if ops is not None:
        return ops.rnnt_loss_forward(logits, targets, logit_lengths, target_lengths, blank, bool(fused), ws), ws
    costs = torch.empty((B,), dtype=torch.float64, device=logits.device)
    if B:
        with torch.cuda.device(logits.device):
            _lib.check(lib.aamd_rnnt_loss_forward(_RNNT_DTYPES[logits.dtype], _lib.ptr(logits), _lib.ptr(targets) or None,
                                                  _lib.ptr(logit_lengths), _lib.ptr(target_lengths), B, T_, U1, V, blank,
                                                  int(bool(fused)), ws.data_ptr(), costs.data_ptr(),
                                                  _lib.current_stream(logits.device)))
    return costs, ws


def _rnnt_backward_launch(logits: Tensor, targets: Tensor, logit_lengths: Tensor, target_lengths: Tensor, blank: int,
                          fused: bool, clamp: float, ws: Tensor, grad_costs: Tensor) -> Tensor:
    """d costs / d logits (clamped) times grad_costs (B,) float64: one read of logits, one write of the result."""
    B, T_, U1, V = logits.shape
    ops = _ops()
    if ops is not None:
        return ops.rnnt_loss_backward(logits, targets, logit_lengths, target_lengths, blank, bool(fused), float(clamp), ws,
                                      grad_costs)
    grad = torch.empty_like(logits)
    if B:
        with torch.cuda.device(logits.device):
            _lib.check(_lib.lib().aamd_rnnt_loss_backward(_RNNT_DTYPES[logits.dtype], _lib.ptr(logits), _lib.ptr(targets) or None,
                                                          _lib.ptr(logit_lengths), _lib.ptr(target_lengths), B, T_, U1, V, blank,
                                                          int(bool(fused)), float(clamp), ws.data_ptr(), grad_costs.data_ptr(),
                                                          grad.data_ptr(), _lib.current_stream(logits.device)))
    return grad


class _RNNTLossFunction(torch.autograd.Function):
    """Costs (B,) in the dtype of logits.  What is kept for backward is logits itself and the float64 workspaces of
    B * T * (U + 1) cells; the gradient is formed in backward, once: a second derivative raises."""

    @staticmethod
    def forward(ctx, logits, targets, logit_lengths, target_lengths, blank, clamp, fused):
        costs, ws = _rnnt_forward_launch(logits, targets, logit_lengths, target_lengths, blank, fused)
        ctx.save_for_backward(logits, targets, logit_lengths, target_lengths, ws)
        ctx.rnnt = (blank, clamp, fused)
        return costs.to(logits.dtype)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_costs):
        logits, targets, logit_lengths, target_lengths, ws = ctx.saved_tensors
        blank, clamp, fused = ctx.rnnt
        grad = _rnnt_backward_launch(logits, targets, logit_lengths, target_lengths, blank, fused, clamp, ws,
                                     grad_costs.to(torch.float64).contiguous())
        return grad, None, None, None, None, None, None


def _rnnt_loss_eager(logits: Tensor, targets: Tensor, logit_lengths: Tensor, target_lengths: Tensor, blank: int = -1,
                     clamp: float = -1.0, reduction: str = "mean", fused_log_softmax: bool = True) -> Tensor:
    r"""RNN transducer loss (reference: F.rnnt_loss, a compiled extension there).  ``logits`` ``(B, T, U + 1, V)``, ``targets``
    ``(B, U)`` int32, ``logit_lengths`` / ``target_lengths`` ``(B,)`` int32.  Forward is one streaming read of ``logits`` (online
    log-sum-exp per ``(b, t, u)`` row, the padding of ragged batches not read) and a float64 alpha / beta lattice per example;
    backward is one read of ``logits`` and one write of the gradient, and nothing of that size is kept in between.  float16 /
    bfloat16 are read and written directly with float32 arithmetic; float64 is the precision path.  Lengths and targets are
    read on the device -- no synchronisation, so the call can be captured in a graph -- and an example with an impossible
    length or label gets a NaN cost and a NaN gradient block instead of the reference's host-side error."""
    bl = _rnnt_check(logits, targets, logit_lengths, target_lengths, blank, reduction)
    if torch.is_grad_enabled() and logits.requires_grad:
        costs = _RNNTLossFunction.apply(logits, targets, logit_lengths, target_lengths, bl, float(clamp), bool(fused_log_softmax))
    else:
        costs = _rnnt_forward_launch(logits.detach(), targets, logit_lengths, target_lengths, bl,
                                     bool(fused_log_softmax))[0].to(logits.dtype)
    if reduction == "mean":
        return costs.mean()
    if reduction == "sum":
        return costs.sum()
    return costs


# --------------------------------------------------------------------------- #
# SoX-style effects (csrc/effects.h)                                          #
# --------------------------------------------------------------------------- #
PHASER_MAX_RING = 512                # AAMD_PHASER_MAX_RING: the longest delay ring (samples) the phaser kernel serves
FLANGER_MAX_RING = 4096              # AAMD_FLANGER_MAX_RING: 40 ms at 96 kHz
EFFECTS_MAX_TABLE = 1 << 24          # AAMD_EFFECTS_MAX_TABLE: the longest modulation table
_FX_OVERDRIVE, _FX_PHASER, _FX_FLANGER = 0, 1, 2
_FX_TABLES: "collections.OrderedDict" = collections.OrderedDict()   # (parameters, device) -> device table, LRU
_FX_PINNED: dict = {}                # tables a captured graph reads: kept for the life of the process
_FX_TABLES_MAX = 64


def effects_tiles() -> Tuple[int, int, int]:
    """(rows per workgroup, samples per LDS tile) of the delay-line kernel and the samples per overdrive chunk
    (csrc/effects.h: fx::kRows, fx::kTile, fx::kOdChunk)."""
    lib = _lib.lib()
    return int(lib.aamd_effects_tiles(0)), int(lib.aamd_effects_tiles(1)), int(lib.aamd_effects_tiles(2))


def _fx_table(key, device, make) -> Tensor:
    """The modulation table of `key` on `device`: built on the host (float64) and uploaded once.  A table is never allocated
    from a capture's pool: the first call with these parameters must run eagerly."""
    k = key + (str(device),)
    capturing = torch.cuda.is_current_stream_capturing()
    with _CACHE_LOCK:
        t = _FX_PINNED.get(k)
        if t is None:
            t = _FX_TABLES.get(k)
            if t is not None:
                _FX_TABLES.move_to_end(k)
                if capturing:
                    _FX_PINNED[k] = t
    if t is not None:
        return t
    if capturing:
        raise RuntimeError("audio_amd: the modulation table of these effect parameters is not on the device yet and cannot be "
                           "built inside a graph capture; run the call once eagerly before capturing it")
    t = torch.from_numpy(make()).to(device)
    with _CACHE_LOCK:
        t = _FX_TABLES.setdefault(k, t)
        _FX_TABLES.move_to_end(k)
        while len(_FX_TABLES) > _FX_TABLES_MAX:
            _FX_TABLES.popitem(last=False)
    return t


def _fx_check_type(waveform: Tensor, what: str) -> None:
    if not isinstance(waveform, Tensor):
        raise TypeError(f"audio_amd: {what}: waveform must be a tensor")
    if waveform.dtype not in _WA_FLOATS:
        raise TypeError(f"audio_amd: {what}: waveform must be float16, bfloat16, float32 or float64 (got {waveform.dtype})")


def _fx_check_device(waveform: Tensor, what: str) -> None:
    """After the checks of the parameters, which need no device: the refusal of a gradient and of a CPU tensor."""
    if waveform.requires_grad and torch.is_grad_enabled():
        raise RuntimeError(f"audio_amd: {what} is forward-only (no gradient is implemented); wrap the call in torch.no_grad() "
                           "or detach the waveform.")
    _wa_require(waveform, f"{what}: waveform")


def _fx_rows(waveform: Tensor) -> Tuple[Tensor, int, int]:
    """(rows, T) view through one row stride (gathered where the strides do not collapse), rows, T."""
    shape = tuple(waveform.shape)
    x2 = _wa_rows(waveform.detach(), shape[:-1], shape[-1])
    return x2, x2.shape[0], x2.shape[1]


def _fx_workspace(effect: int, x2: Tensor, ring: int) -> Tensor:
    n = int(_lib.lib().aamd_effects_workspace(effect, _SA_DTYPES[x2.dtype], x2.shape[0], x2.shape[1], ring))
    return torch.empty(((max(n, 16) + 7) // 8,), dtype=torch.float64, device=x2.device)


def overdrive(waveform: Tensor, gain: float = 20, colour: float = 20) -> Tensor:
    r"""Overdrive (reference: F.overdrive, SoX's effect): ``t = x * 10 ** (gain / 20) + colour / 200`` soft-clipped to
    ``+-2/3`` (``t - t**3 / 3`` in between), ``y[i] = t[i] - t[i-1] + 0.995 y[i-1]``, ``out = clamp(x / 2 + 0.75 y, -1, 1)``
    along the last dim of ``(..., time)``.  The reference is a Python loop over samples; here the recurrence is a chunked scan
    in two launches with a float64 state for every dtype, so results agree with the reference to rounding, not bit for bit.
    Deterministic; forward-only; a plain Python entry point through the C ABI (not registered as a dispatcher op).  Can be
    captured in a graph."""
    _fx_check_type(waveform, "overdrive")
    if waveform.dim() < 1:
        raise ValueError("audio_amd: overdrive expects (..., time), got a 0-dimensional tensor")
    _fx_check_device(waveform, "overdrive")
    out = torch.empty(tuple(waveform.shape), dtype=waveform.dtype, device=waveform.device)
    if out.numel() == 0:
        return out
    x2, rows, T_ = _fx_rows(waveform)
    ws = _fx_workspace(_FX_OVERDRIVE, x2, 0)
    with torch.cuda.device(waveform.device):
        _lib.check(_lib.lib().aamd_overdrive(_SA_DTYPES[x2.dtype], x2.data_ptr(), out.data_ptr(), ws.data_ptr(), rows, T_,
                                             _wa_stride(x2), math.exp(float(gain) * math.log(10) / 20.0), float(colour) / 200,
                                             _lib.current_stream(waveform.device)))
    return out


def phaser(waveform: Tensor, sample_rate: int, gain_in: float = 0.4, gain_out: float = 0.74, delay_ms: float = 3.0,
           decay: float = 0.4, mod_speed: float = 0.5, sinusoidal: bool = True) -> Tensor:
    r"""Phaser (reference: F.phaser, SoX's effect) along the last dim of ``(..., time)``: a delay line of
    ``L = int(delay_ms * sample_rate / 1000 + 0.5)`` samples whose feedback tap is swept by a sine or triangle table of
    ``int(sample_rate / mod_speed + 0.5)`` entries; the result is clamped to ``[-1, 1]``.  Equal to the reference's
    per-sample loop bit for bit in float32 and float64 (float16 / bfloat16 compute in float32 and round once), one launch in
    place of several per sample.  The table is built on the host in float64 and cached per (parameters, device): the first call
    with new parameters cannot run inside a graph capture.  ``L`` up to 512, tables up to 2^24 entries
    (``NotImplementedError`` beyond); ``L < 1`` or an empty table raise ``ValueError``.  Forward-only; a plain Python entry
    point through the C ABI (not registered as a dispatcher op)."""
    _fx_check_type(waveform, "phaser")
    if waveform.dim() < 1:
        raise ValueError("audio_amd: phaser expects (..., time), got a 0-dimensional tensor")
    L = int(delay_ms * 0.001 * sample_rate + 0.5)
    M = int(sample_rate / mod_speed + 0.5)
    if L < 1:
        raise ValueError(f"audio_amd: phaser: delay_ms * sample_rate / 1000 rounds to a delay of {L} samples; at least 1 is needed")
    if M < 1:
        raise ValueError(f"audio_amd: phaser: sample_rate / mod_speed rounds to a modulation table of {M} entries; at least 1 is needed")
    if L > PHASER_MAX_RING:
        raise NotImplementedError(f"audio_amd: phaser serves delays up to {PHASER_MAX_RING} samples (got {L})")
    if M > EFFECTS_MAX_TABLE:
        raise NotImplementedError(f"audio_amd: phaser serves modulation tables up to 2^24 = {EFFECTS_MAX_TABLE} entries (got {M})")
    _fx_check_device(waveform, "phaser")
    out = torch.empty(tuple(waveform.shape), dtype=waveform.dtype, device=waveform.device)
    if out.numel() == 0:
        return out
    table = _fx_table(("phaser", L, M, bool(sinusoidal)), waveform.device,
                      lambda: _host.effects_wave_table("SINE" if sinusoidal else "TRIANGLE", "INT", M, 1.0, float(L), math.pi / 2))
    x2, rows, T_ = _fx_rows(waveform)
    ws = _fx_workspace(_FX_PHASER, x2, L)
    with torch.cuda.device(waveform.device):
        _lib.check(_lib.lib().aamd_phaser(_SA_DTYPES[x2.dtype], x2.data_ptr(), out.data_ptr(), ws.data_ptr(), rows, T_,
                                          _wa_stride(x2), table.data_ptr(), M, L, float(gain_in), float(gain_out), float(decay),
                                          _lib.current_stream(waveform.device)))
    return out


def flanger(waveform: Tensor, sample_rate: int, delay: float = 0.0, depth: float = 2.0, regen: float = 0.0,
            width: float = 71.0, speed: float = 0.5, phase: float = 25.0, modulation: str = "sinusoidal",
            interpolation: str = "linear", *, _general: bool = False) -> Tensor:
    r"""Flanger (reference: F.flanger, SoX's effect) on ``(..., channel, time)`` with at most 4 channels: a delay line of
    ``L = int((delay + depth) / 1000 * sample_rate + 0.5) + 2`` samples read at a delay swept by a table of
    ``int(sample_rate / speed)`` entries (each channel ``phase`` percent of a period further on), linear or quadratic
    interpolation, ``regen`` percent fed back; the result is clamped to ``[-1, 1]``.  Equal to the reference's per-sample loop
    bit for bit in float32 and float64 (float16 / bfloat16 compute in float32 and round once).  ``regen == 0`` has no
    recurrence and runs as a streaming gather: there a non-finite sample reaches only the outputs whose taps read it (the
    reference's ``last * 0`` keeps a NaN alive for the rest of the row) and a stored ``-0.0`` is read as stored.  The table
    is built on the host in float64 and cached per (parameters, device): the first call with new parameters cannot run inside
    a graph capture.  ``L`` up to 4096, tables up to 2^24 entries (``NotImplementedError`` beyond).  Forward-only; a plain
    Python entry point through the C ABI (not registered as a dispatcher op)."""
    if modulation not in ("sinusoidal", "triangular"):
        raise ValueError('Only "sinusoidal" or "triangular" modulation allowed')
    if interpolation not in ("linear", "quadratic"):
        raise ValueError('Only "linear" or "quadratic" interpolation allowed')
    _fx_check_type(waveform, "flanger")
    if waveform.dim() < 2:
        raise ValueError(f"audio_amd: flanger expects (..., channel, time), got {tuple(waveform.shape)}")
    channels = waveform.shape[-2]
    if channels > 4:
        raise ValueError("Max 4 channels allowed")
    feedback_gain = regen / 100
    delay_gain = width / 100
    channel_phase = phase / 100
    in_gain = 1.0 / (1 + delay_gain)
    delay_gain = delay_gain / (1 + delay_gain)
    delay_gain = delay_gain * (1 - abs(feedback_gain))
    delay_min = delay / 1000
    L = int((delay_min + depth / 1000) * sample_rate + 0.5) + 2
    N = int(sample_rate / speed)
    if N < 1:
        raise ValueError(f"audio_amd: flanger: sample_rate / speed gives a modulation table of {N} entries; at least 1 is needed")
    if L < 2:
        raise ValueError(f"audio_amd: flanger: delay and depth give a delay line of {L} samples; they must not be negative")
    if L > FLANGER_MAX_RING:
        raise NotImplementedError(f"audio_amd: flanger serves delay lines up to {FLANGER_MAX_RING} samples (got {L})")
    if N > EFFECTS_MAX_TABLE:
        raise NotImplementedError(f"audio_amd: flanger serves modulation tables up to 2^24 = {EFFECTS_MAX_TABLE} entries (got {N})")
    _fx_check_device(waveform, "flanger")
    out = torch.empty(tuple(waveform.shape), dtype=waveform.dtype, device=waveform.device)
    if out.numel() == 0:
        return out
    table_min = float(math.floor(delay_min * sample_rate + 0.5))
    table = _fx_table(("flanger", N, table_min, L, modulation), waveform.device,
                      lambda: _host.effects_wave_table("SINE" if modulation == "sinusoidal" else "TRIANGLE", "FLOAT", N,
                                                       table_min, float(L) - 2.0, 3 * math.pi / 2))
    cph = (C.c_int64 * 4)(*[int(v) % N for v in _host.flanger_channel_phase(channels, N, channel_phase)])
    x2, rows, T_ = _fx_rows(waveform)
    general = bool(_general) or feedback_gain != 0.0
    ws = _fx_workspace(_FX_FLANGER, x2, L if general else 0)
    with torch.cuda.device(waveform.device):
        _lib.check(_lib.lib().aamd_flanger(_SA_DTYPES[x2.dtype], x2.data_ptr(), out.data_ptr(), ws.data_ptr(), rows, T_,
                                           _wa_stride(x2), channels, table.data_ptr(), N, cph, L, float(feedback_gain),
                                           float(in_gain), float(delay_gain), int(interpolation == "quadratic"), int(general),
                                           _lib.current_stream(waveform.device)))
    return out


# --------------------------------------------------------------------------- #
# InverseMelScale (csrc/inverse_mel.h)                                        #
# --------------------------------------------------------------------------- #
_IMEL_DRIVERS = ("gels", "gelsy", "gelsd", "gelss")
_IMEL_PINNED: dict = {}              # id(P) -> P: pseudo-inverses a captured graph reads, kept for the life of the process


def inverse_mel_tiles() -> Tuple[int, int, int]:
    """(frames of one row per workgroup, bins of n_stft per LDS tile, the most mel bins the kernel serves) of
    csrc/inverse_mel.h (iml::kFrames, iml::kBins, iml::kMaxMels)."""
    lib = _lib.lib()
    return int(lib.aamd_inverse_mel_tiles(0)), int(lib.aamd_inverse_mel_tiles(1)), int(lib.aamd_inverse_mel_tiles(2))


def _inverse_mel_matrix(fb: Tensor, device, dtype: torch.dtype = torch.float32, fragments: bool = False) -> Tensor:
    """The (n_stft, n_mels) pseudo-inverse of `fb` on `device` (`_host.inverse_mel_rank_and_pinv`: float64 SVD, float32
    rank cut), rounded once to `dtype` (float64: not rounded); `fragments`: the float32 one as the flat tile image the kernel
    reads (`_host.inverse_mel_fragments`).  Cached per buffer like every constant derived from one: the
    key holds the buffer's identity, in-place version and storage, so `load_state_dict`, `fb.mul_()` and `.to()` rebuild it.
    Building it copies `fb` to the host, which a graph capture cannot do: the first call must run eagerly."""
    def make():
        if fb.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("audio_amd: the pseudo-inverse of this filterbank is not on the device yet and cannot be built "
                               "inside a graph capture (it needs the filterbank on the host); run the call once eagerly "
                               "before capturing it")
        p = _host.inverse_mel_rank_and_pinv(fb.detach().to(torch.float32).cpu().numpy())[1]
        if dtype != torch.float64:
            p = p.astype(np.float32)
        if fragments:
            p = _host.inverse_mel_fragments(p, inverse_mel_tiles()[1])
        t = torch.from_numpy(np.ascontiguousarray(p)).to(device)
        return t.to(dtype) if dtype in LOW_PRECISION else t
    p = _tensor_cached(fb, ("inverse_mel", str(device), dtype, fragments), make)
    if p.is_cuda and torch.cuda.is_current_stream_capturing():
        with _CACHE_LOCK:
            _IMEL_PINNED[id(p)] = p           # (an id is not reused while its tensor is held here)
    return p


def _imel_rows(x: Tensor) -> Tuple[Tensor, int, int, int]:
    """(..., n_mels, T) as (rows, n_mels, T) that the kernel reads in place -- one row stride, unit stride along mel (the
    frame-major view of a MelSpectrogram) or along time (a contiguous tensor) -- gathered where the strides are anything else.
    Returns the tensor and its (row, mel, frame) strides as the kernel takes them."""
    K, T_ = x.shape[-2], x.shape[-1]
    rows = x.numel() // (K * T_)

    def strides(t):
        sr, sm, st = t.stride()
        return (0 if rows == 1 else sr), (1 if K == 1 else sm), (1 if T_ == 1 else st)

    x3 = x
    if x3.dim() != 3:
        try:
            x3 = x.view(rows, K, T_)
        except RuntimeError:
            x3 = x.contiguous().view(rows, K, T_)
    sr, sm, st = strides(x3)
    if sr < 0 or sm < 1 or st < 1 or (sm != 1 and st != 1):
        x3 = x3.contiguous()
        sr, sm, st = strides(x3)
    return x3, sr, sm, st


def inverse_mel_scale(melspec: Tensor, fb: Tensor, log_input: bool = False) -> Tensor:
    r"""EXTENSION (as ``mel_scale`` is): T.InverseMelScale.forward on a filterbank ``fb`` of shape ``(n_stft, n_mels)``:
    ``(..., n_mels, time) -> (..., n_stft, time)``, ``relu(P @ y)`` per frame with ``P`` the pseudo-inverse of ``fb^T``
    cut at float32's rank (``_host.inverse_mel_rank_and_pinv``; the minimum-norm least-squares solution, what the reference's
    ``lstsq`` drivers return for a full-rank filterbank and ``gelsd`` for a rank-deficient one) and ``y = melspec`` or, with
    ``log_input``, ``exp(melspec)`` evaluated in the load.

    One launch (csrc/inverse_mel.h) on the float32 matrix instructions: FMA chains in ascending mel, one accumulator per
    output, so the bits do not depend on layout, alignment or batch.  float32, float16 and bfloat16 are read in place (unit
    stride along mel or along time; anything else is gathered first), computed in float32 and rounded once.  The result is
    frame-major, returned as the ``(..., n_stft, time)`` view, the layout ``GriffinLim`` and ``InverseSpectrogram`` read.
    ``n_mels`` up to 256 (``NotImplementedError`` beyond).  float64 input, or an input or ``fb`` that requires grad under
    grad mode, takes ``torch.relu(torch.matmul(P, y))`` with ``P`` in the input's dtype (the precision / training path; ``P``
    is a constant of ``fb``: no gradient reaches ``fb``).  The first call for a filterbank builds ``P`` on the host and cannot
    run inside a graph capture; later calls can.  A plain Python entry point through the C ABI (not a dispatcher op)."""
    if not isinstance(melspec, Tensor) or not isinstance(fb, Tensor):
        raise TypeError("audio_amd: inverse_mel_scale: melspec and fb must be tensors")
    if melspec.dtype not in _WA_FLOATS:
        raise TypeError(f"audio_amd: inverse_mel_scale: melspec must be float16, bfloat16, float32 or float64 (got {melspec.dtype})")
    if fb.dim() != 2 or not fb.is_floating_point():
        raise ValueError(f"audio_amd: inverse_mel_scale: fb must be a floating-point (n_stft, n_mels) matrix (got {tuple(fb.shape)})")
    n_stft, n_mels = int(fb.shape[0]), int(fb.shape[1])
    if melspec.dim() < 2 or melspec.shape[-2] != n_mels:
        raise ValueError("Expected an input with {} mel bins. Found: {}".format(
            n_mels, melspec.shape[-2] if melspec.dim() >= 2 else tuple(melspec.shape)))
    _wa_require(melspec, "inverse_mel_scale: melspec")
    if melspec.dtype == torch.float64 or (torch.is_grad_enabled() and (melspec.requires_grad or fb.requires_grad)):
        P = _inverse_mel_matrix(fb, melspec.device, melspec.dtype)
        return torch.relu(torch.matmul(P, melspec.exp() if log_input else melspec))
    limit = inverse_mel_tiles()[2]
    if n_mels > limit:
        raise NotImplementedError(f"audio_amd: inverse_mel_scale serves up to {limit} mel bins (got {n_mels})")
    lead, T_ = tuple(melspec.shape[:-2]), int(melspec.shape[-1])
    out = torch.empty(lead + (T_, n_stft), dtype=melspec.dtype, device=melspec.device)
    if out.numel() == 0 or n_mels == 0:
        return out.zero_().transpose(-1, -2)
    x3, sr, sm, st = _imel_rows(melspec.detach())
    P = _inverse_mel_matrix(fb, melspec.device, fragments=True)
    with torch.cuda.device(melspec.device):
        _lib.check(_lib.lib().aamd_inverse_mel(_SA_DTYPES[x3.dtype], x3.data_ptr(), P.data_ptr(), out.data_ptr(), x3.shape[0],
                                               T_, sr, sm, st, n_stft, n_mels, int(bool(log_input)),
                                               _lib.current_stream(melspec.device)))
    return out.transpose(-1, -2)


# --------------------------------------------------------------------------- #
# Dense filterbank projection (csrc/dense_fbank.h): ChromaScale               #
# --------------------------------------------------------------------------- #
_DFB_PINNED: dict = {}               # id(W) -> W: operand images a captured graph reads, kept for the life of the process


def dense_fbank_tiles() -> Tuple[int, int, int, int]:
    """(frames of one row per workgroup, bins of n_freqs per LDS tile, the most outputs, the most frequency bins the kernel
    serves) of csrc/dense_fbank.h (dfb::kFrames, dfb::kTileK, dfb::kMaxN, dfb::kMaxK)."""
    lib = _lib.lib()
    return tuple(int(lib.aamd_dense_fbank_tiles(i)) for i in range(4))


def _dense_fbank_image(fb: Tensor, device) -> Tensor:
    """The float32 values of `fb` on `device` in the order the kernel's A operand is read (`_host.dense_fbank_fragments`),
    padded with zeros to a multiple of 16 outputs and of 4 bins.  Cached per buffer like every constant derived from one
    (identity, in-place version, storage).  Building it copies `fb` to the host, which a graph capture cannot do: the first
    call must run eagerly."""
    def make():
        if fb.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("audio_amd: the operand image of this filterbank is not on the device yet and cannot be built "
                               "inside a graph capture (it needs the filterbank on the host); run the call once eagerly "
                               "before capturing it")
        w = _host.dense_fbank_fragments(fb.detach().to(torch.float32).cpu().numpy())
        return torch.from_numpy(w).to(device)
    w = _tensor_cached(fb, ("dense_fbank", str(device)), make)
    if w.is_cuda and torch.cuda.is_current_stream_capturing():
        with _CACHE_LOCK:
            _DFB_PINNED[id(w)] = w            # (an id is not reused while its tensor is held here)
    return w


def dense_fbank_scale(specgram: Tensor, fb: Tensor) -> Tensor:
    r"""EXTENSION (as ``mel_scale`` is): the projection of a spectrogram onto a DENSE filterbank ``fb`` of shape
    ``(n_freqs, n_out)`` -- ``ChromaScale.forward``: ``(..., n_freqs, time) -> (..., n_out, time)``,
    ``matmul(specgram^T, fb)^T`` per row.

    One launch (csrc/dense_fbank.h) on the float32 matrix instructions: FMA chains in ascending frequency, one accumulator
    per output, so the bits do not depend on layout, alignment, batch or tiling.  float32, float16 and bfloat16 are read in
    place (unit stride along freq -- the frame-major view every ``Spectrogram`` here returns -- or along time; anything else
    is gathered first), computed in float32 and rounded once.  The result is frame-major, returned as the
    ``(..., n_out, time)`` view, ``MelScale``'s convention.  ``n_out`` up to 128 and ``n_freqs`` up to 4097
    (``NotImplementedError`` beyond).  float64 input, or an input or ``fb`` that requires grad under grad mode, takes
    ``torch.matmul`` (the precision / training path; gradients reach ``fb``).  The first call for a filterbank lays it out on
    the host and cannot run inside a graph capture; later calls can.  A plain Python entry point through the C ABI (not a
    dispatcher op)."""
    if not isinstance(specgram, Tensor) or not isinstance(fb, Tensor):
        raise TypeError("audio_amd: dense_fbank_scale: specgram and fb must be tensors")
    if specgram.dtype not in _WA_FLOATS:
        raise TypeError(f"audio_amd: dense_fbank_scale: specgram must be float16, bfloat16, float32 or float64 (got {specgram.dtype})")
    if fb.dim() != 2 or not fb.is_floating_point():
        raise ValueError(f"audio_amd: dense_fbank_scale: fb must be a floating-point (n_freqs, n_out) matrix (got {tuple(fb.shape)})")
    n_freqs, n_out = int(fb.shape[0]), int(fb.shape[1])
    if specgram.dim() < 2 or specgram.shape[-2] != n_freqs:
        raise ValueError("audio_amd: dense_fbank_scale: expected an input with {} frequency bins, the filterbank's. Found: {}".format(
            n_freqs, specgram.shape[-2] if specgram.dim() >= 2 else tuple(specgram.shape)))
    _wa_require(specgram, "dense_fbank_scale: specgram")
    if specgram.dtype == torch.float64 or (torch.is_grad_enabled() and (specgram.requires_grad or fb.requires_grad)):
        return torch.matmul(specgram.transpose(-1, -2), fb.to(device=specgram.device, dtype=specgram.dtype)).transpose(-1, -2)
    _, _, max_out, max_freqs = dense_fbank_tiles()
    if n_out > max_out:
        raise NotImplementedError(f"audio_amd: dense_fbank_scale serves up to {max_out} outputs (got {n_out})")
    if n_freqs > max_freqs:
        raise NotImplementedError(f"audio_amd: dense_fbank_scale serves up to {max_freqs} frequency bins (got {n_freqs})")
    lead, T_ = tuple(specgram.shape[:-2]), int(specgram.shape[-1])
    out = torch.empty(lead + (T_, n_out), dtype=specgram.dtype, device=specgram.device)
    if out.numel() == 0 or n_freqs == 0:
        return out.zero_().transpose(-1, -2)
    x3, sr, sk, st = _imel_rows(specgram.detach())
    W = _dense_fbank_image(fb, specgram.device)
    with torch.cuda.device(specgram.device):
        _lib.check(_lib.lib().aamd_dense_fbank(_SA_DTYPES[x3.dtype], x3.data_ptr(), W.data_ptr(), out.data_ptr(), x3.shape[0],
                                               T_, sr, sk, st, n_freqs, n_out, _lib.current_stream(specgram.device)))
    return out.transpose(-1, -2)


# --------------------------------------------------------------------------- #
# Voice-activity trimming (csrc/vad.h)                                        #
# --------------------------------------------------------------------------- #
VAD_MAX_FFT = 8192                   # AAMD_VAD_MAX_FFT: the largest measurement transform (the defaults up to 81.9 kHz)
_VAD_TABLES: "collections.OrderedDict" = collections.OrderedDict()   # (win, bins, n_fft, device) -> device tables, LRU
_VAD_PINNED: dict = {}               # tables a captured graph reads: kept for the life of the process
_VAD_TABLES_MAX = 16

_VadPlan = collections.namedtuple("_VadPlan", "L N P M gap fixed s0 s1 c0 c1 boot_max up down smooth trig nra level")


def vad_tiles() -> Tuple[int, int, int, int]:
    """(threads per workgroup of the measurement kernels, the largest and the smallest measurement transform, rows per
    workgroup of the trigger kernel) of csrc/vad.h: vad::kThreads, kMaxN, kMinN, kTrigThreads."""
    lib = _lib.lib()
    return tuple(int(lib.aamd_vad_tiles(i)) for i in range(4))


def _vad_plan(sample_rate, trigger_level, trigger_time, search_time, allowed_gap, pre_trigger_time, boot_time, noise_up_time,
              noise_down_time, noise_reduction_amount, measure_freq, measure_duration, measure_smooth_time, hp_filter_freq,
              lp_filter_freq, hp_lifter_freq, lp_lifter_freq) -> _VadPlan:
    """The reference's derived quantities, in Python arithmetic on the host; the parameter errors."""
    named = dict(sample_rate=sample_rate, trigger_level=trigger_level, trigger_time=trigger_time, search_time=search_time,
                 allowed_gap=allowed_gap, pre_trigger_time=pre_trigger_time, boot_time=boot_time, noise_up_time=noise_up_time,
                 noise_down_time=noise_down_time, noise_reduction_amount=noise_reduction_amount, measure_freq=measure_freq,
                 measure_smooth_time=measure_smooth_time, hp_filter_freq=hp_filter_freq, lp_filter_freq=lp_filter_freq,
                 hp_lifter_freq=hp_lifter_freq, lp_lifter_freq=lp_lifter_freq)
    if measure_duration is not None:
        named["measure_duration"] = measure_duration
    for k, v in named.items():
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
            raise ValueError(f"audio_amd: vad: {k} must be a finite number (got {v!r})")
    for k in ("sample_rate", "measure_freq", "trigger_time", "search_time", "noise_up_time", "noise_down_time",
              "measure_smooth_time", "hp_lifter_freq", "lp_lifter_freq", "measure_duration"):
        if k in named and not named[k] > 0:
            raise ValueError(f"audio_amd: vad: {k} must be positive (got {named[k]!r})")
    for k in ("allowed_gap", "pre_trigger_time", "boot_time", "hp_filter_freq", "lp_filter_freq"):
        if named[k] < 0:
            raise ValueError(f"audio_amd: vad: {k} must not be negative (got {named[k]!r})")
    sr, mf = sample_rate, measure_freq
    md = 2.0 / mf if measure_duration is None else measure_duration
    L = int(sr * md + 0.5)
    if L < 1:
        raise ValueError(f"audio_amd: vad: sample_rate * measure_duration rounds to a measurement of {L} samples; at least 1 is "
                         "needed")
    N = 16
    while N < L:
        N *= 2
    P = int(sr / mf + 0.5)
    if P < 1:
        raise ValueError(f"audio_amd: vad: sample_rate / measure_freq rounds to a measurement period of {P} samples; at least 1 "
                         "is needed")
    s0 = max(int(hp_filter_freq / sr * N + 0.5), 1)
    s1 = min(int(lp_filter_freq / sr * N + 0.5), N // 2)
    if s1 <= s0:
        raise ValueError(f"audio_amd: vad: hp_filter_freq and lp_filter_freq leave no spectrum bin: start {s0}, end {s1}")
    c0 = math.ceil(sr * 0.5 / lp_lifter_freq)
    c1 = min(math.floor(sr * 0.5 / hp_lifter_freq), N // 4)
    if c1 <= c0:
        raise ValueError("Expected cepstrum_start to be smaller than cepstrum_end."
                         f"Found: cepstrum_start: {c0}, cepstrum_end: {c1}.")
    if N > VAD_MAX_FFT:
        raise NotImplementedError(f"audio_amd: vad serves measurement transforms up to {VAD_MAX_FFT} points (the defaults up to "
                                  f"81.9 kHz); {L} samples per measurement need {N}")
    mult = lambda t: math.exp(-1.0 / (t * mf))      # noqa: E731
    return _VadPlan(L=L, N=N, P=P, M=math.ceil(search_time * mf), gap=int(allowed_gap * mf + 0.5),
                    fixed=int(pre_trigger_time * sr + 0.5), s0=s0, s1=s1, c0=c0, c1=c1, boot_max=int(boot_time * mf - 0.5),
                    up=mult(noise_up_time), down=mult(noise_down_time), smooth=mult(measure_smooth_time), trig=mult(trigger_time),
                    nra=float(noise_reduction_amount), level=float(trigger_level))


def _vad_tables(plan: _VadPlan, device) -> Tensor:
    """The two windows and the twiddles of `plan` on `device`: built on the host (float64, rounded once) and uploaded once.
    Never allocated from a capture's pool: the first call with this plan must run eagerly."""
    k = (plan.L, plan.s1 - plan.s0, plan.N, str(device))
    capturing = torch.cuda.is_current_stream_capturing()
    with _CACHE_LOCK:
        t = _VAD_PINNED.get(k)
        if t is None:
            t = _VAD_TABLES.get(k)
            if t is not None:
                _VAD_TABLES.move_to_end(k)
                if capturing:
                    _VAD_PINNED[k] = t
    if t is not None:
        return t
    if capturing:
        raise RuntimeError("audio_amd: the window tables of these vad parameters are not on the device yet and cannot be built "
                           "inside a graph capture; run the call once eagerly before capturing it")
    t = torch.from_numpy(_host.vad_tables(k[0], k[1], k[2])).to(device)
    with _CACHE_LOCK:
        t = _VAD_TABLES.setdefault(k, t)
        _VAD_TABLES.move_to_end(k)
        while len(_VAD_TABLES) > _VAD_TABLES_MAX:
            _VAD_TABLES.popitem(last=False)
    return t


def _vad_frames(T_: int, plan: _VadPlan) -> int:
    return 0 if T_ <= plan.L else (T_ - plan.L - 1) // plan.P + 1


def _vad_measure_rows(x2: Tensor, plan: _VadPlan) -> Tensor:
    """(rows, frames) float32 measurements of the rows of x2, every row a recording of its own: three launches."""
    rows, T_ = x2.shape
    frames = _vad_frames(T_, plan)
    meas = torch.empty((rows, frames), dtype=torch.float32, device=x2.device)
    if meas.numel() == 0:
        return meas
    tables = _vad_tables(plan, x2.device)
    lib = _lib.lib()
    ws = torch.empty((int(lib.aamd_vad_workspace(rows, frames, plan.s1 - plan.s0)) // 4,), dtype=torch.float32, device=x2.device)
    with torch.cuda.device(x2.device):
        _lib.check(lib.aamd_vad_measure(_SA_DTYPES[x2.dtype], x2.data_ptr(), rows, T_, _wa_stride(x2), plan.L, plan.N, plan.P,
                                        plan.s0, plan.s1, plan.c0, plan.c1, plan.boot_max, plan.smooth, plan.up, plan.down,
                                        plan.nra, tables.data_ptr(), ws.data_ptr(), meas.data_ptr(), frames,
                                        _lib.current_stream(x2.device)))
    return meas


def _vad_trigger(meas: Tensor, ring: int, gap: int, period: int, fixed: int, trigger_level: float, trigger_mult: float,
                 joint: bool = True) -> Tuple[Tensor, Tensor, Optional[Tensor]]:
    """The trigger pass over dense float32 (rows, frames) measurements on the device (private: F.vad and F.vad_start call it,
    the tests drive it with synthetic measurements): int64 (first frame per row or -1, start per row or -1, the joint start
    as a 1-element tensor where `joint`).  One launch, two with the joint start; no synchronisation."""
    if meas.dim() != 2 or meas.dtype != torch.float32 or not meas.is_contiguous():
        raise ValueError("audio_amd: vad: the measurements must be a contiguous float32 (rows, frames) tensor")
    _wa_require(meas, "vad: measurements")
    rows, frames = meas.shape
    first = torch.empty((rows,), dtype=torch.int64, device=meas.device)
    start = torch.empty((rows,), dtype=torch.int64, device=meas.device)
    jt = torch.empty((1,), dtype=torch.int64, device=meas.device) if joint else None
    with torch.cuda.device(meas.device):
        _lib.check(_lib.lib().aamd_vad_trigger(_lib.ptr(meas), rows, frames, int(ring), int(gap), int(period), int(fixed),
                                               float(trigger_level), float(trigger_mult), _lib.ptr(first), _lib.ptr(start),
                                               jt.data_ptr() if joint else 0, _lib.current_stream(meas.device)))
    return first, start, jt


def _vad_prepare(waveform: Tensor, what: str, plan_args) -> Tuple[Tensor, _VadPlan]:
    _fx_check_type(waveform, what)
    if waveform.dim() < 1:
        raise ValueError(f"audio_amd: {what} expects (..., time), got a 0-dimensional tensor")
    plan = _vad_plan(*plan_args)
    _fx_check_device(waveform, what)
    return _fx_rows(waveform)[0], plan


def vad_start(waveform: Tensor, sample_rate: int, trigger_level: float = 7.0, trigger_time: float = 0.25,
              search_time: float = 1.0, allowed_gap: float = 0.25, pre_trigger_time: float = 0.0, boot_time: float = 0.35,
              noise_up_time: float = 0.1, noise_down_time: float = 0.01, noise_reduction_amount: float = 1.35,
              measure_freq: float = 20.0, measure_duration: Optional[float] = None, measure_smooth_time: float = 0.4,
              hp_filter_freq: float = 50.0, lp_filter_freq: float = 6000.0, hp_lifter_freq: float = 150.0,
              lp_lifter_freq: float = 2000.0) -> Tensor:
    r"""Where :func:`vad` would start each row of ``(..., time)`` if the row were a single-channel recording of its own (an
    extension; the reference has no batched form): int64 of shape ``waveform.shape[:-1]`` on the device, the first sample to
    keep, or ``-1`` where the row never triggers -- what a batched pipeline builds lengths and masks from.  Parameters as
    :func:`vad`.  Four launches and no synchronisation; can be captured in a graph once the window tables of the parameters
    are cached, i.e. after one eager call (the first call inside a capture raises).  Rows are read in place through their row
    stride; a non-unit sample stride is gathered first.  Deterministic; forward-only; a plain Python entry point through the C
    ABI (not registered as a dispatcher op)."""
    x2, plan = _vad_prepare(waveform, "vad_start", (sample_rate, trigger_level, trigger_time, search_time, allowed_gap,
                                                   pre_trigger_time, boot_time, noise_up_time, noise_down_time,
                                                   noise_reduction_amount, measure_freq, measure_duration, measure_smooth_time,
                                                   hp_filter_freq, lp_filter_freq, hp_lifter_freq, lp_lifter_freq))
    meas = _vad_measure_rows(x2, plan)
    _, start, _ = _vad_trigger(meas, plan.M, plan.gap, plan.P, plan.fixed, plan.level, plan.trig, joint=False)
    return start.view(tuple(waveform.shape[:-1]))


def _vad_measures(waveform: Tensor, sample_rate: int, trigger_level: float = 7.0, trigger_time: float = 0.25,
                  search_time: float = 1.0, allowed_gap: float = 0.25, pre_trigger_time: float = 0.0, boot_time: float = 0.35,
                  noise_up_time: float = 0.1, noise_down_time: float = 0.01, noise_reduction_amount: float = 1.35,
                  measure_freq: float = 20.0, measure_duration: Optional[float] = None, measure_smooth_time: float = 0.4,
                  hp_filter_freq: float = 50.0, lp_filter_freq: float = 6000.0, hp_lifter_freq: float = 150.0,
                  lp_lifter_freq: float = 2000.0) -> Tensor:
    """Diagnostic (private, like ``_compute_nccf``): the ``(rows, frames)`` float32 measurements that the trigger pass of
    :func:`vad` / :func:`vad_start` reads, bit for bit; rows = all leading dimensions flattened."""
    x2, plan = _vad_prepare(waveform, "vad", (sample_rate, trigger_level, trigger_time, search_time, allowed_gap,
                                             pre_trigger_time, boot_time, noise_up_time, noise_down_time, noise_reduction_amount,
                                             measure_freq, measure_duration, measure_smooth_time, hp_filter_freq, lp_filter_freq,
                                             hp_lifter_freq, lp_lifter_freq))
    return _vad_measure_rows(x2, plan)


def vad(waveform: Tensor, sample_rate: int, trigger_level: float = 7.0, trigger_time: float = 0.25, search_time: float = 1.0,
        allowed_gap: float = 0.25, pre_trigger_time: float = 0.0, boot_time: float = 0.35, noise_up_time: float = 0.1,
        noise_down_time: float = 0.01, noise_reduction_amount: float = 1.35, measure_freq: float = 20.0,
        measure_duration: Optional[float] = None, measure_smooth_time: float = 0.4, hp_filter_freq: float = 50.0,
        lp_filter_freq: float = 6000.0, hp_lifter_freq: float = 150.0, lp_lifter_freq: float = 2000.0) -> Tensor:
    r"""Voice-activity detector (reference: F.vad, SoX's effect): trims the silence in front of the first speech of
    ``(..., time)``.  As in the reference all leading dimensions are channels of ONE recording: every ``1 / measure_freq``
    seconds each channel's last ``measure_duration`` seconds are measured (noise-reduced spectrum, cepstral power on a log
    scale); the first channel whose smoothed measurement reaches ``trigger_level`` trims all channels at one common sample,
    found by scanning back over ``search_time``; the result is the view ``waveform[..., start:]``, or ``waveform[..., :0]``
    where nothing triggers.  More than 2 dimensions warn, as the reference does: a batch is not trimmed row by row
    (use :func:`vad_start` for that).

    The reference runs some two dozen small tensor operations and a host read-back per measurement and channel; here all
    measurements of all channels take three launches and the trigger two.  The slice bound is a Python int, so the call makes
    exactly one 8-byte device-to-host copy and therefore cannot be captured in a graph (:func:`vad_start` can).  Arithmetic is
    float32 for every dtype, the trigger float64 and integers.  Differences from the reference: the start is clamped at 0 (the
    reference's negative bound, where ``pre_trigger_time`` reaches before the first sample, wraps to the end of the signal);
    the Hann windows are built on the host in float64 and rounded once, cached per (plan, device); every frame of every
    channel is measured; a channel with a NaN sample measures 0 from there on and does not trigger; a signal of at most
    ``measure_duration`` seconds has no measurement and never triggers.  ``ValueError`` for an empty cepstrum or spectrum
    range and non-positive rates and times, ``TypeError`` for integer dtypes, ``NotImplementedError`` above 8192 samples per
    measurement (the defaults up to 81.9 kHz).  Forward-only; a plain Python entry point through the C ABI (not registered as
    a dispatcher op)."""
    if isinstance(waveform, Tensor) and waveform.dim() > 2:
        warnings.warn("Expected input tensor dimension of 1 for single channel or 2 for multi-channel. Got "
                      f"{waveform.dim()} instead. All leading dimensions are treated as channels of one recording and are "
                      "trimmed at one common sample; use audio_amd.functional.vad_start (F.vad_start) for a start per row of a "
                      "batch.", UserWarning, stacklevel=2)
    x2, plan = _vad_prepare(waveform, "vad", (sample_rate, trigger_level, trigger_time, search_time, allowed_gap, pre_trigger_time,
                                             boot_time, noise_up_time, noise_down_time, noise_reduction_amount, measure_freq,
                                             measure_duration, measure_smooth_time, hp_filter_freq, lp_filter_freq,
                                             hp_lifter_freq, lp_lifter_freq))
    meas = _vad_measure_rows(x2, plan)
    _, _, joint = _vad_trigger(meas, plan.M, plan.gap, plan.P, plan.fixed, plan.level, plan.trig, joint=True)
    start = int(joint.item())                      # the one device-to-host copy: 8 bytes
    return waveform[..., :0] if start < 0 else waveform[..., start:]


# --------------------------------------------------------------------------- #
# spectral centroid (csrc/spectral_feat.h)                                    #
# --------------------------------------------------------------------------- #


def spectral_tiles() -> Tuple[int, int, int]:
    """(threads per workgroup, float32 values per 16-byte vector, the most lanes that share a frame line) of the centroid
    kernel (csrc/spectral_feat.h: sf::kThreads, sf::kVec, sf::kMaxLanes)."""
    lib = _lib.lib()
    return int(lib.aamd_spectral_tiles(0)), int(lib.aamd_spectral_tiles(1)), int(lib.aamd_spectral_tiles(2))


def _device_table(what: str, key, device, make) -> Tensor:
    """A small host-built constant of `key` on `device` (``make()`` returns a CPU tensor), uploaded once and shared with the
    effects' tables (`_FX_TABLES`).  Never allocated from a capture's pool: the first call with these parameters must run
    eagerly."""
    k = key + (str(device),)
    capturing = torch.cuda.is_current_stream_capturing()
    with _CACHE_LOCK:
        t = _FX_PINNED.get(k)
        if t is None:
            t = _FX_TABLES.get(k)
            if t is not None:
                _FX_TABLES.move_to_end(k)
                if capturing:
                    _FX_PINNED[k] = t
    if t is not None:
        return t
    if capturing:
        raise RuntimeError(f"audio_amd: the {what} of these parameters is not on the device yet and cannot be built inside a "
                           "graph capture; run the call once eagerly before capturing it")
    t = make().to(device)
    with _CACHE_LOCK:
        t = _FX_TABLES.setdefault(k, t)
        _FX_TABLES.move_to_end(k)
        while len(_FX_TABLES) > _FX_TABLES_MAX:
            _FX_TABLES.popitem(last=False)
    return t


def _centroid_freqs(sample_rate: int, n_fft: int, device) -> Tensor:
    return _device_table("frequency table", ("centroid_freqs", int(sample_rate), int(n_fft)), device,
                         lambda: torch.from_numpy(_host.centroid_freqs(sample_rate, n_fft)))


def _centroid_reduce(specgram: Tensor, freqs: Tensor, out_dtype: torch.dtype = torch.float32) -> Tensor:
    """The reduction kernel alone: float32 magnitudes ``(..., freq, time)`` in either layout (read in place through their
    strides) and the float32 frequency table ``[freq]`` on the device -> ``(..., time)`` of `out_dtype`."""
    if specgram.dtype != torch.float32 or freqs.dtype != torch.float32:
        raise TypeError("audio_amd: spectral_centroid: the reduction reads float32 magnitudes and frequencies")
    if out_dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise TypeError(f"audio_amd: spectral_centroid: the reduction writes float32, float16 or bfloat16 (got {out_dtype})")
    _wa_require(specgram, "spectral_centroid: specgram")
    if specgram.dim() < 2 or freqs.dim() != 1 or freqs.shape[0] != specgram.shape[-2] or freqs.device != specgram.device:
        raise ValueError("audio_amd: spectral_centroid: expected (..., freq, time) magnitudes and [freq] frequencies on one device")
    lead, n_freq, frames = tuple(specgram.shape[:-2]), specgram.shape[-2], specgram.shape[-1]
    out = torch.empty(lead + (frames,), dtype=out_dtype, device=specgram.device)
    if out.numel() == 0:
        return out
    if n_freq == 0:
        raise ValueError("audio_amd: spectral_centroid: no frequency bins")
    rows = out.numel() // frames
    m3 = specgram.detach().transpose(-1, -2).reshape(rows, frames, n_freq)      # a view wherever the leading strides collapse
    if freqs.data_ptr() % 16 or not freqs.is_contiguous():
        freqs = freqs.clone(memory_format=torch.contiguous_format)
    with torch.cuda.device(specgram.device):
        _lib.check(_lib.lib().aamd_spectral_centroid(_SA_DTYPES[out_dtype], m3.data_ptr(), freqs.data_ptr(), out.data_ptr(), rows,
                                                     frames, n_freq, m3.stride(0) if rows > 1 else 0, m3.stride(1), m3.stride(2),
                                                     _lib.current_stream(specgram.device)))
    return out


def spectral_centroid(waveform: Tensor, sample_rate: int, pad: int, window: Tensor, n_fft: int, hop_length: int,
                      win_length: int) -> Tensor:
    r"""Spectral centroid of ``(..., time)`` audio -> ``(..., time)`` frames (reference: F.spectral_centroid): the mean of the
    frequencies ``linspace(0, sample_rate // 2, 1 + n_fft // 2)`` weighted by the magnitude spectrogram.  Two launches: the
    magnitude spectrogram of whichever STFT family serves `n_fft`, then one reduction over its frame-major memory with
    float64 sums in a fixed order (two calls give the same bits).  A frame of silence gives NaN (0 / 0), as in the reference.
    float16 / bfloat16 compute in float32 and return their dtype; float64, or an input that requires grad, takes the
    differentiable composition.  The frequency table is cached per (sample_rate, n_fft, device): run the call once eagerly
    before capturing it in a graph.  A plain Python entry point through the C ABI (not registered as a dispatcher op)."""
    if not isinstance(waveform, Tensor) or not isinstance(window, Tensor):
        raise TypeError("audio_amd: spectral_centroid: waveform and window must be tensors")
    _wa_require(waveform, "spectral_centroid: waveform")
    if waveform.dtype == torch.float64 or _learnable(waveform, window):
        spec = spectrogram(waveform, pad, window, n_fft, hop_length, win_length, 1.0, False)
        return _diff.spectral_centroid(spec, torch.from_numpy(_host.centroid_freqs(sample_rate, n_fft)))
    freqs = _centroid_freqs(sample_rate, n_fft, waveform.device)        # first: inside a capture a missing table raises here
    spec = _spectrogram_eager(waveform.float() if waveform.dtype in LOW_PRECISION else waveform, pad, window, n_fft, hop_length,
                              win_length, 1.0, False)                  # (..., freq, time) over frame-major memory
    return _centroid_reduce(spec, freqs, waveform.dtype)


# --------------------------------------------------------------------------- #
# pointwise waveform ops (csrc/wave_pointwise.h)                              #
# --------------------------------------------------------------------------- #
_PW_SCALE, _PW_CONTRAST, _PW_DB_TO_AMPLITUDE, _PW_MU_ENCODE, _PW_MU_DECODE, _PW_FADE = range(6)      # AAMD_PW_*
_PW_INTS = {torch.int64: 4, torch.int32: 5, torch.int16: 6, torch.int8: 7, torch.uint8: 8}          # AAMD_PW_I64 ..


def pointwise_tiles() -> Tuple[int, int, int]:
    """(threads per workgroup, samples per workgroup, 16-byte groups a thread keeps in flight) of the pointwise kernel
    (csrc/wave_pointwise.h: pw::kThreads, pw::kChunk, pw::kBatch)."""
    lib = _lib.lib()
    return int(lib.aamd_pointwise_tiles(0)), int(lib.aamd_pointwise_tiles(1)), int(lib.aamd_pointwise_tiles(2))


def _pw_check(x: Tensor, what: str, ints: bool = False) -> None:
    """The type (TypeError); the parameter checks of an op follow, then the device (RuntimeError)."""
    if not isinstance(x, Tensor):
        raise TypeError(f"audio_amd: {what}: the input must be a tensor")
    if x.dtype not in _WA_FLOATS and not (ints and x.dtype in _PW_INTS):
        raise TypeError(f"audio_amd: {what}: the input must be float16, bfloat16, float32 or float64"
                        f"{' or an integer tensor' if ints else ''} (got {x.dtype})")


def _pw_grad(x: Tensor) -> bool:
    return x.requires_grad and torch.is_grad_enabled()


def _pw_launch(op: int, x: Tensor, out_dtype: torch.dtype, p0: float = 0.0, p1: float = 0.0, flag: int = 0,
               table: Optional[Tensor] = None, n_in: int = 0, n_out: int = 0) -> Tensor:
    """One launch of the pointwise kernel over `x` read in place (rows of a wider tensor through one row stride; a non-unit
    sample stride is gathered first) into a new contiguous tensor."""
    out = torch.empty(tuple(x.shape), dtype=out_dtype, device=x.device)
    if out.numel() == 0:
        return out
    x1 = x.detach().reshape(1) if x.dim() == 0 else x.detach()
    x2 = _wa_rows(x1, tuple(x1.shape[:-1]), x1.shape[-1])
    code = _SA_DTYPES[x.dtype] if x.dtype in _SA_DTYPES else _PW_INTS[x.dtype]
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().aamd_pointwise(op, code, x2.data_ptr(), out.data_ptr(), x2.shape[0], x2.shape[1], _wa_stride(x2),
                                             float(p0), float(p1), int(flag), 0 if table is None else table.data_ptr(),
                                             int(n_in), int(n_out), _lib.current_stream(x.device)))
    return out


def _scale(waveform: Tensor, ratio: float, clamp: bool, what: str) -> Tensor:
    """``waveform * ratio`` (ratio rounded once to the compute type), clamped to [-1, 1] where asked: one launch."""
    _wa_require(waveform, f"{what}: waveform")
    if _pw_grad(waveform):
        return _diff.scale(waveform, ratio, clamp)
    return _pw_launch(_PW_SCALE, waveform, waveform.dtype, ratio, 0.0, int(clamp))


def gain(waveform: Tensor, gain_db: float = 1.0) -> Tensor:
    r"""Apply amplification or attenuation to the whole waveform (reference: F.gain): ``waveform * 10 ** (gain_db / 20)``,
    the ratio a Python double rounded once to the compute type, so float32 and float64 results are bit-exact against numpy.
    ``gain_db == 0`` returns the input object.  One launch; float16 / bfloat16 compute in float32; an input that requires
    grad takes the torch expression.  A plain Python entry point through the C ABI."""
    if gain_db == 0:
        return waveform
    _pw_check(waveform, "gain")
    return _scale(waveform, 10 ** (gain_db / 20), False, "gain")


def _vol(waveform: Tensor, gain: float, gain_type: str) -> Tensor:
    """T.Vol.forward: the gain of its type and the clamp to [-1, 1] in one launch."""
    _pw_check(waveform, "Vol")
    if gain_type == "amplitude":
        ratio = float(gain)
    elif gain_type == "db":
        ratio = 10 ** (gain / 20)
    elif gain_type == "power":
        ratio = 10 ** ((10 * math.log10(gain)) / 20)
    else:
        raise ValueError(f"gain_type must be one of amplitude, power or db (got {gain_type!r})")
    return _scale(waveform, ratio, True, "Vol")


def contrast(waveform: Tensor, enhancement_amount: float = 75.0) -> Tensor:
    r"""Contrast enhancement (reference: F.contrast, SoX's effect): ``t = waveform * (pi / 2)``,
    ``sin(t + enhancement_amount / 750 * sin(t * 4))``, with the accurate ``sin``.  One launch; float16 / bfloat16 compute in
    float32; an input that requires grad takes the torch expression.  A plain Python entry point through the C ABI."""
    _pw_check(waveform, "contrast")
    if not 0 <= enhancement_amount <= 100:
        raise ValueError("Allowed range of values for enhancement_amount : 0-100")
    _wa_require(waveform, "contrast: waveform")
    if _pw_grad(waveform):
        return _diff.contrast(waveform, float(enhancement_amount))
    return _pw_launch(_PW_CONTRAST, waveform, waveform.dtype, math.pi / 2, enhancement_amount / 750.0)


def DB_to_amplitude(x: Tensor, ref: float, power: float) -> Tensor:
    r"""Decibels back to power or amplitude (reference: F.DB_to_amplitude): ``ref * pow(pow(10, 0.1 * x), power)`` with the
    accurate ``pow``.  One launch; float16 / bfloat16 compute in float32; an input that requires grad takes the torch
    expression.  A plain Python entry point through the C ABI."""
    _pw_check(x, "DB_to_amplitude")
    _wa_require(x, "DB_to_amplitude: x")
    if _pw_grad(x):
        return _diff.db_to_amplitude(x, float(ref), float(power))
    return _pw_launch(_PW_DB_TO_AMPLITUDE, x, x.dtype, float(ref), float(power))


def _mu_channels(quantization_channels: int) -> float:
    if not isinstance(quantization_channels, int) or isinstance(quantization_channels, bool) or quantization_channels < 2:
        raise ValueError(f"quantization_channels must be an integer of at least 2 (got {quantization_channels!r})")
    return quantization_channels - 1.0


def mu_law_encoding(x: Tensor, quantization_channels: int) -> Tensor:
    r"""Mu-law companding (reference: F.mu_law_encoding): a signal in [-1, 1] -> int64 codes in [0, quantization_channels - 1],
    ``int64((sign(x) log1p(mu |x|) / log1p(mu) + 1) / 2 * mu + 0.5)`` with ``mu = quantization_channels - 1``.  An integer
    input is converted to float32 with the reference's warning.  One launch; float16 / bfloat16 compute in float32; no
    gradient (the result is integer).  A plain Python entry point through the C ABI."""
    _pw_check(x, "mu_law_encoding", ints=True)
    mu = _mu_channels(quantization_channels)
    _wa_require(x, "mu_law_encoding: x", floating=False)
    if not x.is_floating_point():
        warnings.warn("The input Tensor must be of floating type. This will be an error in the v0.12 release.")
        x = x.to(torch.float)
    return _pw_launch(_PW_MU_ENCODE, x, torch.int64, mu)


def mu_law_decoding(x_mu: Tensor, quantization_channels: int) -> Tensor:
    r"""Mu-law expansion (reference: F.mu_law_decoding): codes in [0, quantization_channels - 1] -> a signal in [-1, 1],
    ``y = x_mu / mu * 2 - 1``, ``sign(y) (exp(|y| log1p(mu)) - 1) / mu``.  Integer codes of any integer dtype are read as
    they are and give float32; a floating input keeps its dtype.  One launch; an input that requires grad takes the torch
    expression.  A plain Python entry point through the C ABI."""
    _pw_check(x_mu, "mu_law_decoding", ints=True)
    mu = _mu_channels(quantization_channels)
    _wa_require(x_mu, "mu_law_decoding: x_mu", floating=False)
    if _pw_grad(x_mu):
        return _diff.mu_law_decoding(x_mu, quantization_channels)
    return _pw_launch(_PW_MU_DECODE, x_mu, x_mu.dtype if x_mu.is_floating_point() else torch.float32, mu)


def _fade(waveform: Tensor, fade_in_len: int, fade_out_len: int, fade_shape: str) -> Tensor:
    """T.Fade.forward: ``(fade_in * fade_out) * waveform`` along the last axis.  The two ramps are built on the host in float64,
    rounded once to the waveform's dtype and cached per (parameters, dtype, device); the kernel multiplies inside the ramps
    and copies bits elsewhere."""
    _pw_check(waveform, "Fade")
    if fade_shape not in _host.FADE_SHAPES:
        raise ValueError(f"fade_shape must be one of {', '.join(_host.FADE_SHAPES)} (got {fade_shape!r})")
    n_in, n_out = int(fade_in_len), int(fade_out_len)
    if n_in < 0 or n_out < 0:
        raise ValueError("fade_in_len and fade_out_len must not be negative")
    if waveform.dim() < 1:
        raise ValueError("audio_amd: Fade expects (..., time), got a 0-dimensional tensor")
    length = waveform.shape[-1]
    if n_in > length or n_out > length:
        raise ValueError(f"a fade ({n_in} in, {n_out} out) is longer than the signal ({length} samples)")
    _wa_require(waveform, "Fade: waveform")
    if n_in + n_out == 0:
        table = None
    else:
        table = _device_table("fade table", ("fade", n_in, n_out, fade_shape, str(waveform.dtype)), waveform.device,
                              lambda: _host.round_once(np.concatenate(_host.fade_ramps(n_in, n_out, fade_shape)), waveform.dtype))
    if _pw_grad(waveform):
        ramps = waveform.new_zeros(0) if table is None else table
        return _diff.fade(waveform, ramps[:n_in], ramps[n_in:])
    return _pw_launch(_PW_FADE, waveform, waveform.dtype, table=table, n_in=n_in, n_out=n_out)


# --------------------------------------------------------------------------- #
# image-source room impulse responses (csrc/rir.h)                            #
# --------------------------------------------------------------------------- #
RIR_MAX_FILTER = 1025                # AAMD_RIR_MAX_FILTER: the longest delay filter (taps) the kernel serves
RIR_MAX_ORDER = 64                   # AAMD_RIR_MAX_ORDER: the largest reflection order (357 889 images in 3-D)
_RIR_TABLES: "collections.OrderedDict" = collections.OrderedDict()   # (max_order, D, device) -> int16 lattice, LRU
_RIR_PINNED: dict = {}               # tables a captured graph reads: kept for the life of the process
_RIR_TABLES_MAX = 16


def rir_tiles() -> Tuple[int, int, int, int]:
    """(samples per workgroup, images per chunk, the largest delay_filter_length, the largest max_order) of csrc/rir.h:
    rir::kTile, kChunk, kMaxFl, kMaxOrder."""
    lib = _lib.lib()
    return tuple(int(lib.aamd_rir_tiles(i)) for i in range(4))


def _rir_lattice(max_order: int, D: int, device) -> Tensor:
    """The image lattice of (max_order, D) on `device`: built on the host and uploaded once.  Never allocated from a capture's
    pool: the first call with this (max_order, D) must run eagerly."""
    k = (max_order, D, str(device))
    capturing = torch.cuda.is_current_stream_capturing()
    with _CACHE_LOCK:
        t = _RIR_PINNED.get(k)
        if t is None:
            t = _RIR_TABLES.get(k)
            if t is not None:
                _RIR_TABLES.move_to_end(k)
                if capturing:
                    _RIR_PINNED[k] = t
    if t is not None:
        return t
    if capturing:
        raise RuntimeError("audio_amd: the image lattice of this max_order is not on the device yet and cannot be built inside "
                           "a graph capture; run the call once eagerly before capturing it")
    t = torch.from_numpy(_host.rir_lattice(max_order, D)).to(device)
    with _CACHE_LOCK:
        t = _RIR_TABLES.setdefault(k, t)
        _RIR_TABLES.move_to_end(k)
        while len(_RIR_TABLES) > _RIR_TABLES_MAX:
            _RIR_TABLES.popitem(last=False)
    return t


def _rir_check(what: str, room, source, mic_array, batched: bool, max_order, delay_filter_length, output_length,
               sample_rate, sound_speed) -> int:
    """The checks that need no device, in the order ranks, sizes, dtypes, parameters, limits; returns D."""
    lead = 1 if batched else 0
    for name, t, rank in (("room", room, lead + 1), ("source", source, lead + 1), ("mic_array", mic_array, lead + 2)):
        if not isinstance(t, Tensor):
            raise TypeError(f"audio_amd: {what}: {name} must be a tensor")
        if t.dim() != rank:
            raise ValueError(f"audio_amd: {what}: {name} must have {rank} dimensions (got {t.dim()})")
    D = room.shape[-1]
    if D not in (2, 3):
        raise ValueError(f"audio_amd: {what}: room must have 2 or 3 coordinates (got {D})")
    if source.shape[-1] != D or mic_array.shape[-1] != D:
        raise ValueError(f"audio_amd: {what}: room, source and mic_array must have the same number of coordinates (got {D}, "
                         f"{source.shape[-1]}, {mic_array.shape[-1]})")
    if batched and not (room.shape[0] == source.shape[0] == mic_array.shape[0]):
        raise ValueError(f"audio_amd: {what}: room, source and mic_array must have the same number of rooms (got "
                         f"{room.shape[0]}, {source.shape[0]}, {mic_array.shape[0]})")
    if room.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"audio_amd: {what}: room must be float32 or float64 (got {room.dtype})")
    if source.dtype != room.dtype or mic_array.dtype != room.dtype:
        raise TypeError(f"audio_amd: {what}: room, source and mic_array must have one dtype (got {room.dtype}, {source.dtype}, "
                        f"{mic_array.dtype})")
    for name, v in (("max_order", max_order), ("delay_filter_length", delay_filter_length)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise TypeError(f"audio_amd: {what}: {name} must be an int (got {v!r})")
    if max_order < 0:
        raise ValueError(f"audio_amd: {what}: max_order must not be negative (got {max_order})")
    if delay_filter_length < 3 or delay_filter_length % 2 == 0:
        raise ValueError(f"audio_amd: {what}: delay_filter_length must be odd and at least 3 (got {delay_filter_length})")
    if output_length is not None:
        if isinstance(output_length, bool) or not isinstance(output_length, int):
            raise TypeError(f"audio_amd: {what}: output_length must be an int (got {output_length!r})")
        if output_length < 1:
            raise ValueError(f"audio_amd: {what}: output_length must be at least 1 (got {output_length})")
    for name, v in (("sample_rate", sample_rate), ("sound_speed", sound_speed)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or not v > 0:
            raise ValueError(f"audio_amd: {what}: {name} must be a positive finite number (got {v!r})")
    if delay_filter_length > RIR_MAX_FILTER:
        raise NotImplementedError(f"audio_amd: {what} serves delay filters up to {RIR_MAX_FILTER} taps (got {delay_filter_length})")
    if max_order > RIR_MAX_ORDER:
        raise NotImplementedError(f"audio_amd: {what} serves max_order up to {RIR_MAX_ORDER} (got {max_order})")
    return D


def _rir_absorption(what: str, absorption, B: int, D: int, like: Tensor, batched: bool) -> Tensor:
    """Dense (B, 2 D) of `like`'s dtype on its device, from a float, (B,) / (B, 2 D) (batched) or (2 D,) / (1, 2 D)."""
    if isinstance(absorption, Tensor):
        a = absorption
        if a.dtype != like.dtype:
            raise TypeError(f"audio_amd: {what}: absorption must have the dtype of room ({like.dtype}; got {a.dtype})")
        if not batched:
            if a.dim() == 2 and a.shape[0] > 1:
                raise NotImplementedError(f"audio_amd: {what}: a multi-band absorption of shape {tuple(a.shape)} needs the "
                                          "reference's octave-band filter bank, which is not implemented; pass one band")
            if a.dim() not in (1, 2) or a.shape[-1] != 2 * D:
                raise ValueError(f"audio_amd: {what}: absorption must be a float, ({2 * D},) or (1, {2 * D}) (got {tuple(a.shape)})")
            a = a.reshape(1, 2 * D)
        elif a.dim() == 1 and a.shape[0] == B:
            a = a.unsqueeze(1).expand(B, 2 * D)
        elif a.dim() != 2 or tuple(a.shape) != (B, 2 * D):
            raise ValueError(f"audio_amd: {what}: absorption must be a float, ({B},) or ({B}, {2 * D}) (got {tuple(a.shape)})")
        if a.requires_grad and torch.is_grad_enabled():
            raise RuntimeError(f"audio_amd: {what} is forward-only (no gradient is implemented); wrap the call in "
                               "torch.no_grad() or detach the inputs.")
        _wa_require(a, f"{what}: absorption")
        return a.detach().contiguous()
    if isinstance(absorption, bool) or not isinstance(absorption, (int, float)):
        raise TypeError(f"audio_amd: {what}: absorption must be a float or a tensor (got {type(absorption).__name__})")
    return torch.full((B, 2 * D), float(absorption), dtype=like.dtype, device=like.device)


def _rir_launch(what: str, room: Tensor, source: Tensor, mic_array: Tensor, max_order: int, absorption, output_length: int,
                sound_speed: float, delay_filter_length: int, sample_rate: float, batched: bool) -> Tensor:
    D = room.shape[-1]
    if torch.is_grad_enabled() and (room.requires_grad or source.requires_grad or mic_array.requires_grad):
        raise RuntimeError(f"audio_amd: {what} is forward-only (no gradient is implemented); wrap the call in "
                           "torch.no_grad() or detach the inputs.")
    for name, t in (("room", room), ("source", source), ("mic_array", mic_array)):
        _wa_require(t, f"{what}: {name}")
    if not batched:
        room, source, mic_array = room.unsqueeze(0), source.unsqueeze(0), mic_array.unsqueeze(0)
    B, M = mic_array.shape[0], mic_array.shape[1]
    ab = _rir_absorption(what, absorption, B, D, room, batched)
    room, source, mic_array = room.detach().contiguous(), source.detach().contiguous(), mic_array.detach().contiguous()
    out = torch.empty((B, M, output_length), dtype=room.dtype, device=room.device)
    if out.numel():
        table = _rir_lattice(max_order, D, room.device)
        with torch.cuda.device(room.device):
            _lib.check(_lib.lib().aamd_simulate_rir(_SA_DTYPES[room.dtype], room.data_ptr(), source.data_ptr(), mic_array.data_ptr(),
                                                    ab.data_ptr(), table.data_ptr(), table.shape[0], out.data_ptr(), B, M, D,
                                                    max_order, delay_filter_length, output_length, float(sample_rate),
                                                    float(sound_speed), _lib.current_stream(room.device)))
    return out if batched else out[0]


def simulate_rir_ism_batch(room: Tensor, source: Tensor, mic_array: Tensor, max_order: int,
                           absorption: Union[float, Tensor], output_length: int, sound_speed: float = 343.0,
                           delay_filter_length: int = 81, sample_rate: float = 16000.0) -> Tensor:
    r"""Room impulse responses of a batch of shoebox rooms by the image-source method (an extension; the reference simulates
    one room per call, on the CPU): ``room (B, D)``, ``source (B, D)``, ``mic_array (B, M, D)`` with ``D`` 2 or 3 give
    ``(B, M, output_length)``; every row is a room of its own.  ``absorption`` is a float, ``(B,)`` (one coefficient per
    room) or ``(B, 2 D)`` (per wall: west, east, south, north, floor, ceiling).  The definition is :func:`simulate_rir_ism`'s.
    One launch and no synchronisation: can be captured in a graph once the image lattice of ``(max_order, D)`` is cached,
    i.e. after one eager call (the first call inside a capture raises).  float32 or float64; geometry and sums are float64
    for both and a float32 result is rounded once; a row whose images include a non-finite delay or amplitude (a microphone
    on an image, an absorption above 1) is NaN throughout.  Deterministic: a sample's bits do not depend on ``B``, ``M`` or
    ``output_length``.  Forward-only; a plain Python entry point through the C ABI (not registered as a dispatcher op)."""
    what = "simulate_rir_ism_batch"
    if output_length is None:
        raise ValueError(f"audio_amd: {what}: output_length is required (the default length needs the positions on the host)")
    _rir_check(what, room, source, mic_array, True, max_order, delay_filter_length, output_length, sample_rate, sound_speed)
    return _rir_launch(what, room, source, mic_array, max_order, absorption, output_length, sound_speed, delay_filter_length,
                       sample_rate, True)


def simulate_rir_ism(room: Tensor, source: Tensor, mic_array: Tensor, max_order: int, absorption: Union[float, Tensor],
                     sound_speed: float = 343.0, delay_filter_length: int = 81, center_frequency: Optional[Tensor] = None,
                     sample_rate: float = 16000.0, output_length: Optional[int] = None) -> Tensor:
    r"""Room impulse response of a shoebox room by the image-source method (reference:
    ``torchaudio.prototype.functional.simulate_rir_ism``, single band): ``room (D,)``, ``source (D,)``, ``mic_array (M, D)``
    give ``(M, L)``.

    Images are the integer vectors ``v`` with ``sum |v_d| <= max_order`` (last axis fastest); per axis ``loc = room (v + 1) -
    source`` for odd ``v`` and ``room v + source`` for even ``v``, ``att = prod_d tr_lower^|floor(v / 2)| tr_upper^|floor((v +
    1) / 2)|`` with ``tr = sqrt(1 - absorption)``; per microphone ``a = att / dist`` and ``tau = dist sample_rate /
    sound_speed``.  With ``pad = delay_filter_length // 2`` and ``g(x) = sinc(x) (1 + cos(pi x / pad)) / 2`` on ``|x| <=
    pad``, ``rir[c, n] = sum_i a g(n - pad - tau)``: the reference's scatter from ``ceil(tau)`` on, written as a gather.
    ``L`` is ``output_length`` or ``ceil(max tau) + delay_filter_length``; the latter copies the three position tensors to
    the host once to size the result (`_host.rir_length`).  ``absorption`` is a float, ``(2 D,)`` or ``(1, 2 D)``; more than
    one band raises NotImplementedError (the octave-band filter bank is out of scope) and ``center_frequency`` is accepted
    and unused.  Precision, NaN rows, determinism and the limits (:func:`rir_tiles`) as :func:`simulate_rir_ism_batch`."""
    what = "simulate_rir_ism"
    _rir_check(what, room, source, mic_array, False, max_order, delay_filter_length, output_length, sample_rate, sound_speed)
    if isinstance(absorption, Tensor) and absorption.dim() == 2 and absorption.shape[0] > 1:
        raise NotImplementedError(f"audio_amd: {what}: a multi-band absorption of shape {tuple(absorption.shape)} needs the "
                                  "reference's octave-band filter bank, which is not implemented; pass one band")
    if output_length is None:
        for name, t in (("room", room), ("source", source), ("mic_array", mic_array)):
            _wa_require(t, f"{what}: {name}")
        if mic_array.shape[0] == 0:
            raise ValueError(f"audio_amd: {what}: the default length needs at least one microphone; pass output_length")
        output_length = _host.rir_length(room.detach().cpu().numpy(), source.detach().cpu().numpy(),
                                         mic_array.detach().cpu().numpy(), max_order, sample_rate, sound_speed, delay_filter_length)
    return _rir_launch(what, room, source, mic_array, max_order, absorption, output_length, sound_speed, delay_filter_length,
                       sample_rate, False)


# --------------------------------------------------------------------------- #
# ray-traced energy histograms of shoebox rooms (csrc/ray_trace.h)            #
# --------------------------------------------------------------------------- #
RAY_MAX_BANDS = 8                    # AAMD_RAY_MAX_BANDS
RAY_MAX_MICS = 16                    # AAMD_RAY_MAX_MICS
RAY_MAX_RAYS = 1 << 24               # AAMD_RAY_MAX_RAYS
RAY_MAX_BINS = 65536                 # AAMD_RAY_MAX_BINS
RAY_MAX_BOUNCES = 4096               # AAMD_RAY_MAX_BOUNCES: a room whose sum_d (floor(S_max / room_d) + 2) exceeds it is NaN
RAY_HEADROOM = 64                    # AAMD_RAY_HEADROOM: contributions of every ray a (microphone, bin) may take


def ray_tiles() -> Tuple[int, int, int, int, int, int, int]:
    """(rays per workgroup, the most bands, the most microphones, the most rays, the most bins, the cap on a room's bounce
    bound, the headroom of the fixed-point sums) of csrc/ray_trace.h: ray::kThreads, kMaxBands, kMaxMics, kMaxRays, kMaxBins,
    kMaxBounces, kHeadroom."""
    lib = _lib.lib()
    return tuple(int(lib.aamd_ray_tiles(i)) for i in range(7))


def _ray_check(what: str, room, source, mic_array, batched: bool, num_rays, absorption, scattering, mic_radius, sound_speed,
               energy_thres, time_thres, hist_bin_size) -> Tuple[int, int]:
    """The checks that need no device, in the order ranks, sizes, dtypes, parameters, limits; returns (num_bands, num_bins)."""
    lead = 1 if batched else 0
    for name, t, rank in (("room", room, lead + 1), ("source", source, lead + 1), ("mic_array", mic_array, lead + 2)):
        if not isinstance(t, Tensor):
            raise TypeError(f"audio_amd: {what}: {name} must be a tensor")
        if t.dim() != rank:
            raise ValueError(f"audio_amd: {what}: {name} must have {rank} dimensions (got {t.dim()})")
    D = room.shape[-1]
    if D not in (2, 3):
        raise ValueError(f"audio_amd: {what}: room must have 2 or 3 coordinates (got {D})")
    if source.shape[-1] != D or mic_array.shape[-1] != D:
        raise ValueError(f"audio_amd: {what}: room, source and mic_array must have the same number of coordinates (got {D}, "
                         f"{source.shape[-1]}, {mic_array.shape[-1]})")
    if batched and not (room.shape[0] == source.shape[0] == mic_array.shape[0]):
        raise ValueError(f"audio_amd: {what}: room, source and mic_array must have the same number of rooms (got "
                         f"{room.shape[0]}, {source.shape[0]}, {mic_array.shape[0]})")
    B = room.shape[0] if batched else 1
    bands = []
    for name, c in (("absorption", absorption), ("scattering", scattering)):
        if isinstance(c, Tensor):
            if batched:
                if c.dim() != 3 or c.shape[0] != B or c.shape[2] != 2 * D:
                    raise ValueError(f"audio_amd: {what}: {name} must be a float or ({B}, num_bands, {2 * D}) (got {tuple(c.shape)})")
            elif c.dim() not in (1, 2) or (c.dim() == 2 and c.shape[1] != 2 * D):
                raise ValueError(f"audio_amd: {what}: {name} must be a float, (num_bands,) or (num_bands, {2 * D}) (got "
                                 f"{tuple(c.shape)})")
            bands.append(c.shape[1] if batched else c.shape[0])
            if bands[-1] < 1:
                raise ValueError(f"audio_amd: {what}: {name} must have at least one band (got {tuple(c.shape)})")
        elif isinstance(c, bool) or not isinstance(c, (int, float)):
            raise TypeError(f"audio_amd: {what}: {name} must be a float or a tensor (got {type(c).__name__})")
        else:
            bands.append(1)
    num_bands = max(bands)
    if min(bands) not in (1, num_bands):
        raise ValueError(f"audio_amd: {what}: absorption and scattering must have the same number of bands, or one of them a "
                         f"single band (got {bands[0]} and {bands[1]})")
    if room.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"audio_amd: {what}: room must be float32 or float64 (got {room.dtype})")
    others = [t for t in (source, mic_array, absorption, scattering) if isinstance(t, Tensor)]
    if any(t.dtype != room.dtype for t in others):
        raise TypeError(f"audio_amd: {what}: room, source, mic_array and the coefficient tensors must have one dtype (got "
                        f"{', '.join(str(t.dtype) for t in [room] + others)})")
    if isinstance(num_rays, bool) or not isinstance(num_rays, int):
        raise TypeError(f"audio_amd: {what}: num_rays must be an int (got {num_rays!r})")
    if num_rays < 1:
        raise ValueError(f"audio_amd: {what}: num_rays must be at least 1 (got {num_rays})")
    for name, v in (("mic_radius", mic_radius), ("sound_speed", sound_speed), ("energy_thres", energy_thres),
                    ("time_thres", time_thres), ("hist_bin_size", hist_bin_size)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or not v > 0:
            raise ValueError(f"audio_amd: {what}: {name} must be a positive finite number (got {v!r})")
    num_bins = _host.ray_num_bins(time_thres, hist_bin_size)
    if num_bands > RAY_MAX_BANDS:
        raise NotImplementedError(f"audio_amd: {what} serves up to {RAY_MAX_BANDS} bands (got {num_bands})")
    if mic_array.shape[-2] > RAY_MAX_MICS:
        raise NotImplementedError(f"audio_amd: {what} serves up to {RAY_MAX_MICS} microphones (got {mic_array.shape[-2]})")
    if num_rays > RAY_MAX_RAYS:
        raise NotImplementedError(f"audio_amd: {what} serves up to {RAY_MAX_RAYS} rays (got {num_rays})")
    if num_bins > RAY_MAX_BINS:
        raise NotImplementedError(f"audio_amd: {what} serves up to {RAY_MAX_BINS} bins (got {num_bins} = ceil(time_thres / "
                                  "hist_bin_size))")
    return num_bands, num_bins


def _ray_coefficients(what: str, name: str, c, B: int, D: int, num_bands: int, like: Tensor, batched: bool) -> Tensor:
    """Dense (B, num_bands, 2 D) of `like`'s dtype on its device, from a float or a tensor of one of the checked forms."""
    if not isinstance(c, Tensor):
        return torch.full((B, num_bands, 2 * D), float(c), dtype=like.dtype, device=like.device)
    if c.requires_grad and torch.is_grad_enabled():
        raise RuntimeError(f"audio_amd: {what} is forward-only (no gradient is implemented); wrap the call in "
                           "torch.no_grad() or detach the inputs.")
    _wa_require(c, f"{what}: {name}")
    c = c.detach()
    if not batched:
        c = (c[:, None] if c.dim() == 1 else c)[None]
    return c.expand(B, num_bands, 2 * D).contiguous()


def _ray_launch(what: str, room: Tensor, source: Tensor, mic_array: Tensor, num_rays: int, absorption, scattering,
                mic_radius: float, sound_speed: float, energy_thres: float, time_thres: float, hist_bin_size: float,
                batched: bool) -> Tensor:
    num_bands, num_bins = _ray_check(what, room, source, mic_array, batched, num_rays, absorption, scattering, mic_radius,
                                     sound_speed, energy_thres, time_thres, hist_bin_size)
    D = room.shape[-1]
    if torch.is_grad_enabled() and (room.requires_grad or source.requires_grad or mic_array.requires_grad):
        raise RuntimeError(f"audio_amd: {what} is forward-only (no gradient is implemented); wrap the call in "
                           "torch.no_grad() or detach the inputs.")
    for name, t in (("room", room), ("source", source), ("mic_array", mic_array)):
        _wa_require(t, f"{what}: {name}")
    if not batched:
        room, source, mic_array = room.unsqueeze(0), source.unsqueeze(0), mic_array.unsqueeze(0)
    B, M = mic_array.shape[0], mic_array.shape[1]
    ab = _ray_coefficients(what, "absorption", absorption, B, D, num_bands, room, batched)
    sc = _ray_coefficients(what, "scattering", scattering, B, D, num_bands, room, batched)
    room, source, mic_array = room.detach().contiguous(), source.detach().contiguous(), mic_array.detach().contiguous()
    out = torch.empty((B, M, num_bands, num_bins), dtype=room.dtype, device=room.device)
    if out.numel():
        acc = torch.zeros((B, M, num_bands, num_bins), dtype=torch.int64, device=room.device)
        with torch.cuda.device(room.device):
            _lib.check(_lib.lib().aamd_ray_trace(_SA_DTYPES[room.dtype], room.data_ptr(), source.data_ptr(), mic_array.data_ptr(),
                                                 ab.data_ptr(), sc.data_ptr(), acc.data_ptr(), out.data_ptr(), B, M, D, num_bands,
                                                 num_rays, num_bins, _host.ray_scale_log2(mic_radius), float(mic_radius),
                                                 float(sound_speed), float(energy_thres), float(time_thres),
                                                 float(hist_bin_size), _lib.current_stream(room.device)))
    return out if batched else out[0]


def ray_tracing_batch(room: Tensor, source: Tensor, mic_array: Tensor, num_rays: int, absorption: Union[float, Tensor] = 0.0,
                      scattering: Union[float, Tensor] = 0.0, mic_radius: float = 0.5, sound_speed: float = 343.0,
                      energy_thres: float = 1e-7, time_thres: float = 10.0, hist_bin_size: float = 0.004) -> Tensor:
    r"""Energy histograms of a batch of shoebox rooms by ray tracing (an extension; the reference traces one room per call, on
    the CPU): ``room (B, D)``, ``source (B, D)``, ``mic_array (B, M, D)`` with ``D`` 2 or 3 give ``(B, M, num_bands,
    num_bins)``; every row is a room of its own.  ``absorption`` and ``scattering`` are each a float or ``(B, num_bands, 2
    D)`` (per wall: west, east, south, north, floor, ceiling); one of them may have a single band.  The definition is
    :func:`ray_tracing`'s.  Two launches and no synchronisation; nothing is cached on the host, so the first call can be
    captured in a graph.  float32 or float64; geometry and energies are float64 for both and the result is rounded once.  A
    bad room (see :func:`ray_tracing`) is NaN throughout and the other rooms keep their bits.  Deterministic: the sums are
    fixed point, so a bin's bits do not depend on ``B``, ``M`` or the order in which the rays arrive.  Forward-only; a plain
    Python entry point through the C ABI (not registered as a dispatcher op)."""
    return _ray_launch("ray_tracing_batch", room, source, mic_array, num_rays, absorption, scattering, mic_radius, sound_speed,
                       energy_thres, time_thres, hist_bin_size, True)


def ray_tracing(room: Tensor, source: Tensor, mic_array: Tensor, num_rays: int, absorption: Union[float, Tensor] = 0.0,
                scattering: Union[float, Tensor] = 0.0, mic_radius: float = 0.5, sound_speed: float = 343.0,
                energy_thres: float = 1e-7, time_thres: float = 10.0, hist_bin_size: float = 0.004) -> Tensor:
    r"""Energy histogram of a shoebox room by ray tracing (reference: ``torchaudio.prototype.functional.ray_tracing``): ``room
    (D,)``, ``source (D,)``, ``mic_array (M, D)`` give ``(M, num_bands, num_bins)`` with ``num_bins = ceil(time_thres /
    hist_bin_size)``.  ``absorption`` and ``scattering`` are each a float (one band, all walls), ``(num_bands,)`` (every wall
    alike) or ``(num_bands, 2 D)`` (west, east, south, north, floor, ceiling: wall ``2 d + (upper wall of axis d)``).

    With ``E0 = 2 / num_rays``, ``S_max = time_thres sound_speed``, ``R = mic_radius`` and ``w_bin = sound_speed
    hist_bin_size``, ray ``i`` of ``N`` leaves the source along ``(rho cos phi, rho sin phi, z)`` with ``z = 1 - (2 i + 1) /
    N``, ``rho = sqrt(1 - z^2)``, ``phi = i pi (3 - sqrt 5)`` (in 2-D ``(cos phi, sin phi)`` with ``phi = 2 pi (i + 1/2) /
    N``), carrying ``tr = E0`` in every band, and repeats: (1) the next wall is the first axis that attains ``t = min_d t_d``
    with ``t_d = (room_d - p_d) / dir_d`` for ``dir_d > 0`` and ``p_d / -dir_d`` for ``dir_d < 0``; (2) every microphone with
    ``v = mic - p``, ``u = v . dir``, ``0 <= u <= t`` and ``v . v - u^2 < R^2`` gets ``tr / (r2 p_hit)`` at distance ``d =
    travel + u``, where ``r2 = max(d^2, R^2)`` and ``p_hit = 1 - sqrt(1 - R^2 / r2)``, in bin ``floor(d / w_bin)`` if that is
    a bin; (3) the ray moves to the wall (the hit coordinate is set to 0 or ``room_d`` exactly) and ``tr *= 1 -
    absorption``; (4) if the wall scatters in any band, every microphone at ``v = mic - p``, ``h = |v|`` gets ``st / (r2
    p_hit)`` with ``st = 2 (|v_axis| / h) p_eq tr scattering``, ``p_eq = 1 - sqrt(1 - R^2 / max(h^2, R^2))`` and ``d = travel +
    h``, if ``d < S_max`` and ``max_band st > energy_thres``; (5) ``tr *= 1 - scattering`` and the ray ends if ``travel >
    S_max`` or ``max_band tr < energy_thres``; (6) it reflects.  Every contribution ``e`` enters its sum as ``rint(e 2^k)``
    in int64 with ``k = 62 - ceil(log2(8 H / R^2))``, ``H`` the headroom of :func:`ray_tiles` (64: a step of ``2^-51`` at the
    default radius), and the result is the sum times ``2^-k`` rounded once.  A bin that took more than ``H`` contributions of
    every ray can wrap, and then it is NaN.

    This definition governs where the reference differs: ``r2`` is clamped at ``R^2`` in the product too (the reference
    divides by the unclamped square, which is unbounded for a microphone at the source); geometry and energies are float64
    for float32 inputs; a bad room -- a dimension that is not finite and positive, a source or a microphone not strictly
    inside, a coefficient outside ``[0, 1]`` or NaN, or a bounce bound ``sum_d (floor(S_max / room_d) + 2)`` above the cap of
    :func:`ray_tiles` (4096; the defaults in a 6 x 5 x 3 m room need 2406) -- gives NaN throughout and is not traced.
    Limits, errors, precision and determinism as :func:`ray_tracing_batch`."""
    return _ray_launch("ray_tracing", room, source, mic_array, num_rays, absorption, scattering, mic_radius, sound_speed,
                       energy_thres, time_thres, hist_bin_size, False)


# --------------------------------------------------------------------------- #
# synthesis ops of prototype.functional (csrc/dsp_synth.h)                    #
# --------------------------------------------------------------------------- #
DSP_MAX_TAPS = 2049                  # AAMD_DSP_MAX_TAPS: the longest filter of filter_waveform
DSP_MAX_OSCILLATORS = 256            # AAMD_DSP_MAX_OSCILLATORS: the most oscillators of oscillator_bank
DSP_MAX_MAGNITUDES = 4097            # AAMD_DSP_MAX_MAGNITUDES: the most magnitudes of frequency_impulse_response
_DSP_REDUCTIONS = {"sum": 0, "mean": 1, "none": 2}       # AAMD_DSP_SUM ..
_DSP_WIDE = (torch.float32, torch.float64)


def dsp_tiles() -> Tuple[int, int, int, int, int]:
    """(time steps per chunk of the oscillator scan, outputs per workgroup of filter_waveform, the most taps, the most
    oscillators, the most magnitudes) of csrc/dsp_synth.h: dsp::kOscChunk, kFwTile, kMaxTaps, kMaxOsc, kMaxMags."""
    lib = _lib.lib()
    return tuple(int(lib.aamd_dsp_tiles(i)) for i in range(5))


def _dsp_tensor(what: str, name: str, t, dtypes=None) -> None:
    if not isinstance(t, Tensor):
        raise TypeError(f"audio_amd: {what}: {name} must be a tensor")
    if t.dtype not in (dtypes or _WA_FLOATS):
        names = "float32 or float64" if dtypes else "float16, bfloat16, float32 or float64"
        raise TypeError(f"audio_amd: {what}: {name} must be {names} (got {t.dtype})")


def _dsp_grad(*ts) -> bool:
    return torch.is_grad_enabled() and any(isinstance(t, Tensor) and t.requires_grad for t in ts)


def _dsp_rows3(t: Tensor) -> Tensor:
    """(..., T, N) as (rows, T, N) whose rows are dense -- strides (any, N, 1) -- without a copy wherever the strides allow it."""
    T_, N = t.shape[-2:]
    rows = 1
    for d in t.shape[:-2]:
        rows *= d
    t = t.detach()
    if not ((N <= 1 or t.stride(-1) == 1) and (T_ <= 1 or t.stride(-2) == N)):
        t = t.contiguous()
    if t.dim() != 3:
        try:
            t = t.view(rows, T_, N)
        except RuntimeError:
            t = t.contiguous().view(rows, T_, N)
    if rows > 1 and t.stride(0) < 0:
        t = t.contiguous()
    return t


def oscillator_bank(frequencies: Tensor, amplitudes: Tensor, sample_rate: float, reduction: str = "sum",
                    dtype: Optional[torch.dtype] = torch.float64) -> Tensor:
    r"""A bank of sine oscillators (reference: ``torchaudio.prototype.functional.oscillator_bank``): ``frequencies`` and
    ``amplitudes`` are ``(..., time, N)`` of one shape and dtype; the result is ``(..., time)``, or ``(..., time, N)`` with
    ``reduction="none"``.

    In the input's type (float32 for the half types) ``w = remainder((f * 2 pi) / sample_rate, 2 pi)``; the phase is the
    inclusive prefix sum of ``w`` over time; ``y = a' sin(phase)`` with ``a' = 0`` where ``|f| >= sample_rate / 2``;
    ``"sum"`` and ``"mean"`` reduce the last axis by one fused multiply-add chain in ascending ``n``.  Differences from the
    reference: the prefix sum is always float64 (``dtype`` takes None, float32 or float64 and changes nothing); the phase is
    reduced to ``[-pi, pi]`` in float64 before it is rounded, so a float32 result does not lose accuracy with the length;
    frequencies above Nyquist are silenced without a warning or a synchronisation, so the call can be captured in a graph.
    Two launches (a chunked scan: :func:`dsp_tiles`), no atomics: a sample's bits depend on neither the batch nor the
    length.  A NaN or infinite frequency makes its oscillator NaN from that step on.  At most ``DSP_MAX_OSCILLATORS``
    oscillators.  With an input that requires grad the forward is the same two launches (the same bits) and the
    first-order backward is HIP as well (``csrc/dsp_synth_grad.h``: the forward's phase, ``g sin(phi)`` for the amplitudes
    and a float64 suffix sum of ``g a' cos(phi)`` in a fixed order for the frequencies; two or three launches, only the
    gradients that are needed); under ``create_graph=True`` the backward takes the differentiable composition
    (``_diff.oscillator_bank``), which differentiates to any order.  A plain Python entry point through the C ABI (not
    registered as a dispatcher op)."""
    what = "oscillator_bank"
    _dsp_tensor(what, "frequencies", frequencies)
    _dsp_tensor(what, "amplitudes", amplitudes)
    if frequencies.dim() < 2:
        raise ValueError(f"audio_amd: {what}: frequencies must be (..., time, N) (got {frequencies.dim()} dimension(s))")
    if frequencies.shape != amplitudes.shape:
        raise ValueError(f"audio_amd: {what}: frequencies and amplitudes must have one shape (got {tuple(frequencies.shape)} and "
                         f"{tuple(amplitudes.shape)})")
    if frequencies.dtype != amplitudes.dtype:
        raise TypeError(f"audio_amd: {what}: frequencies and amplitudes must have one dtype (got {frequencies.dtype} and "
                        f"{amplitudes.dtype})")
    if reduction not in _DSP_REDUCTIONS:
        raise ValueError(f"audio_amd: {what}: reduction must be 'sum', 'mean' or 'none' (got {reduction!r})")
    if dtype not in (None, torch.float32, torch.float64):
        raise ValueError(f"audio_amd: {what}: dtype must be None, torch.float32 or torch.float64 (got {dtype!r})")
    try:                                                  # Python and numpy numbers and 0-d tensors, as the reference takes them
        rate = float("nan") if isinstance(sample_rate, bool) else float(sample_rate)
    except (TypeError, ValueError, RuntimeError):
        rate = float("nan")
    if not math.isfinite(rate) or not rate > 0:
        raise ValueError(f"audio_amd: {what}: sample_rate must be a positive finite number (got {sample_rate!r})")
    sample_rate = rate
    T_, N = frequencies.shape[-2:]
    if N > DSP_MAX_OSCILLATORS:
        raise NotImplementedError(f"audio_amd: {what} serves up to {DSP_MAX_OSCILLATORS} oscillators (got {N})")
    _wa_require(frequencies, f"{what}: frequencies")
    _wa_require(amplitudes, f"{what}: amplitudes")
    if amplitudes.device != frequencies.device:
        raise ValueError(f"audio_amd: {what}: frequencies and amplitudes must be on one device")
    if _dsp_grad(frequencies, amplitudes):
        if frequencies.numel() == 0:                      # nothing to launch: the composition carries the (empty) graph
            return _diff.oscillator_bank(frequencies, amplitudes, float(sample_rate), reduction)
        return _OscillatorBankFunction.apply(frequencies, amplitudes, float(sample_rate), reduction)
    return _oscillator_bank_launch(frequencies, amplitudes, float(sample_rate), reduction)


def _oscillator_bank_launch(frequencies: Tensor, amplitudes: Tensor, sample_rate: float, reduction: str) -> Tensor:
    T_, N = frequencies.shape[-2:]
    lead = tuple(frequencies.shape[:-2])
    out = torch.empty(lead + ((T_, N) if reduction == "none" else (T_,)), dtype=frequencies.dtype, device=frequencies.device)
    if out.numel() == 0:
        return out
    if N == 0:
        return out.fill_(float("nan") if reduction == "mean" else 0.0)
    f3, a3 = _dsp_rows3(frequencies), _dsp_rows3(amplitudes)
    rows = f3.shape[0]
    lib = _lib.lib()
    ws = torch.empty((max(int(lib.aamd_oscillator_workspace(rows, T_, N)) // 8, 1),), dtype=torch.float64, device=out.device)
    with torch.cuda.device(out.device):
        _lib.check(lib.aamd_oscillator_bank(_SA_DTYPES[out.dtype], f3.data_ptr(), a3.data_ptr(), out.data_ptr(), ws.data_ptr(), rows,
                                            T_, N, f3.stride(0) if rows > 1 else 0, a3.stride(0) if rows > 1 else 0,
                                            float(sample_rate), _DSP_REDUCTIONS[reduction], _lib.current_stream(out.device)))
    return out


def filter_waveform(waveform: Tensor, kernels: Tensor) -> Tensor:
    r"""A time-varying FIR filter (reference: ``torchaudio.prototype.functional.filter_waveform``): ``waveform`` is ``(...,
    time)``, ``kernels`` is ``(num_filters, L)``, shared by every row, or ``(batch, num_filters, L)`` with ``batch`` the
    number of rows of ``waveform``; ``time`` must be a multiple of ``num_filters``.

    With ``C = time / num_filters`` and ``d = (L - 1) // 2``: ``y[n] = sum_j x[m] h[m // C][j]``, ``m = n + d - j`` inside
    the row -- every input sample is filtered by the filter of its own chunk and the filter delay is compensated, which is
    the reference's unfold, per-chunk convolution, overlap-add and crop as one gather.  One launch, one accumulator per
    output in ascending ``m`` (float32 fused multiply-adds; double for float64; the half types widen on load and round
    once): bits depend on neither the batch nor the tile.  ``L`` up to ``DSP_MAX_TAPS``.  Rows are read in place through
    one row stride.  With an input that requires grad the forward is the same launch (the same bits) and the first-order
    backward is HIP as well (``csrc/dsp_synth_grad.h``: the gradient of ``waveform`` in one launch shaped like the forward,
    the gradient of ``kernels`` as a float64 reduction in a fixed order without atomics; only the gradients that are
    needed, and no ``(rows, time, L)`` temporary); under ``create_graph=True`` the backward takes the differentiable
    composition (``_diff.filter_waveform``), which differentiates to any order.  A plain Python entry point through the C
    ABI (not registered as a dispatcher op)."""
    what = "filter_waveform"
    _dsp_tensor(what, "waveform", waveform)
    _dsp_tensor(what, "kernels", kernels)
    if waveform.dim() < 1:
        raise ValueError(f"audio_amd: {what}: waveform must be (..., time)")
    if kernels.dim() not in (2, 3):
        raise ValueError(f"audio_amd: {what}: kernels must be (num_filters, L) or (batch, num_filters, L) (got {kernels.dim()} "
                         "dimension(s))")
    T_ = waveform.shape[-1]
    F_, L = kernels.shape[-2:]
    if F_ < 1 or L < 1:
        raise ValueError(f"audio_amd: {what}: kernels must hold at least one filter of at least one tap (got {tuple(kernels.shape)})")
    if T_ % F_ != 0:
        raise ValueError(f"audio_amd: {what}: the length ({T_}) must be a multiple of the number of filters ({F_})")
    lead = tuple(waveform.shape[:-1])
    rows = 1
    for d in lead:
        rows *= d
    if kernels.dim() == 3 and kernels.shape[0] != rows:
        raise ValueError(f"audio_amd: {what}: batched kernels must have one set of filters per row of waveform (got "
                         f"{kernels.shape[0]} for {rows} row(s))")
    if waveform.dtype != kernels.dtype:
        raise TypeError(f"audio_amd: {what}: waveform and kernels must have one dtype (got {waveform.dtype} and {kernels.dtype})")
    if L > DSP_MAX_TAPS:
        raise NotImplementedError(f"audio_amd: {what} serves filters up to {DSP_MAX_TAPS} taps (got {L})")
    _wa_require(waveform, f"{what}: waveform")
    _wa_require(kernels, f"{what}: kernels")
    if kernels.device != waveform.device:
        raise ValueError(f"audio_amd: {what}: waveform and kernels must be on one device")
    if _dsp_grad(waveform, kernels):
        if waveform.numel() == 0:                         # nothing to launch: the composition carries the (empty) graph
            return _diff.filter_waveform(waveform.reshape(rows, T_), kernels).reshape(lead + (T_,))
        return _FilterWaveformFunction.apply(waveform, kernels)
    return _filter_waveform_launch(waveform, kernels)


def _filter_waveform_launch(waveform: Tensor, kernels: Tensor) -> Tensor:
    T_ = waveform.shape[-1]
    F_, L = kernels.shape[-2:]
    lead = tuple(waveform.shape[:-1])
    rows = 1
    for d in lead:
        rows *= d
    out = torch.empty(lead + (T_,), dtype=waveform.dtype, device=waveform.device)
    if out.numel() == 0:
        return out
    x2 = _wa_rows(waveform.detach(), lead, T_)
    h = kernels.detach().contiguous()
    with torch.cuda.device(out.device):
        _lib.check(_lib.lib().aamd_filter_waveform(_SA_DTYPES[out.dtype], x2.data_ptr(), h.data_ptr(), out.data_ptr(), rows, T_,
                                                   _wa_stride(x2), F_, L, 1 if kernels.dim() == 3 else 0,
                                                   _lib.current_stream(out.device)))
    return out


class _OscillatorBankFunction(torch.autograd.Function):
    """oscillator_bank in training mode: forward = the two launches of the inference path (the same bits); backward =
    aamd_oscillator_bank_grad (csrc/dsp_synth_grad.h): the forward's phase, grad_amplitudes = g sin(phi) and grad_frequencies =
    the float64 suffix sum of g a' cos(phi), only for the inputs that need one.  All HIP kernels."""

    @staticmethod
    def forward(ctx, frequencies, amplitudes, sample_rate, reduction):
        ctx.save_for_backward(frequencies, amplitudes)
        ctx.args = (sample_rate, reduction)
        return _oscillator_bank_launch(frequencies.detach(), amplitudes.detach(), sample_rate, reduction)

    @staticmethod
    def backward(ctx, dy):
        frequencies, amplitudes = ctx.saved_tensors
        sample_rate, reduction = ctx.args
        need_f, need_a = ctx.needs_input_grad[:2]
        if torch.is_grad_enabled():
            # create_graph=True: differentiate the differentiable composition instead (see _MelSpectrogramFunction)
            with torch.enable_grad():
                y = _diff.oscillator_bank(frequencies, amplitudes, sample_rate, reduction)
                wanted = [t for t, need in ((frequencies, need_f), (amplitudes, need_a)) if need]
                grads = list(torch.autograd.grad(y, wanted, dy, create_graph=True))
            return grads.pop(0) if need_f else None, grads.pop(0) if need_a else None, None, None
        T_, N = frequencies.shape[-2:]
        f3, a3 = _dsp_rows3(frequencies), _dsp_rows3(amplitudes)
        rows = f3.shape[0]
        g = dy.detach().contiguous()
        dev = f3.device
        gf = torch.empty((rows, T_, N), dtype=f3.dtype, device=dev) if need_f else None
        ga = torch.empty((rows, T_, N), dtype=f3.dtype, device=dev) if need_a else None
        lib = _lib.lib()
        ws = torch.empty((max(int(lib.aamd_oscillator_grad_workspace(rows, T_, N)) // 8, 1),), dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.aamd_oscillator_bank_grad(_SA_DTYPES[f3.dtype], f3.data_ptr(), a3.data_ptr(), g.data_ptr(),
                                                     gf.data_ptr() if need_f else None, ga.data_ptr() if need_a else None,
                                                     ws.data_ptr(), rows, T_, N, f3.stride(0) if rows > 1 else 0,
                                                     a3.stride(0) if rows > 1 else 0, float(sample_rate), _DSP_REDUCTIONS[reduction],
                                                     _lib.current_stream(dev)))
        return (gf.reshape(frequencies.shape) if need_f else None, ga.reshape(amplitudes.shape) if need_a else None, None, None)


class _FilterWaveformFunction(torch.autograd.Function):
    """filter_waveform in training mode: forward = the launch of the inference path (the same bits); backward =
    aamd_filter_waveform_grad (csrc/dsp_synth_grad.h): grad_waveform in one launch shaped like the forward, grad_kernels as a
    float64 reduction in a fixed order (one or two launches), only for the inputs that need one.  All HIP kernels; nothing of
    (rows, time, L) is ever allocated."""

    @staticmethod
    def forward(ctx, waveform, kernels):
        ctx.save_for_backward(waveform, kernels)
        return _filter_waveform_launch(waveform.detach(), kernels.detach())

    @staticmethod
    def backward(ctx, dy):
        waveform, kernels = ctx.saved_tensors
        need_x, need_h = ctx.needs_input_grad[:2]
        T_ = waveform.shape[-1]
        F_, L = kernels.shape[-2:]
        lead = tuple(waveform.shape[:-1])
        rows = 1
        for d in lead:
            rows *= d
        if torch.is_grad_enabled():
            # create_graph=True: differentiate the differentiable composition instead (see _MelSpectrogramFunction)
            with torch.enable_grad():
                y = _diff.filter_waveform(waveform.reshape(rows, T_), kernels).reshape(lead + (T_,))
                wanted = [t for t, need in ((waveform, need_x), (kernels, need_h)) if need]
                grads = list(torch.autograd.grad(y, wanted, dy, create_graph=True))
            return grads.pop(0) if need_x else None, grads.pop(0) if need_h else None
        dev = waveform.device
        batched = 1 if kernels.dim() == 3 else 0
        x2 = _wa_rows(waveform.detach(), lead, T_)
        h = kernels.detach().contiguous()
        g = dy.detach().reshape(rows, T_).contiguous()
        gx = torch.empty((rows, T_), dtype=x2.dtype, device=dev) if need_x else None
        gh = torch.empty(tuple(kernels.shape), dtype=x2.dtype, device=dev) if need_h else None
        lib = _lib.lib()
        nbytes = int(lib.aamd_filter_waveform_grad_workspace(rows, T_, F_, L, batched)) if need_h else 0
        ws = torch.empty((max(nbytes // 8, 1),), dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.aamd_filter_waveform_grad(_SA_DTYPES[x2.dtype], x2.data_ptr(), h.data_ptr(), g.data_ptr(),
                                                     gx.data_ptr() if need_x else None, gh.data_ptr() if need_h else None,
                                                     ws.data_ptr(), rows, T_, _wa_stride(x2), F_, L, batched,
                                                     _lib.current_stream(dev)))
        return gx.reshape(waveform.shape) if need_x else None, gh


def dsp_grad_tiles() -> Tuple[int, int]:
    """(samples per unit of time, lags per workgroup) of the filter-gradient reduction of csrc/dsp_synth_grad.h: dsp::kGhPiece,
    kGhLags."""
    lib = _lib.lib()
    return tuple(int(lib.aamd_dsp_grad_tiles(i)) for i in range(2))


def sinc_impulse_response(cutoff: Tensor, window_size: int = 513, high_pass: bool = False) -> Tensor:
    r"""Windowed-sinc low-pass (or high-pass) filters (reference: ``torchaudio.prototype.functional.sinc_impulse_response``):
    ``cutoff`` is ``(...)`` with 1 meaning Nyquist, the result ``(..., window_size)``.  With ``half = window_size // 2`` and
    ``i = -half .. half``: ``g[i] = sinc(cutoff i) hamming(window_size)[i + half]`` (the symmetric window; ``[1]`` for one
    tap), ``h = g / |sum g|``; ``high_pass`` gives ``-h`` with 1 added to the centre tap.  One launch, evaluated in float64
    for float32 and float64 alike and rounded once.  An input that requires grad takes the differentiable composition."""
    what = "sinc_impulse_response"
    _dsp_tensor(what, "cutoff", cutoff, _DSP_WIDE)
    if isinstance(window_size, bool) or not isinstance(window_size, int):
        raise TypeError(f"audio_amd: {what}: window_size must be an int (got {window_size!r})")
    if window_size <= 0 or window_size % 2 == 0:
        raise ValueError(f"audio_amd: {what}: window_size must be odd and positive (got {window_size})")
    if window_size >= 2 ** 31:
        raise ValueError(f"audio_amd: {what}: window_size is beyond 2^31")
    _wa_require(cutoff, f"{what}: cutoff")
    if _dsp_grad(cutoff):
        return _diff.sinc_impulse_response(cutoff, window_size, bool(high_pass))
    out = torch.empty(tuple(cutoff.shape) + (window_size,), dtype=cutoff.dtype, device=cutoff.device)
    if out.numel() == 0:
        return out
    c1 = cutoff.detach().contiguous().reshape(-1)
    with torch.cuda.device(out.device):
        _lib.check(_lib.lib().aamd_sinc_impulse_response(_SA_DTYPES[out.dtype], c1.data_ptr(), out.data_ptr(), c1.shape[0],
                                                         window_size, 1 if high_pass else 0, _lib.current_stream(out.device)))
    return out


def frequency_impulse_response(magnitudes: Tensor) -> Tensor:
    r"""Linear-phase filters from magnitude responses (reference:
    ``torchaudio.prototype.functional.frequency_impulse_response``): ``magnitudes`` is ``(..., n)`` with ``n >= 2``, the
    result ``(..., N)`` with ``N = 2 (n - 1)``: the inverse real FFT, ``ir[k] = (m_0 + (-1)^k m_{n-1} + 2 sum_j m_j cos(2 pi
    j k / N)) / N``, shifted by ``N / 2`` and multiplied by the symmetric Hann window.  One launch: one workgroup per filter,
    one fused multiply-add chain per tap over a host-built cosine table (cached per ``(n, dtype, device)``: run the call once
    eagerly before capturing it in a graph).  No check for negative magnitudes (the reference's synchronises).  ``n`` up to
    ``DSP_MAX_MAGNITUDES``.  An input that requires grad takes the differentiable composition."""
    what = "frequency_impulse_response"
    _dsp_tensor(what, "magnitudes", magnitudes, _DSP_WIDE)
    if magnitudes.dim() < 1 or magnitudes.shape[-1] < 2:
        raise ValueError(f"audio_amd: {what}: magnitudes must be (..., n) with n >= 2 (got {tuple(magnitudes.shape)})")
    n = magnitudes.shape[-1]
    if n > DSP_MAX_MAGNITUDES:
        raise NotImplementedError(f"audio_amd: {what} serves up to {DSP_MAX_MAGNITUDES} magnitudes (got {n})")
    _wa_require(magnitudes, f"{what}: magnitudes")
    if _dsp_grad(magnitudes):
        return _diff.frequency_impulse_response(magnitudes)
    out = torch.empty(tuple(magnitudes.shape[:-1]) + (2 * (n - 1),), dtype=magnitudes.dtype, device=magnitudes.device)
    if out.numel() == 0:
        return out
    dt = magnitudes.dtype
    table = _device_table("cosine table", ("fir_cos", n, str(dt)), out.device, lambda: _host.round_once(_host.fir_cos_table(n), dt))
    m2 = magnitudes.detach().contiguous().reshape(-1, n)
    with torch.cuda.device(out.device):
        _lib.check(_lib.lib().aamd_frequency_impulse_response(_SA_DTYPES[dt], m2.data_ptr(), table.data_ptr(), out.data_ptr(),
                                                              m2.shape[0], n, _lib.current_stream(out.device)))
    return out


def adsr_envelope(num_frames: int, *, attack: float = 0.0, hold: float = 0.0, decay: float = 0.0, sustain: float = 1.0,
                  release: float = 0.0, n_decay: int = 2, dtype: Optional[torch.dtype] = None, device=None) -> Tensor:
    r"""An attack-hold-decay-sustain-release envelope of ``num_frames`` samples (reference:
    ``torchaudio.prototype.functional.adsr_envelope``).  With ``n = num_frames - 1`` and ``na, nh, nd, nr = int(n attack),
    int(n hold), int(n decay), int(n release)``: ``sustain`` everywhere, then ``linspace(0, 1, na + 1)`` over the attack, 1
    over the hold, ``linspace(1, 0, nd + 1)^n_decay (1 - sustain) + sustain`` over the decay and ``linspace(sustain, 0, nr +
    1)`` at the end.  Built on the host in float64 and rounded once to ``dtype`` (default: torch's default dtype).
    ``device=None`` is the current ROCm device (the reference defaults to the CPU)."""
    what = "adsr_envelope"
    if isinstance(num_frames, bool) or not isinstance(num_frames, int):
        raise TypeError(f"audio_amd: {what}: num_frames must be an int (got {num_frames!r})")
    if num_frames < 1:
        raise ValueError(f"audio_amd: {what}: num_frames must be at least 1 (got {num_frames})")
    for name, v in (("attack", attack), ("hold", hold), ("decay", decay), ("sustain", sustain), ("release", release)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not 0 <= v <= 1:
            raise ValueError(f"audio_amd: {what}: {name} must lie in [0, 1] (got {v!r})")
    if attack + hold + decay + release > 1 + 4 * 2.0 ** -52:      # three additions of fractions that sum to 1 on paper
        raise ValueError(f"audio_amd: {what}: attack + hold + decay + release must not exceed 1 (got "
                         f"{attack + hold + decay + release})")
    if isinstance(n_decay, bool) or not isinstance(n_decay, int) or n_decay < 0:
        raise ValueError(f"audio_amd: {what}: n_decay must be a non-negative int (got {n_decay!r})")
    dtype = torch.get_default_dtype() if dtype is None else dtype
    if dtype not in _WA_FLOATS:
        raise TypeError(f"audio_amd: {what}: dtype must be float16, bfloat16, float32 or float64 (got {dtype})")
    dev = torch.device(device) if device is not None else (torch.device("cuda", torch.cuda.current_device())
                                                           if torch.cuda.is_available() else torch.device("cpu"))
    if dev.type != "cuda":
        raise RuntimeError(f"audio_amd: {what}: the result must be on an MI355X (ROCm) device, got {dev}. "
                           "The HIP kernels have no CPU fallback.")
    return _host.round_once(_host.adsr_ramp(num_frames, attack, hold, decay, sustain, release, n_decay), dtype).to(dev)


def extend_pitch(base_frequency: Tensor, pattern: Union[int, List[float], Tensor]) -> Tensor:
    r"""Harmonics of a fundamental (reference: ``torchaudio.prototype.functional.extend_pitch``): ``base_frequency`` is ``(...,
    time, 1)``; ``pattern`` is an int ``k`` (the multipliers ``1 .. k``), a list of floats or a 1-D tensor of the same dtype;
    the result is ``(..., time, N)``, each product rounded once (the half types multiply in float32), in one launch.  A
    list's multipliers are rounded once to the dtype and cached on the device: run the call once eagerly before capturing it
    in a graph.  Under grad the result is the broadcast product."""
    what = "extend_pitch"
    _dsp_tensor(what, "base_frequency", base_frequency)
    if base_frequency.dim() < 2 or base_frequency.shape[-1] != 1:
        raise ValueError(f"audio_amd: {what}: base_frequency must be (..., time, 1) (got {tuple(base_frequency.shape)})")
    dt = base_frequency.dtype
    values = None
    if isinstance(pattern, Tensor):
        if pattern.dim() != 1:
            raise ValueError(f"audio_amd: {what}: a tensor pattern must have one dimension (got {pattern.dim()})")
        if pattern.dtype != dt:
            raise TypeError(f"audio_amd: {what}: pattern must have the dtype of base_frequency ({dt}; got {pattern.dtype})")
    elif isinstance(pattern, bool):
        raise TypeError(f"audio_amd: {what}: pattern must be an int, a list of floats or a tensor (got a bool)")
    elif isinstance(pattern, int):
        if pattern < 0:
            raise ValueError(f"audio_amd: {what}: an int pattern must not be negative (got {pattern})")
        values = tuple(float(i) for i in range(1, pattern + 1))
    elif isinstance(pattern, (list, tuple)):
        if not all(isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v) for v in pattern):
            raise TypeError(f"audio_amd: {what}: a list pattern must hold finite numbers")
        values = tuple(float(v) for v in pattern)
    else:
        raise TypeError(f"audio_amd: {what}: pattern must be an int, a list of floats or a tensor (got {type(pattern).__name__})")
    _wa_require(base_frequency, f"{what}: base_frequency")
    dev = base_frequency.device
    if values is None:
        _wa_require(pattern, f"{what}: pattern")
        if pattern.device != dev:
            raise ValueError(f"audio_amd: {what}: base_frequency and pattern must be on one device")
        pat = pattern
    elif len(values) == 0:
        pat = torch.empty((0,), dtype=dt, device=dev)
    else:
        pat = _device_table("pitch pattern", ("extend_pitch", values, str(dt)), dev,
                            lambda: _host.round_once(np.asarray(values, np.float64), dt))
    if _dsp_grad(base_frequency, pat):
        return base_frequency * pat
    N = pat.shape[0]
    out = torch.empty(tuple(base_frequency.shape[:-1]) + (N,), dtype=dt, device=dev)
    if out.numel() == 0:
        return out
    b1 = base_frequency.detach().contiguous().reshape(-1)
    p1 = pat.detach().contiguous()
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().aamd_extend_pitch(_SA_DTYPES[dt], b1.data_ptr(), p1.data_ptr(), out.data_ptr(), b1.shape[0], N,
                                                _lib.current_stream(dev)))
    return out


# --------------------------------------------------------------------------- #
# CTC forced alignment (csrc/forced_align.h)                                  #
# --------------------------------------------------------------------------- #
FORCED_ALIGN_MAX_L = 2047            # AAMD_FORCED_ALIGN_MAX_L: the longest transcript axis the forward kernel serves
_ALIGN_INTS = (torch.int32, torch.int64)


def forced_align_tiles() -> Tuple[Tuple[Tuple[int, int, int], ...], int, int, int]:
    """(((largest L, states per lane, lanes per workgroup) of every forward configuration, by L), steps the forward's
    gathers run ahead, frames per backtrack block, largest L) of csrc/forced_align.h."""
    lib = _lib.lib()
    configs, prev = [], None
    for L in range(FORCED_ALIGN_MAX_L + 1):
        cur = (int(lib.aamd_forced_align_states_per_lane(L)), int(lib.aamd_forced_align_threads(L)))
        if cur != prev and prev is not None:
            configs.append((L - 1,) + prev)
        prev = cur
    configs.append((FORCED_ALIGN_MAX_L,) + prev)
    return tuple(configs), int(lib.aamd_forced_align_prefetch()), int(lib.aamd_forced_align_backtrack_block()), FORCED_ALIGN_MAX_L


def _forced_align_check(log_probs: Tensor, targets: Tensor, input_lengths: Optional[Tensor], target_lengths: Optional[Tensor],
                        blank: int) -> None:
    """The host-side checks of F.forced_align, with the reference's exception types.  Nothing is read from the device."""
    if log_probs.dim() != 3:
        raise ValueError(f"log_probs must be 3-D (batch, frame, class), got {tuple(log_probs.shape)}")
    if targets.dim() != 2:
        raise ValueError(f"targets must be 2-D (batch, label), got {tuple(targets.shape)}")
    B, T_, C_ = log_probs.shape
    if targets.shape[0] != B:
        raise ValueError(f"batch sizes differ: log_probs {B}, targets {targets.shape[0]}")
    for t, what in ((input_lengths, "input_lengths"), (target_lengths, "target_lengths")):
        if t is not None and (t.dim() != 1 or t.shape[0] != B):
            raise ValueError(f"{what} must be 1-D of the batch size {B}, got {tuple(t.shape)}")
    if T_ < 1 or C_ < 1:
        raise ValueError(f"log_probs needs at least one frame and one class, got {tuple(log_probs.shape)}")
    if log_probs.dtype not in _RNNT_DTYPES:
        raise TypeError(f"log_probs must be float32, float64, float16 or bfloat16 (got {log_probs.dtype})")
    if targets.dtype not in _ALIGN_INTS:
        raise TypeError(f"targets must be int32 or int64 (got {targets.dtype})")
    lengths = [(t, what) for t, what in ((input_lengths, "input_lengths"), (target_lengths, "target_lengths")) if t is not None]
    for t, what in lengths:
        if t.dtype not in _ALIGN_INTS:
            raise TypeError(f"{what} must be int32 or int64 (got {t.dtype})")
    if len(lengths) == 2 and input_lengths.dtype != target_lengths.dtype:
        raise TypeError(f"input_lengths and target_lengths must have one dtype (got {input_lengths.dtype} and "
                        f"{target_lengths.dtype})")
    tensors = [(log_probs, "log_probs"), (targets, "targets")] + lengths
    for t, what in tensors:
        if not t.is_contiguous():
            raise ValueError(f"{what} must be contiguous")
    if blank >= C_ or blank < 0:
        raise ValueError("blank must be within [0, log_probs.shape[-1])")
    if targets.shape[1] > FORCED_ALIGN_MAX_L:
        raise NotImplementedError(f"audio_amd: forced_align serves transcripts up to L = {FORCED_ALIGN_MAX_L} labels (got "
                                  f"{targets.shape[1]}): the lattice of one example belongs to one workgroup")
    for t, what in tensors:
        if not t.is_cuda:
            raise RuntimeError(f"audio_amd: {what} must be on an MI355X (ROCm) device, got {t.device}. "
                               "The HIP kernels have no CPU fallback.")
        if t.device != log_probs.device:
            raise RuntimeError(f"audio_amd: {what} must be on the log_probs' device")


def _forced_align_launch(log_probs: Tensor, targets: Tensor, input_lengths: Tensor, target_lengths: Tensor,
                         blank: int) -> Tuple[Tensor, Tensor]:
    """(paths, scores): the forward and the backtrack through the C ABI.  The workspace is written and read on the device only."""
    B, T_, C_ = log_probs.shape
    L = targets.shape[1]
    lib = _lib.lib()
    paths = torch.empty((B, T_), dtype=targets.dtype, device=log_probs.device)
    scores = torch.empty((B, T_), dtype=log_probs.dtype, device=log_probs.device)
    if B:
        ws = torch.empty((max(int(lib.aamd_forced_align_workspace(B, T_, L)), 16),), dtype=torch.uint8, device=log_probs.device)
        with torch.cuda.device(log_probs.device):
            _lib.check(lib.aamd_forced_align(_RNNT_DTYPES[log_probs.dtype], _lib.ptr(log_probs), _lib.ptr(targets) or None,
                                             int(targets.dtype == torch.int64), _lib.ptr(input_lengths), _lib.ptr(target_lengths),
                                             int(input_lengths.dtype == torch.int64), B, T_, C_, L, blank, ws.data_ptr(),
                                             paths.data_ptr(), scores.data_ptr(), _lib.current_stream(log_probs.device)))
    return paths, scores


def forced_align(log_probs: Tensor, targets: Tensor, input_lengths: Optional[Tensor] = None,
                 target_lengths: Optional[Tensor] = None, blank: int = 0) -> Tuple[Tensor, Tensor]:
    r"""CTC forced alignment (reference: F.forced_align): the most likely frame-level labelling of ``log_probs`` ``(B, T, C)``
    that collapses to ``targets`` ``(B, L)``.  Returns ``paths`` ``(B, T)`` in the dtype of ``targets`` and ``scores`` ``(B, T)``,
    the elements ``log_probs[b, t, paths[b, t]]`` copied bit for bit.  The Viterbi recurrence accumulates in float64 for every
    input dtype; ties keep the smaller move.  The whole time loop and the backtrack run on the device in two launches, the
    lengths and labels are read there -- no synchronisation, so the call can be captured in a graph -- and a ragged batch is
    served (the reference refuses ``B > 1``).  Frames from ``input_lengths[b]`` on get ``blank`` / 0; an example that cannot be
    aligned (a length out of range, fewer frames than labels plus adjacent equal labels, a live label outside ``[0, C)`` or
    equal to ``blank``) gets ``-1`` / NaN over its whole row instead of the reference's host-side error.  A plain Python entry
    point through the C ABI: not registered as a dispatcher op."""
    _forced_align_check(log_probs, targets, input_lengths, target_lengths, blank)
    B, T_, _ = log_probs.shape
    ldt = (input_lengths if input_lengths is not None else target_lengths if target_lengths is not None else targets).dtype
    if input_lengths is None:
        input_lengths = torch.full((B,), T_, dtype=ldt, device=log_probs.device)
    if target_lengths is None:
        target_lengths = torch.full((B,), targets.shape[1], dtype=ldt, device=log_probs.device)
    return _forced_align_launch(log_probs.detach(), targets, input_lengths, target_lengths, int(blank))


@dataclasses.dataclass
class TokenSpan:
    """A run of one token in an alignment (reference: F.TokenSpan): frames ``[start, end)`` and their mean score."""
    token: int
    start: int
    end: int
    score: float

    def __len__(self) -> int:
        return self.end - self.start


def merge_tokens(tokens: Tensor, scores: Tensor, blank: int = 0) -> List[TokenSpan]:
    r"""Runs of equal tokens of a frame-level alignment as ``TokenSpan``s, blank runs dropped (reference: F.merge_tokens).
    ``score`` is the mean of the run's scores in float64.  The result is a Python list, so the two tensors are copied to the
    host once, from any device, and the rest is host bookkeeping."""
    if tokens.ndim != 1 or scores.ndim != 1:
        raise ValueError("`tokens` and `scores` must be 1D Tensor.")
    if len(tokens) != len(scores):
        raise ValueError("`tokens` and `scores` must be the same length.")
    n = len(tokens)
    if n == 0:
        return []
    if tokens.device.type != "cpu":                            # one device-to-host copy of both
        packed = torch.stack((tokens.to(torch.float64), scores.detach().to(torch.float64))).cpu().numpy()
        tok, sc = packed[0].astype(np.int64), packed[1]
    else:
        tok, sc = tokens.numpy().astype(np.int64), scores.detach().to(torch.float64).numpy()
    edges = [0] + (np.flatnonzero(tok[1:] != tok[:-1]) + 1).tolist() + [n]
    return [TokenSpan(token=int(tok[s]), start=s, end=e, score=float(sc[s:e].mean()))
            for s, e in zip(edges[:-1], edges[1:]) if tok[s] != blank]


# --------------------------------------------------------------------------- #
# batched edit distance (csrc/edit_distance.h)                                #
# --------------------------------------------------------------------------- #
EDIT_MAX_REF = 4096                  # AAMD_EDIT_DISTANCE_MAX_REF: the widest reference axis the kernel serves
EDIT_MAX_HYP = 32767                 # AAMD_EDIT_DISTANCE_MAX_HYP: the widest hypothesis axis


def edit_distance_tiles() -> Tuple[Tuple[Tuple[int, int, int], ...], int, int]:
    """(((largest reference width M, rows per lane, lanes per workgroup) of every configuration, by M), largest M, largest
    hypothesis width N) of csrc/edit_distance.h."""
    lib = _lib.lib()
    configs, prev = [], None
    for M in range(EDIT_MAX_REF + 1):
        cur = (int(lib.aamd_edit_distance_states_per_lane(M)), int(lib.aamd_edit_distance_threads(M)))
        if cur != prev and prev is not None:
            configs.append((M - 1,) + prev)
        prev = cur
    configs.append((EDIT_MAX_REF,) + prev)
    return tuple(configs), int(lib.aamd_edit_distance_max_ref()), int(lib.aamd_edit_distance_max_hyp())


def _edit_distance_check(hyps: Tensor, refs: Tensor, hyp_lengths: Optional[Tensor], ref_lengths: Optional[Tensor]) -> None:
    """The host-side checks of F.edit_distance_batch.  Nothing is read from the device."""
    if hyps.dim() < 1 or refs.dim() < 1:
        raise ValueError(f"hyps and refs need a token axis, got {tuple(hyps.shape)} and {tuple(refs.shape)}")
    lead, rlead = tuple(hyps.shape[:-1]), tuple(refs.shape[:-1])
    if len(rlead) > len(lead) or lead[:len(rlead)] != rlead:
        raise ValueError(f"the leading axes of refs {rlead} must be a prefix of those of hyps {lead}")
    for t, what, want in ((hyp_lengths, "hyp_lengths", lead), (ref_lengths, "ref_lengths", rlead)):
        if t is not None and tuple(t.shape) != want:
            raise ValueError(f"{what} must have the shape {want}, got {tuple(t.shape)}")
    tensors = [(hyps, "hyps"), (refs, "refs")] + [(t, what) for t, what in ((hyp_lengths, "hyp_lengths"),
                                                                             (ref_lengths, "ref_lengths")) if t is not None]
    for t, what in tensors:
        if t.dtype not in _ALIGN_INTS:
            raise TypeError(f"{what} must be int32 or int64 (got {t.dtype})")
    for t, what in tensors:
        if not t.is_contiguous():
            raise ValueError(f"{what} must be contiguous")
    if refs.shape[-1] > EDIT_MAX_REF or hyps.shape[-1] > EDIT_MAX_HYP:
        raise NotImplementedError(f"audio_amd: edit_distance serves references up to M = {EDIT_MAX_REF} tokens and hypotheses up "
                                  f"to N = {EDIT_MAX_HYP} (got M = {refs.shape[-1]}, N = {hyps.shape[-1]}): the reference of one "
                                  "pair lies across the registers of one workgroup; the distance is symmetric, so the arguments "
                                  "may be swapped (which swaps deletions and insertions)")
    for t, what in tensors:
        if not t.is_cuda:
            raise RuntimeError(f"audio_amd: {what} must be on an MI355X (ROCm) device, got {t.device}. "
                               "The HIP kernels have no CPU fallback.")
        if t.device != hyps.device:
            raise RuntimeError(f"audio_amd: {what} must be on the hyps' device")


def edit_distance_batch(hyps: Tensor, refs: Tensor, hyp_lengths: Optional[Tensor] = None, ref_lengths: Optional[Tensor] = None,
                        return_ops: bool = False) -> Tensor:
    r"""Levenshtein distance of every hypothesis ``hyps`` ``(*lead, N)`` to its reference ``refs`` ``(*rlead, M)``, ``rlead`` a
    prefix of ``lead``: a reference serves the whole block of hypotheses beneath it, so the ``(B, nbest, N)`` tokens of
    ``ctc_beam_search`` go against ``(B, M)`` transcripts as they are.  Tokens are int32 or int64 (the two tensors may differ;
    they are compared as integers), lengths int32 or int64 of the shapes ``lead`` / ``rlead`` (``None``: the full width).
    Returns int32 ``lead``: the distance; with ``return_ops`` int32 ``(*lead, 4)``: (distance, substitutions, deletions,
    insertions) of one fixed optimal alignment -- every cell takes the first of diagonal, deletion (a reference token without a
    partner), insertion whose cost is smallest -- so ``distance == S + D + I`` and ``N_p == M_p - D + I``.  A pair whose length
    lies outside ``[0, N]`` / ``[0, M]`` (the ``-1`` of a hypothesis the beam did not hold) gets ``-1`` in every field, and no
    token of it is read.  One launch, lengths read on the device, no synchronisation, nothing cached: the first call can be
    captured in a graph.  Integers only: two calls give the same bits, and row p of a batch equals the pair alone.  No
    gradient.  References beyond ``EDIT_MAX_REF`` or hypotheses beyond ``EDIT_MAX_HYP`` tokens raise NotImplementedError.  A
    plain Python entry point through the C ABI: not registered as a dispatcher op."""
    _edit_distance_check(hyps, refs, hyp_lengths, ref_lengths)
    lead = tuple(hyps.shape[:-1])
    pairs, rows = math.prod(lead), math.prod(refs.shape[:-1])
    out = torch.empty(lead + ((4,) if return_ops else ()), dtype=torch.int32, device=hyps.device)
    if pairs:
        is64 = lambda t: int(t is not None and t.dtype == torch.int64)   # noqa: E731
        p = lambda t: (_lib.ptr(t) or None) if t is not None else None   # noqa: E731
        with torch.cuda.device(hyps.device):
            _lib.check(_lib.lib().aamd_edit_distance(p(hyps), is64(hyps), p(refs), is64(refs), p(hyp_lengths), is64(hyp_lengths),
                                                     p(ref_lengths), is64(ref_lengths), pairs, pairs // rows, hyps.shape[-1],
                                                     refs.shape[-1], int(bool(return_ops)), out.data_ptr(),
                                                     _lib.current_stream(hyps.device)))
    return out


def edit_distance(seq1, seq2) -> int:
    r"""Levenshtein distance of two sequences (reference: F.edit_distance, a Python loop over the cells on the host), ``seq1``
    taken as the reference of ``edit_distance_batch``.  Two 1-D integer tensors on the device go to the kernel as one pair;
    any other pair of Python sequences (strings, lists of words) is interned to ids with a dict on the host, uploaded to the
    current ROCm device and goes the same way.  The Python ``int`` costs one small device-to-host copy, so this entry point
    synchronises and cannot be captured in a graph; ``edit_distance_batch`` can."""
    t1, t2 = isinstance(seq1, Tensor), isinstance(seq2, Tensor)
    if t1 != t2:
        raise TypeError("edit_distance takes two tensors or two Python sequences, not one of each")
    if t1:
        if seq1.dim() != 1 or seq2.dim() != 1:
            raise ValueError(f"seq1 and seq2 must be 1-D, got {tuple(seq1.shape)} and {tuple(seq2.shape)}")
        return int(edit_distance_batch(seq2, seq1).item())
    if not torch.cuda.is_available():
        raise RuntimeError("audio_amd: edit_distance must run on an MI355X (ROCm) device and none is available. "
                           "The HIP kernels have no CPU fallback.")
    ids: dict = {}
    a = [ids.setdefault(x, len(ids)) for x in seq1]
    b = [ids.setdefault(x, len(ids)) for x in seq2]
    dev = torch.device("cuda", torch.cuda.current_device())
    both = torch.tensor(a + b, dtype=torch.int32).to(dev)
    return int(edit_distance_batch(both[len(a):], both[:len(a)]).item())


# --------------------------------------------------------------------------- #
# STOI / ESTOI speech intelligibility (csrc/stoi.h)                           #
# --------------------------------------------------------------------------- #
STOI_SAMPLE_RATE = 10000             # the rate the measure is defined at; other rates go through F.resample first


def stoi_tiles() -> Tuple[int, int, int, int, int]:
    """(threads per workgroup, frames per workgroup of the energy kernel, output frames per workgroup of the band kernel,
    segments per workgroup of the segment kernel, threads per row of the finishing kernel) of csrc/stoi.h: stoi::kThreads,
    kEnergyFrames, kTobFrames, kSegTile, kFinishThreads."""
    lib = _lib.lib()
    return tuple(int(lib.aamd_stoi_tiles(i)) for i in range(5))


def _stoi_check(preds: Tensor, target: Tensor, sample_rate: int, lengths: Optional[Tensor]) -> None:
    """The host-side checks of F.stoi, in the order shapes, parameters, dtypes, gradient, device.  Nothing is read from the
    device."""
    if not isinstance(preds, Tensor) or not isinstance(target, Tensor):
        raise TypeError("audio_amd: stoi: preds and target must be tensors")
    if preds.dim() < 1 or target.dim() < 1:
        raise ValueError(f"audio_amd: stoi expects (..., time), got {tuple(preds.shape)} and {tuple(target.shape)}")
    if preds.shape != target.shape:
        raise ValueError(f"audio_amd: stoi: preds and target must have the same shape, got {tuple(preds.shape)} and "
                         f"{tuple(target.shape)}")
    if isinstance(sample_rate, bool) or not isinstance(sample_rate, int) or sample_rate <= 0:
        raise ValueError(f"audio_amd: stoi: sample_rate must be a positive integer (got {sample_rate!r})")
    if lengths is not None and (not isinstance(lengths, Tensor) or tuple(lengths.shape) != tuple(preds.shape[:-1])):
        raise ValueError(f"audio_amd: stoi: lengths must have the shape {tuple(preds.shape[:-1])}, got "
                         f"{tuple(lengths.shape) if isinstance(lengths, Tensor) else type(lengths).__name__}")
    if preds.dtype not in _WA_FLOATS or target.dtype not in _WA_FLOATS:
        raise TypeError(f"audio_amd: stoi: preds and target must be float16, bfloat16, float32 or float64 (got {preds.dtype} "
                        f"and {target.dtype})")
    if preds.dtype != target.dtype:
        raise TypeError(f"audio_amd: stoi: preds and target must share a dtype (got {preds.dtype} and {target.dtype})")
    if lengths is not None and lengths.dtype not in _ALIGN_INTS:
        raise TypeError(f"audio_amd: stoi: lengths must be int32 or int64 (got {lengths.dtype})")
    if torch.is_grad_enabled() and (preds.requires_grad or target.requires_grad):
        raise RuntimeError("audio_amd: stoi is forward-only (no gradient is implemented); wrap the call in torch.no_grad() or "
                           "detach the waveforms.")
    for t, what in ((preds, "preds"), (target, "target"), (lengths, "lengths")):
        if t is not None and not t.is_cuda:
            raise RuntimeError(f"audio_amd: stoi: {what} must be on an MI355X (ROCm) device, got {t.device}. "
                               "The HIP kernels have no CPU fallback.")
        if t is not None and t.device != preds.device:
            raise RuntimeError(f"audio_amd: stoi: {what} must be on the preds' device")


def stoi(preds: Tensor, target: Tensor, sample_rate: int, extended: bool = False, lengths: Optional[Tensor] = None) -> Tensor:
    r"""Short-time objective intelligibility of the processed ``preds`` against the clean ``target``, both ``(..., time)``
    (the argument order and names of torchmetrics' ``short_time_objective_intelligibility``, which loops pystoi over one
    utterance at a time in float64 numpy on the host): every row is scored on its own, the result has the shape
    ``preds.shape[:-1]`` and stays on the device.  ``extended=True`` gives ESTOI.  ``lengths`` (``preds.shape[:-1]``, int32 or
    int64, on the device) ends row b at sample ``lengths[b]``; nothing at or beyond it is read.

    The measure (Taal et al. 2011; Jensen & Taal 2016) at 10 kHz: 256-sample Hann frames (``hanning(258)[1:-1]``) at hop 128;
    the frames of the clean signal within 40 dB of its loudest frame are kept and both signals are rebuilt from them by
    overlap-add; 512-point spectra of the rebuilt signals' frames (all but the last), 15 third-octave band magnitudes from
    150 Hz; over every run of 30 frames the band-wise correlation of the clean and the normalised, clipped processed
    magnitudes (STOI), or the correlation of the row- and column-normalised 15 x 30 blocks (ESTOI), averaged.  Fewer than 30
    such frames score ``1e-5`` (without pystoi's warning).  Any other ``sample_rate`` goes through this package's
    ``F.resample(., sample_rate, 10000)`` with its defaults first (pystoi uses an Octave-compatible polyphase filter, so
    scores differ there), and ``lengths`` becomes ``ceil(lengths * 10000 / sample_rate)``.

    float32 is the kernel path; float16 / bfloat16 are widened on load and return float32; float64 runs the same kernels on
    double and returns float64.  The frame energies and the 40 dB decision are float64 for every dtype, the segment statistic
    too.  Five launches, no atomics, no host read-back: two calls give the same bits, row b of a batch equals the call on row
    b, and a row with ``lengths[b]`` equals the call on ``row[:lengths[b]]``.  The window and the twiddles are computed in the
    kernels, nothing is cached, so the first call can be captured in a graph (at ``sample_rate != 10000`` the resampler's
    cached kernel is needed: run that call once eagerly).  A row with a non-finite sample below its length, or a length
    outside ``[0, time]``, scores NaN; other rows keep their bits.  ``ValueError`` for different shapes, 0-dimensional input,
    ``sample_rate <= 0`` or ``lengths`` of another shape; ``TypeError`` for non-floating or mixed dtypes; no gradient.  A
    plain Python entry point through the C ABI: not registered as a dispatcher op."""
    _stoi_check(preds, target, sample_rate, lengths)
    lead = tuple(preds.shape[:-1])
    preds, target = preds.detach(), target.detach()
    if sample_rate != STOI_SAMPLE_RATE:
        if lengths is not None:
            # ceil(lengths * 10000 / sample_rate) as F.speed does, in integers (exact at every length); a length outside
            # [0, time] stays outside
            scaled = torch.div(lengths.to(torch.int64) * STOI_SAMPLE_RATE + (sample_rate - 1), sample_rate, rounding_mode="floor")
            lengths = torch.where((lengths < 0) | (lengths > preds.shape[-1]), -1, scaled).to(lengths.dtype)
        preds = resample(preds, sample_rate, STOI_SAMPLE_RATE)
        target = resample(target, sample_rate, STOI_SAMPLE_RATE)
    T_ = preds.shape[-1]
    p2, t2 = _wa_rows(preds, lead, T_), _wa_rows(target, lead, T_)
    rows = p2.shape[0]
    if rows > 1 and p2.stride(0) < T_:             # expanded rows: the launcher takes rows that do not overlap
        p2 = p2.contiguous()
    if rows > 1 and t2.stride(0) < T_:
        t2 = t2.contiguous()
    out = torch.empty((rows,), dtype=torch.float64 if preds.dtype == torch.float64 else torch.float32, device=preds.device)
    if rows:
        lib = _lib.lib()
        dt = _SA_DTYPES[p2.dtype]
        ws = torch.empty((max(int(lib.aamd_stoi_workspace(dt, rows, T_)) // 8, 1),), dtype=torch.float64, device=preds.device)
        len1 = lengths.reshape(-1).contiguous() if lengths is not None else None
        with torch.cuda.device(preds.device):
            _lib.check(lib.aamd_stoi(dt, _lib.ptr(p2) or None, _lib.ptr(t2) or None, rows, T_, _wa_stride(p2), _wa_stride(t2),
                                     len1.data_ptr() if len1 is not None else None, int(len1 is not None and len1.dtype == torch.int64),
                                     int(bool(extended)), ws.data_ptr(), out.data_ptr(), _lib.current_stream(preds.device)))
    return out.view(lead)


@_reduced_precision_io
def _convolve_eager(x: Tensor, y: Tensor, mode: str = "full") -> Tensor:
    r"""Linear convolution along the last dim with broadcast leading dims and the reference's full / valid / same crops
    (reference: F.convolve, a grouped conv1d).  The longer operand is taken as the signal, as the reference swaps them.
    The product is evaluated by the package's convolution plans: up to 192 taps as a direct sum in the time domain, longer
    kernels through the block FFT kernels, so those agree with the direct sum to rounding, not bit for bit.
    Differentiable in both operands."""
    _check_shape_compatible(x, y)
    _check_convolve_mode(mode)
    if not x.is_floating_point():
        x = x.float()
    if not y.is_floating_point():
        y = y.float()
    _require_device(x, "x", allow_grad=True, allow_f64=True)
    _require_device(y, "y", allow_grad=True, allow_f64=True)
    if x.dtype != y.dtype:
        raise TypeError(f"audio_amd: convolve operands must share a dtype (got {x.dtype} and {y.dtype})")
    x_size, y_size = x.size(-1), y.size(-1)
    if x_size < y_size:
        x, y = y, x
    n_full = x_size + y_size - 1
    if mode == "full":
        start, out_len = 0, n_full
    elif mode == "valid":
        out_len = max(x_size, y_size) - min(x_size, y_size) + 1
        start = (n_full - out_len) // 2
    else:
        out_len = x_size
        start = (n_full - x_size) // 2
    if torch.is_grad_enabled() and (x.requires_grad or y.requires_grad):
        return _FFTConvolveFunction.apply(x, y, start, out_len)
    return _conv_slice(x, y, start, out_len)


# --------------------------------------------------------------------------- #
# the public entry points                                                     #
# --------------------------------------------------------------------------- #
# Every public function is a small TorchScript-able front (the reference guarantees `torch.jit.script` on this surface:
# test/torchaudio_unittest/functional/torchscript_consistency_impl.py:57, 249, 588-602).  Called from Python it forwards to
# the implementation above (`_<name>_eager`: plan caches, ctypes, autograd Functions -- nothing a compiler should look
# into); inside a scripted program the same call is ONE schema'd operator of the `audio_amd` namespace (audio_amd/_ops.py),
# whose kernel is that same implementation, so scripted and eager results are the same bits.


def _norm_mode(normalized: Union[bool, str]) -> int:
    """`normalized` of the reference's spectrogram as the op schemas' integer: 0 none, 1 "frame_length", 2 "window" / True."""
    if isinstance(normalized, str):
        if normalized == "frame_length":
            return 1
        if normalized == "window":
            return 2
        raise ValueError("Invalid normalized parameter: {}".format(normalized))
    return 2 if normalized else 0


def spectrogram(
    waveform: Tensor,
    pad: int,
    window: Tensor,
    n_fft: int,
    hop_length: int,
    win_length: int,
    power: Optional[float],
    normalized: Union[bool, str],
    center: bool = True,
    pad_mode: str = "reflect",
    onesided: bool = True,
    return_complex: Optional[bool] = None,
) -> Tensor:
    r"""Spectrogram of ``(..., time)`` audio -> ``(..., freq, time)`` (reference: functional/functional.py:54-145); see
    ``_spectrogram_eager``."""
    if not torch.jit.is_scripting():
        return _spectrogram_eager(waveform, pad, window, n_fft, hop_length, win_length, power, normalized, center, pad_mode,
                                  onesided, return_complex)
    return torch.ops.audio_amd.spectrogram(waveform, window, pad, n_fft, hop_length, win_length, power, _norm_mode(normalized),
                                           center, pad_mode, onesided)


def inverse_spectrogram(
    spectrogram: Tensor,
    length: Optional[int],
    pad: int,
    window: Tensor,
    n_fft: int,
    hop_length: int,
    win_length: int,
    normalized: Union[bool, str],
    center: bool = True,
    pad_mode: str = "reflect",
    onesided: bool = True,
) -> Tensor:
    r"""Least-squares inverse of a complex spectrogram (reference: functional/functional.py:148-225); see
    ``_inverse_spectrogram_eager``."""
    if not torch.jit.is_scripting():
        return _inverse_spectrogram_eager(spectrogram, length, pad, window, n_fft, hop_length, win_length, normalized, center,
                                          pad_mode, onesided)
    return torch.ops.audio_amd.inverse_spectrogram(spectrogram, length, window, pad, n_fft, hop_length, win_length,
                                                   _norm_mode(normalized), center, pad_mode, onesided)


def phase_vocoder(complex_specgrams: Tensor, rate: float, phase_advance: Tensor) -> Tensor:
    r"""Stretch a complex spectrogram in time by ``rate`` (reference: functional/functional.py:732-803); see
    ``_phase_vocoder_eager``."""
    if not torch.jit.is_scripting():
        return _phase_vocoder_eager(complex_specgrams, rate, phase_advance)
    return torch.ops.audio_amd.phase_vocoder(complex_specgrams, rate, phase_advance)


def griffinlim(
    specgram: Tensor,
    window: Tensor,
    n_fft: int,
    hop_length: int,
    win_length: int,
    power: float,
    n_iter: int,
    momentum: float,
    length: Optional[int],
    rand_init: bool,
) -> Tensor:
    r"""Griffin-Lim phase recovery (reference: functional/functional.py:255-353); see ``_griffinlim_eager``."""
    if not torch.jit.is_scripting():
        return _griffinlim_eager(specgram, window, n_fft, hop_length, win_length, power, n_iter, momentum, length, rand_init)
    return torch.ops.audio_amd.griffinlim(specgram, window, n_fft, hop_length, win_length, power, n_iter, momentum, length,
                                          rand_init)


def pitch_shift(waveform: Tensor, sample_rate: int, n_steps: int, bins_per_octave: int = 12, n_fft: int = 512,
                win_length: Optional[int] = None, hop_length: Optional[int] = None,
                window: Optional[Tensor] = None) -> Tensor:
    r"""Shift the pitch by ``n_steps`` (reference: functional/functional.py:1596-1641); see ``_pitch_shift_eager``."""
    if not torch.jit.is_scripting():
        return _pitch_shift_eager(waveform, sample_rate, n_steps, bins_per_octave, n_fft, win_length, hop_length, window)
    return torch.ops.audio_amd.pitch_shift(waveform, sample_rate, n_steps, bins_per_octave, n_fft, win_length, hop_length,
                                           window)


def speed(waveform: Tensor, orig_freq: int, factor: float,
          lengths: Optional[Tensor] = None) -> Tuple[Tensor, Optional[Tensor]]:
    r"""Adjust waveform speed (reference: functional/functional.py:2385-2423): resample by 1 / factor.  ``lengths`` keeps its
    own dtype whatever the waveform's (reference :2421)."""
    source_sample_rate = int(factor * orig_freq)
    target_sample_rate = int(orig_freq)
    gcd = math.gcd(source_sample_rate, target_sample_rate)
    source_sample_rate = source_sample_rate // gcd
    target_sample_rate = target_sample_rate // gcd
    if lengths is None:
        out_lengths = None
    else:
        out_lengths = torch.ceil(lengths * target_sample_rate / source_sample_rate).to(lengths.dtype)
    return resample(waveform, source_sample_rate, target_sample_rate), out_lengths


def mel_scale(specgram: Tensor, fb: Tensor) -> Tensor:
    r"""MelScale.forward (reference: transforms/_transforms.py:403-415): (..., freq, time) -> (..., n_mels, time); see
    ``_mel_scale_eager``."""
    if not torch.jit.is_scripting():
        return _mel_scale_eager(specgram, fb)
    return torch.ops.audio_amd.mel_scale(specgram, fb)


def amplitude_to_DB(x: Tensor, multiplier: float, amin: float, db_multiplier: float,
                    top_db: Optional[float] = None) -> Tensor:
    r"""Power / amplitude -> decibel (reference: functional/functional.py:356-404); see ``_amplitude_to_DB_eager``."""
    if not torch.jit.is_scripting():
        return _amplitude_to_DB_eager(x, multiplier, amin, db_multiplier, top_db)
    return torch.ops.audio_amd.amplitude_to_DB(x, multiplier, amin, db_multiplier, top_db)


def _apply_sinc_resample_kernel(waveform: Tensor, orig_freq: int, new_freq: int, gcd: int, kernel: Tensor,
                                width: int) -> Tensor:
    r"""reference: functional/functional.py:1405-1432; see ``_apply_sinc_resample_kernel_eager``."""
    if not torch.jit.is_scripting():
        return _apply_sinc_resample_kernel_eager(waveform, orig_freq, new_freq, gcd, kernel, width)
    return torch.ops.audio_amd.resample_apply(waveform, kernel, orig_freq, new_freq, gcd, width)


def resample(
    waveform: Tensor,
    orig_freq: int,
    new_freq: int,
    lowpass_filter_width: int = 6,
    rolloff: float = 0.99,
    resampling_method: str = "sinc_interp_hann",
    beta: Optional[float] = None,
) -> Tensor:
    r"""Band-limited sinc-interpolation resampling (reference: functional/functional.py:1435-1490); see ``_resample_eager``."""
    if not torch.jit.is_scripting():
        return _resample_eager(waveform, orig_freq, new_freq, lowpass_filter_width, rolloff, resampling_method, beta)
    return torch.ops.audio_amd.resample(waveform, orig_freq, new_freq, lowpass_filter_width, rolloff, resampling_method, beta)


def lfilter(waveform: Tensor, a_coeffs: Tensor, b_coeffs: Tensor, clamp: bool = True, batching: bool = True) -> Tensor:
    r"""IIR filter by the difference equation (reference: functional/filtering.py:1032-1099); see ``_lfilter_eager``."""
    if not torch.jit.is_scripting():
        return _lfilter_eager(waveform, a_coeffs, b_coeffs, clamp, batching)
    return torch.ops.audio_amd.lfilter(waveform, a_coeffs, b_coeffs, clamp, batching)


def biquad_cascade(waveform: Tensor, a_coeffs: Tensor, b_coeffs: Tensor, clamp: bool = True) -> Tensor:
    r"""EXTENSION: ``n_stages`` sequential ``lfilter`` calls fused in one pass; see ``_biquad_cascade_eager``."""
    if not torch.jit.is_scripting():
        return _biquad_cascade_eager(waveform, a_coeffs, b_coeffs, clamp)
    return torch.ops.audio_amd.lfilter_cascade(waveform, a_coeffs, b_coeffs, clamp)


def biquad(waveform: Tensor, b0: float, b1: float, b2: float, a0: float, a1: float, a2: float) -> Tensor:
    r"""Biquad filter (reference: functional/filtering.py:295-333); see ``_biquad_eager``."""
    if not torch.jit.is_scripting():
        return _biquad_eager(waveform, b0, b1, b2, a0, a1, a2)
    return torch.ops.audio_amd.biquad(waveform, b0, b1, b2, a0, a1, a2)


def filtfilt(waveform: Tensor, a_coeffs: Tensor, b_coeffs: Tensor, clamp: bool = True) -> Tensor:
    r"""Forward-backward IIR filtering (reference: functional/filtering.py:672-711); see ``_filtfilt_eager``."""
    if not torch.jit.is_scripting():
        return _filtfilt_eager(waveform, a_coeffs, b_coeffs, clamp)
    return torch.ops.audio_amd.filtfilt(waveform, a_coeffs, b_coeffs, clamp)


# The biquad designers: under TorchScript ONE operator (`audio_amd::designed_biquad`) named by the designer, so that the
# scripted program evaluates the very coefficient formulas of the implementations above.

def lowpass_biquad(waveform: Tensor, sample_rate: int, cutoff_freq: float, Q: float = 0.707) -> Tensor:
    r"""reference: functional/filtering.py:1102-1133."""
    if not torch.jit.is_scripting():
        return _lowpass_biquad_eager(waveform, sample_rate, cutoff_freq, Q)
    return torch.ops.audio_amd.designed_biquad(waveform, "lowpass", sample_rate, [cutoff_freq, Q], False)


def highpass_biquad(waveform: Tensor, sample_rate: int, cutoff_freq: float, Q: float = 0.707) -> Tensor:
    r"""reference: functional/filtering.py:893-923."""
    if not torch.jit.is_scripting():
        return _highpass_biquad_eager(waveform, sample_rate, cutoff_freq, Q)
    return torch.ops.audio_amd.designed_biquad(waveform, "highpass", sample_rate, [cutoff_freq, Q], False)


def allpass_biquad(waveform: Tensor, sample_rate: int, central_freq: float, Q: float = 0.707) -> Tensor:
    r"""reference: functional/filtering.py:70-101."""
    if not torch.jit.is_scripting():
        return _allpass_biquad_eager(waveform, sample_rate, central_freq, Q)
    return torch.ops.audio_amd.designed_biquad(waveform, "allpass", sample_rate, [central_freq, Q], False)


def bandpass_biquad(waveform: Tensor, sample_rate: int, central_freq: float, Q: float = 0.707,
                    const_skirt_gain: bool = False) -> Tensor:
    r"""reference: functional/filtering.py:104-142."""
    if not torch.jit.is_scripting():
        return _bandpass_biquad_eager(waveform, sample_rate, central_freq, Q, const_skirt_gain)
    return torch.ops.audio_amd.designed_biquad(waveform, "bandpass", sample_rate, [central_freq, Q], const_skirt_gain)


def bandreject_biquad(waveform: Tensor, sample_rate: int, central_freq: float, Q: float = 0.707) -> Tensor:
    r"""reference: functional/filtering.py:145-177."""
    if not torch.jit.is_scripting():
        return _bandreject_biquad_eager(waveform, sample_rate, central_freq, Q)
    return torch.ops.audio_amd.designed_biquad(waveform, "bandreject", sample_rate, [central_freq, Q], False)


def equalizer_biquad(waveform: Tensor, sample_rate: int, center_freq: float, gain: float, Q: float = 0.707) -> Tensor:
    r"""reference: functional/filtering.py:851-890."""
    if not torch.jit.is_scripting():
        return _equalizer_biquad_eager(waveform, sample_rate, center_freq, gain, Q)
    return torch.ops.audio_amd.designed_biquad(waveform, "equalizer", sample_rate, [center_freq, gain, Q], False)


def band_biquad(waveform: Tensor, sample_rate: int, central_freq: float, Q: float = 0.707, noise: bool = False) -> Tensor:
    r"""reference: functional/filtering.py:180-229."""
    if not torch.jit.is_scripting():
        return _band_biquad_eager(waveform, sample_rate, central_freq, Q, noise)
    return torch.ops.audio_amd.designed_biquad(waveform, "band", sample_rate, [central_freq, Q], noise)


def treble_biquad(waveform: Tensor, sample_rate: int, gain: float, central_freq: float = 3000., Q: float = 0.707) -> Tensor:
    r"""reference: functional/filtering.py:1363-1411 (high shelf)."""
    if not torch.jit.is_scripting():
        return _treble_biquad_eager(waveform, sample_rate, gain, central_freq, Q)
    return torch.ops.audio_amd.designed_biquad(waveform, "treble", sample_rate, [gain, central_freq, Q], False)


def bass_biquad(waveform: Tensor, sample_rate: int, gain: float, central_freq: float = 100., Q: float = 0.707) -> Tensor:
    r"""reference: functional/filtering.py:232-280 (low shelf)."""
    if not torch.jit.is_scripting():
        return _bass_biquad_eager(waveform, sample_rate, gain, central_freq, Q)
    return torch.ops.audio_amd.designed_biquad(waveform, "bass", sample_rate, [gain, central_freq, Q], False)


def deemph_biquad(waveform: Tensor, sample_rate: int) -> Tensor:
    r"""ISO 908 CD de-emphasis (reference: functional/filtering.py:417-462)."""
    if not torch.jit.is_scripting():
        return _deemph_biquad_eager(waveform, sample_rate)
    params: List[float] = []
    return torch.ops.audio_amd.designed_biquad(waveform, "deemph", sample_rate, params, False)


def riaa_biquad(waveform: Tensor, sample_rate: int) -> Tensor:
    r"""RIAA vinyl playback equalisation (reference: functional/filtering.py:1294-1360)."""
    if not torch.jit.is_scripting():
        return _riaa_biquad_eager(waveform, sample_rate)
    params: List[float] = []
    return torch.ops.audio_amd.designed_biquad(waveform, "riaa", sample_rate, params, False)


_DESIGNERS = {"lowpass": _lowpass_biquad_eager, "highpass": _highpass_biquad_eager, "allpass": _allpass_biquad_eager,
              "bandpass": _bandpass_biquad_eager, "bandreject": _bandreject_biquad_eager, "equalizer": _equalizer_biquad_eager,
              "band": _band_biquad_eager, "treble": _treble_biquad_eager, "bass": _bass_biquad_eager,
              "deemph": _deemph_biquad_eager, "riaa": _riaa_biquad_eager}
_DESIGNERS_WITH_FLAG = ("bandpass", "band")


def _designed_biquad(waveform: Tensor, kind: str, sample_rate: int, params, flag: bool) -> Tensor:
    """Kernel of `audio_amd::designed_biquad` (audio_amd/_ops.py)."""
    fn = _DESIGNERS[kind]
    if kind in _DESIGNERS_WITH_FLAG:
        return fn(waveform, sample_rate, *params, flag)
    return fn(waveform, sample_rate, *params)


def fftconvolve(x: Tensor, y: Tensor, mode: str = "full") -> Tensor:
    r"""Linear convolution along the last dim with broadcast leading dims and the reference's full / valid / same crops
    (reference: functional/functional.py:2222-2258); see ``_fftconvolve_eager``."""
    if not torch.jit.is_scripting():
        return _fftconvolve_eager(x, y, mode)
    return torch.ops.audio_amd.fftconvolve(x, y, mode)


def compute_deltas(specgram: Tensor, win_length: int = 5, mode: str = "replicate") -> Tensor:
    r"""Delta coefficients of a ``(..., freq, time)`` tensor (reference: F.compute_deltas); see ``_compute_deltas_eager``."""
    if not torch.jit.is_scripting():
        return _compute_deltas_eager(specgram, win_length, mode)
    return torch.ops.audio_amd.compute_deltas(specgram, win_length, mode)


def sliding_window_cmn(specgram: Tensor, cmn_window: int = 600, min_cmn_window: int = 100, center: bool = False,
                       norm_vars: bool = False) -> Tensor:
    r"""Sliding-window CMN of a ``(..., time, freq)`` tensor (reference: F.sliding_window_cmn); see
    ``_sliding_window_cmn_eager``."""
    if not torch.jit.is_scripting():
        return _sliding_window_cmn_eager(specgram, cmn_window, min_cmn_window, center, norm_vars)
    return torch.ops.audio_amd.sliding_window_cmn(specgram, cmn_window, min_cmn_window, center, norm_vars)


def detect_pitch_frequency(waveform: Tensor, sample_rate: int, frame_time: float = 10 ** (-2), win_length: int = 30,
                           freq_low: int = 85, freq_high: int = 3400) -> Tensor:
    r"""Pitch in Hz of a ``(..., time)`` waveform (reference: F.detect_pitch_frequency); see
    ``_detect_pitch_frequency_eager``."""
    if not torch.jit.is_scripting():
        if torch.compiler.is_compiling():
            return torch.ops.audio_amd.detect_pitch_frequency(waveform, sample_rate, frame_time, win_length, freq_low,
                                                              freq_high)
        return _detect_pitch_frequency_eager(waveform, sample_rate, frame_time, win_length, freq_low, freq_high)
    return torch.ops.audio_amd.detect_pitch_frequency(waveform, sample_rate, frame_time, win_length, freq_low, freq_high)


def mask_along_axis_iid(specgrams: Tensor, mask_param: int, mask_value: float, axis: int, p: float = 1.0) -> Tensor:
    r"""Per-example masks along ``axis`` of a ``(..., freq, time)`` tensor with at least three dimensions (reference:
    F.mask_along_axis_iid); see ``_mask_along_axis_iid_eager``.  The input itself is returned when the effective
    ``mask_param`` is below 1."""
    if not torch.jit.is_scripting():
        if not torch.compiler.is_compiling():
            return _mask_along_axis_iid_eager(specgrams, mask_param, mask_value, axis, p)
    if p >= 0.0 and p <= 1.0 and (axis == specgrams.dim() - 1 or axis == specgrams.dim() - 2) and specgrams.dim() >= 3:
        if _get_mask_param(mask_param, p, specgrams.size(axis)) < 1:
            return specgrams
    return torch.ops.audio_amd.mask_along_axis_iid(specgrams, mask_param, mask_value, axis, p)


def mask_along_axis(specgram: Tensor, mask_param: int, mask_value: float, axis: int, p: float = 1.0) -> Tensor:
    r"""One mask along ``axis`` of a ``(..., freq, time)`` tensor, shared by every example (reference: F.mask_along_axis);
    see ``_mask_along_axis_eager``.  The input itself is returned when the effective ``mask_param`` is below 1."""
    if not torch.jit.is_scripting():
        if not torch.compiler.is_compiling():
            return _mask_along_axis_eager(specgram, mask_param, mask_value, axis, p)
    if p >= 0.0 and p <= 1.0 and (axis == specgram.dim() - 1 or axis == specgram.dim() - 2) and specgram.dim() >= 2:
        if _get_mask_param(mask_param, p, specgram.size(axis)) < 1:
            return specgram
    return torch.ops.audio_amd.mask_along_axis(specgram, mask_param, mask_value, axis, p)


def add_noise(waveform: Tensor, noise: Tensor, snr: Tensor, lengths: Optional[Tensor] = None) -> Tensor:
    r"""Scale ``noise`` to the signal-to-noise ratio ``snr`` (dB) per row and add it to ``waveform`` (reference:
    F.add_noise); see ``_add_noise_eager``."""
    if not torch.jit.is_scripting():
        if not torch.compiler.is_compiling():
            return _add_noise_eager(waveform, noise, snr, lengths)
    return torch.ops.audio_amd.add_noise(waveform, noise, snr, lengths)


def preemphasis(waveform: Tensor, coeff: float = 0.97) -> Tensor:
    r"""Pre-emphasis along the last dim (reference: F.preemphasis); see ``_preemphasis_eager``."""
    if not torch.jit.is_scripting():
        if not torch.compiler.is_compiling():
            return _preemphasis_eager(waveform, coeff)
    return torch.ops.audio_amd.preemphasis(waveform, coeff)


def deemphasis(waveform: Tensor, coeff: float = 0.97) -> Tensor:
    r"""De-emphasis along the last dim (reference: F.deemphasis); see ``_deemphasis_eager``."""
    if not torch.jit.is_scripting():
        if not torch.compiler.is_compiling():
            return _deemphasis_eager(waveform, coeff)
    return torch.ops.audio_amd.deemphasis(waveform, coeff)


def convolve(x: Tensor, y: Tensor, mode: str = "full") -> Tensor:
    r"""Linear convolution along the last dim (reference: F.convolve); see ``_convolve_eager``."""
    if not torch.jit.is_scripting():
        if not torch.compiler.is_compiling():
            return _convolve_eager(x, y, mode)
    return torch.ops.audio_amd.convolve(x, y, mode)


def psd(specgram: Tensor, mask: Optional[Tensor] = None, normalize: bool = True, eps: float = 1e-10) -> Tensor:
    r"""Power spectral density matrix of ``(..., ch, freq, time)`` (reference: F.psd); see ``_psd_eager``."""
    if not torch.jit.is_scripting():
        if not torch.compiler.is_compiling():
            return _psd_eager(specgram, mask, normalize, eps)
    return torch.ops.audio_amd.psd(specgram, mask, normalize, eps)


def _psd_pair(specgram: Tensor, mask_s: Tensor, mask_n: Tensor, normalize: bool = True, eps: float = 1e-10) -> Tensor:
    if not torch.jit.is_scripting():
        if not torch.compiler.is_compiling():
            return _psd_pair_eager(specgram, mask_s, mask_n, normalize, eps)
    return torch.ops.audio_amd.psd_pair(specgram, mask_s, mask_n, normalize, eps)


def mvdr_weights_souden(psd_s: Tensor, psd_n: Tensor, reference_channel: Union[int, Tensor], diagonal_loading: bool = True,
                        diag_eps: float = 1e-7, eps: float = 1e-8) -> Tensor:
    r"""MVDR weights by Souden's method (reference: F.mvdr_weights_souden); see ``_mvdr_weights_souden_eager``."""
    if not torch.jit.is_scripting():
        if not torch.compiler.is_compiling():
            return _mvdr_weights_souden_eager(psd_s, psd_n, reference_channel, diagonal_loading, diag_eps, eps)
    if isinstance(reference_channel, int):
        return torch.ops.audio_amd.mvdr_weights_souden(psd_s, psd_n, reference_channel, None, diagonal_loading, diag_eps, eps)
    else:
        return torch.ops.audio_amd.mvdr_weights_souden(psd_s, psd_n, -1, reference_channel, diagonal_loading, diag_eps, eps)


def mvdr_weights_rtf(rtf: Tensor, psd_n: Tensor, reference_channel: Optional[Union[int, Tensor]] = None,
                     diagonal_loading: bool = True, diag_eps: float = 1e-7, eps: float = 1e-8) -> Tensor:
    r"""MVDR weights from a relative transfer function (reference: F.mvdr_weights_rtf); see ``_mvdr_weights_rtf_eager``."""
    if not torch.jit.is_scripting():
        if not torch.compiler.is_compiling():
            return _mvdr_weights_rtf_eager(rtf, psd_n, reference_channel, diagonal_loading, diag_eps, eps)
    if reference_channel is None:
        return torch.ops.audio_amd.mvdr_weights_rtf(rtf, psd_n, None, None, diagonal_loading, diag_eps, eps)
    elif isinstance(reference_channel, int):
        return torch.ops.audio_amd.mvdr_weights_rtf(rtf, psd_n, reference_channel, None, diagonal_loading, diag_eps, eps)
    else:
        return torch.ops.audio_amd.mvdr_weights_rtf(rtf, psd_n, None, reference_channel, diagonal_loading, diag_eps, eps)


def rtf_power(psd_s: Tensor, psd_n: Tensor, reference_channel: Union[int, Tensor], n_iter: int = 3,
              diagonal_loading: bool = True, diag_eps: float = 1e-7) -> Tensor:
    r"""Relative transfer function by the power method (reference: F.rtf_power); see ``_rtf_power_eager``."""
    if not torch.jit.is_scripting():
        if not torch.compiler.is_compiling():
            return _rtf_power_eager(psd_s, psd_n, reference_channel, n_iter, diagonal_loading, diag_eps)
    if isinstance(reference_channel, int):
        return torch.ops.audio_amd.rtf_power(psd_s, psd_n, reference_channel, None, n_iter, diagonal_loading, diag_eps)
    else:
        return torch.ops.audio_amd.rtf_power(psd_s, psd_n, -1, reference_channel, n_iter, diagonal_loading, diag_eps)


def apply_beamforming(beamform_weights: Tensor, specgram: Tensor) -> Tensor:
    r"""Apply beamforming weights to a multi-channel spectrogram (reference: F.apply_beamforming); see
    ``_apply_beamforming_eager``."""
    if not torch.jit.is_scripting():
        if not torch.compiler.is_compiling():
            return _apply_beamforming_eager(beamform_weights, specgram)
    return torch.ops.audio_amd.apply_beamforming(beamform_weights, specgram)


def rnnt_loss(logits: Tensor, targets: Tensor, logit_lengths: Tensor, target_lengths: Tensor, blank: int = -1,
              clamp: float = -1.0, reduction: str = "mean", fused_log_softmax: bool = True) -> Tensor:
    r"""RNN transducer loss (reference: F.rnnt_loss); see ``_rnnt_loss_eager``."""
    if not torch.jit.is_scripting():
        if not torch.compiler.is_compiling():
            return _rnnt_loss_eager(logits, targets, logit_lengths, target_lengths, blank, clamp, reduction, fused_log_softmax)
    return torch.ops.audio_amd.rnnt_loss(logits, targets, logit_lengths, target_lengths, blank, clamp, reduction,
                                         fused_log_softmax)
