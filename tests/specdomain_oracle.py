"""Plain references for the stand-alone spectrogram-domain ops: amplitude_to_DB, MelScale, phase_vocoder, GriffinLim and the
MFCC tail.  TEST INFRASTRUCTURE: CPU, torch only, nothing from audio_amd.  Each function is the reference's formula
(functional/functional.py:255-404, 732-803; transforms/_transforms.py:403-415, 692-709) written out in the dtype asked for --
float64 is the truth the device tests compare with, float32 is the reference as a user runs it (pinned on the reference's stored
outputs by tests/test_specdomain_oracle.py) and the yardstick for what float32 can deliver at all.

`bite=` evaluates a deliberately WRONG variant -- the way a kernel would plausibly be wrong -- so that
tests/test_gpu_fuzz_specdomain.py can show, without a device, that its inputs and bars would notice it."""
import math
from typing import Optional

import torch


def _real(dtype):
    return {torch.complex64: torch.float32, torch.complex128: torch.float64}.get(dtype, dtype)


def _cplx(dtype):
    return torch.complex128 if _real(dtype) == torch.float64 else torch.complex64


def amplitude_to_db(x, multiplier, amin, db_multiplier, top_db, dtype=torch.float64, nan_poisons_group=True, bite=None):
    """functional.py:390-402.  One cut-off per leading item of the (-1, C, F, T) view, C = shape[-3] if x.dim() > 2 else 1.
    `nan_poisons_group=False`: the cut-off is the maximum over the group's non-NaN elements (the product's contract for a
    NaN element, README "Contract"); True is the reference, where amax() returns NaN for the whole group.
    bite: "group_size" cuts the flat tensor into groups one element too long; "neighbour_cut" takes group g + 1's cut-off."""
    x = x.to(dtype)
    x_db = multiplier * torch.log10(torch.clamp(x, min=amin))
    x_db = x_db - multiplier * db_multiplier
    if top_db is None:
        return x_db
    shape = x_db.size()
    packed = shape[-3] if x_db.dim() > 2 else 1
    g = x_db.reshape(-1, packed * shape[-2] * shape[-1])
    n_groups, size = g.shape
    src = g if nan_poisons_group else torch.where(torch.isnan(g), torch.full_like(g, -math.inf), g)
    if bite == "group_size":
        flat, fsrc = g.reshape(-1), src.reshape(-1)
        idx = torch.arange(flat.numel()) // (size + 1)
        gmax = torch.full((int(idx.max()) + 1,), -math.inf, dtype=dtype).scatter_reduce(0, idx, fsrc, "amax")
        return torch.max(flat, gmax[idx] - top_db).reshape(shape)
    gmax = src.amax(dim=-1)
    if bite == "neighbour_cut":
        gmax = gmax.roll(-1)
    elif bite is not None:
        raise ValueError(bite)
    return torch.max(g, (gmax - top_db).view(-1, 1)).reshape(shape)


def mel_scale(spec, fb, dtype=torch.float64, bite=None):
    """_transforms.py:413: (..., freq, time) x (freq, n_mels) -> (..., n_mels, time).
    bite: "band_start" applies one band (the middle one that is not empty) one bin too high."""
    fb = fb.to(dtype)
    if bite == "band_start":
        fb = fb.clone()
        live = [m for m in range(fb.shape[1]) if bool((fb[:, m] != 0).any())]
        m = live[len(live) // 2]
        col = fb[:, m].roll(1)
        col[0] = 0.0
        fb[:, m] = col
    elif bite is not None:
        raise ValueError(bite)
    return torch.matmul(spec.to(dtype).transpose(-1, -2), fb).transpose(-1, -2)


def phase_vocoder(spec, rate, phase_advance, bite=None):
    """functional.py:732-803 in the dtype of `spec`.  The time steps are ALWAYS torch.arange(..., dtype=float32), cast up: a
    float64 arange picks other frames and other alphas than the float32 op does (golden pv_slow), and the float64 run is the
    truth for that op.
    bite: "no_pad" reads frame i0 + 1 == n_in as the last frame instead of the zero pad; "floor_wrap" wraps with floor instead
    of round-half-even; "no_readd" forgets to add phase_advance back after the wrap; "drop_first" drops angle(spec[..., 0]),
    the first term of the running sum."""
    if rate == 1.0:
        return spec
    real = _real(spec.dtype)
    n_in = spec.size(-1)
    pa = phase_advance.to(real).reshape(-1, 1)
    time_steps = torch.arange(0, n_in, rate, dtype=torch.float32).to(real)
    alphas = time_steps % 1.0
    phase_0 = spec[..., :1].angle()
    i0 = time_steps.long()
    i1 = (time_steps + 1).long()
    if bite == "no_pad":
        i1 = i1.clamp(max=n_in - 1)
    padded = torch.nn.functional.pad(spec, [0, 2])
    s0 = padded.index_select(-1, i0)
    s1 = padded.index_select(-1, i1)
    angle_0, angle_1 = s0.angle(), s1.angle()
    norm_0, norm_1 = s0.abs(), s1.abs()
    phase = angle_1 - angle_0 - pa
    if bite == "floor_wrap":
        phase = phase - 2 * math.pi * torch.floor(phase / (2 * math.pi))
    else:
        phase = phase - 2 * math.pi * torch.round(phase / (2 * math.pi))
    if bite != "no_readd":
        phase = phase + pa
    if bite == "drop_first":
        phase_0 = torch.zeros_like(phase_0)
    if bite not in (None, "no_pad", "floor_wrap", "no_readd", "drop_first"):
        raise ValueError(bite)
    phase = torch.cat([phase_0, phase[..., :-1]], dim=-1)
    phase_acc = torch.cumsum(phase, -1)
    mag = alphas * norm_1 + (1 - alphas) * norm_0
    return torch.polar(mag, phase_acc)


def griffinlim(specgram, window, n_fft, hop_length, win_length, power, n_iter, momentum, length, dtype=torch.float64,
               bite=None):
    """functional.py:255-353 with rand_init=False, over torch.stft / torch.istft in `dtype`.
    bite: "raw_momentum" leaves the momentum unscaled by 1 / (1 + momentum)."""
    if not 0 <= momentum < 1:
        raise ValueError("momentum must be in range [0, 1). Found: {}".format(momentum))
    if bite == "raw_momentum":
        pass
    elif bite is None:
        momentum = momentum / (1 + momentum)
    else:
        raise ValueError(bite)
    window = window.to(dtype)
    shape = specgram.size()
    mag = specgram.to(dtype).reshape([-1] + list(shape[-2:])).pow(1 / power)
    angles = torch.full(mag.size(), 1, dtype=_cplx(dtype))
    tprev = torch.tensor(0.0, dtype=dtype)
    for _ in range(n_iter):
        inverse = torch.istft(angles * mag, n_fft=n_fft, hop_length=hop_length, win_length=win_length, window=window,
                              length=length)
        rebuilt = torch.stft(inverse, n_fft=n_fft, hop_length=hop_length, win_length=win_length, window=window, center=True,
                             pad_mode="reflect", normalized=False, onesided=True, return_complex=True)
        angles = rebuilt
        if momentum:
            angles = angles - tprev * momentum
        angles = angles / (angles.abs() + 1e-16)
        tprev = rebuilt
    waveform = torch.istft(angles * mag, n_fft=n_fft, hop_length=hop_length, win_length=win_length, window=window, length=length)
    return waveform.reshape(shape[:-2] + waveform.shape[-1:])


def mfcc_tail(mel, dct, log_mels, top_db: Optional[float] = 80.0):
    """_transforms.py:703-709: (..., n_mels, time) mel energies -> (..., n_mfcc, time), in the dtype of `mel`."""
    if log_mels:
        y = torch.log(mel + 1e-6)
    else:
        y = amplitude_to_db(mel, 10.0, 1e-10, 0.0, top_db, dtype=mel.dtype)
    return torch.matmul(y.transpose(-1, -2), dct.to(mel.dtype)).transpose(-1, -2)
