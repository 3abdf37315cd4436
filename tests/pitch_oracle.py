"""Float64 oracle of F.detect_pitch_frequency (torchaudio functional.py: _compute_nccf, _find_max_per_frame, _combine_max,
_median_smoothing, detect_pitch_frequency), in two independent forms of the NCCF, plus a torch restatement of the
reference that runs on CPU.

    nccf_loops   a loop over lags and frames, every sum taken directly;
    nccf_prefix  vectorised: numerators from a strided view, window energies from float64 prefix sums.
    pick         both first-index max reductions and the 0.99 combine (in the NCCF's own dtype), -> 1-based lags
    smooth       the left-replicated lower median over win_length frames, then float32 reciprocal * sample_rate
    torch_reference  the reference restated in torch (any device; CPU here)
"""
import math

import numpy as np
import torch

EPS = 10 ** (-9)


def sizes(length, sample_rate, frame_time=1e-2, win_length=30, freq_low=85, freq_high=3400):
    """The host's size arithmetic, with exactly the reference's Python expressions."""
    lags = int(math.ceil(sample_rate / freq_low))
    fs = int(math.ceil(sample_rate * frame_time))
    F = int(math.ceil(length / fs))
    lag_min = int(math.ceil(sample_rate / freq_high))
    p = (win_length - 1) // 2
    return dict(lags=lags, fs=fs, F=F, lag_min=lag_min, p=p, n_out=F + p - win_length + 1)


def _padded(x, fs, lags):
    x = np.asarray(x, dtype=np.float64)
    L = x.shape[-1]
    F = int(math.ceil(L / fs))
    return np.concatenate([x, np.zeros(x.shape[:-1] + (lags + F * fs - L,))], -1), F


def nccf_loops(x, fs, lags):
    """x (rows, L) -> (rows, F, lags), direct sums."""
    xp, F = _padded(x, fs, lags)
    out = np.zeros((xp.shape[0], F, lags))
    for r in range(xp.shape[0]):
        for k in range(F):
            s1 = xp[r, k * fs:k * fs + fs]
            n1 = (EPS + math.sqrt(float(np.dot(s1, s1)))) ** 2
            for lag in range(1, lags + 1):
                s2 = xp[r, k * fs + lag:k * fs + lag + fs]
                out[r, k, lag - 1] = float(np.dot(s1, s2)) / n1 / (EPS + math.sqrt(float(np.dot(s2, s2)))) ** 2
    return out


def nccf_prefix(x, fs, lags):
    """x (rows, L) -> (rows, F, lags), vectorised (energies from prefix sums of squares)."""
    xp, F = _padded(x, fs, lags)
    rows = xp.shape[0]
    # prefix sums of squares local to each frame's segment x[k fs, k fs + fs + lags): the cancellation in a difference is
    # relative to that segment's energy, not to the energy of the whole row before it
    seg = np.lib.stride_tricks.sliding_window_view(xp, fs + lags, -1)[:, ::fs][:, :F]          # (rows, F, fs + lags)
    c = np.concatenate([np.zeros((rows, F, 1)), np.cumsum(seg * seg, -1)], -1)
    e = np.maximum(c[..., fs:] - c[..., :lags + 1], 0.0)                                       # (rows, F, lags + 1)
    d = (EPS + np.sqrt(e)) ** 2
    starts = np.arange(F)[:, None] * fs + np.arange(lags + 1)[None, :]           # (F, lags + 1): lag 0 = s1
    win = np.lib.stride_tricks.sliding_window_view(xp, fs, -1)                  # (rows, positions, fs)
    s1 = win[:, starts[:, 0]]                                                    # (rows, F, fs)
    num = np.einsum("rkf,rklf->rkl", s1, win[:, starts[:, 1:]])
    return num / d[:, :, :1] / d[:, :, 1:]


def _first_max(v):
    """torch.max(v, -1): NaN first, ties to the first index."""
    nan = np.isnan(v)
    idx = np.where(nan.any(-1), nan.argmax(-1), np.argmax(np.where(nan, -np.inf, v), -1))
    return np.take_along_axis(v, idx[..., None], -1)[..., 0], idx


def pick(nccf, lag_min):
    """(.., F, lags) -> int64 (.., F) 1-based lags; the 0.99 threshold is rounded to the NCCF's dtype."""
    lags = nccf.shape[-1]
    if lag_min >= lags or lags // 2 <= lag_min:
        raise IndexError("empty max slice")
    bv, bi = _first_max(nccf[..., lag_min:])
    hv, hi = _first_max(nccf[..., lag_min:lags // 2])
    thresh = nccf.dtype.type(0.99)
    mask = hv > thresh * bv
    return np.where(mask, hi, bi).astype(np.int64) + lag_min + 1


def smooth(lag, win_length, sample_rate):
    """int (.., F) lags -> float32 (.., n_out) Hz."""
    lag = np.asarray(lag, dtype=np.int64)
    p = (win_length - 1) // 2
    padded = np.concatenate([np.repeat(lag[..., :1], p, -1), lag], -1)
    roll = np.lib.stride_tricks.sliding_window_view(padded, win_length, -1)
    med = np.sort(roll, -1)[..., (win_length - 1) // 2]
    r = np.float32(1.0) / (np.float32(EPS) + med.astype(np.float32))
    return (r * np.float32(sample_rate)).astype(np.float32)


def detect(x, sample_rate, frame_time=1e-2, win_length=30, freq_low=85, freq_high=3400, form="prefix"):
    """End to end from the float64 NCCF: (.., L) -> float32 (.., n_out)."""
    x = np.asarray(x, dtype=np.float64)
    s = sizes(x.shape[-1], sample_rate, frame_time, win_length, freq_low, freq_high)
    f = nccf_prefix if form == "prefix" else nccf_loops
    nccf = f(x.reshape(-1, x.shape[-1]), s["fs"], s["lags"])
    out = smooth(pick(nccf, s["lag_min"]), win_length, sample_rate)
    return out.reshape(x.shape[:-1] + out.shape[-1:])


def torch_reference(waveform, sample_rate, frame_time=1e-2, win_length=30, freq_low=85, freq_high=3400):
    """The reference restated in torch, statement for statement (runs on any device)."""
    shape = list(waveform.size())
    waveform = waveform.reshape([-1] + shape[-1:])
    lags = int(math.ceil(sample_rate / freq_low))
    frame_size = int(math.ceil(sample_rate * frame_time))
    waveform_length = waveform.size()[-1]
    num_of_frames = int(math.ceil(waveform_length / frame_size))
    p = lags + num_of_frames * frame_size - waveform_length
    waveform = torch.nn.functional.pad(waveform, (0, p))
    output_lag = []
    for lag in range(1, lags + 1):
        s1 = waveform[..., :-lag].unfold(-1, frame_size, frame_size)[..., :num_of_frames, :]
        s2 = waveform[..., lag:].unfold(-1, frame_size, frame_size)[..., :num_of_frames, :]
        output_frames = ((s1 * s2).sum(-1) / (EPS + torch.linalg.vector_norm(s1, ord=2, dim=-1)).pow(2)
                         / (EPS + torch.linalg.vector_norm(s2, ord=2, dim=-1)).pow(2))
        output_lag.append(output_frames.unsqueeze(-1))
    nccf = torch.cat(output_lag, -1)
    lag_min = int(math.ceil(sample_rate / freq_high))
    best = torch.max(nccf[..., lag_min:], -1)
    half_size = nccf.shape[-1] // 2
    half = torch.max(nccf[..., lag_min:half_size], -1)
    mask = half[0] > 0.99 * best[0]
    indices = mask * half[1] + ~mask * best[1]
    indices = indices + lag_min + 1
    pad_length = (win_length - 1) // 2
    indices = torch.nn.functional.pad(indices, (pad_length, 0), mode="constant", value=0.0)
    indices[..., :pad_length] = torch.cat(pad_length * [indices[..., pad_length].unsqueeze(-1)], dim=-1)
    roll = indices.unfold(-1, win_length, 1)
    values, _ = torch.median(roll, -1)
    freq = sample_rate / (EPS + values.to(torch.float))
    return freq.reshape(shape[:-1] + list(freq.shape[-1:]))


def tone(n, sample_rate, f0, harmonics=(1.0, 0.5, 0.25), noise=0.01, seed=0, glide=None):
    """A harmonic tone with noise; glide = (f_start, f_end) sweeps f0 linearly."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / sample_rate
    if glide is None:
        phase = 2 * np.pi * f0 * t
    else:
        f = np.linspace(glide[0], glide[1], n)
        phase = 2 * np.pi * np.cumsum(f) / sample_rate
    x = sum(a * np.sin((h + 1) * phase) for h, a in enumerate(harmonics))
    return (x + noise * rng.standard_normal(n)).astype(np.float32)
