"""The contract of LFCC's filterbank, the spectral centroid and the pointwise waveform ops (gain / Vol, contrast,
DB_to_amplitude, mu-law, Fade), restated in numpy from the reference's source: float64 definitions, the same expressions in
a chosen precision (the yardstick of the accuracy bars), and the bars themselves.  torchaudio is not needed."""
import math

import numpy as np
import torch

SHAPES = ("linear", "exponential", "logarithmic", "quarter_sine", "half_sine")


# ---- linear filterbank -------------------------------------------------------------------------------------------------------
def linear_fbanks(n_freqs, f_min, f_max, n_filter, sample_rate):
    """The definition: float32 torch CPU ops in the reference's order."""
    all_freqs = torch.linspace(0, sample_rate // 2, n_freqs)
    f_pts = torch.linspace(f_min, f_max, n_filter + 2)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts.unsqueeze(0) - all_freqs.unsqueeze(1)
    down = (-1.0 * slopes[:, :-2]) / f_diff[:-1]
    up = slopes[:, 2:] / f_diff[1:]
    return torch.max(torch.zeros(1), torch.min(down, up))


# ---- spectral centroid -------------------------------------------------------------------------------------------------------
def centroid_freqs(sample_rate, n_fft):
    return torch.linspace(0, sample_rate // 2, 1 + n_fft // 2).numpy()


def centroid(mag, freqs):
    """(..., frames, n_freq) float32 magnitudes, [n_freq] float32 frequencies -> float64 (..., frames): float64 sums of the
    same float32 values."""
    m = np.asarray(mag, dtype=np.float64)
    f = np.asarray(freqs, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (m * f).sum(-1) / m.sum(-1)


def ulp32(v):
    """The spacing of float32 at |v| (float64 array in, float64 out)."""
    a = np.abs(np.asarray(v, dtype=np.float64)).astype(np.float32)
    return (np.nextafter(a, np.float32(np.inf)) - a).astype(np.float64)


# ---- pointwise ops: the reference's expressions in precision `dt` (np.float32 / np.float64 / np.longdouble) -------------------
def ratio_of_db(gain_db):
    return 10 ** (gain_db / 20)


def scale(x, ratio, clamp, dt):
    y = x.astype(dt) * dt(ratio)
    return np.clip(y, dt(-1), dt(1)) if clamp else y


def contrast(x, amount, dt):
    x = x.astype(dt)
    t = x * dt(math.pi / 2)
    return np.sin(t + dt(amount / 750.0) * np.sin(t * dt(4)))


def db_to_amplitude(x, ref, power, dt):
    x = x.astype(dt)
    return dt(ref) * np.power(np.power(dt(10), dt(0.1) * x), dt(power))


def mu_encode_value(x, q, dt):
    """The value the reference truncates to the code."""
    x = x.astype(dt)
    mu = dt(q - 1.0)
    v = np.sign(x) * np.log1p(mu * np.abs(x)) / np.log1p(mu)
    return (v + dt(1)) / dt(2) * mu + dt(0.5)


def mu_encode(x, q, dt):
    return np.trunc(mu_encode_value(x, q, dt)).astype(np.int64)


def mu_decode(codes, q, dt):
    mu = dt(q - 1.0)
    y = np.asarray(codes).astype(dt) / mu * dt(2) - dt(1)
    return np.sign(y) * (np.exp(np.abs(y) * np.log1p(mu)) - dt(1)) / mu


def mu_band(q):
    """+-1 is allowed where the float64 value before truncation lies this close to an integer."""
    return 8 * 2.0 ** -24 * q


def fade_ramps(n_in, n_out, shape):
    """float64 ramps, clamped to [0, 1]."""
    fi, fo = np.linspace(0.0, 1.0, n_in), np.linspace(0.0, 1.0, n_out)
    if shape == "linear":
        fo = 1.0 - fo
    elif shape == "exponential":
        fi, fo = 2.0 ** (fi - 1.0) * fi, 2.0 ** (-fo) * (1.0 - fo)
    elif shape == "logarithmic":
        fi, fo = np.log10(0.1 + fi) + 1.0, np.log10(1.1 - fo) + 1.0
    elif shape == "quarter_sine":
        fi, fo = np.sin(fi * math.pi / 2), np.sin(fo * math.pi / 2 + math.pi / 2)
    elif shape == "half_sine":
        fi, fo = np.sin(fi * math.pi - math.pi / 2) / 2 + 0.5, np.sin(fo * math.pi + math.pi / 2) / 2 + 0.5
    else:
        raise ValueError(shape)
    return np.clip(fi, 0.0, 1.0), np.clip(fo, 0.0, 1.0)


# ---- number formats ------------------------------------------------------------------------------------------------------------
def round_bf16(a):
    """float64 -> the nearest bfloat16 (ties to even), as float64: the two neighbours are compared in float64, where the
    differences are exact (finite values well inside float32's range)."""
    a = np.asarray(a, dtype=np.float64)
    plain = np.isfinite(a) & (a != 0)
    if not plain.all():                   # zeros (with their sign), infinities and NaN are bfloat16 values already
        out = a.copy()
        out[plain] = round_bf16(a[plain])
        return out
    lo_bits = a.astype(np.float32).view(np.uint32) & np.uint32(0xFFFF0000)
    cands = []
    for d in (-1, 0, 1, 2):               # the truncated float32 RNE value and its bfloat16 neighbours bracket a
        cands.append((lo_bits.astype(np.int64) + d * 0x10000).astype(np.uint32).view(np.float32).astype(np.float64))
    c = np.stack(cands)
    c[:, a == 0] = 0.0
    err = np.abs(c - a)
    best = err.min(axis=0)
    out = np.full(a.shape, np.nan)
    for k in range(4):
        even = ((lo_bits.astype(np.int64) + (k - 1) * 0x10000) >> 16) & 1 == 0
        take = (err[k] == best) & (np.isnan(out) | even)
        out = np.where(take, c[k], out)
    return out


def round_to(a, dtype):
    """float64 -> torch CPU tensor of `dtype`, rounded once."""
    a = np.asarray(a, dtype=np.float64)
    if dtype == torch.float64:
        return torch.from_numpy(a.copy())
    if dtype == torch.float32:
        return torch.from_numpy(a.astype(np.float32))
    if dtype == torch.float16:
        return torch.from_numpy(a.astype(np.float16))
    return torch.from_numpy(round_bf16(a).astype(np.float32)).to(torch.bfloat16)      # exact: the values are bfloat16 already


def half_ulp(ref, dtype):
    """Half a unit in the last place of `dtype` at |ref| (float64 out): the one rounding of a float16 / bfloat16 result."""
    ref = np.abs(np.asarray(ref, dtype=np.float64))
    if dtype == torch.float16:
        return np.maximum(ref * 2.0 ** -11, 2.0 ** -25)
    if dtype == torch.bfloat16:
        return ref * 2.0 ** -8
    return np.zeros_like(ref)
