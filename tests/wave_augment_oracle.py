"""float64 numpy oracle of the waveform augmentation ops (F.add_noise, F.preemphasis, F.convolve), each written twice,
independently: a vectorised expression of the reference's definition and a plain loop.  No torch arithmetic, no GPU."""
import math

import numpy as np


def _lead(*shapes):
    return np.broadcast_shapes(*shapes)


# ---- add_noise -----------------------------------------------------------------------------------------------------------

def add_noise_scale(waveform, noise, snr, lengths=None):
    """The reference's formula as written, float64; log10(0) = -inf is left to IEEE arithmetic."""
    w, n = np.asarray(waveform, np.float64), np.asarray(noise, np.float64)
    snr = np.asarray(snr, np.float64)
    L = w.shape[-1]
    if lengths is not None:
        mask = np.arange(L) < np.asarray(lengths)[..., None]
        mw, mn = w * mask, n * mask
    else:
        mw, mn = w, n
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        es = np.sum(mw * mw, axis=-1)
        en = np.sum(mn * mn, axis=-1)
        original_snr_db = 10 * (np.log10(es) - np.log10(en))
        return 10 ** ((original_snr_db - snr) / 20.0)


def add_noise(waveform, noise, snr, lengths=None):
    w, n = np.asarray(waveform, np.float64), np.asarray(noise, np.float64)
    scale = add_noise_scale(w, n, snr, lengths)
    with np.errstate(invalid="ignore", over="ignore"):
        return w + scale[..., None] * n


def add_noise_loop(waveform, noise, snr, lengths=None):
    """Row by row with math.fsum energies (exactly rounded sums)."""
    w, n = np.asarray(waveform, np.float64), np.asarray(noise, np.float64)
    snr = np.asarray(snr, np.float64)
    L = w.shape[-1]
    lead = _lead(w.shape[:-1], n.shape[:-1], snr.shape, () if lengths is None else np.shape(lengths))
    wb, nb = np.broadcast_to(w, lead + (L,)), np.broadcast_to(n, lead + (L,))
    sb = np.broadcast_to(snr, lead)
    lb = None if lengths is None else np.broadcast_to(np.asarray(lengths), lead)
    out = np.empty(lead + (L,), np.float64)
    scales = np.empty(lead, np.float64)
    for idx in np.ndindex(*lead):
        ln = L if lb is None else lb[idx]
        es = math.fsum(float(wb[idx][i]) ** 2 for i in range(L) if i < ln)
        en = math.fsum(float(nb[idx][i]) ** 2 for i in range(L) if i < ln)
        le = math.log10(es) if es > 0 else -math.inf
        ln_ = math.log10(en) if en > 0 else -math.inf
        if le == -math.inf and ln_ == -math.inf:
            scale = math.nan
        else:
            x = (10 * (le - ln_) - float(sb[idx])) / 20.0
            scale = math.inf if x == math.inf else (0.0 if x == -math.inf else 10.0 ** x)
        scales[idx] = scale
        for i in range(L):
            ni = float(nb[idx][i])
            p = math.nan if (math.isinf(scale) and ni == 0.0) or math.isnan(scale) else scale * ni
            out[idx][i] = float(wb[idx][i]) + p
    return out, scales


def achieved_snr_db(waveform, mixed, lengths=None):
    """SNR of (mixed - waveform) against waveform over the samples below `lengths`, dB."""
    w, o = np.asarray(waveform, np.float64), np.asarray(mixed, np.float64)
    L = w.shape[-1]
    mask = np.ones(o.shape, bool) if lengths is None else np.broadcast_to(np.arange(L) < np.asarray(lengths)[..., None], o.shape)
    wb = np.broadcast_to(w, o.shape)
    es = np.sum((wb * mask) ** 2, axis=-1)
    en = np.sum(((o - wb) * mask) ** 2, axis=-1)
    return 10 * np.log10(es / en)


# ---- preemphasis ---------------------------------------------------------------------------------------------------------

def preemphasis(x, coeff=0.97, dtype=np.float64):
    """The reference's expression evaluated in `dtype`: coeff rounded to it, product and difference rounded separately."""
    x = np.asarray(x, dtype)
    c = dtype(coeff)
    y = x.copy()
    y[..., 1:] = x[..., 1:] - (c * x[..., :-1]).astype(dtype)
    return y


def preemphasis_loop(x, coeff=0.97, dtype=np.float64):
    x = np.asarray(x, dtype)
    c = dtype(coeff)
    y = np.empty_like(x)
    flat_x, flat_y = x.reshape(-1, x.shape[-1]), y.reshape(-1, x.shape[-1])
    for r in range(flat_x.shape[0]):
        for i in range(flat_x.shape[1]):
            if i == 0:
                flat_y[r, i] = flat_x[r, i]
            else:
                p = dtype(c * flat_x[r, i - 1])
                flat_y[r, i] = dtype(flat_x[r, i] - p)
    return y


def preemphasis_transposed(g, coeff=0.97, dtype=np.float64):
    """The adjoint: y[i] = g[i] - c g[i + 1], y[L - 1] = g[L - 1]."""
    g = np.asarray(g, dtype)
    c = dtype(coeff)
    y = g.copy()
    y[..., :-1] = g[..., :-1] - (c * g[..., 1:]).astype(dtype)
    return y


# ---- convolve ------------------------------------------------------------------------------------------------------------

def convolve(x, y, mode="full"):
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    nx, ny = x.shape[-1], y.shape[-1]
    lead = _lead(x.shape[:-1], y.shape[:-1])
    xb, yb = np.broadcast_to(x, lead + (nx,)), np.broadcast_to(y, lead + (ny,))
    full = np.empty(lead + (nx + ny - 1,), np.float64)
    for idx in np.ndindex(*lead):
        full[idx] = np.convolve(xb[idx], yb[idx])
    if mode == "full":
        return full
    n = max(nx, ny) - min(nx, ny) + 1 if mode == "valid" else nx
    start = (full.shape[-1] - n) // 2
    return full[..., start:start + n]
