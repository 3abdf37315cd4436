"""The definition of the first-order gradients of oscillator_bank and filter_waveform (audio_amd/csrc/dsp_synth_grad.h) in numpy:
the four adjoints of tests/dsp_oracle.py's two forwards, in float64, or longdouble where `acc` says so, with the magnitudes the
bars of tests/dsp_grad_cases.py need.  Never imported by the product.  w and a' are the definition's (dsp_oracle.osc_increment,
osc_amplitudes): `remainder` has derivative 1, and a dead step (|f| >= sample_rate / 2) contributes nothing to the frequency
gradient but still receives from the live steps after it."""
import numpy as np

import dsp_oracle as O

LD = O.LD


def oscillator_bank_grad(f, a, g, sample_rate, reduction="sum", acc=np.float64):
    """f, a (..., T, N) float32 or float64; g (..., T), or (..., T, N) for "none".  Returns (gf, ga, |g| as it reaches every
    oscillator, M): gf = (2 pi / sample_rate) sum_{s >= t} g a' cos(phi), ga = g sin(phi) (0 where dead), M (..., 1, N) =
    (2 pi / sample_rate) sum_{all s} |g a'|.  For "mean" g is divided by N first."""
    N = f.shape[-1]
    w = O.osc_increment(f, sample_rate).astype(acc)
    ap = O.osc_amplitudes(f, a, sample_rate).astype(acc)
    dead = np.abs(f) >= f.dtype.type(sample_rate / 2.0)
    ge = g.astype(acc)
    if reduction != "none":
        ge = ge[..., None]
    if reduction == "mean":
        ge = ge / acc(N)
    ge = np.broadcast_to(ge, f.shape)
    scale = acc(2) * O.pi_of(acc) / acc(sample_rate)
    with np.errstate(invalid="ignore"):
        phi = np.cumsum(w, axis=-2)
        ga = np.where(dead, acc(0), ge * np.sin(phi))
        q = ge * ap * np.cos(phi)
        gf = scale * np.flip(np.cumsum(np.flip(q, axis=-2), axis=-2), axis=-2)
        M = scale * np.abs(ge * ap).sum(axis=-2, keepdims=True)
    return gf, ga, np.abs(ge), M


def filter_waveform_grad(x, h, g, acc=np.float64):
    """x, g (rows, T), h (F, L) or (rows, F, L).  Returns (gx, sum_j |h||g|, gh, sum |x||g|, K): gx[m] = sum_j h[m // C][j]
    g[m - d + j]; gh[set][c][j] = sum of x[r][m] g[r][m - d + j] over the m of chunk c (over every row r where h is shared),
    the g index inside the row; K the number of terms of each element of gh."""
    x, h, g = x.astype(acc), h.astype(acc), g.astype(acc)
    rows, T = x.shape
    F, L = h.shape[-2:]
    assert T % F == 0
    C, d = T // F, (L - 1) // 2
    m = np.arange(T)
    n = m[:, None] - d + np.arange(L)[None, :]                      # (T, L): the index into g
    ok = (n >= 0) & (n < T)
    nc = np.clip(n, 0, T - 1)
    j = np.broadcast_to(np.arange(L)[None, :], n.shape)
    gx, gx_mag = np.empty((rows, T), acc), np.empty((rows, T), acc)
    gh, gh_mag = np.zeros(h.shape, acc), np.zeros(h.shape, acc)
    count = ok.reshape(F, C, L).sum(axis=1)
    for r in range(rows):
        hr = h[r] if h.ndim == 3 else h
        terms = np.where(ok, hr[(m // C)[:, None], j] * g[r][nc], acc(0))
        gx[r] = terms.sum(axis=1)
        gx_mag[r] = np.abs(terms).sum(axis=1)
        prod = np.where(ok, x[r][:, None] * g[r][nc], acc(0)).reshape(F, C, L)
        if h.ndim == 3:
            gh[r] = prod.sum(axis=1)
            gh_mag[r] = np.abs(prod).sum(axis=1)
        else:
            gh += prod.sum(axis=1)
            gh_mag += np.abs(prod).sum(axis=1)
    K = np.broadcast_to(count if h.ndim == 3 else count * rows, h.shape)
    return gx, gx_mag, gh, gh_mag, K
