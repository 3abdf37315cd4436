"""The definition of the synthesis ops of audio_amd.prototype.functional (oscillator_bank, filter_waveform,
sinc_impulse_response, frequency_impulse_response, adsr_envelope, extend_pitch) in numpy: float64, or longdouble where
`acc` says so.  Never imported by the product.  The arithmetic that the definition fixes in the input's own type (the phase
increment of the oscillator, the product of extend_pitch) is done in that type; everything after it in `acc`."""
import numpy as np

LD = np.longdouble
PI_LD = np.arctan(LD(1)) * 4


def pi_of(acc):
    return PI_LD if acc is LD else acc(np.pi)


# ---- oscillator_bank -------------------------------------------------------------------------------------------------------
def osc_increment(f, sample_rate):
    """w = remainder((f * 2 pi) / sample_rate, 2 pi) in f's own type (float32 or float64), every operation rounded once."""
    t = f.dtype.type
    two_pi = t(2.0 * np.pi)
    with np.errstate(invalid="ignore", over="ignore"):
        v = (f * two_pi) / t(sample_rate)
        w = np.fmod(v, two_pi)
        return np.where((w != 0) & (w < 0), w + two_pi, w).astype(f.dtype)


def osc_amplitudes(f, a, sample_rate):
    return np.where(np.abs(f) >= f.dtype.type(sample_rate / 2.0), f.dtype.type(0), a)


def oscillator_bank(f, a, sample_rate, reduction="sum", acc=np.float64):
    """(result in `acc`, sum_n |a'|): f and a are (..., T, N) float32 or float64."""
    w = osc_increment(f, sample_rate).astype(acc)
    ap = osc_amplitudes(f, a, sample_rate).astype(acc)
    with np.errstate(invalid="ignore"):
        y = ap * np.sin(np.cumsum(w, axis=-2))
        mag = np.abs(ap).sum(axis=-1)
        if reduction == "none":
            return y, np.abs(ap)
        s = y.sum(axis=-1)
        return (s / acc(f.shape[-1]), mag / f.shape[-1]) if reduction == "mean" else (s, mag)


def oscillator_bank_unreduced_f32(f, a, sample_rate):
    """The reference's float32 tail: the float64 phase cast to float32 as it is, then sin, product and sum in float32."""
    w = osc_increment(f, sample_rate).astype(np.float64)
    ap = osc_amplitudes(f, a, sample_rate)
    ph = np.cumsum(w, axis=-2).astype(np.float32)
    return (ap * np.sin(ph)).sum(axis=-1, dtype=np.float32)


# ---- filter_waveform -------------------------------------------------------------------------------------------------------
def filter_waveform(x, h, acc=np.float64):
    """(y, sum_j |x[m]| |h[m // C][j]|): x (rows, T), h (F, L) or (rows, F, L); y[n] = sum_j x[m] h[m // C][j], m = n + d - j."""
    x = x.astype(acc)
    h = h.astype(acc)
    rows, T = x.shape
    F, L = h.shape[-2:]
    assert T % F == 0
    C, d = T // F, (L - 1) // 2
    m = np.arange(T)[:, None] + d - np.arange(L)[None, :]            # (T, L)
    ok = (m >= 0) & (m < T)
    mc = np.clip(m, 0, T - 1)
    j = np.broadcast_to(np.arange(L)[None, :], m.shape)
    y = np.empty((rows, T), acc)
    mag = np.empty((rows, T), acc)
    for r in range(rows):
        hr = h[r] if h.ndim == 3 else h
        terms = np.where(ok, x[r][mc] * hr[mc // C, j], acc(0))
        y[r] = terms.sum(axis=1)
        mag[r] = np.abs(terms).sum(axis=1)
    return y, mag


def filter_waveform_overlap_add(x, h):
    """The reference's form for one row in float64: chunks of C samples, one full convolution each, overlap-add, crop."""
    T = x.shape[0]
    F, L = h.shape
    C, d = T // F, (L - 1) // 2
    buf = np.zeros(T + L - 1)
    for c in range(F):
        buf[c * C:c * C + C + L - 1] += np.convolve(x[c * C:(c + 1) * C].astype(np.float64), h[c].astype(np.float64))
    return buf[d:d + T]


# ---- the designers ---------------------------------------------------------------------------------------------------------
def sinc_impulse_response(cutoff, window_size=513, high_pass=False, acc=np.float64):
    """cutoff (...) -> (..., window_size) in `acc`."""
    pi = pi_of(acc)
    half = window_size // 2
    i = np.arange(-half, half + 1)
    px = pi * (np.asarray(cutoff).astype(acc)[..., None] * i.astype(acc))
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where(px == 0, acc(1), np.sin(px) / np.where(px == 0, acc(1), px))
    if window_size == 1:
        win = np.ones(1, acc)
    else:
        win = acc(0.54) - acc(0.46) * np.cos(acc(2) * pi * (i + half).astype(acc) / acc(window_size - 1))
    g = s * win
    h = g / np.abs(g.sum(axis=-1, keepdims=True))
    if high_pass:
        h = -h
        h[..., half] = h[..., half] + acc(1)
    return h


def frequency_impulse_response(m, acc=np.float64):
    """(out, bound term): m (..., n) -> (..., N); the second value is (sum_j c_j |m_j|) / N * window."""
    m = np.asarray(m).astype(acc)
    n = m.shape[-1]
    N = 2 * (n - 1)
    pi = pi_of(acc)
    c = np.full(n, acc(2))
    c[0] = c[-1] = acc(1)
    k = np.arange(N)
    q = (np.arange(n)[None, :] * k[:, None]) % N                    # (N, n): j k mod N
    cosm = np.cos(acc(2) * pi * q.astype(acc) / acc(N))
    cosm[:, -1] = np.where(k % 2 == 0, acc(1), acc(-1))
    cosm[:, 0] = acc(1)
    ir = ((m * c)[..., None, :] * cosm).sum(axis=-1) / acc(N)        # (..., N)
    i = np.arange(N)
    win = acc(0.5) * (acc(1) - np.cos(acc(2) * pi * i.astype(acc) / acc(N - 1)))
    out = ir[..., (i + N // 2) % N] * win
    mag = (np.abs(m) * c).sum(axis=-1, keepdims=True) / acc(N) * win
    return out, mag


def adsr_envelope(num_frames, attack=0.0, hold=0.0, decay=0.0, sustain=1.0, release=0.0, n_decay=2):
    """float64 (num_frames,)."""
    n = num_frames - 1
    na, nh, nd, nr = int(n * attack), int(n * hold), int(n * decay), int(n * release)
    out = np.full(num_frames, float(sustain), np.float64)
    if na > 0:
        out[:na + 1] = np.linspace(0.0, 1.0, na + 1)
    if nh > 0:
        out[na:na + nh + 1] = 1.0
    if nd > 0:
        out[na + nh:na + nh + nd + 1] = np.linspace(1.0, 0.0, nd + 1) ** n_decay * (1.0 - sustain) + sustain
    if nr > 0:
        out[-nr - 1:] = np.linspace(sustain, 0.0, nr + 1)
    return out


def extend_pitch(base, pattern):
    """base (..., T, 1) and pattern (N,) of one type (float32 or float64): the products rounded once."""
    return (base * pattern.reshape((1,) * (base.ndim - 1) + (-1,))).astype(base.dtype)
