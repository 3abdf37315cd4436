"""The separation metrics of audio_amd.functional restated in numpy, one row at a time: the contract of F.signal_distortion_ratio,
F.scale_invariant_signal_distortion_ratio, F.scale_invariant_signal_noise_ratio and F.signal_noise_ratio (the definitions of
torchmetrics as the issue states them; this file governs wherever upstream differs).  SDR is given twice: in float64 the
reference's way (zero-padded FFT correlations, a dense solve) and in longdouble (direct sums, Levinson).  The SI family and SNR
take the arithmetic's dtype; ``eps`` is the input dtype's."""
import numpy as np

LD = np.longdouble


def _rows(preds, target, zero_mean, dt):
    p, t = np.asarray(preds).astype(dt), np.asarray(target).astype(dt)
    if zero_mean and p.size:
        p, t = p - p.mean(dtype=dt), t - t.mean(dtype=dt)
    return p, t


def _unit(x, dt):
    return x / max(np.sqrt(np.sum(x * x, dtype=dt)), dt(1e-6))


def _score(coh):
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(10.0 * np.log10(coh / (1 - coh)))


def sdr_float64(preds, target, filter_length=512, zero_mean=False, load_diag=None):
    p, t = _rows(preds, target, zero_mean, np.float64)
    p, t = _unit(p, np.float64), _unit(t, np.float64)
    n = 1 << int(np.ceil(np.log2(max(2 * t.size - 1, 1))))
    tf, pf = np.fft.rfft(t, n), np.fft.rfft(p, n)
    r = np.fft.irfft(tf.real ** 2 + tf.imag ** 2, n)[:filter_length]
    b = np.fft.irfft(np.conj(tf) * pf, n)[:filter_length]
    r, b = np.pad(r, (0, filter_length - r.size)), np.pad(b, (0, filter_length - b.size))
    if load_diag is not None:
        r[0] += load_diag
    idx = np.abs(np.arange(filter_length)[:, None] - np.arange(filter_length)[None, :])
    try:
        h = np.linalg.solve(r[idx], b)
    except np.linalg.LinAlgError:
        return float("nan")
    return _score(np.dot(b, h))


def levinson(r, b):
    """Toeplitz(r) h = b; NaN where a step's prediction error is not finite and positive."""
    dt, L = r.dtype.type, r.size
    if not (np.isfinite(r[0]) and r[0] > 0):
        return np.full(L, np.nan, dt)
    f, x = np.zeros(L, dt), np.zeros(L, dt)
    f[0], x[0] = 1 / r[0], b[0] / r[0]
    for m in range(1, L):
        rev = r[m:0:-1]
        ef, ex = np.dot(rev, f[:m]), np.dot(rev, x[:m])
        d = 1 - ef * ef
        if not (np.isfinite(d) and d > 0):
            return np.full(L, np.nan, dt)
        f[:m + 1] = (np.r_[f[:m], dt(0)] - ef * np.r_[dt(0), f[:m][::-1]]) / d
        x[:m + 1] += (b[m] - ex) * f[:m + 1][::-1]
    return x


def sdr_longdouble(preds, target, filter_length=512, zero_mean=False, load_diag=None):
    p, t = _rows(preds, target, zero_mean, LD)
    p, t = _unit(p, LD), _unit(t, LD)
    N, r, b = t.size, np.zeros(filter_length, LD), np.zeros(filter_length, LD)
    for k in range(min(filter_length, N)):
        r[k], b[k] = np.dot(t[:N - k], t[k:]), np.dot(t[:N - k], p[k:])
    if load_diag is not None:
        r[0] += LD(load_diag)
    return _score(np.dot(b, levinson(r, b)))


def si_sdr(preds, target, zero_mean=False, dtype=np.float64, eps=np.finfo(np.float32).eps):
    p, t = _rows(preds, target, zero_mean, dtype)
    eps = dtype(eps)
    alpha = (np.sum(p * t, dtype=dtype) + eps) / (np.sum(t * t, dtype=dtype) + eps)
    s = alpha * t
    return float(10 * np.log10((np.sum(s * s, dtype=dtype) + eps) / (np.sum((s - p) ** 2, dtype=dtype) + eps)))


def si_snr(preds, target, dtype=np.float64, eps=np.finfo(np.float32).eps):
    return si_sdr(preds, target, True, dtype, eps)


def snr(preds, target, zero_mean=False, dtype=np.float64, eps=np.finfo(np.float32).eps):
    p, t = _rows(preds, target, zero_mean, dtype)
    eps = dtype(eps)
    return float(10 * np.log10((np.sum(t * t, dtype=dtype) + eps) / (np.sum((t - p) ** 2, dtype=dtype) + eps)))


def signals(time, seed=0):
    """Three seeded rows of `time` samples: targets AR(2)-coloured (1.6, -0.8), low-passed, AR(2); preds a 5-tap filtering of
    the target plus white noise at 0, 10 and 30 dB.  Returned as float64 (preds, target), each (3, time)."""
    if time == 0:
        return np.zeros((3, 0)), np.zeros((3, 0))
    rng = np.random.default_rng(seed)
    n = time + 128
    ts = []
    for kind in ("ar", "lp", "ar"):
        e = rng.standard_normal(n)
        if kind == "ar":
            x = np.zeros(n)
            for i in range(n):
                x[i] = e[i] + (1.6 * x[i - 1] if i > 0 else 0.0) - (0.8 * x[i - 2] if i > 1 else 0.0)
        else:
            x = np.convolve(e, np.sinc(0.2 * np.arange(-40, 41)) * np.hanning(81))[:n]
        ts.append(x[128:])
    t = np.stack(ts)
    g = rng.standard_normal((3, 5)) * np.array([1, .5, .2, .1, .05])
    p = np.stack([np.convolve(t[i], g[i])[:time] for i in range(3)])
    p += 10.0 ** (-np.array([0, 10, 30])[:, None] / 20) * np.sqrt(np.mean(p * p, axis=1, keepdims=True)) * rng.standard_normal((3, time))
    return p, t
