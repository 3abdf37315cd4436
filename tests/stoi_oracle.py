"""The definition of F.stoi (STOI / ESTOI at 10 kHz) restated in float64 numpy, phase by phase, and the same definition with the
window products, overlap-add, transform, band sums and square root in float32 (`precision="f32"`: the kept set and the segment
statistic stay float64, the transform is scipy's single-precision rfft).  The float32 variant measures what the number format
costs; the tests derive their bar from it.  TEST INFRASTRUCTURE ONLY: nothing here is imported by the package."""
import numpy as np
import scipy.fft

FS = 10000
N_FRAME = 256
HOP = 128
N_FFT = 512
N_BANDS = 15
SEG = 30
EPS = 2.0 ** -52
DYN_RANGE = 40.0
CLIP = 1.0 + 10.0 ** 0.75          # 1 + 10^(-beta / 20), beta = -15 dB
SHORT = 1e-5
BAND_LO = (7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174)
BAND_HI = (9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219)


def window():
    n = np.arange(N_FRAME, dtype=np.float64)
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * (n + 1.0) / (N_FRAME + 1.0))


def band_table():
    """(lo, hi) of the 15 third-octave bands: the bins nearest to 150 * 2^((2b -+ 1) / 6) Hz on the grid f * 10000 / 512."""
    f = np.arange(N_FFT // 2 + 1, dtype=np.float64) * FS / N_FFT
    b = np.arange(N_BANDS, dtype=np.float64)
    lo = [int(np.argmin((f - 150.0 * 2.0 ** ((2 * k - 1) / 6.0)) ** 2)) for k in b]
    hi = [int(np.argmin((f - 150.0 * 2.0 ** ((2 * k + 1) / 6.0)) ** 2)) for k in b]
    return tuple(lo), tuple(hi)


def n_frames(L):
    return (L - N_FRAME) // HOP + 1 if L >= N_FRAME else 0


def energies(x):
    """e_i in dB of every frame of the clean signal, float64 from the samples as stored."""
    x = np.asarray(x).astype(np.float64)
    K = n_frames(len(x))
    if K == 0:
        return np.zeros((0,), np.float64)
    idx = HOP * np.arange(K)[:, None] + np.arange(N_FRAME)[None, :]
    fr = x[idx] * window()[None, :]
    return 20.0 * np.log10(np.sqrt(np.sum(fr * fr, axis=1)) + EPS)


def kept_frames(x):
    """(ascending kept indices, the smallest |e_i - threshold| in dB)."""
    e = energies(x)
    if len(e) == 0:
        return np.zeros((0,), np.int64), np.inf
    thr = e.max() - DYN_RANGE
    return np.nonzero(e > thr)[0].astype(np.int64), float(np.min(np.abs(e - thr)))


def rebuild(x, kept, dtype=np.float64):
    """Overlap-add at hop 128 of the kept frames of x, windowed, in `dtype`."""
    K = len(kept)
    w = window().astype(dtype)
    x = np.asarray(x).astype(dtype)
    out = np.zeros((HOP * (K - 1) + N_FRAME if K else 0,), dtype)
    for j, i in enumerate(kept):
        out[HOP * j:HOP * j + N_FRAME] += w * x[HOP * i:HOP * i + N_FRAME]
    assert out.dtype == dtype
    return out


def band_magnitudes(xs, dtype=np.float64):
    """T[m, b] of a rebuilt signal: M = K - 1 frames (the last is dropped), window again, 512-point transform, 15 band norms."""
    M = len(range(0, len(xs) - N_FRAME, HOP))
    out = np.zeros((M, N_BANDS), dtype)
    if M == 0:
        return out
    w = window().astype(dtype)
    idx = HOP * np.arange(M)[:, None] + np.arange(N_FRAME)[None, :]
    fr = (xs.astype(dtype)[idx] * w[None, :]).astype(dtype)
    spec = scipy.fft.rfft(fr, n=N_FFT, axis=-1)
    assert spec.dtype == (np.complex64 if dtype == np.float32 else np.complex128)
    p = (spec.real * spec.real + spec.imag * spec.imag).astype(dtype)
    for b in range(N_BANDS):
        out[:, b] = np.sqrt(np.sum(p[:, BAND_LO[b]:BAND_HI[b]], axis=1, dtype=dtype))
    assert out.dtype == dtype
    return out


def _row_col_normalize(a):
    a = a - a.mean(axis=-1, keepdims=True)
    return a / (np.linalg.norm(a, axis=-1, keepdims=True) + EPS)


def segment_sum(Tx, Ty, extended):
    """(the sum over segments of the statistic, J) from float64 band matrices (M, 15)."""
    Tx, Ty = np.asarray(Tx, np.float64), np.asarray(Ty, np.float64)
    M = Tx.shape[0]
    J = M - SEG + 1
    if J < 1:
        return 0.0, 0
    total = 0.0
    for s in range(J):
        a, c = Tx[s:s + SEG].T, Ty[s:s + SEG].T                   # (15, 30)
        if extended:
            A, Cm = _row_col_normalize(a), _row_col_normalize(c)  # rows: bands over time
            A, Cm = _row_col_normalize(A.T), _row_col_normalize(Cm.T)   # columns: frames over bands
            total += float(np.sum(A * Cm))
        else:
            alpha = np.linalg.norm(a, axis=1, keepdims=True) / (np.linalg.norm(c, axis=1, keepdims=True) + EPS)
            cp = np.minimum(alpha * c, CLIP * a)
            total += float(np.sum(_row_col_normalize(a) * _row_col_normalize(cp)))
    return total, J


def stoi(preds, target, extended=False, precision="f64"):
    """The score of one row at 10 kHz."""
    dtype = np.float32 if precision == "f32" else np.float64
    x, y = np.asarray(target), np.asarray(preds)
    assert x.shape == y.shape and x.ndim == 1
    if not (np.all(np.isfinite(x)) and np.all(np.isfinite(y))):
        return float("nan")
    kept, _ = kept_frames(x)
    if len(kept) - 1 < SEG:
        return SHORT
    Tx = band_magnitudes(rebuild(x, kept, dtype), dtype)
    Ty = band_magnitudes(rebuild(y, kept, dtype), dtype)
    total, J = segment_sum(Tx, Ty, extended)
    return total / ((SEG if extended else N_BANDS) * J)


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def gated_harmonic(L, seed):
    """A 24-partial carrier at 120 Hz with 2 % vibrato, times a squared half-sine envelope at 1.3-1.7 Hz, times an on/off gate
    at 0.35 Hz (on for 0.3 of its period), times 0.05, plus 1e-4 white noise; float32.  What this generator gives: at L = 30000,
    seeds 0-3, 63-72 of 233 frames are kept, not contiguous, the nearest e_i 0.23-2.75 dB from the threshold; seed 1 at
    L = 12000 keeps 56 of 92 (1.26 dB); seed 3 at L = 6000 keeps all 45; seed 0 at L = 6000 keeps 19 and scores 1e-5."""
    rng = np.random.default_rng(1000 + seed)
    t = np.arange(L, dtype=np.float64) / FS
    env_rate = 1.3 + 0.4 * rng.random()
    vib_rate = 4.0 + 2.0 * rng.random()
    phase0 = 2.0 * np.pi * rng.random()
    gate_phase = rng.random()
    phase = 2.0 * np.pi * 120.0 * t + 0.02 * 120.0 / vib_rate * np.sin(2.0 * np.pi * vib_rate * t) + phase0
    amps = 1.0 / np.arange(1, 25) * (0.5 + rng.random(24))
    carrier = sum(a * np.sin(h * phase) for h, a in zip(range(1, 25), amps))
    env = np.sin(np.pi * env_rate * t + np.pi * rng.random()) ** 2
    gate = (np.mod(0.35 * t + gate_phase, 1.0) < 0.3).astype(np.float64)
    return (0.05 * carrier * env * gate + 1e-4 * rng.standard_normal(L)).astype(np.float32)


def add_noise_db(x, snr_db, seed):
    """x plus white noise at `snr_db` relative to the whole row's power; float32."""
    rng = np.random.default_rng(5000 + seed)
    n = rng.standard_normal(len(x))
    xs = np.asarray(x, np.float64)
    g = np.sqrt(np.mean(xs * xs) / (np.mean(n * n) * 10.0 ** (snr_db / 10.0)))
    return (xs + g * n).astype(np.float32)


def stationary_noise(L, seed):
    return (0.1 * np.random.default_rng(9000 + seed).standard_normal(L)).astype(np.float32)


# (name, L, seed, snr): the cases of the GPU and the replay tests
CASES = (("L30000_s0_20dB", 30000, 0, 20.0), ("L30000_s1_5dB", 30000, 1, 5.0), ("L30000_s2_m5dB", 30000, 2, -5.0),
         ("L30000_s3_5dB", 30000, 3, 5.0), ("L12000_s1_5dB", 12000, 1, 5.0), ("L12000_s1_m5dB", 12000, 1, -5.0),
         ("L6000_s3_20dB", 6000, 3, 20.0), ("L6000_s3_m5dB", 6000, 3, -5.0), ("L6000_s0_5dB", 6000, 0, 5.0))

_case_cache = {}


def case(name):
    """(target, preds, {mode: (d64, d32)}, kept indices, margin in dB) of a named case, computed once."""
    if name not in _case_cache:
        _, L, seed, snr = next(c for c in CASES if c[0] == name)
        x = gated_harmonic(L, seed)
        y = add_noise_db(x, snr, seed)
        kept, margin = kept_frames(x)
        scores = {ext: (stoi(y, x, ext, "f64"), stoi(y, x, ext, "f32")) for ext in (False, True)}
        for v in (x, y, kept):
            v.setflags(write=False)
        _case_cache[name] = (x, y, scores, kept, margin)
    return _case_cache[name]


def bar(extended):
    """4 x the largest |d32 - d64| over the cases, per mode: the float32 definition's own error, with a margin of 4 because the
    kernel's transform orders its sums differently from scipy's."""
    return 4.0 * max(abs(case(c[0])[2][extended][1] - case(c[0])[2][extended][0]) for c in CASES)
