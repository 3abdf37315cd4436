"""The definition of F.simulate_rir_ism in numpy, written two independent ways: the gather form (every output sample collects
the delay filters that cover it) and the reference's scatter form (every image lays its filter down from ceil(tau) on).  The
same code evaluates in float32, float64 or numpy.longdouble (`dtype`): every array is of that type and every operation is in
it.  Inputs are taken as STORED: a float32 room evaluated in float64 is the float32 values widened.

Order of operations (what "float64 of the definition" means): loc = room (v + 1) - source or room v + source; d2 = the squares of
loc - mic added axis by axis; dist = sqrt(d2); tau = dist * sample_rate / sound_speed left to right; tr = sqrt(1 - absorption);
att = the product over the axes of tr_lower ** |floor(v / 2)| * tr_upper ** |floor((v + 1) / 2)|; a = att / dist."""
import itertools

import numpy as np

LD = np.longdouble


def lattice(max_order: int, D: int) -> np.ndarray:
    """int64 (n_img, D): every integer vector with sum |v_d| <= max_order, in the order of cartesian_prod (last axis fastest)."""
    r = range(-max_order, max_order + 1)
    return np.array([p for p in itertools.product(*([r] * D)) if sum(abs(v) for v in p) <= max_order], dtype=np.int64).reshape(-1, D)


def image_count(max_order: int, D: int) -> int:
    return lattice(max_order, D).shape[0]


def _pi(dtype):
    return dtype(4) * np.arctan(dtype(1))


def _sinc(x, dtype):
    y = _pi(dtype) * x
    safe = np.where(x == 0, dtype(1), y)
    return np.where(x == 0, dtype(1), np.sin(safe) / safe).astype(dtype)


def geometry(room, source, mic_array, max_order, absorption, sample_rate, sound_speed, dtype=np.float64):
    """(dist, a, tau), each (n_img, M) of `dtype`, for one room: room (D,), source (D,), mic_array (M, D), absorption (2 D,)."""
    room, source, mic, ab = (np.asarray(t).astype(dtype) for t in (room, source, mic_array, absorption))
    D = room.shape[0]
    v = lattice(max_order, D)
    d2 = np.zeros((v.shape[0], mic.shape[0]), dtype)
    att = np.ones((v.shape[0],), dtype)
    tr = np.sqrt(dtype(1) - ab)
    for d in range(D):
        odd = v[:, d] % 2 == 1                                   # Python %: -1 is odd
        loc = np.where(odd, room[d] * (v[:, d] + 1).astype(dtype) - source[d], room[d] * v[:, d].astype(dtype) + source[d])
        diff = loc[:, None] - mic[None, :, d]
        d2 = d2 + diff * diff
        lo, hi = np.abs(v[:, d] // 2), np.abs((v[:, d] + 1) // 2)
        att = att * (tr[2 * d] ** lo.astype(dtype) * tr[2 * d + 1] ** hi.astype(dtype))
    dist = np.sqrt(d2)
    with np.errstate(divide="ignore", invalid="ignore"):
        a = att[:, None] / dist
    tau = dist * dtype(sample_rate) / dtype(sound_speed)
    return dist.astype(dtype), a.astype(dtype), tau.astype(dtype)


def length(room, source, mic_array, max_order, sample_rate=16000.0, sound_speed=343.0, delay_filter_length=81) -> int:
    """L of the definition when output_length is not given: ceil(max tau) + fl, in float64."""
    D = np.asarray(room).shape[0]
    _, _, tau = geometry(room, source, mic_array, max_order, np.zeros(2 * D), sample_rate, sound_speed, np.float64)
    return int(np.ceil(tau.max())) + int(delay_filter_length)


def g(x, pad, dtype):
    """sinc(x) (1 + cos(pi x / pad)) / 2 for |x| <= pad, 0 elsewhere."""
    inside = np.abs(x) <= pad
    xs = np.where(inside, x, dtype(0))
    return np.where(inside, _sinc(xs, dtype) * (dtype(0.5) * (dtype(1) + np.cos(_pi(dtype) * xs / dtype(pad)))), dtype(0)).astype(dtype)


def _terms(room, source, mic_array, max_order, absorption, L, sample_rate, sound_speed, fl, dtype):
    """a g(n - pad - tau): (n_img, M, L) of `dtype`."""
    _, a, tau = geometry(room, source, mic_array, max_order, absorption, sample_rate, sound_speed, dtype)
    pad = fl // 2
    n = np.arange(L).astype(dtype)
    x = (n[None, None, :] - dtype(pad)) - tau[:, :, None]
    return (a[:, :, None] * g(x, pad, dtype)).astype(dtype)


def gather(room, source, mic_array, max_order, absorption, output_length, sample_rate=16000.0, sound_speed=343.0,
           delay_filter_length=81, dtype=np.float64) -> np.ndarray:
    """rir[c, n] = sum_i a_ic g(n - pad - tau_ic): (M, L) of `dtype`.  A non-finite a or tau propagates as numpy does."""
    t = _terms(room, source, mic_array, max_order, absorption, output_length, sample_rate, sound_speed, delay_filter_length, dtype)
    out = np.zeros(t.shape[1:], dtype)
    for i in range(t.shape[0]):                                   # ascending image index
        out = out + t[i]
    return out


def abs_terms(room, source, mic_array, max_order, absorption, output_length, sample_rate=16000.0, sound_speed=343.0,
              delay_filter_length=81, dtype=np.float64) -> np.ndarray:
    """sum_i |a_ic g(n - pad - tau_ic)|: (M, L), what a sum's rounding error scales with."""
    t = _terms(room, source, mic_array, max_order, absorption, output_length, sample_rate, sound_speed, delay_filter_length, dtype)
    return np.abs(t).sum(axis=0)


def scatter(room, source, mic_array, max_order, absorption, output_length, sample_rate=16000.0, sound_speed=343.0,
            delay_filter_length=81, dtype=np.float64) -> np.ndarray:
    """The reference's form: rir[ceil(tau) + k] += a sinc(k - pad + ceil(tau) - tau) hann(k + ceil(tau) - tau), k = 0 .. fl - 1,
    with hann(t) = (1 - cos(2 pi t / (fl - 1))) / 2 on [0, fl - 1] and 0 beyond it."""
    fl = int(delay_filter_length)
    pad = fl // 2
    _, a, tau = geometry(room, source, mic_array, max_order, absorption, sample_rate, sound_speed, dtype)
    M = a.shape[1]
    start = np.ceil(tau)
    frac = (start - tau).astype(dtype)
    first = start.astype(np.int64)
    k = np.arange(fl).astype(dtype)
    buf = np.zeros((M, output_length + fl), dtype)
    for i in range(a.shape[0]):
        for c in range(M):
            if first[i, c] >= output_length:
                continue
            t = k + frac[i, c]
            hann = np.where(t <= dtype(fl - 1), dtype(0.5) * (dtype(1) - np.cos(dtype(2) * _pi(dtype) * t / dtype(fl - 1))), dtype(0))
            taps = (a[i, c] * _sinc(t - dtype(pad), dtype) * hann).astype(dtype)
            buf[c, first[i, c]:first[i, c] + fl] += taps
    return buf[:, :output_length]
