"""The definition of F.ray_tracing in numpy, vectorised over the rays of one room.  The same code evaluates in float64 or
numpy.longdouble (`dtype`): every array is of that type and every operation is in it.  Inputs are taken as STORED: a float32
room evaluated in float64 is the float32 values widened.

Order of operations (what "float64 of the definition" means): sums over the axes run left to right, every product is rounded
on its own; ``phi = i * (pi * (3 - sqrt 5))`` (3-D) or ``(2 pi) * (i + 1/2) / N`` (2-D); ``st = 2 * cos * p_eq * tr *
scattering`` left to right; ``e = num / (r2 * p_hit)``.  In float64 the directions take cos and sin from Python's math module
(the C library's, which the CPU replay calls too).

trace() returns, besides the float sum of the contributions, the contract's fixed-point form -- every contribution enters an
int64 sum as rint(e 2^k), k = scale_log2(mic_radius) --, the number of contributions per (microphone, bin), and the smallest
margin of every discrete decision it made (see MARGINS), so that a caller can require inputs on which no float64 rounding
difference flips a decision."""
import math
import types

import numpy as np

LD = np.longdouble
HEADROOM = 64
MAX_BOUNCES = 4096
MARGINS = ("|q - R^2| where 0 <= u <= t", "|u| and |u - t| where q < R^2", "the gap between the two smallest t_d",
           "the distance of d / w_bin from an integer", "|travel - S_max|", "|d - S_max| of a scattered path",
           "|max tr - energy_thres|", "|max st - energy_thres|")


def num_bins(time_thres, hist_bin_size) -> int:
    return int(math.ceil(float(time_thres) / float(hist_bin_size)))


def scale_log2(mic_radius, headroom=HEADROOM) -> int:
    """k = 62 - ceil(log2(8 H / R^2)), the logarithm taken exactly (integer arithmetic on the float's ratio)."""
    num, den = (8.0 * headroom / (float(mic_radius) * float(mic_radius))).as_integer_ratio()
    c = 0                                                        # ceil(log2(num / den))
    while num > den * 2 ** c:
        c += 1
    while c > -2000 and num <= den * 2 ** (c - 1):
        c -= 1
    return 62 - c


def bounce_bound(room, time_thres, sound_speed) -> float:
    s_max = np.float64(time_thres) * np.float64(sound_speed)
    with np.errstate(all="ignore"):
        return float(sum(np.floor(s_max / np.float64(r)) + 2.0 for r in np.asarray(room, np.float64)))


def bad_room(room, source, mic_array, absorption, scattering, time_thres, sound_speed) -> bool:
    room, source, mic = (np.asarray(t, np.float64) for t in (room, source, mic_array))
    ab, sc = np.asarray(absorption, np.float64), np.asarray(scattering, np.float64)
    ok = bool(np.isfinite(room).all() and (room > 0).all())
    ok = ok and bool(((source > 0) & (source < room)).all() and ((mic > 0) & (mic < room[None])).all())
    ok = ok and bool(((ab >= 0) & (ab <= 1)).all() and ((sc >= 0) & (sc <= 1)).all())
    return not (ok and bounce_bound(room, time_thres, sound_speed) <= MAX_BOUNCES)


def directions(n: int, D: int, dtype) -> np.ndarray:
    i = np.arange(n)
    if dtype is np.float64:
        pi, cos, sin = math.pi, (lambda a: np.array([math.cos(x) for x in a])), (lambda a: np.array([math.sin(x) for x in a]))
        golden = math.pi * (3.0 - math.sqrt(5.0))
    else:
        pi, cos, sin = dtype(4) * np.arctan(dtype(1)), np.cos, np.sin
        golden = pi * (dtype(3) - np.sqrt(dtype(5)))
    f = i.astype(dtype)
    if D == 3:
        z = dtype(1) - (2 * i + 1).astype(dtype) / dtype(n)
        rho = np.sqrt(dtype(1) - z * z)
        phi = f * golden
        return np.stack([rho * cos(phi), rho * sin(phi), z], axis=1).astype(dtype)
    phi = (dtype(2) * pi) * (f + dtype(0.5)) / dtype(n)
    return np.stack([cos(phi), sin(phi)], axis=1).astype(dtype)


def _dot(a, b):
    """sum_d a_d b_d, left to right."""
    s = a[:, 0] * b[:, 0]
    for d in range(1, a.shape[1]):
        s = s + a[:, d] * b[:, d]
    return s


def trace(room, source, mic_array, num_rays, absorption, scattering, mic_radius=0.5, sound_speed=343.0, energy_thres=1e-7,
          time_thres=10.0, hist_bin_size=0.004, dtype=np.float64):
    """One good room: room (D,), source (D,), mic_array (M, D), absorption and scattering (NB, 2 D).  Returns a namespace of
    hist (M, NB, bins) of `dtype` (the float sum), acc (M, NB, bins) int64 (the fixed-point sum), count (M, bins), k, margin,
    bounces (the longest ray), bound (K), top (the largest contribution over 4 E0 / R^2), fullest (the largest count)."""
    room, source, mic, ab, sc = (np.asarray(t).astype(dtype) for t in (room, source, mic_array, absorption, scattering))
    assert not bad_room(room, source, mic, ab, sc, time_thres, sound_speed)
    D, M, NB, N = room.shape[0], mic.shape[0], ab.shape[0], int(num_rays)
    bins, k = num_bins(time_thres, hist_bin_size), scale_log2(mic_radius)
    e0, s_max = dtype(2) / dtype(N), dtype(time_thres) * dtype(sound_speed)
    r2c, w_bin, thr = dtype(mic_radius) * dtype(mic_radius), dtype(sound_speed) * dtype(hist_bin_size), dtype(energy_thres)
    scale = dtype(2) ** k
    K = int(bounce_bound(room, time_thres, sound_speed))
    res = types.SimpleNamespace(hist=np.zeros((M, NB, bins), dtype), acc=np.zeros((M, NB, bins), np.int64),
                                count=np.zeros((M, bins), np.int64), k=k, margin=math.inf, bounces=0, bound=K, top=0.0, fullest=0)

    def note(values):
        if values.size:
            res.margin = min(res.margin, float(np.abs(values).min()))

    def deposit(m, d, num):
        y = d / w_bin
        x = np.floor(y)
        note(y - np.rint(y))
        ok = (x >= 0) & (x < bins)
        if not ok.any():
            return
        d, num, b = d[ok], num[ok], x[ok].astype(np.int64)
        rr = np.maximum(d * d, r2c)
        p_hit = dtype(1) - np.sqrt(dtype(1) - r2c / rr)
        e = num / (rr * p_hit)[:, None]
        res.top = max(res.top, float(e.max() / (dtype(4) * e0 / r2c)))
        np.add.at(res.count[m], b, 1)
        for band in range(NB):
            np.add.at(res.hist[m, band], b, e[:, band])
            np.add.at(res.acc[m, band], b, np.rint(e[:, band] * scale).astype(np.int64))

    p, dirs = np.tile(source, (N, 1)), directions(N, D, dtype)
    tr, travel, alive = np.full((N, NB), e0, dtype), np.zeros(N, dtype), np.ones(N, bool)
    for step in range(K):
        idx = np.nonzero(alive)[0]
        if idx.size == 0:
            break
        res.bounces = step + 1
        P, Dr, T, TR, ar = p[idx], dirs[idx], travel[idx], tr[idx], np.arange(idx.size)
        with np.errstate(divide="ignore", invalid="ignore"):
            td = np.where(Dr > 0, (room[None] - P) / Dr, np.where(Dr < 0, P / (-Dr), dtype(np.inf)))
        t, axis = td.min(axis=1), td.argmin(axis=1)                  # argmin: the first axis that attains the minimum
        two = np.sort(td, axis=1)[:, :2]
        note((two[:, 1] - two[:, 0])[np.isfinite(two[:, 1])])
        up = Dr[ar, axis] > 0
        w = 2 * axis + up
        for m in range(M):                                           # 2. direct hits
            v = mic[m][None] - P
            u, vv = _dot(v, Dr), _dot(v, v)
            q = vv - u * u
            note((q - r2c)[(u >= -1e-6) & (u <= t + 1e-6)])
            near = q < r2c + 1e-6
            note(u[near])
            note((u - t)[near])
            hit = (u >= 0) & (u <= t) & (q < r2c)
            if hit.any():
                deposit(m, (T + u)[hit], TR[hit])
        T = T + t                                                    # 3. to the wall
        P = P + t[:, None] * Dr
        P[ar, axis] = np.where(up, room[axis], dtype(0))
        TR = TR * (dtype(1) - ab[:, w].T)
        scw = sc[:, w].T
        sel = (scw > 0).any(axis=1)
        if sel.any():                                                # 4. the scattered share
            for m in range(M):
                v = mic[m][None] - P[sel]
                h2 = _dot(v, v)
                h = np.sqrt(h2)
                cos_theta = np.abs(v[np.arange(v.shape[0]), axis[sel]]) / h
                p_eq = dtype(1) - np.sqrt(dtype(1) - r2c / np.maximum(h2, r2c))
                st = (dtype(2) * cos_theta * p_eq)[:, None] * TR[sel] * scw[sel]
                d, top = T[sel] + h, st.max(axis=1)
                note(d - s_max)
                note(top - thr)
                ok = (d < s_max) & (top > thr)
                if ok.any():
                    deposit(m, d[ok], st[ok])
        TR = TR * (dtype(1) - scw)                                   # 5. attenuate and test
        top = TR.max(axis=1)
        note(T - s_max)
        note(top - thr)
        end = (T > s_max) | (top < thr)
        Dr[ar, axis] = -Dr[ar, axis]                                 # 6. reflect
        p[idx], dirs[idx], travel[idx], tr[idx] = P, Dr, T, TR
        alive[idx[end]] = False
    assert not alive.any(), "a ray outlived the bounce bound"
    res.fullest = int(res.count.max()) if res.count.size else 0
    return res


def final(acc: np.ndarray, k: int, dtype) -> np.ndarray:
    """acc 2^-k rounded once to `dtype` (float32 or float64); NaN for a negative (wrapped) sum."""
    v = np.ldexp(acc.astype(LD), -k)                                 # exact: longdouble holds 64 bits
    out = v.astype(dtype)
    out[acc < 0] = np.nan
    return out
