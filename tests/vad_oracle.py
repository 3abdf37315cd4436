"""F.vad / F.vad_start restated in numpy: the plan, the measurements in float64 (the yardstick) and in float32 (the
reference's own arithmetic: float32 buffers, windows and FFTs, the log in float64), and the trigger in Python floats and
ints, which given the measurements is exact.  Also the seeded synthetic recordings of the tests.

Differences of the two forms of `measures` on those recordings (`err32`, the largest |float32 form - float64 form| over a
sample-rate group's inputs: `tolerance`); the kernels are held to 4 x err32 of the group, measured when the test runs.
Measured with numpy 2.2 on a CPU over the cases of `GROUPS` below: 8 kHz 4.1e-05 (24 rows); 16 kHz 5.0e-05 (67 rows),
measure_duration 0.064 9.9e-07, one sample more 2.1e-06, boot_time 0 2.6e-05, float16 / bfloat16 / float64 inputs 3.6e-06 /
1.0e-04 / 3.4e-05, so 1.0e-04 for the group; 44.1 kHz 5.6e-05 (24 rows).  The value moves with the draw: it is set by
the quiet frames, where the noise-reduced spectrum is a difference of nearly equal numbers.
"""
import collections
import math

import numpy as np

Plan = collections.namedtuple("Plan", "L N P M gap fixed s0 s1 c0 c1 boot_max up down smooth trig nra level")

DEFAULTS = dict(trigger_level=7.0, trigger_time=0.25, search_time=1.0, allowed_gap=0.25, pre_trigger_time=0.0, boot_time=0.35,
                noise_up_time=0.1, noise_down_time=0.01, noise_reduction_amount=1.35, measure_freq=20.0, measure_duration=None,
                measure_smooth_time=0.4, hp_filter_freq=50.0, lp_filter_freq=6000.0, hp_lifter_freq=150.0, lp_lifter_freq=2000.0)


def plan(sample_rate, **kw):
    p = dict(DEFAULTS)
    p.update(kw)
    sr, mf = sample_rate, p["measure_freq"]
    md = 2.0 / mf if p["measure_duration"] is None else p["measure_duration"]
    L = int(sr * md + 0.5)
    N = 16
    while N < L:
        N *= 2
    s0 = max(int(p["hp_filter_freq"] / sr * N + 0.5), 1)
    s1 = min(int(p["lp_filter_freq"] / sr * N + 0.5), N // 2)
    c0 = math.ceil(sr * 0.5 / p["lp_lifter_freq"])
    c1 = min(math.floor(sr * 0.5 / p["hp_lifter_freq"]), N // 4)
    mult = lambda t: math.exp(-1.0 / (t * mf))      # noqa: E731
    return Plan(L=L, N=N, P=int(sr / mf + 0.5), M=math.ceil(p["search_time"] * mf), gap=int(p["allowed_gap"] * mf + 0.5),
                fixed=int(p["pre_trigger_time"] * sr + 0.5), s0=s0, s1=s1, c0=c0, c1=c1,
                boot_max=int(p["boot_time"] * mf - 0.5), up=mult(p["noise_up_time"]), down=mult(p["noise_down_time"]),
                smooth=mult(p["measure_smooth_time"]), trig=mult(p["trigger_time"]), nra=p["noise_reduction_amount"],
                level=p["trigger_level"])


def windows(pl):
    """(w, cw) in float64."""
    i = np.arange(pl.L, dtype=np.float64)
    w = 2.0 / math.sqrt(pl.L) * (0.5 - 0.5 * np.cos(2 * math.pi * i / pl.L))
    nb = pl.s1 - pl.s0
    k = np.arange(nb, dtype=np.float64)
    cw = 2.0 / math.sqrt(nb) * (0.5 - 0.5 * np.cos(2 * math.pi * k / nb))
    return w, cw


def n_frames(T, pl):
    return len(range(pl.L, T, pl.P))


def measures(x, sample_rate, dtype=np.float64, raw=False, **kw):
    """x: (rows, T) -> (rows, frames) of `dtype`'s measurements (float32 form: float32 values, as the kernels store them).
    raw=True: also the unclamped 21 + log(pw / (c1 - c0)) in float64 (-inf where pw <= 0, nan where pw is)."""
    pl = plan(sample_rate, **kw)
    dt = np.dtype(dtype).type
    x = np.asarray(x).astype(dt)
    rows, T = x.shape
    w, cw = (a.astype(dt) for a in windows(pl))
    F = n_frames(T, pl)
    nb = pl.s1 - pl.s0
    spec = np.zeros((rows, nb), dt)
    noise = np.zeros((rows, nb), dt)
    zeros = np.zeros((rows, nb), dt)
    out = np.zeros((rows, F), np.float64)
    unclamped = np.zeros((rows, F), np.float64)
    with np.errstate(all="ignore"):
        for f in range(F):
            pos = pl.L + f * pl.P
            buf = np.zeros((rows, pl.N), dt)
            buf[:, :pl.L] = x[:, pos - pl.L:pos] * w
            d = np.abs(np.fft.rfft(buf, axis=-1))[:, pl.s0:pl.s1].astype(dt)
            boot = f <= pl.boot_max
            mult = f / (1 + f) if boot else pl.smooth
            spec = spec * dt(mult) + d * dt(1 - mult)
            d2 = spec * spec
            m = zeros if boot else np.where(d2 > noise, dt(pl.up), dt(pl.down))
            noise = noise * m + d2 * (dt(1) - m)
            e = np.sqrt(np.maximum(zeros, d2 - dt(pl.nra) * noise))
            cb = np.zeros((rows, pl.N // 2), dt)
            cb[:, pl.s0:pl.s1] = e * cw
            c = np.fft.rfft(cb, axis=-1)[:, pl.c0:pl.c1]
            pw = np.sum((np.abs(c).astype(dt)) ** 2, axis=-1, dtype=dt)
            for r in range(rows):
                p = float(pw[r])
                u = 21 + math.log(p / (pl.c1 - pl.c0)) if p > 0 else (-math.inf if p == p else math.nan)
                unclamped[r, f] = u
                out[r, f] = max(0.0, u) if p > 0 else 0.0
    if dt is np.float32:
        out = out.astype(np.float32)
    return (out, unclamped) if raw else out


def first_frame(meas_row, pl):
    mean = 0.0
    for f, m in enumerate(meas_row):
        mean = mean * pl.trig + float(m) * (1 - pl.trig)
        if mean >= pl.level:
            return f
    return None


def flush_at(meas_row, f, pl):
    jT = jZ = pl.M
    for j in range(pl.M):
        v = float(meas_row[f - j]) if f - j >= 0 else 0.0
        if v >= pl.level and j <= jT + pl.gap:
            jZ = jT = j
        elif v == 0 and jT >= jZ:
            jZ = j
    return min(pl.M - 1, jZ)


def trigger_row(meas_row, pl):
    """(first, start) of one row: (-1, -1) where it never triggers."""
    f = first_frame(meas_row, pl)
    if f is None:
        return -1, -1
    return f, max(0, (f - flush_at(meas_row, f, pl)) * pl.P - pl.fixed)


def trigger_joint(meas, pl):
    """The common start of all rows as channels of one recording; -1 where none triggers."""
    firsts = [first_frame(row, pl) for row in meas]
    hit = [f for f in firsts if f is not None]
    if not hit:
        return -1
    f = min(hit)
    r0 = firsts.index(f)
    flush = max(flush_at(meas[r], f, pl) for r in range(r0, len(meas)))
    return max(0, (f - flush) * pl.P - pl.fixed)


def has_margin(meas_row, unclamped_row, pl, tol):
    """Whether a change of every measurement by up to `tol` leaves trigger_row(meas_row) as it is: the mean stays 2 tol from
    the level at every frame up to the trigger, and the ring's entries at the trigger frame stay 2 tol from the level and,
    unclamped, from 0."""
    mean, first = 0.0, None
    for f, m in enumerate(meas_row):
        mean = mean * pl.trig + float(m) * (1 - pl.trig)
        if abs(mean - pl.level) <= 2 * tol:
            return False
        if mean >= pl.level:
            first = f
            break
    if first is None:
        return True
    for j in range(pl.M):
        if first - j < 0:
            break
        if abs(float(meas_row[first - j]) - pl.level) <= 2 * tol or abs(float(unclamped_row[first - j])) <= 2 * tol:
            return False
    return True


# ---- seeded synthetic recordings ----------------------------------------------------------------------------------------------

def recording(seed, sample_rate, seconds, voiced):
    """A Gaussian floor of amplitude 10^[-3.5, -2.5] and, where voiced, a harmonic voice: f0 in 90-250 Hz, harmonics 1 / h
    below 4 kHz, amplitude 10^[-1, -0.3], 4 Hz amplitude modulation, starting after 0.6-1.4 s.  float32 (T,)."""
    rng = np.random.default_rng(seed)
    T = int(round(sample_rate * seconds))
    t = np.arange(T) / sample_rate
    x = 10.0 ** rng.uniform(-3.5, -2.5) * rng.standard_normal(T)
    f0, amp, onset = rng.uniform(90, 250), 10.0 ** rng.uniform(-1, -0.3), rng.uniform(0.6, 1.4)
    if voiced:
        v = np.zeros(T)
        h = 1
        while h * f0 < min(4000.0, sample_rate / 2):
            v += np.sin(2 * math.pi * h * f0 * t + rng.uniform(0, 2 * math.pi)) / h
            h += 1
        x += amp * v * (0.6 + 0.4 * np.sin(2 * math.pi * 4.0 * t)) * (t >= onset)
    return x.astype(np.float32)


def is_voiced(i):
    return i % 4 != 3


def batch(seed, sample_rate, seconds, rows):
    """(rows, T) float32: three rows in four voiced."""
    return np.stack([recording(1000 * seed + i, sample_rate, seconds, is_voiced(i)) for i in range(rows)])


# name -> (sample rate, seconds, rows, seed, parameters, input type): the measurement cases of the tests.  The cases of one
# sample rate form a group with one tolerance (`tolerance`).  Input type "f16" / "bf16": the samples are rounded to that type
# (the oracle is fed the values as the kernels widen them); "f64": the test perturbs them below half a float32 ulp.
GROUPS = {
    "8k": (8000, 3.0, 24, 1, {}, "f32"),                                   # L = 800, N = 1024, s1 clipped to N / 2
    "16k": (16000, 3.0, 67, 2, {}, "f32"),                                 # N = 2048; more rows than a wave has lanes
    "44k": (44100, 2.5, 24, 3, {}, "f32"),                                 # L = 4410, N = 8192
    "16k_md064": (16000, 3.0, 3, 4, dict(measure_duration=0.064), "f32"),   # L = N = 1024: no zero padding
    "16k_md064p": (16000, 3.0, 3, 5, dict(measure_duration=1025 / 16000), "f32"),   # L = 1025, N = 2048
    "16k_boot0": (16000, 3.0, 3, 6, dict(boot_time=0.0), "f32"),            # boot_max = 0
    "16k_f16": (16000, 3.0, 3, 7, {}, "f16"),
    "16k_bf16": (16000, 3.0, 3, 8, {}, "bf16"),
    "16k_f64": (16000, 3.0, 3, 9, {}, "f64"),
}
E2E = ("8k", "16k", "44k")       # the end-to-end cases: every row of these groups

_CACHE = {}


def _round_to(x, kind):
    if kind == "f16":
        return x.astype(np.float16).astype(np.float32)
    if kind == "bf16":                    # round to nearest even on the upper 16 bits
        u = x.view(np.uint32).astype(np.uint64)
        u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
        return u.astype(np.uint32).view(np.float32)
    return x


def group(name):
    """(x float32 (rows, T) in the compute type's values, sample rate, parameters, float64 measurements, unclamped float64,
    err32): computed once, read-only."""
    if name not in _CACHE:
        sr, seconds, rows, seed, kw, kind = GROUPS[name]
        x = _round_to(batch(seed, sr, seconds, rows), kind)
        m64, u64 = measures(x, sr, np.float64, raw=True, **kw)
        m32 = measures(x, sr, np.float32, **kw)
        err32 = float(np.max(np.abs(m32.astype(np.float64) - m64)))
        for a in (x, m64, u64, m32):
            a.setflags(write=False)
        _CACHE[name] = (x, sr, kw, m64, u64, err32, m32)
    return _CACHE[name][:6]


def group_m32(name):
    group(name)
    return _CACHE[name][6]


def tolerance(sample_rate):
    """4 x err32 of the sample-rate group: the largest difference of the oracle's two forms over all that rate's cases."""
    return 4.0 * max(group(n)[5] for n, g in GROUPS.items() if g[0] == sample_rate)
