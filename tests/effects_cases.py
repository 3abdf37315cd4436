"""Cases shared by tests/test_effects.py (CPU replay) and tests/test_gpu_effects.py: the parameter sets, the inputs and the
oracle's results.  All three effects are causal and their rows independent, so the oracle runs ONCE per (parameter set, compute
type) on the largest input and every smaller case is a corner of that result."""
import functools

import numpy as np
import torch

import effects_oracle as O

NP = {torch.float32: np.float32, torch.float64: np.float64, torch.float16: np.float32, torch.bfloat16: np.float32}

PHASER_SETS = {
    "L5": dict(sample_rate=1000, delay_ms=5.0, mod_speed=2.0),                                  # L = 5, M = 500
    "L1": dict(sample_rate=1000, delay_ms=1.0, mod_speed=2.0),                                  # the lag is 1 throughout
    "triangle": dict(sample_rate=2000, delay_ms=3.0, mod_speed=1.7, sinusoidal=False),
    "clamp": dict(sample_rate=1000, delay_ms=5.0, mod_speed=2.0, decay=0.95, gain_in=0.9, gain_out=1.0),
    # L = 300, M = 500: the float32 ring is in LDS, the float64 ring in the workspace
    "L300": dict(sample_rate=100000, delay_ms=3.0, mod_speed=200.0),
}
FLANGER_SETS = {
    "default": dict(sample_rate=1000),                                                          # L = 4, streaming route
    "quadratic": dict(sample_rate=1000, regen=-60.0, delay=3.0, depth=4.0, speed=3.3, phase=40.0, interpolation="quadratic"),
    "tight": dict(sample_rate=1000, regen=95.0, delay=0.0, depth=0.0),                          # L = 2, lag 0 throughout
    "triangular": dict(sample_rate=1500, regen=50.0, modulation="triangular", delay=30.0, depth=10.0, speed=10.0),
    # L = 708, N = 882: the ring does not fit the LDS in any type -- the workspace route
    "workspace": dict(sample_rate=44100, regen=30.0, delay=10.0, depth=6.0, speed=50.0),
    # regen = 0 with the quadratic tap that aliases onto the sample just written (k + 2 = L at the table's peak)
    "stream_quadratic": dict(sample_rate=1000, delay=1.0, depth=3.0, speed=2.5, interpolation="quadratic"),
}
OVERDRIVE_SETS = {
    "quiet": dict(amp=0.12, gain=20.0, colour=20.0),
    "loud": dict(amp=1.0, gain=20.0, colour=20.0),
    "unit": dict(amp=1.0, gain=0.0, colour=0.0),
}


def _phaser_plan_args(name):
    p = PHASER_SETS[name]
    return dict(sr=p["sample_rate"], delay_ms=p.get("delay_ms", 3.0), mod_speed=p.get("mod_speed", 0.5))


def _flanger_args(name):
    p = dict(FLANGER_SETS[name])
    p["sr"] = p.pop("sample_rate")
    return p


def _phaser_args(name):
    p = dict(PHASER_SETS[name])
    p["sr"] = p.pop("sample_rate")
    return p


def phaser_dims(name):
    return O.phaser_plan(**_phaser_plan_args(name))[:2]


def flanger_dims(name):
    p = _flanger_args(name)
    L, N = O.flanger_plan(p["sr"], 1, **{k: v for k, v in p.items() if k in ("delay", "depth", "regen", "width", "speed",
                                                                               "phase", "modulation")})[:2]
    return L, N


def lengths(L, S, M):
    """The issue's lengths: around the ring, around the tile, and where the table wraps."""
    return sorted({n for n in (1, 2, L - 1, L, L + 1, S - 1, S, S + 1, 2 * S + 3, M + 5, 2 * M + L + 1) if n >= 1})


@functools.lru_cache(maxsize=None)
def base_input(seed, amp, rows, T, dtype):
    """(rows, T) uniform in +-amp, stored in `dtype` (a CPU tensor that nobody writes to)."""
    gen = torch.Generator().manual_seed(seed)
    x = ((torch.rand(rows, T, generator=gen, dtype=torch.float64) * 2 - 1) * amp).to(dtype)
    assert not bool(((x == 0) & torch.signbit(x)).any())            # no -0.0
    return x


def compute_view(x):
    """The stored values in the compute type, as numpy."""
    return (x.float() if x.dtype in (torch.float16, torch.bfloat16) else x).numpy()


def stored(a, dtype):
    """An oracle result rounded once to the storage type (a CPU tensor)."""
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def bits(t):
    """A tensor's elements as integers, for equality bit for bit."""
    t = t.detach().cpu().contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


@functools.lru_cache(maxsize=None)
def phaser_ref(name, rows, T, dtype, seed=11):
    """(input, oracle result stored in dtype, share of clamped outputs)"""
    x = base_input(seed, 0.8, rows, T, dtype)
    xv, dt = compute_view(x), NP[dtype]
    p = _phaser_args(name)
    return x, stored(O.phaser(xv, dt=dt, **p), dtype), O.phaser_clamped_share(xv, dt=dt, **p)


@functools.lru_cache(maxsize=None)
def flanger_ref(name, B, C, T, dtype, seed=12):
    """(input (B, C, T), oracle result stored in dtype, share of clamped outputs)"""
    x = base_input(seed, 0.6, B * C, T, dtype).view(B, C, T)
    xv, dt = compute_view(x), NP[dtype]
    raw = O.flanger_unclamped(xv, dt=dt, **_flanger_args(name))
    return x, stored(np.clip(raw, -1, 1), dtype), float(np.mean(np.abs(raw) > 1))


@functools.lru_cache(maxsize=None)
def overdrive_ref(name, rows, T, dtype, seed=13):
    """(input, float64 oracle on the stored values, float32 sequential restatement, the float64 oracle's state y)"""
    p = OVERDRIVE_SETS[name]
    x = base_input(seed, p["amp"], rows, T, dtype)
    xv = compute_view(x)
    want, y = O.overdrive(xv.astype(np.float64), p["gain"], p["colour"], np.float64, return_state=True)
    ref32 = O.overdrive(xv.astype(np.float32), p["gain"], p["colour"], np.float32)
    return x, want, ref32.astype(np.float64), y


def half_ulp(want, dtype):
    """Half a unit in the last place of `dtype` at |want| (0 for float32 / float64: the bound is stated for them already)."""
    if dtype == torch.float16:
        e = np.floor(np.log2(np.maximum(np.abs(want), 2.0 ** -14)))
        return 0.5 * 2.0 ** (e - 10)
    if dtype == torch.bfloat16:
        e = np.floor(np.log2(np.maximum(np.abs(want), 2.0 ** -126)))
        return 0.5 * 2.0 ** (e - 7)
    return np.zeros_like(want)


def overdrive_bound(want, ref32, y, dtype):
    """The issue's tolerance for one case, computed from the case's own slices of the oracle's results.  float32:
    max(2 max|ref32 - want|, 4 * 2^-23) -- a float64-state scan should beat the reference's float32 loop, the factor covers the
    different rounding points of the pre-stage and the final mix; float64: 1000 * 2^-52 * max(1, max|y|) (200 from the 0.995
    contraction times 4 roundings a step, rounded up); half types: the float32 bound plus half an ulp of the output type."""
    if dtype == torch.float64:
        return np.full_like(want, 1000 * 2.0 ** -52 * max(1.0, float(np.abs(y).max(initial=0.0))))
    b32 = max(2 * float(np.abs(ref32 - want).max(initial=0.0)), 4 * 2.0 ** -23)
    return b32 + half_ulp(want, dtype)
