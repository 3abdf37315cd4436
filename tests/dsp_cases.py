"""The cases and checks that tests/test_dsp_synth.py (the CPU replay of csrc/dsp_synth.h) and tests/test_gpu_dsp_synth.py (the
product on the device) share.  A backend has tiles(), osc(f, a, sample_rate, reduction), fw(x, h), sinc(cutoff, window_size,
high_pass), fir(magnitudes) and pitch(base, pattern) over CPU torch tensors.  Every bar comes from the arithmetic the
definition fixes (tests/dsp_oracle.py and the issue's derivations), never from what a backend returns; each check returns the
largest fraction of its bar that was used, and prints it."""
import functools

import numpy as np
import torch

import dsp_oracle as O

SR = 16000.0
CH, TILE = 512, 1024                                   # dsp::kOscChunk, dsp::kFwTile: asserted against the backends' tiles()
DTYPES = {"f32": torch.float32, "f64": torch.float64, "f16": torch.float16, "bf16": torch.bfloat16}
EPS = {torch.float32: 2.0 ** -24, torch.float64: 2.0 ** -53}
OSC_T = (1, CH - 1, CH, CH + 1, 3 * CH + 5)
OSC_N = (1, 3, 64, 65)
FW_SHAPES = ((TILE + 3, 1, 1), (2 * TILE, 2, 5), (2 * TILE, 2 * TILE, 7), (3 * TILE, 6, 4), (TILE, 4, TILE + 1), (96, 3, 129))
SINC_W = (1, 3, 513, 1025)
SINC_CUT = (1e-3, 0.25, 1.0)
FIR_N = (2, 3, 129, 513)


def wide(t: torch.Tensor) -> np.ndarray:
    """The values of `t` as numpy: float64 stays, everything else is widened (exactly) to float32."""
    return t.numpy() if t.dtype == torch.float64 else t.float().numpy()


def half_ulp(v: np.ndarray, dtype) -> np.ndarray:
    """Half a unit in the last place of float16 / bfloat16 at |v| (0 for the wide types)."""
    if dtype not in (torch.float16, torch.bfloat16):
        return np.zeros_like(v, dtype=np.float64)
    bits, emin = (10, -14) if dtype == torch.float16 else (7, -126)
    e = np.floor(np.log2(np.maximum(np.abs(v).astype(np.float64), 2.0 ** emin)))
    return 0.5 * 2.0 ** (np.maximum(e, emin) - bits)


def used(err, bar, what):
    err, bar = np.asarray(err, np.float64), np.asarray(bar, np.float64)
    ok = err <= bar
    frac = float(np.max(np.where(bar > 0, err / np.where(bar > 0, bar, 1.0), np.where(err > 0, np.inf, 0.0)))) if err.size else 0.0
    print(f"{what}: {frac:.3f} of the bar")
    assert ok.all(), f"{what}: {frac:.3f} of the bar at worst, {int((~ok).sum())} of {ok.size} outside"
    return frac


# ---- oscillator_bank -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def osc_inputs(rows, T, N, dt, seed=0):
    rng = np.random.default_rng(1000 * seed + 7 * T + N)
    f = rng.uniform(-0.55 * SR, 0.55 * SR, (rows, T, N))
    a = rng.uniform(-1.0, 1.0, (rows, T, N))
    return torch.from_numpy(f).to(DTYPES[dt]), torch.from_numpy(a).to(DTYPES[dt])


@functools.lru_cache(maxsize=None)
def osc_oracle(rows, T, N, dt, reduction, seed=0):
    """(float64 result, sum |a'|, the float64 oracle's largest distance from its longdouble form)."""
    f, a = osc_inputs(rows, T, N, dt, seed)
    want, mag = O.oscillator_bank(wide(f), wide(a), SR, reduction)
    own = 0.0
    if dt == "f64":
        ld, _ = O.oscillator_bank(wide(f), wide(a), SR, reduction, acc=O.LD)
        own = float(np.abs(want - ld).max())
    return want, mag, own


def osc_bar(want, mag, own, N, dt, reduction):
    n = 1 if reduction == "none" else N
    if dt == "f64":
        return np.maximum(4.0 * own, 8.0 * 2.0 ** -53 * mag)
    bar = (n + 8) * 2.0 ** -24 * mag                      # for "mean" `mag` is already divided by N
    if reduction == "mean":
        bar = bar + 2.0 ** -24 * np.abs(want)             # the division's rounding
    return bar + half_ulp(np.abs(want) + bar, DTYPES[dt])


def check_osc(B, rows, T, N, dt, reduction="sum", seed=0):
    f, a = osc_inputs(rows, T, N, dt, seed)
    got = B.osc(f, a, SR, reduction)
    assert got.dtype == DTYPES[dt] and tuple(got.shape) == ((rows, T, N) if reduction == "none" else (rows, T))
    want, mag, own = osc_oracle(rows, T, N, dt, reduction, seed)
    return used(np.abs(got.double().numpy() - want), osc_bar(want, mag, own, N, dt, reduction), f"oscillator_bank {dt} T={T} N={N} {reduction}")


def check_osc_prefix(B, dt):
    f, a = osc_inputs(2, 3 * CH + 5, 3, dt)
    whole = B.osc(f, a, SR, "sum")
    for T1 in (1, CH - 1, CH + 1, 2 * CH):
        assert torch.equal(B.osc(f[:, :T1].contiguous(), a[:, :T1].contiguous(), SR, "sum"), whole[:, :T1])


def check_osc_rows(B, dt):
    f, a = osc_inputs(2, CH + 1, 65, dt)
    both = B.osc(f, a, SR, "sum")
    assert torch.equal(B.osc(f, a, SR, "sum"), both)
    for b in range(2):
        assert torch.equal(B.osc(f[b:b + 1].contiguous(), a[b:b + 1].contiguous(), SR, "sum")[0], both[b])
    assert not torch.equal(both[0], both[1])


def check_osc_poison(B, dt):
    T, N, t_nan, t_inf = CH + 40, 3, CH - 3, 17
    f, a = (t.clone() for t in osc_inputs(2, T, N, dt))
    clean = B.osc(f, a, SR, "none")
    f[0, t_nan, 1] = float("nan")
    f[1, t_inf, 2] = float("inf")
    got = B.osc(f, a, SR, "none")
    bad = torch.zeros(2, T, N, dtype=torch.bool)
    bad[0, t_nan:, 1] = True
    bad[1, t_inf:, 2] = True
    assert torch.isnan(got[bad]).all()
    assert torch.equal(got[~bad], clean[~bad])                           # the other oscillators keep their bits
    s = B.osc(f, a, SR, "sum")
    assert torch.isnan(s[0, t_nan:]).all() and torch.isnan(s[1, t_inf:]).all()
    assert torch.equal(s[0, :t_nan], B.osc(*osc_inputs(2, T, N, dt), SR, "sum")[0, :t_nan])


# ---- filter_waveform -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fw_inputs(T, F, L, dt, batched, rows=2):
    rng = np.random.default_rng(31 * T + 7 * F + L + (1 if batched else 0))
    x = rng.standard_normal((rows, T))
    h = rng.standard_normal((rows, F, L) if batched else (F, L)) / np.sqrt(L)
    return torch.from_numpy(x).to(DTYPES[dt]), torch.from_numpy(h).to(DTYPES[dt])


@functools.lru_cache(maxsize=None)
def fw_oracle(T, F, L, dt, batched, rows=2):
    x, h = fw_inputs(T, F, L, dt, batched, rows)
    return O.filter_waveform(wide(x), wide(h))


def fw_bar(want, mag, L, dt):
    eps = 2.0 ** -53 if dt == "f64" else 2.0 ** -24
    bar = (L + 2) * eps * mag
    return bar + half_ulp(np.abs(want) + bar, DTYPES[dt])


def check_fw(B, T, F, L, dt, batched):
    x, h = fw_inputs(T, F, L, dt, batched)
    got = B.fw(x, h)
    assert got.dtype == DTYPES[dt] and got.shape == x.shape
    want, mag = fw_oracle(T, F, L, dt, batched)
    return used(np.abs(got.double().numpy() - want), fw_bar(want, mag, L, dt), f"filter_waveform {dt} T={T} F={F} L={L} {'3-D' if batched else '2-D'}")


def check_fw_shared_equals_expanded(B, dt):
    for T, F, L in ((2 * TILE, 2, 5), (2 * TILE, 2 * TILE, 7), (96, 3, 129)):
        x, h = fw_inputs(T, F, L, dt, False)
        assert torch.equal(B.fw(x, h), B.fw(x, h[None].expand(2, F, L).contiguous()))


def check_fw_rows(B, dt):
    x, h = fw_inputs(3 * TILE, 6, 4, dt, True)
    both = B.fw(x, h)
    assert torch.equal(B.fw(x, h), both)
    for b in range(2):
        assert torch.equal(B.fw(x[b:b + 1].contiguous(), h[b:b + 1].contiguous())[0], both[b])


def check_fw_nonfinite_stays_under_its_filter(B):
    T, F, L = TILE + 3, 1, 5
    x, h = (t.clone() for t in fw_inputs(T, F, L, "f32", False, rows=1))
    clean = B.fw(x, h)
    x[0, 700] = float("inf")
    got = B.fw(x, h)
    d = (L - 1) // 2
    hit = torch.zeros(1, T, dtype=torch.bool)
    hit[0, 700 - d:700 - d + L] = True                                    # n = m - d + j, 0 <= j < L
    assert not torch.isfinite(got[hit]).any() and torch.equal(got[~hit], clean[~hit])


# ---- the designers and extend_pitch ----------------------------------------------------------------------------------------
def check_sinc(B, W, high_pass, dt):
    cut = torch.tensor(SINC_CUT, dtype=DTYPES[dt])
    got = B.sinc(cut, W, high_pass)
    assert got.dtype == DTYPES[dt] and tuple(got.shape) == (len(SINC_CUT), W)
    o64 = O.sinc_impulse_response(wide(cut), W, high_pass)
    old = O.sinc_impulse_response(wide(cut), W, high_pass, acc=O.LD)
    if dt == "f32":
        # One ulp of the float64 oracle rounded to float32 at every tap.  One tap gets more: with cutoff = 1 and high_pass the
        # centre is 1 - g / |sum g| with g / |sum g| = 1 - O(1e-16), so the definition evaluated in float64 yields rounding
        # noise of the size of an ulp of 1 there (the oracle gives 2.2e-16 where longdouble gives -3.3e-19), and no
        # evaluation in float64 is within a float32 ulp of another one's noise.  At that tap alone the bar also takes 4 x
        # the float64 oracle's own distance from its longdouble form.
        o32 = o64.astype(np.float32)
        bar = np.spacing(np.abs(o32)).astype(np.float64)
        if high_pass:
            for r, c in enumerate(SINC_CUT):
                if c == 1.0:
                    bar[r, W // 2] += 4.0 * float(np.abs(o64[r, W // 2] - old[r, W // 2]))
        return used(np.abs(got.numpy().astype(np.float64) - o32), bar, f"sinc f32 W={W} hp={high_pass}")
    bar = np.maximum(4.0 * float(np.abs(o64 - old).max()), 4.0 * np.spacing(np.abs(o64).max(axis=-1, keepdims=True)))
    return used(np.abs(got.numpy() - o64), np.broadcast_to(bar, o64.shape), f"sinc f64 W={W} hp={high_pass}")


def check_sinc_batch(B, dt):
    cut = torch.tensor([[0.1, 0.2, 0.3], [0.4, 0.5, 0.6]], dtype=DTYPES[dt])
    got = B.sinc(cut, 9, False)
    assert tuple(got.shape) == (2, 3, 9)
    for i in range(2):
        for j in range(3):
            assert torch.equal(got[i, j], B.sinc(cut[i, j].reshape(1), 9, False)[0])
    assert np.allclose(got.double().numpy().sum(-1), 1.0, atol=1e-6)


def check_fir(B, n, dt):
    rng = np.random.default_rng(n)
    m = torch.from_numpy(rng.uniform(0.0, 1.0, (2, n))).to(DTYPES[dt])
    got = B.fir(m)
    assert got.dtype == DTYPES[dt] and tuple(got.shape) == (2, 2 * (n - 1))
    want, mag = O.frequency_impulse_response(wide(m))
    return used(np.abs(got.double().numpy() - want), (n + 4) * EPS[DTYPES[dt]] * mag, f"frequency_impulse_response {dt} n={n}")


def check_pitch(B, dt):
    rng = np.random.default_rng(3)
    base = torch.from_numpy(rng.uniform(50.0, 500.0, (2, 301, 1))).to(DTYPES[dt])
    pat = torch.from_numpy(np.array([1.0, 2.0, 3.0009765625, 4.5, 7.123])).to(DTYPES[dt])
    got = B.pitch(base, pat)
    assert got.dtype == DTYPES[dt] and tuple(got.shape) == (2, 301, 5)
    want = O.extend_pitch(wide(base), wide(pat))                           # the wide product, rounded once more for the half types
    assert torch.equal(got, torch.from_numpy(want).to(DTYPES[dt]))
