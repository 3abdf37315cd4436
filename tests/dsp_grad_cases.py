"""The cases and checks that tests/test_dsp_grad.py (the CPU replay of csrc/dsp_synth_grad.h) and tests/test_gpu_dsp_grad.py (the
product on the device, through autograd) share.  A backend has grad_tiles(), osc_grad(f, a, g, sample_rate, reduction,
want=(True, True)) -> (gf, ga) and fw_grad(x, h, g, want=(True, True)) -> (gx, gh) over CPU torch tensors (an unwanted gradient
is None).  Every bar comes from the arithmetic (the derivations are beside each one), never from what a backend returns; each
check goes through dsp_cases.used, which prints the share of the bar that was used."""
import functools

import numpy as np
import torch

import dsp_cases as K
import dsp_grad_oracle as G

SR, CH, TILE, DTYPES = K.SR, K.CH, K.TILE, K.DTYPES
PIECE, LAGS = 1024, 256                                # dsp::kGhPiece, kGhLags: asserted against the backends' grad_tiles()
# the forward's shapes; one chunk length below, at ((2 TILE, 2, 5) above) and above the piece; one tap count below, at and above
# the lag tile; chunks that do not fill the last unit (7 chunks of 300 samples, 3 to a unit)
FW_GRAD_SHAPES = K.FW_SHAPES + ((2 * PIECE - 2, 2, 5), (2 * PIECE + 2, 2, 5), (96, 3, LAGS - 1), (96, 3, LAGS), (96, 3, LAGS + 1),
                                (2100, 7, 3))
FW_ONE_FILTER = (TILE + 3, 1, 1)                       # with rows = 3: the fold over rows has more than two terms


def eps_of(dt):
    return 2.0 ** -53 if dt == "f64" else 2.0 ** -24


# ---- oscillator_bank -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def osc_cotangent(rows, T, N, dt, reduction):
    rng = np.random.default_rng(5 * T + N + 77)
    g = rng.standard_normal((rows, T, N) if reduction == "none" else (rows, T))
    return torch.from_numpy(g).to(DTYPES[dt])


@functools.lru_cache(maxsize=None)
def osc_grad_oracle(rows, T, N, dt, reduction):
    """(gf, ga, |g|, M, own distance of gf, own distance of ga): `own` is the float64 oracle's largest distance from its
    longdouble form (float64 cases only, the convention of dsp_cases.osc_bar)."""
    f, a = K.osc_inputs(rows, T, N, dt)
    g = osc_cotangent(rows, T, N, dt, reduction)
    gf, ga, gmag, M = G.oscillator_bank_grad(K.wide(f), K.wide(a), K.wide(g), SR, reduction)
    own_f = own_a = 0.0
    if dt == "f64":
        lf, la, _, _ = G.oscillator_bank_grad(K.wide(f), K.wide(a), K.wide(g), SR, reduction, acc=G.LD)
        own_f, own_a = float(np.abs(gf - lf).max()), float(np.abs(ga - la).max())
    return gf, ga, gmag, M, own_f, own_a


def ga_bar(want, gmag, own, dt, reduction):
    """float32: the phase is rounded once to float32 (|phi| <= pi: at most 2 * 2^-24, times |cos| <= 1), sin() and the product
    round: the per-oscillator term (1 + 8) 2^-24 |g| of dsp_cases.osc_bar; "mean" divides g by N first (gmag holds |g| / N)
    and that division rounds once.  float64: the oracle's own distance from longdouble, as osc_bar."""
    if dt == "f64":
        return np.maximum(4.0 * own, 8.0 * 2.0 ** -53 * gmag)
    bar = (1 + 8) * 2.0 ** -24 * gmag
    if reduction == "mean":
        bar = bar + 2.0 ** -24 * np.abs(want)
    return bar + K.half_ulp(np.abs(want) + bar, DTYPES[dt])


def gf_bar(want, M, own, T, dt):
    """Every term g a' cos(phi) carries the per-oscillator error of osc_bar, 9 * 2^-24 of |g a'|, and the sum is float64 (its own
    error is 2^-53-sized): 9 * 2^-24 M with M the total over the ROW, not over the suffix, so that a lane may form its suffix as
    a total minus a running prefix; the scale and the rounding to float32 add 2 * 2^-24 |want|.  float64: T float64 additions
    of terms within 8 * 2^-53 each, or the oracle's own distance from longdouble."""
    if dt == "f64":
        return np.maximum(4.0 * own, (T + 8) * 2.0 ** -53 * M) + np.zeros_like(want)
    bar = 9 * 2.0 ** -24 * M + 2 * 2.0 ** -24 * np.abs(want)
    return bar + K.half_ulp(np.abs(want) + bar, DTYPES[dt])


def check_osc_grad(B, rows, T, N, dt, reduction="sum"):
    f, a = K.osc_inputs(rows, T, N, dt)
    g = osc_cotangent(rows, T, N, dt, reduction)
    gf, ga = B.osc_grad(f, a, g, SR, reduction)
    assert gf.dtype == ga.dtype == DTYPES[dt] and tuple(gf.shape) == tuple(ga.shape) == (rows, T, N)
    wf, wa, gmag, M, own_f, own_a = osc_grad_oracle(rows, T, N, dt, reduction)
    what = f"oscillator_bank {dt} T={T} N={N} {reduction}"
    dead = (f.abs() >= SR / 2).numpy()
    assert dead.any() or T == 1                        # osc_inputs reaches 0.55 sample_rate: some oscillators are dead
    assert (ga.double().numpy()[dead] == 0).all(), "a dead oscillator has a zero amplitude gradient, exactly"
    return (K.used(np.abs(ga.double().numpy() - wa), ga_bar(wa, gmag, own_a, dt, reduction), "grad_amplitudes of " + what),
            K.used(np.abs(gf.double().numpy() - wf), gf_bar(wf, M, own_f, T, dt), "grad_frequencies of " + what))


def check_osc_grad_prefix(B, dt):
    T = 3 * CH + 5
    f, a = K.osc_inputs(2, T, 3, dt)
    g = osc_cotangent(2, T, 3, dt, "sum")
    _, whole = B.osc_grad(f, a, g, SR, "sum", want=(False, True))
    for T1 in (1, CH - 1, CH + 1, 2 * CH):
        _, ga = B.osc_grad(f[:, :T1].contiguous(), a[:, :T1].contiguous(), g[:, :T1].contiguous(), SR, "sum", want=(False, True))
        assert torch.equal(ga, whole[:, :T1])


def check_osc_grad_rows(B, dt):
    for N, red in ((65, "sum"), (3, "none")):
        f, a = K.osc_inputs(2, CH + 1, N, dt)
        g = osc_cotangent(2, CH + 1, N, dt, red)
        gf, ga = B.osc_grad(f, a, g, SR, red)
        again = B.osc_grad(f, a, g, SR, red)
        assert torch.equal(again[0], gf) and torch.equal(again[1], ga)
        for b in range(2):
            one = B.osc_grad(f[b:b + 1].contiguous(), a[b:b + 1].contiguous(), g[b:b + 1].contiguous(), SR, red)
            assert torch.equal(one[0][0], gf[b]) and torch.equal(one[1][0], ga[b])
        assert not torch.equal(gf[0], gf[1])


def check_osc_grad_poison(B, dt):
    T, N, t_nan, t_inf = CH + 40, 3, CH - 3, 17
    f, a = (t.clone() for t in K.osc_inputs(2, T, N, dt))
    g = osc_cotangent(2, T, N, dt, "sum")
    clean_f, clean_a = B.osc_grad(f, a, g, SR, "sum")
    assert torch.isfinite(clean_f).all() and torch.isfinite(clean_a).all()
    f[0, t_nan, 1] = float("nan")
    f[1, t_inf, 2] = float("inf")
    gf, ga = B.osc_grad(f, a, g, SR, "sum")
    bad_f = torch.zeros(2, T, N, dtype=torch.bool)
    bad_f[0, :, 1] = True                                              # the whole column: every suffix holds the poisoned steps
    bad_f[1, :, 2] = True
    bad_a = torch.zeros(2, T, N, dtype=torch.bool)
    bad_a[0, t_nan:, 1] = True
    bad_a[1, t_inf:, 2] = True
    assert torch.isnan(gf[bad_f]).all() and torch.isnan(ga[bad_a]).all()
    assert torch.equal(gf[~bad_f], clean_f[~bad_f]) and torch.equal(ga[~bad_a], clean_a[~bad_a])


# ---- filter_waveform -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fw_cotangent(T, dt, rows=2):
    return torch.from_numpy(np.random.default_rng(13 * T + rows).standard_normal((rows, T))).to(DTYPES[dt])


@functools.lru_cache(maxsize=None)
def fw_grad_oracle(T, F, L, dt, batched, rows=2):
    x, h = K.fw_inputs(T, F, L, dt, batched, rows)
    return G.filter_waveform_grad(K.wide(x), K.wide(h), K.wide(fw_cotangent(T, dt, rows)))


def gx_bar(want, mag, L, dt):
    """One fused multiply-add chain of L terms in the compute type, as dsp_cases.fw_bar."""
    bar = (L + 2) * eps_of(dt) * mag
    return bar + K.half_ulp(np.abs(want) + bar, DTYPES[dt])


def gh_bar(want, mag, terms, dt):
    """A float64 sum of `terms` products (exact in float64 for the narrow types; rounded once for float64) in any fixed order:
    (terms + 2) 2^-53 sum |x||g|; then one rounding to float32 (the half types round again: half_ulp)."""
    eps_out = 0.0 if dt == "f64" else 2.0 ** -24
    bar = eps_out * np.abs(want) + (terms + 2) * 2.0 ** -53 * mag
    return bar + K.half_ulp(np.abs(want) + bar, DTYPES[dt])


def check_fw_grad(B, T, F, L, dt, batched, rows=2):
    x, h = K.fw_inputs(T, F, L, dt, batched, rows)
    g = fw_cotangent(T, dt, rows)
    gx, gh = B.fw_grad(x, h, g)
    assert gx.dtype == gh.dtype == DTYPES[dt] and gx.shape == x.shape and gh.shape == h.shape
    wx, mx, wh, mh, terms = fw_grad_oracle(T, F, L, dt, batched, rows)
    what = f"filter_waveform {dt} rows={rows} T={T} F={F} L={L} {'3-D' if batched else '2-D'}"
    return (K.used(np.abs(gx.double().numpy() - wx), gx_bar(wx, mx, L, dt), "grad_waveform of " + what),
            K.used(np.abs(gh.double().numpy() - wh), gh_bar(wh, mh, terms, dt), "grad_kernels of " + what))


def check_fw_grad_exact(B, dt):
    for T, F, L in ((2 * TILE, 2, 5), (2 * TILE, 2 * TILE, 7), (96, 3, 129), (2 * PIECE + 2, 2, 5)):
        g = fw_cotangent(T, dt)
        x, h = K.fw_inputs(T, F, L, dt, False)
        gx, gh = B.fw_grad(x, h, g)
        again = B.fw_grad(x, h, g)
        assert torch.equal(again[0], gx) and torch.equal(again[1], gh)                    # no atomics
        wide = h[None].expand(2, F, L).contiguous()
        assert torch.equal(B.fw_grad(x, wide, g, want=(True, False))[0], gx)              # shared against expanded filters
        _, gh_one = B.fw_grad(x[:1].contiguous(), h, g[:1].contiguous(), want=(False, True))
        _, gh_set = B.fw_grad(x[:1].contiguous(), wide[:1].contiguous(), g[:1].contiguous(), want=(False, True))
        assert torch.equal(gh_one, gh_set[0])                                             # one row: shared is batched[0]
        x, h = K.fw_inputs(T, F, L, dt, True)
        gx, gh = B.fw_grad(x, h, g)
        for b in range(2):
            one = B.fw_grad(x[b:b + 1].contiguous(), h[b:b + 1].contiguous(), g[b:b + 1].contiguous())
            assert torch.equal(one[0][0], gx[b]) and torch.equal(one[1][0], gh[b])        # a row of a batch


def check_fw_grad_nonfinite_stays_under_its_filter(B):
    T, F, L, n = TILE + 3, 1, 5, 700
    x, h = K.fw_inputs(T, F, L, "f32", False, rows=1)
    g = fw_cotangent(T, "f32", rows=1).clone()
    clean, _ = B.fw_grad(x, h, g, want=(True, False))
    g[0, n] = float("inf")
    got, _ = B.fw_grad(x, h, g, want=(True, False))
    d = (L - 1) // 2
    hit = torch.zeros(1, T, dtype=torch.bool)
    hit[0, n + d - L + 1:n + d + 1] = True                                 # n - m + d in [0, L)
    assert not torch.isfinite(got[hit]).any() and torch.equal(got[~hit], clean[~hit])


def check_only_what_is_wanted(B):
    f, a = K.osc_inputs(2, CH + 1, 3, "f32")
    g = osc_cotangent(2, CH + 1, 3, "f32", "sum")
    gf, ga = B.osc_grad(f, a, g, SR, "sum")
    only_f, none_a = B.osc_grad(f, a, g, SR, "sum", want=(True, False))
    none_f, only_a = B.osc_grad(f, a, g, SR, "sum", want=(False, True))
    assert none_a is None and none_f is None and torch.equal(only_f, gf) and torch.equal(only_a, ga)
    x, h = K.fw_inputs(3 * TILE, 6, 4, "f32", False)
    g = fw_cotangent(3 * TILE, "f32")
    gx, gh = B.fw_grad(x, h, g)
    only_x, none_h = B.fw_grad(x, h, g, want=(True, False))
    none_x, only_h = B.fw_grad(x, h, g, want=(False, True))
    assert none_h is None and none_x is None and torch.equal(only_x, gx) and torch.equal(only_h, gh)
