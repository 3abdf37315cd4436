"""The cases and bars that tests/test_spectral_point.py (CPU replay of the kernels) and tests/test_gpu_spectral_point.py (the
C ABI on the device) share.  A backend has two methods over torch CPU tensors:

    pointwise(op, x, out_dtype, p0, p1, flag, table, n_in, n_out) -> (rows, L) tensor; x is a (rows, L) view with unit
        stride along L (its row stride and storage offset are kept: the device backend copies the whole base)
    centroid(m3, freqs, out_dtype) -> (rows, frames) tensor; m3 is a float32 (rows, frames, n_freq) view with any strides

Every bar comes from tests/spectral_point_oracle.py."""
import math

import numpy as np
import torch

import spectral_point_oracle as O

SCALE, CONTRAST, DB_TO_AMP, MU_ENCODE, MU_DECODE, FADE = range(6)
LENGTHS = (0, 1, 3, 4, 5, 1023, 1025)
LAYOUTS = ("dense", "stride", "offset")
FLOATS = (torch.float32, torch.float64, torch.float16, torch.bfloat16)
NP = {torch.float32: np.float32, torch.float64: np.float64}


def rows_view(values: np.ndarray, dtype, layout: str) -> torch.Tensor:
    """float64 (rows, L) values rounded once to `dtype`, stored as rows of a wider buffer: "dense" L elements apart at offset
    0, "stride" L + 3 apart, "offset" L + 3 apart from element 1 (rows that do not start on 16 bytes)."""
    rows, L = values.shape
    stride = L if layout == "dense" else L + 3
    off = 1 if layout == "offset" else 0
    base = torch.zeros(off + rows * stride + 4, dtype=dtype)
    view = base.as_strided((rows, L), (stride, 1), off)
    view.copy_(O.round_to(values, dtype) if dtype in FLOATS else torch.from_numpy(values.astype(np.int64)).to(dtype))
    return view


def f64(t: torch.Tensor) -> np.ndarray:
    return t.double().numpy() if t.is_floating_point() else t.to(torch.int64).numpy().astype(np.float64)


def compute_np(t: torch.Tensor):
    """The values of `t` in its compute precision (float16 / bfloat16 / integers: float32) and that numpy type."""
    dt = NP.get(t.dtype, np.float32)
    return f64(t).astype(dt), dt


def assert_same_bits(got: torch.Tensor, want: torch.Tensor, what=""):
    """Bit for bit, except that any NaN equals any NaN."""
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if not got.is_floating_point():
        assert torch.equal(got, want), what
        return
    g, w = got.double().numpy(), want.double().numpy()
    assert np.array_equal(np.isnan(g), np.isnan(w)), what
    ok = ~np.isnan(w)
    assert np.array_equal(g[ok], w[ok]) and np.array_equal(np.signbit(g[ok]), np.signbit(w[ok])), \
        (what, np.flatnonzero(g[ok] != w[ok])[:5])


def signal(rng, rows, L, lo=-1.0, hi=1.0, specials=False):
    x = rng.uniform(lo, hi, (rows, L))
    if specials and L >= 5:
        x[0, 0], x[0, 1], x[-1, 2], x[-1, 3] = -0.0, np.nan, np.inf, 0.0
    return x


# ---- scale: gain and the three Vol modes, bit-exact ----------------------------------------------------------------------------
SCALE_MODES = {"gain": (O.ratio_of_db(-3.7), 0), "vol_amplitude": (0.7, 1), "vol_db": (O.ratio_of_db(6.0), 1),
               "vol_power": (O.ratio_of_db(10 * math.log10(0.3)), 1), "vol_amplitude_up": (1.9, 1)}


def check_scale(B, dtype, L, layout, seed=0):
    rng = np.random.default_rng(seed + L)
    x = rows_view(signal(rng, 3, L, -2.0, 2.0, specials=True), dtype, layout)
    xc, dt = compute_np(x)
    for name, (ratio, clamp) in SCALE_MODES.items():
        got = B.pointwise(SCALE, x, dtype, ratio, 0.0, clamp, None, 0, 0)
        with np.errstate(invalid="ignore"):
            want = O.scale(xc, ratio, clamp, dt)
        assert_same_bits(got, O.round_to(want.astype(np.float64), dtype), (name, dtype, L, layout))


# ---- fade -------------------------------------------------------------------------------------------------------------------------
def fade_lengths(L):
    """(fade_in_len, fade_out_len): each of {0, 1, L}, and a pair that overlaps."""
    out = {(0, 0), (1, 0), (0, 1), (L, 0), (0, L), (1, 1) if L >= 1 else (0, 0), (L, L)}
    if L >= 4:
        out |= {(L // 2 + 1, L // 2 + 1), (3, 2)}
    return sorted(p for p in out if p[0] <= L and p[1] <= L)


def check_fade(B, dtype, L, layout, shape, seed=0):
    rng = np.random.default_rng(seed + L)
    for n_in, n_out in fade_lengths(L):
        vals = signal(rng, 3, L, -1.5, 1.5)
        if L - n_in - n_out >= 3:                         # specials outside the ramps: their bits must come through
            vals[:, n_in], vals[:, n_in + 1], vals[:, n_in + 2] = -0.0, np.nan, -np.inf
        x = rows_view(vals, dtype, layout)
        fi, fo = O.fade_ramps(n_in, n_out, shape)
        table = O.round_to(np.concatenate([fi, fo]), dtype)
        got = B.pointwise(FADE, x, dtype, 0.0, 0.0, 0, table if n_in + n_out else None, n_in, n_out)
        assert got.dtype == dtype and tuple(got.shape) == (3, L)
        xc, dt = compute_np(x)
        tc = f64(table).astype(dt)
        i = np.arange(L)
        a = np.where(i < n_in, tc[np.minimum(i, max(n_in - 1, 0))] if n_in else dt(1), dt(1)).astype(dt)
        b = np.where(i >= L - n_out, tc[n_in + np.clip(i - (L - n_out), 0, max(n_out - 1, 0))] if n_out else dt(1), dt(1)).astype(dt)
        inside = torch.from_numpy((i < n_in) | (i >= L - n_out))
        with np.errstate(invalid="ignore"):
            want = O.round_to((((a * b).astype(dt))[None, :] * xc).astype(np.float64), dtype)
        what = (dtype, L, layout, shape, n_in, n_out)
        assert_same_bits(got[:, inside], want[:, inside], what)
        bits = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[x.element_size()]
        assert torch.equal(got[:, ~inside].contiguous().view(bits), x[:, ~inside].contiguous().view(bits)), what


# ---- contrast, DB_to_amplitude, mu_law_decoding: 4 x the definition's own error one precision down ------------------------------
def _wider(dt):
    """(the precision the yardstick is evaluated in, the one it is held against)"""
    if dt == np.float32:
        return np.float32, np.float64
    if np.finfo(np.longdouble).eps < np.finfo(np.float64).eps:
        return np.float64, np.longdouble
    return None, None


def check_accuracy(B, op, views, out_dtype, fn, args, p0, p1, relative, what):
    """`fn(values, *args, dt)` is the oracle's expression; `views` are the inputs of one group (every length of a case).  The
    yardstick -- the largest error of the expression's own evaluation one precision down -- is measured here, on the group's
    inputs pooled: a maximum over the three samples of an L = 1 case says nothing about the evaluation's error, which is why
    the bar belongs to the group and not to each length (the rule tests/vad_cases.py uses per sample-rate group)."""
    worst, yard = 0.0, 0.0
    for x in views:
        xc, dt = compute_np(x)
        got = B.pointwise(op, x, out_dtype, p0, p1, 0, None, 0, 0)
        assert got.dtype == out_dtype and got.shape == x.shape, what
        if x.numel() == 0:
            continue
        low, high = _wider(dt)
        if low is None:                                  # no type wider than float64 here: float32's yardstick, scaled
            ref = fn(xc.astype(np.float64), *args, np.float64)
            yard_err = np.abs(fn(xc.astype(np.float32), *args, np.float32).astype(np.float64) - ref) * 2.0 ** -29
        else:
            ref = fn(xc.astype(high), *args, high)
            yard_err = np.abs(fn(xc.astype(low), *args, low).astype(high) - ref).astype(np.float64)
        ref = ref.astype(np.float64)
        err = np.abs(got.double().numpy() - ref) - O.half_ulp(ref, out_dtype)      # beyond the one rounding of a half result
        if relative:
            scale = np.maximum(np.abs(ref), np.finfo(np.float64).tiny)
            err, yard_err = err / scale, yard_err / scale
        worst, yard = max(worst, float(err.max())), max(yard, float(yard_err.max()))
    print("%s: yardstick %.3e, largest error beyond the output rounding %.3e (%.2f of the bar)"
          % (what, yard, worst, worst / (4 * yard) if yard else float("nan")))
    assert yard > 0 and worst <= 4 * yard, (what, worst, yard)
    return worst, yard


ACCURACY_LENGTHS = LENGTHS + (4099,)


def check_contrast(B, dtype, layout, lengths=ACCURACY_LENGTHS, amount=75.0):
    views = [rows_view(signal(np.random.default_rng(11 + L), 3, L), dtype, layout) for L in lengths]
    return check_accuracy(B, CONTRAST, views, dtype, O.contrast, (amount,), math.pi / 2, amount / 750.0, False,
                          ("contrast", dtype, layout, amount))


def check_db_to_amplitude(B, dtype, layout, lengths=ACCURACY_LENGTHS, ref=1.0, power=0.5):
    views = [rows_view(signal(np.random.default_rng(12 + L), 3, L, -40.0, 20.0), dtype, layout) for L in lengths]
    return check_accuracy(B, DB_TO_AMP, views, dtype, lambda v, r, p, dt: O.db_to_amplitude(v, r, p, dt), (ref, power), ref,
                          power, True, ("DB_to_amplitude", dtype, layout, ref, power))


def check_mu_decode(B, dtype, q, layout, lengths=ACCURACY_LENGTHS):
    views = [rows_view(np.random.default_rng(13 + L + q).integers(0, q, (3, L)).astype(np.float64), dtype, layout)
             for L in lengths]
    out_dtype = dtype if dtype in FLOATS else torch.float32
    return check_accuracy(B, MU_DECODE, views, out_dtype, lambda v, qq, dt: O.mu_decode(v, qq, dt), (q,), q - 1.0, 0.0, False,
                          ("mu_law_decoding", dtype, q, layout))


# ---- mu_law_encoding ----------------------------------------------------------------------------------------------------------------
def check_mu_encode(B, dtype, q, L, layout):
    x = rows_view(signal(np.random.default_rng(14 + L + q), 3, L), dtype, layout)
    got = B.pointwise(MU_ENCODE, x, torch.int64, q - 1.0, 0.0, 0, None, 0, 0)
    assert got.dtype == torch.int64 and got.shape == x.shape
    v = O.mu_encode_value(f64(x), q, np.float64)
    want = np.trunc(v).astype(np.int64)
    band = np.abs(v - np.round(v)) <= O.mu_band(q)
    g = got.numpy()
    what = ("mu_law_encoding", dtype, q, L, layout)
    assert np.array_equal(g[~band], want[~band]), what
    assert (np.abs(g[band] - want[band]) <= 1).all(), what
    if v.size >= 1000:
        share = band.mean()
        print("%s: %.4f %% of the inputs lie in the band, %d codes differ there" % (what, 100 * share, int((g != want).sum())))
        assert share <= 0.01, what
    assert g.min(initial=0) >= 0 and g.max(initial=0) <= q - 1


def check_mu_exact_and_round_trip(B, dtype, q):
    x = rows_view(np.array([[-1.0, 0.0, 1.0]]), dtype, "dense")
    got = B.pointwise(MU_ENCODE, x, torch.int64, q - 1.0, 0.0, 0, None, 0, 0)
    assert got.numpy().tolist() == O.mu_encode(np.array([[-1.0, 0.0, 1.0]]), q, np.float64).tolist() == [[0, q // 2, q - 1]]
    x = rows_view(signal(np.random.default_rng(15 + q), 2, 1025), dtype, "dense")
    code = B.pointwise(MU_ENCODE, x, torch.int64, q - 1.0, 0.0, 0, None, 0, 0)
    back = B.pointwise(MU_DECODE, code, torch.float32, q - 1.0, 0.0, 0, None, 0, 0)
    c = code.numpy()
    mid = O.mu_decode(c, q, np.float64)
    step = np.maximum(O.mu_decode(np.minimum(c + 1, q - 1), q, np.float64) - mid, mid - O.mu_decode(np.maximum(c - 1, 0), q, np.float64))
    assert (np.abs(back.double().numpy() - f64(x)) <= step).all(), (dtype, q)


# ---- spectral centroid ------------------------------------------------------------------------------------------------------------
N_FREQS = (1, 2, 33, 63, 64, 65, 201, 257, 4097)
N_FRAMES = (1, 2, 65)
N_ROWS = (1, 3)


def magnitudes(rng, rows, frames, n_freq, layout):
    """float32 |noise| as a (rows, frames, n_freq) view of a wider buffer at element offset 1: "lines" has unit stride along
    frequency (frame-major), "time" along time."""
    row_stride = frames * n_freq + 5
    base = torch.zeros(1 + rows * row_stride + 4, dtype=torch.float32)
    strides = (row_stride, n_freq, 1) if layout == "lines" else (row_stride, 1, frames)
    m3 = base.as_strided((rows, frames, n_freq), strides, 1)
    m3.copy_(torch.from_numpy(np.abs(rng.standard_normal((rows, frames, n_freq))).astype(np.float32)))
    return m3


def freqs_of(n_freq):
    return torch.linspace(0, 8000, n_freq)


def assert_centroid(got, m3, freqs, out_dtype, what):
    want = O.centroid(m3.numpy(), freqs.numpy())
    assert got.dtype == out_dtype and tuple(got.shape) == tuple(want.shape), what
    g = got.double().numpy()
    assert np.array_equal(np.isnan(g), np.isnan(want)), what
    ok = ~np.isnan(want)
    # float64 sums of at most 4097 non-negative terms: relative error <= 4097 * 2^-53 each, far below half a float32 ulp, so the
    # one rounding lands on one of the two float32 neighbours of the exact value
    bound = O.ulp32(want[ok]) + O.half_ulp(want[ok], out_dtype)
    assert (np.abs(g[ok] - want[ok]) <= bound).all(), (what, float(np.abs(g[ok] - want[ok]).max()))


def check_centroid(B, n_freq, frames, rows, layout, out_dtype=torch.float32):
    rng = np.random.default_rng(n_freq * 131 + frames * 7 + rows)
    m3, freqs = magnitudes(rng, rows, frames, n_freq, layout), freqs_of(n_freq)
    assert_centroid(B.centroid(m3, freqs, out_dtype), m3, freqs, out_dtype, (n_freq, frames, rows, layout, out_dtype))


def check_centroid_zero_and_nan_frames(B, layout):
    rng = np.random.default_rng(5)
    for n_freq in (33, 201):
        m3, freqs = magnitudes(rng, 3, 65, n_freq, layout), freqs_of(n_freq)
        clean = B.centroid(m3, freqs, torch.float32)
        m3[1, 7] = 0.0                                   # silence: 0 / 0
        m3[2, 64, n_freq // 2] = float("nan")
        m3[0, 0, 0] = float("nan")
        got = B.centroid(m3, freqs, torch.float32)
        bad = torch.zeros(3, 65, dtype=torch.bool)
        bad[1, 7] = bad[2, 64] = bad[0, 0] = True
        assert torch.isnan(got[bad]).all() and not torch.isnan(got[~bad]).any()
        assert torch.equal(got[~bad], clean[~bad])       # the neighbours keep their bits
        assert_centroid(got, m3, freqs, torch.float32, ("zero / nan", n_freq, layout))
