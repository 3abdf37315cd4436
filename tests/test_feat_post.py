"""F.compute_deltas / F.sliding_window_cmn without a GPU: the float64 oracle's two forms against each other, the window
map's properties, hand-computed cases, a CPU replay of csrc/feat_post.h's phase functions, meta shapes, TorchScript,
and the refusals (CPU tensors, win_length < 3)."""
import ctypes as C
import io
import os
import subprocess

import numpy as np
import pytest
import torch

import feat_post_oracle as O
import audio_amd.functional as F
import audio_amd.transforms as T
from audio_amd import _ops  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
SIM_SRC = os.path.join(HERE, "cpu_sim", "sim_feat_post.cpp")
SIM_OUT = os.path.join(HERE, "cpu_sim", "_build", "libaamd_sim_feat_post.so")
HDR = os.path.join(os.path.dirname(HERE), "audio_amd", "csrc", "feat_post.h")

T_GRID = [1, 2, 5, 99, 100, 101, 599, 601, 1001, 2500]
MODES = ["replicate", "reflect", "circular", "constant"]
PAD_ID = {"reflect": 0, "constant": 1, "replicate": 2, "circular": 3}


def _cmn_cases():
    out = []
    for Tn in T_GRID:
        for win in (1, 2, 7, 600):
            for mn in (0, 100, Tn + 5):
                for center in (False, True):
                    out.append((Tn, win, mn, center))
    return out


def cmvn_condition(x, win, mn, center):
    """Per element: the magnitudes cancelled in norm_vars' sumsq / n - sum^2 / n^2 over |variance| of its window (the
    factor by which sum-order rounding is amplified; a 2-frame window of two nearly equal values is arbitrarily
    ill-conditioned).
    0 where the window has one frame (the output is exactly 0 there)."""
    x = np.asarray(x, dtype=np.float64)
    Tn, F_ = x.shape[-2:]
    xs = x.reshape(-1, Tn, F_)
    s, e = O.cmn_bounds(Tn, win, mn, center)
    n = (e - s).astype(np.float64)[None, :, None]
    z = np.zeros((xs.shape[0], 1, F_))
    p1 = np.concatenate([z, np.cumsum(xs, 1)], 1)
    p2 = np.concatenate([z, np.cumsum(xs * xs, 1)], 1)
    s1, s2 = p1[:, e] - p1[:, s], p2[:, e] - p2[:, s]
    var = np.abs(s2 / n - (s1 / n) ** 2)
    # magnitude of what the prefix-sum form cancels to get var (its prefix sums grow with t)
    scale = (np.abs(p2[:, e]) + np.abs(p2[:, s])) / n + 2 * np.abs(s1 / n) * (np.abs(p1[:, e]) + np.abs(p1[:, s])) / n
    with np.errstate(divide="ignore", invalid="ignore"):
        cond = np.where(n == 1, 0.0, scale / var)
    return cond.reshape(x.shape)


def assert_cmvn_close(got, want, x, win, mn, center, rel, atol=1e-9):
    """|got - want| <= atol + |want| (rel + 1e-13 cond): float64 rounding amplified by the window's conditioning."""
    cond = cmvn_condition(x, win, mn, center).reshape(np.shape(want))
    got = np.asarray(got, np.float64)
    with np.errstate(invalid="ignore"):
        tol = atol + np.abs(want) * (rel + 1e-13 * cond)
        ok = (np.abs(got - want) <= tol) | ~np.isfinite(tol) | (np.isnan(got) & np.isnan(want))
    assert ok.all(), (win, mn, center, np.argwhere(~ok)[:5])


@pytest.mark.parametrize("norm_vars", [False, True])
def test_cmn_oracle_forms_agree(norm_vars):
    rng = np.random.default_rng(0)
    for Tn, win, mn, center in _cmn_cases():
        x = rng.standard_normal((2, Tn, 3)) + 3.0
        a = O.cmn_loop(x, win, mn, center, norm_vars)
        b = O.cmn_prefix(x, win, mn, center, norm_vars)
        if norm_vars:
            assert_cmvn_close(a, b, x, win, mn, center, rel=1e-12)
        else:
            np.testing.assert_allclose(a, b, rtol=0, atol=1e-9, err_msg=str((Tn, win, mn, center)))


@pytest.mark.parametrize("Tn", T_GRID)
def test_cmn_window_map_properties(Tn):
    for win in (0, 1, 2, 7, 8, 600, 601):
        for mn in (0, 1, 100, Tn + 5):
            for center in (False, True):
                s, e = O.cmn_bounds(Tn, win, mn, center)
                assert (s >= 0).all() and (e <= Tn).all()
                if win >= 1 or not center:
                    assert ((e - s) >= 1).all(), (Tn, win, mn, center)
                    assert (s <= np.arange(Tn)).all() and (e > np.arange(Tn)).all()
                if Tn > 1:
                    for arr in (s, e):
                        d = np.diff(arr)
                        assert ((d >= 0) & (d <= 1)).all(), (Tn, win, mn, center)


def test_cmn_hand_cases():
    x = np.array([[1.0], [2.0], [3.0], [4.0]])
    # center=False, window 600, min 100 > T: every frame's window is the whole utterance
    np.testing.assert_allclose(O.cmn_loop(x, 600, 100, False)[:, 0], [-1.5, -0.5, 0.5, 1.5])
    # cmn_window = 1, min 0, no centre: windows [0,1) [0,2) [1,3) [2,4)
    np.testing.assert_allclose(O.cmn_loop(x, 1, 0, False)[:, 0], [0.0, 0.5, 0.5, 0.5])
    # centred window 2: s = t - 1 -> [0,2) [0,2) [1,3) [2,4)
    np.testing.assert_allclose(O.cmn_prefix(x, 2, 0, True)[:, 0], [-0.5, 0.5, 0.5, 0.5])
    # norm_vars over the whole utterance: (x - 2.5) / sqrt(1.25)
    np.testing.assert_allclose(O.cmn_prefix(x, 600, 100, False, True)[:, 0], (x[:, 0] - 2.5) / np.sqrt(1.25))
    # one-frame windows normalise to zero
    np.testing.assert_allclose(O.cmn_loop(x, 0, 0, False, True), 0.0)
    # 2-D input of one frame squeezes to (freq,)
    assert O.cmn_loop(np.ones((1, 3))).shape == (3,)
    assert O.cmn_loop(np.ones((2, 3))).shape == (2, 3)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("win_length", [3, 4, 5, 7, 9])
def test_deltas_oracle_forms_agree(mode, win_length):
    rng = np.random.default_rng(1)
    n = (win_length - 1) // 2
    for Tn in [1, 2, 3, 5, 64, 101]:
        if (mode == "reflect" and n >= Tn) or (mode == "circular" and n > Tn):
            continue
        x = rng.standard_normal((2, 3, Tn))
        np.testing.assert_allclose(O.deltas_pad_corr(x, win_length, mode), O.deltas_conv1d(x, win_length, mode),
                                   rtol=0, atol=1e-12)


def test_deltas_hand_cases():
    x = np.array([0.0, 1.0, 2.0, 3.0, 4.0])
    # a ramp: slope 1 inside; replicate ends (n = 2, denom 10): t=0: (1*(1-0) + 2*(2-0)) / 10 = 0.5
    np.testing.assert_allclose(O.deltas_pad_corr(x, 5), [0.5, 0.8, 1.0, 0.8, 0.5])
    np.testing.assert_allclose(O.deltas_pad_corr(x, 3, "constant"), [0.5, 1.0, 1.0, 1.0, -1.5])
    with pytest.raises(ValueError, match="Window length should be greater than or equal to 3"):
        O.deltas_pad_corr(x, 2)


# ---- CPU replay of csrc/feat_post.h -------------------------------------------------------------------------------------

_sim = None


def sim():
    global _sim
    if _sim is None:
        stale = not os.path.exists(SIM_OUT) or max(os.path.getmtime(SIM_SRC), os.path.getmtime(HDR)) > os.path.getmtime(SIM_OUT)
        if stale:
            os.makedirs(os.path.dirname(SIM_OUT), exist_ok=True)
            tmp = "%s.tmp.%d" % (SIM_OUT, os.getpid())
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", SIM_SRC, "-o", tmp])
            os.replace(tmp, SIM_OUT)
        _sim = C.CDLL(SIM_OUT)
        i64, i32, p = C.c_int64, C.c_int, C.c_void_p
        for name in ("sim_deltas_f32", "sim_deltas_f64"):
            getattr(_sim, name).argtypes = [p, p] + [i64] * 6 + [i32] * 3
        for name in ("sim_cmn_f32", "sim_cmn_f64"):
            getattr(_sim, name).argtypes = [p, p] + [i64] * 8 + [i32] * 3
    return _sim


def _elem_strides(a):
    return [s // a.itemsize for s in a.strides]


def sim_deltas(x3, win_length, mode, adjoint=False):
    """x3: a numpy (C, F, T) view of any strides (its base buffer is what the kernel reads)."""
    fn = sim().sim_deltas_f64 if x3.dtype == np.float64 else sim().sim_deltas_f32
    out = np.zeros(x3.shape, dtype=x3.dtype)
    sc, sf, st = _elem_strides(x3)
    assert fn(x3.ctypes.data, out.ctypes.data, *x3.shape, sc, sf, st, win_length, PAD_ID[mode], int(adjoint)) == 0
    return out


def sim_cmn(x3, win, mn, center, norm_vars, adjoint=False):
    fn = sim().sim_cmn_f64 if x3.dtype == np.float64 else sim().sim_cmn_f32
    out = np.zeros(x3.shape, dtype=x3.dtype)
    sc, st, sf = _elem_strides(x3)
    assert fn(x3.ctypes.data, out.ctypes.data, *x3.shape, sc, st, sf, win, mn, int(center), int(norm_vars), int(adjoint)) == 0
    return out


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("layout", ["time_contiguous", "frame_major"])
def test_sim_deltas_both_layouts(mode, layout):
    rng = np.random.default_rng(2)
    for Tn in [1, 3, 63, 64, 65, 129, 1001]:
        for win_length in (3, 5, 9):
            n = (win_length - 1) // 2
            if (mode == "reflect" and n >= Tn) or (mode == "circular" and n > Tn):
                continue
            F_ = 80 if Tn > 100 else 7
            if layout == "time_contiguous":
                x3 = rng.standard_normal((2, F_, Tn))
            else:
                x3 = np.swapaxes(rng.standard_normal((2, Tn, F_)), 1, 2)          # (C, F, T) view of (C, T, F) storage
            want = O.deltas_pad_corr(x3, win_length, mode)
            np.testing.assert_allclose(sim_deltas(x3, win_length, mode), want, rtol=0, atol=1e-12)
            got32 = sim_deltas(x3.astype(np.float32), win_length, mode)
            np.testing.assert_allclose(got32, want, rtol=0, atol=1e-5 * np.abs(x3).max())


@pytest.mark.parametrize("mode", MODES)
def test_sim_deltas_adjoint_is_the_transpose(mode):
    for Tn in [1, 2, 4, 9, 70]:
        for win_length in (3, 5, 9):
            n = (win_length - 1) // 2
            if (mode == "reflect" and n >= Tn) or (mode == "circular" and n > Tn):
                continue
            # the dense matrix of the forward map, column by column, and the adjoint applied to unit vectors
            eye = np.eye(Tn).reshape(Tn, 1, Tn)
            D = sim_deltas(eye, win_length, mode).reshape(Tn, Tn).T          # D[t, u] = d out[t] / d x[u]
            Dt = sim_deltas(eye, win_length, mode, adjoint=True).reshape(Tn, Tn).T
            np.testing.assert_allclose(Dt, D.T, rtol=0, atol=1e-12, err_msg=str((Tn, win_length)))
            ref = np.stack([O.deltas_pad_corr(np.eye(Tn)[u], win_length, mode) for u in range(Tn)], 1)
            np.testing.assert_allclose(D, ref, rtol=0, atol=1e-12)


@pytest.mark.parametrize("norm_vars", [False, True])
@pytest.mark.parametrize("center", [False, True])
def test_sim_cmn_chunk_boundaries(norm_vars, center):
    rng = np.random.default_rng(4)
    for Tn in [1, 2, 63, 64, 65, 127, 128, 129, 200, 601, 1001]:
        for win, mn in [(600, 100), (7, 0), (1, 0), (2, Tn + 5), (150, 40)]:
            x = rng.standard_normal((2, Tn, 5)) + 2.0
            want = O.cmn_prefix(x, win, mn, center, norm_vars).reshape(x.shape)
            xv = np.swapaxes(np.ascontiguousarray(np.swapaxes(x, 1, 2)), 1, 2)      # a strided (freq-major) view
            x32 = x.astype(np.float32)
            want32 = O.cmn_prefix(x32, win, mn, center, norm_vars).reshape(x.shape)
            for got in (sim_cmn(x, win, mn, center, norm_vars), sim_cmn(xv, win, mn, center, norm_vars)):
                if norm_vars:
                    assert_cmvn_close(got, want, x, win, mn, center, rel=1e-12)
                else:
                    np.testing.assert_allclose(got, want, rtol=0, atol=1e-10, err_msg=str((Tn, win, mn)))
            got32 = sim_cmn(x32, win, mn, center, norm_vars)
            if norm_vars:       # float64 arithmetic on float32 inputs: the result's own rounding on top
                assert_cmvn_close(got32, want32, x32, win, mn, center, rel=2e-7, atol=1e-6)
            else:
                np.testing.assert_allclose(got32, want, rtol=0, atol=2e-6 * np.abs(x).max())


@pytest.mark.parametrize("center", [False, True])
def test_sim_cmn_adjoint_is_the_transpose(center):
    for Tn in [1, 3, 64, 65, 130, 257]:
        for win, mn in [(600, 100), (7, 0), (1, 0), (100, 30), (2, Tn + 5)]:
            eye = np.eye(Tn).reshape(Tn, Tn, 1)
            M = sim_cmn(eye, win, mn, center, False)[:, :, 0].T                 # M[t, u] = d out[t] / d x[u]
            Mt = sim_cmn(eye, win, mn, center, False, adjoint=True)[:, :, 0].T
            np.testing.assert_allclose(Mt, M.T, rtol=0, atol=1e-12, err_msg=str((Tn, win, mn, center)))


# ---- op surface without a device ----------------------------------------------------------------------------------------

def test_meta_shapes_and_strides():
    spec = torch.empty(3, 40, 101, device="meta").transpose(-1, -2).transpose(-1, -2)
    fm = torch.empty(3, 101, 40, device="meta").transpose(-1, -2)                 # frame-major (3, 40, 101)
    for x in (spec, fm, torch.empty(101, device="meta"), torch.empty(2, 3, 40, 101, device="meta")):
        y = torch.ops.audio_amd.compute_deltas(x, 5, "replicate")
        assert y.shape == x.shape and y.is_contiguous()
    for shape, want in [((3, 101, 40), (3, 101, 40)), ((101, 40), (101, 40)), ((1, 40), (40,)), ((2, 1, 40), (2, 1, 40))]:
        y = torch.ops.audio_amd.sliding_window_cmn(torch.empty(shape, device="meta"), 600, 100, False, False)
        assert tuple(y.shape) == want and y.is_contiguous()
    y = torch.ops.audio_amd.sliding_window_cmn(torch.empty(3, 40, 101, device="meta").transpose(-1, -2), 600, 100, True, True)
    assert y.shape == (3, 101, 40) and y.is_contiguous()


def _roundtrip(m):
    buf = io.BytesIO()
    torch.jit.save(m, buf)
    buf.seek(0)
    return torch.jit.load(buf)


def test_torchscript_modules_and_functions():
    for mod in (T.ComputeDeltas(win_length=7, mode="reflect"), T.SlidingWindowCmn(300, 50, True, True)):
        sm = torch.jit.script(mod)
        assert sm.state_dict() == {} and mod.state_dict() == {}
        lm = _roundtrip(sm)
        assert "audio_amd" in lm.code
    sm = torch.jit.script(T.ComputeDeltas())
    assert sm.win_length == 5 and sm.mode == "replicate"
    assert T.ComputeDeltas.__constants__ == ["win_length"]
    c = T.SlidingWindowCmn()
    assert (c.cmn_window, c.min_cmn_window, c.center, c.norm_vars) == (600, 100, False, False)
    assert list(dict(c.named_buffers())) == []
    for fn in (F.compute_deltas, F.sliding_window_cmn):
        sf = torch.jit.script(fn)
        assert "audio_amd::" in str(sf.graph)


def test_cpu_tensors_are_refused():
    x = torch.randn(2, 40, 50)
    with pytest.raises(NotImplementedError, match="CPU"):
        torch.ops.audio_amd.compute_deltas(x, 5, "replicate")
    with pytest.raises(NotImplementedError, match="CPU"):
        torch.ops.audio_amd.sliding_window_cmn(x, 600, 100, False, False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        T.ComputeDeltas()(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        T.SlidingWindowCmn()(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.sliding_window_cmn(x, norm_vars=True)


def test_win_length_below_three_raises():
    for w in (0, 1, 2):
        with pytest.raises(ValueError, match=f"Found win_length {w}"):
            F.compute_deltas(torch.randn(2, 10), win_length=w)
        with pytest.raises(ValueError, match="greater than or equal to 3"):
            T.ComputeDeltas(win_length=w)(torch.randn(2, 10))
