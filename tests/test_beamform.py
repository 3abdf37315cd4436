"""MVDR beamforming without a GPU: the two forms of the complex128 oracle against each other, a CPU replay of
csrc/beamform.h (PSD in both layouts with none, one and two masks; the per-bin solve in its four modes; apply) against the
oracle, signatures, checks and exception types, Meta shapes and strides, TorchScript and torch.compile seeing one op per
stage."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest
import torch

import beamform_oracle as O
import audio_amd.functional as F
import audio_amd.transforms as T
from audio_amd import _ops  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
SIM_SRC = os.path.join(HERE, "cpu_sim", "sim_beamform.cpp")
SIM_OUT = os.path.join(HERE, "cpu_sim", "_build", "libaamd_sim_beamform.so")
HDRS = [os.path.join(os.path.dirname(HERE), "audio_amd", "csrc", h) for h in ("beamform.h", "hd.h")]
CODE = {np.complex64: 0, np.complex128: 1}
REAL = {np.complex64: np.float32, np.complex128: np.float64}
U = {np.complex64: 2.0 ** -23, np.complex128: 2.0 ** -52}


_sim = None


def sim():
    global _sim
    if _sim is None:
        newest = max(os.path.getmtime(p) for p in [SIM_SRC] + HDRS)
        if not os.path.exists(SIM_OUT) or newest > os.path.getmtime(SIM_OUT):
            os.makedirs(os.path.dirname(SIM_OUT), exist_ok=True)
            tmp = "%s.tmp.%d" % (SIM_OUT, os.getpid())
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", SIM_SRC, "-o", tmp])
            os.replace(tmp, SIM_OUT)
        _sim = C.CDLL(SIM_OUT)
    return _sim


def _i64(*v):
    return (C.c_int64 * len(v))(*v)


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _strides(a, unit):
    return [s // unit for s in a.strides]


def layout(x, kind):
    """x (B, C, F, T) in the named memory layout: values unchanged."""
    if kind == "time":
        return np.ascontiguousarray(x)
    assert kind == "frame"
    return np.ascontiguousarray(x.transpose(0, 1, 3, 2)).transpose(0, 1, 3, 2)


def sim_psd(x, m1=None, m2=None, normalize=True, eps=1e-10):
    B, Cc, Fq, Tt = x.shape
    dt = x.dtype.type
    out = np.full(((2 if m2 is not None else 1), B, Fq, Cc, Cc), np.nan, dtype=dt)
    xs = _strides(x, x.itemsize)
    ms = [_i64(*_strides(m, m.itemsize)) if m is not None else None for m in (m1, m2)]
    rc = sim().sim_bf_psd(CODE[dt], _p(x), _i64(B, Cc, Fq, Tt), _i64(*xs), _p(m1), ms[0], _p(m2), ms[1], int(normalize),
                          C.c_double(eps), _p(out))
    assert rc == 0
    return out


def sim_weights(mode, a, b, ref=-1, u=None, loading=True, diag_eps=1e-7, eps=1e-8, n_iter=0, adjoint=False, K=0):
    """a (batch, F, C, C), b per mode; returns (batch, F, C) or (batch, F, C, K)."""
    batch, Fq, Cc = a.shape[:3]
    dt = a.dtype.type
    out = np.full(b.shape if mode == 0 else a.shape[:3], np.nan, dtype=dt)
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    u = np.ascontiguousarray(u.astype(dt)) if u is not None else None
    rc = sim().sim_bf_weights(CODE[dt], mode, _p(a), _p(b), _p(u), _p(out), C.c_int64(batch), C.c_int64(Fq), Cc, K, ref,
                              int(loading), C.c_double(diag_eps), C.c_double(eps), n_iter, int(adjoint))
    assert rc == 0
    return out


def sim_apply(w, x):
    B, Cc, Fq, Tt = x.shape
    dt = x.dtype.type
    frame = Tt > 1 and x.strides[3] != x.itemsize
    out = np.full((B, Tt, Fq) if frame else (B, Fq, Tt), np.nan, dtype=dt)
    res = out.transpose(0, 2, 1) if frame else out
    rc = sim().sim_bf_apply(CODE[dt], _p(np.ascontiguousarray(w)), _p(x), _i64(B, Cc, Fq, Tt), _i64(*_strides(x, x.itemsize)),
                            _p(out), _i64(*_strides(res, res.itemsize)))
    assert rc == 0
    return res


def spec(rng, B, Cc, Fq, Tt, dt=np.complex128):
    return (rng.standard_normal((B, Cc, Fq, Tt)) + 1j * rng.standard_normal((B, Cc, Fq, Tt))).astype(dt)


def masks(rng, B, Fq, Tt, dt):
    return rng.uniform(0.05, 1.0, (B, Fq, Tt)).astype(REAL[dt])


# ---- the oracle's two forms -----------------------------------------------------------------------------------------------------

def test_oracle_forms_agree():
    rng = np.random.default_rng(0)
    x = spec(rng, 2, 3, 4, 9).reshape(2, 1, 3, 4, 9)
    m = rng.uniform(0.05, 1, (2, 1, 4, 9))
    m[0, 0, 1] = 0.0
    for mask in (None, m):
        for norm in (True, False):
            np.testing.assert_allclose(O.psd(x, mask, norm), O.psd_loop(x, mask, norm), rtol=0, atol=1e-12)
    ps, pn = O.psd(x, m), O.psd(x, 1 - m)
    u = rng.standard_normal((2, 1, 3)) + 1j * rng.standard_normal((2, 1, 3))
    for ref in (0, 2, u):
        for loading in (True, False):
            a, b = O.mvdr_weights_souden(ps, pn, ref, loading), O.mvdr_weights_souden_loop(ps, pn, ref, loading)
            np.testing.assert_allclose(a, b, rtol=0, atol=1e-12 * np.abs(a).max())
            for n_iter in (1, 2, 3, 5):
                a, b = O.rtf_power(ps, pn, ref, n_iter, loading), O.rtf_power_loop(ps, pn, ref, n_iter, loading)
                np.testing.assert_allclose(a, b, rtol=0, atol=1e-12 * np.abs(a).max())
    r = O.rtf_power(ps, pn, 0)
    for ref in (None, 1, u):
        a, b = O.mvdr_weights_rtf(r, pn, ref), O.mvdr_weights_rtf_loop(r, pn, ref)
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-12 * np.abs(a).max())
    w = O.mvdr_weights_souden(ps, pn, 0)
    np.testing.assert_allclose(O.apply_beamforming(w, x), O.apply_beamforming_loop(w, x), rtol=0, atol=1e-12)
    # a one-hot vector is the index
    np.testing.assert_allclose(O.mvdr_weights_souden(ps, pn, np.broadcast_to(np.eye(3)[1], (2, 1, 3))),
                               O.mvdr_weights_souden(ps, pn, 1), rtol=1e-13)


# ---- CPU replay of csrc/beamform.h ------------------------------------------------------------------------------------------------

def test_sim_tiles_are_the_exported_constants():
    assert sim().sim_bf_freq_tile() == 16 and sim().sim_bf_time_chunk() == 16


@pytest.mark.parametrize("dt", [np.complex64, np.complex128])
@pytest.mark.parametrize("kind", ["time", "frame"])
@pytest.mark.parametrize("Cc", [1, 2, 3, 4, 8, 16])
def test_sim_psd(dt, kind, Cc):
    rng = np.random.default_rng(Cc)
    FT = sim().sim_bf_freq_tile()
    for Fq, Tt in ((1, 17), (5, 1), (FT - 1, 2 * Cc + 5), (FT, 17), (FT + 1, 131 if Cc <= 3 else 9)):
        x = layout(spec(rng, 2, Cc, Fq, Tt, dt), kind)
        m1, m2 = masks(rng, 2, Fq, Tt, dt), masks(rng, 2, Fq, Tt, dt)
        m2[1, Fq // 2] = 0.0                                   # an all-zero row: the eps path
        for ms, norm in (((), True), ((m1,), True), ((m1,), False), ((m1, m2), True), ((m2, m1), False)):
            got = sim_psd(x, *ms, normalize=norm)
            assert got.shape[0] == max(len(ms), 1)
            for n in range(got.shape[0]):
                mask = ms[n] if ms else None
                want = O.psd(x, mask, norm, wide=True)
                bound = 4 * U[dt] * O.psd_abs_terms(x, mask, norm)
                assert np.all(np.abs(got[n] - want) <= bound), (Fq, Tt, len(ms), norm)
                assert np.array_equal(got[n], got[n].conj().transpose(0, 1, 3, 2))      # exactly Hermitian


def _psd_pair(rng, B, Cc, Fq, Tt, dt):
    x = spec(rng, B, Cc, Fq, Tt)
    m = rng.uniform(0.05, 1.0, (B, Fq, Tt))
    return O.psd(x, m).astype(dt), O.psd(x, 1 - m + 0.05).astype(dt)


@pytest.mark.parametrize("dt", [np.complex64, np.complex128])
@pytest.mark.parametrize("Cc", [1, 2, 3, 4, 8, 16])
def test_sim_weights(dt, Cc):
    rng = np.random.default_rng(100 + Cc)
    B, Fq = 2, 5
    ps, pn = _psd_pair(rng, B, Cc, Fq, 2 * Cc + 5, dt)
    u = rng.standard_normal((B, Cc)) + 1j * rng.standard_normal((B, Cc))
    for loading in (True, False):
        cond = O.condition(pn, loading=loading)
        assert cond <= 1e5
        tol = 8 * cond * U[dt]
        for ref, vec in ((Cc - 1, None), (-1, u)):
            oref = ref if vec is None else vec
            want = O.mvdr_weights_souden(ps, pn, oref, loading)
            got = sim_weights(1, pn, ps, ref, vec, loading)
            assert np.abs(got - want).max() <= tol * np.abs(want).max()
            for n_iter in (1, 2, 3, 5):
                want = O.rtf_power(ps, pn, oref, n_iter, loading)
                got = sim_weights(3, pn, ps, ref, vec, loading, n_iter=n_iter)
                assert np.abs(got - want).max() <= tol * np.abs(want).max(), n_iter
        r = O.rtf_power(ps, pn, 0).astype(dt)
        for ref, vec, oref in ((-1, None, None), (0, None, 0), (-1, u, u)):
            want = O.mvdr_weights_rtf(r, pn, oref, loading)
            got = sim_weights(2, pn, r, ref, vec, loading)
            assert np.abs(got - want).max() <= tol * np.abs(want).max()
    # the plain solve and its adjoint, fewer right-hand sides than channels
    K = max(Cc - 1, 1)
    b = (rng.standard_normal((B, Fq, Cc, K)) + 1j * rng.standard_normal((B, Fq, Cc, K))).astype(dt)
    a = O.loaded(pn).astype(dt)
    cond = O.condition(a, loading=False)
    for adjoint in (False, True):
        A = a.conj().transpose(0, 1, 3, 2) if adjoint else a
        want = np.linalg.solve(A.astype(np.complex128), b.astype(np.complex128))
        got = sim_weights(0, a, b, loading=False, adjoint=adjoint, K=K)
        assert np.abs(got - want).max() <= 8 * cond * U[dt] * np.abs(want).max()


def test_sim_solve_pivots():
    """A zero in the leading position: without row exchanges the elimination divides by zero."""
    a = np.array([[[[0, 2, 1], [1, 1j, 0], [3, 0, 1]]]], dtype=np.complex128)
    b = np.array([[[[1], [2], [3j]]]], dtype=np.complex128)
    got = sim_weights(0, a, b, loading=False, K=1)
    np.testing.assert_allclose(got, np.linalg.solve(a, b), rtol=1e-13)


@pytest.mark.parametrize("dt", [np.complex64, np.complex128])
@pytest.mark.parametrize("kind", ["time", "frame"])
def test_sim_apply(dt, kind):
    rng = np.random.default_rng(7)
    for Cc, Fq, Tt in ((1, 1, 1), (2, 5, 9), (3, 17, 131), (4, 129, 33), (16, 15, 37), (8, 257, 3)):
        x = layout(spec(rng, 2, Cc, Fq, Tt, dt), kind)
        w = (rng.standard_normal((2, Fq, Cc)) + 1j * rng.standard_normal((2, Fq, Cc))).astype(dt)
        got = sim_apply(w, x)
        assert np.all(np.abs(got - O.apply_beamforming(w, x, wide=True)) <= 4 * U[dt] * O.apply_abs_terms(w, x))
    # rows that do not start on a 16-byte boundary (a view cut from a wider buffer)
    base = spec(rng, 2, 3, 6, 40, dt)
    x = base[:, :, :, 1:38] if kind == "time" else layout(base, "frame")[:, :, 1:6, :]
    w = (rng.standard_normal((2, x.shape[2], 3)) + 1j * rng.standard_normal((2, x.shape[2], 3))).astype(dt)
    assert np.all(np.abs(sim_apply(w, x) - O.apply_beamforming(w, x, wide=True)) <= 4 * U[dt] * O.apply_abs_terms(w, x))


# ---- the public surface -----------------------------------------------------------------------------------------------------------

def test_signatures_follow_the_reference():
    def sig(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]
    E = inspect.Parameter.empty
    assert sig(F.psd) == [("specgram", E), ("mask", None), ("normalize", True), ("eps", 1e-10)]
    assert sig(F.mvdr_weights_souden) == [("psd_s", E), ("psd_n", E), ("reference_channel", E), ("diagonal_loading", True),
                                          ("diag_eps", 1e-7), ("eps", 1e-8)]
    assert sig(F.mvdr_weights_rtf) == [("rtf", E), ("psd_n", E), ("reference_channel", None), ("diagonal_loading", True),
                                       ("diag_eps", 1e-7), ("eps", 1e-8)]
    assert sig(F.rtf_power) == [("psd_s", E), ("psd_n", E), ("reference_channel", E), ("n_iter", 3), ("diagonal_loading", True),
                                ("diag_eps", 1e-7)]
    assert sig(F.apply_beamforming) == [("beamform_weights", E), ("specgram", E)]
    assert sig(T.PSD.__init__)[1:] == [("multi_mask", False), ("normalize", True), ("eps", 1e-15)]
    assert sig(T.MVDR.__init__)[1:] == [("ref_channel", 0), ("solution", "ref_channel"), ("multi_mask", False),
                                        ("diag_loading", True), ("diag_eps", 1e-7), ("online", False)]
    assert sig(T.MVDR.forward)[1:] == [("specgram", E), ("mask_s", E), ("mask_n", None)]
    for mod, second in ((T.SoudenMVDR, "psd_s"), (T.RTFMVDR, "rtf")):
        assert sig(mod.forward)[1:] == [("specgram", E), (second, E), ("psd_n", E), ("reference_channel", E),
                                        ("diagonal_loading", True), ("diag_eps", 1e-7), ("eps", 1e-8)]


def test_checks_and_exception_types():
    c = lambda *s: torch.zeros(s, dtype=torch.complex64)
    with pytest.raises(ValueError):
        F.psd(c(2, 3, 5, 7), torch.zeros(2, 5, 8))
    with pytest.raises(ValueError):
        F.psd(c(2, 3, 5, 7), torch.zeros(2, 3, 5, 7))
    with pytest.raises(ValueError):
        F.psd(c(5, 7))
    for fn in (lambda s, n: F.mvdr_weights_souden(s, n, 0), lambda s, n: F.rtf_power(s, n, 0)):
        with pytest.raises(ValueError):
            fn(c(3, 3), c(3, 3))                                  # at least 3-D
        with pytest.raises(TypeError):
            fn(torch.zeros(5, 3, 3), torch.zeros(5, 3, 3))        # complex
        with pytest.raises(ValueError):
            fn(c(5, 3, 4), c(5, 3, 4))                            # square
        with pytest.raises(ValueError):
            fn(c(5, 3, 3), c(4, 3, 3))                            # equal shapes
    for n_iter in (0, -1):
        with pytest.raises(ValueError):
            F.rtf_power(c(5, 3, 3), c(5, 3, 3), 0, n_iter=n_iter)
    with pytest.raises(ValueError):
        F.mvdr_weights_rtf(c(5, 4), c(5, 3, 3))
    with pytest.raises(TypeError):
        F.mvdr_weights_rtf(torch.zeros(5, 3), c(5, 3, 3))
    with pytest.raises(ValueError):
        F.apply_beamforming(c(2, 5, 3), c(1, 3, 5, 7))
    with pytest.raises(TypeError):
        F.apply_beamforming(torch.zeros(2, 5, 3), c(2, 3, 5, 7))
    with pytest.raises(RuntimeError):
        F.mvdr_weights_souden(c(5, 3, 3), c(5, 3, 3), 0.5)
    with pytest.raises(ValueError):
        T.MVDR(solution="best")
    with pytest.raises(ValueError):
        T.MVDR()(torch.zeros(3, 5, 7), torch.zeros(5, 7))


def test_what_is_out_of_scope_says_so():
    with pytest.raises(NotImplementedError, match="eigen"):
        T.MVDR(solution="stv_evd")
    with pytest.raises(NotImplementedError, match="online"):
        T.MVDR(online=True)
    with pytest.raises(NotImplementedError, match="eigen"):
        F.rtf_evd(torch.zeros(5, 3, 3, dtype=torch.complex64))
    c = lambda *s: torch.zeros(s, dtype=torch.complex64)
    for call in (lambda: F.psd(c(17, 5, 7)), lambda: F.mvdr_weights_souden(c(5, 17, 17), c(5, 17, 17), 0),
                 lambda: F.mvdr_weights_rtf(c(5, 17), c(5, 17, 17)), lambda: F.rtf_power(c(5, 17, 17), c(5, 17, 17), 0),
                 lambda: F.apply_beamforming(c(5, 17), c(17, 5, 7))):
        with pytest.raises(NotImplementedError, match="16 channels"):
            call()


def test_cpu_tensors_are_refused():
    c = lambda *s: torch.zeros(s, dtype=torch.complex64)
    x, m, p, r = c(2, 3, 5, 7), torch.zeros(2, 5, 7), c(2, 5, 3, 3), c(2, 5, 3)
    for call in (lambda: F.psd(x), lambda: F.psd(x, m), lambda: T.PSD()(x, m), lambda: F.mvdr_weights_souden(p, p, 0),
                 lambda: F.mvdr_weights_rtf(r, p), lambda: F.rtf_power(p, p, 0), lambda: F.apply_beamforming(r, x),
                 lambda: T.SoudenMVDR()(x, p, p, 0), lambda: T.RTFMVDR()(x, r, p, 0), lambda: T.MVDR()(x, m, m)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def _meta(*shape, dtype=torch.complex64):
    return torch.empty(shape, device="meta", dtype=dtype)


def _frame_major(*lead_c_f_t, dtype=torch.complex64):
    *lead, Fq, Tt = lead_c_f_t
    return _meta(*lead, Tt, Fq, dtype=dtype).transpose(-1, -2)


def test_meta_kernels():
    x = _meta(2, 3, 4, 5, 7)
    assert torch.ops.audio_amd.psd(x, None, True, 1e-10).shape == (2, 3, 5, 4, 4)
    m = _meta(2, 3, 5, 7, dtype=torch.float32)
    out = torch.ops.audio_amd.psd_pair(x, m, m, True, 1e-15)
    assert out.shape == (2, 2, 3, 5, 4, 4) and out.dtype == torch.complex64 and out.is_contiguous()
    p, r = _meta(2, 5, 4, 4, dtype=torch.complex128), _meta(2, 5, 4, dtype=torch.complex128)
    assert torch.ops.audio_amd.mvdr_weights_souden(p, p, 1, None, True, 1e-7, 1e-8).shape == (2, 5, 4)
    assert torch.ops.audio_amd.mvdr_weights_souden(p, p, -1, _meta(2, 4), True, 1e-7, 1e-8).dtype == torch.complex128
    assert torch.ops.audio_amd.mvdr_weights_rtf(r, p, None, None, True, 1e-7, 1e-8).shape == (2, 5, 4)
    assert torch.ops.audio_amd.rtf_power(p, p, 0, None, 3, True, 1e-7).shape == (2, 5, 4)
    # apply keeps the input's (freq, time) stride order
    w = _meta(2, 5, 4)
    out = torch.ops.audio_amd.apply_beamforming(w, _meta(2, 4, 5, 7))
    assert out.shape == (2, 5, 7) and out.stride() == (35, 7, 1)
    out = torch.ops.audio_amd.apply_beamforming(w, _frame_major(2, 4, 5, 7))
    assert out.shape == (2, 5, 7) and out.stride() == (35, 1, 5)


def test_modules_compile_under_torchscript():
    for mod in (T.PSD(), T.PSD(multi_mask=True), T.SoudenMVDR(), T.RTFMVDR(), T.MVDR(), T.MVDR(1, "stv_power", True)):
        s = torch.jit.script(mod)
        assert "audio_amd::" in str(s.inlined_graph)
    s = torch.jit.script(T.SoudenMVDR())
    p = torch.zeros(5, 3, 3, dtype=torch.complex64)
    with pytest.raises(Exception, match="CPU"):           # the op has no CPU kernel: refused by the dispatcher
        s(torch.zeros(3, 5, 7, dtype=torch.complex64), p, p, 0)
    # scripted modules trace on the meta device, with an index and with a vector reference
    x, pm = _frame_major(2, 3, 5, 7), _meta(2, 5, 3, 3)
    for ref in (1, _meta(2, 3)):
        y = s(x, pm, pm, ref)
        assert y.shape == (2, 5, 7) and y.stride() == (35, 1, 5)


def test_torch_compile_sees_one_op_per_stage():
    graphs = []

    def backend(gm, example_inputs):
        graphs.append(gm)
        return gm.forward

    def calls():
        return [str(n.target) for n in graphs[-1].graph.nodes if n.op == "call_function" and "audio_amd" in str(n.target)]

    x = _frame_major(2, 3, 5, 7)
    m = _meta(2, 5, 7, dtype=torch.float32)
    p, r = _meta(2, 5, 3, 3), _meta(2, 5, 3)
    y = torch.compile(T.PSD(), fullgraph=True, backend=backend)(x, m)
    assert y.shape == (2, 5, 3, 3) and calls() == ["audio_amd.psd"]
    y = torch.compile(T.SoudenMVDR(), fullgraph=True, backend=backend)(x, p, p, 0)
    assert y.shape == (2, 5, 7) and y.stride() == (35, 1, 5)
    assert calls() == ["audio_amd.mvdr_weights_souden", "audio_amd.apply_beamforming"]
    y = torch.compile(T.RTFMVDR(), fullgraph=True, backend=backend)(x, r, p, 0)
    assert calls() == ["audio_amd.mvdr_weights_rtf", "audio_amd.apply_beamforming"]
    y = torch.compile(T.MVDR(), fullgraph=True, backend=backend)(x, m, 1 - m)
    assert y.shape == (2, 5, 7) and y.dtype == torch.complex64 and y.stride() == (35, 1, 5)
    assert calls() == ["audio_amd.psd_pair", "audio_amd.mvdr_weights_souden",
                       "audio_amd.apply_beamforming"]
    y = torch.compile(T.MVDR(solution="stv_power"), fullgraph=True, backend=backend)(x, m, 1 - m)
    assert calls() == ["audio_amd.psd_pair", "audio_amd.rtf_power", "audio_amd.mvdr_weights_rtf",
                       "audio_amd.apply_beamforming"]
