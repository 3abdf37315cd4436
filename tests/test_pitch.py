"""F.detect_pitch_frequency without a GPU: the float64 oracle's two NCCF forms and the torch restatement against each other,
the host's size arithmetic and error paths, a CPU replay of csrc/pitch.h's phase functions, meta shapes, TorchScript and
the refusal of CPU tensors."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import pitch_oracle as O
import audio_amd.functional as F
from audio_amd import _ops  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
SIM_SRC = os.path.join(HERE, "cpu_sim", "sim_pitch.cpp")
SIM_OUT = os.path.join(HERE, "cpu_sim", "_build", "libaamd_sim_pitch.so")
HDRS = [os.path.join(os.path.dirname(HERE), "audio_amd", "csrc", h) for h in ("pitch.h", "hd.h")]


# ---- the oracle against itself and against the restated reference -------------------------------------------------------

@pytest.mark.parametrize("L", [1, 159, 160, 161, 500, 1234])
def test_nccf_oracle_forms_agree(L):
    rng = np.random.default_rng(L)
    x = rng.standard_normal((2, L))
    x[1, : L // 2] = 0.0                                         # silence: exact zeros in both forms
    for fs, lags in [(160, 189), (37, 50), (8, 3)]:
        a = O.nccf_loops(x, fs, lags)
        b = O.nccf_prefix(x, fs, lags)
        peak = np.maximum(np.abs(a).max(-1, keepdims=True), 1e-300)
        assert (np.abs(a - b) <= 1e-9 * peak).all(), (fs, lags)


def test_oracle_equals_torch_restatement():
    for sr, f0 in [(8000, 110.0), (16000, 220.0), (22050, 180.0)]:
        x = np.stack([O.tone(sr // 2, sr, f0, seed=1), O.tone(sr // 2, sr, f0 * 1.5, seed=2)])
        want = O.torch_reference(torch.from_numpy(x).double(), sr)
        got = O.detect(x, sr)
        assert got.dtype == np.float32 and want.dtype == torch.float32
        np.testing.assert_array_equal(got, want.numpy())
        # the restatement in float32 too: the same pick on these tones
        np.testing.assert_array_equal(O.torch_reference(torch.from_numpy(x), sr).numpy(), got)


def test_pick_first_index_and_threshold():
    n = np.zeros((1, 40))
    b = O.pick(n, 3)                                                # all ties: the first lag of the half slice wins
    assert b.tolist() == [4]
    n[0, 10] = 1.0
    n[0, 30] = 1.0
    assert O.pick(n, 3).tolist() == [11]
    n[0, 10] = 0.989
    assert O.pick(n, 3).tolist() == [31]                           # 0.989 > 0.99 * 1 is false
    n32 = np.zeros((1, 40), np.float32)
    n32[0, 30] = 1.0
    n32[0, 10] = np.float32(0.99) + np.float32(2 ** -24)
    assert O.pick(n32, 3).tolist() == [11]


def test_smooth_lower_median_and_reciprocal():
    lag = np.array([[5, 9, 7, 6, 8, 10, 4]])
    out = O.smooth(lag, 4, 16000)                                   # p = 1: [5, 5, 9, 7, 6, 8, 10, 4]
    med = [5, 6, 7, 7, 6]
    padded = torch.tensor([5, 5, 9, 7, 6, 8, 10, 4])
    assert torch.median(padded.unfold(-1, 4, 1), -1).values.tolist() == med
    want = (np.float32(1) / (np.float32(1e-9) + np.array(med, np.float32))) * np.float32(16000)
    np.testing.assert_array_equal(out[0], want.astype(np.float32))
    t = torch.tensor(med).to(torch.float)
    np.testing.assert_array_equal(out[0], (16000 / (1e-9 + t)).numpy())


# ---- host planning ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("frame_time", [0.01, 0.025, 1 / 3, 1e-3])
@pytest.mark.parametrize("sr", [8000, 16000, 22050, 44100, 48000])
def test_host_sizes_follow_the_spec(frame_time, sr):
    for L in [1, 100, sr, 3 * sr + 7]:
        lags = int(math.ceil(sr / 85))
        fs = int(math.ceil(sr * frame_time))
        Fn = int(math.ceil(L / fs))
        assert F._pitch_sizes(L, sr, frame_time, 85) == (lags, fs, Fn)
        s = O.sizes(L, sr, frame_time, 30, 85, 3400)
        if s["n_out"] >= 1 and fs <= 8192:
            assert F._pitch_plan(L, sr, frame_time, 30, 85, 3400) == (lags, fs, Fn, s["lag_min"], s["n_out"])
    assert F._pitch_sizes(160000, 16000, 0.01, 85)[1] == 160
    assert F._pitch_sizes(160000, 16000, 1 / 3, 85)[1] == 5334      # ceil(5333.33)
    assert F._pitch_sizes(100, 16000, 0.025, 85) == (189, 400, 1)


def test_error_paths_match_the_reference():
    plan = F._pitch_plan
    with pytest.raises(ZeroDivisionError):
        plan(1000, 16000, 0.01, 30, 0, 3400)
    with pytest.raises(ZeroDivisionError):
        plan(1000, 16000, 0.0, 30, 85, 3400)
    with pytest.raises(ZeroDivisionError):
        plan(1000, 16000, 0.01, 30, 85, 0)
    with pytest.raises(ValueError, match="non-empty list"):
        plan(1000, 16000, 0.01, 30, -85, 3400)                      # no lag at all
    with pytest.raises(IndexError, match="non-zero size"):
        plan(16000, 16000, 0.01, 30, 85, 85)                         # lag_min >= lags // 2
    with pytest.raises(IndexError, match="non-zero size"):
        plan(16000, 16000, 0.01, 30, 85, 160)
    with pytest.raises(IndexError):
        plan(0, 16000, 0.01, 30, 85, 3400)                           # no frame
    for w in (0, 1, 2):
        with pytest.raises(ValueError, match="non-empty list"):
            plan(16000, 16000, 0.01, w, 85, 3400)
    with pytest.raises(RuntimeError, match="maximum size"):
        plan(160 * 15, 16000, 0.01, 30, 85, 3400)                     # 15 frames + 14 < 30
    assert plan(160 * 16, 16000, 0.01, 30, 85, 3400)[4] == 1
    with pytest.raises(NotImplementedError):
        plan(10 ** 6, 96000, 0.0854, 3, 20, 3400)                     # fs = 8199
    with pytest.raises(NotImplementedError):
        plan(10 ** 6, 96000, 0.01, 3, 5, 3400)                        # lags = 19200
    assert plan(10 ** 6, 96000, 0.085, 3, 20, 3400)[:2] == (4800, 8161)      # 96000 * 0.085 = 8160.000000000001
    # the restated reference raises the same types on CPU
    x = torch.randn(1, 160 * 15)
    with pytest.raises(RuntimeError, match="maximum size"):
        O.torch_reference(x, 16000)
    with pytest.raises(ValueError, match="non-empty list"):
        O.torch_reference(torch.randn(1, 16000), 16000, win_length=2)
    with pytest.raises(IndexError):
        O.torch_reference(torch.randn(1, 16000), 16000, freq_high=100)


# ---- CPU replay of csrc/pitch.h ------------------------------------------------------------------------------------------

_sim = None


def sim():
    global _sim
    if _sim is None:
        newest = max(os.path.getmtime(p) for p in [SIM_SRC] + HDRS)
        if not os.path.exists(SIM_OUT) or newest > os.path.getmtime(SIM_OUT):
            os.makedirs(os.path.dirname(SIM_OUT), exist_ok=True)
            tmp = "%s.tmp.%d" % (SIM_OUT, os.getpid())
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", SIM_SRC, "-o", tmp])
            os.replace(tmp, SIM_OUT)
        _sim = C.CDLL(SIM_OUT)
        i64, i32, p = C.c_int64, C.c_int, C.c_void_p
        for name in ("sim_pitch_f32", "sim_pitch_f64"):
            getattr(_sim, name).argtypes = [p, p, p] + [i64] * 3 + [i32] * 6 + [p]
    return _sim


def sim_pitch(x2, sr, fs, lags, lag_min, win, mode):
    """x2: numpy (rows, L) view with unit time stride.  -> (out, lags or None, (T, J, chunks, LDS bytes))"""
    assert x2.strides[-1] == x2.itemsize
    rows, L = x2.shape
    Fn = -(-L // fs)
    fn = sim().sim_pitch_f64 if x2.dtype == np.float64 else sim().sim_pitch_f32
    if mode == 1:
        out = np.zeros((rows, Fn, lags), x2.dtype)
    else:
        out = np.zeros((rows, max(Fn + (win - 1) // 2 - win + 1, 0)), np.float32)
    lag = np.zeros((rows, Fn), np.int32)
    geom = np.zeros(4, np.int64)
    rs = x2.strides[0] // x2.itemsize if rows > 1 else L
    assert fn(x2.ctypes.data, out.ctypes.data, lag.ctypes.data, rows, L, rs, sr, fs, lags, lag_min, win, mode,
              geom.ctypes.data) == 0
    return out, (lag if mode == 0 else None), tuple(int(v) for v in geom)


def _tones(sr, seconds, rows=2, seed=0):
    n = int(sr * seconds)
    x = np.stack([O.tone(n, sr, 100.0 + 70 * r, seed=seed + r) for r in range(rows)])
    x[-1, n // 3: n // 2] = 0.0
    return x


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_sim_nccf_meets_the_oracle(dtype):
    for sr, seconds in [(8000, 0.3), (16000, 0.35), (44100, 0.12)]:
        x = _tones(sr, seconds).astype(dtype)
        s = O.sizes(x.shape[-1], sr)
        got, _, _ = sim_pitch(x, sr, s["fs"], s["lags"], 0, 3, 1)
        # (float64: the direct form; a prefix-sum difference cancels down to ~1e-16 of its frame segment's energy, and a
        # window near silence can hold far less than that)
        want = (O.nccf_prefix if dtype == np.float32 else O.nccf_loops)(x.astype(np.float64), s["fs"], s["lags"])
        peak = np.abs(want).max(-1, keepdims=True)
        tol = 1e-5 if dtype == np.float32 else 1e-12
        assert (np.abs(got - want) <= tol * peak).all(), sr
        silent = peak[..., 0] == 0
        assert silent.any() and (got[silent] == 0).all()


def test_sim_pick_and_median_are_the_oracles_on_its_own_nccf():
    for sr in (8000, 16000, 22050):
        x = _tones(sr, 0.4, rows=3, seed=5)
        s = O.sizes(x.shape[-1], sr)
        nccf, _, _ = sim_pitch(x, sr, s["fs"], s["lags"], 0, 3, 1)
        for win in (3, 4, 30):
            out, lag, _ = sim_pitch(x, sr, s["fs"], s["lags"], s["lag_min"], win, 0)
            np.testing.assert_array_equal(lag, O.pick(nccf, s["lag_min"]))
            np.testing.assert_array_equal(out, O.smooth(lag, win, sr))


def test_sim_lag_tiling_and_lds_boundaries():
    rng = np.random.default_rng(3)
    # (sr, fs, lags, dtype): one chunk with several frames per tile; one frame per tile; lags in chunks (64 KiB and
    # 160 KiB budgets); the largest supported sizes are exercised by planning only (the replay would take minutes)
    for sr, fs, lags, dtype in [(16000, 160, 189, np.float32), (96000, 960, 4800, np.float32),
                                (96000, 2000, 5000, np.float32), (96000, 8192, 1000, np.float64),
                                (16000, 16, 3000, np.float64)]:
        L = fs * 3 + 5
        x = rng.standard_normal((1, L)).astype(dtype)
        got, _, geom = sim_pitch(x, sr, fs, lags, 0, 3, 1)
        T, J, chunks, lds = geom
        assert lds <= 160 * 1024 and J * chunks >= lags and (chunks == 1 or T == 1)
        want = O.nccf_loops(x.astype(np.float64), fs, lags)
        peak = np.abs(want).max(-1, keepdims=True)
        tol = 1e-5 if dtype == np.float32 else 1e-12
        assert (np.abs(got - want) <= tol * peak).all(), (fs, lags)
        if chunks > 1:
            lm = lags // 4
            _, lag, _ = sim_pitch(x, sr, fs, lags, lm, 3, 0)
            np.testing.assert_array_equal(lag, O.pick(got, lm))


def test_sim_plan_covers_the_supported_range():
    for dtype in (np.float32, np.float64):
        for fs, lags in [(8192, 16384), (8192, 1), (1, 16384), (4096, 12000), (160, 189), (441, 519)]:
            x = np.zeros((1, 1), dtype)
            _, _, (T, J, chunks, lds) = sim_pitch(x, 96000, fs, lags, 0, 3, 1)
            assert lds <= 160 * 1024 and T >= 1 and J >= 1 and J * chunks >= lags


# ---- op surface without a device ----------------------------------------------------------------------------------------

def test_meta_shapes():
    op = torch.ops.audio_amd.detect_pitch_frequency
    for shape, sr in [((16000,), 16000), ((2, 16000), 16000), ((2, 3, 4, 8000), 8000), ((1, 44100), 44100)]:
        y = op(torch.empty(shape, device="meta"), sr, 0.01, 30, 85, 3400)
        assert y.dtype == torch.float32 and tuple(y.shape) == tuple(shape[:-1]) + (100 - 15,)
    for dt in (torch.float16, torch.bfloat16, torch.float64):
        assert op(torch.empty(2, 4000, device="meta", dtype=dt), 8000, 0.01, 3, 85, 3400).dtype == torch.float32
    y = op(torch.empty(2, 4000, device="meta"), 8000, 0.025, 4, 100, 2000)
    assert tuple(y.shape) == (2, 20 + 1 - 4 + 1)
    with pytest.raises(RuntimeError, match="maximum size"):
        op(torch.empty(2, 100, device="meta"), 8000, 0.01, 30, 85, 3400)


def test_torchscript_function():
    sf = torch.jit.script(F.detect_pitch_frequency)
    assert "audio_amd::detect_pitch_frequency" in str(sf.graph)


def test_cpu_tensors_are_refused():
    x = torch.randn(2, 16000)
    with pytest.raises(NotImplementedError, match="CPU"):
        torch.ops.audio_amd.detect_pitch_frequency(x, 16000, 0.01, 30, 85, 3400)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.detect_pitch_frequency(x, 16000)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.detect_pitch_frequency(x.half(), 16000)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F._compute_nccf(x, 16000, 0.01, 85)
