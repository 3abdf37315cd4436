"""F.vad / F.vad_start / T.Vad without a GPU: a CPU replay of csrc/vad.h (the three measurement kernels and the two trigger
kernels, with the launch geometry of the C ABI) against tests/vad_oracle.py -- the trigger exactly, the measurements within
4 x the difference of the oracle's own float32 and float64 forms -- the oracle's end-to-end statistics, the host's plan and
tables, signatures, error types, the warning and the refusal of CPU tensors."""
import ctypes as C
import inspect
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import vad_cases as K
import vad_oracle as O
import audio_amd.functional as F
import audio_amd.transforms as T
from audio_amd import _host

HERE = os.path.dirname(os.path.abspath(__file__))
SIM_SRC = os.path.join(HERE, "cpu_sim", "sim_vad.cpp")
SIM_OUT = os.path.join(HERE, "cpu_sim", "_build", "libaamd_sim_vad.so")
HDRS = [os.path.join(os.path.dirname(HERE), "audio_amd", "csrc", h) for h in ("vad.h", "wave_augment.h", "spec_augment.h", "hd.h")]
CODE = {torch.float32: 0, torch.float64: 1, torch.float16: 2, torch.bfloat16: 3}

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
        i64, i32, p, d = C.c_int64, C.c_int, C.c_void_p, C.c_double
        _sim.sim_vad_frames.argtypes, _sim.sim_vad_frames.restype = [i64] * 3, i64
        _sim.sim_vad_measure.argtypes = [i32, p, i64, i64, i64] + [i32] * 8 + [d] * 4 + [p, p, p]
        _sim.sim_vad_trigger.argtypes = [p] + [i64] * 6 + [d, d, p, p, p]
    return _sim


class Replay:
    """The backend of vad_cases: the kernels' phase functions on the CPU, the host code of the product around them."""

    @staticmethod
    def tensor(a):
        return torch.from_numpy(np.array(a))

    @staticmethod
    def measures(x, sample_rate, **kw):
        pl = F._vad_plan(sample_rate, **dict(O.DEFAULTS, **kw))
        rows, T_ = x.shape
        frames = F._vad_frames(T_, pl)
        assert frames == sim().sim_vad_frames(T_, pl.L, pl.P) == O.n_frames(T_, pl)
        nb = pl.s1 - pl.s0
        tables = _host.vad_tables(pl.L, nb, pl.N)
        ws = np.full(max(rows * frames * nb, 1), np.nan, np.float32)
        meas = np.full((rows, frames), np.nan, np.float32)
        assert x.stride(1) == 1
        rc = sim().sim_vad_measure(CODE[x.dtype], x.data_ptr(), rows, T_, x.stride(0), pl.L, pl.N, pl.P, pl.s0, pl.s1, pl.c0,
                                   pl.c1, pl.boot_max, pl.smooth, pl.up, pl.down, pl.nra, tables.ctypes.data, ws.ctypes.data,
                                   meas.ctypes.data)
        assert rc == 0
        return meas

    @staticmethod
    def trigger(meas, pl):
        meas = np.ascontiguousarray(meas, dtype=np.float32)
        rows, frames = meas.shape
        first, start = np.full(rows, -7, np.int64), np.full(rows, -7, np.int64)
        joint = np.full(1, -7, np.int64)
        assert sim().sim_vad_trigger(meas.ctypes.data, rows, frames, pl.M, pl.gap, pl.P, pl.fixed, pl.level, pl.trig,
                                     first.ctypes.data, start.ctypes.data, joint.ctypes.data) == 0
        return first, start, joint[0]


# ---- 1. the trigger, exact -------------------------------------------------------------------------------------------------

def test_trigger_equals_the_oracle_on_synthetic_measurements():
    grid = K.trigger_grid()
    assert len(grid) == 4 * 3 * 2 * 3 * 2
    hit = 0
    for name, meas, pl in grid:
        K.check_trigger(Replay, name, meas, pl)
        hit += any(O.trigger_row(row, pl)[0] >= 0 for row in meas)
    assert hit > len(grid) // 2                       # the draw does trigger


@pytest.mark.parametrize("case", K.constructed_cases(), ids=lambda c: c[0])
def test_trigger_constructed_cases(case):
    K.check_trigger(Replay, *case)


def test_trigger_start_is_clamped_at_zero():
    meas = np.full((1, 8), 20.0, np.float32)
    pl = K.trig_plan(20, 5, 800, 10 ** 6)
    first, start, joint = Replay.trigger(meas, pl)
    assert first[0] >= 0 and start[0] == 0 and joint == 0


# ---- 2. the measurements ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(O.GROUPS))
def test_measures_within_the_oracles_own_float32_error(name):
    K.check_measures(Replay, name)


def test_measures_row_counts_offsets_and_strides():
    K.check_row_counts_and_offsets(Replay)


def test_measures_nan_row_leaves_the_clean_rows_alone():
    K.check_nan_row(Replay)


def test_measures_rows_of_l_and_l_plus_one_samples():
    K.check_short_rows(Replay)


def test_group_shapes_are_the_ones_the_issue_lists():
    shapes = {n: O.plan(g[0], **g[4]) for n, g in O.GROUPS.items()}
    assert (shapes["8k"].L, shapes["8k"].N, shapes["8k"].s1) == (800, 1024, 512)
    assert shapes["16k"].N == 2048 and (shapes["44k"].L, shapes["44k"].N) == (4410, 8192)
    assert (shapes["16k_md064"].L, shapes["16k_md064"].N) == (1024, 1024)
    assert (shapes["16k_md064p"].L, shapes["16k_md064p"].N) == (1025, 2048)
    assert shapes["16k_boot0"].boot_max == 0 and shapes["16k"].boot_max == 6


# ---- 3. / 4. consistency and end to end ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", O.E2E)
def test_oracle_statistics_of_the_end_to_end_cases(name):
    x, sr, kw, m64, u64, _ = O.group(name)
    m32 = O.group_m32(name)
    pl = O.plan(sr, **kw)
    tol = O.tolerance(sr)
    kept = [r for r in range(len(x)) if O.has_margin(m64[r], u64[r], pl, tol)]
    assert 4 * (len(x) - len(kept)) <= len(x)
    voiced = [r for r in range(len(x)) if O.is_voiced(r)]
    assert 3 * sum(O.trigger_row(m64[r], pl)[0] >= 0 for r in voiced) >= len(voiced)
    for r in kept:
        assert O.trigger_row(m32[r], pl) == O.trigger_row(m64[r], pl), r
    for r in range(len(x)):                          # nothing triggers before the voice starts
        f = O.trigger_row(m64[r], pl)[0]
        assert f < 0 or O.is_voiced(r)


@pytest.mark.parametrize("name", O.E2E)
def test_replay_end_to_end_equals_the_float64_oracle(name):
    K.check_end_to_end(Replay, name)


# ---- the host's plan and tables ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sr,kw", [(8000, {}), (16000, {}), (44100, {}), (22050, dict(measure_freq=25.0, search_time=1.63)),
                                   (16000, dict(measure_duration=0.064, boot_time=0.0, allowed_gap=0.0, pre_trigger_time=0.3)),
                                   (48000, dict(trigger_level=5.5, lp_filter_freq=30000.0, hp_lifter_freq=100.0))])
def test_plan_equals_the_oracles(sr, kw):
    got = F._vad_plan(sr, **dict(O.DEFAULTS, **kw))
    assert tuple(got) == tuple(O.plan(sr, **kw)) and got._fields == O.Plan._fields


def test_tables_are_the_float64_windows_rounded_once():
    pl = O.plan(16000)
    w, cw = O.windows(pl)
    t = _host.vad_tables(pl.L, pl.s1 - pl.s0, pl.N)
    assert t.dtype == np.float32 and t.shape == (pl.L + pl.s1 - pl.s0 + pl.N,)
    assert np.array_equal(t[:pl.L], w.astype(np.float32)) and np.array_equal(t[pl.L:pl.L + len(cw)], cw.astype(np.float32))
    tw = t[pl.L + len(cw):].reshape(-1, 2).astype(np.float64)
    k = np.arange(pl.N // 2)
    assert np.max(np.abs(tw[:, 0] + 1j * tw[:, 1] - np.exp(-2j * math.pi * k / pl.N))) < 1e-7


# ---- 5. the surface ---------------------------------------------------------------------------------------------------------

NAMES = ["trigger_level", "trigger_time", "search_time", "allowed_gap", "pre_trigger_time", "boot_time", "noise_up_time",
         "noise_down_time", "noise_reduction_amount", "measure_freq", "measure_duration", "measure_smooth_time", "hp_filter_freq",
         "lp_filter_freq", "hp_lifter_freq", "lp_lifter_freq"]
VALUES = [7.0, 0.25, 1.0, 0.25, 0.0, 0.35, 0.1, 0.01, 1.35, 20.0, None, 0.4, 50.0, 6000.0, 150.0, 2000.0]


@pytest.mark.parametrize("fn", [F.vad, F.vad_start, F._vad_measures])
def test_signatures_and_defaults(fn):
    ps = list(inspect.signature(fn).parameters.values())
    assert [p.name for p in ps] == ["waveform", "sample_rate"] + NAMES
    assert [p.default for p in ps[2:]] == VALUES and all(p.default is inspect.Parameter.empty for p in ps[:2])


def test_module_signature_and_state():
    ps = list(inspect.signature(T.Vad.__init__).parameters.values())[1:]
    assert [p.name for p in ps] == ["sample_rate"] + NAMES and [p.default for p in ps[1:]] == VALUES
    m = T.Vad(16000, trigger_level=6.0)
    assert isinstance(m, torch.nn.Module) and len(m.state_dict()) == 0 and not list(m.buffers()) and m.trigger_level == 6.0


def test_names_are_exported():
    assert {"vad", "vad_start", "vad_tiles"} <= set(F.__all__) and "Vad" in T.__all__
    assert callable(F._vad_measures) and callable(F.vad_tiles)
    assert sim().sim_vad_tiles(1) >= 8192 and sim().sim_vad_tiles(2) == 16 and sim().sim_vad_tiles(3) == 64


@pytest.mark.parametrize("fn", [F.vad, F.vad_start, F._vad_measures])
def test_errors(fn):
    x = torch.zeros(2, 4000)
    with pytest.raises(ValueError, match="cepstrum_start"):
        fn(x, 16000, hp_lifter_freq=3000.0)
    with pytest.raises(ValueError, match="spectrum"):
        fn(x, 16000, hp_filter_freq=7000.0)
    for kw in (dict(measure_freq=0.0), dict(trigger_time=0.0), dict(search_time=-1.0), dict(noise_up_time=0.0),
               dict(noise_down_time=0.0), dict(measure_smooth_time=0.0), dict(measure_duration=0.0), dict(boot_time=-0.1),
               dict(measure_duration=1e-9), dict(measure_freq=float("nan"))):
        with pytest.raises(ValueError):
            fn(x, 16000, **kw)
    for sr in (0, -16000):
        with pytest.raises(ValueError):
            fn(x, sr)
    with pytest.raises(TypeError):
        fn(torch.zeros(2, 4000, dtype=torch.int16), 16000)
    with pytest.raises(NotImplementedError, match="8192"):
        fn(x, 96000)
    with pytest.raises(RuntimeError, match="MI355X"):
        fn(x, 16000)
    with pytest.raises(RuntimeError, match="forward-only"):
        fn(x.clone().requires_grad_(True), 16000)
    with torch.no_grad(), pytest.raises(RuntimeError, match="MI355X"):
        fn(x.clone().requires_grad_(True), 16000)


def test_three_dimensions_warn_and_name_vad_start():
    with pytest.warns(UserWarning, match="vad_start"), pytest.raises(RuntimeError, match="MI355X"):
        F.vad(torch.zeros(2, 2, 4000), 16000)
    with pytest.warns(UserWarning, match="vad_start"), pytest.raises(RuntimeError, match="MI355X"):
        T.Vad(16000)(torch.zeros(2, 2, 4000))


def test_defaults_up_to_81_9_khz_are_served():
    assert F._vad_plan(81900, *VALUES).N == 8192
    with pytest.raises(NotImplementedError):
        F._vad_plan(82000, *VALUES)
