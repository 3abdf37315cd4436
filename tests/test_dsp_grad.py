"""The backward kernels of oscillator_bank and filter_waveform without a GPU: a CPU replay of csrc/dsp_synth_grad.h (the kernels'
phase functions with the launch geometry and the workspaces of the C ABI) against tests/dsp_grad_oracle.py on the shapes that
straddle the scan's chunk, the filter's tile and the two constants the backward adds (the piece of time and the tile of lags of
the filter-gradient reduction); the oracle against central differences of the forward's definition; the bit-exact properties
(two calls, rows, shared against batched filters, the prefix of the amplitude gradient, dead oscillators, poisoning, the
footprint of a non-finite cotangent); the ABI's new symbols."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import dsp_cases as K
import dsp_grad_cases as GK
import dsp_grad_oracle as G
import dsp_oracle as O
import audio_amd.functional as F
from audio_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
SIM_SRC = os.path.join(HERE, "cpu_sim", "sim_dsp_grad.cpp")
SIM_OUT = os.path.join(HERE, "cpu_sim", "_build", "libaamd_sim_dsp_grad.so")
HDRS = [os.path.join(os.path.dirname(HERE), "audio_amd", "csrc", h)
        for h in ("dsp_synth_grad.h", "dsp_synth.h", "wave_augment.h", "spec_augment.h", "hd.h")]
CODE = {torch.float32: 0, torch.float64: 1, torch.float16: 2, torch.bfloat16: 3}
RED = {"sum": 0, "mean": 1, "none": 2}

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
        _sim.sim_oscillator_bank_grad.argtypes = [i32, p, p, p, p, p, i64, i64, i64, i64, i64, d, i32]
        _sim.sim_filter_waveform_grad.argtypes = [i32, p, p, p, p, p, i64, i64, i64, i64, i32, i32]
    return _sim


class Replay:
    """The backend of dsp_grad_cases: the kernels' phase functions on the CPU."""

    @staticmethod
    def grad_tiles():
        return tuple(sim().sim_dsp_grad_tiles(i) for i in range(2))

    @staticmethod
    def osc_grad(f, a, g, sample_rate, reduction, want=(True, True), rc=0):
        f, a, g = f.contiguous(), a.contiguous(), g.contiguous()
        rows, T, N = f.shape
        gf = torch.full((rows, T, N), 7.0, dtype=f.dtype) if want[0] else None
        ga = torch.full((rows, T, N), 7.0, dtype=f.dtype) if want[1] else None
        assert sim().sim_oscillator_bank_grad(CODE[f.dtype], f.data_ptr(), a.data_ptr(), g.data_ptr(),
                                              gf.data_ptr() if want[0] else None, ga.data_ptr() if want[1] else None, rows, T, N,
                                              T * N, T * N, sample_rate, RED[reduction]) == rc
        return gf, ga

    @staticmethod
    def fw_grad(x, h, g, want=(True, True), rc=0):
        x, h, g = x.contiguous(), h.contiguous(), g.contiguous()
        rows, T = x.shape
        gx = torch.full((rows, T), 7.0, dtype=x.dtype) if want[0] else None
        gh = torch.full(tuple(h.shape), 7.0, dtype=x.dtype) if want[1] else None
        assert sim().sim_filter_waveform_grad(CODE[x.dtype], x.data_ptr(), h.data_ptr(), g.data_ptr(),
                                              gx.data_ptr() if want[0] else None, gh.data_ptr() if want[1] else None, rows, T, T,
                                              h.shape[-2], h.shape[-1], 1 if h.dim() == 3 else 0) == rc
        return gx, gh


# ---- 1. structure and the oracle ---------------------------------------------------------------------------------------------------

def test_tiles_are_what_the_cases_straddle():
    assert Replay.grad_tiles() == (GK.PIECE, GK.LAGS)
    assert {"aamd_filter_waveform_grad", "aamd_filter_waveform_grad_workspace", "aamd_oscillator_bank_grad",
            "aamd_oscillator_grad_workspace", "aamd_dsp_grad_tiles"} <= set(_lib.EXPORTED_SYMBOLS)
    assert "dsp_grad_tiles" in F.__all__ and len(F.dsp_tiles.__doc__) > 0
    if os.path.exists(_lib.LIB_PATH):
        assert F.dsp_grad_tiles() == Replay.grad_tiles()
        assert len(F.dsp_tiles()) == 5


def test_the_oracle_is_the_derivative_of_the_definition():
    """Central differences of dsp_oracle's forwards in longdouble, at a handful of elements."""
    rng = np.random.default_rng(2)
    f = rng.uniform(100.0, 3000.0, (1, 9, 2))
    f[0, 4, 1] = 9000.0                                            # a dead step: it receives from the live steps after it
    a = rng.uniform(-1.0, 1.0, (1, 9, 2))
    for red in ("sum", "mean", "none"):
        g = rng.standard_normal((1, 9, 2) if red == "none" else (1, 9))
        gf, ga, _, _ = G.oscillator_bank_grad(f, a, g, K.SR, red, acc=G.LD)

        def loss(f_, a_):
            return (O.oscillator_bank(f_, a_, K.SR, red, acc=G.LD)[0] * g.astype(G.LD)).sum()
        assert ga[0, 4, 1] == 0 and gf[0, 4, 1] != 0
        for t, n in ((0, 0), (4, 1), (8, 1), (3, 0), (7, 0)):
            for which, want, step in ((0, gf, 1e-2), (1, ga, 1e-4)):
                hi, lo = [f.copy(), a.copy()], [f.copy(), a.copy()]
                hi[which][0, t, n] += step
                lo[which][0, t, n] -= step
                num = (loss(*hi) - loss(*lo)) / G.LD(hi[which][0, t, n] - lo[which][0, t, n])
                assert abs(num - want[0, t, n]) <= 1e-6 * max(abs(want[0, t, n]), np.abs(want).max() * 1e-3), (red, t, n, which)
    x, g = rng.standard_normal((1, 12)), rng.standard_normal((1, 12))
    for h in (rng.standard_normal((3, 4)), rng.standard_normal((1, 3, 4))):
        gx, _, gh, _, terms = G.filter_waveform_grad(x, h, g, acc=G.LD)
        assert terms.max() == 4 and terms.min() >= 2

        def loss(x_, h_):
            return (O.filter_waveform(x_, h_, acc=G.LD)[0] * g.astype(G.LD)).sum()
        for m in (0, 3, 4, 11):
            hi, lo = x.copy(), x.copy()
            hi[0, m] += 0.25
            lo[0, m] -= 0.25
            assert abs((loss(hi, h) - loss(lo, h)) / G.LD(0.5) - gx[0, m]) <= 1e-12
        for idx in ((0, 0), (1, 3), (2, 1), (2, 3)):
            idx = idx if h.ndim == 2 else (0,) + idx
            hi, lo = h.copy(), h.copy()
            hi[idx] += 0.25
            lo[idx] -= 0.25
            assert abs((loss(x, hi) - loss(x, lo)) / G.LD(0.5) - gh[idx]) <= 1e-12


# ---- 2. accuracy -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("N", K.OSC_N)
@pytest.mark.parametrize("T", K.OSC_T)
def test_oscillator_bank_grad_within_the_bars(T, N, dt):
    GK.check_osc_grad(Replay, 2, T, N, dt)


@pytest.mark.parametrize("dt", list(K.DTYPES))
@pytest.mark.parametrize("reduction", ["sum", "mean", "none"])
def test_oscillator_bank_grad_reductions_and_half_types(reduction, dt):
    GK.check_osc_grad(Replay, 2, K.CH + 1, 3, dt, reduction)


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("batched", [False, True])
@pytest.mark.parametrize("shape", GK.FW_GRAD_SHAPES)
def test_filter_waveform_grad_within_the_bars(shape, batched, dt):
    GK.check_fw_grad(Replay, *shape, dt, batched)


@pytest.mark.parametrize("dt", list(K.DTYPES))
def test_filter_waveform_grad_half_types_and_one_filter_over_three_rows(dt):
    for batched in (False, True):
        GK.check_fw_grad(Replay, 2 * K.TILE, 2, 5, dt, batched)
        GK.check_fw_grad(Replay, *GK.FW_ONE_FILTER, dt, batched, rows=3)


# ---- 3. exact properties ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_oscillator_grad_prefix_rows_and_poison(dt):
    GK.check_osc_grad_prefix(Replay, dt)
    GK.check_osc_grad_rows(Replay, dt)
    GK.check_osc_grad_poison(Replay, dt)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_filter_grad_rows_shared_filters_and_non_finite_cotangents(dt):
    GK.check_fw_grad_exact(Replay, dt)
    GK.check_fw_grad_nonfinite_stays_under_its_filter(Replay)


def test_only_the_wanted_gradients_are_written():
    GK.check_only_what_is_wanted(Replay)


def test_replay_refuses_what_the_abi_refuses():
    x, h = K.fw_inputs(96, 3, 129, "f32", False)
    g = GK.fw_cotangent(96, "f32")
    Replay.fw_grad(x[:, :95], h, g[:, :95], rc=-1)
    Replay.fw_grad(x, torch.zeros(1, F.DSP_MAX_TAPS + 1), g, rc=-2)
    f = torch.zeros(1, 2, F.DSP_MAX_OSCILLATORS + 1)
    Replay.osc_grad(f, f, torch.zeros(1, 2), K.SR, "sum", rc=-2)
