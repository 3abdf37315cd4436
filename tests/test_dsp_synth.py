"""The synthesis ops of audio_amd.prototype.functional without a GPU: a CPU replay of csrc/dsp_synth.h (the kernels' phase
functions with the launch geometry of the C ABI) against tests/dsp_oracle.py on the shapes that straddle the chunk of the
oscillator scan and the tile of the filter, the bit-exact properties (prefix, rows, shared against batched filters,
poisoning), the pinned difference from the reference's unreduced float32 phase, the host code (the ADSR ramp, the cosine
table), signatures, error types and the refusal of CPU tensors."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest
import torch

import dsp_cases as K
import dsp_oracle as O
import audio_amd.functional as F
from audio_amd import _host, _lib

HERE = os.path.dirname(os.path.abspath(__file__))
SIM_SRC = os.path.join(HERE, "cpu_sim", "sim_dsp.cpp")
SIM_OUT = os.path.join(HERE, "cpu_sim", "_build", "libaamd_sim_dsp.so")
HDRS = [os.path.join(os.path.dirname(HERE), "audio_amd", "csrc", h) for h in ("dsp_synth.h", "wave_augment.h", "spec_augment.h", "hd.h")]
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
        _sim.sim_oscillator_bank.argtypes = [i32, p, p, p, i64, i64, i64, i64, i64, d, i32]
        _sim.sim_filter_waveform.argtypes = [i32, p, p, p, i64, i64, i64, i64, i32, i32]
        _sim.sim_sinc_impulse_response.argtypes = [i32, p, p, i64, i32, i32]
        _sim.sim_frequency_impulse_response.argtypes = [i32, p, p, p, i64, i32]
        _sim.sim_extend_pitch.argtypes = [i32, p, p, p, i64, i64]
    return _sim


class Replay:
    """The backend of dsp_cases: the kernels' phase functions on the CPU, the host's tables around them."""

    @staticmethod
    def tiles():
        return tuple(sim().sim_dsp_tiles(i) for i in range(5))

    @staticmethod
    def osc(f, a, sample_rate, reduction, rc=0):
        f, a = f.contiguous(), a.contiguous()
        rows, T, N = f.shape
        out = torch.full((rows, T, N) if reduction == "none" else (rows, T), 7.0, dtype=f.dtype)
        assert sim().sim_oscillator_bank(CODE[f.dtype], f.data_ptr(), a.data_ptr(), out.data_ptr(), rows, T, N, T * N, T * N,
                                         sample_rate, RED[reduction]) == rc
        return out

    @staticmethod
    def fw(x, h, rc=0):
        x, h = x.contiguous(), h.contiguous()
        rows, T = x.shape
        out = torch.full((rows, T), 7.0, dtype=x.dtype)
        assert sim().sim_filter_waveform(CODE[x.dtype], x.data_ptr(), h.data_ptr(), out.data_ptr(), rows, T, T, h.shape[-2],
                                         h.shape[-1], 1 if h.dim() == 3 else 0) == rc
        return out

    @staticmethod
    def sinc(cutoff, window_size, high_pass, rc=0):
        c1 = cutoff.contiguous().reshape(-1)
        out = torch.full(tuple(cutoff.shape) + (window_size,), 7.0, dtype=cutoff.dtype)
        assert sim().sim_sinc_impulse_response(CODE[cutoff.dtype], c1.data_ptr(), out.data_ptr(), c1.shape[0], window_size,
                                               1 if high_pass else 0) == rc
        return out

    @staticmethod
    def fir(m, rc=0):
        m = m.contiguous()
        n = m.shape[-1]
        table = _host.round_once(_host.fir_cos_table(n), m.dtype)
        out = torch.full(tuple(m.shape[:-1]) + (2 * (n - 1),), 7.0, dtype=m.dtype)
        assert sim().sim_frequency_impulse_response(CODE[m.dtype], m.data_ptr(), table.data_ptr(), out.data_ptr(),
                                                    m.numel() // n, n) == rc
        return out

    @staticmethod
    def pitch(base, pat):
        b1, p1 = base.contiguous().reshape(-1), pat.contiguous()
        out = torch.full(tuple(base.shape[:-1]) + (p1.shape[0],), 7.0, dtype=base.dtype)
        assert sim().sim_extend_pitch(CODE[base.dtype], b1.data_ptr(), p1.data_ptr(), out.data_ptr(), b1.shape[0], p1.shape[0]) == 0
        return out


# ---- 1. structure ----------------------------------------------------------------------------------------------------------------

def test_tiles_are_what_the_cases_straddle():
    assert Replay.tiles() == (K.CH, K.TILE, F.DSP_MAX_TAPS, F.DSP_MAX_OSCILLATORS, F.DSP_MAX_MAGNITUDES)
    assert F.DSP_MAX_TAPS >= 2049 and F.DSP_MAX_MAGNITUDES >= 4097
    if os.path.exists(_lib.LIB_PATH):
        assert F.dsp_tiles() == Replay.tiles()


def test_oscillator_lds_fits_for_every_count():
    reserved = sim().sim_osc_lds_reserved()
    assert max(sim().sim_osc_lds(n) for n in range(1, F.DSP_MAX_OSCILLATORS + 1)) <= reserved
    assert 2 * reserved * 8 + 2 * 256 * 8 <= 64 * 1024               # float64 values and the two float64 columns, static LDS


def test_the_two_forms_of_the_filter_agree():
    for T, Fn, L in ((96, 3, 129), (96, 96, 6), (60, 4, 1), (64, 2, 8)):       # odd and even L, num_filters == time
        rng = np.random.default_rng(L)
        x, h = rng.standard_normal(T), rng.standard_normal((Fn, L))
        y, mag = O.filter_waveform(x[None], h)
        assert np.abs(y[0] - O.filter_waveform_overlap_add(x, h)).max() <= 16 * 2.0 ** -53 * mag.max()


# ---- 2. accuracy -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("N", K.OSC_N)
@pytest.mark.parametrize("T", K.OSC_T)
def test_oscillator_bank_within_the_bar(T, N, dt):
    K.check_osc(Replay, 2, T, N, dt)


@pytest.mark.parametrize("dt", list(K.DTYPES))
@pytest.mark.parametrize("reduction", ["mean", "none"])
def test_oscillator_bank_reductions_and_half_types(reduction, dt):
    K.check_osc(Replay, 2, K.CH + 1, 3, dt, reduction)
    K.check_osc(Replay, 2, K.CH + 1, 65, dt, "sum")


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_oscillator_bank_long_phase(dt):
    K.check_osc(Replay, 1, 40 * K.CH, 2, dt)


def test_the_references_unreduced_float32_phase_misses_the_bar_by_three_orders():
    T, N = 40 * K.CH, 2
    f, a = K.osc_inputs(1, T, N, "f32")
    want, mag, _ = K.osc_oracle(1, T, N, "f32", "sum")
    bar = K.osc_bar(want, mag, 0.0, N, "f32", "sum")
    err = np.abs(O.oscillator_bank_unreduced_f32(K.wide(f), K.wide(a), K.SR) - want)
    print(f"the unreduced float32 phase: {float((err[bar > 0] / bar[bar > 0]).max()):.0f} x the bar")
    pos = bar > 0                                                # both oscillators can be dead: no ratio where the bar is 0
    assert (err[pos] >= 1000.0 * bar[pos]).any() and (err[pos] > bar[pos]).mean() > 0.9


@pytest.mark.parametrize("dt", list(K.DTYPES))
@pytest.mark.parametrize("batched", [False, True])
@pytest.mark.parametrize("shape", K.FW_SHAPES)
def test_filter_waveform_within_the_bar(shape, batched, dt):
    K.check_fw(Replay, *shape, dt, batched)


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("high_pass", [False, True])
@pytest.mark.parametrize("W", K.SINC_W)
def test_sinc_impulse_response_within_the_bar(W, high_pass, dt):
    K.check_sinc(Replay, W, high_pass, dt)
    K.check_sinc_batch(Replay, dt)


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("n", K.FIR_N)
def test_frequency_impulse_response_within_the_bar(n, dt):
    K.check_fir(Replay, n, dt)


@pytest.mark.parametrize("dt", list(K.DTYPES))
def test_extend_pitch_is_the_product_rounded_once(dt):
    K.check_pitch(Replay, dt)


# ---- 3. exact properties ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_oscillator_prefix_rows_and_poison(dt):
    K.check_osc_prefix(Replay, dt)
    K.check_osc_rows(Replay, dt)
    K.check_osc_poison(Replay, dt)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_filter_rows_shared_filters_and_non_finite_samples(dt):
    K.check_fw_shared_equals_expanded(Replay, dt)
    K.check_fw_rows(Replay, dt)
    K.check_fw_nonfinite_stays_under_its_filter(Replay)


def test_replay_refuses_what_the_abi_refuses():
    x, h = K.fw_inputs(96, 3, 129, "f32", False)
    Replay.fw(x[:, :95], h, rc=-1)
    Replay.fw(x, torch.zeros(1, F.DSP_MAX_TAPS + 1), rc=-2)
    f, a = torch.zeros(1, 2, F.DSP_MAX_OSCILLATORS + 1), torch.zeros(1, 2, F.DSP_MAX_OSCILLATORS + 1)
    Replay.osc(f, a, K.SR, "sum", rc=-2)
    Replay.sinc(torch.tensor([0.5]), 4, False, rc=-1)


# ---- 4. the host code --------------------------------------------------------------------------------------------------------------

def test_adsr_ramp_is_the_oracles():
    cases = [dict(), dict(attack=1.0), dict(attack=0.2, hold=0.1, decay=0.3, sustain=0.4, release=0.25, n_decay=3),
             dict(attack=0.5, release=0.5, sustain=0.7), dict(decay=1.0, sustain=0.0, n_decay=1), dict(hold=0.33, sustain=0.5)]
    for kw in cases:
        for num in (1, 2, 7, 100, 1001):
            full = dict(attack=0.0, hold=0.0, decay=0.0, sustain=1.0, release=0.0, n_decay=2)
            full.update(kw)
            got = _host.adsr_ramp(num, **full)
            assert got.dtype == np.float64 and np.array_equal(got, O.adsr_envelope(num, **full))
    assert np.array_equal(_host.adsr_ramp(5, 0.0, 0.0, 0.0, 1.0, 0.0, 2), np.ones(5))
    assert np.array_equal(_host.adsr_ramp(5, 1.0, 0.0, 0.0, 1.0, 0.0, 2), [0.0, 0.25, 0.5, 0.75, 1.0])
    assert np.array_equal(_host.adsr_ramp(1, 1.0, 0.0, 0.0, 0.3, 0.0, 2), [0.3])


def test_cosine_table():
    for n in (2, 3, 129, 513):
        N = 2 * (n - 1)
        t = _host.fir_cos_table(n)
        assert t.shape == (N,) and t[0] == 1.0 and t[N // 2] == -1.0
        assert np.abs(t - np.cos(2 * np.pi * np.arange(N) / N)).max() <= 2.0 ** -52


# ---- 5. the public surface ---------------------------------------------------------------------------------------------------------

def test_signatures_and_exports():
    p = inspect.signature(F.oscillator_bank).parameters
    assert list(p) == ["frequencies", "amplitudes", "sample_rate", "reduction", "dtype"]
    assert (p["reduction"].default, p["dtype"].default) == ("sum", torch.float64)
    assert list(inspect.signature(F.filter_waveform).parameters) == ["waveform", "kernels"]
    p = inspect.signature(F.sinc_impulse_response).parameters
    assert list(p) == ["cutoff", "window_size", "high_pass"] and (p["window_size"].default, p["high_pass"].default) == (513, False)
    assert list(inspect.signature(F.frequency_impulse_response).parameters) == ["magnitudes"]
    p = inspect.signature(F.adsr_envelope).parameters
    assert list(p) == ["num_frames", "attack", "hold", "decay", "sustain", "release", "n_decay", "dtype", "device"]
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(p)[1:])
    assert [p[k].default for k in list(p)[1:]] == [0.0, 0.0, 0.0, 1.0, 0.0, 2, None, None]
    assert list(inspect.signature(F.extend_pitch).parameters) == ["base_frequency", "pattern"]
    names = {"oscillator_bank", "filter_waveform", "sinc_impulse_response", "frequency_impulse_response", "adsr_envelope", "extend_pitch"}
    assert names | {"dsp_tiles"} <= set(F.__all__)
    import audio_amd.prototype.functional as P
    assert names <= set(P.__all__) and all(getattr(P, n) is getattr(F, n) for n in names)
    assert {"aamd_dsp_tiles", "aamd_oscillator_bank", "aamd_oscillator_workspace", "aamd_filter_waveform", "aamd_sinc_impulse_response",
            "aamd_frequency_impulse_response", "aamd_extend_pitch"} <= set(_lib.EXPORTED_SYMBOLS)
    from audio_amd import _diff
    assert all(callable(getattr(_diff, n)) for n in ("oscillator_bank", "filter_waveform", "sinc_impulse_response", "frequency_impulse_response"))


def test_error_types():
    f = torch.zeros(2, 8, 3)
    with pytest.raises(ValueError, match="one shape"):
        F.oscillator_bank(f, f[:, :, :2], 16000.0)
    with pytest.raises(ValueError, match="time, N"):
        F.oscillator_bank(f[0, 0], f[0, 0], 16000.0)
    with pytest.raises(TypeError, match="one dtype"):
        F.oscillator_bank(f, f.double(), 16000.0)
    with pytest.raises(TypeError, match="float16, bfloat16, float32 or float64"):
        F.oscillator_bank(f.long(), f.long(), 16000.0)
    with pytest.raises(ValueError, match="reduction"):
        F.oscillator_bank(f, f, 16000.0, reduction="max")
    with pytest.raises(ValueError, match="dtype"):
        F.oscillator_bank(f, f, 16000.0, dtype=torch.float16)
    with pytest.raises(ValueError, match="sample_rate"):
        F.oscillator_bank(f, f, 0.0)
    big = torch.zeros(1, 2, F.DSP_MAX_OSCILLATORS + 1)
    with pytest.raises(NotImplementedError, match=str(F.DSP_MAX_OSCILLATORS)):
        F.oscillator_bank(big, big, 16000.0)
    x = torch.zeros(2, 12)
    with pytest.raises(ValueError, match="multiple"):
        F.filter_waveform(x, torch.zeros(5, 3))
    with pytest.raises(ValueError, match="dimension"):
        F.filter_waveform(x, torch.zeros(3))
    with pytest.raises(ValueError, match="per row"):
        F.filter_waveform(x, torch.zeros(3, 4, 3))
    with pytest.raises(TypeError, match="one dtype"):
        F.filter_waveform(x, torch.zeros(4, 3, dtype=torch.float64))
    with pytest.raises(TypeError, match="float16, bfloat16, float32 or float64"):
        F.filter_waveform(x.int(), torch.zeros(4, 3, dtype=torch.int32))
    with pytest.raises(NotImplementedError, match=str(F.DSP_MAX_TAPS)):
        F.filter_waveform(x, torch.zeros(4, F.DSP_MAX_TAPS + 1))
    for w in (0, -3, 512):
        with pytest.raises(ValueError, match="window_size"):
            F.sinc_impulse_response(torch.tensor([0.5]), w)
    with pytest.raises(TypeError, match="float32 or float64"):
        F.sinc_impulse_response(torch.tensor([0.5], dtype=torch.float16))
    with pytest.raises(ValueError, match="n >= 2"):
        F.frequency_impulse_response(torch.zeros(3, 1))
    with pytest.raises(TypeError, match="float32 or float64"):
        F.frequency_impulse_response(torch.zeros(3, 4, dtype=torch.int64))
    with pytest.raises(NotImplementedError, match=str(F.DSP_MAX_MAGNITUDES)):
        F.frequency_impulse_response(torch.zeros(1, F.DSP_MAX_MAGNITUDES + 1))
    for kw in (dict(attack=1.5), dict(sustain=-0.1), dict(attack=0.6, release=0.5), dict(hold=float("nan"))):
        with pytest.raises(ValueError):
            F.adsr_envelope(10, **kw)
    with pytest.raises(ValueError, match="num_frames"):
        F.adsr_envelope(0)
    with pytest.raises(TypeError, match="dtype"):
        F.adsr_envelope(10, dtype=torch.int32)
    with pytest.raises(ValueError, match="time, 1"):
        F.extend_pitch(torch.zeros(4, 2), 3)
    with pytest.raises(ValueError, match="one dimension"):
        F.extend_pitch(torch.zeros(4, 1), torch.zeros(2, 2))
    with pytest.raises(TypeError, match="dtype of base_frequency"):
        F.extend_pitch(torch.zeros(4, 1), torch.zeros(2, dtype=torch.float64))
    with pytest.raises(TypeError, match="pattern"):
        F.extend_pitch(torch.zeros(4, 1), "3")
    with pytest.raises(ValueError, match="negative"):
        F.extend_pitch(torch.zeros(4, 1), -1)


def test_cpu_tensors_are_refused():
    match = "must be on an MI355X .* no CPU fallback"
    f = torch.zeros(2, 8, 3)
    with pytest.raises(RuntimeError, match=match):
        F.oscillator_bank(f, f, 16000.0)
    with pytest.raises(RuntimeError, match=match):
        F.filter_waveform(torch.zeros(2, 12), torch.zeros(4, 3))
    with pytest.raises(RuntimeError, match=match):
        F.sinc_impulse_response(torch.tensor([0.5]))
    with pytest.raises(RuntimeError, match=match):
        F.frequency_impulse_response(torch.zeros(2, 5))
    with pytest.raises(RuntimeError, match=match):
        F.extend_pitch(torch.zeros(4, 1), 3)
    with pytest.raises(RuntimeError, match=match):
        F.adsr_envelope(10, attack=0.5, device="cpu")
    with pytest.raises(RuntimeError, match=match):
        F.oscillator_bank(f.clone().requires_grad_(), f, 16000.0)       # the training path is on the device as well
    for rate in (16000, np.float32(16000.0), np.int64(16000), torch.tensor(16000.0)):      # every kind of number passes the checks
        with pytest.raises(RuntimeError, match=match):
            F.oscillator_bank(f, f, rate)
    for rate in (True, "16000.0x", None, float("inf"), np.float32(-1.0)):
        with pytest.raises(ValueError, match="sample_rate"):
            F.oscillator_bank(f, f, rate)
    with pytest.raises(RuntimeError, match=match):                       # fractions that sum to 1 on paper, 1 + 2^-52 in float64
        F.adsr_envelope(10, attack=0.2, hold=0.4, decay=0.3, release=0.1, device="cpu")
    assert 0.2 + 0.4 + 0.3 + 0.1 > 1.0 and _host.adsr_ramp(11, 0.2, 0.4, 0.3, 0.5, 0.1, 2).shape == (11,)


def test_not_dispatcher_ops():
    import audio_amd._ops  # noqa: F401  (registers the audio_amd:: ops)
    for name in ("oscillator_bank", "filter_waveform", "sinc_impulse_response", "frequency_impulse_response", "extend_pitch"):
        assert not hasattr(torch.ops.audio_amd, name)
