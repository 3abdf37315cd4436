"""F.overdrive / F.phaser / F.flanger without a GPU: the oracle's two forms against each other, a CPU replay of
csrc/effects.h (delay-line kernel on both sides of the LDS limit, streaming flanger, overdrive's two launches; four dtypes,
dense and misaligned rows) against the oracle -- bit for bit for phaser and flanger, at the issue's tolerance for overdrive --
the host's table builder, signatures, error types and the refusal of CPU tensors."""
import ctypes as C
import inspect
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import effects_cases as K
import effects_oracle as O
import audio_amd.functional as F
from audio_amd import _host

HERE = os.path.dirname(os.path.abspath(__file__))
SIM_SRC = os.path.join(HERE, "cpu_sim", "sim_effects.cpp")
SIM_OUT = os.path.join(HERE, "cpu_sim", "_build", "libaamd_sim_effects.so")
HDRS = [os.path.join(os.path.dirname(HERE), "audio_amd", "csrc", h) for h in ("effects.h", "wave_augment.h", "spec_augment.h",
                                                                              "hd.h")]
CODE = {torch.float32: 0, torch.float64: 1, torch.float16: 2, torch.bfloat16: 3}
DTYPES = [torch.float32, torch.float64, torch.float16, torch.bfloat16]

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
        _sim.sim_fx_ring_in_lds.argtypes = [i32, i64]
        _sim.sim_fx_delay.argtypes = [i32, i32, i32, p, p, i64, i64, i64, p, i64, i64, i32, p, d, d, d, i32]
        _sim.sim_fx_overdrive.argtypes = [i32, p, p, p, i64, i64, i64, d, d]
    return _sim


def tiles():
    return sim().sim_fx_tiles(0), sim().sim_fx_tiles(1), sim().sim_fx_tiles(2)


def misaligned(x):
    """The rows of x cut from a wider buffer: a storage offset of one element and a row stride of T + 1."""
    rows, T = x.shape
    big = torch.zeros(rows * (T + 1) + 1, dtype=x.dtype)
    view = big[1:].view(rows, T + 1)[:, :T]
    view.copy_(x)
    return view


def _rs(t):
    return t.stride(0) if t.shape[0] > 1 else 0


def sim_phaser(x, sample_rate, gain_in=0.4, gain_out=0.74, delay_ms=3.0, decay=0.4, mod_speed=0.5, sinusoidal=True):
    L, M, m = O.phaser_plan(sample_rate, delay_ms, mod_speed, sinusoidal)
    m = np.ascontiguousarray(m, dtype=np.int32)
    out = torch.empty(x.shape, dtype=x.dtype)
    assert sim().sim_fx_delay(CODE[x.dtype], 0, 1, x.data_ptr(), out.data_ptr(), x.shape[0], x.shape[1], _rs(x),
                              m.ctypes.data, M, L, 1, None, gain_in, decay, gain_out, 0) == 0
    return out


def sim_flanger(x3, sample_rate, general=False, **kw):
    """x3: (B, C, T) whose (B * C, T) view has one row stride."""
    B, Cn, T = x3.shape
    interpolation = kw.pop("interpolation", "linear")
    L, N, lfo, cph, fg, ig, dg = O.flanger_plan(sample_rate, Cn, **kw)
    lfo = np.ascontiguousarray(lfo, dtype=np.float32)
    cph = np.ascontiguousarray(cph % N, dtype=np.int64)
    x2 = x3.view(B * Cn, T)
    out = torch.empty((B * Cn, T), dtype=x3.dtype)
    assert sim().sim_fx_delay(CODE[x3.dtype], 1, int(general), x2.data_ptr(), out.data_ptr(), B * Cn, T, _rs(x2),
                              lfo.ctypes.data, N, L, Cn, cph.ctypes.data, fg, ig, dg, int(interpolation == "quadratic")) == 0
    return out.view(B, Cn, T)


def sim_overdrive(x, gain=20.0, colour=20.0):
    rows, T = x.shape
    out = torch.empty((rows, T), dtype=x.dtype)
    ws = torch.zeros(max(rows * ((T + tiles()[2] - 1) // tiles()[2]), 1), dtype=torch.float64)
    assert sim().sim_fx_overdrive(CODE[x.dtype], x.data_ptr(), out.data_ptr(), ws.data_ptr(), rows, T, _rs(x),
                                  math.exp(gain * math.log(10) / 20.0), colour / 200) == 0
    return out


def same_bits(got, want):
    return torch.equal(K.bits(got), K.bits(want))


# ---- the oracle's forms -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_oracle_forms_agree_bit_for_bit(dt):
    x = K.compute_view(K.base_input(1, 0.8, 3, 1200, torch.float32))
    for name in ("L5", "L1", "triangle", "clamp"):
        p = K._phaser_args(name)
        a, b = O.phaser(x, dt=dt, form="ring", **p), O.phaser(x, dt=dt, form="lag", **p)
        assert a.dtype == dt and np.array_equal(a.view(np.int32 if dt == np.float32 else np.int64),
                                                b.view(np.int32 if dt == np.float32 else np.int64)), name
    x3 = x.reshape(1, 3, -1)
    for name in ("default", "stream_quadratic"):
        p = K._flanger_args(name)
        p.pop("regen", None)
        a, b = O.flanger(x3, dt=dt, **p), O.flanger_gather(x3, dt=dt, **p)
        assert np.array_equal(a.view(np.int32 if dt == np.float32 else np.int64),
                              b.view(np.int32 if dt == np.float32 else np.int64)), name
    # the quadratic tap of that set does alias onto the sample just written
    L, N, lfo = O.flanger_plan(**{k: v for k, v in K._flanger_args("stream_quadratic").items() if k != "interpolation"}, C=1)[:3]
    assert int(np.floor(lfo.max())) + 2 == L


# ---- the host's tables ----------------------------------------------------------------------------------------------------------

def test_host_tables_equal_the_oracle():
    for name in K.PHASER_SETS:
        p = K._phaser_args(name)
        L, M, m = O.phaser_plan(p["sr"], p.get("delay_ms", 3.0), p.get("mod_speed", 0.5), p.get("sinusoidal", True))
        got = _host.effects_wave_table("SINE" if p.get("sinusoidal", True) else "TRIANGLE", "INT", M, 1.0, float(L), math.pi / 2)
        assert got.dtype == np.int32 and got.shape == (M,) and np.array_equal(got, m)
        assert got.min() >= 1 and got.max() <= L and (L == 1 or (got.min() == 1 and got.max() == L))
    for name in K.FLANGER_SETS:
        p = K._flanger_args(name)
        p.pop("interpolation", None)
        L, N, lfo, cph = O.flanger_plan(C=4, **p)[:4]
        wave = "SINE" if p.get("modulation", "sinusoidal") == "sinusoidal" else "TRIANGLE"
        got = _host.effects_wave_table(wave, "FLOAT", N, float(math.floor(p.get("delay", 0.0) / 1000 * p["sr"] + 0.5)), L - 2.0,
                                       3 * math.pi / 2)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), lfo.view(np.int32))
        assert got.min() >= 0 and got.max() <= L - 2
        assert np.array_equal(_host.flanger_channel_phase(4, N, p.get("phase", 25.0) / 100), cph)
    for wave in ("SINE", "TRIANGLE"):
        for kind in ("INT", "FLOAT"):
            for n, mn, mx, ph in ((1, 1.0, 7.0, 0.0), (7, 0.0, 3.0, 1.0), (1000, 2.0, 40.0, 3 * math.pi / 2), (333, -4.0, 4.0, 0.3)):
                a, b = _host.effects_wave_table(wave, kind, n, mn, mx, ph), O.table(wave, kind, n, mn, mx, ph)
                assert a.dtype == b.dtype and np.array_equal(a, b), (wave, kind, n)
    with pytest.raises(ValueError):
        _host.effects_wave_table("SQUARE", "INT", 4, 0.0, 1.0, 0.0)
    with pytest.raises(ValueError):
        _host.effects_wave_table("SINE", "INT", 0, 0.0, 1.0, 0.0)


# ---- CPU replay of csrc/effects.h -----------------------------------------------------------------------------------------------

def test_sim_tiles_are_the_exported_constants():
    assert tiles() == F.effects_tiles()
    # the parameter sets sit where the cases say: float32 ring of L300 in LDS, its float64 ring and the flanger's 708 not
    assert sim().sim_fx_ring_in_lds(0, 300) == 1 and sim().sim_fx_ring_in_lds(1, 300) == 0
    assert sim().sim_fx_ring_in_lds(0, 708) == 0 and sim().sim_fx_ring_in_lds(0, 512) == 1


@pytest.mark.parametrize("name", list(K.PHASER_SETS))
def test_sim_phaser_equals_the_oracle_bit_for_bit(name):
    R, S, _ = tiles()
    L, M = K.phaser_dims(name)
    Ts = K.lengths(L, S, M)
    for dtype in DTYPES:
        x, want, share = K.phaser_ref(name, R + 1, max(Ts), dtype)
        assert (0.1 <= share <= 0.9) if name == "clamp" else share == 0.0
        for rows, T, layout in [(R + 1, max(Ts), misaligned)] + [(3, T, misaligned if i % 2 else (lambda t: t.contiguous()))
                                                                 for i, T in enumerate(Ts)]:
            got = sim_phaser(layout(x[:rows, :T]), **K.PHASER_SETS[name])
            assert same_bits(got, want[:rows, :T]), (name, dtype, rows, T)


@pytest.mark.parametrize("name", list(K.FLANGER_SETS))
def test_sim_flanger_equals_the_oracle_bit_for_bit(name):
    R, S, _ = tiles()
    L, N = K.flanger_dims(name)
    Ts = K.lengths(L, S, N)
    p = dict(K.FLANGER_SETS[name])
    for dtype in DTYPES:
        for Cn, B in ((2, (R + 2) // 2), (1, 3), (4, 2)) if dtype in DTYPES[:2] else ((2, 2),):
            x, want, share = K.flanger_ref(name, B, Cn, max(Ts), dtype)
            assert share == 0.0
            for T in ([max(Ts)] if Cn != 2 else Ts):
                b = B if T == max(Ts) else 2
                xs = x[:b, :, :T]
                xs = misaligned(xs.reshape(b * Cn, T)).view(b, Cn, T) if T % 2 else xs.contiguous()
                got = sim_flanger(xs, **p)
                assert same_bits(got, want[:b, :, :T]), (name, dtype, Cn, T)
                if p.get("regen", 0.0) == 0.0:              # the streaming route against the general kernel on the same input
                    assert same_bits(sim_flanger(xs, general=True, **p), got), (name, dtype, Cn, T)


@pytest.mark.parametrize("name", list(K.OVERDRIVE_SETS))
def test_sim_overdrive_meets_the_tolerance(name):
    R, _, Kc = tiles()
    p = K.OVERDRIVE_SETS[name]
    Tmax = 2 * Kc + 3
    for dtype in DTYPES:
        x, want, ref32, y = K.overdrive_ref(name, 3, Tmax, dtype)
        for i, T in enumerate((1, 2, Kc - 1, Kc, Kc + 1, Tmax)):
            xs = misaligned(x[:, :T]) if i % 2 else x[:, :T].contiguous()
            got = sim_overdrive(xs, p["gain"], p["colour"]).double().numpy()
            bound = K.overdrive_bound(want[:, :T], ref32[:, :T], y[:, :T], dtype)
            err = np.abs(got - want[:, :T])
            assert (err <= bound).all(), (name, dtype, T, float(err.max()), float(np.max(bound)))
    share = O.overdrive_saturated_share(K.compute_view(K.base_input(13, p["amp"], 3, Tmax, torch.float32)), p["gain"], p["colour"])
    assert {"quiet": 0.05 < share < 0.4, "loud": 0.6 < share < 0.98, "unit": share == 0.0}[name]     # both branches are live


def test_sim_non_finite_sample_stays_in_its_row():
    for name, run, ref in (("phaser", lambda t: sim_phaser(t, **K.PHASER_SETS["L5"]), lambda a: O.phaser(a, dt=np.float32, **K._phaser_args("L5"))),
                           ("overdrive", sim_overdrive, lambda a: O.overdrive(a, dt=np.float32))):
        x = K.base_input(5, 0.5, 3, 300, torch.float32).clone()
        clean = run(x)
        x[1, 150] = float("nan")
        got = run(x)
        assert same_bits(got[[0, 2]], clean[[0, 2]]) and same_bits(got[1, :150], clean[1, :150])
        assert np.array_equal(np.isnan(got.numpy()), np.isnan(ref(x.numpy()))), name
        assert torch.isnan(got[1, 150:]).any()


# ---- the Python surface ---------------------------------------------------------------------------------------------------------

def test_signatures_and_defaults_are_the_reference_s():
    def positional(fn):
        return [(n, p.default) for n, p in inspect.signature(fn).parameters.items() if p.kind == p.POSITIONAL_OR_KEYWORD]
    e = inspect.Parameter.empty
    assert positional(F.overdrive) == [("waveform", e), ("gain", 20), ("colour", 20)]
    assert positional(F.phaser) == [("waveform", e), ("sample_rate", e), ("gain_in", 0.4), ("gain_out", 0.74), ("delay_ms", 3.0),
                                    ("decay", 0.4), ("mod_speed", 0.5), ("sinusoidal", True)]
    assert positional(F.flanger) == [("waveform", e), ("sample_rate", e), ("delay", 0.0), ("depth", 2.0), ("regen", 0.0),
                                     ("width", 71.0), ("speed", 0.5), ("phase", 25.0), ("modulation", "sinusoidal"),
                                     ("interpolation", "linear")]
    assert {"overdrive", "phaser", "flanger", "effects_tiles"} <= set(F.__all__)
    R, S, Kc = F.effects_tiles()
    assert R >= 1 and S >= 1 and Kc >= 2


def test_no_operator_is_registered_for_the_effects():
    from audio_amd import _ops  # noqa: F401
    for ns in ("audio_amd", "aamd"):
        for name in ("overdrive", "phaser", "flanger"):
            assert not hasattr(getattr(torch.ops, ns), name)


def test_errors():
    x = torch.zeros(2, 2, 16)
    with pytest.raises(RuntimeError, match="MI355X"):
        F.overdrive(x)
    with pytest.raises(RuntimeError, match="MI355X"):
        F.phaser(x, 8000)
    with pytest.raises(RuntimeError, match="MI355X"):
        F.flanger(x, 8000)
    for fn in (F.overdrive, lambda t: F.phaser(t, 8000), lambda t: F.flanger(t, 8000)):
        with pytest.raises(TypeError):
            fn(torch.zeros(2, 2, 16, dtype=torch.int32))
        with pytest.raises(TypeError):
            fn(torch.zeros(2, 2, 16, dtype=torch.complex64))
        with pytest.raises(RuntimeError, match="forward-only"):
            fn(torch.zeros(2, 2, 16, requires_grad=True))
    # the reference divides by zero here
    with pytest.raises(ValueError):
        F.phaser(x, 100, delay_ms=3.0)                      # L = 0
    with pytest.raises(ValueError):
        F.phaser(x, 1000, mod_speed=1e6)                    # M = 0
    with pytest.raises(ValueError):
        F.flanger(x, 1000, speed=1e6)                       # N = 0
    with pytest.raises(ValueError):
        F.flanger(torch.zeros(16), 1000)
    with pytest.raises(ValueError, match="Max 4 channels allowed"):
        F.flanger(torch.zeros(1, 5, 16), 1000)
    with pytest.raises(ValueError, match="modulation"):
        F.flanger(x, 1000, modulation="square")
    with pytest.raises(ValueError, match="interpolation"):
        F.flanger(x, 1000, interpolation="cubic")
    # the limits, named
    with pytest.raises(NotImplementedError, match="512"):
        F.phaser(x, 96000, delay_ms=5.4)                    # L = 518
    with pytest.raises(NotImplementedError, match="2\\^24"):
        F.phaser(x, 96000, mod_speed=0.005)                 # M = 19.2 M
    with pytest.raises(NotImplementedError, match="4096"):
        F.flanger(x, 96000, delay=30.0, depth=13.0)         # L = 4130
    with pytest.raises(NotImplementedError, match="2\\^24"):
        F.flanger(x, 96000, speed=0.005)
