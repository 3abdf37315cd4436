"""F.simulate_rir_ism / F.simulate_rir_ism_batch without a GPU: a CPU replay of csrc/rir.h (the kernel's phase functions with
the launch geometry of the C ABI) against tests/rir_oracle.py -- a float32 result no further from the float64 oracle than
the oracle's own float32 evaluation, a float64 result within 4 x the float64 oracle's distance from its longdouble form --
the exact structure (image counts, lattice order, the default length), bit-reproducibility, the NaN rows, the host code,
signatures, error types and the refusal of CPU tensors."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest
import torch

import rir_cases as K
import rir_oracle as O
import audio_amd.functional as F
from audio_amd import _host, _lib

HERE = os.path.dirname(os.path.abspath(__file__))
SIM_SRC = os.path.join(HERE, "cpu_sim", "sim_rir.cpp")
SIM_OUT = os.path.join(HERE, "cpu_sim", "_build", "libaamd_sim_rir.so")
HDRS = [os.path.join(os.path.dirname(HERE), "audio_amd", "csrc", h) for h in ("rir.h", "hd.h")]
CODE = {np.dtype(np.float32): 0, np.dtype(np.float64): 1}

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
        _sim.sim_rir.argtypes = [i32, p, p, p, p, p, i64, p, i64, i64, i32, i32, i32, i64, d, d]
        _sim.sim_rir_tiles.argtypes = [i32]
    return _sim


class Replay:
    """The backend of rir_cases: the kernel's phase functions on the CPU, the host's lattice table around them."""

    @staticmethod
    def tiles():
        return tuple(sim().sim_rir_tiles(i) for i in range(4))

    @staticmethod
    def run(room, source, mic, max_order, absorption, L, fl=81, sample_rate=K.FS, sound_speed=K.C, rc=0):
        room, source, mic, ab = (np.ascontiguousarray(t) for t in (room, source, mic, absorption))
        assert room.dtype == source.dtype == mic.dtype == ab.dtype
        B, M, D = mic.shape
        assert room.shape == source.shape == (B, D) and ab.shape == (B, 2 * D)
        table = _host.rir_lattice(max_order, D)
        out = np.full((B, M, L), 7.0, room.dtype)
        got = sim().sim_rir(CODE[room.dtype], room.ctypes.data, source.ctypes.data, mic.ctypes.data, ab.ctypes.data,
                            table.ctypes.data, table.shape[0], out.ctypes.data, B, M, D, max_order, fl, L, sample_rate, sound_speed)
        assert got == rc
        return out


# ---- 1. exact structure -------------------------------------------------------------------------------------------------------

def test_tiles_are_what_the_cases_straddle():
    assert Replay.tiles() == (K.TILE, K.CHUNK, F.RIR_MAX_FILTER, F.RIR_MAX_ORDER)
    assert F.RIR_MAX_FILTER >= 1025 and F.RIR_MAX_ORDER >= 40
    if os.path.exists(_lib.LIB_PATH):
        assert F.rir_tiles() == Replay.tiles()
    assert _host.rir_image_count(5, 3) < K.CHUNK < _host.rir_image_count(6, 3)


def test_image_counts():
    for D, want in ((3, (1, 7, 63, 1561, 7175)), (2, (1, 5, 25, 221, 613))):
        for n, w in zip((0, 1, 3, 10, 17), want):
            assert _host.rir_lattice(n, D).shape == (w, D) and _host.rir_image_count(n, D) == w
    for D in (2, 3):
        for n in (0, 1, 2, 3, 6):
            assert O.image_count(n, D) == _host.rir_image_count(n, D)


def test_lattice_equals_the_oracles_in_order():
    for D in (2, 3):
        for n in (0, 1, 2, 3, 6, 9):
            got = _host.rir_lattice(n, D)
            assert got.dtype == np.int16 and got.flags.c_contiguous
            assert np.array_equal(got.astype(np.int64), O.lattice(n, D))
    assert np.array_equal(O.lattice(1, 2), [[-1, 0], [0, -1], [0, 0], [0, 1], [1, 0]])
    with pytest.raises(ValueError):
        _host.rir_lattice(1, 4)


def test_length_equals_the_oracles_on_50_seeded_rooms():
    for seed in range(50):
        D, N, M = (3, 2)[seed % 2], seed % 5, 1 + seed % 3
        dtype = (np.float32, np.float64)[(seed // 2) % 2]
        room, source, mic, _ = K.rooms(1000 + seed, 1, M, D, dtype, N)
        fl, fs = (81, 3, 255)[seed % 3], (16000.0, 44100.0, 8000.0)[seed % 3]
        assert _host.rir_length(room[0], source[0], mic[0], N, fs, 343.0, fl) == O.length(room[0], source[0], mic[0], N, fs, 343.0, fl)


def test_the_two_forms_of_the_oracle_agree():
    (room, source, mic, ab, N, L, fl), o64, _, _ = K.case("n6_377img_m3_b1_2tile+3", "f64")
    sc = O.scatter(room[0], source[0], mic[0], N, ab[0], L, K.FS, K.C, fl)
    # independent expressions of the same function in float64: a few ulp of the sum of magnitudes
    assert np.abs(sc - o64[0]).max() <= 16 * np.finfo(np.float64).eps * O.abs_terms(room[0], source[0], mic[0], N, ab[0], L, K.FS, K.C, fl).max()
    (room, source, mic, ab, N, L, fl), o64, _, _ = K.case("n3_m1_b1_tile_fl3", "f64")
    sc = O.scatter(room[0], source[0], mic[0], N, ab[0], L, K.FS, K.C, fl)
    assert np.abs(sc - o64[0]).max() <= 16 * np.finfo(np.float64).eps * O.abs_terms(room[0], source[0], mic[0], N, ab[0], L, K.FS, K.C, fl).max()


@pytest.mark.parametrize("dt", list(K.DTYPES))
def test_single_image_is_the_closed_form(dt):
    K.check_single_image(Replay, dt)


# ---- 2. accuracy on the smallest shapes where the kernel can go wrong ---------------------------------------------------------

@pytest.mark.parametrize("dt", list(K.DTYPES))
@pytest.mark.parametrize("name", list(K.SHAPES))
def test_replay_within_the_oracles_own_error(name, dt):
    K.check_accuracy(Replay, name, dt)


# ---- 3. reproducibility, exact --------------------------------------------------------------------------------------------------

def test_two_runs_give_the_same_bits():
    K.check_reproducible(Replay)


@pytest.mark.parametrize("dt", list(K.DTYPES))
def test_prefix_of_a_longer_call_is_the_shorter_call(dt):
    K.check_prefix(Replay, dt)


@pytest.mark.parametrize("dt", list(K.DTYPES))
def test_rows_of_a_batch_are_rooms_of_their_own(dt):
    K.check_rows_are_rooms(Replay, dt)


@pytest.mark.parametrize("dt", list(K.DTYPES))
def test_microphone_on_the_source_poisons_its_row_only(dt):
    K.check_poison(Replay, dt)


def test_replay_refuses_what_the_abi_refuses():
    (room, source, mic, ab, N, L, fl), _, _, _ = K.case("n1_m3_b1_tile", "f32")
    Replay.run(room, source, mic, N, ab, L, 80, rc=-1)
    Replay.run(room, source, mic, N, ab, L, 1, rc=-1)
    Replay.run(room, source, mic, N, ab, L, F.RIR_MAX_FILTER + 2, rc=-2)


# ---- 4. the public surface ---------------------------------------------------------------------------------------------------------

def test_signatures_and_exports():
    p = inspect.signature(F.simulate_rir_ism).parameters
    assert list(p) == ["room", "source", "mic_array", "max_order", "absorption", "sound_speed", "delay_filter_length",
                       "center_frequency", "sample_rate", "output_length"]
    assert (p["sound_speed"].default, p["delay_filter_length"].default, p["center_frequency"].default, p["sample_rate"].default,
            p["output_length"].default) == (343.0, 81, None, 16000.0, None)
    p = inspect.signature(F.simulate_rir_ism_batch).parameters
    assert list(p) == ["room", "source", "mic_array", "max_order", "absorption", "output_length", "sound_speed",
                       "delay_filter_length", "sample_rate"]
    assert p["output_length"].default is inspect.Parameter.empty
    assert (p["sound_speed"].default, p["delay_filter_length"].default, p["sample_rate"].default) == (343.0, 81, 16000.0)
    assert {"simulate_rir_ism", "simulate_rir_ism_batch", "rir_tiles"} <= set(F.__all__)
    import audio_amd.prototype.functional as P
    assert P.simulate_rir_ism is F.simulate_rir_ism and P.simulate_rir_ism_batch is F.simulate_rir_ism_batch
    assert {"aamd_rir_tiles", "aamd_simulate_rir"} <= set(_lib.EXPORTED_SYMBOLS)


def test_not_a_dispatcher_op():
    import audio_amd._ops  # noqa: F401  (registers the audio_amd:: ops)
    assert not hasattr(torch.ops.audio_amd, "simulate_rir_ism")
    assert not hasattr(torch.ops.audio_amd, "simulate_rir_ism_batch")


def _one(dtype=torch.float32, D=3, M=2):
    return torch.full((D,), 4.0, dtype=dtype), torch.full((D,), 1.0, dtype=dtype), torch.full((M, D), 2.0, dtype=dtype)


def test_error_types():
    room, source, mic = _one()
    f, fb = F.simulate_rir_ism, F.simulate_rir_ism_batch
    with pytest.raises(ValueError, match="dimensions"):
        f(room[None], source, mic, 1, 0.1)
    with pytest.raises(ValueError, match="dimensions"):
        f(room, source, mic[0], 1, 0.1)
    with pytest.raises(ValueError, match="dimensions"):
        fb(room, source, mic, 1, 0.1, 100)
    with pytest.raises(ValueError, match="2 or 3"):
        f(*_one(D=4), 1, 0.1)
    with pytest.raises(ValueError, match="same number of coordinates"):
        f(room, source[:2], mic, 1, 0.1)
    with pytest.raises(ValueError, match="same number of rooms"):
        fb(room[None], source[None], mic[None].repeat(2, 1, 1), 1, 0.1, 100)
    for fl in (80, 1, -3):
        with pytest.raises(ValueError, match="delay_filter_length"):
            f(room, source, mic, 1, 0.1, delay_filter_length=fl)
    with pytest.raises(ValueError, match="max_order"):
        f(room, source, mic, -1, 0.1)
    with pytest.raises(ValueError, match="output_length"):
        f(room, source, mic, 1, 0.1, output_length=0)
    with pytest.raises(ValueError, match="output_length"):
        fb(room[None], source[None], mic[None], 1, 0.1, 0)
    with pytest.raises(TypeError, match="float32 or float64"):
        f(*_one(torch.float16), 1, 0.1)
    with pytest.raises(TypeError, match="float32 or float64"):
        f(*(t.long() for t in _one()), 1, 0.1)
    with pytest.raises(TypeError, match="one dtype"):
        f(room, source.double(), mic, 1, 0.1)
    with pytest.raises(NotImplementedError, match=str(F.RIR_MAX_FILTER)):
        f(room, source, mic, 1, 0.1, delay_filter_length=F.RIR_MAX_FILTER + 2)
    with pytest.raises(NotImplementedError, match=str(F.RIR_MAX_ORDER)):
        f(room, source, mic, F.RIR_MAX_ORDER + 1, 0.1)
    with pytest.raises(NotImplementedError, match="octave-band filter bank"):
        f(room, source, mic, 1, torch.full((7, 6), 0.1))


def test_cpu_tensors_and_gradients_are_refused():
    room, source, mic = _one()
    with pytest.raises(RuntimeError, match="must be on an MI355X .* no CPU fallback"):
        F.simulate_rir_ism(room, source, mic, 1, 0.1)
    with pytest.raises(RuntimeError, match="must be on an MI355X .* no CPU fallback"):
        F.simulate_rir_ism(room, source, mic, 1, 0.1, output_length=64)
    with pytest.raises(RuntimeError, match="must be on an MI355X .* no CPU fallback"):
        F.simulate_rir_ism_batch(room[None], source[None], mic[None], 1, 0.1, 64)
    with pytest.raises(RuntimeError, match="forward-only"):
        F.simulate_rir_ism(room, source.clone().requires_grad_(), mic, 1, 0.1, output_length=64)
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
        F.simulate_rir_ism(room, source.clone().requires_grad_(), mic, 1, 0.1, output_length=64)
