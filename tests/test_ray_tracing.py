"""F.ray_tracing / F.ray_tracing_batch without a GPU: a CPU replay of csrc/ray_trace.h (the kernel's phase functions with the
launch geometry of the C ABI) against tests/ray_oracle.py.

Accuracy: |result - float64 oracle| <= 4 x the float64 oracle's own distance from its longdouble form + count 2^-(k+1) for the
quantisation (+ half a float32 ulp for a float32 result); bins the oracle leaves empty are exactly 0.  Measured share of that
bar, replay: 0.00-0.22 for float64 results and 0.90-1.00 for float32 results (the half ulp of the one float32 rounding) over
the 22 cases; the replay's int64 accumulator EQUALS the oracle's on every case, so what is left is the quantisation itself.
Device: see tests/test_gpu_ray_tracing.py.  Then the margin condition on the inputs, the exact
properties (same bits twice, rows of a batch, microphones alone, equal bands, bad rooms), the bounce bound, the host code,
signatures, error types and the refusal of CPU tensors."""
import ctypes as C
import inspect
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import ray_cases as K
import ray_oracle as O
import audio_amd.functional as F
from audio_amd import _host, _lib

HERE = os.path.dirname(os.path.abspath(__file__))
SIM_SRC = os.path.join(HERE, "cpu_sim", "sim_ray.cpp")
SIM_OUT = os.path.join(HERE, "cpu_sim", "_build", "libaamd_sim_ray.so")
HDRS = [os.path.join(os.path.dirname(HERE), "audio_amd", "csrc", h) for h in ("ray_trace.h", "hd.h")]
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
        _sim.sim_ray.argtypes = [i32] + [p] * 7 + [i64, i64, i32, i32, i64, i64, i32] + [d] * 5 + [p]
        _sim.sim_ray_tiles.argtypes = [i32]
    return _sim


class Replay:
    """The backend of ray_cases: the kernels' phase functions on the CPU."""

    @staticmethod
    def tiles():
        return tuple(sim().sim_ray_tiles(i) for i in range(7))

    @staticmethod
    def run(room, source, mic, num_rays, absorption, scattering, mic_radius=0.5, sound_speed=K.C, energy_thres=1e-7,
            time_thres=10.0, hist_bin_size=0.004, rc=0, with_acc=False, k=None):
        room, source, mic, ab, sc = (np.ascontiguousarray(t) for t in (room, source, mic, absorption, scattering))
        assert room.dtype == source.dtype == mic.dtype == ab.dtype == sc.dtype
        B, M, D = mic.shape
        NB = ab.shape[1]
        assert room.shape == source.shape == (B, D) and ab.shape == sc.shape == (B, NB, 2 * D)
        bins = _host.ray_num_bins(time_thres, hist_bin_size)
        k = _host.ray_scale_log2(mic_radius) if k is None else k
        out = np.full((B, M, NB, bins), 7.0, room.dtype)
        acc = np.zeros((B, M, NB, bins), np.int64)
        stats = np.zeros(2, np.int64)
        got = sim().sim_ray(CODE[room.dtype], room.ctypes.data, source.ctypes.data, mic.ctypes.data, ab.ctypes.data, sc.ctypes.data,
                            acc.ctypes.data, out.ctypes.data, B, M, D, NB, num_rays, bins, k, mic_radius, sound_speed, energy_thres,
                            time_thres, hist_bin_size, stats.ctypes.data)
        assert got == rc
        assert stats[1] == 0                                         # no add fell outside the accumulator
        return (out, acc) if with_acc else out


# ---- 1. the condition on the inputs, and the structure -------------------------------------------------------------------------

def test_tiles_are_what_the_cases_straddle():
    want = (K.THREADS, F.RAY_MAX_BANDS, F.RAY_MAX_MICS, F.RAY_MAX_RAYS, F.RAY_MAX_BINS, F.RAY_MAX_BOUNCES, F.RAY_HEADROOM)
    assert Replay.tiles() == want
    assert want[1:] == (8, 16, 1 << 24, 65536, O.MAX_BOUNCES, O.HEADROOM) and _host.RAY_HEADROOM == F.RAY_HEADROOM
    if os.path.exists(_lib.LIB_PATH):
        assert F.ray_tiles() == Replay.tiles()
    # the defaults in a 6 x 5 x 3 m room
    assert O.bounce_bound([6.0, 5.0, 3.0], 10.0, 343.0) == 2406 and 2407 <= F.RAY_MAX_BOUNCES


@pytest.mark.parametrize("dt", list(K.DTYPES))
@pytest.mark.parametrize("name", list(K.SHAPES))
def test_no_decision_of_a_case_is_within_1e_9_of_flipping(name, dt):
    *_, margin = K.case(name, dt)
    assert margin >= K.MARGIN, (name, dt, margin)


def test_the_cases_end_the_ways_they_say():
    _, o64, *_ = K.case("r255_m16_ab0_time_ends", "f64")
    assert o64[0].bounces > 3 and o64[0].bounces <= o64[0].bound     # absorption 0: only the time bound ends a ray
    _, o64, *_ = K.case("r300_m5_energy_ends", "f64")
    _, long_, *_ = K.case("d2_r65_m1_tt.25", "f64")
    assert o64[0].bounces < 8 < long_[0].bounces                     # the energy bound ends them long before 0.25 s
    for name in K.SHAPES:
        _, o64, *_ = K.case(name, "f64")
        assert all(o.bounces <= o.bound for o in o64) and all(o.top <= 1.0 for o in o64)


def test_num_bins_and_the_scale():
    for tt, hb, want in ((10.0, 0.004, 2500), (0.1, 0.004, 25), (0.1, 0.0037, 28), (0.25, 0.004, 63), (1.0, 1.0, 1), (0.05, 0.1, 1)):
        assert _host.ray_num_bins(tt, hb) == O.num_bins(tt, hb) == want == math.ceil(tt / hb)
    assert _host.ray_scale_log2(0.5) == 51                          # 8 * 64 / 0.25 = 2^11: a step of 2^-51 at the default radius
    for r in (0.5, 0.3, 0.4, 1.0, 2.0, 0.25, 1e-3, 0.7071067811865476, 123.456):
        assert _host.ray_scale_log2(r) == O.scale_log2(r)
        assert 8 * O.HEADROOM / (r * r) <= 2.0 ** (62 - O.scale_log2(r)) < 2 * 8 * O.HEADROOM / (r * r)
    with pytest.raises(ValueError, match="mic_radius"):
        _host.ray_scale_log2(1e-200)


# ---- 2. accuracy on the smallest shapes where the kernel can go wrong ---------------------------------------------------------

@pytest.mark.parametrize("dt", list(K.DTYPES))
@pytest.mark.parametrize("name", list(K.SHAPES))
def test_replay_within_the_oracles_own_error(name, dt):
    K.check_accuracy(Replay, name, dt)


@pytest.mark.parametrize("dt", list(K.DTYPES))
@pytest.mark.parametrize("name", list(K.SHAPES))
def test_replay_accumulator_is_the_oracles(name, dt):
    """Exact: the replay's int64 sums are the oracle's (the margin condition holds on every case), and the result is those sums
    times 2^-k rounded once."""
    (room, source, mic, ab, sc), o64, *_ = K.case(name, dt)
    out, acc = Replay.run(room, source, mic, K.SHAPES[name][1], ab, sc, with_acc=True, **K.params(name))
    assert np.array_equal(acc, np.stack([o.acc for o in o64]))
    assert np.array_equal(out, np.stack([O.final(o.acc, o.k, K.DTYPES[dt]) for o in o64]))


def test_a_wrapped_sum_is_nan():
    """With a scale 2^18 too large the fuller bins pass 2^63 and come back negative: NaN, not a number of the wrong sign."""
    name = "r63_m2_sc.3"
    (room, source, mic, ab, sc), *_ = K.case(name, "f64")
    kw, n = K.params(name), K.SHAPES[name][1]
    good = Replay.run(room, source, mic, n, ab, sc, **kw)
    out, acc = Replay.run(room, source, mic, n, ab, sc, with_acc=True, k=_host.ray_scale_log2(kw["mic_radius"]) + 18, **kw)
    assert (acc < 0).any() and np.array_equal(np.isnan(out), acc < 0) and not np.isnan(good).any()


# ---- 3. exact properties ---------------------------------------------------------------------------------------------------------

def test_two_runs_give_the_same_bits():
    K.check_reproducible(Replay)


@pytest.mark.parametrize("dt", list(K.DTYPES))
def test_rows_of_a_batch_are_rooms_and_microphones_stand_alone(dt):
    K.check_rows_are_rooms(Replay, dt)


@pytest.mark.parametrize("dt", list(K.DTYPES))
def test_equal_bands_are_equal(dt):
    K.check_equal_bands(Replay, dt)


@pytest.mark.parametrize("dt", list(K.DTYPES))
def test_a_bad_room_is_nan_and_its_neighbours_keep_their_bits(dt):
    K.check_bad_rooms(Replay, dt)


def test_replay_refuses_what_the_abi_refuses():
    (room, source, mic, ab, sc), *_ = K.case("r1_m1_radius2", "f32")
    Replay.run(room, source, mic, 0, ab, sc, time_thres=0.1, rc=-1)
    Replay.run(room, source, mic, 1, ab, sc, time_thres=0.1, mic_radius=0.0, k=51, rc=-1)
    Replay.run(room, source, mic, 1, ab, sc, time_thres=0.1, hist_bin_size=-1.0, rc=-1)
    Replay.run(room, source, mic, F.RAY_MAX_RAYS + 1, ab, sc, time_thres=0.1, rc=-2)
    Replay.run(room, source, np.repeat(mic, 17, axis=1), 1, ab, sc, time_thres=0.1, rc=-2)
    Replay.run(room, source, mic, 1, np.repeat(ab, 9, axis=1), np.repeat(sc, 9, axis=1), time_thres=0.1, rc=-2)


# ---- 4. the public surface ---------------------------------------------------------------------------------------------------------

def test_signatures_and_exports():
    names = ["room", "source", "mic_array", "num_rays", "absorption", "scattering", "mic_radius", "sound_speed", "energy_thres",
             "time_thres", "hist_bin_size"]
    for f in (F.ray_tracing, F.ray_tracing_batch):
        p = inspect.signature(f).parameters
        assert list(p) == names
        assert [p[n].default for n in names[4:]] == [0.0, 0.0, 0.5, 343.0, 1e-7, 10.0, 0.004]
        assert all(p[n].default is inspect.Parameter.empty for n in names[:4])
    assert {"ray_tracing", "ray_tracing_batch", "ray_tiles"} <= set(F.__all__)
    import audio_amd.prototype.functional as P
    assert P.ray_tracing is F.ray_tracing and P.ray_tracing_batch is F.ray_tracing_batch
    assert {"ray_tracing", "ray_tracing_batch"} <= set(P.__all__)
    assert {"aamd_ray_tiles", "aamd_ray_trace"} <= set(_lib.EXPORTED_SYMBOLS)


def test_not_a_dispatcher_op():
    import audio_amd._ops  # noqa: F401  (registers the audio_amd:: ops)
    assert not hasattr(torch.ops.audio_amd, "ray_tracing")
    assert not hasattr(torch.ops.audio_amd, "ray_tracing_batch")


def _one(dtype=torch.float32, D=3, M=2):
    return torch.full((D,), 4.0, dtype=dtype), torch.full((D,), 1.0, dtype=dtype), torch.full((M, D), 2.0, dtype=dtype)


def test_error_types():
    room, source, mic = _one()
    f, fb = F.ray_tracing, F.ray_tracing_batch
    with pytest.raises(ValueError, match="dimensions"):
        f(room[None], source, mic, 10)
    with pytest.raises(ValueError, match="dimensions"):
        f(room, source, mic[0], 10)
    with pytest.raises(ValueError, match="dimensions"):
        fb(room, source, mic, 10)
    with pytest.raises(ValueError, match="2 or 3"):
        f(*_one(D=4), 10)
    with pytest.raises(ValueError, match="same number of coordinates"):
        f(room, source[:2], mic, 10)
    with pytest.raises(ValueError, match="same number of rooms"):
        fb(room[None], source[None], mic[None].repeat(2, 1, 1), 10)
    for n in (0, -5):
        with pytest.raises(ValueError, match="num_rays"):
            f(room, source, mic, n)
    with pytest.raises(TypeError, match="num_rays"):
        f(room, source, mic, 10.0)
    for name in ("mic_radius", "sound_speed", "energy_thres", "time_thres", "hist_bin_size"):
        for v in (0.0, -1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError, match=name):
                f(room, source, mic, 10, **{name: v})
    for name in ("absorption", "scattering"):
        with pytest.raises(ValueError, match=name):
            f(room, source, mic, 10, **{name: torch.zeros(2, 5)})
        with pytest.raises(ValueError, match=name):
            f(room, source, mic, 10, **{name: torch.zeros(2, 6, 1)})
        with pytest.raises(ValueError, match=name):
            fb(room[None], source[None], mic[None], 10, **{name: torch.zeros(2, 6)})
        with pytest.raises(ValueError, match=name):
            fb(room[None], source[None], mic[None], 10, **{name: torch.zeros(2, 3, 6)})
        with pytest.raises(TypeError, match=name):
            f(room, source, mic, 10, **{name: "0.1"})
        with pytest.raises(TypeError, match="one dtype"):
            f(room, source, mic, 10, **{name: torch.zeros(2, 6, dtype=torch.float64)})
    with pytest.raises(ValueError, match="same number of bands"):
        f(room, source, mic, 10, torch.zeros(3), torch.zeros(2, 6))
    with pytest.raises(TypeError, match="float32 or float64"):
        f(*_one(torch.float16), 10)
    with pytest.raises(TypeError, match="float32 or float64"):
        f(*(t.long() for t in _one()), 10)
    with pytest.raises(TypeError, match="one dtype"):
        f(room, source.double(), mic, 10)
    with pytest.raises(NotImplementedError, match=f"up to {F.RAY_MAX_BANDS} bands"):
        f(room, source, mic, 10, torch.zeros(F.RAY_MAX_BANDS + 1))
    with pytest.raises(NotImplementedError, match=f"up to {F.RAY_MAX_MICS} microphones"):
        f(*_one(M=F.RAY_MAX_MICS + 1), 10)
    with pytest.raises(NotImplementedError, match=f"up to {F.RAY_MAX_RAYS} rays"):
        f(room, source, mic, F.RAY_MAX_RAYS + 1)
    with pytest.raises(NotImplementedError, match=f"up to {F.RAY_MAX_BINS} bins"):
        f(room, source, mic, 10, time_thres=10.0, hist_bin_size=1e-4)


def test_cpu_tensors_and_gradients_are_refused():
    room, source, mic = _one()
    with pytest.raises(RuntimeError, match="must be on an MI355X .* no CPU fallback"):
        F.ray_tracing(room, source, mic, 10)
    with pytest.raises(RuntimeError, match="must be on an MI355X .* no CPU fallback"):
        F.ray_tracing(room, source, mic, 10, torch.zeros(2, 6), 0.1)
    with pytest.raises(RuntimeError, match="must be on an MI355X .* no CPU fallback"):
        F.ray_tracing_batch(room[None], source[None], mic[None], 10)
    with pytest.raises(RuntimeError, match="forward-only"):
        F.ray_tracing(room, source.clone().requires_grad_(), mic, 10)
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
        F.ray_tracing(room, source.clone().requires_grad_(), mic, 10)
