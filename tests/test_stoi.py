"""F.stoi without a GPU: the definition of tests/stoi_oracle.py against its own identities (band table, stoi(x, x) = 1, order in
the noise level), a CPU replay of csrc/stoi.h phase by phase against the definition (energies, kept list, a block of band
magnitudes, the segment sums of both modes, the score), the frame bookkeeping at the smallest inputs with a score, ragged /
non-finite / impossible rows, and the checks, exception types, names and signature of the Python entry point."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest
import torch

import stoi_oracle as O
import audio_amd.functional as F
from audio_amd import _lib, _ops

HERE = os.path.dirname(os.path.abspath(__file__))
SIM_SRC = os.path.join(HERE, "cpu_sim", "sim_stoi.cpp")
SIM_OUT = os.path.join(HERE, "cpu_sim", "_build", "libaamd_sim_stoi.so")
HDRS = [os.path.join(os.path.dirname(HERE), "audio_amd", "csrc", h) for h in ("stoi.h", "wave_augment.h", "spec_augment.h", "hd.h")]
TILES = (256, 8, 8, 16, 64)
DT = {np.dtype(np.float32): 0, np.dtype(np.float64): 1}
EPS32, EPS64 = 2.0 ** -23, 2.0 ** -52
MODES = [False, True]
CASE_NAMES = [c[0] for c in O.CASES]

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
    return _sim


def _p(a):
    return C.c_void_p(a.ctypes.data) if a is not None and a.size else None


def run_sim(preds, target, extended=False, lengths=None, dtype_code=None):
    """preds, target: (rows, T) numpy float32 / float64 (or uint16 bit patterns with dtype_code 2 / 3); -> dict of the score and
    every workspace.  The workspaces start as a poison, so what a kernel leaves unwritten shows."""
    preds, target = np.ascontiguousarray(np.atleast_2d(preds)), np.ascontiguousarray(np.atleast_2d(target))
    rows, T = preds.shape
    code = DT[preds.dtype] if dtype_code is None else dtype_code
    cdt = np.float64 if code == 1 else np.float32
    dims = (C.c_int64 * 4)()
    sim().sim_stoi_dims(C.c_int64(T), dims)
    K_max, M_max, nb_e, nt_seg = (int(v) for v in dims)
    r = dict(e=np.full((rows, K_max), -7e77), bad=np.full((rows, nb_e), 99, np.int32), kept=np.full((rows, K_max), -5, np.int32),
             n_kept=np.full((rows,), -9, np.int32), tob=np.full((rows, 2, M_max, O.N_BANDS), -3.0, cdt),
             part=np.full((rows, nt_seg), -7e77), out=np.full((rows,), -2.0, cdt))
    ln = None if lengths is None else np.ascontiguousarray(lengths)
    rc = sim().sim_stoi(C.c_int(code), _p(preds), _p(target), C.c_int64(rows), C.c_int64(T), C.c_int64(T), C.c_int64(T), _p(ln),
                        C.c_int(0 if ln is None else int(ln.dtype == np.int64)), C.c_int(int(extended)), _p(r["e"]), _p(r["bad"]),
                        _p(r["kept"]), _p(r["n_kept"]), _p(r["tob"]), _p(r["part"]), _p(r["out"]))
    assert rc == 0
    return r


# ---- the definition ------------------------------------------------------------------------------------------------------------
def test_band_table_is_the_literals():
    lo, hi = O.band_table()
    assert lo == (7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174) == O.BAND_LO
    assert hi == (9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219) == O.BAND_HI


def test_window_is_the_inner_part_of_hanning_258():
    assert np.allclose(O.window(), np.hanning(258)[1:-1], rtol=0, atol=1e-15)


@pytest.mark.parametrize("extended", MODES)
def test_a_signal_against_itself_scores_one(extended):
    for seed in range(4):
        x = O.gated_harmonic(30000, seed)
        assert abs(O.stoi(x, x, extended) - 1.0) < 1e-12


@pytest.mark.parametrize("extended", MODES)
def test_score_falls_with_the_noise_level(extended):
    for seed in range(4):
        x = O.gated_harmonic(30000, seed)
        s20, s5, sm5 = (O.stoi(O.add_noise_db(x, db, seed), x, extended) for db in (20.0, 5.0, -5.0))
        assert 1.0 > s20 > s5 > sm5 > 0.0, (seed, s20, s5, sm5)


def test_cases_have_the_properties_they_were_chosen_for():
    """Kept sets that are unambiguous (no energy within 1e-6 dB of the threshold), not contiguous at L = 30000, complete at
    seed 3 / L = 6000 and too short for a score at seed 0 / L = 6000."""
    for name, L, seed, _ in O.CASES:
        x, _, scores, kept, margin = O.case(name)
        assert margin > 1e-6, (name, margin)
        if L == 30000:
            assert 60 <= len(kept) <= 80 and kept[-1] - kept[0] + 1 > len(kept)
    assert len(O.case("L6000_s3_20dB")[3]) == 45
    assert len(O.case("L12000_s1_5dB")[3]) == 56
    assert len(O.case("L6000_s0_5dB")[3]) == 19 and O.case("L6000_s0_5dB")[2][False] == (O.SHORT, O.SHORT)
    assert 0.0 < O.bar(False) < 1e-4 and 0.0 < O.bar(True) < 1e-4


# ---- the replay, phase by phase ----------------------------------------------------------------------------------------------------
def test_sim_constants():
    assert tuple(int(sim().sim_stoi_tiles(i)) for i in range(5)) == TILES


@pytest.mark.parametrize("name", CASE_NAMES)
def test_replay_energies_and_kept_list(name):
    x, y, _, kept, _ = O.case(name)
    r = run_sim(y, x)
    e = O.energies(x)
    assert r["e"].shape == (1, len(e))
    # the sum of 256 squares in another order: relative 256 eps of the energy at the most, 20 log10(sqrt(.)) of it in dB
    assert np.max(np.abs(r["e"][0] - e)) < 10.0 / np.log(10.0) * 256 * EPS64 + 1e-12
    assert r["n_kept"][0] == len(kept) and r["kept"][0, :len(kept)].tolist() == kept.tolist()
    assert (r["kept"][0, len(kept):] == -5).all() and (r["bad"] == 0).all()


def _tob_tolerance(x, y, kept, eps):
    """Per frame: 36 eps ||Z||_2 of the frame's transform of x_s + i y_s -- a 9-stage radix-2 transform's error is at most
    c eps log2(512) ||Z||_2 in the 2-norm (c = 4 covers the rounded twiddles and the two windows), and no band can be off by
    more than the whole error."""
    xs, ys = O.rebuild(x, kept), O.rebuild(y, kept)
    M = len(kept) - 1
    idx = O.HOP * np.arange(M)[:, None] + np.arange(O.N_FRAME)[None, :]
    w = O.window()[None, :]
    z2 = np.sum((xs[idx] * w) ** 2 + (ys[idx] * w) ** 2, axis=1)
    return 36.0 * eps * np.sqrt(O.N_FFT * z2)


@pytest.mark.parametrize("name", ["L30000_s0_20dB", "L12000_s1_m5dB", "L6000_s3_20dB"])
@pytest.mark.parametrize("dtype,eps", [(np.float32, EPS32), (np.float64, EPS64)], ids=["f32", "f64"])
def test_replay_band_magnitudes(name, dtype, eps):
    """Every block of the case (the issue asks for one): both signals, every frame, against the float64 definition."""
    x, y, _, kept, _ = O.case(name)
    r = run_sim(y.astype(dtype), x.astype(dtype))
    M = len(kept) - 1
    Tx, Ty = O.band_magnitudes(O.rebuild(x, kept)), O.band_magnitudes(O.rebuild(y, kept))
    tol = _tob_tolerance(x, y, kept, eps)[:, None]
    assert r["tob"].shape[2] >= M
    assert np.all(np.abs(r["tob"][0, 0, :M] - Tx) <= tol) and np.all(np.abs(r["tob"][0, 1, :M] - Ty) <= tol)
    assert (r["tob"][0, :, M:] == -3.0).all()


@pytest.mark.parametrize("extended", MODES)
@pytest.mark.parametrize("name", ["L30000_s3_5dB", "L12000_s1_5dB", "L6000_s3_m5dB"])
def test_replay_segment_sums(name, extended):
    """The segment phase alone: the definition's statistic of the replay's own band matrices."""
    x, y, _, kept, _ = O.case(name)
    r = run_sim(y, x, extended)
    M = len(kept) - 1
    total, J = O.segment_sum(r["tob"][0, 0, :M], r["tob"][0, 1, :M], extended)
    tiles = -(-J // TILES[3])
    assert r["part"].shape[1] >= tiles and abs(float(np.sum(r["part"][0, :tiles])) - total) < 1e-11 * max(1.0, abs(total))
    assert abs(float(r["out"][0]) - total / ((O.SEG if extended else O.N_BANDS) * J)) < 2.0 ** -23


@pytest.mark.parametrize("extended", MODES)
def test_replay_scores_meet_the_bar(extended):
    bar = O.bar(extended)
    for name in CASE_NAMES:
        x, y, scores, _, _ = O.case(name)
        d64 = scores[extended][0]
        for dtype in (np.float32, np.float64):
            got = float(run_sim(y.astype(dtype), x.astype(dtype), extended)["out"][0])
            assert abs(got - d64) <= bar, (name, dtype, got, d64, bar)


@pytest.mark.parametrize("L,K_all,M,J", [(4095, 30, 29, 0), (4096, 31, 30, 1), (4097, 31, 30, 1), (4223, 31, 30, 1), (4224, 32, 31, 2),
                                         (4352, 33, 32, 3)])
def test_frame_bookkeeping_on_stationary_noise(L, K_all, M, J):
    x = O.stationary_noise(L, 0)
    y = O.add_noise_db(x, 5.0, 0)
    assert O.n_frames(L) == K_all and len(O.kept_frames(x)[0]) == K_all
    for extended in MODES:
        r = run_sim(y, x, extended)
        assert r["n_kept"][0] == K_all and r["kept"][0].tolist() == list(range(K_all))
        want = O.stoi(y, x, extended)
        if J == 0:
            assert want == O.SHORT and float(r["out"][0]) == np.float32(1e-5)
        else:
            assert abs(float(r["out"][0]) - want) <= O.bar(extended)
            assert O.segment_sum(r["tob"][0, 0, :M], r["tob"][0, 1, :M], extended)[1] == J


def test_replay_rows_are_independent_ragged_and_guarded():
    """A batch that mixes the cases: every row equals the row alone; a row with a length equals its slice; a NaN below the length
    or a length outside [0, T] scores NaN and leaves the neighbours' bits; a NaN at or beyond the length is never read."""
    T = 12000
    names = ["L12000_s1_5dB", "L6000_s3_20dB", "L6000_s0_5dB", "L12000_s1_m5dB"]
    xs = np.zeros((6, T), np.float32)
    ys = np.zeros((6, T), np.float32)
    lens = np.array([12000, 6000, 6000, 9001, 12001, -1], np.int64)
    for b, n in enumerate(names):
        x, y = O.case(n)[:2]
        xs[b, :len(x)], ys[b, :len(y)] = x, y
    xs[1, 6000:] = np.nan                                             # beyond the length
    xs[4], ys[4], xs[5], ys[5] = xs[0], ys[0], xs[0], ys[0]
    for extended in MODES:
        got = run_sim(ys, xs, extended, lens)["out"]
        for b in range(4):
            alone = run_sim(ys[b, :lens[b]], xs[b, :lens[b]], extended)["out"][0]
            assert got[b].tobytes() == alone.tobytes(), (b, got[b], alone)
        assert np.isnan(got[4]) and np.isnan(got[5])
        assert got[2] == np.float32(1e-5)
        ys2 = ys.copy()
        ys2[3, 9000] = np.inf                                        # the last sample below the length, covered by no frame
        got2 = run_sim(ys2, xs, extended, lens.astype(np.int32))["out"]
        assert np.isnan(got2[3]) and got2[:3].tobytes() == got[:3].tobytes()


def test_replay_half_rows_are_the_widened_rows():
    x, y = O.case("L6000_s3_20dB")[:2]
    for code, tdt in ((2, torch.float16), (3, torch.bfloat16)):
        xh, yh = torch.from_numpy(x.copy()).to(tdt), torch.from_numpy(y.copy()).to(tdt)
        bits = lambda t: t.view(torch.int16).numpy().view(np.uint16)[None, :]      # noqa: E731
        got = run_sim(bits(yh), bits(xh), dtype_code=code)["out"]
        wide = run_sim(yh.float().numpy(), xh.float().numpy())["out"]
        assert got.dtype == np.float32 and got.tobytes() == wide.tobytes()


# ---- the Python entry point ----------------------------------------------------------------------------------------------------------
def test_names_and_signatures():
    for name in ("stoi", "stoi_tiles"):
        assert name in F.__all__ and callable(getattr(F, name))
    sig = inspect.signature(F.stoi)
    assert list(sig.parameters) == ["preds", "target", "sample_rate", "extended", "lengths"]
    assert [p.default for p in sig.parameters.values()] == [inspect.Parameter.empty] * 3 + [False, None]
    assert list(inspect.signature(F.stoi_tiles).parameters) == []
    for sym in ("aamd_stoi", "aamd_stoi_workspace", "aamd_stoi_tiles"):
        assert sym in _lib.EXPORTED_SYMBOLS
    assert not any("stoi" in name for name in _ops.OPS)
    import audio_amd.transforms as T
    assert not any("stoi" in name.lower() for name in dir(T))


def _z(*shape, dtype=torch.float32):
    return torch.zeros(shape, dtype=dtype)


@pytest.mark.parametrize("args,kwargs,exc,match", [
    ((_z(2, 300), _z(2, 301), 10000), {}, ValueError, "must have the same shape"),
    ((_z(), _z(), 10000), {}, ValueError, r"expects \(\.\.\., time\)"),
    ((_z(2, 300), _z(2, 300), 0), {}, ValueError, "sample_rate must be a positive integer"),
    ((_z(2, 300), _z(2, 300), -16000), {}, ValueError, "sample_rate must be a positive integer"),
    ((_z(2, 300), _z(2, 300), 10000), {"lengths": _z(3, dtype=torch.int32)}, ValueError, r"lengths must have the shape \(2,\)"),
    ((_z(2, 300, dtype=torch.int32), _z(2, 300, dtype=torch.int32), 10000), {}, TypeError, "float16, bfloat16, float32 or float64"),
    ((_z(2, 300), _z(2, 300, dtype=torch.float64), 10000), {}, TypeError, "must share a dtype"),
    ((_z(2, 300), _z(2, 300), 10000), {"lengths": _z(2)}, TypeError, "lengths must be int32 or int64"),
    ((_z(2, 300), _z(2, 300), 10000), {}, RuntimeError, r"preds must be on an MI355X \(ROCm\) device.*no CPU fallback"),
    ((_z(2, 300), _z(2, 300), 16000), {"extended": True}, RuntimeError, r"MI355X \(ROCm\) device.*no CPU fallback"),
], ids=lambda v: None if isinstance(v, (tuple, dict)) else getattr(v, "__name__", str(v))[:40])
def test_host_side_errors(args, kwargs, exc, match):
    with pytest.raises(exc, match=match):
        F.stoi(*args, **kwargs)


def test_a_waveform_that_requires_grad_is_refused():
    p = _z(2, 300).requires_grad_()
    with pytest.raises(RuntimeError, match="stoi is forward-only"):
        F.stoi(p, _z(2, 300), 10000)
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
        F.stoi(p, _z(2, 300), 10000)
