"""Batched edit distance without a GPU: the tie-ruled definition of tests/edit_distance_oracle.py against a plain DP and its
identities, a CPU replay of csrc/edit_distance.h (every configuration, both token and both length dtypes, with and without the
counts) against the definition, field for field, on shapes derived from the kernel's configurations, ragged and n-best batches,
impossible lengths between canaries, and the checks, exception types, names and signatures of the F.edit_distance* entries."""
import ctypes as C
import inspect
import os
import random
import subprocess

import numpy as np
import pytest
import torch

import edit_distance_oracle as O
import audio_amd.functional as F
from audio_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
SIM_SRC = os.path.join(HERE, "cpu_sim", "sim_edit_distance.cpp")
SIM_OUT = os.path.join(HERE, "cpu_sim", "_build", "libaamd_sim_edit_distance.so")
HDRS = [os.path.join(os.path.dirname(HERE), "audio_amd", "csrc", h) for h in ("edit_distance.h", "hd.h")]
INTS = [torch.int32, torch.int64]
CONFIGS, LIMITS = ((256, 4, 64), (1024, 4, 256), (4096, 16, 256)), (4096, 32767)      # test_sim_constants_...
SHAPES = O.exact_shapes(CONFIGS, LIMITS)
PAD = 64
CANARY = 77

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
        for fn in (_sim.sim_ed_states_per_lane, _sim.sim_ed_threads):
            fn.argtypes = [C.c_int64]
    return _sim


def _guarded(values, dtype, offset=0):
    """(whole buffer, the elements `offset` past the leading canaries) holding `values` (any integer array, flattened)."""
    v = torch.as_tensor(np.ascontiguousarray(values).reshape(-1)).to(dtype)
    buf = torch.full((v.numel() + 2 * PAD + offset,), CANARY, dtype=dtype)
    view = buf[PAD + offset:PAD + offset + v.numel()]
    view.copy_(v)
    return buf, view


def _canaries_intact(buf, n, offset=0):
    return bool((buf[:PAD + offset] == CANARY).all()) and bool((buf[PAD + offset + n:] == CANARY).all())


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def run_sim(hyps, refs, hyp_len=None, ref_len=None, hdtype=torch.int32, rdtype=torch.int32, hldtype=torch.int32,
            rldtype=torch.int32, return_ops=True, offset=0):
    """hyps (*lead, N), refs (*rlead, M) integer numpy arrays, lengths numpy arrays or None -> int64 numpy (*lead[, 4]).  Asserts
    the canaries round the output and round the inputs (which the replay must leave as they were)."""
    hyps, refs = np.asarray(hyps), np.asarray(refs)
    lead, N, M = hyps.shape[:-1], hyps.shape[-1], refs.shape[-1]
    pairs, rows = int(np.prod(lead, dtype=np.int64)), int(np.prod(refs.shape[:-1], dtype=np.int64))
    hbuf, h = _guarded(hyps, hdtype, offset)
    rbuf, r = _guarded(refs, rdtype)
    hl = None if hyp_len is None else torch.as_tensor(np.asarray(hyp_len).reshape(-1)).to(hldtype)
    rl = None if ref_len is None else torch.as_tensor(np.asarray(ref_len).reshape(-1)).to(rldtype)
    width = 4 if return_ops else 1
    obuf, out = _guarded(np.full(pairs * width, -7), torch.int32)
    before = (hbuf.clone(), rbuf.clone())
    dims = (C.c_int64 * 4)(pairs, pairs // rows if rows else 1, N, M)
    flags = (C.c_int32 * 5)(int(hdtype == torch.int64), int(rdtype == torch.int64), int(hldtype == torch.int64),
                            int(rldtype == torch.int64), int(return_ops))
    rc = sim().sim_edit_distance(_p(h), _p(r), _p(hl), _p(rl), dims, flags, _p(out))
    assert rc == 0
    assert _canaries_intact(obuf, pairs * width)
    assert torch.equal(hbuf, before[0]) and torch.equal(rbuf, before[1])
    res = out.to(torch.int64).numpy().copy()
    return res.reshape(lead + (4,)) if return_ops else res.reshape(lead)


# ---- the definition ---------------------------------------------------------------------------------------------------------

def test_definition_against_a_plain_dp_on_random_pairs():
    rng = random.Random(1)
    for n in range(450):
        alphabet = (2, 3, 30)[n % 3]
        ref = [rng.randrange(alphabet) for _ in range(rng.randrange(0, 41))]
        hyp = [rng.randrange(alphabet) for _ in range(rng.randrange(0, 41))]
        cell = O.ops(ref, hyp)
        assert cell[0] == O.distance(ref, hyp), (ref, hyp)
        assert O.identities_hold(len(ref), len(hyp), cell), (ref, hyp, cell)


def test_definition_on_every_binary_pair_up_to_length_5():
    pairs = O.binary_pairs(5)
    assert len(pairs) == 63 * 63
    for ref, hyp in pairs:
        cell = O.ops(ref, hyp)
        assert cell[0] == O.distance(ref, hyp) and O.identities_hold(len(ref), len(hyp), cell), (ref, hyp, cell)
    # the tie rule, by hand: diagonal first, then deletion, then insertion
    assert O.ops([0], [1]) == (1, 1, 0, 0)
    assert O.ops([0, 1], [1]) == (1, 0, 1, 0)
    assert O.ops([1], [0, 1]) == (1, 0, 0, 1)
    assert O.ops([0, 1], [1, 0]) == (2, 2, 0, 0)


# ---- the replay -------------------------------------------------------------------------------------------------------------

def test_replay_on_every_binary_pair_up_to_length_5():
    """All 3969 pairs as ONE ragged batch of width 5: the identities, and every field against the definition."""
    pairs = O.binary_pairs(5)
    hyps = np.full((len(pairs), 5), 9, dtype=np.int64)
    refs = np.full((len(pairs), 5), 8, dtype=np.int64)
    hl, rl = np.zeros(len(pairs), dtype=np.int64), np.zeros(len(pairs), dtype=np.int64)
    for p, (ref, hyp) in enumerate(pairs):
        refs[p, :len(ref)], hyps[p, :len(hyp)], rl[p], hl[p] = ref, hyp, len(ref), len(hyp)
    got = run_sim(hyps, refs, hl, rl)
    for p, (ref, hyp) in enumerate(pairs):
        cell = tuple(int(v) for v in got[p])
        assert O.identities_hold(len(ref), len(hyp), cell) and cell == O.ops(ref, hyp), (ref, hyp, cell)


@pytest.mark.parametrize("name", sorted(SHAPES), ids=str)
def test_replay_equals_the_definition(name):
    """Every shape, with a dtype combination walked by the shape; the counts and the distance-only output."""
    M, N = SHAPES[name]
    ref, hyp, want = O.case(name, M, N)
    k = sum(map(ord, name))
    hd, rd = INTS[k % 2], INTS[(k // 2) % 2]
    got = run_sim(np.array(hyp, dtype=np.int64).reshape(1, N), np.array(ref, dtype=np.int64).reshape(1, M), hdtype=hd, rdtype=rd)
    assert tuple(got[0]) == want, (name, got, want)
    assert O.identities_hold(M, N, want)
    dist = run_sim(np.array(hyp, dtype=np.int64).reshape(1, N), np.array(ref, dtype=np.int64).reshape(1, M), hdtype=rd, rdtype=hd,
                   return_ops=False)
    assert dist.shape == (1,) and int(dist[0]) == want[0]


@pytest.mark.parametrize("name", ["M7_N65", "M257_N65", "M1025_N63"], ids=str)                 # one per configuration
@pytest.mark.parametrize("hd,rd", [(a, b) for a in INTS for b in INTS], ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("ld", INTS, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("return_ops", [True, False])
def test_replay_in_every_configuration_and_dtype(name, hd, rd, ld, return_ops):
    """The pair inside wider tensors at an odd element offset, lengths given, garbage beyond them."""
    M, N = SHAPES[name]
    ref, hyp, want = O.case(name, M, N)
    hyps = np.full((2, N + 3), 1234, dtype=np.int64)
    refs = np.full((2, M), 4321, dtype=np.int64)
    hyps[1, :N], refs[1, :M] = hyp, ref
    refs[0, :5], hyps[0, :4] = [1, 2, 3, 4, 5], [1, 3, 4, 5]
    got = run_sim(hyps, refs, [4, N], [5, M], hd, rd, ld, ld, return_ops, offset=1)
    if return_ops:
        assert tuple(got[1]) == want and tuple(got[0]) == (1, 0, 1, 0)
    else:
        assert int(got[1]) == want[0] and int(got[0]) == 1


def test_replay_compares_int64_tokens_as_integers():
    ref, hyp, want = O.high_word_pair()
    low = O.ops([t % O.HIGH for t in ref], [t % O.HIGH for t in hyp])
    assert low != want                                                  # the high words matter
    got = run_sim(np.array([hyp]), np.array([ref]), hdtype=torch.int64, rdtype=torch.int64)
    assert tuple(got[0]) == want
    # an int32 tensor against an int64 one: equal values are equal
    small = [t % O.HIGH for t in ref]
    got = run_sim(np.array([small]), np.array([small]), hdtype=torch.int32, rdtype=torch.int64)
    assert tuple(got[0]) == (0, 0, 0, 0)
    neg = run_sim(np.array([[-1, -2, 3]]), np.array([[-1, -2, 3]]), hdtype=torch.int32, rdtype=torch.int64)
    assert tuple(neg[0]) == (0, 0, 0, 0)


@pytest.mark.parametrize("ld", INTS, ids=lambda d: str(d).split(".")[-1])
def test_replay_on_every_length_of_a_ragged_batch(ld):
    hyps, refs, hl, rl, want = O.grid_batch()
    got = run_sim(hyps, refs, hl, rl, hldtype=ld, rldtype=ld)
    assert np.array_equal(got, want)
    assert np.array_equal(run_sim(hyps, refs, hl, rl, hldtype=ld, rldtype=ld, return_ops=False), want[:, 0])


@pytest.mark.parametrize("M", [9, 257, 1025], ids=lambda m: "M%d" % m)                          # one per configuration
def test_replay_shares_a_reference_across_the_nbest_axis(M):
    hyps, refs, hl, rl, want = O.ragged_batch(M=M)
    assert (hl == -1).any() and (rl == 0).any() and (rl == M).any()
    got = run_sim(hyps, refs, hl, rl, hdtype=torch.int64, hldtype=torch.int64)
    assert np.array_equal(got, want)
    # row p of a batch equals the pair alone
    for b in range(hyps.shape[0]):
        for k in range(hyps.shape[1]):
            alone = run_sim(hyps[b, k][None], refs[b][None], hl[b, k][None], rl[b][None])
            assert np.array_equal(alone[0], want[b, k])
    # two leading reference axes under three hypothesis axes
    h5 = np.stack([hyps, hyps[::-1]]).reshape(2, 3, 2, 2, -1)
    r5 = np.stack([refs, refs[::-1]])
    w5 = np.stack([want, want[::-1]]).reshape(2, 3, 2, 2, 4)
    got = run_sim(h5, r5, np.stack([hl, hl[::-1]]).reshape(2, 3, 2, 2), np.stack([rl, rl[::-1]]))
    assert np.array_equal(got, w5)


@pytest.mark.parametrize("ld", INTS, ids=lambda d: str(d).split(".")[-1])
def test_impossible_lengths_read_nothing_and_give_minus_one(ld):
    """Lengths no tensor can have, CPU only: the outputs are -1, and (run_sim) no byte round the buffers changes.  The token
    buffers are exactly as wide as the tensors, so an index formed from such a length would leave them."""
    N, M = 6, 5
    bad_h = [-2, N + 1, 2 ** 31 - 1] + ([2 ** 32 + 3, -2 ** 40] if ld == torch.int64 else [-2 ** 31, -1])
    bad_r = [-1, M + 1, 2 ** 31 - 1] + ([2 ** 32 + 1, 2 ** 33] if ld == torch.int64 else [-2 ** 31, 2 ** 30])
    P = len(bad_h)
    hyps, refs = np.tile(np.arange(N), (2 * P + 1, 1)), np.tile(np.arange(M), (2 * P + 1, 1))
    hl = np.array(bad_h + [3] * P + [3], dtype=np.int64)
    rl = np.array([2] * P + bad_r + [2], dtype=np.int64)
    got = run_sim(hyps, refs, hl, rl, hldtype=ld, rldtype=ld)
    assert (got[:2 * P] == -1).all()
    assert tuple(got[2 * P]) == O.ops([0, 1], [0, 1, 2])
    assert (run_sim(hyps, refs, hl, rl, hldtype=ld, rldtype=ld, return_ops=False)[:2 * P] == -1).all()
    # a bad reference length condemns the whole block beneath it
    got = run_sim(np.tile(np.arange(N), (2, 3, 1)), np.tile(np.arange(M), (2, 1)), None, np.array([M + 1, M]), rldtype=ld)
    assert (got[0] == -1).all() and (got[1, :, 0] == 1).all()


def test_sim_constants_are_the_exported_ones():
    s = sim()
    assert (int(s.sim_ed_max_ref()), int(s.sim_ed_max_hyp())) == LIMITS == (F.EDIT_MAX_REF, F.EDIT_MAX_HYP)
    lo = 0
    for max_m, ks, nt in CONFIGS:
        for M in (lo if lo == 0 else lo + 1, max_m):
            assert (int(s.sim_ed_states_per_lane(M)), int(s.sim_ed_threads(M))) == (ks, nt)
        assert ks * nt >= max_m
        lo = max_m
    assert CONFIGS[-1][0] == LIMITS[0] and len(CONFIGS) >= 3
    assert LIMITS[0] >= 4096 and 32767 <= LIMITS[1] < 32768              # a field of a cell is 16 bits
    if not os.path.exists(_lib.LIB_PATH):
        return                                                          # the library is not built: nothing to compare with
    assert F.edit_distance_tiles() == (CONFIGS,) + LIMITS


# ---- the host side ----------------------------------------------------------------------------------------------------------

def test_names_and_signatures():
    for name in ("edit_distance", "edit_distance_batch", "edit_distance_tiles"):
        assert name in F.__all__ and callable(getattr(F, name))
    sig = inspect.signature(F.edit_distance_batch)
    assert list(sig.parameters) == ["hyps", "refs", "hyp_lengths", "ref_lengths", "return_ops"]
    assert [p.default for p in sig.parameters.values()] == [inspect.Parameter.empty, inspect.Parameter.empty, None, None, False]
    assert list(inspect.signature(F.edit_distance).parameters) == ["seq1", "seq2"]
    assert list(inspect.signature(F.edit_distance_tiles).parameters) == []
    assert "aamd_edit_distance" in _lib.EXPORTED_SYMBOLS


def _z(*shape, dtype=torch.int32):
    return torch.zeros(shape, dtype=dtype)


@pytest.mark.parametrize("args,exc,match", [
    ((_z(), _z(3)), ValueError, "token axis"),
    ((_z(3), _z()), ValueError, "token axis"),
    ((_z(2, 3, 5), _z(3, 4)), ValueError, "prefix"),
    ((_z(2, 5), _z(2, 3, 4)), ValueError, "prefix"),
    ((_z(2, 3, 5), _z(2, 4), _z(2)), ValueError, "hyp_lengths must have the shape"),
    ((_z(2, 3, 5), _z(2, 4), None, _z(2, 3)), ValueError, "ref_lengths must have the shape"),
    ((_z(2, 10)[:, ::2], _z(2, 4)), ValueError, "hyps must be contiguous"),
    ((_z(2, 5), _z(4, 2).t()), ValueError, "refs must be contiguous"),
    ((_z(2, 5), _z(2, 4), _z(4)[::2]), ValueError, "hyp_lengths must be contiguous"),
    ((_z(2, 5, dtype=torch.float32), _z(2, 4)), TypeError, "hyps must be int32 or int64"),
    ((_z(2, 5), _z(2, 4, dtype=torch.int16)), TypeError, "refs must be int32 or int64"),
    ((_z(2, 5, dtype=torch.bool), _z(2, 4)), TypeError, "hyps must be int32 or int64"),
    ((_z(2, 5), _z(2, 4), _z(2, dtype=torch.bool)), TypeError, "hyp_lengths must be int32 or int64"),
    ((_z(2, 5), _z(2, 4), None, _z(2, dtype=torch.float64)), TypeError, "ref_lengths must be int32 or int64"),
    ((_z(1, 5), _z(1, 4097)), NotImplementedError, "M = 4096"),
    ((_z(1, 32768), _z(1, 4)), NotImplementedError, "N = 32767"),
    ((_z(2, 5), _z(2, 4)), RuntimeError, r"hyps must be on an MI355X \(ROCm\) device.*no CPU fallback"),
    ((_z(0, 5), _z(0, 4)), RuntimeError, r"must be on an MI355X \(ROCm\) device.*no CPU fallback"),
], ids=lambda v: None if isinstance(v, tuple) else getattr(v, "__name__", str(v))[:40])
def test_host_side_errors(args, exc, match):
    with pytest.raises(exc, match=match):
        F.edit_distance_batch(*args)


def test_edit_distance_refuses_cpu_tensors_and_mixed_arguments():
    with pytest.raises(RuntimeError, match=r"must be on an MI355X \(ROCm\) device.*no CPU fallback"):
        F.edit_distance(_z(3), _z(4, dtype=torch.int64))
    with pytest.raises(ValueError, match="1-D"):
        F.edit_distance(_z(2, 3), _z(4))
    with pytest.raises(TypeError, match="two tensors or two Python sequences"):
        F.edit_distance(_z(3), [0, 0, 0])
    with pytest.raises(TypeError, match="int32 or int64"):
        F.edit_distance(_z(3, dtype=torch.float32), _z(3, dtype=torch.float32))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match=r"MI355X \(ROCm\) device.*no CPU fallback"):
            F.edit_distance("kitten", "sitting")
