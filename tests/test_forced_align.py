"""CTC forced alignment without a GPU: the float64 restatements of tests/forced_align_oracle.py against each other, a CPU replay
of csrc/forced_align.h (forward and backtrack; the four dtype paths, both target and length dtypes) against them on inputs
whose sums are exact, impossible lengths and labels between canaries, the checks and exception types of F.forced_align, and
F.merge_tokens / F.TokenSpan on hand-written cases."""
import ctypes as C
import functools
import inspect
import itertools
import os
import subprocess

import numpy as np
import pytest
import torch

import forced_align_oracle as O
import audio_amd.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
SIM_SRC = os.path.join(HERE, "cpu_sim", "sim_forced_align.cpp")
SIM_OUT = os.path.join(HERE, "cpu_sim", "_build", "libaamd_sim_forced_align.so")
HDRS = [os.path.join(os.path.dirname(HERE), "audio_amd", "csrc", h) for h in ("forced_align.h", "wave_augment.h", "spec_augment.h", "hd.h")]
CODE = {torch.float32: 0, torch.float64: 1, torch.float16: 2, torch.bfloat16: 3}
DTYPES = [torch.float32, torch.float64, torch.float16, torch.bfloat16]
INTS = [torch.int32, torch.int64]
CONFIGS, PF, BT, MAX_L = ((127, 4, 64), (511, 4, 256), (2047, 16, 256)), 4, 64, 2047      # test_sim_constants_...
SHAPES = O.exact_shapes(CONFIGS, PF, BT, MAX_L)
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
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", SIM_SRC, "-o", tmp])
            os.replace(tmp, SIM_OUT)
        _sim = C.CDLL(SIM_OUT)
        _sim.sim_fa_workspace.restype = C.c_int64
        _sim.sim_fa_workspace.argtypes = [C.c_int64] * 3
        for fn in (_sim.sim_fa_states_per_lane, _sim.sim_fa_threads):
            fn.argtypes = [C.c_int64]
    return _sim


def _guarded(n, dtype, offset=0):
    """(whole buffer, the n elements `offset` past the leading canaries)."""
    buf = torch.full((n + 2 * PAD + offset,), CANARY, dtype=dtype)
    return buf, buf[PAD + offset:PAD + offset + n]


def _canaries_intact(buf, n, offset=0):
    return bool((buf[:PAD + offset] == CANARY).all()) and bool((buf[PAD + offset + n:] == CANARY).all())


def _p(t):
    return C.c_void_p(t.data_ptr()) if t.numel() else None


def run_sim(lp, targets, in_len, tg_len, blank, dtype=torch.float32, tdtype=torch.int32, ldtype=torch.int32, offset=0):
    """lp (B, T, C) float64 numpy (rounded to `dtype` here) -> (paths int64 numpy, scores as a tensor of `dtype`, the lp tensor);
    asserts the canaries round every buffer the replay writes, and round its inputs."""
    s = sim()
    B, T, Cn = lp.shape
    L = targets.shape[1]
    xbuf, x = _guarded(lp.size, dtype, offset)
    x.copy_(torch.from_numpy(np.ascontiguousarray(lp)).reshape(-1).to(dtype))
    tbuf, tg = _guarded(B * L, tdtype)
    tg.copy_(torch.from_numpy(np.ascontiguousarray(targets)).reshape(-1))
    il, tl = torch.from_numpy(np.asarray(in_len)).to(ldtype), torch.from_numpy(np.asarray(tg_len)).to(ldtype)
    nws = int(s.sim_fa_workspace(B, T, L))
    wbuf, ws = _guarded(nws, torch.uint8)
    pbuf, paths = _guarded(B * T, tdtype)
    sbuf, scores = _guarded(B * T, dtype)
    dims = (C.c_int64 * 4)(B, T, Cn, L)
    rc = s.sim_forced_align(CODE[dtype], _p(x), _p(tg), int(tdtype == torch.int64), _p(il), _p(tl), int(ldtype == torch.int64),
                            dims, blank, _p(ws), _p(paths), _p(scores))
    assert rc == 0
    assert _canaries_intact(wbuf, nws) and _canaries_intact(pbuf, B * T) and _canaries_intact(sbuf, B * T)
    assert _canaries_intact(xbuf, lp.size, offset) and _canaries_intact(tbuf, B * L)
    return paths.to(torch.int64).numpy().reshape(B, T).copy(), scores.reshape(B, T).clone(), x.reshape(B, T, Cn).clone()


def bits(t):
    """The stored bits of a floating tensor, as integers."""
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def gathered(x, paths):
    """x[b, t, paths[b, t]] in the dtype of x."""
    return torch.gather(x, 2, torch.from_numpy(paths).clamp(min=0).unsqueeze(-1)).squeeze(-1)


@functools.lru_cache(maxsize=None)
def case(name):
    """The inputs of a named shape and the oracle's (paths, totals): built once."""
    args = O.exact_case(sum(map(ord, name)), **SHAPES[name])
    return args, O.expected(*args)


def check_exact(name, dtype, tdtype=torch.int32, ldtype=torch.int32, offset=0):
    (lp, targets, in_len, tg_len, blank), (want, _) = case(name)
    paths, scores, x = run_sim(lp, targets, in_len, tg_len, blank, dtype, tdtype, ldtype, offset)
    assert np.array_equal(x.to(torch.float64).numpy(), lp)     # the dtype holds these inputs exactly
    assert np.array_equal(paths, want), name
    want_scores = gathered(x, want)
    for b in range(lp.shape[0]):
        want_scores[b, int(in_len[b]):] = 0
    assert torch.equal(bits(scores), bits(want_scores)), name


# ---- the oracle's forms --------------------------------------------------------------------------------------------------------------

def _tiny_targets(L, Cn, blank):
    labels = [c for c in range(Cn) if c != blank]
    return [np.array(t, dtype=np.int64) for t in itertools.product(labels, repeat=L)]


@pytest.mark.parametrize("exact", [True, False])
def test_oracle_forms_agree_on_every_tiny_case(exact):
    """T <= 6, L <= 3, C <= 4, every transcript (repeats included) that fits: viterbi's total is the best over every labelling,
    and its path is one of the labellings that reach it."""
    rng = np.random.default_rng(1)
    n = 0
    for Cn, blank in ((2, 0), (3, 0), (3, 2), (4, 1)):
        for T in range(1, 7):
            lp = O.exact_lp(rng, T, Cn) if exact else np.log(rng.dirichlet(np.ones(Cn), size=T))
            for L in range(0, 4):
                for target in _tiny_targets(L, Cn, blank)[:6]:
                    if T < L + O.repeats(target):
                        continue
                    path, total = O.viterbi(lp, target, blank)
                    best, paths = O.brute_force(lp, target, blank)
                    assert O.is_alignment(path, target, blank)
                    if exact:                                    # every sum is exact: equal, and the path is a maximiser
                        assert total == best and O.path_total(lp, path) == best and tuple(path) in paths
                    else:
                        assert abs(total - best) <= 2 * T * 2.0 ** -52 * np.abs(lp).sum()
                    n += 1
    assert n > 150


def test_oracle_tie_rule():
    """x1 == x2 > x0 takes x1 (the reference's chain falls through to x0 there); every other tie keeps the smaller move."""
    # t = 2, state 3 (label 2): x0 = -1 - 3 = -4 (it was entered by a skip), x1 = -1 - 1 = -2 (blank), x2 = -1 - 1 = -2 (label 1)
    lp = np.array([[-1.0, -1.0, -1.0], [-1.0, -1.0, -3.0], [-5.0, -5.0, -0.5]])
    path, total = O.viterbi(lp, np.array([1, 2]), 0)
    assert path.tolist() == [1, 0, 2] and total == -2.5         # through the blank; the fall-through to x0 gives [1, 2, 2], -4.5
    assert O.brute_force(lp, np.array([1, 2]), 0)[0] == -2.5
    lp = np.zeros((3, 2))                                        # all ties: stay wherever possible, end in the label
    assert O.viterbi(lp, np.array([1]), 0)[0].tolist() == [1, 1, 1]


# ---- CPU replay of csrc/forced_align.h ------------------------------------------------------------------------------------------

def test_sim_constants_are_the_exported_ones():
    assert F.forced_align_tiles() == (CONFIGS, PF, BT, MAX_L)
    s = sim()
    assert (s.sim_fa_prefetch(), s.sim_fa_backtrack_block(), s.sim_fa_max_l()) == (PF, BT, MAX_L)
    lo = 0
    for last, ks, nt in CONFIGS:
        for L in (lo, last):
            assert (s.sim_fa_states_per_lane(L), s.sim_fa_threads(L)) == (ks, nt)
            assert 2 * L + 1 <= ks * nt
        lo = last + 1


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_sim_paths_equal_the_oracle(name):
    check_exact(name, torch.float32)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tdtype", INTS)
def test_sim_every_dtype(dtype, tdtype):
    for name in ("T1_L0", "T2_L1", "tight_run3", "L64", "L128", "T129_bt", "C5_blank4", "ragged"):
        check_exact(name, dtype, tdtype, ldtype=tdtype)
    check_exact("ragged", dtype, tdtype, ldtype=torch.int64 if tdtype == torch.int32 else torch.int32)
    check_exact("ragged", dtype, tdtype, offset=3)              # log_probs off the 16-byte grid


def test_sim_poisoned_padding_changes_nothing():
    (lp, targets, in_len, tg_len, blank), (want, _) = case("ragged")
    bad_lp, bad_t = lp.copy(), targets.copy()
    for b in range(3):
        bad_lp[b, in_len[b]:] = (np.nan, np.inf, -np.inf)[b]
        bad_t[b, tg_len[b]:] = (-7, 2 ** 30, blank)[b]
    assert not np.array_equal(bad_t, targets)
    paths, scores, _ = run_sim(bad_lp, bad_t, in_len, tg_len, blank)
    assert np.array_equal(paths, want)
    for b in range(3):
        assert bool((scores[b, int(in_len[b]):] == 0).all())


def test_sim_non_finite_log_probs_stay_in_bounds():
    """NaN and infinities inside the live frames: whatever path comes out, it is made of the example's own labels and the
    canaries are intact (asserted in run_sim)."""
    (lp, targets, in_len, tg_len, blank), _ = case("ragged")
    rng = np.random.default_rng(3)
    for fill in (np.nan, np.inf, -np.inf):
        x = lp.copy()
        x[rng.random(x.shape) < 0.3] = fill
        paths, scores, _ = run_sim(x, targets, in_len, tg_len, blank)
        for b in range(3):
            allowed = set(targets[b, :tg_len[b]].tolist()) | {blank}
            assert set(paths[b].tolist()) <= allowed


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.float16, torch.bfloat16])
def test_sim_impossible_examples_give_minus_one_and_nan_and_index_nothing(dtype):
    """Only here, never on a device: the middle example is impossible; its row is -1 / NaN, its neighbours are aligned as
    usual, and the canaries round every buffer are untouched (asserted in run_sim)."""
    T, L, Cn, blank = 12, 5, 6, 0
    lp, targets, in_len, tg_len, _ = O.exact_case(42, T, L, Cn, blank, lens=([12, 9, 6], [5, 4, 2]))
    targets[1, :4] = [1, 1, 1, 2]                               # R = 2: 9 >= 4 + 2
    assert O.repeats(targets[1, :4]) == 2
    want, _ = O.expected(lp, targets, in_len, tg_len, blank)
    assert np.array_equal(run_sim(lp, targets, in_len, tg_len, blank, dtype)[0], want)
    cases = [("il", 0), ("il", T + 1), ("il", -3), ("il", 10 ** 9), ("tl", L + 1), ("tl", -1), ("tl", 10 ** 9),
             ("il", 4 + 2 - 1),                                  # T_b = L_b + R_b - 1
             ("tg", -1), ("tg", Cn), ("tg", blank), ("tg", 2 ** 30), ("tg", -2 ** 31)]
    for what, value in cases:
        t2, il2, tl2 = targets.copy(), in_len.copy(), tg_len.copy()
        if what == "il":
            il2[1] = value
        elif what == "tl":
            tl2[1] = value
        else:
            t2[1, 3] = value                                     # live: target_lengths[1] == 4
        for tdtype in INTS:
            paths, scores, _ = run_sim(lp, t2, il2, tl2, blank, dtype, tdtype, tdtype)
            assert bool((paths[1] == -1).all()) and bool(torch.isnan(scores[1]).all()), (what, value)
            assert np.array_equal(paths[[0, 2]], want[[0, 2]]), (what, value)
    # exactly enough frames is possible, and a dead label outside the classes is not a fault
    il2 = in_len.copy()
    il2[1] = 6
    assert bool((run_sim(lp, targets, il2, tg_len, blank, dtype)[0][1] != -1).all())
    t2 = targets.copy()
    t2[1, 4] = 2 ** 30
    assert np.array_equal(run_sim(lp, t2, in_len, tg_len, blank, dtype)[0], want)


def test_sim_refuses_more_than_the_limit():
    dims = (C.c_int64 * 4)(1, 1, 2, MAX_L + 1)
    assert sim().sim_forced_align(0, None, None, 0, None, None, 0, dims, 0, None, None, None) == -2


# ---- the public surface -----------------------------------------------------------------------------------------------------------

def _cpu_args(B=2, T=6, Cn=5, L=3, dtype=torch.float32, tdtype=torch.int32):
    return (torch.zeros(B, T, Cn, dtype=dtype), torch.ones(B, L, dtype=tdtype), torch.full((B,), T, dtype=torch.int32),
            torch.full((B,), L, dtype=torch.int32))


def test_signatures_follow_the_reference():
    def sig(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]
    E = inspect.Parameter.empty
    assert sig(F.forced_align) == [("log_probs", E), ("targets", E), ("input_lengths", None), ("target_lengths", None), ("blank", 0)]
    assert sig(F.merge_tokens) == [("tokens", E), ("scores", E), ("blank", 0)]
    assert {"forced_align", "merge_tokens", "TokenSpan"} <= set(F.__all__)


def test_checks_and_exception_types():
    x, tg, il, tl = _cpu_args()
    with pytest.raises(ValueError):
        F.forced_align(x[0], tg, il, tl)                        # ranks
    with pytest.raises(ValueError):
        F.forced_align(x, tg[0], il, tl)
    with pytest.raises(ValueError):
        F.forced_align(x, tg, il.view(2, 1), tl)
    with pytest.raises(ValueError):
        F.forced_align(x, tg[:1], il, tl)                       # batch sizes
    with pytest.raises(ValueError):
        F.forced_align(x, tg, il[:1], tl)
    with pytest.raises(ValueError):
        F.forced_align(x, tg, il, torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError):
        F.forced_align(x.transpose(1, 2).contiguous().transpose(1, 2), tg, il, tl)        # contiguity
    with pytest.raises(ValueError):
        F.forced_align(x, torch.ones(2, 6, dtype=torch.int32)[:, ::2], il, tl)
    with pytest.raises(ValueError):
        F.forced_align(x, tg, torch.ones(4, dtype=torch.int32)[::2], tl)
    for blank in (5, -1, 100):
        with pytest.raises(ValueError, match="blank must be within"):
            F.forced_align(x, tg, il, tl, blank=blank)
    with pytest.raises(TypeError):
        F.forced_align(x.to(torch.int32), tg, il, tl)
    with pytest.raises(TypeError):
        F.forced_align(x, tg.to(torch.int16), il, tl)
    with pytest.raises(TypeError):
        F.forced_align(x, tg.float(), il, tl)
    with pytest.raises(TypeError):
        F.forced_align(x, tg, il.to(torch.int16), tl)
    with pytest.raises(TypeError):
        F.forced_align(x, tg, il, tl.float())
    big = _cpu_args(1, 1, 2, MAX_L + 1)
    with pytest.raises(NotImplementedError, match=str(MAX_L)):
        F.forced_align(*big)


def test_cpu_tensors_are_refused():
    for dtype in DTYPES:
        for tdtype in INTS:
            args = _cpu_args(dtype=dtype, tdtype=tdtype)
            for call in (lambda: F.forced_align(*args), lambda: F.forced_align(args[0], args[1]),
                         lambda: F.forced_align(*args, blank=4)):
                with pytest.raises(RuntimeError, match="no CPU fallback"):
                    call()


def test_no_dispatcher_op_is_registered():
    """A plain Python entry point through the C ABI: the op sets of the two namespaces stay as they are."""
    from audio_amd import _ops  # noqa: F401
    assert not hasattr(torch.ops.audio_amd, "forced_align")


# ---- merge_tokens / TokenSpan ------------------------------------------------------------------------------------------------------

def test_token_span():
    s = F.TokenSpan(token=3, start=2, end=7, score=-0.5)
    assert len(s) == 5 and (s.token, s.start, s.end, s.score) == (3, 2, 7, -0.5)
    assert s == F.TokenSpan(3, 2, 7, -0.5)


def test_merge_tokens_on_hand_written_cases():
    tokens = torch.tensor([0, 0, 1, 1, 1, 0, 1, 2, 2, 0])      # leading and trailing blank runs; 1, blank, 1 gives two spans
    scores = torch.tensor([-9.0, -9.0, -1.0, -2.0, -3.0, -9.0, -4.0, -0.5, -1.5, -9.0])
    assert F.merge_tokens(tokens, scores) == [F.TokenSpan(1, 2, 5, -2.0), F.TokenSpan(1, 6, 7, -4.0), F.TokenSpan(2, 7, 9, -1.0)]
    assert F.merge_tokens(tokens, scores, blank=2) == [F.TokenSpan(0, 0, 2, -9.0), F.TokenSpan(1, 2, 5, -2.0),
                                                       F.TokenSpan(0, 5, 6, -9.0), F.TokenSpan(1, 6, 7, -4.0),
                                                       F.TokenSpan(0, 9, 10, -9.0)]
    assert F.merge_tokens(torch.zeros(0, dtype=torch.int64), torch.zeros(0)) == []
    assert F.merge_tokens(torch.zeros(4, dtype=torch.int32), torch.zeros(4)) == []          # all blank
    assert F.merge_tokens(torch.tensor([5]), torch.tensor([-0.25], dtype=torch.float64)) == [F.TokenSpan(5, 0, 1, -0.25)]


def test_merge_tokens_scores_are_float64_means_of_the_stored_values():
    tokens = torch.tensor([1, 1, 1, 2], dtype=torch.int32)
    for dtype in DTYPES:
        scores = torch.tensor([-0.1, -0.2, -0.7, -0.3]).to(dtype)
        spans = F.merge_tokens(tokens, scores)
        want = scores[:3].to(torch.float64).numpy().mean()
        assert spans[0].score == want and spans[1].score == float(scores[3].to(torch.float64))
        assert all(isinstance(s.score, float) and isinstance(s.token, int) for s in spans)


def test_merge_tokens_checks():
    with pytest.raises(ValueError, match="`tokens` and `scores` must be 1D Tensor."):
        F.merge_tokens(torch.zeros(1, 3, dtype=torch.int64), torch.zeros(3))
    with pytest.raises(ValueError, match="`tokens` and `scores` must be 1D Tensor."):
        F.merge_tokens(torch.zeros(3, dtype=torch.int64), torch.zeros(1, 3))
    with pytest.raises(ValueError, match="`tokens` and `scores` must be the same length."):
        F.merge_tokens(torch.zeros(3, dtype=torch.int64), torch.zeros(4))
