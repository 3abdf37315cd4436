"""The transducer loss without a GPU: the three float64 restatements of tests/rnnt_oracle.py against each other, a CPU replay of
csrc/rnnt_loss.h (row pass, lattice, gradient pass; the four dtype paths, fused and not) against them, impossible lengths and
labels between canaries, signatures, checks and exception types, Meta shapes, TorchScript and torch.compile seeing one op."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest
import torch

import rnnt_oracle as O
import audio_amd.functional as F
import audio_amd.transforms as T
from audio_amd import _ops  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
SIM_SRC = os.path.join(HERE, "cpu_sim", "sim_rnnt_loss.cpp")
SIM_OUT = os.path.join(HERE, "cpu_sim", "_build", "libaamd_sim_rnnt_loss.so")
HDRS = [os.path.join(os.path.dirname(HERE), "audio_amd", "csrc", h) for h in ("rnnt_loss.h", "wave_augment.h", "spec_augment.h", "hd.h")]
CODE = {torch.float32: 0, torch.float64: 1, torch.float16: 2, torch.bfloat16: 3}
U_ARITH = {torch.float32: 2.0 ** -23, torch.float64: 2.0 ** -52, torch.float16: 2.0 ** -23, torch.bfloat16: 2.0 ** -23}
# half an ulp of a stored element, relative, and the absolute floor of the format's subnormals
HALF_ULP = {torch.float32: (0.0, 0.0), torch.float64: (0.0, 0.0), torch.float16: (2.0 ** -11, 2.0 ** -25),
            torch.bfloat16: (2.0 ** -8, 0.0)}
DTYPES = [torch.float32, torch.float64, torch.float16, torch.bfloat16]
PAD = 64
CANARY = 12345.5

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
        _sim.sim_rnnt_workspace.restype = C.c_int64
        _sim.sim_rnnt_workspace.argtypes = [C.c_int64] * 3
        _sim.sim_rnnt_team_width.argtypes = [C.c_int, C.c_int64]
    return _sim


def _guarded(n, dtype, offset=0):
    """(whole buffer, the n elements `offset` past the leading canaries)."""
    buf = torch.full((n + 2 * PAD + offset,), CANARY, dtype=dtype)
    return buf, buf[PAD + offset:PAD + offset + n]


def _canaries_intact(buf, n, offset=0):
    return bool((buf[:PAD + offset] == CANARY).all()) and bool((buf[PAD + offset + n:] == CANARY).all())


def _p(t):
    return C.c_void_p(t.data_ptr()) if t.numel() else None


def run_sim(logits, targets, ll, tl, blank, dtype, fused=True, clamp=-1.0, grad_costs=None, offset=0):
    """logits float64 numpy (rounded to `dtype` here) -> (the rounded logits as float64, costs, gradient as float64,
    workspace dict); asserts the canaries round every written buffer."""
    s = sim()
    B, Tt, U1, V = logits.shape
    n = logits.size
    xbuf, x = _guarded(n, dtype, offset)
    x.copy_(torch.from_numpy(np.ascontiguousarray(logits)).reshape(-1).to(dtype))
    tg = torch.from_numpy(np.ascontiguousarray(targets, dtype=np.int32))
    llt, tlt = torch.from_numpy(np.asarray(ll, dtype=np.int32)), torch.from_numpy(np.asarray(tl, dtype=np.int32))
    dims = (C.c_int64 * 4)(B, Tt, U1, V)
    nws = int(s.sim_rnnt_workspace(B, Tt, U1)) // 8
    wbuf, ws = _guarded(nws, torch.float64)
    cbuf, costs = _guarded(B, torch.float64)
    bl = blank + V if blank < 0 else blank
    rc = s.sim_rnnt_forward(CODE[dtype], _p(x), _p(tg), _p(llt), _p(tlt), dims, bl, int(fused), _p(ws), _p(costs))
    assert rc == 0
    gbuf, g = _guarded(n, dtype, offset)
    gc = torch.ones(B, dtype=torch.float64) if grad_costs is None else torch.from_numpy(np.asarray(grad_costs, dtype=np.float64))
    rc = s.sim_rnnt_backward(CODE[dtype], _p(x), _p(tg), _p(llt), _p(tlt), dims, bl, int(fused), C.c_double(clamp), _p(ws), _p(gc),
                             _p(g))
    assert rc == 0
    assert _canaries_intact(wbuf, nws) and _canaries_intact(cbuf, B) and _canaries_intact(gbuf, n, offset)
    assert _canaries_intact(xbuf, n, offset)
    cells = B * Tt * U1
    w = ws.numpy()
    parts = {k: w[i * cells:(i + 1) * cells].reshape(B, Tt, U1) for i, k in enumerate(("denom", "lpb", "lpt", "alpha", "beta"))}
    parts["bad"] = w[5 * cells:].view(np.int32)[:B].copy()
    return (x.to(torch.float64).numpy().reshape(logits.shape), costs.numpy().copy(),
            g.to(torch.float64).numpy().reshape(logits.shape).copy(), parts)


def check(dtype, shape, lengths=None, blank=-1, fused=True, clamp=-1.0, seed=0, offset=0, grad_costs=None, scale=3.0):
    rng = np.random.default_rng(seed)
    logits, targets, ll, tl = O.inputs(rng, *shape, lengths=lengths, scale=scale, blank=blank)
    if not fused:
        logits = O._log_softmax(logits)
    x, costs, grad, ws = run_sim(logits, targets, ll, tl, blank, dtype, fused, clamp, grad_costs, offset)
    want_c, want_g, lats = O.closed_form(x, targets, ll, tl, blank, clamp, fused, grad_costs, want_lattices=True)
    cb, gb = O.bounds(x, ll, tl, U_ARITH[dtype])
    rel, floor = HALF_ULP[dtype]
    scale_g = np.abs(np.asarray(grad_costs, dtype=np.float64)).reshape(-1, 1, 1, 1) if grad_costs is not None else 1.0
    tol_g = gb.reshape(-1, 1, 1, 1) * scale_g + rel * np.abs(want_g) + floor
    fc, fg = (np.abs(costs - want_c) / cb).max(), (np.abs(grad - want_g) / tol_g).max()
    print(f"{dtype} {shape} fused={fused}: cost error {fc:.4f} of its bound, gradient error {fg:.4f}")
    assert fc <= 1.0 and fg <= 1.0, (fc, fg)
    for b in range(shape[0]):
        Tb, Ub = int(ll[b]), int(tl[b])
        assert ws["bad"][b] == 0
        # the padding: exactly zero
        mask = np.ones(shape[1:3], dtype=bool)
        mask[:Tb, :Ub + 1] = False
        assert np.all(grad[b][mask] == 0.0)
        # the lattices, and the cost taken from either end
        alpha, beta = lats[b]
        got_a, got_b = ws["alpha"][b, :Tb, :Ub + 1], ws["beta"][b, :Tb, :Ub + 1]
        assert np.all(np.abs(got_a - alpha) <= cb[b]) and np.all(np.abs(got_b - beta) <= cb[b])
        # -beta[0][0] is the cost; the alpha end is the same sum in another order, both in float64
        alpha_end = got_a[Tb - 1, Ub] + ws["lpb"][b, Tb - 1, Ub]
        largest = max(1.0, np.abs(got_a).max(), np.abs(got_b).max())
        assert abs(alpha_end - got_b[0, 0]) <= 8 * (Tb + Ub) * 2.0 ** -52 * largest
        assert costs[b] == -got_b[0, 0]
    return costs, grad


# ---- the oracle's three forms ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fused", [True, False])
def test_oracle_forms_agree(fused):
    rng = np.random.default_rng(1)
    for shape, lengths, blank in (((3, 4, 4, 5), ([4, 3, 1], [3, 1, 0]), -1), ((2, 3, 3, 4), ([3, 2], [2, 2]), 0),
                                  ((2, 5, 2, 6), ([5, 1], [1, 0]), 2), ((1, 1, 1, 3), ([1], [0]), -1)):
        logits, targets, ll, tl = O.inputs(rng, *shape, lengths=lengths, blank=blank)
        if not fused:
            logits = O._log_softmax(logits)
        gc = rng.standard_normal(shape[0])
        for clamp in (-1.0, 0.05):
            a = O.recurrence(logits, targets, ll, tl, blank, clamp, fused, gc)
            b = O.brute_force(logits, targets, ll, tl, blank, clamp, fused, gc)
            c = O.closed_form(logits, targets, ll, tl, blank, clamp, fused, gc)
            for p, q in ((a, b), (a, c)):
                assert np.abs(p[0] - q[0]).max() <= 1e-10 and np.abs(p[1] - q[1]).max() <= 1e-10
        if shape[0] > 1:                                         # the clamp of these cases bites
            assert np.abs(O.recurrence(logits, targets, ll, tl, blank, 0.05, fused)[1]).max() == 0.05


def test_oracle_recurrence_and_closed_form_agree_beyond_brute_force():
    rng = np.random.default_rng(2)
    logits, targets, ll, tl = O.inputs(rng, 2, 9, 6, 11)
    a, c = O.recurrence(logits, targets, ll, tl), O.closed_form(logits, targets, ll, tl)
    assert np.abs(a[0] - c[0]).max() <= 1e-10 and np.abs(a[1] - c[1]).max() <= 1e-10


# ---- CPU replay of csrc/rnnt_loss.h ----------------------------------------------------------------------------------------------

def test_sim_constants_are_the_exported_ones():
    widths, lat_threads, max_u1 = F.rnnt_tiles()
    assert widths == (8, 16, 32, 64)
    assert lat_threads == sim().sim_rnnt_lattice_threads() and max_u1 == sim().sim_rnnt_max_u1() == 1024
    for dt in DTYPES:
        for V in (1, 15, 16, 17, 29, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1024, 4099):
            assert F.rnnt_team_width(dt, V) == sim().sim_rnnt_team_width(CODE[dt], V) and F.rnnt_team_width(dt, V) in widths


@pytest.mark.parametrize("dtype", DTYPES)
def test_sim_against_the_oracle(dtype):
    check(dtype, (3, 4, 4, 5), ([4, 3, 1], [3, 1, 0]))
    check(dtype, (4, 17, 10, 37), seed=1)                      # every 16-byte residue of the row start
    check(dtype, (2, 5, 3, 261), seed=2)
    check(dtype, (1, 2, 3, 4099), seed=3)                      # several vector iterations per lane and a tail
    check(dtype, (1, 1, 1, 1), ([1], [0]))


@pytest.mark.parametrize("dtype", DTYPES)
def test_sim_rows_that_start_anywhere(dtype):
    for offset in (1, 2, 3, 5):                                # the tensor itself does not start on a 16-byte boundary
        check(dtype, (2, 3, 3, 37), seed=offset, offset=offset)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_sim_vocabularies_round_the_team_widths(dtype):
    vec = 16 // torch.empty((), dtype=dtype).element_size()
    for w in (8, 16, 32, 64):
        for V in (w * vec - 1, w * vec, w * vec + 1, w - 1, w, w + 1):
            check(dtype, (2, 3, 2, V), seed=V)


def test_sim_lattice_shapes():
    nt = sim().sim_rnnt_lattice_threads()
    check(torch.float32, (1, 3, nt + 1, 3), seed=4)            # two columns per lane
    check(torch.float32, (2, 2, 2 * nt + 3, 3), seed=5)        # four
    check(torch.float64, (1, 2, 1024, 2), seed=6)              # the limit
    check(torch.float32, (1, 300, 2, 3), seed=7)               # a long T with a thin U
    check(torch.float64, (2, 40, 1, 4), seed=8)                # no targets at all


@pytest.mark.parametrize("dtype", DTYPES)
def test_sim_blank_clamp_grad_costs_and_not_fused(dtype):
    for blank in (-1, 0, 3):
        check(dtype, (2, 6, 4, 7), blank=blank, seed=10 + blank)
    c, g = check(dtype, (2, 6, 4, 7), clamp=0.1, seed=20, grad_costs=[0.5, -2.0])
    assert np.abs(g[0]).max() == pytest.approx(0.05, rel=2.0 ** -7) and np.abs(g[1]).max() == pytest.approx(0.2, rel=2.0 ** -7)
    for blank in (-1, 2):
        check(dtype, (3, 5, 4, 9), blank=blank, fused=False, seed=30)
    check(dtype, (2, 5, 4, 9), fused=False, clamp=0.2, seed=31, grad_costs=[3.0, 0.25])


def test_sim_extreme_rows():
    """The largest logit in the last element, the first, at blank, at the target; a row of equal values; -inf entries."""
    rng = np.random.default_rng(40)
    logits, targets, ll, tl = O.inputs(rng, 2, 4, 3, 70, lengths=([4, 4], [2, 2]))
    logits[0, 0, 0, -2] = 60.0
    logits[0, 1, 0, 0] = 60.0
    logits[0, 2, 1, -1] = 60.0                                 # blank
    logits[1, 0, 0, targets[1, 0]] = 60.0
    logits[1, 1, 1, :] = 0.25
    logits[1, 2, 0, 5:40] = -np.inf
    for dtype in (torch.float32, torch.float64):
        x, costs, grad, ws = run_sim(logits, targets, ll, tl, -1, dtype)
        want_c, want_g = O.closed_form(x, targets, ll, tl)
        cb, gb = O.bounds(x, ll, tl, U_ARITH[dtype])
        assert np.all(np.abs(costs - want_c) <= cb) and np.all(np.abs(grad - want_g) <= gb.reshape(-1, 1, 1, 1))


def test_sim_poisoned_padding_changes_nothing():
    rng = np.random.default_rng(41)
    logits, targets, ll, tl = O.inputs(rng, 3, 5, 4, 11, lengths=([5, 3, 1], [3, 1, 0]))
    clean = run_sim(logits, targets, ll, tl, -1, torch.float32)
    bad_l, bad_t = logits.copy(), targets.copy()
    for b in range(3):
        fill = (np.nan, np.inf, -np.inf)[b]
        bad_l[b, ll[b]:] = fill
        bad_l[b, :, tl[b] + 1:] = fill
        bad_t[b, tl[b]:] = (-7, 11, 2 ** 30)[b]
    dirty = run_sim(bad_l, bad_t, ll, tl, -1, torch.float32)
    assert np.array_equal(clean[1], dirty[1]) and np.array_equal(clean[2], dirty[2])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.bfloat16])
@pytest.mark.parametrize("fused", [True, False])
def test_sim_impossible_lengths_and_labels_give_nan_and_index_nothing(dtype, fused):
    """Only here, never on a device: the middle example is impossible; its cost and gradient block are NaN, its neighbours
    are judged as usual, and the canaries round every buffer are untouched (asserted in run_sim)."""
    rng = np.random.default_rng(42)
    B, Tt, U1, V = 3, 5, 4, 9
    base = O.inputs(rng, B, Tt, U1, V, lengths=([5, 4, 2], [3, 2, 1]))
    cases = [("ll", 0), ("ll", -3), ("ll", Tt + 1), ("ll", 10 ** 9), ("tl", -1), ("tl", U1), ("tl", 10 ** 9),
             ("tg", V), ("tg", -1), ("tg", 2 ** 30), ("tg", -2 ** 31)]
    for what, value in cases:
        logits, targets, ll, tl = (v.copy() for v in base)
        if not fused:
            logits = O._log_softmax(logits)
        if what == "ll":
            ll[1] = value
        elif what == "tl":
            tl[1] = value
        else:
            targets[1, 1] = value                               # live: target_lengths[1] == 2
        x, costs, grad, ws = run_sim(logits, targets, ll, tl, -1, dtype, fused)
        assert ws["bad"].tolist() == [0, 1, 0], (what, value)
        assert np.isnan(costs[1]) and np.isnan(grad[1]).all(), (what, value)
        keep = [0, 2]
        want_c, want_g = O.closed_form(x[keep], targets[keep], base[2][keep], base[3][keep], -1, -1.0, fused)
        cb, gb = O.bounds(x[keep], base[2][keep], base[3][keep], U_ARITH[dtype])
        rel, floor = HALF_ULP[dtype]
        assert np.all(np.abs(costs[keep] - want_c) <= cb), (what, value)
        assert np.all(np.abs(grad[keep] - want_g) <= gb.reshape(-1, 1, 1, 1) + rel * np.abs(want_g) + floor), (what, value)
    # a dead label outside the vocabulary is not a fault
    logits, targets, ll, tl = (v.copy() for v in base)
    targets[1, 2] = 2 ** 30
    assert run_sim(logits, targets, ll, tl, -1, dtype, True)[3]["bad"].tolist() == [0, 0, 0]


def test_sim_refuses_more_than_the_limit():
    x = torch.zeros(1 * 1 * 1025 * 2)
    dims = (C.c_int64 * 4)(1, 1, 1025, 2)
    assert sim().sim_rnnt_forward(0, _p(x), None, None, None, dims, 1, 1, None, None) == -2


# ---- the public surface -----------------------------------------------------------------------------------------------------------

def _cpu_args(B=2, Tt=3, U1=3, V=5, dtype=torch.float32):
    return (torch.zeros(B, Tt, U1, V, dtype=dtype), torch.zeros(B, U1 - 1, dtype=torch.int32),
            torch.full((B,), Tt, dtype=torch.int32), torch.full((B,), U1 - 1, dtype=torch.int32))


def test_signatures_follow_the_reference():
    def sig(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]
    E = inspect.Parameter.empty
    assert sig(F.rnnt_loss) == [("logits", E), ("targets", E), ("logit_lengths", E), ("target_lengths", E), ("blank", -1),
                                ("clamp", -1), ("reduction", "mean"), ("fused_log_softmax", True)]
    assert sig(T.RNNTLoss.__init__)[1:] == [("blank", -1), ("clamp", -1.0), ("reduction", "mean"), ("fused_log_softmax", True)]
    assert sig(T.RNNTLoss.forward)[1:] == [("logits", E), ("targets", E), ("logit_lengths", E), ("target_lengths", E)]
    assert "rnnt_loss" in F.__all__ and "RNNTLoss" in T.__all__


def test_checks_and_exception_types():
    x, tg, ll, tl = _cpu_args()
    with pytest.raises(ValueError, match="reduction should be one of 'none', 'mean', or 'sum'"):
        F.rnnt_loss(x, tg, ll, tl, reduction="avg")
    with pytest.raises(ValueError):
        F.rnnt_loss(x[0], tg, ll, tl)                          # ranks
    with pytest.raises(ValueError):
        F.rnnt_loss(x, tg[0], ll, tl)
    with pytest.raises(ValueError):
        F.rnnt_loss(x, tg, ll.view(2, 1), tl)
    with pytest.raises(ValueError):
        F.rnnt_loss(x, tg[:1], ll, tl)                         # batch sizes
    with pytest.raises(ValueError):
        F.rnnt_loss(x, tg, ll[:1], tl)
    with pytest.raises(ValueError):
        F.rnnt_loss(x, tg, ll, torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError):
        F.rnnt_loss(x, torch.zeros(2, 3, dtype=torch.int32), ll, tl)          # U + 1
    with pytest.raises(ValueError):
        F.rnnt_loss(x.transpose(1, 2).contiguous().transpose(1, 2), tg, ll, tl)   # contiguity
    with pytest.raises(ValueError):
        F.rnnt_loss(x, torch.zeros(2, 4, dtype=torch.int32)[:, ::2], ll, tl)
    with pytest.raises(TypeError):
        F.rnnt_loss(x.to(torch.int32), tg, ll, tl)
    with pytest.raises(TypeError):
        F.rnnt_loss(x, tg.long(), ll, tl)
    with pytest.raises(TypeError):
        F.rnnt_loss(x, tg, ll.long(), tl)
    with pytest.raises(TypeError):
        F.rnnt_loss(x, tg, ll, tl.to(torch.int16))
    for blank in (5, -6, 100):
        with pytest.raises(ValueError, match="blank"):
            F.rnnt_loss(x, tg, ll, tl, blank=blank)
    with pytest.raises(ValueError, match="reduction"):
        T.RNNTLoss(reduction="avg")(x, tg, ll, tl)
    big = _cpu_args(1, 1, 1026, 2)
    with pytest.raises(NotImplementedError, match="1024"):
        F.rnnt_loss(*big)


def test_cpu_tensors_are_refused():
    for dtype in DTYPES:
        args = _cpu_args(dtype=dtype)
        for call in (lambda: F.rnnt_loss(*args), lambda: F.rnnt_loss(*args, blank=0, clamp=1.0, reduction="none",
                                                                   fused_log_softmax=False), lambda: T.RNNTLoss()(*args)):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                call()


def _meta_args(B=2, Tt=3, U1=4, V=5, dtype=torch.float32):
    return (torch.empty(B, Tt, U1, V, device="meta", dtype=dtype), torch.empty(B, U1 - 1, device="meta", dtype=torch.int32),
            torch.empty(B, device="meta", dtype=torch.int32), torch.empty(B, device="meta", dtype=torch.int32))


def test_meta_kernel():
    for dtype in DTYPES:
        args = _meta_args(dtype=dtype)
        out = torch.ops.audio_amd.rnnt_loss(*args, 4, -1.0, "none", True)
        assert out.shape == (2,) and out.dtype == dtype
        for red in ("mean", "sum"):
            out = torch.ops.audio_amd.rnnt_loss(*args, 4, -1.0, red, False)
            assert out.shape == () and out.dtype == dtype
    with pytest.raises(ValueError, match="reduction"):
        torch.ops.audio_amd.rnnt_loss(*_meta_args(), 4, -1.0, "avg", True)


def test_compiles_under_torchscript():
    for mod in (T.RNNTLoss(), T.RNNTLoss(0, 1.0, "none", False)):
        s = torch.jit.script(mod)
        assert str(s.inlined_graph).count("audio_amd::rnnt_loss") == 1
        with pytest.raises(Exception, match="CPU"):            # the op has no CPU kernel: refused by the dispatcher
            s(*_cpu_args())
    s = torch.jit.script(T.RNNTLoss(reduction="none"))
    assert s(*_meta_args()).shape == (2,)
    f = torch.jit.script(F.rnnt_loss)
    assert f(*_meta_args()).shape == ()


def test_torch_compile_sees_one_op():
    graphs = []

    def backend(gm, example_inputs):
        graphs.append(gm)
        return gm.forward

    y = torch.compile(T.RNNTLoss(reduction="sum"), fullgraph=True, backend=backend)(*_meta_args())
    assert y.shape == ()
    calls = [str(n.target) for n in graphs[-1].graph.nodes if n.op == "call_function" and "audio_amd" in str(n.target)]
    assert calls == ["audio_amd.rnnt_loss"]
