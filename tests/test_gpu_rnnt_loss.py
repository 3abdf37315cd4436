"""F.rnnt_loss / T.RNNTLoss on the MI355X against the float64 restatements of tests/rnnt_oracle.py.

Bounds come from the oracle and the inputs, never from the code under test.  With u the unit roundoff of the kernels'
per-element arithmetic (2^-23 for float32, float16 and bfloat16 tensors, 2^-52 for float64) and
eps_cell = u (V + 8 + 2 max|logits|) the worst-order bound of one log-sum-exp plus its exp / log roundings:

    cost      |err_b| <= (T_b + U_b) eps_cell                      (a path crosses T_b + U_b cells)
    gradient  |err|   <= 2 ((T_b + U_b + 2) eps_cell + 16 u)       (every term is a probability times an occupancy, <= 1)

float16 / bfloat16 results add half an ulp of the stored element.  Every check prints the achieved fraction of its bound.
Impossible lengths and labels are exercised in tests/test_rnnt_loss.py (CPU replay between canaries) only, never here."""
import functools

import numpy as np
import pytest
import torch

import rnnt_oracle as O
import audio_amd.functional as F
import audio_amd.transforms as T

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float32, torch.float64, torch.float16, torch.bfloat16]
U_ARITH = {torch.float32: 2.0 ** -23, torch.float64: 2.0 ** -52, torch.float16: 2.0 ** -23, torch.bfloat16: 2.0 ** -23}
HALF_ULP = {torch.float32: (0.0, 0.0), torch.float64: (0.0, 0.0), torch.float16: (2.0 ** -11, 2.0 ** -25),
            torch.bfloat16: (2.0 ** -8, 0.0)}
WIDTHS, LAT_THREADS, MAX_U1 = (8, 16, 32, 64), 256, 1024       # test_tiles_are_the_exported_constants


def rounded(logits, dtype):
    """The float64 values a tensor of `dtype` holds for these logits."""
    return torch.from_numpy(np.ascontiguousarray(logits)).to(dtype).to(torch.float64).numpy()


def device_args(x, targets, ll, tl, dtype, offset=0):
    n = x.size
    buf = torch.zeros(n + offset, dtype=dtype, device=DEV)
    xt = buf[offset:].view(x.shape)
    xt.copy_(torch.from_numpy(x).to(dtype))
    assert xt.is_contiguous()
    return (xt, torch.from_numpy(np.ascontiguousarray(targets, dtype=np.int32)).to(DEV),
            torch.from_numpy(np.asarray(ll, dtype=np.int32)).to(DEV), torch.from_numpy(np.asarray(tl, dtype=np.int32)).to(DEV))


def run(x, targets, ll, tl, dtype, blank=-1, clamp=-1.0, fused=True, grad_costs=None, offset=0):
    """(costs, gradient) as float64 numpy of the device call with reduction "none" and the cotangent grad_costs."""
    xt, tg, llt, tlt = device_args(x, targets, ll, tl, dtype, offset)
    xt.requires_grad_(True)
    costs = F.rnnt_loss(xt, tg, llt, tlt, blank, clamp, "none", fused)
    assert costs.shape == (x.shape[0],) and costs.dtype == dtype
    gc = torch.ones(x.shape[0], dtype=torch.float64) if grad_costs is None else torch.tensor(grad_costs, dtype=torch.float64)
    costs.backward(gc.to(dtype).to(DEV))
    assert xt.grad.dtype == dtype and xt.grad.shape == xt.shape
    return costs.detach().double().cpu().numpy(), xt.grad.double().cpu().numpy()


def judge(what, dtype, x, ll, tl, got, want, grad_costs=None):
    (costs, grad), (want_c, want_g) = got, want
    cb, gb = O.bounds(x, ll, tl, U_ARITH[dtype])
    rel, floor = HALF_ULP[dtype]
    scale = np.abs(np.asarray(grad_costs, dtype=np.float64)).reshape(-1, 1, 1, 1) if grad_costs is not None else 1.0
    tol_c = cb + rel * np.abs(want_c) + floor                  # the cost is returned in the dtype of logits
    tol_g = gb.reshape(-1, 1, 1, 1) * scale + rel * np.abs(want_g) + floor
    fc, fg = (np.abs(costs - want_c) / tol_c).max(), (np.abs(grad - want_g) / tol_g).max()
    print(f"{what} {dtype} {x.shape}: cost error {fc:.4f} of its bound, gradient error {fg:.4f}")
    assert fc <= 1.0 and fg <= 1.0, (what, fc, fg)
    for b in range(x.shape[0]):                                # exactly zero in the padding
        mask = np.ones(x.shape[1:3], dtype=bool)
        mask[:int(ll[b]), :int(tl[b]) + 1] = False
        assert np.all(grad[b][mask] == 0.0), what


@functools.lru_cache(maxsize=None)
def case(name, dtype):
    """(x as the dtype holds it, targets, logit_lengths, target_lengths, oracle costs, oracle gradients): built once per name."""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "tiny":
        logits, targets, ll, tl = O.inputs(rng, 3, 4, 4, 5, lengths=([4, 3, 1], [3, 1, 0]))
    elif name == "ragged37":
        logits, targets, ll, tl = O.inputs(rng, 4, 17, 10, 37)
    elif name == "v261":
        logits, targets, ll, tl = O.inputs(rng, 2, 33, 21, 261)
    elif name == "v4099":
        logits, targets, ll, tl = O.inputs(rng, 2, 12, 7, 4099, lengths=([12, 9], [6, 4]))
        logits[0, :, 0, -1] = 40.0                             # the largest logit in the last element of the row
        logits[0, :, 1, 0] = 40.0                              # in the first
        logits[0, :, 2, 4098] = 40.0                           # at blank (= -1)
        for t in range(12):
            logits[1, t, 0, targets[1, 0]] = 40.0              # at the target
        logits[1, :, 1, 2049] = 40.0                           # in the middle of a lane's vectors
    elif name == "thin":
        logits, targets, ll, tl = O.inputs(rng, 1, 300, 2, 3)
    elif name == "wide":
        logits, targets, ll, tl = O.inputs(rng, 1, 3, LAT_THREADS + 1, 3)
    else:
        raise KeyError(name)
    x = rounded(logits, dtype)
    oracle = O.brute_force if name == "tiny" else O.closed_form
    return (x, targets, ll, tl) + tuple(oracle(x, targets, ll, tl))


def test_tiles_are_the_exported_constants():
    assert F.rnnt_tiles() == (WIDTHS, LAT_THREADS, MAX_U1)


@pytest.mark.parametrize("dtype", DTYPES)
def test_tiny_lattices_against_every_alignment(dtype):
    x, targets, ll, tl, want_c, want_g = case("tiny", dtype)
    judge("tiny", dtype, x, ll, tl, run(x, targets, ll, tl, dtype), (want_c, want_g))


@pytest.mark.parametrize("dtype", DTYPES)
def test_ragged_batch_with_rows_at_every_residue(dtype):
    x, targets, ll, tl, want_c, want_g = case("ragged37", dtype)
    judge("ragged37", dtype, x, ll, tl, run(x, targets, ll, tl, dtype), (want_c, want_g))
    # the tensor itself off the 16-byte grid
    judge("ragged37+1", dtype, x, ll, tl, run(x, targets, ll, tl, dtype, offset=1), (want_c, want_g))


@pytest.mark.parametrize("name,dtype", [("v261", torch.float32), ("v261", torch.bfloat16), ("v4099", torch.float32),
                                        ("v4099", torch.float16), ("v4099", torch.float64), ("thin", torch.float32),
                                        ("wide", torch.float32), ("wide", torch.float64)])
def test_shapes(name, dtype):
    x, targets, ll, tl, want_c, want_g = case(name, dtype)
    judge(name, dtype, x, ll, tl, run(x, targets, ll, tl, dtype), (want_c, want_g))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_vocabularies_round_the_team_widths(dtype):
    vec = 16 // torch.empty((), dtype=dtype).element_size()
    seen = set()
    for w in WIDTHS:
        for V in (w - 1, w, w + 1, w * vec - 1, w * vec, w * vec + 1):
            if V in seen:
                continue
            seen.add(V)
            assert F.rnnt_team_width(dtype, V) in WIDTHS
            rng = np.random.default_rng(V)
            logits, targets, ll, tl = O.inputs(rng, 2, 3, 2, V)
            x = rounded(logits, dtype)
            judge(f"V={V}", dtype, x, ll, tl, run(x, targets, ll, tl, dtype), O.closed_form(x, targets, ll, tl))
    assert {F.rnnt_team_width(dtype, w * vec) for w in WIDTHS} == set(WIDTHS)         # every team width was launched


def test_poisoned_padding_changes_nothing():
    x, targets, ll, tl, want_c, want_g = case("ragged37", torch.float32)
    clean = run(x, targets, ll, tl, torch.float32)
    bad_x, bad_t = x.copy(), targets.copy()
    for b in range(x.shape[0]):
        fill = (np.nan, np.inf, -np.inf, np.nan)[b]
        bad_x[b, ll[b]:] = fill
        bad_x[b, :, tl[b] + 1:] = fill
        bad_t[b, tl[b]:] = (-7, 37, 2 ** 30, -2 ** 31)[b]
    assert not np.isfinite(bad_x).all() and not np.array_equal(bad_t, targets)
    dirty = run(bad_x, bad_t, ll, tl, torch.float32)
    assert np.array_equal(clean[0], dirty[0]) and np.array_equal(clean[1], dirty[1])
    judge("poisoned", torch.float32, x, ll, tl, dirty, (want_c, want_g))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_blank_clamp_and_cotangent(dtype):
    rng = np.random.default_rng(5)
    for blank in (-1, 0, 4):
        logits, targets, ll, tl = O.inputs(rng, 3, 7, 5, 11, blank=blank)
        x = rounded(logits, dtype)
        judge(f"blank={blank}", dtype, x, ll, tl, run(x, targets, ll, tl, dtype, blank=blank),
              O.closed_form(x, targets, ll, tl, blank))
    gc = [0.5, -2.0, 3.0]
    plain = O.closed_form(x, targets, ll, tl, 4)[1]
    assert all(np.abs(plain[b]).max() > 0.1 for b in range(3))                      # the clamp bites in every example
    want = O.closed_form(x, targets, ll, tl, 4, 0.1, True, gc)
    got = run(x, targets, ll, tl, dtype, blank=4, clamp=0.1, grad_costs=gc)
    judge("clamp", dtype, x, ll, tl, got, want, gc)
    for b in range(3):
        assert np.abs(got[1][b]).max() == pytest.approx(0.1 * abs(gc[b]), rel=1e-6)


@pytest.mark.parametrize("dtype", DTYPES)
def test_not_fused_on_log_probabilities(dtype):
    rng = np.random.default_rng(6)
    logits, targets, ll, tl = O.inputs(rng, 3, 9, 6, 41)
    x = rounded(O._log_softmax(logits), dtype)
    want = O.closed_form(x, targets, ll, tl, -1, -1.0, False)
    got = run(x, targets, ll, tl, dtype, fused=False)
    judge("not fused", dtype, x, ll, tl, got, want)
    assert np.count_nonzero(got[1]) <= 2 * 3 * 9 * 6           # two entries per live cell at most


def test_reductions_and_module():
    x, targets, ll, tl, want_c, want_g = case("tiny", torch.float32)
    xt, tg, llt, tlt = device_args(x, targets, ll, tl, torch.float32)
    none = F.rnnt_loss(xt, tg, llt, tlt, reduction="none")
    assert torch.equal(F.rnnt_loss(xt, tg, llt, tlt), none.mean()) and torch.equal(T.RNNTLoss()(xt, tg, llt, tlt), none.mean())
    assert torch.equal(F.rnnt_loss(xt, tg, llt, tlt, reduction="sum"), none.sum())
    assert torch.equal(T.RNNTLoss(reduction="none")(xt, tg, llt, tlt), none)
    for red, scale in (("mean", 1.0 / 3), ("sum", 1.0)):
        xg = xt.clone().requires_grad_(True)
        T.RNNTLoss(reduction=red)(xg, tg, llt, tlt).backward()
        judge(red, torch.float32, x, ll, tl, (none.double().cpu().numpy(), xg.grad.double().cpu().numpy()),
              (want_c, want_g * scale), [scale] * 3)
    scripted = torch.jit.script(T.RNNTLoss(reduction="none"))
    assert torch.equal(scripted(xt, tg, llt, tlt), none)
    xg = xt.clone().requires_grad_(True)
    scripted(xg, tg, llt, tlt).sum().backward()                # a scripted call is differentiable as the eager one is
    xe = xt.clone().requires_grad_(True)
    F.rnnt_loss(xe, tg, llt, tlt, reduction="sum").backward()
    assert torch.equal(xg.grad, xe.grad)


def test_gradcheck_and_no_second_derivative():
    rng = np.random.default_rng(7)
    logits, targets, ll, tl = O.inputs(rng, 2, 4, 3, 5, lengths=([4, 3], [2, 1]), scale=1.0)
    xt, tg, llt, tlt = device_args(logits, targets, ll, tl, torch.float64)
    xt.requires_grad_(True)
    for fused in (True, False):
        fn = lambda z: F.rnnt_loss(z, tg, llt, tlt, -1, -1.0, "none", fused)            # noqa: E731
        assert torch.autograd.gradcheck(fn, (xt,), eps=1e-6, atol=1e-7, rtol=1e-6)
    with pytest.raises(RuntimeError):
        torch.autograd.gradgradcheck(lambda z: F.rnnt_loss(z, tg, llt, tlt, -1, -1.0, "none", True), (xt,))


def test_two_calls_give_the_same_bits_on_both_routes():
    x, targets, ll, tl, _, _ = case("ragged37", torch.float32)
    a, b = run(x, targets, ll, tl, torch.float32), run(x, targets, ll, tl, torch.float32)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    try:
        F._force_route("ctypes")
        c = run(x, targets, ll, tl, torch.float32)
    finally:
        F._force_route(None)
    assert np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1])


def test_forward_without_grad_keeps_nothing():
    x, targets, ll, tl, want_c, _ = case("tiny", torch.float32)
    xt, tg, llt, tlt = device_args(x, targets, ll, tl, torch.float32)
    out = F.rnnt_loss(xt.requires_grad_(True).detach(), tg, llt, tlt, reduction="none")
    assert not out.requires_grad and out.grad_fn is None
    with torch.no_grad():
        out2 = F.rnnt_loss(xt, tg, llt, tlt, reduction="none")
    assert out2.grad_fn is None and torch.equal(out, out2)


def test_graph_capture_of_forward_and_backward():
    """Lengths and targets are read on the device: one capture serves new values in the same buffers."""
    x0, targets0, ll0, tl0, _, _ = case("ragged37", torch.float32)
    rng = np.random.default_rng(9)
    logits1, targets1, ll1, tl1 = O.inputs(rng, 4, 17, 10, 37)
    x1 = rounded(logits1, torch.float32)
    assert not np.array_equal(ll0, ll1) or not np.array_equal(tl0, tl1)
    xt, tg, llt, tlt = device_args(x0, targets0, ll0, tl0, torch.float32)
    xt.requires_grad_(True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                 # warm up off the default stream, as captures ask
        for _ in range(2):
            F.rnnt_loss(xt, tg, llt, tlt, reduction="sum").backward()
            xt.grad = None
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                              # one stream, no parallel branches
        costs = F.rnnt_loss(xt, tg, llt, tlt, reduction="none")
        costs.sum().backward()
    new = device_args(x1, targets1, ll1, tl1, torch.float32)
    with torch.no_grad():
        for dst, src in zip((xt, tg, llt, tlt), new):
            dst.copy_(src)
    graph.replay()
    torch.cuda.synchronize()
    got = (costs.detach().double().cpu().numpy(), xt.grad.double().cpu().numpy())
    judge("replayed", torch.float32, x1, ll1, tl1, got, O.closed_form(x1, targets1, ll1, tl1))
    eager = run(x1, targets1, ll1, tl1, torch.float32)
    assert np.array_equal(got[0], eager[0]) and np.array_equal(got[1], eager[1])


def test_torch_compile_runs_the_op():
    x, targets, ll, tl, _, _ = case("tiny", torch.float32)
    xt, tg, llt, tlt = device_args(x, targets, ll, tl, torch.float32)
    mod = T.RNNTLoss(reduction="none")
    assert torch.equal(torch.compile(mod, fullgraph=True, backend="eager")(xt, tg, llt, tlt), mod(xt, tg, llt, tlt))
