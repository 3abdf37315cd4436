"""F.ctc_loss / T.CTCLoss on the device against torch.nn.functional.ctc_loss on the CPU in float64 (of torch.log_softmax of the
widened inputs when fused).  Every bar is 4 x the reference's own error -- torch's float32 CPU path, or the float64 result's
rounding to a half type -- taken as the maximum over the whole case list."""
import functools

import pytest
import torch

import audio_amd.functional as F
import audio_amd.transforms as T

pytestmark = pytest.mark.gpu
DEV = "cuda"
CONFIGS, PF = F.ctc_loss_tiles()[:2]
EDGES = [s for top, _, _ in CONFIGS[:-1] for s in (top, top + 1)]           # one below and one above every boundary


def labels(n, V, blank, seed):
    g = torch.Generator().manual_seed(seed)
    return [int(v) + (int(v) >= blank) for v in torch.randint(0, V - 1, (n,), generator=g)]


def need(t):
    return len(t) + sum(a == b for a, b in zip(t, t[1:]))


# name -> (T, V, blank, targets, input_lengths): every example feasible
CASES = {"small": (PF + 5, 5, 0, [[], [1], [1, 1, 2, 2, 1], [3, 3, 3, 3], [], [2, 4]], [PF + 5, PF + 1, 7, 7, 0, 2])}
for V_ in (2, 29, 32, 1027):
    for bl in (0, V_ - 1):
        tg = [labels(n, V_, bl, 10 * V_ + n) for n in (3, 0, 6)]
        CASES[f"V{V_}-blank{bl}"] = (17, V_, bl, tg, [17, 5, need(tg[2])])
for S_ in EDGES:
    tg = [labels(S_, 5, 0, S_), labels(S_ - 3, 5, 0, S_ + 1)]
    CASES[f"S{S_}"] = (max(need(tg[0]), need(tg[1]) + 2) + 2, 5, 0, tg, [need(tg[0]), need(tg[1]) + 2])
W = [1.0, -0.5, 2.0, 0.25, 3.0, 1.5]


@functools.lru_cache(None)
def inputs(name, dtype=torch.float32):
    """Logits (T, N, V) from a seeded normal of scale 2, rounded to `dtype`, as float64 on the CPU."""
    T_, V, _, tg, _ = CASES[name]
    g = torch.Generator().manual_seed(len(name) + T_)
    return (2 * torch.randn(T_, len(tg), V, generator=g, dtype=torch.float64)).to(dtype).double()


@functools.lru_cache(None)
def reference(name, fused=True, dtype=torch.float32, compute=torch.float64):
    """(losses (N,), gradient of sum(W * losses)) of torch's CPU ctc_loss in `compute`, returned as float64."""
    T_, V, blank, tg, il = CASES[name]
    x = inputs(name, dtype).to(compute).clone().requires_grad_()
    S = max(map(len, tg))
    padded = torch.tensor([t + [(blank + 1) % V] * (S - len(t)) for t in tg], dtype=torch.long).reshape(len(tg), S)
    loss = torch.nn.functional.ctc_loss(x.log_softmax(-1) if fused else x, padded, torch.tensor(il),
                                        torch.tensor([len(t) for t in tg]), blank, "none")
    assert loss.isfinite().all()
    (loss * torch.tensor(W[:len(tg)], dtype=compute)).sum().backward()
    return loss.detach().double(), x.grad.double()


def device(name, dtype=torch.float32, fused=True, concat=False, ints=torch.int64, lens=torch.int64, view=False, **kw):
    """(losses, gradient of sum(W * losses)) of F.ctc_loss, reduction "none"."""
    T_, V, blank, tg, il = CASES[name]
    x = inputs(name, dtype).to(dtype).to(DEV)
    x = (x.transpose(0, 1).contiguous().transpose(0, 1) if view else x).requires_grad_()
    S = max(map(len, tg))
    flat = [t + ([] if concat else [V] * (S - len(t))) for t in tg]                        # padding is never read
    targets = torch.tensor(sum(flat, []) if concat else flat, dtype=ints, device=DEV).reshape(-1 if concat else (len(tg), S))
    loss = T.CTCLoss(blank, "none", fused_log_softmax=fused, **kw)(x, targets, torch.tensor(il, dtype=lens, device=DEV),
                                                                  torch.tensor([len(t) for t in tg], dtype=lens, device=DEV))
    (loss * torch.tensor(W[:len(tg)], device=DEV, dtype=loss.dtype)).sum().backward()
    assert loss.dtype == dtype and x.grad.dtype == dtype
    pad = torch.arange(T_)[:, None] >= torch.tensor(il)                                   # padding rows are exactly zero
    assert not x.grad.cpu()[pad].any()
    return loss.detach().cpu(), x.grad.cpu()


def distance(got, want):
    """(largest loss error, largest gradient error of an example over the example's largest gradient element)."""
    top = want[1].abs().amax((0, 2)).clamp_min(1e-300)
    assert got[0].isfinite().all() and got[1].isfinite().all()
    return float((got[0].double() - want[0]).abs().max()), float(((got[1].double() - want[1]).abs().amax((0, 2)) / top).max())


@functools.lru_cache(None)
def bars(fused=True):
    d = [distance(reference(n, fused, compute=torch.float32), reference(n, fused)) for n in CASES]
    return 4 * max(a for a, _ in d), 4 * max(b for _, b in d)


@pytest.mark.parametrize("name", list(CASES))
def test_float32_against_float64_cpu(name):
    """A second call, and concatenated int32 targets with int32 lengths, give the same bits.  The transposed view is read in
    place: its rows start at other residues of 16 bytes, so the row sums take another order and it is held to the bar."""
    got = device(name)
    worst, bar = [distance(g, reference(name)) for g in (got, device(name, view=True))], bars()
    print(f"{name}: loss worst {worst[0][0]:.3e}, bar {bar[0]:.3e}; gradient worst {worst[0][1]:.3e}, bar {bar[1]:.3e}")
    assert all(w[0] <= bar[0] and w[1] <= bar[1] for w in worst)
    for other in (device(name, concat=True, ints=torch.int32, lens=torch.int32), device(name)):
        assert torch.equal(other[0], got[0]) and torch.equal(other[1], got[1])


@pytest.mark.parametrize("dtype", [torch.float64, torch.float16, torch.bfloat16], ids=["f64", "f16", "bf16"])
def test_other_dtypes_on_the_ragged_case(dtype):
    """float64 stays under float32's bar; a half type gets 4 x the reference's own rounding to the type."""
    want = reference("small", dtype=dtype)
    worst, bar = distance(device("small", dtype), want), bars()
    if dtype != torch.float64:
        bar = tuple(4 * v for v in distance((want[0].to(dtype), want[1].to(dtype)), want))
    print(f"{dtype}: loss worst {worst[0]:.3e}, bar {bar[0]:.3e}; gradient worst {worst[1]:.3e}, bar {bar[1]:.3e}")
    assert 0 < bar[0] and worst[0] <= bar[0] and worst[1] <= bar[1]


def test_log_probability_input():
    worst, bar = distance(device("small", fused=False), reference("small", fused=False)), bars(False)
    print(f"not fused: loss worst {worst[0]:.3e}, bar {bar[0]:.3e}; gradient worst {worst[1]:.3e}, bar {bar[1]:.3e}")
    assert worst[0] <= bar[0] and worst[1] <= bar[1]


@pytest.mark.parametrize("reduction", ["mean", "sum"])
def test_reductions_unbatched_and_tuple_lengths(reduction):
    T_, V, blank, tg, il = CASES["small"]
    want, x = reference("small")[0], inputs("small").float().to(DEV)
    sizes = torch.tensor([len(t) for t in tg], dtype=torch.double)
    ref = (want / sizes.clamp_min(1)).mean() if reduction == "mean" else want.sum()
    flat = torch.tensor(sum(tg, []), device=DEV)
    got = F.ctc_loss(x, flat, tuple(il), tuple(len(t) for t in tg), reduction=reduction)
    assert got.shape == () and abs(float(got) - float(ref)) <= bars()[0] * (1 if reduction == "mean" else len(tg))
    one = F.ctc_loss(x[:7, 2], torch.tensor(tg[2], device=DEV), torch.tensor(7, device=DEV), torch.tensor(5, device=DEV),
                     reduction="none")                                                    # (T, V): example 2 alone
    assert one.shape == () and abs(float(one) - float(want[2])) <= bars()[0]


def test_infeasible_flagged_graph_and_second_derivative():
    T_, V, blank, tg, il = CASES["small"]
    x = inputs("small").float().to(DEV)
    S = max(map(len, tg))
    targets = torch.tensor([t + [1] * (S - len(t)) for t in tg], device=DEV)
    tl = torch.tensor([len(t) for t in tg], device=DEV)
    base = F.ctc_loss(x, targets, torch.tensor(il, device=DEV), tl, reduction="none")
    short = torch.tensor([v - (i == 2) for i, v in enumerate(il)], device=DEV)            # one frame below example 2's minimum
    for zero in (False, True):
        xs = x.clone().requires_grad_()
        loss = F.ctc_loss(xs, targets, short, tl, reduction="none", zero_infinity=zero)
        loss.sum().backward()
        assert float(loss[2].detach()) == (0.0 if zero else float("inf")) and torch.equal(loss[[0, 1, 3, 4, 5]], base[[0, 1, 3, 4, 5]])
        assert not zero or (not xs.grad[:, 2].any() and xs.grad[:, 3].any())
    bad_t, bad_l = targets.clone(), torch.tensor(il, device=DEV)
    bad_t[2, 1], bad_l[3] = V, T_ + 1                                                     # a label and a length out of range
    xs = x.clone().requires_grad_()
    loss = F.ctc_loss(xs, bad_t, bad_l, tl, reduction="none")
    loss[[0, 1, 4, 5]].sum().backward()
    assert loss[[2, 3]].isnan().all() and torch.equal(loss[[0, 1, 4, 5]], base[[0, 1, 4, 5]])
    assert xs.grad[:, [2, 3]].isnan().all() and xs.grad[:, [0, 1, 4, 5]].isfinite().all()
    stat, lens = torch.zeros_like(x), torch.tensor(il, device=DEV)                        # captured: replays against eager calls
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = F.ctc_loss(stat, targets, lens, tl)
    for scale in (1.0, 0.5, 1.0):
        stat.copy_(x * scale)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, F.ctc_loss(x * scale, targets, lens, tl))
    with pytest.raises(RuntimeError):                                                     # once-differentiable
        xs = x.clone().requires_grad_()
        gr, = torch.autograd.grad(F.ctc_loss(xs, targets, lens, tl), xs, create_graph=True)
        gr.sum().backward()
