"""F.permutation_invariant_training, F.pit_metric_matrix, F.pit_assignment and F.pit_permutate on the device against
tests/pit_oracle.py.  Bars are 4 x the reference's own error on the same inputs, as in tests/test_gpu_sdr.py."""
import functools

import numpy as np
import pytest
import torch

import pit_oracle as PO
import audio_amd.functional as F
from test_gpu_sdr import DEV, dev, rel, same_bits

pytestmark = pytest.mark.gpu
FUSED = {"si_sdr": (F.scale_invariant_signal_distortion_ratio, {}), "si_sdr_zm": (F.scale_invariant_signal_distortion_ratio, dict(zero_mean=True)),
         "si_snr": ("scale_invariant_signal_noise_ratio", {}), "snr": (F.signal_noise_ratio, {}),
         "snr_zm": ("signal_noise_ratio", dict(zero_mean=True))}
TORCH = {torch.float32: np.float32, torch.float64: np.float64}


def autograd(name, p, t, w, eps):
    """Gradients of sum(w * metric) to p and t through the definition in torch, at the tensors' precision."""
    p, t = p.clone().requires_grad_(), t.clone().requires_grad_()
    pc, tc = (p - p.mean(-1, keepdim=True), t - t.mean(-1, keepdim=True)) if name.endswith("_zm") or name == "si_snr" else (p, t)
    if name.startswith("si"):
        tc = ((pc * tc).sum(-1, keepdim=True) + eps) / ((tc * tc).sum(-1, keepdim=True) + eps) * tc
    (10 * torch.log10(((tc * tc).sum(-1) + eps) / (((tc - pc) ** 2).sum(-1) + eps)) * w.to(p.dtype)).sum().backward()
    return p.grad, t.grad


def times():
    span = max(F.pit_tiles()[1:3])
    return [1, 3, span - 1, span + 1, 2 * span + 5]


def batch(S, time, n=3):
    """n mixtures as (preds, target, planted), float64 (n, S, time)."""
    return tuple(np.stack(x) for x in zip(*(PO.mixtures(S, time, seed) for seed in range(n))))


def ragged(time):
    return [time, (time + 1) // 2, 0]


@functools.lru_cache(None)
def matrix_refs(np_dtype, S):
    """{(name, time): (lower-precision form, higher-precision form)} of the definition, each (3, S, S), example b cut at
    ragged(time)[b]; and 4 x their largest distance."""
    lo, hi = (np.float32, np.float64) if np_dtype == np.float32 else (np.float64, np.longdouble)
    refs, d = {}, 0.0
    for name, (_, kw) in FUSED.items():
        for T in times():
            p, t, _ = (x.astype(np_dtype) if x.ndim == 3 else x for x in batch(S, T))
            forms = [np.stack([PO.matrix(p[b, :, :n], t[b, :, :n], name.replace("_zm", ""), kw.get("zero_mean", False), dt,
                                         np.finfo(np_dtype).eps) for b, n in enumerate(ragged(T))]) for dt in (lo, hi)]
            refs[name, T] = forms
            d = max(d, float(np.abs(forms[0] - forms[1]).max()))
    return refs, 4 * d


@pytest.mark.parametrize("S", [1, 2, 3, 8])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", list(FUSED))
def test_matrix_against_the_definition(name, dtype, S):
    (refs, bar), (fn, kw), worst = matrix_refs(TORCH[dtype], S), FUSED[name], 0.0
    for T in times():
        p, t, _ = batch(S, T)
        wide_p, wide_t = torch.full((3, S, T + 9), float("nan"), dtype=dtype, device=DEV), torch.zeros((3, S, 2 * T), dtype=dtype, device=DEV)
        wide_p[..., 3:T + 3], wide_t[..., 1:T + 1] = dev(p, dtype), dev(t, dtype)
        pv, tv, lens = wide_p[..., 3:T + 3], wide_t[..., 1:T + 1], torch.tensor(ragged(T), device=DEV, dtype=torch.int32)
        got = F.pit_metric_matrix(pv, tv, fn, lengths=lens, **kw)
        assert got.dtype == dtype and got.shape == (3, S, S)
        worst = max(worst, float(np.abs(got.double().cpu().numpy() - refs[name, T][1]).max()))
        rowwise = fn if callable(fn) else getattr(F, fn)                    # a row of length 0: what the row-wise function gives
        assert same_bits(got[2], rowwise(pv[2, :, :0], tv[2, :, :0], **kw)[:, None].expand(S, S).contiguous())
        if dtype == torch.float32:
            for half in (torch.float16, torch.bfloat16):                   # widened on load: the call on the widened tensor
                ph, th = pv.to(half), tv.to(half)
                assert same_bits(F.pit_metric_matrix(ph, th, fn, lengths=lens, **kw), F.pit_metric_matrix(ph.float(), th.float(), fn, lengths=lens, **kw))
    print(f"{name} {dtype} S={S}: worst {worst:.3e} dB, bar {bar:.3e} dB")
    assert worst <= bar


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("eval_func", ["max", "min"])
@pytest.mark.parametrize("S", [1, 2, 3, 5, 8])
def test_assignment_against_brute_force(S, eval_func, dtype):
    rng = np.random.default_rng(10 * S + (eval_func == "min"))
    M = np.concatenate([rng.standard_normal((5, S, S)) * 10, rng.integers(-2, 3, (4, S, S)).astype(np.float64)])   # the last four: many ties
    M = M.astype(TORCH[dtype]).astype(np.float64)
    M[4, S // 2, 0] = np.nan
    best, perm = F.pit_assignment(dev(M, dtype), eval_func)
    assert best.dtype == dtype and perm.dtype == torch.int64 and perm.shape == (9, S)
    for b in range(9):
        if b == 4:                                                          # a NaN entry: NaN and the identity, this example alone
            assert best[b].isnan() and perm[b].tolist() == list(range(S))
            continue
        want, want_perm = PO.assign(M[b], eval_func)
        assert perm[b].tolist() == want_perm.tolist(), (b, M[b])
        assert best[b].item() == TORCH[dtype](want)                         # the right-nested total / S, rounded once to the output type


@pytest.mark.parametrize("S", [2, 3, 8])
def test_end_to_end_recovers_the_planted_permutation(S):
    T = F.pit_tiles()[1] + 1
    p, t, planted = batch(S, T)
    pd, td = dev(p), dev(t)
    for name, (fn, kw) in FUSED.items():
        best, perm = F.permutation_invariant_training(pd, td, fn, **kw)
        assert perm.cpu().numpy().tolist() == planted.tolist(), name
        M = F.pit_metric_matrix(pd, td, fn, **kw).double().cpu().numpy()
        assert best.tolist() == [np.float32(PO.total(M[b], planted[b]) / S) for b in range(3)]
        worst, _ = F.permutation_invariant_training(pd, td, fn, eval_func="min", **kw)
        assert (worst < best).all()
    lined = F.pit_permutate(td, perm)                                       # the references in the estimates' order
    assert torch.equal(lined, td[torch.arange(3, device=DEV)[:, None], perm])
    assert torch.equal(F.pit_permutate(pd[..., 1:], perm), pd[..., 1:][torch.arange(3, device=DEV)[:, None], perm])      # strided rows
    off = perm.clone().int()
    off[1, 0], off[2, S - 1] = S, -1
    got = F.pit_permutate(td[..., 1:T - 2].half(), off)                     # unaligned rows, an index out of range on either side
    want = td[..., 1:T - 2].half()[torch.arange(3, device=DEV)[:, None], off.long().clamp(0, S - 1)]
    assert got[1, 0].isnan().all() and got[2, S - 1].isnan().all()
    keep = torch.ones(3, S, dtype=torch.bool, device=DEV)
    keep[1, 0] = keep[2, S - 1] = False
    assert torch.equal(got[keep], want[keep])
    gbest, gperm = F.permutation_invariant_training(pd, td, lambda a, b: F.signal_noise_ratio(a, b))       # the generic route
    fbest, fperm = F.permutation_invariant_training(pd, td, F.signal_noise_ratio)
    assert torch.equal(gperm, fperm) and float((gbest - fbest).abs().max()) <= matrix_refs(np.float32, S)[1]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("S", [2, 3])
def test_gradient_against_float64_autograd(S, dtype):
    """The reference is float64 autograd through the definition on the targets gathered by the planted permutation (which the
    oracle's assignment equals, tests/test_pit.py).  The bar, of each row's largest element, is 4 x float32 autograd's own
    distance from float64 autograd (both with float32's eps), for either input dtype; float64 input is scored against the
    reference with float64's eps.  On an MI355X float64 input stays within 5.5e-15 of it, float64 autograd on the time-reversed
    rows within 9e-16."""
    T = F.pit_tiles()[1] + 1
    p, t, planted = batch(S, T)
    pd, td, idx = dev(p), dev(t), torch.arange(3, device=DEV)[:, None]
    w, inv, worst, bar = -torch.ones(3, S, device=DEV, dtype=torch.float64) / S, dev(np.argsort(planted, axis=1), torch.int64), 0.0, 0.0
    eps32, eps = float(np.finfo(np.float32).eps), float(np.finfo(TORCH[dtype]).eps)
    for name, (fn, kw) in FUSED.items():
        gathered = td[idx, dev(planted, torch.int64)]
        ref32 = autograd(name, pd.double(), gathered.double(), w, eps32)
        bar = max(bar, 4 * max(rel(g, r) for g, r in zip(autograd(name, pd, gathered, w, eps32), ref32)))
        gp64, gl64 = ref32 if dtype == torch.float32 else autograd(name, pd.double(), gathered.double(), w, eps)
        ref = (gp64, gl64[idx, inv])                                        # back to the references' own order
        pg, tg = pd.to(dtype).clone().requires_grad_(), td.to(dtype).clone().requires_grad_()
        best, perm = F.permutation_invariant_training(pg, tg, fn, **kw)
        assert not perm.requires_grad
        (-best.sum()).backward()
        worst = max(worst, rel(pg.grad, ref[0]), rel(tg.grad, ref[1]))
    print(f"S={S} {dtype} gradients (of the row's largest element): worst {worst:.3e}, bar {bar:.3e}")
    assert worst <= bar
    pl, tl = pd.clone().requires_grad_(), td.clone().requires_grad_()
    F.permutation_invariant_training(pl, tl, "scale_invariant_signal_noise_ratio", lengths=torch.tensor([T, T - 7, 0], device=DEV))[0].sum().backward()
    assert not pl.grad[1, :, T - 7:].any() and not tl.grad[1, :, T - 7:].any() and not pl.grad[2].any() and not tl.grad[2].any()
    assert pl.grad[1, :, :T - 7].all() and tl.grad[0].all()
    with pytest.raises(RuntimeError):                                       # once-differentiable
        pp = pd.clone().requires_grad_()
        g, = torch.autograd.grad(F.permutation_invariant_training(pp, td, fn)[0].sum(), pp, create_graph=True)
        g.sum().backward()


@pytest.mark.parametrize("half", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_gradient_of_the_half_types(half):
    """float16 / bfloat16 gradients come back in the input's type, rounded once.  The reference is float64 autograd on the
    widened inputs (float32's eps: the half types compute as float32 does); the bar is 4 x the distance of that reference from
    its own rounding to the type -- the margin float32 gets over float32 autograd."""
    S, T = 2, F.pit_tiles()[1] + 1
    p, t, planted = batch(S, T)
    ph, th, idx = dev(p).to(half), dev(t).to(half), torch.arange(3, device=DEV)[:, None]
    w, inv = -torch.ones(3, S, device=DEV, dtype=torch.float64) / S, dev(np.argsort(planted, axis=1), torch.int64)
    for name, (fn, kw) in FUSED.items():
        gp64, gl64 = autograd(name, ph.double(), th[idx, dev(planted, torch.int64)].double(), w, float(np.finfo(np.float32).eps))
        refs = (gp64, gl64[idx, inv])                                       # back to the references' own order
        own = max(rel(r.to(half), r) for r in refs)
        pg, tg = ph.clone().requires_grad_(), th.clone().requires_grad_()
        best, perm = F.permutation_invariant_training(pg, tg, fn, **kw)
        assert perm.cpu().numpy().tolist() == planted.tolist(), name
        (-best.sum()).backward()
        assert pg.grad.dtype == half and tg.grad.dtype == half
        worst = max(rel(pg.grad, refs[0]), rel(tg.grad, refs[1]))
        print(f"{name} {half} gradients: worst {worst:.3e}, the reference's own rounding {own:.3e}, bar {4 * own:.3e}")
        assert 0 < own and worst <= 4 * own


@pytest.mark.parametrize("name", ["si_sdr", "si_snr", "snr_zm"])
def test_bit_for_bit(name):
    (fn, kw), S, span = FUSED[name], 3, F.pit_tiles()[1]
    pit = lambda p, t, **k: F.permutation_invariant_training(p, t, fn, **kw, **k)
    pg, tg = (dev(x) for x in batch(S, span + 69)[:2])                      # a FIRST call captured: no other call uses this length
    sp, st = torch.zeros_like(pg), torch.zeros_like(tg)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = pit(sp, st)
    for scale in (1.0, 0.5, 1.0):
        sp.copy_(pg * scale)
        st.copy_(tg)
        g.replay()
        torch.cuda.synchronize()
        assert all(same_bits(a, b) for a, b in zip(out, pit(pg * scale, tg)))
    T = span + 1
    p, t = (dev(x) for x in batch(S, T)[:2])
    whole = pit(p, t)
    assert all(same_bits(a, b) for a, b in zip(whole, pit(p, t)))           # two calls
    lens = [T, span // 2 + 3, 70]
    cut = pit(p, t, lengths=torch.tensor(lens, device=DEV))
    for b in range(3):
        assert all(same_bits(a[b:b + 1], c) for a, c in zip(whole, pit(p[b:b + 1], t[b:b + 1])))                      # a batch against its examples
        assert all(same_bits(a[b:b + 1], c) for a, c in zip(cut, pit(p[b:b + 1, :, :lens[b]], t[b:b + 1, :, :lens[b]])))   # lengths[b] against the slice
    bad = p.clone()
    bad[1, 2, 77] = float("nan")
    got = pit(bad, t, lengths=torch.tensor([T, T, T + 1], device=DEV))      # a NaN sample, an impossible length
    assert same_bits(got[0][0], whole[0][0]) and got[0][1:].isnan().all() and got[1][1:].tolist() == [list(range(S))] * 2
