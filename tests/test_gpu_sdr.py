"""F.signal_distortion_ratio, F.scale_invariant_signal_distortion_ratio, F.scale_invariant_signal_noise_ratio and
F.signal_noise_ratio on the device against tests/sdr_oracle.py.  Every bar is 4 x the reference's own error, taken as the maximum
over the whole case list so that a case where two forms of the reference happen to coincide cannot make it vanish."""
import functools

import numpy as np
import pytest
import torch

import sdr_oracle as O
import audio_amd.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
FILTER_LENGTHS = [1, 7, 16, 17, 64, 65, 511, 512]
SDR_OPTS = [{}] * len(FILTER_LENGTHS) + [dict(zero_mean=True), dict(load_diag=1e-3), dict(use_cg_iter=10),
                                          dict(zero_mean=True, load_diag=0.5)]
SDR_CASES = list(zip(FILTER_LENGTHS + [17, 17, 17, 65], SDR_OPTS))
SI_FNS = {"si_sdr": (lambda p, t, **k: F.scale_invariant_signal_distortion_ratio(p, t, **k), lambda p, t, **k: O.si_sdr(p, t, False, **k)),
          "si_sdr_zm": (lambda p, t, **k: F.scale_invariant_signal_distortion_ratio(p, t, True, **k), lambda p, t, **k: O.si_sdr(p, t, True, **k)),
          "si_snr": (lambda p, t, **k: F.scale_invariant_signal_noise_ratio(p, t, **k), O.si_snr),
          "snr": (lambda p, t, **k: F.signal_noise_ratio(p, t, **k), lambda p, t, **k: O.snr(p, t, False, **k)),
          "snr_zm": (lambda p, t, **k: F.signal_noise_ratio(p, t, True, **k), lambda p, t, **k: O.snr(p, t, True, **k))}


def dev(x, dtype=torch.float32):
    return torch.as_tensor(np.asarray(x), dtype=dtype).to(DEV)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32 if a.element_size() == 4 else torch.int64),
                                                                     b.view(torch.int32 if b.element_size() == 4 else torch.int64))


signals = functools.lru_cache(None)(O.signals)


def sdr_times(fl):
    stage, span = F.sdr_tiles()[2:4]
    return sorted({1, fl - 1, fl + 1, stage - 1, stage + 1, span - 1, span, span + 1, 2 * span + 17})


@functools.lru_cache(None)
def sdr_refs(i):
    """{time: (float64 form, longdouble form)} of case i, each (3,), on float32-representable inputs."""
    fl, opts = SDR_CASES[i]
    kw = {k: v for k, v in opts.items() if k != "use_cg_iter"}
    out = {}
    for T in sdr_times(fl):
        p, t = (x.astype(np.float32) for x in signals(T))
        out[T] = (np.array([O.sdr_float64(p[r], t[r], fl, **kw) for r in range(3)]),
                  np.array([O.sdr_longdouble(p[r], t[r], fl, **kw) for r in range(3)]))
    return out


@functools.lru_cache(None)
def sdr_bar():
    d = [np.abs(a - b)[np.isfinite(a) & np.isfinite(b)] for i in range(len(SDR_CASES)) for a, b in sdr_refs(i).values()]
    return 4 * float(np.concatenate(d).max())


@pytest.mark.parametrize("case", range(len(SDR_CASES)), ids=[f"L{fl}-{'-'.join(o) or 'default'}" for fl, o in SDR_CASES])
def test_sdr_against_the_longdouble_oracle(case):
    """Finite scores within the bar; where the longdouble form is not finite (time 1: coh = 1 exactly; time 0: a singular
    system) the kernel gives the same value.  The float64 FFT form may differ there, so such rows do not enter the bar."""
    fl, opts = SDR_CASES[case]
    bar, worst = sdr_bar(), 0.0
    for T, (_, want) in sdr_refs(case).items():
        p, t = signals(T)
        got = F.signal_distortion_ratio(dev(p), dev(t), filter_length=fl, **opts)
        # the same float32-representable samples as float64 tensors: the float64 result shows the kernels' own distance
        got64 = F.signal_distortion_ratio(dev(p).double(), dev(t).double(), filter_length=fl, **opts).cpu().numpy()
        assert got.dtype == torch.float32 and got64.dtype == np.float64
        fin = np.isfinite(want)
        for g in (got.double().cpu().numpy(), got64):
            assert np.array_equal(g[~fin], want[~fin].astype(np.float64), equal_nan=True), (T, g, want)
        if fin.any():
            worst = max(worst, float(np.abs(got64[fin] - want[fin]).max()))
            half_ulp = np.spacing(np.abs(got.cpu().numpy()[fin])).astype(np.float64) / 2      # the float32 result's one rounding
            assert (np.abs(got.double().cpu().numpy()[fin] - want[fin]) <= half_ulp + bar).all(), T
    print(f"sdr case {SDR_CASES[case]}: worst {worst:.3e} dB, bar {bar:.3e} dB")
    assert worst <= bar


@pytest.mark.parametrize("half", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_sdr_half_types_equal_the_call_on_the_widened_tensor(half):
    """float16 / bfloat16 are widened on load and every sum is float64: the bits of the float32 call on the widened tensor, one
    sample past a span, at a filter length of either class of the correlation kernel."""
    p, t = signals(F.sdr_tiles()[3] + 1)
    ph, th = dev(p).to(half), dev(t).to(half)
    for fl in (17, 65):
        got = F.signal_distortion_ratio(ph, th, filter_length=fl)
        assert got.isfinite().all() and same_bits(got, F.signal_distortion_ratio(ph.float(), th.float(), filter_length=fl))


def si_times():
    chunk = F.sdr_tiles()[1]
    return [1, 3, chunk - 1, chunk + 1, 3 * chunk + 5]


@functools.lru_cache(None)
def si_bar(np_dtype):
    """4 x the largest distance over every function, time and row: float32 definition from float64's, or float64's from
    longdouble's."""
    lo, hi = (np.float32, np.float64) if np_dtype == np.float32 else (np.float64, np.longdouble)
    eps, d = np.finfo(np_dtype).eps, 0.0
    for _, ref in SI_FNS.values():
        for T in si_times():
            p, t = (x.astype(np_dtype) for x in signals(T))
            d = max(d, max(abs(ref(p[r], t[r], dtype=lo, eps=eps) - ref(p[r], t[r], dtype=hi, eps=eps)) for r in range(3)))
    return 4 * d


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", list(SI_FNS))
def test_si_family_against_the_definition(name, dtype):
    fn, ref = SI_FNS[name]
    np_dtype = np.float32 if dtype == torch.float32 else np.float64
    hi, eps, bar, worst = (np.float64 if dtype == torch.float32 else np.longdouble), np.finfo(np_dtype).eps, si_bar(np_dtype), 0.0
    for T in si_times():
        p, t = (x.astype(np_dtype) for x in signals(T))
        want = np.array([ref(p[r], t[r], dtype=hi, eps=eps) for r in range(3)], np.float64)
        got = fn(dev(p, dtype), dev(t, dtype))
        assert got.dtype == dtype and got.shape == (3,)
        worst = max(worst, float(np.abs(got.double().cpu().numpy() - want).max()))
        if dtype == torch.float32:
            for half in (torch.float16, torch.bfloat16):                   # widened on load: the call on the widened tensor
                ph, th = dev(p).to(half), dev(t).to(half)
                assert same_bits(fn(ph, th), fn(ph.float(), th.float()))
    print(f"{name} {dtype}: worst {worst:.3e} dB, bar {bar:.3e} dB")
    assert worst <= bar


def torch_expr(name, p, t, eps=torch.finfo(torch.float32).eps):
    if name.endswith("_zm") or name == "si_snr":
        p, t = p - p.mean(-1, keepdim=True), t - t.mean(-1, keepdim=True)
    if name.startswith("si"):
        t = ((p * t).sum(-1, keepdim=True) + eps) / ((t * t).sum(-1, keepdim=True) + eps) * t
    return 10 * torch.log10(((t * t).sum(-1) + eps) / (((t - p) ** 2).sum(-1) + eps))


def autograd(name, p, t, w, eps=torch.finfo(torch.float32).eps):
    p, t = p.clone().requires_grad_(), t.clone().requires_grad_()
    (torch_expr(name, p, t, eps) * w.to(p.dtype)).sum().backward()
    return p.grad, t.grad


def rel(g, g64):
    """The largest error of a row over the row's largest element; a row whose gradient is exactly zero (one zero-mean sample)
    has no scale and only has to be finite."""
    top = g64.abs().amax(-1)
    assert g.isfinite().all()
    return float(torch.where(top > 0, (g.double() - g64).abs().amax(-1) / top.clamp_min(1e-300), 0.0).max())


@functools.lru_cache(None)
def grad_refs():
    """{(name, time): float64 autograd gradients of float32-representable inputs}, and 4 x float32 autograd's largest distance,
    kept apart for time 1 and for the rest: at one sample SI-SDR's gradient to target is the difference of terms 1e7 times its
    size, float64 autograd is noise there, and one bar over the whole list (hundreds) would check nothing at the other times."""
    refs, d, w = {}, {True: 0.0, False: 0.0}, dev([1.0, -0.5, 2.0])
    for name in SI_FNS:
        for T in si_times():
            p, t = (dev(x) for x in signals(T))
            refs[name, T] = autograd(name, p.double(), t.double(), w)
            d[T == 1] = max(d[T == 1], max(rel(g, g64) for g, g64 in zip(autograd(name, p, t, w), refs[name, T])))
    return refs, {k: 4 * v for k, v in d.items()}


@pytest.mark.parametrize("name", list(SI_FNS))
def test_gradients_against_float64_autograd(name):
    (refs, bar), worst, w = grad_refs(), {True: 0.0, False: 0.0}, dev([1.0, -0.5, 2.0])
    for T in si_times():
        p, t = (dev(x).requires_grad_() for x in signals(T))
        out = SI_FNS[name][0](p, t)
        (out * w).sum().backward()
        worst[T == 1] = max(worst[T == 1], max(rel(g, g64) for g, g64 in zip((p.grad, t.grad), refs[name, T])))
    print(f"{name} gradients (of the row's largest element): time 1 worst {worst[True]:.3e}, bar {bar[True]:.3e}; "
          f"other times worst {worst[False]:.3e}, bar {bar[False]:.3e}")
    assert worst[True] <= bar[True] and worst[False] <= bar[False]
    lengths = torch.tensor([T, T - 7, 0], device=DEV)
    pl, tl = p.detach().clone().requires_grad_(), t.detach().clone().requires_grad_()
    SI_FNS[name][0](pl, tl, lengths=lengths).sum().backward()
    assert not pl.grad[1, T - 7:].any() and not tl.grad[1, T - 7:].any() and not pl.grad[2].any() and pl.grad[1, :T - 7].all()
    with pytest.raises(RuntimeError):                                       # once-differentiable
        pp = p.detach().clone().requires_grad_()
        g, = torch.autograd.grad(SI_FNS[name][0](pp, t.detach()).sum(), pp, create_graph=True)
        g.sum().backward()


@pytest.mark.parametrize("name", list(SI_FNS))
def test_gradients_of_float64_and_half_inputs(name):
    """One sample past a chunk.  float64 input: against float64 autograd with float64's eps, under float32's bar (the sums are
    float64 for every dtype).  float16 / bfloat16: the gradients come back in the input's type, rounded once; the reference is
    float64 autograd on the widened inputs, and the bar 4 x the distance of that reference from its own rounding to the type --
    the margin float32 gets over float32 autograd."""
    fn, w, T = SI_FNS[name][0], dev([1.0, -0.5, 2.0]), si_times()[3]

    def device_grads(p, t):
        p, t = p.clone().requires_grad_(), t.clone().requires_grad_()
        (fn(p, t) * w).sum().backward()
        assert p.grad.dtype == p.dtype and t.grad.dtype == t.dtype
        return p.grad, t.grad

    p, t = (dev(x).double() for x in signals(T))
    refs = autograd(name, p, t, w, eps=torch.finfo(torch.float64).eps)
    worst, bar = max(rel(g, g64) for g, g64 in zip(device_grads(p, t), refs)), grad_refs()[1][False]
    print(f"{name} float64 gradients (of the row's largest element): worst {worst:.3e}, bar {bar:.3e}")
    assert worst <= bar
    for half in (torch.float16, torch.bfloat16):
        ph, th = p.to(half), t.to(half)
        refs = autograd(name, ph.double(), th.double(), w)
        own = max(rel(g64.to(half), g64) for g64 in refs)
        worst = max(rel(g, g64) for g, g64 in zip(device_grads(ph, th), refs))
        print(f"{name} {half} gradients: worst {worst:.3e}, the reference's own rounding {own:.3e}, bar {4 * own:.3e}")
        assert 0 < own and worst <= 4 * own


BIT_FNS = {"sdr": lambda p, t, **k: F.signal_distortion_ratio(p, t, filter_length=65, zero_mean=True, **k),
           "sdr512": lambda p, t, **k: F.signal_distortion_ratio(p, t, **k),
           "si_sdr": SI_FNS["si_sdr"][0], "si_snr": SI_FNS["si_snr"][0], "snr": SI_FNS["snr"][0]}


@pytest.mark.parametrize("name", list(BIT_FNS))
def test_bit_for_bit(name):
    fn, T = BIT_FNS[name], F.sdr_tiles()[3] + 5
    # a FIRST call captured: this length is used by no other call of the file; replayed three times against eager calls
    Tg = T + 64
    pg, tg = (dev(x) for x in signals(Tg))
    sp, st = torch.zeros_like(pg), torch.zeros_like(tg)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = fn(sp, st)
    for scale in (1.0, 0.5, 1.0):
        sp.copy_(pg * scale)
        st.copy_(tg)
        g.replay()
        torch.cuda.synchronize()
        assert same_bits(out, fn(pg * scale, tg))
    p, t = (dev(x) for x in signals(T))
    whole = fn(p, t)
    assert same_bits(whole, fn(p, t))                                       # two calls
    for r in range(3):                                                      # a batch against its rows
        assert same_bits(whole[r], fn(p[r], t[r]))
    lens = [T, F.sdr_tiles()[2] + 3, 70]
    ragged = fn(p, t, lengths=torch.tensor(lens, device=DEV, dtype=torch.int32))
    for r in range(3):                                                      # lengths[b] against the slice
        assert same_bits(ragged[r], fn(p[r, :lens[r]], t[r, :lens[r]]))
    wide_p, wide_t = torch.full((3, T + 9), float("nan"), device=DEV), torch.zeros((3, 2 * T), device=DEV)
    wide_p[:, 3:T + 3], wide_t[:, 1:T + 1] = p, t
    assert same_bits(whole, fn(wide_p[:, 3:T + 3], wide_t[:, 1:T + 1]))     # strided, unaligned views against their copies
    bad_p = p.clone()
    bad_p[1, 77] = float("nan")
    got = fn(bad_p, t, lengths=torch.tensor([T, T, T + 1], device=DEV))     # a NaN sample, an impossible length
    assert same_bits(got[0], whole[0]) and got[1:].isnan().all()
