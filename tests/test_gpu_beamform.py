"""MVDR beamforming on the MI355X against the complex128 oracle (tests/beamform_oracle.py).

Tolerances come from the oracle, never from the code under test: PSD and apply `|err| <= 4 * u * sum|terms|` per element
(u = 2^-23 for complex64, 2^-52 for complex128), weights and RTF `max|err| <= 8 * cond(loaded psd_n) * u * max|w|`.  The
solve is tested in complex64 only where psd_n has full rank (T >= 2C + 5, cond <= 1e5 asserted); rank-deficient cases
(T = 1, T < C) test the solve in complex128."""
import numpy as np
import pytest
import torch

import beamform_oracle as O
import audio_amd.functional as F
import audio_amd.transforms as T

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = {torch.complex64: 2.0 ** -23, torch.complex128: 2.0 ** -52}
REAL = {torch.complex64: torch.float32, torch.complex128: torch.float64}
FT, TC = 16, 16                                   # bf::kFT, bf::kTCMax (test_tiles_are_the_exported_constants)
CHANNELS = [1, 2, 3, 4, 8, 16]
DTYPES = [torch.complex64, torch.complex128]


def spec(rng, lead, Cc, Fq, Tt, dtype, kind="time"):
    x = torch.from_numpy(rng.standard_normal(lead + (Cc, Fq, Tt)) + 1j * rng.standard_normal(lead + (Cc, Fq, Tt))).to(dtype)
    if kind == "frame":
        return x.transpose(-1, -2).contiguous().to(DEV).transpose(-1, -2)
    if kind == "sliced":                          # neither axis has unit stride: the gather
        wide = torch.zeros(lead + (Cc, Fq, 2 * Tt), dtype=dtype)
        wide[..., ::2] = x
        return wide.to(DEV)[..., ::2]
    return x.to(DEV)


def mask(rng, lead, Fq, Tt, dtype):
    return torch.from_numpy(rng.uniform(0.05, 1.0, lead + (Fq, Tt))).to(REAL[dtype]).to(DEV)


def n_(t):
    return t.detach().cpu().resolve_conj().numpy()


def check_psd(got, x, m, normalize, eps=1e-10):
    want = O.psd(n_(x), None if m is None else n_(m), normalize, eps, wide=True)
    bound = 4 * U[x.dtype] * O.psd_abs_terms(n_(x), None if m is None else n_(m), normalize, eps)
    err = np.abs(n_(got) - want)
    assert np.all(err <= bound), float((err / np.maximum(bound, 1e-300)).max())
    assert torch.equal(got, got.mH)


def check_weights(got, want, cond, dtype, what=""):
    ratio = np.abs(n_(got) - want).max() / (cond * U[dtype] * np.abs(want).max())
    print(f"{what}: achieved {ratio:.3g} of cond * u * max|w| (cond {cond:.3g})")
    assert ratio <= 8, (what, ratio)


def test_tiles_are_the_exported_constants():
    assert F.beamform_tiles() == (FT, TC)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Cc", CHANNELS)
def test_psd_shapes_layouts_masks(dtype, Cc):
    rng = np.random.default_rng(Cc)
    cases = [((), 1, 1, "time"), ((2,), 5, 2 * Cc + 5, "frame"), ((2, 3), FT - 1, 131, "time"), ((2,), FT, TC + 1, "frame"),
             ((), FT + 1, TC + 1, "time"), ((2,), FT + 1, 131, "frame"), ((2,), 5, TC + 1, "sliced"), ((), 5, 1, "frame")]
    for lead, Fq, Tt, kind in cases:
        x = spec(rng, lead, Cc, Fq, Tt, dtype, kind)
        m = mask(rng, lead, Fq, Tt, dtype)
        m[..., Fq // 2, :] = 0.0                  # an all-zero row: the eps path
        check_psd(F.psd(x), x, None, True)
        for norm in (True, False):
            got = F.psd(x, m, norm)
            assert got.shape == lead + (Fq, Cc, Cc) and got.dtype == dtype
            check_psd(got, x, m, norm)
        m2 = mask(rng, lead, Fq, Tt, dtype)
        both = F._psd_pair(x, m, m2, True, 1e-15)
        assert torch.equal(both[0], F.psd(x, m, True, 1e-15)) and torch.equal(both[1], F.psd(x, m2, True, 1e-15))
        assert torch.equal(F.psd(x, m), F.psd(x, m))          # two calls, the same bits


def test_psd_module_multi_mask():
    rng = np.random.default_rng(1)
    x = spec(rng, (2,), 3, 5, 9, torch.complex64)
    mm = torch.from_numpy(rng.uniform(0.05, 1, (2, 3, 5, 9))).float().to(DEV)
    got = T.PSD(multi_mask=True)(x, mm)
    check_psd(got, x, mm.mean(-3), True, 1e-15)
    check_psd(T.PSD(normalize=False)(x, mm[:, 0]), x, mm[:, 0], False)
    assert torch.equal(T.PSD()(x), F.psd(x))


def _psds(rng, lead, Cc, Fq, Tt, dtype):
    x = spec(rng, lead, Cc, Fq, Tt, dtype)
    m = mask(rng, lead, Fq, Tt, dtype)
    return x, F.psd(x, m), F.psd(x, 1.05 - m)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Cc", CHANNELS)
def test_weights_full_rank(dtype, Cc):
    rng = np.random.default_rng(50 + Cc)
    for lead, Fq in (((), 1), ((2,), 5), ((2, 3), FT + 1)):
        x, ps, pn = _psds(rng, lead, Cc, Fq, 2 * Cc + 5, dtype)
        u = torch.from_numpy(rng.standard_normal(lead + (Cc,)) + 1j * rng.standard_normal(lead + (Cc,))).to(dtype).to(DEV)
        for loading in (True, False):
            cond = O.condition(n_(pn), loading=loading)
            assert cond <= 1e5, cond
            for ref, oref in ((Cc - 1, Cc - 1), (u, n_(u))):
                got = F.mvdr_weights_souden(ps, pn, ref, loading)
                assert got.shape == lead + (Fq, Cc) and got.dtype == dtype
                check_weights(got, O.mvdr_weights_souden(n_(ps), n_(pn), oref, loading), cond, dtype, f"souden C={Cc}")
                for n_iter in (1, 2, 3, 5):
                    check_weights(F.rtf_power(ps, pn, ref, n_iter, loading),
                                  O.rtf_power(n_(ps), n_(pn), oref, n_iter, loading), cond, dtype, f"rtf_power {n_iter} C={Cc}")
            r = F.rtf_power(ps, pn, 0, 3, loading)
            for ref, oref in ((None, None), (0, 0), (u, n_(u))):
                check_weights(F.mvdr_weights_rtf(r, pn, ref, loading), O.mvdr_weights_rtf(n_(r), n_(pn), oref, loading), cond,
                              dtype, f"rtf C={Cc}")
        # apply, and the module = the chain
        w = F.mvdr_weights_souden(ps, pn, 0)
        y = F.apply_beamforming(w, x)
        assert np.all(np.abs(n_(y) - O.apply_beamforming(n_(w), n_(x), wide=True)) <= 4 * U[dtype] * O.apply_abs_terms(n_(w), n_(x)))
        assert torch.equal(T.SoudenMVDR()(x, ps, pn, 0), y)
        r = F.rtf_power(ps, pn, 0)
        assert torch.equal(T.RTFMVDR()(x, r, pn, 0), F.apply_beamforming(F.mvdr_weights_rtf(r, pn, 0), x))


@pytest.mark.parametrize("Cc", [2, 3, 4, 8, 16])
def test_rank_deficient_noise_psd_in_complex128(Cc):
    """T = 1 and T < C: psd_n has rank T, loading makes it invertible with cond ~ 1e7; PSD and apply in both precisions, the
    solve in complex128 with the same formula."""
    rng = np.random.default_rng(80 + Cc)
    for Tt in sorted({1, Cc - 1}):
        for dtype in DTYPES:
            x = spec(rng, (2,), Cc, 5, Tt, dtype)
            m = mask(rng, (2,), 5, Tt, dtype)
            check_psd(F.psd(x, m), x, m, True)
            w = spec(rng, (2,), 5, Cc, 1, dtype)[..., 0].contiguous()
            y = F.apply_beamforming(w, x)
            assert np.all(np.abs(n_(y) - O.apply_beamforming(n_(w), n_(x), wide=True)) <= 4 * U[dtype] * O.apply_abs_terms(n_(w), n_(x)))
        dtype = torch.complex128
        x, ps, pn = _psds(rng, (2,), Cc, 5, Tt, dtype)
        cond = O.condition(n_(pn))
        check_weights(F.mvdr_weights_souden(ps, pn, 0), O.mvdr_weights_souden(n_(ps), n_(pn), 0), cond, dtype, f"souden T={Tt}")
        check_weights(F.rtf_power(ps, pn, 0), O.rtf_power(n_(ps), n_(pn), 0), cond, dtype, f"rtf_power T={Tt}")
        r = F.rtf_power(ps, pn, 0)
        check_weights(F.mvdr_weights_rtf(r, pn, 0), O.mvdr_weights_rtf(n_(r), n_(pn), 0), cond, dtype, f"rtf T={Tt}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_apply_layouts(dtype):
    rng = np.random.default_rng(3)
    for lead, Cc, Fq, Tt, kind in (((), 1, 1, 1, "time"), ((2,), 2, 5, 9, "frame"), ((2, 3), 3, FT + 1, 131, "time"),
                                   ((2,), 4, 129, 33, "frame"), ((2,), 16, 15, 37, "sliced"), ((), 8, 257, 3, "frame")):
        x = spec(rng, lead, Cc, Fq, Tt, dtype, kind)
        w = spec(rng, lead, Fq, Cc, 1, dtype)[..., 0].contiguous()
        y = F.apply_beamforming(w, x)
        assert y.shape == lead + (Fq, Tt)
        if kind == "frame" and Fq > 1 and Tt > 1:
            assert y.stride(-2) == 1                       # frame-major in, frame-major out
        assert np.all(np.abs(n_(y) - O.apply_beamforming(n_(w), n_(x), wide=True)) <= 4 * U[dtype] * O.apply_abs_terms(n_(w), n_(x)))


def test_seventeen_channels_raise():
    x = torch.zeros(17, 5, 7, dtype=torch.complex64, device=DEV)
    p = torch.zeros(5, 17, 17, dtype=torch.complex64, device=DEV)
    for call in (lambda: F.psd(x), lambda: F.mvdr_weights_souden(p, p, 0), lambda: F.rtf_power(p, p, 0),
                 lambda: F.mvdr_weights_rtf(p[..., 0], p), lambda: F.apply_beamforming(p[..., 0], x)):
        with pytest.raises(NotImplementedError):
            call()


@pytest.mark.parametrize("solution", ["ref_channel", "stv_power"])
def test_mvdr_module(solution):
    rng = np.random.default_rng(9)
    x = spec(rng, (2,), 4, 9, 21, torch.complex64, "frame")
    ms, mn = mask(rng, (2,), 9, 21, torch.complex64), mask(rng, (2,), 9, 21, torch.complex64)
    y = T.MVDR(1, solution)(x, ms, mn)
    assert y.dtype == torch.complex64 and y.shape == (2, 9, 21) and y.stride(-2) == 1
    xd = x.cdouble()
    ps, pn = F.psd(xd, ms.double(), True, 1e-15), F.psd(xd, mn.double(), True, 1e-15)
    if solution == "ref_channel":
        w = F.mvdr_weights_souden(ps, pn, 1)
    else:
        w = F.mvdr_weights_rtf(F.rtf_power(ps, pn, 1), pn, 1)
    assert torch.equal(y, F.apply_beamforming(w, xd).to(torch.complex64))
    want = O.mvdr(n_(x), n_(ms), n_(mn), 1, solution)
    assert np.abs(n_(y) - want).max() <= 8 * 2.0 ** -23 * np.abs(want).max()      # complex128 inside: one final rounding
    with pytest.warns(UserWarning, match="mask_n"):
        y1 = T.MVDR(1, solution)(x, ms)
    assert torch.equal(y1, T.MVDR(1, solution)(x, ms, 1 - ms))
    mm = torch.stack([ms, mn, ms, mn], dim=1)
    assert torch.equal(T.MVDR(1, solution, multi_mask=True)(x, mm, 1 - mm), T.MVDR(1, solution)(x, mm.mean(1), (1 - mm).mean(1)))


def _route_inputs():
    rng = np.random.default_rng(11)
    x = spec(rng, (2,), 3, FT + 1, TC + 1, torch.complex64, "frame")
    m = mask(rng, (2,), FT + 1, TC + 1, torch.complex64)
    return x, m, F.psd(x, m), F.psd(x, 1.05 - m)


def test_shim_and_ctypes_routes_give_equal_bits():
    x, m, ps, pn = _route_inputs()
    res = {}
    try:
        for kind in ("shim", "ctypes"):
            F._force_route(kind)
            r = F.rtf_power(ps, pn, 0)
            res[kind] = (F.psd(x, m), F._psd_pair(x, m, 1 - m), F.mvdr_weights_souden(ps, pn, 1), r,
                         F.mvdr_weights_rtf(r, pn, 1), F.apply_beamforming(r, x), F.apply_beamforming(r, x.contiguous()))
    finally:
        F._force_route(None)
    for a, b in zip(res["shim"], res["ctypes"]):
        assert torch.equal(a, b) and a.stride() == b.stride()


def test_scripted_equals_eager():
    x, m, ps, pn = _route_inputs()
    r = F.rtf_power(ps, pn, 0)
    u = torch.tensor([0.5, 0.25j, 1.0], dtype=torch.complex64, device=DEV).expand(2, 3)
    assert torch.equal(torch.jit.script(T.PSD())(x, m), T.PSD()(x, m))
    for ref in (1, u):
        assert torch.equal(torch.jit.script(T.SoudenMVDR())(x, ps, pn, ref), T.SoudenMVDR()(x, ps, pn, ref))
        assert torch.equal(torch.jit.script(T.RTFMVDR())(x, r, pn, ref), T.RTFMVDR()(x, r, pn, ref))
    for sol in ("ref_channel", "stv_power"):
        assert torch.equal(torch.jit.script(T.MVDR(0, sol))(x, m, 1 - m), T.MVDR(0, sol)(x, m, 1 - m))


def test_torch_compile_fullgraph():
    x, m, ps, pn = _route_inputs()
    for mod, inp in ((T.PSD(), (x, m)), (T.SoudenMVDR(), (x, ps, pn, 0)), (T.MVDR(), (x, m, 1 - m))):
        assert torch.equal(torch.compile(mod, fullgraph=True)(*inp), mod(*inp))


def test_graph_capture_of_souden_mvdr():
    x, m, ps, pn = _route_inputs()
    mod = T.SoudenMVDR()
    eager = mod(x, ps, pn, 0)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        mod(x, ps, pn, 0)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = mod(x, ps, pn, 0)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


def test_spectrogram_mvdr_inverse_without_a_layout_copy():
    g = torch.Generator().manual_seed(0)
    wav = torch.randn(2, 4, 2000, generator=g).to(DEV)
    stft, istft = T.Spectrogram(n_fft=64, power=None), T.InverseSpectrogram(n_fft=64)
    x = stft(wav)
    assert x.shape[:3] == (2, 4, 33) and x.stride(-2) == 1             # frame-major
    m = torch.rand(x.shape[0], x.shape[2], x.shape[3], generator=g).to(DEV) * 0.9 + 0.05
    y = T.MVDR()(x, m, 1 - m)
    assert y.shape == (2, 33, x.shape[-1]) and y.stride(-2) == 1 and y.stride(-1) == 33   # what InverseSpectrogram reads in place
    out = istft(y, 2000)
    assert out.shape == (2, 2000) and torch.isfinite(out).all()
    want = O.mvdr(n_(x), n_(m), n_(1 - m))
    assert np.abs(n_(y) - want).max() <= 8 * 2.0 ** -23 * np.abs(want).max()


# ---- gradients: complex128 at C = 3, F = 2, T = 11, default tolerances -------------------------------------------------------------

def _grad_inputs():
    rng = np.random.default_rng(21)
    x = spec(rng, (), 3, 2, 11, torch.complex128)
    m = mask(rng, (), 2, 11, torch.complex128)
    ps, pn = F.psd(x, m), F.psd(x, 1.05 - m)
    return x, m, ps, pn


def _check(fn, *inputs):
    inputs = [t.clone().requires_grad_(True) for t in inputs]
    assert torch.autograd.gradcheck(fn, inputs)
    assert torch.autograd.gradgradcheck(fn, inputs)


def test_grad_psd():
    x, m, _, _ = _grad_inputs()
    _check(lambda a, b: F.psd(a, b), x, m)
    _check(lambda a: F.psd(a), x)
    _check(lambda b: F.psd(x, b, normalize=False), m)


def test_grad_weights():
    _, _, ps, pn = _grad_inputs()
    u = torch.tensor([0.3, 0.5 + 0.2j, -0.4j], dtype=torch.complex128, device=DEV)
    _check(lambda s, n: F.mvdr_weights_souden(s, n, 1), ps, pn)
    _check(lambda s, n: F.mvdr_weights_souden(s, n, u, diagonal_loading=False), ps, pn)
    r = F.rtf_power(ps, pn, 0)
    _check(lambda a, n: F.mvdr_weights_rtf(a, n, 1), r, pn)
    _check(lambda a, n: F.mvdr_weights_rtf(a, n), r, pn)


def test_grad_rtf_power():
    _, _, ps, pn = _grad_inputs()
    _check(lambda s, n: F.rtf_power(s, n, 0, n_iter=3), ps, pn)


def test_grad_apply():
    x, _, ps, pn = _grad_inputs()
    w = F.mvdr_weights_souden(ps, pn, 0)
    _check(lambda a, b: F.apply_beamforming(a, b), w, x)


def test_grad_mvdr_wrt_masks():
    x, m, _, _ = _grad_inputs()
    for sol in ("ref_channel", "stv_power"):
        mod = T.MVDR(0, sol)
        _check(lambda a, b: mod(x, a, b), m, (1.05 - m))


def test_grad_one_channel_to_second_order():
    """C = 1: a.mH of a (bins, 1, 1) matrix already counts as contiguous and keeps its lazy conjugate bit; the recorded
    backward must solve with A^H all the same."""
    rng = np.random.default_rng(31)
    x = spec(rng, (), 1, 2, 11, torch.complex128)
    m = mask(rng, (), 2, 11, torch.complex128)
    ps, pn = F.psd(x, m), F.psd(x, 1.05 - m)
    _check(lambda s, n: F.mvdr_weights_souden(s, n, 0), ps, pn)
    _check(lambda s, n: F.rtf_power(s, n, 0, n_iter=3), ps, pn)
    r = F.rtf_power(ps, pn, 0)
    _check(lambda a, n: F.mvdr_weights_rtf(a, n, 0), r, pn)


def test_lazily_conjugated_inputs():
    """psd.conj() carries a conjugate bit, not conjugated memory: with and without grad the result is that of the resolved
    tensor, and the gradient checks through it."""
    x, m, ps, pn = _grad_inputs()
    sc, nc = ps.conj(), pn.conj()
    assert sc.is_conj() and nc.is_conj()
    want = F.mvdr_weights_souden(sc.resolve_conj(), nc.resolve_conj(), 1)
    assert torch.equal(F.mvdr_weights_souden(sc, nc, 1), want)
    got = F.mvdr_weights_souden(ps.clone().requires_grad_(True).conj(), pn.clone().requires_grad_(True).conj(), 1)
    assert np.abs(n_(got) - n_(want)).max() <= 1e-12 * np.abs(n_(want)).max()
    _check(lambda s, n: F.mvdr_weights_souden(s.conj(), n.conj(), 1), ps, pn)
    _check(lambda s, n: F.mvdr_weights_souden(s.conj(), n.conj(), 1, diagonal_loading=False), ps, pn)   # the bit reaches A too
    assert torch.equal(F.psd(x.conj(), m), F.psd(x.conj().resolve_conj(), m))
    w = F.mvdr_weights_souden(ps, pn, 0)
    assert torch.equal(F.apply_beamforming(w.conj(), x.conj()),
                       F.apply_beamforming(w.conj().resolve_conj(), x.conj().resolve_conj()))


def test_forward_with_grad_equals_inference_path():
    x, m, ps, pn = _grad_inputs()
    a = F.mvdr_weights_souden(ps.clone().requires_grad_(True), pn, 0)
    b = F.mvdr_weights_souden(ps, pn, 0)
    assert np.abs(n_(a) - n_(b)).max() <= 1e-12 * np.abs(n_(b)).max()
