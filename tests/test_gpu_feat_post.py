"""F.compute_deltas / F.sliding_window_cmn on the device: parity with the float64 oracle, both delta layouts and all pad
modes, reduced precision, the users' pipelines, gradients, TorchScript, both launch routes, determinism, graph capture
and torch.compile."""
import numpy as np
import pytest
import torch

import feat_post_oracle as O
import audio_amd.functional as F
import audio_amd.transforms as T
from audio_amd.compliance import kaldi
from test_feat_post import assert_cmvn_close, cmvn_condition

pytestmark = pytest.mark.gpu
DEV = "cuda"
MODES = ["replicate", "reflect", "circular", "constant"]
T_GRID = [1, 2, 5, 99, 100, 101, 599, 601, 1001, 2500]


def _ok_mode(mode, n, Tn):
    return not ((mode == "reflect" and n >= Tn) or (mode == "circular" and n > Tn))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("layout", ["time_contiguous", "frame_major"])
def test_deltas_parity(mode, layout):
    g = torch.Generator().manual_seed(0)
    for Tn in T_GRID:
        for win_length in (3, 4, 5, 9):
            if not _ok_mode(mode, (win_length - 1) // 2, Tn):
                continue
            if layout == "time_contiguous":
                x = torch.randn(2, 3, 17, Tn, generator=g)
                xd = x.to(DEV)
            else:
                x = torch.randn(2, 3, Tn, 17, generator=g).transpose(-1, -2)
                xd = x.transpose(-1, -2).contiguous().to(DEV).transpose(-1, -2)     # frame-major storage
            want = O.deltas_pad_corr(x.double().numpy(), win_length, mode)
            got = F.compute_deltas(xd, win_length, mode)
            assert got.is_contiguous() and got.shape == x.shape and got.dtype == torch.float32
            assert np.abs(got.cpu().numpy() - want).max() <= 1e-5 * np.abs(x.numpy()).max(), (Tn, win_length)
            got64 = F.compute_deltas(xd.double(), win_length, mode)
            assert np.abs(got64.cpu().numpy() - want).max() <= 1e-12 * np.abs(x.numpy()).max()


def test_deltas_random_shapes_and_1d():
    rng = np.random.default_rng(1)
    for _ in range(12):
        shape = tuple(int(v) for v in rng.integers(1, 6, size=rng.integers(0, 3))) + (int(rng.integers(1, 130)),
                                                                                         int(rng.integers(1, 700)))
        x = torch.from_numpy(rng.standard_normal(shape).astype(np.float32))
        w = int(rng.integers(3, 12))
        want = O.deltas_pad_corr(x.double().numpy(), w)
        got = F.compute_deltas(x.to(DEV), w).cpu().numpy()
        assert np.abs(got - want).max() <= 1e-5 * np.abs(x.numpy()).max(), shape
    x = torch.randn(777)
    got = F.compute_deltas(x.to(DEV)).cpu().numpy()
    assert got.shape == (777,)
    assert np.abs(got - O.deltas_pad_corr(x.double().numpy())).max() <= 1e-5 * x.abs().max().item()


def _cmn_cases():
    for Tn in T_GRID:
        for win in (1, 2, 7, 600):
            for mn in (0, 100, Tn + 5):
                for center in (False, True):
                    yield Tn, win, mn, center


def test_cmn_parity_mean():
    g = torch.Generator().manual_seed(2)
    for Tn, win, mn, center in _cmn_cases():
        x = torch.randn(3, Tn, 13, generator=g) * 4.0 + 10.0
        want = O.cmn_prefix(x.double().numpy(), win, mn, center)
        got = F.sliding_window_cmn(x.to(DEV), win, mn, center).cpu().numpy()
        peak = np.abs(x.numpy()).reshape(3, -1).max(1).reshape(3, 1, 1)
        assert (np.abs(got - want) <= 2e-6 * peak).all(), (Tn, win, mn, center)
        got64 = F.sliding_window_cmn(x.double().to(DEV), win, mn, center).cpu().numpy()
        assert (np.abs(got64 - want) <= 1e-12 * peak).all()


def test_cmn_parity_norm_vars_logmel_like():
    g = torch.Generator().manual_seed(3)
    for Tn, win, mn, center in _cmn_cases():
        x = torch.randn(2, Tn, 11, generator=g) + 6.0          # log-mel like: an offset plus noise
        x32 = x.numpy()
        want = O.cmn_prefix(x32.astype(np.float64), win, mn, center, True)
        got = F.sliding_window_cmn(x.to(DEV), win, mn, center, True).cpu().numpy()
        # element-wise within 1e-5 of the output's peak wherever the window's variance is well above the rounding of
        # its mean (a 2-frame window of two nearly equal values is ill-conditioned in any summation order)
        ok = np.isfinite(want) & (cmvn_condition(x32, win, mn, center) < 1e7)
        if ok.any():
            assert np.abs(got[ok] - want[ok]).max() <= 1e-5 * np.abs(want[ok]).max(), (Tn, win, mn, center)
        assert_cmvn_close(got, want, x32, win, mn, center, rel=2e-7, atol=1e-6)


def test_cmn_strided_and_random_shapes():
    rng = np.random.default_rng(4)
    for _ in range(10):
        lead = tuple(int(v) for v in rng.integers(1, 4, size=rng.integers(0, 3)))
        Tn, F_ = int(rng.integers(1, 1500)), int(rng.integers(1, 300))
        x = torch.from_numpy(rng.standard_normal(lead + (F_, Tn)).astype(np.float32)).to(DEV).transpose(-1, -2)
        win, mn, center = int(rng.integers(0, 700)), int(rng.integers(0, 200)), bool(rng.integers(0, 2))
        want = O.cmn_prefix(x.double().cpu().numpy(), win, mn, center)
        got = F.sliding_window_cmn(x, win, mn, center)
        assert got.is_contiguous()
        assert np.abs(got.cpu().numpy() - want).max() <= 2e-6 * x.abs().max().item(), (lead, Tn, F_)
    one = F.sliding_window_cmn(torch.randn(1, 40, device=DEV))
    assert one.shape == (40,)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_reduced_precision(dtype):
    x = (torch.randn(2, 40, 300, device=DEV) + 5).to(dtype)
    for fn in (lambda t: F.compute_deltas(t), lambda t: F.sliding_window_cmn(t.transpose(-1, -2)),
               lambda t: F.sliding_window_cmn(t.transpose(-1, -2), norm_vars=True)):
        y = fn(x)
        y32 = fn(x.float())
        assert y.dtype == dtype
        assert torch.equal(y, y32.to(dtype))


def test_integer_input_raises():
    with pytest.raises(TypeError):
        F.compute_deltas(torch.ones(2, 3, 10, dtype=torch.int32, device=DEV))
    with pytest.raises(TypeError):
        F.sliding_window_cmn(torch.ones(2, 10, 3, dtype=torch.int64, device=DEV))


def test_pipelines():
    wav = torch.randn(2, 16000 * 3) * 0.3
    mel = T.MelSpectrogram(16000, 400, hop_length=160, n_mels=80).to(DEV)
    m = mel(wav.to(DEV))
    assert m.stride(-2) == 1                                          # frame-major, read in place
    d = F.compute_deltas(m)
    want = O.deltas_pad_corr(m.double().cpu().numpy())
    assert np.abs(d.cpu().numpy() - want).max() <= 1e-5 * m.abs().max().item()
    dd = F.compute_deltas(d)
    want2 = O.deltas_pad_corr(d.double().cpu().numpy())
    assert np.abs(dd.cpu().numpy() - want2).max() <= 1e-5 * d.abs().max().item()
    fb = kaldi.fbank_batch(wav.to(DEV), num_mel_bins=80)
    c = F.sliding_window_cmn(fb)
    wantc = O.cmn_prefix(fb.double().cpu().numpy())
    assert np.abs(c.cpu().numpy() - wantc).max() <= 2e-6 * fb.abs().max().item()
    fd = F.compute_deltas(fb.transpose(-1, -2))
    wantd = O.deltas_pad_corr(fb.transpose(-1, -2).double().cpu().numpy())
    assert np.abs(fd.cpu().numpy() - wantd).max() <= 1e-5 * fb.abs().max().item()


@pytest.mark.parametrize("mode", MODES)
def test_deltas_gradcheck(mode):
    x = torch.randn(2, 3, 11, dtype=torch.float64, device=DEV, requires_grad=True)
    fn = lambda t: F.compute_deltas(t, 5, mode)                       # noqa: E731
    assert torch.autograd.gradcheck(fn, (x,))
    assert torch.autograd.gradgradcheck(fn, (x,))
    xf = torch.randn(2, 11, 3, dtype=torch.float64, device=DEV).transpose(-1, -2).requires_grad_()
    assert torch.autograd.gradcheck(fn, (xf,))


@pytest.mark.parametrize("norm_vars", [False, True])
@pytest.mark.parametrize("center", [False, True])
def test_cmn_gradcheck(norm_vars, center):
    x = (torch.randn(2, 70, 3, dtype=torch.float64, device=DEV) + 2).requires_grad_()
    fn = lambda t: F.sliding_window_cmn(t, 9, 5, center, norm_vars)   # noqa: E731
    assert torch.autograd.gradcheck(fn, (x,))
    assert torch.autograd.gradgradcheck(fn, (x,))
    if norm_vars:                                                    # the training path equals the kernel's forward
        with torch.no_grad():
            k = F.sliding_window_cmn(x, 9, 5, center, True)
        assert torch.allclose(fn(x), k, rtol=0, atol=1e-10)


def test_scripted_equals_eager():
    x = torch.randn(3, 40, 500, device=DEV)
    for mod, inp in ((T.ComputeDeltas(7, "reflect"), x), (T.SlidingWindowCmn(300, 50, True, True), x.transpose(-1, -2))):
        assert torch.equal(torch.jit.script(mod)(inp), mod(inp))
    sf = torch.jit.script(F.compute_deltas)
    assert torch.equal(sf(x, 5, "replicate"), F.compute_deltas(x))
    sc = torch.jit.script(F.sliding_window_cmn)
    assert torch.equal(sc(x, 600, 100, False, False), F.sliding_window_cmn(x))


def test_shim_and_ctypes_routes_are_bit_identical():
    x = torch.randn(4, 80, 333, device=DEV)
    xf = x.transpose(-1, -2).contiguous().transpose(-1, -2)
    outs = {}
    try:
        for route in ("shim", "ctypes"):
            F._force_route(route)
            outs[route] = [F.compute_deltas(x), F.compute_deltas(xf, 9, "circular"), F.sliding_window_cmn(x),
                           F.sliding_window_cmn(xf, 100, 10, True, True), F.compute_deltas(x.double())]
    finally:
        F._force_route(None)
    for a, b in zip(outs["shim"], outs["ctypes"]):
        assert torch.equal(a, b)


def test_deterministic():
    x = torch.randn(8, 1001, 80, device=DEV)
    assert torch.equal(F.sliding_window_cmn(x, norm_vars=True), F.sliding_window_cmn(x, norm_vars=True))
    assert torch.equal(F.compute_deltas(x.transpose(-1, -2)), F.compute_deltas(x.transpose(-1, -2)))


def test_graph_capture():
    x = torch.randn(4, 1001, 80, device=DEV)
    eager = (F.compute_deltas(x.transpose(-1, -2)), F.sliding_window_cmn(x), F.sliding_window_cmn(x, norm_vars=True))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            F.compute_deltas(x.transpose(-1, -2))
            F.sliding_window_cmn(x)
            F.sliding_window_cmn(x, norm_vars=True)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = (F.compute_deltas(x.transpose(-1, -2)), F.sliding_window_cmn(x), F.sliding_window_cmn(x, norm_vars=True))
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(out, eager):
        assert torch.equal(a, b)


def test_torch_compile_fullgraph():
    x = torch.randn(3, 40, 400, device=DEV)
    for mod, inp in ((T.ComputeDeltas(), x), (T.SlidingWindowCmn(norm_vars=True), x.transpose(-1, -2))):
        c = torch.compile(mod, fullgraph=True)
        assert torch.equal(c(inp), mod(inp))
