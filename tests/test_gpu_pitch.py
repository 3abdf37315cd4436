"""F.detect_pitch_frequency on the device: the kernel's NCCF against the float64 oracle, the fused pick and the median
against the oracle applied to the kernel's own intermediate results, end to end on robust tones, batch shapes and
strides, parameters, LDS / lag-tiling and size boundaries, dtypes, both launch routes, determinism, TorchScript,
torch.compile and graph capture."""
import numpy as np
import pytest
import torch

import pitch_oracle as O
import audio_amd.functional as F
from audio_amd import _ops  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _tones(sr, seconds, rows=2, seed=0, gap=True):
    n = int(sr * seconds)
    x = np.stack([O.tone(n, sr, 95.0 + 60 * r, seed=seed + r) for r in range(rows)])
    if gap:
        x[-1, n // 3: n // 2] = 0.0
    return x


def _assert_robust(x, sr, trials=8, **kw):
    """8 perturbations of the oracle NCCF, each 1e-5 of the frame peak, leave the oracle's output unchanged."""
    s = O.sizes(x.shape[-1], sr, kw.get("frame_time", 1e-2), kw.get("win_length", 30), kw.get("freq_low", 85),
                kw.get("freq_high", 3400))
    nccf = O.nccf_prefix(x.reshape(-1, x.shape[-1]), s["fs"], s["lags"])
    base = O.smooth(O.pick(nccf, s["lag_min"]), kw.get("win_length", 30), sr)
    rng = np.random.default_rng(123)
    peak = np.abs(nccf).max(-1, keepdims=True)
    for _ in range(trials):
        pert = nccf + 1e-5 * peak * rng.uniform(-1, 1, nccf.shape)
        np.testing.assert_array_equal(O.smooth(O.pick(pert, s["lag_min"]), kw.get("win_length", 30), sr), base)
    return base.reshape(x.shape[:-1] + base.shape[-1:])


# ---- (a) the NCCF ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sr", [8000, 16000, 44100])
def test_nccf_matches_the_oracle(sr):
    x = _tones(sr, 0.3)
    s = O.sizes(x.shape[-1], sr)
    got = F._compute_nccf(torch.from_numpy(x).to(DEV), sr, 1e-2, 85)
    assert got.shape == (2, s["F"], s["lags"]) and got.dtype == torch.float32
    want = O.nccf_prefix(x, s["fs"], s["lags"])
    peak = np.abs(want).max(-1, keepdims=True)
    assert (np.abs(got.cpu().numpy() - want) <= 1e-5 * peak).all()
    silent = peak[..., 0] == 0
    assert silent.any() and (got.cpu().numpy()[silent] == 0).all()
    got64 = F._compute_nccf(torch.from_numpy(x).double().to(DEV), sr, 1e-2, 85).cpu().numpy()
    want64 = O.nccf_loops(x, s["fs"], s["lags"])
    assert (np.abs(got64 - want64) <= 1e-12 * peak).all()


# ---- (b) the fused pick, (c) the median ------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_pick_and_median_are_the_oracles_on_the_kernels_own_nccf(dtype):
    for sr in (8000, 16000, 22050):
        x = _tones(sr, 0.5, rows=3, seed=7)
        x[0, :1000] = 0.0                                         # silence: exact ties, the first lag wins
        xd = torch.from_numpy(x).to(DEV, dtype)
        s = O.sizes(x.shape[-1], sr)
        nccf = F._compute_nccf(xd, sr, 1e-2, 85).cpu().numpy()
        lag = O.pick(nccf, s["lag_min"])
        assert (lag[0, :1000 // s["fs"]] == s["lag_min"] + 1).all()
        for win in (3, 4, 30):
            got = F.detect_pitch_frequency(xd, sr, win_length=win).cpu().numpy()
            np.testing.assert_array_equal(got, O.smooth(lag, win, sr))


# ---- (d) end to end ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sr", [8000, 16000, 22050, 44100, 48000])
def test_end_to_end_on_tones(sr):
    x = np.stack([O.tone(int(sr * 0.6), sr, f0, seed=i) for i, f0 in enumerate((110.0, 220.0, 330.0))])
    want = _assert_robust(x, sr)
    got = F.detect_pitch_frequency(torch.from_numpy(x).to(DEV), sr).cpu().numpy()
    np.testing.assert_array_equal(got, want)


def test_end_to_end_glides_and_silent_gaps():
    sr = 16000
    a = O.tone(sr, sr, 0, glide=(100.0, 300.0), seed=3)
    b = O.tone(sr, sr, 0, glide=(400.0, 150.0), seed=4)
    a[4000:6500] = 0.0
    b[9000:12000] = 0.0
    x = np.stack([a, b])
    want = _assert_robust(x, sr)
    got = F.detect_pitch_frequency(torch.from_numpy(x).to(DEV), sr).cpu().numpy()
    np.testing.assert_array_equal(got, want)


# ---- shapes, strides, parameters, boundaries ------------------------------------------------------------------------------

def _check_vs_own_nccf(xd, sr, **kw):
    """Output == oracle median of the oracle pick of the kernel's own NCCF (bit for bit)."""
    ft, win, lo, hi = kw.get("frame_time", 1e-2), kw.get("win_length", 30), kw.get("freq_low", 85), kw.get("freq_high", 3400)
    got = F.detect_pitch_frequency(xd, sr, ft, win, lo, hi)
    nccf = F._compute_nccf(xd, sr, ft, lo).cpu().numpy()
    s = O.sizes(xd.shape[-1], sr, ft, win, lo, hi)
    want = O.smooth(O.pick(nccf, s["lag_min"]), win, sr)
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(xd.shape[:-1]) + (s["n_out"],)
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    return got


def test_batch_shapes_and_strided_rows():
    sr = 16000
    base = torch.from_numpy(_tones(sr, 0.4, rows=6, seed=11)).to(DEV)
    _check_vs_own_nccf(base[0], sr)                                   # 1-D
    _check_vs_own_nccf(base, sr)                                      # 2-D
    _check_vs_own_nccf(base.reshape(1, 2, 3, -1), sr)                 # 4-D
    wide = torch.zeros(6, base.shape[-1] + 77, device=DEV)
    wide[:, 5:5 + base.shape[-1]] = base
    view = wide[:, 5:5 + base.shape[-1]]                              # row stride > L, read in place
    assert not view.is_contiguous()
    np.testing.assert_array_equal(_check_vs_own_nccf(view, sr).cpu().numpy(),
                                  F.detect_pitch_frequency(view.contiguous(), sr).cpu().numpy())
    _check_vs_own_nccf(base[:, ::2][:, :4000].contiguous().t().contiguous().t(), sr)   # column-major rows (one copy)


def test_short_rows():
    sr = 16000
    _check_vs_own_nccf(torch.randn(3, 170, device=DEV), sr, win_length=3)    # shorter than lags (189): 2 frames, 1 output
    _check_vs_own_nccf(torch.randn(2, 321, device=DEV), sr, win_length=4)
    x = torch.randn(3, 150, device=DEV)                               # shorter than one frame (160)
    with pytest.raises(RuntimeError, match="maximum size"):
        F.detect_pitch_frequency(x, sr, win_length=3)                 # 1 frame + 1 < 3
    with pytest.raises(RuntimeError, match="maximum size"):
        F.detect_pitch_frequency(x, sr)


@pytest.mark.parametrize("win", [3, 4, 30])
def test_parameters(win):
    sr = 22050
    xd = torch.from_numpy(_tones(sr, 0.5, rows=2, seed=2)).to(DEV)
    _check_vs_own_nccf(xd, sr, win_length=win)
    _check_vs_own_nccf(xd, sr, win_length=win, freq_low=60, freq_high=1000)
    _check_vs_own_nccf(xd, sr, frame_time=0.025, win_length=win, freq_low=150, freq_high=5000)


def test_lds_and_lag_tiling_boundaries():
    rng = np.random.default_rng(5)
    # (sr, frame_time, freq_low, dtype): several frames per tile; one frame per tile; lags in chunks within 64 KiB and
    # within 160 KiB; the largest supported frame size and lag count
    for sr, ft, lo, dt in [(16000, 0.01, 85, torch.float32), (96000, 0.01, 20, torch.float32),
                           (96000, 0.0208, 19, torch.float32), (96000, 0.0853, 20, torch.float64),
                           (96000, 0.01, 6, torch.float32), (96000, 0.0853, 6, torch.float32)]:
        lags, fs, _ = F._pitch_sizes(1, sr, ft, lo)
        assert fs <= 8192 and lags <= 16384
        x = torch.from_numpy(rng.standard_normal((1, fs * 3 + 11))).to(DEV, dt)
        got = F._compute_nccf(x, sr, ft, lo).cpu().numpy()
        want = O.nccf_loops(x.double().cpu().numpy(), fs, lags)
        peak = np.abs(want).max(-1, keepdims=True)
        assert (np.abs(got - want) <= (1e-5 if dt == torch.float32 else 1e-12) * peak).all(), (fs, lags)
        out = F.detect_pitch_frequency(x, sr, ft, 3, lo)
        want_out = O.smooth(O.pick(got, O.sizes(1, sr, ft, 3, lo)["lag_min"]), 3, sr)
        np.testing.assert_array_equal(out.cpu().numpy(), want_out)
    x = torch.randn(1, 20000, device=DEV)
    with pytest.raises(NotImplementedError):
        F.detect_pitch_frequency(x, 96000, 0.0854, 3, 20)             # frame size 8199
    with pytest.raises(NotImplementedError):
        F.detect_pitch_frequency(x, 96000, 0.01, 3, 5)                # 19 200 lags


# ---- dtypes, gradient ------------------------------------------------------------------------------------------------------

def test_dtypes_and_no_gradient():
    sr = 16000
    x = torch.from_numpy(_tones(sr, 0.4, seed=9)).to(DEV)
    for dt in (torch.float16, torch.bfloat16):
        xl = x.to(dt)
        y = F.detect_pitch_frequency(xl, sr)
        assert y.dtype == torch.float32
        assert torch.equal(y, F.detect_pitch_frequency(xl.float(), sr))
    y64 = _check_vs_own_nccf(x.double(), sr)
    assert y64.dtype == torch.float32
    xg = x.clone().requires_grad_(True)
    yg = F.detect_pitch_frequency(xg, sr)
    assert yg.grad_fn is None and not yg.requires_grad
    assert torch.equal(yg, F.detect_pitch_frequency(x, sr))


# ---- routes, determinism, TorchScript, compile, graphs ---------------------------------------------------------------------

def test_shim_and_ctypes_routes_are_bit_identical():
    sr = 16000
    x = torch.from_numpy(_tones(sr, 0.5, rows=4, seed=1)).to(DEV)
    outs = {}
    try:
        for route in ("shim", "ctypes"):
            F._force_route(route)
            outs[route] = [F.detect_pitch_frequency(x, sr), F.detect_pitch_frequency(x.double(), sr, win_length=4),
                           F._compute_nccf(x, sr, 1e-2, 85), F._compute_nccf(x[:, 3:-5], sr, 0.025, 100)]
    finally:
        F._force_route(None)
    for a, b in zip(outs["shim"], outs["ctypes"]):
        assert torch.equal(a, b)


def test_deterministic():
    x = torch.randn(16, 48000, device=DEV)
    assert torch.equal(F.detect_pitch_frequency(x, 16000), F.detect_pitch_frequency(x, 16000))


def test_scripted_equals_eager():
    x = torch.from_numpy(_tones(16000, 0.5, seed=4)).to(DEV)
    sf = torch.jit.script(F.detect_pitch_frequency)
    assert torch.equal(sf(x, 16000, 0.01, 30, 85, 3400), F.detect_pitch_frequency(x, 16000))


def test_torch_compile_fullgraph():
    x = torch.from_numpy(_tones(16000, 0.5, seed=6)).to(DEV)

    def f(t):
        return F.detect_pitch_frequency(t, 16000) * 2.0

    c = torch.compile(f, fullgraph=True)
    assert torch.equal(c(x), f(x))


def test_graph_capture():
    x = torch.from_numpy(_tones(16000, 0.5, rows=4, seed=8)).to(DEV)
    eager = F.detect_pitch_frequency(x, 16000)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            F.detect_pitch_frequency(x, 16000)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = F.detect_pitch_frequency(x, 16000)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


def test_cpu_tensor_is_refused():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.detect_pitch_frequency(torch.randn(2, 16000), 16000)
