"""T.InverseMelScale / F.inverse_mel_scale / pipelines.GriffinLimVocoder on the device against the float64 oracle
(tests/inverse_mel_oracle.py) within the issue's bound, for every configuration, storage type, input layout and log_input
setting; the bit-for-bit invariants (layout, alignment, batch, repetition); the result's layout; the round trip through
MelScale; limits, the precision / training path, graph capture and the vocoder.  Shapes: at most 3 rows and 2 tiles + 3
frames, the frame counts around the tile; the oracle's pseudo-inverses are computed once (O.reference)."""
import warnings

import numpy as np
import pytest
import torch

import inverse_mel_oracle as O
import audio_amd.functional as F
import audio_amd.transforms as T
from audio_amd.pipelines import GriffinLimVocoder

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
BITS = {torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16}


def dtype_id(d):
    return str(d).split(".")[-1]


def tile():
    return F.inverse_mel_tiles()[0]


def module(name, **kw):
    n_stft, n_mels, sr, f_max, norm, scale = O.CONFIGS[name]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return T.InverseMelScale(n_stft, n_mels, sr, 0.0, f_max, norm, scale, **kw).to(DEV)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(BITS[a.dtype]),
                                                                     b.contiguous().view(BITS[b.dtype]))


def shapes(name):
    """(frames, rows): the frame counts around the tile; `taco` (the large product) at one."""
    t = tile()
    if name == "taco":
        return [(2 * t + 3, 3)]
    return [(1, 3), (t - 1, 1), (t, 3), (t + 1, 2), (2 * t + 3, 3)]


# ---- parity -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("log_input", [False, True], ids=["plain", "log_input"])
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
@pytest.mark.parametrize("name", list(O.CONFIGS))
def test_parity_with_the_oracle(name, dtype, log_input):
    n_stft, n_mels = O.CONFIGS[name][:2]
    rank, p = O.reference(name)
    fb = O.filterbank(name).to(DEV)
    worst, clamped, total = 0.0, 0, 0
    for seed, (T_, rows) in enumerate(shapes(name)):
        x = O.mel_values(rows, n_mels, T_, dtype, log_input, 100 + seed)
        x64 = x.to(torch.float64).numpy()
        want, bound = O.inverse_mel(x64, p, log_input), O.bound(x64, p, dtype, log_input)
        clamped, total = clamped + int((want == 0).sum()), total + want.size
        first = None
        for layout in O.LAYOUTS:
            got = F.inverse_mel_scale(O.laid_out(x.to(DEV), layout), fb, log_input=log_input)
            assert got.shape == (rows, n_stft, T_) and got.dtype == dtype and got.device.type == "cuda"
            assert got.stride() == (T_ * n_stft, 1, n_stft)
            ratio = O.worst_ratio(got.to(torch.float64).cpu().numpy(), want, bound)
            worst = max(worst, ratio)
            assert ratio <= 1.0, (layout, T_, rows, ratio)
            if first is None:
                first = got
            else:
                assert same_bits(got, first), (layout, T_, rows)             # layout and alignment change no bit
    share = clamped / total
    print("inverse_mel %s %s log_input=%s rank %d: largest error / bound %.4f, share clamped by relu %.3f"
          % (name, dtype_id(dtype), log_input, rank, worst, share))
    assert 0.05 <= share <= 0.5, share                  # a relu that clamps nothing, or everything, cannot pass


# ---- bit-for-bit invariants ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_rows_and_repetition_change_no_bit(dtype):
    name = "default"
    n_mels = O.CONFIGS[name][1]
    m = module(name)
    x = O.mel_values(3, n_mels, 2 * tile() + 3, dtype, False, 7).to(DEV)
    all3 = m(x)
    assert same_bits(m(x), all3)                                             # two calls
    for r in range(3):
        assert same_bits(m(x[r:r + 1])[0], all3[r]), r                       # a row of a batch, and the row alone
        assert same_bits(m(x[r]), all3[r]), r                                # 2-D input
    fm = x.transpose(1, 2).contiguous().transpose(1, 2)
    assert same_bits(m(fm), all3)
    assert same_bits(m(x.view(3, 1, n_mels, -1)).view(all3.shape), all3)     # leading dims collapse
    wide = torch.zeros(3, n_mels, 2 * x.shape[-1], dtype=dtype, device=DEV)
    wide[:, :, ::2] = x
    assert wide[:, :, ::2].stride() == (2 * n_mels * x.shape[-1], 2 * x.shape[-1], 2)
    assert same_bits(m(wide[:, :, ::2]), all3)                               # neither layout: gathered by the host first


# ---- layout -------------------------------------------------------------------------------------------------------------------

def test_result_is_frame_major_and_its_transpose_is_contiguous():
    """The frame-major buffer is what `.transpose(-1, -2)` exposes without a copy; GriffinLim and InverseSpectrogram accept
    the view (that they copy nothing themselves is not observable from here and not claimed)."""
    name = "tiny"
    n_stft, n_mels = O.CONFIGS[name][:2]
    m = module(name)
    B, T_ = 2, tile() + 1
    out = m(O.mel_values(B, n_mels, T_, torch.float32, False, 3).to(DEV))
    assert out.shape == (B, n_stft, T_) and out.stride() == (T_ * n_stft, 1, n_stft)
    fm = out.transpose(-1, -2)
    assert fm.is_contiguous() and fm.contiguous().data_ptr() == out.data_ptr()
    torch.manual_seed(0)
    wave = T.GriffinLim(n_fft=2 * (n_stft - 1), n_iter=1, power=1).to(DEV)(out)
    assert wave.shape == (B, (n_stft - 1) * (T_ - 1)) and bool(torch.isfinite(wave).all())
    spec = T.InverseSpectrogram(n_fft=2 * (n_stft - 1)).to(DEV)(torch.complex(out, torch.zeros_like(out)))
    assert spec.shape == wave.shape


# ---- round trip ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(O.CONFIGS))
def test_round_trip_through_melscale(name):
    n_stft, n_mels = O.CONFIGS[name][:2]
    _, p = O.reference(name)
    fb = O.filterbank(name)
    # a mel spectrogram that a spectrogram has: fb^T s for s iid uniform(0, 1); inexact only through relu and the rank cut
    s = O.mel_values(2, n_stft, tile() + 1, torch.float64, False, 21)
    x = torch.matmul(fb.double().T, s).float()
    back = F.mel_scale(F.inverse_mel_scale(x.to(DEV), fb.to(DEV)), fb.to(DEV)).cpu()
    x64 = x.double().numpy()
    o_back = np.matmul(fb.double().numpy().T, O.inverse_mel(x64, p))
    got = float(np.abs(back.double().numpy() - x64).max() / np.abs(x64).max())
    ref = float(np.abs(o_back - x64).max() / np.abs(x64).max())
    print("round trip %s: relative error %.4g, the oracle's %.4g" % (name, got, ref))
    assert got < 1.5 * ref


# ---- limits and the precision / training path -----------------------------------------------------------------------------------

def test_limits():
    limit = F.inverse_mel_tiles()[2]
    assert limit == 256
    fb = torch.rand(300, limit + 1, device=DEV)
    with pytest.raises(NotImplementedError, match="256"):
        F.inverse_mel_scale(torch.rand(1, limit + 1, 4, device=DEV), fb)
    fb = torch.rand(40, limit, device=DEV)                                   # the limit itself is served: 145 KB of LDS
    x = torch.rand(2, limit, 5, device=DEV)
    p = F._inverse_mel_matrix(fb, fb.device)
    got = F.inverse_mel_scale(x, fb)
    want = torch.relu(torch.matmul(p.double(), x.double()))
    b = (limit + 2) * 2.0 ** -24 * torch.matmul(p.double().abs(), x.double())
    assert bool(((got.double() - want).abs() <= b).all())
    m = module("tiny")
    with pytest.raises(ValueError, match="Expected an input with 12 mel bins. Found: 11"):
        m(torch.rand(2, 11, 4, device=DEV))
    with pytest.raises(TypeError):
        m(torch.ones(2, 12, 4, device=DEV, dtype=torch.int64))
    assert m(torch.rand(2, 12, 0, device=DEV)).shape == (2, 33, 0)
    assert m(torch.rand(0, 12, 4, device=DEV)).shape == (0, 33, 4)


def test_float64_and_grad_take_the_torch_composition():
    name = "tiny"
    n_stft, n_mels = O.CONFIGS[name][:2]
    _, p = O.reference(name)
    m = module(name)
    x = O.mel_values(2, n_mels, 9, torch.float64, False, 31).to(DEV)
    got = m(x)
    assert got.dtype == torch.float64
    pd = torch.from_numpy(np.array(p)).to(DEV)
    assert torch.allclose(got, torch.relu(torch.matmul(pd, x)), rtol=1e-12, atol=1e-12)
    assert torch.allclose(F.inverse_mel_scale(x.log(), m.fb, log_input=True), got, rtol=1e-10, atol=1e-12)
    x32 = x.float().requires_grad_(True)
    got32 = m(x32)
    assert got32.requires_grad
    assert torch.equal(got32.detach(), torch.relu(torch.matmul(F._inverse_mel_matrix(m.fb, m.fb.device), x32.detach())))
    with torch.no_grad():                                                    # grad mode off: the kernel
        assert not m(x32).requires_grad
    # gradcheck on an input whose products stay away from the relu kink by far more than the bound (bins that no filter
    # reaches are exactly zero on both sides of it: their gradient is zero analytically and numerically)
    live = np.abs(p).sum(axis=1) > 1e-9                 # (their rows of P are zero up to 1e-17: harmless either side)
    for seed in range(64):
        xg = O.mel_values(1, n_mels, 3, torch.float64, False, 200 + seed)
        if np.abs(np.matmul(p, xg.numpy()))[:, live].min() > 1e-3:
            break
    else:
        raise AssertionError("no input away from the kink")
    xg = xg.to(DEV).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda t: m(t), (xg,), eps=1e-6, atol=1e-6)


# ---- graph capture ------------------------------------------------------------------------------------------------------------

def test_graph_capture():
    name = "small"
    n_mels = O.CONFIGS[name][1]
    x = O.mel_values(2, n_mels, tile() + 1, torch.float32, False, 41).to(DEV)
    fresh = module(name)                                                     # its pseudo-inverse is not on the device yet
    g = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="run the call once eagerly"):
        with torch.cuda.graph(g):
            doubled = x * 2                                                  # the capture is not empty
            fresh(doubled)
    torch.cuda.synchronize()
    eager = fresh(x)
    static = x.clone()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fresh(static)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = fresh(static)
    static.copy_(x)
    g.replay()
    torch.cuda.synchronize()
    assert same_bits(out, eager)


# ---- the vocoder --------------------------------------------------------------------------------------------------------------

def test_vocoder():
    T_ = 2 * tile() + 3
    _, p = O.reference("taco")
    x = O.mel_values(2, 80, T_, torch.float32, True, 51).to(DEV)
    lengths = torch.tensor([T_, T_ - 5], device=DEV)
    v = GriffinLimVocoder(n_iter=2).to(DEV)
    assert v.sample_rate == 22050
    torch.manual_seed(0)
    wave, out_lengths = v(x, lengths)
    assert wave.shape == (2, 256 * (T_ - 1)) and wave.dtype == torch.float32 and out_lengths is lengths
    fb = v.inv_mel.fb
    spec = F.inverse_mel_scale(x, fb, log_input=True)
    torch.manual_seed(0)
    want = T.GriffinLim(1024, n_iter=2, power=1, hop_length=256).to(DEV)(spec)
    assert same_bits(wave, want)
    assert v(x)[1] is None
    # exp by torch, then the plain product: each side within its own bound of its own oracle value
    y = torch.exp(x)
    plain = F.inverse_mel_scale(y, fb)
    x64, y64 = x.double().cpu().numpy(), y.double().cpu().numpy()
    want_log, want_plain = O.inverse_mel(x64, p, True), O.inverse_mel(y64, p)
    b_log, b_plain = O.bound(x64, p, torch.float32, True), O.bound(y64, p, torch.float32)
    assert O.worst_ratio(spec.double().cpu().numpy(), want_log, b_log) <= 1.0
    assert O.worst_ratio(plain.double().cpu().numpy(), want_plain, b_plain) <= 1.0
    gap = np.abs(spec.double().cpu().numpy() - plain.double().cpu().numpy())
    assert (gap <= b_log + b_plain + np.abs(want_log - want_plain)).all()
