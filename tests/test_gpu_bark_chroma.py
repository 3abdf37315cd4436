"""F.dense_fbank_scale / T.ChromaScale / T.ChromaSpectrogram and the Bark modules on the device: the dense projection against
the float64 product of the stored operands (tests/fbank_oracle.py) within the issue's bound for the replay's shapes, layouts and
storage types; the bit-for-bit invariants (layout, alignment, batch, repetition, leading shape); the result's layout; the
modules against their compositions bit for bit; limits, the precision / training path and graph capture.  Shapes: at most 3
rows and 2 tiles + 3 frames; a case's reference is computed once and shared by its four layouts."""
import warnings

import numpy as np
import pytest
import torch

import fbank_oracle as O
import audio_amd.functional as F
import audio_amd.transforms as T

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
BITS = {torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16}


def dtype_id(d):
    return str(d).split(".")[-1]


def tile():
    return F.dense_fbank_tiles()[0]


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(BITS[a.dtype]),
                                                                     b.contiguous().view(BITS[b.dtype]))


# ---- parity -------------------------------------------------------------------------------------------------------------------

def test_tiles():
    assert F.dense_fbank_tiles() == (64, 64, 128, 4097)


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_parity_with_the_oracle(dtype):
    worst = 0.0
    for seed, (K, N, T_, rows) in enumerate(O.dense_cases(tile())):
        fb = O.dense_filterbank(K, N)
        fbd = torch.from_numpy(np.array(fb)).to(DEV)
        x = O.spec_values(rows, K, T_, dtype, seed)
        x64 = x.to(torch.float64).numpy()
        want, bound = O.dense(x64, fb), O.dense_bound(x64, fb, dtype)
        first = None
        for layout in O.LAYOUTS:
            got = F.dense_fbank_scale(O.laid_out(x.to(DEV), layout), fbd)
            assert got.shape == (rows, N, T_) and got.dtype == dtype and got.stride() == (T_ * N, 1, N)
            ratio = O.worst_ratio(got.cpu().to(torch.float64).numpy(), want, bound)
            worst = max(worst, ratio)
            assert ratio <= 1.0, (K, N, T_, rows, layout, ratio)
            if first is None:
                first = got
            else:                                                            # layout and alignment change no bit
                assert same_bits(got, first), (K, N, T_, rows, layout)
    print("dense_fbank %s: largest error / bound %.4f" % (dtype_id(dtype), worst))


@pytest.mark.parametrize("cfg", [(16000, 201, 12), (16000, 65, 24), (44100, 2049, 36)], ids=lambda c: "x".join(map(str, c)))
def test_chroma_scale_against_the_oracle(cfg):
    sr, n_freqs, n_chroma = cfg
    m = T.ChromaScale(sr, n_freqs, n_chroma=n_chroma).to(DEV)
    fb = m.fb.cpu().numpy()
    x = O.spec_values(2, n_freqs, tile() + 1, torch.float32, 7)
    x64 = x.double().numpy()
    got = m(x.to(DEV))
    assert got.shape == (2, n_chroma, tile() + 1) and got.stride() == ((tile() + 1) * n_chroma, 1, n_chroma)
    ratio = O.worst_ratio(got.cpu().double().numpy(), O.dense(x64, fb), O.dense_bound(x64, fb, torch.float32))
    print("ChromaScale %s: largest error / bound %.4f" % (cfg, ratio))
    assert ratio <= 1.0
    assert same_bits(got, F.dense_fbank_scale(x.to(DEV), m.fb))
    # against the chroma DEFINITION in float64 (the builder's rounding included): a loose sanity check of the whole chain
    ref = O.dense(x64, O.chroma(sr, n_freqs, n_chroma))
    assert np.abs(got.cpu().double().numpy() - ref).max() <= 1e-4 * np.abs(ref).max()


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_bits_do_not_depend_on_repetition_batch_or_leading_shape(dtype):
    K, N, T_ = 201, 12, 2 * tile() + 3
    fb = torch.from_numpy(np.array(O.dense_filterbank(K, N))).to(DEV)
    x = O.spec_values(3, K, T_, dtype, 21).to(DEV)
    all3 = F.dense_fbank_scale(x, fb)
    assert same_bits(F.dense_fbank_scale(x, fb), all3)
    for r in range(3):
        one = F.dense_fbank_scale(x[r], fb)                                  # 2-D
        assert one.shape == (N, T_) and one.stride() == (1, N) and same_bits(one, all3[r])
        assert same_bits(F.dense_fbank_scale(x[r:r + 1], fb)[0], all3[r])
    x4 = torch.stack([x[:2], x[1:]])                                         # 4-D (2, 2, K, T)
    got4 = F.dense_fbank_scale(x4, fb)
    assert got4.shape == (2, 2, N, T_) and got4.stride() == (2 * T_ * N, T_ * N, 1, N)
    assert same_bits(got4[0], all3[:2]) and same_bits(got4[1], all3[1:])
    # nor on the tile a frame falls in: a unit-stride slice is read in place, a strided one is gathered first
    assert same_bits(F.dense_fbank_scale(x[:, :, 5:], fb), all3[:, :, 5:])
    assert same_bits(F.dense_fbank_scale(x[:, :, ::2], fb), all3[:, :, ::2])


def test_nan_stays_in_its_frame():
    K, N, T_ = 201, 12, tile() + 6
    fb = torch.from_numpy(np.array(O.dense_filterbank(K, N))).to(DEV)
    x = O.spec_values(2, K, T_, torch.float32, 5).to(DEV)
    clean = F.dense_fbank_scale(x, fb)
    x[1, 77, 66] = float("nan")
    got = F.dense_fbank_scale(x, fb)
    assert torch.isnan(got[1, :, 66]).all()
    keep = torch.ones(2, T_, dtype=torch.bool, device=DEV)
    keep[1, 66] = False
    assert same_bits(got.transpose(1, 2)[keep], clean.transpose(1, 2)[keep])


# ---- the modules against their compositions -------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_fft", [400, 512, 480])
def test_chroma_spectrogram_is_spectrogram_then_chroma_scale(n_fft):
    torch.manual_seed(n_fft)
    x = torch.randn(2, 4000, device=DEV)
    m = T.ChromaSpectrogram(16000, n_fft).to(DEV)
    got = m(x)
    T_ = 1 + 4000 // (n_fft // 2)
    assert got.shape == (2, 12, T_) and got.stride() == (T_ * 12, 1, 12)
    spec = T.Spectrogram(n_fft).to(DEV)(x)
    assert spec.shape == (2, n_fft // 2 + 1, T_) and spec.stride(-2) == 1    # frame-major: read in place
    want = T.ChromaScale(16000, n_fft // 2 + 1).to(DEV)(spec)
    assert same_bits(got, want)
    s64 = spec.cpu().double().numpy()
    fb = m.chroma_scale.fb.cpu().numpy()
    assert O.worst_ratio(got.cpu().double().numpy(), O.dense(s64, fb), O.dense_bound(s64, fb, torch.float32)) <= 1.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=dtype_id)
@pytest.mark.parametrize("scale", O.BARK_SCALES)
def test_bark_spectrogram_is_melspectrogram_with_the_bark_filterbank(scale, dtype):
    torch.manual_seed(3)
    x = torch.randn(2, 4000, device=DEV).to(dtype)
    b = T.BarkSpectrogram(16000, 400, n_barks=40, bark_scale=scale).to(DEV)
    m = T.MelSpectrogram(16000, 400, n_mels=40).to(DEV)
    m.mel_scale.fb.copy_(b.bark_scale.fb)
    got, want = b(x), m(x)
    assert got.shape == (2, 40, 21) and got.dtype == dtype and got.stride() == want.stride()
    assert same_bits(got, want)
    assert float(got.float().abs().max()) > 0


def test_bark_scale_and_inverse_bark_scale():
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        m = T.BarkScale(40, 16000, n_stft=201).to(DEV)
        inv = T.InverseBarkScale(201, 40, 16000).to(DEV)
    spec = O.spec_values(2, 201, tile() + 1, torch.float32, 9).to(DEV)
    bark = m(spec)
    assert bark.shape == (2, 40, tile() + 1) and same_bits(bark, F.mel_scale(spec, m.fb))
    ref = O.dense(spec.cpu().double().numpy(), m.fb.cpu().numpy())
    assert np.abs(bark.cpu().double().numpy() - ref).max() <= 1e-5 * np.abs(ref).max()
    back = inv(bark)
    assert back.shape == spec.shape and same_bits(back, F.inverse_mel_scale(bark, inv.fb)) and bool((back >= 0).all())


# ---- limits and the precision / training path -----------------------------------------------------------------------------------

def test_limits():
    _, _, max_out, max_freqs = F.dense_fbank_tiles()
    g = torch.Generator().manual_seed(1)
    fb = torch.rand(max_freqs, max_out, generator=g)
    x = O.spec_values(1, max_freqs, 5, torch.float32, 13)
    got = F.dense_fbank_scale(x.to(DEV), fb.to(DEV))                         # both limits at once are served
    x64 = x.double().numpy()
    assert got.shape == (1, max_out, 5)
    assert O.worst_ratio(got.cpu().double().numpy(), O.dense(x64, fb.numpy()), O.dense_bound(x64, fb.numpy(), torch.float32)) <= 1.0
    with pytest.raises(NotImplementedError, match="up to 128 outputs"):
        F.dense_fbank_scale(torch.rand(1, 33, 4, device=DEV), torch.rand(33, max_out + 1, device=DEV))
    with pytest.raises(NotImplementedError, match="up to 4097 frequency bins"):
        F.dense_fbank_scale(torch.rand(1, max_freqs + 1, 4, device=DEV), torch.rand(max_freqs + 1, 12, device=DEV))
    m = T.ChromaScale(16000, 33).to(DEV)
    with pytest.raises(ValueError, match=r"expected an input with 33 frequency bins.*Found: 32"):
        m(torch.rand(2, 32, 4, device=DEV))
    with pytest.raises(TypeError):
        m(torch.ones(2, 33, 4, device=DEV, dtype=torch.int64))
    assert m(torch.rand(2, 33, 0, device=DEV)).shape == (2, 12, 0)
    assert m(torch.rand(0, 33, 4, device=DEV)).shape == (0, 12, 4)
    assert m(torch.rand(2, 0, 33, 4, device=DEV)).shape == (2, 0, 12, 4)


def test_float64_and_grad_take_matmul():
    m = T.ChromaScale(16000, 33).to(DEV)
    x = O.spec_values(2, 33, 9, torch.float64, 31).to(DEV)
    got = m(x)
    assert got.dtype == torch.float64 and got.shape == (2, 12, 9)
    want = O.dense(x.cpu().numpy(), m.fb.cpu().numpy())
    assert np.abs(got.cpu().numpy() - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    x32 = x.float().requires_grad_(True)
    got32 = m(x32)
    assert got32.requires_grad and got32.grad_fn is not None
    assert torch.equal(got32.detach(), torch.matmul(x32.detach().transpose(-1, -2), m.fb).transpose(-1, -2))
    with torch.no_grad():                                                    # grad mode off: the kernel
        k = m(x32)
    assert k.grad_fn is None and not k.requires_grad and same_bits(k, m(x32.detach()))
    m.fb.requires_grad_(True)                                                # a learnable filterbank: gradients reach it
    loss = m(x.float()).sum()
    loss.backward()
    assert m.fb.grad is not None and m.fb.grad.shape == m.fb.shape
    m64 = T.ChromaScale(16000, 33).to(DEV).double()
    xg = O.spec_values(1, 33, 3, torch.float64, 33).to(DEV).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda t: m64(t), (xg,), eps=1e-6, atol=1e-6)


# ---- graph capture ------------------------------------------------------------------------------------------------------------

def test_graph_capture():
    x = O.spec_values(2, 201, tile() + 1, torch.float32, 41).to(DEV)
    fresh = T.ChromaScale(16000, 201).to(DEV)                                # its operand image is not on the device yet
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
