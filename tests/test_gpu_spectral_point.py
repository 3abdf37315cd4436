"""LFCC, SpectralCentroid, the mu-law pair, Fade, Vol and their functionals on the device.  The cases and bars of
tests/test_spectral_point.py (spectral_point_cases.py) run through the C ABI at the same small shapes -- the bit-exact ones
bit-exact here too -- then the product API end to end: T.LFCC against the float64 oracle on the three STFT families,
F.spectral_centroid against the float64 oracle of the whole chain with a bound derived from the spectrogram's accepted
error, strided inputs, graph capture, bit-reproducibility, and the conventions (empty tensors, dtypes, gradients)."""
import math
import warnings

import numpy as np
import pytest
import torch

import spectral_point_cases as K
import spectral_point_oracle as O
import audio_amd.functional as F
import audio_amd.transforms as T
from audio_amd import _lib
from conftest import peak_rel_err
from oracle import dsp_oracle as D

pytestmark = pytest.mark.gpu
DEV = "cuda"
CODE = {torch.float32: 0, torch.float64: 1, torch.float16: 2, torch.bfloat16: 3, torch.int64: 4, torch.int32: 5, torch.int16: 6,
        torch.int8: 7, torch.uint8: 8}
TOL_MFCC = 1e-4            # TOL["MFCC"] of tests/test_gpu_parity.py
TOL_SPECTROGRAM = 1e-4     # TOL["Spectrogram"]


def on_device(view):
    """`view` with the same strides and storage offset over a device copy of its whole buffer."""
    base = view._base if view._base is not None else view
    return base.to(DEV).as_strided(tuple(view.shape), view.stride(), view.storage_offset())


class Device:
    """The backend of spectral_point_cases: the C ABI on the device."""

    @staticmethod
    def pointwise(op, x, out_dtype, p0, p1, flag, table, n_in, n_out):
        xd = on_device(x)
        rows, L = x.shape
        out = torch.empty((rows, L), dtype=out_dtype, device=DEV)
        td = None if table is None else table.to(DEV)
        _lib.check(_lib.lib().aamd_pointwise(op, CODE[x.dtype], xd.data_ptr(), out.data_ptr(), rows, L, x.stride(0), p0, p1, flag,
                                             0 if td is None else td.data_ptr(), n_in, n_out, _lib.current_stream(out.device)))
        return out.cpu()

    @staticmethod
    def centroid(m3, freqs, out_dtype):
        md, fd = on_device(m3), freqs.to(DEV)
        rows, frames, n_freq = m3.shape
        out = torch.empty((rows, frames), dtype=out_dtype, device=DEV)
        _lib.check(_lib.lib().aamd_spectral_centroid(CODE[out_dtype], md.data_ptr(), fd.data_ptr(), out.data_ptr(), rows, frames,
                                                     n_freq, m3.stride(0), m3.stride(1), m3.stride(2),
                                                     _lib.current_stream(out.device)))
        return out.cpu()


# ---- 1. the cases of the CPU replay, through the C ABI -------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["lines", "time"])
@pytest.mark.parametrize("n_freq", K.N_FREQS)
def test_centroid_within_one_ulp_of_float64_sums(n_freq, layout):
    for frames in K.N_FRAMES:
        for rows in K.N_ROWS:
            K.check_centroid(Device, n_freq, frames, rows, layout)


@pytest.mark.parametrize("out_dtype", [torch.float16, torch.bfloat16], ids=str)
def test_centroid_rounds_once_to_the_output_type(out_dtype):
    for n_freq in (33, 201):
        K.check_centroid(Device, n_freq, 65, 3, "lines", out_dtype)


@pytest.mark.parametrize("layout", ["lines", "time"])
def test_centroid_zero_and_nan_frames(layout):
    K.check_centroid_zero_and_nan_frames(Device, layout)


@pytest.mark.parametrize("layout", K.LAYOUTS)
@pytest.mark.parametrize("dtype", K.FLOATS, ids=str)
def test_scale_gain_and_vol_are_bit_exact(dtype, layout):
    for L in K.LENGTHS + (4099,):
        K.check_scale(Device, dtype, L, layout)


@pytest.mark.parametrize("shape", O.SHAPES)
@pytest.mark.parametrize("dtype", K.FLOATS, ids=str)
def test_fade_is_the_table_times_x_and_bit_copies_elsewhere(dtype, shape):
    for L in K.LENGTHS:
        for layout in K.LAYOUTS:
            K.check_fade(Device, dtype, L, layout, shape)
    K.check_fade(Device, dtype, 4099, "offset", shape)


@pytest.mark.parametrize("layout", K.LAYOUTS)
@pytest.mark.parametrize("dtype", K.FLOATS, ids=str)
def test_contrast_within_4x_the_definitions_own_error(dtype, layout):
    K.check_contrast(Device, dtype, layout)
    K.check_contrast(Device, dtype, layout, (1025,), amount=0.0)
    K.check_contrast(Device, dtype, layout, (1025,), amount=100.0)


@pytest.mark.parametrize("layout", K.LAYOUTS)
@pytest.mark.parametrize("dtype", K.FLOATS, ids=str)
def test_db_to_amplitude_within_4x_the_definitions_own_error(dtype, layout):
    K.check_db_to_amplitude(Device, dtype, layout)
    K.check_db_to_amplitude(Device, dtype, layout, (1025,), ref=0.5, power=1.0)


@pytest.mark.parametrize("layout", K.LAYOUTS)
@pytest.mark.parametrize("dtype", K.FLOATS + (torch.int64, torch.int32, torch.uint8), ids=str)
def test_mu_law_decoding_within_4x_the_definitions_own_error(dtype, layout):
    K.check_mu_decode(Device, dtype, 256, layout)
    # (two channels have two codes, both decoded exactly in every precision: they give no yardstick, see the exact cases)
    for q in (16,) + ((1024,) if dtype not in (torch.uint8,) else ()):
        K.check_mu_decode(Device, dtype, q, layout, (1025,))


@pytest.mark.parametrize("dtype", [torch.int16, torch.int8], ids=str)
def test_mu_law_decoding_reads_the_narrow_integer_types(dtype):
    K.check_mu_decode(Device, dtype, 128, "offset", (1025,))


@pytest.mark.parametrize("q", [2, 16, 256, 1024])
@pytest.mark.parametrize("dtype", K.FLOATS, ids=str)
def test_mu_law_encoding_equals_the_float64_codes_outside_the_band(dtype, q):
    for L in K.LENGTHS + (4099,):
        for layout in K.LAYOUTS:
            K.check_mu_encode(Device, dtype, q, L, layout)


@pytest.mark.parametrize("q", [2, 16, 256, 1024])
@pytest.mark.parametrize("dtype", K.FLOATS, ids=str)
def test_mu_law_exact_cases_and_round_trip(dtype, q):
    K.check_mu_exact_and_round_trip(Device, dtype, q)


def test_tiles_are_the_kernels_constants():
    assert F.spectral_tiles() == (256, 4, 64) and F.pointwise_tiles() == (256, 4096, 4)
    assert [_lib.lib().aamd_spectral_lanes(n) for n in (0, 1, 5, 33, 201, 4097)] == [0, 1, 1, 4, 16, 64]


# ---- 2. T.LFCC end to end ----------------------------------------------------------------------------------------------------------

def two_tones(rows=3, n=4000, seed=0):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 16000.0
    x = (0.4 * np.sin(2 * np.pi * 440 * t) + 0.2 * np.sin(2 * np.pi * 3100 * t))[None, :] + 0.05 * rng.standard_normal((rows, n))
    return x.astype(np.float32)


@pytest.mark.parametrize("log_lf", [False, True])
@pytest.mark.parametrize("n_fft", [400, 512, 480])
def test_lfcc_against_the_float64_oracle(n_fft, log_lf):
    x = two_tones()
    m = T.LFCC(log_lf=log_lf, speckwargs=dict(n_fft=n_fft, hop_length=n_fft // 4))
    want = D.mfcc(x, m.Spectrogram.window.numpy(), m.filter_mat.numpy(), m.dct_mat.numpy(), n_fft, n_fft // 4, log_mels=log_lf)
    m = m.to(DEV)
    got = m(torch.from_numpy(x).to(DEV))
    assert got.dtype == torch.float32 and tuple(got.shape) == want.shape == (3, 40, 1 + 4000 // (n_fft // 4))
    err = peak_rel_err(got.cpu().numpy(), want)
    print("LFCC n_fft=%d log_lf=%s: peak-relative error %.3e" % (n_fft, log_lf, err))
    assert err <= TOL_MFCC
    assert torch.equal(m(torch.from_numpy(x).to(DEV)), got)
    xh = torch.from_numpy(x).half()
    half = m(xh.to(DEV))
    assert half.dtype == torch.float16 and half.shape == got.shape
    m = m.cpu()
    want_h = D.mfcc(xh.double().numpy(), m.Spectrogram.window.numpy(), m.filter_mat.numpy(), m.dct_mat.numpy(), n_fft, n_fft // 4,
                    log_mels=log_lf)
    assert peak_rel_err(half.float().cpu().numpy(), want_h) <= TOL_MFCC + 2.0 ** -11    # float32 arithmetic, one rounding to half


@pytest.mark.parametrize("log_lf", [False, True])
def test_lfcc_gradient_equals_the_torch_compositions(log_lf):
    m = T.LFCC(log_lf=log_lf).to(DEV)
    x = torch.from_numpy(two_tones(2, 2000, 1)).to(DEV).requires_grad_(True)
    w = torch.from_numpy(np.random.default_rng(2).standard_normal((2, 40, 11)).astype(np.float32)).to(DEV)
    out = m(x)
    assert out.requires_grad and tuple(out.shape) == (2, 40, 11)
    (g,) = torch.autograd.grad((out * w).sum(), x)
    x2 = x.detach().clone().requires_grad_(True)
    spec = m.Spectrogram(x2)
    fbs = torch.matmul(spec.transpose(-1, -2), m.filter_mat).transpose(-1, -2)
    fbs = torch.log(fbs + 1e-6) if log_lf else m.amplitude_to_DB(fbs)
    ref = torch.matmul(fbs.transpose(-1, -2), m.dct_mat).transpose(-1, -2)
    (g2,) = torch.autograd.grad((ref * w).sum(), x2)
    assert torch.isfinite(g).all() and float(g.abs().max()) > 0
    # the same differentiable spectrogram and the same torch ops behind it: float32 rounding of re-ordered sums at the most
    assert peak_rel_err(out.detach().cpu().numpy(), ref.detach().cpu().numpy()) <= 8 * 2.0 ** -24
    assert peak_rel_err(g.cpu().numpy(), g2.cpu().numpy()) <= 8 * 2.0 ** -24
    x64 = x.detach().double()
    assert m.double()(x64).dtype == torch.float64


# ---- 3. F.spectral_centroid end to end ---------------------------------------------------------------------------------------------

def centroid_oracle(x, sample_rate, n_fft, hop):
    """float64 oracle of the whole chain and the per-frame bound: the project accepts a magnitude error of eps = 1e-4 of the
    call's peak, so |got - want| <= eps * peak * sum_k |f_k - want| / sum_k m_k."""
    mag = D.spectrogram(x.astype(np.float64), 0, D.hann_window(n_fft), n_fft, hop, n_fft, 1.0, False)      # (rows, F, T)
    f = O.centroid_freqs(sample_rate, n_fft).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        want = (f[:, None] * mag).sum(-2) / mag.sum(-2)
        bound = TOL_SPECTROGRAM * mag.max() * np.abs(f[None, :, None] - want[:, None, :]).sum(-2) / mag.sum(-2)
    return want, bound


@pytest.mark.parametrize("n_fft", [400, 512, 480])
def test_spectral_centroid_against_the_float64_oracle_of_the_chain(n_fft):
    x = two_tones()
    x[1] = 0.0                                           # a row of silence: NaN in every frame
    hop = n_fft // 2
    want, bound = centroid_oracle(x, 16000, n_fft, hop)
    xd = torch.from_numpy(x).to(DEV)
    m = T.SpectralCentroid(16000, n_fft=n_fft).to(DEV)
    got = m(xd)
    assert got.dtype == torch.float32 and tuple(got.shape) == want.shape == (3, 1 + 4000 // hop)
    g = got.cpu().numpy()
    assert np.isnan(g[1]).all() and np.isnan(want[1]).all() and not np.isnan(g[[0, 2]]).any()
    ratio = np.abs(g[[0, 2]] - want[[0, 2]]) / bound[[0, 2]]
    print("spectral_centroid n_fft=%d: largest error / bound %.3e, largest error %.3e Hz" % (n_fft, ratio.max(),
                                                                                             np.abs(g[[0, 2]] - want[[0, 2]]).max()))
    assert (ratio <= 1).all()
    again = F.spectral_centroid(xd, 16000, 0, m.window, n_fft, hop, n_fft)
    assert torch.equal(again.view(torch.int32), got.view(torch.int32))                  # two calls, the same bits (NaN included)
    spec = T.Spectrogram(n_fft=n_fft, power=1.0).to(DEV)(xd)
    assert spec.stride()[-2:] == (1, n_fft // 2 + 1)                                    # frame-major memory
    alone = F._centroid_reduce(spec, torch.from_numpy(O.centroid_freqs(16000, n_fft)).to(DEV))
    assert torch.equal(alone.view(torch.int32), got.view(torch.int32))
    both = F._centroid_reduce(spec.contiguous(), torch.from_numpy(O.centroid_freqs(16000, n_fft)).to(DEV))       # time-contiguous
    assert np.array_equal(np.isnan(both.cpu().numpy()), np.isnan(g))
    assert (np.abs(both.cpu().numpy()[[0, 2]] - g[[0, 2]]) <= O.ulp32(g[[0, 2]])).all()


def test_spectral_centroid_dtypes_gradient_and_empty():
    x = two_tones(2, 3000, 3)
    xd = torch.from_numpy(x).to(DEV)
    w = torch.hann_window(400, device=DEV)
    ref = F.spectral_centroid(xd, 16000, 0, w, 400, 200, 400)
    want, bound = centroid_oracle(x, 16000, 400, 200)
    for dt in (torch.float16, torch.bfloat16):
        got = F.spectral_centroid(xd.to(dt), 16000, 0, w, 400, 200, 400)
        assert got.dtype == dt and got.shape == ref.shape
        wq, bq = centroid_oracle(xd.to(dt).double().cpu().numpy(), 16000, 400, 200)
        assert (np.abs(got.double().cpu().numpy() - wq) <= bq + O.half_ulp(wq, dt)).all()
    got64 = F.spectral_centroid(xd.double(), 16000, 0, w.double(), 400, 200, 400)
    assert got64.dtype == torch.float64 and (np.abs(got64.cpu().numpy() - want) <= 1e-6 * np.abs(want)).all()
    xg = xd.clone().requires_grad_(True)
    out = F.spectral_centroid(xg, 16000, 0, w, 400, 200, 400)
    assert out.requires_grad and (np.abs(out.detach().cpu().numpy() - want) <= bound).all()
    (g,) = torch.autograd.grad(out.sum(), xg)
    assert torch.isfinite(g).all() and float(g.abs().max()) > 0
    with torch.no_grad():
        assert torch.equal(F.spectral_centroid(xg, 16000, 0, w, 400, 200, 400), ref)
    empty = F.spectral_centroid(xd[:0], 16000, 0, w, 400, 200, 400)
    assert tuple(empty.shape) == (0, 16) and empty.dtype == torch.float32
    one = F.spectral_centroid(xd[0], 16000, 0, w, 400, 200, 400)
    assert torch.equal(one, ref[0])
    four = F.spectral_centroid(xd.view(2, 1, 3000), 16000, 0, w, 400, 200, 400)
    assert torch.equal(four, ref.view(2, 1, 16))


def test_spectral_centroid_and_fade_in_a_graph():
    x = torch.from_numpy(two_tones(3, 4000, 4)).to(DEV)
    m = T.SpectralCentroid(22050, n_fft=512).to(DEV)      # a table no other test has put on the device
    fade = T.Fade(37, 41, "half_sine")
    T.Spectrogram(n_fft=512, power=1.0).to(DEV)(x)       # the transform's own constants are on the device
    torch.cuda.synchronize()
    for fn in (m, fade):
        graph = torch.cuda.CUDAGraph()
        with pytest.raises(RuntimeError, match="run the call once eagerly"):
            with torch.cuda.graph(graph):
                doubled = x * 2                          # the capture is not empty
                fn(doubled)
        torch.cuda.synchronize()
    want_c, want_f = m(x), fade(x)                       # once eagerly
    static = x.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_c = m(static)
        out_f = fade(static)
    static.copy_(x)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out_c, want_c) and torch.equal(out_f, want_f)
    static.copy_(x * 0.5 + 0.01)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out_c, m(static)) and torch.equal(out_f, fade(static))


# ---- 4. strided inputs and the product API of the pointwise ops -----------------------------------------------------------------------

def test_every_other_row_of_a_wider_tensor_gives_the_bits_of_its_contiguous_copy():
    rng = np.random.default_rng(6)
    wide = torch.from_numpy(rng.uniform(-1, 1, (2, 6, 1025)).astype(np.float32)).to(DEV)
    x = wide[:, ::2]
    assert tuple(x.shape) == (2, 3, 1025) and not x.is_contiguous()
    xc = x.contiguous()
    w = torch.hann_window(400, device=DEV)
    for fn in (F.contrast, lambda t: F.mu_law_encoding(t, 256), T.Fade(100, 300, "logarithmic"),
               lambda t: F.spectral_centroid(t, 16000, 0, w, 400, 200, 400)):
        a, b = fn(x), fn(xc)
        assert a.shape == b.shape and a.is_contiguous() and torch.equal(a, b) and a.shape[:2] == (2, 3)
    t = wide.transpose(-1, -2)[:, :1000, :]              # a non-unit sample stride is gathered first
    assert torch.equal(F.contrast(t), F.contrast(t.contiguous()))


def test_product_api_of_the_pointwise_ops():
    rng = np.random.default_rng(7)
    xn = rng.uniform(-1.2, 1.2, (2, 3, 777)).astype(np.float32)
    x = torch.from_numpy(xn).to(DEV)
    assert F.gain(x, 0) is x
    K.assert_same_bits(F.gain(x, -2.5).cpu(), torch.from_numpy(O.scale(xn, O.ratio_of_db(-2.5), False, np.float32)))
    K.assert_same_bits(F.gain(x).cpu(), torch.from_numpy(O.scale(xn, O.ratio_of_db(1.0), False, np.float32)))
    for gain, kind, ratio in ((0.8, "amplitude", 0.8), (4.0, "db", O.ratio_of_db(4.0)), (-4.0, "db", O.ratio_of_db(-4.0)),
                              (1.7, "power", O.ratio_of_db(10 * math.log10(1.7))), (0.0, "db", 1.0)):
        K.assert_same_bits(T.Vol(gain, kind)(x).cpu(), torch.from_numpy(O.scale(xn, ratio, True, np.float32)), (gain, kind))
    x64 = x.double()
    K.assert_same_bits(T.Vol(1.3)(x64).cpu(), torch.from_numpy(O.scale(xn.astype(np.float64), 1.3, True, np.float64)))
    codes = T.MuLawEncoding()(x.clamp(-1, 1))
    assert codes.dtype == torch.int64 and codes.shape == x.shape and int(codes.min()) >= 0 and int(codes.max()) <= 255
    back = T.MuLawDecoding()(codes)
    assert back.dtype == torch.float32 and float((back - x.clamp(-1, 1)).abs().max()) < 0.05
    assert torch.equal(T.MuLawDecoding()(codes.to(torch.uint8)), back) and torch.equal(F.mu_law_decoding(codes.int(), 256), back)
    assert F.mu_law_decoding(codes.half(), 256).dtype == torch.float16
    with pytest.warns(UserWarning, match="floating type"):
        ci = F.mu_law_encoding(torch.tensor([-1, 0, 1], device=DEV), 256)
    assert ci.tolist() == [0, 128, 255]
    amp = F.DB_to_amplitude(torch.tensor([-20.0, 0.0, 20.0], device=DEV), 1.0, 0.5)
    assert np.allclose(amp.cpu().numpy(), [0.1, 1.0, 10.0], rtol=1e-6)
    assert F.contrast(x[0, 0, 0]).shape == () and F.gain(x[0, 0, 0], 3.0).shape == ()
    for fn in (lambda t: F.gain(t, 3.0), F.contrast, lambda t: F.DB_to_amplitude(t, 1.0, 1.0), lambda t: F.mu_law_encoding(t, 16),
               lambda t: F.mu_law_decoding(t, 16), T.Fade(0, 0), T.Vol(0.5)):
        for shape in ((0,), (3, 0), (0, 5)):
            e = fn(torch.zeros(shape, device=DEV))
            assert tuple(e.shape) == shape
    with pytest.raises(ValueError, match="longer than the signal"):
        T.Fade(778, 0)(x)
    assert torch.equal(T.Fade(0, 0)(x), x) and T.Fade(0, 0)(x) is not x


def test_an_input_that_requires_grad_takes_the_torch_expression():
    rng = np.random.default_rng(8)
    x = torch.from_numpy(rng.uniform(-1, 1, (2, 500)).astype(np.float32)).to(DEV)
    for fn, tol in ((lambda t: F.gain(t, 3.0), 0.0), (T.Vol(1.5), 0.0), (F.contrast, 1e-6), (T.Fade(50, 60, "exponential"), 1e-7),
                    (lambda t: F.DB_to_amplitude(t * 20, 1.0, 0.5), 1e-5)):
        with torch.no_grad():
            want = fn(x)
        xg = x.clone().requires_grad_(True)
        out = fn(xg)
        assert out.requires_grad and float((out.detach() - want).abs().max()) <= tol * max(1.0, float(want.abs().max()))
        (g,) = torch.autograd.grad(out.sum(), xg)
        assert torch.isfinite(g).all() and g.shape == x.shape
    codes = torch.from_numpy(rng.uniform(0, 255, (2, 500)).astype(np.float32)).to(DEV).requires_grad_(True)
    out = F.mu_law_decoding(codes, 256)
    (g,) = torch.autograd.grad(out.sum(), codes)
    assert out.requires_grad and torch.isfinite(g).all() and float(g.min()) > 0
    enc = F.mu_law_encoding(x.clone().requires_grad_(True), 256)          # an integer result: no gradient
    assert enc.dtype == torch.int64 and not enc.requires_grad
