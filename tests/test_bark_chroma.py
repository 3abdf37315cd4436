"""Bark and chroma spectrograms without a GPU: the filterbank builders against the float64 definition (tests/fbank_oracle.py)
with the definition's own float32 evaluation as the yardstick, the structure of the chroma filterbank, a CPU replay of
csrc/dense_fbank.h (both layouts, dense and misaligned, the three storage types, frame counts around the tile, 1 - 3 rows)
against the float64 product of the stored operands within the issue's bound, signatures, names, error types and the refusal of
CPU tensors."""
import ctypes as C
import inspect
import os
import subprocess
import warnings

import numpy as np
import pytest
import torch

import fbank_oracle as O
import audio_amd.functional as F
import audio_amd.transforms as T
import audio_amd.prototype.functional as PF
import audio_amd.prototype.transforms as PT
from audio_amd import _host

HERE = os.path.dirname(os.path.abspath(__file__))
SIM_SRC = os.path.join(HERE, "cpu_sim", "sim_dense_fbank.cpp")
SIM_OUT = os.path.join(HERE, "cpu_sim", "_build", "libaamd_sim_dense_fbank.so")
HDRS = [os.path.join(os.path.dirname(HERE), "audio_amd", "csrc", h) for h in ("dense_fbank.h", "wave_augment.h",
                                                                              "spec_augment.h", "hd.h")]
CODE = {torch.float32: 0, torch.float16: 2, torch.bfloat16: 3}
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
BITS = {torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16}

_sim = None


def sim():
    global _sim
    if _sim is None:
        newest = max(os.path.getmtime(p) for p in [SIM_SRC] + HDRS)
        if not os.path.exists(SIM_OUT) or newest > os.path.getmtime(SIM_OUT):
            os.makedirs(os.path.dirname(SIM_OUT), exist_ok=True)
            tmp = "%s.tmp.%d" % (SIM_OUT, os.getpid())
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", SIM_SRC, "-o", tmp])
            os.replace(tmp, SIM_OUT)
        _sim = C.CDLL(SIM_OUT)
        i64, i32, p = C.c_int64, C.c_int, C.c_void_p
        _sim.sim_dfb.argtypes = [i32, p, p, p, i64, i64, i64, i64, i64, i32, i32]
        _sim.sim_dfb_lds_bytes.restype = i64
    return _sim


def sim_dense(x, fb32):
    """x: a (rows, K, T) CPU view with unit stride along freq or time; returns (rows, N, T) of x's dtype."""
    rows, K, T_ = x.shape
    sr, sk, st = x.stride()
    sk, st = (1 if K == 1 else sk), (1 if T_ == 1 else st)
    assert sk == 1 or st == 1
    N = fb32.shape[1]
    out = torch.full((rows, T_, N), float("nan"), dtype=x.dtype)
    frag = torch.from_numpy(_host.dense_fbank_fragments(fb32))           # (torch's allocations are 64-byte aligned)
    assert frag.data_ptr() % 16 == 0 and frag.numel() == (K + 3) // 4 * ((N + 15) // 16) * 64
    assert sim().sim_dfb(CODE[x.dtype], x.data_ptr(), frag.data_ptr(), out.data_ptr(), rows, T_, sr, sk, st, K, N) == 0
    return out.transpose(1, 2)


def bits(t):
    return t.contiguous().view(BITS[t.dtype])


# ---- the builders -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scale", O.BARK_SCALES)
@pytest.mark.parametrize("cfg", O.BARK_CONFIGS, ids=lambda c: "x".join(map(str, c)))
def test_bark_builder_against_the_definition(cfg, scale):
    n_freqs, n_barks, sr = cfg
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                  # none of these has an all-zero filter
        fb = F.barkscale_fbanks(n_freqs, 0.0, sr / 2, n_barks, sr, scale)
    assert fb.dtype == torch.float32 and fb.shape == (n_freqs, n_barks) and fb.is_contiguous()
    f64 = O.barkscale_fbanks(n_freqs, 0.0, sr / 2, n_barks, sr, scale)
    f32 = O.barkscale_fbanks(n_freqs, 0.0, sr / 2, n_barks, sr, scale, np.float32)
    assert (f64.max(axis=0) > 0).all()
    ratio = O.builder_ratio(fb.numpy(), f64, f32)
    print("bark %s %s: builder error / the float32 definition's %.3f" % (cfg, scale, ratio))
    assert ratio <= O.MARGIN
    # the triangles: non-negative, at most 1, and banded (one run of non-zeros per filter)
    a = fb.numpy()
    assert (a >= 0).all() and (a <= 1).all()
    for j in range(n_barks):
        nz = np.flatnonzero(a[:, j])
        assert nz.size and nz[-1] - nz[0] + 1 == nz.size


def test_bark_defaults_warn_and_unknown_scales_raise():
    counts = []
    for scale in O.BARK_SCALES:
        with pytest.warns(UserWarning, match=r"At least one bark filterbank has all zero values.*n_barks.*\(128\).*n_freqs.*\(201\)"):
            fb = F.barkscale_fbanks(201, 0.0, 8000.0, 128, 16000, scale)
        f64 = O.barkscale_fbanks(201, 0.0, 8000.0, 128, 16000, scale)
        assert int((fb.numpy().max(axis=0) == 0).sum()) == int((f64.max(axis=0) == 0).sum())
        counts.append(int((f64.max(axis=0) == 0).sum()))
    assert sorted(counts) == [4, 5, 6], counts
    for bad in ("htk", "slaney", "", "Wang"):
        with pytest.raises(ValueError, match="bark_scale should be one of"):
            F.barkscale_fbanks(201, 0.0, 8000.0, 40, 16000, bad)
        with pytest.raises(ValueError, match="bark_scale should be one of"):
            T.BarkScale(40, bark_scale=bad)


@pytest.mark.parametrize("scale", O.BARK_SCALES)
def test_hz_inverts_bark(scale):
    f = np.linspace(0.0, 22000.0, 4401)
    back = O.hz(O.bark(f, scale), scale)
    assert np.abs(back[1:] - f[1:]).max() <= 1e-9 * 22000.0 and (np.abs(back[1:] / f[1:] - 1) <= 1e-9).all() and abs(back[0]) <= 1e-9
    # the host's pair, float32 torch for hz and Python floats for bark: the same functions
    b = np.array([_host._hz_to_bark(float(v), scale) for v in f])
    assert np.abs(b - O.bark(f, scale)).max() <= 1e-12 * 30
    h = _host._bark_to_hz(torch.from_numpy(O.bark(f, scale)), scale).numpy()
    assert np.abs(h[1:] / f[1:] - 1).max() <= 1e-9


@pytest.mark.parametrize("cfg", O.CHROMA_CONFIGS, ids=lambda c: "%d-%d-%d-%s" % (c[0], c[1], c[2], ",".join(c[3]) or "defaults"))
def test_chroma_builder_against_the_definition(cfg):
    sr, n_freqs, n_chroma, kw = cfg
    fb = F.chroma_filterbank(sr, n_freqs, n_chroma, **kw)
    assert fb.dtype == torch.float32 and fb.shape == (n_freqs, n_chroma) and fb.is_contiguous()
    f64, f32 = O.chroma(sr, n_freqs, n_chroma, **kw), O.chroma(sr, n_freqs, n_chroma, dt=np.float32, **kw)
    ratio = O.builder_ratio(fb.numpy(), f64, f32)
    print("chroma %s: builder error / the float32 definition's %.3f; non-zero share %.3f"
          % (cfg, ratio, float((fb != 0).float().mean())))
    assert ratio <= O.MARGIN


def test_chroma_is_dense_with_the_defaults():
    fb = F.chroma_filterbank(16000, 201, 12)
    assert float((fb != 0).float().mean()) >= 0.95                      # no band to walk: the banded kernels do not apply


def test_chroma_odd_n_chroma_shape_and_norms():
    fb = F.chroma_filterbank(16000, 201, 13, octwidth=None)
    assert fb.shape == (201, 13) and torch.isfinite(fb).all()
    assert (fb.double().norm(p=2, dim=1) - 1).abs().max() <= 1e-6
    assert torch.isfinite(F.chroma_filterbank(16000, 201, 13)).all()


@pytest.mark.parametrize("norm", [1, 2, 3, float("inf")])
def test_chroma_rows_have_unit_norm_without_the_octave_weight(norm):
    for sr, n_freqs, n_chroma in [(16000, 201, 12), (16000, 65, 24), (8000, 5, 12)]:
        fb = F.chroma_filterbank(sr, n_freqs, n_chroma, octwidth=None, norm=norm)
        assert (fb.double().norm(p=norm, dim=1) - 1).abs().max() <= 1e-6


def test_chroma_base_c_is_the_column_roll():
    for n_chroma in (12, 24, 36, 13):
        a = F.chroma_filterbank(16000, 201, n_chroma, base_c=False)
        c = F.chroma_filterbank(16000, 201, n_chroma, base_c=True)
        assert torch.equal(c, torch.roll(a, -3 * (n_chroma // 12), dims=1))


def test_chroma_errors():
    with pytest.raises(ValueError, match="n_freqs must be at least 2"):
        F.chroma_filterbank(16000, 1, 12)
    with pytest.raises(ValueError, match="n_chroma must be at least 1"):
        F.chroma_filterbank(16000, 201, 0)
    for bad in (0, -1, -2.5):
        with pytest.raises(ValueError, match="norm must be positive"):
            F.chroma_filterbank(16000, 201, 12, norm=bad)
    with pytest.raises(ValueError, match="needs a real power"):
        T.ChromaSpectrogram(16000, 400, power=None)


# ---- the CPU replay of csrc/dense_fbank.h -----------------------------------------------------------------------------------

def test_operand_image_is_the_kernels_order():
    fb = O.dense_filterbank(33, 17)
    frag = _host.dense_fbank_fragments(fb)
    NT = 2
    assert frag.dtype == np.float32 and frag.shape == (36 // 4 * NT * 64,)
    for k in range(36):
        for n in range(32):
            want = fb[k, n] if k < 33 and n < 17 else 0.0
            assert frag[((k // 4) * NT + n // 16) * 64 + (k % 4) * 16 + n % 16] == want


def test_tiles_are_the_sims_constants_and_lds_fits():
    tiles = tuple(sim().sim_dfb_tiles(i) for i in range(4))
    assert tiles == (64, 64, 128, 4097)
    assert sim().sim_dfb_lds_bytes(12) == 20 * 1024 and sim().sim_dfb_lds_bytes(128) == 48 * 1024
    lib = os.path.join(os.path.dirname(HERE), "audio_amd", "lib", "libaudio_amd.so")
    if os.path.exists(lib):                                             # (the library loads without a GPU)
        assert F.dense_fbank_tiles() == tiles


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_replay_matches_the_float64_product_within_the_bound(dtype):
    worst, share = 0.0, 0.0
    for seed, (K, N, T_, rows) in enumerate(O.dense_cases(sim().sim_dfb_tiles(0))):
        fb = O.dense_filterbank(K, N)
        x = O.spec_values(rows, K, T_, dtype, seed)
        x64 = x.to(torch.float64).numpy()
        want, bound = O.dense(x64, fb), O.dense_bound(x64, fb, dtype)
        first = None
        for layout in O.LAYOUTS:
            got = sim_dense(O.laid_out(x, layout), fb)
            assert got.shape == (rows, N, T_) and got.dtype == dtype and got.stride() == (T_ * N, 1, N)
            ratio = O.worst_ratio(got.to(torch.float64).numpy(), want, bound)
            worst = max(worst, ratio)
            assert ratio <= 1.0, (K, N, T_, rows, layout, ratio)
            if first is None:
                first = bits(got)
            else:                                                          # layout and alignment change no bit
                assert torch.equal(bits(got), first), (K, N, T_, rows, layout)
    print("dense_fbank replay %s: largest error / bound %.4f" % (dtype, worst))


def test_replay_is_the_k_ordered_fmaf_chain():
    """One accumulator per output, products in ascending k: the bits of a float32 fmaf chain written out here (float64
    products of float32 values are exact, so each step is one rounding)."""
    K, N, T_ = 201, 12, 5
    fb = O.dense_filterbank(K, N)
    x = O.spec_values(1, K, T_, torch.float32, 3)
    got = sim_dense(x, fb)[0].numpy()
    acc = np.zeros((N, T_), dtype=np.float32)
    xs = x[0].numpy()
    for k in range(K):
        acc = (fb[k].astype(np.float64)[:, None] * xs[k].astype(np.float64)[None, :] + acc.astype(np.float64)).astype(np.float32)
    assert np.array_equal(got.view(np.int32), acc.view(np.int32))


def test_replay_rows_do_not_depend_on_the_batch():
    K, N = 257, 17
    fb = O.dense_filterbank(K, N)
    x = O.spec_values(3, K, 70, torch.float32, 11)
    all3 = sim_dense(x, fb)
    for r in range(3):
        assert torch.equal(bits(sim_dense(x[r:r + 1].contiguous(), fb)[0]), bits(all3[r]))
    # nor on the tile a frame falls in
    assert torch.equal(bits(sim_dense(x[:, :, 3:].contiguous(), fb)), bits(all3[:, :, 3:]))


@pytest.mark.parametrize("layout", O.LAYOUTS)
def test_replay_nan_stays_in_its_frame(layout):
    K, N, T_ = 201, 12, 70
    fb = O.dense_filterbank(K, N)
    x = O.spec_values(2, K, T_, torch.float32, 5)
    v = O.laid_out(x, layout)
    clean = sim_dense(v, fb)
    v[1, 77, 66] = float("nan")
    v[0, 200, 0] = float("inf")
    got = sim_dense(v, fb)
    assert torch.isnan(got[1, :, 66]).all() and not torch.isfinite(got[0, :, 0]).any()
    keep = torch.ones(2, T_, dtype=torch.bool)
    keep[1, 66] = keep[0, 0] = False
    assert torch.equal(bits(got.transpose(1, 2)[keep]), bits(clean.transpose(1, 2)[keep]))


def test_replay_refuses_what_the_abi_refuses():
    fb = O.dense_filterbank(5, 1)
    frag = torch.from_numpy(_host.dense_fbank_fragments(fb))
    x = torch.rand(1, 5, 3, dtype=torch.float64)
    out = torch.zeros(1, 3, 1, dtype=torch.float64)
    for code in (1, 4, -1):                                              # float64 takes the torch composition
        assert sim().sim_dfb(code, x.data_ptr(), frag.data_ptr(), out.data_ptr(), 1, 3, 15, 3, 1, 5, 1) == -1
    assert sim().sim_dfb(0, x.data_ptr(), frag.data_ptr(), out.data_ptr(), 1, 3, 15, 3, 1, 4098, 1) == -3
    assert sim().sim_dfb(0, x.data_ptr(), frag.data_ptr(), out.data_ptr(), 1, 3, 15, 3, 1, 5, 129) == -3
    assert not out.any()


# ---- the surface ------------------------------------------------------------------------------------------------------------

def params(fn):
    return [(k, v.default) for k, v in inspect.signature(fn).parameters.items() if k != "self"]


def kinds(fn):
    return [v.kind for k, v in inspect.signature(fn).parameters.items() if k != "self"]


def test_signatures():
    E, KW, PK = inspect.Parameter.empty, inspect.Parameter.KEYWORD_ONLY, inspect.Parameter.POSITIONAL_OR_KEYWORD
    hann = torch.hann_window
    assert params(F.barkscale_fbanks) == [("n_freqs", E), ("f_min", E), ("f_max", E), ("n_barks", E), ("sample_rate", E),
                                          ("bark_scale", "traunmuller")]
    chroma_kw = [("tuning", 0.0), ("ctroct", 5.0), ("octwidth", 2.0), ("norm", 2), ("base_c", True)]
    assert params(F.chroma_filterbank) == [("sample_rate", E), ("n_freqs", E), ("n_chroma", E)] + chroma_kw
    assert kinds(F.chroma_filterbank) == [PK] * 3 + [KW] * 5
    assert params(F.dense_fbank_scale) == [("specgram", E), ("fb", E)]
    assert params(F.dense_fbank_tiles) == []
    assert params(T.BarkScale.__init__) == [("n_barks", 128), ("sample_rate", 16000), ("f_min", 0.0), ("f_max", None),
                                            ("n_stft", 201), ("bark_scale", "traunmuller")]
    assert params(T.BarkSpectrogram.__init__) == [
        ("sample_rate", 16000), ("n_fft", 400), ("win_length", None), ("hop_length", None), ("f_min", 0.0), ("f_max", None),
        ("pad", 0), ("n_barks", 128), ("window_fn", hann), ("power", 2.0), ("normalized", False), ("wkwargs", None),
        ("center", True), ("pad_mode", "reflect"), ("bark_scale", "traunmuller")]
    assert params(T.InverseBarkScale.__init__) == [
        ("n_stft", E), ("n_barks", 128), ("sample_rate", 16000), ("f_min", 0.0), ("f_max", None), ("max_iter", 100000),
        ("tolerance_loss", 1e-5), ("tolerance_change", 1e-8), ("sgdargs", None), ("bark_scale", "traunmuller")]
    assert params(T.ChromaScale.__init__) == [("sample_rate", E), ("n_freqs", E), ("n_chroma", 12)] + chroma_kw
    assert kinds(T.ChromaScale.__init__) == [PK] * 2 + [KW] * 6
    assert params(T.ChromaSpectrogram.__init__) == [
        ("sample_rate", E), ("n_fft", E), ("win_length", None), ("hop_length", None), ("pad", 0), ("window_fn", hann),
        ("power", 2.0), ("normalized", False), ("wkwargs", None), ("center", True), ("pad_mode", "reflect"),
        ("n_chroma", 12)] + chroma_kw
    assert kinds(T.ChromaSpectrogram.__init__) == [PK] * 2 + [KW] * 15
    assert params(T.BarkScale.forward) == [("specgram", E)] and params(T.ChromaScale.forward) == [("specgram", E)]
    assert params(T.InverseBarkScale.forward) == [("barkspec", E)]
    assert params(T.BarkSpectrogram.forward) == [("waveform", E)] and params(T.ChromaSpectrogram.forward) == [("waveform", E)]


def test_names_are_exported():
    fnames = {"barkscale_fbanks", "chroma_filterbank"}
    tnames = {"BarkScale", "InverseBarkScale", "BarkSpectrogram", "ChromaScale", "ChromaSpectrogram"}
    assert fnames | {"dense_fbank_scale", "dense_fbank_tiles"} <= set(F.__all__)
    assert tnames <= set(T.__all__)
    assert fnames <= set(PF.__all__) and all(getattr(PF, n) is getattr(F, n) for n in fnames)
    assert tnames == set(PT.__all__) and all(getattr(PT, n) is getattr(T, n) for n in tnames)
    import audio_amd.prototype as P
    assert P.transforms is PT and P.functional is PF


def test_modules_hold_the_builders_buffers():
    m = T.BarkScale(40, 16000, 20.0, 7000.0, 201, "wang")
    assert list(m.state_dict()) == ["fb"] and torch.equal(m.fb, F.barkscale_fbanks(201, 20.0, 7000.0, 40, 16000, "wang"))
    assert (m.n_barks, m.sample_rate, m.f_min, m.f_max, m.bark_scale) == (40, 16000, 20.0, 7000.0, "wang")
    assert T.BarkScale(40).f_max == 8000.0
    with pytest.raises(ValueError, match="Require f_min: 9000.0 <= f_max: 8000.0"):
        T.BarkScale(40, 16000, 9000.0)
    with pytest.raises(ValueError, match="Require f_min: 9000.0 <= f_max: 8000.0"):
        T.InverseBarkScale(201, 40, 16000, 9000.0)
    b = T.BarkSpectrogram(16000, 400, n_barks=40, bark_scale="schroeder")
    assert list(b.state_dict()) == ["spectrogram.window", "bark_scale.fb"]
    assert isinstance(b.spectrogram, T.Spectrogram) and isinstance(b.bark_scale, T.BarkScale)
    assert torch.equal(b.bark_scale.fb, F.barkscale_fbanks(201, 0.0, 8000.0, 40, 16000, "schroeder"))
    assert (b.win_length, b.hop_length, b.spectrogram.power) == (400, 200, 2.0)
    i = T.InverseBarkScale(201, 40, sgdargs={"lr": 0.5})
    assert list(i.state_dict()) == ["fb"] and torch.equal(i.fb, F.barkscale_fbanks(201, 0.0, 8000.0, 40, 16000))
    assert (i.max_iter, i.tolerance_loss, i.tolerance_change, i.sgdargs) == (100000, 1e-5, 1e-8, {"lr": 0.5})
    c = T.ChromaScale(16000, 201, n_chroma=24, tuning=0.1)
    assert list(c.state_dict()) == ["fb"] and torch.equal(c.fb, F.chroma_filterbank(16000, 201, 24, tuning=0.1))
    s = T.ChromaSpectrogram(22050, 512, hop_length=128, power=1.0, n_chroma=12, norm=1)
    assert list(s.state_dict()) == ["spectrogram.window", "chroma_scale.fb"]
    assert isinstance(s.spectrogram, T.Spectrogram) and isinstance(s.chroma_scale, T.ChromaScale)
    assert torch.equal(s.chroma_scale.fb, F.chroma_filterbank(22050, 257, 12, norm=1))
    assert (s.spectrogram.n_fft, s.spectrogram.hop_length, s.spectrogram.power) == (512, 128, 1.0)


def test_dense_fbank_scale_errors():
    fb = F.chroma_filterbank(16000, 33, 12)
    with pytest.raises(ValueError, match=r"expected an input with 33 frequency bins.*Found: 34"):
        F.dense_fbank_scale(torch.rand(2, 34, 5), fb)
    with pytest.raises(ValueError, match="expected an input with 33 frequency bins"):
        F.dense_fbank_scale(torch.rand(33), fb)
    with pytest.raises(TypeError, match="float16, bfloat16, float32 or float64"):
        F.dense_fbank_scale(torch.ones(2, 33, 5, dtype=torch.int32), fb)
    with pytest.raises(TypeError, match="must be tensors"):
        F.dense_fbank_scale([[1.0]], fb)
    with pytest.raises(ValueError, match="n_freqs, n_out"):
        F.dense_fbank_scale(torch.rand(2, 33, 5), fb[0])
    with pytest.raises(ValueError, match=r"expected an input with 33 frequency bins.*Found: 34"):
        T.ChromaScale(16000, 33)(torch.rand(2, 34, 5))


@pytest.mark.parametrize("call", [
    lambda: F.dense_fbank_scale(torch.rand(2, 33, 5), F.chroma_filterbank(16000, 33, 12)),
    lambda: F.dense_fbank_scale(torch.rand(2, 33, 5, dtype=torch.float64), F.chroma_filterbank(16000, 33, 12)),
    lambda: F.dense_fbank_scale(torch.rand(33, 5).half(), F.chroma_filterbank(16000, 33, 12)),
    lambda: T.ChromaScale(16000, 33)(torch.rand(2, 33, 5)),
    lambda: T.ChromaScale(16000, 33)(torch.rand(2, 33, 5, requires_grad=True)),
    lambda: T.ChromaSpectrogram(16000, 64)(torch.rand(2, 400)),
    lambda: T.BarkScale(10, 8000, n_stft=33)(torch.rand(2, 33, 5)),
    lambda: T.InverseBarkScale(33, 10, 8000)(torch.rand(2, 10, 5)),
    lambda: T.BarkSpectrogram(8000, 64, n_barks=10)(torch.rand(2, 400)),
])
def test_cpu_tensors_are_refused(call):
    with pytest.raises(RuntimeError, match=r"must be on an MI355X \(ROCm\) device.*no CPU fallback"):
        call()
