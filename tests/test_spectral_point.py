"""LFCC, SpectralCentroid, the mu-law pair, Fade, Vol and their functionals without a GPU: a CPU replay of
csrc/spectral_feat.h and csrc/wave_pointwise.h (the kernels' phase functions compiled with g++, the launch geometry of the C
ABI) against tests/spectral_point_oracle.py, LFCC end to end on the suite's replay of the three STFT families, the host
constants, signatures, exports, every error with its type and message, and the refusal of CPU tensors."""
import ctypes as C
import inspect
import os
import subprocess
import warnings

import numpy as np
import pytest
import torch

import spectral_point_cases as K
import spectral_point_oracle as O
import audio_amd.functional as F
import audio_amd.transforms as T
from audio_amd import _host

HERE = os.path.dirname(os.path.abspath(__file__))
SIM_SRC = os.path.join(HERE, "cpu_sim", "sim_spectral_point.cpp")
SIM_OUT = os.path.join(HERE, "cpu_sim", "_build", "libaamd_sim_spectral_point.so")
HDRS = [os.path.join(os.path.dirname(HERE), "audio_amd", "csrc", h)
        for h in ("spectral_feat.h", "wave_pointwise.h", "wave_augment.h", "spec_augment.h", "hd.h")]
CODE = {torch.float32: 0, torch.float64: 1, torch.float16: 2, torch.bfloat16: 3, torch.int64: 4, torch.int32: 5, torch.int16: 6,
        torch.int8: 7, torch.uint8: 8}
CANARY = 64          # bytes on either side of a result; a multiple of 16, so the result keeps its alignment

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
        i64, i32, p, d = C.c_int64, C.c_int, C.c_void_p, C.c_double
        _sim.sim_spectral_lanes.argtypes = [i64]
        _sim.sim_spectral_centroid.argtypes = [i32, p, p, p] + [i64] * 6
        _sim.sim_pointwise.argtypes = [i32, i32, p, p, i64, i64, i64, d, d, i32, p, i64, i64]
    return _sim


def _guarded(shape, dtype):
    """A result between two canaries: (the whole byte buffer, the result as a view of it)."""
    n = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
    buf = torch.full((n + 2 * CANARY,), 0xA5, dtype=torch.uint8)
    assert buf.data_ptr() % 16 == 0
    return buf, buf[CANARY:CANARY + n].view(dtype).view(shape)


def _check_canaries(buf):
    assert (buf[:CANARY] == 0xA5).all() and (buf[-CANARY:] == 0xA5).all(), "a kernel wrote outside its result"


class Replay:
    """The backend of spectral_point_cases: the kernels' phase functions on the CPU."""

    @staticmethod
    def pointwise(op, x, out_dtype, p0, p1, flag, table, n_in, n_out):
        rows, L = x.shape
        assert L <= 1 or x.stride(1) == 1
        buf, out = _guarded((rows, L), out_dtype)
        rc = sim().sim_pointwise(op, CODE[x.dtype], x.data_ptr(), out.data_ptr(), rows, L, x.stride(0), p0, p1, flag,
                                 None if table is None else table.data_ptr(), n_in, n_out)
        assert rc == 0, rc
        _check_canaries(buf)
        return out.clone()

    @staticmethod
    def centroid(m3, freqs, out_dtype):
        rows, frames, n_freq = m3.shape
        buf, out = _guarded((rows, frames), out_dtype)
        rc = sim().sim_spectral_centroid(CODE[out_dtype], m3.data_ptr(), freqs.data_ptr(), out.data_ptr(), rows, frames, n_freq,
                                         m3.stride(0), m3.stride(1), m3.stride(2))
        assert rc == 0, rc
        _check_canaries(buf)
        return out.clone()


# ---- 1. host constants, bit-exact -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("args", [(201, 0.0, 8000.0, 128, 16000), (33, 0.0, 8000.0, 40, 16000), (513, 0.0, 8000.0, 128, 16000),
                                  (257, 20.0, 7600.0, 60, 16000), (241, 0.0, 11025.0, 70, 22050)])
def test_linear_fbanks_equals_the_definition(args):
    got = F.linear_fbanks(*args)
    assert got.dtype == torch.float32 and tuple(got.shape) == (args[0], args[3])
    assert torch.equal(got, O.linear_fbanks(*args)) and got is not None and F.linear_fbanks is _host.linear_fbanks


def test_banded_tables_of_the_linear_filterbank():
    """What decides which kernel LFCC runs on: the default is as narrow as the n_fft = 400 kernel needs."""
    for (bins, filters), width in (((201, 128), 4), ((33, 40), 2), ((513, 128), 8)):
        fb = F.linear_fbanks(bins, 0.0, 8000.0, filters, 16000).numpy()
        lo, w, weights, max_width = _host.mel_band_table(fb)
        assert max_width == width and (w > 0).all(), (bins, filters, max_width, int((w == 0).sum()))


def test_lfcc_buffers_and_constants():
    m = T.LFCC()
    assert set(m.state_dict()) == {"Spectrogram.window", "filter_mat", "dct_mat"}
    assert tuple(m.filter_mat.shape) == (201, 128) and tuple(m.dct_mat.shape) == (128, 40) and m.Spectrogram.window.shape == (400,)
    assert torch.equal(m.filter_mat, O.linear_fbanks(201, 0.0, 8000.0, 128, 16000))
    assert torch.equal(m.dct_mat, F.create_dct(40, 128, "ortho"))
    assert T.LFCC.__constants__ == ["sample_rate", "n_filter", "n_lfcc", "dct_type", "top_db", "log_lf"]
    assert m.top_db == 80.0 and m.f_max == 8000.0 and isinstance(m.f_max, float) and m.amplitude_to_DB.top_db == 80.0
    assert isinstance(m.Spectrogram, T.Spectrogram) and m.amplitude_to_DB.multiplier == 10.0
    m = T.LFCC(sample_rate=22050, n_filter=40, n_lfcc=13, f_min=50.0, norm=None, log_lf=True, speckwargs=dict(n_fft=64, hop_length=16))
    assert tuple(m.filter_mat.shape) == (33, 40) and tuple(m.dct_mat.shape) == (40, 13) and m.f_max == 11025.0 and m.log_lf
    assert torch.equal(m.filter_mat, O.linear_fbanks(33, 50.0, 11025.0, 40, 22050))


def test_spectral_centroid_module_buffers_and_constants():
    m = T.SpectralCentroid(16000)
    assert list(m.state_dict()) == ["window"] and m.window.shape == (400,) and torch.equal(m.window, torch.hann_window(400))
    assert T.SpectralCentroid.__constants__ == ["sample_rate", "n_fft", "win_length", "hop_length", "pad"]
    assert (m.n_fft, m.win_length, m.hop_length, m.pad) == (400, 400, 200, 0)
    m = T.SpectralCentroid(8000, n_fft=512, win_length=300, window_fn=torch.hamming_window, wkwargs=dict(periodic=False))
    assert m.hop_length == 150 and torch.equal(m.window, torch.hamming_window(300, periodic=False))
    assert np.array_equal(_host.centroid_freqs(16000, 400), O.centroid_freqs(16000, 400))
    assert _host.centroid_freqs(22050, 512).dtype == np.float32 and _host.centroid_freqs(22050, 512)[-1] == 11025.0


@pytest.mark.parametrize("shape", O.SHAPES)
@pytest.mark.parametrize("dtype", K.FLOATS, ids=str)
def test_fade_tables_are_the_float64_ramps_rounded_once(shape, dtype):
    fi, fo = _host.fade_ramps(17, 9, shape)
    wi, wo = O.fade_ramps(17, 9, shape)
    assert fi.dtype == np.float64 and np.array_equal(fi, wi) and np.array_equal(fo, wo)
    assert fi.min() >= 0 and fi.max() <= 1 and fo.min() >= 0 and fo.max() <= 1 and fi[0] == 0
    rng = np.random.default_rng(3)
    vals = np.concatenate([fi, fo, rng.uniform(0, 1, 4000), 1 - 2.0 ** -9 + rng.uniform(-1, 1, 200) * 2.0 ** -12])
    K.assert_same_bits(_host.round_once(vals, dtype), O.round_to(vals, dtype), (shape, dtype))


def test_round_once_to_bfloat16_is_one_rounding():
    # 1 + 2^-8 + 2^-30 lies just above a tie: one rounding goes up, float32 first (a tie, to even) goes down
    v = np.array([1 + 2.0 ** -8 + 2.0 ** -30, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 3 * 2.0 ** -8 - 2.0 ** -30])
    want = [1 + 2.0 ** -7, 1.0, 1 + 2.0 ** -6, 1 + 2.0 ** -7]
    assert _host.round_once(v, torch.bfloat16).double().tolist() == want == O.round_bf16(v).tolist()


# ---- 2. the surface -----------------------------------------------------------------------------------------------------------

def _sig(fn):
    return [(p.name, p.default) for p in inspect.signature(fn).parameters.values() if p.name != "self"]


def test_signatures_and_defaults():
    E = inspect.Parameter.empty
    assert _sig(F.linear_fbanks) == [("n_freqs", E), ("f_min", E), ("f_max", E), ("n_filter", E), ("sample_rate", E)]
    assert _sig(F.spectral_centroid) == [(n, E) for n in ("waveform", "sample_rate", "pad", "window", "n_fft", "hop_length",
                                                          "win_length")]
    assert _sig(F.gain) == [("waveform", E), ("gain_db", 1.0)]
    assert _sig(F.contrast) == [("waveform", E), ("enhancement_amount", 75.0)]
    assert _sig(F.DB_to_amplitude) == [("x", E), ("ref", E), ("power", E)]
    assert _sig(F.mu_law_encoding) == [("x", E), ("quantization_channels", E)]
    assert _sig(F.mu_law_decoding) == [("x_mu", E), ("quantization_channels", E)]
    assert _sig(T.LFCC.__init__) == [("sample_rate", 16000), ("n_filter", 128), ("f_min", 0.0), ("f_max", None), ("n_lfcc", 40),
                                     ("dct_type", 2), ("norm", "ortho"), ("log_lf", False), ("speckwargs", None)]
    assert _sig(T.SpectralCentroid.__init__) == [("sample_rate", E), ("n_fft", 400), ("win_length", None), ("hop_length", None),
                                                 ("pad", 0), ("window_fn", torch.hann_window), ("wkwargs", None)]
    assert _sig(T.MuLawEncoding.__init__) == _sig(T.MuLawDecoding.__init__) == [("quantization_channels", 256)]
    assert _sig(T.Fade.__init__) == [("fade_in_len", 0), ("fade_out_len", 0), ("fade_shape", "linear")]
    assert _sig(T.Vol.__init__) == [("gain", E), ("gain_type", "amplitude")]
    for cls, arg in ((T.LFCC, "waveform"), (T.SpectralCentroid, "waveform"), (T.MuLawEncoding, "x"), (T.MuLawDecoding, "x_mu"),
                     (T.Fade, "waveform"), (T.Vol, "waveform")):
        assert _sig(cls.forward) == [(arg, E)] and issubclass(cls, torch.nn.Module)
    assert T.MuLawEncoding.__constants__ == T.MuLawDecoding.__constants__ == ["quantization_channels"]
    for m in (T.MuLawEncoding(), T.MuLawDecoding(), T.Fade(3, 4), T.Vol(0.5)):
        assert len(m.state_dict()) == 0


def test_names_are_exported():
    assert {"linear_fbanks", "spectral_centroid", "spectral_tiles", "gain", "contrast", "DB_to_amplitude", "mu_law_encoding",
            "mu_law_decoding", "pointwise_tiles"} <= set(F.__all__)
    assert {"LFCC", "SpectralCentroid", "MuLawEncoding", "MuLawDecoding", "Fade", "Vol"} <= set(T.__all__)
    assert not hasattr(T, "Loudness") and not hasattr(F, "dither") and not hasattr(F, "dcshift")
    assert (sim().sim_spectral_tiles(0), sim().sim_spectral_tiles(1), sim().sim_spectral_tiles(2)) == (256, 4, 64)
    assert (sim().sim_pointwise_tiles(0), sim().sim_pointwise_tiles(1)) == (256, 4096)
    assert [sim().sim_spectral_lanes(n) for n in (1, 4, 5, 33, 201, 252, 253, 257, 4097)] == [1, 1, 1, 4, 16, 16, 16, 32, 64]


def test_errors_with_their_types_and_messages():
    x = torch.zeros(2, 100)
    with pytest.raises(ValueError, match="DCT type not supported: 3"):
        T.LFCC(dct_type=3)
    with pytest.raises(ValueError, match="Cannot select more LFCC coefficients than # fft bins"):
        T.LFCC(n_lfcc=65, speckwargs=dict(n_fft=64))
    for amount in (-0.1, 100.5):
        with pytest.raises(ValueError, match="Allowed range of values for enhancement_amount : 0-100"):
            F.contrast(x, amount)
    for kind in ("amplitude", "power"):
        with pytest.raises(ValueError, match="If gain_type = amplitude or power, gain must be positive."):
            T.Vol(-0.5, kind)
    T.Vol(-3.0, "db")
    with pytest.raises(ValueError, match="gain_type"):
        T.Vol(1.0, "loud")(x)
    with pytest.raises(ValueError, match="fade_shape"):
        T.Fade(1, 1, "cubic")
    m = T.Fade(1, 1)
    m.fade_shape = "cubic"
    with pytest.raises(ValueError, match="fade_shape"):
        m(x)
    for n_in, n_out in ((101, 0), (0, 101)):
        with pytest.raises(ValueError, match="longer than the signal"):
            T.Fade(n_in, n_out)(x)
    with pytest.raises(ValueError, match="negative"):
        T.Fade(-1, 0)(x)
    for fn in (F.mu_law_encoding, F.mu_law_decoding):
        with pytest.raises(ValueError, match="quantization_channels"):
            fn(x, 1)
    for fn in (lambda t: F.gain(t, 2.0), F.contrast, lambda t: F.DB_to_amplitude(t, 1.0, 1.0), T.Fade(1, 1), T.Vol(0.5)):
        with pytest.raises(TypeError):
            fn(torch.zeros(2, 100, dtype=torch.int32))
        with pytest.raises(TypeError):
            fn(torch.zeros(2, 100, dtype=torch.complex64))
    for fn in (lambda t: F.mu_law_encoding(t, 256), lambda t: F.mu_law_decoding(t, 256)):
        for dt in (torch.complex64, torch.bool):
            with pytest.raises(TypeError):
                fn(torch.zeros(2, 100, dtype=dt))
    with pytest.raises(TypeError):
        F.spectral_centroid(torch.zeros(2, 1000, dtype=torch.int16), 16000, 0, torch.hann_window(400), 400, 200, 400)


def _entry_points():
    w = torch.hann_window(400)
    return {"gain": lambda t: F.gain(t, 3.0), "contrast": F.contrast, "DB_to_amplitude": lambda t: F.DB_to_amplitude(t, 1.0, 0.5),
            "mu_law_encoding": lambda t: F.mu_law_encoding(t, 256), "mu_law_decoding": lambda t: F.mu_law_decoding(t, 256),
            "spectral_centroid": lambda t: F.spectral_centroid(t, 16000, 0, w, 400, 200, 400),
            "LFCC": T.LFCC(), "SpectralCentroid": T.SpectralCentroid(16000), "MuLawEncoding": T.MuLawEncoding(),
            "MuLawDecoding": T.MuLawDecoding(), "Fade": T.Fade(10, 10), "Vol": T.Vol(0.5), "Vol db": T.Vol(3.0, "db"),
            "Vol power": T.Vol(0.5, "power")}


@pytest.mark.parametrize("name", list(_entry_points()))
def test_cpu_tensors_are_refused(name):
    fn = _entry_points()[name]
    with pytest.raises(RuntimeError, match=r"must be on an MI355X \(ROCm\) device.*no CPU fallback"):
        fn(torch.zeros(2, 4000))
    if name not in ("mu_law_encoding", "MuLawEncoding"):
        with pytest.raises(RuntimeError, match="MI355X"):
            fn(torch.zeros(2, 4000, requires_grad=True))
    if name in ("mu_law_decoding", "MuLawDecoding"):
        with pytest.raises(RuntimeError, match="MI355X"):
            fn(torch.zeros(2, 4000, dtype=torch.int64))


def test_gain_of_zero_db_returns_the_input_object_and_integers_warn():
    x = torch.zeros(3)
    assert F.gain(x, 0) is x and F.gain(x, 0.0) is x
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        with pytest.raises(RuntimeError, match="MI355X"):
            F.mu_law_encoding(torch.zeros(4, dtype=torch.int32), 256)
    assert not w                                         # the refusal comes first; on the device the conversion warns


# ---- 3. replay of the centroid kernel --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["lines", "time"])
@pytest.mark.parametrize("n_freq", K.N_FREQS)
def test_centroid_replay_within_one_ulp_of_float64_sums(n_freq, layout):
    for frames in K.N_FRAMES:
        for rows in K.N_ROWS:
            K.check_centroid(Replay, n_freq, frames, rows, layout)


@pytest.mark.parametrize("out_dtype", [torch.float16, torch.bfloat16], ids=str)
def test_centroid_replay_rounds_once_to_the_output_type(out_dtype):
    for n_freq in (33, 201):
        K.check_centroid(Replay, n_freq, 65, 3, "lines", out_dtype)


@pytest.mark.parametrize("layout", ["lines", "time"])
def test_centroid_replay_zero_and_nan_frames(layout):
    K.check_centroid_zero_and_nan_frames(Replay, layout)


def test_centroid_replay_every_alignment_of_a_line_gives_the_float64_value():
    """A line that starts 0 .. 3 elements past a 16-byte boundary: whole vectors are loaded as such, the ends element by
    element, and nothing outside the line is read (the neighbours are NaN)."""
    rng = np.random.default_rng(9)
    for n_freq in (1, 2, 3, 4, 5, 7, 8, 9, 201):
        for off in range(4):
            base = torch.full((off + 2 * n_freq + 8,), float("nan"))
            m3 = base.as_strided((1, 2, n_freq), (0, n_freq, 1), off)
            m3.copy_(torch.from_numpy(np.abs(rng.standard_normal((1, 2, n_freq))).astype(np.float32)))
            freqs = K.freqs_of(n_freq)
            K.assert_centroid(Replay.centroid(m3, freqs, torch.float32), m3, freqs, torch.float32, (n_freq, off))


# ---- 4. replay of the pointwise ops ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", K.LAYOUTS)
@pytest.mark.parametrize("dtype", K.FLOATS, ids=str)
def test_scale_replay_gain_and_vol_are_bit_exact(dtype, layout):
    for L in K.LENGTHS + (4099,):
        K.check_scale(Replay, dtype, L, layout)


@pytest.mark.parametrize("shape", O.SHAPES)
@pytest.mark.parametrize("dtype", K.FLOATS, ids=str)
def test_fade_replay_is_the_table_times_x_and_bit_copies_elsewhere(dtype, shape):
    for L in K.LENGTHS:
        for layout in K.LAYOUTS:
            K.check_fade(Replay, dtype, L, layout, shape)
    K.check_fade(Replay, dtype, 4099, "offset", shape)


@pytest.mark.parametrize("layout", K.LAYOUTS)
@pytest.mark.parametrize("dtype", K.FLOATS, ids=str)
def test_contrast_replay_within_4x_the_definitions_own_error(dtype, layout):
    K.check_contrast(Replay, dtype, layout)
    K.check_contrast(Replay, dtype, layout, (1025,), amount=0.0)
    K.check_contrast(Replay, dtype, layout, (1025,), amount=100.0)


@pytest.mark.parametrize("layout", K.LAYOUTS)
@pytest.mark.parametrize("dtype", K.FLOATS, ids=str)
def test_db_to_amplitude_replay_within_4x_the_definitions_own_error(dtype, layout):
    K.check_db_to_amplitude(Replay, dtype, layout)
    K.check_db_to_amplitude(Replay, dtype, layout, (1025,), ref=0.5, power=1.0)


@pytest.mark.parametrize("layout", K.LAYOUTS)
@pytest.mark.parametrize("dtype", K.FLOATS + (torch.int64, torch.int32, torch.uint8), ids=str)
def test_mu_law_decoding_replay_within_4x_the_definitions_own_error(dtype, layout):
    K.check_mu_decode(Replay, dtype, 256, layout)
    # (two channels have two codes, both decoded exactly in every precision: they give no yardstick, see the exact cases)
    for q in (16,) + ((1024,) if dtype not in (torch.uint8,) else ()):
        K.check_mu_decode(Replay, dtype, q, layout, (1025,))


@pytest.mark.parametrize("dtype", [torch.int16, torch.int8], ids=str)
def test_mu_law_decoding_replay_reads_the_narrow_integer_types(dtype):
    K.check_mu_decode(Replay, dtype, 128, "offset", (1025,))


@pytest.mark.parametrize("q", [2, 16, 256, 1024])
@pytest.mark.parametrize("dtype", K.FLOATS, ids=str)
def test_mu_law_encoding_replay_equals_the_float64_codes_outside_the_band(dtype, q):
    for L in K.LENGTHS + (4099,):
        for layout in K.LAYOUTS:
            K.check_mu_encode(Replay, dtype, q, L, layout)


@pytest.mark.parametrize("q", [2, 16, 256, 1024])
@pytest.mark.parametrize("dtype", K.FLOATS, ids=str)
def test_mu_law_replay_exact_cases_and_round_trip(dtype, q):
    K.check_mu_exact_and_round_trip(Replay, dtype, q)


def test_the_band_of_the_encoding_test_is_as_narrow_as_stated():
    """With uniform inputs and 256 channels well under 0.1 % of the inputs lie in the band, and numpy's float32 form of the
    definition disagrees with float64 only inside it."""
    x = np.random.default_rng(0).uniform(-1, 1, 400000)
    v = O.mu_encode_value(x, 256, np.float64)
    band = np.abs(v - np.round(v)) <= O.mu_band(256)
    assert band.mean() < 1e-3
    x32 = x.astype(np.float32)
    v = O.mu_encode_value(x32.astype(np.float64), 256, np.float64)
    band = np.abs(v - np.round(v)) <= O.mu_band(256)
    differs = O.mu_encode(x32, 256, np.float32) != np.trunc(v).astype(np.int64)
    assert not (differs & ~band).any()


# ---- 5. LFCC end to end on the replay of the three STFT families -------------------------------------------------------------------

def _lfcc_replay(x, m):
    """T.LFCC.forward's launches on the CPU: the filterbank kernel of the family that serves n_fft, then dB with the group
    cut-off (or the log) and the DCT kernel."""
    import sim_util as S
    sp = m.Spectrogram
    n_fft, hop = sp.n_fft, sp.hop_length
    w = sp.window.numpy()
    fb, dct = m.filter_mat.numpy(), np.ascontiguousarray(m.dct_mat.numpy())
    rows = x.shape[0]
    if n_fft == 400:
        mel = S.sim_mel400(x, w, S.HostBands(fb), hop=hop)
    elif n_fft == 512:
        mel = S.sim_stft_pow2(x, w, S.make_desc(rows, x.shape[1], n_fft, hop), S.HostBands(fb))
    else:
        mel = S.sim_mel_generic(x, w, S.HostBands(fb), S.make_desc(rows, x.shape[1], n_fft, hop))
    mel_fm = np.ascontiguousarray(np.swapaxes(mel, -1, -2))                 # (rows, T, n_filter)
    T_ = mel_fm.shape[1]
    flat = mel_fm.reshape(rows * T_, -1)
    if m.log_lf:
        out = S.sim_mfcc_dct_mfma(flat, dct, 1)
    else:
        db = S.sim_db_values(flat, 10.0, 1e-10, 0.0)
        gmax = db.reshape(1, -1).max(axis=1)                                 # a 2-D input is one cut-off group
        out = S.sim_mfcc_dct_mfma(db, dct, 2, gmax, rows * T_, 80.0)
    return np.swapaxes(out.reshape(rows, T_, -1), -1, -2)


@pytest.mark.parametrize("log_lf", [False, True])
@pytest.mark.parametrize("n_fft,n_filter", [(400, 128), (512, 128), (480, 128), (64, 40)])
def test_lfcc_end_to_end_on_the_replay(n_fft, n_filter, log_lf):
    from oracle import dsp_oracle as D
    rng = np.random.default_rng(n_fft)
    t = np.arange(4000) / 16000.0
    x = (0.4 * np.sin(2 * np.pi * 440 * t) + 0.2 * np.sin(2 * np.pi * 3100 * t))[None, :] + 0.05 * rng.standard_normal((3, 4000))
    x = x.astype(np.float32)
    m = T.LFCC(n_filter=n_filter, n_lfcc=min(40, n_filter), log_lf=log_lf, speckwargs=dict(n_fft=n_fft, hop_length=n_fft // 4))
    got = _lfcc_replay(x, m)
    want = D.mfcc(x, m.Spectrogram.window.numpy(), m.filter_mat.numpy(), m.dct_mat.numpy(), n_fft, n_fft // 4, log_mels=log_lf)
    assert got.shape == want.shape == (3, min(40, n_filter), 1 + 4000 // (n_fft // 4))
    err = np.abs(got - want).max() / np.abs(want).max()
    print("LFCC replay n_fft=%d log_lf=%s: peak-relative error %.3e" % (n_fft, log_lf, err))
    assert err <= 1e-4                                   # TOL["MFCC"] of tests/test_gpu_parity.py
