"""The generic mixed-radix kernels -- stft_generic_kernel<float | double, EPI_SPEC | EPI_MEL, LONG 0 | 1> (csrc/stft_generic.h),
ola_kernel<float, 0 | 1> / ola_kernel<double> (csrc/istft.h: inverse and STFT adjoint) and kgen::kaldi_generic_kernel<0 | 1, 0 | 1>
(csrc/kaldi_generic.h), 12 instantiations -- on a CENSUS of n_fft against float64, through the public API.

Why: these kernels are the yardstick of every fast-path parity test (`_force_generic`), the whole float64 route and the backward
of every size that is not 400 / 256 / 512 / 1024 / 2048, and until this file the device met them at sizes drawn at random from
eight values and judged them by the peak of a whole tensor of equal-gain rows.  Never launched before: a lone radix-2 stage in
front of odd factors (6, 10, 98, 202, 250), the generic-prime butterfly inside a composite plan (49, 441, 1001, 1102, 201), 3^k and
5^k chains (243, 125), odd composite n_fft (n_freq = N / 2 + 1 with no Nyquist bin: the 2 kk == N edge rule of ola_conj_z), the
power-of-two splits [4,4] [8,4] [8,4,4] [8,8,8,8] [8,8,8,4,4]; onesided=False and hop > n_fft; the mel epilogue at any generic size
but 320 and in the LONG layout (power rows in the free ping-pong buffer); n_fft between 8 192 and the LONG limit; the inverse's,
the float64 entry points' and Kaldi's own LDS boundaries; rows shorter than a workgroup (pb clamped), frame counts that are no
multiple of 2 pb, 300 rows, row-strided views and a base 4 bytes off a 16-byte boundary.

The census, the host mirror of the launchers, the inputs, the float64 references and the per-row judges live in
tests/generic_census.py; tests/test_generic_census.py runs the same cases through the CPU replay and holds the mirror against
the C++ functions.  Boundaries as the mirror computes them from the 160 KB LDS opt-in: the forward's full layout ends at 5 749,
the inverse's at 6 688, the LONG layout at 9 930 -- which the inverse serves, while every forward entry point stops at 8 192 in
validate_desc (api_common.hip), so the forward's first refused size is 8 193 and no forward runs between 8 192 and 9 930; float64
at 2 874 (forward) and 3 344 (inverse); Kaldi's full layout at 5 710 and its pairs per block switch at 2 400 | 2 402.  5 749 and 6 689 are primes, and a prime radix r is
one work item's r^2 complex MACs (3e7): the sizes that RUN on the two sides of a boundary are the nearest with a largest prime
factor <= 600 -- 5 748 | 5 750, 6 688 | 6 690, 5 710 | 5 712 -- while the refusals use the exact first size past each limit
(8 193, 9 931, 2 875, 3 345, Kaldi 8 194).  Primes run up to 509 (one work item, 2.6e5 MACs); Kaldi's 2 402 = 2 x 1 201 is the largest
prime factor that runs.

Every case: six rows with gains 1, 1e-3, 0, 1e-2, 1, 0 (the second all-zero row directly behind a gain-1 row), 2 (2 pb) + 3 frames
(two full workgroups and an odd tail) unless the case is about 3 frames or 300 rows; contiguous, row-strided and 4-byte-offset
inputs in turn; the case's radix plan, pb, blocks and layout asserted from the mirror before the launch.  Bars (none new): forward,
mel and adjoint 2e-5 of EACH ROW's float64 peak (fractional powers in the power domain), inverse max(2e-5, 4 x aten's own float32
istft error) per row under the condition min / max of sum w^2 >= 0.1 (asserted from the float64 window), float64 1e-12 per row,
Kaldi kaldi_fuzz_cases.judge against oracle/kaldi_oracle.py; all-zero rows exactly 0.0; a second forward call bit-equal.  A failure
names n_fft, the plan, the row, the frame and its workgroup.

The inverse's condition: with a periodic Hann window min / max of sum w^2 is >= 0.5 for hops n / 4, n / 3 and n / 2 -- odd n_fft
included -- as long as the row ends at or before the last frame's centre, which every `length` here does; a row that runs on into
the last frame's taper fails it (tests/test_generic_census.py shows both) and is not a case.  Two odd sizes at n // 2 are cases.

Measured on an MI355X: MEASURED_DEVICE below; no case found a kernel or a launcher wrong, every all-zero row came out exactly 0.0
and every second forward call bit-equal; the 168 tests of this file take 4.1 s together, the slowest 0.3 s.
"""
import contextlib
import ctypes as C
import re
import warnings

import numpy as np
import pytest
import torch

import generic_census as G

pytestmark = pytest.mark.gpu
LABEL = "gpu"

# Worst per-row err / bar per instantiation on an MI355X, one run of this file with -s (profiles/INDEX.md names the log); for the
# Kaldi kernels the worst element's |got - ref| over judge's own tolerance.
MEASURED_DEVICE = {
    "stft_generic_kernel<float, EPI_SPEC, 0>": (0.0591, "fwd-251-twosided"), "stft_generic_kernel<float, EPI_SPEC, 1>": (0.0360, "fwd-5750-census"),
    "stft_generic_kernel<float, EPI_MEL, 0>": (0.0303, "mel-5748"), "stft_generic_kernel<float, EPI_MEL, 1>": (0.0498, "mel-8192"),
    "stft_generic_kernel<double, EPI_SPEC, 0>": (0.0019, "f64-fwd-2874"),
    "ola_kernel<float, 0>": (0.0345, "inv-509-hop127"), "ola_kernel<float, 1>": (0.0399, "inv-9930-hop3310-cut"), "ola_kernel<double>": (0.0010, "f64-inv-251"),
    "kaldi_generic_kernel<0, 0>": (0.0360, "kaldi-5710-spectrogram"), "kaldi_generic_kernel<0, 1>": (0.0565, "kaldi-5712-spectrogram"),
    "kaldi_generic_kernel<1, 0>": (0.0188, "kaldi-1102-mfcc"), "kaldi_generic_kernel<1, 1>": (0.0012, "kaldi-5712-fbank"),
}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from audio_amd import _lib
    _lib.lib()
    d = torch.device("cuda", 0)
    # (the LDS opt-in the mirror assumes is pinned by behaviour: 9 930 runs in the LONG layout and 9 931 is refused, below)
    print("[generic-census] device", torch.cuda.get_device_name(0), "LDS opt-in as torch reports it:",
          getattr(torch.cuda.get_device_properties(0), "shared_memory_per_block_optin", None))
    return d


def _policy(c):
    """Sizes another kernel would take run the generic one under POLICY_FORCE_GENERIC."""
    from audio_amd import _lib
    return _lib.kernel_policy(_lib.POLICY_FORCE_GENERIC) if c["n_fft"] in G.FAST_PATH else contextlib.nullcontext()


def _assert_launch(c, n_frames, rows, kernel, onesided=True):
    """The plan, pb, blocks and layout the mirror expects for what is about to be launched."""
    from audio_amd import _host
    la = G.launch(kernel, c["dtype"], c["n_fft"], n_frames, rows, onesided)
    assert la == c["launch"], (c["id"], la, c["launch"])
    assert la["layout"] in ("full", "long") and la["lds"] <= G.LDS_OPTIN, (c["id"], la)
    assert la["plan"] == G.PLANS.get(c["n_fft"], la["plan"]) and int(np.prod(la["plan"])) == c["n_fft"], (c["id"], la)
    assert c["kernel"] == G.kernel_name(kernel, c["dtype"], la["layout"], c.get("epi", "SPEC"), int(c.get("fn", "spectrogram") != "spectrogram"))
    if kernel == "fwd":
        assert n_frames == _host.frame_count(c["length"], c["n_fft"], c["hop"], c["center"], c["pad"]), c["id"]
    return la


def _assert_layout(c, x, xd):
    from audio_amd import functional as F
    assert xd.shape == x.shape and xd.stride() == x.stride(), (c["id"], xd.stride(), x.stride())
    if c["layout"] == "strided":
        assert xd.stride(0) == c["length"] + 5 and F._rows2d(xd).data_ptr() == xd.data_ptr(), c["id"]      # no copy: row_stride is passed
    if c["layout"] == "offset":
        assert xd.data_ptr() % 16 == 4 and xd.is_contiguous(), (c["id"], xd.data_ptr() % 16)


def _bits(t):
    return torch.view_as_real(t) if t.is_complex() else t


def _spectrogram_module(c, dev):
    import audio_amd.transforms as T
    wdt = torch.float64 if c["dtype"] == "f64" else torch.float32
    return T.Spectrogram(n_fft=c["n_fft"], win_length=c["wl"], hop_length=c["hop"], pad=c["pad"], power=c["power"], normalized=c["norm"],
                         center=c["center"], pad_mode=c["pad_mode"], onesided=c["onesided"], window_fn=lambda n: G.window(c, wdt)).to(dev)


def check_forward(c, dev):
    x = G.make_wave(c)
    xd = G.place(x, dev)
    _assert_layout(c, x, xd)
    _assert_launch(c, c["n_frames"], c["rows"], "fwd", c["onesided"])
    t = _spectrogram_module(c, dev)
    with _policy(c), torch.no_grad():
        got = t(xd)
        again = t(xd)
    n_freq = c["n_fft"] // 2 + 1 if c["onesided"] else c["n_fft"]
    assert got.shape == (c["rows"], n_freq, c["n_frames"]), (c["id"], got.shape)
    assert got.dtype == {("f32", True): torch.complex64, ("f32", False): torch.float32, ("f64", True): torch.complex128,
                         ("f64", False): torch.float64}[(c["dtype"], c["power"] is None)], (c["id"], got.dtype)
    assert torch.equal(_bits(got), _bits(again)), (c["id"], "a second call differs")
    return G.judge_forward(c, got.cpu(), x, LABEL)


@pytest.mark.parametrize("c", G.forward_cases(), ids=[c["id"] for c in G.forward_cases()])
def test_census_forward_vs_float64_stft(c, dev):
    """A: stft_generic_kernel<float, EPI_SPEC, 0 | 1> through T.Spectrogram against float64 torch.stft, per row."""
    check_forward(c, dev)


@pytest.mark.parametrize("c", G.mel_cases(), ids=[c["id"] for c in G.mel_cases()])
def test_census_mel_epilogue_vs_float64_composition(c, dev):
    """B: stft_generic_kernel<float, EPI_MEL, 0 | 1> through T.MelSpectrogram against float64 stft -> |.|^p -> matmul."""
    import audio_amd.transforms as T
    x = G.make_wave(c)
    xd = G.place(x, dev)
    _assert_layout(c, x, xd)
    _assert_launch(c, c["n_frames"], c["rows"], "fwd")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")         # (narrow filters at the low end have no bin at small n_fft: the reference warns too)
        m = T.MelSpectrogram(sample_rate=c["sample_rate"], n_fft=c["n_fft"], hop_length=c["hop"], win_length=c["wl"], n_mels=c["n_mels"],
                             pad=c["pad"], power=c["power"], normalized=c["norm"] == "window", center=c["center"], pad_mode=c["pad_mode"])
    fb = m.mel_scale.fb.clone()
    m = m.to(dev)
    with _policy(c), torch.no_grad():
        got = m(xd)
        again = m(xd)
    assert got.shape == (c["rows"], c["n_mels"], c["n_frames"]), (c["id"], got.shape)
    assert torch.equal(got, again), (c["id"], "a second call differs")
    G.judge_mel(c, got.cpu(), x, fb, LABEL)


@pytest.mark.parametrize("c", G.inverse_cases(), ids=[c["id"] for c in G.inverse_cases()])
def test_census_inverse_vs_float64_istft(c, dev):
    """C: ola_kernel<float, 0 | 1> through T.InverseSpectrogram against float64 torch.istft, the suite's yardstick per row."""
    check_inverse(c, dev)


def check_inverse(c, dev):
    import audio_amd.transforms as T
    spec = G.make_spectrum(c)
    _assert_launch(c, c["n_frames"], c["rows"], "inv")
    wdt = torch.float64 if c["dtype"] == "f64" else torch.float32
    inv = T.InverseSpectrogram(n_fft=c["n_fft"], hop_length=c["hop"], normalized=c["norm"], window_fn=lambda n: G.window(c, wdt)).to(dev)
    with _policy(c), torch.no_grad():
        got = inv(spec.to(dev).transpose(-1, -2), c["length_arg"])
    assert got.shape == (c["rows"], c["length"]) and got.dtype == wdt, (c["id"], got.shape, got.dtype)
    return G.judge_inverse(c, got.cpu(), spec, LABEL)


@pytest.mark.parametrize("c", G.adjoint_cases(), ids=[c["id"] for c in G.adjoint_cases()])
def test_census_adjoint_vs_float64_autograd(c, dev):
    """D: the backward of T.Spectrogram (ola_kernel with adjoint = 1 and the forward's padding map) against float64 autograd through
    torch.stft, at the 2e-5 tests/test_gpu_fuzz_backward.py::_check_spectrogram_backward holds for powers None and 2 -- here per row."""
    x = G.make_wave(c)
    r = G.make_spectrum(c)
    _assert_launch(c, c["n_frames"], c["rows"], "inv")
    t = _spectrogram_module(c, dev)
    xg = G.place(x, dev).requires_grad_()
    with _policy(c):
        y = t(xg)
        rd = r.to(dev).transpose(-1, -2)
        ((y * rd.conj()).real.sum() if c["power"] is None else (y * rd.real).sum()).backward()
    assert xg.grad.shape == x.shape, c["id"]
    G.judge_adjoint(c, xg.grad.cpu(), x, r, LABEL)


@pytest.mark.parametrize("c", G.f64_cases(), ids=[c["id"] for c in G.f64_cases()])
def test_census_float64_route_vs_aten(c, dev):
    """E: stft_generic_kernel<double, EPI_SPEC> and ola_kernel<double> through the float64 route (ops.spectrogram_f64 / aamd_istft_f64)
    to 1e-12 of each row's peak, up to the largest n_fft each entry point serves."""
    (check_inverse if c["family"] == "inv" else check_forward)(c, dev)


@pytest.mark.parametrize("c", G.kaldi_cases(), ids=[c["id"] for c in G.kaldi_cases()])
def test_census_kaldi_generic_vs_oracle(c, dev):
    """F: kaldi_generic_kernel<0 | 1, 0 | 1> through compliance.kaldi.*_batch with round_to_power_of_two=False: three utterances, so
    blocks_per_utt > 1 and each utterance's tail block is partial; judged by kaldi_fuzz_cases.judge against the float64 oracle."""
    import audio_amd.compliance.kaldi as K
    from oracle import kaldi_oracle as KO
    assert KO.sizes(16000.0, c["kw"]["frame_shift"], c["kw"]["frame_length"], False) == (c["shift"], c["n_fft"], c["n_fft"]), c["id"]
    la = _assert_launch(c, c["n_frames"], c["n_utt"], "kaldi")
    assert la["bpr"] > 1 and c["n_frames"] % (2 * la["pb"]) != 0, (c["id"], la)
    x = G.make_wave(c, rows=c["n_utt"])
    with _policy(c), torch.no_grad():
        got = getattr(K, c["fn"] + "_batch")(x.to(dev), **c["kw"])
    assert got.shape[:2] == (c["n_utt"], c["n_frames"]), (c["id"], got.shape)
    G.judge_kaldi(c, got.cpu().numpy(), x.numpy(), LABEL)


def _valid_call_still_correct(dev):
    c = next(c for c in G.forward_cases() if c["id"] == "fwd-98-census")
    assert check_forward(c, dev) <= 1.0


REFUSALS = G.refusal_cases()


@pytest.mark.parametrize("r", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_first_size_past_each_limit_is_refused_with_the_launchers_message(r, dev):
    """G: the first n_fft past each limit raises a RuntimeError with the launcher's own text, and the next valid call is correct.
    Each of these launchers returns fail(AAMD_EUNSUPPORTED, ...) from its LDS check, in front of its only launch() (api_stft.hip
    launch_generic, api_istft.hip, api_f64.hip, api_kaldi.hip): the refused call runs nothing on the device."""
    import audio_amd.compliance.kaldi as K
    import audio_amd.transforms as T
    from audio_amd import _lib
    from audio_amd import functional as F
    name, entry, n, message = r
    dtype = "f64" if "f64" in entry else "f32"
    rdt = torch.float64 if dtype == "f64" else torch.float32
    assert G.launch("kaldi" if entry == "kaldi" else ("inv" if "inverse" in entry else "fwd"), dtype, n)["layout"] == "refused"
    hop = n // 4
    if entry.startswith("spectrogram"):
        t = T.Spectrogram(n_fft=n, hop_length=hop, power=None).to(device=dev, dtype=rdt)
        with pytest.raises(RuntimeError, match=re.escape(message)) as e:
            t(torch.zeros(2, 2 * n, dtype=rdt, device=dev))
    elif entry.startswith("inverse"):
        inv = T.InverseSpectrogram(n_fft=n, hop_length=hop).to(device=dev, dtype=rdt)
        spec = torch.zeros(2, n // 2 + 1, 5, dtype=torch.complex128 if dtype == "f64" else torch.complex64, device=dev)
        with pytest.raises(RuntimeError, match=re.escape(message)) as e:
            inv(spec)
    else:
        # the public entry point refuses in Python (NotImplementedError, a RuntimeError); the launcher's own text through the C ABI
        x = torch.zeros(1, n + 320, device=dev)
        with pytest.raises(RuntimeError, match="padded windows above 8192"):
            K.spectrogram(x, frame_length=G.ms_for(n), round_to_power_of_two=False)
        win, out = torch.ones(n, device=dev), torch.zeros(3, n // 2 + 1, device=dev)
        d = _lib.KaldiDesc(n + 320, 3, n, 160, n, 1, 0.97, 1, 1, 0.0, 1, 1, -1, 0, n // 2 + 1, 0.0, None, 1, n + 320)
        with pytest.raises(RuntimeError, match=re.escape(message)) as e:
            _lib.check(_lib.lib().aamd_kaldi_features_f32(x.data_ptr(), win.data_ptr(), F._twiddles(n, dev).data_ptr(), None, out.data_ptr(),
                                                          C.byref(d), _lib.current_stream(dev)))
    assert ("(float64)" in str(e.value)) == (dtype == "f64"), str(e.value)
    torch.cuda.synchronize()
    _valid_call_still_correct(dev)


def test_every_instantiation_ran_and_report(dev):
    """After the cases above (file order): every kernel instantiation was judged on the device at least once (that the census holds
    a case for each is asserted device-free in tests/test_generic_census.py); the worst fraction of its bar per instantiation is
    printed for the record."""
    ran = {k[1]: v for k, v in G.WORST.items() if k[0] == LABEL}
    assert set(ran) <= G.KERNELS_WANTED
    if len(ran) >= 8:            # the whole file ran (a selection of cases leaves a partial record)
        assert set(ran) == G.KERNELS_WANTED, G.KERNELS_WANTED - set(ran)
    for k in sorted(ran):
        print("[generic-census] worst %s %.4f %s" % (k, ran[k][0], ran[k][1]))
        assert ran[k][0] <= 1.0
