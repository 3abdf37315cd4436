"""The synthesis ops of audio_amd.prototype.functional on the device through the product API, against tests/dsp_oracle.py: the
checks of tests/test_dsp_synth.py (dsp_cases.py) on the shapes that straddle the scan's chunk and the filter's tile, then
what only the product has: leading axes and row views read in place, adsr_envelope, the three forms of `pattern`, F.convolve
as a second opinion, graph capture of oscillator_bank -> filter_waveform, refusals, and the differentiable compositions
(values against the kernels, gradcheck in float64)."""
import numpy as np
import pytest
import torch

import dsp_cases as K
import dsp_oracle as O
import audio_amd.functional as F
import audio_amd.prototype.functional as P
from audio_amd import _diff

pytestmark = pytest.mark.gpu
DEV = "cuda"


class Device:
    """The backend of dsp_cases: the entry points on the device."""

    @staticmethod
    def tiles():
        return F.dsp_tiles()

    @staticmethod
    def osc(f, a, sample_rate, reduction):
        return F.oscillator_bank(f.to(DEV), a.to(DEV), sample_rate, reduction).cpu()

    @staticmethod
    def fw(x, h):
        return F.filter_waveform(x.to(DEV), h.to(DEV)).cpu()

    @staticmethod
    def sinc(cutoff, window_size, high_pass):
        return F.sinc_impulse_response(cutoff.to(DEV), window_size, high_pass).cpu()

    @staticmethod
    def fir(m):
        return F.frequency_impulse_response(m.to(DEV)).cpu()

    @staticmethod
    def pitch(base, pat):
        return F.extend_pitch(base.to(DEV), pat.to(DEV)).cpu()


def test_tiles_are_what_the_cases_straddle():
    assert Device.tiles() == (K.CH, K.TILE, F.DSP_MAX_TAPS, F.DSP_MAX_OSCILLATORS, F.DSP_MAX_MAGNITUDES)
    assert P.oscillator_bank is F.oscillator_bank and P.filter_waveform is F.filter_waveform


# ---- accuracy ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("N", K.OSC_N)
@pytest.mark.parametrize("T", K.OSC_T)
def test_oscillator_bank_within_the_bar(T, N, dt):
    K.check_osc(Device, 2, T, N, dt)


@pytest.mark.parametrize("dt", list(K.DTYPES))
@pytest.mark.parametrize("reduction", ["mean", "none"])
def test_oscillator_bank_reductions_and_half_types(reduction, dt):
    K.check_osc(Device, 2, K.CH + 1, 3, dt, reduction)
    K.check_osc(Device, 2, K.CH + 1, 65, dt, "sum")


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_oscillator_bank_long_phase(dt):
    K.check_osc(Device, 1, 40 * K.CH, 2, dt)


@pytest.mark.parametrize("dt", list(K.DTYPES))
@pytest.mark.parametrize("batched", [False, True])
@pytest.mark.parametrize("shape", K.FW_SHAPES)
def test_filter_waveform_within_the_bar(shape, batched, dt):
    K.check_fw(Device, *shape, dt, batched)


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("high_pass", [False, True])
@pytest.mark.parametrize("W", K.SINC_W)
def test_sinc_impulse_response_within_the_bar(W, high_pass, dt):
    K.check_sinc(Device, W, high_pass, dt)
    K.check_sinc_batch(Device, dt)


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("n", K.FIR_N)
def test_frequency_impulse_response_within_the_bar(n, dt):
    K.check_fir(Device, n, dt)


@pytest.mark.parametrize("dt", list(K.DTYPES))
def test_extend_pitch_is_the_product_rounded_once(dt):
    K.check_pitch(Device, dt)
    base = torch.from_numpy(np.random.default_rng(4).uniform(50.0, 500.0, (3, 17, 1))).to(K.DTYPES[dt]).to(DEV)
    by_int = F.extend_pitch(base, 4)
    assert by_int.shape == (3, 17, 4)
    assert torch.equal(by_int, F.extend_pitch(base, [1.0, 2.0, 3.0, 4.0]))
    assert torch.equal(by_int, F.extend_pitch(base, torch.tensor([1.0, 2.0, 3.0, 4.0], dtype=base.dtype, device=DEV)))
    assert torch.equal(by_int[..., 0:1], base)
    assert F.extend_pitch(base, 0).shape == (3, 17, 0)
    assert torch.equal(F.extend_pitch(base.transpose(0, 1), 4), by_int.transpose(0, 1))      # gathered first


@pytest.mark.parametrize("dt", list(K.DTYPES))
def test_adsr_envelope_is_the_oracle_rounded_once(dt):
    from audio_amd import _host
    cases = [dict(), dict(attack=1.0), dict(attack=0.2, hold=0.1, decay=0.3, sustain=0.4, release=0.25, n_decay=3)]
    for kw in cases:
        for num in (1, 7, 1001):
            got = F.adsr_envelope(num, dtype=K.DTYPES[dt], **kw)
            assert got.is_cuda and got.dtype == K.DTYPES[dt] and got.shape == (num,)
            assert torch.equal(got.cpu(), _host.round_once(O.adsr_envelope(num, **kw), K.DTYPES[dt]))
    assert F.adsr_envelope(5).dtype == torch.get_default_dtype()
    assert torch.equal(F.adsr_envelope(5, device=DEV), torch.ones(5, device=DEV))


# ---- exact properties --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_oscillator_prefix_rows_and_poison(dt):
    K.check_osc_prefix(Device, dt)
    K.check_osc_rows(Device, dt)
    K.check_osc_poison(Device, dt)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_filter_rows_shared_filters_and_non_finite_samples(dt):
    K.check_fw_shared_equals_expanded(Device, dt)
    K.check_fw_rows(Device, dt)
    K.check_fw_nonfinite_stays_under_its_filter(Device)


def test_leading_axes_and_row_views_are_read_in_place():
    f, a = (t.to(DEV) for t in K.osc_inputs(2, K.CH + 1, 3, "f32"))
    want = F.oscillator_bank(f, a, K.SR)
    wide_f = torch.zeros(2, K.CH + 9, 3, device=DEV)
    wide_f[:, 5:K.CH + 6] = f
    assert torch.equal(F.oscillator_bank(wide_f[:, 5:K.CH + 6], a, K.SR), want)             # rows of a longer tensor
    assert torch.equal(F.oscillator_bank(f[None, :, None].expand(1, 2, 1, -1, -1), a[None, :, None], K.SR)[0, :, 0], want)
    assert torch.equal(F.oscillator_bank(f[0], a[0], K.SR), want[0])
    ft = f.transpose(1, 2).contiguous().transpose(1, 2)                                       # N is not innermost: gathered
    assert torch.equal(F.oscillator_bank(ft, a, K.SR), want)
    x, h = (t.to(DEV) for t in K.fw_inputs(2 * K.TILE, 2, 5, "f32", False))
    want = F.filter_waveform(x, h)
    wide_x = torch.zeros(2, 2 * K.TILE + 7, device=DEV)
    wide_x[:, 3:3 + 2 * K.TILE] = x
    assert torch.equal(F.filter_waveform(wide_x[:, 3:3 + 2 * K.TILE], h), want)              # a row view with an element offset
    assert torch.equal(F.filter_waveform(x[0], h), want[0])
    assert torch.equal(F.filter_waveform(x.reshape(2, 1, -1), h), want.reshape(2, 1, -1))
    xs = torch.stack([x, x], dim=-1)[..., 0]                                                 # a sample stride of 2: gathered
    assert torch.equal(F.filter_waveform(xs, h), want)


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_one_filter_is_convolve_same(dt):
    T, L = K.TILE + 3, 129
    rng = np.random.default_rng(9)
    x = torch.from_numpy(rng.standard_normal((2, T))).to(K.DTYPES[dt])
    h = torch.from_numpy(rng.standard_normal((1, L)) / np.sqrt(L)).to(K.DTYPES[dt])
    got = F.filter_waveform(x.to(DEV), h.to(DEV)).cpu()
    ref = F.convolve(x.to(DEV), h.to(DEV).expand(2, L), "same").cpu()
    want, mag = O.filter_waveform(K.wide(x), K.wide(h))
    bar = K.fw_bar(want, mag, L, dt)
    K.used(np.abs(got.double().numpy() - want), bar, f"filter_waveform with one filter {dt}")
    K.used(np.abs(got.double().numpy() - ref.double().numpy()), bar, f"filter_waveform against F.convolve {dt}")


def test_graph_capture_replays_the_eager_bits():
    f, a = (t.to(DEV) for t in K.osc_inputs(2, 2 * K.TILE, 3, "f32"))
    _, h = K.fw_inputs(2 * K.TILE, 2, 5, "f32", False)
    h = h.to(DEV)
    eager = F.filter_waveform(F.oscillator_bank(f, a, K.SR), h)
    static = f.clone()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        F.filter_waveform(F.oscillator_bank(static, a, K.SR), h)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = F.filter_waveform(F.oscillator_bank(static, a, K.SR), h)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    static.copy_(f * 0.5)                                                                    # the graph reads its inputs in place
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, F.filter_waveform(F.oscillator_bank(static, a, K.SR), h)) and not torch.equal(out, eager)


def test_refusals_on_the_device():
    f = torch.zeros(2, 8, 3, device=DEV)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.oscillator_bank(f, f.cpu(), 16000.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.filter_waveform(torch.zeros(2, 12, device=DEV), torch.zeros(4, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.extend_pitch(torch.zeros(4, 1, device=DEV), torch.zeros(2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.adsr_envelope(4, device="cpu")
    with pytest.raises(NotImplementedError, match=str(F.DSP_MAX_TAPS)):
        F.filter_waveform(torch.zeros(2, 12, device=DEV), torch.zeros(4, F.DSP_MAX_TAPS + 1, device=DEV))
    with pytest.raises(ValueError, match="multiple"):
        F.filter_waveform(torch.zeros(2, 12, device=DEV), torch.zeros(5, 3, device=DEV))
    with pytest.raises(TypeError, match="one dtype"):
        F.oscillator_bank(f, f.half(), 16000.0)
    assert F.oscillator_bank(f[:0], f[:0], 16000.0).shape == (0, 8)
    assert F.oscillator_bank(f[:, :0], f[:, :0], 16000.0, "none").shape == (2, 0, 3)
    assert torch.equal(F.oscillator_bank(f[:, :, :0], f[:, :, :0], 16000.0), torch.zeros(2, 8, device=DEV))
    assert F.filter_waveform(torch.zeros(0, 12, device=DEV), torch.zeros(4, 3, device=DEV)).shape == (0, 12)
    assert F.sinc_impulse_response(torch.zeros(0, device=DEV), 5).shape == (0, 5)
    assert F.frequency_impulse_response(torch.zeros(0, 4, device=DEV)).shape == (0, 6)
    assert not hasattr(torch.ops.audio_amd, "oscillator_bank")
    assert torch.equal(F.oscillator_bank(f, f, np.float32(16000.0)), F.oscillator_bank(f, f, 16000.0))
    env = F.adsr_envelope(11, attack=0.2, hold=0.4, decay=0.3, release=0.1, sustain=0.5)       # 1 + 2^-52 in float64
    assert env.shape == (11,) and env[0] == 0 and env[-1] == 0


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_frequency_impulse_response_at_the_limit(dt):
    """The largest LDS request of the family: 49 KB in float32, 98 KB (opted into) in float64."""
    n = F.DSP_MAX_MAGNITUDES
    m = torch.zeros(2, n, dtype=K.DTYPES[dt])
    m[0, :] = 1.0                                              # a flat response: a unit impulse at the centre, times the window
    m[1, 0] = 1.0                                              # the constant term alone: 1 / N everywhere, times the window
    got = F.frequency_impulse_response(m.to(DEV)).cpu()
    N = 2 * (n - 1)
    assert got.shape == (2, N) and got.dtype == K.DTYPES[dt]
    i = np.arange(N)
    win = 0.5 * (1.0 - np.cos(2.0 * np.pi * i / (N - 1)))
    want = np.zeros((2, N))
    want[0, N // 2] = win[N // 2]
    want[1] = win / N
    mag = np.stack([np.full(N, 1.0) * win, win / N])          # (sum_j c_j |m_j|) / N * window: N / N and 1 / N
    K.used(np.abs(got.double().numpy() - want), (n + 4) * K.EPS[K.DTYPES[dt]] * mag, f"frequency_impulse_response {dt} n={n}")


# ---- the differentiable compositions ---------------------------------------------------------------------------------------------

def test_compositions_agree_with_the_kernels_in_float64():
    f, a = (t.to(DEV) for t in K.osc_inputs(2, K.CH + 1, 3, "f64"))
    for red in ("sum", "mean", "none"):
        want, mag, own = K.osc_oracle(2, K.CH + 1, 3, "f64", red)
        got = F.oscillator_bank(f.clone().requires_grad_(), a, K.SR, red)
        assert got.requires_grad and got.dtype == torch.float64
        bar = K.osc_bar(want, mag, own, 3, "f64", red)
        K.used(np.abs(got.detach().cpu().numpy() - want), bar, f"_diff.oscillator_bank {red}")
        kern = F.oscillator_bank(f, a, K.SR, red)                  # each is within the bar of the oracle: twice the bar apart at most
        K.used((got.detach() - kern).abs().cpu().numpy(), 2 * bar, f"_diff.oscillator_bank {red} against the kernel")
    for T, Fn, L, batched in ((2 * K.TILE, 2, 5, False), (96, 3, 129, True)):
        x, h = (t.to(DEV) for t in K.fw_inputs(T, Fn, L, "f64", batched))
        want, mag = K.fw_oracle(T, Fn, L, "f64", batched)
        got = F.filter_waveform(x, h.clone().requires_grad_())
        assert got.requires_grad
        K.used(np.abs(got.detach().cpu().numpy() - want), K.fw_bar(want, mag, L, "f64"), "_diff.filter_waveform")
        K.used((got.detach() - F.filter_waveform(x, h)).abs().cpu().numpy(), 2 * K.fw_bar(want, mag, L, "f64"),
               "_diff.filter_waveform against the kernel")
    cut = torch.tensor(K.SINC_CUT, dtype=torch.float64, device=DEV)
    for hp in (False, True):
        got = F.sinc_impulse_response(cut.clone().requires_grad_(), 513, hp)
        o64 = O.sinc_impulse_response(cut.cpu().numpy(), 513, hp)
        old = O.sinc_impulse_response(cut.cpu().numpy(), 513, hp, acc=O.LD)
        bar = np.maximum(4.0 * float(np.abs(o64 - old).max()), 4.0 * np.spacing(np.abs(o64).max(axis=-1, keepdims=True)))
        K.used(np.abs(got.detach().cpu().numpy() - o64), np.broadcast_to(bar, o64.shape), "_diff.sinc_impulse_response")
        K.used((got.detach() - F.sinc_impulse_response(cut, 513, hp)).abs().cpu().numpy(), np.broadcast_to(2 * bar, o64.shape),
               "_diff.sinc_impulse_response against the kernel")
    m = torch.from_numpy(np.random.default_rng(129).uniform(0.0, 1.0, (2, 129))).to(DEV)
    want, mag = O.frequency_impulse_response(m.cpu().numpy())
    got = F.frequency_impulse_response(m.clone().requires_grad_())
    K.used(np.abs(got.detach().cpu().numpy() - want), (129 + 4) * 2.0 ** -53 * mag, "_diff.frequency_impulse_response")
    K.used((got.detach() - F.frequency_impulse_response(m)).abs().cpu().numpy(), 2 * (129 + 4) * 2.0 ** -53 * mag,
           "_diff.frequency_impulse_response against the kernel")


def test_gradcheck_of_the_compositions():
    rng = np.random.default_rng(11)
    T, N, L = 24, 3, 5
    f = torch.from_numpy(rng.uniform(100.0, 3000.0, (2, T, N))).to(DEV).requires_grad_()
    a = torch.from_numpy(rng.uniform(-1.0, 1.0, (2, T, N))).to(DEV).requires_grad_()
    for red in ("sum", "mean", "none"):
        assert torch.autograd.gradcheck(lambda f_, a_: F.oscillator_bank(f_, a_, K.SR, red), (f, a))
    assert torch.autograd.gradgradcheck(lambda f_, a_: _diff.oscillator_bank(f_, a_, K.SR, "sum"), (f[:1, :6], a[:1, :6]))
    x = torch.from_numpy(rng.standard_normal((2, T))).to(DEV).requires_grad_()
    for h in (rng.standard_normal((4, L)), rng.standard_normal((2, 24, 4)), rng.standard_normal((3, 1))):
        h = torch.from_numpy(h).to(DEV).requires_grad_()
        assert torch.autograd.gradcheck(F.filter_waveform, (x, h))
    assert torch.autograd.gradgradcheck(F.filter_waveform, (x[:1, :8], torch.from_numpy(rng.standard_normal((2, 3))).to(DEV).requires_grad_()))
    cut = torch.tensor([0.1, 0.45, 0.9], dtype=torch.float64, device=DEV).requires_grad_()
    for hp in (False, True):
        assert torch.autograd.gradcheck(lambda c: F.sinc_impulse_response(c, 9, hp), (cut,))
    assert torch.autograd.gradgradcheck(lambda c: F.sinc_impulse_response(c, 5, False), (cut,))
    m = torch.from_numpy(rng.uniform(0.1, 1.0, (2, 5))).to(DEV).requires_grad_()
    assert torch.autograd.gradcheck(F.frequency_impulse_response, (m,))
    base = torch.from_numpy(rng.uniform(50.0, 500.0, (2, 6, 1))).to(DEV).requires_grad_()
    assert torch.autograd.gradcheck(lambda b: F.extend_pitch(b, 3), (base,))
    with torch.no_grad():
        assert not F.oscillator_bank(f, a, K.SR).requires_grad                               # the kernels, under no_grad
