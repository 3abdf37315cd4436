"""The backward kernels of oscillator_bank and filter_waveform on the device, through F.*(...).backward(): the checks of
tests/test_dsp_grad.py (dsp_grad_cases.py) against tests/dsp_grad_oracle.py, then what only the product has: the forward under
grad is the forward under no_grad bit for bit, only the wanted gradients are computed, gradcheck in float64, a non-contiguous
cotangent, leading axes, and the memory the filter's training path may take."""
import numpy as np
import pytest
import torch

import dsp_cases as K
import dsp_grad_cases as GK
import audio_amd.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"


class Device:
    """The backend of dsp_grad_cases: the entry points on the device, differentiated by autograd."""

    @staticmethod
    def grad_tiles():
        return F.dsp_grad_tiles()

    @staticmethod
    def osc_grad(f, a, g, sample_rate, reduction, want=(True, True)):
        f, a = f.to(DEV).requires_grad_(want[0]), a.to(DEV).requires_grad_(want[1])
        F.oscillator_bank(f, a, sample_rate, reduction).backward(g.to(DEV))
        return tuple(None if t.grad is None else t.grad.cpu() for t in (f, a))

    @staticmethod
    def fw_grad(x, h, g, want=(True, True)):
        x, h = x.to(DEV).requires_grad_(want[0]), h.to(DEV).requires_grad_(want[1])
        F.filter_waveform(x, h).backward(g.to(DEV))
        return tuple(None if t.grad is None else t.grad.cpu() for t in (x, h))


def test_tiles_are_what_the_cases_straddle():
    assert Device.grad_tiles() == (GK.PIECE, GK.LAGS)
    assert F.dsp_tiles() == (K.CH, K.TILE, F.DSP_MAX_TAPS, F.DSP_MAX_OSCILLATORS, F.DSP_MAX_MAGNITUDES)


# ---- accuracy ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("N", K.OSC_N)
@pytest.mark.parametrize("T", K.OSC_T)
def test_oscillator_bank_grad_within_the_bars(T, N, dt):
    GK.check_osc_grad(Device, 2, T, N, dt)


@pytest.mark.parametrize("dt", list(K.DTYPES))
@pytest.mark.parametrize("reduction", ["sum", "mean", "none"])
def test_oscillator_bank_grad_reductions_and_half_types(reduction, dt):
    GK.check_osc_grad(Device, 2, K.CH + 1, 3, dt, reduction)


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("batched", [False, True])
@pytest.mark.parametrize("shape", GK.FW_GRAD_SHAPES)
def test_filter_waveform_grad_within_the_bars(shape, batched, dt):
    GK.check_fw_grad(Device, *shape, dt, batched)


@pytest.mark.parametrize("dt", list(K.DTYPES))
def test_filter_waveform_grad_half_types_and_one_filter_over_three_rows(dt):
    for batched in (False, True):
        GK.check_fw_grad(Device, 2 * K.TILE, 2, 5, dt, batched)
        GK.check_fw_grad(Device, *GK.FW_ONE_FILTER, dt, batched, rows=3)


# ---- exact properties --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_oscillator_grad_prefix_rows_and_poison(dt):
    GK.check_osc_grad_prefix(Device, dt)
    GK.check_osc_grad_rows(Device, dt)
    GK.check_osc_grad_poison(Device, dt)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_filter_grad_rows_shared_filters_and_non_finite_cotangents(dt):
    GK.check_fw_grad_exact(Device, dt)
    GK.check_fw_grad_nonfinite_stays_under_its_filter(Device)


def test_only_the_wanted_gradients_are_computed():
    GK.check_only_what_is_wanted(Device)


# ---- what only the product has -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", list(K.DTYPES))
def test_the_forward_under_grad_is_the_forward_under_no_grad(dt):
    f, a = (t.to(DEV) for t in K.osc_inputs(2, K.CH + 1, 3, dt))
    for red in ("sum", "mean", "none"):
        y = F.oscillator_bank(f.clone().requires_grad_(), a.clone().requires_grad_(), K.SR, red)
        assert y.requires_grad and type(y.grad_fn).__name__ == "_OscillatorBankFunctionBackward"
        with torch.no_grad():
            assert torch.equal(y, F.oscillator_bank(f, a, K.SR, red))
    for batched in (False, True):
        x, h = (t.to(DEV) for t in K.fw_inputs(2 * K.TILE, 2, 5, dt, batched))
        y = F.filter_waveform(x.clone().requires_grad_(), h.clone().requires_grad_())
        assert y.requires_grad and type(y.grad_fn).__name__ == "_FilterWaveformFunctionBackward"
        with torch.no_grad():
            assert torch.equal(y, F.filter_waveform(x, h))


def test_gradcheck_of_the_kernels_in_float64():
    rng = np.random.default_rng(21)
    f = torch.from_numpy(rng.uniform(100.0, 3000.0, (2, 12, 3))).to(DEV).requires_grad_()
    a = torch.from_numpy(rng.uniform(-1.0, 1.0, (2, 12, 3))).to(DEV).requires_grad_()
    for red in ("sum", "mean", "none"):
        assert torch.autograd.gradcheck(lambda f_, a_: F.oscillator_bank(f_, a_, K.SR, red), (f, a))
    x = torch.from_numpy(rng.standard_normal((2, 24))).to(DEV).requires_grad_()
    for shape in ((3, 4), (2, 3, 5)):
        h = torch.from_numpy(rng.standard_normal(shape)).to(DEV).requires_grad_()
        assert torch.autograd.gradcheck(F.filter_waveform, (x, h))


def test_a_non_contiguous_cotangent_and_leading_axes():
    x, h = (t.to(DEV) for t in K.fw_inputs(2 * K.TILE, 2, 5, "f32", False))
    g = GK.fw_cotangent(2 * K.TILE, "f32").to(DEV)
    want = Device.fw_grad(x.cpu(), h.cpu(), g.cpu())
    gt = g.t().contiguous().t()                                            # the same values, time no longer innermost
    assert not gt.is_contiguous()
    xr, hr = x.clone().requires_grad_(), h.clone().requires_grad_()
    F.filter_waveform(xr, hr).backward(gt)
    assert torch.equal(xr.grad.cpu(), want[0]) and torch.equal(hr.grad.cpu(), want[1])
    xr, hr = x.reshape(2, 1, -1).clone().requires_grad_(), h.clone().requires_grad_()   # a leading axis, a summed loss
    F.filter_waveform(xr, hr).backward(g.reshape(2, 1, -1))
    assert xr.grad.shape == xr.shape and torch.equal(xr.grad.reshape(2, -1).cpu(), want[0]) and torch.equal(hr.grad.cpu(), want[1])
    f, a = (t.to(DEV) for t in K.osc_inputs(2, K.CH + 1, 3, "f32"))
    go = GK.osc_cotangent(2, K.CH + 1, 3, "f32", "none").to(DEV)
    want = Device.osc_grad(f.cpu(), a.cpu(), go.cpu(), K.SR, "none")
    got = go.transpose(1, 2).contiguous().transpose(1, 2)
    assert not got.is_contiguous()
    fr, ar = f[:, None].clone().requires_grad_(), a[:, None].clone().requires_grad_()
    F.oscillator_bank(fr, ar, K.SR, "none").backward(got[:, None])
    assert fr.grad.shape == fr.shape and torch.equal(fr.grad[:, 0].cpu(), want[0]) and torch.equal(ar.grad[:, 0].cpu(), want[1])


def test_the_training_path_of_the_filter_allocates_no_gather():
    """float32 (4, 16384) through shared (16, 257) filters, both gradients: x, h, y, g, the gradients and a float64 workspace of
    rows * F * L partial sums are under 2 MB together; one (rows, T, L) float32 gather is 67 MB.  The peak may rise by less than
    an eighth of that."""
    rows, T, Fn, L = 4, 16384, 16, 257
    rng = np.random.default_rng(5)
    x = torch.from_numpy(rng.standard_normal((rows, T))).float().to(DEV).requires_grad_()
    h = torch.from_numpy(rng.standard_normal((Fn, L)) / np.sqrt(L)).float().to(DEV).requires_grad_()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    F.filter_waveform(x, h).sum().backward()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"peak memory rose by {rise} bytes; the bar is {rows * T * L * 4 // 8}")
    assert x.grad is not None and h.grad is not None
    assert rise < rows * T * L * 4 / 8
