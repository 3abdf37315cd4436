"""The separation metrics without a GPU: identities of the oracle (tests/sdr_oracle.py) and the host-side errors of the entry
points, which are raised before anything touches a device."""
import numpy as np
import pytest
import torch

import sdr_oracle as O
import audio_amd.functional as F

P, T = O.signals(700)
SI = [F.scale_invariant_signal_distortion_ratio, F.scale_invariant_signal_noise_ratio, F.signal_noise_ratio]
ALL = SI + [F.signal_distortion_ratio]


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.longdouble])
def test_si_sdr_of_a_scaled_target_sits_at_the_eps_ceiling(dtype):
    """preds = c target leaves only eps in the denominator: about 10 log10(sum t^2 / eps), far above any real score."""
    eps = np.finfo(np.float32).eps if dtype == np.float32 else np.finfo(np.float64).eps
    got = O.si_sdr(0.5 * T[0], T[0], False, dtype, eps)
    assert got > 10 * np.log10(1 / eps) - 30 and np.isfinite(got)


@pytest.mark.parametrize("row", range(3))
def test_oracle_identities(row):
    p, t = P[row] + 0.25, T[row] - 0.5
    assert O.si_snr(p, t) == O.si_sdr(p, t, True)
    assert abs(O.si_sdr(3.0 * p, t) - O.si_sdr(p, t)) < 1e-6                # up to the eps terms (1.2e-7 against sums of order 1e3)
    want = O.sdr_longdouble(p, t, 32)
    assert abs(O.sdr_float64(p, t, 32) - want) < 1e-8
    for cp, ct in ((7.0, 1.0), (1.0, 1e-3), (-2.0, 5.0)):                  # SDR ignores the scale of either input
        assert abs(O.sdr_longdouble(cp * p, ct * t, 32) - want) < 1e-9
    assert O.sdr_longdouble(p, t, 32, zero_mean=True) == pytest.approx(O.sdr_longdouble(p - p.mean(), t - t.mean(), 32), abs=1e-9)
    assert O.sdr_longdouble(p, t, 32, load_diag=0.1) < want                  # a loaded diagonal explains less of preds
    assert np.isnan(O.sdr_longdouble(p, 0 * t, 8)) and np.isnan(O.sdr_float64(p, 0 * t, 8))


@pytest.mark.parametrize("fn", ALL)
def test_host_side_errors(fn):
    x = torch.zeros(2, 16)
    with pytest.raises(ValueError, match="same shape"):
        fn(x, torch.zeros(2, 15))
    with pytest.raises(ValueError, match=r"expects \(\.\.\., time\)"):
        fn(torch.tensor(1.0), torch.tensor(1.0))
    with pytest.raises(ValueError, match="lengths must have the shape"):
        fn(x, x, lengths=torch.zeros(3, dtype=torch.int32))
    with pytest.raises(TypeError, match="float16, bfloat16, float32 or float64"):
        fn(x.int(), x.int())
    with pytest.raises(TypeError, match="share a dtype"):
        fn(x, x.double())
    with pytest.raises(TypeError, match="int32 or int64"):
        fn(x, x, lengths=torch.zeros(2))
    with pytest.raises(RuntimeError, match=r"preds must be on an MI355X \(ROCm\) device.*no CPU fallback"):
        fn(x, x)


def test_sdr_parameter_errors():
    x = torch.zeros(2, 16)
    with pytest.raises(NotImplementedError, match="filter_length above 512"):
        F.signal_distortion_ratio(x, x, filter_length=513)
    with pytest.raises(ValueError, match="filter_length must be a positive integer"):
        F.signal_distortion_ratio(x, x, filter_length=0)
    with pytest.raises(RuntimeError, match="signal_distortion_ratio is forward-only"):
        F.signal_distortion_ratio(x.clone().requires_grad_(), x)
