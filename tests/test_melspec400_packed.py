"""The headline instantiation of the n_fft = 400 kernel (hop 160, 80-mel HTK bank) can issue its paired operations as packed
fp32 (csrc/melspec400.h, AR_PK_*, one compile-time switch per phase); `POLICY_MEL400_SCALAR` routes the same shape to its scalar
twin, which performs the same IEEE operations one instruction each.  The two must agree bit for bit, on ordinary and on special
values, and both must meet the float64 oracle at the bar of the other mel tests (1e-4 of the peak).

Shapes: the smallest that reach every branch of the tile loop (tests/test_melspec400_tile_trim.py):
  short      3 x 5 920    a clip shorter than two interior tiles, both edges unstaged
  cross5     5 x 20 800   rows crossed in mid-claim, frames % 6 = 5
  cross0     5 x 20 960   frames % 6 = 0
  unaligned  a view one sample into 5 x 20 801: no tile is staged
  special    4 x 20 800   rows of zeros, denormals, full-scale +-1, and samples with +-inf and NaN among them

The product ships with every packed phase switched off (none beat the scalar stream), so both paths run the pinned
scalar kernel today.  Built with all three AAMD_M400_PK_* switches on, the four ordinary cases and the oracle comparisons passed
(peak-relative error 3.4e-6 .. 4.7e-6 on either path) and the special-values comparison FAILED: the inf / NaN row came out with
other NaN bit patterns than the scalar twin's.  A phase that is switched on later has to pass this file as it stands."""
import functools

import numpy as np
import pytest
import torch

from conftest import peak_rel_err

pytestmark = pytest.mark.gpu

# name: (rows, length of the buffer, view offset)
CASES = {
    "short": (3, 5920, 0),
    "cross5": (5, 20800, 0),
    "cross0": (5, 20960, 0),
    "unaligned": (5, 20801, 1),
}


def case_input(name):
    rows, length, off = CASES[name]
    x = 0.5 * np.random.RandomState(7000 + sorted(CASES).index(name)).standard_normal((rows, length))
    return np.clip(x, -1.0, 1.0).astype(np.float32)


def special_input():
    rs = np.random.RandomState(7100)
    x = np.zeros((4, 20800), dtype=np.float32)
    x[1] = (rs.standard_normal(20800) * 1e-40).astype(np.float32)          # denormals
    x[2] = np.where(rs.rand(20800) < 0.5, -1.0, 1.0).astype(np.float32)    # full scale
    x[3] = np.clip(0.5 * rs.standard_normal(20800), -1.0, 1.0).astype(np.float32)
    x[3, 3000] = np.inf
    x[3, 7001] = -np.inf
    x[3, 11000:11003] = np.nan
    x[3, 15000] = np.inf
    x[3, 15100] = np.nan
    assert (np.abs(x[1][x[1] != 0]) < np.finfo(np.float32).tiny).all()
    return x


@functools.lru_cache(maxsize=None)
def both_paths(name):
    """(packed, scalar) outputs of the case as host arrays, computed once for all tests."""
    import audio_amd.transforms as T
    from audio_amd import _lib
    if name == "special":
        x, off = special_input(), 0
    else:
        x, off = case_input(name), CASES[name][2]
    xd = torch.from_numpy(x).cuda()[:, off:]
    t = T.MelSpectrogram(sample_rate=16000, n_fft=400, hop_length=160, n_mels=80).cuda()
    packed = t(xd).cpu().numpy()
    with _lib.kernel_policy(_lib.POLICY_MEL400_SCALAR):
        scalar = t(xd).cpu().numpy()
    return packed, scalar


@functools.lru_cache(maxsize=None)
def oracle(name):
    from oracle import dsp_oracle as O
    rows, length, off = CASES[name]
    fb = O.melscale_fbanks(201, 0.0, 8000.0, 80, 16000)
    return O.mel_spectrogram(case_input(name)[:, off:].astype(np.float64), O.hann_window(400), fb, 400, 160)


@pytest.mark.parametrize("name", sorted(CASES))
def test_packed_equals_scalar_bit_for_bit(name):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    packed, scalar = both_paths(name)
    assert packed.shape == scalar.shape and packed.dtype == np.float32
    assert np.isfinite(packed).all()
    assert np.array_equal(packed.view(np.int32), scalar.view(np.int32))


def test_special_values_propagate_as_in_the_scalar_twin():
    """Zeros, denormals, full scale, +-inf and NaN: each packed half gives exactly what the scalar instruction gives."""
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    packed, scalar = both_paths("special")
    assert np.array_equal(packed.view(np.int32), scalar.view(np.int32))
    assert (packed[0] == 0.0).all()                          # the row of zeros
    assert np.isfinite(packed[:3]).all() and (packed[2] > 0).any()
    assert np.isnan(packed[3]).any() and np.isfinite(packed[3]).any()      # the inf / NaN frames and the clean ones between them


@pytest.mark.parametrize("path", ["packed", "scalar"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_both_paths_against_the_oracle(name, path):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    got = both_paths(name)[0 if path == "packed" else 1]
    exp = oracle(name)
    assert got.shape == exp.shape
    err = peak_rel_err(got, exp)
    print(name, path, "peak_rel_err", err)
    assert err <= 1e-4, (name, path, err)
