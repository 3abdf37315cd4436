"""The tile loop of the n_fft = 400 kernel after its bookkeeping was trimmed (csrc/melspec400.h: the tile's row, position and
row offsets are carried from claim to claim, the staging test is two 32-bit compares, the signature instantiation's stores
take a scalar base): every branch touched, at the smallest shapes that reach it, against the float64 oracle with the
tolerance of the other mel tests (1e-4 of the peak).

Shapes (hop 160 unless stated; tiles_per_row = ceil(frames / 6); rows of >= 16 tiles carry, shorter ones divide):
  short      3 x 5 920      7 tiles per row: a clip shorter than two interior tiles, division path, both edges unstaged
  cross5     5 x 20 800     22 tiles per row, 8 workgroups of 14 tiles: runs cross row boundaries in mid-claim; frames % 6 = 5
  cross0     5 x 20 960     frames = 132 = 0 (mod 6)
  unaligned  5 x 20 800     a view one sample into a wider buffer: no tile is staged, every gather is the direct one
  many       40 x 16 000    17 tiles per row, 56 workgroups of 13 tiles: every wave steps over row boundaries
  tiny       4000 x 1 600   2 tiles per row, 8 000 tiles > 256 x 12 waves, 250 of 256 workgroups get tiles
  mels64     5 x 20 800     n_mels = 64: the generic NR = 4 instantiation (its stores keep the per-lane form)
  hop100 / hop200           5 x 20 800 at the two other hops of the kernel
  complex    5 x 20 800     Spectrogram(power=None): the complex epilogue, whose row offset is carried as well

Bit equality with the commit before the change: tests/golden/melspec400_tile_trim_parent.json holds, per case, the SHA-256
of the input and of the output that commit produced on an MI355X; where the input generated here hashes the same, the output
must too (nothing in the change may alter a rounding)."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from conftest import peak_rel_err

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "melspec400_tile_trim_parent.json")

# name: (kind, rows, length of the buffer, view offset, hop, n_mels)
CASES = {
    "short": ("mel", 3, 5920, 0, 160, 80),
    "cross5": ("mel", 5, 20800, 0, 160, 80),
    "cross0": ("mel", 5, 20960, 0, 160, 80),
    "unaligned": ("mel", 5, 20801, 1, 160, 80),
    "many": ("mel", 40, 16000, 0, 160, 80),
    "tiny": ("mel", 4000, 1600, 0, 160, 80),
    "mels64": ("mel", 5, 20800, 0, 160, 64),
    "hop100": ("mel", 5, 20800, 0, 100, 80),
    "hop200": ("mel", 5, 20800, 0, 200, 80),
    "complex": ("spec_complex", 5, 20800, 0, 160, 0),
}


def case_input(name):
    """The case's waveform (float32, host): MT19937 normal samples, the same on every machine."""
    kind, rows, length, off, hop, n_mels = CASES[name]
    seed = 1000 + sorted(CASES).index(name)
    x = 0.5 * np.random.RandomState(seed).standard_normal((rows, length))
    return np.clip(x, -1.0, 1.0).astype(np.float32)


def case_run(name, x):
    """The product's output for the case as a host array."""
    import audio_amd.transforms as T
    kind, rows, length, off, hop, n_mels = CASES[name]
    xd = torch.from_numpy(x).cuda()[:, off:]
    if kind == "mel":
        t = T.MelSpectrogram(sample_rate=16000, n_fft=400, hop_length=hop, n_mels=n_mels).cuda()
    else:
        t = T.Spectrogram(n_fft=400, hop_length=hop, power=None).cuda()
    return t(xd).cpu().numpy()


def case_oracle(name, x):
    from oracle import dsp_oracle as O
    kind, rows, length, off, hop, n_mels = CASES[name]
    x64 = x[:, off:].astype(np.float64)
    if kind == "mel":
        fb = O.melscale_fbanks(201, 0.0, 8000.0, n_mels, 16000)
        return O.mel_spectrogram(x64, O.hann_window(400), fb, 400, hop)
    return O.spectrogram(x64, 0, O.hann_window(400), 400, hop, 400, None, False)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.fixture(scope="module")
def golden():
    if not os.path.exists(GOLDEN):      # no saved parent output: the oracle comparison stands alone
        return {}
    with open(GOLDEN, encoding="ascii") as f:
        return json.load(f)


@pytest.mark.parametrize("name", sorted(CASES))
def test_tile_trim_against_oracle_and_parent(name, golden):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    x = case_input(name)
    got = case_run(name, x)
    exp = case_oracle(name, x)
    assert got.shape == exp.shape
    err = peak_rel_err(got, exp)
    print(name, "peak_rel_err", err)
    assert np.isfinite(got).all()
    assert err <= 1e-4, (name, err)
    g = golden.get(name)
    if g is not None and sha(x) == g["input_sha256"]:      # the saved parent-commit output belongs to this very input
        assert sha(got) == g["output_sha256"], f"{name}: output differs from the parent commit's bit pattern"
