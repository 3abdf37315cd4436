"""F.stoi on the MI355X against the float64 definition of tests/stoi_oracle.py.  The bar is computed from the oracle alone, per
mode: 4 x the largest |d32 - d64| over the file's cases, d32 the definition with the window products, overlap-add, transform,
band sums and square root in float32 (scipy's single-precision rfft); the margin of 4 is for the kernel's transform ordering
its sums differently.  Everything else here is bit for bit: calls against calls.  Rows have at most 30000 samples, batches at
most 8 rows; the reference of a case is computed once (stoi_oracle.case) and shared."""
import numpy as np
import pytest
import torch

import stoi_oracle as O
import audio_amd.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
MODES = [False, True]
CASE_NAMES = [c[0] for c in O.CASES]
TILES = (256, 8, 8, 16, 64)


def dev(a, dtype=None):
    t = torch.from_numpy(np.array(a)).to(DEV)                           # a copy: the shared references are read-only
    return t if dtype is None else t.to(dtype)


def same_bits(a, b):
    ints = {torch.float32: torch.int32, torch.float64: torch.int64}
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(ints[a.dtype]), b.view(ints[b.dtype]))


def mixed_batch(T=30000):
    """The nine cases in two batches' worth of rows, zero-padded to T, with their lengths: (target, preds, lengths, names)."""
    xs, ys = np.zeros((len(CASE_NAMES), T), np.float32), np.zeros((len(CASE_NAMES), T), np.float32)
    lens = np.zeros((len(CASE_NAMES),), np.int64)
    for b, name in enumerate(CASE_NAMES):
        x, y = O.case(name)[:2]
        xs[b, :len(x)], ys[b, :len(y)], lens[b] = x, y, len(x)
    return xs, ys, lens


def test_tiles_are_the_exported_constants():
    assert F.stoi_tiles() == TILES


@pytest.mark.parametrize("extended", MODES)
def test_every_case_meets_the_bar(extended):
    bar = O.bar(extended)
    for name in CASE_NAMES:
        x, y, scores, kept, margin = O.case(name)
        assert margin > 1e-6                                            # a condition of the case: the kept set is unambiguous
        d64 = scores[extended][0]
        got = F.stoi(dev(y), dev(x), 10000, extended)
        assert got.shape == () and got.dtype == torch.float32 and got.device.type == "cuda"
        err = abs(float(got) - d64)
        print(f"{name} extended={extended}: got {float(got):.9f} d64 {d64:.9f} err {err:.3e} bar {bar:.3e}")
        if d64 == O.SHORT:
            assert float(got) == float(np.float32(1e-5))
        assert err <= bar, (name, float(got), d64, bar)


@pytest.mark.parametrize("extended", MODES)
def test_mixed_batch_with_lengths_meets_the_bar_and_equals_the_single_rows(extended):
    xs, ys, lens = mixed_batch()
    bar = O.bar(extended)
    for lo, hi in ((0, 8), (8, len(CASE_NAMES))):
        for ldt in (torch.int64, torch.int32):
            got = F.stoi(dev(ys[lo:hi]), dev(xs[lo:hi]), 10000, extended, lengths=dev(lens[lo:hi], ldt))
            assert got.shape == (hi - lo,)
            for b in range(lo, hi):
                d64 = O.case(CASE_NAMES[b])[2][extended][0]
                assert abs(float(got[b - lo]) - d64) <= bar, (CASE_NAMES[b], float(got[b - lo]), d64, bar)
                alone = F.stoi(dev(ys[b, :lens[b]]), dev(xs[b, :lens[b]]), 10000, extended)
                assert same_bits(got[b - lo], alone), (CASE_NAMES[b], float(got[b - lo]), float(alone))
    assert float(got[-1]) == float(np.float32(1e-5))                    # L6000_s0: 19 kept frames


@pytest.mark.parametrize("extended", MODES)
def test_batch_rows_equal_single_rows_and_two_calls_agree(extended):
    names = ["L30000_s0_20dB", "L30000_s1_5dB", "L30000_s2_m5dB", "L30000_s3_5dB"]
    x = dev(np.stack([O.case(n)[0] for n in names]))
    y = dev(np.stack([O.case(n)[1] for n in names]))
    a = F.stoi(y.view(2, 2, -1), x.view(2, 2, -1), 10000, extended)
    b = F.stoi(y.view(2, 2, -1), x.view(2, 2, -1), 10000, extended)
    assert a.shape == (2, 2) and same_bits(a, b)
    for r in range(4):
        assert same_bits(a.view(-1)[r], F.stoi(y[r], x[r], 10000, extended))
    wide = torch.zeros((4, 30011), device=DEV)                          # rows at a stride that is no multiple of 16 bytes
    wide[:, 3:30003] = y
    assert same_bits(a.view(-1), F.stoi(wide[:, 3:30003], x, 10000, extended))


@pytest.mark.parametrize("extended", MODES)
def test_other_dtypes(extended):
    """float64 meets the float32 bar and returns float64; float16 / bfloat16 equal the call on the widened tensor."""
    bar = O.bar(extended)
    for name in ("L30000_s1_5dB", "L12000_s1_m5dB", "L6000_s0_5dB"):
        x, y, scores, _, _ = O.case(name)
        got = F.stoi(dev(y, torch.float64), dev(x, torch.float64), 10000, extended)
        assert got.dtype == torch.float64 and abs(float(got) - scores[extended][0]) <= bar
    x, y = O.case("L12000_s1_5dB")[:2]
    for dt in (torch.float16, torch.bfloat16):
        xh, yh = dev(np.stack([x, x]), dt), dev(np.stack([y, x]), dt)
        got = F.stoi(yh, xh, 10000, extended)
        assert got.dtype == torch.float32 and same_bits(got, F.stoi(yh.float(), xh.float(), 10000, extended))


def test_16_khz_goes_through_the_package_resampler():
    g = torch.Generator().manual_seed(5)
    t = (0.1 * torch.randn((3, 30000), generator=g)).to(DEV)
    p = t + (0.05 * torch.randn((3, 30000), generator=g)).to(DEV)
    lens = torch.tensor([30000, 17001, 8000], device=DEV)
    for extended in MODES:
        want = F.stoi(F.resample(p, 16000, 10000), F.resample(t, 16000, 10000), 10000, extended)
        got = F.stoi(p, t, 16000, extended)
        assert same_bits(got, want) and 0.0 < float(got.min()) and float(got.max()) < 1.0
        want = F.stoi(F.resample(p, 16000, 10000), F.resample(t, 16000, 10000), 10000, extended,
                      lengths=torch.ceil(lens * 10000 / 16000).to(lens.dtype))
        assert same_bits(F.stoi(p, t, 16000, extended, lengths=lens), want)


def test_non_finite_rows_and_bad_lengths_score_nan_and_neighbours_keep_their_bits():
    names = ["L12000_s1_5dB", "L12000_s1_m5dB", "L12000_s1_5dB", "L12000_s1_m5dB"]
    x = dev(np.stack([O.case(n)[0] for n in names]))
    y = dev(np.stack([O.case(n)[1] for n in names]))
    for extended in MODES:
        clean = F.stoi(y, x, 10000, extended)
        for where, value, signal in ((0, float("nan"), y), (11999, float("inf"), y), (5000, float("-inf"), x)):
            s2 = signal.clone()
            s2[1, where] = value
            got = F.stoi(s2 if signal is y else y, s2 if signal is x else x, 10000, extended)
            assert torch.isnan(got[1]) and same_bits(got[[0, 2, 3]], clean[[0, 2, 3]])
        y2 = y.clone()
        y2[1, 9000:] = float("nan")                                     # at and beyond the length: never read
        lens = torch.tensor([12000, 9000, 12001, -1], device=DEV)
        got = F.stoi(y2, x, 10000, extended, lengths=lens)
        assert same_bits(got[0], clean[0]) and torch.isnan(got[2]) and torch.isnan(got[3])
        assert same_bits(got[1], F.stoi(y[1, :9000], x[1, :9000], 10000, extended))


def test_empty_and_too_short_inputs():
    assert F.stoi(torch.zeros((0, 500), device=DEV), torch.zeros((0, 500), device=DEV), 10000).shape == (0,)
    for T in (0, 1, 255, 256, 4095):
        got = F.stoi(torch.ones((2, T), device=DEV), torch.ones((2, T), device=DEV), 10000)
        assert got.tolist() == [float(np.float32(1e-5))] * 2


def test_a_captured_call_replays_the_eager_result():
    """No table is cached (the window and the twiddles are computed in the kernels), so nothing has to be warmed; the issue's
    form, a second call captured, is what runs here.  The process keeps its default number of hardware queues."""
    x, y = O.case("L30000_s3_5dB")[:2]
    t, p = dev(np.stack([x, x])), dev(np.stack([y, x]))
    eager = [F.stoi(p, t, 10000, ext) for ext in MODES]
    st, sp = torch.zeros_like(t), torch.zeros_like(p)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        F.stoi(sp, st, 10000)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = [F.stoi(sp, st, 10000, ext) for ext in MODES]
    st.copy_(t)
    sp.copy_(p)
    g.replay()
    torch.cuda.synchronize()
    for out, want in zip(outs, eager):
        assert same_bits(out, want)


def test_forward_only_and_cpu_tensors():
    t = torch.zeros((2, 5000), device=DEV)
    with pytest.raises(RuntimeError, match="stoi is forward-only"):
        F.stoi(t.clone().requires_grad_(), t, 10000)
    with torch.no_grad():
        assert F.stoi(t.clone().requires_grad_(), t, 10000).shape == (2,)
    with pytest.raises(RuntimeError, match=r"target must be on an MI355X \(ROCm\) device.*no CPU fallback"):
        F.stoi(t, t.cpu(), 10000)
    with pytest.raises(RuntimeError, match=r"lengths must be on an MI355X \(ROCm\) device.*no CPU fallback"):
        F.stoi(t, t, 10000, lengths=torch.tensor([5000, 5000]))
