"""F.vad / F.vad_start / T.Vad on the device through the product API, against tests/vad_oracle.py: the trigger entry with
synthetic measurements (exact), the measurements within 4 x the difference of the oracle's own two forms, vad_start and vad
against the oracle's trigger on the device's own measurements (exact), vad_start against the float64 oracle where it has
margin, views, warnings, graph capture and bit-reproducibility.  The checks are those of tests/test_vad.py (vad_cases.py);
the shapes are the smallest that reach every transform size and more rows than a wave has lanes."""
import warnings

import numpy as np
import pytest
import torch

import vad_cases as K
import vad_oracle as O
import audio_amd.functional as F
import audio_amd.transforms as T

pytestmark = pytest.mark.gpu
DEV = "cuda"


class Device:
    """The backend of vad_cases: the product's private entry points on the device."""

    @staticmethod
    def tensor(a):
        return torch.from_numpy(np.array(a)).to(DEV)

    @staticmethod
    def measures(x, sample_rate, **kw):
        return F._vad_measures(x, sample_rate, **kw).cpu().numpy()

    @staticmethod
    def trigger(meas, pl):
        m = torch.from_numpy(np.ascontiguousarray(meas, dtype=np.float32)).to(DEV)
        first, start, joint = F._vad_trigger(m, pl.M, pl.gap, pl.P, pl.fixed, pl.level, pl.trig)
        return first.cpu().numpy(), start.cpu().numpy(), int(joint.cpu()[0])


# ---- 1. the trigger, exact -------------------------------------------------------------------------------------------------

def test_trigger_equals_the_oracle_on_synthetic_measurements():
    for name, meas, pl in K.trigger_grid():
        K.check_trigger(Device, name, meas, pl)


@pytest.mark.parametrize("case", K.constructed_cases(), ids=lambda c: c[0])
def test_trigger_constructed_cases(case):
    K.check_trigger(Device, *case)


# ---- 2. the measurements ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(O.GROUPS))
def test_measures_within_the_oracles_own_float32_error(name):
    K.check_measures(Device, name)


def test_measures_row_counts_offsets_and_strides():
    K.check_row_counts_and_offsets(Device)


def test_measures_nan_row_leaves_the_clean_rows_alone():
    K.check_nan_row(Device)


def test_measures_rows_of_l_and_l_plus_one_samples():
    K.check_short_rows(Device)
    x = Device.tensor(O.group("16k")[0][:2, :1600])
    assert F.vad_start(x, 16000).tolist() == [-1, -1] and F.vad(x, 16000).shape == (2, 0)


# ---- 3. consistency, exact --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["8k", "16k", "44k", "16k_boot0", "16k_bf16"])
def test_vad_start_and_vad_equal_the_oracles_trigger_on_the_devices_measurements(name):
    x, sr, kw, _, _, _ = O.group(name)
    pl = O.plan(sr, **kw)
    t = Device.tensor(x)
    meas = F._vad_measures(t, sr, **kw).cpu().numpy()
    start = F.vad_start(t, sr, **kw)
    assert start.dtype == torch.int64 and start.shape == (len(x),) and start.device.type == "cuda"
    assert start.tolist() == [O.trigger_row(row, pl)[1] for row in meas]
    for lo, hi in ((0, len(x)), (0, 1), (len(x) - 3, len(x))):           # channels of one recording
        s = O.trigger_joint(meas[lo:hi], pl)
        out = F.vad(t[lo:hi], sr, **kw)
        want = t[lo:hi, s:] if s >= 0 else t[lo:hi, :0]
        assert out.shape == want.shape and torch.equal(out, want)
        assert out.untyped_storage().data_ptr() == t.untyped_storage().data_ptr()      # a view of the input
        assert out.storage_offset() == want.storage_offset() and out.stride() == want.stride()


def test_vad_shapes_views_and_the_module():
    x, sr, kw, _, _, _ = O.group("16k")
    t = Device.tensor(x[:6])
    one = F.vad(t[0], sr)                                                 # (time,)
    assert one.dim() == 1 and torch.equal(one, F.vad(t[:1], sr)[0])
    assert F.vad_start(t[0], sr).shape == () and int(F.vad_start(t[0], sr)) == int(F.vad_start(t[:1], sr)[0])
    with pytest.warns(UserWarning, match="vad_start"):
        cube = F.vad(t.view(2, 3, -1), sr)
    assert cube.shape[:2] == (2, 3) and torch.equal(cube.reshape(6, -1), F.vad(t, sr))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert F.vad_start(t.view(2, 3, -1), sr).shape == (2, 3)
        assert torch.equal(T.Vad(sr, trigger_level=6.0)(t), F.vad(t, sr, trigger_level=6.0))
    quiet = torch.zeros(2, 16000, device=DEV)
    none = F.vad(quiet, sr)
    assert none.shape == (2, 0) and none.untyped_storage().data_ptr() == quiet.untyped_storage().data_ptr()
    assert F.vad_start(quiet, sr).tolist() == [-1, -1]
    stepped = t[:, ::2]                                                   # a non-unit sample stride is gathered
    assert torch.equal(F.vad_start(stepped, sr), F.vad_start(stepped.contiguous(), sr))
    assert F.vad(stepped, sr).untyped_storage().data_ptr() == t.untyped_storage().data_ptr()


def test_pre_trigger_time_before_the_first_sample_clamps_to_zero():
    x, sr, kw, _, _, _ = O.group("16k")
    t = Device.tensor(x[:3])
    assert int(F.vad_start(t, sr).max()) > 0
    got = F.vad_start(t, sr, pre_trigger_time=3.0)
    assert got.tolist() == [0 if v >= 0 else -1 for v in F.vad_start(t, sr).tolist()]


# ---- 4. end to end ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", O.E2E)
def test_vad_start_equals_the_float64_oracle_where_it_has_margin(name):
    x, sr, kw, m64, u64, _ = O.group(name)
    pl = O.plan(sr, **kw)
    tol = O.tolerance(sr)
    start = F.vad_start(Device.tensor(x), sr, **kw).tolist()
    kept = [r for r in range(len(x)) if O.has_margin(m64[r], u64[r], pl, tol)]
    assert 4 * (len(x) - len(kept)) <= len(x)
    for r in kept:
        assert start[r] == O.trigger_row(m64[r], pl)[1], (name, r)


# ---- 5. the surface ---------------------------------------------------------------------------------------------------------

def test_tiles_and_limits():
    threads, max_n, min_n, trig = F.vad_tiles()
    assert (threads, min_n, trig) == (256, 16, 64) and max_n >= 8192 and max_n == F.VAD_MAX_FFT
    with pytest.raises(NotImplementedError, match=str(max_n)):
        F.vad_start(torch.zeros(1, 30000, device=DEV), 96000)
    with pytest.raises(RuntimeError, match="forward-only"):
        F.vad_start(torch.zeros(1, 30000, device=DEV, requires_grad=True), 16000)


def test_two_calls_give_the_same_bits():
    x, sr, kw, _, _, _ = O.group("44k")
    t = Device.tensor(x)
    a, b = F._vad_measures(t, sr), F._vad_measures(t, sr)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(F.vad_start(t, sr), F.vad_start(t, sr))


def test_graph_capture_of_vad_start_and_the_eager_first_rule():
    x, sr, kw, _, _, _ = O.group("16k")
    t = Device.tensor(x[:5])
    eager = F.vad_start(t, sr)                                            # the tables are on the device from here on
    static = torch.zeros_like(t)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        F.vad_start(static, sr)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = F.vad_start(static, sr)
    static.copy_(t)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    g = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="eagerly"):
        with torch.cuda.graph(g):
            doubled = t * 2                                               # the capture is not empty
            F.vad_start(doubled, sr, measure_duration=0.0801)             # no other test uses this plan
    torch.cuda.synchronize()
    assert F.vad_start(t, sr, measure_duration=0.0801).shape == (5,)
