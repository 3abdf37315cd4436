"""F.ray_tracing / F.ray_tracing_batch on the device through the product API, against tests/ray_oracle.py: the checks of
tests/test_ray_tracing.py (ray_cases.py) on the smallest shapes that reach every ray count around a workgroup, the band
classes, both dimensions and every way a ray ends, then what only the product has: the forms of the coefficients, the
single-room entry, the refusals and graph capture with no warm-up call.

Accuracy: the bar of ray_cases.case (4 x the float64 oracle's own distance from its longdouble form + count 2^-(k+1), + half a
float32 ulp for float32).  Measured share of the bar on an MI355X: 0.00-0.22 for float64 results, 0.90-1.00 for float32 results
(the half ulp of the one float32 rounding); 19 of the 22 results equal the fixed-point oracle's bits, the other three differ
through sin / cos of the ray directions."""
import numpy as np
import pytest
import torch

import ray_cases as K
import audio_amd.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


class Device:
    """The backend of ray_cases: the batch entry point on the device."""

    @staticmethod
    def tiles():
        return F.ray_tiles()

    @staticmethod
    def run(room, source, mic, num_rays, absorption, scattering, mic_radius=0.5, sound_speed=K.C, energy_thres=1e-7,
            time_thres=10.0, hist_bin_size=0.004):
        out = F.ray_tracing_batch(dev(room), dev(source), dev(mic), num_rays, dev(absorption), dev(scattering), mic_radius,
                                  sound_speed, energy_thres, time_thres, hist_bin_size)
        return out.cpu().numpy()


def test_tiles_are_what_the_cases_straddle():
    assert Device.tiles() == (K.THREADS, F.RAY_MAX_BANDS, F.RAY_MAX_MICS, F.RAY_MAX_RAYS, F.RAY_MAX_BINS, F.RAY_MAX_BOUNCES,
                              F.RAY_HEADROOM)


@pytest.mark.parametrize("dt", list(K.DTYPES))
@pytest.mark.parametrize("name", list(K.SHAPES))
def test_device_within_the_oracles_own_error(name, dt):
    K.check_accuracy(Device, name, dt)


def test_two_calls_give_the_same_bits():
    K.check_reproducible(Device)
    K.check_reproducible(Device, "r64_m5_nb3_unequal_sc.3", "f64")


@pytest.mark.parametrize("dt", list(K.DTYPES))
def test_rows_of_a_batch_are_rooms_and_microphones_stand_alone(dt):
    K.check_rows_are_rooms(Device, dt)


@pytest.mark.parametrize("dt", list(K.DTYPES))
def test_equal_bands_are_equal(dt):
    K.check_equal_bands(Device, dt)


@pytest.mark.parametrize("dt", list(K.DTYPES))
def test_a_bad_room_is_nan_and_its_neighbours_keep_their_bits(dt):
    K.check_bad_rooms(Device, dt)


def test_coefficient_forms_give_the_same_bits():
    name = "r64_m5_nb3_unequal_sc.3"
    (room, source, mic, ab, sc), *_ = K.case(name, "f32")
    N, kw = K.SHAPES[name][1], K.params(name)
    r, s, m = dev(room), dev(source), dev(mic)
    D = room.shape[1]
    want = F.ray_tracing_batch(r, s, m, N, dev(ab), dev(sc), **kw)                 # sc is 0.3 everywhere
    assert want.shape == (1, 5, 3, K.O.num_bins(kw["time_thres"], kw["hist_bin_size"]))
    assert torch.equal(F.ray_tracing_batch(r, s, m, N, dev(ab), 0.3, **kw), want)   # float32(0.3) in both
    assert torch.equal(F.ray_tracing_batch(r, s, m, N, dev(ab), dev(sc[:, :1]), **kw), want)
    # the single-room entry: (num_bands, 2 D), (num_bands,) and a float
    one = F.ray_tracing(r[0], s[0], m[0], N, dev(ab[0]), dev(sc[0]), **kw)
    assert torch.equal(one, want[0])
    assert torch.equal(F.ray_tracing(r[0], s[0], m[0], N, dev(ab[0]), dev(sc[0, :, 0]), **kw), want[0])
    assert torch.equal(F.ray_tracing(r[0], s[0], m[0], N, dev(ab[0]), dev(sc[0, :1, 0]), **kw), want[0])
    per_band = dev(ab[0, :, 0].copy())
    alike = F.ray_tracing(r[0], s[0], m[0], N, per_band, 0.3, **kw)
    assert torch.equal(alike, F.ray_tracing(r[0], s[0], m[0], N, per_band[:, None].expand(3, 2 * D), 0.3, **kw))
    assert not torch.equal(alike, want[0])
    flat = F.ray_tracing(r[0], s[0], m[0], N, 0.25, 0.0, **kw)
    assert flat.shape == (5, 1, want.shape[-1])
    assert torch.equal(flat, F.ray_tracing(r[0], s[0], m[0], N, dev(np.full((1, 2 * D), 0.25, np.float32)), dev(np.zeros(1, np.float32)), **kw))
    assert F.ray_tracing(r[0], s[0], m[0], N, time_thres=0.05).shape == (5, 1, 13)  # the defaults: no absorption, no scattering


def test_refusals_on_the_device():
    name = "r63_m2_sc.3"
    (room, source, mic, ab, sc), *_ = K.case(name, "f32")
    N, kw = K.SHAPES[name][1], K.params(name)
    r, s, m, a, c = dev(room), dev(source), dev(mic), dev(ab), dev(sc)
    with pytest.raises(RuntimeError, match="forward-only"):
        F.ray_tracing_batch(r, s.clone().requires_grad_(), m, N, a, c, **kw)
    with pytest.raises(RuntimeError, match="forward-only"):
        F.ray_tracing_batch(r, s, m, N, a.clone().requires_grad_(), c, **kw)
    with torch.no_grad():
        assert F.ray_tracing_batch(r, s.clone().requires_grad_(), m, N, a, c, **kw).shape[:3] == (1, 2, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.ray_tracing_batch(r, s, m, N, a, c.cpu(), **kw)
    with pytest.raises(TypeError, match="one dtype"):
        F.ray_tracing_batch(r, s, m, N, a.double(), c, **kw)
    with pytest.raises(ValueError, match="absorption"):
        F.ray_tracing_batch(r, s, m, N, a[:, :, :5], c, **kw)
    with pytest.raises(NotImplementedError, match="bins"):
        F.ray_tracing_batch(r, s, m, N, a, c, hist_bin_size=1e-4)
    assert F.ray_tracing_batch(r[:0], s[:0], m[:0], N, 0.1, 0.0, **kw).shape[:3] == (0, 2, 1)
    assert not hasattr(torch.ops.audio_amd, "ray_tracing")


def test_graph_capture_with_no_warm_up_replays_the_eager_bits():
    (room, source, mic, ab, sc), *_ = K.case(K.BATCH, "f32")
    # no other test uses this ray count or these parameters: the captured call is the first of its kind in the process
    N, kw = 77, dict(K.params(K.BATCH), time_thres=0.06, hist_bin_size=0.003)
    r, s, m, a, c = dev(room), dev(source), dev(mic), dev(ab), dev(sc)
    static = s.clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = F.ray_tracing_batch(r, static, m, N, a, c, **kw)
    g.replay()
    torch.cuda.synchronize()
    first = out.clone()
    g.replay()
    torch.cuda.synchronize()
    eager = F.ray_tracing_batch(r, s, m, N, a, c, **kw)
    assert torch.equal(first, eager) and torch.equal(out, eager) and eager.isfinite().all() and eager.sum() > 0
    static.copy_(s * 1.03125)                                   # the graph reads its inputs in place
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, F.ray_tracing_batch(r, static, m, N, a, c, **kw)) and not torch.equal(out, eager)
