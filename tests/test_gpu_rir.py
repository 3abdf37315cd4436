"""F.simulate_rir_ism / F.simulate_rir_ism_batch on the device through the product API, against tests/rir_oracle.py: the checks
of tests/test_rir.py (rir_cases.py) on the smallest shapes that reach every tile edge, both sides of one image chunk and the
three filter lengths, then what only the product has: the three forms of `absorption`, the single-room entry and its default
length, the refusals, graph capture, and the response convolved by F.fftconvolve."""
import numpy as np
import pytest
import torch

import rir_cases as K
import rir_oracle as O
import audio_amd.functional as F
from conftest import peak_rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


class Device:
    """The backend of rir_cases: the batch entry point on the device."""

    @staticmethod
    def tiles():
        return F.rir_tiles()

    @staticmethod
    def run(room, source, mic, max_order, absorption, L, fl=81, sample_rate=K.FS, sound_speed=K.C):
        out = F.simulate_rir_ism_batch(dev(room), dev(source), dev(mic), max_order, dev(absorption), L, sound_speed, fl, sample_rate)
        return out.cpu().numpy()


def test_tiles_are_what_the_cases_straddle():
    assert Device.tiles() == (K.TILE, K.CHUNK, F.RIR_MAX_FILTER, F.RIR_MAX_ORDER)


@pytest.mark.parametrize("dt", list(K.DTYPES))
def test_single_image_is_the_closed_form(dt):
    K.check_single_image(Device, dt)


@pytest.mark.parametrize("dt", list(K.DTYPES))
@pytest.mark.parametrize("name", list(K.SHAPES))
def test_device_within_the_oracles_own_error(name, dt):
    K.check_accuracy(Device, name, dt)


def test_two_calls_give_the_same_bits():
    K.check_reproducible(Device)
    K.check_reproducible(Device, "n3_m3_b5_tile+1_fl255", "f64")


@pytest.mark.parametrize("dt", list(K.DTYPES))
def test_prefix_of_a_longer_call_is_the_shorter_call(dt):
    K.check_prefix(Device, dt)


@pytest.mark.parametrize("dt", list(K.DTYPES))
def test_rows_of_a_batch_are_rooms_of_their_own(dt):
    K.check_rows_are_rooms(Device, dt)


@pytest.mark.parametrize("dt", list(K.DTYPES))
def test_microphone_on_the_source_poisons_its_row_only(dt):
    K.check_poison(Device, dt)


def test_absorption_forms_give_the_same_bits():
    (room, source, mic, ab, N, L, fl), _, _, _ = K.case("n3_m3_b5_tile+1", "f32")
    r, s, m = dev(room), dev(source), dev(mic)
    B, D = room.shape
    per_room = ab[:, 0].copy()
    want = F.simulate_rir_ism_batch(r, s, m, N, dev(np.repeat(per_room[:, None], 2 * D, axis=1)), L)
    assert torch.equal(F.simulate_rir_ism_batch(r, s, m, N, dev(per_room), L), want)
    flat = F.simulate_rir_ism_batch(r, s, m, N, 0.25, L)
    assert torch.equal(flat, F.simulate_rir_ism_batch(r, s, m, N, dev(np.full((B, 2 * D), 0.25, np.float32)), L))
    assert torch.equal(flat, F.simulate_rir_ism_batch(r, s, m, N, dev(np.full((B,), 0.25, np.float32)), L))
    assert not torch.equal(flat, want)
    # the single-room entry: a float, (2 D,) and (1, 2 D)
    one = F.simulate_rir_ism(r[1], s[1], m[1], N, 0.25, output_length=L)
    assert torch.equal(one, flat[1])
    walls = dev(ab[1])
    assert torch.equal(F.simulate_rir_ism(r[1], s[1], m[1], N, walls, output_length=L),
                       F.simulate_rir_ism(r[1], s[1], m[1], N, walls[None], output_length=L))
    assert torch.equal(F.simulate_rir_ism(r[1], s[1], m[1], N, walls, output_length=L, center_frequency=dev(np.float32([1000.0]))),
                       F.simulate_rir_ism_batch(r, s, m, N, dev(ab), L)[1])


def test_single_room_default_length_is_the_oracles():
    for name, dt in (("n3_m3_b5_tile+1", "f32"), ("d2_n2_m3_b5_2tile+3", "f64")):
        (room, source, mic, ab, N, _, fl), _, _, _ = K.case(name, dt)
        L = O.length(room[0], source[0], mic[0], N, K.FS, K.C, fl)
        out = F.simulate_rir_ism(dev(room[0]), dev(source[0]), dev(mic[0]), N, dev(ab[0]), delay_filter_length=fl)
        assert out.shape == (mic.shape[1], L) and out.dtype == dev(room).dtype
        want = O.gather(room[0], source[0], mic[0], N, ab[0], L, K.FS, K.C, fl)
        assert peak_rel_err(out.cpu().numpy(), want) <= (1e-6 if dt == "f32" else 1e-13)
        sr = F.simulate_rir_ism(dev(room[0]), dev(source[0]), dev(mic[0]), N, dev(ab[0]), sample_rate=8000.0, sound_speed=340.0)
        assert sr.shape[1] == O.length(room[0], source[0], mic[0], N, 8000.0, 340.0, 81)


def test_refusals_on_the_device():
    (room, source, mic, ab, N, L, fl), _, _, _ = K.case("n1_m3_b1_tile", "f32")
    r, s, m, a = dev(room), dev(source), dev(mic), dev(ab)
    with pytest.raises(RuntimeError, match="forward-only"):
        F.simulate_rir_ism_batch(r, s.clone().requires_grad_(), m, N, a, L)
    with pytest.raises(RuntimeError, match="forward-only"):
        F.simulate_rir_ism_batch(r, s, m, N, a.clone().requires_grad_(), L)
    with torch.no_grad():
        assert F.simulate_rir_ism_batch(r, s.clone().requires_grad_(), m, N, a, L).shape == (1, 3, L)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.simulate_rir_ism_batch(r, s, m, N, a.cpu(), L)
    with pytest.raises(TypeError, match="dtype of room"):
        F.simulate_rir_ism_batch(r, s, m, N, a.double(), L)
    with pytest.raises(ValueError, match="absorption"):
        F.simulate_rir_ism_batch(r, s, m, N, a[:, :5], L)
    with pytest.raises(NotImplementedError, match="octave-band filter bank"):
        F.simulate_rir_ism(r[0], s[0], m[0], N, a.repeat(7, 1), output_length=L)
    assert F.simulate_rir_ism_batch(r[:0], s[:0], m[:0], N, 0.1, L).shape == (0, 3, L)
    assert not hasattr(torch.ops.audio_amd, "simulate_rir_ism")


def test_graph_capture_replays_the_eager_bits():
    (room, source, mic, ab, N, L, fl), _, _, _ = K.case("n3_m3_b5_tile+1", "f32")
    r, s, m, a = dev(room), dev(source), dev(mic), dev(ab)
    eager = F.simulate_rir_ism_batch(r, s, m, N, a, L)           # the lattice is on the device from here on
    static = s.clone()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        F.simulate_rir_ism_batch(r, static, m, N, a, L)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = F.simulate_rir_ism_batch(r, static, m, N, a, L)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    static.copy_(s + 0.125)                                     # the graph reads its inputs in place
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, F.simulate_rir_ism_batch(r, static, m, N, a, L)) and not torch.equal(out, eager)
    g = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="run the call once eagerly"):
        with torch.cuda.graph(g):
            moved = s * 1                                       # the capture is not empty
            F.simulate_rir_ism_batch(r, moved, m, 7, a, L)       # no other test uses this max_order
    torch.cuda.synchronize()
    assert F.simulate_rir_ism_batch(r, s, m, 7, a, L).shape == eager.shape


def test_fftconvolve_with_the_simulated_response():
    B, T, L, N = 4, 4000, 1200, 3
    room, source, mic, ab = K.rooms(77, B, 1, 3, np.float32, N)
    x = np.random.default_rng(5).standard_normal((B, T)).astype(np.float32)
    h = F.simulate_rir_ism_batch(dev(room), dev(source), dev(mic), N, dev(ab), L)[:, 0]
    y = F.fftconvolve(dev(x), h)
    assert y.shape == (B, T + L - 1)
    want = np.stack([np.convolve(x[b].astype(np.float64), O.gather(room[b], source[b], mic[b], N, ab[b], L)[0]) for b in range(B)])
    assert peak_rel_err(y.cpu().numpy(), want) <= 2e-5
