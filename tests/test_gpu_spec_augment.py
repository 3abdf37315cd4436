"""SpecAugment masking on the device: parity through F._spec_augment_apply with explicit draws and bounds against the loop
oracle (vector-path edge shapes, both dense layouts and a sliced view, four dtypes, policies up to a chained 33 masks,
pinned masks), strides, special values, a device mask_value, seed reproduction of every public function and module against
the restated reference on the same device, the shared path's ValueError, gradients, launch routes, determinism, graph
capture and the MelSpectrogram pipeline.  Every comparison is exact, on bit views."""
import numpy as np
import pytest
import torch

import spec_augment_oracle as O
import audio_amd.functional as F
import audio_amd.transforms as T
from audio_amd import _ops  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float32, torch.float64, torch.float16, torch.bfloat16]
# every listed n_time and n_freq, examples 1 and 3 and the leading shape (2, 3)
SHAPES = [((1,), 1, 1), ((3,), 2, 3), ((1,), 3, 2), ((3,), 4, 5), ((1,), 5, 4), ((2, 3), 5, 7), ((3,), 80, 8), ((1,), 81, 9),
          ((3,), 3, 63), ((1,), 4, 64), ((3,), 129, 65), ((1,), 2, 257), ((3,), 80, 1001), ((1,), 129, 1001), ((2, 3), 1, 65)]


def bits(t):
    return O.bit_view(t).numpy()


def same_strides(a, b):
    return [s for s, n in zip(a.stride(), a.shape) if n > 1] == [s for s, n in zip(b.stride(), b.shape) if n > 1]


def special(x):
    flat = x.reshape(-1)
    for k, v in enumerate([float("nan"), float("inf"), -float("inf"), -0.0]):
        flat[(k * 7 + 1) % flat.numel()] = v
    return x


def layouts(x):
    """x: CPU (..., F, T) -> device tensors of the same values: time-contiguous, frame-major, a sliced view"""
    lead, Fq, Tm = tuple(x.shape[:-2]), x.shape[-2], x.shape[-1]
    big = torch.zeros(lead + (Fq + 1, 2 * Tm + 1), dtype=x.dtype)
    big[..., :Fq, 1:2 * Tm:2] = x
    return {"time": x.to(DEV), "frame": x.transpose(-1, -2).contiguous().to(DEV).transpose(-1, -2),
            "sliced": big.to(DEV)[..., :Fq, 1:2 * Tm:2]}


def policies(Fq, Tm):
    small_t, small_f = max(Tm // 16, 1), max(Fq // 16, 1)
    return {"1t": [(1, min(100, Tm + 2))], "1f": [(0, min(27, Fq + 2))],
            "2+2": [(1, min(100, Tm + 2))] * 2 + [(0, min(27, Fq + 2))] * 2,
            "10+2": [(1, max(Tm // 8, 1))] * 10 + [(0, max(Fq // 4, 1))] * 2,
            "33": [(1, small_t)] * 20 + [(0, small_f)] * 13}


@pytest.mark.parametrize("lead,Fq,Tm", SHAPES)
def test_parity_with_explicit_draws(lead, Fq, Tm):
    g = torch.Generator().manual_seed(Fq * 1009 + Tm)
    base = torch.randn(lead + (Fq, Tm), generator=g, dtype=torch.float64)
    for dtype in DTYPES:
        x = special(base.to(dtype))
        xs = layouts(x)
        for name, plan in policies(Fq, Tm).items():
            d = torch.rand((len(plan), 2) + lead, generator=g).to(dtype)
            masks = [O.bounds(d[m], prm, Tm if a == 1 else Fq, dtype) for m, (a, prm) in enumerate(plan)]
            want = O.apply(x, masks, [a for a, _ in plan], -1.5)
            dd = d.to(DEV)
            for lay, xd in xs.items():
                y = F._spec_augment_apply(xd, dd, plan, -1.5)
                assert y.shape == xd.shape and y.dtype == dtype
                if lay != "sliced":                                    # (the stride of a one-element axis says nothing)
                    assert same_strides(y, xd), (lay, y.stride(), xd.stride())
                else:
                    assert y.is_contiguous()
                assert np.array_equal(bits(y), want), (dtype, name, lay)


@pytest.mark.parametrize("dtype", DTYPES)
def test_pinned_masks(dtype):
    g = torch.Generator().manual_seed(7)
    for lead, Fq, Tm in [((3,), 5, 9), ((1,), 4, 64), ((2, 3), 3, 65), ((1,), 80, 7), ((3,), 81, 257)]:
        x = special(torch.randn(lead + (Fq, Tm), generator=g).to(dtype))
        xs = layouts(x)
        for axis, size in ((1, Tm), (0, Fq)):
            # start = 0, end = size, the whole axis, empty, one misaligned element inside a 16-byte vector, bounds beyond
            # the axis on either side, touching and overlapping pairs
            for b in [[(0, 3)], [(size - 2, size)], [(0, size)], [(4, 4)], [(5, 6)], [(-7, 2)], [(size - 1, size + 50)],
                      [(1, 3), (3, 5)], [(1, 4), (2, 6)], [(0, 1), (size - 1, size)]]:
                want = O.apply(x, b, [axis] * len(b), 3.0)
                for lay, xd in xs.items():
                    y = F._spec_augment_apply(xd, b, [axis] * len(b), 3.0)
                    assert np.array_equal(bits(y), want), (lead, Fq, Tm, axis, b, lay)


def test_special_values_pass_bitwise_and_device_mask_value():
    for dtype in DTYPES:
        x = torch.zeros(2, 6, 11, dtype=dtype)
        ib = x.view(O.BITS[x.element_size()])
        ib.reshape(-1)[:] = torch.arange(x.numel()) * 37 + (1 << (8 * x.element_size() - 2))      # arbitrary bit patterns
        nan_payload = {2: 0x7e01, 4: 0x7fc00123, 8: 0x7ff8000000000456}[x.element_size()]
        ib[0, 0, 0] = nan_payload
        ib[1, 5, 10] = -(1 << (8 * x.element_size() - 1))                                          # -0.0
        x[0, 1, 1] = float("inf")
        for xd in layouts(x).values():
            y = F._spec_augment_apply(xd, [(2, 4)], [1], 0.0)
            want = O.apply(x, [(2, 4)], [1], 0.0)
            assert np.array_equal(bits(y), want)
            assert bits(y)[0, 0, 0] == nan_payload
            v = torch.tensor(-0.0, dtype=dtype, device=DEV)                                        # a 0-d device tensor
            y = F._spec_augment_apply(xd, [(2, 4), (1, 2)], [1, 0], v)
            assert np.array_equal(bits(y), O.apply(x, [(2, 4), (1, 2)], [1, 0], -0.0))
            y = F._spec_augment_apply(xd, [(0, 11)], [1], torch.tensor(float("nan"), device=DEV))   # another dtype: cast
            assert torch.isnan(y).all()


def _reference_and_ours(make_ref, make_ours, seed=5):
    torch.manual_seed(seed)
    want = make_ref()
    torch.manual_seed(seed)
    got = make_ours()
    return want, got


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_seed_reproduction_of_the_reference(dtype):
    g = torch.Generator().manual_seed(9)
    x = torch.randn(2, 3, 80, 301, generator=g).to(dtype)
    for lay, xd in layouts(x).items():
        for axis, param, p in [(3, 100, 1.0), (2, 27, 1.0), (3, 100, 0.2), (3, 400, 1.0), (2, 81, 0.5)]:
            want, got = _reference_and_ours(lambda: O.torch_reference_mask_along_axis_iid(xd, param, 1.25, axis, p),
                                            lambda: F.mask_along_axis_iid(xd, param, 1.25, axis, p))
            assert np.array_equal(bits(got), bits(want)), (lay, axis, param, p)
            want, got = _reference_and_ours(lambda: O.torch_reference_mask_along_axis(xd, param, 1.25, axis, p),
                                            lambda: F.mask_along_axis(xd, param, 1.25, axis, p))
            assert np.array_equal(bits(got), bits(want)), (lay, axis, param, p)
        mods = [(T.FrequencyMasking(27), lambda t: O.torch_reference_mask_along_axis(t, 27, 0.0, 2)),
                (T.FrequencyMasking(27, iid_masks=True), lambda t: O.torch_reference_mask_along_axis_iid(t, 27, 0.0, 2)),
                (T.TimeMasking(100, p=0.2), lambda t: O.torch_reference_mask_along_axis(t, 100, 0.0, 3, 0.2)),
                (T.TimeMasking(100, iid_masks=True, p=0.2), lambda t: O.torch_reference_mask_along_axis_iid(t, 100, 0.0, 3, 0.2)),
                (T.SpecAugment(2, 100, 2, 27, p=0.2), lambda t: O.torch_reference_spec_augment(t, 2, 100, 2, 27, True, 0.2)),
                (T.SpecAugment(2, 100, 2, 27, zero_masking=True),
                 lambda t: O.torch_reference_spec_augment(t, 2, 100, 2, 27, True, 1.0, True)),
                (T.SpecAugment(3, 50, 1, 10, iid_masks=False), lambda t: O.torch_reference_spec_augment(t, 3, 50, 1, 10, False)),
                # the time masks' effective param is int(301 * 0.003) == 0: they draw nothing, the frequency masks do
                (T.SpecAugment(2, 100, 2, 27, p=0.003), lambda t: O.torch_reference_spec_augment(t, 2, 100, 2, 27, True, 0.003)),
                (T.SpecAugment(2, 100, 2, 0), lambda t: O.torch_reference_spec_augment(t, 2, 100, 2, 0))]
        for mod, ref in mods:
            want, got = _reference_and_ours(lambda: ref(xd), lambda: mod(xd))
            assert np.array_equal(bits(got), bits(want)), (lay, mod)
            torch.manual_seed(5)
            scripted = torch.jit.script(mod)(xd)
            assert np.array_equal(bits(scripted), bits(got)), (lay, mod)
    # 2-D input: SpecAugment takes the shared path whatever iid_masks says
    x2 = layouts(x[0, 0])["frame"]
    want, got = _reference_and_ours(lambda: O.torch_reference_spec_augment(x2, 2, 100, 2, 27),
                                    lambda: T.SpecAugment(2, 100, 2, 27)(x2))
    assert got.stride() == x2.stride() and np.array_equal(bits(got), bits(want))


def test_seeded_bounds_where_the_type_does_not_hold_the_axis_length():
    """float16 beyond 2048 frames, bfloat16 beyond 256: `size - value` is formed from the unrounded size on the device."""
    for dtype, Tm in [(torch.float16, 4099), (torch.bfloat16, 1003)]:
        xd = torch.randn(64, 2, Tm, device=DEV).to(dtype)
        want, got = _reference_and_ours(lambda: O.torch_reference_mask_along_axis_iid(xd, 100, 0.0, 2),
                                        lambda: F.mask_along_axis_iid(xd, 100, 0.0, 2))
        assert np.array_equal(bits(got), bits(want)), dtype


def test_shared_path_value_error(monkeypatch):
    x = torch.randn(2, 8, 9, device=DEV)
    real = torch.rand
    monkeypatch.setattr(torch, "rand", lambda *a, **k: torch.ones(*a, **k))        # value = mask_param: end - start >= mask_param
    with pytest.raises(ValueError, match="Number of columns to be masked should be less than mask_param"):
        F.mask_along_axis(x, 4, 0.0, 2)
    with pytest.raises(ValueError, match="Number of columns"):
        T.SpecAugment(1, 4, 1, 4, iid_masks=False)(x)
    monkeypatch.setattr(torch, "rand", real)
    assert F.mask_along_axis(x, 4, 0.0, 2).shape == x.shape


def test_gradients_float64():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 5, 7, generator=g, dtype=torch.float64).to(DEV).requires_grad_(True)
    xt = torch.randn(2, 7, 5, generator=g, dtype=torch.float64).to(DEV).transpose(-1, -2).requires_grad_(True)
    d = torch.rand(3, 2, 2, generator=g, dtype=torch.float64).to(DEV)
    plan = [(1, 4), (0, 3), (1, 2)]
    for t in (x, xt):
        fn = lambda a: F._spec_augment_apply(a, d, plan, 0.5)                                 # noqa: E731
        assert torch.autograd.gradcheck(fn, (t,))
        assert torch.autograd.gradgradcheck(fn, (t,))
        # mask_value = mean(x): gradient flows into the mean, as in SpecAugment(zero_masking=False)
        fm = lambda a: F._spec_augment_apply(a, d, plan, a.mean())                            # noqa: E731
        assert torch.autograd.gradcheck(fm, (t,))
        assert torch.autograd.gradgradcheck(fm, (t,))
    # the module itself, its draws pinned by the seed

    def module(a):
        torch.manual_seed(21)
        return T.SpecAugment(2, 4, 1, 3)(a)

    assert torch.autograd.gradcheck(module, (x,))
    assert torch.autograd.gradgradcheck(module, (x,))
    torch.manual_seed(21)
    want = O.torch_reference_spec_augment(x, 2, 4, 1, 3)
    assert np.array_equal(bits(module(x)), bits(want))


def test_backward_float32_is_the_mask_over_the_cotangent():
    g = torch.Generator().manual_seed(4)
    for lay in ("time", "frame", "sliced"):
        x = layouts(torch.randn(3, 80, 65, generator=g))[lay].requires_grad_(True)
        d = torch.rand(4, 2, 3, generator=g).to(DEV)
        plan = [(1, 30), (1, 30), (0, 27), (0, 27)]
        y = F._spec_augment_apply(x, d, plan, 2.0)
        ct = torch.randn(3, 80, 65, generator=g).to(DEV)
        gx, = torch.autograd.grad(y, x, ct)
        masks = [O.bounds(d[m].cpu(), prm, 65 if a == 1 else 80, torch.float32) for m, (a, prm) in enumerate(plan)]
        assert np.array_equal(bits(gx), O.apply(ct, masks, [a for a, _ in plan], 0.0))


def test_both_launch_routes_and_determinism():
    g = torch.Generator().manual_seed(6)
    x = special(torch.randn(3, 81, 257, generator=g))
    d = torch.rand(12, 2, 3, generator=g).to(DEV)
    plan = [(1, 40)] * 10 + [(0, 27)] * 2
    out = {}
    try:
        for route in ("shim", "ctypes"):
            F._force_route(route)
            for dtype in (torch.float32, torch.bfloat16, torch.float64):
                for lay, xd in layouts(x.to(dtype)).items():
                    v = torch.tensor(0.75, dtype=dtype, device=DEV)
                    res = [bits(F._spec_augment_apply(xd, d.to(dtype), plan, 0.25)), bits(F._spec_augment_apply(xd, d.to(dtype), plan, v)),
                           bits(F._spec_augment_apply(xd, [(3, 9), (0, 2)], [1, 0], 0.25))]
                    again = bits(F._spec_augment_apply(xd, d.to(dtype), plan, 0.25))
                    assert np.array_equal(res[0], again)                                  # call to call
                    out.setdefault((dtype, lay), []).append(res)
    finally:
        F._force_route(None)
    for key, (a, b) in out.items():
        for ra, rb in zip(a, b):
            assert np.array_equal(ra, rb), key


def test_graph_capture_of_the_iid_module():
    x = torch.randn(4, 80, 301, device=DEV)
    mod = T.TimeMasking(100, iid_masks=True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        mod(x, 7.0)                                                     # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = mod(x, 7.0)
    xb = bits(x)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        yb = bits(y)
        filled = yb == O.value_bits(7.0, torch.float32)
        assert np.array_equal(yb[~filled], xb[~filled])                 # the input off the mask
        cols = filled.all(axis=1)                                       # (example, time): whole columns are filled
        assert np.array_equal(filled, np.broadcast_to(cols[:, None, :], filled.shape))
        for e in range(4):
            idx = np.nonzero(cols[e])[0]
            assert idx.size <= 100 and (idx.size == 0 or idx[-1] - idx[0] + 1 == idx.size)   # one run, at most mask_param wide


def test_pipeline_reads_the_frame_major_mel_in_place():
    torch.manual_seed(0)
    wav = torch.randn(4, 16000, device=DEV)
    mel = T.MelSpectrogram(16000, 400, hop_length=160, n_mels=80).to(DEV)(wav)
    assert mel.shape == (4, 80, 101) and mel.stride() == (8080, 1, 80)
    aug = T.SpecAugment(2, 100, 2, 27)
    want, got = _reference_and_ours(lambda: O.torch_reference_spec_augment(mel, 2, 100, 2, 27), lambda: aug(mel))
    assert got.stride() == mel.stride()
    assert np.array_equal(bits(got), bits(want))
    assert not np.array_equal(bits(got), bits(mel))
