"""SpecAugment masking without a GPU: the loop oracle against the restated reference with injected draws, the effective
mask_param, a CPU replay of csrc/spec_augment.h (bounds arithmetic in four dtypes, index maps, the whole kernel in both
paths), error types and messages, the early return, Meta shapes and strides, TorchScript, torch.compile on the meta device
and the refusal of CPU tensors.  Every comparison is exact, on bit views."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import spec_augment_oracle as O
import audio_amd.functional as F
import audio_amd.transforms as T
from audio_amd import _ops  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
SIM_SRC = os.path.join(HERE, "cpu_sim", "sim_spec_augment.cpp")
SIM_OUT = os.path.join(HERE, "cpu_sim", "_build", "libaamd_sim_spec_augment.so")
HDRS = [os.path.join(os.path.dirname(HERE), "audio_amd", "csrc", h) for h in ("spec_augment.h", "hd.h")]
DTYPES = [torch.float32, torch.float64, torch.float16, torch.bfloat16]
CODE = {torch.float32: 0, torch.float64: 1, torch.float16: 2, torch.bfloat16: 3}


# ---- the oracle against the restated reference ------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_loop_oracle_equals_restated_reference_iid(dtype):
    g = torch.Generator().manual_seed(1)
    for shape, axis, param in [((3, 5, 7), 2, 4), ((2, 3, 8, 9), 2, 5), ((3, 80, 65), 2, 100), ((4, 6, 5), 1, 9)]:
        x = torch.randn(shape, generator=g).to(dtype)
        d = torch.rand((2,) + shape[:-2], generator=g).to(dtype)
        want = O.torch_reference_mask_along_axis_iid(x, param, -1.5, axis, rand=O.injected([d[0], d[1]]))
        s, e = O.bounds(d, param, shape[axis], dtype)
        got = O.apply(x, [(s, e)], [O.TIME if axis == len(shape) - 1 else O.FREQ], -1.5)
        assert np.array_equal(got, O.bit_view(want).numpy())


def test_loop_oracle_equals_restated_spec_augment():
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, 3, 20, 40, generator=g)
    draws = [torch.rand(2, 3, generator=g) for _ in range(8)]
    want = O.torch_reference_spec_augment(x, 2, 10, 2, 6, rand=O.injected(draws))
    masks, axes = [], []
    for m in range(4):
        param, size, axis = (10, 40, O.TIME) if m < 2 else (6, 20, O.FREQ)
        masks.append(O.bounds(torch.stack(draws[2 * m:2 * m + 2]), param, size, torch.float32))
        axes.append(axis)
    assert np.array_equal(O.apply(x, masks, axes, x.mean()), O.bit_view(want).numpy())
    # shared masks: float32 draws of one element whatever the dtype
    d = [torch.tensor([0.7]), torch.tensor([0.5])]
    want = O.torch_reference_mask_along_axis(x.half(), 10, 2.0, 3, rand=O.injected(d))
    assert np.array_equal(O.apply(x.half(), [(16, 23)], [O.TIME], 2.0), O.bit_view(want).numpy())     # 0.5 * (40 - 7) = 16.5
    with pytest.raises(ValueError, match="Number of columns"):
        O.torch_reference_mask_along_axis(x, 10, 0.0, 3, rand=O.injected([torch.tensor([1.0]), torch.tensor([0.5])]))


def test_get_mask_param():
    assert F._get_mask_param(100, 1.0, 50) == 100                    # p == 1: mask_param as given, even beyond the axis
    assert F._get_mask_param(100, 0.2, 1001) == 100
    assert F._get_mask_param(100, 0.2, 400) == 80
    assert F._get_mask_param(100, 0.2, 4) == 0                       # int(0.8) == 0: no mask at all
    assert F._get_mask_param(100, 0.0, 4000) == 0
    assert F._get_mask_param(27, 0.999, 80) == 27
    for mp, p, n in [(100, 0.2, 400), (7, 0.5, 3), (0, 1.0, 9), (5, 0.3, 10)]:
        assert F._get_mask_param(mp, p, n) == O.get_mask_param(mp, p, n)
    assert torch.jit.script(F._get_mask_param)(100, 0.2, 4) == 0


# ---- CPU replay of csrc/spec_augment.h -------------------------------------------------------------------------------------

_sim = None


def sim():
    global _sim
    if _sim is None:
        newest = max(os.path.getmtime(p) for p in [SIM_SRC] + HDRS)
        if not os.path.exists(SIM_OUT) or newest > os.path.getmtime(SIM_OUT):
            os.makedirs(os.path.dirname(SIM_OUT), exist_ok=True)
            tmp = "%s.tmp.%d" % (SIM_OUT, os.getpid())
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", SIM_SRC, "-o", tmp])
            os.replace(tmp, SIM_OUT)
        _sim = C.CDLL(SIM_OUT)
        i64, i32, p, u64 = C.c_int64, C.c_int, C.c_void_p, C.c_uint64
        _sim.sim_sa_bounds.argtypes = [i32, p, p, i64, i64, i64, p, p]
        _sim.sim_sa_vector_bits.argtypes = [i64, i64, i64, i32, i32, i32, i32, i32, p]
        _sim.sim_sa_vector_bits.restype = C.c_uint32
        _sim.sim_sa_run.argtypes = [p, p] + [i64] * 6 + [i32] * 3 + [p, p, p, p, p, u64, p, i32]
    return _sim


def _bits64(t):
    """the elements' bits, zero-extended to uint64"""
    v = O.bit_view(t).numpy()
    return v.astype(np.int64).astype(np.uint64) & np.uint64((1 << (8 * v.itemsize)) - 1)


def sim_bounds(draws, param, size, dtype):
    d = draws.to(dtype)
    r0, r1 = np.ascontiguousarray(_bits64(d[0]).reshape(-1)), np.ascontiguousarray(_bits64(d[1]).reshape(-1))
    s, e = np.zeros(r0.size, np.int64), np.zeros(r0.size, np.int64)
    sim().sim_sa_bounds(CODE[dtype], r0.ctypes.data, r1.ctypes.data, r0.size, param, size, s.ctypes.data, e.ctypes.data)
    return s, e


def _below_one(dtype):
    return {torch.float32: 1 - 2.0 ** -24, torch.float64: 1 - 2.0 ** -53, torch.float16: 1 - 2.0 ** -11,
            torch.bfloat16: 1 - 2.0 ** -8}[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
def test_sim_bounds_are_the_oracles(dtype):
    g = torch.Generator().manual_seed(3)
    # draws of exactly 0, the largest value below 1, tiny ones (float16 subnormal products) and 1.0 (what a rounded cast can
    # give), each paired with each; plus random ones
    edge = torch.tensor([0.0, _below_one(dtype), 0.5, 2.0 ** -14, 2.0 ** -20, 1.0], dtype=torch.float64)
    r0 = torch.cat([torch.rand(400, generator=g, dtype=torch.float64), edge])
    r1 = torch.cat([edge, torch.rand(8, generator=g, dtype=torch.float64)])
    d = torch.stack([r0.repeat_interleave(r1.numel()), r1.repeat(r0.numel())])
    assert float(d.to(dtype)[0].max()) == 1.0 and float(d.to(dtype)[0].min()) == 0.0
    # (mask_param, size): the recipe's, mask_param > size (negative start), value < 1 (empty), sizes float16 cannot hold
    big = 60001 if dtype == torch.float16 else 70001                # (float16 holds no 70001)
    for param, size in [(100, 1001), (27, 80), (1, 1), (9, 4), (300, 7), (1, 5), (2049, 5000), (100, big), (3, 2)]:
        s, e = sim_bounds(d, param, size, dtype)
        ws, we = O.bounds(d, param, size, dtype)
        assert np.array_equal(s, ws) and np.array_equal(e, we), (param, size)
        if param > size:
            assert (ws < 0).any()
        assert (we == ws).any()


def test_sim_bounds_negative_start_and_empty_masks():
    d = torch.tensor([[0.99, 0.99, 0.001, 0.5], [0.99, 0.0, 0.5, 0.5]], dtype=torch.float64)
    for dtype in DTYPES:
        s, e = sim_bounds(d, 300, 7, dtype)
        ws, we = O.bounds(d, 300, 7, dtype)
        assert np.array_equal(s, ws) and np.array_equal(e, we)
        assert s[0] < -200 and e[0] >= 7                               # the whole axis
        assert e[2] == s[2]                                            # value = 0.3: an empty mask
    x = torch.arange(3 * 4 * 7, dtype=torch.float32).reshape(3, 4, 7)
    got = O.apply(x, [(np.array([-283, 0, 3]), np.array([14, 297, 3]))], [O.TIME], 9.0)
    assert (got[:2] == O.value_bits(9.0, torch.float32)).all() and np.array_equal(got[2], O.bit_view(x[2]).numpy())


def test_sim_index_maps_and_vector_bits():
    oi = (C.c_int32 * 2)()
    for O_, I, n in [(5, 7, 4), (3, 1, 4), (4, 3, 8), (9, 2, 2), (2, 16, 8), (7, 5, 4)]:
        for ilo, ihi, olo, ohi in [(0, 0, 0, 0), (1, 3, 0, 0), (0, I, 0, 0), (0, 0, 1, 2), (I - 1, I, O_ - 1, O_), (2, 4, 2, 3)]:
            for rel in range(0, O_ * I - n + 1):
                bits = sim().sim_sa_vector_bits(O_, I, rel, n, ilo, ihi, olo, ohi, oi)
                assert (oi[0], oi[1]) == divmod(rel, I)
                want = 0
                for k in range(n):
                    o, i = divmod(rel + k, I)
                    if ilo <= i < ihi or olo <= o < ohi:
                        want |= 1 << k
                assert bits == want, (O_, I, n, rel, ilo, ihi, olo, ohi)


def _aligned(shape, np_dtype, offset_bytes=0):
    n = int(np.prod(shape)) * np.dtype(np_dtype).itemsize
    raw = np.zeros(n + 64, np.uint8)
    at = (-raw.ctypes.data) % 16 + offset_bytes
    return raw[at:at + n].view(np_dtype).reshape(shape)


def sim_run(x, time_inner, axes, dtype, draws=None, params=None, bounds=None, value=0.0, value_tensor=False,
            force_gather=False, misalign=0):
    """x: (E, O, I) torch CPU tensor of any strides.  -> (bit view of the dense (E, O, I) result, dense path taken)"""
    E, O_, I = x.shape
    xb = x.view(O.BITS[x.element_size()]).numpy()                      # shares x's strides
    if xb.flags["C_CONTIGUOUS"]:
        buf = _aligned(xb.shape, xb.dtype, misalign)
        buf[...] = xb
        xb = buf
    out = _aligned(xb.shape, xb.dtype)
    out[...] = 0x55
    n = len(axes)
    ax = (C.c_int32 * max(n, 1))(*axes)
    es = xb.itemsize
    se, so, si = (s // es for s in xb.strides)
    vb = O.value_bits(value, dtype) & ((1 << (8 * es)) - 1)
    vt = np.array([vb], dtype=np.uint64).view(np.uint8)[:es].copy() if value_tensor else None
    if draws is not None:
        d = np.ascontiguousarray(O.bit_view(draws.to(dtype)).numpy())
        assert d.shape == (n, 2, E)
        pr = (C.c_int64 * max(n, 1))(*params)
        rc = sim().sim_sa_run(xb.ctypes.data, out.ctypes.data, E, O_, I, se, so, si, CODE[dtype], int(time_inner), n, ax, pr,
                              d.ctypes.data, None, None, 0 if value_tensor else vb, vt.ctypes.data if value_tensor else None,
                              int(force_gather))
    else:
        st = (C.c_int64 * max(n, 1))(*[b[0] for b in bounds])
        en = (C.c_int64 * max(n, 1))(*[b[1] for b in bounds])
        rc = sim().sim_sa_run(xb.ctypes.data, out.ctypes.data, E, O_, I, se, so, si, CODE[dtype], int(time_inner), n, ax, None,
                              None, st, en, 0 if value_tensor else vb, vt.ctypes.data if value_tensor else None,
                              int(force_gather))
    assert rc >= 0
    return out, rc == 1


def _special(x):
    """plant NaN (with a payload), infinities and -0.0"""
    flat = x.reshape(-1)
    vals = [float("nan"), float("inf"), -float("inf"), -0.0]
    for k, v in enumerate(vals):
        flat[(k * 7 + 1) % flat.numel()] = v
    return x


@pytest.mark.parametrize("dtype", DTYPES)
def test_sim_kernel_meets_the_loop_oracle(dtype):
    g = torch.Generator().manual_seed(4)
    for E, Fq, Tm in [(1, 1, 1), (3, 2, 3), (2, 5, 7), (3, 4, 9), (1, 80, 65), (3, 5, 63), (2, 81, 8), (1, 3, 257)]:
        x = _special(torch.randn(E, Fq, Tm, generator=g).to(dtype))
        # time masks first, as SpecAugment orders them; mask_param beyond the axis included; overlapping masks abound
        plan = [(O.TIME, max(Tm // 3, 1)), (O.TIME, Tm + 2), (O.FREQ, max(Fq // 2, 1)), (O.FREQ, 1), (O.TIME, 3)]
        d = torch.rand(len(plan), 2, E, generator=g)
        masks = [O.bounds(d[m], prm, Tm if a == O.TIME else Fq, dtype) for m, (a, prm) in enumerate(plan)]
        want = O.apply(x, masks, [a for a, _ in plan], -2.5)
        for layout in ("time", "frame", "sliced", "gather", "misaligned"):
            if layout == "frame":                                      # frame-major: (E, T, F) dense, frequency is inner
                x3, time_inner = x.transpose(1, 2).contiguous(), False
            elif layout == "sliced":
                big = torch.zeros(E, Fq + 1, 2 * Tm + 1, dtype=dtype)
                big[:, :Fq, 1:2 * Tm:2] = x
                x3, time_inner = big[:, :Fq, 1:2 * Tm:2], True
            else:
                x3, time_inner = x, True
            got, dense = sim_run(x3, time_inner, [a for a, _ in plan], dtype, draws=d, params=[m for _, m in plan], value=-2.5,
                                 value_tensor=layout == "frame", force_gather=layout == "gather",
                                 misalign=x.element_size() if layout == "misaligned" else 0)
            # (a one-element example is dense whatever its strides)
            assert dense == (layout in ("time", "frame") or (layout == "sliced" and x3.is_contiguous())), layout
            if not time_inner:
                got = got.transpose(0, 2, 1)
            assert np.array_equal(got, want), (E, Fq, Tm, layout)


def test_sim_pinned_touching_and_overlapping_masks():
    g = torch.Generator().manual_seed(5)
    for dtype in (torch.float32, torch.float16, torch.float64):
        for Fq, Tm in [(5, 9), (4, 64), (3, 65), (80, 7)]:
            x = _special(torch.randn(2, Fq, Tm, generator=g).to(dtype))
            cases = [[(0, 3)], [(Tm - 2, Tm)], [(0, Tm)], [(4, 4)], [(5, 6)], [(-7, 2)], [(Tm - 1, Tm + 50)],
                     [(1, 3), (3, 5)], [(1, 4), (2, 6)], [(0, 1), (Tm - 1, Tm)], [(k, k + 1) for k in range(0, 64, 2)]]
            for b in cases:
                for axis, size in ((O.TIME, Tm), (O.FREQ, Fq)):
                    want = O.apply(x, b, [axis] * len(b), 7.0)
                    for x3, time_inner in ((x, True), (x.transpose(1, 2).contiguous(), False)):
                        got, dense = sim_run(x3, time_inner, [axis] * len(b), dtype, bounds=b, value=7.0)
                        assert dense
                        assert np.array_equal(got if time_inner else got.transpose(0, 2, 1), want), (Fq, Tm, b, axis)
    # more than 32 masks are not one launch
    assert sim().sim_sa_run(None, None, 1, 1, 1, 1, 1, 1, 0, 1, 33, None, None, None, None, None, 0, None, 0) == -1


# ---- errors and the early return --------------------------------------------------------------------------------------------

def test_error_types_and_messages():
    x = torch.randn(2, 3, 8, 9)
    for fn in (F.mask_along_axis_iid, O.torch_reference_mask_along_axis_iid):
        with pytest.raises(ValueError, match="at least three dimensions"):
            fn(x[0, 0], 3, 0.0, 1)
        with pytest.raises(ValueError, match="Only Frequency and Time masking are supported"):
            fn(x, 3, 0.0, 1)
        with pytest.raises(ValueError, match="between 0.0 and 1.0"):
            fn(x, 3, 0.0, 3, p=1.5)
    for fn in (F.mask_along_axis, O.torch_reference_mask_along_axis):
        with pytest.raises(ValueError, match="at least two dimensions"):
            fn(x[0, 0, 0], 3, 0.0, 0)
        with pytest.raises(ValueError, match="Only Frequency and Time masking are supported"):
            fn(x, 3, 0.0, 0)
        with pytest.raises(ValueError, match="between 0.0 and 1.0"):
            fn(x, 3, 0.0, 2, p=-0.1)
    with pytest.raises(ValueError, match="between 0.0 and 1.0"):
        T.TimeMasking(10, p=1.2)
    with pytest.raises(ValueError, match="between 0.0 and 1.0"):
        T.SpecAugment(1, 10, 1, 10, p=2.0)(x)
    with pytest.raises(TypeError, match="floating-point"):
        F.mask_along_axis_iid(torch.ones(2, 3, 4, dtype=torch.int32), 2, 0.0, 2)
    with pytest.raises(TypeError, match="floating-point"):
        F.mask_along_axis(torch.ones(2, 3, 4, dtype=torch.int64), 2, 0.0, 2)
    with pytest.raises(TypeError, match="floating-point"):
        T.SpecAugment(1, 2, 1, 2)(torch.ones(2, 3, 4, dtype=torch.int32))


def test_early_return_is_the_same_object_and_draws_nothing():
    x = torch.randn(2, 3, 8, 9)
    torch.manual_seed(11)
    state = torch.get_rng_state()
    assert F.mask_along_axis_iid(x, 0, 0.0, 3) is x
    assert F.mask_along_axis(x, 0, 0.0, 2) is x
    assert F.mask_along_axis_iid(x, 100, 0.0, 3, p=0.1) is x           # int(9 * 0.1) == 0
    assert F.mask_along_axis(x, 100, 0.0, 3, p=0.1) is x
    assert T.TimeMasking(100, iid_masks=True, p=0.05)(x) is x
    assert T.TimeMasking(100, p=0.05)(x) is x
    assert T.FrequencyMasking(0)(x) is x
    assert T.SpecAugment(2, 100, 2, 0, p=0.05)(x) is x
    assert T.SpecAugment(0, 100, 0, 27)(x) is x
    assert torch.jit.script(T.SpecAugment(2, 100, 2, 0, p=0.05))(x) is x
    assert torch.jit.script(T.TimeMasking(100, True, 0.05))(x) is x
    assert torch.equal(torch.get_rng_state(), state)


# ---- op surface without a device --------------------------------------------------------------------------------------------

def _meta_calls(x):
    ops = torch.ops.audio_amd
    return [ops.mask_along_axis(x, 5, 0.0, x.dim() - 1, 1.0), ops.mask_along_axis_iid(x, 5, 0.0, x.dim() - 2, 1.0),
            ops.spec_augment(x, 2, 100, 2, 27, True, 1.0, False)]


@pytest.mark.parametrize("dtype", DTYPES)
def test_meta_shapes_and_strides(dtype):
    dense = torch.empty(2, 3, 80, 101, device="meta", dtype=dtype)
    frame_major = torch.empty(2, 3, 101, 80, device="meta", dtype=dtype).transpose(-1, -2)
    sliced = torch.empty(2, 3, 80, 202, device="meta", dtype=dtype)[..., ::2]
    for x, strides in [(dense, dense.stride()), (frame_major, frame_major.stride()), (sliced, dense.stride())]:
        for y in _meta_calls(x):
            assert y.shape == x.shape and y.dtype == dtype and y.stride() == strides
    assert frame_major.stride()[-2:] == (1, 80)


def test_torchscript_compiles_every_module():
    for mod, op in [(T.FrequencyMasking(27), "mask_along_axis"), (T.FrequencyMasking(27, iid_masks=True), "mask_along_axis_iid"),
                    (T.TimeMasking(100, p=0.2), "mask_along_axis"), (T.TimeMasking(100, iid_masks=True), "mask_along_axis_iid"),
                    (T.SpecAugment(2, 100, 2, 27), "spec_augment")]:
        sm = torch.jit.script(mod)
        g = str(sm.inlined_graph)
        assert g.count("audio_amd::") == g.count("audio_amd::" + op + "(") >= 1, op
        assert not list(mod.buffers()) and not list(mod.parameters())
    assert T.SpecAugment.__constants__ == ["n_time_masks", "time_mask_param", "n_freq_masks", "freq_mask_param", "iid_masks",
                                           "p", "zero_masking"]
    assert T.TimeMasking.__constants__ == ["mask_param", "axis", "iid_masks", "p"]
    m = T.TimeMasking(100, True, 0.2)
    assert (m.mask_param, m.axis, m.iid_masks, m.p) == (100, 2, True, 0.2)
    m = T.FrequencyMasking(27)
    assert (m.mask_param, m.axis, m.iid_masks, m.p) == (27, 1, False, 1.0)
    for fn in (F.mask_along_axis, F.mask_along_axis_iid):
        assert "audio_amd::" + fn.__name__ in str(torch.jit.script(fn).graph)


def test_torch_compile_on_meta_sees_one_op_per_module():
    graphs = []

    def backend(gm, example_inputs):
        graphs.append(gm)
        return gm.forward

    x = torch.empty(4, 101, 80, device="meta").transpose(-1, -2)
    for mod, op in [(T.SpecAugment(2, 100, 2, 27), "audio_amd.spec_augment"),
                    (T.SpecAugment(10, 100, 2, 27, iid_masks=False, zero_masking=True), "audio_amd.spec_augment"),
                    (T.TimeMasking(100, iid_masks=True, p=0.5), "audio_amd.mask_along_axis_iid"),
                    (T.FrequencyMasking(27), "audio_amd.mask_along_axis")]:
        y = torch.compile(mod, fullgraph=True, backend=backend)(x)
        assert y.shape == x.shape and y.stride() == x.stride()
        calls = [str(n.target) for n in graphs[-1].graph.nodes if n.op == "call_function"]
        assert calls == [op], calls


def test_cpu_tensors_are_refused():
    x = torch.randn(2, 8, 9)
    for call in (lambda: torch.ops.audio_amd.mask_along_axis(x, 3, 0.0, 2, 1.0),
                 lambda: torch.ops.audio_amd.mask_along_axis_iid(x, 3, 0.0, 2, 1.0),
                 lambda: torch.ops.audio_amd.spec_augment(x, 1, 3, 1, 3, True, 1.0, False)):
        with pytest.raises(NotImplementedError, match="CPU"):
            call()
    for call in (lambda: F.mask_along_axis(x, 3, 0.0, 2), lambda: F.mask_along_axis_iid(x.half(), 3, 0.0, 1),
                 lambda: T.SpecAugment(2, 3, 2, 3)(x), lambda: T.TimeMasking(3)(x), lambda: T.FrequencyMasking(3, True)(x),
                 lambda: F._spec_augment_apply(x, [(0, 1)], [1], 0.0),
                 lambda: F._spec_augment_apply(x, torch.rand(1, 2, 2), [(1, 3)], 0.0)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
