"""Waveform augmentation without a GPU: the two forms of the float64 oracle against each other, a CPU replay of
csrc/wave_augment.h (reduce + apply in forward and gradient mode, pre-emphasis and its transpose, four dtypes, aligned and
misaligned rows, broadcast rows, lengths, zero energies) against the oracle, error types and messages, Meta shapes,
TorchScript and the refusal of CPU tensors."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import wave_augment_oracle as O
import audio_amd.functional as F
import audio_amd.transforms as T
from audio_amd import _ops  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
SIM_SRC = os.path.join(HERE, "cpu_sim", "sim_wave_augment.cpp")
SIM_OUT = os.path.join(HERE, "cpu_sim", "_build", "libaamd_sim_wave_augment.so")
HDRS = [os.path.join(os.path.dirname(HERE), "audio_amd", "csrc", h) for h in ("wave_augment.h", "spec_augment.h", "hd.h")]
CODE = {torch.float32: 0, torch.float64: 1, torch.float16: 2, torch.bfloat16: 3}
CHUNK = F.WAVE_AUGMENT_CHUNK
LENGTHS = [1, 2, 3, 4, 5, 1023, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3]

_sim = None


def sim():
    global _sim
    if _sim is None:
        newest = max(os.path.getmtime(p) for p in [SIM_SRC] + HDRS)
        if not os.path.exists(SIM_OUT) or newest > os.path.getmtime(SIM_OUT):
            os.makedirs(os.path.dirname(SIM_OUT), exist_ok=True)
            tmp = "%s.tmp.%d" % (SIM_OUT, os.getpid())
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", SIM_SRC, "-o", tmp])
            os.replace(tmp, SIM_OUT)
        _sim = C.CDLL(SIM_OUT)
        i64, i32, p = C.c_int64, C.c_int, C.c_void_p
        _sim.sim_wa_workspace_doubles.argtypes = [i64, i64]
        _sim.sim_wa_workspace_doubles.restype = i64
        _sim.sim_wa_add_noise.argtypes = [i32] + [p] * 6 + [i64] * 5 + [p, i64, p, i64, i32]
        _sim.sim_wa_preemphasis.argtypes = [i32, p, p, i64, i64, i64, C.c_double, i32]
    return _sim


def _rs(t):
    return t.stride(0) if t.shape[0] > 1 else 0


def sim_add_noise(w, n, snr, lengths=None, g=None):
    """w, n (and g): (rows, L) CPU tensors of any row stride (0: expanded); snr float64 (rows,), lengths int64 (rows,)."""
    rows, L = w.shape
    out = torch.empty((rows, L), dtype=w.dtype)
    out2 = torch.empty((rows, L), dtype=w.dtype) if g is not None else None
    ws = torch.zeros(int(sim().sim_wa_workspace_doubles(rows, L)), dtype=torch.float64)
    snr = snr.to(torch.float64)
    rc = sim().sim_wa_add_noise(CODE[w.dtype], w.data_ptr(), n.data_ptr(), g.data_ptr() if g is not None else None,
                                out.data_ptr(), out2.data_ptr() if g is not None else None, ws.data_ptr(), rows, L, _rs(w),
                                _rs(n), _rs(g) if g is not None else 0, snr.data_ptr(), _rs(snr),
                                lengths.data_ptr() if lengths is not None else None,
                                _rs(lengths) if lengths is not None else 0, int(g is not None))
    assert rc == 0
    return (out, out2, ws[:rows].clone()) if g is not None else out


def sim_preemphasis(x, coeff, transposed=False):
    out = torch.empty(x.shape, dtype=x.dtype)
    assert sim().sim_wa_preemphasis(CODE[x.dtype], x.data_ptr(), out.data_ptr(), x.shape[0], x.shape[1], _rs(x), coeff,
                                    int(transposed)) == 0
    return out


def misaligned_rows(rows, L, dtype, gen, offset=1, pad=1):
    """(rows, L) cut from a wider buffer: a storage offset of `offset` elements and a row stride of L + pad."""
    base = (torch.rand(rows * (L + pad) + offset + 8, generator=gen, dtype=torch.float64) - 0.5).to(dtype)
    return base[offset:offset + rows * (L + pad)].view(rows, L + pad)[:, :L]


def ordered_bits(t):
    b = t.view(torch.int16).to(torch.int32)
    return torch.where(b < 0, -(b & 0x7fff), b)


# ---- the oracle's two forms ---------------------------------------------------------------------------------------------------

def test_oracle_forms_agree():
    rng = np.random.default_rng(0)
    w, n = rng.standard_normal((3, 37)), rng.standard_normal((1, 37))
    snr = np.array([-20.0, 0.0, 35.0])
    for lengths in (None, np.array([0, 20, 44])):
        a = O.add_noise(w, n, snr, lengths)
        b, scales = O.add_noise_loop(w, n, snr, lengths)
        fin = np.isfinite(a)
        assert np.array_equal(np.isnan(a), np.isnan(b))
        np.testing.assert_allclose(a[fin], b[fin], rtol=1e-12, atol=0)
    x = rng.standard_normal((2, 3, 11))
    for dt in (np.float32, np.float64):
        assert np.array_equal(O.preemphasis(x, 0.97, dt), O.preemphasis_loop(x, 0.97, dt))
    # the transpose really is the adjoint: <P x, g> = <x, P^T g>
    g = rng.standard_normal((2, 3, 11))
    np.testing.assert_allclose(np.sum(O.preemphasis(x) * g), np.sum(x * O.preemphasis_transposed(g)), rtol=1e-12)
    assert O.convolve(x, rng.standard_normal((1, 3, 4)), "valid").shape == (2, 3, 8)
    assert O.convolve(x, rng.standard_normal((1, 3, 4)), "same").shape == (2, 3, 11)


def test_oracle_zero_energy_rows():
    w = np.array([[0.0, 0.0, 0.0], [1.0, 2.0, 0.0], [0.0, 0.0, 0.0]])
    n = np.array([[1.0, 0.0, 2.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]])
    a = O.add_noise(w, n, np.zeros(3))
    b, scales = O.add_noise_loop(w, n, np.zeros(3))
    assert scales[0] == 0.0 and scales[1] == np.inf and np.isnan(scales[2])
    assert np.array_equal(a[0], w[0]) and np.isnan(a[1]).all() and np.isnan(a[2]).all()
    assert np.array_equal(np.isnan(a), np.isnan(b))


# ---- CPU replay of csrc/wave_augment.h ------------------------------------------------------------------------------------------

def test_sim_chunk_is_the_exported_constant():
    assert sim().sim_wa_chunk() == CHUNK


@pytest.mark.parametrize("L", LENGTHS)
def test_sim_add_noise_f32_and_f64(L):
    gen = torch.Generator().manual_seed(L)
    snr = torch.tensor([-20.0, 0.0, 35.0], dtype=torch.float64)
    lens = torch.tensor([L + 7, max(L // 2, 1), L], dtype=torch.int64)
    for dtype, eps, k in ((torch.float32, 2.0 ** -23, 2.0), (torch.float64, 2.0 ** -44, 1.0)):
        w = misaligned_rows(3, L, dtype, gen)                       # offset of one element, row stride L + 1
        n = (torch.rand(1, L, generator=gen, dtype=torch.float64) - 0.5).to(dtype).expand(3, L)    # one shared noise row
        for lengths in (None, lens):
            got = sim_add_noise(w, n, snr, lengths).double().numpy()
            ln = None if lengths is None else lengths.numpy()
            want = O.add_noise(w.numpy(), n.numpy(), snr.numpy(), ln)
            s = O.add_noise_scale(w.numpy(), n.numpy(), snr.numpy(), ln)[:, None]
            bound = eps * (np.abs(w.double().numpy()) + k * np.abs(s * n.double().numpy()))
            assert (np.abs(got - want) <= bound).all(), (dtype, L, lengths)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_sim_add_noise_half_is_the_float32_result_rounded(dtype):
    gen = torch.Generator().manual_seed(5)
    for L in (5, 1023, CHUNK + 1):
        w = misaligned_rows(3, L, dtype, gen)
        n = misaligned_rows(3, L, dtype, gen, offset=3, pad=2)
        snr = torch.tensor([-20.0, 0.0, 35.0], dtype=torch.float64)
        lens = torch.tensor([L, 1, L + 7])
        got = sim_add_noise(w, n, snr, lens)
        ref = sim_add_noise(w.float().contiguous(), n.float().contiguous(), snr, lens).to(dtype)
        assert (ordered_bits(got) - ordered_bits(ref)).abs().max() <= 1


def test_sim_add_noise_zero_energy_rows():
    L = CHUNK + 5
    w = torch.zeros(4, L)
    n = torch.zeros(4, L)
    w[1, :7] = 1.0          # silent noise
    n[0, 3] = 2.0           # silent signal
    w[3, 10:] = 1.0         # energy beyond the length only: both silent under lengths = 10
    n[3, 10:] = 1.0
    lens = torch.tensor([L, L, L, 10])
    got = sim_add_noise(w, n, torch.zeros(4, dtype=torch.float64), lens).numpy()
    want = O.add_noise(w.numpy(), n.numpy(), np.zeros(4), lens.numpy())
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want))
    assert np.array_equal(got[0], w[0].numpy()) and np.isnan(got[2]).all() and np.isnan(got[3]).all()


def test_sim_lengths_of_zero_and_beyond():
    L = 1023
    gen = torch.Generator().manual_seed(9)
    w, n = torch.rand(3, L, generator=gen) - 0.5, torch.rand(3, L, generator=gen) - 0.5
    snr = torch.zeros(3, dtype=torch.float64)
    full = sim_add_noise(w, n, snr)
    got = sim_add_noise(w, n, snr, torch.tensor([0, L, L + 7]))
    assert np.isnan(got[0].numpy()).all()                       # a length of 0: both energies zero
    assert torch.equal(got[1:], full[1:])                       # a length at or beyond L masks nothing


def test_sim_add_noise_gradient_mode():
    gen = torch.Generator().manual_seed(11)
    for L in (37, CHUNK + 1):
        w = misaligned_rows(3, L, torch.float64, gen)
        n = (torch.rand(1, L, generator=gen, dtype=torch.float64) - 0.5).expand(3, L)
        g = torch.rand(3, L, generator=gen, dtype=torch.float64) - 0.5
        snr = torch.tensor([-20.0, 0.0, 35.0], dtype=torch.float64)
        for lengths in (None, torch.tensor([L, max(L // 2, 1), 5])):
            gw, gn, gs = sim_add_noise(w, n, snr, lengths, g)
            wt = w.clone().requires_grad_()
            nt = n.clone().requires_grad_()
            st = snr.clone().requires_grad_()
            if lengths is not None:
                mask = torch.arange(L) < lengths.unsqueeze(-1)
                mw, mn = wt * mask, nt * mask
            else:
                mw, mn = wt, nt
            es, en = (mw * mw).sum(-1), (mn * mn).sum(-1)
            scale = 10 ** ((10 * (torch.log10(es) - torch.log10(en)) - st) / 20.0)
            out = wt + scale.unsqueeze(-1) * nt
            rw, rn, rs = torch.autograd.grad(out, [wt, nt, st], g)
            torch.testing.assert_close(gw, rw, rtol=1e-11, atol=1e-13)
            torch.testing.assert_close(gn, rn, rtol=1e-11, atol=1e-13)
            torch.testing.assert_close(gs, rs, rtol=1e-11, atol=1e-13)


@pytest.mark.parametrize("L", LENGTHS)
def test_sim_preemphasis_is_exact_in_float32_and_float64(L):
    gen = torch.Generator().manual_seed(100 + L)
    for dtype, npdt in ((torch.float32, np.float32), (torch.float64, np.float64)):
        for x in (misaligned_rows(3, L, dtype, gen), (torch.rand(1, L, generator=gen, dtype=torch.float64) - 0.5).to(dtype)):
            got = sim_preemphasis(x, 0.97).numpy()
            assert np.array_equal(got, O.preemphasis(x.numpy(), 0.97, npdt)), (dtype, L)
            got_t = sim_preemphasis(x, 0.97, transposed=True).numpy()
            assert np.array_equal(got_t, O.preemphasis_transposed(x.numpy(), 0.97, npdt)), (dtype, L)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_sim_preemphasis_half_within_one_ulp(dtype):
    gen = torch.Generator().manual_seed(3)
    for L in (1, 7, 8, 9, 1023, CHUNK + 1):
        x = misaligned_rows(2, L, dtype, gen)
        got = sim_preemphasis(x, 0.97)
        want = torch.from_numpy(O.preemphasis(x.double().numpy(), float(np.float32(0.97)))).to(dtype)
        assert (ordered_bits(got) - ordered_bits(want)).abs().max() <= 1


# ---- host side: checks, shapes, scripting, refusal of CPU tensors ---------------------------------------------------------------

def test_add_noise_checks_and_messages():
    w, n, snr = torch.zeros(2, 8), torch.zeros(2, 8), torch.zeros(2)
    with pytest.raises(ValueError, match="Input leading dimensions don't match."):
        F.add_noise(w, n, torch.zeros(2, 1))
    with pytest.raises(ValueError, match="Input leading dimensions don't match."):
        F.add_noise(w, torch.zeros(8), snr)
    with pytest.raises(ValueError, match="Input leading dimensions don't match."):
        F.add_noise(w, n, snr, torch.zeros(2, 1))
    with pytest.raises(ValueError, match=r"Length dimensions of waveform and noise don't match \(got 8 and 9\)."):
        F.add_noise(w, torch.zeros(2, 9), snr)
    with pytest.raises(TypeError, match="float16, bfloat16, float32 or float64"):
        F.add_noise(w.to(torch.int16), n.to(torch.int16), snr)
    with pytest.raises(TypeError, match="snr"):
        F.add_noise(w, n, torch.zeros(2, dtype=torch.int64))


def test_cpu_tensors_are_refused():
    w, n, snr = torch.zeros(2, 8), torch.zeros(2, 8), torch.zeros(2)
    for call in (lambda: F.add_noise(w, n, snr), lambda: T.AddNoise()(w, n, snr, torch.tensor([3, 4])),
                 lambda: F.preemphasis(w), lambda: T.Preemphasis()(w), lambda: F.deemphasis(w), lambda: T.Deemphasis()(w),
                 lambda: F.convolve(w, n), lambda: T.Convolve()(w, n)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(TypeError):
        F.preemphasis(torch.zeros(2, 8, dtype=torch.int32))


def test_convolve_checks_and_messages():
    with pytest.raises(ValueError, match="The operands must be the same dimension"):
        F.convolve(torch.zeros(2, 8), torch.zeros(8))
    with pytest.raises(ValueError, match="Leading dimensions of x and y are not broadcastable"):
        F.convolve(torch.zeros(2, 8), torch.zeros(3, 8))
    with pytest.raises(ValueError, match="Unrecognized mode value 'circular'"):
        F.convolve(torch.zeros(2, 8), torch.zeros(2, 3), "circular")
    with pytest.raises(ValueError, match="Unrecognized mode value 'circular'"):
        T.Convolve("circular")                              # checked in the constructor, as T.FFTConvolve does


def test_signatures_are_the_references():
    import inspect
    assert str(inspect.signature(F.add_noise)) == \
        "(waveform: 'Tensor', noise: 'Tensor', snr: 'Tensor', lengths: 'Optional[Tensor]' = None) -> 'Tensor'"
    assert list(inspect.signature(F.preemphasis).parameters) == ["waveform", "coeff"]
    assert inspect.signature(F.preemphasis).parameters["coeff"].default == 0.97
    assert inspect.signature(F.deemphasis).parameters["coeff"].default == 0.97
    assert list(inspect.signature(F.convolve).parameters) == ["x", "y", "mode"]
    assert inspect.signature(F.convolve).parameters["mode"].default == "full"
    assert T.Preemphasis().coeff == 0.97 and T.Deemphasis(0.9).coeff == 0.9 and T.Convolve().mode == "full"
    for name in ("add_noise", "preemphasis", "deemphasis", "convolve"):
        assert name in F.__all__
    for name in ("AddNoise", "Preemphasis", "Deemphasis", "Convolve"):
        assert name in T.__all__


def test_meta_kernels():
    m = lambda *shape, dtype=torch.float32: torch.empty(shape, device="meta", dtype=dtype)
    out = torch.ops.audio_amd.add_noise(m(3, 2, 16, dtype=torch.bfloat16), m(1, 1, 16, dtype=torch.bfloat16), m(3, 1), None)
    assert out.shape == (3, 2, 16) and out.dtype == torch.bfloat16
    out = torch.ops.audio_amd.add_noise(m(1, 16), m(4, 16), m(1), m(4, dtype=torch.int64))
    assert out.shape == (4, 16)
    x = m(4, 33)[:, 1:]
    for op in (torch.ops.audio_amd.preemphasis, torch.ops.audio_amd.deemphasis):
        out = op(x, 0.97)
        assert out.shape == (4, 32) and out.is_contiguous()
    assert torch.ops.audio_amd.convolve(m(2, 5), m(1, 300), "full").shape == (2, 304)
    assert torch.ops.audio_amd.convolve(m(2, 5), m(1, 300), "same").shape == (2, 5)
    assert torch.ops.audio_amd.convolve(m(2, 5), m(1, 300), "valid").shape == (2, 296)


def test_modules_compile_under_torchscript():
    for mod in (T.AddNoise(), T.Preemphasis(0.9), T.Deemphasis(0.9), T.Convolve("same")):
        s = torch.jit.script(mod)
        assert "audio_amd::" in str(s.inlined_graph)
    s = torch.jit.script(T.AddNoise())
    with pytest.raises(Exception, match="CPU"):           # the op has no CPU kernel: refused by the dispatcher
        s(torch.zeros(2, 8), torch.zeros(2, 8), torch.zeros(2), None)
