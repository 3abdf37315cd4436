"""The checks of F.vad / F.vad_start that the CPU replay (tests/test_vad.py) and the device (tests/test_gpu_vad.py) share.
A backend offers
    measures(x, sample_rate, **kw) -> float32 ndarray (rows, frames)   x: a 2-D torch tensor (any float dtype, rows of one
                                                                        stride, on the backend's device)
    trigger(meas, pl) -> (first, start, joint)                          meas: float32 ndarray (rows, frames), pl: O.Plan
    tensor(a) -> a torch tensor of ndarray a's values on the backend's device
"""
import math

import numpy as np
import torch

import vad_oracle as O


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def trig_plan(M, gap, P, fixed, level=7.0, trig=math.exp(-1.0 / 5.0)):
    return O.Plan(L=0, N=0, P=P, M=M, gap=gap, fixed=fixed, s0=0, s1=0, c0=0, c1=0, boot_max=0, up=0.0, down=0.0, smooth=0.0,
                  trig=trig, nra=0.0, level=level)


def synthetic_meas(seed, rows, frames, level=7.0):
    """Per element one of: 0, the float32 just below the level, the level, values above it, values below it, NaN, +inf."""
    rng = np.random.default_rng(seed)
    lv = np.float32(level)
    kind = rng.choice(7, size=(rows, frames), p=[0.3, 0.1, 0.1, 0.3, 0.15, 0.02, 0.03])
    m = np.zeros((rows, frames), np.float32)
    m[kind == 1] = np.nextafter(lv, np.float32(0))
    m[kind == 2] = lv
    m[kind == 3] = rng.uniform(level, 3 * level, size=(rows, frames)).astype(np.float32)[kind == 3]
    m[kind == 4] = rng.uniform(0.01, level, size=(rows, frames)).astype(np.float32)[kind == 4]
    m[kind == 5] = np.nan
    m[kind == 6] = np.inf
    return m


def trigger_grid():
    """(name, meas, plan): every M x gap x fixed x frames x rows of the issue's list, two mean multipliers."""
    out = []
    seed = 0
    for M in (1, 2, 20, 33):
        for gap in (0, 5, M + 3):
            for frames in (max(1, M // 2), M + 17):
                for rows in (1, 3, 67):
                    for fixed, trig in ((0, math.exp(-1.0 / 5.0)), (10 ** 6, 0.3)):
                        seed += 1
                        out.append(("M%d_gap%d_F%d_R%d_fixed%d" % (M, gap, frames, rows, fixed),
                                    synthetic_meas(seed, rows, frames), trig_plan(M, gap, 800, fixed, trig=trig)))
    return out


def constructed_cases():
    z = np.zeros(30, np.float32)
    never = z.copy()
    z50 = np.zeros(50, np.float32)                                                       # the ring stays behind frame 0
    low_then_loud = z50.copy(); low_then_loud[:30] = 5.0; low_then_loud[30:] = 20.0      # noqa: E702   first 30, flush 0
    zero_then_loud = z50.copy(); zero_then_loud[30:] = 20.0                              # noqa: E702   first 30, flush 1
    pl = trig_plan(20, 5, 800, 0, trig=0.5)
    same_frame = np.stack([low_then_loud, zero_then_loud])
    spike = z.copy(); spike[6] = 20.0; spike[15:] = 20.0                                 # noqa: E702   triggers late, flush 5 at 10
    loud8 = z.copy(); loud8[8:] = 20.0                                                   # noqa: E702   first = 10
    pl2 = trig_plan(20, 5, 800, 0)
    later_below = np.stack([spike, loud8])
    return [("same_frame_smaller_flush_on_lower_row", same_frame, pl, 23200), ("lower_row_triggers_later", later_below, pl2, 5600),
            # a row from r* on with nothing at the level in its ring flushes the whole ring: M - 1 = 19 measurements
            ("silent_row_after_the_trigger", np.stack([spike, loud8, never]), pl2, 0),
            ("nothing_triggers", np.stack([never, never]), pl, -1), ("no_frames", np.zeros((3, 0), np.float32), pl, -1)]


def check_trigger(backend, name, meas, pl, joint_want=None):
    first, start, joint = backend.trigger(meas, pl)
    want = [O.trigger_row(row, pl) for row in meas]
    assert [int(v) for v in first] == [w[0] for w in want], name
    assert [int(v) for v in start] == [w[1] for w in want], name
    assert int(joint) == O.trigger_joint(meas, pl), name
    if joint_want is not None:
        assert int(joint) == joint_want, name


def strided(backend, x, dtype=torch.float32):
    """x's rows cut from a wider buffer: a storage offset of one element and a row stride of T + 3."""
    t = backend.tensor(x).to(dtype)
    rows, T = t.shape
    big = torch.zeros(rows * (T + 3) + 1, dtype=dtype, device=t.device)
    view = big[1:].view(rows, T + 3)[:, :T]
    view.copy_(t)
    assert view.storage_offset() == 1 and view.stride(0) == T + 3
    return view


def check_measures(backend, name):
    x, sr, kw, m64, _, _ = O.group(name)
    kind = O.GROUPS[name][5]
    tol = O.tolerance(sr)
    t = backend.tensor(x)
    if kind == "f16":
        t = t.to(torch.float16)
    elif kind == "bf16":
        t = t.to(torch.bfloat16)
    elif kind == "f64":
        t = t.to(torch.float64) * (1 + 2e-9)
        assert torch.equal(t.to(torch.float32).cpu(), torch.from_numpy(np.array(x)))
    if kind != "f32":
        assert np.array_equal(t.to(torch.float32).cpu().numpy(), x)          # the oracle saw the compute type's values
    got = backend.measures(t, sr, **kw)
    assert got.shape == m64.shape and got.dtype == np.float32
    err = float(np.max(np.abs(got.astype(np.float64) - m64)))
    print("vad measures %s: err %.3e, tolerance %.3e (4 x err32 of the %d Hz group)" % (name, err, tol, sr))
    assert err <= tol, (name, err, tol)
    return got


def check_row_counts_and_offsets(backend, name="16k"):
    """1 and 3 rows, and rows at an odd element offset of a wider buffer, give the bits of the same rows in the full batch."""
    x, sr, kw, _, _, _ = O.group(name)
    full = backend.measures(backend.tensor(x), sr, **kw)
    assert np.array_equal(bits(backend.measures(backend.tensor(x[:1]), sr, **kw)), bits(full[:1]))
    assert np.array_equal(bits(backend.measures(backend.tensor(x[:3]), sr, **kw)), bits(full[:3]))
    assert np.array_equal(bits(backend.measures(strided(backend, x[:5]), sr, **kw)), bits(full[:5]))
    half = strided(backend, x[:3], torch.float16)
    want = backend.measures(half.contiguous(), sr, **kw)
    assert np.array_equal(bits(backend.measures(half, sr, **kw)), bits(want))


def check_nan_row(backend, name="16k_md064p"):
    x, sr, kw, _, _, _ = O.group(name)
    clean = backend.measures(backend.tensor(x), sr, **kw)
    pl = O.plan(sr, **kw)
    y = np.array(x)
    at = pl.L + 7 * pl.P - 3                       # inside frame 7's window, not in frame 5's
    y[1, at] = np.nan
    got = backend.measures(backend.tensor(y), sr, **kw)
    assert np.array_equal(bits(got[[0, 2]]), bits(clean[[0, 2]]))
    first_hit = (at - pl.L) // pl.P + 1            # the first frame whose window ends beyond `at`
    assert np.array_equal(bits(got[1, :first_hit]), bits(clean[1, :first_hit]))
    assert np.all(got[1, first_hit:] == 0)
    first, start, _ = backend.trigger(got, pl)
    want = [O.trigger_row(row, pl) for row in got]
    assert [int(v) for v in start] == [w[1] for w in want]


def check_short_rows(backend):
    """A row of exactly L samples has no frame, one of L + 1 has one."""
    x, sr, kw, _, _, _ = O.group("16k")
    pl = O.plan(sr, **kw)
    assert backend.measures(backend.tensor(x[:2, :pl.L]), sr, **kw).shape == (2, 0)
    got = backend.measures(backend.tensor(x[:2, :pl.L + 1]), sr, **kw)
    want = O.measures(x[:2, :pl.L + 1], sr, **kw)
    assert got.shape == want.shape == (2, 1)
    assert float(np.max(np.abs(got - want))) <= O.tolerance(sr)


def check_end_to_end(backend, name, got_meas=None):
    """The backend's own trigger on its own measurements equals the float64 oracle's start wherever the oracle has margin."""
    x, sr, kw, m64, u64, _ = O.group(name)
    pl = O.plan(sr, **kw)
    tol = O.tolerance(sr)
    meas = backend.measures(backend.tensor(x), sr, **kw) if got_meas is None else got_meas
    first, start, _ = backend.trigger(meas, pl)
    kept = [r for r in range(len(x)) if O.has_margin(m64[r], u64[r], pl, tol)]
    assert 4 * (len(x) - len(kept)) <= len(x)
    for r in kept:
        assert (int(first[r]), int(start[r])) == O.trigger_row(m64[r], pl), (name, r)
