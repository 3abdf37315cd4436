"""F.overdrive / F.phaser / F.flanger on the device against the oracle (tests/effects_oracle.py): phaser and flanger bit for
bit in float32 and float64 (half types: the float32 oracle on the widened input, rounded once), overdrive at the issue's
tolerance; rows around the workgroup, dense and misaligned; lengths around the ring, the tile, the table's wrap and the
overdrive chunk; the streaming flanger against the general kernel; a NaN in one row; routes, limits and graph capture.
The shapes are the smallest at which the kernels can go wrong; the oracle runs once per parameter set (effects_cases.py)."""
import numpy as np
import pytest
import torch

import effects_cases as K
import effects_oracle as O
import audio_amd.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
WIDE = [torch.float32, torch.float64]
HALF = [torch.float16, torch.bfloat16]


def on_device(x, layout):
    """A CPU (rows, T) tensor on the device: dense, or as rows of a wider tensor (row stride T + 1) behind a storage offset of
    one element, so that the rows are misaligned."""
    if layout == "dense":
        return x.contiguous().to(DEV)
    rows, T = x.shape
    big = torch.zeros(rows * (T + 1) + 1, dtype=x.dtype)
    big[1:].view(rows, T + 1)[:, :T].copy_(x)
    return big.to(DEV)[1:].view(rows, T + 1)[:, :T]


def same_bits(got, want):
    return got.shape == want.shape and torch.equal(K.bits(got), K.bits(want))


def row_counts():
    R = F.effects_tiles()[0]
    return [1, 3, R - 1, R, R + 1, 2 * R + 2]


def check_result(out, x):
    assert out.shape == x.shape and out.dtype == x.dtype and out.is_contiguous() and out.device == x.device


# ---- phaser ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", WIDE)
@pytest.mark.parametrize("name", list(K.PHASER_SETS))
def test_phaser_equals_the_oracle_bit_for_bit(name, dtype):
    R, S, _ = F.effects_tiles()
    L, M = K.phaser_dims(name)
    Ts = K.lengths(L, S, M)
    x, want, share = K.phaser_ref(name, 2 * R + 2, max(Ts), dtype)
    print("phaser", name, dtype, "L", L, "M", M, "clamped share", share)
    assert (0.1 <= share <= 0.9) if name == "clamp" else share == 0.0       # a clamp that hides everything cannot pass
    p = K.PHASER_SETS[name]
    for rows in row_counts():                                                # every row count at two lengths
        for T, layout in ((S + 1, "dense"), (max(Ts), "wider")):
            xd = on_device(x[:rows, :T], layout)
            got = F.phaser(xd, **p)
            check_result(got, xd)
            assert same_bits(got.cpu(), want[:rows, :T]), (rows, T, layout)
    for i, T in enumerate(Ts):                                               # every length at two row counts
        for rows, layout in ((3, "wider" if i % 2 else "dense"), (R + 1, "dense" if i % 2 else "wider")):
            got = F.phaser(on_device(x[:rows, :T], layout), **p)
            assert same_bits(got.cpu(), want[:rows, :T]), (rows, T, layout)
    got = F.phaser(x[:6, :S + 1].reshape(2, 3, S + 1).to(DEV), **p)          # a leading shape
    assert same_bits(got.cpu(), want[:6, :S + 1].reshape(2, 3, S + 1))


@pytest.mark.parametrize("dtype", HALF)
def test_phaser_half_types_round_once(dtype):
    R, S, _ = F.effects_tiles()
    for name in ("L5", "clamp", "L300"):
        L, M = K.phaser_dims(name)
        T = 2 * M + L + 1
        x, want, _ = K.phaser_ref(name, R + 1, T, dtype)
        for rows, layout in ((3, "wider"), (R + 1, "dense")):
            got = F.phaser(on_device(x[:rows], layout), **K.PHASER_SETS[name])
            assert got.dtype == dtype and same_bits(got.cpu(), want[:rows]), (name, rows)


# ---- flanger --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", WIDE)
@pytest.mark.parametrize("name", list(K.FLANGER_SETS))
def test_flanger_equals_the_oracle_bit_for_bit(name, dtype):
    R, S, _ = F.effects_tiles()
    L, N = K.flanger_dims(name)
    Ts = K.lengths(L, S, N)
    p = K.FLANGER_SETS[name]
    streaming = p.get("regen", 0.0) == 0.0

    def run(xs, layout):
        b, c, T = xs.shape
        xd = on_device(xs.reshape(b * c, T), layout).view(b, c, T)
        got = F.flanger(xd, **p)
        check_result(got, xd)
        if streaming:                                                        # the streaming route against the general kernel
            assert same_bits(F.flanger(xd, **p, _general=True).cpu(), got.cpu()), (b, c, T, layout)
        return got.cpu()

    x, want, share = K.flanger_ref(name, R + 1, 2, max(Ts), dtype)           # two channels: up to 2 R + 2 rows
    print("flanger", name, dtype, "L", L, "N", N, "clamped share", share)
    assert share == 0.0
    for rows in row_counts():
        if rows % 2 == 0:
            for T, layout in ((S + 1, "dense"), (max(Ts), "wider")):
                assert same_bits(run(x[:rows // 2, :, :T], layout), want[:rows // 2, :, :T]), (rows, T)
    for i, T in enumerate(Ts):
        assert same_bits(run(x[:2, :, :T], "wider" if i % 2 else "dense"), want[:2, :, :T]), T
    for C, B in ((1, 3), (1, R - 1), (1, R + 1), (4, 2)):                    # odd row counts; every channel count
        x, want, share = K.flanger_ref(name, B, C, N + 5, dtype)
        assert share == 0.0
        assert same_bits(run(x, "wider"), want), (C, B)
    x, want, _ = K.flanger_ref(name, 1, 4, N + 5, dtype)                     # a 2-D (C, T) input
    got = F.flanger(x[0].to(DEV), **p)
    assert same_bits(got.cpu(), want[0])


@pytest.mark.parametrize("dtype", HALF)
def test_flanger_half_types_round_once(dtype):
    for name in ("default", "quadratic", "workspace", "stream_quadratic"):
        L, N = K.flanger_dims(name)
        x, want, _ = K.flanger_ref(name, 2, 2, 2 * N + L + 1, dtype)
        xd = on_device(x.reshape(4, -1), "wider").view(x.shape)
        got = F.flanger(xd, **K.FLANGER_SETS[name])
        assert got.dtype == dtype and same_bits(got.cpu(), want), name


# ---- overdrive ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", WIDE + HALF)
@pytest.mark.parametrize("name", list(K.OVERDRIVE_SETS))
def test_overdrive_meets_the_tolerance(name, dtype):
    R, _, Kc = F.effects_tiles()
    p = K.OVERDRIVE_SETS[name]
    Tmax = 2 * Kc + 3
    x, want, ref32, y = K.overdrive_ref(name, R + 1, Tmax, dtype)
    share = O.overdrive_saturated_share(K.compute_view(x), p["gain"], p["colour"])
    print("overdrive", name, dtype, "saturated share of the pre-stage", share)
    assert {"quiet": 0.05 < share < 0.4, "loud": 0.6 < share < 0.98, "unit": share == 0.0}[name]
    cases = [(rows, Kc + 1, "dense") for rows in (1, 3, R + 1)] + [(3, T, "wider" if i % 2 else "dense")
                                                                  for i, T in enumerate((1, 2, Kc - 1, Kc, Kc + 1, Tmax))]
    worst = 0.0
    for rows, T, layout in cases + [(6, Tmax, "lead")]:
        if layout == "lead":
            xd = x[:6].reshape(2, 3, Tmax).to(DEV)
        else:
            xd = on_device(x[:rows, :T], layout)
        got = F.overdrive(xd, p["gain"], p["colour"])
        check_result(got, xd)
        w, r, s = want[:rows, :T], ref32[:rows, :T], y[:rows, :T]
        bound = K.overdrive_bound(w, r, s, dtype)
        err = np.abs(got.double().cpu().numpy().reshape(rows, T) - w)
        ratio = float(np.max(err / bound))
        worst = max(worst, ratio)
        print("overdrive", name, dtype, (rows, T, layout), "max|got - want|", float(err.max()), "max|ref32 - want|",
              float(np.abs(r - w).max()), "bound", float(np.max(bound)), "ratio", ratio)
        assert (err <= bound).all(), (rows, T, layout)
    print("overdrive", name, dtype, "largest ratio", worst)


# ---- non-finite input -----------------------------------------------------------------------------------------------------------

def test_a_nan_stays_in_its_row():
    runs = {
        "phaser": (lambda t: F.phaser(t, **K.PHASER_SETS["L5"]), lambda a: O.phaser(a, dt=np.float32, **K._phaser_args("L5")), True),
        "flanger": (lambda t: F.flanger(t.view(1, 3, -1), **K.FLANGER_SETS["quadratic"]).view(3, -1),
                    lambda a: O.flanger(a.reshape(1, 3, -1), dt=np.float32, **K._flanger_args("quadratic")).reshape(3, -1), True),
        "overdrive": (F.overdrive, lambda a: O.overdrive(a, dt=np.float32), False),
    }
    Kc = F.effects_tiles()[2]
    for name, (run, ref, exact) in runs.items():
        T = Kc + 300 if name == "overdrive" else 300
        x = K.base_input(5, 0.5, 3, T, torch.float32).clone()
        clean = run(x.to(DEV)).cpu()
        x[1, 150] = float("nan")
        got = run(x.to(DEV)).cpu()
        want = ref(x.numpy())
        assert same_bits(got[[0, 2]], clean[[0, 2]]) and same_bits(got[1, :150], clean[1, :150]), name
        assert np.array_equal(np.isnan(got.numpy()), np.isnan(want)), name
        assert np.isnan(want[1, 150:]).any()
        if exact:
            fin = ~np.isnan(want)
            assert np.array_equal(got.numpy()[fin].view(np.int32), want[fin].view(np.int32)), name


# ---- routes and limits ----------------------------------------------------------------------------------------------------------

def test_two_calls_give_the_same_bits_and_empty_input():
    R, S, Kc = F.effects_tiles()
    x = K.base_input(6, 0.7, 2 * 3, 2 * Kc + 3, torch.float32).to(DEV)
    calls = {"overdrive": lambda t: F.overdrive(t), "phaser": lambda t: F.phaser(t, **K.PHASER_SETS["L5"]),
             "flanger": lambda t: F.flanger(t, **K.FLANGER_SETS["quadratic"]),
             "flanger, streaming": lambda t: F.flanger(t, **K.FLANGER_SETS["default"])}
    for name, fn in calls.items():
        a, b = fn(x.view(2, 3, -1)), fn(x.view(2, 3, -1))
        assert same_bits(a.cpu(), b.cpu()), name
        for dtype in WIDE + HALF:
            e = fn(torch.empty(2, 3, 0, dtype=dtype, device=DEV))
            assert e.shape == (2, 3, 0) and e.dtype == dtype
            e = fn(torch.empty(0, 3, 17, dtype=dtype, device=DEV))
            assert e.shape == (0, 3, 17)
    # a gathered input: time is not the unit-stride axis
    xt = x.view(2, 3, -1)[:, :, :S + 1].transpose(1, 2).contiguous().transpose(1, 2)
    assert xt.stride(-1) != 1
    assert same_bits(F.phaser(xt, **K.PHASER_SETS["L5"]).cpu(), F.phaser(xt.contiguous(), **K.PHASER_SETS["L5"]).cpu())


def test_limits_and_refusals():
    x = torch.zeros(2, 2, 16, device=DEV)
    with pytest.raises(NotImplementedError, match="512"):
        F.phaser(x, 96000, delay_ms=5.4)
    with pytest.raises(NotImplementedError, match="2\\^24"):
        F.phaser(x, 96000, mod_speed=0.005)
    with pytest.raises(NotImplementedError, match="4096"):
        F.flanger(x, 96000, delay=30.0, depth=13.0)
    with pytest.raises(NotImplementedError, match="2\\^24"):
        F.flanger(x, 96000, speed=0.005)
    with pytest.raises(RuntimeError, match="forward-only"):
        F.overdrive(torch.zeros(2, 16, device=DEV, requires_grad=True))
    with torch.no_grad():
        assert F.overdrive(torch.zeros(2, 16, device=DEV, requires_grad=True)).shape == (2, 16)
    # the largest rings the kernels serve do run: phaser 512 (LDS in float32), flanger 4096 (workspace)
    x = K.base_input(7, 0.5, 4, 700, torch.float32)
    got = F.phaser(x.to(DEV), 102400, delay_ms=5.0, mod_speed=400.0)
    assert same_bits(got.cpu(), K.stored(O.phaser(x.numpy(), 102400, delay_ms=5.0, mod_speed=400.0, dt=np.float32), torch.float32))
    got = F.flanger(x.view(2, 2, -1).to(DEV), 102350, delay=30.0, depth=10.0, speed=400.0, regen=20.0)
    want = O.flanger(x.view(2, 2, -1).numpy(), 102350, delay=30.0, depth=10.0, speed=400.0, regen=20.0, dt=np.float32)
    assert O.flanger_plan(102350, 2, delay=30.0, depth=10.0, speed=400.0)[0] == 4096
    assert same_bits(got.cpu(), K.stored(want, torch.float32))


def test_graph_capture():
    x = K.base_input(8, 0.6, 6, 700, torch.float32).to(DEV).view(2, 3, -1)
    fresh = dict(sample_rate=1000, delay_ms=7.0, mod_speed=2.5)                # no other test uses these parameters
    calls = {"overdrive": lambda t: F.overdrive(t), "phaser": lambda t: F.phaser(t, **K.PHASER_SETS["triangle"]),
             "flanger": lambda t: F.flanger(t, **K.FLANGER_SETS["triangular"]),
             "flanger, streaming": lambda t: F.flanger(t, **K.FLANGER_SETS["default"])}
    for name, fn in calls.items():
        eager = fn(x)                                                            # the table is on the device from here on
        static = x.clone()
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            fn(static)
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = fn(static)
        static.copy_(x)
        g.replay()
        torch.cuda.synchronize()
        assert same_bits(out.cpu(), eager.cpu()), name
    g = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="eagerly"):
        with torch.cuda.graph(g):
            doubled = x * 2                                                      # the capture is not empty
            F.phaser(doubled, **fresh)
    torch.cuda.synchronize()
    assert same_bits(F.phaser(x, **fresh).cpu(), K.stored(O.phaser(x.cpu().numpy(), 1000, delay_ms=7.0, mod_speed=2.5, dt=np.float32),
                                                          torch.float32))
