"""Cases and checks of the ray-traced energy histograms shared by the CPU replay (tests/test_ray_tracing.py) and the device
(tests/test_gpu_ray_tracing.py).  A backend has ``run(room, source, mic, num_rays, absorption, scattering, mic_radius,
sound_speed, energy_thres, time_thres, hist_bin_size) -> numpy (B, M, NB, bins)`` over numpy inputs of one dtype: room (B, D),
source (B, D), mic (B, M, D), absorption and scattering (B, NB, 2 D); and ``tiles()``, the seven numbers of F.ray_tiles().

Rooms are seeded and generic -- about 6.1 x 5.3 x 3.2 m, the source near 0.31, 0.42, 0.53 of the room, the microphones in
the middle 60 % --, never round: the oracle reports the smallest margin of every discrete decision of a case, and
test_ray_tracing.py requires 1e-9 of every case, so that no float64 rounding difference between the oracle, the replay and
the device can flip a decision.  The seeds below were chosen for that (a scattered share st = 2 cos p_eq tr s sweeps a
continuum that reaches down to energy_thres, so a case with scattering keeps rays x bounces x microphones small).
References are computed once per case and shared."""
import functools
import zlib

import numpy as np

import ray_oracle as O

THREADS = 256                     # what the kernel exports; test_ray_tracing.py asserts it, since the ray counts straddle it
C = 343.0
MARGIN = 1e-9

# name: D, rays, M, B, bands, absorption, scattering, mic_radius, energy_thres, time_thres, hist_bin_size, seed
#   absorption: a number (all walls, all bands), "equal" (random walls, every band the same) or "unequal" (random per band)
#   scattering: a number, "wall" (0.4 on the north wall only, the others 0) or "unequal" (random per band and wall, some 0)
SHAPES = {
    "r1_m1_radius2": (3, 1, 1, 1, 1, 0.1, 0.0, 2.0, 1e-7, 0.1, 0.004, 0),
    "r63_m2_sc.3": (3, 63, 2, 1, 1, 0.1, 0.3, 0.5, 1e-7, 0.05, 0.004, 0),
    "r64_m5_nb3_unequal_sc.3": (3, 64, 5, 1, 3, "unequal", 0.3, 0.5, 1e-7, 0.05, 0.004, 0),
    "d2_r65_m1_tt.25": (2, 65, 1, 1, 1, 0.2, 0.0, 0.5, 1e-7, 0.25, 0.004, 0),
    "r255_m16_ab0_time_ends": (3, THREADS - 1, 16, 1, 1, 0.0, 0.0, 0.4, 1e-7, 0.05, 0.004, 0),
    "r256_m2_nb8_equal_wall": (3, THREADS, 2, 1, 8, "equal", "wall", 0.5, 1e-7, 0.1, 0.004, 2),
    "r257_m1_nb8_unequal_hb.0037": (3, THREADS + 1, 1, 1, 8, "unequal", "unequal", 0.3, 2e-4, 0.1, 0.0037, 0),
    "r300_m5_energy_ends": (3, 300, 5, 1, 1, 0.3, 0.0, 0.5, 1e-3, 0.25, 0.004, 0),
    "r300_m2_sc.3_energy_ends": (3, 300, 2, 1, 1, 0.3, 0.3, 0.5, 1e-3, 0.25, 0.004, 0),
    "d2_r300_m2_nb3_sc.3": (2, 300, 2, 1, 3, "equal", 0.3, 0.5, 5e-4, 0.1, 0.004, 0),
    "b3_r65_m2_nb3": (3, 65, 2, 3, 3, "unequal", "wall", 0.5, 1e-7, 0.1, 0.004, 0),
}
DTYPES = {"f32": np.float32, "f64": np.float64}
BATCH = "b3_r65_m2_nb3"


def rooms(seed: int, B: int, M: int, D: int, NB: int, absorption, scattering, dtype):
    """B seeded generic rooms with their coefficients, rounded to `dtype`, which is what a backend and the oracle both read."""
    rng = np.random.default_rng(seed)
    room = (np.array([6.1, 5.3, 3.2])[:D] * rng.uniform(0.85, 1.15, (B, D)))
    source = room * (np.array([0.31, 0.42, 0.53])[:D] + rng.uniform(-0.05, 0.05, (B, D)))
    mic = room[:, None] * rng.uniform(0.2, 0.8, (B, M, D))

    def coefficients(kind, lo, hi):
        if kind == "equal":
            return np.repeat(rng.uniform(lo, hi, (B, 1, 2 * D)), NB, axis=1)
        if kind == "unequal":
            return rng.uniform(lo, hi, (B, NB, 2 * D))
        if kind == "wall":
            c = np.zeros((B, NB, 2 * D))
            c[:, :, 3] = 0.4
            return c
        return np.full((B, NB, 2 * D), float(kind))

    ab = coefficients(absorption, 0.05, 0.5)
    sc = coefficients(scattering, 0.1, 0.5)
    if scattering == "unequal":
        sc[:, :, 0] = 0.0                                            # a wall that scatters in no band
        sc[:, ::2, 4] = 0.0                                          # and one that scatters in some
    return tuple(t.astype(dtype) for t in (room, source, mic, ab, sc))


def params(name: str):
    D, N, M, B, NB, _, _, R, ethr, tt, hb, _ = SHAPES[name]
    return dict(mic_radius=R, sound_speed=C, energy_thres=ethr, time_thres=tt, hist_bin_size=hb)


@functools.lru_cache(maxsize=None)
def case(name: str, dt: str):
    """(inputs, the float64 oracle's results per room, the bar per element, the smallest margin) of a shape in a dtype.  The bar
    is 4 x the largest distance of the float64 oracle's float sum from its longdouble form, plus count 2^-(k+1) for the
    quantisation of the contributions, plus, for float32, half an ulp of the oracle value."""
    D, N, M, B, NB, absorption, scattering, R, ethr, tt, hb, seed = SHAPES[name]
    dtype = DTYPES[dt]
    inputs = rooms(1000 * (zlib.crc32(name.encode()) % 100000) + 2 * seed + (dt == "f64"), B, M, D, NB, absorption, scattering, dtype)
    room, source, mic, ab, sc = inputs
    kw = params(name)
    o64 = [O.trace(room[b], source[b], mic[b], N, ab[b], sc[b], dtype=np.float64, **kw) for b in range(B)]
    old = [O.trace(room[b], source[b], mic[b], N, ab[b], sc[b], dtype=O.LD, **kw) for b in range(B)]
    own = max(float(np.abs(o.hist.astype(O.LD) - l.hist).max()) for o, l in zip(o64, old))
    hist = np.stack([o.hist for o in o64])
    count = np.stack([o.count for o in o64])
    bar = 4.0 * own + count[:, :, None, :] * 2.0 ** -(o64[0].k + 1) + np.zeros_like(hist)
    if dt == "f32":
        bar = bar + 0.5 * np.spacing(np.abs(hist).astype(np.float32)).astype(np.float64)
    for t in inputs + (hist, count, bar):
        t.setflags(write=False)
    return inputs, o64, hist, count, bar, min(o.margin for o in o64)


def run_case(backend, name: str, dt: str):
    (room, source, mic, ab, sc), *_ = case(name, dt)
    return backend.run(room, source, mic, SHAPES[name][1], ab, sc, **params(name))


def check_accuracy(backend, name: str, dt: str) -> float:
    inputs, o64, hist, count, bar, margin = case(name, dt)
    out = run_case(backend, name, dt)
    assert out.shape == hist.shape and out.dtype == DTYPES[dt]
    assert np.isfinite(out).all()
    err = np.abs(out.astype(np.float64) - hist)
    share = float((err / bar).max()) if bar.min() > 0 else float((err > bar).any())
    fixed = np.stack([O.final(o.acc, o.k, DTYPES[dt]) for o in o64])
    print(f"ray {name} {dt}: share of the bar {share:.3f}; margin {margin:.2e}; contributions {int(count.sum())}, fullest bin "
          f"{max(o.fullest for o in o64)}, largest / bound {max(o.top for o in o64):.3f}; bounces {max(o.bounces for o in o64)} of "
          f"{max(o.bound for o in o64)}; equal to the fixed-point oracle: {np.array_equal(out, fixed)}")
    assert count.sum() > 0 and hist.max() > 0                        # the case does have energy in it
    assert not out[np.broadcast_to(count[:, :, None, :] == 0, out.shape)].any()   # bins the oracle leaves empty are exactly 0
    assert (err <= bar).all(), (name, dt, share)
    return share


def check_reproducible(backend, name: str = "r257_m1_nb8_unequal_hb.0037", dt: str = "f32"):
    a, b = run_case(backend, name, dt), run_case(backend, name, dt)
    assert a.tobytes() == b.tobytes()


def check_rows_are_rooms(backend, dt: str):
    """Row b of a batch call is the single-room call on room b, bit for bit; a microphone alone gives its rows of the call."""
    (room, source, mic, ab, sc), *_ = case(BATCH, dt)
    N, kw = SHAPES[BATCH][1], params(BATCH)
    full = backend.run(room, source, mic, N, ab, sc, **kw)
    rows = [backend.run(room[b:b + 1], source[b:b + 1], mic[b:b + 1], N, ab[b:b + 1], sc[b:b + 1], **kw)[0] for b in range(room.shape[0])]
    assert np.stack(rows).tobytes() == full.tobytes()
    assert len({r.tobytes() for r in rows}) == len(rows)             # the rooms do differ
    for name in (BATCH, "r64_m5_nb3_unequal_sc.3"):
        (room, source, mic, ab, sc), *_ = case(name, dt)
        N, kw = SHAPES[name][1], params(name)
        full = backend.run(room, source, mic, N, ab, sc, **kw)
        for m in range(mic.shape[1]):
            one = backend.run(room, source, mic[:, m:m + 1], N, ab, sc, **kw)
            assert one.tobytes() == np.ascontiguousarray(full[:, m:m + 1]).tobytes(), (name, m)


def check_equal_bands(backend, dt: str):
    """Bands with equal coefficient rows are equal to each other; bands with unequal rows are not."""
    for name in ("r256_m2_nb8_equal_wall", "d2_r300_m2_nb3_sc.3"):
        out = run_case(backend, name, dt)
        for band in range(1, out.shape[2]):
            assert out[:, :, band].tobytes() == out[:, :, 0].tobytes(), (name, band)
    out = run_case(backend, "r257_m1_nb8_unequal_hb.0037", dt)
    assert len({out[:, :, band].tobytes() for band in range(out.shape[2])}) == out.shape[2]


def bad_rooms(dt: str):
    """(kind, inputs) with room 1 of the batch case made bad in each of the ways of the contract."""
    (room, source, mic, ab, sc), *_ = case(BATCH, dt)
    out = []
    for kind in ("dimension nan", "dimension zero", "dimension inf", "source on a wall", "microphone outside", "absorption 1.5",
                 "scattering nan", "scattering negative", "bounce bound"):
        r, s, m, a, c = (t.copy() for t in (room, source, mic, ab, sc))
        if kind.startswith("dimension"):
            r[1, 1] = {"nan": np.nan, "zero": 0.0, "inf": np.inf}[kind.split()[1]]
        elif kind == "source on a wall":
            s[1, 0] = 0.0
        elif kind == "microphone outside":
            m[1, -1, 2] = r[1, 2] * 1.25
        elif kind == "absorption 1.5":
            a[1, 2, 4] = 1.5
        elif kind == "scattering nan":
            c[1, 0, 0] = np.nan
        elif kind == "scattering negative":
            c[1, 1, 5] = -0.25
        else:                                                        # a floor-to-ceiling gap of 5 mm: S_max / 0.005 > 4096 bounces
            r[1, 2], s[1, 2], m[1, :, 2] = 0.005, 0.002, 0.003
            assert O.bounce_bound(r[1], params(BATCH)["time_thres"], C) > O.MAX_BOUNCES
        assert O.bad_room(r[1], s[1], m[1], a[1], c[1], params(BATCH)["time_thres"], C)
        out.append((kind, (r, s, m, a, c)))
    return out


def check_bad_rooms(backend, dt: str):
    """A bad room is NaN throughout, and its neighbours keep their bits."""
    clean = run_case(backend, BATCH, dt)
    N, kw = SHAPES[BATCH][1], params(BATCH)
    for kind, (r, s, m, a, c) in bad_rooms(dt):
        out = backend.run(r, s, m, N, a, c, **kw)
        assert np.isnan(out[1]).all(), kind
        assert out[0].tobytes() == clean[0].tobytes() and out[2].tobytes() == clean[2].tobytes(), kind
