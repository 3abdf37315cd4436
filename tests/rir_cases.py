"""Cases and checks of the image-source room simulation shared by the CPU replay (tests/test_rir.py) and the device
(tests/test_gpu_rir.py).  A backend has ``run(room, source, mic, max_order, absorption, L, fl=81, sample_rate=16000.0,
sound_speed=343.0) -> numpy (B, M, L)`` over numpy inputs of one dtype: room (B, D), source (B, D), mic (B, M, D), absorption
(B, 2 D); and ``tiles() -> (samples per workgroup, images per chunk, largest filter, largest order)``.

Rooms are seeded; every microphone is kept at least 0.1 m from every image (asserted with the oracle's distances), so no
case rests on a near-singular amplitude.  References are computed once per case and shared."""
import functools

import numpy as np

import rir_oracle as O

TILE, CHUNK = 512, 256            # what the kernel exports; test_rir.py asserts it, since the shapes below straddle them
FS, C = 16000.0, 343.0

# name: (D, max_order, M, B, L, fl)
SHAPES = {
    "n0_m1_b1_tile-1": (3, 0, 1, 1, TILE - 1, 81),
    "n1_m3_b1_tile": (3, 1, 3, 1, TILE, 81),
    "n3_m3_b5_tile+1": (3, 3, 3, 5, TILE + 1, 81),
    "d2_n2_m3_b5_2tile+3": (2, 2, 3, 5, 2 * TILE + 3, 81),
    "n5_231img_m1_b1_tile+1": (3, 5, 1, 1, TILE + 1, 81),
    "n6_377img_m3_b1_2tile+3": (3, 6, 3, 1, 2 * TILE + 3, 81),
    "n3_m1_b1_tile_fl3": (3, 3, 1, 1, TILE, 3),
    "n3_m3_b5_tile+1_fl255": (3, 3, 3, 5, TILE + 1, 255),
    "n3_m1_b1_len1": (3, 3, 1, 1, 1, 81),
    "n1_m1_b1_before_direct_path": (3, 1, 1, 1, 20, 81),
}
DTYPES = {"f32": np.float32, "f64": np.float64}


def rooms(seed: int, B: int, M: int, D: int, dtype, max_order: int):
    """B seeded rooms of 3 - 6 m a side (2.4 - 3.5 m high) with the source and the microphones at least 0.5 m from the walls
    and every microphone at least 0.1 m from every image (asserted).  Values are rounded to `dtype`, which is what a backend
    and the oracle both read."""
    rng = np.random.default_rng(seed)
    for _ in range(100):
        room = rng.uniform([3.0, 3.0, 2.4][:D], [6.0, 6.0, 3.5][:D], (B, D))
        source = 0.5 + rng.uniform(0, 1, (B, D)) * (room - 1.0)
        mic = 0.5 + rng.uniform(0, 1, (B, M, D)) * (room[:, None] - 1.0)
        ab = rng.uniform(0.05, 0.6, (B, 2 * D))
        room, source, mic, ab = (t.astype(dtype) for t in (room, source, mic, ab))
        near = min(O.geometry(room[b], source[b], mic[b], max_order, ab[b], FS, C)[0].min() for b in range(B))
        if near >= 0.1:
            return room, source, mic, ab
    raise AssertionError("no draw keeps the microphones 0.1 m from the images")


@functools.lru_cache(maxsize=None)
def case(name: str, dt: str):
    """(inputs, float64 oracle, the yardstick one precision up, the bar) of a shape in a dtype.
    float32: the yardstick is the oracle in float64, the bar 1 x the distance of the oracle's own float32 evaluation from it.
    float64: the yardstick is the oracle in longdouble, the bar 4 x the distance of the float64 oracle from it."""
    D, N, M, B, L, fl = SHAPES[name]
    dtype = DTYPES[dt]
    seed = sorted(SHAPES).index(name) * 2 + (dt == "f64")
    room, source, mic, ab = rooms(seed, B, M, D, dtype, N)

    def oracle(t):
        return np.stack([O.gather(room[b], source[b], mic[b], N, ab[b], L, FS, C, fl, dtype=t) for b in range(B)])

    o64 = oracle(np.float64)
    if dt == "f32":
        yard, bar = o64, float(np.abs(oracle(np.float32).astype(np.float64) - o64).max())
    else:
        yard = oracle(O.LD)
        bar = 4.0 * float(np.abs(o64.astype(O.LD) - yard).max())
    for t in (room, source, mic, ab, o64, yard):
        t.setflags(write=False)
    return (room, source, mic, ab, N, L, fl), o64, yard, bar


def run_case(backend, name: str, dt: str):
    (room, source, mic, ab, N, L, fl), _, _, _ = case(name, dt)
    return backend.run(room, source, mic, N, ab, L, fl)


def check_accuracy(backend, name: str, dt: str) -> float:
    (room, source, mic, ab, N, L, fl), o64, yard, bar = case(name, dt)
    out = backend.run(room, source, mic, N, ab, L, fl)
    assert out.shape == o64.shape and out.dtype == DTYPES[dt]
    assert np.isfinite(out).all()
    err = float(np.abs(out.astype(O.LD) - yard.astype(O.LD)).max())
    peak = float(np.abs(o64).max())
    print(f"rir {name} {dt}: err {err:.3e} bar {bar:.3e} ratio {err / bar if bar else float(err != 0):.3f} peak {peak:.3e}")
    if "len1" in name or "before_direct_path" in name:
        assert peak == 0.0 and not out.any()                     # shorter than the direct path's delay: all zeros
    else:
        assert peak > 1e-3                                       # the case does have a response in it
    assert err <= bar, (name, dt, err, bar)
    return err / bar if bar else 0.0


def check_single_image(backend, dt: str):
    """max_order = 0: one image, g(n - pad - tau) / dist from the closed form."""
    (room, source, mic, ab, N, L, fl), _, yard, bar = case("n0_m1_b1_tile-1", dt)
    assert N == 0
    up = np.float64 if dt == "f32" else O.LD
    r, s, m = (t[0].astype(up) for t in (room, source, mic))
    dist = np.sqrt(((s - m[0]) ** 2).sum())
    tau = dist * up(FS) / up(C)
    want = O.g(np.arange(L).astype(up) - up(fl // 2) - tau, fl // 2, up) / dist
    # the closed form adds the squares in another order: tau may move by a few ulp, and |g'| < 1.5
    slack = float((8 * np.finfo(up).eps * tau * 1.5 + 16 * np.finfo(up).eps) / dist)
    assert np.abs(want - yard[0, 0]).max() <= slack              # the oracle is the closed form
    out = backend.run(room, source, mic, N, ab, L, fl)
    assert np.abs(out[0, 0].astype(up) - want).max() <= bar + slack


def check_reproducible(backend, name: str = "n6_377img_m3_b1_2tile+3", dt: str = "f32"):
    a, b = run_case(backend, name, dt), run_case(backend, name, dt)
    assert a.tobytes() == b.tobytes()


def check_prefix(backend, dt: str):
    """The first L1 samples of a longer call are the shorter call, bit for bit, across a tile boundary."""
    (room, source, mic, ab, N, L2, fl), _, _, _ = case("n6_377img_m3_b1_2tile+3", dt)
    long = backend.run(room, source, mic, N, ab, L2, fl)
    for L1 in (1, TILE - 1, TILE, TILE + 1):
        short = backend.run(room, source, mic, N, ab, L1, fl)
        assert short.tobytes() == np.ascontiguousarray(long[:, :, :L1]).tobytes(), L1


def check_rows_are_rooms(backend, dt: str):
    """Row b of a batch call is the single-room call on room b, bit for bit."""
    for name in ("n3_m3_b5_tile+1", "d2_n2_m3_b5_2tile+3"):
        (room, source, mic, ab, N, L, fl), _, _, _ = case(name, dt)
        full = backend.run(room, source, mic, N, ab, L, fl)
        rows = [backend.run(room[b:b + 1], source[b:b + 1], mic[b:b + 1], N, ab[b:b + 1], L, fl)[0] for b in range(room.shape[0])]
        assert np.stack(rows).tobytes() == full.tobytes()
        assert len({r.tobytes() for r in rows}) == len(rows)     # the rooms do differ
        one_mic = backend.run(room, source, mic[:, 1:2], N, ab, L, fl)
        assert one_mic.tobytes() == np.ascontiguousarray(full[:, 1:2]).tobytes()


def check_poison(backend, dt: str):
    """A microphone exactly on the source: that (room, microphone) row is NaN throughout, every other row keeps its bits."""
    (room, source, mic, ab, N, L, fl), _, _, _ = case("n3_m3_b5_tile+1", dt)
    clean = backend.run(room, source, mic, N, ab, L, fl)
    mic2 = mic.copy()
    mic2[2, 1] = source[2]
    out = backend.run(room, source, mic2, N, ab, L, fl)
    assert np.isnan(out[2, 1]).all()
    keep = np.ones(out.shape[:2], bool)
    keep[2, 1] = False
    assert np.isfinite(out[keep]).all() and out[keep].tobytes() == clean[keep].tobytes()
    ab2 = ab.copy()
    ab2[4, 3] = 1.5                                              # an absorption above 1: every microphone of that room
    out = backend.run(room, source, mic, N, ab2, L, fl)
    assert np.isnan(out[4]).all() and out[:4].tobytes() == clean[:4].tobytes()
