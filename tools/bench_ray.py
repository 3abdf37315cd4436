#!/usr/bin/env python
"""Device time of F.ray_tracing_batch on 256 rooms x 4 microphones x 10 000 rays, one band, time_thres 1.0 s, with scattering 0
and 0.2, and on 1 room x 8 microphones x 100 000 rays x 7 bands, float32, beside the definition restated in plain torch on the
same device.

The restatement steps all rays of all rooms in lockstep under masks, in float64 as the definition is, and adds every
contribution with index_add_ into a float64 histogram; it asks the device every 16 bounces whether a ray is still alive.  For
256 rooms it is timed on the first `--ref-rooms` rooms of the same batch and scaled to all rooms; the line says so.  Both are
measured by one protocol in alternating rounds: device events around `--iters` calls after `--warmup`, divided by the calls,
rotating over `--sets` draws of rooms; median and minimum of `--rounds` such measurements.  Beside them: the number of
contributions (counted by the restatement, scaled the same way), hence the bytes of 64-bit integer atomics per second of
the kernel, to set against the chip-wide atomic rate.

Restatement (labelled as such; torchaudio is not needed and the code under test is not used by it)."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import audio_amd.functional as F  # noqa: E402

C = 343.0
GOLDEN = math.pi * (3.0 - math.sqrt(5.0))


def timed(fn, sets, iters, warmup):
    for i in range(warmup):
        fn(sets[i % len(sets)])
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(iters):
        fn(sets[i % len(sets)])
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters          # us per call


def draw(B, M, NB, scattering, seed, dev):
    g = torch.Generator().manual_seed(seed)
    room = torch.tensor([4.0, 5.0, 2.8]) + torch.rand(B, 3, generator=g) * torch.tensor([4.0, 4.0, 1.0])
    source = room * (0.2 + 0.6 * torch.rand(B, 3, generator=g))
    mic = room[:, None] * (0.2 + 0.6 * torch.rand(B, M, 3, generator=g))
    ab = 0.1 + 0.4 * torch.rand(B, NB, 6, generator=g)
    sc = torch.full((B, NB, 6), float(scattering))
    return tuple(t.to(dev) for t in (room, source, mic, ab, sc))


def restated(room, source, mic, ab, sc, N, R, ethr, tt, hb, bounces):
    """All rays of all rooms in lockstep under masks: ((B, M, NB, bins) float64, contributions)."""
    dt = torch.float64
    room, source, mic, ab, sc = (t.to(dt) for t in (room, source, mic, ab, sc))
    dev = room.device
    (B, M, D), NB = mic.shape, ab.shape[1]
    bins, e0, s_max, r2, w_bin = int(math.ceil(tt / hb)), 2.0 / N, tt * C, R * R, C * hb
    i = torch.arange(N, device=dev, dtype=dt)
    z = 1.0 - (2.0 * i + 1.0) / N
    rho, phi = torch.sqrt(1.0 - z * z), i * GOLDEN
    dirs = torch.stack([rho * torch.cos(phi), rho * torch.sin(phi), z], -1)[None].expand(B, N, D).clone()
    p = source[:, None].expand(B, N, D).clone()
    tr = torch.full((B, N, NB), e0, device=dev, dtype=dt)
    travel = torch.zeros(B, N, device=dev, dtype=dt)
    alive = torch.ones(B, N, device=dev, dtype=torch.bool)
    hist = torch.zeros(B * M * NB * bins, device=dev, dtype=dt)
    count = torch.zeros((), device=dev, dtype=torch.int64)
    rows = torch.arange(B, device=dev)[:, None, None] * M                                     # (B, 1, 1)
    bands = torch.arange(NB, device=dev)[None, None]
    walls = room[:, None].expand(B, N, D)
    abw, scw_all = ab.transpose(1, 2), sc.transpose(1, 2)                                     # (B, 2 D, NB)
    scatters = bool((sc > 0).any().item())
    inf = torch.tensor(math.inf, device=dev, dtype=dt)

    def deposit(mask, m, d, num):
        nonlocal count
        x = torch.floor(d / w_bin)
        ok = mask & (x >= 0) & (x < bins)
        rr = torch.clamp(d * d, min=r2)
        e = num / (rr * (1.0 - torch.sqrt(1.0 - r2 / rr)))[..., None]
        idx = ((rows + m) * NB + bands) * bins + x.clamp(0, bins - 1).long()[..., None]
        hist.index_add_(0, idx.reshape(-1), torch.where(ok[..., None], e, 0.0).reshape(-1))
        count = count + ok.sum() * NB

    for k in range(bounces):
        td = torch.where(dirs > 0, (walls - p) / dirs, torch.where(dirs < 0, p / (-dirs), inf))
        t, axis = td.min(-1)
        ax = axis[..., None]
        up = dirs.gather(-1, ax).squeeze(-1) > 0
        w = (2 * axis + up)[..., None].expand(B, N, NB)
        for m in range(M):
            v = mic[:, m, None] - p
            u = (v * dirs).sum(-1)
            q = (v * v).sum(-1) - u * u
            deposit(alive & (u >= 0) & (u <= t) & (q < r2), m, travel + u, tr)
        travel = travel + t
        p = (p + t[..., None] * dirs).scatter(-1, ax, torch.where(up, walls.gather(-1, ax).squeeze(-1), 0.0)[..., None])
        tr = tr * (1.0 - abw.gather(1, w))
        scw = scw_all.gather(1, w)
        if scatters:
            some = alive & (scw > 0).any(-1)
            for m in range(M):
                v = mic[:, m, None] - p
                h2 = (v * v).sum(-1)
                h = torch.sqrt(h2)
                p_eq = 1.0 - torch.sqrt(1.0 - r2 / torch.clamp(h2, min=r2))
                st = (2.0 * (v.gather(-1, ax).squeeze(-1).abs() / h) * p_eq)[..., None] * tr * scw
                d = travel + h
                deposit(some & (d < s_max) & (st.max(-1).values > ethr), m, d, st)
        tr = tr * (1.0 - scw)
        alive = alive & ~((travel > s_max) | (tr.max(-1).values < ethr))
        dirs = dirs.scatter(-1, ax, -dirs.gather(-1, ax))
        if k % 16 == 15 and not bool(alive.any().item()):
            break
    return hist.view(B, M, NB, bins), count


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--ref-rooms", type=int, default=8)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sets", type=int, default=2)
    ap.add_argument("--json", default=None, help="also write the results here")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_ray measures the device: no GPU, no number"
    dev = torch.device("cuda")
    R, ethr, tt, hb = 0.5, 1e-7, 1.0, 0.004
    rows_out = []
    for B, M, N, NB, scattering in ((256, 4, 10000, 1, 0.0), (256, 4, 10000, 1, 0.2), (1, 8, 100000, 7, 0.1)):
        sets = [draw(B, M, NB, scattering, 100 + i, dev) for i in range(a.sets)]
        nref = min(B, a.ref_rooms)
        short = [tuple(t[:nref].contiguous() for t in s) for s in sets]
        bound = int(max((torch.floor(tt * C / s[0].double()) + 2).sum(-1).max().item() for s in sets))
        ours = lambda s: F.ray_tracing_batch(s[0], s[1], s[2], N, s[3], s[4], R, C, ethr, tt, hb)          # noqa: E731
        ref = lambda s: restated(s[0], s[1], s[2], s[3], s[4], N, R, ethr, tt, hb, bound)                  # noqa: E731
        want, count = ref(short[0])
        got = ours(short[0]).double()
        worst = ((got - want).abs().max() / want.abs().max()).item()         # the two do compute the same thing
        t_ours, t_ref = [], []
        for _ in range(a.rounds):                                            # alternating
            t_ours.append(timed(ours, sets, a.iters, a.warmup))
            t_ref.append(timed(ref, short, 1, 0))
        scale = B / nref
        adds = int(count.item()) * scale
        us = statistics.median(t_ours)
        row = {"case": "ray_tracing_batch", "rooms": B, "mics": M, "rays": N, "bands": NB, "scattering": scattering,
               "time_thres": tt, "bins": int(math.ceil(tt / hb)), "bounce_bound": bound, "us_median": us, "us_min": min(t_ours),
               "contributions_scaled": adds, "atomic_bytes": adds * 8, "atomic_GB_per_s": adds * 8 / us * 1e-3,
               "chip_wide_float_atomic_GB_per_s": 1300.0,
               "restated_us_median_scaled": statistics.median(t_ref) * scale, "restated_us_min_scaled": min(t_ref) * scale,
               "restated_rooms": nref, "max_difference_over_peak_float32": worst}
        rows_out.append(row)
        print("ray_tracing_batch %d rooms x %d mics x %d rays x %d bands, scattering %.1f: %10.1f us (min %10.1f); %.3g 8-byte atomic "
              "adds, %.1f GB/s of them; restated in torch on %d rooms, scaled: %.0f us (x%.1f); max |difference| / peak %.2e" %
              (B, M, N, NB, scattering, us, row["us_min"], adds, row["atomic_GB_per_s"], nref, row["restated_us_median_scaled"],
               row["restated_us_median_scaled"] / us, worst), flush=True)
        del sets, short
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows_out, f, indent=1)


if __name__ == "__main__":
    main()
