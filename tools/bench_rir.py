#!/usr/bin/env python
"""Device time of F.simulate_rir_ism_batch on 256 rooms x 4 microphones at order 17 (7175 images) with 8192 samples, and on
1 room x 8 microphones at order 10 (1561 images) with 4096 samples, float32, beside the definition restated in plain torch
on the same device.

The restatement is the reference's scatter form: the image lattice, the per-image delays and amplitudes, an (images, fl)
block of taps per microphone and one index_add_ into the response, in float32 as the reference computes float32 inputs.  Its
(rooms, images, microphones, fl) temporaries do not fit for 256 rooms, so it is timed on the first `--ref-rooms` rooms of the
same batch and scaled to all rooms; the line says so.  Both are measured by one protocol in alternating rounds: device events
around `--iters` calls after `--warmup`, divided by the calls, rotating over `--sets` draws of rooms; median and minimum of
`--rounds` such measurements.  Beside them: the number of filter taps laid down (rooms x microphones x images x fl, less
what falls beyond the output) and the time per tap.

Restatement (labelled as such; torchaudio is not needed and the code under test is not used by it)."""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import audio_amd.functional as F  # noqa: E402
from audio_amd import _host  # noqa: E402


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


def draw(B, M, seed, dev):
    g = torch.Generator().manual_seed(seed)
    room = torch.tensor([4.0, 5.0, 2.8]) + torch.rand(B, 3, generator=g) * torch.tensor([4.0, 4.0, 1.0])
    source = 0.5 + torch.rand(B, 3, generator=g) * (room - 1.0)
    mic = 0.5 + torch.rand(B, M, 3, generator=g) * (room[:, None] - 1.0)
    ab = 0.1 + 0.5 * torch.rand(B, 6, generator=g)
    return tuple(t.to(dev) for t in (room, source, mic, ab))


def restated(room, source, mic, ab, lattice, L, fl=81, fs=16000.0, c=343.0):
    """The reference's scatter form for (B, ...) inputs: (B, M, L)."""
    B, M, _ = mic.shape
    pad = fl // 2
    v = lattice.to(room.dtype)                                                       # (I, 3)
    odd = (lattice % 2 == 1)
    loc = torch.where(odd, room[:, None] * (v + 1) - source[:, None], room[:, None] * v + source[:, None])      # (B, I, 3)
    tr = torch.sqrt(1 - ab)
    lo, hi = torch.div(lattice, 2, rounding_mode="floor").abs(), torch.div(lattice + 1, 2, rounding_mode="floor").abs()
    att = (tr[:, None, 0::2] ** lo * tr[:, None, 1::2] ** hi).prod(-1)               # (B, I)
    dist = torch.linalg.norm(loc[:, :, None] - mic[:, None], dim=-1)                 # (B, I, M)
    amp = att[:, :, None] / dist
    tau = dist * fs / c
    first = torch.ceil(tau)
    k = torch.arange(fl, device=room.device, dtype=room.dtype)
    t = k + (first - tau)[..., None]                                                 # (B, I, M, fl)
    taps = amp[..., None] * torch.sinc(t - pad) * torch.where(t <= fl - 1, 0.5 - 0.5 * torch.cos(2 * math.pi * t / (fl - 1)), 0.0)
    idx = first.long()[..., None] + torch.arange(fl, device=room.device)
    keep = idx < L
    rows = (torch.arange(B, device=room.device)[:, None, None, None] * M + torch.arange(M, device=room.device)[None, None, :, None])
    flat = torch.where(keep, rows * L + idx, 0)
    out = torch.zeros(B * M * L, device=room.device, dtype=room.dtype)
    out.index_add_(0, flat.reshape(-1), torch.where(keep, taps, 0.0).reshape(-1))
    return out.view(B, M, L)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--ref-rooms", type=int, default=4)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sets", type=int, default=3)
    ap.add_argument("--json", default=None, help="also write the results here")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_rir measures the device: no GPU, no number"
    dev = torch.device("cuda")
    rows_out = []
    for B, M, N, L in ((256, 4, 17, 8192), (1, 8, 10, 4096)):
        fl = 81
        sets = [draw(B, M, 100 + i, dev) for i in range(a.sets)]
        nref = min(B, a.ref_rooms)
        short = [tuple(t[:nref].contiguous() for t in s) for s in sets]
        lattice = torch.from_numpy(_host.rir_lattice(N, 3).astype(np.int64)).to(dev)
        ours = lambda s: F.simulate_rir_ism_batch(s[0], s[1], s[2], N, s[3], L)                      # noqa: E731
        ref = lambda s: restated(s[0], s[1], s[2], s[3], lattice, L, fl)                             # noqa: E731
        worst = (ours(short[0]) - ref(short[0])).abs().max().item()          # the two do compute the same thing
        t_ours, t_ref = [], []
        for _ in range(a.rounds):                                            # alternating
            t_ours.append(timed(ours, sets, a.iters, a.warmup))
            t_ref.append(timed(ref, short, a.iters, a.warmup))
        r, s_, m, _ = sets[0]
        far = torch.tensor(_host.rir_lattice(N, 3).astype(np.float32)).abs().sum(1).max().item()
        taps = 0
        with torch.no_grad():                                                # taps inside the output, counted on the first set
            v = lattice.to(r.dtype)
            loc = torch.where(lattice % 2 == 1, r[:, None] * (v + 1) - s_[:, None], r[:, None] * v + s_[:, None])
            tau = torch.linalg.norm(loc[:, :, None] - m[:, None], dim=-1) * 16000.0 / 343.0
            taps = int((torch.clamp(L - torch.ceil(tau), 0, fl)).sum().item())
        scale = B / nref
        row = {"case": "simulate_rir_ism_batch", "rooms": B, "mics": M, "max_order": N, "images": int(lattice.shape[0]),
               "output_length": L, "delay_filter_length": fl, "us_median": statistics.median(t_ours), "us_min": min(t_ours),
               "taps_inside_output": taps, "ps_per_tap": statistics.median(t_ours) * 1e6 / max(taps, 1),
               "restated_us_median_scaled": statistics.median(t_ref) * scale, "restated_us_min_scaled": min(t_ref) * scale,
               "restated_rooms": nref, "max_abs_difference_float32": worst, "largest_image_order": far}
        rows_out.append(row)
        print("simulate_rir_ism_batch %d rooms x %d mics, order %d (%d images), %d samples: %10.1f us (min %10.1f); %.3g taps inside "
              "the output, %.2f ps per tap; restated in torch on %d rooms, scaled: %.0f us (x%.0f); max |difference| %.2e" %
              (B, M, N, lattice.shape[0], L, row["us_median"], row["us_min"], taps, row["ps_per_tap"], nref,
               row["restated_us_median_scaled"], row["restated_us_median_scaled"] / row["us_median"], worst))
        del sets, short
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows_out, f, indent=1)


if __name__ == "__main__":
    main()
