#!/usr/bin/env python
"""Device time of the SpecAugment masking kernel at the ASR front-end's shape ((256, 80, 1001) float32, frame-major as
MelSpectrogram returns it), beside a plain device copy of the same tensor and the reference's composition restated in torch.

  (a) the kernel alone (F._spec_augment_apply with fixed draws) for 1, 2+2 and 10+2 masks
  (b) a plain device copy of the same tensor (clone), in the same run: the kernel moves the same bytes or fewer
  (c) the whole T.SpecAugment(2, 100, 2, 27) call, draws and mean included
  (d) the restated reference (tests/spec_augment_oracle.py, torch_reference_spec_augment) on the same device

Inputs rotate over more than twice the 256 MiB Infinity Cache, so every call streams from HBM, and the variants are
interleaved: `--rounds` rounds, each timing every variant once (device events around `--iters` calls).  Reported per
variant: the median round, the spread (min .. max over the rounds), and the fraction of 8 TB/s on input + output bytes."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import audio_amd.functional as F  # noqa: E402
import audio_amd.transforms as T  # noqa: E402
import spec_augment_oracle as O  # noqa: E402

PEAK = 8.0e12
MALL = 256 << 20


def timed(fn, bufs, iters, start):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(iters):
        fn(bufs[(start + i) % len(bufs)])
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters          # us per call


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--json", default=None, help="also write the results here")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_spec_augment measures the device: no GPU, no number"
    dev = torch.device("cuda")
    B, Fm, Tn = a.batch, 80, 1001
    nbytes = B * Fm * Tn * 4
    n_bufs = max(2, -(-2 * MALL // nbytes) + 1)      # > 2 x the Infinity Cache in total
    bufs = [torch.randn(B, Tn, Fm, device=dev).transpose(-1, -2) for _ in range(n_bufs)]
    assert bufs[0].shape == (B, Fm, Tn) and bufs[0].stride(-2) == 1

    def fixed(n_time, n_freq):
        plan = [(1, 100)] * n_time + [(0, 27)] * n_freq
        d = torch.rand(len(plan), 2, B, device=dev)
        return lambda x: F._spec_augment_apply(x, d, plan, 0.0)

    aug = T.SpecAugment(2, 100, 2, 27)
    variants = [("(a) kernel, 1 time mask", fixed(1, 0)), ("(a) kernel, 2+2 masks", fixed(2, 2)),
                ("(a) kernel, 10+2 masks", fixed(10, 2)), ("(b) clone", lambda x: x.clone()),
                ("(c) T.SpecAugment(2,100,2,27)", aug),
                ("(d) restated reference", lambda x: O.torch_reference_spec_augment(x, 2, 100, 2, 27))]
    for _, fn in variants:                           # warm-up: allocator, caches, first launches
        for i in range(3):
            fn(bufs[i % n_bufs])
    torch.cuda.synchronize()
    times = {name: [] for name, _ in variants}
    for r in range(a.rounds):
        for k, (name, fn) in enumerate(variants):
            times[name].append(timed(fn, bufs, a.iters, r * a.iters + k))
    rows = []
    for name, _ in variants:
        t = times[name]
        med = statistics.median(t)
        frac = 2 * nbytes / (med * 1e-6) / PEAK
        rows.append({"case": name, "us_median": round(med, 2), "us_min": round(min(t), 2), "us_max": round(max(t), 2),
                     "bytes": 2 * nbytes, "frac_8TBps": round(frac, 3)})
        print(f"{name:32s} {med:9.2f} us  (min {min(t):8.2f} .. max {max(t):8.2f} over {a.rounds} rounds)  "
              f"{2 * nbytes / 1e6:6.1f} MB  {frac:5.3f} of 8 TB/s", flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
