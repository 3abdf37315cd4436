#!/usr/bin/env python
"""Device time of F.ctc_loss (csrc/ctc_loss.h), forward and forward + backward, float32, reduction "mean", at

    (1500, 32, 32)     S = 200   characters, 30 s of 20 ms frames
    (1500, 32, 1024)   S = 300   word pieces
    (1500, 8, 5000)    S = 300   a large word-piece vocabulary

with ragged input lengths (T down to 0.7 T) and target lengths (S down to 0.7 S).  Beside it the composition a user had before:
torch.nn.functional.ctc_loss(torch.log_softmax(x, -1), ...) on the same device with the same autograd.  Both sides are timed by
ONE protocol: `--rounds` alternating rounds, each round device events around `--iters` calls after `--warmup` calls, over input
sets taken in rotation whose bytes exceed twice the Infinity Cache (256 MB); the figure is the median over the rounds, the
rounds' extremes and the allocator's peak above the inputs are kept in the JSON, with the bytes of logits (and of the gradient)
at 8 TB/s as the floor."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import audio_amd.functional as F  # noqa: E402
from bench_sdr import timed  # noqa: E402

CASES = [("chars", (1500, 32, 32), 200), ("pieces", (1500, 32, 1024), 300), ("pieces5k", (1500, 8, 5000), 300)]
HBM_BYTES_PER_S, CACHE_BYTES = 8e12, 256e6


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cases", default=",".join(c[0] for c in CASES))
    ap.add_argument("--json", default=None, help="also write the results here")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_ctc_loss measures the device: no GPU, no number"
    dev, rows = torch.device("cuda"), []
    for name, shape, S in CASES:
        if name not in a.cases.split(","):
            continue
        T_, N, V = shape
        g = torch.Generator(device=dev).manual_seed(0)
        in_bytes = T_ * N * V * 4
        n_sets = int(2 * CACHE_BYTES // in_bytes) + 2
        sets = [(torch.randn(shape, device=dev, generator=g).mul_(2).requires_grad_(),) for _ in range(n_sets)]
        plain = [(x.detach(),) for x, in sets]
        targets = torch.randint(1, V, (N, S), device=dev, generator=g)
        in_len = torch.linspace(T_, 0.7 * T_, N, device=dev).long()
        tg_len = torch.linspace(S, 0.7 * S, N, device=dev).long()
        ours_fn = lambda x: F.ctc_loss(x, targets, in_len, tg_len)  # noqa: E731
        ref_fn = lambda x: torch.nn.functional.ctc_loss(torch.log_softmax(x, -1), targets, in_len, tg_len)  # noqa: E731

        def with_backward(fn):
            def run(x):
                x.grad = None
                fn(x).backward()
            return run

        l0, l1 = float(ours_fn(plain[0][0])), float(ref_fn(plain[0][0]))
        assert abs(l0 - l1) <= 1e-4 * abs(l1), (name, l0, l1)
        for what, f_ours, f_ref, data, passes in (("forward", ours_fn, ref_fn, plain, 1),
                                                  ("forward+backward", with_backward(ours_fn), with_backward(ref_fn), sets, 3)):
            ours, theirs = [], []
            for _ in range(a.rounds):
                ours.append(timed(f_ours, data, a.iters, a.warmup))
                theirs.append(timed(f_ref, data, a.iters, a.warmup))
            us, ref_us = statistics.median(o[0] for o in ours), statistics.median(o[0] for o in theirs)
            floor = passes * in_bytes / HBM_BYTES_PER_S * 1e6
            r = {"case": f"ctc_loss mean {what} {name} {shape} S={S} float32", "us": round(us, 1),
                 "rounds_us": [round(min(o[0] for o in ours), 1), round(max(o[0] for o in ours), 1)],
                 "peak_MB": round(max(o[1] for o in ours), 1), "input_MB": round(in_bytes / 1e6, 1), "input_sets": n_sets,
                 "composition": "torch.nn.functional.ctc_loss(torch.log_softmax(x, -1), ...) on the same device",
                 "composition_us": round(ref_us, 1),
                 "composition_rounds_us": [round(min(o[0] for o in theirs), 1), round(max(o[0] for o in theirs), 1)],
                 "composition_peak_MB": round(max(o[1] for o in theirs), 1), "speedup": round(ref_us / us, 2),
                 f"floor_us_{passes}_passes_at_8TBps": round(floor, 1), "fraction_of_floor": round(floor / us, 3)}
            rows.append(r)
            print(json.dumps(r), flush=True)
        del sets, plain
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
