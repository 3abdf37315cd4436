#!/usr/bin/env python
"""Device time of F.forced_align on a ragged-free batch of utterances (32 x 1500 frames x 32 classes, 200 labels) and on one
long recording (1 x 30000 x 32, 2000 labels), beside the reference's algorithm restated in plain torch on the same device.

Time = device events around `--iters` calls after `--warmup`, divided by the calls; `--rounds` such measurements per case,
kernel and restatement alternating, median and minimum reported, and the time per step and example beside them.  The
restatement's time is wall clock around a synchronised call, since it ends on the host.

Restatement (labelled as such; torchaudio is not needed and the code under test is not used): what the reference's GPU path
does -- one step of the recurrence per iteration over all states of one example (a handful of element-wise launches where
the reference has one kernel), the (T, 2 L + 1) back-pointer matrix copied to the host, the walk back there, one example at a
time since the reference refuses a batch.  It accumulates in the dtype of the input."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import audio_amd.functional as F  # noqa: E402


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters          # us per call


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6


def ref_forced_align(log_probs, targets, blank):
    """Restatement of the reference's device path: (paths (B, T) int64 on the host, totals (B,))."""
    B, T, _ = log_probs.shape
    L = targets.shape[1]
    S = 2 * L + 1
    dev = log_probs.device
    ninf = torch.full((2,), float("-inf"), device=dev, dtype=log_probs.dtype)
    paths, totals = torch.zeros(B, T, dtype=torch.int64), []
    for b in range(B):
        label = torch.full((S,), blank, device=dev, dtype=torch.int64)
        label[1::2] = targets[b].long()
        skip = torch.zeros(S, device=dev, dtype=torch.bool)
        skip[3::2] = label[3::2] != label[1:-2:2]
        lp = log_probs[b][:, label]                 # (T, S): the gathers of every step
        alpha = torch.full((S,), float("-inf"), device=dev, dtype=log_probs.dtype)
        alpha[:2] = lp[0, :2]
        back = torch.zeros(T, S, device=dev, dtype=torch.int8)
        for t in range(1, T):                       # one step per iteration, as the reference launches one kernel per step
            x1 = torch.cat((ninf[:1], alpha[:-1]))
            x2 = torch.where(skip, torch.cat((ninf, alpha[:-2])), ninf[0])
            best, mv = torch.stack((alpha, x1, x2)).max(0)
            back[t] = mv
            alpha = best + lp[t]
        hb = back.cpu().numpy()                     # the back-pointer matrix goes to the host
        fin = alpha.cpu()
        s = S - 1 if S == 1 or fin[S - 1] > fin[S - 2] else S - 2
        totals.append(float(fin[s]))
        lab = label.cpu().numpy()
        for t in range(T - 1, -1, -1):              # and is walked there
            paths[b, t] = int(lab[s])
            s -= int(hb[t, s])
    return paths, totals


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", type=int, nargs=4, action="append", metavar=("B", "T", "C", "L"))
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-reference", action="store_true", help="skip the restated per-step algorithm (seconds per call)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_forced_align: no GPU; a timing from a CPU says nothing about these kernels")
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    for B, T, Cn, L in args.shapes or [(32, 1500, 32, 200), (1, 30000, 32, 2000)]:
        lp = torch.log_softmax(torch.randn(B, T, Cn, device=dev, generator=g) * 3.0, -1)
        targets = torch.randint(1, Cn, (B, L), device=dev, generator=g, dtype=torch.int32)

        def ours():
            return F.forced_align(lp, targets)

        def ref():
            return ref_forced_align(lp, targets, 0)

        paths, scores = ours()
        line = {"case": "forced_align", "shape": [B, T, Cn, L], "dtype": "float32"}
        if not args.no_reference:                   # the two reach the same totals before either is timed
            want = ref()[1]
            got = scores.double().sum(1).cpu().tolist()
            assert all(abs(a - b) <= 1e-4 * abs(b) for a, b in zip(got, want)), (got, want)
        t_ours, t_ref = [], []
        for _ in range(args.rounds):
            t_ours.append(timed(ours, args.iters, args.warmup))
            if not args.no_reference:
                t_ref.append(wall(ref))
        line.update({"us_median": statistics.median(t_ours), "us_min": min(t_ours),
                     "ns_per_step_per_example": statistics.median(t_ours) * 1e3 / (B * T)})
        if t_ref:
            line.update({"restated_reference_us_median": statistics.median(t_ref),
                         "restated_reference_ns_per_step_per_example": statistics.median(t_ref) * 1e3 / (B * T),
                         "speedup_vs_restated_reference": statistics.median(t_ref) / statistics.median(t_ours)})
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
