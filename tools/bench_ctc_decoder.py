#!/usr/bin/env python
"""Device time of audio_amd.models.decoder.ctc_beam_search at beam 10 on (32, 1500, 32), (32, 1500, 1024) and (8, 1500, 5000)
float32 emissions, with blank_skip_threshold = log 0.95 and 0 (nothing skipped).

Emissions: log_softmax of seeded normals times 3, with blank boosted on `--blank-share` of the frames (default 0.6: a trained
CTC model emits blank on most frames), so that log 0.95 skips about that share and 0 skips none.

Time = device events around `--iters` calls after `--warmup`, divided by the calls; `--rounds` such measurements per case,
median and minimum reported, and the time per unskipped frame of one example beside them (the beam pass walks the unskipped
frames of an example in order; the examples run side by side).  The two kernels' own durations come from one profiled call
(torch.profiler, device activity): the row pass is the only full read of the B T V 4 bytes, and its share of the 8 TB/s
HBM roofline is reported; null where the profiler gives no device events.  Nothing is compared: the reference's decoder
is CUDA-only."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from audio_amd.models.decoder import ctc_beam_search  # noqa: E402

HBM_BYTES_PER_S = 8e12


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


def kernel_times(fn):
    """{"row": us, "beam": us} of one call, or {} when the profiler records no device activity."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        out = {}
        for ev in prof.key_averages():
            t = getattr(ev, "device_time_total", None)
            if t is None:
                t = getattr(ev, "cuda_time_total", 0.0)
            for which in ("row", "beam"):
                if "cd" in ev.key and which + "_kernel" in ev.key:
                    out[which] = out.get(which, 0.0) + float(t) / max(ev.count, 1)
        return out
    except Exception as e:                          # a profiler that cannot start is no reason to lose the timings
        print("bench_ctc_decoder: no kernel durations (%s)" % e, file=sys.stderr)
        return {}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", type=int, nargs=3, action="append", metavar=("B", "T", "V"))
    ap.add_argument("--beam", type=int, default=10)
    ap.add_argument("--blank-share", type=float, default=0.6)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_ctc_decoder: no GPU; a timing from a CPU says nothing about these kernels")
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    for B, T, V in args.shapes or [(32, 1500, 32), (32, 1500, 1024), (8, 1500, 5000)]:
        x = torch.randn(B, T, V, device=dev, generator=g) * 3.0
        boost = torch.rand(B, T, device=dev, generator=g) < args.blank_share
        x[..., 0] += boost * (18.0 + math.log(V))
        lp = torch.log_softmax(x, -1)
        del x
        for label, thr in (("log0.95", math.log(0.95)), ("0", 0.0)):
            def ours():
                return ctc_beam_search(lp, None, args.beam, 1, 0, thr)

            tokens, lens, scores = ours()
            unskipped = int((lp[..., 0] <= thr).sum(1).max())          # the longest walk of the beam pass
            assert int(lens.min()) >= 0 and bool(torch.isfinite(scores).all())
            ts = [timed(ours, args.iters, args.warmup) for _ in range(args.rounds)]
            k = kernel_times(ours)
            line = {"case": "ctc_beam_search", "shape": [B, T, V], "dtype": "float32", "beam": args.beam, "threshold": label,
                    "blank_share": args.blank_share, "unskipped_frames_max": unskipped,
                    "mean_tokens": float(lens.double().mean()),
                    "us_median": statistics.median(ts), "us_min": min(ts),
                    "us_per_unskipped_frame_of_one_example": statistics.median(ts) / max(unskipped, 1),
                    "row_kernel_us": k.get("row"), "beam_kernel_us": k.get("beam"),
                    "row_pass_fraction_of_8TBps": (B * T * V * 4 / HBM_BYTES_PER_S * 1e6 / k["row"]) if k.get("row") else None}
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
