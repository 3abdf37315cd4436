#!/usr/bin/env python
"""Device time of F.detect_pitch_frequency (defaults: frame_time 10 ms, win_length 30, 85 .. 3400 Hz, float32) beside the
reference restated in plain torch on the same device: 256 x 10 s at 16 kHz (the BASELINE batch) and 8 x 10 s at 44.1 kHz.

Each case rotates over enough input buffers that together they exceed twice the 256 MiB Infinity Cache.  Time = device
events around `--iters` calls after `--warmup`, divided by the calls.  FLOP = 2 x rows x frames x lags x frame_size (the
numerator FMAs; energies, picks and the median are not counted); the fraction is of the 157.3 TFLOP/s FP32 vector peak.

Restatement (labelled as such; torchaudio is not needed): tests/pitch_oracle.py's torch_reference, the reference's
lag loop of unfolds, products, sums and vector norms, then max, combine and median, timed on `--ref-batch` rows and
scaled linearly to the full batch."""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import audio_amd.functional as F  # noqa: E402
from pitch_oracle import torch_reference  # noqa: E402

PEAK_FP32 = 157.3e12
MALL = 256 << 20


def timed(fn, bufs, iters, warmup):
    for i in range(warmup):
        fn(bufs[i % len(bufs)])
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(iters):
        fn(bufs[i % len(bufs)])
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters          # us per call


def rotation(make, nbytes):
    n = max(2, -(-2 * MALL // nbytes) + 1)          # > 2 x the Infinity Cache in total
    return [make() for _ in range(n)]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ref-batch", type=int, default=8)
    ap.add_argument("--json", default=None, help="also write the results here")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_pitch measures the device: no GPU, no number"
    dev = torch.device("cuda")
    rows_out = []
    for rows, sr in ((256, 16000), (8, 44100)):
        L = 10 * sr
        lags, fs, frames = F._pitch_sizes(L, sr, 1e-2, 85)
        nbytes = rows * L * 4
        bufs = rotation(lambda: torch.randn(rows, L, device=dev) * 0.1, nbytes)
        us = timed(lambda x: F.detect_pitch_frequency(x, sr), bufs, a.iters, a.warmup)
        rb = min(a.ref_batch, rows)
        small = [x[:rb] for x in bufs[:2]]
        ref = timed(lambda x: torch_reference(x, sr), small, 2, 1) * (rows / rb)
        flop = 2.0 * rows * frames * lags * fs
        frac = flop / (us * 1e-6) / PEAK_FP32
        r = {"case": f"{rows} x 10 s @ {sr} Hz", "us": round(us, 1), "gflop": round(flop / 1e9, 2),
             "tflops": round(flop / (us * 1e-6) / 1e12, 1), "frac_fp32_peak": round(frac, 3),
             "restated_reference": f"torch_reference on {rb} rows, x{rows / rb:g}", "restated_us": round(ref, 1),
             "speedup": round(ref / us, 1)}
        rows_out.append(r)
        print(f"{r['case']:24s} {us:9.1f} us  {r['tflops']:6.1f} TFLOP/s = {frac:5.3f} of FP32 peak  "
              f"| restated reference: {ref:11.1f} us ({ref / us:7.1f} x)", flush=True)
        del bufs, small
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows_out, f, indent=1)


if __name__ == "__main__":
    main()
