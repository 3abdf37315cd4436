#!/usr/bin/env python
"""Device time of F.inverse_mel_scale (csrc/inverse_mel.h) at two shapes, float32, in both input layouts, beside
relu(matmul(P, x)) restated in plain torch on the same device:

    (256, 80, 1001) -> 201   the ASR front-end's batch, the default filterbank (rank 75)
    (32, 80, 800)   -> 513   the Tacotron2 Griffin-Lim bundle's filterbank (slaney / slaney, 22 050 Hz, f_max 8000)

Each case rotates over enough input buffers that together they exceed twice the 256 MiB Infinity Cache, so every call
streams its input from HBM.  Both sides are timed by ONE protocol: `--rounds` alternating rounds (kernel, composition,
kernel, ...), each round device events around `--iters` calls after `--warmup` calls, divided by the calls; the figure is
the median over the rounds, and the rounds' extremes are kept in the JSON.  The kernel
is compute-bound: FLOP = 2 * frames * n_stft * n_mels against the 157.3 TFLOP/s float32 matrix peak (52 us for the first
shape); bytes = input + output, each once, against 8 TB/s (36 us)."""
import argparse
import json
import os
import statistics
import sys
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import audio_amd.functional as F  # noqa: E402

PEAK_FLOPS = 157.3e12
PEAK_BYTES = 8.0e12
MALL = 256 << 20
CASES = [("asr", 256, 80, 1001, 201, dict(f_max=8000.0, sample_rate=16000, norm=None, mel_scale="htk")),
         ("taco", 32, 80, 800, 513, dict(f_max=8000.0, sample_rate=22050, norm="slaney", mel_scale="slaney"))]


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
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None, help="also write the results here")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_inverse_mel measures the device: no GPU, no number"
    dev = torch.device("cuda")
    rows = []
    for name, B, K, Tn, n_stft, fbk in CASES:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            fb = F.melscale_fbanks(n_stft, 0.0, fbk["f_max"], K, fbk["sample_rate"], fbk["norm"], fbk["mel_scale"]).to(dev)
        P = F._inverse_mel_matrix(fb, dev)
        flop = 2.0 * B * Tn * n_stft * K
        nbytes_in, nbytes = B * K * Tn * 4, B * Tn * (K + n_stft) * 4
        for layout in ("time-major", "frame-major"):
            if layout == "time-major":
                bufs = rotation(lambda: torch.rand(B, K, Tn, device=dev), nbytes_in)
            else:
                bufs = rotation(lambda: torch.rand(B, Tn, K, device=dev).transpose(1, 2), nbytes_in)
            ours, theirs = [], []
            for _ in range(a.rounds):
                ours.append(timed(lambda x: F.inverse_mel_scale(x, fb), bufs, a.iters, a.warmup))
                theirs.append(timed(lambda x: torch.relu(torch.matmul(P, x)), bufs, a.iters, a.warmup))
            us, ref = statistics.median(ours), statistics.median(theirs)
            got, want = F.inverse_mel_scale(bufs[0], fb), torch.relu(torch.matmul(P, bufs[0]))
            r = {"case": f"{name} ({B},{K},{Tn})->{n_stft} {layout}", "us": round(us, 2),
                 "frac_fp32_matrix_peak": round(flop / (us * 1e-6) / PEAK_FLOPS, 3),
                 "floor_compute_us": round(flop / PEAK_FLOPS * 1e6, 1), "floor_bytes_us": round(nbytes / PEAK_BYTES * 1e6, 1),
                 "restated_reference": "relu(matmul(P, x)) (restated)", "restated_us": round(ref, 1),
                 "speedup": round(ref / us, 2), "rounds_us": [round(min(ours), 2), round(max(ours), 2)],
                 "restated_rounds_us": [round(min(theirs), 1), round(max(theirs), 1)], "max_abs_diff_vs_restated": float((got - want).abs().max())}
            rows.append(r)
            print(f"{r['case']:44s} {us:9.2f} us  {r['frac_fp32_matrix_peak']:5.3f} of the fp32 matrix peak "
                  f"(floors {r['floor_compute_us']} / {r['floor_bytes_us']} us)   | relu(matmul) restated: {ref:9.1f} us "
                  f"({ref / us:5.2f} x)", flush=True)
            del bufs
            torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
