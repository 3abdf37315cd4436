#!/usr/bin/env python
"""Device time of F.vad_start on (256, 160000) float32 at 16 kHz (256 utterances of 10 s) and on (8, 441000) at 44.1 kHz,
beside the reference's loop over measurements and channels restated in plain torch on the same device.

The restated loop runs some two dozen small tensor operations and one host read-back per measurement and channel, so it is
timed on the first `--ref-rows` rows and `--ref-frames` measurements of the same batch and scaled to all rows and frames; the
line says so.  Each case rotates over enough inputs that together they exceed twice the 256 MiB Infinity Cache.  Time =
device events around `--iters` calls after `--warmup`, divided by the calls; `--rounds` such measurements per case, median
and minimum reported.  The share of each launch comes from a separate profiled run (torch.profiler, device activity), not
from the timed one.  The floor each case is set against is one read of the waveform at 8 TB/s.

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

MALL = 256 << 20
HBM_BYTES_PER_US = 8e6          # 8 TB/s


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


def ref_vad_measurements(x, sr, frames, measure_freq=20.0, boot_time=0.35, noise_up_time=0.1, noise_down_time=0.01,
                         noise_reduction_amount=1.35, measure_smooth_time=0.4, hp_filter_freq=50.0, lp_filter_freq=6000.0,
                         hp_lifter_freq=150.0, lp_lifter_freq=2000.0, trigger_level=7.0, trigger_time=0.25):
    """Restatement of the reference's loop (functional/filtering.py vad and _measure) over the first `frames` measurements of
    every row of x as channels, without the early exit: the per-measurement tensor operations and the float() read-back."""
    dev = x.device
    L = int(sr * (2.0 / measure_freq) + 0.5)
    N = 16
    while N < L:
        N *= 2
    P = int(sr / measure_freq + 0.5)
    s0, s1 = max(int(hp_filter_freq / sr * N + 0.5), 1), min(int(lp_filter_freq / sr * N + 0.5), N // 2)
    c0, c1 = math.ceil(sr * 0.5 / lp_lifter_freq), min(math.floor(sr * 0.5 / hp_lifter_freq), N // 4)
    w = torch.hann_window(L, periodic=True, device=dev) * (2.0 / math.sqrt(L))
    cw = torch.hann_window(s1 - s0, periodic=True, device=dev) * (2.0 / math.sqrt(s1 - s0))
    up, down = (torch.tensor(math.exp(-1 / (t * measure_freq)), device=dev) for t in (noise_up_time, noise_down_time))
    smooth, trig = math.exp(-1 / (measure_smooth_time * measure_freq)), math.exp(-1 / (trigger_time * measure_freq))
    boot_max = int(boot_time * measure_freq - 0.5)
    rows = x.shape[0]
    spec = [torch.zeros(N, device=dev) for _ in range(rows)]
    noise = [torch.zeros(N, device=dev) for _ in range(rows)]
    mean = [0.0] * rows
    hits = 0
    for f in range(frames):
        pos = L + f * P
        for r in range(rows):
            buf = torch.zeros(N, device=dev)
            buf[:L] = x[r, pos - L:pos] * w
            d = torch.fft.rfft(buf)[s0:s1].abs()
            mult = f / (1 + f) if f <= boot_max else smooth
            spec[r][s0:s1].mul_(mult).add_(d * (1 - mult))
            d = spec[r][s0:s1] ** 2
            zeros = torch.zeros(s1 - s0, device=dev)
            m = zeros if f <= boot_max else torch.where(d > noise[r][s0:s1], up, down)
            noise[r][s0:s1].mul_(m).add_(d * (1 - m))
            d = torch.sqrt(torch.max(zeros, d - noise_reduction_amount * noise[r][s0:s1]))
            cb = torch.zeros(N >> 1, device=dev)
            cb[s0:s1] = d * cw
            c = torch.fft.rfft(cb)
            result = float(torch.sum(c[c0:c1].abs().pow(2)))
            result = math.log(result / (c1 - c0)) if result > 0 else -math.inf
            mean[r] = mean[r] * trig + max(0, 21 + result) * (1 - trig)
            hits += mean[r] >= trigger_level
    return hits


def launch_shares(fn, x):
    """Device time per kernel name of one call, from a profiled run of its own; None where the profiler gives no device
    activity."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn(x)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for _ in range(3):
                fn(x)
            torch.cuda.synchronize()
        out = {}
        for e in prof.key_averages():
            t = getattr(e, "device_time_total", None)
            if t is None:
                t = getattr(e, "cuda_time_total", 0.0)
            if "vad" in e.key and t > 0:
                out[e.key.split("(")[0]] = t / 3.0
        return out or None
    except Exception as exc:                        # the timed numbers do not depend on the profiler
        print("launch shares not measured:", exc)
        return None


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--ref-rows", type=int, default=2)
    ap.add_argument("--ref-frames", type=int, default=20)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default=None, help="also write the results here")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_vad measures the device: no GPU, no number"
    dev = torch.device("cuda")
    rows_out = []
    for B, T_, sr in ((256, 160000, 16000), (8, 441000, 44100)):
        n_sets = max(2, -(-2 * MALL // (B * T_ * 4)) + 1)
        sets = [0.01 * torch.randn(B, T_, device=dev) for _ in range(n_sets)]
        plan = F._vad_plan(sr, 7.0, 0.25, 1.0, 0.25, 0.0, 0.35, 0.1, 0.01, 1.35, 20.0, None, 0.4, 50.0, 6000.0, 150.0, 2000.0)
        frames = F._vad_frames(T_, plan)
        t = [timed(lambda x: F.vad_start(x, sr), sets, a.iters, a.warmup) for _ in range(a.rounds)]
        short = [s[:a.ref_rows].contiguous() for s in sets[:2]]
        ref = timed(lambda x: ref_vad_measurements(x, sr, a.ref_frames), short, 1, 1)
        scale = (B * frames) / (a.ref_rows * a.ref_frames)
        floor = B * T_ * 4 / HBM_BYTES_PER_US
        shares = launch_shares(lambda x: F.vad_start(x, sr), sets[0])
        row = {"case": "vad_start", "shape": [B, T_], "sample_rate": sr, "frames": frames, "n_fft": plan.N,
               "us_median": statistics.median(t), "us_min": min(t), "read_floor_us_at_8TBps": floor,
               "restated_loop_us_scaled": ref * scale, "restated_loop_rows": a.ref_rows, "restated_loop_frames": a.ref_frames,
               "kernel_us": shares}
        rows_out.append(row)
        print("vad_start (%d, %d) at %d Hz: %10.1f us (min %10.1f), %d frames of %d points; one read at 8 TB/s: %.1f us (x%.0f); "
              "restated loop on %d rows x %d frames, scaled: %.0f us (x%.0f)" %
              (B, T_, sr, row["us_median"], row["us_min"], frames, plan.N, floor, row["us_median"] / floor, a.ref_rows, a.ref_frames,
               ref * scale, ref * scale / row["us_median"]))
        if shares:
            total = sum(shares.values())
            for k, v in sorted(shares.items(), key=lambda kv: -kv[1]):
                print("    %-60s %10.1f us  %5.1f %%" % (k[:60], v, 100 * v / total))
        del sets, short
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows_out, f, indent=1)


if __name__ == "__main__":
    main()
