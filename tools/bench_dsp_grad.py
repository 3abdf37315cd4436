#!/usr/bin/env python
"""Device time of forward + backward of F.oscillator_bank on (16, 64000, 64) and (256, 16000, 1) and of F.filter_waveform on
(64, 160000) with 1000 filters of 513 and of 65 taps and on (4, 16000) with 16000 filters of 65 taps, float32, every input
requiring grad, beside the differentiable torch compositions (audio_amd._diff) that served the training path before the
backward kernels (csrc/dsp_synth_grad.h) and still serve create_graph=True.

The protocol is tools/bench_dsp.py's: both sides in alternating rounds, device events around `--iters` calls of
torch.autograd.grad(op(inputs), inputs, cotangent) after `--warmup`, divided by the calls, rotating over `--sets` draws of the
inputs; median and minimum of `--rounds` such measurements, and the peak of the allocator above the inputs for one call of each
side.  Where a composition cannot allocate its temporaries that is the result, not a time.  Both sides are also compared once:
the largest difference between their gradients, relative to the largest gradient."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import audio_amd.functional as F  # noqa: E402
from audio_amd import _diff  # noqa: E402


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


def peak_of(fn, s):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn(s)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    return out, peak


def measure(name, meta, ours, ref, sets, a):
    got, peak_ours = peak_of(ours, sets[0])
    row = dict(meta, case=name, dtype="float32", peak_bytes=peak_ours)
    try:
        want, peak_ref = peak_of(ref, sets[0])
        row["composition_peak_bytes"] = peak_ref
        row["max_relative_difference_of_the_gradients"] = max(
            ((g - w).abs().max() / w.abs().max()).item() for g, w in zip(got, want))
        del want
        composed = True
    except torch.cuda.OutOfMemoryError:
        row["composition"] = "cannot allocate"
        composed = False
    del got
    torch.cuda.empty_cache()
    t_ours, t_ref = [], []
    for _ in range(a.rounds):                                                            # alternating
        t_ours.append(timed(ours, sets, a.iters, a.warmup))
        if composed:
            try:
                t_ref.append(timed(ref, sets, a.iters, a.warmup))
            except torch.cuda.OutOfMemoryError:
                row["composition"] = "cannot allocate"
                composed, t_ref = False, []
                torch.cuda.empty_cache()
    row.update(us_median=statistics.median(t_ours), us_min=min(t_ours))
    if t_ref:
        row.update(composition_us_median=statistics.median(t_ref), composition_us_min=min(t_ref))
    print("%s %s forward + backward: %10.1f us (min %10.1f), peak %.1f MB; composition: %s" % (
        name, meta, row["us_median"], row["us_min"], peak_ours / 1e6,
        "%.1f us (x%.2f), peak %.1f MB, gradients within %.1e" % (
            row["composition_us_median"], row["composition_us_median"] / row["us_median"], row["composition_peak_bytes"] / 1e6,
            row["max_relative_difference_of_the_gradients"]) if t_ref else "cannot allocate"), flush=True)
    return row


def write(path, rows):
    """After every case: a long run that is cut short keeps what it measured."""
    if path:
        with open(path, "w") as f:
            json.dump(rows, f, indent=1)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sets", type=int, default=2)
    ap.add_argument("--json", default=None, help="also write the results here")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_dsp_grad measures the device: no GPU, no number"
    dev = torch.device("cuda")
    sr = 16000.0
    rows_out = []
    for B, T, N in ((16, 64000, 64), (256, 16000, 1)):
        g = torch.Generator(device=dev).manual_seed(B)
        sets = [(((torch.rand(B, T, N, device=dev, generator=g) - 0.5) * 1.1 * sr).requires_grad_(),
                 torch.rand(B, T, N, device=dev, generator=g).requires_grad_(), torch.randn(B, T, device=dev, generator=g))
                for _ in range(a.sets)]
        ours = lambda s: torch.autograd.grad(F.oscillator_bank(s[0], s[1], sr), (s[0], s[1]), s[2])           # noqa: E731
        ref = lambda s: torch.autograd.grad(_diff.oscillator_bank(s[0], s[1], sr, "sum"), (s[0], s[1]), s[2])  # noqa: E731
        rows_out.append(measure("oscillator_bank", {"shape": [B, T, N]}, ours, ref, sets, a))
        write(a.json, rows_out)
        del sets
        torch.cuda.empty_cache()
    for B, T, Fn, L in ((4, 16000, 16000, 65), (64, 160000, 1000, 65), (64, 160000, 1000, 513)):
        g = torch.Generator(device=dev).manual_seed(L + Fn)
        sets = [(torch.randn(B, T, device=dev, generator=g).requires_grad_(),
                 (torch.randn(Fn, L, device=dev, generator=g) / math.sqrt(L)).requires_grad_(),
                 torch.randn(B, T, device=dev, generator=g)) for _ in range(a.sets)]
        ours = lambda s: torch.autograd.grad(F.filter_waveform(s[0], s[1]), (s[0], s[1]), s[2])               # noqa: E731
        ref = lambda s: torch.autograd.grad(_diff.filter_waveform(s[0], s[1]), (s[0], s[1]), s[2])            # noqa: E731
        row = measure("filter_waveform", {"shape": [B, T], "num_filters": Fn, "taps": L}, ours, ref, sets, a)
        row["multiply_adds"] = 3 * B * T * L                                 # forward, grad_waveform, grad_kernels
        row["Gfma_per_s"] = row["multiply_adds"] / row["us_median"] / 1e3
        rows_out.append(row)
        write(a.json, rows_out)
        del sets
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
