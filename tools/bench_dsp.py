#!/usr/bin/env python
"""Device time of F.oscillator_bank on (16, 64000, 64) and (256, 16000, 1) and of F.filter_waveform on (64, 160000) with 1000
filters of 513 and of 65 taps and on (4, 16000) with 16000 filters of 65 taps (one filter per sample), float32, beside the
reference's compositions restated in plain torch on the same device.

The restatements: oscillator_bank as the reference writes it (the remainder of the phase increment, a float64 cumsum over
time cast back to float32 as it is, sin, product, sum over the oscillators); filter_waveform as unfold into chunks, one FFT
convolution per chunk against that chunk's filter (rfft, product, irfft), overlap-add (F.fold) and crop.  Both sides are
measured by one protocol in alternating rounds: device events around `--iters` calls after `--warmup`, divided by the calls,
rotating over `--sets` draws of the inputs (the oscillator's larger case is more than twice the Infinity Cache per draw);
median and minimum of `--rounds` such measurements.  Beside them: the bytes each of our calls must move (the oscillator reads
the frequencies twice and the amplitudes once) and the multiply-adds of the filter, as rates.

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


def restated_oscillator_bank(f, a, sample_rate):
    a = torch.where(f.abs() >= sample_rate / 2, torch.zeros((), dtype=a.dtype, device=a.device), a)
    w = f * (2 * math.pi) / sample_rate % (2 * math.pi)
    phases = torch.cumsum(w, dim=-2, dtype=torch.float64).to(f.dtype)
    return (a * torch.sin(phases)).sum(-1)


def restated_filter_waveform(x, kernels):
    B, T = x.shape
    Fn, L = kernels.shape
    C = T // Fn
    n = C + L - 1
    chunks = x.unfold(-1, C, C)                                                        # (B, F, C)
    y = torch.fft.irfft(torch.fft.rfft(chunks, n) * torch.fft.rfft(kernels, n), n)      # (B, F, n)
    total = (Fn - 1) * C + n
    out = torch.nn.functional.fold(y.transpose(1, 2), (1, total), (1, n), stride=(1, C)).reshape(B, total)
    d = (L - 1) // 2
    return out[:, d:d + T]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sets", type=int, default=3)
    ap.add_argument("--json", default=None, help="also write the results here")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_dsp measures the device: no GPU, no number"
    dev = torch.device("cuda")
    sr = 16000.0
    rows_out = []
    for B, T, N in ((16, 64000, 64), (256, 16000, 1)):
        g = torch.Generator(device=dev).manual_seed(B)
        sets = [((torch.rand(B, T, N, device=dev, generator=g) - 0.5) * 1.1 * sr, torch.rand(B, T, N, device=dev, generator=g))
                for _ in range(a.sets)]
        ours = lambda s: F.oscillator_bank(s[0], s[1], sr)                               # noqa: E731
        ref = lambda s: restated_oscillator_bank(s[0], s[1], sr)                          # noqa: E731
        worst = (ours(sets[0]) - ref(sets[0])).abs().max().item()
        t_ours, t_ref = [], []
        for _ in range(a.rounds):                                                        # alternating
            t_ours.append(timed(ours, sets, a.iters, a.warmup))
            t_ref.append(timed(ref, sets, a.iters, a.warmup))
        moved = B * T * N * 4 * 3 + B * T * 4
        row = {"case": "oscillator_bank", "shape": [B, T, N], "dtype": "float32", "us_median": statistics.median(t_ours),
               "us_min": min(t_ours), "bytes_moved": moved, "GB_per_s": moved / statistics.median(t_ours) / 1e3,
               "restated_us_median": statistics.median(t_ref), "restated_us_min": min(t_ref),
               "max_abs_difference_from_the_unreduced_float32_reference": worst}
        rows_out.append(row)
        print("oscillator_bank (%d, %d, %d): %10.1f us (min %10.1f), %.0f GB/s of its own traffic; restated in torch: %.1f us "
              "(x%.2f); max |difference| %.2e" % (B, T, N, row["us_median"], row["us_min"], row["GB_per_s"],
                                                  row["restated_us_median"], row["restated_us_median"] / row["us_median"], worst))
        del sets
        torch.cuda.empty_cache()
    for B, T, Fn, L in ((64, 160000, 1000, 513), (64, 160000, 1000, 65), (4, 16000, 16000, 65)):
        g = torch.Generator(device=dev).manual_seed(L + Fn)
        sets = [(torch.randn(B, T, device=dev, generator=g), torch.randn(Fn, L, device=dev, generator=g) / math.sqrt(L))
                for _ in range(a.sets)]
        ours = lambda s: F.filter_waveform(s[0], s[1])                                   # noqa: E731
        ref = lambda s: restated_filter_waveform(s[0], s[1])                              # noqa: E731
        worst = (ours(sets[0]) - ref(sets[0])).abs().max().item()
        t_ours, t_ref = [], []
        for _ in range(a.rounds):
            t_ours.append(timed(ours, sets, a.iters, a.warmup))
            t_ref.append(timed(ref, sets, a.iters, a.warmup))
        fmas = B * T * L
        row = {"case": "filter_waveform", "shape": [B, T], "num_filters": Fn, "taps": L, "dtype": "float32",
               "us_median": statistics.median(t_ours), "us_min": min(t_ours), "multiply_adds": fmas,
               "Gfma_per_s": fmas / statistics.median(t_ours) / 1e3, "kernel_bytes": Fn * L * 4,
               "restated_us_median": statistics.median(t_ref), "restated_us_min": min(t_ref), "max_abs_difference": worst}
        rows_out.append(row)
        print("filter_waveform (%d, %d), %d filters of %d taps: %10.1f us (min %10.1f), %.0f Gfma/s; restated in torch: %.1f us "
              "(x%.2f); max |difference| %.2e" % (B, T, Fn, L, row["us_median"], row["us_min"], row["Gfma_per_s"],
                                                  row["restated_us_median"], row["restated_us_median"] / row["us_median"], worst))
        del sets
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows_out, f, indent=1)


if __name__ == "__main__":
    main()
