#!/usr/bin/env python
"""Device time of F.add_noise (with and without lengths) and F.preemphasis on a (256, 160000) float32 batch (256 utterances
of 10 s at 16 kHz), beside the reference's compositions restated in plain torch on the same device.

Each case rotates over enough input sets that together they exceed twice the 256 MiB Infinity Cache, so every call streams
its inputs from HBM.  Time = device events around `--iters` calls after `--warmup`, divided by the calls; `--rounds` such
measurements per case, kernel and restatement alternating, median and minimum reported.  Roofline bytes: add_noise moves
five row-sets in its two launches (waveform and noise read twice, the result written once; the minimum is three),
preemphasis two.  The fraction is of 8 TB/s.

Restatements (labelled as such; torchaudio is not needed and the code under test is not used): add_noise = masks, two
vector norms, logs, a power, a broadcast multiply and an add; preemphasis = clone and an in-place subtraction of a slice."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import audio_amd.functional as F  # noqa: E402

PEAK = 8.0e12
MALL = 256 << 20


def timed(fn, sets, iters, warmup):
    for i in range(warmup):
        fn(*sets[i % len(sets)])
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(iters):
        fn(*sets[i % len(sets)])
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters          # us per call


def ref_add_noise(waveform, noise, snr, lengths=None):
    """Restatement of the reference's add_noise."""
    L = waveform.size(-1)
    if lengths is not None:
        mask = torch.arange(0, L, device=lengths.device).expand(waveform.shape) < lengths.unsqueeze(-1)
        masked_waveform, masked_noise = waveform * mask, noise * mask
    else:
        masked_waveform, masked_noise = waveform, noise
    energy_signal = torch.linalg.vector_norm(masked_waveform, ord=2, dim=-1) ** 2
    energy_noise = torch.linalg.vector_norm(masked_noise, ord=2, dim=-1) ** 2
    original_snr_db = 10 * (torch.log10(energy_signal) - torch.log10(energy_noise))
    scale = 10 ** ((original_snr_db - snr) / 20.0)
    return waveform + scale.unsqueeze(-1) * noise


def ref_preemphasis(waveform, coeff=0.97):
    """Restatement of the reference's preemphasis."""
    waveform = waveform.clone()
    waveform[..., 1:] -= coeff * waveform[..., :-1]
    return waveform


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--length", type=int, default=160000)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None, help="also write the results here")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_wave_augment measures the device: no GPU, no number"
    dev = torch.device("cuda")
    B, L = a.batch, a.length
    rowset = B * L * 4
    n_sets = max(2, -(-2 * MALL // (2 * rowset)) + 1)           # waveform + noise per set; > 2 x the Infinity Cache in total
    sets = [(0.1 * torch.randn(B, L, device=dev), 0.1 * torch.randn(B, L, device=dev)) for _ in range(n_sets)]
    snr = torch.linspace(-5.0, 30.0, B, device=dev)
    lengths = torch.randint(L // 2, L + 1, (B,), device=dev)
    rows = []

    def case(name, fn, ref, moved, minimum, label):
        ours, theirs = [], []
        for _ in range(a.rounds):
            ours.append(timed(fn, sets, a.iters, a.warmup))
            theirs.append(timed(ref, sets, max(a.iters // 3, 3), 2))
        us, us_min, ref_us = statistics.median(ours), min(ours), statistics.median(theirs)
        frac = moved / (us * 1e-6) / PEAK
        r = {"case": name, "us_median": round(us, 2), "us_min": round(us_min, 2), "bytes_moved": moved,
             "bytes_minimum": minimum, "frac_8TBps": round(frac, 3), "floor_us": round(moved / PEAK * 1e6, 1),
             "restated_reference": label, "restated_us_median": round(ref_us, 1), "speedup": round(ref_us / us, 2)}
        rows.append(r)
        print(f"{name:38s} {us:9.2f} us (min {us_min:8.2f})  {moved / 1e6:7.1f} MB  {frac:5.3f} of 8 TB/s   "
              f"| {label}: {ref_us:9.1f} us  ({ref_us / us:5.2f} x)", flush=True)

    with torch.no_grad():
        case(f"add_noise ({B},{L}) f32", lambda w, n: F.add_noise(w, n, snr), lambda w, n: ref_add_noise(w, n, snr),
             5 * rowset, 3 * rowset, "torch composition (restated)")
        case(f"add_noise ({B},{L}) f32 lengths", lambda w, n: F.add_noise(w, n, snr, lengths),
             lambda w, n: ref_add_noise(w, n, snr, lengths), 5 * rowset, 3 * rowset, "torch composition (restated)")
        case(f"preemphasis ({B},{L}) f32", lambda w, n: F.preemphasis(w), lambda w, n: ref_preemphasis(w),
             2 * rowset, 2 * rowset, "clone + sliced subtraction (restated)")
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
