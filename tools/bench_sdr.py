#!/usr/bin/env python
"""Device time of F.signal_distortion_ratio (filter_length 512) and F.scale_invariant_signal_distortion_ratio, forward and
forward + backward (csrc/sdr.h), float32, at three shapes:

    (256, 160000)    a validation batch of 10 s utterances at 16 kHz
    (32, 40000)      a training batch of short crops
    (8, 441000)      a few long recordings

Beside SDR the definition restated in torch on the same device (float64, zero-padded torch.fft correlations, a Toeplitz
gather and torch.linalg.solve); beside SI-SDR the torch expression and its autograd.  Both sides are timed by ONE protocol:
`--rounds` alternating rounds, each round device events around `--iters` calls after `--warmup` calls, over `--sets` input
sets taken in rotation so that no call finds its operands where the last one left them; the figure is the median over the
rounds, the rounds' extremes and the allocator's peak above the inputs are kept in the JSON.  The restatement's rounds time
`--ref-iters` calls."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import audio_amd.functional as F  # noqa: E402

CASES = [("val16k", (256, 160000)), ("crops", (32, 40000)), ("long44k", (8, 441000))]
EPS = torch.finfo(torch.float32).eps


def sdr_restated(preds, target, L=512):
    p, t = preds.double(), target.double()
    p = p / p.norm(dim=-1, keepdim=True).clamp_min(1e-6)
    t = t / t.norm(dim=-1, keepdim=True).clamp_min(1e-6)
    n = 1 << (2 * t.shape[-1] - 1).bit_length()
    tf, pf = torch.fft.rfft(t, n), torch.fft.rfft(p, n)
    r = torch.fft.irfft(tf.real ** 2 + tf.imag ** 2, n)[..., :L]
    b = torch.fft.irfft(tf.conj() * pf, n)[..., :L]
    i = torch.arange(L, device=t.device)
    h = torch.linalg.solve(r[..., (i[:, None] - i[None, :]).abs()], b)
    coh = (b * h).sum(-1)
    return 10 * torch.log10(coh / (1 - coh))


def si_sdr_restated(preds, target):
    alpha = ((preds * target).sum(-1, keepdim=True) + EPS) / ((target ** 2).sum(-1, keepdim=True) + EPS)
    s = alpha * target
    return 10 * torch.log10(((s ** 2).sum(-1) + EPS) / (((s - preds) ** 2).sum(-1) + EPS))


def timed(fn, sets, iters, warmup):
    """(us per call, allocator peak above what was held at entry in MB); call k takes input set k mod len(sets)."""
    for k in range(warmup):
        fn(*sets[k % len(sets)])
    torch.cuda.synchronize()
    for x in (x for s in sets for x in s):                                       # the warm-up's gradients are not "held at entry"
        x.grad = None
    torch.cuda.reset_peak_memory_stats()
    held = torch.cuda.memory_allocated()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for k in range(iters):
        fn(*sets[k % len(sets)])
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters, (torch.cuda.max_memory_allocated() - held) / 1e6


def with_backward(fn):
    def run(p, t):
        p.grad = None
        fn(p, t).sum().backward()
    return run


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ref-iters", type=int, default=3)
    ap.add_argument("--sets", type=int, default=3)
    ap.add_argument("--cases", default=",".join(c[0] for c in CASES))
    ap.add_argument("--json", default=None, help="also write the results here")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_sdr measures the device: no GPU, no number"
    dev, rows = torch.device("cuda"), []
    for name, shape in CASES:
        if name not in a.cases.split(","):
            continue
        g = torch.Generator(device=dev).manual_seed(0)
        sets = []
        for _ in range(a.sets):
            t = torch.randn(shape, device=dev, generator=g)
            t = t + 0.9 * torch.roll(t, 1, -1)                                   # coloured, so the system is not the identity
            sets.append(((t + 0.3 * torch.randn(shape, device=dev, generator=g)).requires_grad_(), t))
        plain = [(p.detach(), t) for p, t in sets]
        plans = [("sdr L=512", lambda p, t: F.signal_distortion_ratio(p, t), sdr_restated, plain, 1e-6,
                  "float64 torch.fft correlations, Toeplitz gather, torch.linalg.solve"),
                 ("si_sdr forward", lambda p, t: F.scale_invariant_signal_distortion_ratio(p, t), si_sdr_restated, plain, 1e-3,
                  "the torch expression in float32"),
                 ("si_sdr forward+backward", with_backward(lambda p, t: F.scale_invariant_signal_distortion_ratio(p, t)),
                  with_backward(si_sdr_restated), sets, None, "the torch expression in float32 and its autograd")]
        for what, ours_fn, ref_fn, data, tol, ref_name in plans:
            if tol is not None:
                diff = float((ours_fn(*data[0]).double() - ref_fn(*data[0]).double()).abs().max())
                assert diff < tol * 20, (name, what, diff)
            ours, theirs = [], []
            for _ in range(a.rounds):
                ours.append(timed(ours_fn, data, a.iters, a.warmup))
                theirs.append(timed(ref_fn, data, a.ref_iters, 1))
            us, ref_us = statistics.median(o[0] for o in ours), statistics.median(o[0] for o in theirs)
            r = {"case": f"{what} {name} {shape} float32", "us": round(us, 1), "rounds_us": [round(min(o[0] for o in ours), 1), round(max(o[0] for o in ours), 1)],
                 "peak_MB": round(max(o[1] for o in ours), 1), "input_MB": round(2 * shape[0] * shape[1] * 4 / 1e6, 1),
                 "max_abs_diff_vs_restated_dB": diff if tol is not None else None, "restated_reference": ref_name,
                 "restated_us": round(ref_us, 1), "restated_rounds_us": [round(min(o[0] for o in theirs), 1), round(max(o[0] for o in theirs), 1)],
                 "restated_peak_MB": round(max(o[1] for o in theirs), 1), "speedup": round(ref_us / us, 2)}
            if what.startswith("sdr"):
                r["GFLOP_matrix"] = round(shape[0] * shape[1] * 2 * 528 * 2 / 1e9, 2)
            rows.append(r)
            print(json.dumps(r), flush=True)
        del sets, plain
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
