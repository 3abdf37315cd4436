#!/usr/bin/env python
"""Device time of F.permutation_invariant_training with SI-SNR (csrc/pit.h), forward and forward + backward, float32, at

    (256, 2, 64000)    a training batch of two-speaker 4 s crops at 16 kHz
    (64, 4, 160000)    four sources, 10 s
    (16, 8, 160000)    eight sources, 10 s

Beside it the composition the package offered before: F.scale_invariant_signal_noise_ratio on the S^2 expanded pairs (made
contiguous by the row-wise entry point), then for S <= 4 a torch maximum over the stacked permutations on the device and for
S = 8 the host's itertools search over the matrix, with the same autograd.  Both sides are timed by ONE protocol: `--rounds`
alternating rounds, each round device events around `--iters` calls after `--warmup` calls, over input sets taken in rotation
whose bytes exceed twice the Infinity Cache (256 MB), so that no call finds its operands where the last one left them; the
figure is the median over the rounds, the rounds' extremes and the allocator's peak above the inputs are kept in the JSON,
with the fused forward's fraction of its byte floor: each waveform read twice at 8 TB/s."""
import argparse
import itertools
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

CASES = [("two_spk", (256, 2, 64000)), ("four_src", (64, 4, 160000)), ("eight_src", (16, 8, 160000))]
HBM_BYTES_PER_S, CACHE_BYTES = 8e12, 256e6


def composed(preds, target):
    B, S, T = preds.shape
    m = F.scale_invariant_signal_noise_ratio(preds[:, :, None].expand(B, S, S, T), target[:, None, :].expand(B, S, S, T))
    rows = torch.arange(S, device=m.device)
    if S <= 4:
        perms = torch.tensor(list(itertools.permutations(range(S))), device=m.device)
        totals = m[:, rows, perms].sum(-1)                                       # (B, S!)
        best, k = totals.max(-1)
        return best / S, perms[k]
    host = m.detach().cpu().tolist()                                              # the reference's route from three sources on
    perm = torch.tensor([max(itertools.permutations(range(S)), key=lambda q: sum(host[b][i][q[i]] for i in range(S)))
                         for b in range(B)], device=m.device)
    return torch.gather(m, 2, perm.unsqueeze(-1)).squeeze(-1).mean(-1), perm


def with_backward(fn):
    def run(p, t):
        p.grad = None
        fn(p, t)[0].sum().backward()
    return run


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ref-iters", type=int, default=2)
    ap.add_argument("--cases", default=",".join(c[0] for c in CASES))
    ap.add_argument("--json", default=None, help="also write the results here")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_pit measures the device: no GPU, no number"
    dev, rows = torch.device("cuda"), []
    for name, shape in CASES:
        if name not in a.cases.split(","):
            continue
        B, S, T = shape
        in_bytes = 2 * B * S * T * 4
        n_sets = int(2 * CACHE_BYTES // in_bytes) + 2
        g = torch.Generator(device=dev).manual_seed(0)
        sets = []
        for _ in range(n_sets):
            t = torch.randn(shape, device=dev, generator=g)
            t = t + 0.9 * torch.roll(t, 1, -1)
            p = t[:, torch.randperm(S).tolist()] + 0.3 * torch.randn(shape, device=dev, generator=g)
            sets.append((p.requires_grad_(), t))
        plain = [(p.detach(), t) for p, t in sets]
        ours_fn = lambda p, t: F.permutation_invariant_training(p, t, F.scale_invariant_signal_noise_ratio)  # noqa: E731
        (b0, p0), (b1, p1) = ours_fn(*plain[0]), composed(*plain[0])
        assert torch.equal(p0, p1) and float((b0 - b1).abs().max()) < 1e-3, (name, float((b0 - b1).abs().max()))
        for what, f_ours, f_ref, data in (("forward", ours_fn, composed, plain),
                                          ("forward+backward", with_backward(ours_fn), with_backward(composed), sets)):
            ours, theirs = [], []
            for _ in range(a.rounds):
                ours.append(timed(f_ours, data, a.iters, a.warmup))
                theirs.append(timed(f_ref, data, a.ref_iters, 1))
            us, ref_us = statistics.median(o[0] for o in ours), statistics.median(o[0] for o in theirs)
            r = {"case": f"pit si_snr {what} {name} {shape} float32", "us": round(us, 1),
                 "rounds_us": [round(min(o[0] for o in ours), 1), round(max(o[0] for o in ours), 1)],
                 "peak_MB": round(max(o[1] for o in ours), 1), "input_MB": round(in_bytes / 1e6, 1), "input_sets": n_sets,
                 "composition": "S^2 expanded rows through F.scale_invariant_signal_noise_ratio, " +
                                ("torch max over the stacked permutations" if S <= 4 else "host itertools search"),
                 "composition_us": round(ref_us, 1),
                 "composition_rounds_us": [round(min(o[0] for o in theirs), 1), round(max(o[0] for o in theirs), 1)],
                 "composition_peak_MB": round(max(o[1] for o in theirs), 1), "speedup": round(ref_us / us, 2)}
            if what == "forward":
                r["floor_us_two_reads_at_8TBps"] = round(2 * in_bytes / HBM_BYTES_PER_S * 1e6, 1)
                r["fraction_of_floor"] = round(r["floor_us_two_reads_at_8TBps"] / us, 3)
            rows.append(r)
            print(json.dumps(r), flush=True)
        del sets, plain
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
