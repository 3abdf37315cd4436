#!/usr/bin/env python
"""Device time of F.edit_distance_batch (csrc/edit_distance.h), with and without the error counts, at three shapes:

    (32, 10, 1500) int32 hypotheses, lengths uniform in [100, 300], against (32, 300) references   an n-best list to score
    (256, 1, 400) against (256, 400)                                                               a batch of transcripts
    (8, 1, 4000) against (8, 4096)                                                                 the widest configuration

Beside it the same distance restated in torch on the same device: row by row over the reference,
``t = min(prev[j-1] + sub, prev[j] + 1)`` and the insertion chain as ``arange + cummin(t - arange)``, the row of every pair's own
reference length kept and read at its hypothesis length; and the reference's pure-Python loop over the cells of one pair on
the host, timed on a few pairs (cut to 600 tokens a side) and scaled by cells.  The kernel and the restatement are timed by ONE
protocol: `--rounds` alternating rounds, each round device events around `--iters` calls after `--warmup` calls, divided by the calls; the figure is
the median over the rounds and the rounds' extremes are kept in the JSON.  The restatement costs thousands of launches a call,
so its rounds time `--ref-iters` calls.  A DP cell is one (reference token, hypothesis token) pair inside the lengths."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import audio_amd.functional as F  # noqa: E402

CASES = [("nbest", (32, 10, 1500), (32, 300), (100, 300)), ("batch", (256, 1, 400), (256, 400), None),
         ("wide", (8, 1, 4000), (8, 4096), None)]
ALPHABET = 32


def restated(hyps, refs, hyp_len, ref_len):
    """The distance of every pair, (*lead): the row recurrence in torch, on the tensors' device."""
    lead, N, M = hyps.shape[:-1], hyps.shape[-1], refs.shape[-1]
    per_ref = hyps[..., 0].numel() // max(refs[..., 0].numel(), 1)
    h = hyps.reshape(-1, N)
    r = refs.reshape(-1, M).repeat_interleave(per_ref, 0)
    hl = hyp_len.reshape(-1, 1).long()
    rl = ref_len.reshape(-1).repeat_interleave(per_ref, 0).long()
    ar = torch.arange(N + 1, device=h.device, dtype=torch.int32)
    prev = ar.expand(h.shape[0], N + 1).contiguous()
    out = prev.gather(1, hl).squeeze(1)                          # the pairs with an empty reference
    for i in range(M):
        sub = (r[:, i:i + 1] != h).to(torch.int32)
        t = torch.minimum(prev[:, :-1] + sub, prev[:, 1:] + 1)
        t = torch.cat([torch.full_like(t[:, :1], i + 1), t], 1)
        prev = ar + torch.cummin(t - ar, 1).values
        out = torch.where(rl == i + 1, prev.gather(1, hl).squeeze(1), out)
    return out.reshape(lead)


def python_loop(seq1, seq2):
    """The reference's F.edit_distance: two rolling rows in pure Python."""
    len2 = len(seq2)
    dold, dnew = list(range(len2 + 1)), [0] * (len2 + 1)
    for i in range(1, len(seq1) + 1):
        dnew[0] = i
        for j in range(1, len2 + 1):
            if seq1[i - 1] == seq2[j - 1]:
                dnew[j] = dold[j - 1]
            else:
                dnew[j] = min(dold[j - 1], dnew[j - 1], dold[j]) + 1
        dnew, dold = dold, dnew
    return int(dold[-1])


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


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ref-iters", type=int, default=1)
    ap.add_argument("--host-pairs", type=int, default=2)
    ap.add_argument("--json", default=None, help="also write the results here")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_edit_distance measures the device: no GPU, no number"
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(0)
    rows = []
    for name, hshape, rshape, lens in CASES:
        lead, N, M = hshape[:-1], hshape[-1], rshape[-1]
        hyps = torch.randint(0, ALPHABET, hshape, generator=g, dtype=torch.int32)
        refs = torch.randint(0, ALPHABET, rshape, generator=g, dtype=torch.int32)
        hl = (torch.randint(lens[0], lens[1] + 1, lead, generator=g, dtype=torch.int32) if lens
              else torch.full(lead, N, dtype=torch.int32))
        rl = torch.full(rshape[:-1], M, dtype=torch.int32)
        cells = int((hl.long() * M).sum())
        # the host loop, on the first pairs
        t0, host_cells = time.perf_counter(), 0
        for p in range(a.host_pairs):                           # at most 600 tokens a side: the loop's cost is per cell
            hp = hyps.reshape(-1, N)[p, :min(int(hl.reshape(-1)[p]), 600)].tolist()
            rp = refs.reshape(-1, M)[0, :600].tolist()
            python_loop(rp, hp)
            host_cells += len(hp) * len(rp)
        host_us = (time.perf_counter() - t0) * 1e6 / host_cells * cells
        d = [t.to(dev) for t in (hyps, refs, hl, rl)]
        want = restated(*d)
        for return_ops in (False, True):
            got = F.edit_distance_batch(*d, return_ops=return_ops)
            assert torch.equal(got[..., 0] if return_ops else got, want), name
            ours, theirs = [], []
            for _ in range(a.rounds):
                ours.append(timed(lambda: F.edit_distance_batch(*d, return_ops=return_ops), a.iters, a.warmup))
                if not return_ops:
                    theirs.append(timed(lambda: restated(*d), a.ref_iters, 1))
            us = statistics.median(ours)
            r = {"case": f"edit_distance_batch {name} {hshape} vs {rshape}" + (" return_ops" if return_ops else ""),
                 "pairs": int(hl.numel()), "cells": cells, "us": round(us, 2), "ns_per_cell": round(us * 1e3 / cells, 4),
                 "rounds_us": [round(min(ours), 2), round(max(ours), 2)]}
            if theirs:
                ref = statistics.median(theirs)
                r.update({"restated_reference": "row recurrence with cummin, torch, same device", "restated_us": round(ref, 1),
                          "speedup": round(ref / us, 2), "restated_rounds_us": [round(min(theirs), 1), round(max(theirs), 1)],
                          "host_python_loop_us_scaled": round(host_us, 0), "host_pairs_timed": a.host_pairs})
            rows.append(r)
            print(json.dumps(r), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
