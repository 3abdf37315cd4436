#!/usr/bin/env python
"""Device time of F.stoi (csrc/stoi.h), STOI and ESTOI, at three shapes:

    (256, 160000) float32 at 16 kHz     a validation batch of 10 s utterances
    (32, 40000) at 10 kHz               the measure alone, no resampling
    (8, 441000) at 44.1 kHz             a few long recordings

For the rates other than 10 kHz the two F.resample calls are timed on their own and the measure on the resampled signals, so
the resampler's share of the whole call is separate.  Beside it the definition restated in torch on the same device (unfold,
a stable argsort of the keep flags in place of the scan, torch.fft.rfft, a 0/1 band matrix, unfold over frames; float32 up
to the band magnitudes, float64 after), and the float64 numpy definition of tests/stoi_oracle.py on the host, timed on
`--host-rows` rows and scaled by rows.  The kernel and the restatement are timed by ONE protocol: `--rounds` alternating
rounds, each round device events around `--iters` calls after `--warmup` calls, divided by the calls; the figure is the median
over the rounds and the rounds' extremes are kept in the JSON.  The restatement's rounds time `--ref-iters` calls."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import audio_amd.functional as F  # noqa: E402
import stoi_oracle as O  # noqa: E402

CASES = [("val16k", (256, 160000), 16000), ("at10k", (32, 40000), 10000), ("long44k", (8, 441000), 44100)]
EPS = 2.0 ** -52


def _normalize(a, dim):
    a = a - a.mean(dim, keepdim=True)
    return a / (a.norm(dim=dim, keepdim=True) + EPS)


def restated(preds, target, extended):
    """(B,) scores of (B, T) float32 signals at 10 kHz: the definition in torch, on the tensors' device, without a read-back."""
    dev, B = preds.device, preds.shape[0]
    w64 = torch.from_numpy(O.window()).to(dev)
    w = w64.float()
    fx, fy = target.unfold(-1, 256, 128), preds.unfold(-1, 256, 128)                   # (B, K, 256)
    K = fx.shape[1]
    e = 20.0 * torch.log10(((fx.double() * w64) ** 2).sum(-1).sqrt() + EPS)
    keep = e > e.max(1, keepdim=True).values - 40.0
    n = keep.sum(1)
    order = torch.argsort((~keep).to(torch.int8), dim=1, stable=True)                  # the kept frames first, ascending
    live = (torch.arange(K, device=dev)[None, :] < n[:, None])[..., None]
    mats = []
    for f in (fx, fy):
        fk = (f * w).gather(1, order[..., None].expand(-1, -1, 256)) * live
        s = torch.zeros((B, K + 1, 128), device=dev)
        s[:, :K] += fk[..., :128]
        s[:, 1:] += fk[..., 128:]
        fr = s.reshape(B, -1).unfold(-1, 256, 128)[:, :K] * w                         # frame m is valid for m < n - 1
        p = torch.fft.rfft(fr, n=512).abs() ** 2
        bands = torch.zeros((257, 15), device=dev)
        for b in range(15):
            bands[O.BAND_LO[b]:O.BAND_HI[b], b] = 1.0
        mats.append((p @ bands).sqrt().double())
    J = n - 1 - 29                                                                      # segments per row (may be < 1)
    a = mats[0].unfold(1, 30, 1)                                                        # (B, K - 29, 15, 30)
    c = mats[1].unfold(1, 30, 1)
    if extended:
        A, Cm = _normalize(_normalize(a, 3), 2), _normalize(_normalize(c, 3), 2)
        per = (A * Cm).sum((2, 3))
        div = 30.0
    else:
        alpha = a.norm(dim=3, keepdim=True) / (c.norm(dim=3, keepdim=True) + EPS)
        cp = torch.minimum(alpha * c, (1.0 + 10.0 ** 0.75) * a)
        per = (_normalize(a, 3) * _normalize(cp, 3)).sum((2, 3))
        div = 15.0
    valid = torch.arange(per.shape[1], device=dev)[None, :] < J[:, None]
    score = (per * valid).sum(1) / (div * J.clamp(min=1))
    return torch.where(J >= 1, score, torch.full_like(score, 1e-5))


def speechlike(shape, rate, seed):
    """Gated harmonic rows at `rate` and their noisy versions at 5 dB: (target, preds), float32 on the host."""
    rows, T = shape
    rng = np.random.default_rng(seed)
    t = np.arange(T, dtype=np.float64) / rate
    x = np.empty(shape, np.float32)
    for r in range(rows):
        ph = 2 * np.pi * 120.0 * t + 2 * np.pi * rng.random()
        car = sum(np.sin(h * ph) / h for h in range(1, 13))
        env = np.sin(np.pi * (1.3 + 0.4 * rng.random()) * t + np.pi * rng.random()) ** 2
        gate = np.mod(0.35 * t + rng.random(), 1.0) < 0.6
        x[r] = 0.05 * car * env * gate + 1e-4 * rng.standard_normal(T)
    noise = rng.standard_normal(shape).astype(np.float32)
    g = np.sqrt((x.astype(np.float64) ** 2).mean() / 10.0 ** 0.5)
    return torch.from_numpy(x), torch.from_numpy(x + g.astype(np.float32) * noise)


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
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ref-iters", type=int, default=2)
    ap.add_argument("--host-rows", type=int, default=2)
    ap.add_argument("--cases", default=",".join(c[0] for c in CASES))
    ap.add_argument("--json", default=None, help="also write the results here")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_stoi measures the device: no GPU, no number"
    dev = torch.device("cuda")
    rows = []
    for name, shape, rate in CASES:
        if name not in a.cases.split(","):
            continue
        target, preds = (t.to(dev) for t in speechlike(shape, rate, 0))
        if rate != 10000:
            t10, p10 = F.resample(target, rate, 10000), F.resample(preds, rate, 10000)
            res_us = statistics.median(timed(lambda: (F.resample(target, rate, 10000), F.resample(preds, rate, 10000)), a.iters,
                                             a.warmup) for _ in range(a.rounds))
        else:
            t10, p10, res_us = target, preds, 0.0
        # the host definition, on the first rows
        hx, hy = t10[:a.host_rows].cpu().numpy(), p10[:a.host_rows].cpu().numpy()
        for extended in (False, True):
            t0 = time.perf_counter()
            host = [O.stoi(hy[r], hx[r], extended) for r in range(a.host_rows)]
            host_us = (time.perf_counter() - t0) * 1e6 / a.host_rows * shape[0]
            got = F.stoi(p10, t10, 10000, extended)
            ref = restated(p10, t10, extended)
            diff = (got.double() - ref).abs()               # a frame within rounding of the 40 dB threshold may flip in one row
            assert float(diff.median()) < 1e-4, (name, extended, got[:4], ref[:4])
            assert max(abs(float(got[r]) - host[r]) for r in range(a.host_rows)) < 1e-4, (name, extended)
            ours, whole, theirs = [], [], []
            for _ in range(a.rounds):
                ours.append(timed(lambda: F.stoi(p10, t10, 10000, extended), a.iters, a.warmup))
                if rate != 10000:
                    whole.append(timed(lambda: F.stoi(preds, target, rate, extended), a.iters, a.warmup))
                theirs.append(timed(lambda: restated(p10, t10, extended), a.ref_iters, 1))
            us, ref_us = statistics.median(ours), statistics.median(theirs)
            frames = shape[0] * max((t10.shape[-1] - 256) // 128 + 1, 0)
            r = {"case": f"stoi {name} {shape} at {rate} Hz" + (" extended" if extended else ""), "rows": shape[0],
                 "samples_at_10k": int(t10.shape[-1]), "frames": frames, "mean_score": round(float(got.mean()), 4),
                 "max_abs_diff_vs_restated": float(diff.max()),
                 "us_at_10k": round(us, 1), "ns_per_frame": round(us * 1e3 / frames, 2), "rounds_us": [round(min(ours), 1), round(max(ours), 1)],
                 "resample_both_us": round(res_us, 1),
                 "whole_call_us": round(statistics.median(whole), 1) if whole else round(us, 1),
                 "resample_share": round(res_us / statistics.median(whole), 3) if whole else 0.0,
                 "bytes_read_MB": round(2 * shape[0] * t10.shape[-1] * 4 * 2 / 1e6, 1),
                 "restated_reference": "the definition in torch (unfold, argsort, rfft, band matrix), same device",
                 "restated_us": round(ref_us, 1), "speedup": round(ref_us / us, 2),
                 "restated_rounds_us": [round(min(theirs), 1), round(max(theirs), 1)],
                 "host_numpy_us_scaled": round(host_us, 0), "host_rows_timed": a.host_rows,
                 "speedup_vs_host": round(host_us / (statistics.median(whole) if whole else us), 1)}
            assert math.isfinite(r["us_at_10k"])
            rows.append(r)
            print(json.dumps(r), flush=True)
        del target, preds, t10, p10
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
