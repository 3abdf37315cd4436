#!/usr/bin/env python
"""Device time of F.compute_deltas and F.sliding_window_cmn at the ASR front-end's shape (256 utterances of 10 s: 1 001 frames
x 80 features, float32), beside the reference's compositions restated in plain torch on the same device.

Each case rotates over enough input buffers that together they exceed the 256 MiB Infinity Cache, so every call streams
its input from HBM.  Time = device events around `--iters` calls after `--warmup`, divided by the calls.  Bytes =
algorithmic input + output (each element read once and written once); the fraction is of 8 TB/s.

Restatements (labelled as such; torchaudio is not needed): compute_deltas = F.pad + grouped conv1d; sliding_window_cmn =
the reference's per-frame loop (a few device ops per frame), timed on `--loop-batch` utterances and scaled linearly to the
full batch (its cost is per-op launches, not bytes)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import audio_amd.functional as F  # noqa: E402
import audio_amd.transforms as T  # noqa: E402

PEAK = 8.0e12
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


def ref_deltas(x, win_length=5, mode="replicate"):
    """Restatement of the reference's compute_deltas: pad + grouped conv1d."""
    shape = x.size()
    x = x.reshape(1, -1, shape[-1])
    n = (win_length - 1) // 2
    denom = n * (n + 1) * (2 * n + 1) / 3
    xp = torch.nn.functional.pad(x, (n, n), mode=mode)
    kernel = torch.arange(-n, n + 1, 1, device=x.device, dtype=x.dtype).repeat(x.shape[1], 1, 1)
    return (torch.nn.functional.conv1d(xp, kernel, groups=x.shape[1]) / denom).reshape(shape)


def ref_cmn(specgram, cmn_window=600, min_cmn_window=100, center=False, norm_vars=False):
    """Restatement of the reference's sliding_window_cmn: the per-frame loop with a running float32 sum."""
    input_shape = specgram.shape
    num_frames, num_feats = input_shape[-2:]
    specgram = specgram.view(-1, num_frames, num_feats)
    C = specgram.shape[0]
    lws = lwe = -1
    cur_sum = torch.zeros(C, num_feats, dtype=specgram.dtype, device=specgram.device)
    cur_sumsq = torch.zeros_like(cur_sum)
    out = torch.zeros_like(specgram)
    for t in range(num_frames):
        if center:
            ws = t - cmn_window // 2
            we = ws + cmn_window
        else:
            ws = t - cmn_window
            we = t + 1
        if ws < 0:
            we -= ws
            ws = 0
        if not center and we > t:
            we = max(t + 1, min_cmn_window)
        if we > num_frames:
            ws -= we - num_frames
            we = num_frames
            ws = max(ws, 0)
        if lws == -1:
            part = specgram[:, ws:we, :]
            cur_sum += torch.sum(part, 1)
            if norm_vars:
                cur_sumsq += torch.cumsum(part ** 2, 1)[:, -1, :]
        else:
            if ws > lws:
                f = specgram[:, lws, :]
                cur_sum -= f
                if norm_vars:
                    cur_sumsq -= f ** 2
            if we > lwe:
                f = specgram[:, lwe, :]
                cur_sum += f
                if norm_vars:
                    cur_sumsq += f ** 2
        n = we - ws
        lws, lwe = ws, we
        out[:, t, :] = specgram[:, t, :] - cur_sum / n
        if norm_vars:
            if n == 1:
                out[:, t, :] = torch.zeros(C, num_feats, dtype=specgram.dtype, device=specgram.device)
            else:
                var = cur_sumsq / n - cur_sum ** 2 / n ** 2
                out[:, t, :] *= torch.pow(var, -0.5)
    return out.view(input_shape)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--loop-batch", type=int, default=16)
    ap.add_argument("--json", default=None, help="also write the results here")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_feat_post measures the device: no GPU, no number"
    dev = torch.device("cuda")
    B, Tn, Fm = a.batch, 1001, 80
    nbytes = B * Tn * Fm * 4
    rows = []

    def report(name, us, ref_us, ref_label):
        frac = (2 * nbytes) / (us * 1e-6) / PEAK
        r = {"case": name, "us": round(us, 2), "bytes": 2 * nbytes, "frac_8TBps": round(frac, 3),
             "restated_reference": ref_label, "restated_us": round(ref_us, 1), "speedup": round(ref_us / us, 1)}
        rows.append(r)
        print(f"{name:34s} {us:9.2f} us  {2 * nbytes / 1e6:7.1f} MB  {frac:5.3f} of 8 TB/s   "
              f"| {ref_label}: {ref_us:10.1f} us  ({ref_us / us:6.1f} x)", flush=True)

    # deltas, time-contiguous (B, 80, 1001)
    tc = rotation(lambda: torch.randn(B, Fm, Tn, device=dev), nbytes)
    us = timed(lambda x: F.compute_deltas(x), tc, a.iters, a.warmup)
    ref = timed(lambda x: ref_deltas(x), tc, max(a.iters // 5, 3), 2)
    report("deltas (256,80,1001) time-contig", us, ref, "pad+grouped conv1d (restated)")
    del tc
    # deltas, frame-major: real MelSpectrogram outputs
    mel = T.MelSpectrogram(16000, 400, hop_length=160, n_mels=Fm).to(dev)
    with torch.no_grad():
        fm = rotation(lambda: mel(torch.randn(B, 160000, device=dev) * 0.1), nbytes)
    assert fm[0].shape == (B, Fm, Tn) and fm[0].stride(-2) == 1
    us = timed(lambda x: F.compute_deltas(x), fm, a.iters, a.warmup)
    ref = timed(lambda x: ref_deltas(x), fm, max(a.iters // 5, 3), 2)
    report("deltas (256,80,1001) frame-major", us, ref, "pad+grouped conv1d (restated)")
    del fm
    # CMN (B, 1001, 80), default arguments
    cm = rotation(lambda: torch.randn(B, Tn, Fm, device=dev) + 5.0, nbytes)
    small = [x[:a.loop_batch] for x in cm[:2]]
    for nv in (False, True):
        us = timed(lambda x: F.sliding_window_cmn(x, norm_vars=nv), cm, a.iters, a.warmup)
        ref = timed(lambda x: ref_cmn(x, norm_vars=nv), small, 2, 1) * (B / a.loop_batch)
        report(f"cmn (256,1001,80) norm_vars={nv}", us, ref, f"per-frame loop on {a.loop_batch}, x{B // a.loop_batch} (restated)")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
