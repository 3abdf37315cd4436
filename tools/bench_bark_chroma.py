#!/usr/bin/env python
"""Device time of the dense filterbank projection (csrc/dense_fbank.h) behind T.ChromaScale, of T.ChromaSpectrogram end to
end and of T.BarkSpectrogram beside T.MelSpectrogram, float32, at two shapes:

    (256, 160000), n_fft 400, hop 200    the ASR front-end's batch: a (256, 201, 801) spectrogram, 165 MB
    (32, 441000), n_fft 2048, hop 512    ten seconds of 44.1 kHz music: a (32, 1025, 862) spectrogram, 113 MB

ChromaScale runs on the frame-major spectrogram the Spectrogram module returns, beside
``torch.matmul(spec.transpose(-1, -2), fb)`` restated in plain torch on the same tensors.  Each case rotates over enough
input buffers that together they exceed twice the 256 MiB Infinity Cache, so every call streams its input from HBM.  Both
sides are timed by ONE protocol: `--rounds` alternating rounds (kernel, restatement, kernel, ...), each round device events
around `--iters` calls after `--warmup` calls, divided by the calls; the figure is the median over the rounds, and the rounds'
extremes are kept in the JSON.  The projection is bound by the one read of the spectrogram: its roofline is the
spectrogram's bytes at 8 TB/s (21 us for the first shape)."""
import argparse
import json
import os
import statistics
import sys
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import audio_amd.transforms as T  # noqa: E402

PEAK_BYTES = 8.0e12
MALL = 256 << 20
CASES = [("asr", 256, 160000, 16000, 400, 200), ("music", 32, 441000, 44100, 2048, 512)]


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


def alternating(ours_fn, theirs_fn, bufs, a):
    ours, theirs = [], []
    for _ in range(a.rounds):
        ours.append(timed(ours_fn, bufs, a.iters, a.warmup))
        theirs.append(timed(theirs_fn, bufs, a.iters, a.warmup))
    return ours, theirs


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None, help="also write the results here")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_bark_chroma measures the device: no GPU, no number"
    dev = torch.device("cuda")
    rows = []
    for name, B, L, sr, n_fft, hop in CASES:
        spec_mod = T.Spectrogram(n_fft, hop_length=hop).to(dev)
        chroma = T.ChromaSpectrogram(sr, n_fft, hop_length=hop).to(dev)
        scale, fb = chroma.chroma_scale, chroma.chroma_scale.fb
        K, Tn = n_fft // 2 + 1, 1 + L // hop
        # ---- ChromaScale alone on the frame-major spectrogram
        nbytes = B * K * Tn * 4
        specs = rotation(lambda: spec_mod(torch.randn(B, L, device=dev)), nbytes)
        assert specs[0].shape == (B, K, Tn) and specs[0].stride(-2) == 1
        ours, theirs = alternating(lambda s: scale(s), lambda s: torch.matmul(s.transpose(-1, -2), fb), specs, a)
        us, ref = statistics.median(ours), statistics.median(theirs)
        got, want = scale(specs[0]), torch.matmul(specs[0].transpose(-1, -2), fb).transpose(-1, -2)
        floor = nbytes / PEAK_BYTES * 1e6
        r = {"case": f"ChromaScale {name} ({B},{K},{Tn})->12 frame-major", "us": round(us, 2), "roofline_us": round(floor, 1),
             "frac_of_roofline": round(floor / us, 3), "restated_reference": "matmul(spec^T, fb) (restated)",
             "restated_us": round(ref, 1), "speedup": round(ref / us, 2), "rounds_us": [round(min(ours), 2), round(max(ours), 2)],
             "restated_rounds_us": [round(min(theirs), 1), round(max(theirs), 1)],
             "max_rel_diff_vs_restated": float((got - want).abs().max() / want.abs().max())}
        rows.append(r)
        print(f"{r['case']:56s} {us:9.2f} us  {r['frac_of_roofline']:5.3f} of the roofline ({r['roofline_us']} us)   | "
              f"matmul restated: {ref:9.1f} us ({ref / us:5.2f} x)", flush=True)
        del specs, got, want
        torch.cuda.empty_cache()
        # ---- ChromaSpectrogram end to end, beside Spectrogram + the restated matmul; BarkSpectrogram beside MelSpectrogram
        waves = rotation(lambda: torch.randn(B, L, device=dev), B * L * 4)
        ours, theirs = alternating(lambda w: chroma(w), lambda w: torch.matmul(spec_mod(w).transpose(-1, -2), fb), waves, a)
        us, ref = statistics.median(ours), statistics.median(theirs)
        r = {"case": f"ChromaSpectrogram {name} ({B},{L}) n_fft {n_fft} hop {hop}", "us": round(us, 2),
             "restated_reference": "matmul(Spectrogram(x)^T, fb) (Spectrogram is this package's)", "restated_us": round(ref, 1),
             "speedup": round(ref / us, 2), "rounds_us": [round(min(ours), 2), round(max(ours), 2)],
             "restated_rounds_us": [round(min(theirs), 1), round(max(theirs), 1)]}
        rows.append(r)
        print(f"{r['case']:56s} {us:9.2f} us   | Spectrogram + matmul restated: {ref:9.1f} us ({ref / us:5.2f} x)", flush=True)
        n_bands = 128 if n_fft >= 2048 else 40                # (128 Bark bands need more than 201 bins: no all-zero filter)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            bark = T.BarkSpectrogram(sr, n_fft, hop_length=hop, n_barks=n_bands).to(dev)
            mel = T.MelSpectrogram(sr, n_fft, hop_length=hop, n_mels=n_bands).to(dev)
        ours, theirs = alternating(lambda w: bark(w), lambda w: mel(w), waves, a)
        us, ref = statistics.median(ours), statistics.median(theirs)
        r = {"case": f"BarkSpectrogram {name} ({B},{L}) n_fft {n_fft} hop {hop} {n_bands} bands", "us": round(us, 2),
             "restated_reference": "MelSpectrogram of the same shape (this package's)", "restated_us": round(ref, 1),
             "speedup": round(ref / us, 2), "rounds_us": [round(min(ours), 2), round(max(ours), 2)],
             "restated_rounds_us": [round(min(theirs), 1), round(max(theirs), 1)]}
        rows.append(r)
        print(f"{r['case']:56s} {us:9.2f} us   | MelSpectrogram: {ref:9.1f} us ({ref / us:5.2f} x)", flush=True)
        del waves
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
