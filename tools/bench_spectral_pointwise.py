#!/usr/bin/env python
"""Device time of the pointwise waveform ops (gain, Vol, contrast, DB_to_amplitude, mu-law encoding and decoding, Fade), of
F.spectral_centroid and of T.LFCC on the (256, 160000) float32 batch, beside the reference's composition restated in plain
torch on the same device and beside torch.clone of the same tensor.

Protocol (that of tools/bench_feat_post.py): every case rotates over enough inputs that together they exceed twice the
256 MiB Infinity Cache; time = device events around `--iters` calls after `--warmup`, divided by the calls; `--rounds` rounds
in which the kernel, the restatement and the copy alternate; median and minimum reported.  The roofline figure is the op's
input plus output bytes at 8 TB/s over the kernel's time.  spectral_centroid is reported as a whole and as its two launches
(the magnitude spectrogram, the reduction over spectrograms that rotate the same way), with the bytes a fused epilogue would
not move.

Restatements (labelled as such; torchaudio is not needed and the code under test is not used by them, except that the
centroid's restatement starts from the product's own spectrogram)."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import audio_amd.functional as F  # noqa: E402
import audio_amd.transforms as T  # noqa: E402

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


def ref_contrast(x, amount=75.0):
    t = x * (math.pi / 2)
    return torch.sin(t + (amount / 750.0) * torch.sin(t * 4))


def ref_db_to_amplitude(x, ref=1.0, power=0.5):
    return ref * torch.pow(torch.pow(10.0, 0.1 * x), power)


def ref_mu_encode(x, q=256):
    mu = torch.tensor(q - 1.0, dtype=x.dtype, device=x.device)
    v = torch.sign(x) * torch.log1p(mu * torch.abs(x)) / torch.log1p(mu)
    return ((v + 1) / 2 * mu + 0.5).to(torch.int64)


def ref_mu_decode(c, q=256):
    c = c.to(torch.float)
    mu = torch.tensor(q - 1.0, dtype=c.dtype, device=c.device)
    y = (c / mu) * 2 - 1.0
    return torch.sign(y) * (torch.exp(torch.abs(y) * torch.log1p(mu)) - 1.0) / mu


def ref_fade(x, n_in=8000, n_out=16000):
    """T.Fade.forward with half_sine ramps, as the reference builds them on every call."""
    n = x.shape[-1]
    fi = torch.linspace(0, 1, n_in, device=x.device)
    fi = torch.cat((torch.sin(fi * math.pi - math.pi / 2) / 2 + 0.5, torch.ones(n - n_in, device=x.device))).clamp(0, 1)
    fo = torch.linspace(0, 1, n_out, device=x.device)
    fo = torch.cat((torch.ones(n - n_out, device=x.device), torch.sin(fo * math.pi + math.pi / 2) / 2 + 0.5)).clamp(0, 1)
    return (fi * fo) * x


def ref_centroid_tail(spec, freqs):
    return (freqs * spec).sum(dim=-2) / spec.sum(dim=-2)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--length", type=int, default=160000)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None, help="also write the results here")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_spectral_pointwise measures the device: no GPU, no number"
    dev = torch.device("cuda")
    B, L = a.rows, a.length
    n_sets = max(2, -(-2 * MALL // (B * L * 4)) + 1)
    waves = [torch.rand(B, L, device=dev) * 2 - 1 for _ in range(n_sets)]
    fade = T.Fade(8000, 16000, "half_sine")
    vol = T.Vol(0.7)
    cases = [
        ("gain", lambda x: F.gain(x, -3.0), lambda x: x * (10 ** (-3.0 / 20)), waves, 4, 4),
        ("Vol", vol, lambda x: torch.clamp(x * 0.7, -1, 1), waves, 4, 4),
        ("contrast", F.contrast, ref_contrast, waves, 4, 4),
        ("DB_to_amplitude", lambda x: F.DB_to_amplitude(x, 1.0, 0.5), ref_db_to_amplitude, waves, 4, 4),
        ("mu_law_encoding", lambda x: F.mu_law_encoding(x, 256), ref_mu_encode, waves, 4, 8),
        ("Fade", fade, ref_fade, waves, 4, 4),
    ]
    rows_out = []

    def report(name, fn, ref, sets, bytes_moved, copy=True):
        k, r, c = [], [], []
        for _ in range(a.rounds):                    # the three alternate within a round
            k.append(timed(fn, sets, a.iters, a.warmup))
            r.append(timed(ref, sets, a.iters, a.warmup))
            if copy:
                c.append(timed(torch.clone, sets, a.iters, a.warmup))
        floor = bytes_moved / HBM_BYTES_PER_US
        row = {"case": name, "shape": list(sets[0].shape), "dtype": str(sets[0].dtype), "us_median": statistics.median(k),
               "us_min": min(k), "torch_restatement_us_median": statistics.median(r), "torch_restatement_us_min": min(r),
               "clone_us_median": statistics.median(c) if c else None, "bytes": bytes_moved,
               "roofline_fraction_at_8TBps": floor / statistics.median(k),
               "ratio_to_clone": statistics.median(k) / statistics.median(c) if c else None}
        rows_out.append(row)
        print("%-34s %9.1f us (min %9.1f)  torch restatement %9.1f us (x%5.2f)  clone %s  %.3f of 8 TB/s on %d MB" %
              (name, row["us_median"], row["us_min"], row["torch_restatement_us_median"],
               row["torch_restatement_us_median"] / row["us_median"],
               "%9.1f us (x%4.2f)" % (row["clone_us_median"], row["ratio_to_clone"]) if c else "    --", row["roofline_fraction_at_8TBps"],
               bytes_moved >> 20))
        return row

    for name, fn, ref, sets, b_in, b_out in cases:
        report(name, fn, ref, sets, B * L * (b_in + b_out))
    codes = [F.mu_law_encoding(w, 256) for w in waves]
    report("mu_law_decoding (int64 codes)", lambda c: F.mu_law_decoding(c, 256), ref_mu_decode, codes, B * L * (8 + 4))
    del codes
    small = [c.to(torch.uint8) for c in (F.mu_law_encoding(w, 256) for w in waves)]
    report("mu_law_decoding (uint8 codes)", lambda c: F.mu_law_decoding(c, 256), ref_mu_decode, small, B * L * (1 + 4))
    del small
    halves = [w.half() for w in waves]
    report("contrast (float16)", F.contrast, ref_contrast, halves, B * L * 4)
    report("Vol (float16)", vol, lambda x: torch.clamp(x * 0.7, -1, 1), halves, B * L * 4)
    del halves
    torch.cuda.empty_cache()

    # spectral centroid: the whole call, then its two launches
    for n_fft in (400, 512, 480):
        hop = n_fft // 2
        m = T.SpectralCentroid(16000, n_fft=n_fft).to(dev)
        spec_m = T.Spectrogram(n_fft=n_fft, power=1.0).to(dev)
        freqs = torch.linspace(0, 8000, n_fft // 2 + 1, device=dev)
        col = freqs.reshape(-1, 1)
        n_freq, frames = n_fft // 2 + 1, 1 + L // hop
        spec_bytes = B * frames * n_freq * 4
        whole = report("spectral_centroid n_fft=%d" % n_fft, m, lambda x: ref_centroid_tail(spec_m(x), col), waves,
                       B * L * 4 + B * frames * 4, copy=False)
        first = report("  magnitude spectrogram", spec_m, spec_m, waves, B * L * 4 + spec_bytes, copy=False)
        specs = [spec_m(w) for w in waves[:max(2, -(-2 * MALL // spec_bytes) + 1)]]
        second = report("  centroid reduction", lambda s: F._centroid_reduce(s, freqs), lambda s: ref_centroid_tail(s, col), specs,
                        spec_bytes + B * frames * 4)
        whole["spectrogram_bytes_a_fused_epilogue_would_not_move"] = 2 * spec_bytes
        whole["launch_us_median"] = {"spectrogram": first["us_median"], "reduction": second["us_median"]}
        del specs
        torch.cuda.empty_cache()

    # LFCC: the exact two-kernel MFCC path with the linear filterbank, beside MFCC's own two-kernel path on the same batch
    lfcc = T.LFCC().to(dev)
    mfcc = T.MFCC(melkwargs=dict(n_mels=128)).to(dev)
    mfcc.fused = False
    n_frames = 1 + L // 200
    report("LFCC (128 filters, 40 coefficients)", lfcc, mfcc, waves, B * L * 4 + B * n_frames * 40 * 4, copy=False)
    rows_out[-1]["torch_restatement_is"] = "T.MFCC(n_mels=128, fused=False): the same two kernels with the mel filterbank"
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows_out, f, indent=1)


if __name__ == "__main__":
    main()
