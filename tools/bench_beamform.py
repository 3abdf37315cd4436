#!/usr/bin/env python
"""Device time of T.PSD, F.mvdr_weights_souden, F.apply_beamforming and T.MVDR on a 32 x 8 channel x 257 x 1001 complex64
spectrogram (frame-major, as T.Spectrogram(power=None) returns it), beside the reference's compositions restated in plain
torch on the same device.

The streaming cases rotate over enough input sets that together they exceed twice the 256 MiB Infinity Cache, so every call
streams its inputs from HBM.  Time = device events around `--iters` calls after `--warmup`, divided by the calls; `--rounds`
such measurements per case, kernel and restatement alternating, median and minimum reported.  Roofline bytes are what the
algorithm needs: psd reads the spectrogram and the mask and writes the matrices, apply reads the spectrogram and writes one
channel.  The fraction is of 8 TB/s.

Restatements (labelled as such; torchaudio is not needed and the code under test is not used): psd = einsum over a
(..., time, ch, ch) product; Souden weights = torch.linalg.solve, a trace and a column; apply = einsum."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import audio_amd.functional as F  # noqa: E402
import audio_amd.transforms as T  # noqa: E402

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


def ref_psd(specgram, mask, normalize=True, eps=1e-15):
    """Restatement of the reference's psd."""
    specgram = specgram.transpose(-3, -2)
    psd = torch.einsum("...ct,...et->...tce", [specgram, specgram.conj()])
    if normalize:
        mask = mask / (mask.sum(dim=-1, keepdim=True) + eps)
    return (psd * mask[..., None, None]).sum(dim=-3)


def ref_souden(psd_s, psd_n, ref, diag_eps=1e-7, eps=1e-8):
    """Restatement of the reference's mvdr_weights_souden."""
    tr = torch.diagonal(psd_n, dim1=-1, dim2=-2).sum(-1).real
    psd_n = psd_n + (tr * diag_eps + 1e-8)[..., None, None] * torch.eye(psd_n.shape[-1], dtype=psd_n.dtype, device=psd_n.device)
    numerator = torch.linalg.solve(psd_n, psd_s)
    ws = numerator / (torch.diagonal(numerator, dim1=-1, dim2=-2).sum(-1)[..., None, None] + eps)
    return ws[..., :, ref]


def ref_apply(w, specgram):
    """Restatement of the reference's apply_beamforming."""
    return torch.einsum("...fc,...cft->...ft", [w.conj(), specgram])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--channels", type=int, default=8)
    ap.add_argument("--freq", type=int, default=257)
    ap.add_argument("--time", type=int, default=1001)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-reference", action="store_true", help="skip the restated compositions (the psd one needs 4 GB)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_beamform: no GPU; a timing from a CPU says nothing about these kernels")
    dev = "cuda"
    B, Cc, Fq, Tt = args.batch, args.channels, args.freq, args.time
    spec_bytes = B * Cc * Fq * Tt * 8
    n_sets = max(2, -(-2 * MALL // spec_bytes) + 1)
    g = torch.Generator(device=dev).manual_seed(0)
    specs = [torch.view_as_complex(torch.randn(B, Cc, Tt, Fq, 2, device=dev, generator=g)).transpose(-1, -2) for _ in range(n_sets)]
    masks = [torch.rand(B, Fq, Tt, device=dev, generator=g) * 0.95 + 0.05 for _ in range(n_sets)]
    psd_s, psd_n = F.psd(specs[0], masks[0]), F.psd(specs[0], 1.05 - masks[0])
    w = F.mvdr_weights_souden(psd_s, psd_n, 0)
    psd_mod, mvdr = T.PSD(), T.MVDR()
    out_bytes = B * Fq * Tt * 8
    cases = [
        ("psd", lambda x, m: psd_mod(x, m), ref_psd, list(zip(specs, masks)), spec_bytes + B * Fq * Tt * 4 + B * Fq * Cc * Cc * 8),
        ("mvdr_weights_souden", lambda s, n: F.mvdr_weights_souden(s, n, 0), lambda s, n: ref_souden(s, n, 0), [(psd_s, psd_n)],
         2 * B * Fq * Cc * Cc * 8 + B * Fq * Cc * 8),
        ("apply_beamforming", lambda x, m: F.apply_beamforming(w, x), lambda x, m: ref_apply(w, x), list(zip(specs, masks)),
         spec_bytes + out_bytes),
        ("MVDR", lambda x, m: mvdr(x, m, 1.05 - m), None, list(zip(specs, masks)), None),
    ]
    for name, ours, ref, sets, nbytes in cases:
        t_ours, t_ref = [], []
        for _ in range(args.rounds):
            t_ours.append(timed(ours, sets, args.iters, args.warmup))
            if ref is not None and not args.no_reference:
                t_ref.append(timed(ref, sets, max(args.iters // 4, 1), 1))
        line = {"case": name, "shape": [B, Cc, Fq, Tt], "dtype": "complex64", "layout": "frame-major", "input_sets": len(sets),
                "us_median": statistics.median(t_ours), "us_min": min(t_ours)}
        if nbytes is not None:
            line["roofline_bytes"] = nbytes
            line["fraction_of_8TBps"] = nbytes / (min(t_ours) * 1e-6) / PEAK
        if t_ref:
            line["restated_reference_us_median"] = statistics.median(t_ref)
            line["speedup_vs_restated_reference"] = statistics.median(t_ref) / statistics.median(t_ours)
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
