#!/usr/bin/env python
"""Device time of F.overdrive, F.phaser and F.flanger on a (256, 160000) float32 batch (256 utterances of 10 s at 16 kHz),
beside the reference's per-sample loops restated in plain torch on the same device.

The restated loops launch several kernels per sample, so they are timed on the first `--ref-samples` samples (2 000) of the
same batch and scaled to the full length; the line says so.  Each kernel case rotates over enough inputs that together they
exceed twice the 256 MiB Infinity Cache.  Time = device events around `--iters` calls after `--warmup`, divided by the
calls; `--rounds` such measurements per case, median and minimum reported.  The flanger's default route (regen = 0, a
streaming gather) is also set against its copy floor: `out.copy_(x)` on the same tensors, one read and one write.

Restatements (labelled as such; torchaudio is not needed and the code under test is not used)."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import audio_amd.functional as F  # noqa: E402
from audio_amd import _host  # noqa: E402

MALL = 256 << 20


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


def ref_overdrive(x, gain=20.0, colour=20.0):
    """Restatement of the reference's overdrive (_overdrive_core_loop_generic)."""
    g = math.exp(gain * math.log(10) / 20.0)
    temp = x * g + colour / 200
    mask1, mask2 = temp < -1, temp > 1
    temp = torch.where(mask1, torch.tensor(-2.0 / 3, device=x.device), torch.where(mask2, torch.tensor(2.0 / 3, device=x.device),
                                                                                   temp - temp ** 3 * (1.0 / 3)))
    out = torch.zeros_like(x)
    last_in = torch.zeros(x.shape[:-1], device=x.device)
    last_out = torch.zeros(x.shape[:-1], device=x.device)
    for i in range(x.shape[-1]):
        last_out = temp[:, i] - last_in + 0.995 * last_out
        last_in = temp[:, i]
        out[:, i] = x[:, i] * 0.5 + last_out * 0.75
    return out.clamp(-1, 1)


def ref_phaser(x, sr, gain_in=0.4, gain_out=0.74, delay_ms=3.0, decay=0.4, mod_speed=0.5):
    """Restatement of the reference's phaser loop (table from the host)."""
    L, M = int(delay_ms * 0.001 * sr + 0.5), int(sr / mod_speed + 0.5)
    mod = _host.effects_wave_table("SINE", "INT", M, 1.0, float(L), math.pi / 2).tolist()
    buf = torch.zeros(x.shape[0], L, device=x.device)
    outs = []
    delay_pos = mod_pos = 0
    for i in range(x.shape[-1]):
        idx = (delay_pos + mod[mod_pos]) % L
        mod_pos = (mod_pos + 1) % M
        delay_pos = (delay_pos + 1) % L
        temp = x[:, i] * gain_in + buf[:, idx] * decay
        buf[:, delay_pos] = temp
        outs.append(temp)
    return (torch.stack(outs, dim=-1) * gain_out).clamp(-1, 1)


def ref_flanger(x, sr, delay=0.0, depth=2.0, regen=0.0, width=71.0, speed=0.5):
    """Restatement of the reference's flanger loop, one channel, linear interpolation (table from the host)."""
    fg, dg = regen / 100, width / 100
    ig = 1.0 / (1 + dg)
    dg = dg / (1 + dg) * (1 - abs(fg))
    L = int((delay / 1000 + depth / 1000) * sr + 0.5) + 2
    N = int(sr / speed)
    lfo = _host.effects_wave_table("SINE", "FLOAT", N, float(math.floor(delay / 1000 * sr + 0.5)), L - 2.0, 3 * math.pi / 2).tolist()
    bufs = torch.zeros(x.shape[0], L, device=x.device)
    last = torch.zeros(x.shape[0], device=x.device)
    outs = []
    pos = 0
    for i in range(x.shape[-1]):
        pos = (pos + L - 1) % L
        d = lfo[i % N]
        k, fr = int(d), d - int(d)
        bufs[:, pos] = x[:, i] + last * fg
        d0, d1 = bufs[:, (pos + k) % L], bufs[:, (pos + k + 1) % L]
        last = d0 + (d1 - d0) * fr
        outs.append(x[:, i] * ig + last * dg)
    return torch.stack(outs, dim=-1).clamp(-1, 1)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--length", type=int, default=160000)
    ap.add_argument("--sample-rate", type=int, default=16000)
    ap.add_argument("--ref-samples", type=int, default=2000)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default=None, help="also write the results here")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_effects measures the device: no GPU, no number"
    dev = torch.device("cuda")
    B, L, sr = a.batch, a.length, a.sample_rate
    rowset = B * L * 4
    n_sets = max(2, -(-2 * MALL // rowset) + 1)
    sets = [0.3 * torch.randn(B, L, device=dev) for _ in range(n_sets)]
    out = torch.empty(B, L, device=dev)
    short = [s[:, :a.ref_samples].contiguous() for s in sets[:2]]
    scale = L / a.ref_samples
    cases = [
        ("overdrive", lambda x: F.overdrive(x), lambda x: ref_overdrive(x)),
        ("phaser", lambda x: F.phaser(x, sr), lambda x: ref_phaser(x, sr)),
        ("flanger regen=0 (streaming gather)", lambda x: F.flanger(x.unsqueeze(1), sr), lambda x: ref_flanger(x, sr)),
        ("flanger regen=50 (delay-line kernel)", lambda x: F.flanger(x.unsqueeze(1), sr, regen=50.0),
         lambda x: ref_flanger(x, sr, regen=50.0)),
    ]
    rows = []
    for name, ours, ref in cases:
        t = [timed(ours, sets, a.iters, a.warmup) for _ in range(a.rounds)]
        r = timed(ref, short, 1, 1) * scale
        row = {"case": name, "shape": [B, L], "us_median": statistics.median(t), "us_min": min(t),
               "restated_loop_us_scaled": r, "restated_loop_samples": a.ref_samples}
        rows.append(row)
        print("%-40s %10.1f us (min %10.1f)   restated loop on %d samples, scaled to %d: %12.0f us   x%.0f" %
              (name, row["us_median"], row["us_min"], a.ref_samples, L, r, r / row["us_median"]))
    t = [timed(lambda x: out.copy_(x), sets, a.iters, a.warmup) for _ in range(a.rounds)]
    floor = {"case": "copy floor of the streaming flanger (out.copy_(x))", "us_median": statistics.median(t), "us_min": min(t)}
    rows.append(floor)
    print("%-40s %10.1f us (min %10.1f)   streaming flanger / floor: %.2f" %
          ("copy floor (out.copy_(x))", floor["us_median"], floor["us_min"], rows[2]["us_median"] / floor["us_median"]))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
