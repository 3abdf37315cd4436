#!/usr/bin/env python
"""Device time of F.rnnt_loss, forward and forward + backward, on a 32 x 300 x 100 x 1024 float32 joiner output and on a
character vocabulary (V = 29), beside the reference's composition restated in plain torch on the same device.

Inputs rotate over enough sets that together they exceed twice the 256 MiB Infinity Cache (one 3.9 GB tensor does by itself;
two sets are kept so that no call sees the buffer it has just written).  Time = device events around `--iters` calls after
`--warmup`, divided by the calls; `--rounds` such measurements per case, kernel and restatement alternating, median and
minimum reported.  Roofline bytes are what the design needs when the batch is not ragged: one read of logits forward, one
more read and one write of the gradient backward -- three times the bytes of logits for a training step.  The fraction is
of 8 TB/s.

Restatement (labelled as such; torchaudio is not needed and the code under test is not used): log_softmax, two gathers, the
alpha recurrence one anti-diagonal at a time over skewed (batch, diagonal, u) views, everything under torch autograd."""
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
NEG = -1e30          # "no path": finite, so that autograd through logaddexp of two such values stays finite


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


def ref_rnnt_loss(logits, targets, logit_lengths, target_lengths, blank):
    """Restatement of the transducer loss as a torch composition: mean over the batch of -log P(targets | logits)."""
    B, T, U1, V = logits.shape
    lp = torch.log_softmax(logits, -1)
    lpb = lp[..., blank]                                                            # (B, T, U1)
    lpt = lp[:, :, :U1 - 1].gather(-1, targets.long()[:, None, :, None].expand(B, T, U1 - 1, 1)).squeeze(-1)
    lpt = torch.nn.functional.pad(lpt, (0, 1), value=NEG)                           # (B, T, U1): no label leaves u = U
    D = T + U1 - 1
    d = torch.arange(D, device=logits.device)[:, None]
    u = torch.arange(U1, device=logits.device)[None, :]
    t = d - u                                                                       # (D, U1): the frame of cell u on diagonal d
    valid = (t >= 0) & (t < T)
    tidx = t.clamp(0, T - 1)[None].expand(B, D, U1)
    neg = torch.full((), NEG, device=logits.device, dtype=logits.dtype)
    sb = torch.where(valid[None], lpb.gather(1, tidx), neg)                         # sb[b][d][u] = lpb[b][d - u][u]
    st = torch.where(valid[None], lpt.gather(1, tidx), neg)
    alpha = [torch.where(u[0] == 0, torch.zeros((), device=logits.device, dtype=logits.dtype), neg).expand(B, U1)]
    for k in range(1, D):
        prev = alpha[-1]
        by_label = torch.nn.functional.pad((prev + st[:, k - 1])[:, :-1], (1, 0), value=NEG)
        alpha.append(torch.logaddexp(prev + sb[:, k - 1], by_label))
    alpha = torch.stack(alpha, 1)                                                   # (B, D, U1), skewed
    bi = torch.arange(B, device=logits.device)
    tb, ub = logit_lengths.long() - 1, target_lengths.long()
    return -(alpha[bi, tb + ub, ub] + lpb[bi, tb, ub]).mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--time", type=int, default=300)
    ap.add_argument("--targets", type=int, default=99, help="U; logits have U + 1 = 100 rows along the target axis")
    ap.add_argument("--vocab", type=int, nargs="+", default=[1024, 29])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-reference", action="store_true", help="skip the restated composition (it keeps several tensors of the size of logits)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_rnnt_loss: no GPU; a timing from a CPU says nothing about these kernels")
    dev = "cuda"
    B, T, U = args.batch, args.time, args.targets
    g = torch.Generator(device=dev).manual_seed(0)
    for V in args.vocab:
        nbytes = B * T * (U + 1) * V * 4
        n_sets = max(2, -(-2 * MALL // nbytes) + 1)
        targets = torch.randint(0, V - 1, (B, U), device=dev, generator=g, dtype=torch.int32)
        ll = torch.full((B,), T, device=dev, dtype=torch.int32)
        tl = torch.full((B,), U, device=dev, dtype=torch.int32)
        sets = [(torch.randn(B, T, U + 1, V, device=dev, generator=g).requires_grad_(True),) for _ in range(n_sets)]

        def fwd(x):
            with torch.no_grad():
                return F.rnnt_loss(x, targets, ll, tl)

        def fwd_bwd(x):
            x.grad = None
            F.rnnt_loss(x, targets, ll, tl).backward()

        def ref_fwd(x):
            with torch.no_grad():
                return ref_rnnt_loss(x, targets, ll, tl, V - 1)

        def ref_fwd_bwd(x):
            x.grad = None
            ref_rnnt_loss(x, targets, ll, tl, V - 1).backward()

        # the two agree before either is timed
        a, b = float(fwd(sets[0][0])), float(ref_fwd(sets[0][0]))
        assert abs(a - b) <= 1e-3 * abs(b), (a, b)
        for name, ours, ref, passes in (("forward", fwd, ref_fwd, 1), ("forward_backward", fwd_bwd, ref_fwd_bwd, 3)):
            t_ours, t_ref = [], []
            for _ in range(args.rounds):
                t_ours.append(timed(ours, sets, args.iters, args.warmup))
                if not args.no_reference:
                    t_ref.append(timed(ref, sets, max(args.iters // 4, 1), 1))
            line = {"case": "rnnt_loss_" + name, "shape": [B, T, U + 1, V], "dtype": "float32", "input_sets": n_sets,
                    "us_median": statistics.median(t_ours), "us_min": min(t_ours), "roofline_bytes": passes * nbytes,
                    "fraction_of_8TBps": passes * nbytes / (min(t_ours) * 1e-6) / PEAK}
            if t_ref:
                line["restated_reference_us_median"] = statistics.median(t_ref)
                line["speedup_vs_restated_reference"] = statistics.median(t_ref) / statistics.median(t_ours)
            print(json.dumps(line), flush=True)
        del sets


if __name__ == "__main__":
    main()
