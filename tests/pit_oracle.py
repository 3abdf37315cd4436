"""Permutation-invariant training restated in numpy: the pairwise matrix through tests/sdr_oracle.py, the assignment by brute
force (the contract of F.pit_assignment, tie rule included), and the seeded mixtures the tests share."""
import functools
import itertools

import numpy as np

import sdr_oracle as O

METRICS = {"si_sdr": O.si_sdr, "si_snr": O.si_sdr, "snr": O.snr}


def matrix(preds, target, name, zero_mean=False, dtype=np.float64, eps=np.finfo(np.float32).eps):
    """M[i][j]: the metric of preds[i] against target[j]; si_snr is si_sdr with zero_mean."""
    zm = True if name == "si_snr" else zero_mean
    return np.array([[METRICS[name](p, t, zm, dtype, eps) for t in target] for p in preds], np.float64)


def total(M, perm):
    """The right-nested float64 sum M[0][perm[0]] + (M[1][perm[1]] + (...))."""
    t = np.float64(M[len(perm) - 1][perm[-1]])
    for i in range(len(perm) - 2, -1, -1):
        t = np.float64(M[i][perm[i]]) + t
    return t


def assign(M, eval_func="max"):
    """(best total / S, permutation): permutations in lexicographic order under a strict comparison, so the first of equal
    totals stays."""
    best, best_perm = None, None
    for perm in itertools.permutations(range(len(M))):
        t = total(M, perm)
        if best is None or (t > best if eval_func == "max" else t < best):
            best, best_perm = t, perm
    return best / len(M), np.array(best_perm)


def margin(M, eval_func="max"):
    """The gap between the best and the second-best distinct totals; inf with one permutation."""
    ts = sorted({float(total(M, p)) for p in itertools.permutations(range(len(M)))}, reverse=eval_func == "max")
    return abs(ts[0] - ts[1]) if len(ts) > 1 else float("inf")


@functools.lru_cache(None)
def mixtures(S, time, seed=0):
    """(preds, target, planted), float64 (S, time): the targets are rows of sdr_oracle.signals under different seeds; preds[i]
    is target[planted[i]] plus white noise 10 dB below it, planted a seeded permutation other than the identity (S > 1)."""
    rng = np.random.default_rng(1000 * seed + S)
    target = np.stack([O.signals(time, 100 * seed + s)[1][s % 3] for s in range(S)])
    planted = rng.permutation(S)
    while S > 1 and (planted == np.arange(S)).all():
        planted = rng.permutation(S)
    clean = target[planted]
    noise = rng.standard_normal((S, time)) * np.sqrt(np.mean(clean * clean, axis=1, keepdims=True) + 1e-30) * 10 ** -0.5
    return clean + noise, target, planted


def mix_cases(span):
    """(S, time, seed) of every mixture the GPU tests assign: one sample past the Gram span, and a length no other test uses
    for the captured call."""
    return [(S, span + 1, seed) for S in (2, 3, 8) for seed in range(3)] + [(3, span + 69, seed) for seed in range(3)]
