"""float64 restatements of CTC forced alignment for the tests of F.forced_align, independent of csrc/forced_align.h.

    viterbi(lp, target, blank)       the recurrence over the states 0 .. 2 L (even: blank, odd: target[i // 2]) with strict
                                     comparisons taken in the order stay, advance, skip (a tie keeps the smaller move), the final
                                     state 2 L if alpha[2 L] > alpha[2 L - 1] else 2 L - 1, and the walk back
    brute_force(lp, target, blank)   every frame-level labelling of a tiny case, those that collapse to the target kept
    path_total(lp, path)             the sum a labelling collects
    is_alignment(path, target, blank)  the labelling collapses to the target

lp is (T, C) float64; the caller rounds it to the dtype under test first."""
import itertools

import numpy as np


def collapse(path, blank):
    out, prev = [], None
    for p in path:
        p = int(p)
        if p != prev and p != blank:
            out.append(p)
        prev = p
    return out


def is_alignment(path, target, blank):
    return collapse(path, blank) == [int(v) for v in target]


def path_total(lp, path):
    return float(sum(float(lp[t, int(p)]) for t, p in enumerate(path)))


def repeats(target):
    return int(sum(1 for i in range(1, len(target)) if target[i] == target[i - 1]))


def viterbi(lp, target, blank=0):
    """(path (T,) int64, total) -- total is alpha of the final state, the float64 sum along the path in frame order."""
    lp = np.asarray(lp, dtype=np.float64)
    T = lp.shape[0]
    L = len(target)
    S = 2 * L + 1
    label = np.array([blank if i % 2 == 0 else int(target[i // 2]) for i in range(S)], dtype=np.int64)
    skip = np.zeros(S, dtype=bool)                            # state i may be entered from i - 2
    skip[3::2] = label[3::2] != label[1:-2:2]
    alpha = np.full(S, -np.inf)
    alpha[0] = lp[0, label[0]]
    if S > 1:
        alpha[1] = lp[0, label[1]]
    moves = np.zeros((T, S), dtype=np.int8)
    ninf = np.full(2, -np.inf)
    with np.errstate(invalid="ignore"):
        for t in range(1, T):                                 # every state of a step at once; the rule per state is the issue's
            x1 = np.concatenate((ninf[:1], alpha[:-1]))
            x2 = np.where(skip, np.concatenate((ninf, alpha[:-2]))[:S], -np.inf)
            m1 = x1 > alpha
            best = np.where(m1, x1, alpha)
            m2 = skip & (x2 > best)
            best = np.where(m2, x2, best)
            moves[t] = np.where(m2, 2, np.where(m1, 1, 0))
            alpha = best + lp[t, label]
    s = S - 1
    if L > 0 and not alpha[S - 1] > alpha[S - 2]:
        s = S - 2
    total = float(alpha[s])
    path = np.zeros(T, dtype=np.int64)
    for t in range(T - 1, -1, -1):
        path[t] = label[s]
        if t:
            s -= int(moves[t, s])
    return path, total


def brute_force(lp, target, blank=0):
    """The best total over every labelling that collapses to the target, and the labellings that reach it."""
    lp = np.asarray(lp, dtype=np.float64)
    T, C = lp.shape
    best, argbest = -np.inf, []
    for path in itertools.product(range(C), repeat=T):
        if not is_alignment(path, target, blank):
            continue
        total = path_total(lp, path)
        if total > best:
            best, argbest = total, [path]
        elif total == best:
            argbest.append(path)
    return best, argbest


def exact_lp(rng, T, C):
    """-k / 64 with integer k in [1, 255]: held exactly by float64, float32, float16 and bfloat16, every partial sum exact in
    float64, ties frequent."""
    return -rng.integers(1, 256, size=(T, C)).astype(np.float64) / 64.0


def random_target(rng, L, C, blank):
    """L labels without blank."""
    labels = [c for c in range(C) if c != blank]
    return rng.choice(labels, size=L).astype(np.int64) if L else np.zeros(0, dtype=np.int64)


def no_adjacent_repeats(rng, L, C, blank):
    """L labels without blank, no two neighbours equal (needs at least two labels besides blank)."""
    labels = [c for c in range(C) if c != blank]
    tg = np.zeros(L, dtype=np.int64)
    for i in range(L):
        tg[i] = rng.choice([c for c in labels if i == 0 or c != tg[i - 1]])
    return tg


def exact_case(seed, T, L, C, blank=0, runs=(), lens=None, no_repeats=False):
    """(lp (B, T, C) of exact_lp values, targets (B, L), input_lengths, target_lengths, blank); lens = (T_b, L_b) lists for a
    ragged batch, one full-length example otherwise.  T = None: exactly L + R frames, R the adjacent equal labels.  Every
    example can be aligned."""
    rng = np.random.default_rng(seed)
    B = 1 if lens is None else len(lens[0])
    targets = np.stack([no_adjacent_repeats(rng, L, C, blank) if no_repeats else random_target(rng, L, C, blank)
                        for _ in range(B)])
    for start, n in runs:
        targets[:, start:start + n] = targets[:, start:start + 1]
    if T is None:
        T = L + repeats(targets[0])
    in_len, tg_len = ([T], [L]) if lens is None else lens
    lp = np.stack([exact_lp(rng, T, C) for _ in range(B)])
    in_len, tg_len = np.asarray(in_len, dtype=np.int64), np.asarray(tg_len, dtype=np.int64)
    for b in range(B):
        assert in_len[b] >= tg_len[b] + repeats(targets[b, :tg_len[b]]), "the case cannot be aligned"
    return lp, targets, in_len, tg_len, blank


def expected(lp, targets, in_len, tg_len, blank):
    """(paths (B, T) with blank in the padding, totals (B,)) of viterbi per example."""
    B, T, _ = lp.shape
    paths, totals = np.full((B, T), blank, dtype=np.int64), np.zeros(B)
    for b in range(B):
        Tb, Lb = int(in_len[b]), int(tg_len[b])
        paths[b, :Tb], totals[b] = viterbi(lp[b, :Tb], targets[b, :Lb], blank)
    return paths, totals


def exact_shapes(configs, pf, bt, max_l):
    """name -> arguments of exact_case: the smallest shapes that cross each boundary of kernels with these constants
    (configs: (largest L, states per lane, lanes) per forward configuration; pf: prefetch depth; bt: backtrack block)."""
    shapes = {}
    for T in (1, 2):
        for L in (0, 1):
            shapes[f"T{T}_L{L}"] = dict(T=T, L=L, C=4)
    shapes["tight"] = dict(T=None, L=5, C=6, no_repeats=True)                    # T = L + R, no repeats: every move is a skip
    shapes["tight_run3"] = dict(T=None, L=6, C=6, no_repeats=True, runs=((2, 3),))                # three equal labels in a row
    shapes["tight_100"] = dict(T=None, L=100, C=8, no_repeats=True)            # the steepest descent the backtrack can meet
    shapes["tight_300"] = dict(T=None, L=300, C=8, no_repeats=True)
    for L in (63, 64):                                                        # 2 L + 1 crosses 128
        shapes[f"L{L}"] = dict(T=2 * L + 3, L=L, C=7)
    for last, _, _ in configs[:-1]:                                           # a change of states per lane or of the width
        for L in (last, last + 1):
            shapes[f"L{L}"] = dict(T=2 * L + 3, L=L, C=9)
    for T in (pf - 1, pf, pf + 1):
        shapes[f"T{T}_pf"] = dict(T=T, L=2, C=4)
    for T in (bt - 1, bt, bt + 1, 2 * bt + 1):
        shapes[f"T{T}_bt"] = dict(T=T, L=10, C=5)
    shapes["C2"] = dict(T=9, L=3, C=2)                                        # one label: every neighbour is a repeat
    shapes["C5_blank4"] = dict(T=12, L=5, C=5, blank=4)
    shapes["ragged"] = dict(T=20, L=6, C=6, lens=([20, 7, 1], [6, 2, 0]))
    shapes["T700_L300"] = dict(T=700, L=300, C=32)
    shapes["largest"] = dict(T=2 * max_l + 40, L=max_l, C=8)
    return shapes
