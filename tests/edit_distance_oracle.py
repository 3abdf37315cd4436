"""The definition of F.edit_distance_batch restated in pure Python, a plain ``min`` DP for the distance alone, and the builders of
the cases the CPU replay and the GPU tests share.

Cell (i, j) of a reference r[0..M) and a hypothesis h[0..N) holds (cost, S, D, I): (0, j) = (j, 0, 0, j), (i, 0) = (i, 0, i, 0),
and for i, j >= 1 the first of diagonal (i-1, j-1) + (sub, sub, 0, 0), deletion (i-1, j) + (1, 0, 1, 0), insertion (i, j-1) +
(1, 0, 0, 1) whose cost is smallest.  The result is cell (M, N)."""
import functools
import itertools
import random

import numpy as np


def ops(ref, hyp):
    """(cost, S, D, I) of the tie-ruled DP."""
    M, N = len(ref), len(hyp)
    prev = [(j, 0, 0, j) for j in range(N + 1)]
    for i in range(1, M + 1):
        cur = [(i, 0, i, 0)]
        ri = ref[i - 1]
        for j in range(1, N + 1):
            sub = int(ri != hyp[j - 1])
            d, u, l = prev[j - 1], prev[j], cur[j - 1]
            best = (d[0] + sub, d[1] + sub, d[2], d[3])
            if u[0] + 1 < best[0]:
                best = (u[0] + 1, u[1], u[2] + 1, u[3])
            if l[0] + 1 < best[0]:
                best = (l[0] + 1, l[1], l[2], l[3] + 1)
            cur.append(best)
        prev = cur
    return prev[N]


def distance(ref, hyp):
    """The Levenshtein distance by the textbook recurrence: no tie rule, no counts."""
    M, N = len(ref), len(hyp)
    prev = list(range(N + 1))
    for i in range(1, M + 1):
        cur = [i] + [0] * N
        for j in range(1, N + 1):
            cur[j] = min(prev[j - 1] + (ref[i - 1] != hyp[j - 1]), prev[j] + 1, cur[j - 1] + 1)
        prev = cur
    return prev[N]


def identities_hold(M, N, cell):
    c, s, d, i = cell
    return (c == s + d + i and N == M - d + i and s + d <= M and s + i <= N and c <= max(M, N) and c >= abs(M - N)
            and min(s, d, i) >= 0)


def binary_pairs(max_len=5):
    """Every ordered pair of binary strings of up to max_len tokens, the empty one included: 63 ^ 2 = 3969 for 5."""
    words = [w for n in range(max_len + 1) for w in itertools.product((0, 1), repeat=n)]
    return [(list(a), list(b)) for a in words for b in words]


# ---- shapes that follow the kernel ------------------------------------------------------------------------------------------
NS = (0, 1, 2, 63, 64, 65, 300)


def exact_shapes(configs, limits):
    """{name: (M, N)} from F.edit_distance_tiles().  M: 0, 1, around the rows per lane KS of every configuration (KS - 1, KS,
    KS + 1), around its first wave seam (63 KS, 64 KS - 1, 64 KS, 64 KS + 1, 65 KS) and its second (128 KS + 1), its largest
    width and the next one, the overall limit.  N walks through {0, 1, 2, 63, 64, 65, 300}, and every M also meets 65 (64 at
    the limit, 2 beyond 1100: the longest case is 4096 x 64 cells)."""
    max_ref, _ = limits
    ms = {0, 1, max_ref}
    for max_m, ks, _nt in configs:
        ms |= {ks - 1, ks, ks + 1, 63 * ks, 64 * ks - 1, 64 * ks, 64 * ks + 1, 65 * ks, 128 * ks + 1, max_m, max_m + 1}
    shapes = {}
    for k, M in enumerate(sorted(m for m in ms if m <= max_ref)):
        walk = NS[k % len(NS)]
        for N in {walk if M * walk <= 600 * 300 else 1, 64 if M == max_ref else 65 if M <= 1100 else 2}:
            shapes["M%d_N%d" % (M, N)] = (M, N)
    for N in NS:                                                # every N at a ragged width and just past the first seam
        shapes["M7_N%d" % N] = (7, N)
        shapes["M%d_N%d" % (64 * configs[0][1] + 1, N)] = (64 * configs[0][1] + 1, N)
    return shapes


def _rand_tokens(rng, n, alphabet):
    return [rng.randrange(alphabet) for _ in range(n)]


def _edited(rng, ref, n_edits, alphabet, N):
    """A hypothesis of exactly N tokens made from ref by random edits, then cut or padded to N."""
    h = list(ref)
    for _ in range(n_edits):
        kind = rng.randrange(3)
        if kind == 0 and h:
            h[rng.randrange(len(h))] = rng.randrange(alphabet)
        elif kind == 1 and h:
            del h[rng.randrange(len(h))]
        else:
            h.insert(rng.randrange(len(h) + 1), rng.randrange(alphabet))
    h = h[:N]
    return h + _rand_tokens(rng, N - len(h), alphabet)


KINDS = ("alpha2", "alpha3", "alpha30", "edited", "identical", "disjoint")


def exact_pair(seed, M, N, kind):
    """(ref, hyp) as lists of Python ints."""
    rng = random.Random(seed * 7919 + M * 131 + N)
    if kind.startswith("alpha"):
        a = int(kind[5:])
        return _rand_tokens(rng, M, a), _rand_tokens(rng, N, a)
    if kind == "edited":
        ref = _rand_tokens(rng, M, 30)
        return ref, _edited(rng, ref, max(1, min(M, N) // 8), 30, N)
    if kind == "identical":
        ref = _rand_tokens(rng, M, 30)
        return ref, (ref * (N // M + 1))[:N] if M else [0] * N       # the reference, repeated where N > M
    if kind == "disjoint":
        return _rand_tokens(rng, M, 5), [5 + t for t in _rand_tokens(rng, N, 5)]
    raise ValueError(kind)


def kind_of(name):
    return KINDS[sum(map(ord, name)) % len(KINDS)]


@functools.lru_cache(maxsize=None)
def case(name, M, N):
    """(ref, hyp, (cost, S, D, I)) of a named shape: built once, shared by every test that needs it."""
    ref, hyp = exact_pair(len(name), M, N, kind_of(name))
    want = ops(ref, hyp)
    if kind_of(name) == "disjoint":
        assert want[0] == max(M, N)
    if kind_of(name) == "identical" and N <= M:
        assert want == (M - N, 0, M - N, 0)
    return ref, hyp, want


HIGH = 1 << 32


def high_word_pair():
    """int64 tokens above 2 ^ 32 that differ only in the high word: equal as 32-bit values, different as integers."""
    rng = random.Random(5)
    ref = [rng.randrange(4) + HIGH * (1 + rng.randrange(3)) for _ in range(37)]
    hyp = [t if rng.random() < 0.6 else (t % HIGH) + HIGH * (1 + rng.randrange(3)) for t in ref][:33]
    return ref, hyp, ops(ref, hyp)


@functools.lru_cache(maxsize=None)
def ragged_batch(B=3, nbest=4, N=21, M=9, seed=11, garbage=99):
    """An n-best batch with every length from 0 to the width somewhere, -1 hypothesis lengths, and garbage beyond the lengths.
    Returns (hyps (B, nbest, N), refs (B, M), hyp_len (B, nbest), ref_len (B,), want (B, nbest, 4)) as numpy int64."""
    rng = random.Random(seed)
    hyps = np.full((B, nbest, N), garbage, dtype=np.int64)
    refs = np.full((B, M), garbage + 1, dtype=np.int64)
    hl = np.zeros((B, nbest), dtype=np.int64)
    rl = np.zeros((B,), dtype=np.int64)
    want = np.zeros((B, nbest, 4), dtype=np.int64)
    lens = list(range(N + 1))
    rng.shuffle(lens)
    for b in range(B):
        rl[b] = (0, M, M // 2, 1)[b % 4] if b < 4 else rng.randrange(M + 1)
        refs[b, :rl[b]] = _rand_tokens(rng, int(rl[b]), 3)
        for k in range(nbest):
            n = lens[(b * nbest + k) % len(lens)]
            if (b * nbest + k) % 5 == 4:
                hl[b, k] = -1
                want[b, k] = -1
                continue
            hl[b, k] = n
            hyps[b, k, :n] = _rand_tokens(rng, n, 3)
            want[b, k] = ops(list(refs[b, :rl[b]]), list(hyps[b, k, :n]))
    return hyps, refs, hl, rl, want


@functools.lru_cache(maxsize=None)
def grid_batch(N=13, M=6):
    """Every hypothesis length 0 .. N against every reference length 0 .. M, as one flat batch with garbage beyond the lengths:
    (hyps (P, N), refs (P, M), hyp_len (P,), ref_len (P,), want (P, 4))."""
    rng = random.Random(17)
    P = (N + 1) * (M + 1)
    hyps = np.full((P, N), 98, dtype=np.int64)
    refs = np.full((P, M), 99, dtype=np.int64)
    hl, rl, want = np.zeros(P, dtype=np.int64), np.zeros(P, dtype=np.int64), np.zeros((P, 4), dtype=np.int64)
    for p, (n, m) in enumerate(itertools.product(range(N + 1), range(M + 1))):
        hl[p], rl[p] = n, m
        hyps[p, :n] = _rand_tokens(rng, n, 2)
        refs[p, :m] = _rand_tokens(rng, m, 2)
        want[p] = ops(list(refs[p, :m]), list(hyps[p, :n]))
    return hyps, refs, hl, rl, want
