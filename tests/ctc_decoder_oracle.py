"""float64 oracle of CTC prefix beam search without a language model (audio_amd.models.decoder), numpy / Python only.

search()  the definition over the full K V candidate set of every frame (no reduction to the largest tokens): a beam of at
          most K distinct prefixes with (pb, pnb), started as {(): (0, -inf)}; a frame with lp[blank] > thr is skipped entirely;
          otherwise prefix l with last token e and tot = logaddexp(pb, pnb) gives  l: pb' += tot + lp[blank];  l (not empty):
          pnb' += pnb + lp[e];  l + c, c != blank: pnb' += (c == e ? pb : tot) + lp[c]; contributions to one prefix merge with
          logaddexp; the K largest logaddexp(pb', pnb') that are neither -inf nor NaN stay, ties by the prefix as a tuple (so
          of two extensions of one prefix the smaller token first).
brute()   the exact posterior of every collapsed sequence by enumerating all V ** T alignments.
"""
import itertools
import math
from typing import Dict, List, NamedTuple, Tuple

import numpy as np

NEG = -np.inf
EPS = 2.0 ** -52


def lae(a, b):
    with np.errstate(invalid="ignore"):
        return np.logaddexp(a, b)


class Result(NamedTuple):
    hyps: List[Tuple[Tuple[int, ...], float]]       # the final beam in rank order: (tokens, score)
    gap: float                                      # the smallest gap between adjacent scores at or inside any cut-off
    frames: int                                     # unskipped frames
    scale: float                                    # the largest max(1, |score|) in any beam


def search(lp: np.ndarray, beam: int, blank: int, thr: float) -> Result:
    lp = np.asarray(lp, dtype=np.float64)
    T, V = lp.shape
    cur: Dict[Tuple[int, ...], Tuple[float, float]] = {(): (0.0, NEG)}
    gap, frames, scale = math.inf, 0, 1.0
    nonblank = np.arange(V) != blank
    for t in range(T):
        row = lp[t]
        if row[blank] > thr:
            continue
        frames += 1
        new: Dict[Tuple[int, ...], List[float]] = {}
        ext_rows = []                                # (parent, scores of parent + c over every c; -inf where it is no candidate)
        with np.errstate(invalid="ignore"):
            for l, (pb, pnb) in cur.items():
                tot = lae(pb, pnb)
                new[l] = [tot + row[blank], pnb + row[l[-1]] if l else NEG]
            for l, (pb, pnb) in cur.items():
                tot = lae(pb, pnb)
                ext = tot + row
                if l:
                    ext[l[-1]] = pb + row[l[-1]]
                ext = np.where(nonblank, ext, NEG)
                for q in cur:                        # an extension that is an entry of the beam merges into it
                    if len(q) == len(l) + 1 and q[:-1] == l:
                        new[q][1] = lae(new[q][1], ext[q[-1]])
                        ext[q[-1]] = NEG
                ext_rows.append((l, ext))
        cands = [(float(lae(pb, pnb)), l, (float(pb), float(pnb))) for l, (pb, pnb) in new.items()]
        if ext_rows:
            allv = np.concatenate([e for _, e in ext_rows])
            allv = allv[allv > NEG]                  # NaN compares false
            cut = NEG
            if allv.size > beam + 1:
                cut = np.partition(allv, allv.size - beam - 1)[allv.size - beam - 1]
            for l, ext in ext_rows:
                for c in np.flatnonzero(ext >= cut):
                    cands.append((float(ext[c]), l + (int(c),), (NEG, float(ext[c]))))
        cands = [c for c in cands if c[0] > NEG]     # never -inf, never NaN
        cands.sort(key=lambda c: (-c[0], c[1]))
        kept = cands[:beam]
        for x, y in zip(cands[:beam], cands[1:beam + 1]):
            gap = min(gap, x[0] - y[0])
        for c in kept:
            scale = max(scale, abs(c[0]))
        cur = {l: v for _, l, v in kept}
    hyps = sorted(((l, float(lae(pb, pnb))) for l, (pb, pnb) in cur.items()), key=lambda h: (-h[1], h[0]))
    return Result(hyps, gap, frames, scale)


def brute(lp: np.ndarray, blank: int) -> Dict[Tuple[int, ...], float]:
    lp = np.asarray(lp, dtype=np.float64)
    T, V = lp.shape
    mass: Dict[Tuple[int, ...], List[float]] = {}
    for path in itertools.product(range(V), repeat=T):
        seq = tuple(c for i, c in enumerate(path) if c != blank and (i == 0 or c != path[i - 1]))
        mass.setdefault(seq, []).append(sum(lp[t, c] for t, c in enumerate(path)))
    out = {}
    for seq, terms in mass.items():
        m = max(terms)
        out[seq] = m + math.log(math.fsum(math.exp(x - m) for x in terms))
    return out


def bound(res: Result) -> float:
    """The score bound of the kernels against search(): at most 4 additions and 4 logaddexp per prefix and frame, each a few ulp
    of a value of at most `scale`, and logaddexp is 1-Lipschitz in its inputs, so the errors add up over the unskipped frames."""
    return 16 * max(res.frames, 1) * EPS * res.scale


def decided(res: Result) -> bool:
    return res.gap > 1000 * bound(res)


# ---- cases ---------------------------------------------------------------------------------------------------------------------
# name: (T, V, K, seed).  Ragged batches of 3 with one full-length example; the seeds were chosen when the tests were written so
# that every example is decided for float32 and float64 inputs at both thresholds used (test_ctc_decoder.py asserts it).
CASES = {
    "general": (50, 32, 8, 1),
    "few_tokens": (40, 5, 10, 1),
    "one_token": (30, 2, 4, 1),
    "greedy": (64, 40, 1, 1),
    "k_limit": (48, 64, 32, 1),
    "long_row": (64, 1024, 10, 1),
    "full_beam": (33, 3, 16, 1),
}
THR = math.log(0.95)


def lengths_of(T: int) -> List[int]:
    return [T, max(1, (2 * T) // 3), max(1, T // 3 + 1)]


def logits(seed: int, B: int, T: int, V: int, blank: int = 0, scale: float = 3.0, blank_share: float = 0.4) -> np.ndarray:
    """Seeded normals times `scale`; a `blank_share` of the frames is dominated by blank (they are the ones a threshold of
    log 0.95 skips).  float64; the caller takes log_softmax and rounds to its dtype."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, T, V)) * scale
    boost = rng.random((B, T)) < blank_share
    x[..., blank] += np.where(boost, 6.0 * scale + math.log(V), 0.0)
    return x


def emissions(seed: int, B: int, T: int, V: int, dtype: str = "float32", blank: int = 0, scale: float = 3.0,
              blank_share: float = 0.4) -> np.ndarray:
    """log_softmax of logits(), rounded to `dtype` (a torch dtype's name) and returned in float64: what the tensor holds."""
    import torch
    x = torch.log_softmax(torch.from_numpy(logits(seed, B, T, V, blank, scale, blank_share)), dim=-1)
    return x.to(getattr(torch, dtype)).to(torch.float64).numpy()


def case(name: str, dtype: str = "float32"):
    """(emissions (3, T, V) float64 holding `dtype` values, lengths, K) of a named case."""
    T, V, K, seed = CASES[name]
    return emissions(seed, 3, T, V, dtype), lengths_of(T), K


def expected(lp: np.ndarray, lengths, K: int, blank: int = 0, thr: float = THR) -> List[Result]:
    return [search(lp[b, :n], K, blank, thr) for b, n in enumerate(lengths)]


def own_token_case() -> np.ndarray:
    """(1, 3, 4) float32-exact log-probabilities, K = 1, threshold 0: after frames 0 and 1 the beam is {(1,)} with all of its mass
    ending in blank as far as float64 can tell (tot == pb bit for bit).  In frame 2 token 1 is the SMALLEST non-blank value, so it
    is not among the frame's K + 1 = 2 largest tokens, yet pb + lp[1], tot + lp[2] and tot + lp[3] round to one float64
    (-2^40 - 1; the three values differ by 2^-24 and 2^-23, the sums' spacing is 2^-12): three extensions of one prefix with
    bit-equal scores, of which the smaller token ranks first.  The answer is (1, 1), and only the candidate (parent x its own
    last token) can give it."""
    a = -2.0 ** 40
    return np.array([[[2 * a, a, 2 * a, 2 * a],
                      [0.0, -200.0, -200.0, -200.0],
                      [-5.0, -1.0, -1.0 + 2.0 ** -24, -1.0 + 2.0 ** -23]]])
