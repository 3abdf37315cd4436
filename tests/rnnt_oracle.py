"""The transducer loss restated three times on the CPU in float64, independently of csrc/rnnt_loss.h and of each other:

  recurrence(...)    the alpha recurrence cell by cell under torch autograd: costs, and gradients through autograd
  brute_force(...)   every alignment of a tiny lattice enumerated, log-sum-exp of the path scores under autograd
  closed_form(...)   alpha and beta in numpy and the gradient written out from them

All return the per-example gradient d cost_b / d logits (clamped per element when clamp > 0) times grad_costs[b].
tests/test_rnnt_loss.py asserts that the three agree to 1e-10 before anything else is judged by them."""
import itertools

import numpy as np
import torch


def _blank(blank, V):
    return blank + V if blank < 0 else blank


def _finish(grad, clamp, grad_costs):
    g = np.array(grad, dtype=np.float64)
    if clamp > 0:
        g = np.clip(g, -clamp, clamp)
    if grad_costs is not None:
        g = g * np.asarray(grad_costs, dtype=np.float64).reshape(-1, 1, 1, 1)
    return g


def recurrence(logits, targets, logit_lengths, target_lengths, blank=-1, clamp=-1.0, fused=True, grad_costs=None):
    x = torch.tensor(np.asarray(logits, dtype=np.float64), requires_grad=True)
    B, T, U1, V = x.shape
    bl = _blank(blank, V)
    lp = torch.log_softmax(x, -1) if fused else x
    costs = []
    for b in range(B):
        Tb, Ub = int(logit_lengths[b]), int(target_lengths[b])
        alpha = [[None] * (Ub + 1) for _ in range(Tb)]
        for t in range(Tb):
            for u in range(Ub + 1):
                terms = []
                if t > 0:
                    terms.append(alpha[t - 1][u] + lp[b, t - 1, u, bl])
                if u > 0:
                    terms.append(alpha[t][u - 1] + lp[b, t, u - 1, int(targets[b][u - 1])])
                if not terms:
                    alpha[t][u] = torch.zeros((), dtype=torch.float64)
                elif len(terms) == 1:
                    alpha[t][u] = terms[0]
                else:
                    alpha[t][u] = torch.logaddexp(terms[0], terms[1])
        costs.append(-(alpha[Tb - 1][Ub] + lp[b, Tb - 1, Ub, bl]))
    costs = torch.stack(costs)
    costs.sum().backward()                       # examples are independent: block b of the gradient is d cost_b
    return costs.detach().numpy(), _finish(x.grad.numpy(), clamp, grad_costs)


def brute_force(logits, targets, logit_lengths, target_lengths, blank=-1, clamp=-1.0, fused=True, grad_costs=None):
    x = torch.tensor(np.asarray(logits, dtype=np.float64), requires_grad=True)
    B, T, U1, V = x.shape
    bl = _blank(blank, V)
    lp = torch.log_softmax(x, -1) if fused else x
    costs = []
    for b in range(B):
        Tb, Ub = int(logit_lengths[b]), int(target_lengths[b])
        moves = Tb - 1 + Ub                     # Tb - 1 blanks and Ub labels in any order, then the closing blank
        scores = []
        for labels_at in itertools.combinations(range(moves), Ub):
            t = u = 0
            score = torch.zeros((), dtype=torch.float64)
            for k in range(moves):
                if k in labels_at:
                    score = score + lp[b, t, u, int(targets[b][u])]
                    u += 1
                else:
                    score = score + lp[b, t, u, bl]
                    t += 1
            assert (t, u) == (Tb - 1, Ub)
            scores.append(score + lp[b, t, u, bl])
        costs.append(-torch.logsumexp(torch.stack(scores), 0))
    costs = torch.stack(costs)
    costs.sum().backward()
    return costs.detach().numpy(), _finish(x.grad.numpy(), clamp, grad_costs)


def _log_softmax(x):
    m = x.max(-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(-1, keepdims=True))


def lattices(lp_b, tg, Tb, Ub, bl):
    """alpha, beta (Tb, Ub + 1) of one example from its log-probabilities (T, U1, V)."""
    alpha = np.full((Tb, Ub + 1), -np.inf)
    beta = np.full((Tb, Ub + 1), -np.inf)
    alpha[0, 0] = 0.0
    for t in range(Tb):
        for u in range(Ub + 1):
            if t == 0 and u == 0:
                continue
            a = alpha[t - 1, u] + lp_b[t - 1, u, bl] if t > 0 else -np.inf
            c = alpha[t, u - 1] + lp_b[t, u - 1, tg[u - 1]] if u > 0 else -np.inf
            alpha[t, u] = np.logaddexp(a, c)
    beta[Tb - 1, Ub] = lp_b[Tb - 1, Ub, bl]
    for t in range(Tb - 1, -1, -1):
        for u in range(Ub, -1, -1):
            if t == Tb - 1 and u == Ub:
                continue
            a = beta[t + 1, u] + lp_b[t, u, bl] if t + 1 < Tb else -np.inf
            c = beta[t, u + 1] + lp_b[t, u, tg[u]] if u < Ub else -np.inf
            beta[t, u] = np.logaddexp(a, c)
    return alpha, beta


def closed_form(logits, targets, logit_lengths, target_lengths, blank=-1, clamp=-1.0, fused=True, grad_costs=None,
                want_lattices=False):
    x = np.asarray(logits, dtype=np.float64)
    B, T, U1, V = x.shape
    bl = _blank(blank, V)
    lp = _log_softmax(x) if fused else x
    costs = np.zeros(B)
    grad = np.zeros_like(x)
    lats = []
    for b in range(B):
        Tb, Ub = int(logit_lengths[b]), int(target_lengths[b])
        tg = [int(k) for k in targets[b][:Ub]]
        alpha, beta = lattices(lp[b], tg, Tb, Ub, bl)
        lats.append((alpha, beta))
        logz = beta[0, 0]
        costs[b] = -logz
        for t in range(Tb):
            for u in range(Ub + 1):
                occ = np.exp(alpha[t, u] + beta[t, u] - logz)
                g = occ * np.exp(lp[b, t, u]) if fused else np.zeros(V)
                nxt = beta[t + 1, u] if t + 1 < Tb else (0.0 if u == Ub else -np.inf)
                g[bl] -= np.exp(alpha[t, u] + lp[b, t, u, bl] + nxt - logz)
                if u < Ub:
                    g[tg[u]] -= np.exp(alpha[t, u] + lp[b, t, u, tg[u]] + beta[t, u + 1] - logz)
                grad[b, t, u] = g
    out = (costs, _finish(grad, clamp, grad_costs))
    return out + (lats,) if want_lattices else out


def inputs(rng, B, T, U1, V, lengths=None, scale=3.0, blank=-1):
    """(logits float64, targets int32 without the blank, logit_lengths, target_lengths): the first example is full length."""
    bl = _blank(blank, V)
    logits = scale * rng.standard_normal((B, T, U1, V))
    labels = np.array([k for k in range(V) if k != bl], dtype=np.int32)
    targets = labels[rng.integers(0, len(labels), (B, max(U1 - 1, 0)))].astype(np.int32).reshape(B, U1 - 1)
    if lengths is None:
        ll = np.array([T] + [int(rng.integers(1, T + 1)) for _ in range(B - 1)], dtype=np.int32)
        tl = np.array([U1 - 1] + [int(rng.integers(0, U1)) for _ in range(B - 1)], dtype=np.int32)
    else:
        ll, tl = (np.array(v, dtype=np.int32) for v in lengths)
    return logits, targets, ll, tl


def bounds(logits, logit_lengths, target_lengths, u):
    """(cost bound (B,), gradient bound (B,)) of a kernel whose per-element arithmetic has unit roundoff u, from the inputs alone:
    eps_cell = u (V + 8 + 2 max|logits|) per log-sum-exp, (T_b + U_b) cells along a path."""
    x = np.asarray(logits, dtype=np.float64)
    V = x.shape[-1]
    finite = x[np.isfinite(x)]
    eps_cell = u * (V + 8 + 2 * (np.abs(finite).max() if finite.size else 0.0))
    n = np.asarray(logit_lengths, dtype=np.float64) + np.asarray(target_lengths, dtype=np.float64)
    return n * eps_cell, 2 * ((n + 2) * eps_cell + 16 * u)
