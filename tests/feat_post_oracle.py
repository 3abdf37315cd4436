"""Float64 numpy restatement of F.compute_deltas and F.sliding_window_cmn, each in two independent forms.

compute_deltas(specgram, win_length, mode): (..., freq, time); pad n = (win_length - 1) // 2 frames with `mode`, then
out[t] = sum_{j=-n..n} j * xpad[t + n + j] / denom, denom = n (n + 1) (2n + 1) / 3.
sliding_window_cmn(specgram, cmn_window, min_cmn_window, center, norm_vars): (..., time, freq); window [s(t), e(t)) of
the reference's per-frame loop, mean (and variance) over it.
"""
import numpy as np
import torch

_NP_PAD = {"replicate": "edge", "reflect": "reflect", "circular": "wrap", "constant": "constant"}


def _n_denom(win_length):
    if win_length < 3:
        raise ValueError(f"Window length should be greater than or equal to 3. Found win_length {win_length}")
    n = (win_length - 1) // 2
    return n, n * (n + 1) * (2 * n + 1) / 3


def deltas_pad_corr(x, win_length=5, mode="replicate"):
    """Form 1: numpy pad + explicit correlation."""
    x = np.asarray(x, dtype=np.float64)
    n, denom = _n_denom(win_length)
    shape = x.shape
    rows = x.reshape(-1, shape[-1])
    T = shape[-1]
    xp = np.pad(rows, ((0, 0), (n, n)), mode=_NP_PAD[mode])
    out = np.zeros_like(rows)
    for j in range(-n, n + 1):
        out += j * xp[:, n + j:n + j + T]
    return (out / denom).reshape(shape)


def deltas_conv1d(x, win_length=5, mode="replicate"):
    """Form 2: the reference's composition on CPU float64 -- torch pad + grouped conv1d."""
    x = torch.as_tensor(np.asarray(x, dtype=np.float64))
    n, denom = _n_denom(win_length)
    shape = x.shape
    x = x.reshape(1, -1, shape[-1])
    kernel = torch.arange(-n, n + 1, 1, dtype=torch.float64).repeat(x.shape[1], 1, 1)
    xp = torch.nn.functional.pad(x, (n, n), mode=mode)
    out = torch.nn.functional.conv1d(xp, kernel, groups=x.shape[1]) / denom
    return out.reshape(shape).numpy()


def cmn_bounds(T, cmn_window=600, min_cmn_window=100, center=False):
    """(s, e) of every frame: the reference's per-frame window logic, literally."""
    s_all, e_all = np.zeros(T, np.int64), np.zeros(T, np.int64)
    for t in range(T):
        if center:
            s = t - cmn_window // 2
            e = s + cmn_window
        else:
            s = t - cmn_window
            e = t + 1
        if s < 0:
            e -= s
            s = 0
        if not center and e > t:
            e = max(t + 1, min_cmn_window)
        if e > T:
            s -= e - T
            e = T
            if s < 0:
                s = 0
        s_all[t], e_all[t] = s, e
    return s_all, e_all


def _finish(shape, out):
    out = out.reshape(shape)
    if len(shape) == 2:
        out = out.squeeze(0) if out.shape[0] == 1 else out
    return out


def cmn_loop(x, cmn_window=600, min_cmn_window=100, center=False, norm_vars=False):
    """Form 1: the per-frame loop with running sums (float64), adding one frame and dropping one per step."""
    x = np.asarray(x, dtype=np.float64)
    shape = x.shape
    T, F = shape[-2:]
    xs = x.reshape(-1, T, F)
    out = np.zeros_like(xs)
    s_all, e_all = cmn_bounds(T, cmn_window, min_cmn_window, center)
    cur = np.zeros((xs.shape[0], F))
    cursq = np.zeros((xs.shape[0], F))
    ls = le = -1
    for t in range(T):
        s, e = int(s_all[t]), int(e_all[t])
        if ls == -1:
            part = xs[:, s:e, :]
            cur += part.sum(1)
            cursq += (part ** 2).sum(1)
        else:
            if s > ls:
                cur -= xs[:, ls, :]
                cursq -= xs[:, ls, :] ** 2
            if e > le:
                cur += xs[:, le, :]
                cursq += xs[:, le, :] ** 2
        n = e - s
        ls, le = s, e
        out[:, t, :] = xs[:, t, :] - cur / n
        if norm_vars:
            if n == 1:
                out[:, t, :] = 0.0
            else:
                var = cursq / n - cur ** 2 / n ** 2
                with np.errstate(divide="ignore", invalid="ignore"):
                    out[:, t, :] *= var ** -0.5
    return _finish(shape, out)


def cmn_prefix(x, cmn_window=600, min_cmn_window=100, center=False, norm_vars=False):
    """Form 2: vectorised -- prefix sums gathered at the (s, e) map (computed here in closed form, independently)."""
    x = np.asarray(x, dtype=np.float64)
    shape = x.shape
    T, F = shape[-2:]
    xs = x.reshape(-1, T, F)
    t = np.arange(T)
    if center:
        s = t - cmn_window // 2
        e = s + cmn_window
    else:
        s = t - cmn_window
        e = t + 1
    e = np.where(s < 0, e - s, e)
    s = np.maximum(s, 0)
    if not center:
        e = np.where(e > t, np.maximum(t + 1, min_cmn_window), e)
    over = e > T
    s = np.where(over, np.maximum(s - (e - T), 0), s)
    e = np.minimum(e, T)
    n = (e - s).astype(np.float64)[None, :, None]
    p1 = np.concatenate([np.zeros((xs.shape[0], 1, F)), np.cumsum(xs, 1)], 1)
    p2 = np.concatenate([np.zeros((xs.shape[0], 1, F)), np.cumsum(xs * xs, 1)], 1)
    s1 = p1[:, e, :] - p1[:, s, :]
    s2 = p2[:, e, :] - p2[:, s, :]
    out = xs - s1 / n
    if norm_vars:
        with np.errstate(divide="ignore", invalid="ignore"):
            scaled = out * (s2 / n - s1 ** 2 / n ** 2) ** -0.5
        out = np.where(n == 1, 0.0, scaled)
    return _finish(shape, out)
