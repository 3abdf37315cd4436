"""float64 numpy restatement of the InverseMelScale contract (README, "Contract"), and what the CPU and GPU tests share: the
configurations, the input layouts and the error bound.

    A      = fb^T                       (n_mels x n_stft), the float32 filterbank's values as float64
    P      = sum over sigma_i > rcond sigma_max of v_i u_i^T / sigma_i,   rcond = 2^-23 max(n_stft, n_mels)
    result = relu(P y) per frame,       y = x, or exp(x) with log_input

Nothing here imports the product's builder: the SVD cut below is this file's own."""
import functools

import numpy as np
import torch

# name: (n_stft, n_mels, sample_rate, f_max, norm, mel_scale)
CONFIGS = {
    "tiny": (33, 12, 16000, 8000.0, None, "htk"),
    "small": (65, 20, 16000, 8000.0, "slaney", "slaney"),
    "default": (201, 80, 16000, 8000.0, None, "htk"),          # rank 75
    "odd": (257, 127, 16000, 8000.0, None, "htk"),             # n_mels % 4 != 0, rank 114, zero filters
    "taco": (513, 80, 22050, 8000.0, "slaney", "slaney"),      # full rank, n_stft beyond one LDS tile
}
RANKS = {"tiny": 12, "small": 20, "default": 75, "odd": 114, "taco": 80}
LAYOUTS = ("frame_major", "time_major", "frame_major_misaligned", "time_major_misaligned")
EPS = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}      # half an ulp of 1.0


def rcond(n_stft, n_mels):
    return 2.0 ** -23 * max(n_stft, n_mels)


def singular_values(fb):
    return np.linalg.svd(np.asarray(fb, dtype=np.float64).T, compute_uv=False)


def pinv(fb):
    """(rank, P (n_stft, n_mels) float64) of fb^T by the rule above."""
    a = np.asarray(fb, dtype=np.float64).T
    u, s, vt = np.linalg.svd(a, full_matrices=False)
    cut = rcond(a.shape[1], a.shape[0]) * s.max()
    p = np.zeros((a.shape[1], a.shape[0]))
    rank = 0
    for i in range(s.shape[0]):
        if s[i] > cut:
            p += np.outer(vt[i], u[:, i]) / s[i]
            rank += 1
    return rank, p


def inverse_mel(x, p, log_input=False):
    """x: (..., n_mels, T) float64 -> (..., n_stft, T)."""
    y = np.exp(x) if log_input else x
    return np.maximum(np.matmul(p, y), 0.0)


def bound(x, p, dtype, log_input=False):
    """The issue's bound on |got - want| per output: (K_pad + 2) 2^-24 sum_m |P32[f][m]| |y[v][m]| -- the forward bound of a
    float32 FMA chain of K_pad terms plus the rounding of P -- with + 4 in place of + 2 under log_input (expf within 1 ulp),
    plus half an ulp of a half output type at |want|."""
    k_pad = (p.shape[1] + 3) // 4 * 4
    y = np.exp(x) if log_input else x
    p32 = np.abs(p.astype(np.float32).astype(np.float64))
    b = (k_pad + (4 if log_input else 2)) * 2.0 ** -24 * np.matmul(p32, np.abs(y))
    if dtype in EPS:
        want = np.abs(inverse_mel(x, p, log_input))
        tiny = 2.0 ** -24 if dtype == torch.float16 else 2.0 ** -133           # the subnormal spacing
        b = b + np.maximum(2.0 ** np.floor(np.log2(np.maximum(want, 1e-300))) * EPS[dtype], tiny / 2)
    return b


def worst_ratio(got, want, b):
    """The largest |got - want| / bound; inf where an error exceeds a zero bound (a bin no filter reaches has an all-zero row
    of P: its bound is 0 and its output must be exactly 0) or is not finite."""
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    if not np.isfinite(err).all() or (err[b == 0] != 0).any():
        return float("inf")
    return float((err[b > 0] / b[b > 0]).max()) if (b > 0).any() else 0.0


@functools.lru_cache(maxsize=None)
def filterbank(name):
    """The configuration's filterbank as the module builds it (float32 torch tensor, (n_stft, n_mels))."""
    import warnings
    from audio_amd import _host
    n_stft, n_mels, sr, f_max, norm, scale = CONFIGS[name]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                     # `odd` has all-zero filters: that is its point
        return _host.melscale_fbanks(n_stft, 0.0, f_max, n_mels, sr, norm, scale)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(rank, P float64) of the configuration: computed once, shared by the tests, never written to."""
    rank, p = pinv(filterbank(name).numpy())
    p.setflags(write=False)
    return rank, p


def mel_values(rows, n_mels, T, dtype, log_input, seed):
    """iid uniform(0, 1) mel values (their logarithm under log_input) rounded to `dtype`: a CPU tensor (rows, n_mels, T)."""
    g = torch.Generator().manual_seed(seed)
    u = torch.rand((rows, n_mels, T), generator=g, dtype=torch.float64)
    if log_input:
        u = torch.log(torch.clamp(u, min=2.0 ** -20))
    return u.to(dtype)


def laid_out(x, layout):
    """The values of x (rows, n_mels, T) as a (rows, n_mels, T) view in one of LAYOUTS, on x's device.  The misaligned ones
    are cut from a wider buffer: a storage offset of one element and rows one element longer than they need to be."""
    rows, K, T = x.shape
    if layout == "time_major":
        v = x.contiguous()
    elif layout == "frame_major":
        v = x.transpose(1, 2).contiguous().transpose(1, 2)
    elif layout == "time_major_misaligned":
        big = torch.zeros(rows * K * (T + 1) + 1, dtype=x.dtype, device=x.device)
        v = big[1:].view(rows, K, T + 1)[:, :, :T]
        v.copy_(x)
    elif layout == "frame_major_misaligned":
        big = torch.zeros(rows * T * (K + 1) + 1, dtype=x.dtype, device=x.device)
        v = big[1:].view(rows, T, K + 1)[:, :, :K].transpose(1, 2)
        v.copy_(x)
    else:
        raise ValueError(layout)
    assert v.shape == x.shape and torch.equal(v, x)
    return v
