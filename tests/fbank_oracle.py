"""numpy restatement of the Bark and chroma filterbank definitions (README, "Contract") and of the dense projection, and what
the CPU and GPU tests share: the configurations, the inputs, the cases and the error bounds.

Every definition is one function of a dtype: evaluated with ``np.float64`` it is the reference; evaluated with ``np.float32``
every intermediate is rounded to float32, which measures what a float32 evaluation of the same definition loses -- the
yardstick the builders are held to (at most ``MARGIN`` times that loss).

    bark(f):   wang 6 asinh(f / 600);  schroeder 7 asinh(f / 650);
               traunmuller b = 26.81 f / (1960 + f) - 0.53, then b += 0.15 (2 - b) where b < 2, b += 0.22 (b - 20.1) where b > 20.1
    hz(b):     the exact inverse, per element
    bark fb:   triangles max(0, min(down, up)) between hz(linspace(bark(f_min), bark(f_max), n_barks + 2))
    chroma fb: librosa's filters.chroma (see `chroma`)
    dense projection: out[v][n] = sum_k x[v][k] W[k][n]

Nothing here imports the product's builders."""
import functools

import numpy as np
import torch

from inverse_mel_oracle import EPS, LAYOUTS, laid_out, worst_ratio  # noqa: F401  (shared with the InverseMelScale tests)

MARGIN = 4.0                       # a different but legitimate order of float32 operations
BARK_SCALES = ("traunmuller", "schroeder", "wang")
# (n_freqs, n_barks, sample_rate): no all-zero filter in any of them, for any scale
BARK_CONFIGS = [(201, 40, 16000), (257, 64, 16000), (33, 10, 8000), (513, 128, 22050)]
# (sample_rate, n_freqs, n_chroma, keyword arguments): value parity, even n_chroma only
CHROMA_CONFIGS = [
    (16000, 201, 12, {}), (22050, 1025, 12, {}), (16000, 33, 12, {}), (16000, 65, 24, {}), (44100, 2049, 36, {}), (8000, 5, 12, {}),
    (16000, 201, 12, {"octwidth": None}), (16000, 201, 12, {"base_c": False}), (16000, 201, 12, {"tuning": 0.3}),
    (16000, 201, 12, {"norm": 1}), (16000, 201, 12, {"norm": float("inf")}),
]


# ---- Bark ---------------------------------------------------------------------------------------------------------------------
def bark(f, scale, dt=np.float64):
    f = np.asarray(f, dtype=dt)
    if scale == "wang":
        return (dt(6.0) * np.arcsinh(f / dt(600.0))).astype(dt)
    if scale == "schroeder":
        return (dt(7.0) * np.arcsinh(f / dt(650.0))).astype(dt)
    if scale != "traunmuller":
        raise ValueError(scale)
    b = (dt(26.81) * f / (dt(1960.0) + f) - dt(0.53)).astype(dt)
    b = np.where(b < 2, b + dt(0.15) * (dt(2.0) - b), np.where(b > dt(20.1), b + dt(0.22) * (b - dt(20.1)), b))
    return b.astype(dt)


def hz(b, scale, dt=np.float64):
    b = np.asarray(b, dtype=dt)
    if scale == "wang":
        return (dt(600.0) * np.sinh(b / dt(6.0))).astype(dt)
    if scale == "schroeder":
        return (dt(650.0) * np.sinh(b / dt(7.0))).astype(dt)
    if scale != "traunmuller":
        raise ValueError(scale)
    b = np.where(b < 2, (b - dt(0.3)) / dt(0.85), np.where(b > dt(20.1), (b + dt(4.422)) / dt(1.22), b)).astype(dt)
    return (dt(1960.0) * (b + dt(0.53)) / (dt(26.28) - b)).astype(dt)


def barkscale_fbanks(n_freqs, f_min, f_max, n_barks, sample_rate, scale="traunmuller", dt=np.float64):
    all_freqs = np.linspace(0, sample_rate // 2, n_freqs).astype(dt)
    m_pts = np.linspace(float(bark(f_min, scale, dt)), float(bark(f_max, scale, dt)), n_barks + 2).astype(dt)
    f_pts = hz(m_pts, scale, dt)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts[None, :] - all_freqs[:, None]
    down = -slopes[:, :-2] / f_diff[:-1]
    up = slopes[:, 2:] / f_diff[1:]
    fb = np.maximum(dt(0.0), np.minimum(down, up))
    assert fb.dtype == dt
    return fb


# ---- chroma -------------------------------------------------------------------------------------------------------------------
def chroma(sample_rate, n_freqs, n_chroma, tuning=0.0, ctroct=5.0, octwidth=2.0, norm=2, base_c=True, dt=np.float64):
    freqs = np.linspace(0, sample_rate // 2, n_freqs).astype(dt)[1:]
    a440 = dt(440.0 * 2.0 ** (tuning / n_chroma))
    bins = dt(n_chroma) * np.log2(freqs / (a440 / dt(16.0)))
    bins = np.concatenate([[bins[0] - dt(1.5 * n_chroma)], bins]).astype(dt)
    widths = np.concatenate([np.maximum(bins[1:] - bins[:-1], dt(1.0)), [dt(1.0)]]).astype(dt)
    D = bins[:, None] - np.arange(n_chroma).astype(dt)[None, :]
    n2 = dt(round(n_chroma / 2))
    D = np.remainder(D + n2, dt(n_chroma)) - n2
    fb = np.exp(dt(-0.5) * (dt(2.0) * D / widths[:, None]) ** 2)
    if norm == float("inf"):
        length = np.abs(fb).max(axis=1)
    elif norm == 1:
        length = np.abs(fb).sum(axis=1, dtype=dt)
    elif norm == 2:
        length = np.sqrt((fb * fb).sum(axis=1, dtype=dt))
    else:
        length = (np.abs(fb) ** dt(norm)).sum(axis=1, dtype=dt) ** dt(1.0 / norm)
    fb = fb / np.maximum(length, dt(1e-12))[:, None]
    if octwidth is not None:
        fb = fb * np.exp(dt(-0.5) * ((bins / dt(n_chroma) - dt(ctroct)) / dt(octwidth)) ** 2)[:, None]
    if base_c:
        fb = np.roll(fb, -3 * (n_chroma // 12), axis=1)
    assert fb.dtype == dt
    return fb


def builder_ratio(built, f64, f32):
    """(the builder's largest absolute difference from the float64 form) / (the float32 form's): at most MARGIN."""
    mine = np.abs(np.asarray(built, dtype=np.float64) - f64).max()
    yard = np.abs(f32.astype(np.float64) - f64).max()
    return float(mine / yard) if yard > 0 else (0.0 if mine == 0 else float("inf"))


# ---- the dense projection -----------------------------------------------------------------------------------------------------
DENSE_K = (5, 33, 65, 201, 257, 1025)
DENSE_N = (1, 12, 16, 17, 128)


def dense_frames(tile):
    return (1, tile - 1, tile, tile + 1, 2 * tile + 3)


def dense_cases(tile):
    """(K, N, frames, rows): every K with every N; the frame counts and 1 - 3 rows rotate, so that each K and each N meets
    every frame count around the tile."""
    fr = dense_frames(tile)
    return [(K, N, fr[(i + j) % 5], 1 + (i + 2 * j) % 3) for i, K in enumerate(DENSE_K) for j, N in enumerate(DENSE_N)]


@functools.lru_cache(maxsize=None)
def dense_filterbank(K, N):
    """A dense (K, N) float32 filterbank: the chroma definition where it has this shape (12 outputs: real chroma values,
    subnormal entries included), else a chroma-like positive matrix with entries over many decades."""
    if N in (12, 24, 36) and K >= 2:
        fb = chroma(16000, K, N).astype(np.float32)
    else:
        g = np.random.default_rng(1000 * K + N)
        fb = np.exp(-8.0 * g.random((K, N)) ** 2).astype(np.float32) * (g.random((K, N)) < 0.97)
        fb = fb.astype(np.float32)
    fb.setflags(write=False)
    return fb


def spec_values(rows, K, T, dtype, seed):
    """Power-spectrogram-like values rounded to `dtype`: a CPU tensor (rows, K, T); chi-square with two degrees of freedom
    under an envelope that falls by e^4 over the frequency axis."""
    g = torch.Generator().manual_seed(seed)
    re = torch.randn((rows, K, T), generator=g, dtype=torch.float64)
    im = torch.randn((rows, K, T), generator=g, dtype=torch.float64)
    env = torch.exp(-4.0 * torch.arange(K, dtype=torch.float64) / max(K, 1)).view(1, K, 1)
    return ((re * re + im * im) * env).to(dtype)


def dense(x, w):
    """x: (..., K, T) float64, w: (K, N) -> (..., N, T) float64."""
    return np.swapaxes(np.matmul(np.swapaxes(x, -1, -2), np.asarray(w, dtype=np.float64)), -1, -2)


def dense_bound(x, w, dtype):
    """The issue's bound on |got - want| per output: (K + 2) 2^-24 sum_k |W[k][n]| |x[v][k]| -- the forward bound of a
    float32 FMA chain of K terms -- plus K 2^-149 for subnormal products, plus half an ulp of a half output type at |want|."""
    K = w.shape[0]
    b = (K + 2) * 2.0 ** -24 * dense(np.abs(x), np.abs(np.asarray(w, dtype=np.float64))) + K * 2.0 ** -149
    if dtype in EPS:
        want = np.abs(dense(x, w))
        tiny = 2.0 ** -24 if dtype == torch.float16 else 2.0 ** -133           # the subnormal spacing
        b = b + np.maximum(2.0 ** np.floor(np.log2(np.maximum(want, 1e-300))) * EPS[dtype], tiny / 2)
    return b
