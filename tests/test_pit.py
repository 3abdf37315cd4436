"""Permutation-invariant training without a GPU: identities of the oracle (tests/pit_oracle.py), the margin the GPU tests rely
on, and the host-side errors of the entry points, which are raised before anything touches a device."""
import numpy as np
import pytest
import torch

import pit_oracle as PO
import audio_amd.functional as F


@pytest.mark.parametrize("S", [1, 2, 3, 5])
def test_oracle_identities(S):
    rng = np.random.default_rng(S)
    planted = rng.permutation(S)
    M = -np.ones((S, S))
    M[np.arange(S), planted] = 1.0
    best, perm = PO.assign(M)
    assert (perm == planted).all() and best == 1.0
    best, perm = PO.assign(np.full((S, S), 2.5))                             # the tie rule: the first in lexicographic order
    assert (perm == np.arange(S)).all() and best == 2.5
    R = rng.standard_normal((S, S))
    (b0, p0), (b1, p1) = PO.assign(R, "min"), PO.assign(-R, "max")
    assert b0 == -b1 and (p0 == p1).all()
    assert PO.margin(M) == (4.0 if S > 1 else float("inf"))              # one swap turns two +1 into -1


def test_mixtures_leave_a_margin_rounding_cannot_close():
    """The best total of every mixture the GPU tests assign leads the next by at least 1 dB for every fused metric."""
    worst = float("inf")
    for S, time, seed in PO.mix_cases(F.pit_tiles()[1]):
        p, t, planted = PO.mixtures(S, time, seed)
        for name in PO.METRICS:
            M = PO.matrix(p, t, name)
            assert (PO.assign(M)[1] == planted).all()
            worst = min(worst, PO.margin(M))
    print(f"smallest margin {worst:.2f} dB")
    assert worst >= 1.0


def test_host_side_errors():
    x, pit = torch.zeros(2, 3, 16), F.permutation_invariant_training
    si = F.scale_invariant_signal_distortion_ratio
    for fn in (lambda *a, **k: pit(*a, **k), lambda p, t, m, **k: F.pit_metric_matrix(p, t, m, **k)):
        with pytest.raises(ValueError, match=r"expects \(batch, sources, time\)"):
            fn(x[0], x[0], si)
        with pytest.raises(ValueError, match="same shape"):
            fn(x, torch.zeros(2, 3, 15), si)
        with pytest.raises(ValueError, match="at least one source"):
            fn(x[:, :0], x[:, :0], si)
        with pytest.raises(NotImplementedError, match="PIT_MAX_SOURCES = 8"):
            fn(torch.zeros(1, 9, 4), torch.zeros(1, 9, 4), si)
        with pytest.raises(ValueError, match="lengths must have the shape"):
            fn(x, x, si, lengths=torch.zeros(3, dtype=torch.int32))
        with pytest.raises(TypeError, match="float16, bfloat16, float32 or float64"):
            fn(x.int(), x.int(), "signal_noise_ratio")
        with pytest.raises(TypeError, match="share a dtype"):
            fn(x, x.double(), si)
        with pytest.raises(TypeError, match="int32 or int64"):
            fn(x, x, si, lengths=torch.zeros(2))
        with pytest.raises(TypeError, match="takes no argument 'zero_mean'"):
            fn(x, x, F.scale_invariant_signal_noise_ratio, zero_mean=True)
        with pytest.raises(TypeError, match="takes no argument 'filter_length'"):
            fn(x, x, si, filter_length=3)
        with pytest.raises(ValueError, match="fused metrics only"):
            fn(x, x, lambda p, t: (p * t).sum(-1), lengths=torch.zeros(2, dtype=torch.int32))
        with pytest.raises(RuntimeError, match=r"preds must be on an MI355X \(ROCm\) device.*no CPU fallback"):
            fn(x, x, si)
    with pytest.raises(ValueError, match="eval_func must be 'max' or 'min'"):
        pit(x, x, si, eval_func="mean")
    with pytest.raises(NotImplementedError, match="permutation-wise"):
        pit(x, x, si, mode="permutation-wise")
    with pytest.raises(ValueError, match="mode must be"):
        pit(x, x, si, mode="other")
    with pytest.raises(ValueError, match="must return a tensor of shape"):
        pit(x, x, lambda p, t: (p * t).sum())
    m = torch.zeros(2, 3, 3)
    for bad, err, msg in ((m[0], ValueError, "expects"), (torch.zeros(1, 9, 9), NotImplementedError, "PIT_MAX_SOURCES = 8"),
                          (m.half(), TypeError, "float32 or float64"), (m, RuntimeError, "no CPU fallback")):
        with pytest.raises(err, match=msg):
            F.pit_assignment(bad)
    with pytest.raises(ValueError, match="eval_func"):
        F.pit_assignment(m, "mean")
    for args, err, msg in (((x, torch.zeros(2, 2, dtype=torch.int64)), ValueError, "expects preds"),
                           ((x, torch.zeros(2, 3)), TypeError, "int32 or int64"),
                           ((x, torch.zeros(2, 3, dtype=torch.int64)), RuntimeError, "no CPU fallback")):
        with pytest.raises(err, match=msg):
            F.pit_permutate(*args)
    assert {"permutation_invariant_training", "pit_metric_matrix", "pit_assignment", "pit_permutate", "pit_tiles"} <= set(F.__all__)
    assert F.pit_tiles()[3] == F.PIT_MAX_SOURCES == 8
