"""F.forced_align on the MI355X against the float64 restatements of tests/forced_align_oracle.py.

Exact cases: log_probs = -k / 64 with integer k in [1, 255].  float64, float32, float16 and bfloat16 all hold these exactly and
every partial sum is exact in float64, so the Viterbi path is decided by the recurrence and its tie rule alone (ties are
frequent): paths must equal the oracle's element for element and scores the gathered elements bit for bit.

Random cases: log_softmax of seeded normals rounded to the dtype.  The returned path must collapse to the transcript, and its
total, recomputed in float64 from the stored inputs, must lie within 2 T_b^2 2^-52 max|lp| of the oracle's optimum: the
worst-order bound of T_b float64 additions of terms no larger than T_b max|lp|, derived from the inputs and not from the
kernel.  Every check prints the achieved fraction of its bound.

Impossible lengths and labels are exercised in tests/test_forced_align.py (CPU replay between canaries) only, never here."""
import functools

import numpy as np
import pytest
import torch

import forced_align_oracle as O
import audio_amd.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float32, torch.float64, torch.float16, torch.bfloat16]
INTS = [torch.int32, torch.int64]
CONFIGS, PF, BT, MAX_L = ((127, 4, 64), (511, 4, 256), (2047, 16, 256)), 4, 64, 2047      # test_tiles_are_the_exported_constants
SHAPES = O.exact_shapes(CONFIGS, PF, BT, MAX_L)


def bits(t):
    """The stored bits of a floating tensor, as integers."""
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def device_args(lp, targets, in_len, tg_len, dtype, tdtype, ldtype=None, offset=0):
    buf = torch.zeros(lp.size + offset, dtype=dtype, device=DEV)
    x = buf[offset:].view(lp.shape)
    x.copy_(torch.from_numpy(lp).to(dtype))
    assert x.is_contiguous() and x.storage_offset() == offset
    ldtype = ldtype or tdtype
    return (x, torch.from_numpy(np.ascontiguousarray(targets)).to(tdtype).to(DEV), torch.from_numpy(in_len).to(ldtype).to(DEV),
            torch.from_numpy(tg_len).to(ldtype).to(DEV))


@functools.lru_cache(maxsize=None)
def case(name):
    """The inputs of a named shape and the oracle's (paths, totals): built once, shared by every dtype."""
    args = O.exact_case(sum(map(ord, name)), **SHAPES[name])
    return args, O.expected(*args)


def check_exact(name, dtype, tdtype, ldtype=None, offset=0, defaults=False):
    (lp, targets, in_len, tg_len, blank), (want, _) = case(name)
    x, tg, il, tl = device_args(lp, targets, in_len, tg_len, dtype, tdtype, ldtype, offset)
    assert torch.equal(x.double().cpu(), torch.from_numpy(lp))                       # the dtype holds these inputs exactly
    paths, scores = F.forced_align(x, tg, blank=blank) if defaults else F.forced_align(x, tg, il, tl, blank)
    assert paths.shape == scores.shape == lp.shape[:2] and paths.dtype == tdtype and scores.dtype == dtype
    assert np.array_equal(paths.cpu().numpy(), want), name
    want_scores = torch.gather(x, 2, torch.from_numpy(want).to(DEV).unsqueeze(-1)).squeeze(-1)
    for b in range(lp.shape[0]):                                # the padding: blank (in `want`) and exactly zero
        want_scores[b, int(in_len[b]):] = 0
    assert torch.equal(bits(scores), bits(want_scores)), name


def test_tiles_are_the_exported_constants():
    assert F.forced_align_tiles() == (CONFIGS, PF, BT, MAX_L)


@pytest.mark.parametrize("tdtype", INTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_cases_equal_the_oracle(dtype, tdtype):
    for name in sorted(SHAPES):
        check_exact(name, dtype, tdtype)


def test_default_lengths_length_dtypes_and_an_offset_view():
    for name in ("T1_L0", "tight_run3", "L64", "T129_bt"):      # one example of full length: the defaults say the same
        check_exact(name, torch.float32, torch.int64, defaults=True)
    check_exact("ragged", torch.float32, torch.int32, ldtype=torch.int64)
    check_exact("ragged", torch.float16, torch.int64, ldtype=torch.int32)
    for dtype in DTYPES:                                        # log_probs at a non-zero element offset
        check_exact("ragged", dtype, torch.int32, offset=3)
        check_exact("L128", dtype, torch.int64, offset=1)


@pytest.mark.parametrize("shape,lens,dtypes", [
    ((3, 50, 12, 10), ([50, 31, 9], [10, 4, 0]), DTYPES),
    ((2, 300, 32, 150), ([300, 290], [150, 97]), [torch.float32, torch.bfloat16]),
    ((1, 1300, 16, 600), ([1300], [600]), [torch.float32, torch.float64]),
])
def test_random_cases_reach_the_optimum(shape, lens, dtypes):
    B, T, Cn, L = shape
    rng = np.random.default_rng(T)
    raw = torch.log_softmax(torch.from_numpy(rng.standard_normal((B, T, Cn)) * 3.0), dim=-1)
    targets = np.stack([O.random_target(rng, L, Cn, 0) for _ in range(B)])
    in_len, tg_len = np.asarray(lens[0], dtype=np.int64), np.asarray(lens[1], dtype=np.int64)
    for dtype in dtypes:
        lp = raw.to(dtype).to(torch.float64).numpy()            # what the tensor holds
        x, tg, il, tl = device_args(lp, targets, in_len, tg_len, dtype, torch.int32)
        paths, scores = F.forced_align(x, tg, il, tl)
        paths, scores = paths.cpu().numpy(), scores.double().cpu().numpy()
        for b in range(B):
            Tb, Lb = int(in_len[b]), int(tg_len[b])
            assert Tb >= Lb + O.repeats(targets[b, :Lb])
            assert O.is_alignment(paths[b, :Tb], targets[b, :Lb], 0)
            got, (_, best) = O.path_total(lp[b], paths[b, :Tb]), O.viterbi(lp[b, :Tb], targets[b, :Lb], 0)
            bound = 2.0 * Tb * Tb * 2.0 ** -52 * np.abs(lp[b, :Tb]).max()
            print(f"{dtype} {shape} example {b}: total {got:.6f}, optimum {best:.6f}, {abs(got - best) / bound:.4f} of the bound")
            assert abs(got - best) <= bound
            assert np.array_equal(scores[b, :Tb], lp[b, np.arange(Tb), paths[b, :Tb]])
            assert np.all(paths[b, Tb:] == 0) and np.all(scores[b, Tb:] == 0.0)


def test_poisoned_padding_changes_nothing():
    (lp, targets, in_len, tg_len, blank), (want, _) = case("ragged")
    bad_lp, bad_t = lp.copy(), targets.copy()
    for b in range(3):
        bad_lp[b, in_len[b]:] = (np.nan, np.inf, -np.inf)[b]
        bad_t[b, tg_len[b]:] = (-7, 2 ** 30, blank)[b]
    assert not np.array_equal(bad_t, targets)
    x, tg, il, tl = device_args(bad_lp, bad_t, in_len, tg_len, torch.float32, torch.int32)
    paths, scores = F.forced_align(x, tg, il, tl, blank)
    assert np.array_equal(paths.cpu().numpy(), want)
    for b in range(3):
        assert bool((scores[b, int(in_len[b]):] == 0).all())


def test_two_calls_give_the_same_bits():
    (lp, targets, in_len, tg_len, blank), _ = case("T700_L300")
    x, tg, il, tl = device_args(lp, targets, in_len, tg_len, torch.float32, torch.int64)
    a, b = F.forced_align(x, tg, il, tl, blank), F.forced_align(x, tg, il, tl, blank)
    assert torch.equal(a[0], b[0]) and torch.equal(bits(a[1]), bits(b[1]))


def test_graph_capture_and_replay():
    """Lengths and labels are read on the device: one capture serves new values in the same buffers."""
    (lp0, targets0, il0, tl0, blank), _ = case("ragged")
    lp1, targets1, il1, tl1, _ = O.exact_case(99, 20, 6, 6, lens=([13, 20, 4], [3, 6, 1]))
    want1, _ = O.expected(lp1, targets1, il1, tl1, blank)
    x, tg, il, tl = device_args(lp0, targets0, il0, tl0, torch.float32, torch.int32)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                 # warm up off the default stream, as captures ask
        for _ in range(2):
            F.forced_align(x, tg, il, tl, blank)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                              # one stream, no parallel branches
        paths, scores = F.forced_align(x, tg, il, tl, blank)
    new = device_args(lp1, targets1, il1, tl1, torch.float32, torch.int32)
    for dst, src in zip((x, tg, il, tl), new):
        dst.copy_(src)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(paths.cpu().numpy(), want1)
    eager = F.forced_align(*new, blank)
    assert torch.equal(paths, eager[0]) and torch.equal(bits(scores), bits(eager[1]))


def test_merge_tokens_of_a_device_result_equals_its_cpu_copy():
    (lp, targets, in_len, tg_len, blank), (want, _) = case("T129_bt")
    for dtype in (torch.float32, torch.bfloat16):
        x, tg, il, tl = device_args(lp, targets, in_len, tg_len, dtype, torch.int64)
        paths, scores = F.forced_align(x, tg, il, tl, blank)
        spans = F.merge_tokens(paths[0], scores[0], blank)
        assert spans == F.merge_tokens(paths[0].cpu(), scores[0].cpu(), blank)
        assert [s.token for s in spans] == targets[0].tolist()
        assert all(len(s) >= 1 and s.score == lp[0, s.start:s.end, s.token].mean() for s in spans)
