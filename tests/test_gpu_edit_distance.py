"""F.edit_distance_batch / F.edit_distance on the MI355X against the pure-Python definition of tests/edit_distance_oracle.py:
integers only, so every field of every pair must equal the oracle's element for element.  The shapes follow
F.edit_distance_tiles() (rows per lane, wave seams, every configuration's largest width and the next, the limit); the longest
pair is 4096 x 64 cells.

Impossible lengths other than the decoder's -1 are exercised in tests/test_edit_distance.py (CPU replay between canaries) only,
never here."""
import numpy as np
import pytest
import torch

import edit_distance_oracle as O
import audio_amd.functional as F
from audio_amd.models.decoder import ctc_beam_search

pytestmark = pytest.mark.gpu
DEV = "cuda"
INTS = [torch.int32, torch.int64]
CONFIGS, LIMITS = ((256, 4, 64), (1024, 4, 256), (4096, 16, 256)), (4096, 32767)      # test_tiles_are_the_exported_constants
SHAPES = O.exact_shapes(CONFIGS, LIMITS)


def dev(a, dtype=torch.int32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


def test_tiles_are_the_exported_constants():
    assert F.edit_distance_tiles() == (CONFIGS,) + LIMITS == (CONFIGS, F.EDIT_MAX_REF, F.EDIT_MAX_HYP)


@pytest.mark.parametrize("hd,rd", [(a, b) for a in INTS for b in INTS], ids=lambda d: str(d).split(".")[-1])
def test_every_exact_shape_equals_the_definition(hd, rd):
    """One call per shape (the width picks the configuration), all four fields and the distance-only output."""
    for name in sorted(SHAPES):
        M, N = SHAPES[name]
        ref, hyp, want = O.case(name, M, N)
        h, r = dev(np.array(hyp, dtype=np.int64).reshape(1, N), hd), dev(np.array(ref, dtype=np.int64).reshape(1, M), rd)
        got = F.edit_distance_batch(h, r, return_ops=True)
        assert got.shape == (1, 4) and got.dtype == torch.int32
        assert tuple(got[0].tolist()) == want, (name, got, want)
        dist = F.edit_distance_batch(h, r)
        assert dist.shape == (1,) and dist.dtype == torch.int32 and int(dist[0]) == want[0], name


@pytest.mark.parametrize("name", ["M7_N65", "M257_N65", "M1025_N63"], ids=str)                 # one per configuration
@pytest.mark.parametrize("ld", INTS, ids=lambda d: str(d).split(".")[-1])
def test_pair_inside_wider_tensors_at_an_element_offset(name, ld):
    M, N = SHAPES[name]
    ref, hyp, want = O.case(name, M, N)
    hyps = np.full((2, N + 3), 1234, dtype=np.int64)
    refs = np.full((2, M), 4321, dtype=np.int64)
    hyps[1, :N], refs[1, :M] = hyp, ref
    refs[0, :5], hyps[0, :4] = [1, 2, 3, 4, 5], [1, 3, 4, 5]
    for dtype in INTS:
        buf = torch.zeros(hyps.size + 1, dtype=dtype, device=DEV)
        h = buf[1:].view(hyps.shape)
        h.copy_(dev(hyps, dtype))
        assert h.is_contiguous() and h.storage_offset() == 1
        got = F.edit_distance_batch(h, dev(refs, dtype), dev([4, N], ld), dev([5, M], ld), return_ops=True)
        assert got.tolist() == [[1, 0, 1, 0], list(want)]


def test_int64_tokens_are_compared_as_integers():
    ref, hyp, want = O.high_word_pair()
    got = F.edit_distance_batch(dev([hyp], torch.int64), dev([ref], torch.int64), return_ops=True)
    assert tuple(got[0].tolist()) == want
    small = [t % O.HIGH for t in ref] + [-1, -2]
    assert int(F.edit_distance_batch(dev(small, torch.int32), dev(small, torch.int64))) == 0


def test_every_length_of_a_ragged_batch():
    hyps, refs, hl, rl, want = O.grid_batch()
    got = F.edit_distance_batch(dev(hyps), dev(refs), dev(hl), dev(rl, torch.int64), return_ops=True)
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(F.edit_distance_batch(dev(hyps), dev(refs), dev(hl), dev(rl, torch.int64)).cpu().numpy(), want[:, 0])


@pytest.mark.parametrize("M", [9, 257, 1025], ids=lambda m: "M%d" % m)                          # one per configuration
def test_minus_one_lengths_in_a_ragged_nbest_batch(M):
    hyps, refs, hl, rl, want = O.ragged_batch(M=M)
    assert (hl == -1).any()
    h, r, hlen, rlen = dev(hyps), dev(refs, torch.int64), dev(hl), dev(rl)
    got = F.edit_distance_batch(h, r, hlen, rlen, return_ops=True)
    assert got.shape == hyps.shape[:2] + (4,) and np.array_equal(got.cpu().numpy(), want)
    again = F.edit_distance_batch(h, r, hlen, rlen, return_ops=True)
    assert torch.equal(got, again)                                                  # two calls give identical bits
    for b, k in ((0, 1), (1, 2), (2, 3)):                                            # row p of a batch equals the pair alone
        alone = F.edit_distance_batch(h[b, k], r[b], hlen[b, k], rlen[b], return_ops=True)
        assert alone.shape == (4,) and torch.equal(alone, got[b, k])
    empty = F.edit_distance_batch(h[:0], r[:0], hlen[:0], rlen[:0], return_ops=True)
    assert empty.shape == (0, hyps.shape[1], 4)


def test_widths_of_zero_are_legal():
    z = torch.zeros((2, 0), dtype=torch.int32, device=DEV)
    r = dev([[1, 2, 3], [4, 5, 6]])
    assert F.edit_distance_batch(z, r, return_ops=True).tolist() == [[3, 0, 3, 0]] * 2
    assert F.edit_distance_batch(r, z, return_ops=True).tolist() == [[3, 0, 0, 3]] * 2
    assert F.edit_distance_batch(z, z).tolist() == [0, 0]


def test_edit_distance_on_tensors_strings_and_word_lists():
    ref, hyp, want = O.case("M257_N65", *SHAPES["M257_N65"])
    assert F.edit_distance(dev(ref), dev(hyp, torch.int64)) == want[0]
    for a, b in (("kitten", "sitting"), ("", "abc"), ("abc", ""), ("", ""), ("flaw", "lawn"),
                 ("the quick brown fox".split(), "the quack brown box jumps".split()), (("a", "b"), ["a", "b"])):
        got = F.edit_distance(a, b)
        assert isinstance(got, int) and got == O.distance(list(a), list(b)), (a, b, got)
    assert F.edit_distance("kitten", "sitting") == 3


def test_graph_capture_of_a_first_call_and_replay():
    """Lengths and tokens are read on the device and nothing is cached on the host: the capture needs no warm-up call, and
    one capture serves new contents of the same buffers.  (A width no other test of this file uses.)"""
    rng = np.random.default_rng(4)
    B, nbest, N, M = 3, 2, 37, 29

    def make(seed):
        g = np.random.default_rng(seed)
        hyps, refs = g.integers(0, 3, (B, nbest, N)), g.integers(0, 3, (B, M))
        hl, rl = g.integers(0, N + 1, (B, nbest)), g.integers(0, M + 1, (B,))
        hl[1, 1] = -1
        want = np.array([[O.ops(list(refs[b, :rl[b]]), list(hyps[b, k, :hl[b, k]])) if hl[b, k] >= 0 else (-1,) * 4
                          for k in range(nbest)] for b in range(B)])
        return (hyps, refs, hl, rl), want

    (a0, want0), (a1, want1) = make(rng.integers(1 << 30)), make(rng.integers(1 << 30))
    bufs = [dev(x) for x in a0]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                              # one stream, one launch, no parallel branches
        out = F.edit_distance_batch(*bufs, return_ops=True)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want0)
    for dst, src in zip(bufs, a1):
        dst.copy_(dev(src))
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want1)
    assert torch.equal(out, F.edit_distance_batch(*bufs, return_ops=True))


def test_beam_search_output_goes_straight_in():
    """ctc_beam_search(emis, beam_size=4, nbest=3) on a (4, 60, 8) emission: its tensors, -1 lengths included, against (4, U)
    transcripts with no copy, checked against the oracle on the host copies."""
    g = torch.Generator().manual_seed(12)
    emis = torch.log_softmax(3.0 * torch.randn(4, 60, 8, generator=g), dim=-1).to(DEV)
    emis[3, :, 0] = 0.0                                        # every frame of the last example is skipped: one empty hypothesis
    toks, tok_lens, _ = ctc_beam_search(emis, beam_size=4, nbest=3)
    U = 25
    refs = torch.randint(1, 8, (4, U), generator=g).to(DEV)
    ref_lens = torch.tensor([25, 17, 0, 9], device=DEV)
    got = F.edit_distance_batch(toks, refs, tok_lens, ref_lens, return_ops=True)
    assert got.shape == (4, 3, 4)
    t, tl, r, rl = toks.cpu().tolist(), tok_lens.cpu().tolist(), refs.cpu().tolist(), ref_lens.cpu().tolist()
    assert any(n == -1 for row in tl for n in row) and any(n > 0 for row in tl for n in row)
    want = [[list(O.ops(r[b][:rl[b]], t[b][k][:tl[b][k]])) if tl[b][k] >= 0 else [-1] * 4 for k in range(3)] for b in range(4)]
    assert got.tolist() == want
    best = F.edit_distance_batch(toks, refs, tok_lens, ref_lens)
    assert best.tolist() == [[w[0] for w in row] for row in want]
