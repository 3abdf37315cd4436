"""audio_amd.models.decoder on the MI355X against the float64 oracle of tests/ctc_decoder_oracle.py.

Decided cases: log_softmax of seeded normals times a scale, rounded to float32 / float64; the oracle gets what the tensor
holds.  Tokens and lengths must equal the oracle's exactly and scores lie within 16 n 2^-52 S of its scores (n: the example's
unskipped frames, S: the largest max(1, |score|) in any beam): at most 4 additions and 4 logaddexp per prefix and frame, each a
few ulp, and logaddexp is 1-Lipschitz in its inputs, so the errors add up -- a bound from the inputs, never from the kernel's
output.  A case is decided when the oracle's smallest gap between adjacent scores at any cut-off exceeds 1000 x that bound; the
recorded seeds all are (asserted here and in test_ctc_decoder.py), so no case is left out.  Every check prints the achieved
fraction of its bound.

Half precision gives many exact score ties, which an oracle cannot decide: there the result must equal the float32 run of the
same values bit for bit.  Flagged lengths are exercised in tests/test_ctc_decoder.py (CPU replay between canaries) only."""
import functools

import numpy as np
import pytest
import torch

import ctc_decoder_oracle as O
from audio_amd.models import CUCTCDecoder, CUCTCHypothesis, ctc_beam_search, cuda_ctc_decoder

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float32, torch.float64, torch.float16, torch.bfloat16]


def name_of(dtype):
    return str(dtype).split(".")[1]


def on_device(lp, dtype, offset=0):
    buf = torch.zeros(lp.size + offset, dtype=dtype, device=DEV)
    x = buf[offset:].view(lp.shape)
    x.copy_(torch.from_numpy(np.ascontiguousarray(lp)).to(dtype))
    assert x.is_contiguous() and x.storage_offset() == offset
    return x


def lens_on_device(lengths, ldtype=torch.int32):
    return torch.tensor(list(lengths), dtype=ldtype, device=DEV)


def same_bits(a, b):
    return all(torch.equal(x, y) for x, y in zip(a[:2], b[:2])) and torch.equal(a[2].view(torch.int64), b[2].view(torch.int64))


@functools.lru_cache(maxsize=None)
def case(name, dtype, thr=O.THR):
    """The inputs of a named case in `dtype` and the oracle's results: built once."""
    lp, lengths, K = O.case(name, name_of(dtype))
    want = O.expected(lp, lengths, K, 0, thr)
    assert all(O.decided(r) for r in want), name
    return lp, lengths, K, want


def check_against_oracle(got, want, nbest, what):
    tokens, lens, scores = (t.cpu().numpy() for t in got)
    assert tokens.dtype == np.int32 and lens.dtype == np.int32 and scores.dtype == np.float64
    worst = 0.0
    for b, res in enumerate(want):
        assert O.decided(res), (what, b, res.gap, O.bound(res))
        for h in range(nbest):
            if h < len(res.hyps):
                toks, score = res.hyps[h]
                assert lens[b, h] == len(toks) and tuple(tokens[b, h, :len(toks)]) == toks, (what, b, h, toks, tokens[b, h])
                assert not tokens[b, h, len(toks):].any()
                assert abs(scores[b, h] - score) <= O.bound(res), (what, b, h, scores[b, h], score, O.bound(res))
                worst = max(worst, abs(scores[b, h] - score) / O.bound(res))
            else:
                assert lens[b, h] == -1 and scores[b, h] == -np.inf and not tokens[b, h].any()
    print("%s: %.4f of the bound" % (what, worst))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("name", sorted(O.CASES))
def test_decided_cases_equal_the_oracle(name, dtype):
    lp, lengths, K, want = case(name, dtype)
    nbest = min(K, 4)
    got = ctc_beam_search(on_device(lp, dtype), lens_on_device(lengths), beam_size=K, nbest=nbest)
    assert got[0].shape == (3, nbest, lp.shape[1]) and got[1].shape == got[2].shape == (3, nbest)
    check_against_oracle(got, want, nbest, "%s %s" % (name, name_of(dtype)))


def test_nothing_skipped():
    lp, lengths, K, want = case("general", torch.float32, 0.0)
    got = ctc_beam_search(on_device(lp, torch.float32), lens_on_device(lengths), K, K, blank_skip_threshold=0.0)
    check_against_oracle(got, want, K, "general, threshold 0")


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("shape,K", [((3, 50, 32), 8), ((2, 64, 300), 10)])
def test_half_precision_equals_its_float32_run(shape, K, dtype):
    B, T, V = shape
    x = on_device(O.emissions(11, B, T, V, "float32"), dtype)
    lengths = lens_on_device(O.lengths_of(T)[:B])
    got, ref = ctc_beam_search(x, lengths, K, K), ctc_beam_search(x.float(), lengths, K, K)
    assert same_bits(got, ref)
    assert int(got[1].max()) > 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_tie_takes_the_smaller_token(dtype):
    """K = 1; frame 0 holds its two best non-blank tokens (2 and 3) at one value, then blank-heavy frames that are not skipped."""
    p = np.array([[0.1, 0.05, 0.4, 0.4, 0.05], [0.6, 0.1, 0.1, 0.1, 0.1], [0.7, 0.1, 0.05, 0.05, 0.1]])
    x = on_device(np.log(p)[None], dtype)
    assert bool(x[0, 0, 2] == x[0, 0, 3]) and bool(x[0, 0, 2] > x[0, 0, 1])
    tokens, lens, _ = ctc_beam_search(x, None, 1, 1, blank_skip_threshold=0.0)
    assert lens.tolist() == [[1]] and tokens[0, 0].tolist() == [2, 0, 0]
    assert O.search(x[0].double().cpu().numpy(), 1, 0, 0.0).hyps[0][0] == (2,)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_own_last_token_outside_the_record_wins_its_tie(dtype):
    """K = 1: three extensions of one prefix with bit-equal scores, the smallest token being the prefix's own last token, which
    is not among the frame's K + 1 largest (ctc_decoder_oracle.own_token_case)."""
    lp = O.own_token_case()
    assert O.search(lp[0], 1, 0, 0.0).hyps[0] == ((1, 1), -2.0 ** 40 - 1)
    x = on_device(lp, dtype)
    assert np.array_equal(x.double().cpu().numpy(), lp)
    tokens, lens, scores = ctc_beam_search(x, None, 1, 1, blank_skip_threshold=0.0)
    assert lens.tolist() == [[2]] and tokens[0, 0].tolist() == [1, 1, 0] and scores.tolist() == [[-2.0 ** 40 - 1]]


def test_edges():
    one = O.emissions(3, 1, 1, 6, "float32", blank_share=0.0)                                            # T = 1
    check_against_oracle(ctc_beam_search(on_device(one, torch.float32), lens_on_device([1]), 4, 4), O.expected(one, [1], 4), 4, "T = 1")
    lp = O.emissions(5, 3, 12, 6, "float32")
    x = on_device(lp, torch.float32)
    got = ctc_beam_search(x, lens_on_device([0, 12, 5]), 4, 2)                                           # an empty example
    assert got[1][0].tolist() == [0, -1] and got[2][0].tolist() == [0.0, -np.inf] and not bool(got[0][0].any())
    check_against_oracle(got, O.expected(lp, [0, 12, 5], 4), 2, "an empty example")
    tokens, lens, scores = ctc_beam_search(x, lens_on_device([12, 12, 12]), 4, 4, blank_skip_threshold=-1e9)   # every frame skipped
    assert lens.tolist() == [[0, -1, -1, -1]] * 3 and scores[:, 0].tolist() == [0.0] * 3 and not bool(tokens.any())
    two = O.emissions(9, 1, 1, 2, "float32", blank_share=0.0)                                            # 2 live prefixes, nbest 4
    got = ctc_beam_search(on_device(two, torch.float32), lens_on_device([1]), 4, 4, blank_skip_threshold=0.0)
    assert sorted(got[1][0].tolist()) == [-1, -1, 0, 1] and got[2][0, 2:].tolist() == [-np.inf] * 2
    check_against_oracle(got, O.expected(two, [1], 4, 0, 0.0), 4, "fewer live prefixes than nbest")


def test_default_lengths_int64_lengths_an_offset_view_and_a_blank():
    lp, lengths, K, want = case("general", torch.float32)
    full = O.expected(lp, [lp.shape[1]] * 3, K)
    check_against_oracle(ctc_beam_search(on_device(lp, torch.float32), None, K, 2), full, 2, "lengths=None")
    check_against_oracle(ctc_beam_search(on_device(lp, torch.float32), lens_on_device(lengths, torch.int64), K, 2), want, 2, "int64")
    for dtype, offset in ((torch.float32, 3), (torch.float64, 1)):
        lp, lengths, K, want = case("general", dtype)
        got = ctc_beam_search(on_device(lp, dtype, offset), lens_on_device(lengths), K, 2)
        check_against_oracle(got, want, 2, "offset %d" % offset)
    lp = O.emissions(13, 2, 20, 7, "float32", blank=4)
    want = O.expected(lp, [20, 9], 5, 4)
    assert all(O.decided(r) for r in want)
    check_against_oracle(ctc_beam_search(on_device(lp, torch.float32), lens_on_device([20, 9]), 5, 5, blank=4), want, 5, "blank 4")


def test_poisoned_padding_changes_nothing():
    lp, lengths, K, _ = case("general", torch.float32)
    bad = lp.copy()
    for b in range(3):
        bad[b, lengths[b]:] = (np.nan, np.inf, -np.inf)[b]
    assert not np.array_equal(bad, lp, equal_nan=True)
    ln = lens_on_device(lengths)
    assert same_bits(ctc_beam_search(on_device(bad, torch.float32), ln, K, K), ctc_beam_search(on_device(lp, torch.float32), ln, K, K))


def test_two_calls_give_the_same_bits():
    lp, lengths, K, _ = case("k_limit", torch.float32)
    x, ln = on_device(lp, torch.float32), lens_on_device(lengths)
    assert same_bits(ctc_beam_search(x, ln, K, K), ctc_beam_search(x, ln, K, K))


def test_graph_capture_and_replay():
    """Lengths are read on the device: one capture serves new values in the same buffers."""
    lp0, lengths0, K, _ = case("general", torch.float32)
    lp1 = O.emissions(77, 3, lp0.shape[1], lp0.shape[2], "float32")
    lengths1 = [31, 50, 7]
    x, ln = on_device(lp0, torch.float32), lens_on_device(lengths0)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                 # warm up off the default stream, as captures ask
        for _ in range(2):
            ctc_beam_search(x, ln, K, 3)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                              # one stream, no parallel branches
        got = ctc_beam_search(x, ln, K, 3)
    x.copy_(on_device(lp1, torch.float32))
    ln.copy_(lens_on_device(lengths1))
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(got, ctc_beam_search(x, ln, K, 3))
    check_against_oracle(got, O.expected(lp1, lengths1, K), 3, "replay")


def test_the_decoder_object():
    lp, lengths, K, want = case("general", torch.float32)
    vocab = ["<blk>"] + ["w%d" % i for i in range(1, lp.shape[2])]
    x, ln = on_device(lp, torch.float32), lens_on_device(lengths)
    out = cuda_ctc_decoder(vocab, nbest=4, beam_size=K)(x, ln)
    tokens, lens, scores = (t.cpu() for t in ctc_beam_search(x, ln, K, 4))
    assert isinstance(out, list) and len(out) == 3
    for b, hyps in enumerate(out):
        assert len(hyps) == int((lens[b] >= 0).sum()) == min(4, len(want[b].hyps))
        for h, hyp in enumerate(hyps):
            assert isinstance(hyp, CUCTCHypothesis)
            assert hyp.tokens == tokens[b, h, :int(lens[b, h])].tolist() == list(want[b].hyps[h][0])
            assert hyp.words == [vocab[t] for t in hyp.tokens] and hyp.score == float(scores[b, h])
        assert [h.score for h in hyps] == sorted((h.score for h in hyps), reverse=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    assert CUCTCDecoder(vocab, beam_size=K, nbest=4, cuda_stream=side)(x, ln) == out
    torch.cuda.current_stream().wait_stream(side)
    one = cuda_ctc_decoder(["-", "a"], nbest=4, beam_size=4)(on_device(O.emissions(9, 1, 1, 2, "float32", blank_share=0.0), torch.float32),
                                                             lens_on_device([1]))
    assert len(one) == 1 and len(one[0]) == 2                                                           # missing hypotheses are left out
