"""CTC prefix beam search without a GPU: the float64 oracle of tests/ctc_decoder_oracle.py against exhaustive enumeration, the
recorded cases' decidedness, a CPU replay of csrc/ctc_decoder.h (row pass, beam pass and its backtrack; the four dtype paths,
both length dtypes) against the oracle with every buffer between canaries -- flagged lengths and non-finite log-probabilities
included -- and the public surface of audio_amd.models.decoder."""
import ctypes as C
import functools
import inspect
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import ctc_decoder_oracle as O
import audio_amd.models.decoder as D
from audio_amd.models import CUCTCDecoder, CUCTCHypothesis, ctc_beam_search, cuda_ctc_decoder

HERE = os.path.dirname(os.path.abspath(__file__))
SIM_SRC = os.path.join(HERE, "cpu_sim", "sim_ctc_decoder.cpp")
SIM_OUT = os.path.join(HERE, "cpu_sim", "_build", "libaamd_sim_ctc_decoder.so")
HDRS = [os.path.join(os.path.dirname(HERE), "audio_amd", "csrc", h)
        for h in ("ctc_decoder.h", "rnnt_loss.h", "wave_augment.h", "spec_augment.h", "hd.h")]
CODE = {torch.float32: 0, torch.float64: 1, torch.float16: 2, torch.bfloat16: 3}
DTYPES = [torch.float32, torch.float64, torch.float16, torch.bfloat16]
MAX_BEAM, ROW_THREADS, BEAM_THREADS = 32, 256, 256             # test_sim_constants_are_the_exported_ones
PAD = 64
CANARY = 77

_sim = None


def sim():
    global _sim
    if _sim is None:
        newest = max(os.path.getmtime(p) for p in [SIM_SRC] + HDRS)
        if not os.path.exists(SIM_OUT) or newest > os.path.getmtime(SIM_OUT):
            os.makedirs(os.path.dirname(SIM_OUT), exist_ok=True)
            tmp = "%s.tmp.%d" % (SIM_OUT, os.getpid())
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", SIM_SRC, "-o", tmp])
            os.replace(tmp, SIM_OUT)
        _sim = C.CDLL(SIM_OUT)
        _sim.sim_cd_workspace.restype = C.c_int64
        _sim.sim_cd_workspace.argtypes = [C.c_int64] * 3
    return _sim


def _guarded(n, dtype, offset=0):
    """(whole buffer, the n elements `offset` past the leading canaries)."""
    buf = torch.full((n + 2 * PAD + offset,), CANARY, dtype=dtype)
    return buf, buf[PAD + offset:PAD + offset + n]


def _canaries_intact(buf, n, offset=0):
    return bool((buf[:PAD + offset] == CANARY).all()) and bool((buf[PAD + offset + n:] == CANARY).all())


def _p(t):
    return C.c_void_p(t.data_ptr())


def run_sim(lp, lengths, beam, nbest, blank=0, thr=O.THR, dtype=torch.float32, ldtype=torch.int32, offset=0):
    """lp (B, T, V) float64 numpy (rounded to `dtype` here) -> (tokens (B, N, T), lengths (B, N), scores (B, N)) as numpy; asserts
    the canaries round every buffer the replay writes, and round its input."""
    s = sim()
    B, T, V = lp.shape
    xbuf, x = _guarded(lp.size, dtype, offset)
    x.copy_(torch.from_numpy(np.ascontiguousarray(lp)).reshape(-1).to(dtype))
    ln = torch.tensor(list(lengths), dtype=ldtype)
    nws = int(s.sim_cd_workspace(B, T, beam))
    assert nws > 0 and nws % 16 == 0
    wbuf, ws = _guarded(nws, torch.uint8)
    tbuf, tokens = _guarded(B * nbest * T, torch.int32)
    lbuf, out_len = _guarded(B * nbest, torch.int32)
    sbuf, scores = _guarded(B * nbest, torch.float64)
    dims = (C.c_int64 * 3)(B, T, V)
    rc = s.sim_ctc_beam_search(CODE[dtype], _p(x), _p(ln), int(ldtype == torch.int64), dims, blank, beam, nbest, C.c_double(thr),
                               _p(ws), _p(tokens), _p(out_len), _p(scores))
    assert rc == 0
    assert _canaries_intact(wbuf, nws) and _canaries_intact(tbuf, B * nbest * T) and _canaries_intact(lbuf, B * nbest)
    assert _canaries_intact(sbuf, B * nbest) and _canaries_intact(xbuf, lp.size, offset)
    return (tokens.reshape(B, nbest, T).numpy().copy(), out_len.reshape(B, nbest).numpy().copy(),
            scores.reshape(B, nbest).numpy().copy())


def held(lp, dtype):
    """What a tensor of `dtype` holds of lp, in float64."""
    return torch.from_numpy(np.ascontiguousarray(lp)).to(dtype).to(torch.float64).numpy()


def check_against_oracle(got, want, nbest, T):
    """Tokens and lengths equal the oracle's, scores within its operation-count bound; returns the largest achieved fraction."""
    tokens, lens, scores = got
    worst = 0.0
    for b, res in enumerate(want):
        for h in range(nbest):
            if h < len(res.hyps):
                toks, score = res.hyps[h]
                assert lens[b, h] == len(toks) and tuple(tokens[b, h, :len(toks)]) == toks, (b, h, toks, tokens[b, h])
                assert not tokens[b, h, len(toks):].any()
                assert abs(scores[b, h] - score) <= O.bound(res), (b, h, scores[b, h], score, O.bound(res))
                worst = max(worst, abs(scores[b, h] - score) / O.bound(res))
            else:
                assert lens[b, h] == -1 and scores[b, h] == -np.inf and not tokens[b, h].any()
    return worst


@functools.lru_cache(maxsize=None)
def case(name, dtype, thr=O.THR):
    """The inputs of a named case in `dtype` and the oracle's results: built once."""
    lp, lengths, K = O.case(name, str(dtype).split(".")[1])
    return lp, lengths, K, O.expected(lp, lengths, K, 0, thr)


# ---- the oracle ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T,V", [(4, 3), (5, 3), (4, 4)])
def test_oracle_with_an_unbounded_beam_is_the_exact_posterior(T, V):
    for blank in (0, V - 1):
        lp = O.emissions(7 * T + V, 1, T, V, "float64", blank, 1.0, 0.0)[0]
        want = O.brute(lp, blank)
        got = dict(O.search(lp, 10 ** 9, blank, math.inf).hyps)
        assert set(got) == set(want)
        for seq, mass in want.items():
            assert abs(got[seq] - mass) <= 1e-12, (seq, got[seq], mass)
        assert abs(math.fsum(math.exp(v) for v in got.values()) - 1.0) <= 1e-12


@pytest.mark.parametrize("name", sorted(O.CASES))
def test_every_recorded_case_is_decided(name):
    """The smallest gap between adjacent scores at any cut-off exceeds 1000 x the score bound: a condition on the inputs."""
    for dtype in (torch.float32, torch.float64):
        for thr in (O.THR, 0.0):
            for res in case(name, dtype, thr)[3]:
                assert O.decided(res), (name, dtype, thr, res.gap, O.bound(res))
                assert res.hyps and res.frames >= 1


def test_half_precision_emissions_tie_exactly():
    """Why the half-precision GPU test compares with the float32 run instead of the oracle."""
    gaps = [res.gap for name in ("general", "few_tokens", "full_beam") for dt in ("float16", "bfloat16")
            for res in O.expected(*O.case(name, dt)[:3])]
    assert min(gaps) == 0.0


# ---- CPU replay of csrc/ctc_decoder.h ----------------------------------------------------------------------------------------

def test_sim_constants_are_the_exported_ones():
    s = sim()
    assert (s.sim_cd_max_beam(), s.sim_cd_row_threads(), s.sim_cd_beam_threads()) == (MAX_BEAM, ROW_THREADS, BEAM_THREADS)
    assert D.CTC_DECODER_MAX_BEAM == MAX_BEAM
    for K in (1, 10, 32):
        assert D.ctc_decoder_tiles(K) == (MAX_BEAM, ROW_THREADS, BEAM_THREADS, s.sim_cd_record_slots(K), s.sim_cd_candidates(K))
        assert (s.sim_cd_record_slots(K), s.sim_cd_candidates(K)) == (K + 1, K * (K + 3))
    from audio_amd import _lib
    for B, T, K in ((3, 50, 8), (1, 1, 1), (2, 1500, 32)):
        assert int(_lib.lib().aamd_ctc_decoder_workspace(B, T, 32, K)) == s.sim_cd_workspace(B, T, K) > 0
    assert int(_lib.lib().aamd_ctc_decoder_workspace(1, 10, 32, 33)) == 0 == s.sim_cd_workspace(1, 10, 33)
    assert int(_lib.lib().aamd_ctc_decoder_workspace(1, 10, 1, 4)) == 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("name", sorted(O.CASES))
def test_sim_equals_the_oracle_on_the_decided_cases(name, dtype):
    lp, lengths, K, want = case(name, dtype)
    nbest = min(K, 4)
    worst = check_against_oracle(run_sim(lp, lengths, K, nbest, dtype=dtype), want, nbest, lp.shape[1])
    print("%s %s: %.3f of the bound" % (name, dtype, worst))


def test_sim_small_random_cases():
    """80 seeded shapes with V <= 6, K <= 6, T <= 44, any blank, both thresholds: small beams over small vocabularies drop prefixes
    and take them back, so a prefix gets a second node (the replay's driver counts them) and entries whose hashes agree while
    their nodes differ are compared token by token."""
    s = sim()
    s.sim_cd_returned_prefixes.restype = C.c_long
    before = s.sim_cd_returned_prefixes()
    for seed in range(80):
        rng = np.random.default_rng(seed)
        V, K, T = int(rng.integers(2, 7)), int(rng.integers(1, 7)), int(rng.integers(1, 45))
        blank, scale = int(rng.integers(0, V)), float(rng.choice([0.5, 1.5, 3.0]))
        lp = O.emissions(seed, 2, T, V, "float64", blank, scale, 0.3)
        lengths = [T, int(rng.integers(0, T + 1))]
        thr = float(rng.choice([O.THR, 0.0]))
        want = O.expected(lp, lengths, K, blank, thr)
        assert all(O.decided(r) for r in want), seed
        check_against_oracle(run_sim(lp, lengths, K, K, blank, thr, torch.float64), want, K, T)
    returned = s.sim_cd_returned_prefixes() - before
    print("prefixes that came back into a beam: %d" % returned)
    assert returned >= 20


def test_sim_nothing_skipped_int64_lengths_and_an_offset():
    lp, lengths, K, want = case("general", torch.float32, 0.0)
    check_against_oracle(run_sim(lp, lengths, K, K, thr=0.0, ldtype=torch.int64, offset=3), want, K, lp.shape[1])
    assert max(len(r.hyps) for r in want) == K


@pytest.mark.parametrize("dtype", DTYPES)
def test_sim_half_precision_equals_its_float32_run(dtype):
    lp = held(O.emissions(11, 3, 50, 32, "float32"), dtype)
    got = run_sim(lp, O.lengths_of(50), 8, 8, dtype=dtype, offset=1)
    ref = run_sim(lp, O.lengths_of(50), 8, 8, dtype=torch.float32)
    for g, r in zip(got, ref):
        assert np.array_equal(g.view(np.int64) if g.dtype == np.float64 else g, r.view(np.int64) if r.dtype == np.float64 else r)


def tie_case():
    """K = 1; frame 0 holds its two best non-blank tokens (2 and 3) at one value, then blank-heavy frames that are not skipped."""
    p = np.array([[0.1, 0.05, 0.4, 0.4, 0.05], [0.6, 0.1, 0.1, 0.1, 0.1], [0.7, 0.1, 0.05, 0.05, 0.1]])
    return np.log(p)[None]


@pytest.mark.parametrize("dtype", DTYPES)
def test_sim_tie_takes_the_smaller_token(dtype):
    lp = held(tie_case(), dtype)
    assert lp[0, 0, 2] == lp[0, 0, 3] > lp[0, 0, 1]
    tokens, lens, _ = run_sim(lp, [3], 1, 1, thr=0.0, dtype=dtype)
    assert lens[0, 0] == 1 and tokens[0, 0, 0] == 2
    assert O.search(lp[0], 1, 0, 0.0).hyps[0][0] == (2,)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_sim_own_last_token_outside_the_record_wins_its_tie(dtype):
    lp = O.own_token_case()
    assert np.array_equal(held(lp, dtype), lp)
    res = O.search(lp[0], 1, 0, 0.0)
    assert res.hyps[0] == ((1, 1), -2.0 ** 40 - 1) and res.gap == 0.0
    tokens, lens, scores = run_sim(lp, [3], 1, 1, thr=0.0, dtype=dtype)
    assert lens[0, 0] == 2 and tokens[0, 0].tolist() == [1, 1, 0] and scores[0, 0] == -2.0 ** 40 - 1


def test_sim_edges():
    one = O.emissions(3, 1, 1, 6, "float32", blank_share=0.0)
    check_against_oracle(run_sim(one, [1], 4, 4), O.expected(one, [1], 4), 4, 1)                        # T = 1
    lp = O.emissions(5, 3, 12, 6, "float32")
    tokens, lens, scores = run_sim(lp, [0, 12, 5], 4, 2)                                                  # an empty example
    assert lens[0].tolist() == [0, -1] and scores[0].tolist() == [0.0, -np.inf] and not tokens[0].any()
    check_against_oracle((tokens, lens, scores), O.expected(lp, [0, 12, 5], 4), 2, 12)
    tokens, lens, scores = run_sim(lp, [12, 12, 12], 4, 4, thr=-1e9)                                      # every frame skipped
    assert lens.tolist() == [[0, -1, -1, -1]] * 3 and scores[:, 0].tolist() == [0.0] * 3 and not tokens.any()
    two = O.emissions(9, 1, 1, 2, "float32", blank_share=0.0)                                            # 2 live prefixes, nbest 4
    tokens, lens, scores = run_sim(two, [1], 4, 4, thr=0.0)
    assert sorted(lens[0].tolist()) == [-1, -1, 0, 1] and scores[0, 2:].tolist() == [-np.inf] * 2
    check_against_oracle((tokens, lens, scores), O.expected(two, [1], 4, 0, 0.0), 4, 1)
    lp = O.emissions(13, 2, 20, 7, "float32", blank=4)                                                   # a non-zero blank
    check_against_oracle(run_sim(lp, [20, 9], 5, 5, blank=4), O.expected(lp, [20, 9], 5, 4), 5, 20)


def test_sim_poisoned_padding_changes_nothing():
    lp, lengths, K, _ = case("general", torch.float32)
    bad = lp.copy()
    for b in range(3):
        bad[b, lengths[b]:] = (np.nan, np.inf, -np.inf)[b]
    assert not np.array_equal(bad, lp, equal_nan=True)
    for g, r in zip(run_sim(bad, lengths, K, K), run_sim(lp, lengths, K, K)):
        assert np.array_equal(g, r)


@pytest.mark.parametrize("ldtype", [torch.int32, torch.int64])
def test_sim_flagged_lengths_between_canaries(ldtype):
    lp, _, K, _ = case("general", torch.float32)
    T = lp.shape[1]
    tokens, lens, scores = run_sim(lp, [-1, T, T + 1], K, 3, ldtype=ldtype)
    for b in (0, 2):
        assert lens[b].tolist() == [-1] * 3 and np.isnan(scores[b]).all() and not tokens[b].any()
    check_against_oracle((tokens[1:2], lens[1:2], scores[1:2]), O.expected(lp[1:2], [T], K), 3, T)     # the neighbour is untouched


@pytest.mark.parametrize("dtype", DTYPES)
def test_sim_non_finite_log_probs_stay_in_bounds(dtype):
    """NaN / +inf / -inf inside live frames: the canaries of run_sim hold, lengths stay in [-1, T], tokens in [0, V)."""
    rng = np.random.default_rng(21)
    for thr in (O.THR, 0.0):
        lp = O.emissions(17, 3, 30, 9, "float32", blank_share=0.2)
        for b, v in enumerate((np.nan, np.inf, -np.inf)):
            lp[b][rng.random((30, 9)) < 0.15] = v
        lp[0, 3] = np.nan
        lp[1, 4] = -np.inf
        lp[2, :, 0] = -np.inf                                                                            # blank never possible
        tokens, lens, scores = run_sim(lp, [30, 30, 30], 6, 6, thr=thr, dtype=dtype)
        assert ((lens >= -1) & (lens <= 30)).all() and ((tokens >= 0) & (tokens < 9)).all()
        assert not np.isnan(scores).any()                                                                # a NaN score is never kept


# ---- the public surface --------------------------------------------------------------------------------------------------------

def test_signatures():
    sig = lambda f: str(inspect.signature(f))
    assert sig(ctc_beam_search) == ("(log_probs: 'Tensor', lengths: 'Optional[Tensor]' = None, beam_size: 'int' = 10, "
                                    "nbest: 'int' = 1, blank: 'int' = 0, blank_skip_threshold: 'float' = -0.05129329438755058)"
                                    " -> 'Tuple[Tensor, Tensor, Tensor]'")
    assert sig(CUCTCDecoder.__init__) == ("(self, vocab_list: 'List[str]', blank_id: 'int' = 0, beam_size: 'int' = 10, "
                                          "nbest: 'int' = 1, blank_skip_threshold: 'float' = -0.05129329438755058, "
                                          "cuda_stream: 'Optional[torch.cuda.Stream]' = None)")
    assert sig(CUCTCDecoder.__call__) == "(self, log_prob: 'Tensor', encoder_out_lens: 'Tensor') -> 'List[List[CUCTCHypothesis]]'"
    assert sig(cuda_ctc_decoder) == ("(tokens: 'Union[str, List[str]]', nbest: 'int' = 1, beam_size: 'int' = 10, "
                                     "blank_skip_threshold: 'float' = 0.95) -> 'CUCTCDecoder'")
    assert CUCTCHypothesis._fields == ("tokens", "words", "score")
    assert math.log(0.95) == -0.05129329438755058
    h = CUCTCHypothesis(tokens=[1], words=["a"], score=-1.0)
    assert h.tokens == [1] and h.words == ["a"] and h.score == -1.0


def test_checks_and_exception_types():
    x = torch.zeros(2, 5, 4)
    with pytest.raises(ValueError):
        ctc_beam_search(torch.zeros(5, 4))
    with pytest.raises(ValueError):
        ctc_beam_search(x, torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError):
        ctc_beam_search(torch.zeros(2, 5, 1))
    with pytest.raises(ValueError):
        ctc_beam_search(x.transpose(0, 1))
    with pytest.raises(TypeError):
        ctc_beam_search(x.to(torch.int32))
    with pytest.raises(TypeError):
        ctc_beam_search(x, torch.zeros(2))
    with pytest.raises(ValueError):
        ctc_beam_search(x, nbest=3, beam_size=2)
    with pytest.raises(ValueError):
        ctc_beam_search(x, beam_size=0)
    with pytest.raises(ValueError):
        ctc_beam_search(x, blank=4)
    with pytest.raises(NotImplementedError, match="beam_size <= 32"):
        ctc_beam_search(x, beam_size=33)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ctc_beam_search(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cuda_ctc_decoder(["-", "a", "b", "c"])(x, torch.tensor([5, 5], dtype=torch.int32))


def test_decoder_object_checks(tmp_path):
    with pytest.raises(ValueError):
        CUCTCDecoder(["-", "a"], blank_id=1)
    with pytest.raises(ValueError):
        CUCTCDecoder(["-", "a"], nbest=3, beam_size=2)
    with pytest.raises(NotImplementedError):
        CUCTCDecoder(["-", "a"], beam_size=33)
    with pytest.raises(ValueError):
        cuda_ctc_decoder(["-", "a"], blank_skip_threshold=0.0)
    with pytest.raises(ValueError):
        cuda_ctc_decoder(["-", "a"])(torch.zeros(1, 3, 5), torch.tensor([3]))
    path = tmp_path / "tokens.txt"
    path.write_text("<blk>\na\nb\n|\n", encoding="utf-8")
    d = cuda_ctc_decoder(str(path), nbest=2, beam_size=5, blank_skip_threshold=0.9)
    assert d.vocab_list == ["<blk>", "a", "b", "|"] and (d.nbest, d.beam_size, d.blank_id) == (2, 5, 0)
    assert d.blank_skip_threshold == math.log(0.9) and d.cuda_stream is None
    assert cuda_ctc_decoder(["-", "a"]).blank_skip_threshold == math.log(0.95)
