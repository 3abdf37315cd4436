"""CTC prefix beam search on the device (csrc/ctc_decoder.h): ``ctc_beam_search`` and the reference's ``cuda_ctc_decoder``
surface (``torchaudio.models.decoder``: ``CUCTCHypothesis``, ``CUCTCDecoder``, ``cuda_ctc_decoder``).

The contract is the definition in ``ctc_beam_search``'s docstring, restated in float64 by ``tests/ctc_decoder_oracle.py``.
The names, parameters and defaults of the three reference objects are written from memory of the reference, whose decoder
is a CUDA-only extension that is not available to compare against; no equality with the reference's results is claimed.
"""
from __future__ import annotations

import math
import os
from typing import List, NamedTuple, Optional, Tuple, Union

import torch
from torch import Tensor

from .. import _lib

__all__ = ["CUCTCHypothesis", "CUCTCDecoder", "cuda_ctc_decoder", "ctc_beam_search", "ctc_decoder_tiles", "CTC_DECODER_MAX_BEAM"]

CTC_DECODER_MAX_BEAM = 32            # AAMD_CTC_DECODER_MAX_BEAM: the widest beam the beam kernel serves
_DTYPES = {torch.float32: 0, torch.float64: 1, torch.float16: 2, torch.bfloat16: 3}      # AAMD_SA_*
_INTS = (torch.int32, torch.int64)


def ctc_decoder_tiles(beam_size: int = 10) -> Tuple[int, int, int, int, int]:
    """(widest beam, threads of a row-pass workgroup, threads of a beam-pass workgroup, (value, token) slots of a frame's
    record, candidates of a frame: per entry the stay, one extension per record slot and the extension by its own last token) of
    csrc/ctc_decoder.h for a beam of ``beam_size``."""
    lib = _lib.lib()
    return (int(lib.aamd_ctc_decoder_max_beam()), int(lib.aamd_ctc_decoder_row_threads()), int(lib.aamd_ctc_decoder_beam_threads()),
            int(lib.aamd_ctc_decoder_record_slots(beam_size)), int(lib.aamd_ctc_decoder_candidates(beam_size)))


def _check(log_probs: Tensor, lengths: Optional[Tensor], beam_size: int, nbest: int, blank: int) -> None:
    """The host-side checks of ctc_beam_search.  Nothing is read from the device."""
    if not isinstance(log_probs, Tensor) or log_probs.dim() != 3:
        raise ValueError(f"log_probs must be 3-D (batch, frame, vocab), got {tuple(getattr(log_probs, 'shape', ()))}")
    B, T, V = log_probs.shape
    if lengths is not None and (lengths.dim() != 1 or lengths.shape[0] != B):
        raise ValueError(f"lengths must be 1-D of the batch size {B}, got {tuple(lengths.shape)}")
    if T < 1 or V < 2:
        raise ValueError(f"log_probs needs at least one frame and two vocabulary entries, got {tuple(log_probs.shape)}")
    if log_probs.dtype not in _DTYPES:
        raise TypeError(f"log_probs must be float32, float64, float16 or bfloat16 (got {log_probs.dtype})")
    if lengths is not None and lengths.dtype not in _INTS:
        raise TypeError(f"lengths must be int32 or int64 (got {lengths.dtype})")
    tensors = [(log_probs, "log_probs")] + ([(lengths, "lengths")] if lengths is not None else [])
    for t, what in tensors:
        if not t.is_contiguous():
            raise ValueError(f"{what} must be contiguous")
    if beam_size < 1 or nbest < 1:
        raise ValueError(f"beam_size and nbest must be at least 1 (got {beam_size} and {nbest})")
    if nbest > beam_size:
        raise ValueError(f"nbest must not exceed beam_size (got {nbest} > {beam_size})")
    if blank < 0 or blank >= V:
        raise ValueError("blank must be within [0, log_probs.shape[-1])")
    if beam_size > CTC_DECODER_MAX_BEAM:
        raise NotImplementedError(f"audio_amd: ctc_beam_search serves beam_size <= {CTC_DECODER_MAX_BEAM} (got {beam_size}): the "
                                  "beam of one example belongs to one workgroup")
    lib = _lib.lib()
    max_frames, max_nodes = int(lib.aamd_ctc_decoder_max_frames()), int(lib.aamd_ctc_decoder_max_nodes())
    if B * T > max_frames or 1 + beam_size * T > max_nodes:
        raise NotImplementedError(f"audio_amd: ctc_beam_search serves batch * frames <= {max_frames} and 1 + beam_size * frames <= "
                                  f"{max_nodes} (got batch {B}, frames {T}, beam_size {beam_size}): node ids of the prefix trie "
                                  "are 32-bit")
    for t, what in tensors:
        if not t.is_cuda:
            raise RuntimeError(f"audio_amd: {what} must be on an MI355X (ROCm) device, got {t.device}. "
                               "The HIP kernels have no CPU fallback.")
        if t.device != log_probs.device:
            raise RuntimeError(f"audio_amd: {what} must be on the log_probs' device")


def ctc_beam_search(log_probs: Tensor, lengths: Optional[Tensor] = None, beam_size: int = 10, nbest: int = 1, blank: int = 0,
                    blank_skip_threshold: float = math.log(0.95)) -> Tuple[Tensor, Tensor, Tensor]:
    r"""CTC prefix beam search without a language model, on the device: ``(tokens, token_lengths, scores)`` of the ``nbest``
    best prefixes of every example of ``log_probs`` ``(B, T, V)`` (float32 / float64 / float16 / bfloat16, dense) with
    ``lengths`` ``(B,)`` (int32 / int64; ``None``: ``T``).

    Example ``b`` keeps a beam of at most ``beam_size`` distinct prefixes, each with ``(pb, pnb)``, the log mass of its
    alignments that end in blank / not in blank; the beam starts as ``{(): (0, -inf)}``.  A frame with
    ``log_probs[b, t, blank] > blank_skip_threshold`` (a log-probability) is skipped entirely.  For every other frame each
    prefix ``l`` with last token ``e`` and ``tot = logaddexp(pb, pnb)`` contributes ``tot + lp[blank]`` to ``pb'`` of ``l``,
    ``pnb + lp[e]`` to ``pnb'`` of ``l`` (if ``l`` is not empty) and ``(pb if c == e else tot) + lp[c]`` to ``pnb'`` of
    ``l + c`` for every ``c != blank``; contributions to one prefix merge with ``logaddexp``, and the new beam is the
    ``beam_size`` prefixes with the largest ``logaddexp(pb', pnb')`` that is neither ``-inf`` nor NaN.  Of two extensions of
    one prefix with bit-equal scores the smaller token ranks first; any other exact tie resolves in a fixed way (two calls
    give the same bits).  All sums are float64 for every input dtype.

    ``tokens`` is ``(B, nbest, T)`` int32, zero beyond each length; ``token_lengths`` ``(B, nbest)`` int32, ``-1`` where the
    beam held fewer hypotheses; ``scores`` ``(B, nbest)`` float64 in descending order, ``-inf`` for a missing hypothesis.  An
    example with a length outside ``[0, T]`` gets lengths ``-1`` and scores NaN.  Two launches (a row pass over
    ``log_probs``, a beam pass per example); the lengths are read on the device, nothing is synchronised, so the call can be
    captured in a graph.  No gradient: the results are detached.  Not registered as a dispatcher op."""
    beam_size, nbest, blank = int(beam_size), int(nbest), int(blank)
    _check(log_probs, lengths, beam_size, nbest, blank)
    B, T, V = log_probs.shape
    dev = log_probs.device
    log_probs = log_probs.detach()
    if lengths is None:
        lengths = torch.full((B,), T, dtype=torch.int32, device=dev)
    tokens = torch.empty((B, nbest, T), dtype=torch.int32, device=dev)
    token_lengths = torch.empty((B, nbest), dtype=torch.int32, device=dev)
    scores = torch.empty((B, nbest), dtype=torch.float64, device=dev)
    if B:
        lib = _lib.lib()
        ws = torch.empty((max(int(lib.aamd_ctc_decoder_workspace(B, T, V, beam_size)), 16),), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.aamd_ctc_beam_search(_DTYPES[log_probs.dtype], _lib.ptr(log_probs), _lib.ptr(lengths),
                                                int(lengths.dtype == torch.int64), B, T, V, blank, beam_size, nbest,
                                                float(blank_skip_threshold), ws.data_ptr(), tokens.data_ptr(),
                                                token_lengths.data_ptr(), scores.data_ptr(), _lib.current_stream(dev)))
    return tokens, token_lengths, scores


class CUCTCHypothesis(NamedTuple):
    r"""One hypothesis of :class:`CUCTCDecoder` (reference: ``torchaudio.models.decoder.CUCTCHypothesis``): the token ids, the
    vocabulary entries they name, and the score (log mass of the prefix, a float64 accumulation)."""
    tokens: List[int]
    words: List[str]
    score: float


class CUCTCDecoder:
    r"""CTC prefix beam search decoder on the device (reference: ``torchaudio.models.decoder.CUCTCDecoder``; its names,
    parameters and defaults are written from memory of the reference).  Differences: the reference's ``AssertionError``\ s are
    ``ValueError`` / ``TypeError`` / ``RuntimeError`` here; int64 lengths and float16 / bfloat16 / float64 emissions are
    accepted; scores are float64 sums.  ``blank_id`` other than 0 raises ``ValueError`` as the reference refuses it
    (``ctc_beam_search`` takes any blank)."""

    def __init__(self, vocab_list: List[str], blank_id: int = 0, beam_size: int = 10, nbest: int = 1,
                 blank_skip_threshold: float = math.log(0.95), cuda_stream: Optional[torch.cuda.Stream] = None):
        if blank_id != 0:
            raise ValueError(f"blank_id must be 0 (got {blank_id})")
        if beam_size < 1 or nbest < 1 or nbest > beam_size:
            raise ValueError(f"1 <= nbest <= beam_size is required (got nbest {nbest}, beam_size {beam_size})")
        if beam_size > CTC_DECODER_MAX_BEAM:
            raise NotImplementedError(f"audio_amd: CUCTCDecoder serves beam_size <= {CTC_DECODER_MAX_BEAM} (got {beam_size})")
        self.vocab_list = list(vocab_list)
        self.blank_id = blank_id
        self.beam_size = int(beam_size)
        self.nbest = int(nbest)
        self.blank_skip_threshold = float(blank_skip_threshold)
        self.cuda_stream = cuda_stream

    def __call__(self, log_prob: Tensor, encoder_out_lens: Tensor) -> List[List[CUCTCHypothesis]]:
        """``log_prob`` ``(B, T, V)`` and ``encoder_out_lens`` ``(B,)`` on the device -> for every example its hypotheses,
        best first; hypotheses the beam did not hold are left out.  The launches go to ``cuda_stream`` or the current stream;
        then the three result tensors are copied to the host once (bookkeeping of a result that is a Python list)."""
        if isinstance(log_prob, Tensor) and log_prob.dim() == 3 and log_prob.shape[2] != len(self.vocab_list):
            raise ValueError(f"log_prob has {log_prob.shape[2]} vocabulary entries, vocab_list {len(self.vocab_list)}")
        if self.cuda_stream is not None:
            with torch.cuda.stream(self.cuda_stream):
                tokens, lens, scores = ctc_beam_search(log_prob, encoder_out_lens, self.beam_size, self.nbest, self.blank_id,
                                                       self.blank_skip_threshold)
                packed = self._pack(tokens, lens, scores).cpu()
        else:
            tokens, lens, scores = ctc_beam_search(log_prob, encoder_out_lens, self.beam_size, self.nbest, self.blank_id,
                                                   self.blank_skip_threshold)
            packed = self._pack(tokens, lens, scores).cpu()
        B, N, T = tokens.shape
        packed = packed.reshape(B, N, T + 2)
        out: List[List[CUCTCHypothesis]] = []
        for b in range(B):
            if bool(torch.isnan(packed[b, :, 1]).any()):
                raise ValueError(f"example {b}: encoder_out_lens[{b}] lies outside [0, {T}]")
            hyps = []
            for h in range(N):
                n = int(packed[b, h, 0])
                if n < 0:
                    continue
                toks = [int(v) for v in packed[b, h, 2:2 + n].tolist()]
                hyps.append(CUCTCHypothesis(tokens=toks, words=[self.vocab_list[t] for t in toks], score=float(packed[b, h, 1])))
            out.append(hyps)
        return out

    @staticmethod
    def _pack(tokens: Tensor, lens: Tensor, scores: Tensor) -> Tensor:
        """(B, N, 2 + T) float64: length, score, tokens (int32 is exact in float64) -- one tensor, one copy."""
        return torch.cat((lens.to(torch.float64).unsqueeze(-1), scores.unsqueeze(-1), tokens.to(torch.float64)), dim=-1)


def cuda_ctc_decoder(tokens: Union[str, List[str]], nbest: int = 1, beam_size: int = 10,
                     blank_skip_threshold: float = 0.95) -> CUCTCDecoder:
    r"""Builds a :class:`CUCTCDecoder` (reference: ``torchaudio.models.decoder.cuda_ctc_decoder``).  ``tokens`` is the
    vocabulary as a list, or the path of a file with one token per line; ``blank_skip_threshold`` is a probability here and is
    passed on as its logarithm."""
    if isinstance(tokens, (str, os.PathLike)):
        with open(tokens, "r", encoding="utf-8") as f:
            vocab = [line.rstrip("\r\n") for line in f]
    else:
        vocab = list(tokens)
    if not 0.0 < blank_skip_threshold <= 1.0:
        raise ValueError(f"blank_skip_threshold must be a probability in (0, 1] (got {blank_skip_threshold})")
    return CUCTCDecoder(vocab_list=vocab, beam_size=beam_size, nbest=nbest, blank_skip_threshold=math.log(blank_skip_threshold))
