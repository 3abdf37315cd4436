"""Model-side components that run on the device (reference: torchaudio.models): the CTC beam search decoder."""
from . import decoder
from .decoder import CUCTCDecoder, CUCTCHypothesis, ctc_beam_search, cuda_ctc_decoder

__all__ = ["decoder", "CUCTCDecoder", "CUCTCHypothesis", "ctc_beam_search", "cuda_ctc_decoder"]
