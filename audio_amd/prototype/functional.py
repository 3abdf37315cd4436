"""``torchaudio.prototype.functional``: the room simulation and the synthesis entry points and the Bark and chroma filterbank
builders, defined in ``audio_amd.functional``."""
from ..functional import (adsr_envelope, barkscale_fbanks, chroma_filterbank, extend_pitch, filter_waveform,  # noqa: F401
                          frequency_impulse_response, oscillator_bank, ray_tracing, ray_tracing_batch, simulate_rir_ism,
                          simulate_rir_ism_batch, sinc_impulse_response)

__all__ = ["simulate_rir_ism", "simulate_rir_ism_batch", "ray_tracing", "ray_tracing_batch", "oscillator_bank", "adsr_envelope",
           "extend_pitch", "sinc_impulse_response", "frequency_impulse_response", "filter_waveform", "barkscale_fbanks",
           "chroma_filterbank"]
