"""``torchaudio.prototype.functional``: the room simulation and the synthesis entry points, defined in
``audio_amd.functional``."""
from ..functional import (adsr_envelope, extend_pitch, filter_waveform, frequency_impulse_response,  # noqa: F401
                          oscillator_bank, ray_tracing, ray_tracing_batch, simulate_rir_ism, simulate_rir_ism_batch,
                          sinc_impulse_response)

__all__ = ["simulate_rir_ism", "simulate_rir_ism_batch", "ray_tracing", "ray_tracing_batch", "oscillator_bank", "adsr_envelope",
           "extend_pitch", "sinc_impulse_response", "frequency_impulse_response", "filter_waveform"]
