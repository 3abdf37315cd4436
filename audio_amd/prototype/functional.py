"""``torchaudio.prototype.functional``: the room simulation entry points, defined in ``audio_amd.functional``."""
from ..functional import simulate_rir_ism, simulate_rir_ism_batch  # noqa: F401

__all__ = ["simulate_rir_ism", "simulate_rir_ism_batch"]
