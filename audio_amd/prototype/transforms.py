"""``torchaudio.prototype.transforms``: the Bark and chroma modules, defined in ``audio_amd.transforms``."""
from ..transforms import BarkScale, BarkSpectrogram, ChromaScale, ChromaSpectrogram, InverseBarkScale  # noqa: F401

__all__ = ["BarkScale", "InverseBarkScale", "BarkSpectrogram", "ChromaScale", "ChromaSpectrogram"]
