"""The reference's ``torchaudio.prototype`` import path for what this package serves of it."""
from . import functional  # noqa: F401
from . import transforms  # noqa: F401

__all__ = ["functional", "transforms"]
