"""Quantizers (reference: python/cuvs/cuvs/preprocessing/quantize)."""
from . import binary  # noqa: F401
