"""Preprocessing (reference: python/cuvs/cuvs/preprocessing)."""
from . import quantize  # noqa: F401
