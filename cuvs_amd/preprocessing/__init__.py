"""Preprocessing (reference: python/cuvs/cuvs/preprocessing)."""
from . import pca  # noqa: F401
from . import quantize  # noqa: F401
from . import spectral_embedding  # noqa: F401
