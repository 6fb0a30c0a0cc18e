"""Quantizers (reference: python/cuvs/cuvs/preprocessing/quantize)."""
from . import binary  # noqa: F401
from . import pq  # noqa: F401
from . import scalar  # noqa: F401
