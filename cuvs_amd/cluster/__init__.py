"""Clustering (reference: python/cuvs/cuvs/cluster/)."""
from . import agglomerative, kmeans, spectral  # noqa: F401
