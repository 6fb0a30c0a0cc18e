"""Clustering (reference: python/cuvs/cuvs/cluster/)."""
from . import agglomerative, kmeans  # noqa: F401
