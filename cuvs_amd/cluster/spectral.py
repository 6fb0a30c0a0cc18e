"""Spectral clustering (reference: cpp/include/cuvs/cluster/spectral.hpp - fit_predict; C entry points:
include/cuvs_amd/spectral.h): the spectral embedding of the normalised Laplacian with nothing dropped,
then the non-hierarchical Lloyd k-means fit (k-means++ seeding, n_init trials) and its prediction.

X is a torch tensor on the device, fp32, row-major and contiguous; a graph is a COO triple (rows int32, cols int32, vals
fp32) on the device and is assumed symmetric."""
import ctypes as C

import torch

from .._lib import Tensor, check, lib
from ..common import auto_sync_resources
from ..preprocessing.spectral_embedding import _warn_unless_converged


class _CParams(C.Structure):
    _fields_ = [
        ("n_clusters", C.c_int),
        ("n_components", C.c_int),
        ("n_init", C.c_int),
        ("n_neighbors", C.c_int),
        ("tolerance", C.c_float),
        ("seed", C.c_uint64),
    ]


class Params:
    def __init__(self, n_clusters=8, n_components=8, n_init=10, n_neighbors=15, tolerance=1e-5, seed=0):
        self.n_clusters = n_clusters
        self.n_components = n_components
        self.n_init = n_init
        self.n_neighbors = n_neighbors
        self.tolerance = tolerance
        self.seed = seed

    def _c(self):
        return _CParams(self.n_clusters, self.n_components, self.n_init, self.n_neighbors, self.tolerance, self.seed)


@auto_sync_resources
def fit_predict(params, X=None, graph=None, labels=None, resources=None):
    """Labels int32 [n] in [0, n_clusters) of the rows of X, or of the vertices of `graph` = (rows, cols, vals, n)."""
    if (X is None) == (graph is None):
        raise ValueError("pass either X or graph")
    p = params._c()
    if graph is None:
        if labels is None:
            labels = torch.empty(X.shape[0], dtype=torch.int32, device=X.device)
        tx, tl = Tensor(X), Tensor(labels)
        check(lib().cuvsAmdSpectralClusteringFitPredict(resources.get_c_obj(), C.byref(p), tx.ptr, tl.ptr))
    else:
        rows, cols, vals, n = graph
        if labels is None:
            labels = torch.empty(n, dtype=torch.int32, device=rows.device)
        ts = [Tensor(t) for t in (rows, cols, vals)]
        tl = Tensor(labels)
        check(lib().cuvsAmdSpectralClusteringFitPredictGraph(resources.get_c_obj(), C.byref(p), *[t.ptr for t in ts], C.c_int64(n), tl.ptr))
    _warn_unless_converged("spectral.fit_predict")
    return labels
