"""Spectral embedding (reference: cpp/include/cuvs/preprocessing/spectral_embedding.hpp - transform,
helpers::create_connectivity_graph; C entry points: include/cuvs_amd/spectral.h).

X is a torch tensor on the device, fp32, row-major and contiguous; graphs are COO triples (rows int32, cols int32, vals fp32)
on the device and are assumed symmetric. The Laplacian follows scipy.sparse.csgraph.laplacian, the eigenvectors come from a
thick-restart Lanczos iteration in fp32, and every column of the embedding has its entry of largest magnitude positive."""
import ctypes as C
import warnings

import numpy as np
import torch

from .._lib import Tensor, check, lib
from ..common import auto_sync_resources
from ..neighbors._util import optional_tensor as _t


class _CParams(C.Structure):
    _fields_ = [
        ("n_components", C.c_int),
        ("n_neighbors", C.c_int),
        ("norm_laplacian", C.c_bool),
        ("drop_first", C.c_bool),
        ("tolerance", C.c_float),
        ("seed", C.c_uint64),
    ]


class Params:
    """n_components counts the eigenpairs computed, i.e. the columns before drop_first takes the first away."""

    def __init__(self, n_components=2, n_neighbors=15, norm_laplacian=True, drop_first=True, tolerance=1e-5, seed=0):
        self.n_components = n_components
        self.n_neighbors = n_neighbors
        self.norm_laplacian = norm_laplacian
        self.drop_first = drop_first
        self.tolerance = tolerance
        self.seed = seed

    @property
    def n_columns(self):
        return self.n_components - (1 if self.drop_first else 0)

    def _c(self):
        return _CParams(self.n_components, self.n_neighbors, self.norm_laplacian, self.drop_first, self.tolerance, self.seed)


def last_stats():
    """Counters of the calling thread's last solve: matrix-vector products, restarts, ncv and converged (0 or 1)."""
    out = (C.c_uint64 * 4)()
    check(lib().cuvsAmdSpectralLastStats(out))
    return dict(matvecs=out[0], restarts=out[1], ncv=out[2], converged=out[3])


def _warn_unless_converged(what):
    stats = last_stats()
    if not stats["converged"]:
        warnings.warn(f"{what}: the eigen-solver stopped at its cap of {stats['matvecs']} matrix-vector products before reaching "
                      "the tolerance; the last Ritz pairs are returned", RuntimeWarning, stacklevel=3)


def _outputs(params, n, device, embedding, eigenvalues, order):
    if embedding is None:
        if order == "F":
            embedding = torch.empty((params.n_columns, n), dtype=torch.float32, device=device).t()
        else:
            embedding = torch.empty((n, params.n_columns), dtype=torch.float32, device=device)
    if eigenvalues is True:
        eigenvalues = torch.empty(params.n_components, dtype=torch.float32, device=device)
    return embedding, (None if eigenvalues is False else eigenvalues)


@auto_sync_resources
def create_connectivity_graph(params, X, resources=None):
    """The symmetrised kNN connectivity graph of X: (rows int32, cols int32, vals fp32), sorted by (row, col), values 0.5 or 1."""
    n, cap = X.shape[0], 2 * X.shape[0] * max(int(params.n_neighbors), 0)
    rows = torch.empty(cap, dtype=torch.int32, device=X.device)
    cols = torch.empty(cap, dtype=torch.int32, device=X.device)
    vals = torch.empty(cap, dtype=torch.float32, device=X.device)
    nnz = C.c_int64(0)
    p = params._c()
    ts = [Tensor(t) for t in (X, rows, cols, vals)]
    check(lib().cuvsAmdSpectralConnectivityGraph(resources.get_c_obj(), C.byref(p), *[t.ptr for t in ts], C.byref(nnz)))
    return rows[:nnz.value], cols[:nnz.value], vals[:nnz.value]


@auto_sync_resources
def transform(params, X, embedding=None, eigenvalues=False, order="C", resources=None):
    """The embedding [n, n_columns] of X. `eigenvalues=True` (or a buffer, host numpy or device torch) also returns the
    n_components eigenvalues; `order="F"` makes the embedding column-major, as the reference's is."""
    embedding, eigenvalues = _outputs(params, X.shape[0], X.device, embedding, eigenvalues, order)
    p = params._c()
    tx, te = Tensor(X), Tensor(embedding)
    tv, pv = _t(eigenvalues)
    check(lib().cuvsAmdSpectralEmbeddingTransform(resources.get_c_obj(), C.byref(p), tx.ptr, te.ptr, pv))
    _warn_unless_converged("spectral_embedding.transform")
    return embedding if eigenvalues is None else (embedding, eigenvalues)


@auto_sync_resources
def transform_graph(params, rows, cols, vals, n, embedding=None, eigenvalues=False, order="C", resources=None):
    """The same from a symmetric COO graph on the device; params.n_neighbors is ignored."""
    embedding, eigenvalues = _outputs(params, n, rows.device, embedding, eigenvalues, order)
    p = params._c()
    ts = [Tensor(t) for t in (rows, cols, vals)]
    te = Tensor(embedding)
    tv, pv = _t(eigenvalues)
    check(lib().cuvsAmdSpectralEmbeddingTransformGraph(resources.get_c_obj(), C.byref(p), *[t.ptr for t in ts], C.c_int64(n), te.ptr, pv))
    _warn_unless_converged("spectral_embedding.transform_graph")
    return embedding if eigenvalues is None else (embedding, eigenvalues)


@auto_sync_resources
def eigsh(rows, cols, vals, n, k, norm_laplacian=True, ncv=0, tolerance=1e-5, seed=0, resources=None):
    """The solver on its own: (eigenvalues fp32 [k] ascending, eigenvectors fp32 [k, n] of unit norm) of the graph's Laplacian."""
    values = torch.empty(max(k, 0), dtype=torch.float32, device=rows.device)
    vectors = torch.empty((max(k, 0), n), dtype=torch.float32, device=rows.device)
    ts = [Tensor(t) for t in (rows, cols, vals)]
    tv, tx = Tensor(values), Tensor(vectors)
    check(lib().cuvsAmdSpectralEigsh(resources.get_c_obj(), *[t.ptr for t in ts], C.c_int64(n), C.c_bool(norm_laplacian), C.c_int(k),
                                     C.c_int(ncv), C.c_float(tolerance), C.c_uint64(seed), tv.ptr, tx.ptr))
    _warn_unless_converged("spectral_embedding.eigsh")
    return values, vectors


@auto_sync_resources
def laplacian_matvec(rows, cols, vals, n, x, norm_laplacian=True, resources=None):
    """Test hook: (y = L x by the solver's own operator, the degree scaling)."""
    y = torch.empty(n, dtype=torch.float32, device=x.device)
    diag = torch.empty(n, dtype=torch.float32, device=x.device)
    ts = [Tensor(t) for t in (rows, cols, vals)]
    tx, ty, td = Tensor(x), Tensor(y), Tensor(diag)
    check(lib().cuvsAmdSpectralLaplacianMatvec(resources.get_c_obj(), *[t.ptr for t in ts], C.c_int64(n), C.c_bool(norm_laplacian), tx.ptr,
                                               ty.ptr, td.ptr))
    return y, diag


@auto_sync_resources
def orthogonalize(V, u, resources=None):
    """Test hook: u (in place) after the solver's two Gram-Schmidt passes against the rows of V and the normalisation; returns
    (u, the norm before the division)."""
    norm = C.c_float(0)
    tv, tu = Tensor(V), Tensor(u)
    check(lib().cuvsAmdSpectralOrthogonalize(resources.get_c_obj(), tv.ptr, tu.ptr, C.byref(norm)))
    return u, float(np.float32(norm.value))
