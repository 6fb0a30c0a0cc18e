"""Sparse (CSR) pairwise distances (reference: cuvs::distance::pairwise_distance over CSR views,
cpp/include/cuvs/distance/distance.hpp:389-466; C entry points: include/cuvs_amd/sparse.h; contract: DESIGN.md 3.1x).

A sparse matrix is a ``scipy.sparse`` matrix (converted with tocsr / sum_duplicates / sort_indices, cast to int32 / fp32 and
copied to the device) or a tuple ``(indptr, indices, data, shape)`` of device tensors, which is handed to the library as it is."""
import ctypes as C

import torch

from .._lib import Tensor, check, lib
from ..common import auto_sync_resources

SPARSE_DISTANCES = ["sqeuclidean", "euclidean", "l2", "cosine", "l1", "cityblock", "l2_unexpanded", "l2_sqrt_unexpanded",
                    "inner_product", "chebyshev", "canberra", "lp", "minkowski", "correlation", "jaccard", "hellinger",
                    "jensenshannon", "hamming", "kl_divergence", "russellrao", "dice"]


def metric_id(metric):
    from . import DISTANCE_TYPES

    if isinstance(metric, str):
        if metric not in SPARSE_DISTANCES:
            raise ValueError("metric %s is not supported for sparse inputs" % metric)
        return DISTANCE_TYPES[metric]
    return int(metric)


class DeviceCsr:
    """indptr int32 [rows + 1], indices int32 [nnz], data fp32 [nnz] on the device, and the shape"""

    def __init__(self, indptr, indices, data, shape):
        self.indptr, self.indices, self.data = indptr, indices, data
        self.shape = (int(shape[0]), int(shape[1]))
        self.tensors = (Tensor(indptr), Tensor(indices), Tensor(data))

    @property
    def ptrs(self):
        return tuple(t.ptr for t in self.tensors)


def as_csr(X, device=None):
    if isinstance(X, DeviceCsr):
        return X
    if isinstance(X, (tuple, list)):
        indptr, indices, data, shape = X
        return DeviceCsr(indptr, indices, data, shape)
    if hasattr(X, "tocsr"):
        import numpy as np

        device = device if device is not None else torch.device("cuda")
        m = X.tocsr().copy()
        m.sum_duplicates()
        m.sort_indices()
        if m.nnz >= 2 ** 31:
            raise ValueError("nnz must be below 2^31")
        return DeviceCsr(torch.from_numpy(m.indptr.astype(np.int32)).to(device), torch.from_numpy(m.indices.astype(np.int32)).to(device),
                         torch.from_numpy(m.data.astype(np.float32)).to(device), m.shape)
    raise TypeError("a sparse matrix is a scipy.sparse matrix or a tuple (indptr, indices, data, shape) of device tensors")


@auto_sync_resources
def validate_csr(X, resources=None):
    """Raises CuvsError unless X is a canonical CSR matrix (cuvsAmdSparseCsrValidate)."""
    x = as_csr(X)
    check(lib().cuvsAmdSparseCsrValidate(resources.get_c_obj(), *x.ptrs, C.c_int64(x.shape[0]), C.c_int64(x.shape[1])))


@auto_sync_resources
def sparse_pairwise_distance(X, Y=None, out=None, metric="euclidean", metric_arg=2.0, resources=None):
    """Distances between the rows of the sparse matrices X (m, k) and Y (n, k) -> (m, n) float32 on the device. Y=None: X
    against itself."""
    x = as_csr(X)
    y = x if Y is None else as_csr(Y, x.data.device)
    if x.shape[1] != y.shape[1]:
        raise ValueError("Inputs must have same number of columns. a=%s, b=%s" % (x.shape[1], y.shape[1]))
    m, n = x.shape[0], y.shape[0]
    if out is None:
        out = torch.empty((m, n), dtype=torch.float32, device=x.data.device)
    to = Tensor(out)
    check(lib().cuvsAmdSparsePairwiseDistance(resources.get_c_obj(), *x.ptrs, C.c_int64(m), *y.ptrs, C.c_int64(n), C.c_int64(x.shape[1]),
                                              to.ptr, C.c_int(metric_id(metric)), C.c_float(metric_arg)))
    return out


def sparse_last_stats():
    """Counters of the calling thread's last sparse pairwise / search call."""
    out = (C.c_uint64 * 4)()
    check(lib().cuvsAmdSparseLastStats(out))
    return dict(ranges_visited=out[0], ranges_skipped=out[1], long_row_pieces=out[2], tiles=out[3])


def set_sparse_walk_form(intersection=0, union=0):
    """Comparator hook of the timing and of the tests: the form of the walk over the rows of Y in the intersection and the union
    kernel (1: one entry per load, 8 / 4 rows per thread; 2 - 4: through the wave's LDS stage, 8 entries x 1 row, 16 x 1,
    8 x 2); 0 chooses by shape. Process-wide; results never depend on it."""
    check(lib().cuvsAmdSparseSetForm(C.c_int(intersection), C.c_int(union)))
