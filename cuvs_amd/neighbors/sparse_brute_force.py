"""Sparse brute-force kNN over CSR rows (reference: cuvs::neighbors::brute_force::{sparse_index, build, sparse_search_params,
search}, cpp/include/cuvs/neighbors/brute_force.hpp:594-700; C entry points: include/cuvs_amd/sparse.h).

The dataset and the queries are ``scipy.sparse`` matrices or ``(indptr, indices, data, shape)`` tuples of device tensors
(cuvs_amd.distance.sparse_pairwise_distance has the conversion rules)."""
import ctypes as C

import torch

from .._lib import check, lib, Tensor
from ..common import auto_sync_resources
from ..distance._sparse import as_csr, metric_id

DEFAULT_BATCH_SIZE = 2 << 14  # sparse_search_params


class _CIndex(C.Structure):
    _fields_ = [("addr", C.c_size_t)]


class Index:
    def __init__(self):
        self._p = C.POINTER(_CIndex)()
        check(lib().cuvsAmdSparseBruteForceIndexCreate(C.byref(self._p)))
        self.trained = False
        self.shape = (0, 0)
        self._keep = None  # the index is a non-owning view of the three arrays

    def __del__(self):
        try:
            if self._p:
                lib().cuvsAmdSparseBruteForceIndexDestroy(self._p)
        except Exception:
            pass

    def __repr__(self):
        return "Index(type=SparseBruteForce, shape=%s)" % (self.shape,)


@auto_sync_resources
def build(dataset, metric="euclidean", metric_arg=2.0, resources=None):
    ds = as_csr(dataset)
    idx = Index()
    check(lib().cuvsAmdSparseBruteForceBuild(resources.get_c_obj(), *ds.ptrs, C.c_int64(ds.shape[0]), C.c_int64(ds.shape[1]),
                                             C.c_int(metric_id(metric)), C.c_float(metric_arg), idx._p))
    idx._keep = ds
    idx.shape = ds.shape
    idx.trained = True
    return idx


@auto_sync_resources
def search(index, queries, k, batch_size_index=DEFAULT_BATCH_SIZE, batch_size_query=DEFAULT_BATCH_SIZE, neighbors=None,
           distances=None, neighbors_dtype=torch.int64, resources=None):
    """Returns (distances [m, k] float32, neighbors [m, k] int64 or int32): best first, ties to the smaller row id."""
    if not index.trained:
        raise ValueError("Index needs to be built before calling search.")
    q = as_csr(queries, index._keep.data.device)
    if q.shape[1] != index.shape[1]:
        raise ValueError("Inputs must have same number of columns. index=%s, queries=%s" % (index.shape[1], q.shape[1]))
    m = q.shape[0]
    if neighbors is None:
        neighbors = torch.empty((m, k), dtype=neighbors_dtype, device=q.data.device)
    if distances is None:
        distances = torch.empty((m, k), dtype=torch.float32, device=q.data.device)
    tn, td = Tensor(neighbors), Tensor(distances)
    check(lib().cuvsAmdSparseBruteForceSearch(resources.get_c_obj(), index._p, *q.ptrs, C.c_int64(m), C.c_int64(k),
                                              C.c_int64(batch_size_index), C.c_int64(batch_size_query), tn.ptr, td.ptr))
    return distances, neighbors
