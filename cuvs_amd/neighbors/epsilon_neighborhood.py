"""Epsilon neighbourhood: everything within a radius of each row of x, by brute force (reference:
cpp/include/cuvs/neighbors/epsilon_neighborhood.hpp and the CSR forms of ball_cover::eps_nn; C entry points:
include/cuvs_amd/eps_neighbors.h). `eps` is the squared radius; pair (i, j) is inside when the fp32 chain
acc = fmaf(x[i][t] - y[j][t], x[i][t] - y[j][t], acc), t ascending, ends at acc <= eps.

x and y are torch tensors on the device, fp32 or fp16 (the same type), row-major and contiguous; they are handed to the library
as they are, which refuses anything else."""
import ctypes as C

import torch

from .._lib import Tensor, check, lib
from ..common import auto_sync_resources
from ..distance import DISTANCE_TYPES
from ._util import optional_tensor as _t


def _metric(metric):
    return DISTANCE_TYPES[metric] if isinstance(metric, str) else int(metric)


@auto_sync_resources
def compute(x, y, eps, adj=None, vd=None, vd_dtype=torch.int64, metric="l2_unexpanded", resources=None):
    """Dense form: adj bool [m, n] and vd [m + 1] (vd[i] the degree of row i, vd[m] the number of edges). Buffers that are
    passed are filled and returned; `adj=False` / `vd=False` leave that output out (None is returned in its place)."""
    m, n = x.shape[0], y.shape[0]
    if adj is None:
        adj = torch.empty((m, n), dtype=torch.bool, device=x.device)
    elif adj is False:
        adj = None
    if vd is None:
        vd = torch.empty(m + 1, dtype=vd_dtype, device=x.device)
    elif vd is False:
        vd = None
    tx, ty = Tensor(x), Tensor(y)
    ta, pa = _t(adj)
    tv, pv = _t(vd)
    check(lib().cuvsAmdEpsNeighbors(resources.get_c_obj(), tx.ptr, ty.ptr, pa, pv, C.c_float(eps), C.c_int(_metric(metric))))
    return adj, vd


@auto_sync_resources
def csr_count(x, y, eps, indptr=None, vd=None, metric="l2_unexpanded", resources=None):
    """First call of the two-call protocol: indptr int64 [m + 1] (indptr[m] the number of edges); vd, when given, gets the
    degrees."""
    if indptr is None:
        indptr = torch.empty(x.shape[0] + 1, dtype=torch.int64, device=x.device)
    tx, ty, ti = Tensor(x), Tensor(y), Tensor(indptr)
    tv, pv = _t(vd)
    check(lib().cuvsAmdEpsNeighborsCsr(resources.get_c_obj(), tx.ptr, ty.ptr, ti.ptr, None, None, pv, C.c_float(eps),
                                       C.c_int(_metric(metric)), None))
    return indptr


@auto_sync_resources
def csr_fill(x, y, eps, indptr, indices, distances=None, vd=None, max_k=None, metric="l2_unexpanded", resources=None):
    """Second call of the two-call protocol (indptr is read; row i's ids go to indices[indptr[i]:indptr[i + 1]] in
    ascending order), or, with max_k, the one-call form (indptr is written, indices holds m * max_k; returns the largest
    degree found)."""
    tx, ty, ti, tn = Tensor(x), Tensor(y), Tensor(indptr), Tensor(indices)
    td, pd = _t(distances)
    tv, pv = _t(vd)
    mk = C.c_int64(max_k) if max_k is not None else None
    check(lib().cuvsAmdEpsNeighborsCsr(resources.get_c_obj(), tx.ptr, ty.ptr, ti.ptr, tn.ptr, pd, pv, C.c_float(eps),
                                       C.c_int(_metric(metric)), C.byref(mk) if mk is not None else None))
    return mk.value if mk is not None else None


def csr(x, y, eps, max_k=None, return_distances=False, resources=None):
    """CSR form: (indptr, indices[, distances][, max_k_found]). Without max_k both calls of the count / fill protocol are
    made here; with max_k one call keeps the first max_k ids of every row and also returns the largest degree found."""
    m = x.shape[0]
    if max_k is None:
        indptr = csr_count(x, y, eps, resources=resources)
        if resources is not None:
            resources.sync()
        nnz = int(indptr[m].item())
        indices = torch.empty(nnz, dtype=torch.int64, device=x.device)
        distances = torch.empty(nnz, dtype=torch.float32, device=x.device) if return_distances else None
        csr_fill(x, y, eps, indptr, indices, distances, resources=resources)
        return (indptr, indices, distances) if return_distances else (indptr, indices)
    indptr = torch.empty(m + 1, dtype=torch.int64, device=x.device)
    indices = torch.empty(m * max_k, dtype=torch.int64, device=x.device)
    distances = torch.empty(m * max_k, dtype=torch.float32, device=x.device) if return_distances else None
    found = csr_fill(x, y, eps, indptr, indices, distances, max_k=max_k, resources=resources)
    if resources is not None:
        resources.sync()
    nnz = int(indptr[m].item())
    out = (indptr, indices[:nnz]) + ((distances[:nnz],) if return_distances else ())
    return out + (found,)


def last_stats():
    """Counters of the calling thread's last call: pair tiles, row slabs, edges, pairs the matrix-core screen handed to the
    exact chain (0: there is no screen)."""
    out = (C.c_uint64 * 4)()
    check(lib().cuvsAmdEpsNeighborsLastStats(out))
    return dict(tiles=out[0], slabs=out[1], edges=out[2], resolved_exactly=out[3])
