"""Random ball cover: a landmark index over 2-D / 3-D points, exact k-NN and eps_nn through it by the triangle inequality
(reference: cpp/include/cuvs/neighbors/ball_cover.hpp; C entry points: include/cuvs_amd/ball_cover.h).

Metrics: "euclidean" (the L2 chain of DESIGN 3.1t, then sqrtf) and "haversine" over (latitude, longitude) rows in radians.
With post-filtering and weight 1 (the defaults) knn_query returns what brute force returns under (distance, id), whatever
landmarks were drawn. Rows and queries are fp32 torch tensors on the device; the library refuses anything else."""
import ctypes as C
import operator

import torch

from .._lib import DLDataType, DLManagedTensor, Tensor, check, lib, view_to_torch
from ..common import auto_sync_resources
from ..distance import DISTANCE_TYPES
from ._util import optional_tensor as _t
from ._util import out_buffers

METRICS = {"euclidean": 1, "l2": 1, "l2_sqrt_unexpanded": 5, "haversine": 13}
_ARRAYS = {"R_indptr": 0, "R_1nn_cols": 1, "R_1nn_dists": 2, "R_radius": 3, "R": 4, "X_reordered": 5, "R_rows": 6}


def _metric(metric):
    if isinstance(metric, str):
        return METRICS[metric] if metric in METRICS else DISTANCE_TYPES[metric]  # (the library refuses the others)
    return int(metric)


class _CIndexParams(C.Structure):
    _fields_ = [("metric", C.c_int), ("n_landmarks", C.c_uint32), ("seed", C.c_uint32)]


class _CIndex(C.Structure):
    _fields_ = [("addr", C.c_size_t), ("dtype", DLDataType)]


class IndexParams:
    """metric: "euclidean" or "haversine"; n_landmarks: 0 takes floor(sqrt(m)); the landmarks are a fixed function of
    (m, n_landmarks, seed)."""

    def __init__(self, *, metric="euclidean", n_landmarks=0, seed=0):
        self._p = None
        for name, v in (("n_landmarks", n_landmarks), ("seed", seed)):  # c_uint32 would wrap them silently
            try:
                ok = 0 <= operator.index(v) < 2 ** 32
            except TypeError:
                ok = False
            if not ok:
                raise ValueError(f"ball cover: {name} must be an integer in [0, 2^32), got {v!r}")
        self._p = C.POINTER(_CIndexParams)()
        check(lib().cuvsAmdBallCoverIndexParamsCreate(C.byref(self._p)))
        p = self._p.contents
        p.metric = _metric(metric)
        p.n_landmarks = operator.index(n_landmarks)
        p.seed = operator.index(seed)
        self.metric = metric

    def __del__(self):
        try:
            if self._p is not None:
                lib().cuvsAmdBallCoverIndexParamsDestroy(self._p)
        except Exception:
            pass


class Index:
    def __init__(self):
        self._p = C.POINTER(_CIndex)()
        check(lib().cuvsAmdBallCoverIndexCreate(C.byref(self._p)))
        self.trained = False

    def __del__(self):
        try:
            lib().cuvsAmdBallCoverIndexDestroy(self._p)
        except Exception:
            pass

    def _scalar(self, fn):
        v = C.c_int64(0)
        check(getattr(lib(), fn)(self._p, C.byref(v)))
        return v.value

    n_landmarks = property(lambda self: self._scalar("cuvsAmdBallCoverIndexGetNLandmarks"))
    m = property(lambda self: self._scalar("cuvsAmdBallCoverIndexGetSize"))
    dim = property(lambda self: self._scalar("cuvsAmdBallCoverIndexGetDim"))

    @property
    def metric(self):
        v = C.c_int(0)
        check(lib().cuvsAmdBallCoverIndexGetMetric(self._p, C.byref(v)))
        return v.value

    def __len__(self):
        return self.m

    def array(self, name):
        """A copy of one array of the index as a torch tensor on the device: R_indptr, R_1nn_cols, R_1nn_dists, R_radius, R,
        X_reordered or R_rows (the landmarks' row ids)."""
        view = DLManagedTensor()
        check(lib().cuvsAmdBallCoverIndexGetArray(self._p, C.c_int(_ARRAYS[name]), C.byref(view)))
        return view_to_torch(view, "cuda")

    R_indptr = property(lambda self: self.array("R_indptr"))
    R_1nn_cols = property(lambda self: self.array("R_1nn_cols"))
    R_1nn_dists = property(lambda self: self.array("R_1nn_dists"))
    R_radius = property(lambda self: self.array("R_radius"))
    R = property(lambda self: self.array("R"))
    X_reordered = property(lambda self: self.array("X_reordered"))
    R_rows = property(lambda self: self.array("R_rows"))


@auto_sync_resources
def build(params, dataset, resources=None):
    """dataset: fp32 [m, dim] on the device. The index keeps its own reordered copy of the rows."""
    idx = Index()
    t = Tensor(dataset)
    check(lib().cuvsAmdBallCoverBuild(resources.get_c_obj(), params._p, t.ptr, idx._p))
    idx.trained = True
    return idx


@auto_sync_resources
def knn_query(index, queries, k, perform_post_filtering=True, weight=1.0, neighbors=None, distances=None, resources=None):
    """(distances fp32 [q, k], neighbors int64 [q, k]), rows sorted by (distance, id)."""
    if not index.trained:
        raise ValueError("Index needs to be built before calling knn_query.")
    neighbors, distances = out_buffers(queries.shape[0], k, neighbors, distances)
    tq, tn, td = Tensor(queries), Tensor(neighbors), Tensor(distances)
    check(lib().cuvsAmdBallCoverKnnQuery(resources.get_c_obj(), index._p, tq.ptr, tn.ptr, td.ptr, C.c_bool(perform_post_filtering),
                                         C.c_float(weight)))
    return distances, neighbors


@auto_sync_resources
def all_knn_query(params, dataset, k, perform_post_filtering=True, weight=1.0, neighbors=None, distances=None, return_index=False,
                  resources=None):
    """build + a query of the dataset against itself: (distances, neighbors[, index])."""
    neighbors, distances = out_buffers(dataset.shape[0], k, neighbors, distances)
    idx = Index() if return_index else None
    tx, tn, td = Tensor(dataset), Tensor(neighbors), Tensor(distances)
    check(lib().cuvsAmdBallCoverAllKnnQuery(resources.get_c_obj(), params._p, tx.ptr, tn.ptr, td.ptr, C.c_bool(perform_post_filtering),
                                            C.c_float(weight), idx._p if idx is not None else None))
    if idx is not None:
        idx.trained = True
        return distances, neighbors, idx
    return distances, neighbors


@auto_sync_resources
def eps_nn(index, queries, eps, adj=None, vd=None, vd_dtype=torch.int64, resources=None):
    """Dense form over an L2 index, eps the radius: adj bool [q, m] and vd [q + 1], as epsilon_neighborhood.compute with the
    squared value. `adj=False` / `vd=False` leave that output out."""
    q, m = queries.shape[0], index.m
    if adj is None:
        adj = torch.empty((q, m), dtype=torch.bool, device=queries.device)
    elif adj is False:
        adj = None
    if vd is None:
        vd = torch.empty(q + 1, dtype=vd_dtype, device=queries.device)
    elif vd is False:
        vd = None
    tq = Tensor(queries)
    ta, pa = _t(adj)
    tv, pv = _t(vd)
    check(lib().cuvsAmdBallCoverEpsNn(resources.get_c_obj(), index._p, tq.ptr, pa, pv, C.c_float(eps)))
    return adj, vd


@auto_sync_resources
def csr_count(index, queries, eps, indptr=None, vd=None, resources=None):
    """First call of the two-call protocol: indptr int64 [q + 1]; vd, when given, gets the degrees."""
    if indptr is None:
        indptr = torch.empty(queries.shape[0] + 1, dtype=torch.int64, device=queries.device)
    tq, ti = Tensor(queries), Tensor(indptr)
    tv, pv = _t(vd)
    check(lib().cuvsAmdBallCoverEpsNnCsr(resources.get_c_obj(), index._p, tq.ptr, ti.ptr, None, None, pv, C.c_float(eps), None))
    return indptr


@auto_sync_resources
def csr_fill(index, queries, eps, indptr, indices, distances=None, vd=None, max_k=None, resources=None):
    """Second call of the two-call protocol, or, with max_k, the one-call form (returns the largest degree found)."""
    tq, ti, tn = Tensor(queries), Tensor(indptr), Tensor(indices)
    td, pd = _t(distances)
    tv, pv = _t(vd)
    mk = C.c_int64(max_k) if max_k is not None else None
    check(lib().cuvsAmdBallCoverEpsNnCsr(resources.get_c_obj(), index._p, tq.ptr, ti.ptr, tn.ptr, pd, pv, C.c_float(eps),
                                         C.byref(mk) if mk is not None else None))
    return mk.value if mk is not None else None


def eps_nn_csr(index, queries, eps, max_k=None, return_distances=False, resources=None):
    """CSR form: (indptr, indices[, distances][, max_k_found]); column ids are original row ids in ascending order, distances the
    squared chain values, as epsilon_neighborhood.csr."""
    q = queries.shape[0]
    if max_k is None:
        indptr = csr_count(index, queries, eps, resources=resources)
        if resources is not None:
            resources.sync()
        nnz = int(indptr[q].item())
        indices = torch.empty(nnz, dtype=torch.int64, device=queries.device)
        distances = torch.empty(nnz, dtype=torch.float32, device=queries.device) if return_distances else None
        csr_fill(index, queries, eps, indptr, indices, distances, resources=resources)
        return (indptr, indices, distances) if return_distances else (indptr, indices)
    indptr = torch.empty(q + 1, dtype=torch.int64, device=queries.device)
    indices = torch.empty(q * max_k, dtype=torch.int64, device=queries.device)
    distances = torch.empty(q * max_k, dtype=torch.float32, device=queries.device) if return_distances else None
    found = csr_fill(index, queries, eps, indptr, indices, distances, max_k=max_k, resources=resources)
    if resources is not None:
        resources.sync()
    nnz = int(indptr[q].item())
    out = (indptr, indices[:nnz]) + ((distances[:nnz],) if return_distances else ())
    return out + (found,)


def last_stats():
    """Counters of the calling thread's last k-NN or eps_nn call."""
    out = (C.c_uint64 * 4)()
    check(lib().cuvsAmdBallCoverLastStats(out))
    return dict(lists_visited=out[0], points_scored=out[1], points_skipped=out[2], queries=out[3])
