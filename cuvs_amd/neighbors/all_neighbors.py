"""All-neighbours kNN graph build (reference: python/cuvs/cuvs/neighbors/all_neighbors/all_neighbors.pyx over
c/include/cuvs/neighbors/all_neighbors.h)."""
import ctypes as C

import numpy as np
import torch

from .._lib import Tensor, check, lib
from ..common import auto_sync_resources
from ..distance import DISTANCE_NAMES, DISTANCE_TYPES
from . import ivf_pq as _ivf_pq
from . import nn_descent as _nn_descent

ALGOS = {"brute_force": 0, "ivf_pq": 1, "nn_descent": 2}
_ALGO_NAMES = {v: k for k, v in ALGOS.items()}


class _CParams(C.Structure):
    _fields_ = [
        ("algo", C.c_int),
        ("overlap_factor", C.c_size_t),
        ("n_clusters", C.c_size_t),
        ("metric", C.c_int),
        ("ivf_pq_params", C.c_void_p),
        ("nn_descent_params", C.c_void_p),
    ]


def _algo_from(algo):
    if isinstance(algo, str):
        if algo not in ALGOS:
            raise ValueError(f"Invalid algo: {algo}")
        return ALGOS[algo]
    if isinstance(algo, int):
        return algo
    raise ValueError(f"Invalid algo type: {type(algo)}")


class AllNeighborsParams:
    """Holds a cuvsAllNeighborsIndexParams by value. The nested parameter objects stay owned by their Python wrappers
    (kept alive here); the struct only borrows their pointers, so nothing is freed twice."""

    def __init__(self, *, algo="nn_descent", overlap_factor=2, n_clusters=1, metric="sqeuclidean", ivf_pq_params=None,
                 nn_descent_params=None):
        self.params = _CParams()
        self.params.algo = _algo_from(algo)
        self.params.overlap_factor = overlap_factor
        self.params.n_clusters = n_clusters
        self.params.metric = DISTANCE_TYPES[metric]
        if ivf_pq_params is not None:
            if not isinstance(ivf_pq_params, _ivf_pq.IndexParams):
                raise TypeError("ivf_pq_params must be an instance of cuvs_amd.neighbors.ivf_pq.IndexParams")
            if DISTANCE_TYPES[ivf_pq_params.metric] != DISTANCE_TYPES[metric]:
                raise ValueError(f"Metric conflict: AllNeighborsParams metric '{metric}' does not match IVF-PQ metric "
                                 f"'{ivf_pq_params.metric}'. Please ensure both use the same metric.")
        if nn_descent_params is not None:
            if not isinstance(nn_descent_params, _nn_descent.IndexParams):
                raise TypeError("nn_descent_params must be an instance of cuvs_amd.neighbors.nn_descent.IndexParams")
            nnd_metric = int(nn_descent_params._p.contents.metric)
            if nnd_metric != DISTANCE_TYPES[metric]:
                raise ValueError(f"Metric conflict: AllNeighborsParams metric '{metric}' does not match NN-Descent metric "
                                 f"'{DISTANCE_NAMES.get(nnd_metric, nnd_metric)}'. Please ensure both use the same metric.")
        self._ivf_pq_params = ivf_pq_params
        self._nn_descent_params = nn_descent_params
        self.params.ivf_pq_params = C.cast(ivf_pq_params._p, C.c_void_p) if ivf_pq_params is not None else None
        self.params.nn_descent_params = C.cast(nn_descent_params._p, C.c_void_p) if nn_descent_params is not None else None

    def get_handle(self):
        return C.addressof(self.params)

    @property
    def algo(self):
        return _ALGO_NAMES.get(self.params.algo, self.params.algo)

    @property
    def overlap_factor(self):
        return self.params.overlap_factor

    @property
    def n_clusters(self):
        return self.params.n_clusters

    @property
    def metric(self):
        for name, value in DISTANCE_TYPES.items():
            if value == self.params.metric:
                return name
        return self.params.metric


@auto_sync_resources
def build(dataset, k, params, *, indices=None, distances=None, core_distances=None, alpha=1.0, resources=None):
    """kNN graph of `dataset` against itself. dataset: float32 [n, dim]; a torch device tensor is a device dataset, a numpy
    array (or host tensor) a host dataset - batching (n_clusters > 1) needs the latter. indices (int64 [n, k]), distances
    (float32 [n, k]) and core_distances (float32 [n]) are optional device output buffers. With core_distances, distances
    holds mutual-reachability distances. Returns (indices, distances, core_distances); the latter two are None unless
    their buffers were given."""
    if not isinstance(params, AllNeighborsParams):
        raise TypeError("params must be an instance of AllNeighborsParams")
    on_device = isinstance(dataset, torch.Tensor) and dataset.is_cuda
    if on_device and params.n_clusters > 1:
        raise ValueError("Batched all-neighbors build is not supported with data on device. Put data on host for batch build.")
    if core_distances is not None and distances is None:
        raise ValueError("distances must be provided when core_distances is provided")
    for name, out in (("indices", indices), ("distances", distances), ("core_distances", core_distances)):
        if out is not None and not (isinstance(out, torch.Tensor) and out.is_cuda):
            raise ValueError(f"{name} must be a device tensor")
    if isinstance(dataset, torch.Tensor):
        ds = dataset.contiguous()
    else:
        ds = np.ascontiguousarray(dataset)
    if len(ds.shape) != 2:
        raise ValueError("dataset must be a matrix")
    if indices is None:
        indices = torch.empty((ds.shape[0], k), dtype=torch.int64, device="cuda")
    td, ti = Tensor(ds), Tensor(indices)
    tdist = Tensor(distances) if distances is not None else None
    tcore = Tensor(core_distances) if core_distances is not None else None
    fn = lib().cuvsAllNeighborsBuild
    fn.argtypes = [C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float]
    check(fn(resources.get_c_obj(), params.get_handle(), C.addressof(td.m), C.addressof(ti.m),
             C.addressof(tdist.m) if tdist is not None else None, C.addressof(tcore.m) if tcore is not None else None,
             C.c_float(alpha)))
    return indices, distances, core_distances


@auto_sync_resources
def partition(dataset, params, resources=None):
    """The clustering step of a batched build on its own (cuvsAmdAllNeighborsPartition): returns (centroids float32
    [n_clusters, dim], nearest_clusters int64 [n, overlap_factor]) as numpy arrays."""
    ds = np.ascontiguousarray(dataset, dtype=np.float32)
    cent = np.empty((params.n_clusters, ds.shape[1]), dtype=np.float32)
    near = np.empty((ds.shape[0], params.overlap_factor), dtype=np.int64)
    td, tc, tn = Tensor(ds), Tensor(cent), Tensor(near)
    fn = lib().cuvsAmdAllNeighborsPartition
    fn.argtypes = [C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    check(fn(resources.get_c_obj(), params.get_handle(), C.addressof(td.m), C.addressof(tc.m), C.addressof(tn.m)))
    return cent, near


@auto_sync_resources
def merge(inverted_indices, batch_indices, batch_distances, global_indices, global_distances, select_min=True, resources=None):
    """One launch of the remap-merge kernel (cuvsAmdAllNeighborsMerge); all arguments are device tensors, the global
    matrices are updated in place."""
    ts = [Tensor(t) for t in (inverted_indices, batch_indices, batch_distances, global_indices, global_distances)]
    fn = lib().cuvsAmdAllNeighborsMerge
    fn.argtypes = [C.c_size_t] + [C.c_void_p] * 5 + [C.c_int]
    check(fn(resources.get_c_obj(), *[C.addressof(t.m) for t in ts], C.c_int(1 if select_min else 0)))
    return global_indices, global_distances
