"""HNSW: a CAGRA graph handed over to host search (reference: python/cuvs/cuvs/neighbors/hnsw/hnsw.pyx over
c/include/cuvs/neighbors/hnsw.h). `from_cagra` and `build` run on the device; the index lives in host memory, and `load`,
`save`, `extend` and `search` are host code that needs no GPU (they take no resources handle into the library)."""
import ctypes as C
import os

import numpy as np

from .._lib import DLDataType, Tensor, _NP_DT, check, lib
from ..common import auto_sync_resources
from ..distance import DISTANCE_TYPES

_METRIC_NAMES = {v: k for k, v in DISTANCE_TYPES.items()}
_HIERARCHY = {"none": 0, "cpu": 1, "gpu": 2}
_HIERARCHY_NAMES = {v: k for k, v in _HIERARCHY.items()}


class _CAceParams(C.Structure):
    _fields_ = [("npartitions", C.c_size_t), ("build_dir", C.c_char_p), ("use_disk", C.c_bool),
                ("max_host_memory_gb", C.c_double), ("max_gpu_memory_gb", C.c_double)]


class _CIndexParams(C.Structure):
    _fields_ = [("hierarchy", C.c_int), ("ef_construction", C.c_int), ("num_threads", C.c_int), ("M", C.c_size_t),
                ("metric", C.c_int), ("ace_params", C.POINTER(_CAceParams))]


class _CIndex(C.Structure):
    _fields_ = [("addr", C.c_size_t), ("dtype", DLDataType)]


class _CExtendParams(C.Structure):
    _fields_ = [("num_threads", C.c_int)]


class _CSearchParams(C.Structure):
    _fields_ = [("ef", C.c_int32), ("num_threads", C.c_int32)]


class AceParams:
    """npartitions (0), build_dir ("/tmp/hnsw_ace_build"), use_disk (False), max_host_memory_gb (0), max_gpu_memory_gb (0).
    Only use_disk / build_dir act: `build` then also writes <build_dir>/hnsw_index.bin."""

    def __init__(self, *, npartitions=0, build_dir="/tmp/hnsw_ace_build", use_disk=False, max_host_memory_gb=0.0, max_gpu_memory_gb=0.0):
        self._p = C.POINTER(_CAceParams)()
        check(lib().cuvsHnswAceParamsCreate(C.byref(self._p)))
        self._build_dir = os.fsencode(str(build_dir))  # kept alive: the struct holds the pointer
        p = self._p.contents
        p.npartitions = npartitions
        p.build_dir = self._build_dir
        p.use_disk = use_disk
        p.max_host_memory_gb = max_host_memory_gb
        p.max_gpu_memory_gb = max_gpu_memory_gb

    npartitions = property(lambda self: self._p.contents.npartitions)
    build_dir = property(lambda self: os.fsdecode(self._p.contents.build_dir))
    use_disk = property(lambda self: self._p.contents.use_disk)
    max_host_memory_gb = property(lambda self: self._p.contents.max_host_memory_gb)
    max_gpu_memory_gb = property(lambda self: self._p.contents.max_gpu_memory_gb)

    def __del__(self):
        try:
            lib().cuvsHnswAceParamsDestroy(self._p)
        except Exception:
            pass


class IndexParams:
    """hierarchy ("gpu"; "none", "cpu"), ef_construction (200), num_threads (0; accepted, unused), M (32) and metric
    ("sqeuclidean"; "inner_product") for `build`, ace_params (None; `build` requires them)."""

    def __init__(self, *, hierarchy="gpu", ef_construction=200, num_threads=0, M=32, metric="sqeuclidean", ace_params=None):
        self._p = C.POINTER(_CIndexParams)()
        check(lib().cuvsHnswIndexParamsCreate(C.byref(self._p)))
        p = self._p.contents
        p.hierarchy = _HIERARCHY[hierarchy]
        p.ef_construction = ef_construction
        p.num_threads = num_threads
        p.M = M
        p.metric = DISTANCE_TYPES[metric]
        self._ace = ace_params
        if ace_params is not None:
            p.ace_params = ace_params._p

    hierarchy = property(lambda self: _HIERARCHY_NAMES[self._p.contents.hierarchy])
    ef_construction = property(lambda self: self._p.contents.ef_construction)
    num_threads = property(lambda self: self._p.contents.num_threads)
    M = property(lambda self: self._p.contents.M)
    metric = property(lambda self: _METRIC_NAMES[self._p.contents.metric])
    ace_params = property(lambda self: self._ace)

    def __del__(self):
        try:
            lib().cuvsHnswIndexParamsDestroy(self._p)
        except Exception:
            pass


class ExtendParams:
    """num_threads (0; accepted, unused: the insert is sequential)."""

    def __init__(self, *, num_threads=0):
        self._p = C.POINTER(_CExtendParams)()
        check(lib().cuvsHnswExtendParamsCreate(C.byref(self._p)))
        self._p.contents.num_threads = num_threads

    num_threads = property(lambda self: self._p.contents.num_threads)

    def __del__(self):
        try:
            lib().cuvsHnswExtendParamsDestroy(self._p)
        except Exception:
            pass


class SearchParams:
    """ef (200), num_threads (0: OMP_NUM_THREADS if set, else the hardware concurrency)."""

    def __init__(self, *, ef=200, num_threads=0):
        self._p = C.POINTER(_CSearchParams)()
        check(lib().cuvsHnswSearchParamsCreate(C.byref(self._p)))
        self._p.contents.ef = ef
        self._p.contents.num_threads = num_threads

    ef = property(lambda self: self._p.contents.ef)
    num_threads = property(lambda self: self._p.contents.num_threads)

    def __del__(self):
        try:
            lib().cuvsHnswSearchParamsDestroy(self._p)
        except Exception:
            pass


class Index:
    def __init__(self):
        self._p = C.POINTER(_CIndex)()
        check(lib().cuvsHnswIndexCreate(C.byref(self._p)))
        self.trained = False

    def __del__(self):
        try:
            lib().cuvsHnswIndexDestroy(self._p)
        except Exception:
            pass

    def __repr__(self):
        return f"Index(type=HNSW, trained={self.trained})"


def _host(a, what):
    if not isinstance(a, np.ndarray):
        raise TypeError(f"{what} must be a host numpy array")
    return np.ascontiguousarray(a)


@auto_sync_resources
def from_cagra(index_params, cagra_index, dataset=None, resources=None):
    """Converts a cuvs_amd.neighbors.cagra index. dataset (optional; torch on the device or numpy on the host): the rows, for
    an index that holds VPQ codes only."""
    idx = Index()
    if dataset is None:
        check(lib().cuvsHnswFromCagra(resources.get_c_obj(), index_params._p, cagra_index._p, idx._p))
    else:
        ds = np.ascontiguousarray(dataset) if isinstance(dataset, np.ndarray) else dataset.contiguous()
        check(lib().cuvsHnswFromCagraWithDataset(resources.get_c_obj(), index_params._p, cagra_index._p, idx._p, Tensor(ds).ptr))
    idx.trained = True
    return idx


@auto_sync_resources
def build(index_params, dataset, resources=None):
    """CAGRA build (graph_degree 2 M, intermediate 3 M) on the device followed by the conversion. dataset: host numpy
    [n, dim] float32 / float16 / int8 / uint8 (a device torch tensor is taken too)."""
    ds = np.ascontiguousarray(dataset) if isinstance(dataset, np.ndarray) else dataset.contiguous()
    idx = Index()
    check(lib().cuvsHnswBuild(resources.get_c_obj(), index_params._p, Tensor(ds).ptr, idx._p))
    idx.trained = True
    return idx


def save(filename, index, resources=None):
    """hnswlib's saveIndex layout (host only)."""
    check(lib().cuvsHnswSerialize(C.c_size_t(0), os.fsencode(str(filename)), index._p))


def load(index_params, filename, dim, dtype, metric="sqeuclidean", resources=None):
    """Reads a file of `save`, or with hierarchy "none" one of cagra.save(..., to_hnswlib) (host only). dtype: numpy dtype of the rows."""
    idx = Index()
    code, bits = _NP_DT[np.dtype(dtype)]
    idx._p.contents.dtype = DLDataType(code, bits, 1)
    check(lib().cuvsHnswDeserialize(C.c_size_t(0), index_params._p, os.fsencode(str(filename)), C.c_int(dim),
                                    C.c_int(DISTANCE_TYPES[metric]), idx._p))
    idx.trained = True
    return idx


def extend(extend_params, index, data, resources=None):
    """Appends host rows (numpy, the index's dtype); an index of hierarchy "none" is refused (host only)."""
    check(lib().cuvsHnswExtend(C.c_size_t(0), extend_params._p, Tensor(_host(data, "data")).ptr, index._p))
    return index


def search(search_params, index, queries, k, neighbors=None, distances=None, resources=None):
    """queries: host numpy [m, dim] of the index's dtype. Returns (distances float32 [m, k], neighbors uint64 [m, k]) on the
    host; slots past the rows a walk reached hold 2^64 - 1 and the largest float (host only)."""
    q = _host(queries, "queries")
    m = q.shape[0]
    neighbors = np.empty((m, k), dtype=np.uint64) if neighbors is None else neighbors
    distances = np.empty((m, k), dtype=np.float32) if distances is None else distances
    check(lib().cuvsHnswSearch(C.c_size_t(0), search_params._p, index._p, Tensor(q).ptr, Tensor(neighbors).ptr, Tensor(distances).ptr))
    return distances, neighbors
