"""Tiered index: an ANN index (CAGRA, IVF-Flat or IVF-PQ) over the first rows plus an exact brute-force tail over the rows
added since (reference: python/cuvs/cuvs/neighbors/tiered_index/tiered_index.pyx over c/include/cuvs/neighbors/tiered_index.h).
compact, info, search_tiers, tail_search and merge_tiers are this library's extensions (include/cuvs_amd/extensions.h)."""
import contextlib
import ctypes as C

import numpy as np
import torch

from .._lib import DLDataType, Tensor, check, cuvsFilter, lib
from ..common import auto_sync_resources
from ..distance import DISTANCE_NAMES, DISTANCE_TYPES
from . import cagra as _cagra
from . import ivf_flat as _ivf_flat
from . import ivf_pq as _ivf_pq
from ._util import as_device, make_filter, out_buffers

ALGO_TYPES = {"cagra": 0, "ivf_flat": 1, "ivf_pq": 2}
ALGO_NAMES = {v: k for k, v in ALGO_TYPES.items()}
_UPSTREAM = {"cagra": _cagra, "ivf_flat": _ivf_flat, "ivf_pq": _ivf_pq}


class _CIndexParams(C.Structure):
    _fields_ = [
        ("metric", C.c_int),
        ("algo", C.c_int),
        ("min_ann_rows", C.c_int64),
        ("create_ann_index_on_extend", C.c_bool),
        ("cagra_params", C.c_void_p),
        ("ivf_flat_params", C.c_void_p),
        ("ivf_pq_params", C.c_void_p),
    ]


class _CIndex(C.Structure):
    _fields_ = [("addr", C.c_size_t), ("dtype", DLDataType), ("algo", C.c_int)]


class IndexParams:
    """metric: "sqeuclidean" | "euclidean" | "inner_product" | "cosine"; algo: "cagra" | "ivf_flat" | "ivf_pq";
    upstream_params: that algo's IndexParams (None: its defaults; when given, its metric is the one that counts, as in the
    reference); min_ann_rows: an ANN tier is built over more rows than this; create_ann_index_on_extend: rebuild the ANN tier
    over all rows when an extend leaves more than min_ann_rows rows in the tail."""

    def __init__(self, *, metric="sqeuclidean", algo="cagra", upstream_params=None, min_ann_rows=None,
                 create_ann_index_on_extend=None):
        if algo not in ALGO_TYPES:
            raise ValueError(f"Unknown algorithm '{algo}'")
        self._p = C.POINTER(_CIndexParams)()
        check(lib().cuvsTieredIndexParamsCreate(C.byref(self._p)))
        p = self._p.contents
        p.metric = DISTANCE_TYPES[metric]
        p.algo = ALGO_TYPES[algo]
        if min_ann_rows is not None:
            p.min_ann_rows = min_ann_rows
        if create_ann_index_on_extend is not None:
            p.create_ann_index_on_extend = create_ann_index_on_extend
        self._upstream_params = upstream_params
        if upstream_params is not None:
            want = _UPSTREAM[algo].IndexParams
            if not isinstance(upstream_params, want):
                raise TypeError(f"Expected {algo}.IndexParams, got {upstream_params.__class__} ")
            setattr(p, algo + "_params", C.cast(upstream_params._p, C.c_void_p))

    def __del__(self):
        try:
            lib().cuvsTieredIndexParamsDestroy(self._p)
        except Exception:
            pass

    @property
    def metric(self):
        return DISTANCE_NAMES[self._p.contents.metric]

    @property
    def algo(self):
        return ALGO_NAMES[self._p.contents.algo]

    @property
    def min_ann_rows(self):
        return self._p.contents.min_ann_rows

    @property
    def create_ann_index_on_extend(self):
        return self._p.contents.create_ann_index_on_extend

    @property
    def upstream_params(self):
        return self._upstream_params


class Index:
    def __init__(self):
        self._p = C.POINTER(_CIndex)()
        check(lib().cuvsTieredIndexCreate(C.byref(self._p)))
        self._trained = False

    @property
    def trained(self):
        return self._trained

    @property
    def algo(self):
        return ALGO_NAMES[self._p.contents.algo]

    def __del__(self):
        try:
            lib().cuvsTieredIndexDestroy(self._p)
        except Exception:
            pass


@contextlib.contextmanager
def _upstream_ready(index_params):
    """cagra.IndexParams keeps its build algorithm on the Python side and writes it into the struct for the length of a build
    (cagra.build); the same here for the calls that read the upstream parameters."""
    up = index_params.upstream_params
    if isinstance(up, _cagra.IndexParams):
        up._p.contents.build_algo = up._c_build_algo()
        try:
            yield
        finally:
            up._p.contents.build_algo = 1  # keep Destroy's graph_build_params bookkeeping valid
    else:
        yield


def _rows(x):
    """float32 rows as they are handed to the library: a device tensor stays on the device, anything else is host memory."""
    if isinstance(x, torch.Tensor):
        return x.contiguous()
    return np.ascontiguousarray(x)


@auto_sync_resources
def build(index_params, dataset, resources=None):
    """dataset: float32 [n, dim], device tensor or host array."""
    idx = Index()
    t = Tensor(_rows(dataset))
    with _upstream_ready(index_params):
        check(lib().cuvsTieredIndexBuild(resources.get_c_obj(), index_params._p, t.ptr, idx._p))
    idx._trained = True
    return idx


def _search_params_ptr(search_params, index):
    if search_params is None:
        return None
    want = _UPSTREAM[index.algo].SearchParams
    if not isinstance(search_params, want):
        raise TypeError(f"Expected {index.algo}.SearchParams, got {search_params.__class__}")
    return C.cast(search_params._p, C.c_void_p)


def _filter(filter):
    """filter: None, a tensor of uint32 (or int32) words of a bitset over the index's rows (1 keeps a row), or the (words, type)
    pair the other modules take."""
    if filter is None or isinstance(filter, tuple):
        return make_filter(filter)
    return make_filter((filter, 1))


@auto_sync_resources
def search(search_params, index, queries, k, neighbors=None, distances=None, resources=None, filter=None):
    """search_params: the ANN algo's SearchParams, or None for its defaults. Returns (distances, neighbors)."""
    if not index.trained:
        raise ValueError("Index needs to be built before calling search.")
    q = as_device(queries)
    neighbors, distances = out_buffers(q.shape[0], k, neighbors, distances)
    flt, keep = _filter(filter)
    tq, tn, td = Tensor(q), Tensor(neighbors), Tensor(distances)
    fn = lib().cuvsTieredIndexSearch
    fn.argtypes = [C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, cuvsFilter]
    check(fn(resources.get_c_obj(), _search_params_ptr(search_params, index), index._p, tq.ptr, tn.ptr, td.ptr, flt))
    del keep
    return distances, neighbors


@auto_sync_resources
def extend(index, new_vectors, resources=None):
    """Appends float32 rows (device tensor or host array) behind the rows already held."""
    t = Tensor(_rows(new_vectors))
    check(lib().cuvsTieredIndexExtend(resources.get_c_obj(), t.ptr, index._p))
    return index


@auto_sync_resources
def merge(index_params, indices, resources=None, output=None):
    """The rows of `indices` in order behind one index; `output`: an Index to receive the result (what it held is freed)."""
    out = output if output is not None else Index()
    arr = (C.POINTER(_CIndex) * len(indices))(*[i._p for i in indices])
    fn = lib().cuvsTieredIndexMerge
    fn.argtypes = [C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    with _upstream_ready(index_params):
        check(fn(resources.get_c_obj(), C.cast(index_params._p, C.c_void_p), C.cast(arr, C.c_void_p), len(indices),
                 C.cast(out._p, C.c_void_p)))
    out._trained = True
    return out


@auto_sync_resources
def compact(index, resources=None):
    """Rebuilds the ANN tier over all rows when the tail is not empty (cuvsAmdTieredIndexCompact)."""
    check(lib().cuvsAmdTieredIndexCompact(resources.get_c_obj(), index._p))
    return index


def info(index):
    """(size, ann_rows, capacity, dim) of a built index."""
    v = [C.c_int64(0) for _ in range(4)]
    check(lib().cuvsAmdTieredIndexGetInfo(index._p, *[C.byref(x) for x in v]))
    return tuple(x.value for x in v)


@auto_sync_resources
def search_tiers(search_params, index, queries, k, resources=None, filter=None):
    """The two inputs of a search's merge: (ann_distances, ann_neighbors, tail_distances, tail_neighbors), each [m, k]."""
    q = as_device(queries)
    an, ad = out_buffers(q.shape[0], k, None, None)
    tn, td = out_buffers(q.shape[0], k, None, None)
    flt, keep = _filter(filter)
    ts = [Tensor(x) for x in (q, an, ad, tn, td)]
    fn = lib().cuvsAmdTieredIndexSearchTiers
    fn.argtypes = [C.c_size_t, C.c_void_p, C.c_void_p] + [C.c_void_p] * 5 + [cuvsFilter]
    check(fn(resources.get_c_obj(), _search_params_ptr(search_params, index), index._p, *[t.ptr for t in ts], flt))
    del keep
    return ad, an, td, tn


PATHS = {"auto": 0, "composed": 1, "fused": 2}


@auto_sync_resources
def tail_search(metric, tail, ann_rows, queries, seed_neighbors, seed_distances, bitset=None, path="auto", resources=None):
    """The tail phase of a search on its own (cuvsAmdTieredTailSearch): all tensors on the device. Returns
    (distances, neighbors)."""
    q = as_device(queries)
    k = seed_neighbors.shape[1]
    neighbors, distances = out_buffers(q.shape[0], k, None, None)
    ts = [Tensor(as_device(tail)), Tensor(q), Tensor(seed_neighbors), Tensor(seed_distances)]
    tb = None
    if bitset is not None:
        tb = Tensor(bitset)
        tb.m.dl_tensor.dtype.code = 1  # int32 words are read as uint32
    tn, td = Tensor(neighbors), Tensor(distances)
    fn = lib().cuvsAmdTieredTailSearch
    fn.argtypes = [C.c_size_t, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                   C.c_void_p]
    check(fn(resources.get_c_obj(), DISTANCE_TYPES[metric], ts[0].ptr, ann_rows, ts[1].ptr, ts[2].ptr, ts[3].ptr,
             tb.ptr if tb is not None else None, PATHS[path], tn.ptr, td.ptr))
    return distances, neighbors


@auto_sync_resources
def merge_tiers(a_neighbors, a_distances, b_neighbors, b_distances, ann_rows, select_min=True, resources=None):
    """One launch of the merge kernel (cuvsAmdTieredMerge): A [m, k] + B [m, kb] -> (distances, neighbors) [m, k]."""
    neighbors, distances = out_buffers(a_neighbors.shape[0], a_neighbors.shape[1], None, None)
    ts = [Tensor(x) for x in (a_neighbors, a_distances, b_neighbors, b_distances)]
    tn, td = Tensor(neighbors), Tensor(distances)
    fn = lib().cuvsAmdTieredMerge
    fn.argtypes = [C.c_size_t] + [C.c_void_p] * 4 + [C.c_int64, C.c_int, C.c_void_p, C.c_void_p]
    check(fn(resources.get_c_obj(), *[t.ptr for t in ts], ann_rows, 1 if select_min else 0, tn.ptr, td.ptr))
    return distances, neighbors


def counters():
    """(composed tail phases, single-launch tail phases, tail phases redone exactly) since the library was loaded."""
    out = (C.c_ulonglong * 3)()
    lib().cuvsAmdTieredCounters(out)
    return tuple(out)
