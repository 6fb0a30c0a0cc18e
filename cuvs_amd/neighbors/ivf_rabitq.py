"""IVF-RaBitQ: IVF lists of 1-bit RaBitQ codes plus extended bits, searched in two stages (reference:
cpp/include/cuvs/neighbors/ivf_rabitq.hpp; C entry points: include/cuvs_amd/ivf_rabitq.h)."""
import ctypes as C

import numpy as np
import torch

from .._lib import DLDataType, Tensor, check, lib
from ..common import auto_sync_resources
from ..distance import DISTANCE_TYPES
from ._util import as_device, out_buffers

SEARCH_MODES = {"lut16": 0, "lut32": 1, "quant4": 2, "quant8": 3}


class _CIndexParams(C.Structure):
    _fields_ = [
        ("metric", C.c_int),
        ("n_lists", C.c_uint32),
        ("bits_per_dim", C.c_uint32),
        ("kmeans_n_iters", C.c_uint32),
        ("max_train_points_per_cluster", C.c_uint32),
        ("fast_quantize_flag", C.c_bool),
        ("streaming_batch_size", C.c_uint32),
        ("force_streaming", C.c_bool),
    ]


class _CSearchParams(C.Structure):
    _fields_ = [("n_probes", C.c_uint32), ("mode", C.c_int)]


class _CIndex(C.Structure):
    _fields_ = [("addr", C.c_size_t), ("dtype", DLDataType)]


class IndexParams:
    def __init__(self, *, n_lists=1024, metric="sqeuclidean", bits_per_dim=3, kmeans_n_iters=20, max_train_points_per_cluster=256,
                 fast_quantize_flag=True, streaming_batch_size=100000, force_streaming=False):
        self._p = C.POINTER(_CIndexParams)()
        check(lib().cuvsAmdIvfRabitqIndexParamsCreate(C.byref(self._p)))
        p = self._p.contents
        p.metric = DISTANCE_TYPES[metric]
        p.n_lists = n_lists
        p.bits_per_dim = bits_per_dim
        p.kmeans_n_iters = kmeans_n_iters
        p.max_train_points_per_cluster = max_train_points_per_cluster
        p.fast_quantize_flag = fast_quantize_flag
        p.streaming_batch_size = streaming_batch_size
        p.force_streaming = force_streaming
        self.metric = metric

    def __del__(self):
        try:
            lib().cuvsAmdIvfRabitqIndexParamsDestroy(self._p)
        except Exception:
            pass


class SearchParams:
    def __init__(self, *, n_probes=20, mode="quant4"):
        self._p = C.POINTER(_CSearchParams)()
        check(lib().cuvsAmdIvfRabitqSearchParamsCreate(C.byref(self._p)))
        self._p.contents.n_probes = n_probes
        self._p.contents.mode = SEARCH_MODES[mode] if isinstance(mode, str) else int(mode)

    @property
    def n_probes(self):
        return self._p.contents.n_probes

    @property
    def mode(self):
        return self._p.contents.mode

    def __del__(self):
        try:
            lib().cuvsAmdIvfRabitqSearchParamsDestroy(self._p)
        except Exception:
            pass


class Index:
    def __init__(self):
        self._p = C.POINTER(_CIndex)()
        check(lib().cuvsAmdIvfRabitqIndexCreate(C.byref(self._p)))
        self.trained = False

    def __del__(self):
        try:
            lib().cuvsAmdIvfRabitqIndexDestroy(self._p)
        except Exception:
            pass

    def _scalar(self, fn):
        v = C.c_int64(0)
        check(getattr(lib(), fn)(self._p, C.byref(v)))
        return v.value

    n_lists = property(lambda self: self._scalar("cuvsAmdIvfRabitqIndexGetNLists"))
    dim = property(lambda self: self._scalar("cuvsAmdIvfRabitqIndexGetDim"))
    bits_per_dim = property(lambda self: self._scalar("cuvsAmdIvfRabitqIndexGetBitsPerDim"))

    def __len__(self):
        return self._scalar("cuvsAmdIvfRabitqIndexGetSize")


def _prep(ds):
    if isinstance(ds, torch.Tensor):
        return ds.contiguous()
    return np.ascontiguousarray(ds)


@auto_sync_resources
def build(index_params, dataset, resources=None):
    """dataset: fp32 [n, dim]; a torch tensor on the device, or a host tensor / numpy array (streamed in batches when
    index_params.force_streaming is set or the dataset is large)."""
    idx = Index()
    t = Tensor(_prep(dataset))
    check(lib().cuvsAmdIvfRabitqBuild(resources.get_c_obj(), index_params._p, t.ptr, idx._p))
    idx.trained = True
    return idx


@auto_sync_resources
def search(search_params, index, queries, k, neighbors=None, distances=None, resources=None):
    if not index.trained:
        raise ValueError("Index needs to be built before calling search.")
    q = as_device(queries)
    neighbors, distances = out_buffers(q.shape[0], k, neighbors, distances)
    tq, tn, td = Tensor(q), Tensor(neighbors), Tensor(distances)
    check(lib().cuvsAmdIvfRabitqSearch(resources.get_c_obj(), search_params._p, index._p, tq.ptr, tn.ptr, td.ptr))
    return distances, neighbors


def last_search_stats():
    """Counters of the calling thread's last search: (row, query) pairs screened in the tail, survivors of the screen, head rows
    re-scored, bytes the screen read."""
    out = (C.c_uint64 * 4)()
    check(lib().cuvsAmdIvfRabitqLastSearchStats(out))
    return dict(screened=out[0], survivors=out[1], head_rows=out[2], screen_bytes=out[3])


def scaling_factor(padded_dim, ex_bits):
    """the constant scaling factor t of the extended codes for a (padded dimension, extended bits) pair"""
    t = C.c_float(0)
    check(lib().cuvsAmdIvfRabitqScalingFactor(C.c_uint32(padded_dim), C.c_uint32(ex_bits), C.byref(t)))
    return np.float32(t.value)


def export_for_oracle(index, resources=None):
    """Host copy of the index, rows in list order, in the file's encodings (include/cuvs_amd/ivf_rabitq.h:
    cuvsAmdIvfRabitqExport); `centers` (unrotated) only for an index that was built here; tests only."""
    from ..common import Resources

    resources = resources or Resources()
    n, n_lists, dim, ex = len(index), index.n_lists, index.dim, index.bits_per_dim - 1
    D = (dim + 63) // 64 * 64
    out = dict(
        centers_rot=np.empty((n_lists, D), np.float32), rotation=np.empty((D, D), np.float32),
        list_sizes=np.empty(n_lists, np.uint32), ids=np.empty(n, np.uint32), bit_codes=np.empty((n, D // 32), np.uint32),
        short_factors=np.empty((n, 3), np.float32), ex_codes=np.empty((n, D * ex // 8), np.uint8),
        ex_factors=np.empty((n, 2), np.float32))
    t = C.c_float(0)
    ptr = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    check(lib().cuvsAmdIvfRabitqExport(resources.get_c_obj(), index._p, ptr(out["centers_rot"]), ptr(out["rotation"]),
                                       ptr(out["list_sizes"]), ptr(out["ids"]), ptr(out["bit_codes"]), ptr(out["short_factors"]),
                                       ptr(out["ex_codes"]), ptr(out["ex_factors"]), C.byref(t)))
    centers = np.empty((n_lists, dim), np.float32)
    if lib().cuvsAmdIvfRabitqExportCenters(resources.get_c_obj(), index._p, ptr(centers)) == 1:
        out["centers"] = centers
    out.update(t=np.float32(t.value), dim=dim, ex_bits=ex, n=n)
    return out


@auto_sync_resources
def save(filename, index, resources=None):
    check(lib().cuvsAmdIvfRabitqSerialize(resources.get_c_obj(), C.c_char_p(filename.encode()), index._p))


@auto_sync_resources
def load(filename, resources=None):
    idx = Index()
    check(lib().cuvsAmdIvfRabitqDeserialize(resources.get_c_obj(), C.c_char_p(filename.encode()), idx._p))
    idx.trained = True
    return idx
