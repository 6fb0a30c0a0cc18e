"""Vamana (DiskANN) graph build and file output (reference: python/cuvs/cuvs/neighbors/vamana/vamana.pyx over
c/include/cuvs/neighbors/vamana.h). The index is built on the device and written in DiskANN's formats; it is not searched here
(`Index.graph` can be handed to cagra.from_graph once its unused slots are replaced)."""
import ctypes as C

import numpy as np
import torch

from .._lib import CuvsError, DLDataType, Tensor, check, lib
from ..common import auto_sync_resources
from ..distance import DISTANCE_TYPES

_METRIC_NAMES = {v: k for k, v in DISTANCE_TYPES.items()}


class _CParams(C.Structure):
    _fields_ = [
        ("metric", C.c_int),
        ("graph_degree", C.c_uint32),
        ("visited_size", C.c_uint32),
        ("vamana_iters", C.c_float),
        ("alpha", C.c_float),
        ("max_fraction", C.c_float),
        ("batch_base", C.c_float),
        ("queue_size", C.c_uint32),
        ("reverse_batchsize", C.c_uint32),
    ]


class _CIndex(C.Structure):
    _fields_ = [("addr", C.c_size_t), ("dtype", DLDataType)]


class IndexParams:
    """metric ("sqeuclidean" only), graph_degree (32; one of 32, 64, 128, 256), visited_size (64), vamana_iters (1),
    alpha (1.2), max_fraction (0.06), batch_base (2), queue_size (127), reverse_batchsize (1000000)."""

    def __init__(self, *, metric="sqeuclidean", graph_degree=32, visited_size=64, vamana_iters=1, alpha=1.2, max_fraction=0.06,
                 batch_base=2.0, queue_size=127, reverse_batchsize=1000000):
        self._p = C.POINTER(_CParams)()
        check(lib().cuvsVamanaIndexParamsCreate(C.byref(self._p)))
        p = self._p.contents
        p.metric = DISTANCE_TYPES[metric]
        p.graph_degree = graph_degree
        p.visited_size = visited_size
        p.vamana_iters = vamana_iters
        p.alpha = alpha
        p.max_fraction = max_fraction
        p.batch_base = batch_base
        p.queue_size = queue_size
        p.reverse_batchsize = reverse_batchsize

    metric = property(lambda self: _METRIC_NAMES[self._p.contents.metric])
    graph_degree = property(lambda self: self._p.contents.graph_degree)
    visited_size = property(lambda self: self._p.contents.visited_size)
    vamana_iters = property(lambda self: self._p.contents.vamana_iters)
    alpha = property(lambda self: self._p.contents.alpha)
    max_fraction = property(lambda self: self._p.contents.max_fraction)
    batch_base = property(lambda self: self._p.contents.batch_base)
    queue_size = property(lambda self: self._p.contents.queue_size)
    reverse_batchsize = property(lambda self: self._p.contents.reverse_batchsize)

    def __del__(self):
        try:
            lib().cuvsVamanaIndexParamsDestroy(self._p)
        except Exception:
            pass


class Index:
    def __init__(self):
        self._p = C.POINTER(_CIndex)()
        check(lib().cuvsVamanaIndexCreate(C.byref(self._p)))
        self.trained = False
        self._shape = None
        self._res = None

    def __del__(self):
        try:
            lib().cuvsVamanaIndexDestroy(self._p)
        except Exception:
            pass

    @property
    def dim(self):
        d = C.c_int(0)
        check(lib().cuvsVamanaIndexGetDims(self._p, C.byref(d)))
        return d.value

    @property
    def medoid(self):
        m = C.c_uint32(0)
        check(lib().cuvsAmdVamanaIndexGetMedoid(self._p, C.byref(m)))
        return m.value

    @property
    def graph(self):
        """uint32 [n, graph_degree] on the device (an int32 torch tensor with the same bits); unused slots hold 0xFFFFFFFF."""
        from ..common import Resources

        if self._shape is None:
            raise CuvsError("the Vamana index is not built")
        res = self._res or Resources()
        out = torch.empty(self._shape, dtype=torch.int32, device="cuda")
        t = Tensor(out)
        t.m.dl_tensor.dtype.code = 1  # uint32; torch has no such dtype
        check(lib().cuvsAmdVamanaIndexGetGraph(res.get_c_obj(), self._p, t.ptr))
        res.sync()
        return out

    def __repr__(self):
        return f"Index(type=Vamana, trained={self.trained})"


@auto_sync_resources
def build(index_params, dataset, resources=None):
    """dataset: torch (device or host) or numpy (host) [n, dim] float32 / int8 / uint8. Returns an Index."""
    ds = dataset.contiguous() if isinstance(dataset, torch.Tensor) else np.ascontiguousarray(dataset)
    idx = Index()
    check(lib().cuvsVamanaBuild(resources.get_c_obj(), index_params._p, Tensor(ds).ptr, idx._p))
    idx.trained = True
    idx._shape = (ds.shape[0], int(index_params.graph_degree))
    idx._res = resources
    return idx


@auto_sync_resources
def save(filename, index, include_dataset=True, resources=None, *, sector_aligned=False):
    """Writes DiskANN's graph file `filename` (sector_aligned: `<filename>_disk.index` in the SSD layout) and, with
    include_dataset, the rows as `<filename>.data`."""
    fn = lib().cuvsAmdVamanaSerializeSectorAligned if sector_aligned else lib().cuvsVamanaSerialize
    check(fn(resources.get_c_obj(), str(filename).encode(), index._p, C.c_bool(include_dataset)))
