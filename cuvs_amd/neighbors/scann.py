"""ScaNN index build (reference: cuvs::neighbors::experimental::scann, cpp/include/cuvs/neighbors/scann.hpp, build-only there;
C entry points: include/cuvs_amd/scann.h; arithmetic and deviations: DESIGN.md 3.1z).

The dataset is a torch tensor on the device, or a numpy array / host tensor that is streamed in batches of 65536 rows (same index
bit for bit); fp32, row-major. `save` writes the .npy files that open-source ScaNN reads. There is no search here."""
import ctypes as C
import os

import numpy as np
import torch

from .._lib import DLManagedTensor, Tensor, check, lib, view_to_torch
from ..common import auto_sync_resources
from ..distance import DISTANCE_TYPES


class _CParams(C.Structure):
    _fields_ = [("metric", C.c_int), ("metric_arg", C.c_float), ("n_leaves", C.c_uint32), ("kmeans_n_rows_train", C.c_int64),
                ("kmeans_n_iters", C.c_uint32), ("partitioning_eta", C.c_float), ("soar_lambda", C.c_float), ("pq_dim", C.c_uint32),
                ("pq_bits", C.c_uint32), ("pq_n_rows_train", C.c_int64), ("pq_train_iters", C.c_uint32), ("reordering_bf16", C.c_bool),
                ("reordering_noise_shaping_threshold", C.c_float)]


class _CIndex(C.Structure):
    _fields_ = [("addr", C.c_size_t)]


class IndexParams:
    """scann.hpp:40-85. `pq_dim` is the width of a subspace (dim % pq_dim == 0), not the number of subspaces."""

    def __init__(self, metric="sqeuclidean", metric_arg=2.0, n_leaves=1000, kmeans_n_rows_train=100000, kmeans_n_iters=24,
                 partitioning_eta=1.0, soar_lambda=1.0, pq_dim=8, pq_bits=8, pq_n_rows_train=100000, pq_train_iters=10,
                 reordering_bf16=False, reordering_noise_shaping_threshold=float("nan")):
        self._p = C.POINTER(_CParams)()
        check(lib().cuvsAmdScannIndexParamsCreate(C.byref(self._p)))
        c = self._p.contents
        c.metric = DISTANCE_TYPES[metric] if isinstance(metric, str) else int(metric)
        c.metric_arg = metric_arg
        c.n_leaves = n_leaves
        c.kmeans_n_rows_train = kmeans_n_rows_train
        c.kmeans_n_iters = kmeans_n_iters
        c.partitioning_eta = partitioning_eta
        c.soar_lambda = soar_lambda
        c.pq_dim = pq_dim
        c.pq_bits = pq_bits
        c.pq_n_rows_train = pq_n_rows_train
        c.pq_train_iters = pq_train_iters
        c.reordering_bf16 = reordering_bf16
        c.reordering_noise_shaping_threshold = reordering_noise_shaping_threshold

    def __getattr__(self, name):
        if name != "_p" and name in {f[0] for f in _CParams._fields_}:
            return getattr(self._p.contents, name)
        raise AttributeError(name)

    def __del__(self):
        try:
            if self._p:
                lib().cuvsAmdScannIndexParamsDestroy(self._p)
        except Exception:
            pass


_HOST_DT = {(0, 16): np.int16, (1, 8): np.uint8}


class Index:
    def __init__(self):
        self._p = C.POINTER(_CIndex)()
        check(lib().cuvsAmdScannIndexCreate(C.byref(self._p)))
        self.trained = False
        self._device = "cuda"

    def __del__(self):
        try:
            if self._p:
                lib().cuvsAmdScannIndexDestroy(self._p)
        except Exception:
            pass

    def _int(self, fn):
        v = C.c_int64(0)
        check(getattr(lib(), fn)(self._p, C.byref(v)))
        return v.value

    def _device_view(self, fn):
        m = DLManagedTensor()
        check(getattr(lib(), fn)(self._p, C.byref(m)))
        return view_to_torch(m, self._device)

    def _host_view(self, fn):
        """a copy of a host array of the index"""
        m = DLManagedTensor()
        check(getattr(lib(), fn)(self._p, C.byref(m)))
        t = m.dl_tensor
        shape = tuple(t.shape[i] for i in range(t.ndim))
        dt = np.dtype(_HOST_DT[(t.dtype.code, t.dtype.bits)])
        n = int(np.prod(shape)) * dt.itemsize
        out = np.empty(shape, dt)
        if n:
            C.memmove(out.ctypes.data, t.data, n)
        if m.deleter:
            m.deleter(C.pointer(m))
        return out

    size = property(lambda self: self._int("cuvsAmdScannIndexGetSize"))
    dim = property(lambda self: self._int("cuvsAmdScannIndexGetDim"))
    n_leaves = property(lambda self: self._int("cuvsAmdScannIndexGetNLeaves"))
    pq_dim = property(lambda self: self._int("cuvsAmdScannIndexGetPqDim"))
    pq_bits = property(lambda self: self._int("cuvsAmdScannIndexGetPqBits"))
    centers = property(lambda self: self._device_view("cuvsAmdScannIndexGetCenters"))
    labels = property(lambda self: self._device_view("cuvsAmdScannIndexGetLabels"))
    soar_labels = property(lambda self: self._device_view("cuvsAmdScannIndexGetSoarLabels"))
    pq_codebook = property(lambda self: self._device_view("cuvsAmdScannIndexGetPqCodebook"))
    quantized_residuals = property(lambda self: self._host_view("cuvsAmdScannIndexGetCodes"))
    quantized_soar_residuals = property(lambda self: self._host_view("cuvsAmdScannIndexGetSoarCodes"))

    @property
    def has_bf16(self):
        v = C.c_bool(False)
        check(lib().cuvsAmdScannIndexHasBf16(self._p, C.byref(v)))
        return v.value

    @property
    def bf16_dataset(self):
        """int16 [n_rows, dim]: the bf16 bits of the rows (None without reordering_bf16)"""
        return self._host_view("cuvsAmdScannIndexGetBf16Dataset") if self.has_bf16 else None

    def __repr__(self):
        return "Index(type=ScaNN, size=%d, dim=%d, n_leaves=%d)" % (self.size, self.dim, self.n_leaves) if self.trained else "Index(type=ScaNN)"


@auto_sync_resources
def build(index_params, dataset, resources=None):
    """dataset: fp32 [n_rows, dim], a device tensor, a host tensor or a numpy array (handed over as it is: other types are refused)"""
    idx = Index()
    t = Tensor(dataset)
    check(lib().cuvsAmdScannBuild(resources.get_c_obj(), index_params._p, t.ptr, idx._p))
    if isinstance(dataset, torch.Tensor) and dataset.is_cuda:
        idx._device = dataset.device
    idx.trained = True
    return idx


@auto_sync_resources
def save(dirname, index, resources=None):
    """Writes the index files into the directory (created when missing)."""
    os.makedirs(dirname, exist_ok=True)
    check(lib().cuvsAmdScannSerialize(resources.get_c_obj(), os.fsencode(dirname), index._p))


def _u32(t):
    w = Tensor(t)
    w.m.dl_tensor.dtype.code = 1  # int32 storage, uint32 values
    return w


@auto_sync_resources
def avq_centers(dataset, labels, centers, eta=1.0, resources=None):
    """The AVQ centres of the leaves, in place in `centers` (fp32 [n_leaves, dim] holding the k-means centres); returns it."""
    tx, tl, tc = Tensor(dataset), _u32(labels), Tensor(centers)
    check(lib().cuvsAmdScannAvqCenters(resources.get_c_obj(), tx.ptr, tl.ptr, tc.ptr, C.c_float(eta)))
    return centers


@auto_sync_resources
def soar_labels(dataset, centers, labels, soar_lambda=1.0, out=None, resources=None):
    """The SOAR (spilled) leaf of every row: int32 [n_rows] on the device."""
    if out is None:
        out = torch.empty(dataset.shape[0], dtype=torch.int32, device=dataset.device)
    tx, tc, tl, to = Tensor(dataset), Tensor(centers), _u32(labels), _u32(out)
    check(lib().cuvsAmdScannSoarLabels(resources.get_c_obj(), tx.ptr, tc.ptr, tl.ptr, C.c_float(soar_lambda), to.ptr))
    return out


@auto_sync_resources
def quantize_bf16(dataset, threshold=float("nan"), out=None, resources=None):
    """The bf16 bits of the rows as int16 [n_rows, dim] on the device: round to nearest even, or AVQ noise shaping of the rows
    with |x| > threshold."""
    if out is None:
        out = torch.empty(tuple(dataset.shape), dtype=torch.int16, device=dataset.device)
    tx, to = Tensor(dataset), Tensor(out)
    check(lib().cuvsAmdScannQuantizeBf16(resources.get_c_obj(), tx.ptr, C.c_float(threshold), to.ptr))
    return out
