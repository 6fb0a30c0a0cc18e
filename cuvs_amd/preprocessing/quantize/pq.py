"""Product quantizer (reference: python/cuvs/cuvs/preprocessing/quantize/pq/pq.pyx over
c/include/cuvs/preprocessing/quantize/pq.h): fp32 rows -> pq_dim codes of pq_bits bits per row (code j in bits
[j * pq_bits, (j + 1) * pq_bits) of the row's bytes), optionally on the residual to a VQ centre."""
import ctypes as C

import numpy as np
import torch

from ..._lib import DLDataType, DLManagedTensor, Tensor, check, lib, view_to_torch
from ...common import auto_sync_resources

_KMEANS_TYPES = {"kmeans": 0, "kmeans_balanced": 1}


class _CParams(C.Structure):
    _fields_ = [("pq_bits", C.c_uint32), ("pq_dim", C.c_uint32), ("use_subspaces", C.c_bool), ("use_vq", C.c_bool),
                ("vq_n_centers", C.c_uint32), ("kmeans_n_iters", C.c_uint32), ("pq_kmeans_type", C.c_int),
                ("max_train_points_per_pq_code", C.c_uint32), ("max_train_points_per_vq_cluster", C.c_uint32)]


class _CQuantizer(C.Structure):
    _fields_ = [("addr", C.c_size_t), ("dtype", DLDataType)]


class QuantizerParams:
    """pq_bits in [4, 16] (8); pq_dim codes per row (0: ceil(dim / 4)); use_subspaces: a codebook per piece (True);
    use_vq: quantize the residual to a k-means centre (False); vq_n_centers (0: sqrt(n_rows) rounded up to a multiple of 8);
    kmeans_n_iters (25); pq_kmeans_type "kmeans_balanced" (default) or "kmeans"; max_train_points_per_pq_code (256);
    max_train_points_per_vq_cluster (1024)."""

    def __init__(self, *, pq_bits=8, pq_dim=0, use_subspaces=True, use_vq=False, vq_n_centers=0, kmeans_n_iters=25,
                 pq_kmeans_type="kmeans_balanced", max_train_points_per_pq_code=256, max_train_points_per_vq_cluster=1024):
        if pq_kmeans_type not in _KMEANS_TYPES:
            raise ValueError(f"pq_kmeans_type must be one of {sorted(_KMEANS_TYPES)}, got {pq_kmeans_type!r}")
        self._p = C.POINTER(_CParams)()
        check(lib().cuvsProductQuantizerParamsCreate(C.byref(self._p)))
        p = self._p.contents
        p.pq_bits, p.pq_dim, p.use_subspaces, p.use_vq = pq_bits, pq_dim, use_subspaces, use_vq
        p.vq_n_centers, p.kmeans_n_iters = vq_n_centers, kmeans_n_iters
        p.pq_kmeans_type = _KMEANS_TYPES[pq_kmeans_type]
        p.max_train_points_per_pq_code = max_train_points_per_pq_code
        p.max_train_points_per_vq_cluster = max_train_points_per_vq_cluster

    def __getattr__(self, name):
        if name in {f[0] for f in _CParams._fields_}:
            v = getattr(self._p.contents, name)
            return {0: "kmeans", 1: "kmeans_balanced"}[v] if name == "pq_kmeans_type" else v
        raise AttributeError(name)

    def __del__(self):
        try:
            lib().cuvsProductQuantizerParamsDestroy(self._p)
        except Exception:
            pass


class Quantizer:
    """A built product quantizer (cuvsProductQuantizer)."""

    def __init__(self):
        self._p = C.POINTER(_CQuantizer)()
        check(lib().cuvsProductQuantizerCreate(C.byref(self._p)))

    def __del__(self):
        try:
            lib().cuvsProductQuantizerDestroy(self._p)
        except Exception:
            pass

    def _scalar(self, fn, ctype):
        v = ctype()
        check(getattr(lib(), fn)(self._p, C.byref(v)))
        return v.value

    def _tensor(self, fn):
        m = DLManagedTensor()
        check(getattr(lib(), fn)(self._p, C.byref(m)))
        return view_to_torch(m, "cuda")

    pq_bits = property(lambda self: self._scalar("cuvsProductQuantizerGetPqBits", C.c_uint32))
    pq_dim = property(lambda self: self._scalar("cuvsProductQuantizerGetPqDim", C.c_uint32))
    encoded_dim = property(lambda self: self._scalar("cuvsProductQuantizerGetEncodedDim", C.c_uint32))
    use_vq = property(lambda self: self._scalar("cuvsProductQuantizerGetUseVq", C.c_bool))
    pq_codebook = property(lambda self: self._tensor("cuvsProductQuantizerGetPqCodebook"),
                           doc="fp32 [pq_dim * 2^pq_bits, pq_len] (use_subspaces) or [2^pq_bits, pq_len], a device copy")
    vq_codebook = property(lambda self: self._tensor("cuvsProductQuantizerGetVqCodebook"),
                           doc="fp32 [vq_n_centers, dim], empty without VQ, a device copy")


def _check_dataset(dataset):
    dt = np.dtype(str(dataset.dtype).replace("torch.", "")) if isinstance(dataset, torch.Tensor) else np.asarray(dataset).dtype
    if dt != np.dtype("float32"):
        raise TypeError(f"dataset dtype {dt} is not float32")
    if len(dataset.shape) != 2:
        raise ValueError("dataset must be a 2-D matrix")


@auto_sync_resources
def build(params, dataset, resources=None):
    """cuvsProductQuantizerBuild: trains the codebooks on `dataset` (fp32; host numpy / torch, or device torch)."""
    _check_dataset(dataset)
    q = Quantizer()
    check(lib().cuvsProductQuantizerBuild(resources.get_c_obj(), params._p, Tensor(dataset).ptr, q._p))
    return q


@auto_sync_resources
def from_codebooks(params, pq_codebook, vq_codebook=None, resources=None):
    """cuvsAmdProductQuantizerFromCodebooks: a quantizer over caller-supplied device codebooks (copied)."""
    q = Quantizer()
    vq = Tensor(vq_codebook) if vq_codebook is not None else None
    check(lib().cuvsAmdProductQuantizerFromCodebooks(resources.get_c_obj(), params._p, Tensor(pq_codebook).ptr,
                                                     vq.ptr if vq is not None else None, q._p))
    return q


@auto_sync_resources
def transform(quantizer, dataset, codes_output=None, vq_labels=None, resources=None):
    """cuvsProductQuantizerTransform -> (codes, vq_labels): codes uint8 [n, encoded_dim] and, with VQ, labels uint32 [n],
    both on the device (allocated when not given); vq_labels is None without VQ."""
    _check_dataset(dataset)
    n = int(dataset.shape[0])
    if codes_output is None:
        codes_output = torch.empty((n, quantizer.encoded_dim), dtype=torch.uint8, device="cuda")
    if quantizer.use_vq and vq_labels is None:
        vq_labels = torch.empty((n,), dtype=torch.uint32, device="cuda")
    tl = Tensor(vq_labels) if (quantizer.use_vq and vq_labels is not None) else None
    check(lib().cuvsProductQuantizerTransform(resources.get_c_obj(), quantizer._p, Tensor(dataset).ptr, Tensor(codes_output).ptr,
                                              tl.ptr if tl is not None else None))
    return codes_output, (vq_labels if quantizer.use_vq else None)


@auto_sync_resources
def inverse_transform(quantizer, codes, output=None, vq_labels=None, resources=None):
    """cuvsProductQuantizerInverseTransform: fp32 [n, dim] on the device from device codes (and labels, with VQ)."""
    if output is None:
        book = quantizer.pq_codebook
        output = torch.empty((int(codes.shape[0]), quantizer.pq_dim * int(book.shape[1])), dtype=torch.float32, device="cuda")
    tl = Tensor(vq_labels) if vq_labels is not None else None
    check(lib().cuvsProductQuantizerInverseTransform(resources.get_c_obj(), quantizer._p, Tensor(codes).ptr, Tensor(output).ptr,
                                                     tl.ptr if tl is not None else None))
    return output
