"""Scalar quantizer (reference: python/cuvs/cuvs/preprocessing/quantize/scalar/scalar.pyx over
c/include/cuvs/preprocessing/quantize/scalar.h): fp16 / fp32 / fp64 rows <-> int8 codes over a trained [min, max]."""
import ctypes as C

import numpy as np
import torch

from ..._lib import Tensor, check, lib
from ...common import Resources

_DTYPES = (np.dtype("float32"), np.dtype("float64"), np.dtype("float16"))


class _CParams(C.Structure):
    _fields_ = [("quantile", C.c_float)]


class _CQuantizer(C.Structure):
    _fields_ = [("min_", C.c_double), ("max_", C.c_double)]


class QuantizerParams:
    """quantile: share of the sampled elements inside [min, max], centred; in (0, 1] (default 0.99)."""

    def __init__(self, *, quantile=0.99):
        self._p = C.POINTER(_CParams)()
        check(lib().cuvsScalarQuantizerParamsCreate(C.byref(self._p)))
        self._p.contents.quantile = quantile

    @property
    def quantile(self):
        return self._p.contents.quantile

    def __del__(self):
        try:
            lib().cuvsScalarQuantizerParamsDestroy(self._p)
        except Exception:
            pass


class Quantizer:
    """A trained scalar quantizer (cuvsScalarQuantizer: {min_, max_})."""

    def __init__(self):
        self._p = C.POINTER(_CQuantizer)()
        check(lib().cuvsScalarQuantizerCreate(C.byref(self._p)))

    min = property(lambda self: self._p.contents.min_)
    max = property(lambda self: self._p.contents.max_)

    def __del__(self):
        try:
            lib().cuvsScalarQuantizerDestroy(self._p)
        except Exception:
            pass


def _dtype_of(x):
    return np.dtype(str(x.dtype).replace("torch.", "")) if isinstance(x, torch.Tensor) else np.asarray(x).dtype


def _check_dataset(dataset):
    if _dtype_of(dataset) not in _DTYPES:
        raise TypeError(f"dataset dtype {_dtype_of(dataset)} is not one of float32, float64, float16")
    if len(dataset.shape) != 2:
        raise ValueError("dataset must be a 2-D matrix")


def _is_host(x):
    return not (isinstance(x, torch.Tensor) and x.is_cuda)


def _call(fn, resources, first, *args):
    """Host tensors are processed on the host: without a `resources` argument no device handle is made for them (the C entry
    points take 0). Device tensors get a handle and a sync, as auto_sync_resources does."""
    if resources is None and _is_host(first):
        check(fn(C.c_size_t(0), *args))
        return
    own = resources is None
    resources = Resources() if own else resources
    check(fn(resources.get_c_obj(), *args))
    if own:
        resources.sync()


def _empty_like(x, dtype):
    if isinstance(x, torch.Tensor):
        return torch.empty(tuple(x.shape), dtype=getattr(torch, str(np.dtype(dtype))), device=x.device)
    return np.empty(x.shape, dtype=dtype)


def train(params, dataset, resources=None):
    """cuvsScalarQuantizerTrain: [min, max] of `dataset` (host numpy / torch, or device torch; fp16, fp32 or fp64)."""
    _check_dataset(dataset)
    q = Quantizer()
    _call(lib().cuvsScalarQuantizerTrain, resources, dataset, params._p, Tensor(dataset).ptr, q._p)
    return q


def transform(quantizer, dataset, output=None, resources=None):
    """cuvsScalarQuantizerTransform: int8 [n, dim] in the kind of memory the dataset is in (allocated when not given)."""
    _check_dataset(dataset)
    if output is None:
        output = _empty_like(dataset, np.int8)
    _call(lib().cuvsScalarQuantizerTransform, resources, dataset, quantizer._p, Tensor(dataset).ptr, Tensor(output).ptr)
    return output


def inverse_transform(quantizer, dataset, output=None, resources=None, dtype=np.float32):
    """cuvsScalarQuantizerInverseTransform: int8 codes -> `output` (fp16 / fp32 / fp64; allocated as `dtype` when not given)."""
    if output is None:
        output = _empty_like(dataset, dtype)
    _call(lib().cuvsScalarQuantizerInverseTransform, resources, dataset, quantizer._p, Tensor(dataset).ptr, Tensor(output).ptr)
    return output
