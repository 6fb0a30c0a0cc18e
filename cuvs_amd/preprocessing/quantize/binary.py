"""Binary quantizer (reference: python/cuvs/cuvs/preprocessing/quantize/binary/binary.pyx over
c/include/cuvs/preprocessing/quantize/binary.h): float rows -> uint8 codes, bit j of byte b set when x[8b + j] >
threshold[8b + j]; the codes are what CAGRA and NN-descent search with metric="bitwise_hamming"."""
import ctypes as C

import numpy as np
import torch

from ..._lib import DLDataType, Tensor, check, lib
from ...common import auto_sync_resources

_THRESHOLDS = {"zero": 0, "mean": 1, "sampling_median": 2}
_DTYPES = (np.dtype("float32"), np.dtype("float64"), np.dtype("float16"))


class _CParams(C.Structure):
    _fields_ = [("threshold", C.c_int), ("sampling_ratio", C.c_float)]


class _CQuantizer(C.Structure):
    _fields_ = [("addr", C.c_size_t), ("dtype", DLDataType)]


class QuantizerParams:
    """threshold: "zero", "mean" (default) or "sampling_median"; sampling_ratio: share of the rows the median is taken
    over, in (0, 1] (default 0.1)."""

    def __init__(self, *, threshold="mean", sampling_ratio=0.1):
        if threshold not in _THRESHOLDS:
            raise ValueError(f"threshold must be one of {sorted(_THRESHOLDS)}, got {threshold!r}")
        self._p = C.POINTER(_CParams)()
        check(lib().cuvsBinaryQuantizerParamsCreate(C.byref(self._p)))
        self._p.contents.threshold = _THRESHOLDS[threshold]
        self._p.contents.sampling_ratio = sampling_ratio
        self.threshold = threshold

    @property
    def sampling_ratio(self):
        return self._p.contents.sampling_ratio

    def __del__(self):
        try:
            lib().cuvsBinaryQuantizerParamsDestroy(self._p)
        except Exception:
            pass


class Quantizer:
    """A trained binary quantizer (cuvsBinaryQuantizer)."""

    def __init__(self):
        self._p = C.POINTER(_CQuantizer)()
        check(lib().cuvsBinaryQuantizerCreate(C.byref(self._p)))
        self.dim = 0
        self.dtype = None
        self.trained = False

    def __del__(self):
        try:
            lib().cuvsBinaryQuantizerDestroy(self._p)
        except Exception:
            pass

    @property
    def threshold(self):
        """The thresholds [dim] in the training dtype, on the device (empty for "zero")."""
        from ...common import Resources

        out = torch.empty((self.dim,), dtype=getattr(torch, str(self.dtype)), device="cuda")
        res = Resources()
        check(lib().cuvsAmdBinaryQuantizerGetThreshold(res.get_c_obj(), self._p, Tensor(out).ptr))
        res.sync()
        return out


def _dtype_of(x):
    return np.dtype(str(x.dtype).replace("torch.", "")) if isinstance(x, torch.Tensor) else np.asarray(x).dtype


def _check_dataset(dataset):
    if _dtype_of(dataset) not in _DTYPES:
        raise TypeError(f"dataset dtype {_dtype_of(dataset)} is not one of float32, float64, float16")
    if len(dataset.shape) != 2:
        raise ValueError("dataset must be a 2-D matrix")


@auto_sync_resources
def train(quantizer_params, dataset, resources=None):
    """cuvsBinaryQuantizerTrain: thresholds of `dataset` (host numpy / torch, or device torch; fp16, fp32 or fp64)."""
    _check_dataset(dataset)
    q = Quantizer()
    check(lib().cuvsBinaryQuantizerTrain(resources.get_c_obj(), quantizer_params._p, Tensor(dataset).ptr, q._p))
    q.dim = 0 if quantizer_params.threshold == "zero" else int(dataset.shape[1])
    q.dtype = _dtype_of(dataset)
    q.trained = True
    return q


@auto_sync_resources
def transform(dataset, output=None, quantizer=None, resources=None):
    """cuvsBinaryQuantizerTransform (quantizer None: threshold zero) or cuvsBinaryQuantizerTransformWithParams. The codes
    are uint8 [n, >= ceil(dim / 8)] in the kind of memory the dataset is in; a missing `output` is allocated there."""
    _check_dataset(dataset)
    if output is None:
        cols = (int(dataset.shape[1]) + 7) // 8
        if isinstance(dataset, torch.Tensor):
            output = torch.empty((dataset.shape[0], cols), dtype=torch.uint8, device=dataset.device)
        else:
            output = np.empty((dataset.shape[0], cols), dtype=np.uint8)
    td, to = Tensor(dataset), Tensor(output)
    if quantizer is None:
        check(lib().cuvsBinaryQuantizerTransform(resources.get_c_obj(), td.ptr, to.ptr))
    else:
        check(lib().cuvsBinaryQuantizerTransformWithParams(resources.get_c_obj(), quantizer._p, td.ptr, to.ptr))
    return output
