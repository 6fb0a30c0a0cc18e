"""The scalar quantizer's host path through the C ABI with a null handle (host tensors need no device), and the rows the
scalar tests share. Used by tests/test_pq_scalar_quantizer_cpu.py and tests/test_scalar_quantizer_gpu.py."""
import ctypes as C

import numpy as np


def _c(lib_, fn, *args):
    r = getattr(lib_, fn)(*args)
    assert r == 1, lib_.cuvsGetLastErrorText()
    return r


def host_quantizer(mn, mx):
    from cuvs_amd.preprocessing.quantize import scalar

    q = scalar.Quantizer()
    q._p.contents.min_, q._p.contents.max_ = mn, mx
    return q


def host_transform(q, x):
    from cuvs_amd._lib import Tensor, lib

    out = np.full(x.shape, 77, np.int8)
    _c(lib(), "cuvsScalarQuantizerTransform", C.c_size_t(0), q._p, Tensor(x).ptr, Tensor(out).ptr)
    return out


def host_inverse(q, codes, dtype):
    from cuvs_amd._lib import Tensor, lib

    out = np.zeros(codes.shape, dtype)
    _c(lib(), "cuvsScalarQuantizerInverseTransform", C.c_size_t(0), q._p, Tensor(codes).ptr, Tensor(out).ptr)
    return out


def host_train(x, quantile):
    from cuvs_amd._lib import Tensor, lib
    from cuvs_amd.preprocessing.quantize import scalar

    q, params = scalar.Quantizer(), scalar.QuantizerParams(quantile=quantile)
    _c(lib(), "cuvsScalarQuantizerTrain", C.c_size_t(0), params._p, Tensor(x).ptr, q._p)
    return q


def special_rows(dtype, mn, mx, rng):
    """rows holding min, max, the values one ulp either side of both, +-inf and NaN, among uniform values"""
    t = np.dtype(dtype).type
    x = rng.uniform(float(mn) - 0.2, float(mx) + 0.2, (8, 37)).astype(dtype)
    sp = [t(mn), t(mx), np.nextafter(t(mn), t(-np.inf)), np.nextafter(t(mn), t(np.inf)), np.nextafter(t(mx), t(-np.inf)),
          np.nextafter(t(mx), t(np.inf)), t(np.inf), t(-np.inf), t(np.nan), t(0)]
    x[0, : len(sp)] = sp
    x[5, -len(sp):] = sp
    return x
