"""numpy restatement of the binary quantizer (cpp/src/preprocessing/quantize/detail/binary.cuh, host rules), used by the
GPU tests as the expected thresholds and codes.

  * codes: bit j of byte b is x[8b + j] > threshold[8b + j] (threshold 0 for "zero"), i.e.
    np.packbits(x > thr, axis=1, bitorder="little"); fp16 compares in fp32; NaN gives 0; bytes past ceil(dim / 8) are 0.
  * "mean": the column mean (the GPU accumulates in fp64 for fp32 / fp64 rows, fp32 for fp16) rounded to the input dtype.
  * "sampling_median" (binary.cuh:292-324): ns = max(ceil(floor(n * ratio) / 2) * 2, 2) - 1 samples, n * ratio in fp32;
    stride = the first of 611323, 611333, 611389, 611393 that does not divide n; sample i is row (i * stride) % n; the
    threshold is element (ns - 1) / 2 of each sorted sample column - a value of the data, so it is restated exactly."""
import numpy as np

PRIMES = (611323, 611333, 611389, 611393)


def cmp_dtype(dtype):
    return np.float64 if np.dtype(dtype) == np.float64 else np.float32


def median_sample(n, ratio):
    """(ns, stride, rows) of the sampling-median rule"""
    scaled = int(np.float32(n) * np.float32(ratio))
    ns = max((scaled + 1) // 2 * 2, 2) - 1
    stride = next(p for p in PRIMES if n % p != 0)
    rows = (np.arange(ns, dtype=np.int64) * stride) % n
    return ns, stride, rows


def thresholds(x, kind, ratio=0.1):
    """expected thresholds of x [n, dim] (None for "zero"; "mean" as float64, before the rounding to x.dtype)"""
    if kind == "zero":
        return None
    if kind == "mean":
        return x.astype(np.float64).mean(axis=0)
    ns, _, rows = median_sample(x.shape[0], ratio)
    s = np.sort(x[rows].astype(cmp_dtype(x.dtype)), axis=0)
    return s[(ns - 1) // 2].astype(x.dtype)


def transform(x, thr=None, out_cols=None):
    """expected codes [n, out_cols] uint8 of x with thresholds thr (None: zero)"""
    c = cmp_dtype(x.dtype)
    t = np.zeros(x.shape[1], c) if thr is None else np.asarray(thr).astype(c)
    bits = x.astype(c) > t[None, :]
    codes = np.packbits(bits, axis=1, bitorder="little")
    if out_cols is not None and out_cols > codes.shape[1]:
        codes = np.concatenate([codes, np.zeros((x.shape[0], out_cols - codes.shape[1]), np.uint8)], axis=1)
    return codes


def hamming(a, b):
    """popcount distances between the uint8 rows of a [m, d] and b [n, d] -> [m, n] int64"""
    x = np.bitwise_xor(a[:, None, :], b[None, :, :])
    return np.unpackbits(x, axis=2).sum(axis=2, dtype=np.int64)
