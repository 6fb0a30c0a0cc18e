"""numpy restatement of the scalar quantizer (cpp/src/preprocessing/quantize/detail/scalar.cuh), used by the tests as the
expected codes, reconstructions and trained [min, max].

  * min and max are rounded to the data's dtype T first; scale = 255 / ((double)max - (double)min) (1 when max <= min) and
    offset = -128 - (double)min * scale are doubles.
  * code(x) = -128 when not (min < x), else 127 when not (x < max) (so NaN gives -128), else
    lroundf((float)(scale * (double)x + offset)): the double is rounded to float before it is rounded half away from zero.
  * inverse(q) = (T)(((double)q - offset) / scale), one rounding from double to T.
  * train: all elements of the sampled rows sorted; pos_max = ceil((0.5 + 0.5 q) * size) - 1, pos_min = size - pos_max - 1,
    q the float32 quantile widened to double."""
import math

import numpy as np


def scale_offset(dtype, mn, mx):
    tmin, tmax = np.dtype(dtype).type(mn), np.dtype(dtype).type(mx)
    scale = 255.0 / (float(tmax) - float(tmin)) if float(tmax) > float(tmin) else 1.0
    return tmin, tmax, scale, -128.0 - float(tmin) * scale


def transform(x, mn, mx):
    x = np.asarray(x)
    tmin, tmax, scale, offset = scale_offset(x.dtype, mn, mx)
    with np.errstate(invalid="ignore", over="ignore"):
        v = (scale * x.astype(np.float64) + offset).astype(np.float32).astype(np.float64)
        r = np.sign(v) * np.floor(np.abs(v) + 0.5)  # round half away from zero (exact: |v| < 2^24)
        r = np.where(np.isfinite(r), r, 0.0)
        out = np.clip(r, -128, 127).astype(np.int8)
        out = np.where(~(x < tmax), np.int8(127), out)
        out = np.where(~(tmin < x), np.int8(-128), out)
    return out.astype(np.int8)


def inverse_transform(q, mn, mx, dtype):
    _, _, scale, offset = scale_offset(dtype, mn, mx)
    return ((np.asarray(q).astype(np.float64) - offset) / scale).astype(dtype)


def positions(size, quantile):
    pos_max = math.ceil((0.5 + 0.5 * float(np.float32(quantile))) * size) - 1
    return size - pos_max - 1, pos_max


def train_full(x, quantile):
    """[min, max] when every row is sampled (n_rows <= 1000000 // dim): a pure order statistic"""
    s = np.sort(np.asarray(x).ravel())
    pos_min, pos_max = positions(s.size, quantile)
    return float(s[pos_min]), float(s[pos_max])


def n_sampled_rows(n_rows, dim):
    return min(1000000 // dim, n_rows)
