"""GPU: the binary quantizer (cuvsBinaryQuantizer*) against the numpy restatement tests/binary_quantizer_ref.py.

  * the reference's table (cpp/tests/preprocessing/binary_quantization.cu:125-131): {5, 100, 1000} rows x {7, 128, 1999}
    columns x {zero, mean, sampling_median} x {trained on host, device} x {f32, f64, f16}, data uniform [-1, 1). Host and
    device transforms are byte-identical and equal np.packbits(x > thr, bitorder="little") with the thresholds read back;
    median thresholds equal the restatement exactly, mean thresholds are within 1 ulp of T of the float64 mean, and host
    and device training give the same thresholds;
  * the reference Python test's cases (python/cuvs/cuvs/tests/test_binary_quantizer.py), strided rows, padded outputs;
  * every error path."""
import numpy as np
import pytest

from tests import binary_quantizer_ref as B

pytestmark = pytest.mark.gpu

DTYPES = {"f32": np.float32, "f64": np.float64, "f16": np.float16}


def _torch(x):
    import torch

    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _ulp(v, dtype):
    v = np.asarray(v, dtype)
    return np.abs(np.nextafter(v, np.asarray(np.inf, dtype)).astype(np.float64) - v.astype(np.float64))


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("train_on", ["host", "device"])
@pytest.mark.parametrize("threshold", ["zero", "mean", "sampling_median"])
@pytest.mark.parametrize("cols", [7, 128, 1999])
@pytest.mark.parametrize("rows", [5, 100, 1000])
def test_reference_table(rows, cols, threshold, train_on, dtype, res):
    from cuvs_amd.preprocessing.quantize import binary

    rng = np.random.default_rng(rows * 7919 + cols)
    x = rng.uniform(-1, 1, (rows, cols)).astype(DTYPES[dtype])
    xd = _torch(x)
    params = binary.QuantizerParams(threshold=threshold)
    q = binary.train(params, x if train_on == "host" else xd, resources=res)
    other = binary.train(params, xd if train_on == "host" else x, resources=res)
    thr = q.threshold.cpu().numpy()
    assert thr.dtype == x.dtype and thr.shape == ((0,) if threshold == "zero" else (cols,))
    assert np.array_equal(thr, other.threshold.cpu().numpy(), equal_nan=True)   # host and device rows: the same thresholds
    if threshold == "sampling_median":
        assert np.array_equal(thr, B.thresholds(x, "sampling_median", 0.1))
    elif threshold == "mean":
        m = B.thresholds(x, "mean")
        assert (np.abs(thr.astype(np.float64) - m) <= _ulp(m.astype(x.dtype), x.dtype)).all()
    dev = binary.transform(xd, quantizer=q, resources=res)
    res.sync()
    host = binary.transform(x, quantizer=q, resources=res)
    dev = dev.cpu().numpy()
    assert dev.shape == host.shape == (rows, (cols + 7) // 8) and dev.dtype == np.uint8
    assert np.array_equal(dev, host)
    assert np.array_equal(dev, B.transform(x, None if threshold == "zero" else thr))


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.float16])
@pytest.mark.parametrize("device_memory", [True, False])
@pytest.mark.parametrize("inplace", [True, False])
@pytest.mark.parametrize("n_cols", [10, 50])
@pytest.mark.parametrize("n_rows", [50, 100])
def test_reference_python_cases(n_rows, n_cols, inplace, device_memory, dtype, res):
    from cuvs_amd.preprocessing.quantize import binary

    x = np.random.default_rng(n_rows + n_cols).random((n_rows, n_cols)).astype(dtype)
    cols = int(np.ceil(n_cols / 8))
    out = np.zeros((n_rows, cols), np.uint8) if inplace else None
    if device_memory:
        out_d = _torch(out) if inplace else None
        got = binary.transform(_torch(x), output=out_d, resources=res)
        res.sync()
        actual = (out_d if inplace else got).cpu().numpy()
    else:
        got = binary.transform(x, output=out, resources=res)
        actual = out if inplace else got
    assert np.array_equal(actual, np.packbits(x > 0, axis=-1, bitorder="little"))


@pytest.mark.parametrize("device_memory", [True, False])
def test_strided_rows_padded_output_and_nan(device_memory, res):
    """rows with a stride, an output wider than ceil(dim / 8) (padding bytes written as 0; a row pitch that is not a multiple
    of 8 takes the byte stores), more output rows than input rows (left untouched), NaN -> 0, dims around 64"""
    from cuvs_amd.preprocessing.quantize import binary

    rng = np.random.default_rng(5)
    for dim in (1, 63, 64, 65, 200):
        base = rng.uniform(-1, 1, (33, dim + 9)).astype(np.float32)
        base[3, 0] = np.nan
        x = base[:, :dim]
        for extra in (0, 3, 8):
            cols = (dim + 7) // 8 + extra
            out = np.full((40, cols), 0xAB, np.uint8)
            q = binary.train(binary.QuantizerParams(threshold="mean"), x, resources=res)
            thr = q.threshold.cpu().numpy()
            if device_memory:
                od = _torch(out)
                binary.transform(_torch(base)[:, :dim], output=od, quantizer=q, resources=res)
                res.sync()
                got = od.cpu().numpy()
            else:
                got = out
                binary.transform(x, output=got, quantizer=q, resources=res)
            assert np.array_equal(got[:33], B.transform(x, thr, cols)), (dim, extra)
            assert (got[33:] == 0xAB).all()


def test_errors(res):
    import torch
    from cuvs_amd._lib import CuvsError
    from cuvs_amd.preprocessing.quantize import binary

    x = np.random.default_rng(0).uniform(-1, 1, (100, 20)).astype(np.float32)
    xd = _torch(x)
    for ratio in (0.0, -0.5, 1.5):
        with pytest.raises(CuvsError, match="sampling ratio"):
            binary.train(binary.QuantizerParams(threshold="sampling_median", sampling_ratio=ratio), xd, resources=res)
    q = binary.train(binary.QuantizerParams(), xd, resources=res)
    with pytest.raises(CuvsError, match="dimension must be larger"):
        binary.transform(xd, output=torch.empty((100, 2), dtype=torch.uint8, device="cuda"), quantizer=q, resources=res)
    with pytest.raises(CuvsError, match="size must be larger"):
        binary.transform(xd, output=torch.empty((99, 3), dtype=torch.uint8, device="cuda"), quantizer=q, resources=res)
    with pytest.raises(CuvsError, match="dtype differs"):
        binary.transform(xd.double(), quantizer=q, resources=res)
    with pytest.raises(CuvsError, match="differs from the threshold length"):
        binary.transform(xd[:, :16], quantizer=q, resources=res)
    with pytest.raises(CuvsError, match="same kind of memory"):
        binary.transform(xd, output=np.empty((100, 3), np.uint8), quantizer=q, resources=res)
    with pytest.raises(CuvsError, match="must be uint8"):
        binary.transform(xd, output=torch.empty((100, 3), dtype=torch.int32, device="cuda"), resources=res)
    with pytest.raises(CuvsError, match="at least one column"):
        binary.transform(np.empty((4, 0), np.float32), output=np.empty((4, 0), np.uint8), resources=res)
    with pytest.raises(CuvsError, match="at least one column"):
        binary.train(binary.QuantizerParams(), xd[:, :0], resources=res)
    with pytest.raises(TypeError):
        binary.train(binary.QuantizerParams(), xd.to(torch.int8), resources=res)
    with pytest.raises(ValueError):
        binary.QuantizerParams(threshold="median")


def test_mean_and_transform_over_several_row_chunks(res):
    """host rows are staged through the device in ~256 MB row chunks (MEAN training and transform alike); device rows are
    reduced in the same chunks, so the thresholds of host and device rows are equal here too"""
    from cuvs_amd.preprocessing.quantize import binary

    x = np.random.default_rng(11).uniform(-1, 1, (70000, 1024)).astype(np.float32)   # 287 MB: two chunks
    xd = _torch(x)
    qh = binary.train(binary.QuantizerParams(threshold="mean"), x, resources=res)
    qd = binary.train(binary.QuantizerParams(threshold="mean"), xd, resources=res)
    th, td = qh.threshold.cpu().numpy(), qd.threshold.cpu().numpy()
    assert np.array_equal(th, td)
    m = B.thresholds(x, "mean")
    assert (np.abs(th.astype(np.float64) - m) <= _ulp(m.astype(np.float32), np.float32)).all()
    host = binary.transform(x, quantizer=qh, resources=res)
    dev = binary.transform(xd, quantizer=qd, resources=res)
    res.sync()
    assert np.array_equal(host, dev.cpu().numpy())
    assert np.array_equal(host, B.transform(x, th))
