"""GPU: the scalar quantizer on device rows against its host path (byte for byte), the reference's Python check, and the
statistics of a subsampled Train."""
import numpy as np
import pytest
import torch

from cuvs_amd._lib import CuvsError
from cuvs_amd.preprocessing.quantize import scalar
from tests import scalar_quantizer_ref as S
from tests.scalar_quantizer_host import host_inverse, host_train, host_transform, special_rows

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype", [np.float16, np.float32, np.float64])
@pytest.mark.parametrize("shape", [(300, 37), (1, 1), (129, 1024), (1000, 333)])
def test_device_equals_host_byte_for_byte(dtype, shape):
    rng = np.random.default_rng(5)
    data = rng.normal(0, 1, shape).astype(dtype)
    qh = host_train(data, 0.99)
    qd = scalar.train(scalar.QuantizerParams(quantile=0.99), torch.from_numpy(data).cuda())
    assert (qd.min, qd.max) == (qh.min, qh.max) == S.train_full(data, 0.99)  # fully sampled: exact
    x = data.copy()
    if shape[1] >= 37:
        x[:8, :37] = special_rows(dtype, qh.min, qh.max, rng)
    want = host_transform(qh, x)
    got = scalar.transform(qd, torch.from_numpy(x).cuda())
    assert got.dtype == torch.int8 and np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(want, S.transform(x, qh.min, qh.max))
    # an unaligned view of device memory takes the element-wise path
    if x.size > 3:
        flat = torch.from_numpy(np.concatenate([np.zeros(1, dtype), x.ravel()])).cuda()[1:].view(shape)
        assert np.array_equal(scalar.transform(qd, flat).cpu().numpy(), want)
    back = scalar.inverse_transform(qd, got, dtype=dtype)
    assert np.array_equal(back.cpu().numpy().view(np.uint8), host_inverse(qh, want, dtype).view(np.uint8))


@pytest.mark.parametrize("n_rows", [50, 100])
@pytest.mark.parametrize("n_cols", [10, 50])
@pytest.mark.parametrize("inplace", [True, False])
@pytest.mark.parametrize("device_memory", [True, False])
@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.float16])
def test_reference_python_check(n_rows, n_cols, inplace, device_memory, dtype):
    # python/cuvs/cuvs/tests/test_scalar_quantizer.py
    input1 = np.random.default_rng(n_rows + n_cols).random((n_rows, n_cols)).astype(dtype)
    src = torch.from_numpy(input1).cuda() if device_memory else input1
    output = None
    if inplace:
        output = torch.zeros((n_rows, n_cols), dtype=torch.int8, device="cuda") if device_memory else np.zeros((n_rows, n_cols), np.int8)
    quantizer = scalar.train(scalar.QuantizerParams(quantile=0.99), src)
    transformed = scalar.transform(quantizer, src, output=output)
    actual = output if inplace else transformed
    actual = actual.cpu().numpy() if device_memory else actual
    start, end = quantizer.min, quantizer.max
    with np.errstate(invalid="ignore"):
        expected = np.int8(255 * (input1 - start) / (end - start) - 128)
    assert np.allclose(expected, actual, atol=2, rtol=2)


def test_subsampled_train_statistics():
    # 4M x 64 rows: 15625 rows = 1,000,000 elements are sampled. min and max are elements of the data; the share of ALL
    # elements inside [min, max] is the sample quantile's coverage, whose standard deviation is sqrt(q (1 - q) / n_sampled)
    n, dim, q = 4_000_000, 64, 0.99
    g = torch.Generator(device="cuda").manual_seed(7)
    x = torch.randn((n, dim), generator=g, device="cuda", dtype=torch.float32)
    quant = scalar.train(scalar.QuantizerParams(quantile=q), x)
    mn, mx = np.float32(quant.min), np.float32(quant.max)
    assert float(mn) == quant.min and float(mx) == quant.max
    assert bool((x == float(mn)).any()) and bool((x == float(mx)).any())
    inside = float(((x >= float(mn)) & (x <= float(mx))).sum().item()) / (n * dim)
    n_sampled = S.n_sampled_rows(n, dim) * dim
    bound = 5.0 * np.sqrt(q * (1 - q) / n_sampled)
    print(f"coverage {inside:.6f} vs {q}: |diff| {abs(inside - q):.2e}, allowed {bound:.2e}")
    assert abs(inside - q) <= bound


def test_subsampled_train_host_equals_device():
    # the same rows are drawn on the host and on the device (40000 x 64: 15625 of the rows)
    x = np.random.default_rng(8).normal(0, 1, (40000, 64)).astype(np.float32)
    qh = host_train(x, 0.99)
    qd = scalar.train(scalar.QuantizerParams(quantile=0.99), torch.from_numpy(x).cuda())
    assert (qd.min, qd.max) == (qh.min, qh.max)


def test_refusals():
    q = scalar.train(scalar.QuantizerParams(), torch.rand((64, 8), device="cuda"))
    x = torch.rand((64, 8), device="cuda")
    with pytest.raises(CuvsError):
        scalar.transform(q, x[:, ::2])  # non-contiguous
    with pytest.raises(CuvsError):
        scalar.transform(q, x, output=torch.zeros((64, 8), dtype=torch.uint8, device="cuda"))  # wrong dtype
    with pytest.raises(CuvsError):
        scalar.transform(q, x, output=torch.zeros((64, 7), dtype=torch.int8, device="cuda"))  # wrong shape
    with pytest.raises(CuvsError):
        scalar.transform(q, x, output=np.zeros((64, 8), np.int8))  # other kind of memory
    with pytest.raises(TypeError):
        scalar.transform(q, x.to(torch.int32))
    with pytest.raises(CuvsError):
        scalar.inverse_transform(q, torch.zeros((64, 8), dtype=torch.int8, device="cuda"),
                                 output=torch.zeros((63, 8), dtype=torch.float32, device="cuda"))
