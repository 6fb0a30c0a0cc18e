"""CPU: the C ABI of the product and scalar quantizers (exported symbols, struct layouts against the reference's headers,
parameter defaults, getters on an unbuilt quantizer) and the scalar quantizer's host path, bit for bit against the numpy
restatement tests/scalar_quantizer_ref.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import scalar_quantizer_ref as S
from tests.scalar_quantizer_host import host_inverse, host_quantizer, host_train, host_transform, special_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "cuvs_amd", "libcuvs_c.so")
GOLDEN = os.path.join(ROOT, "tests", "golden")
HEADERS = [os.path.join(ROOT, "include", "cuvs", "preprocessing", "quantize", h) for h in ("pq.h", "scalar.h")]


def _prototypes():
    names = []
    for h in HEADERS:
        names += re.findall(r"CUVS_EXPORT\s+cuvsError_t\s+(\w+)\s*\(", open(h).read())
    return names


def test_every_prototype_is_exported():
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB]).decode()
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    protos = _prototypes()
    assert len(protos) == 13 + 7
    for s in protos + ["cuvsAmdProductQuantizerFromCodebooks", "cuvsAmdPqEncodeCounters"]:
        assert s in names, s


def test_struct_layouts_match_the_reference_headers(tmp_path):
    # tests/golden/pq_scalar_quantizer_abi_layout.txt: the same probe compiled against the reference's c/include
    # (gen_pq_scalar_quantizer_abi_layout.sh)
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(GOLDEN, "pq_scalar_quantizer_abi_probe.c"),
                           "-o", str(exe)])
    assert subprocess.check_output([str(exe)]).decode() == open(os.path.join(GOLDEN, "pq_scalar_quantizer_abi_layout.txt")).read()


def test_umbrella_header_includes_both_quantizers(tmp_path):
    body = ("#include <cuvs/core/all.h>\nint main(void) { struct cuvsProductQuantizerParams p = {8, 0, true, false, 0, 25,"
            " CUVS_KMEANS_TYPE_KMEANS_BALANCED, 256, 1024}; cuvsScalarQuantizer q = {0.0, 1.0};"
            " return (int)p.pq_bits - 8 + (int)q.min_; }\n")
    (tmp_path / "all.c").write_text(body)
    (tmp_path / "all.cpp").write_text(body)
    inc = os.path.join(ROOT, "include")
    subprocess.check_call(["gcc", "-std=c99", "-I", inc, "-c", str(tmp_path / "all.c"), "-o", str(tmp_path / "c.o")])
    subprocess.check_call(["g++", "-std=c++17", "-I", inc, "-c", str(tmp_path / "all.cpp"), "-o", str(tmp_path / "cpp.o")])


def test_params_defaults_match_the_reference():
    from cuvs_amd.preprocessing.quantize import pq, scalar

    lib = C.CDLL(LIB)
    p = C.POINTER(pq._CParams)()
    assert lib.cuvsProductQuantizerParamsCreate(C.byref(p)) == 1
    c = p.contents  # c/src/preprocessing/quantize/pq.cpp cuvsProductQuantizerParamsCreate
    assert (c.pq_bits, c.pq_dim, c.use_subspaces, c.use_vq, c.vq_n_centers, c.kmeans_n_iters, c.pq_kmeans_type,
            c.max_train_points_per_pq_code, c.max_train_points_per_vq_cluster) == (8, 0, True, False, 0, 25, 1, 256, 1024)
    assert lib.cuvsProductQuantizerParamsDestroy(p) == 1
    s = C.POINTER(scalar._CParams)()
    assert lib.cuvsScalarQuantizerParamsCreate(C.byref(s)) == 1
    assert s.contents.quantile == np.float32(0.99)  # scalar.cpp:127
    assert lib.cuvsScalarQuantizerParamsDestroy(s) == 1
    qp = pq.QuantizerParams()
    assert (qp.pq_bits, qp.pq_dim, qp.use_subspaces, qp.use_vq, qp.pq_kmeans_type) == (8, 0, True, False, "kmeans_balanced")
    assert np.float32(scalar.QuantizerParams().quantile) == np.float32(0.99)


def test_getters_on_an_unbuilt_quantizer_fail_with_a_message():
    from cuvs_amd._lib import DLManagedTensor
    from cuvs_amd.preprocessing.quantize import pq

    lib = C.CDLL(LIB)
    lib.cuvsGetLastErrorText.restype = C.c_char_p
    q = C.POINTER(pq._CQuantizer)()
    assert lib.cuvsProductQuantizerCreate(C.byref(q)) == 1
    assert q.contents.addr == 0
    u, b, m = C.c_uint32(), C.c_bool(), DLManagedTensor()
    for fn, arg in (("GetPqBits", u), ("GetPqDim", u), ("GetEncodedDim", u), ("GetUseVq", b), ("GetPqCodebook", m),
                    ("GetVqCodebook", m)):
        assert getattr(lib, "cuvsProductQuantizer" + fn)(q, C.byref(arg)) == 0, fn
        assert b"not built" in lib.cuvsGetLastErrorText(), fn
    assert lib.cuvsProductQuantizerDestroy(q) == 1


# ---------------------------------------------------------------------------------------------- scalar host path
@pytest.mark.parametrize("dtype", [np.float16, np.float32, np.float64])
@pytest.mark.parametrize("quantile", [1.0, 0.99, 0.5])
def test_scalar_host_path_bit_for_bit(dtype, quantile):
    rng = np.random.default_rng(3)
    data = rng.normal(0, 1, (300, 37)).astype(dtype)
    q = host_train(data, quantile)
    assert (q.min, q.max) == S.train_full(data, quantile)  # fully sampled: exactly sorted[pos_min], sorted[pos_max]
    x = special_rows(dtype, q.min, q.max, rng)
    codes = host_transform(q, x)
    assert np.array_equal(codes, S.transform(x, q.min, q.max))
    assert codes[0, 0] == -128 and codes[0, 1] == 127 and codes[0, 8] == -128  # min, max, NaN
    all_codes = np.arange(-128, 128, dtype=np.int8).reshape(4, 64)
    back = host_inverse(q, all_codes, dtype)
    assert np.array_equal(back.view(np.uint8), S.inverse_transform(all_codes, q.min, q.max, dtype).view(np.uint8))


@pytest.mark.parametrize("dtype", [np.float16, np.float32, np.float64])
def test_scalar_host_path_max_equals_min(dtype):
    rng = np.random.default_rng(4)
    q = host_quantizer(0.25, 0.25)
    x = special_rows(dtype, 0.25, 0.25, rng)
    assert np.array_equal(host_transform(q, x), S.transform(x, 0.25, 0.25))
    codes = np.arange(-128, 128, dtype=np.int8).reshape(4, 64)
    assert np.array_equal(host_inverse(q, codes, dtype).view(np.uint8), S.inverse_transform(codes, 0.25, 0.25, dtype).view(np.uint8))


def test_scalar_rounding_goes_through_float():
    # scale * x + offset = 0.5 - 2^-30 in double rounds to 0.5f and then away from zero to 1; rounding the double would give 0
    mn, mx = 0.0, 255.0  # scale 1, offset -128
    x = np.array([[128.5 - 2.0 ** -30, 128.5, 127.5, 129.49]], np.float64)
    q = host_quantizer(mn, mx)
    assert host_transform(q, x).tolist() == [[1, 1, -1, 1]] == S.transform(x, mn, mx).tolist()


def test_scalar_refusals():
    from cuvs_amd._lib import Tensor, lib

    q = host_quantizer(0.0, 1.0)
    x = np.zeros((4, 6), np.float32)
    L = lib()
    assert L.cuvsScalarQuantizerTransform(C.c_size_t(0), q._p, Tensor(x).ptr, Tensor(np.zeros((4, 6), np.uint8)).ptr) == 0
    assert L.cuvsScalarQuantizerTransform(C.c_size_t(0), q._p, Tensor(x).ptr, Tensor(np.zeros((4, 5), np.int8)).ptr) == 0
    assert L.cuvsScalarQuantizerTransform(C.c_size_t(0), q._p, Tensor(x[:, ::2]).ptr, Tensor(np.zeros((4, 3), np.int8)).ptr) == 0
    assert L.cuvsScalarQuantizerTransform(C.c_size_t(0), q._p, Tensor(x.astype(np.int32)).ptr, Tensor(np.zeros((4, 6), np.int8)).ptr) == 0
    from cuvs_amd.preprocessing.quantize import scalar

    for bad in (0.0, 1.5, -1.0):
        params = scalar.QuantizerParams(quantile=bad)
        assert L.cuvsScalarQuantizerTrain(C.c_size_t(0), params._p, Tensor(x).ptr, q._p) == 0
        assert b"quantile" in L.cuvsGetLastErrorText()


@pytest.mark.parametrize("dtype", [np.float32, np.float16])
def test_scalar_host_subsampled_train(dtype):
    # 40000 x 64 host rows: 15625 rows (1,000,000 elements) are drawn on the host. min and max are elements of the data, the draw
    # is deterministic, and the share of ALL elements inside [min, max] is within five standard deviations of a sample quantile
    n, dim, q = 40000, 64, 0.99
    x = np.random.default_rng(8).normal(0, 1, (n, dim)).astype(dtype)
    quant = host_train(x, q)
    again = host_train(x, q)
    assert (quant.min, quant.max) == (again.min, again.max)
    mn, mx = np.dtype(dtype).type(quant.min), np.dtype(dtype).type(quant.max)
    assert float(mn) == quant.min and float(mx) == quant.max and (x == mn).any() and (x == mx).any()
    assert (quant.min, quant.max) != S.train_full(x, q)  # (not the order statistic of all rows: rows were drawn)
    inside = float(((x >= mn) & (x <= mx)).mean())
    n_sampled = S.n_sampled_rows(n, dim) * dim
    assert n_sampled == 1000000
    assert abs(inside - q) <= 5.0 * np.sqrt(q * (1 - q) / n_sampled)


def test_python_layer_needs_no_device_for_host_rows():
    from cuvs_amd.preprocessing.quantize import scalar

    x = np.random.default_rng(9).random((200, 10)).astype(np.float32)
    q = scalar.train(scalar.QuantizerParams(quantile=0.99), x)
    assert (q.min, q.max) == S.train_full(x, 0.99)
    codes = scalar.transform(q, x)
    assert np.array_equal(codes, S.transform(x, q.min, q.max))
    back = scalar.inverse_transform(q, codes)
    assert np.array_equal(back.view(np.uint8), S.inverse_transform(codes, q.min, q.max, np.float32).view(np.uint8))
