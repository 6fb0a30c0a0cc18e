"""CPU: the binary quantizer's C ABI (exported symbols, struct / enum layouts against the reference's header, parameter
defaults) and self-checks of the numpy restatement tests/binary_quantizer_ref.py."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests import binary_quantizer_ref as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "cuvs_amd", "libcuvs_c.so")
GOLDEN = os.path.join(ROOT, "tests", "golden")

SYMBOLS = ("cuvsBinaryQuantizerParamsCreate", "cuvsBinaryQuantizerParamsDestroy", "cuvsBinaryQuantizerCreate",
           "cuvsBinaryQuantizerDestroy", "cuvsBinaryQuantizerTrain", "cuvsBinaryQuantizerTransform",
           "cuvsBinaryQuantizerTransformWithParams", "cuvsAmdBinaryQuantizerGetThreshold", "cuvsAmdCagraBuildKnnGraph")


def test_symbols_exported():
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB]).decode()
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for s in SYMBOLS:
        assert s in names, s


def test_struct_layouts_match_the_reference_header(tmp_path):
    # tests/golden/binary_quantizer_abi_layout.txt: the same probe compiled against the reference's c/include
    # (gen_binary_quantizer_abi_layout.sh)
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(GOLDEN, "binary_quantizer_abi_probe.c"),
                           "-o", str(exe)])
    assert subprocess.check_output([str(exe)]).decode() == open(os.path.join(GOLDEN, "binary_quantizer_abi_layout.txt")).read()


def test_umbrella_header_includes_the_quantizer(tmp_path):
    src = tmp_path / "all.c"
    src.write_text("#include <cuvs/core/all.h>\nint main(void) { struct cuvsBinaryQuantizerParams p = {SAMPLING_MEDIAN, 0.5f};"
                   " return (int)p.threshold - 2; }\n")
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "all.o")])


def test_params_defaults_match_the_reference():
    from cuvs_amd.preprocessing.quantize import binary

    lib = C.CDLL(LIB)
    p = C.POINTER(binary._CParams)()
    assert lib.cuvsBinaryQuantizerParamsCreate(C.byref(p)) == 1
    assert (p.contents.threshold, p.contents.sampling_ratio) == (1, np.float32(0.1))  # binary.cpp:95-101: MEAN, 0.1
    assert lib.cuvsBinaryQuantizerParamsDestroy(p) == 1
    qp = binary.QuantizerParams()
    assert (qp.threshold, np.float32(qp.sampling_ratio)) == ("mean", np.float32(0.1))
    q = C.POINTER(binary._CQuantizer)()
    assert lib.cuvsBinaryQuantizerCreate(C.byref(q)) == 1
    assert q.contents.addr == 0
    assert lib.cuvsBinaryQuantizerDestroy(q) == 1


# ---------------------------------------------------------------------------------------------- restatement self-checks
def test_transform_matches_a_bit_loop():
    rng = np.random.default_rng(0)
    for dtype in (np.float32, np.float64, np.float16):
        for dim in (1, 7, 8, 9, 64, 65, 130):
            x = rng.uniform(-1, 1, (5, dim)).astype(dtype)
            thr = rng.uniform(-0.5, 0.5, dim).astype(dtype)
            x[0, 0] = np.nan
            out_cols = (dim + 7) // 8 + 2
            want = np.zeros((5, out_cols), np.uint8)
            for i in range(5):
                for j in range(dim):
                    if np.float64(x[i, j]) > np.float64(thr[j]):   # NaN compares false
                        want[i, j // 8] |= 1 << (j % 8)
            assert np.array_equal(B.transform(x, thr, out_cols), want)
            assert np.array_equal(B.transform(x, None), np.packbits(x > 0, axis=1, bitorder="little"))


def test_median_sample_rule():
    # ns is odd, at least 1 and at most n; the stride skips the primes that divide n
    for n, ratio in ((5, 0.1), (100, 0.1), (1000, 0.1), (1000, 1.0), (999, 1.0), (7, 0.5), (1, 1.0)):
        ns, stride, rows = B.median_sample(n, ratio)
        assert ns % 2 == 1 and 1 <= ns <= n and rows.max() < n
        assert stride == 611323
    assert B.median_sample(1000, 0.1)[0] == 99
    assert B.median_sample(611323 * 2, 0.1)[1] == 611333
    assert B.median_sample(611323 * 611333, 1e-9)[1] == 611389
    # the threshold is an element of its column: the ((ns - 1) / 2)-th of the sample
    rng = np.random.default_rng(1)
    x = rng.uniform(-1, 1, (1000, 13)).astype(np.float32)
    thr = B.thresholds(x, "sampling_median", 0.1)
    ns, _, rows = B.median_sample(1000, 0.1)
    for j in range(13):
        col = x[rows, j]
        assert thr[j] in x[:, j]
        assert (col < thr[j]).sum() == (ns - 1) // 2 == (col > thr[j]).sum()


def test_hamming_matches_popcount():
    rng = np.random.default_rng(2)
    a = rng.integers(0, 256, (4, 9), dtype=np.uint8)
    b = rng.integers(0, 256, (6, 9), dtype=np.uint8)
    want = np.array([[sum(bin(int(u) ^ int(v)).count("1") for u, v in zip(r, s)) for s in b] for r in a])
    assert np.array_equal(B.hamming(a, b), want)
