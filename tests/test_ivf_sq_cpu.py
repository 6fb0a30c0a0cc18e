"""CPU: IVF-SQ's C ABI (struct layouts, defaults, exported symbols, the reference's C driver) and self-checks of the numpy
restatement tests/ivf_sq_ref.py (exact fp32 fma, roundf ties, container round trip)."""
import ctypes as C
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from tests import ivf_sq_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "cuvs_amd", "libcuvs_c.so")
GOLDEN = os.path.join(ROOT, "tests", "golden")


def test_struct_layouts_match_the_reference_headers(tmp_path):
    # tests/golden/ivf_sq_abi_layout.txt: the same probe compiled against the reference's c/include (gen_ivf_sq_abi_layout.sh)
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(GOLDEN, "ivf_sq_abi_probe.c"), "-o", str(exe)])
    assert subprocess.check_output([str(exe)]).decode() == open(os.path.join(GOLDEN, "ivf_sq_abi_layout.txt")).read()


def test_symbols_exported_and_defaults_match_the_reference():
    from cuvs_amd.neighbors import ivf_sq

    lib = C.CDLL(LIB)
    for s in ("cuvsIvfSqBuild", "cuvsIvfSqSearch", "cuvsIvfSqExtend", "cuvsIvfSqSerialize", "cuvsIvfSqDeserialize",
              "cuvsIvfSqIndexGetSize", "cuvsIvfSqIndexGetCenters"):
        assert hasattr(lib, s), s
    p = C.POINTER(ivf_sq._CIndexParams)()
    assert lib.cuvsIvfSqIndexParamsCreate(C.byref(p)) == 1
    v = p.contents
    # c/src/neighbors/ivf_sq.cpp: cuvsIvfSqIndexParamsCreate
    assert (v.metric, v.metric_arg, v.add_data_on_build, v.n_lists, v.kmeans_n_iters, v.max_train_points_per_cluster,
            v.conservative_memory_allocation) == (0, 2.0, True, 1024, 20, 256, False)
    assert lib.cuvsIvfSqIndexParamsDestroy(p) == 1
    sp = C.POINTER(ivf_sq._CSearchParams)()
    assert lib.cuvsIvfSqSearchParamsCreate(C.byref(sp)) == 1
    assert sp.contents.n_probes == 20
    assert lib.cuvsIvfSqSearchParamsDestroy(sp) == 1
    idx = C.POINTER(ivf_sq._CIndex)()
    assert lib.cuvsIvfSqIndexCreate(C.byref(idx)) == 1
    n = C.c_int64(0)
    assert lib.cuvsIvfSqIndexGetNLists(idx, C.byref(n)) == 0  # not built: CUVS_ERROR
    assert lib.cuvsIvfSqIndexDestroy(idx) == 1


def test_reference_c_driver_compiles_and_links(tmp_path):
    """The reference's IVF-SQ C driver compiles unchanged against include/ and links against libcuvs_c.so."""
    src = "/root/reference/c/tests/neighbors/run_ivf_sq_c.c"
    if not os.path.exists(src):
        pytest.skip("no reference tree on this machine")
    so = tmp_path / "driver.so"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror=implicit-function-declaration", "-fPIC", "-shared", "-I",
                           os.path.join(ROOT, "include"), src, "-o", str(so), "-L", os.path.dirname(LIB), "-lcuvs_c",
                           "-Wl,--no-undefined", "-Wl,-rpath," + os.path.dirname(LIB)])
    C.CDLL(str(so))


# ---------------------------------------------------------------------------------------------- restatement self-checks
def _exact_fmaf(a, b, c):
    """correctly rounded fp32 fma through exact rationals (round to nearest, ties to even)"""
    x = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    f = np.float32(float(x))
    best = None
    for cand in (np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))):
        err = abs(Fraction(float(cand)) - x)
        even = (int(np.asarray(cand).view(np.uint32)) & 1) == 0
        if best is None or err < best[0] or (err == best[0] and even):
            best = (err, cand)
    return best[1]


def test_fmaf_is_exact_where_double_rounding_is_not():
    a = np.float32(2.0 ** -12 * (1 + 2.0 ** -18))
    b = np.float32(2.0 ** -12 * (1 - 2.0 ** -18))
    c = np.float32(1 + 2.0 ** -23)
    naive = np.float32(np.float64(a) * np.float64(b) + np.float64(c))
    want = _exact_fmaf(a, b, c)
    assert naive != want  # the plain f64 add-then-round double-rounds here
    assert S.fmaf(a, b, c) == want
    assert S.fmaf(-a, b, -c) == -want
    rng = np.random.default_rng(7)
    for _ in range(3000):
        a, b, c = (np.float32(v) for v in rng.standard_normal(3) * (2.0 ** rng.integers(-20, 20, 3)))
        assert S.fmaf(a, b, c) == _exact_fmaf(a, b, c), (a, b, c)
    # vectorised over arrays with broadcasting
    av = rng.standard_normal(64).astype(np.float32)
    assert np.array_equal(S.fmaf(av, np.float32(3.0), av[::-1]), np.array([_exact_fmaf(x, np.float32(3.0), y) for x, y in zip(av, av[::-1])]))


def test_roundf_rounds_half_away_from_zero():
    x = np.array([0.5, 1.5, 2.5, -0.5, -2.5, 0.49999997, 254.5, 255.49998], np.float32)
    assert S.roundf(x).tolist() == [1.0, 2.0, 3.0, -1.0, -3.0, 0.0, 255.0, 255.0]
    codes = S.encode(np.array([[0.0, 10.0, -5.0]], np.float32), np.zeros(3, np.float32), np.zeros(3, np.float32),
                     np.ones(3, np.float32) * np.float32(0.04))
    assert codes.tolist() == [[0, 250, 0]]


def test_container_round_trip(tmp_path):
    rng = np.random.default_rng(3)
    n_lists, dim = 5, 37
    centers = rng.standard_normal((n_lists, dim)).astype(np.float32)
    vmin = rng.standard_normal(dim).astype(np.float32)
    delta = rng.random(dim).astype(np.float32) + np.float32(0.01)
    sizes = [0, 1, 33, 64, 70]
    codes = [rng.integers(0, 256, (s, dim), dtype=np.uint8) for s in sizes]
    ids = [rng.integers(0, 1 << 40, s).astype(np.int64) for s in sizes]
    norms = rng.random(n_lists).astype(np.float32)
    p = str(tmp_path / "sq.bin")
    S.write_file(p, centers, vmin, delta, codes, ids, metric=2, center_norms=norms)
    back = S.parse_file(p)
    assert (back["version"], back["size"], back["dim"], back["n_lists"], back["metric"]) == (1, sum(sizes), dim, n_lists, 2)
    for name, v in (("centers", centers), ("center_norms", norms), ("vmin", vmin), ("delta", delta)):
        assert np.array_equal(back[name], v), name
    assert back["list_sizes"].tolist() == sizes
    for L in range(n_lists):
        assert np.array_equal(back["codes"][L], codes[L]) and np.array_equal(back["ids"][L], ids[L])
    # the 32-row x 16-byte interleave: row r, dim d of a group sits at (d // 16) * 512 + r * 16 + d % 16
    rec = S._interleave(codes[4], 96, 48)
    assert rec.reshape(-1)[1 * 512 + 5 * 16 + 3] == codes[4][5, 19]
    assert rec.reshape(-1)[32 * 48 + 2 * 512 + 1 * 16 + 4] == codes[4][33, 36]
