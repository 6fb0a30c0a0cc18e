"""CPU: the numpy twin of the sparse (CSR) distances and of the sparse kNN against the reference's own test tables and against
scipy, the C header and the exported symbols, the C++ overloads, and the host-only helper under the sanitizers."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import sparse_distance_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "sparse_reference_table.json")
EXPORTS = ["cuvsAmdSparseCsrValidate", "cuvsAmdSparsePairwiseDistance", "cuvsAmdSparseBruteForceIndexCreate",
           "cuvsAmdSparseBruteForceIndexDestroy", "cuvsAmdSparseBruteForceBuild", "cuvsAmdSparseBruteForceSearch",
           "cuvsAmdSparseLastStats", "cuvsAmdSparseSetForm"]


def compare_approx(a, b, eps):
    """CompareApprox of the reference's tests (cpp/tests/test_utils.h:41-54), elementwise"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    with np.errstate(all="ignore"):
        diff = np.abs(a - b)
        m = np.maximum(np.abs(a), np.abs(b))
        ratio = np.where(diff > np.float32(eps), diff / m, diff)
    return ratio <= np.float32(eps)


def golden():
    return json.load(open(TABLE))


def golden_csr(row):
    return R.Csr(row["indptr"], row["indices"], row["data"], row["n_cols"])


def test_table_is_complete():
    t = golden()
    rows = t["sparse_distance"]["rows"]
    assert len(rows) == 20 and len(t["sparse_brute_force"]["rows"]) == 1
    assert {r["metric"] for r in rows} == {"CosineExpanded", "JaccardExpanded", "L2Expanded", "InnerProduct", "L2Unexpanded", "Canberra",
                                           "LpUnexpanded", "Linf", "HellingerExpanded", "L1", "CorrelationExpanded",
                                           "RusselRaoExpanded", "HammingUnexpanded", "JensenShannon", "DiceExpanded"}
    for r in rows:
        n = len(r["indptr"]) - 1
        assert len(r["expected"]) == n * n and r["lines"] and R.is_canonical(golden_csr(r)), r["lines"]
        assert r["metric_id"] in R.SUPPORTED


@pytest.mark.parametrize("i", range(20))
def test_twin_meets_the_reference_distance_rows(i):
    r = golden()["sparse_distance"]["rows"][i]
    x = golden_csr(r)
    got = R.pairwise(x, x, r["metric_id"], r["metric_arg"])
    want = np.asarray(r["expected"], np.float32).reshape(x.rows, x.rows)
    ok = compare_approx(want, got, 1e-3)
    assert ok.all(), (r["lines"], r["metric"], got[~ok], want[~ok])


def test_twin_meets_the_reference_knn_row():
    r = golden()["sparse_brute_force"]["rows"][0]
    x = golden_csr(r)
    assert R.is_canonical(x) and (x.data == 0).sum() == 2  # the table's rows hold stored zeros
    ids, d = R.knn(x, x, r["k"], r["metric_id"])
    assert (ids.ravel() == np.asarray(r["expected_indices"])).all()
    assert compare_approx(np.asarray(r["expected_distances"], np.float32), d.ravel(), 1e-4).all()


SCIPY = {R.L2Expanded: "sqeuclidean", R.L2SqrtExpanded: "euclidean", R.CosineExpanded: "cosine", R.L1: "cityblock",
         R.L2Unexpanded: "sqeuclidean", R.L2SqrtUnexpanded: "euclidean", R.Linf: "chebyshev", R.Canberra: "canberra",
         R.LpUnexpanded: "minkowski", R.CorrelationExpanded: "correlation", R.JensenShannon: "jensenshannon"}
SCIPY_BINARY = {R.JaccardExpanded: "jaccard", R.DiceExpanded: "dice", R.HammingUnexpanded: "hamming", R.RusselRaoExpanded: "russellrao"}


@pytest.fixture(scope="module")
def small():
    rng = np.random.default_rng(11)
    x = R.random_csr(rng, 23, 40, 0.3, stored_zeros=5)
    y = R.random_csr(rng, 31, 40, 0.3, stored_zeros=5)
    xb = R.random_csr(rng, 23, 40, 0.3, binary=True)
    yb = R.random_csr(rng, 31, 40, 0.3, binary=True)
    return x, y, xb, yb


@pytest.mark.parametrize("metric", sorted(SCIPY) + sorted(SCIPY_BINARY) + [R.InnerProduct, R.HellingerExpanded, R.KLDivergence])
def test_twin_against_scipy(small, metric):
    from scipy.spatial.distance import cdist

    x, y, xb, yb = small
    if metric in SCIPY_BINARY:
        x, y = xb, yb
    dx, dy = x.dense(np.float64), y.dense(np.float64)
    got = R.pairwise(x, y, metric, 3.0, diagonal=False)
    got64, _, _ = R.pairwise64(x, y, metric, 3.0, diagonal=False)
    if metric in SCIPY:
        kw = {"p": 3.0} if metric == R.LpUnexpanded else {}
        if metric == R.JensenShannon:  # scipy normalises the rows to sum 1; the reference does not
            dx, dy = dx / dx.sum(axis=1, keepdims=True), dy / dy.sum(axis=1, keepdims=True)
            x, y = R.Csr.from_dense(dx), R.Csr.from_dense(dy)
            got = R.pairwise(x, y, metric, diagonal=False)
        want = cdist(dx, dy, SCIPY[metric], **kw)
    elif metric in SCIPY_BINARY:
        want = cdist(dx != 0, dy != 0, SCIPY_BINARY[metric])
    elif metric == R.InnerProduct:
        want = dx @ dy.T
    elif metric == R.HellingerExpanded:
        want = np.sqrt(np.maximum(1 - np.sqrt(dx) @ np.sqrt(dy).T, 0))
    else:  # KL over the shared columns
        with np.errstate(all="ignore"):
            t = dx[:, None, :] * np.log(dx[:, None, :] / dy[None, :, :])
        want = 0.5 * np.where((dx[:, None, :] != 0) & (dy[None, :, :] != 0), t, 0).sum(axis=2)
    scale = np.maximum(np.abs(want), 1)
    assert (np.abs(got - want) <= 2e-4 * scale).all(), np.abs(got - want).max()
    if metric != R.JensenShannon:
        assert (np.abs(got64 - want) <= 2e-4 * scale).all()


def test_twin_split_rule_and_row_statistics():
    rng = np.random.default_rng(5)
    x = R.random_csr(rng, 6, 64, 0.4)
    y = R.random_csr(rng, 5, 64, 0.1, full_rows=(1,), long_rows=((3, 17),))
    short = np.flatnonzero(np.diff(y.indptr) <= 16)
    assert sorted(set(range(5)) - set(short.tolist())) == [1, 3]
    # an unsplit chain and one cut after every 16 stored entries: the same sets, another order of additions
    for metric in (R.InnerProduct, R.L1, R.Linf, R.HammingUnexpanded):
        whole, _ = R.chains(x, y, metric)
        cut, _ = R.chains(x, y, metric, split=16)
        assert (whole[:, short] == cut[:, short]).all()  # short rows are one piece
        assert np.allclose(whole, cut, rtol=1e-5)
        if metric in (R.Linf, R.HammingUnexpanded):
            assert (whole == cut).all()  # max and counts do not depend on the cut
    whole, _ = R.chains(x, y, R.InnerProduct)
    cut, _ = R.chains(x, y, R.InnerProduct, split=16)
    assert (whole[:, [1, 3]] != cut[:, [1, 3]]).any()
    assert sorted(R.split_boundaries(y, 16)) == sorted({15: [1], 31: [1], 47: [1], int(y.indices[y.indptr[3] + 15]): [3]})
    sq, sm, ones = R.row_stats(y)
    d = y.dense(np.float64)
    assert np.allclose(sq, (d * d).sum(axis=1), rtol=1e-5) and np.allclose(sm, d.sum(axis=1), rtol=1e-5)
    assert (ones == (y.dense() == 1).sum(axis=1)).all()


def test_header_is_c99_and_symbols_are_exported(tmp_path):
    src = tmp_path / "c.c"
    src.write_text('#include <cuvs_amd/sparse.h>\nint main(void) { return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])
    from cuvs_amd._lib import lib

    assert all(hasattr(lib(), s) for s in EXPORTS)
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "cuvs_amd", "libcuvs_c.so")], text=True)
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(EXPORTS) <= names


def test_cpp_overloads_compile(tmp_path):
    src = tmp_path / "w.cpp"
    src.write_text(
        "#include <cuvs_amd/neighbors.hpp>\n"
        "namespace bf = cuvs::neighbors::brute_force;\n"
        "void f(const cuvs::resources& r, const cuvs::csr_view& x, cuvs::device_matrix_view<float> out,\n"
        "       cuvs::device_matrix_view<int64_t> i64, cuvs::device_matrix_view<int32_t> i32) {\n"
        "  cuvs::distance::pairwise_distance(r, x, x, out, CosineExpanded);\n"
        "  cuvs::distance::pairwise_distance(r, x, x, out, LpUnexpanded, 1.5f);\n"
        "  bf::sparse_index idx = bf::build(r, x, L2SqrtExpanded);\n"
        "  bf::sparse_search_params p;\n"
        "  static_assert(sizeof(p.batch_size_index) == 4, \"\");\n"
        "  bf::search(r, p, idx, x, i64, out);\n"
        "  bf::search(r, p, idx, x, i32, out);\n"
        "}\nint main() { return bf::sparse_search_params().batch_size_query == 32768 ? 0 : 1; }\n")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_host_helper_under_the_sanitizers(tmp_path):
    exe = tmp_path / "sparse_distance_host_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-I", os.path.join(ROOT, "cuvs_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "sparse_distance_host_test.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "sparse distance host OK" in out.stdout


def test_host_constants_match_the_twin():
    text = open(os.path.join(ROOT, "cuvs_amd", "csrc", "sparse_distance_host.hpp")).read()
    assert "constexpr int kSplit   = %d;" % R.SPLIT in text
    from tests import test_sparse_distance_gpu as G

    for name, value in (("kRangeI ", G.RANGE_I), ("kRangeU ", G.RANGE_U)):
        assert "constexpr int %s = %d;" % (name, value) in text, name


def test_twin_counts_the_terms_of_a_chain():
    x = R.Csr([0, 3, 3], [0, 2, 5], [1.0, 0.0, 2.0], 6)  # a stored zero is no entry
    y = R.Csr([0, 2, 4], [2, 5, 0, 1], [1.0, 1.0, 3.0, 4.0], 6)
    count = np.zeros((2, 2), np.int64)
    R.chains(x, y, R.InnerProduct, count=count)
    assert count.tolist() == [[1, 1], [0, 0]]
    count[:] = 0
    R.chains(x, y, R.L1, count=count)
    assert count.tolist() == [[3, 3], [2, 2]]
