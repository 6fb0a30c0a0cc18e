"""CPU: the numpy twin of single-linkage clustering - Boruvka against Kruskal under the contract's edge order, the twin
against scipy, the reference's table rows - and the build checks: the C header, the C++ wrappers, the exported symbols and
the host-only helper under the sanitizers."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import single_linkage_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "linkage_tables.json")
EXPORTS = ["cuvsAmdSingleLinkage", "cuvsAmdBuildLinkage", "cuvsAmdBuildDendrogram", "cuvsAmdSingleLinkageLastStats",
           "cuvsAmdLinkageParamsCreate", "cuvsAmdLinkageParamsDestroy"]
L2SQRT = 1


def knn_ids(w, k):
    """ids of the k smallest weights of every row, the row itself first (any exact kNN serves the twin)"""
    n = w.shape[0]
    w = w.copy()
    w[np.arange(n), np.arange(n)] = -1.0
    return np.argsort(w, axis=1, kind="stable")[:, :k]


@pytest.mark.parametrize("make", [R.uniform, R.lattice, R.duplicated])
@pytest.mark.parametrize("n,dim", [(2, 1), (3, 3), (127, 16), (129, 3), (257, 1), (257, 16)])
def test_boruvka_equals_kruskal(make, n, dim):
    x = make(n, dim, 100 * n + dim)
    w = R.weights(x, 0)
    assert (w == w.T).all(), "the chain is symmetric by construction"
    sk, dk, bk = R.kruskal(w)
    sb, db, bb, stats = R.boruvka(w)
    assert len(sk) == n - 1
    assert (sk == sb).all() and (dk == db).all() and (bk == bb).all()
    assert 1 <= stats["dense_rounds"] <= int(np.ceil(np.log2(n))) + 1
    if make is not R.uniform and n > 100:
        iu = np.triu_indices(n, 1)
        assert len(np.unique(R.bits(w)[iu])) < len(iu[0]) // 4, "the input is meant to have massive ties"
    # the kNN-graph linkage: the forest of the graph, then the complete graph over its components
    if n > 3:
        adj = R.adjacency(knn_ids(w, 3), n)
        sk, dk, bk = R.kruskal(w, adj)
        sb, db, bb, stats = R.boruvka(w, adj)
        assert (sk == sb).all() and (dk == db).all() and (bk == bb).all()
        assert stats["edges"] == adj.sum() // 2


def test_knn_graph_with_k_2_is_exact():
    x = R.uniform(200, 5, 3)
    w = R.weights(x, L2SQRT)
    adj = R.adjacency(knn_ids(w, 2), 200)
    exact = R.kruskal(w)
    graph = R.boruvka(w, adj)
    assert all((a == b).all() for a, b in zip(exact, graph[:3]))
    assert graph[3]["components"] > 1 and graph[3]["dense_rounds"] >= 1


@pytest.mark.parametrize("n,dim,seed", [(150, 7, 1), (257, 16, 2), (60, 1, 3)])
def test_pairwise_twin_against_scipy(n, dim, seed):
    from scipy.cluster.hierarchy import linkage

    x = R.uniform(n, dim, seed)
    src, dst, w, _ = R.linkage(x, L2SQRT)
    z = linkage(x.astype(np.float64), "single")
    err = np.abs(w.astype(np.float64) - z[:, 2]) / z[:, 2]
    print("largest relative error of the merge heights:", err.max())
    assert err.max() <= (dim + 2) * 2.0 ** -24
    assert len(np.unique(z[:, 2])) == n - 1 and len(np.unique(w)) == n - 1, "the comparison of the merges would be vacuous"
    children, delta, size = R.dendrogram(src, dst, w)
    assert (delta == w).all()
    assert (np.sort(children, axis=1) == np.sort(z[:, :2].astype(np.int64), axis=1)).all()
    assert (size == z[:, 3].astype(np.int64)).all()


@pytest.mark.parametrize("n_clusters", [2, 4])
def test_labels_against_fcluster(n_clusters):
    from scipy.cluster.hierarchy import fcluster, linkage

    x, _ = R.blobs(4, 40, 6, 11)
    src, dst, w, _ = R.linkage(x, L2SQRT)
    children, _, _ = R.dendrogram(src, dst, w)
    z = linkage(x.astype(np.float64), "single")
    n = len(x)
    below, above = z[n - 1 - n_clusters, 2], z[n - n_clusters, 2]  # the last merge kept and the first merge cut
    assert (above - below) / above > 1e-3, "the cut would depend on rounding"
    ours = R.flat_labels(children, n, n_clusters)
    assert len(np.unique(ours)) == n_clusters
    assert R.same_partition(ours, fcluster(z, n_clusters, "maxclust"))


def test_reference_tables():
    rows = json.load(open(TABLE))["rows"]
    assert len(rows) == 8 and sum(r["use_knn"] for r in rows) == 4
    for r in rows:
        n = r["n_row"]
        x = np.asarray(r["data"], np.float32).reshape(n, r["n_col"])
        ids = None
        if r["use_knn"]:
            k = R.build_k(n, r["c"])
            assert k == 2, "at k = 2 the kNN-graph linkage is exact"
            ids = knn_ids(R.weights(x, L2SQRT), k)
        src, dst, w, _ = R.linkage(x, L2SQRT, ids)
        children, _, _ = R.dendrogram(src, dst, w)
        labels = R.flat_labels(children, n, r["n_clusters"])
        assert R.rand_index(labels, r["expected_labels"]) == 1.0, (n, r["n_clusters"], r["use_knn"])


def test_dendrogram_and_labels_on_hand_made_trees():
    # a chain merged from the far end
    children, delta, size = R.dendrogram([3, 2, 1, 0], [4, 3, 2, 1], [1, 2, 3, 4])
    assert children.tolist() == [[3, 4], [2, 5], [1, 6], [0, 7]] and size.tolist() == [2, 3, 4, 5]
    assert R.flat_labels(children, 5, 1).tolist() == [0, 0, 0, 0, 0]
    assert R.flat_labels(children, 5, 2).tolist() == [1, 0, 0, 0, 0]  # roots 7 and 0 get labels 0 and 1
    assert R.flat_labels(children, 5, 5).tolist() == [4, 3, 2, 1, 0]
    # a star around row 2
    children, _, size = R.dendrogram([2, 2, 2], [0, 1, 3], [1, 1, 5])
    assert children.tolist() == [[2, 0], [4, 1], [5, 3]] and size.tolist() == [2, 3, 4]
    assert R.flat_labels(children, 4, 2).tolist() == [0, 0, 0, 1]  # roots 5 and 3
    assert R.flat_labels(children, 4, 4).tolist() == [3, 2, 1, 0]
    # two pairs joined last
    children, _, _ = R.dendrogram([0, 2, 1], [1, 3, 2], [1, 2, 9])
    assert children.tolist() == [[0, 1], [2, 3], [4, 5]]
    assert R.flat_labels(children, 4, 2).tolist() == [1, 1, 0, 0]
    assert R.flat_labels(children, 4, 3).tolist() == [0, 0, 2, 1]  # roots 4, 3, 2


def test_mutual_reachability_weight():
    x = R.uniform(50, 4, 5)
    d = R.weights(x, L2SQRT)
    core = np.sort(d, axis=1)[:, 4]
    w = R.weights(x, L2SQRT, core, 0.7)
    expect = np.maximum(np.maximum(core[:, None], core[None, :]), (np.float32(0.7) * d).astype(np.float32))
    assert (w == expect).all() and (w == w.T).all()
    sk, dk, bk = R.kruskal(w)
    sb, db, bb, _ = R.boruvka(w)
    assert (sk == sb).all() and (dk == db).all() and (bk == bb).all()
    assert len(np.unique(bk)) < len(bk), "core distances make ties: the order decides"


def test_header_is_c99_and_symbols_are_exported(tmp_path):
    src = tmp_path / "c.c"
    src.write_text('#include <cuvs_amd/single_linkage.h>\nint main(void) { struct cuvsAmdLinkageParams p; (void)p; return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])
    from cuvs_amd._lib import lib

    assert all(hasattr(lib(), s) for s in EXPORTS)
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "cuvs_amd", "libcuvs_c.so")], text=True)
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(EXPORTS) <= names
    header = open(os.path.join(ROOT, "include", "cuvs_amd", "single_linkage.h")).read()
    assert all(s + "(" in header for s in EXPORTS)


def test_cpp_wrappers_compile(tmp_path):
    src = tmp_path / "w.cpp"
    src.write_text(
        "#include <cuvs_amd/cluster.hpp>\n"
        "namespace ag = cuvs::cluster::agglomerative;\n"
        "void f(const cuvs::resources& r, cuvs::device_matrix_view<const float> x, cuvs::device_matrix_view<int64_t> d64,\n"
        "       cuvs::device_matrix_view<int32_t> d32, int64_t* v64, int32_t* v32, float* w, cuvsAllNeighborsIndexParams_t an) {\n"
        "  ag::single_linkage(r, x, d64, v64, L2SqrtExpanded, 3);\n"
        "  ag::single_linkage(r, x, d32, v32, L2Expanded, 3, ag::PAIRWISE, 5);\n"
        "  ag::helpers::linkage_graph_params::distance_params dp;\n"
        "  dp.dist_linkage = ag::PAIRWISE;\n"
        "  ag::helpers::build_linkage(r, x, dp, L2SqrtExpanded, v64, v64, w, d64, w, v64);\n"
        "  ag::helpers::linkage_graph_params::mutual_reachability_params mp;\n"
        "  mp.min_samples = 7; mp.alpha = 0.5f; mp.all_neighbors_params = an;\n"
        "  ag::helpers::build_linkage(r, x, mp, L2SqrtExpanded, v32, v32, w, d32, w, v32, w);\n"
        "  ag::helpers::build_dendrogram(r, (const int32_t*)v32, (const int32_t*)v32, (const float*)w, 9, d32, w, v32);\n"
        "}\nint main() { return 0; }\n")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_host_helper_under_the_sanitizers(tmp_path):
    exe = tmp_path / "single_linkage_host_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-I", os.path.join(ROOT, "cuvs_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "single_linkage_host_test.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "single linkage host OK" in out.stdout


def test_python_module_is_importable():
    from cuvs_amd.cluster import agglomerative

    assert all(hasattr(agglomerative, f) for f in ("single_linkage", "build_linkage", "build_dendrogram", "last_stats"))
