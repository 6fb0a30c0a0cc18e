"""GPU: single-linkage clustering against its numpy twin (tests/single_linkage_ref.py), bit for bit: the spanning tree in
the three linkages, the dendrogram, the flat labels, the statistics and the refusals."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

from tests import single_linkage_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "linkage_tables.json")
NAMES = {0: "sqeuclidean", 1: "euclidean", 4: "l2_unexpanded", 5: "l2_sqrt_unexpanded"}
MAKERS = {"uniform": R.uniform, "lattice": R.lattice, "duplicated": R.duplicated}


def agg():
    from cuvs_amd.cluster import agglomerative

    return agglomerative


def dev(x):
    return torch.from_numpy(np.array(x, order="C")).cuda()  # (a copy: the cached inputs are read-only)


def host(t):
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def pairwise_case(kind, n, dim, metric):
    x = MAKERS[kind](n, dim, 1000 * n + dim)
    x.setflags(write=False)
    src, dst, w, stats = R.linkage(x, metric)
    children, delta, size = R.dendrogram(src, dst, w)
    return x, src, dst, w, stats, children, delta, size


def assert_linkage(out, src, dst, w, children=None, delta=None, size=None):
    assert (host(out["mst_src"]) == src).all()
    assert (host(out["mst_dst"]) == dst).all()
    assert (R.bits(host(out["mst_weights"])) == R.bits(w)).all()
    if children is not None:
        assert (host(out["dendrogram"]) == children).all()
        assert (R.bits(host(out["out_distances"])) == R.bits(delta)).all()
        assert (host(out["out_sizes"]) == size).all()


# every n of the tile edges (127, 128, 129), one multi-tile grid (257, 300), the unaligned-load path (dim 1, 3, 7, 33), each
# metric once, the tie-heavy inputs once each
PAIRWISE_CASES = [
    ("uniform", 2, 1, 0), ("uniform", 3, 3, 1), ("uniform", 127, 7, 4), ("uniform", 128, 16, 5), ("uniform", 129, 33, 0),
    ("uniform", 257, 3, 1), ("uniform", 300, 16, 0), ("uniform", 300, 7, 1), ("lattice", 257, 3, 0), ("duplicated", 129, 16, 1),
]


@pytest.mark.parametrize("kind,n,dim,metric", PAIRWISE_CASES)
def test_pairwise_equals_the_twin(res, kind, n, dim, metric):
    x, src, dst, w, stats, children, delta, size = pairwise_case(kind, n, dim, metric)
    out = agg().build_linkage(dev(x), metric=NAMES[metric], linkage="pairwise", resources=res)
    res.sync()
    assert_linkage(out, src, dst, w, children, delta, size)
    assert out["core_dists"] is None
    st = agg().last_stats()
    side = (n + 127) // 128
    assert st == dict(k=0, graph_edges=0, sparse_rounds=0, components=n, dense_rounds=stats["dense_rounds"],
                      tiles=stats["dense_rounds"] * side * side)


def test_pairwise_rows_that_are_not_16_byte_aligned(res):
    x, src, dst, w, *_ = pairwise_case("uniform", 300, 16, 0)
    flat = torch.zeros(300 * 16 + 1, dtype=torch.float32, device="cuda")
    view = flat[1:].view(300, 16)
    view.copy_(dev(x))
    assert view.data_ptr() % 16 == 4
    out = agg().build_linkage(view, metric="sqeuclidean", linkage="pairwise", resources=res)
    res.sync()
    assert_linkage(out, src, dst, w)


def test_pairwise_more_tiles_than_workgroups(res):
    """841 pair tiles: the persistent workgroups take more than one tile each. The twin's Kruskal is too slow here: the
    device tree must span, carry the twin's weights, and have the weights of scipy's minimum spanning tree over them."""
    from scipy.sparse.csgraph import minimum_spanning_tree

    n = 3600
    x = R.uniform(n, 2, 77)
    out = agg().build_linkage(dev(x), metric="sqeuclidean", linkage="pairwise", outputs=dict(dendrogram=False, out_distances=False,
                                                                                                out_sizes=False), resources=res)
    res.sync()
    st = agg().last_stats()
    assert st["tiles"] == st["dense_rounds"] * 29 * 29 and 1 <= st["dense_rounds"] <= 13
    src, dst, wd = host(out["mst_src"]), host(out["mst_dst"]), host(out["mst_weights"])
    w = R.weights(x, 0)
    assert (w[np.triu_indices(n, 1)] > 0).all()
    assert (src < dst).all() and (R.bits(wd) == R.bits(w[src, dst])).all()
    assert (np.lexsort((dst, src, R.bits(wd))) == np.arange(n - 1)).all(), "the edges are not in key order"
    uf = R._UF(n)
    assert all(uf.union(int(a), int(b)) for a, b in zip(src, dst)), "the edges do not span"
    best = np.sort(minimum_spanning_tree(w.astype(np.float64)).data)
    assert (np.sort(wd.astype(np.float64)) == best).all()


def knn_ids(x, metric, k, res):
    """the documented call: the public brute-force search of X against itself"""
    from cuvs_amd.neighbors import brute_force

    xd = dev(x)
    _, ids = brute_force.search(brute_force.build(xd, metric=NAMES[metric], resources=res), xd, k, resources=res)
    res.sync()
    return host(ids)


def test_knn_graph_with_components_to_connect(res):
    x, _ = R.blobs(3, 40, 4, 5)
    n, c, metric = len(x), 2, 1
    k = R.build_k(n, c)
    assert k == 8 and k < 40
    src, dst, w, stats = R.linkage(x, metric, knn_ids(x, metric, k, res))
    children, delta, size = R.dendrogram(src, dst, w)
    out = agg().build_linkage(dev(x), metric=NAMES[metric], linkage="knn_graph", c=c, resources=res)
    res.sync()
    assert_linkage(out, src, dst, w, children, delta, size)
    st = agg().last_stats()
    assert st["components"] == 3 and st["dense_rounds"] >= 1, st
    assert st == dict(k=k, graph_edges=stats["edges"], sparse_rounds=stats["sparse_rounds"], components=stats["components"],
                      dense_rounds=stats["dense_rounds"], tiles=stats["dense_rounds"])
    # the same rows by the exact linkage: the blobs are joined by the same edges
    exact = R.linkage(x, metric)
    assert (exact[2][-2:] == w[-2:]).all()


def test_knn_graph_connected(res):
    x = R.uniform(200, 3, 9)
    k = R.build_k(200, 15)
    assert k == 22
    src, dst, w, stats = R.linkage(x, 0, knn_ids(x, 0, k, res))
    out = agg().build_linkage(dev(x), metric="sqeuclidean", linkage="knn_graph", c=15, dtype=torch.int32, resources=res)
    res.sync()
    assert out["mst_src"].dtype == torch.int32 and out["dendrogram"].dtype == torch.int32
    assert_linkage(out, src, dst, w, *R.dendrogram(src, dst, w))
    st = agg().last_stats()
    assert st["components"] == 1 and st["dense_rounds"] == 0 and st["tiles"] == 0 and st["sparse_rounds"] >= 1, st
    assert st["sparse_rounds"] == stats["sparse_rounds"] and st["graph_edges"] == stats["edges"]


@pytest.mark.parametrize("alpha,metric,explicit", [(1.0, 1, False), (0.7, 0, True)])
def test_mutual_reachability(res, alpha, metric, explicit):
    from cuvs_amd.neighbors import all_neighbors

    x, _ = R.blobs(2, 60, 5, 21, spread=0.5, gap=3.0)
    n, k = len(x), 6
    params = all_neighbors.AllNeighborsParams(algo="brute_force", metric=NAMES[metric])
    ids = torch.empty((n, k), dtype=torch.int64, device="cuda")
    dist = torch.empty((n, k), dtype=torch.float32, device="cuda")
    core = torch.empty(n, dtype=torch.float32, device="cuda")
    all_neighbors.build(dev(x), k, params, indices=ids, distances=dist, core_distances=core, alpha=alpha, resources=res)
    res.sync()
    src, dst, w, stats = R.linkage(x, metric, host(ids), host(core), alpha)
    out = agg().build_linkage(dev(x), metric=NAMES[metric], space="mutual_reachability", min_samples=k, alpha=alpha,
                              all_neighbors_params=params if explicit else None, resources=res)
    res.sync()
    assert (R.bits(host(out["core_dists"])) == R.bits(host(core))).all()
    assert_linkage(out, src, dst, w, *R.dendrogram(src, dst, w))
    st = agg().last_stats()
    assert st["k"] == k and st["graph_edges"] == stats["edges"] and st["components"] == stats["components"]
    assert (w >= host(core)[src]).all() and (w >= host(core)[dst]).all()


def test_labels_on_the_reference_tables(res):
    rows = json.load(open(TABLE))["rows"]
    assert len(rows) == 8
    for r in rows:
        n = r["n_row"]
        x = np.asarray(r["data"], np.float32).reshape(n, r["n_col"])
        ids = knn_ids(x, 1, R.build_k(n, r["c"]), res) if r["use_knn"] else None
        src, dst, w, _ = R.linkage(x, 1, ids)
        children, _, _ = R.dendrogram(src, dst, w)
        twin = R.flat_labels(children, n, r["n_clusters"])
        dend, labels = agg().single_linkage(dev(x), r["n_clusters"], metric="euclidean", linkage="knn_graph" if r["use_knn"] else "pairwise",
                                            c=r["c"], dtype=torch.int32, resources=res)
        res.sync()
        assert labels.dtype == torch.int32 and (host(dend) == children).all()
        assert (host(labels) == twin).all()
        assert R.rand_index(host(labels), r["expected_labels"]) == 1.0, (n, r["n_clusters"], r["use_knn"])


@pytest.mark.parametrize("n_clusters,dtype", [(1, torch.int64), (2, torch.int32), (4, torch.int64), (160, torch.int32)])
def test_labels_on_blobs(res, n_clusters, dtype):
    from scipy.cluster.hierarchy import fcluster, linkage

    x, _ = R.blobs(4, 40, 6, 11)
    n = len(x)
    src, dst, w, _ = R.linkage(x, 1)
    children, _, _ = R.dendrogram(src, dst, w)
    dend, labels = agg().single_linkage(dev(x), n_clusters, metric="euclidean", linkage="pairwise", dtype=dtype, resources=res)
    res.sync()
    assert labels.dtype == dtype and dend.dtype == dtype
    assert (host(dend) == children).all()
    assert (host(labels) == R.flat_labels(children, n, n_clusters)).all()
    if 1 < n_clusters < n:
        z = linkage(x.astype(np.float64), "single")
        assert (z[n - n_clusters, 2] - z[n - 1 - n_clusters, 2]) / z[n - n_clusters, 2] > 1e-3
        assert R.same_partition(host(labels), fcluster(z, n_clusters, "maxclust"))
    else:
        assert len(np.unique(host(labels))) == n_clusters


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_build_dendrogram_alone(res, dtype):
    rng = np.random.default_rng(4)
    n = 500
    src = np.array([rng.integers(0, i) for i in range(1, n)])
    dst = np.arange(1, n)
    perm = rng.permutation(n - 1)
    src, dst = src[perm], dst[perm]
    w = np.sort(rng.random(n - 1, dtype=np.float32))
    children, delta, size = R.dendrogram(src, dst, w)
    got = agg().build_dendrogram(dev(src).to(dtype), dev(dst).to(dtype), dev(w), resources=res)
    res.sync()
    assert got[0].dtype == dtype and got[2].dtype == dtype
    assert (host(got[0]) == children).all() and (host(got[1]) == delta).all() and (host(got[2]) == size).all()
    assert size[-1] == n


def test_refusals(res):
    from cuvs_amd._lib import CuvsError

    a = agg()
    x = dev(R.uniform(20, 4, 1))

    def refused(match, fn, *args, **kw):
        with pytest.raises(CuvsError, match=match):
            fn(*args, resources=res, **kw)

    refused("must be fp32", a.single_linkage, x.half(), 2)
    refused("must be fp32", a.single_linkage, x.double(), 2)
    refused("device memory", a.single_linkage, x.cpu(), 2, dendrogram=torch.empty((19, 2), dtype=torch.int64, device="cuda"),
            labels=torch.empty(20, dtype=torch.int64, device="cuda"))
    refused("2-D", a.single_linkage, x.reshape(-1), 2, dendrogram=torch.empty((19, 2), dtype=torch.int64, device="cuda"),
            labels=torch.empty(20, dtype=torch.int64, device="cuda"))
    refused("contiguous", a.single_linkage, x.t(), 2)
    refused("n >= 2", a.single_linkage, x[:1], 1)
    refused(r"n_clusters must be in \[1, n\]", a.single_linkage, x, 0)
    refused(r"n_clusters must be in \[1, n\]", a.single_linkage, x, 21)
    refused("L2Expanded.*L2SqrtExpanded.*L2Unexpanded.*L2SqrtUnexpanded", a.single_linkage, x, 2, metric="cosine")
    refused("L2Expanded.*L2SqrtExpanded.*L2Unexpanded.*L2SqrtUnexpanded", a.build_linkage, x, metric="inner_product")
    refused("PAIRWISE", a.single_linkage, x, 2, linkage=7)
    refused("one type", a.single_linkage, x, 2, dendrogram=torch.empty((19, 2), dtype=torch.int32, device="cuda"))
    refused(r"labels must have shape \[20\]", a.single_linkage, x, 2, labels=torch.empty(21, dtype=torch.int64, device="cuda"))
    refused(r"dendrogram must have shape \[19, 2\]", a.single_linkage, x, 2, dendrogram=torch.empty((20, 2), dtype=torch.int64, device="cuda"))
    refused("int32 or int64", a.single_linkage, x, 2, labels=torch.empty(20, dtype=torch.float32, device="cuda"),
            dendrogram=torch.empty((19, 2), dtype=torch.float32, device="cuda"))
    refused(r"min_samples must be in \[2, n\]", a.build_linkage, x, space="mutual_reachability", min_samples=1)
    refused(r"min_samples must be in \[2, n\]", a.build_linkage, x, space="mutual_reachability", min_samples=21)
    refused("core_dists must not be NULL", a.build_linkage, x, space="mutual_reachability", outputs=dict(core_dists=False))
    refused("core_dists must be NULL", a.build_linkage, x, outputs=dict(core_dists=torch.empty(20, device="cuda")))
    refused("mst_weights must be fp32", a.build_linkage, x, outputs=dict(mst_weights=torch.empty(19, dtype=torch.float64, device="cuda")))
    refused("MUTUAL_REACHABILITY", a.build_linkage, x, space=5)
    refused("cols must have shape", a.build_dendrogram, torch.zeros(5, dtype=torch.int64, device="cuda"),
            torch.zeros(4, dtype=torch.int64, device="cuda"), torch.zeros(5, device="cuda"))
    refused("closes a cycle", a.build_dendrogram, torch.zeros(2, dtype=torch.int64, device="cuda"),
            torch.ones(2, dtype=torch.int64, device="cuda"), torch.zeros(2, device="cuda"))
    # the library still works after the refusals
    out = a.build_linkage(x, metric="sqeuclidean", linkage="pairwise", resources=res)
    res.sync()
    assert_linkage(out, *R.linkage(host(x), 0)[:3])


def test_stats_vector():
    from cuvs_amd._lib import lib

    out = (C.c_uint64 * 8)(*([12345] * 8))
    assert lib().cuvsAmdSingleLinkageLastStats(out) == 1
    assert out[6] == 12345 and out[7] == 12345, "six values are written"
    assert list(agg().last_stats()) == ["k", "graph_edges", "sparse_rounds", "components", "dense_rounds", "tiles"]
    assert lib().cuvsAmdSingleLinkageLastStats(None) == 0


def test_second_call_on_the_handle_with_another_shape(res):
    big = pairwise_case("uniform", 300, 16, 0)
    small = pairwise_case("uniform", 127, 7, 4)
    for x, src, dst, w, *_ in (big, small, big):
        out = agg().build_linkage(dev(x), metric=NAMES[0 if x.shape[0] == 300 else 4], linkage="pairwise", resources=res)
        res.sync()
        assert_linkage(out, src, dst, w)
    x, _ = R.blobs(3, 40, 4, 5)
    first = agg().build_linkage(dev(x), metric="euclidean", linkage="knn_graph", c=2, resources=res)
    again = agg().build_linkage(dev(x), metric="euclidean", linkage="knn_graph", c=2, resources=res)
    res.sync()
    assert all((host(first[k]) == host(again[k])).all() for k in ("mst_src", "mst_dst", "mst_weights", "dendrogram"))
