"""GPU: cuvsAllNeighbors* - the remap-merge kernel, single and batched builds and mutual reachability against the numpy
restatement (tests/all_neighbors_ref.py) bit for bit; NN-descent / IVF-PQ builders against the recall table of the
reference's own test (tests/golden/all_neighbors_reference_table.json); refusals; the Python surface."""
import functools
import json
import os

import numpy as np
import pytest

import oracle
from tests import all_neighbors_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF_METRICS = ["sqeuclidean", "euclidean", "cosine", "l2_unexpanded", "l2_sqrt_unexpanded", "inner_product"]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _assert_same(got_i, got_d, want_i, want_d):
    got_i, got_d = got_i.cpu().numpy(), got_d.cpu().numpy()
    bad = np.argwhere(got_i != want_i)
    assert bad.size == 0, f"{len(bad)} ids differ, first at {bad[0]}: {got_i[tuple(bad[0])]} != {want_i[tuple(bad[0])]}"
    bad = np.argwhere(_bits(got_d) != _bits(want_d))
    assert bad.size == 0, f"{len(bad)} distances differ, first at {bad[0]}: {got_d[tuple(bad[0])]!r} != {want_d[tuple(bad[0])]!r}"


def _rows_sorted_and_distinct(ids, d, select_min):
    fid, _ = R.fill_values(select_min)
    key = R.float_key(d if select_min else -d).astype(np.int64)
    assert (np.diff(key, axis=1) >= 0).all(), "a row is not sorted"
    tie = np.diff(key, axis=1) == 0
    real = (ids[:, 1:] != fid) & (ids[:, :-1] != fid)
    assert (np.diff(ids.astype(np.float64), axis=1)[tie & real] > 0).all(), "equal distances are not ordered by id"
    for row in ids:
        r = row[row != fid]
        assert len(np.unique(r)) == len(r), "an id appears twice in a row"


def _uniform(n, dim, seed):
    return np.random.default_rng(seed).random((n, dim), dtype=np.float32) - np.float32(0.5)


def _blobs(n, dim, seed=0, centers=5):
    """make_blobs defaults: centres uniform in [-10, 10], unit standard deviation."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-10.0, 10.0, (centers, dim))
    return (c[rng.integers(0, centers, n)] + rng.standard_normal((n, dim))).astype(np.float32)


# ---------------------------------------------------------------- 1. the merge kernel alone
def _pair_dist(g, ids, ties):
    h = (np.int64(g) * 2654435761 + ids.astype(np.int64) * 40503) % 100003
    if ties:
        h = h % 4  # runs of equal distances with distinct ids
    return (h.astype(np.float32) + np.float32(1)) / np.float32(8)


def _merge_case(kind, k, seed):
    """300 cluster rows into a 500-row global matrix. Batch rows hold min(k, 300) distinct local ids (the rest are the -1 /
    worst-value padding select_k writes); global rows are sorted, their ids are ids of batch entries (same pair, same
    distance: duplicates) or ids >= n (no overlap), and may be partly unfilled."""
    rng = np.random.default_rng(seed)
    n, m = 500, 300
    select_min = kind != "max"
    ties = kind == "ties"
    fid, fd = R.fill_values(select_min)
    inv = np.sort(rng.choice(n, m, replace=False)).astype(np.int64)
    nb = min(k, m)

    def write(ids_out, d_out, r, g, ids_sort, ids_store):
        d = _pair_dist(g, ids_sort, ties)
        order = np.lexsort((ids_sort, R.float_key(d if select_min else -d)))
        ids_out[r, : len(order)] = ids_store[order]
        d_out[r, : len(order)] = d[order]

    bi = np.full((m, k), -1, np.int64)
    bd = np.full((m, k), fd, np.float32)
    for b in range(m):
        loc = rng.choice(m, nb, replace=False).astype(np.int64)
        write(bi, bd, b, inv[b], inv[loc], loc)
    gi = np.full((n, k), fid, np.int64)
    gd = np.full((n, k), fd, np.float32)
    row_of = {int(g): b for b, g in enumerate(inv)}
    for g in range(n):
        if kind == "fill":
            break
        b = row_of.get(g)
        if b is None or kind == "disjoint":
            ids = n + rng.choice(5000, int(rng.integers(0, k + 1)), replace=False)
        elif kind == "dup":
            ids = inv[bi[b, :nb]]
        else:  # about half of the batch row's entries are in the global row already
            take = inv[bi[b, :nb]][rng.random(nb) < 0.5][:k]
            ids = np.concatenate([take, n + rng.choice(5000, int(rng.integers(0, k - len(take) + 1)), replace=False)])
        ids = ids.astype(np.int64)
        write(gi, gd, g, g, ids, ids)
    return inv, bi, bd, gi, gd, select_min


@pytest.mark.parametrize("kind", ["fill", "dup", "disjoint", "half", "ties", "max"])
@pytest.mark.parametrize("k", [1, 2, 16, 23, 32, 33, 64, 65, 200, 1024])
def test_merge_kernel_equals_the_restatement(res, k, kind):
    import torch
    from cuvs_amd.neighbors import all_neighbors as AN

    inv, bi, bd, gi, gd, select_min = _merge_case(kind, k, 1000 + k)
    want_i, want_d = R.remap_merge(inv, bi, bd, gi.copy(), gd.copy(), select_min)
    t = [torch.from_numpy(a).cuda() for a in (inv, bi, bd, gi, gd)]
    AN.merge(*t, select_min=select_min, resources=res)
    res.sync()
    _assert_same(t[3], t[4], want_i, want_d)
    got_i, got_d = t[3].cpu().numpy(), t[4].cpu().numpy()
    _rows_sorted_and_distinct(got_i[inv], got_d[inv], select_min)
    untouched = np.setdiff1d(np.arange(gi.shape[0]), inv)
    assert (got_i[untouched] == gi[untouched]).all() and (_bits(got_d[untouched]) == _bits(gd[untouched])).all()
    if kind == "dup":  # nothing new: the merged rows are the batch rows
        assert (got_i[inv][:, : min(k, 300)] == inv[bi[:, : min(k, 300)]]).all()


# ---------------------------------------------------------------- 2. single build, brute force
@functools.lru_cache(maxsize=None)
def _single_case(metric):
    import torch
    from cuvs_amd.neighbors import brute_force

    x = _uniform(1000, 33, 7)
    xd = torch.from_numpy(x).cuda()
    d, i = brute_force.search(brute_force.build(xd, metric=metric), xd, 16)
    return x, xd, i.cpu().numpy(), d.cpu().numpy()


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("metric", BF_METRICS)
def test_single_brute_force_equals_brute_force_search(res, metric, where):
    import torch
    from cuvs_amd.neighbors import all_neighbors as AN

    x, xd, want_i, want_d = _single_case(metric)
    p = AN.AllNeighborsParams(algo="brute_force", metric=metric)
    dist = torch.empty((1000, 16), dtype=torch.float32, device="cuda")
    ids, dist, core = AN.build(x if where == "host" else xd, 16, p, distances=dist, resources=res)
    res.sync()
    assert core is None
    _assert_same(ids, dist, want_i, want_d)


def test_single_brute_force_without_distances(res):
    from cuvs_amd.neighbors import all_neighbors as AN

    x, xd, want_i, _ = _single_case("sqeuclidean")
    ids, dist, core = AN.build(xd, 16, AN.AllNeighborsParams(algo="brute_force"), resources=res)
    res.sync()
    assert dist is None and core is None
    assert (ids.cpu().numpy() == want_i).all()


# ---------------------------------------------------------------- 3. batched brute force
def _exact_knn(metric):
    return lambda rows, inv_c, k: oracle.brute_force_knn(rows, rows, k, metric)


@pytest.mark.parametrize("dim,k", [(16, 16), (33, 23)])
@pytest.mark.parametrize("n_clusters,overlap", [(4, 2), (7, 2), (10, 3)])
@pytest.mark.parametrize("metric", ["sqeuclidean", "euclidean", "cosine", "inner_product"])
def test_batched_brute_force_equals_the_restatement(res, metric, n_clusters, overlap, dim, k):
    import torch
    from cuvs_amd.neighbors import all_neighbors as AN

    x = _uniform(2000, dim, 11)
    p = AN.AllNeighborsParams(algo="brute_force", metric=metric, n_clusters=n_clusters, overlap_factor=overlap)
    cent, near = AN.partition(x, p, resources=res)
    cent2, near2 = AN.partition(x, p, resources=res)
    assert (_bits(cent) == _bits(cent2)).all() and (near == near2).all(), "the partition is not deterministic"
    _, want_near = oracle.brute_force_knn(x, cent, overlap, metric)
    assert (near == want_near).all(), "a row is not assigned to its nearest centroids"
    select_min = metric != "inner_product"
    want_i, want_d = R.batched_build(x, k, near, n_clusters, _exact_knn(metric), select_min)
    dist = torch.empty((2000, k), dtype=torch.float32, device="cuda")
    ids, dist, _ = AN.build(x, k, p, distances=dist, resources=res)
    res.sync()
    _assert_same(ids, dist, want_i, want_d)
    _rows_sorted_and_distinct(want_i, want_d, select_min)


def test_batched_build_skips_a_cluster_below_k(res):
    import torch
    from cuvs_amd.neighbors import all_neighbors as AN
    from cuvs_amd.neighbors import brute_force

    rng = np.random.default_rng(5)
    x = np.concatenate([rng.standard_normal((1980, 8)), 1000.0 + rng.standard_normal((20, 8))]).astype(np.float32)
    k = 32
    p = AN.AllNeighborsParams(algo="brute_force", n_clusters=3, overlap_factor=1)
    _, near = AN.partition(x, p, resources=res)
    inv, sizes, offsets = R.inverted_lists(near, 3)
    assert (sizes < k).any(), f"vacuous: no cluster below k rows (sizes {sizes.tolist()})"
    assert (sizes >= k).any()
    dist = torch.empty((2000, k), dtype=torch.float32, device="cuda")
    ids, dist, _ = AN.build(x, k, p, distances=dist, resources=res)
    res.sync()
    want_i, want_d = R.batched_build(x, k, near, 3, _exact_knn("sqeuclidean"))
    _assert_same(ids, dist, want_i, want_d)
    skipped_rows = np.concatenate([inv[offsets[c] : offsets[c] + sizes[c]] for c in range(3) if sizes[c] < k])
    fid, fd = R.fill_values(True)
    got_i, got_d = ids.cpu().numpy(), dist.cpu().numpy()
    assert (got_i[skipped_rows] == fid).all() and (got_d[skipped_rows] == fd).all()
    # the same build step by step: brute force per cluster + the merge hook
    gi = torch.full((2000, k), fid, dtype=torch.int64, device="cuda")
    gd = torch.full((2000, k), float(fd), dtype=torch.float32, device="cuda")
    for c in range(3):
        if sizes[c] < k:
            continue
        inv_c = inv[offsets[c] : offsets[c] + sizes[c]]
        rows = torch.from_numpy(x[inv_c]).cuda()
        bd, bi = brute_force.search(brute_force.build(rows), rows, k)
        AN.merge(torch.from_numpy(inv_c).cuda(), bi, bd, gi, gd, resources=res)
    res.sync()
    _assert_same(gi, gd, got_i, got_d)


# ---------------------------------------------------------------- 4. mutual reachability, brute force
def _reach_knn(metric, core, alpha):
    def knn(rows, inv_c, k):
        d = oracle.pairwise(rows, rows, metric)
        return oracle.select_k(R.reach_epilogue(d, core[inv_c], core[inv_c], alpha), k)

    return knn


@pytest.mark.parametrize("alpha", [1.0, 0.5])
@pytest.mark.parametrize("metric", ["sqeuclidean", "euclidean", "cosine"])
@pytest.mark.parametrize("n,n_clusters", [(1000, 1), (2000, 4)])
def test_mutual_reachability_equals_the_restatement(res, n, n_clusters, metric, alpha):
    import torch
    from cuvs_amd.neighbors import all_neighbors as AN

    k = 16
    x = _uniform(n, 33, 13)
    p = AN.AllNeighborsParams(algo="brute_force", metric=metric, n_clusters=n_clusters, overlap_factor=2)
    plain_d = torch.empty((n, k), dtype=torch.float32, device="cuda")
    AN.build(x, k, p, distances=plain_d, resources=res)
    dist = torch.empty((n, k), dtype=torch.float32, device="cuda")
    core = torch.empty((n,), dtype=torch.float32, device="cuda")
    ids, dist, core = AN.build(x, k, p, distances=dist, core_distances=core, alpha=alpha, resources=res)
    res.sync()
    assert (_bits(core.cpu().numpy()) == _bits(plain_d.cpu().numpy()[:, k - 1])).all()
    if n_clusters == 1:
        near = np.zeros((n, 1), np.int64)
    else:
        _, near = AN.partition(x, p, resources=res)
    first_i, first_d = R.batched_build(x, k, near, n_clusters, _exact_knn(metric))
    want_core = R.core_distances(first_d)
    assert (_bits(core.cpu().numpy()) == _bits(want_core)).all()
    want_i, want_d = R.batched_build(x, k, near, n_clusters, _reach_knn(metric, want_core, alpha))
    _assert_same(ids, dist, want_i, want_d)


# ---------------------------------------------------------------- 5. NN-descent and IVF-PQ against the reference's table
def _table():
    with open(os.path.join(ROOT, "tests", "golden", "all_neighbors_reference_table.json")) as f:
        return json.load(f)


def _min_recall(group, algo, metric):
    rows = [r for r in _table()["rows"] if (r["group"], r["algo"], r["metric"]) == (group, algo, metric)]
    assert len(rows) == 1
    return rows[0]["min_recall"]


@functools.lru_cache(maxsize=None)
def _blob_truth(metric):
    x = _blobs(5000, 64)
    return x, oracle.brute_force_knn(x, x, 16, metric)[1]


_ALGO_METRICS = [("brute_force", m) for m in ("sqeuclidean", "euclidean", "inner_product", "cosine")] + [("ivf_pq", "sqeuclidean")] + \
    [("nn_descent", m) for m in ("sqeuclidean", "euclidean", "cosine", "inner_product")]
# every (algo, metric) single and at (4, 2); 7 and 10 clusters once per builder
_RECALL_CASES = [(a, m, 1) for a, m in _ALGO_METRICS] + [(a, m, 4) for a, m in _ALGO_METRICS] + \
    [("nn_descent", "sqeuclidean", 7), ("ivf_pq", "sqeuclidean", 7), ("brute_force", "sqeuclidean", 10), ("nn_descent", "cosine", 10)]


@pytest.mark.parametrize("algo,metric,n_clusters", _RECALL_CASES)
def test_recall_meets_the_reference_table(res, algo, metric, n_clusters):
    import torch
    from cuvs_amd.neighbors import all_neighbors as AN
    from cuvs_amd.neighbors import ivf_pq, nn_descent

    n, k = 5000, 16
    x, truth = _blob_truth(metric)
    kw = {}
    if algo == "nn_descent":  # the settings of the reference's test
        kw["nn_descent_params"] = nn_descent.IndexParams(metric=metric, graph_degree=k, intermediate_graph_degree=2 * k,
                                                         max_iterations=100)
    elif algo == "ivf_pq":
        kw["ivf_pq_params"] = ivf_pq.IndexParams(metric=metric, n_lists=max(5, n * 2 // (5000 * n_clusters)))
    p = AN.AllNeighborsParams(algo=algo, metric=metric, n_clusters=n_clusters, overlap_factor=2, **kw)
    dist = torch.empty((n, k), dtype=torch.float32, device="cuda")
    ids, dist, _ = AN.build(x if n_clusters > 1 else torch.from_numpy(x).cuda(), k, p, distances=dist, resources=res)
    res.sync()
    got, got_d = ids.cpu().numpy(), dist.cpu().numpy()
    recall = oracle.recall(got, truth)
    want = _min_recall("inputsSingle" if n_clusters == 1 else "inputsBatch", algo, metric)
    print(f"all_neighbors recall {algo} {metric} n_clusters={n_clusters}: {recall:.4f} (table {want})")
    assert recall >= want - _table()["recall_eps"]
    fid, _ = R.fill_values(metric != "inner_product")
    for row in got:
        r = row[row != fid]
        assert len(np.unique(r)) == len(r), "an id appears twice in a row"
    if algo == "nn_descent" and metric != "inner_product":  # the shift: every row starts with itself at distance 0
        assert (got[:, 0] == np.arange(n)).all() and (got_d[:, 0] == 0.0).all()


def test_the_table_lists_nn_descent_mutual_reachability_rows_which_are_refused_here(res):
    import torch
    from cuvs_amd._lib import CuvsError
    from cuvs_amd.neighbors import all_neighbors as AN

    rows = [r for r in _table()["rows"] if r["mutual_reach"] and r["algo"] == "nn_descent"]
    assert len(rows) == 6
    x = _uniform(200, 8, 1)
    for r in rows[:3]:
        p = AN.AllNeighborsParams(algo="nn_descent", metric=r["metric"])
        d = torch.empty((200, 4), dtype=torch.float32, device="cuda")
        c = torch.empty((200,), dtype=torch.float32, device="cuda")
        with pytest.raises(CuvsError, match="NN Descent"):
            AN.build(x, 4, p, distances=d, core_distances=c, resources=res)


# ---------------------------------------------------------------- 6. refusals
def test_refusals(res):
    import torch
    from cuvs_amd._lib import CuvsError
    from cuvs_amd.neighbors import all_neighbors as AN

    x = _uniform(300, 8, 2)
    xd = torch.from_numpy(x).cuda()
    k = 4
    dist = torch.empty((300, k), dtype=torch.float32, device="cuda")
    core = torch.empty((300,), dtype=torch.float32, device="cuda")
    P = AN.AllNeighborsParams
    with pytest.raises(ValueError, match="not supported with data on device"):
        AN.build(xd, k, P(algo="brute_force", n_clusters=4), resources=res)
    # the same refusal from the C entry point (a pinned / device tensor reaching it directly)
    p4 = P(algo="brute_force", n_clusters=4)
    from cuvs_amd._lib import Tensor, lib
    import ctypes as C
    td, ti = Tensor(xd), Tensor(torch.empty((300, k), dtype=torch.int64, device="cuda"))
    fn = lib().cuvsAllNeighborsBuild
    fn.argtypes = [C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float]
    assert fn(res.get_c_obj(), p4.get_handle(), C.addressof(td.m), C.addressof(ti.m), None, None, 1.0) == 0
    assert b"Batched all-neighbors build is not supported with data on device" in lib().cuvsGetLastErrorText()
    with pytest.raises(CuvsError, match="overlap_factor should be smaller than n_clusters"):
        AN.build(x, k, P(algo="brute_force", n_clusters=2, overlap_factor=2), resources=res)
    with pytest.raises(CuvsError, match="IVFPQ should be L2Expanded"):
        AN.build(x, k, P(algo="ivf_pq", metric="cosine"), resources=res)
    with pytest.raises(CuvsError, match="cannot be calculated using IVFPQ"):
        AN.build(x, k, P(algo="ivf_pq"), distances=dist, core_distances=core, resources=res)
    with pytest.raises(CuvsError, match="NN Descent is not supported"):
        AN.build(x, k, P(algo="nn_descent"), distances=dist, core_distances=core, resources=res)
    with pytest.raises(ValueError, match="distances must be provided"):
        AN.build(x, k, P(algo="brute_force"), core_distances=core, resources=res)
    with pytest.raises(CuvsError, match="indices should be of type int64_t"):
        AN.build(x, k, P(algo="brute_force"), indices=torch.empty((300, k), dtype=torch.int32, device="cuda"), resources=res)
    with pytest.raises(CuvsError, match="dataset must be float32"):
        AN.build(xd.half(), k, P(algo="brute_force"), resources=res)
    with pytest.raises(CuvsError, match="batched build takes k <= 1024"):
        AN.build(_uniform(1100, 4, 3), 1025, P(algo="brute_force", n_clusters=2, overlap_factor=1), resources=res)
    with pytest.raises(CuvsError, match="all-neighbors build with brute force should be"):
        AN.build(x, k, P(algo="brute_force", metric="l1"), resources=res)
    with pytest.raises(CuvsError, match="mutual reachability distance should be"):
        AN.build(x, k, P(algo="brute_force", metric="inner_product"), distances=dist, core_distances=core, resources=res)


# ---------------------------------------------------------------- 7. the Python surface
def test_python_surface():
    from cuvs_amd.neighbors import all_neighbors as AN
    from cuvs_amd.neighbors import ivf_pq, nn_descent
    import cuvs_amd.neighbors

    assert cuvs_amd.neighbors.all_neighbors is AN
    p = AN.AllNeighborsParams()
    assert (p.algo, p.overlap_factor, p.n_clusters, p.metric) == ("nn_descent", 2, 1, "sqeuclidean")
    assert p.params.ivf_pq_params is None and p.params.nn_descent_params is None
    p = AN.AllNeighborsParams(algo="ivf_pq", overlap_factor=3, n_clusters=8, metric="inner_product")
    assert (p.algo, p.overlap_factor, p.n_clusters, p.metric) == ("ivf_pq", 3, 8, "inner_product")
    assert AN.AllNeighborsParams(algo=0).algo == "brute_force"
    with pytest.raises(ValueError, match="Invalid algo"):
        AN.AllNeighborsParams(algo="hnsw")
    nnd = nn_descent.IndexParams(metric="cosine")
    with pytest.raises(ValueError, match="Metric conflict"):
        AN.AllNeighborsParams(algo="nn_descent", metric="sqeuclidean", nn_descent_params=nnd)
    with pytest.raises(ValueError, match="Metric conflict"):
        AN.AllNeighborsParams(algo="ivf_pq", metric="sqeuclidean", ivf_pq_params=ivf_pq.IndexParams(metric="inner_product"))
    p = AN.AllNeighborsParams(algo="nn_descent", metric="cosine", nn_descent_params=nnd)
    assert p.params.nn_descent_params is not None
    del p  # the nested struct is borrowed: freed once, by its own wrapper
    del nnd
    with pytest.raises(TypeError):
        AN.build(np.zeros((4, 2), np.float32), 2, object())
