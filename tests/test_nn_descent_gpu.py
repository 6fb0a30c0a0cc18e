"""GPU: NN-descent kNN-graph builder (CAGRA build_algo = NN_DESCENT; reference cpp/src/neighbors/detail/nn_descent.cuh,
tests cpp/tests/neighbors/ann_nn_descent.cuh: graph recall against brute force >= min_recall)."""
import ctypes as C

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu


def _nn_descent(x, K, metric=0, n_iters=20):
    import torch
    from cuvs_amd._lib import check, lib
    from cuvs_amd.common import Resources

    res = Resources()
    tx = torch.from_numpy(x).cuda()
    out = torch.empty((x.shape[0], K), dtype=torch.int32, device="cuda")
    fn = lib().cuvsAmdNnDescent
    fn.restype = C.c_int
    check(fn(res.get_c_obj(), C.c_void_p(tx.data_ptr()), C.c_int64(x.shape[0]), C.c_int64(x.shape[1]),
             C.c_uint32(K), C.c_int(metric), C.c_int(n_iters), C.c_void_p(out.data_ptr())))
    res.sync()
    return out.cpu().numpy().view(np.uint32).astype(np.int64)


@pytest.mark.parametrize("metric", ["sqeuclidean", "inner_product", "cosine"])
def test_graph_recall(metric):
    rng = np.random.default_rng(0)
    n, d, K = 20000, 32, 32
    x = rng.standard_normal((n, d)).astype(np.float32)
    g = _nn_descent(x, K, metric={"sqeuclidean": 0, "cosine": 2, "inner_product": 6}[metric])
    assert g.shape == (n, K) and (g < n).all()
    assert (g != np.arange(n)[:, None]).all()                    # no self edges
    assert all(len(np.unique(r)) == K for r in g[:500])          # no duplicate edges
    rows = rng.choice(n, 300, replace=False)
    if metric == "cosine":
        xn = x / np.linalg.norm(x, axis=1, keepdims=True)
        sim = xn[rows] @ xn.T
    elif metric == "inner_product":
        sim = x[rows] @ x.T
    else:
        sim = -((x[rows][:, None, :] - x[None, :, :]) ** 2).sum(-1) if n <= 2000 else None
        if sim is None:
            sim = -(np.sum(x[rows] ** 2, 1)[:, None] + np.sum(x ** 2, 1)[None, :] - 2 * x[rows] @ x.T)
    sim[np.arange(len(rows)), rows] = -np.inf
    truth = np.argsort(-sim, axis=1, kind="stable")[:, :K]
    rec = np.mean([len(np.intersect1d(g[r], t)) for r, t in zip(rows, truth)]) / K
    assert rec >= 0.9, rec


def test_cagra_build_with_nn_descent():
    import torch
    from cuvs_amd.neighbors import cagra

    rng = np.random.default_rng(1)
    x = rng.standard_normal((30000, 48)).astype(np.float32)
    q = rng.standard_normal((200, 48)).astype(np.float32)
    index = cagra.build(cagra.IndexParams(intermediate_graph_degree=64, graph_degree=32, build_algo="nn_descent",
                                          nn_descent_niter=20), torch.from_numpy(x).cuda())
    g = index.graph.cpu().numpy().view(np.uint32).astype(np.int64)
    assert g.shape == (30000, 32) and (g < 30000).all() and (g != np.arange(30000)[:, None]).all()
    d, i = cagra.search(cagra.SearchParams(itopk_size=64), index, torch.from_numpy(q).cuda(), 10)
    torch.cuda.synchronize()
    _, ti = oracle.exact_knn(q, x, 10)
    # (the descent depends on atomic order like the reference's: 0.947 .. 0.955 over runs; ann_nn_descent.cuh asks for 0.9)
    assert oracle.recall(i.cpu().numpy().astype(np.int64) & 0xFFFFFFFF, ti) >= 0.93


@pytest.mark.parametrize("host_dataset", [False, True])
def test_standalone_c_api(host_dataset):
    """cuvsNNDescentBuild / GetGraph / GetDistances (c/include/cuvs/neighbors/nn_descent.h; reference python test
    python/cuvs/cuvs/tests/test_nn_descent.py: graph recall against brute force)."""
    import torch
    from cuvs_amd._lib import CuvsError
    from cuvs_amd.neighbors import nn_descent

    rng = np.random.default_rng(3)
    n, d, deg = 12000, 24, 32
    x = rng.standard_normal((n, d)).astype(np.float32)
    out_graph = np.zeros((n, deg), np.uint32) if host_dataset else None
    idx = nn_descent.build(nn_descent.IndexParams(graph_degree=deg, intermediate_graph_degree=48),
                           x if host_dataset else torch.from_numpy(x).cuda(), graph=out_graph)
    g = idx.graph.cpu().numpy().view(np.uint32).astype(np.int64)
    dist = idx.distances.cpu().numpy()
    assert g.shape == (n, deg) and dist.shape == (n, deg) and (g < n).all()
    if out_graph is not None:
        assert (out_graph.astype(np.int64) == g).all()
    rows = rng.choice(n, 200, replace=False)
    d2 = np.sum(x[rows] ** 2, 1)[:, None] + np.sum(x ** 2, 1)[None, :] - 2 * x[rows] @ x.T
    d2[np.arange(len(rows)), rows] = np.inf
    truth = np.argsort(d2, axis=1, kind="stable")[:, :deg]
    rec = np.mean([len(np.intersect1d(g[r], t)) for r, t in zip(rows, truth)]) / deg
    assert rec >= 0.9, rec
    # distances are the squared L2 distances of the listed neighbours, ascending
    want = ((x[rows][:, None, :] - x[g[rows]]) ** 2).sum(-1)
    np.testing.assert_allclose(dist[rows], want, rtol=1e-4, atol=1e-4)
    assert (np.diff(dist[rows], axis=1) >= 0).all()
    # no distances when not requested
    idx2 = nn_descent.build(nn_descent.IndexParams(graph_degree=16, intermediate_graph_degree=32, return_distances=False,
                                                   max_iterations=3), torch.from_numpy(x[:2000]).cuda())
    with pytest.raises(CuvsError):
        idx2.distances


# ----------------------------------------------------------------------------------- whole-graph invariants, every row
FLT_MAX = np.float32(3.4028234663852886e38)
_DT = {"f32": np.float32, "f16": np.float16, "i8": np.int8, "u8": np.uint8}


def _typed_rows(n, dim, dt, seed):
    """float rows ~ N(0.1, 2.0), int8 uniform [-5, 5), uint8 uniform [0, 5): the reference's generators (ann_nn_descent.cuh:162-173)"""
    rng = np.random.default_rng(seed)
    if dt == "i8":
        return rng.integers(-5, 5, (n, dim)).astype(np.int8)
    if dt == "u8":
        return rng.integers(0, 5, (n, dim)).astype(np.uint8)
    return (rng.standard_normal((n, dim)) * 2.0 + 0.1).astype(_DT[dt])


def _build_graph(x, metric, host=False, degree=32, intermediate=64):
    import torch
    from cuvs_amd.neighbors import nn_descent

    idx = nn_descent.build(nn_descent.IndexParams(metric=metric, graph_degree=degree, intermediate_graph_degree=intermediate),
                           x if host else torch.from_numpy(x).cuda())
    return idx.graph.cpu().numpy().view(np.uint32).astype(np.int64), idx.distances.cpu().numpy()


def _check_graph(x, metric, g, dist):
    """Every row of the graph: ids in [0, n) or 0xffffffff, invalid ids at the tail only and with distance FLT_MAX, no self
    edge, no duplicate, distances ordered (ascending; descending for inner product) and equal to the float64 distance of the
    listed pair within the bound DERIVED in nn_descent_ref.exact_distance_and_bound (U = 2^-24 times the number of roundings
    on the path of a term, times the sum of the terms' magnitudes, carried through the root and the cosine quotient with the
    error of the fp32 norms) - integer rows under L2 / inner product have exact sums and must match exactly."""
    from tests import nn_descent_ref as R

    n = x.shape[0]
    deg = g.shape[1]
    assert g.shape == dist.shape
    invalid = g == 0xFFFFFFFF
    assert ((g >= 0) & (g < n) | invalid).all()
    assert (invalid[:, 1:] >= invalid[:, :-1]).all()                       # once invalid, invalid to the end of the row
    assert (dist[invalid] == FLT_MAX).all() and np.isfinite(dist).all()
    assert (g != np.arange(n)[:, None]).all()
    s = np.sort(np.where(invalid, -1 - np.arange(deg)[None, :], g), axis=1)   # invalid slots get distinct negative stand-ins
    assert (s[:, 1:] != s[:, :-1]).all(), "duplicate edge"
    step = np.diff(dist.astype(np.float64), axis=1)
    both = ~invalid[:, 1:]
    assert ((step <= 0) if metric == "inner_product" else (step >= 0))[both].all()
    rows, cols = np.nonzero(~invalid)
    a, b = rows, g[rows, cols]
    got = dist[rows, cols]
    want, bound = R.exact_distance_and_bound(x, a, b, metric)
    if x.dtype.kind in "iu" and metric != "cosine":
        exact = want.astype(np.float32) if metric != "euclidean" else np.sqrt(((x[a].astype(np.int64) - x[b]) ** 2).sum(1).astype(np.float32))
        assert (got == exact).all()
    err = np.abs(got.astype(np.float64) - want)
    assert (err <= bound).all(), (err.max(), bound[err.argmax()])
    return rows, cols


_GRAPH_CASES = [(n, dt, m) for n in (33, 130, 300, 500, 2000) for dt in ("f32", "f16", "i8", "u8")
                for m in ("sqeuclidean", "euclidean", "inner_product", "cosine")]


@pytest.mark.parametrize("n,dt,metric", _GRAPH_CASES)
def test_graph_invariants(n, dt, metric):
    """graph degree 32 over lists of 64 (internally 96): n = 33 is K = n - 1; 130 and 300 have neither clusters nor hubs;
    500 has hubs (inner product) without clusters; 2000 has clusters, and hubs under inner product. dim 20 ends inside a
    16-byte piece for every row type."""
    x = _typed_rows(n, 20, dt, n)
    g, dist = _build_graph(x, metric)
    assert g.shape == (n, 32)
    _check_graph(x, metric, g, dist)


@pytest.mark.parametrize("dt,metric", [("f32", "cosine"), ("i8", "inner_product")])
def test_graph_invariants_host_dataset(dt, metric):
    x = _typed_rows(300, 20, dt, 77)
    g, dist = _build_graph(x, metric, host=True)
    _check_graph(x, metric, g, dist)


@pytest.mark.parametrize("dt", ["f32", "i8"])
def test_cosine_with_a_zero_row(dt):
    """detail/nn_descent.cuh:534-537: a pair with a zero row has cosine distance 0 - not 0 / 0"""
    n, zero = 300, 41
    x = _typed_rows(n, 20, dt, 5)
    x[zero] = 0
    g, dist = _build_graph(x, "cosine")
    assert np.isfinite(dist).all()
    rows, cols = _check_graph(x, "cosine", g, dist)
    with_zero = (rows == zero) | (g[rows, cols] == zero)
    assert with_zero.sum() >= 32 and (dist[rows, cols][with_zero] == 0).all()
    assert (dist[zero] == 0).all() and (g[zero] != 0xFFFFFFFF).all()


@pytest.mark.parametrize("dt", ["f16", "i8"])
def test_cagra_build_with_nn_descent_typed_rows(dt):
    import torch
    from cuvs_amd.neighbors import cagra

    rng = np.random.default_rng(2)
    n, dim = 2000, 32
    if dt == "i8":   # the whole int8 range: few ties between distances, so the exact neighbours are well defined
        x, q = (rng.integers(-128, 128, (m, dim)).astype(np.int8) for m in (n, 100))
    else:
        x, q = (rng.standard_normal((m, dim)).astype(np.float16) for m in (n, 100))
    index = cagra.build(cagra.IndexParams(intermediate_graph_degree=64, graph_degree=32, build_algo="nn_descent",
                                          nn_descent_niter=20), torch.from_numpy(x).cuda())
    g = index.graph.cpu().numpy().view(np.uint32).astype(np.int64)
    assert g.shape == (n, 32) and (g < n).all() and (g != np.arange(n)[:, None]).all()
    d, i = cagra.search(cagra.SearchParams(itopk_size=64), index, torch.from_numpy(q).cuda(), 10)
    torch.cuda.synchronize()
    _, ti = oracle.exact_knn(q.astype(np.float32), x.astype(np.float32), 10)
    assert oracle.recall(i.cpu().numpy().astype(np.int64) & 0xFFFFFFFF, ti) >= 0.93    # the threshold of the fp32 test above
