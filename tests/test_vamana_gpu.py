"""GPU: the Vamana search kernel, prune kernel and whole build equal tests/vamana_ref.py bit for bit; the built graph passes the
reference's own test (graph checks, recall through a CAGRA search of the graph); the files equal the twin's writers."""
import ctypes as C
import functools
import struct

import numpy as np
import pytest
import torch

from tests import vamana_ref as ref
from cuvs_amd._lib import CuvsError, Tensor, check, lib
from cuvs_amd.neighbors import cagra, vamana

pytestmark = pytest.mark.gpu
INVALID = ref.INVALID


def _u32(t):
    """A Tensor over an int32 torch tensor that holds uint32 bits."""
    x = Tensor(t)
    x.m.dl_tensor.dtype.code = 1
    return x


def _dev_u32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()


def _host_u32(t):
    return t.cpu().numpy().view(np.uint32)


def rows_of(n, dim, dtype, seed=1234):
    rng = np.random.default_rng(seed)
    x = rng.normal(0.1, 2.0, (n, dim))
    if dtype == np.float32:
        return x.astype(np.float32)
    lo, hi = (-128, 127) if dtype == np.int8 else (0, 255)
    return np.clip(np.rint(x * 20 + (0 if dtype == np.int8 else 100)), lo, hi).astype(dtype)


def params_pair(**kw):
    return vamana.IndexParams(**kw), ref.Params(**kw)


@functools.lru_cache(maxsize=None)
def twin_topology(degree, visited):
    """A graph the twin built over 300 rows; the search tests walk it over other rows of the same count as a fixed graph."""
    g, med = ref.build(rows_of(300, 16, np.float32, seed=7), ref.Params(graph_degree=degree, visited_size=visited))
    return g, med


def hand_made_graph(n, degree):
    """Short rows, nodes nobody points to, a node without edges, a repeated neighbour."""
    g = np.full((n, degree), INVALID, dtype=np.uint32)
    for i in range(n):
        if i % 7 == 3:
            continue  # no edges at all
        k = 1 + (i * 5) % 9
        nb = [(i * 13 + 1 + 3 * j) % (n - 20) for j in range(k)]  # the last 20 nodes are unreachable
        nb = [v for v in nb if v != i]
        if i % 11 == 0 and nb:
            nb.append(nb[0])
        g[i, :len(nb)] = nb
    return g


def gpu_search(res, cp, x, graph, med, qids):
    V = ref.Params(graph_degree=cp.graph_degree, visited_size=cp.visited_size).visited
    xd = torch.from_numpy(x).cuda()
    gd, qd = _dev_u32(graph), _dev_u32(qids)
    oi = torch.empty((len(qids), V), dtype=torch.int32, device="cuda")
    od = torch.empty((len(qids), V), dtype=torch.float32, device="cuda")
    check(lib().cuvsAmdVamanaGreedySearch(res.get_c_obj(), cp._p, Tensor(xd).ptr, _u32(gd).ptr, C.c_uint32(med), _u32(qd).ptr,
                                          _u32(oi).ptr, Tensor(od).ptr))
    res.sync()
    return _host_u32(oi), od.cpu().numpy()


def check_search(res, x, graph, med, qids, **kw):
    cp, rp = params_pair(**kw)
    ids, dists = gpu_search(res, cp, x, graph, med, qids)
    for r, q in enumerate(qids):
        wi, wd = ref.greedy_search(x, graph, med, int(q), rp)
        assert np.array_equal(ids[r], wi), f"ids of query {q}"
        assert np.array_equal(dists[r].view(np.uint32), wd.view(np.uint32)), f"distance bits of query {q}"
    return ids


QIDS = np.arange(0, 300, 5, dtype=np.uint32)


@pytest.mark.parametrize("dtype", [np.float32, np.int8, np.uint8], ids=["f32", "i8", "u8"])
@pytest.mark.parametrize("dim", [1, 3, 17, 64, 128, 137])
def test_search_kernel_equals_the_twin_on_a_twin_built_graph(res, dim, dtype):
    g, med = twin_topology(32, 64)
    ids = check_search(res, rows_of(300, dim, dtype), g, med, QIDS)
    assert (ids != INVALID).sum(axis=1).min() > 8  # the walks are real walks


@pytest.mark.parametrize("degree,visited,dim,dtype", [(64, 128, 64, np.float32), (64, 128, 17, np.uint8), (32, 128, 137, np.int8),
                                                      (32, 100, 3, np.float32)])
def test_search_kernel_other_degrees_and_list_sizes(res, degree, visited, dim, dtype):
    g, med = twin_topology(degree, 128 if degree == 64 else 64)
    check_search(res, rows_of(300, dim, dtype), g, med, QIDS, graph_degree=degree, visited_size=visited)


@pytest.mark.parametrize("dtype", [np.float32, np.uint8], ids=["f32", "u8"])
def test_search_kernel_on_a_hand_made_graph_with_short_rows_and_unreachable_nodes(res, dtype):
    g = hand_made_graph(300, 32)
    ids = check_search(res, rows_of(300, 17, dtype), g, 5, np.arange(300, dtype=np.uint32))
    assert not np.isin(ids[ids != INVALID], np.arange(280, 300)).any()
    # a medoid without edges: only the medoid itself is expanded
    ids = check_search(res, rows_of(300, 17, dtype), g, 3, QIDS)
    assert ((ids != INVALID).sum(axis=1) == (QIDS != 3)).all()


def test_search_kernel_with_a_frontier_bound_that_bites(res):
    g, med = twin_topology(32, 64)
    x = rows_of(300, 64, np.float32)
    bounded = check_search(res, x, g, med, QIDS, queue_size=15)
    free = check_search(res, x, g, med, QIDS)
    assert not np.array_equal(bounded, free)


def test_search_kernel_when_every_distance_ties(res):
    g, med = twin_topology(32, 64)
    rng = np.random.default_rng(5)
    x = rng.integers(0, 2, (300, 3)).astype(np.float32)  # 8 distinct rows: the order is decided by the ids
    check_search(res, x, g, med, QIDS)
    check_search(res, x.astype(np.int8), g, med, QIDS, queue_size=15)


# ---------------------------------------------------------------- prune kernel
def gpu_prune(res, cp, x, graph, nodes, cand_ids, cand_d):
    xd = torch.from_numpy(x).cuda()
    gd, nd, cid = _dev_u32(graph), _dev_u32(nodes), _dev_u32(cand_ids)
    cdd = torch.from_numpy(np.ascontiguousarray(cand_d, dtype=np.float32)).cuda()
    out = torch.empty((len(nodes), cp.graph_degree), dtype=torch.int32, device="cuda")
    check(lib().cuvsAmdVamanaRobustPrune(res.get_c_obj(), cp._p, Tensor(xd).ptr, _u32(gd).ptr, _u32(nd).ptr, _u32(cid).ptr,
                                         Tensor(cdd).ptr, _u32(out).ptr))
    res.sync()
    return _host_u32(out)


def candidates(x, node, ids, V):
    """ids (any order) as a padded candidate row in (distance, id) order with the library's distances."""
    ids = np.asarray(ids, dtype=np.int64)
    d = ref.l2_to(x, ids, x[node].astype(np.float32))
    o = np.lexsort((ids, d))
    ci = np.full(V, INVALID, dtype=np.uint32)
    cd = np.full(V, ref.FLT_MAX, dtype=np.float32)
    ci[:len(ids)] = ids[o]
    cd[:len(ids)] = d[o]
    return ci, cd


def check_prune(res, x, graph, cases, **kw):
    """cases: (node, candidate ids). Returns the kernel's rows."""
    cp, rp = params_pair(**kw)
    nodes = np.array([c[0] for c in cases], dtype=np.uint32)
    rows = [candidates(x, n, ids, rp.visited) for n, ids in cases]
    got = gpu_prune(res, cp, x, graph, nodes, np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]))
    for r, (n, _) in enumerate(cases):
        want, _ = ref.robust_prune(x, graph[n], int(n), rows[r][0], rows[r][1], rp)
        assert np.array_equal(got[r], want), f"case {r} (node {n})"
    return got


def _distinct(rng, n, count, avoid):
    pool = np.setdiff1d(np.arange(n), np.asarray(list(avoid)))
    return rng.choice(pool, size=count, replace=False)


@pytest.mark.parametrize("alpha", [1.0, 1.2])
@pytest.mark.parametrize("dtype", [np.float32, np.int8], ids=["f32", "i8"])
def test_prune_kernel_equals_the_twin(res, alpha, dtype):
    n, D, V = 300, 32, 64
    rng = np.random.default_rng(11)
    x = rows_of(n, 33, dtype)
    x[200:220] = x[100:120]  # duplicate rows: d(accepted, k) = 0
    graph = np.full((n, D), INVALID, dtype=np.uint32)
    for i in range(n):
        k = [0, 5, 32][i % 3]
        graph[i, :k] = _distinct(rng, n, k, [i])
    cases = [
        (0, _distinct(rng, n, 10, [0])),                                   # empty adjacency, small pool: no pruning
        (1, _distinct(rng, n, 27, [1] + graph[1, :5].tolist())),           # a pool of exactly `degree` entries
        (4, _distinct(rng, n, 28, [4] + graph[4, :5].tolist())),           # one more than the degree: the smallest prune
        (2, _distinct(rng, n, 64, [2] + graph[2].tolist())),               # a pool of exactly degree + visited entries
        (5, np.concatenate([graph[5, :20], _distinct(rng, n, 30, [5] + graph[5].tolist())])),  # candidates that repeat edges
        (8, np.concatenate([[8], _distinct(rng, n, 50, [8] + graph[8].tolist())])),   # the node among its candidates
        (100, np.concatenate([np.arange(101, 120), np.arange(200, 220), _distinct(rng, 100, 20, [])])),  # duplicate rows
        (205, np.concatenate([[105], np.arange(100, 105), np.arange(206, 220), _distinct(rng, 100, 40, [])])),  # a twin at d = 0
        (7, []),                                                            # no candidates, five edges
        (3, []),                                                            # nothing at all
    ]
    got = check_prune(res, x, graph, cases, alpha=alpha)
    assert (got[0] != INVALID).sum() == 10 and (got[1] != INVALID).sum() == 32 and (got[9] == INVALID).all()
    # a different alpha gives a different row somewhere: the passes are really taken
    if alpha == 1.2:
        other = gpu_prune(res, vamana.IndexParams(alpha=1.0), x, graph, np.array([2], dtype=np.uint32),
                          *[a[None] for a in candidates(x, 2, cases[3][1], V)])
        assert not np.array_equal(other[0], got[3])


def test_prune_kernel_degree_256_visited_512(res):
    n, D, V = 600, 256, 512
    rng = np.random.default_rng(12)
    x = rows_of(n, 24, np.float32)
    graph = np.full((n, D), INVALID, dtype=np.uint32)
    for i in range(0, n, 2):
        graph[i] = _distinct(rng, n, D, [i])
    cases = [(0, _distinct(rng, n, 343, [0] + graph[0].tolist())),  # the whole pool: 599 = every other row
             (2, _distinct(rng, n, 300, [2])),
             (1, _distinct(rng, n, 512, [1])),
             (3, _distinct(rng, n, 100, [3]))]
    got = check_prune(res, x, graph, cases, graph_degree=D, visited_size=V)
    assert (got[3] != INVALID).sum() == 100


# ---------------------------------------------------------------- whole build
def gpu_build(x, device=True, **kw):
    cp = vamana.IndexParams(**kw)
    idx = vamana.build(cp, torch.from_numpy(x).cuda() if device else x)
    return idx, _host_u32(idx.graph), idx.medoid


@functools.lru_cache(maxsize=None)
def twin_build(n, dim, dtype, items):
    x = rows_of(n, dim, dtype)
    g, med = ref.build(x, ref.Params(**dict(items)))
    return x, g, med


BUILD_CASES = [
    (10, 3, np.float32, {}),                                               # max_batchsize 0 -> 1, n below the degree
    (33, 64, np.int8, {}),
    (33, 3, np.uint8, {"max_fraction": 1.0}),
    (300, 137, np.float32, {}),
    (300, 64, np.uint8, {"vamana_iters": 1.5, "max_fraction": 1.0}),
    (300, 64, np.int8, {"reverse_batchsize": 100, "max_fraction": 1.0}),   # several pieces of reverse destinations
    (300, 3, np.float32, {"visited_size": 100}),                           # rounded to 128
    (300, 137, np.uint8, {"vamana_iters": 1.5}),
    (300, 64, np.float32, {"graph_degree": 64, "visited_size": 128, "alpha": 1.0}),
    (1000, 64, np.float32, {}),
]


@pytest.mark.parametrize("n,dim,dtype,kw", BUILD_CASES,
                         ids=[f"{n}x{d}-{np.dtype(t).name}-{'-'.join(f'{k}={v}' for k, v in kw.items()) or 'defaults'}"
                              for n, d, t, kw in BUILD_CASES])
def test_build_equals_the_twin(n, dim, dtype, kw):
    x, want, med = twin_build(n, dim, dtype, tuple(sorted(kw.items())))
    idx, got, got_med = gpu_build(x, **kw)
    assert got_med == med
    assert np.array_equal(got, want), f"{(got != want).any(axis=1).sum()} rows differ"
    assert idx.trained and idx.dim == dim
    ref.check_graph(got, n, dim, kw.get("graph_degree", 32))


def test_build_from_the_host_and_twice_gives_the_same_bits():
    x, want, med = twin_build(300, 137, np.float32, ())
    _, a, ma = gpu_build(x, device=False)
    _, b, mb = gpu_build(x)
    assert ma == mb == med and np.array_equal(a, want) and np.array_equal(b, want)


def test_medoid_of_integer_rows_is_the_fp64_argmin():
    rng = np.random.default_rng(3)
    for dtype in (np.float32, np.int8, np.uint8):
        x = rng.integers(0, 100, (256, 20)).astype(dtype)
        x64 = x.astype(np.float64)
        d = ((x64 - x64.mean(axis=0)) ** 2).sum(axis=1)
        idx, _, med = gpu_build(x)
        assert med == int(np.argmin(d)) == ref.medoid(x)


# ---------------------------------------------------------------- the reference's own test (ann_vamana.cuh:131-247)
@pytest.mark.parametrize("degree", [32, 64, 128])
def test_graph_checks_and_recall_through_cagra(res, degree):
    n, dim = 1000, 64
    x = rows_of(n, dim, np.float32)
    q = np.random.default_rng(4321).normal(0.1, 2.0, (100, dim)).astype(np.float32)
    idx, g, med = gpu_build(x, graph_degree=degree, visited_size=2 * degree)
    max_degree, fraction = ref.check_graph(g, n, dim, degree)
    print(f"degree {degree}: max degree {max_degree}, edge fraction {fraction:.3f}")
    assert max_degree >= min(degree, dim)
    assert fraction > 0.75
    g0 = np.where(g == INVALID, 0, g).astype(np.uint32)  # the invalid edges replaced by node 0, as the reference does
    cidx = cagra.from_graph(_dev_u32(g0), torch.from_numpy(x).cuda(), resources=res)
    _, nb = cagra.search(cagra.SearchParams(itopk_size=64), cidx, torch.from_numpy(q).cuda(), 10, resources=res)
    res.sync()
    d = ((q.astype(np.float64)[:, None, :] - x.astype(np.float64)[None, :, :]) ** 2).sum(axis=2)
    truth = np.argsort(d, axis=1, kind="stable")[:, :10]
    r = ref.recall(_host_u32(nb).astype(np.int64), truth)
    print(f"degree {degree}: recall@10 through CAGRA {r:.4f}")
    assert r >= 0.2


# ---------------------------------------------------------------- files and the Python surface
@pytest.mark.parametrize("dtype,dim", [(np.float32, 137), (np.int8, 64), (np.float32, 1100)], ids=["f32", "i8", "f32-multisector"])
def test_files_equal_the_twin_writers(tmp_path, dtype, dim):
    x = rows_of(60, dim, dtype)
    idx, g, med = gpu_build(x, max_fraction=1.0)
    base = str(tmp_path / "v")
    vamana.save(base, idx)
    raw = open(base, "rb").read()
    assert raw == ref.index_bytes(g, med)
    size, max_degree, start, frozen = struct.unpack("<QIIQ", raw[:24])
    assert size == len(raw) and start == med and frozen == 0 and max_degree == (g != INVALID).sum(axis=1).max()
    assert open(base + ".data", "rb").read() == ref.data_bytes(x)
    base2 = str(tmp_path / "w")
    vamana.save(base2, idx, include_dataset=False)
    assert open(base2, "rb").read() == raw and not (tmp_path / "w.data").exists()
    base3 = str(tmp_path / "s")
    vamana.save(base3, idx, sector_aligned=True)
    disk = open(base3 + "_disk.index", "rb").read()
    assert disk == ref.disk_index_bytes(g, med, x)
    assert len(disk) % 4096 == 0 and struct.unpack("<Q", disk[8 + 8 * 8:8 + 9 * 8])[0] == len(disk)
    assert open(base3 + ".data", "rb").read() == ref.data_bytes(x)
    assert not (tmp_path / "s").exists()


def test_python_surface(tmp_path):
    x = rows_of(100, 16, np.float32)
    idx = vamana.build(vamana.IndexParams(graph_degree=32, visited_size=64), torch.from_numpy(x).cuda())
    assert idx.trained and idx.dim == 16 and 0 <= idx.medoid < 100
    g = idx.graph
    assert g.is_cuda and tuple(g.shape) == (100, 32) and g.dtype == torch.int32
    vamana.save(str(tmp_path / "p"), idx)
    assert (tmp_path / "p").exists() and (tmp_path / "p.data").exists()
    assert "trained=True" in repr(idx)
    for kw, text in (({"metric": "inner_product"}, "L2Expanded"), ({"graph_degree": 48}, "graph_degree"),
                     ({"visited_size": 32}, "visited_size"), ({"vamana_iters": 0.9}, "vamana_iters")):
        with pytest.raises(CuvsError, match=text):
            vamana.build(vamana.IndexParams(**kw), torch.from_numpy(x).cuda())
    with pytest.raises(CuvsError, match="Unsupported dataset DLtensor dtype"):
        vamana.build(vamana.IndexParams(), torch.from_numpy(x.astype(np.float16)).cuda())
    with pytest.raises(CuvsError, match="not built"):
        vamana.save(str(tmp_path / "q"), vamana.Index())
