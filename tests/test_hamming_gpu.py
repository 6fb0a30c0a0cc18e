"""GPU: BitwiseHamming (metric 20) in NN-descent and CAGRA over uint8 / int8 rows.

  1. NN-descent: the BitwiseHamming rows of the reference's table (golden/reference_test_tables.py NN_DESCENT_CASES,
     ann_nn_descent.cuh:466-477) on uint8 uniform [0, 5) and int8 uniform [-5, 5) rows (:164-173); pass = eval_neighbours
     recall >= 0.90 (eps 0.001) against the exact Hamming kNN graph, and the returned distances are the popcounts.
  2. CAGRA: the BitwiseHamming rows of ann_cagra.cuh:1521-1605 (uint8 uniform [1, 20), :200-205) without the rows the
     reference skips itself (IVF_PQ builds; k * dim * 8 / 5 < n_rows, :335-344), through a serialize / deserialize round trip;
     pass = recall >= 0.995 and distances equal to the popcounts. The reference's refusals of IVF_PQ and float rows.
  3. Walk parity: squared L2 over the rows expanded to 0/1 floats IS the Hamming distance, and every sum in it is an exact
     integer, so a Hamming walk and an sqeuclidean walk over the expanded rows on the same graph must agree bit for bit -
     and the single-wave walk with the CPU oracle (oracle_cagra.c) too.
  4. The exact kNN graph of ITERATIVE_CAGRA_SEARCH / AUTO: exact distances, tie-aware equal to torch's exact kNN.
  5. End to end: float corpus -> train(MEAN) -> transform -> CAGRA Hamming build -> search, plus extend, merge, filter.
  6. Brute force, IVF-Flat, IVF-PQ and pairwise distance still refuse bitwise_hamming."""
import math

import numpy as np
import pytest

from tests.golden import reference_test_tables as T
from tests.test_reference_tables_gpu import _eval_neighbours

pytestmark = pytest.mark.gpu

HAM = "bitwise_hamming"


def _bits(x):
    """uint8 / int8 rows [n, d] (torch, device) -> [n, 8 d] float64 0/1 (bit j of byte b -> column 8 b + j)"""
    import torch

    u = x.view(torch.uint8).to(torch.int32)
    shifts = torch.arange(8, device=x.device, dtype=torch.int32)
    return ((u[:, :, None] >> shifts) & 1).reshape(x.shape[0], -1).double()


def _hamming(q, x):
    """exact Hamming distances [m, n] (float64) of the byte rows of q and x, as a 0/1 matmul (exact integers)"""
    bq, bx = _bits(q), _bits(x)
    return bq.sum(1)[:, None] + bx.sum(1)[None, :] - 2.0 * (bq @ bx.T)


def _exact_knn(q, x, k):
    import torch

    d = _hamming(q, x)
    v, i = torch.topk(d, k, dim=1, largest=False)
    return v.float(), i


def _pair_popcounts(q, x, ids):
    """popcount(q[r] ^ x[ids[r, j]]) for every returned id (ids int64, device)"""
    import torch

    rows = x[ids.clamp(0, x.shape[0] - 1)].view(torch.uint8)
    xo = (rows ^ q.view(torch.uint8)[:, None, :]).to(torch.int32)
    shifts = torch.arange(8, device=q.device, dtype=torch.int32)
    return ((xo[..., None] >> shifts) & 1).sum(dim=(2, 3)).float()


def _ids64(i):
    import torch

    return i.to(torch.int64) & 0xFFFFFFFF if i.dtype != torch.int64 else i


def _randint(shape, lo, hi, dtype, seed):
    import torch

    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return torch.randint(lo, hi, shape, generator=g, device="cuda", dtype=torch.int32).to(dtype)


# ----------------------------------------------------------------------------------------------------- 1. NN-descent
def _nnd_params():
    out = []
    for n, c in enumerate(T.NN_DESCENT_CASES):
        if c[3] != HAM:
            continue
        for dt in ("u8", "i8"):
            out.append(pytest.param(c, dt, id=f"{dt}-{n:03d}-n{c[0]}-d{c[1]}-deg{c[2]}-{'host' if c[4] else 'device'}"))
    return out


@pytest.mark.parametrize("case,dt", _nnd_params())
def test_nn_descent_reference_rows(case, dt, res):
    import torch
    from cuvs_amd.neighbors import nn_descent

    n, dim, degree, metric, host, min_recall = case
    x = _randint((n, dim), 0, 5, torch.uint8, 1234) if dt == "u8" else _randint((n, dim), -5, 5, torch.int8, 1234)
    index = nn_descent.build(nn_descent.IndexParams(metric=metric, graph_degree=degree, intermediate_graph_degree=2 * degree,
                                                    max_iterations=100), x.cpu().numpy() if host else x, resources=res)
    graph = _ids64(index.graph)
    dist = index.distances
    td, ti = _exact_knn(x, x, degree)   # the exact kNN graph, self included (as in the reference)
    _eval_neighbours(ti, graph, td, dist, 0.001, min_recall, test_unique=False)
    assert torch.equal(dist, _pair_popcounts(x, x, graph))


def test_nn_descent_refuses_float_rows(res):
    import torch
    from cuvs_amd._lib import CuvsError
    from cuvs_amd.neighbors import nn_descent

    x = torch.rand((500, 16), device="cuda")
    with pytest.raises(CuvsError, match="Data type needs to be int8 or uint8 for NN Descent to run with BitwiseHamming"):
        nn_descent.build(nn_descent.IndexParams(metric=HAM, graph_degree=32, intermediate_graph_degree=64), x, resources=res)


# -------------------------------------------------------------------------------------------------- 2. CAGRA table
def _cagra_rows():
    rows = []
    # ann_cagra.cuh:1521-1547 "Varying dim and build algo": {100 queries} x {1000 rows} x dim x {k 16} x {IVF_PQ, NN_DESCENT,
    # ITERATIVE_CAGRA_SEARCH} x {AUTO} x {max_queries 10} x {team 0} x {itopk 64} x {width 1} x metrics x {host false} x
    # {include_serialized_dataset true} x {source indices false} x {0.995}
    for dim in (1, 3, 5, 7, 8, 17, 64, 128, 137, 192, 256, 512, 1024):
        for build in ("ivf_pq", "nn_descent", "iterative_cagra_search"):
            rows.append(dict(line=1523, dim=dim, build=build, team=0, include=True))
    # :1549-1575 "Varying team_size, graph_build_algo": dim 64, team 0, include_serialized_dataset false
    for build in ("ivf_pq", "nn_descent", "iterative_cagra_search"):
        rows.append(dict(line=1551, dim=64, build=build, team=0, include=False))
    # :1577-1603 "Vary team size only": dim 64, NN_DESCENT, team {8, 16, 32}, include_serialized_dataset false
    for team in (8, 16, 32):
        rows.append(dict(line=1579, dim=64, build="nn_descent", team=team, include=False))
    n_rows, k = 1000, 16
    # the reference's own skips (:335-344): IVF_PQ builds, and k * dim * 8 / 5 < n_rows (too many ties for a ground truth)
    return [r for r in rows if r["build"] != "ivf_pq" and not (k * r["dim"] * 8 // 5 < n_rows)]


@pytest.mark.parametrize("c", [pytest.param(r, id=f"l{r['line']}-d{r['dim']}-{r['build']}-team{r['team']}-{'ds' if r['include'] else 'nods'}")
                               for r in _cagra_rows()])
def test_cagra_reference_rows(c, res, tmp_path):
    import torch
    from cuvs_amd.neighbors import cagra

    x = _randint((1000, c["dim"]), 1, 20, torch.uint8, 1234)
    q = _randint((100, c["dim"]), 1, 20, torch.uint8, 4321)
    index = cagra.build(cagra.IndexParams(metric=HAM, build_algo=c["build"]), x, resources=res)
    fn = str(tmp_path / "cagra_ham.bin")
    cagra.save(fn, index, include_dataset=c["include"], resources=res)
    index = cagra.load(fn, resources=res)
    if not c["include"]:  # update_dataset (:456-460): the loaded graph with the caller's rows
        index = cagra.from_graph(index.graph, x, metric=HAM, resources=res)
    sp = cagra.SearchParams(algo="auto", max_queries=10, team_size=c["team"], itopk_size=64)
    d, i = cagra.search(sp, index, q, 16, resources=res)
    res.sync()
    ii = _ids64(i)
    td, ti = _exact_knn(q, x, 16)
    _eval_neighbours(ti, ii, td, d, 0.001, 0.995)
    assert torch.equal(d, _pair_popcounts(q, x, ii))


def test_cagra_refusals(res):
    import torch
    from cuvs_amd._lib import CuvsError
    from cuvs_amd.neighbors import cagra

    x = _randint((1000, 64), 1, 20, torch.uint8, 1)
    with pytest.raises(CuvsError, match="IVF_PQ for CAGRA graph build does not support BitwiseHamming"):
        cagra.build(cagra.IndexParams(metric=HAM, build_algo="ivf_pq"), x, resources=res)
    for b in ("nn_descent", "iterative_cagra_search"):
        with pytest.raises(CuvsError, match="BitwiseHamming distance is only supported for int8_t and uint8_t"):
            cagra.build(cagra.IndexParams(metric=HAM, build_algo=b), x.float(), resources=res)
    # a Hamming index over float rows cannot be searched; hnswlib has no Hamming space
    g = cagra.build(cagra.IndexParams(metric=HAM, build_algo="iterative_cagra_search", graph_degree=32,
                                      intermediate_graph_degree=64), x, resources=res)
    bad = cagra.from_graph(g.graph, x.float(), metric=HAM, resources=res)
    with pytest.raises(CuvsError, match="only supported for int8_t and uint8_t"):
        cagra.search(cagra.SearchParams(), bad, x[:4].float(), 4, resources=res)
    from cuvs_amd._lib import check, lib
    import ctypes as C

    with pytest.raises(CuvsError, match="hnswlib"):
        check(lib().cuvsCagraSerializeToHnswlib(res.get_c_obj(), C.c_char_p(b"/dev/null"), g._p))


# ------------------------------------------------------------------------------------------------- 3. walk parity
def _filter_words(n, seed):
    import torch

    keep = np.random.default_rng(seed).random(n) < 0.7
    words = np.zeros((n + 31) // 32, np.uint32)
    for r in np.nonzero(keep)[0]:
        words[r >> 5] |= np.uint32(1 << (r & 31))
    return torch.from_numpy(words.view(np.int32)).cuda(), words, keep


@pytest.mark.parametrize("filtered", [False, True])
@pytest.mark.parametrize("dim", [16, 37, 64])
def test_walk_parity_with_expanded_rows(dim, filtered, res):
    import torch
    import oracle
    from cuvs_amd._lib import BITSET
    from cuvs_amd.neighbors import cagra

    n, nq, k = 3000, 2048, 10
    x = _randint((n, dim), 0, 256, torch.uint8, 11 + dim)
    q = _randint((nq, dim), 0, 256, torch.uint8, 12 + dim)
    xf, qf = _bits(x).float().contiguous(), _bits(q).float().contiguous()
    g = cagra.build(cagra.IndexParams(metric=HAM, build_algo="iterative_cagra_search", graph_degree=32,
                                      intermediate_graph_degree=64), x, resources=res).graph
    ham = cagra.from_graph(g, x, metric=HAM, resources=res)
    l2 = cagra.from_graph(g, xf, metric="sqeuclidean", resources=res)
    fw, words, keep = _filter_words(n, dim) if filtered else (None, None, None)
    flt = (fw, BITSET) if filtered else None
    # single-wave walk: Hamming == expanded-row walk == CPU oracle
    sp = cagra.SearchParams(algo="single_cta", itopk_size=64)
    dh, ih = cagra.search(sp, ham, q, k, resources=res, filter=flt)
    dl, il = cagra.search(sp, l2, qf, k, resources=res, filter=flt)
    res.sync()
    assert torch.equal(ih, il) and torch.equal(dh, dl)
    od, oi = oracle.cagra_search(xf.cpu().numpy(), g.cpu().numpy().view(np.uint32), qf.cpu().numpy(), k, itopk_size=64,
                                 filter_words=words)
    assert np.array_equal(_ids64(ih).cpu().numpy(), oi) and np.array_equal(dh.cpu().numpy(), od)
    # multi-wave walk. Unfiltered: one wave per query (itopk 32, width 1, a batch that fills the GPU) makes the walk
    # deterministic, so the two walks agree bit for bit. Filtered: the plan widens itopk to 64 for any filter
    # (search_plan.cuh:220-228), i.e. two waves per query that race for parents (as the reference's MULTI_CTA CTAs do), so not
    # even one walk is reproducible - there the two walks must agree in quality, and the Hamming walk must be exact and filtered.
    sp = cagra.SearchParams(algo="multi_cta", itopk_size=32, search_width=1)
    dh, ih = cagra.search(sp, ham, q, k, resources=res, filter=flt)
    dl, il = cagra.search(sp, l2, qf, k, resources=res, filter=flt)
    res.sync()
    assert torch.equal(dh, _pair_popcounts(q, x, _ids64(ih)))
    if not filtered:
        assert torch.equal(ih, il) and torch.equal(dh, dl)
    else:
        got = _ids64(ih).cpu().numpy()
        assert (got < n).all() and keep[got].all()
        assert abs(dh.double().mean().item() - dl.double().mean().item()) <= 0.01 * dl.double().mean().item()


# ---------------------------------------------------------------------------------------------- 4. exact kNN graph
@pytest.mark.parametrize("build", ["iterative_cagra_search", "auto"])
@pytest.mark.parametrize("dim,dt", [(8, "u8"), (31, "i8"), (128, "u8")])
def test_exact_knn_graph(dim, dt, build, res):
    import torch
    from cuvs_amd.neighbors import cagra

    n, K = 2500, 48
    x = _randint((n, dim), 0, 256, torch.uint8, 7) if dt == "u8" else _randint((n, dim), -128, 128, torch.int8, 7)
    knn = _ids64(cagra.build_knn_graph(cagra.IndexParams(metric=HAM, build_algo=build, intermediate_graph_degree=K), x, K,
                                       resources=res))
    res.sync()
    assert (knn < n).all()
    assert not (knn == torch.arange(n, device="cuda")[:, None]).any()
    s = torch.sort(knn, dim=1).values
    assert not (s[:, 1:] == s[:, :-1]).any()
    d = _hamming(x, x)
    d.fill_diagonal_(math.inf)
    exact = torch.sort(d, dim=1).values[:, :K]
    got = torch.gather(d, 1, knn)
    assert torch.equal(got, _pair_popcounts(x, x, knn).double())   # the 0/1 matmul and the popcounts agree
    assert torch.equal(torch.sort(got, dim=1).values, exact)       # tie-aware: the K smallest distances of every row


# -------------------------------------------------------------------------------------------------- 5. end to end
E2E_MIN_RECALL = 0.95  # measured once: 0.972 (itopk 128); merged index: same threshold


def _clustered(n, dim, seed):
    import torch

    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    centers = torch.randn((64, dim), generator=g, device="cuda") * 2.0
    lab = torch.randint(0, 64, (n,), generator=g, device="cuda")
    return centers[lab] + torch.randn((n, dim), generator=g, device="cuda")


def _tie_aware_recall(d, i, q, x, k):
    """share of returned rows whose exact distance is within the k-th exact distance (distances checked exact first)"""
    import torch

    ii = _ids64(i)
    assert torch.equal(d, _pair_popcounts(q, x, ii))
    td, _ = _exact_knn(q, x, k)
    return float(((d <= td[:, -1:]) & (ii >= 0) & (ii < x.shape[0])).float().mean().item())


def test_end_to_end_quantize_build_search_extend_merge_filter(res):
    import torch
    from cuvs_amd._lib import BITSET
    from cuvs_amd.neighbors import cagra
    from cuvs_amd.preprocessing.quantize import binary

    n, dim, nq, k = 100000, 512, 1000, 10
    xf = _clustered(n + 2000 + nq, dim, 3)
    qz = binary.train(binary.QuantizerParams(threshold="mean"), xf[:n], resources=res)
    codes = binary.transform(xf, quantizer=qz, resources=res)
    res.sync()
    x, extra, q = codes[:n].contiguous(), codes[n:n + 2000].contiguous(), codes[n + 2000:].contiguous()
    assert x.shape == (n, dim // 8) and x.dtype == torch.uint8
    index = cagra.build(cagra.IndexParams(metric=HAM, build_algo="auto"), x, resources=res)
    sp = cagra.SearchParams(itopk_size=128)
    d, i = cagra.search(sp, index, q, k, resources=res)
    res.sync()
    recall = _tie_aware_recall(d, i, q, x, k)
    print(f"end-to-end tie-aware recall@{k}: {recall:.4f}")
    assert recall >= E2E_MIN_RECALL
    # extend: every new row finds itself (distance 0)
    cagra.extend(index, extra, resources=res)
    assert len(index) == n + 2000
    # (on these codes the walk misses an exact match now and then for the index's own rows as well: measured shares of self
    # queries at distance 0, new rows / first 2000 old rows: itopk 64: 0.860 / 0.879, 128: 0.911 / 0.924, 256: 0.982 / 1.000)
    d, i = cagra.search(cagra.SearchParams(itopk_size=256), index, extra, 1, resources=res)
    res.sync()
    assert (d[:, 0] == 0).float().mean().item() >= 0.95
    # merge of two Hamming indexes searches the concatenation
    half = n // 2
    a = cagra.build(cagra.IndexParams(metric=HAM, build_algo="auto"), x[:half].contiguous(), resources=res)
    b = cagra.build(cagra.IndexParams(metric=HAM, build_algo="auto"), x[half:].contiguous(), resources=res)
    merged = cagra.merge(cagra.IndexParams(metric=HAM, build_algo="auto"), [a, b], resources=res)
    assert len(merged) == n
    d, i = cagra.search(sp, merged, q, k, resources=res)
    res.sync()
    assert _tie_aware_recall(d, i, q, x, k) >= E2E_MIN_RECALL
    # a filtered search never returns a removed row
    fw, _, keep = _filter_words(n, 9)
    d, i = cagra.search(sp, merged, q, k, resources=res, filter=(fw, BITSET))
    res.sync()
    got = _ids64(i).cpu().numpy()
    assert (got < n).all() and keep[got].all()


# ------------------------------------------------------------------------------------------- 6. unchanged refusals
def test_other_indexes_still_refuse_bitwise_hamming(res):
    import torch
    from cuvs_amd._lib import CuvsError
    from cuvs_amd.distance import pairwise_distance
    from cuvs_amd.neighbors import brute_force, ivf_flat, ivf_pq

    x8 = _randint((2000, 32), 0, 256, torch.uint8, 5)
    xf = x8.float()
    for x in (x8, xf):
        with pytest.raises(CuvsError):
            brute_force.build(x, metric=HAM, resources=res)
        with pytest.raises(CuvsError):
            ivf_flat.build(ivf_flat.IndexParams(n_lists=16, metric=HAM), x, resources=res)
        with pytest.raises(CuvsError):
            ivf_pq.build(ivf_pq.IndexParams(n_lists=16, pq_dim=16, metric=HAM), x, resources=res)
    with pytest.raises(CuvsError):
        pairwise_distance(xf[:10], xf[:20], metric=HAM)
