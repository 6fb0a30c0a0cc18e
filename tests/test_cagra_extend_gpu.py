"""GPU: cuvsCagraExtend against its numpy twin (tests/cagra_extend_ref.py, restated from the reference's add_nodes.cuh), graph
for graph. The walk of the twin is oracle.cagra_search, the bit-exact twin of the single-workgroup walk, and everything after the
walk is integer bookkeeping, so the graphs are compared element for element. Base graphs are exact kNN graphs handed to
cagra.from_graph, so nothing but extend is under test. cuvsCagraMerge is pinned to cagra.build on the concatenated rows."""
import numpy as np
import pytest

import oracle
from tests import cagra_extend_ref as ref

pytestmark = pytest.mark.gpu


def _index(x0, graph0, metric):
    import torch
    from cuvs_amd.neighbors import cagra

    g = torch.from_numpy(np.ascontiguousarray(graph0).view(np.int32).copy()).cuda()
    return cagra.from_graph(g, torch.from_numpy(x0.copy()).cuda(), metric=metric)


def _graph(index):
    import torch

    g = index.graph.cpu().numpy().view(np.uint32).copy()
    torch.cuda.synchronize()
    return g


def _extend(index, new_rows, chunk, host=False):
    import torch
    from cuvs_amd.neighbors import cagra

    cagra.extend(index, new_rows.copy() if host else torch.from_numpy(new_rows.copy()).cuda(), max_chunk_size=chunk)
    torch.cuda.synchronize()


def _assert_equal(got, want, what):
    assert got.shape == want.shape, f"{what}: graph {got.shape}, twin {want.shape}"
    bad = np.nonzero((got != want).any(1))[0]
    print(f"{what}: rows that differ from the twin: {bad.size} of {got.shape[0]}" + (f", first {bad[0]}" if bad.size else ""))
    assert bad.size == 0, f"{what}: {bad.size} rows differ from the twin, first {bad[0]}: {got[bad[0]]} != {want[bad[0]]}"


@pytest.mark.parametrize("case", ref.SHAPES + ref.DTYPES + ref.METRICS, ids=ref.case_id)
def test_extend_matches_twin(case):
    n0, m, dim, degree, chunk, dtype, metric = case
    x, g0 = ref.inputs(case)
    index = _index(x[:n0], g0, metric)
    _extend(index, x[n0:], chunk)
    assert len(index) == n0 + m and index.graph_degree == degree
    _assert_equal(_graph(index), ref.twin(case), ref.case_id(case))


def test_walk_of_extend_matches_oracle():
    """the walk extend runs (single workgroup, itopk max(4 degree, 256), k = 2 degree), on its own: a difference between the
    device walk and the oracle shows here before it shows as a different graph"""
    import torch
    from cuvs_amd.neighbors import cagra

    for case in (ref.SHAPES[1], ref.SHAPES[2]):
        n0, m, dim, degree, chunk, dtype, metric = case
        x, g0 = ref.inputs(case)
        index = _index(x[:n0], g0, metric)
        k = min(2 * degree, n0)
        d, i = cagra.search(cagra.SearchParams(algo="single_cta", **ref.search_params(degree)), index,
                            torch.from_numpy(x[n0:].copy()).cuda(), k)
        torch.cuda.synchronize()
        od, oi = oracle.cagra_search(x[:n0], g0, x[n0:], k, metric=metric, **ref.search_params(degree))
        gi = i.cpu().numpy().view(np.uint32)
        gi = np.where(gi == ref.INVALID, -1, gi.astype(np.int64))
        print(f"{ref.case_id(case)}: id mismatch rate {(gi != oi).mean():.4f}, padded {(oi < 0).mean():.4f}")
        assert (gi == oi).all() and (d.cpu().numpy() == od).all()


def test_repeated_calls():
    """20 calls of 25 rows, the incremental use extend exists for: the graph of the twin applied 20 times, and no added row is
    left without an incoming edge (a later call must not take away the reverse edges of an earlier one: a row without any is
    reached through a random seed only)"""
    case, calls = ref.REPEATED, ref.REPEATED_CALLS
    n0, m, dim, degree, chunk, dtype, metric = case
    x, g0 = ref.inputs(case, calls)
    index = _index(x[:n0], g0, metric)
    for c in range(calls):
        _extend(index, x[n0 + c * m:n0 + (c + 1) * m], chunk)
    assert len(index) == n0 + calls * m
    got = _graph(index)
    indeg = ref.in_degree(got)
    print(f"repeated calls: added rows with in-degree 0: {(indeg[n0:] == 0).sum()} of {calls * m}, min {indeg[n0:].min()}")
    _assert_equal(got, ref.twin(case, calls), "repeated calls")
    assert (indeg[n0:] >= 1).all()


def test_host_rows_give_the_same_graph():
    case = ref.SHAPES[1]
    n0, m, dim, degree, chunk, dtype, metric = case
    x, g0 = ref.inputs(case)
    index = _index(x[:n0], g0, metric)
    _extend(index, x[n0:], chunk, host=True)
    assert len(index) == n0 + m
    _assert_equal(_graph(index), ref.twin(case), "host rows")


def test_no_rows_added():
    import torch
    from cuvs_amd.neighbors import cagra

    case = ref.SHAPES[0]
    n0, m, dim, degree, chunk, dtype, metric = case
    x, g0 = ref.inputs(case)
    index = _index(x[:n0], g0, metric)
    cagra.extend(index, torch.empty((0, dim), dtype=torch.float32, device="cuda"))
    assert len(index) == n0
    assert (_graph(index) == g0).all()


def test_failed_extend_leaves_the_index_as_it_was():
    """Ten rows under a degree-16 graph (every list repeats ids): an added row finds at most ten distinct rows, fewer than its
    list needs, which add_nodes.cuh:266-271 refuses. The index keeps its rows, its graph and its answers."""
    import torch
    from cuvs_amd._lib import CuvsError
    from cuvs_amd.neighbors import cagra

    x = ref.rows(15, 8, ref.F32, 77)
    g0 = np.array([[(r + 1 + j % 9) % 10 for j in range(16)] for r in range(10)], np.uint32)
    index = _index(x[:10], g0, ref.SQ)
    with pytest.raises(ValueError, match="Number of edges is not enough"):
        ref.extend_twin(x, g0, 10, 16, ref.SQ, 0)
    with pytest.raises(CuvsError, match="Number of edges is not enough"):
        cagra.extend(index, torch.from_numpy(x[10:].copy()).cuda())
    assert len(index) == 10
    assert (_graph(index) == g0).all()
    d, i = cagra.search(cagra.SearchParams(itopk_size=64, algo="single_cta"), index, torch.from_numpy(x[10:].copy()).cuda(), 5)
    torch.cuda.synchronize()
    od, oi = oracle.cagra_search(x[:10], g0, x[10:], 5, itopk_size=64)
    assert (i.cpu().numpy().view(np.uint32).astype(np.int64) == oi).all() and (d.cpu().numpy() == od).all()


def test_merge_equals_build_on_the_concatenated_rows():
    import torch
    from cuvs_amd.neighbors import cagra

    x = ref.rows(657, 24, ref.F32, 41)
    p = cagra.IndexParams(intermediate_graph_degree=32, graph_degree=16)
    parts = [cagra.build(p, torch.from_numpy(x[a:b].copy()).cuda()) for a, b in ((0, 300), (300, 500), (500, 657))]
    merged = cagra.merge(p, parts)
    whole = cagra.build(p, torch.from_numpy(x.copy()).cuda())
    assert len(merged) == 657 and merged.graph_degree == 16
    gm, gw = _graph(merged), _graph(whole)
    assert gm.shape == (657, 16) and (gm == gw).all(), f"{(gm != gw).any(1).sum()} rows differ"
    # ... and it is a graph over all the rows: edges cross the parts in both directions
    assert (gm[:300] >= 300).any() and (gm[500:] < 300).any()
