"""CPU: the numpy twin of cuvsCagraExtend (tests/cagra_extend_ref.py) against graphs written out by hand from the rules of the
reference's add_nodes.cuh, and the properties of the graphs it gives over the inputs of tests/test_cagra_extend_gpu.py."""
import numpy as np
import pytest

from tests import cagra_extend_ref as ref

INV = ref.INVALID


def _table_search(table):
    """a walk whose results are given: table[first element of the query] -> ids, nearest first"""

    def search(dataset, graph, queries, k, itopk_size=None, metric=None):
        assert itopk_size == 256 and metric == ref.SQ
        ids = np.array([table[int(q[0])][:k] for q in queries], np.int64)
        return np.zeros(ids.shape, np.float32), ids

    return search


def test_worked_example():
    """Degree 4, six rows, two rows added in one chunk. K = 8 candidates of which the six-row graph can give six, so two
    columns are invalid.

    Incoming counts of the starting graph: ids 0..5 -> 5 5 4 4 3 3.

    Row 6, walk 2 4 0 5 1 3: detour counts 0 1 2 1 4 4 (e.g. 4 is listed by 2; 0 by 2 and 4; 5 by 4 only), invalid 9 9. The stable
    sort keeps 4 ahead of 5 (both 1): rank list 2 4 5 0. Target 2 = [0 1 3 4]: slot 3 holds 4 (3 incoming), slot 2 holds 3 (4
    incoming, strictly more) -> slot 2 becomes 6, 3 is evicted. Target 4 = [0 2 5 1]: slot 3 holds 1 (5), slot 2 holds 5 (3) ->
    slot 3 becomes 6, 1 is evicted. Interleaved 2 | 3 | 4 | 1.

    Row 7, walk 4 2 5 3 0 1 over the SAME starting graph: counts 0 1 1 2 4 5, rank list 4 2 5 3. The reverse edges see row 6's:
    target 4 = [0 2 5 6]: slot 3 holds 6 (2 incoming, set when row 6 was added), slot 2 holds 5 (3) -> slot 2 becomes 7, 5
    evicted. Target 2 = [0 1 6 4]: slot 3 holds 4 (3), slot 2 holds 6 (2) -> slot 3 becomes 7, 4 evicted. Interleaved: 4 | 5 |
    2 (4 repeats) | evicted 5 and 4 both repeat, list exhausted | 3 (2 and 5 repeat)."""
    graph0 = np.array([[1, 2, 3, 4], [0, 2, 3, 5], [0, 1, 3, 4], [0, 1, 2, 5], [0, 2, 5, 1], [1, 3, 4, 0]], np.uint32)
    x = np.arange(8, dtype=np.float32)[:, None] * np.ones((1, 2), np.float32)  # row r = (r, r): the table is keyed by r
    table = {6: [2, 4, 0, 5, 1, 3], 7: [4, 2, 5, 3, 0, 1]}
    got = ref.extend_twin(x, graph0, 6, 4, ref.SQ, 0, search=_table_search(table))
    want = np.array([[1, 2, 3, 4], [0, 2, 3, 5], [0, 1, 6, 7], [0, 1, 2, 5], [0, 2, 7, 6], [1, 3, 4, 0],
                     [2, 3, 4, 1], [4, 5, 2, 3]], np.uint32)
    assert got.dtype == np.uint32 and (got == want).all(), got


def test_worked_example_in_chunks_of_one():
    """The same rows a chunk each. Row 6 as above. Row 7's walk now runs over seven rows, and both the detour counts and the
    incoming counts are taken from the seven-row graph: ids 0..6 -> 5 5 5 4 4 3 2.

    Walk 4 2 6 5 3 0 1: 2 is listed by 4 = [0 2 5 6]: 1; 6 by 4 and 2 = [0 1 6 4]: 2; 5 by 4 only: 1; 3 by 6 = [2 3 4 1] and
    5: 2; 0 by 4, 2, 5, 3: 4; 1 by 2, 6, 5, 3, 0: 5; invalid 9 -> stable order 4 2 5 6 3 0 1, rank list 4 2 5 6. Target 4: slot
    3 holds 6 (2), slot 2 holds 5 (3) -> slot 2 becomes 7, 5 evicted. Target 2: slot 3 holds 4 (4), slot 2 holds 6 (2) -> slot
    3 becomes 7, 4 evicted. Interleaved 4 | 5 | 2 | - | 6: the row lists row 6, which the one-chunk graph cannot."""
    graph0 = np.array([[1, 2, 3, 4], [0, 2, 3, 5], [0, 1, 3, 4], [0, 1, 2, 5], [0, 2, 5, 1], [1, 3, 4, 0]], np.uint32)
    x = np.arange(8, dtype=np.float32)[:, None] * np.ones((1, 2), np.float32)
    table = {6: [2, 4, 0, 5, 1, 3], 7: [4, 2, 6, 5, 3, 0, 1]}
    got = ref.extend_twin(x, graph0, 6, 4, ref.SQ, 1, search=_table_search(table))
    want = np.array([[1, 2, 3, 4], [0, 2, 3, 5], [0, 1, 6, 7], [0, 1, 2, 5], [0, 2, 7, 6], [1, 3, 4, 0],
                     [2, 3, 4, 1], [4, 5, 2, 6]], np.uint32)
    assert (got == want).all(), got


def test_reverse_edge_rule_skips_taken_ids_and_falls_back_to_slot_0():
    """add_nodes.cuh:203-231 with counts given by hand. Target 0 = [4 5 6 7]: 7 has 9 incoming edges, 6 has 2 -> slot 3, 7
    evicted. Target 1 = [4 5 8 7]: 7 is taken for this row already and 8 has no incoming edge (not strictly more than 0), so the
    defaults hold: slot 0 is overwritten and the evicted id is n_new = 10, which the interleaving skips: 0 | 7 | 1 | - | 2."""
    graph = np.array([[4, 5, 6, 7], [4, 5, 8, 7], [0, 1, 3, 4], [0, 1, 2, 4], [0, 1, 2, 3], [0, 1, 2, 3], [0, 1, 2, 3],
                      [0, 1, 2, 3], [0, 1, 2, 3], [INV] * 4], np.uint32)
    incoming = np.array([1, 1, 1, 1, 1, 1, 2, 9, 0, 0], np.int64)
    ref.add_row(graph, incoming, 9, np.array([0, 1, 2, 3]), 10, 4)
    assert graph[0].tolist() == [4, 5, 6, 9] and graph[1].tolist() == [9, 5, 8, 7]
    assert graph[9].tolist() == [0, 7, 1, 2]
    assert incoming[9] == 2 and incoming[7] == 9  # only the new row's count changes


def test_too_few_valid_candidates_is_an_error():
    """degree 4 over three rows: the walk gives three ids, the rank list's fourth entry is invalid and the two evicted ids
    repeat entries of the rank list: three edges, which add_nodes.cuh:266-271 refuses"""
    graph0 = np.array([[1, 2, 1, 2], [0, 2, 0, 2], [0, 1, 0, 1]], np.uint32)
    x = np.arange(4, dtype=np.float32)[:, None] * np.ones((1, 2), np.float32)
    with pytest.raises(ValueError, match="Number of edges is not enough"):
        ref.extend_twin(x, graph0, 3, 4, ref.SQ, 0, search=_table_search({3: [0, 1, 2]}))


def test_no_rows_added():
    x, g = ref.inputs(ref.SHAPES[0])
    got = ref.extend_twin(x[:600], g, 600, 16, ref.SQ, 0)
    assert got.shape == (600, 16) and (got == g).all()


# ------------------------------------------------------------------ properties over the GPU tests' inputs
ALL = [(c, 1) for c in ref.SHAPES + ref.DTYPES + ref.METRICS] + [(ref.REPEATED, ref.REPEATED_CALLS)]


@pytest.mark.parametrize("case,calls", ALL, ids=lambda v: ref.case_id(v) if isinstance(v, tuple) else str(v))
def test_graph_properties(case, calls):
    n0, m, dim, degree, chunk, dtype, metric = case
    n_total = n0 + calls * m
    g = ref.twin(case, calls).astype(np.int64)
    assert g.shape == (n_total, degree)
    assert (g < n_total).all(), "an id outside the graph"
    assert (g != np.arange(n_total)[:, None]).all(), "a self edge"
    s = np.sort(g, axis=1)
    assert (s[:, 1:] != s[:, :-1]).all(), "a duplicate edge"
    indeg = ref.in_degree(g)
    print(f"{ref.case_id(case)} x{calls}: added rows with in-degree 0: {(indeg[n0:] == 0).sum()}, min {indeg[n0:].min()}")
    assert (indeg[n0:] >= 1).all(), "an added row without an incoming edge"
    assert (g[:n0] >= n0).any() and (g[:n0] != ref.inputs(case, calls)[1]).any()  # (reverse edges were placed)


def test_chunks_link_to_earlier_chunks():
    case = ref.SHAPES[1]
    n0, m, _, _, chunk, _, _ = case
    g = ref.twin(case).astype(np.int64)
    assert (g[n0 + chunk:] >= n0).any(), "no row of a later chunk lists a row added before it"
    first = g[n0:n0 + chunk]
    assert (first >= n0 + chunk).any(), "no row of the first chunk was given a reverse edge by a later chunk"
