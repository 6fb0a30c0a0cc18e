"""Numpy restatement of cuvsCagraExtend (cuvs_amd/csrc/cagra.hip cagra_extend), which restates the reference's
cpp/src/neighbors/detail/cagra/add_nodes.cuh:24-344. Every decision the library takes is taken here by the same rule, so the
graphs are compared element for element.

Per chunk of added rows (add_graph_nodes, :297-343):
  0. incoming-edge counts = histogram of the graph the chunk starts from (:40-53)
  1. a walk for the 2 * degree nearest rows of every added row (:69-70, :96-121)
  2. re-ordering of these candidates by detour count (:148-189)
  3. reverse edges, row after row, and the row's own list interleaved from the rank list and the evicted ids (:191-275)

Two places where the reference leaves the result open and this project fixes it:
  * the walk is the single-workgroup walk (SINGLE_CTA). The reference passes default search parameters, whose AUTO may pick
    the multi-CTA walk; that walk races for parents and is not reproducible, so neither the library nor this twin uses it.
  * step 2 sorts with std::sort (:179-183), which leaves the order of equal detour counts unspecified. Here the sort is
    stable: equal counts keep the order of the walk's results (nearest first)."""
import numpy as np

import oracle

INVALID = 0xFFFFFFFF


def search_params(degree):
    """the walk of step 1: itopk_size = max(2 * base_degree, 256) with base_degree = 2 * degree (:38, :69-70); every other
    parameter keeps the default of cuvsCagraSearchParamsCreate, which are the defaults of oracle.cagra_search"""
    return dict(itopk_size=max(4 * degree, 256))


def _walk(search, x_cur, graph_cur, queries, K, degree, metric):
    """ids [len(queries), K] uint32 of the walk over the n_cur rows searchable so far; a graph with fewer than K rows is
    searched for k = n_cur and the missing columns are invalid; so is every id outside the graph (:129, :158)"""
    n_cur = x_cur.shape[0]
    k = min(K, n_cur)
    _, ids = search(x_cur, graph_cur, queries, k, metric=metric, **search_params(degree))
    ids = np.asarray(ids).astype(np.int64)
    out = np.full((queries.shape[0], K), INVALID, np.int64)
    out[:, :k] = np.where((ids < 0) | (ids >= n_cur), INVALID, ids)
    return out


def rank_list(cand, graph, n_cur, degree):
    """step 2 for one row (:155-187): the detour count of candidate i is the number of valid candidates j < i whose list holds
    candidate i; an invalid id counts 2 * degree + 1. Stable sort by count (this project's rule for ties, see the module text);
    the first `degree` entries."""
    K = cand.shape[0]
    valid = cand < n_cur
    holds = np.zeros((K, K), bool)  # holds[j, i]: the list of candidate j contains candidate i
    holds[valid] = (graph[cand[valid]][:, None, :] == cand[None, :, None]).any(2)
    earlier = np.tri(K, K, -1, dtype=bool).T  # [j, i]: j < i
    count = (holds & earlier).sum(0)
    count[~valid] = K + 1
    return cand[np.argsort(count, kind="stable")][:degree]


def add_row(graph, incoming, new_id, ranks, n_new, degree):
    """step 3 for one row (:195-275), in place on graph [n_new, degree] and incoming [n_new]"""
    half = degree // 2
    evicted = []
    for i in range(half):
        target = int(ranks[i])
        if target >= n_new:
            raise ValueError(f"Invalid node ID found in updated_graph ({target})")  # :200-202
        take_id, take_slot, take_count = n_new, 0, 0  # the defaults (:203-205): slot 0, an id that is skipped below
        for j in range(degree - 1, half - 1, -1):
            nb = int(graph[target, j])
            if nb >= n_new:
                raise ValueError(f"Invalid node ID found in updated_graph ({nb})")  # :209-211
            if incoming[nb] > take_count and nb not in evicted:  # strictly more incoming edges; not taken for this row yet
                take_id, take_slot, take_count = nb, j, int(incoming[nb])
        graph[target, take_slot] = new_id
        evicted.append(take_id)
    incoming[new_id] = half  # :233; no other count changes
    # the row's own list: rank list and evicted ids in turns (:237-265), duplicates and ids >= n_new skipped
    lists, pos, out, turn = (list(map(int, ranks)), evicted), [0, 0], [], 0
    while len(out) < degree and (pos[0] < degree or pos[1] < half):
        src = lists[turn]
        while pos[turn] < len(src):
            c = src[pos[turn]]
            if c < n_new and c not in out:
                out.append(c)  # (the position is not advanced, as in the reference: the entry is a duplicate the next time)
                break
            pos[turn] += 1
        turn = 1 - turn
    if len(out) < degree:
        raise ValueError(f"Number of edges is not enough (target_new_node_id:{new_id}, num_add:{len(out)}, degree:{degree})")
    graph[new_id] = out


def extend_twin(x_all, graph0, n0, degree, metric, max_chunk_size, search=oracle.cagra_search):
    """The graph [n0 + m, degree] uint32 after extending the index (rows x_all[:n0], graph graph0) by the rows x_all[n0:].
    `search(dataset, graph, queries, k, itopk_size=..., metric=...)` -> (distances, ids) is the walk of step 1.

    The bound called new_size in add_node_core is the row count after the CURRENT chunk (:35-37 with the index of :304-341);
    it is used as the default evicted id and as the limit of valid ids, so a later chunk's rows are never named before they
    exist."""
    x_all = np.asarray(x_all)
    n_total = x_all.shape[0]
    m = n_total - n0
    graph = np.full((n_total, degree), INVALID, np.uint32)
    graph[:n0] = np.asarray(graph0).astype(np.int64) & INVALID
    chunk = max(m, 1) if max_chunk_size == 0 else int(max_chunk_size)  # 0: one chunk that holds everything (:297-298)
    for c0 in range(0, m, chunk):
        n_cur = n0 + c0  # rows the chunk searches: the old rows and all earlier chunks (:310-326)
        n_new = min(n_cur + chunk, n_total)
        incoming = np.bincount(graph[:n_cur].ravel(), minlength=n_new)[:n_new].astype(np.int64)  # step 0 (:40-53)
        cand = _walk(search, x_all[:n_cur], graph[:n_cur], x_all[n_cur:n_new], 2 * degree, degree, metric)
        start = graph[:n_cur].astype(np.int64)  # step 2 reads the graph the chunk starts from: it runs before any of step 3
        ranks = [rank_list(c, start, n_cur, degree) for c in cand]
        for r, rk in enumerate(ranks):
            add_row(graph, incoming, n_cur + r, rk, n_new, degree)
    return graph


def in_degree(graph):
    return np.bincount(np.asarray(graph).astype(np.int64).ravel() & INVALID, minlength=graph.shape[0])


# ---------------------------------------------------------------- inputs shared by the CPU and the GPU tests
F32, F16, I8, U8 = "float32", "float16", "int8", "uint8"
SQ, IP, COS = "sqeuclidean", "inner_product", "cosine"
# (n0, m, dim, degree, max_chunk_size, dtype, metric)
SHAPES = [
    (600, 300, 16, 16, 0, F32, SQ),    # one chunk
    (500, 257, 33, 32, 64, F32, SQ),   # odd dim; a 1-row last chunk; chunks that link to earlier chunks
    (70, 40, 8, 32, 16, F32, SQ),      # fewer rows than the walk's list: results padded with invalid ids
    (1000, 1, 24, 24, 0, F32, SQ),     # a single added row; a degree that is not a power of two
    (40, 30, 8, 32, 16, F32, SQ),      # fewer than 2 * degree rows: the walk is asked for k = n_cur
]
DTYPES = [(600, 300, 16, 16, 0, dt, SQ) for dt in (F16, I8, U8)]
METRICS = [(600, 300, 16, 16, 0, F32, mt) for mt in (IP, COS)]
REPEATED = (800, 25, 16, 16, 0, F32, SQ)  # 20 calls of 25 rows
REPEATED_CALLS = 20


def case_id(case):
    return "-".join(str(v) for v in case)


def rows(n, dim, dtype, seed):
    rng = np.random.default_rng(seed)
    if dtype == I8:
        x = rng.integers(-20, 20, size=(n, dim))
    elif dtype == U8:
        x = rng.integers(0, 40, size=(n, dim))
    else:
        x = rng.standard_normal((n, dim))
    return x.astype(dtype)


def knn_graph(x, degree, metric):
    """exact kNN graph [n, degree] uint32 in float64, self excluded, ties to the lower id"""
    x = np.asarray(x).astype(np.float64)
    if metric == SQ:
        sq = (x * x).sum(1)
        d = sq[:, None] + sq[None, :] - 2.0 * x @ x.T
    elif metric == IP:
        d = -(x @ x.T)
    else:
        xn = x / np.linalg.norm(x, axis=1, keepdims=True)
        d = 1.0 - xn @ xn.T
    np.fill_diagonal(d, np.inf)
    return np.argsort(d, axis=1, kind="stable")[:, :degree].astype(np.uint32)


_INPUTS = {}


def inputs(case, calls=1):
    """(x_all [n0 + calls * m, dim], graph0 [n0, degree]) of a case, made once and read-only"""
    key = (case, calls)
    if key not in _INPUTS:
        n0, m, dim, degree, _, dtype, metric = case
        x = rows(n0 + calls * m, dim, dtype, 1000 + n0 + m + dim)
        g = knn_graph(x[:n0], degree, metric)
        x.setflags(write=False)
        g.setflags(write=False)
        _INPUTS[key] = (x, g)
    return _INPUTS[key]


_TWINS = {}


def twin(case, calls=1):
    """extend_twin over inputs(case) with the oracle walk, applied `calls` times (m rows a call); computed once, read-only"""
    key = (case, calls)
    if key not in _TWINS:
        n0, m, dim, degree, chunk, dtype, metric = case
        x, g = inputs(case, calls)
        for c in range(calls):
            n_cur = n0 + c * m
            g = extend_twin(x[:n_cur + m], g, n_cur, degree, metric, chunk)
        g.setflags(write=False)
        _TWINS[key] = g
    return _TWINS[key]
