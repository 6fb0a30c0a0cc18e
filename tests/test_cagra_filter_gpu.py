"""GPU: filtered CAGRA search and source-id maps against the CPU twin.

The single-workgroup walk is deterministic, so a filtered search is pinned bit for bit against
oracle.cagra_search(filter_words=...) on the graph read back from the index. The multi-wave walk races for parents, so it is
checked through invariants and a recall floor taken from the oracle's single walk. An independent float64 anchor (exact
filtered kNN) holds even if the bit-level comparison is ever relaxed.

The contract pinned here: the filter is a bitset over SOURCE ids (the rows themselves, or source_indices[row] for an index
loaded from a file that carries them); the single walk filters when it writes results, so a heavy filter may give fewer than
k neighbours - trailing padding, id -1 (int64) / 0xffffffff (uint32) at distance FLT_MAX."""
import functools

import numpy as np
import pytest

import oracle
from tests import refformat as rf

pytestmark = pytest.mark.gpu

N, NQ, K = 4013, 64, 10  # 4013 rows: the last bitset word is partial (4013 = 125 * 32 + 13)
FLT_MAX = np.finfo(np.float32).max
F32, F16, I8, U8 = "float32", "float16", "int8", "uint8"


# ------------------------------------------------------------------ data, indexes, filters (built once, never modified)
@functools.lru_cache(maxsize=None)
def _data(dtype, n=N):
    rng = np.random.default_rng({F32: 1, F16: 2, I8: 3, U8: 4}[dtype])
    if dtype == I8:
        x, q = rng.integers(-20, 20, size=(n, 48)), rng.integers(-20, 20, size=(NQ, 48))
    elif dtype == U8:
        x, q = rng.integers(0, 40, size=(n, 48)), rng.integers(0, 40, size=(NQ, 48))
    else:
        x, q = rng.standard_normal((n, 32)), rng.standard_normal((NQ, 32))
    x, q = x.astype(dtype), q.astype(dtype)
    x.setflags(write=False)
    q.setflags(write=False)
    return x, q


@functools.lru_cache(maxsize=None)
def _index(dtype, metric):
    """(index, graph read back as uint32 [n, 32])"""
    import torch
    from cuvs_amd.neighbors import cagra

    x, _ = _data(dtype)
    index = cagra.build(cagra.IndexParams(metric=metric, intermediate_graph_degree=64, graph_degree=32), torch.from_numpy(x.copy()).cuda())
    graph = index.graph.cpu().numpy().view(np.uint32).copy()
    graph.setflags(write=False)
    return index, graph


def _pack(keep):
    """bool per bit -> uint32 words, bit i of word i // 32 (the last word zero-padded)"""
    pad = np.zeros((-keep.size) % 32, bool)
    return np.packbits(np.concatenate([keep, pad]), bitorder="little").view(np.uint32).copy()


@functools.lru_cache(maxsize=None)
def _keep(share, n=N):
    keep = np.ones(n, bool) if share == 1.0 else np.random.default_rng(int(share * 1000) + n).random(n) < share
    keep.setflags(write=False)
    return keep


def _dev_words(words):
    import torch

    return torch.from_numpy(words.view(np.int32)).cuda()


def _gpu_search(index, q, k, words, out, **params):
    """ids as int64 with -1 for padding (after checking the sentinel of the requested output type), float32 distances"""
    import torch
    from cuvs_amd._lib import BITSET
    from cuvs_amd.neighbors import cagra

    tq = torch.from_numpy(q.copy()).cuda()
    nb = torch.empty((q.shape[0], k), dtype=torch.int64 if out == "int64" else torch.int32, device="cuda")
    flt = None if words is None else (_dev_words(words) if isinstance(words, np.ndarray) else words, BITSET)
    d, i = cagra.search(cagra.SearchParams(**params), index, tq, k, neighbors=nb, filter=flt)
    torch.cuda.synchronize()
    d = d.cpu().numpy()
    if out == "int64":
        ids = i.cpu().numpy()
        assert ids.dtype == np.int64 and (ids >= -1).all()
    else:
        raw = i.cpu().numpy().view(np.uint32)
        ids = np.where(raw == 0xFFFFFFFF, -1, raw.astype(np.int64))
    return d, ids


# ------------------------------------------------------------------ float64 anchor
def _sq64(q, x):
    q, x = q.astype(np.float64), x.astype(np.float64)
    return (q * q).sum(1)[:, None] + (x * x).sum(1)[None, :] - 2.0 * q @ x.T


def _check_invariants(d, ids, q, x, keep):
    """sqeuclidean results [nq, k] (ids: rows, -1 = padding) against float64 distances and the row filter `keep`"""
    pad = ids < 0
    assert (pad[:, 1:] >= pad[:, :-1]).all(), "padding before a real neighbour"
    assert (d[pad] == FLT_MAX).all(), "padding distance is not FLT_MAX"
    assert (ids[~pad] < x.shape[0]).all()
    assert keep[ids[~pad]].all(), "a filtered-out row came back"
    for r in ids:
        real = r[r >= 0]
        assert len(np.unique(real)) == len(real), "an id repeats"
    assert (d[:, 1:] >= d[:, :-1]).all(), "distances decrease"
    d64 = _sq64(q, x)
    want = np.take_along_axis(d64, np.where(pad, 0, ids), axis=1)
    np.testing.assert_allclose(d[~pad], want[~pad], rtol=1e-4, atol=0)


def _recall_filled(ids, q, x, keep):
    """(recall@k against exact filtered kNN in float64, share of slots filled). A returned row counts when it is at least as
    near as the k-th true neighbour, so equal distances (integer rows) are no misses."""
    d64 = _sq64(q, x)
    d64[:, ~keep] = np.inf
    kth = np.sort(d64, axis=1)[:, ids.shape[1] - 1]
    got = np.where(ids >= 0, np.take_along_axis(d64, np.where(ids < 0, 0, ids), axis=1), np.inf)
    return float((got <= kth[:, None]).mean()), float((ids >= 0).mean())


# ------------------------------------------------------------------ 1. single-workgroup walk, filtered, bit-exact
SQ, IP, COS = "sqeuclidean", "inner_product", "cosine"
# dtype, metric, search_width, itopk, keep share, neighbours type: every value at least twice
CASES = [
    (F32, SQ, 1, 64, 1.0, "uint32"),
    (F32, SQ, 1, 64, 0.7, "int64"),
    (F32, SQ, 1, 64, 0.5, "uint32"),
    (F32, SQ, 1, 64, 0.1, "int64"),
    (F32, SQ, 1, 256, 0.1, "uint32"),
    (F32, SQ, 2, 256, 0.5, "int64"),
    (F32, SQ, 2, 64, 0.7, "uint32"),
    (F32, IP, 1, 64, 0.5, "uint32"),
    (F32, IP, 2, 256, 0.1, "int64"),
    (F32, COS, 1, 64, 0.7, "int64"),
    (F32, COS, 2, 256, 1.0, "uint32"),
    (F16, SQ, 1, 64, 0.5, "int64"),
    (F16, SQ, 2, 256, 0.1, "uint32"),
    (F16, IP, 1, 256, 0.7, "uint32"),
    (F16, COS, 2, 64, 0.1, "int64"),
    (I8, SQ, 1, 64, 0.5, "uint32"),
    (I8, SQ, 2, 256, 0.1, "int64"),
    (I8, IP, 2, 64, 0.7, "int64"),
    (I8, COS, 1, 256, 0.5, "uint32"),
    (U8, SQ, 1, 64, 0.1, "int64"),
    (U8, SQ, 2, 256, 0.7, "uint32"),
    (U8, IP, 1, 256, 1.0, "int64"),
    (U8, COS, 2, 64, 0.5, "uint32"),
    (U8, COS, 1, 64, 0.7, "int64"),
]
_id = lambda c: "-".join(str(v) for v in c)  # noqa: E731


@functools.lru_cache(maxsize=None)
def _single_walk(case):
    """(GPU distances, GPU ids, oracle distances, oracle ids) of one row of CASES"""
    dtype, metric, width, itopk, share, out = case
    x, q = _data(dtype)
    index, graph = _index(dtype, metric)
    words = _pack(_keep(share))
    gd, gi = _gpu_search(index, q, K, words, out, itopk_size=itopk, search_width=width, algo="single_cta")
    od, oi = oracle.cagra_search(x, graph, q, K, itopk_size=itopk, search_width=width, metric=metric, filter_words=words)
    return gd, gi, od, oi


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_single_walk_filtered_matches_oracle(case):
    dtype, metric, width, itopk, share, out = case
    gd, gi, od, oi = _single_walk(case)
    print(f"{_id(case)}: id mismatch rate {(gi != oi).mean():.4f}, filled {(oi >= 0).mean():.4f}")
    assert (gi == oi).all(), f"id mismatch rate {(gi != oi).mean():.4f}"
    assert (gd == od).all()
    if share == 1.0:  # an all-ones bitset changes nothing
        x, q = _data(dtype)
        index, graph = _index(dtype, metric)
        ud, ui = _gpu_search(index, q, K, None, out, itopk_size=itopk, search_width=width, algo="single_cta")
        assert (ui == gi).all() and (ud == gd).all()
        pd_, pi = oracle.cagra_search(x, graph, q, K, itopk_size=itopk, search_width=width, metric=metric)
        assert (pi == gi).all() and (pd_ == gd).all()


# ------------------------------------------------------------------ 2. independent anchor
# keep 0.5 / itopk 64 and keep 0.1 / itopk 256: every slot filled and recall >= 0.95 (the CPU twin measured 0.988 and 1.000 on an
# exact-kNN graph of the same shape)
ABSOLUTE_FLOORS = {(1, 64, 0.5), (1, 256, 0.1)}


@pytest.mark.parametrize("case", [c for c in CASES if c[0] == F32 and c[1] == SQ], ids=_id)
def test_single_walk_filtered_against_exact_knn(case):
    dtype, metric, width, itopk, share, out = case
    gd, gi, od, oi = _single_walk(case)
    x, q = _data(dtype)
    keep = _keep(share)
    _check_invariants(gd, gi, q, x, keep)
    g_recall, g_filled = _recall_filled(gi, q, x, keep)
    o_recall, o_filled = _recall_filled(oi, q, x, keep)
    print(f"{_id(case)}: oracle recall {o_recall:.4f} filled {o_filled:.4f}; gpu recall {g_recall:.4f} filled {g_filled:.4f}")
    assert g_recall == o_recall and g_filled == o_filled
    if (width, itopk, share) in ABSOLUTE_FLOORS:
        assert g_filled == 1.0 and g_recall >= 0.95


# ------------------------------------------------------------------ 3. short results
def test_filter_that_keeps_four_rows():
    """The kept rows are the exact nearest neighbours of queries 0..3, so those walks reach at least one of them; everything
    else is padding."""
    x, q = _data(F32)
    index, graph = _index(F32, SQ)
    kept_rows = np.unique(_sq64(q[:4], x).argmin(1))
    keep = np.zeros(N, bool)
    keep[kept_rows] = True
    words = _pack(keep)
    od, oi = oracle.cagra_search(x, graph, q, K, itopk_size=64, filter_words=words)
    assert (oi >= 0).any() and (oi < 0).any()  # (the case holds both real neighbours and padding)
    for out in ("uint32", "int64"):
        gd, gi = _gpu_search(index, q, K, words, out, itopk_size=64, algo="single_cta")
        assert (gi == oi).all() and (gd == od).all()
        _check_invariants(gd, gi, q, x, keep)
        assert ((gi >= 0).sum(1) <= len(kept_rows)).all()


def test_all_zero_bitset():
    """Nothing passes: every slot is padding and nothing fails. filtering_rate is clamped at 0.999 and not taken as 1.0 ("no
    filter"): the multi-wave plan widens its list by it (search_plan.cuh:199-245), here past the 1024 entries this library
    walks with, which is refused on the host before the walk is launched."""
    from cuvs_amd._lib import CuvsError

    x, q = _data(F32)
    index, graph = _index(F32, SQ)
    words = np.zeros((N + 31) // 32, np.uint32)
    for out in ("uint32", "int64"):
        gd, gi = _gpu_search(index, q, K, words, out, itopk_size=64, algo="single_cta")
        assert (gi == -1).all() and (gd == FLT_MAX).all()
    od, oi = oracle.cagra_search(x, graph, q, K, itopk_size=64, filter_words=words)
    assert (oi == -1).all() and (od == FLT_MAX).all()
    with pytest.raises(CuvsError, match="itopk_size up to 1024"):
        _gpu_search(index, q, K, words, "int64", itopk_size=64, algo="multi_cta")
    ud, ui = _gpu_search(index, q, K, None, "int64", itopk_size=64, algo="single_cta")
    pd_, pi = oracle.cagra_search(x, graph, q, K, itopk_size=64)
    assert (ui == pi).all() and (ud == pd_).all()


# ------------------------------------------------------------------ 4. multi-wave walk with a filter
MULTI_WAVE_MARGIN = 0.05  # the walks traverse differently; the filtered multi-wave list is widened by filtering_rate


@pytest.mark.parametrize("nq", [5, 64])
@pytest.mark.parametrize("share", [0.5, 0.1])
@pytest.mark.parametrize("dtype", [F32, I8])
def test_multi_wave_filtered(dtype, share, nq):
    x, q = _data(dtype)
    q = q[:nq]
    index, graph = _index(dtype, SQ)
    keep = _keep(share)
    words = _pack(keep)
    gd, gi = _gpu_search(index, q, K, words, "int64", itopk_size=64, algo="multi_cta")
    _check_invariants(gd, gi, q, x, keep)
    _, oi = oracle.cagra_search(x, graph, q, K, itopk_size=64, filter_words=words)
    o_recall, o_filled = _recall_filled(oi, q, x, keep)
    g_recall, g_filled = _recall_filled(gi, q, x, keep)
    print(f"{dtype}-{share}-{nq}: single-walk oracle recall {o_recall:.4f} filled {o_filled:.4f}; "
          f"multi-wave recall {g_recall:.4f} filled {g_filled:.4f}")
    assert g_recall >= o_recall - MULTI_WAVE_MARGIN


# ------------------------------------------------------------------ 5. source-id map with a filter
def _source_map():
    return (3 * (N - 1 - np.arange(N, dtype=np.int64)) + 7).astype(np.uint32)


@pytest.fixture(scope="module")
def mapped(tmp_path_factory):
    """the float32 / sqeuclidean index as a reference-format file with source ids, loaded back"""
    from cuvs_amd.neighbors import cagra

    x, _ = _data(F32)
    _, graph = _index(F32, SQ)
    f = str(tmp_path_factory.mktemp("cagra_filter") / "cagra_src.bin")
    rf.write_cagra(f, graph, x, metric=0, dtype=np.float32, source_indices=_source_map())
    return cagra.load(f)


@pytest.mark.parametrize("out", ["uint32", "int64"])
@pytest.mark.parametrize("share", [0.5, 0.1])  # 0.1 at itopk 64 leaves padding: the sentinels pass through the id map
def test_source_map_filtered_single_walk(mapped, share, out):
    x, q = _data(F32)
    _, graph = _index(F32, SQ)
    src = _source_map().astype(np.int64)
    keep_src = np.random.default_rng(77 + int(share * 10)).random(3 * N + 8) < share
    words = _pack(keep_src)  # over source ids
    gd, gi = _gpu_search(mapped, q, K, words, out, itopk_size=64, algo="single_cta")
    od, oi = oracle.cagra_search(x, graph, q, K, itopk_size=64, filter_words=_pack(keep_src[src]))  # per row
    want = np.where(oi >= 0, src[np.where(oi < 0, 0, oi)], -1)
    if share == 0.1:
        assert (oi < 0).any()
    print(f"mapped-{share}-{out}: id mismatch rate {(gi != want).mean():.4f}")
    assert (gi == want).all() and (gd == od).all()


@pytest.mark.parametrize("out", ["uint32", "int64"])
@pytest.mark.parametrize("share", [0.5, 0.1])
def test_source_map_filtered_multi_wave(mapped, share, out):
    x, q = _data(F32)
    src = _source_map().astype(np.int64)
    keep_src = np.random.default_rng(77 + int(share * 10)).random(3 * N + 8) < share
    gd, gi = _gpu_search(mapped, q, K, _pack(keep_src), out, itopk_size=64, algo="multi_cta")
    real = gi >= 0
    assert keep_src[gi[real]].all(), "a filtered-out source id came back"
    row_of = np.full(3 * N + 8, -1, np.int64)
    row_of[src] = np.arange(N)
    rows = np.where(real, row_of[np.where(real, gi, 0)], -1)
    assert (rows[real] >= 0).all(), "an id outside the source map came back"
    _check_invariants(gd, rows, q, x, keep_src[src])


# ------------------------------------------------------------------ 6. refusals, all raised on the host
def test_refusals_leave_the_index_usable(mapped):
    import torch
    from cuvs_amd._lib import BITSET, CuvsError
    from cuvs_amd.neighbors import cagra

    x, q = _data(F32)
    index, graph = _index(F32, SQ)
    src = _source_map().astype(np.int64)
    sp = dict(itopk_size=64, algo="single_cta")
    pd_, pi = oracle.cagra_search(x, graph, q, K, itopk_size=64)

    def still_answers():
        d, i = _gpu_search(index, q, K, None, "int64", **sp)
        assert (i == pi).all() and (d == pd_).all()
        d, i = _gpu_search(mapped, q, K, None, "int64", **sp)
        assert (i == src[pi]).all() and (d == pd_).all()

    still_answers()
    n_words = (N + 31) // 32
    ones = np.full(n_words, 0xFFFFFFFF, np.uint32)
    # a bitset one word short for a plain index: search
    with pytest.raises(CuvsError, match=f"bitset filter holds {32 * (n_words - 1)} bits, the index {N} rows"):
        _gpu_search(index, q, K, ones[:-1], "int64", **sp)
    still_answers()
    # ... and merge (two inputs: 2 N rows)
    p = cagra.IndexParams(intermediate_graph_degree=64, graph_degree=32)
    m_words = (2 * N + 31) // 32
    short = _dev_words(np.full(m_words - 1, 0xFFFFFFFF, np.uint32))
    with pytest.raises(CuvsError, match=f"bitset filter holds {32 * (m_words - 1)} bits, the index {2 * N} rows"):
        cagra.merge(p, [index, index], filter=(short, BITSET))
    still_answers()
    # a bitset sized for the rows of a mapped index, whose source ids go up to 3 N + 4
    with pytest.raises(CuvsError, match=f"bitset filter holds {32 * n_words} bits, the index {3 * N + 5} source ids"):
        _gpu_search(mapped, q, K, ones, "int64", **sp)
    still_answers()
    # a 2-D filter tensor
    for ix, words in ((index, ones), (mapped, np.full((3 * N + 8 + 31) // 32, 0xFFFFFFFF, np.uint32))):
        with pytest.raises(CuvsError, match="1-D"):
            _gpu_search(ix, q, K, _dev_words(words).reshape(1, -1), "int64", **sp)
    with pytest.raises(CuvsError, match="1-D"):
        cagra.merge(p, [index, index], filter=(_dev_words(np.full(m_words, 0xFFFFFFFF, np.uint32)).reshape(1, -1), BITSET))
    still_answers()
    # extend on a mapped index; merge with a mapped input (refused, the map is not dropped silently)
    with pytest.raises(CuvsError, match="source_indices"):
        cagra.extend(mapped, torch.from_numpy(x[:100].copy()).cuda())
    assert len(mapped) == N
    still_answers()
    with pytest.raises(CuvsError, match="source_indices"):
        cagra.merge(p, [index, mapped])
    still_answers()


# ------------------------------------------------------------------ 7. extend after load without a map
def test_extend_after_load_then_filtered_search(tmp_path):
    import torch
    from cuvs_amd.neighbors import cagra

    x, q = _data(F32)
    index, _ = _index(F32, SQ)
    f = str(tmp_path / "cagra.bin")
    cagra.save(f, index)
    loaded = cagra.load(f)
    extra = np.random.default_rng(500).standard_normal((500, 32)).astype(np.float32)
    cagra.extend(loaded, torch.from_numpy(extra).cuda())
    assert len(loaded) == N + 500
    x_all = np.concatenate([x, extra])
    graph = loaded.graph.cpu().numpy().view(np.uint32)
    assert graph.shape == (N + 500, 32) and (graph < N + 500).all()
    keep = _keep(0.5, N + 500)
    words = _pack(keep)
    _, oi = oracle.cagra_search(x_all, graph, q, K, itopk_size=128, filter_words=words)
    o_recall, o_filled = _recall_filled(oi, q, x_all, keep)
    for algo in ("single_cta", "auto"):
        gd, gi = _gpu_search(loaded, q, K, words, "int64", itopk_size=128, algo=algo)
        _check_invariants(gd, gi, q, x_all, keep)
        g_recall, g_filled = _recall_filled(gi, q, x_all, keep)
        print(f"extend-{algo}: oracle recall {o_recall:.4f} filled {o_filled:.4f}; gpu recall {g_recall:.4f} filled {g_filled:.4f}")
        assert g_recall >= o_recall - 0.02
    assert (gi >= N).any()  # (new rows are found)
