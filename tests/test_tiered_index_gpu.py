"""GPU: the tiered index (cuvsTieredIndex*) - the tail phase against the numpy restatement bit for bit on both
paths, the composition end to end for the three ANN algos, thresholds, merge, refusals and the Python surface."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle
from tests import tiered_index_ref as R

pytestmark = pytest.mark.gpu

METRICS = ["sqeuclidean", "euclidean", "inner_product", "cosine"]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _assert_same(got, want, what=""):
    """(distances, ids) pairs: the same ids and the same distance bits."""
    gd, gi = (x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x) for x in got)
    wd, wi = want
    bad = np.nonzero((gi != wi).any(1) | (_bits(gd) != _bits(wd)).any(1))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} rows differ, first {bad[0]}: ids {gi[bad[0]]} / {wi[bad[0]]}, d {gd[bad[0]]} / {wd[bad[0]]}"


def _dev(a, dtype=None):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.view(dtype)
    return t.cuda()


def _words(keep):
    """bool [n] -> device int32 words of the bitset (read as uint32 by the library)."""
    import torch

    return _dev(R.pack_bits(keep), torch.int32)


def _rows(n, dim, seed, ties=False, nonzero=False):
    rng = np.random.default_rng(seed)
    if ties:
        x = rng.integers(-4, 5, size=(n, dim)).astype(np.float32)
        if nonzero:  # (cosine: no zero vector)
            x[(x == 0).all(1), 0] = 1.0
        return x
    return rng.normal(0.1, 2.0, size=(n, dim)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------- 1. the tail phase alone
ANN_ROWS = 77  # not a multiple of 32: tail row j sits at bit 77 + j

# (m, dim, tail, k): both sides of the 64-query boundary of the single-launch kernel, dims that leave the vector loads, tails
# at the edges of a 256-row tile and of the 1024-entry buffer, k up to beyond the tail and beyond one wave's merge
TAIL_SHAPES = [
    (1, 128, 1, 1), (1, 29, 127, 10), (7, 1, 129, 10), (7, 29, 1000, 64), (64, 128, 1000, 10), (64, 29, 5000, 65),
    (65, 128, 129, 10), (65, 29, 1000, 300), (200, 128, 5000, 10), (33, 16, 127, 300), (16, 128, 5000, 64), (5, 29, 1025, 1),
]


def _good_a(q, ann, k, metric, keep_ann):
    """The true neighbours of the hidden ANN part; filtered or missing slots are padding (id -1)."""
    bits = None if keep_ann is None else R.pack_bits(keep_ann)
    d, i = oracle.brute_force_knn(q, ann, k, metric, keep_bits=bits)
    select_min = metric != "inner_product"
    pad = (i < 0) | (d == R.worst(select_min))
    return np.where(pad, R.worst(select_min), d).astype(np.float32), np.where(pad, -1, i).astype(np.int64)


def _a_variants(q, ann, k, metric, keep_ann, seed):
    select_min = metric != "inner_product"
    gd, gi = _good_a(q, ann, k, metric, keep_ann)
    out = {"good": (gd, gi)}
    rng = np.random.default_rng(seed)
    # poor: real entries, all far away - every tail row beats the bound (beyond 1024 rows that overflows the buffer)
    pi = np.stack([np.sort(rng.choice(len(ann), size=min(k, len(ann)), replace=False)) for _ in range(len(q))]).astype(np.int64)
    pi = np.concatenate([pi, np.full((len(q), k - pi.shape[1]), -1, np.int64)], axis=1)
    pd = np.full((len(q), k), 1e30 if select_min else -1e30, np.float32)
    out["poor"] = (pd, pi)
    pads = [-1, R.I64_MAX, 0xFFFFFFFF, ANN_ROWS, ANN_ROWS + 3]
    for name, cnt in (("pad_last", 1), ("pad_half", max(1, k // 2)), ("pad_all", k)):
        d, i = gd.copy(), gi.copy()
        for j in range(k - cnt, k):
            i[:, j] = pads[j % len(pads)]
            d[:, j] = [0.0, R.F32_MAX, -R.F32_MAX, -3.0][j % 4]  # a padding slot's distance says nothing
        out[name] = (d, i)
    return out


@functools.lru_cache(maxsize=None)
def _tail_case(m, dim, tail, k, metric, ties):
    nz = metric == "cosine"
    seed = 1000 * m + tail + k
    q = _rows(m, dim, seed, ties, nz)
    ann = _rows(ANN_ROWS, dim, seed + 1, ties, nz)
    x = _rows(tail, dim, seed + 2, ties, nz)
    rng = np.random.default_rng(seed + 3)
    n = ANN_ROWS + tail
    filters = {"none": None, "random": rng.random(n) < 0.4}
    none_left = np.ones(n, bool)
    none_left[ANN_ROWS:] = False  # the whole tail filtered
    few = np.zeros(n, bool)
    few[rng.choice(n, size=min(n, max(1, k // 2)), replace=False)] = True  # fewer than k rows left in total
    filters["tail_gone"] = none_left
    filters["few_left"] = few
    return q, ann, x, filters


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("m,dim,tail,k", TAIL_SHAPES)
def test_tail_phase_equals_the_restatement(res, m, dim, tail, k, metric):
    from cuvs_amd.neighbors import tiered_index as T

    q, ann, x, filters = _tail_case(m, dim, tail, k, metric, False)
    _check_tail(res, T, q, ann, x, filters, k, metric, ["none", "random"] + (["tail_gone", "few_left"] if m in (7, 65) else []))


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("m,dim,tail,k", [(7, 29, 1000, 64), (64, 128, 1000, 10), (65, 128, 129, 10), (16, 128, 5000, 64)])
def test_tail_phase_with_ties_equals_the_restatement(res, m, dim, tail, k, metric):
    """Integer-valued rows in [-4, 4]: distances repeat inside the tail and across the tiers."""
    from cuvs_amd.neighbors import tiered_index as T

    q, ann, x, filters = _tail_case(m, dim, tail, k, metric, True)
    _check_tail(res, T, q, ann, x, filters, k, metric, ["none", "random"])


def _check_tail(res, T, q, ann, x, filters, k, metric, filter_names):
    select_min = metric != "inner_product"
    m, dim = q.shape
    tail = len(x)
    fused_ok = m <= 64 and m * ((dim + 15) // 16 * 16) <= 8192 and k <= 1024
    dq, dx = _dev(q), _dev(x)
    for fname in filter_names:
        keep = filters[fname]
        bits = None if keep is None else _words(keep)
        tb = None if keep is None else R.tail_bits(R.pack_bits(keep), ANN_ROWS, tail)
        b = R.globalize(*oracle.brute_force_knn(q, x, k, metric, keep_bits=tb), ANN_ROWS, select_min)
        if fname == "tail_gone":
            assert (b[1] == R.I64_MAX).all()
        for aname, a in _a_variants(q, ann, k, metric, None if keep is None else keep[:ANN_ROWS], m + k).items():
            want = R.merge(a, b, ANN_ROWS, select_min)
            if fname == "few_left" and aname == "good":
                assert (want[1] == R.I64_MAX).any()  # fewer than k rows in total: padding in the result
            da_d, da_i = _dev(a[0]), _dev(a[1])
            before = T.counters()
            for path in ["composed", "auto"] + (["fused"] if fused_ok else []):
                got = T.tail_search(metric, dx, ANN_ROWS, dq, da_i, da_d, bitset=bits, path=path, resources=res)
                _assert_same(got, want, f"{fname}/{aname}/{path}")
            after = T.counters()
            assert after[0] > before[0] and (after[1] > before[1]) == fused_ok  # both kernels ran (where the second one can)
            if aname == "poor" and fname == "none" and tail > 1024 and k <= 1024:
                assert after[2] - before[2] == (3 if fused_ok else 2)  # every path overflowed and was redone exactly
            if tail <= 1024:
                assert after[2] == before[2]
    if not fused_ok:
        with pytest.raises(Exception, match="single-launch tail kernel takes"):
            T.tail_search(metric, dx, ANN_ROWS, dq, da_i, da_d, path="fused", resources=res)


@pytest.mark.parametrize("select_min", [True, False])
@pytest.mark.parametrize("k,kb", [(1, 1), (10, 10), (10, 300), (64, 64), (65, 5), (300, 300), (1024, 1024), (2048, 2048)])
def test_merge_kernel_equals_the_restatement(res, k, kb, select_min):
    from cuvs_amd.neighbors import tiered_index as T

    rng = np.random.default_rng(k * 7 + kb)
    m, ann_rows, n_tail = 9, 5000, 4000
    ai = np.stack([rng.choice(ann_rows, size=k, replace=False) for _ in range(m)]).astype(np.int64)
    bi = ann_rows + np.stack([rng.choice(n_tail, size=kb, replace=False) for _ in range(m)]).astype(np.int64)
    ad = rng.integers(0, 50, size=(m, k)).astype(np.float32) / 4  # ties inside and across the tiers
    bd = rng.integers(0, 50, size=(m, kb)).astype(np.float32) / 4
    ad[0, 0], bd[0, 0] = 0.0, -0.0
    for r in range(m):  # padding at several positions, in the forms the ANN tiers use; its distance says nothing
        for j in rng.choice(k, size=(r * k) // (m - 1), replace=False):
            ai[r, j] = [-1, R.I64_MAX, 0xFFFFFFFF, ann_rows][j % 4]
            ad[r, j] = [-7.0, R.F32_MAX, 0.0, -R.F32_MAX][j % 4]
        for j in rng.choice(kb, size=((m - 1 - r) * kb) // (m - 1), replace=False):
            bi[r, j] = R.I64_MAX
            bd[r, j] = R.worst(select_min)
    want = R.merge((ad, ai), (bd, bi), ann_rows, select_min)
    got = T.merge_tiers(_dev(ai), _dev(ad), _dev(bi), _dev(bd), ann_rows, select_min, resources=res)
    _assert_same(got, want)
    assert (want[1][m - 1] == R.I64_MAX).all() or kb > 0


# ---------------------------------------------------------------------------------------------------- 2. composition end to end
def _upstream(algo, metric):
    from cuvs_amd.neighbors import cagra, ivf_flat, ivf_pq

    if algo == "cagra":
        return cagra.IndexParams(metric=metric, graph_degree=16, intermediate_graph_degree=32, build_algo="nn_descent")
    if algo == "ivf_flat":
        return ivf_flat.IndexParams(metric=metric, n_lists=16, kmeans_n_iters=10)
    return ivf_pq.IndexParams(metric=metric, n_lists=16, pq_dim=8, kmeans_n_iters=10)


def _search_params(algo, **kw):
    from cuvs_amd.neighbors import cagra, ivf_flat, ivf_pq

    return {"cagra": cagra.SearchParams, "ivf_flat": ivf_flat.SearchParams, "ivf_pq": ivf_pq.SearchParams}[algo](**kw)


def _check_composition(res, T, idx, sp, rows, q, k, metric, keep=None, standalone=None):
    """search == merge(A, B) with A, B from search_tiers; B == the oracle on the tail; with a filter no cleared id comes back."""
    select_min = metric != "inner_product"
    size, ann_rows, _, _ = T.info(idx)
    assert size == len(rows)
    flt = None if keep is None else _words(keep)
    ad, ai, td, ti = (x.cpu().numpy() for x in T.search_tiers(sp, idx, _dev(q), k, resources=res, filter=flt))
    got = T.search(sp, idx, _dev(q), k, resources=res, filter=flt)
    _assert_same(got, R.merge((ad, ai), (td, ti), ann_rows, select_min), "search vs merge(A, B)")
    tail = rows[ann_rows:]
    if len(tail):
        tb = None if keep is None else R.tail_bits(R.pack_bits(keep), ann_rows, len(tail))
        want_b = R.globalize(*oracle.brute_force_knn(q, tail, k, metric, keep_bits=tb), ann_rows, select_min)
        _assert_same((td, ti), want_b, "B vs the oracle on the tail")
    else:
        assert (ti == R.I64_MAX).all() and (td == R.worst(select_min)).all()
    gi = got[1].cpu().numpy()
    real = gi != R.I64_MAX
    assert ((gi[real] >= 0) & (gi[real] < size)).all()
    if keep is not None:
        assert keep[gi[real]].all(), "a filtered id came back"
    alone = None if standalone is None else standalone(k, flt)
    if alone is not None:
        _assert_same((ad, ai), alone, "A vs the standalone ANN index")
    return got


@pytest.mark.parametrize("algo", ["cagra", "ivf_flat", "ivf_pq"])
@pytest.mark.parametrize("metric", ["sqeuclidean", "inner_product"])
def test_composition_through_build_and_extends(res, algo, metric):
    import torch

    from cuvs_amd.neighbors import ivf_flat, ivf_pq, tiered_index as T

    rows = _rows(600 + 1 + 1 + 1 + 130 + 40, 16, 11)
    q = _rows(33, 16, 12)
    up = _upstream(algo, metric)
    params = T.IndexParams(metric=metric, algo=algo, upstream_params=up, min_ann_rows=500, create_ann_index_on_extend=False)
    idx = T.build(params, _dev(rows[:600]), resources=res)
    assert T.info(idx) == (600, 600, 637, 16)
    sp = _search_params(algo, n_probes=16) if algo != "cagra" else _search_params(algo)
    standalone = None
    if algo == "ivf_flat":
        # the IVF-Flat build is deterministic: the ANN tier answers as a standalone index over the same rows
        ref_idx = ivf_flat.build(up, _dev(rows[:600]), resources=res)
        standalone = lambda k, flt: tuple(  # noqa: E731
            x.cpu().numpy() for x in ivf_flat.search(sp, ref_idx, _dev(q), k, resources=res, filter=None if flt is None else (flt, 1)))
    if algo == "ivf_pq":
        # two standalone IVF-PQ builds of the same rows: reproducible run to run here (fixed seeds), so the tier is compared too
        ref_idx = ivf_pq.build(up, _dev(rows[:600]), resources=res)
        ref2 = ivf_pq.build(up, _dev(rows[:600]), resources=res)
        a1 = ivf_pq.search(sp, ref_idx, _dev(q), 10, resources=res)
        a2 = ivf_pq.search(sp, ref2, _dev(q), 10, resources=res)
        assert torch.equal(a1[1], a2[1]) and torch.equal(a1[0].view(torch.int32), a2[0].view(torch.int32))
        standalone = lambda k, flt: (  # noqa: E731  (unfiltered searches only: ivf_pq.search takes no filter)
            tuple(x.cpu().numpy() for x in ivf_pq.search(sp, ref_idx, _dev(q), k, resources=res)) if flt is None else None)
    rng = np.random.default_rng(5)
    size = 600
    steps = [(1, "device"), (1, "device"), (1, "device"), (130, "device"), (40, "host")]
    caps = [637, 637, 637, 1274, 1274]  # max(size + new_rows, 2 * capacity) when the rows do not fit
    _check_composition(res, T, idx, sp, rows[:size], q, 10, metric, standalone=standalone)
    for (n_new, where), cap in zip(steps, caps):
        new = rows[size:size + n_new]
        T.extend(idx, _dev(new) if where == "device" else new, resources=res)
        size += n_new
        assert T.info(idx) == (size, 600, cap, 16)
        for keep in (None, rng.random(size) < 0.4):
            _check_composition(res, T, idx, sp, rows[:size], q, 10, metric, keep=keep, standalone=standalone)
    # (the growth step above is the dangling-pointer case of CAGRA: the tier was re-pointed at the new allocation)
    for keep in (None, rng.random(size) < 0.4):
        _check_composition(res, T, idx, sp, rows[:size], q, 64, metric, keep=keep, standalone=standalone)


def test_ivf_flat_with_all_lists_probed_is_exact_on_integer_rows(res):
    """Integer-valued rows: every squared distance is exactly representable, so with n_probes = n_lists the tiered result has
    the distances of the fp64 ground truth, no case left out."""
    from cuvs_amd.neighbors import ivf_flat, tiered_index as T

    rows = _rows(773, 16, 21, ties=True)
    q = _rows(33, 16, 22, ties=True)
    up = ivf_flat.IndexParams(n_lists=16, kmeans_n_iters=10)
    idx = T.build(T.IndexParams(algo="ivf_flat", upstream_params=up, min_ann_rows=500), _dev(rows[:600]), resources=res)
    T.extend(idx, _dev(rows[600:]), resources=res)
    assert T.info(idx)[:2] == (773, 600)
    d, i = (x.cpu().numpy() for x in T.search(ivf_flat.SearchParams(n_probes=16), idx, _dev(q), 10, resources=res))
    full = ((q.astype(np.float64)[:, None, :] - rows.astype(np.float64)[None, :, :]) ** 2).sum(2)
    assert (d.astype(np.float64) == np.sort(full, axis=1)[:, :10]).all()
    assert (np.take_along_axis(full, i, 1) == d).all()
    # ties: (distance, id) ascending
    assert all((d[r, j], i[r, j]) < (d[r, j + 1], i[r, j + 1]) for r in range(len(q)) for j in range(9))


# ---------------------------------------------------------------------------------------------------- 3. thresholds
@pytest.mark.parametrize("algo", ["cagra", "ivf_flat", "ivf_pq"])
def test_thresholds(res, algo):
    from cuvs_amd.neighbors import brute_force, tiered_index as T

    rows = _rows(502, 16, 31)
    q = _rows(9, 16, 32)
    params = T.IndexParams(algo=algo, upstream_params=_upstream(algo, "sqeuclidean"), min_ann_rows=500,
                           create_ann_index_on_extend=True)
    idx = T.build(params, _dev(rows[:500]), resources=res)
    assert T.info(idx) == (500, 0, 531, 16)  # 500 is not more than 500: all tail
    # a tail-only index answers as cuvsBruteForceSearch on the same rows, padding and all (k = 10 and k beyond the rows)
    bf = brute_force.build(_dev(rows[:500]), resources=res)
    for k in (10, 600):
        got = T.search(None, idx, _dev(q), k, resources=res)
        want = brute_force.search(bf, _dev(q), k, resources=res)
        _assert_same(got, tuple(x.cpu().numpy() for x in want), "tail-only vs brute force")
    ad, ai, td, ti = T.search_tiers(None, idx, _dev(q), 10, resources=res)
    assert (ai.cpu().numpy() == R.I64_MAX).all() and (ad.cpu().numpy() == R.F32_MAX).all()
    T.extend(idx, _dev(rows[500:501]), resources=res)
    assert T.info(idx) == (501, 501, 531, 16)  # 501 > 500: compacted
    T.compact(idx, resources=res)  # an empty tail: nothing happens
    assert T.info(idx) == (501, 501, 531, 16)
    T.extend(idx, _dev(rows[501:502]), resources=res)
    assert T.info(idx) == (502, 501, 531, 16)
    T.compact(idx, resources=res)
    assert T.info(idx) == (502, 502, 531, 16)
    idx2 = T.build(params, rows[:501], resources=res)  # host rows; an ANN tier at once
    assert T.info(idx2) == (501, 501, 532, 16)


# ---------------------------------------------------------------------------------------------------- 4. merge
@pytest.mark.parametrize("algo", ["cagra", "ivf_flat", "ivf_pq"])
def test_merge(res, algo):
    from cuvs_amd.neighbors import tiered_index as T

    metric = "sqeuclidean"
    rows = _rows(1000, 16, 41)
    q = _rows(33, 16, 42)
    up = _upstream(algo, metric)
    p500 = T.IndexParams(algo=algo, upstream_params=up, min_ann_rows=500)
    a = T.build(p500, _dev(rows[:600]), resources=res)
    b = T.build(p500, _dev(rows[600:]), resources=res)
    assert T.info(a)[:2] == (600, 600) and T.info(b)[:2] == (400, 0)
    sp = _search_params(algo, n_probes=16) if algo != "cagra" else _search_params(algo)
    a_alone = tuple(x.cpu().numpy() for x in T.search(sp, a, _dev(q), 10, resources=res))

    p2000 = T.IndexParams(algo=algo, upstream_params=up, min_ann_rows=2000)
    mrg = T.merge(p2000, [a, b], resources=res)
    assert T.info(mrg) == (1000, 600, 1000, 16)  # the ANN tier of the first is kept, the second's rows are tail
    _check_composition(res, T, mrg, sp, rows, q, 10, metric)
    ad, ai, td, ti = (x.cpu().numpy() for x in T.search_tiers(sp, mrg, _dev(q), 10, resources=res))
    _assert_same((ad, ai), a_alone, "the kept ANN tier")
    assert (ti >= 600).all()  # ids of the second index are shifted by 600
    # extending the merged index past its (exact) capacity must not disturb the shared tier of `a`
    T.extend(mrg, _dev(rows[:5]), resources=res)
    assert T.info(mrg) == (1005, 600, 2000, 16)
    _check_composition(res, T, mrg, sp, np.concatenate([rows, rows[:5]]), q, 10, metric)
    _assert_same(T.search(sp, a, _dev(q), 10, resources=res), a_alone, "`a` after the merged index grew")

    p300 = T.IndexParams(algo=algo, upstream_params=up, min_ann_rows=300, create_ann_index_on_extend=False)
    cmp_ = T.merge(p300, [a, b], resources=res)
    assert T.info(cmp_)[:2] == (1000, 1000)  # 400 > 300: compacted, whatever create_ann_index_on_extend says
    _check_composition(res, T, cmp_, sp, rows, q, 10, metric)

    one = T.merge(p2000, [a], resources=res)
    assert T.info(one) == T.info(a)
    _assert_same(T.search(sp, one, _dev(q), 10, resources=res), a_alone, "merge of one index")
    T.extend(one, _dev(rows[600:610]), resources=res)  # the copy grows on its own
    assert T.info(one)[:2] == (610, 600) and T.info(a)[:2] == (600, 600)

    # into a handle that already holds an index: the old one is freed, the handle answers as the merged one
    T.merge(p2000, [a, b], resources=res, output=one)
    assert T.info(one) == (1000, 600, 1000, 16)
    _check_composition(res, T, one, sp, rows, q, 10, metric)

    other_dim = T.build(p500, _dev(_rows(50, 8, 43)), resources=res)
    with pytest.raises(Exception, match="indices must all have the same dimensionality"):
        T.merge(p2000, [a, other_dim], resources=res)
    other_algo = "ivf_flat" if algo != "ivf_flat" else "ivf_pq"
    c = T.build(T.IndexParams(algo=other_algo, min_ann_rows=500), _dev(rows[:100]), resources=res)
    with pytest.raises(Exception, match="indices must all have the same index algorithm"):
        T.merge(p2000, [a, c], resources=res)
    with pytest.raises(Exception, match="must have at least one index to merge"):
        T.merge(p2000, [], resources=res)


# ---------------------------------------------------------------------------------------------------- 5. refusals
def test_refusals(res):
    import torch

    from cuvs_amd._lib import BITMAP
    from cuvs_amd.neighbors import tiered_index as T

    rows = _rows(100, 16, 51)
    p = T.IndexParams(algo="ivf_flat", min_ann_rows=500)
    with pytest.raises(Exception, match="Unsupported dataset DLtensor dtype: 2 and bits: 16"):
        T.build(p, _dev(rows).half(), resources=res)
    with pytest.raises(Exception, match="Unsupported dataset DLtensor dtype: 0 and bits: 8"):
        T.build(p, _dev(rows).to(torch.int8), resources=res)
    with pytest.raises(Exception, match="unsupported metric"):
        T.build(T.IndexParams(metric="l1", algo="ivf_flat"), _dev(rows), resources=res)
    idx = T.build(p, _dev(rows), resources=res)
    with pytest.raises(Exception, match="Dimension of new vectors must match existing data"):
        T.extend(idx, _dev(_rows(3, 8, 52)), resources=res)
    with pytest.raises(Exception, match="Unsupported dataset DLtensor dtype: 2 and bits: 16"):
        T.extend(idx, _dev(rows[:3]).half(), resources=res)
    assert T.info(idx) == (100, 0, 106, 16)
    q = _dev(_rows(4, 16, 53))
    words = _words(np.ones(100, bool))
    with pytest.raises(Exception, match="Unsupported filter type: BITMAP"):
        T.search(None, idx, q, 5, resources=res, filter=(words, BITMAP))
    with pytest.raises(Exception, match="neighbors should be of type int64_t"):
        T.search(None, idx, q, 5, neighbors=torch.empty((4, 5), dtype=torch.int32, device="cuda"), resources=res)
    with pytest.raises(Exception, match="distances should be of type float32"):
        T.search(None, idx, q, 5, distances=torch.empty((4, 5), dtype=torch.float64, device="cuda"), resources=res)
    with pytest.raises(Exception, match="type mismatch between index and queries"):
        T.search(None, idx, q.to(torch.int8), 5, resources=res)
    with pytest.raises(Exception, match="bitset filter holds 96 bits, the index 100 rows"):
        T.search(None, idx, q, 5, resources=res, filter=words[:3])
    with pytest.raises(Exception, match="not built"):
        T.info(T.Index())
    with pytest.raises(ValueError, match="Index needs to be built"):
        T.search(None, T.Index(), q, 5, resources=res)
    # the upstream search's own refusal comes through unchanged: IVF-PQ takes no k beyond its rows
    pq = T.build(T.IndexParams(algo="ivf_pq", upstream_params=_upstream("ivf_pq", "sqeuclidean"), min_ann_rows=50), _dev(rows),
                 resources=res)
    T.extend(pq, _dev(rows[:4]), resources=res)
    from cuvs_amd.neighbors import ivf_pq

    with pytest.raises(Exception) as tiered_err:
        T.search(None, pq, q, 200, resources=res)
    standalone = ivf_pq.build(_upstream("ivf_pq", "sqeuclidean"), _dev(rows), resources=res)
    with pytest.raises(Exception) as own_err:
        ivf_pq.search(ivf_pq.SearchParams(), standalone, q, 200, resources=res)
    assert str(tiered_err.value).split(" (")[0] == str(own_err.value).split(" (")[0]


# ---------------------------------------------------------------------------------------------------- the Python surface
def test_python_surface_equals_the_c_calls(res):
    """build / extend / search / merge / compact through cuvs_amd.neighbors.tiered_index with torch tensors, against the same
    calls made on the C ABI by hand."""
    import torch

    from cuvs_amd._lib import NO_FILTER, Tensor, check, cuvsFilter, lib
    from cuvs_amd.neighbors import ivf_flat, tiered_index as T

    rows = torch.from_numpy(_rows(700, 16, 61)).cuda()
    q = torch.from_numpy(_rows(12, 16, 62)).cuda()
    up = ivf_flat.IndexParams(n_lists=8, kmeans_n_iters=10)
    params = T.IndexParams(algo="ivf_flat", upstream_params=up, min_ann_rows=300)
    sp = ivf_flat.SearchParams(n_probes=8)

    idx = T.build(params, rows[:400], resources=res)
    T.extend(idx, rows[400:500], resources=res)
    other = T.build(params, rows[500:], resources=res)
    mrg = T.merge(T.IndexParams(algo="ivf_flat", upstream_params=up, min_ann_rows=1000), [idx, other], resources=res)
    assert idx.trained and mrg.trained and T.info(mrg)[:2] == (700, 400)
    d1, n1 = T.search(sp, mrg, q, 10, resources=res)
    T.compact(mrg, resources=res)
    assert T.info(mrg)[:2] == (700, 700)
    d2, n2 = T.search(sp, mrg, q, 10, resources=res)

    L = lib()
    h = res.get_c_obj()
    cp = C.POINTER(T._CIndexParams)()
    check(L.cuvsTieredIndexParamsCreate(C.byref(cp)))
    cp.contents.algo, cp.contents.min_ann_rows = 1, 300
    cp.contents.ivf_flat_params = C.cast(up._p, C.c_void_p)
    ci, co, cm = (C.POINTER(T._CIndex)() for _ in range(3))
    for x in (ci, co, cm):
        check(L.cuvsTieredIndexCreate(C.byref(x)))
    check(L.cuvsTieredIndexBuild(h, cp, Tensor(rows[:400].contiguous()).ptr, ci))
    check(L.cuvsTieredIndexExtend(h, Tensor(rows[400:500].contiguous()).ptr, ci))
    check(L.cuvsTieredIndexBuild(h, cp, Tensor(rows[500:].contiguous()).ptr, co))
    cp.contents.min_ann_rows = 1000
    arr = (C.POINTER(T._CIndex) * 2)(ci, co)
    L.cuvsTieredIndexMerge.argtypes = [C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    check(L.cuvsTieredIndexMerge(h, C.cast(cp, C.c_void_p), C.cast(arr, C.c_void_p), 2, C.cast(cm, C.c_void_p)))
    L.cuvsTieredIndexSearch.argtypes = [C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, cuvsFilter]

    def c_search():
        nb = torch.empty((12, 10), dtype=torch.int64, device="cuda")
        ds = torch.empty((12, 10), dtype=torch.float32, device="cuda")
        check(L.cuvsTieredIndexSearch(h, C.cast(sp._p, C.c_void_p), cm, Tensor(q).ptr, Tensor(nb).ptr, Tensor(ds).ptr,
                                      cuvsFilter(0, NO_FILTER)))
        res.sync()
        return ds, nb

    _assert_same((d1, n1), tuple(x.cpu().numpy() for x in c_search()), "before compact")
    check(L.cuvsAmdTieredIndexCompact(h, cm))
    _assert_same((d2, n2), tuple(x.cpu().numpy() for x in c_search()), "after compact")
    for x in (ci, co, cm):
        check(L.cuvsTieredIndexDestroy(x))
    check(L.cuvsTieredIndexParamsDestroy(cp))
