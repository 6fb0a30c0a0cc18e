"""GPU: cuvsIvfFlat* through the C ABI.

* search parity: GPU search vs the CPU oracle searching the SAME exported index — identical ids/distances;
* recall >= n_probes / n_lists, the reference's threshold (cpp/tests/neighbors/ann_ivf_flat.cuh:102), on its
  input shapes (:524-...: n=10000, q=1000, dims incl. odd ones, k 10/16, n_lists 1024-ish scaled down);
* structural invariants (every id once, ascending in-list order), extend, dtypes.
"""
import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu


def _gen(n, d, q, seed, dtype=np.float32):
    rng = np.random.default_rng(seed)
    if dtype in (np.int8, np.uint8):
        return (rng.integers(1, 20, size=(n, d)).astype(dtype), rng.integers(1, 20, size=(q, d)).astype(dtype))
    x = (rng.random((n, d), dtype=np.float32) * 1.9 + 0.1).astype(dtype)
    qq = (rng.random((q, d), dtype=np.float32) * 1.9 + 0.1).astype(dtype)
    return x, qq


def _build(x, **kw):
    import torch
    from cuvs_amd.neighbors import ivf_flat

    return ivf_flat.build(ivf_flat.IndexParams(**kw), torch.from_numpy(x).cuda())


def _search(index, q, k, n_probes):
    import torch
    from cuvs_amd.neighbors import ivf_flat

    d, i = ivf_flat.search(ivf_flat.SearchParams(n_probes=n_probes), index, torch.from_numpy(q).cuda(), k)
    torch.cuda.synchronize()
    return d.cpu().numpy(), i.cpu().numpy()


@pytest.mark.parametrize("metric", ["sqeuclidean", "euclidean", "inner_product"])
@pytest.mark.parametrize("n,d,n_lists,k,n_probes", [(10000, 16, 64, 10, 8), (5000, 33, 32, 16, 5), (3000, 1, 16, 4, 16),
                                                    (4000, 128, 16, 100, 4), (2000, 257, 8, 7, 3)])
def test_search_parity_with_oracle_on_same_index(metric, n, d, n_lists, k, n_probes):
    from cuvs_amd.neighbors import ivf_flat

    x, q = _gen(n, d, 150, seed=n + d)
    index = _build(x, n_lists=n_lists, metric=metric, kmeans_n_iters=10)
    gd, gi = _search(index, q, k, n_probes)
    ex = ivf_flat.export_for_oracle(index, np.float32)
    od, oi = oracle.ivf_flat_search(ex, q, k, n_probes, metric=metric)
    assert (gi == oi).all(), f"id mismatch rate {(gi != oi).mean():.4f}"
    assert (gd == od).all(), f"max |d| diff {np.abs(gd - od).max()}"


@pytest.mark.parametrize("dtype,scale", [(np.float16, 1.0), (np.int8, 1 / 128), (np.uint8, 1 / 256)])
def test_other_dtypes_parity(dtype, scale):
    from cuvs_amd.neighbors import ivf_flat

    x, q = _gen(6000, 40, 100, seed=9, dtype=dtype)
    index = _build(x, n_lists=24, kmeans_n_iters=10)
    gd, gi = _search(index, q, 10, 6)
    ex = ivf_flat.export_for_oracle(index, dtype)
    od, oi = oracle.ivf_flat_search(ex, q, 10, 6, coarse_scale=scale)
    assert (gi == oi).all() and (gd == od).all()


@pytest.mark.parametrize("dtype,scale", [(np.int8, 1 / 128), (np.uint8, 1 / 256)])
@pytest.mark.parametrize("metric", ["sqeuclidean", "inner_product"])
@pytest.mark.parametrize("dim", [2500, 37])
def test_int8_integer_accumulation(dtype, scale, metric, dim):
    """int8 / uint8 rows: the reference accumulates in 32-bit integers (dp4a, metric_impl.cuh:12-49) and converts the
    exact sum once. Full-range values at dim 2500 give sums far beyond 2^24, where an fp32 chain would round at every
    step: ids and distances equal the integer oracle. dim 37: a partial last chunk."""
    from cuvs_amd.neighbors import ivf_flat

    rng = np.random.default_rng(dim)
    lo, hi = (-128, 128) if dtype == np.int8 else (0, 256)
    x = rng.integers(lo, hi, size=(3000, dim)).astype(dtype)
    q = rng.integers(lo, hi, size=(60, dim)).astype(dtype)
    x[10] = x[2000]  # ties
    index = _build(x, n_lists=12, metric=metric, kmeans_n_iters=10)
    gd, gi = _search(index, q, 10, 5)
    ex = ivf_flat.export_for_oracle(index, dtype)
    od, oi = oracle.ivf_flat_search(ex, q, 10, 5, metric=metric, coarse_scale=scale)
    assert (gi == oi).all() and (gd == od).all()
    if metric == "sqeuclidean" and dim == 2500:
        exact = ((x[gi[:, 0]].astype(np.int64) - q.astype(np.int64)) ** 2).sum(1)
        assert exact.max() > 2 ** 24 and (gd[:, 0] == exact.astype(np.float32)).all()


def test_recall_threshold_and_structure():
    from cuvs_amd.neighbors import ivf_flat

    n, d, nq, k, n_lists, n_probes = 10000, 32, 1000, 16, 128, 40
    x, q = _gen(n, d, nq, seed=1234)
    index = _build(x, n_lists=n_lists)
    gd, gi = _search(index, q, k, n_probes)
    td, ti = oracle.exact_knn(q, x, k)
    r = oracle.recall(gi, ti)
    assert r >= n_probes / n_lists, r  # ann_ivf_flat.cuh:102
    assert r > 0.8  # uniform random data: recall tracks the probed fraction
    # found neighbours carry exact distances (flat index): compare where ids agree
    same = gi == ti
    np.testing.assert_allclose(gd[same], td[same], rtol=1e-4, atol=1e-4)
    ex = ivf_flat.export_for_oracle(index, np.float32)
    assert ex["list_sizes"].sum() == n
    all_ids = np.concatenate(ex["ids"])
    assert np.array_equal(np.sort(all_ids), np.arange(n))
    for ids, rows in zip(ex["ids"], ex["rows"]):
        assert (np.diff(ids) > 0).all()
        assert (rows == x[ids]).all()  # lists hold the original vectors bit for bit


def test_probe_all_lists_equals_exact_search():
    x, q = _gen(3000, 24, 64, seed=4)
    index = _build(x, n_lists=16)
    gd, gi = _search(index, q, 10, 16)
    td, ti = oracle.exact_knn(q, x, 10)
    assert oracle.recall(gi, ti) > 0.999


def test_extend():
    import torch
    from cuvs_amd.neighbors import ivf_flat

    x, q = _gen(5000, 20, 80, seed=6)
    index = _build(x[:3000], n_lists=16)
    ivf_flat.extend(index, torch.from_numpy(x[3000:]).cuda(), torch.arange(3000, 5000, dtype=torch.int64, device="cuda"))
    gd, gi = _search(index, q, 10, 16)
    td, ti = oracle.exact_knn(q, x, 10)
    assert oracle.recall(gi, ti) > 0.999
    ex = ivf_flat.export_for_oracle(index, np.float32)
    assert np.array_equal(np.sort(np.concatenate(ex["ids"])), np.arange(5000))


@pytest.mark.parametrize("dtype", [np.float32, np.int8])
def test_extend_halves_give_the_lists_file_and_results_of_one_build(dtype, tmp_path):
    """One build over all rows (A), an empty index extended twice by halves from device tensors (B) and from host rows
    with host ids (C): the same lists, the same file byte for byte, the same search results bit for bit. dim 20 leaves a
    padded last chunk for both types (4 and 16 elements per chunk), list sizes are no multiples of 64 and the second
    extend moves every list."""
    import torch
    from cuvs_amd.neighbors import ivf_flat

    x, q = _gen(5000, 20, 80, seed=6, dtype=dtype)
    xt = torch.from_numpy(x).cuda()
    a = _build(x, n_lists=16)
    b = _build(x, n_lists=16, add_data_on_build=False)
    c = _build(x, n_lists=16, add_data_on_build=False)
    assert ivf_flat.export_for_oracle(b, dtype)["list_sizes"].sum() == 0
    for lo, hi in ((0, 2500), (2500, 5000)):
        ivf_flat.extend(b, xt[lo:hi], torch.arange(lo, hi, dtype=torch.int64, device="cuda"))
        ivf_flat.extend(c, x[lo:hi], np.arange(lo, hi, dtype=np.int64))
    ea = ivf_flat.export_for_oracle(a, dtype)
    assert (ea["list_sizes"] % 64 != 0).any() and ea["list_sizes"].sum() == 5000
    da, ia = _search(a, q, 10, 5)
    ivf_flat.save(str(tmp_path / "a.bin"), a)
    file_a = open(tmp_path / "a.bin", "rb").read()
    for name, other in (("b", b), ("c", c)):
        eo = ivf_flat.export_for_oracle(other, dtype)
        assert np.array_equal(ea["list_sizes"], eo["list_sizes"]), name
        for L in range(16):
            assert np.array_equal(ea["ids"][L], eo["ids"][L]) and np.array_equal(ea["rows"][L], eo["rows"][L]), (name, L)
        ivf_flat.save(str(tmp_path / f"{name}.bin"), other)
        assert open(tmp_path / f"{name}.bin", "rb").read() == file_a, name
        do, io = _search(other, q, 10, 5)
        assert np.array_equal(ia, io) and np.array_equal(da.view(np.uint32), do.view(np.uint32)), name


def test_host_dataset_build():
    from cuvs_amd.neighbors import ivf_flat

    x, q = _gen(4000, 16, 50, seed=8)
    index = ivf_flat.build(ivf_flat.IndexParams(n_lists=16), x)  # numpy (host) dataset, as the reference allows
    gd, gi = _search(index, q, 5, 16)
    _, ti = oracle.exact_knn(q, x, 5)
    assert oracle.recall(gi, ti) > 0.999


@pytest.mark.parametrize("dtype", [np.float32, np.float16])
@pytest.mark.parametrize("n,d,n_lists,k,n_probes", [(8000, 24, 32, 10, 6), (3000, 130, 16, 20, 16)])
def test_cosine_parity_and_recall(dtype, n, d, n_lists, k, n_probes):
    """CosineExpanded (ivf_flat_search.cuh:130-175 coarse, interleaved scan with in-kernel row norms,
    post-process 1 - cos): bit-identical to the oracle on the same index, and correct against numpy."""
    from cuvs_amd.neighbors import ivf_flat

    x, q = _gen(n, d, 120, seed=n + d, dtype=dtype)
    index = _build(x, n_lists=n_lists, metric="cosine", kmeans_n_iters=10)
    gd, gi = _search(index, q, k, n_probes)
    ex = ivf_flat.export_for_oracle(index, dtype)
    od, oi = oracle.ivf_flat_search(ex, q, k, n_probes, metric="cosine")
    assert (gi == oi).all(), f"id mismatch rate {(gi != oi).mean():.4f}"
    assert (gd == od).all(), f"max |d| diff {np.abs(gd - od).max()}"
    # against float64 numpy: distances are 1 - cos of the returned ids; probing every list is exact search
    xf, qf = x.astype(np.float64), q.astype(np.float64)
    cosd = 1.0 - (qf @ xf.T) / (np.linalg.norm(qf, axis=1)[:, None] * np.linalg.norm(xf, axis=1)[None, :])
    np.testing.assert_allclose(gd, np.take_along_axis(cosd, gi, axis=1), rtol=1e-3, atol=2e-3)
    if n_probes == n_lists:
        truth = np.argsort(cosd, axis=1, kind="stable")[:, :k]
        assert oracle.recall(gi, truth) > 0.99


@pytest.mark.parametrize("metric", ["sqeuclidean", "inner_product"])
def test_large_k_non_fused_path(metric):
    """k > 256: the reference leaves its fused top-k for "write every score + select_k" (ivf_flat_search.cuh:180,283);
    so does this library - results identical to the oracle, including the padding when fewer than k rows are probed."""
    from cuvs_amd.neighbors import ivf_flat

    x, q = _gen(6000, 24, 40, seed=5)
    index = _build(x, n_lists=16, metric=metric, kmeans_n_iters=10)
    ex = ivf_flat.export_for_oracle(index, np.float32)
    for k, n_probes in ((512, 6), (1000, 2), (300, 16)):
        gd, gi = _search(index, q, k, n_probes)
        od, oi = oracle.ivf_flat_search(ex, q, k, n_probes, metric=metric)
        assert (gi == oi).all() and (gd == od).all(), (k, n_probes)


def test_inner_product_on_unnormalised_rows():
    """The lists are trained, filled and probed with the SAME metric (ivf_flat_build.cuh:188,438): with an L2-trained
    coarse quantizer the inner-product probes were not the lists the rows had been assigned to. Every row must sit in
    the list whose centre has the largest dot product."""
    from cuvs_amd.neighbors import ivf_flat

    rng = np.random.default_rng(8)
    x = (rng.standard_normal((20000, 32)) * rng.uniform(0.2, 3.0, size=(20000, 1))).astype(np.float32)  # norms vary 15x
    q = rng.standard_normal((300, 32)).astype(np.float32)
    index = _build(x, n_lists=64, metric="inner_product", kmeans_n_iters=20)
    ex = ivf_flat.export_for_oracle(index, np.float32)
    centers = ex["centers"]
    for L in range(0, 64, 7):
        rows = ex["rows"][L]
        if len(rows):
            assert (np.argmax(rows @ centers.T, axis=1) == L).mean() > 0.999
    gd, gi = _search(index, q, 10, 8)
    _, ti = oracle.brute_force_knn(q, x, 10, metric="inner_product")
    # the reference's own bar is recall >= n_probes / n_lists (ann_ivf_flat.cuh:102); isotropic rows with norms spread
    # 15x are a hard case for maximum-inner-product search with 8 of 64 lists
    assert oracle.recall(gi, ti) >= 0.4, oracle.recall(gi, ti)
    od, oi = oracle.ivf_flat_search(ex, q, 10, 8, metric="inner_product")
    assert (gi == oi).all() and (gd == od).all()


# ------------------------------------------------------------------------------------------------ scan-kernel grid
# The admission and merge code of the list scan (cuvs_amd/csrc/ivf_list_scan.hpp) through IVF-Flat's kernels: the edges of the
# one-slot lists (k <= 64), the four-slot lists (k <= 256) and the non-fused path, every element type, planted ties, a filter.
_DTYPES = {"f32": (np.float32, 1.0), "f16": (np.float16, 1.0), "i8": (np.int8, 1 / 128), "u8": (np.uint8, 1 / 256)}


def _dup_data(n, d, nq, seed, dtype, dup):
    x, q = _gen(n, d, nq, seed, dtype)
    x[n - dup:] = x[:dup]  # duplicated rows: exact ties of every metric
    q[:5] = x[:5]          # queries equal to (duplicated) rows
    return x, q


def _grid_cases():
    ks = [1, 10, 64, 65, 256, 257]
    names = list(_DTYPES)
    out, n = [], 0
    for metric in ("sqeuclidean", "euclidean", "inner_product", "cosine"):
        for dim in (1, 3, 16, 17, 33, 128, 257):
            if metric == "cosine" and dim == 1:
                dim = 2
            k, dt, filt = ks[n % len(ks)], names[n % len(names)], n % 2 == 1
            out.append(pytest.param(metric, dim, k, dt, filt, id=f"{metric}-d{dim}-k{k}-{dt}{'-filter' if filt else ''}"))
            n += 1
    return out


def _probe_ranks(ex, q, n_probes, metric, scale):
    """[n_queries, n_lists] rank of every list among a query's probes (n_lists: not probed), from the oracle itself: the
    index cut down to the first row of every list, its id the list number, searched with 1 .. n_probes probes"""
    sizes = np.minimum(ex["list_sizes"], 1)
    cut = dict(ex, list_sizes=sizes, rows=[r[:1] for r in ex["rows"]],
               ids=[np.full(int(c), L, np.int64) for L, c in enumerate(sizes)])
    rank = np.full((len(q), len(sizes)), len(sizes), np.int64)
    for p in range(n_probes, 0, -1):  # a list probed with p probes has rank < p: the smallest such p - 1 stays
        _, oi = oracle.ivf_flat_search(cut, q, p, p, metric=metric, coarse_scale=scale)
        for r in range(len(q)):
            rank[r, oi[r][oi[r] != np.iinfo(np.int64).max]] = p - 1
    return rank


def _oracle_filtered(ex, q, k, n_probes, metric, scale, keep, n):
    """The oracle's ranking of every probed row (k = n: each once, ordered by (distance, flat row), then padding) with the
    masked ids dropped, and the k best of it. Which rows of equal distance make it across the k-th place is decided as the
    search decides it (ivf_common.hpp, oracle_ivf_flat.c): by probe rank, then by position in the list - with integer rows
    such ties between rows of different lists are common. The winners keep the oracle's order."""
    od, oi = oracle.ivf_flat_search(ex, q, n, n_probes, metric=metric, coarse_scale=scale)
    rank = _probe_ranks(ex, q, n_probes, metric, scale)
    list_of = np.empty(n, np.int64)
    for L, ids in enumerate(ex["ids"]):
        assert (np.diff(ids) > 0).all(), "in-list order is ascending id: ids stand in for the position in the list below"
        list_of[ids] = L
    wd = np.full((len(q), k), np.finfo(np.float32).max, np.float32)
    wi = np.full((len(q), k), np.iinfo(np.int64).max, np.int64)
    for r in range(len(q)):
        found = oi[r] != np.iinfo(np.int64).max
        pos = np.nonzero(found & keep[np.where(found, oi[r], 0)])[0]
        d, ids = od[r, pos], oi[r, pos]
        group = np.concatenate([[0], np.cumsum(d[1:] != d[:-1])])  # runs of equal distance, best first
        sel = np.sort(np.lexsort((ids, rank[r, list_of[ids]], group))[:k])  # (in-list order is ascending id)
        wd[r, :len(sel)], wi[r, :len(sel)] = d[sel], ids[sel]
    return wd, wi


@pytest.mark.parametrize("metric,dim,k,dt,filt", _grid_cases())
def test_search_parity_grid(metric, dim, k, dt, filt):
    import torch
    from cuvs_amd._lib import BITSET
    from cuvs_amd.neighbors import ivf_flat

    n, n_lists, n_probes, nq = 4000, 20, 6, 60
    dtype, scale = _DTYPES[dt]
    x, q = _dup_data(n, dim, nq, 100 + dim, dtype, 400)
    index = _build(x, n_lists=n_lists, metric=metric, kmeans_n_iters=10)
    ex = ivf_flat.export_for_oracle(index, dtype)
    if filt:
        keep = np.random.default_rng(dim).random(n) < 0.7
        bits = np.zeros((n + 31) // 32, np.uint32)
        np.bitwise_or.at(bits, np.nonzero(keep)[0] >> 5, (np.uint32(1) << (np.nonzero(keep)[0] & 31).astype(np.uint32)))
        gd, gi = ivf_flat.search(ivf_flat.SearchParams(n_probes=n_probes), index, torch.from_numpy(q).cuda(), k,
                                 filter=(torch.from_numpy(bits.view(np.int32)).cuda(), BITSET))
        torch.cuda.synchronize()
        gd, gi = gd.cpu().numpy(), gi.cpu().numpy()
        wd, wi = _oracle_filtered(ex, q, k, n_probes, metric, scale, keep, n)
    else:
        gd, gi = _search(index, q, k, n_probes)
        wd, wi = oracle.ivf_flat_search(ex, q, k, n_probes, metric=metric, coarse_scale=scale)
    assert np.array_equal(gi, wi), f"ids differ in {np.count_nonzero((gi != wi).any(1))} rows"
    assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32)), "distances differ"


@pytest.mark.parametrize("dt", ["f32", "i8"])
def test_search_many_probes_two_phase(dt):
    """n_probes > 8 (L2: the nearest list of every query is scanned first) with fewer than 256 queries, which keeps the
    matrix-core tail phase out: head and tail both run on the scan kernel, with several work items per list"""
    from cuvs_amd.neighbors import ivf_flat

    dtype, scale = _DTYPES[dt]
    x, q = _dup_data(6000, 40, 200, 5, dtype, 300)
    index = _build(x, n_lists=24, kmeans_n_iters=10)
    ex = ivf_flat.export_for_oracle(index, dtype)
    for k in (10, 100):
        gd, gi = _search(index, q, k, 12)
        wd, wi = oracle.ivf_flat_search(ex, q, k, 12, coarse_scale=scale)
        assert np.array_equal(gi, wi) and np.array_equal(gd.view(np.uint32), wd.view(np.uint32)), k
