"""GPU: the sparse (CSR) pairwise distances and the sparse brute-force kNN against the numpy twin (tests/sparse_distance_ref.py)
bit for bit, the transcendental metrics inside a derived error bound, the reference's own test tables, determinism and the
refusals."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from tests import sparse_distance_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "sparse_reference_table.json")

EXACT = [R.InnerProduct, R.L2Expanded, R.L2SqrtExpanded, R.CosineExpanded, R.CorrelationExpanded, R.JaccardExpanded, R.DiceExpanded,
         R.RusselRaoExpanded, R.HellingerExpanded, R.L1, R.L2Unexpanded, R.L2SqrtUnexpanded, R.Linf, R.Canberra, R.HammingUnexpanded]
BINARY = [R.JaccardExpanded, R.DiceExpanded, R.RusselRaoExpanded, R.HammingUnexpanded]
RANGE_I, RANGE_U = 2048, 1024  # sparse_distance_host.hpp kRangeI, kRangeU
FORMS = {1: (8, 4), 2: (1, 1), 3: (1, 1), 4: (2, 2)}  # form of the walk -> virtual rows of y per thread (intersection, union)


def dev(c):
    return (torch.from_numpy(c.indptr).cuda(), torch.from_numpy(c.indices).cuda(), torch.from_numpy(c.data).cuda(), (c.rows, c.n_cols))


def bits(a):
    """the bit patterns; every NaN counts as one value (0 / 0 has no defined sign or payload: x86 gives -nan, the device +nan)"""
    a = np.ascontiguousarray(a, np.float32)
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))


def edge_csr(rng, rows, n_cols, density):
    """a sparse matrix whose first row holds the first and the last column"""
    c = R.random_csr(rng, rows, n_cols, density)
    d = c.dense()
    d[0, 0], d[0, n_cols - 1] = 0.5, 0.25
    return R.Csr.from_dense(d)


@functools.lru_cache(maxsize=None)
def case(name):
    """(x, y): x is y for 'self'"""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "one":
        return R.Csr([0, 1], [0], [0.75], 1), R.Csr([0, 1], [0], [0.5], 1)
    if name in ("mid", "mid_binary", "self"):
        b = name == "mid_binary"
        x = R.random_csr(rng, 48, 256, 0.25, binary=b, empty_rows=(0, 17, 47), stored_zeros=40, duplicate=((5, 4), (30, 4)))
        y = R.random_csr(rng, 80, 256, 0.25, binary=b, empty_rows=(3, 79), stored_zeros=60, duplicate=((9, 8), (70, 8)))
        return (x, x) if name == "self" else (x, y)
    if name == "odd":
        return R.random_csr(rng, 129, 300, 0.12, empty_rows=(128,)), R.random_csr(rng, 257, 300, 0.12, empty_rows=(0, 256), stored_zeros=9)
    if name == "narrow":
        return R.random_csr(rng, 130, 17, 0.5), R.random_csr(rng, 127, 17, 0.5, stored_zeros=20)
    if name == "wide":
        return R.random_wide_csr(rng, 5, 100000, 0.0004), R.random_wide_csr(rng, 300, 100000, 0.0004)
    if name.startswith("cols"):
        n_cols = int(name[4:])
        return edge_csr(rng, 6, n_cols, 0.02), edge_csr(rng, 40, n_cols, 0.02)
    if name == "long":  # rows holding every column on both sides, a y row one entry past the split threshold, an x row past it
        x = R.random_csr(rng, 6, 3000, 0.01, full_rows=(2,), long_rows=((4, R.SPLIT + 1),), empty_rows=(5,))
        y = R.random_csr(rng, 7, 3000, 0.01, full_rows=(1,), long_rows=((3, R.SPLIT + 1), (5, R.SPLIT)), empty_rows=(6,), stored_zeros=30)
        return x, y
    if name == "long_binary":
        x = R.random_csr(rng, 6, 3000, 0.01, binary=True, full_rows=(2,), long_rows=((4, R.SPLIT + 1),))
        y = R.random_csr(rng, 7, 3000, 0.01, binary=True, full_rows=(1,), long_rows=((3, R.SPLIT + 1),))
        return x, y
    if name == "empty":  # nnz == 0
        return R.random_csr(rng, 5, 33, 0.3), R.Csr(np.zeros(8, np.int32), [], [], 33)
    if name == "empty_x":
        return R.Csr(np.zeros(4, np.int32), [], [], 33), R.random_csr(rng, 9, 33, 0.3)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def twin(name, metric, p=2.0):
    x, y = case(name)
    return R.pairwise(x, y, metric, p)


def gpu_pairwise(name, metric, p=2.0, out=None):
    from cuvs_amd.distance import sparse_pairwise_distance

    x, y = case(name)
    dx = dev(x)
    got = sparse_pairwise_distance(dx, None if name == "self" else dev(y), out=out, metric=metric, metric_arg=p)
    torch.cuda.synchronize()
    return got.cpu().numpy()


def test_only_the_contracts_arithmetic_can_pass():
    x, y = case("mid")
    asc = R.pairwise(x, y, R.InnerProduct)
    desc = R.pairwise(x, y, R.InnerProduct, descending=True)
    mul_add = R.pairwise(x, y, R.InnerProduct, order="mul_add")
    assert np.allclose(asc, desc, rtol=1e-5) and np.allclose(asc, mul_add, rtol=1e-5)
    assert (bits(asc) != bits(desc)).sum() >= asc.size // 4
    assert (bits(asc) != bits(mul_add)).sum() >= asc.size // 4


CASES = ["one", "mid", "odd", "narrow", "wide", "long", "empty", "empty_x", "self"]


@pytest.mark.parametrize("metric", EXACT)
@pytest.mark.parametrize("name", CASES)
def test_bit_for_bit(name, metric):
    want = twin(name, metric)
    got = gpu_pairwise(name, metric)
    assert got.shape == want.shape
    same = bits(got) == bits(want)
    assert same.all(), (name, metric, int((~same).sum()), got[~same][:4], want[~same][:4])


@pytest.mark.parametrize("metric", BINARY)
@pytest.mark.parametrize("name", ["mid_binary", "long_binary"])
def test_bit_for_bit_binary(name, metric):
    want = twin(name, metric)
    got = gpu_pairwise(name, metric)
    assert (bits(got) == bits(want)).all()
    assert len(np.unique(want)) > 4


@pytest.mark.parametrize("metric", [R.InnerProduct, R.CosineExpanded, R.L1, R.HammingUnexpanded])
@pytest.mark.parametrize("n_cols", [RANGE_U - 1, RANGE_U + 1, RANGE_I - 1, RANGE_I + 1])
def test_bit_for_bit_at_the_range_edges(n_cols, metric):
    name = "cols%d" % n_cols
    assert (bits(gpu_pairwise(name, metric)) == bits(twin(name, metric))).all()


def ranges_with_entries(x, width):
    """column ranges a tile of virtual rows of y has to visit: per tile of four x rows, the ranges of `width` columns that hold a
    stored entry of them"""
    total = 0
    for a0 in range(0, x.rows, 4):
        cols = x.indices[x.indptr[a0]:x.indptr[min(a0 + 4, x.rows)]]
        total += len(np.unique(cols // width))
    return total


@pytest.fixture
def walk_form():
    from cuvs_amd.distance import set_sparse_walk_form

    yield set_sparse_walk_form
    set_sparse_walk_form(0, 0)


@pytest.mark.parametrize("form", [0, 1, 2, 3, 4])
def test_statistics_of_the_last_call(walk_form, form):
    from cuvs_amd.distance import sparse_last_stats

    walk_form(form, form)
    x, y = case("wide")
    for fam, (metric, width) in enumerate(((R.CosineExpanded, RANGE_I), (R.L1, RANGE_U))):
        gpu_pairwise("wide", metric)
        st = sparse_last_stats()
        if form == 0:  # by shape: 40 entries per row over 49 / 98 ranges is below the stage's threshold
            b_tiles = -(-300 // (256 * FORMS[1][fam]))
        else:
            b_tiles = -(-300 // (256 * FORMS[form][fam]))
        tiles = 2 * b_tiles  # 5 rows of x in fours
        assert st["tiles"] == tiles and st["long_row_pieces"] == 0
        want = ranges_with_entries(x, width) * b_tiles  # counted from the data, not from the call
        assert st["ranges_visited"] == want and 0 < want < tiles * -(-100000 // width)
        assert st["ranges_skipped"] == tiles * -(-100000 // width) - want
    x, y = case("long")
    gpu_pairwise("long", R.L1)
    st = sparse_last_stats()
    assert st["long_row_pieces"] == 3 + 2
    assert st["tiles"] == 2 and st["ranges_visited"] == ranges_with_entries(x, RANGE_U) == 2 * 3


@pytest.mark.parametrize("metric", [R.CosineExpanded, R.HellingerExpanded, R.L1, R.Canberra, R.HammingUnexpanded])
@pytest.mark.parametrize("name", ["odd", "wide", "long", "self", "empty"])
@pytest.mark.parametrize("form", [1, 2, 3, 4])
def test_every_form_of_the_walk_gives_the_same_bits(walk_form, form, name, metric):
    walk_form(form, form)
    assert (bits(gpu_pairwise(name, metric)) == bits(twin(name, metric))).all()


def test_rows_of_x_in_several_slabs(monkeypatch):
    """the raw accumulators of the split pieces leave the workspace budget: x is processed in two slabs, each with its own
    combine pass"""
    from cuvs_amd.common import Resources
    from cuvs_amd.distance import sparse_last_stats, sparse_pairwise_distance

    monkeypatch.setenv("CUVS_AMD_DEBUG_SWITCHES", "1")
    monkeypatch.setenv("CUVS_AMD_WORKSPACE_MB", "1")
    res = Resources()
    rng = np.random.default_rng(77)
    m = n = 400
    x = R.random_csr(rng, m, 2050, 0.01, empty_rows=(3,))
    y = R.random_csr(rng, n, 2050, 0.01, long_rows=tuple((j, R.SPLIT + 1) for j in range(n)))
    slots = 2 * n
    slab = (1 << 20) // (4 * slots) // 4 * 4
    assert slab < m <= 2 * slab  # two slabs, the second shorter
    for metric in (R.InnerProduct, R.CosineExpanded):
        got = sparse_pairwise_distance(dev(x), dev(y), metric=metric, resources=res)
        res.sync()
        assert sparse_last_stats()["long_row_pieces"] == 2 * slots
        assert (bits(got.cpu().numpy()) == bits(R.pairwise(x, y, metric))).all()


# ---------------------------------------------------------------------------------------------- transcendental metrics
# ulp bounds of the device functions: the library's math functions are OCML's, which implements the OpenCL C full-profile
# accuracy table (OpenCL C specification, "Relative error as ULPs"): log <= 3 ulp, pow <= 16 ulp, sqrt <= 3 ulp.
ULP_LOG, ULP_POW, ULP_SQRT = 3, 16, 3
TRANSCENDENTAL = [(R.LpUnexpanded, 1.5), (R.LpUnexpanded, 2.0), (R.LpUnexpanded, 3.0), (R.JensenShannon, 2.0), (R.KLDivergence, 2.0)]


@pytest.mark.parametrize("name", ["mid", "long"])
@pytest.mark.parametrize("metric,p", TRANSCENDENTAL)
def test_transcendental_metrics_inside_the_bound(name, metric, p):
    """|got - want64| <= K 2^-24 sum|term| |f'(acc)|, K = chain length + the ulp bounds of the metric's functions (KL: logf;
    JensenShannon: logf and sqrtf; Lp: powf). The chain length is the number of terms the fp64 twin applied to the pair plus
    the additions that combine the pieces of a long row; sum|term| is the twin's. f is the epilogue: 0.5 acc (KL),
    sqrt(0.5 acc) (JensenShannon), acc^(1/p) (Lp); its derivative carries the chain's bound to the value that is returned
    (f' = 0.5, want / (2 acc), want / (p acc)): tighter than the literal K 2^-24 sum|term| where f' < 1 (KL, Lp with acc > 1),
    wider where f' > 1 (JensenShannon with acc < 1/8, Lp with small acc), which is what an error of acc becomes in the value.
    A pair without terms must be exact."""
    x, y = case(name)
    got = gpu_pairwise(name, metric, p).astype(np.float64)
    count = np.zeros((x.rows, y.rows), np.int64)
    want, acc, mass = R.pairwise64(x, y, metric, p, count=count)
    pieces = np.maximum((np.diff(y.indptr)[None, :] + R.SPLIT - 1) // R.SPLIT, 1)
    length = count + (pieces - 1)
    with np.errstate(all="ignore"):
        if metric == R.KLDivergence:
            ulps, slope = ULP_LOG, 0.5
        elif metric == R.JensenShannon:
            ulps, slope = ULP_LOG + ULP_SQRT, np.where(acc > 0, 0.5 * want / acc, 0.0)
        else:
            ulps, slope = ULP_POW, np.where(acc > 0, want / (p * acc), 0.0)
    bound = 2.0 ** -24 * (length + ulps) * mass * np.abs(slope)
    err = np.abs(got - want)
    print("metric %d p %g %s: largest error / bound %.3g, mean chain length %.1f" %
          (metric, p, name, np.nanmax(np.where(bound > 0, err / np.maximum(bound, 1e-300), 0.0)), length.mean()))
    assert np.isfinite(got).all() and (err <= bound).all()
    assert (count > 0).mean() > 0.3 and (want != 0).mean() > 0.3


# ---------------------------------------------------------------------------------------------- the reference's tables
def compare_approx(a, b, eps):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    with np.errstate(all="ignore"):
        diff = np.abs(a - b)
        ratio = np.where(diff > np.float32(eps), diff / np.maximum(np.abs(a), np.abs(b)), diff)
    return ratio <= np.float32(eps)


@pytest.mark.parametrize("i", range(20))
def test_reference_distance_rows(i):
    from cuvs_amd.distance import sparse_pairwise_distance

    r = json.load(open(TABLE))["sparse_distance"]["rows"][i]
    x = dev(R.Csr(r["indptr"], r["indices"], r["data"], r["n_cols"]))
    got = sparse_pairwise_distance(x, x, metric=r["metric_id"], metric_arg=r["metric_arg"]).cpu().numpy()
    want = np.asarray(r["expected"], np.float32).reshape(got.shape)
    assert compare_approx(want, got, 1e-3).all(), (r["lines"], r["metric"])


def test_reference_knn_row():
    from cuvs_amd.neighbors import sparse_brute_force

    r = json.load(open(TABLE))["sparse_brute_force"]["rows"][0]
    x = dev(R.Csr(r["indptr"], r["indices"], r["data"], r["n_cols"]))
    index = sparse_brute_force.build(x, metric=r["metric_id"])
    d, i = sparse_brute_force.search(index, x, r["k"], r["batch_size_index"], r["batch_size_query"], neighbors_dtype=torch.int32)
    assert i.dtype == torch.int32 and (i.cpu().numpy().ravel() == np.asarray(r["expected_indices"])).all()
    assert compare_approx(np.asarray(r["expected_distances"], np.float32), d.cpu().numpy().ravel(), 1e-4).all()


# ---------------------------------------------------------------------------------------------- kNN
KNN_METRICS = [R.L2SqrtExpanded, R.CosineExpanded, R.InnerProduct, R.L1, R.JaccardExpanded]


@functools.lru_cache(maxsize=None)
def knn_case(metric):
    rng = np.random.default_rng(300 + metric)
    b = metric == R.JaccardExpanded
    # equal rows on both sides of the index batch boundaries at 64, 128, ...: ties across batches
    dup = ((64, 63), (65, 63), (128, 63), (255, 63), (299, 63), (100, 20), (200, 20))
    index = R.random_csr(rng, 300, 64, 0.12, binary=b, empty_rows=(7, 150), duplicate=dup, stored_zeros=0 if b else 25)
    queries = R.random_csr(rng, 70, 64, 0.12, binary=b, empty_rows=(36,))
    ids, d = R.knn(queries, index, 300, metric)
    return index, queries, ids, d


@pytest.mark.parametrize("k", [1, 10, 64, 300])
@pytest.mark.parametrize("metric", KNN_METRICS)
def test_knn(metric, k):
    from cuvs_amd.neighbors import sparse_brute_force

    index, queries, ids, d = knn_case(metric)
    ties = (d[:, 1:] == d[:, :-1]) & (ids[:, 1:] // 64 != ids[:, :-1] // 64)
    assert ties.sum() > 70  # equal distances whose rows sit in different index batches
    ix = sparse_brute_force.build(dev(index), metric=metric)
    q = dev(queries)
    first = None
    for bi, bq, dtype in ((64, 37, torch.int64), (300, 70, torch.int64), (1000, 1000, torch.int32), (64, 37, torch.int32), (7, 70, torch.int64)):
        gd, gi = sparse_brute_force.search(ix, q, k, bi, bq, neighbors_dtype=dtype)
        torch.cuda.synchronize()
        assert gi.dtype == dtype
        gd, gi = gd.cpu().numpy(), gi.cpu().numpy().astype(np.int64)
        assert (gi == ids[:, :k]).all(), (metric, k, bi, bq)
        assert (bits(gd) == bits(d[:, :k])).all(), (metric, k, bi, bq)
        first = (gd, gi) if first is None else first
        assert (bits(gd) == bits(first[0])).all() and (gi == first[1]).all()  # the batch sizes never change results


@pytest.mark.parametrize("metric", KNN_METRICS)
def test_knn_nine_rows_in_batches_of_two(metric):
    from cuvs_amd.neighbors import sparse_brute_force

    rng = np.random.default_rng(9)
    x = R.random_csr(rng, 9, 12, 0.4, binary=metric == R.JaccardExpanded, duplicate=((8, 1), (4, 1)), empty_rows=(6,))
    ids, d = R.knn(x, x, 9, metric)
    ix = sparse_brute_force.build(dev(x), metric=metric)
    for k in (1, 3, 9):
        gd, gi = sparse_brute_force.search(ix, dev(x), k, 2, 2)
        assert (gi.cpu().numpy() == ids[:, :k]).all() and (bits(gd.cpu().numpy()) == bits(d[:, :k])).all()


# ---------------------------------------------------------------------------------------------- determinism
@pytest.mark.parametrize("metric", [R.CosineExpanded, R.L1, R.JensenShannon])
def test_two_runs_give_the_same_bytes(metric):
    from cuvs_amd.neighbors import sparse_brute_force

    x, y = case("odd")
    a = gpu_pairwise("odd", metric, out=torch.full((x.rows, y.rows), float("nan"), device="cuda"))
    b = gpu_pairwise("odd", metric, out=torch.full((x.rows, y.rows), 7.0, device="cuda"))
    assert a.tobytes() == b.tobytes()
    ix = sparse_brute_force.build(dev(y), metric=metric)
    outs = []
    for fill in (-1, 77):
        n = torch.full((x.rows, 10), fill, dtype=torch.int64, device="cuda")
        d = torch.full((x.rows, 10), float(fill), device="cuda")
        sparse_brute_force.search(ix, dev(x), 10, 100, 50, neighbors=n, distances=d)
        torch.cuda.synchronize()
        outs.append((n.cpu().numpy().tobytes(), d.cpu().numpy().tobytes()))
    assert outs[0] == outs[1]


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals():
    from cuvs_amd._lib import CuvsError
    from cuvs_amd.distance import sparse_pairwise_distance
    from cuvs_amd.neighbors import sparse_brute_force

    x, y = case("narrow")
    dx, dy = dev(x), dev(y)
    for metric in (13, 14, 20, 99):  # Haversine, BrayCurtis, BitwiseHamming, no metric at all
        with pytest.raises(CuvsError, match="metric %d" % metric):
            sparse_pairwise_distance(dx, dy, metric=metric)
        with pytest.raises(CuvsError, match="metric %d" % metric):
            sparse_brute_force.build(dy, metric=metric)
    with pytest.raises(CuvsError, match="Haversine"):
        sparse_pairwise_distance(dx, dy, metric=13)
    for name in ("braycurtis", "bitwise_hamming", "haversine"):
        with pytest.raises(ValueError, match="not supported"):
            sparse_pairwise_distance(dx, dy, metric=name)
    for p in (0.0, -2.0):
        with pytest.raises(CuvsError, match="metric_arg"):
            sparse_pairwise_distance(dx, dy, metric="lp", metric_arg=p)
    ix = sparse_brute_force.build(dy, metric="cosine")
    with pytest.raises(CuvsError, match="larger than the number of index rows"):
        sparse_brute_force.search(ix, dx, y.rows + 1)
    with pytest.raises(CuvsError, match="batch_size"):
        sparse_brute_force.search(ix, dx, 3, 0, 5)
    other = dev(R.Csr(x.indptr, x.indices, x.data, x.n_cols + 1))
    with pytest.raises(ValueError, match="same number of columns"):
        sparse_pairwise_distance(other, dy)
    with pytest.raises(ValueError, match="same number of columns"):
        sparse_brute_force.search(ix, other, 3)
    # wrong dtypes
    with pytest.raises(CuvsError, match="indptr must be int32"):
        sparse_pairwise_distance((dx[0].long(), dx[1], dx[2], dx[3]), dy)
    with pytest.raises(CuvsError, match="indices must be int32"):
        sparse_pairwise_distance(dx, (dy[0], dy[1].long(), dy[2], dy[3]))
    with pytest.raises(CuvsError, match="data must be fp32"):
        sparse_pairwise_distance((dx[0], dx[1], dx[2].double(), dx[3]), dy)
    with pytest.raises(CuvsError, match="data must be fp32"):
        sparse_brute_force.build((dy[0], dy[1], dy[2].half(), dy[3]))
    with pytest.raises(CuvsError, match="out must be fp32"):
        sparse_pairwise_distance(dx, dy, out=torch.empty((x.rows, y.rows), dtype=torch.float64, device="cuda"))
    with pytest.raises(CuvsError, match="out must have shape"):
        sparse_pairwise_distance(dx, dy, out=torch.empty((y.rows, x.rows), device="cuda"))
    with pytest.raises(CuvsError, match="neighbors must be int64 or int32"):
        sparse_brute_force.search(ix, dx, 3, neighbors=torch.empty((x.rows, 3), dtype=torch.uint8, device="cuda"))
    # host tensors
    host = (dx[0].cpu(), dx[1].cpu(), dx[2].cpu(), dx[3])
    with pytest.raises(CuvsError, match="device"):
        sparse_pairwise_distance(host, dy)
    with pytest.raises(CuvsError, match="device"):
        sparse_pairwise_distance(dx, dy, out=torch.empty((x.rows, y.rows)))
    with pytest.raises(CuvsError, match="device"):
        sparse_brute_force.build(host)
    # a scipy matrix goes through the documented conversion
    import scipy.sparse as sp

    sx = sp.csr_matrix((x.data, x.indices, x.indptr), shape=(x.rows, x.n_cols))
    got = sparse_pairwise_distance(sx.tocoo(), dy, metric="cityblock").cpu().numpy()
    assert (bits(got) == bits(twin("narrow", R.L1))).all()


def test_the_validator_names_the_first_bad_row():
    """non-canonical matrices go to the validator only, never to a compute entry point"""
    from cuvs_amd._lib import CuvsError
    from cuvs_amd.distance import validate_csr

    good = R.Csr([0, 2, 2, 5, 7], [1, 4, 0, 2, 3, 1, 5], np.arange(1, 8), 6)
    validate_csr(dev(good))
    validate_csr(dev(R.Csr([0], [], [], 0)))

    def bad(indptr, indices, n_cols=6):
        return dev(R.Csr(indptr, indices, np.ones(len(indices)), n_cols))

    with pytest.raises(CuvsError, match="columns of row 2 are not strictly ascending"):
        validate_csr(bad([0, 2, 2, 5, 7], [1, 4, 2, 0, 3, 1, 5]))  # an unsorted row
    with pytest.raises(CuvsError, match="columns of row 3 are not strictly ascending"):
        validate_csr(bad([0, 2, 2, 5, 7], [1, 4, 0, 2, 3, 5, 5]))  # a repeated column
    with pytest.raises(CuvsError, match="row 0 holds a column outside"):
        validate_csr(bad([0, 2, 2, 5, 7], [1, 6, 0, 2, 3, 1, 5]))  # a column >= n_cols
    with pytest.raises(CuvsError, match="row 2 holds a column outside"):
        validate_csr(bad([0, 2, 2, 5, 7], [1, 4, -1, 2, 3, 1, 5]))
    with pytest.raises(CuvsError, match="indptr decreases or leaves .* at row 1"):
        validate_csr(bad([0, 3, 2, 5, 7], [1, 4, 5, 2, 3, 1, 5]))  # a decreasing indptr
    with pytest.raises(CuvsError, match=r"indptr\[4\] is not nnz \(7\)"):
        validate_csr(bad([0, 2, 2, 5, 6], [1, 4, 0, 2, 3, 1, 5]))  # indptr[rows] != nnz
    with pytest.raises(CuvsError, match="at row 3"):
        validate_csr(bad([0, 2, 2, 5, 9], [1, 4, 0, 2, 3, 1, 5]))  # indptr[rows] past the arrays: nothing is read there
    with pytest.raises(CuvsError, match=r"indptr\[0\] is not 0"):
        validate_csr(bad([1, 2, 2, 5, 7], [1, 4, 0, 2, 3, 1, 5]))
