"""GPU: IVF-RaBitQ (cuvs_amd/csrc/ivf_rabitq.hip) against the numpy restatement tests/ivf_rabitq_ref.py - both code streams, all
five factors and the scaling factor bit for bit, search ids and distance bit patterns in all four modes - plus the edges of the
head / tail contract, the streamed build, recall against the library's brute force with the reference's floors, the file, refusals
and concurrent searches."""
import threading

import numpy as np
import pytest

from tests import ivf_rabitq_ref as R
from tests.test_ivf_rabitq_cpu import FLOORS, clustered, recall, uniform

pytestmark = pytest.mark.gpu

ARRAYS = ("list_sizes", "ids", "bit_codes", "short_factors", "ex_codes", "ex_factors", "centers_rot", "rotation")


def _data(n, dim, seed=0, dup=0):
    rng = np.random.default_rng(seed)
    x = rng.random((n, dim), dtype=np.float32) * np.float32(1.9) + np.float32(0.1)
    if dup:
        x[n - dup:] = x[:dup]  # duplicated rows: exact ties
    return x


def _build(x, res, metric="sqeuclidean", n_lists=16, bits=3, host=False, **kw):
    import torch
    from cuvs_amd.neighbors import ivf_rabitq

    p = ivf_rabitq.IndexParams(n_lists=n_lists, metric=metric, bits_per_dim=bits, kmeans_n_iters=10, **kw)
    src = x if host else torch.from_numpy(x).cuda()
    return ivf_rabitq.build(p, src, resources=res)


def _search(index, q, k, n_probes, res, mode="quant4"):
    import torch
    from cuvs_amd.neighbors import ivf_rabitq

    d, i = ivf_rabitq.search(ivf_rabitq.SearchParams(n_probes=n_probes, mode=mode), index, torch.from_numpy(q).cuda(), k, resources=res)
    res.sync()
    return d.cpu().numpy(), i.cpu().numpy()


def _same(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _assert_search_equal(got, want):
    (d, i), (wd, wi) = got, want
    assert np.array_equal(i, wi), f"ids differ in {np.count_nonzero((i != wi).any(1))} rows"
    assert np.array_equal(d.view(np.uint32), wd.view(np.uint32)), "distances differ"


# ------------------------------------------------------------------------------------------------ 1. encode parity
@pytest.mark.parametrize("bits", [1, 2, 3, 4, 8, 9])
@pytest.mark.parametrize("dim", [1, 7, 64, 65, 200])
def test_encode_parity(dim, bits, res):
    from cuvs_amd.neighbors import ivf_rabitq

    n, n_lists = 3000, 16
    x = _data(n, dim, seed=dim, dup=100)
    index = _build(x, res, n_lists=n_lists, bits=bits)
    assert (len(index), index.n_lists, index.dim, index.bits_per_dim) == (n, n_lists, dim, bits)
    ex = ivf_rabitq.export_for_oracle(index, resources=res)
    D = R.padded_dim(dim)
    assert ex["rotation"].shape == (D, D) and ex["ex_bits"] == bits - 1
    sizes = ex["list_sizes"].astype(np.int64)
    assert sizes.sum() == n and sorted(ex["ids"].tolist()) == list(range(n)), "the lists partition the rows"
    start = np.concatenate([[0], np.cumsum(sizes)])
    labels = np.repeat(np.arange(n_lists), sizes)
    for L in range(n_lists):
        assert np.all(np.diff(ex["ids"][start[L]:start[L + 1]].astype(np.int64)) > 0), "rows of a list are in input order"
    assert _same(ex["centers_rot"], R.rotate(ex["centers"], ex["rotation"]))
    t = R.scaling_factor(D, bits - 1)
    assert np.float32(ex["t"]).view(np.uint32) == t.view(np.uint32)
    b, short, codes, exf = R.encode(R.rotate(x[ex["ids"]], ex["rotation"]), ex["centers_rot"][labels], t, bits - 1)
    assert _same(ex["bit_codes"], R.pack_bits(b)), "1-bit codes"
    assert _same(ex["short_factors"], short), "short factors"
    assert _same(ex["ex_codes"], R.pack_ex(codes, bits - 1)), "extended codes"
    assert _same(ex["ex_factors"], exf), "extended factors"


# ------------------------------------------------------------------------------------------------ 2. search parity
def _parity_cases():
    dims, ks, bitss, metrics = (3, 64, 96, 130), (1, 10, 64, 300), (1, 3, 9), ("sqeuclidean", "euclidean")
    out = []
    for n in range(24):  # a rotating subset of the product: every value of every axis, every (mode, bits) pair
        dim, k, mode = dims[n % 4], ks[(n + n // 4) % 4], R.MODES[(n // 2) % 4]
        bits, metric = bitss[n % 3], metrics[(n // 3) % 2]
        out.append(pytest.param(dim, k, mode, bits, metric, id=f"{n:02d}-d{dim}-k{k}-{mode}-b{bits}-{metric}"))
    return out


@pytest.mark.parametrize("dim,k,mode,bits,metric", _parity_cases())
def test_search_parity(dim, k, mode, bits, metric, res):
    from cuvs_amd.neighbors import ivf_rabitq

    n, n_lists, n_probes, nq = 4000, 20, 6, 60
    x = _data(n, dim, seed=100 + dim, dup=400)
    q = _data(nq, dim, seed=200 + dim)
    q[:5] = x[:5]  # queries equal to (duplicated) rows
    index = _build(x, res, metric, n_lists, bits)
    ex = ivf_rabitq.export_for_oracle(index, resources=res)
    _assert_search_equal(_search(index, q, k, n_probes, res, mode), R.search(ex, q, k, n_probes, mode, metric))


# ------------------------------------------------------------------------------------------------ 3. edges
@pytest.fixture(scope="module")
def edge_index(res):
    from cuvs_amd.neighbors import ivf_rabitq

    x = _data(4000, 40, seed=7, dup=300)
    index = _build(x, res, "sqeuclidean", 20, 3)
    return x, index, ivf_rabitq.export_for_oracle(index, resources=res)


def test_all_lists_probed(edge_index, res):
    x, index, ex = edge_index
    q = _data(30, 40, seed=8)
    for mode in ("quant4", "lut32"):
        _assert_search_equal(_search(index, q, 10, 20, res, mode), R.search(ex, q, 10, 20, mode))


def test_k_beyond_the_probed_rows_is_padded(edge_index, res):
    x, index, ex = edge_index
    q = _data(20, 40, seed=9)
    d, i = _search(index, q, 300, 1, res)  # one list of about 200 rows
    _assert_search_equal((d, i), R.search(ex, q, 300, 1))
    assert (i == np.iinfo(np.int64).max).any() and (d[i == np.iinfo(np.int64).max] == np.finfo(np.float32).max).all()


def test_head_spans_two_lists(edge_index, res):
    x, index, ex = edge_index
    assert ex["list_sizes"].max() < 300  # k = 300 needs more than the nearest list
    q = _data(40, 40, seed=10)
    for mode in ("quant8", "lut16"):
        _assert_search_equal(_search(index, q, 300, 6, res, mode), R.search(ex, q, 300, 6, mode))


def test_zero_rotated_query(edge_index, res):
    x, index, ex = edge_index
    q = _data(8, 40, seed=11)
    q[3] = 0  # q' = 0: w = 0, ip1 = 0
    for mode in R.MODES:
        _assert_search_equal(_search(index, q, 10, 8, res, mode), R.search(ex, q, 10, 8, mode))


def test_every_tail_row_survives_the_screen(tmp_path, res):
    """Every tail row survives: an index whose rows all carry a huge f_error (written as a file from the exported arrays and loaded),
    searched with queries far from all centres. low = est - f_error sqrt(g) is then -inf for every row, below any T. All of them
    must arrive at the re-score: survivors == screened, equal to the restatement's count, results equal bit for bit."""
    from cuvs_amd.neighbors import ivf_rabitq

    x = _data(3000, 40, seed=14, dup=200)
    ex = ivf_rabitq.export_for_oracle(_build(x, res, "sqeuclidean", 12, 3), resources=res)
    ex["short_factors"] = ex["short_factors"].copy()
    ex["short_factors"][:, 2] = np.float32(3e38)
    p = str(tmp_path / "all.bin")
    R.write_file(p, ex)
    index = ivf_rabitq.load(p, resources=res)
    q = _data(70, 40, seed=15) + np.float32(30.0)  # far from all centres (g > 0 for every probe)
    for mode, k, n_probes in (("quant4", 10, 12), ("quant8", 300, 9), ("lut32", 10, 12)):
        stats = {}
        want = R.search(ex, q, k, n_probes, mode, stats=stats)
        assert stats["survivors"] == stats["screened"] > 1000 * len(q), "the case is built to let every tail row through"
        got = _search(index, q, k, n_probes, res, mode)
        st = ivf_rabitq.last_search_stats()
        assert st["survivors"] == st["screened"] == stats["screened"], "no row may be dropped"
        _assert_search_equal(got, want)


def test_far_queries_mass_survival_nothing_dropped(res):
    """Queries far from all centres: the bound's error term f_error sqrt(g) and the spread of the rows' distances both grow like the
    distance to the centres, so the share of tail rows that pass the screen does not tend to one (the bound is 1.9 standard
    deviations of the estimator, not of the data: here 30 % pass). Thousands of survivors per query - far beyond any per-block cap -
    must all arrive: their number equals the restatement's and the results are equal bit for bit."""
    from cuvs_amd.neighbors import ivf_rabitq

    x = _data(2000, 128, seed=12)
    index = _build(x, res, "sqeuclidean", 8, 3)
    ex = ivf_rabitq.export_for_oracle(index, resources=res)
    rng = np.random.default_rng(13)
    q = (rng.choice([-1.0, 1.0], (70, 128)) * 100.0 + rng.standard_normal((70, 128))).astype(np.float32)
    stats = {}
    want = R.search(ex, q, 10, 8, "quant4", stats=stats)
    print(f"far queries: {stats['survivors']} of {stats['screened']} tail rows survive the screen")
    assert stats["survivors"] >= 0.2 * stats["screened"] and stats["survivors"] >= 300 * len(q)
    got = _search(index, q, 10, 8, res)
    st = ivf_rabitq.last_search_stats()
    assert (st["screened"], st["survivors"]) == (stats["screened"], stats["survivors"]), "no row may be dropped"
    _assert_search_equal(got, want)


def test_early_returns_leave_the_outputs_alone(edge_index, res):
    import torch
    from cuvs_amd.neighbors import ivf_rabitq

    x, index, ex = edge_index
    q = torch.from_numpy(_data(4, 40, seed=13)).cuda()
    nb = torch.full((4, 5), 77, dtype=torch.int64, device="cuda")
    ds = torch.full((4, 5), 3.5, dtype=torch.float32, device="cuda")
    ivf_rabitq.search(ivf_rabitq.SearchParams(n_probes=0), index, q, 5, neighbors=nb, distances=ds, resources=res)
    res.sync()
    assert (nb == 77).all() and (ds == 3.5).all()
    d, i = ivf_rabitq.search(ivf_rabitq.SearchParams(n_probes=4), index, q, 0, resources=res)
    assert d.shape == (4, 0) and i.shape == (4, 0)
    d, i = ivf_rabitq.search(ivf_rabitq.SearchParams(n_probes=4), index, q[:0], 5, resources=res)
    assert d.shape == (0, 5)


# ------------------------------------------------------------------------------------------------ 4. streaming build
def test_streamed_host_build_equals_device_build(res):
    from cuvs_amd.neighbors import ivf_rabitq

    x = _data(3500, 33, seed=21)
    a = ivf_rabitq.export_for_oracle(_build(x, res, n_lists=12, bits=4), resources=res)
    b = ivf_rabitq.export_for_oracle(_build(x, res, n_lists=12, bits=4, host=True, force_streaming=True, streaming_batch_size=1000),
                                     resources=res)
    c = ivf_rabitq.export_for_oracle(_build(x, res, n_lists=12, bits=4, host=True), resources=res)
    for name in ARRAYS + ("centers",):
        assert _same(a[name], b[name]), name
        assert _same(a[name], c[name]), name


# ------------------------------------------------------------------------------------------------ 5. recall
_RECALL = {}


def _recall_case(kind, bits, res):
    import torch
    from cuvs_amd.neighbors import brute_force

    if kind not in _RECALL:
        x, q = clustered(4096, 256) if kind == "clustered" else uniform(4096, 256)
        _, truth = brute_force.search(brute_force.build(torch.from_numpy(x).cuda(), resources=res), torch.from_numpy(q).cuda(), 10,
                                      resources=res)
        res.sync()
        _RECALL[kind] = (x, q, truth.cpu().numpy())
    if (kind, bits) not in _RECALL:
        _RECALL[(kind, bits)] = _build(_RECALL[kind][0], res, n_lists=32, bits=bits)
    return _RECALL[(kind, bits)], _RECALL[kind][1], _RECALL[kind][2]


@pytest.mark.parametrize("kind,bits,mode,n_probes,floor", [
    ("clustered", 3, "quant4", 20, FLOORS["default"]), ("clustered", 1, "quant4", 20, FLOORS["bits_per_dim_1"]),
    ("clustered", 5, "quant8", 20, FLOORS["default"]), ("clustered", 3, "quant4", 1, 1 * FLOORS["per_probe_up_to_5_probes"]),
    ("clustered", 3, "quant4", 5, 5 * FLOORS["per_probe_up_to_5_probes"]), ("uniform", 3, "quant4", 20, FLOORS["default"]),
    ("uniform", 3, "quant4", 1, FLOORS["per_probe_up_to_5_probes"])])
def test_recall_against_brute_force(kind, bits, mode, n_probes, floor, res):
    index, q, truth = _recall_case(kind, bits, res)
    _, nb = _search(index, q, 10, n_probes, res, mode)
    r = recall(nb, truth)
    print(f"{kind} bits={bits} mode={mode} n_probes={n_probes}: recall@10 {r:.3f} (floor {floor})")
    assert r >= floor


# ------------------------------------------------------------------------------------------------ 6. files
@pytest.mark.parametrize("metric,bits", [("sqeuclidean", 3), ("euclidean", 1), ("sqeuclidean", 9)])
def test_save_load_search_and_file_bytes(metric, bits, tmp_path, res):
    from cuvs_amd.neighbors import ivf_rabitq

    x = _data(3000, 21, seed=31)
    q = _data(40, 21, seed=32)
    index = _build(x, res, metric, 12, bits)
    p1, p2, p3 = (str(tmp_path / f"{i}.bin") for i in range(3))
    ivf_rabitq.save(p1, index, resources=res)
    back = ivf_rabitq.load(p1, resources=res)
    assert (len(back), back.n_lists, back.dim, back.bits_per_dim) == (3000, 12, 21, bits)
    want = _search(index, q, 10, 4, res)
    _assert_search_equal(_search(back, q, 10, 4, res), want)
    ex = ivf_rabitq.export_for_oracle(index, resources=res)
    R.write_file(p2, ex, metric)
    assert open(p1, "rb").read() == open(p2, "rb").read(), "the file equals the Python writer's from the exported arrays"
    ivf_rabitq.save(p3, back, resources=res)
    assert open(p1, "rb").read() == open(p3, "rb").read()
    exb = ivf_rabitq.export_for_oracle(back, resources=res)
    assert "centers" not in exb
    for name in ARRAYS:
        assert _same(ex[name], exb[name]), name


def test_file_from_the_restatement_loads_and_searches(tmp_path, res):
    from cuvs_amd.neighbors import ivf_rabitq

    rng = np.random.default_rng(33)
    x = rng.standard_normal((700, 19)).astype(np.float32)
    centers = x[:6].copy()
    rot, _ = np.linalg.qr(rng.standard_normal((64, 64)))
    ex = R.build(x, centers, rot.astype(np.float32), 4)
    ex["ids"] = (ex["ids"].astype(np.uint32) * np.uint32(7) + np.uint32(5))  # ids are the file's, not row numbers
    p = str(tmp_path / "r.bin")
    R.write_file(p, ex)
    index = ivf_rabitq.load(p, resources=res)
    q = rng.standard_normal((30, 19)).astype(np.float32)
    for mode in ("quant4", "lut32"):
        _assert_search_equal(_search(index, q, 20, 3, res, mode), R.search(ex, q, 20, 3, mode))


def test_damaged_files_are_refused(tmp_path, res):
    from cuvs_amd._lib import CuvsError
    from cuvs_amd.neighbors import ivf_rabitq

    x = _data(600, 10, seed=34)
    index = _build(x, res, "sqeuclidean", 4, 3)
    good = str(tmp_path / "good.bin")
    ivf_rabitq.save(good, index, resources=res)
    raw = open(good, "rb").read()
    bad = str(tmp_path / "bad.bin")

    def refused(data, match):
        open(bad, "wb").write(bytes(data))
        with pytest.raises(CuvsError, match=match):
            ivf_rabitq.load(bad, resources=res)

    def patched(offset, value):
        b = bytearray(raw)
        b[offset:offset + 8] = np.uint64(value).tobytes()
        return b

    refused(patched(24, 9), "ex_bits")
    refused(patched(16, 0), "n_lists")
    refused(patched(8, 0), "dim")
    refused(patched(41, int(np.frombuffer(raw[41:49], np.uint64)[0]) + 1), "sum")
    refused(patched(0, 601), "sum|short")
    refused(patched(0, 1 << 40), "n=")
    refused(raw + b"\x00", "trailing")
    off = R.section_offsets(600, 10, 4, 2)
    assert off["end"] == len(raw)
    for name, at in off.items():
        if name == "header":
            continue
        if name != "end":
            refused(raw[:at], "short")  # cut at the start of a section
        refused(raw[:at - 1], "short")  # and one byte before it
    refused(raw[:7], "short")
    refused(b"", "short")
    # the process lives and the good file still loads
    assert len(ivf_rabitq.load(good, resources=res)) == 600


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals(res):
    import torch
    from cuvs_amd._lib import CuvsError
    from cuvs_amd.neighbors import ivf_rabitq

    x = _data(2000, 8, seed=41)
    index = _build(x, res, "sqeuclidean", 8)
    with pytest.raises(CuvsError, match="n_lists"):
        _build(x[:5], res, "sqeuclidean", 8)
    for bits in (0, 10):
        with pytest.raises(CuvsError, match="bits_per_dim"):
            _build(x, res, "sqeuclidean", 8, bits)
    with pytest.raises(CuvsError, match="metric"):
        _build(x, res, "inner_product", 8)
    with pytest.raises(CuvsError, match="fast_quantize_flag"):
        _build(x, res, "sqeuclidean", 8, fast_quantize_flag=False)
    with pytest.raises(CuvsError, match="float32"):
        ivf_rabitq.build(ivf_rabitq.IndexParams(n_lists=8), torch.ones((100, 8), dtype=torch.float16, device="cuda"), resources=res)
    with pytest.raises(CuvsError, match="n_probes"):
        _search(index, x[:4], 5, 9, res)
    with pytest.raises(CuvsError, match="dim"):
        _search(index, _data(4, 9), 5, 2, res)
    d, i = _search(index, x[:4], 5, 8, res)  # the index is still usable
    assert i.shape == (4, 5)


# ------------------------------------------------------------------------------------------------ 8. concurrency
def test_four_threads_four_handles_one_index(res):
    import torch
    from cuvs_amd.common import Resources
    from cuvs_amd.neighbors import ivf_rabitq

    x = _data(8000, 32, seed=51, dup=100)
    q = _data(200, 32, seed=52)
    index = _build(x, res, "sqeuclidean", 32)
    cases = [(10, "quant4"), (100, "quant8"), (10, "lut32"), (300, "quant4")]
    want = {c: _search(index, q, c[0], 10, res, c[1]) for c in cases}
    out, errs = {}, []

    def run(c):
        try:
            torch.cuda.set_device(0)
            r = Resources(stream=torch.cuda.Stream())
            for _ in range(3):
                d, i = ivf_rabitq.search(ivf_rabitq.SearchParams(n_probes=10, mode=c[1]), index, torch.from_numpy(q).cuda(), c[0],
                                         resources=r)
                r.sync()
                out[c] = (d.cpu().numpy(), i.cpu().numpy())
        except Exception as e:  # pragma: no cover - reported below
            errs.append(e)

    ts = [threading.Thread(target=run, args=(c,)) for c in cases]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs
    for c in cases:
        _assert_search_equal(out[c], want[c])
