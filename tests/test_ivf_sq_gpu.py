"""GPU: IVF-SQ (cuvs_amd/csrc/ivf_sq.hip) against the numpy restatement tests/ivf_sq_ref.py - quantizer and every code byte,
search ids and distances bit for bit - plus the reference's own test table (tests/golden/ivf_sq_reference_table.json),
extend, the file container, refusals and concurrent searches."""
import json
import os
import threading

import numpy as np
import pytest

from tests import ivf_sq_ref as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _data(n, dim, dtype=np.float32, seed=0, dup=0):
    rng = np.random.default_rng(seed)
    x = (rng.random((n, dim), dtype=np.float32) * np.float32(1.9) + np.float32(0.1)).astype(dtype)
    if dup:
        x[n - dup:] = x[:dup]  # duplicated rows: exact ties of every metric
    return x


def _build(x, res, metric="sqeuclidean", n_lists=16, **kw):
    import torch
    from cuvs_amd.neighbors import ivf_sq

    p = ivf_sq.IndexParams(n_lists=n_lists, metric=metric, max_train_points_per_cluster=256, kmeans_n_iters=10, **kw)
    src = torch.from_numpy(x).cuda() if not isinstance(x, torch.Tensor) else x
    return ivf_sq.build(p, src, resources=res)


def _search(index, q, k, n_probes, res, filter=None):
    import torch
    from cuvs_amd.neighbors import ivf_sq

    d, i = ivf_sq.search(ivf_sq.SearchParams(n_probes=n_probes), index, torch.from_numpy(q).cuda(), k, resources=res,
                         filter=filter)
    res.sync()
    return d.cpu().numpy(), i.cpu().numpy()


# ------------------------------------------------------------------------------------------------ 1. encode parity
@pytest.mark.parametrize("dtype", [np.float32, np.float16])
@pytest.mark.parametrize("metric,dim", [("sqeuclidean", 33), ("cosine", 17), ("inner_product", 5)])
def test_encode_parity(dtype, metric, dim, res):
    from cuvs_amd.neighbors import ivf_sq

    n, n_lists = 3000, 16  # n <= n_lists * 256: the whole dataset is the training sample
    x = _data(n, dim, dtype, seed=dim)
    index = _build(x, res, metric, n_lists)
    assert len(index) == n and index.n_lists == n_lists and index.dim == dim
    ex = ivf_sq.export_for_oracle(index, resources=res)
    labels = np.empty(n, np.int64)
    for L in range(n_lists):
        labels[ex["ids"][L]] = L
        assert np.all(np.diff(ex["ids"][L]) > 0), "rows are appended in input order"
    assert sorted(np.concatenate(ex["ids"]).tolist()) == list(range(n))
    vmin, delta = S.quantizer(S.residuals(x, ex["centers"], labels, dtype))
    assert np.array_equal(ex["vmin"], vmin) and np.array_equal(ex["delta"], delta)
    for L in range(n_lists):
        want = S.encode(x[ex["ids"][L]], ex["centers"][L], vmin, delta)
        assert np.array_equal(ex["codes"][L], want), f"list {L}"


# ------------------------------------------------------------------------------------------------ 2. search parity
def _parity_cases():
    ks = [1, 10, 64, 100, 256, 300]
    out, n = [], 0
    for metric in ("sqeuclidean", "euclidean", "inner_product", "cosine"):
        for dim in (1, 3, 16, 17, 33, 128, 257):
            if metric == "cosine" and dim == 1:
                dim = 2
            k = ks[n % len(ks)]
            qdt = "f16" if n % 3 == 1 else "f32"
            filt = n % 2 == 1
            out.append(pytest.param(metric, dim, k, qdt, filt, id=f"{metric}-d{dim}-k{k}-{qdt}{'-filter' if filt else ''}"))
            n += 1
    return out


@pytest.mark.parametrize("metric,dim,k,qdt,filt", _parity_cases())
def test_search_parity(metric, dim, k, qdt, filt, res):
    import torch
    from cuvs_amd._lib import BITSET
    from cuvs_amd.neighbors import ivf_sq

    n, n_lists, n_probes, nq = 4000, 20, 6, 60
    x = _data(n, dim, np.float32, seed=100 + dim, dup=400)
    q = _data(nq, dim, np.float16 if qdt == "f16" else np.float32, seed=200 + dim)
    q[:5] = x[:5].astype(q.dtype)  # queries equal to (duplicated) rows
    index = _build(x, res, metric, n_lists)
    ex = ivf_sq.export_for_oracle(index, resources=res)
    flt, bits = None, None
    if filt:
        rng = np.random.default_rng(dim)
        keep = rng.random(n) < 0.7
        bits = np.zeros((n + 31) // 32, np.uint32)
        np.bitwise_or.at(bits, np.nonzero(keep)[0] >> 5, (np.uint32(1) << (np.nonzero(keep)[0] & 31).astype(np.uint32)))
        flt = (torch.from_numpy(bits.view(np.int32)).cuda(), BITSET)
    d, i = _search(index, q, k, n_probes, res, flt)
    wd, wi = S.search(ex, q, k, n_probes, metric, keep_bits=bits)
    assert np.array_equal(i, wi), f"ids differ in {np.count_nonzero((i != wi).any(1))} rows"
    assert np.array_equal(d.view(np.uint32), wd.view(np.uint32)), "distances differ"


def test_search_many_probes_two_phase(res):
    """n_probes > 8 (L2: the nearest list of every query is scanned first) and more than one work item per list"""
    from cuvs_amd.neighbors import ivf_sq

    x = _data(6000, 40, seed=5, dup=300)
    q = _data(300, 40, seed=6)
    index = _build(x, res, "sqeuclidean", 24)
    ex = ivf_sq.export_for_oracle(index, resources=res)
    for k in (10, 100):
        d, i = _search(index, q, k, 12, res)
        wd, wi = S.search(ex, q, k, 12, "sqeuclidean")
        assert np.array_equal(i, wi) and np.array_equal(d.view(np.uint32), wd.view(np.uint32))


# ------------------------------------------------------------------------------------------------ 3. reference table
_TABLE = json.load(open(os.path.join(ROOT, "tests", "golden", "ivf_sq_reference_table.json")))


def _table_params():
    out = []
    for dt in ("float", "half"):
        for n, row in enumerate(_TABLE[dt]):
            out.append(pytest.param(dt, row["case"], id=f"{dt}-inputs-{n:03d}-L{row['line']}"))
    return out


@pytest.mark.parametrize("dt,case", _table_params())
def test_ivf_sq_reference_table(dt, case, res):
    import torch
    from cuvs_amd.neighbors import ivf_sq
    from tests.test_reference_tables_gpu import _eval_neighbours, _gen, _naive_knn

    nq, n, dim, k, nprobe, nlist, metric, host = case
    x = _gen(n, dim, "f16" if dt == "half" else "f32", 1234)
    q = _gen(nq, dim, "f16" if dt == "half" else "f32", 4321)
    ip = ivf_sq.IndexParams(n_lists=nlist, metric=metric, max_train_points_per_cluster=256, add_data_on_build=True)
    index = ivf_sq.build(ip, x.cpu().numpy() if host else x, resources=res)
    d, i = ivf_sq.search(ivf_sq.SearchParams(n_probes=nprobe), index, q, k, resources=res)
    res.sync()
    td, ti = _naive_knn(q, x, k, metric, chunk=16384)
    _eval_neighbours(ti, i, td, d, 0.1, min(1.0, nprobe / nlist))
    del torch


# ------------------------------------------------------------------------------------------------ 4. extend
def test_extend_halves_serialize_to_the_same_bytes(tmp_path, res):
    import torch
    from cuvs_amd.neighbors import ivf_sq

    x = _data(5000, 24, seed=11)
    xt = torch.from_numpy(x).cuda()
    a = _build(xt, res, "sqeuclidean", 16)
    b = _build(xt, res, "sqeuclidean", 16, add_data_on_build=False)
    assert len(b) == 0
    ivf_sq.extend(b, xt[:2500], torch.arange(0, 2500, dtype=torch.int64, device="cuda"), resources=res)
    ivf_sq.extend(b, xt[2500:], torch.arange(2500, 5000, dtype=torch.int64, device="cuda"), resources=res)
    pa, pb = str(tmp_path / "a.bin"), str(tmp_path / "b.bin")
    ivf_sq.save(pa, a, resources=res)
    ivf_sq.save(pb, b, resources=res)
    assert open(pa, "rb").read() == open(pb, "rb").read()


def test_extend_after_build_is_searchable_and_host_inputs_work(res):
    from cuvs_amd._lib import CuvsError
    from cuvs_amd.neighbors import ivf_sq

    x = _data(4000, 16, seed=12)
    extra = _data(500, 16, seed=13)
    index = _build(x, res, "sqeuclidean", 16)
    with pytest.raises(CuvsError, match="indices"):
        ivf_sq.extend(index, extra, None, resources=res)  # a non-empty index needs ids
    ivf_sq.extend(index, extra, np.arange(10**6, 10**6 + 500, dtype=np.int64), resources=res)  # host rows + host ids
    assert len(index) == 4500
    d, i = _search(index, extra[:50], 1, 16, res)
    assert (i[:, 0] == np.arange(10**6, 10**6 + 50)).all()  # every extended row is its own nearest neighbour
    ex = ivf_sq.export_for_oracle(index, resources=res)
    wd, wi = S.search(ex, extra[:50], 10, 5, "sqeuclidean")
    d, i = _search(index, extra[:50], 10, 5, res)
    assert np.array_equal(i, wi) and np.array_equal(d.view(np.uint32), wd.view(np.uint32))
    # a build from host memory equals the build from device memory
    h = ivf_sq.export_for_oracle(_build(x, res, "sqeuclidean", 16), resources=res)
    import torch

    g = ivf_sq.build(ivf_sq.IndexParams(n_lists=16, max_train_points_per_cluster=256, kmeans_n_iters=10), x, resources=res)
    gx = ivf_sq.export_for_oracle(g, resources=res)
    assert all(np.array_equal(a, b) for a, b in zip(h["codes"], gx["codes"])) and np.array_equal(h["centers"], gx["centers"])
    del torch


# ------------------------------------------------------------------------------------------------ 5. serialize
@pytest.mark.parametrize("metric", ["sqeuclidean", "inner_product", "cosine"])
def test_save_load_search_and_reserialize(metric, tmp_path, res):
    from cuvs_amd.neighbors import ivf_sq

    x = _data(3000, 21, seed=21)
    q = _data(40, 21, seed=22)
    index = _build(x, res, metric, 12)
    p1, p2 = str(tmp_path / "1.bin"), str(tmp_path / "2.bin")
    ivf_sq.save(p1, index, resources=res)
    back = ivf_sq.load(p1, resources=res)
    assert len(back) == 3000 and back.n_lists == 12 and back.dim == 21
    d0, i0 = _search(index, q, 10, 4, res)
    d1, i1 = _search(back, q, 10, 4, res)
    assert np.array_equal(i0, i1) and np.array_equal(d0, d1)
    ivf_sq.save(p2, back, resources=res)
    assert open(p1, "rb").read() == open(p2, "rb").read()
    f = S.parse_file(p1)
    assert f["metric"] == S.METRICS[metric] and f["size"] == 3000


def test_file_from_the_restatement_loads_and_searches(tmp_path, res):
    from cuvs_amd.neighbors import ivf_sq

    rng = np.random.default_rng(31)
    n_lists, dim = 6, 19
    centers = rng.standard_normal((n_lists, dim)).astype(np.float32)
    vmin = (-rng.random(dim) - 0.5).astype(np.float32)
    delta = (rng.random(dim) * 0.01 + 0.002).astype(np.float32)
    sizes = [0, 5, 40, 64, 100, 33]
    codes = [rng.integers(0, 256, (s, dim), dtype=np.uint8) for s in sizes]
    ids = [rng.permutation(10**5)[:s].astype(np.int64) + L * 10**5 for L, s in enumerate(sizes)]
    p = str(tmp_path / "r.bin")
    S.write_file(p, centers, vmin, delta, codes, ids, metric=0, center_norms=(centers * centers).sum(1))
    index = ivf_sq.load(p, resources=res)
    ex = dict(centers=centers, vmin=vmin, delta=delta, list_sizes=np.array(sizes, np.uint32), codes=codes, ids=ids)
    q = (rng.standard_normal((30, dim)) * 0.8).astype(np.float32)
    d, i = _search(index, q, 20, 3, res)
    wd, wi = S.search(ex, q, 20, 3, "sqeuclidean")
    assert np.array_equal(i, wi) and np.array_equal(d.view(np.uint32), wd.view(np.uint32))


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals(res, tmp_path):
    import torch
    from cuvs_amd._lib import BITMAP, CuvsError
    from cuvs_amd.neighbors import ivf_sq

    x = _data(2000, 8, seed=41)
    index = _build(x, res, "sqeuclidean", 8)
    bits = torch.full((1 * ((2000 + 31) // 32),), -1, dtype=torch.int32, device="cuda")
    with pytest.raises(CuvsError, match="BITMAP"):
        _search(index, x[:4], 5, 2, res, filter=(bits, BITMAP))
    with pytest.raises(CuvsError, match="dtype"):
        ivf_sq.build(ivf_sq.IndexParams(n_lists=8), torch.ones((100, 8), dtype=torch.int8, device="cuda"), resources=res)
    with pytest.raises(CuvsError, match="n_lists"):
        _build(x[:5], res, "sqeuclidean", 8)
    with pytest.raises(CuvsError, match="Cosine"):
        _build(_data(100, 1), res, "cosine", 4)
    with pytest.raises(CuvsError, match="metric"):
        _build(x, res, "l1", 8)
    with pytest.raises(CuvsError, match="dtype"):
        _search(index, x[:4].astype(np.int8), 5, 2, res)
    bad = str(tmp_path / "bad.bin")
    ivf_sq.save(bad, index, resources=res)
    raw = bytearray(open(bad, "rb").read())
    raw[1] = ord("i")  # "|i1": not the code type
    open(bad, "wb").write(bytes(raw))
    with pytest.raises(CuvsError, match="dtype prefix"):
        ivf_sq.load(bad, resources=res)


# ------------------------------------------------------------------------------------------------ 7. concurrency
def test_two_threads_two_handles_one_index(res):
    import torch
    from cuvs_amd.common import Resources
    from cuvs_amd.neighbors import ivf_sq

    x = _data(8000, 32, seed=51, dup=100)
    q = _data(400, 32, seed=52)
    index = _build(x, res, "sqeuclidean", 32)
    want = {k: _search(index, q, k, 10, res) for k in (10, 100)}
    out, errs = {}, []

    def run(k):
        try:
            torch.cuda.set_device(0)
            r = Resources(stream=torch.cuda.Stream())
            for _ in range(3):
                d, i = ivf_sq.search(ivf_sq.SearchParams(n_probes=10), index, torch.from_numpy(q).cuda(), k, resources=r)
                r.sync()
                out[k] = (d.cpu().numpy(), i.cpu().numpy())
        except Exception as e:  # pragma: no cover - reported below
            errs.append(e)

    ts = [threading.Thread(target=run, args=(k,)) for k in (10, 100)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs
    for k in (10, 100):
        assert np.array_equal(out[k][1], want[k][1]) and np.array_equal(out[k][0], want[k][0])
