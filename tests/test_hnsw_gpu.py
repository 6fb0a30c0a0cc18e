"""GPU: cuvsHnswFromCagra / cuvsHnswBuild (cuvs_amd/csrc/hnsw.hip) and the host search of what they make, against the numpy
twin tests/hnsw_ref.py and the reference's own vectors (tests/golden/hnsw_reference_table.json)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests import hnsw_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = json.load(open(os.path.join(ROOT, "tests", "golden", "hnsw_reference_table.json")))


def _mods():
    from cuvs_amd.neighbors import cagra, hnsw

    return cagra, hnsw


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


def int_rows(rng, n, dim, dtype):
    v = rng.integers(-8, 9, size=(n, dim))
    return (v + 8).astype(dtype) if np.dtype(dtype) == np.uint8 else v.astype(dtype)


def cagra_graph(index):
    import torch

    g = index.graph.cpu().numpy().view(np.uint32).copy()
    torch.cuda.synchronize()
    return g


def saved(hnsw_index, path):
    _, hnsw = _mods()
    hnsw.save(path, hnsw_index)
    return open(path, "rb").read()


def to_hnswlib_bytes(res, cagra_index, path):
    from cuvs_amd._lib import check, lib

    check(lib().cuvsCagraSerializeToHnswlib(res.get_c_obj(), os.fsencode(str(path)), cagra_index._p))
    res.sync()
    return open(path, "rb").read()


# ---------------------------------------------------------------- the reference's vectors
def _check_table(hnsw, index, ef):
    q = np.asarray(TABLE["queries"], dtype=np.float32)
    d, i = hnsw.search(hnsw.SearchParams(ef=ef), index, q, 1)
    print("neighbors", i.ravel().tolist(), "distances", d.ravel().tolist())
    assert i.ravel().tolist() == TABLE["neighbors"]
    assert np.abs(d.ravel() - np.asarray(TABLE["distances"], dtype=np.float32)).max() <= TABLE["distance_tolerance"]


def test_reference_export_deserialize_search(res, tmp_path):
    cagra, hnsw = _mods()
    x = np.asarray(TABLE["dataset"], dtype=np.float32)
    ci = cagra.build(cagra.IndexParams(), x, resources=res)
    f = tmp_path / "cagra_hnswlib.index"
    to_hnswlib_bytes(res, ci, f)
    _check_table(hnsw, hnsw.load(hnsw.IndexParams(hierarchy="none"), f, 2, np.float32), 200)


def test_reference_ace_build_search(res):
    _, hnsw = _mods()
    a = TABLE["ace"]
    ace = hnsw.AceParams(npartitions=a["npartitions"], build_dir="/tmp/hnsw_ace_test", use_disk=False)
    p = hnsw.IndexParams(hierarchy=a["hierarchy"], ef_construction=a["ef_construction"], M=a["M"], metric="sqeuclidean", ace_params=ace)
    _check_table(hnsw, hnsw.build(p, np.asarray(TABLE["dataset"], dtype=np.float32), resources=res), a["ef"])


def test_reference_ace_disk_build_deserialize_search(res, tmp_path):
    from cuvs_amd._lib import CuvsError

    _, hnsw = _mods()
    a = TABLE["ace"]
    build_dir = tmp_path / "hnsw_ace_disk_test" / "nested"
    ace = hnsw.AceParams(npartitions=a["npartitions"], build_dir=build_dir, use_disk=True)
    p = hnsw.IndexParams(hierarchy=a["hierarchy"], ef_construction=a["ef_construction"], M=a["M"], metric="sqeuclidean", ace_params=ace)
    x = np.asarray(TABLE["dataset"], dtype=np.float32)
    built = hnsw.build(p, x, resources=res)
    f = build_dir / "hnsw_index.bin"
    assert f.exists()
    _check_table(hnsw, hnsw.load(p, f, 2, np.float32), a["ef"])
    assert saved(built, tmp_path / "again.bin") == f.read_bytes()
    with pytest.raises(CuvsError, match="ACE parameters must be set for hnsw::build"):
        hnsw.build(hnsw.IndexParams(M=16), x, resources=res)


# ---------------------------------------------------------------- the GPU hierarchy
@pytest.fixture(scope="module")
def base(res, tmp_path_factory):
    """3000 integer-valued rows, dim 32, CAGRA degree 32, converted with the GPU hierarchy; the file and the twin's parse of it"""
    cagra, hnsw = _mods()
    rng = np.random.default_rng(42)
    x = int_rows(rng, 3000, 32, np.float32)
    ci = cagra.build(cagra.IndexParams(graph_degree=32, intermediate_graph_degree=64), _dev(x), resources=res)
    res.sync()
    hi = hnsw.from_cagra(hnsw.IndexParams(hierarchy="gpu", ef_construction=40), ci, resources=res)
    blob = saved(hi, tmp_path_factory.mktemp("hnsw") / "gpu.bin")
    return dict(x=x, cagra=ci, graph=cagra_graph(ci), hnsw=hi, blob=blob, twin=R.Index.from_bytes(blob, 32, np.float32, R.L2, R.GPU))


def test_gpu_hierarchy_levels_and_lists(base):
    t, x = base["twin"], base["x"]
    n = 3000
    assert (t.M, t.maxM, t.maxM0, t.ef_construction) == (16, 16, 32, 40)
    want_levels = R.levels_of(np.arange(n), 16)
    assert want_levels.max() >= 2
    assert np.array_equal(t.levels, want_levels)
    assert t.maxlevel == int(want_levels.max())
    assert t.entry == int(np.nonzero(want_levels == want_levels.max())[0][-1])
    assert t.mult == 1.0 / np.log(16.0)
    for l in range(1, t.maxlevel + 1):
        ids = np.nonzero(want_levels >= l)[0]
        K = min(16, len(ids) - 1)
        sub = x[ids].astype(np.float64)
        d2 = ((sub[:, None, :] - sub[None, :, :]) ** 2).sum(-1)  # exact: integer data
        np.fill_diagonal(d2, np.inf)
        want = np.sort(d2, axis=1)[:, :K]
        for a, i in enumerate(ids.tolist()):
            links = t.links(i, l)
            assert len(links) == K and len(set(links.tolist())) == K and i not in links
            assert (want_levels[links] >= l).all()
            got = ((x[links].astype(np.float64) - x[i].astype(np.float64)) ** 2).sum(-1)
            assert (np.diff(got) >= 0).all(), f"level {l} row {i}: distances not ascending"
            assert np.array_equal(got, want[a]), f"level {l} row {i}: not the {K} nearest of the level"


def test_level0_is_the_cagra_graph(base):
    t = base["twin"]
    assert (t.l0[:, 0] == 32).all() and np.array_equal(t.l0[:, 1:], base["graph"])
    assert np.array_equal(t.rows, base["x"]) and np.array_equal(t.labels, np.arange(3000, dtype=np.uint64))


def test_search_on_the_device_built_index_equals_the_twin(base):
    _, hnsw = _mods()
    q = int_rows(np.random.default_rng(1), 40, 32, np.float32)
    want_i, want_d = base["twin"].search(q, 10, 48)
    for nt in (1, 4):
        d, i = hnsw.search(hnsw.SearchParams(ef=48, num_threads=nt), base["hnsw"], q, 10)
        assert np.array_equal(i, want_i) and np.array_equal(d, want_d)


def test_recall_next_to_cagra_search(res):
    import torch

    cagra, hnsw = _mods()
    rng = np.random.default_rng(7)
    x = rng.standard_normal((5000, 32)).astype(np.float32)
    q = rng.standard_normal((200, 32)).astype(np.float32)
    d2 = (q.astype(np.float64) ** 2).sum(1)[:, None] - 2.0 * q.astype(np.float64) @ x.astype(np.float64).T + (x.astype(np.float64) ** 2).sum(1)[None]
    truth = np.argsort(d2, axis=1)[:, :10]
    ci = cagra.build(cagra.IndexParams(graph_degree=32, intermediate_graph_degree=64), _dev(x), resources=res)
    _, ci_n = cagra.search(cagra.SearchParams(itopk_size=64), ci, _dev(q), 10, resources=res)
    res.sync()
    ci_n = ci_n.cpu().numpy().view(np.uint32)
    torch.cuda.synchronize()
    hi = hnsw.from_cagra(hnsw.IndexParams(hierarchy="gpu"), ci, resources=res)
    _, hn = hnsw.search(hnsw.SearchParams(ef=64), hi, q, 10)

    def recall(got):
        return float(np.mean([len(set(g.tolist()) & set(t.tolist())) / 10.0 for g, t in zip(got, truth)]))

    r_hnsw, r_cagra = recall(hn), recall(ci_n)
    print(f"recall@10: hnsw ef 64 {r_hnsw:.4f}, cagra itopk 64 {r_cagra:.4f}")
    assert r_hnsw >= r_cagra - 0.05


# ---------------------------------------------------------------- packing
@pytest.mark.parametrize("dtype", [np.float32, np.float16, np.int8, np.uint8], ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("dim,degree", [(5, 7), (32, 32)])
def test_packed_records(monkeypatch, tmp_path, dtype, dim, degree):
    """1000 rows in chunks of 300 (four chunks, the last of 100), through hnsw_pack_kernel and through the host loop"""
    import cuvs_amd

    cagra, hnsw = _mods()
    rng = np.random.default_rng(dim)
    x = int_rows(rng, 1000, dim, dtype)
    g = rng.integers(0, 1000, size=(1000, degree)).astype(np.uint32)
    blobs = []
    for host_loop in ("0", "1"):
        monkeypatch.setenv("CUVS_AMD_HNSW_PACK_ROWS", "300")
        monkeypatch.setenv("CUVS_AMD_HNSW_PACK_HOST", host_loop)
        r = cuvs_amd.common.Resources()
        ci = cagra.from_graph(_dev(g.view(np.int32)), _dev(x), resources=r)
        hi = hnsw.from_cagra(hnsw.IndexParams(hierarchy="gpu"), ci, resources=r)
        r.sync()
        blobs.append(saved(hi, tmp_path / f"p{host_loop}.bin"))
    assert blobs[0] == blobs[1]
    t = R.Index.from_bytes(blobs[0], dim, dtype, R.L2, R.GPU)
    assert t.maxM0 == 2 * ((degree + 1) // 2)
    assert (t.l0[:, 0] == degree).all() and np.array_equal(t.l0[:, 1:degree + 1], g) and (t.l0[:, degree + 1:] == 0).all()
    assert np.array_equal(t.rows, x) and np.array_equal(t.labels, np.arange(1000, dtype=np.uint64))
    assert np.array_equal(t.levels, R.levels_of(np.arange(1000), t.M))


# ---------------------------------------------------------------- NONE, CPU, extend
@pytest.mark.parametrize("dtype,dim", [(np.float32, 32), (np.uint8, 5)])
def test_none_writes_the_bytes_of_the_cagra_export(res, tmp_path, dtype, dim):
    cagra, hnsw = _mods()
    x = int_rows(np.random.default_rng(2), 1500, dim, dtype)
    ci = cagra.build(cagra.IndexParams(graph_degree=16, intermediate_graph_degree=32), _dev(x), resources=res)
    res.sync()
    hi = hnsw.from_cagra(hnsw.IndexParams(hierarchy="none"), ci, resources=res)
    want = to_hnswlib_bytes(res, ci, tmp_path / "export.bin")
    assert saved(hi, tmp_path / "none.bin") == want
    q = x[:16]
    d, i = hnsw.search(hnsw.SearchParams(ef=32), hi, q, 5)
    want_i, want_d = R.Index.from_bytes(want, dim, dtype, R.L2, R.NONE).search(q, 5, 32)
    assert np.array_equal(i, want_i) and np.array_equal(d, want_d)


def test_cpu_hierarchy_equals_the_twin(res, tmp_path):
    cagra, hnsw = _mods()
    x = int_rows(np.random.default_rng(3), 2000, 32, np.int8)
    ci = cagra.build(cagra.IndexParams(graph_degree=32, intermediate_graph_degree=64, metric="inner_product"), _dev(x), resources=res)
    res.sync()
    hi = hnsw.from_cagra(hnsw.IndexParams(hierarchy="cpu", ef_construction=40), ci, resources=res)
    t = R.Index.from_graph(x, cagra_graph(ci), R.IP, R.CPU, 40)
    t.build_cpu_hierarchy()
    assert t.maxlevel >= 2
    assert saved(hi, tmp_path / "cpu.bin") == t.to_bytes()


def test_extend_of_a_gpu_hierarchy_equals_the_twin(res, tmp_path):
    cagra, hnsw = _mods()
    x = int_rows(np.random.default_rng(4), 2200, 32, np.float32)
    ci = cagra.build(cagra.IndexParams(graph_degree=32, intermediate_graph_degree=64), _dev(x[:2000]), resources=res)
    res.sync()
    hi = hnsw.from_cagra(hnsw.IndexParams(hierarchy="gpu", ef_construction=40), ci, resources=res)
    t = R.Index.from_bytes(saved(hi, tmp_path / "before.bin"), 32, np.float32, R.L2, R.GPU)
    hnsw.extend(hnsw.ExtendParams(), hi, x[2000:])
    t.extend(x[2000:])
    assert saved(hi, tmp_path / "after.bin") == t.to_bytes()
    d, i = hnsw.search(hnsw.SearchParams(ef=64), hi, x[2000:2020], 1)
    found = i.ravel() == np.arange(2000, 2020)  # the added rows are found (the walk is approximate: most, not all)
    assert found.mean() >= 0.9 and (d.ravel()[found] == 0).all()


# ---------------------------------------------------------------- refusals
def test_refusals(res, base, tmp_path):
    import torch

    from cuvs_amd._lib import CuvsError, Tensor, check, lib

    cagra, hnsw = _mods()
    rng = np.random.default_rng(6)
    # a compressed index: only with the rows
    x = rng.standard_normal((3000, 32)).astype(np.float32)
    vp = cagra.build(cagra.IndexParams(graph_degree=16, intermediate_graph_degree=32, compression=cagra.CompressionParams()), _dev(x),
                     resources=res)
    res.sync()
    assert vp.compressed
    with pytest.raises(CuvsError, match="VPQ"):
        hnsw.from_cagra(hnsw.IndexParams(), vp, resources=res)
    with pytest.raises(CuvsError, match="dataset is"):
        hnsw.from_cagra(hnsw.IndexParams(), vp, dataset=x[:100], resources=res)
    with pytest.raises(CuvsError, match="dtype differs"):
        hnsw.from_cagra(hnsw.IndexParams(), vp, dataset=x.astype(np.float16), resources=res)
    for ds in (x, _dev(x)):  # host and device rows
        hi = hnsw.from_cagra(hnsw.IndexParams(), vp, dataset=ds, resources=res)
        d, i = hnsw.search(hnsw.SearchParams(ef=64), hi, x[:50], 1)
        found = i.ravel() == np.arange(50)  # a row is its own nearest neighbour; the walk is approximate, so most, not all
        assert found.mean() >= 0.9 and (d.ravel()[found] == 0).all()
    # metrics without a space
    bits = rng.integers(0, 256, size=(600, 16)).astype(np.uint8)
    ham = cagra.build(cagra.IndexParams(metric="bitwise_hamming", build_algo="auto", graph_degree=16, intermediate_graph_degree=32),
                      _dev(bits), resources=res)
    with pytest.raises(CuvsError, match="Hamming"):
        hnsw.from_cagra(hnsw.IndexParams(), ham, resources=res)
    cos = cagra.build(cagra.IndexParams(metric="cosine", graph_degree=16, intermediate_graph_degree=32), _dev(x[:600]), resources=res)
    with pytest.raises(CuvsError, match="Unsupported metric type was used"):
        hnsw.from_cagra(hnsw.IndexParams(), cos, resources=res)
    with pytest.raises(CuvsError, match="Unsupported metric type was used"):
        hnsw.build(hnsw.IndexParams(metric="cosine", ace_params=hnsw.AceParams()), x[:600], resources=res)
    # extend on NONE
    none = hnsw.from_cagra(hnsw.IndexParams(hierarchy="none"), base["cagra"], resources=res)
    with pytest.raises(CuvsError, match="immutable"):
        hnsw.extend(hnsw.ExtendParams(), none, base["x"][:4])
    # search arguments
    hi, q = base["hnsw"], base["x"][:4]
    with pytest.raises(CuvsError, match="type mismatch between index and queries"):
        hnsw.search(hnsw.SearchParams(), hi, q.astype(np.float16), 3)
    with pytest.raises(CuvsError, match="neighbors should be of type uint64_t"):
        hnsw.search(hnsw.SearchParams(), hi, q, 3, neighbors=np.zeros((4, 3), dtype=np.uint32))
    with pytest.raises(CuvsError, match="distances should be of type float32"):
        hnsw.search(hnsw.SearchParams(), hi, q, 3, distances=np.zeros((4, 3), dtype=np.float64))
    sp = hnsw.SearchParams()
    host = dict(q=q, n=np.zeros((4, 3), dtype=np.uint64), d=np.zeros((4, 3), dtype=np.float32))
    dev = dict(q=_dev(q), n=torch.zeros((4, 3), dtype=torch.int64, device="cuda"), d=torch.zeros((4, 3), dtype=torch.float32, device="cuda"))
    for which, text in (("q", "queries"), ("n", "neighbors"), ("d", "distances")):
        args = dict(host)
        args[which] = dev[which]
        tn = Tensor(args["n"])
        tn.m.dl_tensor.dtype.code = 1  # uint64; torch has no such dtype
        with pytest.raises(CuvsError, match=f"{text} should have host compatible memory"):
            check(lib().cuvsHnswSearch(C.c_size_t(0), sp._p, hi._p, Tensor(args["q"]).ptr, tn.ptr, Tensor(args["d"]).ptr))
