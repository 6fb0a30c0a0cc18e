"""GPU: CAGRA over a VPQ-compressed dataset (cuvsCagraIndexParams::compression).

The walk over codes computes team_distances<float> on the decoded row float(vq_book[label][d]) + float(pq_book[code][d % pq_len]),
so two twins exist: oracle.cagra_search over the decoded fp32 rows on the CPU, and an uncompressed index made by
cagra.from_graph(graph, decoded rows) on the device. The single-workgroup walk is pinned to both bit for bit; the multi-wave
walk, whose claims race, through the distances of shared ids and a recall comparison with the twin index."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle
from tests import cagra_vpq_ref as V
from tests import product_quantizer_ref as P

pytestmark = pytest.mark.gpu

NQ, K = 64, 10
F32, F16, I8, U8 = "float32", "float16", "int8", "uint8"


# ------------------------------------------------------------------ data and indexes (made once, never modified)
@functools.lru_cache(maxsize=None)
def _data(dtype, n, dim, nq=NQ):
    """the reference's rows (ann_cagra.cuh): uniform [0.1, 2.0) for float types, integers in [1, 20) for int8 / uint8"""
    rng = np.random.default_rng(1000 * dim + n + {F32: 1, F16: 2, I8: 3, U8: 4}[dtype])
    if dtype in (I8, U8):
        x, q = rng.integers(1, 20, size=(n, dim)), rng.integers(1, 20, size=(nq, dim))
    else:
        x, q = rng.uniform(0.1, 2.0, size=(n, dim)), rng.uniform(0.1, 2.0, size=(nq, dim))
    x, q = x.astype(dtype), q.astype(dtype)
    x.setflags(write=False)
    q.setflags(write=False)
    return x, q


class _Built:
    pass


@functools.lru_cache(maxsize=None)
def _built(dtype, n, dim, pq_dim, vq_n, nq=NQ):
    import torch
    from cuvs_amd.neighbors import cagra

    x, q = _data(dtype, n, dim, nq)
    b = _Built()
    comp = cagra.CompressionParams(pq_dim=pq_dim, vq_n_centers=vq_n)
    b.index = cagra.build(cagra.IndexParams(graph_degree=16, intermediate_graph_degree=32, compression=comp), torch.from_numpy(x.copy()).cuda())
    b.x, b.q = x, q
    b.graph = b.index.graph.cpu().numpy().view(np.uint32).copy()
    vq, pq, codes = b.index.vpq()
    b.vq, b.pq, b.codes = vq.cpu().numpy(), pq.cpu().numpy(), codes.cpu().numpy()
    b.decoded = V.decode(b.vq, b.pq, b.codes)
    for a in (b.graph, b.vq, b.pq, b.codes, b.decoded):
        a.setflags(write=False)
    return b


@functools.lru_cache(maxsize=None)
def _twin(dtype, n, dim, pq_dim, vq_n):
    """the uncompressed fp32 index over the decoded rows and the same graph"""
    import torch
    from cuvs_amd.neighbors import cagra

    b = _built(dtype, n, dim, pq_dim, vq_n)
    return cagra.from_graph(torch.from_numpy(b.graph.view(np.int32).copy()).cuda(), torch.from_numpy(b.decoded.copy()).cuda())


def _pack(keep):
    pad = np.zeros((-keep.size) % 32, bool)
    return np.packbits(np.concatenate([keep, pad]), bitorder="little").view(np.uint32).copy()


def _search(index, q, k=K, words=None, out="uint32", **params):
    """(distances float32, ids int64 with -1 for padding)"""
    import torch
    from cuvs_amd._lib import BITSET
    from cuvs_amd.neighbors import cagra

    tq = torch.from_numpy(np.array(q, copy=True)).cuda()
    nb = torch.empty((q.shape[0], k), dtype=torch.int64 if out == "int64" else torch.int32, device="cuda")
    flt = None if words is None else (torch.from_numpy(words.view(np.int32)).cuda(), BITSET)
    d, i = cagra.search(cagra.SearchParams(**params), index, tq, k, neighbors=nb, filter=flt)
    torch.cuda.synchronize()
    if out == "int64":
        ids = i.cpu().numpy()
    else:
        raw = i.cpu().numpy().view(np.uint32)
        ids = np.where(raw == 0xFFFFFFFF, -1, raw.astype(np.int64))
    return d.cpu().numpy(), ids


def _oracle(b, k=K, words=None, **params):
    od, oi = oracle.cagra_search(b.decoded, b.graph, b.q.astype(np.float32), k, filter_words=words, **params)
    return od, oi


def _same_bits(got, want):
    (gd, gi), (wd, wi) = got, want
    return np.array_equal(gi, wi) and np.array_equal(gd.view(np.uint32), wd.view(np.uint32))


# ------------------------------------------------------------------ artefacts
ART = (F32, 3000, 32, 8, 16)


def test_artefacts_shapes_padding_and_fp16_books():
    b = _built(*ART)
    n, dim, pq_dim, vq_n = 3000, 32, 8, 16
    assert b.index.compressed and len(b.index) == n and b.index.dim == dim
    assert b.index._vpq_info() == [vq_n, 256, 4, V.row_len(pq_dim), dim] and V.row_len(pq_dim) == 4 * (1 + -(-pq_dim * 8 // 32))
    assert b.vq.shape == (vq_n, dim) and b.vq.dtype == np.float16
    assert b.pq.shape == (256, 4) and b.pq.dtype == np.float16
    assert b.codes.shape == (n, V.row_len(pq_dim)) and b.codes.dtype == np.uint8
    assert np.isfinite(b.vq.astype(np.float32)).all() and np.isfinite(b.pq.astype(np.float32)).all()
    # the books are fp16 on the device (the accessor copies, it does not convert), and these values are the ones the walk reads:
    # the parity tests decode with them and compare distance bits
    labels, codes, pad = V.split_codes(b.codes, pq_dim)
    assert labels.max() < vq_n and not pad.any()
    # dim 6, pq_len 2: pq_dim 3, one padding byte per row, and it is zero
    b6 = _built(F32, 3000, 6, 3, 16)
    assert b6.codes.shape == (3000, 8) and not V.split_codes(b6.codes, 3)[2].any()
    b136 = _built(F32, 3000, 136, 34, 16)
    assert b136.codes.shape == (3000, 4 + 36) and not V.split_codes(b136.codes, 34)[2].any()


def test_labels_and_codes_are_the_best_for_the_rounded_books():
    """the bounds of tests/test_product_quantizer_gpu.py: the label within the bound of the expanded form kmeans_predict
    evaluates, the codes within (1 + 4 (pq_len + 2) 2^-24) of the fp64 best - against the fp16 books the index exposes"""
    for key in (ART, (F16, 3000, 32, 8, 16), (U8, 3000, 32, 8, 16), (F32, 3000, 6, 3, 16)):
        b = _built(*key)
        dim, pq_dim = key[2], key[3]
        pq_len = dim // pq_dim
        x = b.x.astype(np.float32)
        vq32, pq32 = b.vq.astype(np.float32), b.pq.astype(np.float32)
        labels, codes, _ = V.split_codes(b.codes, pq_dim)
        x64, v64 = x.astype(np.float64), vq32.astype(np.float64)
        d = ((x64[:, None, :] - v64[None, :, :]) ** 2).sum(2)
        slack = 8 * (dim + 4) * 2.0 ** -24 * ((x64 ** 2).sum(1) + (v64 ** 2).sum(1).max())
        assert (d[np.arange(len(x)), labels] <= d.min(1) + slack).all()
        r = P.residual(x, vq32, labels)
        worst, differ = P.distance_excess(r, pq32, codes.astype(np.int64), pq_dim, pq_len, 8, False)
        allowed = 4 * (pq_len + 2) * 2.0 ** -24
        print(f"{key}: {differ} of {codes.size} codes differ from the fp64 argmin, worst excess {worst:.3e}, allowed {allowed:.3e}")
        assert worst <= allowed


def test_default_heuristics():
    import torch
    from cuvs_amd.neighbors import cagra

    x, _ = _data(F32, 3000, 32)
    ip = cagra.IndexParams(graph_degree=16, intermediate_graph_degree=32, compression=cagra.CompressionParams())
    index = cagra.build(ip, torch.from_numpy(x.copy()).cuda())
    vq_n, pq_n, pq_len, row_len, dim = index._vpq_info()
    assert (vq_n, pq_n, pq_len, row_len, dim) == (56, 256, 4, 12, 32)  # sqrt(3000) = 54 -> 56; pq_dim = 32 / 4
    # a host dataset builds the same way
    hidx = cagra.build(ip, x.copy())
    assert hidx.compressed and hidx._vpq_info() == [56, 256, 4, 12, 32]


# ------------------------------------------------------------------ walk parity (single workgroup)
PARITY = [
    (F32, 3000, 6, 3, 16),      # pq_len 2; dim no multiple of 4, one padding byte in the code row
    (F32, 3000, 8, 4, 16),      # pq_len 2
    (F32, 3000, 32, 8, 16),     # pq_len 4
    (F32, 3000, 136, 34, 16),   # pq_len 4; two padding bytes, the second 32-element round has two active lanes
    (F32, 2000, 768, 192, 16),  # pq_len 4; the long loop with several pieces in flight
    (F16, 3000, 32, 8, 16), (I8, 3000, 32, 8, 16), (U8, 3000, 32, 8, 16),
    (F16, 3000, 64, 32, 16),    # pq_len 2 over more than one round
]


@pytest.mark.parametrize("key", PARITY, ids=["%s-n%d-dim%d-pqdim%d-vq%d" % k for k in PARITY])
def test_single_walk_equals_the_oracle_and_the_twin_index(key):
    b = _built(*key)
    got = _search(b.index, b.q, algo="single_cta", itopk_size=64)
    assert (got[1] >= 0).all()
    assert _same_bits(got, _oracle(b, itopk_size=64))
    twin = _search(_twin(*key), b.q.astype(np.float32), algo="single_cta", itopk_size=64)
    assert _same_bits(got, twin)
    # an independent anchor: the distances are those of the decoded rows
    d64 = ((b.q.astype(np.float64)[:, None, :] - b.decoded.astype(np.float64)[got[1]]) ** 2).sum(2)
    np.testing.assert_allclose(got[0], d64, rtol=1e-5)


def test_wide_walk_random_samplings_and_int64_neighbours():
    b = _built(*ART)
    got = _search(b.index, b.q, out="int64", algo="single_cta", itopk_size=64, search_width=2, num_random_samplings=2)
    assert _same_bits(got, _oracle(b, itopk_size=64, search_width=2, num_random_samplings=2))
    twin = _search(_twin(*ART), b.q, out="int64", algo="single_cta", itopk_size=64, search_width=2, num_random_samplings=2)
    assert _same_bits(got, twin)


@pytest.mark.parametrize("which", ["every_other", "all_but_20"])
def test_filtered_walk_equals_the_oracle(which):
    b = _built(*ART)
    n = len(b.x)
    keep = np.zeros(n, bool)
    if which == "every_other":
        keep[::2] = True
    else:
        keep[np.random.default_rng(5).choice(n, 20, replace=False)] = True
    words = _pack(keep)
    got = _search(b.index, b.q, words=words, algo="single_cta", itopk_size=64)
    want = _oracle(b, words=words, itopk_size=64)
    assert _same_bits(got, want)
    real = got[1][got[1] >= 0]
    assert keep[real].all()
    if which == "every_other":
        assert (got[1] >= 0).all()


def test_work_counters_count_rows_of_a_compressed_walk():
    import torch
    from cuvs_amd._lib import lib
    from cuvs_amd.common import Resources
    from cuvs_amd.neighbors import cagra

    b = _built(*ART)
    res = Resources()
    out = (C.c_uint64 * 3)()
    assert lib().cuvsAmdCagraWorkCounters(res.get_c_obj(), 1, out) == 1
    cagra.search(cagra.SearchParams(algo="single_cta", itopk_size=64), b.index, torch.from_numpy(b.q.copy()).cuda(), K, resources=res)
    res.sync()
    assert lib().cuvsAmdCagraWorkCounters(res.get_c_obj(), 0, out) == 1
    rows, graph_rows, walkers = list(out)
    assert walkers == NQ and graph_rows >= NQ and rows >= NQ * (64 + 16)  # every walker scores its seeds at least


# ------------------------------------------------------------------ multi-wave walk
def _recall(ids, truth):
    return float(np.mean([len(set(a[a >= 0]) & set(t)) / len(t) for a, t in zip(ids, truth)]))


@pytest.mark.parametrize("key", [ART, (F16, 3000, 64, 32, 16)], ids=["f32-dim32-pqlen4", "f16-dim64-pqlen2"])
def test_multi_wave_walk(key):
    b = _built(*key)
    qf = b.q.astype(np.float32)
    sd, si = _search(b.index, b.q, algo="single_cta", itopk_size=64)
    md, mi = _search(b.index, b.q, algo="multi_cta", itopk_size=64)
    assert (mi >= 0).all() and (md[:, 1:] >= md[:, :-1]).all()
    shared = 0
    for r in range(NQ):
        assert len(set(mi[r])) == K
        pos = {int(i): j for j, i in enumerate(si[r])}
        for j, i in enumerate(mi[r]):
            if int(i) in pos:
                shared += 1
                assert md[r, j].view(np.uint32) == sd[r, pos[int(i)]].view(np.uint32)
    assert shared > NQ * K // 2
    d64 = ((qf.astype(np.float64) ** 2).sum(1)[:, None] + (b.decoded.astype(np.float64) ** 2).sum(1)[None, :]
           - 2.0 * qf.astype(np.float64) @ b.decoded.astype(np.float64).T)
    truth = np.argsort(d64, axis=1, kind="stable")[:, :K]
    _, ti = _search(_twin(*key), qf, algo="multi_cta", itopk_size=64)
    mine, twin = _recall(mi, truth), _recall(ti, truth)
    print(f"{key}: multi_cta recall@{K} over the decoded rows: compressed {mine:.4f}, twin index {twin:.4f}")
    assert mine >= twin - 0.02  # the claims race: two runs of the same walk differ by about this much


# ------------------------------------------------------------------ files
def _roundtrip_same(b, index):
    return _same_bits(_search(index, b.q, algo="single_cta", itopk_size=64), _search(b.index, b.q, algo="single_cta", itopk_size=64))


def test_reference_format_file(tmp_path):
    from cuvs_amd.neighbors import cagra

    b = _built(*ART)
    path = str(tmp_path / "vpq.cagra")
    cagra.save(path, b.index)
    f = V.parse_cagra_vpq(path)
    assert (f["prefix"], f["version"], f["size"], f["dim"], f["graph_degree"], f["metric"], f["content_map"]) == (b"<f4\0", 5, 3000, 32, 16, 0, 1)
    assert (f["tag"], f["cuda_dtype"], f["n_rows"], f["ds_dim"], f["vq_n_centers"], f["pq_n_centers"], f["pq_len"],
            f["encoded_row_length"]) == (3, V.CUDA_R_16F, 3000, 32, 16, 256, 4, 12)
    assert np.array_equal(f["graph"], b.graph)
    assert f["vq_code_book"].dtype == np.float16 and np.array_equal(f["vq_code_book"].view(np.uint16), b.vq.view(np.uint16))
    assert f["pq_code_book"].dtype == np.float16 and np.array_equal(f["pq_code_book"].view(np.uint16), b.pq.view(np.uint16))
    assert f["data"].dtype == np.uint8 and np.array_equal(f["data"], b.codes)
    loaded = cagra.load(path)
    assert loaded.compressed and loaded._vpq_info() == b.index._vpq_info()
    assert _roundtrip_same(b, loaded)
    lv, lp, lc = (t.cpu().numpy() for t in loaded.vpq())
    assert np.array_equal(lc, b.codes) and np.array_equal(lv.view(np.uint16), b.vq.view(np.uint16)) and np.array_equal(lp.view(np.uint16), b.pq.view(np.uint16))
    # without the dataset the file is what any index writes, and loads as an index without rows
    bare = str(tmp_path / "bare.cagra")
    cagra.save(bare, b.index, include_dataset=False)
    from tests import refformat as rf
    assert rf.parse_cagra(bare)["content_map"] == 0
    assert not cagra.load(bare).compressed


def test_fp16_index_file_roundtrip(tmp_path):
    from cuvs_amd.neighbors import cagra

    b = _built(F16, 3000, 64, 32, 16)
    path = str(tmp_path / "vpq16.cagra")
    cagra.save(path, b.index)
    assert V.parse_cagra_vpq(path)["prefix"] == b"<e2\0"
    assert _roundtrip_same(b, cagra.load(path))


def test_native_container(tmp_path, monkeypatch):
    from cuvs_amd.neighbors import cagra

    b = _built(*ART)
    monkeypatch.setenv("CUVS_AMD_NATIVE_FORMAT", "1")
    path = str(tmp_path / "vpq_native.bin")
    cagra.save(path, b.index)
    assert open(path, "rb").read(8) == b"CUVSAMD1"
    loaded = cagra.load(path)
    assert loaded.compressed and loaded._vpq_info() == b.index._vpq_info()
    assert np.array_equal(loaded.vpq()[2].cpu().numpy(), b.codes)
    assert _roundtrip_same(b, loaded)


@pytest.mark.parametrize("book_dtype", [np.float16, np.float32], ids=["fp16-books", "fp32-books"])
def test_file_of_the_tests_own_writer_loads(tmp_path, book_dtype):
    from cuvs_amd.neighbors import cagra

    b = _built(*ART)
    path = str(tmp_path / "own.cagra")
    V.write_cagra_vpq(path, b.graph, b.vq, b.pq, b.codes, dtype=np.float32, book_dtype=book_dtype)  # fp32 books hold fp16-exact values
    loaded = cagra.load(path)
    assert loaded.compressed and _roundtrip_same(b, loaded)
    assert np.array_equal(loaded.vpq()[0].cpu().numpy().view(np.uint16), b.vq.view(np.uint16))


def test_corrupted_files_are_refused(tmp_path):
    from cuvs_amd._lib import CuvsError
    from cuvs_amd.neighbors import cagra

    b = _built(*ART)
    bad_label = b.codes.copy()
    bad_label[1234, :4] = np.array([16], "<u4").view(np.uint8)  # vq_n_centers is 16
    pq3 = np.zeros((256, 3), np.float16)
    cases = [
        ("label", dict(codes=bad_label), {}, "VQ label 16"),
        ("row_len", {}, dict(encoded_row_length=16), "encoded_row_length 16, expected 12"),
        ("pq_n", {}, dict(pq_n_centers=512), "pq_n_centers 512"),
        ("pq_len", dict(pq=pq3), {}, "pq_len 3"),
    ]
    for name, arrays, override, text in cases:
        path = str(tmp_path / (name + ".cagra"))
        V.write_cagra_vpq(path, b.graph, b.vq, arrays.get("pq", b.pq), arrays.get("codes", b.codes), **override)
        with pytest.raises(CuvsError, match=text):
            cagra.load(path)
    # a file without rows and a file of another metric have messages of their own
    path = str(tmp_path / "empty.cagra")
    V.write_cagra_vpq(path, b.graph[:0], b.vq, b.pq, b.codes[:0])
    with pytest.raises(CuvsError, match="holds no rows"):
        cagra.load(path)
    path = str(tmp_path / "ip.cagra")
    V.write_cagra_vpq(path, b.graph, b.vq, b.pq, b.codes, metric=6)
    with pytest.raises(CuvsError, match="only supported with L2Expanded"):
        cagra.load(path)


# ------------------------------------------------------------------ refusals
def test_entry_points_that_need_the_rows_refuse_and_leave_the_index_intact(tmp_path):
    import torch
    from cuvs_amd._lib import CuvsError, DLManagedTensor, lib
    from cuvs_amd.common import Resources
    from cuvs_amd.neighbors import cagra, mg, tiered_index

    b = _built(*ART)
    want = _oracle(b, itopk_size=64)

    def intact():
        """the index still answers the parity query"""
        assert b.index.compressed and len(b.index) == 3000
        assert _same_bits(_search(b.index, b.q, algo="single_cta", itopk_size=64), want)

    intact()
    L = lib()
    L.cuvsGetLastErrorText.restype = C.c_char_p
    m = DLManagedTensor()
    assert L.cuvsCagraIndexGetDataset(b.index._p, C.byref(m)) == 0
    assert "cuvsCagraIndexGetDataset: the index holds a VPQ dataset" in L.cuvsGetLastErrorText().decode()
    intact()
    with pytest.raises(CuvsError, match="cuvsCagraExtend: the index holds a VPQ dataset"):
        cagra.extend(b.index, torch.from_numpy(b.x[:10].copy()).cuda())
    intact()
    plain = cagra.IndexParams(graph_degree=16, intermediate_graph_degree=32)
    with pytest.raises(CuvsError, match="cuvsCagraMerge: the index holds a VPQ dataset"):
        cagra.merge(plain, [b.index, b.index])
    intact()
    res = Resources()
    assert L.cuvsCagraSerializeToHnswlib(res.get_c_obj(), C.c_char_p(str(tmp_path / "h.bin").encode()), b.index._p) == 0
    assert "cuvsCagraSerializeToHnswlib: the index holds a VPQ dataset" in L.cuvsGetLastErrorText().decode()
    intact()
    comp = cagra.IndexParams(graph_degree=16, intermediate_graph_degree=32, compression=cagra.CompressionParams(pq_dim=8, vq_n_centers=16))
    with pytest.raises(CuvsError, match="tiered_index: CAGRA compression parameters are not supported"):
        tiered_index.build(tiered_index.IndexParams(algo="cagra", upstream_params=comp, min_ann_rows=100), torch.from_numpy(b.x.copy()).cuda())
    intact()
    with pytest.raises(CuvsError, match="cuvsMultiGpuCagraBuild: VPQ compression parameters are not supported"):
        mg.build("cagra", comp, b.x.copy(), mode="replicated")
    intact()
    # a merge of uncompressed indexes does not compress either: the parameters are refused, the inputs stay as they were
    tx = torch.from_numpy(b.x.copy()).cuda()
    u = cagra.build(plain, tx)
    before = _search(u, b.q, algo="single_cta", itopk_size=64)
    with pytest.raises(CuvsError, match="cuvsCagraMerge: VPQ compression parameters are not supported"):
        cagra.merge(comp, [u, u])
    assert not u.compressed and _same_bits(_search(u, b.q, algo="single_cta", itopk_size=64), before)


# ------------------------------------------------------------------ recall, the reference's table reduced
@pytest.mark.parametrize("dim", [64, 192])
def test_recall_against_the_original_rows(dim):
    """ann_cagra.cuh:1632-1665 reduced: n 10000, 100 queries, k 16, itopk 64, pq_len 2, vq_n_centers 100; recall by id against
    the exact neighbours of the ORIGINAL rows >= 0.6 (the reference's min_recall, :1648; it also accepts equal distances)."""
    n, nq, k = 10000, 100, 16
    b = _built(F32, n, dim, dim // 2, 100, nq)
    _, ids = _search(b.index, b.q, k=k, itopk_size=64)
    x64, q64 = b.x.astype(np.float64), b.q.astype(np.float64)
    d = (q64 ** 2).sum(1)[:, None] + (x64 ** 2).sum(1)[None, :] - 2.0 * q64 @ x64.T
    truth = np.argsort(d, axis=1, kind="stable")[:, :k]
    rec = _recall(ids, truth)
    print(f"dim {dim}: recall@{k} by id against the original rows {rec:.4f}")
    assert rec >= 0.6
