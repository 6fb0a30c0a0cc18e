"""GPU: exact Hamming kNN and Hamming distance matrices over packed bit codes (cuvs_amd.neighbors.binary_brute_force, DESIGN
3.1zc) against numpy on unpacked bits. Everything is an exact integer: ids and distances are compared with array_equal.

Shapes follow the kernel's constants (cuvs_amd/csrc/binary_knn.hip): a K chunk is CHUNK = 64 bytes, a workgroup owns 128
queries and steps over 256 dataset rows, a wave's row tile is 32 rows, the fused epilogue serves k <= 64."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CHUNK = 64
FLT_MAX = np.finfo(np.float32).max


def _codes(seed, rows, nbytes, dtype=np.uint8):
    rng = np.random.default_rng(seed)
    lo, hi = (0, 256) if dtype == np.uint8 else (-128, 128)
    return rng.integers(lo, hi, size=(rows, nbytes), dtype=dtype)


def _ref_matrix(q, x):
    bq = np.unpackbits(q.view(np.uint8), axis=1).astype(np.int64)
    bx = np.unpackbits(x.view(np.uint8), axis=1).astype(np.int64)
    return bq @ (1 - bx).T + (1 - bq) @ bx.T


def _ref_knn(q, x, k, keep=None):
    """(ids [m, k], distances [m, k], valid slots [m]) by (distance, id) among the rows `keep` ([m, n] bool) leaves."""
    dist = _ref_matrix(q, x)
    keep = np.ones(dist.shape, bool) if keep is None else np.broadcast_to(keep, dist.shape)
    ids = np.full((len(q), k), -1, np.int64)
    out = np.full((len(q), k), FLT_MAX, np.float32)
    cnt = np.zeros(len(q), np.int64)
    for i in range(len(q)):
        cand = np.flatnonzero(keep[i])
        top = cand[np.lexsort((cand, dist[i, cand]))[:k]]
        cnt[i] = len(top)
        ids[i, : len(top)] = top
        out[i, : len(top)] = dist[i, top]
    return ids, out, cnt


def _check_knn(res, x, q, k, tx=None, tq=None, keep=None, prefilter=None):
    import torch
    from cuvs_amd.neighbors import binary_brute_force as bbf

    tx = torch.from_numpy(x).cuda() if tx is None else tx
    tq = torch.from_numpy(q).cuda() if tq is None else tq
    d, i = bbf.knn(tx, tq, k, prefilter=prefilter, resources=res)
    stats = bbf.last_stats(res)
    res.sync()
    d, i = d.cpu().numpy(), i.cpu().numpy()
    ri, rd, cnt = _ref_knn(q, x, k, keep)
    real = np.arange(k)[None, :] < cnt[:, None]
    assert np.array_equal(i[real], ri[real]) and np.array_equal(d[real], rd[real])
    assert ((i[~real] < 0) | (i[~real] >= len(x))).all()
    return stats


@pytest.mark.parametrize(
    "nbytes",
    [1, 3, 16, 37, pytest.param(CHUNK, id="chunk"), pytest.param(CHUNK + 1, id="chunk+1"), pytest.param(2 * CHUNK + 2, id="2chunks+2")],
)
def test_k_tails(res, nbytes):
    """byte tail, word tail, exactly one chunk, one chunk + 1 byte, two chunks + tail; nbytes = 1 (9 distances) is the tie stress"""
    stats = _check_knn(res, _codes(1, 1000, nbytes), _codes(2, 70, nbytes), 10)
    assert stats[2] == (nbytes + CHUNK - 1) // CHUNK and stats[3] == (2 if nbytes > 2 * CHUNK else 1)


def test_queries_restaged_when_the_lists_need_the_lds(res):
    """k = 20: 32-slot lists leave room for one chunk of expanded queries, so 130 bytes are three stagings per row step"""
    assert _check_knn(res, _codes(3, 1000, 2 * CHUNK + 2), _codes(4, 70, 2 * CHUNK + 2), 20)[3] == 3


@pytest.mark.parametrize("n", [31, 32, 33, 257])
@pytest.mark.parametrize("m", [1, 33, 129, 300])
def test_row_and_query_tails(res, m, n):
    _check_knn(res, _codes(5, n, 16), _codes(6, m, 16), min(10, n))


def test_signed_bytes(res):
    _check_knn(res, _codes(7, 1000, 37, np.int8), _codes(8, 70, 37, np.int8), 10)


@pytest.mark.parametrize("k", [1, 64, 65, 200, 600])
def test_k_edges(res, k):
    """64 is the last fused k, 65 the first on the tiled fallback, 600 is k > n padding"""
    stats = _check_knn(res, _codes(9, 500, 16), _codes(10, 70, 16), k)
    assert stats[1] == (1 if k <= 64 else 0)


def test_column_splits(res):
    stats = _check_knn(res, _codes(11, 40000, 16), _codes(12, 3, 16), 10)
    assert stats[0] >= 2 and stats[1] == 1


def test_strided_rows(res):
    import torch

    wx, wq = _codes(13, 1000, 50), _codes(14, 70, 43)
    x, q = np.ascontiguousarray(wx[:, 5:42]), np.ascontiguousarray(wq[:, 3:40])
    _check_knn(res, x, q, 10, tx=torch.from_numpy(wx).cuda()[:, 5:42], tq=torch.from_numpy(wq).cuda()[:, 3:40])


@pytest.mark.parametrize("kind", ["bitset", "bitmap"])
def test_filters(res, kind):
    """BITSET: ~70 % of the rows kept, one whole 128-row span removed. BITMAP: another mask per query, query 0 keeps 4 rows (< k)"""
    import torch
    from cuvs_amd._lib import BITMAP, BITSET

    x, q = _codes(15, 1000, 16), _codes(16, 70, 16)
    rng = np.random.default_rng(17)
    if kind == "bitset":
        keep = rng.random(1000) < 0.7
        keep[256:384] = False
        keep = keep[None, :]
    else:
        keep = rng.random((70, 1000)) < 0.5
        keep[0] = False
        keep[0, [3, 500, 501, 999]] = True
    bits = np.packbits(keep.reshape(-1), bitorder="little")
    words = np.concatenate([bits, np.zeros(-len(bits) % 4, np.uint8)]).view(np.int32)
    stats = _check_knn(res, x, q, 10, keep=keep, prefilter=(torch.from_numpy(words).cuda(), BITSET if kind == "bitset" else BITMAP))
    assert stats[1] == 0


@pytest.mark.parametrize("nbytes", [3, CHUNK + 1, 2 * CHUNK + 2])
def test_pairwise_distance(res, nbytes):
    import torch
    from cuvs_amd.neighbors import binary_brute_force as bbf

    x, q = _codes(1, 1000, nbytes), _codes(2, 70, nbytes)
    out = bbf.pairwise_distance(torch.from_numpy(q).cuda(), torch.from_numpy(x).cuda(), resources=res)
    res.sync()
    assert np.array_equal(out.cpu().numpy(), _ref_matrix(q, x).astype(np.float32))


@pytest.mark.parametrize(
    "case, message",
    [
        ("float rows", "uint8 or int8"),
        ("mismatched dtypes", "same dtype"),
        ("mismatched nbytes", "nbytes mismatch"),
        ("neighbors dtype", "neighbors must be int64"),
        ("distances dtype", "distances must be float32"),
        ("host tensors", "device memory"),
    ],
)
def test_refusals(res, case, message):
    import torch
    from cuvs_amd._lib import CuvsError
    from cuvs_amd.neighbors import binary_brute_force as bbf

    x, q = torch.from_numpy(_codes(1, 100, 16)).cuda(), torch.from_numpy(_codes(2, 8, 16)).cuda()
    kw = {}
    if case == "float rows":
        x, q = x.float(), q.float()
    elif case == "mismatched dtypes":
        q = q.view(torch.int8)
    elif case == "mismatched nbytes":
        q = q[:, :8].contiguous()
    elif case == "neighbors dtype":
        kw["neighbors"] = torch.empty((8, 4), dtype=torch.int32, device="cuda")
    elif case == "distances dtype":
        kw["distances"] = torch.empty((8, 4), dtype=torch.float64, device="cuda")
    else:
        x, q = x.cpu(), q.cpu()
    with pytest.raises(CuvsError, match=message):
        bbf.knn(x, q, 4, resources=res, **kw)
