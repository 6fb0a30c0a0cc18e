"""GPU: the head phase's single-pair list scan (pq_head_kernel) with its score keys out of the LDS - a thread keeps its smallest
key, that key's row and its second smallest key in registers; rows of threads with several keys at or below the threshold, and
the rows behind a mass of ties, are scored again - at three workgroups per CU (fp16 LUT up to 32 KiB), two (up to 64 KiB) or one.
Every case: ids AND distances of ivf_pq.search on a default handle equal the oracle's on the exported index and those of a
handle created under CUVS_AMD_PQ_SCAN3=0 (the LUT scan kernels), after the plan hook confirmed that the shape takes the head
kernel (head1, matrix-core tail)."""
import functools

import numpy as np
import pytest

import oracle
from tests.test_ivf_pq_plan_cpu import COSINE, IP, L2, MATRIX_CORE_TAIL, plan_hook

pytestmark = pytest.mark.gpu

_DT = {"f32": np.float32, "f16": np.float16, "fp8": np.uint8}
_METRIC = {"sqeuclidean": L2, "inner_product": IP, "cosine": COSINE}


def _data(n, dim, nq, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    x = ((rng.random((n, dim), dtype=np.float32) * 1.9 + 0.1) * scale).astype(np.float32)
    q = ((rng.random((nq, dim), dtype=np.float32) * 1.9 + 0.1) * scale).astype(np.float32)
    return x, q


@functools.lru_cache(maxsize=None)
def _index(n, dim, seed, scale, n_lists, pq_dim, pq_bits, kind, metric):
    import torch
    from cuvs_amd.neighbors import ivf_pq

    x, q = _data(n, dim, 300, seed, scale)
    index = ivf_pq.build(ivf_pq.IndexParams(n_lists=n_lists, pq_dim=pq_dim, pq_bits=pq_bits, kmeans_n_iters=6, metric=metric,
                                            codebook_kind=kind), torch.from_numpy(x).cuda())
    return index, ivf_pq.export_for_oracle(index, per_cluster=kind == "cluster"), q


def _handles(monkeypatch, **env):
    """a default handle and one created under the given switches"""
    import cuvs_amd

    r0 = cuvs_amd.common.Resources()
    for name, v in env.items():
        monkeypatch.setenv(name, v)
    r1 = cuvs_amd.common.Resources()
    for name in env:
        monkeypatch.delenv(name)
    return r0, r1


def _assert_head_kernel(index, ex, metric, kind, k, nq, n_probes, lut, acc, batch):
    sh = dict(dim=index.dim, rot_dim=index.pq_dim * index.pq_len, pq_dim=index.pq_dim, pq_len=index.pq_len, pq_bits=index.pq_bits,
              kind=1 if kind == "cluster" else 0, metric=_METRIC[metric])
    p = plan_hook(sh, ex["list_sizes"], k, nq, n_probes=n_probes, lut=_DT[lut], score=_DT[acc], batch=batch)
    assert p["path"] == MATRIX_CORE_TAIL and p["head1"], p


def _check(monkeypatch, index, ex, q, *, metric="sqeuclidean", kind="subspace", k=10, n_probes=4, lut="f16", acc="f32", batch=4096,
           keep=None, other=None):
    """search on a default handle == oracle == LUT scan kernels (== a handle created under `other`, when given)"""
    import torch
    from cuvs_amd._lib import BITSET
    from cuvs_amd.neighbors import ivf_pq

    _assert_head_kernel(index, ex, metric, kind, k, len(q), n_probes, lut, acc, batch)
    sp = ivf_pq.SearchParams(n_probes=n_probes, lut_dtype=_DT[lut], internal_distance_dtype=_DT[acc], max_internal_batch_size=batch)
    qt = torch.from_numpy(q).cuda()
    words, flt = None, None
    if keep is not None:
        words = np.packbits(keep, bitorder="little")
        words = np.concatenate([words, np.zeros((-len(words)) % 4, dtype=np.uint8)]).view(np.uint32)
        flt = (torch.from_numpy(words.view(np.int32)).cuda(), BITSET)
    r0, r1 = _handles(monkeypatch, CUVS_AMD_PQ_SCAN3="0")
    d0, i0 = ivf_pq.search(sp, index, qt, k, resources=r0, filter=flt)
    d1, i1 = ivf_pq.search(sp, index, qt, k, resources=r1, filter=flt)
    r0.sync(); r1.sync()
    od, oi = oracle.ivf_pq_search(ex, q, k, n_probes, metric=metric, lut=lut, acc=acc, keep_bits=words)
    gd, gi = d0.cpu().numpy(), i0.cpu().numpy()
    assert (gi == oi).all(), f"ids differ from the oracle's: rate {(gi != oi).mean():.5f}"
    assert (gd == od).all(), "distances differ from the oracle's"
    assert torch.equal(i0, i1) and torch.equal(d0, d1), "results differ from the LUT scan kernels'"
    if other is not None:
        _, r2 = _handles(monkeypatch, **other)
        d2, i2 = ivf_pq.search(sp, index, qt, k, resources=r2, filter=flt)
        r2.sync()
        assert torch.equal(i0, i2) and torch.equal(d0, d2), f"results differ under {other}"
    return gd, gi


def test_lists_beyond_the_chunk_capacity_and_below_the_workgroup(monkeypatch):
    """40000 x 64 rows in blobs of 26203 rows (a list of four chunks of 16 rows per thread, the candidates carried over), of 403
    (shorter than the 512-thread workgroup: threads without a row), of 7 (fewer than k) - no length a multiple of 64 - and nine
    ordinary ones: a search has a head phase from nine probes on (the plan's rule), which three lists cannot give."""
    import torch
    from cuvs_amd.neighbors import ivf_pq

    rng = np.random.default_rng(11)
    dim, n_lists = 64, 12
    sizes = [26203, 403, 7] + [1487] * 8 + [1491]
    assert sum(sizes) == 40000
    corners = np.zeros((n_lists, dim), np.float32)
    for c in range(n_lists):
        corners[c, 4 * c:4 * c + 4] = 40.0

    def blob(c, n):
        return (corners[c] + rng.random((n, dim), dtype=np.float32) * 1.9 + 0.1).astype(np.float32)

    train = np.concatenate([blob(c, 1000) for c in range(n_lists)])
    ip = ivf_pq.IndexParams(n_lists=n_lists, pq_dim=32, kmeans_n_iters=10, kmeans_trainset_fraction=1.0, add_data_on_build=False)
    index = ivf_pq.build(ip, torch.from_numpy(train).cuda())
    x = np.concatenate([blob(c, n) for c, n in enumerate(sizes)])
    ivf_pq.extend(index, torch.from_numpy(x).cuda(), torch.arange(len(x), dtype=torch.int64).cuda())
    ex = ivf_pq.export_for_oracle(index)
    got = [int(v) for v in ex["list_sizes"]]   # (the blobs, give or take one that the clustering split or merged)
    assert sum(got) == 40000 and any(s > 3 * 16 * 512 and s % 64 for s in got), got
    assert any(10 <= s < 512 and s % 64 for s in got) and any(0 < s < 10 for s in got), got
    q = np.concatenate([blob(c, 25) for c in range(n_lists)])   # every list is the nearest of 25 queries
    _check(monkeypatch, index, ex, q, k=10, n_probes=9)


@functools.lru_cache(maxsize=None)
def _ties_index(metric):
    import torch
    from cuvs_amd.neighbors import ivf_pq

    rng = np.random.default_rng(5)
    n, dim = 56000, 64
    x, q = _data(n, dim, 300, 6)
    copies = rng.random(n) < 0.2                     # ~11200 rows: 8 distinct rows, ~1400 copies each (head_cand: 512 / 1024)
    x[copies] = x[:8][rng.integers(0, 8, size=int(copies.sum()))]
    q[:40] = x[:8][rng.integers(0, 8, size=40)] + 0.01   # queries next to the copied rows
    if metric == "inner_product":
        q[40:80] = 0.0
    index = ivf_pq.build(ivf_pq.IndexParams(n_lists=10, pq_dim=32, kmeans_n_iters=6, metric=metric), torch.from_numpy(x).cuda())
    return index, ivf_pq.export_for_oracle(index), q


@pytest.mark.parametrize("metric", ["sqeuclidean", "inner_product"])
@pytest.mark.parametrize("k", [10, 200])
def test_masses_of_ties(metric, k, monkeypatch):
    """About a thousand copies of each of 8 rows: more keys tie at the threshold than head_cand(k) holds (512 / 1024), the
    chunk's k smallest (key, row) are taken one by one, the earliest rows win. All-zero queries under inner product: every
    score of a list ties."""
    index, ex, q = _ties_index(metric)
    _check(monkeypatch, index, ex, q, metric=metric, k=k, n_probes=9)


@pytest.mark.parametrize("k", [10, 100, 200])
def test_group_minima_of_four_two_and_one_threads(k, monkeypatch):
    """k <= 64: minima of groups of four threads; k <= 128: of two; beyond: of one, and candidate buffers of 1024 entries."""
    index, ex, q = _index(56000, 64, 21, 1.0, 10, 32, 8, "subspace", "sqeuclidean")
    _check(monkeypatch, index, ex, q, k=k, n_probes=9, lut="f32")


@pytest.mark.parametrize("lut,acc", [("f16", "f32"), ("f16", "f16"), ("f32", "f32"), ("fp8", "f32")])
def test_lut_and_score_types_at_pq_dim_64(lut, acc, monkeypatch):
    """pq_dim 64: fp16 entries (32 KiB) run three workgroups per CU with the fused convert-add (fp32 scores) or the fp16 add
    chain, fp32 entries and fp8 entries kept in fp32 (64 KiB) two."""
    index, ex, q = _index(30000, 128, 22, 1.0, 12, 64, 8, "subspace", "sqeuclidean")
    _check(monkeypatch, index, ex, q, k=10, n_probes=9, lut=lut, acc=acc)


@pytest.mark.parametrize("metric", ["inner_product", "cosine"])
def test_inner_product_and_cosine(metric, monkeypatch):
    index, ex, q = _index(30000, 128, 22, 1.0, 12, 64, 8, "subspace", metric)
    _check(monkeypatch, index, ex, q, metric=metric, k=10, n_probes=9)


@pytest.mark.parametrize("dim,pq_dim,pq_bits,kind", [(64, 32, 5, "subspace"), (64, 16, 8, "subspace"), (64, 32, 8, "cluster"),
                                                    (256, 128, 8, "subspace")])
def test_codebook_shapes(dim, pq_dim, pq_bits, kind, monkeypatch):
    """5-bit codes; pq_len 4; a PER_CLUSTER codebook; pq_dim 128 (fp16 entries: 64 KiB, two workgroups per CU and the lookups'
    second unrolled group; fp32 entries: 128 KiB, one 1024-thread workgroup)"""
    index, ex, q = _index(20000, dim, 23, 1.0, 10, pq_dim, pq_bits, kind, "sqeuclidean")
    _check(monkeypatch, index, ex, q, kind=kind, k=10, n_probes=9, lut="f16")
    if pq_dim == 128:
        _check(monkeypatch, index, ex, q, kind=kind, k=10, n_probes=9, lut="f32")


@pytest.mark.parametrize("acc", ["f32", "f16"])
def test_subnormal_fp16_lut_entries(acc, monkeypatch):
    """The data scaled by 1e-3: squared differences of 1e-6 and less - LUT entries below fp16's smallest normal 6.1e-5 - meet
    the fused convert-add."""
    index, ex, q = _index(30000, 128, 24, 1e-3, 12, 64, 8, "subspace", "sqeuclidean")
    lut = np.array(ex["pq_centers"])
    assert float(np.abs(lut).max()) < 0.05, "the residuals' codebook is of the order of the scaled data"
    _check(monkeypatch, index, ex, q, k=10, n_probes=9, lut="f16", acc=acc)


def test_bitset_prefilter_removing_half_of_the_rows_and_one_list(monkeypatch):
    index, ex, q = _index(40000, 64, 21, 1.0, 12, 32, 8, "subspace", "sqeuclidean")
    keep = np.random.default_rng(9).random(40000) < 0.5
    gone = int(np.argmax(ex["list_sizes"]))
    keep[np.asarray(ex["ids"][gone])] = False
    gd, gi = _check(monkeypatch, index, ex, q, k=10, n_probes=9, keep=keep)
    found = gi[gi >= 0]
    assert keep[found[found < 40000]].all(), "a rejected row came back"


def test_ticket_form_and_several_head_launches(monkeypatch):
    """CUVS_AMD_PQ_OVERLAP=0: the head kernel's persistent form, as many workgroups per CU as are resident, items by ticket;
    max_internal_batch_size below the batch: several head launches per search."""
    index, ex, q = _index(40000, 64, 21, 1.0, 12, 32, 8, "subspace", "sqeuclidean")
    a = _check(monkeypatch, index, ex, q, k=10, n_probes=9, other={"CUVS_AMD_PQ_OVERLAP": "0"})
    b = _check(monkeypatch, index, ex, q, k=10, n_probes=9, batch=100, other={"CUVS_AMD_PQ_OVERLAP": "0"})
    assert (a[0] == b[0]).all() and (a[1] == b[1]).all()
