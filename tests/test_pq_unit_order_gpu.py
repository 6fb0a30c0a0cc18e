"""GPU: the hand-out order of the matrix-core filter's work units (order_units_kernel: the cheap units last, the XCD shares
strided over the array - pq_filter4_kernel and pq_filter_kernel). The order is scheduling only: every case asserts, after the plan
hook confirmed the matrix-core tail with head1, that ids AND distances of a default handle equal the oracle's on the exported index
and those of handles created under CUVS_AMD_PQ_UNIT_ORDER=0 (list order, contiguous shares), under the other cost order and under
CUVS_AMD_PQ_SCAN3=0 (the LUT scan kernels), and that the filter's counters (CUVS_AMD_SCAN_DEBUG=1024) - pairs screened, survivors,
subtiles, units - are those of list order: every unit is taken exactly once. (The head items keep query order: no
CUVS_AMD_PQ_HEAD_ORDER to compare against.)"""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle
from tests.test_pq_head_occupancy_gpu import _DT, _assert_head_kernel, _handles, _index

pytestmark = pytest.mark.gpu

OTHER_ORDER = "1"   # the candidate that is not the default (CUVS_AMD_PQ_UNIT_ORDER: 1 largest first, 2 list order + cheap tail)


def _stats():
    from cuvs_amd._lib import lib

    st = (C.c_uint64 * 6)()
    lib().cuvsAmdIvfPqLastFilterStats6(st)
    return [int(v) for v in st]


def _counters(monkeypatch, capfd, sp, index, qt, k, **env):
    """(pairs screened, survivors, subtiles, units) of the search's last launch on a handle with the filter's counters on"""
    from cuvs_amd.neighbors import ivf_pq

    _, r = _handles(monkeypatch, CUVS_AMD_SCAN_DEBUG="1024", **env)
    d, i = ivf_pq.search(sp, index, qt, k, resources=r)
    r.sync()
    capfd.readouterr()   # (the counters' stderr lines)
    return _stats()[:4], d, i


def _check(monkeypatch, capfd, index, ex, q, *, metric="sqeuclidean", k=10, n_probes=9, batch=4096):
    import torch
    from cuvs_amd.neighbors import ivf_pq

    _assert_head_kernel(index, ex, metric, "subspace", k, len(q), n_probes, "f16", "f32", batch)
    sp = ivf_pq.SearchParams(n_probes=n_probes, lut_dtype=_DT["f16"], internal_distance_dtype=_DT["f32"], max_internal_batch_size=batch)
    qt = torch.from_numpy(q).cuda()
    r0, _ = _handles(monkeypatch)
    d0, i0 = ivf_pq.search(sp, index, qt, k, resources=r0)
    r0.sync()
    od, oi = oracle.ivf_pq_search(ex, q, k, n_probes, metric=metric, lut="f16", acc="f32")
    gd, gi = d0.cpu().numpy(), i0.cpu().numpy()
    assert (gi == oi).all(), f"ids differ from the oracle's: rate {(gi != oi).mean():.5f}"
    assert (gd == od).all(), "distances differ from the oracle's"
    for env in ({"CUVS_AMD_PQ_UNIT_ORDER": "0"}, {"CUVS_AMD_PQ_UNIT_ORDER": OTHER_ORDER}, {"CUVS_AMD_PQ_SCAN3": "0"}):
        _, r1 = _handles(monkeypatch, **env)
        d1, i1 = ivf_pq.search(sp, index, qt, k, resources=r1)
        r1.sync()
        assert torch.equal(i0, i1) and torch.equal(d0, d1), f"results differ under {env}"
    st_list, _, _ = _counters(monkeypatch, capfd, sp, index, qt, k, CUVS_AMD_PQ_UNIT_ORDER="0")
    st_new, d2, i2 = _counters(monkeypatch, capfd, sp, index, qt, k)
    st_other, _, _ = _counters(monkeypatch, capfd, sp, index, qt, k, CUVS_AMD_PQ_UNIT_ORDER=OTHER_ORDER)
    print(f"counters (pairs screened, survivors, subtiles, units): list order {st_list}, default {st_new}, other {st_other}")
    assert torch.equal(i0, i2) and torch.equal(d0, d2), "results differ with the counters on"
    assert st_list[3] > 0 and st_list[0] > 0 and st_list[2] > 0, "the filter's counters are off"
    assert st_new == st_list and st_other == st_list, "a unit was taken twice or not at all"
    return st_new


def test_two_units_of_different_group_counts_per_list(monkeypatch, capfd):
    """40000 x 64, 12 lists, 300 queries, 9 probes: 2400 tail pairs on 12 lists - lists probed by more than 128 queries have a
    unit of four query groups and one of fewer."""
    index, ex, q = _index(40000, 64, 21, 1.0, 12, 32, 8, "subspace", "sqeuclidean")
    st = _check(monkeypatch, capfd, index, ex, q)
    assert st[3] > 12, "some list has two units"


def test_unit_count_that_is_no_multiple_of_eight(monkeypatch, capfd):
    """the XCD shares differ in length. (A search has a head phase - and with it this tail - from 256 queries on: 300 queries
    give every list two units, 24 in all; with more queries some lists have a third one.) The query count is the first of the
    row whose unit count is no multiple of 8."""
    import torch
    from cuvs_amd.neighbors import ivf_pq

    index, ex, q = _index(40000, 64, 21, 1.0, 12, 32, 8, "subspace", "sqeuclidean")
    more = (np.random.default_rng(77).random((120, 64), dtype=np.float32) * 1.9 + 0.1).astype(np.float32)
    q = np.concatenate([q, more])
    sp = ivf_pq.SearchParams(n_probes=9, lut_dtype=_DT["f16"], internal_distance_dtype=_DT["f32"], max_internal_batch_size=4096)
    for nq in (330, 340, 350, 360, 370, 380, 400, 420):
        st, _, _ = _counters(monkeypatch, capfd, sp, index, torch.from_numpy(q[:nq]).cuda(), 10)
        if st[3] % 8 != 0:
            break
    assert st[3] % 8 != 0, st
    st = _check(monkeypatch, capfd, index, ex, q[:nq])
    assert st[3] % 8 != 0, st


def test_fewer_than_sixteen_units(monkeypatch, capfd):
    """10 lists, 9 probes, launches of 20 queries (a search has this tail phase only from 256 queries on, so: 300 queries at
    max_internal_batch_size 20): at most 10 units per launch - some XCD shares hold one unit, others two or none, the strided
    mapping's edge"""
    index, ex, q = _index(56000, 64, 21, 1.0, 10, 32, 8, "subspace", "sqeuclidean")
    st = _check(monkeypatch, capfd, index, ex, q, batch=20)
    assert 8 < st[3] < 16, st


@functools.lru_cache(maxsize=None)
def _blob_index():
    import torch
    from cuvs_amd.neighbors import ivf_pq

    rng = np.random.default_rng(11)
    dim, n_lists = 64, 12
    sizes = [26203, 403, 7] + [1487] * 8 + [1491]
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
    q = np.concatenate([blob(c, 25) for c in range(n_lists)])   # every list is the nearest of 25 queries
    return index, ivf_pq.export_for_oracle(index), q


def test_unit_costs_three_orders_of_magnitude_apart(monkeypatch, capfd):
    """lists of 26203 / 403 / 7 rows next to ordinary ones: several row chunks per list, a list shorter than a subtile"""
    index, ex, q = _blob_index()
    got = [int(v) for v in ex["list_sizes"]]
    assert max(got) > 3 * 8192 and any(0 < s < 32 for s in got), got
    st = _check(monkeypatch, capfd, index, ex, q)
    assert st[3] >= 12 + 3, "the long list has four row chunks"


@pytest.mark.parametrize("metric", ["inner_product", "cosine"])
def test_inner_product_and_cosine(metric, monkeypatch, capfd):
    """inner product runs pq_filter_kernel (units of up to 64 queries), cosine pq_filter4_kernel without row terms"""
    index, ex, q = _index(30000, 128, 22, 1.0, 12, 64, 8, "subspace", metric)
    _check(monkeypatch, capfd, index, ex, q, metric=metric)


def test_several_launches_per_search(monkeypatch, capfd):
    """max_internal_batch_size below the batch: units, order and tickets are rebuilt for every launch"""
    index, ex, q = _index(40000, 64, 21, 1.0, 12, 32, 8, "subspace", "sqeuclidean")
    _check(monkeypatch, capfd, index, ex, q, batch=100)
