"""GPU: cuvsAmdEpsNeighbors* (cuvs_amd/csrc/eps_neighbors.hip) against the numpy twin tests/eps_neighbors_ref.py, bit for bit:
the inputs put thousands of pairs within a few ulp of the radius, so any arithmetic other than the contract's chain flips
membership."""
import json
import os

import numpy as np
import pytest
import torch

from tests import eps_neighbors_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = json.load(open(os.path.join(ROOT, "tests", "golden", "eps_neighbors_reference_table.json")))

SPHERES = [(64, 4096, 3), (64, 4096, 16), (64, 4096, 67), (64, 4096, 128), (1, 1, 1), (129, 257, 17), (130, 127, 18), (257, 300, 67)]
ids = lambda c: "x".join(map(str, c))  # noqa: E731


def E():
    from cuvs_amd.neighbors import epsilon_neighborhood

    return epsilon_neighborhood


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()  # (a copy: the shared inputs are read-only)


def garbage(m, dtype):
    return torch.full((m + 1,), -123456789, dtype=dtype, device="cuda")


def dense(x, y, eps, res, vd_dtype=torch.int64, adj=True, vd=True):
    """compute() into pre-filled buffers -> (adj bytes or None, vd or None) on the host"""
    a = torch.full((x.shape[0], y.shape[0]), 0xFF, dtype=torch.uint8, device="cuda") if adj else False
    v = garbage(x.shape[0], vd_dtype) if vd else False
    a, v = E().compute(x, y, float(eps), adj=a, vd=v, resources=res)
    res.sync()
    return (a.cpu().numpy() if adj else None), (v.cpu().numpy() if vd else None)


def two_calls(x, y, eps, res, distances=True, vd=True):
    m = x.shape[0]
    indptr = garbage(m, torch.int64)
    v = garbage(m, torch.int64) if vd else None
    E().csr_count(x, y, float(eps), indptr=indptr, vd=v, resources=res)
    res.sync()
    nnz = int(indptr[m].item())
    indices = torch.full((nnz,), -1, dtype=torch.int64, device="cuda")  # exactly nnz
    dist = torch.full((nnz,), -1.0, dtype=torch.float32, device="cuda") if distances else None
    E().csr_fill(x, y, float(eps), indptr, indices, dist, resources=res)
    res.sync()
    return indptr.cpu().numpy(), indices.cpu().numpy(), (dist.cpu().numpy() if distances else None), (v.cpu().numpy() if vd else None)


# ---------------------------------------------------------------------------------------------- 1: membership
@pytest.mark.parametrize("case", SPHERES, ids=ids)
def test_membership_bit_for_bit(res, case):
    m, n, dim = case
    x, y, eps, acc, want = R.spheres_twin(m, n, dim, dim)
    vd_want = R.degrees(want)
    if n >= 4096:
        assert 2000 < vd_want[-1] < 20000
    dx, dy = dev(x), dev(y)
    for vd_dtype in (torch.int64, torch.int32):
        adj, vd = dense(dx, dy, eps, res, vd_dtype)
        print(case, vd_dtype, "pairs that differ:", int((adj != want).sum()), "edges:", int(vd[-1]), "want", int(vd_want[-1]))
        assert set(np.unique(adj)) <= {0, 1}
        assert (adj == want.astype(np.uint8)).all()
        assert (vd == vd_want).all() and vd[m] == want.sum()
    adj, vd = dense(dx, dy, eps, res, adj=False)
    assert adj is None and (vd == vd_want).all()
    adj, vd = dense(dx, dy, eps, res, vd=False)
    assert vd is None and (adj == want.astype(np.uint8)).all()
    # a bool adjacency matrix, allocated by the call
    a, v = E().compute(dx, dy, float(eps), vd_dtype=torch.int32, resources=res)
    res.sync()
    assert a.dtype == torch.bool and v.dtype == torch.int32 and (a.cpu().numpy() == want).all() and (v.cpu().numpy() == vd_want).all()


# ---------------------------------------------------------------------------------------------- 2: integers
def test_integers_on_the_radius_count_as_inside(res):
    kat = R.int_kat(1)
    acc = R.chain(kat, kat)
    want = R.member(acc, 6.0)
    assert int((acc == 6).sum()) == 884 and int(want.sum()) == 2936
    d = dev(kat)
    adj, vd = dense(d, d, 6.0, res)
    assert (adj == want).all() and (vd == R.degrees(want)).all()
    adj, vd = dense(d, d, -1.0, res)
    assert not adj.any() and not vd.any()
    empty = d[:, :0].contiguous()  # dim == 0
    for eps in (0.0, 2.5):
        adj, vd = dense(empty, empty, eps, res)
        assert (adj == 1).all() and (vd[:-1] == 130).all() and vd[-1] == 130 * 130
    adj, vd = dense(empty, empty, -0.5, res)
    assert not adj.any() and not vd.any()
    # NaN compares false
    nan = kat.copy()
    nan[3, 2] = np.nan
    adj, vd = dense(dev(nan), d, 1e30, res)
    assert vd[3] == 0 and not adj[3].any() and (np.delete(vd[:-1], 3) == 130).all()
    # no rows on one side or the other
    adj, vd = dense(d[:0], d, 6.0, res)
    assert adj.shape == (0, 130) and (vd == [0]).all()
    adj, vd = dense(d, d[:0], 6.0, res)
    assert adj.shape == (130, 0) and (vd == 0).all() and len(vd) == 131


# ---------------------------------------------------------------------------------------------- 3: CSR, two calls
@pytest.mark.parametrize("case", [(64, 4096, 67), (64, 4096, 16), (1, 1, 1), (129, 257, 17), (257, 300, 67)], ids=ids)
def test_csr_two_calls(res, case):
    m, n, dim = case
    x, y, eps, acc, want = R.spheres_twin(m, n, dim, dim)
    indptr_w, indices_w, dist_w = R.csr_of(want, acc)
    indptr, indices, dist, vd = two_calls(dev(x), dev(y), eps, res)
    assert (indptr == indptr_w).all()
    assert (indices == indices_w).all()  # ascending within a row, not merely the same set
    assert (dist.view(np.uint32) == dist_w.view(np.uint32)).all()
    assert (vd == R.degrees(want)).all()
    # the wrapper that makes both calls
    out = E().csr(dev(x), dev(y), float(eps), return_distances=True, resources=res)
    assert len(out) == 3 and all((o.cpu().numpy() == w).all() for o, w in zip(out, (indptr_w, indices_w, dist_w)))
    out = E().csr(dev(x), dev(y), float(eps))
    assert len(out) == 2 and (out[1].cpu().numpy() == indices_w).all()


def test_csr_without_rows(res):
    kat = dev(R.int_kat(1))
    indptr, indices, dist, vd = two_calls(kat[:0], kat, 6.0, res)
    assert (indptr == [0]).all() and (vd == [0]).all() and len(indices) == 0
    indptr, indices, dist, vd = two_calls(kat, kat[:0], 6.0, res)
    assert (indptr == 0).all() and len(indptr) == 131 and (vd == 0).all()


# ---------------------------------------------------------------------------------------------- 4: max_k
def test_max_k_keeps_the_first_ids(res):
    x, y, eps, acc, want = R.spheres_twin(64, 4096, 16, 16)
    deg = R.degrees(want)[:-1]
    largest = int(deg.max())
    below_median = int(np.median(deg)) // 2
    assert 1 < below_median < np.median(deg) < largest
    dx, dy = dev(x), dev(y)
    for cap in (below_median, largest, 1):
        indptr_w, indices_w, dist_w = R.csr_of(want, acc, max_k=cap)
        m = x.shape[0]
        indptr, vd = garbage(m, torch.int64), garbage(m, torch.int64)
        indices = torch.full((m * cap,), -1, dtype=torch.int64, device="cuda")
        dist = torch.full((m * cap,), -1.0, dtype=torch.float32, device="cuda")
        found = E().csr_fill(dx, dy, float(eps), indptr, indices, dist, vd=vd, max_k=cap, resources=res)
        res.sync()
        nnz = int(indptr_w[-1])
        assert (indptr.cpu().numpy() == indptr_w).all()
        assert (indices.cpu().numpy()[:nnz] == indices_w).all()  # the first max_k in ascending order
        assert (indices.cpu().numpy()[nnz:] == -1).all()
        assert (dist.cpu().numpy()[:nnz].view(np.uint32) == dist_w.view(np.uint32)).all()
        assert (vd.cpu().numpy() == R.degrees(want)).all()  # the full degrees
        assert found == largest
        out = E().csr(dx, dy, float(eps), max_k=cap, return_distances=True)
        assert len(out) == 4 and out[3] == largest and (out[1].cpu().numpy() == indices_w).all()
        assert (out[2].cpu().numpy().view(np.uint32) == dist_w.view(np.uint32)).all()
    out = E().csr(dx, dy, float(eps), max_k=0)
    assert (out[0].cpu().numpy() == 0).all() and len(out[1]) == 0 and out[2] == largest


# ---------------------------------------------------------------------------------------------- 5: slabs
def test_row_slabs(res, monkeypatch):
    import cuvs_amd

    m, n, dim = 257, 300, 67
    x, y, eps, acc, want = R.spheres_twin(m, n, dim, dim)
    dx, dy = dev(x), dev(y)
    plain_dense = dense(dx, dy, eps, res)
    assert E().last_stats()["slabs"] == 1 and E().last_stats()["tiles"] == 9 and E().last_stats()["edges"] == want.sum()
    plain_csr = two_calls(dx, dy, eps, res)
    assert E().last_stats()["slabs"] == 1
    monkeypatch.setenv("CUVS_AMD_EPS_SLAB_ROWS", "100")
    forced = cuvs_amd.common.Resources()
    slab_dense = dense(dx, dy, eps, forced)
    st = E().last_stats()
    assert st["slabs"] == 3 and st["tiles"] == 9 and st["edges"] == want.sum() and st["resolved_exactly"] == 0
    slab_csr = two_calls(dx, dy, eps, forced)
    assert E().last_stats()["slabs"] == 3 and E().last_stats()["edges"] == want.sum()
    for a, b in zip(plain_dense + plain_csr, slab_dense + slab_csr):
        assert a.dtype == b.dtype and (a.view(np.uint8) == b.view(np.uint8)).all()
    assert (slab_dense[0] == want).all() and (slab_csr[1] == R.csr_of(want)[1]).all()
    # the one-call form carries its offsets over the slab borders
    cap = 5
    indptr = garbage(m, torch.int64)
    indices = torch.full((m * cap,), -1, dtype=torch.int64, device="cuda")
    found = E().csr_fill(dx, dy, float(eps), indptr, indices, max_k=cap, resources=forced)
    forced.sync()
    indptr_w, indices_w = R.csr_of(want, max_k=cap)
    assert (indptr.cpu().numpy() == indptr_w).all() and (indices.cpu().numpy()[:indptr_w[-1]] == indices_w).all()
    assert found == R.degrees(want)[:-1].max() and E().last_stats()["slabs"] == 3


# ---------------------------------------------------------------------------------------------- 6: aliasing, fp16
def test_x_is_y_and_row_slices(res):
    for n, dim in ((300, 18), (300, 16), (130, 20)):
        _, y, eps, _, _ = R.spheres_twin(64, n, dim, dim)
        want = R.member(R.chain(y, y), eps)
        dy = dev(y)
        adj, vd = dense(dy, dy, eps, res)
        assert (adj == want).all() and (vd == R.degrees(want)).all() and adj.diagonal().all()
        batch = n // 3
        for b in range(3):  # the reference's batches: x is a row slice of y
            dx = dy[b * batch:(b + 1) * batch]
            assert dx.data_ptr() == dy.data_ptr() + b * batch * dim * 4
            adj, vd = dense(dx, dy, eps, res)
            assert (adj == want[b * batch:(b + 1) * batch]).all()
            indptr, indices, dist, _ = two_calls(dx, dy, eps, res)
            assert (indices == R.csr_of(want[b * batch:(b + 1) * batch])[1]).all()


@pytest.mark.parametrize("case", [(64, 4096, 16), (129, 257, 17), (70, 130, 24)], ids=ids)
def test_fp16_rows(res, case):
    m, n, dim = case
    x, y, _ = R.spheres(m, n, dim, dim)
    x16, y16 = x.astype(np.float16), y.astype(np.float16)
    acc = R.chain(x16, y16)  # on the widened values
    eps = np.float32(np.median(acc[np.arange(n) % m, np.arange(n)]))
    want = R.member(acc, eps)
    assert 0 < want.sum() < want.size
    adj, vd = dense(dev(x16), dev(y16), eps, res)
    assert (adj == want).all() and (vd == R.degrees(want)).all()
    indptr, indices, dist, _ = two_calls(dev(x16), dev(y16), eps, res)
    indptr_w, indices_w, dist_w = R.csr_of(want, acc)
    assert (indptr == indptr_w).all() and (indices == indices_w).all() and (dist.view(np.uint32) == dist_w.view(np.uint32)).all()


# ---------------------------------------------------------------------------------------------- 7: the reference's table
RUN = [r for r in TABLE["inputsfi_rbc"]["rows"] + TABLE["inputsfi"]["rows"] if r["run"]]


@pytest.mark.parametrize("row", RUN, ids=lambda r: "line%d" % r["line"])
def test_reference_table(res, row):
    n_row, n_col, batches = row["n_row"], row["n_col"], row["n_batches"]
    rows, _, _ = R.blobs(n_row, n_col, row["n_centers"], 1000 * n_row + n_col)
    data = dev(rows)
    batch = n_row // batches
    eps = float(np.float32(row["eps"]) * np.float32(row["eps"]))
    for b in range(batches):
        x = data[b * batch:(b + 1) * batch]
        adj, vd = E().compute(x, data, eps, resources=res)
        res.sync()
        assert (vd[:batch] == n_row // row["n_centers"]).all()  # epsilon_neighborhood.cu:123-124
        assert int(vd[batch]) == batch * (n_row // row["n_centers"])
        indptr, indices = E().csr(x, data, eps, resources=res)
        res.sync()
        assert torch.equal(indptr, torch.arange(batch + 1, device="cuda") * (n_row // row["n_centers"]))
        assert torch.equal(indices, adj.nonzero()[:, 1])  # dense == CSR, row by row in ascending order


# ---------------------------------------------------------------------------------------------- 8: refusals
def test_refusals(res):
    from cuvs_amd._lib import CuvsError

    e = E()
    x = torch.rand(10, 6, device="cuda")
    y = torch.rand(20, 6, device="cuda")
    for metric in ("sqeuclidean", "l2_sqrt_unexpanded", "inner_product", "cosine"):
        with pytest.raises(CuvsError, match="Currently only L2Unexpanded distance metric is supported. Other metrics will be supported"):
            e.compute(x, y, 1.0, metric=metric, resources=res)
        with pytest.raises(CuvsError, match="Currently only L2Unexpanded distance metric is supported"):
            e.csr_count(x, y, 1.0, metric=metric, resources=res)
    with pytest.raises(CuvsError, match="fp64 rows are not supported"):
        e.compute(x.double(), y.double(), 1.0, resources=res)
    with pytest.raises(CuvsError, match="same dtype"):
        e.compute(x, y.half(), 1.0, resources=res)
    with pytest.raises(CuvsError, match="fp32 or fp16"):
        e.compute(x.to(torch.int8), y.to(torch.int8), 1.0, resources=res)
    with pytest.raises(CuvsError, match="dim mismatch: x has 6 columns, y has 5"):
        e.compute(x, y[:, :5].contiguous(), 1.0, resources=res)
    with pytest.raises(CuvsError, match="x must be row-major and contiguous"):
        e.compute(torch.rand(6, 10, device="cuda").t(), y, 1.0, resources=res)
    with pytest.raises(CuvsError, match="y must be row-major and contiguous"):
        e.csr_count(x, torch.rand(20, 12, device="cuda")[:, ::2], 1.0, resources=res)
    with pytest.raises(CuvsError, match="x must be accessible on device memory"):
        e.compute(x.cpu(), y, 1.0, resources=res)
    with pytest.raises(CuvsError, match="y must be accessible on device memory"):
        e.compute(x, y.cpu(), 1.0, resources=res)
    with pytest.raises(CuvsError, match=r"adj must have shape \[10, 20\]"):
        e.compute(x, y, 1.0, adj=torch.zeros(20, 10, dtype=torch.bool, device="cuda"), resources=res)
    with pytest.raises(CuvsError, match="adj must be bool or uint8"):
        e.compute(x, y, 1.0, adj=torch.zeros(10, 20, dtype=torch.int32, device="cuda"), resources=res)
    with pytest.raises(CuvsError, match="adj must be accessible on device memory"):
        e.compute(x, y, 1.0, adj=torch.zeros(10, 20, dtype=torch.uint8), resources=res)
    with pytest.raises(CuvsError, match=r"vd must have shape \[11\]"):
        e.compute(x, y, 1.0, vd=torch.zeros(10, dtype=torch.int64, device="cuda"), resources=res)
    with pytest.raises(CuvsError, match="vd must be int32 or int64"):
        e.compute(x, y, 1.0, vd=torch.zeros(11, dtype=torch.float32, device="cuda"), resources=res)
    with pytest.raises(CuvsError, match=r"indptr must have shape \[11\]"):
        e.csr_count(x, y, 1.0, indptr=torch.zeros(12, dtype=torch.int64, device="cuda"), resources=res)
    with pytest.raises(CuvsError, match="indptr must be int64"):
        e.csr_count(x, y, 1.0, indptr=torch.zeros(11, dtype=torch.int32, device="cuda"), resources=res)
    with pytest.raises(CuvsError, match="vd must be int64"):
        e.csr_count(x, y, 1.0, vd=torch.zeros(11, dtype=torch.int32, device="cuda"), resources=res)
    # int32 degrees could overflow from m * n = 2^31 on (nothing is computed: the call is refused)
    bx, by = torch.zeros(32768, 1, device="cuda"), torch.zeros(65536, 1, device="cuda")
    with pytest.raises(CuvsError, match=r"vd must be int64 when m \* n >= 2\^31"):
        e.compute(bx, by, 1.0, adj=False, vd=torch.zeros(32769, dtype=torch.int32, device="cuda"), resources=res)
    # a fill into a buffer one short of indptr[m]
    indptr = e.csr_count(x, y, 100.0, resources=res)
    res.sync()
    assert int(indptr[10]) == 200
    with pytest.raises(CuvsError, match=r"indices holds 199 entries but indptr\[m\] is 200"):
        e.csr_fill(x, y, 100.0, indptr, torch.zeros(199, dtype=torch.int64, device="cuda"), resources=res)
    with pytest.raises(CuvsError, match="distances holds 199 entries"):
        e.csr_fill(x, y, 100.0, indptr, torch.zeros(200, dtype=torch.int64, device="cuda"),
                   torch.zeros(199, dtype=torch.float32, device="cuda"), resources=res)
    with pytest.raises(CuvsError, match="indices must be int64"):
        e.csr_fill(x, y, 100.0, indptr, torch.zeros(200, dtype=torch.int32, device="cuda"), resources=res)
    with pytest.raises(CuvsError, match=r"indices holds 19 entries but m \* max_k is 20"):
        e.csr_fill(x, y, 100.0, indptr, torch.zeros(19, dtype=torch.int64, device="cuda"), max_k=2, resources=res)
    # a fill whose indptr has less room than the row's degree writes only what the row's range holds
    small = torch.arange(11, dtype=torch.int64, device="cuda") * 3
    indices = torch.full((31,), -1, dtype=torch.int64, device="cuda")
    e.csr_fill(x, y, 100.0, small, indices, resources=res)
    res.sync()
    assert (indices.cpu().numpy() == np.concatenate([np.tile(np.arange(3), 10), [-1]])).all()


# ---------------------------------------------------------------------------------------------- 9: determinism
def test_the_same_call_twice_gives_identical_bytes(res):
    x, y, eps, acc, want = R.spheres_twin(129, 257, 17, 17)
    dx, dy = dev(x), dev(y)
    first = dense(dx, dy, eps, res) + dense(dx, dy, eps, res, torch.int32) + two_calls(dx, dy, eps, res)
    second = dense(dx, dy, eps, res) + dense(dx, dy, eps, res, torch.int32) + two_calls(dx, dy, eps, res)
    for a, b in zip(first, second):
        assert a.tobytes() == b.tobytes()


# ---------------------------------------------------------------------------------------------- offsets past 2^31
def test_adjacency_offsets_past_2_31(res):
    m, n = 33000, 66001  # m * n > 2^31 bytes of adjacency, rows that are not 16-byte aligned
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.rand(m, 1, device="cuda", generator=g)
    y = torch.rand(n, 1, device="cuda", generator=g)
    eps = float(np.float32(0.01))
    adj, vd = E().compute(x, y, eps, resources=res)
    res.sync()
    total = 0
    for r0 in range(0, m, 3000):  # dim 1: the chain is the rounded square of one fp32 difference
        d = x[r0:r0 + 3000] - y.t()
        want = d * d <= torch.tensor(eps, dtype=torch.float32, device="cuda")
        assert torch.equal(adj[r0:r0 + 3000], want)
        assert torch.equal(vd[r0:r0 + 3000], want.sum(dim=1))
        total += int(want.sum())
    assert int(vd[m]) == total > 2 ** 27
