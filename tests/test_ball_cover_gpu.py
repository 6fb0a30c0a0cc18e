"""GPU: cuvsAmdBallCover* (cuvs_amd/csrc/ball_cover.hip) against the numpy twin tests/ball_cover_ref.py. The index
arrays are the twin's bit for bit; the default search equals the twin's brute force under (distance, id), ids and distance
bits, for every landmark count and seed; the approximate modes equal the twin's restatement; eps_nn equals the semantics of
cuvsAmdEpsNeighbors* with the squared radius. The inputs sit on the pruning boundaries: lattices (exact distances, ties,
pairs exactly on a radius), shells a few ulp around one radius, duplicated rows (empty lists, id tie-breaks)."""
import functools

import numpy as np
import pytest
import torch

from tests import ball_cover_ref as R
from tests import eps_neighbors_ref as E

pytestmark = pytest.mark.gpu

F32 = np.float32


def BC():
    from cuvs_amd.neighbors import ball_cover

    return ball_cover


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()  # (a copy: the shared inputs are read-only)


def host(t):
    return t.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def data(name):
    """(X, Q): Q holds rows of X and rows that are not in X; shared between the tests and never written"""
    if name == "lattice2":
        X = R.lattice(2, 50)
        Q = np.concatenate([X[:96], X[:32] + F32(0.5)])
    elif name == "lattice3":
        X = R.lattice(3, 14)
        Q = np.concatenate([X[:96], X[:32] + F32(0.5)])
    elif name == "blobs2":
        X = R.blobs(3000, 2, 1)
        Q = np.concatenate([X[:96], R.blobs(32, 2, 2)])
    elif name == "blobs3":
        X = R.blobs(3000, 3, 3)
        Q = np.concatenate([X[:96], R.blobs(32, 3, 4)])
    elif name == "shell2":
        X, Q = R.shell(3000, 6, 2, 5)
    elif name == "shell3":
        X, Q = R.shell(3000, 6, 3, 6)
    elif name == "duplicated":
        X = R.duplicated(3000, 2, 7)
        Q = np.concatenate([X[:96], R.duplicated(32, 2, 8)])
    else:
        raise KeyError(name)
    X.setflags(write=False)
    Q.setflags(write=False)
    return X, Q


@functools.lru_cache(maxsize=None)
def pairs(name):
    """the twin's distances of every (query, row) pair, computed once"""
    X, Q = data(name)
    d = R.l2(Q, X)
    d.setflags(write=False)
    return d


L2_INPUTS = ["lattice2", "lattice3", "blobs2", "blobs3", "shell2", "shell3", "duplicated"]


def check_knn(got, want, what):
    gd, gi = got
    wi, wd = want
    assert (host(gi) == wi).all(), what
    assert (bits(host(gd)) == bits(wd)).all(), what


# ---------------------------------------------------------------------------------------------- build
@pytest.mark.parametrize("name,rows,n_landmarks,seed", [("lattice2", 2500, 0, 0), ("blobs3", 3000, 0, 1), ("duplicated", 3000, 0, 2),
                                                        ("duplicated", 600, 600, 0), ("shell2", 3000, 1, 0), ("shell3", 65, 7, 3),
                                                        ("blobs2", 1, 0, 0), ("blobs2", 2, 2, 0), ("blobs2", 64, 0, 5)])
def test_build_arrays_equal_twin(name, rows, n_landmarks, seed):
    X = data(name)[0][:rows]
    ix = BC().build(BC().IndexParams(metric="euclidean", n_landmarks=n_landmarks, seed=seed), dev(X))
    tw = R.build(X, "euclidean", n_landmarks, seed)
    assert (ix.n_landmarks, ix.m, ix.dim, ix.metric) == (tw["L"], rows, X.shape[1], 1) and len(ix) == rows
    for key in ("R_rows", "R_indptr", "R_1nn_cols"):
        assert (host(ix.array(key)) == tw[key]).all(), key
    for key in ("R_1nn_dists", "R_radius", "R", "X_reordered"):
        assert (bits(host(ix.array(key))) == bits(tw[key])).all(), key
    assert (host(ix.R_indptr) == tw["R_indptr"]).all() and host(ix.X_reordered).shape == X.shape
    if name == "duplicated" and n_landmarks == 600:
        assert (np.diff(tw["R_indptr"]) == 0).sum() > 10  # copies drawn as two landmarks: empty lists


def test_the_index_owns_its_rows():
    X, Q = data("blobs2")
    x = dev(X)
    ix = BC().build(BC().IndexParams(), x)
    x.fill_(float("nan"))
    del x
    check_knn(BC().knn_query(ix, dev(Q), 5), R.brute(X, Q, 5, d=pairs("blobs2")), "after the caller's rows are gone")


# ---------------------------------------------------------------------------------------------- exact k-NN
@pytest.mark.parametrize("name", L2_INPUTS)
def test_exact_knn_equals_brute_force(name):
    X, Q = data(name)
    m, d = len(X), pairs(name)
    x, q = dev(X), dev(Q)
    default = R.isqrt(m)
    want = {k: R.brute(X, Q, k, d=d) for k in (1, 2, 5, 11, 25, default)}
    for n_landmarks, seed in ((1, 0), (1, 1), (0, 0), (0, 1), (m, 0), (m, 1)):
        ix = BC().build(BC().IndexParams(n_landmarks=n_landmarks, seed=seed), x)
        for k in ((1,) if n_landmarks == 1 else (1, 2, 5, 11, 25, default)):
            check_knn(BC().knn_query(ix, q, k), want[k], (name, n_landmarks, seed, k))
    # rows sorted by (distance, id): the twin's brute force is, and the outputs equal it; ties are present
    wi, wd = want[25]
    assert name not in ("lattice2", "lattice3") or (np.diff(wd, axis=1) == 0).mean() > 0.3


@pytest.mark.parametrize("name", ["lattice2", "blobs3", "duplicated"])
def test_all_knn_query_equals_brute_force(name):
    X = data(name)[0][:1024]
    d = R.l2(X, X)
    for k, seed in ((5, 0), (11, 1)):
        dd, ii, ix = BC().all_knn_query(BC().IndexParams(seed=seed), dev(X), k, return_index=True)
        check_knn((dd, ii), R.brute(X, X, k, d=d), (name, k))
        assert ix.n_landmarks == 32 and ix.m == 1024
        check_knn(BC().knn_query(ix, dev(X[:64]), k), R.brute(X, X[:64], k, d=d[:64]), "the index all_knn_query hands back")
    dd, ii = BC().all_knn_query(BC().IndexParams(), dev(X), 2)  # without the index
    check_knn((dd, ii), R.brute(X, X, 2, d=d), name)
    assert name == "duplicated" or (host(ii)[:, 0] == np.arange(1024)).all()  # the self match is an ordinary candidate


@pytest.mark.parametrize("m", [1, 2, 3, 63, 64, 65])
def test_edge_sizes(m):
    X = data("lattice2")[0][:m]
    Q = np.concatenate([X, X[:1] + F32(0.25)])
    d = R.l2(Q, X)
    for n_landmarks in (0, m, 1):
        ix = BC().build(BC().IndexParams(n_landmarks=n_landmarks, seed=m), dev(X))
        L = ix.n_landmarks
        assert L == (n_landmarks or R.isqrt(m))
        for k in {1, L}:
            check_knn(BC().knn_query(ix, dev(Q), k), R.brute(X, Q, k, d=d), (m, n_landmarks, k))
        for k in {1, L}:  # every mode gives sorted rows; one list per landmark row: never a padded slot
            dd, ii = BC().knn_query(ix, dev(Q), k, perform_post_filtering=False)
            tw = R.knn(R.build(X, "euclidean", n_landmarks, m), Q, k, post_filter=False)
            assert (host(ii) == tw[0]).all() and (bits(host(dd)) == bits(tw[1])).all() and (host(ii) != R.PAD_ID).all()


def test_k_256():
    rng = np.random.default_rng(12)
    X = rng.uniform(-1, 1, size=(65536, 2)).astype(F32)
    Q = np.concatenate([X[:4], rng.uniform(-1, 1, size=(4, 2)).astype(F32)])
    ix = BC().build(BC().IndexParams(), dev(X))
    assert ix.n_landmarks == 256
    d = R.l2(Q, X)
    for k in (256, 129, 65):  # the three sizes of the sorted list
        check_knn(BC().knn_query(ix, dev(Q), k), R.brute(X, Q, k, d=d), k)
    stats = BC().last_stats()
    assert stats["queries"] == 8 and stats["points_scored"] < 8 * 65536 // 2


# ---------------------------------------------------------------------------------------------- approximate modes
@pytest.mark.parametrize("name", ["blobs2", "lattice3", "duplicated"])
def test_approximate_modes_equal_twin(name):
    X, Q = data(name)
    Q = Q[64:]  # 32 rows of X and 32 others
    exact = R.brute(X, Q, 5, d=pairs(name)[64:])
    differs = 0
    for seed in (0, 1):
        ix = BC().build(BC().IndexParams(seed=seed), dev(X))
        tw = R.build(X, "euclidean", 0, seed)
        for k in ((5, 11) if seed == 0 else (5,)):
            for post, weight in ((False, 1.0), (True, 0.5), (True, 0.9), (True, 1.0)):
                dd, ii = BC().knn_query(ix, dev(Q), k, perform_post_filtering=post, weight=weight)
                ti, td, ts = R.knn(tw, Q, k, post, weight)
                assert (host(ii) == ti).all() and (bits(host(dd)) == bits(td)).all(), (name, seed, k, post, weight)
                st = BC().last_stats()
                assert (st["lists_visited"], st["points_scored"], st["points_skipped"]) == (ts["lists_visited"], ts["points_scored"],
                                                                                         ts["points_skipped"])
                if k == 5 and not post:
                    differs += int((ti != exact[0]).sum())
    assert name != "blobs2" or differs > 0  # the first pass alone is approximate: the comparison is not vacuous


def test_pruning_happens():
    X, Q = data("blobs2")
    ix = BC().build(BC().IndexParams(), dev(X))
    BC().knn_query(ix, dev(Q), 5)
    st = BC().last_stats()
    _, _, ts = R.knn(R.build(X, "euclidean", 0, 0), Q, 5)
    print("points scored per query: device", st["points_scored"] / len(Q), "twin", ts["points_scored"] / len(Q), "of", len(X))
    assert ts["points_scored"] < len(Q) * len(X) // 2
    assert st["queries"] == len(Q) and 0 < st["points_scored"] < len(Q) * len(X) // 2


# ---------------------------------------------------------------------------------------------- eps_nn
@functools.lru_cache(maxsize=None)
def eps_data(name):
    """(X, Q, radii, acc): acc the chain of every (query, row) pair"""
    if name == "lattice2":
        X, Q = data(name)
        radii = (5.0, 3.0)
    elif name == "lattice3":
        X, Q = data(name)
        radii = (3.0,)
    elif name == "shell2":
        X, Q = R.shell(3000, 6, 2, 9, radius=0.75)
        radii = (0.75,)
    elif name == "shell16":
        X, Q = R.shell(2000, 6, 16, 10, radius=0.75)
        radii = (0.75,)
    elif name == "int16":
        X = E.int_kat(3, 2000, 16)
        Q, radii = X[:100], (3.0, 5.0)
    elif name == "int32":
        X = E.int_kat(4, 2000, 32)
        Q, radii = X[:100], (5.0,)
    elif name == "dim1":
        X = np.arange(300, dtype=F32)[np.random.default_rng(1).permutation(300)][:, None] * F32(0.25)
        Q, radii = X[:40], (0.75, 3.0)
    else:
        raise KeyError(name)
    acc = E.chain(Q, X)
    acc.setflags(write=False)
    return X, Q, radii, acc


@pytest.mark.parametrize("name", ["lattice2", "lattice3", "shell2", "shell16", "int16", "int32", "dim1"])
def test_eps_nn_equals_brute_force_semantics(name):
    X, Q, radii, acc = eps_data(name)
    nq, m = len(Q), len(X)
    q = dev(Q)
    for n_landmarks, seed in ((0, 0), (0, 1), (1, 0)):
        ix = BC().build(BC().IndexParams(n_landmarks=n_landmarks, seed=seed), dev(X))
        for eps in radii:
            want = E.member(acc, F32(eps) * F32(eps))
            vd = E.degrees(want)
            on = int((acc == F32(eps) * F32(eps)).sum())
            assert name in ("shell2", "shell16") or on > 50  # pairs exactly on the radius
            what = (name, n_landmarks, seed, eps)
            # dense, into garbage
            adj = torch.full((nq, m), 0xFF, dtype=torch.uint8, device="cuda")
            v64 = torch.full((nq + 1,), -123456789, dtype=torch.int64, device="cuda")
            BC().eps_nn(ix, q, eps, adj=adj, vd=v64)
            assert (host(adj) == want.astype(np.uint8)).all() and (host(v64) == vd).all(), what
            if seed == 0:
                v32 = torch.full((nq + 1,), -12345, dtype=torch.int32, device="cuda")
                a2, none = BC().eps_nn(ix, q, eps, vd=False)
                assert none is None and a2.dtype == torch.bool and (host(a2) == want).all()
                none, v = BC().eps_nn(ix, q, eps, adj=False, vd=v32)
                assert none is None and (host(v32) == vd).all()
            # CSR, two calls
            wp, wi, wdist = E.csr_of(want, acc)
            indptr = torch.full((nq + 1,), -5, dtype=torch.int64, device="cuda")
            v64.fill_(-7)
            BC().csr_count(ix, q, eps, indptr=indptr, vd=v64)
            assert (host(indptr) == wp).all() and (host(v64) == vd).all(), what
            indices = torch.full((int(wp[-1]) + 3,), -9, dtype=torch.int64, device="cuda")
            dist = torch.full((int(wp[-1]) + 3,), -1.0, dtype=torch.float32, device="cuda")
            BC().csr_fill(ix, q, eps, indptr, indices, dist)
            assert (host(indices)[:-3] == wi).all() and (host(indices)[-3:] == -9).all(), what
            assert (bits(host(dist)[:-3]) == bits(wdist)).all() and (host(dist)[-3:] == -1.0).all(), what
            indices.fill_(-9)
            BC().csr_fill(ix, q, eps, indptr, indices)  # without distances
            assert (host(indices)[:-3] == wi).all()
            # CSR, one call with max_k
            for max_k in (3, int(vd[:-1].max()) + 2):
                kp, ki, kd = E.csr_of(want, acc, max_k=max_k)
                indptr.fill_(-5)
                indices = torch.full((nq * max_k,), -9, dtype=torch.int64, device="cuda")
                dist = torch.full((nq * max_k,), -1.0, dtype=torch.float32, device="cuda")
                v64.fill_(-7)
                found = BC().csr_fill(ix, q, eps, indptr, indices, dist, vd=v64, max_k=max_k)
                assert found == int(vd[:-1].max()) and (host(indptr) == kp).all() and (host(v64) == vd).all(), what
                nnz = int(kp[-1])
                assert (host(indices)[:nnz] == ki).all() and (host(indices)[nnz:] == -9).all(), what
                assert (bits(host(dist)[:nnz]) == bits(kd)).all(), what
    # the convenience form
    ix = BC().build(BC().IndexParams(), dev(X))
    want = E.member(acc, F32(radii[0]) * F32(radii[0]))
    wp, wi, wdist = E.csr_of(want, acc)
    p, i, dd = BC().eps_nn_csr(ix, q, radii[0], return_distances=True)
    assert (host(p) == wp).all() and (host(i) == wi).all() and (bits(host(dd)) == bits(wdist)).all()
    st = BC().last_stats()
    assert st["queries"] == nq and st["points_scored"] + st["points_skipped"] <= nq * m


def test_eps_nn_equals_the_brute_force_entry_point():
    from cuvs_amd.neighbors import epsilon_neighborhood as EN

    X, Q, radii, _ = eps_data("shell16")
    ix = BC().build(BC().IndexParams(), dev(X))
    a, v = BC().eps_nn(ix, dev(Q), 0.75)
    b, w = EN.compute(dev(Q), dev(X), 0.75 * 0.75)
    assert torch.equal(a, b) and torch.equal(v, w)
    p, i, d = BC().eps_nn_csr(ix, dev(Q), 0.75, return_distances=True)
    p2, i2, d2 = EN.csr(dev(Q), dev(X), 0.75 * 0.75, return_distances=True)
    assert torch.equal(p, p2) and torch.equal(i, i2) and torch.equal(d.view(torch.int32), d2.view(torch.int32))
    assert BC().last_stats()["points_scored"] < len(Q) * len(X) // 2


# ---------------------------------------------------------------------------------------------- haversine
def test_haversine():
    X = R.geo(3000, 3)
    Q = np.concatenate([X[:100], R.geo(28, 4)])
    x, q = dev(X), dev(Q)
    d64 = R.haversine(Q, X, np.float64)
    d32 = R.haversine(Q, X).astype(np.float64)
    pos = d64 > 0
    assert (d32[~pos] == 0).all()
    e_cpu = float(np.max(np.abs(d32 - d64)[pos] / d64[pos]))
    out = {}
    for n_landmarks in (1, 0, 3000):
        ix = BC().build(BC().IndexParams(metric="haversine", n_landmarks=n_landmarks, seed=1), x)
        assert ix.metric == 13
        for k in ((1,) if n_landmarks == 1 else (1, 5, 25)):
            dd, ii = BC().knn_query(ix, q, k)
            out[(n_landmarks, k)] = (host(dd), host(ii))
        if n_landmarks == 0:
            st = BC().last_stats()
            assert st["points_scored"] < len(Q) * len(X) // 2
    # (a) the landmarks do not matter, bit for bit
    for k in (1, 5, 25):
        assert (out[(0, k)][1] == out[(3000, k)][1]).all() and (bits(out[(0, k)][0]) == bits(out[(3000, k)][0])).all()
    assert (out[(1, 1)][1] == out[(0, 1)][1]).all() and (bits(out[(1, 1)][0]) == bits(out[(0, 1)][0])).all()
    # (b) the distances against fp64, (c) nothing nearer was left out
    dd, ii = out[(0, 25)]
    ref = np.take_along_axis(d64, ii, axis=1)
    zero = ref == 0
    assert (dd[zero] == 0).all()
    e_dev = float(np.max(np.abs(dd.astype(np.float64) - ref)[~zero] / ref[~zero]))
    print("haversine: e_cpu", e_cpu, "device deviation", e_dev)
    assert e_dev <= 4 * e_cpu
    assert (np.diff(dd.astype(np.float64), axis=1) >= 0).all()
    kth = ref.max(axis=1)
    left_out = np.ones_like(d64, bool)
    np.put_along_axis(left_out, ii, False, axis=1)
    assert (np.where(left_out, d64, np.inf).min(axis=1) >= kth - 4 * e_cpu * kth).all()
    assert ((ii >= 0) & (ii < 3000)).all() and all(len(set(r)) == 25 for r in ii.tolist())


def test_haversine_landmarks_do_not_matter_on_the_globe():
    """(a) on a second input: rows all over the globe, so the balls are wide and up to half a turn from a query, where the
    formula is least accurate; antipodal and seam queries. Two seeds per landmark count."""
    X, Q = R.globe(2000, 96, 9)
    x, q = dev(X), dev(Q)
    d64 = R.haversine(Q, X, np.float64)
    out = {}
    for n_landmarks, seed in ((1, 0), (0, 0), (0, 1), (2000, 0), (2000, 1)):
        ix = BC().build(BC().IndexParams(metric="haversine", n_landmarks=n_landmarks, seed=seed), x)
        for k in ((1,) if n_landmarks == 1 else (1, 5, 25)):
            dd, ii = BC().knn_query(ix, q, k)
            out[(n_landmarks, seed, k)] = (host(dd), host(ii))
    for k in (1, 5, 25):
        first = out[(0, 0, k)]
        for key in ((0, 1, k), (2000, 0, k), (2000, 1, k)) + (((1, 0, 1),) if k == 1 else ()):
            assert (out[key][1] == first[1]).all() and (bits(out[key][0]) == bits(first[0])).all(), key
    # the seam and antipodal queries found their nearest row: by fp64 it is the one returned, up to the formula's fp32 error at
    # these small distances (2^-11 relative + 2^-20 absolute, the bound test_haversine_twin_against_fp64 holds the formula to)
    dd, ii = out[(0, 0, 1)]
    assert (np.take_along_axis(d64, ii, axis=1)[:, 0] <= d64.min(axis=1) * (1 + 2.0 ** -11) + 2.0 ** -20).all()


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_library_usable():
    from cuvs_amd._lib import CuvsError

    X, Q = data("blobs2")
    x, q = dev(X), dev(Q)
    ix = BC().build(BC().IndexParams(), x)

    def refused(fn, *parts):
        with pytest.raises(CuvsError) as e:
            fn()
        text = str(e.value)
        assert text and all(p in text for p in parts), text

    refused(lambda: BC().build(BC().IndexParams(metric="sqeuclidean"), x), "not supported")
    refused(lambda: BC().build(BC().IndexParams(metric="l2_unexpanded"), x), "not supported")
    x4 = dev(np.random.default_rng(0).random((500, 4)).astype(F32))
    ix4 = BC().build(BC().IndexParams(), x4)  # (eps_nn takes it)
    refused(lambda: BC().knn_query(ix4, x4, 2), "dim 2 or 3")
    refused(lambda: BC().all_knn_query(BC().IndexParams(), x4, 2), "dim 2 or 3")
    refused(lambda: BC().build(BC().IndexParams(metric="haversine"), dev(np.zeros((10, 3), F32))), "Haversine needs dim == 2")
    refused(lambda: BC().knn_query(ix, q, ix.n_landmarks + 1), "must not exceed n_landmarks")
    refused(lambda: BC().knn_query(ix, q, 257), "k must be in [1, 256]")
    hav = BC().build(BC().IndexParams(metric="haversine"), dev(R.geo(500, 1)))
    refused(lambda: BC().eps_nn(hav, dev(R.geo(5, 2)), 0.1), "eps_nn needs an L2 index")
    refused(lambda: BC().eps_nn_csr(hav, dev(R.geo(5, 2)), 0.1), "eps_nn needs an L2 index")
    refused(lambda: BC().build(BC().IndexParams(), x.half()), "fp32")
    refused(lambda: BC().knn_query(ix, q.half(), 2), "fp32")
    refused(lambda: BC().build(BC().IndexParams(), torch.from_numpy(np.array(X))), "device")
    refused(lambda: BC().knn_query(ix, torch.from_numpy(np.array(Q)), 2, neighbors=torch.empty((len(Q), 2), dtype=torch.int64, device="cuda"),
                                   distances=torch.empty((len(Q), 2), dtype=torch.float32, device="cuda")), "device")
    refused(lambda: BC().build(BC().IndexParams(n_landmarks=3001), x), "n_landmarks")
    refused(lambda: BC().eps_nn(ix, q, -1.0), "eps")
    refused(lambda: BC().knn_query(_unbuilt(), q, 2), "not been built")
    # the process is still usable
    check_knn(BC().knn_query(ix, q, 5), R.brute(X, Q, 5, d=pairs("blobs2")), "after the refusals")


def _unbuilt():
    ix = BC().Index()
    ix.trained = True
    return ix
