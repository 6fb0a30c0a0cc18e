"""GPU: spectral embedding and clustering (include/cuvs_amd/spectral.h) against the numpy twin
(tests/spectral_ref.py) and float64 references: the connectivity graph bit for bit, the solver's own matrix-vector product and
re-orthogonalisation through their hooks, the solver on graphs with known spectra, determinism, the transform and the
clustering end to end, and the refusals. tests/test_spectral_cpu.py asserts the conditions of the inputs (neighbour margins,
spectral gaps, connected components), so a failure here is never the input's fault."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import spectral_ref as R

pytestmark = pytest.mark.gpu

U = R.U32


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def dev_graph(g):
    r, c, v, n = g
    return dev(r.astype(np.int32)), dev(c.astype(np.int32)), dev(v.astype(np.float32)), n


def se():
    from cuvs_amd.preprocessing import spectral_embedding

    return spectral_embedding


# ---------------------------------------------------------------- 1. connectivity graph
@pytest.mark.parametrize("n,dim,k", R.KNN_SHAPES)
def test_connectivity_graph_bit_for_bit(res, n, dim, k):
    x, ids, margin, (rows, cols, vals, _) = R.knn_graph_case(n, dim, k)
    r, c, v = se().create_connectivity_graph(se().Params(n_neighbors=k), dev(x), resources=res)
    r, c, v = r.cpu().numpy(), c.cpu().numpy(), v.cpu().numpy()
    assert len(r) == len(rows) and len(r) <= 2 * n * k
    assert (r == rows).all() and (c == cols).all() and (v == vals).all()
    keys = (r.astype(np.int64) << 32) | c
    assert (np.diff(keys) > 0).all() and set(np.unique(v)) <= {0.5, 1.0}
    w = np.zeros((n, n), np.float32)
    w[r, c] = v
    assert (w == w.T).all()


# ---------------------------------------------------------------- 2. the matrix-vector product
def matvec_graphs():
    out = {"knn%d" % n: R.knn_graph_case(n, dim, k)[3] for n, dim, k in R.KNN_SHAPES}
    out["hub257"] = R.hub(257)
    out["messy41"] = R.messy(41)
    out["complete70"] = R.complete(70)  # 69 entries per row: a whole wave per row
    z = np.zeros(0, np.int32)
    out["n1"] = (z, z, np.zeros(0, np.float32), 1)
    out["n2"] = R.path(2)
    for n in (63, 64, 65):
        out["ring%d" % n] = R.ring(n)
    return out


@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("name", ["knn33", "knn257", "knn1000", "hub257", "messy41", "complete70", "n1", "n2", "ring63", "ring64", "ring65"])
def test_matvec_hook_against_float64(res, name, norm):
    r, c, v, n = matvec_graphs()[name]
    lap, _ = R.laplacian(r, c, v, n, norm)
    op = R.Operator(r, c, v, n, norm)
    x = R.start_vector(11, n)
    dr, dc, dv, _ = dev_graph((r, c, v, n))
    y, diag = se().laplacian_matvec(dr, dc, dv, n, dev(x), norm_laplacian=norm, resources=res)
    y, diag = y.cpu().numpy().astype(np.float64), diag.cpu().numpy()
    x64 = x.astype(np.float64)
    nnz_i = np.count_nonzero(R.dense_adjacency(r, c, v, n), axis=1)
    bound = (nnz_i + 3) * U * (np.abs(lap) @ np.abs(x64))
    err = np.abs(y - lap @ x64)
    print(name, norm, "largest error over its bound:", (err / np.maximum(bound, 1e-300)).max() if n > 1 else 0.0)
    assert np.isfinite(y).all() and (err <= bound).all()
    assert (diag == op.scaling).all()


# ---------------------------------------------------------------- 3. the re-orthogonalisation
def ortho_case(n, j, near, seed):
    rng = np.random.default_rng(seed)
    v = np.linalg.qr(rng.standard_normal((n, j)))[0].T.astype(np.float32) if j else np.zeros((0, n), np.float32)
    u = rng.standard_normal(n)
    if near and j:
        a = rng.standard_normal(j)
        inside = v.astype(np.float64).T @ (a / np.linalg.norm(a))
        u = inside + 1e-3 * u / np.linalg.norm(u)
    return v, u.astype(np.float32)


def cgs2_f64(v, u):
    v, u = v.astype(np.float64), u.astype(np.float64)
    for _ in range(2):
        u = u - v.T @ (v @ u)
    return u / np.linalg.norm(u)


ORTHO_SHAPES = [(1, 0)] + [(n, j) for n in (64, 65, 1023, 1025, 5000) for j in (1, 2, 20, 41)] + [(300001, 2)]
# (n = 1 has no direction orthogonal to a row: it runs with an empty basis; 300001 columns make two elements per thread)


def numpy_levels(v, u, exact, orders=8):
    """What the two-pass scheme reaches in numpy float32 on these inputs: (max |V u|, direction error against float64), each the
    largest over `orders` summation orders - the n axis as it stands and seeded permutations of it. One run alone is a single
    draw of rounding noise (with one or two basis rows the statistic is one or two numbers far below 2^-24, and which BLAS
    kernel numpy calls decides it), so a ratio of two single draws says nothing; the largest of a few draws is the level."""
    v64 = v.astype(np.float64)
    lev, err = 0.0, 0.0
    for t in range(orders):
        perm = np.arange(len(u)) if t == 0 else np.random.default_rng(1000 + t).permutation(len(u))
        ref, _ = R.cgs2(np.ascontiguousarray(v[:, perm]), u[perm])
        out = np.empty_like(ref)
        out[perm] = ref
        o64 = out.astype(np.float64)
        lev = max(lev, np.abs(v64 @ o64).max() if len(v) else 0.0)
        err = max(err, np.linalg.norm(o64 - exact))
    return lev, err


@pytest.mark.parametrize("near", [False, True])
@pytest.mark.parametrize("n,j", ORTHO_SHAPES)
def test_orthogonalize_hook(res, n, j, near):
    v, u = ortho_case(n, j, near, 100 * j + n % 97)
    exact = cgs2_f64(v, u)
    lev_ref, dir_ref = numpy_levels(v, u, exact, 8 if n < 100000 else 2)
    got, norm = se().orthogonalize(dev(v), dev(u), resources=res)
    got = got.cpu().numpy()
    g64, v64 = got.astype(np.float64), v.astype(np.float64)
    assert np.isfinite(got).all() and norm > 0
    assert abs(np.linalg.norm(g64) - 1.0) <= 4 * U
    lev_dev = np.abs(v64 @ g64).max() if j else 0.0
    dir_dev = np.linalg.norm(g64 - exact)
    print("n", n, "j", j, "near" if near else "random", "max |V u| device", lev_dev, "numpy float32", lev_ref, "direction error device",
          dir_dev, "numpy float32", dir_ref)
    assert lev_dev <= 4 * lev_ref
    assert dir_dev <= 4 * dir_ref


# ---------------------------------------------------------------- 4. the solver
def check_eigenpairs(name, tol, evals, x, stats, k):
    (r, c, v, n), norm, _ = R.solver_cases()[name]
    lap, ev, vec = R.exact_spectrum(name)
    r_arpack = R.arpack_residual(name, int(stats["ncv"]))
    bound = tol + 4.0 * r_arpack
    resid = R.residuals(lap, evals, x)
    x64 = x.astype(np.float64)
    orth = np.abs(x64 @ x64.T - np.eye(k)).max()
    sine = R.subspace_sine(x, vec[:k])
    gap = ev[k] - ev[k - 1]
    print(name, "tol", tol, stats, "r_arpack", r_arpack, "residuals", resid, "eigenvalue error", np.abs(evals - ev[:k]).max(),
          "orthogonality", orth, "sine", sine, "of", 2.0 * np.linalg.norm(resid) / gap)
    assert np.isfinite(x).all()
    assert resid.max() <= bound  # (a)
    assert (np.diff(evals) >= 0).all() and np.abs(evals.astype(np.float64) - ev[:k]).max() <= bound  # (b)
    assert orth <= 8 * U * np.sqrt(n)  # (c)
    assert sine <= 2.0 * np.linalg.norm(resid) / gap  # (d)
    assert stats["converged"] == 1 and stats["matvecs"] <= 10 * n  # (e)


@pytest.mark.parametrize("tol", [1e-5, 0.0])
@pytest.mark.parametrize("name", ["ring200_unnorm", "ring200_norm", "three_unnorm", "three_norm", "grid_unnorm", "grid_norm", "blobs_norm",
                                  "blobs_unnorm", "uniform_norm", "uniform_unnorm"])
def test_solver_on_known_spectra(res, name, tol):
    g, norm, k = R.solver_cases()[name]
    dr, dc, dv, n = dev_graph(g)
    evals, x = se().eigsh(dr, dc, dv, n, k, norm_laplacian=norm, ncv=0, tolerance=tol, seed=0, resources=res)
    stats = se().last_stats()
    assert stats["ncv"] == R.ncv_rule(n, k)
    check_eigenpairs(name, tol, evals.cpu().numpy(), x.cpu().numpy(), stats, k)


# ---------------------------------------------------------------- 5. determinism
@pytest.mark.parametrize("name", ["ring200_norm", "blobs_unnorm"])
def test_solver_is_deterministic(res, name):
    g, norm, k = R.solver_cases()[name]
    dr, dc, dv, n = dev_graph(g)
    e1, x1 = se().eigsh(dr, dc, dv, n, k, norm_laplacian=norm, tolerance=0.0, seed=5, resources=res)
    e2, x2 = se().eigsh(dr, dc, dv, n, k, norm_laplacian=norm, tolerance=0.0, seed=5, resources=res)
    assert torch.equal(e1, e2) and torch.equal(x1, x2)
    e3, x3 = se().eigsh(dr, dc, dv, n, k, norm_laplacian=norm, tolerance=0.0, seed=6, resources=res)
    assert not torch.equal(x1, x3)
    check_eigenpairs(name, 0.0, e3.cpu().numpy(), x3.cpu().numpy(), se().last_stats(), k)


# ---------------------------------------------------------------- 6. transform end to end
@pytest.mark.parametrize("shape", R.TRANSFORM_SHAPES)
def test_transform_end_to_end(res, shape):
    from scipy.sparse import csr_matrix
    from scipy.sparse.linalg import eigsh as arpack

    n, dim, clusters, comps, k, std, norm, drop = shape
    tol = 1e-5
    x, labels, _, _ = R.blobs_graph(n, dim, clusters, k, std, 42)
    dx = dev(x)
    p = se().Params(n_components=comps, n_neighbors=k, norm_laplacian=norm, drop_first=drop, tolerance=tol, seed=42)
    c_out = comps - (1 if drop else 0)
    emb, evals = se().transform(p, dx, eigenvalues=True, resources=res)
    assert tuple(emb.shape) == (n, c_out) and emb.is_contiguous() and tuple(evals.shape) == (comps,)
    emb_f = se().transform(p, dx, order="F", resources=res)
    assert emb_f.stride() == (1, n) and torch.equal(emb_f, emb)
    host_vals = np.zeros(comps, np.float32)
    se().transform(p, dx, eigenvalues=host_vals, resources=res)
    assert (host_vals == evals.cpu().numpy()).all()
    # transform is the graph followed by transform_graph, bit for bit
    gr, gc, gv = se().create_connectivity_graph(p, dx, resources=res)
    emb_g, evals_g = se().transform_graph(p, gr, gc, gv, n, eigenvalues=True, resources=res)
    assert torch.equal(emb_g, emb) and torch.equal(evals_g, evals)
    other = se().Params(n_components=comps, n_neighbors=k, norm_laplacian=norm, drop_first=not drop and comps > 1, tolerance=tol, seed=42)
    assert tuple(se().transform(other, dx, resources=res).shape) == (n, comps - (1 if other.drop_first else 0))
    emb, evals = emb.cpu().numpy(), evals.cpu().numpy()
    assert np.isfinite(emb).all()
    top = np.argmax(np.abs(emb), axis=0)
    assert (emb[top, np.arange(c_out)] > 0).all(), "the sign rule"
    # the embedding is the solver's eigenvectors, scaled, cut and signed: the same float32 operations
    g = (gr.cpu().numpy(), gc.cpu().numpy(), gv.cpu().numpy(), n)
    ev_s, xs = se().eigsh(gr, gc, gv, n, comps, norm_laplacian=norm, tolerance=tol, seed=42, resources=res)
    stats = se().last_stats()
    xs = xs.cpu().numpy()
    op = R.Operator(*g, norm)
    e = (xs.T / op.scaling[:, None]).astype(np.float32) if norm else xs.T.copy()
    assert (R.sign_flip(e[:, 1:] if drop else e) == emb).all() and (ev_s.cpu().numpy() == evals).all()
    # against float64 and the twin, on the device's own graph
    lap, _ = R.laplacian(*g, norm)
    ev, vec = np.linalg.eigh(lap)
    k2 = R.cluster_end(ev, comps)
    w, av = arpack(csr_matrix(lap.astype(np.float32)), k=comps, which="SA", ncv=int(stats["ncv"]), tol=R.EPS32, v0=R.start_vector(0, n))
    bound = tol + 4.0 * float(R.residuals(lap, np.sort(w), av.T[np.argsort(w)]).max())
    resid = R.residuals(lap, evals, xs)
    _, t_evals, t_xs, _ = R.embedding(*g, comps, norm, drop, tol, 42)
    t_resid = R.residuals(lap, t_evals, t_xs)
    gap = ev[k2] - ev[comps - 1]
    sine, t_sine = R.subspace_sine(xs, vec.T[:k2]), R.subspace_sine(t_xs, vec.T[:k2])
    print(shape, stats, "bound", bound, "residuals", resid, "twin", t_resid, "sine", sine, "twin", t_sine, "gap", gap, "group", k2)
    assert resid.max() <= bound and np.abs(evals - ev[:comps]).max() <= bound
    assert sine <= 2.0 * np.linalg.norm(resid) / gap and t_sine <= 2.0 * np.linalg.norm(t_resid) / gap
    assert np.abs(evals - t_evals).max() <= 2 * bound


# ---------------------------------------------------------------- 7. clustering
def cluster(res, shape, std, seed_blobs):
    from cuvs_amd.cluster import spectral

    n, dim, clusters, k, n_init, seed = shape
    x, labels, _, _ = R.blobs_graph(n, dim, clusters, k, std, seed_blobs)
    p = spectral.Params(n_clusters=clusters, n_components=clusters, n_init=n_init, n_neighbors=k, tolerance=0.0, seed=seed)
    dx = dev(x)
    found = spectral.fit_predict(p, dx, resources=res)
    assert found.dtype == torch.int32 and tuple(found.shape) == (n,)
    gr, gc, gv = se().create_connectivity_graph(se().Params(n_neighbors=k), dx, resources=res)
    again = spectral.fit_predict(p, graph=(gr, gc, gv, n), resources=res)
    assert torch.equal(found, again), "the dataset and the graph entry points agree"
    found = found.cpu().numpy()
    assert found.min() >= 0 and found.max() < clusters
    return R.adjusted_rand_index(found, labels)


@pytest.mark.parametrize("shape", R.CLUSTER_SHAPES)
def test_clustering_of_separated_blobs(res, shape):
    assert cluster(res, shape, 0.3, shape[5]) == 1.0


def test_clustering_of_overlapping_blobs(res):
    ari = cluster(res, R.OVERLAP_SHAPE, 2.5, R.OVERLAP_SHAPE[5])
    print("adjusted Rand index:", ari)
    assert ari > 0.7


# ---------------------------------------------------------------- 8. refusals
def test_refusals_leave_the_outputs_untouched(res):
    from cuvs_amd._lib import CuvsError, Tensor, lib
    from cuvs_amd.cluster import spectral

    n, k = 40, 5
    x = dev(R.uniform(n, 4, 3))
    gr, gc, gv = se().create_connectivity_graph(se().Params(n_neighbors=k), x, resources=res)
    P = se().Params

    def refused(call, *outputs):
        before = [o.clone() for o in outputs]
        with pytest.raises(CuvsError):
            call()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(before, outputs))

    emb = torch.full((n, 1), 7.0, device="cuda")
    emb2 = torch.full((n, 2), 7.0, device="cuda")
    lab = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    # a tensor that is not fp32, or lives on the host where the device is required
    refused(lambda: se().transform(P(), x.double(), embedding=emb, resources=res), emb)
    refused(lambda: se().transform(P(), x.cpu(), embedding=emb, resources=res), emb)
    refused(lambda: se().transform(P(), x, embedding=emb.cpu(), resources=res))
    refused(lambda: se().transform_graph(P(), gr, gc, gv.double(), n, embedding=emb, resources=res), emb)
    refused(lambda: spectral.fit_predict(spectral.Params(n_clusters=2, n_components=2), x, labels=lab.cpu(), resources=res))
    # n_components < 1, n_components >= n, drop_first with n_components < 2
    refused(lambda: se().transform(P(n_components=0, drop_first=False), x, embedding=torch.empty((n, 0), device="cuda"), resources=res))
    refused(lambda: se().transform(P(n_components=n, drop_first=True), x, embedding=torch.full((n, n - 1), 7.0, device="cuda"), resources=res))
    refused(lambda: se().transform(P(n_components=1, drop_first=True), x, embedding=torch.empty((n, 0), device="cuda"), resources=res))
    # n_neighbors < 1 or >= n
    refused(lambda: se().transform(P(n_neighbors=0), x, embedding=emb, resources=res), emb)
    refused(lambda: se().transform(P(n_neighbors=n), x, embedding=emb, resources=res), emb)
    # n_clusters < 1 or > n
    refused(lambda: spectral.fit_predict(spectral.Params(n_clusters=0, n_components=2, n_neighbors=k), x, labels=lab, resources=res), lab)
    refused(lambda: spectral.fit_predict(spectral.Params(n_clusters=n + 1, n_components=2, n_neighbors=k), x, labels=lab, resources=res), lab)
    # index tensors that are not int32
    refused(lambda: se().transform_graph(P(), gr.long(), gc, gv, n, embedding=emb, resources=res), emb)
    refused(lambda: spectral.fit_predict(spectral.Params(n_clusters=2, n_components=2), graph=(gr, gc.long(), gv, n), labels=lab, resources=res), lab)
    refused(lambda: spectral.fit_predict(spectral.Params(n_clusters=2, n_components=2, n_neighbors=k), x, labels=lab.long(), resources=res))
    # capacity smaller than 2 n k
    cap = 2 * n * k
    rows = torch.full((cap - 1,), -7, dtype=torch.int32, device="cuda")
    cols = torch.full((cap,), -7, dtype=torch.int32, device="cuda")
    vals = torch.full((cap,), -7.0, device="cuda")
    nnz = C.c_int64(-7)

    def small_capacity():
        from cuvs_amd._lib import check

        p = P(n_neighbors=k)._c()
        ts = [Tensor(t) for t in (x, rows, cols, vals)]
        check(lib().cuvsAmdSpectralConnectivityGraph(res.get_c_obj(), C.byref(p), *[t.ptr for t in ts], C.byref(nnz)))

    refused(small_capacity, rows, cols, vals)
    assert nnz.value == -7
    # nnz < 0

    def negative_nnz():
        from cuvs_amd._lib import check

        p = P()._c()
        ts = [Tensor(t) for t in (gr, gc, gv, emb)]
        for t in ts[:3]:
            t._shape[0] = -1
        check(lib().cuvsAmdSpectralEmbeddingTransformGraph(res.get_c_obj(), C.byref(p), ts[0].ptr, ts[1].ptr, ts[2].ptr, C.c_int64(n), ts[3].ptr,
                                                           None))

    refused(negative_nnz, emb)
    # entries outside [0, n) are refused too (the kernels index with them)
    bad = gr.clone()
    bad[0] = n
    refused(lambda: se().transform_graph(P(), bad, gc, gv, n, embedding=emb, resources=res), emb)
    # and a well-formed call still works afterwards
    out = se().transform(P(n_components=3, n_neighbors=k), x, embedding=emb2, resources=res)
    assert out is emb2 and torch.isfinite(emb2).all() and not (emb2 == 7.0).all()


def test_iteration_cap_raises_a_warning(res):
    # a basis of k + 1 vectors makes every cycle one step: the ring is far from converged after 10 n products (the twin: CPU test).
    # The solver returns its last Ritz pairs with success and says so.
    g, norm, k = R.solver_cases()["ring200_norm"]
    dr, dc, dv, n = dev_graph(g)
    with pytest.warns(RuntimeWarning, match="matrix-vector products"):
        evals, x = se().eigsh(dr, dc, dv, n, k, norm_laplacian=norm, ncv=k + 1, tolerance=0.0, seed=0, resources=res)
    stats = se().last_stats()
    assert stats["converged"] == 0 and stats["matvecs"] == 10 * n and stats["ncv"] == k + 1
    evals, x = evals.cpu().numpy(), x.cpu().numpy().astype(np.float64)
    assert np.isfinite(x).all() and (np.diff(evals) >= 0).all() and evals[0] > -1e-5 and evals[-1] < 0.1
    assert np.abs(x @ x.T - np.eye(k)).max() <= 8 * U * np.sqrt(n)
