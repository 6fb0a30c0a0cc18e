"""CPU: the numpy twin of spectral embedding and clustering (tests/spectral_ref.py) - its Laplacian against scipy, its solver
against numpy.linalg.eigh by the criteria the GPU tests use on the same graphs, the conditions those tests rely on (neighbour
margins, spectral gaps, connected components) - the host-only helper against numpy.linalg.eigh, and the build checks."""
import os
import subprocess

import numpy as np
import pytest

from tests import spectral_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ["cuvsAmdSpectralEmbeddingParamsCreate", "cuvsAmdSpectralEmbeddingParamsDestroy", "cuvsAmdSpectralConnectivityGraph",
           "cuvsAmdSpectralEmbeddingTransform", "cuvsAmdSpectralEmbeddingTransformGraph", "cuvsAmdSpectralClusteringParamsCreate",
           "cuvsAmdSpectralClusteringParamsDestroy", "cuvsAmdSpectralClusteringFitPredict", "cuvsAmdSpectralClusteringFitPredictGraph",
           "cuvsAmdSpectralEigsh", "cuvsAmdSpectralLaplacianMatvec", "cuvsAmdSpectralOrthogonalize", "cuvsAmdSpectralLastStats"]


# ---------------------------------------------------------------- the twin's pieces
def test_mix_hash_and_start_vector():
    # mix_hash.hpp by hand: seed 0, i 0 is the finalizer of 0; the values tests/hnsw_ref.py pins come from the same function
    from tests import hnsw_ref

    i = np.arange(1000, dtype=np.uint32)
    assert (R.mix_hash(5, i) == np.array([hnsw_ref.level_hash(5, int(t)) for t in i], np.uint32)).all()
    u = R.start_vector(0, 4096)
    assert u.dtype == np.float32 and u.min() >= -1.0 and u.max() < 1.0 and abs(float(u.mean())) < 0.05
    assert (R.start_vector(0, 64, 1) != R.start_vector(0, 64, 0)).any() and (R.start_vector(1 << 32, 64) != R.start_vector(1, 64)).any()
    # exact in float32: the same numbers from float64 arithmetic
    h = R.mix_hash(int(R.mix_hash(0, np.uint32(0))), np.arange(64, dtype=np.uint32))
    assert (u[:64].astype(np.float64) == (h >> 8).astype(np.float64) * 2.0 ** -23 - 1.0).all()


@pytest.mark.parametrize("norm", [False, True])
def test_twin_laplacian_against_scipy(norm):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import laplacian

    r, c, v, n = R.messy(41)
    assert (r == c).any(), "self-loops"
    keys = (r.astype(np.int64) << 32) | c
    assert len(np.unique(keys)) < len(keys), "duplicate entries"
    w = R.dense_adjacency(r, c, v, n)
    assert (w == w.T).all() and w[n - 1].sum() == 0 and w[:, n - 1].sum() == 0, "symmetric, one isolated vertex"
    lap, scaling = R.laplacian(r, c, v, n, norm)
    off = r != c
    m = coo_matrix((v[off].astype(np.float64), (r[off], c[off])), shape=(n, n)).tocsr()  # (duplicates summed)
    ref, d = laplacian(m, normed=norm, return_diag=True)
    assert np.abs(lap - ref.toarray()).max() <= 1e-12
    assert np.abs(scaling - d).max() <= 1e-12
    # the solver's float32 operator is that matrix to float32 accuracy, row by row
    op = R.Operator(r, c, v, n, norm)
    x = R.start_vector(3, n)
    y = op.matvec(x).astype(np.float64)
    bound = (np.count_nonzero(w, axis=1) + 3) * R.U32 * (np.abs(lap) @ np.abs(x.astype(np.float64)))
    assert (np.abs(y - lap @ x.astype(np.float64)) <= bound).all()
    assert (op.deg.astype(np.float64) == w.sum(1)).all(), "the degrees are exact for these weights"
    assert np.abs(op.scaling.astype(np.float64) - scaling).max() <= R.U32 * scaling.max()


def test_sign_rule_and_rand_index():
    e = np.array([[1.0, -3.0, 2.0], [-2.0, 3.0, -2.0], [0.5, 1.0, 1.0]])
    f = R.sign_flip(e)
    assert (f[:, 0] == -e[:, 0]).all() and (f[:, 1] == -e[:, 1]).all() and (f[:, 2] == e[:, 2]).all()  # ties: the lowest index
    a = np.array([0, 0, 1, 1, 2, 2])
    assert R.adjusted_rand_index(a, np.array([2, 2, 0, 0, 1, 1])) == 1.0
    assert abs(R.adjusted_rand_index(a, np.array([0, 0, 1, 2, 2, 2])) - 0.4444444444444444) < 1e-12  # sklearn's value
    assert abs(R.adjusted_rand_index(np.array([0, 0, 1, 1]), np.array([0, 1, 0, 1])) + 0.5) < 1e-12


# ---------------------------------------------------------------- conditions of the GPU tests
@pytest.mark.parametrize("n,dim,k", R.KNN_SHAPES)
def test_knn_inputs_are_unambiguous(n, dim, k):
    x, ids, margin, (rows, cols, vals, _) = R.knn_graph_case(n, dim, k)
    assert margin > 1e-4, "a neighbour set would depend on rounding"
    assert (ids[:, 0] == np.arange(n)).all() and ids.min() >= 0 and ids.max() < n, "every row is its own first neighbour; none is left out"
    assert len(np.unique(np.concatenate([rows, cols]))) == n
    keys = (rows.astype(np.int64) << 32) | cols
    assert (np.diff(keys) > 0).all() and set(np.unique(vals)) <= {0.5, 1.0} and len(rows) <= 2 * n * k
    w = np.zeros((n, n), np.float32)
    w[rows, cols] = vals
    assert (w == w.T).all() and (np.diag(w) == 1.0).all()


@pytest.mark.parametrize("name", sorted(R.solver_cases()))
def test_solver_inputs_have_a_gap(name):
    (r, c, v, n), norm, k = R.solver_cases()[name]
    _, ev, _ = R.exact_spectrum(name)
    print(name, "gap", ev[k] - ev[k - 1], "first eigenvalues", ev[:k + 1])
    assert ev[k] - ev[k - 1] >= 1e-3
    w = R.dense_adjacency(r, c, v, n)
    assert (w == w.T).all()
    if name.startswith("ring200_unnorm"):
        exact = np.sort(2.0 - 2.0 * np.cos(2.0 * np.pi * np.arange(n) / n))
        assert np.abs(ev - exact).max() < 1e-12 and abs(ev[1] - ev[2]) < 1e-12 and abs(ev[3] - ev[4]) < 1e-12, "degenerate pairs"
    if name.startswith("three"):
        assert np.abs(ev[:3]).max() < 1e-12 and ev[3] > 1e-3, "a zero eigenvalue of multiplicity 3"


@pytest.mark.parametrize("tol", [1e-5, 0.0])
@pytest.mark.parametrize("name", sorted(R.solver_cases()))
def test_twin_solver_against_eigh(name, tol):
    """criteria (a) to (e) of the GPU solver test, on the twin"""
    (r, c, v, n), norm, k = R.solver_cases()[name]
    lap, ev, vec = R.exact_spectrum(name)
    evals, x, stats = R.eigsh(r, c, v, n, norm, k, 0, tol, 0)
    bound = tol + 4.0 * R.arpack_residual(name, stats["ncv"])
    res = R.residuals(lap, evals, x)
    orth = np.abs(x.astype(np.float64) @ x.astype(np.float64).T - np.eye(k)).max()
    sine = R.subspace_sine(x, vec[:k])
    print(name, tol, stats, "residual", res.max(), "bound", bound, "orthogonality", orth, "sine", sine)
    assert res.max() <= bound
    assert (np.diff(evals) >= 0).all() and np.abs(evals - ev[:k]).max() <= bound
    assert orth <= 8 * R.U32 * np.sqrt(n)
    assert sine <= 2.0 * np.linalg.norm(res) / (ev[k] - ev[k - 1])
    assert stats["converged"] == 1 and stats["matvecs"] <= 10 * n and stats["ncv"] == 20


def test_twin_solver_survives_an_exhausted_krylov_space():
    # the start vector of a graph of isolated vertices spans an invariant subspace at once; tiny graphs exhaust R^n
    z = np.zeros(0, np.int32)
    evals, x, stats = R.eigsh(z, z, np.zeros(0, np.float32), 30, True, 3, 0, 1e-5, 0)
    assert np.isfinite(x).all() and (evals == 0).all() and np.abs(x @ x.T - np.eye(3)).max() < 1e-5
    r, c, v, n = R.path(3)
    evals, x, stats = R.eigsh(r, c, v, n, False, 2, 0, 0.0, 0)
    assert stats["converged"] == 1 and np.abs(evals - [0.0, 1.0]).max() < 1e-5 and np.isfinite(x).all()


def test_twin_solver_stops_at_the_cap():
    # the input of the GPU test of the warning: with ncv = k + 1 the ring does not converge within 10 n products
    g, norm, k = R.solver_cases()["ring200_norm"]
    evals, x, stats = R.eigsh(*g, norm, k, k + 1, 0.0, 0)
    assert stats["converged"] == 0 and stats["matvecs"] == 10 * g[3] and np.isfinite(x).all()


@pytest.mark.parametrize("shape", R.TRANSFORM_SHAPES)
def test_transform_inputs(shape):
    """the eigenvalue groups the embedding's columns are compared in end within the spectrum, and the twin's embedding obeys the
    sign rule"""
    n, dim, clusters, comps, k, std, norm, drop = shape
    x, labels, margin, (r, c, v, _) = R.blobs_graph(n, dim, clusters, k, std, 42)
    lap, _ = R.laplacian(r, c, v, n, norm)
    ev = np.linalg.eigvalsh(lap)
    k2 = R.cluster_end(ev, comps)
    print(shape, "components kept", comps, "group ends at", k2, "gap", ev[k2] - ev[comps - 1])
    assert k2 < n // 2 and ev[k2] - ev[comps - 1] >= 1e-3
    emb, evals, xs, stats = R.embedding(r, c, v, n, comps, norm, drop, 1e-5, 0)
    assert emb.shape == (n, comps - (1 if drop else 0)) and stats["converged"] == 1
    idx = np.argmax(np.abs(emb), axis=0)
    assert (emb[idx, np.arange(emb.shape[1])] > 0).all()
    assert R.subspace_sine(xs, np.linalg.eigh(lap)[1].T[:k2]) <= 2.0 * np.linalg.norm(R.residuals(lap, evals, xs)) / (ev[k2] - ev[comps - 1])


@pytest.mark.parametrize("shape", R.CLUSTER_SHAPES)
def test_cluster_inputs_are_disconnected_blobs(shape):
    n, dim, clusters, k, n_init, seed = shape
    x, labels, margin, (r, c, v, _) = R.blobs_graph(n, dim, clusters, k, 0.3, seed)
    count, comp = R.n_components(r, c, n)
    assert count == clusters and R.adjusted_rand_index(comp, labels) == 1.0
    # then the rows of the embedding are constant per component up to the residual
    emb, evals, xs, stats = R.embedding(r, c, v, n, clusters, True, False, 0.0, seed)
    assert np.abs(evals).max() < 1e-5
    spread = max(np.abs(emb[labels == t] - emb[labels == t].mean(0)).max() for t in range(clusters))
    centres = np.stack([emb[labels == t].mean(0) for t in range(clusters)])
    apart = min(np.linalg.norm(centres[a] - centres[b]) for a in range(clusters) for b in range(a))
    print(shape, "spread within a component", spread, "smallest distance between components", apart)
    assert spread < 1e-3 * apart


def test_overlap_input_is_clusterable():
    from scipy.cluster.vq import kmeans2

    n, dim, clusters, k, n_init, seed = R.OVERLAP_SHAPE
    x, labels, margin, (r, c, v, _) = R.blobs_graph(n, dim, clusters, k, 2.5, seed)
    emb, evals, xs, stats = R.embedding(r, c, v, n, clusters, True, False, 0.0, seed)
    _, found = kmeans2(emb.astype(np.float64), clusters, minit="++", seed=1)
    ari = R.adjusted_rand_index(found, labels)
    print("adjusted Rand index of k-means on the twin's embedding:", ari)
    assert ari > 0.9


# ---------------------------------------------------------------- the host helper and the build
def test_host_helper_against_eigh(tmp_path):
    exe = tmp_path / "spectral_host_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-I", os.path.join(ROOT, "cuvs_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "spectral_host_test.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = out.stdout.split("\n")
    assert "spectral host OK" in lines
    pos, seen = 0, []
    while lines[pos].startswith("order "):
        m = int(lines[pos].split()[1])
        vals = np.array([float(t) for t in lines[pos + 1:pos + 1 + 2 * m * m + m]])
        pos += 1 + 2 * m * m + m
        t, evals, vecs = vals[:m * m].reshape(m, m), vals[m * m:m * m + m], vals[m * m + m:].reshape(m, m)
        assert (t == t.T).all() and (m < 3 or np.count_nonzero(np.triu(t, 2)) > 0), "arrow plus tridiagonal"
        bound = 16 * m * 2.0 ** -52 * np.linalg.norm(t, 2)
        ref = np.linalg.eigh(t)[0]
        err, orth = np.abs(evals - ref).max(), np.abs(vecs.T @ vecs - np.eye(m)).max()
        back = np.abs(t @ vecs - vecs * evals[None, :]).max()
        print("order", m, "eigenvalue error", err, "orthogonality", orth, "residual", back, "bound", bound)
        assert (np.diff(evals) >= 0).all() and err <= bound and orth <= bound and back <= bound
        seen.append(m)
    assert seen == [1, 2, 21, 129]


def test_header_is_c_and_cpp_and_symbols_are_exported(tmp_path):
    src = tmp_path / "c.c"
    src.write_text('#include <cuvs_amd/spectral.h>\nint main(void) { struct cuvsAmdSpectralEmbeddingParams p; struct '
                   'cuvsAmdSpectralClusteringParams q; (void)p; (void)q; return 0; }\n')
    inc = os.path.join(ROOT, "include")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Werror", "-fsyntax-only", "-I", inc, str(src)])
    cpp = tmp_path / "c.cpp"
    cpp.write_text(src.read_text())
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", inc, str(cpp)])
    from cuvs_amd._lib import lib

    assert all(hasattr(lib(), s) for s in EXPORTS)
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "cuvs_amd", "libcuvs_c.so")], text=True)
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(EXPORTS) <= names
    header = open(os.path.join(inc, "cuvs_amd", "spectral.h")).read()
    assert all(s + "(" in header for s in EXPORTS)
    assert "ASSUMED SYMMETRIC" in header


def test_python_modules_are_exported():
    from cuvs_amd import cluster, preprocessing

    assert all(hasattr(preprocessing.spectral_embedding, f) for f in ("Params", "transform", "transform_graph", "create_connectivity_graph"))
    assert all(hasattr(cluster.spectral, f) for f in ("Params", "fit_predict"))
    p = preprocessing.spectral_embedding.Params()
    assert (p.n_components, p.n_neighbors, p.norm_laplacian, p.drop_first, p.seed) == (2, 15, True, True, 0) and p.n_columns == 1
