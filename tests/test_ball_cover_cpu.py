"""CPU: the numpy twin of the random ball cover (tests/ball_cover_ref.py). Its index search against its own brute force on
inputs that sit on the pruning boundaries, for every landmark count and three seeds: this is what proves the margin of
DESIGN 3.1u conservative, independently of any device. Then: a boundary input on which the search without the margin is
wrong, the haversine formula against fp64, the C header, the C++ namespace, the exported symbols and the host-only helper
under the sanitizers."""
import functools
import os
import subprocess

import numpy as np
import pytest

from tests import ball_cover_ref as R
from tests import eps_neighbors_ref as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ["cuvsAmdBallCoverIndexParamsCreate", "cuvsAmdBallCoverIndexParamsDestroy", "cuvsAmdBallCoverIndexCreate",
           "cuvsAmdBallCoverIndexDestroy", "cuvsAmdBallCoverBuild", "cuvsAmdBallCoverKnnQuery", "cuvsAmdBallCoverAllKnnQuery",
           "cuvsAmdBallCoverEpsNn", "cuvsAmdBallCoverEpsNnCsr", "cuvsAmdBallCoverIndexGetNLandmarks", "cuvsAmdBallCoverIndexGetSize",
           "cuvsAmdBallCoverIndexGetDim", "cuvsAmdBallCoverIndexGetMetric", "cuvsAmdBallCoverIndexGetArray", "cuvsAmdBallCoverLastStats"]


@functools.lru_cache(maxsize=None)
def adversarial(name):
    """(X, Q): small editions of the inputs of the GPU tests"""
    if name == "lattice2":
        X = R.lattice(2, 20)
        return X, np.concatenate([X[:24], X[:8] + np.float32(0.5)])
    if name == "lattice3":
        X = R.lattice(3, 8)
        return X, np.concatenate([X[:24], X[:8] + np.float32(0.5)])
    if name == "blobs":
        X = R.blobs(500, 2, 3)
        return X, np.concatenate([X[:16], R.blobs(16, 2, 4)])
    if name == "shell":
        return R.shell(480, 4, 2, 5)
    if name == "shell3":
        return R.shell(480, 4, 3, 6)
    if name == "duplicated":
        X = R.duplicated(400, 2, 7)
        return X, X[:32]
    raise KeyError(name)


INPUTS = ["lattice2", "lattice3", "blobs", "shell", "shell3", "duplicated"]


@pytest.mark.parametrize("name", INPUTS)
def test_twin_search_equals_twin_brute_force(name):
    X, Q = adversarial(name)
    m = len(X)
    d = R.l2(Q, X)
    for n_landmarks in (1, 2, 0, m):
        for seed in (0, 1, 2):
            index = R.build(X, "euclidean", n_landmarks, seed)
            for k in {1, min(5, index["L"]), min(11, index["L"])}:
                want_i, want_d = R.brute(X, Q, k, d=d)
                got_i, got_d, _ = R.knn(index, Q, k)
                assert (got_i == want_i).all() and (got_d.view(np.uint32) == want_d.view(np.uint32)).all(), (name, n_landmarks, seed, k)


def test_twin_build_invariants():
    X = R.duplicated(400, 2, 7)
    for n_landmarks, seed in ((0, 0), (400, 1), (7, 2)):
        ix = R.build(X, "euclidean", n_landmarks, seed)
        L = ix["L"]
        assert L == (n_landmarks or 20) and len(set(ix["R_rows"].tolist())) == L
        assert sorted(ix["R_1nn_cols"].tolist()) == list(range(400)) and ix["R_indptr"][-1] == 400
        for l in range(L):
            beg, end = ix["R_indptr"][l], ix["R_indptr"][l + 1]
            sd, cols = ix["R_1nn_dists"][beg:end], ix["R_1nn_cols"][beg:end]
            assert (np.diff(sd) >= 0).all() and ((np.diff(sd) > 0) | (np.diff(cols) > 0)).all()
            assert ix["R_radius"][l] == (sd[-1] if end > beg else 0)
    # the landmarks are a function of (m, n, seed) and a prefix of a larger draw
    assert (R.landmarks(400, 7, 2) == R.landmarks(400, 400, 2)[:7]).all() and (R.landmarks(400, 7, 2) != R.landmarks(400, 7, 3)).any()
    # copies drawn as two landmarks: the later one's list is empty, its radius 0
    ix = R.build(X, "euclidean", 400, 0)
    sizes = np.diff(ix["R_indptr"])
    assert (sizes == 0).sum() > 50 and (ix["R_radius"][sizes == 0] == 0).all()


def test_twin_approximate_modes_are_subsets():
    X, Q = adversarial("blobs")
    index = R.build(X, "euclidean", 0, 0)
    k = 5
    exact_i, exact_d = R.brute(X, Q, k)
    for post, weight in ((False, 1.0), (True, 0.5), (True, 0.9)):
        ids, dd, _ = R.knn(index, Q, k, post, weight)
        assert (np.diff(dd.astype(np.float64), axis=1) >= 0).all()      # sorted by distance
        assert (dd >= exact_d).all()                                    # never better than the exact answer
    # one landmark holds every row: the search is exact in every mode
    one = R.build(X, "euclidean", 1, 0)
    ids, dd, _ = R.knn(one, Q, 1, False)
    assert (ids == R.brute(X, Q, 1)[0]).all()
    # the k nearest lists always hold the k landmark rows themselves, so a drawn index never pads
    tiny = R.build(X[:3], "euclidean", 3, 0)
    ids, dd, _ = R.knn(tiny, X[:3] + np.float32(100), 3, False)
    assert (np.sort(ids, axis=1) == np.arange(3)).all() and (dd < R.PAD_DIST).all()
    # the fill itself: one row named twice as a landmark leaves three lists with two rows between them
    short = R.build(X[:2], "euclidean", landmark_rows=[0, 0, 1])
    assert np.diff(short["R_indptr"]).tolist() == [1, 0, 1]
    for post in (False, True):
        ids, dd, _ = R.knn(short, X[:4], 3, post)
        want_i, want_d = R.brute(X[:2], X[:4], 2)
        assert (ids[:, :2] == want_i).all() and (dd[:, :2] == want_d).all()
        assert (ids[:, 2] == R.PAD_ID).all() and (dd[:, 2] == R.PAD_DIST).all()


def test_margin_is_necessary():
    """Three points on a ray from landmark A at the origin, p = s (1, 1), the query q = t (1, 1) and landmark B = p' = (2 t - s)
    (1, 1), with integer s < t: p and p' are equally far from q, bit for bit, and the smaller id (p) wins. p is the last row
    of A's list. Where fl(fl(t sqrt 2) - fl(s sqrt 2)) > fl((t - s) sqrt 2), the expression without its margin skips A's list
    and returns p'."""
    s2 = np.float64(2.0)
    found = None
    for t in range(3, 400):
        for s in range(1, t):  # s < 2 (t - s): p is nearer to A than to B
            dq, dp, dqp = np.float32(np.sqrt(s2 * t * t)), np.float32(np.sqrt(s2 * s * s)), np.float32(np.sqrt(s2 * (t - s) * (t - s)))
            if np.float32(dq - dp) > dqp and s < 2 * (t - s):
                found = (s, t)
                break
        if found:
            break
    assert found is not None, "no boundary input: the margin could be dropped"
    s, t = found
    X = np.array([[0, 0], [s, s], [2 * t - s, 2 * t - s]], np.float32)
    Q = np.array([[t, t]], np.float32)
    index = R.build(X, "euclidean", landmark_rows=[0, 2])
    assert index["R_1nn_cols"].tolist() == [0, 1, 2] and index["R_indptr"].tolist() == [0, 2, 3]
    want = R.brute(X, Q, 1)
    assert want[0].tolist() == [[1]]
    got = R.knn(index, Q, 1)
    assert (got[0] == want[0]).all() and (got[1] == want[1]).all()
    wrong = R.knn(index, Q, 1, c=0.0)
    assert wrong[0].tolist() == [[2]]  # the tie at the same distance bits went to the larger id


def test_twin_eps_walk_equals_membership():
    for name, dim_pad, radii in (("lattice2", 0, (5.0, 3.0)), ("lattice3", 0, (3.0,)), ("shell", 0, (1.0, 0.75)), ("duplicated", 0, (0.75,)),
                                 ("blobs", 14, (0.75,))):
        X, Q = adversarial(name)
        if dim_pad:  # eps_nn takes up to 32 columns
            rng = np.random.default_rng(11)
            X = np.concatenate([X, rng.normal(0, 0.05, (len(X), dim_pad)).astype(np.float32)], axis=1)
            Q = np.concatenate([Q, rng.normal(0, 0.05, (len(Q), dim_pad)).astype(np.float32)], axis=1)
        acc = E.chain(Q, X)
        for eps in radii:
            want = E.member(acc, np.float32(eps) * np.float32(eps))
            for n_landmarks, seed in ((0, 0), (0, 1), (1, 0), (len(X), 0)):
                got, _ = R.eps_adj(R.build(X, "euclidean", n_landmarks, seed), Q, eps)
                assert (got == want).all(), (name, eps, n_landmarks, seed)
    # the shell rows sit a few ulp around radius 1 of their query: both sides of the comparison occur
    X, Q = adversarial("shell")
    on = E.member(E.chain(Q[:4], X), np.float32(1.0))[np.arange(480) % 4, np.arange(480)]
    assert 0.05 < on.mean() < 0.95


def test_twin_prunes_the_blobs():
    """the bound the GPU test asserts, shown on the twin first: fewer than half of q * m rows are scored"""
    X = R.blobs(3000, 2, 1)
    Q = X[:64]
    index = R.build(X, "euclidean", 0, 0)
    _, _, stats = R.knn(index, Q, 5)
    assert stats["points_scored"] < len(Q) * len(X) // 2
    assert stats["points_scored"] < len(Q) * len(X) // 10  # (in fact far fewer)


def test_haversine_twin_against_fp64():
    X = R.geo(600, 3)
    d32 = R.haversine(X[:100], X)
    d64 = R.haversine(X[:100], X, np.float64)
    pos = d64 > 0
    assert (d32[~pos] == 0).all()
    e_cpu = float(np.max(np.abs(d32.astype(np.float64) - d64)[pos] / d64[pos]))
    print("haversine e_cpu", e_cpu, "largest absolute deviation", np.abs(d32.astype(np.float64) - d64).max())
    # the margins of the pruning expressions cover the formula's own error with room: 2^-8 relative, 2^-16 absolute
    assert (np.abs(d32.astype(np.float64) - d64) <= 2.0 ** -11 * d64 + 2.0 ** -20).all()
    # symmetric bit for bit, zero on the diagonal, the seam is no obstacle
    assert (R.haversine(X[:50], X[:50]).T.view(np.uint32) == R.haversine(X[:50], X[:50]).view(np.uint32)).all()
    a = np.array([[0.1, np.pi - 1e-3]], np.float32)
    b = np.array([[0.1, -np.pi + 1e-3]], np.float32)
    assert R.haversine(a, b)[0, 0] < 2.1e-3
    # the index search is exact under the computed distances
    index = R.build(X, "haversine", 0, 0)
    want = R.brute(X, X[:40], 5, "haversine")
    got = R.knn(index, X[:40], 5)
    assert (got[0] == want[0]).all() and (got[1] == want[1]).all()


@pytest.mark.parametrize("name", ["geo", "globe"])
def test_twin_haversine_search_equals_twin_brute_force(name):
    """the haversine margins (an estimate with a safety factor) on both inputs of the GPU tests, in small: blobs
    with pole and seam rows, and rows all over the globe with antipodal and seam queries"""
    if name == "geo":
        X = R.geo(400, 3)
        Q = np.concatenate([X[:24], R.geo(8, 4)])
    else:
        X, Q = R.globe(400, 30, 9)
    d = R.haversine(Q, X)
    for n_landmarks, seed in ((1, 0), (2, 0), (2, 1), (0, 0), (0, 1), (0, 2), (400, 0), (400, 1)):
        index = R.build(X, "haversine", n_landmarks, seed)
        for k in {1, min(5, index["L"]), min(11, index["L"])}:
            want_i, want_d = R.brute(X, Q, k, "haversine", d=d)
            got_i, got_d, _ = R.knn(index, Q, k)
            assert (got_i == want_i).all() and (got_d.view(np.uint32) == want_d.view(np.uint32)).all(), (name, n_landmarks, seed, k)


def test_header_is_c99_and_symbols_are_exported(tmp_path):
    src = tmp_path / "c.c"
    src.write_text('#include <cuvs_amd/ball_cover.h>\nint main(void) { return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])
    from cuvs_amd._lib import lib

    assert all(hasattr(lib(), s) for s in EXPORTS)
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "cuvs_amd", "libcuvs_c.so")], text=True)
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(EXPORTS) <= names
    declared = set()
    for line in open(os.path.join(ROOT, "include", "cuvs_amd", "ball_cover.h")):
        if "CUVS_EXPORT" in line:
            declared.add(line.split("(")[0].split()[-1])
    assert declared == set(EXPORTS)


def test_index_params_refuse_what_uint32_would_wrap():
    from cuvs_amd.neighbors import ball_cover

    for bad in (dict(n_landmarks=-1), dict(n_landmarks=2 ** 32), dict(seed=-1), dict(seed=2 ** 32), dict(n_landmarks=1.5), dict(seed="3")):
        with pytest.raises(ValueError, match="must be an integer in"):
            ball_cover.IndexParams(**bad)
    params = ball_cover.IndexParams(metric="haversine", n_landmarks=np.int64(7), seed=2 ** 32 - 1)
    p = params._p.contents
    assert (p.metric, p.n_landmarks, p.seed) == (13, 7, 2 ** 32 - 1)


def test_cpp_wrappers_compile(tmp_path):
    src = tmp_path / "w.cpp"
    src.write_text(
        "#include <cuvs_amd/neighbors.hpp>\n"
        "namespace bc = cuvs_amd::neighbors::ball_cover;\n"
        "void f(const cuvs::resources& r, cuvs::device_matrix_view<const float> x, cuvs::device_matrix_view<int64_t> n,\n"
        "       cuvs::device_matrix_view<float> d, cuvs::device_matrix_view<bool> adj, int64_t* v64, float* dist, int64_t* max_k) {\n"
        "  bc::index_params p;\n"
        "  p.metric = Haversine; p.n_landmarks = 10; p.seed = 3;\n"
        "  bc::index idx = bc::build(r, p, x);\n"
        "  bc::knn_query(r, idx, x, n, d);\n"
        "  bc::knn_query(r, idx, x, n, d, false, 0.5f);\n"
        "  bc::index idx2 = bc::all_knn_query(r, p, x, n, d);\n"
        "  bc::eps_nn(r, idx, x, adj, v64, 0.5f);\n"
        "  bc::eps_nn(r, idx, x, v64, (int64_t*)nullptr, (float*)nullptr, 0, v64, 0.5f);\n"
        "  bc::eps_nn(r, idx, x, v64, v64, dist, 100, (int64_t*)nullptr, 0.5f, max_k);\n"
        "  (void)(idx.n_landmarks() + idx.size() + idx.dim() + (int64_t)idx.metric() + (int64_t)bc::last_stats()[1]);\n"
        "}\nint main() { return 0; }\n")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_host_helper_under_the_sanitizers(tmp_path):
    exe = tmp_path / "ball_cover_host_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-I", os.path.join(ROOT, "cuvs_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "ball_cover_host_test.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ball cover host OK" in out.stdout
    # the host's landmark draw is the twin's
    for m, n, seed in ((1, 1, 0), (65, 8, 0), (3000, 54, 1), (400, 400, 2)):
        got = subprocess.run([str(exe), str(m), str(n), str(seed)], capture_output=True, text=True, timeout=300)
        assert got.returncode == 0 and [int(v) for v in got.stdout.split()] == R.landmarks(m, n, seed).tolist()
