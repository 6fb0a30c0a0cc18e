"""CPU: the numpy twin of cuvs_amd.stats (tests/stats_ref.py) against sklearn, the reference's own test inputs, the tie and
"drop self, else the last" rules on integer rows, the edge semantics, the C header and the exported symbols, and the host-only
helper under the sanitizers."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import stats_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
EXPORTS = ["cuvsAmdSilhouetteScore", "cuvsAmdNeighborRanks", "cuvsAmdTrustworthinessScore", "cuvsAmdStatsLastStats"]
SKLEARN_NAME = {S.L2Expanded: "sqeuclidean", S.L2Unexpanded: "sqeuclidean", S.L2SqrtExpanded: "euclidean", S.L2SqrtUnexpanded: "euclidean",
                S.L1: "manhattan", S.CosineExpanded: "cosine"}
SHAPES = [(257, 17, 5), (129, 3, 2), (300, 67, 7)]
ids = lambda c: "x".join(map(str, c))  # noqa: E731


# ---------------------------------------------------------------------------------------------- twin against sklearn
@pytest.mark.parametrize("case", SHAPES, ids=ids)
def test_silhouette_twin_against_sklearn(case):
    """One fp32 chain distance is within relative (dim + 2) 2^-24 of the exact one (dim roundings of the chain, one of the
    difference, one of the sqrt), so a and b are too, and s = (b - a) / max(a, b) moves by at most 4 (dim + 3) 2^-24; 2^-24 more
    for sklearn's own fp64 arithmetic, generously. Measured: at most 8.1e-8 against bounds of 1.5e-6 .. 1.7e-5."""
    from sklearn.metrics import silhouette_samples

    n, dim, n_labels = case
    x = S.uniform(n, dim, n)  # uniform [0, 100)
    y = S.label_sets(n, n_labels, n)["random"]
    bound = 4 * (dim + 3) * 2.0 ** -24 + 2.0 ** -24
    for metric in (S.L2Expanded, S.L2SqrtExpanded, S.L2Unexpanded, S.L2SqrtUnexpanded, S.L1):
        scores, mean, s, a, b = S.silhouette(x, y, n_labels, metric)
        want = silhouette_samples(x.astype(np.float64), y, metric=SKLEARN_NAME[metric])
        err = np.abs(s - want).max()
        print(case, metric, "max |s_twin - s_sklearn| =", err, "bound", bound)
        assert err <= bound
        assert abs(mean - want.mean()) <= bound and scores.dtype == np.float32
    # the expanded ids share the unexpanded arithmetic
    assert (S.distances(x, S.L2Expanded) == S.distances(x, S.L2Unexpanded)).all()
    assert (S.distances(x, S.L2SqrtExpanded) == S.distances(x, S.L2SqrtUnexpanded)).all()


@pytest.mark.parametrize("case", SHAPES, ids=ids)
def test_silhouette_twin_against_sklearn_cosine(case):
    """Cosine distances are 1 - c with an absolute error of (dim + 4) 2^-24 (the dot chain, two norms, product, quotient, the
    difference), so the bound is per sample: 4 (dim + 4) 2^-24 / max(a_i, b_i). Uniform positive rows keep max(a, b) above 0.05."""
    from sklearn.metrics import silhouette_samples

    n, dim, n_labels = case
    x = S.uniform(n, dim, n + 1, 0.0, 1.0)
    y = S.label_sets(n, n_labels, n)["random"]
    scores, mean, s, a, b = S.silhouette(x, y, n_labels, S.CosineExpanded)
    want = silhouette_samples(x.astype(np.float64), y, metric="cosine")
    assert np.maximum(a, b).min() > 0.05
    bound = 4 * (dim + 4) * 2.0 ** -24 / np.maximum(a, b)
    print(case, "max err / bound =", (np.abs(s - want) / bound).max())
    assert (np.abs(s - want) <= bound).all()


@pytest.mark.parametrize("case", S.TRUST_CASES, ids=ids)
def test_trustworthiness_twin_equals_sklearn(case):
    """The penalty is an integer, so the twin equals sklearn exactly wherever fp32 and fp64 order the rows alike: the seeds of
    TRUST_CASES were chosen by running this (seeds 0 .. 5 all agree at every shape). No tolerance."""
    from sklearn.manifold import trustworthiness

    n, dim, dim_e, k, seed = case
    x, e = S.embedding(n, dim, dim_e, seed)
    score, t, nbr = S.trustworthiness(x, e, k)
    want = trustworthiness(x.astype(np.float64), e.astype(np.float64), n_neighbors=k)
    print(case, "twin", score, "sklearn", want, "penalty", t)
    assert score == want and 0.4 < score < 0.9 and t > 0


def test_trustworthiness_rank_flip_illustration():
    """What the seeds avoid: at (257, 17 -> 3, k = 5), seed 27, one fp32-against-fp64 ordering differs by one place, and the
    scores differ by one unit of the penalty: 2 / (n k (2 n - 3 k - 1)) = 3.1e-6. The device follows the twin, not sklearn."""
    from sklearn.manifold import trustworthiness

    x, e = S.embedding(257, 17, 3, 27)
    score, t, _ = S.trustworthiness(x, e, 5)
    want = trustworthiness(x.astype(np.float64), e.astype(np.float64), n_neighbors=5)
    unit = 2.0 / (257 * 5 * (2 * 257 - 15 - 1))
    assert score != want and abs(abs(score - want) - unit) < 1e-12


# ---------------------------------------------------------------------------------------------- the reference's fixtures
def test_reference_trustworthiness_inputs():
    fx = json.load(open(os.path.join(GOLDEN, "stats_trustworthiness_reference.json")))
    x = np.array(fx["X"], np.float32).reshape(fx["n"], fx["dim"])
    e = np.array(fx["X_embedded"], np.float32).reshape(fx["n"], fx["dim_embedded"])
    assert x.shape == (50, 30) and e.shape == (50, 8) and fx["n_neighbors"] == 5 and fx["metric"] == "L2SqrtUnexpanded"
    score, t, _ = S.trustworthiness(x, e, 5)
    print("reference inputs: score", score, "penalty", t)
    assert fx["score_above"] == 0.9375 and fx["score_below"] == 0.9379
    assert 0.9375 < score < 0.9379  # trustworthiness.cu:343


def test_reference_silhouette_rows():
    """The parameter rows of the reference's silhouette test (its inputs come from a std:: engine, so only the rows are kept):
    every row is a legal call here, and the twin agrees with sklearn on data of the same kind within the reference's tolerance."""
    from sklearn.metrics import silhouette_score

    table = json.load(open(os.path.join(GOLDEN, "stats_silhouette_reference_table.json")))
    assert len(table["rows"]) == 7 and [r["line"] for r in table["rows"]] == list(range(206, 213))
    assert {r["metric"] for r in table["rows"]} == {"L2Expanded", "L2SqrtUnexpanded", "L2Unexpanded", "CosineExpanded", "L1"}
    for r in table["rows"]:
        n, dim, n_labels, metric = r["n"], r["dim"], r["labels"], S.METRIC_IDS[r["metric"]]
        assert 2 <= n_labels <= n - 1 and 1 <= r["chunk"] <= n
        rng = np.random.default_rng(n * dim * n_labels)
        x = (rng.random((n, dim)) * 100).astype(np.float32)
        y = rng.integers(0, n_labels, n).astype(np.int32)
        y[:2] = (0, 1)  # sklearn wants two labels
        _, mean, _, _, _ = S.silhouette(x, y, n_labels, metric)
        want = silhouette_score(x.astype(np.float64), y, metric=SKLEARN_NAME[metric])
        assert abs(mean - want) <= table["tolerance"], r


# ---------------------------------------------------------------------------------------------- integers: ties, duplicates
def test_integer_kat_ranks_follow_the_tie_rule():
    x = S.int_kat(1)
    n = len(x)
    v = S.chain(x, "sq")
    assert (v == np.rint(v)).all() and (v[20:30][:, 20:30] == 0).all()
    rng = np.random.default_rng(3)
    nbr = np.stack([rng.choice(np.delete(np.arange(n), i), 6, replace=False) for i in range(n)]).astype(np.int64)
    nbr[25, :3] = (3, 20, 29)  # duplicates of row 25 itself: distance 0, ranked by index
    ranks, penalty = S.neighbor_ranks(x, nbr)
    for i in range(n):  # a pure-Python sort of (distance, index) is the rule
        order = sorted((float(v[i, l]), l) for l in range(n) if l != i)
        place = {l: r + 1 for r, (_, l) in enumerate(order)}
        assert [place[j] for j in nbr[i]] == list(ranks[i])
    assert list(ranks[25, :3]) == [1, 2, 10]  # rows 3, 20 .. 24, 26 .. 29 are at distance 0 from row 25
    assert penalty == int(np.maximum(ranks - 6, 0).sum()) > 0
    ties = sum(len(set(v[i])) < n for i in range(n))
    assert ties == n  # every row has tied distances


def test_integer_kat_drop_self_else_the_last():
    e = S.int_kat(2)
    k = 5
    nbr = S.embedded_neighbors(e, k)
    n = len(e)
    assert ((nbr != np.arange(n)[:, None]).all()) and nbr.shape == (n, k)
    v = S.chain(e, "sq")
    in_list = []
    for i in range(n):  # the k + 1 nearest by (distance, index), the row itself among them at distance 0
        first = [l for _, l in sorted((float(v[i, l]), l) for l in range(n))][:k + 1]
        in_list.append(i in first)
        assert list(nbr[i]) == ([l for l in first if l != i] if i in first else first[:k])
    # row 22 has the copies 3, 20, 21 before it: its own id is in the list of 6 and is dropped
    assert in_list[22] and list(nbr[22][:3]) == [3, 20, 21]
    # row 29 has 3, 20 .. 28 before it: the list of 6 does not reach its own id, the last entry goes
    assert not in_list[29] and list(nbr[29]) == [3, 20, 21, 22, 23]
    # X_embedded = X on integer rows: the search and the ranks see the same exact distances and break ties alike
    x = S.int_kat(1)
    score, t, _ = S.trustworthiness(x, x, k)
    assert t == 0 and score == 1.0


# ---------------------------------------------------------------------------------------------- edge semantics
def test_twin_edge_semantics():
    x = np.array([[0.0], [1.0], [3.0], [7.0], [8.0]], np.float32)
    # a singleton scores 0; label 2 is empty and is skipped by the min
    y = np.array([0, 0, 1, 3, 3], np.int32)
    _, mean, s, a, b = S.silhouette(x, y, 4, S.L2SqrtUnexpanded)
    assert s[2] == 0.0
    assert a[0] == 1.0 and b[0] == 3.0 and s[0] == 2.0 / 3.0          # nearest other label: the singleton at 3
    assert a[3] == 1.0 and b[3] == 4.0 and s[3] == 0.75
    assert mean == float(np.cumsum(s)[-1] / 5)
    # a == b scores 0: row 1 is as far from its own row as from the other label
    x2 = np.array([[0.0], [2.0], [4.0], [4.0]], np.float32)
    _, _, s2, a2, b2 = S.silhouette(x2, np.array([0, 0, 1, 1], np.int32), 2, S.L1)
    assert a2[1] == b2[1] == 2.0 and s2[1] == 0.0 and s2[0] == 0.5
    # n_labels = n - 1: every row alone but one pair
    y3 = np.array([0, 1, 2, 3, 3], np.int32)
    _, _, s3, _, _ = S.silhouette(x, y3, 4, S.L2Unexpanded)
    assert (s3[:3] == 0.0).all() and s3[3] == (16.0 - 1.0) / 16.0
    # all rows under one label (legal when other labels are empty): no b, the score is 0
    _, mean4, s4, _, _ = S.silhouette(x, np.zeros(5, np.int32), 2, S.L2Unexpanded)
    assert (s4 == 0.0).all() and mean4 == 0.0


def test_expanded_form_moves_the_scores():
    """The arithmetic discriminator of the GPU test, shown here first: on rows with squared norms near 20 and distances below 1
    the expanded fp32 form moves some s_i by more than 2^-23, the bound the device is held to against the chain."""
    x, y, n_labels = S.near_ties()
    _, _, s, _, _ = S.silhouette(x, y, n_labels, S.L2Unexpanded)
    s_exp, _, _, _ = S.silhouette_from_distances(S.expanded_fp32(x), y, n_labels)
    moved = np.abs(s_exp - s) > 2.0 ** -23
    print("rows moved by the expanded form:", int(moved.sum()), "of", len(s), "largest", np.abs(s_exp - s).max())
    assert moved.sum() > len(s) // 10


def test_compiled_chain_is_the_numpy_chain():
    for kind in ("sq", "l1", "dot"):
        for n, dim, seed in ((150, 19, 3), (64, 1, 4), (33, 128, 5)):
            x = S.uniform(n, dim, seed, -3.0, 5.0)
            assert (S.chain_numpy(x, kind).view(np.uint32) == S.chain_compiled(x, kind).view(np.uint32)).all()


# ---------------------------------------------------------------------------------------------- header, exports, host helper
def test_header_is_c99_and_symbols_are_exported(tmp_path):
    src = tmp_path / "c.c"
    src.write_text('#include <cuvs_amd/stats.h>\nint main(void) { return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])
    from cuvs_amd._lib import lib

    assert all(hasattr(lib(), s) for s in EXPORTS)
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "cuvs_amd", "libcuvs_c.so")], text=True)
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(EXPORTS) <= names
    import cuvs_amd

    assert all(hasattr(cuvs_amd.stats, f) for f in ("silhouette_score", "silhouette_samples", "trustworthiness_score", "neighbor_ranks"))


def test_cpp_wrappers_compile(tmp_path):
    src = tmp_path / "w.cpp"
    src.write_text(
        "#include <cuvs_amd/stats.hpp>\n"
        "namespace st = cuvs::stats;\n"
        "double f(const cuvs::resources& r, cuvs::device_matrix_view<const float> x, cuvs::device_matrix_view<const float> e,\n"
        "         cuvs::device_matrix_view<const int64_t> nb, cuvs::device_matrix_view<int32_t> ranks, const int32_t* y, float* s) {\n"
        "  float a = st::silhouette_score(r, x, y, s, 5);\n"
        "  float b = st::silhouette_score_batched(r, x, y, nullptr, 5, 100, L1);\n"
        "  uint64_t t = st::neighbor_ranks(r, x, nb, ranks);\n"
        "  return a + b + (double)t + st::trustworthiness_score(r, x, e, 5) + st::silhouette_score_f64(r, x, y, s, 5);\n"
        "}\nint main() { return 0; }\n")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_host_helper_under_the_sanitizers(tmp_path):
    exe = tmp_path / "stats_host_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-I", os.path.join(ROOT, "cuvs_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "stats_host_test.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "stats host OK" in out.stdout
