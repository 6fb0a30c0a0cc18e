"""GPU: cuvsAmdSilhouetteScore, cuvsAmdNeighborRanks and cuvsAmdTrustworthinessScore (cuvs_amd/csrc/stats.hip) against the numpy
twin tests/stats_ref.py. Silhouette: the device and the twin round the same fp64 quantity once to fp32, up to the
summation order of the fp64 sums (at most 2 n 2^-53 relative), so the samples agree within one ulp below 1, 2^-23, and the means
within 4 n 2^-53. Ranks, penalties and trustworthiness scores are integers or formulas of integers: they are equal."""
import ctypes as C
import functools
import json
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

from tests import stats_ref as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SIL_SHAPES = [(3, 1, 2), (127, 3, 2), (128, 16, 5), (129, 17, 5), (257, 67, 7), (300, 128, 299), (4096, 16, 64)]
RANK_SHAPES = [(3, 1, 1), (127, 3, 5), (129, 17, 12), (257, 67, 64), (2048, 128, 15)]
ids = lambda c: "x".join(map(str, c))  # noqa: E731


def ST():
    from cuvs_amd import stats

    return stats


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()  # (a copy: the shared inputs are read-only)


@functools.lru_cache(maxsize=None)
def sil_distances(n, dim, metric):
    """the twin's distances of the shape's rows, computed once per arithmetic and shared"""
    if metric in (S.L2Unexpanded, S.L2SqrtUnexpanded):
        return sil_distances(n, dim, metric - 4)  # the same arithmetic as the expanded ids
    d = S.distances(S.uniform(n, dim, 7 * n + dim), metric)
    d.setflags(write=False)
    return d


def gpu_silhouette(x, y, n_labels, metric, res, batch=None, scores=True):
    """-> (scores fp32 on the host or None, mean); the output buffer holds garbage before the call"""
    buf = torch.full((x.shape[0],), float("nan"), dtype=torch.float32, device="cuda") if scores else None
    mean = ST().silhouette_score(x, y, n_labels, metric=metric, batch_size=batch, scores=buf, resources=res)
    res.sync()
    return (buf.cpu().numpy() if scores else None), mean


# ---------------------------------------------------------------------------------------------- 1: silhouette, bit level
@pytest.mark.parametrize("metric", S.SILHOUETTE_METRICS, ids=lambda m: "metric%d" % m)
@pytest.mark.parametrize("case", SIL_SHAPES, ids=ids)
def test_silhouette_pins_to_the_twin(res, case, metric):
    n, dim, n_labels = case
    x = S.uniform(n, dim, 7 * n + dim)
    d = sil_distances(n, dim, metric)
    dx = dev(x)
    for name, y in S.label_sets(n, n_labels, n).items():
        want, want_mean, _, _, _ = S.silhouette(x, y, n_labels, metric, d=d)
        got, mean = gpu_silhouette(dx, dev(y), n_labels, metric, res)
        err = np.abs(got.astype(np.float64) - want.astype(np.float64)).max()
        print(case, metric, name, "max |scores - twin| =", err, "|mean - twin| =", abs(mean - want_mean), "mean", mean)
        assert not np.isnan(got).any()  # the garbage is gone
        assert err <= 2.0 ** -23
        assert abs(mean - want_mean) <= 4 * n * 2.0 ** -53
        _, mean_only = gpu_silhouette(dx, dev(y), n_labels, metric, res, scores=False)
        assert mean_only == mean


def test_silhouette_with_more_labels_than_the_sort_keeps_in_lds(res):
    """beyond 4096 labels the cursors of the counting sort live in memory (sil_place_kernel<false>); n_labels = n - 1"""
    n, dim, n_labels = 4200, 3, 4199
    x = S.uniform(n, dim, 11)
    y = np.random.default_rng(12).integers(0, n_labels, n).astype(np.int32)
    want, want_mean, _, _, _ = S.silhouette(x, y, n_labels, S.L2Unexpanded)
    got, mean = gpu_silhouette(dev(x), dev(y), n_labels, S.L2Unexpanded, res)
    assert np.abs(got.astype(np.float64) - want.astype(np.float64)).max() <= 2.0 ** -23
    assert abs(mean - want_mean) <= 4 * n * 2.0 ** -53 and (want != 0).sum() > 1000


def test_label_sets_cover_the_edges():
    """what the label sets of the shapes above contain (no GPU work)"""
    e = S.label_sets(257, 7, 257)["edges"]
    cnt = np.bincount(e, minlength=7)
    assert cnt[0] == 128 and cnt[1] == 1 and cnt[2] == 0 and cnt.sum() == 257  # a boundary on the tile edge, a singleton, an empty label
    assert np.cumsum(cnt)[3] % 128 != 0                                         # a boundary inside a tile
    r = S.label_sets(300, 299, 300)["random"]
    cnt = np.bincount(r, minlength=299)
    assert (cnt == 0).any() and (cnt == 1).any() and (cnt > 1).any()
    assert (np.diff(S.label_sets(4096, 64, 4096)["sorted"]) >= 0).all() and (np.diff(S.label_sets(4096, 64, 4096)["reversed"]) <= 0).all()


# ---------------------------------------------------------------------------------------------- 2: the arithmetic
def test_the_chain_holds_where_the_expanded_form_moves(res):
    """tests/test_stats_cpu.py::test_expanded_form_moves_the_scores shows that the expanded fp32 form moves these samples by more
    than 2^-23; the device stays within it of the chain under every L2 id"""
    x, y, n_labels = S.near_ties()
    for metric in (S.L2Expanded, S.L2Unexpanded):
        want, want_mean, _, _, _ = S.silhouette(x, y, n_labels, metric)
        got, mean = gpu_silhouette(dev(x), dev(y), n_labels, metric, res)
        assert np.abs(got.astype(np.float64) - want.astype(np.float64)).max() <= 2.0 ** -23
        assert abs(mean - want_mean) <= 4 * len(x) * 2.0 ** -53


# ---------------------------------------------------------------------------------------------- 3: invariance
def test_silhouette_is_bit_identical_for_every_slab(res, monkeypatch):
    import cuvs_amd

    n, dim, n_labels = 257, 67, 7
    x, y = dev(S.uniform(n, dim, 7 * n + dim)), dev(S.label_sets(n, n_labels, n)["edges"])
    for metric in (S.L2SqrtUnexpanded, S.CosineExpanded):
        first = gpu_silhouette(x, y, n_labels, metric, res)
        st = ST().last_stats()
        assert st["slabs"] == 1 and st["tiles"] == 9 and st["straddling_or_passed"] > 0  # a straddling tile occurred
        again = gpu_silhouette(x, y, n_labels, metric, res)  # run to run
        assert first[0].tobytes() == again[0].tobytes() and first[1] == again[1]
        for batch, slabs in ((1, 257), (100, 3), (128, 3), (n, 1)):
            got = gpu_silhouette(x, y, n_labels, metric, res, batch=batch)
            assert ST().last_stats()["slabs"] == slabs
            assert got[0].tobytes() == first[0].tobytes() and got[1] == first[1], batch
    monkeypatch.setenv("CUVS_AMD_STATS_SLAB_ROWS", "64")
    forced = cuvs_amd.common.Resources()
    got = gpu_silhouette(x, y, n_labels, S.CosineExpanded, forced)
    assert ST().last_stats()["slabs"] == 5
    assert got[0].tobytes() == first[0].tobytes() and got[1] == first[1]


# ---------------------------------------------------------------------------------------------- 4: ranks
@functools.lru_cache(maxsize=None)
def rank_inputs(n, dim, k):
    """(x, {name: neighbors}): the true nearest rows, random rows and the farthest rows by (chain, index)"""
    x = S.uniform(n, dim, 3 * n + dim, -1.0, 1.0)
    v = S.chain(x, "sq").astype(np.float64)
    v[np.diag_indices(n)] = -1.0  # the row itself sorts first and is cut off
    order = np.argsort(v, axis=1, kind="stable")[:, 1:]
    rng = np.random.default_rng(n)
    rand = np.stack([rng.choice(order[i], k, replace=False) for i in range(n)])
    return x, dict(nearest=order[:, :k].copy(), random=rand, farthest=order[:, -k:].copy())


def gpu_ranks(x, nbr, res, ranks=True):
    buf = torch.full(tuple(nbr.shape), -77, dtype=torch.int32, device="cuda") if ranks else False
    out, penalty = ST().neighbor_ranks(x, nbr, ranks=buf, resources=res)
    res.sync()
    return (out.cpu().numpy() if ranks else None), penalty


@pytest.mark.parametrize("case", RANK_SHAPES, ids=ids)
def test_ranks_equal_the_twin(res, case):
    n, dim, k = case
    x, lists = rank_inputs(n, dim, k)
    dx = dev(x)
    for name, nbr in lists.items():
        want, want_penalty = S.neighbor_ranks(x, nbr)
        got, penalty = gpu_ranks(dx, dev(nbr), res)
        passed = ST().last_stats()["straddling_or_passed"]
        print(case, name, "ranks that differ:", int((got != want).sum()), "penalty", penalty, "want", want_penalty, "past the screen", passed)
        assert (got == want).all() and penalty == want_penalty
        if name == "nearest":  # every rank is at most k
            assert penalty == 0 and got.max() <= k and (np.sort(got, axis=1) == np.arange(1, k + 1)).all()
        if name == "farthest":  # every pair passes the screen
            assert passed == n * (n - 1) and got.max() == n - 1
        if name == "random" and n == 2048:
            assert got.max() > 1024  # the count spans many column tiles
        _, penalty_only = gpu_ranks(dx, dev(nbr), res, ranks=False)
        assert penalty_only == penalty


def test_ranks_integer_kat_with_duplicates(res, monkeypatch):
    import cuvs_amd

    x = S.int_kat(1)
    n = len(x)
    rng = np.random.default_rng(3)
    nbr = np.stack([rng.choice(np.delete(np.arange(n), i), 6, replace=False) for i in range(n)]).astype(np.int64)
    nbr[25, :3] = (3, 20, 29)
    nbr[26, :2] = (5, 5)  # the same id twice gets the same rank twice
    want, want_penalty = S.neighbor_ranks(x, nbr)
    assert list(want[25, :3]) == [1, 2, 10] and want[26, 0] == want[26, 1]
    got, penalty = gpu_ranks(dev(x), dev(nbr), res)
    assert (got == want).all() and penalty == want_penalty
    monkeypatch.setenv("CUVS_AMD_STATS_SLAB_ROWS", "50")  # three slabs
    forced = cuvs_amd.common.Resources()
    got, penalty = gpu_ranks(dev(x), dev(nbr), forced)
    assert ST().last_stats()["slabs"] == 3 and (got == want).all() and penalty == want_penalty


# ---------------------------------------------------------------------------------------------- 5: trustworthiness
@pytest.mark.parametrize("case", S.TRUST_CASES, ids=ids)
def test_trustworthiness_equals_the_twin(res, case):
    n, dim, dim_e, k, seed = case
    x, e = S.embedding(n, dim, dim_e, seed)
    want, t, nbr = S.trustworthiness(x, e, k)
    for metric in ("euclidean", "sqeuclidean", "l2_unexpanded", "l2_sqrt_unexpanded"):  # the ranks are on the squared chain
        got = ST().trustworthiness_score(dev(x), dev(e), n_neighbors=k, metric=metric, resources=res)
        print(case, metric, "score", got, "twin", want)
        assert got == want
    _, penalty = gpu_ranks(dev(x), dev(nbr), res, ranks=False)
    assert penalty == t


def test_trustworthiness_of_the_reference_inputs(res):
    fx = json.load(open(os.path.join(GOLDEN, "stats_trustworthiness_reference.json")))
    x = np.array(fx["X"], np.float32).reshape(fx["n"], fx["dim"])
    e = np.array(fx["X_embedded"], np.float32).reshape(fx["n"], fx["dim_embedded"])
    got = ST().trustworthiness_score(dev(x), dev(e), n_neighbors=fx["n_neighbors"], metric="l2_sqrt_unexpanded", resources=res)
    assert 0.9375 < got < 0.9379 and got == S.trustworthiness(x, e, 5)[0]


def test_trustworthiness_of_an_identity_embedding_is_one(res):
    """Integer rows in [0, 3): the expanded distances of the search and the chain of the ranks are both exact, and both break ties
    by the smaller index, so each row's 5 neighbours have the ranks 1 .. 5: the penalty is 0 and the score exactly 1.0.
    Duplicated rows exercise "drop the own id if present, else the last"."""
    x = dev(S.int_kat(1))
    assert ST().trustworthiness_score(x, x, n_neighbors=5, resources=res) == 1.0
    e = S.int_kat(2)
    want = S.trustworthiness(S.int_kat(1), e, 5)[0]
    assert ST().trustworthiness_score(x, dev(e), n_neighbors=5, resources=res) == want < 1.0


# ---------------------------------------------------------------------------------------------- 6: layers
def test_python_c_and_cpp_layers_agree(res, tmp_path):
    from cuvs_amd._lib import Tensor, lib

    n, dim, dim_e, n_labels, k, chunk = 300, 67, 2, 7, 5, 100
    x, e = S.embedding(n, dim, dim_e, 0)
    y = S.label_sets(n, n_labels, n)["edges"]
    nbr = rank_inputs(257, 67, 64)[1]["random"][:, :k].copy()
    nbr = np.concatenate([nbr, nbr[:43]]).astype(np.int64)  # 300 rows of ids below 257, none its own row
    nbr[257:] = (nbr[257:] + 1) % 257
    assert (nbr != np.arange(n)[:, None]).all()
    dx, de, dy, dn = dev(x), dev(e), dev(y), dev(nbr)
    # Python
    scores, mean = gpu_silhouette(dx, dy, n_labels, "l2_sqrt_unexpanded", res)
    samples = ST().silhouette_samples(dx, dy, metric="l2_sqrt_unexpanded", resources=res)  # n_unique_labels from labels.max() + 1
    assert samples.cpu().numpy().tobytes() == scores.tobytes()
    ranks, penalty = gpu_ranks(dx, dn, res)
    trust = ST().trustworthiness_score(dx, de, n_neighbors=k, resources=res)
    # C
    c_mean, c_pen, c_trust = C.c_double(0), C.c_uint64(0), C.c_double(0)
    c_scores = torch.zeros(n, dtype=torch.float32, device="cuda")
    c_ranks = torch.zeros((n, k), dtype=torch.int32, device="cuda")
    h = res.get_c_obj()
    assert lib().cuvsAmdSilhouetteScore(h, Tensor(dx).ptr, Tensor(dy).ptr, C.c_int64(n_labels), C.c_int(5), C.c_int64(chunk),
                                        Tensor(c_scores).ptr, C.byref(c_mean)) == 1
    assert lib().cuvsAmdNeighborRanks(h, Tensor(dx).ptr, Tensor(dn).ptr, Tensor(c_ranks).ptr, C.byref(c_pen)) == 1
    assert lib().cuvsAmdTrustworthinessScore(h, Tensor(dx).ptr, Tensor(de).ptr, C.c_int64(k), C.c_int(5), C.byref(c_trust)) == 1
    res.sync()
    assert c_mean.value == mean and c_scores.cpu().numpy().tobytes() == scores.tobytes()
    assert c_pen.value == penalty and (c_ranks.cpu().numpy() == ranks).all() and c_trust.value == trust
    # C++
    data = tmp_path / "inputs.bin"
    with open(data, "wb") as f:
        f.write(struct.pack("<6q", n, dim, dim_e, n_labels, k, chunk))
        for a in (x, e, y, nbr):
            f.write(np.ascontiguousarray(a).tobytes())
    exe = tmp_path / "stats_api_demo"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"),
                           "-I/opt/rocm/include", os.path.join(ROOT, "tests", "cpp", "stats_api_demo.cpp"), "-L",
                           os.path.join(ROOT, "cuvs_amd"), "-lcuvs_c", "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "cuvs_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)])
    out = subprocess.run([str(exe), str(data)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "stats api OK" in out.stdout, out.stdout + out.stderr
    said = dict(line.split(" ", 1) for line in out.stdout.splitlines() if " " in line)
    assert float.fromhex(said["silhouette"]) == mean
    assert float.fromhex(said["scores_sum"]) == float(np.cumsum(scores.astype(np.float64))[-1])
    assert int(said["penalty"]) == penalty and int(said["rank_sum"]) == int(ranks.sum())
    assert float.fromhex(said["trustworthiness"]) == trust
    assert "n_labels must be in [2, n - 1]" in said["refusal"]


# ---------------------------------------------------------------------------------------------- 7: refusals
def test_refusals_leave_the_outputs_untouched(res):
    from cuvs_amd._lib import CuvsError

    st = ST()
    n = 40
    x = torch.rand(n, 6, device="cuda")
    y = (torch.arange(n, device="cuda") % 4).to(torch.int32)
    scores = torch.full((n,), -5.0, dtype=torch.float32, device="cuda")

    def sil(match, X=x, labels=y, n_labels=4, metric="sqeuclidean", out=scores):
        with pytest.raises(CuvsError, match=match):
            st.silhouette_score(X, labels, n_labels, metric=metric, scores=out, resources=res)
        res.sync()
        assert (scores == -5.0).all()

    sil(r"n_labels must be in \[2, n - 1\]: n_labels is 1, n is 40", n_labels=1)
    sil(r"n_labels must be in \[2, n - 1\]: n_labels is 40", n_labels=40)
    bad = y.clone()
    bad[7], bad[9] = 4, -1
    sil(r"labels holds 2 values outside \[0, 4\)", labels=bad)
    sil("labels must be int32", labels=y.long())
    sil(r"labels must have shape \[40\]", labels=y[:39])
    sil("labels must be accessible on device memory", labels=y.cpu())
    sil("X must be fp32", X=x.double())
    sil("X must be fp32", X=x.half())
    sil("X must be row-major and contiguous", X=torch.rand(6, n, device="cuda").t())
    sil("X must be accessible on device memory", X=x.cpu())
    sil("X must be a 2-D matrix", X=x[:, 0].contiguous())
    sil("scores must be fp32", out=torch.zeros(n, dtype=torch.float64, device="cuda"))
    sil(r"scores must have shape \[40\]", out=torch.zeros(n + 1, dtype=torch.float32, device="cuda"))
    for metric in ("inner_product", "chebyshev", "hamming"):
        sil("is not supported by the silhouette score", metric=metric)
    # L1 is admitted here only: the pairwise distances keep refusing it
    assert np.isfinite(st.silhouette_score(x, y, 4, metric="l1", resources=res))

    nbr = torch.stack([(torch.arange(n, device="cuda") + s) % n for s in (1, 2, 3)], dim=1).contiguous()
    ranks = torch.full((n, 3), -9, dtype=torch.int32, device="cuda")

    def rk(match, X=x, neighbors=nbr, out=ranks):
        with pytest.raises(CuvsError, match=match):
            st.neighbor_ranks(X, neighbors, ranks=out, resources=res)
        res.sync()
        assert (ranks == -9).all()

    own = nbr.clone()
    own[11, 2] = 11
    rk("neighbors holds a row's own id", neighbors=own)
    far = nbr.clone()
    far[39, 0] = n
    rk(r"neighbors holds an id outside \[0, 40\)", neighbors=far)
    far[39, 0] = -1
    rk(r"neighbors holds an id outside \[0, 40\)", neighbors=far)
    wide = torch.zeros((200, 65), dtype=torch.int64, device="cuda")
    rk(r"k = 65 columns: k must be in \[1, 64\]", X=torch.rand(200, 6, device="cuda"), neighbors=wide)
    rk("neighbors must be int64", neighbors=nbr.to(torch.int32))
    rk(r"neighbors must have shape \[40, k\]", neighbors=nbr[:39])
    rk("ranks must be int32", out=torch.zeros((n, 3), dtype=torch.int64, device="cuda"))
    rk(r"ranks must have shape \[40, 3\]", out=torch.zeros((n, 4), dtype=torch.int32, device="cuda"))

    e = torch.rand(n, 2, device="cuda")
    for match, kw in (("must be less than n / 2", dict(n_neighbors=20)), ("at most 64", dict(n_neighbors=65)),
                      ("n_neighbors must be positive", dict(n_neighbors=0)),
                      ("is not supported by the trustworthiness score", dict(metric="cosine")),
                      ("is not supported by the trustworthiness score", dict(metric="l1"))):
        with pytest.raises(CuvsError, match=match):
            st.trustworthiness_score(x, e, resources=res, **kw)
    with pytest.raises(CuvsError, match="X_embedded has 39 rows, X has 40"):
        st.trustworthiness_score(x, e[:39], resources=res)
    with pytest.raises(CuvsError, match="X_embedded must be fp32"):
        st.trustworthiness_score(x, e.double(), resources=res)
    assert 0.0 < st.trustworthiness_score(x, e, n_neighbors=19, resources=res) <= 1.0
