"""Numpy twin of cuvs_amd.stats, used only by the tests. It restates the contract of include/cuvs_amd/stats.h
literally: the per-pair distances are fp32 chains (eps_neighbors_ref.chain and the exact fmaf of ivf_sq_ref.py), the sums S[i][c]
and everything after them are fp64. The order of the fp64 sums is numpy's, not the device's: the two differ by summation-order
noise only, which the bounds of tests/test_stats_gpu.py account for. The inputs of the tests are built here too."""
import ctypes
import functools
import os
import subprocess
import tempfile

import numpy as np

from tests import eps_neighbors_ref as E
from tests.ivf_sq_ref import fmaf

F32, F64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# cuvsDistanceType ids
L2Expanded, L2SqrtExpanded, CosineExpanded, L1, L2Unexpanded, L2SqrtUnexpanded = 0, 1, 2, 3, 4, 5
SILHOUETTE_METRICS = [L2Expanded, L2SqrtExpanded, CosineExpanded, L1, L2Unexpanded, L2SqrtUnexpanded]
METRIC_IDS = dict(L2Expanded=0, L2SqrtExpanded=1, CosineExpanded=2, L1=3, L2Unexpanded=4, L2SqrtUnexpanded=5)
CHAIN_OF = {0: "sq", 1: "sq", 4: "sq", 5: "sq", 3: "l1", 2: "dot"}


# ---------------------------------------------------------------------------------------------- chains
def chain_numpy(x, kind):
    """fp32 [n, n]: the chain of every pair of rows of x, t ascending, one rounding per operation"""
    x = np.asarray(x, F32)
    if kind == "sq":
        return E.chain(x, x)
    acc = np.zeros((x.shape[0], x.shape[0]), F32)
    for t in range(x.shape[1]):
        if kind == "l1":
            d = x[:, t][:, None] - x[:, t][None, :]
            acc = acc + np.abs(d)
        else:
            acc = fmaf(np.broadcast_to(x[:, t][:, None], acc.shape), np.broadcast_to(x[:, t][None, :], acc.shape), acc)
        assert acc.dtype == F32
    return acc


@functools.lru_cache(maxsize=None)
def _compiled():
    """tests/cpp/stats_chain.c as a shared library in a temporary directory"""
    out = os.path.join(tempfile.mkdtemp(prefix="stats_chain_"), "libstats_chain.so")
    subprocess.check_call(["gcc", "-O2", "-march=x86-64-v3", "-ffp-contract=off", "-fopenmp", "-shared", "-fPIC", "-std=c11",
                           os.path.join(ROOT, "tests", "cpp", "stats_chain.c"), "-o", out, "-lm"])
    lib = ctypes.CDLL(out)
    lib.stats_chain.restype = None
    return lib


def chain_compiled(x, kind):
    x = np.ascontiguousarray(x, F32)
    out = np.empty((x.shape[0], x.shape[0]), F32)
    _compiled().stats_chain(x.ctypes.data_as(ctypes.c_void_p), ctypes.c_int64(x.shape[0]), ctypes.c_int64(x.shape[1]),
                            ctypes.c_int(["sq", "l1", "dot"].index(kind)), out.ctypes.data_as(ctypes.c_void_p))
    return out


def chain(x, kind):
    """the numpy chain, or its compiled restatement (held to it bit for bit by test_stats_cpu.py) where numpy takes too long"""
    x = np.asarray(x, F32)
    return chain_numpy(x, kind) if x.shape[0] * x.shape[0] * max(x.shape[1], 1) <= (1 << 21) else chain_compiled(x, kind)


def distances(x, metric):
    """d(i, j) fp32 [n, n] of the contract"""
    x = np.asarray(x, F32)
    acc = chain(x, CHAIN_OF[metric])
    if metric in (L2SqrtExpanded, L2SqrtUnexpanded):
        return np.sqrt(acc)  # fp32 sqrt, correctly rounded
    if metric == CosineExpanded:
        nx = np.zeros(x.shape[0], F32)
        for t in range(x.shape[1]):
            nx = fmaf(x[:, t], x[:, t], nx)
        s = np.sqrt(nx)
        den = s[:, None] * s[None, :]
        assert den.dtype == F32
        with np.errstate(invalid="ignore", divide="ignore"):
            return (F32(1.0) - acc / den).astype(F32)
    return acc


# ---------------------------------------------------------------------------------------------- silhouette
def silhouette_from_distances(d, labels, n_labels):
    """(s fp64 [n], a, b, mean) from fp32 distances: S[i][c] in fp64 over j != i, then the formulas of stats.h"""
    labels = np.asarray(labels)
    n = len(labels)
    d64 = d.astype(F64)
    d64[np.diag_indices(n)] = 0.0  # the pair i == j is skipped
    cnt = np.bincount(labels, minlength=n_labels).astype(F64)
    order = np.argsort(labels, kind="stable")  # the columns of a label side by side, one sum per label that has a row
    present = np.nonzero(cnt)[0]
    starts = np.concatenate([[0], np.cumsum(cnt[present]).astype(np.int64)[:-1]])
    S = np.zeros((n, n_labels), F64)
    S[:, present] = np.add.reduceat(d64[:, order], starts, axis=1)
    own = cnt[labels]
    with np.errstate(invalid="ignore", divide="ignore"):
        a = S[np.arange(n), labels] / (own - 1.0)
        mean_other = S / cnt[None, :]
        mean_other[:, cnt == 0] = np.inf  # an empty label is skipped by the min
        mean_other[np.arange(n), labels] = np.inf
        b = np.fmin.reduce(mean_other, axis=1)
        s = (b - a) / np.maximum(a, b)
    s[(own == 1.0) | (a == b) | np.isinf(b)] = 0.0
    return s, a, b, float(np.cumsum(s)[-1] / n)  # the sum in index order


def silhouette(x, labels, n_labels, metric, d=None):
    """(scores fp32, mean, s fp64, a, b); `d`: distances(x, metric) computed before"""
    s, a, b, mean = silhouette_from_distances(distances(x, metric) if d is None else d, labels, n_labels)
    return s.astype(F32), mean, s, a, b


# ---------------------------------------------------------------------------------------------- ranks, trustworthiness
def neighbor_ranks(x, neighbors):
    """(ranks int32 [n, k], penalty_sum): ranks[i][q] = 1 + #{l != i, l != j: (v(i, l), l) < (v(i, j), j)}, j = neighbors[i][q]"""
    x = np.asarray(x, F32)
    neighbors = np.asarray(neighbors, np.int64)
    n, k = neighbors.shape
    v = chain(x, "sq")
    idx = np.arange(n)
    ranks = np.empty((n, k), np.int32)
    for q in range(k):
        j = neighbors[:, q]
        assert ((j >= 0) & (j < n) & (j != idx)).all()
        t = v[idx, j]
        before = (v < t[:, None]) | ((v == t[:, None]) & (idx[None, :] < j[:, None]))
        before[idx, idx] = False  # l != i (l == j is never before itself)
        ranks[:, q] = 1 + before.sum(axis=1)
    penalty = int(np.maximum(ranks.astype(np.int64) - k, 0).sum())
    return ranks, penalty


def embedded_neighbors(e, k):
    """the k nearest other rows of every row of e: the brute-force search at k + 1, the row's own id dropped if present, else the last"""
    import oracle

    _, knn = oracle.brute_force_knn(e, e, k + 1)
    out = np.empty((len(e), k), np.int64)
    for i in range(len(e)):
        row = [j for j in knn[i] if j != i]
        out[i] = row[:k]
    return out


def trustworthiness_formula(n, k, t):
    return 1.0 - ((2.0 / ((float(n) * k) * ((2.0 * n) - (3.0 * k) - 1.0))) * t)


def trustworthiness(x, e, k):
    """(score, penalty_sum, neighbors)"""
    nbr = embedded_neighbors(np.asarray(e, F32), k)
    _, t = neighbor_ranks(x, nbr)
    return trustworthiness_formula(len(x), k, t), t, nbr


# ---------------------------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def uniform(n, dim, seed, low=0.0, high=100.0):
    x = (np.random.default_rng(seed).random((n, dim)) * (high - low) + low).astype(F32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def label_sets(n, n_labels, seed):
    """{name: int32 labels}: random, the same sorted and reverse sorted, and (from n = 257 and 5 labels on) `edges`: label 0 holds
    exactly 128 rows (a boundary on a tile edge), label 1 is a singleton, label 2 is empty, the others share the rest (boundaries
    inside tiles); shuffled"""
    rng = np.random.default_rng(seed)
    rand = rng.integers(0, n_labels, n).astype(np.int32)
    out = dict(random=rand, sorted=np.sort(rand), reversed=np.sort(rand)[::-1].copy())
    if n >= 257 and n_labels >= 5:
        rest = n - 129
        others = n_labels - 3
        counts = [128, 1, 0] + [rest // others + (1 if r < rest % others else 0) for r in range(others)]
        edges = np.repeat(np.arange(n_labels), counts).astype(np.int32)
        assert len(edges) == n
        rng.shuffle(edges)
        out["edges"] = edges
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def near_ties(seed=16):
    """(x, labels, 8): the spheres of eps_neighbors_ref, 300 rows on spheres of radius 0.5 around 8 centres in [0.1, 2)^16, a
    centre's rows one label: distances of 0.25 .. 1 between rows whose squared norms are near 20, so the cancellation of the
    expanded form costs about two decimal digits"""
    _, y, _ = E.spheres(8, 300, 16, seed)
    labels = (np.arange(300) % 8).astype(np.int32)
    labels.setflags(write=False)
    return y, labels, 8


def expanded_fp32(x):
    """|x|^2 + |y|^2 - 2 x.y in fp32, clamped at 0: the arithmetic the contract refuses"""
    x = np.asarray(x, F32)
    xx = (x * x).sum(axis=1, dtype=F32)
    return np.maximum((xx[:, None] + xx[None, :] - F32(2) * (x @ x.T)).astype(F32), F32(0))


@functools.lru_cache(maxsize=None)
def embedding(n, dim, dim_e, seed):
    """x standard normal fp32, e = x @ P + 0.3 noise"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, dim)).astype(F32)
    p = rng.standard_normal((dim, dim_e))
    e = (x.astype(F64) @ p + 0.3 * rng.standard_normal((n, dim_e))).astype(F32)
    x.setflags(write=False)
    e.setflags(write=False)
    return x, e


# (n, dim, dim_e, k, seed): the twin equals sklearn.manifold.trustworthiness exactly at these seeds (test_stats_cpu.py)
TRUST_CASES = [(257, 17, 3, 5, 0), (130, 30, 8, 12, 0), (300, 67, 2, 1, 0)]


def int_kat(seed, rows=130, dim=8, copies=10):
    """eps_neighbors_ref.int_kat with duplicated rows: rows 20 .. 20 + copies - 1 are copies of row 3, rows 60 and 61 of row 7.
    Every chain value is an exact small integer under any arithmetic; ties are everywhere."""
    x = E.int_kat(seed, rows, dim).copy()
    x[20:20 + copies] = x[3]
    x[60:62] = x[7]
    return x
