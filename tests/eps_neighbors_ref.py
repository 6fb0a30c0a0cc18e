"""Numpy twin of the epsilon-neighbourhood search, used only by the tests: membership of pair (i, j) is
acc <= eps, acc the fp32 chain acc = fmaf(d, d, acc) from 0 with d = x[i][t] - y[j][t] (one fp32 subtraction), t ascending,
one accumulator per pair. The fma is the exact one of tests/ivf_sq_ref.py. Inputs that sit on the radius are built here too."""
import functools

import numpy as np

from tests.ivf_sq_ref import fmaf

F32, F64 = np.float32, np.float64


def chain(x, y):
    """acc [m, n] fp32 of every pair; fp16 rows are widened first"""
    x = np.asarray(x).astype(F32)
    y = np.asarray(y).astype(F32)
    acc = np.zeros((x.shape[0], y.shape[0]), F32)
    for t in range(x.shape[1]):
        d = x[:, t][:, None] - y[:, t][None, :]  # fp32 - fp32: one rounding
        assert d.dtype == F32
        acc = fmaf(d, d, acc)
    return acc


def chain_pairs(x, y, rows, cols):
    """the chain of the listed pairs only"""
    x = np.asarray(x).astype(F32)[rows]
    y = np.asarray(y).astype(F32)[cols]
    acc = np.zeros(len(rows), F32)
    for t in range(x.shape[1]):
        d = x[:, t] - y[:, t]
        acc = fmaf(d, d, acc)
    return acc


def member(acc, eps):
    """bool [m, n]; NaN compares false"""
    with np.errstate(invalid="ignore"):
        return acc <= F32(eps)


def degrees(adj):
    """vd [m + 1]: row sums and the total"""
    d = adj.sum(axis=1).astype(np.int64)
    return np.concatenate([d, [d.sum()]])


def csr_of(adj, acc=None, max_k=None):
    """(indptr, indices[, distances]) with ascending column ids, at most max_k per row (the first ones)"""
    m = adj.shape[0]
    rows = [np.nonzero(adj[i])[0][:max_k] for i in range(m)]
    indptr = np.zeros(m + 1, np.int64)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    indices = np.concatenate(rows).astype(np.int64) if m else np.zeros(0, np.int64)
    if acc is None:
        return indptr, indices
    dist = np.concatenate([acc[i][r] for i, r in enumerate(rows)]).astype(F32) if m else np.zeros(0, F32)
    return indptr, indices, dist


# ---------------------------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def spheres(m, n, dim, seed):
    """x uniform in [0.1, 2), y[j] on the sphere of radius 0.5 around x[j % m] (fp64, rounded to fp32), eps the fp32 median of
    the chain over the pairs (j % m, j): those n pairs lie within a few ulp of eps, so any other arithmetic flips some.
    Returns (x, y, eps); the arrays are shared between tests and must not be written."""
    rng = np.random.default_rng(seed)
    x = (rng.random((m, dim)) * 1.9 + 0.1).astype(F32)
    u = rng.standard_normal((n, dim))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    own = np.arange(n) % m
    y = (x[own].astype(F64) + 0.5 * u).astype(F32)
    eps = F32(np.median(chain_pairs(x, y, own, np.arange(n))))
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y, eps


@functools.lru_cache(maxsize=None)
def spheres_twin(m, n, dim, seed):
    """(x, y, eps, acc, adj) of a spheres input, computed once"""
    x, y, eps = spheres(m, n, dim, seed)
    acc = chain(x, y)
    acc.setflags(write=False)
    adj = member(acc, eps)
    adj.setflags(write=False)
    return x, y, eps, acc, adj


def int_kat(seed, rows=130, dim=8):
    """integers in [0, 3): every value of the chain is exact in fp32 under any arithmetic, many pairs sit on the radius"""
    return np.random.default_rng(seed).integers(0, 3, size=(rows, dim)).astype(F32)


def blobs(n_row, n_col, n_centers, seed):
    """n_row / n_centers rows around each of n_centers centres (uniform in [-10, 10], standard deviation 0.01), shuffled.
    Returns (rows fp32, labels, centres)."""
    rng = np.random.default_rng(seed)
    centers = rng.uniform(-10.0, 10.0, size=(n_centers, n_col))
    labels = np.repeat(np.arange(n_centers), n_row // n_centers)
    assert len(labels) == n_row
    rng.shuffle(labels)
    rows = (centers[labels] + rng.normal(0.0, 0.01, size=(n_row, n_col))).astype(F32)
    return rows, labels, centers


def min_center_distance(centers):
    d = np.linalg.norm(centers[:, None, :] - centers[None, :, :], axis=2)
    d[np.diag_indices(len(centers))] = np.inf
    return float(d.min())
