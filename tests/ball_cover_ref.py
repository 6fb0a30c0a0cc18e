"""Numpy twin of the random ball cover, used only by the tests. The contract, restated:

1. Distances. L2: acc = fmaf(d, d, acc) from 0 with d = a[t] - b[t], t ascending (the chain of 3.1t), then a correctly
   rounded sqrt. Haversine: the reference's formula in fp32, sin_0 = sin(0.5 (a0 - b0)), sin_1 = sin(0.5 (a1 - b1)),
   2 asin(sqrt(sin_0 sin_0 + cos(a0) cos(b0) sin_1 sin_1)), the products from the left. One function per metric serves
   the build, the landmark pass and the list scan. Every comparison is on (distance, id).
2. Build. Landmark l is the row with the l-th smallest (level_hash(seed, i), i): a function of (m, n_landmarks, seed).
   n_landmarks 0 is floor(sqrt(m)). A row goes to its nearest landmark by (distance, landmark); a list is sorted by
   (distance to the landmark, row id); R_radius is a list's last distance, 0 for an empty list, which is never visited.
3. Pass one: the k nearest landmarks by (distance, landmark), their lists in that order. Without post-filtering the
   top-k of those rows is the answer, padded with (INT64_MAX, FLT_MAX).
4. Pass two: with tau the k-th distance after pass one (inf when there is none) and bound = fmaf(c, tau, tau) + s, every
   other non-empty list l is visited, in ascending l, iff  weight * (fmaf(-c, dq, dq) - fmaf(c, rad, rad)) <= bound,
   dq the query's distance to landmark l, rad = R_radius[l]. Inside a visited list, with tau the current k-th distance,
   row p (distance dp to the landmark) is skipped iff  fmaf(-c, dq, dq) - fmaf(c, dp, dp) > bound  (a prefix of the list)
   or  fmaf(-c, dp, dp) - fmaf(c, dq, dq) > bound  (a suffix). c = 2^-17 and s = 0 for L2, c = 2^-8 and s = 2^-16 for
   Haversine.
5. eps_nn: pair (i, j) is inside iff the L2 chain's acc <= fp32(eps * eps); lists and rows are skipped by the same
   expressions with tau = eps.
"""
import numpy as np

from tests.eps_neighbors_ref import chain
from tests.hnsw_ref import level_hash
from tests.ivf_sq_ref import fmaf

F32, F64 = np.float32, np.float64
PAD_ID, PAD_DIST = np.iinfo(np.int64).max, np.finfo(F32).max
MARGIN = {"euclidean": F32(2.0 ** -17), "haversine": F32(2.0 ** -8)}
SLACK = {"euclidean": F32(0), "haversine": F32(2.0 ** -16)}


# ---------------------------------------------------------------------------------------------- distances
def l2(a, b):
    """fp32 [na, nb]"""
    return np.sqrt(chain(a, b))


def haversine(a, b, dtype=F32):
    """[na, nb] in `dtype`, the operations in the kernel's order"""
    a = np.asarray(a, F32).astype(dtype)
    b = np.asarray(b, F32).astype(dtype)
    half = dtype(0.5)
    sin_0 = np.sin(half * (a[:, 0][:, None] - b[:, 0][None, :]))
    sin_1 = np.sin(half * (a[:, 1][:, None] - b[:, 1][None, :]))
    rdist = sin_0 * sin_0 + np.cos(a[:, 0])[:, None] * np.cos(b[:, 0])[None, :] * sin_1 * sin_1
    out = dtype(2) * np.arcsin(np.sqrt(rdist))
    assert out.dtype == dtype
    return out


def dist(metric, a, b):
    return haversine(a, b) if metric == "haversine" else l2(a, b)


# ---------------------------------------------------------------------------------------------- build
def isqrt(m):
    r = int(np.sqrt(float(m)))
    while r * r > m:
        r -= 1
    while (r + 1) * (r + 1) <= m:
        r += 1
    return r


def landmarks(m, n_landmarks, seed):
    n = n_landmarks if n_landmarks > 0 else max(1, isqrt(m))
    i = np.arange(m, dtype=np.int64)
    return np.lexsort((i, level_hash(seed, i)))[:n].astype(np.int64)


def build(X, metric="euclidean", n_landmarks=0, seed=0, landmark_rows=None):
    X = np.ascontiguousarray(X, F32)
    m = X.shape[0]
    rows = landmarks(m, n_landmarks, seed) if landmark_rows is None else np.asarray(landmark_rows, np.int64)
    L = len(rows)
    R = X[rows]
    d = dist(metric, X, R)                      # [m, L]
    label = np.argmin(d, axis=1)                # the first minimum: (distance, landmark)
    dmin = d[np.arange(m), label]
    order = np.lexsort((np.arange(m), dmin, label))
    cols = order.astype(np.int64)
    indptr = np.zeros(L + 1, np.int64)
    indptr[1:] = np.cumsum(np.bincount(label, minlength=L))
    sd = dmin[order]
    radius = np.zeros(L, F32)
    for l in range(L):
        if indptr[l + 1] > indptr[l]:
            radius[l] = sd[indptr[l + 1] - 1]
    return dict(metric=metric, m=m, dim=X.shape[1], L=L, R_rows=rows, R=R, R_indptr=indptr, R_1nn_cols=cols, R_1nn_dists=sd,
                R_radius=radius, X_reordered=X[order])


# ---------------------------------------------------------------------------------------------- brute force
def brute(X, Q, k, metric="euclidean", d=None):
    """top-k under (distance, id) by a stable sort: (ids int64 [q, k], distances fp32 [q, k])"""
    d = dist(metric, Q, X) if d is None else d
    order = np.argsort(d, axis=1, kind="stable")[:, :k]
    return order.astype(np.int64), np.take_along_axis(d, order, axis=1)


# ---------------------------------------------------------------------------------------------- pruning expressions
def below(dq, dp, bound, c):
    return (fmaf(-c, dq, dq) - fmaf(c, dp, dp)) > bound


def beyond(dq, dp, bound, c):
    return (fmaf(-c, dp, dp) - fmaf(c, dq, dq)) > bound


def bound_of(c, t, s=F32(0)):
    """fmaf(c, t, t) + s; an infinite t stays infinite, as on the device"""
    return F32(np.inf) if np.isinf(t) else F32(fmaf(c, t, t) + s)


def window(sd, dq, bound, c):
    """[w0, w1) of a list's sorted distances; the expressions are monotone along the list"""
    lo = below(dq, sd, bound, c)
    hi = beyond(dq, sd, bound, c)
    assert (np.diff(lo.astype(np.int8)) <= 0).all() and (np.diff(hi.astype(np.int8)) >= 0).all()
    keep_lo = np.nonzero(~lo)[0]
    w0 = int(keep_lo[0]) if len(keep_lo) else len(sd)
    cut = np.nonzero(hi[w0:])[0]
    w1 = w0 + int(cut[0]) if len(cut) else len(sd)
    return w0, w1


# ---------------------------------------------------------------------------------------------- k-NN through the index
def knn(index, Q, k, post_filter=True, weight=1.0, c=None):
    """(ids [q, k], distances [q, k], stats): the search of the contract, one query at a time"""
    metric = index["metric"]
    s = SLACK[metric] if c is None else F32(0)
    c = MARGIN[metric] if c is None else F32(c)
    Q = np.ascontiguousarray(Q, F32)
    L, indptr, cols, sd, radius = index["L"], index["R_indptr"], index["R_1nn_cols"], index["R_1nn_dists"], index["R_radius"]
    assert 1 <= k <= L
    ids = np.full((len(Q), k), PAD_ID, np.int64)
    dd = np.full((len(Q), k), PAD_DIST, F32)
    stats = dict(lists_visited=0, points_scored=0, points_skipped=0)
    dqr_all = dist(metric, Q, index["R"])
    for qi in range(len(Q)):
        q, dqr = Q[qi:qi + 1], dqr_all[qi]
        best_d, best_i = np.zeros(0, F32), np.zeros(0, np.int64)

        def tau():
            return best_d[k - 1] if len(best_d) >= k else F32(np.inf)

        def scan(l):
            nonlocal best_d, best_i
            beg, end = indptr[l], indptr[l + 1]
            if end == beg:
                return
            t = tau()
            w0, w1 = window(sd[beg:end], dqr[l], bound_of(c, t, s), c)
            stats["lists_visited"] += 1
            stats["points_scored"] += w1 - w0
            stats["points_skipped"] += (end - beg) - (w1 - w0)
            d = dist(metric, q, index["X_reordered"][beg + w0:beg + w1])[0]
            best_d = np.concatenate([best_d, d])
            best_i = np.concatenate([best_i, cols[beg + w0:beg + w1]])
            o = np.lexsort((best_i, best_d))[:k]
            best_d, best_i = best_d[o], best_i[o]

        near = np.lexsort((np.arange(L), dqr))[:k]
        for l in near:
            scan(l)
        if post_filter:
            t1 = tau()
            bound = bound_of(c, t1, s)
            with np.errstate(invalid="ignore"):
                visit = F32(weight) * (fmaf(-c, dqr, dqr) - fmaf(c, radius, radius)) <= bound
            visit[near] = False
            visit &= indptr[1:] > indptr[:-1]
            for l in np.nonzero(visit)[0]:
                scan(l)
        ids[qi, :len(best_i)] = best_i
        dd[qi, :len(best_d)] = best_d
    return ids, dd, stats


# ---------------------------------------------------------------------------------------------- eps_nn through the index
def eps_adj(index, Q, eps, c=None):
    """bool [q, m] by the walk of the index (to be compared with member(chain(Q, X), fp32(eps * eps)))"""
    c = MARGIN["euclidean"] if c is None else F32(c)
    Q = np.ascontiguousarray(Q, F32)
    eps = F32(eps)
    eps2 = F32(eps * eps)
    bound = fmaf(c, eps, eps)
    indptr, cols, sd, radius = index["R_indptr"], index["R_1nn_cols"], index["R_1nn_dists"], index["R_radius"]
    adj = np.zeros((len(Q), index["m"]), bool)
    dqr_all = l2(Q, index["R"])
    stats = dict(lists_visited=0, points_scored=0, points_skipped=0)
    for qi in range(len(Q)):
        dqr = dqr_all[qi]
        visit = ~below(dqr, radius, bound, c) & (indptr[1:] > indptr[:-1])
        for l in np.nonzero(visit)[0]:
            beg, end = indptr[l], indptr[l + 1]
            w0, w1 = window(sd[beg:end], dqr[l], bound, c)
            stats["lists_visited"] += 1
            stats["points_scored"] += w1 - w0
            stats["points_skipped"] += (end - beg) - (w1 - w0)
            acc = chain(Q[qi:qi + 1], index["X_reordered"][beg + w0:beg + w1])[0]
            adj[qi, cols[beg + w0:beg + w1][acc <= eps2]] = True
    return adj, stats


# ---------------------------------------------------------------------------------------------- inputs
def lattice(dim, side):
    """every integer point of [0, side)^dim, shuffled: exact distances, hundreds of ties, 3-4-5 and 1-2-2 triples"""
    g = np.stack(np.meshgrid(*[np.arange(side)] * dim, indexing="ij"), axis=-1).reshape(-1, dim).astype(F32)
    return g[np.random.default_rng(dim * 1000 + side).permutation(len(g))]


def blobs(m, dim, seed, centers=25):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-10.0, 10.0, size=(centers, dim))
    return (c[rng.integers(0, centers, m)] + rng.normal(0.0, 0.3, size=(m, dim))).astype(F32)


def shell(m, n_q, dim, seed, radius=1.0):
    """(X, Q): the rows lie within a few ulp of `radius` around one of the queries (fp64 directions rounded to fp32), so each
    query sees m / n_q near-ties at its k-th distance; further queries sit exactly at the boundary of those shells"""
    rng = np.random.default_rng(seed)
    Q = rng.uniform(-2.0, 2.0, size=(n_q, dim)).astype(F32)
    u = rng.standard_normal((m, dim))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    X = (Q[np.arange(m) % n_q].astype(F64) + radius * u).astype(F32)
    return X, np.concatenate([Q, X[:n_q]])


def duplicated(m, dim, seed):
    """30 % of the rows are copies of other rows: empty lists when two copies are drawn as landmarks, ties broken by id"""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1.0, 1.0, size=(m, dim)).astype(F32)
    dup = rng.choice(m, size=(3 * m) // 10, replace=False)
    X[dup] = X[rng.integers(0, m, len(dup))]
    return X


def geo(m, seed):
    """(latitude, longitude) in radians: blobs in degrees converted as the reference's test does, rows near a pole and rows
    on both sides of the +-pi longitude seam"""
    rng = np.random.default_rng(seed)
    c = np.stack([rng.uniform(-60, 60, 25), rng.uniform(-170, 170, 25)], axis=1)
    deg = c[rng.integers(0, 25, m)] + rng.normal(0.0, 1.0, size=(m, 2))
    n = m // 10
    deg[:n] = np.stack([rng.uniform(88.0, 89.9, n), rng.uniform(-180, 180, n)], axis=1)
    deg[n:2 * n] = np.stack([rng.uniform(-30, 30, n), np.where(rng.random(n) < 0.5, 1, -1) * rng.uniform(179.0, 179.999, n)], axis=1)
    return (deg * np.pi / 180.0).astype(F32)


def globe(m, n_q, seed):
    """(X, Q) in radians: rows all over the globe, so landmark balls are wide and lie up to half a turn from a query, where
    asin's argument is near 1 and the formula is least accurate. A third of the queries are antipodes of rows, a third sit
    on the +-pi seam, the rest are rows."""
    rng = np.random.default_rng(seed)
    X = (np.stack([rng.uniform(-89.0, 89.0, m), rng.uniform(-180.0, 180.0, m)], axis=1) * np.pi / 180.0).astype(F32)
    n = n_q // 3
    anti = np.stack([-X[:n, 0], np.where(X[:n, 1] > 0, X[:n, 1] - F32(np.pi), X[:n, 1] + F32(np.pi))], axis=1)
    seam = np.stack([rng.uniform(-1.4, 1.4, n), np.where(rng.random(n) < 0.5, 1, -1) * np.pi], axis=1)
    return X, np.concatenate([anti, seam, X[n:n_q - n]]).astype(F32)
