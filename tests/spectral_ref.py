"""numpy twin of spectral embedding and spectral clustering (include/cuvs_amd/spectral.h): the connectivity
graph, the Laplacian in scipy's csgraph semantics, the hashed start vector, the thick-restart Lanczos iteration in float32,
the sign rule and the adjusted Rand index. The float32 sums run in numpy's order, not the device's: the GPU tests compare by
the bounds of the contract, never bit for bit, except for the graph (integers and the values 0.5 / 1.0)."""
import numpy as np

EPS32 = 2.0 ** -23
U32 = 2.0 ** -24
F32 = np.float32


# ---------------------------------------------------------------- the hash (cuvs_amd/csrc/mix_hash.hpp)
def mix_hash(seed, i):
    with np.errstate(over="ignore"):
        x = (np.asarray(i, np.uint32) + np.uint32(seed) * np.uint32(0x9E3779B9)).astype(np.uint32)
        x ^= x >> np.uint32(16)
        x = (x * np.uint32(0x85EBCA6B)).astype(np.uint32)
        x ^= x >> np.uint32(13)
        x = (x * np.uint32(0xC2B2AE35)).astype(np.uint32)
        x ^= x >> np.uint32(16)
    return x


def start_vector(seed, n, salt=0):
    """uniform [-1, 1): the top 24 bits of mix_hash(fold(seed) + salt, i), exact in float32"""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    fold = int(mix_hash(seed >> 32, np.uint32(seed & 0xFFFFFFFF)))
    h = mix_hash((fold + int(salt)) & 0xFFFFFFFF, np.arange(n, dtype=np.uint32))
    return ((h >> np.uint32(8)).astype(F32) * F32(2.0 ** -23) - F32(1.0)).astype(F32)


# ---------------------------------------------------------------- inputs
def uniform(n, dim, seed):
    return np.random.default_rng(seed).random((n, dim), dtype=F32)


def row_margins(x, k):
    """per row, the relative difference between the k-th and the (k + 1)-th smallest distance, the row itself counted"""
    x = x.astype(np.float64)
    sq = (x * x).sum(1)
    d = np.sqrt(np.maximum(sq[:, None] + sq[None, :] - 2.0 * x @ x.T, 0.0))
    d[np.arange(len(x)), np.arange(len(x))] = 0.0
    ds = np.sort(d, axis=1)
    return (ds[:, k] - ds[:, k - 1]) / ds[:, k]


def separated_uniform(n, dim, k, seed, margin=2e-4):
    """uniform rows, those whose k-th and (k + 1)-th neighbour are closer than `margin` (relative) drawn again until none is
    left: at these shapes plain uniform rows nearly always hold a few such rows, and their neighbour sets would hang on rounding"""
    rng = np.random.default_rng(seed)
    x = rng.random((n, dim), dtype=F32)
    for _ in range(200):
        bad = np.nonzero(row_margins(x, k) < margin)[0]
        if len(bad) == 0:
            return x
        x[bad] = rng.random((len(bad), dim), dtype=F32)
    raise AssertionError("no separated rows found")


def blobs(n, dim, n_clusters, std, seed):
    """rows i of cluster i % n_clusters around centres uniform in [-10, 10]"""
    rng = np.random.default_rng(seed)
    centers = rng.uniform(-10.0, 10.0, (n_clusters, dim))
    labels = np.arange(n) % n_clusters
    x = centers[labels] + std * rng.standard_normal((n, dim))
    return x.astype(F32), labels.astype(np.int32)


def knn_ids(x, k):
    """the k nearest rows of every row in float64, the row itself among them; and the smallest relative margin between a
    row's k-th and (k + 1)-th distance"""
    x = x.astype(np.float64)
    d = np.sqrt(np.maximum(((x[:, None, :] - x[None, :, :]) ** 2).sum(-1), 0.0)) if len(x) <= 600 else None
    if d is None:
        sq = (x * x).sum(1)
        d = np.sqrt(np.maximum(sq[:, None] + sq[None, :] - 2.0 * x @ x.T, 0.0))
        d[np.arange(len(x)), np.arange(len(x))] = 0.0
    order = np.argsort(d, axis=1, kind="stable")
    ds = np.take_along_axis(d, order, 1)
    margin = ((ds[:, k] - ds[:, k - 1]) / ds[:, k]).min() if k < len(x) else 1.0
    return order[:, :k], margin


def connectivity_graph(ids, n):
    """directed entries (i, ids[i][t]) of weight 1, symmetrised as 0.5 (a_ij + a_ji), sorted by (row, col), zeros dropped"""
    ids = np.asarray(ids, np.int64)
    k = ids.shape[1]
    src = np.repeat(np.arange(n, dtype=np.int64), k)
    dst = ids.reshape(-1)
    ok = (dst >= 0) & (dst < n)
    src, dst = src[ok], dst[ok]
    keys = np.concatenate([(src << 32) | dst, (dst << 32) | src])
    uniq, counts = np.unique(keys, return_counts=True)
    return (uniq >> 32).astype(np.int32), (uniq & 0xFFFFFFFF).astype(np.int32), (F32(0.5) * counts.astype(F32)).astype(F32)


def ring(n):
    i = np.arange(n)
    r = np.concatenate([i, (i + 1) % n])
    c = np.concatenate([(i + 1) % n, i])
    return r.astype(np.int32), c.astype(np.int32), np.ones(2 * n, F32), n


def path(n):
    i = np.arange(n - 1)
    r = np.concatenate([i, i + 1])
    c = np.concatenate([i + 1, i])
    return r.astype(np.int32), c.astype(np.int32), np.ones(2 * (n - 1), F32), n


def disjoint(*graphs):
    rows, cols, vals, base = [], [], [], 0
    for r, c, v, n in graphs:
        rows.append(r + base)
        cols.append(c + base)
        vals.append(v)
        base += n
    return np.concatenate(rows).astype(np.int32), np.concatenate(cols).astype(np.int32), np.concatenate(vals), base


def grid(a, b):
    idx = np.arange(a * b).reshape(a, b)
    e = np.concatenate([np.stack([idx[:, :-1].ravel(), idx[:, 1:].ravel()], 1), np.stack([idx[:-1].ravel(), idx[1:].ravel()], 1)])
    r = np.concatenate([e[:, 0], e[:, 1]])
    c = np.concatenate([e[:, 1], e[:, 0]])
    return r.astype(np.int32), c.astype(np.int32), np.ones(len(r), F32), a * b


def hub(n):
    """vertex 0 joined to every other vertex, the others also to their ring neighbour: one row of n - 1 entries, the rest 2 to 3"""
    i = np.arange(1, n)
    r1, c1 = np.zeros(n - 1, np.int64), i
    j = np.arange(1, n - 1)
    r = np.concatenate([r1, c1, j, j + 1])
    c = np.concatenate([c1, r1, j + 1, j])
    return r.astype(np.int32), c.astype(np.int32), np.ones(len(r), F32), n


def messy(n):
    """a ring with self-loops, duplicated entries (both directions, so it stays symmetric) and the isolated vertex n - 1"""
    r, c, v, _ = ring(n - 1)
    loops = np.arange(0, n - 1, 3, dtype=np.int32)
    dup = np.arange(0, n - 2, 2, dtype=np.int32)
    rows = np.concatenate([r, loops, dup, dup + 1, dup, dup + 1])
    cols = np.concatenate([c, loops, dup + 1, dup, dup + 1, dup])
    vals = np.concatenate([v, np.full(len(loops), 2.0, F32), np.full(2 * len(dup), 0.5, F32), np.full(2 * len(dup), 0.25, F32)])
    return rows.astype(np.int32), cols.astype(np.int32), vals.astype(F32), n


def complete(n):
    r, c = np.nonzero(~np.eye(n, dtype=bool))
    return r.astype(np.int32), c.astype(np.int32), np.ones(len(r), F32), n


def n_components(rows, cols, n):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components

    return connected_components(coo_matrix((np.ones(len(rows)), (rows, cols)), shape=(n, n)), directed=False)


# ---------------------------------------------------------------- the Laplacian
def dense_adjacency(rows, cols, vals, n):
    """float64 [n, n]: duplicates summed, the diagonal ignored"""
    w = np.zeros((n, n))
    np.add.at(w, (np.asarray(rows, np.int64), np.asarray(cols, np.int64)), np.asarray(vals, np.float64))
    w[np.arange(n), np.arange(n)] = 0.0
    return w


def laplacian(rows, cols, vals, n, norm):
    """(L float64 [n, n], scaling float64 [n]) in scipy.sparse.csgraph.laplacian's semantics; scaling is sqrt(deg) (1 for an
    isolated vertex) when normalised, deg otherwise"""
    w = dense_adjacency(rows, cols, vals, n)
    deg = w.sum(1)
    if not norm:
        return np.diag(deg) - w, deg
    dd = np.where(deg == 0, 1.0, np.sqrt(deg))
    lap = -w / dd[:, None] / dd[None, :]
    lap[np.arange(n), np.arange(n)] = np.where(deg == 0, 0.0, 1.0)
    return lap, dd


class Operator:
    """the solver's own float32 operator: off-diagonal values -w / sqrt(deg_i deg_j) (or -w) in CSR order, the diagonal apart"""

    def __init__(self, rows, cols, vals, n, norm):
        from scipy.sparse import csr_matrix

        rows, cols, vals = np.asarray(rows, np.int64), np.asarray(cols, np.int64), np.asarray(vals, F32)
        keep = rows != cols
        rows, cols, vals = rows[keep], cols[keep], vals[keep]
        order = np.argsort((rows << 32) | cols, kind="stable")
        rows, cols, vals = rows[order], cols[order], vals[order]
        deg = np.zeros(n, F32)
        for r, v in zip(rows, vals):  # in entry order, as a thread per row sums it
            deg[r] = F32(deg[r] + v)
        self.n, self.norm, self.deg = n, norm, deg
        if norm:
            self.dd = np.where(deg == 0, F32(1), np.sqrt(deg)).astype(F32)
            den = np.sqrt((deg[rows] * deg[cols]).astype(F32)).astype(F32)
            lv = (-vals / np.where(den == 0, F32(1), den)).astype(F32)
            self.diag = np.where(deg == 0, F32(0), F32(1)).astype(F32)
            self.scaling = self.dd
            self.scale = 2.0
        else:
            lv = (-vals).astype(F32)
            self.diag = deg.copy()
            self.scaling = deg
            self.scale = 2.0 * float(deg.max()) if n else 0.0
        self.m = csr_matrix((lv, (rows, cols)), shape=(n, n), dtype=F32)  # (sums duplicates; the device keeps them apart)

    def matvec(self, x):
        x = np.asarray(x, F32)
        return (self.m @ x + self.diag * x).astype(F32)


# ---------------------------------------------------------------- the solver
def ncv_rule(n, k):
    return max(min(n - k, max(2 * k + 1, 20)), k + 1)


def cgs2(v, u):
    """two passes of classical Gram-Schmidt of u against the rows of v in float32, then the normalisation"""
    u = np.asarray(u, F32).copy()
    for _ in range(2):
        if len(v):
            c = (v @ u).astype(F32)
            u = (u - v.T @ c).astype(F32)
    nrm = F32(np.sqrt(F32(np.dot(u, u))))
    return (u / nrm).astype(F32) if nrm > 0 else np.zeros_like(u), nrm


def eigsh(rows, cols, vals, n, norm, k, ncv=0, tol=1e-5, seed=0):
    """the k smallest eigenpairs of the Laplacian: (eigenvalues float32 ascending, vectors float32 [k, n], stats)"""
    op = Operator(rows, cols, vals, n, norm)
    m = ncv_rule(n, k) if ncv == 0 else ncv
    assert k < m <= n
    tol = EPS32 if (tol <= 0 or tol > EPS32) else tol  # (never above fp32 resolution: spectral_host.hpp stop_tolerance)
    thresh = 8.0 * EPS32 * op.scale
    cap = 10 * n
    v = np.zeros((m + 1, n), F32)
    v[0], _ = cgs2(v[:0], start_vector(seed, n, 0))
    l, theta, arrow = 0, np.zeros(0), np.zeros(0)
    matvecs = restarts = rescues = 0
    while True:
        m_end = min(m, l + cap - matvecs)
        alpha, beta = np.zeros(m), np.zeros(m + 1)
        for j in range(l, m_end):
            w = op.matvec(v[j])
            alpha[j] = F32(np.dot(v[j], w))
            v[j + 1], beta[j + 1] = cgs2(v[:j + 1], w)
            matvecs += 1
        m_eff, collapsed = m_end, False
        for j in range(l, m_end):
            if not beta[j + 1] > thresh:
                m_eff, collapsed = j + 1, True
                break
        t = np.zeros((m_eff, m_eff))
        for i in range(l):
            t[i, i] = theta[i]
            t[i, l] = t[l, i] = arrow[i]
        for j in range(l, m_eff):
            t[j, j] = alpha[j]
            if j + 1 < m_eff:
                t[j, j + 1] = t[j + 1, j] = beta[j + 1]
        evals, s = np.linalg.eigh(t)
        kk = min(k, m_eff)
        beta_last = 0.0 if collapsed else beta[m_eff]
        resid = np.abs(beta_last * s[m_eff - 1, :kk])
        converged = kk == k and ((not collapsed and resid.max() <= tol) or (collapsed and m_eff == n))
        x = (s[:, :kk].T @ v[:m_eff].astype(np.float64)).astype(F32)
        if converged or matvecs >= cap:
            assert kk == k
            return evals[:k].astype(F32), x, dict(matvecs=matvecs, restarts=restarts, ncv=m, converged=int(converged))
        nv = np.zeros_like(v)
        nv[:kk] = x
        if collapsed:
            rescues += 1
            nv[kk], _ = cgs2(nv[:kk], start_vector(seed, n, rescues))
            arrow = np.zeros(kk)
        else:
            nv[kk] = v[m_eff]
            arrow = beta_last * s[m_eff - 1, :kk]
        v, theta, l = nv, evals[:kk], kk
        restarts += 1


# ---------------------------------------------------------------- embedding
def sign_flip(emb):
    """every column's entry of largest magnitude becomes positive, the lowest index on ties"""
    emb = np.asarray(emb).copy()
    idx = np.argmax(np.abs(emb), axis=0)  # (argmax returns the first maximum)
    sign = np.where(emb[idx, np.arange(emb.shape[1])] < 0, -1, 1).astype(emb.dtype)
    return emb * sign[None, :]


def embedding(rows, cols, vals, n, n_comp, norm=True, drop_first=True, tol=1e-5, seed=0):
    evals, x, stats = eigsh(rows, cols, vals, n, norm, n_comp, 0, tol, seed)
    op = Operator(rows, cols, vals, n, norm)
    e = x.T.copy()
    if norm:
        e = (e / op.dd[:, None]).astype(F32)
    if drop_first:
        e = e[:, 1:]
    return sign_flip(e), evals, x, stats


# ---------------------------------------------------------------- criteria
def residuals(lap, evals, x):
    """||L v - lambda v||_2 per row of x, v normalised in float64"""
    v = x.astype(np.float64)
    v = v / np.linalg.norm(v, axis=1, keepdims=True)
    return np.linalg.norm(v @ lap.T - np.asarray(evals, np.float64)[:, None] * v, axis=1)


def subspace_sine(x, exact):
    """the largest sine between a vector of the row space of x [k, n] and the row space of exact [k2, n], k2 >= k: the norm of
    (I - P_exact) Q_x. For k2 = k this is the sine of the largest principal angle between the two spaces."""
    qx, _ = np.linalg.qr(x.astype(np.float64).T)
    qe, _ = np.linalg.qr(exact.astype(np.float64).T)
    return float(np.linalg.norm(qx - qe @ (qe.T @ qx), 2))


def cluster_end(evals, k, gap=1e-3):
    """the smallest k2 >= k with evals[k2] - evals[k2 - 1] >= gap: the end of the group of eigenvalues the k-th belongs to"""
    k2 = k
    while k2 < len(evals) and evals[k2] - evals[k2 - 1] < gap:
        k2 += 1
    return k2


def adjusted_rand_index(a, b):
    a, b = np.asarray(a), np.asarray(b)
    _, ai = np.unique(a, return_inverse=True)
    _, bi = np.unique(b, return_inverse=True)
    table = np.zeros((ai.max() + 1, bi.max() + 1), np.int64)
    np.add.at(table, (ai, bi), 1)
    comb = lambda v: v * (v - 1) / 2.0  # noqa: E731
    sum_ij = comb(table).sum()
    sum_a, sum_b = comb(table.sum(1)).sum(), comb(table.sum(0)).sum()
    expected = sum_a * sum_b / comb(len(a))
    max_index = 0.5 * (sum_a + sum_b)
    return 1.0 if max_index == expected else float((sum_ij - expected) / (max_index - expected))


# ---------------------------------------------------------------- the inputs the CPU and the GPU tests share
KNN_SHAPES = [(33, 3, 2), (257, 16, 10), (1000, 7, 15)]  # (n, dim, k)
KNN_SEEDS = {33: 1, 257: 1, 1000: 1}
# (n, dim, clusters, components, k, std, norm_laplacian, drop_first): rows 1, 3, 4, 5 and 2 of the reference's embedding test
TRANSFORM_SHAPES = [(100, 10, 3, 2, 10, 1.0, True, False), (100, 10, 3, 2, 10, 0.5, True, False), (100, 10, 3, 2, 10, 1.0, False, False),
                    (100, 10, 3, 2, 10, 1.0, True, True), (500, 20, 5, 3, 15, 1.0, True, False)]
# (n, dim, clusters = components, k, n_init, seed): the first three rows of the reference's clustering test, std 0.3
CLUSTER_SHAPES = [(100, 10, 2, 10, 3, 42), (200, 20, 3, 15, 3, 123), (500, 15, 4, 20, 3, 456)]
OVERLAP_SHAPE = (600, 10, 3, 12, 3, 7)  # std 2.5
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def knn_graph_case(n, dim, k):
    """(x, ids, margin, graph) of the uniform rows of a kNN shape"""
    def make():
        x = separated_uniform(n, dim, k, KNN_SEEDS[n])
        ids, margin = knn_ids(x, k)
        return x, ids, margin, connectivity_graph(ids, n) + (n,)
    return cached(("knn", n, dim, k), make)


def blobs_graph(n, dim, clusters, k, std, seed):
    def make():
        x, labels = blobs(n, dim, clusters, std, seed)
        ids, margin = knn_ids(x, k)
        return x, labels, margin, connectivity_graph(ids, n) + (n,)
    return cached(("blobs", n, dim, clusters, k, std, seed), make)


def solver_cases():
    """name -> (graph, norm_laplacian, k): graphs with known spectra and kNN graphs"""
    def make():
        three = disjoint(ring(60), ring(90), path(50))
        blob = blobs_graph(500, 15, 4, 20, 1.0, 1)[3]
        unif = cached(("unif500",), lambda: connectivity_graph(knn_ids(uniform(500, 3, 2), 10)[0], 500) + (500,))
        return {
            "ring200_unnorm": (ring(200), False, 5), "ring200_norm": (ring(200), True, 3),
            "three_unnorm": (three, False, 3), "three_norm": (three, True, 3),
            "grid_unnorm": (grid(20, 15), False, 4), "grid_norm": (grid(20, 15), True, 4),
            "blobs_norm": (blob, True, 4), "blobs_unnorm": (blob, False, 4),
            "uniform_norm": (unif, True, 4), "uniform_unnorm": (unif, False, 4),
        }
    return cached(("solver",), make)


def exact_spectrum(name):
    """(L float64, eigenvalues, eigenvectors as rows) of a solver case by numpy.linalg.eigh"""
    def make():
        (r, c, v, n), norm, _ = solver_cases()[name]
        lap, _ = laplacian(r, c, v, n, norm)
        ev, vec = np.linalg.eigh(lap)
        return lap, ev, vec.T.copy()
    return cached(("exact", name), make)


def arpack_residual(name, ncv):
    """the largest true residual scipy's eigsh (ARPACK) reaches in float32 on a solver case with the same ncv and tol = eps32"""
    def make():
        from scipy.sparse import csr_matrix
        from scipy.sparse.linalg import eigsh as arpack

        (r, c, v, n), norm, k = solver_cases()[name]
        lap, _, _ = exact_spectrum(name)
        w, vec = arpack(csr_matrix(lap.astype(F32)), k=k, which="SA", ncv=ncv, tol=EPS32, v0=start_vector(0, n).astype(F32))
        order = np.argsort(w)
        return float(residuals(lap, w[order], vec.T[order]).max())
    return cached(("arpack", name, ncv), make)
