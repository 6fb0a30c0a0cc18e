"""Independent numpy restatement of single-linkage clustering, used only by the tests: the fp32 chain, the
edge weight, the total order on edges, Kruskal and Boruvka under that order, the dendrogram and the flat labels.

Everything here works on the full n x n weight matrix: the tests keep n small."""
import numpy as np

from tests.ivf_sq_ref import fmaf

F32 = np.float32
NO = np.uint64(0xFFFFFFFFFFFFFFFF)
SQRT_METRICS = (1, 5)
METRICS = {"sqeuclidean": 0, "euclidean": 1, "l2_unexpanded": 4, "l2_sqrt_unexpanded": 5}
PAIRWISE, KNN_GRAPH = 0, 1


def build_k(n, c):
    return min(n, max(2, int(np.floor(np.log2(n))) + c))


def chain(x):
    """acc = fmaf(d, d, acc) from 0, d = x[i][t] - x[j][t], t ascending: fp32 [n, n]"""
    x = np.asarray(x, F32)
    acc = np.zeros((x.shape[0], x.shape[0]), F32)
    for t in range(x.shape[1]):
        d = (x[:, None, t] - x[None, :, t]).astype(F32)
        acc = fmaf(d, d, acc)
    return acc


def weights(x, metric, core=None, alpha=1.0):
    """the edge weight of every pair: fp32 [n, n]"""
    d = chain(x)
    if metric in SQRT_METRICS:
        d = np.sqrt(d, dtype=F32)
    if core is None:
        return d
    core = np.asarray(core, F32)
    return np.fmax(core[:, None], np.fmax(core[None, :], (F32(alpha) * d).astype(F32))).astype(F32)


def bits(w):
    return np.ascontiguousarray(w, F32).view(np.uint32)


def sort_edges(src, dst, wbits):
    """ascending (bits(w), min, max); src < dst on return"""
    lo, hi = np.minimum(src, dst).astype(np.int64), np.maximum(src, dst).astype(np.int64)
    wbits = np.asarray(wbits, np.uint32)
    order = np.lexsort((hi, lo, wbits))
    return lo[order], hi[order], wbits[order]


def adjacency(ids, n):
    """the symmetrised, de-duplicated kNN graph without self entries: bool [n, n]"""
    adj = np.zeros((n, n), bool)
    for i in range(n):
        for j in ids[i]:
            if 0 <= j < n and j != i:
                adj[i, j] = adj[j, i] = True
    return adj


class _UF:
    def __init__(self, n):
        self.p = list(range(n))

    def find(self, v):
        while self.p[v] != v:
            self.p[v] = self.p[self.p[v]]
            v = self.p[v]
        return v

    def union(self, a, b):
        a, b = self.find(a), self.find(b)
        if a == b:
            return False
        self.p[max(a, b)] = min(a, b)
        return True


def kruskal(w, adj=None):
    """The tree by Kruskal: first the forest of `adj` (when given), then the complete graph over its components."""
    n = w.shape[0]
    wb = bits(w)
    uf = _UF(n)
    out = []
    iu, ju = np.triu_indices(n, 1)
    for allowed in ([adj] if adj is not None else []) + [None]:
        sel = np.ones(len(iu), bool) if allowed is None else allowed[iu, ju]
        s, d, b = sort_edges(iu[sel], ju[sel], wb[iu[sel], ju[sel]])
        for e in range(len(s)):
            if uf.union(int(s[e]), int(d[e])):
                out.append((int(s[e]), int(d[e]), int(b[e])))
    a = np.array(out, np.int64).reshape(-1, 3)
    return sort_edges(a[:, 0], a[:, 1], a[:, 2].astype(np.uint32))


def _boruvka_rounds(wb, color, allowed, out):
    """Rounds as the device runs them, until one component is left or no component has an edge. Returns the rounds that
    joined components."""
    n = wb.shape[0]
    ids = np.arange(n, dtype=np.uint64)
    key = (wb.astype(np.uint64) << np.uint64(32)) | ids[None, :]
    rounds = 0
    while len(set(color.tolist())) > 1:
        mask = color[:, None] != color[None, :]
        if allowed is not None:
            mask &= allowed
        row_best = np.where(mask, key, NO).min(axis=1)
        comp_w, comp_pair = {}, {}
        for i in range(n):
            if row_best[i] != NO:
                c = int(color[i])
                comp_w[c] = min(comp_w.get(c, 1 << 32), int(row_best[i]) >> 32)
        for i in range(n):
            if row_best[i] != NO and (int(row_best[i]) >> 32) == comp_w[int(color[i])]:
                j, c = int(row_best[i]) & 0xFFFFFFFF, int(color[i])
                pair = (min(i, j), max(i, j))
                comp_pair[c] = min(comp_pair.get(c, pair), pair)
        if not comp_pair:
            break
        parent = {int(c): int(c) for c in set(color.tolist())}
        for c, (a, b) in comp_pair.items():
            other = int(color[b]) if int(color[a]) == c else int(color[a])
            if comp_pair.get(other) == (a, b) and c < other:
                continue
            parent[c] = other
            out.append((a, b, comp_w[c]))

        def root(c):
            while parent[c] != c:
                c = parent[c]
            return c

        color[:] = [root(int(c)) for c in color]
        rounds += 1
    return rounds


def boruvka(w, adj=None):
    """The tree by Boruvka rounds, sparse over `adj` first (when given), then dense. Returns (src, dst, bits, stats) with
    stats = dict(edges, sparse_rounds, components, dense_rounds)."""
    n = w.shape[0]
    wb = bits(w)
    color = np.arange(n, dtype=np.int64)
    out = []
    stats = dict(edges=0, sparse_rounds=0, components=n, dense_rounds=0)
    if adj is not None:
        stats["edges"] = int(adj.sum()) // 2
        stats["sparse_rounds"] = _boruvka_rounds(wb, color, adj, out)
        stats["components"] = len(set(color.tolist()))
    stats["dense_rounds"] = _boruvka_rounds(wb, color, None, out)
    a = np.array(out, np.int64).reshape(-1, 3)
    s, d, b = sort_edges(a[:, 0], a[:, 1], a[:, 2].astype(np.uint32))
    return s, d, b, stats


def linkage(x, metric, ids=None, core=None, alpha=1.0):
    """(src, dst, weights fp32, stats): PAIRWISE without ids, else the kNN-graph linkage over those ids"""
    w = weights(x, metric, core, alpha)
    adj = adjacency(ids, len(x)) if ids is not None else None
    s, d, b, stats = boruvka(w, adj)
    return s, d, b.view(F32), stats


def dendrogram(src, dst, w):
    """children [m, 2], out_delta, out_size of the merges in the given order (the reference's build_dendrogram_host)"""
    m = len(src)
    n = m + 1
    parent = [-1] * (2 * n - 1)
    size = [1] * n + [0] * (n - 1)

    def find(v):
        while parent[v] != -1:
            v = parent[v]
        return v

    children = np.zeros((m, 2), np.int64)
    sizes = np.zeros(m, np.int64)
    for e in range(m):
        a, b = find(int(src[e])), find(int(dst[e]))
        assert a != b
        children[e] = (a, b)
        sizes[e] = size[a] + size[b]
        size[n + e] = sizes[e]
        parent[a] = parent[b] = n + e
    return children, np.asarray(w, F32).copy(), sizes


def flat_labels(children, n, n_clusters):
    """extract_flattened_clusters: the n_clusters smallest children of the last n_clusters - 1 merges, sorted descending,
    are the roots with labels 0, 1, ...; every leaf takes the label of the root above it"""
    if n_clusters == 1:
        return np.zeros(n, np.int64)
    tail = sorted(children[n - 1 - (n_clusters - 1):].ravel().tolist(), reverse=True)
    roots = tail[len(tail) - n_clusters:]
    label = {int(r): t for t, r in enumerate(roots)}
    up = {}
    for e in range(n - 1):
        up[int(children[e, 0])] = up[int(children[e, 1])] = n + e
    out = np.zeros(n, np.int64)
    for i in range(n):
        v = i
        while v not in label:
            v = up[v]
        out[i] = label[v]
    return out


def rand_index(a, b):
    a, b = np.asarray(a), np.asarray(b)
    same_a = a[:, None] == a[None, :]
    same_b = b[:, None] == b[None, :]
    iu = np.triu_indices(len(a), 1)
    return float((same_a[iu] == same_b[iu]).mean())


def same_partition(a, b):
    return len(a) < 2 or rand_index(a, b) == 1.0


# ---------------------------------------------------------------------------------------------- inputs
def uniform(n, dim, seed):
    return np.random.default_rng(seed).random((n, dim), dtype=F32)


def lattice(n, dim, seed):
    """small integers: massive ties"""
    return np.random.default_rng(seed).integers(0, 4, (n, dim)).astype(F32)


def duplicated(n, dim, seed):
    """every row several times"""
    rng = np.random.default_rng(seed)
    base = rng.random((max(1, n // 3), dim), dtype=F32)
    return base[rng.integers(0, len(base), n)]


def blobs(n_blobs, per_blob, dim, seed, spread=0.05, gap=10.0):
    """blobs farther apart than their diameter; rows shuffled"""
    rng = np.random.default_rng(seed)
    centers = (np.arange(n_blobs)[:, None] * gap * np.ones((1, dim))).astype(F32)
    x = np.concatenate([c + spread * rng.standard_normal((per_blob, dim)) for c in centers]).astype(F32)
    lab = np.repeat(np.arange(n_blobs), per_blob)
    perm = rng.permutation(len(x))
    return np.ascontiguousarray(x[perm]), lab[perm]
