"""Numpy restatement of cuvs_amd/csrc/vamana.hip: insert order, medoid, distance arithmetic, greedy search,
RobustPrune, the batched build, and byte writers for the three file layouts. Everything the device decides is decided here by
the same rule, so graphs are compared bit for bit.

Order: every list is sorted on (float_to_key(distance), id); for the non-negative distances of squared L2 the key order is the
order of the float's bit pattern, so a word here is `bits(distance) << 32 | id`."""
import struct

import numpy as np

INVALID = 0xFFFFFFFF
FLT_MAX = np.float32(np.finfo(np.float32).max)
MEAN_CHUNK = 1024
MASK64 = (1 << 64) - 1


# ---------------------------------------------------------------- parameters
class Params:
    def __init__(self, graph_degree=32, visited_size=64, vamana_iters=1.0, alpha=1.2, max_fraction=0.06, batch_base=2.0,
                 queue_size=127, reverse_batchsize=1000000):
        self.degree = int(graph_degree)
        v = int(visited_size)
        if v & (v - 1):  # rounded up by doubling from the degree
            power = self.degree
            while power < v:
                power <<= 1
            v = power
        self.visited = v
        self.iters = np.float32(vamana_iters)
        self.alpha = np.float32(alpha)
        self.max_fraction = np.float32(max_fraction)
        self.base = float(np.float32(batch_base))
        self.queue = max(int(queue_size), 1)
        self.reverse_batch = max(int(reverse_batchsize), 1)

    def max_batch(self, n):
        mb = np.float32(self.max_fraction * np.float32(n))
        if mb >= np.float32(n):
            return n
        return min(max(int(mb), 1), n)


# ---------------------------------------------------------------- insert order and medoid
def insert_order(n):
    """Fisher-Yates from the back over xorshift64* seeded with 0x9E3779B97F4A7C15."""
    perm = list(range(n))
    x = 0x9E3779B97F4A7C15
    for i in range(n - 1, 0, -1):
        x ^= x >> 12
        x ^= (x << 25) & MASK64
        x ^= x >> 27
        j = ((x * 0x2545F4914F6CDD1D) & MASK64) % (i + 1)
        perm[i], perm[j] = perm[j], perm[i]
    return np.array(perm, dtype=np.uint32)


def column_mean(X):
    """fp64 column sums: the rows of a 1024-row chunk added in order, then the chunk sums added in order; rounded once."""
    n = X.shape[0]
    total = np.zeros(X.shape[1], dtype=np.float64)
    for r0 in range(0, n, MEAN_CHUNK):
        total = total + np.cumsum(X[r0:r0 + MEAN_CHUNK].astype(np.float32).astype(np.float64), axis=0)[-1]
    return (total / np.float64(n)).astype(np.float32)


def l2_to(X, rows, q):
    """The device's squared L2 of X[rows] to the float32 vector q: an 8-lane team, lane t owns the 16-byte pieces t, t + 8, ...
    and adds (x - q)^2 in element order (multiply and add rounded separately); the partial sums are combined as
    ((p0+p1)+(p2+p3))+((p4+p5)+(p6+p7))."""
    vl = 16 // X.dtype.itemsize
    x = X[np.asarray(rows, dtype=np.int64)].astype(np.float32)
    m, dim = x.shape
    if m == 0:
        return np.zeros(0, dtype=np.float32)
    t = x - q[None, :]
    sq = t * t
    pad = (-dim) % (8 * vl)
    if pad:
        sq = np.concatenate([sq, np.zeros((m, pad), dtype=np.float32)], axis=1)  # x + 0 = x: the lanes skip these
    sq = sq.reshape(m, -1, 8, vl).transpose(0, 2, 1, 3).reshape(m, 8, -1)
    p = np.cumsum(sq, axis=2, dtype=np.float32)[:, :, -1]
    p = p[:, 0::2] + p[:, 1::2]
    p = p[:, 0::2] + p[:, 1::2]
    return (p[:, 0] + p[:, 1]).astype(np.float32)


def medoid(X):
    d = l2_to(X, np.arange(X.shape[0]), column_mean(X))
    return int(np.lexsort((np.arange(X.shape[0]), d))[0])


def _bits(d):
    return np.asarray(d, dtype=np.float32).view(np.uint32).astype(np.uint64)


def _dist(word_hi):
    return np.asarray(word_hi, dtype=np.uint64).astype(np.uint32).view(np.float32)


# ---------------------------------------------------------------- greedy search
def greedy_search(X, graph, medoid_id, q, p):
    """The walk of row q over `graph` from the medoid. The list holds words bits(d) << 32 | id << 1 | pending. Each round expands
    the closest pending entry, appends its neighbours (scored), sorts, drops the later of two entries of one node, keeps the
    `queue` closest pending entries, and cuts the list at `visited`; it ends when nothing is pending or `visited` nodes have
    been expanded. Returns (ids, dists) [visited]: the expanded entries of the final list without q, padded."""
    n = X.shape[0]
    V = p.visited
    qf = X[q].astype(np.float32)
    lst = np.array([(_bits(l2_to(X, [medoid_id], qf))[0] << np.uint64(32)) | np.uint64(medoid_id << 1 | 1)], dtype=np.uint64)
    n_exp = 0
    while n_exp < V:
        pend = np.nonzero(lst & np.uint64(1))[0]
        if pend.size == 0:
            break
        pos = pend[0]
        node = int(lst[pos] >> np.uint64(1)) & 0x7FFFFFFF
        lst[pos] &= ~np.uint64(1)
        n_exp += 1
        nb = graph[node].astype(np.int64)
        nb = nb[nb < n]
        if nb.size:
            new = (_bits(l2_to(X, nb, qf)) << np.uint64(32)) | (nb.astype(np.uint64) << np.uint64(1)) | np.uint64(1)
            lst = np.sort(np.concatenate([lst, new]))
        first = np.ones(lst.size, dtype=bool)
        first[1:] = (lst[1:] >> np.uint64(1)) != (lst[:-1] >> np.uint64(1))
        lst = lst[first]
        pending = (lst & np.uint64(1)) != 0
        rank = np.cumsum(pending) - pending
        lst = lst[~pending | (rank < p.queue)][:V]
    ids = ((lst >> np.uint64(1)) & np.uint64(0x7FFFFFFF)).astype(np.uint32)
    keep = ((lst & np.uint64(1)) == 0) & (ids != q)
    out_ids = np.full(V, INVALID, dtype=np.uint32)
    out_d = np.full(V, FLT_MAX, dtype=np.float32)
    k = int(keep.sum())
    out_ids[:k] = ids[keep]
    out_d[:k] = _dist(lst[keep] >> np.uint64(32))
    return out_ids, out_d


# ---------------------------------------------------------------- RobustPrune
def robust_prune(X, graph_row, node, cand_ids, cand_dists, p):
    """Pool = candidates + the node's adjacency (scored), without the node and without the later of two entries of one id, in
    (distance, id) order. A pool of more than `degree` entries is pruned in passes cur_alpha = 1, 1.2, ... <= alpha: a pass
    accepts the first entry that is neither accepted nor occluded beyond cur_alpha and raises the occlusion factor of every later
    live entry k (not accepted, factor <= alpha) to max(factor, d(node, k) / d(accepted, k)), FLT_MAX when d(accepted, k) is 0.
    Returns (ids, words) [degree] padded with INVALID / all ones."""
    n = X.shape[0]
    D = p.degree
    cand_ids = np.asarray(cand_ids, dtype=np.int64)
    ok = (cand_ids < n) & (cand_ids != node)
    pool = (_bits(np.asarray(cand_dists, dtype=np.float32)[ok]) << np.uint64(32)) | cand_ids[ok].astype(np.uint64)
    nb = graph_row.astype(np.int64)
    nb = nb[(nb < n) & (nb != node)]
    if nb.size:
        adj = (_bits(l2_to(X, nb, X[node].astype(np.float32))) << np.uint64(32)) | nb.astype(np.uint64)
        pool = np.concatenate([pool, adj])
    pool = np.sort(pool)
    ids = (pool & np.uint64(0xFFFFFFFF)).astype(np.int64)
    first = np.ones(pool.size, dtype=bool)
    first[1:] = ids[1:] != ids[:-1]
    pool, ids = pool[first], ids[first]
    if pool.size > D:
        dist = _dist(pool >> np.uint64(32))
        occ = np.zeros(pool.size, dtype=np.float32)
        n_acc = 0
        cur_alpha = np.float32(1.0)
        while cur_alpha <= p.alpha and n_acc < D:
            start = 0
            while n_acc < D:
                free = np.nonzero((occ[start:] >= 0) & (occ[start:] <= cur_alpha))[0]
                if free.size == 0:
                    break
                i = start + int(free[0])
                occ[i] = -1.0
                n_acc += 1
                start = i + 1
                if n_acc == D:
                    break
                live = np.nonzero((occ[i + 1:] >= 0) & (occ[i + 1:] <= p.alpha))[0] + i + 1
                if live.size:
                    djk = l2_to(X, ids[live], X[ids[i]].astype(np.float32))
                    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                        f = np.where(djk == 0, FLT_MAX, dist[live] / djk).astype(np.float32)
                    occ[live] = np.maximum(occ[live], f)
            cur_alpha = np.float32(np.float64(cur_alpha) * 1.2)
        pool = pool[occ == -1.0]
    out = np.full(D, INVALID, dtype=np.uint32)
    words = np.full(D, np.uint64(MASK64), dtype=np.uint64)
    out[:pool.size] = (pool & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    words[:pool.size] = pool
    return out, words


# ---------------------------------------------------------------- the batched build
def batches(n, p):
    """(start, size) of every insert batch: sizes grow by `base` from 1 to max_batch; a fractional vamana_iters is a partial
    second pass that starts at max_batch."""
    out = []
    iters = np.float32(p.iters)
    mb = p.max_batch(n)
    start, step = 0, 1
    while True:
        limit = int(float(iters) * n)
        if start >= limit:
            break
        if start + step > limit:
            step = limit - start
        if start + step > n:
            step = n - start
        out.append((start, step))
        start += step
        if start >= n:
            start = 0
            iters = np.float32(iters - np.float32(1.0))
            step = mb
        step = max(1, min(int(float(step) * p.base), mb))
    return out


def build(X, p):
    """Returns (graph uint32 [n, degree], medoid)."""
    n = X.shape[0]
    D = p.degree
    graph = np.full((n, D), INVALID, dtype=np.uint32)
    order = insert_order(n)
    med = medoid(X)
    for start, m in batches(n, p):
        rows = order[start:start + m]
        found = [greedy_search(X, graph, med, int(r), p) for r in rows]  # the graph is frozen for the batch
        edges = []
        for r, (ids, dists) in zip(rows, found):
            new_ids, words = robust_prune(X, graph[r], int(r), ids, dists, p)
            graph[r] = new_ids
            for w in words[new_ids != INVALID]:
                # (dst, key, src)
                edges.append((int(w) & 0xFFFFFFFF, int(w) >> 32, int(r)))
        edges.sort()
        i = 0
        while i < len(edges):
            dst = edges[i][0]
            j = i
            while j < len(edges) and edges[j][0] == dst:
                j += 1
            seg = edges[i:min(j, i + p.visited)]  # the closest `visited` sources of a destination
            c_ids = np.full(p.visited, INVALID, dtype=np.uint32)
            c_d = np.full(p.visited, FLT_MAX, dtype=np.float32)
            c_ids[:len(seg)] = [e[2] for e in seg]
            c_d[:len(seg)] = np.array([e[1] for e in seg], dtype=np.uint32).view(np.float32)
            graph[dst], _ = robust_prune(X, graph[dst], dst, c_ids, c_d, p)
            i = j
    return graph, med


# ---------------------------------------------------------------- graph checks and a beam search for recall
def check_graph(graph, n, dim, degree):
    """The conditions of the reference's CheckGraph plus well-formedness. Returns (max degree, edge fraction)."""
    valid = graph != INVALID
    counts = valid.sum(axis=1)
    assert (valid == (np.arange(graph.shape[1])[None, :] < counts[:, None])).all(), "an unused slot in front of a used one"
    assert (graph[valid] < n).all(), "an id beyond the rows"
    assert not (graph == np.arange(n, dtype=np.uint32)[:, None]).any(), "a self edge"
    for i in range(n):
        row = graph[i, :counts[i]]
        assert np.unique(row).size == row.size, f"a duplicate edge in row {i}"
    bound = min(degree, dim)
    return int(counts.max()), float(counts.sum()) / (n * bound)


def beam_search(X, graph, med, Q, k, width=64):
    """Best-first search of width `width` from the medoid, fp64 distances; ids [m, k]."""
    Xd = X.astype(np.float64)
    out = np.zeros((Q.shape[0], k), dtype=np.int64)
    for qi, q in enumerate(Q.astype(np.float64)):
        seen = {med}
        lst = [(float(((Xd[med] - q) ** 2).sum()), med, False)]
        while True:
            pos = next((i for i, e in enumerate(lst) if not e[2]), None)
            if pos is None:
                break
            d, node, _ = lst[pos]
            lst[pos] = (d, node, True)
            nb = [int(v) for v in graph[node] if v != INVALID and int(v) not in seen]
            seen.update(nb)
            if nb:
                dd = ((Xd[nb] - q) ** 2).sum(axis=1)
                lst = sorted(lst + [(float(a), b, False) for a, b in zip(dd, nb)])[:width]
        ids = [e[1] for e in lst[:k]]
        out[qi, :len(ids)] = ids
        out[qi, len(ids):] = -1
    return out


def recall(found, truth):
    return float(np.mean([len(set(f.tolist()) & set(t.tolist())) / len(t) for f, t in zip(found, truth)]))


# ---------------------------------------------------------------- file layouts
def _counts(graph):
    return (graph != INVALID).sum(axis=1)


def index_bytes(graph, med):
    """uint64 size, uint32 largest degree, uint32 medoid, uint64 0; per node uint32 count + ids."""
    counts = _counts(graph)
    body = b"".join(struct.pack("<I", int(c)) + graph[i, :c].astype("<u4").tobytes() for i, c in enumerate(counts))
    size = 24 + len(body)
    return struct.pack("<QIIQ", size, int(counts.max()) if len(counts) else 0, int(med), 0) + body


def data_bytes(X):
    return struct.pack("<ii", X.shape[0], X.shape[1]) + np.ascontiguousarray(X).tobytes()


def disk_index_bytes(graph, med, X):
    """A 4096-byte sector of metadata (int32 9, int32 1, nine uint64), then the nodes (row, uint32 count, ids; node_len bytes
    each) packed per sector, or every node at the start of its own run of sectors when node_len > 4096."""
    sector = 4096
    n, dim = X.shape
    counts = _counts(graph)
    max_degree = int(counts.max())
    row_bytes = dim * X.dtype.itemsize
    node_len = (max_degree + 1) * 4 + row_bytes
    per_sector = sector // node_len
    per_node = -(-node_len // sector)
    n_sectors = -(-n // per_sector) if per_sector > 0 else n * per_node
    size = (n_sectors + 1) * sector
    out = bytearray(size)
    out[0:8] = struct.pack("<ii", 9, 1)
    out[8:80] = struct.pack("<9Q", n, dim, int(med), node_len, per_sector, 0, 0, 0, size)
    for i in range(n):
        at = sector * (1 + i // per_sector) + (i % per_sector) * node_len if per_sector > 0 else sector * (1 + i * per_node)
        node = np.ascontiguousarray(X[i]).tobytes() + struct.pack("<I", int(counts[i])) + graph[i, :counts[i]].astype("<u4").tobytes()
        out[at:at + len(node)] = node
    return bytes(out)
