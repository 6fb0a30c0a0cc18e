"""The numpy twin of cuvs_amd/csrc/hnsw_host.hpp: the level rule, the distances, the search, the insert and the
reader / writer of hnswlib's saveIndex layout, restated independently. Tests compare the library with it bit for bit.

File: a 96-byte header {u64 offset_level0 = 0, max_elements, cur_element_count, size_data_per_element, label_offset, offset_data;
i32 maxlevel, enterpoint; u64 maxM, maxM0, M; f64 mult; u64 ef_construction}, then per row the level-0 record {u32 count,
u32 links[maxM0], row, u64 label}, then per row {u32 bytes, bytes / (4 maxM + 4) blocks of {u32 count, u32 links[maxM]}}."""
import heapq
import math
import struct

import numpy as np

NONE, CPU, GPU = 0, 1, 2
L2, IP = 0, 6  # L2Expanded, InnerProduct
LEVEL_SEED = 100
BASE_SEEDS = 32
U32 = 0xFFFFFFFF


def level_hash(seed, i):
    x = (np.asarray(i, dtype=np.uint64) + np.uint64((seed * 0x9E3779B9) & U32)) & np.uint64(U32)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x85EBCA6B)) & np.uint64(U32)
    x ^= x >> np.uint64(13)
    x = (x * np.uint64(0xC2B2AE35)) & np.uint64(U32)
    x ^= x >> np.uint64(16)
    return x


def level_thresholds(M):
    out = []
    if M < 2:
        return out
    t = 4294967296.0
    while len(out) < 32:
        t = t / float(M)
        f = math.floor(t)
        if f < 1:
            break
        out.append(int(f))
    return out


def levels_of(ids, M):
    """level(i) = #{k >= 1 : h(i) < T_k}"""
    h = level_hash(LEVEL_SEED, ids)
    lv = np.zeros(h.shape, dtype=np.int32)
    for t in level_thresholds(M):
        lv += (h < np.uint64(t)).astype(np.int32)
    return lv


def _as_f32(a):
    return a.astype(np.float32)


class Index:
    def __init__(self, rows, metric, hierarchy):
        self.rows = np.ascontiguousarray(rows)
        self.metric, self.hierarchy = metric, hierarchy
        self.n, self.dim = self.rows.shape
        self.max_elements = self.n

    # ------------------------------------------------------------ construction
    @classmethod
    def from_graph(cls, rows, graph, metric, hierarchy, ef_construction=200):
        """What cuvsHnswFromCagra starts from: level 0 is `graph` [n, degree]; levels by the rule unless hierarchy is NONE
        (upper lists empty until build_cpu_hierarchy / set by the caller)."""
        ix = cls(rows, metric, hierarchy)
        n, deg = graph.shape
        if hierarchy == NONE:
            ix.M = ix.maxM = deg // 2
            ix.maxM0 = deg
            ix.mult, ix.ef_construction = 0.42424242, 500
            ix.maxlevel, ix.entry = 1, n // 2
            ix.levels = np.zeros(n, dtype=np.int32)
        else:
            ix.M = ix.maxM = (deg + 1) // 2
            ix.maxM0 = 2 * ix.M
            ix.mult = 1.0 / math.log(ix.M) if ix.M >= 2 else 0.0
            ix.ef_construction = ef_construction
            ix.levels = levels_of(np.arange(n), ix.M)
            ix._entry_from_levels()
        ix.l0 = np.zeros((n, ix.maxM0 + 1), dtype=np.uint32)
        ix.l0[:, 0] = deg
        ix.l0[:, 1:deg + 1] = graph
        ix.labels = np.arange(n, dtype=np.uint64)
        ix.upper = [np.zeros((int(l), ix.maxM + 1), dtype=np.uint32) for l in ix.levels]
        return ix

    def _entry_from_levels(self):
        self.maxlevel = int(self.levels.max())
        self.entry = int(np.nonzero(self.levels == self.maxlevel)[0][-1])

    # ------------------------------------------------------------ distances
    def dist_rows(self, q, ids):
        """distances of vector q to rows[ids]: fp32 / fp16 in fp32 summed in index order, int8 / uint8 in exact int32"""
        a = self.rows[np.asarray(ids, dtype=np.int64)]
        if self.rows.dtype.kind == "f":
            a, qf = _as_f32(a), _as_f32(q)
            if self.metric == L2:
                t = a - qf
                p = t * t
            else:
                p = a * qf
            s = np.cumsum(p, axis=1, dtype=np.float32)[:, -1]
            return s if self.metric == L2 else (np.float32(1) - s).astype(np.float32)
        a, qi = a.astype(np.int32), q.astype(np.int32)
        if self.metric == L2:
            t = a - qi
            return (t * t).sum(axis=1, dtype=np.int32).astype(np.float32)
        return (np.float32(1) - (a * qi).sum(axis=1, dtype=np.int32).astype(np.float32)).astype(np.float32)

    def dist(self, q, i):
        return float(self.dist_rows(q, [i])[0])

    def links(self, i, level):
        l = self.l0[i] if level == 0 else self.upper[i][level - 1]
        return l[1:1 + int(l[0])]

    def cap(self, level):
        return self.maxM0 if level == 0 else self.maxM

    def set_links(self, i, level, ids):
        l = self.l0[i] if level == 0 else self.upper[i][level - 1]
        l[:] = 0
        l[0] = len(ids)
        l[1:1 + len(ids)] = ids

    # ------------------------------------------------------------ search
    def greedy(self, q, level, cur, curd):
        changed = True
        while changed:
            changed = False
            ids = self.links(cur, level)
            if len(ids) == 0:
                break
            ds = self.dist_rows(q, ids)
            for c, d in zip(ids.tolist(), ds.tolist()):
                if d < curd:
                    curd, cur, changed = d, c, True
        return cur, curd

    def search_layer(self, q, ep, epd, ef, level):
        """best-first; every comparison on (distance, id); returns at most ef pairs, ascending"""
        visited = {ep}
        top = [(-epd, -ep)]  # max-heap
        cand = [(epd, ep)]
        while cand:
            c = cand[0]
            worst = (-top[0][0], -top[0][1])
            if len(top) >= ef and c > worst:
                break
            heapq.heappop(cand)
            ids = [e for e in self.links(c[1], level).tolist() if e not in visited]
            if not ids:
                continue
            # (a list holds an id once, so marking after the filter equals marking one by one)
            ds = self.dist_rows(q, ids).tolist()
            for e, d in zip(ids, ds):
                if e in visited:
                    continue
                visited.add(e)
                p = (d, e)
                if len(top) < ef or p < (-top[0][0], -top[0][1]):
                    heapq.heappush(cand, p)
                    heapq.heappush(top, (-d, -e))
                    if len(top) > ef:
                        heapq.heappop(top)
        return sorted((-a, -b) for a, b in top)

    def search_one(self, q, k, ef):
        cur = self.entry
        curd = self.dist(q, cur)
        if self.hierarchy == NONE:
            for i in range(BASE_SEEDS):
                s = i * (self.max_elements // BASE_SEEDS)
                if s >= self.n:
                    continue
                d = self.dist(q, s)
                if d < curd:
                    curd, cur = d, s
        else:
            for l in range(self.maxlevel, 0, -1):
                cur, curd = self.greedy(q, l, cur, curd)
        w = self.search_layer(q, cur, curd, max(ef, k), 0)
        ids = np.full(k, np.iinfo(np.uint64).max, dtype=np.uint64)
        ds = np.full(k, np.finfo(np.float32).max, dtype=np.float32)
        for j, (d, e) in enumerate(w[:k]):
            ids[j], ds[j] = self.labels[e], d
        return ids, ds

    def search(self, queries, k, ef):
        out = [self.search_one(q, k, ef) for q in queries]
        return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])

    # ------------------------------------------------------------ insert
    def heuristic(self, cands, cap):
        out = []
        for d, c in cands:
            if len(out) >= cap:
                break
            if out and bool((self.dist_rows(self.rows[c], out) < np.float32(d)).any()):
                continue
            out.append(c)
        return out

    def insert(self, q, min_level):
        L = int(self.levels[q])
        if self.maxlevel < 0:
            self.maxlevel, self.entry = L, q
            return
        qrow = self.rows[q]
        cur = self.entry
        curd = self.dist(qrow, cur)
        for l in range(self.maxlevel, L, -1):
            cur, curd = self.greedy(qrow, l, cur, curd)
        for l in range(min(L, self.maxlevel), min_level - 1, -1):
            w = self.search_layer(qrow, cur, curd, max(self.ef_construction, 1), l)
            sel = self.heuristic(w, self.M)
            self.set_links(q, l, sel)
            for nb in sel:
                cur_links = self.links(nb, l).tolist()
                if len(cur_links) < self.cap(l):
                    self.set_links(nb, l, cur_links + [q])
                    continue
                ds = self.dist_rows(self.rows[nb], cur_links + [q]).tolist()
                c = sorted(zip(ds, cur_links + [q]))
                self.set_links(nb, l, self.heuristic(c, self.cap(l)))
            curd, cur = w[0]
        if L >= self.maxlevel:
            self.maxlevel, self.entry = L, q

    def build_cpu_hierarchy(self):
        """rows of level >= 1 inserted into the levels >= 1 only, in id order (level 0 is given)"""
        self.maxlevel = -1
        for i in np.nonzero(self.levels >= 1)[0].tolist():
            self.insert(i, 1)
        if self.maxlevel < 0:
            self._entry_from_levels()

    def build_exact_hierarchy(self):
        """a stand-in for the GPU hierarchy: for every level the exact kNN (ascending (distance, id)) among its rows"""
        for l in range(self.maxlevel, 0, -1):
            ids = np.nonzero(self.levels >= l)[0]
            if len(ids) < 2:
                continue
            K = min(self.maxM, len(ids) - 1)
            for i in ids.tolist():
                others = ids[ids != i]
                ds = self.dist_rows(self.rows[i], others)
                order = np.lexsort((others, ds))[:K]
                self.set_links(i, l, others[order].tolist())

    def extend(self, more):
        assert self.hierarchy != NONE
        more = np.ascontiguousarray(more, dtype=self.rows.dtype)
        n0, m = self.n, more.shape[0]
        self.rows = np.concatenate([self.rows, more])
        self.n = n0 + m
        self.max_elements = max(self.max_elements, self.n)
        self.l0 = np.concatenate([self.l0, np.zeros((m, self.maxM0 + 1), dtype=np.uint32)])
        self.labels = np.arange(self.n, dtype=np.uint64)
        new_levels = levels_of(np.arange(n0, self.n), self.M)
        self.levels = np.concatenate([self.levels, new_levels])
        self.upper += [np.zeros((int(l), self.maxM + 1), dtype=np.uint32) for l in new_levels]
        for i in range(n0, self.n):
            self.insert(i, 0)

    # ------------------------------------------------------------ files
    def to_bytes(self):
        es = self.rows.dtype.itemsize
        offset_data = 4 * self.maxM0 + 4
        per = offset_data + self.dim * es + 8
        out = [struct.pack("<6Q2i3QdQ", 0, self.max_elements, self.n, per, per - 8, offset_data, self.maxlevel, self.entry,
                           self.maxM, self.maxM0, self.M, self.mult, self.ef_construction)]
        rec = np.zeros((self.n, per), dtype=np.uint8)
        rec[:, :offset_data] = self.l0.view(np.uint8).reshape(self.n, offset_data)
        rec[:, offset_data:per - 8] = self.rows.view(np.uint8).reshape(self.n, self.dim * es)
        rec[:, per - 8:] = self.labels.view(np.uint8).reshape(self.n, 8)
        out.append(rec.tobytes())
        for u in self.upper:
            out.append(struct.pack("<I", u.size * 4))
            out.append(u.tobytes())
        return b"".join(out)

    @classmethod
    def from_bytes(cls, blob, dim, dtype, metric, hierarchy):
        (z, max_el, n, per, label_off, offset_data, maxlevel, entry, maxM, maxM0, M, mult, efc) = struct.unpack_from("<6Q2i3QdQ", blob, 0)
        dtype = np.dtype(dtype)
        assert z == 0 and offset_data == 4 * maxM0 + 4 and per == offset_data + dim * dtype.itemsize + 8 and label_off == per - 8
        rec = np.frombuffer(blob, dtype=np.uint8, count=n * per, offset=96).reshape(n, per)
        rows = np.ascontiguousarray(rec[:, offset_data:per - 8]).view(dtype).reshape(n, dim)
        ix = cls(rows, metric, hierarchy)
        ix.max_elements, ix.maxlevel, ix.entry = max_el, maxlevel, entry
        ix.maxM, ix.maxM0, ix.M, ix.mult, ix.ef_construction = maxM, maxM0, M, mult, efc
        ix.l0 = np.ascontiguousarray(rec[:, :offset_data]).view(np.uint32).reshape(n, maxM0 + 1).copy()
        ix.labels = np.ascontiguousarray(rec[:, per - 8:]).view(np.uint64).reshape(n).copy()
        pos = 96 + n * per
        ix.upper, levels = [], []
        for _ in range(n):
            (b,) = struct.unpack_from("<I", blob, pos)
            pos += 4
            assert b % (4 * maxM + 4) == 0
            ix.upper.append(np.frombuffer(blob, dtype=np.uint32, count=b // 4, offset=pos).reshape(-1, maxM + 1).copy())
            levels.append(b // (4 * maxM + 4))
            pos += b
        assert pos == len(blob), "trailing bytes"
        ix.levels = np.asarray(levels, dtype=np.int32)
        return ix


def exact_knn_graph(rows, degree, metric):
    """level-0 graph for CPU tests: exact kNN, ascending (distance, id), self excluded"""
    ix = Index(rows, metric, NONE)
    n = rows.shape[0]
    g = np.zeros((n, degree), dtype=np.uint32)
    ids = np.arange(n)
    for i in range(n):
        ds = ix.dist_rows(rows[i], ids)
        ds[i] = np.inf
        g[i] = np.lexsort((ids, ds))[:degree]
    return g
