"""Independent numpy restatement of the sparse (CSR) pairwise distances and of the sparse brute-force kNN, used
only by the tests. One fp32 accumulator per pair, a sequential chain over the columns in ascending order, with the exact fp32
fma of tests/ivf_sq_ref.py; vectorised over the pairs by looping over the columns. `prec=64` runs the same sets in double
arithmetic and also returns the sum of |term| of every pair (the error bounds of the transcendental metrics)."""
import numpy as np

from tests.ivf_sq_ref import fmaf

F32, F64 = np.float32, np.float64

# cuvsDistanceType
L2Expanded, L2SqrtExpanded, CosineExpanded, L1, L2Unexpanded, L2SqrtUnexpanded, InnerProduct, Linf, Canberra, LpUnexpanded = range(10)
CorrelationExpanded, JaccardExpanded, HellingerExpanded, Haversine, BrayCurtis, JensenShannon, HammingUnexpanded = range(10, 17)
KLDivergence, RusselRaoExpanded, DiceExpanded = 17, 18, 19

INTERSECTION = (InnerProduct, L2Expanded, L2SqrtExpanded, CosineExpanded, CorrelationExpanded, JaccardExpanded, DiceExpanded,
                RusselRaoExpanded, HellingerExpanded, KLDivergence)
UNION = (L1, L2Unexpanded, L2SqrtUnexpanded, Linf, Canberra, LpUnexpanded, HammingUnexpanded, JensenShannon)
SUPPORTED = INTERSECTION + UNION

SPLIT = 1024  # stored entries of a y row per chain segment (sparse_distance_host.hpp kSplit)


class Csr:
    """indptr int32 [rows + 1], indices int32 [nnz], data fp32 [nnz]"""

    def __init__(self, indptr, indices, data, n_cols):
        self.indptr = np.ascontiguousarray(indptr, np.int32)
        self.indices = np.ascontiguousarray(indices, np.int32)
        self.data = np.ascontiguousarray(data, F32)
        self.n_cols = int(n_cols)
        self.rows = len(self.indptr) - 1

    @staticmethod
    def from_dense(d):
        d = np.asarray(d, F32)
        indptr, indices, data = [0], [], []
        for row in d:
            nz = np.flatnonzero(row != 0)
            indices.extend(nz.tolist())
            data.extend(row[nz].tolist())
            indptr.append(len(indices))
        return Csr(indptr, indices, data, d.shape[1])

    def dense(self, dtype=F32):
        out = np.zeros((self.rows, self.n_cols), dtype)
        for r in range(self.rows):
            b, e = self.indptr[r], self.indptr[r + 1]
            out[r, self.indices[b:e]] = self.data[b:e]
        return out

    def slice(self, r0, r1):
        b, e = self.indptr[r0], self.indptr[r1]
        return Csr(self.indptr[r0:r1 + 1] - b, self.indices[b:e], self.data[b:e], self.n_cols)


def is_canonical(c):
    ip = c.indptr.astype(np.int64)
    if ip[0] != 0 or ip[-1] != len(c.indices) or (np.diff(ip) < 0).any():
        return False
    for r in range(c.rows):
        cols = c.indices[ip[r]:ip[r + 1]].astype(np.int64)
        if len(cols) and (cols[0] < 0 or cols[-1] >= c.n_cols or (np.diff(cols) <= 0).any()):
            return False
    return True


def row_stats(c):
    """sq = fmaf(v, v, sq), sum = sum + v, ones = number of v == 1.0f: chains over the stored entries in ascending order"""
    width = int(np.diff(c.indptr).max()) if c.rows else 0
    sq, sm, ones = np.zeros(c.rows, F32), np.zeros(c.rows, F32), np.zeros(c.rows, F32)
    start, cnt = c.indptr[:-1].astype(np.int64), np.diff(c.indptr)
    for t in range(width):
        on = cnt > t
        v = np.zeros(c.rows, F32)
        v[on] = c.data[start[on] + t]
        sq = np.where(on, fmaf(v, v, sq), sq)
        sm = np.where(on, sm + v, sm).astype(F32)
        ones = ones + (on & (v == 1)).astype(F32)
    return sq, sm, ones


# ---------------------------------------------------------------------------------------------- the terms of the chains
def _term(metric, p, prec, order="fma"):
    """term(a, b, acc) -> (new acc, |term|); a and b broadcast against acc"""
    T = F32 if prec == 32 else F64
    if prec == 32:
        fma = fmaf if order == "fma" else (lambda x, y, z: (x * y).astype(F32) + z)  # (multiply-then-add: a probe of the tests)
    else:
        fma = lambda x, y, z: x * y + z

    with np.errstate(all="ignore"):
        if metric in (InnerProduct, L2Expanded, L2SqrtExpanded, CosineExpanded, CorrelationExpanded, JaccardExpanded, DiceExpanded,
                      RusselRaoExpanded):
            return lambda a, b, acc: (fma(a, b, acc), np.abs(a * b))
        if metric == HellingerExpanded:
            return lambda a, b, acc: (fma(np.sqrt(a), np.sqrt(b), acc), np.abs(np.sqrt(a) * np.sqrt(b)))
        if metric == KLDivergence:
            def kl(a, b, acc):
                with np.errstate(all="ignore"):
                    lg = np.log((a / b).astype(T)).astype(T)
                    return fma(a, lg, acc), np.abs(a * lg)
            return kl
        if metric == L1:
            return lambda a, b, acc: ((acc + np.abs(a - b)).astype(T), np.abs(a - b) + 0 * acc)
        if metric in (L2Unexpanded, L2SqrtUnexpanded):
            def l2(a, b, acc):
                d = (a - b).astype(T)
                return fma(d, d, acc), d * d + 0 * acc
            return l2
        if metric == Linf:
            return lambda a, b, acc: (np.maximum(acc, np.abs(a - b)).astype(T), np.abs(a - b) + 0 * acc)
        if metric == Canberra:
            def canberra(a, b, acc):
                with np.errstate(all="ignore"):
                    d = (np.abs(a) + np.abs(b)).astype(T)
                    t = (((d != 0) * np.abs(a - b)).astype(T) / (d + (d == 0)).astype(T)).astype(T)
                    return (acc + t).astype(T), t + 0 * acc
            return canberra
        if metric == LpUnexpanded:
            pp = T(p)

            def lp(a, b, acc):
                t = np.power(np.abs(a - b).astype(T), pp).astype(T)
                return (acc + t).astype(T), t + 0 * acc
            return lp
        if metric == HammingUnexpanded:
            return lambda a, b, acc: ((acc + ((a != b) + 0 * acc)).astype(T), ((a != b) + 0 * acc))
        if metric == JensenShannon:
            def js(a, b, acc):
                with np.errstate(all="ignore"):
                    a, b = a + 0 * b, b + 0 * a
                    m = (T(0.5) * (a + b).astype(T)).astype(T)
                    az, bz = a == 0, b == 0
                    x = ((~az * m).astype(T) / (az + a).astype(T)).astype(T)
                    y = ((~bz * m).astype(T) / (bz + b).astype(T)).astype(T)
                    xz, yz = x == 0, y == 0
                    t1 = (-a * (~xz * np.log((x + xz).astype(T)).astype(T)).astype(T)).astype(T)
                    t2 = (-b * (~yz * np.log((y + yz).astype(T)).astype(T)).astype(T)).astype(T)
                    t = (t1 + t2).astype(T)
                    return (acc + t).astype(T), np.abs(t1) + np.abs(t2) + 0 * acc
            return js
    raise ValueError("metric %d is not a sparse metric" % metric)


def _combine(metric, total, seg):
    if metric == Linf:
        return np.maximum(total, seg)
    return (total + seg).astype(total.dtype)


def split_boundaries(y, split=SPLIT):
    """{column: rows of y whose chain segment ends after that column}: a row with more than `split` stored entries is cut
    after every `split`-th one; the last segment has no end"""
    out = {}
    for j in range(y.rows):
        b, e = int(y.indptr[j]), int(y.indptr[j + 1])
        for cut in range(b + split, e, split):
            out.setdefault(int(y.indices[cut - 1]), []).append(j)
    return out


def chains(x, y, metric, p=2.0, prec=32, order="fma", descending=False, split=SPLIT, count=None):
    """raw accumulators [m, n] of every pair (and the sums of |term|, fp64; `count`, an int64 [m, n] array of zeros, receives
    the number of terms of every chain): the chain over I or U in ascending column order,
    cut into segments by the long rows of y and combined in segment order"""
    T = F32 if prec == 32 else F64
    m, n = x.rows, y.rows
    term = _term(metric, p, prec, order)
    union = metric in UNION
    acc, total, mass = np.zeros((m, n), T), np.zeros((m, n), T), np.zeros((m, n), F64)
    first = np.ones(n, bool)  # no segment of the row has been folded yet
    cuts = split_boundaries(y, split) if not descending else {}

    def by_column(c):
        rows = np.repeat(np.arange(c.rows), np.diff(c.indptr))
        keep = c.data != 0  # a stored zero is an absent entry
        order_ = np.argsort(c.indices[keep], kind="stable")
        cols, rows, vals = c.indices[keep][order_], rows[keep][order_], c.data[keep][order_]
        uniq, start = np.unique(cols, return_index=True)
        return {int(u): (rows[s:e_], vals[s:e_].astype(T)) for u, s, e_ in zip(uniq, start, list(start[1:]) + [len(cols)])}

    xa, yb = by_column(x), by_column(y)
    columns = sorted(set(xa) | set(yb) | set(cuts), reverse=descending)
    none = (np.zeros(0, np.int64), np.zeros(0, T))
    with np.errstate(all="ignore"):
        for c in columns:
            ia, va = xa.get(c, none)
            jb, vb = yb.get(c, none)
            if len(ia) and len(jb):
                blk = np.ix_(ia, jb)
                acc[blk], t = term(va[:, None], vb[None, :], acc[blk])
                mass[blk] += t
                if count is not None:
                    count[blk] += 1
            if union:
                zero = T(0)
                if len(ia):
                    others = np.setdiff1d(np.arange(n), jb)
                    blk = np.ix_(ia, others)
                    acc[blk], t = term(va[:, None], zero, acc[blk])
                    mass[blk] += t
                    if count is not None:
                        count[blk] += 1
                if len(jb):
                    others = np.setdiff1d(np.arange(m), ia)
                    blk = np.ix_(others, jb)
                    acc[blk], t = term(zero, vb[None, :], acc[blk])
                    mass[blk] += t
                    if count is not None:
                        count[blk] += 1
            for j in cuts.get(c, ()):
                total[:, j] = acc[:, j] if first[j] else _combine(metric, total[:, j], acc[:, j])
                first[j] = False
                acc[:, j] = 0
        for j in range(n):
            total[:, j] = acc[:, j] if first[j] else _combine(metric, total[:, j], acc[:, j])
    return total, mass


def epilogue(metric, acc, sx, sy, n_cols, p=2.0, prec=32, diagonal=False):
    """acc [m, n] -> distances; sx and sy are the (sq, sum, ones) of the rows of x and y"""
    T = F32 if prec == 32 else F64
    one, zero = T(1), T(0)
    sqa, suma, onea = (v.astype(T)[:, None] for v in sx)
    sqb, sumb, oneb = (v.astype(T)[None, :] for v in sy)

    def clamp(v):
        return np.where(np.abs(v) < T(F32(1e-4)), zero, v).astype(T)

    with np.errstate(all="ignore"):
        if metric == InnerProduct:
            return acc
        if metric in (L2Expanded, L2SqrtExpanded):
            v = (((T(-2) * acc).astype(T) + sqa).astype(T) + sqb).astype(T)
            v = clamp(v)
            return v if metric == L2Expanded else np.sqrt(np.maximum(v, zero)).astype(T)
        if metric == CosineExpanded:
            norms = (np.sqrt(sqa).astype(T) * np.sqrt(sqb).astype(T)).astype(T)
            cos = (((norms != 0) * acc).astype(T) / ((norms == 0) + norms).astype(T)).astype(T)
            both = (sqa == 0) & (sqb == 0)
            return clamp((one - ((~both * cos).astype(T) + both).astype(T)).astype(T))
        if metric == CorrelationExpanded:
            nn = T(n_cols)
            numer = ((nn * acc).astype(T) - (suma * sumb).astype(T)).astype(T)
            qd = ((nn * sqa).astype(T) - (suma * suma).astype(T)).astype(T)
            rd = ((nn * sqb).astype(T) - (sumb * sumb).astype(T)).astype(T)
            return clamp((one - (numer / np.sqrt((qd * rd).astype(T)).astype(T)).astype(T)).astype(T))
        if metric == JaccardExpanded:
            un = (onea + oneb).astype(T)
            denom = (un - acc).astype(T)
            jacc = (((denom != 0) * acc).astype(T) / ((denom == 0) + denom).astype(T)).astype(T)
            both = un == 0
            return (one - ((~both * jacc).astype(T) + both).astype(T)).astype(T)
        if metric == DiceExpanded:
            un = (onea + oneb).astype(T)
            dice = ((T(2) * acc).astype(T) / un).astype(T)
            return np.where(un == 0, zero, (one - dice).astype(T)).astype(T)
        if metric == RusselRaoExpanded:
            inv = T(F32(1.0 / float(n_cols)))
            out = ((T(n_cols) - acc).astype(T) * inv).astype(T)
            if diagonal:
                k = min(out.shape)
                out[np.arange(k), np.arange(k)] = 0
            return out
        if metric == HellingerExpanded:
            r = (one - acc).astype(T)
            return np.where(r > 0, np.sqrt(np.where(r > 0, r, zero)), zero).astype(T)
        if metric == KLDivergence:
            return (T(0.5) * acc).astype(T)
        if metric in (L1, L2Unexpanded, Linf, Canberra):
            return acc
        if metric == L2SqrtUnexpanded:
            return np.sqrt(acc).astype(T)
        if metric == LpUnexpanded:
            return np.power(acc, (one / T(p)).astype(T)).astype(T)
        if metric == HammingUnexpanded:
            return (acc * T(F32(1.0 / float(n_cols)))).astype(T)
        if metric == JensenShannon:
            return np.sqrt((T(0.5) * acc).astype(T)).astype(T)
    raise ValueError("metric %d is not a sparse metric" % metric)


def pairwise(x, y, metric, p=2.0, prec=32, order="fma", descending=False, split=SPLIT, diagonal=True):
    assert x.n_cols == y.n_cols
    acc, _ = chains(x, y, metric, p, prec, order, descending, split)
    return epilogue(metric, acc, row_stats(x), row_stats(y), x.n_cols, p, prec, diagonal)


def pairwise64(x, y, metric, p=2.0, split=SPLIT, diagonal=True, count=None):
    """(fp64 distances, fp64 raw chain, sum of |term|) of every pair; `count` as in chains()"""
    acc, mass = chains(x, y, metric, p, 64, split=split, count=count)
    out = epilogue(metric, acc, row_stats(x), row_stats(y), x.n_cols, p, 64, diagonal)
    return out, acc, mass


def knn(queries, index, k, metric, p=2.0):
    """ids and distances of the k best index rows of every query: ascending (distance, id), inner product descending by
    distance; no RusselRao diagonal"""
    d = pairwise(queries, index, metric, p, diagonal=False)
    key = -d if metric == InnerProduct else d
    ids = np.lexsort((np.broadcast_to(np.arange(index.rows), d.shape), key), axis=1)[:, :k]
    return ids.astype(np.int64), np.take_along_axis(d, ids, axis=1)


# ---------------------------------------------------------------------------------------------- test inputs
def random_csr(rng, rows, n_cols, density, binary=False, empty_rows=(), stored_zeros=0, duplicate=(), full_rows=(), long_rows=()):
    """a canonical CSR matrix: `empty_rows` hold nothing, `duplicate` = (dst, src) pairs of equal rows, `full_rows` hold every
    column, `long_rows` = (row, entries) rows with exactly that many; `stored_zeros` entries are overwritten with 0.0"""
    dense_mask = rng.random((rows, n_cols)) < density
    for r in empty_rows:
        dense_mask[r] = False
    for r in full_rows:
        dense_mask[r] = True
    for r, cnt in long_rows:
        dense_mask[r] = False
        dense_mask[r, rng.choice(n_cols, cnt, replace=False)] = True
    vals = np.ones((rows, n_cols), F32) if binary else (rng.random((rows, n_cols)).astype(F32) + F32(0.05))
    for dst, src in duplicate:
        dense_mask[dst], vals[dst] = dense_mask[src], vals[src]
    indptr = np.concatenate([[0], np.cumsum(dense_mask.sum(axis=1))]).astype(np.int32)
    rr, cc = np.nonzero(dense_mask)
    data = vals[rr, cc].astype(F32)
    if stored_zeros and len(data):
        data[rng.choice(len(data), min(stored_zeros, len(data)), replace=False)] = 0
    return Csr(indptr, cc.astype(np.int32), data, n_cols)


def random_wide_csr(rng, rows, n_cols, density):
    """the same for a matrix too wide to draw densely"""
    indptr, indices, data = [0], [], []
    for _ in range(rows):
        cnt = rng.binomial(n_cols, density)
        cols = np.sort(rng.choice(n_cols, cnt, replace=False))
        indices.extend(cols.tolist())
        data.extend((rng.random(cnt) + 0.05).tolist())
        indptr.append(len(indices))
    return Csr(indptr, indices, data, n_cols)
