"""The numpy twin of the ScaNN search (cuvs_amd/csrc/scann_search.hip): the search-side lists, the approximate
scores in fp64 on the bf16-rounded operands, the dedupe rule, and the re-rank as exact fp32 fma chains. `a` is the dict of index
arrays the getters return: centers, labels, soar_labels, pq_codebook, codes, soar_codes and, for the re-rank, bf16."""
import numpy as np

from tests import scann_ref as R

L2, IP = "sqeuclidean", "inner_product"


def bf16(x):
    return R.bf16_value(R.bf16_rne_bits(np.asarray(x, np.float32))).astype(np.float32)


def lists(a):
    """(row, leaf, codes) of every entry, ordered by (leaf, row): one entry per row in its primary leaf with the primary codes, one
    more in its SOAR leaf with the SOAR codes where that leaf differs"""
    lab, soar = a["labels"].astype(np.int64), a["soar_labels"].astype(np.int64)
    two = soar != lab
    rows = np.concatenate([np.arange(len(lab)), np.flatnonzero(two)])
    leaf = np.concatenate([lab, soar[two]])
    codes = np.concatenate([a["codes"], a["soar_codes"][two]]).astype(np.int64)
    order = np.lexsort((rows, leaf))
    return rows[order], leaf[order], codes[order]


def decode(codebook, codes, pq_dim):
    """r~ [n_entries, dim]: the concatenation of the fp32 codebook entries the codes select"""
    d = np.arange(codebook.shape[1])
    return codebook[codes[:, d // pq_dim], d]


def entry_t(centers, leaf, rt):
    """t = 2 <centre, r~> + |r~|^2 in fp64"""
    c, r = centers[leaf].astype(np.float64), rt.astype(np.float64)
    return 2.0 * (c * r).sum(1) + (r * r).sum(1)


def coarse(q, centers, metric):
    """[m, n_leaves] fp64: |q - c|^2, or <q, c>"""
    q, c = q.astype(np.float64), centers.astype(np.float64)
    return ((q[:, None, :] - c[None]) ** 2).sum(2) if metric == L2 else q @ c.T


def entry_scores(q, a, metric, pq_dim):
    """(row, leaf, score, tol) with score and tol fp64 [m, n_entries]; tol = 2^-23 (dim + 8) (|base| + |t| + 2 sum |qb rb|)"""
    rows, leaf, codes = lists(a)
    rt = decode(a["pq_codebook"], codes, pq_dim)
    qb, rb = bf16(q).astype(np.float64), bf16(rt).astype(np.float64)
    dot, mass = qb @ rb.T, np.abs(qb) @ np.abs(rb).T
    base = coarse(q, a["centers"], metric)[:, leaf]
    t = entry_t(a["centers"], leaf, rt)[None, :] if metric == L2 else np.zeros((1, len(rows)))
    score = base + t - 2.0 * dot if metric == L2 else base + dot
    tol = 2.0 ** -23 * (q.shape[1] + 8) * (np.abs(base) + np.abs(t) + 2.0 * mass)
    return rows, leaf, score, tol


def row_scores(rows, key, tol, n_rows):
    """per query the best (lowest) key over a row's entries, and the largest tol among them: [m, n_rows]; rows without an entry inf"""
    best = np.full((key.shape[0], n_rows), np.inf)
    slack = np.zeros((key.shape[0], n_rows))
    for e, r in enumerate(rows):
        best[:, r] = np.minimum(best[:, r], key[:, e])
        slack[:, r] = np.maximum(slack[:, r], tol[:, e])
    return best, slack


def dedupe(rows, key, m):
    """one query: the best min(2 m, available) entries by (key, row), the first occurrence of every row, the first m of those"""
    order = np.lexsort((rows, key))[:2 * m]
    head = rows[order]
    _, first = np.unique(head, return_index=True)
    keep = np.sort(first)[:m]
    return head[keep], key[order][keep]


def rerank(q, bf16_bits, cand, metric, k):
    """one query: the fp32 chain over the bf16 rows widened to fp32, t ascending; the best k by (distance, row)"""
    x = R.bf16_value(bf16_bits[cand].view(np.uint16)).astype(np.float32)
    qq = np.broadcast_to(q.astype(np.float32), x.shape)
    d = R.chain(qq - x, qq - x) if metric == L2 else R.chain(qq, x)
    order = np.lexsort((cand, d if metric == L2 else -d))[:k]
    return cand[order], d[order]
