"""CPU twin of the NN-descent steps (cuvs_amd/csrc/nn_descent.hip), restated from their definitions in numpy.

Not a test module: tests/test_nn_descent_cpu.py checks it against brute-force definitions, tests/test_nn_descent_steps_gpu.py
compares the kernels with it through the cuvsAmdNnDescentStep hook.

Conventions of the state (all uint32): a list entry is (id | NEW for an entry that arrived since the last sample, key);
an empty slot is (NONE, NONE); `key` is the order-preserving image of the fp32 distance (float_to_key); S = 32 samples.
"""
import ctypes as C

import numpy as np

import oracle

NEW = 0x80000000
NONE = 0xFFFFFFFF
S = 32
METRICS = ("sqeuclidean", "inner_product", "cosine", "bitwise_hamming")
_MODE = {"sqeuclidean": 0, "inner_product": 1, "cosine": 2}
_MASK = np.uint32(0x7FFFFFFF)


def float_to_key(f):
    """Order-preserving map fp32 -> uint32: negative floats have every bit flipped, the others get the sign bit."""
    u = np.asarray(f, np.float32).view(np.uint32)
    return np.where(u & np.uint32(NEW), ~u, u | np.uint32(NEW)).astype(np.uint32)


def key_to_float(k):
    k = np.asarray(k, np.uint32)
    return np.where(k & np.uint32(NEW), k & _MASK, ~k).astype(np.uint32).view(np.float32)


def row_norms(x):
    """|row| in fp32 for the cosine key (float64 sum, one rounding of the root): the tests hand the SAME array to the kernel."""
    return np.sqrt((np.asarray(x, np.float64) ** 2).sum(1)).astype(np.float32)


def pair_keys(x, a, b, metric, norms=None):
    """Keys of the row pairs (a[i], b[i]) of x (float32 / float16 / int8 / uint8 [n, dim]).

    sqeuclidean / inner_product / cosine: an 8-lane team; lane t takes elements t VL + 8 VL j + e (VL = 16 bytes of the row
    type) in order with a single-rounding fp32 fma, the partial sums meet by the xor butterfly 1, 2, 4 (oracle_nn_descent.c, fmaf);
    inner product is negated; cosine = 1 - dot / (|a| |b|), and 0 where |a| |b| is not positive.
    bitwise_hamming: the number of differing bits of the rows' bytes."""
    x = np.ascontiguousarray(x)
    a = np.ascontiguousarray(a, np.uint32).ravel()
    b = np.ascontiguousarray(b, np.uint32).ravel()
    assert a.shape == b.shape and (a.size == 0 or max(a.max(), b.max()) < x.shape[0])
    if metric == "bitwise_hamming":
        assert x.dtype.itemsize == 1
        bits = np.unpackbits(x.view(np.uint8)[a] ^ x.view(np.uint8)[b], axis=1)
        return float_to_key(bits.sum(1, dtype=np.int64).astype(np.float32))
    keys = np.empty(a.size, np.uint32)
    xf = np.ascontiguousarray(x, np.float32)   # exact for every row type
    nr = None
    if metric == "cosine":
        nr = np.ascontiguousarray(norms, np.float32)
        assert nr.shape == (x.shape[0],)
    p = lambda arr: arr.ctypes.data_as(C.c_void_p)
    oracle.lib().oracle_nnd_pair_keys(p(xf), C.c_int64(x.shape[1]), C.c_int(16 // x.dtype.itemsize), C.c_int(_MODE[metric]),
                                      p(nr) if nr is not None else None, p(a), p(b), C.c_int64(a.size), p(keys))
    return keys


U = 2.0 ** -24   # unit roundoff of fp32, round to nearest


def _gamma(k):
    """(1 + d1) ... (1 + dk) = 1 + t with |t| <= k U / (1 - k U) for |di| <= U (Higham, Accuracy and Stability, lemma 3.1)."""
    return k * U / (1.0 - k * U)


def exact_distance_and_bound(x, a, b, metric, norm_rel_err=None):
    """float64 distance of the row pairs (a[i], b[i]) and a bound on |fp32 result of the team arithmetic - it|.

    metric: sqeuclidean, euclidean (the root is taken in fp32 when the graph is returned), inner_product, cosine.
    Derivation. A lane's chain has L = min(dim, VL ceil(dim / 8 VL)) fused multiply-adds, then 3 butterfly additions.
      * inner product: the products inside the fma are exact; a term x_i y_i passes through at most L + 3 roundings, so
        |computed - dot| <= gamma(L + 3) sum|x_i y_i| =: E_ip.
      * squared L2: fl(x_i - y_i) = (x_i - y_i)(1 + d), squared: two more factors, so E_2 = gamma(L + 5) sum (x_i - y_i)^2
        = gamma(L + 5) d (all terms are non-negative).
      * euclidean: |sqrt(d') - sqrt(d)| <= min(sqrt|d' - d|, |d' - d| / sqrt(d)) =: e, and the fp32 root adds U (sqrt(d) + e).
      * cosine: the fp32 norms carry a relative error eps_n each (norm_rel_err; default gamma(dim + 2): dim squares summed in
        ANY order are within gamma(dim + 1), the root halves that and rounds once). fl(|a| |b|) = N (1 + t), |t| <= eps_t :=
        2 eps_n + eps_n^2 + U(1 + eps_n)^2; the quotient rounds once more: |q' - dot / N| <= (E_ip / N + |dot| / N (eps_t + U))
        / (1 - eps_t) =: e_q; the subtraction from 1 rounds once: bound = e_q + U (|1 - dot / N| + e_q).
        A pair with a zero row has distance 0 by the reference's rule, exactly."""
    x = np.asarray(x)
    dim = x.shape[1]
    vl = 16 // x.dtype.itemsize
    L = min(dim, vl * -(-dim // (8 * vl)))
    xa, xb = x[a].astype(np.float64), x[b].astype(np.float64)
    if metric in ("sqeuclidean", "euclidean"):
        d = ((xa - xb) ** 2).sum(-1)
        e2 = _gamma(L + 5) * d
        if metric == "sqeuclidean":
            return d, e2
        root = np.sqrt(d)
        e = np.minimum(np.sqrt(e2), np.divide(e2, root, out=np.full_like(e2, np.inf), where=root > 0))
        return root, e + U * (root + e)
    dot, e_ip = (xa * xb).sum(-1), _gamma(L + 3) * np.abs(xa * xb).sum(-1)
    if metric == "inner_product":
        return dot, e_ip
    assert metric == "cosine"
    eps_n = _gamma(dim + 2) if norm_rel_err is None else norm_rel_err
    eps_t = 2 * eps_n + eps_n ** 2 + U * (1 + eps_n) ** 2
    N = np.sqrt((xa * xa).sum(-1)) * np.sqrt((xb * xb).sum(-1))
    ok = N > 0
    Ns = np.where(ok, N, 1.0)
    e_q = (e_ip / Ns + np.abs(dot) / Ns * (eps_t + U)) / (1.0 - eps_t)
    d = 1.0 - dot / Ns
    return np.where(ok, d, 0.0), np.where(ok, e_q + U * (np.abs(d) + e_q), 0.0)


def xs64(u):
    """xorshift64* of uint64 arrays (wrapping arithmetic)."""
    u = np.asarray(u, np.uint64).copy()
    u ^= u >> np.uint64(12)
    u ^= u << np.uint64(25)
    u ^= u >> np.uint64(27)
    return u * np.uint64(0x2545F4914F6CDD1D)


# --------------------------------------------------------------------------------------------------------------- merge
def merge(ids, keys, prop_ids, prop_keys, prop_cnt):
    """List [n, K] + the first min(prop_cnt, P) proposals [n, P] -> (ids, keys, worst, prop_cnt).

    A proposal of v itself or of NONE is empty, every other one carries NEW. Entries are ordered by (key, id without flag,
    flag); an entry whose unflagged id equals its predecessor's is dropped (so of a listed neighbour and its re-proposal the
    list's copy survives, with the flag it had); the first K stay, the tail is (NONE, NONE); worst = the K-th key of a full list,
    NONE otherwise; the proposal counters return to 0."""
    ids, keys = np.asarray(ids, np.uint32), np.asarray(keys, np.uint32)
    n, K = ids.shape
    P = prop_ids.shape[1]
    out_i = np.full((n, K), NONE, np.uint32)
    out_k = np.full((n, K), NONE, np.uint32)
    worst = np.full(n, NONE, np.uint32)
    for v in range(n):
        c = min(int(prop_cnt[v]), P)
        pi = np.asarray(prop_ids[v, :c], np.uint32)
        live = (pi != NONE) & (pi != v)
        ei = np.concatenate([ids[v], pi[live] | np.uint32(NEW)])
        ek = np.concatenate([keys[v], np.asarray(prop_keys[v, :c], np.uint32)[live]])
        live = ei != NONE
        ei, ek = ei[live], ek[live]
        order = np.lexsort((ei >> 31, ei & _MASK, ek))   # last key is the primary one
        ei, ek = ei[order], ek[order]
        bare = ei & _MASK
        first = np.ones(ei.size, bool)
        first[1:] = bare[1:] != bare[:-1]
        ei, ek = ei[first][:K], ek[first][:K]
        out_i[v, :ei.size], out_k[v, :ei.size] = ei, ek
        if ei.size == K:
            worst[v] = ek[K - 1]
    return out_i, out_k, worst, np.zeros(n, np.uint32)


def count_new(ids):
    ids = np.asarray(ids, np.uint32)
    return int(((ids != NONE) & ((ids & np.uint32(NEW)) != 0)).sum())


# -------------------------------------------------------------------------------------------------------------- sample
def sample(ids):
    """Lists [n, K] -> dict: ids (the sampled new entries lose their flag), fwd_new / fwd_old [n, S] (the first S flagged /
    unflagged entries in list order, NONE-padded), rev_new_cnt / rev_old_cnt [n] (how many rows sampled u), rev_new_set /
    rev_old_set (per row u: the sorted rows that sampled it - a reverse list holds these, or 32 of them)."""
    ids = np.asarray(ids, np.uint32).copy()
    n, K = ids.shape
    out = dict(fwd_new=np.full((n, S), NONE, np.uint32), fwd_old=np.full((n, S), NONE, np.uint32))
    pubs = dict(new=[[] for _ in range(n)], old=[[] for _ in range(n)])
    for v in range(n):
        valid = ids[v] != NONE
        flagged = valid & ((ids[v] & np.uint32(NEW)) != 0)
        take_new = np.nonzero(flagged)[0][:S]
        take_old = np.nonzero(valid & ~flagged)[0][:S]
        ids[v, take_new] &= _MASK
        out["fwd_new"][v, :take_new.size] = ids[v, take_new]
        out["fwd_old"][v, :take_old.size] = ids[v, take_old]
        for u in ids[v, take_new]:
            pubs["new"][int(u)].append(v)
        for u in ids[v, take_old]:
            pubs["old"][int(u)].append(v)
    out["ids"] = ids
    for kind in ("new", "old"):
        out[f"rev_{kind}_cnt"] = np.array([len(p) for p in pubs[kind]], np.uint32)
        out[f"rev_{kind}_set"] = [sorted(p) for p in pubs[kind]]
    return out


# ---------------------------------------------------------------------------------------------------------------- join
def join(x, metric, norms, fwd_new, fwd_old, rev_new, rev_old, rev_new_cnt, rev_old_cnt, worst):
    """The local join of every row -> (prop_cnt [n], proposals: per target the sorted list of (candidate, key)).

    For row v: cn = its forward new samples + the first min(count, S) reverse new ones, co likewise for old (NONE skipped).
    Every pair i < j of cn and every pair of cn x co, except pairs of a row with itself, gets its key; each endpoint whose
    worst key the pair's key beats receives the other endpoint as a proposal. prop_cnt counts ALL of them (the buffer keeps
    the first P that arrive)."""
    n = fwd_new.shape[0]
    pa, pb = [], []
    for v in range(n):
        cn = [int(u) for u in fwd_new[v] if u != NONE] + [int(u) for u in rev_new[v, :min(int(rev_new_cnt[v]), S)] if u != NONE]
        co = [int(u) for u in fwd_old[v] if u != NONE] + [int(u) for u in rev_old[v, :min(int(rev_old_cnt[v]), S)] if u != NONE]
        for i in range(len(cn)):
            for j in range(i + 1, len(cn)):
                pa.append(cn[i]); pb.append(cn[j])
            for o in co:
                pa.append(cn[i]); pb.append(o)
    pa, pb = np.array(pa, np.uint32), np.array(pb, np.uint32)
    keep = pa != pb
    pa, pb = pa[keep], pb[keep]
    keys = pair_keys(x, pa, pb, metric, norms)
    props = [[] for _ in range(n)]
    worst = np.asarray(worst, np.uint32)
    for a, b, k in zip(pa.tolist(), pb.tolist(), keys.tolist()):
        if k < worst[a]:
            props[a].append((b, k))
        if k < worst[b]:
            props[b].append((a, k))
    return np.array([len(p) for p in props], np.uint32), [sorted(p) for p in props]


# ---------------------------------------------------------------------------------------------------------------- init
def init(x, metric, norms, K, P, seed, perm=None, cl_off=None, labels=None, hubs=None):
    """The initial proposals of every row -> (prop_ids [n, c], prop_keys [n, c], prop_cnt [n]) with c = min(K, P).

    Slot c of row v: a pseudo-random row xs64((v K + c) ^ seed) % n, except that
      * with a clustering (perm = rows grouped by cluster, cl_off = cluster offsets, labels), an EVEN slot c with
        c / 2 + 1 < cluster size holds the (c / 2 + 1)-th row after v in its cluster, cyclically;
      * with hubs, every FOURTH slot (c % 4 == 3) with c / 4 < len(hubs) holds hubs[c / 4] - this rule comes first.
    A slot that would hold v itself holds (v + 1) % n."""
    n = x.shape[0]
    c_n = min(K, P)
    v = np.arange(n, dtype=np.uint64)[:, None]
    c = np.arange(c_n, dtype=np.uint64)[None, :]
    u = (xs64((v * np.uint64(K) + c) ^ np.uint64(seed)) % np.uint64(n)).astype(np.int64)
    if perm is not None:
        perm, cl_off, labels = (np.asarray(t).astype(np.int64) for t in (perm, cl_off, labels))
        pos_of = np.empty(n, np.int64)
        pos_of[perm] = np.arange(n)
        for r in range(n):
            begin = cl_off[labels[r]]
            size = cl_off[labels[r] + 1] - begin
            for s in range(0, c_n, 2):
                if s // 2 + 1 < size:
                    u[r, s] = perm[begin + (pos_of[r] - begin + 1 + s // 2) % size]
    if hubs is not None:
        hubs = np.asarray(hubs).astype(np.int64)
        for s in range(3, c_n, 4):
            if s // 4 < len(hubs):
                u[:, s] = hubs[s // 4]
    rows = np.arange(n)[:, None]
    u = np.where(u == rows, (u + 1) % n, u).astype(np.uint32)
    keys = pair_keys(x, np.broadcast_to(rows, u.shape).ravel(), u.ravel(), metric, norms).reshape(u.shape)
    return u, keys, np.full(n, c_n, np.uint32)
