"""numpy front-end of oracle/liboracle.so — the CPU restatement of the reference's hot path.

TEST INFRASTRUCTURE ONLY: imported by tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg.
Nothing under cuvs_amd/ imports this package.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

METRICS = {"sqeuclidean": 0, "euclidean": 1, "l2": 1, "cosine": 2, "l2_unexpanded": 4, "l2_sqrt_unexpanded": 5,
           "inner_product": 6}


def lib():
    global _LIB
    if _LIB is None:
        path = os.path.join(_HERE, "liboracle.so")
        if not os.path.exists(path):
            raise ImportError(f"{path} missing: run `make oracle/liboracle.so`")
        _LIB = C.CDLL(path)
    return _LIB


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _metric(m):
    return METRICS[m] if isinstance(m, str) else int(m)


def num_threads():
    return lib().oracle_num_threads()


def set_num_threads(n=0):
    """OpenMP threads of the oracle's loops (0: every online core) - launchers such as torchrun pin OMP_NUM_THREADS=1."""
    lib().oracle_set_num_threads(int(n))


def row_norms(x, sqrt=False):
    x = _f32(x)
    out = np.empty(x.shape[0], np.float32)
    lib().oracle_row_norms(_p(x), C.c_int64(x.shape[0]), C.c_int64(x.shape[1]), _p(out), C.c_int(int(sqrt)))
    return out


def pairwise(q, x, metric="sqeuclidean", clamp_eps=1e-6):
    q, x = _f32(q), _f32(x)
    out = np.empty((q.shape[0], x.shape[0]), np.float32)
    lib().oracle_pairwise(_p(q), C.c_int64(q.shape[0]), _p(x), C.c_int64(x.shape[0]), C.c_int64(q.shape[1]),
                          C.c_int(_metric(metric)), C.c_float(clamp_eps), _p(out))
    return out


def select_k(vals, k, select_min=True, in_idx=None, idx_offset=0):
    vals = _f32(vals)
    rows, ln = vals.shape
    ov = np.empty((rows, k), np.float32)
    oi = np.empty((rows, k), np.int64)
    ii = None if in_idx is None else np.ascontiguousarray(in_idx, dtype=np.int64)
    lib().oracle_select_k(_p(vals), _p(ii) if ii is not None else None, C.c_int64(rows), C.c_int64(ln), C.c_int(k),
                          C.c_int(int(select_min)), C.c_int64(idx_offset), _p(ov), _p(oi))
    return ov, oi


def brute_force_knn(q, x, k, metric="sqeuclidean", clamp_eps=1e-6, keep_bits=None, bitmap=False):
    """Bit-for-bit twin of cuvsBruteForceSearch. Returns (distances, indices)."""
    q, x = _f32(q), _f32(x)
    oi = np.empty((q.shape[0], k), np.int64)
    od = np.empty((q.shape[0], k), np.float32)
    kb = None if keep_bits is None else np.ascontiguousarray(keep_bits, dtype=np.uint32)
    lib().oracle_brute_force_knn(_p(q), C.c_int64(q.shape[0]), _p(x), C.c_int64(x.shape[0]), C.c_int64(q.shape[1]),
                                 C.c_int(k), C.c_int(_metric(metric)), C.c_float(clamp_eps),
                                 _p(kb) if kb is not None else None, C.c_int(int(bitmap)), _p(oi), _p(od))
    return od, oi


def exact_knn(q, x, k, metric="sqeuclidean"):
    """The reference's CPU path (refine_host with every row as candidate). Returns (distances, indices)."""
    q, x = _f32(q), _f32(x)
    oi = np.empty((q.shape[0], k), np.int64)
    od = np.empty((q.shape[0], k), np.float32)
    lib().oracle_exact_knn(_p(q), C.c_int64(q.shape[0]), _p(x), C.c_int64(x.shape[0]), C.c_int64(q.shape[1]),
                           C.c_int(k), C.c_int(_metric(metric)), _p(oi), _p(od))
    return od, oi


def recall(found, truth):
    """Fraction of true neighbours found (reference: python/cuvs/cuvs/tests/ann_utils.py:24-30)."""
    found, truth = np.asarray(found), np.asarray(truth)
    hits = 0
    for f, t in zip(found, truth):
        hits += len(np.intersect1d(f, t))
    return hits / truth.size


_LUT_MODES = {"f32": 0, "f16": 1, "fp8": 2}


_COARSE_MODES = {"f32": 0, "f16": 1, "i8": 2}


def ivf_pq_search(exported, queries, k, n_probes, metric="sqeuclidean", scale=1.0, lut="f32", acc="f32", coarse="f32",
                  keep_bits=None):
    """Search an index exported with cuvs_amd.neighbors.ivf_pq.export_for_oracle. lut: "f32" | "f16" | "fp8" (the
    reference's fp_8bit<5, signed-for-inner-product>), acc: "f32" | "f16" (search_params.lut_dtype /
    internal_distance_dtype), coarse: "f32" | "f16" | "i8" (coarse_search_dtype: coarse search and query rotation in
    that type), keep_bits: optional uint32 words of a bitset over source ids (1 keeps the row).
    Returns (distances, neighbors); bit-for-bit twin of cuvsIvfPqSearch."""
    q = _f32(queries)
    centers = _f32(exported["centers"])
    centers_rot = _f32(exported["centers_rot"])
    rotation = _f32(exported["rotation"])
    pqc = _f32(exported["pq_centers"])
    sizes = np.ascontiguousarray(exported["list_sizes"], dtype=np.uint32)
    start = np.zeros(len(sizes) + 1, np.int64)
    np.cumsum(sizes, out=start[1:])
    codes = np.ascontiguousarray(np.concatenate(exported["codes"], axis=0), dtype=np.uint8)
    ids = np.ascontiguousarray(np.concatenate(exported["ids"], axis=0), dtype=np.int64)
    nq = q.shape[0]
    nb = np.empty((nq, k), np.int64)
    ds = np.empty((nq, k), np.float32)
    kb = None if keep_bits is None else np.ascontiguousarray(keep_bits, dtype=np.uint32)
    lib().oracle_ivf_pq_search(
        _p(q), C.c_int64(nq), C.c_int(q.shape[1]), _p(centers), _p(centers_rot), _p(rotation), _p(pqc),
        C.c_int(len(sizes)), C.c_int(rotation.shape[0]), C.c_int(int(exported["pq_dim"])),
        C.c_int(int(exported["pq_len"])), C.c_int(int(exported["pq_bits"])), _p(sizes), _p(start), _p(codes), _p(ids),
        C.c_int(_metric(metric)), C.c_int(n_probes), C.c_int(k), C.c_float(scale), _p(nb), _p(ds),
        C.c_int(int(bool(exported.get("per_cluster", False)))), C.c_int(_LUT_MODES[lut]), C.c_int(_LUT_MODES[acc]),
        C.c_int(_COARSE_MODES[coarse]),
        _p(kb) if kb is not None else None)
    return ds, nb


def fp8_round_trip(values, signed=False, to_half=False):
    """decode(encode(v)) of the reference's fp_8bit<5, signed> (ivf_pq_fp_8bit.cuh:32-100), element-wise."""
    L = lib()
    L.oracle_fp8_encode.restype = C.c_uint8
    L.oracle_fp8_decode_f32.restype = C.c_float
    L.oracle_fp8_decode_f16.restype = C.c_float
    dec = L.oracle_fp8_decode_f16 if to_half else L.oracle_fp8_decode_f32
    v = np.asarray(values, np.float32)
    out = np.array([dec(C.c_uint8(L.oracle_fp8_encode(C.c_float(float(x)), C.c_int(int(signed)))), C.c_int(int(signed)))
                    for x in v.ravel()], np.float32)
    return out.reshape(v.shape)


def pq_encode(resid, pq_centers, pq_bits):
    resid = _f32(resid)
    pqc = _f32(pq_centers)
    pq_dim, pq_len, _ = pqc.shape
    out = np.empty((resid.shape[0], pq_dim), np.uint8)
    lib().oracle_pq_encode(_p(resid), C.c_int64(resid.shape[0]), C.c_int(resid.shape[1]), _p(pqc), C.c_int(pq_dim),
                           C.c_int(pq_len), C.c_int(pq_bits), _p(out))
    return out


def refine(dataset, queries, candidates, k, metric="sqeuclidean"):
    """CPU twin of cuvsRefine. Returns (distances, indices)."""
    x, q = _f32(dataset), _f32(queries)
    cand = np.ascontiguousarray(candidates, dtype=np.int64)
    oi = np.empty((q.shape[0], k), np.int64)
    od = np.empty((q.shape[0], k), np.float32)
    lib().oracle_refine(_p(x), C.c_int64(x.shape[0]), C.c_int64(x.shape[1]), _p(q), C.c_int64(q.shape[0]), _p(cand),
                        C.c_int(cand.shape[1]), C.c_int(k), C.c_int(_metric(metric)), _p(oi), _p(od))
    return od, oi


def ivf_flat_search(exported, queries, k, n_probes, metric="sqeuclidean", coarse_scale=1.0):
    """Search an index exported with cuvs_amd.neighbors.ivf_flat.export_for_oracle. `queries` in the index dtype;
    coarse_scale = 1/128 (int8) or 1/256 (uint8): the coarse quantizer sees mapped floats (ann_utils.cuh:134-196)."""
    int_mode = int(np.asarray(queries).dtype in (np.int8, np.uint8) and metric != "cosine")
    q_raw = _f32(np.asarray(queries).astype(np.float32))
    q_coarse = _f32(q_raw * np.float32(coarse_scale))
    centers = _f32(exported["centers"])
    sizes = np.ascontiguousarray(exported["list_sizes"], dtype=np.uint32)
    start = np.zeros(len(sizes) + 1, np.int64)
    np.cumsum(sizes, out=start[1:])
    rows = _f32(np.concatenate([r.astype(np.float32) for r in exported["rows"]], axis=0))
    ids = np.ascontiguousarray(np.concatenate(exported["ids"], axis=0), dtype=np.int64)
    nq = q_raw.shape[0]
    nb = np.empty((nq, k), np.int64)
    ds = np.empty((nq, k), np.float32)
    lib().oracle_ivf_flat_search(_p(q_coarse), _p(q_raw), C.c_int64(nq), C.c_int(q_raw.shape[1]), _p(centers),
                                 C.c_int(len(sizes)), _p(sizes), _p(start), _p(rows), _p(ids), C.c_int(_metric(metric)),
                                 C.c_int(n_probes), C.c_int(k), C.c_int(int_mode), _p(nb), _p(ds))
    return ds, nb


def cagra_search(dataset, graph, queries, k, itopk_size=64, search_width=1, max_iterations=0, min_iterations=0,
                 hashmap_min_bitlen=0, rand_xor_mask=0x128394, metric="sqeuclidean", filter_words=None, num_random_samplings=1):
    """CPU twin of cuvsCagraSearch (same parameter derivation as cuvs_amd/csrc/cagra.hip: search_plan.cuh:199-245).
    dataset/queries in the index dtype; graph uint32 [n, degree]. Returns (distances, neighbors)."""
    raw = np.asarray(dataset)
    vl = 16 // raw.dtype.itemsize
    x, q = _f32(raw.astype(np.float32)), _f32(np.asarray(queries).astype(np.float32))
    g = np.ascontiguousarray(graph, dtype=np.uint32)
    n, degree = g.shape
    width = max(1, int(search_width))
    itopk = max(int(itopk_size) if itopk_size else 64, k)
    if itopk % 32:
        itopk += 32 - itopk % 32
    max_iter = int(max_iterations)
    if max_iter == 0:
        max_iter = itopk // width
        reach = 1
        while reach < n:
            reach *= max(2, degree // 2)
            max_iter += 1
    if int(max_iterations) < int(min_iterations):  # the reference tests the original field (search_plan.cuh:216)
        max_iter = int(min_iterations)
    bits = 11
    while (1 << bits) < 2 * (itopk + 2 * width * degree):
        bits += 1
    bits = max(bits, int(hashmap_min_bitlen))
    reset = max(1, ((1 << bits) // 2 - itopk) // (width * degree))
    nq = q.shape[0]
    oi = np.empty((nq, k), np.int64)
    od = np.empty((nq, k), np.float32)
    fw = None if filter_words is None else np.ascontiguousarray(filter_words, dtype=np.uint32)
    lib().oracle_cagra_search(_p(x), C.c_int64(n), C.c_int64(x.shape[1]), C.c_int(vl), _p(g), C.c_int(degree), _p(q),
                              C.c_int64(nq), C.c_int(k), C.c_int(itopk), C.c_int(width), C.c_int(max_iter),
                              C.c_int(int(min_iterations)), C.c_int(bits), C.c_int(reset), C.c_uint64(rand_xor_mask),
                              C.c_int({6: 1, 2: 2}.get(_metric(metric), 0)), _p(fw) if fw is not None else None, _p(oi), _p(od),
                              C.c_int(max(1, int(num_random_samplings))))
    return od, oi


def cagra_optimize(knn_graph, graph_degree, guarantee_connectivity=False):
    """CPU twin of graph::optimize (oracle_cagra_optimize.c). Returns (graph [n, degree] uint32, components left by the
    connectivity pass - 0 when it was not asked for)."""
    g = np.ascontiguousarray(knn_graph, dtype=np.uint32)
    n, K = g.shape
    out = np.empty((n, graph_degree), np.uint32)
    fn = lib().oracle_cagra_optimize
    fn.restype = C.c_int64
    left = fn(_p(g), C.c_int64(n), C.c_uint32(K), C.c_uint32(graph_degree), C.c_int(int(guarantee_connectivity)), _p(out))
    return out, int(left)


def cagra_mst(knn_graph, graph_degree):
    """The spanning forest alone: (rows [n, degree] front-packed with 0xffffffff fillers, counts [n], components left)."""
    g = np.ascontiguousarray(knn_graph, dtype=np.uint32)
    n, K = g.shape
    mst = np.empty((n, graph_degree), np.uint32)
    cnt = np.empty(n, np.uint32)
    fn = lib().oracle_cagra_mst
    fn.restype = C.c_int64
    left = fn(_p(g), C.c_int64(n), C.c_uint32(K), C.c_uint32(graph_degree), _p(mst), _p(cnt))
    return mst, cnt, int(left)


KMEANS_TRACE = ("adjust_passes", "extra_iters", "primes_skipped", "meso_truncated", "meso_cyclic", "meso_empty",
                "empty_at_return", "flat_route")


def _trace_arg(trace):
    """trace: None, or a C-contiguous int64 array of 8 counters (KMEANS_TRACE names them) that the call overwrites."""
    if trace is None:
        return None
    assert trace.dtype == np.int64 and trace.shape == (8,) and trace.flags.c_contiguous
    return _p(trace)


def _pitched(buf, col0, dim):
    """Rows of a C-contiguous float32 matrix `buf`, columns [col0, col0 + dim): (buf kept alive, pointer, n, ld, dim)."""
    buf = _f32(buf)
    n, ld = buf.shape
    dim = ld - col0 if dim is None else int(dim)
    assert 0 <= col0 and dim >= 1 and col0 + dim <= ld
    return buf, C.c_void_p(buf.ctypes.data + 4 * col0), n, ld, dim


def kmeans_balanced_fit(x, n_clusters, n_iters=20, hierarchical=True, inner_product=False, trace=None):
    """CPU twin of the balanced k-means (cuvs_amd/csrc/kmeans_balanced.hip). Returns (centers, labels); the labels are
    predicted against the returned centres (inner_product: the largest dot product)."""
    x = _f32(x)
    n, dim = x.shape
    centers = np.empty((n_clusters, dim), np.float32)
    labels = np.empty(n, np.uint32)
    lib().oracle_kmeans_balanced_fit_ex(_p(x), C.c_int64(n), C.c_int(dim), C.c_int(n_clusters), C.c_int(n_iters),
                                        C.c_int(int(hierarchical)), C.c_int(int(inner_product)), _p(centers), _p(labels),
                                        _trace_arg(trace))
    return centers, labels


def kmeans_build_clusters(buf, n_clusters, n_iters=10, inner_product=False, col0=0, dim=None, trace=None):
    """Twin of kmeans_build_clusters on columns [col0, col0 + dim) of `buf` (row pitch buf.shape[1]).
    Returns (centers, labels, sizes)."""
    buf, px, n, ld, dim = _pitched(buf, col0, dim)
    centers = np.empty((n_clusters, dim), np.float32)
    labels = np.empty(n, np.uint32)
    sizes = np.empty(n_clusters, np.uint32)
    lib().oracle_kmeans_build_clusters_ex(px, C.c_int64(n), C.c_int64(ld), C.c_int(dim), C.c_int(n_clusters),
                                          C.c_int(n_iters), C.c_int(int(inner_product)), _p(centers), _p(labels), _p(sizes),
                                          _trace_arg(trace))
    return centers, labels, sizes


def kmeans_cluster_means(buf, labels, n_clusters, col0=0, dim=None):
    """Twin of calc_centers_and_sizes (the M-step) for given labels. Returns (centers, sizes)."""
    buf, px, n, ld, dim = _pitched(buf, col0, dim)
    labels = np.ascontiguousarray(labels, dtype=np.uint32)
    assert labels.shape == (n,) and (labels < n_clusters).all()
    centers = np.empty((n_clusters, dim), np.float32)
    sizes = np.empty(n_clusters, np.uint32)
    lib().oracle_kmeans_calc_centers(px, C.c_int64(n), C.c_int64(ld), C.c_int(dim), C.c_int(n_clusters), _p(labels),
                                     _p(centers), _p(sizes))
    return centers, sizes


def kmeans_adjust_centers(centers, buf, labels, sizes, threshold, i_primes, col0=0, dim=None):
    """Twin of one adjust_centers pass. Returns (new centers, adjusted flag, new i_primes)."""
    buf, px, n, ld, dim = _pitched(buf, col0, dim)
    centers = _f32(centers).copy()
    k = centers.shape[0]
    assert centers.shape == (k, dim)
    labels = np.ascontiguousarray(labels, dtype=np.uint32)
    sizes = np.ascontiguousarray(sizes, dtype=np.uint32)
    assert labels.shape == (n,) and sizes.shape == (k,) and (labels < k).all()
    ip = C.c_int(int(i_primes))
    fn = lib().oracle_kmeans_adjust_centers
    fn.restype = C.c_int
    adjusted = fn(_p(centers), C.c_int(k), C.c_int(dim), px, C.c_int64(ld), C.c_int64(n), _p(labels), _p(sizes),
                  C.c_float(threshold), C.byref(ip))
    return centers, int(adjusted), ip.value


def kmeans_lloyd(x, init_centroids, max_iter=300, tol=1e-4, sample_weights=None, trace=False):
    """Lloyd iterations as the reference runs them (cpp/src/cluster/detail/kmeans.cuh:813-925): per iteration the
    cost against the CURRENT centroids, weighted means (a cluster with zero weight keeps its centroid,
    kmeans_common.cuh:585-600), squared centroid shift, then the stopping rule of kmeans_common.cuh:629-648 evaluated in
    float32 like the reference's DataT. Weights are rescaled to sum to n (kmeans.cuh:713-726). Arithmetic is float64
    here: the HIP path is compared within a stated tolerance, not bit for bit.
    Returns (centroids float32 [k, d], labels int32 [n], inertia, n_iter); with trace=True a fifth item, one dict per
    iteration: cost (float64), ratio (float32 cost / prior cost, None in the first iteration), shift (float64) and
    which branches of the stopping rule fired (by_ratio, by_shift)."""
    x64 = np.asarray(x, dtype=np.float64)
    cur = np.asarray(init_centroids, dtype=np.float64).copy()
    n, k = x64.shape[0], cur.shape[0]
    w = np.ones(n) if sample_weights is None else np.asarray(sample_weights, dtype=np.float64) * n / np.sum(sample_weights)

    def assign(c):
        d = ((x64 * x64).sum(1)[:, None] - 2.0 * x64 @ c.T) + (c * c).sum(1)[None, :]
        lab = d.argmin(1)
        return lab, ((x64 - c[lab]) ** 2).sum(1)

    prior, ran, steps = 0.0, 0, []
    for it in range(1, max_iter + 1):
        lab, dist = assign(cur)
        cost = float((w * dist).sum())
        nxt = cur.copy()
        for c in range(k):
            m = lab == c
            ws = w[m].sum()
            if ws > 0:
                nxt[c] = (w[m, None] * x64[m]).sum(0) / ws
        shift = float(((nxt - cur) ** 2).sum())
        cur, ran = nxt, it
        by_ratio = bool(cost != 0.0 and it > 1 and np.float32(cost / prior) > np.float32(1.0) - np.float32(tol))
        by_shift = bool(np.float32(shift) < np.float32(tol))
        done = by_ratio or by_shift
        steps.append({"cost": cost, "ratio": float(np.float32(cost / prior)) if it > 1 and prior != 0.0 else None,
                      "ratio64": cost / prior if it > 1 and prior != 0.0 else None, "shift": shift,
                      "by_ratio": by_ratio, "by_shift": by_shift})
        prior = cost
        if done:
            break
    lab, dist = assign(cur)
    out = (cur.astype(np.float32), lab.astype(np.int32), float((w * dist).sum()), ran)
    return out + (steps,) if trace else out


def kmeans_lloyd_margin(steps, tol, dim):
    """True when no decision of the stopping rule in a kmeans_lloyd trace can be flipped by float32 rounding on the
    device. An iteration is safe when its shift is at most tol / 2 (it stops whatever the ratio says), or when its shift
    is at least 2 * tol and its cost ratio is clear of the threshold 1 - tol:
      * by 1e-3 where the float32 threshold is below 1 (the two costs agree with float64 far better than that);
      * where tol is below the float32 epsilon the threshold is exactly 1.0f, which only a cost that RISES by 2^-24 can
        exceed. Each row's distance carries at most (dim + 1) roundings of 2^-24, so the device's ratio is within
        2 * (dim + 2) * 2^-24 of the float64 one: the float64 ratio must stay that far below 1."""
    thr = np.float32(1.0) - np.float32(tol)
    for s in steps:
        if s["shift"] <= 0.5 * tol:
            continue
        if s["shift"] < 2.0 * tol:
            return False
        if s["ratio"] is None:
            continue
        if thr == np.float32(1.0):
            if s["ratio64"] > 1.0 - 2.0 * (dim + 2) * 2.0 ** -24:
                return False
        elif abs(s["ratio"] - float(thr)) < 1e-3:
            return False
    return True


# ---- seeding of the Lloyd fit (cuvs_amd/csrc/kmeans_capi.hip: seed_centroids), restated step for step ----------------

_M64 = (1 << 64) - 1


class mt19937_64:
    """std::mt19937_64: seeded with 5489 its 10000th output is 9981545732273789042 ([rand.predef])."""

    def __init__(self, seed):
        s = [int(seed) & _M64]
        for i in range(1, 312):
            s.append((6364136223846793005 * (s[-1] ^ (s[-1] >> 62)) + i) & _M64)
        self.s, self.i = s, 312

    def _twist(self):
        s = self.s
        for i in range(312):
            y = (s[i] & 0xFFFFFFFF80000000) | (s[(i + 1) % 312] & 0x7FFFFFFF)
            s[i] = s[(i + 156) % 312] ^ (y >> 1) ^ (0xB5026F5AA96619E9 if y & 1 else 0)
        self.i = 0

    def __call__(self):
        if self.i >= 312:
            self._twist()
        y = self.s[self.i]
        self.i += 1
        y ^= (y >> 29) & 0x5555555555555555
        y ^= (y << 17) & 0x71D67FFFEDA60000
        y ^= (y << 37) & 0xFFF7EEE000000000
        return y ^ (y >> 43)


def kmeans_trial_seeds(n_init, seed=0):
    """The seed each of the n_init trials of a fit hands to its seeding: successive outputs of mt19937_64(seed)."""
    gen = mt19937_64(seed)
    return [gen() for _ in range(n_init)]


def _mix64(z):
    """splitmix64 finaliser on uint64 arrays (wraps around like the device code)."""
    z = z + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def _row_sqdist_f32(x, c):
    """|x_i - c|^2 as one 64-lane wave computes it: lane l accumulates dims l, l + 64, ... by fma, then a butterfly sum."""
    n, dim = x.shape
    t = np.zeros((n, -(-dim // 64) * 64), dtype=np.float32)
    t[:, :dim] = x - c[None, :]
    t = t.reshape(n, -1, 64)
    acc = np.zeros((n, 64), dtype=np.float32)
    for j in range(t.shape[1]):  # fma: exact product (48 bits fit a double), one rounding of the sum
        acc = (t[:, j].astype(np.float64) ** 2 + acc.astype(np.float64)).astype(np.float32)
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lanes ^ off]
    return acc[:, 0]


def kmeans_seed_rows(x, k, init, trial_seed, sample_weights=None, forced=None):
    """The k rows seed_centroids picks for one trial, and a per-round trace.

    init is "Random" (Floyd's algorithm on the generator, ids sorted; integer only, so exact) or "KMeansPlusPlus" (the
    exponential race of pp_round_kernel / pp_pick_kernel: per round j, mind = min(mind, |x - c_j|^2) in float32, a
    counter hash of (round seed, j, row) mapped to u in float32 exactly as the kernel maps it (its top value rounds to
    1.0, whose key is -inf and never wins), key = w * mind / -log(u), arg max with ties to the smaller row). Weights
    are rescaled to sum to n in float32 like normalized_weights; the first seed ignores them. `forced`, a list of row
    ids, replaces the twin's own pick in the rounds it covers (entry 0 is the first seed), so a comparison can follow
    another implementation's picks. The trace holds one dict per k-means++ round: pick (the twin's own arg max),
    best, second (keys), second_row, and used (the row carried forward). The device takes the logarithm with its
    fast instruction; the twin takes it in float64 and rounds to float32."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    n, dim = x.shape
    gen = mt19937_64(trial_seed)
    if init == "Random":
        chosen, ids = set(), []
        for j in range(n - k, n):
            t = gen() % (j + 1)
            if t in chosen:
                t = j
            chosen.add(t)
            ids.append(t)
        return sorted(ids), []
    assert init == "KMeansPlusPlus"
    w = None
    if sample_weights is not None:
        w32 = np.asarray(sample_weights, dtype=np.float32)
        w = w32 * np.float32(n / float(w32.astype(np.float64).sum()))
    forced = list(forced) if forced is not None else []
    first = gen() % n
    round_seed = np.uint64(gen())
    ids = [int(forced[0]) if forced else int(first)]
    rows = np.arange(n, dtype=np.uint64)
    mind, steps = None, []
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for j in range(k - 1):
            d = _row_sqdist_f32(x, x[ids[j]])
            mind = d if mind is None else np.minimum(d, mind)
            h = _mix64(round_seed ^ _mix64((np.uint64(j + 1) << np.uint64(40)) ^ rows))
            u = ((h >> np.uint64(40)).astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 16777216.0)
            e = (-np.log(u.astype(np.float64))).astype(np.float32)
            key = (mind if w is None else w * mind) / e
            live = np.where(key > np.float32(-1.0), key, np.float32(-np.inf))  # NaN and -inf never beat the start, -1
            pick = int(np.argmax(live))  # first occurrence: ties keep the smaller row
            if not live[pick] > -1.0:
                pick, best, second, second_row = 0, float("-inf"), float("-inf"), -1  # pp_pick_kernel's fallback
            else:
                best = float(live[pick])
                rest = live.copy()
                rest[pick] = -np.inf
                second_row = int(np.argmax(rest))
                second = float(rest[second_row])
            used = int(forced[j + 1]) if j + 1 < len(forced) else pick
            steps.append({"pick": pick, "best": best, "second": second, "second_row": second_row, "used": used})
            ids.append(used)
    return ids, steps
