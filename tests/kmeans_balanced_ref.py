"""Shared by tests/test_kmeans_balanced_cpu.py and tests/test_kmeans_balanced_gpu.py: the inputs of every case, the twin's
results (computed once per process) and the checks against float64 numpy that a mistake shared by the HIP code and its twin
(oracle/oracle_kmeans.c) cannot pass.

Data: standard normal x 3, every fifth row x 1e3 (the order of a float32 sum then shows in its last bits). "skew": 70 % of the
rows are copies of row 1 plus 1e-3 noise. Pitched inputs sit in a NaN-filled buffer, so a read outside a row's columns poisons
the result."""
import functools

import numpy as np

import oracle

U = 2.0 ** -24  # unit roundoff of float32


def gamma(n):
    """Higham's gamma_n = n u / (1 - n u): the relative error bound of n float32 additions in any order."""
    return n * U / (1.0 - n * U)


def make_rows(seed, n, dim, skew=False, lognormal=False):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, dim)) * 3.0
    x[::5] *= 1e3
    if skew:
        idx = rng.permutation(n)[: int(0.7 * n)]
        x[idx] = x[1] + 1e-3 * rng.standard_normal((len(idx), dim))
    if lognormal:
        x *= np.exp(rng.standard_normal(n))[:, None]
    return x.astype(np.float32)


def pitched(x, ld, col0):
    """x in columns [col0, col0 + dim) of a NaN-filled [n, ld] buffer."""
    n, dim = x.shape
    assert col0 + dim <= ld
    buf = np.full((n, ld), np.nan, np.float32)
    buf[:, col0:col0 + dim] = x
    return buf


# ---------------------------------------------------------------------------------------------- A: cluster means
MEANS_DIMS = (1, 2, 3, 12, 16, 31, 32, 33, 64, 65, 100, 128, 200)


def slots(dim):
    """S of cluster_means_kernel: partial sums per cluster and dimension."""
    if dim > 32:
        return 4
    dp = 1
    while dp < dim:
        dp <<= 1
    return 4 * (64 // dp)


def means_sizes(dim):
    S = slots(dim)
    return [0, 1, S - 1, S, S + 1, 4 * S - 1, 4 * S, 4 * S + 1, 8 * S + 3, 0, 1000]


@functools.lru_cache(maxsize=None)
def means_case(dim):
    """(x [n, dim], labels [n], k): one cluster of every size of means_sizes(dim), rows interleaved by a fixed shuffle."""
    sizes = means_sizes(dim)
    labels = np.repeat(np.arange(len(sizes), dtype=np.uint32), sizes)
    labels = labels[np.random.default_rng(1000 + dim).permutation(len(labels))]
    x = make_rows(2000 + dim, len(labels), dim)
    x.setflags(write=False)
    labels.setflags(write=False)
    return x, labels, len(sizes)


MEANS_PITCHES = ("dense", "pitched")  # ld = dim, and ld = dim + 5 with 3 columns in front


def means_buf(dim, pitch):
    x, _, _ = means_case(dim)
    return (x, 0) if pitch == "dense" else (pitched(x, dim + 5, 3), 3)


@functools.lru_cache(maxsize=None)
def twin_means(dim, pitch):
    _, labels, k = means_case(dim)
    buf, col0 = means_buf(dim, pitch)
    return oracle.kmeans_cluster_means(buf, labels, k, col0=col0, dim=dim)


def check_means(x, labels, k, centers, sizes):
    """sizes == bincount, empty clusters exactly 0, and per cluster and dimension
    |c - mean64| <= gamma_cnt * sum|x| / cnt + u * |mean64|: the any-order summation bound plus the rounding of the division.
    Returns the worst ratio to that bound."""
    cnt = np.bincount(labels, minlength=k)
    assert (np.asarray(sizes, dtype=np.int64) == cnt).all(), "sizes differ from bincount(labels)"
    assert np.isfinite(centers).all(), "non-finite centre"
    x64 = x.astype(np.float64)
    order = np.argsort(labels, kind="stable")
    start = np.concatenate([[0], np.cumsum(cnt)])
    worst = 0.0
    for c in range(k):
        if cnt[c] == 0:
            assert (centers[c] == 0).all(), f"empty cluster {c} is not zero"
            continue
        rows = x64[order[start[c]:start[c + 1]]]
        mean = rows.sum(0) / cnt[c]
        bound = gamma(int(cnt[c])) * np.abs(rows).sum(0) / cnt[c] + U * np.abs(mean)
        err = np.abs(centers[c].astype(np.float64) - mean)
        assert (err <= bound).all(), f"cluster {c} (size {cnt[c]}): error {err.max():.3e} beyond the summation bound"
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
    return worst


# ---------------------------------------------------------------------------------------------- C: build_clusters
# (n, ld, col0, dim, k, skew); 6177 = 29 * 71 * 3: adjust_centers has to skip a prime
BUILD_CASES = ((3000, 96, 24, 12, 256, False), (2500, 64, 62, 2, 16, False), (2048, 1, 0, 1, 64, False),
               (6177, 64, 0, 64, 48, True), (5000, 130, 1, 128, 40, True), (4000, 65, 0, 65, 7, False),
               (700, 33, 0, 33, 700, False), (701, 100, 0, 100, 700, True))
BUILD_ITERS = 10


@functools.lru_cache(maxsize=None)
def build_case(i, inner_product):
    """(x [n, dim], buf [n, ld], col0): inner product runs on rows scaled by a log-normal factor."""
    n, ld, col0, dim, k, skew = BUILD_CASES[i]
    x = make_rows(3000 + i, n, dim, skew=skew, lognormal=inner_product)
    buf = pitched(x, ld, col0)
    x.setflags(write=False)
    buf.setflags(write=False)
    return x, buf, col0


@functools.lru_cache(maxsize=None)
def twin_build(i, inner_product):
    """(centers, labels, sizes, trace) of the twin."""
    n, ld, col0, dim, k, skew = BUILD_CASES[i]
    _, buf, _ = build_case(i, inner_product)
    trace = np.zeros(8, np.int64)
    c, lab, sz = oracle.kmeans_build_clusters(buf, k, BUILD_ITERS, inner_product, col0=col0, dim=dim, trace=trace)
    return c, lab, sz, dict(zip(oracle.KMEANS_TRACE, trace.tolist()))


# ---------------------------------------------------------------------------------------------- D: adjust_centers
# (n, dim, ld, col0, threshold, i_primes before, i_primes after): k = 9, average = n // 9, average * threshold an integer.
# 1160 = 29 * 40: from the end of the table the pass wraps to 29, skips it and takes 71. 12354 = 29 * 71 * 6: it skips both.
ADJUST_CASES = ((1160, 100, 105, 3, 0.25, 39, 1), (12354, 5, 5, 0, 0.25, 39, 2))
PRIMES = (29, 71, 113)


@functools.lru_cache(maxsize=None)
def adjust_case(i):
    """(x, buf, labels, sizes, centers): sizes 0, 1, 6, 7, 8, exactly average * threshold, one more, and two large."""
    n, dim, ld, col0, threshold, _, _ = ADJUST_CASES[i]
    k, average = 9, n // 9
    edge = average * threshold
    assert edge == int(edge) and edge > 8
    sizes = [0, 1, 6, 7, 8, int(edge), int(edge) + 1]
    rest = n - sum(sizes)
    sizes += [rest // 2 - 40, rest - (rest // 2 - 40)]
    assert min(sizes[-2:]) >= average and len(sizes) == k
    rng = np.random.default_rng(4000 + i)
    labels = np.repeat(np.arange(k, dtype=np.uint32), sizes)[rng.permutation(n)]
    x = make_rows(4100 + i, n, dim)
    centers = (rng.standard_normal((k, dim)) * 3).astype(np.float32)
    sizes = np.asarray(sizes, np.uint32)
    buf = pitched(x, ld, col0)
    for a in (x, buf, labels, sizes, centers):
        a.setflags(write=False)
    return x, buf, labels, sizes, centers


@functools.lru_cache(maxsize=None)
def twin_adjust(i):
    n, dim, ld, col0, threshold, ip0, _ = ADJUST_CASES[i]
    _, buf, labels, sizes, centers = adjust_case(i)
    return oracle.kmeans_adjust_centers(centers, buf, labels, sizes, threshold, ip0, col0=col0, dim=dim)


def check_adjust(i, new_centers, adjusted, i_primes):
    """Every cluster of size <= average * threshold is re-seeded with (wc * c[li] + x[row]) / (wc + 1), wc = min(size, 7), where
    row is the first of (prime * (l + 1 + t * k)) % n, t = 0, 1, ..., whose cluster has at least the average size; the
    arithmetic is float32, one rounding per operation. Every other centre keeps its bytes."""
    n, dim, ld, col0, threshold, _, ip1 = ADJUST_CASES[i]
    x, _, labels, sizes, centers = adjust_case(i)
    k, average = len(sizes), n // len(sizes)
    prime = PRIMES[ip1]
    assert all(n % p == 0 for p in PRIMES[:ip1]) and n % prime != 0
    assert i_primes == ip1 and adjusted == 1
    touched = 0
    for l in range(k):
        if float(sizes[l]) > average * threshold:
            assert new_centers[l].tobytes() == centers[l].tobytes(), f"centre {l} (size {sizes[l]}) was changed"
            continue
        t = 0
        while True:
            row = (prime * (l + 1 + t * k)) % n
            t += 1
            if sizes[labels[row]] >= average:
                break
        wc = np.float32(min(int(sizes[l]), 7))
        want = (wc * centers[labels[row]] + x[row]) / (wc + np.float32(1))
        assert want.dtype == np.float32
        assert new_centers[l].tobytes() == want.tobytes(), f"centre {l} (size {sizes[l]}) is not the published re-seed"
        touched += 1
    assert touched == 6  # sizes 0, 1, 6, 7, 8 and the one exactly at the threshold


# ---------------------------------------------------------------------------------------------- E: balanced_fit
# (n, dim, k, hierarchical, skew); k = 1 and k = 2 ask for the hierarchy and get the flat route (n_meso <= 1)
FIT_CASES = ((20000, 128, 1024, True, False), (6000, 96, 300, True, True), (300, 16, 256, True, True),
             (4000, 33, 3, True, False), (4000, 200, 50, True, False), (500, 8, 1, True, False), (500, 8, 2, True, False),
             (3000, 64, 48, False, False))
FIT_ITERS = 10


@functools.lru_cache(maxsize=None)
def fit_case(i, lognormal):
    n, dim, k, hier, skew = FIT_CASES[i]
    x = make_rows(5000 + i, n, dim, skew=skew, lognormal=lognormal)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def twin_fit(i, inner_product, lognormal=None):
    """(centers, labels, trace) of the twin; inner product runs on the log-normal-scaled rows unless told otherwise."""
    n, dim, k, hier, skew = FIT_CASES[i]
    x = fit_case(i, inner_product if lognormal is None else lognormal)
    trace = np.zeros(8, np.int64)
    c, lab = oracle.kmeans_balanced_fit(x, k, FIT_ITERS, hier, inner_product, trace)
    return c, lab, dict(zip(oracle.KMEANS_TRACE, trace.tolist()))


def check_assignment(x, centers, labels, inner_product):
    """No NaN, and every label within rounding of the float64 best: with v = |c|^2 - 2 x.c (inner product: -2 x.c),
    v[label] - min v <= E[label] + E[argmin], E = gamma_{d+2} * (|c|^2 + 2 |x| |c|). Returns the worst ratio."""
    assert np.isfinite(centers).all(), "non-finite centre"
    n, dim = x.shape
    k = centers.shape[0]
    assert labels.shape == (n,) and (labels < k).all()
    c64 = centers.astype(np.float64)
    cn2 = (c64 * c64).sum(1)
    cn = np.sqrt(cn2)
    g = gamma(dim + 2)
    worst = 0.0
    for r0 in range(0, n, 2048):
        xs = x[r0:r0 + 2048].astype(np.float64)
        lab = labels[r0:r0 + 2048].astype(np.int64)
        v = -2.0 * (xs @ c64.T)
        if not inner_product:
            v += cn2[None, :]
        E = g * (cn2[None, :] + 2.0 * np.sqrt((xs * xs).sum(1))[:, None] * cn[None, :])
        rows = np.arange(len(xs))
        best = v.argmin(1)
        gap = v[rows, lab] - v[rows, best]
        tol = E[rows, lab] + E[rows, best]
        bad = gap > tol
        assert not bad.any(), f"row {r0 + int(np.flatnonzero(bad)[0])}: label beyond rounding of the best centre"
        worst = max(worst, float((gap / np.maximum(tol, 1e-300)).max()))
    return worst
