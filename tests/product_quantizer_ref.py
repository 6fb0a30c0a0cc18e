"""numpy side of the product quantizer tests: adversarial codebooks and rows, the bit rule of the packed codes, the fp64
distance bound, the reference's make_blobs data, and a plain Lloyd baseline for the training-quality test."""
import numpy as np

# (n_rows, pq_dim, pq_len, pq_bits, use_subspaces, use_vq): encoder cases of tests/test_product_quantizer_gpu.py. Row counts
# are multiples of no tile; pq_len 50 and 256 take the plain encoder by the fallback rule (pq_len > 32).
ENCODER_CASES = [
    (1, 8, 8, 8, True, False), (63, 4, 1, 4, True, False), (65, 3, 2, 5, False, False), (300, 1, 1, 8, True, False),
    (1000, 7, 3, 7, True, True), (999, 16, 4, 8, False, True), (513, 6, 5, 9, True, False), (2049, 8, 8, 10, True, True),
    (777, 4, 16, 12, False, False), (1025, 4, 32, 8, True, True), (4096, 4, 256, 10, False, False),
    (299, 60, 50, 8, False, True), (2000, 2, 2, 16, True, False), (1500, 12, 8, 5, True, False),
]
# default path == plain path only (too large for the fp64 check on the host)
PARITY_ONLY_CASES = [(100000, 32, 4, 8, True, False), (20000, 192, 4, 8, True, False), (20000, 96, 8, 8, True, True)]


def uses_default_path(pq_len):
    """the fallback rule of pq_quantize.hip (pq_use_default)"""
    return pq_len <= 32


def rows_per_lane(pq_len):
    """R of pq_encode_kernel<PL, R> when the launch is large enough (pq_encode in pq_quantize.hip)"""
    return 4 if pq_len <= 8 else 2


def multi_row_threshold(pq_len, num_cus):
    """the smallest row count that gets R > 1 rows per lane: ceil(n / (256 R)) >= 2 * compute units (pq_launch_default)"""
    return (2 * num_cus - 1) * 256 * rows_per_lane(pq_len) + 1


def runs_multi_row(case, num_cus):
    return uses_default_path(case[2]) and case[0] >= multi_row_threshold(case[2], num_cus)


# (pq_dim, pq_len, pq_bits, use_subspaces, use_vq) of the cases that reach R = 4 (PL 1, 2, 4, 8) and R = 2 (PL 16, 32); the row
# count comes from the device's compute units. Code rows of 4 bytes (full-word stores), 3 and 2 bytes (byte stores).
MULTI_ROW_SHAPES = [(8, 1, 4, True, False), (4, 2, 5, False, False), (3, 4, 4, True, True), (2, 8, 6, True, False),
                    (2, 16, 4, True, False), (2, 32, 5, False, True)]


def multi_row_cases(num_cus):
    """encoder cases just past the threshold, with a tail that is a multiple of neither 256 nor 256 R"""
    out = []
    for pq_dim, pq_len, bits, sub, vq in MULTI_ROW_SHAPES:
        r = rows_per_lane(pq_len)
        n = 2 * num_cus * 256 * r + 128 * r + 77
        assert n >= multi_row_threshold(pq_len, num_cus) and n % 256 != 0
        out.append((n, pq_dim, pq_len, bits, sub, vq))
    return out


def boundary_rows(n, pq_len):
    """rows at the start, around a boundary between the R row groups of a workgroup, around a workgroup boundary, and the tail"""
    r = rows_per_lane(pq_len)
    pieces = [np.arange(0, 300), np.arange(256 * 3 - 100, 256 * 3 + 100), np.arange(256 * r * 7 - 150, 256 * r * 7 + 150),
              np.arange(n - 400, n)]
    return np.unique(np.concatenate(pieces))


def make_book(rng, n_entries, pq_len):
    """half the entries normal, the other half their twins (every coordinate perturbed by a relative 2^-21 times a normal
    draw), shuffled: most rows then have two candidates within rounding of each other"""
    half = rng.normal(0, 1, (n_entries // 2, pq_len))
    twins = half * (1.0 + 2.0 ** -21 * rng.normal(0, 1, half.shape))
    book = np.concatenate([half, twins]).astype(np.float32)
    return book[rng.permutation(n_entries)]


def make_case(case, seed=0):
    """(rows [n, dim], pq_book, vq_book or None) of an encoder case, all float32"""
    n, pq_dim, pq_len, bits, subspaces, vq = case
    rng = np.random.default_rng(seed + 1000 * bits + pq_len)
    book_n, dim = 1 << bits, pq_dim * pq_len
    book = make_book(rng, (pq_dim if subspaces else 1) * book_n, pq_len)
    x = np.empty((n, pq_dim, pq_len), np.float32)
    for j in range(pq_dim):
        pick = rng.integers(0, book_n, n) + (j * book_n if subspaces else 0)
        x[:, j, :] = book[pick] + np.float32(0.05) * rng.normal(0, 1, (n, pq_len)).astype(np.float32)
    x = x.reshape(n, dim)
    vq_book = None
    if vq:
        vq_book = rng.normal(0, 4, (24, dim)).astype(np.float32)
        x = (x + vq_book[rng.integers(0, 24, n)]).astype(np.float32)
    return np.ascontiguousarray(x), book, vq_book


def encoded_dim(pq_dim, pq_bits):
    return (pq_dim * pq_bits + 7) // 8


def unpack_codes(codes, pq_dim, pq_bits):
    """code j of a row = bits [j * pq_bits, (j + 1) * pq_bits) of its bytes, little endian -> [n, pq_dim] int64"""
    bits = np.unpackbits(np.asarray(codes, np.uint8), axis=1, bitorder="little")[:, : pq_dim * pq_bits]
    w = (1 << np.arange(pq_bits, dtype=np.int64))
    return (bits.reshape(len(codes), pq_dim, pq_bits).astype(np.int64) * w).sum(axis=2)


def unused_bits_are_zero(codes, pq_dim, pq_bits):
    bits = np.unpackbits(np.asarray(codes, np.uint8), axis=1, bitorder="little")
    return not bits[:, pq_dim * pq_bits:].any()


def residual(x, vq_book, labels):
    """the fp32-rounded residual the encoder sees (one fp32 subtraction)"""
    return x if vq_book is None else (x - vq_book[labels]).astype(np.float32)


def sub_book(book, j, pq_bits, subspaces):
    return book[j * (1 << pq_bits):(j + 1) * (1 << pq_bits)] if subspaces else book


def distance_excess(r, book, codes, pq_dim, pq_len, pq_bits, subspaces):
    """max over (row, subspace) of d64(code) / d64(best) - 1 and the number of codes that are not the fp64 argmin; d64 in
    float64 over the fp32 values, summed coordinate by coordinate"""
    n = len(r)
    worst, differ = 0.0, 0
    r64 = r.reshape(n, pq_dim, pq_len).astype(np.float64)
    for j in range(pq_dim):
        b = sub_book(book, j, pq_bits, subspaces).astype(np.float64)
        d = np.zeros((n, len(b)))
        for k in range(pq_len):
            d += (r64[:, j, k, None] - b[None, :, k]) ** 2
        best = d.min(axis=1)
        mine = d[np.arange(n), codes[:, j]]
        differ += int((d.argmin(axis=1) != codes[:, j]).sum())
        with np.errstate(divide="ignore", invalid="ignore"):
            ex = np.where(best > 0, mine / best - 1.0, np.where(mine > 0, np.inf, 0.0))
        worst = max(worst, float(ex.max()))
    return worst, differ


def decode(book, codes, pq_len, pq_bits, subspaces, vq_book=None, labels=None):
    """book[code] (+ vq[label], one fp32 add)"""
    n, pq_dim = codes.shape
    out = np.empty((n, pq_dim, pq_len), np.float32)
    for j in range(pq_dim):
        out[:, j, :] = sub_book(book, j, pq_bits, subspaces)[codes[:, j]]
    out = out.reshape(n, pq_dim * pq_len)
    return out if vq_book is None else (out + vq_book[labels]).astype(np.float32)


def make_blobs(n, dim, seed, n_centers=5, box=10.0):
    """the data of the reference's C++ test: centres uniform in [-box, box]^dim, unit normal noise, shuffled"""
    rng = np.random.default_rng(seed)
    centers = rng.uniform(-box, box, (n_centers, dim))
    x = centers[np.arange(n) % n_centers] + rng.normal(0, 1, (n, dim))
    return np.ascontiguousarray(x[rng.permutation(n)].astype(np.float32))


def strided_trainset(x, n_train):
    return x[np.arange(n_train) * (len(x) // n_train)]


def lloyd(x, k, n_iters, rng):
    """plain Lloyd: random rows as seeds, empty clusters re-seeded from random rows"""
    x = x.astype(np.float64)
    c = x[rng.choice(len(x), k, replace=False)].copy()
    for _ in range(n_iters):
        d = (x * x).sum(1)[:, None] - 2.0 * x @ c.T + (c * c).sum(1)[None, :]
        lab = d.argmin(1)
        cnt = np.bincount(lab, minlength=k)
        s = np.zeros_like(c)
        np.add.at(s, lab, x)
        live = cnt > 0
        c[live] = s[live] / cnt[live, None]
        if (~live).any():
            c[~live] = x[rng.choice(len(x), int((~live).sum()), replace=False)]
    return c


def lloyd_pq_mse(x, pq_dim, pq_bits, n_iters, seed, max_train_points_per_pq_code=256, vq_book=None):
    """mean squared reconstruction error per row of a subspace PQ trained by `lloyd` on the strided trainset"""
    rng = np.random.default_rng(seed)
    n, dim = x.shape
    k, pq_len = 1 << pq_bits, dim // pq_dim
    if vq_book is not None:
        v = vq_book.astype(np.float64)
        lab = ((x.astype(np.float64) ** 2).sum(1)[:, None] - 2.0 * x.astype(np.float64) @ v.T + (v * v).sum(1)[None, :]).argmin(1)
        x = (x - vq_book[lab]).astype(np.float32)
    train = strided_trainset(x, min(n, max_train_points_per_pq_code * k))
    err = 0.0
    for j in range(pq_dim):
        c = lloyd(train[:, j * pq_len:(j + 1) * pq_len], k, n_iters, rng)
        p = x[:, j * pq_len:(j + 1) * pq_len].astype(np.float64)
        d = (p * p).sum(1)[:, None] - 2.0 * p @ c.T + (c * c).sum(1)[None, :]
        err += float(np.maximum(d.min(1), 0).sum())
    return err / n
