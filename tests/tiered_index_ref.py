"""numpy restatement of the tiered index (cuvs_amd/csrc/tiered_index.hip): the merge of the two tiers, the
tail's exact top-k in the form the library hands it out, and the growth policy of the storage. TEST INFRASTRUCTURE ONLY."""
import numpy as np

I64_MAX = np.iinfo(np.int64).max
F32_MAX = np.finfo(np.float32).max


def worst(select_min):
    return np.float32(F32_MAX) if select_min else np.float32(-F32_MAX)


def float_key(d):
    """Order-preserving uint32 of float32 values (device_utils.hpp float_to_key): the total order the kernels sort by. It
    refines `<` on floats only in putting -0.0 before +0.0."""
    u = np.ascontiguousarray(d, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def merge(a, b, ann_rows, select_min=True):
    """a = (distances [m, k], ids [m, k]): an ANN result over rows [0, ann_rows); an entry is real iff 0 <= id < ann_rows,
    whatever its distance. b = (distances [m, kb], ids [m, kb]): entries with id INT64_MAX (or negative) are padding.
    Returns (distances, ids) [m, k]: the first k of the union of the real entries by (distance, id) - inner product:
    (-distance, id) -, the slots that remain INT64_MAX / the worst value."""
    ad, ai = np.asarray(a[0], np.float32), np.asarray(a[1], np.int64)
    bd, bi = np.asarray(b[0], np.float32), np.asarray(b[1], np.int64)
    m, k = ai.shape
    out_d = np.full((m, k), worst(select_min), np.float32)
    out_i = np.full((m, k), I64_MAX, np.int64)
    for r in range(m):
        ra = (ai[r] >= 0) & (ai[r] < ann_rows)
        rb = (bi[r] >= 0) & (bi[r] != I64_MAX)
        ids = np.concatenate([ai[r][ra], bi[r][rb]])
        d = np.concatenate([ad[r][ra], bd[r][rb]]).astype(np.float32)
        order = np.lexsort((ids, float_key(d if select_min else -d)))[:k]
        out_i[r, : len(order)] = ids[order]
        out_d[r, : len(order)] = d[order]
    return out_d, out_i


def globalize(d, i, ann_rows, select_min=True):
    """A brute-force result over the tail rows alone (oracle.brute_force_knn: missing slots -1, filtered rows the worst value)
    -> the form of the tail tier: global ids, INT64_MAX / the worst value where no admissible row stands."""
    d = np.array(d, np.float32)
    i = np.array(i, np.int64)
    pad = (i < 0) | (d == worst(select_min))
    i = np.where(pad, I64_MAX, i + ann_rows)
    d = np.where(pad, worst(select_min), d).astype(np.float32)
    return d, i


def tail_bits(bits, ann_rows, n_tail):
    """The tail's slice of a bitset over global ids as uint32 words that count from 0 (what a brute force over the tail alone
    reads)."""
    bits = np.asarray(bits, dtype=np.uint32)
    g = np.arange(ann_rows, ann_rows + n_tail, dtype=np.int64)
    keep = (bits[g >> 5] >> (g & 31).astype(np.uint32)) & np.uint32(1)
    out = np.zeros((n_tail + 31) // 32, np.uint32)
    j = np.arange(n_tail, dtype=np.int64)
    np.bitwise_or.at(out, j >> 5, (keep << (j & 31).astype(np.uint32)).astype(np.uint32))
    return out


def initial_capacity(n):
    return n + n // 16


def grown_capacity(size, capacity, new_rows):
    """Capacity after appending new_rows to `size` rows held in an allocation of `capacity` rows."""
    if size + new_rows <= capacity:
        return capacity
    return max(size + new_rows, 2 * capacity)


def builds_ann(n, min_ann_rows):
    return n > min_ann_rows


def pack_bits(keep):
    """bool [n] -> uint32 words, bit i = keep[i]."""
    keep = np.asarray(keep, dtype=bool)
    out = np.zeros((len(keep) + 31) // 32, np.uint32)
    j = np.nonzero(keep)[0]
    np.bitwise_or.at(out, j >> 5, (np.uint32(1) << (j & 31).astype(np.uint32)).astype(np.uint32))
    return out
