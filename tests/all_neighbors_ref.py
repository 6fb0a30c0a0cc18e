"""numpy restatement of the all-neighbours build (cuvs_amd/csrc/all_neighbors.hip): inverted lists,
remap + merge, reachability epilogue, the shift and the batched pipeline. TEST INFRASTRUCTURE ONLY.

The batched pipeline takes the partition (the nearest-cluster matrix) as an input and the local exact kNN as a callback
`knn(rows, k) -> (distances [m, k], local ids [m, k])`, so nothing here depends on k-means."""
import numpy as np

I64_MAX = np.iinfo(np.int64).max
I64_MIN = np.iinfo(np.int64).min
F32_MAX = np.finfo(np.float32).max


def fill_values(select_min):
    """(id, distance) of a global slot that holds no neighbour yet."""
    return (I64_MAX, np.float32(F32_MAX)) if select_min else (I64_MIN, np.float32(-F32_MAX))


def float_key(d):
    """Order-preserving uint32 of float32 values (device_utils.hpp float_to_key): the total order the kernel sorts by.
    It refines `<` on floats only in putting -0.0 before +0.0."""
    u = np.ascontiguousarray(d, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def inverted_lists(nearest, n_clusters):
    """nearest [n, overlap] -> (inv [n * overlap], sizes, offsets): the rows of cluster c are
    inv[offsets[c] : offsets[c] + sizes[c]], ascending (get_inverted_indices)."""
    nearest = np.asarray(nearest, dtype=np.int64)
    sizes = np.bincount(nearest.ravel(), minlength=n_clusters).astype(np.int64)
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    inv = np.empty(nearest.size, np.int64)
    cur = offsets.copy()
    for i in range(nearest.shape[0]):
        for c in nearest[i]:
            inv[cur[c]] = i
            cur[c] += 1
    return inv, sizes, offsets


def remap_merge(inv, batch_i, batch_d, glob_i, glob_d, select_min=True):
    """One cluster's local graph into the global matrices, in place. Per cluster row b with g = inv[b]: the entries of
    glob[g] and of batch[b] (local ids mapped through inv; ids outside [0, m) are no entries) are ordered by (distance,
    id) - inner product: (-distance, id) -, an entry whose id appeared earlier in that order is dropped, the first k
    survivors are kept and the slots that remain hold the fill values."""
    inv = np.asarray(inv, dtype=np.int64)
    m, k = batch_i.shape
    fid, fd = fill_values(select_min)
    for b in range(m):
        g = inv[b]
        li = batch_i[b]
        ok = (li >= 0) & (li < m)
        ids = np.concatenate([glob_i[g], inv[np.where(ok, li, 0)][ok]])
        d = np.concatenate([glob_d[g], batch_d[b][ok]]).astype(np.float32)
        key = float_key(d if select_min else -d)
        order = np.lexsort((ids, key))
        ids, d = ids[order], d[order]
        _, first = np.unique(ids, return_index=True)  # the first occurrence of every id in that order
        keep = np.sort(first)[:k]
        glob_i[g] = fid
        glob_d[g] = fd
        glob_i[g, : len(keep)] = ids[keep]
        glob_d[g, : len(keep)] = d[keep]
    return glob_i, glob_d


def reach_epilogue(d, core_rows, core_cols, alpha):
    """d' = max(core[col], max(core[row], alpha * d)), all in float32."""
    v = np.float32(alpha) * np.asarray(d, dtype=np.float32)
    return np.maximum(core_cols[None, :].astype(np.float32), np.maximum(core_rows[:, None].astype(np.float32), v)).astype(np.float32)


def core_distances(distances):
    return np.ascontiguousarray(distances[:, -1], dtype=np.float32)


def shift(ids, d, first=None):
    """Rows one column to the right, the last column dropped; column 0 = (row id, first[row] or 0)."""
    n = ids.shape[0]
    oi = np.concatenate([np.arange(n, dtype=np.int64)[:, None], ids[:, :-1]], axis=1)
    col0 = np.zeros(n, np.float32) if first is None else np.asarray(first, dtype=np.float32)
    od = np.concatenate([col0[:, None], d[:, :-1]], axis=1).astype(np.float32)
    return oi, od


def batched_build(x, k, nearest, n_clusters, knn, select_min=True):
    """The batched pipeline: fill, then per cluster (ascending; clusters below k rows are skipped) gather, local kNN,
    remap + merge. knn(rows, inv_c, k) -> (distances, local ids)."""
    n = x.shape[0]
    inv, sizes, offsets = inverted_lists(nearest, n_clusters)
    fid, fd = fill_values(select_min)
    gi = np.full((n, k), fid, np.int64)
    gd = np.full((n, k), fd, np.float32)
    for c in range(n_clusters):
        if sizes[c] < k:
            continue
        inv_c = inv[offsets[c] : offsets[c] + sizes[c]]
        bd, bi = knn(x[inv_c], inv_c, k)
        remap_merge(inv_c, bi, bd, gi, gd, select_min)
    return gi, gd


def slow_merge(inv, batch_i, batch_d, glob_i, glob_d, select_min=True):
    """The same merge by plain Python sets and tuples (no -0.0 in the inputs): the check of remap_merge itself."""
    m, k = batch_i.shape
    fid, fd = fill_values(select_min)
    out_i, out_d = glob_i.copy(), glob_d.copy()
    for b in range(m):
        g = int(inv[b])
        ent = [(float(glob_d[g, j]), int(glob_i[g, j])) for j in range(k)]
        ent += [(float(batch_d[b, j]), int(inv[batch_i[b, j]])) for j in range(k) if 0 <= batch_i[b, j] < m]
        ent.sort(key=lambda e: (e[0] if select_min else -e[0], e[1]))
        seen, kept = set(), []
        for dist, idx in ent:
            if idx not in seen:
                seen.add(idx)
                kept.append((dist, idx))
        kept = kept[:k]
        for j in range(k):
            out_d[g, j], out_i[g, j] = kept[j] if j < len(kept) else (fd, fid)
    return out_i, out_d
