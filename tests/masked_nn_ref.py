"""Plain numpy reference of cuvs_amd.distance.masked_l2_nn and cross_component_nn in fp64: every distance, then the mask, then
the argmin with ties to the smaller index (np.argmin takes the first minimum). DESIGN 3.1zb."""
import numpy as np

FLT_MAX = np.float32(np.finfo(np.float32).max)
U = 2.0 ** -24


def sqdist64(x, y):
    x, y = x.astype(np.float64), y.astype(np.float64)
    return ((x[:, None, :] - y[None, :, :]) ** 2).sum(-1)


def groups_of(n, ends):
    """group of every row of y (-1: past the last end)"""
    g = np.searchsorted(ends, np.arange(n), side="right")
    return np.where(g < len(ends), g, -1)


def admissible(adj, ends, n):
    g = groups_of(n, ends)
    return adj.astype(bool)[:, np.maximum(g, 0)] & (g >= 0)[None, :]


def nearest(d, ok):
    """(idx int64, d64 of the pick or inf) of every row over the admissible columns"""
    dm = np.where(ok, d, np.inf)
    idx = dm.argmin(1)
    best = dm[np.arange(len(dm)), idx] if dm.shape[1] else np.full(len(dm), np.inf)
    return np.where(np.isinf(best), -1, idx).astype(np.int64), best


def as_output(best, sqrt):
    """fp32 output of exact (integer) squared distances"""
    out = np.where(np.isinf(best), 0.0, best).astype(np.float32)
    out = np.sqrt(out) if sqrt else out  # (np.sqrt of fp32 is the correctly rounded fp32 root)
    return np.where(np.isinf(best), FLT_MAX, out).astype(np.float32)


def masked_l2_nn(x, y, adj, ends, sqrt=False):
    idx, best = nearest(sqdist64(x, y), admissible(adj, ends, len(y)))
    return idx, as_output(best, sqrt)


def bound(x, y, d64):
    """|d_device - d64| <= B: the dot chain of length dim (gamma_dim |x||y| <= gamma_dim (xn + yn) / 2, twice), the two norms
    (64 strided chains and a 6-step butterfly: depth ceil(dim / 64) + 6), their sum, and the rounding of the fma's result;
    1 % for the second-order terms. The clamp at 0 moves towards d64 >= 0."""
    dim = x.shape[1]
    xn, yn = (x.astype(np.float64) ** 2).sum(1), (y.astype(np.float64) ** 2).sum(1)
    return 1.01 * U * ((dim + -(-dim // 64) + 8) * (xn[:, None] + yn[None, :]) + d64)


def int_rows(rng, n, dim):
    return rng.integers(-3, 4, (n, dim)).astype(np.float32)


def masked_case(m, n, dim, G, density, seed=0):
    """integer rows, group ends and a mask with, where the shape has room: group_idxs[-1] < n, an empty group, an all-false row,
    rows 0..127 switched off for every group that meets columns 128..255 (a dead tile) and for one more group"""
    rng = np.random.default_rng(seed + 7 * m + n)
    last = n - 1 if n > 1 else n
    ends = np.sort(np.append(rng.integers(0, last + 1, G - 1), last)).astype(np.int64)
    if G >= 3:
        ends[1] = ends[0]
    adj = rng.random((m, G)) < density
    g = groups_of(n, ends)
    if n > 128:
        dead = g[128:min(n, 256)]
        adj[:128, np.unique(dead[dead >= 0])] = False
    if G > 1:
        adj[:128, G // 2] = False
    adj[m // 2] = m == 1  # an all-false row (the only row of a 1 x 1 problem stays on)
    return int_rows(rng, m, dim), int_rows(rng, n, dim), adj, ends


def cross_component_nn(x, colors, n_components, sqrt=False):
    d = sqdist64(x, x)
    idx, best = nearest(d, colors[:, None] != colors[None, :])
    src, dst = np.full(n_components, -1, np.int64), np.full(n_components, -1, np.int64)
    w = np.full(n_components, np.inf)
    for c in range(n_components):
        rows = [(best[i], i, idx[i]) for i in np.flatnonzero(colors == c) if idx[i] >= 0]
        if rows:
            w[c], src[c], dst[c] = min(rows)
    return idx, as_output(best, sqrt), src, dst, as_output(w, sqrt)
