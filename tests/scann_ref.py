"""The numpy twin of the ScaNN build (cuvs_amd/csrc/scann.hip): AVQ centres, SOAR labels, bf16 rows with noise
shaping, and the index files. fp32 chains are the exact fmaf of ivf_sq_ref.py, k ascending, one accumulator from 0."""
import numpy as np

from tests.ivf_sq_ref import fmaf

F32, F64 = np.float32, np.float64
MAX_ROUNDS = 10


def uniform(n, dim, seed, lo=0.1, hi=2.0):
    return np.random.default_rng(seed).uniform(lo, hi, (n, dim)).astype(F32)


def chain(u, v):
    """rowwise chain(u_i, v_i): fp32 [n]"""
    u, v = np.broadcast_arrays(np.asarray(u, F32), np.asarray(v, F32))
    acc = np.zeros(u.shape[:-1], F32)
    for k in range(u.shape[-1]):
        acc = fmaf(u[..., k], v[..., k], acc)
    return acc


def chain_pairs(u, v):
    """chain(u_i, v_j) of every pair: fp32 [n, m]"""
    u, v = np.asarray(u, F32), np.asarray(v, F32)
    acc = np.zeros((len(u), len(v)), F32)
    for k in range(u.shape[1]):
        acc = fmaf(np.broadcast_to(u[:, k][:, None], acc.shape), np.broadcast_to(v[:, k][None, :], acc.shape), acc)
    return acc


def nearest_labels(x, centers):
    """the fp64 nearest centre (what a partition looks like; the device's own predict has its own parity tests)"""
    d = ((x.astype(F64)[:, None, :] - centers.astype(F64)[None, :, :]) ** 2).sum(-1)
    return d.argmin(1).astype(np.int32)


# ---------------------------------------------------------------------------------------------- AVQ centres
def avq_weights(x, eta, T):
    x = x.astype(T)
    nrm = np.sqrt((x * x).sum(1))
    with np.errstate(divide="ignore", invalid="ignore"):
        w1 = np.where(nrm > 0, nrm ** T(eta - 1), 0).astype(T)
        w3 = np.where(nrm > 0, nrm ** T(eta - 3), 0).astype(T)
    return w1, w3


def avq_system(xc, w1, w3, eta, T):
    S = w1.sum(dtype=T)
    A = S * np.eye(xc.shape[1], dtype=T) + T(eta - 1) * ((xc * w3[:, None]).T @ xc)
    b = (w1[:, None] * xc).sum(0, dtype=T)
    return S, A.astype(T), b.astype(T)


def avq_centers(x, labels, centers, eta, T=F64):
    """(centres, rescale, unrescaled centres, condition numbers): the formulas of DESIGN 3.1z in precision T, vectorised numpy
    (np.linalg.solve). T = float64 is the reference of the tests, T = float32 the plain restatement that sets their tolerance."""
    x = np.asarray(x).astype(T)
    out = np.asarray(centers).astype(T).copy()
    w1, w3 = avq_weights(x, eta, T)
    num, den = T(0), T(0)
    updated, conds = [], []
    for c in range(len(out)):
        idx = np.flatnonzero(labels == c)
        if len(idx) == 0 or not w1[idx].sum() > 0:
            continue
        S, A, b = avq_system(x[idx], w1[idx], w3[idx], eta, T)
        out[c] = T(eta) * (b / S if eta == 1 else np.linalg.solve(A, b))
        conds.append(float(np.linalg.cond(A.astype(F64))))
        updated.append(c)
    raw = out.copy()
    for c in updated:
        idx = np.flatnonzero(labels == c)
        num += x[idx].sum(0, dtype=T) @ out[c]
        den += T(len(idx)) * (out[c] @ out[c])
    with np.errstate(divide="ignore", invalid="ignore"):
        r = num / den
    r = T(r) if den != 0 and np.isfinite(den) and np.isfinite(r) else T(1)
    out[updated] = out[updated] * r
    return out, r, raw, conds


def avq_gradient(x, labels, c_raw, eta, leaf):
    """gradient (up to the factor -2) of sum_i w1_i (|r_i|^2 + (eta - 1) <r_i, x_i>^2 / |x_i|^2), r_i = x_i - c, at c = c_raw[leaf],
    and the size of its terms; fp64"""
    x = x.astype(F64)
    idx = np.flatnonzero(labels == leaf)
    w1, w3 = avq_weights(x, eta, F64)
    r = x[idx] - c_raw[leaf]
    terms = w1[idx, None] * r + (eta - 1) * w3[idx, None] * x[idx] * (x[idx] * r).sum(1)[:, None]
    return terms.sum(0), np.abs(terms).sum(0)


def avq_means_chain32(x, labels, centers):
    """eta = 1 exactly as the device computes it: per leaf the members in ascending row id, sum = sum + x (what fmaf(1, x, sum) is),
    S = the count of non-zero rows as a sequential fp32 sum, centre = sum / S, then the rescale: per leaf chain(sum x, centre) and
    n * chain(centre, centre), both sums in fp64 leaf by leaf, the quotient rounded to fp32"""
    x = np.asarray(x, F32)
    out = np.asarray(centers, F32).copy()
    nz = (x != 0).any(1)
    num, den, updated = 0.0, 0.0, []
    for c in range(len(out)):
        idx = np.flatnonzero(labels == c)
        S = F32(0)
        sx = np.zeros(x.shape[1], F32)
        b = np.zeros(x.shape[1], F32)
        for i in idx:
            w = F32(1) if nz[i] else F32(0)
            S = F32(S + w)
            b = fmaf(np.full(x.shape[1], w, F32), x[i], b)
            sx = (sx + x[i]).astype(F32)
        if not S > 0:
            continue
        out[c] = (b / S).astype(F32)
        num += float(chain(sx[None], out[c][None])[0])
        den += float(F32(F32(len(idx)) * chain(out[c][None], out[c][None])[0]))
        updated.append(c)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = F32(np.float64(num) / np.float64(den)) if updated else F32(np.nan)
    r = r if den != 0 and np.isfinite(den) and np.isfinite(r) else F32(1)
    out[updated] = (out[updated] * r).astype(F32)
    return out, r


# ---------------------------------------------------------------------------------------------- SOAR labels
def soar_parts(x, centers, labels):
    """what does not depend on lambda: (t = a - p [n, n_leaves], -2 b, cn, nr)"""
    x, centers = np.asarray(x, F32), np.asarray(centers, F32)
    r = (x - centers[labels]).astype(F32)
    nr = np.sqrt(chain(r, r)).astype(F32)
    with np.errstate(divide="ignore", invalid="ignore"):
        rh = np.where(nr[:, None] == 0, F32(0), r / nr[:, None]).astype(F32)
    p = chain(rh, x)
    a, b, cn = chain_pairs(rh, centers), chain_pairs(x, centers), chain(centers, centers)
    return (a - p[:, None]).astype(F32), (F32(-2) * b).astype(F32), cn, nr


def soar_scores(x, centers, labels, lam, parts=None):
    """fp32 scores [n, n_leaves] in the canonical arithmetic"""
    t, m2b, cn, nr = parts if parts is not None else soar_parts(x, centers, labels)
    s = ((t * t).astype(F32) * F32(lam)).astype(F32)
    s = (s + m2b).astype(F32)
    return (s + cn[None, :]).astype(F32), nr


def soar_labels(x, centers, labels, lam, parts=None):
    s, _ = soar_scores(x, centers, labels, lam, parts)
    return s.argmin(1).astype(np.int32)  # numpy's argmin returns the first of equal minima


def soar_scores64(x, centers, labels, lam):
    """|r'|^2 + lambda <rh, r'>^2 with r' = x - c_j, in fp64 (Theorem 3.1 of arXiv 2404.00774)"""
    x, centers = x.astype(F64), centers.astype(F64)
    r = x - centers[labels]
    nr = np.sqrt((r * r).sum(1))
    with np.errstate(divide="ignore", invalid="ignore"):
        rh = np.where(nr[:, None] == 0, 0.0, r / nr[:, None])
    rp = x[:, None, :] - centers[None, :, :]
    return (rp * rp).sum(-1) + lam * (rp * rh[:, None, :]).sum(-1) ** 2


# ---------------------------------------------------------------------------------------------- bf16 rows
def bf16_rne_bits(x):
    """round to nearest even on the bit pattern: uint16"""
    u = np.asarray(x, F32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16)


def bf16_value(bits):
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(F32)


def wave_sum(partials):
    """the butterfly over 64 partials: p[i] += p[i + off], off = 32 .. 1; partials [n, 64] fp32"""
    p = partials.astype(F32).copy()
    off = 32
    while off > 0:
        p[:, :off] = (p[:, :off] + p[:, off:2 * off]).astype(F32)
        off //= 2
    return p[:, 0]


def strided_chain(u, v):
    """lane l: acc = fmaf(u_d, v_d, acc) over d = l, l + 64, ...; then the butterfly"""
    n, dim = u.shape
    part = np.zeros((n, 64), F32)
    for d in range(dim):
        part[:, d % 64] = fmaf(u[:, d], v[:, d], part[:, d % 64])
    return wave_sum(part)


def bf16_neighbor(qb, x):
    """(bits of the bf16 neighbour of q on the other side of x, whether there is one)"""
    q = bf16_value(qb)
    neg = (qb >> 15) != 0
    away = (q < x) != neg
    can = away | ((qb & 0x7FFF) != 0)
    nb = np.where(away, qb.astype(np.int32) + 1, qb.astype(np.int32) - 1).astype(np.int32) & 0xFFFF
    nb = nb.astype(np.uint16)
    ok = (q != x) & can & ((nb & 0x7F80) != 0x7F80)
    return nb, ok


def quantize_bf16(x, threshold=float("nan"), history=None):
    """int16 [n, dim]: the bf16 bits of the rows. `history`, a list, receives the bits after plain rounding and after every round."""
    x = np.ascontiguousarray(x, F32)
    n, dim = x.shape
    qb = bf16_rne_bits(x)
    if history is not None:
        history.append(qb.copy())
    T = F32(threshold)
    if np.isnan(T) or n == 0:
        return qb.view(np.int16)
    sq = strided_chain(x, x)
    t2 = F32(T * T)
    rows = np.flatnonzero((sq > t2) & (sq != 0))
    if len(rows) == 0:
        return qb.view(np.int16)
    xs, q = x[rows], qb[rows]
    sqs = sq[rows]
    nrm = np.sqrt(sqs).astype(F32)
    ratio = (t2 / sqs).astype(F32)
    em1 = (((F32(dim - 1) * ratio).astype(F32) / (F32(1) - ratio).astype(F32)).astype(F32) - F32(1)).astype(F32)
    D = (strided_chain((xs - bf16_value(q)).astype(F32), xs) / nrm).astype(F32)
    active = np.ones(len(rows), bool)  # rows whose last round changed something
    for _ in range(MAX_ROUNDS):
        changed = np.zeros(len(rows), bool)
        for d in range(dim):
            xd, qd = xs[:, d], bf16_value(q[:, d])
            nb, ok = bf16_neighbor(q[:, d], xd)
            qn = bf16_value(nb)
            e0, e1 = (xd - qd).astype(F32), (xd - qn).astype(F32)
            with np.errstate(all="ignore"):
                delta = (((e1 - e0).astype(F32) * xd).astype(F32) / nrm).astype(F32)
                A = ((F32(2) * em1).astype(F32) * delta).astype(F32)
                B = (((e1 * e1).astype(F32) - (e0 * e0).astype(F32)).astype(F32) + (em1 * (delta * delta).astype(F32)).astype(F32)).astype(F32)
                take = active & ok & (((A * D).astype(F32) + B).astype(F32) < 0)
            D = np.where(take, (D + delta).astype(F32), D)
            q[:, d] = np.where(take, nb, q[:, d])
            changed |= take
        active = active & changed
        qb[rows] = q
        if history is not None:
            history.append(qb.copy())
        if not active.any():
            break
    return qb.view(np.int16)


def avq_row_loss(x, bits, threshold):
    """fp64: (eta_x |r_par|^2 + |r_perp|^2 of every row, r = x - q (rows at or below the threshold: |r|^2), the sum of the absolute
    values of the two terms it is evaluated from: its own rounding error is a few 2^-53 of that)"""
    x64 = x.astype(F64)
    r = x64 - bf16_value(np.asarray(bits).view(np.uint16)).astype(F64)
    sq = (x64 * x64).sum(1)
    t2 = float(threshold) ** 2
    with np.errstate(divide="ignore", invalid="ignore"):
        eta = np.where(sq > t2, (x.shape[1] - 1) * (t2 / sq) / (1 - t2 / sq), 1.0)
        par = np.where(sq > 0, (r * x64).sum(1) ** 2 / sq, 0.0)
    return (r * r).sum(1) + (eta - 1) * par, (r * r).sum(1) + np.abs(eta - 1) * par


# ---------------------------------------------------------------------------------------------- index files
def interleave_labels(labels, soar):
    out = np.empty(2 * len(labels), np.int32)
    out[0::2] = labels
    out[1::2] = np.where(soar == labels, -1, soar)
    return out


def sub_books(codebook, pq_dim):
    """index codebook [2^bits, dim] -> the product quantizer's layout [n_sub * 2^bits, pq_dim] (entry e of subspace j at j * 2^bits + e)"""
    book_n, dim = codebook.shape
    n_sub = dim // pq_dim
    return np.ascontiguousarray(codebook.reshape(book_n, n_sub, pq_dim).transpose(1, 0, 2).reshape(n_sub * book_n, pq_dim))


def read_metadata(path):
    """the three 0-d .npy records of cuvs_metadata.bin"""
    with open(path, "rb") as f:
        out = [np.load(f) for _ in range(3)]
        assert f.read() == b""
    return out
