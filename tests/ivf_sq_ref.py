"""Independent numpy restatement of IVF-SQ, used only by the tests: the quantizer, the encoder, the search arithmetic of
DESIGN 3.2 (with an exact fp32 fma) and the reference's file container (ivf_sq_serialize.cuh).

The coarse search is the repository's CPU oracle (the same pairwise distances and tie rule as the IVF-Flat oracle)."""
import io

import numpy as np

from tests import refformat as R

F32, F64 = np.float32, np.float64
METRICS = {"sqeuclidean": 0, "euclidean": 1, "cosine": 2, "inner_product": 6}
METRIC_NAMES = {v: k for k, v in METRICS.items()}


# ---------------------------------------------------------------------------------------------- fp32 arithmetic
def fmaf(a, b, c):
    """Correctly rounded fp32 fma, elementwise. The f64 product of two fp32 values is exact; the f64 sum is rounded to odd
    (TwoSum error term), so that the final rounding to fp32 is not a double rounding."""
    a64 = np.asarray(a, F32).astype(F64)
    b64 = np.asarray(b, F32).astype(F64)
    c64 = np.asarray(c, F32).astype(F64)
    p = a64 * b64
    s = p + c64
    bp = s - c64
    e = (p - bp) + (c64 - (s - bp))
    bits = np.asarray(s).view(np.int64)
    need = (e != 0) & ((bits & 1) == 0)
    toward = np.where(np.signbit(e) == np.signbit(s), 1, -1).astype(np.int64)
    odd = np.where(need, bits + toward, bits).view(F64)
    return odd.astype(F32)


def roundf(x):
    """C roundf: half away from zero (exact in f64 for fp32 inputs)."""
    x = np.asarray(x, F32).astype(F64)
    return (np.sign(x) * np.floor(np.abs(x) + 0.5)).astype(F32)


def f2k(v):
    """order-preserving uint32 key of fp32 values (device_utils.hpp float_to_key)"""
    u = np.asarray(v, F32).view(np.uint32).astype(np.uint64)
    return np.where(u & 0x80000000, (~u) & 0xFFFFFFFF, u | 0x80000000).astype(np.uint64)


# ---------------------------------------------------------------------------------------------- quantizer + encoder
def residuals(x, centers, labels, dtype):
    r = np.asarray(x).astype(F32) - centers[labels]
    if np.dtype(dtype) == np.float16:
        r = r.astype(np.float16).astype(F32)
    return r


def quantizer(resid):
    """per-dimension vmin, delta from training residuals (ivf_sq_build.cuh: 5 % margin, 255 steps)"""
    lo = resid.min(axis=0).astype(F32)
    hi = resid.max(axis=0).astype(F32)
    rng = (hi - lo).astype(F32)
    margin = (rng * F32(0.05)).astype(F32)
    delta = np.where(rng > 0, ((rng + F32(2.0) * margin).astype(F32) / F32(255.0)).astype(F32), F32(1.0)).astype(F32)
    vmin = (lo - margin).astype(F32)
    return vmin, delta


def encode(x, center, vmin, delta):
    """codes of rows x [n, dim] against one centre (or [n, dim] centres)"""
    val = np.asarray(x).astype(F32) - np.asarray(center, F32)
    t = ((val - vmin).astype(F32) / delta).astype(F32)
    return np.clip(roundf(t), 0, 255).astype(np.uint8)


# ---------------------------------------------------------------------------------------------- search
def coarse_probes(q, centers, metric, n_probes):
    import oracle

    if metric in ("sqeuclidean", "euclidean"):
        d = oracle.pairwise(q, centers, "sqeuclidean")
        keys = f2k(d)
    elif metric == "cosine":
        d = oracle.pairwise(q, centers, "cosine")
        keys = f2k(d)
    else:
        d = oracle.pairwise(q, centers, "inner_product")
        keys = (~f2k(d).astype(np.uint64)) & 0xFFFFFFFF
    n_lists = centers.shape[0]
    cols = np.broadcast_to(np.arange(n_lists, dtype=np.uint64), keys.shape)
    order = np.lexsort((cols, keys), axis=1)
    return order[:, :n_probes]


def list_scores(qs, codes, center, vmin, delta, metric, qnorm=None):
    """scores [len(qs), len(codes)] of one list, smaller is better"""
    qs = np.asarray(qs, F32)
    x = codes.astype(F32)
    nq, n = qs.shape[0], x.shape[0]
    acc = np.zeros((nq, n), F32)
    dim = qs.shape[1]
    if metric in ("sqeuclidean", "euclidean"):
        qt = ((qs - vmin).astype(F32) - center).astype(F32)
        for d in range(dim):
            diff = fmaf(-x[None, :, d], delta[d], qt[:, d, None])
            acc = fmaf(diff, diff, acc)
        return acc
    aux = (center + vmin).astype(F32)
    vn = np.zeros(n, F32)
    for d in range(dim):
        v = fmaf(x[:, d], delta[d], aux[d])
        acc = fmaf(qs[:, d, None], v[None, :], acc)
        vn = fmaf(v, v, vn)
    if metric == "inner_product":
        return (-acc).astype(F32)
    denom = (qnorm[:, None] * np.sqrt(vn)[None, :]).astype(F32)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(denom > 0, (F32(1.0) - (acc / denom).astype(F32)).astype(F32), F32(0.0))
    return s.astype(F32)


def search(exported, queries, k, n_probes, metric, keep_bits=None):
    """(distances, neighbors) of cuvsIvfSqSearch on an exported index (cuvs_amd.neighbors.ivf_sq.export_for_oracle).
    Candidates of all probes: the k best by (score key, probe rank, in-list position), reported in (score key, flat row)
    order; filtered rows never enter; missing slots: FLT_MAX / INT64_MAX."""
    import oracle

    q = np.asarray(queries).astype(F32)
    nq = q.shape[0]
    centers, vmin, delta = exported["centers"], exported["vmin"], exported["delta"]
    sizes = np.asarray(exported["list_sizes"], np.int64)
    n_lists = len(sizes)
    n_probes = min(n_probes, n_lists)
    start = np.zeros(n_lists + 1, np.int64)
    np.cumsum(sizes, out=start[1:])
    probes = coarse_probes(q, centers, metric, n_probes)
    qnorm = oracle.row_norms(q, sqrt=True) if metric == "cosine" else None
    per_q = [[] for _ in range(nq)]
    for L in range(n_lists):
        qi, rank = np.nonzero(probes == L)
        if len(qi) == 0 or sizes[L] == 0:
            continue
        s = list_scores(q[qi], exported["codes"][L], centers[L], vmin, delta, metric, None if qnorm is None else qnorm[qi])
        ids = exported["ids"][L]
        keep = np.ones(len(ids), bool)
        if keep_bits is not None:
            keep = ((keep_bits[ids >> 5] >> (ids & 31).astype(np.uint32)) & 1).astype(bool)
        pos = np.nonzero(keep)[0]
        for j in range(len(qi)):
            per_q[qi[j]].append((s[j, pos], np.full(len(pos), rank[j]), pos, start[L] + pos, ids[pos]))
    out_d = np.full((nq, k), np.finfo(F32).max, F32)
    out_i = np.full((nq, k), np.iinfo(np.int64).max, np.int64)
    for i in range(nq):
        if not per_q[i]:
            continue
        s, rk, pos, flat, ids = (np.concatenate(c) for c in zip(*per_q[i]))
        key = f2k(s)
        sel = np.lexsort((pos, rk, key))[:k]
        sel = sel[np.lexsort((flat[sel], key[sel]))]
        d = s[sel]
        if metric == "inner_product":
            d = -d
        elif metric == "euclidean":
            d = np.sqrt(d)
        out_d[i, :len(sel)] = d
        out_i[i, :len(sel)] = ids[sel]
    return out_d, out_i


# ---------------------------------------------------------------------------------------------- file container
def _interleave(codes, rows32, dim_pad):
    """[n, dim] codes -> the reference's list record [rows32, dim_pad]: 32-row groups of 16-byte chunks"""
    n, dim = codes.shape
    padded = np.zeros((rows32, dim_pad), np.uint8)
    padded[:n, :dim] = codes
    g = padded.reshape(rows32 // 32, 32, dim_pad // 16, 16).transpose(0, 2, 1, 3)
    return np.ascontiguousarray(g).reshape(rows32, dim_pad)


def _deinterleave(rec, n, dim):
    rows32, dim_pad = rec.shape
    g = rec.reshape(rows32 // 32, dim_pad // 16, 32, 16).transpose(0, 2, 1, 3).reshape(rows32, dim_pad)
    return np.ascontiguousarray(g[:n, :dim])


def write_file(path, centers, vmin, delta, codes, ids, metric=0, center_norms=None, conservative=False):
    """codes / ids: one [size, dim] uint8 array and one int64 array per list"""
    n_lists, dim = centers.shape
    dim_pad = (dim + 15) // 16 * 16
    sizes = np.array([len(i) for i in ids], np.uint32)
    with open(path, "wb") as f:
        f.write(b"|u1\0")
        R.write_scalar(f, 1, np.int32)
        R.write_scalar(f, int(sizes.sum()), np.int64)
        R.write_scalar(f, dim, np.uint32)
        R.write_scalar(f, n_lists, np.uint32)
        R.write_scalar(f, metric, np.int32)
        R.write_scalar(f, conservative, np.bool_)
        R.write_record(f, np.asarray(centers, F32))
        R.write_scalar(f, center_norms is not None, np.bool_)
        if center_norms is not None:
            R.write_record(f, np.asarray(center_norms, F32))
        R.write_record(f, np.asarray(vmin, F32))
        R.write_record(f, np.asarray(delta, F32))
        R.write_record(f, sizes)
        for L in range(n_lists):
            rows32 = (int(sizes[L]) + 31) // 32 * 32
            R.write_scalar(f, rows32, np.uint32)
            if rows32 == 0:
                continue
            R.write_record(f, _interleave(np.asarray(codes[L], np.uint8), rows32, dim_pad))
            pid = np.full(rows32, -1, np.int64)
            pid[:sizes[L]] = ids[L]
            R.write_record(f, pid)


def parse_file(path):
    with open(path, "rb") as fh:
        f = io.BytesIO(fh.read())
    prefix = f.read(4)
    assert prefix == b"|u1\0", prefix
    out = dict(version=R.scalar(f), size=R.scalar(f), dim=R.scalar(f), n_lists=R.scalar(f), metric=R.scalar(f),
               conservative=bool(R.scalar(f)))
    out["centers"] = R.read_record(f)
    out["center_norms"] = R.read_record(f) if R.scalar(f) else None
    out["vmin"] = R.read_record(f)
    out["delta"] = R.read_record(f)
    out["list_sizes"] = R.read_record(f)
    out["codes"], out["ids"] = [], []
    for L in range(out["n_lists"]):
        rows32 = R.scalar(f)
        n = int(out["list_sizes"][L])
        if rows32 == 0:
            out["codes"].append(np.zeros((0, out["dim"]), np.uint8))
            out["ids"].append(np.zeros(0, np.int64))
            continue
        out["codes"].append(_deinterleave(R.read_record(f), n, out["dim"]))
        out["ids"].append(R.read_record(f)[:n])
    assert f.read() == b""
    return out
