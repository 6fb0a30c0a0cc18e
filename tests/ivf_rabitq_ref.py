"""numpy restatement of IVF-RaBitQ (cuvs_amd/csrc/ivf_rabitq.hip), written from the contract of DESIGN.md 3.1s: codes and
factors, the scaling factor t, the two-stage search, the file. fp32 throughout; every product and every sum is rounded on
its own (the library is built without fp contraction), and every reduction over the dimensions has the kernels' order:
lane l of 64 adds the terms of dimensions l, l + 64, ... in that order, then the 64 partials are combined by the xor
butterfly 32, 16, 8, 4, 2, 1. Rotations go through oracle.pairwise (the k-ordered fma chain of the distance GEMM)."""
import io

import numpy as np

F32 = np.float32
F64 = np.float64
EPSILON = F32(1.9)
MODES = ("lut16", "lut32", "quant4", "quant8")
_LANES = np.arange(64)


def padded_dim(dim):
    return (dim + 63) // 64 * 64


def pad(x, D):
    x = np.asarray(x, F32)
    out = np.zeros((x.shape[0], D), F32)
    out[:, :x.shape[1]] = x
    return out


def rotate(x, rotation):
    """x' = P pad(x): row i of the result holds the dot products of pad(x_i) with the rows of P"""
    import oracle

    rotation = np.asarray(rotation, F32)
    return oracle.pairwise(pad(x, rotation.shape[1]), rotation, "inner_product")


def lane_sum(terms):
    """sum over the last axis (a multiple of 64 long) in the kernels' order"""
    t = np.asarray(terms, F32)
    t = t.reshape(t.shape[:-1] + (t.shape[-1] // 64, 64))
    acc = np.zeros(t.shape[:-2] + (64,), F32)
    for i in range(t.shape[-2]):
        acc = acc + t[..., i, :]
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[..., _LANES ^ o]
    return np.ascontiguousarray(acc[..., 0])


# ------------------------------------------------------------------------------------------------ the scaling factor t
_TIGHT_START = (0, 0.15, 0.20, 0.52, 0.59, 0.71, 0.75, 0.77, 0.81)
_T_CACHE = {}


def _splitmix64(i, seed):
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + (i + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def best_rescale_factor(o, ex_bits):
    """the rescale factor t that maximises <o, o_bar(t)> / |o_bar(t)| for o_bar = floor(t o + 1e-5) + 1/2 clipped to 2^ex levels: every
    t at which one component steps up is an event; events in (t, component) order"""
    dim, top = o.shape[0], (1 << ex_bits) - 1
    t_end = F64(top + 10) / o.max()
    t_start = t_end * F64(_TIGHT_START[ex_bits])
    cur = (t_start * o + F64(1e-5)).astype(np.int64)
    den0 = F64(dim) * F64(0.25) + F64(np.sum(cur * cur + cur))
    num0 = np.add.accumulate((cur.astype(F64) + F64(0.5)) * o)[-1]
    u = cur[:, None] + 1 + np.arange(top + 1)[None, :]
    with np.errstate(divide="ignore"):
        tu = u.astype(F64) / o[:, None]
    keep = (np.arange(top + 1)[None, :] == 0) | ((u <= top) & (tu < t_end))
    comp = np.broadcast_to(np.arange(dim)[:, None], u.shape)[keep]
    tu, u = tu[keep], u[keep]
    order = np.lexsort((comp, tu))
    tu, u, comp = tu[order], u[order], comp[order]
    den = den0 + np.cumsum(2.0 * u.astype(F64))
    num = np.add.accumulate(np.concatenate([[num0], o[comp]]))[1:]
    ip = num / np.sqrt(den)
    best = int(np.argmax(ip))
    return tu[best] if ip[best] > 0 else F64(0)


def scaling_factor(D, ex_bits):
    """t(D, ex): the mean best rescale factor over 100 unit vectors of this library's fixed-seed generator (splitmix64, twelve
    32-bit uniforms summed per component), as cuvs_amd/csrc/ivf_rabitq_host.hpp computes it"""
    if ex_bits == 0:
        return F32(0)
    if (D, ex_bits) in _T_CACHE:
        return _T_CACHE[(D, ex_bits)]
    seed = 0x7261626974710000 + D * 16 + ex_bits
    idx = np.arange(100 * D * 12, dtype=np.uint64).reshape(100, D, 12)
    s = (_splitmix64(idx, seed) >> np.uint64(32)).sum(axis=2, dtype=np.uint64)
    v = s.astype(F64) / F64(4294967296.0) - F64(6.0)
    nrm = np.sqrt(np.add.accumulate(v * v, axis=1)[:, -1])
    o = np.abs(v) / nrm[:, None]
    total = F64(0)
    for r in range(100):
        total = total + best_rescale_factor(o[r], ex_bits)
    t = F32(total / F64(100))
    _T_CACHE[(D, ex_bits)] = t
    return t


# ------------------------------------------------------------------------------------------------ codes and factors
def encode(xr, cr, t, ex_bits):
    """xr [n, D] rotated rows, cr [D] or [n, D] their rotated centres. Returns bits [n, D] uint8 (r >= 0), short factors [n, 3],
    ex codes [n, D] uint8 (flipped where the bit is 0), ex factors [n, 2]."""
    xr = np.asarray(xr, F32)
    cr = np.broadcast_to(np.asarray(cr, F32), xr.shape)
    n, D = xr.shape
    with np.errstate(all="ignore"):
        r = xr - cr
        b = r >= 0
        xu = np.where(b, F32(0.5), F32(-0.5))
        l2, ipr, ipc, xq = lane_sum(r * r), lane_sum(r * xu), lane_sum(cr * xu), lane_sum(xu * xu)
        l2n = np.sqrt(np.fmax(l2, F32(0)))
        denom = np.where(ipr == 0, F32(np.inf), ipr)
        fadd = l2 + (F32(2) * l2) * (ipc / denom)
        frs = (F32(-2) * l2) / denom
        ratio = (l2 * xq) / (denom * denom)
        inner = np.fmax((ratio - F32(1)) / np.fmax(F32(D - 1), F32(1)), F32(0))
        ferr = F32(2) * ((l2n * EPSILON) * np.sqrt(inner))
        short = np.stack([fadd, frs, ferr], axis=1).astype(F32)
        codes = np.zeros((n, D), np.uint8)
        exf = np.zeros((n, 2), F32)
        if ex_bits > 0:
            top = (1 << ex_bits) - 1
            val = np.where(l2n[:, None] > 0, np.abs(r) / l2n[:, None], F32(0)).astype(F32)
            code = np.minimum((F32(t) * val + F32(1e-5)).astype(np.int32), top)
            ipn = lane_sum((code.astype(F32) + F32(0.5)) * val)
            cf = np.where(b, code, (~code) & top)
            xu2 = (cf + (b.astype(np.int32) << ex_bits)).astype(F32) - (F32(1 << ex_bits) - F32(0.5))
            ipr2, ipc2 = lane_sum(r * xu2), lane_sum(cr * xu2)
            inv = F32(1) / ipn
            inv = np.where(np.isfinite(inv), inv, F32(1)).astype(F32)
            denom2 = np.where(ipr2 == 0, F32(np.inf), ipr2)
            exf = np.stack([l2 + ((F32(2) * l2) * ipc2) / denom2, (F32(-2) * l2n) * inv], axis=1).astype(F32)
            codes = cf.astype(np.uint8)
    return b.astype(np.uint8), short, codes, exf


def pack_bits(bits):
    """[n, D] 0/1 -> [n, D / 32] uint32, dimension 32 w + i at bit 31 - i (the file's and the export hook's order)"""
    n, D = bits.shape
    wts = (np.uint32(1) << (np.uint32(31) - np.arange(32, dtype=np.uint32)))
    return (bits.reshape(n, D // 32, 32).astype(np.uint32) * wts).sum(axis=2, dtype=np.uint32)


def unpack_bits(words, D):
    sh = np.uint32(31) - np.arange(32, dtype=np.uint32)
    return ((words[:, :, None] >> sh) & np.uint32(1)).astype(np.uint8).reshape(words.shape[0], D)


def pack_ex(codes, ex_bits):
    """[n, D] codes -> [n, D ex / 8] bytes: an MSB-first stream of ex bits per dimension"""
    n, D = codes.shape
    if ex_bits == 0:
        return np.zeros((n, 0), np.uint8)
    sh = ex_bits - 1 - np.arange(ex_bits)
    stream = ((codes[:, :, None].astype(np.uint16) >> sh) & 1).astype(np.uint8).reshape(n, D * ex_bits)
    return np.packbits(stream, axis=1)


def unpack_ex(stream, D, ex_bits):
    n = stream.shape[0]
    if ex_bits == 0:
        return np.zeros((n, D), np.uint8)
    b = np.unpackbits(stream, axis=1)[:, :D * ex_bits].reshape(n, D, ex_bits).astype(np.uint16)
    return (b << (ex_bits - 1 - np.arange(ex_bits))).sum(axis=2).astype(np.uint8)


def build(x, centers, rotation, bits_per_dim, labels=None):
    """An index in the export hook's form from rows, (unrotated) centres and a rotation; labels: nearest centre by exact L2
    unless given. Rows of a list in input order."""
    x, centers, rotation = np.asarray(x, F32), np.asarray(centers, F32), np.asarray(rotation, F32)
    n, dim = x.shape
    D, ex = rotation.shape[0], bits_per_dim - 1
    if labels is None:
        d = (x * x).sum(1)[:, None] - 2.0 * (x.astype(F64) @ centers.T.astype(F64)) + (centers * centers).sum(1)[None, :]
        labels = d.argmin(1)
    order = np.lexsort((np.arange(n), labels))
    cr = rotate(centers, rotation)
    t = scaling_factor(D, ex)
    xr = rotate(x[order], rotation)
    b, short, codes, exf = encode(xr, cr[labels[order]], t, ex)
    return dict(centers=centers, centers_rot=cr, rotation=rotation, list_sizes=np.bincount(labels, minlength=len(centers)).astype(np.uint32),
                ids=order.astype(np.uint32), bit_codes=pack_bits(b), short_factors=short, ex_codes=pack_ex(codes, ex), ex_factors=exf,
                t=t, dim=dim, ex_bits=ex, n=n)


# ------------------------------------------------------------------------------------------------ search
def quantize_query(qr, mode):
    """(q_hat [D] as the screen uses it, w)"""
    if mode in ("quant4", "quant8"):
        qmax = F32(7 if mode == "quant4" else 127)
        w = F32(np.abs(qr).max()) / qmax
        if not w > 0:
            return np.zeros(qr.shape, np.int64), F32(0)
        return np.clip(np.rint(qr / w), -qmax, qmax).astype(np.int64), w
    if mode == "lut16":
        return qr.astype(np.float16).astype(F32), F32(1)
    return qr, F32(1)


def search(ex, queries, k, n_probes, mode="quant4", metric="sqeuclidean", stats=None):
    """(distances [m, k] fp32, neighbors [m, k] int64) of cuvsAmdIvfRabitqSearch on an exported index"""
    q = np.asarray(queries, F32)
    D, exb = ex["rotation"].shape[0], int(ex["ex_bits"])
    sizes = ex["list_sizes"].astype(np.int64)
    start = np.concatenate([[0], np.cumsum(sizes)])
    bits = unpack_bits(ex["bit_codes"], D)
    u_all = ((bits.astype(np.uint16) << exb) | unpack_ex(ex["ex_codes"], D, exb)).astype(F32)
    short, exf, ids = ex["short_factors"], ex["ex_factors"], ex["ids"].astype(np.int64)
    fa_fin, frs_fin = (exf[:, 0], exf[:, 1]) if exb > 0 else (short[:, 0], short[:, 1])
    cs = F32(((1 << (exb + 1)) - 1) / 2)
    import oracle

    qr = rotate(q, ex["rotation"])
    S = lane_sum(qr)
    cd = oracle.pairwise(qr, ex["centers_rot"], "sqeuclidean")
    nq = q.shape[0]
    out_d = np.full((nq, k), np.finfo(F32).max, F32)
    out_i = np.full((nq, k), np.iinfo(np.int64).max, np.int64)
    n_lists = len(sizes)
    for qi in range(nq):
        probes = np.lexsort((np.arange(n_lists), cd[qi]))[:n_probes]
        g = np.fmax(cd[qi, probes], F32(0))
        cum = np.cumsum(sizes[probes])
        hit = np.nonzero(cum >= k)[0]
        head_len = int(hit[0]) + 1 if len(hit) else n_probes
        rows = [np.arange(start[L], start[L + 1]) for L in probes]

        def final(rr, gg):
            with np.errstate(all="ignore"):
                dot = lane_sum(qr[qi][None, :] * u_all[rr])
                return (fa_fin[rr] + gg) + frs_fin[rr] * (dot - cs * S[qi])

        hr = np.concatenate(rows[:head_len])
        hg = np.concatenate([np.full(len(rows[p]), g[p], F32) for p in range(head_len)])
        cand_d, cand_i = final(hr, hg), ids[hr]
        T = F32(np.inf)
        if len(hr) >= k:
            o = np.lexsort((cand_i, cand_d))
            T = cand_d[o[k - 1]]
        if head_len < n_probes:
            tr = np.concatenate(rows[head_len:])
            tg = np.concatenate([np.full(len(rows[p]), g[p], F32) for p in range(head_len, n_probes)])
            qh, w = quantize_query(qr[qi], mode)
            if mode in ("quant4", "quant8"):
                ip1 = w * (bits[tr].astype(np.int64) @ qh).astype(F32)
            else:
                ip1 = np.zeros(len(tr), F32)
                bt = bits[tr]
                for j in range(D):
                    ip1 = ip1 + np.where(bt[:, j] != 0, qh[j], F32(0))
            with np.errstate(all="ignore"):
                est = (short[tr, 0] + tg) + short[tr, 1] * (ip1 - F32(0.5) * S[qi])
                low = est - short[tr, 2] * np.sqrt(tg)
                keep = low < T
            if stats is not None:
                stats["screened"] = stats.get("screened", 0) + len(tr)
                stats["survivors"] = stats.get("survivors", 0) + int(keep.sum())
            sr = tr[keep]
            cand_d = np.concatenate([cand_d, final(sr, tg[keep])])
            cand_i = np.concatenate([cand_i, ids[sr]])
        o = np.lexsort((cand_i, cand_d))[:k]
        d = cand_d[o]
        if metric == "euclidean":
            d = np.sqrt(np.fmax(d, F32(0)))
        out_d[qi, :len(o)] = d
        out_i[qi, :len(o)] = cand_i[o]
    return out_d, out_i


# ------------------------------------------------------------------------------------------------ the file
def write_file(path, ex, metric="sqeuclidean"):
    """The reference's layout (IVFGPU::save): n, dim, n_lists, ex_bits as uint64; one bool; two floats (t; the metric: 0 squared L2,
    1 L2); list sizes as uint64; rotation; rotated centres; bit codes; short factors; ex codes; ex factors; ids."""
    with open(path, "wb") as f:
        f.write(np.array([ex["n"], ex["dim"], len(ex["list_sizes"]), ex["ex_bits"]], np.uint64).tobytes())
        f.write(b"\x01")
        f.write(np.array([ex["t"], 1.0 if metric == "euclidean" else 0.0], F32).tobytes())
        f.write(ex["list_sizes"].astype(np.uint64).tobytes())
        for name, dt in (("rotation", F32), ("centers_rot", F32), ("bit_codes", np.uint32), ("short_factors", F32),
                         ("ex_codes", np.uint8), ("ex_factors", F32), ("ids", np.uint32)):
            f.write(np.ascontiguousarray(ex[name], dtype=dt).tobytes())


def section_offsets(n, dim, n_lists, ex_bits):
    """byte offset of every section of a file, and its total length"""
    D = padded_dim(dim)
    lens = [("header", 41), ("list_sizes", 8 * n_lists), ("rotation", 4 * D * D), ("centers_rot", 4 * n_lists * D),
            ("bit_codes", 4 * n * (D // 32)), ("short_factors", 12 * n), ("ex_codes", n * D * ex_bits // 8), ("ex_factors", 8 * n),
            ("ids", 4 * n)]
    out, pos = {}, 0
    for name, ln in lens:
        out[name] = pos
        pos += ln
    out["end"] = pos
    return out


def parse_file(path):
    with open(path, "rb") as fh:
        f = io.BytesIO(fh.read())
    n, dim, n_lists, ex_bits = (int(v) for v in np.frombuffer(f.read(32), np.uint64))
    f.read(1)
    t, metric = np.frombuffer(f.read(8), F32)
    D = padded_dim(dim)
    sizes = np.frombuffer(f.read(8 * n_lists), np.uint64).astype(np.uint32)

    def arr(dt, *shape):
        cnt = int(np.prod(shape))
        return np.frombuffer(f.read(cnt * np.dtype(dt).itemsize), dt).reshape(shape).copy()

    out = dict(n=n, dim=dim, ex_bits=ex_bits, t=F32(t), metric="euclidean" if metric == 1.0 else "sqeuclidean", list_sizes=sizes,
               rotation=arr(F32, D, D), centers_rot=arr(F32, n_lists, D), bit_codes=arr(np.uint32, n, D // 32),
               short_factors=arr(F32, n, 3), ex_codes=arr(np.uint8, n, D * ex_bits // 8), ex_factors=arr(F32, n, 2),
               ids=arr(np.uint32, n))
    assert f.read() == b"", "trailing bytes"
    return out
