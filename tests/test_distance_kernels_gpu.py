"""GPU: the distance GEMM kernels of cuvs_amd/csrc/distance.hip held directly - dist_tile_kernel, dist_mfma_kernel<VEC=true> and
<VEC=false>, fused_l2_argmin and the row norms - through the typed hooks cuvsAmdPairwiseDistanceTyped / cuvsAmdFusedArgminTyped
(caller's pointers and pitches) and, for the row slabs, through the public pairwise_distance.

  A  bit for bit against the CPU twin (oracle.pairwise / oracle.row_norms), every built type pair, all six metrics, the tile
     edges, and one logical input through all three load paths
  B  against numpy float64 within a bound derived from the kernel's arithmetic (an error the twin shares would pass A)
  C  the 32768-row slabs of cuvsPairwiseDistance, row- and column-major
  D  fused_l2_argmin: labels and minima bit for bit, constructed ties, float64 cross-check, the 65535-tile slab
  E  matrices without columns or without rows

Data: signed (standard normal), every fifth row scaled by 1e3 so that qn + xn - 2 dot cancels, and planted rows of x:
bit-for-bit copies of rows of q, a copy that differs in one element by one ulp, near copies (squared distance below the
square root of the self-neighbour clamp's eps, norms different - the clamp must NOT fire there), and one all-zero row in
each operand (not for cosine: 0 / 0). fp16, int8 and uint8 values are drawn in the type; the twin gets them widened to fp32.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

U = 2.0 ** -24  # unit roundoff of fp32
M_L2Expanded, M_L2SqrtExpanded, M_CosineExpanded, M_L2Unexpanded, M_L2SqrtUnexpanded, M_InnerProduct = 0, 1, 2, 4, 5, 6
METRICS = (M_L2Expanded, M_L2SqrtExpanded, M_CosineExpanded, M_L2Unexpanded, M_L2SqrtUnexpanded, M_InnerProduct)
L2_METRICS = (M_L2Expanded, M_L2SqrtExpanded, M_L2Unexpanded, M_L2SqrtUnexpanded)
SQRT_METRICS = (M_L2SqrtExpanded, M_L2SqrtUnexpanded)
DTYPES = {"f32": (np.float32, 0), "f16": (np.float16, 1), "i8": (np.int8, 2), "u8": (np.uint8, 3)}  # numpy type, hook code
TYPE_PAIRS = [("f32", "f32"), ("f16", "f16"), ("f16", "f32"), ("i8", "f32"), ("u8", "f32")]  # the built pairwise_distance<TQ, TX>
SENTINEL = -7.0  # pre-fill of every output buffer: no metric of these inputs produces it


def _clamp_eps(xk):
    return 1e-3 if xk == "f16" else 1e-6  # pairwise_distance: by the width of TX


# ---------------------------------------------------------------------------------------------------------------- data
def _draw(rng, rows, dim, kind):
    if kind == "i8":
        return rng.integers(-128, 128, (rows, dim), dtype=np.int8)
    if kind == "u8":
        return rng.integers(0, 256, (rows, dim), dtype=np.uint8)
    v = rng.standard_normal((rows, dim)).astype(np.float32)
    v[2::5] *= np.float32(1e3)  # rows 2, 7, 12, ...
    return v.astype(DTYPES[kind][0])


def _one_ulp(row):
    r, k = row.copy(), row.shape[0] // 2
    if r.dtype.kind == "f":
        r[k] = np.nextafter(r[k], r.dtype.type(np.inf))
    else:
        r[k] = r[k] - 1 if r[k] > 0 else r[k] + 1
    return r


def _near(row):
    """Squared distance to `row` of 2e-4 (fp16: 1e-2) - its square is below the clamp's eps - with a different norm."""
    r = row.copy()
    if r.dtype.kind == "f":
        r[0] = r[0] + r.dtype.type(0.1 if r.dtype == np.float16 else 0.014)
    else:
        r[0] = r[0] - 1 if r[0] > 0 else r[0] + 1
    return r


class Case:
    pass


@functools.lru_cache(maxsize=None)
def _case(m, n, dim, qk, xk, zero_rows):
    """The inputs of one case (read-only, shared by the tests): q [m, dim] of kind qk, x [n, dim] of kind xk with the planted rows."""
    rng = np.random.default_rng(1000 * m + 10 * n + dim)
    c = Case()
    c.m, c.n, c.dim, c.qk, c.xk = m, n, dim, qk, xk
    q, x = _draw(rng, m, dim, qk), _draw(rng, n, dim, xk)
    zq = m - 2 if (zero_rows and m >= 4) else -1
    src = [i for i in range(m) if i % 5 != 2 and i != zq]  # unscaled rows of q
    slots = list(dict.fromkeys([n - 1, 0, n // 2, n // 3, (2 * n) // 3, n // 4]))  # rows of x to plant, over the column tiles
    c.copies, c.planted_x = [], []
    for k, j in enumerate(slots):
        i = src[(37 * k) % len(src)]
        wide = q[i].astype(x.dtype)  # exact: x is q's type or fp32
        if k < 2:
            x[j] = wide
            c.copies.append((i, j))
        elif k == 2:
            x[j] = _one_ulp(wide)
        elif k < 5:
            x[j] = _near(wide)
        elif zero_rows:
            x[j] = 0
        else:
            continue
        c.planted_x.append(j)
    if zq >= 0:
        q[zq] = 0
    c.q, c.x = q, x
    c.q32, c.x32 = q.astype(np.float32), x.astype(np.float32)
    for a in (c.q, c.x, c.q32, c.x32):
        a.setflags(write=False)
    return c


def _case_for(metric, m, n, dim, qk="f32", xk="f32"):
    return _case(m, n, dim, qk, xk, metric != M_CosineExpanded)


# ---------------------------------------------------------------------------------------------------------------- device
def _dev(a, ld=None, off=0):
    """The rows of `a` at pitch `ld`, `off` elements into a device buffer; the padding holds NaN (the integer types: their
    maximum), so a read beyond a row's `dim` elements shows in the result. Returns (owner, address of row 0)."""
    import torch

    rows, dim = a.shape
    ld = dim if ld is None else ld
    buf = np.full(off + rows * ld + 16, np.nan if a.dtype.kind == "f" else np.iinfo(a.dtype).max, a.dtype)
    if rows * dim > 0:
        buf[off:off + rows * ld].reshape(rows, ld)[:, :dim] = a
    t = torch.from_numpy(buf).cuda()
    return t, t.data_ptr() + off * a.itemsize


def _pairwise(res, q, x, metric, ldq=None, ldx=None, off=0, ldo=None):
    """cuvsAmdPairwiseDistanceTyped on q [m, dim], x [n, dim] -> the whole [m, ldo] output buffer, pre-filled with SENTINEL."""
    import torch
    from cuvs_amd._lib import check, lib

    kinds = {np.dtype(t): code for t, code in DTYPES.values()}
    (m, dim), n = q.shape, x.shape[0]
    ldo = n if ldo is None else ldo
    qt, qp = _dev(q, ldq, off)
    xt, xp = _dev(x, ldx, off)
    out = torch.full((m * ldo + 16,), SENTINEL, dtype=torch.float32, device="cuda")
    fn = lib().cuvsAmdPairwiseDistanceTyped
    fn.argtypes = [C.c_size_t, C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_int64,
                   C.c_int, C.c_void_p, C.c_int64]
    fn.restype = C.c_int
    torch.cuda.synchronize()
    check(fn(res.get_c_obj(), qp, kinds[q.dtype], dim if ldq is None else ldq, m, xp, kinds[x.dtype], dim if ldx is None else ldx, n,
             dim, metric, out.data_ptr(), ldo))
    res.sync()
    h = out.cpu().numpy()
    assert (h[m * ldo:] == SENTINEL).all(), "written past the end of the output"
    return h[:m * ldo].reshape(m, ldo)


def _argmin(res, q, centers, ldq=None, off=0, want_min=True):
    """cuvsAmdFusedArgminTyped -> (labels, min_val or None)."""
    import torch
    from cuvs_amd._lib import check, lib

    kinds = {np.dtype(t): code for t, code in DTYPES.values()}
    (m, dim), n = q.shape, centers.shape[0]
    qt, qp = _dev(q, ldq, off)
    ct = torch.from_numpy(np.ascontiguousarray(centers, dtype=np.float32)).cuda()
    labels = torch.full((m + 16,), -5, dtype=torch.int32, device="cuda")
    mv = torch.full((m + 16,), SENTINEL, dtype=torch.float32, device="cuda")
    fn = lib().cuvsAmdFusedArgminTyped
    fn.argtypes = [C.c_size_t, C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]
    fn.restype = C.c_int
    torch.cuda.synchronize()
    check(fn(res.get_c_obj(), qp, kinds[q.dtype], dim if ldq is None else ldq, m, ct.data_ptr(), n, dim, labels.data_ptr(),
             mv.data_ptr() if want_min else None))
    res.sync()
    lab, val = labels.cpu().numpy(), mv.cpu().numpy()
    assert (lab[m:] == -5).all() and (val[m:] == SENTINEL).all(), "written past the end of the outputs"
    if not want_min:
        assert (val == SENTINEL).all()
    return lab[:m].astype(np.int64), (val[:m] if want_min else None)


def _public(x, y, metric, col_major=False):
    """The public cuvs_amd.distance.pairwise_distance on host arrays -> host [m, n]."""
    import torch
    from cuvs_amd.distance import pairwise_distance

    (m, n) = x.shape[0], y.shape[0]
    tx, ty = torch.tensor(x).cuda(), torch.tensor(y).cuda()  # (copies: the shared inputs are read-only)
    if col_major:
        tx, ty = tx.t().contiguous().t(), ty.t().contiguous().t()
        out = torch.full((n, m), SENTINEL, dtype=torch.float32, device="cuda").t()
    else:
        out = torch.full((m, n), SENTINEL, dtype=torch.float32, device="cuda")
    assert pairwise_distance(tx, ty, out=out, metric=metric) is out
    return out.cpu().numpy()


def _dist_old_handle(monkeypatch):
    """A handle that keeps pairwise_distance off dist_tile_kernel (the switch is read when the handle is created)."""
    import cuvs_amd

    monkeypatch.setenv("CUVS_AMD_DIST_OLD", "1")
    r = cuvs_amd.common.Resources()
    monkeypatch.delenv("CUVS_AMD_DIST_OLD")
    return r


# ---------------------------------------------------------------------------------------------------------------- A
def _check_exact(got, c, metric):
    want = oracle.pairwise(c.q32, c.x32, metric, _clamp_eps(c.xk))
    assert got.shape == want.shape
    assert (got == want).all(), "%d of %d elements differ from the CPU twin" % ((got != want).sum(), want.size)
    if metric in L2_METRICS:
        assert not np.isnan(got).any() and (got >= 0).all()
        for i, j in c.copies:
            assert got[i, j] == 0.0 and not np.signbit(got[i, j])


# (1, 1): every staged row is row 0; (129, 1), (1, 129): one live row in the last tile; (128, 128): exactly one tile
SHAPES_A = [(1, 1), (129, 1), (1, 129), (128, 128), (257, 129), (127, 257), (129, 127)]
# 1-4 k-tiles of 16 (both double-buffer parities), the partial-chunk tails of load4, the tile kernel's dims (16, 32, 48, 64)
DIMS_A = [1, 3, 4, 15, 16, 17, 20, 32, 48, 64]


@pytest.mark.parametrize("dim", DIMS_A)
@pytest.mark.parametrize("m,n", SHAPES_A)
def test_fp32_matches_the_twin_bit_for_bit(m, n, dim, res):
    for metric in METRICS:
        c = _case_for(metric, m, n, dim)
        _check_exact(_pairwise(res, c.q, c.x, metric), c, metric)


@pytest.mark.parametrize("m,n,dim", [(129, 257, 20), (257, 129, 48)])
@pytest.mark.parametrize("qk,xk", TYPE_PAIRS)
def test_every_type_pair_matches_the_twin_bit_for_bit(qk, xk, m, n, dim, res):
    """Same-type pairs take dist_tile_kernel at dim 48, the mixed pairs dist_mfma_kernel<VEC=true> at both dims. Every product of
    two fp16 / int8 / uint8 values is exact in fp32, so the twin on the widened values is the same arithmetic."""
    for metric in METRICS:
        c = _case_for(metric, m, n, dim, qk, xk)
        _check_exact(_pairwise(res, c.q, c.x, metric), c, metric)


@pytest.mark.parametrize("kind", ["f32", "f16"])
@pytest.mark.parametrize("dim", [16, 48, 64])
def test_three_load_paths_give_the_same_bits(dim, kind, res, monkeypatch):
    """One logical input through dist_tile_kernel (aligned, pitches multiples of 4), dist_mfma_kernel<VEC=true> (a handle with
    the tile kernel switched off) and dist_mfma_kernel<VEC=false> (base pointers moved by one element into a padded buffer;
    pitch dim + 1), plus the tile kernel at pitch dim + 4 and with an output pitch beyond n: one matrix, bit for bit."""
    old = _dist_old_handle(monkeypatch)
    m, n = 257, 129
    for metric in METRICS:
        c = _case_for(metric, m, n, dim, kind, kind)
        tile = _pairwise(res, c.q, c.x, metric)
        _check_exact(tile, c, metric)
        assert (_pairwise(old, c.q, c.x, metric) == tile).all(), "dist_mfma_kernel<VEC=true>"
        assert (_pairwise(res, c.q, c.x, metric, off=1) == tile).all(), "dist_mfma_kernel<VEC=false>, misaligned base"
        assert (_pairwise(res, c.q, c.x, metric, ldq=dim + 1, ldx=dim + 1) == tile).all(), "dist_mfma_kernel<VEC=false>, odd pitch"
        assert (_pairwise(res, c.q, c.x, metric, ldq=dim + 4, ldx=dim + 4) == tile).all(), "dist_tile_kernel, strided"
        assert (_pairwise(old, c.q, c.x, metric, ldq=dim + 4, ldx=dim + 4) == tile).all(), "dist_mfma_kernel<VEC=true>, strided"
        for r in (res, old):
            wide = _pairwise(r, c.q, c.x, metric, ldo=n + 7)
            assert (wide[:, :n] == tile).all() and (wide[:, n:] == SENTINEL).all(), "output pitch beyond n"


def test_hook_rejects_a_type_pair_that_is_not_built(res):
    from cuvs_amd._lib import CuvsError

    c = _case_for(M_L2Expanded, 1, 1, 4)
    with pytest.raises(CuvsError, match="no instance"):
        _pairwise(res, c.q, c.x.astype(np.float16), M_L2Expanded)


# ---------------------------------------------------------------------------------------------------------------- B
def _check_float64(got, c, metric):
    """|GPU - float64| within a bound derived from the kernel's arithmetic, u = 2^-24, on the rows that were not planted.

    dot: a chain of `dim` fmas, |fl(dot) - dot| <= dim u S with S = sum |q_k x_k| (first order in u throughout).
    norm: each lane sums every 64th square by fma (ceil(dim / 64) roundings), then a 6-step butterfly:
          |fl(|v|^2) - |v|^2| <= (ceil(dim / 64) + 6) u |v|^2  <=  7 u |v|^2  for dim <= 64 (the cases here).
    squared L2 = fma(-2, dot, qn + xn): 2 dim u S + 7 u (|q|^2 + |x|^2) + u (|q|^2 + |x|^2) [the sum qn + xn] + u |result|
          [the fma]; with 2 S <= |q|^2 + |x|^2 and |result| <= 2 (|q|^2 + |x|^2) that is (dim + 10) u (|q|^2 + |x|^2). The
          tolerance is twice that - 2 (dim + 10) u (|q|^2 + |x|^2) - which also covers the second-order terms. The clamp to
          >= 0 only moves a value towards the true one. Pairs whose fp32 norms are bit-equal are left out (the self-neighbour
          clamp may return 0 there): under 1 % of a case's pairs, asserted.
    sqrt metrics: the square of the GPU value under the same bound plus 4 u relative (sqrtf rounds once: (1 + u)^2).
    inner product: (dim + 1) u S.
    cosine = 1 - dot / (sqrt(qn) sqrt(xn)): dim u from the dot (S <= |q| |x|), 7 u / 2 + u from each root, u each from the
          product, the quotient and the difference, all relative to a cosine of magnitude <= 1: (dim + 12) u, under the
          tolerance 2 (dim + 10) u.
    """
    keep = np.setdiff1d(np.arange(c.n), c.planted_x)
    assert keep.size >= c.n - 6
    q, x, g = c.q32.astype(np.float64), c.x32.astype(np.float64)[keep], got[:, keep].astype(np.float64)
    dim = c.dim
    assert dim <= 64
    qq, xx = (q * q).sum(1), (x * x).sum(1)
    if metric == M_InnerProduct:
        err, tol = np.abs(g - q @ x.T), (dim + 1) * U * (np.abs(q) @ np.abs(x).T)
    elif metric == M_CosineExpanded:
        err, tol = np.abs(g - (1.0 - (q @ x.T) / np.sqrt(qq[:, None] * xx[None, :]))), 2 * (dim + 10) * U
    else:
        d2 = ((q[:, None, :] - x[None, :, :]) ** 2).sum(-1)
        tol = 2 * (dim + 10) * U * (qq[:, None] + xx[None, :])
        if metric in SQRT_METRICS:
            g = g * g
            tol = tol + 4 * U * np.maximum(g, d2)
        same_norm = oracle.row_norms(c.q32)[:, None] == oracle.row_norms(c.x32)[keep][None, :]
        assert same_norm.mean() < 0.01
        err = np.where(same_norm, 0.0, np.abs(g - d2))
    worst = float(np.max(err / np.maximum(tol, np.finfo(np.float64).tiny))) if err.size else 0.0
    assert (err <= tol).all(), "error up to %.3f of the bound" % worst
    return worst


CASES_B = [(257, 129, d, "f32", "f32") for d in DIMS_A] + [(129, 257, 17, "f32", "f32")] + \
          [(m, n, d, qk, xk) for qk, xk in TYPE_PAIRS[1:] for m, n, d in [(129, 257, 20), (257, 129, 48)]]


@pytest.mark.parametrize("m,n,dim,qk,xk", CASES_B)
def test_within_the_derived_bound_of_float64(m, n, dim, qk, xk, res):
    c = _case(m, n, dim, qk, xk, False)  # (the all-zero rows are planted rows: left out here)
    for metric in METRICS:
        _check_float64(_pairwise(res, c.q, c.x, metric), c, metric)


# ---------------------------------------------------------------------------------------------------------------- C
@functools.lru_cache(maxsize=None)
def _slab_data(m, n, kind):
    rng = np.random.default_rng(m + 3 * n)
    x, y = _draw(rng, m, 4, kind), _draw(rng, n, 4, kind)
    big, small = (x, y) if m > n else (y, x)
    big[100], big[32768 + 50], big[len(big) - 1] = small[1], small[0], small[2]  # copies in both slabs: zeros / the clamp
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


@pytest.mark.parametrize("metric", ["sqeuclidean", "cosine"])
@pytest.mark.parametrize("kind", ["f32", "f16"])
@pytest.mark.parametrize("m,n", [(32768 + 130, 3), (3, 32768 + 130)])
def test_row_slabs_of_the_public_call(m, n, kind, metric):
    """cuvsPairwiseDistance walks x in slabs of 32768 rows (norms and output offset by the slab). Row-major crosses the slab at
    the first shape; the column-major form computes distance(y, x), so it crosses at the second."""
    x, y = _slab_data(m, n, kind)
    row = _public(x, y, metric)
    want = oracle.pairwise(x.astype(np.float32), y.astype(np.float32), metric, _clamp_eps(kind))
    assert (row == want).all(), "%d elements differ from the CPU twin, first at %s" % ((row != want).sum(), np.argwhere(row != want)[:1])
    col = _public(x, y, metric, col_major=True)
    assert np.allclose(col, row, rtol=1e-5, atol=1e-5)


# ---------------------------------------------------------------------------------------------------------------- D
def _argmin_reference(q32, centers):
    dots = oracle.pairwise(q32, centers, "inner_product")
    cn = oracle.row_norms(centers)
    # -2 * dot is exact, so the sum rounds once - exactly the kernel's fma(-2, dot, cn)
    v = cn[None, :] + np.float32(-2) * dots
    assert v.dtype == np.float32
    return v.argmin(1), v.min(1)  # argmin: the first minimum


def _check_argmin_float64(labels, q32, centers):
    """The chosen centre is a float64 minimiser up to the rounding of the two values compared: each of the kernel's
    cn_j - 2 dot_j is within (dim + 10) u (|q|^2 + |c_j|^2) of the truth (section B without the query norm), i.e. half the
    squared-L2 tolerance tol_j of B, so d64(chosen) - min d64 <= (tol_chosen + tol_min) / 2."""
    q, c = q32.astype(np.float64), centers.astype(np.float64)
    dim = q.shape[1]
    d2 = ((q[:, None, :] - c[None, :, :]) ** 2).sum(-1)
    tol = 2 * (dim + 10) * U * ((q * q).sum(1)[:, None] + (c * c).sum(1)[None, :])
    rows, best = np.arange(len(q)), d2.argmin(1)
    assert (d2[rows, labels] - d2[rows, best] <= (tol[rows, labels] + tol[rows, best]) / 2).all()


@pytest.mark.parametrize("dim", [1, 5, 16, 20, 33, 64])
@pytest.mark.parametrize("kind", ["f32", "f16", "i8", "u8"])
def test_fused_argmin_matches_the_twin(kind, dim, res):
    """n over 1, 2 and the column-tile edge, m over the row-tile edge, the query pitch over dense / odd (VEC=false) / padded."""
    rng = np.random.default_rng(7 * dim + len(kind))
    q_all = _draw(rng, 260, dim, kind)
    c_all = (rng.standard_normal((300, dim)) * (1.0 if kind in ("f32", "f16") else 40.0)).astype(np.float32)
    for n in (1, 2, 127, 128, 129, 300):
        centers = c_all[:n]
        want_l, want_v = _argmin_reference(q_all.astype(np.float32), centers)
        for m in (1, 129, 260):
            q = q_all[:m]
            for ldq in (dim, dim + 1, dim + 4):
                lab, val = _argmin(res, q, centers, ldq=ldq)
                assert (lab == want_l[:m]).all() and (val == want_v[:m]).all(), (n, m, ldq)
            _check_argmin_float64(lab, q.astype(np.float32), centers)
    lab, val = _argmin(res, q_all, c_all, off=1, want_min=False)  # misaligned base (VEC=false), no min_val
    assert val is None and (lab == want_l).all()


def _tie_inputs(kind, dim):
    """Small integers: every sum is exact in any order, so equal centres tie exactly. Centres 3, 19, 70 and 200 are one vector:
    two j fragments of one lane, the other column wave, the second column tile."""
    rng = np.random.default_rng(dim)
    lo = 0 if kind == "u8" else -3
    centers = rng.integers(-3, 4, (300, dim)).astype(np.float32)
    centers[3] = rng.integers(0, 4, dim)
    centers[[19, 70, 200]] = centers[3]
    q = rng.integers(lo, 4, (260, dim)).astype(DTYPES[kind][0])
    planted = [5, 77, 130, 259]
    q[planted] = centers[3].astype(q.dtype)
    ci, qi = centers.astype(np.int64), q.astype(np.int64)
    v = (ci * ci).sum(1)[None, :] - 2 * (qi @ ci.T)
    return q, centers, planted, v.argmin(1), v.min(1).astype(np.float32)


@pytest.mark.parametrize("dim", [16, 33])
@pytest.mark.parametrize("kind", ["f32", "f16", "i8", "u8"])
def test_fused_argmin_ties_go_to_the_smallest_index(kind, dim, res):
    q, centers, planted, want_l, want_v = _tie_inputs(kind, dim)
    assert (want_l[planted] == 3).all()
    for ldq in (dim, dim + 1, dim + 4):
        lab, val = _argmin(res, q, centers, ldq=ldq)
        assert (lab[planted] == 3).all()
        assert (lab == want_l).all() and (val == want_v).all()
    lab, val = _argmin(res, q, np.tile(centers[3], (300, 1)))  # all centres identical: every lane of both column waves ties
    c3 = centers[3].astype(np.int64)
    assert (lab == 0).all() and (val == ((c3 * c3).sum() - 2 * (q.astype(np.int64) @ c3)).astype(np.float32)).all()


def test_fused_argmin_row_slabs(res):
    """More rows than one launch's 65535 row tiles: the second slab's queries, labels and minima are offset by the first's rows."""
    m, n, dim = 65535 * 128 + 131, 5, 4
    rng = np.random.default_rng(11)
    q = rng.integers(-8, 9, (m, dim), dtype=np.int8)
    centers = rng.integers(-8, 9, (n, dim)).astype(np.float32)
    centers[3] = centers[1]  # a tie, first index wins
    v = (centers * centers).sum(1)[None, :] - 2 * (q.astype(np.float32) @ centers.T)  # small integers: exact in fp32
    lab, val = _argmin(res, q, centers)
    assert (lab == v.argmin(1)).all() and (val == v.min(1)).all()
    assert (lab != 3).all()


# ---------------------------------------------------------------------------------------------------------------- E
@pytest.mark.parametrize("metric", ["sqeuclidean", "euclidean", "inner_product"])
def test_matrices_without_columns(metric, res):
    """dim == 0 stays off dist_tile_kernel (whose first load is unconditional); every distance of two empty vectors is 0."""
    x, y = np.empty((5, 0), np.float32), np.empty((4, 0), np.float32)
    want = oracle.pairwise(x, y, metric)
    assert want.shape == (5, 4) and (want == 0).all()
    assert (_public(x, y, metric) == want).all()
    assert (_public(x, y, metric, col_major=True) == want).all()
    code = {"sqeuclidean": M_L2Expanded, "euclidean": M_L2SqrtExpanded, "inner_product": M_InnerProduct}[metric]
    for kind in ("f32", "f16"):
        t = DTYPES[kind][0]
        assert (_pairwise(res, x.astype(t), y.astype(t), code) == want).all()


def test_matrices_without_rows(res):
    import torch
    from cuvs_amd.distance import pairwise_distance

    some, none = np.ones((4, 8), np.float32), np.empty((0, 8), np.float32)
    for q, x in ((none, some), (some, none)):
        for metric in METRICS:
            out = _pairwise(res, q, x, metric, ldo=4)  # _pairwise checks the 16 pre-filled elements behind m * ldo
            assert out.size == 0 or (out == SENTINEL).all()
        for col_major in (False, True):
            assert _public(q, x, "sqeuclidean", col_major).size == 0
    lab, val = _argmin(res, none, some)
    assert lab.size == 0 and val.size == 0
    assert pairwise_distance(torch.empty((0, 8), device="cuda"), torch.ones((4, 8), device="cuda")).shape == (0, 4)
