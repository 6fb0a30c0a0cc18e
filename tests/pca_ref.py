"""numpy restatement of the PCA semantics of include/cuvs/preprocessing/pca.h (not a test module).

fit(X, k, dtype): dtype float64 is the truth the GPU tests measure against, float32 the comparator whose own error sets the
scale of the allowed error. transform_exact / inverse_transform_exact restate the projections bit for bit: the fp32 chain
acc = fmaf(a_k, w_k, acc) in ascending k from 0, with the centring, the whitening scale and the final `+ mu` as single fp32
operations."""
import numpy as np

EPS32 = float(np.finfo(np.float32).eps)


def apply_v_sign(components):
    """The entry of largest magnitude of every row is made positive (lowest index on a tie; an all-zero row stays)."""
    out = components.copy()
    for i in range(out.shape[0]):
        j = int(np.argmax(np.abs(out[i])))
        if out[i, j] < 0:
            out[i] = -out[i]
    return out


def apply_u_sign(components, Xc):
    """The entry of largest magnitude of column i of Xc components^T is made positive (same tie rule)."""
    out = components.copy()
    T = Xc @ out.T
    for i in range(out.shape[0]):
        j = int(np.argmax(np.abs(T[:, i])))
        if T[j, i] < 0:
            out[i] = -out[i]
    return out


def fit(X, k, dtype=np.float64, flip_signs_based_on_U=False):
    X = np.asarray(X).astype(dtype)
    n, d = X.shape
    mu = X.mean(axis=0, dtype=dtype)
    Xc = X - mu
    cov = (Xc.T @ Xc) / dtype(n - 1)
    lam, V = np.linalg.eigh(cov)
    order = np.argsort(-lam, kind="stable")
    lam, V = lam[order], V[:, order]
    comp = np.ascontiguousarray(V[:, :k].T)
    comp = apply_u_sign(comp, Xc) if flip_signs_based_on_U else apply_v_sign(comp)
    ev = np.maximum(lam[:k], dtype(0))
    return dict(mu=mu, cov=cov, eigenvalues=lam, components=comp, explained_var=ev,
                explained_var_ratio=ev / np.trace(cov), singular_vals=np.sqrt(ev * dtype(n - 1)),
                noise_vars=(lam[k:].mean() if k < d else dtype(0)))


def fma32(a, b, c):
    """Correctly rounded fp32 a * b + c for fp32 arrays, in float64 arithmetic. The product of two fp32 numbers is exact in
    float64; the sum s = fl64(p + c) comes with its exact error e (TwoSum). Rounding s to fp32 can differ from rounding p + c
    only when s lies exactly half way between two fp32 numbers and e is not 0: then e decides the direction."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    r = s.astype(np.float32)
    up = np.nextafter(r, np.float32(np.inf)).astype(np.float64)
    dn = np.nextafter(r, np.float32(-np.inf)).astype(np.float64)
    r64 = r.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        go_up = (e > 0) & (s == (r64 + up) / 2)
        go_dn = (e < 0) & (s == (r64 + dn) / 2)
    r = np.where(go_up, up.astype(np.float32), r)
    r = np.where(go_dn, dn.astype(np.float32), r)
    return r.astype(np.float32)


def chain(A, B):
    """[n, K] fp32 times [K, N] fp32 as the fmaf chain in ascending K from acc = 0."""
    A = np.asarray(A, dtype=np.float32)
    B = np.asarray(B, dtype=np.float32)
    acc = np.zeros((A.shape[0], B.shape[1]), dtype=np.float32)
    for kk in range(A.shape[1]):
        acc = fma32(A[:, kk:kk + 1], B[kk:kk + 1, :], acc)
    return acc


def _f32(*arrays):
    return [np.asarray(a, dtype=np.float32) for a in arrays]


def transform_exact(X, components, singular_vals, mu, whiten):
    X, W, sv, mu = _f32(X, components, singular_vals, mu)
    if whiten:
        root = np.sqrt(np.float32(X.shape[0] - 1))
        with np.errstate(divide="ignore"):
            scale = np.where(sv == 0, np.float32(0), root / sv).astype(np.float32)
        W = W * scale[:, None]
    return chain(X - mu, W.T)


def inverse_transform_exact(T, components, singular_vals, mu, whiten):
    T, W, sv, mu = _f32(T, components, singular_vals, mu)
    if whiten:
        W = W * (sv / np.sqrt(np.float32(T.shape[0] - 1)))[:, None]
    return chain(T, W) + mu


def long_rows_case():
    """300000 x 8 rows around 1000 and their float64 fit: the case of a long reduction under a large mean."""
    X = (1000 + np.random.default_rng(11).standard_normal((300000, 8))).astype(np.float32)
    return X, fit(X, 8, np.float64)


# The case that runs the covariance past one fp32 chain. n_pairs = 1 at d = 8, so the kernel's row range is
# round_up(ceil(n / 256), 64) = 8640 rows: one flush into fp64 after 8192, then 448 more. Every centred entry is +-(1 + 2^-12),
# whose square 1 + 2^-11 + 2^-24 adds exactly (but for the last term) to an fp32 sum below 8192 and is rounded UP by about 2^-11
# on every addition to a sum in [8192, 16384): a chain that is not broken at 8192 rows ends about 2.5e-5 too high, relative.
FLUSH_CASE_N, FLUSH_CASE_D, FLUSH_CASE_A, FLUSH_CASE_SPLIT_ROWS = 2200000, 8, 1 + 2.0 ** -12, 8640


def flush_case():
    """Rows of +-(1 + 2^-12): column j carries the signs of row j + 1 of the 16 x 16 Hadamard matrix, period 16, so that the
    column means are exactly 0 and the columns orthogonal. Returns X and the exact covariance a^2 n / (n - 1) I."""
    H = np.array([[1.0]])
    while H.shape[0] < 16:
        H = np.block([[H, H], [H, -H]])
    n, d = FLUSH_CASE_N, FLUSH_CASE_D
    assert n % 16 == 0
    X = np.tile((H[1:d + 1].T * FLUSH_CASE_A).astype(np.float32), (n // 16, 1))
    lam = float(np.float32(FLUSH_CASE_A)) ** 2 * n / (n - 1)
    return X, lam
