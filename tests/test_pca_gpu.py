"""GPU: cuvsPca* against the numpy restatement tests/pca_ref.py.

Accuracy is a rule, not a number: every quantity of the GPU fit may be off from the float64 restatement by at most
max(8 x the float32 restatement's error on the same input, a floor from backward-error scale). The floors: d eps32 relative to
the largest eigenvalue for eigenvalues, singular_vals^2 / (n - 1), noise_vars and the residual |C64 v_i - l_i v_i|_2; d eps32 for
max|W W^T - I| and explained_var_ratio; one fp32 ulp of the largest |mu| for mu; d eps32 / relgap_i for components[i]
(Davis-Kahan). The 8 x covers a different solver and summation order than LAPACK / BLAS.

The projections are held bit for bit to the fp32 fmaf chain of tests/pca_ref.py."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

from cuvs_amd._lib import Tensor, check, lib
from cuvs_amd.preprocessing import pca
from tests import pca_ref
from tests.pca_ref import EPS32

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = json.load(open(os.path.join(ROOT, "tests", "golden", "pca_reference_table.json")))
COMPONENT_SHAPES = [(1000, 72, 9), (257, 33, 5), (4099, 130, 17)]
FULL_SHAPES = [(300, 40, 40), (20, 48, 48)]


@functools.lru_cache(maxsize=None)
def _data():
    """The accuracy inputs, drawn in the order of COMPONENT_SHAPES + FULL_SHAPES from one generator."""
    rng = np.random.default_rng(7)
    out = {}
    for n, d, k in COMPONENT_SHAPES + FULL_SHAPES:
        s = 2.0 ** (-np.arange(d) / 4)
        Q = np.linalg.qr(rng.standard_normal((d, d)))[0]
        X = ((rng.standard_normal((n, d)) * s) @ Q.T + 3 * rng.standard_normal(d)).astype(np.float32)
        X.setflags(write=False)
        out[(n, d, k)] = X
    return out


@functools.lru_cache(maxsize=None)
def _refs(shape):
    X = _data()[shape]
    return pca_ref.fit(X, shape[2], np.float64), pca_ref.fit(X, shape[2], np.float32)


def _dev(a, layout):
    """A device copy of the 2-D array `a`, row-major ("C") or column-major ("F")."""
    t = torch.from_numpy(np.array(a, order="C")).cuda()
    return t if layout == "C" else t.t().contiguous().t()


def _empty(shape, layout):
    t = torch.empty(shape, dtype=torch.float32, device="cuda")
    return t if layout == "C" else torch.empty(shape[::-1], dtype=torch.float32, device="cuda").t()


def gpu_fit(res, X, k, layout="F", comp_layout="F", flip_u=False, trans_layout=None, **params):
    """cuvsPcaFit (or FitTransform when trans_layout is given) through the C ABI; numpy results."""
    p = pca.Params(n_components=k, **params)
    x = _dev(X, layout) if not isinstance(X, torch.Tensor) else X
    n, d = x.shape
    comp = _empty((k, d), comp_layout)
    vec = [torch.empty(m, dtype=torch.float32, device="cuda") for m in (k, k, k, d, 1)]
    args = [Tensor(comp).ptr] + [Tensor(v).ptr for v in vec] + [C.c_bool(flip_u)]
    if trans_layout is None:
        check(lib().cuvsPcaFit(res.get_c_obj(), p._p, Tensor(x).ptr, *args))
        trans = None
    else:
        trans = _empty((n, k), trans_layout)
        check(lib().cuvsPcaFitTransform(res.get_c_obj(), p._p, Tensor(x).ptr, Tensor(trans).ptr, *args))
    res.sync()
    sweeps = C.c_int(-1)
    check(lib().cuvsAmdPcaLastSweeps(C.byref(sweeps)))
    out = dict(components=comp.cpu().numpy(), explained_var=vec[0].cpu().numpy(), explained_var_ratio=vec[1].cpu().numpy(),
               singular_vals=vec[2].cpu().numpy(), mu=vec[3].cpu().numpy(), noise_vars=vec[4].cpu().numpy()[0], sweeps=sweeps.value,
               dev=(comp, vec[2], vec[3]))
    if trans is not None:
        out["trans_input"] = trans
    return out


def gpu_transform(res, x, comp, sv, mu, k, whiten, out_layout, inverse=False):
    p = pca.Params(n_components=k, whiten=whiten)
    rows = x.shape[0]
    out = _empty((rows, comp.shape[1] if inverse else k), out_layout)
    fn = lib().cuvsPcaInverseTransform if inverse else lib().cuvsPcaTransform
    check(fn(res.get_c_obj(), p._p, Tensor(x).ptr, Tensor(comp).ptr, Tensor(sv).ptr, Tensor(mu).ptr, Tensor(out).ptr))
    res.sync()
    return out


def _residual(cov64, lam, comp):
    return np.linalg.norm(cov64 @ comp.T.astype(np.float64) - comp.T.astype(np.float64) * lam.astype(np.float64), axis=0).max()


def _errors(got, r64, n, d, k):
    """Error of one fit (the GPU's or the float32 restatement's) against the float64 restatement, quantity by quantity."""
    lam0 = r64["eigenvalues"][0]
    W = np.asarray(got["components"], dtype=np.float64)
    return dict(
        eigenvalues=np.abs(got["explained_var"] - r64["explained_var"]).max() / lam0,
        singular_sq=np.abs(np.asarray(got["singular_vals"], dtype=np.float64) ** 2 - r64["singular_vals"] ** 2).max() / (n - 1) / lam0,
        noise_vars=abs(float(got["noise_vars"]) - float(r64["noise_vars"])) / lam0,
        residual=_residual(r64["cov"], np.asarray(got["explained_var"]), np.asarray(got["components"])) / lam0,
        orthonormal=np.abs(W @ W.T - np.eye(k)).max(),
        ratio=np.abs(got["explained_var_ratio"] - r64["explained_var_ratio"]).max(),
        mu=np.abs(got["mu"] - r64["mu"]).max(),
    )


def _check_rule(got, shape, componentwise, label="gpu", skip=()):
    n, d, k = shape
    r64, r32 = _refs(shape)
    e_gpu, e_32 = _errors(got, r64, n, d, k), _errors(r32, r64, n, d, k)
    floors = dict.fromkeys(e_gpu, d * EPS32)
    floors["mu"] = float(np.spacing(np.float32(np.abs(r64["mu"]).max())))
    bad = []
    for q in e_gpu:
        if q in skip:
            continue
        bound = max(8 * e_32[q], floors[q])
        print(f"pca accuracy {label} {shape} {q}: gpu {e_gpu[q]:.3e} f32 {e_32[q]:.3e} floor {floors[q]:.3e} bound {bound:.3e}")
        if not e_gpu[q] <= bound:
            bad.append(q)
    if componentwise:
        lam = r64["eigenvalues"]
        relgap = (lam[:k] - lam[1:k + 1]) / lam[0]
        assert relgap.min() >= 1e-3, f"precondition: relative gaps {relgap.min():.2e}"
        c_gpu = np.abs(got["components"] - r64["components"]).max(axis=1)
        c_32 = np.abs(r32["components"] - r64["components"]).max(axis=1)
        bound = np.maximum(8 * c_32, d * EPS32 / relgap)
        print(f"pca accuracy {label} {shape} components: worst gpu/bound {np.max(c_gpu / bound):.3e}, gpu max {c_gpu.max():.3e}")
        if not np.all(c_gpu <= bound):
            bad.append("components")
    assert not bad, f"{label} {shape}: beyond the accuracy rule: {bad}"


@pytest.mark.parametrize("shape", COMPONENT_SHAPES + FULL_SHAPES)
def test_fit_meets_the_accuracy_rule(res, shape):
    n, d, k = shape
    got = gpu_fit(res, _data()[shape], k)
    assert got["sweeps"] >= 1
    _check_rule(got, shape, componentwise=shape in COMPONENT_SHAPES)
    if n < d:  # rank-deficient: the trailing spectrum is clamped, never negative or NaN
        for q in ("explained_var", "singular_vals"):
            assert np.all(np.isfinite(got[q])) and np.all(got[q] >= 0)
        assert np.all(got["explained_var"][n:] <= d * EPS32 * got["explained_var"][0])


def test_long_rows_and_a_large_mean(res):
    """Held to the floor d eps32 alone: the float32 restatement adds 300000 rows around 1000 in order and is itself off by
    5.6 lambda_0 here, which would make the rule's other term no bound at all. tests/test_pca_cpu.py shows that an uncentred
    Gram matrix and an unbroken fp32 chain miss this bound by more than 10 x."""
    X, r64 = pca_ref.long_rows_case()
    n, d = X.shape
    got = gpu_fit(res, X, d, layout="C")
    e_gpu = np.abs(got["explained_var"] - r64["explained_var"]).max() / r64["eigenvalues"][0]
    print(f"pca long rows: eigenvalues gpu {e_gpu:.3e} floor {d * EPS32:.3e}")
    assert e_gpu <= d * EPS32
    assert np.abs(got["mu"] - r64["mu"]).max() <= np.spacing(np.float32(np.abs(r64["mu"]).max()))


@pytest.mark.parametrize("layout", ["F", "C"])
def test_row_ranges_longer_than_one_fp32_chain(res, layout):
    """2.2M x 8: a covariance workgroup owns 8640 rows and has to move its fp32 sums into fp64 after 8192 of them. The data
    (tests/pca_ref.py flush_case) puts a chain that is not broken there 2.5e-5 off; the bound is the floor d eps32 = 9.5e-7."""
    X, lam = pca_ref.flush_case()
    n, d = X.shape
    got = gpu_fit(res, X, d, layout=layout)
    assert np.all(got["mu"] == 0)
    e_gpu = np.abs(got["explained_var"].astype(np.float64) - lam).max() / lam
    print(f"pca flush case {layout}: eigenvalues gpu {e_gpu:.3e} floor {d * EPS32:.3e}")
    assert e_gpu <= d * EPS32
    assert abs(float(got["explained_var_ratio"].sum()) - 1) <= d * EPS32 and abs(float(got["noise_vars"])) <= d * EPS32 * lam


@functools.lru_cache(maxsize=None)
def _projection_case(shape, whiten):
    """The GPU's own fit of the case, and the exact chain's results for it (computed once, shared by the layout pairings)."""
    import cuvs_amd

    n, d, k = shape
    rng = np.random.default_rng(23)
    X = (rng.standard_normal((n, d)) * 2.0 ** (-np.arange(d) / 8) + rng.standard_normal(d)).astype(np.float32)
    res = cuvs_amd.common.Resources()
    fit = gpu_fit(res, X, k)
    T = pca_ref.transform_exact(X, fit["components"], fit["singular_vals"], fit["mu"], whiten)
    Y = pca_ref.inverse_transform_exact(T, fit["components"], fit["singular_vals"], fit["mu"], whiten)
    assert np.all(np.isfinite(T)) and np.all(np.isfinite(Y))
    return X, fit, T, Y


@pytest.mark.parametrize("out_layout", ["F", "C"])
@pytest.mark.parametrize("in_layout", ["F", "C"])
@pytest.mark.parametrize("whiten", [False, True])
@pytest.mark.parametrize("shape", [(257, 33, 5), (64, 130, 130)])
def test_projections_are_the_fmaf_chain_bit_for_bit(res, shape, whiten, in_layout, out_layout):
    n, d, k = shape
    X, fit, T, Y = _projection_case(shape, whiten)
    comp_layout = in_layout  # components travels in each layout once per output layout
    comp, sv, mu = _dev(fit["components"], comp_layout), fit["dev"][1], fit["dev"][2]
    t = gpu_transform(res, _dev(X, in_layout), comp, sv, mu, k, whiten, out_layout)
    assert np.array_equal(t.cpu().numpy(), T)
    y = gpu_transform(res, _dev(T, in_layout), comp, sv, mu, k, whiten, out_layout, inverse=True)
    assert np.array_equal(y.cpu().numpy(), Y)


@pytest.mark.parametrize("whiten", [False, True])
def test_fit_transform_returns_the_bits_of_transform(res, whiten):
    shape = (257, 33, 5)
    X = _data()[shape]
    for layout, trans_layout in (("F", "F"), ("C", "C"), ("F", "C")):
        got = gpu_fit(res, X, 5, layout=layout, trans_layout=trans_layout, whiten=whiten)
        comp, sv, mu = got["dev"]
        t = gpu_transform(res, _dev(X, layout), comp, sv, mu, 5, whiten, trans_layout)
        assert torch.equal(t, got["trans_input"])
        exact = pca_ref.transform_exact(X, got["components"], got["singular_vals"], got["mu"], whiten)
        assert np.array_equal(t.cpu().numpy(), exact)


def test_fit_does_not_depend_on_the_layout(res):
    shape = (1000, 72, 9)
    X = _data()[shape]
    f = gpu_fit(res, X, 9, layout="F", comp_layout="F")
    c = gpu_fit(res, X, 9, layout="C", comp_layout="C")
    assert np.array_equal(f["mu"], c["mu"])
    _check_rule(c, shape, componentwise=True, label="row-major")
    _check_rule(f, shape, componentwise=True, label="column-major")


def test_fit_is_deterministic(res):
    shape = (4099, 130, 17)
    a, b = gpu_fit(res, _data()[shape], 17), gpu_fit(res, _data()[shape], 17)
    for q in ("components", "explained_var", "explained_var_ratio", "singular_vals", "mu", "noise_vars"):
        assert np.array_equal(a[q], b[q]), q
    assert a["sweeps"] == b["sweeps"]


def test_sign_rules(res):
    shape = (257, 33, 5)
    X = _data()[shape]
    v, u = gpu_fit(res, X, 5), gpu_fit(res, X, 5, flip_u=True)
    for row in v["components"]:
        assert row[np.argmax(np.abs(row))] > 0
    assert np.array_equal(v["components"], pca_ref.apply_v_sign(v["components"]))
    comp, sv, mu = u["dev"]
    T = gpu_transform(res, _dev(X, "F"), comp, sv, mu, 5, False, "C").cpu().numpy()
    for i in range(5):
        assert T[np.argmax(np.abs(T[:, i])), i] > 0
    signs = np.sign((v["components"] * u["components"]).sum(axis=1))
    assert np.all(np.abs(signs) == 1)
    assert np.array_equal(u["components"], v["components"] * signs[:, None])
    for q in ("explained_var", "singular_vals", "mu"):
        assert np.array_equal(u[q], v[q])


def test_jacobi_parameters(res):
    shape = (1000, 72, 9)
    X = _data()[shape]
    r64 = _refs(shape)[0]
    resid = lambda g: _residual(r64["cov"], g["explained_var"], g["components"])  # noqa: E731
    full = gpu_fit(res, X, 9, algorithm="cov_eig_jacobi")
    _check_rule(full, shape, componentwise=True, label="jacobi-15")
    assert 1 <= full["sweeps"] <= 15
    one = gpu_fit(res, X, 9, algorithm="cov_eig_jacobi", n_iterations=1)
    assert one["sweeps"] == 1
    assert resid(one) > resid(full)
    loose = gpu_fit(res, X, 9, algorithm="cov_eig_jacobi", tol=1e-2)
    assert 1 <= loose["sweeps"] <= full["sweeps"]
    assert loose["sweeps"] < full["sweeps"] or resid(loose) == resid(full)
    dq = gpu_fit(res, X, 9)
    assert dq["sweeps"] == full["sweeps"] and np.array_equal(dq["components"], full["components"])


def test_input_is_left_alone_with_copy_false(res):
    X = _data()[(257, 33, 5)]
    for layout in ("F", "C"):
        x = _dev(X, layout)
        before = x.clone()
        gpu_fit(res, x, 5, copy=False, trans_layout="C")
        assert torch.equal(x, before)


def test_whitening_with_a_zero_singular_value_stays_finite(res):
    rng = np.random.default_rng(5)
    X = rng.standard_normal((200, 6)).astype(np.float32)
    X[:, 3] = X[:, 1]
    got = gpu_fit(res, X, 6, whiten=True, trans_layout="C")
    comp, sv, mu = got["dev"]
    sv[-1] = 0.0  # whatever rounding left of the null direction: the contract is about an exact zero
    t = gpu_transform(res, _dev(X, "C"), comp, sv, mu, 6, True, "C")
    y = gpu_transform(res, t, comp, sv, mu, 6, True, "C", inverse=True)
    assert torch.isfinite(got["trans_input"]).all() and torch.isfinite(t).all() and torch.isfinite(y).all()
    assert torch.all(t[:, -1] == 0)


# ---- the reference's own checks (tests/golden/pca_reference_table.json)
@pytest.mark.parametrize("algorithm", ["cov_eig_dq", "cov_eig_jacobi"])
def test_reference_known_answer(res, algorithm):
    ka = TABLE["known_answer"]
    n, d, tol = ka["n_rows"], ka["n_cols"], ka["tolerance"]
    X = np.array(ka["input_col_major"], dtype=np.float32).reshape(d, n).T
    got = gpu_fit(res, X, d, algorithm=algorithm, trans_layout="F")
    assert np.abs(got["components"] - np.array(ka["components_col_major"]).reshape(d, d).T).max() < tol
    assert np.abs(got["explained_var"] - np.array(ka["explained_vars"])).max() < tol
    assert np.abs(got["trans_input"].cpu().numpy() - np.array(ka["trans_data_col_major"]).reshape(d, n).T).max() < tol


@pytest.mark.parametrize("row", TABLE["parameter_table"], ids=lambda r: f"{r['n_row2']}x{r['n_col2']}")
def test_reference_round_trips(res, row):
    n, d, tol = row["n_row2"], row["n_col2"], row["tolerance"]
    algorithm = pca.SOLVER_NAMES[row["algorithm"]]
    rng = np.random.default_rng(row["seed"])
    lo, hi = TABLE["random_data"]["low"], TABLE["random_data"]["high"]
    X = rng.uniform(lo, hi, (n, d)).astype(np.float32)
    got = gpu_fit(res, X, d, algorithm=algorithm, trans_layout="F")
    comp, sv, mu = got["dev"]
    back = gpu_transform(res, got["trans_input"], comp, sv, mu, d, False, "F", inverse=True)
    assert np.abs(back.cpu().numpy() - X).max() < tol
    k = max(1, d // TABLE["dim_reduction"]["n_components_divisor"])
    X2 = np.random.default_rng(row["seed"] + 1).uniform(lo, hi, (n, d)).astype(np.float32)
    got = gpu_fit(res, X2, k, algorithm=algorithm, trans_layout="F")
    comp, sv, mu = got["dev"]
    back = gpu_transform(res, got["trans_input"], comp, sv, mu, k, False, "F", inverse=True)
    assert np.abs(back.cpu().numpy() - X2).max() > TABLE["dim_reduction"]["error_above"]


def test_python_module_meets_the_reference_python_bounds():
    b = TABLE["python_bounds"]
    gen = torch.Generator(device="cpu").manual_seed(0)
    for n in b["round_trip"]["n_rows"]:
        for d in b["round_trip"]["n_cols"]:
            X = torch.rand((n, d), generator=gen).cuda()
            params = pca.Params(n_components=d)
            r = pca.fit_transform(params, X)
            assert isinstance(r, pca.FitTransformOutput) and r.trans_input.shape == (n, d) and r.components.shape == (d, d)
            back = pca.inverse_transform(params, r.trans_input, r.components, r.singular_vals, r.mu)
            assert float((X - back).abs().max()) < b["round_trip"]["max_abs_error_below"]
            f = pca.fit(pca.Params(n_components=d, copy=True), X)
            assert isinstance(f, pca.FitOutput) and f.singular_vals.shape == (d,) and f.mu.shape == (d,)
            t = pca.transform(params, X, f.components, f.singular_vals, f.mu)
            assert t.is_contiguous() and torch.equal(t, r.trans_input)
            back = pca.inverse_transform(params, t, f.components, f.singular_vals, f.mu)
            assert float((X - back).abs().max()) < b["round_trip"]["max_abs_error_below"]
    dr = b["dim_reduction"]
    X = torch.rand((dr["n_rows"], dr["n_cols"]), generator=gen).cuda()
    for k in dr["n_components"]:
        params = pca.Params(n_components=k)
        r = pca.fit_transform(params, X)
        assert r.trans_input.shape == (dr["n_rows"], k)
        # a caller's buffers, column-major, are filled in place
        buf = torch.empty((dr["n_cols"], dr["n_rows"]), dtype=torch.float32, device="cuda").t()
        back = pca.inverse_transform(params, r.trans_input, r.components, r.singular_vals, r.mu, output=buf)
        assert back is buf
        err = float((X - back).abs().max())
        assert dr["error_above"] < err < dr["error_below"]
        tb = torch.empty((k, dr["n_rows"]), dtype=torch.float32, device="cuda").t()
        assert torch.equal(pca.transform(params, X, r.components, r.singular_vals, r.mu, trans_input=tb), r.trans_input)
    ev = b["explained_variance"]
    X = torch.rand((ev["n_rows"], ev["n_cols"]), generator=gen).cuda()
    f = pca.fit(pca.Params(n_components=ev["n_cols"]), X)
    assert abs(float(f.explained_var_ratio.sum()) - 1.0) < ev["ratio_sum_within"]
    assert bool((f.explained_var >= 0).all()) and bool((f.singular_vals >= 0).all())
    u = pca.fit(pca.Params(n_components=4), X, flip_signs_based_on_U=True)
    assert torch.equal(u.components.abs(), f.components[:4].abs())
