"""CPU: the PCA C ABI (include/cuvs/preprocessing/pca.h) is exported with the reference's layout and defaults, refuses bad
arguments before it touches a device, and tests/pca_ref.py restates the reference's own known answer."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from tests import pca_ref
from cuvs_amd._lib import Tensor, kDLCUDA, lib
from cuvs_amd.preprocessing import pca

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
TABLE = json.load(open(os.path.join(GOLDEN, "pca_reference_table.json")))


def test_every_prototype_of_the_header_is_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cuvs", "preprocessing", "pca.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"CUVS_EXPORT\s+cuvsError_t\s+(cuvsPca\w+)\s*\(", text)))
    assert names == ["cuvsPcaFit", "cuvsPcaFitTransform", "cuvsPcaInverseTransform", "cuvsPcaParamsCreate",
                     "cuvsPcaParamsDestroy", "cuvsPcaTransform"]
    for n in names + ["cuvsAmdPcaLastSweeps"]:
        assert hasattr(lib(), n), n


def test_struct_layout_matches_the_reference_header(tmp_path):
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(GOLDEN, "pca_abi_probe.c"), "-o", str(exe)])
    assert subprocess.check_output([str(exe)]).decode() == open(os.path.join(GOLDEN, "pca_abi_layout.txt")).read()


def test_umbrella_header_declares_pca_as_c99_and_cxx17(tmp_path):
    src = tmp_path / "p.c"
    src.write_text("#include <cuvs/core/all.h>\n"
                   "int main(void) { struct cuvsPcaParams p; p.algorithm = CUVS_PCA_COV_EIG_JACOBI; p.whiten = false;\n"
                   "  return cuvsPcaTransform == 0 || p.algorithm != 1 || p.whiten; }\n")
    inc = os.path.join(ROOT, "include")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Werror", "-Wno-address", "-fsyntax-only", "-I", inc, str(src)])
    subprocess.check_call(["g++", "-std=c++17", "-Werror", "-Wno-address", "-fsyntax-only", "-x", "c++", "-I", inc, str(src)])


def test_parameter_defaults():
    p = C.POINTER(pca._CParams)()
    assert lib().cuvsPcaParamsCreate(C.byref(p)) == 1
    c = p.contents
    assert (c.n_components, c.copy, c.whiten, c.algorithm, c.tol, c.n_iterations) == (1, True, False, 0, 0.0, 15)
    assert lib().cuvsPcaParamsDestroy(p) == 1
    assert lib().cuvsPcaParamsCreate(None) == 0
    q = pca.Params()
    assert (q.n_components, q.copy, q.whiten, q.algorithm, q.tol, q.n_iterations) == (1, True, False, "cov_eig_dq", 0.0, 15)
    q = pca.Params(n_components=10, copy=False, whiten=True, algorithm="cov_eig_jacobi", tol=1e-4, n_iterations=50)
    assert (q.n_components, q.copy, q.whiten, q.algorithm, q.n_iterations) == (10, False, True, "cov_eig_jacobi", 50)
    assert abs(q.tol - 1e-4) < 1e-7
    with pytest.raises(ValueError):
        pca.Params(algorithm="svd")


def test_float64_restatement_reproduces_the_reference_known_answer():
    ka = TABLE["known_answer"]
    n, d, tol = ka["n_rows"], ka["n_cols"], ka["tolerance"]
    X = np.array(ka["input_col_major"]).reshape(d, n).T
    r = pca_ref.fit(X, d)
    assert np.abs(r["components"] - np.array(ka["components_col_major"]).reshape(d, d).T).max() < tol
    assert np.abs(r["explained_var"] - np.array(ka["explained_vars"])).max() < tol
    T = (X - r["mu"]) @ r["components"].T
    assert np.abs(T - np.array(ka["trans_data_col_major"]).reshape(d, n).T).max() < tol
    T32 = pca_ref.transform_exact(X, r["components"], r["singular_vals"], r["mu"], False)
    assert np.abs(T32 - T).max() < 1e-5
    back = pca_ref.inverse_transform_exact(T32, r["components"], r["singular_vals"], r["mu"], False)
    assert np.abs(back - X).max() < 1e-5


def test_fma32_is_the_c_library_fmaf():
    libm = C.CDLL("libm.so.6")
    libm.fmaf.restype = C.c_float
    libm.fmaf.argtypes = [C.c_float] * 3
    rng = np.random.default_rng(3)
    a = rng.standard_normal(4000).astype(np.float32)
    b = rng.standard_normal(4000).astype(np.float32)
    c = (-(a.astype(np.float64) * b.astype(np.float64)) * (1 + rng.integers(-3, 4, 4000) * 2.0 ** -24)).astype(np.float32)
    # half-way cases whose tail is below the fp64 rounding unit: (1 + 2^-15)(1 - 2^-15) = 1 - 2^-30, added to 2^24 + 2 the fp64 sum
    # is the fp32 mid-point 2^24 + 3, which ties-to-even would take up to 2^24 + 4; the tail says down
    a[:2] = np.float32(1 + 2.0 ** -15)
    b[:2] = [1 - 2.0 ** -15, -(1 - 2.0 ** -15)]
    c[:2] = [2.0 ** 24 + 2, -(2.0 ** 24 + 2)]
    got = pca_ref.fma32(a, b, c)
    want = np.array([libm.fmaf(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], dtype=np.float32)
    assert np.array_equal(got, want)
    assert got[0] == 2.0 ** 24 + 2 and got[1] == -(2.0 ** 24 + 2)


# ---- validation: numpy-backed tensors and a null handle; a case that passes validation would fail on the null handle, so
# every message is checked to name its own cause
class _Args:
    """The tensors of one well-formed call at (n, d, k); `device` marks them as device memory without there being any."""

    def __init__(self, n=6, d=4, k=2, device=True, dtype=np.float32):
        self.n, self.d, self.k, self.device = n, d, k, device
        z = lambda *s: np.zeros(s, dtype=dtype)  # noqa: E731
        self.t = dict(input=z(n, d), trans_input=z(n, k), components=z(k, d), explained_var=z(k), explained_var_ratio=z(k),
                      singular_vals=z(k), mu=z(d), noise_vars=z(1), output=z(n, d))
        self.params = pca.Params(n_components=k)

    def tensor(self, name):
        t = Tensor(self.t[name])
        if self.device:
            t.m.dl_tensor.device.device_type = kDLCUDA
        return t


_CALLS = {
    "cuvsPcaFit": ["input", "components", "explained_var", "explained_var_ratio", "singular_vals", "mu", "noise_vars"],
    "cuvsPcaFitTransform": ["input", "trans_input", "components", "explained_var", "explained_var_ratio", "singular_vals", "mu",
                            "noise_vars"],
    "cuvsPcaTransform": ["input", "components", "singular_vals", "mu", "trans_input"],
    "cuvsPcaInverseTransform": ["trans_input", "components", "singular_vals", "mu", "output"],
}


def _error_of(call, args):
    tensors = [args.tensor(name) for name in _CALLS[call]]
    extra = [C.c_bool(False)] if "Fit" in call else []
    lib().cuvsSetLastErrorText(b"")
    status = getattr(lib(), call)(C.c_size_t(0), args.params._p, *[t.ptr for t in tensors], *extra)
    assert status == 0, f"{call} accepted the arguments"
    text = lib().cuvsGetLastErrorText()
    assert text, f"{call} left no message"
    return text.decode()


@pytest.mark.parametrize("call", sorted(_CALLS))
def test_bad_arguments_are_refused_without_a_device(call):
    first = _CALLS[call][0]
    last = _CALLS[call][-1] if "Fit" not in call else "components"
    # well-formed arguments reach the null handle: validation itself lets them through
    assert "null cuvsResources_t" in _error_of(call, _Args())
    assert "device memory" in _error_of(call, _Args(device=False))
    assert "float32" in _error_of(call, _Args(dtype=np.float64))
    a = _Args()
    a.t[first] = np.zeros((a.t[first].shape[0], 2 * a.t[first].shape[1]), dtype=np.float32)[:, ::2]
    assert "strides" in _error_of(call, a)
    a = _Args(k=2, d=4)
    a.params = pca.Params(n_components=5)
    assert "n_components" in _error_of(call, a)
    a = _Args()
    a.params = pca.Params(n_components=0)
    assert "n_components" in _error_of(call, a)
    assert "4096" in _error_of(call, _Args(n=3, d=4097, k=2))
    assert "2 rows" in _error_of(call, _Args(n=1))
    a = _Args()
    a.t[last] = np.zeros((a.t[last].shape[0] + 1, a.t[last].shape[1]), dtype=np.float32)
    assert last in _error_of(call, a) and "must be [" in _error_of(call, a)
    a = _Args()
    a.t["mu"] = np.zeros(a.d + 1, dtype=np.float32)
    assert "mu" in _error_of(call, a)
    if "Fit" in call:  # a bounded solver without a sweep would hand back the identity
        a = _Args()
        a.params = pca.Params(n_components=2, algorithm="cov_eig_jacobi", n_iterations=0)
        assert "n_iterations" in _error_of(call, a)
    # either layout of every matrix passes validation
    a = _Args()
    for name in ("input", "trans_input", "components", "output"):
        a.t[name] = np.asfortranarray(a.t[name])
    assert "null cuvsResources_t" in _error_of(call, a)


# ---- the two long-row GPU cases of tests/test_pca_gpu.py would catch what they are there for: the faulty variants, restated
# here in numpy, miss the bound d * eps32 those tests assert
def test_long_rows_bound_rejects_an_uncentred_gram_and_an_unbroken_chain():
    X, r64 = pca_ref.long_rows_case()
    n, d = X.shape
    lam0, floor = r64["eigenvalues"][0], d * pca_ref.EPS32
    err = lambda cov: np.abs(np.sort(np.linalg.eigvalsh(cov.astype(np.float64)))[::-1] - r64["eigenvalues"]).max() / lam0  # noqa: E731
    mu = r64["mu"].astype(np.float32)
    Xc = X - mu
    # centred, but one fp32 chain over all rows (np.cumsum adds in order)
    chain = np.array([[np.cumsum(Xc[:, i] * Xc[:, j], dtype=np.float32)[-1] for j in range(d)] for i in range(d)])
    assert err(chain / np.float32(n - 1)) > 10 * floor
    # X^T X - n mu mu^T with the Gram matrix held in fp32
    gram = (X.astype(np.float64).T @ X.astype(np.float64)).astype(np.float32)
    uncentred = (gram.astype(np.float64) - n * np.outer(mu, mu).astype(np.float64)) / (n - 1)
    assert err(uncentred) > 10 * floor
    # what the kernel does: chains of 1216 rows in fp32, combined in fp64
    parts = [np.cumsum(Xc[r:r + 1216, :, None] * Xc[r:r + 1216, None, :], axis=0, dtype=np.float32)[-1].astype(np.float64)
             for r in range(0, n, 1216)]
    assert err(np.sum(parts, axis=0) / (n - 1)) <= floor


def test_flush_case_bound_rejects_a_chain_past_8192_rows():
    a2 = float(np.float32(pca_ref.FLUSH_CASE_A)) ** 2
    rows = pca_ref.FLUSH_CASE_SPLIT_ROWS
    assert rows > 8192

    def chain(count, start=np.float32(0)):
        s = start
        for _ in range(count):
            s = np.float32(float(s) + a2)  # the sum is exact in float64, rounded once: an fp32 fma
        return s

    upto = chain(8192)
    unbroken = float(chain(rows - 8192, upto))
    flushed = float(upto) + float(chain(rows - 8192))
    floor = 8 * pca_ref.EPS32
    assert abs(unbroken - rows * a2) / (rows * a2) > 10 * floor
    assert abs(flushed - rows * a2) / (rows * a2) <= floor / 4
