"""PCA (reference: python/cuvs/cuvs/preprocessing/pca/pca.pyx over c/include/cuvs/preprocessing/pca.h): fit, transform and
inverse transform of fp32 device matrices.

Differences from the reference's module: matrices are torch device tensors and are passed on in the layout they come in
(row-major or column-major, no copy to Fortran order: the C layer takes both); the arrays this module allocates are row-major,
where the reference returns Fortran-ordered cupy arrays, so a projected corpus goes straight into an index build.
`trans_input=` / `output=` buffers of either layout are filled in place."""
import ctypes as C
from collections import namedtuple

import torch

from .._lib import Tensor, check, lib
from ..common import Resources

SOLVER_NAMES = {0: "cov_eig_dq", 1: "cov_eig_jacobi"}
_SOLVER_IDS = {v: k for k, v in SOLVER_NAMES.items()}


class _CParams(C.Structure):
    _fields_ = [("n_components", C.c_int), ("copy", C.c_bool), ("whiten", C.c_bool), ("algorithm", C.c_int),
                ("tol", C.c_float), ("n_iterations", C.c_int)]


class Params:
    """n_components (1), copy (True; the input is never written either way), whiten (False), algorithm ("cov_eig_dq" or
    "cov_eig_jacobi"), tol (0.0) and n_iterations (15) of the Jacobi solver."""

    def __init__(self, *, n_components=None, copy=None, whiten=None, algorithm=None, tol=None, n_iterations=None):
        self._p = C.POINTER(_CParams)()
        check(lib().cuvsPcaParamsCreate(C.byref(self._p)))
        p = self._p.contents
        if n_components is not None:
            p.n_components = n_components
        if copy is not None:
            p.copy = copy
        if whiten is not None:
            p.whiten = whiten
        if algorithm is not None:
            if algorithm not in _SOLVER_IDS:
                raise ValueError(f"algorithm must be one of {sorted(_SOLVER_IDS)}, got {algorithm!r}")
            p.algorithm = _SOLVER_IDS[algorithm]
        if tol is not None:
            p.tol = tol
        if n_iterations is not None:
            p.n_iterations = n_iterations

    n_components = property(lambda self: self._p.contents.n_components)
    copy = property(lambda self: self._p.contents.copy)
    whiten = property(lambda self: self._p.contents.whiten)
    algorithm = property(lambda self: SOLVER_NAMES[self._p.contents.algorithm])
    tol = property(lambda self: self._p.contents.tol)
    n_iterations = property(lambda self: self._p.contents.n_iterations)

    def __del__(self):
        try:
            lib().cuvsPcaParamsDestroy(self._p)
        except Exception:
            pass


FitOutput = namedtuple("FitOutput", "components explained_var explained_var_ratio singular_vals mu noise_vars")
FitTransformOutput = namedtuple("FitTransformOutput",
                                "trans_input components explained_var explained_var_ratio singular_vals mu noise_vars")


def _check_matrix(x, what):
    if not (isinstance(x, torch.Tensor) and x.is_cuda):
        raise TypeError(f"{what} must be a torch tensor on the device")
    if x.dtype != torch.float32:
        raise TypeError(f"{what} must be float32, got {x.dtype}")
    if x.dim() != 2:
        raise ValueError(f"{what} must be a 2-D matrix")


def _call(fn, resources, *args):
    own = resources is None
    resources = Resources() if own else resources
    check(fn(resources.get_c_obj(), *args))
    if own:
        resources.sync()


def _fit_outputs(params, x):
    k, d = params.n_components, x.shape[1]
    e = lambda *shape: torch.empty(shape, dtype=torch.float32, device=x.device)  # noqa: E731
    return FitOutput(e(k, d), e(k), e(k), e(k), e(d), e(1))


def fit(params, X, resources=None, *, flip_signs_based_on_U=False):
    """cuvsPcaFit: FitOutput(components [k, d], explained_var [k], explained_var_ratio [k], singular_vals [k], mu [d],
    noise_vars [1]) of X [n, d]."""
    _check_matrix(X, "X")
    out = _fit_outputs(params, X)
    _call(lib().cuvsPcaFit, resources, params._p, Tensor(X).ptr, *[Tensor(t).ptr for t in out], C.c_bool(flip_signs_based_on_U))
    return out


def fit_transform(params, X, resources=None, *, trans_input=None, flip_signs_based_on_U=False):
    """cuvsPcaFitTransform: fit, and trans_input [n, k] = transform(X) with the fitted outputs."""
    _check_matrix(X, "X")
    out = _fit_outputs(params, X)
    if trans_input is None:
        trans_input = torch.empty((X.shape[0], params.n_components), dtype=torch.float32, device=X.device)
    _call(lib().cuvsPcaFitTransform, resources, params._p, Tensor(X).ptr, Tensor(trans_input).ptr, *[Tensor(t).ptr for t in out],
          C.c_bool(flip_signs_based_on_U))
    return FitTransformOutput(trans_input, *out)


def transform(params, X, components, singular_vals, mu, trans_input=None, resources=None):
    """cuvsPcaTransform: (X - mu) components^T as [n, k] (row-major when allocated here)."""
    _check_matrix(X, "X")
    if trans_input is None:
        trans_input = torch.empty((X.shape[0], params.n_components), dtype=torch.float32, device=X.device)
    _call(lib().cuvsPcaTransform, resources, params._p, Tensor(X).ptr, Tensor(components).ptr, Tensor(singular_vals).ptr,
          Tensor(mu).ptr, Tensor(trans_input).ptr)
    return trans_input


def inverse_transform(params, trans_input, components, singular_vals, mu, output=None, resources=None):
    """cuvsPcaInverseTransform: trans_input components + mu as [n, d] (row-major when allocated here)."""
    _check_matrix(trans_input, "trans_input")
    if output is None:
        output = torch.empty((trans_input.shape[0], components.shape[1]), dtype=torch.float32, device=trans_input.device)
    _call(lib().cuvsPcaInverseTransform, resources, params._p, Tensor(trans_input).ptr, Tensor(components).ptr,
          Tensor(singular_vals).ptr, Tensor(mu).ptr, Tensor(output).ptr)
    return output
