/*
 * Principal component analysis — drop-in for c/include/cuvs/preprocessing/pca.h.
 * Enum values, struct field order and the argument lists are ABI. Implemented by cuvs_amd/csrc/pca.hip.
 *
 * With n = rows, d = columns, k = n_components (1 <= k <= d <= 4096, n >= 2), all tensors fp32 on the device:
 *   mu[j]            column mean (summed in fp64, rounded once)
 *   C                (X - mu)^T (X - mu) / (n - 1), centred while it is accumulated
 *   explained_var    the k largest eigenvalues of C, descending, clamped at 0
 *   components[i]    the unit eigenvector of eigenvalue i ([k, d])
 *   singular_vals    sqrt(explained_var * (n - 1))
 *   explained_var_ratio  explained_var / trace(C)
 *   noise_vars[0]    mean of the d - k eigenvalues not kept (0 when k == d)
 *   transform        (X - mu) W^T, inverse transform T W + mu, with W = components; when `whiten` is set row i of W is
 *                    first scaled by sqrtf(n - 1) / singular_vals[i] (transform) or its inverse (inverse transform), n being
 *                    the row count of that call's input; a zero singular value gives scale 0 both ways
 * Sign of components[i]: its entry of largest magnitude is positive (lowest index on a tie); with flip_signs_based_on_U
 * the entry of largest magnitude of column i of (X - mu) components^T is positive instead.
 *
 * Layouts: the reference takes column-major (Fortran-contiguous) matrices only. This library takes those and, for each
 * 2-D argument independently, C-contiguous (row-major) ones as well; any other stride pattern is refused.
 * `copy`: the input is never written, whatever `copy` says (the reference merely MAY overwrite it when copy is false).
 * Both solver values run the same device eigensolver (parallel cyclic Jacobi): COV_EIG_DQ until a sweep rotates nothing,
 * COV_EIG_JACOBI for at most n_iterations sweeps or until the largest |a_pq| / sqrt(a_pp a_qq) of a sweep is <= tol
 * (tol 0: until a sweep rotates nothing).
 * Arguments are validated before the device is touched.
 */
#pragma once
#include <cuvs/core/c_api.h>
#include <cuvs/core/export.h>
#include <dlpack/dlpack.h>
#include <stdbool.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

enum cuvsPcaSolver {
  CUVS_PCA_COV_EIG_DQ     = 0, /* covariance + eigendecomposition run to convergence */
  CUVS_PCA_COV_EIG_JACOBI = 1  /* covariance + eigendecomposition bounded by tol / n_iterations */
};

struct cuvsPcaParams {
  int n_components;             /* 1: components kept */
  bool copy;                    /* true: accepted and ignored, the input is never written */
  bool whiten;                  /* false: scale the projections to unit variance per component */
  enum cuvsPcaSolver algorithm; /* CUVS_PCA_COV_EIG_DQ */
  float tol;                    /* 0: COV_EIG_JACOBI stops when a sweep's largest relative off-diagonal is <= tol */
  int n_iterations;             /* 15: most sweeps of COV_EIG_JACOBI */
};
typedef struct cuvsPcaParams* cuvsPcaParams_t;
CUVS_EXPORT cuvsError_t cuvsPcaParamsCreate(cuvsPcaParams_t* params);
CUVS_EXPORT cuvsError_t cuvsPcaParamsDestroy(cuvsPcaParams_t params);

/* input [n, d]; components [k, d]; explained_var, explained_var_ratio, singular_vals [k]; mu [d]; noise_vars [1] */
CUVS_EXPORT cuvsError_t cuvsPcaFit(cuvsResources_t res,
                                   cuvsPcaParams_t params,
                                   DLManagedTensor* input,
                                   DLManagedTensor* components,
                                   DLManagedTensor* explained_var,
                                   DLManagedTensor* explained_var_ratio,
                                   DLManagedTensor* singular_vals,
                                   DLManagedTensor* mu,
                                   DLManagedTensor* noise_vars,
                                   bool flip_signs_based_on_U);

/* cuvsPcaFit, then trans_input [n, k] = cuvsPcaTransform of the input with the fitted outputs (the same bits) */
CUVS_EXPORT cuvsError_t cuvsPcaFitTransform(cuvsResources_t res,
                                            cuvsPcaParams_t params,
                                            DLManagedTensor* input,
                                            DLManagedTensor* trans_input,
                                            DLManagedTensor* components,
                                            DLManagedTensor* explained_var,
                                            DLManagedTensor* explained_var_ratio,
                                            DLManagedTensor* singular_vals,
                                            DLManagedTensor* mu,
                                            DLManagedTensor* noise_vars,
                                            bool flip_signs_based_on_U);

/* trans_input [n, k] = (input - mu) components^T; element (r, i) is the fp32 chain acc = fmaf(input[r][j] - mu[j], W[i][j], acc)
 * over j ascending from acc = 0 */
CUVS_EXPORT cuvsError_t cuvsPcaTransform(cuvsResources_t res,
                                         cuvsPcaParams_t params,
                                         DLManagedTensor* input,
                                         DLManagedTensor* components,
                                         DLManagedTensor* singular_vals,
                                         DLManagedTensor* mu,
                                         DLManagedTensor* trans_input);

/* output [n, d] = trans_input components + mu; the same chain over i ascending, mu added last */
CUVS_EXPORT cuvsError_t cuvsPcaInverseTransform(cuvsResources_t res,
                                                cuvsPcaParams_t params,
                                                DLManagedTensor* trans_input,
                                                DLManagedTensor* components,
                                                DLManagedTensor* singular_vals,
                                                DLManagedTensor* mu,
                                                DLManagedTensor* output);
#ifdef __cplusplus
}
#endif
