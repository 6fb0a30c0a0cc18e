/* Spectral embedding and spectral clustering. The reference has these in C++ only
 * (cpp/include/cuvs/preprocessing/spectral_embedding.hpp: transform, helpers::create_connectivity_graph;
 * cpp/include/cuvs/cluster/spectral.hpp: fit_predict); these entry points are extensions in the conventions of the cuvs* C
 * layer. Implemented by cuvs_amd/csrc/spectral.hip; DESIGN.md 3.1w has the contract.
 *
 * Graph: the exact kNN graph of cuvsAllNeighborsBuild (brute force, L2SqrtExpanded, k = n_neighbors, ids as returned, the row
 * itself among them), every (i, j) a directed entry of weight 1, symmetrised as 0.5 (a_ij + a_ji), sorted by (row, col).
 * Laplacian: scipy.sparse.csgraph.laplacian's semantics - duplicate entries are summed, diagonal entries of the input are
 * ignored, deg_i = sum of w_ij over j != i; L = D - W, or L = I - D^-1/2 W D^-1/2 with sqrt(deg_i) replaced by 1 and L_ii = 0
 * for an isolated vertex. A graph passed in as COO is ASSUMED SYMMETRIC; this is not checked. Entries outside [0, n) are refused.
 * Solver: thick-restart Lanczos in fp32 with two passes of classical Gram-Schmidt against the whole basis per step; no
 * floating-point atomics, so the same inputs and seed give bit-identical output on the same device.
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

struct cuvsAmdSpectralEmbeddingParams {
  int n_components;    /* 2: eigenpairs computed; columns of the embedding BEFORE drop_first takes one away */
  int n_neighbors;     /* 15: k of the kNN graph (ignored by the *Graph entry points) */
  bool norm_laplacian; /* true */
  bool drop_first;     /* true: the first eigenvector (constant on a connected graph) is left out */
  float tolerance;     /* 1e-5; 0: fp32 machine epsilon. Values above machine epsilon are tightened to it */
  uint64_t seed;       /* 0: sets the start vector */
};
typedef struct cuvsAmdSpectralEmbeddingParams* cuvsAmdSpectralEmbeddingParams_t;

CUVS_EXPORT cuvsError_t cuvsAmdSpectralEmbeddingParamsCreate(cuvsAmdSpectralEmbeddingParams_t* params);
CUVS_EXPORT cuvsError_t cuvsAmdSpectralEmbeddingParamsDestroy(cuvsAmdSpectralEmbeddingParams_t params);

/* dataset fp32 [n, dim], row-major, on the device. rows, cols (int32) and vals (fp32): device vectors of capacity at least
 * 2 n n_neighbors (< 2^31); *nnz receives the number of entries written. Values are 0.5 or 1.0. */
CUVS_EXPORT cuvsError_t cuvsAmdSpectralConnectivityGraph(cuvsResources_t res, cuvsAmdSpectralEmbeddingParams_t params,
                                                         DLManagedTensor* dataset, DLManagedTensor* rows, DLManagedTensor* cols,
                                                         DLManagedTensor* vals, int64_t* nnz);

/* embedding fp32 [n, c_out] on the device, c_out = n_components - (drop_first ? 1 : 0), row-major or column-major (strides
 * (1, n)). Column c is eigenvector c (+ 1 with drop_first) in ascending order of eigenvalue, of unit 2-norm, divided row-wise
 * by sqrt(deg) if norm_laplacian, its entry of largest magnitude positive (lowest index on ties). eigenvalues: fp32
 * [n_components] on the host or the device, or NULL. */
CUVS_EXPORT cuvsError_t cuvsAmdSpectralEmbeddingTransform(cuvsResources_t res, cuvsAmdSpectralEmbeddingParams_t params,
                                                          DLManagedTensor* dataset, DLManagedTensor* embedding,
                                                          DLManagedTensor* eigenvalues);

/* the same from a symmetric COO graph: rows, cols int32 [nnz], vals fp32 [nnz] on the device */
CUVS_EXPORT cuvsError_t cuvsAmdSpectralEmbeddingTransformGraph(cuvsResources_t res, cuvsAmdSpectralEmbeddingParams_t params,
                                                               DLManagedTensor* rows, DLManagedTensor* cols, DLManagedTensor* vals,
                                                               int64_t n, DLManagedTensor* embedding, DLManagedTensor* eigenvalues);

struct cuvsAmdSpectralClusteringParams {
  int n_clusters;   /* 8 */
  int n_components; /* 8: columns of the embedding (normalised Laplacian, nothing dropped) */
  int n_init;       /* 10: k-means++ restarts of the Lloyd fit */
  int n_neighbors;  /* 15 */
  float tolerance;  /* 1e-5: of the eigen-solver */
  uint64_t seed;    /* 0: the eigen-solver's start vector and the k-means seed */
};
typedef struct cuvsAmdSpectralClusteringParams* cuvsAmdSpectralClusteringParams_t;

CUVS_EXPORT cuvsError_t cuvsAmdSpectralClusteringParamsCreate(cuvsAmdSpectralClusteringParams_t* params);
CUVS_EXPORT cuvsError_t cuvsAmdSpectralClusteringParamsDestroy(cuvsAmdSpectralClusteringParams_t params);

/* labels int32 [n] on the device, in [0, n_clusters) */
CUVS_EXPORT cuvsError_t cuvsAmdSpectralClusteringFitPredict(cuvsResources_t res, cuvsAmdSpectralClusteringParams_t params,
                                                            DLManagedTensor* dataset, DLManagedTensor* labels);
CUVS_EXPORT cuvsError_t cuvsAmdSpectralClusteringFitPredictGraph(cuvsResources_t res, cuvsAmdSpectralClusteringParams_t params,
                                                                 DLManagedTensor* rows, DLManagedTensor* cols,
                                                                 DLManagedTensor* vals, int64_t n, DLManagedTensor* labels);

/* The solver on its own: the k smallest eigenpairs of the Laplacian of the graph, ascending. eigenvalues fp32 [k] (host or
 * device), eigenvectors fp32 [k, n] row-major on the device, each of unit 2-norm; no degree scaling and no sign rule.
 * ncv = 0: max(min(n - k, max(2 k + 1, 20)), k + 1); otherwise k < ncv <= min(n, 1024). At most 10 n matrix-vector products:
 * at the cap the last Ritz pairs are returned with CUVS_SUCCESS and cuvsAmdSpectralLastStats reports converged = 0. */
CUVS_EXPORT cuvsError_t cuvsAmdSpectralEigsh(cuvsResources_t res, DLManagedTensor* rows, DLManagedTensor* cols,
                                             DLManagedTensor* vals, int64_t n, bool norm_laplacian, int k, int ncv, float tolerance,
                                             uint64_t seed, DLManagedTensor* eigenvalues, DLManagedTensor* eigenvectors);

/* Test and tuning hooks. One application y = L x of the solver's own operator (x, y fp32 [n] on the device); diag_out (fp32
 * [n] or NULL) receives the degree scaling: sqrt(deg) (1 for an isolated vertex) if norm_laplacian, deg otherwise. */
CUVS_EXPORT cuvsError_t cuvsAmdSpectralLaplacianMatvec(cuvsResources_t res, DLManagedTensor* rows, DLManagedTensor* cols,
                                                       DLManagedTensor* vals, int64_t n, bool norm_laplacian, DLManagedTensor* x,
                                                       DLManagedTensor* y, DLManagedTensor* diag_out);
/* The solver's own re-orthogonalisation: two passes of classical Gram-Schmidt of u (fp32 [n], in place) against the rows of V
 * (fp32 [j, n] row-major, j <= 1024), then u /= ||u||; *norm_out (host, or NULL) receives the norm before the division. */
CUVS_EXPORT cuvsError_t cuvsAmdSpectralOrthogonalize(cuvsResources_t res, DLManagedTensor* V, DLManagedTensor* u, float* norm_out);
/* calling thread's last solve: matrix-vector products, restarts, ncv, converged (0 or 1) */
CUVS_EXPORT cuvsError_t cuvsAmdSpectralLastStats(uint64_t out[4]);

#ifdef __cplusplus
}
#endif
