/* Epsilon neighbourhood: everything within a radius of each query row, by brute force. The reference has this in C++ only
 * (cpp/include/cuvs/neighbors/epsilon_neighborhood.hpp: dense adjacency + degrees; the CSR output protocols are those of
 * ball_cover::eps_nn, cpp/include/cuvs/neighbors/ball_cover.hpp:247-283); these entry points are extensions in the
 * conventions of the cuvs* C layer. Implemented by cuvs_amd/csrc/eps_neighbors.hip; DESIGN.md 3.1t has the arithmetic
 * contract: pair (i, j) is inside when acc <= eps, acc the fp32 chain acc = fmaf(d, d, acc), d = x[i][t] - y[j][t], t ascending.
 */
#pragma once
#include <cuvs/core/c_api.h>
#include <cuvs/core/export.h>
#include <cuvs/distance/distance.h>
#include <dlpack/dlpack.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* x [m, dim], y [n, dim]: fp32 or fp16 (same type), row-major, contiguous, on the device.
 * adj: bool/uint8 [m, n] or NULL. vd: int32 or int64 [m + 1] or NULL. eps: squared radius. metric: L2Unexpanded only.
 * adj bytes are 0 or 1, vd[i] is the degree of row i and vd[m] the number of edges; both are overwritten. */
CUVS_EXPORT cuvsError_t cuvsAmdEpsNeighbors(cuvsResources_t res, DLManagedTensor* x, DLManagedTensor* y, DLManagedTensor* adj,
                                            DLManagedTensor* vd, float eps, cuvsDistanceType metric);

/* indptr int64 [m + 1]; indices int64 [>= nnz] or NULL; distances fp32 like indices or NULL; vd int64 [m + 1] or NULL.
 * max_k == NULL: two calls. indices == NULL fills indptr (indptr[m] = nnz); with indices, indptr is read and the lists are filled.
 * max_k != NULL: one call, at most *max_k ids per row (the first in ascending order), indices holds m * *max_k; on return
 * *max_k is the largest degree found.
 * The column ids of a row are in ascending order; distances are the chain's values of the kept pairs. */
CUVS_EXPORT cuvsError_t cuvsAmdEpsNeighborsCsr(cuvsResources_t res, DLManagedTensor* x, DLManagedTensor* y,
                                               DLManagedTensor* indptr, DLManagedTensor* indices, DLManagedTensor* distances,
                                               DLManagedTensor* vd, float eps, cuvsDistanceType metric, int64_t* max_k);

/* calling thread's last call: pair tiles, slabs, edges, pairs resolved exactly by the screen (0 without it) */
CUVS_EXPORT cuvsError_t cuvsAmdEpsNeighborsLastStats(uint64_t out[4]);

#ifdef __cplusplus
}
#endif
