/* Masked L2 nearest neighbour and cross-component nearest neighbours. The reference has these in C++ only
 * (cpp/src/distance/masked_nn.cuh: cuvs::distance::masked_l2_nn; cpp/src/sparse/neighbors/cross_component_nn.cuh); these
 * entry points are extensions in the conventions of the cuvs* C layer. Implemented by cuvs_amd/csrc/masked_nn.hip; DESIGN.md
 * 3.1zb has the contract.
 *
 * Arithmetic: d(i, j) = max(fmaf(-2, dot, xn[i] + yn[j]), 0) with dot the fp32 chain acc = fmaf(x[i][t], y[j][t], acc), t
 * ascending. The minimum is taken over (bits of d, j): ties go to the smaller j, and the result does not depend on the run.
 * NaN inputs are not supported. Nothing of size m x n is allocated.
 */
#pragma once
#include <cuvs/core/c_api.h>
#include <cuvs/core/export.h>
#include <dlpack/dlpack.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* x fp32 [m, dim], y fp32 [n, dim], n < 2^32 - 1: row-major, contiguous, on the device. x_norm fp32 [m], y_norm fp32 [n]:
 * squared norms, either may be NULL (computed here). adj bool / uint8 [m, G]. group_idxs int64 [G] on the device: the END index
 * of every group of rows of y, non-decreasing, the last <= n; empty groups are allowed, rows of y past the last end belong to
 * no group. out_idx int64 [m], out_dist fp32 [m]:
 *   (out_dist[i], out_idx[i]) = min over j with adj[i][group(j)] != 0 of (d(i, j), j); FLT_MAX and -1 when there is no such j.
 * sqrt != 0 writes sqrtf of the minimum (the minimum is taken on the squared value). init_out == 0 reduces into the values
 * out_idx / out_dist hold on entry (distances squared, or their square roots when sqrt != 0): two calls over complementary
 * masks equal one call. Tiles of 128 x 128 pairs whose groups are all switched off for all their rows are not computed. */
CUVS_EXPORT cuvsError_t cuvsAmdMaskedL2NN(cuvsResources_t res, DLManagedTensor* x, DLManagedTensor* y, DLManagedTensor* x_norm,
                                          DLManagedTensor* y_norm, DLManagedTensor* adj, DLManagedTensor* group_idxs, int sqrt,
                                          int init_out, DLManagedTensor* out_idx, DLManagedTensor* out_dist);

/* x fp32 [n, dim], n < 2^31. colors int32 [n], values in [0, n_components), in any order. row_nn_idx int64 [n] and row_nn_dist
 * fp32 [n] (each may be NULL): for every row i the nearest row j of another colour, ties to the smaller j. edge_src, edge_dst
 * int64 [n_components], edge_weight fp32 [n_components]: for every colour c the edge (i, j, w) with the smallest (w, i, j) over
 * i of colour c and j of another colour. Ids are the caller's row ids. -1, -1, FLT_MAX stand for "none" (a colour without
 * rows, a single colour). sqrt as above. */
CUVS_EXPORT cuvsError_t cuvsAmdCrossComponentNN(cuvsResources_t res, DLManagedTensor* x, DLManagedTensor* colors,
                                                int64_t n_components, int sqrt, DLManagedTensor* row_nn_idx,
                                                DLManagedTensor* row_nn_dist, DLManagedTensor* edge_src, DLManagedTensor* edge_dst,
                                                DLManagedTensor* edge_weight);

/* the last call of either kind on this handle by the calling thread: 128 x 128 pair tiles of the problem, and those computed.
 * Waits for the handle's stream. */
CUVS_EXPORT cuvsError_t cuvsAmdMaskedNNLastStats(cuvsResources_t res, uint64_t out[2]);

#ifdef __cplusplus
}
#endif
