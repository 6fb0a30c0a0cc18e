/* Exact Hamming k-nearest neighbours and Hamming distance matrices over packed bit codes (the rows cuvsBinaryQuantizer*
 * writes, or any uint8 / int8 rows read as bits). The reference has no brute force for BitwiseHamming; these entry points are
 * extensions in the conventions of the cuvs* C layer. Implemented by cuvs_amd/csrc/binary_knn.hip; DESIGN.md 3.1zc has the
 * design.
 *
 * Arithmetic: hamming(a, b) = popcount(a) + popcount(b) - 2 a.b over the 8 * nbytes bits of a row, a.b on the int8 matrix
 * cores, everything in integers; the fp32 results are exact (8 * nbytes < 2^24). int8 rows are read as bytes.
 */
#pragma once
#include <cuvs/core/c_api.h>
#include <cuvs/core/export.h>
#include <cuvs/neighbors/common.h>
#include <dlpack/dlpack.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* dataset [n, nbytes] and queries [m, nbytes]: uint8 or int8 (both the same), on the device, n < 2^32 - 1, 8 * nbytes < 2^24.
 * The last stride is 1; the row stride may be larger than nbytes (a column slice of a wider buffer). neighbors int64 [m, k]
 * and distances fp32 [m, k], contiguous, on the device: for every query the k rows with the smallest (distance, id), in that
 * order; distances are popcounts. prefilter: NO_FILTER, BITSET (one bit per row) or BITMAP (m x n bits), uint32 words on the
 * device, bit = 1 keeps the row, as in cuvsBruteForceSearch. Slots beyond the rows that exist and pass the filter hold
 * FLT_MAX and id -1. k <= 64 without a filter runs the fused kernel (nothing of size m x n is allocated); any other k and
 * any filter go through fp32 distance tiles and the tiled brute-force selection. Asynchronous on the handle's stream. */
CUVS_EXPORT cuvsError_t cuvsAmdBinaryKnn(cuvsResources_t res, DLManagedTensor* dataset, DLManagedTensor* queries,
                                         DLManagedTensor* neighbors, DLManagedTensor* distances, cuvsFilter prefilter);

/* x [m, nbytes], y [n, nbytes] as above; out fp32 [m, n], contiguous: out[i][j] = hamming(x[i], y[j]). */
CUVS_EXPORT cuvsError_t cuvsAmdBinaryPairwiseDistance(cuvsResources_t res, DLManagedTensor* x, DLManagedTensor* y,
                                                      DLManagedTensor* out);

/* What the calling thread's last call of either kind launched: out[0] column splits of the tile kernel's grid (of its last
 * launch), out[1] 1 when the fused top-k epilogue ran, 0 for the store epilogue, out[2] 64-byte K chunks per row, out[3]
 * K stages (1: the expanded queries stay resident in the LDS; more: they are re-staged that many times per 256 dataset rows). */
CUVS_EXPORT cuvsError_t cuvsAmdBinaryKnnLastStats(cuvsResources_t res, uint64_t out[4]);

#ifdef __cplusplus
}
#endif
