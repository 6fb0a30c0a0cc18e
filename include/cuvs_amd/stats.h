/* cuvs::stats: silhouette score and trustworthiness on the device. The reference has these in C++ only
 * (cpp/include/cuvs/stats/silhouette_score.hpp, trustworthiness_score.hpp); these entry points are extensions in the
 * conventions of the cuvs* C layer. Implemented by cuvs_amd/csrc/stats.hip; DESIGN.md 3.1y has the contract.
 *
 * Distances are exact fp32 chains on the vector pipe, t ascending, one accumulator per pair, every operation rounded once:
 *   the four L2 ids   acc = fmaf(x[i][t] - x[j][t], x[i][t] - x[j][t], acc); the Sqrt ids take sqrtf(acc). L2Expanded and
 *                     L2SqrtExpanded deliberately share this unexpanded arithmetic: a score built on the cancellation of
 *                     |x|^2 + |y|^2 - 2 x.y is worth less.
 *   L1                acc = acc + fabsf(x[i][t] - x[j][t])   (admitted by the silhouette score only)
 *   CosineExpanded    1.0f - dot / (sqrtf(nx) * sqrtf(ny)), dot, nx, ny fma chains; a zero-norm row gives NaN for its pairs.
 * Nothing of size n x n is allocated, no floating-point atomics are used, and results do not depend on the run.
 *
 * Out of scope: fp64 and fp16 inputs, host-resident inputs, int64 labels, n_neighbors > 64, other metrics, a matrix-core
 * screen, the reference's fp64 overloads.
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

/* X fp32 [n, dim] row-major, contiguous, on the device, n < 2^31. labels int32 [n] on the device, values in [0, n_labels),
 * 2 <= n_labels <= n - 1. scores fp32 [n] on the device or NULL. batch_rows caps the rows processed at a time (<= 0: the
 * library chooses from the handle's workspace limit); the result is bit-identical for every batch_rows.
 * With S[i][c] the fp64 sum of d(i, j) over j != i of label c and cnt[c] the label counts, all in fp64:
 *   a_i = S[i][c_i] / (cnt[c_i] - 1), b_i = min over c != c_i with cnt[c] > 0 of S[i][c] / cnt[c],
 *   s_i = 0 when cnt[c_i] == 1 or a_i == b_i (or no other label has a row), else (b_i - a_i) / max(a_i, b_i).
 * scores[i] = (float)s_i (overwritten whatever it held); *mean = the fp64 sum of s_i in index order, divided by n. */
CUVS_EXPORT cuvsError_t cuvsAmdSilhouetteScore(cuvsResources_t res, DLManagedTensor* X, DLManagedTensor* labels,
                                               int64_t n_labels, cuvsDistanceType metric, int64_t batch_rows,
                                               DLManagedTensor* scores, double* mean);

/* X as above; neighbors int64 [n, k], 1 <= k <= 64, every id in [0, n) and different from its row; ranks int32 [n, k] or
 * NULL. With v(i, l) the squared-L2 chain between rows i and l of X and j = neighbors[i][q]:
 *   ranks[i][q] = 1 + #{ l : l != i, l != j, (v(i, l), l) < (v(i, j), j) lexicographically }
 * (the 1-based rank among the other rows, ties to the smaller index); *penalty_sum = sum of max(0, ranks[i][q] - k). */
CUVS_EXPORT cuvsError_t cuvsAmdNeighborRanks(cuvsResources_t res, DLManagedTensor* X, DLManagedTensor* neighbors,
                                             DLManagedTensor* ranks, uint64_t* penalty_sum);

/* X fp32 [n, dim], X_embedded fp32 [n, dim_e]; 1 <= n_neighbors <= 64 and n_neighbors < n / 2 (sklearn's rule). metric: one of
 * the four L2 ids; the ranks are always taken on the squared chain (sqrtf is monotone and can only create ties).
 * The n_neighbors nearest other rows of X_embedded come from the brute-force search at k = n_neighbors + 1 (the entry whose id
 * is the row's own is dropped if present, else the last); t = the penalty sum of cuvsAmdNeighborRanks on X;
 * *score = 1.0 - ((2.0 / ((double(n) * k) * ((2.0 * n) - (3.0 * k) - 1.0))) * t). */
CUVS_EXPORT cuvsError_t cuvsAmdTrustworthinessScore(cuvsResources_t res, DLManagedTensor* X, DLManagedTensor* X_embedded,
                                                    int64_t n_neighbors, cuvsDistanceType metric, double* score);

/* calling thread's last call: pair tiles, slabs, straddling tiles (silhouette) or pairs past the screen (ranks), 0 */
CUVS_EXPORT cuvsError_t cuvsAmdStatsLastStats(uint64_t out[4]);

#ifdef __cplusplus
}
#endif
