/* ScaNN search over an index built by cuvsAmdScannBuild (scann.h): coarse search over the AVQ centres, a scan of the PQ codes of
 * both residuals of the probed leaves on the bf16 matrix cores, exact removal of the rows that SOAR placed twice, and an optional
 * re-rank against the index's bf16 rows. The reference has no search; these entry points are extensions in the conventions of the
 * cuvs* C layer. Implemented by cuvs_amd/csrc/scann_search.hip; DESIGN.md 3.1za has the contract of the scores and the kernels.
 *
 * The search-side lists are built by the first search of an index, under a lock of that index: searches of one index from
 * several host threads, each with its own cuvsResources_t, are safe.
 * For an fp32 re-rank against the caller's own rows, hand the returned neighbours to cuvsRefine (cuvs/neighbors/refine.h).
 */
#pragma once
#include <cuvs_amd/scann.h>
#ifdef __cplusplus
extern "C" {
#endif

struct cuvsAmdScannSearchParams {
  uint32_t n_probes;  /* 20: leaves searched per query, clamped to n_leaves */
  uint32_t n_reorder; /* 0: candidates kept for the re-rank against the bf16 rows (<= 4096); 0: no re-rank, the approximate scores */
};
typedef struct cuvsAmdScannSearchParams* cuvsAmdScannSearchParams_t;

CUVS_EXPORT cuvsError_t cuvsAmdScannSearchParamsCreate(cuvsAmdScannSearchParams_t* params);
CUVS_EXPORT cuvsError_t cuvsAmdScannSearchParamsDestroy(cuvsAmdScannSearchParams_t params);

/* queries fp32 [m, dim], neighbors int64 [m, k], distances fp32 [m, k], all on the device, row-major and contiguous.
 * 1 <= k; with a re-rank k <= n_reorder <= 4096, without one k <= 4096. The metric is the one recorded in the index: L2Expanded
 * (squared distances, ascending) or InnerProduct (dot products, descending); ties go to the lower row id. Slots that cannot be
 * filled hold the id INT64_MAX and the distance FLT_MAX, as after cuvsIvfFlatSearch. Any other metric, n_reorder > 0 on an index
 * without reordering_bf16, and mismatched shapes return CUVS_ERROR with a text before anything is launched. */
CUVS_EXPORT cuvsError_t cuvsAmdScannSearch(cuvsResources_t res, cuvsAmdScannSearchParams_t params, cuvsAmdScannIndex_t index,
                                           DLManagedTensor* queries, DLManagedTensor* neighbors, DLManagedTensor* distances);

/* The calling thread's last search: work units scanned, (entry, query) pairs scored, units that read the codebook from global
 * memory instead of LDS, candidates dropped as duplicates (summed over the queries). */
CUVS_EXPORT cuvsError_t cuvsAmdScannSearchLastStats(uint64_t out[4]);

#ifdef __cplusplus
}
#endif
