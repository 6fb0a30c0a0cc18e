/*
 * Tiered index entry points — drop-in for c/include/cuvs/neighbors/tiered_index.h (enum values, the index struct and
 * the params struct are ABI). Rows [0, ann_rows) are served by an ANN index (CAGRA, IVF-Flat or IVF-PQ), rows
 * [ann_rows, size) by an exact brute-force tail; a search merges the two. Implemented by cuvs_amd/csrc/tiered_index.hip;
 * semantics in DESIGN.md 3.1n.
 */
#pragma once
#include <cuvs/core/c_api.h>
#include <cuvs/core/export.h>
#include <cuvs/distance/distance.h>
#include <cuvs/neighbors/cagra.h>
#include <cuvs/neighbors/common.h>
#include <cuvs/neighbors/ivf_flat.h>
#include <cuvs/neighbors/ivf_pq.h>
#include <dlpack/dlpack.h>
#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  CUVS_TIERED_INDEX_ALGO_CAGRA    = 0,
  CUVS_TIERED_INDEX_ALGO_IVF_FLAT = 1,
  CUVS_TIERED_INDEX_ALGO_IVF_PQ   = 2
} cuvsTieredIndexANNAlgo;

typedef struct {
  uintptr_t addr;
  DLDataType dtype;
  cuvsTieredIndexANNAlgo algo;
} cuvsTieredIndex;
typedef cuvsTieredIndex* cuvsTieredIndex_t;
CUVS_EXPORT cuvsError_t cuvsTieredIndexCreate(cuvsTieredIndex_t* index);
CUVS_EXPORT cuvsError_t cuvsTieredIndexDestroy(cuvsTieredIndex_t index);

struct cuvsTieredIndexParams {
  cuvsDistanceType metric;                  /* L2Expanded */
  cuvsTieredIndexANNAlgo algo;              /* CAGRA */
  int64_t min_ann_rows;                     /* 100000: an ANN tier is built over more rows than this */
  bool create_ann_index_on_extend;          /* false: true rebuilds the ANN tier when the tail outgrows min_ann_rows */
  cuvsCagraIndexParams_t cagra_params;      /* NULL = that algo's defaults (each of the three) */
  cuvsIvfFlatIndexParams_t ivf_flat_params;
  cuvsIvfPqIndexParams_t ivf_pq_params;
};
typedef struct cuvsTieredIndexParams* cuvsTieredIndexParams_t;
CUVS_EXPORT cuvsError_t cuvsTieredIndexParamsCreate(cuvsTieredIndexParams_t* index_params);
CUVS_EXPORT cuvsError_t cuvsTieredIndexParamsDestroy(cuvsTieredIndexParams_t index_params);

/* dataset: fp32 [n, dim], host or device */
CUVS_EXPORT cuvsError_t cuvsTieredIndexBuild(cuvsResources_t res,
                                             cuvsTieredIndexParams_t index_params,
                                             DLManagedTensor* dataset,
                                             cuvsTieredIndex_t index);
/* search_params: cuvsCagraSearchParams_t / cuvsIvfFlatSearchParams_t / cuvsIvfPqSearchParams_t by index->algo, NULL =
 * defaults. queries fp32 [m, dim], neighbors int64 [m, k], distances fp32 [m, k], all on the device; prefilter NO_FILTER
 * or BITSET over the `size` global ids (1 keeps the row). */
CUVS_EXPORT cuvsError_t cuvsTieredIndexSearch(cuvsResources_t res,
                                              void* search_params,
                                              cuvsTieredIndex_t index,
                                              DLManagedTensor* queries,
                                              DLManagedTensor* neighbors,
                                              DLManagedTensor* distances,
                                              cuvsFilter prefilter);
/* new_vectors: fp32 [n_new, dim], host or device; appended behind the rows already held */
CUVS_EXPORT cuvsError_t cuvsTieredIndexExtend(cuvsResources_t res,
                                              DLManagedTensor* new_vectors,
                                              cuvsTieredIndex_t index);
/* rows of indices[0], indices[1], ... in that order; the ANN tier of indices[0] is kept */
CUVS_EXPORT cuvsError_t cuvsTieredIndexMerge(cuvsResources_t res,
                                             cuvsTieredIndexParams_t index_params,
                                             cuvsTieredIndex_t* indices,
                                             size_t num_indices,
                                             cuvsTieredIndex_t output_index);
#ifdef __cplusplus
}
#endif
