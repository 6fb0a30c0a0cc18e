/*
 * IVF-SQ entry points — drop-in for c/include/cuvs/neighbors/ivf_sq.h.
 * Struct field order and sizes are ABI: callers mutate fields directly.
 * Implemented by cuvs_amd/csrc/ivf_sq.hip.
 */
#pragma once
#include <cuvs/core/c_api.h>
#include <cuvs/distance/distance.h>
#include <cuvs/neighbors/common.h>
#include <dlpack/dlpack.h>
#include <stdbool.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

struct cuvsIvfSqIndexParams {
  cuvsDistanceType metric;              /* default L2Expanded; also L2SqrtExpanded, InnerProduct, CosineExpanded */
  float metric_arg;                     /* 2.0 */
  bool add_data_on_build;               /* true */
  uint32_t n_lists;                     /* 1024 */
  uint32_t kmeans_n_iters;              /* 20 */
  uint32_t max_train_points_per_cluster; /* 256: the k-means sample holds at most n_lists * this many rows */
  bool conservative_memory_allocation;  /* false */
};
typedef struct cuvsIvfSqIndexParams* cuvsIvfSqIndexParams_t;
CUVS_EXPORT cuvsError_t cuvsIvfSqIndexParamsCreate(cuvsIvfSqIndexParams_t* index_params);
CUVS_EXPORT cuvsError_t cuvsIvfSqIndexParamsDestroy(cuvsIvfSqIndexParams_t index_params);

struct cuvsIvfSqSearchParams {
  uint32_t n_probes; /* 20 */
};
typedef struct cuvsIvfSqSearchParams* cuvsIvfSqSearchParams_t;
CUVS_EXPORT cuvsError_t cuvsIvfSqSearchParamsCreate(cuvsIvfSqSearchParams_t* params);
CUVS_EXPORT cuvsError_t cuvsIvfSqSearchParamsDestroy(cuvsIvfSqSearchParams_t params);

typedef struct {
  uintptr_t addr;
  DLDataType dtype;
} cuvsIvfSqIndex;
typedef cuvsIvfSqIndex* cuvsIvfSqIndex_t;
CUVS_EXPORT cuvsError_t cuvsIvfSqIndexCreate(cuvsIvfSqIndex_t* index);
CUVS_EXPORT cuvsError_t cuvsIvfSqIndexDestroy(cuvsIvfSqIndex_t index);

CUVS_EXPORT cuvsError_t cuvsIvfSqIndexGetNLists(cuvsIvfSqIndex_t index, int64_t* n_lists);
CUVS_EXPORT cuvsError_t cuvsIvfSqIndexGetDim(cuvsIvfSqIndex_t index, int64_t* dim);
CUVS_EXPORT cuvsError_t cuvsIvfSqIndexGetSize(cuvsIvfSqIndex_t index, int64_t* size);
CUVS_EXPORT cuvsError_t cuvsIvfSqIndexGetCenters(cuvsIvfSqIndex_t index, DLManagedTensor* centers);

/* dataset host or device, fp32/fp16, row-major [n, dim] */
CUVS_EXPORT cuvsError_t cuvsIvfSqBuild(cuvsResources_t res,
                                       cuvsIvfSqIndexParams_t index_params,
                                       DLManagedTensor* dataset,
                                       cuvsIvfSqIndex_t index);

/* queries fp32/fp16 [m, dim], neighbors int64 [m, k], distances fp32 [m, k], filter NO_FILTER or BITSET */
CUVS_EXPORT cuvsError_t cuvsIvfSqSearch(cuvsResources_t res,
                                        cuvsIvfSqSearchParams_t search_params,
                                        cuvsIvfSqIndex_t index,
                                        DLManagedTensor* queries,
                                        DLManagedTensor* neighbors,
                                        DLManagedTensor* distances,
                                        cuvsFilter filter);

CUVS_EXPORT cuvsError_t cuvsIvfSqSerialize(cuvsResources_t res, const char* filename, cuvsIvfSqIndex_t index);
CUVS_EXPORT cuvsError_t cuvsIvfSqDeserialize(cuvsResources_t res, const char* filename, cuvsIvfSqIndex_t index);
/* new_indices may be NULL only while the index is empty (ids continue from the current size) */
CUVS_EXPORT cuvsError_t cuvsIvfSqExtend(cuvsResources_t res,
                                        DLManagedTensor* new_vectors,
                                        DLManagedTensor* new_indices,
                                        cuvsIvfSqIndex_t index);
#ifdef __cplusplus
}
#endif
