/*
 * All-neighbours kNN graph of a dataset against itself - drop-in for c/include/cuvs/neighbors/all_neighbors.h
 * (struct layout and entry points of the reference; implementation: cuvs_amd/csrc/all_neighbors.hip).
 * Struct field order and sizes are ABI: callers mutate fields directly.
 */
#pragma once
#include <cuvs/core/c_api.h>
#include <cuvs/core/export.h>
#include <cuvs/distance/distance.h>
#include <cuvs/neighbors/ivf_pq.h>
#include <cuvs/neighbors/nn_descent.h>
#include <dlpack/dlpack.h>
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* builder of the local kNN graphs (the whole dataset when n_clusters == 1, else one cluster at a time) */
typedef enum {
  CUVS_ALL_NEIGHBORS_ALGO_BRUTE_FORCE = 0, /* exact */
  CUVS_ALL_NEIGHBORS_ALGO_IVF_PQ      = 1, /* IVF-PQ search + exact refine; L2Expanded only */
  CUVS_ALL_NEIGHBORS_ALGO_NN_DESCENT  = 2
} cuvsAllNeighborsAlgo;

struct cuvsAllNeighborsIndexParams {
  cuvsAllNeighborsAlgo algo;                    /* BRUTE_FORCE */
  size_t overlap_factor;                        /* 1: clusters every row is assigned to (< n_clusters when batching) */
  size_t n_clusters;                            /* 1: no batching; > 1 needs a host dataset */
  cuvsDistanceType metric;                      /* L2Expanded */
  cuvsIvfPqIndexParams_t ivf_pq_params;         /* NULL: the defaults of the CAGRA-side IVF-PQ graph builder */
  cuvsNNDescentIndexParams_t nn_descent_params; /* NULL: the defaults of cuvsNNDescentIndexParamsCreate */
};
typedef struct cuvsAllNeighborsIndexParams* cuvsAllNeighborsIndexParams_t;

CUVS_EXPORT cuvsError_t cuvsAllNeighborsIndexParamsCreate(cuvsAllNeighborsIndexParams_t* index_params);
/* also destroys the nested parameter structs that are not NULL */
CUVS_EXPORT cuvsError_t cuvsAllNeighborsIndexParamsDestroy(cuvsAllNeighborsIndexParams_t index_params);

/* dataset: fp32 row-major [n, dim], host or device (read from the tensor). indices: int64 [n, k] on the device, k from its
 * shape. distances: fp32 [n, k] on the device or NULL. core_distances: fp32 [n] on the device or NULL; when given, `distances`
 * receives mutual-reachability distances max(core[i], core[j], alpha * d(i, j)) and core_distances the distance to each
 * row's k-th neighbour. A device dataset needs n_clusters == 1. */
CUVS_EXPORT cuvsError_t cuvsAllNeighborsBuild(cuvsResources_t res, cuvsAllNeighborsIndexParams_t params,
                                              DLManagedTensor* dataset, DLManagedTensor* indices,
                                              DLManagedTensor* distances, DLManagedTensor* core_distances, float alpha);

#ifdef __cplusplus
}
#endif
