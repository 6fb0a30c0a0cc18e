/*
 * HNSW: a CAGRA graph handed over to host search — drop-in for c/include/cuvs/neighbors/hnsw.h. Struct field order, types and
 * the argument lists are ABI. The conversion runs on the device (cuvs_amd/csrc/hnsw.hip); the index itself, its search, its
 * insert and its files are host code (cuvs_amd/csrc/hnsw_host.hpp) written against the published algorithm and hnswlib's
 * saveIndex layout; hnswlib itself is not used. The exact rules are in DESIGN.md 3.1r and restated in tests/hnsw_ref.py.
 *
 * Search, insert and the level of a row are deterministic: every comparison is on the pair (distance, id), the level of row i
 * is a fixed integer hash of i, the insert runs sequentially in id order (num_threads of the index and extend params is
 * accepted and unused). A search gives the same answer at every thread count.
 *
 * cuvsHnswDeserialize, cuvsHnswSearch, cuvsHnswExtend, cuvsHnswSerialize and the Create / Destroy functions never touch the
 * device nor `res`: they work on a machine without a GPU.
 *
 * The enumerators NONE, CPU and GPU are unscoped, as in the reference.
 */
#pragma once
#include <cuvs/core/c_api.h>
#include <cuvs/core/export.h>
#include <cuvs/distance/distance.h>
#include <cuvs/neighbors/cagra.h>
#include <dlpack/dlpack.h>
#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

enum cuvsHnswHierarchy {
  NONE = 0, /* base layer only: level 0 is the CAGRA graph, a search starts from 32 fixed seeds; immutable */
  CPU  = 1, /* upper levels by sequential insertion on the host */
  GPU  = 2  /* upper levels by exact / IVF-PQ kNN among the rows of each level, on the device */
};

/* ACE build parameters. Partitioning is a memory strategy, not a result contract: the fields are accepted and, apart from
 * use_disk / build_dir, unused (as cuvsCagraBuild treats build_algo == ACE). */
struct cuvsHnswAceParams {
  size_t npartitions;        /* 0 */
  const char* build_dir;     /* "/tmp/hnsw_ace_build": with use_disk, cuvsHnswBuild also writes <build_dir>/hnsw_index.bin */
  bool use_disk;             /* false */
  double max_host_memory_gb; /* 0 */
  double max_gpu_memory_gb;  /* 0 */
};
typedef struct cuvsHnswAceParams* cuvsHnswAceParams_t;
CUVS_EXPORT cuvsError_t cuvsHnswAceParamsCreate(cuvsHnswAceParams_t* params);
CUVS_EXPORT cuvsError_t cuvsHnswAceParamsDestroy(cuvsHnswAceParams_t params);

struct cuvsHnswIndexParams {
  enum cuvsHnswHierarchy hierarchy; /* GPU */
  int ef_construction;              /* 200: candidate list of an insert (CPU hierarchy, extend) */
  int num_threads;                  /* 0: accepted, unused (the insert is sequential) */
  size_t M;                         /* 32: cuvsHnswBuild only; graph_degree = 2 M, intermediate_graph_degree = 3 M */
  cuvsDistanceType metric;          /* L2Expanded: cuvsHnswBuild only; L2Expanded or InnerProduct */
  cuvsHnswAceParams_t ace_params;   /* NULL; cuvsHnswBuild requires it */
};
typedef struct cuvsHnswIndexParams* cuvsHnswIndexParams_t;
CUVS_EXPORT cuvsError_t cuvsHnswIndexParamsCreate(cuvsHnswIndexParams_t* params);
CUVS_EXPORT cuvsError_t cuvsHnswIndexParamsDestroy(cuvsHnswIndexParams_t params);

typedef struct {
  uintptr_t addr;   /* the index in host memory, 0 before it is made */
  DLDataType dtype; /* element type of the rows: float32, float16, int8 or uint8 */
} cuvsHnswIndex;
typedef cuvsHnswIndex* cuvsHnswIndex_t;
CUVS_EXPORT cuvsError_t cuvsHnswIndexCreate(cuvsHnswIndex_t* index);
CUVS_EXPORT cuvsError_t cuvsHnswIndexDestroy(cuvsHnswIndex_t index);

struct cuvsHnswExtendParams {
  int num_threads; /* 0: accepted, unused */
};
typedef struct cuvsHnswExtendParams* cuvsHnswExtendParams_t;
CUVS_EXPORT cuvsError_t cuvsHnswExtendParamsCreate(cuvsHnswExtendParams_t* params);
CUVS_EXPORT cuvsError_t cuvsHnswExtendParamsDestroy(cuvsHnswExtendParams_t params);

/* Level 0 of the HNSW index is the CAGRA graph. A VPQ-compressed CAGRA index needs the WithDataset form; BitwiseHamming,
 * cosine and sqrt-L2 indexes are refused. dataset_tensor: host or device rows of the index's shape and dtype. */
CUVS_EXPORT cuvsError_t cuvsHnswFromCagra(cuvsResources_t res,
                                          cuvsHnswIndexParams_t params,
                                          cuvsCagraIndex_t cagra_index,
                                          cuvsHnswIndex_t hnsw_index);
CUVS_EXPORT cuvsError_t cuvsHnswFromCagraWithDataset(cuvsResources_t res,
                                                     cuvsHnswIndexParams_t params,
                                                     cuvsCagraIndex_t cagra_index,
                                                     cuvsHnswIndex_t hnsw_index,
                                                     DLManagedTensor* dataset_tensor);

/* CAGRA build (graph_degree 2 M, intermediate 3 M, params->metric) followed by the conversion with params->hierarchy. */
CUVS_EXPORT cuvsError_t cuvsHnswBuild(cuvsResources_t res,
                                      cuvsHnswIndexParams_t params,
                                      DLManagedTensor* dataset,
                                      cuvsHnswIndex_t index);

/* Appends host rows of the index's dtype; refused for a NONE index. Exclusive: no search may run on the index meanwhile. */
CUVS_EXPORT cuvsError_t cuvsHnswExtend(cuvsResources_t res,
                                       cuvsHnswExtendParams_t params,
                                       DLManagedTensor* additional_dataset,
                                       cuvsHnswIndex_t index);

struct cuvsHnswSearchParams {
  int32_t ef;          /* 200: candidate list of a search (at least k is used) */
  int32_t num_threads; /* 0: OMP_NUM_THREADS if set, else the hardware concurrency */
};
typedef struct cuvsHnswSearchParams* cuvsHnswSearchParams_t;
CUVS_EXPORT cuvsError_t cuvsHnswSearchParamsCreate(cuvsHnswSearchParams_t* params);
CUVS_EXPORT cuvsError_t cuvsHnswSearchParamsDestroy(cuvsHnswSearchParams_t params);

/* queries [m, dim] of the index's dtype, neighbors uint64 [m, k], distances float32 [m, k], all in host memory. Slots past
 * the rows a walk can reach hold id UINT64_MAX and distance FLT_MAX. Concurrent searches of one index are safe. */
CUVS_EXPORT cuvsError_t cuvsHnswSearch(cuvsResources_t res,
                                       cuvsHnswSearchParams_t params,
                                       cuvsHnswIndex_t index,
                                       DLManagedTensor* queries,
                                       DLManagedTensor* neighbors,
                                       DLManagedTensor* distances);

/* hnswlib's saveIndex layout. A NONE index gives the bytes of cuvsCagraSerializeToHnswlib. */
CUVS_EXPORT cuvsError_t cuvsHnswSerialize(cuvsResources_t res, const char* filename, cuvsHnswIndex_t index);

/* index->dtype says what the rows are and is set by the caller beforehand; params->hierarchy says how the file is searched
 * (NONE: the file of cuvsCagraSerializeToHnswlib). The file is untrusted: whatever does not fit is refused with text. */
CUVS_EXPORT cuvsError_t cuvsHnswDeserialize(cuvsResources_t res,
                                            cuvsHnswIndexParams_t params,
                                            const char* filename,
                                            int dim,
                                            cuvsDistanceType metric,
                                            cuvsHnswIndex_t index);
#ifdef __cplusplus
}
#endif
