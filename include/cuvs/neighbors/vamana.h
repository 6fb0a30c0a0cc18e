/*
 * Vamana (DiskANN) graph build on the device and DiskANN file output — drop-in for c/include/cuvs/neighbors/vamana.h.
 * Struct field order, types and the argument lists are ABI. Implemented by cuvs_amd/csrc/vamana.hip; the exact rules of
 * the search, the prune and the batch schedule are in DESIGN.md 3.1p and restated in tests/vamana_ref.py.
 *
 * The build is deterministic: the insert order is a fixed permutation, the medoid is the row nearest to the column mean
 * (lowest id on a tie), and every comparison uses the total order (distance, id). Two builds of the same rows give the
 * same bits. The index holds the graph as uint32 [n, graph_degree] (unused slots 0xFFFFFFFF, behind the used ones), the
 * medoid and a device copy of the rows; it can be written out but not searched (the files are read by DiskANN).
 * The graph itself is read back with cuvsAmdVamanaIndexGetGraph (<cuvs_amd/extensions.h>).
 */
#pragma once
#include <cuvs/core/c_api.h>
#include <cuvs/core/export.h>
#include <cuvs/distance/distance.h>
#include <cuvs/neighbors/common.h>
#include <dlpack/dlpack.h>
#include <stdbool.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

struct cuvsVamanaIndexParams {
  cuvsDistanceType metric;    /* L2Expanded: the only metric */
  uint32_t graph_degree;      /* 32: most edges per node (R); one of 32, 64, 128, 256 */
  uint32_t visited_size;      /* 64: nodes a search keeps and expands at most (L); > graph_degree, <= 1024; a value that is
                                 no power of two is rounded up by doubling from graph_degree */
  float vamana_iters;         /* 1: times the rows are inserted; the fraction is a partial second pass; >= 1 */
  float alpha;                /* 1.2: the prune's last occlusion factor */
  float max_fraction;         /* 0.06: the largest insert batch as a fraction of the rows (above 1: 1; at least one row) */
  float batch_base;           /* 2: growth of the batch size from one batch to the next */
  uint32_t queue_size;        /* 127: most pending (seen, not yet expanded) nodes of a search */
  uint32_t reverse_batchsize; /* 1000000: destinations per launch of the reverse-edge prune */
};
typedef struct cuvsVamanaIndexParams* cuvsVamanaIndexParams_t;
CUVS_EXPORT cuvsError_t cuvsVamanaIndexParamsCreate(cuvsVamanaIndexParams_t* params);
CUVS_EXPORT cuvsError_t cuvsVamanaIndexParamsDestroy(cuvsVamanaIndexParams_t params);

typedef struct {
  uintptr_t addr;   /* the built index, 0 before cuvsVamanaBuild */
  DLDataType dtype; /* element type of the rows it was built from */
} cuvsVamanaIndex;
typedef cuvsVamanaIndex* cuvsVamanaIndex_t;
CUVS_EXPORT cuvsError_t cuvsVamanaIndexCreate(cuvsVamanaIndex_t* index);
CUVS_EXPORT cuvsError_t cuvsVamanaIndexDestroy(cuvsVamanaIndex_t index);
CUVS_EXPORT cuvsError_t cuvsVamanaIndexGetDims(cuvsVamanaIndex_t index, int* dim);

/* dataset: row-major [n, dim] of float32, int8 or uint8, on the device or on the host (copied to the device once).
 * Parameters and dtype are checked before the device is touched. */
CUVS_EXPORT cuvsError_t cuvsVamanaBuild(cuvsResources_t res,
                                        cuvsVamanaIndexParams_t params,
                                        DLManagedTensor* dataset,
                                        cuvsVamanaIndex_t index);

/* The graph file of the open-source DiskANN: uint64 file size, uint32 largest degree, uint32 medoid, uint64 0, then per node
 * a uint32 count and that many uint32 ids. With include_dataset also `<filename>.data`: int32 n, int32 dim, the rows. */
CUVS_EXPORT cuvsError_t cuvsVamanaSerialize(cuvsResources_t res,
                                            const char* filename,
                                            cuvsVamanaIndex_t index,
                                            bool include_dataset);
#ifdef __cplusplus
}
#endif
