/* Single-linkage agglomerative clustering: minimum spanning tree, dendrogram, flat labels. The reference has this in C++ only
 * (cpp/include/cuvs/cluster/agglomerative.hpp: single_linkage, helpers::build_linkage, helpers::build_dendrogram); these entry
 * points are extensions in the conventions of the cuvs* C layer. Implemented by cuvs_amd/csrc/single_linkage.hip; DESIGN.md
 * 3.1v has the contract: the base distance is the fp32 chain acc = fmaf(d, d, acc), d = x[i][t] - x[j][t], t ascending (its
 * correctly rounded square root for the Sqrt metrics), edges are ordered by (bits of the weight, min(i, j), max(i, j)), and
 * the tree is the unique minimum spanning tree under that order.
 */
#pragma once
#include <cuvs/core/c_api.h>
#include <cuvs/core/export.h>
#include <cuvs/distance/distance.h>
#include <cuvs/neighbors/all_neighbors.h>
#include <dlpack/dlpack.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  CUVS_AMD_LINKAGE_PAIRWISE  = 0, /* the exact tree of the complete graph (no n x n memory) */
  CUVS_AMD_LINKAGE_KNN_GRAPH = 1  /* the forest of a kNN graph, its components joined over the complete graph */
} cuvsAmdLinkage;

typedef enum {
  CUVS_AMD_LINKAGE_SPACE_DISTANCE            = 0, /* w(i, j) = d(i, j) */
  CUVS_AMD_LINKAGE_SPACE_MUTUAL_REACHABILITY = 1  /* w(i, j) = max(core[i], core[j], alpha * d(i, j)) */
} cuvsAmdLinkageSpace;

struct cuvsAmdLinkageParams {
  cuvsAmdLinkageSpace space; /* DISTANCE */
  int c;                     /* 15: distance space, KNN_GRAPH: k = min(n, max(2, floor(log2 n) + c)) */
  cuvsAmdLinkage linkage;    /* KNN_GRAPH; distance space only (mutual reachability always starts from the kNN graph) */
  int min_samples;           /* 5: mutual reachability: k of the kNN graph and of the core distances, in [2, n] */
  float alpha;               /* 1.0: mutual reachability: the factor of d(i, j) */
  /* mutual reachability: how cuvsAllNeighborsBuild makes the kNN graph; NULL: brute force. Its metric is overridden by
   * the call's. Borrowed: cuvsAmdLinkageParamsDestroy leaves it alone. */
  cuvsAllNeighborsIndexParams_t all_neighbors_params;
};
typedef struct cuvsAmdLinkageParams* cuvsAmdLinkageParams_t;

CUVS_EXPORT cuvsError_t cuvsAmdLinkageParamsCreate(cuvsAmdLinkageParams_t* params);
CUVS_EXPORT cuvsError_t cuvsAmdLinkageParamsDestroy(cuvsAmdLinkageParams_t params);

/* X fp32 [n, dim], row-major, contiguous, on the device, 2 <= n < 2^30. dendrogram [n - 1, 2] and labels [n]: int32 or int64 (the
 * same type) on the device. metric: L2Expanded, L2SqrtExpanded, L2Unexpanded or L2SqrtUnexpanded. n_clusters in [1, n].
 * c is read with KNN_GRAPH only. Distance space. */
CUVS_EXPORT cuvsError_t cuvsAmdSingleLinkage(cuvsResources_t res, DLManagedTensor* X, DLManagedTensor* dendrogram,
                                             DLManagedTensor* labels, cuvsDistanceType metric, int64_t n_clusters,
                                             cuvsAmdLinkage linkage, int c);

/* mst_src, mst_dst (int32 or int64) and mst_weights (fp32), each [n - 1]: the tree's edges in ascending order of
 * (bits(w), src, dst), src < dst. dendrogram [n - 1, 2], out_distances fp32 [n - 1], out_sizes [n - 1]: the merges of those
 * edges in that order (the children of merge e, its height and the size of the new node n + e). The index tensors have one
 * type. core_dists fp32 [n]: required and written in mutual-reachability space, NULL otherwise. Any other output may be NULL. */
CUVS_EXPORT cuvsError_t cuvsAmdBuildLinkage(cuvsResources_t res, DLManagedTensor* X, cuvsAmdLinkageParams_t params,
                                            cuvsDistanceType metric, DLManagedTensor* mst_src, DLManagedTensor* mst_dst,
                                            DLManagedTensor* mst_weights, DLManagedTensor* dendrogram,
                                            DLManagedTensor* out_distances, DLManagedTensor* out_sizes,
                                            DLManagedTensor* core_dists);

/* rows, cols (int32 or int64) and data (fp32), each [n - 1] on the device: the edges of a spanning tree in merge order.
 * children [n - 1, 2], out_delta fp32 [n - 1], out_size [n - 1] as above. */
CUVS_EXPORT cuvsError_t cuvsAmdBuildDendrogram(cuvsResources_t res, DLManagedTensor* rows, DLManagedTensor* cols,
                                               DLManagedTensor* data, DLManagedTensor* children, DLManagedTensor* out_delta,
                                               DLManagedTensor* out_size);

/* calling thread's last linkage: k of the kNN graph (0: PAIRWISE), undirected graph edges after symmetrising, sparse rounds that
 * joined components, components after the sparse phase, dense rounds, pair tiles evaluated */
CUVS_EXPORT cuvsError_t cuvsAmdSingleLinkageLastStats(uint64_t out[6]);

#ifdef __cplusplus
}
#endif
