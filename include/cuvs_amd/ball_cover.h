/* Random ball cover: a landmark index over low-dimensional points, exact k-NN and eps_nn through it by the triangle
 * inequality. The reference has this in C++ only (cpp/include/cuvs/neighbors/ball_cover.hpp: build, knn_query,
 * all_knn_query, eps_nn); these entry points are extensions in the conventions of eps_neighbors.h and ivf_rabitq.h.
 * Implemented by cuvs_amd/csrc/ball_cover.hip; DESIGN.md 3.1u has the contract: distances, the landmark draw, the list
 * order, the visit expression and its margin. Inputs are assumed finite (no NaN, no infinity); Haversine rows are
 * (latitude, longitude) in radians with latitudes inside (-pi/2, pi/2). The equality with brute force further assumes
 * that no squared coordinate difference, and no sum of them, underflows to a subnormal or overflows: every non-zero
 * |a[t] - b[t]| between two rows, queries or landmarks lies in about [2^-62, 2^61] (the margin's relative error bound
 * does not hold for subnormal squares). eps_nn computes fp32(eps * eps) literally: where it overflows to infinity every
 * pair is inside, where it underflows to 0 only pairs at distance exactly 0 are.
 */
#pragma once
#include <cuvs/core/c_api.h>
#include <cuvs/core/export.h>
#include <cuvs/distance/distance.h>
#include <dlpack/dlpack.h>
#include <stdbool.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

struct cuvsAmdBallCoverIndexParams {
  cuvsDistanceType metric; /* L2SqrtExpanded (default), L2SqrtUnexpanded (the same arithmetic) or Haversine */
  uint32_t n_landmarks;    /* 0: floor(sqrt(m)) */
  uint32_t seed;           /* 0; the landmarks are a fixed function of (m, n_landmarks, seed) */
};
typedef struct cuvsAmdBallCoverIndexParams* cuvsAmdBallCoverIndexParams_t;
CUVS_EXPORT cuvsError_t cuvsAmdBallCoverIndexParamsCreate(cuvsAmdBallCoverIndexParams_t* params);
CUVS_EXPORT cuvsError_t cuvsAmdBallCoverIndexParamsDestroy(cuvsAmdBallCoverIndexParams_t params);

typedef struct {
  uintptr_t addr;
  DLDataType dtype;
} cuvsAmdBallCoverIndex;
typedef cuvsAmdBallCoverIndex* cuvsAmdBallCoverIndex_t;
CUVS_EXPORT cuvsError_t cuvsAmdBallCoverIndexCreate(cuvsAmdBallCoverIndex_t* index);
CUVS_EXPORT cuvsError_t cuvsAmdBallCoverIndexDestroy(cuvsAmdBallCoverIndex_t index);

/* dataset fp32 [m, dim], row-major, on the device, 1 <= m < 2^32; L2: 1 <= dim <= 32, Haversine: dim == 2. The index keeps
 * its own reordered copy of the rows: the caller's buffer need not outlive the call (the reference keeps a view). */
CUVS_EXPORT cuvsError_t cuvsAmdBallCoverBuild(cuvsResources_t res, cuvsAmdBallCoverIndexParams_t params,
                                              DLManagedTensor* dataset, cuvsAmdBallCoverIndex_t index);

/* queries fp32 [q, dim] on the device, neighbors int64 [q, k], distances fp32 [q, k]; 1 <= k <= 256, k <= n_landmarks; dim 2
 * or 3 (L2), 2 (Haversine). Rows are sorted by (distance, id). perform_post_filtering == false: the rows of the k nearest
 * landmarks only (missing slots hold INT64_MAX / FLT_MAX). With post-filtering and weight == 1 the result is that of
 * brute force under (distance, id), ids and distance bits; weight < 1 shrinks the distance to a landmark's ball in the
 * visit decision and is approximate. */
CUVS_EXPORT cuvsError_t cuvsAmdBallCoverKnnQuery(cuvsResources_t res, cuvsAmdBallCoverIndex_t index, DLManagedTensor* queries,
                                                 DLManagedTensor* neighbors, DLManagedTensor* distances,
                                                 bool perform_post_filtering, float weight);
/* build + a query of the dataset against itself (the self match is an ordinary candidate). index_out may be NULL; otherwise
 * it is a created index that receives the built one. */
CUVS_EXPORT cuvsError_t cuvsAmdBallCoverAllKnnQuery(cuvsResources_t res, cuvsAmdBallCoverIndexParams_t params,
                                                    DLManagedTensor* dataset, DLManagedTensor* neighbors,
                                                    DLManagedTensor* distances, bool perform_post_filtering, float weight,
                                                    cuvsAmdBallCoverIndex_t index_out);

/* eps_nn over an L2 index: pair (i, j) is inside when the chain of eps_neighbors.h ends at acc <= fp32(eps * eps); eps is
 * the radius (>= 0). The outputs are those of cuvsAmdEpsNeighbors / cuvsAmdEpsNeighborsCsr called with the squared value,
 * byte for byte: adj bool/uint8 [q, m] or NULL, vd int32 or int64 [q + 1] or NULL (int64 in the CSR form); indptr, indices,
 * distances and max_k as there (column ids are original row ids in ascending order, distances the chain's values). */
CUVS_EXPORT cuvsError_t cuvsAmdBallCoverEpsNn(cuvsResources_t res, cuvsAmdBallCoverIndex_t index, DLManagedTensor* queries,
                                              DLManagedTensor* adj, DLManagedTensor* vd, float eps);
CUVS_EXPORT cuvsError_t cuvsAmdBallCoverEpsNnCsr(cuvsResources_t res, cuvsAmdBallCoverIndex_t index, DLManagedTensor* queries,
                                                 DLManagedTensor* indptr, DLManagedTensor* indices, DLManagedTensor* distances,
                                                 DLManagedTensor* vd, float eps, int64_t* max_k);

CUVS_EXPORT cuvsError_t cuvsAmdBallCoverIndexGetNLandmarks(cuvsAmdBallCoverIndex_t index, int64_t* n_landmarks);
CUVS_EXPORT cuvsError_t cuvsAmdBallCoverIndexGetSize(cuvsAmdBallCoverIndex_t index, int64_t* m);
CUVS_EXPORT cuvsError_t cuvsAmdBallCoverIndexGetDim(cuvsAmdBallCoverIndex_t index, int64_t* dim);
CUVS_EXPORT cuvsError_t cuvsAmdBallCoverIndexGetMetric(cuvsAmdBallCoverIndex_t index, cuvsDistanceType* metric);

/* the arrays of the index as non-owning device views (valid while the index lives; call the view's deleter) */
typedef enum {
  CUVS_AMD_BALL_COVER_R_INDPTR    = 0, /* int64 [n_landmarks + 1] */
  CUVS_AMD_BALL_COVER_R_1NN_COLS  = 1, /* int64 [m]: original row ids, list by list, by (distance to the landmark, id) */
  CUVS_AMD_BALL_COVER_R_1NN_DISTS = 2, /* fp32 [m] */
  CUVS_AMD_BALL_COVER_R_RADIUS    = 3, /* fp32 [n_landmarks]: the last distance of a list, 0 for an empty one */
  CUVS_AMD_BALL_COVER_R           = 4, /* fp32 [n_landmarks, dim]: the landmark rows */
  CUVS_AMD_BALL_COVER_X_REORDERED = 5, /* fp32 [m, dim] */
  CUVS_AMD_BALL_COVER_R_ROWS      = 6  /* int64 [n_landmarks]: the original row id of every landmark */
} cuvsAmdBallCoverArray;
CUVS_EXPORT cuvsError_t cuvsAmdBallCoverIndexGetArray(cuvsAmdBallCoverIndex_t index, cuvsAmdBallCoverArray which,
                                                      DLManagedTensor* out);

/* calling thread's last k-NN or eps_nn call: landmark lists visited, points scored, points of visited lists skipped by the
 * window, queries */
CUVS_EXPORT cuvsError_t cuvsAmdBallCoverLastStats(uint64_t out[4]);

#ifdef __cplusplus
}
#endif
