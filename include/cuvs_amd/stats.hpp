// C++ surface over the C ABI of include/cuvs_amd/stats.h: cuvs::stats::{silhouette_score, silhouette_score_batched,
// trustworthiness_score} with the reference's names (cpp/include/cuvs/stats/silhouette_score.hpp, trustworthiness_score.hpp),
// and neighbor_ranks, the kernel under the trustworthiness score. Header-only, C++17, no HIP and no RAFT headers; views,
// resources and errors are those of neighbors.hpp. fp32 rows and int32 labels only (stats.h lists what is out of scope).
#pragma once
#include <cuvs_amd/neighbors.hpp>
#include <cuvs_amd/stats.h>

namespace cuvs {
namespace stats {

// the mean silhouette coefficient; silhouette_score_per_sample (fp32 [n] on the device) may be null
inline float silhouette_score(const resources& res, device_matrix_view<const float> X, const int32_t* labels,
                              float* silhouette_score_per_sample, int64_t n_unique_labels,
                              cuvsDistanceType metric = L2Unexpanded)
{
  detail::tensor<const float> tx(X);
  detail::vector_tensor<const int32_t> tl(labels, X.extent(0));
  detail::vector_tensor<float> ts(silhouette_score_per_sample, X.extent(0));
  double mean = 0.0;
  check(cuvsAmdSilhouetteScore(res.get(), tx.get(), tl.get(), n_unique_labels, metric, 0, ts.get(), &mean), "cuvsAmdSilhouetteScore");
  return (float)mean;
}

// the same value, bit for bit, with at most `chunk` rows in flight
inline float silhouette_score_batched(const resources& res, device_matrix_view<const float> X, const int32_t* labels,
                                      float* silhouette_score_per_sample, int64_t n_unique_labels, int64_t chunk,
                                      cuvsDistanceType metric = L2Unexpanded)
{
  detail::tensor<const float> tx(X);
  detail::vector_tensor<const int32_t> tl(labels, X.extent(0));
  detail::vector_tensor<float> ts(silhouette_score_per_sample, X.extent(0));
  double mean = 0.0;
  check(cuvsAmdSilhouetteScore(res.get(), tx.get(), tl.get(), n_unique_labels, metric, chunk, ts.get(), &mean),
        "cuvsAmdSilhouetteScore");
  return (float)mean;
}

// the fp64 mean of either form
inline double silhouette_score_f64(const resources& res, device_matrix_view<const float> X, const int32_t* labels,
                                   float* silhouette_score_per_sample, int64_t n_unique_labels, int64_t chunk = 0,
                                   cuvsDistanceType metric = L2Unexpanded)
{
  detail::tensor<const float> tx(X);
  detail::vector_tensor<const int32_t> tl(labels, X.extent(0));
  detail::vector_tensor<float> ts(silhouette_score_per_sample, X.extent(0));
  double mean = 0.0;
  check(cuvsAmdSilhouetteScore(res.get(), tx.get(), tl.get(), n_unique_labels, metric, chunk, ts.get(), &mean),
        "cuvsAmdSilhouetteScore");
  return mean;
}

// ranks int32 [n, k] (may be a null view) of the listed neighbours among the rows of X; returns the penalty sum
inline uint64_t neighbor_ranks(const resources& res, device_matrix_view<const float> X, device_matrix_view<const int64_t> neighbors,
                               device_matrix_view<int32_t> ranks)
{
  detail::tensor<const float> tx(X);
  detail::tensor<const int64_t> tn(neighbors);
  detail::tensor<int32_t> tr(ranks);
  uint64_t penalty = 0;
  check(cuvsAmdNeighborRanks(res.get(), tx.get(), tn.get(), ranks.ptr ? tr.get() : nullptr, &penalty), "cuvsAmdNeighborRanks");
  return penalty;
}

inline double trustworthiness_score(const resources& res, device_matrix_view<const float> X, device_matrix_view<const float> X_embedded,
                                    int n_neighbors, cuvsDistanceType metric = L2SqrtUnexpanded)
{
  detail::tensor<const float> tx(X), te(X_embedded);
  double score = 0.0;
  check(cuvsAmdTrustworthinessScore(res.get(), tx.get(), te.get(), n_neighbors, metric, &score), "cuvsAmdTrustworthinessScore");
  return score;
}

}  // namespace stats
}  // namespace cuvs
