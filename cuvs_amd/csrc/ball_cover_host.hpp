// Host-only parts of the random ball cover (ball_cover.hip): the landmark draw, the order of the landmark lists, the argument
// checks and the slabs of the CSR fill. No HIP and no DLPack types in here: tests/cpp/ball_cover_host_test.cpp builds this
// header alone under the sanitizers. DESIGN 3.1u.
#pragma once

#include "eps_neighbors_host.hpp"
#include "mix_hash.hpp"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <numeric>
#include <utility>
#include <vector>

namespace cuvs_amd {
namespace bc_host {

using eps_host::refuse;

constexpr int kL2Sqrt = 1, kL2SqrtUnexpanded = 5, kHaversine = 13;
constexpr int kMaxK = 256, kMaxEpsDim = 32;

// margins of the pruning expressions. Relative: a computed L2 distance of dim <= 32 is within 18 unit roundoffs
// (2^-24) of the true one and 2^-17 is 128 of them; the haversine formula loses up to 5e-4 relative where asinf's argument is
// near 1 (points almost opposite each other) and 2^-8 is eight times that. Absolute (Haversine only): a longitude difference
// near 2 pi is rounded to 2.4e-7, which the formula hands on to small distances across the +-pi seam; 2^-16 is 60 times that.
inline float margin_of(int metric) { return metric == kHaversine ? 0x1p-8f : 0x1p-17f; }
inline float slack_of(int metric) { return metric == kHaversine ? 0x1p-16f : 0.f; }

inline bool metric_ok(int metric) { return metric == kL2Sqrt || metric == kL2SqrtUnexpanded || metric == kHaversine; }

inline void check_build(int metric, int64_t m, int64_t dim, int64_t n_landmarks)
{
  if (!metric_ok(metric))
    refuse("ball cover: metric %d is not supported (L2SqrtExpanded, L2SqrtUnexpanded or Haversine; the squared L2 forms are not metrics)",
           metric);
  if (m < 1) refuse("ball cover: the dataset needs at least one row");
  if (m >= (int64_t(1) << 32)) refuse("ball cover: m must be below 2^32");
  if (metric == kHaversine && dim != 2) refuse("ball cover: Haversine needs dim == 2 (latitude, longitude), got %lld", (long long)dim);
  if (dim < 1 || dim > kMaxEpsDim) refuse("ball cover: dim must be in [1, %d], got %lld", kMaxEpsDim, (long long)dim);
  if (n_landmarks < 0 || n_landmarks > m)
    refuse("ball cover: n_landmarks (%lld) must not exceed the number of rows (%lld)", (long long)n_landmarks, (long long)m);
}

inline void check_knn(int metric, int64_t dim, int64_t qdim, int64_t k, int64_t n_landmarks, float weight)
{
  if (qdim != dim) refuse("ball cover: queries have %lld columns, the index has %lld", (long long)qdim, (long long)dim);
  if (metric == kHaversine ? dim != 2 : (dim != 2 && dim != 3))
    refuse("ball cover: k-NN needs dim 2 or 3 (L2) or 2 (Haversine), the index has dim %lld", (long long)dim);
  if (k < 1 || k > kMaxK) refuse("ball cover: k must be in [1, %d], got %lld", kMaxK, (long long)k);
  if (k > n_landmarks) refuse("ball cover: k (%lld) must not exceed n_landmarks (%lld)", (long long)k, (long long)n_landmarks);
  if (!(weight >= 0.f) || !std::isfinite(weight)) refuse("ball cover: weight must be finite and not negative");
}

inline void check_eps(int metric, int64_t dim, int64_t qdim, float eps)
{
  if (metric == kHaversine) refuse("ball cover: eps_nn needs an L2 index, this one is Haversine");
  if (qdim != dim) refuse("ball cover: queries have %lld columns, the index has %lld", (long long)qdim, (long long)dim);
  if (!(eps >= 0.f) || !std::isfinite(eps)) refuse("ball cover: eps (the radius) must be finite and not negative");
}

// floor(sqrt(m)), exactly
inline int64_t isqrt(int64_t m)
{
  int64_t r = (int64_t)std::sqrt((double)m);
  while (r * r > m) --r;
  while ((r + 1) * (r + 1) <= m) ++r;
  return r;
}
inline int64_t landmarks_of(int64_t m, int64_t n_landmarks) { return n_landmarks > 0 ? n_landmarks : std::max<int64_t>(1, isqrt(m)); }

// landmark l is the row with the l-th smallest (hash, row id), the hash being that of the HNSW levels (mix_hash.hpp): n
// distinct rows, a function of (m, n, seed) alone
inline std::vector<int64_t> draw_landmarks(int64_t m, int64_t n, uint32_t seed)
{
  std::vector<uint64_t> key((size_t)m);
  for (int64_t i = 0; i < m; ++i) key[(size_t)i] = ((uint64_t)mix_hash(seed, (uint32_t)i) << 32) | (uint64_t)(uint32_t)i;
  if (n < m) std::nth_element(key.begin(), key.begin() + n, key.end());
  std::sort(key.begin(), key.begin() + n);
  std::vector<int64_t> rows((size_t)n);
  for (int64_t l = 0; l < n; ++l) rows[(size_t)l] = (int64_t)(key[(size_t)l] & 0xFFFFFFFFu);
  return rows;
}

// rows grouped by label, each list by (distance, row id). dists are not negative, so their bits order like their values.
// Writes indptr [n + 1], cols [m], sorted dists [m] and radius [n] (the last distance of a list, 0 for an empty one).
inline void order_lists(const uint32_t* label, const float* dist, int64_t m, int64_t n, int64_t* indptr, int64_t* cols, float* sdist,
                        float* radius)
{
  std::fill(indptr, indptr + n + 1, int64_t(0));
  for (int64_t i = 0; i < m; ++i) indptr[label[i] + 1] += 1;
  for (int64_t l = 0; l < n; ++l) indptr[l + 1] += indptr[l];
  std::vector<int64_t> at(indptr, indptr + n);
  for (int64_t i = 0; i < m; ++i) cols[at[label[i]]++] = i;  // ascending row id inside a list
  for (int64_t l = 0; l < n; ++l) {
    int64_t* b = cols + indptr[l];
    int64_t* e = cols + indptr[l + 1];
    std::stable_sort(b, e, [&](int64_t x, int64_t y) { return dist[x] < dist[y]; });
    radius[l] = b == e ? 0.f : dist[*(e - 1)];
  }
  for (int64_t i = 0; i < m; ++i) sdist[i] = dist[cols[i]];
}

// rows [r0, r1) of one slab of the CSR fill: as many rows as keep the scratch (16 bytes per edge) inside the budget, one at least
inline int64_t slab_end(const int64_t* degrees, int64_t rows, int64_t r0, int64_t budget_bytes)
{
  int64_t edges = 0, r = r0;
  while (r < rows) {
    if (r > r0 && (edges + degrees[r]) > budget_bytes / 16) break;
    edges += degrees[r];
    ++r;
  }
  return r;
}

}  // namespace bc_host
}  // namespace cuvs_amd
