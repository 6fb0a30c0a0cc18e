// Host-only parts of cuvs::stats (stats.hip): argument checks, the column segments of the label-sorted rows, the row-slab sizes
// and the score formulas. No HIP and no DLPack types in here: tests/cpp/stats_host_test.cpp builds this header alone under the
// sanitizers. sil_sample() is also what the device evaluates (STATS_HD).
#pragma once

#include "eps_neighbors_host.hpp"

#include <cmath>
#include <limits>
#include <vector>

#if defined(__HIPCC__)
#define STATS_HD __host__ __device__
#else
#define STATS_HD
#endif

namespace cuvs_amd {
namespace stats_host {

using eps_host::check_placed;
using eps_host::refuse;
using eps_host::tensor_desc;

constexpr int kTile         = eps_host::kTile;  // the pair tile is kTile x kTile
constexpr int kMaxNeighbors = 64;

// what the pair tile accumulates, and what the epilogue makes of it
enum class chain_t : int { sq = 0, l1 = 1, dot = 2 };
enum class post_t : int { none = 0, sqrt = 1, cosine = 2 };
struct metric_plan {
  chain_t chain;
  post_t post;
};

// silhouette: the four L2 ids (one arithmetic: the chain of squared differences), L1, CosineExpanded
inline metric_plan check_silhouette_metric(int metric)
{
  switch (metric) {
    case 0:
    case 4: return {chain_t::sq, post_t::none};
    case 1:
    case 5: return {chain_t::sq, post_t::sqrt};
    case 3: return {chain_t::l1, post_t::none};
    case 2: return {chain_t::dot, post_t::cosine};
    default:
      refuse("metric %d is not supported by the silhouette score: L2Expanded, L2SqrtExpanded, L2Unexpanded, L2SqrtUnexpanded, L1 "
             "or CosineExpanded",
             metric);
  }
}

// trustworthiness: the four L2 ids; the ranks are always taken on the squared chain
inline void check_trustworthiness_metric(int metric)
{
  if (!(metric == 0 || metric == 1 || metric == 4 || metric == 5))
    refuse("metric %d is not supported by the trustworthiness score: L2Expanded, L2SqrtExpanded, L2Unexpanded or L2SqrtUnexpanded",
           metric);
}

// X fp32 [n, dim]
inline void check_matrix(const tensor_desc& x, const char* what, int64_t* n, int64_t* dim)
{
  if (!x.present) refuse("%s must not be NULL", what);
  if (x.ndim != 2) refuse("%s must be a 2-D matrix", what);
  if (!(x.code == 2 && x.bits == 32 && x.lanes == 1)) refuse("%s must be fp32 (fp64 and fp16 rows are not supported)", what);
  check_placed(x, what);
  if (x.shape[0] < 0 || x.shape[1] < 0) refuse("%s has a negative extent", what);
  if (x.shape[0] >= (int64_t(1) << 31)) refuse("%s has %lld rows: n must be below 2^31", what, (long long)x.shape[0]);
  *n   = x.shape[0];
  *dim = x.shape[1];
}

// a vector of n elements: labels (int32), scores (fp32)
inline void check_vector(const tensor_desc& v, const char* what, int64_t n, bool f32, bool optional)
{
  if (!v.present) {
    if (optional) return;
    refuse("%s must not be NULL", what);
  }
  const bool ok = f32 ? (v.code == 2 && v.bits == 32 && v.lanes == 1) : (v.code == 0 && v.bits == 32 && v.lanes == 1);
  if (!ok) refuse(f32 ? "%s must be fp32" : "%s must be int32 (int64 labels are not supported)", what);
  if (v.ndim != 1 || v.shape[0] != n) refuse("%s must have shape [%lld]", what, (long long)n);
  check_placed(v, what);
}

// the reference's rule (silhouette_score.cuh): 2 <= n_labels <= n - 1
inline void check_n_labels(int64_t n_labels, int64_t n)
{
  if (n_labels < 2 || n_labels > n - 1)
    refuse("n_labels must be in [2, n - 1]: n_labels is %lld, n is %lld", (long long)n_labels, (long long)n);
}

// counts of the label-count pass; `bad` is the number of labels outside [0, n_labels)
inline void check_label_counts(int64_t bad, int64_t n_labels)
{
  if (bad != 0) refuse("labels holds %lld values outside [0, %lld)", (long long)bad, (long long)n_labels);
}

// neighbors int64 [n, k], 1 <= k <= kMaxNeighbors; returns k
inline int check_neighbors(const tensor_desc& nb, int64_t n)
{
  if (!nb.present) refuse("neighbors must not be NULL");
  if (!(nb.code == 0 && nb.bits == 64 && nb.lanes == 1)) refuse("neighbors must be int64");
  if (nb.ndim != 2 || nb.shape[0] != n) refuse("neighbors must have shape [%lld, k]", (long long)n);
  check_placed(nb, "neighbors");
  const int64_t k = nb.shape[1];
  if (k < 1 || k > kMaxNeighbors) refuse("neighbors has k = %lld columns: k must be in [1, %d]", (long long)k, kMaxNeighbors);
  return (int)k;
}

inline void check_ranks(const tensor_desc& r, int64_t n, int k)
{
  if (!r.present) return;
  if (!(r.code == 0 && r.bits == 32 && r.lanes == 1)) refuse("ranks must be int32");
  if (r.ndim != 2 || r.shape[0] != n || r.shape[1] != k) refuse("ranks must have shape [%lld, %d]", (long long)n, k);
  check_placed(r, "ranks");
}

// flags of the neighbour-id pass: bit 0 an id equal to its row, bit 1 an id outside [0, n)
inline void check_neighbor_flags(unsigned flags, int64_t n)
{
  if (flags & 2u) refuse("neighbors holds an id outside [0, %lld)", (long long)n);
  if (flags & 1u) refuse("neighbors holds a row's own id (neighbors[i][q] == i)");
}

// sklearn's rule: n_neighbors < n / 2 (the reference divides by zero at 2 n = 3 k + 1)
inline void check_n_neighbors(int64_t k, int64_t n)
{
  if (k < 1) refuse("n_neighbors must be positive");
  if (k > kMaxNeighbors) refuse("n_neighbors = %lld is not supported: n_neighbors must be at most %d", (long long)k, kMaxNeighbors);
  if (2 * k >= n) refuse("n_neighbors = %lld must be less than n / 2 (n is %lld)", (long long)k, (long long)n);
}

// ---------------------------------------------------------------- column segments
// The rows sorted by label (stable) occupy positions [0, n). A segment is a run of positions inside one column tile and one
// label; the segments are in position order, hence in label order, and every tile owns tile_first[t] .. tile_first[t + 1] - 1.
struct segments {
  std::vector<int32_t> lo, hi, label;  // [count]: positions [lo, hi) carry `label`
  std::vector<int32_t> tile_first;     // [col_tiles + 1]
  std::vector<int32_t> label_first;    // [n_labels]: first position of a label (where the counting sort starts to write)
  int64_t straddling = 0;              // column tiles that hold more than one segment
  int64_t count() const { return (int64_t)lo.size(); }
};

inline segments build_segments(const int32_t* counts, int64_t n_labels, int64_t n)
{
  segments s;
  const int64_t tiles = (n + kTile - 1) / kTile;
  s.tile_first.assign((size_t)tiles + 1, 0);
  s.label_first.resize((size_t)n_labels);
  int64_t pos = 0;
  for (int64_t c = 0; c < n_labels; ++c) {
    s.label_first[(size_t)c] = (int32_t)pos;
    int64_t end = pos + counts[c];
    if (end > n) refuse("the label counts add up to more than n");
    while (pos < end) {
      const int64_t stop = std::min<int64_t>(end, (pos / kTile + 1) * kTile);
      s.lo.push_back((int32_t)pos);
      s.hi.push_back((int32_t)stop);
      s.label.push_back((int32_t)c);
      s.tile_first[(size_t)(pos / kTile) + 1] += 1;
      pos = stop;
    }
  }
  if (pos != n) refuse("the label counts add up to %lld, n is %lld", (long long)pos, (long long)n);
  for (int64_t t = 0; t < tiles; ++t) {
    if (s.tile_first[(size_t)t + 1] > 1) s.straddling += 1;
    s.tile_first[(size_t)t + 1] += s.tile_first[(size_t)t];
  }
  return s;
}

// ---------------------------------------------------------------- slabs
// rows per slab: as many as `budget_bytes` holds at `row_bytes` each, a multiple of the tile (at least one tile), capped by the
// caller's `batch_rows` (> 0) and by the test hook `forced` (> 0)
inline int64_t slab_rows(int64_t n, int64_t row_bytes, int64_t budget_bytes, int64_t batch_rows, int64_t forced)
{
  if (n <= 0) return 0;
  int64_t rows = budget_bytes / std::max<int64_t>(row_bytes, 1);
  rows         = std::max<int64_t>(rows / kTile * kTile, kTile);
  if (batch_rows > 0) rows = std::min(rows, batch_rows);
  if (forced > 0) rows = std::min(rows, forced);
  return std::min(n, rows);
}

// silhouette: one fp64 partial per (row, segment)
inline int64_t silhouette_row_bytes(int64_t n_segments) { return n_segments * 8; }
// ranks: the k sorted thresholds of a row (fp32), their ids (int32), their columns in the caller's list (1 byte), the buckets
inline int64_t ranks_row_bytes(int k) { return (int64_t)k * 13; }

// ---------------------------------------------------------------- formulas
// s_i from S[i][own] (`s_own`), the size of the own cluster and b_i (+inf: no other label has a row). Semantics of the
// reference's SilOp / populateAKernel and of sklearn: a singleton scores 0, a == b scores 0.
STATS_HD inline double sil_sample(double s_own, double cnt_own, double b)
{
  if (cnt_own == 1.0) return 0.0;
  const double a = s_own / (cnt_own - 1.0);
  if (a == b || b == std::numeric_limits<double>::infinity()) return 0.0;
  return (b - a) / (a > b ? a : b);
}

// the fp64 sum in index order, divided by n
inline double sil_mean(const double* s, int64_t n)
{
  double sum = 0.0;
  for (int64_t i = 0; i < n; ++i) sum += s[i];
  return sum / (double)n;
}

// the reference's trustworthiness_score.cuh, literally, with t the penalty sum
inline double trustworthiness(int64_t n, int64_t k, uint64_t t)
{
  return 1.0 - ((2.0 / (((double)n * (double)k) * ((2.0 * (double)n) - (3.0 * (double)k) - 1.0))) * (double)t);
}

}  // namespace stats_host
}  // namespace cuvs_amd
