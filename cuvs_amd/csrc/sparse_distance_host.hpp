// Host-only parts of the sparse (CSR) pairwise distances and of the sparse brute-force kNN (sparse_distance.hip): the
// metric-to-family table, argument checks, batch arithmetic, the plan of virtual rows (long-row split) and the slab size. No
// HIP and no DLPack types in here: tests/cpp/sparse_distance_host_test.cpp builds this header alone under the sanitizers.
#pragma once

#include "eps_neighbors_host.hpp"

#include <climits>
#include <cmath>
#include <vector>

namespace cuvs_amd {
namespace sparse_host {

using eps_host::refuse;
using eps_host::tensor_desc;

constexpr int kThreads = 256;   // workgroup
constexpr int kTA      = 4;     // rows of x per workgroup: one 16-byte LDS read serves a column
constexpr int kRangeI  = 2048;  // columns per range of the intersection kernel (dense image, 32 KiB)
constexpr int kRangeU  = 1024;  // columns per range of the union kernel (kTA sorted lists of at most that many entries, 32 KiB)
constexpr int kSplit   = 1024;  // stored entries of a y row per chain segment
// forms of the walk over the rows of y (sparse_distance.hip kForms): which one a shape gets
constexpr int kFormDirect = 1;        // 8 (intersection) / 4 (union) rows per thread, one entry per load
constexpr int kFormStaged = 2;        // 1 row per thread through the wave's LDS stage, 8 entries per refill
constexpr double kStageMinPerStep = 8.0;  // stored entries of a y row per range step from which the stage is used

enum : int { kNone = 0, kIntersection = 1, kUnion = 2 };

// cuvsDistanceType
enum : int {
  L2Expanded = 0, L2SqrtExpanded = 1, CosineExpanded = 2, L1 = 3, L2Unexpanded = 4, L2SqrtUnexpanded = 5, InnerProduct = 6,
  Linf = 7, Canberra = 8, LpUnexpanded = 9, CorrelationExpanded = 10, JaccardExpanded = 11, HellingerExpanded = 12,
  Haversine = 13, BrayCurtis = 14, JensenShannon = 15, HammingUnexpanded = 16, KLDivergence = 17, RusselRaoExpanded = 18,
  DiceExpanded = 19, BitwiseHamming = 20
};

inline const char* metric_name(int metric)
{
  static const char* names[] = {"L2Expanded", "L2SqrtExpanded", "CosineExpanded", "L1", "L2Unexpanded", "L2SqrtUnexpanded",
                                "InnerProduct", "Linf", "Canberra", "LpUnexpanded", "CorrelationExpanded", "JaccardExpanded",
                                "HellingerExpanded", "Haversine", "BrayCurtis", "JensenShannon", "HammingUnexpanded",
                                "KLDivergence", "RusselRaoExpanded", "DiceExpanded", "BitwiseHamming"};
  return metric >= 0 && metric <= 20 ? names[metric] : "unknown";
}

inline int family_of(int metric)
{
  switch (metric) {
    case InnerProduct: case L2Expanded: case L2SqrtExpanded: case CosineExpanded: case CorrelationExpanded: case JaccardExpanded:
    case DiceExpanded: case RusselRaoExpanded: case HellingerExpanded: case KLDivergence: return kIntersection;
    case L1: case L2Unexpanded: case L2SqrtUnexpanded: case Linf: case Canberra: case LpUnexpanded: case HammingUnexpanded:
    case JensenShannon: return kUnion;
    default: return kNone;
  }
}

// the chains of a split row are combined by fmaxf (Linf), by integer addition (Hamming's count) or by fp32 addition
enum : int { kCombineAdd = 0, kCombineMax = 1, kCombineCount = 2 };
inline int combine_of(int metric) { return metric == Linf ? kCombineMax : (metric == HammingUnexpanded ? kCombineCount : kCombineAdd); }

// nearest = smallest, except for the similarity (distance.hpp:72-85 is_min_close)
inline bool select_min(int metric) { return metric != InnerProduct; }

inline int check_metric(int metric, float metric_arg)
{
  const int fam = family_of(metric);
  if (fam == kNone) refuse("sparse distances do not support metric %d (%s)", metric, metric_name(metric));
  if (metric == LpUnexpanded && !(metric_arg > 0.f)) refuse("LpUnexpanded needs metric_arg (p) > 0, got %g", (double)metric_arg);
  return fam;
}

// the three arrays of a CSR matrix of `rows` rows as their DLPack shapes bound them; returns nnz
inline int64_t check_csr(const tensor_desc& indptr, const tensor_desc& indices, const tensor_desc& data, int64_t rows, int64_t n_cols,
                         const char* what)
{
  if (!indptr.present || !indices.present || !data.present) refuse("%s: indptr, indices and data must not be NULL", what);
  if (rows < 0 || n_cols < 0) refuse("%s: negative extent", what);
  if (rows >= INT_MAX || n_cols > INT_MAX) refuse("%s: rows and columns are int32", what);
  if (!(indptr.code == 0 && indptr.bits == 32 && indptr.lanes == 1)) refuse("%s: indptr must be int32 (int64 is not supported)", what);
  if (!(indices.code == 0 && indices.bits == 32 && indices.lanes == 1)) refuse("%s: indices must be int32 (int64 is not supported)", what);
  if (!(data.code == 2 && data.bits == 32 && data.lanes == 1)) refuse("%s: data must be fp32 (fp16 and fp64 are not supported)", what);
  if (indptr.ndim != 1 || indices.ndim != 1 || data.ndim != 1) refuse("%s: indptr, indices and data must be vectors", what);
  if (indptr.shape[0] != rows + 1) refuse("%s: indptr must have shape [%lld] (rows + 1), got [%lld]", what, (long long)(rows + 1), (long long)indptr.shape[0]);
  if (indices.shape[0] != data.shape[0])
    refuse("%s: indices holds %lld entries but data holds %lld", what, (long long)indices.shape[0], (long long)data.shape[0]);
  if (indices.shape[0] >= (int64_t(1) << 31)) refuse("%s: nnz must be below 2^31", what);
  if (!indptr.on_device || !indices.on_device || !data.on_device) refuse("%s: indptr, indices and data must be accessible on device memory", what);
  if (!indptr.contiguous || !indices.contiguous || !data.contiguous) refuse("%s: indptr, indices and data must be contiguous", what);
  return indices.shape[0];
}

// out fp32 [m, n]
inline void check_out(const tensor_desc& out, int64_t m, int64_t n)
{
  if (!out.present) refuse("out must not be NULL");
  if (!(out.code == 2 && out.bits == 32 && out.lanes == 1)) refuse("out must be fp32");
  if (out.ndim != 2 || out.shape[0] != m || out.shape[1] != n) refuse("out must have shape [%lld, %lld]", (long long)m, (long long)n);
  eps_host::check_placed(out, "out");
}

// neighbors int32 / int64 [n_queries, k], distances fp32 [n_queries, k]; returns the bytes of a neighbour id
inline int check_knn(const tensor_desc& neighbors, const tensor_desc& distances, int64_t n_queries, int64_t k, int64_t n_index,
                     int64_t batch_size_index, int64_t batch_size_query)
{
  if (k <= 0) refuse("k must be positive");
  if (k > n_index) refuse("k (%lld) is larger than the number of index rows (%lld)", (long long)k, (long long)n_index);
  if (k > (1 << 24)) refuse("k must be at most 2^24");
  if (batch_size_index <= 0 || batch_size_query <= 0) refuse("batch_size_index and batch_size_query must be positive");
  if (!neighbors.present || !distances.present) refuse("neighbors and distances must not be NULL");
  const bool i64 = neighbors.code == 0 && neighbors.bits == 64 && neighbors.lanes == 1;
  const bool i32 = neighbors.code == 0 && neighbors.bits == 32 && neighbors.lanes == 1;
  if (!i64 && !i32) refuse("neighbors must be int64 or int32");
  if (!(distances.code == 2 && distances.bits == 32 && distances.lanes == 1)) refuse("distances must be fp32");
  if (neighbors.ndim != 2 || neighbors.shape[0] != n_queries || neighbors.shape[1] != k)
    refuse("neighbors must have shape [%lld, %lld]", (long long)n_queries, (long long)k);
  if (distances.ndim != 2 || distances.shape[0] != n_queries || distances.shape[1] != k)
    refuse("distances must have shape [%lld, %lld]", (long long)n_queries, (long long)k);
  eps_host::check_placed(neighbors, "neighbors");
  eps_host::check_placed(distances, "distances");
  return i64 ? 8 : 4;
}

// ---------------------------------------------------------------- batches
inline int64_t n_batches(int64_t rows, int64_t batch) { return rows <= 0 ? 0 : (rows + batch - 1) / batch; }
// rows [begin, begin + count) of batch b
inline void batch_rows(int64_t rows, int64_t batch, int64_t b, int64_t* begin, int64_t* count)
{
  *begin = b * batch;
  *count = std::min(batch, rows - *begin);
}

// the distance tile of a search, batch_index x batch_query floats, stays inside the workspace budget: fewer queries per batch
// first, then fewer index rows
inline void cap_tile(int64_t budget_bytes, int64_t* batch_index, int64_t* batch_query)
{
  const int64_t cap = std::max<int64_t>(1, budget_bytes / 4);
  if (*batch_index > cap / std::max<int64_t>(*batch_query, 1)) *batch_query = std::max<int64_t>(1, cap / std::max<int64_t>(*batch_index, 1));
  if (*batch_index > cap) *batch_index = cap;
}

// ---------------------------------------------------------------- virtual rows (the long-row split)
// A thread of the pair kernels owns one virtual row: the stored entries [begin, end) of row `row` of y. A row with more than
// kSplit stored entries is cut after every kSplit-th one; every piece is a chain of its own from 0 (slot: where its raw
// accumulators go), and the pieces are combined in order afterwards. slot < 0: the whole row, finished by the thread.
struct vrow {
  int row, begin, end, slot;
};
struct split_row {
  int row, first_slot, pieces, pad;
};

// rows [r0, r0 + rows) of a matrix whose (host copy of) indptr is given; `row` is relative to r0, begin / end are absolute
inline void plan_vrows(const int* indptr, int64_t r0, int64_t rows, int split, std::vector<vrow>* vrows, std::vector<split_row>* splits)
{
  vrows->clear();
  splits->clear();
  int slots = 0;
  for (int64_t r = 0; r < rows; ++r) {
    const int b = indptr[r0 + r], e = indptr[r0 + r + 1];
    if (e - b <= split) {
      vrows->push_back(vrow{(int)r, b, e, -1});
      continue;
    }
    const int pieces = (int)(((int64_t)e - b + split - 1) / split);
    splits->push_back(split_row{(int)r, slots, pieces, 0});
    for (int s = 0; s < pieces; ++s)  // (in 64 bits: a row may end at nnz = 2^31 - 1)
      vrows->push_back(vrow{(int)r, (int)(b + (int64_t)s * split), (int)std::min<int64_t>(e, b + ((int64_t)s + 1) * split), slots++});
  }
}

inline int64_t total_slots(const std::vector<split_row>& splits)
{
  return splits.empty() ? 0 : (int64_t)splits.back().first_slot + splits.back().pieces;
}

// rows of x per launch: the raw accumulators of the split pieces (4 bytes per slot and row of x) stay inside the budget
inline int64_t slab_rows(int64_t m, int64_t slots, int64_t budget_bytes)
{
  if (m <= 0) return 0;
  if (slots <= 0) return m;
  int64_t rows = budget_bytes / (4 * slots);
  rows         = std::max<int64_t>(rows / kTA * kTA, kTA);
  return std::min(m, rows);
}

// pair tiles of a launch: kTA rows of x by vrows_per_thread * kThreads virtual rows of y
inline int64_t n_tiles(int64_t x_rows, int64_t n_vrows, int vrows_per_thread)
{
  const int64_t per = (int64_t)kThreads * vrows_per_thread;
  return ((x_rows + kTA - 1) / kTA) * ((n_vrows + per - 1) / per);
}

// column ranges a matrix of n_cols columns has
inline int64_t n_ranges(int64_t n_cols, int range) { return (n_cols + range - 1) / range; }

// ---------------------------------------------------------------- the validator's verdict
enum : int { kBadIndptr0 = 1, kBadIndptrOrder = 2, kBadIndptrEnd = 3, kBadColumn = 4, kBadOrder = 5 };
constexpr unsigned long long kValid = ~0ull;
inline unsigned long long verdict_key(int64_t row, int code) { return ((unsigned long long)row << 8) | (unsigned)code; }

inline void check_verdict(unsigned long long key, const char* what, int64_t rows, int64_t nnz, int64_t n_cols)
{
  if (key == kValid) return;
  const long long row = (long long)(key >> 8);
  switch ((int)(key & 255)) {
    case kBadIndptr0: refuse("%s is not a canonical CSR matrix: indptr[0] is not 0", what);
    case kBadIndptrOrder: refuse("%s is not a canonical CSR matrix: indptr decreases or leaves [0, nnz] at row %lld", what, row);
    case kBadIndptrEnd: refuse("%s is not a canonical CSR matrix: indptr[%lld] is not nnz (%lld)", what, (long long)rows, (long long)nnz);
    case kBadColumn: refuse("%s is not a canonical CSR matrix: row %lld holds a column outside [0, %lld)", what, row, (long long)n_cols);
    default: refuse("%s is not a canonical CSR matrix: the columns of row %lld are not strictly ascending", what, row);
  }
}

}  // namespace sparse_host
}  // namespace cuvs_amd
