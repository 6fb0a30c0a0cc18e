// Host-only parts of single-linkage clustering (single_linkage.hip): argument checks, the k of the kNN graph, the round
// bound, the union-find that turns the sorted spanning tree into a dendrogram (the reference's build_dendrogram_host,
// cpp/src/cluster/detail/agglomerative.cuh:97-160) and the label roots of a cut (extract_flattened_clusters :293-316).
// No HIP and no DLPack types in here: tests/cpp/single_linkage_host_test.cpp builds this header alone under the sanitizers.
#pragma once

#include "eps_neighbors_host.hpp"

#include <algorithm>
#include <cstdint>
#include <functional>
#include <vector>

namespace cuvs_amd {
namespace sl_host {

using eps_host::refuse;
using eps_host::tensor_desc;

enum : int { kPairwise = 0, kKnnGraph = 1 };        // cuvsAmdLinkage
enum : int { kDistance = 0, kMutualReachability = 1 };  // cuvsAmdLinkageSpace

// true for the sqrt forms
inline bool check_metric(int metric)
{
  if (metric != 0 && metric != 1 && metric != 4 && metric != 5)
    refuse("single linkage accepts the metrics L2Expanded (0), L2SqrtExpanded (1), L2Unexpanded (4) and L2SqrtUnexpanded (5); got %d",
           metric);
  return metric == 1 || metric == 5;
}

inline void check_linkage(int linkage)
{
  if (linkage != kPairwise && linkage != kKnnGraph) refuse("linkage must be PAIRWISE (0) or KNN_GRAPH (1); got %d", linkage);
}

inline void check_space(int space)
{
  if (space != kDistance && space != kMutualReachability)
    refuse("space must be DISTANCE (0) or MUTUAL_REACHABILITY (1); got %d", space);
}

// X fp32 [n, dim], row-major, contiguous, on the device; 2 <= n < 2^30
inline void check_x(const tensor_desc& x, int64_t* n, int64_t* dim)
{
  if (!x.present) refuse("X must not be NULL");
  if (x.ndim != 2) refuse("X must be a 2-D matrix");
  if (!(x.code == 2 && x.bits == 32 && x.lanes == 1))
    refuse("X must be fp32 (fp16, fp64 and integer rows are not supported)");
  if (!x.on_device) refuse("X must be accessible on device memory (host rows are not supported)");
  if (!x.contiguous) refuse("X must be row-major and contiguous");
  if (x.shape[0] < 2) refuse("single linkage needs n >= 2 rows; got %lld", (long long)x.shape[0]);
  if (x.shape[0] >= (int64_t(1) << 30)) refuse("single linkage needs n < 2^30 rows; got %lld", (long long)x.shape[0]);
  if (x.shape[1] < 1) refuse("X must have at least one column");
  *n   = x.shape[0];
  *dim = x.shape[1];
}

// an int32 / int64 output [rows] or [rows, cols] (cols == 0: a vector); `bytes` carries the call's index type (0: not seen
// yet) - one type per call. A tensor that is not present is passed over when `required` is false.
inline void check_index(const tensor_desc& t, int64_t rows, int64_t cols, const char* what, bool required, int* bytes)
{
  if (!t.present) {
    if (required) refuse("%s must not be NULL", what);
    return;
  }
  const bool i64 = t.code == 0 && t.bits == 64 && t.lanes == 1;
  const bool i32 = t.code == 0 && t.bits == 32 && t.lanes == 1;
  if (!i64 && !i32) refuse("%s must be int32 or int64", what);
  if (*bytes != 0 && *bytes != (i64 ? 8 : 4)) refuse("%s: the index tensors of one call must have one type (int32 or int64)", what);
  *bytes = i64 ? 8 : 4;
  if (cols == 0) {
    if (t.ndim != 1 || t.shape[0] != rows) refuse("%s must have shape [%lld]", what, (long long)rows);
  } else if (t.ndim != 2 || t.shape[0] != rows || t.shape[1] != cols) {
    refuse("%s must have shape [%lld, %lld]", what, (long long)rows, (long long)cols);
  }
  eps_host::check_placed(t, what);
}

inline void check_f32_vector(const tensor_desc& t, int64_t rows, const char* what, bool required)
{
  if (!t.present) {
    if (required) refuse("%s must not be NULL", what);
    return;
  }
  if (!(t.code == 2 && t.bits == 32 && t.lanes == 1)) refuse("%s must be fp32", what);
  if (t.ndim != 1 || t.shape[0] != rows) refuse("%s must have shape [%lld]", what, (long long)rows);
  eps_host::check_placed(t, what);
}

inline void check_n_clusters(int64_t n_clusters, int64_t n)
{
  if (n_clusters < 1 || n_clusters > n)
    refuse("n_clusters must be in [1, n]: got %lld with n = %lld", (long long)n_clusters, (long long)n);
}

inline void check_min_samples(int64_t min_samples, int64_t n)
{
  if (min_samples < 2 || min_samples > n)
    refuse("min_samples must be in [2, n]: got %lld with n = %lld", (long long)min_samples, (long long)n);
}

inline int floor_log2(int64_t n)
{
  int l = 0;
  while ((n >> (l + 1)) != 0) ++l;
  return l;
}

// neighbours per row of the kNN graph (the reference's build_k, cpp/src/neighbors/detail/knn_graph.cuh:24-28)
inline int64_t build_k(int64_t n, int c) { return std::min<int64_t>(n, std::max<int64_t>(2, (int64_t)floor_log2(n) + c)); }

// a Boruvka round at least halves the components: ceil(log2 n) rounds reach one, plus one to spare
inline int max_dense_rounds(int64_t n)
{
  const int f = floor_log2(n);
  return ((int64_t(1) << f) == n ? f : f + 1) + 1;
}

// the reference's UnionFind over 2 n - 1 nodes: no union by rank, the new node of merge e is n + e
struct union_find {
  std::vector<int64_t> parent, size;
  int64_t next_label;
  explicit union_find(int64_t n) : parent((size_t)(2 * n - 1), -1), size((size_t)(2 * n - 1), 0), next_label(n)
  {
    std::fill(size.begin(), size.begin() + n, 1);
  }
  int64_t find(int64_t v)
  {
    int64_t root = v;
    while (parent[(size_t)root] != -1) root = parent[(size_t)root];
    while (v != root) {  // path compression
      const int64_t up   = parent[(size_t)v];
      parent[(size_t)v] = root;
      v                 = up;
    }
    return root;
  }
  void merge(int64_t a, int64_t b)
  {
    size[(size_t)next_label] = size[(size_t)a] + size[(size_t)b];
    parent[(size_t)a]        = next_label;
    parent[(size_t)b]        = next_label;
    ++next_label;
  }
};

// edges in merge order -> children [n_edges, 2], out_delta, out_size. An edge whose ends are outside [0, n_edges] or already in
// one tree is refused: the input is no spanning tree.
template <typename IdxT>
void build_dendrogram(const IdxT* rows, const IdxT* cols, const float* data, int64_t n_edges, IdxT* children, float* out_delta,
                      IdxT* out_size)
{
  const int64_t n = n_edges + 1;
  union_find u(n);
  for (int64_t e = 0; e < n_edges; ++e) {
    const int64_t a = (int64_t)rows[e], b = (int64_t)cols[e];
    if (a < 0 || a >= n || b < 0 || b >= n) refuse("edge %lld has an end outside [0, %lld)", (long long)e, (long long)n);
    const int64_t aa = u.find(a), bb = u.find(b);
    if (aa == bb) refuse("edge %lld closes a cycle: the edges are no spanning tree", (long long)e);
    children[2 * e]     = (IdxT)aa;
    children[2 * e + 1] = (IdxT)bb;
    out_delta[e]        = data[e];
    out_size[e]         = (IdxT)(u.size[(size_t)aa] + u.size[(size_t)bb]);
    u.merge(aa, bb);
  }
}

// the roots of the cut into n_clusters (> 1): the n_clusters smallest ids among the children of the last n_clusters - 1 merges,
// in descending order - roots[t] gets label t
template <typename IdxT>
std::vector<int64_t> label_roots(const IdxT* children, int64_t n, int64_t n_clusters)
{
  const int64_t n_edges = n - 1, take = (n_clusters - 1) * 2;
  std::vector<int64_t> r((size_t)take);
  for (int64_t t = 0; t < take; ++t) r[(size_t)t] = (int64_t)children[2 * n_edges - take + t];
  std::sort(r.begin(), r.end(), std::greater<int64_t>());
  return std::vector<int64_t>(r.end() - n_clusters, r.end());
}

}  // namespace sl_host
}  // namespace cuvs_amd
