// Host-only parts of the masked L2 nearest neighbour and of cross_component_nn (masked_nn.hip): argument checks, the key
// packing, and the plan of a call (row slabs of bounded pair count, the fixed grid). No HIP and no DLPack types in here.
#pragma once

#include "eps_neighbors_host.hpp"

#include <cfloat>
#include <cstring>

#if defined(__HIPCC__)
#define MNN_HD __host__ __device__
#else
#define MNN_HD
#endif

namespace cuvs_amd {
namespace mnn_host {

using eps_host::check_placed;
using eps_host::refuse;
using eps_host::tensor_desc;

constexpr int kTile            = eps_host::kTile;  // the pair tile is kTile x kTile
constexpr int64_t kPairCap     = int64_t(1) << 22;  // (row tile, column tile) pairs marked, scanned and listed at a time
constexpr int kWgPerCu         = 3;                 // resident workgroups of mnn_tile_kernel per CU (164 VGPRs, 39.5 KiB of LDS)
constexpr unsigned long long kNoKey = (0x7f7fffffull << 32) | 0xffffffffull;  // FLT_MAX, id -1

// key = bits(d) << 32 | column for d >= 0 (the bits of a non-negative float ascend with its value): min over keys is the
// smallest distance, ties to the smaller column
MNN_HD inline unsigned long long pack_key(uint32_t d_bits, uint32_t col) { return ((unsigned long long)d_bits << 32) | col; }

inline bool is_f32(const tensor_desc& t) { return t.code == 2 && t.bits == 32 && t.lanes == 1; }
inline bool is_int(const tensor_desc& t, int bits) { return t.code == 0 && t.bits == bits && t.lanes == 1; }

// fp32 [rows, cols] on the device
inline void check_rows(const tensor_desc& t, const char* what, int64_t* rows, int64_t* cols)
{
  if (!t.present) refuse("%s must not be NULL", what);
  if (t.ndim != 2) refuse("%s must be a 2-D matrix", what);
  if (!is_f32(t)) refuse("%s must be fp32", what);
  check_placed(t, what);
  if (t.shape[0] < 0 || t.shape[1] < 0) refuse("%s has a negative extent", what);
  *rows = t.shape[0];
  *cols = t.shape[1];
}

// a vector of `len` elements; kind: 'f' fp32, 'i' int32, 'l' int64
inline void check_vec(const tensor_desc& t, const char* what, int64_t len, char kind, bool optional)
{
  if (!t.present) {
    if (optional) return;
    refuse("%s must not be NULL", what);
  }
  const bool ok = kind == 'f' ? is_f32(t) : is_int(t, kind == 'i' ? 32 : 64);
  if (!ok) refuse("%s must be %s", what, kind == 'f' ? "fp32" : (kind == 'i' ? "int32" : "int64"));
  if (t.ndim != 1 || t.shape[0] != len) refuse("%s must have shape [%lld]", what, (long long)len);
  check_placed(t, what);
}

struct mnn_shape {
  int64_t m = 0, n = 0, dim = 0, groups = 0;
};

inline mnn_shape check_masked_nn(const tensor_desc& x, const tensor_desc& y, const tensor_desc& xn, const tensor_desc& yn,
                                 const tensor_desc& adj, const tensor_desc& group_idxs, const tensor_desc& out_idx,
                                 const tensor_desc& out_dist)
{
  mnn_shape s;
  int64_t dim_y = 0;
  check_rows(x, "x", &s.m, &s.dim);
  check_rows(y, "y", &s.n, &dim_y);
  if (dim_y != s.dim) refuse("dim mismatch: x has %lld columns, y has %lld", (long long)s.dim, (long long)dim_y);
  if (s.n >= (int64_t(1) << 32) - 1) refuse("y has %lld rows: n must be below 2^32 - 1", (long long)s.n);
  check_vec(xn, "x_norm", s.m, 'f', true);
  check_vec(yn, "y_norm", s.n, 'f', true);
  if (!group_idxs.present) refuse("group_idxs must not be NULL");
  if (!is_int(group_idxs, 64)) refuse("group_idxs must be int64");
  if (group_idxs.ndim != 1) refuse("group_idxs must be a vector");
  check_placed(group_idxs, "group_idxs");
  s.groups = group_idxs.shape[0];
  if (!adj.present) refuse("adj must not be NULL");
  if (!(adj.bits == 8 && adj.lanes == 1 && (adj.code == 1 || adj.code == 6))) refuse("adj must be bool or uint8");
  if (adj.ndim != 2 || adj.shape[0] != s.m || adj.shape[1] != s.groups)
    refuse("adj must have shape [%lld, %lld]: one column per entry of group_idxs", (long long)s.m, (long long)s.groups);
  check_placed(adj, "adj");
  check_vec(out_idx, "out_idx", s.m, 'l', false);
  check_vec(out_dist, "out_dist", s.m, 'f', false);
  return s;
}

inline void check_cross_component(const tensor_desc& x, const tensor_desc& colors, int64_t n_components, const tensor_desc& row_idx,
                                  const tensor_desc& row_dist, const tensor_desc& src, const tensor_desc& dst, const tensor_desc& w,
                                  int64_t* n, int64_t* dim)
{
  check_rows(x, "x", n, dim);
  if (*n >= (int64_t(1) << 31)) refuse("x has %lld rows: n must be below 2^31", (long long)*n);
  check_vec(colors, "colors", *n, 'i', false);
  if (n_components < 1 || n_components >= (int64_t(1) << 31)) refuse("n_components must be in [1, 2^31): it is %lld", (long long)n_components);
  check_vec(row_idx, "row_nn_idx", *n, 'l', true);
  check_vec(row_dist, "row_nn_dist", *n, 'f', true);
  check_vec(src, "edge_src", n_components, 'l', false);
  check_vec(dst, "edge_dst", n_components, 'l', false);
  check_vec(w, "edge_weight", n_components, 'f', false);
}

// ---------------------------------------------------------------- the plan
// Row tiles are taken in slabs of at most kPairCap (row tile, column tile) pairs, so that the flags, their prefix sums and the
// pair list stay bounded whatever m x n is; a slab's pairs are numbered row-tile-major.
struct plan {
  int64_t row_tiles = 0, col_tiles = 0;
  int64_t slab_tiles = 0;  // row tiles per slab (>= 1)
  int64_t slabs      = 0;
  int64_t grid       = 0;  // workgroups of mnn_tile_kernel
};

inline plan make_plan(int64_t m, int64_t n, int64_t num_cus, int64_t pair_cap = kPairCap)
{
  plan p;
  p.row_tiles = (m + kTile - 1) / kTile;
  p.col_tiles = (n + kTile - 1) / kTile;
  if (p.row_tiles == 0 || p.col_tiles == 0) return p;
  if (p.col_tiles > pair_cap) refuse("y has %lld rows: more column tiles than a slab of pairs holds", (long long)n);
  p.slab_tiles = std::min<int64_t>(p.row_tiles, std::max<int64_t>(1, pair_cap / p.col_tiles));
  p.slabs      = (p.row_tiles + p.slab_tiles - 1) / p.slab_tiles;
  p.grid       = std::max<int64_t>(1, std::min<int64_t>(p.slab_tiles * p.col_tiles, num_cus * kWgPerCu));
  return p;
}

}  // namespace mnn_host
}  // namespace cuvs_amd
