// Host-only parts of the epsilon-neighbourhood search (eps_neighbors.hip): argument checks, CSR offsets from degrees, the
// max_k truncation and the row-slab size. No HIP and no DLPack types in here: tests/cpp/eps_neighbors_host_test.cpp builds
// this header alone under the sanitizers.
#pragma once

#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include <string>

namespace cuvs_amd {
namespace eps_host {

constexpr int kTile = 128;  // the pair tile is kTile x kTile

[[noreturn]] inline void refuse(const char* fmt, ...)
{
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  throw std::invalid_argument(buf);
}

// what the checks need to know of a DLTensor
struct tensor_desc {
  bool present    = false;  // the pointer was not NULL
  int ndim        = 0;
  int64_t shape[2] = {0, 0};
  bool contiguous = true;   // row-major without gaps
  bool on_device  = true;
  int code        = 2;      // DLPack type code: 0 int, 1 uint, 2 float, 6 bool
  int bits        = 32;
  int lanes       = 1;
};

enum class rows_t : int { f32 = 0, f16 = 1 };

inline void check_metric(int metric)
{
  if (metric != 4)  // L2Unexpanded
    refuse("Currently only L2Unexpanded distance metric is supported. Other metrics will be supported in future versions.");
}

inline void check_placed(const tensor_desc& t, const char* what)
{
  if (!t.on_device) refuse("%s must be accessible on device memory", what);
  if (!t.contiguous) refuse("%s must be row-major and contiguous", what);
}

// x [m, dim], y [n, dim]: fp32 or fp16, the same type
inline rows_t check_rows(const tensor_desc& x, const tensor_desc& y, int64_t* m, int64_t* n, int64_t* dim)
{
  if (!x.present || !y.present) refuse("x and y must not be NULL");
  if (x.ndim != 2 || y.ndim != 2) refuse("x and y must be 2-D matrices");
  if (x.code == 2 && x.bits == 64) refuse("fp64 rows are not supported: x and y must be fp32 or fp16");
  if (y.code == 2 && y.bits == 64) refuse("fp64 rows are not supported: x and y must be fp32 or fp16");
  if (x.code != y.code || x.bits != y.bits || x.lanes != y.lanes)
    refuse("x and y must have the same dtype (mixed dtypes are not supported)");
  if (!(x.code == 2 && x.lanes == 1 && (x.bits == 32 || x.bits == 16))) refuse("x and y must be fp32 or fp16");
  if (x.shape[0] < 0 || y.shape[0] < 0 || x.shape[1] < 0) refuse("negative extent");
  if (x.shape[1] != y.shape[1])
    refuse("dim mismatch: x has %lld columns, y has %lld", (long long)x.shape[1], (long long)y.shape[1]);
  check_placed(x, "x");
  check_placed(y, "y");
  *m   = x.shape[0];
  *n   = y.shape[0];
  *dim = x.shape[1];
  return x.bits == 32 ? rows_t::f32 : rows_t::f16;
}

// adj: bool / uint8 [m, n]
inline void check_adj(const tensor_desc& adj, int64_t m, int64_t n)
{
  if (!adj.present) return;
  const bool byte = adj.bits == 8 && adj.lanes == 1 && (adj.code == 1 || adj.code == 6);
  if (!byte) refuse("adj must be bool or uint8");
  if (adj.ndim != 2 || adj.shape[0] != m || adj.shape[1] != n)
    refuse("adj must have shape [%lld, %lld]", (long long)m, (long long)n);
  check_placed(adj, "adj");
}

// a vector of m + 1 integers (vd, indptr); returns the element size
inline int check_row_vector(const tensor_desc& v, int64_t m, const char* what, bool allow_int32, int64_t n)
{
  if (!v.present) return 0;
  const bool i64 = v.code == 0 && v.bits == 64 && v.lanes == 1;
  const bool i32 = v.code == 0 && v.bits == 32 && v.lanes == 1;
  if (!(i64 || (allow_int32 && i32))) refuse(allow_int32 ? "%s must be int32 or int64" : "%s must be int64", what);
  if (v.ndim != 1 || v.shape[0] != m + 1) refuse("%s must have shape [%lld] (m + 1)", what, (long long)(m + 1));
  check_placed(v, what);
  if (i32 && (m != 0 && n != 0) && (m > (INT64_MAX / n) || m * n >= (int64_t(1) << 31)))
    refuse("%s must be int64 when m * n >= 2^31 (int32 degrees could overflow)", what);
  return i64 ? 8 : 4;
}

// indices int64 [len], distances fp32 [len]; returns len
inline int64_t check_list(const tensor_desc& v, const char* what, bool f32)
{
  const bool ok = f32 ? (v.code == 2 && v.bits == 32 && v.lanes == 1) : (v.code == 0 && v.bits == 64 && v.lanes == 1);
  if (!ok) refuse(f32 ? "%s must be fp32" : "%s must be int64", what);
  if (v.ndim != 1) refuse("%s must be a vector", what);
  check_placed(v, what);
  return v.shape[0];
}

// rows of a list a row keeps: all of them without a cap
inline int64_t kept(int64_t degree, int64_t max_k) { return max_k < 0 ? degree : std::min(degree, max_k); }

// offsets[i] = carry + sum over r < i of kept(degrees[r]) for i in [0, rows]; returns offsets[rows] (the next carry). max_k < 0:
// no cap. `offsets` holds rows + 1 values.
inline int64_t offsets_from_counts(const int64_t* degrees, int64_t rows, int64_t max_k, int64_t carry, int64_t* offsets)
{
  int64_t run = carry;
  for (int64_t i = 0; i < rows; ++i) {
    offsets[i] = run;
    run += kept(degrees[i], max_k);
  }
  offsets[rows] = run;
  return run;
}

inline int64_t largest_degree(const int64_t* degrees, int64_t rows)
{
  int64_t best = 0;
  for (int64_t i = 0; i < rows; ++i) best = std::max(best, degrees[i]);
  return best;
}

// a fill call: indptr as the caller passed it (host copy), the length of its list buffers
inline void check_fill(const int64_t* indptr, int64_t m, int64_t indices_len, int64_t distances_len, bool has_distances)
{
  if (indptr[0] < 0) refuse("indptr[0] is negative");
  for (int64_t i = 0; i < m; ++i)
    if (indptr[i + 1] < indptr[i]) refuse("indptr is not ascending at row %lld", (long long)i);
  const int64_t nnz = indptr[m];
  if (indices_len < nnz) refuse("indices holds %lld entries but indptr[m] is %lld", (long long)indices_len, (long long)nnz);
  if (has_distances && distances_len < nnz)
    refuse("distances holds %lld entries but indptr[m] is %lld", (long long)distances_len, (long long)nnz);
}

// the one-call form: indices holds m * max_k
inline void check_max_k(int64_t max_k, int64_t m, int64_t indices_len, int64_t distances_len, bool has_distances)
{
  if (max_k < 0) refuse("max_k must not be negative");
  if (m != 0 && max_k > INT64_MAX / std::max<int64_t>(m, 1)) refuse("m * max_k overflows");
  if (indices_len < m * max_k)
    refuse("indices holds %lld entries but m * max_k is %lld", (long long)indices_len, (long long)(m * max_k));
  if (has_distances && distances_len < m * max_k)
    refuse("distances holds %lld entries but m * max_k is %lld", (long long)distances_len, (long long)(m * max_k));
}

// workspace of one slab row: the bit mask (16 bytes per column tile), the tile counts (1 byte each), the degree (8 bytes)
inline int64_t slab_row_bytes(int64_t n)
{
  const int64_t tiles = (n + kTile - 1) / kTile;
  return tiles * 17 + 8;
}

// rows per slab: as many as the budget holds, a multiple of the tile (at least one tile) unless `forced` (> 0) asks for fewer
inline int64_t slab_rows(int64_t m, int64_t n, int64_t budget_bytes, int64_t forced)
{
  if (m <= 0) return 0;
  if (forced > 0) return std::min(m, forced);
  int64_t rows = budget_bytes / std::max<int64_t>(slab_row_bytes(n), 1);
  rows         = std::max<int64_t>(rows / kTile * kTile, kTile);
  return std::min(m, rows);
}

}  // namespace eps_host
}  // namespace cuvs_amd
