// Spectral embedding and spectral clustering (include/cuvs_amd/spectral.h; semantics of the reference's
// cpp/src/preprocessing/spectral/detail/spectral_embedding.cuh and cpp/src/cluster/detail/spectral.cuh). DESIGN 3.1w.
//
// The reference takes its eigen-solver from RAFT (lanczos_compute_eigenpairs), whose source is not on disk; the one here is
// written from scratch: thick-restart Lanczos for the smallest eigenpairs of the graph Laplacian L (the largest of -L, as the
// reference configures it), two passes of classical Gram-Schmidt against the whole basis per step.
//
// One Lanczos step j is six launches and no host round trip:
//   spmv       w = L v_j, a sub-wave group of 8 / 16 / 32 / 64 lanes per CSR row; per-workgroup partials of v_j . w
//   dots (A)   every workgroup owns a chunk of the n axis, keeps its chunk of w in registers and streams the j + 1 basis rows
//              over it: partial[row][chunk]
//   update (B) c[row] = the partials summed in a fixed order (every workgroup sums them again: they sit in L2),
//              w -= V^T c over the same chunking; the second B also emits the partials of ||w||^2
//   A, B       once more
//   normalise  beta = sqrt(sum of the partials), v_{j+1} = w / beta; alpha_j and beta_{j+1} stay on the device
// Algorithmic bytes of a step: A and B each read the j + 1 rows once, twice over: 4 (j + 1) n 4 bytes; the vectors themselves
// (w read and written, v_{j+1} written, the CSR arrays) are the lower-order rest.
// At the end of a cycle the host reads alpha and beta (one copy), solves the projected problem in double
// (spectral_host.hpp), and the device forms the Ritz vectors X = S^T V in double, rounded once, into the second basis buffer.
// Every reduction runs in a fixed order (shuffle butterflies and sequential sums, no floating-point atomics).
#include "common.hpp"
#include "device_utils.hpp"
#include "dl_desc.hpp"
#include "ops.hpp"
#include "spectral_host.hpp"

#include <cuvs/cluster/kmeans.h>
#include <cuvs/neighbors/all_neighbors.h>
#include <cuvs_amd/spectral.h>

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <string>
#include <vector>

namespace cuvs_amd {
namespace {

namespace H = spectral_host;
using eps_host::refuse;
using eps_host::tensor_desc;

constexpr int kThreads = 256;
constexpr int kMaxE    = 8;  // elements of the n axis per thread of the re-orthogonalisation kernels
constexpr int kSpmvIts = 2;  // CSR rows per sub-wave group of the matrix-vector product (both in flight at once)
constexpr int kRowBlock = 4;  // basis rows whose loads a re-orthogonalisation thread has in flight at once
constexpr int kRitzTile = 8;
constexpr unsigned long long kNoKey = ~0ull;

thread_local uint64_t g_sp_stats[4] = {0, 0, 0, 0};

// ---------------------------------------------------------------- connectivity graph
// both directions of every (row, neighbour) entry as src << 32 | dst (the row itself included); ids outside the matrix: kNoKey
__global__ void sp_emit_knn_kernel(const int64_t* __restrict__ ids, int64_t n, int64_t k, unsigned long long* __restrict__ keys)
{
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n * k) return;
  const int64_t i = e / k, j = ids[e];
  const bool ok = j >= 0 && j < n;
  keys[2 * e]     = ok ? (((unsigned long long)i << 32) | (unsigned long long)j) : kNoKey;
  keys[2 * e + 1] = ok ? (((unsigned long long)j << 32) | (unsigned long long)i) : kNoKey;
}

// a run of equal keys has one entry (a_ij alone) or two (a_ij and a_ji, or the doubled diagonal): 0.5 (a_ij + a_ji)
__global__ void sp_graph_out_kernel(const unsigned long long* __restrict__ keys, const int* __restrict__ counts, int64_t runs,
                                    int* __restrict__ rows, int* __restrict__ cols, float* __restrict__ vals)
{
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= runs) return;
  rows[e] = (int)(keys[e] >> 32);
  cols[e] = (int)(keys[e] & 0xffffffffull);
  vals[e] = 0.5f * (float)counts[e];
}

// ---------------------------------------------------------------- COO -> CSR
// counters[0]: entries outside [0, n); counters[1]: entries left out (those and the diagonal)
__global__ void sp_coo_keys_kernel(const int* __restrict__ rows, const int* __restrict__ cols, int64_t nnz, int64_t n,
                                   unsigned long long* __restrict__ keys, uint32_t* __restrict__ counters)
{
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= nnz) return;
  const int64_t r = rows[e], c = cols[e];
  const bool inside = r >= 0 && r < n && c >= 0 && c < n;
  const bool keep   = inside && r != c;
  keys[e] = keep ? (((unsigned long long)r << 32) | (unsigned long long)c) : kNoKey;
  if (!inside) atomicAdd(counters, 1u);
  if (!keep) atomicAdd(counters + 1, 1u);
}

// offsets[r] = the first entry of row r or of a later row; thread `nnz` closes the rows behind the last entry
__global__ void sp_offsets_kernel(const unsigned long long* __restrict__ keys, int64_t nnz, int64_t n, int* __restrict__ offsets)
{
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e > nnz) return;
  const int64_t r    = e < nnz ? (int64_t)(keys[e] >> 32) : n;
  const int64_t prev = e > 0 ? (int64_t)(keys[e - 1] >> 32) : -1;
  for (int64_t rr = prev + 1; rr <= r; ++rr) offsets[rr] = (int)e;
}

// a thread per row sums its weights in entry order (duplicates stay separate entries: the products add them up)
__global__ void sp_degree_kernel(const int* __restrict__ offsets, const float* __restrict__ w, int64_t n, int norm,
                                 float* __restrict__ deg, float* __restrict__ scaling, float* __restrict__ diag)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float d = 0.f;
  for (int e = offsets[i]; e < offsets[i + 1]; ++e) d += w[e];
  deg[i] = d;
  if (norm) {
    scaling[i] = d == 0.f ? 1.f : sqrtf(d);
    diag[i]    = d == 0.f ? 0.f : 1.f;
  } else {
    scaling[i] = d;
    diag[i]    = d;
  }
}

// the off-diagonal values of L: -w / sqrt(deg_i deg_j) (one product, one root and one division round), or -w
__global__ void sp_values_kernel(const unsigned long long* __restrict__ keys, const float* __restrict__ w, int64_t nnz,
                                 const float* __restrict__ deg, int norm, int* __restrict__ col, float* __restrict__ lv)
{
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= nnz) return;
  const int64_t r = (int64_t)(keys[e] >> 32), c = (int64_t)(keys[e] & 0xffffffffull);
  col[e] = (int)c;
  if (norm) {
    const float den = sqrtf(deg[r] * deg[c]);
    lv[e] = -w[e] / (den == 0.f ? 1.f : den);
  } else {
    lv[e] = -w[e];
  }
}

// ---------------------------------------------------------------- y = L x and the partials of x . y
// G lanes per row; a workgroup takes kSpmvIts * 256 / G consecutive rows, 256 / G at a time (few rows per workgroup: a row is
// three dependent loads - offsets, entries, x - and only many rows in flight hide them). The group's lanes stride over the row's
// entries, a shuffle butterfly adds them up, the diagonal term goes last. part[blockIdx.x] = the workgroup's share of x . y.
template <int G>
__global__ __launch_bounds__(kThreads) void sp_spmv_kernel(const int* __restrict__ offsets, const int* __restrict__ col,
                                                           const float* __restrict__ lv, const float* __restrict__ diag,
                                                           const float* __restrict__ x, float* __restrict__ y, int64_t n,
                                                           float* __restrict__ part)
{
  __shared__ float s_part[kThreads / kWave];
  const int tid = threadIdx.x, sub = tid & (G - 1), grp = tid / G;
  constexpr int kGroups = kThreads / G;
  float dot = 0.f;
#pragma unroll
  for (int it = 0; it < kSpmvIts; ++it) {
    const int64_t r = (int64_t)blockIdx.x * (kSpmvIts * kGroups) + it * kGroups + grp;
    float acc = 0.f;
    if (r < n) {
      const int b = offsets[r], e = offsets[r + 1];
      for (int t = b + sub; t < e; t += G) acc = fmaf(lv[t], x[col[t]], acc);
    }
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) acc += __shfl_xor(acc, o, kWave);
    if (r < n && sub == 0) {
      const float xr = x[r];
      const float yr = fmaf(diag[r], xr, acc);
      y[r] = yr;
      dot  = fmaf(xr, yr, dot);
    }
  }
  dot = wave_sum(dot);
  if ((tid & (kWave - 1)) == 0) s_part[tid / kWave] = dot;
  __syncthreads();
  if (tid == 0) part[blockIdx.x] = ((s_part[0] + s_part[1]) + s_part[2]) + s_part[3];
}

// ---------------------------------------------------------------- re-orthogonalisation
// the sum of v[0 .. cnt) by one wave: lanes stride over it, then the butterfly (the same order whoever asks)
__device__ inline float wave_strided_sum(const float* __restrict__ v, int cnt)
{
  float a = 0.f;
  for (int t0 = threadIdx.x & (kWave - 1); t0 < cnt; t0 += 8 * kWave) {  // eight loads in flight, added in index order
    float b[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) b[q] = t0 + q * kWave < cnt ? v[t0 + q * kWave] : 0.f;
#pragma unroll
    for (int q = 0; q < 8; ++q)
      if (t0 + q * kWave < cnt) a += b[q];
  }
  return wave_sum(a);
}

// pass A: partial[row * gridDim.x + blockIdx.x] = sum over the workgroup's chunk of V[row][i] u[i]
__global__ __launch_bounds__(kThreads) void sp_dots_kernel(const float* __restrict__ V, int64_t ld, int j, const float* __restrict__ u,
                                                           int64_t n, int e_cnt, float* __restrict__ partial)
{
  __shared__ float s_part[H::kMaxNcv + 1][kThreads / kWave];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int64_t base = (int64_t)blockIdx.x * kThreads * e_cnt + tid;
  float ur[kMaxE];
#pragma unroll
  for (int r = 0; r < kMaxE; ++r) {
    const int64_t i = base + (int64_t)r * kThreads;
    ur[r] = (r < e_cnt && i < n) ? u[i] : 0.f;
  }
  for (int row0 = 0; row0 < j; row0 += kRowBlock) {  // kRowBlock rows' loads are issued before the first is used
    float p[kRowBlock];
#pragma unroll
    for (int q = 0; q < kRowBlock; ++q) p[q] = 0.f;
#pragma unroll
    for (int r = 0; r < kMaxE; ++r) {
      const int64_t i = base + (int64_t)r * kThreads;
      if (r < e_cnt && i < n) {
        float v[kRowBlock];
#pragma unroll
        for (int q = 0; q < kRowBlock; ++q) v[q] = row0 + q < j ? V[(int64_t)(row0 + q) * ld + i] : 0.f;
#pragma unroll
        for (int q = 0; q < kRowBlock; ++q) p[q] = fmaf(v[q], ur[r], p[q]);
      }
    }
#pragma unroll
    for (int q = 0; q < kRowBlock; ++q) {
      const float t = wave_sum(p[q]);
      if (lane == 0 && row0 + q < j) s_part[row0 + q][wave] = t;
    }
  }
  __syncthreads();
  for (int row = tid; row < j; row += kThreads)
    partial[(int64_t)row * gridDim.x + blockIdx.x] = ((s_part[row][0] + s_part[row][1]) + s_part[row][2]) + s_part[row][3];
}

// pass B: c[row] = sum of partial[row][*], u -= V^T c over the same chunking; norm_part (optional): the chunk's share of ||u||^2
__global__ __launch_bounds__(kThreads) void sp_update_kernel(const float* __restrict__ V, int64_t ld, int j, float* __restrict__ u,
                                                             int64_t n, int e_cnt, const float* __restrict__ partial,
                                                             float* __restrict__ norm_part)
{
  __shared__ float s_c[H::kMaxNcv + 1];
  __shared__ float s_n[kThreads / kWave];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int chunks = gridDim.x;
  for (int row = wave; row < j; row += kThreads / kWave) {
    const float c = wave_strided_sum(partial + (int64_t)row * chunks, chunks);
    if (lane == 0) s_c[row] = c;
  }
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * kThreads * e_cnt + tid;
  float ur[kMaxE];
#pragma unroll
  for (int r = 0; r < kMaxE; ++r) {
    const int64_t i = base + (int64_t)r * kThreads;
    ur[r] = (r < e_cnt && i < n) ? u[i] : 0.f;
  }
  for (int row0 = 0; row0 < j; row0 += kRowBlock) {  // (the rows are applied in ascending order, as one at a time would)
#pragma unroll
    for (int r = 0; r < kMaxE; ++r) {
      const int64_t i = base + (int64_t)r * kThreads;
      if (r < e_cnt && i < n) {
        float v[kRowBlock];
#pragma unroll
        for (int q = 0; q < kRowBlock; ++q) v[q] = row0 + q < j ? V[(int64_t)(row0 + q) * ld + i] : 0.f;
#pragma unroll
        for (int q = 0; q < kRowBlock; ++q)
          if (row0 + q < j) ur[r] = fmaf(-s_c[row0 + q], v[q], ur[r]);
      }
    }
  }
  float p = 0.f;
#pragma unroll
  for (int r = 0; r < kMaxE; ++r) {
    const int64_t i = base + (int64_t)r * kThreads;
    if (r < e_cnt && i < n) {
      u[i] = ur[r];
      p    = fmaf(ur[r], ur[r], p);
    }
  }
  if (norm_part != nullptr) {
    p = wave_sum(p);
    if (lane == 0) s_n[wave] = p;
    __syncthreads();
    if (tid == 0) norm_part[blockIdx.x] = ((s_n[0] + s_n[1]) + s_n[2]) + s_n[3];
  }
}

// beta = sqrt(sum of norm_part), out = u / beta (zero when beta is zero: no NaN leaves a collapsed step). Workgroup 0 records
// beta and - in the solver - alpha = the sum of the matrix-vector product's partials.
__global__ __launch_bounds__(kThreads) void sp_normalize_kernel(const float* __restrict__ u, int64_t n,
                                                                const float* __restrict__ norm_part, int chunks,
                                                                float* __restrict__ out, float* __restrict__ beta_slot,
                                                                const float* __restrict__ alpha_part, int alpha_cnt,
                                                                float* __restrict__ alpha_slot)
{
  __shared__ float s_sq;
  const int tid = threadIdx.x, wave = tid / kWave;
  if (wave == 0) {
    const float sq = wave_strided_sum(norm_part, chunks);
    if (tid == 0) s_sq = sq;
  } else if (wave == 1 && blockIdx.x == 0 && alpha_part != nullptr) {
    const float a = wave_strided_sum(alpha_part, alpha_cnt);
    if (tid == kWave) *alpha_slot = a;
  }
  __syncthreads();
  const float beta = sqrtf(s_sq);
  if (blockIdx.x == 0 && tid == 0 && beta_slot != nullptr) *beta_slot = beta;
  const int64_t i = (int64_t)blockIdx.x * kThreads + tid;
  if (i < n) out[i] = beta > 0.f ? u[i] / beta : 0.f;
}

__global__ void sp_hash_kernel(float* __restrict__ u, int64_t n, uint32_t fold, uint32_t salt)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) u[i] = H::hashed_uniform(fold, salt, (uint32_t)i);
}

// ---------------------------------------------------------------- Ritz vectors: out[t][i] = sum_r S[r][t] V[r][i]
// a thread per column i and kRitzTile Ritz vectors (blockIdx.y); S [m, kept] in double, the sum in double, rounded once
__global__ __launch_bounds__(kThreads) void sp_ritz_kernel(const float* __restrict__ V, int64_t ld, int m, const double* __restrict__ S,
                                                           int kept, float* __restrict__ out, int64_t n)
{
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const int t0 = blockIdx.y * kRitzTile;
  double acc[kRitzTile];
#pragma unroll
  for (int t = 0; t < kRitzTile; ++t) acc[t] = 0.0;
  for (int r = 0; r < m; ++r) {
    const double v = i < n ? (double)V[(int64_t)r * ld + i] : 0.0;
#pragma unroll
    for (int t = 0; t < kRitzTile; ++t)
      if (t0 + t < kept) acc[t] = fma(S[(int64_t)r * kept + t0 + t], v, acc[t]);
  }
  if (i >= n) return;
#pragma unroll
  for (int t = 0; t < kRitzTile; ++t)
    if (t0 + t < kept) out[(int64_t)(t0 + t) * ld + i] = (float)acc[t];
}

// ---------------------------------------------------------------- embedding
// a workgroup per output column: the entry of largest magnitude of X[c + drop][i] / scaling[i], the lowest index on ties
__global__ __launch_bounds__(kThreads) void sp_sign_kernel(const float* __restrict__ X, int64_t n, int drop,
                                                           const float* __restrict__ scaling, float* __restrict__ sign)
{
  __shared__ float s_abs[kThreads], s_val[kThreads];
  __shared__ int64_t s_idx[kThreads];
  const float* __restrict__ xr = X + (int64_t)(blockIdx.x + drop) * n;
  float best = -1.f, val = 0.f;
  int64_t idx = -1;
  for (int64_t i = threadIdx.x; i < n; i += kThreads) {
    const float v = scaling != nullptr ? xr[i] / scaling[i] : xr[i];
    if (fabsf(v) > best) { best = fabsf(v); val = v; idx = i; }  // (i ascends: a tie keeps the lower index)
  }
  s_abs[threadIdx.x] = best; s_val[threadIdx.x] = val; s_idx[threadIdx.x] = idx;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int t = 1; t < kThreads; ++t)
      if (s_idx[t] >= 0 && (s_abs[t] > best || (s_abs[t] == best && s_idx[t] < idx))) { best = s_abs[t]; val = s_val[t]; idx = s_idx[t]; }
    sign[blockIdx.x] = val < 0.f ? -1.f : 1.f;
  }
}

__global__ void sp_embed_kernel(const float* __restrict__ X, int64_t n, int drop, int c_out, const float* __restrict__ scaling,
                                const float* __restrict__ sign, float* __restrict__ out, int64_t row_stride, int64_t col_stride)
{
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * c_out) return;
  const int64_t c = t / n, i = t - c * n;  // (consecutive threads read consecutive entries of one eigenvector)
  const float v = X[(c + drop) * n + i];
  out[i * row_stride + c * col_stride] = (scaling != nullptr ? v / scaling[i] : v) * sign[c];
}

// ---------------------------------------------------------------- host side
#define SP_LAUNCH(kernel, items, ...)                                                                              \
  do {                                                                                                             \
    hipLaunchKernelGGL(kernel, dim3(grid_blocks((items), kThreads)), dim3(kThreads), 0, res.stream, __VA_ARGS__); \
    HIP_TRY(hipGetLastError());                                                                                    \
  } while (0)

template <typename Call>
void with_temp(resources& res, dev_buf<char>& temp, Call&& call)  // hipcub's two-step convention: size query, then the run
{
  size_t bytes = 0;
  HIP_TRY(call(static_cast<void*>(nullptr), bytes));
  if (bytes > temp.bytes()) temp = dev_buf<char>(res, bytes);
  bytes = std::max<size_t>(temp.bytes(), 1);
  HIP_TRY(call(static_cast<void*>(temp.data()), bytes));
}

struct dl_view {  // a DLManagedTensor describing device memory for the library's own entry points
  DLManagedTensor m{};
  int64_t shape[2];
  dl_view(void* data, uint8_t code, uint8_t bits, int64_t rows, int64_t cols, int device)
  {
    shape[0] = rows; shape[1] = cols;
    m.dl_tensor.data        = data;
    m.dl_tensor.device      = {kDLROCM, device};
    m.dl_tensor.ndim        = 2;
    m.dl_tensor.dtype       = {code, bits, 1};
    m.dl_tensor.shape       = shape;
    m.dl_tensor.strides     = nullptr;
    m.dl_tensor.byte_offset = 0;
  }
};

// ---- argument checks (every one of them before the first write to an output)
void check_dataset(const tensor_desc& x, int64_t* n, int64_t* dim)
{
  if (!x.present) refuse("dataset must not be NULL");
  if (!(x.code == 2 && x.bits == 32 && x.lanes == 1)) refuse("dataset must be fp32");
  if (!x.on_device) refuse("dataset must be accessible on device memory");
  if (x.ndim != 2 || !x.contiguous) refuse("dataset must be a row-major, contiguous matrix");
  if (x.shape[0] < 1 || x.shape[1] < 1) refuse("dataset must have at least one row and one column");
  *n   = x.shape[0];
  *dim = x.shape[1];
}

// a device vector of `code` / 32 bits; returns its length
int64_t check_vector(const tensor_desc& t, const char* what, int code)
{
  if (!t.present) refuse("%s must not be NULL", what);
  if (!(t.code == code && t.bits == 32 && t.lanes == 1)) refuse(code == 0 ? "%s must be int32" : "%s must be fp32", what);
  if (t.ndim != 1) refuse("%s must be a vector", what);
  if (t.shape[0] < 0) refuse("%s has a negative length (nnz < 0)", what);
  eps_host::check_placed(t, what);
  return t.shape[0];
}

int64_t check_coo(DLManagedTensor* rows, DLManagedTensor* cols, DLManagedTensor* vals, int64_t n)
{
  if (n < 1 || n >= (int64_t(1) << 31)) refuse("n must be in [1, 2^31); got %lld", (long long)n);
  const int64_t nnz = check_vector(desc_of(rows), "rows", 0);
  if (check_vector(desc_of(cols), "cols", 0) != nnz || check_vector(desc_of(vals), "vals", 2) != nnz)
    refuse("rows, cols and vals must have one length");
  if (nnz >= (int64_t(1) << 31)) refuse("nnz must be below 2^31; got %lld", (long long)nnz);
  return nnz;
}

void check_components(int n_components, bool drop_first, int64_t n)
{
  if (n_components < 1) refuse("n_components must be at least 1; got %d", n_components);
  if (n_components >= n) refuse("n_components must be below n: got %d with n = %lld", n_components, (long long)n);
  if (drop_first && n_components < 2) refuse("drop_first needs n_components >= 2");
}

void check_neighbors(int n_neighbors, int64_t n)
{
  if (n_neighbors < 1 || n_neighbors >= n) refuse("n_neighbors must be in [1, n): got %d with n = %lld", n_neighbors, (long long)n);
  if (2 * n * (int64_t)n_neighbors >= (int64_t(1) << 31))
    refuse("the connectivity graph holds up to %lld entries; fewer than 2^31 are supported", (long long)(2 * n * n_neighbors));
}

struct embedding_out {
  float* ptr;
  int64_t row_stride, col_stride;
};

embedding_out check_embedding(DLManagedTensor* e, int64_t n, int c_out)
{
  if (e == nullptr) refuse("embedding must not be NULL");
  const DLTensor& t = e->dl_tensor;
  if (!dtype_is(t.dtype, kDLFloat, 32)) refuse("embedding must be fp32");
  if (!is_device_accessible(t)) refuse("embedding must be accessible on device memory");
  if (t.ndim != 2 || t.shape[0] != n || t.shape[1] != c_out) refuse("embedding must have shape [%lld, %d]", (long long)n, c_out);
  if (is_c_contiguous(t)) return {static_cast<float*>(dl_data(t)), (int64_t)c_out, 1};
  if (is_f_contiguous(t)) return {static_cast<float*>(dl_data(t)), 1, n};
  refuse("embedding must be row-major or column-major without gaps");
}

void check_eigenvalues(DLManagedTensor* ev, int k)
{
  if (ev == nullptr) return;
  const DLTensor& t = ev->dl_tensor;
  if (!dtype_is(t.dtype, kDLFloat, 32)) refuse("eigenvalues must be fp32");
  if (t.ndim != 1 || t.shape[0] != k) refuse("eigenvalues must have shape [%d]", k);
  if (!is_device_accessible(t) && !is_host_accessible(t)) refuse("eigenvalues must be on the host or the device");
}

// ---- the operator
struct sp_operator {
  int64_t n = 0, nnz = 0;
  bool norm = false;
  int group = 8;
  double scale = 0.0;  // bounds ||L||_inf
  dev_buf<int> offsets, col;
  dev_buf<float> lv, diag, scaling;
};

sp_operator build_operator(resources& res, const int* rows, const int* cols, const float* vals, int64_t nnz, int64_t n, bool norm)
{
  sp_operator op;
  op.n = n; op.norm = norm;
  profile_begin(res, "sp_laplacian");
  dev_buf<unsigned long long> keys(res, (size_t)nnz), keys2(res, (size_t)nnz);
  dev_buf<float> w2(res, (size_t)nnz);
  dev_buf<uint32_t> counters(res, 2);
  dev_buf<char> temp;
  HIP_TRY(hipMemsetAsync(counters.data(), 0, counters.bytes(), res.stream));
  uint32_t outside = 0, dropped = 0;
  if (nnz > 0) {
    SP_LAUNCH(sp_coo_keys_kernel, nnz, rows, cols, nnz, n, keys.data(), counters.data());
    outside = read_word(res, counters.data());
    dropped = read_word(res, counters.data() + 1);
    if (outside != 0) refuse("%u entries of the graph lie outside [0, n)", outside);
    // (a stable sort: duplicates keep their input order, and with it the order in which they are added)
    with_temp(res, temp, [&](void* t, size_t& b) {
      return hipcub::DeviceRadixSort::SortPairs(t, b, keys.data(), keys2.data(), vals, w2.data(), (int)nnz, 0, 64, res.stream);
    });
  }
  op.nnz     = nnz - dropped;
  op.offsets = dev_buf<int>(res, (size_t)n + 1);
  op.col     = dev_buf<int>(res, (size_t)std::max<int64_t>(op.nnz, 1));
  op.lv      = dev_buf<float>(res, (size_t)std::max<int64_t>(op.nnz, 1));
  op.diag    = dev_buf<float>(res, (size_t)n);
  op.scaling = dev_buf<float>(res, (size_t)n);
  dev_buf<float> deg(res, (size_t)n);
  SP_LAUNCH(sp_offsets_kernel, op.nnz + 1, keys2.data(), op.nnz, n, op.offsets.data());
  SP_LAUNCH(sp_degree_kernel, n, op.offsets.data(), w2.data(), n, (int)norm, deg.data(), op.scaling.data(), op.diag.data());
  if (op.nnz > 0) SP_LAUNCH(sp_values_kernel, op.nnz, keys2.data(), w2.data(), op.nnz, deg.data(), (int)norm, op.col.data(), op.lv.data());
  if (norm) {
    op.scale = 2.0;
  } else {
    const std::vector<float> h = to_host(res, deg.data(), (size_t)n);
    op.scale = 2.0 * (double)*std::max_element(h.begin(), h.end());
  }
  const double mean = (double)op.nnz / (double)n;
  op.group = mean <= 12.0 ? 8 : (mean <= 24.0 ? 16 : (mean <= 48.0 ? 32 : 64));
  profile_end(res, "sp_laplacian");
  sync(res);  // (the scratch arrays go away)
  return op;
}

int spmv_blocks(int64_t n, int group) { return (int)grid_blocks(n, kSpmvIts * kThreads / group); }

void spmv(resources& res, const sp_operator& op, const float* x, float* y, float* part)
{
  const dim3 grid(spmv_blocks(op.n, op.group)), block(kThreads);
#define SP_SPMV(G) \
  hipLaunchKernelGGL(sp_spmv_kernel<G>, grid, block, 0, res.stream, op.offsets.data(), op.col.data(), op.lv.data(), op.diag.data(), x, y, op.n, part)
  switch (op.group) {
    case 8: SP_SPMV(8); break;
    case 16: SP_SPMV(16); break;
    case 32: SP_SPMV(32); break;
    default: SP_SPMV(64); break;
  }
#undef SP_SPMV
  HIP_TRY(hipGetLastError());
}

// ---- the re-orthogonalisation
struct ortho_plan {
  int e_cnt, chunks;
};

ortho_plan plan_ortho(int64_t n)
{
  int e = 1;
  while (e < kMaxE && (n + (int64_t)kThreads * e - 1) / ((int64_t)kThreads * e) > 1024) e *= 2;
  return {e, (int)grid_blocks(n, kThreads * e)};
}

// u (in place) against the first j rows of V, twice; then out = u / ||u||. partial holds j * chunks floats, norm_part chunks.
void orthogonalize(resources& res, const float* V, int64_t ld, int j, float* u, int64_t n, const ortho_plan& pl, float* partial,
                   float* norm_part, float* out, float* beta_slot, const float* alpha_part, int alpha_cnt, float* alpha_slot)
{
  const dim3 grid(pl.chunks), block(kThreads);
  for (int pass = 0; pass < 2; ++pass) {
    if (j > 0) hipLaunchKernelGGL(sp_dots_kernel, grid, block, 0, res.stream, V, ld, j, (const float*)u, n, pl.e_cnt, partial);
    hipLaunchKernelGGL(sp_update_kernel, grid, block, 0, res.stream, V, ld, j, u, n, pl.e_cnt, (const float*)partial,
                       pass == 1 ? norm_part : nullptr);
  }
  hipLaunchKernelGGL(sp_normalize_kernel, dim3(grid_blocks(n, kThreads)), block, 0, res.stream, (const float*)u, n,
                     (const float*)norm_part, pl.chunks, out, beta_slot, alpha_part, alpha_cnt, alpha_slot);
  HIP_TRY(hipGetLastError());
}

// ---- the solver
struct sp_eigen {
  dev_buf<float> x;  // [k, n]
  std::vector<float> values;
};

sp_eigen solve(resources& res, const sp_operator& op, int k, int ncv, float tolerance, uint64_t seed)
{
  const int64_t n = op.n;
  if (k < 1 || k >= n) refuse("the number of eigenpairs must be in [1, n): got %d with n = %lld", k, (long long)n);
  const int64_t rule = H::ncv_rule(n, k);
  const int64_t m64  = ncv == 0 ? rule : ncv;
  if (m64 <= k || m64 > n || m64 > H::kMaxNcv)
    refuse("ncv must be above k and at most min(n, %d): got %lld with k = %d, n = %lld", H::kMaxNcv, (long long)m64, k, (long long)n);
  const int m = (int)m64;
  uint64_t* st = g_sp_stats;
  st[0] = st[1] = st[3] = 0;
  st[2] = (uint64_t)m;

  const ortho_plan pl = plan_ortho(n);
  const int sblocks   = spmv_blocks(n, op.group);
  dev_buf<float> va(res, (size_t)(m + 1) * n), vb(res, (size_t)(m + 1) * n), w(res, (size_t)n);
  dev_buf<float> ab(res, (size_t)(2 * m + 1));  // alpha [m], then beta [m + 1]
  dev_buf<float> partial(res, (size_t)(m + 1) * pl.chunks), norm_part(res, (size_t)pl.chunks), spart(res, (size_t)sblocks);
  dev_buf<double> s_dev(res, (size_t)m * k);
  float* V  = va.data();
  float* V2 = vb.data();
  const uint32_t fold = H::seed_fold(seed);
  const double collapse = H::collapse_threshold(op.scale);
  const int64_t cap = 10 * n;

  profile_begin(res, "sp_lanczos");
  SP_LAUNCH(sp_hash_kernel, n, w.data(), n, fold, 0u);
  orthogonalize(res, V, n, 0, w.data(), n, pl, partial.data(), norm_part.data(), V, nullptr, nullptr, 0, nullptr);

  int locked = 0;
  uint32_t rescues = 0;
  int64_t matvecs = 0;
  std::vector<double> theta, arrow, alpha((size_t)m), beta((size_t)m + 1);
  H::cycle c;
  for (;;) {
    const int m_end = (int)std::min<int64_t>(m, locked + (cap - matvecs));
    HIP_TRY(hipMemsetAsync(ab.data(), 0, ab.bytes(), res.stream));
    for (int j = locked; j < m_end; ++j) {
      spmv(res, op, V + (int64_t)j * n, w.data(), spart.data());
      orthogonalize(res, V, n, j + 1, w.data(), n, pl, partial.data(), norm_part.data(), V + (int64_t)(j + 1) * n,
                    ab.data() + m + j + 1, spart.data(), sblocks, ab.data() + j);
    }
    matvecs += m_end - locked;
    const std::vector<float> h = to_host(res, ab.data(), (size_t)(2 * m + 1));  // the cycle's one round trip
    for (int j = 0; j < m; ++j) alpha[(size_t)j] = (double)h[(size_t)j];
    for (int j = 0; j <= m; ++j) beta[(size_t)j] = (double)h[(size_t)(m + j)];
    c = H::end_of_cycle(n, k, locked, m_end, theta.data(), arrow.data(), alpha.data(), beta.data(), (double)tolerance, collapse);
    copy_async(res, s_dev.data(), c.s.data(), c.s.size() * sizeof(double));
    hipLaunchKernelGGL(sp_ritz_kernel, dim3(grid_blocks(n, kThreads), (c.kept + kRitzTile - 1) / kRitzTile), dim3(kThreads), 0,
                       res.stream, (const float*)V, n, c.m_eff, (const double*)s_dev.data(), c.kept, V2, n);
    HIP_TRY(hipGetLastError());
    const bool last = c.converged || matvecs >= cap;
    if (last) break;
    if (c.collapsed) {  // the Krylov space is exhausted: go on from a fresh pseudo-random vector, orthogonal to what is kept
      rescues += 1;
      SP_LAUNCH(sp_hash_kernel, n, w.data(), n, fold, rescues);
      orthogonalize(res, V2, n, c.kept, w.data(), n, pl, partial.data(), norm_part.data(), V2 + (int64_t)c.kept * n, nullptr,
                    nullptr, 0, nullptr);
    } else {
      copy_async(res, V2 + (int64_t)c.kept * n, V + (int64_t)c.m_eff * n, (size_t)n * sizeof(float));
    }
    std::swap(V, V2);
    theta  = c.theta;
    arrow  = c.arrow;
    locked = c.kept;
    st[1] += 1;
  }
  sync(res);
  profile_end(res, "sp_lanczos");
  st[0] = (uint64_t)matvecs;
  st[3] = c.converged ? 1 : 0;
  if (c.kept != k) CUVS_FAIL("the eigen-solver holds %d of the %d eigenpairs asked for", c.kept, k);
  sp_eigen out;
  out.values.assign(c.theta.begin(), c.theta.end());
  if (V2 == vb.data()) {
    out.x = std::move(vb);
  } else {
    out.x = std::move(va);
  }
  return out;
}

void write_eigenvalues(resources& res, DLManagedTensor* ev, const std::vector<float>& values)
{
  if (ev == nullptr) return;
  copy_async(res, dl_data(ev->dl_tensor), values.data(), values.size() * sizeof(float));
  sync(res);
}

// eigenvectors -> the embedding: the degree scaling, the dropped column, the sign rule
void write_embedding(resources& res, const sp_operator& op, const sp_eigen& eig, int n_components, bool drop_first, const embedding_out& out)
{
  const int drop = drop_first ? 1 : 0, c_out = n_components - drop;
  const float* scaling = op.norm ? op.scaling.data() : nullptr;
  dev_buf<float> sign(res, (size_t)c_out);
  hipLaunchKernelGGL(sp_sign_kernel, dim3(c_out), dim3(kThreads), 0, res.stream, (const float*)eig.x.data(), op.n, drop, scaling, sign.data());
  SP_LAUNCH(sp_embed_kernel, op.n * c_out, (const float*)eig.x.data(), op.n, drop, c_out, scaling, (const float*)sign.data(), out.ptr,
            out.row_stride, out.col_stride);
}

struct coo_dev {
  dev_buf<int> rows, cols;
  dev_buf<float> vals;
  int64_t nnz = 0;
};

// the connectivity graph of a device dataset into buffers of capacity 2 n k; returns the entries written
int64_t connectivity_graph(cuvsResources_t res_h, resources& res, DLManagedTensor* dataset, int64_t n, int k, int* rows, int* cols,
                           float* vals)
{
  const int64_t cap = 2 * n * k;
  profile_begin(res, "sp_knn");
  dev_buf<int64_t> ids(res, (size_t)(n * k));
  {
    dl_view ids_t(ids.data(), kDLInt, 64, n, k, res.device);
    cuvsAllNeighborsIndexParams an{CUVS_ALL_NEIGHBORS_ALGO_BRUTE_FORCE, 1, 1, L2SqrtExpanded, nullptr, nullptr};
    if (cuvsAllNeighborsBuild(res_h, &an, dataset, &ids_t.m, nullptr, nullptr, 1.0f) != CUVS_SUCCESS)
      CUVS_FAIL("cuvsAllNeighborsBuild: %s", last_error_text().c_str());
  }
  profile_end(res, "sp_knn");
  profile_begin(res, "sp_symmetrise");
  dev_buf<unsigned long long> keys(res, (size_t)cap), sorted(res, (size_t)cap);
  dev_buf<int> counts(res, (size_t)cap);
  dev_buf<uint32_t> runs(res, 1);
  dev_buf<char> temp;
  SP_LAUNCH(sp_emit_knn_kernel, n * k, ids.data(), n, (int64_t)k, keys.data());
  with_temp(res, temp, [&](void* t, size_t& b) {
    return hipcub::DeviceRadixSort::SortKeys(t, b, keys.data(), sorted.data(), (int)cap, 0, 64, res.stream);
  });
  with_temp(res, temp, [&](void* t, size_t& b) {
    return hipcub::DeviceRunLengthEncode::Encode(t, b, sorted.data(), keys.data(), counts.data(), runs.data(), (int)cap, res.stream);
  });
  int64_t nnz = read_word(res, runs.data());
  if (nnz > 0 && to_host(res, keys.data() + nnz - 1, 1)[0] == kNoKey) --nnz;  // the run of ids outside the matrix
  if (nnz > 0) SP_LAUNCH(sp_graph_out_kernel, nnz, keys.data(), counts.data(), nnz, rows, cols, vals);
  profile_end(res, "sp_symmetrise");
  sync(res);
  return nnz;
}

coo_dev connectivity_graph(cuvsResources_t res_h, resources& res, DLManagedTensor* dataset, int64_t n, int k)
{
  coo_dev g;
  g.rows = dev_buf<int>(res, (size_t)(2 * n * k));
  g.cols = dev_buf<int>(res, (size_t)(2 * n * k));
  g.vals = dev_buf<float>(res, (size_t)(2 * n * k));
  g.nnz  = connectivity_graph(res_h, res, dataset, n, k, g.rows.data(), g.cols.data(), g.vals.data());
  return g;
}

void transform(resources& res, const cuvsAmdSpectralEmbeddingParams& p, const int* rows, const int* cols, const float* vals, int64_t nnz,
               int64_t n, const embedding_out& out, DLManagedTensor* eigenvalues)
{
  const sp_operator op = build_operator(res, rows, cols, vals, nnz, n, p.norm_laplacian);
  const sp_eigen eig   = solve(res, op, p.n_components, 0, p.tolerance, p.seed);
  write_embedding(res, op, eig, p.n_components, p.drop_first, out);
  write_eigenvalues(res, eigenvalues, eig.values);
  sync(res);
}

void check_clustering(const cuvsAmdSpectralClusteringParams* p, int64_t n, DLManagedTensor* labels)
{
  if (p == nullptr) refuse("params must not be NULL");
  if (p->n_clusters < 1 || p->n_clusters > n) refuse("n_clusters must be in [1, n]: got %d with n = %lld", p->n_clusters, (long long)n);
  check_components(p->n_components, false, n);
  if (p->n_init < 1) refuse("n_init must be at least 1; got %d", p->n_init);
  if (check_vector(desc_of(labels), "labels", 0) != n) refuse("labels must have shape [%lld]", (long long)n);
}

void fit_predict(resources& res, const cuvsAmdSpectralClusteringParams& p, const int* rows, const int* cols, const float* vals, int64_t nnz,
                 int64_t n, DLManagedTensor* labels)
{
  const int nc = p.n_components;
  dev_buf<float> emb(res, (size_t)n * nc), centroids(res, (size_t)p.n_clusters * nc);
  const cuvsAmdSpectralEmbeddingParams ep{nc, p.n_neighbors, true, false, p.tolerance, p.seed};
  transform(res, ep, rows, cols, vals, nnz, n, embedding_out{emb.data(), (int64_t)nc, 1}, nullptr);
  // the non-hierarchical Lloyd fit of cuvsKMeansFit with the library's defaults (max_iter 300, tol 1e-4), k-means++ seeding
  const lloyd_params lp{p.n_clusters, (int)KMeansPlusPlus, 300, 1e-4, p.n_init, p.seed};
  double inertia = 0.0;
  int n_iter     = 0;
  lloyd_fit(res, emb.data(), n, nc, nullptr, lp, centroids.data(), &inertia, &n_iter);
  kmeans_predict<float>(res, emb.data(), n, nc, centroids.data(), p.n_clusters, static_cast<uint32_t*>(dl_data(labels->dl_tensor)));
  sync(res);
}

}  // namespace
}  // namespace cuvs_amd

using namespace cuvs_amd;

extern "C" {

cuvsError_t cuvsAmdSpectralEmbeddingParamsCreate(cuvsAmdSpectralEmbeddingParams_t* params)
{
  return (cuvsError_t)translate_exceptions([=] {
    CUVS_EXPECTS(params != nullptr, "params is null");
    *params = new cuvsAmdSpectralEmbeddingParams{2, 15, true, true, 1e-5f, 0};
  });
}

cuvsError_t cuvsAmdSpectralEmbeddingParamsDestroy(cuvsAmdSpectralEmbeddingParams_t params)
{
  return (cuvsError_t)translate_exceptions([=] { delete params; });
}

cuvsError_t cuvsAmdSpectralClusteringParamsCreate(cuvsAmdSpectralClusteringParams_t* params)
{
  return (cuvsError_t)translate_exceptions([=] {
    CUVS_EXPECTS(params != nullptr, "params is null");
    *params = new cuvsAmdSpectralClusteringParams{8, 8, 10, 15, 1e-5f, 0};
  });
}

cuvsError_t cuvsAmdSpectralClusteringParamsDestroy(cuvsAmdSpectralClusteringParams_t params)
{
  return (cuvsError_t)translate_exceptions([=] { delete params; });
}

cuvsError_t cuvsAmdSpectralConnectivityGraph(cuvsResources_t res_h, cuvsAmdSpectralEmbeddingParams_t params, DLManagedTensor* dataset,
                                             DLManagedTensor* rows, DLManagedTensor* cols, DLManagedTensor* vals, int64_t* nnz)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& res = *as_res(res_h);
    if (params == nullptr || nnz == nullptr) refuse("params and nnz must not be NULL");
    int64_t n = 0, dim = 0;
    check_dataset(desc_of(dataset), &n, &dim);
    check_neighbors(params->n_neighbors, n);
    const int64_t cap = 2 * n * params->n_neighbors;
    if (check_vector(desc_of(rows), "rows", 0) < cap || check_vector(desc_of(cols), "cols", 0) < cap ||
        check_vector(desc_of(vals), "vals", 2) < cap)
      refuse("rows, cols and vals must hold at least 2 n n_neighbors = %lld entries", (long long)cap);
    *nnz = connectivity_graph(res_h, res, dataset, n, params->n_neighbors, static_cast<int*>(dl_data(rows->dl_tensor)),
                              static_cast<int*>(dl_data(cols->dl_tensor)), static_cast<float*>(dl_data(vals->dl_tensor)));
  });
}

cuvsError_t cuvsAmdSpectralEmbeddingTransform(cuvsResources_t res_h, cuvsAmdSpectralEmbeddingParams_t params, DLManagedTensor* dataset,
                                              DLManagedTensor* embedding, DLManagedTensor* eigenvalues)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& res = *as_res(res_h);
    if (params == nullptr) refuse("params must not be NULL");
    int64_t n = 0, dim = 0;
    check_dataset(desc_of(dataset), &n, &dim);
    check_components(params->n_components, params->drop_first, n);
    check_neighbors(params->n_neighbors, n);
    const embedding_out out = check_embedding(embedding, n, params->n_components - (params->drop_first ? 1 : 0));
    check_eigenvalues(eigenvalues, params->n_components);
    const coo_dev g = connectivity_graph(res_h, res, dataset, n, params->n_neighbors);
    transform(res, *params, g.rows.data(), g.cols.data(), g.vals.data(), g.nnz, n, out, eigenvalues);
  });
}

cuvsError_t cuvsAmdSpectralEmbeddingTransformGraph(cuvsResources_t res_h, cuvsAmdSpectralEmbeddingParams_t params, DLManagedTensor* rows,
                                                   DLManagedTensor* cols, DLManagedTensor* vals, int64_t n, DLManagedTensor* embedding,
                                                   DLManagedTensor* eigenvalues)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& res = *as_res(res_h);
    if (params == nullptr) refuse("params must not be NULL");
    const int64_t nnz = check_coo(rows, cols, vals, n);
    check_components(params->n_components, params->drop_first, n);
    const embedding_out out = check_embedding(embedding, n, params->n_components - (params->drop_first ? 1 : 0));
    check_eigenvalues(eigenvalues, params->n_components);
    transform(res, *params, static_cast<const int*>(dl_data(rows->dl_tensor)), static_cast<const int*>(dl_data(cols->dl_tensor)),
              static_cast<const float*>(dl_data(vals->dl_tensor)), nnz, n, out, eigenvalues);
  });
}

cuvsError_t cuvsAmdSpectralClusteringFitPredict(cuvsResources_t res_h, cuvsAmdSpectralClusteringParams_t params, DLManagedTensor* dataset,
                                                DLManagedTensor* labels)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& res = *as_res(res_h);
    int64_t n = 0, dim = 0;
    check_dataset(desc_of(dataset), &n, &dim);
    check_clustering(params, n, labels);
    check_neighbors(params->n_neighbors, n);
    const coo_dev g = connectivity_graph(res_h, res, dataset, n, params->n_neighbors);
    fit_predict(res, *params, g.rows.data(), g.cols.data(), g.vals.data(), g.nnz, n, labels);
  });
}

cuvsError_t cuvsAmdSpectralClusteringFitPredictGraph(cuvsResources_t res_h, cuvsAmdSpectralClusteringParams_t params, DLManagedTensor* rows,
                                                     DLManagedTensor* cols, DLManagedTensor* vals, int64_t n, DLManagedTensor* labels)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& res = *as_res(res_h);
    const int64_t nnz = check_coo(rows, cols, vals, n);
    check_clustering(params, n, labels);
    fit_predict(res, *params, static_cast<const int*>(dl_data(rows->dl_tensor)), static_cast<const int*>(dl_data(cols->dl_tensor)),
                static_cast<const float*>(dl_data(vals->dl_tensor)), nnz, n, labels);
  });
}

cuvsError_t cuvsAmdSpectralEigsh(cuvsResources_t res_h, DLManagedTensor* rows, DLManagedTensor* cols, DLManagedTensor* vals, int64_t n,
                                 bool norm_laplacian, int k, int ncv, float tolerance, uint64_t seed, DLManagedTensor* eigenvalues,
                                 DLManagedTensor* eigenvectors)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& res = *as_res(res_h);
    const int64_t nnz = check_coo(rows, cols, vals, n);
    if (k < 1 || k >= n) refuse("k must be in [1, n): got %d with n = %lld", k, (long long)n);
    check_eigenvalues(eigenvalues, k);
    const tensor_desc x = desc_of(eigenvectors);
    if (!x.present || !(x.code == 2 && x.bits == 32 && x.lanes == 1) || x.ndim != 2 || x.shape[0] != k || x.shape[1] != n)
      refuse("eigenvectors must be fp32 [%d, %lld]", k, (long long)n);
    eps_host::check_placed(x, "eigenvectors");
    const sp_operator op = build_operator(res, static_cast<const int*>(dl_data(rows->dl_tensor)),
                                          static_cast<const int*>(dl_data(cols->dl_tensor)),
                                          static_cast<const float*>(dl_data(vals->dl_tensor)), nnz, n, norm_laplacian);
    const sp_eigen eig = solve(res, op, k, ncv, tolerance, seed);
    copy_async(res, dl_data(eigenvectors->dl_tensor), eig.x.data(), (size_t)k * n * sizeof(float));
    write_eigenvalues(res, eigenvalues, eig.values);
    sync(res);
  });
}

cuvsError_t cuvsAmdSpectralLaplacianMatvec(cuvsResources_t res_h, DLManagedTensor* rows, DLManagedTensor* cols, DLManagedTensor* vals,
                                           int64_t n, bool norm_laplacian, DLManagedTensor* x, DLManagedTensor* y, DLManagedTensor* diag_out)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& res = *as_res(res_h);
    const int64_t nnz = check_coo(rows, cols, vals, n);
    if (check_vector(desc_of(x), "x", 2) != n || check_vector(desc_of(y), "y", 2) != n) refuse("x and y must have shape [n]");
    if (diag_out != nullptr && check_vector(desc_of(diag_out), "diag_out", 2) != n) refuse("diag_out must have shape [n]");
    const sp_operator op = build_operator(res, static_cast<const int*>(dl_data(rows->dl_tensor)),
                                          static_cast<const int*>(dl_data(cols->dl_tensor)),
                                          static_cast<const float*>(dl_data(vals->dl_tensor)), nnz, n, norm_laplacian);
    dev_buf<float> part(res, (size_t)spmv_blocks(n, op.group));
    spmv(res, op, static_cast<const float*>(dl_data(x->dl_tensor)), static_cast<float*>(dl_data(y->dl_tensor)), part.data());
    if (diag_out != nullptr) copy_async(res, dl_data(diag_out->dl_tensor), op.scaling.data(), (size_t)n * sizeof(float));
    sync(res);
  });
}

cuvsError_t cuvsAmdSpectralOrthogonalize(cuvsResources_t res_h, DLManagedTensor* V, DLManagedTensor* u, float* norm_out)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& res = *as_res(res_h);
    const tensor_desc v = desc_of(V);
    if (!v.present || !(v.code == 2 && v.bits == 32 && v.lanes == 1) || v.ndim != 2) refuse("V must be an fp32 matrix [j, n]");
    eps_host::check_placed(v, "V");
    const int64_t j = v.shape[0], n = v.shape[1];
    if (j < 0 || j > H::kMaxNcv) refuse("V must have at most %d rows; got %lld", H::kMaxNcv, (long long)j);
    if (n < 1 || check_vector(desc_of(u), "u", 2) != n) refuse("u must have shape [n] with n >= 1");
    const ortho_plan pl = plan_ortho(n);
    dev_buf<float> partial(res, (size_t)std::max<int64_t>(j, 1) * pl.chunks), norm_part(res, (size_t)pl.chunks), beta(res, 1), out(res, (size_t)n);
    float* up = static_cast<float*>(dl_data(u->dl_tensor));
    orthogonalize(res, static_cast<const float*>(dl_data(V->dl_tensor)), n, (int)j, up, n, pl, partial.data(), norm_part.data(), out.data(),
                  beta.data(), nullptr, 0, nullptr);
    copy_async(res, up, out.data(), (size_t)n * sizeof(float));
    const float h = to_host(res, beta.data(), 1)[0];
    if (norm_out != nullptr) *norm_out = h;
  });
}

cuvsError_t cuvsAmdSpectralLastStats(uint64_t out[4])
{
  return (cuvsError_t)translate_exceptions([=] {
    CUVS_EXPECTS(out != nullptr, "out is null");
    for (int i = 0; i < 4; ++i) out[i] = g_sp_stats[i];
  });
}

}  // extern "C"
