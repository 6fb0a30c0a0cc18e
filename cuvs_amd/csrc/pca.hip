// PCA (drop-in for c/src/preprocessing/pca.cpp; the reference forwards to raft::linalg::pca_*, which is not in its tree, so the
// semantics are the ones written out in include/cuvs/preprocessing/pca.h).
//
//   fit        mean (fp64 partial sums over fixed row chunks) -> covariance (fp32 matrix cores, centred while staging, every
//              fp32 chain flushed into fp64 after kChain rows, row ranges combined in fp64 in a fixed order) -> parallel cyclic
//              Jacobi on the d x d fp64 matrix in device memory -> eigenvalue order and the k-vectors on the host (d numbers)
//              -> components with their sign on the device
//   transform / inverse transform   one kernel: a tall operand in either layout times a small [K, N] matrix, no split over K,
//              accumulation from 0 in ascending K on v_mfma_f32_32x32x2_f32, which is bit for bit the chain
//              acc = fmaf(a_k, w_k, acc)
//
// Both matrix kernels share one tile shape: a workgroup of four waves owns a 64 x 64 output tile (32 x 32 per wave) and
// stages kKT steps of K for both operands in LDS as [k][i], so that a lane's operand of the 32x32x2 instruction
// (A[i = lane & 31][k = lane >> 5]) is one conflict-free word. Operands are described by two strides, which is all that
// separates row-major from column-major inputs; the staging picks the thread mapping whose global reads are contiguous.
//
// Determinism: the number and extent of the mean chunks and of the covariance row ranges depend on (n, d) alone, partial
// results are added in index order, the Jacobi schedule is fixed, and the only atomics are integer counters and maxima.
// The same input gives the same bits on every run and every CU count, and for either input layout.
#include "common.hpp"

#include <cuvs/preprocessing/pca.h>
#include <cuvs_amd/extensions.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <numeric>
#include <vector>

namespace cuvs_amd {
namespace {

constexpr int kTile     = 64;         // output tile edge of a workgroup
constexpr int kKT       = 64;         // K steps staged at a time
constexpr int kPad      = kTile + 1;  // LDS row pitch in words: a column of the staged tile falls on 32 different banks
constexpr int kChain    = 8192;       // longest fp32 accumulation chain of the covariance
constexpr int kMaxCols  = 4096;
constexpr int kDqSweeps = 30;         // COV_EIG_DQ's cap on sweeps (a converging run needs 6 to 10)
constexpr double kEps32 = 1.1920928955078125e-07;

using f32x16 = __attribute__((ext_vector_type(16))) float;

// element (kk, i) of a matrix operand is p[kk * sk + i * si], minus sub[kk] or sub[i] when sub is set
struct operand {
  const float* p;
  int64_t sk, si;
  const float* sub;
  int sub_on_k;
};

// s[kk][i] = operand(k0 + kk, i0 + i) for kk < kKT, i < kTile; 0 outside [0, kmax) x [0, imax)
__device__ inline void pca_stage(float (*s)[kPad], const operand& o, int64_t k0, int64_t kmax, int64_t i0, int64_t imax)
{
  const int t = threadIdx.x;
  if (o.si == 1) {
    const int i      = t & 63;
    const int64_t gi = i0 + i;
#pragma unroll 4
    for (int kk = t >> 6; kk < kKT; kk += 4) {
      const int64_t gk = k0 + kk;
      float v          = 0.f;
      if (gk < kmax && gi < imax) {
        v = o.p[gk * o.sk + gi];
        if (o.sub) v = v - o.sub[o.sub_on_k ? gk : gi];
      }
      s[kk][i] = v;
    }
  } else {
    const int kk     = t & 63;
    const int64_t gk = k0 + kk;
#pragma unroll 4
    for (int i = t >> 6; i < kTile; i += 4) {
      const int64_t gi = i0 + i;
      float v          = 0.f;
      if (gk < kmax && gi < imax) {
        v = o.p[gk * o.sk + gi * o.si];
        if (o.sub) v = v - o.sub[o.sub_on_k ? gk : gi];
      }
      s[kk][i] = v;
    }
  }
}

// one staged K block through the matrix core: the wave's 32 x 32 tile at (wi, wj) of the workgroup's 64 x 64
__device__ inline f32x16 pca_mfma_block(const float (*sA)[kPad], const float (*sB)[kPad], int wi, int wj, f32x16 acc)
{
  const int lane = threadIdx.x & 63, h = lane >> 5, c = lane & 31;
#pragma unroll 8
  for (int kk = 0; kk < kKT; kk += 2) {
    const float a = sA[kk + h][wi * 32 + c];
    const float b = sB[kk + h][wj * 32 + c];
    acc           = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
  }
  return acc;
}
// row of accumulator register `reg` inside the wave's 32 x 32 tile (its column is lane & 31)
__device__ inline int pca_acc_row(int reg) { return (reg & 3) + 8 * (reg >> 2) + 4 * ((threadIdx.x & 63) >> 5); }

// ---------------------------------------------------------------- mean
// partial[chunk][col]: fp64 sum of the chunk's rows. A thread (q, col) adds rows 16 q .. 16 q + 15 of each staged 64-row
// block in order, the four q are combined in order at the end: the order does not depend on the layout of x.
__global__ __launch_bounds__(256) void pca_colsum_kernel(operand x, int64_t n, int d, int64_t chunk_rows, double* __restrict__ partial)
{
  __shared__ float s[kKT][kPad];
  __shared__ double red[4][kTile];
  const int t = threadIdx.x, q = t >> 6, c = t & 63;
  const int64_t c0 = (int64_t)blockIdx.x * kTile;
  const int64_t r0 = (int64_t)blockIdx.y * chunk_rows, r1 = r0 + chunk_rows < n ? r0 + chunk_rows : n;
  double acc = 0.0;
  for (int64_t k0 = r0; k0 < r1; k0 += kKT) {
    pca_stage(s, x, k0, r1, c0, d);
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 16; ++r) acc += (double)s[q * 16 + r][c];
    __syncthreads();
  }
  red[q][c] = acc;
  __syncthreads();
  if (q == 0 && c0 + c < d) partial[(int64_t)blockIdx.y * d + c0 + c] = ((red[0][c] + red[1][c]) + red[2][c]) + red[3][c];
}

__global__ void pca_mean_kernel(const double* __restrict__ partial, int n_chunks, int d, int64_t n, float* __restrict__ mu)
{
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= d) return;
  double s = 0.0;
  for (int c = 0; c < n_chunks; ++c) s += partial[(int64_t)c * d + j];
  mu[j] = (float)(s / (double)n);
}

// ---------------------------------------------------------------- covariance
// workgroup (pair, split): the 64 x 64 tile (ti <= tj) of sum over the split's rows of (x - mu)(x - mu)^T, as fp64
__global__ __launch_bounds__(256) void pca_cov_kernel(operand x, int64_t n, int d, int n_tiles, int64_t split_rows,
                                                      double* __restrict__ partial)
{
  __shared__ float sA[kKT][kPad], sB[kKT][kPad];
  int p = blockIdx.x, ti = 0;
  while (p >= n_tiles - ti) { p -= n_tiles - ti; ++ti; }
  const int tj = ti + p;
  const int wave = threadIdx.x >> 6, wi = wave >> 1, wj = wave & 1;
  const int64_t r0 = (int64_t)blockIdx.y * split_rows, r1 = r0 + split_rows < n ? r0 + split_rows : n;
  const float (*pB)[kPad] = ti == tj ? sA : sB;
  f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  double wide[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) wide[r] = 0.0;
  int in_chain = 0;
  for (int64_t k0 = r0; k0 < r1; k0 += kKT) {
    pca_stage(sA, x, k0, r1, (int64_t)ti * kTile, d);
    if (ti != tj) pca_stage(sB, x, k0, r1, (int64_t)tj * kTile, d);
    __syncthreads();
    acc = pca_mfma_block(sA, pB, wi, wj, acc);
    __syncthreads();
    in_chain += kKT;
    if (in_chain >= kChain) {
#pragma unroll
      for (int r = 0; r < 16; ++r) { wide[r] += (double)acc[r]; acc[r] = 0.f; }
      in_chain = 0;
    }
  }
  double* out = partial + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * (kTile * kTile);
#pragma unroll
  for (int r = 0; r < 16; ++r)
    out[(wi * 32 + pca_acc_row(r)) * kTile + wj * 32 + (threadIdx.x & 31)] = wide[r] + (double)acc[r];
}

// C[i][j] = C[j][i] = (sum of the splits in index order) / (n - 1)
__global__ __launch_bounds__(256) void pca_cov_reduce_kernel(const double* __restrict__ partial, int n_pairs, int n_splits, int n_tiles,
                                                             int d, int64_t n, double* __restrict__ cov)
{
  int p = blockIdx.x, ti = 0;
  while (p >= n_tiles - ti) { p -= n_tiles - ti; ++ti; }
  const int tj = ti + p;
  const int e = blockIdx.y * 256 + threadIdx.x, a = e >> 6, b = e & 63;
  const int gi = ti * kTile + a, gj = tj * kTile + b;
  if (gi >= d || gj >= d || (ti == tj && a > b)) return;
  double s = 0.0;
  for (int sp = 0; sp < n_splits; ++sp) s += partial[((int64_t)sp * n_pairs + blockIdx.x) * (kTile * kTile) + e];
  s /= (double)(n - 1);
  cov[(int64_t)gi * d + gj] = s;
  cov[(int64_t)gj * d + gi] = s;
}

// ---------------------------------------------------------------- Jacobi
// Round r of a sweep over m = d rounded up to even players pairs them by the circle method: m / 2 disjoint (p, q), every pair
// once in m - 1 rounds. A pair with q >= d (odd d) is a bye.
__device__ inline void pca_pair(int r, int idx, int m, int& p, int& q)
{
  int a, b;
  if (idx == 0) { a = r; b = m - 1; }
  else { a = (r + idx) % (m - 1); b = (r - idx + (m - 1)) % (m - 1); }
  p = a < b ? a : b;
  q = a < b ? b : a;
}

__global__ void pca_identity_kernel(double* __restrict__ v, int d)
{
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < (int64_t)d * d) v[t] = (t / d == t % d) ? 1.0 : 0.0;
}

// (c, s) of every pair of round r; stats[0] counts the rotations of the sweep, stats[1] keeps the largest
// |a_pq| / sqrt(a_pp a_qq) met (as the bits of a non-negative float)
__global__ void pca_jacobi_angles_kernel(const double* __restrict__ a, int d, int m, int r, double2* __restrict__ cs,
                                         unsigned* __restrict__ stats)
{
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= m / 2) return;
  int p, q;
  pca_pair(r, idx, m, p, q);
  double c = 1.0, s = 0.0;
  if (q < d) {
    const double app = a[(int64_t)p * d + p], aqq = a[(int64_t)q * d + q], apq = a[(int64_t)p * d + q];
    const double lim = sqrt(fabs(app * aqq));
    if (apq != 0.0 && fabs(apq) > kEps32 * lim) {
      const double theta = (aqq - app) / (2.0 * apq);
      const double tt    = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));
      c = 1.0 / sqrt(tt * tt + 1.0);
      s = tt * c;
      const double ratio = lim > 0.0 ? fabs(apq) / lim : (double)FLT_MAX;
      atomicAdd(&stats[0], 1u);
      atomicMax(&stats[1], __float_as_uint((float)(ratio < (double)FLT_MAX ? ratio : (double)FLT_MAX)));
    }
  }
  cs[idx] = make_double2(c, s);
}

// A <- J^T A J and Vt <- J^T Vt for the round's rotations J. Thread (i, u): for u < m / 2 the 2 x 2 block of A at rows
// (p_i, q_i), columns (p_u, q_u), u >= i, and its mirror image, which nobody else reads or writes: in place. For
// u >= m / 2 column u - m / 2 of rows (p_i, q_i) of Vt (row e of Vt is eigenvector e).
__global__ __launch_bounds__(256) void pca_jacobi_apply_kernel(double* __restrict__ a, double* __restrict__ vt, int d, int m, int r,
                                                               const double2* __restrict__ cs)
{
  const int i = blockIdx.y, u = blockIdx.x * blockDim.x + threadIdx.x, half = m / 2;
  if (u >= half + d) return;
  int pi, qi;
  pca_pair(r, i, m, pi, qi);
  const double2 ri = cs[i];
  const double ci = ri.x, si = ri.y;
  const bool has_qi = qi < d;
  if (u >= half) {
    if (si == 0.0) return;
    const int col   = u - half;
    const double vp = vt[(int64_t)pi * d + col], vq = vt[(int64_t)qi * d + col];
    vt[(int64_t)pi * d + col] = ci * vp - si * vq;
    vt[(int64_t)qi * d + col] = si * vp + ci * vq;
    return;
  }
  if (u < i) return;
  int pj, qj;
  pca_pair(r, u, m, pj, qj);
  const double2 rj = cs[u];
  const double cj = rj.x, sj = rj.y;
  if (si == 0.0 && sj == 0.0) return;
  const bool has_qj = qj < d;
  const double m00 = a[(int64_t)pi * d + pj];
  const double m01 = has_qj ? a[(int64_t)pi * d + qj] : 0.0;
  const double m10 = has_qi ? a[(int64_t)qi * d + pj] : 0.0;
  const double m11 = has_qi && has_qj ? a[(int64_t)qi * d + qj] : 0.0;
  const double t00 = cj * m00 - sj * m01, t01 = sj * m00 + cj * m01;
  const double t10 = cj * m10 - sj * m11, t11 = sj * m10 + cj * m11;
  double b00 = ci * t00 - si * t10, b01 = ci * t01 - si * t11;
  double b10 = si * t00 + ci * t10, b11 = si * t01 + ci * t11;
  if (u == i) { b01 = 0.0; b10 = 0.0; }  // the rotated pair's own off-diagonal entry: zero by construction
  a[(int64_t)pi * d + pj] = b00;
  a[(int64_t)pj * d + pi] = b00;
  if (has_qj) { a[(int64_t)pi * d + qj] = b01; a[(int64_t)qj * d + pi] = b01; }
  if (has_qi) { a[(int64_t)qi * d + pj] = b10; a[(int64_t)pj * d + qi] = b10; }
  if (has_qi && has_qj) { a[(int64_t)qi * d + qj] = b11; a[(int64_t)qj * d + qi] = b11; }
}

__global__ void pca_diag_kernel(const double* __restrict__ a, int d, double* __restrict__ diag)
{
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < d) diag[j] = a[(int64_t)j * d + j];
}

// ---------------------------------------------------------------- components and signs
// workgroup i: components[i] = row order[i] of vt as fp32; with v_sign the entry of largest magnitude (lowest index on a tie)
// is made positive
__global__ __launch_bounds__(256) void pca_components_kernel(const double* __restrict__ vt, const int* __restrict__ order, int d,
                                                             int v_sign, float* __restrict__ out, int64_t so_i, int64_t so_j)
{
  __shared__ unsigned long long best[256];
  const int i = blockIdx.x, t = threadIdx.x;
  const double* row = vt + (int64_t)order[i] * d;
  unsigned long long key = 0;  // |v| bits, then the lower index, then the sign
  for (int j = t; j < d; j += 256) {
    const unsigned bits = __float_as_uint((float)row[j]);
    const unsigned long long k2 =
      ((unsigned long long)(bits & 0x7fffffffu) << 32) | ((unsigned long long)(0x7fffffffu - (unsigned)j) << 1) | (bits >> 31);
    key = k2 > key ? k2 : key;
  }
  best[t] = key;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) best[t] = best[t + w] > best[t] ? best[t + w] : best[t];
    __syncthreads();
  }
  const bool flip = v_sign && (best[0] >> 32) != 0 && (best[0] & 1);
  for (int j = t; j < d; j += 256) {
    const float v = (float)row[j];
    out[i * so_i + j * so_j] = flip ? -v : v;
  }
}

// keys[col] = max over the rows of (|t| bits, lower row first, sign) of t [rows, k] row-major; row0 is the first row's index
__global__ __launch_bounds__(256) void pca_col_absargmax_kernel(const float* __restrict__ tmat, int64_t rows, int k, int64_t row0,
                                                                unsigned long long* __restrict__ keys)
{
  const int col = blockIdx.x * 64 + (threadIdx.x & 63);
  if (col >= k) return;
  const int64_t rb = (int64_t)blockIdx.y * 1024, re = rb + 1024 < rows ? rb + 1024 : rows;
  unsigned long long key = 0;
  for (int64_t r = rb + (threadIdx.x >> 6); r < re; r += 4) {
    const unsigned bits = __float_as_uint(tmat[r * k + col]);
    const unsigned long long k2 = ((unsigned long long)(bits & 0x7fffffffu) << 32) |
                                  ((unsigned long long)(0x7fffffffu - (unsigned)(row0 + r)) << 1) | (bits >> 31);
    key = k2 > key ? k2 : key;
  }
  atomicMax(&keys[col], key);
}

__global__ void pca_flip_rows_kernel(float* __restrict__ comp, int k, int d, int64_t so_i, int64_t so_j,
                                     const unsigned long long* __restrict__ keys)
{
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)k * d) return;
  const int i = (int)(t / d), j = (int)(t % d);
  if ((keys[i] >> 32) != 0 && (keys[i] & 1)) comp[i * so_i + j * so_j] = -comp[i * so_i + j * so_j];
}

// ---------------------------------------------------------------- projections
// w [K, N] row-major for the projection kernel: the transform's is components^T (K = d, N = k), the inverse's components
// (K = k, N = d), row i of components times its whitening scale as one fp32 multiplication
__global__ void pca_prepare_w_kernel(const float* __restrict__ comp, int64_t sc_i, int64_t sc_j, int k, int d,
                                     const float* __restrict__ sv, int whiten, int inverse, float sqrt_nm1, float* __restrict__ w)
{
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)k * d) return;
  const int i = (int)(t / d), j = (int)(t % d);
  float v = comp[i * sc_i + j * sc_j];
  if (whiten) {
    const float s     = sv[i];
    const float scale = inverse ? s / sqrt_nm1 : (s == 0.f ? 0.f : sqrt_nm1 / s);
    v                 = v * scale;
  }
  w[inverse ? (int64_t)i * d + j : (int64_t)j * k + i] = v;
}

// out[r][j] = sum over kk ascending of a(kk, r) b(kk, j), plus add[j]; a's centring happens while it is staged
__global__ __launch_bounds__(256) void pca_project_kernel(operand a, operand b, int64_t rows, int n_out, int kdim,
                                                          float* __restrict__ out, int64_t so_r, int64_t so_c,
                                                          const float* __restrict__ add)
{
  __shared__ float sA[kKT][kPad], sB[kKT][kPad];
  const int wave = threadIdx.x >> 6, wi = wave >> 1, wj = wave & 1;
  const int64_t r0 = (int64_t)blockIdx.x * kTile;
  const int64_t j0 = (int64_t)blockIdx.y * kTile;
  f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < kdim; k0 += kKT) {
    pca_stage(sA, a, k0, kdim, r0, rows);
    pca_stage(sB, b, k0, kdim, j0, n_out);
    __syncthreads();
    acc = pca_mfma_block(sA, sB, wi, wj, acc);
    __syncthreads();
  }
  if (so_r == 1 && so_c != 1) {
    // column-major output: the tile goes through LDS as [column][row] so that a store instruction runs along the rows
#pragma unroll
    for (int r = 0; r < 16; ++r) sA[wj * 32 + (threadIdx.x & 31)][wi * 32 + pca_acc_row(r)] = acc[r];
    __syncthreads();
    const int64_t row = r0 + (threadIdx.x & 63);
    if (row >= rows) return;
    for (int c = threadIdx.x >> 6; c < kTile; c += 4) {
      const int64_t col = j0 + c;
      if (col >= n_out) break;
      const float v = sA[c][threadIdx.x & 63];
      out[row + col * so_c] = add ? v + add[col] : v;
    }
    return;
  }
  const int64_t col = j0 + wj * 32 + (threadIdx.x & 31);
  if (col >= n_out) return;
  const float plus = add ? add[col] : 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t row = r0 + wi * 32 + pca_acc_row(r);
    if (row < rows) out[row * so_r + col * so_c] = add ? acc[r] + plus : acc[r];
  }
}

// ---------------------------------------------------------------- host side
struct pca_mat {
  float* p;
  int64_t rows, cols;
  bool col_major;
  int64_t sr() const { return col_major ? 1 : cols; }
  int64_t sc() const { return col_major ? rows : 1; }
};

void pca_check_common(DLManagedTensor* t, const char* what)
{
  CUVS_EXPECTS(t != nullptr, "pca: %s is null", what);
  const DLTensor& d = t->dl_tensor;
  CUVS_EXPECTS(is_device_accessible(d), "pca: %s must be in device memory (host-only tensors are not supported)", what);
  CUVS_EXPECTS(dtype_is(d.dtype, kDLFloat, 32), "pca: %s must be float32 (dtype code %d, %d bits given)", what, (int)d.dtype.code,
               (int)d.dtype.bits);
}

pca_mat pca_matrix(DLManagedTensor* t, const char* what, int64_t rows, int64_t cols)
{
  pca_check_common(t, what);
  const DLTensor& d = t->dl_tensor;
  CUVS_EXPECTS(d.ndim == 2, "pca: %s must be a 2-D matrix", what);
  CUVS_EXPECTS(rows < 0 || (d.shape[0] == rows && d.shape[1] == cols), "pca: %s must be [%lld, %lld] but is [%lld, %lld]", what,
               (long long)rows, (long long)cols, (long long)d.shape[0], (long long)d.shape[1]);
  const bool c = is_c_contiguous(d), f = is_f_contiguous(d);
  CUVS_EXPECTS(c || f, "pca: %s must be column-major (Fortran-contiguous) or row-major (C-contiguous); other strides are not supported",
               what);
  return pca_mat{static_cast<float*>(dl_data(d)), d.shape[0], d.shape[1], !c};
}

float* pca_vector(DLManagedTensor* t, const char* what, int64_t len, bool scalar_ok = false)
{
  pca_check_common(t, what);
  const DLTensor& d = t->dl_tensor;
  if (scalar_ok && d.ndim == 0) return static_cast<float*>(dl_data(d));
  CUVS_EXPECTS(d.ndim == 1, "pca: %s must be a 1-D vector", what);
  CUVS_EXPECTS(d.shape[0] == len, "pca: %s must have %lld elements but has %lld", what, (long long)len, (long long)d.shape[0]);
  CUVS_EXPECTS(d.strides == nullptr || len == 1 || d.strides[0] == 1, "pca: %s must be contiguous", what);
  return static_cast<float*>(dl_data(d));
}

void pca_check_dims(const cuvsPcaParams* params, int64_t n, int64_t d)
{
  const int64_t k = params->n_components;
  CUVS_EXPECTS(d >= 1 && d <= kMaxCols, "pca: the number of columns must be in [1, %d] but is %lld", kMaxCols, (long long)d);
  CUVS_EXPECTS(k >= 1 && k <= d, "pca: n_components must be in [1, n_cols = %lld] but is %lld", (long long)d, (long long)k);
  CUVS_EXPECTS(n >= 2, "pca: at least 2 rows are needed but there are %lld", (long long)n);
  CUVS_EXPECTS(n < (int64_t(1) << 31), "pca: at most 2^31 - 1 rows are supported but there are %lld", (long long)n);
}

thread_local int pca_last_sweeps = 0;

struct fit_args {
  pca_mat x, comp;
  float *ev, *evr, *sv, *mu, *noise;
  int k;
  bool u_sign;
};

void pca_launch_project(resources& res, const operand& a, const operand& b, int64_t rows, int n_out, int kdim, float* out, int64_t so_r,
                        int64_t so_c, const float* add)
{
  const int64_t row_tiles = (rows + kTile - 1) / kTile;
  CUVS_EXPECTS(row_tiles < (int64_t(1) << 31), "pca: too many rows for one launch");
  profile_begin(res, "pca_project_kernel");
  hipLaunchKernelGGL(pca_project_kernel, dim3((unsigned)row_tiles, (unsigned)ceil_div(n_out, kTile)), dim3(256), 0, res.stream, a, b, rows,
                     n_out, kdim, out, so_r, so_c, add);
  profile_end(res, "pca_project_kernel");
  HIP_TRY(hipGetLastError());
}

void pca_transform_impl(resources& res, const cuvsPcaParams* params, const pca_mat& x, const pca_mat& comp, const float* sv, const float* mu,
                        const pca_mat& out)
{
  const int d = (int)x.cols, k = (int)comp.rows;
  dev_buf<float> w(res, (size_t)d * k);
  hipLaunchKernelGGL(pca_prepare_w_kernel, dim3(grid_blocks((int64_t)d * k, 256)), dim3(256), 0, res.stream, comp.p, comp.sr(), comp.sc(), k, d,
                     sv, params->whiten ? 1 : 0, 0, sqrtf((float)(x.rows - 1)), w.data());
  HIP_TRY(hipGetLastError());
  pca_launch_project(res, operand{x.p, x.sc(), x.sr(), mu, 1}, operand{w.data(), k, 1, nullptr, 0}, x.rows, k, d, out.p, out.sr(), out.sc(),
                     nullptr);
}

void pca_inverse_impl(resources& res, const cuvsPcaParams* params, const pca_mat& t, const pca_mat& comp, const float* sv, const float* mu,
                      const pca_mat& out)
{
  const int d = (int)comp.cols, k = (int)comp.rows;
  dev_buf<float> w(res, (size_t)d * k);
  hipLaunchKernelGGL(pca_prepare_w_kernel, dim3(grid_blocks((int64_t)d * k, 256)), dim3(256), 0, res.stream, comp.p, comp.sr(), comp.sc(), k, d,
                     sv, params->whiten ? 1 : 0, 1, sqrtf((float)(t.rows - 1)), w.data());
  HIP_TRY(hipGetLastError());
  pca_launch_project(res, operand{t.p, t.sc(), t.sr(), nullptr, 0}, operand{w.data(), d, 1, nullptr, 0}, t.rows, d, k, out.p, out.sr(),
                     out.sc(), mu);
}

// the symmetric eigenproblem of cov (destroyed: its diagonal ends up as the eigenvalues), vt's rows the eigenvectors
int pca_jacobi(resources& res, const cuvsPcaParams* params, double* cov, double* vt, int d)
{
  const bool bounded   = params->algorithm == CUVS_PCA_COV_EIG_JACOBI;
  const int max_sweeps = bounded ? params->n_iterations : kDqSweeps;
  const int m = (d + 1) / 2 * 2, half = m / 2;
  hipLaunchKernelGGL(pca_identity_kernel, dim3(grid_blocks((int64_t)d * d, 256)), dim3(256), 0, res.stream, vt, d);
  HIP_TRY(hipGetLastError());
  if (d == 1) return 0;
  dev_buf<double2> cs(res, (size_t)half);
  dev_buf<unsigned> stats(res, 2);  // cleared before every sweep, read after it
  int sweeps = 0;
  profile_begin(res, "pca_jacobi");
  while (sweeps < max_sweeps) {
    unsigned* st = stats.data();
    HIP_TRY(hipMemsetAsync(st, 0, stats.bytes(), res.stream));
    for (int r = 0; r < m - 1; ++r) {
      hipLaunchKernelGGL(pca_jacobi_angles_kernel, dim3(ceil_div(half, 128)), dim3(128), 0, res.stream, cov, d, m, r, cs.data(), st);
      hipLaunchKernelGGL(pca_jacobi_apply_kernel, dim3(ceil_div(half + d, 256), half), dim3(256), 0, res.stream, cov, vt, d, m, r, cs.data());
    }
    HIP_TRY(hipGetLastError());
    ++sweeps;
    // the one readback of the sweep: how many pairs it rotated and the largest relative off-diagonal entry it met
    const std::vector<unsigned> h = to_host(res, st, 2);
    float ratio;
    memcpy(&ratio, &h[1], sizeof(float));
    if (h[0] == 0) { --sweeps; break; }  // nothing rotated: this sweep only looked
    if (bounded && params->tol > 0.f && ratio <= params->tol) break;
  }
  profile_end(res, "pca_jacobi");
  return sweeps;
}

void pca_fit_impl(resources& res, const cuvsPcaParams* params, const fit_args& f)
{
  const int64_t n = f.x.rows;
  const int d = (int)f.x.cols, k = f.k;
  const operand xo{f.x.p, f.x.sr(), f.x.sc(), nullptr, 0};  // (kk = row, i = column)

  // mean: chunk extents from n alone, at most 1024 of them
  const int64_t chunk_rows = std::max<int64_t>(4096, round_up((n + 1023) / 1024, kKT));
  const int n_chunks       = ceil_div(n, chunk_rows);
  {
    dev_buf<double> part(res, (size_t)n_chunks * d);
    profile_begin(res, "pca_colsum_kernel");
    hipLaunchKernelGGL(pca_colsum_kernel, dim3(ceil_div(d, kTile), n_chunks), dim3(256), 0, res.stream, xo, n, d, chunk_rows, part.data());
    profile_end(res, "pca_colsum_kernel");
    hipLaunchKernelGGL(pca_mean_kernel, dim3(ceil_div(d, 256)), dim3(256), 0, res.stream, part.data(), n_chunks, d, n, f.mu);
    HIP_TRY(hipGetLastError());
  }

  // covariance: row ranges from (n, d) alone; about 2048 workgroups, at most 256 ranges, at least 1024 rows each
  const int n_tiles = ceil_div(d, kTile), n_pairs = n_tiles * (n_tiles + 1) / 2;
  const int want_splits    = std::min(256, std::max(1, ceil_div(2048, n_pairs)));
  const int64_t split_rows = std::max<int64_t>(1024, round_up((n + want_splits - 1) / want_splits, kKT));
  const int n_splits       = ceil_div(n, split_rows);
  dev_buf<double> cov(res, (size_t)d * d), vt(res, (size_t)d * d);
  {
    dev_buf<double> part(res, (size_t)n_splits * n_pairs * kTile * kTile);
    operand xc = xo;
    xc.sub = f.mu;
    xc.sub_on_k = 0;
    profile_begin(res, "pca_cov_kernel");
    hipLaunchKernelGGL(pca_cov_kernel, dim3(n_pairs, n_splits), dim3(256), 0, res.stream, xc, n, d, n_tiles, split_rows, part.data());
    profile_end(res, "pca_cov_kernel");
    hipLaunchKernelGGL(pca_cov_reduce_kernel, dim3(n_pairs, kTile * kTile / 256), dim3(256), 0, res.stream, part.data(), n_pairs, n_splits,
                       n_tiles, d, n, cov.data());
    HIP_TRY(hipGetLastError());
  }

  pca_last_sweeps = pca_jacobi(res, params, cov.data(), vt.data(), d);

  // eigenvalues in descending order (the lower index first among equals) and the k-vectors: d numbers on the host
  dev_buf<double> diag(res, (size_t)d);
  hipLaunchKernelGGL(pca_diag_kernel, dim3(ceil_div(d, 256)), dim3(256), 0, res.stream, cov.data(), d, diag.data());
  HIP_TRY(hipGetLastError());
  const std::vector<double> lam = to_host(res, diag.data(), (size_t)d);
  std::vector<int> order((size_t)d);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return lam[(size_t)a] > lam[(size_t)b]; });
  double trace = 0.0, rest = 0.0;
  for (int j = 0; j < d; ++j) trace += lam[(size_t)order[(size_t)j]];
  for (int j = k; j < d; ++j) rest += lam[(size_t)order[(size_t)j]];
  std::vector<float> vecs((size_t)3 * k + 1);
  for (int i = 0; i < k; ++i) {
    const double l = std::max(lam[(size_t)order[(size_t)i]], 0.0);
    vecs[(size_t)i]         = (float)l;
    vecs[(size_t)k + i]     = (float)(trace > 0.0 ? l / trace : 0.0);
    vecs[(size_t)2 * k + i] = (float)std::sqrt(l * (double)(n - 1));
  }
  vecs[(size_t)3 * k] = d > k ? (float)(rest / (double)(d - k)) : 0.f;
  dev_buf<int> d_order(res, (size_t)k);
  copy_async(res, d_order.data(), order.data(), (size_t)k * sizeof(int));
  copy_async(res, f.ev, vecs.data(), (size_t)k * sizeof(float));
  copy_async(res, f.evr, vecs.data() + k, (size_t)k * sizeof(float));
  copy_async(res, f.sv, vecs.data() + 2 * k, (size_t)k * sizeof(float));
  copy_async(res, f.noise, vecs.data() + 3 * k, sizeof(float));
  hipLaunchKernelGGL(pca_components_kernel, dim3(k), dim3(256), 0, res.stream, vt.data(), d_order.data(), d, f.u_sign ? 0 : 1, f.comp.p,
                     f.comp.sr(), f.comp.sc());
  HIP_TRY(hipGetLastError());

  if (f.u_sign) {
    // column abs-argmax of (x - mu) components^T, a bounded block of rows at a time
    dev_buf<unsigned long long> keys(res, (size_t)k);
    HIP_TRY(hipMemsetAsync(keys.data(), 0, keys.bytes(), res.stream));
    const int64_t block_rows = std::min<int64_t>(n, std::max<int64_t>(1024, (int64_t(16) << 20) / k / 1024 * 1024));
    dev_buf<float> w(res, (size_t)d * k), t(res, (size_t)block_rows * k);
    hipLaunchKernelGGL(pca_prepare_w_kernel, dim3(grid_blocks((int64_t)d * k, 256)), dim3(256), 0, res.stream, f.comp.p, f.comp.sr(),
                       f.comp.sc(), k, d, f.sv, 0, 0, 1.f, w.data());
    for (int64_t r0 = 0; r0 < n; r0 += block_rows) {
      const int64_t rows = std::min(block_rows, n - r0);
      pca_launch_project(res, operand{f.x.p + r0 * f.x.sr(), f.x.sc(), f.x.sr(), f.mu, 1}, operand{w.data(), k, 1, nullptr, 0}, rows, k, d,
                         t.data(), k, 1, nullptr);
      hipLaunchKernelGGL(pca_col_absargmax_kernel, dim3(ceil_div(k, 64), ceil_div(rows, 1024)), dim3(256), 0, res.stream, t.data(), rows, k,
                         r0, keys.data());
    }
    hipLaunchKernelGGL(pca_flip_rows_kernel, dim3(grid_blocks((int64_t)d * k, 256)), dim3(256), 0, res.stream, f.comp.p, k, d, f.comp.sr(),
                       f.comp.sc(), keys.data());
    HIP_TRY(hipGetLastError());
  }
  sync(res);  // the host vectors above are still being copied
}

fit_args pca_fit_validate(cuvsPcaParams_t params, DLManagedTensor* input, DLManagedTensor* components, DLManagedTensor* explained_var,
                          DLManagedTensor* explained_var_ratio, DLManagedTensor* singular_vals, DLManagedTensor* mu,
                          DLManagedTensor* noise_vars, bool u_sign)
{
  CUVS_EXPECTS(params != nullptr, "pca: params is null");
  fit_args f;
  f.x = pca_matrix(input, "input", -1, -1);
  pca_check_dims(params, f.x.rows, f.x.cols);
  CUVS_EXPECTS(params->algorithm != CUVS_PCA_COV_EIG_JACOBI || params->n_iterations >= 1,
               "pca: n_iterations must be at least 1 for CUVS_PCA_COV_EIG_JACOBI but is %d", params->n_iterations);
  f.k      = params->n_components;
  f.comp   = pca_matrix(components, "components", f.k, f.x.cols);
  f.ev     = pca_vector(explained_var, "explained_var", f.k);
  f.evr    = pca_vector(explained_var_ratio, "explained_var_ratio", f.k);
  f.sv     = pca_vector(singular_vals, "singular_vals", f.k);
  f.mu     = pca_vector(mu, "mu", f.x.cols);
  f.noise  = pca_vector(noise_vars, "noise_vars", 1, true);
  f.u_sign = u_sign;
  return f;
}

}  // namespace
}  // namespace cuvs_amd

using namespace cuvs_amd;

extern "C" {

cuvsError_t cuvsPcaParamsCreate(cuvsPcaParams_t* params)
{
  return (cuvsError_t)translate_exceptions([=] {
    CUVS_EXPECTS(params != nullptr, "params is null");
    *params = new cuvsPcaParams{1, true, false, CUVS_PCA_COV_EIG_DQ, 0.0f, 15};  // c/src/preprocessing/pca.cpp
  });
}
cuvsError_t cuvsPcaParamsDestroy(cuvsPcaParams_t params)
{
  return (cuvsError_t)translate_exceptions([=] { delete params; });
}

cuvsError_t cuvsPcaFit(cuvsResources_t res_h, cuvsPcaParams_t params, DLManagedTensor* input, DLManagedTensor* components,
                       DLManagedTensor* explained_var, DLManagedTensor* explained_var_ratio, DLManagedTensor* singular_vals,
                       DLManagedTensor* mu, DLManagedTensor* noise_vars, bool flip_signs_based_on_U)
{
  return (cuvsError_t)translate_exceptions([=] {
    const fit_args f =
      pca_fit_validate(params, input, components, explained_var, explained_var_ratio, singular_vals, mu, noise_vars, flip_signs_based_on_U);
    pca_fit_impl(*as_res(res_h), params, f);
  });
}

cuvsError_t cuvsPcaFitTransform(cuvsResources_t res_h, cuvsPcaParams_t params, DLManagedTensor* input, DLManagedTensor* trans_input,
                                DLManagedTensor* components, DLManagedTensor* explained_var, DLManagedTensor* explained_var_ratio,
                                DLManagedTensor* singular_vals, DLManagedTensor* mu, DLManagedTensor* noise_vars,
                                bool flip_signs_based_on_U)
{
  return (cuvsError_t)translate_exceptions([=] {
    const fit_args f =
      pca_fit_validate(params, input, components, explained_var, explained_var_ratio, singular_vals, mu, noise_vars, flip_signs_based_on_U);
    const pca_mat out = pca_matrix(trans_input, "trans_input", f.x.rows, f.k);
    resources& res    = *as_res(res_h);
    pca_fit_impl(res, params, f);
    pca_transform_impl(res, params, f.x, f.comp, f.sv, f.mu, out);
    sync(res);
  });
}

cuvsError_t cuvsPcaTransform(cuvsResources_t res_h, cuvsPcaParams_t params, DLManagedTensor* input, DLManagedTensor* components,
                             DLManagedTensor* singular_vals, DLManagedTensor* mu, DLManagedTensor* trans_input)
{
  return (cuvsError_t)translate_exceptions([=] {
    CUVS_EXPECTS(params != nullptr, "pca: params is null");
    const pca_mat x = pca_matrix(input, "input", -1, -1);
    pca_check_dims(params, x.rows, x.cols);
    const int64_t k    = params->n_components;
    const pca_mat comp = pca_matrix(components, "components", k, x.cols);
    const float* sv    = pca_vector(singular_vals, "singular_vals", k);
    const float* m     = pca_vector(mu, "mu", x.cols);
    const pca_mat out  = pca_matrix(trans_input, "trans_input", x.rows, k);
    resources& res     = *as_res(res_h);
    pca_transform_impl(res, params, x, comp, sv, m, out);
    sync(res);
  });
}

cuvsError_t cuvsPcaInverseTransform(cuvsResources_t res_h, cuvsPcaParams_t params, DLManagedTensor* trans_input, DLManagedTensor* components,
                                    DLManagedTensor* singular_vals, DLManagedTensor* mu, DLManagedTensor* output)
{
  return (cuvsError_t)translate_exceptions([=] {
    CUVS_EXPECTS(params != nullptr, "pca: params is null");
    const pca_mat t    = pca_matrix(trans_input, "trans_input", -1, -1);
    const pca_mat comp = pca_matrix(components, "components", -1, -1);
    pca_check_dims(params, t.rows, comp.cols);
    const int64_t k = params->n_components;
    CUVS_EXPECTS(comp.rows == k, "pca: components must be [%lld, %lld] but is [%lld, %lld]", (long long)k, (long long)comp.cols,
                 (long long)comp.rows, (long long)comp.cols);
    CUVS_EXPECTS(t.cols == k, "pca: trans_input must have n_components = %lld columns but has %lld", (long long)k, (long long)t.cols);
    const float* sv   = pca_vector(singular_vals, "singular_vals", k);
    const float* m    = pca_vector(mu, "mu", comp.cols);
    const pca_mat out = pca_matrix(output, "output", t.rows, comp.cols);
    resources& res    = *as_res(res_h);
    pca_inverse_impl(res, params, t, comp, sv, m, out);
    sync(res);
  });
}

cuvsError_t cuvsAmdPcaLastSweeps(int* sweeps)
{
  return (cuvsError_t)translate_exceptions([=] {
    CUVS_EXPECTS(sweeps != nullptr, "sweeps is null");
    *sweeps = pca_last_sweeps;
  });
}

}  // extern "C"
