// ScaNN index build (reference: cpp/src/neighbors/scann/detail/scann_{build,avq,soar,quantize,serialize}.cuh; C entry points
// include/cuvs_amd/scann.h; contract and deviations: DESIGN.md 3.1z). The partitioning, the product quantizer and the row
// loaders are the library's own (ops.hpp, pq_quantize.hpp); three stages are new here:
//
//   AVQ centres   avq_vec_kernel accumulates S = sum w1, b = sum w1 x and sum x of every leaf, avq_gram_kernel the weighted
//                 Gram matrices sum w3 x x^T of a batch of leaves on the fp32 matrix cores (one 64 x 64 tile of the lower
//                 triangle per workgroup, the members as the K dimension, in ascending row id), avq_solve_kernel factors
//                 S I + (eta - 1) G by Cholesky with a workgroup per leaf (in LDS while the matrix fits, else in the
//                 workspace) and solves. The rows are walked in batches of 65536; every accumulator is carried from batch to
//                 batch, so the chain of a leaf is the same whatever the batches are and wherever the rows live. No atomics.
//   SOAR labels   soar_tile_kernel: the unit residual rh_i and the row x_i are stacked as operand rows of one 128 x 128 x 16
//                 fp32-MFMA tile against the centres (a wave holds <rh_i, c_j> and <x_i, c_j> of the same 32 rows x 64
//                 centres), the score is finished in the epilogue and a workgroup walks all centre tiles with the running
//                 (score, id) of its 64 rows in registers. The tile, its staging and its k-ordered fma chain are those of
//                 distance.hip (distance_tile.hpp).
//   bf16 rows     bf16_kernel: a wave per row; the constants of 64 coordinates in parallel, the accept step lane by lane.
#include "common.hpp"
#include "device_utils.hpp"
#include "distance_tile.hpp"
#include "ops.hpp"
#include "pq_quantize.hpp"
#include "scann_host.hpp"

#include <cuvs_amd/scann.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

namespace cuvs_amd {
namespace {

namespace H = scann_host;

constexpr int kThreads = 256;

// ================================================================ AVQ centres
// w1 = |x|^(eta - 1), w3 = |x|^(eta - 3) from the canonical squared norm (row_norms); a zero row has weights 0
__global__ void avq_weights_kernel(const float* __restrict__ sq, int64_t n, float eta, float* __restrict__ w1, float* __restrict__ w3)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float s = sq[i];
  float a = 0.f, b = 0.f;
  if (s > 0.f) {
    const float nrm = sqrtf(s);
    a               = eta == 1.0f ? 1.0f : powf(nrm, eta - 1.0f);
    b               = powf(nrm, eta - 3.0f);
  }
  w1[i] = a;
  w3[i] = b;
}

struct avq_acc {
  float* S;         // [n_leaves]      sum w1
  float* b;         // [n_leaves, dim] sum w1 x
  float* sx;        // [n_leaves, dim] sum x
  uint32_t* count;  // [n_leaves]      members
};

// a workgroup per leaf, a thread per coordinate: the members of this batch in ascending row id, one chain per accumulator
__global__ __launch_bounds__(kThreads) void avq_vec_kernel(const float* __restrict__ x, int dim, const uint32_t* __restrict__ perm,
                                                            const uint32_t* __restrict__ off, const float* __restrict__ w1, avq_acc a)
{
  const uint32_t leaf = blockIdx.x;
  const uint32_t m0 = off[leaf], m1 = off[leaf + 1];
  if (m0 == m1) return;
  for (int d = threadIdx.x; d < dim; d += kThreads) {
    float b = a.b[(int64_t)leaf * dim + d], sx = a.sx[(int64_t)leaf * dim + d];
    for (uint32_t m = m0; m < m1; ++m) {
      const uint32_t row = perm[m];
      const float v      = x[(int64_t)row * dim + d];
      b                  = __fmaf_rn(w1[row], v, b);
      sx                 = sx + v;
    }
    a.b[(int64_t)leaf * dim + d]  = b;
    a.sx[(int64_t)leaf * dim + d] = sx;
  }
  if (threadIdx.x == 0) {
    float S = a.S[leaf];
    for (uint32_t m = m0; m < m1; ++m) S = S + w1[perm[m]];
    a.S[leaf] = S;
    a.count[leaf] += m1 - m0;
  }
}

constexpr int kGramTile = 64;  // a workgroup's tile of the Gram matrix: 2 x 2 waves of 2 x 2 MFMA tiles
constexpr int kGramLd   = 80;  // k-major pitch of the staged members: 16 k lands the four lane groups on different banks

// G[leaf][r][c] += sum over the batch's members of (w3 x_r) x_c, r >= c by tiles; the accumulators continue from G
__global__ __launch_bounds__(kThreads) void avq_gram_kernel(const float* __restrict__ x, int dim, const uint32_t* __restrict__ perm,
                                                             const uint32_t* __restrict__ off, const float* __restrict__ w3,
                                                             uint32_t leaf0, float* __restrict__ G)
{
  __shared__ float As[BK * kGramLd];
  __shared__ float Bs[BK * kGramLd];
  const uint32_t leaf = leaf0 + blockIdx.y;
  const uint32_t m0 = off[leaf], m1 = off[leaf + 1];
  if (m0 == m1) return;  // workgroup-uniform
  int tr = 0;
  while ((tr + 1) * (tr + 2) / 2 <= (int)blockIdx.x) ++tr;
  const int tc = (int)blockIdx.x - tr * (tr + 1) / 2;
  const int r0 = tr * kGramTile, c0 = tc * kGramTile;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, l15 = lane & 15, lg = lane >> 4;
  float* Gl = G + (int64_t)blockIdx.y * dim * dim;

  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int row = r0 + wm * 32 + i * 16 + lg * 4 + e, col = c0 + wn * 32 + j * 16 + l15;
        acc[i][j][e]  = (row < dim && col < dim) ? Gl[(int64_t)row * dim + col] : 0.f;
      }

  const int sk = tid >> 4, sc = (tid & 15) * 4;
  for (uint32_t mm = m0; mm < m1; mm += BK) {
    float a[4] = {0.f, 0.f, 0.f, 0.f}, b[4] = {0.f, 0.f, 0.f, 0.f};
    if (mm + sk < m1) {
      const uint32_t row = perm[mm + sk];
      const float w      = w3[row];
      const float* xr    = x + (int64_t)row * dim;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (r0 + sc + e < dim) a[e] = w * xr[r0 + sc + e];
        if (c0 + sc + e < dim) b[e] = xr[c0 + sc + e];
      }
    }
    __syncthreads();  // the previous step's operands have been read
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      As[sk * kGramLd + sc + e] = a[e];
      Bs[sk * kGramLd + sc + e] = b[e];
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int k = 4 * c + lg;
      float av[2], bv[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) av[i] = As[k * kGramLd + wm * 32 + i * 16 + l15];
#pragma unroll
      for (int j = 0; j < 2; ++j) bv[j] = Bs[k * kGramLd + wn * 32 + j * 16 + l15];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], bv[j], acc[i][j], 0, 0, 0);
    }
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int row = r0 + wm * 32 + i * 16 + lg * 4 + e, col = c0 + wn * 32 + j * 16 + l15;
        if (row < dim && col < dim) Gl[(int64_t)row * dim + col] = acc[i][j][e];
      }
}

// centre = eta * inverse(S I + (eta - 1) G) b by Cholesky (lower triangle), a workgroup per leaf. IN_LDS: the matrix lives in
// LDS; otherwise it is factored in place in the workspace. Every element has one writer per step: the result is reproducible.
template <bool IN_LDS>
__global__ __launch_bounds__(kThreads) void avq_solve_kernel(float* __restrict__ G, int dim, uint32_t leaf0, avq_acc a, float eta,
                                                              float* __restrict__ centers)
{
  extern __shared__ float smem[];
  const uint32_t leaf = leaf0 + blockIdx.x;
  const float S       = a.S[leaf];
  if (!(S > 0.f)) return;  // no members, or zero rows only: the centre stays
  const int tid = threadIdx.x;
  float* Gl     = G + (int64_t)blockIdx.x * dim * dim;
  float* M      = IN_LDS ? smem : Gl;
  float* y      = IN_LDS ? smem + (int64_t)dim * dim : smem;
  const float em1 = eta - 1.0f;
  for (int idx = tid; idx < dim * dim; idx += kThreads) {
    const int i = idx / dim, k = idx - i * dim;
    if (k <= i) M[idx] = em1 * Gl[idx] + (i == k ? S : 0.f);
  }
  for (int d = tid; d < dim; d += kThreads) y[d] = a.b[(int64_t)leaf * dim + d];
  __syncthreads();
  for (int j = 0; j < dim; ++j) {
    if (tid == 0) M[j * dim + j] = sqrtf(M[j * dim + j]);
    __syncthreads();
    const float diag = M[j * dim + j];
    for (int i = j + 1 + tid; i < dim; i += kThreads) M[i * dim + j] = M[i * dim + j] / diag;
    __syncthreads();
    const int rem = dim - j - 1;
    for (int idx = tid; idx < rem * rem; idx += kThreads) {
      const int q = idx / rem;
      const int i = j + 1 + q, k = j + 1 + (idx - q * rem);
      if (k <= i) M[i * dim + k] = M[i * dim + k] - M[i * dim + j] * M[k * dim + j];
    }
    __syncthreads();
  }
  for (int j = 0; j < dim; ++j) {  // L y' = b
    if (tid == 0) y[j] = y[j] / M[j * dim + j];
    __syncthreads();
    const float yj = y[j];
    for (int i = j + 1 + tid; i < dim; i += kThreads) y[i] = y[i] - M[i * dim + j] * yj;
    __syncthreads();
  }
  for (int j = dim - 1; j >= 0; --j) {  // L^T z = y'
    if (tid == 0) y[j] = y[j] / M[j * dim + j];
    __syncthreads();
    const float yj = y[j];
    for (int i = tid; i < j; i += kThreads) y[i] = y[i] - M[j * dim + i] * yj;
    __syncthreads();
  }
  for (int d = tid; d < dim; d += kThreads) centers[(int64_t)leaf * dim + d] = eta * y[d];
}

// eta == 1: centre = b / S
__global__ void avq_mean_kernel(avq_acc a, int64_t n_leaves, int dim, float* __restrict__ centers)
{
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_leaves * dim) return;
  const float S = a.S[t / dim];
  if (S > 0.f) centers[t] = a.b[t] / S;
}

// per leaf: <sum x, centre> and n |centre|^2, chains over the coordinates in ascending order
__global__ void avq_rescale_parts_kernel(avq_acc a, int64_t n_leaves, int dim, const float* __restrict__ centers,
                                         float* __restrict__ num, float* __restrict__ den)
{
  const int64_t leaf = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (leaf >= n_leaves) return;
  float dot = 0.f, cc = 0.f;
  if (a.S[leaf] > 0.f) {
    const float* c  = centers + leaf * dim;
    const float* sx = a.sx + leaf * dim;
    for (int d = 0; d < dim; ++d) {
      dot = __fmaf_rn(sx[d], c[d], dot);
      cc  = __fmaf_rn(c[d], c[d], cc);
    }
    cc = (float)a.count[leaf] * cc;
  }
  num[leaf] = dot;
  den[leaf] = cc;
}
// the two sums in fp64, leaf by leaf, by one thread; a zero or non-finite denominator or quotient gives 1
__global__ void avq_rescale_kernel(const float* __restrict__ num, const float* __restrict__ den, int64_t n_leaves, float* __restrict__ out)
{
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  double n = 0.0, d = 0.0;
  for (int64_t i = 0; i < n_leaves; ++i) {
    n += (double)num[i];
    d += (double)den[i];
  }
  const float r = (float)(n / d);
  *out          = (d != 0.0 && isfinite(d) && isfinite(r)) ? r : 1.0f;
}
__global__ void avq_scale_kernel(avq_acc a, int64_t n_leaves, int dim, const float* __restrict__ rescale, float* __restrict__ centers)
{
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_leaves * dim) return;
  if (a.S[t / dim] > 0.f) centers[t] = centers[t] * *rescale;
}

// rows [r0, r0 + cnt) of a dataset on the device or on the host, as a device pointer (host rows through a staging buffer that
// the next call reuses: the caller finishes its work on a batch before it asks for the next)
struct row_source {
  const float* data;
  int64_t n, dim;
  bool is_host;
  dev_buf<float> stage;
  const float* batch(resources& res, int64_t r0, int64_t cnt)
  {
    if (!is_host) return data + r0 * dim;
    if (stage.size() == 0) stage = dev_buf<float>(res, (size_t)(std::min(n, H::kMaxBatchRows) * dim));
    sync(res);  // the previous batch is done with the buffer
    copy_async(res, stage.data(), data + r0 * dim, (size_t)(cnt * dim) * sizeof(float));
    sync(res);  // the host rows may be pageable
    return stage.data();
  }
};

void avq_centers(resources& res, row_source& src, const uint32_t* labels, int64_t n_leaves, float eta, float* centers)
{
  const int64_t n = src.n, dim = src.dim;
  const bool plain = eta == 1.0f;
  dev_buf<float> S(res, (size_t)n_leaves), b(res, (size_t)(n_leaves * dim)), sx(res, (size_t)(n_leaves * dim));
  dev_buf<uint32_t> count(res, (size_t)n_leaves);
  HIP_TRY(hipMemsetAsync(S.data(), 0, S.bytes(), res.stream));
  HIP_TRY(hipMemsetAsync(b.data(), 0, b.bytes(), res.stream));
  HIP_TRY(hipMemsetAsync(sx.data(), 0, sx.bytes(), res.stream));
  HIP_TRY(hipMemsetAsync(count.data(), 0, count.bytes(), res.stream));
  avq_acc acc{S.data(), b.data(), sx.data(), count.data()};

  const int64_t batch_rows = std::min(n, H::kMaxBatchRows);
  dev_buf<float> sq(res, (size_t)batch_rows), w1(res, (size_t)batch_rows), w3(res, (size_t)batch_rows);
  dev_buf<uint32_t> perm(res, (size_t)batch_rows), off(res, (size_t)(n_leaves + 1));
  const int64_t leaf_batch = plain ? n_leaves : std::min<int64_t>(H::avq_leaf_batch(n_leaves, dim, res.workspace_limit), 65535);
  dev_buf<float> G;
  if (!plain) G = dev_buf<float>(res, (size_t)(leaf_batch * dim * dim));
  const bool in_lds  = H::avq_solve_in_lds(dim, res.lds_per_block);
  const size_t lds   = (size_t)((in_lds ? dim * dim : 0) + 2 * dim) * sizeof(float);
  const int n_tiles  = ceil_div(dim, kGramTile);
  const int lower    = n_tiles * (n_tiles + 1) / 2;
  if (!plain) {
    CUVS_EXPECTS(lds <= res.lds_per_block, "dim %lld is too large for the AVQ solve", (long long)dim);
    if (in_lds)
      HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(avq_solve_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  }

  for (int64_t l0 = 0; l0 < n_leaves; l0 += leaf_batch) {
    const int64_t nl = std::min(leaf_batch, n_leaves - l0);
    if (!plain) HIP_TRY(hipMemsetAsync(G.data(), 0, (size_t)(nl * dim * dim) * sizeof(float), res.stream));
    for (int64_t r0 = 0; r0 < n; r0 += batch_rows) {
      const int64_t cnt = std::min(batch_rows, n - r0);
      const float* x    = src.batch(res, r0, cnt);
      row_norms<float>(res, x, cnt, dim, dim, sq.data(), false);
      hipLaunchKernelGGL(avq_weights_kernel, dim3(grid_blocks(cnt, kThreads)), dim3(kThreads), 0, res.stream, sq.data(), cnt, eta,
                         w1.data(), w3.data());
      group_by_label(res, labels + r0, cnt, (uint32_t)n_leaves, perm.data(), off.data());
      if (l0 == 0) {
        profile_begin(res, "avq_vec_kernel");
        hipLaunchKernelGGL(avq_vec_kernel, dim3((unsigned)n_leaves), dim3(kThreads), 0, res.stream, x, (int)dim, perm.data(), off.data(),
                           w1.data(), acc);
        profile_end(res, "avq_vec_kernel");
      }
      if (!plain) {
        profile_begin(res, "avq_gram_kernel");
        hipLaunchKernelGGL(avq_gram_kernel, dim3((unsigned)lower, (unsigned)nl), dim3(kThreads), 0, res.stream, x, (int)dim, perm.data(),
                           off.data(), w3.data(), (uint32_t)l0, G.data());
        profile_end(res, "avq_gram_kernel");
      }
      HIP_TRY(hipGetLastError());
    }
    if (!plain) {
      profile_begin(res, "avq_solve_kernel");
      if (in_lds)
        hipLaunchKernelGGL(avq_solve_kernel<true>, dim3((unsigned)nl), dim3(kThreads), lds, res.stream, G.data(), (int)dim, (uint32_t)l0, acc,
                           eta, centers);
      else
        hipLaunchKernelGGL(avq_solve_kernel<false>, dim3((unsigned)nl), dim3(kThreads), lds, res.stream, G.data(), (int)dim, (uint32_t)l0,
                           acc, eta, centers);
      profile_end(res, "avq_solve_kernel");
      HIP_TRY(hipGetLastError());
    }
  }
  if (plain)
    hipLaunchKernelGGL(avq_mean_kernel, dim3(grid_blocks(n_leaves * dim, kThreads)), dim3(kThreads), 0, res.stream, acc, n_leaves, (int)dim,
                       centers);
  dev_buf<float> num(res, (size_t)n_leaves), den(res, (size_t)n_leaves), rescale(res, 1);
  hipLaunchKernelGGL(avq_rescale_parts_kernel, dim3(grid_blocks(n_leaves, kThreads)), dim3(kThreads), 0, res.stream, acc, n_leaves, (int)dim,
                     centers, num.data(), den.data());
  hipLaunchKernelGGL(avq_rescale_kernel, dim3(1), dim3(64), 0, res.stream, num.data(), den.data(), n_leaves, rescale.data());
  hipLaunchKernelGGL(avq_scale_kernel, dim3(grid_blocks(n_leaves * dim, kThreads)), dim3(kThreads), 0, res.stream, acc, n_leaves, (int)dim,
                     rescale.data(), centers);
  HIP_TRY(hipGetLastError());
  sync(res);  // the scratch buffers and the staging buffer go out of scope
}

// ================================================================ SOAR labels
// cn_j = chain(c_j, c_j)
__global__ void soar_center_norms_kernel(const float* __restrict__ centers, int64_t n_leaves, int dim, float* __restrict__ cn)
{
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_leaves) return;
  const float* c = centers + j * dim;
  float acc      = 0.f;
  for (int k = 0; k < dim; ++k) acc = __fmaf_rn(c[k], c[k], acc);
  cn[j] = acc;
}

// a thread per row: r = x - c[label], nr = sqrtf(chain(r, r)), rh = r / nr (zeros when nr == 0), p = chain(rh, x)
__global__ void soar_prep_kernel(const float* __restrict__ x, int64_t n, int dim, const float* __restrict__ centers,
                                 const uint32_t* __restrict__ labels, float* __restrict__ rh, float* __restrict__ p)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float* xr = x + i * dim;
  const float* c  = centers + (int64_t)labels[i] * dim;
  float acc       = 0.f;
  for (int k = 0; k < dim; ++k) {
    const float r = xr[k] - c[k];
    acc           = __fmaf_rn(r, r, acc);
  }
  const float nr = sqrtf(acc);
  float pp       = 0.f;
  float* o       = rh + i * dim;
  for (int k = 0; k < dim; ++k) {
    const float r = xr[k] - c[k];
    const float h = nr == 0.f ? 0.f : r / nr;
    o[k]          = h;
    pp            = __fmaf_rn(h, xr[k], pp);
  }
  p[i] = pp;
}

constexpr int kSoarRows = 64;  // data rows of a workgroup: 128 operand rows

// operand row r of the tile -> (which matrix, data row): wave row wm holds data rows wm * 32 .. + 31, MFMA tiles i = 0, 1 their
// rh rows and i = 2, 3 their x rows, so that a lane has <rh_i, c_j> in acc[i] and <x_i, c_j> in acc[i + 2]
__device__ __forceinline__ void soar_load(const float* __restrict__ x, const float* __restrict__ rh, int64_t row0, int r, int64_t m,
                                          int64_t dim, int64_t k0, bool vec, float (&v)[4])
{
  const int i        = (r >> 4) & 3;
  const int64_t drow = row0 + (r >> 6) * 32 + (i & 1) * 16 + (r & 15);
  const float* src   = (i >> 1) ? x : rh;
  if (vec) load4<float, true>(src, drow, m, dim, k0, dim, v);
  else load4<float, false>(src, drow, m, dim, k0, dim, v);
}

__device__ __forceinline__ void soar_load_center(const float* __restrict__ centers, int64_t row, int64_t n_leaves, int64_t dim, int64_t k0,
                                                 bool vec, float (&v)[4])
{
  if (vec) load4<float, true>(centers, row, n_leaves, dim, k0, dim, v);
  else load4<float, false>(centers, row, n_leaves, dim, k0, dim, v);
}

__global__ __launch_bounds__(kThreads) void soar_tile_kernel(const float* __restrict__ x, const float* __restrict__ rh,
                                                              const float* __restrict__ p, int64_t m, int64_t dim,
                                                              const float* __restrict__ centers, const float* __restrict__ cn,
                                                              int64_t n_leaves, float lambda, bool vec, uint32_t* __restrict__ out)
{
  __shared__ __attribute__((aligned(16))) float As[2][BK * LDT];
  __shared__ __attribute__((aligned(16))) float Bs[2][BK * LDT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, l15 = lane & 15, lg = lane >> 4;
  const int64_t row0 = (int64_t)blockIdx.x * kSoarRows;
  const int nkt      = (int)((dim + BK - 1) / BK);
  const int sr0 = tid >> 2, sr1 = (tid + 256) >> 2, sc = tid & 3;

  float pv[8], best_v[8];
  uint32_t best_i[8];
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    const int64_t row = row0 + wm * 32 + (t >> 2) * 16 + lg * 4 + (t & 3);
    pv[t]             = row < m ? p[row] : 0.f;
    best_v[t]         = std::numeric_limits<float>::infinity();
    best_i[t]         = 0xffffffffu;
  }

  const int64_t n_col_tiles = (n_leaves + BN - 1) / BN;
  for (int64_t ct = 0; ct < n_col_tiles; ++ct) {
    const int64_t col0 = ct * BN;
    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    float ra0[4], ra1[4], rb0[4], rb1[4];
    soar_load(x, rh, row0, sr0, m, dim, sc * 4, vec, ra0);
    soar_load(x, rh, row0, sr1, m, dim, sc * 4, vec, ra1);
    soar_load_center(centers, col0 + sr0, n_leaves, dim, sc * 4, vec, rb0);
    soar_load_center(centers, col0 + sr1, n_leaves, dim, sc * 4, vec, rb1);
    __syncthreads();  // the previous centre tile is done with the LDS buffers
    stage_store(As[0], sr0, sc, ra0);
    stage_store(As[0], sr1, sc, ra1);
    stage_store(Bs[0], sr0, sc, rb0);
    stage_store(Bs[0], sr1, sc, rb1);
    __syncthreads();

    for (int kt = 0; kt < nkt; ++kt) {
      const int buf = kt & 1;
      if (kt + 1 < nkt) {
        const int64_t k0 = (int64_t)(kt + 1) * BK + sc * 4;
        soar_load(x, rh, row0, sr0, m, dim, k0, vec, ra0);
        soar_load(x, rh, row0, sr1, m, dim, k0, vec, ra1);
        soar_load_center(centers, col0 + sr0, n_leaves, dim, k0, vec, rb0);
        soar_load_center(centers, col0 + sr1, n_leaves, dim, k0, vec, rb1);
      }
      const float* A = As[buf];
      const float* B = Bs[buf];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int k   = 4 * c + lg;
        const int swz = c << 3;
        float a[4], b[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] = A[k * LDT + ((wm * 64 + i * 16 + l15) ^ swz)];
#pragma unroll
        for (int j = 0; j < 4; ++j) b[j] = B[k * LDT + ((wn * 64 + j * 16 + l15) ^ swz)];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
      }
      if (kt + 1 < nkt) {
        stage_store(As[buf ^ 1], sr0, sc, ra0);
        stage_store(As[buf ^ 1], sr1, sc, ra1);
        stage_store(Bs[buf ^ 1], sr0, sc, rb0);
        stage_store(Bs[buf ^ 1], sr1, sc, rb1);
      }
      __syncthreads();
    }

    // epilogue: C layout col = lane & 15, row = (lane >> 4) * 4 + e. A lane visits its columns in ascending order, so the
    // strict comparison keeps the lowest id
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t col = col0 + wn * 64 + j * 16 + l15;
      if (col >= n_leaves) continue;
      const float cnv = cn[col];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int t   = i * 4 + e;
          const float d = acc[i][j][e] - pv[t];
          const float s = ((d * d) * lambda + (-2.0f * acc[i + 2][j][e])) + cnv;
          if (s < best_v[t]) { best_v[t] = s; best_i[t] = (uint32_t)col; }
        }
    }
  }

  // the 16 lanes that share a row, then the two column waves
  __syncthreads();
  float* red_v    = As[0];                               // [2][64]
  uint32_t* red_i = reinterpret_cast<uint32_t*>(Bs[0]);  // [2][64]
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    float v    = best_v[t];
    uint32_t i = best_i[t];
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) {
      const float ov    = __shfl_xor(v, o, kWave);
      const uint32_t oi = __shfl_xor(i, o, kWave);
      if (ov < v || (ov == v && oi < i)) { v = ov; i = oi; }
    }
    if (l15 == 0) {
      const int r               = wm * 32 + (t >> 2) * 16 + lg * 4 + (t & 3);
      red_v[wn * kSoarRows + r] = v;
      red_i[wn * kSoarRows + r] = i;
    }
  }
  __syncthreads();
  if (tid < kSoarRows) {
    const int64_t row = row0 + tid;
    if (row < m) {
      const float v0 = red_v[tid], v1 = red_v[kSoarRows + tid];
      const uint32_t i0 = red_i[tid], i1 = red_i[kSoarRows + tid];
      const uint32_t i  = ((v1 < v0) || (v1 == v0 && i1 < i0)) ? i1 : i0;
      out[row]          = i == 0xffffffffu ? 0u : i;  // no finite score (non-finite input): leaf 0
    }
  }
}

struct soar_scratch {
  dev_buf<float> cn, rh, p;
  soar_scratch(resources& res, int64_t batch_rows, int64_t dim, int64_t n_leaves)
    : cn(res, (size_t)n_leaves), rh(res, (size_t)(batch_rows * dim)), p(res, (size_t)batch_rows)
  {
  }
};

void soar_center_norms(resources& res, const float* centers, int64_t n_leaves, int64_t dim, float* cn)
{
  hipLaunchKernelGGL(soar_center_norms_kernel, dim3(grid_blocks(n_leaves, kThreads)), dim3(kThreads), 0, res.stream, centers, n_leaves,
                     (int)dim, cn);
  HIP_TRY(hipGetLastError());
}

// SOAR labels of the device rows x [cnt, dim]; s.cn holds the centre norms
void soar_batch(resources& res, const float* x, int64_t cnt, int64_t dim, const float* centers, int64_t n_leaves,
                const uint32_t* labels, float lambda, soar_scratch& s, uint32_t* out)
{
  hipLaunchKernelGGL(soar_prep_kernel, dim3(grid_blocks(cnt, kThreads)), dim3(kThreads), 0, res.stream, x, cnt, (int)dim, centers, labels,
                     s.rh.data(), s.p.data());
  profile_begin(res, "soar_tile_kernel");
  const bool vec = vec_ok(x, dim, dim) && vec_ok(s.rh.data(), dim, dim) && vec_ok(centers, dim, dim);
  hipLaunchKernelGGL(soar_tile_kernel, dim3(grid_blocks(cnt, kSoarRows)), dim3(kThreads), 0, res.stream, x, s.rh.data(), s.p.data(), cnt,
                     dim, centers, s.cn.data(), n_leaves, lambda, vec, out);
  profile_end(res, "soar_tile_kernel");
  HIP_TRY(hipGetLastError());
}

// ================================================================ bf16 rows
__device__ __forceinline__ uint16_t bf16_rne(float f)
{
  uint32_t u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);  // NaN stays NaN
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
__device__ __forceinline__ float bf16_value(uint16_t b) { return __uint_as_float((uint32_t)b << 16); }

// 64 strided fmaf partials and a fixed butterfly: every lane ends with the same sum
__device__ __forceinline__ float bf16_wave_sum(float acc)
{
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc = acc + __shfl_xor(acc, o, kWave);
  return acc;
}

// a wave per row: round to nearest even; with a threshold T and |x|^2 > T^2, up to 10 rounds of coordinate
// descent on the AVQ loss over the coordinates in ascending order
__global__ __launch_bounds__(kThreads) void bf16_kernel(const float* __restrict__ x, int64_t n, int dim, float threshold,
                                                        uint16_t* __restrict__ out)
{
  const int lane = lane_id();
  for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < n; row += (int64_t)gridDim.x * 4) {
    const float* xr = x + row * dim;
    uint16_t* o     = out + row * dim;
    float acc       = 0.f;
    for (int d = lane; d < dim; d += kWave) {
      const float v = xr[d];
      acc           = __fmaf_rn(v, v, acc);
      o[d]          = bf16_rne(v);
    }
    const float sq = bf16_wave_sum(acc);
    const float t2 = threshold * threshold;
    if (!(sq > t2) || sq == 0.f) continue;  // wave-uniform; a NaN threshold ends here
    const float nrm   = sqrtf(sq);
    const float ratio = t2 / sq;
    const float em1   = (((float)(dim - 1) * ratio) / (1.0f - ratio)) - 1.0f;
    acc               = 0.f;
    for (int d = lane; d < dim; d += kWave) {
      const float v = xr[d];
      acc           = __fmaf_rn(v - bf16_value(o[d]), v, acc);
    }
    float D = bf16_wave_sum(acc) / nrm;
    for (int round = 0; round < H::kMaxNoiseShapingRounds; ++round) {
      bool changed = false;
      for (int base = 0; base < dim; base += kWave) {
        const int d = base + lane;
        bool valid  = false;
        float A = 0.f, B = 0.f, delta = 0.f;
        uint16_t nb = 0;
        if (d < dim) {
          const float xd    = xr[d];
          const uint16_t qb = o[d];
          const float qd    = bf16_value(qb);
          if (qd != xd) {
            // the neighbour on the other side of x: away from zero when (q < x) for a positive q or (q > x) for a negative one
            const bool away = (qd < xd) != ((qb >> 15) != 0);
            const bool can  = away || (qb & 0x7fffu) != 0;
            nb              = away ? (uint16_t)(qb + 1) : (uint16_t)(qb - 1);
            if (can && (nb & 0x7f80u) != 0x7f80u) {
              const float qn = bf16_value(nb);
              const float e0 = xd - qd, e1 = xd - qn;
              delta = ((e1 - e0) * xd) / nrm;
              A     = (2.0f * em1) * delta;
              B     = ((e1 * e1) - (e0 * e0)) + em1 * (delta * delta);
              valid = true;
            }
          }
        }
        const int steps = min(kWave, dim - base);
        bool mine       = false;
        for (int l = 0; l < steps; ++l) {
          const float a  = __shfl(A, l, kWave);
          const float b  = __shfl(B, l, kWave);
          const float dl = __shfl(delta, l, kWave);
          const int v    = __shfl((int)valid, l, kWave);
          if (v && (a * D + b < 0.f)) {
            D = D + dl;
            if (lane == l) mine = true;
          }
        }
        if (mine) o[d] = nb;
        changed = changed || __any(mine);
      }
      if (!changed) break;
    }
  }
}

void bf16_batch(resources& res, const float* x, int64_t cnt, int64_t dim, float threshold, int16_t* out)
{
  if (cnt == 0) return;
  const unsigned blocks = (unsigned)std::min<int64_t>((cnt + 3) / 4, (int64_t)res.num_cus * 32);
  profile_begin(res, "bf16_kernel");
  hipLaunchKernelGGL(bf16_kernel, dim3(blocks), dim3(kThreads), 0, res.stream, x, cnt, (int)dim, threshold, reinterpret_cast<uint16_t*>(out));
  profile_end(res, "bf16_kernel");
  HIP_TRY(hipGetLastError());
}

// ================================================================ small kernels of the build
__global__ void scann_max_label_kernel(const uint32_t* __restrict__ labels, int64_t n, uint32_t* __restrict__ out)
{
  uint32_t m = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) m = max(m, labels[i]);
  atomicMax(out, m);
}

// train[i] -= centers[labels[i * ratio]]: the primary residuals of the strided sample
__global__ void scann_sample_residual_kernel(float* __restrict__ train, int64_t m, int dim, int64_t ratio,
                                             const uint32_t* __restrict__ labels, const float* __restrict__ centers)
{
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= m * dim) return;
  const int64_t i = t / dim;
  train[t]        = train[t] - centers[(int64_t)labels[i * ratio] * dim + (t - i * dim)];
}

// codebook[e][j * pq_len + k] = book[(j * book_n + e) * pq_len + k] (scann_build.cuh:295-306)
__global__ void scann_codebook_kernel(const float* __restrict__ book, int64_t book_n, int n_sub, int pq_len, float* __restrict__ out)
{
  const int64_t t     = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t dim   = (int64_t)n_sub * pq_len;
  if (t >= book_n * dim) return;
  const int64_t e = t / dim;
  const int col   = (int)(t - e * dim);
  const int j = col / pq_len, k = col - j * pq_len;
  out[t] = book[((int64_t)j * book_n + e) * pq_len + k];
}

// ================================================================ the index
struct scann_index {
  H::params p;
  int64_t n = 0, dim = 0, n_leaves = 0, n_sub = 0, book_n = 0;
  dev_buf<float> centers, codebook;
  dev_buf<uint32_t> labels, soar_labels;
  std::vector<uint8_t> codes, soar_codes;
  std::vector<int16_t> bf16;
  int device = 0;
};

void check_label_range(resources& res, const uint32_t* labels, int64_t n, int64_t n_leaves)
{
  dev_buf<uint32_t> word(res, 1);
  HIP_TRY(hipMemsetAsync(word.data(), 0, sizeof(uint32_t), res.stream));
  const unsigned blocks = (unsigned)std::min<int64_t>(grid_blocks(n, kThreads), 1024);
  hipLaunchKernelGGL(scann_max_label_kernel, dim3(blocks), dim3(kThreads), 0, res.stream, labels, n, word.data());
  HIP_TRY(hipGetLastError());
  const uint32_t mx = read_word(res, word.data());
  if ((int64_t)mx >= n_leaves) H::refuse("labels must be below n_leaves (%lld): found %u", (long long)n_leaves, mx);
}

std::unique_ptr<scann_index> scann_build(resources& res, const H::params& p, const float* data, int64_t n, int64_t dim, bool is_host)
{
  H::check_params(p, n, dim);
  auto idx      = std::make_unique<scann_index>();
  idx->p        = p;
  idx->n        = n;
  idx->dim      = dim;
  idx->n_leaves = p.n_leaves;
  idx->n_sub    = dim / p.pq_dim;
  idx->book_n   = int64_t(1) << p.pq_bits;
  idx->device   = res.device;
  const int64_t n_leaves = idx->n_leaves, batch_rows = std::min(n, H::kMaxBatchRows);
  row_source src{data, n, dim, is_host, {}};

  // 1. partition: hierarchical balanced k-means on a strided sample, then the label of every row
  idx->centers = dev_buf<float>::persistent((size_t)(n_leaves * dim));
  {
    const int64_t m = H::kmeans_train_rows(p, n);
    dev_buf<float> train(res, (size_t)(m * dim));
    HIP_TRY(hipMemcpy2DAsync(train.data(), dim * sizeof(float), data, (size_t)(dim * (n / m)) * sizeof(float), dim * sizeof(float), m,
                             hipMemcpyDefault, res.stream));
    kmeans_params kp;
    kp.n_iters = (int)p.kmeans_n_iters;
    kmeans_balanced_fit(res, train.data(), m, dim, (int)n_leaves, kp, idx->centers.data());
    sync(res);
  }
  idx->labels      = dev_buf<uint32_t>::persistent((size_t)n);
  idx->soar_labels = dev_buf<uint32_t>::persistent((size_t)n);
  for (int64_t r0 = 0; r0 < n; r0 += batch_rows) {
    const int64_t cnt = std::min(batch_rows, n - r0);
    kmeans_predict<float>(res, src.batch(res, r0, cnt), cnt, dim, idx->centers.data(), (int)n_leaves, idx->labels.data() + r0);
  }

  // 2. AVQ centres
  avq_centers(res, src, idx->labels.data(), n_leaves, p.partitioning_eta, idx->centers.data());

  // 3. SOAR labels
  {
    soar_scratch s(res, batch_rows, dim, n_leaves);
    soar_center_norms(res, idx->centers.data(), n_leaves, dim, s.cn.data());
    for (int64_t r0 = 0; r0 < n; r0 += batch_rows) {
      const int64_t cnt = std::min(batch_rows, n - r0);
      soar_batch(res, src.batch(res, r0, cnt), cnt, dim, idx->centers.data(), n_leaves, idx->labels.data() + r0, p.soar_lambda, s,
                 idx->soar_labels.data() + r0);
    }
    sync(res);
  }

  // 4. PQ codebook on the primary residuals of a strided sample (scann_build.cuh:150-174)
  std::unique_ptr<product_quantizer> q;
  {
    const int64_t m = H::pq_train_rows(p, n), ratio = n / m;
    dev_buf<float> train(res, (size_t)(m * dim));
    HIP_TRY(hipMemcpy2DAsync(train.data(), dim * sizeof(float), data, (size_t)(dim * ratio) * sizeof(float), dim * sizeof(float), m,
                             hipMemcpyDefault, res.stream));
    hipLaunchKernelGGL(scann_sample_residual_kernel, dim3(grid_blocks(m * dim, kThreads)), dim3(kThreads), 0, res.stream, train.data(), m,
                       (int)dim, ratio, idx->labels.data(), idx->centers.data());
    HIP_TRY(hipGetLastError());
    cuvsProductQuantizerParams qp{};
    qp.pq_bits        = p.pq_bits;
    qp.pq_dim         = (uint32_t)idx->n_sub;
    qp.use_subspaces  = true;
    qp.use_vq         = false;
    qp.vq_n_centers   = 0;
    qp.kmeans_n_iters = p.pq_train_iters;
    qp.pq_kmeans_type = CUVS_KMEANS_TYPE_KMEANS_BALANCED;
    qp.max_train_points_per_pq_code    = (uint32_t)(std::min<int64_t>(p.pq_n_rows_train, H::kMaxPqTrainRows) / idx->book_n);
    qp.max_train_points_per_vq_cluster = 1024;
    q = pq_build(res, qp, f32_rows{train.data(), m, dim, true});
  }
  idx->codebook = dev_buf<float>::persistent((size_t)(idx->book_n * dim));
  hipLaunchKernelGGL(scann_codebook_kernel, dim3(grid_blocks(idx->book_n * dim, kThreads)), dim3(kThreads), 0, res.stream, q->pq_book.data(),
                     idx->book_n, (int)idx->n_sub, (int)p.pq_dim, idx->codebook.data());
  HIP_TRY(hipGetLastError());

  // 5. codes of both residuals: the centres serve the encoder as its VQ book (r = x - centre, one fp32 subtraction), so no
  // residual is ever written; 6. the bf16 rows
  q->vq_n    = n_leaves;
  q->vq_book = dev_buf<float>::persistent((size_t)(n_leaves * dim));
  copy_async(res, q->vq_book.data(), idx->centers.data(), (size_t)(n_leaves * dim) * sizeof(float));
  const int64_t cb = q->code_bytes();
  idx->codes.resize((size_t)(n * idx->n_sub));
  idx->soar_codes.resize((size_t)(n * idx->n_sub));
  if (p.reordering_bf16) idx->bf16.resize((size_t)(n * dim));
  dev_buf<uint8_t> packed(res, (size_t)(2 * batch_rows * cb));
  dev_buf<int16_t> bf;
  if (p.reordering_bf16) bf = dev_buf<int16_t>(res, (size_t)(batch_rows * dim));
  std::vector<uint8_t> h_packed((size_t)(2 * batch_rows * cb));
  for (int64_t r0 = 0; r0 < n; r0 += batch_rows) {
    const int64_t cnt = std::min(batch_rows, n - r0);
    const float* x    = src.batch(res, r0, cnt);
    pq_encode(res, *q, x, dim, cnt, idx->labels.data() + r0, packed.data());
    pq_encode(res, *q, x, dim, cnt, idx->soar_labels.data() + r0, packed.data() + batch_rows * cb);
    copy_async(res, h_packed.data(), packed.data(), packed.bytes());
    if (p.reordering_bf16) {
      bf16_batch(res, x, cnt, dim, p.reordering_noise_shaping_threshold, bf.data());
      copy_async(res, idx->bf16.data() + r0 * dim, bf.data(), (size_t)(cnt * dim) * sizeof(int16_t));
    }
    sync(res);
    H::unpack_codes(h_packed.data(), cnt, idx->n_sub, (int)p.pq_bits, idx->codes.data() + r0 * idx->n_sub);
    H::unpack_codes(h_packed.data() + batch_rows * cb, cnt, idx->n_sub, (int)p.pq_bits, idx->soar_codes.data() + r0 * idx->n_sub);
  }
  sync(res);
  return idx;
}

void scann_serialize(resources& res, const scann_index& idx, const char* dir)
{
  if (dir == nullptr) H::refuse("the directory name is null");
  const std::vector<float> centers   = to_host(res, idx.centers.data(), idx.centers.size());
  const std::vector<float> codebook  = to_host(res, idx.codebook.data(), idx.codebook.size());
  const std::vector<uint32_t> labels = to_host(res, idx.labels.data(), idx.labels.size());
  const std::vector<uint32_t> soar   = to_host(res, idx.soar_labels.data(), idx.soar_labels.size());
  H::host_index h;
  h.n_rows = idx.n; h.dim = idx.dim; h.n_leaves = idx.n_leaves; h.n_sub = idx.n_sub; h.book_n = idx.book_n;
  h.pq_dim = idx.p.pq_dim;
  h.centers = centers.data(); h.labels = labels.data(); h.soar = soar.data(); h.codebook = codebook.data();
  h.codes = idx.codes.data(); h.soar_codes = idx.soar_codes.data();
  h.bf16 = idx.p.reordering_bf16 ? idx.bf16.data() : nullptr;
  H::write_files(dir, h);
}

// ================================================================ argument checks of the C layer
struct matrix_arg {
  void* data;
  int64_t rows, cols;
  bool is_host;
};

matrix_arg matrix_of(DLManagedTensor* t, const char* what, uint8_t code, uint8_t bits, bool allow_host, bool want_device = true)
{
  if (t == nullptr) H::refuse("%s must not be NULL", what);
  const DLTensor& d = t->dl_tensor;
  if (!dtype_is(d.dtype, code, bits))
    H::refuse("%s must be %s%d, got DLPack type code %d with %d bits", what, code == kDLFloat ? "fp" : code == kDLInt ? "int" : "uint",
              (int)bits, (int)d.dtype.code, (int)d.dtype.bits);
  if (d.ndim != 2 || d.shape[0] < 0 || d.shape[1] < 1) H::refuse("%s must be a 2-D matrix", what);
  if (!is_c_contiguous(d)) H::refuse("%s must be row-major and contiguous", what);
  const bool dev = is_device_accessible(d);
  if (want_device) {
    if (!dev && !(allow_host && is_host_accessible(d)))
      H::refuse(allow_host ? "%s must be accessible on host or device memory" : "%s must be accessible on device memory", what);
  } else if (!is_host_accessible(d)) {
    H::refuse("%s must be accessible on host memory", what);
  }
  return matrix_arg{dl_data(d), d.shape[0], d.shape[1], !dev};
}

uint32_t* labels_of(DLManagedTensor* t, const char* what, int64_t n)
{
  if (t == nullptr) H::refuse("%s must not be NULL", what);
  const DLTensor& d = t->dl_tensor;
  if (!(dtype_is(d.dtype, kDLUInt, 32) || dtype_is(d.dtype, kDLInt, 32))) H::refuse("%s must be uint32 or int32", what);
  if (d.ndim != 1 || d.shape[0] != n || !is_c_contiguous(d)) H::refuse("%s must be a contiguous vector of length %lld", what, (long long)n);
  if (!is_device_accessible(d)) H::refuse("%s must be accessible on device memory", what);
  return static_cast<uint32_t*>(dl_data(d));
}

scann_index& index_of(cuvsAmdScannIndex_t index)
{
  if (index == nullptr || index->addr == 0) H::refuse("the ScaNN index is not built");
  return *reinterpret_cast<scann_index*>(index->addr);
}

void host_view(DLManagedTensor* out, void* data, DLDataType dt, int64_t rows, int64_t cols)
{
  fill_dl_view(out, data, dt, rows, cols, 2, 0);
  out->dl_tensor.device = DLDevice{kDLCPU, 0};
}

}  // namespace
}  // namespace cuvs_amd

using namespace cuvs_amd;

extern "C" {

cuvsError_t cuvsAmdScannIndexParamsCreate(cuvsAmdScannIndexParams_t* params)
{
  return (cuvsError_t)translate_exceptions([=] {
    CUVS_EXPECTS(params != nullptr, "params is null");
    const H::params d;
    *params = new cuvsAmdScannIndexParams{L2Expanded,
                                          d.metric_arg,
                                          d.n_leaves,
                                          d.kmeans_n_rows_train,
                                          d.kmeans_n_iters,
                                          d.partitioning_eta,
                                          d.soar_lambda,
                                          d.pq_dim,
                                          d.pq_bits,
                                          d.pq_n_rows_train,
                                          d.pq_train_iters,
                                          d.reordering_bf16,
                                          d.reordering_noise_shaping_threshold};
  });
}

cuvsError_t cuvsAmdScannIndexParamsDestroy(cuvsAmdScannIndexParams_t params)
{
  return (cuvsError_t)translate_exceptions([=] { delete params; });
}

cuvsError_t cuvsAmdScannIndexCreate(cuvsAmdScannIndex_t* index)
{
  return (cuvsError_t)translate_exceptions([=] {
    CUVS_EXPECTS(index != nullptr, "index is null");
    *index = new cuvsAmdScannIndex{0};
  });
}

cuvsError_t cuvsAmdScannIndexDestroy(cuvsAmdScannIndex_t index)
{
  return (cuvsError_t)translate_exceptions([=] {
    if (index == nullptr) return;
    delete reinterpret_cast<scann_index*>(index->addr);
    delete index;
  });
}

cuvsError_t cuvsAmdScannBuild(cuvsResources_t res_h, cuvsAmdScannIndexParams_t params, DLManagedTensor* dataset, cuvsAmdScannIndex_t index)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& res = *as_res(res_h);
    if (params == nullptr || index == nullptr) H::refuse("params and index must not be NULL");
    const matrix_arg ds = matrix_of(dataset, "dataset", kDLFloat, 32, true);
    H::params p;
    p.metric              = (int)params->metric;
    p.metric_arg          = params->metric_arg;
    p.n_leaves            = params->n_leaves;
    p.kmeans_n_rows_train = params->kmeans_n_rows_train;
    p.kmeans_n_iters      = params->kmeans_n_iters;
    p.partitioning_eta    = params->partitioning_eta;
    p.soar_lambda         = params->soar_lambda;
    p.pq_dim              = params->pq_dim;
    p.pq_bits             = params->pq_bits;
    p.pq_n_rows_train     = params->pq_n_rows_train;
    p.pq_train_iters      = params->pq_train_iters;
    p.reordering_bf16     = params->reordering_bf16;
    p.reordering_noise_shaping_threshold = params->reordering_noise_shaping_threshold;
    auto built = scann_build(res, p, static_cast<const float*>(ds.data), ds.rows, ds.cols, ds.is_host);
    delete reinterpret_cast<scann_index*>(index->addr);
    index->addr = reinterpret_cast<uintptr_t>(built.release());
  });
}

cuvsError_t cuvsAmdScannSerialize(cuvsResources_t res_h, const char* dir, cuvsAmdScannIndex_t index)
{
  return (cuvsError_t)translate_exceptions([=] { scann_serialize(*as_res(res_h), index_of(index), dir); });
}

#define SCANN_GETTER(NAME, TYPE, EXPR)                                             \
  cuvsError_t NAME(cuvsAmdScannIndex_t index, TYPE* out)                           \
  {                                                                                \
    return (cuvsError_t)translate_exceptions([=] {                                 \
      CUVS_EXPECTS(out != nullptr, "output pointer is null");                      \
      const scann_index& idx = index_of(index);                                    \
      *out                   = (EXPR);                                             \
    });                                                                            \
  }
SCANN_GETTER(cuvsAmdScannIndexGetSize, int64_t, idx.n)
SCANN_GETTER(cuvsAmdScannIndexGetDim, int64_t, idx.dim)
SCANN_GETTER(cuvsAmdScannIndexGetNLeaves, int64_t, idx.n_leaves)
SCANN_GETTER(cuvsAmdScannIndexGetPqDim, int64_t, (int64_t)idx.p.pq_dim)
SCANN_GETTER(cuvsAmdScannIndexGetPqBits, int64_t, (int64_t)idx.p.pq_bits)
SCANN_GETTER(cuvsAmdScannIndexHasBf16, bool, idx.p.reordering_bf16)
#undef SCANN_GETTER

cuvsError_t cuvsAmdScannIndexGetCenters(cuvsAmdScannIndex_t index, DLManagedTensor* out)
{
  return (cuvsError_t)translate_exceptions([=] {
    scann_index& idx = index_of(index);
    fill_dl_view(out, idx.centers.data(), DLDataType{kDLFloat, 32, 1}, idx.n_leaves, idx.dim, 2, idx.device);
  });
}
cuvsError_t cuvsAmdScannIndexGetLabels(cuvsAmdScannIndex_t index, DLManagedTensor* out)
{
  return (cuvsError_t)translate_exceptions([=] {
    scann_index& idx = index_of(index);
    fill_dl_view(out, idx.labels.data(), DLDataType{kDLUInt, 32, 1}, idx.n, 1, 1, idx.device);
  });
}
cuvsError_t cuvsAmdScannIndexGetSoarLabels(cuvsAmdScannIndex_t index, DLManagedTensor* out)
{
  return (cuvsError_t)translate_exceptions([=] {
    scann_index& idx = index_of(index);
    fill_dl_view(out, idx.soar_labels.data(), DLDataType{kDLUInt, 32, 1}, idx.n, 1, 1, idx.device);
  });
}
cuvsError_t cuvsAmdScannIndexGetPqCodebook(cuvsAmdScannIndex_t index, DLManagedTensor* out)
{
  return (cuvsError_t)translate_exceptions([=] {
    scann_index& idx = index_of(index);
    fill_dl_view(out, idx.codebook.data(), DLDataType{kDLFloat, 32, 1}, idx.book_n, idx.dim, 2, idx.device);
  });
}
cuvsError_t cuvsAmdScannIndexGetCodes(cuvsAmdScannIndex_t index, DLManagedTensor* out)
{
  return (cuvsError_t)translate_exceptions([=] {
    scann_index& idx = index_of(index);
    host_view(out, idx.codes.data(), DLDataType{kDLUInt, 8, 1}, idx.n, idx.n_sub);
  });
}
cuvsError_t cuvsAmdScannIndexGetSoarCodes(cuvsAmdScannIndex_t index, DLManagedTensor* out)
{
  return (cuvsError_t)translate_exceptions([=] {
    scann_index& idx = index_of(index);
    host_view(out, idx.soar_codes.data(), DLDataType{kDLUInt, 8, 1}, idx.n, idx.n_sub);
  });
}
cuvsError_t cuvsAmdScannIndexGetBf16Dataset(cuvsAmdScannIndex_t index, DLManagedTensor* out)
{
  return (cuvsError_t)translate_exceptions([=] {
    scann_index& idx = index_of(index);
    if (!idx.p.reordering_bf16) H::refuse("the index was built without reordering_bf16");
    host_view(out, idx.bf16.data(), DLDataType{kDLInt, 16, 1}, idx.n, idx.dim);
  });
}

cuvsError_t cuvsAmdScannAvqCenters(cuvsResources_t res_h, DLManagedTensor* dataset, DLManagedTensor* labels, DLManagedTensor* centers_inout,
                                   float eta)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& res = *as_res(res_h);
    H::check_eta(eta);
    const matrix_arg ds = matrix_of(dataset, "dataset", kDLFloat, 32, false);
    const matrix_arg c  = matrix_of(centers_inout, "centers", kDLFloat, 32, false);
    if (c.cols != ds.cols) H::refuse("centers have %lld columns, the dataset has %lld", (long long)c.cols, (long long)ds.cols);
    if (c.rows < 1) H::refuse("n_leaves must be at least 1");
    const uint32_t* lab = labels_of(labels, "labels", ds.rows);
    if (ds.rows == 0) return;
    check_label_range(res, lab, ds.rows, c.rows);
    row_source src{static_cast<const float*>(ds.data), ds.rows, ds.cols, false, {}};
    avq_centers(res, src, lab, c.rows, eta, static_cast<float*>(c.data));
  });
}

cuvsError_t cuvsAmdScannSoarLabels(cuvsResources_t res_h, DLManagedTensor* dataset, DLManagedTensor* centers, DLManagedTensor* labels,
                                   float lambda, DLManagedTensor* soar_labels_out)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& res = *as_res(res_h);
    H::check_lambda(lambda);
    const matrix_arg ds = matrix_of(dataset, "dataset", kDLFloat, 32, false);
    const matrix_arg c  = matrix_of(centers, "centers", kDLFloat, 32, false);
    if (c.cols != ds.cols) H::refuse("centers have %lld columns, the dataset has %lld", (long long)c.cols, (long long)ds.cols);
    if (c.rows < 1) H::refuse("n_leaves must be at least 1");
    const uint32_t* lab = labels_of(labels, "labels", ds.rows);
    uint32_t* out       = labels_of(soar_labels_out, "soar_labels", ds.rows);
    if (ds.rows == 0) return;
    check_label_range(res, lab, ds.rows, c.rows);
    const int64_t batch_rows = std::min(ds.rows, H::kMaxBatchRows);
    soar_scratch s(res, batch_rows, ds.cols, c.rows);
    soar_center_norms(res, static_cast<const float*>(c.data), c.rows, ds.cols, s.cn.data());
    for (int64_t r0 = 0; r0 < ds.rows; r0 += batch_rows) {
      const int64_t cnt = std::min(batch_rows, ds.rows - r0);
      soar_batch(res, static_cast<const float*>(ds.data) + r0 * ds.cols, cnt, ds.cols, static_cast<const float*>(c.data), c.rows, lab + r0,
                 lambda, s, out + r0);
    }
    sync(res);
  });
}

cuvsError_t cuvsAmdScannQuantizeBf16(cuvsResources_t res_h, DLManagedTensor* dataset, float threshold, DLManagedTensor* out)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& res = *as_res(res_h);
    const matrix_arg ds = matrix_of(dataset, "dataset", kDLFloat, 32, false);
    const matrix_arg o  = matrix_of(out, "out", kDLInt, 16, false);
    if (o.rows != ds.rows || o.cols != ds.cols) H::refuse("out must have shape [%lld, %lld]", (long long)ds.rows, (long long)ds.cols);
    if (threshold < 0.f || std::isinf(threshold)) H::refuse("the noise shaping threshold must be non-negative and finite, or NaN");
    bf16_batch(res, static_cast<const float*>(ds.data), ds.rows, ds.cols, threshold, static_cast<int16_t*>(o.data));
    sync(res);
  });
}

}  // extern "C"
