// Product quantizer (drop-in for c/src/preprocessing/quantize/pq.cpp; semantics of
// cpp/src/preprocessing/quantize/detail/pq.cuh and cpp/src/neighbors/detail/vpq_dataset.cuh): fp32 rows [n, dim] ->
// pq_dim codes of pq_bits bits per row, optionally on the residual to a VQ (k-means) centre.
//
// Canonical arithmetic of the encoder, for row i and subspace j:
//   r_k = x[i, j * pq_len + k] (- vq[label_i, j * pq_len + k], one fp32 subtraction, with VQ)
//   d(c) = fmaf chain over k = 0 .. pq_len - 1 of t_k * t_k, t_k = r_k - book[c, k], from 0
//   code = the lowest c with minimal d
// Code j occupies bits [j * pq_bits, (j + 1) * pq_bits) of the row's bytes, little endian; every byte is stored once.
//
// Two encoders return the same bytes:
//   pq_encode_plain_kernel: the above written down (a lane per row, a loop over the book read from memory);
//     CUVS_AMD_PQ_ENCODE=plain selects it for every shape. Comparator of the tests, baseline of the timing.
//   pq_encode_kernel<PL, R>: the same arithmetic in the same order, organised for reuse. A 256-lane workgroup owns 256 R rows
//     and walks the subspaces; per subspace the book (or a 32 KB tile of it: 65536 entries at 16 bits) is staged once in LDS,
//     pq_len padded to PL with zeros (t = 0 - 0, fmaf(0, 0, d) = d: the chain is bitwise unchanged). A lane keeps the R
//     residual pieces in registers and reads each book entry once (an LDS broadcast: all lanes read the same address) for R
//     distances, so an entry costs PL / 4 LDS reads against 2 R PL vector operations. No screening and no re-scoring: there is
//     nothing to prove beyond the order of the operations. The packed codes stay in a 64-bit register per row and leave as
//     4-byte (or 1-byte) stores.
// Fallback rule (pq_use_default): pq_len <= 32 goes through pq_encode_kernel, pq_len > 32 through the plain kernel (R * PL
// residual registers no longer fit without scratch).
//
// Training follows the reference: strided trainsets, VQ by hierarchical balanced k-means, PQ codebooks by the flat balanced EM
// (kmeans_build_clusters) or by Lloyd iterations from k-means++ seeds (cuvsKMeansFit), one run per subspace.
#include "common.hpp"
#include "device_utils.hpp"
#include "ops.hpp"
#include "pq_quantize.hpp"

#include <cuvs/cluster/kmeans.h>
#include <cuvs_amd/extensions.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <limits>
#include <vector>

namespace cuvs_amd {
namespace {

const DLDataType kPqF32{kDLFloat, 32, 1};

std::atomic<unsigned long long> g_encode_launches[3];  // default (any R), plain, default with R > 1 rows per lane

// ---------------------------------------------------------------- encoders
struct encode_args {
  const float* x;       // [n, dim], row pitch ld
  int64_t ld, n;
  int dim, pq_dim, pq_len, pq_bits;
  int book_n;
  int64_t book_stride;  // floats between the books of consecutive subspaces (0: one shared book)
  const float* book;
  const float* vq;            // [vq_n, dim] or nullptr
  const uint32_t* labels;     // [n] (with vq)
  uint8_t* codes;             // [n, code_bytes]
  int code_bytes;
  int w32;                    // rows of codes are 4-byte aligned: full words leave as one store
};

// appends `bits` bits to a row's register at position (nb, ob) and stores what is complete; pq_advance moves the position
__device__ __forceinline__ void pq_push_code(unsigned long long& acc, int nb, int ob, uint8_t* o, uint32_t code, int bits, int w32)
{
  acc |= (unsigned long long)code << nb;
  nb += bits;
  if (w32) {
    if (nb >= 32) {
      *reinterpret_cast<uint32_t*>(o + ob) = (uint32_t)acc;
      acc >>= 32;
    }
  } else {
    while (nb >= 8) {
      o[ob++] = (uint8_t)acc;
      acc >>= 8; nb -= 8;
    }
  }
}
__device__ __forceinline__ void pq_advance(int& nb, int& ob, int bits, int w32)
{
  nb += bits;
  if (w32) {
    if (nb >= 32) { nb -= 32; ob += 4; }
  } else {
    ob += nb >> 3;
    nb &= 7;
  }
}
__device__ __forceinline__ void pq_flush_codes(unsigned long long acc, int nb, int ob, uint8_t* o)
{
  while (nb > 0) {  // the unused high bits of the last byte are zero
    o[ob++] = (uint8_t)acc;
    acc >>= 8; nb -= 8;
  }
}

__global__ __launch_bounds__(256) void pq_encode_plain_kernel(encode_args a)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  const float* xr = a.x + i * a.ld;
  const float* vr = a.vq != nullptr ? a.vq + (int64_t)a.labels[i] * a.dim : nullptr;
  uint8_t* o      = a.codes + i * a.code_bytes;
  unsigned long long acc = 0;
  int nb = 0, ob = 0;
  for (int j = 0; j < a.pq_dim; ++j) {
    const float* b = a.book + (int64_t)j * a.book_stride;
    float best     = std::numeric_limits<float>::infinity();
    uint32_t code  = 0;
    for (int c = 0; c < a.book_n; ++c) {
      float d = 0.f;
      for (int k = 0; k < a.pq_len; ++k) {
        float r = xr[j * a.pq_len + k];
        if (vr != nullptr) r = r - vr[j * a.pq_len + k];
        const float t = r - b[(int64_t)c * a.pq_len + k];
        d             = __fmaf_rn(t, t, d);
      }
      if (d < best) { best = d; code = (uint32_t)c; }
    }
    pq_push_code(acc, nb, ob, o, code, a.pq_bits, 0);
    pq_advance(nb, ob, a.pq_bits, 0);
  }
  pq_flush_codes(acc, nb, ob, o);
}

constexpr int kPqTileFloats = 8192;  // 32 KB of LDS for the book tile

template <int PL, int R>
__global__ __launch_bounds__(256) void pq_encode_kernel(encode_args a)
{
  __shared__ float tile[kPqTileFloats];
  constexpr int kTileC = kPqTileFloats / PL;
  const int tid        = threadIdx.x;
  int64_t row[R];
  bool live[R];
  const float* xr[R];
  const float* vr[R];
  uint8_t* o[R];
  unsigned long long acc[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int64_t i = ((int64_t)blockIdx.x * R + r) * 256 + tid;
    live[r]         = i < a.n;
    row[r]          = live[r] ? i : a.n - 1;  // lanes past the end redo the last row and store nothing
    xr[r]           = a.x + row[r] * a.ld;
    vr[r]           = a.vq != nullptr ? a.vq + (int64_t)a.labels[row[r]] * a.dim : nullptr;
    o[r]            = a.codes + row[r] * a.code_bytes;
    acc[r]          = 0;
  }
  int nb = 0, ob = 0;
  // whole 16-byte pieces of the row when the pieces are aligned
  const bool vec = PL >= 4 && a.pq_len == PL && (a.ld & 3) == 0 && (reinterpret_cast<uintptr_t>(a.x) & 15) == 0 &&
                   (a.vq == nullptr || ((a.dim & 3) == 0 && (reinterpret_cast<uintptr_t>(a.vq) & 15) == 0));
  for (int j = 0; j < a.pq_dim; ++j) {
    float res[R][PL];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (vec) {
        if constexpr (PL >= 4) {
#pragma unroll
          for (int k = 0; k < PL; k += 4) {
            const float4 v = *reinterpret_cast<const float4*>(xr[r] + j * PL + k);
            res[r][k] = v.x; res[r][k + 1] = v.y; res[r][k + 2] = v.z; res[r][k + 3] = v.w;
          }
          if (vr[r] != nullptr) {
#pragma unroll
            for (int k = 0; k < PL; k += 4) {
              const float4 v = *reinterpret_cast<const float4*>(vr[r] + j * PL + k);
              res[r][k] = res[r][k] - v.x; res[r][k + 1] = res[r][k + 1] - v.y;
              res[r][k + 2] = res[r][k + 2] - v.z; res[r][k + 3] = res[r][k + 3] - v.w;
            }
          }
        }
      } else {
#pragma unroll
        for (int k = 0; k < PL; ++k) {
          float v = 0.f;
          if (k < a.pq_len) {
            v = xr[r][j * a.pq_len + k];
            if (vr[r] != nullptr) v = v - vr[r][j * a.pq_len + k];
          }
          res[r][k] = v;
        }
      }
    }
    float best[R];
    uint32_t code[R];
#pragma unroll
    for (int r = 0; r < R; ++r) { best[r] = std::numeric_limits<float>::infinity(); code[r] = 0; }
    const float* b = a.book + (int64_t)j * a.book_stride;
    for (int c0 = 0; c0 < a.book_n; c0 += kTileC) {
      const int cn = min(kTileC, a.book_n - c0);
      __syncthreads();  // the previous tile is no longer read
      for (int e = tid; e < cn * PL; e += 256) {
        const int c = e / PL, k = e - c * PL;
        tile[e]     = k < a.pq_len ? b[(int64_t)(c0 + c) * a.pq_len + k] : 0.f;
      }
      __syncthreads();
#pragma unroll 2
      for (int c = 0; c < cn; ++c) {
        float bk[PL];
#pragma unroll
        for (int k = 0; k < PL; ++k) bk[k] = tile[c * PL + k];
#pragma unroll
        for (int r = 0; r < R; ++r) {
          float d = 0.f;
#pragma unroll
          for (int k = 0; k < PL; ++k) {
            const float t = res[r][k] - bk[k];
            d             = __fmaf_rn(t, t, d);
          }
          if (d < best[r]) { best[r] = d; code[r] = (uint32_t)(c0 + c); }
        }
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r)
      if (live[r]) pq_push_code(acc[r], nb, ob, o[r], code[r], a.pq_bits, a.w32);
    pq_advance(nb, ob, a.pq_bits, a.w32);
  }
#pragma unroll
  for (int r = 0; r < R; ++r)
    if (live[r]) pq_flush_codes(acc[r], nb, ob, o[r]);
}

// the one place that decides which encoder a shape gets
inline bool pq_use_default(const tuning& t, int64_t pq_len) { return !t.pq_encode_plain && pq_len <= 32; }

template <int PL, int RMAX>
void pq_launch_default(resources& res, const encode_args& a)
{
  // R rows per lane when that still gives every CU two workgroups, else one row per lane
  const int64_t blocks_r = (a.n + 256 * RMAX - 1) / (256 * RMAX);
  if (blocks_r >= 2 * (int64_t)res.num_cus) {
    g_encode_launches[2]++;
    hipLaunchKernelGGL((pq_encode_kernel<PL, RMAX>), dim3(grid_blocks(a.n, 256 * RMAX)), dim3(256), 0, res.stream, a);
  } else {
    hipLaunchKernelGGL((pq_encode_kernel<PL, 1>), dim3(grid_blocks(a.n, 256)), dim3(256), 0, res.stream, a);
  }
}

}  // namespace

void pq_encode(resources& res, const product_quantizer& q, const float* x, int64_t ld, int64_t n, const uint32_t* labels,
               uint8_t* codes)
{
  if (n == 0) return;
  encode_args a{};
  a.x = x; a.ld = ld; a.n = n;
  a.dim = (int)q.dim; a.pq_dim = (int)q.p.pq_dim; a.pq_len = (int)q.pq_len; a.pq_bits = (int)q.p.pq_bits;
  a.book_n      = (int)q.book_n;
  a.book_stride = q.p.use_subspaces ? q.book_n * q.pq_len : 0;
  a.book        = q.pq_book.data();
  a.vq          = q.vq_n > 0 ? q.vq_book.data() : nullptr;
  a.labels      = labels;
  a.codes       = codes;
  a.code_bytes  = (int)q.code_bytes();
  a.w32         = (a.code_bytes % 4 == 0 && reinterpret_cast<uintptr_t>(codes) % 4 == 0) ? 1 : 0;
  if (!pq_use_default(res.tune, q.pq_len)) {
    profile_begin(res, "pq_encode_plain_kernel");
    hipLaunchKernelGGL(pq_encode_plain_kernel, dim3(grid_blocks(n, 256)), dim3(256), 0, res.stream, a);
    profile_end(res, "pq_encode_plain_kernel");
    g_encode_launches[1]++;
  } else {
    profile_begin(res, "pq_encode_kernel");
    const int pl = (int)q.pq_len;
    if (pl <= 1)       pq_launch_default<1, 4>(res, a);
    else if (pl <= 2)  pq_launch_default<2, 4>(res, a);
    else if (pl <= 4)  pq_launch_default<4, 4>(res, a);
    else if (pl <= 8)  pq_launch_default<8, 4>(res, a);
    else if (pl <= 16) pq_launch_default<16, 2>(res, a);
    else               pq_launch_default<32, 2>(res, a);
    profile_end(res, "pq_encode_kernel");
    g_encode_launches[0]++;
  }
  HIP_TRY(hipGetLastError());
}

namespace {

// ---------------------------------------------------------------- decoder
// a lane writes V consecutive columns of one subspace: rows leave as coalesced 4 V-byte stores; the book is read through the
// caches (a subspace's book is 8 KB at 8 bits x pq_len 8)
template <int V>
__global__ __launch_bounds__(256) void pq_decode_kernel(const uint8_t* __restrict__ codes, int code_bytes, int64_t n, int dim,
                                                        int pq_len, int pq_bits, const float* __restrict__ book,
                                                        int64_t book_stride, const float* __restrict__ vq,
                                                        const uint32_t* __restrict__ labels, float* __restrict__ out)
{
  const int per_row   = dim / V;
  const int64_t total = n * per_row;
  const uint32_t mask = (1u << pq_bits) - 1u;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = t / per_row;
    const int col   = (int)(t - i * per_row) * V;
    const int j = col / pq_len, k = col - j * pq_len;
    const int bit        = j * pq_bits;
    const uint8_t* c     = codes + i * code_bytes;
    const int b0         = bit >> 3;
    uint32_t w           = c[b0];
    if (b0 + 1 < code_bytes) w |= (uint32_t)c[b0 + 1] << 8;
    if (b0 + 2 < code_bytes) w |= (uint32_t)c[b0 + 2] << 16;
    const uint32_t code  = (w >> (bit & 7)) & mask;
    const float* src     = book + (int64_t)j * book_stride + (int64_t)code * pq_len + k;
    float v[V];
#pragma unroll
    for (int u = 0; u < V; ++u) v[u] = src[u];
    if (vq != nullptr) {
      const float* vs = vq + (int64_t)labels[i] * dim + col;
#pragma unroll
      for (int u = 0; u < V; ++u) v[u] = v[u] + vs[u];
    }
    float* dst = out + i * dim + col;
    if constexpr (V == 4) *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
    else dst[0] = v[0];
  }
}

// ---------------------------------------------------------------- training
__global__ void pq_subtract_centers_kernel(float* __restrict__ x, int64_t n, int dim, const uint32_t* __restrict__ labels,
                                           const float* __restrict__ centers)
{
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * dim) return;
  const int64_t i = t / dim;
  x[t]            = x[t] - centers[(int64_t)labels[i] * dim + (t - i * dim)];
}

__global__ void pq_gather_columns_kernel(const float* __restrict__ x, int64_t n, int64_t ld, int cols, float* __restrict__ out)
{
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * cols) return;
  const int64_t i = t / cols;
  out[t]          = x[i * ld + (t - i * cols)];
}

// vpq_dataset.cuh:44-69: row i * (n / n_samples) of the dataset is sample i (host or device rows)
void pq_subsample(resources& res, const float* x, int64_t ld, int64_t n, int64_t dim, int64_t n_samples, float* out)
{
  const int64_t ratio = n / n_samples;
  HIP_TRY(hipMemcpy2DAsync(out, dim * sizeof(float), x, ld * ratio * sizeof(float), dim * sizeof(float), n_samples, hipMemcpyDefault,
                           res.stream));
}

DLManagedTensor pq_dl_matrix(float* data, int64_t* shape)
{
  DLManagedTensor t{};
  t.dl_tensor.data   = data;
  t.dl_tensor.device = DLDevice{kDLROCM, 0};
  t.dl_tensor.ndim   = 2;
  t.dl_tensor.dtype  = kPqF32;
  t.dl_tensor.shape  = shape;
  return t;
}

// one PQ codebook [book_n, pq_len] from rows x [n, pq_len] with pitch ld
void pq_train_book(resources& res, const product_quantizer& q, const float* x, int64_t n, int64_t ld, float* centers,
                   dev_buf<float>& packed, dev_buf<uint32_t>& labels, dev_buf<uint32_t>& sizes)
{
  const int pq_len = (int)q.pq_len, book_n = (int)q.book_n;
  if (q.p.pq_kmeans_type == CUVS_KMEANS_TYPE_KMEANS_BALANCED) {
    kmeans_build_clusters(res, x, n, ld, pq_len, book_n, (int)q.p.kmeans_n_iters, centers, labels.data(), sizes.data());
    return;
  }
  // classic k-means as the reference's C entry point configures it (pq.hpp:53-57: cluster::kmeans::params with n_clusters and
  // max_iter set, everything else default, so the seeding is k-means++ and tol 1e-4)
  const float* xc = x;
  if (ld != pq_len) {
    hipLaunchKernelGGL(pq_gather_columns_kernel, dim3(grid_blocks(n * pq_len, 256)), dim3(256), 0, res.stream, x, n, ld, pq_len,
                       packed.data());
    HIP_TRY(hipGetLastError());
    xc = packed.data();
  }
  cuvsKMeansParams_t kp = nullptr;
  CUVS_EXPECTS(cuvsKMeansParamsCreate(&kp) == CUVS_SUCCESS, "%s", last_error_text().c_str());
  kp->n_clusters = book_n;
  kp->max_iter   = (int)q.p.kmeans_n_iters;
  int64_t xs[2] = {n, pq_len}, cs[2] = {book_n, pq_len};
  DLManagedTensor xt = pq_dl_matrix(const_cast<float*>(xc), xs), ct = pq_dl_matrix(centers, cs);
  double inertia = 0;
  int n_iter     = 0;
  const cuvsError_t e = cuvsKMeansFit(reinterpret_cast<cuvsResources_t>(&res), kp, &xt, nullptr, &ct, &inertia, &n_iter);
  cuvsKMeansParamsDestroy(kp);
  CUVS_EXPECTS(e == CUVS_SUCCESS, "%s", last_error_text().c_str());
}

f32_rows pq_dataset_view(DLManagedTensor* t)
{
  CUVS_EXPECTS(t != nullptr, "null argument");
  const DLTensor& d = t->dl_tensor;
  CUVS_EXPECTS(dtype_is(d.dtype, kDLFloat, 32), "Unsupported dataset DLtensor dtype: %d and bits: %d", (int)d.dtype.code,
               (int)d.dtype.bits);
  CUVS_EXPECTS(d.ndim == 2 && d.shape[1] > 0, "dataset must be a 2-D matrix");
  CUVS_EXPECTS(is_c_contiguous(d), "dataset must be row-major and contiguous");
  CUVS_EXPECTS(is_device_accessible(d) || is_host_accessible(d), "dataset must be accessible on host or device memory");
  return f32_rows{static_cast<const float*>(dl_data(d)), d.shape[0], d.shape[1], is_device_accessible(d)};
}

void pq_check_params(const cuvsProductQuantizerParams& p)
{
  CUVS_EXPECTS(p.pq_bits >= 4 && p.pq_bits <= 16, "PQ bits must be within [4, 16], got %u", p.pq_bits);
  CUVS_EXPECTS(p.pq_kmeans_type == CUVS_KMEANS_TYPE_KMEANS || p.pq_kmeans_type == CUVS_KMEANS_TYPE_KMEANS_BALANCED,
               "unknown pq_kmeans_type %d", (int)p.pq_kmeans_type);
}

}  // namespace

std::unique_ptr<product_quantizer> pq_build(resources& res, const cuvsProductQuantizerParams& params, const f32_rows& ds)
{
  pq_check_params(params);
  auto q     = std::make_unique<product_quantizer>();
  q->p       = params;
  const int64_t n = ds.n, dim = ds.dim;
  // pq.cuh:24-30
  if (q->p.pq_dim == 0) q->p.pq_dim = (uint32_t)((dim + 3) / 4);
  if (q->p.vq_n_centers == 0) q->p.vq_n_centers = (uint32_t)round_up((int64_t)std::sqrt((double)n), 8);
  CUVS_EXPECTS(dim % q->p.pq_dim == 0, "Dimension must be divisible by pq_dim");
  q->dim    = dim;
  q->pq_len = dim / q->p.pq_dim;
  q->book_n = int64_t(1) << q->p.pq_bits;
  const int64_t n_train = std::min<int64_t>(n, (int64_t)q->p.max_train_points_per_pq_code * q->book_n);
  CUVS_EXPECTS(n_train >= q->book_n, "The number of training samples must be equal to or greater than the number of PQ centers");
  CUVS_EXPECTS(q->p.kmeans_n_iters > 0, "kmeans_n_iters must be positive");

  if (q->p.use_vq) {
    q->vq_n = q->p.vq_n_centers;
    const int64_t n_vq_train = std::min<int64_t>(n, (int64_t)q->p.max_train_points_per_vq_cluster * q->vq_n);
    CUVS_EXPECTS(n_vq_train >= q->vq_n, "The number of VQ training samples (%lld) must not be smaller than vq_n_centers (%lld)",
                 (long long)n_vq_train, (long long)q->vq_n);
    dev_buf<float> vq_train(res, (size_t)(n_vq_train * dim));
    pq_subsample(res, ds.data, dim, n, dim, n_vq_train, vq_train.data());
    q->vq_book = dev_buf<float>::persistent((size_t)(q->vq_n * dim));
    kmeans_params kp;
    kp.n_iters = (int)q->p.kmeans_n_iters;
    kmeans_balanced_fit(res, vq_train.data(), n_vq_train, dim, (int)q->vq_n, kp, q->vq_book.data());
  }

  dev_buf<float> train(res, (size_t)(n_train * dim));
  pq_subsample(res, ds.data, dim, n, dim, n_train, train.data());
  if (q->vq_n > 0) {
    dev_buf<uint32_t> labels(res, (size_t)n_train);
    kmeans_predict<float>(res, train.data(), n_train, dim, q->vq_book.data(), (int)q->vq_n, labels.data());
    hipLaunchKernelGGL(pq_subtract_centers_kernel, dim3(grid_blocks(n_train * dim, 256)), dim3(256), 0, res.stream, train.data(),
                       n_train, (int)dim, labels.data(), q->vq_book.data());
    HIP_TRY(hipGetLastError());
  }
  const bool classic = q->p.pq_kmeans_type == CUVS_KMEANS_TYPE_KMEANS;
  dev_buf<uint32_t> sizes(res, (size_t)q->book_n);
  if (q->p.use_subspaces) {
    q->pq_book = dev_buf<float>::persistent((size_t)(q->p.pq_dim * q->book_n * q->pq_len));
    dev_buf<uint32_t> labels(res, (size_t)n_train);
    dev_buf<float> packed;
    if (classic && q->p.pq_dim > 1) packed = dev_buf<float>(res, (size_t)(n_train * q->pq_len));
    for (uint32_t m = 0; m < q->p.pq_dim; ++m)
      pq_train_book(res, *q, train.data() + (int64_t)m * q->pq_len, n_train, dim, q->pq_book.data() + (int64_t)m * q->book_n * q->pq_len,
                    packed, labels, sizes);
  } else {
    q->pq_book = dev_buf<float>::persistent((size_t)(q->book_n * q->pq_len));
    dev_buf<uint32_t> labels(res, (size_t)(n_train * q->p.pq_dim));
    dev_buf<float> packed;
    pq_train_book(res, *q, train.data(), n_train * q->p.pq_dim, q->pq_len, q->pq_book.data(), packed, labels, sizes);
  }
  sync(res);
  return q;
}

namespace {

product_quantizer& get_pq(cuvsProductQuantizer_t q)
{
  CUVS_EXPECTS(q != nullptr && q->addr != 0, "product quantizer is not built");
  return *reinterpret_cast<product_quantizer*>(q->addr);
}

uint32_t* pq_labels_view(DLManagedTensor* t, int64_t n)
{
  const DLTensor& d = t->dl_tensor;
  CUVS_EXPECTS(is_device_accessible(d), "vq_labels must be accessible on device memory");
  CUVS_EXPECTS(dtype_is(d.dtype, kDLUInt, 32), "vq_labels must be uint32");
  CUVS_EXPECTS(d.ndim == 1 && d.shape[0] == n && is_c_contiguous(d), "vq_labels must be a contiguous vector of length %lld",
               (long long)n);
  return static_cast<uint32_t*>(dl_data(d));
}

uint8_t* pq_codes_view(DLManagedTensor* t, const product_quantizer& q, int64_t* n)
{
  CUVS_EXPECTS(t != nullptr, "null argument");
  const DLTensor& d = t->dl_tensor;
  CUVS_EXPECTS(is_device_accessible(d), "codes must be accessible on device memory");
  CUVS_EXPECTS(dtype_is(d.dtype, kDLUInt, 8), "codes must be uint8");
  CUVS_EXPECTS(d.ndim == 2 && is_c_contiguous(d), "codes must be a row-major contiguous matrix");
  CUVS_EXPECTS(d.shape[1] == q.code_bytes(), "codes must have %lld columns but have %lld", (long long)q.code_bytes(),
               (long long)d.shape[1]);
  *n = d.shape[0];
  return static_cast<uint8_t*>(dl_data(d));
}

void pq_transform(resources& res, const product_quantizer& q, const f32_rows& ds, DLManagedTensor* codes_t, DLManagedTensor* labels_t)
{
  CUVS_EXPECTS(ds.dim == q.dim, "dataset has %lld columns, the quantizer was built for %lld", (long long)ds.dim, (long long)q.dim);
  int64_t n_codes = 0;
  uint8_t* codes  = pq_codes_view(codes_t, q, &n_codes);
  CUVS_EXPECTS(n_codes == ds.n, "codes must have %lld rows but have %lld", (long long)ds.n, (long long)n_codes);
  uint32_t* labels = nullptr;
  dev_buf<uint32_t> own_labels;
  if (q.vq_n > 0) {
    if (labels_t != nullptr) labels = pq_labels_view(labels_t, ds.n);
    else { own_labels = dev_buf<uint32_t>(res, (size_t)ds.n); labels = own_labels.data(); }
  }
  if (ds.n == 0) return;
  // host rows are staged through the device in chunks of about 256 MB
  const int64_t chunk = ds.device ? ds.n : std::max<int64_t>(1, std::min<int64_t>(ds.n, (int64_t(256) << 20) / (ds.dim * 4)));
  dev_buf<float> staged;
  if (!ds.device) staged = dev_buf<float>(res, (size_t)(chunk * ds.dim));
  for (int64_t r0 = 0; r0 < ds.n; r0 += chunk) {
    const int64_t cnt = std::min(chunk, ds.n - r0);
    const float* x    = ds.data + r0 * ds.dim;
    if (!ds.device) {
      copy_async(res, staged.data(), x, (size_t)(cnt * ds.dim) * sizeof(float));
      x = staged.data();
    }
    if (q.vq_n > 0) kmeans_predict<float>(res, x, cnt, ds.dim, q.vq_book.data(), (int)q.vq_n, labels + r0);
    pq_encode(res, q, x, ds.dim, cnt, labels != nullptr ? labels + r0 : nullptr, codes + r0 * q.code_bytes());
    if (!ds.device) sync(res);  // the staging buffer is reused
  }
  sync(res);
}

void pq_inverse(resources& res, const product_quantizer& q, DLManagedTensor* codes_t, DLManagedTensor* out_t, DLManagedTensor* labels_t)
{
  int64_t n            = 0;
  const uint8_t* codes = pq_codes_view(codes_t, q, &n);
  CUVS_EXPECTS(out_t != nullptr, "null argument");
  const DLTensor& o = out_t->dl_tensor;
  CUVS_EXPECTS(is_device_accessible(o), "out must be accessible on device memory");
  CUVS_EXPECTS(dtype_is(o.dtype, kDLFloat, 32), "Unsupported out DLtensor dtype: %d and bits: %d", (int)o.dtype.code, (int)o.dtype.bits);
  CUVS_EXPECTS(o.ndim == 2 && is_c_contiguous(o) && o.shape[0] == n && o.shape[1] == q.dim, "out must be a contiguous [%lld, %lld] matrix",
               (long long)n, (long long)q.dim);
  const uint32_t* labels = nullptr;
  if (q.vq_n > 0) {
    CUVS_EXPECTS(labels_t != nullptr, "vq_labels are required: the quantizer uses VQ");
    labels = pq_labels_view(labels_t, n);
  }
  if (n == 0) return;
  float* out         = static_cast<float*>(dl_data(o));
  const float* vq    = q.vq_n > 0 ? q.vq_book.data() : nullptr;
  const int64_t bstr = q.p.use_subspaces ? q.book_n * q.pq_len : 0;
  const bool v4      = q.pq_len % 4 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0;
  const int64_t items = n * (q.dim / (v4 ? 4 : 1));
  const dim3 grid((unsigned)std::min<int64_t>((items + 255) / 256, (int64_t)res.num_cus * 16));
  profile_begin(res, "pq_decode_kernel");
  if (v4)
    hipLaunchKernelGGL(pq_decode_kernel<4>, grid, dim3(256), 0, res.stream, codes, (int)q.code_bytes(), n, (int)q.dim, (int)q.pq_len,
                       (int)q.p.pq_bits, q.pq_book.data(), bstr, vq, labels, out);
  else
    hipLaunchKernelGGL(pq_decode_kernel<1>, grid, dim3(256), 0, res.stream, codes, (int)q.code_bytes(), n, (int)q.dim, (int)q.pq_len,
                       (int)q.p.pq_bits, q.pq_book.data(), bstr, vq, labels, out);
  profile_end(res, "pq_decode_kernel");
  HIP_TRY(hipGetLastError());
  sync(res);
}

void pq_adopt(cuvsProductQuantizer_t quantizer, std::unique_ptr<product_quantizer> q)
{
  delete reinterpret_cast<product_quantizer*>(quantizer->addr);
  quantizer->addr  = reinterpret_cast<uintptr_t>(q.release());
  quantizer->dtype = kPqF32;
}

const float* pq_device_f32_matrix(DLManagedTensor* t, const char* what, int64_t* rows, int64_t* cols)
{
  const DLTensor& d = t->dl_tensor;
  CUVS_EXPECTS(is_device_accessible(d) && dtype_is(d.dtype, kDLFloat, 32) && d.ndim == 2 && is_c_contiguous(d),
               "%s must be a device float32 row-major matrix", what);
  *rows = d.shape[0];
  *cols = d.shape[1];
  return static_cast<const float*>(dl_data(d));
}

}  // namespace
}  // namespace cuvs_amd

using namespace cuvs_amd;

extern "C" {

cuvsError_t cuvsProductQuantizerParamsCreate(cuvsProductQuantizerParams_t* params)
{
  return (cuvsError_t)translate_exceptions([=] {
    CUVS_EXPECTS(params != nullptr, "params is null");
    *params = new cuvsProductQuantizerParams{8, 0, true, false, 0, 25, CUVS_KMEANS_TYPE_KMEANS_BALANCED, 256, 1024};
  });
}
cuvsError_t cuvsProductQuantizerParamsDestroy(cuvsProductQuantizerParams_t params)
{
  return (cuvsError_t)translate_exceptions([=] { delete params; });
}
cuvsError_t cuvsProductQuantizerCreate(cuvsProductQuantizer_t* quantizer)
{
  return (cuvsError_t)translate_exceptions([=] {
    CUVS_EXPECTS(quantizer != nullptr, "quantizer is null");
    *quantizer = new cuvsProductQuantizer{0, DLDataType{0, 0, 0}};
  });
}
cuvsError_t cuvsProductQuantizerDestroy(cuvsProductQuantizer_t quantizer)
{
  return (cuvsError_t)translate_exceptions([=] {
    if (quantizer == nullptr) return;
    delete reinterpret_cast<product_quantizer*>(quantizer->addr);
    delete quantizer;
  });
}

cuvsError_t cuvsProductQuantizerBuild(cuvsResources_t res_h, cuvsProductQuantizerParams_t params, DLManagedTensor* dataset,
                                      cuvsProductQuantizer_t quantizer)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& res = *as_res(res_h);
    CUVS_EXPECTS(params != nullptr && dataset != nullptr && quantizer != nullptr, "null argument");
    pq_adopt(quantizer, pq_build(res, *params, pq_dataset_view(dataset)));
  });
}

cuvsError_t cuvsProductQuantizerTransform(cuvsResources_t res_h, cuvsProductQuantizer_t quantizer, DLManagedTensor* dataset,
                                          DLManagedTensor* codes_out, DLManagedTensor* vq_labels)
{
  return (cuvsError_t)translate_exceptions(
    [=] { pq_transform(*as_res(res_h), get_pq(quantizer), pq_dataset_view(dataset), codes_out, vq_labels); });
}

cuvsError_t cuvsProductQuantizerInverseTransform(cuvsResources_t res_h, cuvsProductQuantizer_t quantizer, DLManagedTensor* pq_codes,
                                                 DLManagedTensor* out, DLManagedTensor* vq_labels)
{
  return (cuvsError_t)translate_exceptions([=] { pq_inverse(*as_res(res_h), get_pq(quantizer), pq_codes, out, vq_labels); });
}

cuvsError_t cuvsProductQuantizerGetPqBits(cuvsProductQuantizer_t quantizer, uint32_t* pq_bits)
{
  return (cuvsError_t)translate_exceptions([=] { *pq_bits = get_pq(quantizer).p.pq_bits; });
}
cuvsError_t cuvsProductQuantizerGetPqDim(cuvsProductQuantizer_t quantizer, uint32_t* pq_dim)
{
  return (cuvsError_t)translate_exceptions([=] { *pq_dim = get_pq(quantizer).p.pq_dim; });
}
cuvsError_t cuvsProductQuantizerGetPqCodebook(cuvsProductQuantizer_t quantizer, DLManagedTensor* pq_codebook)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& q = get_pq(quantizer);
    CUVS_EXPECTS(pq_codebook != nullptr, "null argument");
    fill_dl_view(pq_codebook, q.pq_book.data(), kPqF32, (q.p.use_subspaces ? (int64_t)q.p.pq_dim : 1) * q.book_n, q.pq_len, 2, 0);
  });
}
cuvsError_t cuvsProductQuantizerGetVqCodebook(cuvsProductQuantizer_t quantizer, DLManagedTensor* vq_codebook)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& q = get_pq(quantizer);
    CUVS_EXPECTS(vq_codebook != nullptr, "null argument");
    fill_dl_view(vq_codebook, q.vq_book.data(), kPqF32, q.vq_n, q.vq_n > 0 ? q.dim : 0, 2, 0);
  });
}
cuvsError_t cuvsProductQuantizerGetEncodedDim(cuvsProductQuantizer_t quantizer, uint32_t* encoded_dim)
{
  return (cuvsError_t)translate_exceptions([=] { *encoded_dim = (uint32_t)get_pq(quantizer).code_bytes(); });
}
cuvsError_t cuvsProductQuantizerGetUseVq(cuvsProductQuantizer_t quantizer, bool* use_vq)
{
  return (cuvsError_t)translate_exceptions([=] { *use_vq = get_pq(quantizer).vq_n > 0; });
}

cuvsError_t cuvsAmdProductQuantizerFromCodebooks(cuvsResources_t res_h, cuvsProductQuantizerParams_t params, DLManagedTensor* pq_codebook,
                                                 DLManagedTensor* vq_codebook, cuvsProductQuantizer_t quantizer)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& res = *as_res(res_h);
    CUVS_EXPECTS(params != nullptr && pq_codebook != nullptr && quantizer != nullptr, "null argument");
    pq_check_params(*params);
    CUVS_EXPECTS(params->pq_dim > 0, "pq_dim must be set");
    auto q    = std::make_unique<product_quantizer>();
    q->p      = *params;
    q->book_n = int64_t(1) << params->pq_bits;
    int64_t rows = 0, cols = 0;
    const float* book   = pq_device_f32_matrix(pq_codebook, "pq_codebook", &rows, &cols);
    const int64_t want  = (params->use_subspaces ? (int64_t)params->pq_dim : 1) * q->book_n;
    CUVS_EXPECTS(rows == want && cols > 0, "pq_codebook must have %lld rows but has %lld", (long long)want, (long long)rows);
    q->pq_len  = cols;
    q->dim     = cols * params->pq_dim;
    q->pq_book = dev_buf<float>::persistent((size_t)(rows * cols));
    copy_async(res, q->pq_book.data(), book, q->pq_book.bytes());
    q->p.use_vq = vq_codebook != nullptr;
    if (vq_codebook != nullptr) {
      const float* vq = pq_device_f32_matrix(vq_codebook, "vq_codebook", &rows, &cols);
      CUVS_EXPECTS(rows > 0 && cols == q->dim, "vq_codebook must be [vq_n_centers, %lld]", (long long)q->dim);
      q->vq_n           = rows;
      q->p.vq_n_centers = (uint32_t)rows;
      q->vq_book        = dev_buf<float>::persistent((size_t)(rows * cols));
      copy_async(res, q->vq_book.data(), vq, q->vq_book.bytes());
    }
    sync(res);
    pq_adopt(quantizer, std::move(q));
  });
}

void cuvsAmdPqEncodeCounters(unsigned long long out[3])
{
  out[2] = g_encode_launches[2].load();
  out[0] = g_encode_launches[0].load();
  out[1] = g_encode_launches[1].load();
}

}  // extern "C"
