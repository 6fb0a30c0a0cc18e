// Binary quantizer (drop-in for c/src/preprocessing/quantize/binary.cpp; semantics of
// cpp/src/preprocessing/quantize/detail/binary.cuh): fp16 / fp32 / fp64 rows -> uint8 codes, bit j of byte b set when
// x[8b + j] > threshold[8b + j] (threshold 0 for ZERO; NaN gives 0). Output bytes past ceil(dim / 8) are written as 0
// (binary.cuh:447-450). Thresholds are kept in the input dtype.
//
// transform is the hot path: one streaming pass, a wave per 64 consecutive inputs of a row. On wave64 the ballot of the
// 64 comparisons is already the 8 output bytes in little bit order, so one 8-byte store covers 64 inputs.
// Training: MEAN is a two-stage column reduction on the device over ~256 MB row chunks (fp64 accumulators for fp32 / fp64
// rows, fp32 for fp16);
// SAMPLING_MEDIAN gathers the reference's strided host sample (binary.cuh:292-324) - on the device for device rows - and
// selects each column's median over it on the host, so host and device rows give the same thresholds.
#include "common.hpp"
#include "device_utils.hpp"

#include <cuvs/preprocessing/quantize/binary.h>

#include <algorithm>
#include <cmath>
#include <vector>

namespace cuvs_amd {
namespace {

enum class bq_t : int { f32 = 0, f16 = 1, f64 = 2 };

bq_t bq_of(const DLDataType& d)
{
  if (dtype_is(d, kDLFloat, 32)) return bq_t::f32;
  if (dtype_is(d, kDLFloat, 16)) return bq_t::f16;
  if (dtype_is(d, kDLFloat, 64)) return bq_t::f64;
  CUVS_FAIL("Unsupported dataset DLtensor dtype: %d and bits: %d", (int)d.code, (int)d.bits);
}

struct binary_quantizer {
  bq_t dtype    = bq_t::f32;
  int64_t dim   = 0;         // thresholds held (0: ZERO)
  dev_buf<char> threshold;   // [dim] of dtype
};

// comparison / accumulation types: fp16 compares in fp32 (binary.cuh compute_t) and sums in fp32; fp32 sums in fp64
template <typename T> struct bq_traits { using cmp = float; using acc = double; };
template <> struct bq_traits<__half> { using cmp = float; using acc = float; };
template <> struct bq_traits<double> { using cmp = double; using acc = double; };

__host__ __device__ inline float to_cmp(__half v) { return __half2float(v); }
__host__ __device__ inline float to_cmp(float v) { return v; }
__host__ __device__ inline double to_cmp(double v) { return v; }
template <typename T> __host__ __device__ inline T from_acc(double v) { return (T)v; }
template <> __host__ __device__ inline __half from_acc<__half>(double v) { return __float2half((float)v); }

// row-major view of a DLPack matrix: unit column stride, row stride >= dim
struct rows_view {
  const void* data;
  int64_t n, dim, ld;
  bool device;
};
rows_view view_rows(const DLTensor& t, const char* what)
{
  CUVS_EXPECTS(t.ndim == 2, "%s must be a 2-D matrix", what);
  CUVS_EXPECTS(t.shape[1] > 0, "%s must have at least one column", what);
  const int64_t ld = t.strides ? t.strides[0] : t.shape[1];
  CUVS_EXPECTS(t.strides == nullptr || t.shape[1] <= 1 || t.strides[1] == 1, "%s must be row-major", what);
  CUVS_EXPECTS(t.shape[0] <= 1 || ld >= t.shape[1], "%s must be row-major", what);
  CUVS_EXPECTS(is_device_accessible(t) || is_host_accessible(t), "%s must be accessible on host or device memory", what);
  return rows_view{dl_data(t), t.shape[0], t.shape[1], std::max<int64_t>(ld, 1), is_device_accessible(t)};
}

// ---------------------------------------------------------------- transform
constexpr int kBqUnroll = 16;  // consecutive 64-input pieces per wave and step

// pieces: (row, s) for s < ceil(out_dim / 8); piece s covers inputs [64 s, 64 s + 64) and output bytes [8 s, 8 s + 8). A wave
// takes kBqUnroll consecutive pieces per step (one division per step, the pieces after it by increment). The loads of all
// pieces of a step are issued first, without a branch - a piece outside the matrix reads element (0, 0) - and compared after,
// so each lane has kBqUnroll row loads (and as many threshold loads, THR) in flight instead of one load and its wait per piece.
template <typename T, bool THR>
__global__ __launch_bounds__(256) void bq_transform_kernel(const T* __restrict__ x, int64_t ld_x, const T* __restrict__ thr,
                                                           int64_t n, int64_t dim, uint8_t* __restrict__ out, int64_t ld_out,
                                                           int64_t out_dim, int vec_store)
{
  using C = typename bq_traits<T>::cmp;
  const int lane       = threadIdx.x & 63;
  const int64_t segs   = (out_dim + 7) / 8;
  const int64_t total  = n * segs;
  const int64_t wave   = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t waves  = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t w0 = wave * kBqUnroll; w0 < total; w0 += waves * kBqUnroll) {  // wave-uniform
    int64_t r = w0 / segs, s = w0 - r * segs;
    int64_t rr[kBqUnroll], ss[kBqUnroll];
    T xv[kBqUnroll], tv[kBqUnroll];
#pragma unroll
    for (int u = 0; u < kBqUnroll; ++u) {
      rr[u] = r; ss[u] = s;
      if (++s == segs) { s = 0; ++r; }
      const bool ok   = w0 + u < total && ss[u] * 64 + lane < dim;
      const int64_t c = ok ? ss[u] * 64 + lane : 0;
      xv[u]           = x[(ok ? rr[u] : 0) * ld_x + c];
      if constexpr (THR) tv[u] = thr[c];
    }
#pragma unroll
    for (int u = 0; u < kBqUnroll; ++u) {
      const bool ok = w0 + u < total && ss[u] * 64 + lane < dim;
      const C v     = to_cmp(xv[u]);
      bool bit;
      if constexpr (THR) bit = ok && v > (C)to_cmp(tv[u]);  // false for NaN
      else               bit = ok && v > (C)0;
      const unsigned long long m = __ballot(bit);
      if (w0 + u >= total) break;  // wave-uniform
      uint8_t* o       = out + rr[u] * ld_out + ss[u] * 8;
      const int64_t nb = min((int64_t)8, out_dim - ss[u] * 8);
      if (vec_store && nb == 8) {
        if (lane == 0) *reinterpret_cast<unsigned long long*>(o) = m;
      } else if (lane < nb) {
        o[lane] = (uint8_t)(m >> (8 * lane));
      }
    }
  }
}

template <typename T>
void bq_transform_device(resources& res, const T* x, int64_t ld_x, const T* thr, int64_t n, int64_t dim, uint8_t* out,
                         int64_t ld_out, int64_t out_dim)
{
  if (n == 0) return;  // (dim >= 1: transform_with; the kernel reads element (0, 0) for pieces outside the matrix)
  const int64_t total  = n * ((out_dim + 7) / 8);
  const int64_t blocks = std::min<int64_t>((total + 4 * kBqUnroll - 1) / (4 * kBqUnroll), (int64_t)res.num_cus * 8);
  const int vec        = (reinterpret_cast<uintptr_t>(out) % 8 == 0 && ld_out % 8 == 0) ? 1 : 0;
  const dim3 grid((unsigned)std::max<int64_t>(blocks, 1));
  profile_begin(res, "bq_transform_kernel");
  if (thr != nullptr)
    hipLaunchKernelGGL((bq_transform_kernel<T, true>), grid, dim3(256), 0, res.stream, x, ld_x, thr, n, dim, out, ld_out, out_dim, vec);
  else
    hipLaunchKernelGGL((bq_transform_kernel<T, false>), grid, dim3(256), 0, res.stream, x, ld_x, thr, n, dim, out, ld_out, out_dim, vec);
  profile_end(res, "bq_transform_kernel");
  HIP_TRY(hipGetLastError());
}

// rows per chunk when host rows are staged through the device (and the row chunks of the MEAN reduction): about 256 MB
inline int64_t bq_chunk_rows(int64_t n, int64_t row_bytes)
{
  return std::max<int64_t>(1, std::min<int64_t>(n, (int64_t(256) << 20) / std::max<int64_t>(row_bytes, 1)));
}

template <typename T>
void bq_transform(resources& res, const binary_quantizer& q, const rows_view& ds, uint8_t* out, int64_t ld_out, int64_t out_dim)
{
  const T* thr = q.dim > 0 ? reinterpret_cast<const T*>(q.threshold.data()) : nullptr;
  if (ds.device) {
    bq_transform_device<T>(res, static_cast<const T*>(ds.data), ds.ld, thr, ds.n, ds.dim, out, ld_out, out_dim);
    sync(res);
    return;
  }
  // host rows: staged through the device in chunks of rows, the codes copied back into the host output
  const int64_t chunk = bq_chunk_rows(ds.n, ds.dim * (int64_t)sizeof(T) + out_dim);
  dev_buf<T> xb(res, (size_t)chunk * ds.dim);
  dev_buf<uint8_t> ob(res, (size_t)chunk * out_dim);
  for (int64_t r0 = 0; r0 < ds.n; r0 += chunk) {
    const int64_t cnt = std::min(chunk, ds.n - r0);
    HIP_TRY(hipMemcpy2DAsync(xb.data(), ds.dim * sizeof(T), static_cast<const T*>(ds.data) + r0 * ds.ld, ds.ld * sizeof(T),
                             ds.dim * sizeof(T), cnt, hipMemcpyHostToDevice, res.stream));
    bq_transform_device<T>(res, xb.data(), ds.dim, thr, cnt, ds.dim, ob.data(), out_dim, out_dim);
    HIP_TRY(hipMemcpy2DAsync(out + r0 * ld_out, ld_out, ob.data(), out_dim, out_dim, cnt, hipMemcpyDeviceToHost, res.stream));
    sync(res);
  }
}

// ---------------------------------------------------------------- MEAN
// stage 1: column sums of a slab of rows (one thread per column, consecutive threads read consecutive columns)
template <typename T>
__global__ void bq_colsum_kernel(const T* __restrict__ x, int64_t ld_x, int64_t n, int64_t dim, int64_t rows_per,
                                 typename bq_traits<T>::acc* __restrict__ partial)
{
  using A         = typename bq_traits<T>::acc;
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= dim) return;
  const int64_t r0 = (int64_t)blockIdx.y * rows_per, r1 = min(n, r0 + rows_per);
  A s = 0;
  for (int64_t r = r0; r < r1; ++r) s += (A)to_cmp(x[r * ld_x + c]);
  partial[(int64_t)blockIdx.y * dim + c] = s;
}

// stage 2: the slab sums of one row chunk added to the running column sums in slab order; the last chunk divides by n and
// rounds to T
template <typename T>
__global__ void bq_mean_kernel(const typename bq_traits<T>::acc* __restrict__ partial, int slabs, int64_t dim, int64_t n,
                               typename bq_traits<T>::acc* __restrict__ sums, int last, T* __restrict__ thr)
{
  using A         = typename bq_traits<T>::acc;
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= dim) return;
  A s = sums[c];
  for (int i = 0; i < slabs; ++i) s += partial[(int64_t)i * dim + c];
  sums[c] = s;
  if (last) thr[c] = from_acc<T>((double)(s / (A)n));
}

// column means over row chunks of ~256 MB: host rows are staged chunk by chunk (the memory bound of the host transform),
// device rows are read in place in the same chunks, so host and device rows give the same sums in the same order
template <typename T>
void bq_train_mean(resources& res, const rows_view& ds, T* thr)
{
  using A             = typename bq_traits<T>::acc;
  const int64_t n = ds.n, dim = ds.dim;
  const int64_t chunk = bq_chunk_rows(n, dim * (int64_t)sizeof(T));
  dev_buf<A> sums(res, (size_t)dim), partial(res, (size_t)std::min<int64_t>(chunk, 1024) * dim);
  dev_buf<T> staged;
  if (!ds.device) staged = dev_buf<T>(res, (size_t)(chunk * dim));
  HIP_TRY(hipMemsetAsync(sums.data(), 0, sums.bytes(), res.stream));
  for (int64_t r0 = 0; r0 < n; r0 += chunk) {
    const int64_t cnt = std::min(chunk, n - r0);
    const T* x        = static_cast<const T*>(ds.data) + r0 * ds.ld;
    int64_t ld        = ds.ld;
    if (!ds.device) {
      HIP_TRY(hipMemcpy2DAsync(staged.data(), dim * sizeof(T), x, ds.ld * sizeof(T), dim * sizeof(T), cnt, hipMemcpyHostToDevice,
                               res.stream));
      x  = staged.data();
      ld = dim;
    }
    const int slabs   = (int)std::min<int64_t>(cnt, 1024);
    const int64_t per = (cnt + slabs - 1) / slabs;
    const int used    = (int)((cnt + per - 1) / per);
    hipLaunchKernelGGL(bq_colsum_kernel<T>, dim3((unsigned)((dim + 255) / 256), (unsigned)used), dim3(256), 0, res.stream, x, ld,
                       cnt, dim, per, partial.data());
    hipLaunchKernelGGL(bq_mean_kernel<T>, dim3(grid_blocks(dim, 256)), dim3(256), 0, res.stream, partial.data(), used, dim, n,
                       sums.data(), r0 + cnt >= n ? 1 : 0, thr);
    HIP_TRY(hipGetLastError());
    if (!ds.device) sync(res);  // (the staging buffer is reused; the host rows may be pageable)
  }
  sync(res);
}

// ---------------------------------------------------------------- SAMPLING_MEDIAN
// binary.cuh:292-324: ns = max(ceil(floor(n * ratio) / 2) * 2, 2) - 1 samples (n * ratio in fp32, as there); row
// (i * stride) % n is sample i, stride the first of four primes that does not divide n
struct median_sample {
  int64_t ns, stride;
};
median_sample median_sample_of(int64_t n, float ratio)
{
  const int64_t scaled = (int64_t)((float)n * ratio);
  const int64_t ns     = std::max<int64_t>((scaled + 1) / 2 * 2, 2) - 1;
  const int64_t primes[4] = {611323, 611333, 611389, 611393};
  int i = 0;
  while (i < 4 && n % primes[i] == 0) ++i;
  CUVS_EXPECTS(i < 4, "binary quantizer: no sampling stride for %lld rows", (long long)n);
  return median_sample{ns, primes[i]};
}

template <typename T>
__global__ void bq_gather_sample_kernel(const T* __restrict__ x, int64_t ld_x, int64_t n, int64_t dim, int64_t ns, int64_t stride,
                                        typename bq_traits<T>::cmp* __restrict__ out)
{
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= ns * dim) return;
  const int64_t i = t / dim, c = t - i * dim;
  out[t]          = to_cmp(x[((i * stride) % n) * ld_x + c]);
}

template <typename T>
void bq_train_median(resources& res, const rows_view& ds, float ratio, T* thr)
{
  using C                = typename bq_traits<T>::cmp;
  const median_sample sm = median_sample_of(ds.n, ratio);
  const int64_t ns = sm.ns, dim = ds.dim;
  std::vector<C> sample((size_t)(ns * dim));
  if (ds.device) {
    dev_buf<C> d(res, (size_t)(ns * dim));
    hipLaunchKernelGGL(bq_gather_sample_kernel<T>, dim3(grid_blocks(ns * dim, 256)), dim3(256), 0, res.stream,
                       static_cast<const T*>(ds.data), ds.ld, ds.n, dim, ns, sm.stride, d.data());
    HIP_TRY(hipGetLastError());
    copy_async(res, sample.data(), d.data(), sample.size() * sizeof(C));
    sync(res);
  } else {
    const T* x = static_cast<const T*>(ds.data);
    for (int64_t i = 0; i < ns; ++i)
      for (int64_t c = 0; c < dim; ++c) sample[(size_t)(i * dim + c)] = to_cmp(x[((i * sm.stride) % ds.n) * ds.ld + c]);
  }
  // the element (ns - 1) / 2 of every sorted column (exact: the threshold is a value of the data)
  std::vector<T> h((size_t)dim);
  std::vector<C> col((size_t)ns);
  for (int64_t c = 0; c < dim; ++c) {
    for (int64_t i = 0; i < ns; ++i) col[(size_t)i] = sample[(size_t)(i * dim + c)];
    std::nth_element(col.begin(), col.begin() + (ns - 1) / 2, col.end());
    h[(size_t)c] = from_acc<T>((double)col[(size_t)((ns - 1) / 2)]);
  }
  copy_async(res, thr, h.data(), (size_t)dim * sizeof(T));
  sync(res);
}

template <typename T>
void bq_train(resources& res, const cuvsBinaryQuantizerParams& p, const rows_view& ds, binary_quantizer& q)
{
  if (p.threshold == ZERO) return;  // no thresholds (binary.cuh: an empty threshold vector)
  CUVS_EXPECTS(p.threshold == MEAN || p.threshold == SAMPLING_MEDIAN, "Unsupported threshold");
  CUVS_EXPECTS(ds.n > 0, "binary quantizer: the training dataset is empty");
  if (p.threshold == SAMPLING_MEDIAN)
    CUVS_EXPECTS(p.sampling_ratio > 0.f && p.sampling_ratio <= 1.f, "The sampling ratio must be within the range (0, 1].");
  q.dim       = ds.dim;
  q.threshold = dev_buf<char>::persistent((size_t)ds.dim * sizeof(T));
  T* thr      = reinterpret_cast<T*>(q.threshold.data());
  if (p.threshold == SAMPLING_MEDIAN) {
    bq_train_median<T>(res, ds, p.sampling_ratio, thr);
    return;
  }
  bq_train_mean<T>(res, ds, thr);
}

binary_quantizer& get_bq(cuvsBinaryQuantizer_t q)
{
  CUVS_EXPECTS(q != nullptr && q->addr != 0, "binary quantizer is not trained");
  return *reinterpret_cast<binary_quantizer*>(q->addr);
}

void transform_with(resources& res, const binary_quantizer& q, DLManagedTensor* dataset, DLManagedTensor* out)
{
  CUVS_EXPECTS(dataset != nullptr && out != nullptr, "null argument");
  const rows_view ds = view_rows(dataset->dl_tensor, "dataset");
  CUVS_EXPECTS(bq_of(dataset->dl_tensor.dtype) == q.dtype, "binary quantizer: the dataset dtype differs from the quantizer's");
  CUVS_EXPECTS(q.dim == 0 || ds.dim == q.dim, "binary quantizer: dataset dim %lld differs from the threshold length %lld",
               (long long)ds.dim, (long long)q.dim);
  const DLTensor& o = out->dl_tensor;
  CUVS_EXPECTS(dtype_is(o.dtype, kDLUInt, 8), "the quantized dataset must be uint8");
  const rows_view ov = view_rows(o, "the quantized dataset");
  CUVS_EXPECTS(ov.device == ds.device, "the quantized dataset must be in the same kind of memory as the dataset");
  const int64_t min_dim = (ds.dim + 7) / 8;
  CUVS_EXPECTS(ov.dim >= min_dim, "The quantized dataset dimension must be larger or equal to %lld but is %lld passed",
               (long long)min_dim, (long long)ov.dim);
  CUVS_EXPECTS(ov.n >= ds.n, "The quantized dataset size must be larger or equal to the input dataset size (%lld) but is %lld passed",
               (long long)ds.n, (long long)ov.n);
  uint8_t* op = static_cast<uint8_t*>(const_cast<void*>(ov.data));
  switch (q.dtype) {
    case bq_t::f32: bq_transform<float>(res, q, ds, op, ov.ld, ov.dim); break;
    case bq_t::f16: bq_transform<__half>(res, q, ds, op, ov.ld, ov.dim); break;
    case bq_t::f64: bq_transform<double>(res, q, ds, op, ov.ld, ov.dim); break;
  }
}

}  // namespace
}  // namespace cuvs_amd

using namespace cuvs_amd;

extern "C" {

cuvsError_t cuvsBinaryQuantizerParamsCreate(cuvsBinaryQuantizerParams_t* params)
{
  return (cuvsError_t)translate_exceptions([=] {
    CUVS_EXPECTS(params != nullptr, "params is null");
    *params = new cuvsBinaryQuantizerParams{MEAN, 0.1f};  // binary.cpp:95-101
  });
}
cuvsError_t cuvsBinaryQuantizerParamsDestroy(cuvsBinaryQuantizerParams_t params)
{
  return (cuvsError_t)translate_exceptions([=] { delete params; });
}
cuvsError_t cuvsBinaryQuantizerCreate(cuvsBinaryQuantizer_t* quantizer)
{
  return (cuvsError_t)translate_exceptions([=] {
    CUVS_EXPECTS(quantizer != nullptr, "quantizer is null");
    *quantizer = new cuvsBinaryQuantizer{0, DLDataType{0, 0, 0}};
  });
}
cuvsError_t cuvsBinaryQuantizerDestroy(cuvsBinaryQuantizer_t quantizer)
{
  return (cuvsError_t)translate_exceptions([=] {
    if (quantizer == nullptr) return;
    delete reinterpret_cast<binary_quantizer*>(quantizer->addr);
    delete quantizer;
  });
}

cuvsError_t cuvsBinaryQuantizerTrain(cuvsResources_t res_h, cuvsBinaryQuantizerParams_t params, DLManagedTensor* dataset,
                                     cuvsBinaryQuantizer_t quantizer)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& res = *as_res(res_h);
    CUVS_EXPECTS(params != nullptr && dataset != nullptr && quantizer != nullptr, "null argument");
    const bq_t t       = bq_of(dataset->dl_tensor.dtype);
    const rows_view ds = view_rows(dataset->dl_tensor, "dataset");
    auto q             = std::make_unique<binary_quantizer>();
    q->dtype           = t;
    switch (t) {
      case bq_t::f32: bq_train<float>(res, *params, ds, *q); break;
      case bq_t::f16: bq_train<__half>(res, *params, ds, *q); break;
      case bq_t::f64: bq_train<double>(res, *params, ds, *q); break;
    }
    delete reinterpret_cast<binary_quantizer*>(quantizer->addr);
    quantizer->addr  = reinterpret_cast<uintptr_t>(q.release());
    quantizer->dtype = dataset->dl_tensor.dtype;
  });
}

cuvsError_t cuvsBinaryQuantizerTransformWithParams(cuvsResources_t res_h, cuvsBinaryQuantizer_t quantizer, DLManagedTensor* dataset,
                                                   DLManagedTensor* out)
{
  return (cuvsError_t)translate_exceptions([=] { transform_with(*as_res(res_h), get_bq(quantizer), dataset, out); });
}

// binary.cpp:161-179: a ZERO quantizer (which holds no thresholds, so nothing is trained)
cuvsError_t cuvsBinaryQuantizerTransform(cuvsResources_t res_h, DLManagedTensor* dataset, DLManagedTensor* out)
{
  return (cuvsError_t)translate_exceptions([=] {
    CUVS_EXPECTS(dataset != nullptr, "null argument");
    binary_quantizer q;
    q.dtype = bq_of(dataset->dl_tensor.dtype);
    transform_with(*as_res(res_h), q, dataset, out);
  });
}

__attribute__((visibility("default"))) cuvsError_t cuvsAmdBinaryQuantizerGetThreshold(cuvsResources_t res_h,
                                                                                      cuvsBinaryQuantizer_t quantizer,
                                                                                      DLManagedTensor* out)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& res = *as_res(res_h);
    auto& q   = get_bq(quantizer);
    CUVS_EXPECTS(out != nullptr, "null argument");
    const DLTensor& o = out->dl_tensor;
    CUVS_EXPECTS(o.ndim == 1 && o.shape[0] == q.dim && (o.strides == nullptr || q.dim <= 1 || o.strides[0] == 1),
                 "threshold output must be a contiguous vector of length %lld", (long long)q.dim);
    CUVS_EXPECTS(bq_of(o.dtype) == q.dtype, "threshold output dtype differs from the quantizer's");
    copy_async(res, dl_data(o), q.threshold.data(), q.threshold.bytes());
    sync(res);
  });
}

}  // extern "C"
