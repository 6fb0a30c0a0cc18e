// Scalar quantizer (drop-in for c/src/preprocessing/quantize/scalar.cpp; semantics of
// cpp/src/preprocessing/quantize/detail/scalar.cuh): fp16 / fp32 / fp64 rows <-> int8 codes over [min_, max_].
//
//   transform(x) = -128 when !(min < x), else 127 when !(x < max), else lroundf((float)(scale * (double)x + offset))
//   inverse(q)   = (T)(((double)q - offset) / scale)
//   scale = 255 / ((double)max - (double)min) (1 when max <= min), offset = -128 - (double)min * scale
// with min and max rounded to T first (the C struct carries doubles, the reference's quantizer<T> holds T). fp16 compares in
// fp32. The double -> float conversion before the rounding is the reference's and part of the contract. One functor, sq_op,
// is compiled for host and device, so both kinds of memory give the same bytes.
//
// Both directions are one streaming pass: a lane handles 16 bytes of the fp side per piece (4 fp32 / 8 fp16 / 2 fp64),
// kSqUnroll pieces per step with all loads issued before the first conversion, as bq_transform_kernel does.
// Training: the quantile is an order statistic of min(1000000 / dim, n) sampled rows (all of them when they fit: exact);
// the sample is gathered (on the device for device rows) and selected on the host, so host and device rows agree.
#include "common.hpp"
#include "device_utils.hpp"

#include <cuvs/preprocessing/quantize/scalar.h>

#include <algorithm>
#include <cmath>
#include <random>
#include <thread>
#include <unordered_set>
#include <vector>

namespace cuvs_amd {
namespace {

using half_t = _Float16;  // converts from double with one rounding on host and device alike

template <typename T> struct sq_traits { using cmp = T; };
template <> struct sq_traits<half_t> { using cmp = float; };

template <typename T>
struct sq_op {
  using C = typename sq_traits<T>::cmp;
  C min_, max_;
  double scale, offset;
  sq_op(double mn, double mx)
  {
    const T tmin = (T)mn, tmax = (T)mx;
    min_   = (C)tmin;
    max_   = (C)tmax;
    scale  = (double)tmax > (double)tmin ? 255.0 / ((double)tmax - (double)tmin) : 1.0;
    offset = -128.0 - (double)tmin * scale;
  }
  __host__ __device__ inline int8_t quantize(T x) const
  {
    const C v = (C)x;
    if (!(min_ < v)) return (int8_t)-128;  // NaN lands here
    if (!(v < max_)) return (int8_t)127;
    return (int8_t)lroundf((float)(scale * (double)v + offset));
  }
  __host__ __device__ inline T dequantize(int8_t q) const { return (T)(((double)q - offset) / scale); }
};

constexpr int kSqUnroll = 8;  // 16-byte pieces in flight per lane

template <typename T> struct sq_vec { static constexpr int n = 16 / (int)sizeof(T); };
template <int BYTES> struct sq_codes;
template <> struct sq_codes<2> { using type = uint16_t; };
template <> struct sq_codes<4> { using type = uint32_t; };
template <> struct sq_codes<8> { using type = unsigned long long; };

// pieces [0, n_vec) are 16 bytes of x each; the elements past them (and everything, when a pointer is not aligned: n_vec 0) go
// one by one
template <typename T>
__global__ __launch_bounds__(256) void sq_transform_kernel(const T* __restrict__ x, int64_t total, int64_t n_vec,
                                                           int8_t* __restrict__ out, sq_op<T> op)
{
  constexpr int V = sq_vec<T>::n;
  using code_t    = typename sq_codes<V>::type;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nthr = (int64_t)gridDim.x * blockDim.x;
  const uint4* xv   = reinterpret_cast<const uint4*>(x);
  code_t* ov        = reinterpret_cast<code_t*>(out);
  for (int64_t p0 = tid; p0 < n_vec; p0 += nthr * kSqUnroll) {
    uint4 v[kSqUnroll];
#pragma unroll
    for (int u = 0; u < kSqUnroll; ++u) {
      const int64_t p = p0 + (int64_t)u * nthr;
      v[u]            = xv[p < n_vec ? p : 0];
    }
#pragma unroll
    for (int u = 0; u < kSqUnroll; ++u) {
      const int64_t p = p0 + (int64_t)u * nthr;
      if (p >= n_vec) break;
      T e[V];
      __builtin_memcpy(e, &v[u], 16);
      code_t c = 0;
#pragma unroll
      for (int i = 0; i < V; ++i) c |= (code_t)(uint8_t)op.quantize(e[i]) << (8 * i);
      ov[p] = c;
    }
  }
  for (int64_t i = n_vec * V + tid; i < total; i += nthr) out[i] = op.quantize(x[i]);
}

template <typename T>
__global__ __launch_bounds__(256) void sq_inverse_kernel(const int8_t* __restrict__ q, int64_t total, int64_t n_vec,
                                                         T* __restrict__ out, sq_op<T> op)
{
  constexpr int V = sq_vec<T>::n;
  using code_t    = typename sq_codes<V>::type;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nthr = (int64_t)gridDim.x * blockDim.x;
  const code_t* qv  = reinterpret_cast<const code_t*>(q);
  uint4* ov         = reinterpret_cast<uint4*>(out);
  for (int64_t p0 = tid; p0 < n_vec; p0 += nthr * kSqUnroll) {
    code_t c[kSqUnroll];
#pragma unroll
    for (int u = 0; u < kSqUnroll; ++u) {
      const int64_t p = p0 + (int64_t)u * nthr;
      c[u]            = qv[p < n_vec ? p : 0];
    }
#pragma unroll
    for (int u = 0; u < kSqUnroll; ++u) {
      const int64_t p = p0 + (int64_t)u * nthr;
      if (p >= n_vec) break;
      T e[V];
#pragma unroll
      for (int i = 0; i < V; ++i) e[i] = op.dequantize((int8_t)(uint8_t)(c[u] >> (8 * i)));
      uint4 v;
      __builtin_memcpy(&v, e, 16);
      ov[p] = v;
    }
  }
  for (int64_t i = n_vec * V + tid; i < total; i += nthr) out[i] = op.dequantize(q[i]);
}

inline unsigned sq_grid(resources& res, int64_t n_vec, int64_t total)
{
  const int64_t want = std::max<int64_t>((std::max(n_vec, total / 16) + 256 * kSqUnroll - 1) / (256 * kSqUnroll), 1);
  return (unsigned)std::min<int64_t>(want, (int64_t)res.num_cus * 8);
}

// host side: the same functor over slices of the elements
template <typename Fn>
void sq_parallel_for(int64_t total, Fn&& fn)
{
  const int64_t nt = std::max<int64_t>(1, std::min<int64_t>({(int64_t)std::thread::hardware_concurrency(), 16, total / (1 << 16)}));
  if (nt == 1) { fn(0, total); return; }
  std::vector<std::thread> th;
  const int64_t per = (total + nt - 1) / nt;
  for (int64_t t = 0; t < nt; ++t) th.emplace_back([=, &fn] { fn(t * per, std::min(total, (t + 1) * per)); });
  for (auto& t : th) t.join();
}

resources& sq_need(resources* r)
{
  CUVS_EXPECTS(r != nullptr, "null cuvsResources_t");
  return *r;
}

struct sq_matrix {
  void* data;
  int64_t n, dim;
  bool device;
};
sq_matrix sq_view(DLManagedTensor* t, const char* what)
{
  CUVS_EXPECTS(t != nullptr, "null argument");
  const DLTensor& d = t->dl_tensor;
  CUVS_EXPECTS(d.ndim == 2, "%s must be a 2-D matrix", what);
  CUVS_EXPECTS(is_c_contiguous(d), "%s must be row-major and contiguous", what);
  CUVS_EXPECTS(is_device_accessible(d) || is_host_accessible(d), "%s must be accessible on host or device memory", what);
  return sq_matrix{dl_data(d), d.shape[0], d.shape[1], is_device_accessible(d)};
}

template <typename T>
void sq_transform(resources* rp, const cuvsScalarQuantizer& q, const sq_matrix& ds, const sq_matrix& out)
{
  const sq_op<T> op(q.min_, q.max_);
  const int64_t total = ds.n * ds.dim;
  if (total == 0) return;
  const T* x = static_cast<const T*>(ds.data);
  int8_t* o  = static_cast<int8_t*>(out.data);
  if (!ds.device) {
    sq_parallel_for(total, [=](int64_t b, int64_t e) { for (int64_t i = b; i < e; ++i) o[i] = op.quantize(x[i]); });
    return;
  }
  resources& res = sq_need(rp);
  constexpr int V     = sq_vec<T>::n;
  const bool aligned  = reinterpret_cast<uintptr_t>(x) % 16 == 0 && reinterpret_cast<uintptr_t>(o) % V == 0;
  const int64_t n_vec = aligned ? total / V : 0;
  profile_begin(res, "sq_transform_kernel");
  hipLaunchKernelGGL(sq_transform_kernel<T>, dim3(sq_grid(res, n_vec, total)), dim3(256), 0, res.stream, x, total, n_vec, o, op);
  profile_end(res, "sq_transform_kernel");
  HIP_TRY(hipGetLastError());
  sync(res);
}

template <typename T>
void sq_inverse(resources* rp, const cuvsScalarQuantizer& q, const sq_matrix& codes, const sq_matrix& out)
{
  const sq_op<T> op(q.min_, q.max_);
  const int64_t total = codes.n * codes.dim;
  if (total == 0) return;
  const int8_t* c = static_cast<const int8_t*>(codes.data);
  T* o            = static_cast<T*>(out.data);
  if (!codes.device) {
    sq_parallel_for(total, [=](int64_t b, int64_t e) { for (int64_t i = b; i < e; ++i) o[i] = op.dequantize(c[i]); });
    return;
  }
  resources& res = sq_need(rp);
  constexpr int V     = sq_vec<T>::n;
  const bool aligned  = reinterpret_cast<uintptr_t>(o) % 16 == 0 && reinterpret_cast<uintptr_t>(c) % V == 0;
  const int64_t n_vec = aligned ? total / V : 0;
  profile_begin(res, "sq_inverse_kernel");
  hipLaunchKernelGGL(sq_inverse_kernel<T>, dim3(sq_grid(res, n_vec, total)), dim3(256), 0, res.stream, c, total, n_vec, o, op);
  profile_end(res, "sq_inverse_kernel");
  HIP_TRY(hipGetLastError());
  sync(res);
}

// ---------------------------------------------------------------- train
template <typename T>
__global__ void sq_gather_rows_kernel(const T* __restrict__ x, int64_t dim, const int64_t* __restrict__ rows, int64_t ns,
                                      T* __restrict__ out)
{
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= ns * dim) return;
  const int64_t i = t / dim;
  out[t]          = x[rows[i] * dim + (t - i * dim)];
}

// ns distinct rows of n, ascending (Floyd's sampling over this library's own generator; the reference draws with RAFT's
// device generator, whose stream is not reproduced here)
std::vector<int64_t> sq_sample_rows(int64_t n, int64_t ns)
{
  std::mt19937_64 gen(137);  // scalar.cuh:71 uses the same seed for its own generator
  std::unordered_set<int64_t> seen;
  seen.reserve((size_t)ns * 2);
  for (int64_t j = n - ns; j < n; ++j) {
    const int64_t t = (int64_t)(gen() % (uint64_t)(j + 1));
    if (!seen.insert(t).second) seen.insert(j);
  }
  std::vector<int64_t> rows(seen.begin(), seen.end());
  std::sort(rows.begin(), rows.end());
  return rows;
}

template <typename T>
void sq_train(resources* rp, double quantile, const sq_matrix& ds, cuvsScalarQuantizer& q)
{
  using C = typename sq_traits<T>::cmp;
  CUVS_EXPECTS(ds.n > 0 && ds.dim > 0, "scalar quantizer: the training dataset is empty");
  const int64_t ns = std::min<int64_t>(1000000 / ds.dim, ds.n);
  CUVS_EXPECTS(ns > 0, "scalar quantizer: rows of more than 1000000 columns cannot be sampled");
  const int64_t size = ns * ds.dim;
  std::vector<T> sample((size_t)size);
  const T* x = static_cast<const T*>(ds.data);
  if (!ds.device && ns == ds.n) {
    std::copy(x, x + size, sample.begin());
  } else if (ns == ds.n) {
    resources& res = sq_need(rp);
    copy_async(res, sample.data(), x, (size_t)size * sizeof(T));
    sync(res);
  } else {
    const std::vector<int64_t> rows = sq_sample_rows(ds.n, ns);
    if (ds.device) {
      resources& res = sq_need(rp);
      dev_buf<int64_t> d_rows(res, (size_t)ns);
      dev_buf<T> d_sample(res, (size_t)size);
      copy_async(res, d_rows.data(), rows.data(), (size_t)ns * sizeof(int64_t));
      hipLaunchKernelGGL(sq_gather_rows_kernel<T>, dim3(grid_blocks(size, 256)), dim3(256), 0, res.stream, x, ds.dim, d_rows.data(),
                         ns, d_sample.data());
      HIP_TRY(hipGetLastError());
      copy_async(res, sample.data(), d_sample.data(), (size_t)size * sizeof(T));
      sync(res);
    } else {
      for (int64_t i = 0; i < ns; ++i) std::copy(x + rows[(size_t)i] * ds.dim, x + (rows[(size_t)i] + 1) * ds.dim, sample.begin() + i * ds.dim);
    }
  }
  // scalar.cuh:86-88
  const double half_quantile_pos = (0.5 + 0.5 * quantile) * (double)size;
  const int64_t pos_max          = (int64_t)std::ceil(half_quantile_pos) - 1;
  const int64_t pos_min          = size - pos_max - 1;
  CUVS_EXPECTS(pos_max >= 0 && pos_max < size && pos_min >= 0 && pos_min < size, "scalar quantizer: quantile position out of range");
  auto lt = [](const T& a, const T& b) { return (C)a < (C)b; };
  std::nth_element(sample.begin(), sample.begin() + pos_max, sample.end(), lt);
  const T vmax = sample[(size_t)pos_max];
  // pos_min <= pos_max: it lies in the lower part the first selection left
  std::nth_element(sample.begin(), sample.begin() + std::min(pos_min, pos_max), sample.begin() + pos_max + 1, lt);
  const T vmin = sample[(size_t)std::min(pos_min, pos_max)];
  q.min_ = (double)vmin;
  q.max_ = (double)vmax;
}

enum class sq_t : int { f32, f16, f64 };
sq_t sq_of(const DLDataType& d, const char* what)
{
  if (dtype_is(d, kDLFloat, 32)) return sq_t::f32;
  if (dtype_is(d, kDLFloat, 16)) return sq_t::f16;
  if (dtype_is(d, kDLFloat, 64)) return sq_t::f64;
  CUVS_FAIL("Unsupported %s DLtensor dtype: %d and bits: %d", what, (int)d.code, (int)d.bits);
}

}  // namespace
}  // namespace cuvs_amd

using namespace cuvs_amd;

extern "C" {

cuvsError_t cuvsScalarQuantizerParamsCreate(cuvsScalarQuantizerParams_t* params)
{
  return (cuvsError_t)translate_exceptions([=] {
    CUVS_EXPECTS(params != nullptr, "params is null");
    *params = new cuvsScalarQuantizerParams{0.99f};  // scalar.cpp:127
  });
}
cuvsError_t cuvsScalarQuantizerParamsDestroy(cuvsScalarQuantizerParams_t params)
{
  return (cuvsError_t)translate_exceptions([=] { delete params; });
}
cuvsError_t cuvsScalarQuantizerCreate(cuvsScalarQuantizer_t* quantizer)
{
  return (cuvsError_t)translate_exceptions([=] {
    CUVS_EXPECTS(quantizer != nullptr, "quantizer is null");
    *quantizer = new cuvsScalarQuantizer{0.0, 0.0};
  });
}
cuvsError_t cuvsScalarQuantizerDestroy(cuvsScalarQuantizer_t quantizer)
{
  return (cuvsError_t)translate_exceptions([=] { delete quantizer; });
}

cuvsError_t cuvsScalarQuantizerTrain(cuvsResources_t res_h, cuvsScalarQuantizerParams_t params, DLManagedTensor* dataset,
                                     cuvsScalarQuantizer_t quantizer)
{
  return (cuvsError_t)translate_exceptions([=] {
    resources* res = res_h != 0 ? as_res(res_h) : nullptr;  // host rows need no device: the handle may be 0
    CUVS_EXPECTS(params != nullptr && dataset != nullptr && quantizer != nullptr, "null argument");
    CUVS_EXPECTS(params->quantile > 0.0f && params->quantile <= 1.0f,
                 "quantile for scalar quantization needs to be within (0, 1] but is %f", (double)params->quantile);
    const sq_t t       = sq_of(dataset->dl_tensor.dtype, "dataset");
    const sq_matrix ds = sq_view(dataset, "dataset");
    switch (t) {
      case sq_t::f32: sq_train<float>(res, (double)params->quantile, ds, *quantizer); break;
      case sq_t::f16: sq_train<half_t>(res, (double)params->quantile, ds, *quantizer); break;
      case sq_t::f64: sq_train<double>(res, (double)params->quantile, ds, *quantizer); break;
    }
  });
}

cuvsError_t cuvsScalarQuantizerTransform(cuvsResources_t res_h, cuvsScalarQuantizer_t quantizer, DLManagedTensor* dataset,
                                         DLManagedTensor* out)
{
  return (cuvsError_t)translate_exceptions([=] {
    resources* res = res_h != 0 ? as_res(res_h) : nullptr;  // host rows need no device: the handle may be 0
    CUVS_EXPECTS(quantizer != nullptr && dataset != nullptr && out != nullptr, "null argument");
    const sq_t t       = sq_of(dataset->dl_tensor.dtype, "dataset");
    const sq_matrix ds = sq_view(dataset, "dataset"), ov = sq_view(out, "the quantized dataset");
    CUVS_EXPECTS(dtype_is(out->dl_tensor.dtype, kDLInt, 8), "the quantized dataset must be int8");
    CUVS_EXPECTS(ov.device == ds.device, "the quantized dataset must be in the same kind of memory as the dataset");
    CUVS_EXPECTS(ov.n == ds.n && ov.dim == ds.dim, "the quantized dataset must be [%lld, %lld] but is [%lld, %lld]", (long long)ds.n,
                 (long long)ds.dim, (long long)ov.n, (long long)ov.dim);
    switch (t) {
      case sq_t::f32: sq_transform<float>(res, *quantizer, ds, ov); break;
      case sq_t::f16: sq_transform<half_t>(res, *quantizer, ds, ov); break;
      case sq_t::f64: sq_transform<double>(res, *quantizer, ds, ov); break;
    }
  });
}

cuvsError_t cuvsScalarQuantizerInverseTransform(cuvsResources_t res_h, cuvsScalarQuantizer_t quantizer, DLManagedTensor* dataset,
                                                DLManagedTensor* out)
{
  return (cuvsError_t)translate_exceptions([=] {
    resources* res = res_h != 0 ? as_res(res_h) : nullptr;  // host rows need no device: the handle may be 0
    CUVS_EXPECTS(quantizer != nullptr && dataset != nullptr && out != nullptr, "null argument");
    const sq_matrix cv = sq_view(dataset, "the quantized dataset"), ov = sq_view(out, "out");
    CUVS_EXPECTS(dtype_is(dataset->dl_tensor.dtype, kDLInt, 8), "the quantized dataset must be int8");
    const sq_t t = sq_of(out->dl_tensor.dtype, "out");
    CUVS_EXPECTS(ov.device == cv.device, "out must be in the same kind of memory as the quantized dataset");
    CUVS_EXPECTS(ov.n == cv.n && ov.dim == cv.dim, "out must be [%lld, %lld] but is [%lld, %lld]", (long long)cv.n, (long long)cv.dim,
                 (long long)ov.n, (long long)ov.dim);
    switch (t) {
      case sq_t::f32: sq_inverse<float>(res, *quantizer, cv, ov); break;
      case sq_t::f16: sq_inverse<half_t>(res, *quantizer, cv, ov); break;
      case sq_t::f64: sq_inverse<double>(res, *quantizer, cv, ov); break;
    }
  });
}

}  // extern "C"
