// C++ surface over the C ABI: cuvs::neighbors::{brute_force, ivf_flat, ivf_pq, cagra, vamana}::build / search with the
// reference's names (cpp/include/cuvs/neighbors/{brute_force,ivf_flat,ivf_pq,cagra}.hpp). Header-only, C++17, no RAFT:
// `raft::resources` -> cuvs::resources (RAII over cuvsResources_t), `raft::device_matrix_view<T, int64_t>` ->
// cuvs::device_matrix_view<T> (data_handle(), extent(i) - the two members the reference call sites use). Parameter
// structs carry the reference's C++ field names and defaults (ivf_pq.hpp:40-236, ivf_flat.hpp:29-103,
// cagra.hpp:84-360) and are copied field by field into the C structs. Errors become cuvs::error exceptions carrying
// cuvsGetLastErrorText(), like the reference's raft::exception.
#pragma once
#include <cuvs/core/all.h>
#include <cuvs_amd/ball_cover.h>
#include <cuvs_amd/eps_neighbors.h>
#include <cuvs_amd/extensions.h>
#include <cuvs_amd/ivf_rabitq.h>
#include <cuvs_amd/scann.h>
#include <cuvs_amd/sparse.h>

#include <array>
#include <cmath>
#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
#include <type_traits>

namespace cuvs {

struct error : std::runtime_error {
  using std::runtime_error::runtime_error;
};
inline void check(cuvsError_t e, const char* what)
{
  if (e != CUVS_SUCCESS) {
    const char* t = cuvsGetLastErrorText();
    throw error(std::string(what) + ": " + (t ? t : "unknown error"));
  }
}

class resources {
 public:
  resources() { check(cuvsResourcesCreate(&h_), "cuvsResourcesCreate"); }
  ~resources() { cuvsResourcesDestroy(h_); }
  resources(const resources&)            = delete;
  resources& operator=(const resources&) = delete;
  cuvsResources_t get() const { return h_; }
  void sync_stream() const { check(cuvsStreamSync(h_), "cuvsStreamSync"); }

 private:
  cuvsResources_t h_ = 0;
};

// row-major [rows, cols] view of memory the caller owns (device memory unless `on_host`)
template <typename T>
struct device_matrix_view {
  T* ptr         = nullptr;
  int64_t rows   = 0, cols = 0;
  bool on_host   = false;
  T* data_handle() const { return ptr; }
  int64_t extent(int i) const { return i == 0 ? rows : cols; }
};
template <typename T>
device_matrix_view<T> make_device_matrix_view(T* p, int64_t rows, int64_t cols) { return {p, rows, cols, false}; }
template <typename T>
device_matrix_view<T> make_host_matrix_view(T* p, int64_t rows, int64_t cols) { return {p, rows, cols, true}; }

namespace detail {
template <typename T>
DLDataType dl_dtype()
{
  using U = std::remove_cv_t<T>;
  if constexpr (std::is_same_v<U, float>) return {kDLFloat, 32, 1};
  else if constexpr (std::is_same_v<U, int8_t>) return {kDLInt, 8, 1};
  else if constexpr (std::is_same_v<U, uint8_t>) return {kDLUInt, 8, 1};
  else if constexpr (std::is_same_v<U, int64_t>) return {kDLInt, 64, 1};
  else if constexpr (std::is_same_v<U, uint32_t>) return {kDLUInt, 32, 1};
  else if constexpr (std::is_same_v<U, int32_t>) return {kDLInt, 32, 1};
  else if constexpr (std::is_same_v<U, bool>) return {kDLBool, 8, 1};
  else if constexpr (std::is_same_v<U, int16_t>) return {kDLInt, 16, 1};
  else if constexpr (sizeof(U) == 2) return {kDLFloat, 16, 1};  // __half / _Float16
  else static_assert(sizeof(U) == 0, "unsupported element type");
}
// a DLManagedTensor describing a view; lives as long as the call it is passed to
template <typename T>
struct tensor {
  DLManagedTensor m{};
  int64_t shape[2];
  explicit tensor(const device_matrix_view<T>& v)
  {
    shape[0] = v.rows; shape[1] = v.cols;
    m.dl_tensor.data        = const_cast<std::remove_cv_t<T>*>(v.ptr);
    m.dl_tensor.device      = {v.on_host ? kDLCPU : kDLCUDA, 0};
    m.dl_tensor.ndim        = 2;
    m.dl_tensor.dtype       = dl_dtype<T>();
    m.dl_tensor.shape       = shape;
    m.dl_tensor.strides     = nullptr;
    m.dl_tensor.byte_offset = 0;
  }
  DLManagedTensor* get() { return &m; }
};
// a DLManagedTensor describing a device vector of `len` elements
template <typename T>
struct vector_tensor {
  DLManagedTensor m{};
  int64_t shape[1];
  vector_tensor(T* p, int64_t len)
  {
    shape[0]                = len;
    m.dl_tensor.data        = const_cast<std::remove_cv_t<T>*>(p);
    m.dl_tensor.device      = {kDLCUDA, 0};
    m.dl_tensor.ndim        = 1;
    m.dl_tensor.dtype       = dl_dtype<T>();
    m.dl_tensor.shape       = shape;
    m.dl_tensor.strides     = nullptr;
    m.dl_tensor.byte_offset = 0;
  }
  DLManagedTensor* get() { return m.dl_tensor.data ? &m : nullptr; }  // a null pointer leaves the argument out
};
template <typename P, cuvsError_t (*Create)(P*), cuvsError_t (*Destroy)(P)>
struct c_params {
  P p = nullptr;
  c_params() { check(Create(&p), "params create"); }
  ~c_params() { Destroy(p); }
  c_params(const c_params&) = delete;
};
}  // namespace detail

// a canonical CSR matrix the caller owns, on the device (include/cuvs_amd/sparse.h): indptr [rows + 1], indices and data [nnz]
struct csr_view {
  const int32_t* indptr  = nullptr;
  const int32_t* indices = nullptr;
  const float* data      = nullptr;
  int64_t rows = 0, cols = 0, nnz = 0;
};

namespace detail {
struct csr_tensors {
  vector_tensor<const int32_t> indptr, indices;
  vector_tensor<const float> data;
  explicit csr_tensors(const csr_view& v) : indptr(v.indptr, v.rows + 1), indices(v.indices, v.nnz), data(v.data, v.nnz) {}
};
}  // namespace detail

namespace distance {
// distance.hpp:389-466: pairwise_distance(res, csr x, csr y, dense out, metric, metric_arg); out is [x.rows, y.rows]
inline void pairwise_distance(const resources& res, const csr_view& x, const csr_view& y, device_matrix_view<float> out,
                              cuvsDistanceType metric, float metric_arg = 2.0f)
{
  detail::csr_tensors tx(x), ty(y);
  detail::tensor<float> o(out);
  check(cuvsAmdSparsePairwiseDistance(res.get(), &tx.indptr.m, &tx.indices.m, &tx.data.m, x.rows, &ty.indptr.m, &ty.indices.m, &ty.data.m,
                                      y.rows, x.cols, o.get(), metric, metric_arg),
        "cuvsAmdSparsePairwiseDistance");
}
}  // namespace distance

namespace neighbors {

namespace filtering {
// cuvs::neighbors::filtering::bitset_filter (cpp/include/cuvs/neighbors/common.hpp): bit i of the device words = 1 keeps
// source row i
struct bitset_filter {
  const uint32_t* words = nullptr;  // device memory
  int64_t n_bits        = 0;
};
}  // namespace filtering

namespace brute_force {
template <typename T = float>
class index {
 public:
  index() { check(cuvsBruteForceIndexCreate(&h_), "cuvsBruteForceIndexCreate"); }
  ~index() { if (h_) cuvsBruteForceIndexDestroy(h_); }
  index(index&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
  index(const index&) = delete;
  cuvsBruteForceIndex_t get() const { return h_; }

 private:
  cuvsBruteForceIndex_t h_ = nullptr;
};
// brute_force.hpp: build(res, index_params / metric, dataset) - the index VIEWS the dataset (keep it alive)
template <typename T>
index<T> build(const resources& res, device_matrix_view<const T> dataset, cuvsDistanceType metric = L2Expanded,
               float metric_arg = 2.0f)
{
  index<T> idx;
  detail::tensor<const T> d(dataset);
  check(cuvsBruteForceBuild(res.get(), d.get(), metric, metric_arg, idx.get()), "cuvsBruteForceBuild");
  return idx;
}
template <typename T>
void search(const resources& res, const index<T>& idx, device_matrix_view<const T> queries,
            device_matrix_view<int64_t> neighbors, device_matrix_view<float> distances)
{
  detail::tensor<const T> q(queries);
  detail::tensor<int64_t> n(neighbors);
  detail::tensor<float> d(distances);
  cuvsFilter none{0, NO_FILTER};
  check(cuvsBruteForceSearch(res.get(), idx.get(), q.get(), n.get(), d.get(), none), "cuvsBruteForceSearch");
}

// brute_force.hpp:594-700: sparse_index, build, sparse_search_params, search - the index VIEWS the three arrays (keep them alive)
class sparse_index {
 public:
  sparse_index() { check(cuvsAmdSparseBruteForceIndexCreate(&h_), "cuvsAmdSparseBruteForceIndexCreate"); }
  ~sparse_index() { if (h_) cuvsAmdSparseBruteForceIndexDestroy(h_); }
  sparse_index(sparse_index&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
  sparse_index(const sparse_index&) = delete;
  cuvsAmdSparseBruteForceIndex_t get() const { return h_; }

 private:
  cuvsAmdSparseBruteForceIndex_t h_ = nullptr;
};
struct sparse_search_params {
  int batch_size_index = 2 << 14;
  int batch_size_query = 2 << 14;
};
inline sparse_index build(const resources& res, const csr_view& dataset, cuvsDistanceType metric = L2Expanded, float metric_arg = 2.0f)
{
  sparse_index idx;
  detail::csr_tensors t(dataset);
  check(cuvsAmdSparseBruteForceBuild(res.get(), &t.indptr.m, &t.indices.m, &t.data.m, dataset.rows, dataset.cols, metric, metric_arg,
                                     idx.get()),
        "cuvsAmdSparseBruteForceBuild");
  return idx;
}
// IdxT: int64_t or int32_t (the reference's type)
template <typename IdxT>
void search(const resources& res, const sparse_search_params& params, const sparse_index& idx, const csr_view& queries,
            device_matrix_view<IdxT> neighbors, device_matrix_view<float> distances)
{
  detail::csr_tensors q(queries);
  detail::tensor<IdxT> n(neighbors);
  detail::tensor<float> d(distances);
  check(cuvsAmdSparseBruteForceSearch(res.get(), idx.get(), &q.indptr.m, &q.indices.m, &q.data.m, queries.rows, neighbors.cols,
                                      params.batch_size_index, params.batch_size_query, n.get(), d.get()),
        "cuvsAmdSparseBruteForceSearch");
}
}  // namespace brute_force

namespace ivf_flat {
struct index_params {  // ivf_flat.hpp:29-75
  cuvsDistanceType metric              = L2Expanded;
  float metric_arg                     = 2.0f;
  bool add_data_on_build               = true;
  uint32_t n_lists                     = 1024;
  uint32_t kmeans_n_iters              = 20;
  double kmeans_trainset_fraction      = 0.5;
  bool adaptive_centers                = false;
  bool conservative_memory_allocation  = false;
};
struct search_params {  // ivf_flat.hpp:77-103
  uint32_t n_probes = 20;
};
template <typename T = float>
class index {
 public:
  index() { check(cuvsIvfFlatIndexCreate(&h_), "cuvsIvfFlatIndexCreate"); }
  ~index() { if (h_) cuvsIvfFlatIndexDestroy(h_); }
  index(index&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
  index(const index&) = delete;
  cuvsIvfFlatIndex_t get() const { return h_; }

 private:
  cuvsIvfFlatIndex_t h_ = nullptr;
};
template <typename T>
index<T> build(const resources& res, const index_params& p, device_matrix_view<const T> dataset)
{
  detail::c_params<cuvsIvfFlatIndexParams_t, cuvsIvfFlatIndexParamsCreate, cuvsIvfFlatIndexParamsDestroy> cp;
  *cp.p = cuvsIvfFlatIndexParams{p.metric, p.metric_arg, p.add_data_on_build, p.n_lists, p.kmeans_n_iters,
                                 p.kmeans_trainset_fraction, p.adaptive_centers, p.conservative_memory_allocation};
  index<T> idx;
  detail::tensor<const T> d(dataset);
  check(cuvsIvfFlatBuild(res.get(), cp.p, d.get(), idx.get()), "cuvsIvfFlatBuild");
  return idx;
}
template <typename T>
void search(const resources& res, const search_params& p, const index<T>& idx, device_matrix_view<const T> queries,
            device_matrix_view<int64_t> neighbors, device_matrix_view<float> distances)
{
  detail::c_params<cuvsIvfFlatSearchParams_t, cuvsIvfFlatSearchParamsCreate, cuvsIvfFlatSearchParamsDestroy> cp;
  cp.p->n_probes = p.n_probes;
  detail::tensor<const T> q(queries);
  detail::tensor<int64_t> n(neighbors);
  detail::tensor<float> d(distances);
  cuvsFilter none{0, NO_FILTER};
  check(cuvsIvfFlatSearch(res.get(), cp.p, idx.get(), q.get(), n.get(), d.get(), none), "cuvsIvfFlatSearch");
}
}  // namespace ivf_flat

namespace ivf_sq {
struct index_params {  // ivf_sq.hpp: 8-bit scalar-quantized IVF lists
  cuvsDistanceType metric               = L2Expanded;
  float metric_arg                      = 2.0f;
  bool add_data_on_build                = true;
  uint32_t n_lists                      = 1024;
  uint32_t kmeans_n_iters               = 20;
  uint32_t max_train_points_per_cluster = 256;
  bool conservative_memory_allocation   = false;
};
struct search_params {
  uint32_t n_probes = 20;
};
class index {  // codes are uint8 whatever the row type (float / half) the index was built from
 public:
  index() { check(cuvsIvfSqIndexCreate(&h_), "cuvsIvfSqIndexCreate"); }
  ~index() { if (h_) cuvsIvfSqIndexDestroy(h_); }
  index(index&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
  index(const index&) = delete;
  cuvsIvfSqIndex_t get() const { return h_; }

 private:
  cuvsIvfSqIndex_t h_ = nullptr;
};
template <typename T>
index build(const resources& res, const index_params& p, device_matrix_view<const T> dataset)
{
  detail::c_params<cuvsIvfSqIndexParams_t, cuvsIvfSqIndexParamsCreate, cuvsIvfSqIndexParamsDestroy> cp;
  *cp.p = cuvsIvfSqIndexParams{p.metric, p.metric_arg, p.add_data_on_build, p.n_lists, p.kmeans_n_iters,
                               p.max_train_points_per_cluster, p.conservative_memory_allocation};
  index idx;
  detail::tensor<const T> d(dataset);
  check(cuvsIvfSqBuild(res.get(), cp.p, d.get(), idx.get()), "cuvsIvfSqBuild");
  return idx;
}
template <typename T>
void search(const resources& res, const search_params& p, const index& idx, device_matrix_view<const T> queries,
            device_matrix_view<int64_t> neighbors, device_matrix_view<float> distances)
{
  detail::c_params<cuvsIvfSqSearchParams_t, cuvsIvfSqSearchParamsCreate, cuvsIvfSqSearchParamsDestroy> cp;
  cp.p->n_probes = p.n_probes;
  detail::tensor<const T> q(queries);
  detail::tensor<int64_t> n(neighbors);
  detail::tensor<float> d(distances);
  cuvsFilter none{0, NO_FILTER};
  check(cuvsIvfSqSearch(res.get(), cp.p, idx.get(), q.get(), n.get(), d.get(), none), "cuvsIvfSqSearch");
}
}  // namespace ivf_sq

namespace ivf_rabitq {
struct index_params {  // ivf_rabitq.hpp:38-85
  cuvsDistanceType metric               = L2Expanded;
  uint32_t n_lists                      = 1024;
  uint32_t bits_per_dim                 = 3;
  uint32_t kmeans_n_iters               = 20;
  uint32_t max_train_points_per_cluster = 256;
  bool fast_quantize_flag               = true;
  uint32_t streaming_batch_size         = 100000;
  bool force_streaming                  = false;
};
enum class search_mode { LUT16 = 0, LUT32 = 1, QUANT4 = 2, QUANT8 = 3 };
struct search_params {
  uint32_t n_probes = 20;
  search_mode mode  = search_mode::QUANT4;
};
class index {
 public:
  index() { check(cuvsAmdIvfRabitqIndexCreate(&h_), "cuvsAmdIvfRabitqIndexCreate"); }
  ~index() { if (h_) cuvsAmdIvfRabitqIndexDestroy(h_); }
  index(index&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
  index(const index&) = delete;
  cuvsAmdIvfRabitqIndex_t get() const { return h_; }

 private:
  cuvsAmdIvfRabitqIndex_t h_ = nullptr;
};
// dataset: fp32 rows on the device (make_device_matrix_view) or on the host (make_host_matrix_view)
inline index build(const resources& res, const index_params& p, device_matrix_view<const float> dataset)
{
  detail::c_params<cuvsAmdIvfRabitqIndexParams_t, cuvsAmdIvfRabitqIndexParamsCreate, cuvsAmdIvfRabitqIndexParamsDestroy> cp;
  *cp.p = cuvsAmdIvfRabitqIndexParams{p.metric, p.n_lists, p.bits_per_dim, p.kmeans_n_iters, p.max_train_points_per_cluster,
                                      p.fast_quantize_flag, p.streaming_batch_size, p.force_streaming};
  index idx;
  detail::tensor<const float> d(dataset);
  check(cuvsAmdIvfRabitqBuild(res.get(), cp.p, d.get(), idx.get()), "cuvsAmdIvfRabitqBuild");
  return idx;
}
inline void search(const resources& res, const search_params& p, const index& idx, device_matrix_view<const float> queries,
                   device_matrix_view<int64_t> neighbors, device_matrix_view<float> distances)
{
  detail::c_params<cuvsAmdIvfRabitqSearchParams_t, cuvsAmdIvfRabitqSearchParamsCreate, cuvsAmdIvfRabitqSearchParamsDestroy> cp;
  cp.p->n_probes = p.n_probes;
  cp.p->mode     = static_cast<cuvsAmdIvfRabitqSearchMode>(p.mode);
  detail::tensor<const float> q(queries);
  detail::tensor<int64_t> n(neighbors);
  detail::tensor<float> d(distances);
  check(cuvsAmdIvfRabitqSearch(res.get(), cp.p, idx.get(), q.get(), n.get(), d.get()), "cuvsAmdIvfRabitqSearch");
}
}  // namespace ivf_rabitq

namespace ivf_pq {
enum class codebook_gen { PER_SUBSPACE = 0, PER_CLUSTER = 1 };
struct index_params {  // ivf_pq.hpp:40-160
  cuvsDistanceType metric               = L2Expanded;
  float metric_arg                      = 2.0f;
  bool add_data_on_build                = true;
  uint32_t n_lists                      = 1024;
  uint32_t kmeans_n_iters               = 20;
  double kmeans_trainset_fraction       = 0.5;
  uint32_t pq_bits                      = 8;
  uint32_t pq_dim                       = 0;
  codebook_gen codebook_kind            = codebook_gen::PER_SUBSPACE;
  bool force_random_rotation            = false;
  bool conservative_memory_allocation   = false;
  uint32_t max_train_points_per_pq_code = 256;
};
struct search_params {  // ivf_pq.hpp:162-236
  uint32_t n_probes                      = 20;
  cudaDataType_t lut_dtype               = CUDA_R_32F;
  cudaDataType_t internal_distance_dtype = CUDA_R_32F;
  cudaDataType_t coarse_search_dtype     = CUDA_R_32F;
  uint32_t max_internal_batch_size       = 4096;
  double preferred_shmem_carveout        = 1.0;
};
class index {
 public:
  index() { check(cuvsIvfPqIndexCreate(&h_), "cuvsIvfPqIndexCreate"); }
  ~index() { if (h_) cuvsIvfPqIndexDestroy(h_); }
  index(index&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
  index(const index&) = delete;
  cuvsIvfPqIndex_t get() const { return h_; }
  int64_t size() const { int64_t v = 0; check(cuvsIvfPqIndexGetSize(h_, &v), "cuvsIvfPqIndexGetSize"); return v; }
  int64_t n_lists() const { int64_t v = 0; check(cuvsIvfPqIndexGetNLists(h_, &v), "cuvsIvfPqIndexGetNLists"); return v; }
  int64_t pq_dim() const { int64_t v = 0; check(cuvsIvfPqIndexGetPqDim(h_, &v), "cuvsIvfPqIndexGetPqDim"); return v; }

 private:
  cuvsIvfPqIndex_t h_ = nullptr;
};
template <typename T>
index build(const resources& res, const index_params& p, device_matrix_view<const T> dataset)
{
  detail::c_params<cuvsIvfPqIndexParams_t, cuvsIvfPqIndexParamsCreate, cuvsIvfPqIndexParamsDestroy> cp;
  cp.p->metric = p.metric; cp.p->metric_arg = p.metric_arg; cp.p->add_data_on_build = p.add_data_on_build;
  cp.p->n_lists = p.n_lists; cp.p->kmeans_n_iters = p.kmeans_n_iters;
  cp.p->kmeans_trainset_fraction = p.kmeans_trainset_fraction; cp.p->pq_bits = p.pq_bits; cp.p->pq_dim = p.pq_dim;
  cp.p->codebook_kind = (cuvsIvfPqCodebookGen)p.codebook_kind; cp.p->force_random_rotation = p.force_random_rotation;
  cp.p->conservative_memory_allocation = p.conservative_memory_allocation;
  cp.p->max_train_points_per_pq_code   = p.max_train_points_per_pq_code;
  index idx;
  detail::tensor<const T> d(dataset);
  check(cuvsIvfPqBuild(res.get(), cp.p, d.get(), idx.get()), "cuvsIvfPqBuild");
  return idx;
}
template <typename T>
void extend(const resources& res, device_matrix_view<const T> new_vectors, device_matrix_view<const int64_t> new_indices,
            index* idx)
{
  detail::tensor<const T> v(new_vectors);
  detail::tensor<const int64_t> ids(new_indices);
  ids.m.dl_tensor.ndim = 1;  // [n] ids
  check(cuvsIvfPqExtend(res.get(), v.get(), ids.get(), idx->get()), "cuvsIvfPqExtend");
}
template <typename T>
void search(const resources& res, const search_params& p, const index& idx, device_matrix_view<const T> queries,
            device_matrix_view<int64_t> neighbors, device_matrix_view<float> distances)
{
  detail::c_params<cuvsIvfPqSearchParams_t, cuvsIvfPqSearchParamsCreate, cuvsIvfPqSearchParamsDestroy> cp;
  cp.p->n_probes = p.n_probes; cp.p->lut_dtype = p.lut_dtype; cp.p->internal_distance_dtype = p.internal_distance_dtype;
  cp.p->coarse_search_dtype = p.coarse_search_dtype; cp.p->max_internal_batch_size = p.max_internal_batch_size;
  cp.p->preferred_shmem_carveout = p.preferred_shmem_carveout;
  detail::tensor<const T> q(queries);
  detail::tensor<int64_t> n(neighbors);
  detail::tensor<float> d(distances);
  check(cuvsIvfPqSearch(res.get(), cp.p, idx.get(), q.get(), n.get(), d.get()), "cuvsIvfPqSearch");
}
// search with a sample filter (ivf_pq.hpp:1818-1828); the C entry point is this library's (cuvs_amd/extensions.h)
template <typename T>
void search(const resources& res, const search_params& p, const index& idx, device_matrix_view<const T> queries,
            device_matrix_view<int64_t> neighbors, device_matrix_view<float> distances,
            const filtering::bitset_filter& sample_filter)
{
  detail::c_params<cuvsIvfPqSearchParams_t, cuvsIvfPqSearchParamsCreate, cuvsIvfPqSearchParamsDestroy> cp;
  cp.p->n_probes = p.n_probes; cp.p->lut_dtype = p.lut_dtype; cp.p->internal_distance_dtype = p.internal_distance_dtype;
  cp.p->coarse_search_dtype = p.coarse_search_dtype; cp.p->max_internal_batch_size = p.max_internal_batch_size;
  cp.p->preferred_shmem_carveout = p.preferred_shmem_carveout;
  detail::tensor<const T> q(queries);
  detail::tensor<int64_t> n(neighbors);
  detail::tensor<float> d(distances);
  detail::tensor<const uint32_t> f(device_matrix_view<const uint32_t>{sample_filter.words, 1, (sample_filter.n_bits + 31) / 32, false});
  f.m.dl_tensor.ndim = 1; f.shape[0] = (sample_filter.n_bits + 31) / 32;
  cuvsFilter flt{reinterpret_cast<uintptr_t>(f.get()), BITSET};
  check(cuvsAmdIvfPqSearchFiltered(res.get(), cp.p, idx.get(), q.get(), n.get(), d.get(), flt), "cuvsAmdIvfPqSearchFiltered");
}
}  // namespace ivf_pq

namespace cagra {
struct index_params {  // cagra.hpp:84-200
  cuvsDistanceType metric          = L2Expanded;
  size_t intermediate_graph_degree = 128;
  size_t graph_degree              = 64;
  cuvsCagraGraphBuildAlgo build_algo = IVF_PQ;
  size_t nn_descent_niter          = 20;
  bool guarantee_connectivity      = false;  // cagra.hpp:193 (handle switch here: cuvsAmdCagraSetGuaranteeConnectivity)
};
enum class search_algo { SINGLE_CTA = 0, MULTI_CTA = 1, MULTI_KERNEL = 2, AUTO = 100 };
struct search_params {  // cagra.hpp:203-360
  size_t max_queries          = 0;
  size_t itopk_size           = 64;
  size_t max_iterations       = 0;
  search_algo algo            = search_algo::AUTO;
  size_t team_size            = 0;
  size_t search_width         = 1;
  size_t min_iterations       = 0;
  size_t thread_block_size    = 0;
  size_t hashmap_min_bitlen   = 0;
  float hashmap_max_fill_rate = 0.5f;
  uint32_t num_random_samplings = 1;
  uint64_t rand_xor_mask      = 0x128394;
};
template <typename T = float>
class index {
 public:
  index() { check(cuvsCagraIndexCreate(&h_), "cuvsCagraIndexCreate"); }
  ~index() { if (h_) cuvsCagraIndexDestroy(h_); }
  index(index&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
  index(const index&) = delete;
  cuvsCagraIndex_t get() const { return h_; }
  int64_t size() const { int64_t v = 0; check(cuvsCagraIndexGetSize(h_, &v), "cuvsCagraIndexGetSize"); return v; }
  int64_t graph_degree() const
  {
    int64_t v = 0;
    check(cuvsCagraIndexGetGraphDegree(h_, &v), "cuvsCagraIndexGetGraphDegree");
    return v;
  }

 private:
  cuvsCagraIndex_t h_ = nullptr;
};
template <typename T>
index<T> build(const resources& res, const index_params& p, device_matrix_view<const T> dataset)
{
  detail::c_params<cuvsCagraIndexParams_t, cuvsCagraIndexParamsCreate, cuvsCagraIndexParamsDestroy> cp;
  cp.p->metric = p.metric; cp.p->intermediate_graph_degree = p.intermediate_graph_degree;
  cp.p->graph_degree = p.graph_degree; cp.p->build_algo = p.build_algo; cp.p->nn_descent_niter = p.nn_descent_niter;
  index<T> idx;
  detail::tensor<const T> d(dataset);
  check(cuvsAmdCagraSetGuaranteeConnectivity(res.get(), p.guarantee_connectivity ? 1 : 0), "cuvsAmdCagraSetGuaranteeConnectivity");
  const cuvsError_t rc = cuvsCagraBuild(res.get(), cp.p, d.get(), idx.get());
  cuvsAmdCagraSetGuaranteeConnectivity(res.get(), 0);
  check(rc, "cuvsCagraBuild");
  return idx;
}
// neighbors: uint32_t (the reference's index type) or int64_t
template <typename T, typename IdxT>
void search(const resources& res, const search_params& p, const index<T>& idx, device_matrix_view<const T> queries,
            device_matrix_view<IdxT> neighbors, device_matrix_view<float> distances)
{
  detail::c_params<cuvsCagraSearchParams_t, cuvsCagraSearchParamsCreate, cuvsCagraSearchParamsDestroy> cp;
  cp.p->max_queries = p.max_queries; cp.p->itopk_size = p.itopk_size; cp.p->max_iterations = p.max_iterations;
  cp.p->algo = (cuvsCagraSearchAlgo)p.algo; cp.p->team_size = p.team_size; cp.p->search_width = p.search_width;
  cp.p->min_iterations = p.min_iterations; cp.p->thread_block_size = p.thread_block_size;
  cp.p->hashmap_min_bitlen = p.hashmap_min_bitlen; cp.p->hashmap_max_fill_rate = p.hashmap_max_fill_rate;
  cp.p->num_random_samplings = p.num_random_samplings; cp.p->rand_xor_mask = p.rand_xor_mask;
  detail::tensor<const T> q(queries);
  detail::tensor<IdxT> n(neighbors);
  detail::tensor<float> d(distances);
  cuvsFilter none{0, NO_FILTER};
  check(cuvsCagraSearch(res.get(), cp.p, idx.get(), q.get(), n.get(), d.get(), none), "cuvsCagraSearch");
}
}  // namespace cagra

namespace vamana {
struct index_params {  // vamana.hpp: the C fields under the reference's C++ names and defaults
  cuvsDistanceType metric    = L2Expanded;
  uint32_t graph_degree      = 32;
  uint32_t visited_size      = 64;
  float vamana_iters         = 1.0f;
  float alpha                = 1.2f;
  float max_fraction         = 0.06f;
  float batch_base           = 2.0f;
  uint32_t queue_size        = 127;
  uint32_t reverse_batchsize = 1000000;
};
template <typename T = float>
class index {
 public:
  index() { check(cuvsVamanaIndexCreate(&h_), "cuvsVamanaIndexCreate"); }
  ~index() { if (h_) cuvsVamanaIndexDestroy(h_); }
  index(index&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
  index(const index&) = delete;
  cuvsVamanaIndex_t get() const { return h_; }
  int dim() const { int v = 0; check(cuvsVamanaIndexGetDims(h_, &v), "cuvsVamanaIndexGetDims"); return v; }
  uint32_t medoid() const { uint32_t v = 0; check(cuvsAmdVamanaIndexGetMedoid(h_, &v), "cuvsAmdVamanaIndexGetMedoid"); return v; }

 private:
  cuvsVamanaIndex_t h_ = nullptr;
};
// dataset: a device or a host view of float, int8_t or uint8_t rows; the index keeps its own device copy
template <typename T>
index<T> build(const resources& res, const index_params& p, device_matrix_view<const T> dataset)
{
  detail::c_params<cuvsVamanaIndexParams_t, cuvsVamanaIndexParamsCreate, cuvsVamanaIndexParamsDestroy> cp;
  *cp.p = cuvsVamanaIndexParams{p.metric, p.graph_degree, p.visited_size, p.vamana_iters, p.alpha, p.max_fraction, p.batch_base,
                                p.queue_size, p.reverse_batchsize};
  index<T> idx;
  detail::tensor<const T> d(dataset);
  check(cuvsVamanaBuild(res.get(), cp.p, d.get(), idx.get()), "cuvsVamanaBuild");
  return idx;
}
// vamana.hpp serialize(res, file_prefix, index, include_dataset, sector_aligned)
template <typename T>
void serialize(const resources& res, const std::string& file_prefix, const index<T>& idx, bool include_dataset = true,
               bool sector_aligned = false)
{
  if (sector_aligned)
    check(cuvsAmdVamanaSerializeSectorAligned(res.get(), file_prefix.c_str(), idx.get(), include_dataset),
          "cuvsAmdVamanaSerializeSectorAligned");
  else
    check(cuvsVamanaSerialize(res.get(), file_prefix.c_str(), idx.get(), include_dataset), "cuvsVamanaSerialize");
}
}  // namespace vamana

namespace epsilon_neighborhood {
// epsilon_neighborhood.hpp compute(handle, x, y, adj, vd, eps, metric): adj bool [m, n] and vd [m + 1] (IdxT int32_t or
// int64_t) on the device; a view with a null pointer leaves that output out. eps is the squared radius.
template <typename T, typename IdxT>
void compute(const resources& res, device_matrix_view<const T> x, device_matrix_view<const T> y, device_matrix_view<bool> adj,
             IdxT* vd, float eps, cuvsDistanceType metric = L2Unexpanded)
{
  detail::tensor<const T> tx(x), ty(y);
  detail::tensor<bool> ta(adj);
  detail::vector_tensor<IdxT> tv(vd, x.extent(0) + 1);
  check(cuvsAmdEpsNeighbors(res.get(), tx.get(), ty.get(), adj.ptr ? ta.get() : nullptr, tv.get(), eps, metric), "cuvsAmdEpsNeighbors");
}
// The CSR forms of ball_cover::eps_nn served by brute force: indptr int64 [m + 1]; indices (int64, `indices_len` entries) and
// distances (fp32, as long) may be null; vd int64 [m + 1] may be null. max_k == nullptr: the count call (indices null) and the
// fill call; otherwise one call that keeps the first *max_k ids of a row and returns the largest degree in *max_k.
template <typename T>
void csr(const resources& res, device_matrix_view<const T> x, device_matrix_view<const T> y, int64_t* indptr, int64_t* indices,
         float* distances, int64_t indices_len, int64_t* vd, float eps, int64_t* max_k = nullptr,
         cuvsDistanceType metric = L2Unexpanded)
{
  detail::tensor<const T> tx(x), ty(y);
  detail::vector_tensor<int64_t> tp(indptr, x.extent(0) + 1), ti(indices, indices_len), tv(vd, x.extent(0) + 1);
  detail::vector_tensor<float> td(distances, indices_len);
  check(cuvsAmdEpsNeighborsCsr(res.get(), tx.get(), ty.get(), tp.get(), ti.get(), td.get(), tv.get(), eps, metric, max_k),
        "cuvsAmdEpsNeighborsCsr");
}
}  // namespace epsilon_neighborhood

namespace ball_cover {
// ball_cover.hpp: a landmark index over 2-D / 3-D fp32 rows (eps_nn: up to 32 columns), exact k-NN and eps_nn through it.
// Unlike the reference's index, this one owns a reordered copy of the rows: the dataset need not outlive build().
struct index_params {
  cuvsDistanceType metric = L2SqrtExpanded;  // L2SqrtExpanded, L2SqrtUnexpanded or Haversine
  uint32_t n_landmarks    = 0;               // 0: floor(sqrt(m))
  uint32_t seed           = 0;
};
class index {
 public:
  index() { check(cuvsAmdBallCoverIndexCreate(&h_), "cuvsAmdBallCoverIndexCreate"); }
  ~index() { if (h_) cuvsAmdBallCoverIndexDestroy(h_); }
  index(index&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
  index(const index&) = delete;
  cuvsAmdBallCoverIndex_t get() const { return h_; }
  int64_t n_landmarks() const { int64_t v = 0; check(cuvsAmdBallCoverIndexGetNLandmarks(h_, &v), "cuvsAmdBallCoverIndexGetNLandmarks"); return v; }
  int64_t size() const { int64_t v = 0; check(cuvsAmdBallCoverIndexGetSize(h_, &v), "cuvsAmdBallCoverIndexGetSize"); return v; }
  int64_t dim() const { int64_t v = 0; check(cuvsAmdBallCoverIndexGetDim(h_, &v), "cuvsAmdBallCoverIndexGetDim"); return v; }
  cuvsDistanceType metric() const
  {
    cuvsDistanceType v = L2SqrtExpanded;
    check(cuvsAmdBallCoverIndexGetMetric(h_, &v), "cuvsAmdBallCoverIndexGetMetric");
    return v;
  }

 private:
  cuvsAmdBallCoverIndex_t h_ = nullptr;
};
using c_index_params = detail::c_params<cuvsAmdBallCoverIndexParams_t, cuvsAmdBallCoverIndexParamsCreate, cuvsAmdBallCoverIndexParamsDestroy>;
inline index build(const resources& res, const index_params& p, device_matrix_view<const float> dataset)
{
  c_index_params cp;
  *cp.p = cuvsAmdBallCoverIndexParams{p.metric, p.n_landmarks, p.seed};
  index idx;
  detail::tensor<const float> d(dataset);
  check(cuvsAmdBallCoverBuild(res.get(), cp.p, d.get(), idx.get()), "cuvsAmdBallCoverBuild");
  return idx;
}
// neighbors int64 [q, k] and distances fp32 [q, k], rows sorted by (distance, id); the defaults give brute force's answer
inline void knn_query(const resources& res, const index& idx, device_matrix_view<const float> queries, device_matrix_view<int64_t> neighbors,
                      device_matrix_view<float> distances, bool perform_post_filtering = true, float weight = 1.0f)
{
  detail::tensor<const float> q(queries);
  detail::tensor<int64_t> n(neighbors);
  detail::tensor<float> d(distances);
  check(cuvsAmdBallCoverKnnQuery(res.get(), idx.get(), q.get(), n.get(), d.get(), perform_post_filtering, weight), "cuvsAmdBallCoverKnnQuery");
}
// build + the dataset queried against itself; returns the index
inline index all_knn_query(const resources& res, const index_params& p, device_matrix_view<const float> dataset,
                           device_matrix_view<int64_t> neighbors, device_matrix_view<float> distances, bool perform_post_filtering = true,
                           float weight = 1.0f)
{
  c_index_params cp;
  *cp.p = cuvsAmdBallCoverIndexParams{p.metric, p.n_landmarks, p.seed};
  index idx;
  detail::tensor<const float> x(dataset);
  detail::tensor<int64_t> n(neighbors);
  detail::tensor<float> d(distances);
  check(cuvsAmdBallCoverAllKnnQuery(res.get(), cp.p, x.get(), n.get(), d.get(), perform_post_filtering, weight, idx.get()),
        "cuvsAmdBallCoverAllKnnQuery");
  return idx;
}
// eps_nn, dense: adj bool [q, m] and vd [q + 1] as epsilon_neighborhood::compute; eps is the radius
template <typename IdxT>
void eps_nn(const resources& res, const index& idx, device_matrix_view<const float> queries, device_matrix_view<bool> adj, IdxT* vd, float eps)
{
  detail::tensor<const float> q(queries);
  detail::tensor<bool> ta(adj);
  detail::vector_tensor<IdxT> tv(vd, queries.extent(0) + 1);
  check(cuvsAmdBallCoverEpsNn(res.get(), idx.get(), q.get(), adj.ptr ? ta.get() : nullptr, tv.get(), eps), "cuvsAmdBallCoverEpsNn");
}
// eps_nn, CSR: the protocols of epsilon_neighborhood::csr
inline void eps_nn(const resources& res, const index& idx, device_matrix_view<const float> queries, int64_t* indptr, int64_t* indices,
                   float* distances, int64_t indices_len, int64_t* vd, float eps, int64_t* max_k = nullptr)
{
  detail::tensor<const float> q(queries);
  detail::vector_tensor<int64_t> tp(indptr, queries.extent(0) + 1), ti(indices, indices_len), tv(vd, queries.extent(0) + 1);
  detail::vector_tensor<float> td(distances, indices_len);
  check(cuvsAmdBallCoverEpsNnCsr(res.get(), idx.get(), q.get(), tp.get(), ti.get(), td.get(), tv.get(), eps, max_k), "cuvsAmdBallCoverEpsNnCsr");
}
// the calling thread's last query: lists visited, rows scored, rows skipped by the window, queries
inline std::array<uint64_t, 4> last_stats()
{
  std::array<uint64_t, 4> out{};
  check(cuvsAmdBallCoverLastStats(out.data()), "cuvsAmdBallCoverLastStats");
  return out;
}
}  // namespace ball_cover

namespace experimental {
namespace scann {
// scann.hpp: build-only. Partitions by balanced k-means, AVQ centres, SOAR labels, PQ codes of both residuals, optional bf16 rows,
// and the files open-source ScaNN reads (include/cuvs_amd/scann.h). pq_dim is the width of a subspace.
struct index_params {
  cuvsDistanceType metric     = L2Expanded;
  float metric_arg            = 2.0f;
  uint32_t n_leaves           = 1000;
  int64_t kmeans_n_rows_train = 100000;
  uint32_t kmeans_n_iters     = 24;
  float partitioning_eta      = 1;
  float soar_lambda           = 1;
  uint32_t pq_dim             = 8;
  uint32_t pq_bits            = 8;
  int64_t pq_n_rows_train     = 100000;
  uint32_t pq_train_iters     = 10;
  bool reordering_bf16        = false;
  float reordering_noise_shaping_threshold = NAN;
};
class index {
 public:
  index() { check(cuvsAmdScannIndexCreate(&h_), "cuvsAmdScannIndexCreate"); }
  ~index() { if (h_) cuvsAmdScannIndexDestroy(h_); }
  index(index&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
  index(const index&) = delete;
  cuvsAmdScannIndex_t get() const { return h_; }
  int64_t size() const { return scalar(cuvsAmdScannIndexGetSize); }
  int64_t dim() const { return scalar(cuvsAmdScannIndexGetDim); }
  int64_t n_leaves() const { return scalar(cuvsAmdScannIndexGetNLeaves); }
  int64_t pq_dim() const { return scalar(cuvsAmdScannIndexGetPqDim); }
  int64_t pq_bits() const { return scalar(cuvsAmdScannIndexGetPqBits); }
  // views into the index (valid while it lives): the first four on the device, the codes and the bf16 rows on the host
  device_matrix_view<const float> centers() const { return view<const float>(cuvsAmdScannIndexGetCenters, false); }
  device_matrix_view<const uint32_t> labels() const { return view<const uint32_t>(cuvsAmdScannIndexGetLabels, false); }
  device_matrix_view<const uint32_t> soar_labels() const { return view<const uint32_t>(cuvsAmdScannIndexGetSoarLabels, false); }
  device_matrix_view<const float> pq_codebook() const { return view<const float>(cuvsAmdScannIndexGetPqCodebook, false); }
  device_matrix_view<const uint8_t> quantized_residuals() const { return view<const uint8_t>(cuvsAmdScannIndexGetCodes, true); }
  device_matrix_view<const uint8_t> quantized_soar_residuals() const { return view<const uint8_t>(cuvsAmdScannIndexGetSoarCodes, true); }
  device_matrix_view<const int16_t> bf16_dataset() const
  {
    bool has = false;
    check(cuvsAmdScannIndexHasBf16(h_, &has), "cuvsAmdScannIndexHasBf16");
    return has ? view<const int16_t>(cuvsAmdScannIndexGetBf16Dataset, true) : device_matrix_view<const int16_t>{nullptr, 0, 0, true};
  }

 private:
  int64_t scalar(cuvsError_t (*fn)(cuvsAmdScannIndex_t, int64_t*)) const
  {
    int64_t v = 0;
    check(fn(h_, &v), "cuvsAmdScannIndexGet*");
    return v;
  }
  template <typename T>
  device_matrix_view<T> view(cuvsError_t (*fn)(cuvsAmdScannIndex_t, DLManagedTensor*), bool on_host) const
  {
    DLManagedTensor m{};
    check(fn(h_, &m), "cuvsAmdScannIndexGet*");
    device_matrix_view<T> v{static_cast<T*>(m.dl_tensor.data), m.dl_tensor.shape[0], m.dl_tensor.ndim > 1 ? m.dl_tensor.shape[1] : 1, on_host};
    if (m.deleter) m.deleter(&m);
    return v;
  }
  cuvsAmdScannIndex_t h_ = nullptr;
};
using c_index_params = detail::c_params<cuvsAmdScannIndexParams_t, cuvsAmdScannIndexParamsCreate, cuvsAmdScannIndexParamsDestroy>;
// dataset on the device (make_device_matrix_view) or on the host (make_host_matrix_view: streamed in batches, same index)
inline index build(const resources& res, const index_params& p, device_matrix_view<const float> dataset)
{
  c_index_params cp;
  *cp.p = cuvsAmdScannIndexParams{p.metric,  p.metric_arg, p.n_leaves,        p.kmeans_n_rows_train, p.kmeans_n_iters, p.partitioning_eta, p.soar_lambda,
                                  p.pq_dim,  p.pq_bits,    p.pq_n_rows_train, p.pq_train_iters,      p.reordering_bf16,
                                  p.reordering_noise_shaping_threshold};
  index idx;
  detail::tensor<const float> d(dataset);
  check(cuvsAmdScannBuild(res.get(), cp.p, d.get(), idx.get()), "cuvsAmdScannBuild");
  return idx;
}
// writes the index files into the existing directory
inline void serialize(const resources& res, const std::string& scann_assets_dir, const index& idx)
{
  check(cuvsAmdScannSerialize(res.get(), scann_assets_dir.c_str(), idx.get()), "cuvsAmdScannSerialize");
}
// the three stages on their own (device tensors; labels uint32 [n_rows])
inline void avq_centers(const resources& res, device_matrix_view<const float> dataset, const uint32_t* labels, device_matrix_view<float> centers,
                        float eta)
{
  detail::tensor<const float> d(dataset);
  detail::tensor<float> c(centers);
  detail::vector_tensor<const uint32_t> l(labels, dataset.extent(0));
  check(cuvsAmdScannAvqCenters(res.get(), d.get(), &l.m, c.get(), eta), "cuvsAmdScannAvqCenters");
}
inline void soar_labels(const resources& res, device_matrix_view<const float> dataset, device_matrix_view<const float> centers,
                        const uint32_t* labels, float lambda, uint32_t* soar_labels_out)
{
  detail::tensor<const float> d(dataset), c(centers);
  detail::vector_tensor<const uint32_t> l(labels, dataset.extent(0));
  detail::vector_tensor<uint32_t> o(soar_labels_out, dataset.extent(0));
  check(cuvsAmdScannSoarLabels(res.get(), d.get(), c.get(), &l.m, lambda, &o.m), "cuvsAmdScannSoarLabels");
}
inline void quantize_bf16(const resources& res, device_matrix_view<const float> dataset, float threshold, device_matrix_view<int16_t> out)
{
  detail::tensor<const float> d(dataset);
  detail::tensor<int16_t> o(out);
  check(cuvsAmdScannQuantizeBf16(res.get(), d.get(), threshold, o.get()), "cuvsAmdScannQuantizeBf16");
}
}  // namespace scann
}  // namespace experimental

}  // namespace neighbors
}  // namespace cuvs

// the extensions (ball_cover, epsilon_neighborhood, ivf_rabitq entry points) are also reachable under the library's own name
namespace cuvs_amd {
namespace neighbors = ::cuvs::neighbors;
}
