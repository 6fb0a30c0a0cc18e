// cuvsHnsw* (drop-in for c/src/neighbors/hnsw.cpp): a CAGRA graph handed over to host search as an HNSW index. DESIGN 3.1r.
//
// The device's share is the conversion, and only that: the level of every row (a hash, hnsw_levels_kernel), the rows of each
// level gathered and their kNN among themselves by the CAGRA build's own machinery (cagra_rows_knn_graph: exact below 200000
// rows, IVF-PQ + refine above), local ids mapped back (hnsw_remap_kernel), and the level-0 records {count, links, row, label}
// interleaved in device memory (hnsw_pack_kernel) and streamed out through two pinned buffers. The index, its search, its
// insert and its files are host code by the API's contract (host tensors, uint64 neighbours, a thread count): hnsw_host.hpp.
// cuvsHnswDeserialize / Search / Extend / Serialize and the Create / Destroy functions never touch the HIP runtime nor `res`.
#include "ops.hpp"
#include "hnsw_host.hpp"

#include <cuvs/neighbors/hnsw.h>

#include <sys/stat.h>

using namespace cuvs_amd;
namespace hh = cuvs_amd::hnsw;

namespace {

constexpr uint32_t kNoNode = 0xffffffffu;

__global__ void hnsw_levels_kernel(hh::level_rule rule, int64_t n, uint32_t* __restrict__ levels)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) levels[i] = (uint32_t)hh::level_of(rule, (uint32_t)i);
}

// rows[ids[i]] -> out[i] (a wave per row, strided over the rows; words where the rows allow it)
__global__ __launch_bounds__(256) void hnsw_gather_kernel(const char* __restrict__ rows, const uint32_t* __restrict__ ids, int64_t n_ids,
                                                          size_t row_bytes, int words, char* __restrict__ out)
{
  const int lane = threadIdx.x & 63;
  for (int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < n_ids; i += (int64_t)gridDim.x * 4) {
    const char* src = rows + (size_t)ids[i] * row_bytes;
    char* dst       = out + (size_t)i * row_bytes;
    if (words) {
      for (size_t w = lane; w < row_bytes / 4; w += 64) reinterpret_cast<uint32_t*>(dst)[w] = reinterpret_cast<const uint32_t*>(src)[w];
    } else {
      for (size_t b = lane; b < row_bytes; b += 64) dst[b] = src[b];
    }
  }
}

// kNN ids among the n_ids gathered rows -> ids of the index (what is no local id stays kNoNode)
__global__ void hnsw_remap_kernel(uint32_t* __restrict__ knn, int64_t count, const uint32_t* __restrict__ ids, int64_t n_ids)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const uint32_t v = knn[i];
  knn[i] = v < (uint64_t)n_ids ? ids[v] : kNoNode;
}

// Level-0 records of rows r0 .. r0 + nr: {uint32 degree, uint32 links[max_m0] (degree used, the rest 0), row, uint64 label}.
// A wave per record, its lanes over consecutive 4-byte words of the record: the graph row, the dataset row and the record are
// each one contiguous stream per wave (coalesced loads and stores of 256 B). WORDS = false is the same at byte granularity for
// records that are no multiple of 4 bytes (odd dims of 1- and 2-byte rows) or rows that do not start on a word.
template <bool WORDS>
__global__ __launch_bounds__(256) void hnsw_pack_kernel(const uint32_t* __restrict__ graph, const char* __restrict__ rows, int64_t r0,
                                                        int64_t nr, uint32_t degree, uint32_t max_m0, size_t row_bytes,
                                                        size_t per_elem, char* __restrict__ out)
{
  const int lane        = threadIdx.x & 63;
  const size_t off_data = 4 * (size_t)max_m0 + 4, off_label = off_data + row_bytes;
  for (int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < nr; i += (int64_t)gridDim.x * 4) {
    const uint64_t id   = (uint64_t)(r0 + i);
    const uint32_t* g   = graph + id * degree;
    const char* row     = rows + id * row_bytes;
    char* rec           = out + (size_t)i * per_elem;
    if constexpr (WORDS) {
      uint32_t* o           = reinterpret_cast<uint32_t*>(rec);
      const uint32_t* rw    = reinterpret_cast<const uint32_t*>(row);
      const size_t w_data   = off_data / 4, w_label = off_label / 4, w_all = per_elem / 4;
      for (size_t w = lane; w < w_all; w += 64) {
        uint32_t v;
        if (w == 0) v = degree;
        else if (w <= degree) v = g[w - 1];
        else if (w < w_data) v = 0u;
        else if (w < w_label) v = rw[w - w_data];
        else v = w == w_label ? (uint32_t)id : (uint32_t)(id >> 32);
        o[w] = v;
      }
    } else {
      for (size_t b = lane; b < per_elem; b += 64) {
        uint8_t v;
        if (b < off_data) {
          const size_t w   = b / 4;
          const uint32_t x = w == 0 ? degree : (w <= degree ? g[w - 1] : 0u);
          v = (uint8_t)(x >> (8 * (b & 3)));
        } else if (b < off_label) {
          v = (uint8_t)row[b - off_data];
        } else {
          v = (uint8_t)(id >> (8 * (b - off_label)));
        }
        rec[b] = (char)v;
      }
    }
  }
}

struct pinned_buf {
  char* p = nullptr;
  ~pinned_buf() { if (p) (void)hipHostFree(p); }
};
struct event_pair {
  hipEvent_t e[2] = {nullptr, nullptr};
  ~event_pair() { for (auto x : e) if (x) (void)hipEventDestroy(x); }
};

// level 0 of the index: the records packed on the device chunk by chunk, each chunk copied out through one of two pinned
// buffers while the next is packed. CUVS_AMD_HNSW_PACK_HOST=1 (behind the debug gate): graph and rows copied out and
// interleaved by the host, as cuvsCagraSerializeToHnswlib does (the comparator of scripts/bench_hnsw.py and of the tests).
void pack_level0(resources& res, const uint32_t* graph, const char* rows, uint32_t degree, hh::index& ix)
{
  const size_t n = ix.n, per = ix.per_elem, rb = ix.dim * hh::dtype_size(ix.dtype);
  size_t chunk = std::max<size_t>(1, (size_t(32) << 20) / per);
  if (res.tune.hnsw_pack_rows > 0) chunk = (size_t)res.tune.hnsw_pack_rows;
  chunk = std::min(chunk, n);
  if (res.tune.hnsw_pack_host) {
    std::vector<uint32_t> g(chunk * degree);
    std::vector<char> r(chunk * rb);
    for (size_t r0 = 0; r0 < n; r0 += chunk) {
      const size_t nr = std::min(chunk, n - r0);
      copy_async(res, g.data(), graph + r0 * degree, nr * degree * 4);
      copy_async(res, r.data(), rows + r0 * rb, nr * rb);
      sync(res);
      for (size_t i = 0; i < nr; ++i) hh::make_record(ix, r0 + i, g.data() + i * degree, degree, r.data() + i * rb);
    }
    return;
  }
  const bool words = per % 4 == 0 && rb % 4 == 0 && (reinterpret_cast<uintptr_t>(rows) & 3) == 0;
  pinned_buf host[2];
  event_pair ev;
  dev_buf<char> dev[2] = {dev_buf<char>(res, chunk * per), dev_buf<char>(res, chunk * per)};
  for (int b = 0; b < 2; ++b) {
    HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&host[b].p), chunk * per));
    HIP_TRY(hipEventCreateWithFlags(&ev.e[b], hipEventDisableTiming));
  }
  const unsigned grid_cap = (unsigned)res.num_cus * 16;
  size_t prev_r0 = 0, prev_nr = 0;
  int c = 0;
  for (size_t r0 = 0; r0 < n; r0 += chunk, ++c) {
    const size_t nr = std::min(chunk, n - r0);
    const int b     = c & 1;
    const dim3 grid((unsigned)std::min<size_t>((nr + 3) / 4, grid_cap));
    if (words)
      hipLaunchKernelGGL(hnsw_pack_kernel<true>, grid, dim3(256), 0, res.stream, graph, rows, (int64_t)r0, (int64_t)nr, degree,
                         (uint32_t)ix.maxM0, rb, per, dev[b].data());
    else
      hipLaunchKernelGGL(hnsw_pack_kernel<false>, grid, dim3(256), 0, res.stream, graph, rows, (int64_t)r0, (int64_t)nr, degree,
                         (uint32_t)ix.maxM0, rb, per, dev[b].data());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(host[b].p, dev[b].data(), nr * per, hipMemcpyDeviceToHost, res.stream));
    HIP_TRY(hipEventRecord(ev.e[b], res.stream));
    if (prev_nr) {  // the chunk before this one has arrived: into the index while this one is packed and copied
      HIP_TRY(hipEventSynchronize(ev.e[b ^ 1]));
      memcpy(ix.rec(prev_r0), host[b ^ 1].p, prev_nr * per);
    }
    prev_r0 = r0; prev_nr = nr;
  }
  HIP_TRY(hipEventSynchronize(ev.e[(c - 1) & 1]));
  memcpy(ix.rec(prev_r0), host[(c - 1) & 1].p, prev_nr * per);
}

// the GPU hierarchy: for every level l >= 1 the kNN graph of the rows of level >= l among themselves (K = min(M, n_l - 1))
void gpu_hierarchy(resources& res, const char* rows, hh::index& ix)
{
  const int64_t n = (int64_t)ix.n;
  const size_t rb = ix.dim * hh::dtype_size(ix.dtype);
  const hh::level_rule rule = hh::make_level_rule(ix.M);
  constexpr uint32_t n_labels = hh::kMaxLevels + 1;
  dev_buf<uint32_t> lev(res, n), perm(res, n), off(res, n_labels + 1);
  hipLaunchKernelGGL(hnsw_levels_kernel, dim3(grid_blocks(n, 256)), dim3(256), 0, res.stream, rule, n, lev.data());
  HIP_TRY(hipGetLastError());
  group_by_label(res, lev.data(), n, n_labels, perm.data(), off.data());  // rows ordered by (level, id)
  const std::vector<uint32_t> hlev = to_host(res, lev.data(), (size_t)n);
  const std::vector<uint32_t> hoff = to_host(res, off.data(), (size_t)n_labels + 1);
  for (int64_t i = 0; i < n; ++i) {
    ix.levels[i] = (int32_t)hlev[i];
    ix.upper[i].assign((size_t)hlev[i] * (ix.maxM + 1), 0u);
  }
  hh::set_entry_from_levels(ix);
  const bool words = rb % 4 == 0 && (reinterpret_cast<uintptr_t>(rows) & 3) == 0;
  std::vector<uint32_t> ids, knn, list;
  for (int l = ix.maxlevel; l >= 1; --l) {
    const int64_t first = hoff[l], n_l = n - first;  // the rows of level >= l: perm[first .. n)
    if (n_l < 2) continue;                           // a set of one point has no list
    const uint32_t K = (uint32_t)std::min<int64_t>((int64_t)ix.maxM, n_l - 1);
    const uint32_t* ids_d = perm.data() + first;
    dev_buf<char> sub(res, (size_t)n_l * rb);
    dev_buf<uint32_t> g(res, (size_t)n_l * K);
    hipLaunchKernelGGL(hnsw_gather_kernel, dim3((unsigned)std::min<int64_t>((n_l + 3) / 4, (int64_t)res.num_cus * 16)), dim3(256), 0,
                       res.stream, rows, ids_d, n_l, rb, words ? 1 : 0, sub.data());
    HIP_TRY(hipGetLastError());
    cagra_rows_knn_graph(res, sub.data(), (elem_t)ix.dtype, n_l, (int64_t)ix.dim, K, ix.metric, g.data());
    hipLaunchKernelGGL(hnsw_remap_kernel, dim3(grid_blocks(n_l * (int64_t)K, 256)), dim3(256), 0, res.stream, g.data(), n_l * (int64_t)K,
                       ids_d, n_l);
    HIP_TRY(hipGetLastError());
    ids = to_host(res, ids_d, (size_t)n_l);
    knn = to_host(res, g.data(), (size_t)n_l * K);
    for (int64_t i = 0; i < n_l; ++i) {
      list.clear();
      for (uint32_t j = 0; j < K; ++j)
        if (knn[(size_t)i * K + j] != kNoNode) list.push_back(knn[(size_t)i * K + j]);
      ix.set_list(ids[i], l, list.data(), list.size());
    }
  }
}

void check_metric(int metric)
{
  CUVS_EXPECTS(metric != M_BitwiseHamming, "hnsw: there is no BitwiseHamming space; a Hamming index cannot be converted");
  CUVS_EXPECTS(metric == M_L2Expanded || metric == M_InnerProduct, "Unsupported metric type was used");
}
int check_hierarchy(int h)
{
  CUVS_EXPECTS(h == NONE || h == CPU || h == GPU, "hnsw: unknown hierarchy %d", h);
  return h;
}
hh::index& get_hnsw(cuvsHnswIndex_t index)
{
  CUVS_EXPECTS(index != nullptr && index->addr != 0, "HNSW index is not built");
  return *reinterpret_cast<hh::index*>(index->addr);
}
void set_hnsw(cuvsHnswIndex_t index, std::unique_ptr<hh::index> ix, DLDataType dt)
{
  delete reinterpret_cast<hh::index*>(index->addr);
  index->addr  = reinterpret_cast<uintptr_t>(ix.release());
  index->dtype = dt;
}

void from_cagra(cuvsResources_t res_h, cuvsHnswIndexParams_t params, cuvsCagraIndex_t cagra_index, cuvsHnswIndex_t hnsw_index,
                DLManagedTensor* dataset_tensor, bool with_dataset)
{
  CUVS_EXPECTS(params && cagra_index && hnsw_index, "null argument");
  CUVS_EXPECTS(!with_dataset || dataset_tensor != nullptr, "dataset_tensor is null");
  const cagra_view cv = cagra_index_view(cagra_index->addr);
  const int hierarchy = check_hierarchy((int)params->hierarchy);
  // refusals come from the arguments alone, before the handle or the device is touched
  check_metric(cv.metric);
  if (with_dataset) {
    auto& ds = dataset_tensor->dl_tensor;
    CUVS_EXPECTS(ds.ndim == 2 && is_c_contiguous(ds), "dataset must be a row-major matrix");
    CUVS_EXPECTS(ds.shape[0] == cv.n && ds.shape[1] == cv.dim, "hnsw::from_cagra: the dataset is [%ld, %ld], the index holds [%ld, %ld]",
                 (long)ds.shape[0], (long)ds.shape[1], (long)cv.n, (long)cv.dim);
    CUVS_EXPECTS(elem_of(ds.dtype) == cv.dtype, "hnsw::from_cagra: the dataset's dtype differs from the index's");
    CUVS_EXPECTS(is_device_accessible(ds) || is_host_accessible(ds), "dataset must be accessible on host or device memory");
  } else {
    CUVS_EXPECTS(!cv.vpq && cv.data != nullptr, "hnsw::from_cagra: the CAGRA index holds a VPQ dataset (compressed rows only); pass the "
                                                "original rows with cuvsHnswFromCagraWithDataset");
  }
  CUVS_EXPECTS(cv.n > 0 && cv.n < (int64_t(1) << 32) - 1 && cv.degree > 0, "hnsw::from_cagra: the CAGRA index is empty");
  auto& res = *as_res(res_h);
  const size_t rb = (size_t)cv.dim * elem_size(cv.dtype);
  const char* rows = static_cast<const char*>(cv.data);
  dev_buf<char> up;
  if (with_dataset) {
    auto& ds = dataset_tensor->dl_tensor;
    rows     = static_cast<const char*>(dl_data(ds));
    if (!is_device_accessible(ds)) {
      up = dev_buf<char>(res, (size_t)cv.n * rb);
      copy_async(res, up.data(), rows, up.bytes());
      sync(res);  // (pageable source)
      rows = up.data();
    }
  }
  auto ix = hh::make_index((int)cv.dtype, cv.metric, hierarchy, (size_t)cv.dim, (size_t)cv.n, cv.degree,
                           (size_t)std::max(1, params->ef_construction));
  pack_level0(res, cv.graph, rows, cv.degree, *ix);
  if (hierarchy == CPU) hh::build_cpu_hierarchy(*ix);
  if (hierarchy == GPU) gpu_hierarchy(res, rows, *ix);
  sync(res);
  set_hnsw(hnsw_index, std::move(ix), cagra_index->dtype);
}

void make_dirs(const std::string& dir)
{
  for (size_t i = 1; i <= dir.size(); ++i)
    if (i == dir.size() || dir[i] == '/') (void)mkdir(dir.substr(0, i).c_str(), 0755);
}

struct cagra_handles {
  cuvsCagraIndexParams_t params = nullptr;
  cuvsCagraIndex_t index        = nullptr;
  ~cagra_handles()
  {
    if (index) (void)cuvsCagraIndexDestroy(index);
    if (params) (void)cuvsCagraIndexParamsDestroy(params);
  }
};
void expect_ok(cuvsError_t e, const char* what)
{
  if (e != CUVS_SUCCESS) {
    const char* t = cuvsGetLastErrorText();
    CUVS_FAIL("%s: %s", what, t ? t : "failed");
  }
}
}  // namespace

extern "C" {

cuvsError_t cuvsHnswAceParamsCreate(cuvsHnswAceParams_t* params)
{
  return (cuvsError_t)translate_exceptions([=] { *params = new cuvsHnswAceParams{0, "/tmp/hnsw_ace_build", false, 0, 0}; });
}
cuvsError_t cuvsHnswAceParamsDestroy(cuvsHnswAceParams_t params)
{
  return (cuvsError_t)translate_exceptions([=] { delete params; });
}
cuvsError_t cuvsHnswIndexParamsCreate(cuvsHnswIndexParams_t* params)
{
  return (cuvsError_t)translate_exceptions([=] { *params = new cuvsHnswIndexParams{GPU, 200, 0, 32, L2Expanded, nullptr}; });
}
cuvsError_t cuvsHnswIndexParamsDestroy(cuvsHnswIndexParams_t params)
{
  return (cuvsError_t)translate_exceptions([=] { delete params; });
}
cuvsError_t cuvsHnswIndexCreate(cuvsHnswIndex_t* index)
{
  return (cuvsError_t)translate_exceptions([=] { *index = new cuvsHnswIndex{0, DLDataType{0, 0, 0}}; });
}
cuvsError_t cuvsHnswIndexDestroy(cuvsHnswIndex_t index)
{
  return (cuvsError_t)translate_exceptions([=] {
    if (!index) return;
    delete reinterpret_cast<hh::index*>(index->addr);
    delete index;
  });
}
cuvsError_t cuvsHnswExtendParamsCreate(cuvsHnswExtendParams_t* params)
{
  return (cuvsError_t)translate_exceptions([=] { *params = new cuvsHnswExtendParams{0}; });
}
cuvsError_t cuvsHnswExtendParamsDestroy(cuvsHnswExtendParams_t params)
{
  return (cuvsError_t)translate_exceptions([=] { delete params; });
}
cuvsError_t cuvsHnswSearchParamsCreate(cuvsHnswSearchParams_t* params)
{
  return (cuvsError_t)translate_exceptions([=] { *params = new cuvsHnswSearchParams{200, 0}; });
}
cuvsError_t cuvsHnswSearchParamsDestroy(cuvsHnswSearchParams_t params)
{
  return (cuvsError_t)translate_exceptions([=] { delete params; });
}

cuvsError_t cuvsHnswFromCagra(cuvsResources_t res, cuvsHnswIndexParams_t params, cuvsCagraIndex_t cagra_index,
                              cuvsHnswIndex_t hnsw_index)
{
  return (cuvsError_t)translate_exceptions([=] { from_cagra(res, params, cagra_index, hnsw_index, nullptr, false); });
}
cuvsError_t cuvsHnswFromCagraWithDataset(cuvsResources_t res, cuvsHnswIndexParams_t params, cuvsCagraIndex_t cagra_index,
                                         cuvsHnswIndex_t hnsw_index, DLManagedTensor* dataset_tensor)
{
  return (cuvsError_t)translate_exceptions([=] { from_cagra(res, params, cagra_index, hnsw_index, dataset_tensor, true); });
}

cuvsError_t cuvsHnswBuild(cuvsResources_t res, cuvsHnswIndexParams_t params, DLManagedTensor* dataset, cuvsHnswIndex_t index)
{
  return (cuvsError_t)translate_exceptions([=] {
    CUVS_EXPECTS(params && dataset && index, "null argument");
    CUVS_EXPECTS(params->ace_params != nullptr, "ACE parameters must be set for hnsw::build");
    check_metric((int)params->metric);
    (void)check_hierarchy((int)params->hierarchy);
    (void)elem_of(dataset->dl_tensor.dtype);
    CUVS_EXPECTS(params->M >= 1 && params->M <= 128, "hnsw::build: M must be in 1..128 (got %zu)", params->M);
    // the partitioning fields of the ACE parameters are a memory strategy and stay unused (as cuvsCagraBuild treats ACE)
    cagra_handles h;
    expect_ok(cuvsCagraIndexParamsCreate(&h.params), "cuvsCagraIndexParamsCreate");
    h.params->metric                    = params->metric;
    h.params->graph_degree              = 2 * params->M;
    h.params->intermediate_graph_degree = 3 * params->M;
    expect_ok(cuvsCagraIndexCreate(&h.index), "cuvsCagraIndexCreate");
    expect_ok(cuvsCagraBuild(res, h.params, dataset, h.index), "cuvsCagraBuild");
    from_cagra(res, params, h.index, index, nullptr, false);
    if (params->ace_params->use_disk) {
      const std::string dir = params->ace_params->build_dir ? params->ace_params->build_dir : "/tmp/hnsw_ace_build";
      make_dirs(dir);
      hh::save(get_hnsw(index), (dir + "/hnsw_index.bin").c_str());
    }
  });
}

cuvsError_t cuvsHnswExtend(cuvsResources_t, cuvsHnswExtendParams_t params, DLManagedTensor* additional_dataset, cuvsHnswIndex_t index)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& ix = get_hnsw(index);
    CUVS_EXPECTS(params && additional_dataset, "null argument");
    auto& t = additional_dataset->dl_tensor;
    CUVS_EXPECTS(is_host_accessible(t), "additional_dataset should have host compatible memory");
    CUVS_EXPECTS(t.ndim == 2 && is_c_contiguous(t) && (size_t)t.shape[1] == ix.dim, "additional_dataset must be [m, dim] row-major");
    CUVS_EXPECTS((int)elem_of(t.dtype) == ix.dtype, "additional_dataset dtype differs from the index dtype");
    hh::extend(ix, dl_data(t), (size_t)t.shape[0]);  // params->num_threads: accepted, unused (the insert is sequential)
  });
}

cuvsError_t cuvsHnswSearch(cuvsResources_t, cuvsHnswSearchParams_t params, cuvsHnswIndex_t index_c, DLManagedTensor* queries_tensor,
                           DLManagedTensor* neighbors_tensor, DLManagedTensor* distances_tensor)
{
  return (cuvsError_t)translate_exceptions([=] {
    CUVS_EXPECTS(params && queries_tensor && neighbors_tensor && distances_tensor, "null argument");
    auto& queries   = queries_tensor->dl_tensor;
    auto& neighbors = neighbors_tensor->dl_tensor;
    auto& distances = distances_tensor->dl_tensor;
    CUVS_EXPECTS(is_host_accessible(queries), "queries should have host compatible memory");
    CUVS_EXPECTS(is_host_accessible(neighbors), "neighbors should have host compatible memory");
    CUVS_EXPECTS(is_host_accessible(distances), "distances should have host compatible memory");
    CUVS_EXPECTS(dtype_is(neighbors.dtype, kDLUInt, 64), "neighbors should be of type uint64_t");
    CUVS_EXPECTS(dtype_is(distances.dtype, kDLFloat, 32), "distances should be of type float32");
    auto& ix = get_hnsw(index_c);
    CUVS_EXPECTS(queries.dtype.code == index_c->dtype.code && queries.dtype.bits == index_c->dtype.bits,
                 "type mismatch between index and queries");
    CUVS_EXPECTS(queries.ndim == 2 && neighbors.ndim == 2 && distances.ndim == 2, "tensors must be 2-D");
    CUVS_EXPECTS(is_c_contiguous(queries) && is_c_contiguous(neighbors) && is_c_contiguous(distances), "tensors must be C-contiguous");
    CUVS_EXPECTS((size_t)queries.shape[1] == ix.dim, "queries dim mismatch");
    const int64_t m = queries.shape[0], k = neighbors.shape[1];
    CUVS_EXPECTS(neighbors.shape[0] == m && distances.shape[0] == m && distances.shape[1] == k, "neighbors/distances shape mismatch");
    CUVS_EXPECTS(params->ef > 0, "ef must be positive (got %d)", (int)params->ef);
    hh::search(ix, dl_data(queries), (size_t)m, (size_t)k, (size_t)params->ef, params->num_threads,
               static_cast<uint64_t*>(dl_data(neighbors)), static_cast<float*>(dl_data(distances)));
  });
}

cuvsError_t cuvsHnswSerialize(cuvsResources_t, const char* filename, cuvsHnswIndex_t index)
{
  return (cuvsError_t)translate_exceptions([=] { hh::save(get_hnsw(index), filename); });
}

cuvsError_t cuvsHnswDeserialize(cuvsResources_t, cuvsHnswIndexParams_t params, const char* filename, int dim, cuvsDistanceType metric,
                                cuvsHnswIndex_t index)
{
  return (cuvsError_t)translate_exceptions([=] {
    CUVS_EXPECTS(params && index, "null argument");
    const DLDataType dt = index->dtype;
    CUVS_EXPECTS(dtype_is(dt, kDLFloat, 32) || dtype_is(dt, kDLFloat, 16) || dtype_is(dt, kDLInt, 8) || dtype_is(dt, kDLUInt, 8),
                 "Unsupported dtype in file %s", filename ? filename : "(null)");
    check_metric((int)metric);
    set_hnsw(index, hh::load(filename, dim, (int)metric, (int)elem_of(dt), check_hierarchy((int)params->hierarchy)), dt);
  });
}

}  // extern "C"
