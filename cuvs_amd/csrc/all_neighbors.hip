// All-neighbours kNN graph build (cuvsAllNeighbors*): the dataset against itself, either in one piece or - for a host
// dataset - cluster by cluster with every row in `overlap_factor` clusters, the local graphs merged into the global
// [n, k] graph on the device. A restatement of cpp/src/neighbors/all_neighbors/{all_neighbors,all_neighbors_batched,
// all_neighbors_builder,all_neighbors_merge}.cuh and c/src/neighbors/all_neighbors.cpp; DESIGN.md 3.1m.
//
// The local builders are the library's own: brute force (cuvsBruteForce*), NN-descent (knn_graph_nn_descent) and
// IVF-PQ + refine. A distance here is one k-ordered fp32 fma chain per pair over canonical norms, so a pair has the same
// bits in whichever cluster it is computed: the merge removes duplicates EXACTLY (the reference looks through a 4-wide
// window because its GEMM distances move with the matrix shape, all_neighbors_merge.cuh:113-119) and never leaves the
// device (the reference remaps ids on the host and keeps the global matrices in managed memory).
#include "ops.hpp"
#include "device_utils.hpp"
#include "ivf_pq.hpp"

#include <cuvs/neighbors/all_neighbors.h>
#include <cuvs/neighbors/brute_force.h>
#include <cuvs_amd/extensions.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <thread>
#include <vector>

namespace cuvs_amd {
namespace {

constexpr uint32_t kAnPadKey   = 0xffffffffu;  // sorts behind every distance key
constexpr int kAnMaxK          = 1024;         // the reference's merge limit (all_neighbors_merge.cuh)
constexpr int kAnWaveMaxP      = 128;          // 2k padded to a power of two: one wave per row up to here
constexpr int kAnGatherThreads = 16;           // host workers of the row gather (a fixed bound, not the machine's core count)

// ------------------------------------------------------------------ remap + merge
template <bool kWaveOnly>
__device__ inline void an_sync()
{
  if constexpr (kWaveOnly) {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  } else {
    __syncthreads();
  }
}

// bitonic sort of P (power of two) entries in LDS, ascending by (id, key): equal ids become neighbours, the best first
template <bool kWaveOnly>
__device__ inline void an_sort_by_id(uint32_t* keys, int64_t* ids, int P, int tid, int nthr)
{
  for (int size = 2; size <= P; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      an_sync<kWaveOnly>();
      for (int t = tid; t < (P >> 1); t += nthr) {
        const int lo = 2 * t - (t & (stride - 1));
        const int hi = lo + stride;
        const bool up = (lo & size) == 0;
        const uint32_t ka = keys[lo], kb = keys[hi];
        const int64_t ia = ids[lo], ib = ids[hi];
        const bool a_gt_b = ia > ib || (ia == ib && ka > kb);
        if (a_gt_b == up) {
          keys[lo] = kb; keys[hi] = ka;
          ids[lo] = ib; ids[hi] = ia;
        }
      }
    }
  }
  an_sync<kWaveOnly>();
}

// One cluster's local graph into the global one. Per cluster row b: g = inv[b]; the k entries of global[g] and the k
// entries of batch[b] - local ids mapped through inv[] here - are ordered by (distance, id) (inner product: (-distance,
// id)), entries whose id appeared earlier in that order are dropped, the first k survivors go back to global[g] and the
// slots that remain hold the fill values. Two sorts: by (id, key) to find every id's best entry, then by (key, id).
// kWaveOnly: a wave per row (4 rows per workgroup), P <= 128; else a 256-thread workgroup per row, P <= 2048.
// A global row appears at most once in a cluster, so rows do not meet within a launch.
template <bool kWaveOnly>
__global__ __launch_bounds__(256) void an_remap_merge_kernel(const int64_t* __restrict__ inv, int64_t m,
                                                             const int64_t* __restrict__ batch_i,
                                                             const float* __restrict__ batch_d, int64_t* __restrict__ glob_i,
                                                             float* __restrict__ glob_d, int64_t n, int k, int P,
                                                             bool select_min, int64_t b0)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char an_smem[];
  constexpr int nthr  = kWaveOnly ? 64 : 256;
  constexpr int slots = kWaveOnly ? 4 : 1;
  const int tid       = kWaveOnly ? (int)(threadIdx.x & 63) : (int)threadIdx.x;
  const int slot      = kWaveOnly ? (int)(threadIdx.x >> 6) : 0;
  const int64_t b     = b0 + (kWaveOnly ? (int64_t)blockIdx.x * 4 + slot : (int64_t)blockIdx.x);
  if (b >= m) return;  // uniform over the wave (wave per row) or the workgroup
  const int64_t g = inv[b];
  if (g < 0 || g >= n) return;  // never written out of bounds, whatever the inverted list holds
  int64_t* ids   = reinterpret_cast<int64_t*>(an_smem) + (size_t)slot * P;
  uint32_t* keys = reinterpret_cast<uint32_t*>(an_smem + (size_t)slots * P * sizeof(int64_t)) + (size_t)slot * P;
  for (int j = tid; j < P; j += nthr) {
    uint32_t key = kAnPadKey;
    int64_t id   = INT64_MAX;
    if (j < k) {
      id            = glob_i[g * k + j];
      const float d = glob_d[g * k + j];
      key           = float_to_key(select_min ? d : -d);
    } else if (j < 2 * k) {
      const int64_t l = batch_i[b * k + (j - k)];
      if (l >= 0 && l < m) {  // (a local builder's "none" entries stay padding)
        id            = inv[l];
        const float d = batch_d[b * k + (j - k)];
        key           = float_to_key(select_min ? d : -d);
      }
    }
    ids[j]  = id;
    keys[j] = key;
  }
  an_sort_by_id<kWaveOnly>(keys, ids, P, tid, nthr);
  uint32_t drop = 0;  // P / nthr <= 8 entries per thread
  for (int c = 0, j = tid; j < P; j += nthr, ++c)
    if (j > 0 && ids[j] == ids[j - 1]) drop |= 1u << c;
  an_sync<kWaveOnly>();
  for (int c = 0, j = tid; j < P; j += nthr, ++c)
    if ((drop >> c) & 1u) { keys[j] = kAnPadKey; ids[j] = INT64_MAX; }
  if constexpr (kWaveOnly) {
    wave_bitonic_sort<int64_t>(keys, ids, P);
  } else {
    block_bitonic_sort<int64_t>(keys, ids, P);
  }
  for (int j = tid; j < k; j += nthr) {
    const uint32_t key = keys[j];
    if (key == kAnPadKey) {
      glob_i[g * k + j] = select_min ? INT64_MAX : INT64_MIN;
      glob_d[g * k + j] = select_min ? FLT_MAX : -FLT_MAX;
    } else {
      const float v     = key_to_float(key);
      glob_i[g * k + j] = ids[j];
      glob_d[g * k + j] = select_min ? v : -v;
    }
  }
}

void an_launch_merge(resources& res, const int64_t* inv, int64_t m, const int64_t* batch_i, const float* batch_d,
                     int64_t* glob_i, float* glob_d, int64_t n, int k, bool select_min)
{
  if (m == 0) return;
  CUVS_EXPECTS(k >= 1 && k <= kAnMaxK, "all_neighbors: the merge takes 1 <= k <= %d (k = %d)", kAnMaxK, k);
  const int P        = next_pow2(2 * k);
  const int64_t slab = int64_t(1) << 22;  // cluster rows per launch (the 2^32-thread grid limit)
  for (int64_t b0 = 0; b0 < m; b0 += slab) {
    const int64_t rows = std::min(slab, m - b0);
    if (P <= kAnWaveMaxP) {
      hipLaunchKernelGGL(an_remap_merge_kernel<true>, dim3(grid_blocks(rows, 4)), dim3(256), (size_t)4 * P * 12, res.stream, inv, m,
                         batch_i, batch_d, glob_i, glob_d, n, k, P, select_min, b0);
    } else {
      hipLaunchKernelGGL(an_remap_merge_kernel<false>, dim3(grid_blocks(rows, 1)), dim3(256), (size_t)P * 12, res.stream, inv, m,
                         batch_i, batch_d, glob_i, glob_d, n, k, P, select_min, b0);
    }
  }
  HIP_TRY(hipGetLastError());
}

// ------------------------------------------------------------------ small kernels
// mutual reachability, in place over a distance tile (rows r0.., all of the tile's columns c0..):
// d' = max(core[col], max(core[row], alpha * d))  (reachability ReachabilityPostProcess)
__global__ void an_reach_epilogue_kernel(float* __restrict__ d, int64_t m, int64_t n_tile, int64_t ldo,
                                         const float* __restrict__ core_rows, const float* __restrict__ core_cols, float alpha)
{
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n_tile) return;
  const float cc = core_cols[c];
  for (int64_t r = blockIdx.y; r < m; r += gridDim.y) {
    const float v  = alpha * d[r * ldo + c];
    d[r * ldo + c] = fmaxf(cc, fmaxf(core_rows[r], v));
  }
}

__global__ void an_gather_core_kernel(const float* __restrict__ core, const int64_t* __restrict__ inv, int64_t m,
                                      float* __restrict__ out)
{
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b < m) out[b] = core[inv[b]];
}

__global__ void an_fill_kernel(int64_t* __restrict__ ids, float* __restrict__ d, int64_t total, int64_t id, float v)
{
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    ids[i] = id;
    d[i]   = v;
  }
}

// rows one column to the right, the last column dropped; column 0 = (row id, first[row] or 0) (raft::matrix::shift)
__global__ void an_shift_kernel(int64_t* __restrict__ ids, float* __restrict__ d, int64_t n, int k,
                                const float* __restrict__ first)
{
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  for (int j = k - 1; j > 0; --j) {
    ids[r * k + j] = ids[r * k + j - 1];
    if (d != nullptr) d[r * k + j] = d[r * k + j - 1];
  }
  ids[r * k] = r;
  if (d != nullptr) d[r * k] = first != nullptr ? first[r] : 0.0f;
}

__global__ void an_last_column_kernel(const float* __restrict__ d, int64_t n, int k, float* __restrict__ core)
{
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r < n) core[r] = d[r * k + k - 1];
}

// NN-descent's uint32 graph + order-preserving keys -> the first k columns as int64 ids + distances
__global__ void an_nnd_emit_kernel(const uint32_t* __restrict__ ids, const uint32_t* __restrict__ keys, int64_t m, uint32_t K,
                                   int k, int metric, int64_t* __restrict__ out_i, float* __restrict__ out_d)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m * k) return;
  const int64_t r = i / k, c = i % k;
  const uint32_t id = ids[r * K + c];
  const bool ip     = metric == M_InnerProduct;
  if (id == 0xffffffffu) {
    out_i[i] = ip ? INT64_MIN : INT64_MAX;
    out_d[i] = ip ? -FLT_MAX : FLT_MAX;
    return;
  }
  float v = key_to_float(keys[r * K + c]);
  if (ip) v = -v;
  if (metric == M_L2SqrtExpanded || metric == M_L2SqrtUnexpanded) v = sqrtf(v);
  out_i[i] = (int64_t)id;
  out_d[i] = v;
}

// ------------------------------------------------------------------ host-side helpers
struct dl_view {  // a non-owning DLManagedTensor of a device matrix, for the library's own C entry points
  DLManagedTensor t;
  int64_t shape[2];
  dl_view(void* data, DLDataType dt, int64_t rows, int64_t cols, int device)
  {
    shape[0] = rows; shape[1] = cols;
    t.dl_tensor.data        = data;
    t.dl_tensor.device      = DLDevice{kDLCUDA, device};
    t.dl_tensor.ndim        = 2;
    t.dl_tensor.dtype       = dt;
    t.dl_tensor.shape       = shape;
    t.dl_tensor.strides     = nullptr;
    t.dl_tensor.byte_offset = 0;
    t.manager_ctx           = nullptr;
    t.deleter               = nullptr;
  }
};

void an_check(cuvsError_t st)
{
  if (st != CUVS_SUCCESS) throw error(last_error_text());
}

struct pinned_buf {
  float* p = nullptr;
  explicit pinned_buf(size_t floats) { HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&p), std::max<size_t>(floats, 1) * sizeof(float))); }
  pinned_buf(const pinned_buf&)            = delete;
  pinned_buf& operator=(const pinned_buf&) = delete;
  ~pinned_buf() { (void)hipHostFree(p); }
};

// dst[i] = data[rows[i]] by at most kAnGatherThreads workers; join() before dst is read
struct row_gather {
  std::vector<std::thread> pool;
  void start(const float* data, int64_t dim, const int64_t* rows, int64_t m, float* dst)
  {
    join();
    const int nt = (int)std::max<int64_t>(1, std::min<int64_t>(kAnGatherThreads, m / 2048));
    for (int t = 0; t < nt; ++t) {
      const int64_t b0 = m * t / nt, b1 = m * (t + 1) / nt;
      pool.emplace_back([=] {
        for (int64_t b = b0; b < b1; ++b) memcpy(dst + b * dim, data + rows[b] * dim, (size_t)dim * sizeof(float));
      });
    }
  }
  void join()
  {
    for (auto& th : pool) th.join();
    pool.clear();
  }
  ~row_gather() { join(); }
};

struct event_pair {
  hipEvent_t e[2] = {nullptr, nullptr};
  event_pair() { for (auto& x : e) HIP_TRY(hipEventCreateWithFlags(&x, hipEventDisableTiming)); }
  event_pair(const event_pair&)            = delete;
  event_pair& operator=(const event_pair&) = delete;
  ~event_pair() { for (auto x : e) if (x) (void)hipEventDestroy(x); }
};

uint64_t an_splitmix(uint64_t x)
{
  x += 0x9e3779b97f4a7c15ull;
  x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
  x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
  return x ^ (x >> 31);
}

// ------------------------------------------------------------------ partition (all_neighbors_batched.cuh:60-269)
struct an_partition {
  int64_t n = 0;
  int n_clusters = 0, overlap = 0;
  std::vector<int64_t> nearest;  // [n, overlap]
  std::vector<int64_t> inv;      // [n * overlap]: row ids of cluster 0 ascending, then cluster 1, ...
  std::vector<int64_t> sizes, offsets;
};

// centroids: balanced k-means on a fixed-seed stratified row sample (one row out of each of `ns` equal strides);
// assignment: every row to its `overlap` nearest centroids under the build's metric, exact top-k with the (value, index)
// tie rule, in row batches of ceil(n / n_clusters)
void an_make_partition(resources& res, const float* data, int64_t n, int64_t dim, int n_clusters, int overlap, int metric,
                       an_partition& part, dev_buf<float>& centroids)
{
  CUVS_EXPECTS(n >= n_clusters, "all_neighbors: n_clusters (%d) exceeds the number of rows (%ld)", n_clusters, (long)n);
  part.n = n; part.n_clusters = n_clusters; part.overlap = overlap;
  int64_t ns = std::min<int64_t>(n / n_clusters, 50000);
  if (ns <= 1000) ns = std::min<int64_t>(n, 5000);  // (k-means on fewer rows does not work well, :78-81)
  {
    std::vector<int64_t> rows((size_t)ns);
    for (int64_t j = 0; j < ns; ++j) {
      const int64_t lo = n * j / ns, hi = n * (j + 1) / ns;
      rows[(size_t)j]  = lo + (int64_t)(an_splitmix((uint64_t)j) % (uint64_t)(hi - lo));
    }
    pinned_buf sample((size_t)ns * dim);
    row_gather gather;
    gather.start(data, dim, rows.data(), ns, sample.p);
    gather.join();
    dev_buf<float> sample_d(res, (size_t)ns * dim);
    copy_async(res, sample_d.data(), sample.p, sample_d.bytes());
    centroids = dev_buf<float>(res, (size_t)n_clusters * dim);
    kmeans_params kp;
    kp.inner_product = metric == M_InnerProduct;
    kmeans_balanced_fit(res, sample_d.data(), ns, dim, n_clusters, kp, centroids.data());
    sync(res);  // the pinned sample goes away
  }
  const int64_t batch = (n + n_clusters - 1) / n_clusters;
  dev_buf<float> x(res, (size_t)batch * dim), tile(res, (size_t)batch * n_clusters), ov(res, (size_t)batch * overlap);
  dev_buf<int64_t> oi(res, (size_t)batch * overlap);
  dev_buf<float> qn, cn;
  if (metric != M_InnerProduct) {
    qn = dev_buf<float>(res, batch);
    cn = dev_buf<float>(res, n_clusters);
    row_norms<float>(res, centroids.data(), n_clusters, dim, dim, cn.data(), metric == M_CosineExpanded);
  }
  part.nearest.assign((size_t)n * overlap, 0);
  for (int64_t r0 = 0; r0 < n; r0 += batch) {
    const int64_t mr = std::min(batch, n - r0);
    copy_async(res, x.data(), data + r0 * dim, (size_t)mr * dim * sizeof(float));
    if (qn.data()) row_norms<float>(res, x.data(), mr, dim, dim, qn.data(), metric == M_CosineExpanded);
    pairwise_distance<float, float>(res, x.data(), mr, dim, centroids.data(), n_clusters, dim, dim, qn.data(), cn.data(), metric,
                                    tile.data(), n_clusters);
    select_k<int64_t, int64_t>(res, tile.data(), nullptr, mr, n_clusters, n_clusters, overlap, ov.data(), oi.data(),
                               metric != M_InnerProduct);
    copy_async(res, part.nearest.data() + r0 * overlap, oi.data(), (size_t)mr * overlap * sizeof(int64_t));
    sync(res);
  }
  // inverted lists (get_inverted_indices, :235-269): rows in ascending order within a cluster
  part.sizes.assign(n_clusters, 0);
  part.offsets.assign(n_clusters + 1, 0);
  for (int64_t c : part.nearest) {
    CUVS_EXPECTS(c >= 0 && c < n_clusters, "all_neighbors: cluster assignment out of range");
    part.sizes[(size_t)c] += 1;
  }
  for (int c = 0; c < n_clusters; ++c) part.offsets[c + 1] = part.offsets[c] + part.sizes[c];
  part.inv.assign((size_t)n * overlap, 0);
  std::vector<int64_t> fill(part.offsets.begin(), part.offsets.end() - 1);
  for (int64_t i = 0; i < n; ++i)
    for (int j = 0; j < overlap; ++j) part.inv[(size_t)fill[(size_t)part.nearest[(size_t)i * overlap + j]]++] = i;
}

// ------------------------------------------------------------------ local builders
struct an_ctx {
  uintptr_t res_h;
  resources& res;
  int algo, metric, k;
  cuvsIvfPqIndexParams_t pq;
  cuvsNNDescentIndexParams_t nnd;
  float alpha;
};

// exact kNN of the rows against themselves with the reachability epilogue between the distance tile and select_k
// (the tiled path of brute force: select per column tile, then one select over the partial results)
void an_brute_force_reach(an_ctx& c, const float* x, int64_t m, int64_t dim, const float* core, int64_t* out_i, float* out_d)
{
  resources& res = c.res;
  const int k    = c.k;
  dev_buf<float> norms(res, m);
  row_norms<float>(res, x, m, dim, dim, norms.data(), c.metric == M_CosineExpanded);
  const int64_t ws_floats = (int64_t)(res.workspace_limit / sizeof(float));
  const int64_t m_tile    = std::min<int64_t>(m, 4096);
  const int64_t n_tile    = std::min<int64_t>(m, std::max<int64_t>(128, (ws_floats / m_tile) / 128 * 128));
  const int64_t n_ct      = (m + n_tile - 1) / n_tile;
  dev_buf<float> tile(res, (size_t)m_tile * n_tile), part_v;
  dev_buf<int64_t> part_i;
  if (n_ct > 1) {
    part_v = dev_buf<float>(res, (size_t)m_tile * n_ct * k);
    part_i = dev_buf<int64_t>(res, (size_t)m_tile * n_ct * k);
  }
  for (int64_t r0 = 0; r0 < m; r0 += m_tile) {
    const int64_t mr = std::min(m_tile, m - r0);
    for (int64_t ct = 0; ct < n_ct; ++ct) {
      const int64_t c0 = ct * n_tile, nc = std::min(n_tile, m - c0);
      pairwise_distance<float, float>(res, x + r0 * dim, mr, dim, x + c0 * dim, nc, dim, dim, norms.data() + r0, norms.data() + c0,
                                      c.metric, tile.data(), n_tile);
      hipLaunchKernelGGL(an_reach_epilogue_kernel, dim3(grid_blocks(nc, 256), (unsigned)std::min<int64_t>(mr, 1024)), dim3(256), 0,
                         res.stream, tile.data(), mr, nc, n_tile, core + r0, core + c0, c.alpha);
      if (n_ct == 1) {
        select_k<int64_t, int64_t>(res, tile.data(), nullptr, mr, nc, n_tile, k, out_d + r0 * k, out_i + r0 * k, true, c0);
      } else {
        select_k<int64_t, int64_t>(res, tile.data(), nullptr, mr, nc, n_tile, k, part_v.data(), part_i.data(), true, c0, n_ct * k,
                                   ct * k);
      }
    }
    if (n_ct > 1)
      select_k<int64_t, int64_t>(res, part_v.data(), part_i.data(), mr, n_ct * k, n_ct * k, k, out_d + r0 * k, out_i + r0 * k, true);
  }
  HIP_TRY(hipGetLastError());
}

void an_brute_force(an_ctx& c, float* x, int64_t m, int64_t dim, const float* core, int64_t* out_i, float* out_d)
{
  if (core != nullptr) return an_brute_force_reach(c, x, m, dim, core, out_i, out_d);
  // the library's own brute force: build (norms) + search of the rows against themselves
  struct index_guard {
    cuvsBruteForceIndex_t p = nullptr;
    ~index_guard() { if (p) (void)cuvsBruteForceIndexDestroy(p); }
  } bi;
  an_check(cuvsBruteForceIndexCreate(&bi.p));
  const DLDataType f32{kDLFloat, 32, 1}, i64{kDLInt, 64, 1};
  dl_view dv(x, f32, m, dim, c.res.device), iv(out_i, i64, m, c.k, c.res.device), ov(out_d, f32, m, c.k, c.res.device);
  an_check(cuvsBruteForceBuild(c.res_h, &dv.t, (cuvsDistanceType)c.metric, 2.0f, bi.p));
  an_check(cuvsBruteForceSearch(c.res_h, bi.p, &dv.t, &iv.t, &ov.t, cuvsFilter{0, NO_FILTER}));
  sync(c.res);  // the index's norms go away with it
}

void an_nn_descent(an_ctx& c, const float* x, int64_t m, int64_t dim, int64_t* out_i, float* out_d)
{
  resources& res = c.res;
  // defaults of cuvsNNDescentIndexParamsCreate
  cuvsNNDescentIndexParams p{L2Expanded, 2.0f, 64, 128, 20, 0.0001f, true, NND_DIST_COMP_AUTO};
  if (c.nnd != nullptr) p = *c.nnd;
  const size_t degree = std::max<size_t>(p.graph_degree, (size_t)c.k);  // all_neighbors_builder.cuh:327-334
  uint32_t K          = (uint32_t)std::max(p.intermediate_graph_degree, degree);
  K                   = (uint32_t)std::min<int64_t>(K, m - 1);  // as cuvsNNDescentBuild
  CUVS_EXPECTS(m >= 2 && (uint32_t)c.k <= K, "all_neighbors: NN-descent needs more than k rows (k = %d, rows = %ld)", c.k, (long)m);
  dev_buf<float> norms;
  if (c.metric == M_CosineExpanded) {
    norms = dev_buf<float>(res, m);
    row_norms<float>(res, x, m, dim, dim, norms.data(), true);
  }
  dev_buf<uint32_t> ids(res, (size_t)m * K), keys(res, (size_t)m * K);
  knn_graph_nn_descent(res, x, elem_t::f32, m, dim, K, c.metric, norms.data(), (int)p.max_iterations, ids.data(), keys.data(),
                       p.termination_threshold > 0.f ? p.termination_threshold : 1e-4f);
  hipLaunchKernelGGL(an_nnd_emit_kernel, dim3(grid_blocks(m * (int64_t)c.k, 256)), dim3(256), 0, res.stream, ids.data(), keys.data(),
                     m, K, c.k, c.metric, out_i, out_d);
  HIP_TRY(hipGetLastError());
}

void an_ivf_pq(an_ctx& c, const float* x, int64_t m, int64_t dim, int64_t* out_i, float* out_d)
{
  resources& res = c.res;
  ivf_pq_build_params bp;
  ivf_pq_search_params sp;
  if (c.pq == nullptr) {  // the defaults of knn_graph_ivf_pq (cagra.hip)
    bp.metric                   = M_L2Expanded;
    bp.n_lists                  = (uint32_t)std::max<int64_t>(1, std::min<int64_t>(65536, (int64_t)std::sqrt((double)m)));
    bp.kmeans_n_iters           = 10;
    bp.kmeans_trainset_fraction = std::min(1.0, std::max(0.02, 2.0e6 / (double)m));
    bp.pq_bits                  = 8;
    bp.pq_dim                   = (uint32_t)std::max<int64_t>(8, std::min<int64_t>(64, round_up(dim / 2, 8)));
    sp.n_probes                 = std::max<uint32_t>(8, bp.n_lists / 50);
    sp.lut_dtype                = 2;
    sp.internal_distance_dtype  = 2;
    sp.max_internal_batch_size  = 16384;
  } else {
    const cuvsIvfPqIndexParams& p = *c.pq;
    bp.metric                       = M_L2Expanded;
    bp.n_lists                      = p.n_lists;
    bp.kmeans_n_iters               = p.kmeans_n_iters;
    bp.kmeans_trainset_fraction     = p.kmeans_trainset_fraction;
    bp.pq_bits                      = p.pq_bits;
    bp.pq_dim                       = p.pq_dim;
    bp.codebook_kind                = (int)p.codebook_kind;
    bp.force_random_rotation        = p.force_random_rotation;
    bp.max_train_points_per_pq_code = p.max_train_points_per_pq_code;
    bp.codes_layout                 = (int)p.codes_layout;
    // (search: the defaults of cuvsIvfPqSearchParamsCreate, as all_neighbors_builder.cuh:188 passes default search params)
  }
  bp.n_lists  = (uint32_t)std::max<int64_t>(1, std::min<int64_t>(bp.n_lists, m));
  sp.n_probes = std::min(sp.n_probes, bp.n_lists);
  auto idx    = ivf_pq_build(res, bp, x, elem_t::f32, m, dim, false);
  // all_neighbors_builder.cuh:130-132 with refinement_rate 2
  const int cand_k = (int)std::min<int64_t>(std::max<int64_t>((int64_t)c.k * 2, c.k), m);
  CUVS_EXPECTS(c.k <= cand_k, "all_neighbors: IVF-PQ needs at least k rows (k = %d, rows = %ld)", c.k, (long)m);
  const int64_t b = 16384;
  dev_buf<int64_t> cand(res, (size_t)std::min(b, m) * cand_k);
  dev_buf<float> cd(res, (size_t)std::min(b, m) * cand_k);
  for (int64_t r0 = 0; r0 < m; r0 += b) {
    const int64_t mr = std::min(b, m - r0);
    ivf_pq_search(res, sp, *idx, x + r0 * dim, elem_t::f32, mr, cand_k, cand.data(), cd.data());
    refine(res, x, elem_t::f32, m, dim, x + r0 * dim, mr, cand.data(), cand_k, c.k, c.metric, out_i + r0 * c.k, out_d + r0 * c.k);
  }
  sync(res);  // the index goes away
}

// kNN graph of device rows x [m, dim] against themselves -> out_i / out_d [m, k]; core: the rows' core distances (second,
// mutual-reachability pass; brute force only) or nullptr
void an_local_build(an_ctx& c, float* x, int64_t m, int64_t dim, const float* core, int64_t* out_i, float* out_d)
{
  switch (c.algo) {
    case CUVS_ALL_NEIGHBORS_ALGO_BRUTE_FORCE: an_brute_force(c, x, m, dim, core, out_i, out_d); break;
    case CUVS_ALL_NEIGHBORS_ALGO_NN_DESCENT: an_nn_descent(c, x, m, dim, out_i, out_d); break;
    case CUVS_ALL_NEIGHBORS_ALGO_IVF_PQ: an_ivf_pq(c, x, m, dim, out_i, out_d); break;
    default: CUVS_FAIL("Invalid all-neighbors build algo %d", c.algo);
  }
}

// ------------------------------------------------------------------ batched build (single_gpu_batch_build, :289-336)
// Cluster c + 1 is gathered into the second pinned buffer by host threads while cluster c runs on the device; what is
// computed does not depend on that overlap (the device work of the clusters is serialised on the stream).
void an_batch_pass(an_ctx& c, const float* data, int64_t n, int64_t dim, const an_partition& part, const int64_t* inv_d,
                   int64_t* glob_i, float* glob_d, const float* core)
{
  resources& res        = c.res;
  const int k           = c.k;
  const bool select_min = c.metric != M_InnerProduct;
  // The reference pre-fills inner-product distances with numeric_limits<float>::min() (all_neighbors_batched.cuh), the
  // smallest POSITIVE float, which outranks every negative product; the worst value of a maximising metric is -FLT_MAX.
  hipLaunchKernelGGL(an_fill_kernel, dim3((unsigned)std::min<int64_t>((n * k + 255) / 256, 1 << 16)), dim3(256), 0, res.stream, glob_i,
                     glob_d, n * k, select_min ? INT64_MAX : INT64_MIN, select_min ? FLT_MAX : -FLT_MAX);
  std::vector<int> active;
  int64_t max_m = 0;
  for (int cl = 0; cl < part.n_clusters; ++cl) {
    const int64_t m = part.sizes[cl];
    // a cluster with fewer than k rows is skipped (:311-315); NN-descent lists exclude the row itself, so it needs k + 1
    if (m < k || (c.algo == CUVS_ALL_NEIGHBORS_ALGO_NN_DESCENT && m <= k)) continue;
    active.push_back(cl);
    max_m = std::max(max_m, m);
  }
  if (active.empty()) return;
  pinned_buf stage0((size_t)max_m * dim), stage1((size_t)max_m * dim);
  float* stage[2] = {stage0.p, stage1.p};
  event_pair copied;
  dev_buf<float> x(res, (size_t)max_m * dim), batch_d(res, (size_t)max_m * k), core_local;
  dev_buf<int64_t> batch_i(res, (size_t)max_m * k);
  if (core != nullptr) core_local = dev_buf<float>(res, max_m);
  row_gather gather;
  auto start_gather = [&](size_t a) {
    const int cl = active[a];
    gather.start(data, dim, part.inv.data() + part.offsets[cl], part.sizes[cl], stage[a & 1]);
  };
  start_gather(0);
  for (size_t a = 0; a < active.size(); ++a) {
    const int cl         = active[a];
    const int64_t m      = part.sizes[cl];
    const int64_t* inv_c = inv_d + part.offsets[cl];
    gather.join();
    copy_async(res, x.data(), stage[a & 1], (size_t)m * dim * sizeof(float));
    HIP_TRY(hipEventRecord(copied.e[a & 1], res.stream));
    if (a + 1 < active.size()) {
      if (a >= 1) HIP_TRY(hipEventSynchronize(copied.e[(a + 1) & 1]));  // cluster a - 1 has left that staging buffer
      start_gather(a + 1);
    }
    if (core != nullptr)
      hipLaunchKernelGGL(an_gather_core_kernel, dim3(grid_blocks(m, 256)), dim3(256), 0, res.stream, core, inv_c, m,
                         core_local.data());
    an_local_build(c, x.data(), m, dim, core_local.data(), batch_i.data(), batch_d.data());
    an_launch_merge(res, inv_c, m, batch_i.data(), batch_d.data(), glob_i, glob_d, n, k, select_min);
  }
  sync(res);  // the staging buffers go away
}

const char* an_metric_refusal = "Distance metric for all-neighbors build with brute force should be L2Expanded, L2SqrtExpanded, "
                                "CosineExpanded, L2Unexpanded, L2SqrtUnexpanded or InnerProduct (metric %d is not built here)";

// check_params_validity (all_neighbors.cuh:20-79) + the argument checks of build()
void an_validate(const cuvsAllNeighborsIndexParams& p, bool has_dist, bool has_core, bool device_dataset, int64_t k)
{
  const int metric = (int)p.metric;
  const bool mrd_ok = metric == M_L2Expanded || metric == M_L2SqrtExpanded || metric == M_CosineExpanded;
  switch (p.algo) {
    case CUVS_ALL_NEIGHBORS_ALGO_BRUTE_FORCE:
      CUVS_EXPECTS(metric_supported(metric), an_metric_refusal, metric);
      CUVS_EXPECTS(!has_core || mrd_ok,
                   "Distance metric for all-neighbors build with brute force for computing mutual reachability distance should be "
                   "L2Expanded, L2SqrtExpanded, or CosineExpanded.");
      break;
    case CUVS_ALL_NEIGHBORS_ALGO_NN_DESCENT:
      CUVS_EXPECTS(metric == M_L2Expanded || metric == M_L2SqrtExpanded || metric == M_CosineExpanded || metric == M_InnerProduct,
                   "Distance metric for all-neighbors build with NN Descent should be L2Expanded, L2SqrtExpanded, CosineExpanded, "
                   "or InnerProduct.");
      CUVS_EXPECTS(!has_core,
                   "mutual reachability distance with NN Descent is not supported: it needs the reachability epilogue inside the "
                   "NN-descent kernels (use brute force for core_distances)");
      break;
    case CUVS_ALL_NEIGHBORS_ALGO_IVF_PQ:
      CUVS_EXPECTS(metric == M_L2Expanded, "Distance metric for all-neighbors build with IVFPQ should be L2Expanded");
      CUVS_EXPECTS(!has_core, "mutual reachability distance cannot be calculated using IVFPQ");
      break;
    default: CUVS_FAIL("Invalid all-neighbors build algo %d", (int)p.algo);
  }
  CUVS_EXPECTS(!has_core || has_dist, "distances matrix should be allocated to get mutual reachability distance.");
  CUVS_EXPECTS(p.n_clusters >= 1, "all_neighbors: n_clusters must be at least 1");
  if (p.n_clusters > 1) {
    CUVS_EXPECTS(!device_dataset,
                 "Batched all-neighbors build is not supported with data on device. Put data on host for batch build.");
    CUVS_EXPECTS(p.overlap_factor >= 1 && p.overlap_factor < p.n_clusters,
                 "overlap_factor should be smaller than n_clusters. We recommend starting from overlap_factor=2 and gradually "
                 "increasing it for better knn graph recall.");
    CUVS_EXPECTS(k <= kAnMaxK, "all_neighbors: a batched build takes k <= %d (k = %ld)", kAnMaxK, (long)k);
  }
}

}  // namespace
}  // namespace cuvs_amd

using namespace cuvs_amd;

extern "C" {

cuvsError_t cuvsAllNeighborsIndexParamsCreate(cuvsAllNeighborsIndexParams_t* index_params)
{
  return (cuvsError_t)translate_exceptions([=] {
    CUVS_EXPECTS(index_params != nullptr, "index_params is null");
    // c/src/neighbors/all_neighbors.cpp:214-227
    *index_params = new cuvsAllNeighborsIndexParams{CUVS_ALL_NEIGHBORS_ALGO_BRUTE_FORCE, 1, 1, L2Expanded, nullptr, nullptr};
  });
}

cuvsError_t cuvsAllNeighborsIndexParamsDestroy(cuvsAllNeighborsIndexParams_t index_params)
{
  return (cuvsError_t)translate_exceptions([=] {
    if (index_params == nullptr) return;
    if (index_params->ivf_pq_params != nullptr) an_check(cuvsIvfPqIndexParamsDestroy(index_params->ivf_pq_params));
    if (index_params->nn_descent_params != nullptr) an_check(cuvsNNDescentIndexParamsDestroy(index_params->nn_descent_params));
    delete index_params;
  });
}

cuvsError_t cuvsAllNeighborsBuild(cuvsResources_t res_h, cuvsAllNeighborsIndexParams_t params, DLManagedTensor* dataset_tensor,
                                  DLManagedTensor* indices_tensor, DLManagedTensor* distances_tensor,
                                  DLManagedTensor* core_tensor, float alpha)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& res = *as_res(res_h);
    CUVS_EXPECTS(params != nullptr && dataset_tensor != nullptr && indices_tensor != nullptr,
                 "cuvsAllNeighborsBuild: params, dataset and indices must not be null");
    CUVS_EXPECTS(res.mg_devices.size() <= 1, "cuvsAllNeighborsBuild: multi-GPU resources handles are not supported");
    auto& ds = dataset_tensor->dl_tensor;
    auto& it = indices_tensor->dl_tensor;
    CUVS_EXPECTS(ds.ndim == 2 && is_c_contiguous(ds), "dataset must be a row-major matrix");
    CUVS_EXPECTS(dtype_is(ds.dtype, kDLFloat, 32), "dataset must be float32 (Unsupported dataset DLtensor dtype: %d and bits: %d)",
                 (int)ds.dtype.code, (int)ds.dtype.bits);
    CUVS_EXPECTS(is_device_accessible(it), "indices should have device compatible memory");
    CUVS_EXPECTS(dtype_is(it.dtype, kDLInt, 64), "indices should be of type int64_t");
    CUVS_EXPECTS(it.ndim == 2 && is_c_contiguous(it), "indices must be a row-major matrix");
    const int64_t n = ds.shape[0], dim = ds.shape[1], k = it.shape[1];
    CUVS_EXPECTS(it.shape[0] == n, "number of rows in dataset should be the same as number of rows in indices matrix");
    CUVS_EXPECTS(n >= 1 && dim >= 1 && k >= 1 && k < (int64_t(1) << 30), "all_neighbors: empty dataset or k out of range");
    float* dist = nullptr;
    if (distances_tensor != nullptr) {
      auto& dt = distances_tensor->dl_tensor;
      CUVS_EXPECTS(is_device_accessible(dt), "distances should have device compatible memory");
      CUVS_EXPECTS(dtype_is(dt.dtype, kDLFloat, 32), "distances should be of type float32");
      CUVS_EXPECTS(dt.ndim == 2 && is_c_contiguous(dt) && dt.shape[0] == n && dt.shape[1] == k,
                   "indices matrix and distances matrix has to be the same shape.");
      dist = static_cast<float*>(dl_data(dt));
    }
    float* core = nullptr;
    if (core_tensor != nullptr) {
      auto& ct = core_tensor->dl_tensor;
      CUVS_EXPECTS(is_device_accessible(ct), "core_distances should have device compatible memory");
      CUVS_EXPECTS(dtype_is(ct.dtype, kDLFloat, 32), "core_distances should be of type float32");
      CUVS_EXPECTS(ct.ndim == 1 && ct.shape[0] == n && is_c_contiguous(ct), "core_distances must be a vector of one value per row");
      core = static_cast<float*>(dl_data(ct));
    }
    const bool on_device = is_device_accessible(ds);
    an_validate(*params, dist != nullptr, core != nullptr, on_device, k);

    int64_t* ids = static_cast<int64_t*>(dl_data(it));
    dev_buf<float> dist_tmp;
    if (dist == nullptr) {
      dist_tmp = dev_buf<float>(res, (size_t)n * k);
      dist     = dist_tmp.data();
    }
    an_ctx c{res_h, res, (int)params->algo, (int)params->metric, (int)k, params->ivf_pq_params, params->nn_descent_params, alpha};
    const bool batched = params->n_clusters > 1;
    const float* host  = static_cast<const float*>(dl_data(ds));
    an_partition part;  // computed once, used by both passes (the reference's BatchBuildAux)
    dev_buf<int64_t> inv_d;
    dev_buf<float> staged, centroids;
    float* x = nullptr;
    if (batched) {
      an_make_partition(res, host, n, dim, (int)params->n_clusters, (int)params->overlap_factor, c.metric, part, centroids);
      inv_d = dev_buf<int64_t>(res, part.inv.size());
      copy_async(res, inv_d.data(), part.inv.data(), inv_d.bytes());
    } else if (on_device) {
      x = static_cast<float*>(dl_data(ds));
    } else {
      staged = dev_buf<float>(res, (size_t)n * dim);
      copy_async(res, staged.data(), host, staged.bytes());
      x = staged.data();
    }
    auto pass = [&](const float* core_in) {
      if (batched) an_batch_pass(c, host, n, dim, part, inv_d.data(), ids, dist, core_in);
      else an_local_build(c, x, n, dim, core_in, ids, dist);
    };
    pass(nullptr);
    // NN-descent lists leave the row itself out: shifted to agree with brute force and IVF-PQ (all_neighbors.cuh:140-149)
    if (c.algo == CUVS_ALL_NEIGHBORS_ALGO_NN_DESCENT && c.metric != M_InnerProduct)
      hipLaunchKernelGGL(an_shift_kernel, dim3(grid_blocks(n, 256)), dim3(256), 0, res.stream, ids, dist, n, (int)k,
                         (const float*)nullptr);
    if (core != nullptr) {
      hipLaunchKernelGGL(an_last_column_kernel, dim3(grid_blocks(n, 256)), dim3(256), 0, res.stream, dist, n, (int)k, core);
      pass(core);
    }
    HIP_TRY(hipGetLastError());
    sync(res);  // scratch and staged rows go away
  });
}

// ---- test hooks (include/cuvs_amd/extensions.h)
cuvsError_t cuvsAmdAllNeighborsPartition(cuvsResources_t res_h, cuvsAllNeighborsIndexParams_t params,
                                         DLManagedTensor* dataset_host, DLManagedTensor* centroids_out,
                                         DLManagedTensor* nearest_clusters_out)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& res = *as_res(res_h);
    CUVS_EXPECTS(params && dataset_host && centroids_out && nearest_clusters_out, "null argument");
    auto& ds = dataset_host->dl_tensor;
    auto& ce = centroids_out->dl_tensor;
    auto& nc = nearest_clusters_out->dl_tensor;
    CUVS_EXPECTS(ds.ndim == 2 && is_c_contiguous(ds) && dtype_is(ds.dtype, kDLFloat, 32) && !is_device_accessible(ds),
                 "dataset must be a row-major float32 matrix on the host");
    const int64_t n = ds.shape[0], dim = ds.shape[1];
    CUVS_EXPECTS(params->n_clusters > 1 && params->overlap_factor >= 1 && params->overlap_factor < params->n_clusters,
                 "overlap_factor should be smaller than n_clusters.");
    CUVS_EXPECTS(metric_supported((int)params->metric), "all_neighbors: unsupported metric %d", (int)params->metric);
    CUVS_EXPECTS(ce.ndim == 2 && is_c_contiguous(ce) && dtype_is(ce.dtype, kDLFloat, 32) &&
                   ce.shape[0] == (int64_t)params->n_clusters && ce.shape[1] == dim,
                 "centroids_out must be float32 [n_clusters, dim]");
    CUVS_EXPECTS(nc.ndim == 2 && is_c_contiguous(nc) && dtype_is(nc.dtype, kDLInt, 64) && !is_device_accessible(nc) &&
                   nc.shape[0] == n && nc.shape[1] == (int64_t)params->overlap_factor,
                 "nearest_clusters_out must be int64 [n, overlap_factor] on the host");
    an_partition part;
    dev_buf<float> centroids;
    an_make_partition(res, static_cast<const float*>(dl_data(ds)), n, dim, (int)params->n_clusters, (int)params->overlap_factor,
                      (int)params->metric, part, centroids);
    copy_async(res, dl_data(ce), centroids.data(), centroids.bytes());
    sync(res);
    memcpy(dl_data(nc), part.nearest.data(), part.nearest.size() * sizeof(int64_t));
  });
}

cuvsError_t cuvsAmdAllNeighborsMerge(cuvsResources_t res_h, DLManagedTensor* inverted_indices, DLManagedTensor* batch_indices,
                                     DLManagedTensor* batch_distances, DLManagedTensor* global_indices,
                                     DLManagedTensor* global_distances, int select_min)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& res = *as_res(res_h);
    CUVS_EXPECTS(inverted_indices && batch_indices && batch_distances && global_indices && global_distances, "null argument");
    auto& iv = inverted_indices->dl_tensor;
    auto& bi = batch_indices->dl_tensor;
    auto& bd = batch_distances->dl_tensor;
    auto& gi = global_indices->dl_tensor;
    auto& gd = global_distances->dl_tensor;
    for (const DLTensor* t : {&iv, &bi, &bd, &gi, &gd})
      CUVS_EXPECTS(is_device_accessible(*t) && is_c_contiguous(*t), "all tensors must be C-contiguous device tensors");
    CUVS_EXPECTS(dtype_is(iv.dtype, kDLInt, 64) && dtype_is(bi.dtype, kDLInt, 64) && dtype_is(gi.dtype, kDLInt, 64),
                 "inverted_indices, batch_indices and global_indices must be int64");
    CUVS_EXPECTS(dtype_is(bd.dtype, kDLFloat, 32) && dtype_is(gd.dtype, kDLFloat, 32), "distances must be float32");
    CUVS_EXPECTS(iv.ndim == 1 && bi.ndim == 2 && bd.ndim == 2 && gi.ndim == 2 && gd.ndim == 2, "bad tensor rank");
    const int64_t m = iv.shape[0], k = bi.shape[1], n = gi.shape[0];
    CUVS_EXPECTS(bi.shape[0] == m && bd.shape[0] == m && bd.shape[1] == k && gi.shape[1] == k && gd.shape[0] == n && gd.shape[1] == k,
                 "shape mismatch between the batch and the global matrices");
    CUVS_EXPECTS(k >= 1 && k <= kAnMaxK, "all_neighbors: the merge takes 1 <= k <= %d (k = %ld)", kAnMaxK, (long)k);
    an_launch_merge(res, static_cast<const int64_t*>(dl_data(iv)), m, static_cast<const int64_t*>(dl_data(bi)),
                    static_cast<const float*>(dl_data(bd)), static_cast<int64_t*>(dl_data(gi)), static_cast<float*>(dl_data(gd)), n,
                    (int)k, select_min != 0);
  });
}

}  // extern "C"
