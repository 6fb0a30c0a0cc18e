// Tiered index (cuvsTieredIndex*): rows [0, ann_rows) behind an ANN index (CAGRA, IVF-Flat or IVF-PQ), rows
// [ann_rows, size) in an append-only brute-force tail, one search over both. A restatement of
// cpp/src/neighbors/detail/tiered_index.cuh and c/src/neighbors/tiered_index.cpp; DESIGN.md 3.1n.
//
// The ANN tiers are the library's own indexes, driven through their C entry points. The tail phase is the new work: the
// ANN result A is a bound the plain brute force does not have - a tail row matters only if it beats the query's k-th ANN
// value - so the tail is screened against that bound and the few survivors are merged with A by (distance, id):
//   composed   pairwise_threshold_append over the tail (thr = the bound, col_off = ann_rows, the bitset over global ids)
//              into a per-query buffer, then tiered_merge_kernel. Any batch size; the comparator of the kernel below.
//   fused      tiered_tail_kernel, one launch for up to 64 queries: the tail split over the compute units, the queries
//              staged once per workgroup, distances in the canonical chain (one ascending-k fp32 fma chain per pair, the
//              order of v_mfma_f32_16x16x4_f32 and of oracle.c canon_dot), screen + filter bit + append, and the last
//              workgroup to finish - an atomic ticket behind a __threadfence, nobody waits - merges and writes the result.
// A query whose buffer overflows (a poor A, a filter that emptied A, rows arriving in improving order) flags the batch, which
// is then redone exactly: brute force over the tail + tiered_merge_kernel. Correctness never depends on the cap.
#include "ops.hpp"
#include "device_utils.hpp"
#include "distance_tile.hpp"

#include <cuvs/neighbors/brute_force.h>
#include <cuvs/neighbors/tiered_index.h>
#include <cuvs_amd/extensions.h>

#include <algorithm>
#include <atomic>
#include <cfloat>
#include <memory>
#include <vector>

namespace cuvs_amd {
namespace {

constexpr uint32_t kTiPadKey = 0xffffffffu;  // sorts behind every distance key
constexpr int kTiCap         = 1024;         // appended tail candidates per query; more -> the exact redo
constexpr int kTiMaxK        = 1024;         // k of the threshold paths (k + cap entries are sorted in LDS)
constexpr int kTiMergeMaxP   = 4096;         // entries of one merge (k + kb padded to a power of two)
constexpr int kTiWaveMaxP    = 128;          // a wave per row up to here, a workgroup per row beyond
constexpr int kTiFusedMaxM   = 64;           // queries of one tiered_tail_kernel launch
constexpr int kTiQFloats     = 8192;         // LDS floats for the staged queries: m * round_up(dim, 16) <= this
constexpr int kTiRows        = 256;          // tail rows of a tile: one per thread
constexpr int kTiKC          = 16;           // k chunk of the staged tile
constexpr int kTiLdx         = kTiRows + 1;  // k-major pitch of the staged tile

std::atomic<unsigned long long> g_ti_composed{0}, g_ti_fused{0}, g_ti_redo{0};

// ------------------------------------------------------------------ storage and tiers
struct ti_storage {
  int64_t capacity = 0, dim = 0;
  dev_buf<float> data;   // [capacity, dim]
  dev_buf<float> norms;  // [capacity] canonical |x|^2 (L2) or |x| (cosine); empty for inner product
};

// The ANN tier: one of the library's indexes behind its C handle. Immutable once built, so indexes may share it (merge).
// `backing` keeps the allocation alive that a viewing tier (CAGRA built over device rows) points into.
struct ti_ann {
  int algo     = 0;
  int64_t rows = 0;
  cuvsCagraIndex_t cagra  = nullptr;
  cuvsIvfFlatIndex_t flat = nullptr;
  cuvsIvfPqIndex_t pq     = nullptr;
  std::shared_ptr<ti_storage> backing;
  ~ti_ann()
  {
    if (cagra) cuvsCagraIndexDestroy(cagra);
    if (flat) cuvsIvfFlatIndexDestroy(flat);
    if (pq) cuvsIvfPqIndexDestroy(pq);
  }
};

// build parameters, held by value (the caller's structs need not outlive the build)
struct ti_params {
  int metric                = M_L2Expanded;
  int algo                  = 0;
  int64_t min_ann_rows      = 100000;
  bool create_ann_on_extend = false;
  bool has_cagra = false, has_flat = false, has_pq = false;
  cuvsCagraIndexParams cagra{};  // (graph_build_params is not kept: the CAGRA build here reads none of it)
  cuvsIvfFlatIndexParams flat{};
  cuvsIvfPqIndexParams pq{};
};

struct tiered_index {
  ti_params p;
  int64_t dim = 0, size = 0;
  std::shared_ptr<ti_storage> st;
  std::shared_ptr<ti_ann> ann;
  int64_t ann_rows() const { return ann ? ann->rows : 0; }
};

inline bool ti_keeps_norms(int metric) { return metric != M_InnerProduct; }

void ti_call(cuvsError_t rc)
{
  if (rc != CUVS_SUCCESS) throw error(last_error_text());  // the upstream text, unchanged
}

ti_params ti_convert_params(const cuvsTieredIndexParams& c)
{
  ti_params p;
  p.metric               = (int)c.metric;
  p.algo                 = (int)c.algo;
  p.min_ann_rows         = c.min_ann_rows;
  p.create_ann_on_extend = c.create_ann_index_on_extend;
  CUVS_EXPECTS(p.algo == CUVS_TIERED_INDEX_ALGO_CAGRA || p.algo == CUVS_TIERED_INDEX_ALGO_IVF_FLAT ||
                 p.algo == CUVS_TIERED_INDEX_ALGO_IVF_PQ,
               "unsupported tiered index algorithm");
  // upstream parameters, when given, carry their own metric (c/src/neighbors/tiered_index.cpp:38-52: the upstream
  // conversion runs after the metric assignment)
  if (p.algo == CUVS_TIERED_INDEX_ALGO_CAGRA && c.cagra_params != nullptr) {
    p.has_cagra = true;
    p.cagra     = *c.cagra_params;
    p.metric    = (int)p.cagra.metric;
    CUVS_EXPECTS(p.cagra.compression == nullptr, "tiered_index: CAGRA compression parameters are not supported");
    CUVS_EXPECTS(p.cagra.build_algo != ACE, "tiered_index: the ACE graph build is not supported");
    p.cagra.graph_build_params = nullptr;  // the caller's struct need not outlive this call
  } else if (p.algo == CUVS_TIERED_INDEX_ALGO_IVF_FLAT && c.ivf_flat_params != nullptr) {
    p.has_flat = true;
    p.flat     = *c.ivf_flat_params;
    p.metric   = (int)p.flat.metric;
  } else if (p.algo == CUVS_TIERED_INDEX_ALGO_IVF_PQ && c.ivf_pq_params != nullptr) {
    p.has_pq = true;
    p.pq     = *c.ivf_pq_params;
    p.metric = (int)p.pq.metric;
  }
  CUVS_EXPECTS(metric_supported(p.metric),
               "tiered_index: unsupported metric %d (the L2 family, inner product and cosine are served by both tiers)", p.metric);
  return p;
}

void ti_device_view(DLManagedTensor* t, int64_t* shape, const void* data, DLDataType dt, int64_t rows, int64_t cols, int device)
{
  shape[0] = rows;
  shape[1] = cols;
  t->dl_tensor.data        = const_cast<void*>(data);
  t->dl_tensor.device      = DLDevice{kDLROCM, device};
  t->dl_tensor.ndim        = 2;
  t->dl_tensor.dtype       = dt;
  t->dl_tensor.shape       = shape;
  t->dl_tensor.strides     = nullptr;
  t->dl_tensor.byte_offset = 0;
  t->manager_ctx           = nullptr;
  t->deleter               = nullptr;
}

// a new ANN tier over rows [0, n) of the storage, with the stored parameters
std::shared_ptr<ti_ann> ti_build_ann(cuvsResources_t res_h, const ti_params& p, const std::shared_ptr<ti_storage>& st, int64_t n)
{
  auto& res = *as_res(res_h);
  auto ann  = std::make_shared<ti_ann>();
  ann->algo = p.algo;
  ann->rows = n;
  DLManagedTensor ds;
  int64_t shape[2];
  ti_device_view(&ds, shape, st->data.data(), DLDataType{kDLFloat, 32, 1}, n, st->dim, res.device);
  if (p.algo == CUVS_TIERED_INDEX_ALGO_CAGRA) {
    cuvsCagraIndexParams_t cp = nullptr;
    ti_call(cuvsCagraIndexParamsCreate(&cp));
    void* own_gb = cp->graph_build_params;  // the defaults' own allocation: kept for the destroy
    if (p.has_cagra) {
      *cp                    = p.cagra;
      cp->graph_build_params = own_gb;
    } else {
      cp->metric = (cuvsDistanceType)p.metric;
    }
    cuvsError_t rc = cuvsCagraIndexCreate(&ann->cagra);
    if (rc == CUVS_SUCCESS) rc = cuvsCagraBuild(res_h, cp, &ds, ann->cagra);
    cp->build_algo = IVF_PQ;  // so that the destroy frees own_gb as what it is
    cuvsCagraIndexParamsDestroy(cp);
    ti_call(rc);
    ann->backing = st;  // device rows: the index views them
  } else if (p.algo == CUVS_TIERED_INDEX_ALGO_IVF_FLAT) {
    cuvsIvfFlatIndexParams_t fp = nullptr;
    ti_call(cuvsIvfFlatIndexParamsCreate(&fp));
    if (p.has_flat) *fp = p.flat; else fp->metric = (cuvsDistanceType)p.metric;
    cuvsError_t rc = cuvsIvfFlatIndexCreate(&ann->flat);
    if (rc == CUVS_SUCCESS) rc = cuvsIvfFlatBuild(res_h, fp, &ds, ann->flat);
    cuvsIvfFlatIndexParamsDestroy(fp);
    ti_call(rc);
  } else {
    cuvsIvfPqIndexParams_t pp = nullptr;
    ti_call(cuvsIvfPqIndexParamsCreate(&pp));
    if (p.has_pq) *pp = p.pq; else pp->metric = (cuvsDistanceType)p.metric;
    cuvsError_t rc = cuvsIvfPqIndexCreate(&ann->pq);
    if (rc == CUVS_SUCCESS) rc = cuvsIvfPqBuild(res_h, pp, &ds, ann->pq);
    cuvsIvfPqIndexParamsDestroy(pp);
    ti_call(rc);
  }
  return ann;
}

std::shared_ptr<ti_storage> ti_new_storage(int64_t capacity, int64_t dim, int metric)
{
  auto st      = std::make_shared<ti_storage>();
  st->capacity = capacity;
  st->dim      = dim;
  st->data     = dev_buf<float>::persistent((size_t)capacity * dim);
  if (ti_keeps_norms(metric)) st->norms = dev_buf<float>::persistent((size_t)capacity);
  return st;
}

// rows (host or device, C-contiguous fp32 [n, dim]) -> storage rows [at, at + n), with their canonical norms
void ti_append_rows(resources& res, ti_storage& st, int64_t at, const void* rows, int64_t n, int metric)
{
  if (n == 0) return;
  float* dst = st.data.data() + at * st.dim;
  copy_async(res, dst, rows, (size_t)n * st.dim * sizeof(float));
  if (st.norms.data() != nullptr)
    row_norms<float>(res, dst, n, st.dim, st.dim, st.norms.data() + at, metric == M_CosineExpanded);
}

void ti_copy_rows(resources& res, ti_storage& dst, int64_t at, const ti_storage& src, int64_t n)
{
  copy_async(res, dst.data.data() + at * dst.dim, src.data.data(), (size_t)n * dst.dim * sizeof(float));
  if (dst.norms.data() != nullptr && src.norms.data() != nullptr)
    copy_async(res, dst.norms.data() + at, src.norms.data(), (size_t)n * sizeof(float));
}

void ti_compact(cuvsResources_t res_h, tiered_index& idx)
{
  if (idx.size == idx.ann_rows()) return;  // nothing in the tail
  idx.ann = ti_build_ann(res_h, idx.p, idx.st, idx.size);
}

// ------------------------------------------------------------------ the merge
template <bool kWaveOnly>
__device__ inline void ti_sync()
{
  if constexpr (kWaveOnly) {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  } else {
    __syncthreads();
  }
}

// One query: the k entries of A (an ANN result over rows [0, ann_rows): an entry is real iff 0 <= id < ann_rows, whatever its
// distance) and nb entries of B (real iff 0 <= id < INT64_MAX) -> the first k of the union by (distance, id), inner product by
// (-distance, id); slots beyond the real entries hold INT64_MAX and the worst value. keys / ids: P >= k + nb LDS entries.
template <bool kWaveOnly>
__device__ inline void ti_merge_row(const int64_t* __restrict__ a_i, const float* __restrict__ a_d, int k,
                                    const int64_t* __restrict__ b_i, const float* __restrict__ b_d, int nb, int64_t ann_rows,
                                    bool select_min, int64_t* __restrict__ out_i, float* __restrict__ out_d, uint32_t* keys,
                                    int64_t* ids, int P, int tid, int nthr)
{
  for (int j = tid; j < P; j += nthr) {
    uint32_t key = kTiPadKey;
    int64_t id   = INT64_MAX;
    if (j < k) {
      const int64_t v = a_i[j];
      if (v >= 0 && v < ann_rows) { id = v; const float d = a_d[j]; key = float_to_key(select_min ? d : -d); }
    } else if (j < k + nb) {
      const int64_t v = b_i[j - k];
      if (v >= 0 && v != INT64_MAX) { id = v; const float d = b_d[j - k]; key = float_to_key(select_min ? d : -d); }
    }
    keys[j] = key;
    ids[j]  = id;
  }
  ti_sync<kWaveOnly>();
  if constexpr (kWaveOnly) {
    wave_bitonic_sort<int64_t>(keys, ids, P);
  } else {
    block_bitonic_sort<int64_t>(keys, ids, P);
  }
  ti_sync<kWaveOnly>();
  for (int j = tid; j < k; j += nthr) {
    const int64_t id = ids[j];
    if (id == INT64_MAX) {
      out_i[j] = INT64_MAX;
      out_d[j] = select_min ? FLT_MAX : -FLT_MAX;
    } else {
      const float v = key_to_float(keys[j]);
      out_i[j]      = id;
      out_d[j]      = select_min ? v : -v;
    }
  }
}

// A [m, k] + B [m, <= kb] (row pitch ldb; b_cnt: optional per-row entry counts, clamped to kb - a count beyond kb raises
// *overflow) -> out [m, k]. kWaveOnly: a wave per row, four rows per workgroup, P <= 128; else a workgroup per row.
template <bool kWaveOnly>
__global__ __launch_bounds__(256) void tiered_merge_kernel(const int64_t* __restrict__ a_i, const float* __restrict__ a_d,
                                                           int64_t m, int k, const int64_t* __restrict__ b_i,
                                                           const float* __restrict__ b_d, int64_t ldb, int kb,
                                                           const int* __restrict__ b_cnt, int64_t ann_rows, bool select_min,
                                                           int64_t* __restrict__ out_i, float* __restrict__ out_d, int P,
                                                           int* __restrict__ overflow)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char ti_smem[];
  constexpr int nthr  = kWaveOnly ? 64 : 256;
  constexpr int slots = kWaveOnly ? 4 : 1;
  const int tid       = kWaveOnly ? (int)(threadIdx.x & 63) : (int)threadIdx.x;
  const int slot      = kWaveOnly ? (int)(threadIdx.x >> 6) : 0;
  const int64_t row   = kWaveOnly ? (int64_t)blockIdx.x * 4 + slot : (int64_t)blockIdx.x;
  if (row >= m) return;  // uniform over the wave / the workgroup
  int64_t* ids   = reinterpret_cast<int64_t*>(ti_smem) + (size_t)slot * P;
  uint32_t* keys = reinterpret_cast<uint32_t*>(ti_smem + (size_t)slots * P * sizeof(int64_t)) + (size_t)slot * P;
  int nb         = kb;
  if (b_cnt != nullptr) {
    nb = b_cnt[row];
    if (nb > kb) { if (tid == 0) *overflow = 1; nb = kb; }
  }
  ti_merge_row<kWaveOnly>(a_i + row * k, a_d + row * k, k, b_i + row * ldb, b_d + row * ldb, nb, ann_rows, select_min,
                          out_i + row * k, out_d + row * k, keys, ids, P, tid, nthr);
}

void ti_launch_merge(resources& res, const int64_t* a_i, const float* a_d, int64_t m, int k, const int64_t* b_i, const float* b_d,
                     int64_t ldb, int kb, const int* b_cnt, int64_t ann_rows, bool select_min, int64_t* out_i, float* out_d,
                     int* overflow)
{
  if (m == 0) return;
  int P = 2;
  while (P < k + kb) P <<= 1;
  CUVS_EXPECTS(P <= kTiMergeMaxP, "tiered_index: the merge takes k + kb <= %d entries (k = %d, kb = %d)", kTiMergeMaxP, k, kb);
  if (P <= kTiWaveMaxP) {
    hipLaunchKernelGGL((tiered_merge_kernel<true>), dim3(grid_blocks(m, 4)), dim3(256), (size_t)4 * P * 12, res.stream, a_i, a_d, m,
                       k, b_i, b_d, ldb, kb, b_cnt, ann_rows, select_min, out_i, out_d, P, overflow);
  } else {
    hipLaunchKernelGGL((tiered_merge_kernel<false>), dim3(grid_blocks(m, 1)), dim3(256), (size_t)P * 12, res.stream, a_i, a_d, m, k,
                       b_i, b_d, ldb, kb, b_cnt, ann_rows, select_min, out_i, out_d, P, overflow);
  }
  HIP_TRY(hipGetLastError());
}

// ------------------------------------------------------------------ small helpers of the tail phase
// thr[q] = the bound the tail has to beat: A's worst real value when all k entries are real, else the worst value of all
__device__ inline float ti_bound(const int64_t* __restrict__ a_i, const float* __restrict__ a_d, int k, int64_t ann_rows,
                                 bool select_min, int lane)
{
  float b  = select_min ? -FLT_MAX : FLT_MAX;
  bool pad = false;
  for (int j = lane; j < k; j += 64) {
    const int64_t v = a_i[j];
    if (v >= 0 && v < ann_rows) {
      const float d = a_d[j];
      b             = select_min ? fmaxf(b, d) : fminf(b, d);
    } else {
      pad = true;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float o = __shfl_xor(b, off, 64);
    b             = select_min ? fmaxf(b, o) : fminf(b, o);
  }
  if (__ballot(pad) != 0ull) b = select_min ? FLT_MAX : -FLT_MAX;
  return b;
}

__global__ __launch_bounds__(256) void tiered_bound_kernel(const int64_t* __restrict__ a_i, const float* __restrict__ a_d, int64_t m,
                                                           int k, int64_t ann_rows, bool select_min, float* __restrict__ thr)
{
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= m) return;
  const float b = ti_bound(a_i + row * k, a_d + row * k, k, ann_rows, select_min, threadIdx.x & 63);
  if ((threadIdx.x & 63) == 0) thr[row] = b;
}

// out bit j = in bit (off + j), j < n: the tail's slice of a bitset over global ids, for a search that counts from 0
__global__ void tiered_shift_bits_kernel(const uint32_t* __restrict__ in, int64_t off, int64_t n, uint32_t* __restrict__ out)
{
  const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w * 32 >= n) return;
  const int64_t bit0 = off + w * 32;
  const int64_t last = off + n - 1;  // the last bit the caller's bitset is known to hold
  const int sh       = (int)(bit0 & 31);
  uint32_t v         = in[bit0 >> 5] >> sh;
  if (sh != 0 && ((bit0 >> 5) + 1) <= (last >> 5)) v |= in[(bit0 >> 5) + 1] << (32 - sh);
  const int64_t left = n - w * 32;
  if (left < 32) v &= (1u << left) - 1u;
  out[w] = v;
}

// brute-force results over the tail -> global ids; slots that hold no admissible row (missing, or filtered: the worst value)
// -> INT64_MAX and the worst value
__global__ void tiered_globalize_kernel(int64_t* __restrict__ ids, float* __restrict__ d, int64_t total, int64_t ann_rows,
                                        bool select_min)
{
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const float worst = select_min ? FLT_MAX : -FLT_MAX;
  const int64_t v   = ids[t];
  if (v < 0 || d[t] == worst) { ids[t] = INT64_MAX; d[t] = worst; } else { ids[t] = v + ann_rows; }
}

__global__ void tiered_fill_kernel(int64_t* __restrict__ ids, float* __restrict__ d, int64_t total, float worst)
{
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < total) { ids[t] = INT64_MAX; d[t] = worst; }
}

struct ti_tail {
  int metric;
  const float* rows;   // [n, dim] device
  const float* norms;  // [n] or nullptr
  int64_t n, dim, ann_rows;
};

// B: the exact top-k of the tail with global ids (bits: over global ids, or nullptr)
void ti_tail_exact(resources& res, const ti_tail& t, const float* q, int64_t m, int k, const uint32_t* bits, int64_t* b_i, float* b_d)
{
  const bool select_min = t.metric != M_InnerProduct;
  dev_buf<uint32_t> local;
  if (bits != nullptr) {
    const int64_t words = (t.n + 31) / 32;
    local               = dev_buf<uint32_t>(res, (size_t)words);
    hipLaunchKernelGGL(tiered_shift_bits_kernel, dim3(grid_blocks(words, 256)), dim3(256), 0, res.stream, bits, t.ann_rows, t.n,
                       local.data());
  }
  bf_search_view(res, t.metric, t.rows, t.n, t.dim, t.norms, q, m, k, b_i, b_d, bits != nullptr ? local.data() : nullptr);
  hipLaunchKernelGGL(tiered_globalize_kernel, dim3(grid_blocks(m * k, 256)), dim3(256), 0, res.stream, b_i, b_d, m * k, t.ann_rows,
                     select_min);
  HIP_TRY(hipGetLastError());
}

// ------------------------------------------------------------------ the single-launch tail phase
struct ti_fused_args {
  const float* q;       // [m, dim]
  const float* x;       // [n, dim] tail rows
  const float* xn;      // [n] or nullptr
  const int64_t* a_i;   // [m, k]
  const float* a_d;
  const uint32_t* bits; // over global ids, or nullptr
  float* buf_v;         // [m, cap]
  int64_t* buf_i;
  int* cnt;             // [m] zeroed; cnt[m] = the ticket, cnt[m + 1] = the overflow flag
  int64_t* out_i;       // [m, k]
  float* out_d;
  int64_t n, dim, ann_rows;
  int m, k, cap, metric;
  int tiles_per_wg;
};

// QT: queries held in registers per pass over a tile (m <= 64 is covered in ceil(m / QT) passes)
template <int QT, bool VEC>
__global__ __launch_bounds__(256) void tiered_tail_kernel(ti_fused_args a)
{
  __shared__ __attribute__((aligned(16))) float s_q[kTiQFloats];      // queries, zero-padded to dimp; later the merge's LDS
  __shared__ __attribute__((aligned(16))) float s_x[kTiKC * kTiLdx];  // k-major tile of 256 rows x 16 columns
  __shared__ float s_qn[kTiFusedMaxM], s_thr[kTiFusedMaxM];
  __shared__ int s_last;
  const int tid         = threadIdx.x;
  const int lane        = tid & 63;
  const int wave        = tid >> 6;
  const bool select_min = a.metric != M_InnerProduct;
  const int dimp        = (int)((a.dim + kTiKC - 1) / kTiKC * kTiKC);

  // queries once per workgroup; their canonical norms (distance.hip row_norms: 64 strided fma partials + butterfly) and bounds
  for (int e = tid; e < a.m * dimp; e += 256) {
    const int i = e / dimp, c = e - i * dimp;
    s_q[e]      = c < a.dim ? a.q[(int64_t)i * a.dim + c] : 0.f;
  }
  for (int i = wave; i < a.m; i += 4) {
    const float* r = a.q + (int64_t)i * a.dim;
    float acc      = 0.f;
    for (int64_t j = lane; j < a.dim; j += 64) acc = __fmaf_rn(r[j], r[j], acc);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc = acc + __shfl_xor(acc, off, 64);
    const float b = ti_bound(a.a_i + (int64_t)i * a.k, a.a_d + (int64_t)i * a.k, a.k, a.ann_rows, select_min, lane);
    if (lane == 0) {
      s_qn[i]  = a.metric == M_InnerProduct ? 0.f : (a.metric == M_CosineExpanded ? sqrtf(acc) : acc);
      s_thr[i] = b;
    }
  }
  __syncthreads();

  for (int t = 0; t < a.tiles_per_wg; ++t) {
    const int64_t row0 = ((int64_t)blockIdx.x * a.tiles_per_wg + t) * kTiRows;
    if (row0 >= a.n) break;  // workgroup-uniform
    const int64_t row = row0 + tid;
    const float xnv   = (a.xn != nullptr && row < a.n) ? a.xn[row] : 0.f;
    bool keep         = row < a.n;
    if (keep && a.bits != nullptr) {
      const int64_t bit = a.ann_rows + row;
      keep              = (a.bits[bit >> 5] >> (bit & 31)) & 1u;
    }
    for (int q0 = 0; q0 < a.m; q0 += QT) {
      float acc[QT];
#pragma unroll
      for (int i = 0; i < QT; ++i) acc[i] = 0.f;
      for (int k0 = 0; k0 < dimp; k0 += kTiKC) {
        __syncthreads();  // the previous chunk has been read
#pragma unroll
        for (int u = 0; u < 4; ++u) {  // 256 rows x 4 chunks of 4 columns
          const int e = tid + 256 * u;
          const int r = e >> 2, c = e & 3;
          float v[4];
          load4<float, VEC>(a.x, row0 + r, a.n, a.dim, k0 + 4 * c, a.dim, v);
#pragma unroll
          for (int w = 0; w < 4; ++w) s_x[(4 * c + w) * kTiLdx + r] = v[w];
        }
        __syncthreads();
#pragma unroll 1
        for (int kk = 0; kk < kTiKC; kk += 4) {  // (not unrolled: 4 QT query values are live at a time, not 16 QT)
          float xv[4];
#pragma unroll
          for (int w = 0; w < 4; ++w) xv[w] = s_x[(kk + w) * kTiLdx + tid];
#pragma unroll
          for (int i = 0; i < QT; ++i) {
            // (queries past m read zeros or another query's row inside s_q: their sums are never used)
            const int qi   = (q0 + i < a.m) ? q0 + i : 0;
            const f32x4 qv = *reinterpret_cast<const f32x4*>(&s_q[qi * dimp + k0 + kk]);
            acc[i]         = __fmaf_rn(qv[0], xv[0], acc[i]);  // ascending k: the canonical chain
            acc[i]         = __fmaf_rn(qv[1], xv[1], acc[i]);
            acc[i]         = __fmaf_rn(qv[2], xv[2], acc[i]);
            acc[i]         = __fmaf_rn(qv[3], xv[3], acc[i]);
          }
        }
      }
      if (keep) {
#pragma unroll
        for (int i = 0; i < QT; ++i) {
          const int qi = q0 + i;
          if (qi >= a.m) break;
          const float d = finish_distance(acc[i], s_qn[qi], xnv, a.metric, 1e-6f);
          if (select_min ? d < s_thr[qi] : d > s_thr[qi]) {  // strictly: a tie goes to the ANN entry, whose id is smaller
            const int pos = atomicAdd(&a.cnt[qi], 1);
            if (pos < a.cap) {
              a.buf_v[(int64_t)qi * a.cap + pos] = d;
              a.buf_i[(int64_t)qi * a.cap + pos] = a.ann_rows + row;
            }
          }
        }
      }
    }
  }

  // the last workgroup to arrive merges; nobody waits
  __threadfence();
  __syncthreads();
  if (tid == 0) s_last = atomicAdd(&a.cnt[a.m], 1) == (int)gridDim.x - 1;
  __syncthreads();
  if (!s_last) return;
  __threadfence();
  int max_cnt = 0;
  for (int i = 0; i < a.m; ++i) max_cnt = max(max_cnt, __hip_atomic_load(&a.cnt[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  if (max_cnt > a.cap) {  // workgroup-uniform: the host redoes the batch exactly
    if (tid == 0) a.cnt[a.m + 1] = 1;
    return;
  }
  int P = 2;
  while (P < a.k + max_cnt) P <<= 1;
  unsigned char* smem = reinterpret_cast<unsigned char*>(s_q);  // 32 KiB: 2048 entries of 12 bytes, or four waves' 128
  if (P <= kTiWaveMaxP) {
    int64_t* ids   = reinterpret_cast<int64_t*>(smem) + (size_t)wave * P;
    uint32_t* keys = reinterpret_cast<uint32_t*>(smem + (size_t)4 * P * sizeof(int64_t)) + (size_t)wave * P;
    for (int i = wave; i < a.m; i += 4) {
      const int nb = __hip_atomic_load(&a.cnt[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      ti_merge_row<true>(a.a_i + (int64_t)i * a.k, a.a_d + (int64_t)i * a.k, a.k, a.buf_i + (int64_t)i * a.cap,
                         a.buf_v + (int64_t)i * a.cap, nb, a.ann_rows, select_min, a.out_i + (int64_t)i * a.k,
                         a.out_d + (int64_t)i * a.k, keys, ids, P, lane, 64);
      ti_sync<true>();
    }
  } else {
    int64_t* ids   = reinterpret_cast<int64_t*>(smem);
    uint32_t* keys = reinterpret_cast<uint32_t*>(smem + (size_t)P * sizeof(int64_t));
    for (int i = 0; i < a.m; ++i) {
      const int nb = __hip_atomic_load(&a.cnt[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      ti_merge_row<false>(a.a_i + (int64_t)i * a.k, a.a_d + (int64_t)i * a.k, a.k, a.buf_i + (int64_t)i * a.cap,
                          a.buf_v + (int64_t)i * a.cap, nb, a.ann_rows, select_min, a.out_i + (int64_t)i * a.k,
                          a.out_d + (int64_t)i * a.k, keys, ids, P, tid, 256);
      __syncthreads();
    }
  }
}

bool ti_fused_ok(int64_t m, int64_t dim, int k, int64_t n)
{
  return n >= 1 && m >= 1 && m <= kTiFusedMaxM && k <= kTiMaxK && m * round_up(dim, kTiKC) <= kTiQFloats;
}

// the (batch, tail) region in which the single-launch kernel is the default: where it measured faster than the composed path
// (scripts/tiered_tail_bench.py)
bool ti_fused_preferred(int64_t m, int64_t n)
{
  (void)m; (void)n;
  return false;  // not measured yet: the kernel runs where CUVS_AMD_TIERED_PATH=fused or cuvsAmdTieredTailSearch(path 2) asks for it
}

template <int QT>
void ti_launch_fused_qt(resources& res, const ti_fused_args& a, unsigned grid, bool vec)
{
  if (vec) {
    hipLaunchKernelGGL((tiered_tail_kernel<QT, true>), dim3(grid), dim3(256), 0, res.stream, a);
  } else {
    hipLaunchKernelGGL((tiered_tail_kernel<QT, false>), dim3(grid), dim3(256), 0, res.stream, a);
  }
}

// returns false when a query's buffer overflowed (nothing usable was written)
bool ti_tail_fused(resources& res, const ti_tail& t, const float* q, int64_t m, int k, const int64_t* a_i, const float* a_d,
                   const uint32_t* bits, int64_t* out_i, float* out_d)
{
  const int cap = (int)std::min<int64_t>(kTiCap, t.n);  // (a tail of at most cap rows cannot overflow)
  dev_buf<float> buf_v(res, (size_t)m * cap);
  dev_buf<int64_t> buf_i(res, (size_t)m * cap);
  dev_buf<int> cnt(res, (size_t)m + 2);
  HIP_TRY(hipMemsetAsync(cnt.data(), 0, cnt.bytes(), res.stream));
  ti_fused_args a;
  a.q = q; a.x = t.rows; a.xn = t.norms; a.a_i = a_i; a.a_d = a_d; a.bits = bits;
  a.buf_v = buf_v.data(); a.buf_i = buf_i.data(); a.cnt = cnt.data(); a.out_i = out_i; a.out_d = out_d;
  a.n = t.n; a.dim = t.dim; a.ann_rows = t.ann_rows; a.m = (int)m; a.k = k; a.cap = cap; a.metric = t.metric;
  // the tail over at least as many workgroups as there are compute units (while there are that many tiles); beyond four
  // workgroups per unit a workgroup takes several tiles, so that the queries are staged fewer times
  const int64_t tiles = (t.n + kTiRows - 1) / kTiRows;
  a.tiles_per_wg      = (int)std::max<int64_t>(1, (tiles + 4 * (int64_t)res.num_cus - 1) / (4 * (int64_t)res.num_cus));
  const unsigned grid = (unsigned)((tiles + a.tiles_per_wg - 1) / a.tiles_per_wg);
  const bool vec      = vec_ok(t.rows, t.dim, t.dim);
  profile_begin(res, "tiered_tail_kernel");
  if (m <= 4) ti_launch_fused_qt<4>(res, a, grid, vec);
  else if (m <= 16) ti_launch_fused_qt<16>(res, a, grid, vec);
  else ti_launch_fused_qt<32>(res, a, grid, vec);
  profile_end(res, "tiered_tail_kernel");
  HIP_TRY(hipGetLastError());
  g_ti_fused++;
  if (t.n <= cap) return true;
  return read_word(res, reinterpret_cast<const uint32_t*>(cnt.data() + m + 1)) == 0u;
}

// the composed path; returns false when a query's buffer overflowed
bool ti_tail_composed(resources& res, const ti_tail& t, const float* q, int64_t m, int k, const int64_t* a_i, const float* a_d,
                      const uint32_t* bits, int64_t* out_i, float* out_d)
{
  const bool select_min = t.metric != M_InnerProduct;
  const int cap         = (int)std::min<int64_t>(kTiCap, t.n);
  const int64_t m_tile  = std::min<int64_t>(m, 4096);
  dev_buf<float> buf_v(res, (size_t)m_tile * cap), thr(res, (size_t)m_tile), qn;
  dev_buf<int64_t> buf_i(res, (size_t)m_tile * cap);
  dev_buf<int> cnt(res, (size_t)m_tile + 1);  // cnt[m_tile]: the overflow flag
  if (t.metric != M_InnerProduct) {
    qn = dev_buf<float>(res, (size_t)m);
    row_norms<float>(res, q, m, t.dim, t.dim, qn.data(), t.metric == M_CosineExpanded);
  }
  HIP_TRY(hipMemsetAsync(cnt.data(), 0, cnt.bytes(), res.stream));
  for (int64_t r0 = 0; r0 < m; r0 += m_tile) {
    const int64_t mr = std::min(m_tile, m - r0);
    if (r0 > 0) HIP_TRY(hipMemsetAsync(cnt.data(), 0, (size_t)m_tile * sizeof(int), res.stream));
    hipLaunchKernelGGL(tiered_bound_kernel, dim3(grid_blocks(mr, 4)), dim3(256), 0, res.stream, a_i + r0 * k, a_d + r0 * k, mr, k,
                       t.ann_rows, select_min, thr.data());
    pairwise_threshold_append<float, float>(res, q + r0 * t.dim, mr, t.dim, t.rows, t.n, t.dim, t.dim,
                                            qn.data() ? qn.data() + r0 : nullptr, t.norms, t.metric, buf_v.data(), buf_i.data(),
                                            cnt.data(), 0, cap, t.ann_rows, r0, t.ann_rows + t.n, bits, bits != nullptr ? 1 : 0, 1,
                                            thr.data());
    ti_launch_merge(res, a_i + r0 * k, a_d + r0 * k, mr, k, buf_i.data(), buf_v.data(), cap, cap, cnt.data(), t.ann_rows, select_min,
                    out_i + r0 * k, out_d + r0 * k, cnt.data() + m_tile);
  }
  g_ti_composed++;
  if (t.n <= cap) return true;
  return read_word(res, reinterpret_cast<const uint32_t*>(cnt.data() + m_tile)) == 0u;
}

// path: 0 the library's choice, 1 composed, 2 fused (refused beyond its shapes)
void ti_tail_phase(resources& res, const ti_tail& t, const float* q, int64_t m, int k, const int64_t* a_i, const float* a_d,
                   const uint32_t* bits, int64_t* out_i, float* out_d, int path)
{
  if (m == 0) return;
  const bool select_min = t.metric != M_InnerProduct;
  const bool fused_ok   = ti_fused_ok(m, t.dim, k, t.n);
  CUVS_EXPECTS(path != 2 || fused_ok,
               "tiered_index: the single-launch tail kernel takes 1 <= m <= %d, k <= %d and m * round_up(dim, %d) <= %d", kTiFusedMaxM,
               kTiMaxK, kTiKC, kTiQFloats);
  bool done = false;
  if (k <= kTiMaxK) {
    if (path == 2 || (path == 0 && fused_ok && ti_fused_preferred(m, t.n))) {
      done = ti_tail_fused(res, t, q, m, k, a_i, a_d, bits, out_i, out_d);
    } else {
      done = ti_tail_composed(res, t, q, m, k, a_i, a_d, bits, out_i, out_d);
    }
    if (done) return;
    g_ti_redo++;
  }
  // exactly: the tail's own top-k, then the merge
  dev_buf<int64_t> b_i(res, (size_t)m * k);
  dev_buf<float> b_d(res, (size_t)m * k);
  ti_tail_exact(res, t, q, m, k, bits, b_i.data(), b_d.data());
  ti_launch_merge(res, a_i, a_d, m, k, b_i.data(), b_d.data(), k, k, nullptr, t.ann_rows, select_min, out_i, out_d, nullptr);
}

// ------------------------------------------------------------------ search
struct ti_search_io {
  DLManagedTensor* queries;
  const float* q;
  int64_t m, k;
  const uint32_t* bits;
  cuvsFilter filter;
};

void ti_check_out(const DLTensor& nb, const DLTensor& ds, int64_t m, int64_t k)
{
  CUVS_EXPECTS(is_device_accessible(nb), "neighbors should have device compatible memory");
  CUVS_EXPECTS(is_device_accessible(ds), "distances should have device compatible memory");
  CUVS_EXPECTS(dtype_is(nb.dtype, kDLInt, 64), "neighbors should be of type int64_t");
  CUVS_EXPECTS(dtype_is(ds.dtype, kDLFloat, 32), "distances should be of type float32");
  CUVS_EXPECTS(nb.ndim == 2 && ds.ndim == 2 && is_c_contiguous(nb) && is_c_contiguous(ds), "outputs must be C-contiguous matrices");
  CUVS_EXPECTS(nb.shape[0] == m && ds.shape[0] == m && nb.shape[1] == k && ds.shape[1] == k, "neighbors/distances shape mismatch");
}

ti_search_io ti_check_search(const cuvsTieredIndex& handle, const tiered_index& idx, DLManagedTensor* queries_tensor,
                             DLManagedTensor* neighbors_tensor, cuvsFilter filter)
{
  CUVS_EXPECTS(queries_tensor != nullptr && neighbors_tensor != nullptr, "null argument");
  auto& queries = queries_tensor->dl_tensor;
  CUVS_EXPECTS(is_device_accessible(queries), "queries should have device compatible memory");
  CUVS_EXPECTS(queries.dtype.code == handle.dtype.code && queries.dtype.bits == handle.dtype.bits,
               "type mismatch between index and queries");
  CUVS_EXPECTS(queries.ndim == 2 && is_c_contiguous(queries), "queries must be a C-contiguous matrix");
  CUVS_EXPECTS(queries.shape[1] == idx.dim, "queries dim %ld != index dim %ld", (long)queries.shape[1], (long)idx.dim);
  ti_search_io io{};
  io.queries = queries_tensor;
  io.q       = static_cast<const float*>(dl_data(queries));
  io.m       = queries.shape[0];
  io.k       = neighbors_tensor->dl_tensor.ndim == 2 ? neighbors_tensor->dl_tensor.shape[1] : 0;
  io.filter  = filter;
  if (filter.type != NO_FILTER) {
    CUVS_EXPECTS(filter.type == BITSET, "Unsupported filter type: BITMAP");
    CUVS_EXPECTS(filter.addr != 0, "prefilter tensor is null");
    auto& ft = reinterpret_cast<DLManagedTensor*>(filter.addr)->dl_tensor;
    CUVS_EXPECTS(dtype_is(ft.dtype, kDLUInt, 32) && is_device_accessible(ft), "prefilter must be a device uint32 tensor");
    int64_t words = 1;
    for (int i = 0; i < ft.ndim; ++i) words *= ft.shape[i];
    CUVS_EXPECTS(words * 32 >= idx.size, "bitset filter holds %ld bits, the index %ld rows", (long)(words * 32), (long)idx.size);
    io.bits = static_cast<const uint32_t*>(dl_data(ft));
  }
  CUVS_EXPECTS(io.k >= 1, "k must be positive");
  return io;
}

// the ANN tier's own search into device [m, k] buffers
void ti_search_ann(cuvsResources_t res_h, const tiered_index& idx, void* search_params, const ti_search_io& io, int64_t* out_i,
                   float* out_d)
{
  auto& res = *as_res(res_h);
  DLManagedTensor nb, ds;
  int64_t s1[2], s2[2];
  ti_device_view(&nb, s1, out_i, DLDataType{kDLInt, 64, 1}, io.m, io.k, res.device);
  ti_device_view(&ds, s2, out_d, DLDataType{kDLFloat, 32, 1}, io.m, io.k, res.device);
  const ti_ann& ann = *idx.ann;
  if (ann.algo == CUVS_TIERED_INDEX_ALGO_CAGRA) {
    cuvsCagraSearchParams_t sp = static_cast<cuvsCagraSearchParams_t>(search_params), own = nullptr;
    if (sp == nullptr) { ti_call(cuvsCagraSearchParamsCreate(&own)); sp = own; }
    const cuvsError_t rc = cuvsCagraSearch(res_h, sp, ann.cagra, io.queries, &nb, &ds, io.filter);
    if (own) cuvsCagraSearchParamsDestroy(own);
    ti_call(rc);
  } else if (ann.algo == CUVS_TIERED_INDEX_ALGO_IVF_FLAT) {
    cuvsIvfFlatSearchParams_t sp = static_cast<cuvsIvfFlatSearchParams_t>(search_params), own = nullptr;
    if (sp == nullptr) { ti_call(cuvsIvfFlatSearchParamsCreate(&own)); sp = own; }
    const cuvsError_t rc = cuvsIvfFlatSearch(res_h, sp, ann.flat, io.queries, &nb, &ds, io.filter);
    if (own) cuvsIvfFlatSearchParamsDestroy(own);
    ti_call(rc);
  } else {
    cuvsIvfPqSearchParams_t sp = static_cast<cuvsIvfPqSearchParams_t>(search_params), own = nullptr;
    if (sp == nullptr) { ti_call(cuvsIvfPqSearchParamsCreate(&own)); sp = own; }
    const cuvsError_t rc = cuvsAmdIvfPqSearchFiltered(res_h, sp, ann.pq, io.queries, &nb, &ds, io.filter);
    if (own) cuvsIvfPqSearchParamsDestroy(own);
    ti_call(rc);
  }
}

ti_tail ti_tail_of(const tiered_index& idx)
{
  const int64_t ar = idx.ann_rows();
  return ti_tail{idx.p.metric, idx.st->data.data() + ar * idx.dim, idx.st->norms.data() ? idx.st->norms.data() + ar : nullptr,
                 idx.size - ar, idx.dim, ar};
}

tiered_index& get_tiered(cuvsTieredIndex_t index)
{
  CUVS_EXPECTS(index != nullptr && index->addr != 0, "tiered index is not built");
  return *reinterpret_cast<tiered_index*>(index->addr);
}

void ti_check_rows_dtype(const DLTensor& ds)
{
  CUVS_EXPECTS(dtype_is(ds.dtype, kDLFloat, 32), "Unsupported dataset DLtensor dtype: %d and bits: %d", (int)ds.dtype.code,
               (int)ds.dtype.bits);
}

}  // namespace
}  // namespace cuvs_amd

using namespace cuvs_amd;

extern "C" {

cuvsError_t cuvsTieredIndexCreate(cuvsTieredIndex_t* index)
{
  return (cuvsError_t)translate_exceptions([=] {
    CUVS_EXPECTS(index != nullptr, "index is null");
    *index = new cuvsTieredIndex{0, DLDataType{0, 0, 0}, CUVS_TIERED_INDEX_ALGO_CAGRA};
  });
}

cuvsError_t cuvsTieredIndexDestroy(cuvsTieredIndex_t index)
{
  return (cuvsError_t)translate_exceptions([=] {
    if (index == nullptr) return;
    delete reinterpret_cast<tiered_index*>(index->addr);
    delete index;
  });
}

cuvsError_t cuvsTieredIndexParamsCreate(cuvsTieredIndexParams_t* params)
{
  return (cuvsError_t)translate_exceptions([=] {
    CUVS_EXPECTS(params != nullptr, "params is null");
    *params = new cuvsTieredIndexParams{L2Expanded, CUVS_TIERED_INDEX_ALGO_CAGRA, 100000, false, nullptr, nullptr, nullptr};
  });
}

cuvsError_t cuvsTieredIndexParamsDestroy(cuvsTieredIndexParams_t params)
{
  return (cuvsError_t)translate_exceptions([=] { delete params; });
}

cuvsError_t cuvsTieredIndexBuild(cuvsResources_t res_h, cuvsTieredIndexParams_t params, DLManagedTensor* dataset_tensor,
                                 cuvsTieredIndex_t index)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& res = *as_res(res_h);
    CUVS_EXPECTS(params != nullptr && dataset_tensor != nullptr && index != nullptr, "null argument");
    auto& ds = dataset_tensor->dl_tensor;
    ti_check_rows_dtype(ds);
    CUVS_EXPECTS(ds.ndim == 2, "dataset should be a 2-dimensional tensor");
    CUVS_EXPECTS(ds.shape != nullptr, "dataset should have an initialized shape");
    CUVS_EXPECTS(is_c_contiguous(ds), "dataset must be C-contiguous");
    auto idx       = std::make_unique<tiered_index>();
    idx->p         = ti_convert_params(*params);
    const int64_t n = ds.shape[0];
    idx->dim       = ds.shape[1];
    CUVS_EXPECTS(idx->dim >= 1, "dataset must have at least one column");
    idx->st = ti_new_storage(n + n / 16, idx->dim, idx->p.metric);
    ti_append_rows(res, *idx->st, 0, dl_data(ds), n, idx->p.metric);
    idx->size = n;
    if (n > idx->p.min_ann_rows) idx->ann = ti_build_ann(res_h, idx->p, idx->st, n);
    sync(res);  // host rows may go away once the call returns
    delete reinterpret_cast<tiered_index*>(index->addr);
    index->addr  = reinterpret_cast<uintptr_t>(idx.release());
    index->dtype = ds.dtype;
    index->algo  = params->algo;
  });
}

cuvsError_t cuvsTieredIndexExtend(cuvsResources_t res_h, DLManagedTensor* new_vectors, cuvsTieredIndex_t index)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& res = *as_res(res_h);
    CUVS_EXPECTS(new_vectors != nullptr, "null argument");
    auto& idx = get_tiered(index);
    auto& nv  = new_vectors->dl_tensor;
    ti_check_rows_dtype(nv);
    CUVS_EXPECTS(nv.ndim == 2 && is_c_contiguous(nv), "new vectors must be a C-contiguous matrix");
    CUVS_EXPECTS(nv.shape[1] == idx.dim, "Dimension of new vectors must match existing data");
    const int64_t n_new = nv.shape[0];
    if (idx.size + n_new > idx.st->capacity) {
      const int64_t cap = std::max<int64_t>(idx.size + n_new, 2 * idx.st->capacity);
      auto grown        = ti_new_storage(cap, idx.dim, idx.p.metric);
      ti_copy_rows(res, *grown, 0, *idx.st, idx.size);  // rows and norms are copied, not recomputed
      // a viewing ANN tier follows its rows: [0, ann_rows) are the same bytes in the new allocation. A tier shared with
      // another index (merge) stays where it is - its `backing` keeps that allocation alive.
      if (idx.ann && idx.ann->cagra != nullptr && idx.ann->backing == idx.st && idx.ann.use_count() == 1) {
        cagra_repoint_dataset(idx.ann->cagra->addr, grown->data.data());
        idx.ann->backing = grown;
      }
      sync(res);  // the copies have left the old allocation before it is released
      idx.st = std::move(grown);
    }
    ti_append_rows(res, *idx.st, idx.size, dl_data(nv), n_new, idx.p.metric);
    idx.size += n_new;
    if (idx.p.create_ann_on_extend && idx.size - idx.ann_rows() > idx.p.min_ann_rows) ti_compact(res_h, idx);
    sync(res);
  });
}

cuvsError_t cuvsAmdTieredIndexCompact(cuvsResources_t res_h, cuvsTieredIndex_t index)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& res = *as_res(res_h);
    ti_compact(res_h, get_tiered(index));
    sync(res);
  });
}

cuvsError_t cuvsAmdTieredIndexGetInfo(cuvsTieredIndex_t index, int64_t* size, int64_t* ann_rows, int64_t* capacity, int64_t* dim)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& idx = get_tiered(index);
    if (size) *size = idx.size;
    if (ann_rows) *ann_rows = idx.ann_rows();
    if (capacity) *capacity = idx.st->capacity;
    if (dim) *dim = idx.dim;
  });
}

cuvsError_t cuvsTieredIndexMerge(cuvsResources_t res_h, cuvsTieredIndexParams_t params, cuvsTieredIndex_t* indices,
                                 size_t num_indices, cuvsTieredIndex_t output_index)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& res = *as_res(res_h);
    CUVS_EXPECTS(num_indices >= 1, "must have at least one index to merge");
    CUVS_EXPECTS(params != nullptr && indices != nullptr && output_index != nullptr, "null argument");
    int64_t n_rows = 0, dim = 0;
    for (size_t i = 0; i < num_indices; ++i) {
      CUVS_EXPECTS(indices[i] != nullptr,
                   "Null pointer detected in 'indices'. Ensure all elements are valid before usage.");
      CUVS_EXPECTS(indices[i]->dtype.code == indices[0]->dtype.code, "indices must all have the same dtype");
      CUVS_EXPECTS(indices[i]->dtype.bits == indices[0]->dtype.bits, "indices must all have the same dtype");
      CUVS_EXPECTS(indices[i]->algo == indices[0]->algo, "indices must all have the same index algorithm");
      auto& src = get_tiered(indices[i]);
      n_rows += src.size;
      if (dim) {
        CUVS_EXPECTS(dim == src.dim, "indices must all have the same dimensionality");
      } else {
        dim = src.dim;
      }
    }
    auto& first = get_tiered(indices[0]);
    auto idx    = std::make_unique<tiered_index>();
    idx->dim    = dim;
    idx->ann    = first.ann;  // its rows are still the first rows
    if (num_indices == 1) {
      // a copy of the one index: rows and norms copied, the (immutable) ANN tier shared, the build parameters kept
      idx->p  = first.p;
      idx->st = ti_new_storage(first.st->capacity, dim, idx->p.metric);
      ti_copy_rows(res, *idx->st, 0, *first.st, first.size);
      idx->size = first.size;
    } else {
      idx->p = ti_convert_params(*params);
      CUVS_EXPECTS(idx->p.algo == (int)indices[0]->algo, "index_params->algo differs from the algorithm of the indices");
      for (size_t i = 0; i < num_indices; ++i)
        CUVS_EXPECTS(ti_keeps_norms(get_tiered(indices[i]).p.metric) == ti_keeps_norms(idx->p.metric) &&
                       (get_tiered(indices[i]).p.metric == M_CosineExpanded) == (idx->p.metric == M_CosineExpanded),
                     "tiered_index::merge: the stored norms of index %zu do not serve metric %d", i, idx->p.metric);
      idx->st = ti_new_storage(n_rows, dim, idx->p.metric);
      for (size_t i = 0; i < num_indices; ++i) {
        auto& src = get_tiered(indices[i]);
        ti_copy_rows(res, *idx->st, idx->size, *src.st, src.size);
        idx->size += src.size;
      }
      if (idx->size - idx->ann_rows() > idx->p.min_ann_rows) ti_compact(res_h, *idx);
    }
    sync(res);
    const DLDataType dt = indices[0]->dtype;
    const auto algo     = indices[0]->algo;
    delete reinterpret_cast<tiered_index*>(output_index->addr);  // (may be one of `indices`: everything needed was copied)
    output_index->addr  = reinterpret_cast<uintptr_t>(idx.release());
    output_index->dtype = dt;
    output_index->algo  = algo;
  });
}

cuvsError_t cuvsTieredIndexSearch(cuvsResources_t res_h, void* search_params, cuvsTieredIndex_t index, DLManagedTensor* queries_tensor,
                                  DLManagedTensor* neighbors_tensor, DLManagedTensor* distances_tensor, cuvsFilter prefilter)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& res = *as_res(res_h);
    CUVS_EXPECTS(queries_tensor && neighbors_tensor && distances_tensor, "null argument");
    CUVS_EXPECTS(is_device_accessible(queries_tensor->dl_tensor), "queries should have device compatible memory");
    CUVS_EXPECTS(is_device_accessible(neighbors_tensor->dl_tensor), "neighbors should have device compatible memory");
    CUVS_EXPECTS(is_device_accessible(distances_tensor->dl_tensor), "distances should have device compatible memory");
    CUVS_EXPECTS(dtype_is(neighbors_tensor->dl_tensor.dtype, kDLInt, 64), "neighbors should be of type int64_t");
    CUVS_EXPECTS(dtype_is(distances_tensor->dl_tensor.dtype, kDLFloat, 32), "distances should be of type float32");
    auto& idx = get_tiered(index);
    auto io   = ti_check_search(*index, idx, queries_tensor, neighbors_tensor, prefilter);
    ti_check_out(neighbors_tensor->dl_tensor, distances_tensor->dl_tensor, io.m, io.k);
    int64_t* out_i = static_cast<int64_t*>(dl_data(neighbors_tensor->dl_tensor));
    float* out_d   = static_cast<float*>(dl_data(distances_tensor->dl_tensor));
    const ti_tail t = ti_tail_of(idx);
    if (t.n == 0) {  // (an index always holds an ANN tier or a tail, or no row at all)
      CUVS_EXPECTS(idx.ann != nullptr, "tiered index holds no rows");
      ti_search_ann(res_h, idx, search_params, io, out_i, out_d);
      return;
    }
    if (!idx.ann) {  // the exact brute-force result, as cuvsBruteForceSearch gives it
      bf_search_view(res, t.metric, t.rows, t.n, t.dim, t.norms, io.q, io.m, (int)io.k, out_i, out_d, io.bits);
      return;
    }
    CUVS_EXPECTS(io.k <= kTiMergeMaxP / 2, "tiered_index: k = %ld is beyond the merge of two tiers (k <= %d)", (long)io.k,
                 kTiMergeMaxP / 2);
    dev_buf<int64_t> a_i(res, (size_t)io.m * io.k);
    dev_buf<float> a_d(res, (size_t)io.m * io.k);
    ti_search_ann(res_h, idx, search_params, io, a_i.data(), a_d.data());
    ti_tail_phase(res, t, io.q, io.m, (int)io.k, a_i.data(), a_d.data(), io.bits, out_i, out_d, res.tune.tiered_path);
  });
}

cuvsError_t cuvsAmdTieredIndexSearchTiers(cuvsResources_t res_h, void* search_params, cuvsTieredIndex_t index,
                                          DLManagedTensor* queries_tensor, DLManagedTensor* ann_neighbors,
                                          DLManagedTensor* ann_distances, DLManagedTensor* tail_neighbors,
                                          DLManagedTensor* tail_distances, cuvsFilter prefilter)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& res = *as_res(res_h);
    CUVS_EXPECTS(queries_tensor && ann_neighbors && ann_distances && tail_neighbors && tail_distances, "null argument");
    auto& idx = get_tiered(index);
    auto io   = ti_check_search(*index, idx, queries_tensor, ann_neighbors, prefilter);
    ti_check_out(ann_neighbors->dl_tensor, ann_distances->dl_tensor, io.m, io.k);
    ti_check_out(tail_neighbors->dl_tensor, tail_distances->dl_tensor, io.m, io.k);
    const ti_tail t   = ti_tail_of(idx);
    const float worst = t.metric != M_InnerProduct ? FLT_MAX : -FLT_MAX;
    int64_t* an = static_cast<int64_t*>(dl_data(ann_neighbors->dl_tensor));
    float* ad   = static_cast<float*>(dl_data(ann_distances->dl_tensor));
    int64_t* tn = static_cast<int64_t*>(dl_data(tail_neighbors->dl_tensor));
    float* td   = static_cast<float*>(dl_data(tail_distances->dl_tensor));
    const int64_t total = io.m * io.k;
    if (total == 0) return;
    if (idx.ann) {
      ti_search_ann(res_h, idx, search_params, io, an, ad);
    } else {
      hipLaunchKernelGGL(tiered_fill_kernel, dim3(grid_blocks(total, 256)), dim3(256), 0, res.stream, an, ad, total, worst);
    }
    if (t.n > 0) {
      ti_tail_exact(res, t, io.q, io.m, (int)io.k, io.bits, tn, td);
    } else {
      hipLaunchKernelGGL(tiered_fill_kernel, dim3(grid_blocks(total, 256)), dim3(256), 0, res.stream, tn, td, total, worst);
    }
    HIP_TRY(hipGetLastError());
  });
}

cuvsError_t cuvsAmdTieredTailSearch(cuvsResources_t res_h, cuvsDistanceType metric, DLManagedTensor* tail_tensor, int64_t ann_rows,
                                    DLManagedTensor* queries_tensor, DLManagedTensor* seed_neighbors, DLManagedTensor* seed_distances,
                                    DLManagedTensor* bitset, int path, DLManagedTensor* neighbors_tensor,
                                    DLManagedTensor* distances_tensor)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& res = *as_res(res_h);
    CUVS_EXPECTS(tail_tensor && queries_tensor && seed_neighbors && seed_distances && neighbors_tensor && distances_tensor,
                 "null argument");
    CUVS_EXPECTS(metric_supported((int)metric), "tiered_index: unsupported metric %d", (int)metric);
    CUVS_EXPECTS(path >= 0 && path <= 2, "path must be 0, 1 or 2");
    CUVS_EXPECTS(ann_rows >= 0, "ann_rows must not be negative");
    auto& tl = tail_tensor->dl_tensor;
    auto& qs = queries_tensor->dl_tensor;
    for (const DLTensor* x : {&tl, &qs})
      CUVS_EXPECTS(is_device_accessible(*x) && dtype_is(x->dtype, kDLFloat, 32) && x->ndim == 2 && is_c_contiguous(*x),
                   "tail and queries must be C-contiguous fp32 matrices on the device");
    CUVS_EXPECTS(qs.shape[1] == tl.shape[1], "queries dim %ld != tail dim %ld", (long)qs.shape[1], (long)tl.shape[1]);
    const int64_t m = qs.shape[0], n = tl.shape[0], dim = tl.shape[1];
    CUVS_EXPECTS(n >= 1, "the tail must hold at least one row");
    const int64_t k = neighbors_tensor->dl_tensor.ndim == 2 ? neighbors_tensor->dl_tensor.shape[1] : 0;
    CUVS_EXPECTS(k >= 1 && k <= kTiMergeMaxP / 2, "k must be in [1, %d]", kTiMergeMaxP / 2);
    ti_check_out(neighbors_tensor->dl_tensor, distances_tensor->dl_tensor, m, k);
    ti_check_out(seed_neighbors->dl_tensor, seed_distances->dl_tensor, m, k);
    const uint32_t* bits = nullptr;
    if (bitset != nullptr) {
      auto& ft = bitset->dl_tensor;
      CUVS_EXPECTS(dtype_is(ft.dtype, kDLUInt, 32) && is_device_accessible(ft), "bitset must be a device uint32 tensor");
      int64_t words = 1;
      for (int i = 0; i < ft.ndim; ++i) words *= ft.shape[i];
      CUVS_EXPECTS(words * 32 >= ann_rows + n, "bitset holds %ld bits, the ids reach %ld", (long)(words * 32), (long)(ann_rows + n));
      bits = static_cast<const uint32_t*>(dl_data(ft));
    }
    dev_buf<float> norms;
    if (ti_keeps_norms((int)metric)) {
      norms = dev_buf<float>(res, (size_t)n);
      row_norms<float>(res, static_cast<const float*>(dl_data(tl)), n, dim, dim, norms.data(), (int)metric == M_CosineExpanded);
    }
    const ti_tail t{(int)metric, static_cast<const float*>(dl_data(tl)), norms.data(), n, dim, ann_rows};
    ti_tail_phase(res, t, static_cast<const float*>(dl_data(qs)), m, (int)k, static_cast<const int64_t*>(dl_data(seed_neighbors->dl_tensor)),
                  static_cast<const float*>(dl_data(seed_distances->dl_tensor)), bits,
                  static_cast<int64_t*>(dl_data(neighbors_tensor->dl_tensor)), static_cast<float*>(dl_data(distances_tensor->dl_tensor)),
                  path);
  });
}

cuvsError_t cuvsAmdTieredMerge(cuvsResources_t res_h, DLManagedTensor* a_neighbors, DLManagedTensor* a_distances,
                               DLManagedTensor* b_neighbors, DLManagedTensor* b_distances, int64_t ann_rows, int select_min,
                               DLManagedTensor* out_neighbors, DLManagedTensor* out_distances)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& res = *as_res(res_h);
    CUVS_EXPECTS(a_neighbors && a_distances && b_neighbors && b_distances && out_neighbors && out_distances, "null argument");
    auto& an = a_neighbors->dl_tensor;
    auto& bn = b_neighbors->dl_tensor;
    CUVS_EXPECTS(an.ndim == 2 && bn.ndim == 2, "neighbors must be matrices");
    const int64_t m = an.shape[0], k = an.shape[1], kb = bn.shape[1];
    CUVS_EXPECTS(k >= 1 && kb >= 1, "k and kb must be positive");
    ti_check_out(an, a_distances->dl_tensor, m, k);
    ti_check_out(bn, b_distances->dl_tensor, m, kb);
    ti_check_out(out_neighbors->dl_tensor, out_distances->dl_tensor, m, k);
    ti_launch_merge(res, static_cast<const int64_t*>(dl_data(an)), static_cast<const float*>(dl_data(a_distances->dl_tensor)), m, (int)k,
                    static_cast<const int64_t*>(dl_data(bn)), static_cast<const float*>(dl_data(b_distances->dl_tensor)), kb, (int)kb,
                    nullptr, ann_rows, select_min != 0, static_cast<int64_t*>(dl_data(out_neighbors->dl_tensor)),
                    static_cast<float*>(dl_data(out_distances->dl_tensor)), nullptr);
  });
}

void cuvsAmdTieredCounters(unsigned long long out[3])
{
  out[0] = g_ti_composed.load();
  out[1] = g_ti_fused.load();
  out[2] = g_ti_redo.load();
}

}  // extern "C"
