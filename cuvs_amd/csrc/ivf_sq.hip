// IVF-SQ on MI355X: index build/extend, list-major scan over 8-bit scalar-quantized rows, C ABI (drop-in for
// c/src/neighbors/ivf_sq.cpp).
//
// Reference: cpp/src/neighbors/ivf_sq/ivf_sq_build.cuh (training of the per-dimension quantizer on the residuals of a
// row sample, encoding), ivf_sq_search.cuh + detail/jit_lto_kernels (scan arithmetic), ivf_sq_serialize.cuh (file),
// cpp/include/cuvs/neighbors/ivf_sq.hpp (list layout of the file: 32-row groups of 16-byte chunks).
//
// MI355X design (the schedule of ivf_flat.hip): all lists in one flat allocation, rows in tiles of 64 (one wave64 lane
// per row), [tile][chunk][lane] x 16 codes, the dimension padded to 16 with code 0 -> one chunk load of a wave is 1 KiB
// and coalesced. (query, probe) pairs grouped by list, up to 8 queries per work item share one pass over the list's
// codes; a lane converts every code byte to fp32 once and applies it to all queries of the item. The per-pair query
// terms ([dim_pad][8] fp32 per item) and the per-dimension quantizer values are read with wave-uniform addresses
// (scalar cache -> SGPRs). Per-wave register top lists with shared k-th bounds (k <= 256), or every score written out
// and selected (k > 256). DESIGN 3.2 has the arithmetic contract.
#include "ivf_list_scan.hpp"
#include "ivf_lists.hpp"
#include "npy_io.hpp"

#include <cuvs/neighbors/ivf_sq.h>

#include <algorithm>
#include <cfloat>
#include <type_traits>

namespace cuvs_amd {

struct ivf_sq_index : ivf_lists {  // data: [padded_rows / 64, n_chunks, 64, 16 codes], the dimension padded to 16
  int metric   = 0;
  elem_t dtype = elem_t::f32;  // element type of the rows the index was built from (f32 / f16)
  bool conservative_memory_allocation = false;
  uint32_t dim = 0;
  dev_buf<float> centers;            // [n_lists, dim]
  dev_buf<float> center_norms;       // [n_lists] canonical |c|^2
  dev_buf<float> center_norms_sqrt;  // [n_lists] |c| (cosine only)
  dev_buf<float> vmin, delta;        // [dim] the scalar quantizer
};

namespace {

constexpr int kSqThreads = 512;
constexpr int kSqWaves   = kSqThreads / 64;
constexpr int kSqQPB     = 8;
constexpr int kSqStop    = 4;  // chunk loads issued 4 at a time (dot products)

typedef float f32x2_t __attribute__((ext_vector_type(2)));

inline bool sq_metric_ok(int m)
{
  return m == M_L2Expanded || m == M_L2SqrtExpanded || m == M_InnerProduct || m == M_CosineExpanded;
}

// ------------------------------------------------------------------ training of the quantizer
// residual of every sample row against its centre, in place; fp16 data: rounded back to fp16 (the reference keeps the
// training residuals in the element type)
__global__ void sq_residuals_kernel(float* __restrict__ x, const float* __restrict__ centers, const uint32_t* __restrict__ labels,
                                    int64_t n, uint32_t dim, int round_half)
{
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * dim) return;
  const int64_t i = t / dim;
  const uint32_t d = (uint32_t)(t % dim);
  float r = x[t] - centers[(size_t)labels[i] * dim + d];
  if (round_half) r = __half2float(__float2half_rn(r));
  x[t] = r;
}

// per-dimension min / max: workgroup b takes a run of rows, thread t the dimensions t, t + 256, ... (coalesced row reads);
// partials [blocks, dim] reduced by sq_quantizer_kernel (min / max are exact in any order)
constexpr int kMinMaxBlocks = 256;
__global__ __launch_bounds__(256) void sq_minmax_partial_kernel(const float* __restrict__ x, int64_t n, uint32_t dim,
                                                                float* __restrict__ pmin, float* __restrict__ pmax)
{
  const int64_t per = (n + gridDim.x - 1) / gridDim.x;
  const int64_t r0 = (int64_t)blockIdx.x * per, r1 = min(n, r0 + per);
  for (uint32_t d = threadIdx.x; d < dim; d += blockDim.x) {
    float lo = FLT_MAX, hi = -FLT_MAX;
    for (int64_t r = r0; r < r1; ++r) {
      const float v = x[(size_t)r * dim + d];
      lo = fminf(lo, v);
      hi = fmaxf(hi, v);
    }
    pmin[(size_t)blockIdx.x * dim + d] = lo;
    pmax[(size_t)blockIdx.x * dim + d] = hi;
  }
}

// ivf_sq_build.cuh: margin = 5 % of the range on both sides; 255 steps over the widened range; empty range: step 1
__global__ void sq_quantizer_kernel(const float* __restrict__ pmin, const float* __restrict__ pmax, int blocks, uint32_t dim,
                                    float* __restrict__ vmin, float* __restrict__ delta)
{
  const uint32_t d = blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= dim) return;
  float lo = FLT_MAX, hi = -FLT_MAX;
  for (int b = 0; b < blocks; ++b) {
    lo = fminf(lo, pmin[(size_t)b * dim + d]);
    hi = fmaxf(hi, pmax[(size_t)b * dim + d]);
  }
  const float range  = hi - lo;
  const float margin = range * 0.05f;
  delta[d] = range > 0.0f ? (range + 2.0f * margin) / 255.0f : 1.0f;
  vmin[d]  = lo - margin;
}

// ------------------------------------------------------------------ encoding (extend)
struct sq_pack_args {
  const void* src;           // rows [*, dim] of T
  const uint32_t* perm;      // new-row ids sorted by (list, row)
  const uint32_t* labels;
  const uint32_t* new_off;
  const uint32_t* old_sizes;
  const uint32_t* list_off;
  const int64_t* new_ids;
  const float* centers;
  const float* vmin;
  const float* delta;
  int64_t id_base, j0, batch;
  int src_is_batch;          // 1: src holds rows j0.. in sorted order (host staging); 0: src is the full device array
  uint32_t dim, n_chunks;
  uint8_t* data;
  int64_t* indices;
};

// code = clamp(round((x - c - vmin) / delta), 0, 255): fp32 subtraction, correctly rounded division, half away from zero
__device__ inline uint8_t sq_encode(float x, float c, float vmin, float delta)
{
  const float val  = x - c;
  const float code = roundf((val - vmin) / delta);
  return (uint8_t)fminf(fmaxf(code, 0.0f), 255.0f);
}

// one thread per (sorted row, chunk of 16 dimensions): 16 codes -> one 16-byte store at the row's slot
template <typename T>
__global__ void sq_pack_kernel(sq_pack_args a)
{
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= a.batch * a.n_chunks) return;
  const int64_t jb  = t / a.n_chunks;
  const uint32_t ch = (uint32_t)(t % a.n_chunks);
  const int64_t j   = a.j0 + jb;
  const uint32_t row = a.perm[j];
  const uint32_t L   = a.labels[row];
  const int64_t fr   = (int64_t)a.list_off[L] + a.old_sizes[L] + (j - (int64_t)a.new_off[L]);
  const T* src       = static_cast<const T*>(a.src) + (a.src_is_batch ? jb : (int64_t)row) * a.dim;
  const float* c     = a.centers + (size_t)L * a.dim;
  alignas(16) uint8_t codes[16];
#pragma unroll
  for (uint32_t e = 0; e < 16; ++e) {
    const uint32_t d = ch * 16 + e;
    codes[e]         = d < a.dim ? sq_encode(to_float(src[d]), c[d], a.vmin[d], a.delta[d]) : (uint8_t)0;
  }
  const size_t addr = (((size_t)(fr >> 6) * a.n_chunks + ch) * 64 + (size_t)(fr & 63)) * 16;
  *reinterpret_cast<uint4*>(a.data + addr) = *reinterpret_cast<const uint4*>(codes);
  if (ch == 0) a.indices[fr] = a.new_ids ? a.new_ids[row] : a.id_base + (int64_t)row;
}

// ------------------------------------------------------------------ search
// per-dimension step (padded dims: 1) and, for dot products, aux[L][d] = c_d + vmin_d of every list (padded dims: 0).
// With a zero query term and code 0 a padded dimension adds exactly nothing to any score.
__global__ void sq_search_terms_kernel(const float* __restrict__ centers, const float* __restrict__ vmin,
                                       const float* __restrict__ delta, uint32_t n_lists, uint32_t dim, uint32_t dim_pad,
                                       int with_aux, float* __restrict__ delta_pad, float* __restrict__ aux)
{
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < dim_pad) delta_pad[t] = t < dim ? delta[t] : 1.0f;
  if (!with_aux || t >= (int64_t)n_lists * dim_pad) return;
  const uint32_t L = (uint32_t)(t / dim_pad), d = (uint32_t)(t % dim_pad);
  aux[t] = d < dim ? centers[(size_t)L * dim + d] + vmin[d] : 0.0f;
}

// Query terms of every work item, [dim_pad][QPB] fp32 + one row of |q| (cosine). L2: (q_d - vmin_d) - c_d of the item's list;
// dot products: q_d. Queries are the batch's fp32 copy (qf).
__global__ void sq_query_tiles_kernel(const work_item* __restrict__ items, const uint32_t* __restrict__ n_items,
                                      const uint32_t* __restrict__ sorted_pairs, const float* __restrict__ qf,
                                      const float* __restrict__ qnorm, const float* __restrict__ centers,
                                      const float* __restrict__ vmin, uint32_t n_probes, uint32_t n_lists, uint32_t dim,
                                      uint32_t dim_pad, int is_l2, float* __restrict__ tiles)
{
  constexpr int QPB = kSqQPB;
  const uint32_t w = blockIdx.x;
  if (w >= *n_items) return;
  const work_item item = items[w];
  const uint32_t L     = item.list >= n_lists ? item.list - n_lists : item.list;
  __shared__ uint32_t qid[QPB];
  if (threadIdx.x < QPB)
    qid[threadIdx.x] = threadIdx.x < item.count ? sorted_pairs[item.first + threadIdx.x] / n_probes : 0xffffffffu;
  __syncthreads();
  float* out = tiles + (size_t)w * (dim_pad + 1) * QPB;
  for (uint32_t t = threadIdx.x; t < dim_pad * QPB; t += blockDim.x) {
    const uint32_t d = t / QPB, j = t % QPB;
    float v = 0.f;
    if (qid[j] != 0xffffffffu && d < dim) {
      v = qf[(size_t)qid[j] * dim + d];
      if (is_l2) v = (v - vmin[d]) - centers[(size_t)L * dim + d];
    }
    out[t] = v;
  }
  if (threadIdx.x < QPB)
    out[(size_t)dim_pad * QPB + threadIdx.x] = (qnorm != nullptr && qid[threadIdx.x] != 0xffffffffu) ? qnorm[qid[threadIdx.x]] : 0.f;
}

struct sq_scan_args : list_scan_args {
  const float* delta_pad;  // [dim_pad]
  const float* aux;        // [n_lists, dim_pad] (dot products)
};

// METRIC 0: L2 (both variants), 1: inner product, 2: cosine. ALL: the non-fused path (every score written out).
// Per (pair, dim): L2 diff = fma(-code, delta_d, qt_d), acc = fma(diff, diff, acc); dot products v = fma(code, delta_d, aux_d)
// once per (row, dim), acc = fma(q_d, v, acc) per pair (cosine: vn = fma(v, v, vn) once per row). Scores: smaller is better
// (inner product negated; cosine 1 - acc / (|q| sqrt(vn))).
template <int E, int METRIC, bool ALL = false>
__global__ __launch_bounds__(kSqThreads) void ivf_sq_scan_kernel(sq_scan_args a)
{
  constexpr int QPB = kSqQPB;
  constexpr bool IP = METRIC != 0;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  list_scan_item s;
  if (!list_scan_begin<QPB, kSqWaves>(a, smem, s)) return;
  const uint32_t dim_pad = a.n_chunks * 16;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  // wave-uniform pointers: scalar loads
  const float* __restrict__ qt  = a.qtiles + (size_t)s.w * (dim_pad + 1) * QPB;
  const float* __restrict__ dl  = a.delta_pad;
  const float* __restrict__ aux = IP ? a.aux + (size_t)s.L * dim_pad : nullptr;

  list_scan_tops<QPB, E> tops;
  tops.init();
  const size_t g0       = (size_t)(s.base_row >> 6);
  const uint4* data16   = reinterpret_cast<const uint4*>(a.data);
  const uint32_t n_tile = (s.len + 63) / 64;

  for (uint32_t tile = wave; tile < n_tile; tile += kSqWaves) {
    const uint32_t tile0 = tile * 64;
    const bool valid     = tile0 + lane < s.len;
    f32x2_t accv[QPB / 2];
#pragma unroll
    for (int j = 0; j < QPB / 2; ++j) accv[j] = f32x2_t{0.f, 0.f};
    float vn = 0.f;  // cosine: |v|^2 of this lane's decoded row
    const uint4* cp = data16 + ((g0 + tile) * a.n_chunks) * 64 + lane;
    float bf[QPB];  // L2 early stop: the k-th bounds at the start of the tile (they only decrease) - as in ivf_flat.hip
#pragma unroll
    for (int j = 0; j < QPB; ++j) {
      const uint32_t kk = __builtin_amdgcn_readfirstlane(s.kthb[j]);
      bf[j] = (IP || j >= (int)s.item.count) ? -INFINITY : (kk >= 0xff800000u ? INFINITY : key_to_float(kk));
    }
    auto chunk_step = [&](const uint4& cw, const uint32_t ch) {
      const uint32_t words[4] = {cw.x, cw.y, cw.z, cw.w};
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const uint32_t d = ch * 16 + (uint32_t)e;
        const float x    = (float)((words[e >> 2] >> (8 * (e & 3))) & 0xffu);  // v_cvt_f32_ubyteN
        const float* qr  = qt + (size_t)d * QPB;
        const f32x2_t qv[QPB / 2] = {f32x2_t{qr[0], qr[1]}, f32x2_t{qr[2], qr[3]}, f32x2_t{qr[4], qr[5]}, f32x2_t{qr[6], qr[7]}};
        const float dd = dl[d];
        if constexpr (!IP) {
          const f32x2_t nx = f32x2_t{-x, -x}, dv = f32x2_t{dd, dd};
#pragma unroll
          for (int j = 0; j < QPB / 2; ++j) {
            const f32x2_t t = __builtin_elementwise_fma(nx, dv, qv[j]);
            accv[j]         = __builtin_elementwise_fma(t, t, accv[j]);
          }
        } else {
          const float y    = __fmaf_rn(x, dd, aux[d]);
          const f32x2_t yy = f32x2_t{y, y};
          if (METRIC == 2) vn = __fmaf_rn(y, y, vn);
#pragma unroll
          for (int j = 0; j < QPB / 2; ++j) accv[j] = __builtin_elementwise_fma(qv[j], yy, accv[j]);
        }
      }
    };
    if constexpr (IP) {
      for (uint32_t ch0 = 0; ch0 < a.n_chunks; ch0 += kSqStop) {
        uint4 cws[kSqStop];  // padded rows of a tile are zero-filled: always readable
#pragma unroll
        for (int c = 0; c < kSqStop; ++c) cws[c] = cp[(size_t)min(ch0 + (uint32_t)c, a.n_chunks - 1u) * 64];
        keep_loads_together(cws);
#pragma unroll
        for (int c = 0; c < kSqStop; ++c) {
          const uint32_t ch = ch0 + (uint32_t)c;
          if (ch >= a.n_chunks) break;  // wave-uniform
          chunk_step(cws[c], ch);
        }
      }
    } else {
      for (uint32_t ch = 0; ch < a.n_chunks; ++ch) {
        if (!ALL && ch > 0) {
          // partial sums of squares only grow: once every row of the tile is above every query's bound, stop (tested after
          // every chunk: a chunk holds 16 dimensions here, four times IVF-Flat's fp32 chunk)
          bool below = false;
#pragma unroll
          for (int j = 0; j < QPB; ++j) below = below || (accv[j >> 1][j & 1] <= bf[j]);
          if (__ballot(valid && below) == 0ull) break;  // wave-uniform
        }
        chunk_step(cp[(size_t)ch * 64], ch);
      }
    }
    float acc[QPB];
#pragma unroll
    for (int j = 0; j < QPB; ++j) acc[j] = accv[j >> 1][j & 1];
    if (METRIC == 2) {
      const float xn = sqrtf(vn);
#pragma unroll
      for (int j = 0; j < QPB; ++j) {
        const float denom = qt[(size_t)dim_pad * QPB + j] * xn;
        acc[j]            = denom > 0.0f ? 1.0f - acc[j] / denom : 0.0f;
      }
    }
#pragma unroll
    for (int j = 0; j < QPB; ++j) {
      if (j >= (int)s.item.count) break;
      list_scan_offer<QPB, E, ALL>(a, s, j, METRIC == 1 ? -acc[j] : acc[j], tile0, lane, tops);  // smaller is better
    }
  }

  if constexpr (!ALL) list_scan_merge<QPB, kSqWaves, E>(a, s, smem, tops);
}

__global__ void sq_postprocess_kernel(const uint32_t* __restrict__ pos, const float* __restrict__ d_in, int64_t n,
                                      const int64_t* __restrict__ indices, int metric, int64_t* __restrict__ neighbors,
                                      float* __restrict__ distances)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t p = pos[i];
  neighbors[i]     = p == 0xffffffffu ? INT64_MAX : indices[p];
  float d          = d_in[i];
  if (p == 0xffffffffu) d = FLT_MAX;
  else if (metric == M_InnerProduct) d = -d;
  else if (metric == M_L2SqrtExpanded) d = sqrtf(d);
  distances[i] = d;
}

// one list's codes row-major [n_rows, dim] (test export)
__global__ void sq_unpack_list_kernel(const uint8_t* __restrict__ data, uint32_t n_chunks, uint32_t dim, int64_t flat_row0,
                                      uint32_t n_rows, uint8_t* __restrict__ out)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)n_rows * dim) return;
  const int64_t fr = flat_row0 + i / dim;
  const uint32_t d = (uint32_t)(i % dim);
  out[i] = data[(((size_t)(fr >> 6) * n_chunks + d / 16) * 64 + (size_t)(fr & 63)) * 16 + d % 16];
}

void launch_sq_scan(resources& res, const sq_scan_args& a, int metric_kind, size_t smem, unsigned grid, bool big_k)
{
  profile_begin(res, "ivf_sq_scan_kernel");
  list_scan_dispatch(a.all_scores != nullptr, big_k, metric_kind, [&](auto e, auto metric, auto all) {
    list_scan_launch(res, ivf_sq_scan_kernel<decltype(e)::value, decltype(metric)::value, decltype(all)::value>, kSqThreads, a, smem,
                     grid);
  });
  profile_end(res, "ivf_sq_scan_kernel");
  HIP_TRY(hipGetLastError());
}

std::unique_ptr<ivf_sq_index> sq_empty_index(resources& res, int metric, uint32_t n_lists, uint32_t dim, bool cma)
{
  auto idx      = std::make_unique<ivf_sq_index>();
  idx->metric   = metric;
  idx->n_lists  = n_lists;
  idx->dim      = dim;
  idx->n_chunks = (dim + 15) / 16;
  idx->conservative_memory_allocation = cma;
  idx->centers      = dev_buf<float>::persistent((size_t)n_lists * dim);
  idx->vmin         = dev_buf<float>::persistent(dim);
  idx->delta        = dev_buf<float>::persistent(dim);
  idx->list_sizes   = dev_buf<uint32_t>::persistent(n_lists);
  idx->list_offsets = dev_buf<uint32_t>::persistent(n_lists + 1);
  HIP_TRY(hipMemsetAsync(idx->list_sizes.data(), 0, idx->list_sizes.bytes(), res.stream));
  HIP_TRY(hipMemsetAsync(idx->list_offsets.data(), 0, idx->list_offsets.bytes(), res.stream));
  idx->h_list_sizes.assign(n_lists, 0);
  idx->h_list_offsets.assign(n_lists + 1, 0);
  return idx;
}

}  // namespace

void ivf_sq_extend(resources& res, ivf_sq_index& idx, const void* data, elem_t et, int64_t n_new, bool is_host,
                   const int64_t* new_ids, bool ids_on_host)
{
  if (n_new == 0) return;
  CUVS_EXPECTS(et == elem_t::f32 || et == elem_t::f16, "ivf_sq::extend: vectors must be float32 or float16");
  CUVS_EXPECTS(new_ids != nullptr || idx.size == 0, "You must pass data indices when the index is non-empty.");
  CUVS_EXPECTS(idx.size + n_new < (int64_t(1) << 32) - 64 * (int64_t)idx.n_lists, "index too large for 32-bit row offsets");
  dev_buf<uint32_t> labels(res, n_new);
  ivf_assign_lists(res, idx.metric, idx.centers.data(), idx.center_norms.data(), idx.n_lists, idx.dim, data, et, is_host, n_new,
                   labels.data());
  ivf_lists_grow(res, idx, labels.data(), data, (size_t)idx.dim * elem_size(et), n_new, is_host, new_ids, ids_on_host,
                 [&](const ivf_pack_dest& d, int64_t j0, int64_t batch, const void* src, int src_is_batch) {
                   sq_pack_args a;
                   a.src = src; a.perm = d.perm; a.labels = d.labels; a.new_off = d.new_off; a.old_sizes = d.old_sizes;
                   a.list_off = d.list_off; a.new_ids = d.new_ids; a.id_base = d.id_base; a.j0 = j0; a.batch = batch;
                   a.src_is_batch = src_is_batch; a.centers = idx.centers.data(); a.vmin = idx.vmin.data();
                   a.delta = idx.delta.data(); a.dim = idx.dim; a.n_chunks = idx.n_chunks; a.data = d.data; a.indices = d.indices;
                   const int64_t work = batch * idx.n_chunks;
                   if (et == elem_t::f32) hipLaunchKernelGGL(sq_pack_kernel<float>, dim3(grid_blocks(work, 256)), dim3(256), 0, res.stream, a);
                   else                   hipLaunchKernelGGL(sq_pack_kernel<__half>, dim3(grid_blocks(work, 256)), dim3(256), 0, res.stream, a);
                 });
  ivf_set_center_norms(res, idx.metric, idx.centers.data(), idx.n_lists, idx.dim, idx.center_norms, idx.center_norms_sqrt);
  sync(res);
}

std::unique_ptr<ivf_sq_index> ivf_sq_build(resources& res, const cuvsIvfSqIndexParams& p, const void* data, elem_t et,
                                           int64_t n, int64_t dim, bool is_host)
{
  CUVS_EXPECTS(et == elem_t::f32 || et == elem_t::f16, "ivf_sq::build: dataset must be float32 or float16");
  CUVS_EXPECTS(n > 0 && dim > 0, "empty dataset");
  CUVS_EXPECTS(p.n_lists > 0 && n >= p.n_lists, "number of rows can't be less than n_lists");
  CUVS_EXPECTS(p.max_train_points_per_cluster > 0, "max_train_points_per_cluster must be > 0");
  const int metric = (int)p.metric;
  CUVS_EXPECTS(sq_metric_ok(metric), "ivf_sq: unsupported metric %d (L2Expanded, L2SqrtExpanded, InnerProduct, CosineExpanded)",
               metric);
  CUVS_EXPECTS(metric != M_CosineExpanded || dim > 1, "Cosine metric requires more than one dim");
  CUVS_EXPECTS(dim < (int64_t(1) << 24), "ivf_sq: dim too large");
  auto idx   = sq_empty_index(res, metric, p.n_lists, (uint32_t)dim, p.conservative_memory_allocation);
  idx->dtype = et;
  // training sample: min(n, n_lists * max_train_points_per_cluster) distinct rows, chosen by a seeded shuffle (all rows
  // when the dataset is no larger), gathered in ascending row order
  const int64_t n_train = std::min<int64_t>(n, (int64_t)p.n_lists * p.max_train_points_per_cluster);
  const std::vector<uint32_t> pick = pick_train_rows(n, n_train);
  dev_buf<float> trainset(res, (size_t)n_train * dim);
  {
    dev_buf<uint32_t> ids(res, n_train);
    copy_async(res, ids.data(), pick.data(), (size_t)n_train * sizeof(uint32_t));
    load_gather_as_float(res, data, et, is_host, dim, ids.data(), n_train, trainset.data());
    sync(res);
  }
  {
    // k-means on the sample (cosine: on unit-length copies), then the sample's labels with the index metric
    dev_buf<float> fit(res, (size_t)n_train * dim);
    HIP_TRY(hipMemcpyAsync(fit.data(), trainset.data(), trainset.bytes(), hipMemcpyDeviceToDevice, res.stream));
    if (metric == M_CosineExpanded) normalize_rows(res, fit.data(), n_train, dim);
    kmeans_params kp;
    kp.n_iters       = (int)p.kmeans_n_iters;
    kp.inner_product = metric == M_InnerProduct;
    kmeans_balanced_fit(res, fit.data(), n_train, dim, (int)p.n_lists, kp, idx->centers.data());
    ivf_set_center_norms(res, metric, idx->centers.data(), idx->n_lists, idx->dim, idx->center_norms, idx->center_norms_sqrt);
    HIP_TRY(hipMemcpyAsync(fit.data(), trainset.data(), trainset.bytes(), hipMemcpyDeviceToDevice, res.stream));
    dev_buf<uint32_t> labels(res, n_train);
    ivf_assign_lists(res, metric, idx->centers.data(), idx->center_norms.data(), idx->n_lists, idx->dim, fit.data(), n_train,
                     labels.data());
    // residuals -> per-dimension range -> quantizer
    hipLaunchKernelGGL(sq_residuals_kernel, dim3(grid_blocks(n_train * dim, 256)), dim3(256), 0, res.stream, trainset.data(),
                       idx->centers.data(), labels.data(), n_train, (uint32_t)dim, et == elem_t::f16 ? 1 : 0);
    dev_buf<float> pmin(res, (size_t)kMinMaxBlocks * dim), pmax(res, (size_t)kMinMaxBlocks * dim);
    hipLaunchKernelGGL(sq_minmax_partial_kernel, dim3(kMinMaxBlocks), dim3(256), 0, res.stream, trainset.data(), n_train,
                       (uint32_t)dim, pmin.data(), pmax.data());
    hipLaunchKernelGGL(sq_quantizer_kernel, dim3(grid_blocks(dim, 256)), dim3(256), 0, res.stream, pmin.data(), pmax.data(),
                       kMinMaxBlocks, (uint32_t)dim, idx->vmin.data(), idx->delta.data());
    HIP_TRY(hipGetLastError());
    sync(res);
  }
  trainset.release();
  if (p.add_data_on_build) ivf_sq_extend(res, *idx, data, et, n, is_host, nullptr, false);
  sync(res);
  return idx;
}

void ivf_sq_search(resources& res, const ivf_sq_index& idx, uint32_t n_probes_in, const void* queries, elem_t et,
                   int64_t n_queries, int k, int64_t* neighbors, float* distances, const uint32_t* filter_bits)
{
  CUVS_EXPECTS(k > 0, "ivf_sq::search: k must be positive");
  CUVS_EXPECTS(n_probes_in > 0, "n_probes must be positive");
  CUVS_EXPECTS(et == elem_t::f32 || et == elem_t::f16, "ivf_sq::search: queries must be float32 or float16");
  if (n_queries == 0) return;
  const uint32_t n_probes = std::min<uint32_t>(n_probes_in, idx.n_lists);
  const int qpb           = kSqQPB;
  const bool large_k      = k > 256;  // beyond the register top lists: every score written, then select_k
  const bool big_k        = k > 64 && !large_k;
  const int k_scan        = large_k ? 1 : k;
  const uint32_t dim_pad  = idx.n_chunks * 16;
  const int metric_kind   = idx.metric == M_InnerProduct ? 1 : idx.metric == M_CosineExpanded ? 2 : 0;
  const bool cosm = idx.metric == M_CosineExpanded;
  const size_t smem      = list_scan_smem_bytes(qpb, kSqWaves, (uint32_t)k_scan);
  const size_t scores_ld = large_k ? largest_lists_total(idx.h_list_sizes, n_probes) : 0;
  int64_t max_batch = 1 << 15;
  {
    int64_t per_q = (int64_t)idx.n_lists * 4 + (int64_t)n_probes * k_scan * 8 + idx.dim * 4 +
                    ((int64_t)n_probes / qpb + 1) * (dim_pad + 1) * qpb * 4;
    if (large_k) per_q += (int64_t)scores_ld * 8 + (int64_t)k * 12;
    per_q += round_up((int64_t)idx.n_lists, 128) * 4 + round_up((int64_t)idx.n_lists, 128) / 4;
    max_batch = balanced_batch(n_queries, std::min(max_batch, std::max<int64_t>(1, (int64_t)res.ivf_batch_limit / per_q)));
  }
  const int64_t bs     = std::min<int64_t>(max_batch, n_queries);
  const int64_t np_max = bs * n_probes;
  // two-phase schedule (ivf_common.hpp): the nearest probe of every query first leaves tight bounds for the L2 early stop
  const uint32_t head     = (n_probes > 8 && metric_kind == 0 && !large_k) ? 1u : 0u;
  const uint32_t n_labels = head > 0 ? 2 * idx.n_lists : idx.n_lists;
  dev_buf<float> qf(res, (size_t)bs * idx.dim), qn(res, bs), pd(res, (size_t)np_max);
  dev_buf<float> dist;
  dev_buf<uint32_t> probes(res, np_max), sorted_pairs(res, np_max), pair_off(res, n_labels + 1), item_off(res, n_labels + 1),
    cand_i(res, large_k ? (size_t)bs * scores_ld : (size_t)np_max * k), top_i(res, (size_t)bs * k), query_kth(res, bs),
    pair_seg(res, large_k ? (size_t)np_max : 0), phase_labels(res, head > 0 ? (size_t)np_max : 0);
  const size_t max_items = (size_t)(np_max / qpb + n_labels + 1);
  dev_buf<work_item> items(res, max_items);
  dev_buf<float> qtiles(res, max_items * (dim_pad + 1) * qpb);
  dev_buf<float> cand_d(res, large_k ? (size_t)bs * scores_ld : (size_t)np_max * k), top_d(res, (size_t)bs * k);
  dev_buf<float> delta_pad(res, dim_pad), aux(res, metric_kind != 0 ? (size_t)idx.n_lists * dim_pad : 0);
  hipLaunchKernelGGL(sq_search_terms_kernel, dim3(grid_blocks(std::max<int64_t>(dim_pad, (int64_t)idx.n_lists * dim_pad), 256)),
                     dim3(256), 0, res.stream, idx.centers.data(), idx.vmin.data(), idx.delta.data(), idx.n_lists, idx.dim,
                     dim_pad, metric_kind != 0 ? 1 : 0, delta_pad.data(), aux.data());
  const size_t esz = elem_size(et);

  for (int64_t q0 = 0; q0 < n_queries; q0 += max_batch) {
    const int64_t nq      = std::min(max_batch, n_queries - q0);
    const int64_t n_pairs = nq * n_probes;
    load_range_as_float(res, queries, et, false, idx.dim, q0, nq, qf.data());
    (void)esz;
    coarse_search(res, idx.centers.data(), idx.dim, idx.n_lists, idx.dim, idx.center_norms.data(), idx.center_norms_sqrt.data(),
                  idx.metric, qf.data(), nq, n_probes, bs, qn.data(), dist, pd.data(), probes.data());
    const uint32_t* labels = probes.data();
    if (head > 0) {
      hipLaunchKernelGGL(phase_labels_kernel, dim3(grid_blocks(n_pairs, 256)), dim3(256), 0, res.stream, probes.data(), n_pairs,
                         n_probes, head, idx.n_lists, phase_labels.data());
      labels = phase_labels.data();
    }
    build_work_items(res, labels, n_pairs, n_labels, qpb, sorted_pairs.data(), pair_off.data(), item_off.data(), items.data());
    HIP_TRY(hipMemsetAsync(query_kth.data(), 0xff, (size_t)nq * sizeof(uint32_t), res.stream));
    if (large_k) {
      HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(cand_d.data()), 0x7f7fffff, (size_t)nq * scores_ld, res.stream));
      HIP_TRY(hipMemsetAsync(cand_i.data(), 0xff, (size_t)nq * scores_ld * sizeof(uint32_t), res.stream));
      hipLaunchKernelGGL(pair_segments_kernel, dim3(grid_blocks(nq, 256)), dim3(256), 0, res.stream, probes.data(),
                         idx.list_sizes.data(), nq, n_probes, pair_seg.data());
    }
    // (cosine: qn holds |q| from the coarse search's row_norms)
    hipLaunchKernelGGL(sq_query_tiles_kernel, dim3((unsigned)(n_pairs / qpb + n_labels + 1)), dim3(256), 0, res.stream,
                       items.data(), item_off.data() + n_labels, sorted_pairs.data(), qf.data(), cosm ? qn.data() : nullptr,
                       idx.centers.data(), idx.vmin.data(), n_probes, idx.n_lists, idx.dim, dim_pad, metric_kind == 0 ? 1 : 0,
                       qtiles.data());
    sq_scan_args a{};
    a.items = items.data(); a.n_lists = idx.n_lists; a.sorted_pairs = sorted_pairs.data(); a.qtiles = qtiles.data();
    a.delta_pad = delta_pad.data(); a.aux = aux.data(); a.data = idx.data.data(); a.list_offsets = idx.list_offsets.data();
    a.list_sizes = idx.list_sizes.data(); a.out_d = cand_d.data(); a.out_i = cand_i.data(); a.query_kth = query_kth.data();
    a.filter_bits = filter_bits; a.indices = idx.indices.data(); a.n_probes = n_probes; a.n_chunks = idx.n_chunks;
    a.k = (uint32_t)k_scan; a.all_scores = large_k ? cand_d.data() : nullptr; a.all_rows = cand_i.data();
    a.pair_seg = pair_seg.data(); a.scores_ld = scores_ld;
    // grids are upper bounds of the (device-side) item counts of each phase; surplus workgroups exit at once
    if (head > 0) {
      a.item_begin = nullptr; a.item_end = item_off.data() + idx.n_lists;
      launch_sq_scan(res, a, metric_kind, smem, (unsigned)(nq * head / qpb + idx.n_lists + 1), big_k);
      a.item_begin = item_off.data() + idx.n_lists; a.item_end = item_off.data() + 2 * idx.n_lists;
      launch_sq_scan(res, a, metric_kind, smem, (unsigned)(nq * (n_probes - head) / qpb + idx.n_lists + 1), big_k);
    } else {
      a.item_begin = nullptr; a.item_end = item_off.data() + idx.n_lists;
      launch_sq_scan(res, a, metric_kind, smem, (unsigned)(n_pairs / qpb + idx.n_lists + 1), big_k);
    }
    if (!large_k)
      select_k<uint32_t, uint32_t>(res, cand_d.data(), cand_i.data(), nq, (int64_t)n_probes * k, (int64_t)n_probes * k, k,
                                   top_d.data(), top_i.data(), true);
    else
      select_k<uint32_t, uint32_t>(res, cand_d.data(), cand_i.data(), nq, (int64_t)scores_ld, (int64_t)scores_ld, k, top_d.data(),
                                   top_i.data(), true);
    hipLaunchKernelGGL(sq_postprocess_kernel, dim3(grid_blocks(nq * k, 256)), dim3(256), 0, res.stream, top_i.data(), top_d.data(),
                       nq * k, idx.indices.data(), idx.metric, neighbors + q0 * k, distances + q0 * k);
  }
  HIP_TRY(hipGetLastError());
}

}  // namespace cuvs_amd

using namespace cuvs_amd;

namespace {
ivf_sq_index& get_sq(cuvsIvfSqIndex_t index)
{
  CUVS_EXPECTS(index != nullptr && index->addr != 0, "IVF-SQ index is not built");
  return *reinterpret_cast<ivf_sq_index*>(index->addr);
}

const uint32_t* sq_filter_bits(const cuvsFilter& filter)
{
  if (filter.type == NO_FILTER) return nullptr;
  CUVS_EXPECTS(filter.type == BITSET, "Unsupported filter type: BITMAP");
  CUVS_EXPECTS(filter.addr != 0, "filter tensor is null");
  auto& ft = reinterpret_cast<DLManagedTensor*>(filter.addr)->dl_tensor;
  CUVS_EXPECTS(dtype_is(ft.dtype, kDLUInt, 32) && is_device_accessible(ft), "filter must be a device uint32 tensor");
  return static_cast<const uint32_t*>(dl_data(ft));
}

bool sq_input_dtype_ok(const DLDataType& d) { return d.code == kDLFloat && (d.bits == 32 || d.bits == 16); }
}  // namespace

extern "C" {

cuvsError_t cuvsIvfSqIndexParamsCreate(cuvsIvfSqIndexParams_t* params)
{
  return (cuvsError_t)translate_exceptions(
    [=] { *params = new cuvsIvfSqIndexParams{L2Expanded, 2.0f, true, 1024, 20, 256, false}; });
}
cuvsError_t cuvsIvfSqIndexParamsDestroy(cuvsIvfSqIndexParams_t params)
{
  return (cuvsError_t)translate_exceptions([=] { delete params; });
}
cuvsError_t cuvsIvfSqSearchParamsCreate(cuvsIvfSqSearchParams_t* params)
{
  return (cuvsError_t)translate_exceptions([=] { *params = new cuvsIvfSqSearchParams{20}; });
}
cuvsError_t cuvsIvfSqSearchParamsDestroy(cuvsIvfSqSearchParams_t params)
{
  return (cuvsError_t)translate_exceptions([=] { delete params; });
}
cuvsError_t cuvsIvfSqIndexCreate(cuvsIvfSqIndex_t* index)
{
  return (cuvsError_t)translate_exceptions([=] { *index = new cuvsIvfSqIndex{0, DLDataType{0, 0, 0}}; });
}
cuvsError_t cuvsIvfSqIndexDestroy(cuvsIvfSqIndex_t index)
{
  return (cuvsError_t)translate_exceptions([=] {
    if (!index) return;
    delete reinterpret_cast<ivf_sq_index*>(index->addr);
    delete index;
  });
}
cuvsError_t cuvsIvfSqIndexGetNLists(cuvsIvfSqIndex_t index, int64_t* n_lists)
{
  return (cuvsError_t)translate_exceptions([=] { *n_lists = get_sq(index).n_lists; });
}
cuvsError_t cuvsIvfSqIndexGetDim(cuvsIvfSqIndex_t index, int64_t* dim)
{
  return (cuvsError_t)translate_exceptions([=] { *dim = get_sq(index).dim; });
}
cuvsError_t cuvsIvfSqIndexGetSize(cuvsIvfSqIndex_t index, int64_t* size)
{
  return (cuvsError_t)translate_exceptions([=] { *size = get_sq(index).size; });
}
cuvsError_t cuvsIvfSqIndexGetCenters(cuvsIvfSqIndex_t index, DLManagedTensor* centers)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& idx = get_sq(index);
    fill_dl_view(centers, idx.centers.data(), DLDataType{kDLFloat, 32, 1}, idx.n_lists, idx.dim, 2, 0);
  });
}

cuvsError_t cuvsIvfSqBuild(cuvsResources_t res_h, cuvsIvfSqIndexParams_t params, DLManagedTensor* dataset_tensor,
                           cuvsIvfSqIndex_t index)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& res = *as_res(res_h);
    CUVS_EXPECTS(params && dataset_tensor && index, "null argument");
    auto& ds = dataset_tensor->dl_tensor;
    CUVS_EXPECTS(sq_input_dtype_ok(ds.dtype), "Unsupported dataset DLtensor dtype: %d and bits: %d", (int)ds.dtype.code,
                 (int)ds.dtype.bits);
    CUVS_EXPECTS(ds.ndim == 2 && is_c_contiguous(ds), "dataset must be a row-major matrix");
    auto idx = ivf_sq_build(res, *params, dl_data(ds), elem_of(ds.dtype), ds.shape[0], ds.shape[1], !is_device_accessible(ds));
    delete reinterpret_cast<ivf_sq_index*>(index->addr);
    index->addr  = reinterpret_cast<uintptr_t>(idx.release());
    index->dtype = DLDataType{ds.dtype.code, ds.dtype.bits, 1};
  });
}

cuvsError_t cuvsIvfSqSearch(cuvsResources_t res_h, cuvsIvfSqSearchParams_t params, cuvsIvfSqIndex_t index_c,
                            DLManagedTensor* queries_tensor, DLManagedTensor* neighbors_tensor,
                            DLManagedTensor* distances_tensor, cuvsFilter filter)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& res = *as_res(res_h);
    auto& idx = get_sq(index_c);
    CUVS_EXPECTS(params && queries_tensor && neighbors_tensor && distances_tensor, "null argument");
    const uint32_t* bits = sq_filter_bits(filter);
    auto& queries   = queries_tensor->dl_tensor;
    auto& neighbors = neighbors_tensor->dl_tensor;
    auto& distances = distances_tensor->dl_tensor;
    CUVS_EXPECTS(is_device_accessible(queries), "queries should have device compatible memory");
    CUVS_EXPECTS(is_device_accessible(neighbors), "neighbors should have device compatible memory");
    CUVS_EXPECTS(is_device_accessible(distances), "distances should have device compatible memory");
    CUVS_EXPECTS(dtype_is(neighbors.dtype, kDLInt, 64), "neighbors should be of type int64_t");
    CUVS_EXPECTS(dtype_is(distances.dtype, kDLFloat, 32), "distances should be of type float32");
    CUVS_EXPECTS(sq_input_dtype_ok(queries.dtype), "Unsupported queries DLtensor dtype: %d and bits: %d",
                 (int)queries.dtype.code, (int)queries.dtype.bits);
    CUVS_EXPECTS(queries.ndim == 2 && neighbors.ndim == 2 && distances.ndim == 2, "tensors must be 2-D");
    CUVS_EXPECTS(is_c_contiguous(queries) && is_c_contiguous(neighbors) && is_c_contiguous(distances),
                 "tensors must be C-contiguous");
    CUVS_EXPECTS(queries.shape[1] == idx.dim, "queries dim %ld != index dim %u", (long)queries.shape[1], idx.dim);
    const int64_t m = queries.shape[0], k = neighbors.shape[1];
    CUVS_EXPECTS(neighbors.shape[0] == m && distances.shape[0] == m && distances.shape[1] == k,
                 "neighbors/distances shape mismatch");
    ivf_sq_search(res, idx, params->n_probes, dl_data(queries), elem_of(queries.dtype), m, (int)k,
                  static_cast<int64_t*>(dl_data(neighbors)), static_cast<float*>(dl_data(distances)), bits);
  });
}

cuvsError_t cuvsIvfSqExtend(cuvsResources_t res_h, DLManagedTensor* new_vectors, DLManagedTensor* new_indices,
                            cuvsIvfSqIndex_t index_c)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& res = *as_res(res_h);
    auto& idx = get_sq(index_c);
    CUVS_EXPECTS(new_vectors != nullptr, "new_vectors is null");
    auto& v = new_vectors->dl_tensor;
    CUVS_EXPECTS(sq_input_dtype_ok(v.dtype), "Unsupported vectors DLtensor dtype: %d and bits: %d", (int)v.dtype.code,
                 (int)v.dtype.bits);
    CUVS_EXPECTS(v.ndim == 2 && is_c_contiguous(v) && v.shape[1] == idx.dim, "new_vectors must be [n, dim] row-major");
    const bool on_device = is_device_accessible(v);
    const int64_t* ids   = nullptr;
    bool ids_host        = false;
    if (new_indices != nullptr) {
      auto& t = new_indices->dl_tensor;
      CUVS_EXPECTS(dtype_is(t.dtype, kDLInt, 64) && t.ndim == 1 && t.shape[0] == v.shape[0], "new_indices must be int64 [n]");
      CUVS_EXPECTS(is_device_accessible(t) == on_device, "extend inputs must both either be on device memory or host memory");
      ids      = static_cast<const int64_t*>(dl_data(t));
      ids_host = !is_device_accessible(t);
    }
    if (index_c->dtype.code == 0 && index_c->dtype.bits == 0) index_c->dtype = DLDataType{v.dtype.code, v.dtype.bits, 1};
    ivf_sq_extend(res, idx, dl_data(v), elem_of(v.dtype), v.shape[0], !on_device, ids, ids_host);
  });
}

}  // extern "C"

namespace {
constexpr int kSqRefVersion = 1;  // ivf_sq_serialize.cuh

// the reference's list record interleave (ivf_sq.hpp: kIndexGroupSize 32, kVecLen 16): byte offset of (row r, dim d) in a
// list record [rows32, dim_pad]
inline size_t ref_sq_offset(uint32_t r, uint32_t d, uint32_t dim_pad)
{
  return (size_t)(r / 32) * 32 * dim_pad + (size_t)(d / 16) * 32 * 16 + (size_t)(r % 32) * 16 + d % 16;
}

// Record sequence: dtype prefix "|u1", version, size, dim, n_lists, metric, conservative_memory_allocation, centers,
// has_norms [, center norms], vmin, delta, list_sizes, then per list: rows32 = roundUp(size, 32) [, codes [rows32, dim_pad]
// in the reference's 32-row interleave, ids [rows32]]. Our lists are stored in 64-row tiles: re-interleaved on the host.
void sq_write_ref(resources& res, const char* filename, const ivf_sq_index& idx)
{
  npy_writer w(filename);
  char prefix[4];
  elem_prefix(elem_t::u8, prefix);
  w.raw(prefix, 4);
  w.scalar<int32_t>(kSqRefVersion);
  w.scalar<int64_t>(idx.size);
  w.scalar<uint32_t>(idx.dim);
  w.scalar<uint32_t>(idx.n_lists);
  w.scalar<int32_t>(idx.metric);
  w.scalar<bool>(idx.conservative_memory_allocation);
  w.device_array(res, 'f', 4, {idx.n_lists, idx.dim}, idx.centers.data());
  const bool has_norms = idx.metric != M_InnerProduct;
  w.scalar<bool>(has_norms);
  if (has_norms)
    w.device_array(res, 'f', 4, {idx.n_lists}, idx.metric == M_CosineExpanded ? idx.center_norms_sqrt.data() : idx.center_norms.data());
  w.device_array(res, 'f', 4, {idx.dim}, idx.vmin.data());
  w.device_array(res, 'f', 4, {idx.dim}, idx.delta.data());
  w.host_array<uint32_t>(idx.h_list_sizes.data(), {idx.n_lists});
  const uint32_t dim_pad = idx.n_chunks * 16;
  std::vector<uint8_t> ours, theirs;
  std::vector<int64_t> ids;
  for (uint32_t L = 0; L < idx.n_lists; ++L) {
    const uint32_t size = idx.h_list_sizes[L], rows32 = (uint32_t)round_up(size, 32);
    w.scalar<uint32_t>(rows32);
    if (rows32 == 0) continue;
    const uint32_t cap = idx.h_list_offsets[L + 1] - idx.h_list_offsets[L];
    ours.resize((size_t)cap * idx.n_chunks * 16);
    ids.assign(rows32, -1);
    copy_async(res, ours.data(), idx.data.data() + (size_t)idx.h_list_offsets[L] * idx.n_chunks * 16, ours.size());
    copy_async(res, ids.data(), idx.indices.data() + idx.h_list_offsets[L], (size_t)size * sizeof(int64_t));
    sync(res);
    theirs.assign((size_t)rows32 * dim_pad, 0);
    for (uint32_t r = 0; r < size; ++r) {
      const uint8_t* row = ours.data() + ((size_t)(r / 64) * idx.n_chunks * 64 + r % 64) * 16;
      for (uint32_t ch = 0; ch < idx.n_chunks; ++ch)
        memcpy(theirs.data() + ref_sq_offset(r, ch * 16, dim_pad), row + (size_t)ch * 64 * 16, 16);
    }
    w.header('u', 1, {rows32, dim_pad});
    w.raw(theirs.data(), theirs.size());
    w.host_array<int64_t>(ids.data(), {rows32});
  }
  w.close();
}

std::unique_ptr<ivf_sq_index> sq_read_ref(resources& res, const char* filename)
{
  npy_reader r(filename);
  char prefix[4];
  r.raw(prefix, 4);
  elem_t code_t;
  CUVS_EXPECTS(parse_elem_prefix(prefix, &code_t) && code_t == elem_t::u8,
               "ivf_sq::deserialize: serialized dtype prefix does not match requested type");
  const int ver = r.scalar<int32_t>();
  CUVS_EXPECTS(ver == kSqRefVersion, "serialization version mismatch, expected %d, got %d ", kSqRefVersion, ver);
  const int64_t size     = r.scalar<int64_t>();
  const uint32_t dim     = r.scalar<uint32_t>();
  const uint32_t n_lists = r.scalar<uint32_t>();
  const int metric       = r.scalar<int32_t>();
  const bool cma         = r.scalar<bool>();
  CUVS_EXPECTS(sq_metric_ok(metric), "ivf_sq::deserialize: invalid metric value %d", metric);
  CUVS_EXPECTS(n_lists <= (1u << 24), "ivf_sq::deserialize: n_lists=%u exceeds maximum %u", n_lists, 1u << 24);
  CUVS_EXPECTS(dim > 0 && n_lists > 0 && dim < (1u << 24), "ivf_sq::deserialize: bad header");
  auto idx  = sq_empty_index(res, metric, n_lists, dim, cma);
  idx->size = size;
  idx->centers = r.device_array<float>(res, (int64_t)n_lists * dim);
  if (r.scalar<bool>()) (void)r.host_array<float>(n_lists);
  // canonical norms (the build's own rounding) rather than the file's
  ivf_set_center_norms(res, idx->metric, idx->centers.data(), idx->n_lists, idx->dim, idx->center_norms, idx->center_norms_sqrt);
  idx->vmin  = r.device_array<float>(res, dim);
  idx->delta = r.device_array<float>(res, dim);
  idx->h_list_sizes = r.host_array<uint32_t>(n_lists);
  int64_t total = 0, live = 0;
  for (uint32_t L = 0; L < n_lists; ++L) {
    idx->h_list_offsets[L] = (uint32_t)total;
    total += round_up(idx->h_list_sizes[L], 64);
    live += idx->h_list_sizes[L];
  }
  CUVS_EXPECTS(total < (int64_t(1) << 32), "ivf_sq::deserialize: index too large");
  CUVS_EXPECTS(live == size, "ivf_sq::deserialize: list sizes (%ld) do not add up to the index size (%ld)", (long)live, (long)size);
  idx->h_list_offsets[n_lists] = (uint32_t)total;
  idx->padded_rows             = total;
  copy_async(res, idx->list_sizes.data(), idx->h_list_sizes.data(), n_lists * sizeof(uint32_t));
  copy_async(res, idx->list_offsets.data(), idx->h_list_offsets.data(), (n_lists + 1) * sizeof(uint32_t));
  idx->data    = dev_buf<uint8_t>::persistent((size_t)total * idx->n_chunks * 16);
  idx->indices = dev_buf<int64_t>::persistent((size_t)total);
  HIP_TRY(hipMemsetAsync(idx->data.data(), 0, idx->data.bytes(), res.stream));
  HIP_TRY(hipMemsetAsync(idx->indices.data(), 0xff, idx->indices.bytes(), res.stream));
  sync(res);
  const uint32_t dim_pad = idx->n_chunks * 16;
  std::vector<uint8_t> ours;
  std::vector<char> theirs;
  for (uint32_t L = 0; L < n_lists; ++L) {
    const uint32_t rows = r.scalar<uint32_t>(), sz = idx->h_list_sizes[L];
    CUVS_EXPECTS(rows >= sz, "ivf_sq::deserialize: list %u holds %u rows, list_sizes says %u", L, rows, sz);
    if (rows == 0) continue;
    r.array(1, (int64_t)rows * dim_pad, theirs);
    std::vector<int64_t> ids = r.host_array<int64_t>(rows);
    if (sz == 0) continue;
    ours.assign((size_t)round_up(sz, 64) * idx->n_chunks * 16, 0);
    for (uint32_t rr = 0; rr < sz; ++rr) {
      uint8_t* row = ours.data() + ((size_t)(rr / 64) * idx->n_chunks * 64 + rr % 64) * 16;
      for (uint32_t ch = 0; ch < idx->n_chunks; ++ch)
        memcpy(row + (size_t)ch * 64 * 16, theirs.data() + ref_sq_offset(rr, ch * 16, dim_pad), 16);
    }
    copy_async(res, idx->data.data() + (size_t)idx->h_list_offsets[L] * idx->n_chunks * 16, ours.data(), ours.size());
    copy_async(res, idx->indices.data() + idx->h_list_offsets[L], ids.data(), (size_t)sz * sizeof(int64_t));
    sync(res);
  }
  return idx;
}
}  // namespace

extern "C" {
cuvsError_t cuvsIvfSqSerialize(cuvsResources_t res_h, const char* filename, cuvsIvfSqIndex_t index)
{
  return (cuvsError_t)translate_exceptions([=] { sq_write_ref(*as_res(res_h), filename, get_sq(index)); });
}
cuvsError_t cuvsIvfSqDeserialize(cuvsResources_t res_h, const char* filename, cuvsIvfSqIndex_t index)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& res = *as_res(res_h);
    CUVS_EXPECTS(index != nullptr, "index is null");
    auto idx = sq_read_ref(res, filename);
    delete reinterpret_cast<ivf_sq_index*>(index->addr);
    index->addr  = reinterpret_cast<uintptr_t>(idx.release());
    index->dtype = DLDataType{0, 0, 0};
  });
}

// test hooks (not in the reference ABI): list size; one list's codes row-major [size, dim] + source ids; the quantizer
__attribute__((visibility("default"))) int cuvsAmdIvfSqListSize(cuvsIvfSqIndex_t index, uint32_t label, uint32_t* size)
{
  return translate_exceptions([=] {
    auto& idx = get_sq(index);
    CUVS_EXPECTS(label < idx.n_lists, "label out of range");
    *size = idx.h_list_sizes[label];
  });
}

__attribute__((visibility("default"))) int cuvsAmdIvfSqUnpackList(cuvsResources_t res_h, cuvsIvfSqIndex_t index, uint32_t label,
                                                                   uint8_t* out_codes, int64_t* out_ids)
{
  return translate_exceptions([=] {
    auto& res = *as_res(res_h);
    auto& idx = get_sq(index);
    CUVS_EXPECTS(label < idx.n_lists, "label out of range");
    const uint32_t sz = idx.h_list_sizes[label];
    if (sz == 0) return;
    const int64_t total = (int64_t)sz * idx.dim;
    hipLaunchKernelGGL(sq_unpack_list_kernel, dim3(grid_blocks(total, 256)), dim3(256), 0, res.stream, idx.data.data(), idx.n_chunks,
                       idx.dim, (int64_t)idx.h_list_offsets[label], sz, out_codes);
    copy_async(res, out_ids, idx.indices.data() + idx.h_list_offsets[label], (size_t)sz * sizeof(int64_t));
    HIP_TRY(hipGetLastError());
  });
}

// host copies of vmin [dim] and delta [dim]
__attribute__((visibility("default"))) int cuvsAmdIvfSqGetQuantizer(cuvsResources_t res_h, cuvsIvfSqIndex_t index, float* vmin,
                                                                     float* delta)
{
  return translate_exceptions([=] {
    auto& res = *as_res(res_h);
    auto& idx = get_sq(index);
    copy_async(res, vmin, idx.vmin.data(), idx.vmin.bytes());
    copy_async(res, delta, idx.delta.data(), idx.delta.bytes());
    sync(res);
  });
}

}  // extern "C"
