// ScaNN search (C entry points include/cuvs_amd/scann_search.h; contract, layouts and measurements: DESIGN.md 3.1za). The
// coarse search, the grouping of the (query, probe) pairs and select_k are the library's own (ivf_lists.hpp, ivf_common.hpp,
// ops.hpp); new here:
//
//   lists         built by the first search of an index under its lock: scann_host::build_search_lists on the host (a counting
//                 sort of the primary and the SOAR entries into their leaves, the codes as 32-entry word tiles, the constant t of
//                 every entry, the bf16 codebook), one upload, and the bf16 rows for the re-rank.
//   scann_scan_kernel   a workgroup per unit = up to 32 queries of one leaf x up to kUnitEntries of its entries. The unit's 32 bf16
//                 query rows and, while it fits half the LDS, the bf16 codebook are staged once. A wave takes 32-entry tiles: per
//                 K step of 16 dimensions a lane (entry = lane % 32, half = lane / 32) decodes the 8 dimensions of its half from
//                 its entry's code bytes straight into the operand registers and the wave issues one
//                 v_mfma_f32_32x32x16_bf16 against the query fragment read from LDS. The queries are the instruction's first
//                 source and the entries its second: an accumulator column is an entry, so the 32 lanes of a half-wave store 128
//                 contiguous bytes of one query's score row.
//   scann_dedupe_kernel a workgroup per query: the best 2 M entries by (score, row), first occurrence of every row through a hash
//                 table in LDS, the first M of those.
//   scann_rerank_kernel a wave per (query, candidate): the fp32 fma chain over the bf16 row in ascending dimension - 64
//                 coordinates are loaded at once, the chain itself runs over the lanes' values one by one.
#include "common.hpp"
#include "device_utils.hpp"
#include "ivf_common.hpp"
#include "ivf_lists.hpp"
#include "ops.hpp"
#include "scann_host.hpp"
#include "scann_index.hpp"

#include <cuvs_amd/scann_search.h>

#include <algorithm>
#include <cfloat>
#include <vector>

namespace cuvs_amd {

namespace H = scann_host;

struct scann_search_lists {
  int dim_pad = 0, n_words = 0;
  uint32_t max_leaf = 0;
  std::vector<uint32_t> h_leaf_size;
  dev_buf<uint32_t> leaf_size, tile_off, ids, words;
  dev_buf<float> t, center_norms, unused_sqrt;
  dev_buf<uint16_t> book, rows;  // bf16 codebook [book_n, dim_pad]; bf16 rows [n, dim] (with reordering_bf16)
};

namespace {

constexpr int kScanThreads  = 256;
constexpr int kScanQueries  = 32;    // queries of a unit: one matrix-core operand
constexpr int kUnitEntries  = 2048;  // entries of a unit: 16 tiles per wave - the codebook staging is spread over 2 M products
constexpr int kQueryPad     = 8;     // bf16 elements between staged query rows: 16-byte reads of 32 rows spread over the banks
constexpr uint32_t kNoRow   = H::kNoRow;

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ uint16_t bf16_rne_dev(float f)
{
  uint32_t u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}

// qb [nq, dim_pad]: the queries rounded to bf16, zeros past dim
__global__ void scann_query_bf16_kernel(const float* __restrict__ q, int64_t nq, int dim, int dim_pad, uint16_t* __restrict__ qb)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nq * dim_pad) return;
  const int64_t r = i / dim_pad;
  const int d     = (int)(i - r * dim_pad);
  qb[i]           = d < dim ? bf16_rne_dev(q[r * dim + d]) : (uint16_t)0;
}

// the slots of a query's score row behind the entries of its probed leaves: nothing found
__global__ void scann_fill_tail_kernel(const uint32_t* __restrict__ probes, const uint32_t* __restrict__ leaf_size, uint32_t n_probes,
                                       size_t ld, float* __restrict__ scores, uint32_t* __restrict__ rows)
{
  const int64_t q = blockIdx.x;
  uint32_t used   = 0;
  for (uint32_t p = 0; p < n_probes; ++p) used += leaf_size[probes[q * n_probes + p]];
  for (size_t i = used + threadIdx.x; i < ld; i += blockDim.x) {
    scores[q * ld + i] = FLT_MAX;
    rows[q * ld + i]   = kNoRow;
  }
}

struct scan_args {
  const work_item* items;
  const uint32_t* n_items;       // device scalar
  const uint32_t* sorted_pairs;  // pair = query * n_probes + probe rank
  const float* pd;               // [n_pairs] coarse value: |q - c|^2, or <q, c>
  const uint32_t* pair_seg;      // [n_pairs] first column of the pair's leaf in the query's score row
  const uint16_t* qb;            // [nq, dim_pad]
  const uint32_t *leaf_size, *tile_off, *ids, *words;
  const float* t;
  const uint16_t* book;          // [book_n, dim_pad]
  float* all_scores;             // [nq, ld]
  uint32_t* all_rows;
  size_t ld;
  uint32_t n_probes;
  int dim_pad, n_words, width, shift, book_n, is_ip;
  unsigned long long* stats;
};

// the code of subspace s of the lane's entry (w points at the entry's first word; a tile's words are 32 apart)
__device__ __forceinline__ uint32_t code_of(const uint32_t* __restrict__ w, int s) { return (w[(s >> 2) * 32] >> ((s & 3) * 8)) & 255u; }

// The lane's 8 dimensions d0 .. d0 + 7 of its entry. VEC: dimensions fetched per codebook read - the subspace width where it
// divides 8, 8 where it is a multiple of 8, else 1 (a subspace may then straddle the lane's dimensions: code by code). SHIFT:
// the width is a power of two.
template <int VEC, bool SHIFT>
__device__ __forceinline__ uint4 decode_fragment(const uint16_t* __restrict__ book, const uint32_t* __restrict__ w, int d0, int dim_pad,
                                                 int width, int shift)
{
  uint4 f;
  if constexpr (VEC == 8) {
    const int s = SHIFT ? d0 >> shift : d0 / width;
    f           = *reinterpret_cast<const uint4*>(book + (size_t)code_of(w, s) * dim_pad + d0);
  } else if constexpr (VEC == 4) {  // subspaces d0 / 4 and d0 / 4 + 1: two bytes of one word
    const uint32_t word = w[(d0 >> 4) * 32] >> (((d0 >> 2) & 3) * 8);
    const uint2 lo      = *reinterpret_cast<const uint2*>(book + (size_t)(word & 255u) * dim_pad + d0);
    const uint2 hi      = *reinterpret_cast<const uint2*>(book + (size_t)((word >> 8) & 255u) * dim_pad + d0 + 4);
    f                   = uint4{lo.x, lo.y, hi.x, hi.y};
  } else if constexpr (VEC == 2) {  // subspaces d0 / 2 .. + 3: one word
    const uint32_t word = w[(d0 >> 3) * 32];
    uint32_t v[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) v[t] = *reinterpret_cast<const uint32_t*>(book + (size_t)((word >> (8 * t)) & 255u) * dim_pad + d0 + 2 * t);
    f = uint4{v[0], v[1], v[2], v[3]};
  } else {
    int s = SHIFT ? d0 >> shift : d0 / width;
    int r = d0 - s * width;
    uint32_t v[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      v[t] = book[(size_t)code_of(w, s) * dim_pad + d0 + t];
      if (++r == width) { r = 0; ++s; }
    }
    f = uint4{v[0] | (v[1] << 16), v[2] | (v[3] << 16), v[4] | (v[5] << 16), v[6] | (v[7] << 16)};
  }
  return f;
}

template <int VEC, bool SHIFT, bool BOOK_LDS>
__global__ __launch_bounds__(kScanThreads) void scann_scan_kernel(const scan_args a)
{
  extern __shared__ __attribute__((aligned(16))) uint16_t scan_smem[];  // queries [32][dim_pad + 8] | codebook [book_n][dim_pad]
  __shared__ float base_s[kScanQueries];
  __shared__ uint32_t seg_s[kScanQueries], query_s[kScanQueries];
  if (blockIdx.x >= *a.n_items) return;
  const work_item it     = a.items[blockIdx.x];
  const uint32_t len     = a.leaf_size[it.list];
  const uint32_t e_begin = blockIdx.y * (uint32_t)kUnitEntries;
  if (e_begin >= len) return;
  const uint32_t e_end = min(len, e_begin + (uint32_t)kUnitEntries);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, h = lane >> 5;
  const int qld = a.dim_pad + kQueryPad, vpr = a.dim_pad >> 3;
  uint16_t* qs  = scan_smem;
  uint16_t* bs  = scan_smem + kScanQueries * qld;

  if (tid < kScanQueries) {
    const bool on       = (uint32_t)tid < it.count;
    const uint32_t pair = on ? a.sorted_pairs[it.first + tid] : 0u;
    query_s[tid]        = on ? pair / a.n_probes : kNoRow;
    base_s[tid]         = on ? a.pd[pair] : 0.f;
    seg_s[tid]          = on ? a.pair_seg[pair] : 0u;
  }
  __syncthreads();
  for (int i = tid; i < kScanQueries * vpr; i += kScanThreads) {
    const int r = i / vpr, c = i - r * vpr;
    uint4 v     = uint4{0u, 0u, 0u, 0u};
    if (query_s[r] != kNoRow) v = reinterpret_cast<const uint4*>(a.qb + (size_t)query_s[r] * a.dim_pad)[c];
    *reinterpret_cast<uint4*>(qs + r * qld + c * 8) = v;
  }
  if constexpr (BOOK_LDS) {
    for (int i = tid; i < a.book_n * vpr; i += kScanThreads) reinterpret_cast<uint4*>(bs)[i] = reinterpret_cast<const uint4*>(a.book)[i];
  }
  __syncthreads();
  const uint16_t* book = BOOK_LDS ? bs : a.book;

  const uint32_t tile0 = a.tile_off[it.list];
  for (uint32_t sub = e_begin / 32u + wave; sub * 32u < e_end; sub += kScanThreads / 64) {  // wave-uniform
    const uint32_t* w = a.words + ((size_t)(tile0 + sub) * a.n_words) * 32 + li;
    f32x16 acc        = {};
    for (int d0 = 8 * h; d0 < a.dim_pad; d0 += 16) {
      const uint4 qf = *reinterpret_cast<const uint4*>(qs + li * qld + d0);
      const uint4 ef = decode_fragment<VEC, SHIFT>(book, w, d0, a.dim_pad, a.width, a.shift);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, qf), __builtin_bit_cast(bf16x8, ef), acc, 0, 0, 0);
    }
    // accumulator register v of lane (li, h): query (v & 3) + 8 (v >> 2) + 4 h of the unit, entry li of the tile
    const uint32_t e = sub * 32u + li;
    if (e >= e_end) continue;
    const size_t slot  = (size_t)(tile0 + sub) * 32 + li;
    const uint32_t row = a.ids[slot];
    const float tj     = a.t[slot];
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const uint32_t qi = (uint32_t)((v & 3) + 8 * (v >> 2) + 4 * h);
      if (qi >= it.count) continue;
      const float s    = a.is_ip ? -(base_s[qi] + acc[v]) : __fmaf_rn(-2.0f, acc[v], base_s[qi] + tj);
      const size_t out = (size_t)query_s[qi] * a.ld + seg_s[qi] + e;
      a.all_scores[out] = s;
      a.all_rows[out]   = row;
    }
  }
  if (tid == 0) {
    atomicAdd(&a.stats[0], 1ull);
    atomicAdd(&a.stats[1], (unsigned long long)(e_end - e_begin) * it.count);
    if (!BOOK_LDS) atomicAdd(&a.stats[2], 1ull);
  }
}

// A workgroup per query: d2 / i2 [n2] are the query's best entries ascending by (score, row), padding (kNoRow) last. Every row's
// first occurrence is found through an open-addressed table in LDS (slots >= 2 n2, a power of two): the smallest position of
// every row id; the kept entries are compacted in order and the first m written, the rest of the m slots padded.
__global__ __launch_bounds__(256) void scann_dedupe_kernel(const float* __restrict__ d2, const uint32_t* __restrict__ i2, int n2, int m,
                                                           int slots, float* __restrict__ out_d, uint32_t* __restrict__ out_i,
                                                           unsigned long long* __restrict__ stats)
{
  extern __shared__ uint32_t dd_smem[];  // keys [slots] | first position [slots]
  __shared__ int scan_smem[17];
  uint32_t* keys       = dd_smem;
  uint32_t* first      = dd_smem + slots;
  const uint32_t mask  = (uint32_t)slots - 1u;
  const float* d       = d2 + (size_t)blockIdx.x * n2;
  const uint32_t* id   = i2 + (size_t)blockIdx.x * n2;
  for (int s = threadIdx.x; s < slots; s += 256) { keys[s] = kNoRow; first[s] = 0xffffffffu; }
  __syncthreads();
  auto home = [&](uint32_t row) { return (row * 2654435761u) >> 7 & mask; };
  for (int p = threadIdx.x; p < n2; p += 256) {
    const uint32_t row = id[p];
    if (row == kNoRow) continue;
    uint32_t s = home(row);
    while (true) {  // ends: the table has more slots than there are rows
      const uint32_t old = atomicCAS(&keys[s], kNoRow, row);
      if (old == kNoRow || old == row) break;
      s = (s + 1u) & mask;
    }
    atomicMin(&first[s], (uint32_t)p);
  }
  __syncthreads();
  auto kept = [&](int p) {
    const uint32_t row = id[p];
    if (row == kNoRow) return false;
    uint32_t s = home(row);
    while (keys[s] != row) s = (s + 1u) & mask;
    return first[s] == (uint32_t)p;
  };
  // a thread takes a run of consecutive positions: its count, one block scan, then its writes
  const int per = (n2 + 255) / 256, b = threadIdx.x * per, e = min(n2, b + per);
  int mine = 0, dropped = 0;
  for (int p = b; p < e; ++p) {
    const bool k = kept(p);
    mine += k ? 1 : 0;
    dropped += (!k && id[p] != kNoRow) ? 1 : 0;
  }
  int total;
  int at = block_exclusive_scan(mine, scan_smem, &total);
  for (int p = b; p < e && at < m; ++p) {
    if (!kept(p)) continue;
    out_d[(size_t)blockIdx.x * m + at] = d[p];
    out_i[(size_t)blockIdx.x * m + at] = id[p];
    ++at;
  }
  for (int p = total + threadIdx.x; p < m; p += 256) {
    out_d[(size_t)blockIdx.x * m + p] = FLT_MAX;
    out_i[(size_t)blockIdx.x * m + p] = kNoRow;
  }
  dropped = wave_sum_i(dropped);
  if ((threadIdx.x & 63) == 0 && dropped != 0) atomicAdd(&stats[3], (unsigned long long)dropped);
}

// A wave per (query, candidate): acc = fmaf(q_t - x_t, q_t - x_t, acc) (L2) or fmaf(q_t, x_t, acc) (inner product, stored
// negated: smaller is better downstream), t ascending, x the bf16 row widened to fp32. A missing candidate scores FLT_MAX.
__global__ __launch_bounds__(256) void scann_rerank_kernel(const float* __restrict__ q, int64_t n_cand_total, int m, int dim,
                                                           const uint16_t* __restrict__ rows, const uint32_t* __restrict__ cand,
                                                           int is_ip, float* __restrict__ out)
{
  const int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= n_cand_total) return;  // wave-uniform
  const int lane     = threadIdx.x & 63;
  const uint32_t row = cand[c];
  if (row == kNoRow) {
    if (lane == 0) out[c] = FLT_MAX;
    return;
  }
  const float* qr    = q + (c / m) * dim;
  const uint16_t* xr = rows + (size_t)row * dim;
  float acc          = 0.f;
  for (int base = 0; base < dim; base += kWave) {
    const int t    = base + lane;
    const float qv = t < dim ? qr[t] : 0.f;
    const float xv = t < dim ? __uint_as_float((uint32_t)xr[t] << 16) : 0.f;
    const float u  = is_ip ? qv : qv - xv;
    const float v  = is_ip ? xv : u;
    const int steps = min(kWave, dim - base);
#pragma unroll
    for (int l = 0; l < kWave; ++l) {
      const float ul = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(u), l));
      const float vl = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(v), l));
      if (l < steps) acc = __fmaf_rn(ul, vl, acc);
    }
  }
  if (lane == 0) out[c] = is_ip ? -acc : acc;
}

// (score, row) -> (distance, id) of the C interface: inner products come back positive; an empty slot as after cuvsIvfFlatSearch
__global__ void scann_postprocess_kernel(const float* __restrict__ d, const uint32_t* __restrict__ id, int64_t nq, int k, int ld,
                                         int is_ip, int64_t* __restrict__ neighbors, float* __restrict__ distances)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nq * k) return;
  const int64_t q = i / k, j = i - q * k;
  const uint32_t row = id[q * ld + j];
  const float v      = d[q * ld + j];
  neighbors[i]       = row == kNoRow ? INT64_MAX : (int64_t)row;
  distances[i]       = row == kNoRow ? FLT_MAX : (is_ip ? -v : v);
}

template <int VEC, bool SHIFT>
void launch_scan(resources& res, const scan_args& a, bool book_lds, size_t smem, dim3 grid)
{
  auto go = [&](auto kern) {
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    hipLaunchKernelGGL(kern, grid, dim3(kScanThreads), smem, res.stream, a);
  };
  if (book_lds) go(scann_scan_kernel<VEC, SHIFT, true>);
  else          go(scann_scan_kernel<VEC, SHIFT, false>);
}

std::shared_ptr<scann_search_lists> ensure_lists(resources& res, scann_index& idx)
{
  std::lock_guard<std::mutex> lock(idx.search_mu);
  if (idx.search) return idx.search;
  const std::vector<float> centers   = to_host(res, idx.centers.data(), idx.centers.size());
  const std::vector<float> codebook  = to_host(res, idx.codebook.data(), idx.codebook.size());
  const std::vector<uint32_t> labels = to_host(res, idx.labels.data(), idx.labels.size());
  const std::vector<uint32_t> soar   = to_host(res, idx.soar_labels.data(), idx.soar_labels.size());
  H::host_index h;
  h.n_rows = idx.n; h.dim = idx.dim; h.n_leaves = idx.n_leaves; h.n_sub = idx.n_sub; h.book_n = idx.book_n;
  h.pq_dim = idx.p.pq_dim;
  h.centers = centers.data(); h.labels = labels.data(); h.soar = soar.data(); h.codebook = codebook.data();
  h.codes = idx.codes.data(); h.soar_codes = idx.soar_codes.data();
  const H::search_lists s = H::build_search_lists(h, idx.p.metric == M_L2Expanded);
  auto out         = std::make_shared<scann_search_lists>();
  out->dim_pad     = (int)s.dim_pad;
  out->n_words     = (int)s.n_words;
  out->h_leaf_size = s.leaf_size;
  for (uint32_t v : s.leaf_size) out->max_leaf = std::max(out->max_leaf, v);
  auto upload = [&](auto& dst, const auto& src) {
    using T = typename std::decay_t<decltype(src)>::value_type;
    dst     = dev_buf<T>::persistent(src.size());
    copy_async(res, dst.data(), src.data(), src.size() * sizeof(T));
  };
  upload(out->leaf_size, s.leaf_size);
  upload(out->tile_off, s.tile_off);
  upload(out->ids, s.ids);
  upload(out->words, s.words);
  upload(out->t, s.t);
  upload(out->book, s.book_bf16);
  if (idx.p.reordering_bf16) {
    out->rows = dev_buf<uint16_t>::persistent(idx.bf16.size());
    copy_async(res, out->rows.data(), idx.bf16.data(), idx.bf16.size() * sizeof(int16_t));
  }
  ivf_set_center_norms(res, idx.p.metric, idx.centers.data(), (uint32_t)idx.n_leaves, (uint32_t)idx.dim, out->center_norms, out->unused_sqrt);
  sync(res);  // the host arrays go out of scope; other handles' streams may use the lists from here on
  idx.search = out;
  return out;
}

thread_local uint64_t g_scann_search_stats[4] = {0, 0, 0, 0};

void scann_search(resources& res, scann_index& idx, uint32_t n_probes_in, uint32_t n_reorder, const float* queries, int64_t m, int k,
                  int64_t* neighbors, float* distances)
{
  for (uint64_t& v : g_scann_search_stats) v = 0;
  if (m == 0) return;
  const std::shared_ptr<scann_search_lists> lists = ensure_lists(res, idx);
  const scann_search_lists& L = *lists;
  const int is_ip          = idx.p.metric == M_InnerProduct ? 1 : 0;
  const uint32_t n_leaves  = (uint32_t)idx.n_leaves;
  const uint32_t n_probes  = std::min(n_probes_in, n_leaves);
  const int keep           = n_reorder > 0 ? (int)n_reorder : k;  // M of the dedupe rule
  const int n2             = 2 * keep;
  const size_t ld          = (size_t)round_up((int64_t)std::max<size_t>(largest_lists_total(L.h_leaf_size, n_probes), 1), 4);
  const int dim = (int)idx.dim, dim_pad = L.dim_pad;

  // the unit's LDS: the query rows, and the codebook while both fit half the LDS (two workgroups per CU)
  const size_t q_bytes    = (size_t)kScanQueries * (dim_pad + kQueryPad) * sizeof(uint16_t);
  const size_t book_bytes = (size_t)idx.book_n * dim_pad * sizeof(uint16_t);
  const bool book_lds     = q_bytes + book_bytes <= res.lds_per_block / 2;
  const size_t smem       = q_bytes + (book_lds ? book_bytes : 0);
  CUVS_EXPECTS(smem <= res.lds_per_block, "dim %d is too large for the ScaNN scan", dim);
  const int width = (int)idx.p.pq_dim;
  const bool pow2 = (width & (width - 1)) == 0;
  int shift       = 0;
  while ((1 << shift) < width) ++shift;
  const int vec = width % 8 == 0 ? 8 : (8 % width == 0 && width > 1) ? width : 1;

  // queries per batch: the score rows (value + row id), the coarse distances and the small per-query arrays within the limit
  const int64_t per_q = (int64_t)ld * 8 + (int64_t)round_up(n_leaves, 128) * 5 + (int64_t)n_probes * 24 + (int64_t)dim_pad * 2 +
                        (int64_t)n2 * 8 + (int64_t)keep * 12 + (int64_t)k * 8;
  const int64_t bs    = balanced_batch(m, std::max<int64_t>(1, (int64_t)res.ivf_batch_limit / per_q));
  const int64_t np_max = bs * n_probes;
  CUVS_EXPECTS(np_max < (int64_t(1) << 31), "ScaNN search: too many (query, probe) pairs in a batch");
  const size_t max_items = (size_t)(np_max / kScanQueries + n_leaves + 1);
  dev_buf<float> qn(res, bs), pd(res, np_max), dist, scores(res, (size_t)bs * ld), top2_d(res, (size_t)bs * n2), cand_d(res, (size_t)bs * keep),
    rr_d(res, n_reorder > 0 ? (size_t)bs * keep : 0), out_d(res, n_reorder > 0 ? (size_t)bs * k : 0);
  dev_buf<uint32_t> probes(res, np_max), sorted_pairs(res, np_max), pair_off(res, n_leaves + 1), item_off(res, n_leaves + 1),
    pair_seg(res, np_max), rows(res, (size_t)bs * ld), top2_i(res, (size_t)bs * n2), cand_i(res, (size_t)bs * keep),
    out_i(res, n_reorder > 0 ? (size_t)bs * k : 0);
  dev_buf<work_item> items(res, max_items);
  dev_buf<uint16_t> qb(res, (size_t)bs * dim_pad);
  dev_buf<unsigned long long> stats(res, 4);
  HIP_TRY(hipMemsetAsync(stats.data(), 0, stats.bytes(), res.stream));
  const int slots        = next_pow2(2 * n2);
  const size_t dd_smem   = (size_t)slots * 2 * sizeof(uint32_t);
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(scann_dedupe_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)dd_smem));

  for (int64_t q0 = 0; q0 < m; q0 += bs) {
    const int64_t nq = std::min(bs, m - q0), n_pairs = nq * n_probes;
    const float* qf  = queries + q0 * dim;
    coarse_search(res, idx.centers.data(), dim, n_leaves, (uint32_t)dim, L.center_norms.data(), nullptr, idx.p.metric, qf, nq, n_probes, bs,
                  qn.data(), dist, pd.data(), probes.data());
    build_work_items(res, probes.data(), n_pairs, n_leaves, kScanQueries, sorted_pairs.data(), pair_off.data(), item_off.data(), items.data());
    hipLaunchKernelGGL(pair_segments_kernel, dim3(grid_blocks(nq, 256)), dim3(256), 0, res.stream, probes.data(), L.leaf_size.data(), nq,
                       n_probes, pair_seg.data());
    hipLaunchKernelGGL(scann_fill_tail_kernel, dim3((unsigned)nq), dim3(256), 0, res.stream, probes.data(), L.leaf_size.data(), n_probes, ld,
                       scores.data(), rows.data());
    hipLaunchKernelGGL(scann_query_bf16_kernel, dim3(grid_blocks(nq * dim_pad, 256)), dim3(256), 0, res.stream, qf, nq, dim, dim_pad, qb.data());
    scan_args a;
    a.items = items.data(); a.n_items = item_off.data() + n_leaves; a.sorted_pairs = sorted_pairs.data(); a.pd = pd.data();
    a.pair_seg = pair_seg.data(); a.qb = qb.data(); a.leaf_size = L.leaf_size.data(); a.tile_off = L.tile_off.data(); a.ids = L.ids.data();
    a.words = L.words.data(); a.t = L.t.data(); a.book = L.book.data(); a.all_scores = scores.data(); a.all_rows = rows.data(); a.ld = ld;
    a.n_probes = n_probes; a.dim_pad = dim_pad; a.n_words = L.n_words; a.width = width; a.shift = shift; a.book_n = (int)idx.book_n;
    a.is_ip = is_ip; a.stats = stats.data();
    // the grid is an upper bound of the (device-side) unit count: surplus workgroups leave at once
    const dim3 grid((unsigned)(n_pairs / kScanQueries + n_leaves + 1), (unsigned)std::max(1, ceil_div(L.max_leaf, kUnitEntries)));
    profile_begin(res, "scann_scan_kernel");
    if (vec == 8 && pow2)      launch_scan<8, true>(res, a, book_lds, smem, grid);
    else if (vec == 8)         launch_scan<8, false>(res, a, book_lds, smem, grid);
    else if (vec == 4)         launch_scan<4, true>(res, a, book_lds, smem, grid);
    else if (vec == 2)         launch_scan<2, true>(res, a, book_lds, smem, grid);
    else if (pow2)             launch_scan<1, true>(res, a, book_lds, smem, grid);
    else                       launch_scan<1, false>(res, a, book_lds, smem, grid);
    profile_end(res, "scann_scan_kernel");
    HIP_TRY(hipGetLastError());

    select_k<uint32_t, uint32_t>(res, scores.data(), rows.data(), nq, (int64_t)ld, (int64_t)ld, n2, top2_d.data(), top2_i.data(), true);
    hipLaunchKernelGGL(scann_dedupe_kernel, dim3((unsigned)nq), dim3(256), dd_smem, res.stream, top2_d.data(), top2_i.data(), n2, keep, slots,
                       cand_d.data(), cand_i.data(), stats.data());
    const float* fin_d    = cand_d.data();
    const uint32_t* fin_i = cand_i.data();
    int fin_ld            = keep;
    if (n_reorder > 0) {
      profile_begin(res, "scann_rerank_kernel");
      hipLaunchKernelGGL(scann_rerank_kernel, dim3(grid_blocks(nq * keep, 4)), dim3(256), 0, res.stream, qf, nq * keep, keep, dim, L.rows.data(),
                         cand_i.data(), is_ip, rr_d.data());
      profile_end(res, "scann_rerank_kernel");
      select_k<uint32_t, uint32_t>(res, rr_d.data(), cand_i.data(), nq, keep, keep, k, out_d.data(), out_i.data(), true);
      fin_d = out_d.data(); fin_i = out_i.data(); fin_ld = k;
    }
    hipLaunchKernelGGL(scann_postprocess_kernel, dim3(grid_blocks(nq * k, 256)), dim3(256), 0, res.stream, fin_d, fin_i, nq, k, fin_ld, is_ip,
                       neighbors + q0 * k, distances + q0 * k);
    HIP_TRY(hipGetLastError());
  }
  const std::vector<unsigned long long> hs = to_host(res, stats.data(), 4);  // (waits for the search: the buffers go out of scope)
  for (int i = 0; i < 4; ++i) g_scann_search_stats[i] = hs[i];
}

void* device_matrix(DLManagedTensor* t, const char* what, uint8_t code, uint8_t bits, int64_t* rows, int64_t* cols)
{
  if (t == nullptr) H::refuse("%s must not be NULL", what);
  const DLTensor& d = t->dl_tensor;
  if (!dtype_is(d.dtype, code, bits)) H::refuse("%s must be %s%d", what, code == kDLFloat ? "fp" : "int", (int)bits);
  if (d.ndim != 2 || d.shape[0] < 0 || d.shape[1] < 1) H::refuse("%s must be a 2-D matrix", what);
  if (!is_c_contiguous(d)) H::refuse("%s must be row-major and contiguous", what);
  if (!is_device_accessible(d)) H::refuse("%s must be accessible on device memory", what);
  *rows = d.shape[0];
  *cols = d.shape[1];
  return dl_data(d);
}

}  // namespace
}  // namespace cuvs_amd

using namespace cuvs_amd;

extern "C" {

cuvsError_t cuvsAmdScannSearchParamsCreate(cuvsAmdScannSearchParams_t* params)
{
  return (cuvsError_t)translate_exceptions([=] {
    CUVS_EXPECTS(params != nullptr, "params is null");
    *params = new cuvsAmdScannSearchParams{20u, 0u};
  });
}

cuvsError_t cuvsAmdScannSearchParamsDestroy(cuvsAmdScannSearchParams_t params)
{
  return (cuvsError_t)translate_exceptions([=] { delete params; });
}

cuvsError_t cuvsAmdScannSearch(cuvsResources_t res_h, cuvsAmdScannSearchParams_t params, cuvsAmdScannIndex_t index, DLManagedTensor* queries,
                               DLManagedTensor* neighbors, DLManagedTensor* distances)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& res = *as_res(res_h);
    if (params == nullptr) H::refuse("params must not be NULL");
    scann_index& idx = index_of(index);
    int64_t m, qd, nr, k, dr, dk;
    const float* q = static_cast<const float*>(device_matrix(queries, "queries", kDLFloat, 32, &m, &qd));
    int64_t* nb    = static_cast<int64_t*>(device_matrix(neighbors, "neighbors", kDLInt, 64, &nr, &k));
    float* ds      = static_cast<float*>(device_matrix(distances, "distances", kDLFloat, 32, &dr, &dk));
    if (nr != m || dr != m || dk != k) H::refuse("neighbors and distances must both have shape [%lld, k]", (long long)m);
    H::check_search(idx.p.metric, params->n_probes, params->n_reorder, k, idx.p.reordering_bf16, idx.dim, qd);
    scann_search(res, idx, params->n_probes, params->n_reorder, q, m, (int)k, nb, ds);
  });
}

cuvsError_t cuvsAmdScannSearchLastStats(uint64_t out[4])
{
  return (cuvsError_t)translate_exceptions([=] {
    CUVS_EXPECTS(out != nullptr, "out is null");
    for (int i = 0; i < 4; ++i) out[i] = g_scann_search_stats[i];
  });
}

}  // extern "C"
