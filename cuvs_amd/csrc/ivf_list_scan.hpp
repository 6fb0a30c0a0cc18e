// Device half of a list-major IVF search that is the same whatever the rows are made of (ivf_flat.hip: raw elements,
// ivf_sq.hip: 8-bit codes): a workgroup takes one work item (up to QPB (query, probe) pairs of one list), every wave scores
// tiles of 64 rows in its own way and hands the scores to the code here, which owns the shared k-th bounds, the admission into the
// per-wave register top lists (tie order on (distance, row), NaNs, the bitset filter), the merge of the wave lists and the
// per-pair output. The host half (coarse search, list assignment, list growth) is in ivf_lists.hpp.
#pragma once
#include "ivf_common.hpp"

#include <cfloat>
#include <type_traits>

namespace cuvs_amd {
namespace {

// what every list scan is launched with; the kernels' own argument structs derive from it
struct list_scan_args {
  const work_item* items;
  const uint32_t* item_begin;  // device scalars: this launch covers items [*item_begin, *item_end); nullptr: from 0
  const uint32_t* item_end;
  uint32_t n_lists;            // item.list >= n_lists: tail-phase label of list item.list - n_lists
  const uint32_t* sorted_pairs;
  const float* qtiles;         // [n_items, dim_pad + 1, QPB] fp32 query tile of every work item
  const uint8_t* data;
  const uint32_t* list_offsets;
  const uint32_t* list_sizes;
  float* out_d;
  uint32_t* out_i;
  uint32_t* query_kth;
  const uint32_t* filter_bits;  // optional bitset over source ids (1 keeps), sample_filter.cuh semantics
  const int64_t* indices;       // flat row -> source id (only read when filtering)
  uint32_t n_probes, n_chunks, k;
  float* all_scores;         // non-fused path (large k, ivf_common.hpp): [n_queries, scores_ld] score of every probed row
  uint32_t* all_rows;        //   flat row of every column (0xffffffff: nothing there)
  const uint32_t* pair_seg;  //   first column of each pair in its query's row
  size_t scores_ld;
};

// dynamic LDS of a scan workgroup: the merge area (QPB x WAVES x k (distance, row) entries), then kthb[16], then pid[16]
__host__ __device__ constexpr size_t list_scan_merge_bytes(int qpb, int waves, uint32_t k)
{
  return (((size_t)qpb * waves * k * 8) + 15) & ~size_t(15);
}
__host__ __device__ constexpr size_t list_scan_smem_bytes(int qpb, int waves, uint32_t k)
{
  return list_scan_merge_bytes(qpb, waves, k) + 2 * 16 * 4;
}

// a workgroup's work item
struct list_scan_item {
  work_item item;
  uint32_t w;         // index of the item (its query tile)
  uint32_t L;         // list
  uint32_t base_row;  // first flat row of the list
  uint32_t len;       // rows in the list
  uint32_t* kthb;     // LDS [QPB]: k-th bound (as sort key) of every pair's query, shared by the waves
  uint32_t* pid;      // LDS [QPB]: pair ids (0xffffffff: none)
};

// false: a surplus workgroup (grids are upper bounds of the device-side item counts), nothing to do. All threads call it.
template <int QPB, int WAVES>
__device__ __forceinline__ bool list_scan_begin(const list_scan_args& a, char* smem, list_scan_item& s)
{
  const uint32_t item0 = a.item_begin ? *a.item_begin : 0u;
  s.w                  = item0 + blockIdx.x;
  if (s.w >= *a.item_end) return false;
  s.item = a.items[s.w];
  s.kthb = reinterpret_cast<uint32_t*>(smem + list_scan_merge_bytes(QPB, WAVES, a.k));
  s.pid  = s.kthb + 16;
  s.L        = s.item.list >= a.n_lists ? s.item.list - a.n_lists : s.item.list;
  s.base_row = a.list_offsets[s.L];
  s.len      = a.list_sizes[s.L];
  const int tid = threadIdx.x;
  if (tid < QPB) {
    const uint32_t p = tid < (int)s.item.count ? a.sorted_pairs[s.item.first + tid] : 0xffffffffu;
    s.pid[tid]       = p;
    s.kthb[tid]      = p != 0xffffffffu ? a.query_kth[p / a.n_probes] : 0u;
  }
  __syncthreads();
  return true;
}

// the per-wave top lists of the item's pairs
template <int QPB, int E>
struct list_scan_tops {
  static_assert(QPB <= 8, "one fresh bit per query");
  wave_top<E> top[QPB];
  uint32_t fresh;  // bit j: this wave's list of query j is still empty (wave-uniform)
  __device__ __forceinline__ void init()
  {
#pragma unroll
    for (int j = 0; j < QPB; ++j) top[j].init();
    fresh = 0xffu;
  }
};

// the compiler sinks every load of a group to its first use (one load, one wait, sixteen fmas, next load ...); an empty asm that
// takes all four as operands keeps them issued back to back
template <int N>
__device__ __forceinline__ void keep_loads_together(uint4 (&w)[N])
{
  static_assert(N == 4, "four chunks per group");
  // (not volatile: an asm with unmodelled side effects counts as a memory clobber, and the wave-uniform loads of the query tile
  // stop being scalar loads)
  asm(""
      : "+v"(w[0].x), "+v"(w[0].y), "+v"(w[0].z), "+v"(w[0].w), "+v"(w[1].x), "+v"(w[1].y), "+v"(w[1].z), "+v"(w[1].w),
        "+v"(w[2].x), "+v"(w[2].y), "+v"(w[2].z), "+v"(w[2].w), "+v"(w[3].x), "+v"(w[3].y), "+v"(w[3].z), "+v"(w[3].w));
}

// This lane's score dj (smaller is better) of row tile0 + lane for query j of the item: stored (ALL, the non-fused path) or
// admitted into the wave's top list of that query. The kernels call it for j < item.count.
template <int QPB, int E, bool ALL>
__device__ __forceinline__ void list_scan_offer(const list_scan_args& a, const list_scan_item& s, const int j, const float dj,
                                                const uint32_t tile0, const int lane, list_scan_tops<QPB, E>& t)
{
  const uint32_t v = tile0 + (uint32_t)lane;
  const bool valid = v < s.len;
  const int kr     = (int)a.k - 1;
  if constexpr (ALL) {  // non-fused path: every score goes to the query's row (filtered rows keep the fill)
    bool keep = valid;
    if (keep && a.filter_bits != nullptr) {
      const int64_t sid = a.indices[(size_t)s.base_row + v];
      keep              = (a.filter_bits[sid >> 5] >> (sid & 31)) & 1u;
    }
    const uint32_t p = s.pid[j];
    if (keep) {
      const size_t o  = (size_t)(p / a.n_probes) * a.scores_ld + a.pair_seg[p] + v;
      a.all_scores[o] = dj;
      a.all_rows[o]   = s.base_row + v;
    }
    return;
  }
  const uint32_t bound = s.kthb[j];
  unsigned long long m = __ballot(valid && float_to_key(dj) <= bound);
  if (m == 0ull) return;
  // the wave's first candidates of query j (its list is empty: cold bounds let nearly every row of the first tile through):
  // one sorting network instead of up to 64 serial insertions - the list that results is the same, entry for entry
  const bool first = ((t.fresh >> j) & 1u) != 0u;
  t.fresh &= ~(1u << j);
  if (first && a.filter_bits == nullptr && __popcll(m) >= 12 && __ballot(dj != dj) == 0ull) {
    const bool c = ((m >> lane) & 1ull) != 0ull;
    float sd     = c ? dj : INFINITY;
    uint32_t si  = c ? v : 0xffffffffu;
    wave_sort64(sd, si, lane);
    t.top[j].d[0] = sd;
    t.top[j].i[0] = si;
    const float kd0 = t.top[j].rank_d(kr);
    if (lane == 0 && kd0 < INFINITY) atomicMin(&s.kthb[j], float_to_key(kd0));
    return;
  }
  float kd      = t.top[j].rank_d(kr);
  uint32_t ki   = t.top[j].rank_i(kr);
  bool improved = false;
  while (m != 0ull) {
    const int src = (int)__ffsll((long long)m) - 1;
    m &= m - 1ull;
    const float cd    = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(dj), src));
    const uint32_t ci = tile0 + (uint32_t)src;
    if (a.filter_bits != nullptr) {  // pre-filter: rows whose source id is masked out never enter the top list
      const int64_t sid = a.indices[(size_t)s.base_row + ci];
      if (!((a.filter_bits[sid >> 5] >> (sid & 31)) & 1u)) continue;
    }
    if ((cd < kd) || (cd == kd && ci < ki)) {
      t.top[j].insert(cd, ci, lane);
      kd       = t.top[j].rank_d(kr);
      ki       = t.top[j].rank_i(kr);
      improved = true;
    }
  }
  if (improved && lane == 0 && kd < INFINITY) atomicMin(&s.kthb[j], float_to_key(kd));
}

// After the scan loop: the wave lists of every pair merged into the pair's k best (out_d / out_i, FLT_MAX / 0xffffffff where
// fewer were found) and the query's k-th bound lowered for the launches that follow. All threads of the workgroup call it;
// the merge area at the start of smem is free by then.
template <int QPB, int WAVES, int E>
__device__ __forceinline__ void list_scan_merge(const list_scan_args& a, const list_scan_item& s, char* smem,
                                                const list_scan_tops<QPB, E>& t)
{
  const int tid  = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  __syncthreads();
  if constexpr (E > 1) {
    // k > 64: the sorted wave lists are merged by the whole workgroup, one query after the other (ivf_common.hpp)
    constexpr int KP2 = E == 2 ? 128 : 256;
    float* sd    = reinterpret_cast<float*>(smem);
    uint32_t* si = reinterpret_cast<uint32_t*>(smem + (size_t)WAVES * KP2 * 4);
    for (int j = 0; j < QPB; ++j) {
      if (j >= (int)s.item.count) break;  // workgroup-uniform
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const int r   = e * 64 + lane;
        const bool in = r < (int)a.k;
        sd[wave * KP2 + r] = in ? t.top[j].d[e] : INFINITY;
        si[wave * KP2 + r] = in ? t.top[j].i[e] : 0xffffffffu;
      }
      __syncthreads();
      merge_sorted_lists<WAVES * 64>(sd, si, WAVES, KP2, tid);
      const size_t o = (size_t)s.pid[j] * a.k;
      for (int r = tid; r < (int)a.k; r += WAVES * 64) {
        const bool ok  = si[r] != 0xffffffffu;
        a.out_d[o + r] = ok ? sd[r] : FLT_MAX;
        a.out_i[o + r] = ok ? s.base_row + si[r] : 0xffffffffu;
      }
      if (tid == 0 && si[a.k - 1] != 0xffffffffu && sd[a.k - 1] < INFINITY)
        atomicMin(&a.query_kth[s.pid[j] / a.n_probes], float_to_key(sd[a.k - 1]));
      __syncthreads();  // the next query reuses the area
    }
  } else {
    // k <= 64: every wave list is one slot per lane; wave j inserts the lists of query j into a fresh one
    const int kr   = (int)a.k - 1;
    float* mg_d    = reinterpret_cast<float*>(smem);
    uint32_t* mg_i = reinterpret_cast<uint32_t*>(smem + (size_t)QPB * WAVES * a.k * 4);
#pragma unroll
    for (int j = 0; j < QPB; ++j) {
      if (lane < (int)a.k) {
        mg_d[((size_t)j * WAVES + wave) * a.k + lane] = t.top[j].d[0];
        mg_i[((size_t)j * WAVES + wave) * a.k + lane] = t.top[j].i[0];
      }
    }
    __syncthreads();
    if (wave < QPB && wave < (int)s.item.count) {
      const int j = wave;
      wave_top<1> fin;
      fin.init();
      float kd    = INFINITY;
      uint32_t ki = 0xffffffffu;
      const int n = WAVES * (int)a.k;
      for (int b0 = 0; b0 < n; b0 += 64) {
        float md    = INFINITY;
        uint32_t mi = 0xffffffffu;
        if (b0 + lane < n) { md = mg_d[(size_t)j * n + b0 + lane]; mi = mg_i[(size_t)j * n + b0 + lane]; }
        unsigned long long m = __ballot(mi != 0xffffffffu && ((md < kd) || (md == kd && mi < ki)));
        while (m != 0ull) {
          const int src = (int)__ffsll((long long)m) - 1;
          m &= m - 1ull;
          const float cd    = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(md), src));
          const uint32_t ci = __builtin_amdgcn_readlane(mi, src);
          if ((cd < kd) || (cd == kd && ci < ki)) {
            fin.insert(cd, ci, lane);
            kd = fin.rank_d(kr);
            ki = fin.rank_i(kr);
          }
        }
      }
      const size_t o = (size_t)s.pid[j] * a.k;
      if (lane < (int)a.k) {
        const bool ok     = fin.i[0] != 0xffffffffu;
        a.out_d[o + lane] = ok ? fin.d[0] : FLT_MAX;
        a.out_i[o + lane] = ok ? s.base_row + fin.i[0] : 0xffffffffu;
      }
      if (lane == 0 && kd < INFINITY) atomicMin(&a.query_kth[s.pid[j] / a.n_probes], float_to_key(kd));
    }
  }
}

// (every score stored, k in 65..256, metric kind 0: L2, 1: inner product, 2: cosine) -> f(E, METRIC, ALL) as integral constants
template <typename F>
void list_scan_dispatch(const bool all, const bool big_k, const int metric_kind, F&& f)
{
  auto by_metric = [&](auto e, auto all_c) {
    if (metric_kind == 2)      f(e, std::integral_constant<int, 2>{}, all_c);
    else if (metric_kind == 1) f(e, std::integral_constant<int, 1>{}, all_c);
    else                       f(e, std::integral_constant<int, 0>{}, all_c);
  };
  if (all)        by_metric(std::integral_constant<int, 1>{}, std::true_type{});
  else if (big_k) by_metric(std::integral_constant<int, 4>{}, std::false_type{});
  else            by_metric(std::integral_constant<int, 1>{}, std::false_type{});
}

template <typename Args>
void list_scan_launch(resources& res, void (*kern)(Args), const int threads, const Args& a, const size_t smem, const unsigned grid)
{
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
  hipLaunchKernelGGL(kern, dim3(grid), dim3(threads), smem, res.stream, a);
}

}  // namespace
}  // namespace cuvs_amd
