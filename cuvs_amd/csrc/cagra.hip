// CAGRA on MI355X: graph build (kNN graph + rank-based prune + reverse-edge merge), graph search, C ABI
// (drop-in for c/src/neighbors/cagra.cpp).
//
// Reference: cpp/src/neighbors/detail/cagra/graph_core.cuh (kern_fused_prune :206-330 — 2-hop detour
// counting, kern_make_rev_graph_k :178-200, kern_merge_graph :375-470, optimize :1706-1809),
// cagra_build.cuh:1629-1760 (kNN graph by IVF-PQ + refine), search_plan.cuh:199-245 (max_iterations rule),
// search_single_cta_jit.cuh:105-452 (search loop), device_common_jit.cuh:36-181 (seeding, child distances),
// hashmap.hpp:23-148 (open addressing), compute_distance_impl.cuh:23-64 (team distance).
//
// MI355X design of the search: ONE wave64 per query (the reference's "single CTA" sized for 32-lane warps
// does not transfer): the wave keeps the sorted internal top list and the candidate list in LDS, dedups
// children with a small LDS hash (reset every few iterations like the reference's SMALL hash mode), computes
// child distances with 8 teams of 8 lanes (each team streams one dataset row in 128-byte pieces, 16 B per
// lane, so 8 rows are in flight per wave) and merges with a wave-level bitonic sort. ~12 KB of LDS per query
// lets a CU hold 13+ concurrent queries, which is what hides the dependent-gather latency of the walk.
#include "ivf_pq.hpp"
#include "ivf_pq_filter_common.hpp"
#include "ops.hpp"
#include "device_utils.hpp"
#include "serialize.hpp"
#include "npy_io.hpp"
#include "pq_quantize.hpp"

#include <cuvs/neighbors/cagra.h>
#include <cuvs_amd/extensions.h>

#include <algorithm>
#include <type_traits>
#include <cfloat>
#include <cmath>

namespace cuvs_amd {

// A VPQ-compressed dataset: row i is vq_book[label_i] + pq_book[code_i[s]] per subspace s, both books fp16, one
// PQ book shared by all subspaces, 8-bit codes. In memory a row is [uint32 label][8 x lane_bytes code bytes]: the codes that
// lane t of an 8-lane team needs (the 4-element pieces at d = 4 t + 32 j, ascending j) are contiguous, lane after lane, each
// lane's share padded with zeros to a multiple of 4 bytes. Files and cuvsAmdCagraIndexGetVpq show the reference's layout
// [uint32 label][pq_dim code bytes][zero padding to 4].
struct cagra_vpq {
  uint32_t vq_n = 0, pq_len = 0, pq_dim = 0;
  uint32_t row_len    = 0;  // bytes of a row in the reference's layout: 4 * (1 + ceil(pq_dim / 4))
  uint32_t lane_bytes = 0;  // bytes of one lane's codes of a row
  uint32_t stride     = 0;  // bytes of a row in memory: 4 + 8 * lane_bytes
  dev_buf<__half> vq_book;  // [vq_n, dim]
  dev_buf<__half> pq_book;  // [256, pq_len]
  dev_buf<uint8_t> codes;   // [n, stride]
  bool on() const { return codes.data() != nullptr; }
  void set_shape(int64_t dim, uint32_t vq_centers, uint32_t len)
  {
    vq_n       = vq_centers;
    pq_len     = len;
    pq_dim     = (uint32_t)(dim / len);
    row_len    = 4u * (1u + (pq_dim + 3u) / 4u);
    lane_bytes = (uint32_t)round_up(((dim + 31) / 32) * (4 / len), 4);
    stride     = 4u + 8u * lane_bytes;
  }
};
constexpr uint32_t kVpqBookN = 256;  // entries of the PQ book (pq_bits = 8)

struct cagra_index {
  int metric   = 0;
  elem_t dtype = elem_t::f32;
  int64_t n = 0, dim = 0;
  uint32_t degree = 0;
  const void* data = nullptr;  // device rows [n, dim]
  dev_buf<char> owned;
  dev_buf<uint32_t> graph;     // [n, degree]
  dev_buf<float> norms;        // [n] canonical |x| (cosine only; the reference's dataset_norms)
  // optional: the source id of every row (cagra.hpp index::source_indices, written by the reference's serializer as content-map
  // bit 1, cagra_serialize.cuh:72-83): a search reports source_indices[row] instead of the row (search_multi_cta.cuh:266-272)
  dev_buf<uint32_t> source_indices;
  int64_t source_bits = 0;  // max(source_indices) + 1, found once at load: the bits a filter over source ids has to hold
  cagra_vpq vpq;            // set: the rows are held compressed and `data` is null
};

// canonical row norms of the dataset for the cosine metric (no-op otherwise)
static void cagra_set_norms(resources& res, cagra_index& idx)
{
  if (idx.metric != M_CosineExpanded || idx.data == nullptr) return;
  idx.norms = dev_buf<float>::persistent(idx.n);
  switch (idx.dtype) {
    case elem_t::f32: row_norms<float>(res, static_cast<const float*>(idx.data), idx.n, idx.dim, idx.dim, idx.norms.data(), true); break;
    case elem_t::f16: row_norms<__half>(res, static_cast<const __half*>(idx.data), idx.n, idx.dim, idx.dim, idx.norms.data(), true); break;
    case elem_t::i8: row_norms<int8_t>(res, static_cast<const int8_t*>(idx.data), idx.n, idx.dim, idx.dim, idx.norms.data(), true); break;
    case elem_t::u8: row_norms<uint8_t>(res, static_cast<const uint8_t*>(idx.data), idx.n, idx.dim, idx.dim, idx.norms.data(), true); break;
  }
}

namespace {

constexpr uint32_t kInvalidNode = 0xffffffffu;
constexpr uint32_t kParentFlag  = 0x80000000u;

// ------------------------------------------------------------------ graph optimisation
// kern_fused_prune restated: one wave per node. For every neighbour D (rank kAD) of the node and every neighbour B of D,
// the FIRST rank kAB > kAD at which the node lists B gets a detour count. The node's list is looked up through a small
// open-addressing table (id -> lowest rank) instead of a linear scan of up to K LDS words per candidate; a hit at a
// rank <= kAD (duplicate ids in the list) falls back to the scan, so the counts are exactly those of the scan. The row
// of the next neighbour is loaded while the current one is processed (the 127 row gathers of a node were serial).
template <int PER>  // ids per lane and neighbour row: K <= 64 * PER; 16 / PER rows are in flight
__global__ __launch_bounds__(256) void prune_kernel(const uint32_t* __restrict__ knn, int64_t n, uint32_t K,
                                                    uint32_t out_degree, uint32_t* __restrict__ out, int64_t nid0, int dbg)
{
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  uint32_t tsize = 64;
  while (tsize < 2 * K) tsize <<= 1;  // <= 50 % load
  uint32_t* s_idx = reinterpret_cast<uint32_t*>(smem) + (size_t)wave * (2 * K + 2 * tsize);
  uint32_t* s_det = s_idx + K;
  uint32_t* t_key = s_det + K;
  uint32_t* t_pos = t_key + tsize;
  const int64_t nid = nid0 + (int64_t)blockIdx.x * 4 + wave;
  if (nid >= n) return;
  for (uint32_t k = lane; k < K; k += 64) {
    uint32_t v = knn[nid * K + k];
    s_idx[k]   = v;
    s_det[k]   = (v == (uint32_t)nid) ? K : 0;
  }
  for (uint32_t t = lane; t < tsize; t += 64) { t_key[t] = kInvalidNode; t_pos[t] = 0xffffffffu; }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  // table: id -> lowest rank holding it (invalid ids are not entered). A list with duplicate or invalid ids (not what a
  // kNN graph holds, but legal input) keeps the scan as the fallback; a wave whose list has neither never scans - one
  // scanning lane would hold up the other 63
  bool odd = false;
  for (uint32_t k = lane; k < K; k += 64) {
    const uint32_t v = s_idx[k];
    if (v >= n) { odd = true; continue; }
    uint32_t pos = (v * 2654435761u) & (tsize - 1);
    for (;;) {
      const uint32_t old = atomicCAS(&t_key[pos], kInvalidNode, v);
      if (old == v) odd = true;  // a second rank with this id
      if (old == kInvalidNode || old == v) { atomicMin(&t_pos[pos], k); break; }
      pos = (pos + 1) & (tsize - 1);
    }
  }
  const bool has_odd = __ballot(odd) != 0ull;  // wave-uniform
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  constexpr int D = 16 / PER;  // neighbour rows loaded ahead as a block
  uint32_t nxt[D][PER];
  auto load_block = [&](const uint32_t kAD0, uint32_t (&blk)[D][PER]) {
#pragma unroll
    for (int dd = 0; dd < D; ++dd) {
      const uint32_t kAD = kAD0 + dd;
      const uint32_t iD  = kAD + 1 < K ? s_idx[kAD] : kInvalidNode;
#pragma unroll
      for (int u = 0; u < PER; ++u) {
        const uint32_t kDB = lane + 64 * u;
        blk[dd][u] = (kDB < K && iD < n) ? knn[(int64_t)iD * K + kDB] : kInvalidNode;
      }
    }
  };
  load_block(0, nxt);
  for (uint32_t kAD0 = 0; kAD0 + 1 < ((dbg & 1) ? 0u : K); kAD0 += D) {
    uint32_t cur[D][PER];
#pragma unroll
    for (int dd = 0; dd < D; ++dd)
#pragma unroll
      for (int u = 0; u < PER; ++u) cur[dd][u] = nxt[dd][u];
    load_block(kAD0 + D, nxt);
#pragma unroll
    for (int dd = 0; dd < D; ++dd) {
      const uint32_t kAD = kAD0 + dd;
      if (kAD + 1 >= K) break;  // wave-uniform
      const uint32_t iD = s_idx[kAD];
      if (iD >= n) continue;
#pragma unroll
      for (int u = 0; u < PER; ++u) {
        const uint32_t cand = cur[dd][u];
        if (lane + 64 * u >= K) continue;
        if (cand >= n) {  // invalid candidate: the scan matches the first invalid entry of the node's list, if any
          if (has_odd)
            for (uint32_t kAB = kAD + 1; kAB < K; ++kAB)
              if (s_idx[kAB] == cand) { atomicAdd(&s_det[kAB], 1u); break; }
          continue;
        }
        uint32_t pos = (cand * 2654435761u) & (tsize - 1), hit = 0xffffffffu;
        for (;;) {
          const uint32_t key = t_key[pos];
          if (key == cand) { hit = t_pos[pos]; break; }
          if (key == kInvalidNode) break;
          pos = (pos + 1) & (tsize - 1);
        }
        if (hit == 0xffffffffu) continue;  // the node does not list cand
        if (hit > kAD) {
          atomicAdd(&s_det[hit], 1u);
        } else if (has_odd) {  // lowest rank is not behind kAD: a duplicate further down would still count
          for (uint32_t kAB = kAD + 1; kAB < K; ++kAB)
            if (s_idx[kAB] == cand) { atomicAdd(&s_det[kAB], 1u); break; }
        }
      }
    }
    __builtin_amdgcn_wave_barrier();
  }
  for (uint32_t k = lane; k < K; k += 64) {
    uint32_t d = min(s_det[k], 0xffffu);
    if (s_idx[k] >= n) d = 0xffffu;
    s_det[k] = d;
  }
  __builtin_amdgcn_wave_barrier();
  for (uint32_t i = 0; i < ((dbg & 2) ? 0u : out_degree); ++i) {
    uint32_t best = 0xffffffffu;
    for (uint32_t k = lane; k < K; k += 64) {
      uint32_t tag = (s_det[k] << 16) | k;
      if (s_det[k] < 0xffffu && tag < best) best = tag;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) best = min(best, (uint32_t)__shfl_xor((int)best, off, kWave));
    uint32_t sel = kInvalidNode;
    if (best != 0xffffffffu) {
      sel = s_idx[best & 0xffffu];
      for (uint32_t k = lane; k < K; k += 64)
        if (s_idx[k] == sel) s_det[k] = 0xffffu;
    }
    __builtin_amdgcn_wave_barrier();
    if (lane == 0) out[nid * out_degree + i] = sel;
  }
}

// edge list of ranks [r0, r0 + nr) in (rank-major, source-ascending) order: dest[e], e = (k - r0) * n + src
__global__ void edge_dest_kernel(const uint32_t* __restrict__ g, int64_t n, uint32_t degree, uint32_t r0, uint32_t nr,
                                 uint32_t* dest)
{
  int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n * (int64_t)nr) return;
  int64_t k = r0 + e / n, src = e % n;
  uint32_t d = g[src * degree + k];
  dest[e]    = d < n ? d : (uint32_t)(n);  // invalid edges go to the extra bucket n
}

// the first `degree` reverse edges of every node in (rank, source) order, collected rank chunk by rank chunk (a chunk
// holds fewer than 2^32 edges, so n * degree itself is not bounded)
__global__ void append_reverse_kernel(const uint32_t* __restrict__ perm, const uint32_t* __restrict__ off, int64_t n,
                                      uint32_t degree, uint32_t* __restrict__ rev, uint32_t* __restrict__ rev_cnt)
{
  const int64_t nid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (nid >= n) return;
  const uint32_t b = off[nid], e = off[nid + 1];
  const uint32_t c = rev_cnt[nid];
  const uint32_t take = min(e - b, degree - c);
  for (uint32_t t = 0; t < take; ++t) rev[(size_t)nid * degree + c + t] = perm[b + t] % (uint32_t)n;  // source node
  rev_cnt[nid] = c + take;
}

// kern_merge_graph restated: the protected head of a row is its spanning-forest edges (guarantee_connectivity; mst ==
// nullptr otherwise) followed by the pruned edges not among them, at least degree/2 entries; reverse edges are inserted
// behind the protected head.
__global__ __launch_bounds__(256) void merge_graph_kernel(uint32_t* __restrict__ g, int64_t n, uint32_t degree,
                                                          const uint32_t* __restrict__ rev,
                                                          const uint32_t* __restrict__ rev_cnt, int64_t nid0,
                                                          const uint32_t* __restrict__ mst,
                                                          const uint32_t* __restrict__ mst_cnt)
{
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  uint32_t* row  = reinterpret_cast<uint32_t*>(smem) + (size_t)wave * degree;
  const int64_t nid = nid0 + (int64_t)blockIdx.x * 4 + wave;
  if (nid >= n) return;
  uint32_t n_mst = 0;
  if (mst != nullptr) {
    n_mst = min(mst_cnt[nid], degree);
    for (uint32_t i = lane; i < n_mst; i += 64) row[i] = mst[nid * degree + i];
    __builtin_amdgcn_wave_barrier();
    uint32_t out = n_mst;
    for (uint32_t pj = 0; pj < degree && out < degree; ++pj) {
      const uint32_t v = g[nid * degree + pj];
      bool dup = false;
      for (uint32_t m = lane; m < out; m += 64) dup |= row[m] == v;
      if (__ballot(dup) == 0) {
        if (lane == 0) row[out] = v;
        ++out;
      }
      __builtin_amdgcn_wave_barrier();
    }
    for (uint32_t i = out + lane; i < degree; i += 64) row[i] = kInvalidNode;
    __builtin_amdgcn_wave_barrier();
  } else {
    for (uint32_t i = lane; i < degree; i += 64) row[i] = g[nid * degree + i];
    __builtin_amdgcn_wave_barrier();
  }
  const uint32_t prot = max(n_mst, degree / 2);
  if (prot < degree) {
    uint32_t kr = min(rev_cnt[nid], degree);
    while (kr) {
      kr -= 1;
      const uint32_t rv = rev[(size_t)nid * degree + kr];  // source node of the kr-th reverse edge
      // position of rv in the row (degree if absent)
      uint32_t pos = degree;
      for (uint32_t i = lane; i < degree; i += 64)
        if (row[i] == rv) pos = i;
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) pos = min(pos, (uint32_t)__shfl_xor((int)pos, off, kWave));
      if (pos < prot) continue;
      uint32_t num_shift = pos - prot;
      if (pos >= degree) num_shift = degree - prot - 1;
      // shift row[prot .. prot + num_shift) one to the right
      uint32_t tmp[4];
      for (uint32_t c = 0, i = lane; c < 4; ++c, i += 64) tmp[c] = (i < num_shift) ? row[prot + i] : 0;
      __builtin_amdgcn_wave_barrier();
      for (uint32_t c = 0, i = lane; c < 4; ++c, i += 64)
        if (i < num_shift) row[prot + i + 1] = tmp[c];
      if (lane == 0) row[prot] = rv;
      __builtin_amdgcn_wave_barrier();
    }
  }
  for (uint32_t i = lane; i < degree; i += 64) g[nid * degree + i] = row[i];
}

// drop the self match from [n_rows, K + 1] kNN results (rows r0..): keep the first K ids != row
__global__ void strip_self_kernel(const int64_t* __restrict__ ids, int64_t n_rows, int64_t r0, uint32_t K,
                                  uint32_t kp1, uint32_t* __restrict__ knn)
{
  int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_rows) return;
  uint32_t o = 0;
  for (uint32_t j = 0; j < kp1 && o < K; ++j) {
    int64_t v = ids[r * kp1 + j];
    if (v == r0 + r) continue;
    knn[(r0 + r) * K + o++] = (v < 0 || v == INT64_MAX) ? kInvalidNode : (uint32_t)v;
  }
  for (; o < K; ++o) knn[(r0 + r) * K + o] = kInvalidNode;
}

template <typename T>
__global__ void to_float_kernel(const T* __restrict__ in, int64_t n, float* __restrict__ out)
{
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = to_float(in[i]);
}

// exact kNN graph by tiled brute force (small datasets)
template <typename T>
void knn_graph_bruteforce(resources& res, const T* data, int64_t n, int64_t dim, uint32_t K, int metric,
                          uint32_t* knn)
{
  const uint32_t kp1    = (uint32_t)std::min<int64_t>(K + 1, n);
  const bool select_min = metric != M_InnerProduct;
  dev_buf<float> norms;
  if (metric != M_InnerProduct) {
    norms = dev_buf<float>(res, n);
    row_norms<T>(res, data, n, dim, dim, norms.data(), metric == M_CosineExpanded);
  }
  const int64_t m_tile = std::max<int64_t>(1, std::min<int64_t>(n, (int64_t)(res.workspace_limit / 4) / n));
  dev_buf<float> tile(res, (size_t)m_tile * n), dv(res, (size_t)m_tile * kp1);
  dev_buf<int64_t> di(res, (size_t)m_tile * kp1);
  for (int64_t r0 = 0; r0 < n; r0 += m_tile) {
    int64_t mr = std::min(m_tile, n - r0);
    pairwise_distance<T, T>(res, data + r0 * dim, mr, dim, data, n, dim, dim, norms.data() ? norms.data() + r0 : nullptr,
                            norms.data(),
                            metric == M_InnerProduct ? M_InnerProduct : (metric == M_CosineExpanded ? M_CosineExpanded : M_L2Expanded),
                            tile.data(), n);
    select_k<int64_t, int64_t>(res, tile.data(), nullptr, mr, n, n, (int)kp1, dv.data(), di.data(), select_min);
    hipLaunchKernelGGL(strip_self_kernel, dim3(grid_blocks(mr, 256)), dim3(256), 0, res.stream, di.data(), mr, r0, K,
                       kp1, knn);
  }
}

// approximate kNN graph: IVF-PQ search of the dataset against itself + exact refine (cagra_build.cuh:1629-1760)
void knn_graph_ivf_pq(resources& res, const void* data, elem_t et, int64_t n, int64_t dim, uint32_t K, int metric,
                      uint32_t* knn)
{
  ivf_pq_build_params bp;
  bp.metric                   = metric == M_InnerProduct ? M_InnerProduct : (metric == M_CosineExpanded ? M_CosineExpanded : M_L2Expanded);
  bp.n_lists                  = (uint32_t)std::max<int64_t>(1, std::min<int64_t>(65536, (int64_t)std::sqrt((double)n)));
  bp.kmeans_n_iters           = 10;
  bp.kmeans_trainset_fraction = std::min(1.0, std::max(0.02, 2.0e6 / (double)n));
  bp.pq_bits                  = 8;
  bp.pq_dim                   = (uint32_t)std::max<int64_t>(8, std::min<int64_t>(64, round_up(dim / 2, 8)));
  if (res.tune.cagra_pq_lists > 0) bp.n_lists = (uint32_t)res.tune.cagra_pq_lists;
  auto pq = ivf_pq_build(res, bp, data, et, n, dim, false);
  ivf_pq_search_params sp;
  sp.n_probes                = std::max<uint32_t>(8, bp.n_lists / 50);
  if (res.tune.cagra_pq_probes > 0) sp.n_probes = (uint32_t)res.tune.cagra_pq_probes;
  sp.lut_dtype               = 2;
  sp.internal_distance_dtype = 2;
  // a shape of the wide matrix-core path (ivf_pq_wide.hip; 768 dimensions: pq_dim 64 x pq_len 12): scores summed in fp32 - the
  // screen's margin for fp16 sums (6 % of the bound) lets four times the rows through to the exact re-score (measured at 2M x 768:
  // 34 vs 19 ms per batch of 16384; the LUT scan of rounds 1-5: 60 ms)
  if (pqw_shape(pq->rot_dim)) sp.internal_distance_dtype = 0;
  sp.max_internal_batch_size = 16384;
  const int kp1   = (int)K + 1;
  int k_pq        = std::min(256, 2 * kp1);
  if (res.tune.cagra_kpq > 0) k_pq = std::max(kp1, std::min(256, res.tune.cagra_kpq));
  const int64_t b = 16384;
  dev_buf<int64_t> cand(res, (size_t)b * k_pq), ri(res, (size_t)b * kp1);
  dev_buf<float> cd(res, (size_t)b * k_pq), rd(res, (size_t)b * kp1);
  const size_t esz = elem_size(et);
  for (int64_t r0 = 0; r0 < n; r0 += b) {
    int64_t mr      = std::min(b, n - r0);
    const void* qry = static_cast<const char*>(data) + (size_t)r0 * dim * esz;
    ivf_pq_search(res, sp, *pq, qry, et, mr, k_pq, cand.data(), cd.data());
    refine(res, data, et, n, dim, qry, mr, cand.data(), k_pq, std::min(kp1, k_pq), bp.metric, ri.data(), rd.data());
    hipLaunchKernelGGL(strip_self_kernel, dim3(grid_blocks(mr, 256)), dim3(256), 0, res.stream, ri.data(), mr, r0, K,
                       (uint32_t)std::min(kp1, k_pq), knn);
  }
  sync(res);
}

// graph::optimize (graph_core.cuh:1706-1809); guarantee_connectivity adds the spanning-forest pass of cagra_mst.hip
void optimize_graph(resources& res, const uint32_t* knn, int64_t n, uint32_t K, uint32_t degree, uint32_t* graph,
                    bool guarantee_connectivity)
{
  CUVS_EXPECTS(degree <= K, "graph_degree (%u) must not exceed intermediate_graph_degree (%u)", degree, K);
  CUVS_EXPECTS(degree <= 256 && K <= 1024, "cagra: degree <= 256 and intermediate degree <= 1024 supported");
  CUVS_EXPECTS(n < (int64_t(1) << 32) - 1, "cagra: at most 2^32 - 2 rows (uint32 graph)");
  uint32_t tsize = 64;
  while (tsize < 2 * K) tsize <<= 1;
  size_t smem = (size_t)4 * (2 * K + 2 * tsize) * sizeof(uint32_t);
  auto launch_prune = [&](auto per_tag, int64_t r0, int64_t rows) {
    constexpr int PER = decltype(per_tag)::value;
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(prune_kernel<PER>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)smem));
    hipLaunchKernelGGL(prune_kernel<PER>, dim3(grid_blocks(rows, 4)), dim3(256), smem, res.stream, knn, n, K, degree, graph, r0,
                       res.tune.prune_dbg);
  };
  const int64_t slab = int64_t(1) << 25;  // rows per launch of the wave-per-row kernels (2^23 workgroups)
  for (int64_t r0 = 0; r0 < n; r0 += slab) {
    const int64_t rows = std::min(slab, n - r0);
    if (K <= 64)       launch_prune(std::integral_constant<int, 1>{}, r0, rows);
    else if (K <= 128) launch_prune(std::integral_constant<int, 2>{}, r0, rows);
    else if (K <= 256) launch_prune(std::integral_constant<int, 4>{}, r0, rows);
    else if (K <= 512) launch_prune(std::integral_constant<int, 8>{}, r0, rows);
    else               launch_prune(std::integral_constant<int, 16>{}, r0, rows);
  }
  // reverse edges grouped by destination, ordered by (rank, source): the edge list is sorted a chunk of ranks at a
  // time (a chunk stays below 2^32 edges; 100M rows x degree 64 takes two)
  uint32_t ranks = (uint32_t)std::min<int64_t>(degree, std::max<int64_t>(1, ((int64_t(1) << 32) - 1024) / n));
  if (res.tune.cagra_rank_chunk > 0) ranks = (uint32_t)std::min<int>(res.tune.cagra_rank_chunk, (int)degree);
  const int64_t chunk_edges = n * (int64_t)ranks;
  dev_buf<uint32_t> mst, mst_cnt;
  if (guarantee_connectivity) {
    mst     = dev_buf<uint32_t>(res, (size_t)n * degree);
    mst_cnt = dev_buf<uint32_t>(res, n);
    const int64_t left = cagra_mst_optimize(res, knn, n, K, degree, mst.data(), mst_cnt.data());
    if (left > 1)
      fprintf(stderr, "[cuvs_amd] cagra: guarantee_connectivity left %lld components (rows out of protected slots)\n", (long long)left);
  }
  dev_buf<uint32_t> dest(res, chunk_edges), perm(res, chunk_edges), off(res, n + 2), rev(res, (size_t)n * degree), rev_cnt(res, n);
  HIP_TRY(hipMemsetAsync(rev_cnt.data(), 0, rev_cnt.bytes(), res.stream));
  for (uint32_t r0 = 0; r0 < degree; r0 += ranks) {
    const uint32_t nr = std::min(ranks, degree - r0);
    hipLaunchKernelGGL(edge_dest_kernel, dim3(grid_blocks(n * (int64_t)nr, 256)), dim3(256), 0, res.stream, graph, n, degree,
                       r0, nr, dest.data());
    group_by_label(res, dest.data(), n * (int64_t)nr, (uint32_t)(n + 1), perm.data(), off.data());
    hipLaunchKernelGGL(append_reverse_kernel, dim3(grid_blocks(n, 256)), dim3(256), 0, res.stream, perm.data(), off.data(), n,
                       degree, rev.data(), rev_cnt.data());
  }
  for (int64_t r0 = 0; r0 < n; r0 += slab)
    hipLaunchKernelGGL(merge_graph_kernel, dim3(grid_blocks(std::min(slab, n - r0), 4)), dim3(256),
                       (size_t)4 * degree * sizeof(uint32_t), res.stream, graph, n, degree, rev.data(), rev_cnt.data(), r0,
                       (const uint32_t*)mst.data(), (const uint32_t*)mst_cnt.data());
  HIP_TRY(hipGetLastError());
}

// ------------------------------------------------------------------ search
struct search_args {
  const void* data;
  const uint32_t* graph;
  const void* queries;
  const uint32_t* filter_bits;  // optional bitset over source ids (1 keeps)
  const uint32_t* source;       // optional source id of every row (index::source_indices); nullptr: a row is its own source id
  void* out_idx;                // uint32 or int64 [nq, k]
  float* out_dist;
  int64_t n, dim;
  uint32_t degree, itopk, width, max_iter, min_iter, k, np2, hash_bits, reset_interval;
  uint32_t n_distill;  // num_random_samplings: random candidates per seed slot, the nearest one is kept (device_common_jit.cuh:60-83)
  uint64_t rand_xor_mask;
  int is_ip, idx64;    // is_ip: 0 L2, 1 inner product, 2 cosine (1 - q.x / (|q| |x|), |x| from `norms`)
  const float* norms;  // [n] canonical |x| (cosine)
  // optional work counters (cuvsAmdCagraWorkCounters; SURVEY 8d: bytes(q) = n_dist * dim * sizeof(T) + n_iter * degree * 4
  // with n_dist, n_iter MEASURED): [0] rows scored, [1] walk iterations (graph rows read), [2] walkers (waves). One atomic
  // per wave and counter at the end of the walk; nullptr: not counted.
  unsigned long long* work = nullptr;
  // VPQ-compressed rows (cagra_vpq): `data` is null then
  const uint8_t* codes  = nullptr;
  const __half* vq_book = nullptr;
  const __half* pq_book = nullptr;
  uint32_t code_stride = 0, lane_words = 0;
};

// the filter is evaluated on the source id of a row (to_source_index, search_single_cta_jit.cuh:86-87,306-309)
__device__ inline bool filter_keeps(const search_args& a, uint32_t node)
{
  const uint32_t sid = a.source != nullptr ? a.source[node] : node;
  return (a.filter_bits[sid >> 5] >> (sid & 31)) & 1u;
}

__device__ inline uint32_t hash_slot(uint32_t key, uint32_t bits) { return (key ^ (key >> bits)) & ((1u << bits) - 1u); }

// returns true when `key` was not in the table (and is now)
__device__ inline bool hash_insert(uint32_t* table, uint32_t bits, uint32_t key)
{
  const uint32_t mask = (1u << bits) - 1u;
  uint32_t pos        = hash_slot(key, bits);
  for (uint32_t probe = 0; probe <= mask; ++probe) {
    uint32_t old = atomicCAS(&table[pos], kInvalidNode, key);
    if (old == kInvalidNode) return true;
    if (old == key) return false;
    pos = (pos + 1) & mask;
  }
  return false;  // table full: treat as seen
}

__device__ inline uint64_t xorshift64(uint64_t u)
{
  u ^= u >> 12;
  u ^= u << 25;
  u ^= u >> 27;
  return u * 0x2545F4914F6CDD1DULL;
}

// distances of the nodes idx[first .. first+count) to the query; 8 teams of 8 lanes, one row per team.
// Arithmetic (oracle twin: oracle_cagra.c): team lane t accumulates the elements of its 16-byte pieces in
// order with fmaf, then the 8 partial sums are combined by the xor butterfly (1, 2, 4).
template <typename T>
__device__ inline uint32_t team_distances(const T* __restrict__ data, int64_t dim, const float* __restrict__ qf,
                                      uint32_t* __restrict__ keys, const uint32_t* __restrict__ idx, uint32_t first,
                                      uint32_t count, int is_ip, int lane, const float* __restrict__ norms = nullptr,
                                      float qn = 1.f)
{
  constexpr int VL = 16 / sizeof(T);
  const int team = lane >> 3, tl = lane & 7;
  const bool vec = (dim % VL == 0) && ((reinterpret_cast<uintptr_t>(data) & 15) == 0);
  uint32_t n_scored = 0u;  // rows whose distance was computed (children already in the hash are skipped)
  for (uint32_t c0 = 0; c0 < count; c0 += 8) {
    const uint32_t c    = c0 + team;
    const uint32_t node = c < count ? (idx[first + c] & ~kParentFlag) : kInvalidNode;
    const bool ok       = c < count && idx[first + c] != kInvalidNode;
    n_scored += (uint32_t)__popcll(__ballot(ok && tl == 0));
    float acc           = 0.f;
    if (ok) {
      const T* row = data + (int64_t)node * dim;
      int64_t d0   = (int64_t)tl * VL;
      auto accumulate = [&](const uint4& w, const int64_t dd) {
        const T* el = reinterpret_cast<const T*>(&w);
#pragma unroll
        for (int e = 0; e < VL; ++e) {
          const float x = to_float(el[e]), q = qf[dd + e];
          if (is_ip) {
            acc = __fmaf_rn(x, q, acc);
          } else {
            float t = x - q;
            acc     = __fmaf_rn(t, t, acc);
          }
        }
      };
      if (vec) {
        // four 16-byte pieces in flight per lane (the walk is bound by the latency of these dependent row gathers);
        // the pieces are accumulated in the same order as one at a time
        constexpr int64_t S = 8 * VL;
        for (; d0 + 3 * S < dim; d0 += 4 * S) {
          const uint4 w0 = *reinterpret_cast<const uint4*>(row + d0);
          const uint4 w1 = *reinterpret_cast<const uint4*>(row + d0 + S);
          const uint4 w2 = *reinterpret_cast<const uint4*>(row + d0 + 2 * S);
          const uint4 w3 = *reinterpret_cast<const uint4*>(row + d0 + 3 * S);
          accumulate(w0, d0); accumulate(w1, d0 + S); accumulate(w2, d0 + 2 * S); accumulate(w3, d0 + 3 * S);
        }
      }
      for (; d0 < dim; d0 += 8 * VL) {
        T el[VL];
        if (vec) {
          *reinterpret_cast<uint4*>(el) = *reinterpret_cast<const uint4*>(row + d0);
        } else {
#pragma unroll
          for (int e = 0; e < VL; ++e) el[e] = d0 + e < dim ? row[d0 + e] : T(0);
        }
#pragma unroll
        for (int e = 0; e < VL; ++e) {
          if (d0 + e < dim) {
            const float x = to_float(el[e]), q = qf[d0 + e];
            if (is_ip) {
              acc = __fmaf_rn(x, q, acc);
            } else {
              float t = x - q;
              acc     = __fmaf_rn(t, t, acc);
            }
          }
        }
      }
    }
    acc = acc + __shfl_xor(acc, 1, kWave);
    acc = acc + __shfl_xor(acc, 2, kWave);
    acc = acc + __shfl_xor(acc, 4, kWave);
    if (is_ip == 2 && ok) acc = 1.0f - acc / (qn * norms[node]);  // the brute-force cosine epilogue
    if (tl == 0 && c < count) keys[first + c] = ok ? float_to_key(is_ip == 1 ? -acc : acc) : 0xffffffffu;
  }
  return n_scored;
}

// BitwiseHamming distances of the nodes idx[first .. first+count) to the query (uint8 / int8 rows, compared as bytes): the same
// 8 teams of 8 lanes and 16-byte pieces as team_distances; lane t XORs its pieces with the query's (staged in LDS as bytes)
// and counts the set bits, the 8 counts are summed by the xor butterfly. The count is the distance (exact in fp32).
__device__ inline uint32_t team_hamming(const uint8_t* __restrict__ data, int64_t dim, const uint8_t* __restrict__ qb,
                                        uint32_t* __restrict__ keys, const uint32_t* __restrict__ idx, uint32_t first,
                                        uint32_t count, int lane)
{
  const int team = lane >> 3, tl = lane & 7;
  const bool vec = (dim % 16 == 0) && ((reinterpret_cast<uintptr_t>(data) & 15) == 0);
  auto bits = [](const uint4& w, const uint4& q) {
    return (uint32_t)(__popc(w.x ^ q.x) + __popc(w.y ^ q.y) + __popc(w.z ^ q.z) + __popc(w.w ^ q.w));
  };
  uint32_t n_scored = 0u;
  for (uint32_t c0 = 0; c0 < count; c0 += 8) {
    const uint32_t c    = c0 + team;
    const uint32_t node = c < count ? (idx[first + c] & ~kParentFlag) : kInvalidNode;
    const bool ok       = c < count && idx[first + c] != kInvalidNode;
    n_scored += (uint32_t)__popcll(__ballot(ok && tl == 0));
    uint32_t cnt = 0u;
    if (ok) {
      const uint8_t* row = data + (int64_t)node * dim;
      int64_t d0         = (int64_t)tl * 16;
      if (vec) {
        // four 16-byte pieces in flight per lane, as in team_distances
        for (; d0 + 3 * 128 < dim; d0 += 4 * 128) {
          const uint4 w0 = *reinterpret_cast<const uint4*>(row + d0);
          const uint4 w1 = *reinterpret_cast<const uint4*>(row + d0 + 128);
          const uint4 w2 = *reinterpret_cast<const uint4*>(row + d0 + 256);
          const uint4 w3 = *reinterpret_cast<const uint4*>(row + d0 + 384);
          cnt += bits(w0, *reinterpret_cast<const uint4*>(qb + d0)) + bits(w1, *reinterpret_cast<const uint4*>(qb + d0 + 128)) +
                 bits(w2, *reinterpret_cast<const uint4*>(qb + d0 + 256)) + bits(w3, *reinterpret_cast<const uint4*>(qb + d0 + 384));
        }
        for (; d0 < dim; d0 += 128)
          cnt += bits(*reinterpret_cast<const uint4*>(row + d0), *reinterpret_cast<const uint4*>(qb + d0));
      } else {  // byte tail: the 16 bytes of a piece are loaded first (clamped index, no branch), then counted
        for (; d0 < dim; d0 += 128) {
          uint32_t w[16];
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const int64_t d = min(d0 + e, dim - 1);
            w[e]            = (uint32_t)(row[d] ^ qb[d]);
          }
#pragma unroll
          for (int e = 0; e < 16; ++e) cnt += d0 + e < dim ? (uint32_t)__popc(w[e]) : 0u;
        }
      }
    }
    cnt += (uint32_t)__shfl_xor((int)cnt, 1, kWave);
    cnt += (uint32_t)__shfl_xor((int)cnt, 2, kWave);
    cnt += (uint32_t)__shfl_xor((int)cnt, 4, kWave);
    if (tl == 0 && c < count) keys[first + c] = ok ? float_to_key((float)cnt) : 0xffffffffu;
  }
  return n_scored;
}

// L2 distances of the nodes idx[first .. first+count) of a VPQ-compressed dataset to the query: team_distances<float> on the
// decoded row x[d] = float(vq_book[label][d]) + float(pq_book[code[d / PL]][d % PL]) (one fp32 addition of two fp16 values),
// same teams, same 4-element pieces at d = 4 t + 32 j, same order, same butterfly - so a search over the decoded fp32 rows
// returns the same bits. Per row a lane reads the label, its own code bytes (contiguous in memory, 16 of them per load: 16
// pieces at PL 4, 8 at PL 2), then per group of four pieces the four 8-byte pieces of the VQ centre (global memory; the table
// is small and shared by all rows of a centre) and the PQ entries from the book staged in LDS (`book`: one 32-bit word per
// entry at PL 2, two at PL 4).
typedef uint32_t vpq_words4 __attribute__((ext_vector_type(4), aligned(4)));

template <int PL>
__device__ inline uint32_t team_vpq_distances(const search_args& a, const uint32_t* __restrict__ book, const float* __restrict__ qf,
                                              uint32_t* __restrict__ keys, const uint32_t* __restrict__ idx, uint32_t first,
                                              uint32_t count, int lane)
{
  static_assert(PL == 2 || PL == 4, "pq_len 2 or 4");
  const int team = lane >> 3, tl = lane & 7;
  const int64_t dim = a.dim;
  const bool vec    = (dim & 3) == 0;  // the 4-element pieces of a VQ row are whole and 8-byte aligned
  uint32_t n_scored = 0u;
  for (uint32_t c0 = 0; c0 < count; c0 += 8) {
    const uint32_t c    = c0 + team;
    const uint32_t node = c < count ? (idx[first + c] & ~kParentFlag) : kInvalidNode;
    const bool ok       = c < count && idx[first + c] != kInvalidNode;
    n_scored += (uint32_t)__popcll(__ballot(ok && tl == 0));
    float acc = 0.f;
    if (ok) {
      const uint8_t* row   = a.codes + (size_t)node * a.code_stride;
      const uint32_t label = *reinterpret_cast<const uint32_t*>(row);
      const uint32_t* cw   = reinterpret_cast<const uint32_t*>(row + 4) + (size_t)tl * a.lane_words;
      const __half* vq     = a.vq_book + (size_t)label * dim;
      // four pieces j0 .. j0 + 3 of this lane; cb: their code bytes, lowest first (4 bytes at PL 4, 8 at PL 2)
      auto score4 = [&](const unsigned long long cb, const int64_t j0) {
        uint2 v[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          const int64_t d = 4 * tl + 32 * (j0 + p);
          v[p]            = make_uint2(0u, 0u);
          if (d < dim) {
            if (vec) {
              v[p] = *reinterpret_cast<const uint2*>(vq + d);
            } else {
              __half* h = reinterpret_cast<__half*>(&v[p]);
#pragma unroll
              for (int e = 0; e < 4; ++e)
                if (d + e < dim) h[e] = vq[d + e];
            }
          }
        }
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          const int64_t d = 4 * tl + 32 * (j0 + p);
          if (d < dim) {
            uint2 b;
            if constexpr (PL == 4) {
              b = *reinterpret_cast<const uint2*>(book + 2u * (uint32_t)((cb >> (8 * p)) & 255u));
            } else {
              b.x = book[(uint32_t)((cb >> (16 * p)) & 255u)];
              b.y = book[(uint32_t)((cb >> (16 * p + 8)) & 255u)];
            }
            const __half* vh = reinterpret_cast<const __half*>(&v[p]);
            const __half* bh = reinterpret_cast<const __half*>(&b);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              if (d + e < dim) {
                const float x = __half2float(vh[e]) + __half2float(bh[e]);
                const float s = x - qf[d + e];
                acc           = __fmaf_rn(s, s, acc);
              }
            }
          }
        }
      };
      for (uint32_t w0 = 0; w0 < a.lane_words; w0 += 4) {
        uint32_t w[4];
        if (w0 + 4 <= a.lane_words) {
          const vpq_words4 t = *reinterpret_cast<const vpq_words4*>(cw + w0);
          w[0] = t.x; w[1] = t.y; w[2] = t.z; w[3] = t.w;
        } else {
#pragma unroll
          for (int u = 0; u < 4; ++u) w[u] = w0 + u < a.lane_words ? cw[w0 + u] : 0u;
        }
        if constexpr (PL == 4) {
#pragma unroll
          for (int u = 0; u < 4; ++u)
            if (w0 + u < a.lane_words) score4(w[u], (int64_t)(w0 + u) * 4);
        } else {
#pragma unroll
          for (int u = 0; u < 4; u += 2)
            if (w0 + u < a.lane_words) score4((unsigned long long)w[u] | ((unsigned long long)w[u + 1] << 32), (int64_t)(w0 + u) * 2);
        }
      }
    }
    acc = acc + __shfl_xor(acc, 1, kWave);
    acc = acc + __shfl_xor(acc, 2, kWave);
    acc = acc + __shfl_xor(acc, 4, kWave);
    if (tl == 0 && c < count) keys[first + c] = ok ? float_to_key(acc) : 0xffffffffu;
  }
  return n_scored;
}

// 32-bit words of LDS that hold the PQ book of a compressed dataset: fp16 [256, PL]
template <int PL>
__host__ __device__ constexpr uint32_t vpq_book_words() { return kVpqBookN * PL / 2; }

// 32-bit words of LDS that hold the query: fp32 elements, or (BitwiseHamming) bytes padded to 16
template <bool HAM>
__host__ __device__ inline int64_t query_words(int64_t dim)
{
  return HAM ? ((dim + 15) & ~int64_t(15)) / 4 : ((dim + 3) & ~int64_t(3));
}

__device__ inline float wave_query_norm(const float* qf, int64_t dim, int lane)
{
  float s = 0.f;
  for (int64_t d = lane; d < dim; d += 64) s = __fmaf_rn(qf[d], qf[d], s);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s = s + __shfl_xor(s, off, kWave);
  return sqrtf(s);
}

// HAM: BitwiseHamming over the bytes of uint8 / int8 rows (T = uint8_t), the query staged as bytes
// PL != 0: a VPQ-compressed dataset with this pq_len (T: the dtype of the queries); the PQ book sits in front of the query
template <typename T, bool HAM = false, int PL = 0>
__global__ __launch_bounds__(64) void cagra_search_kernel(search_args a)
{
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane   = threadIdx.x;
  const int64_t qi = blockIdx.x;
  constexpr uint32_t kBook = vpq_book_words<PL>();
  uint32_t* book   = reinterpret_cast<uint32_t*>(smem);
  float* qf        = reinterpret_cast<float*>(smem) + kBook;
  uint8_t* qb      = reinterpret_cast<uint8_t*>(smem);
  uint32_t* keys   = reinterpret_cast<uint32_t*>(smem) + kBook + query_words<HAM>(a.dim);
  uint32_t* idx    = keys + a.np2;
  uint32_t* table  = idx + a.np2;
  const uint32_t hsize = 1u << a.hash_bits;
  const T* data    = static_cast<const T*>(a.data);

  if constexpr (HAM) {
    for (int64_t d = lane; d < a.dim; d += 64) qb[d] = static_cast<const uint8_t*>(a.queries)[qi * a.dim + d];
  } else {
    for (int64_t d = lane; d < a.dim; d += 64) qf[d] = to_float(static_cast<const T*>(a.queries)[qi * a.dim + d]);
  }
  if constexpr (PL != 0)
    for (uint32_t i = lane; i < kBook; i += 64) book[i] = reinterpret_cast<const uint32_t*>(a.pq_book)[i];
  for (uint32_t i = lane; i < a.np2; i += 64) { keys[i] = 0xffffffffu; idx[i] = kInvalidNode; }
  for (uint32_t i = lane; i < hsize; i += 64) table[i] = kInvalidNode;
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();

  float qn = 1.f;  // cosine: canonical |q| (64 strided fma partial sums + butterfly, as row_norms)
  if (a.is_ip == 2) qn = wave_query_norm(qf, a.dim, lane);

  // ---- seeds (compute_distance_to_random_nodes, device_common_jit.cuh:36-104; call site search_single_cta_jit.cuh:157-171):
  // every slot of the result buffer - itopk + search_width * degree of them - draws num_random_samplings pseudo-random
  // nodes, gid = slot + n_slots * j -> xorshift64(gid ^ rand_xor_mask) % n, and keeps the nearest (the first on ties); a
  // winner that is already in the visited table is dropped. The stream does not depend on the query (as in the reference).
  const uint32_t n_cand = a.width * a.degree;
  const uint32_t n_seed = a.itopk + n_cand;
  uint32_t* tkeys   = table + hsize;
  uint32_t* tidx    = tkeys + n_seed;
  uint32_t* parents = tidx + n_seed;  // [width]
  uint32_t n_dist = 0u;
  for (uint32_t j = 0; j < a.n_distill; ++j) {
    for (uint32_t i = lane; i < n_seed; i += 64) {
      const uint64_t gid = (uint64_t)i + (uint64_t)n_seed * j;
      tidx[i]            = (uint32_t)(xorshift64(gid ^ a.rand_xor_mask) % (uint64_t)a.n);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if constexpr (PL != 0) n_dist += team_vpq_distances<PL>(a, book, qf, tkeys, tidx, 0, n_seed, lane);
    else if constexpr (HAM) n_dist += team_hamming(reinterpret_cast<const uint8_t*>(data), a.dim, qb, tkeys, tidx, 0, n_seed, lane);
    else               n_dist += team_distances<T>(data, a.dim, qf, tkeys, tidx, 0, n_seed, a.is_ip, lane, a.norms, qn);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (uint32_t i = lane; i < n_seed; i += 64)
      if (tkeys[i] < keys[i]) { keys[i] = tkeys[i]; idx[i] = tidx[i]; }
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  for (uint32_t i = lane; i < n_seed; i += 64) {
    const uint32_t node = idx[i];
    if (node != kInvalidNode && !hash_insert(table, a.hash_bits, node)) { idx[i] = kInvalidNode; keys[i] = 0xffffffffu; }
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  uint32_t n_rows_read = 0u;  // graph rows read (parents expanded)

  uint32_t iter         = 0;
  while (true) {
    wave_bitonic_sort<uint32_t>(keys, idx, (int)a.np2);
    if (iter >= a.max_iter) break;
    // hash reset (SMALL hash mode of the reference): keep only the current top list
    if (iter > 0 && a.reset_interval > 0 && (iter % a.reset_interval) == 0) {
      for (uint32_t i = lane; i < hsize; i += 64) table[i] = kInvalidNode;
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
      for (uint32_t i = lane; i < a.itopk; i += 64)
        if (idx[i] != kInvalidNode) hash_insert(table, a.hash_bits, idx[i] & ~kParentFlag);
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
    // ---- pick up to `width` best entries that were not parents yet (pickup_next_parents)
    uint32_t n_parents = 0;
    for (uint32_t base = 0; base < a.itopk && n_parents < a.width; base += 64) {
      const uint32_t i = base + lane;
      const bool cand  = i < a.itopk && idx[i] != kInvalidNode && !(idx[i] & kParentFlag);
      unsigned long long m = __ballot(cand);
      while (m != 0ull && n_parents < a.width) {
        const int src = (int)__ffsll((long long)m) - 1;
        m &= m - 1ull;
        const uint32_t pos = base + src;
        if (lane == 0) { parents[n_parents] = idx[pos]; idx[pos] |= kParentFlag; }
        ++n_parents;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (n_parents == 0 && iter >= a.min_iter) break;
    // ---- children -> candidate region (dedup through the hash)
    for (uint32_t i = lane; i < n_cand; i += 64) {
      const uint32_t w = i / a.degree, c = i % a.degree;
      uint32_t child   = kInvalidNode;
      if (w < n_parents) {
        child = a.graph[(int64_t)parents[w] * a.degree + c];
        if (child >= a.n || !hash_insert(table, a.hash_bits, child)) child = kInvalidNode;
      }
      idx[a.itopk + i]  = child;
      keys[a.itopk + i] = 0xffffffffu;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if constexpr (PL != 0) n_dist += team_vpq_distances<PL>(a, book, qf, keys, idx, a.itopk, n_cand, lane);
    else if constexpr (HAM) n_dist += team_hamming(reinterpret_cast<const uint8_t*>(data), a.dim, qb, keys, idx, a.itopk, n_cand, lane);
    else               n_dist += team_distances<T>(data, a.dim, qf, keys, idx, a.itopk, n_cand, a.is_ip, lane, a.norms, qn);
    n_rows_read += n_parents;
    ++iter;
  }
  if (a.work != nullptr && lane == 0) {
    atomicAdd(&a.work[0], (unsigned long long)n_dist);
    atomicAdd(&a.work[1], (unsigned long long)n_rows_read);
    atomicAdd(&a.work[2], 1ull);
  }

  // ---- results: first k entries of the sorted list that pass the filter
  uint32_t written = 0;
  for (uint32_t base = 0; base < a.itopk && written < a.k; base += 64) {
    const uint32_t i = base + lane;
    bool ok          = i < a.itopk && idx[i] != kInvalidNode;
    uint32_t node    = ok ? (idx[i] & ~kParentFlag) : 0;
    if (ok && a.filter_bits) ok = filter_keeps(a, node);
    const unsigned long long m = __ballot(ok);
    const uint32_t rank        = written + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    if (ok && rank < a.k) {
      float d = key_to_float(keys[i]);
      if (a.is_ip == 1) d = -d;
      a.out_dist[qi * a.k + rank] = d;
      if (a.idx64) static_cast<int64_t*>(a.out_idx)[qi * a.k + rank] = node;
      else         static_cast<uint32_t*>(a.out_idx)[qi * a.k + rank] = node;
    }
    written += (uint32_t)__popcll(m);
  }
  for (uint32_t r = min(written, a.k) + lane; r < a.k; r += 64) {
    a.out_dist[qi * a.k + r] = FLT_MAX;
    if (a.idx64) static_cast<int64_t*>(a.out_idx)[qi * a.k + r] = -1;
    else         static_cast<uint32_t*>(a.out_idx)[qi * a.k + r] = kInvalidNode;
  }
}

// ------------------------------------------------------------------ multi-wave search (small batches)
// The reference's MULTI_CTA mode (search_multi_cta_jit.cuh:33-365) gives every query several CTAs, each with its
// own 32-entry top list and ONE parent per iteration, which claim parents through a per-query "traversed" hash
// table in global memory; a final top-k merges the CTAs' lists. Here the unit is a wave: one workgroup per
// query, W waves, each wave runs the reference's per-CTA loop on its own LDS slice, and the traversed table
// lives in LDS (waves of one workgroup share it, so no global table and no extra merge kernel). Waves do not
// synchronise inside the walk; as in the reference the claim order is a race, so results are equal in quality
// (recall tests) but not bit-reproducible.
constexpr uint32_t kMwTopk = 32;  // per-wave top list (the reference's multi_cta_itopk_size)

struct mw_args {
  search_args s;
  uint32_t n_waves, np2_local, vis_bits, trav_bits, merge_np2;
};

// hash table with removal (hashmap.hpp:37-134 SUPPORT_REMOVE semantics): a removed key leaves key|MSB behind
__device__ inline bool trav_insert(uint32_t* table, uint32_t bits, uint32_t key)
{
  const uint32_t mask = (1u << bits) - 1u, removed = key | kParentFlag;
  uint32_t pos = hash_slot(key, bits);
  for (uint32_t probe = 0; probe <= mask; ++probe) {
    uint32_t old = atomicCAS(&table[pos], kInvalidNode, key);
    if (old == kInvalidNode) return true;
    if (old == key) return false;
    old = atomicCAS(&table[pos], removed, key);
    if (old == removed) return true;
    if (old == key) return false;
    pos = (pos + 1) & mask;
  }
  return false;
}
__device__ inline bool trav_contains(const uint32_t* table, uint32_t bits, uint32_t key)
{
  const uint32_t mask = (1u << bits) - 1u, removed = key | kParentFlag;
  uint32_t pos = hash_slot(key, bits);
  for (uint32_t probe = 0; probe <= mask; ++probe) {
    const uint32_t v = table[pos];
    if (v == key) return true;
    if (v == kInvalidNode || v == removed) return false;
    pos = (pos + 1) & mask;
  }
  return false;
}
__device__ inline void trav_remove(uint32_t* table, uint32_t bits, uint32_t key)
{
  const uint32_t mask = (1u << bits) - 1u;
  uint32_t pos = hash_slot(key, bits);
  for (uint32_t probe = 0; probe <= mask; ++probe) {
    const uint32_t old = atomicCAS(&table[pos], key, key | kParentFlag);
    if (old == key || old == kInvalidNode) return;
    pos = (pos + 1) & mask;
  }
}

template <typename T, bool HAM = false, int PL = 0>
__global__ __launch_bounds__(1024) void cagra_search_multi_kernel(mw_args m)
{
  const search_args& a = m.s;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane   = threadIdx.x & 63;
  const int wave   = threadIdx.x >> 6;
  const int64_t qi = blockIdx.x;
  const uint32_t W = m.n_waves, np2 = m.np2_local, vsize = 1u << m.vis_bits, tsize = 1u << m.trav_bits;
  constexpr uint32_t kBook = vpq_book_words<PL>();
  uint32_t* book   = reinterpret_cast<uint32_t*>(smem);
  float* qf        = reinterpret_cast<float*>(smem) + kBook;
  uint8_t* qb      = reinterpret_cast<uint8_t*>(smem);
  uint32_t* trav   = reinterpret_cast<uint32_t*>(smem) + kBook + query_words<HAM>(a.dim);
  uint32_t* mkeys  = trav + tsize;             // merge area [merge_np2]
  uint32_t* midx   = mkeys + m.merge_np2;
  uint32_t* wbase  = midx + m.merge_np2 + (size_t)wave * (2 * np2 + vsize);
  uint32_t* m_tmp  = midx + m.merge_np2 + (size_t)W * (2 * np2 + vsize);  // seed candidates: 2 * degree words per wave
  uint32_t* keys   = wbase;                    // this wave's list: [np2] = 32 top + degree candidates
  uint32_t* idx    = keys + np2;
  uint32_t* vis    = idx + np2;                // this wave's visited table (rebuilt every iteration)
  const T* data    = static_cast<const T*>(a.data);

  if constexpr (HAM) {
    for (int64_t d = threadIdx.x; d < a.dim; d += blockDim.x) qb[d] = static_cast<const uint8_t*>(a.queries)[qi * a.dim + d];
  } else {
    for (int64_t d = threadIdx.x; d < a.dim; d += blockDim.x) qf[d] = to_float(static_cast<const T*>(a.queries)[qi * a.dim + d]);
  }
  if constexpr (PL != 0)
    for (uint32_t i = threadIdx.x; i < kBook; i += blockDim.x) book[i] = reinterpret_cast<const uint32_t*>(a.pq_book)[i];
  for (uint32_t i = threadIdx.x; i < tsize; i += blockDim.x) trav[i] = kInvalidNode;
  for (uint32_t i = lane; i < np2; i += 64) { keys[i] = 0xffffffffu; idx[i] = kInvalidNode; }
  for (uint32_t i = lane; i < vsize; i += 64) vis[i] = kInvalidNode;
  __syncthreads();

  float qn = 1.f;
  if (a.is_ip == 2) qn = wave_query_norm(qf, a.dim, lane);

  // ---- seeds (search_multi_cta_jit.cuh:134-148): `degree` slots per wave, num_random_samplings candidates per slot with
  // gid = wave + W * (slot + degree * j), the nearest kept; a winner already in this wave's visited table is dropped
  uint32_t n_dist = 0u;
  {
    const uint32_t n_seed = min(a.degree, np2);
    uint32_t* tkeys = m_tmp + (size_t)wave * 2 * a.degree;
    uint32_t* tidx  = tkeys + a.degree;
    for (uint32_t j = 0; j < a.n_distill; ++j) {
      for (uint32_t i = lane; i < n_seed; i += 64) {
        const uint64_t gid = (uint64_t)wave + (uint64_t)W * ((uint64_t)i + (uint64_t)n_seed * j);
        tidx[i]            = (uint32_t)(xorshift64(gid ^ a.rand_xor_mask) % (uint64_t)a.n);
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
      if constexpr (PL != 0) n_dist += team_vpq_distances<PL>(a, book, qf, tkeys, tidx, 0, n_seed, lane);
      else if constexpr (HAM) n_dist += team_hamming(reinterpret_cast<const uint8_t*>(data), a.dim, qb, tkeys, tidx, 0, n_seed, lane);
      else               n_dist += team_distances<T>(data, a.dim, qf, tkeys, tidx, 0, n_seed, a.is_ip, lane, a.norms, qn);
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
      for (uint32_t i = lane; i < n_seed; i += 64)
        if (tkeys[i] < keys[i]) { keys[i] = tkeys[i]; idx[i] = tidx[i]; }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (uint32_t i = lane; i < n_seed; i += 64) {
      const uint32_t node = idx[i];
      if (node != kInvalidNode && !hash_insert(vis, m.vis_bits, node)) { idx[i] = kInvalidNode; keys[i] = 0xffffffffu; }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
  uint32_t n_rows_read = 0u;

  uint32_t iter = 0;
  while (true) {
    wave_bitonic_sort<uint32_t>(keys, idx, (int)np2);
    if (iter + 1 >= a.max_iter) break;
    // ---- next parent (pickup_next_parent, search_multi_cta_helpers.cuh:16-80): the best entry of the first 64
    // that is not a parent yet and that THIS wave manages to claim in the traversed table; entries claimed by
    // another wave are dropped from this list
    uint32_t parent = kInvalidNode;
    {
      const uint32_t e   = lane < (int)np2 ? idx[lane] : kInvalidNode;
      unsigned long long c = __ballot(e != kInvalidNode && !(e & kParentFlag));
      int chosen = -1;
      while (c != 0ull) {
        const int src = (int)__ffsll((long long)c) - 1;
        c &= c - 1ull;
        const uint32_t node = __builtin_amdgcn_readlane(e, src);
        bool mine = false;
        if (lane == 0) mine = trav_insert(trav, m.trav_bits, node);
        mine = __builtin_amdgcn_readfirstlane((int)mine) != 0;
        if (mine) { chosen = src; parent = node; break; }
        if (lane == 0) { idx[src] = kInvalidNode; keys[src] = 0xffffffffu; }
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
      if (chosen >= 0) {
        if (chosen < (int)kMwTopk) {
          if (lane == 0) idx[chosen] = parent | kParentFlag;
        } else {
          // parent found in the overflow half: move it into the last free slot of the top half, if any
          const uint32_t t     = lane < (int)kMwTopk ? idx[lane] : 0u;
          unsigned long long f = __ballot(lane < (int)kMwTopk && t == kInvalidNode);
          if (f == 0ull) {
            if (lane == 0) trav_remove(trav, m.trav_bits, parent);
            parent = kInvalidNode;
          } else if (lane == 0) {
            const int j = 63 - __builtin_clzll(f);
            idx[j] = parent | kParentFlag; keys[j] = keys[chosen];
            idx[chosen] = kInvalidNode;    keys[chosen] = 0xffffffffu;
          }
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
    if (parent == kInvalidNode && iter >= a.min_iter) break;
    // ---- rebuild the visited table from the list; parents pushed out of the top half are released
    for (uint32_t i = lane; i < vsize; i += 64) vis[i] = kInvalidNode;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (uint32_t i = lane; i < np2; i += 64) {
      const uint32_t e = idx[i];
      if (e == kInvalidNode) continue;
      if (i >= kMwTopk && (e & kParentFlag)) {
        trav_remove(trav, m.trav_bits, e & ~kParentFlag);
        idx[i] = kInvalidNode; keys[i] = 0xffffffffu;
      } else {
        hash_insert(vis, m.vis_bits, e & ~kParentFlag);
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    // ---- children of the parent -> candidate region
    for (uint32_t c = lane; c < np2 - kMwTopk; c += 64) {
      uint32_t child = kInvalidNode;
      if (parent != kInvalidNode && c < a.degree) {
        child = a.graph[(int64_t)parent * a.degree + c];
        if (child >= a.n || !hash_insert(vis, m.vis_bits, child)) child = kInvalidNode;
      }
      idx[kMwTopk + c]  = child;
      keys[kMwTopk + c] = 0xffffffffu;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if constexpr (PL != 0) n_dist += team_vpq_distances<PL>(a, book, qf, keys, idx, kMwTopk, a.degree, lane);
    else if constexpr (HAM) n_dist += team_hamming(reinterpret_cast<const uint8_t*>(data), a.dim, qb, keys, idx, kMwTopk, a.degree, lane);
    else               n_dist += team_distances<T>(data, a.dim, qf, keys, idx, kMwTopk, a.degree, a.is_ip, lane, a.norms, qn);
    n_rows_read += parent != kInvalidNode ? 1u : 0u;
    // ---- drop what another wave has expanded meanwhile; a parent that fails the filter leaves the list
    for (uint32_t i = lane; i < np2; i += 64) {
      const uint32_t e = idx[i];
      if (e == kInvalidNode) continue;
      bool drop = false;
      if (!(e & kParentFlag)) {
        drop = trav_contains(trav, m.trav_bits, e);
      } else if (a.filter_bits != nullptr && (e & ~kParentFlag) == parent) {
        drop = !filter_keeps(a, parent);
      }
      if (drop) { idx[i] = kInvalidNode; keys[i] = 0xffffffffu; }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    ++iter;
  }

  if (a.work != nullptr && lane == 0) {
    atomicAdd(&a.work[0], (unsigned long long)n_dist);
    atomicAdd(&a.work[1], (unsigned long long)n_rows_read);
    atomicAdd(&a.work[2], 1ull);
  }
  // ---- this wave's 32 results: parents are unique by construction, the others must win the traversed table
  // (duplicates across waves lose); filtered-out nodes are dropped
  {
    uint32_t e = lane < (int)kMwTopk ? idx[lane] : kInvalidNode;
    uint32_t kk = lane < (int)kMwTopk ? keys[lane] : 0xffffffffu;
    bool ok = e != kInvalidNode;
    const uint32_t node = e & ~kParentFlag;
    if (ok && a.filter_bits) ok = filter_keeps(a, node);
    if (ok && !(e & kParentFlag)) ok = trav_insert(trav, m.trav_bits, node);
    if (lane < (int)kMwTopk) {
      mkeys[wave * kMwTopk + lane] = ok ? kk : 0xffffffffu;
      midx[wave * kMwTopk + lane]  = ok ? node : kInvalidNode;
    }
  }
  for (uint32_t i = W * kMwTopk + threadIdx.x; i < m.merge_np2; i += blockDim.x) { mkeys[i] = 0xffffffffu; midx[i] = kInvalidNode; }
  __syncthreads();
  if (wave != 0) return;
  wave_bitonic_sort<uint32_t>(mkeys, midx, (int)m.merge_np2);
  for (uint32_t r = lane; r < a.k; r += 64) {
    const bool ok  = r < m.merge_np2 && midx[r] != kInvalidNode;
    float d        = ok ? key_to_float(mkeys[r]) : FLT_MAX;
    if (ok && a.is_ip == 1) d = -d;
    a.out_dist[qi * a.k + r] = d;
    if (a.idx64) static_cast<int64_t*>(a.out_idx)[qi * a.k + r] = ok ? (int64_t)midx[r] : -1;
    else         static_cast<uint32_t*>(a.out_idx)[qi * a.k + r] = ok ? midx[r] : kInvalidNode;
  }
}

template <typename T, bool HAM = false, int PL = 0>
void launch_search_multi(resources& res, const mw_args& m, int64_t nq, size_t smem)
{
  auto kern = cagra_search_multi_kernel<T, HAM, PL>;
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
  profile_begin(res, "cagra_search_multi_kernel");
  hipLaunchKernelGGL(kern, dim3((unsigned)nq), dim3(64 * m.n_waves), smem, res.stream, m);
  profile_end(res, "cagra_search_multi_kernel");
  HIP_TRY(hipGetLastError());
}

template <typename T, bool HAM = false, int PL = 0>
void launch_search(resources& res, const search_args& a, int64_t nq, size_t smem)
{
  auto kern = cagra_search_kernel<T, HAM, PL>;
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
  profile_begin(res, "cagra_search_kernel");
  hipLaunchKernelGGL(kern, dim3((unsigned)nq), dim3(64), smem, res.stream, a);
  profile_end(res, "cagra_search_kernel");
  HIP_TRY(hipGetLastError());
}

// the walks over a VPQ-compressed dataset: T is the dtype of the queries
template <int PL>
void launch_search_vpq(resources& res, elem_t qt, const search_args& a, const mw_args* m, int64_t nq, size_t smem)
{
  switch (qt) {
    case elem_t::f32: m ? launch_search_multi<float, false, PL>(res, *m, nq, smem) : launch_search<float, false, PL>(res, a, nq, smem); break;
    case elem_t::f16: m ? launch_search_multi<__half, false, PL>(res, *m, nq, smem) : launch_search<__half, false, PL>(res, a, nq, smem); break;
    case elem_t::i8: m ? launch_search_multi<int8_t, false, PL>(res, *m, nq, smem) : launch_search<int8_t, false, PL>(res, a, nq, smem); break;
    case elem_t::u8: m ? launch_search_multi<uint8_t, false, PL>(res, *m, nq, smem) : launch_search<uint8_t, false, PL>(res, a, nq, smem); break;
  }
}

}  // namespace

__global__ void popcount_kernel(const uint32_t* __restrict__ bits, int64_t n_bits, unsigned long long* __restrict__ out)
{
  const int64_t n_words = (n_bits + 31) / 32;
  unsigned long long c  = 0;
  for (int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; w < n_words; w += (int64_t)gridDim.x * blockDim.x) {
    uint32_t v = bits[w];
    if (w == n_words - 1 && (n_bits & 31)) v &= (1u << (n_bits & 31)) - 1u;
    c += (unsigned)__popc(v);
  }
  for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(out, c);
}

int64_t count_set_bits(resources& res, const uint32_t* bits, int64_t n_bits)
{
  dev_buf<unsigned long long> cnt(res, 1);
  HIP_TRY(hipMemsetAsync(cnt.data(), 0, sizeof(unsigned long long), res.stream));
  hipLaunchKernelGGL(popcount_kernel, dim3(256), dim3(256), 0, res.stream, bits, n_bits, cnt.data());
  unsigned long long h = 0;
  HIP_TRY(hipMemcpyAsync(&h, cnt.data(), sizeof(h), hipMemcpyDeviceToHost, res.stream));
  HIP_TRY(hipStreamSynchronize(res.stream));
  return (int64_t)h;
}

// rows whose source id has its bit set (an index with source_indices: the filter is a bitset over source ids)
__global__ void count_kept_rows_kernel(const uint32_t* __restrict__ bits, const uint32_t* __restrict__ source, int64_t n,
                                       unsigned long long* __restrict__ out)
{
  unsigned long long c = 0;
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t sid = source[r];
    c += (bits[sid >> 5] >> (sid & 31)) & 1u;
  }
  for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(out, c);
}

int64_t count_kept_rows(resources& res, const uint32_t* bits, const uint32_t* source, int64_t n)
{
  dev_buf<unsigned long long> cnt(res, 1);
  HIP_TRY(hipMemsetAsync(cnt.data(), 0, sizeof(unsigned long long), res.stream));
  hipLaunchKernelGGL(count_kept_rows_kernel, dim3(256), dim3(256), 0, res.stream, bits, source, n, cnt.data());
  unsigned long long h = 0;
  HIP_TRY(hipMemcpyAsync(&h, cnt.data(), sizeof(h), hipMemcpyDeviceToHost, res.stream));
  HIP_TRY(hipStreamSynchronize(res.stream));
  return (int64_t)h;
}

// ------------------------------------------------------------------ search plan (host only)
// The reference's plan rules restated (search_plan.cuh): algorithm choice of AUTO (:121-131), adjust_search_params
// (:199-245: max_iterations, the filter-rate dependent itopk of MULTI_CTA, itopk rounded to 32) and calc_hashmap_params
// (:248-340: small-hash bit length and reset interval of SINGLE_CTA, visited / traversed hash sizes and CTAs per query
// of MULTI_CTA). `ref_*` fields are what the reference would run with; `run_*` fields are what this library launches
// (see cagra_search for the two places it deliberately differs: AUTO and the LDS hash sizing).
struct cagra_plan {
  uint32_t itopk, max_iterations, search_width;
  int ref_algo;                                   // SINGLE_CTA / MULTI_CTA / MULTI_KERNEL after AUTO resolution
  uint32_t ref_small_hash_bitlen, ref_hash_bitlen, ref_small_hash_reset_interval, ref_mc_num_cta_per_query;
  uint32_t mc_max_iterations;                     // max_iterations if the multi-CTA rule applies (itopk 32 per CTA)
  int run_algo;
  uint32_t run_waves_per_query;
};

inline uint32_t hash_size_of(uint32_t bitlen) { return 1u << bitlen; }  // hashmap.hpp:23

cagra_plan make_cagra_plan(const cuvsCagraSearchParams& p, int64_t n_rows, uint32_t degree, uint32_t topk, int64_t n_queries,
                           int num_cus, float filtering_rate)
{
  cagra_plan pl{};
  const uint32_t width = (uint32_t)std::max<size_t>(1, p.search_width);
  pl.search_width      = width;
  size_t itopk         = std::max<size_t>(p.itopk_size ? p.itopk_size : 64, (size_t)topk);
  // ---- algorithm: search_plan.cuh:121-131 (persistent mode is not offered by the C search entry point)
  int algo = (int)p.algo;
  const size_t max_queries = p.max_queries ? p.max_queries : (size_t)n_queries;  // cagra.cuh: max_queries = min(n_queries, ...)
  if (algo == (int)AUTO) algo = (itopk <= 512 && max_queries >= (size_t)num_cus * 2) ? (int)SINGLE_CTA : (int)MULTI_CTA;
  pl.ref_algo = algo;
  auto reach_iterations = [&](uint32_t it) {
    int64_t reach = 1;
    while (reach < n_rows) { reach *= std::max<int64_t>(2, degree / 2); it += 1; }
    return it;
  };
  // ---- adjust_search_params :199-245
  uint32_t max_it = (uint32_t)p.max_iterations;
  if (p.max_iterations == 0) max_it = reach_iterations(algo == (int)MULTI_CTA ? 32u / 1u : (uint32_t)(itopk / width));
  // the reference tests the ORIGINAL field (search_plan.cuh:216): with max_iterations = 0 and min_iterations > 0 the walk
  // runs exactly min_iterations, not the reach-based count
  if ((uint32_t)p.max_iterations < (uint32_t)p.min_iterations) max_it = (uint32_t)p.min_iterations;
  pl.max_iterations    = std::max<uint32_t>(max_it, (uint32_t)p.max_iterations);
  pl.mc_max_iterations = (uint32_t)p.max_iterations < (uint32_t)p.min_iterations
                           ? (uint32_t)p.min_iterations
                           : (p.max_iterations ? (uint32_t)p.max_iterations : reach_iterations(32u));
  if (algo == (int)MULTI_CTA && filtering_rate > 0.f && filtering_rate < 1.f) {
    size_t adj = (size_t)((float)topk / (1.0 - filtering_rate) + (float)(itopk - topk) / std::sqrt(1.0 - filtering_rate));
    if (adj % 32) adj += 32 - adj % 32;
    if (itopk < adj) itopk = adj;
  }
  if (itopk % 32) itopk += 32 - itopk % 32;
  pl.itopk = (uint32_t)itopk;
  // ---- calc_hashmap_params :248-340
  const float fill = p.hashmap_max_fill_rate > 0.f ? p.hashmap_max_fill_rate : 0.5f;
  const uint32_t min_user = (uint32_t)p.hashmap_min_bitlen;
  pl.ref_small_hash_reset_interval = 1024 * 1024;
  if (algo == (int)MULTI_CTA) {
    pl.ref_mc_num_cta_per_query = (uint32_t)std::max<size_t>(width, (itopk + 31) / 32);
    const uint32_t max_visited  = 32 + degree * 2;
    uint32_t sb = 8;
    while ((float)max_visited > hash_size_of(sb) * fill) ++sb;
    pl.ref_small_hash_bitlen = sb;
    const size_t max_trav = (size_t)pl.ref_mc_num_cta_per_query * std::max<size_t>(32, pl.max_iterations);
    uint32_t hb = std::max<uint32_t>(11, min_user);
    while ((float)max_trav > hash_size_of(hb) * fill) ++hb;
    pl.ref_hash_bitlen = hb;
  } else {
    uint32_t hb = 0;
    if (p.hashmap_mode == AUTO_HASH || p.hashmap_mode == SMALL) {
      const size_t max_visited = itopk + (size_t)width * degree;
      hb = std::max<uint32_t>(8, min_user);
      while ((float)max_visited > hash_size_of(hb) * fill) ++hb;
      if (hb > 13) {
        CUVS_EXPECTS(p.hashmap_mode == AUTO_HASH, "small-hash cannot be used because the required hash size exceeds the limit (%u)",
                     hash_size_of(13));
        hb = 0;
      } else {
        pl.ref_small_hash_bitlen = hb;
        uint32_t interval = 1;
        while ((float)(itopk + (size_t)width * degree * (interval + 1)) <= hash_size_of(hb) * fill) ++interval;
        pl.ref_small_hash_reset_interval = interval;
      }
    }
    if (hb == 0) {
      const size_t max_visited = itopk + (size_t)width * degree * pl.max_iterations;
      hb = std::max<uint32_t>(11, min_user);
      while ((float)max_visited > hash_size_of(hb) * fill) ++hb;
      CUVS_EXPECTS(hb <= 20, "hash_bitlen cannot be largen than 20 (1M). You can decrease itopk_size, search_width or "
                             "max_iterations to reduce the required hashmap size.");
    }
    pl.ref_hash_bitlen = hb;
  }
  return pl;
}

// rows -> source ids of an index that carries them (search_multi_cta.cuh:266-272, search_multi_kernel.cuh:658-668); slots without a
// neighbour stay as they are. n: entries of `source` itself
__global__ void cagra_source_ids_kernel(void* out_idx, int64_t n_out, int idx64, const uint32_t* __restrict__ source, int64_t n)
{
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_out) return;
  if (idx64) {
    int64_t* o = static_cast<int64_t*>(out_idx);
    if (o[t] >= 0 && o[t] < n) o[t] = (int64_t)source[o[t]];
  } else {
    uint32_t* o = static_cast<uint32_t*>(out_idx);
    if ((int64_t)o[t] < n) o[t] = source[o[t]];
  }
}

void cagra_search(resources& res, const cagra_index& idx, const cuvsCagraSearchParams& p, const void* queries,
                  int64_t nq, int k, void* out_idx, bool idx64, float* out_dist, const uint32_t* filter_bits)
{
  if (nq == 0) return;
  const bool vpq = idx.vpq.on();
  CUVS_EXPECTS(idx.graph.data() != nullptr && (idx.data != nullptr || vpq), "cagra index has no graph/dataset");
  CUVS_EXPECTS(k >= 1, "k must be positive");
  CUVS_EXPECTS(nq < (int64_t(1) << 24), "cagra::search: split the query batch (max 2^24 queries per call)");
  search_args a;
  a.data = idx.data; a.graph = idx.graph.data(); a.queries = queries; a.filter_bits = filter_bits;
  a.source = idx.source_indices.data();
  if (vpq) {
    CUVS_EXPECTS(idx.metric == M_L2Expanded, "VPQ compression is only supported with L2Expanded distance mertric");
    a.codes = idx.vpq.codes.data(); a.vq_book = idx.vpq.vq_book.data(); a.pq_book = idx.vpq.pq_book.data();
    a.code_stride = idx.vpq.stride; a.lane_words = idx.vpq.lane_bytes / 4;
  }
  CUVS_EXPECTS(a.source == nullptr || (int64_t)idx.source_indices.size() == idx.n, "cagra::search: %zu source ids for %ld rows",
               idx.source_indices.size(), (long)idx.n);
  a.out_idx = out_idx; a.out_dist = out_dist; a.n = idx.n; a.dim = idx.dim; a.degree = idx.degree;
  a.width = (uint32_t)std::max<size_t>(1, p.search_width);
  a.n_distill = (uint32_t)std::max<uint32_t>(1u, p.num_random_samplings);
  // share of rows the bitset removes: the reference derives it from the bitset's population count when the caller
  // does not give one (cagra.cuh:374-381; the C search params have no such field) and widens the multi-CTA itopk. The
  // bitset is over source ids, so with a map the rows whose source bit is set are counted
  float filtering_rate = 0.f;
  if (filter_bits != nullptr) {
    const int64_t kept = a.source != nullptr ? count_kept_rows(res, filter_bits, a.source, idx.n)
                                             : count_set_bits(res, filter_bits, idx.n);
    filtering_rate     = std::min(std::max((float)(idx.n - kept) / (float)idx.n, 0.0f), 0.999f);
  }
  const cagra_plan pl = make_cagra_plan(p, idx.n, idx.degree, (uint32_t)k, nq, res.num_cus, filtering_rate);
  const uint32_t itopk = pl.itopk;
  CUVS_EXPECTS(itopk <= 1024, "cagra::search: itopk_size up to 1024 is supported");
  a.itopk    = itopk;
  a.min_iter = (uint32_t)p.min_iterations;
  a.max_iter = pl.max_iterations;
  a.k        = (uint32_t)k;
  a.np2      = (uint32_t)next_pow2((int)(itopk + a.width * idx.degree));
  // LDS hash of the walk: exact (open addressing, no false positives), so its size and reset interval change the
  // number of re-visited rows but never a result; sized for <= 50 % fill like the reference's small hash (plan above)
  uint32_t bits = 11;
  while ((1u << bits) < 2 * (itopk + 2 * a.width * idx.degree)) ++bits;
  bits = std::max<uint32_t>(bits, (uint32_t)p.hashmap_min_bitlen);
  CUVS_EXPECTS(bits <= 15, "cagra::search: hash table does not fit the LDS budget");
  a.hash_bits      = bits;
  a.reset_interval = std::max<uint32_t>(1, ((1u << bits) / 2 - itopk) / (a.width * idx.degree));
  a.rand_xor_mask  = p.rand_xor_mask;
  // BitwiseHamming walks its own instantiation of the kernels (popcounts over the row bytes); every other metric keeps the
  // L2 / inner product / cosine arithmetic it always had
  const bool ham = idx.metric == M_BitwiseHamming;
  CUVS_EXPECTS(!ham || idx.dtype == elem_t::u8 || idx.dtype == elem_t::i8,
               "BitwiseHamming distance is only supported for int8_t and uint8_t data types. Current data type is not supported.");
  // (a compressed index: the fp16 PQ book, 1 or 2 KB, in front of the query; 16-byte aligned by its size)
  const size_t q_bytes = (size_t)(ham ? query_words<true>(idx.dim) : query_words<false>(idx.dim)) * 4 +
                         (vpq ? (size_t)kVpqBookN * idx.vpq.pq_len * sizeof(__half) : 0);
  a.is_ip          = ham ? 3 : (idx.metric == M_InnerProduct ? 1 : (idx.metric == M_CosineExpanded ? 2 : 0));
  a.norms          = idx.norms.data();
  a.work           = res.cagra_work;
  CUVS_EXPECTS(a.is_ip != 2 || a.norms != nullptr, "cagra::search: cosine index without dataset norms");
  a.idx64          = idx64 ? 1 : 0;
  // ---- algorithm choice: AUTO follows the reference (search_plan.cuh:121-131: one walker per query once the batch
  // alone fills the GPU, several per query otherwise) so that matched parameters walk the graph the same way.
  // CUVS_AMD_CAGRA_AUTO=multi makes AUTO take the multi-wave walk at every batch size (on MI355X it measured faster at
  // equal recall: 1M x 768 fp16, itopk 64, batch 10k: 18.9 vs 26.7 ms).
  int algo = pl.ref_algo;
  if ((int)p.algo == (int)AUTO) {
    if (res.tune.cagra_auto_multi) algo = (int)MULTI_CTA;
    if (!(itopk <= 16 * kMwTopk && idx.degree <= 224 && (size_t)k <= itopk)) algo = (int)SINGLE_CTA;  // limits of the multi-wave walk
  }
  // MULTI_KERNEL (search_multi_kernel.cuh) exists in the reference because an itopk list above 512 entries does not
  // fit one CTA's shared memory there, so the walk is split into sample / top-k / pickup / distance kernels with the
  // list in global memory. 160 KB of LDS holds the 1024-entry list, its merge buffer and the hash of one walk, so the
  // same request runs as the single-workgroup walk here: same traversal, no round trips through HBM between steps.
  if (algo == (int)MULTI_KERNEL) algo = (int)SINGLE_CTA;
  CUVS_EXPECTS(algo == (int)SINGLE_CTA || algo == (int)MULTI_CTA,
               "cagra::search: algo must be SINGLE_CTA, MULTI_CTA, MULTI_KERNEL or AUTO");
  if (algo == (int)MULTI_CTA && idx.degree <= 224) {
    mw_args m;
    m.s = a;
    // waves per query: the reference's num_cta_per_query = max(search_width, itopk / 32) (search_multi_cta.cuh:124),
    // raised while the launch would leave most of the GPU idle
    uint32_t W = (uint32_t)std::max<size_t>(std::max<size_t>(p.search_width, 1), (itopk + kMwTopk - 1) / kMwTopk);
    while (W < 16 && nq * (int64_t)W * 2 <= 4 * (int64_t)res.num_cus) W *= 2;
    W = std::min<uint32_t>(W, 16);
    CUVS_EXPECTS((uint32_t)k <= W * kMwTopk, "`num_cta_per_query` (%u) * 32 must be equal to or greater than `topk` (%d)", W, k);
    m.n_waves   = W;
    m.np2_local = (uint32_t)next_pow2((int)(kMwTopk + idx.degree));
    m.vis_bits  = 8;
    while ((1u << m.vis_bits) < 2 * (kMwTopk + idx.degree)) ++m.vis_bits;
    m.s.max_iter = pl.mc_max_iterations;  // search_plan.cuh:199-215 with the multi-CTA list size
    m.trav_bits  = 11;  // every wave claims <= max_iter parents and inserts <= 32 results; keep the fill <= 50 %
    while ((1u << m.trav_bits) < 2 * W * (m.s.max_iter + kMwTopk)) ++m.trav_bits;
    m.merge_np2 = (uint32_t)next_pow2((int)(W * kMwTopk));
    size_t msmem = q_bytes + ((size_t)4 << m.trav_bits) + (size_t)m.merge_np2 * 8 +
                   (size_t)W * (2 * m.np2_local + (1u << m.vis_bits)) * 4 + (size_t)W * 2 * idx.degree * 4;
    CUVS_EXPECTS(msmem <= 160 * 1024, "cagra::search: dim too large for the multi-wave LDS layout");
    if (vpq) {
      if (idx.vpq.pq_len == 4) launch_search_vpq<4>(res, idx.dtype, a, &m, nq, msmem);
      else                     launch_search_vpq<2>(res, idx.dtype, a, &m, nq, msmem);
    } else if (ham) {
      launch_search_multi<uint8_t, true>(res, m, nq, msmem);
    } else {
      switch (idx.dtype) {
        case elem_t::f32: launch_search_multi<float>(res, m, nq, msmem); break;
        case elem_t::f16: launch_search_multi<__half>(res, m, nq, msmem); break;
        case elem_t::i8: launch_search_multi<int8_t>(res, m, nq, msmem); break;
        case elem_t::u8: launch_search_multi<uint8_t>(res, m, nq, msmem); break;
      }
    }
    if (idx.source_indices.data() != nullptr)
      hipLaunchKernelGGL(cagra_source_ids_kernel, dim3((unsigned)grid_blocks(nq * k, 256)), dim3(256), 0, res.stream, out_idx, nq * (int64_t)k,
                         idx64 ? 1 : 0, idx.source_indices.data(), (int64_t)idx.source_indices.size());
    return;
  }
  size_t smem = q_bytes + (size_t)a.np2 * 8 + ((size_t)4 << bits) +
                (size_t)(2 * (itopk + a.width * idx.degree) + a.width) * 4;  // + seed candidates, parent list
  CUVS_EXPECTS(smem <= 160 * 1024, "cagra::search: dim/itopk too large for LDS");
  if (vpq) {
    if (idx.vpq.pq_len == 4) launch_search_vpq<4>(res, idx.dtype, a, nullptr, nq, smem);
    else                     launch_search_vpq<2>(res, idx.dtype, a, nullptr, nq, smem);
  } else if (ham) {
    launch_search<uint8_t, true>(res, a, nq, smem);
  } else {
    switch (idx.dtype) {
      case elem_t::f32: launch_search<float>(res, a, nq, smem); break;
      case elem_t::f16: launch_search<__half>(res, a, nq, smem); break;
      case elem_t::i8: launch_search<int8_t>(res, a, nq, smem); break;
      case elem_t::u8: launch_search<uint8_t>(res, a, nq, smem); break;
    }
  }
  if (idx.source_indices.data() != nullptr)
    hipLaunchKernelGGL(cagra_source_ids_kernel, dim3((unsigned)grid_blocks(nq * k, 256)), dim3(256), 0, res.stream, out_idx, nq * (int64_t)k,
                       idx64 ? 1 : 0, idx.source_indices.data(), (int64_t)idx.source_indices.size());
}

// ------------------------------------------------------------------ extend (add_nodes.cuh)
// the fields cuvsCagraSearchParamsCreate fills in (c/src/neighbors/cagra.cpp: the defaults of cagra::search_params)
static cuvsCagraSearchParams cagra_default_search_params()
{
  cuvsCagraSearchParams p{};
  p.itopk_size              = 64;
  p.search_width            = 1;
  p.algo                    = AUTO;
  p.hashmap_mode            = AUTO_HASH;
  p.hashmap_max_fill_rate   = 0.5f;
  p.num_random_samplings    = 1;
  p.rand_xor_mask           = 0x128394;
  p.persistent              = false;
  p.persistent_lifetime     = 2;
  p.persistent_device_usage = 1.0f;
  return p;
}

// add_node_core (add_nodes.cuh:24-277) for one chunk: rows n_cur .. n_cur + cm of the host graph `g` ([>= n_cur + cm, degree],
// rows below n_cur filled) from `cand` [cm, 2 degree], the walk's results of the chunk's rows over the first n_cur rows
// (invalid: any id >= n_cur). Integer bookkeeping only; tests/cagra_extend_ref.py restates it line for line.
static void cagra_add_nodes_host(std::vector<uint32_t>& g, const std::vector<uint32_t>& cand, int64_t n_cur, int64_t cm, uint32_t degree)
{
  const uint32_t K = 2 * degree, half = degree / 2;
  const uint64_t n_new = (uint64_t)(n_cur + cm);  // the reference's new_size: rows once this chunk is in
  // step 0 (:40-53): incoming edges of every row of the graph the chunk starts from
  std::vector<uint32_t> incoming((size_t)n_new, 0u);
  for (size_t e = 0; e < (size_t)n_cur * degree; ++e)
    if (g[e] < n_new) ++incoming[g[e]];
  // step 2 (:148-189): the detour count of candidate i is the number of valid candidates j < i whose list holds i; an
  // invalid id gets 2 degree + 1. The lists read are those of rows below n_cur, which step 3 has not touched yet. The
  // reference sorts with std::sort, which leaves ties open; here the sort is stable (nearest first among equal counts).
  std::vector<std::pair<uint32_t, uint32_t>> by_id(K);  // (id, position among the candidates), sorted: id -> positions
  std::vector<uint32_t> count(K), last_j(K), order(K);
  for (int64_t v = 0; v < cm; ++v) {
    const uint32_t* c = cand.data() + (size_t)v * K;
    for (uint32_t i = 0; i < K; ++i) {
      by_id[i]  = {c[i], i};
      count[i]  = (int64_t)c[i] < n_cur ? 0u : K + 1;
      last_j[i] = 0xffffffffu;
      order[i]  = i;
    }
    std::sort(by_id.begin(), by_id.end());
    for (uint32_t j = 0; j < K; ++j) {
      if ((int64_t)c[j] >= n_cur) continue;
      const uint32_t* row = g.data() + (size_t)c[j] * degree;
      for (uint32_t k = 0; k < degree; ++k) {
        auto it = std::lower_bound(by_id.begin(), by_id.end(), std::make_pair(row[k], 0u));
        for (; it != by_id.end() && it->first == row[k]; ++it) {
          const uint32_t i = it->second;
          if (i > j && (int64_t)c[i] < n_cur && last_j[i] != j) { last_j[i] = j; ++count[i]; }  // once per (j, i) (:168-174)
        }
      }
    }
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return count[a] < count[b]; });
    uint32_t* mine = g.data() + (size_t)(n_cur + v) * degree;
    for (uint32_t i = 0; i < degree; ++i) mine[i] = c[order[i]];
  }
  // step 3 (:191-275), row after row: each of the row's degree / 2 first targets gives up the neighbour of its list's tail
  // half that has strictly the most incoming edges (and was not taken for this row yet); the row's own list is its rank
  // list and the evicted ids in turns
  std::vector<uint32_t> rev(half), temp(degree);
  for (int64_t v = 0; v < cm; ++v) {
    const uint32_t me = (uint32_t)(n_cur + v);
    uint32_t* mine    = g.data() + (size_t)me * degree;
    for (uint32_t i = 0; i < half; ++i) {
      const uint32_t target = mine[i];
      if (target >= n_new) CUVS_FAIL("Invalid node ID found in updated_graph (%u)", target);
      uint32_t take_id = (uint32_t)n_new, take_slot = 0, take_count = 0;
      uint32_t* trow = g.data() + (size_t)target * degree;
      for (int32_t j = (int32_t)degree - 1; j >= (int32_t)half; --j) {
        const uint32_t nb = trow[j];
        if (nb >= n_new) CUVS_FAIL("Invalid node ID found in updated_graph (%u)", nb);
        if (incoming[nb] > take_count && std::find(rev.begin(), rev.begin() + i, nb) == rev.begin() + i) {
          take_count = incoming[nb];
          take_id    = nb;
          take_slot  = (uint32_t)j;
        }
      }
      trow[take_slot] = me;
      rev[i]          = take_id;
    }
    incoming[me] = half;
    uint32_t pos[2] = {0, 0}, turn = 0, n_add = 0;
    const uint32_t* list[2] = {mine, rev.data()};
    const uint32_t len[2]   = {degree, half};
    while (n_add < degree && (pos[0] < degree || pos[1] < half)) {
      for (; pos[turn] < len[turn]; ++pos[turn]) {
        const uint32_t cnd = list[turn][pos[turn]];
        if (cnd >= n_new) continue;
        if (std::find(temp.begin(), temp.begin() + n_add, cnd) != temp.begin() + n_add) continue;
        temp[n_add++] = cnd;  // (the position stays, as in the reference: the entry is a duplicate at the next turn)
        break;
      }
      turn = 1 - turn;
    }
    if (n_add < degree)
      CUVS_FAIL("Number of edges is not enough (target_new_node_id:%lu, num_add:%lu, degree:%lu)", (unsigned long)me, (unsigned long)n_add,
                (unsigned long)degree);
    std::copy(temp.begin(), temp.end(), mine);
  }
}

// New rows are added chunk by chunk as in the reference (add_graph_nodes, add_nodes.cuh:279-344): every row of a chunk walks
// the graph of the old rows and the chunks before it for its 2 degree nearest rows (itopk max(4 degree, 256)); the candidates
// are re-ordered by detour count, each of the row's degree / 2 first targets gets a reverse edge in place of the tail
// neighbour with the most incoming edges, and the row's list interleaves its rank list with the evicted ids. The walk runs on
// the device; the re-ordering and the reverse edges are done on the host over a host copy of the graph, as in the reference.
// One deviation: the reference searches with default parameters, whose AUTO may pick the multi-CTA walk, which races for
// parents; the walk here is always the single-workgroup one, so the graph is reproducible (and pinned by a CPU twin).
// The new dataset and graph are built on the side and become the index's only when every chunk has succeeded.
void cagra_extend(resources& res, cagra_index& idx, const void* new_rows, bool new_is_host, int64_t m, uint32_t max_chunk)
{
  // the walk below reports source ids and the new rows would have none: the reference's add_nodes.cuh defines nothing for an
  // index with source_indices, so it is refused before anything is touched
  CUVS_EXPECTS(idx.source_indices.data() == nullptr, "cagra::extend: an index that carries source_indices cannot be extended");
  if (m == 0) return;
  CUVS_EXPECTS(idx.data != nullptr && idx.graph.data() != nullptr, "cagra::extend: index has no graph/dataset");
  CUVS_EXPECTS(idx.n + m < (int64_t(1) << 32) - 1, "cagra: at most 2^32 - 2 rows (uint32 graph)");
  const size_t esz = elem_size(idx.dtype), row_bytes = (size_t)idx.dim * esz;
  const int64_t n0 = idx.n, n1 = idx.n + m;
  const uint32_t degree = idx.degree, K = 2 * degree;
  cagra_index ext;  // the extended index, on the side
  ext.metric = idx.metric; ext.dtype = idx.dtype; ext.dim = idx.dim; ext.degree = degree;
  ext.owned  = dev_buf<char>::persistent((size_t)n1 * row_bytes);
  ext.data   = ext.owned.data();
  ext.graph  = dev_buf<uint32_t>::persistent((size_t)n1 * degree);
  std::vector<uint32_t> g((size_t)n1 * degree, kInvalidNode);
  copy_async(res, ext.owned.data(), idx.data, (size_t)n0 * row_bytes);
  // rows the device cannot reach are host rows; anything else (device, pinned or managed memory) is left to the runtime to place
  HIP_TRY(hipMemcpyAsync(ext.owned.data() + (size_t)n0 * row_bytes, new_rows, (size_t)m * row_bytes,
                         new_is_host ? hipMemcpyHostToDevice : hipMemcpyDefault, res.stream));
  copy_async(res, g.data(), idx.graph.data(), (size_t)n0 * degree * sizeof(uint32_t));
  sync(res);
  cuvsCagraSearchParams sp = cagra_default_search_params();
  sp.itopk_size            = std::max<size_t>(4 * (size_t)degree, 256);  // add_nodes.cuh:69-70
  sp.algo                  = SINGLE_CTA;
  const int64_t chunk = max_chunk == 0 ? m : (int64_t)max_chunk;  // 0: one chunk (add_nodes.cuh:297-298)
  const int64_t batch = std::min<int64_t>(chunk, 65536);          // queries per launch (the chunk decides the graph, not this)
  dev_buf<uint32_t> nb(res, (size_t)batch * K);
  dev_buf<float> nd(res, (size_t)batch * K);
  std::vector<uint32_t> cand, got;
  for (int64_t c0 = 0; c0 < m; c0 += chunk) {
    const int64_t cm = std::min(chunk, m - c0);
    ext.n = n0 + c0;              // the graph searched by this chunk: old rows + the chunks before it
    cagra_set_norms(res, ext);    // cosine: |x| of everything searchable so far
    copy_async(res, ext.graph.data(), g.data(), (size_t)ext.n * degree * sizeof(uint32_t));
    const int k = (int)std::min<int64_t>(K, ext.n);  // a graph of fewer than 2 degree rows: the missing columns stay invalid
    cand.assign((size_t)cm * K, kInvalidNode);
    for (int64_t b0 = 0; b0 < cm; b0 += batch) {
      const int64_t bm = std::min(batch, cm - b0);
      cagra_search(res, ext, sp, static_cast<const char*>(ext.data) + (size_t)(ext.n + b0) * row_bytes, bm, k, nb.data(), false,
                   nd.data(), nullptr);
      got.resize((size_t)bm * k);
      copy_async(res, got.data(), nb.data(), got.size() * sizeof(uint32_t));
      sync(res);
      for (int64_t v = 0; v < bm; ++v)
        for (int j = 0; j < k; ++j) {
          const uint32_t id = got[(size_t)v * k + j];
          if ((int64_t)id < ext.n) cand[(size_t)(b0 + v) * K + j] = id;  // add_nodes.cuh:129,158: anything else is invalid
        }
    }
    cagra_add_nodes_host(g, cand, ext.n, cm, degree);
  }
  copy_async(res, ext.graph.data(), g.data(), g.size() * sizeof(uint32_t));
  ext.n = n1;
  cagra_set_norms(res, ext);
  sync(res);
  idx.owned = std::move(ext.owned);
  idx.data  = idx.owned.data();
  idx.graph = std::move(ext.graph);
  idx.norms = std::move(ext.norms);
  idx.n     = n1;
}

// rows of bytes -> [n, 8 dim] floats of their bits (bit j of byte b -> column 8 b + j): squared L2 over them is the Hamming
// distance, and every product and partial sum of a float GEMM over 0/1 values is a small integer, so it is exact. Grid-stride:
// n x 8 dim elements may exceed what one launch of one element per thread can address
__global__ void expand_bits_kernel(const uint8_t* __restrict__ in, int64_t n_bytes, float* __restrict__ out)
{
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_bytes * 8; i += (int64_t)gridDim.x * blockDim.x)
    out[i] = (float)((in[i >> 3] >> (i & 7)) & 1u);
}

// the kNN graph [n, K] the CAGRA graph is optimised from, by build algorithm (idx: metric, rows, dtype; cosine norms are set
// for NN-descent)
void cagra_knn_graph(resources& res, const cuvsCagraIndexParams& p, cagra_index& idx, uint32_t K, uint32_t* knn)
{
  const int metric = idx.metric;
  const elem_t et  = idx.dtype;
  const int64_t n = idx.n, dim = idx.dim;
  const bool small = n <= 200000 || p.build_algo == ITERATIVE_CAGRA_SEARCH;
  if (metric == M_BitwiseHamming) {
    // NN_DESCENT, or AUTO above 200000 rows (the reference's pick, cagra_build.cuh:2208-2219); otherwise the exact graph
    // over the rows expanded to 0/1 floats (this library's stand-in for ITERATIVE_CAGRA_SEARCH)
    if (p.build_algo == NN_DESCENT || !small) {
      knn_graph_nn_descent(res, idx.data, et, n, dim, K, metric, nullptr, (int)p.nn_descent_niter, knn);
    } else {
      // (scratch: n x 32 dim bytes for the expanded rows)
      dev_buf<float> f(res, (size_t)n * dim * 8);
      hipLaunchKernelGGL(expand_bits_kernel, dim3((unsigned)std::min<int64_t>((n * dim * 8 + 255) / 256, (int64_t)res.num_cus * 64)),
                         dim3(256), 0, res.stream, static_cast<const uint8_t*>(idx.data), n * dim, f.data());
      knn_graph_bruteforce<float>(res, f.data(), n, dim * 8, K, M_L2Expanded, knn);
      sync(res);
    }
    return;
  }
  if (p.build_algo == NN_DESCENT) {
    cagra_set_norms(res, idx);  // cosine: the join needs |x|
    knn_graph_nn_descent(res, idx.data, et, n, dim, K, metric, idx.norms.data(), (int)p.nn_descent_niter, knn);
  } else if (small) {
    if (et == elem_t::f32) {
      knn_graph_bruteforce<float>(res, static_cast<const float*>(idx.data), n, dim, K, metric, knn);
    } else if (et == elem_t::f16) {
      knn_graph_bruteforce<__half>(res, static_cast<const __half*>(idx.data), n, dim, K, metric, knn);
    } else {
      dev_buf<float> f(res, (size_t)n * dim);
      if (et == elem_t::i8)
        hipLaunchKernelGGL((to_float_kernel<int8_t>), dim3(grid_blocks(n * dim, 256)), dim3(256), 0, res.stream,
                           static_cast<const int8_t*>(idx.data), n * dim, f.data());
      else
        hipLaunchKernelGGL((to_float_kernel<uint8_t>), dim3(grid_blocks(n * dim, 256)), dim3(256), 0, res.stream,
                           static_cast<const uint8_t*>(idx.data), n * dim, f.data());
      knn_graph_bruteforce<float>(res, f.data(), n, dim, K, metric, knn);
      sync(res);
    }
  } else {
    knn_graph_ivf_pq(res, idx.data, et, n, dim, K, metric, knn);
  }
}

// metric and dtype checks of a build (the reference's messages for BitwiseHamming: cagra_build.cuh:2220-2237)
void cagra_check_build(const cuvsCagraIndexParams& p, elem_t et)
{
  const int metric = (int)p.metric;
  CUVS_EXPECTS(metric_is_l2(metric) || metric == M_InnerProduct || metric == M_CosineExpanded || metric == M_BitwiseHamming,
               "cagra: unsupported metric %d", metric);
  if (metric != M_BitwiseHamming) return;
  CUVS_EXPECTS(p.build_algo != IVF_PQ,
               "IVF_PQ for CAGRA graph build does not support BitwiseHamming as a metric. Please use nn-descent or the iterative "
               "CAGRA search build.");
  CUVS_EXPECTS(et == elem_t::u8 || et == elem_t::i8,
               "BitwiseHamming distance is only supported for int8_t and uint8_t data types. Current data type is not supported.");
}

// ------------------------------------------------------------------ VPQ compression
// position of subspace s's code among the 8 * lane_bytes code bytes of a row in memory (cagra_vpq)
__host__ __device__ inline uint32_t vpq_code_pos(uint32_t s, uint32_t pq_len, uint32_t lane_bytes)
{
  if (pq_len == 4) return (s & 7u) * lane_bytes + (s >> 3);          // lane s % 8, piece s / 8
  return ((s & 15u) >> 1) * lane_bytes + 2u * (s >> 4) + (s & 1u);   // lane (s % 16) / 2, piece s / 16, its two codes in order
}

// rows in memory from labels (a uint32 every label_pitch bytes) and codes (pq_dim bytes every code_pitch bytes): a thread per
// byte of the output
__global__ void vpq_pack_kernel(const uint8_t* __restrict__ labels, size_t label_pitch, const uint8_t* __restrict__ codes,
                                size_t code_pitch, int64_t n, uint32_t pq_dim, uint32_t pq_len, uint32_t lane_bytes,
                                uint8_t* __restrict__ out)
{
  const uint32_t stride = 4u + 8u * lane_bytes;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n * stride; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r  = t / stride;
    const uint32_t b = (uint32_t)(t - r * stride);
    uint8_t v        = 0;
    if (b < 4) {
      v = labels[(size_t)r * label_pitch + b];
    } else {
      const uint32_t lane = (b - 4) / lane_bytes, k = (b - 4) % lane_bytes;
      const uint32_t sub  = pq_len == 4 ? lane + 8u * k : 2u * lane + 16u * (k >> 1) + (k & 1u);
      if (sub < pq_dim) v = codes[(size_t)r * code_pitch + sub];
    }
    out[t] = v;
  }
}

// rows r0 .. r0 + n in the reference's layout [n, row_len] from the rows in memory: a thread per byte of the output
__global__ void vpq_unpack_kernel(const uint8_t* __restrict__ mem, int64_t n, uint32_t pq_dim, uint32_t pq_len, uint32_t lane_bytes,
                                  uint32_t row_len, uint8_t* __restrict__ out)
{
  const uint32_t stride = 4u + 8u * lane_bytes;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n * row_len; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r  = t / row_len;
    const uint32_t b = (uint32_t)(t - r * row_len);
    const uint8_t* m = mem + (size_t)r * stride;
    out[t]           = b < 4 ? m[b] : (b - 4 < pq_dim ? m[4 + vpq_code_pos(b - 4, pq_len, lane_bytes)] : (uint8_t)0);
  }
}

// the largest label of rows in the reference's layout (an untrusted file: a label indexes the VQ table)
__global__ void vpq_max_label_kernel(const uint8_t* __restrict__ rows, int64_t n, uint32_t row_len, uint32_t* __restrict__ out)
{
  uint32_t mx = 0;
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x)
    mx = max(mx, *reinterpret_cast<const uint32_t*>(rows + (size_t)r * row_len));
  for (int off = 32; off > 0; off >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, off, 64));
  if ((threadIdx.x & 63) == 0) atomicMax(out, mx);
}

// fp32 -> fp16 (round to nearest even); `rounded` (optional, may be `x`) receives the rounded values as fp32
__global__ void vpq_round_book_kernel(const float* x, int64_t n, __half* __restrict__ out, float* rounded)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const __half h = __float2half_rn(x[i]);
  out[i]         = h;
  if (rounded != nullptr) rounded[i] = __half2float(h);
}
void vpq_round_book(resources& res, const float* x, int64_t n, __half* out, float* rounded)
{
  hipLaunchKernelGGL(vpq_round_book_kernel, dim3(grid_blocks(n, 256)), dim3(256), 0, res.stream, x, n, out, rounded);
  HIP_TRY(hipGetLastError());
}

inline unsigned vpq_grid(const resources& res, int64_t items) { return (unsigned)std::min<int64_t>((items + 255) / 256, (int64_t)res.num_cus * 32); }

constexpr int64_t kVpqIoBytes = int64_t(64) << 20;  // rows in the reference's layout pass through buffers of this size

// The rows of a file (the reference's layout, delivered by `read(host buffer, bytes)` in order) become the index's codes, a
// chunk at a time: neither the file's rows nor a second copy of the dataset is ever resident. The file is untrusted: a label
// outside the VQ table is refused (one device reduction per chunk), and the half-filled index is dropped by the caller.
template <typename Read>
void vpq_load_rows(resources& res, cagra_index& idx, Read&& read)
{
  auto& v = idx.vpq;
  CUVS_EXPECTS(idx.n > 0, "cagra::deserialize: the VPQ dataset holds no rows");
  const int64_t step = std::max<int64_t>(1, kVpqIoBytes / v.row_len);
  v.codes = dev_buf<uint8_t>::persistent((size_t)idx.n * v.stride);
  dev_buf<uint8_t> rows(res, (size_t)std::min(step, idx.n) * v.row_len);
  dev_buf<uint32_t> mx(res, 1);
  std::vector<uint8_t> h(rows.size());
  for (int64_t r0 = 0; r0 < idx.n; r0 += step) {
    const int64_t cnt = std::min(step, idx.n - r0);
    read(h.data(), (size_t)cnt * v.row_len);
    copy_async(res, rows.data(), h.data(), (size_t)cnt * v.row_len);
    HIP_TRY(hipMemsetAsync(mx.data(), 0, sizeof(uint32_t), res.stream));
    hipLaunchKernelGGL(vpq_max_label_kernel, dim3(vpq_grid(res, cnt)), dim3(256), 0, res.stream, rows.data(), cnt, v.row_len, mx.data());
    hipLaunchKernelGGL(vpq_pack_kernel, dim3(vpq_grid(res, cnt * (int64_t)v.stride)), dim3(256), 0, res.stream, rows.data(),
                       (size_t)v.row_len, rows.data() + 4, (size_t)v.row_len, cnt, v.pq_dim, v.pq_len, v.lane_bytes,
                       v.codes.data() + (size_t)r0 * v.stride);
    HIP_TRY(hipGetLastError());
    const uint32_t top = read_word(res, mx.data());  // (also: the host buffer is free again)
    CUVS_EXPECTS(top < v.vq_n, "cagra: the VPQ dataset holds the VQ label %u, the VQ codebook has %u centres", top, v.vq_n);
  }
}

// rows r0 .. r0 + cnt of a compressed index in the reference's layout, into `out` (device)
void vpq_export_rows(resources& res, const cagra_index& idx, int64_t r0, int64_t cnt, uint8_t* out)
{
  const auto& v = idx.vpq;
  if (cnt == 0) return;
  hipLaunchKernelGGL(vpq_unpack_kernel, dim3(vpq_grid(res, cnt * (int64_t)v.row_len)), dim3(256), 0, res.stream,
                     v.codes.data() + (size_t)r0 * v.stride, cnt, v.pq_dim, v.pq_len, v.lane_bytes, v.row_len, out);
  HIP_TRY(hipGetLastError());
}

// all rows of a compressed index in the reference's layout, handed to `write(host buffer, bytes)` a chunk at a time
template <typename Write>
void vpq_store_rows(resources& res, const cagra_index& idx, Write&& write)
{
  const auto& v = idx.vpq;
  const int64_t step = std::max<int64_t>(1, kVpqIoBytes / v.row_len);
  dev_buf<uint8_t> rows(res, (size_t)std::min(step, idx.n) * v.row_len);
  std::vector<uint8_t> h(rows.size());
  for (int64_t r0 = 0; r0 < idx.n; r0 += step) {
    const int64_t cnt = std::min(step, idx.n - r0);
    vpq_export_rows(res, idx, r0, cnt, rows.data());
    copy_async(res, h.data(), rows.data(), (size_t)cnt * v.row_len);
    sync(res);
    write(h.data(), (size_t)cnt * v.row_len);
  }
}

// The parameters a compressed build runs with: the zero fields filled by the reference's heuristics
// (vpq_dataset.cuh:124-144), the train-set sizes of make_pq_params_from_vpq (pq.cuh:385-407). Host only; refuses what the
// search over codes does not serve.
struct vpq_plan {
  uint32_t pq_dim, pq_len, vq_n, n_iters, max_pq, max_vq;
  int64_t n_train, n_vq_train;
};
vpq_plan cagra_vpq_plan(const cuvsCagraIndexParams& p, int64_t n, int64_t dim)
{
  const cuvsCagraCompressionParams& c = *p.compression;
  CUVS_EXPECTS((int)p.metric == M_L2Expanded, "VPQ compression is only supported with L2Expanded distance mertric");
  CUVS_EXPECTS(dim > 0 && n > 0, "cagra: empty dataset");
  vpq_plan pl{};
  const uint32_t pq_bits = c.pq_bits == 0 ? 8u : c.pq_bits;
  CUVS_EXPECTS(pq_bits == 8, "cagra: VPQ compression supports pq_bits = 8 only (got %u)", pq_bits);
  pl.pq_dim = c.pq_dim == 0 ? (uint32_t)((dim + 3) / 4) : c.pq_dim;
  CUVS_EXPECTS(dim % pl.pq_dim == 0, "cagra: VPQ compression needs dim (%ld) to be a multiple of pq_dim (%u)", (long)dim, pl.pq_dim);
  pl.pq_len = (uint32_t)(dim / pl.pq_dim);
  CUVS_EXPECTS(pl.pq_len == 2 || pl.pq_len == 4, "cagra: VPQ compression supports pq_len = dim / pq_dim of 2 or 4 only (got %u)", pl.pq_len);
  CUVS_EXPECTS(n >= (int64_t)kVpqBookN, "cagra: VPQ compression needs at least 256 rows to train the PQ codebook (got %ld)", (long)n);
  pl.vq_n = c.vq_n_centers == 0 ? (uint32_t)round_up((int64_t)(uint32_t)std::sqrt((double)n), 8) : c.vq_n_centers;
  CUVS_EXPECTS((int64_t)pl.vq_n <= n, "cagra: vq_n_centers (%u) exceeds the number of rows (%ld)", pl.vq_n, (long)n);
  pl.n_iters = c.kmeans_n_iters;
  CUVS_EXPECTS(pl.n_iters > 0, "cagra: kmeans_n_iters of the compression parameters must be positive");
  const double vq_frac = c.vq_kmeans_trainset_fraction == 0 ? std::min(1.0, 100.0 * pl.vq_n / (double)n) : c.vq_kmeans_trainset_fraction;
  const double pq_frac = c.pq_kmeans_trainset_fraction == 0 ? std::min(1.0, 1000.0 * kVpqBookN / (double)n) : c.pq_kmeans_trainset_fraction;
  CUVS_EXPECTS(vq_frac > 0 && vq_frac <= 1 && pq_frac > 0 && pq_frac <= 1, "cagra: the k-means trainset fractions of the compression parameters must be in (0, 1]");
  pl.max_vq     = (uint32_t)std::min<double>(1024.0, (double)n * vq_frac / pl.vq_n);
  pl.max_pq     = (uint32_t)std::min<double>(256.0, (double)n * pq_frac / kVpqBookN);
  pl.n_train    = std::min<int64_t>(n, (int64_t)pl.max_pq * kVpqBookN);
  pl.n_vq_train = std::min<int64_t>(n, (int64_t)pl.max_vq * pl.vq_n);
  CUVS_EXPECTS(pl.n_train >= (int64_t)kVpqBookN,
               "cagra: the PQ training set of VPQ compression holds %ld rows, at least 256 are needed (pq_kmeans_trainset_fraction)",
               (long)pl.n_train);
  CUVS_EXPECTS(pl.n_vq_train >= (int64_t)pl.vq_n,
               "cagra: the VQ training set of VPQ compression holds %ld rows, vq_n_centers (%u) are needed (vq_kmeans_trainset_fraction)",
               (long)pl.n_vq_train, pl.vq_n);
  return pl;
}

// device rows of any dtype -> fp32 [m, dim]: every row_step-th row from `src` on
void vpq_rows_to_float(resources& res, const void* src, elem_t et, int64_t row_step, int64_t m, int64_t dim, float* out,
                       dev_buf<char>& staging)
{
  const size_t row_bytes = (size_t)dim * elem_size(et);
  const void* packed     = src;
  if (row_step > 1 || et == elem_t::f32) {
    void* dst = et == elem_t::f32 ? static_cast<void*>(out) : static_cast<void*>(staging.data());
    HIP_TRY(hipMemcpy2DAsync(dst, row_bytes, src, row_bytes * (size_t)row_step, row_bytes, (size_t)m, hipMemcpyDefault, res.stream));
    packed = dst;
  }
  const int64_t cnt = m * dim;
  switch (et) {
    case elem_t::f32: break;
    case elem_t::f16:
      hipLaunchKernelGGL((to_float_kernel<__half>), dim3(grid_blocks(cnt, 256)), dim3(256), 0, res.stream, static_cast<const __half*>(packed), cnt, out);
      break;
    case elem_t::i8:
      hipLaunchKernelGGL((to_float_kernel<int8_t>), dim3(grid_blocks(cnt, 256)), dim3(256), 0, res.stream, static_cast<const int8_t*>(packed), cnt, out);
      break;
    case elem_t::u8:
      hipLaunchKernelGGL((to_float_kernel<uint8_t>), dim3(grid_blocks(cnt, 256)), dim3(256), 0, res.stream, static_cast<const uint8_t*>(packed), cnt, out);
      break;
  }
  HIP_TRY(hipGetLastError());
}

// vpq_build restated (pq.cuh:409-442) over the device rows of `idx`: trains the VQ centres and the shared PQ book on strided
// subsamples, rounds both books to fp16 and encodes every row AGAINST THE ROUNDED BOOKS (the reference encodes against the
// fp32 books and rounds afterwards: here the codes are the best ones for the values the search reads). Rows pass through fp32
// a chunk at a time; the original rows are dropped at the end.
void cagra_compress(resources& res, cagra_index& idx, const vpq_plan& pl)
{
  const int64_t n = idx.n, dim = idx.dim;
  const size_t esz = elem_size(idx.dtype);
  auto& v = idx.vpq;
  v.set_shape(dim, pl.vq_n, pl.pq_len);
  std::unique_ptr<product_quantizer> q;
  {
    const int64_t m = std::max(pl.n_train, pl.n_vq_train);  // one strided subsample holds both train sets
    dev_buf<float> train(res, (size_t)(m * dim));
    dev_buf<char> staging;
    if (idx.dtype != elem_t::f32) staging = dev_buf<char>(res, (size_t)m * dim * esz);
    vpq_rows_to_float(res, idx.data, idx.dtype, n / m, m, dim, train.data(), staging);
    cuvsProductQuantizerParams qp{};
    qp.pq_bits = 8; qp.pq_dim = pl.pq_dim; qp.use_subspaces = false; qp.use_vq = true; qp.vq_n_centers = pl.vq_n;
    qp.kmeans_n_iters = pl.n_iters; qp.pq_kmeans_type = CUVS_KMEANS_TYPE_KMEANS_BALANCED;
    qp.max_train_points_per_pq_code = pl.max_pq; qp.max_train_points_per_vq_cluster = pl.max_vq;
    q = pq_build(res, qp, f32_rows{train.data(), m, dim, true});
  }
  v.vq_book = dev_buf<__half>::persistent((size_t)v.vq_n * dim);
  v.pq_book = dev_buf<__half>::persistent((size_t)kVpqBookN * v.pq_len);
  vpq_round_book(res, q->vq_book.data(), (int64_t)v.vq_n * dim, v.vq_book.data(), q->vq_book.data());
  vpq_round_book(res, q->pq_book.data(), (int64_t)kVpqBookN * v.pq_len, v.pq_book.data(), q->pq_book.data());
  v.codes = dev_buf<uint8_t>::persistent((size_t)n * v.stride);
  const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(n, (int64_t(256) << 20) / (dim * 4)));
  dev_buf<float> f;
  dev_buf<char> staging;  // (contiguous rows need none)
  if (idx.dtype != elem_t::f32) f = dev_buf<float>(res, (size_t)(chunk * dim));
  dev_buf<uint32_t> labels(res, (size_t)chunk);
  dev_buf<uint8_t> codes(res, (size_t)chunk * pl.pq_dim);
  for (int64_t r0 = 0; r0 < n; r0 += chunk) {
    const int64_t cnt = std::min(chunk, n - r0);
    const char* src   = static_cast<const char*>(idx.data) + (size_t)r0 * dim * esz;
    const float* x    = reinterpret_cast<const float*>(src);
    if (idx.dtype != elem_t::f32) {
      vpq_rows_to_float(res, src, idx.dtype, 1, cnt, dim, f.data(), staging);
      x = f.data();
    }
    kmeans_predict<float>(res, x, cnt, dim, q->vq_book.data(), (int)v.vq_n, labels.data());
    pq_encode(res, *q, x, dim, cnt, labels.data(), codes.data());
    hipLaunchKernelGGL(vpq_pack_kernel, dim3(vpq_grid(res, cnt * (int64_t)v.stride)), dim3(256), 0, res.stream,
                       reinterpret_cast<const uint8_t*>(labels.data()), sizeof(uint32_t), codes.data(), (size_t)pl.pq_dim, cnt, v.pq_dim,
                       v.pq_len, v.lane_bytes, v.codes.data() + (size_t)r0 * v.stride);
    HIP_TRY(hipGetLastError());
  }
  sync(res);
  idx.owned = dev_buf<char>();
  idx.data  = nullptr;
}

std::unique_ptr<cagra_index> cagra_build(resources& res, const cuvsCagraIndexParams& p, const void* data, elem_t et,
                                         int64_t n, int64_t dim, bool is_host)
{
  const int metric = (int)p.metric;
  cagra_check_build(p, et);
  vpq_plan vplan{};
  // refusals come before any device work (host arithmetic only; cuvsCagraBuild has made the same call before it looked at
  // its handle, the tiered index and the multi-GPU index never get here with compression parameters)
  if (p.compression != nullptr) vplan = cagra_vpq_plan(p, n, dim);
  CUVS_EXPECTS(n > 1, "cagra: need at least two rows");
  auto idx    = std::make_unique<cagra_index>();
  idx->metric = metric;
  idx->dtype  = et;
  idx->n      = n;
  idx->dim    = dim;
  const size_t esz = elem_size(et);
  if (is_host) {
    idx->owned = dev_buf<char>::persistent((size_t)n * dim * esz);
    copy_async(res, idx->owned.data(), data, idx->owned.bytes());
    sync(res);
    idx->data = idx->owned.data();
  } else {
    idx->data = data;  // non-owning view of the caller's device dataset (cagra.hpp: update_dataset semantics)
  }
  uint32_t degree = (uint32_t)std::min<int64_t>((int64_t)p.graph_degree, n - 1);
  uint32_t K      = (uint32_t)std::min<int64_t>(std::max<size_t>(p.intermediate_graph_degree, degree), n - 1);
  idx->degree     = degree;
  dev_buf<uint32_t> knn(res, (size_t)n * K);
  cagra_knn_graph(res, p, *idx, K, knn.data());
  idx->graph = dev_buf<uint32_t>::persistent((size_t)n * degree);
  optimize_graph(res, knn.data(), n, K, degree, idx->graph.data(), res.cagra_guarantee_connectivity);
  cagra_set_norms(res, *idx);
  sync(res);
  // the graph is made on the original rows; the index then keeps the compressed rows only (cagra_build.cuh:2301-2311)
  if (p.compression != nullptr) cagra_compress(res, *idx, vplan);
  return idx;
}

// mg.hip: rows held and metric of the index behind a cuvsCagraIndex handle
void cagra_index_info(uintptr_t addr, int64_t* size, int* metric)
{
  CUVS_EXPECTS(addr != 0, "cagra index is empty");
  auto* idx = reinterpret_cast<const cagra_index*>(addr);
  *size     = idx->n;
  *metric   = idx->metric;
}

// hnsw.hip: what the conversion to HNSW reads of the index behind a cuvsCagraIndex handle
cagra_view cagra_index_view(uintptr_t addr)
{
  CUVS_EXPECTS(addr != 0, "CAGRA index is not built");
  auto* idx = reinterpret_cast<const cagra_index*>(addr);
  return cagra_view{idx->metric, idx->dtype, idx->n, idx->dim, idx->degree, idx->data, idx->graph.data(), idx->vpq.on()};
}

// hnsw.hip: the kNN graph of rows among themselves by the build's own size rule (cagra_knn_graph under the default build_algo)
void cagra_rows_knn_graph(resources& res, const void* data, elem_t et, int64_t n, int64_t dim, uint32_t K, int metric, uint32_t* knn)
{
  cagra_index rows;
  rows.metric = metric;
  rows.dtype  = et;
  rows.n      = n;
  rows.dim    = dim;
  rows.data   = data;
  cuvsCagraIndexParams p{};
  p.metric     = (cuvsDistanceType)metric;
  p.build_algo = IVF_PQ;
  cagra_knn_graph(res, p, rows, K, knn);
}

// tiered_index.hip: the rows a viewing index was built over have moved (same bytes, new address)
void cagra_repoint_dataset(uintptr_t addr, const void* data)
{
  CUVS_EXPECTS(addr != 0, "cagra index is empty");
  auto* idx = reinterpret_cast<cagra_index*>(addr);
  CUVS_EXPECTS(idx->owned.data() == nullptr, "cagra index owns its rows: nothing to re-point");
  idx->data = data;
}

}  // namespace cuvs_amd

using namespace cuvs_amd;

namespace {
cagra_index& get_cagra(cuvsCagraIndex_t index)
{
  CUVS_EXPECTS(index != nullptr && index->addr != 0, "CAGRA index is not built");
  return *reinterpret_cast<cagra_index*>(index->addr);
}

// the entry points that need the original rows (the reference refuses them for every dataset that is not strided)
void cagra_refuse_vpq(const cagra_index& idx, const char* what)
{
  CUVS_EXPECTS(!idx.vpq.on(), "%s: the index holds a VPQ dataset (compressed rows only), the original rows are not kept", what);
}

// a BITSET filter is read as ceil(n_bits / 32) words: refused on the host when the tensor is not 1-D or holds fewer
void cagra_check_bitset(const DLTensor& ft, int64_t n_bits, const char* what)
{
  CUVS_EXPECTS(ft.ndim == 1 && is_c_contiguous(ft), "cagra: the bitset filter must be a 1-D contiguous tensor of uint32 words (got %d dimensions)",
               (int)ft.ndim);
  CUVS_EXPECTS(ft.shape[0] >= (n_bits + 31) / 32, "bitset filter holds %ld bits, the index %ld %s", (long)(ft.shape[0] * 32),
               (long)n_bits, what);
}
}  // namespace

extern "C" {

cuvsError_t cuvsCagraIndexParamsCreate(cuvsCagraIndexParams_t* params)
{
  return (cuvsError_t)translate_exceptions([=] {
    *params                       = new cuvsCagraIndexParams{L2Expanded, 128, 64, IVF_PQ, 20, nullptr, nullptr};
    (*params)->graph_build_params = new cuvsIvfPqParams{nullptr, nullptr, 1};
  });
}
cuvsError_t cuvsCagraIndexParamsDestroy(cuvsCagraIndexParams_t params)
{
  return (cuvsError_t)translate_exceptions([=] {
    if (!params) return;
    if (params->graph_build_params != nullptr) {
      if (params->build_algo == ACE) {
        auto* ace = static_cast<cuvsAceParams*>(params->graph_build_params);
        if (ace->build_dir) free(const_cast<char*>(ace->build_dir));
        delete ace;
      } else if (params->build_algo == IVF_PQ) {
        delete static_cast<cuvsIvfPqParams*>(params->graph_build_params);
      }
    }
    delete params;
  });
}
cuvsError_t cuvsCagraCompressionParamsCreate(cuvsCagraCompressionParams_t* params)
{
  return (cuvsError_t)translate_exceptions([=] { *params = new cuvsCagraCompressionParams{8, 0, 0, 25, 0, 0}; });
}
cuvsError_t cuvsCagraCompressionParamsDestroy(cuvsCagraCompressionParams_t params)
{
  return (cuvsError_t)translate_exceptions([=] { delete params; });
}
cuvsError_t cuvsAceParamsCreate(cuvsAceParams_t* params)
{
  return (cuvsError_t)translate_exceptions([=] { *params = new cuvsAceParams{1, 120, nullptr, false, 0, 0}; });
}
cuvsError_t cuvsAceParamsDestroy(cuvsAceParams_t params)
{
  return (cuvsError_t)translate_exceptions([=] {
    if (params && params->build_dir) free(const_cast<char*>(params->build_dir));
    delete params;
  });
}
cuvsError_t cuvsCagraIndexParamsFromHnswParams(cuvsCagraIndexParams_t params, int64_t, int64_t, int M, int,
                                               enum cuvsCagraHnswHeuristicType, cuvsDistanceType metric)
{
  return (cuvsError_t)translate_exceptions([=] {
    CUVS_EXPECTS(params != nullptr, "params is null");
    params->metric                    = metric;
    params->graph_degree              = (size_t)std::max(2, 2 * M);
    params->intermediate_graph_degree = (size_t)std::max(4, 3 * M);
  });
}
cuvsError_t cuvsCagraExtendParamsCreate(cuvsCagraExtendParams_t* params)
{
  return (cuvsError_t)translate_exceptions([=] { *params = new cuvsCagraExtendParams{0}; });
}
cuvsError_t cuvsCagraExtendParamsDestroy(cuvsCagraExtendParams_t params)
{
  return (cuvsError_t)translate_exceptions([=] { delete params; });
}
cuvsError_t cuvsCagraSearchParamsCreate(cuvsCagraSearchParams_t* params)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto* p = new cuvsCagraSearchParams(cagra_default_search_params());
    *params = p;
  });
}
cuvsError_t cuvsCagraSearchParamsDestroy(cuvsCagraSearchParams_t params)
{
  return (cuvsError_t)translate_exceptions([=] { delete params; });
}
cuvsError_t cuvsCagraIndexCreate(cuvsCagraIndex_t* index)
{
  return (cuvsError_t)translate_exceptions([=] { *index = new cuvsCagraIndex{0, DLDataType{0, 0, 0}}; });
}
cuvsError_t cuvsCagraIndexDestroy(cuvsCagraIndex_t index)
{
  return (cuvsError_t)translate_exceptions([=] {
    if (!index) return;
    delete reinterpret_cast<cagra_index*>(index->addr);
    delete index;
  });
}
cuvsError_t cuvsCagraIndexGetDims(cuvsCagraIndex_t index, int64_t* dim)
{
  return (cuvsError_t)translate_exceptions([=] { *dim = get_cagra(index).dim; });
}
cuvsError_t cuvsCagraIndexGetSize(cuvsCagraIndex_t index, int64_t* size)
{
  return (cuvsError_t)translate_exceptions([=] { *size = get_cagra(index).n; });
}
cuvsError_t cuvsCagraIndexGetGraphDegree(cuvsCagraIndex_t index, int64_t* graph_degree)
{
  return (cuvsError_t)translate_exceptions([=] { *graph_degree = get_cagra(index).degree; });
}
cuvsError_t cuvsCagraIndexGetDataset(cuvsCagraIndex_t index, DLManagedTensor* dataset)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& idx = get_cagra(index);
    cagra_refuse_vpq(idx, "cuvsCagraIndexGetDataset");
    fill_dl_view(dataset, const_cast<void*>(idx.data), index->dtype, idx.n, idx.dim, 2, 0);
  });
}
cuvsError_t cuvsCagraIndexGetGraph(cuvsCagraIndex_t index, DLManagedTensor* graph)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& idx = get_cagra(index);
    fill_dl_view(graph, idx.graph.data(), DLDataType{kDLUInt, 32, 1}, idx.n, idx.degree, 2, 0);
  });
}

cuvsError_t cuvsCagraBuild(cuvsResources_t res_h, cuvsCagraIndexParams_t params, DLManagedTensor* dataset_tensor,
                           cuvsCagraIndex_t index)
{
  return (cuvsError_t)translate_exceptions([=] {
    CUVS_EXPECTS(params && dataset_tensor && index, "null argument");
    auto& ds = dataset_tensor->dl_tensor;
    CUVS_EXPECTS(ds.ndim == 2 && is_c_contiguous(ds), "dataset must be a row-major matrix");
    // what a compressed build cannot serve is refused from the arguments alone, before the handle or the device is touched
    if (params->compression != nullptr) (void)cagra_vpq_plan(*params, ds.shape[0], ds.shape[1]);
    auto& res = *as_res(res_h);
    auto idx = cagra_build(res, *params, dl_data(ds), elem_of(ds.dtype), ds.shape[0], ds.shape[1],
                           !is_device_accessible(ds));
    delete reinterpret_cast<cagra_index*>(index->addr);
    index->addr  = reinterpret_cast<uintptr_t>(idx.release());
    index->dtype = ds.dtype;
  });
}

cuvsError_t cuvsCagraIndexFromArgs(cuvsResources_t res_h, cuvsDistanceType metric, DLManagedTensor* graph_tensor,
                                   DLManagedTensor* dataset_tensor, cuvsCagraIndex_t index)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& res = *as_res(res_h);
    CUVS_EXPECTS(graph_tensor && dataset_tensor && index, "null argument");
    auto& g  = graph_tensor->dl_tensor;
    auto& ds = dataset_tensor->dl_tensor;
    CUVS_EXPECTS(dtype_is(g.dtype, kDLUInt, 32) && g.ndim == 2 && is_c_contiguous(g), "graph must be uint32 [n, degree]");
    CUVS_EXPECTS(ds.ndim == 2 && is_c_contiguous(ds) && ds.shape[0] == g.shape[0], "dataset/graph shape mismatch");
    auto idx    = std::make_unique<cagra_index>();
    idx->metric = (int)metric;
    idx->dtype  = elem_of(ds.dtype);
    idx->n      = ds.shape[0];
    idx->dim    = ds.shape[1];
    idx->degree = (uint32_t)g.shape[1];
    const size_t esz = elem_size(idx->dtype);
    if (is_device_accessible(ds)) {
      idx->data = dl_data(ds);
    } else {
      idx->owned = dev_buf<char>::persistent((size_t)idx->n * idx->dim * esz);
      copy_async(res, idx->owned.data(), dl_data(ds), idx->owned.bytes());
      idx->data = idx->owned.data();
    }
    idx->graph = dev_buf<uint32_t>::persistent((size_t)idx->n * idx->degree);
    copy_async(res, idx->graph.data(), dl_data(g), idx->graph.bytes());
    cagra_set_norms(res, *idx);
    sync(res);
    delete reinterpret_cast<cagra_index*>(index->addr);
    index->addr  = reinterpret_cast<uintptr_t>(idx.release());
    index->dtype = ds.dtype;
  });
}

cuvsError_t cuvsCagraSearch(cuvsResources_t res_h, cuvsCagraSearchParams_t params, cuvsCagraIndex_t index_c,
                            DLManagedTensor* queries_tensor, DLManagedTensor* neighbors_tensor,
                            DLManagedTensor* distances_tensor, cuvsFilter filter)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& res = *as_res(res_h);
    auto& idx = get_cagra(index_c);
    CUVS_EXPECTS(params && queries_tensor && neighbors_tensor && distances_tensor, "null argument");
    auto& queries   = queries_tensor->dl_tensor;
    auto& neighbors = neighbors_tensor->dl_tensor;
    auto& distances = distances_tensor->dl_tensor;
    CUVS_EXPECTS(is_device_accessible(queries), "queries should have device compatible memory");
    CUVS_EXPECTS(is_device_accessible(neighbors), "neighbors should have device compatible memory");
    CUVS_EXPECTS(is_device_accessible(distances), "distances should have device compatible memory");
    const bool idx64 = dtype_is(neighbors.dtype, kDLInt, 64);
    CUVS_EXPECTS(idx64 || dtype_is(neighbors.dtype, kDLUInt, 32), "neighbors should be of type uint32_t or int64_t");
    CUVS_EXPECTS(dtype_is(distances.dtype, kDLFloat, 32), "distances should be of type float32");
    CUVS_EXPECTS(queries.ndim == 2 && neighbors.ndim == 2 && distances.ndim == 2, "tensors must be 2-D");
    CUVS_EXPECTS(is_c_contiguous(queries) && is_c_contiguous(neighbors) && is_c_contiguous(distances),
                 "tensors must be C-contiguous");
    CUVS_EXPECTS(queries.dtype.code == index_c->dtype.code && queries.dtype.bits == index_c->dtype.bits,
                 "Unsupported queries DLtensor dtype: %d and bits: %d", (int)queries.dtype.code,
                 (int)queries.dtype.bits);
    CUVS_EXPECTS(queries.shape[1] == idx.dim, "queries dim mismatch");
    int64_t m = queries.shape[0], k = neighbors.shape[1];
    CUVS_EXPECTS(neighbors.shape[0] == m && distances.shape[0] == m && distances.shape[1] == k,
                 "neighbors/distances shape mismatch");
    const uint32_t* bits = nullptr;
    if (filter.type != NO_FILTER) {
      CUVS_EXPECTS(filter.type == BITSET && filter.addr != 0, "cagra: only BITSET filters are supported");
      auto& ft = reinterpret_cast<DLManagedTensor*>(filter.addr)->dl_tensor;
      CUVS_EXPECTS(dtype_is(ft.dtype, kDLUInt, 32) && is_device_accessible(ft), "filter must be a device uint32 tensor");
      // the bitset is over source ids: the rows themselves, or the image of the index's source_indices
      cagra_check_bitset(ft, idx.source_indices.data() != nullptr ? idx.source_bits : idx.n,
                         idx.source_indices.data() != nullptr ? "source ids" : "rows");
      bits = static_cast<const uint32_t*>(dl_data(ft));
    }
    cagra_search(res, idx, *params, dl_data(queries), m, (int)k, dl_data(neighbors), idx64,
                 static_cast<float*>(dl_data(distances)), bits);
  });
}

namespace {
constexpr int kCagraRefVersion = 5;  // cagra_serialize.cuh:30
// cudaDataType_t codes the reference stores in front of a strided dataset (dataset_serialize.hpp:82-101)
inline uint32_t cuda_dtype_code(elem_t e) { return e == elem_t::f32 ? 0u : e == elem_t::f16 ? 2u : e == elem_t::i8 ? 3u : 8u; }
inline char npy_kind(elem_t e) { return e == elem_t::f32 ? 'f' : e == elem_t::f16 ? 'e' : e == elem_t::i8 ? 'i' : 'u'; }
}  // namespace

cuvsError_t cuvsCagraSerialize(cuvsResources_t res_h, const char* filename, cuvsCagraIndex_t index, bool include_dataset)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& res = *as_res(res_h);
    auto& idx = get_cagra(index);
    if (write_native_container(res)) {
      file_writer w(filename, KIND_CAGRA);
      w.scalar<int32_t>(idx.metric); w.scalar<int32_t>((int)idx.dtype); w.scalar<int64_t>(idx.n); w.scalar<int64_t>(idx.dim);
      w.scalar<uint32_t>(idx.degree); w.scalar<uint8_t>(index->dtype.code); w.scalar<uint8_t>(index->dtype.bits);
      // dataset: 0 none, 1 rows, 2 VPQ (vq_n_centers, pq_len, then the two fp16 books and the rows in the reference's layout)
      const bool vpq = idx.vpq.on();
      w.scalar<uint8_t>(include_dataset ? (vpq ? 2 : 1) : 0);
      w.device_array(res, idx.graph.data(), idx.graph.bytes());
      if (include_dataset && vpq) {
        w.scalar<uint32_t>(idx.vpq.vq_n); w.scalar<uint32_t>(idx.vpq.pq_len);
        w.device_array(res, idx.vpq.vq_book.data(), idx.vpq.vq_book.bytes());
        w.device_array(res, idx.vpq.pq_book.data(), idx.vpq.pq_book.bytes());
        w.scalar<uint64_t>((uint64_t)idx.n * idx.vpq.row_len);
        vpq_store_rows(res, idx, [&](const void* p, size_t bytes) { w.raw(p, bytes); });
      } else if (include_dataset) {
        w.device_array(res, idx.data, (size_t)idx.n * idx.dim * elem_size(idx.dtype));
      }
      return;
    }
    // reference record sequence (cagra_serialize.cuh:49-75, dataset_serialize.hpp:38-60,82-87): dtype prefix,
    // version, size (IdxT = uint32), dim, graph_degree, metric, graph [n, degree], content_map (bit 0 = dataset,
    // bit 1 = source_indices), then the dataset: tag 2 (strided), cudaDataType, n_rows (int64), dim, stride, rows
    npy_writer w(filename);
    char prefix[4];
    elem_prefix(idx.dtype, prefix);
    w.raw(prefix, 4);
    w.scalar<int32_t>(kCagraRefVersion);
    w.scalar<uint32_t>((uint32_t)idx.n);
    w.scalar<uint32_t>((uint32_t)idx.dim);
    w.scalar<uint32_t>(idx.degree);
    w.scalar<int32_t>(idx.metric);
    w.device_array(res, 'u', 4, {idx.n, idx.degree}, idx.graph.data());
    const bool with_vpq  = include_dataset && idx.vpq.on() && idx.n > 0;
    const bool with_data = (include_dataset && idx.data != nullptr && idx.n > 0) || with_vpq;
    const bool with_src = idx.source_indices.data() != nullptr;
    w.scalar<uint32_t>((with_data ? 1u : 0u) | (with_src ? 2u : 0u));
    if (with_vpq) {
      // dataset_serialize.hpp:60-73,107-111: tag 3 (VPQ), CUDA_R_16F, n_rows (int64), dim, vq_n_centers, pq_n_centers, pq_len,
      // encoded_row_length (uint32 each), then vq_code_book, pq_code_book and the rows [uint32 label][codes][zero padding]
      const auto& v = idx.vpq;
      w.scalar<uint32_t>(3u);
      w.scalar<uint32_t>(cuda_dtype_code(elem_t::f16));
      w.scalar<int64_t>(idx.n);
      w.scalar<uint32_t>((uint32_t)idx.dim);
      w.scalar<uint32_t>(v.vq_n);
      w.scalar<uint32_t>(kVpqBookN);
      w.scalar<uint32_t>(v.pq_len);
      w.scalar<uint32_t>(v.row_len);
      w.device_array(res, 'e', 2, {(int64_t)v.vq_n, idx.dim}, v.vq_book.data());
      w.device_array(res, 'e', 2, {(int64_t)kVpqBookN, (int64_t)v.pq_len}, v.pq_book.data());
      w.header('u', 1, {idx.n, (int64_t)v.row_len});  // the rows leave in chunks, converted to the reference's layout
      vpq_store_rows(res, idx, [&](const void* p, size_t bytes) { w.raw(p, bytes); });
    } else if (with_data) {
      const size_t es = elem_size(idx.dtype);
      w.scalar<uint32_t>(2u);
      w.scalar<uint32_t>(cuda_dtype_code(idx.dtype));
      w.scalar<int64_t>(idx.n);
      w.scalar<uint32_t>((uint32_t)idx.dim);
      w.scalar<uint32_t>((uint32_t)(round_up(idx.dim * (int64_t)es, 16) / es));  // 16-byte aligned row stride
      w.device_array(res, npy_kind(idx.dtype), (uint32_t)es, {idx.n, idx.dim}, idx.data);
    }
    if (with_src) w.device_array(res, 'u', 4, {idx.n}, idx.source_indices.data());  // cagra_serialize.cuh:83
    w.close();
  });
}

cuvsError_t cuvsCagraDeserialize(cuvsResources_t res_h, const char* filename, cuvsCagraIndex_t index)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& res = *as_res(res_h);
    CUVS_EXPECTS(index != nullptr, "index is null");
    auto idx = std::make_unique<cagra_index>();
    DLDataType dl;
    if (is_native_container(filename)) {
      file_reader r(filename, KIND_CAGRA);
      idx->metric = r.scalar<int32_t>(); idx->dtype = (elem_t)r.scalar<int32_t>(); idx->n = r.scalar<int64_t>();
      idx->dim = r.scalar<int64_t>(); idx->degree = r.scalar<uint32_t>();
      uint8_t code = r.scalar<uint8_t>(), bits = r.scalar<uint8_t>(), has_data = r.scalar<uint8_t>();
      idx->graph = r.device_array<uint32_t>(res);
      if (has_data == 2) {
        const uint32_t vq_n = r.scalar<uint32_t>(), pq_len = r.scalar<uint32_t>();
        CUVS_EXPECTS(idx->dim > 0 && (pq_len == 2 || pq_len == 4) && idx->dim % pq_len == 0 && vq_n > 0,
                     "cagra::deserialize: bad VPQ dataset header (pq_len %u, vq_n_centers %u)", pq_len, vq_n);
        idx->vpq.set_shape(idx->dim, vq_n, pq_len);
        idx->vpq.vq_book = r.device_array<__half>(res);
        idx->vpq.pq_book = r.device_array<__half>(res);
        const uint64_t row_bytes = r.scalar<uint64_t>();
        CUVS_EXPECTS(idx->metric == M_L2Expanded, "VPQ compression is only supported with L2Expanded distance mertric");
        CUVS_EXPECTS((int64_t)idx->vpq.vq_book.size() == (int64_t)vq_n * idx->dim && idx->vpq.pq_book.size() == (size_t)kVpqBookN * pq_len &&
                       row_bytes == (uint64_t)idx->n * idx->vpq.row_len,
                     "cagra::deserialize: the VPQ dataset does not match the graph");
        vpq_load_rows(res, *idx, [&](void* p, size_t bytes) { r.raw(p, bytes); });
        sync(res);
      } else if (has_data) {
        idx->owned = r.device_array<char>(res);
        idx->data  = idx->owned.data();
      }
      dl = DLDataType{code, bits, 1};
    } else {
      // reference format (cagra_serialize.cuh:270-330; dtype dispatch c/src/neighbors/cagra.cpp:876-900)
      npy_reader r(filename);
      char prefix[4];
      r.raw(prefix, 4);
      CUVS_EXPECTS(parse_elem_prefix(prefix, &idx->dtype), "Unsupported index dtype in file %s", filename);
      int ver = r.scalar<int32_t>();
      CUVS_EXPECTS(ver == kCagraRefVersion, "serialization version mismatch, expected %d, got %d ", kCagraRefVersion, ver);
      idx->n      = (int64_t)r.scalar<uint32_t>();
      idx->dim    = (int64_t)r.scalar<uint32_t>();
      idx->degree = r.scalar<uint32_t>();
      idx->metric = r.scalar<int32_t>();
      CUVS_EXPECTS(metric_is_l2(idx->metric) || idx->metric == M_InnerProduct || idx->metric == M_CosineExpanded ||
                     (idx->metric == M_BitwiseHamming && (idx->dtype == elem_t::u8 || idx->dtype == elem_t::i8)),
                   "cagra::deserialize: unsupported metric value %d", idx->metric);
      CUVS_EXPECTS(idx->degree > 0 && idx->degree <= 1024, "cagra::deserialize: graph_degree=%u exceeds maximum %u",
                   idx->degree, 1024u);
      idx->graph = r.device_array<uint32_t>(res, idx->n * (int64_t)idx->degree);
      uint32_t content = r.scalar<uint32_t>();
      if (content & 1u) {
        uint32_t tag = r.scalar<uint32_t>();
        if (tag == 1u) {
          (void)r.scalar<uint32_t>();  // empty dataset: suggested dim only
        } else if (tag == 3u) {
          // a VPQ dataset (dataset_serialize.hpp:135-160). The file is untrusted: everything the walk indexes with is checked here
          const uint32_t code = r.scalar<uint32_t>();
          CUVS_EXPECTS(code == cuda_dtype_code(elem_t::f16) || code == cuda_dtype_code(elem_t::f32),
                       "cagra::deserialize: VPQ codebook element type %u is neither CUDA_R_16F nor CUDA_R_32F", code);
          const int64_t rows    = r.scalar<int64_t>();
          const uint32_t dim    = r.scalar<uint32_t>(), vq_n = r.scalar<uint32_t>(), pq_n = r.scalar<uint32_t>();
          const uint32_t pq_len = r.scalar<uint32_t>(), row_len = r.scalar<uint32_t>();
          CUVS_EXPECTS(idx->metric == M_L2Expanded, "VPQ compression is only supported with L2Expanded distance mertric");
          CUVS_EXPECTS(pq_n == kVpqBookN, "cagra::deserialize: VPQ dataset with pq_n_centers %u (only 256, pq_bits 8, is supported)", pq_n);
          CUVS_EXPECTS(pq_len == 2 || pq_len == 4, "cagra::deserialize: VPQ dataset with pq_len %u (only 2 and 4 are supported)", pq_len);
          CUVS_EXPECTS(dim > 0 && dim % pq_len == 0, "cagra::deserialize: VPQ dataset dim %u is not a multiple of pq_len %u", dim, pq_len);
          CUVS_EXPECTS(rows == idx->n && (int64_t)dim == idx->dim && vq_n > 0, "cagra::deserialize: dataset shape does not match the graph");
          idx->vpq.set_shape(idx->dim, vq_n, pq_len);
          CUVS_EXPECTS(row_len == idx->vpq.row_len, "cagra::deserialize: VPQ dataset with encoded_row_length %u, expected %u", row_len,
                       idx->vpq.row_len);
          auto read_book = [&](int64_t count) {
            if (code == cuda_dtype_code(elem_t::f16)) return r.device_array<__half>(res, count);
            dev_buf<float> b = r.device_array<float>(res, count);  // fp32 codebooks (vpq_dataset<float>) are rounded to fp16
            auto out = dev_buf<__half>::persistent((size_t)count);
            vpq_round_book(res, b.data(), count, out.data(), nullptr);
            sync(res);
            return out;
          };
          idx->vpq.vq_book = read_book((int64_t)vq_n * dim);
          idx->vpq.pq_book = read_book((int64_t)kVpqBookN * pq_len);
          const npy_header eh = r.header();
          CUVS_EXPECTS(eh.itemsize == 1 && !eh.fortran && eh.count() == rows * (int64_t)row_len,
                       "cagra::deserialize: the encoded rows of the VPQ dataset are not %ld x %u bytes", (long)rows, row_len);
          vpq_load_rows(res, *idx, [&](void* p, size_t bytes) { r.raw(p, bytes); });
          sync(res);
        } else {
          CUVS_EXPECTS(tag == 2u, "Failed to deserialize dataset: unknown instance tag %u", tag);
          uint32_t code = r.scalar<uint32_t>();
          CUVS_EXPECTS(code == cuda_dtype_code(idx->dtype), "cagra::deserialize: dataset element type %u does not match the index dtype", code);
          int64_t rows = r.scalar<int64_t>();
          uint32_t dim = r.scalar<uint32_t>();
          (void)r.scalar<uint32_t>();  // stride: rows are stored unpadded
          CUVS_EXPECTS(rows == idx->n && dim == idx->dim, "cagra::deserialize: dataset shape does not match the graph");
          idx->owned = r.device_bytes(res, (uint32_t)elem_size(idx->dtype), rows * (int64_t)dim);
          idx->data  = idx->owned.data();
        }
      }
      if (content & 2u) {  // cagra_serialize.cuh:314-321
        idx->source_indices = r.device_array<uint32_t>(res, idx->n);
        const std::vector<uint32_t> src = to_host(res, idx->source_indices.data(), (size_t)idx->n);
        idx->source_bits = src.empty() ? 0 : (int64_t)*std::max_element(src.begin(), src.end()) + 1;
      }
      dl = dl_of(idx->dtype);
    }
    cagra_set_norms(res, *idx);
    sync(res);
    delete reinterpret_cast<cagra_index*>(index->addr);
    index->addr  = reinterpret_cast<uintptr_t>(idx.release());
    index->dtype = dl;
  });
}

// hnswlib "base layer only" export (cagra_serialize.cuh:98-258): 96-byte header, then per node
// {int degree, uint32 links[degree], T row[dim], size_t label}, then one zero int per node (no upper levels).
cuvsError_t cuvsCagraSerializeToHnswlib(cuvsResources_t res_h, const char* filename, cuvsCagraIndex_t index)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& res = *as_res(res_h);
    auto& idx = get_cagra(index);
    cagra_refuse_vpq(idx, "cuvsCagraSerializeToHnswlib");
    CUVS_EXPECTS(idx.data != nullptr && idx.n > 0, "Invalid CAGRA dataset of size 0 during serialization");
    CUVS_EXPECTS(idx.metric != M_BitwiseHamming, "cagra::serialize_to_hnswlib: hnswlib has no BitwiseHamming space; a Hamming "
                                                 "index cannot be exported");
    CUVS_EXPECTS(filename != nullptr, "filename is null");
    FILE* f = fopen(filename, "wb");
    CUVS_EXPECTS(f != nullptr, "Cannot open file %s", filename);
    struct closer { FILE* f; ~closer() { if (f) fclose(f); } } guard{f};
    auto put = [&](const void* p, size_t n) { CUVS_EXPECTS(fwrite(p, 1, n, f) == n, "Error writing HNSW file"); };
    const size_t es = elem_size(idx.dtype), n = (size_t)idx.n, dim = (size_t)idx.dim, deg = idx.degree;
    const size_t per_elem = deg * 4 + 4 + dim * es + 8;
    const size_t hdr[6]   = {0, n, n, per_elem, per_elem - 8, deg * 4 + 4};
    put(hdr, sizeof(hdr));            // offset_level_0, max_element, curr_element_count, size_data_per_element,
                                      // label_offset, offset_data
    const int max_level = 1, entry = (int)(n / 2);
    put(&max_level, 4);
    put(&entry, 4);
    const size_t m[3] = {deg / 2, deg, deg / 2};  // max_M, max_M0, M
    put(m, sizeof(m));
    const double mult = 0.42424242;
    put(&mult, 8);
    const size_t ef_construction = 500;
    put(&ef_construction, 8);
    const size_t step = std::max<size_t>(1, (size_t(64) << 20) / (dim * es + deg * 4));
    std::vector<uint32_t> g(step * deg);
    std::vector<char> rows(step * dim * es), out(step * per_elem);
    for (size_t r0 = 0; r0 < n; r0 += step) {
      const size_t nr = std::min(step, n - r0);
      copy_async(res, g.data(), idx.graph.data() + r0 * deg, nr * deg * 4);
      copy_async(res, rows.data(), static_cast<const char*>(idx.data) + r0 * dim * es, nr * dim * es);
      sync(res);
      char* o = out.data();
      for (size_t i = 0; i < nr; ++i) {
        const int d32 = (int)deg;
        const size_t label = r0 + i;
        memcpy(o, &d32, 4); o += 4;
        memcpy(o, g.data() + i * deg, deg * 4); o += deg * 4;
        memcpy(o, rows.data() + i * dim * es, dim * es); o += dim * es;
        memcpy(o, &label, 8); o += 8;
      }
      put(out.data(), nr * per_elem);
    }
    std::vector<int> zeros(std::min<size_t>(n, 1 << 20), 0);
    for (size_t r0 = 0; r0 < n; r0 += zeros.size()) put(zeros.data(), std::min(zeros.size(), n - r0) * 4);
    int rc  = fclose(f);
    guard.f = nullptr;
    CUVS_EXPECTS(rc == 0, "Error writing output %s", filename);
  });
}

cuvsError_t cuvsCagraExtend(cuvsResources_t res_h, cuvsCagraExtendParams_t params, DLManagedTensor* additional_dataset,
                            cuvsCagraIndex_t index)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& res = *as_res(res_h);
    auto& idx = get_cagra(index);
    cagra_refuse_vpq(idx, "cuvsCagraExtend");
    CUVS_EXPECTS(additional_dataset != nullptr, "additional_dataset is null");
    auto& t = additional_dataset->dl_tensor;
    CUVS_EXPECTS(t.ndim == 2 && is_c_contiguous(t) && t.shape[1] == idx.dim, "additional_dataset must be [m, dim] row-major");
    CUVS_EXPECTS(elem_of(t.dtype) == idx.dtype, "additional_dataset dtype differs from the index dtype");
    CUVS_EXPECTS(is_device_accessible(t) || is_host_accessible(t), "additional_dataset must be accessible on host or device memory");
    cagra_extend(res, idx, dl_data(t), !is_device_accessible(t), t.shape[0], params ? params->max_chunk_size : 0u);
  });
}

// Physical merge (cagra_merge.cuh): the datasets of the input indexes are concatenated in order and a new graph is
// built over all rows with `params`; ids of index i are shifted by the sizes of the indexes before it.
namespace {
// rows[keep[i]] -> out[i] (row_bytes is a multiple of the element size; byte copy, one workgroup per row, strided over the rows)
__global__ void gather_rows_kernel(const char* __restrict__ rows, const int64_t* __restrict__ keep, int64_t n_keep, size_t row_bytes,
                                   char* __restrict__ out)
{
  for (int64_t i = blockIdx.x; i < n_keep; i += gridDim.x) {
    const char* src = rows + (size_t)keep[i] * row_bytes;
    char* dst       = out + (size_t)i * row_bytes;
    for (size_t b = threadIdx.x; b < row_bytes; b += blockDim.x) dst[b] = src[b];
  }
}
}  // namespace

cuvsError_t cuvsCagraMerge(cuvsResources_t res_h, cuvsCagraIndexParams_t params, cuvsCagraIndex_t* indices,
                           size_t num_indices, cuvsFilter filter, cuvsCagraIndex_t output_index)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& res = *as_res(res_h);
    CUVS_EXPECTS(params && indices && output_index && num_indices > 0, "null argument");
    // a BITSET over the concatenated rows keeps the rows whose bit is set (cagra_merge.cuh:94-131: the merged index is built on
    // the kept rows, in order); bitmaps are refused as in the reference (:45-46)
    CUVS_EXPECTS(filter.type == NO_FILTER || filter.type == BITSET, "Bitmap filter isn't supported inside cagra::merge");
    // the reference's merge builds over an uncompressed dataset only (cagra_merge.cuh); compress the merged rows with a build
    CUVS_EXPECTS(params->compression == nullptr, "cuvsCagraMerge: VPQ compression parameters are not supported");
    const uint32_t* bits = nullptr;
    if (filter.type == BITSET) {
      CUVS_EXPECTS(filter.addr != 0, "cagra::merge: the filter has no tensor");
      auto& ft = reinterpret_cast<DLManagedTensor*>(filter.addr)->dl_tensor;
      CUVS_EXPECTS(dtype_is(ft.dtype, kDLUInt, 32) && is_device_accessible(ft), "filter must be a device uint32 tensor");
      bits = static_cast<const uint32_t*>(dl_data(ft));
    }
    auto& first = get_cagra(indices[0]);
    int64_t total = 0;
    for (size_t i = 0; i < num_indices; ++i) {
      auto& ix = get_cagra(indices[i]);
      cagra_refuse_vpq(ix, "cuvsCagraMerge");
      CUVS_EXPECTS(ix.data != nullptr, "cagra::merge: index %zu has no dataset", i);
      // the merged index numbers its rows by position in the concatenation, and the BITSET is over those positions: an input
      // that reports source ids would be renumbered silently, so it is refused
      CUVS_EXPECTS(ix.source_indices.data() == nullptr, "cagra::merge: index %zu carries source_indices and cannot be merged", i);
      CUVS_EXPECTS(ix.dim == first.dim && ix.dtype == first.dtype, "cagra::merge: indexes differ in dim or dtype");
      total += ix.n;
    }
    if (filter.type == BITSET) cagra_check_bitset(reinterpret_cast<DLManagedTensor*>(filter.addr)->dl_tensor, total, "rows");
    const size_t row_bytes = (size_t)first.dim * elem_size(first.dtype);
    auto all = dev_buf<char>::persistent((size_t)total * row_bytes);
    size_t off = 0;
    for (size_t i = 0; i < num_indices; ++i) {
      auto& ix = get_cagra(indices[i]);
      copy_async(res, all.data() + off, ix.data, (size_t)ix.n * row_bytes);
      off += (size_t)ix.n * row_bytes;
    }
    sync(res);
    if (bits != nullptr) {  // the kept rows, compacted in order
      const size_t words = ((size_t)total + 31) / 32;
      std::vector<uint32_t> hb = to_host(res, bits, words);
      std::vector<int64_t> keep;
      keep.reserve((size_t)total);
      for (int64_t r = 0; r < total; ++r)
        if ((hb[(size_t)r >> 5] >> (r & 31)) & 1u) keep.push_back(r);
      CUVS_EXPECTS(!keep.empty(), "cagra::merge: the filter keeps no row");
      dev_buf<int64_t> kd(res, keep.size());
      copy_async(res, kd.data(), keep.data(), keep.size() * sizeof(int64_t));
      auto kept = dev_buf<char>::persistent(keep.size() * row_bytes);
      hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)std::min<int64_t>((int64_t)keep.size(), 65535)), dim3(256), 0, res.stream,
                         all.data(), kd.data(), (int64_t)keep.size(), row_bytes, kept.data());
      sync(res);  // (keep is pageable host memory)
      all   = std::move(kept);
      total = (int64_t)keep.size();
    }
    auto idx   = cagra_build(res, *params, all.data(), first.dtype, total, first.dim, false);
    idx->owned = std::move(all);  // the merged index owns the concatenated rows (idx->data already points at them)
    delete reinterpret_cast<cagra_index*>(output_index->addr);
    output_index->addr  = reinterpret_cast<uintptr_t>(idx.release());
    output_index->dtype = indices[0]->dtype;
  });
}

}  // extern "C"


// Measured work of the graph walks run on this handle (CAGRA bytes(q) = n_dist * dim * sizeof(T) + n_iter *
// degree * 4 with n_dist and n_iter measured; the reference has its per-phase _CLK_BREAKDOWN counters,
// search_single_cta_jit.cuh:91-103,425-451). enable != 0: zero the counters and count from now on; enable == 0: stop and
// return {rows scored, graph rows read, walkers} of the searches since (include/cuvs_amd/extensions.h).
extern "C" __attribute__((visibility("default"))) cuvsError_t cuvsAmdCagraWorkCounters(cuvsResources_t res_h, int enable,
                                                                                       uint64_t out[3])
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& res = *cuvs_amd::as_res(res_h);
    if (enable) {
      if (res.cagra_work == nullptr) HIP_TRY(hipMalloc(reinterpret_cast<void**>(&res.cagra_work), 3 * sizeof(unsigned long long)));
      HIP_TRY(hipMemsetAsync(res.cagra_work, 0, 3 * sizeof(unsigned long long), res.stream));
      return;
    }
    CUVS_EXPECTS(res.cagra_work != nullptr && out != nullptr, "cagra work counters were not enabled on this handle");
    unsigned long long h[3];
    HIP_TRY(hipMemcpyAsync(h, res.cagra_work, sizeof(h), hipMemcpyDeviceToHost, res.stream));
    HIP_TRY(hipStreamSynchronize(res.stream));
    for (int i = 0; i < 3; ++i) out[i] = h[i];
    (void)hipFree(res.cagra_work);
    res.cagra_work = nullptr;
  });
}

// cagra::index_params::guarantee_connectivity (cpp/include/cuvs/neighbors/cagra.hpp:193) has no field in the C struct
// cuvsCagraIndexParams (c/include/cuvs/neighbors/cagra.h): the switch lives on the handle and applies to the
// cuvsCagraBuild / cuvsCagraExtend calls made with it (include/cuvs_amd/extensions.h).
extern "C" __attribute__((visibility("default"))) cuvsError_t cuvsAmdCagraSetGuaranteeConnectivity(cuvsResources_t res_h, int on)
{
  return (cuvsError_t)translate_exceptions([=] { cuvs_amd::as_res(res_h)->cagra_guarantee_connectivity = on != 0; });
}

// The VPQ dataset of a compressed index (include/cuvs_amd/extensions.h; the reference reads it through the C++ index only).
extern "C" __attribute__((visibility("default"))) cuvsError_t cuvsAmdCagraIndexGetVpqInfo(cuvsCagraIndex_t index, uint32_t out[5])
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& idx = get_cagra(index);
    CUVS_EXPECTS(idx.vpq.on(), "cuvsAmdCagraIndexGetVpqInfo: the index holds no VPQ dataset");
    CUVS_EXPECTS(out != nullptr, "null argument");
    out[0] = idx.vpq.vq_n; out[1] = cuvs_amd::kVpqBookN; out[2] = idx.vpq.pq_len; out[3] = idx.vpq.row_len; out[4] = (uint32_t)idx.dim;
  });
}

extern "C" __attribute__((visibility("default"))) cuvsError_t cuvsAmdCagraIndexGetVpq(cuvsResources_t res_h, cuvsCagraIndex_t index,
                                                                                      DLManagedTensor* vq_book, DLManagedTensor* pq_book,
                                                                                      DLManagedTensor* codes)
{
  return (cuvsError_t)translate_exceptions([=] {
    using namespace cuvs_amd;
    auto& res = *as_res(res_h);
    auto& idx = get_cagra(index);
    CUVS_EXPECTS(idx.vpq.on(), "cuvsAmdCagraIndexGetVpq: the index holds no VPQ dataset");
    CUVS_EXPECTS(vq_book && pq_book && codes, "null argument");
    const auto& v = idx.vpq;
    auto check = [](const DLTensor& t, uint8_t code, uint8_t bits, int64_t rows, int64_t cols, const char* what) {
      CUVS_EXPECTS(is_device_accessible(t) && dtype_is(t.dtype, code, bits) && t.ndim == 2 && is_c_contiguous(t) && t.shape[0] == rows &&
                     t.shape[1] == cols,
                   "cuvsAmdCagraIndexGetVpq: %s must be a device %s [%ld, %ld] row-major matrix", what, bits == 16 ? "float16" : "uint8",
                   (long)rows, (long)cols);
    };
    check(vq_book->dl_tensor, kDLFloat, 16, v.vq_n, idx.dim, "vq_book");
    check(pq_book->dl_tensor, kDLFloat, 16, kVpqBookN, v.pq_len, "pq_book");
    check(codes->dl_tensor, kDLUInt, 8, idx.n, v.row_len, "codes");
    copy_async(res, dl_data(vq_book->dl_tensor), v.vq_book.data(), v.vq_book.bytes());
    copy_async(res, dl_data(pq_book->dl_tensor), v.pq_book.data(), v.pq_book.bytes());
    vpq_export_rows(res, idx, 0, idx.n, static_cast<uint8_t*>(dl_data(codes->dl_tensor)));
    sync(res);
  });
}

// cagra::helpers::optimize (cpp/include/cuvs/neighbors/cagra_optimize.hpp; graph_core.cuh:1706-1809): kNN graph
// [n, K] uint32 (host or device) -> search graph [n, degree] uint32 (host or device); components_left (optional):
// connected components of the spanning forest (1 when guarantee_connectivity succeeded, 0 when it was not asked for).
extern "C" __attribute__((visibility("default"))) cuvsError_t cuvsAmdCagraOptimize(cuvsResources_t res_h,
                                                                                   DLManagedTensor* knn_tensor,
                                                                                   DLManagedTensor* graph_tensor,
                                                                                   int guarantee_connectivity)
{
  return (cuvsError_t)translate_exceptions([=] {
    using namespace cuvs_amd;
    auto& res = *as_res(res_h);
    CUVS_EXPECTS(knn_tensor && graph_tensor, "null argument");
    auto& kg = knn_tensor->dl_tensor;
    auto& g  = graph_tensor->dl_tensor;
    CUVS_EXPECTS(dtype_is(kg.dtype, kDLUInt, 32) && kg.ndim == 2 && is_c_contiguous(kg), "knn_graph must be uint32 [n, K]");
    CUVS_EXPECTS(dtype_is(g.dtype, kDLUInt, 32) && g.ndim == 2 && is_c_contiguous(g) && g.shape[0] == kg.shape[0],
                 "graph must be uint32 [n, degree]");
    const int64_t n = kg.shape[0];
    const uint32_t K = (uint32_t)kg.shape[1], degree = (uint32_t)g.shape[1];
    dev_buf<uint32_t> knn_d, g_d;
    const uint32_t* knn = static_cast<const uint32_t*>(dl_data(kg));
    if (!is_device_accessible(kg)) {
      knn_d = dev_buf<uint32_t>(res, (size_t)n * K);
      copy_async(res, knn_d.data(), knn, knn_d.bytes());
      knn = knn_d.data();
    }
    uint32_t* out = static_cast<uint32_t*>(dl_data(g));
    if (!is_device_accessible(g)) {
      g_d = dev_buf<uint32_t>(res, (size_t)n * degree);
      out = g_d.data();
    }
    optimize_graph(res, knn, n, K, degree, out, guarantee_connectivity != 0);
    if (!is_device_accessible(g)) copy_async(res, dl_data(g), out, (size_t)n * degree * sizeof(uint32_t));
    sync(res);
  });
}

// Test hook (not part of the reference ABI): the search plan for given parameters, computed on the host without
// touching a GPU - tests pin it to the reference's rules (search_plan.cuh:121-131,199-340).
extern "C" __attribute__((visibility("default"))) int cuvsAmdCagraSearchPlan(cuvsCagraSearchParams_t params, int64_t n_rows,
                                                                              uint32_t graph_degree, uint32_t topk,
                                                                              int64_t n_queries, int num_cus,
                                                                              float filtering_rate, uint32_t out[10])
{
  return translate_exceptions([=] {
    const cuvs_amd::cagra_plan pl =
      cuvs_amd::make_cagra_plan(*params, n_rows, graph_degree, topk, n_queries, num_cus, filtering_rate);
    out[0] = pl.itopk; out[1] = pl.max_iterations; out[2] = pl.search_width; out[3] = (uint32_t)pl.ref_algo;
    out[4] = pl.ref_small_hash_bitlen; out[5] = pl.ref_hash_bitlen; out[6] = pl.ref_small_hash_reset_interval;
    out[7] = pl.ref_mc_num_cta_per_query; out[8] = pl.mc_max_iterations; out[9] = 0;
  });
}

// Test hook (not part of the reference ABI): the intermediate kNN graph cuvsCagraBuild optimises, by params->build_algo and
// params->metric, for a device or host dataset; knn_graph: uint32 [n, K] on the device (K <= n - 1).
extern "C" __attribute__((visibility("default"))) cuvsError_t cuvsAmdCagraBuildKnnGraph(cuvsResources_t res_h,
                                                                                        cuvsCagraIndexParams_t params,
                                                                                        DLManagedTensor* dataset_tensor,
                                                                                        DLManagedTensor* knn_tensor)
{
  return (cuvsError_t)translate_exceptions([=] {
    using namespace cuvs_amd;
    auto& res = *as_res(res_h);
    CUVS_EXPECTS(params && dataset_tensor && knn_tensor, "null argument");
    auto& ds = dataset_tensor->dl_tensor;
    auto& kg = knn_tensor->dl_tensor;
    CUVS_EXPECTS(ds.ndim == 2 && is_c_contiguous(ds), "dataset must be a row-major matrix");
    CUVS_EXPECTS(dtype_is(kg.dtype, kDLUInt, 32) && kg.ndim == 2 && is_c_contiguous(kg) && is_device_accessible(kg) &&
                   kg.shape[0] == ds.shape[0] && kg.shape[1] >= 1 && kg.shape[1] < ds.shape[0],
                 "knn_graph must be a device uint32 [n, K] matrix with K < n");
    cagra_index idx;
    idx.metric = (int)params->metric;
    idx.dtype  = elem_of(ds.dtype);
    idx.n      = ds.shape[0];
    idx.dim    = ds.shape[1];
    cagra_check_build(*params, idx.dtype);
    if (is_device_accessible(ds)) {
      idx.data = dl_data(ds);
    } else {
      idx.owned = dev_buf<char>::persistent((size_t)idx.n * idx.dim * elem_size(idx.dtype));
      copy_async(res, idx.owned.data(), dl_data(ds), idx.owned.bytes());
      idx.data = idx.owned.data();
    }
    cagra_knn_graph(res, *params, idx, (uint32_t)kg.shape[1], static_cast<uint32_t*>(dl_data(kg)));
    sync(res);
  });
}
