// Vamana (DiskANN) graph build: batched insertion = greedy search from the medoid + RobustPrune + reverse edges, and the
// DiskANN file writers (reference: cpp/src/neighbors/detail/vamana/{vamana_build,greedy_search,robust_prune,
// vamana_serialize}.cuh behind c/src/neighbors/vamana.cpp). The structure of the batch loop is the reference's; the kernels
// are written for wave64 and LDS, and every rule is fixed so that the result is ONE graph (numpy twin:
// tests/vamana_ref.py):
//   order       every comparison is on (float_to_key(distance), id); lists are sorted as packed 64-bit words
//   distance    squared L2 in fp32 by an 8-lane team: lane t takes the 16-byte pieces t, t + 8, ... of the row and adds
//               (x - q)^2 element by element in ascending order (unfused multiply, then add), the 8 partial sums are
//               combined by the xor butterfly 1, 2, 4, i.e. ((p0+p1)+(p2+p3))+((p4+p5)+(p6+p7))
//   insert order  Fisher-Yates over xorshift64* with a fixed seed;  medoid: the row nearest to the column mean
#include "common.hpp"
#include "device_utils.hpp"

#include <cuvs/neighbors/vamana.h>
#include <cuvs_amd/extensions.h>

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cfloat>
#include <fstream>
#include <memory>
#include <string>
#include <vector>

namespace cuvs_amd {
namespace {

constexpr uint32_t kInvalidNode = 0xffffffffu;
constexpr uint64_t kEmptyWord   = ~uint64_t(0);
constexpr uint32_t kMaxVisited  = 1024;  // pool of the prune: graph_degree + visited_size <= 1280 words of LDS
constexpr int kMeanChunk        = 1024;  // rows per fp64 partial sum of the column mean

struct vamana_index {
  int64_t n       = 0;
  int dim         = 0;
  uint32_t degree = 0;
  uint32_t medoid = 0;
  elem_t et       = elem_t::f32;
  dev_buf<uint32_t> graph;  // [n, degree]
  dev_buf<char> rows;       // [n, dim] of et
};

// the parameters after validation and rounding
struct build_plan {
  uint32_t degree, visited, queue;
  float alpha, iters;
  double base;
  int64_t max_batch, reverse_batch;
};

// ---------------------------------------------------------------- device helpers
template <typename T>
__device__ inline float team_l2(const T* __restrict__ row, const float* __restrict__ qf, int dim, int tl, bool ok, bool vec)
{
  constexpr int VL = 16 / sizeof(T);
  float acc        = 0.f;
  if (ok) {
    for (int d0 = tl * VL; d0 < dim; d0 += 8 * VL) {
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
          const float t = __fsub_rn(to_float(el[e]), qf[d0 + e]);
          acc           = __fadd_rn(acc, __fmul_rn(t, t));
        }
      }
    }
  }
  acc = __fadd_rn(acc, __shfl_xor(acc, 1, kWave));
  acc = __fadd_rn(acc, __shfl_xor(acc, 2, kWave));
  acc = __fadd_rn(acc, __shfl_xor(acc, 4, kWave));
  return acc;
}

template <typename T>
__device__ inline void stage_row(const T* __restrict__ row, int dim, float* __restrict__ qf)
{
  for (int d = threadIdx.x; d < dim; d += kWave) qf[d] = to_float(row[d]);
}

// bitonic sort of n (power of two, >= 64) words in LDS, ascending, by the ONE wave of the block
__device__ inline void wave_sort_words(uint64_t* w, int n)
{
  for (int size = 2; size <= n; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      for (int t = threadIdx.x; t < (n >> 1); t += kWave) {
        const int lo  = 2 * t - (t & (stride - 1));
        const int hi  = lo + stride;
        const bool up = ((lo & size) == 0);
        const uint64_t a = w[lo], b = w[hi];
        if ((a > b) == up) {
          w[lo] = b;
          w[hi] = a;
        }
      }
    }
  }
  __syncthreads();
}

__device__ inline uint64_t lanes_below(int lane) { return (uint64_t(1) << lane) - 1u; }

// ---------------------------------------------------------------- greedy search
// word of the search list: key << 32 | id << 1 | pending (1: seen, not yet expanded). The expanded copy of a node sorts
// in front of a pending copy of the same node, so dropping the later of two neighbours with the same (key, id) keeps it.
struct search_args {
  const void* data;
  int64_t n;
  int dim;
  const uint32_t* graph;
  uint32_t degree, medoid, visited, queue;
  const uint32_t* query_ids;
  int64_t b0;
  uint32_t* out_ids;  // [m, visited]
  float* out_dists;   // [m, visited]
};

template <typename T>
__global__ __launch_bounds__(64) void vamana_search_kernel(search_args a)
{
  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint64_t* w  = reinterpret_cast<uint64_t*>(smem);  // [visited] the list, sorted
  uint64_t* nw = w + a.visited;                      // [degree] the neighbours of the expanded node, as they come
  uint64_t* mg = nw + a.degree;                      // [visited + degree] the two merged
  float* qf    = reinterpret_cast<float*>(mg + a.visited + a.degree);  // [dim]
  const int lane = threadIdx.x, team = lane >> 3, tl = lane & 7;
  const int64_t b   = a.b0 + blockIdx.x;
  const uint32_t q  = a.query_ids[b];
  const T* data     = static_cast<const T*>(a.data);
  constexpr int VL  = 16 / sizeof(T);
  const bool vec    = (a.dim % VL == 0) && ((reinterpret_cast<uintptr_t>(data) & 15) == 0);
  uint32_t* out_ids = a.out_ids + b * a.visited;
  float* out_dists  = a.out_dists + b * a.visited;
  uint32_t len = 0, n_out = 0;
  if (q < a.n && a.medoid < a.n) {  // (uniform)
    stage_row(data + (int64_t)q * a.dim, a.dim, qf);
    __syncthreads();
    {
      const float d = team_l2(data + (int64_t)a.medoid * a.dim, qf, a.dim, tl, team == 0, vec);
      if (lane == 0) w[0] = (uint64_t)float_to_key(d) << 32 | (uint64_t)a.medoid << 1 | 1u;
    }
    len = 1;
    __syncthreads();
    for (uint32_t n_exp = 0; n_exp < a.visited;) {
      // the closest pending node
      uint32_t pos = kInvalidNode;
      for (uint32_t base = 0; base < len; base += kWave) {
        const uint32_t i    = base + lane;
        const uint64_t mask = __ballot(i < len && (w[i] & 1u));
        if (mask) {
          pos = base + (uint32_t)__ffsll((unsigned long long)mask) - 1u;
          break;
        }
      }
      if (pos == kInvalidNode) break;
      const uint32_t node = (uint32_t)(w[pos] >> 1) & 0x7fffffffu;
      __syncthreads();
      if (lane == 0) w[pos] &= ~uint64_t(1);
      ++n_exp;
      // its neighbours, scored 8 at a time
      const uint32_t* grow = a.graph + (int64_t)node * a.degree;
      for (uint32_t c0 = 0; c0 < a.degree; c0 += 8) {
        const uint32_t c  = c0 + team;
        const uint32_t nb = c < a.degree ? grow[c] : kInvalidNode;
        const bool ok     = nb < a.n && nb < 0x80000000u;
        const float d     = team_l2(data + (int64_t)(ok ? nb : 0) * a.dim, qf, a.dim, tl, ok, vec);
        if (tl == 0 && c < a.degree) nw[c] = ok ? ((uint64_t)float_to_key(d) << 32 | (uint64_t)nb << 1 | 1u) : kEmptyWord;
      }
      __syncthreads();
      // merge by rank: the list is sorted already, so a word's place in the sorted whole is its own index plus the number of
      // words of the other array in front of it. The neighbours are counted by a scan that every lane reads in step (an LDS
      // broadcast), the list by a binary search; of two equal words the list's goes first, of two equal neighbours the earlier
      const uint32_t total = len + a.degree;
      for (uint32_t t = lane; t < total; t += kWave) {
        const bool old   = t < len;
        const uint32_t j = t - len;
        const uint64_t x = old ? w[t] : nw[j];
        uint32_t rank    = 0;
#pragma unroll 4
        for (uint32_t i = 0; i < a.degree; ++i) {
          const uint64_t y = nw[i];
          rank += (y < x || (!old && y == x && i < j)) ? 1u : 0u;
        }
        if (old) {
          rank += t;
        } else {
          uint32_t lo = 0, hi = len;  // the number of list words <= x
          while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (w[mid] <= x) lo = mid + 1; else hi = mid;
          }
          rank += lo;
        }
        mg[rank] = x;
      }
      __syncthreads();
      // one pass: drop duplicates, keep the `queue` closest pending nodes, cut at `visited`
      uint32_t new_len = 0, pending_seen = 0;
      uint64_t carry = kEmptyWord;
      for (uint32_t base = 0; base < total; base += kWave) {
        const uint64_t cur  = base + lane < total ? mg[base + lane] : kEmptyWord;
        uint64_t prev       = __shfl_up((unsigned long long)cur, 1, kWave);
        if (lane == 0) prev = carry;
        const bool cand     = cur != kEmptyWord && (prev == kEmptyWord || (cur >> 1) != (prev >> 1));
        const bool pending  = cand && (cur & 1u);
        const uint64_t pm   = __ballot(pending);
        const uint32_t rank = pending_seen + (uint32_t)__popcll(pm & lanes_below(lane));
        const bool keep     = cand && (!pending || rank < a.queue);
        const uint64_t km   = __ballot(keep);
        const uint32_t dst  = new_len + (uint32_t)__popcll(km & lanes_below(lane));
        carry               = __shfl((unsigned long long)cur, kWave - 1, kWave);
        if (keep && dst < a.visited) w[dst] = cur;
        pending_seen += (uint32_t)__popcll(pm);
        new_len += (uint32_t)__popcll(km);
      }
      len = new_len < a.visited ? new_len : a.visited;
      __syncthreads();
    }
    // the expanded nodes of the list, without the row itself
    for (uint32_t base = 0; base < len; base += kWave) {
      const uint32_t i   = base + lane;
      const uint64_t cur = i < len ? w[i] : kEmptyWord;
      const uint32_t id  = (uint32_t)(cur >> 1) & 0x7fffffffu;
      const bool keep    = i < len && !(cur & 1u) && id != q;
      const uint64_t km  = __ballot(keep);
      if (keep) {
        const uint32_t dst = n_out + (uint32_t)__popcll(km & lanes_below(lane));
        out_ids[dst]       = id;
        out_dists[dst]     = key_to_float((uint32_t)(cur >> 32));
      }
      n_out += (uint32_t)__popcll(km);
    }
  }
  for (uint32_t i = n_out + lane; i < a.visited; i += kWave) {
    out_ids[i]   = kInvalidNode;
    out_dists[i] = FLT_MAX;
  }
}

// ---------------------------------------------------------------- RobustPrune
// word of the pool: key << 32 | id. Forward: the candidates of row node_ids[b] come from a search (cand_ids / cand_dists).
// Reverse (REV): the candidates of destination dst are the sources of the sorted edge list, edge_key = dst << 32 | key, from
// seg_start[b] while the destination stays the same, at most `visited` of them.
struct prune_args {
  const void* data;
  int64_t n;
  int dim;
  const uint32_t* graph;
  uint32_t degree, visited, cap;
  float alpha;
  int64_t b0;
  const uint32_t* node_ids;
  const uint32_t* cand_ids;
  const float* cand_dists;
  const uint32_t* seg_start;
  const uint64_t* edge_key;
  const uint32_t* edge_src;
  int64_t n_edges;
  uint32_t* out_ids;    // [m, degree] or nullptr
  uint32_t* out_keys;   // [m, degree] or nullptr
  uint32_t* graph_out;  // [n, degree] or nullptr: row `node` receives the result
};

template <typename T, bool REV>
__global__ __launch_bounds__(64) void vamana_prune_kernel(prune_args a)
{
  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint64_t* w = reinterpret_cast<uint64_t*>(smem);                                          // [cap]
  float* occ  = reinterpret_cast<float*>(smem + (size_t)a.cap * sizeof(uint64_t));          // [degree + visited]
  float* qf   = occ + ((a.degree + a.visited + 3u) & ~3u);                                  // [dim]
  const int lane = threadIdx.x, team = lane >> 3, tl = lane & 7;
  const int64_t b  = a.b0 + blockIdx.x;
  const T* data    = static_cast<const T*>(a.data);
  constexpr int VL = 16 / sizeof(T);
  const bool vec   = (a.dim % VL == 0) && ((reinterpret_cast<uintptr_t>(data) & 15) == 0);
  int64_t s        = 0;
  uint32_t p;
  if (REV) {
    s = a.seg_start[b];
    p = (uint32_t)(a.edge_key[s] >> 32);
  } else {
    p = a.node_ids[b];
  }
  uint32_t len = 0;
  if (p < a.n) {  // (uniform)
    stage_row(data + (int64_t)p * a.dim, a.dim, qf);
    for (uint32_t j = lane; j < a.visited; j += kWave) {
      uint32_t id = kInvalidNode, key = 0;
      if (REV) {
        if (s + j < a.n_edges) {
          const uint64_t e = a.edge_key[s + j];
          if ((uint32_t)(e >> 32) == p) {
            id  = a.edge_src[s + j];
            key = (uint32_t)e;
          }
        }
      } else {
        id  = a.cand_ids[b * a.visited + j];
        key = float_to_key(a.cand_dists[b * a.visited + j]);
      }
      w[j] = (id < a.n && id != p) ? ((uint64_t)key << 32 | id) : kEmptyWord;
    }
    __syncthreads();
    const uint32_t* grow = a.graph + (int64_t)p * a.degree;
    for (uint32_t c0 = 0; c0 < a.degree; c0 += 8) {
      const uint32_t c  = c0 + team;
      const uint32_t nb = c < a.degree ? grow[c] : kInvalidNode;
      const bool ok     = nb < a.n && nb != p;
      const float d     = team_l2(data + (int64_t)(ok ? nb : 0) * a.dim, qf, a.dim, tl, ok, vec);
      if (tl == 0 && c < a.degree) w[a.visited + c] = ok ? ((uint64_t)float_to_key(d) << 32 | nb) : kEmptyWord;
    }
    const uint32_t total = a.visited + a.degree;
    for (uint32_t i = total + lane; i < a.cap; i += kWave) w[i] = kEmptyWord;
    wave_sort_words(w, (int)a.cap);
    // drop the later of two neighbours with the same id (equal ids carry equal keys)
    uint64_t carry = kEmptyWord;
    for (uint32_t base = 0; base < total; base += kWave) {
      const uint64_t cur  = w[base + lane];
      uint64_t prev       = __shfl_up((unsigned long long)cur, 1, kWave);
      if (lane == 0) prev = carry;
      const bool keep     = cur != kEmptyWord && (prev == kEmptyWord || (uint32_t)cur != (uint32_t)prev);
      const uint64_t km   = __ballot(keep);
      const uint32_t dst  = len + (uint32_t)__popcll(km & lanes_below(lane));
      carry               = __shfl((unsigned long long)cur, kWave - 1, kWave);
      __syncthreads();
      if (keep) w[dst] = cur;
      len += (uint32_t)__popcll(km);
    }
    __syncthreads();
    if (len > a.degree) {
      for (uint32_t i = lane; i < len; i += kWave) occ[i] = 0.f;
      __syncthreads();
      uint32_t n_acc = 0;
      for (float cur_alpha = 1.0f; cur_alpha <= a.alpha && n_acc < a.degree; cur_alpha = (float)((double)cur_alpha * 1.2)) {
        uint32_t start = 0;
        while (n_acc < a.degree) {
          // the first entry from `start` that is neither accepted (-1) nor occluded
          uint32_t i = kInvalidNode;
          for (uint32_t base = start & ~(uint32_t)(kWave - 1); base < len; base += kWave) {
            const uint32_t k    = base + lane;
            const float o       = k < len ? occ[k] : -1.f;
            const uint64_t mask = __ballot(k >= start && k < len && o >= 0.f && o <= cur_alpha);
            if (mask) {
              i = base + (uint32_t)__ffsll((unsigned long long)mask) - 1u;
              break;
            }
          }
          if (i == kInvalidNode) break;
          __syncthreads();
          if (lane == 0) occ[i] = -1.f;
          ++n_acc;
          start = i + 1;
          if (n_acc == a.degree) break;
          stage_row(data + (int64_t)(uint32_t)w[i] * a.dim, a.dim, qf);
          __syncthreads();
          // d(accepted, k) of the live entries behind it, 8 at a time
          for (uint32_t k0 = i + 1; k0 < len; k0 += 8) {
            const uint32_t k = k0 + team;
            const float o    = k < len ? occ[k] : -1.f;
            const bool live  = k < len && o >= 0.f && o <= a.alpha;
            const uint64_t e = live ? w[k] : 0;
            const float djk  = team_l2(data + (int64_t)(uint32_t)e * a.dim, qf, a.dim, tl, live, vec);
            if (live && tl == 0) {
              const float f = djk == 0.f ? FLT_MAX : key_to_float((uint32_t)(e >> 32)) / djk;
              occ[k]        = fmaxf(o, f);
            }
          }
          __syncthreads();
        }
      }
    }
  }
  // the accepted entries (all of a pool that needed no pruning) in pool order
  const bool pruned = len > a.degree;
  uint32_t n_out    = 0;
  for (uint32_t base = 0; base < len && n_out < a.degree; base += kWave) {
    const uint32_t i  = base + lane;
    const bool keep   = i < len && (!pruned || occ[i] == -1.f);
    const uint64_t km = __ballot(keep);
    if (keep) {
      const uint32_t dst = n_out + (uint32_t)__popcll(km & lanes_below(lane));
      const uint64_t e   = w[i];
      if (a.out_ids) a.out_ids[b * a.degree + dst] = (uint32_t)e;
      if (a.out_keys) a.out_keys[b * a.degree + dst] = (uint32_t)(e >> 32);
      if (a.graph_out) a.graph_out[(int64_t)p * a.degree + dst] = (uint32_t)e;
    }
    n_out += (uint32_t)__popcll(km);
  }
  for (uint32_t i = n_out + lane; i < a.degree; i += kWave) {
    if (a.out_ids) a.out_ids[b * a.degree + i] = kInvalidNode;
    if (a.out_keys) a.out_keys[b * a.degree + i] = 0xffffffffu;
    if (a.graph_out && p < a.n) a.graph_out[(int64_t)p * a.degree + i] = kInvalidNode;
  }
}

// ---------------------------------------------------------------- reverse edges
// edge i of the batch: row r = i / degree took new_ids[i] as a neighbour -> (dst = new_ids[i], key, src = order[r])
__global__ void vamana_edges_kernel(const uint32_t* __restrict__ new_ids, const uint32_t* __restrict__ new_keys,
                                    const uint32_t* __restrict__ order, int64_t n_edges, uint32_t degree,
                                    uint64_t* __restrict__ edge_key, uint32_t* __restrict__ edge_src)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_edges) return;
  const uint32_t dst = new_ids[i];
  edge_key[i]        = dst == kInvalidNode ? kEmptyWord : ((uint64_t)dst << 32 | new_keys[i]);
  edge_src[i]        = order[i / degree];
}
// 1 where a destination's run of the sorted edge list begins
__global__ void vamana_heads_kernel(const uint64_t* __restrict__ edge_key, int64_t n_edges, uint8_t* __restrict__ head)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_edges) return;
  const uint64_t e = edge_key[i];
  head[i]          = e != kEmptyWord && (i == 0 || (uint32_t)(edge_key[i - 1] >> 32) != (uint32_t)(e >> 32));
}

// ---------------------------------------------------------------- medoid
// column sums in fp64: chunk c adds its kMeanChunk rows in order, then the chunk sums are added in order
template <typename T>
__global__ void vamana_colsum_kernel(const T* __restrict__ data, int64_t n, int dim, double* __restrict__ partial)
{
  const int j = blockIdx.y * blockDim.x + threadIdx.x;
  if (j >= dim) return;
  const int64_t r0 = (int64_t)blockIdx.x * kMeanChunk, r1 = r0 + kMeanChunk < n ? r0 + kMeanChunk : n;
  double s = 0.0;
  for (int64_t r = r0; r < r1; ++r) s += (double)to_float(data[r * dim + j]);
  partial[(int64_t)blockIdx.x * dim + j] = s;
}
__global__ void vamana_mean_kernel(const double* __restrict__ partial, int n_chunks, int dim, int64_t n, float* __restrict__ mean)
{
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= dim) return;
  double s = 0.0;
  for (int c = 0; c < n_chunks; ++c) s += partial[(int64_t)c * dim + j];
  mean[j] = (float)(s / (double)n);
}
// a wave scores 8 rows at a time against the mean; the smallest (key, id) wins, whatever the order of the atomics
template <typename T>
__global__ __launch_bounds__(64) void vamana_medoid_kernel(const T* __restrict__ data, int64_t n, int dim,
                                                           const float* __restrict__ mean, int64_t rows_per_block,
                                                           unsigned long long* __restrict__ best)
{
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* qf = reinterpret_cast<float*>(smem);
  const int lane = threadIdx.x, team = lane >> 3, tl = lane & 7;
  constexpr int VL = 16 / sizeof(T);
  const bool vec   = (dim % VL == 0) && ((reinterpret_cast<uintptr_t>(data) & 15) == 0);
  for (int d = lane; d < dim; d += kWave) qf[d] = mean[d];
  __syncthreads();
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block, r1 = r0 + rows_per_block < n ? r0 + rows_per_block : n;
  unsigned long long mine = ~0ull;
  for (int64_t c0 = r0; c0 < r1; c0 += 8) {
    const int64_t r = c0 + team;
    const bool ok   = r < r1;
    const float d   = team_l2(data + (ok ? r : 0) * dim, qf, dim, tl, ok, vec);
    if (ok) {
      const unsigned long long word = (unsigned long long)float_to_key(d) << 32 | (uint32_t)r;
      mine                          = word < mine ? word : mine;
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_xor(mine, off, kWave);
    mine                       = o < mine ? o : mine;
  }
  if (lane == 0 && mine != ~0ull) atomicMin(best, mine);
}

// ---------------------------------------------------------------- host side
uint32_t search_cap(uint32_t degree, uint32_t visited)
{
  uint32_t cap = kWave;
  while (cap < degree + visited) cap <<= 1;
  return cap;
}
size_t search_lds(uint32_t degree, uint32_t visited, int dim) { return (size_t)(degree + visited) * 16 + (size_t)dim * 4; }
size_t prune_lds(uint32_t cap, uint32_t degree, uint32_t visited, int dim)
{
  return (size_t)cap * 8 + (size_t)((degree + visited + 3u) & ~3u) * 4 + (size_t)dim * 4;
}

// every refusal of the build, before the device is touched (vamana_build.cuh:564-573, c/src/neighbors/vamana.cpp:131)
build_plan make_plan(const cuvsVamanaIndexParams& p, int64_t n, int64_t dim)
{
  CUVS_EXPECTS((int)p.metric == M_L2Expanded, "Currently only L2Expanded metric is supported");
  CUVS_EXPECTS(p.graph_degree == 32 || p.graph_degree == 64 || p.graph_degree == 128 || p.graph_degree == 256,
               "Provided graph_degree not currently supported");
  CUVS_EXPECTS(p.visited_size > p.graph_degree, "visited_size must be > graph_degree");
  CUVS_EXPECTS(p.vamana_iters >= 1.0f, "vamana_iters must be at least 1.0 to insert the entire input dataset");
  build_plan pl{};
  pl.degree  = p.graph_degree;
  pl.visited = p.visited_size;
  if ((pl.visited & (pl.visited - 1)) != 0) {  // vamana_build.cuh:126-132
    CUVS_EXPECTS(p.visited_size <= kMaxVisited, "visited_size above %u is not supported", kMaxVisited);
    uint32_t power = p.graph_degree;
    while (power < pl.visited) power <<= 1;
    pl.visited = power;
  }
  CUVS_EXPECTS(pl.visited <= kMaxVisited, "visited_size above %u is not supported", kMaxVisited);
  CUVS_EXPECTS(n >= 1 && n < (int64_t(1) << 31), "the dataset must have between 1 and 2^31 - 1 rows");
  CUVS_EXPECTS(dim >= 1 && dim < (int64_t(1) << 31), "rows must have between 1 and 2^31 - 1 elements");
  CUVS_EXPECTS(std::max(prune_lds(search_cap(pl.degree, pl.visited), pl.degree, pl.visited, (int)dim),
                        search_lds(pl.degree, pl.visited, (int)dim)) <= 64 * 1024,
               "rows of %ld elements do not fit the kernels' LDS", (long)dim);
  // (NaN fails each of these comparisons)
  CUVS_EXPECTS(p.alpha >= 1.0f, "alpha must be at least 1.0");
  CUVS_EXPECTS(p.max_fraction >= 0.0f, "max_fraction must not be negative");
  CUVS_EXPECTS(p.batch_base >= 1.0f, "batch_base must be at least 1.0");
  pl.queue     = std::max<uint32_t>(p.queue_size, 1u);
  pl.alpha     = p.alpha;
  pl.iters     = p.vamana_iters;
  pl.base      = (double)p.batch_base;
  const float mb = std::min(p.max_fraction, 1.0f) * (float)n;  // int(max_fraction * n) of the reference, at least one row, at most all
  pl.max_batch   = mb >= (float)n ? n : std::max<int64_t>((int64_t)mb, 1);
  pl.max_batch   = std::min(pl.max_batch, n);
  // the edges of a batch are indexed by 32-bit words (the run starts, the device select's count)
  CUVS_EXPECTS(pl.max_batch * pl.degree < (int64_t(1) << 31),
               "a batch of %ld rows has 2^31 edges or more: lower max_fraction or graph_degree", (long)pl.max_batch);
  pl.reverse_batch = std::max<int64_t>(p.reverse_batchsize, 1);
  return pl;
}

elem_t vamana_elem(const DLDataType& d)
{
  if (dtype_is(d, kDLFloat, 32)) return elem_t::f32;
  if (dtype_is(d, kDLInt, 8)) return elem_t::i8;
  if (dtype_is(d, kDLUInt, 8)) return elem_t::u8;
  CUVS_FAIL("Unsupported dataset DLtensor dtype: %d and bits: %d", (int)d.code, (int)d.bits);
}

// the insert order: Fisher-Yates from the back over xorshift64* seeded with 0x9E3779B97F4A7C15
std::vector<uint32_t> insert_order(int64_t n)
{
  std::vector<uint32_t> perm(n);
  for (int64_t i = 0; i < n; ++i) perm[i] = (uint32_t)i;
  uint64_t x = 0x9E3779B97F4A7C15ULL;
  for (int64_t i = n - 1; i > 0; --i) {
    x ^= x >> 12;
    x ^= x << 25;
    x ^= x >> 27;
    const uint64_t j = (x * 0x2545F4914F6CDD1DULL) % (uint64_t)(i + 1);
    std::swap(perm[i], perm[j]);
  }
  return perm;
}

#define VAMANA_DISPATCH(et, CALL)                                   \
  switch (et) {                                                     \
    case elem_t::f32: { using T = float; CALL; } break;             \
    case elem_t::i8: { using T = int8_t; CALL; } break;             \
    case elem_t::u8: { using T = uint8_t; CALL; } break;            \
    default: CUVS_FAIL("vamana: unsupported element type");         \
  }

constexpr int64_t kLaunchChunk = int64_t(1) << 22;  // workgroups per launch (64 threads each: far below the 2^32-thread grid limit)

void launch_search(resources& res, elem_t et, search_args a, int64_t m)
{
  const size_t lds = search_lds(a.degree, a.visited, a.dim);
  for (int64_t b0 = 0; b0 < m; b0 += kLaunchChunk) {
    a.b0 = b0;
    const unsigned g = (unsigned)std::min(kLaunchChunk, m - b0);
    VAMANA_DISPATCH(et, hipLaunchKernelGGL((vamana_search_kernel<T>), dim3(g), dim3(kWave), lds, res.stream, a));
    HIP_TRY(hipGetLastError());
  }
}
template <bool REV>
void launch_prune(resources& res, elem_t et, prune_args a, int64_t first, int64_t m)
{
  const size_t lds = prune_lds(a.cap, a.degree, a.visited, a.dim);
  for (int64_t b0 = 0; b0 < m; b0 += kLaunchChunk) {
    a.b0 = first + b0;
    const unsigned g = (unsigned)std::min(kLaunchChunk, m - b0);
    VAMANA_DISPATCH(et, hipLaunchKernelGGL((vamana_prune_kernel<T, REV>), dim3(g), dim3(kWave), lds, res.stream, a));
    HIP_TRY(hipGetLastError());
  }
}

uint32_t find_medoid(resources& res, elem_t et, const void* data, int64_t n, int dim)
{
  const int n_chunks = ceil_div(n, kMeanChunk);
  dev_buf<double> partial(res, (size_t)n_chunks * dim);
  dev_buf<float> mean(res, dim);
  dev_buf<unsigned long long> best(res, 1);
  HIP_TRY(hipMemsetAsync(best.data(), 0xff, sizeof(unsigned long long), res.stream));
  VAMANA_DISPATCH(et, hipLaunchKernelGGL((vamana_colsum_kernel<T>), dim3(n_chunks, ceil_div(dim, 64)), dim3(64), 0, res.stream,
                                         static_cast<const T*>(data), n, dim, partial.data()));
  hipLaunchKernelGGL(vamana_mean_kernel, dim3(ceil_div(dim, 64)), dim3(64), 0, res.stream, partial.data(), n_chunks, dim, n,
                     mean.data());
  const int64_t rows_per_block = 256;
  VAMANA_DISPATCH(et, hipLaunchKernelGGL((vamana_medoid_kernel<T>), dim3(grid_blocks(n, (int)rows_per_block)), dim3(kWave),
                                         (size_t)dim * 4, res.stream, static_cast<const T*>(data), n, dim, mean.data(),
                                         rows_per_block, best.data()));
  HIP_TRY(hipGetLastError());
  return (uint32_t)to_host(res, best.data(), 1)[0];
}

void build_graph(resources& res, const build_plan& pl, elem_t et, const void* data, int64_t n, int dim, uint32_t medoid,
                 uint32_t* graph)
{
  const uint32_t degree = pl.degree, V = pl.visited, cap = search_cap(degree, V);
  HIP_TRY(hipMemsetAsync(graph, 0xff, (size_t)n * degree * sizeof(uint32_t), res.stream));
  const std::vector<uint32_t> order_h = insert_order(n);
  dev_buf<uint32_t> order(res, n);
  copy_async(res, order.data(), order_h.data(), order.bytes());

  const int64_t mb = pl.max_batch, max_edges = mb * degree;
  dev_buf<uint32_t> vis_ids(res, (size_t)mb * V), new_ids(res, max_edges), new_keys(res, max_edges);
  dev_buf<float> vis_dists(res, (size_t)mb * V);
  dev_buf<uint64_t> edge_key(res, max_edges), edge_key2(res, max_edges);
  dev_buf<uint32_t> edge_src(res, max_edges), edge_src2(res, max_edges), seg_start(res, max_edges), n_seg(res, 1);
  dev_buf<uint8_t> head(res, max_edges);
  hipcub::CountingInputIterator<uint32_t> iota(0u);
  dev_buf<char> temp;
  auto with_temp = [&](auto&& call) {  // hipcub's two-step convention: size query, then the run
    size_t bytes = 0;
    HIP_TRY(call(static_cast<void*>(nullptr), bytes));
    if (bytes > temp.bytes()) temp = dev_buf<char>(res, bytes);
    bytes = std::max<size_t>(temp.bytes(), 1);
    HIP_TRY(call(static_cast<void*>(temp.data()), bytes));
  };

  search_args sa{data, n, dim, graph, degree, medoid, V, pl.queue, nullptr, 0, vis_ids.data(), vis_dists.data()};
  prune_args pa{};
  pa.data = data; pa.n = n; pa.dim = dim; pa.graph = graph; pa.degree = degree; pa.visited = V; pa.cap = cap; pa.alpha = pl.alpha;

  // the batch schedule of vamana_build.cuh:222-535 (float arithmetic as there)
  float iters       = pl.iters;
  int64_t step_size = 1;
  for (int64_t start = 0;;) {
    const int64_t limit = (int64_t)((double)iters * (double)n);  // (the reference's float product loses rows beyond 2^24)
    if (start >= limit) break;
    if (start + step_size > limit) step_size = limit - start;
    if (start + step_size > n) step_size = n - start;
    const int64_t m = step_size, n_edges = m * degree;

    profile_begin(res, "vamana_search");
    sa.query_ids = order.data() + start;
    launch_search(res, et, sa, m);
    profile_end(res, "vamana_search");

    profile_begin(res, "vamana_prune");
    prune_args f = pa;
    f.node_ids = order.data() + start; f.cand_ids = vis_ids.data(); f.cand_dists = vis_dists.data();
    f.out_ids = new_ids.data(); f.out_keys = new_keys.data(); f.graph_out = graph;
    launch_prune<false>(res, et, f, 0, m);
    profile_end(res, "vamana_prune");

    profile_begin(res, "vamana_reverse_sort");
    hipLaunchKernelGGL(vamana_edges_kernel, dim3(grid_blocks(n_edges, 256)), dim3(256), 0, res.stream, new_ids.data(),
                       new_keys.data(), order.data() + start, n_edges, degree, edge_key.data(), edge_src.data());
    // (dst, key, src) order: a stable sort by src, then a stable sort by dst << 32 | key
    with_temp([&](void* t, size_t& b) {
      return hipcub::DeviceRadixSort::SortPairs(t, b, edge_src.data(), edge_src2.data(), edge_key.data(), edge_key2.data(),
                                                (size_t)n_edges, 0, 32, res.stream);
    });
    with_temp([&](void* t, size_t& b) {
      return hipcub::DeviceRadixSort::SortPairs(t, b, edge_key2.data(), edge_key.data(), edge_src2.data(), edge_src.data(),
                                                (size_t)n_edges, 0, 64, res.stream);
    });
    hipLaunchKernelGGL(vamana_heads_kernel, dim3(grid_blocks(n_edges, 256)), dim3(256), 0, res.stream, edge_key.data(), n_edges,
                       head.data());
    with_temp([&](void* t, size_t& b) {
      return hipcub::DeviceSelect::Flagged(t, b, iota, head.data(), seg_start.data(), n_seg.data(), (int)n_edges, res.stream);
    });
    HIP_TRY(hipGetLastError());
    const int64_t n_dst = read_word(res, n_seg.data());  // the batch's one host round trip
    profile_end(res, "vamana_reverse_sort");

    profile_begin(res, "vamana_reverse_prune");
    prune_args r = pa;
    r.seg_start = seg_start.data(); r.edge_key = edge_key.data(); r.edge_src = edge_src.data(); r.n_edges = n_edges;
    r.graph_out = graph;
    for (int64_t d0 = 0; d0 < n_dst; d0 += pl.reverse_batch)
      launch_prune<true>(res, et, r, d0, std::min(pl.reverse_batch, n_dst - d0));
    profile_end(res, "vamana_reverse_prune");

    start += step_size;
    if (start >= n) {
      start = 0;
      iters -= 1.0f;
      step_size = pl.max_batch;
    }
    const double grown = (double)step_size * pl.base;  // truncated as the reference's int() unless the cap comes first
    step_size          = grown < (double)pl.max_batch ? std::max<int64_t>(1, (int64_t)grown) : pl.max_batch;
  }
}

const DLTensor& device_matrix(DLManagedTensor* t, const char* what)
{
  CUVS_EXPECTS(t != nullptr, "%s is null", what);
  const DLTensor& d = t->dl_tensor;
  CUVS_EXPECTS(d.ndim == 2 && is_c_contiguous(d), "%s must be a row-major matrix", what);
  CUVS_EXPECTS(is_device_accessible(d), "%s must be in device memory", what);
  return d;
}

vamana_index& built(cuvsVamanaIndex_t index)
{
  CUVS_EXPECTS(index != nullptr && index->addr != 0, "the Vamana index is not built");
  return *reinterpret_cast<vamana_index*>(index->addr);
}

void write_file(const std::string& name, const std::vector<char>& bytes)
{
  std::ofstream of(name, std::ios::out | std::ios::binary);
  CUVS_EXPECTS((bool)of, "Cannot open file %s", name.c_str());
  of.write(bytes.data(), (std::streamsize)bytes.size());
  of.close();
  CUVS_EXPECTS((bool)of, "Error writing output %s", name.c_str());
}
template <typename V>
void put(std::vector<char>& out, size_t at, V v)
{
  memcpy(out.data() + at, &v, sizeof(V));
}

// `<filename>.data`: int32 n, int32 dim, the rows (vamana_serialize.cuh:28-47)
void write_dataset(const std::string& name, const vamana_index& idx, const std::vector<char>& rows)
{
  std::vector<char> out(8 + rows.size());
  put(out, 0, (int32_t)idx.n);
  put(out, 4, (int32_t)idx.dim);
  if (!rows.empty()) memcpy(out.data() + 8, rows.data(), rows.size());
  write_file(name, out);
}

uint32_t row_edges(const uint32_t* g, uint32_t degree)
{
  uint32_t c = 0;
  while (c < degree && g[c] != kInvalidNode) ++c;
  return c;
}

void serialize(resources& res, const char* filename, cuvsVamanaIndex_t index, bool include_dataset, bool sector_aligned)
{
  CUVS_EXPECTS(filename != nullptr, "filename is null");
  vamana_index& idx = built(index);
  const std::vector<uint32_t> g = to_host(res, idx.graph.data(), idx.graph.size());
  std::vector<char> rows;
  if (include_dataset || sector_aligned) rows = to_host(res, idx.rows.data(), idx.rows.size());
  const std::string base(filename);
  const uint32_t degree = idx.degree;
  if (!sector_aligned) {  // vamana_serialize.cuh:341-399
    size_t size = 24;
    uint32_t max_degree = 0;
    for (int64_t i = 0; i < idx.n; ++i) {
      const uint32_t c = row_edges(&g[i * degree], degree);
      size += 4 * (size_t)(c + 1);
      max_degree = std::max(max_degree, c);
    }
    std::vector<char> out(size);
    put(out, 0, (uint64_t)size);
    put(out, 8, max_degree);
    put(out, 12, idx.medoid);
    put(out, 16, (uint64_t)0);
    size_t at = 24;
    for (int64_t i = 0; i < idx.n; ++i) {
      const uint32_t c = row_edges(&g[i * degree], degree);
      put(out, at, c);
      if (c) memcpy(out.data() + at + 4, &g[i * degree], 4 * (size_t)c);
      at += 4 * (size_t)(c + 1);
    }
    write_file(base, out);
  } else {  // vamana_serialize.cuh:123-297
    const uint64_t sector = 4096, npts = (uint64_t)idx.n, ndims = (uint64_t)idx.dim;
    const uint64_t row_bytes = ndims * elem_size(idx.et);
    uint32_t max_degree = 0;
    for (int64_t i = 0; i < idx.n; ++i) max_degree = std::max(max_degree, row_edges(&g[i * degree], degree));
    const uint64_t node_len = ((uint64_t)max_degree + 1) * 4 + row_bytes;
    const uint64_t per_sector = sector / node_len;  // 0: a node spans sectors
    const uint64_t sectors_per_node = (node_len + sector - 1) / sector;
    const uint64_t n_sectors = per_sector > 0 ? (npts + per_sector - 1) / per_sector : npts * sectors_per_node;
    const uint64_t file_size = (n_sectors + 1) * sector;
    std::vector<char> out(file_size, 0);
    put(out, 0, (int32_t)9);
    put(out, 4, (int32_t)1);
    const uint64_t meta[9] = {npts, ndims, (uint64_t)idx.medoid, node_len, per_sector, 0, 0, 0, file_size};
    memcpy(out.data() + 8, meta, sizeof(meta));
    for (uint64_t i = 0; i < npts; ++i) {
      const uint64_t at = per_sector > 0 ? sector * (1 + i / per_sector) + (i % per_sector) * node_len
                                         : sector * (1 + i * sectors_per_node);
      const uint32_t c = row_edges(&g[i * degree], degree);
      memcpy(out.data() + at, rows.data() + i * row_bytes, row_bytes);
      put(out, at + row_bytes, c);
      if (c) memcpy(out.data() + at + row_bytes + 4, &g[i * degree], 4 * (size_t)c);
    }
    write_file(base + "_disk.index", out);
  }
  if (include_dataset) write_dataset(base + ".data", idx, rows);
}

}  // namespace
}  // namespace cuvs_amd

extern "C" {
cuvsError_t cuvsVamanaIndexParamsCreate(cuvsVamanaIndexParams_t* params)
{
  return (cuvsError_t)cuvs_amd::translate_exceptions([=] {
    CUVS_EXPECTS(params != nullptr, "params is null");
    // defaults of c/src/neighbors/vamana.cpp:157-171
    *params = new cuvsVamanaIndexParams{L2Expanded, 32, 64, 1.0f, 1.2f, 0.06f, 2.0f, 127, 1000000};
  });
}
cuvsError_t cuvsVamanaIndexParamsDestroy(cuvsVamanaIndexParams_t params)
{
  return (cuvsError_t)cuvs_amd::translate_exceptions([=] { delete params; });
}
cuvsError_t cuvsVamanaIndexCreate(cuvsVamanaIndex_t* index)
{
  return (cuvsError_t)cuvs_amd::translate_exceptions([=] {
    CUVS_EXPECTS(index != nullptr, "index is null");
    *index = new cuvsVamanaIndex{0, DLDataType{kDLFloat, 32, 1}};
  });
}
cuvsError_t cuvsVamanaIndexDestroy(cuvsVamanaIndex_t index)
{
  return (cuvsError_t)cuvs_amd::translate_exceptions([=] {
    if (index == nullptr) return;
    delete reinterpret_cast<cuvs_amd::vamana_index*>(index->addr);
    delete index;
  });
}
cuvsError_t cuvsVamanaIndexGetDims(cuvsVamanaIndex_t index, int* dim)
{
  return (cuvsError_t)cuvs_amd::translate_exceptions([=] {
    CUVS_EXPECTS(dim != nullptr, "dim is null");
    *dim = cuvs_amd::built(index).dim;
  });
}

cuvsError_t cuvsVamanaBuild(cuvsResources_t res_h, cuvsVamanaIndexParams_t params, DLManagedTensor* dataset_tensor,
                            cuvsVamanaIndex_t index)
{
  using namespace cuvs_amd;
  return (cuvsError_t)translate_exceptions([=] {
    CUVS_EXPECTS(params && dataset_tensor && index, "null argument");
    const DLTensor& ds = dataset_tensor->dl_tensor;
    const elem_t et    = vamana_elem(ds.dtype);
    CUVS_EXPECTS(ds.ndim == 2 && is_c_contiguous(ds), "dataset must be a row-major matrix");
    const int64_t n = ds.shape[0], dim = ds.shape[1];
    const build_plan pl = make_plan(*params, n, dim);
    resources& res      = *as_res(res_h);
    auto idx    = std::make_unique<vamana_index>();
    idx->n      = n;
    idx->dim    = (int)dim;
    idx->degree = pl.degree;
    idx->et     = et;
    idx->rows   = dev_buf<char>::persistent((size_t)n * dim * elem_size(et));
    idx->graph  = dev_buf<uint32_t>::persistent((size_t)n * pl.degree);
    copy_async(res, idx->rows.data(), dl_data(ds), idx->rows.bytes());  // host or device: the index keeps its own copy
    idx->medoid = find_medoid(res, et, idx->rows.data(), n, (int)dim);
    build_graph(res, pl, et, idx->rows.data(), n, (int)dim, idx->medoid, idx->graph.data());
    sync(res);
    delete reinterpret_cast<vamana_index*>(index->addr);
    index->addr  = reinterpret_cast<uintptr_t>(idx.release());
    index->dtype = ds.dtype;
  });
}

cuvsError_t cuvsVamanaSerialize(cuvsResources_t res_h, const char* filename, cuvsVamanaIndex_t index, bool include_dataset)
{
  using namespace cuvs_amd;
  return (cuvsError_t)translate_exceptions([=] { serialize(*as_res(res_h), filename, index, include_dataset, false); });
}
cuvsError_t cuvsAmdVamanaSerializeSectorAligned(cuvsResources_t res_h, const char* filename, cuvsVamanaIndex_t index,
                                                bool include_dataset)
{
  using namespace cuvs_amd;
  return (cuvsError_t)translate_exceptions([=] { serialize(*as_res(res_h), filename, index, include_dataset, true); });
}

cuvsError_t cuvsAmdVamanaIndexGetGraph(cuvsResources_t res_h, cuvsVamanaIndex_t index, DLManagedTensor* out)
{
  using namespace cuvs_amd;
  return (cuvsError_t)translate_exceptions([=] {
    vamana_index& idx = built(index);
    CUVS_EXPECTS(out != nullptr, "out is null");
    const DLTensor& g = out->dl_tensor;
    CUVS_EXPECTS(dtype_is(g.dtype, kDLUInt, 32) && g.ndim == 2 && is_c_contiguous(g) && g.shape[0] == idx.n &&
                   g.shape[1] == idx.degree,
                 "out must be uint32 [%ld, %u]", (long)idx.n, idx.degree);
    resources& res = *as_res(res_h);
    copy_async(res, dl_data(g), idx.graph.data(), idx.graph.bytes());
    sync(res);
  });
}
cuvsError_t cuvsAmdVamanaIndexGetMedoid(cuvsVamanaIndex_t index, uint32_t* medoid)
{
  return (cuvsError_t)cuvs_amd::translate_exceptions([=] {
    CUVS_EXPECTS(medoid != nullptr, "medoid is null");
    *medoid = cuvs_amd::built(index).medoid;
  });
}

cuvsError_t cuvsAmdVamanaGreedySearch(cuvsResources_t res_h, cuvsVamanaIndexParams_t params, DLManagedTensor* dataset,
                                      DLManagedTensor* graph, uint32_t medoid, DLManagedTensor* query_ids,
                                      DLManagedTensor* out_ids, DLManagedTensor* out_dists)
{
  using namespace cuvs_amd;
  return (cuvsError_t)translate_exceptions([=] {
    CUVS_EXPECTS(params != nullptr, "params is null");
    const DLTensor& ds = device_matrix(dataset, "dataset");
    const elem_t et    = vamana_elem(ds.dtype);
    const int64_t n = ds.shape[0], dim = ds.shape[1];
    const build_plan pl = make_plan(*params, n, dim);
    const DLTensor& g   = device_matrix(graph, "graph");
    CUVS_EXPECTS(dtype_is(g.dtype, kDLUInt, 32) && g.shape[0] == n && g.shape[1] == pl.degree,
                 "graph must be uint32 [n, graph_degree]");
    CUVS_EXPECTS(query_ids != nullptr && out_ids != nullptr && out_dists != nullptr, "null argument");
    const DLTensor& q = query_ids->dl_tensor;
    CUVS_EXPECTS(dtype_is(q.dtype, kDLUInt, 32) && q.ndim == 1 && is_c_contiguous(q) && is_device_accessible(q),
                 "query_ids must be a uint32 vector in device memory");
    const int64_t m    = q.shape[0];
    const DLTensor& oi = device_matrix(out_ids, "out_ids");
    const DLTensor& od = device_matrix(out_dists, "out_dists");
    CUVS_EXPECTS(dtype_is(oi.dtype, kDLUInt, 32) && oi.shape[0] == m && oi.shape[1] == pl.visited,
                 "out_ids must be uint32 [m, %u]", pl.visited);
    CUVS_EXPECTS(dtype_is(od.dtype, kDLFloat, 32) && od.shape[0] == m && od.shape[1] == pl.visited,
                 "out_dists must be float32 [m, %u]", pl.visited);
    CUVS_EXPECTS(medoid < n, "medoid must be a row of the dataset");
    resources& res = *as_res(res_h);
    search_args a{dl_data(ds), n, (int)dim, static_cast<const uint32_t*>(dl_data(g)), pl.degree, medoid, pl.visited, pl.queue,
                  static_cast<const uint32_t*>(dl_data(q)), 0,
                  static_cast<uint32_t*>(dl_data(oi)), static_cast<float*>(dl_data(od))};
    if (m > 0) launch_search(res, et, a, m);
  });
}

cuvsError_t cuvsAmdVamanaRobustPrune(cuvsResources_t res_h, cuvsVamanaIndexParams_t params, DLManagedTensor* dataset,
                                     DLManagedTensor* graph, DLManagedTensor* node_ids, DLManagedTensor* cand_ids,
                                     DLManagedTensor* cand_dists, DLManagedTensor* out_ids)
{
  using namespace cuvs_amd;
  return (cuvsError_t)translate_exceptions([=] {
    CUVS_EXPECTS(params != nullptr, "params is null");
    const DLTensor& ds = device_matrix(dataset, "dataset");
    const elem_t et    = vamana_elem(ds.dtype);
    const int64_t n = ds.shape[0], dim = ds.shape[1];
    const build_plan pl = make_plan(*params, n, dim);
    const DLTensor& g   = device_matrix(graph, "graph");
    CUVS_EXPECTS(dtype_is(g.dtype, kDLUInt, 32) && g.shape[0] == n && g.shape[1] == pl.degree,
                 "graph must be uint32 [n, graph_degree]");
    CUVS_EXPECTS(node_ids != nullptr, "node_ids is null");
    const DLTensor& q = node_ids->dl_tensor;
    CUVS_EXPECTS(dtype_is(q.dtype, kDLUInt, 32) && q.ndim == 1 && is_c_contiguous(q) && is_device_accessible(q),
                 "node_ids must be a uint32 vector in device memory");
    const int64_t m    = q.shape[0];
    const DLTensor& ci = device_matrix(cand_ids, "cand_ids");
    const DLTensor& cd = device_matrix(cand_dists, "cand_dists");
    const DLTensor& oi = device_matrix(out_ids, "out_ids");
    CUVS_EXPECTS(dtype_is(ci.dtype, kDLUInt, 32) && ci.shape[0] == m && ci.shape[1] == pl.visited,
                 "cand_ids must be uint32 [m, %u]", pl.visited);
    CUVS_EXPECTS(dtype_is(cd.dtype, kDLFloat, 32) && cd.shape[0] == m && cd.shape[1] == pl.visited,
                 "cand_dists must be float32 [m, %u]", pl.visited);
    CUVS_EXPECTS(dtype_is(oi.dtype, kDLUInt, 32) && oi.shape[0] == m && oi.shape[1] == pl.degree,
                 "out_ids must be uint32 [m, %u]", pl.degree);
    resources& res = *as_res(res_h);
    prune_args a{};
    a.data = dl_data(ds); a.n = n; a.dim = (int)dim; a.graph = static_cast<const uint32_t*>(dl_data(g));
    a.degree = pl.degree; a.visited = pl.visited; a.cap = search_cap(pl.degree, pl.visited); a.alpha = pl.alpha;
    a.node_ids = static_cast<const uint32_t*>(dl_data(q)); a.cand_ids = static_cast<const uint32_t*>(dl_data(ci));
    a.cand_dists = static_cast<const float*>(dl_data(cd)); a.out_ids = static_cast<uint32_t*>(dl_data(oi));
    if (m > 0) launch_prune<false>(res, et, a, 0, m);
  });
}
}  // extern "C"
