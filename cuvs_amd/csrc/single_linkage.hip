// Single-linkage clustering (include/cuvs_amd/single_linkage.h; semantics of the reference's cuvs::cluster::agglomerative,
// cpp/src/cluster/detail/{single_linkage,mst,connectivities,agglomerative}.cuh). DESIGN 3.1v.
//
// Contract: the base distance of a pair is the fp32 chain acc = fmaf(d, d, acc) from 0, d = x[i][t] - x[j][t], t ascending
// (its correctly rounded square root for the Sqrt metrics); every edge weight, whoever computes it, is sl_weight of that
// chain; edges are totally ordered by (bits(w), min(i, j), max(i, j)). Under a strict total order the minimum spanning
// forest is unique, so Boruvka rounds - every component takes its smallest outgoing edge - give the same tree whatever the
// scheduling; all reductions are integer minima.
//
// One Boruvka round, over the kNN graph (sparse) or over the complete graph (dense), is
//   row best   row_best[i] = min over the offered j with color[j] != color[i] of (bits(w) << 32 | j)
//              sparse: sl_edge_best_kernel, a thread per directed edge; dense: sl_tile_kernel, the 128 x 128 VALU pair tile
//              of eps_neighbors.hip (k-major LDS staging, 8 x 8 accumulators per thread, persistent workgroups) with one
//              64-bit atomicMin per (row, tile)
//   component  comp_w[c] = min bits(w) over the rows of c; comp_pair[c] = min (min(i, j) << 32 | max(i, j)) over the rows that
//              attain it (the full key does not fit 64 bits, hence two passes)
//   hook       the representative c of a component with an edge moves under the component at the edge's other end and
//              records the edge in its own slot (a representative is retired once, so slot c is written once); of a mutual
//              pick the smaller representative stays a root and the edge is recorded once
//   jump       pointer jumping to the roots, then every row takes the root of its representative
// The recorded slots are sorted by the key, the n - 1 edges go to the host, and the union-find of the dendrogram runs there
// (n - 1 sequential steps, as in the reference). Labels: a thread per dendrogram slot walks up to a labelled ancestor.
//
// The tile's load / stage / accumulate code is a copy of eps_tile_kernel's, not a shared header: that kernel sits at the
// register budget of three waves per SIMD and its code must not move.
#include "common.hpp"
#include "dl_desc.hpp"
#include "single_linkage_host.hpp"

#include <cuvs/neighbors/brute_force.h>
#include <cuvs_amd/single_linkage.h>

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <string>
#include <vector>

namespace cuvs_amd {
namespace {

namespace H = sl_host;

constexpr int kT       = eps_host::kTile;
constexpr int kKB      = 16;
constexpr int kThreads = 256;
constexpr int kWgPerCu = 3;  // persistent workgroups per CU: the tile kernel holds 144 VGPRs, three waves fit a SIMD (16 KiB LDS each)
constexpr unsigned long long kNoKey = ~0ull;

typedef float f2 __attribute__((ext_vector_type(2)));
typedef float f4 __attribute__((ext_vector_type(4)));

thread_local uint64_t g_sl_stats[6] = {0, 0, 0, 0, 0, 0};

// the one edge-weight function: `chain` of the pair, the rows' core distances (mutual reachability only)
__device__ inline float sl_weight(float chain, bool sq, bool mr, float core_i, float core_j, float alpha)
{
  const float d = sq ? sqrtf(chain) : chain;  // correctly rounded (the compiler's default for fp32 sqrt in HIP)
  return mr ? fmaxf(core_i, fmaxf(core_j, alpha * d)) : d;
}

// eight consecutive elements k .. k + 7 of one row; zero past `dim` and for a row outside the matrix
__device__ inline void sl_load8(const float* __restrict__ base, int64_t row, bool row_ok, int64_t dim, int64_t k, bool vec, float out[8])
{
  const float* p = base + row * dim + k;
  if (vec && row_ok && k + 8 <= dim) {
    const f4 v0 = *reinterpret_cast<const f4*>(p), v1 = *reinterpret_cast<const f4*>(p + 4);
    out[0] = v0.x; out[1] = v0.y; out[2] = v0.z; out[3] = v0.w;
    out[4] = v1.x; out[5] = v1.y; out[6] = v1.z; out[7] = v1.w;
    return;
  }
#pragma unroll
  for (int c = 0; c < 8; ++c) out[c] = (row_ok && k + c < dim) ? p[c] : 0.f;
}

struct sl_tile_args {
  int64_t n, dim;
  int vec_rows;  // rows are 16-byte aligned and dim is a multiple of 4
  int sq, mr;
  float alpha;
  const float* core;             // [n] (mr)
  const int* color;              // [n]
  unsigned long long* row_best;  // [n]
};

// Thread (ty, tx) of the 16 x 16 grid owns rows {64 h + 4 ty + c} and columns {16 j + tx}; the column operand sits in LDS at
// the permuted position 64 (j / 4) + 4 tx + j % 4 so that a thread's eight columns are two 16-byte reads (eps_tile_kernel).
__global__ __launch_bounds__(kThreads) void sl_tile_kernel(const float* __restrict__ x, sl_tile_args a)
{
  __shared__ __attribute__((aligned(16))) float xs[kKB][kT];
  __shared__ __attribute__((aligned(16))) float ys[kKB][kT];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tx = lane & 15, ty = wave * 4 + (lane >> 4);
  const int p = tid & (kT - 1), kh = tid >> 7;
  const int ycol_of_p = (((p >> 6) << 2) | (p & 3)) * 16 + ((p & 63) >> 2);

  const int64_t side  = (a.n + kT - 1) / kT;
  const int64_t tiles = side * side;

  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t rt = tile / side, ct = tile - rt * side;
    const int64_t row0 = rt * kT, col0 = ct * kT;

    f2 acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = (f2)(0.f);

    const int64_t xrow = row0 + p, yrow = col0 + ycol_of_p;
    const bool x_ok = xrow < a.n, y_ok = yrow < a.n;
    float px[8], py[8];
    sl_load8(x, xrow, x_ok, a.dim, (int64_t)kh * 8, a.vec_rows != 0, px);
    sl_load8(x, yrow, y_ok, a.dim, (int64_t)kh * 8, a.vec_rows != 0, py);
    for (int64_t k0 = 0; k0 < a.dim; k0 += kKB) {
      __syncthreads();  // the previous chunk has been read
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        xs[kh * 8 + c][p] = px[c];
        ys[kh * 8 + c][p] = py[c];
      }
      __syncthreads();
      if (k0 + kKB < a.dim) {  // the next chunk is in flight while this one is computed
        sl_load8(x, xrow, x_ok, a.dim, k0 + kKB + kh * 8, a.vec_rows != 0, px);
        sl_load8(x, yrow, y_ok, a.dim, k0 + kKB + kh * 8, a.vec_rows != 0, py);
      }
#pragma unroll
      for (int kk = 0; kk < kKB; ++kk) {
        const f4 a0 = *reinterpret_cast<const f4*>(&xs[kk][ty * 4]);
        const f4 a1 = *reinterpret_cast<const f4*>(&xs[kk][64 + ty * 4]);
        const f4 b0 = *reinterpret_cast<const f4*>(&ys[kk][tx * 4]);
        const f4 b1 = *reinterpret_cast<const f4*>(&ys[kk][64 + tx * 4]);
        const float av[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
        const f2 bv[4]    = {b0.xy, b0.zw, b1.xy, b1.zw};
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const f2 d = (f2)(av[i]) - bv[j];
            acc[i][j]  = __builtin_elementwise_fma(d, d, acc[i][j]);
          }
      }
    }

    // ---- nearest row of another component: per row the smallest (bits(w) << 32 | j) over the thread's eight columns, then
    // over the 16 threads that share the row (the lanes that differ in tx), then one atomicMin
    int ccol[8];
    float kcol[8];
    bool ok_c[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int64_t col = col0 + j * 16 + tx;
      ok_c[j] = col < a.n;
      ccol[j] = ok_c[j] ? a.color[col] : -1;
      kcol[j] = (a.mr && ok_c[j]) ? a.core[col] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int64_t row = row0 + (i >> 2) * 64 + ty * 4 + (i & 3);
      const bool ok_r   = row < a.n;
      const int crow    = ok_r ? a.color[row] : -1;
      const float krow  = (a.mr && ok_r) ? a.core[row] : 0.f;
      // (the thread's columns ascend with j, so a strict comparison of the weights alone keeps the smallest j of a tie)
      uint32_t best_w = 0xffffffffu, best_j = 0xffffffffu;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float v    = (j & 1) ? acc[i][j >> 1].y : acc[i][j >> 1].x;
        const uint32_t w = __float_as_uint(sl_weight(v, a.sq != 0, a.mr != 0, krow, kcol[j], a.alpha));
        if (ok_c[j] && crow != ccol[j] && (w < best_w || best_j == 0xffffffffu)) {  // (i == j has one colour)
          best_w = w;
          best_j = (uint32_t)(col0 + j * 16 + tx);
        }
      }
      unsigned long long best = (ok_r && best_j != 0xffffffffu) ? (((unsigned long long)best_w << 32) | best_j) : kNoKey;
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) {
        const unsigned long long other = __shfl_xor(best, o, 64);
        if (other < best) best = other;
      }
      // the row's value only ever falls, so a candidate that does not beat a plain (possibly stale) read of it cannot win:
      // after the first few column tiles of a row nearly every atomic is saved
      if (tx == 0 && best != kNoKey && best < __atomic_load_n(a.row_best + row, __ATOMIC_RELAXED)) atomicMin(a.row_best + row, best);
    }
  }
}

// ---------------------------------------------------------------- the kNN graph as a list of directed edges
// both directions of every (row, neighbour) entry as src << 32 | dst; self entries and ids outside the matrix become kNoKey
__global__ void sl_emit_kernel(const int64_t* __restrict__ ids, int64_t n, int64_t k, unsigned long long* __restrict__ keys)
{
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n * k) return;
  const int64_t i = e / k, j = ids[e];
  const bool ok = j >= 0 && j < n && j != i;
  keys[2 * e]     = ok ? (((unsigned long long)i << 32) | (unsigned long long)j) : kNoKey;
  keys[2 * e + 1] = ok ? (((unsigned long long)j << 32) | (unsigned long long)i) : kNoKey;
}

// bits(w) of every directed edge: a thread per edge runs the chain
__global__ void sl_reweight_kernel(const float* __restrict__ x, int64_t dim, const unsigned long long* __restrict__ keys, int64_t n_edges,
                                   int sq, int mr, float alpha, const float* __restrict__ core, uint32_t* __restrict__ w_bits)
{
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_edges) return;
  const int64_t i = (int64_t)(keys[e] >> 32), j = (int64_t)(keys[e] & 0xffffffffull);
  const float* xi = x + i * dim;
  const float* xj = x + j * dim;
  float acc = 0.f;
  for (int64_t t = 0; t < dim; ++t) {
    const float d = xi[t] - xj[t];
    acc = fmaf(d, d, acc);
  }
  w_bits[e] = __float_as_uint(sl_weight(acc, sq != 0, mr != 0, mr ? core[i] : 0.f, mr ? core[j] : 0.f, alpha));
}

__global__ void sl_edge_best_kernel(const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ w_bits, int64_t n_edges,
                                    const int* __restrict__ color, unsigned long long* __restrict__ row_best)
{
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_edges) return;
  const uint32_t s = (uint32_t)(keys[e] >> 32), d = (uint32_t)keys[e];
  if (color[s] != color[d]) atomicMin(row_best + s, ((unsigned long long)w_bits[e] << 32) | d);
}

// ---------------------------------------------------------------- the steps every round shares
__global__ void sl_init_kernel(int64_t n, int* __restrict__ color, uint32_t* __restrict__ mst_w, unsigned long long* __restrict__ mst_pair)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  color[i]    = (int)i;
  mst_w[i]    = 0xffffffffu;
  mst_pair[i] = kNoKey;
}

__global__ void sl_comp_w_kernel(int64_t n, const int* __restrict__ color, const unsigned long long* __restrict__ row_best,
                                 uint32_t* __restrict__ comp_w)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned long long b = row_best[i];
  if (b != kNoKey) atomicMin(comp_w + color[i], (uint32_t)(b >> 32));
}

__global__ void sl_comp_pair_kernel(int64_t n, const int* __restrict__ color, const unsigned long long* __restrict__ row_best,
                                    const uint32_t* __restrict__ comp_w, unsigned long long* __restrict__ comp_pair)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned long long b = row_best[i];
  if (b == kNoKey) return;
  const int c = color[i];
  if ((uint32_t)(b >> 32) != comp_w[c]) return;
  // the smallest j of row i gives the row's smallest (min, max) pair: below i it is the smallest first entry, above i the
  // smallest second entry
  const unsigned long long j = b & 0xffffffffull, ii = (unsigned long long)i;
  atomicMin(comp_pair + c, j < ii ? ((j << 32) | ii) : ((ii << 32) | j));
}

// counters[0]: components hooked in this round
__global__ void sl_hook_kernel(int64_t n, const int* __restrict__ color, const uint32_t* __restrict__ comp_w,
                               const unsigned long long* __restrict__ comp_pair, int* __restrict__ parent, uint32_t* __restrict__ mst_w,
                               unsigned long long* __restrict__ mst_pair, uint32_t* __restrict__ counters)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || color[i] != (int)i) return;
  const int c = (int)i;
  const unsigned long long pair = comp_pair[c];
  int up = c;
  if (pair != kNoKey) {
    const int ca = color[pair >> 32], cb = color[pair & 0xffffffffull];
    const int other   = ca == c ? cb : ca;
    const bool mutual = comp_pair[other] == pair;
    if (!(mutual && c < other)) {
      up          = other;
      mst_w[c]    = comp_w[c];
      mst_pair[c] = pair;
      atomicAdd(counters, 1u);
    }
  }
  parent[c] = up;
}

// every representative ends under its root. A pointer only ever moves to an ancestor and a root never moves, so reading
// another thread's pointer before or after its update is equally right.
__global__ void sl_jump_kernel(int64_t n, const int* __restrict__ color, int* parent)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || color[i] != (int)i) return;
  int up = __atomic_load_n(parent + i, __ATOMIC_RELAXED);
  for (;;) {
    const int above = __atomic_load_n(parent + up, __ATOMIC_RELAXED);
    if (above == up) break;
    __atomic_store_n(parent + i, above, __ATOMIC_RELAXED);
    up = above;
  }
}

__global__ void sl_recolor_kernel(int64_t n, int* __restrict__ color, const int* __restrict__ parent)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) color[i] = parent[color[i]];
}

// ---------------------------------------------------------------- labels
// levels[v]: the merge that consumes node v (the reference's write_levels_kernel)
__global__ void sl_levels_kernel(const int64_t* __restrict__ children, int64_t n_slots, int* __restrict__ levels)
{
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n_slots) levels[children[t]] = (int)(t / 2);
}

__global__ void sl_label_roots_kernel(const int64_t* __restrict__ roots, int64_t n_clusters, int* __restrict__ labels)
{
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n_clusters) labels[roots[t]] = (int)t;
}

// a thread per dendrogram slot at or below the cut walks up to a labelled ancestor (the reference's inherit_labels). A label
// is written once, so a walk that reads it early goes on upwards to the same answer.
__global__ void sl_inherit_kernel(const int64_t* __restrict__ children, const int* __restrict__ levels, int64_t n, int* labels,
                                  int cut_level, int64_t n_slots)
{
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_slots) return;
  const int64_t node = children[t];
  int level          = (int)(t / 2);
  if (level > cut_level) return;
  int label = __atomic_load_n(labels + node, __ATOMIC_RELAXED);
  for (int64_t step = 0; label == -1 && step < n; ++step) {  // (a dendrogram is at most n - 1 levels deep)
    const int64_t up = level + n;
    level            = levels[up];
    label            = __atomic_load_n(labels + up, __ATOMIC_RELAXED);
  }
  __atomic_store_n(labels + node, label, __ATOMIC_RELAXED);
}

template <typename IdxT>
__global__ void sl_write_labels_kernel(const int* __restrict__ labels, int64_t n, IdxT* __restrict__ out)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = (IdxT)labels[i];
}

// ---------------------------------------------------------------- host side
#define SL_LAUNCH(kernel, items, ...)                                                                              \
  do {                                                                                                             \
    hipLaunchKernelGGL(kernel, dim3(grid_blocks((items), kThreads)), dim3(kThreads), 0, res.stream, __VA_ARGS__); \
    HIP_TRY(hipGetLastError());                                                                                    \
  } while (0)

// a DLManagedTensor describing device memory for the library's own entry points
struct dl_view {
  DLManagedTensor m{};
  int64_t shape[2];
  dl_view(void* data, uint8_t code, uint8_t bits, int64_t rows, int64_t cols, int device)
  {
    shape[0] = rows; shape[1] = cols;
    m.dl_tensor.data        = data;
    m.dl_tensor.device      = {kDLROCM, device};
    m.dl_tensor.ndim        = cols < 0 ? 1 : 2;
    m.dl_tensor.dtype       = {code, bits, 1};
    m.dl_tensor.shape       = shape;
    m.dl_tensor.strides     = nullptr;
    m.dl_tensor.byte_offset = 0;
  }
};

void c_check(cuvsError_t e, const char* what)
{
  if (e != CUVS_SUCCESS) CUVS_FAIL("%s: %s", what, last_error_text().c_str());
}

struct sl_params {
  int metric, space, linkage, c, min_samples;
  float alpha;
  cuvsAllNeighborsIndexParams_t an;
};

struct sl_tree {  // the n - 1 edges in ascending key order
  std::vector<int64_t> src, dst;
  std::vector<float> w;
};

struct sl_state {
  dev_buf<int> color, parent;
  dev_buf<unsigned long long> row_best, comp_pair, mst_pair;
  dev_buf<uint32_t> comp_w, mst_w, counters;
};

// the steps after row_best is filled; returns the components hooked
uint32_t finish_round(resources& res, sl_state& s, int64_t n)
{
  SL_LAUNCH(sl_comp_w_kernel, n, n, s.color.data(), s.row_best.data(), s.comp_w.data());
  SL_LAUNCH(sl_comp_pair_kernel, n, n, s.color.data(), s.row_best.data(), s.comp_w.data(), s.comp_pair.data());
  SL_LAUNCH(sl_hook_kernel, n, n, s.color.data(), s.comp_w.data(), s.comp_pair.data(), s.parent.data(), s.mst_w.data(),
            s.mst_pair.data(), s.counters.data());
  SL_LAUNCH(sl_jump_kernel, n, n, s.color.data(), s.parent.data());
  SL_LAUNCH(sl_recolor_kernel, n, n, s.color.data(), s.parent.data());
  return read_word(res, s.counters.data());
}

void begin_round(resources& res, sl_state& s)
{
  HIP_TRY(hipMemsetAsync(s.row_best.data(), 0xff, s.row_best.bytes(), res.stream));
  HIP_TRY(hipMemsetAsync(s.comp_w.data(), 0xff, s.comp_w.bytes(), res.stream));
  HIP_TRY(hipMemsetAsync(s.comp_pair.data(), 0xff, s.comp_pair.bytes(), res.stream));
  HIP_TRY(hipMemsetAsync(s.counters.data(), 0, s.counters.bytes(), res.stream));
}

template <typename Call>
void with_temp(resources& res, dev_buf<char>& temp, Call&& call)  // hipcub's two-step convention: size query, then the run
{
  size_t bytes = 0;
  HIP_TRY(call(static_cast<void*>(nullptr), bytes));
  if (bytes > temp.bytes()) temp = dev_buf<char>(res, bytes);
  bytes = std::max<size_t>(temp.bytes(), 1);
  HIP_TRY(call(static_cast<void*>(temp.data()), bytes));
}

// the linkage: kNN graph (unless PAIRWISE), sparse rounds, dense rounds, the sort by key. `core` is the caller's [n] buffer
// in mutual-reachability space (written here), null otherwise.
sl_tree linkage(cuvsResources_t res_h, resources& res, DLManagedTensor* X, int64_t n, int64_t dim, const sl_params& p, float* core)
{
  uint64_t* st = g_sl_stats;
  for (int i = 0; i < 6; ++i) st[i] = 0;
  const float* x = static_cast<const float*>(dl_data(X->dl_tensor));
  const bool sq = metric_is_sqrt(p.metric), mr = p.space == H::kMutualReachability;
  const bool graph = mr || p.linkage == H::kKnnGraph;

  sl_state s;
  s.color     = dev_buf<int>(res, (size_t)n);
  s.parent    = dev_buf<int>(res, (size_t)n);
  s.row_best  = dev_buf<unsigned long long>(res, (size_t)n);
  s.comp_pair = dev_buf<unsigned long long>(res, (size_t)n);
  s.mst_pair  = dev_buf<unsigned long long>(res, (size_t)n);
  s.comp_w    = dev_buf<uint32_t>(res, (size_t)n);
  s.mst_w     = dev_buf<uint32_t>(res, (size_t)n);
  s.counters  = dev_buf<uint32_t>(res, 2);
  dev_buf<char> temp;
  SL_LAUNCH(sl_init_kernel, n, n, s.color.data(), s.mst_w.data(), s.mst_pair.data());
  int64_t comps = n;

  if (graph) {
    // ---- kNN ids: the public searches; their distances are in the expanded form and are discarded
    const int64_t k = mr ? p.min_samples : H::build_k(n, p.c);
    CUVS_EXPECTS(2 * n * k < (int64_t(1) << 31), "the kNN graph holds %lld directed entries; at most 2^31 - 1 are supported",
                 (long long)(2 * n * k));
    st[0] = (uint64_t)k;
    profile_begin(res, "sl_knn");
    dev_buf<int64_t> ids(res, (size_t)(n * k));
    dev_buf<unsigned long long> keys(res, (size_t)(2 * n * k)), edges(res, (size_t)(2 * n * k));
    {
      dev_buf<float> dist(res, (size_t)(n * k));
      dl_view ids_t(ids.data(), kDLInt, 64, n, k, res.device), dist_t(dist.data(), kDLFloat, 32, n, k, res.device);
      if (mr) {
        cuvsAllNeighborsIndexParams an = p.an != nullptr
                                           ? *p.an
                                           : cuvsAllNeighborsIndexParams{CUVS_ALL_NEIGHBORS_ALGO_BRUTE_FORCE, 1, 1, L2Expanded, nullptr, nullptr};
        an.metric = (cuvsDistanceType)p.metric;
        dl_view core_t(core, kDLFloat, 32, n, -1, res.device);
        c_check(cuvsAllNeighborsBuild(res_h, &an, X, &ids_t.m, &dist_t.m, &core_t.m, p.alpha), "cuvsAllNeighborsBuild");
      } else {
        cuvsBruteForceIndex_t index = nullptr;
        c_check(cuvsBruteForceIndexCreate(&index), "cuvsBruteForceIndexCreate");
        cuvsError_t e = cuvsBruteForceBuild(res_h, X, (cuvsDistanceType)p.metric, 2.0f, index);
        if (e == CUVS_SUCCESS) e = cuvsBruteForceSearch(res_h, index, X, &ids_t.m, &dist_t.m, cuvsFilter{0, NO_FILTER});
        const std::string text = e == CUVS_SUCCESS ? std::string() : last_error_text();
        cuvsBruteForceIndexDestroy(index);
        if (e != CUVS_SUCCESS) CUVS_FAIL("brute-force kNN: %s", text.c_str());
      }
    }
    profile_end(res, "sl_knn");
    // ---- symmetrise and de-duplicate: sort the directed entries, keep the first of every run
    profile_begin(res, "sl_symmetrise");
    SL_LAUNCH(sl_emit_kernel, n * k, ids.data(), n, k, keys.data());
    with_temp(res, temp, [&](void* t, size_t& b) {
      return hipcub::DeviceRadixSort::SortKeys(t, b, keys.data(), edges.data(), (int)(2 * n * k), 0, 64, res.stream);
    });
    with_temp(res, temp, [&](void* t, size_t& b) {
      return hipcub::DeviceSelect::Unique(t, b, edges.data(), keys.data(), s.counters.data() + 1, (int)(2 * n * k), res.stream);
    });
    int64_t n_edges = read_word(res, s.counters.data() + 1);
    if (n_edges > 0 && to_host(res, keys.data() + n_edges - 1, 1)[0] == kNoKey) --n_edges;  // the run of dropped entries
    st[1] = (uint64_t)(n_edges / 2);
    profile_end(res, "sl_symmetrise");
    ids   = dev_buf<int64_t>();
    edges = dev_buf<unsigned long long>();
    if (n_edges > 0) {
      dev_buf<uint32_t> w_bits(res, (size_t)n_edges);
      profile_begin(res, "sl_sparse_rounds");  // (with the re-weighting)
      SL_LAUNCH(sl_reweight_kernel, n_edges, x, dim, keys.data(), n_edges, (int)sq, (int)mr, p.alpha, core, w_bits.data());
      // ---- the forest of the graph: rounds until no component has an edge that leaves it
      while (comps > 1) {
        begin_round(res, s);
        SL_LAUNCH(sl_edge_best_kernel, n_edges, keys.data(), w_bits.data(), n_edges, s.color.data(), s.row_best.data());
        const uint32_t hooked = finish_round(res, s, n);
        if (hooked == 0) break;
        comps -= hooked;
        st[2] += 1;
      }
      profile_end(res, "sl_sparse_rounds");
    }
  }
  st[3] = (uint64_t)comps;

  // ---- rounds over the complete graph
  const int max_rounds = H::max_dense_rounds(n);
  sl_tile_args a{};
  a.n = n; a.dim = dim; a.sq = sq; a.mr = mr; a.alpha = p.alpha; a.core = core;
  a.vec_rows = (dim % 4 == 0 && reinterpret_cast<uintptr_t>(x) % 16 == 0) ? 1 : 0;
  a.color    = s.color.data();
  a.row_best = s.row_best.data();
  const int64_t side = (n + kT - 1) / kT;
  const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(side * side, (int64_t)res.num_cus * kWgPerCu));
  while (comps > 1) {
    if ((int)st[4] >= max_rounds)
      CUVS_FAIL("single linkage: %lld components are left after %d rounds over the complete graph", (long long)comps, max_rounds);
    const std::string round_name = "sl_dense_round_" + std::to_string(st[4]);
    profile_begin(res, round_name.c_str());
    begin_round(res, s);
    profile_begin(res, "sl_tile_kernel");
    hipLaunchKernelGGL(sl_tile_kernel, dim3(grid), dim3(kThreads), 0, res.stream, x, a);
    profile_end(res, "sl_tile_kernel");
    HIP_TRY(hipGetLastError());
    const uint32_t hooked = finish_round(res, s, n);
    profile_end(res, round_name.c_str());
    st[4] += 1;
    st[5] += (uint64_t)(side * side);
    if (hooked == 0) CUVS_FAIL("single linkage: a round over the complete graph joined none of the %lld components", (long long)comps);
    comps -= hooked;
  }

  // ---- the slots in ascending (bits(w), min, max): a stable sort by the pair, then a stable sort by the weight. The slot of
  // the last root is empty and sorts behind the n - 1 edges.
  profile_begin(res, "sl_sort");
  dev_buf<unsigned long long> pair2(res, (size_t)n);
  dev_buf<uint32_t> w2(res, (size_t)n);
  with_temp(res, temp, [&](void* t, size_t& b) {
    return hipcub::DeviceRadixSort::SortPairs(t, b, s.mst_pair.data(), pair2.data(), s.mst_w.data(), w2.data(), (int)n, 0, 64, res.stream);
  });
  with_temp(res, temp, [&](void* t, size_t& b) {
    return hipcub::DeviceRadixSort::SortPairs(t, b, w2.data(), s.mst_w.data(), pair2.data(), s.mst_pair.data(), (int)n, 0, 32, res.stream);
  });
  HIP_TRY(hipGetLastError());
  profile_end(res, "sl_sort");
  const std::vector<unsigned long long> pairs = to_host(res, s.mst_pair.data(), (size_t)n - 1);
  const std::vector<uint32_t> bits           = to_host(res, s.mst_w.data(), (size_t)n - 1);
  sl_tree tree;
  tree.src.resize((size_t)n - 1); tree.dst.resize((size_t)n - 1); tree.w.resize((size_t)n - 1);
  for (size_t e = 0; e + 1 < (size_t)n; ++e) {
    CUVS_EXPECTS(pairs[e] != kNoKey, "single linkage: the tree has fewer than n - 1 edges");
    tree.src[e] = (int64_t)(pairs[e] >> 32);
    tree.dst[e] = (int64_t)(pairs[e] & 0xffffffffull);
    memcpy(&tree.w[e], &bits[e], sizeof(float));
  }
  return tree;
}

struct sl_dendrogram {
  std::vector<int64_t> children, size;
  std::vector<float> delta;
};

// (profile: the stream is idle here, so the two events are apart by the host's time in the union-find)
sl_dendrogram dendrogram_of(resources& res, const sl_tree& t)
{
  const size_t m = t.src.size();
  sl_dendrogram d;
  d.children.resize(2 * m); d.size.resize(m); d.delta.resize(m);
  profile_begin(res, "sl_dendrogram");
  H::build_dendrogram<int64_t>(t.src.data(), t.dst.data(), t.w.data(), (int64_t)m, d.children.data(), d.delta.data(), d.size.data());
  profile_end(res, "sl_dendrogram");
  return d;
}

// host int64 values into a device index tensor of either type
void upload_index(resources& res, DLManagedTensor* out, int bytes, const std::vector<int64_t>& v)
{
  if (out == nullptr || v.empty()) return;
  void* dst = dl_data(out->dl_tensor);
  if (bytes == 8) {
    copy_async(res, dst, v.data(), v.size() * sizeof(int64_t));
    sync(res);
  } else {
    std::vector<int32_t> narrow(v.begin(), v.end());
    copy_async(res, dst, narrow.data(), narrow.size() * sizeof(int32_t));
    sync(res);
  }
}

void upload_f32(resources& res, DLManagedTensor* out, const std::vector<float>& v)
{
  if (out == nullptr || v.empty()) return;
  copy_async(res, dl_data(out->dl_tensor), v.data(), v.size() * sizeof(float));
  sync(res);
}

template <typename IdxT>
std::vector<int64_t> download_index(resources& res, const DLManagedTensor* t, size_t count)
{
  const std::vector<IdxT> h = to_host(res, static_cast<const IdxT*>(dl_data(t->dl_tensor)), count);
  return std::vector<int64_t>(h.begin(), h.end());
}

// flat labels of the cut into n_clusters (the reference's extract_flattened_clusters)
void flat_labels(resources& res, const std::vector<int64_t>& children, int64_t n, int64_t n_clusters, DLManagedTensor* labels, int bytes)
{
  void* out = dl_data(labels->dl_tensor);
  profile_begin(res, "sl_labels");
  if (n_clusters == 1) {
    HIP_TRY(hipMemsetAsync(out, 0, (size_t)n * bytes, res.stream));
    profile_end(res, "sl_labels");
    sync(res);
    return;
  }
  const int64_t n_slots = 2 * (n - 1);
  const std::vector<int64_t> roots = H::label_roots(children.data(), n, n_clusters);
  dev_buf<int64_t> children_d(res, (size_t)n_slots), roots_d(res, roots.size());
  dev_buf<int> levels(res, (size_t)n_slots + 1), tmp(res, (size_t)n_slots + 1);  // nodes 0 .. 2 n - 2
  copy_async(res, children_d.data(), children.data(), children_d.bytes());
  copy_async(res, roots_d.data(), roots.data(), roots_d.bytes());
  HIP_TRY(hipMemsetAsync(tmp.data(), 0xff, tmp.bytes(), res.stream));
  HIP_TRY(hipMemsetAsync(levels.data(), 0, levels.bytes(), res.stream));
  SL_LAUNCH(sl_levels_kernel, n_slots, children_d.data(), n_slots, levels.data());
  SL_LAUNCH(sl_label_roots_kernel, n_clusters, roots_d.data(), n_clusters, tmp.data());
  const int cut_level = (int)((n - 1) - (n_clusters - 1));
  SL_LAUNCH(sl_inherit_kernel, n_slots, children_d.data(), levels.data(), n, tmp.data(), cut_level, n_slots);
  if (bytes == 8) SL_LAUNCH(sl_write_labels_kernel<int64_t>, n, tmp.data(), n, static_cast<int64_t*>(out));
  else            SL_LAUNCH(sl_write_labels_kernel<int32_t>, n, tmp.data(), n, static_cast<int32_t*>(out));
  profile_end(res, "sl_labels");
  sync(res);  // (the host vectors behind the copies go away)
}

}  // namespace
}  // namespace cuvs_amd

using namespace cuvs_amd;

extern "C" {

cuvsError_t cuvsAmdLinkageParamsCreate(cuvsAmdLinkageParams_t* params)
{
  return (cuvsError_t)translate_exceptions([=] {
    CUVS_EXPECTS(params != nullptr, "params is null");
    *params = new cuvsAmdLinkageParams{CUVS_AMD_LINKAGE_SPACE_DISTANCE, 15, CUVS_AMD_LINKAGE_KNN_GRAPH, 5, 1.0f, nullptr};
  });
}

cuvsError_t cuvsAmdLinkageParamsDestroy(cuvsAmdLinkageParams_t params)
{
  return (cuvsError_t)translate_exceptions([=] { delete params; });
}

cuvsError_t cuvsAmdSingleLinkage(cuvsResources_t res_h, DLManagedTensor* X, DLManagedTensor* dendrogram, DLManagedTensor* labels,
                                 cuvsDistanceType metric, int64_t n_clusters, cuvsAmdLinkage linkage_kind, int c)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& res = *as_res(res_h);
    H::check_metric((int)metric);
    H::check_linkage((int)linkage_kind);
    int64_t n = 0, dim = 0;
    H::check_x(desc_of(X), &n, &dim);
    int bytes = 0;
    H::check_index(desc_of(dendrogram), n - 1, 2, "dendrogram", true, &bytes);
    H::check_index(desc_of(labels), n, 0, "labels", true, &bytes);
    H::check_n_clusters(n_clusters, n);
    const sl_params p{(int)metric, H::kDistance, (int)linkage_kind, c, 0, 1.0f, nullptr};
    const sl_tree tree    = linkage(res_h, res, X, n, dim, p, nullptr);
    const sl_dendrogram d = dendrogram_of(res, tree);
    upload_index(res, dendrogram, bytes, d.children);
    flat_labels(res, d.children, n, n_clusters, labels, bytes);
  });
}

cuvsError_t cuvsAmdBuildLinkage(cuvsResources_t res_h, DLManagedTensor* X, cuvsAmdLinkageParams_t params, cuvsDistanceType metric,
                                DLManagedTensor* mst_src, DLManagedTensor* mst_dst, DLManagedTensor* mst_weights,
                                DLManagedTensor* dendrogram, DLManagedTensor* out_distances, DLManagedTensor* out_sizes,
                                DLManagedTensor* core_dists)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& res = *as_res(res_h);
    if (params == nullptr) H::refuse("params must not be NULL");
    H::check_metric((int)metric);
    H::check_space((int)params->space);
    const bool mr = params->space == CUVS_AMD_LINKAGE_SPACE_MUTUAL_REACHABILITY;
    if (!mr) H::check_linkage((int)params->linkage);
    int64_t n = 0, dim = 0;
    H::check_x(desc_of(X), &n, &dim);
    int bytes = 0;
    H::check_index(desc_of(mst_src), n - 1, 0, "mst_src", false, &bytes);
    H::check_index(desc_of(mst_dst), n - 1, 0, "mst_dst", false, &bytes);
    H::check_index(desc_of(dendrogram), n - 1, 2, "dendrogram", false, &bytes);
    H::check_index(desc_of(out_sizes), n - 1, 0, "out_sizes", false, &bytes);
    H::check_f32_vector(desc_of(mst_weights), n - 1, "mst_weights", false);
    H::check_f32_vector(desc_of(out_distances), n - 1, "out_distances", false);
    if (mr) {
      H::check_f32_vector(desc_of(core_dists), n, "core_dists", true);
      H::check_min_samples(params->min_samples, n);
    } else if (core_dists != nullptr) {
      H::refuse("core_dists must be NULL in distance space");
    }
    const sl_params p{(int)metric, (int)params->space, (int)params->linkage, params->c, params->min_samples, params->alpha,
                      params->all_neighbors_params};
    const sl_tree tree =
      linkage(res_h, res, X, n, dim, p, mr ? static_cast<float*>(dl_data(core_dists->dl_tensor)) : nullptr);
    upload_index(res, mst_src, bytes, tree.src);
    upload_index(res, mst_dst, bytes, tree.dst);
    upload_f32(res, mst_weights, tree.w);
    if (dendrogram != nullptr || out_distances != nullptr || out_sizes != nullptr) {
      const sl_dendrogram d = dendrogram_of(res, tree);
      upload_index(res, dendrogram, bytes, d.children);
      upload_f32(res, out_distances, d.delta);
      upload_index(res, out_sizes, bytes, d.size);
    }
  });
}

cuvsError_t cuvsAmdBuildDendrogram(cuvsResources_t res_h, DLManagedTensor* rows, DLManagedTensor* cols, DLManagedTensor* data,
                                   DLManagedTensor* children, DLManagedTensor* out_delta, DLManagedTensor* out_size)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& res = *as_res(res_h);
    const eps_host::tensor_desc r = desc_of(rows);
    if (!r.present || r.ndim != 1 || r.shape[0] < 1) H::refuse("rows must be a vector of n - 1 >= 1 edges");
    const int64_t m = r.shape[0];
    if (m + 1 >= (int64_t(1) << 30)) H::refuse("single linkage needs n < 2^30 rows; got %lld", (long long)(m + 1));
    int bytes = 0;
    H::check_index(r, m, 0, "rows", true, &bytes);
    H::check_index(desc_of(cols), m, 0, "cols", true, &bytes);
    H::check_f32_vector(desc_of(data), m, "data", true);
    H::check_index(desc_of(children), m, 2, "children", true, &bytes);
    H::check_f32_vector(desc_of(out_delta), m, "out_delta", true);
    H::check_index(desc_of(out_size), m, 0, "out_size", true, &bytes);
    sl_tree tree;
    tree.src = bytes == 8 ? download_index<int64_t>(res, rows, (size_t)m) : download_index<int32_t>(res, rows, (size_t)m);
    tree.dst = bytes == 8 ? download_index<int64_t>(res, cols, (size_t)m) : download_index<int32_t>(res, cols, (size_t)m);
    tree.w   = to_host(res, static_cast<const float*>(dl_data(data->dl_tensor)), (size_t)m);
    const sl_dendrogram d = dendrogram_of(res, tree);
    upload_index(res, children, bytes, d.children);
    upload_f32(res, out_delta, d.delta);
    upload_index(res, out_size, bytes, d.size);
  });
}

cuvsError_t cuvsAmdSingleLinkageLastStats(uint64_t out[6])
{
  return (cuvsError_t)translate_exceptions([=] {
    CUVS_EXPECTS(out != nullptr, "out is null");
    for (int i = 0; i < 6; ++i) out[i] = g_sl_stats[i];
  });
}

}  // extern "C"
