// Masked L2 nearest neighbour and cross-component nearest neighbours (include/cuvs_amd/masked_nn.h; semantics of the reference's
// cpp/src/distance/masked_nn.cuh, detail/masked_nn.cuh, detail/compress_to_bits.cuh and
// cpp/src/sparse/neighbors/cross_component_nn.cuh). DESIGN 3.1zb.
//
// The rows of y are cut into G contiguous groups; adj[m, G] says which groups a row of x may look at. The work is the 128 x 128
// pair tiles of the distance GEMM (distance_tile.hpp: k-major LDS staging with the XOR swizzle, double buffered, fp32 MFMA,
// one k-ordered chain per pair), but only the tiles that can hold an admissible pair are computed:
//   1. mnn_compress_kernel reads adj once (coalesced, transposed through LDS, one ballot per 64 rows) into, per 128-row tile rt,
//      tile_any[rt] (G bits: the OR over the tile's rows, empty groups left out) and row_mask[rt][g] (128 bits, one per row of the tile).
//      cross_component_nn's mask is "every group but my own": it is never built. The tile kernel takes row_group[m] instead
//      (template parameter SRC), and tile_any shrinks to tile_mono[rt], the tile's colour if it has only one.
//   2. mnn_mark_kernel flags the (rt, ct) pairs whose columns meet a group set in tile_any; a device prefix sum and
//      mnn_compact_kernel list them rt-major. The count stays on the device.
//   3. mnn_tile_kernel runs on a fixed grid; a workgroup takes pairs blockIdx.x + i * gridDim.x below the count. The epilogue
//      keeps the tile in registers: d = max(fmaf(-2, acc, xn + yn), 0), elements whose (row, group(column)) bit is clear are
//      dropped, the rest compete as keys bits(d) << 32 | column: a lane's four columns, the 16 lanes of a row (DPP), the two
//      waves of a row (LDS atomic), then one 64-bit atomicMin per row and tile into keys[m].
// Keys are unique per (row, column) and min is order-free: results are bit-identical from run to run and for every grid.
#include "common.hpp"
#include "dl_desc.hpp"
#include "distance_tile.hpp"
#include "masked_nn_host.hpp"
#include "ops.hpp"

#include <cuvs_amd/masked_nn.h>

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cfloat>

namespace cuvs_amd {
namespace {

namespace H = mnn_host;

constexpr int kThreads = 256;
constexpr int kStage   = 16;  // group ends of a column tile staged in LDS; a tile that spans more searches group_idxs itself
constexpr unsigned long long kNoKey = H::kNoKey;
constexpr uint32_t kMaxBits = 0x7f7fffffu;  // FLT_MAX
enum : int { kAdj = 0, kRowGroup = 1 };     // where the mask comes from

// first index in [lo, hi) whose entry is greater than v (hi if none)
template <typename T>
__device__ inline int64_t upper_bound(const T* a, int64_t lo, int64_t hi, int64_t v)
{
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if ((int64_t)a[mid] <= v) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// ---------------------------------------------------------------- 1: the mask as bits
// grid (row tiles, ceil(G / 64)): adj[128 rows][64 groups] goes through LDS so that a lane holds a row and a ballot a group
__global__ __launch_bounds__(kThreads) void mnn_compress_kernel(const uint8_t* __restrict__ adj, int64_t m, int64_t G,
                                                                 const int64_t* __restrict__ ends,
                                                                 unsigned long long* __restrict__ row_mask,
                                                                 unsigned long long* __restrict__ tile_any)
{
  __shared__ uint8_t s[BM][68];  // 17 words a row: the column reads below are conflict-free
  __shared__ unsigned long long s_any;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t rt = blockIdx.x, row0 = rt * BM, g0 = (int64_t)blockIdx.y * 64;
  for (int e = tid; e < BM * 64; e += kThreads) {
    const int r = e >> 6, c = e & 63;
    const int64_t row = row0 + r, g = g0 + c;
    s[r][c] = (row < m && g < G) ? (uint8_t)(adj[row * G + g] != 0) : (uint8_t)0;
  }
  if (tid == 0) s_any = 0ull;
  __syncthreads();
  unsigned long long any = 0ull;
  for (int t = 0; t < 16; ++t) {
    const int c = wave * 16 + t;
    const unsigned long long lo = __ballot(s[lane][c] != 0), hi = __ballot(s[64 + lane][c] != 0);
    if (lane == 0 && g0 + c < G) {
      row_mask[(rt * G + g0 + c) * 2]     = lo;
      row_mask[(rt * G + g0 + c) * 2 + 1] = hi;
    }
    // (an empty group has no column to switch on: it keeps no tile alive)
    const bool holds = g0 + c < G && ends[g0 + c] > (g0 + c > 0 ? ends[g0 + c - 1] : 0);
    any |= (unsigned long long)(holds && (lo | hi) != 0ull) << c;
  }
  if (lane == 0) atomicOr(&s_any, any);
  __syncthreads();
  if (tid == 0) tile_any[rt * gridDim.y + blockIdx.y] = s_any;
}

// the colour of a row tile whose rows all have one colour, else -1
__global__ __launch_bounds__(kThreads) void mnn_mono_kernel(const int32_t* __restrict__ row_group, int64_t m, int64_t row_tiles,
                                                             int32_t* __restrict__ tile_mono)
{
  const int64_t rt = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (rt >= row_tiles) return;
  const int64_t r0 = rt * BM, r1 = min(r0 + BM, m);
  const int32_t c = row_group[r0];
  bool mono = true;
  for (int64_t r = r0 + 1; r < r1; ++r) mono = mono && row_group[r] == c;
  tile_mono[rt] = mono ? c : -1;
}

// the groups of a column tile's first and last column; glo == G: the tile lies past the last group, ghi is clamped to G - 1
__global__ __launch_bounds__(kThreads) void mnn_coltile_kernel(const int64_t* __restrict__ ends, int64_t G, int64_t n, int64_t col_tiles,
                                                                uint32_t* __restrict__ ct_glo, uint32_t* __restrict__ ct_ghi)
{
  const int64_t ct = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (ct >= col_tiles) return;
  const int64_t c0 = ct * BN, c1 = min(c0 + BN, n) - 1;
  ct_glo[ct] = (uint32_t)upper_bound(ends, 0, G, c0);
  ct_ghi[ct] = (uint32_t)min(upper_bound(ends, 0, G, c1), G - 1);
}

// ---------------------------------------------------------------- 2: the live pairs
template <int SRC>
__global__ __launch_bounds__(kThreads) void mnn_mark_kernel(int64_t rt0, int64_t slab_tiles, int64_t col_tiles, int64_t G,
                                                             const uint32_t* __restrict__ ct_glo, const uint32_t* __restrict__ ct_ghi,
                                                             const unsigned long long* __restrict__ tile_any,
                                                             const int32_t* __restrict__ tile_mono, uint32_t* __restrict__ flags)
{
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= slab_tiles * col_tiles) return;
  const int64_t rt = rt0 + p / col_tiles, ct = p % col_tiles;
  const int64_t glo = ct_glo[ct], ghi = ct_ghi[ct];
  bool live = false;
  if (glo < G) {
    if constexpr (SRC == kAdj) {
      const int64_t words = (G + 63) / 64;
      for (int64_t w = glo >> 6; w <= (ghi >> 6) && !live; ++w) {
        unsigned long long bits = tile_any[rt * words + w];
        if (w == (glo >> 6)) bits &= ~0ull << (glo & 63);
        if (w == (ghi >> 6)) bits &= ~0ull >> (63 - (ghi & 63));
        live = bits != 0ull;
      }
    } else {
      const int32_t c = tile_mono[rt];
      live = !(c >= 0 && glo == c && ghi == c);
    }
  }
  flags[p] = live ? 1u : 0u;
}

__global__ __launch_bounds__(kThreads) void mnn_compact_kernel(const uint32_t* __restrict__ flags, const uint32_t* __restrict__ offs,
                                                                int64_t pairs_total, uint32_t* __restrict__ pairs,
                                                                uint32_t* __restrict__ count, unsigned long long* __restrict__ live_total)
{
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= pairs_total) return;
  if (flags[p]) pairs[offs[p]] = (uint32_t)p;
  if (p == pairs_total - 1) {
    *count = offs[p] + flags[p];
    *live_total += offs[p] + flags[p];  // (one thread of one kernel at a time on the stream)
  }
}

// ---------------------------------------------------------------- 3: the tiles
struct mnn_args {
  const float *x, *y, *xn, *yn;
  int64_t m, n, dim, G;
  const int64_t* ends;                  // [G] group ends
  const uint4* row_mask;                // kAdj: [row tiles, G] 128 bits
  const int32_t* row_group;             // kRowGroup: [m]
  const uint32_t* col_ids;              // kRowGroup: [n] the id a column competes with, or null (its position)
  const uint32_t *ct_glo, *ct_ghi;      // [column tiles]
  const uint32_t *pairs, *count;        // the slab's live pairs (rt-major) and their number
  int64_t rt0, col_tiles;
  unsigned long long* keys;             // [m]
};

// min over the 16 lanes of a DPP row; every lane ends with it
__device__ inline unsigned long long row16_min(unsigned long long v)
{
#define MNN_STEP(CTRL)                                                                                                  \
  {                                                                                                                     \
    const uint32_t lo = (uint32_t)__builtin_amdgcn_mov_dpp((int)(uint32_t)v, CTRL, 0xf, 0xf, true);                     \
    const uint32_t hi = (uint32_t)__builtin_amdgcn_mov_dpp((int)(uint32_t)(v >> 32), CTRL, 0xf, 0xf, true);             \
    const unsigned long long o = ((unsigned long long)hi << 32) | lo;                                                   \
    v = o < v ? o : v;                                                                                                  \
  }
  MNN_STEP(0xB1)   // quad_perm [1, 0, 3, 2]
  MNN_STEP(0x4E)   // quad_perm [2, 3, 0, 1]
  MNN_STEP(0x141)  // row_half_mirror
  MNN_STEP(0x140)  // row_mirror
#undef MNN_STEP
  return v;
}

template <int SRC, bool VEC>
__global__ __launch_bounds__(kThreads, H::kWgPerCu) void mnn_tile_kernel(mnn_args a)
{
  __shared__ __attribute__((aligned(16))) float As[2][BK * LDT];
  __shared__ __attribute__((aligned(16))) float Bs[2][BK * LDT];
  __shared__ __attribute__((aligned(16))) float s_qn[BM], s_xn[BN];
  __shared__ unsigned long long s_key[BM];
  __shared__ uint32_t s_ge[kStage];
  __shared__ int32_t s_rg[BM];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, l15 = lane & 15, lg = lane >> 4;
  // staging and fragment addresses: those of dist_tile_kernel (distance.hip)
  const int sr0 = tid >> 2, sc = tid & 3;
  const int st0 = (4 * sc) * LDT + (sr0 ^ (sc << 3));
  const int st1 = (4 * sc) * LDT + ((sr0 + 64) ^ (sc << 3));
  const int ra_[2] = {lg * LDT + wm * 64 + l15, lg * LDT + wm * 64 + (l15 ^ 8)};
  const int rb_[2] = {lg * LDT + wn * 64 + l15, lg * LDT + wn * 64 + (l15 ^ 8)};
  const int nkt = (int)((a.dim + BK - 1) / BK);  // the last k-tile is zero-filled past dim: fma(0, 0, acc) = acc
  const uint32_t count = *a.count;
  if (tid < BM) s_key[tid] = kNoKey;

  for (uint32_t p = blockIdx.x; p < count; p += gridDim.x) {
    const uint32_t pr = a.pairs[p];
    const int64_t rt = a.rt0 + pr / a.col_tiles, ct = pr % a.col_tiles;
    const int64_t row0 = rt * BM, col0 = ct * BN;
    const int64_t glo = a.ct_glo[ct], ghi = a.ct_ghi[ct];
    const bool staged = ghi - glo < kStage;
    __syncthreads();  // the previous pair's keys are flushed, its norms and ends read
    if (tid < BM) {
      const int64_t row = row0 + tid;
      s_qn[tid] = a.xn[min(row, a.m - 1)];
      if constexpr (SRC == kRowGroup) s_rg[tid] = row < a.m ? a.row_group[row] : -1;
    } else {
      s_xn[tid - BM] = a.yn[min(col0 + tid - BM, a.n - 1)];
    }
    if (staged && tid <= ghi - glo) s_ge[tid] = (uint32_t)a.ends[glo + tid];

    // rows past m / n are clamped to the last row; their results are dropped below
    const int64_t xa0 = min(row0 + sr0, a.m - 1), xa1 = min(row0 + sr0 + 64, a.m - 1);
    const int64_t yb0 = min(col0 + sr0, a.n - 1), yb1 = min(col0 + sr0 + 64, a.n - 1);
    float ga0[4], ga1[4], gb0[4], gb1[4];
    auto fetch = [&](int64_t k0) {
      load4<float, VEC>(a.x, xa0, a.m, a.dim, k0 + sc * 4, a.dim, ga0);
      load4<float, VEC>(a.x, xa1, a.m, a.dim, k0 + sc * 4, a.dim, ga1);
      load4<float, VEC>(a.y, yb0, a.n, a.dim, k0 + sc * 4, a.dim, gb0);
      load4<float, VEC>(a.y, yb1, a.n, a.dim, k0 + sc * 4, a.dim, gb1);
    };
    auto stash = [&](int buf) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        As[buf][st0 + e * LDT] = ga0[e]; As[buf][st1 + e * LDT] = ga1[e];
        Bs[buf][st0 + e * LDT] = gb0[e]; Bs[buf][st1 + e * LDT] = gb1[e];
      }
    };
    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (nkt > 0) {
      fetch(0);
      stash(0);
    }
    __syncthreads();

    for (int kt = 0; kt < nkt; ++kt) {
      const int buf = kt & 1;
      if (kt + 1 < nkt) fetch((int64_t)(kt + 1) * BK);
      const float* A = As[buf];
      const float* B = Bs[buf];
      float fa[2][4], fb[2][4];
      auto read_frags = [&](const int c, float (&va)[4], float (&vb)[4]) {
#pragma unroll
        for (int i = 0; i < 4; ++i) va[i] = A[ra_[c & 1] + (4 * c) * LDT + ((i ^ (c >> 1)) * 16)];
#pragma unroll
        for (int j = 0; j < 4; ++j) vb[j] = B[rb_[c & 1] + (4 * c) * LDT + ((j ^ (c >> 1)) * 16)];
      };
      read_frags(0, fa[0], fb[0]);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        if (c < 3) read_frags(c + 1, fa[(c + 1) & 1], fb[(c + 1) & 1]);
        __builtin_amdgcn_sched_group_barrier(0x100, 8, 0);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[c & 1][i], fb[c & 1][j], acc[i][j], 0, 0, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 16, 0);
      }
      if (kt + 1 < nkt) stash(buf ^ 1);
      __syncthreads();
    }

    // ---- epilogue: C layout col = lane & 15, row = (lane >> 4) * 4 + e. The lane's four columns: group, mask, id, norm
    int32_t gj[4];
    uint32_t cid[4], mw[4][2];
    float xnv[4];
    bool lane_any = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int cl      = wn * 64 + j * 16 + l15;
      const int64_t col = col0 + cl;
      xnv[j] = s_xn[cl];
      gj[j]  = -1;
      cid[j] = (uint32_t)col;
      mw[j][0] = mw[j][1] = 0u;
      if (col < a.n) {
        const int64_t g = staged ? glo + upper_bound(s_ge, 0, ghi - glo + 1, col) : upper_bound(a.ends, glo, ghi + 1, col);
        if (g < a.G) {
          gj[j] = (int32_t)g;
          if constexpr (SRC == kAdj) {
            const uint4 mk = a.row_mask[rt * a.G + g];
            mw[j][0] = wm ? mk.z : mk.x;  // rows wm * 64 .. + 31
            mw[j][1] = wm ? mk.w : mk.y;  // rows wm * 64 + 32 .. + 63
            lane_any = lane_any || (mw[j][0] | mw[j][1]) != 0u;
          } else {
            if (a.col_ids != nullptr) cid[j] = a.col_ids[col];
            lane_any = true;
          }
        }
      }
    }
    if (__any(lane_any)) {  // (wave-uniform: the DPP steps below see every lane)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const f32x4 qn4 = *reinterpret_cast<const f32x4*>(&s_qn[wm * 64 + i * 16 + lg * 4]);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int rl = wm * 64 + i * 16 + lg * 4 + e;
          unsigned long long best = kNoKey;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            bool ok;
            if constexpr (SRC == kAdj) ok = (mw[j][i >> 1] >> ((i & 1) * 16 + lg * 4 + e)) & 1u;
            else ok = gj[j] >= 0 && gj[j] != s_rg[rl];
            float v = __fmaf_rn(-2.0f, acc[i][j][e], qn4[e] + xnv[j]);
            v       = v > 0.f ? v : 0.f;
            const unsigned long long key = H::pack_key(__float_as_uint(v), cid[j]);
            best = (ok && key < best) ? key : best;
          }
          best = row16_min(best);
          if (l15 == 0 && best != kNoKey) atomicMin(&s_key[rl], best);
        }
      }
    }
    __syncthreads();
    if (tid < BM) {
      const unsigned long long k = s_key[tid];
      if (k != kNoKey) {
        if (row0 + tid < a.m) atomicMin(&a.keys[row0 + tid], k);
        s_key[tid] = kNoKey;
      }
    }
  }
}

// ---------------------------------------------------------------- init / finish
// keys from nothing (init_out) or from the caller's values. A stored square root does not give its square back, so the squared
// distance of (i, out_idx[i]) is recomputed by the tile's own arithmetic and taken when its root is the stored value.
__global__ __launch_bounds__(kThreads) void mnn_init_kernel(unsigned long long* __restrict__ keys, int64_t m, int init_out, int sq_root,
                                                             const int64_t* __restrict__ out_idx, const float* __restrict__ out_dist,
                                                             const float* __restrict__ x, const float* __restrict__ y,
                                                             const float* __restrict__ xn, const float* __restrict__ yn, int64_t n,
                                                             int64_t dim)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  if (init_out) {
    keys[i] = kNoKey;
    return;
  }
  const int64_t idx = out_idx[i];
  const float s = out_dist[i];
  float d = s;
  if (sq_root) {
    d = s * s;
    if (idx >= 0 && idx < n) {
      float acc = 0.f;
      for (int64_t t = 0; t < dim; ++t) acc = __fmaf_rn(x[i * dim + t], y[idx * dim + t], acc);
      float v = __fmaf_rn(-2.0f, acc, xn[i] + yn[idx]);
      v       = v > 0.f ? v : 0.f;
      if (sqrtf(v) == s) d = v;
    }
  }
  d = d > 0.f ? d : 0.f;
  if (!(d < FLT_MAX)) d = FLT_MAX;
  keys[i] = H::pack_key(__float_as_uint(d), (idx >= 0 && idx < n) ? (uint32_t)idx : 0xffffffffu);
}

__global__ __launch_bounds__(kThreads) void mnn_finish_kernel(const unsigned long long* __restrict__ keys, int64_t m, int sq_root,
                                                               int64_t* __restrict__ out_idx, float* __restrict__ out_dist)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const unsigned long long k = keys[i];
  const uint32_t col = (uint32_t)k, bits = (uint32_t)(k >> 32);
  const float d = __uint_as_float(bits);
  out_idx[i]    = col == 0xffffffffu ? -1 : (int64_t)col;
  out_dist[i]   = (sq_root && bits != kMaxBits) ? sqrtf(d) : d;
}

// ---------------------------------------------------------------- cross-component kernels
// counts[c] of every colour, counts[n_colors] the number of colours outside [0, n_colors)
__global__ __launch_bounds__(kThreads) void cc_count_kernel(const int32_t* __restrict__ colors, int64_t n, int64_t n_colors,
                                                             uint32_t* __restrict__ counts, uint32_t* __restrict__ ids)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t c = colors[i];
  atomicAdd(&counts[(c >= 0 && c < n_colors) ? c : n_colors], 1u);
  ids[i] = (uint32_t)i;
}

__global__ __launch_bounds__(kThreads) void cc_gather_kernel(const float* __restrict__ x, const uint32_t* __restrict__ perm, int64_t n,
                                                              int64_t dim, float* __restrict__ out)
{
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n * dim) return;
  const int64_t i = e / dim, t = e - i * dim;
  out[e] = x[(int64_t)perm[i] * dim + t];
}

// position p of the colour order is the caller's row perm[p]: its key goes to row_key[perm[p]], its weight competes for the colour
__global__ __launch_bounds__(kThreads) void cc_rows_kernel(const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ perm,
                                                            const int32_t* __restrict__ sorted_color, int64_t n, int sq_root,
                                                            unsigned long long* __restrict__ row_key, int64_t* __restrict__ row_idx,
                                                            float* __restrict__ row_dist, uint32_t* __restrict__ comp_w)
{
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const unsigned long long k = keys[p];
  const int64_t r = perm[p];
  const uint32_t j = (uint32_t)k, bits = (uint32_t)(k >> 32);
  row_key[r] = k;
  if (row_idx != nullptr) row_idx[r] = j == 0xffffffffu ? -1 : (int64_t)j;
  if (row_dist != nullptr) row_dist[r] = (sq_root && bits != kMaxBits) ? sqrtf(__uint_as_float(bits)) : __uint_as_float(bits);
  if (j != 0xffffffffu) atomicMin(&comp_w[sorted_color[p]], bits);
}

// among the rows that attain their colour's smallest weight, the smallest (i, j)
__global__ __launch_bounds__(kThreads) void cc_pair_kernel(const unsigned long long* __restrict__ row_key, const int32_t* __restrict__ colors,
                                                            int64_t n, const uint32_t* __restrict__ comp_w,
                                                            unsigned long long* __restrict__ comp_pair)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned long long k = row_key[i];
  const uint32_t j = (uint32_t)k;
  if (j == 0xffffffffu) return;
  const int32_t c = colors[i];
  if ((uint32_t)(k >> 32) == comp_w[c]) atomicMin(&comp_pair[c], ((unsigned long long)i << 32) | j);
}

__global__ __launch_bounds__(kThreads) void cc_edges_kernel(const uint32_t* __restrict__ comp_w, const unsigned long long* __restrict__ comp_pair,
                                                             int64_t n_colors, int sq_root, int64_t* __restrict__ src,
                                                             int64_t* __restrict__ dst, float* __restrict__ w)
{
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n_colors) return;
  const unsigned long long pr = comp_pair[c];
  const bool none = pr == ~0ull;
  src[c] = none ? -1 : (int64_t)(pr >> 32);
  dst[c] = none ? -1 : (int64_t)(pr & 0xffffffffull);
  const float d = __uint_as_float(comp_w[c]);
  w[c] = none ? FLT_MAX : (sq_root ? sqrtf(d) : d);
}

// ---------------------------------------------------------------- host side
#define MNN_LAUNCH(kernel, items, ...)                                                                                          \
  do {                                                                                                                          \
    if ((items) > 0) {                                                                                                          \
      hipLaunchKernelGGL(kernel, dim3(grid_blocks((items), kThreads)), dim3(kThreads), 0, res.stream, __VA_ARGS__);             \
      HIP_TRY(hipGetLastError());                                                                                               \
    }                                                                                                                           \
  } while (0)

template <typename Call>
void with_temp(resources& res, dev_buf<char>& temp, Call&& call)  // hipcub's two-step convention: size query, then the run
{
  size_t bytes = 0;
  HIP_TRY(call(static_cast<void*>(nullptr), bytes));
  if (bytes > temp.bytes()) temp = dev_buf<char>(res, bytes);
  bytes = std::max<size_t>(temp.bytes(), 1);
  HIP_TRY(call(static_cast<void*>(temp.data()), bytes));
}

thread_local uint64_t g_pairs = 0;  // (row tile, column tile) pairs of the calling thread's last call

// the live pairs go to the handle's pinned words without a wait; cuvsAmdMaskedNNLastStats synchronises and reads them
void post_live(resources& res, const unsigned long long* live)
{
  if (res.host_word == nullptr) HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&res.host_word), 64));
  HIP_TRY(hipMemcpyAsync(res.host_word + 2, live, sizeof(unsigned long long), hipMemcpyDeviceToHost, res.stream));
}

struct mnn_problem {
  const float *x, *y, *xn, *yn;
  int64_t m, n, dim, G;
  const int64_t* ends;
  const uint8_t* adj;        // kAdj
  const int32_t* row_group;  // kRowGroup
  const uint32_t* col_ids;
};

// keys[m] <- min(keys[m], the admissible pairs): compress, then per slab of row tiles mark, scan, list, run
template <int SRC>
void masked_tiles(resources& res, const mnn_problem& P, unsigned long long* keys, unsigned long long* live_total)
{
  if (P.m == 0 || P.n == 0 || P.G == 0) return;
  const H::plan pl = H::make_plan(P.m, P.n, res.num_cus);
  const int64_t words = (P.G + 63) / 64;
  dev_buf<unsigned long long> row_mask, tile_any;
  dev_buf<int32_t> tile_mono;
  if constexpr (SRC == kAdj) {
    CUVS_EXPECTS(words <= 65535, "masked_l2_nn: more than 65535 * 64 groups");
    row_mask = dev_buf<unsigned long long>(res, (size_t)(pl.row_tiles * P.G * 2));
    tile_any = dev_buf<unsigned long long>(res, (size_t)(pl.row_tiles * words));
    hipLaunchKernelGGL(mnn_compress_kernel, dim3((unsigned)pl.row_tiles, (unsigned)words), dim3(kThreads), 0, res.stream, P.adj, P.m, P.G,
                       P.ends, row_mask.data(), tile_any.data());
    HIP_TRY(hipGetLastError());
  } else {
    tile_mono = dev_buf<int32_t>(res, (size_t)pl.row_tiles);
    MNN_LAUNCH(mnn_mono_kernel, pl.row_tiles, P.row_group, P.m, pl.row_tiles, tile_mono.data());
  }
  dev_buf<uint32_t> ct_glo(res, (size_t)pl.col_tiles), ct_ghi(res, (size_t)pl.col_tiles);
  MNN_LAUNCH(mnn_coltile_kernel, pl.col_tiles, P.ends, P.G, P.n, pl.col_tiles, ct_glo.data(), ct_ghi.data());

  const int64_t slab_pairs = pl.slab_tiles * pl.col_tiles;
  dev_buf<uint32_t> flags(res, (size_t)slab_pairs), offs(res, (size_t)slab_pairs), pairs(res, (size_t)slab_pairs), count(res, 1);
  dev_buf<char> temp;
  mnn_args a{};
  a.x = P.x; a.y = P.y; a.xn = P.xn; a.yn = P.yn; a.m = P.m; a.n = P.n; a.dim = P.dim; a.G = P.G; a.ends = P.ends;
  a.row_mask = reinterpret_cast<const uint4*>(row_mask.data()); a.row_group = P.row_group; a.col_ids = P.col_ids;
  a.ct_glo = ct_glo.data(); a.ct_ghi = ct_ghi.data(); a.pairs = pairs.data(); a.count = count.data();
  a.col_tiles = pl.col_tiles; a.keys = keys;
  const bool vec = vec_ok(P.x, P.dim, P.dim) && vec_ok(P.y, P.dim, P.dim);
  for (int64_t rt0 = 0; rt0 < pl.row_tiles; rt0 += pl.slab_tiles) {
    const int64_t tiles = std::min(pl.slab_tiles, pl.row_tiles - rt0), np = tiles * pl.col_tiles;
    MNN_LAUNCH(mnn_mark_kernel<SRC>, np, rt0, tiles, pl.col_tiles, P.G, ct_glo.data(), ct_ghi.data(), tile_any.data(), tile_mono.data(),
               flags.data());
    with_temp(res, temp, [&](void* t, size_t& b) {
      return hipcub::DeviceScan::ExclusiveSum(t, b, flags.data(), offs.data(), (int)np, res.stream);
    });
    MNN_LAUNCH(mnn_compact_kernel, np, flags.data(), offs.data(), np, pairs.data(), count.data(), live_total);
    a.rt0 = rt0;
    profile_begin(res, "mnn_tile_kernel");
    if (vec) hipLaunchKernelGGL((mnn_tile_kernel<SRC, true>), dim3((unsigned)pl.grid), dim3(kThreads), 0, res.stream, a);
    else hipLaunchKernelGGL((mnn_tile_kernel<SRC, false>), dim3((unsigned)pl.grid), dim3(kThreads), 0, res.stream, a);
    profile_end(res, "mnn_tile_kernel");
    HIP_TRY(hipGetLastError());
  }
  g_pairs = (uint64_t)(pl.row_tiles * pl.col_tiles);
}

// norms the caller did not give
const float* norms_or(resources& res, const float* given, const float* rows, int64_t n, int64_t dim, dev_buf<float>& own)
{
  if (given != nullptr || n == 0) return given;
  own = dev_buf<float>(res, (size_t)n);
  row_norms<float>(res, rows, n, dim, dim, own.data(), false);
  return own.data();
}

void masked_l2_nn(resources& res, mnn_problem P, bool sq_root, bool init_out, int64_t* out_idx, float* out_dist)
{
  g_pairs = 0;
  if (P.m == 0) return;
  dev_buf<float> own_xn, own_yn;
  P.xn = norms_or(res, P.xn, P.x, P.m, P.dim, own_xn);
  P.yn = norms_or(res, P.yn, P.y, P.n, P.dim, own_yn);
  dev_buf<unsigned long long> keys(res, (size_t)P.m), live(res, 1);
  HIP_TRY(hipMemsetAsync(live.data(), 0, sizeof(unsigned long long), res.stream));
  MNN_LAUNCH(mnn_init_kernel, P.m, keys.data(), P.m, (int)init_out, (int)sq_root, out_idx, out_dist, P.x, P.y, P.xn, P.yn, P.n, P.dim);
  masked_tiles<kAdj>(res, P, keys.data(), live.data());
  MNN_LAUNCH(mnn_finish_kernel, P.m, keys.data(), P.m, (int)sq_root, out_idx, out_dist);
  post_live(res, live.data());
}

void cross_component_nn(resources& res, const float* x, int64_t n, int64_t dim, const int32_t* colors, int64_t n_colors, bool sq_root,
                        int64_t* row_idx, float* row_dist, int64_t* src, int64_t* dst, float* w)
{
  g_pairs = 0;
  // ---- colour counts; nothing is written before the colours are known to be in range
  dev_buf<uint32_t> counts(res, (size_t)n_colors + 1), ids(res, (size_t)n), perm(res, (size_t)n), comp_w(res, (size_t)n_colors);
  HIP_TRY(hipMemsetAsync(counts.data(), 0, counts.bytes(), res.stream));
  MNN_LAUNCH(cc_count_kernel, n, colors, n, n_colors, counts.data(), ids.data());
  const uint32_t bad = read_word(res, counts.data() + n_colors);
  if (bad != 0) H::refuse("colors holds %u values outside [0, %lld)", bad, (long long)n_colors);

  dev_buf<unsigned long long> comp_pair(res, (size_t)n_colors), live(res, 1);
  HIP_TRY(hipMemsetAsync(comp_w.data(), 0xff, comp_w.bytes(), res.stream));
  HIP_TRY(hipMemsetAsync(comp_pair.data(), 0xff, comp_pair.bytes(), res.stream));
  HIP_TRY(hipMemsetAsync(live.data(), 0, sizeof(unsigned long long), res.stream));
  if (n > 0) {
    // ---- rows in colour order (stable: a colour's rows keep their order), the group ends from the counts
    dev_buf<int32_t> sorted(res, (size_t)n);
    dev_buf<int64_t> ends(res, (size_t)n_colors);
    dev_buf<char> temp;
    int bits = 1;
    while ((int64_t(1) << bits) < n_colors) ++bits;
    with_temp(res, temp, [&](void* t, size_t& b) {
      return hipcub::DeviceRadixSort::SortPairs(t, b, reinterpret_cast<const uint32_t*>(colors), reinterpret_cast<uint32_t*>(sorted.data()),
                                                ids.data(), perm.data(), (int)n, 0, bits, res.stream);
    });
    with_temp(res, temp, [&](void* t, size_t& b) {
      return hipcub::DeviceScan::InclusiveSum(t, b, counts.data(), ends.data(), (int)n_colors, res.stream);
    });
    dev_buf<float> xs(res, (size_t)(n * dim)), norms(res, (size_t)n);
    MNN_LAUNCH(cc_gather_kernel, n * dim, x, perm.data(), n, dim, xs.data());
    row_norms<float>(res, xs.data(), n, dim, dim, norms.data(), false);

    dev_buf<unsigned long long> keys(res, (size_t)n), row_key(res, (size_t)n);
    MNN_LAUNCH(mnn_init_kernel, n, keys.data(), n, 1, 0, (const int64_t*)nullptr, (const float*)nullptr, (const float*)nullptr,
               (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, n, dim);
    mnn_problem P{};
    P.x = xs.data(); P.y = xs.data(); P.xn = norms.data(); P.yn = norms.data(); P.m = n; P.n = n; P.dim = dim; P.G = n_colors;
    P.ends = ends.data(); P.row_group = sorted.data(); P.col_ids = perm.data();
    masked_tiles<kRowGroup>(res, P, keys.data(), live.data());
    MNN_LAUNCH(cc_rows_kernel, n, keys.data(), perm.data(), sorted.data(), n, (int)sq_root, row_key.data(), row_idx, row_dist, comp_w.data());
    MNN_LAUNCH(cc_pair_kernel, n, row_key.data(), colors, n, comp_w.data(), comp_pair.data());
  }
  MNN_LAUNCH(cc_edges_kernel, n_colors, comp_w.data(), comp_pair.data(), n_colors, (int)sq_root, src, dst, w);
  post_live(res, live.data());
}

template <typename T>
T* ptr_of(DLManagedTensor* t) { return t ? static_cast<T*>(dl_data(t->dl_tensor)) : nullptr; }

}  // namespace
}  // namespace cuvs_amd

using namespace cuvs_amd;

extern "C" {

cuvsError_t cuvsAmdMaskedL2NN(cuvsResources_t res_h, DLManagedTensor* x, DLManagedTensor* y, DLManagedTensor* x_norm,
                              DLManagedTensor* y_norm, DLManagedTensor* adj, DLManagedTensor* group_idxs, int sq_root, int init_out,
                              DLManagedTensor* out_idx, DLManagedTensor* out_dist)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& res = *as_res(res_h);
    const H::mnn_shape s = H::check_masked_nn(desc_of(x), desc_of(y), desc_of(x_norm), desc_of(y_norm), desc_of(adj), desc_of(group_idxs),
                                              desc_of(out_idx), desc_of(out_dist));
    mnn_problem P{};
    P.x = ptr_of<const float>(x); P.y = ptr_of<const float>(y); P.xn = ptr_of<const float>(x_norm); P.yn = ptr_of<const float>(y_norm);
    P.m = s.m; P.n = s.n; P.dim = s.dim; P.G = s.groups;
    P.ends = ptr_of<const int64_t>(group_idxs); P.adj = ptr_of<const uint8_t>(adj);
    masked_l2_nn(res, P, sq_root != 0, init_out != 0, ptr_of<int64_t>(out_idx), ptr_of<float>(out_dist));
  });
}

cuvsError_t cuvsAmdCrossComponentNN(cuvsResources_t res_h, DLManagedTensor* x, DLManagedTensor* colors, int64_t n_components, int sq_root,
                                    DLManagedTensor* row_nn_idx, DLManagedTensor* row_nn_dist, DLManagedTensor* edge_src,
                                    DLManagedTensor* edge_dst, DLManagedTensor* edge_weight)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& res = *as_res(res_h);
    int64_t n = 0, dim = 0;
    H::check_cross_component(desc_of(x), desc_of(colors), n_components, desc_of(row_nn_idx), desc_of(row_nn_dist), desc_of(edge_src),
                             desc_of(edge_dst), desc_of(edge_weight), &n, &dim);
    cross_component_nn(res, ptr_of<const float>(x), n, dim, ptr_of<const int32_t>(colors), n_components, sq_root != 0,
                       ptr_of<int64_t>(row_nn_idx), ptr_of<float>(row_nn_dist), ptr_of<int64_t>(edge_src), ptr_of<int64_t>(edge_dst),
                       ptr_of<float>(edge_weight));
  });
}

cuvsError_t cuvsAmdMaskedNNLastStats(cuvsResources_t res_h, uint64_t out[2])
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& res = *as_res(res_h);
    CUVS_EXPECTS(out != nullptr, "out is null");
    sync(res);
    out[0] = g_pairs;
    out[1] = 0;
    if (res.host_word != nullptr) memcpy(&out[1], res.host_word + 2, sizeof(uint64_t));
  });
}

}  // extern "C"
