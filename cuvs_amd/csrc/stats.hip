// cuvs::stats: silhouette score and trustworthiness (include/cuvs_amd/stats.h; semantics of the reference's
// cpp/src/stats/detail/{silhouette_score,batched/silhouette_score,trustworthiness_score}.cuh). DESIGN 3.1y.
//
// Both scores are "every row against every row, exact, reduced on the fly": the pair tile of eps_neighbors.hip (DESIGN 3.1t:
// 256 threads, 128 x 128 pairs, K chunks of 16 staged k-major in LDS, 8 x 8 accumulators, the fp32 chain on the vector pipe)
// with two new epilogues. The staging is a copy of 3.1t's with a row indirection; eps_neighbors.hip is untouched.
//
// Silhouette: the rows are sorted by label (stable counting sort on the device), so that the columns of a label are a run of
// positions. The host cuts [0, n) into segments, each inside one column tile and one label (stats_host.hpp); a tile reduces the
// columns of each of its segments in fp64 in a fixed order (a thread's 8 columns, then the 16 lanes of a row) and writes one
// partial per (row, segment): no atomics. sil_finish_kernel adds a row's partials of a label in segment order and forms a, b, s.
// The order of every sum depends on n, the labels and the tile size only.
//
// Ranks: per row the k thresholds v(i, neighbors[i][q]) are computed by the same chain and sorted with their ids
// (rank_prep_kernel). A workgroup keeps the sorted thresholds of its 128 rows in LDS and sweeps a run of column tiles: a pair
// is screened against its row's largest threshold (a register); one that passes finds its position by binary search and does
// one LDS integer atomicAdd on bucket[row][position]. Buckets are integers, so combining them over column runs in any order is
// deterministic; rank_finish_kernel's prefix sum over a row's buckets gives its k ranks.
#include "common.hpp"
#include "dl_desc.hpp"
#include "ops.hpp"
#include "stats_host.hpp"

#include <cuvs_amd/stats.h>

#include <algorithm>
#include <climits>
#include <vector>

namespace cuvs_amd {
namespace {

namespace H = stats_host;

constexpr int kT       = H::kTile;
constexpr int kKB      = 16;  // K chunk
constexpr int kThreads = 256;
constexpr int kWgPerCu = 2;   // persistent workgroups per CU: the tile kernels hold ~220 VGPRs (the fp64 epilogue, the search), two waves fit a SIMD

enum : int { kSq = 0, kL1 = 1, kDot = 2 };           // H::chain_t
enum : int { kPostNone = 0, kPostSqrt = 1, kPostCosine = 2 };  // H::post_t

typedef float f2 __attribute__((ext_vector_type(2)));
typedef float f4 __attribute__((ext_vector_type(4)));

thread_local uint64_t g_stats[4] = {0, 0, 0, 0};

// eight consecutive elements k .. k + 7 of one row; zero past `dim` and for a row outside the matrix.
// `vec`: rows are 16-byte aligned (dim a multiple of 4, the base aligned).
__device__ inline void st_load8(const float* __restrict__ base, int64_t row, bool row_ok, int64_t dim, int64_t k, bool vec, float out[8])
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

// The pair tile of 3.1t over rows of one matrix: thread (ty, tx) of the 16 x 16 grid ends with the chains of tile rows
// {64 h + 4 ty + c} against tile columns {16 j + tx}, acc[i][j >> 1].{x, y}. `xrow` / `yrow` are the matrix rows this thread
// stages at LDS position tid % 128 of the two operands (the column operand sits at the permuted position of 3.1t).
// Zero padding past dim leaves every chain unchanged: fma(0, 0, acc) and acc + |0| return acc.
template <int MODE>
__device__ __forceinline__ void pair_tile(const float* __restrict__ x, int64_t dim, bool vec, int64_t xrow, bool x_ok, int64_t yrow,
                                          bool y_ok, float (*xs)[kT], float (*ys)[kT], f2 (&acc)[8][4])
{
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tx = lane & 15, ty = wave * 4 + (lane >> 4);
  const int p = tid & (kT - 1), kh = tid >> 7;
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f2)(0.f);
  float px[8], py[8];
  if (dim > 0) {
    st_load8(x, xrow, x_ok, dim, (int64_t)kh * 8, vec, px);
    st_load8(x, yrow, y_ok, dim, (int64_t)kh * 8, vec, py);
  }
  for (int64_t k0 = 0; k0 < dim; k0 += kKB) {
    __syncthreads();  // the previous chunk has been read
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      xs[kh * 8 + c][p] = px[c];
      ys[kh * 8 + c][p] = py[c];
    }
    __syncthreads();
    if (k0 + kKB < dim) {  // the next chunk is in flight while this one is computed
      st_load8(x, xrow, x_ok, dim, k0 + kKB + kh * 8, vec, px);
      st_load8(x, yrow, y_ok, dim, k0 + kKB + kh * 8, vec, py);
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
          if constexpr (MODE == kSq) {
            const f2 d = (f2)(av[i]) - bv[j];
            acc[i][j]  = __builtin_elementwise_fma(d, d, acc[i][j]);
          } else if constexpr (MODE == kL1) {
            const f2 d = (f2)(av[i]) - bv[j];
            acc[i][j]  = acc[i][j] + __builtin_elementwise_abs(d);
          } else {
            acc[i][j] = __builtin_elementwise_fma((f2)(av[i]), bv[j], acc[i][j]);
          }
        }
    }
  }
}

// tile column c (0 .. 127) is staged at LDS position p with c = ycol_of(p)
__device__ inline int ycol_of(int p) { return (((p >> 6) << 2) | (p & 3)) * 16 + ((p & 63) >> 2); }

// ---------------------------------------------------------------- silhouette: labels
// counts[c] of every label, counts[n_labels] the number of labels outside [0, n_labels)
__global__ __launch_bounds__(kThreads) void sil_count_kernel(const int32_t* __restrict__ labels, int64_t n, int64_t n_labels,
                                                             int32_t* __restrict__ counts)
{
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int64_t c = labels[i];
    atomicAdd(&counts[(c >= 0 && c < n_labels) ? c : n_labels], 1);
  }
}

// Stable counting sort of the row ids by label, in two kernels. sil_chunk_kernel (a workgroup per 256 rows): the number of
// earlier rows of the chunk with the row's label, and, for the last row of a label in the chunk, a flag. sil_place_kernel (one
// workgroup walking the chunks in order): a row's position is its label's cursor plus that number; the last row of a label in
// the chunk moves the cursor past itself. cursor[c] starts at the first position of label c; the cursors sit in LDS where
// n_labels allows (kLdsLabels), else they are read and written through the L2 by integer atomics.
// perm[position] = row id, sorted[position] = label.
constexpr int kLdsLabels = 4096;

__global__ __launch_bounds__(kThreads) void sil_chunk_kernel(const int32_t* __restrict__ labels, int64_t n, uint16_t* __restrict__ place)
{
  __shared__ int32_t lab[kThreads];
  const int tid   = threadIdx.x;
  const int64_t i = (int64_t)blockIdx.x * kThreads + tid;
  const int32_t c = i < n ? labels[i] : -1;
  lab[tid] = c;
  __syncthreads();
  int before = 0;
  bool last  = true;
  for (int j = 0; j < kThreads; ++j) {
    const bool same = lab[j] == c;
    before += (same && j < tid) ? 1 : 0;
    last = last && !(same && j > tid);
  }
  if (i < n) place[i] = (uint16_t)(before | (last ? 0x8000 : 0));
}

template <bool LDS>
__global__ __launch_bounds__(kThreads) void sil_place_kernel(const int32_t* __restrict__ labels, const uint16_t* __restrict__ place,
                                                             int64_t n, int64_t n_labels, int32_t* cursor, int32_t* __restrict__ perm,
                                                             int32_t* __restrict__ sorted)
{
  __shared__ int32_t cur[LDS ? kLdsLabels : 1];
  const int tid = threadIdx.x;
  if constexpr (LDS) {
    for (int64_t c = tid; c < n_labels; c += kThreads) cur[c] = cursor[c];
  }
  __syncthreads();
  int32_t c  = tid < n ? labels[tid] : -1;
  uint16_t w = tid < n ? place[tid] : 0;
  for (int64_t base = 0; base < n; base += kThreads) {
    const int64_t i = base + tid, nx = i + kThreads;
    const int32_t c_next  = nx < n ? labels[nx] : -1;  // the next chunk is in flight
    const uint16_t w_next = nx < n ? place[nx] : 0;
    int32_t pos = 0;
    if (c >= 0) {
      pos         = (LDS ? cur[c] : atomicAdd(&cursor[c], 0)) + (w & 0x7fff);
      perm[pos]   = (int32_t)i;
      sorted[pos] = c;
    }
    __syncthreads();  // every cursor of the chunk has been read
    if (c >= 0 && (w & 0x8000)) {
      if constexpr (LDS) cur[c] = pos + 1;
      else atomicExch(&cursor[c], pos + 1);
    }
    __syncthreads();
    c = c_next;
    w = w_next;
  }
}

// sqrtf of the fma chain of squares of every row (cosine)
__global__ __launch_bounds__(kThreads) void sil_norm_kernel(const float* __restrict__ x, int64_t n, int64_t dim, float* __restrict__ out)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float* r = x + i * dim;
  float acc = 0.f;
  for (int64_t t = 0; t < dim; ++t) acc = fmaf(r[t], r[t], acc);
  out[i] = sqrtf(acc);
}

// ---------------------------------------------------------------- silhouette: tiles
struct sil_args {
  const float* x;
  const int32_t* perm;        // [n] row id of a position
  const float* rnorm;         // [n] by row id (cosine) or null
  int64_t n, dim;
  int64_t row_begin, rows;    // the slab: positions [row_begin, row_begin + rows)
  int vec, post;
  const int32_t* tile_first;  // [col_tiles + 1]
  const int32_t* seg_lo;
  const int32_t* seg_hi;
  double* partial;            // [segments, rows]
};

template <int MODE>
__global__ __launch_bounds__(kThreads) void sil_tile_kernel(sil_args a)
{
  __shared__ __attribute__((aligned(16))) float xs[kKB][kT];
  __shared__ __attribute__((aligned(16))) float ys[kKB][kT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tx = lane & 15, ty = wave * 4 + (lane >> 4);
  const int p = tid & (kT - 1), ycol = ycol_of(p);
  const int64_t row_end = a.row_begin + a.rows;
  const int64_t row_tiles = (a.rows + kT - 1) / kT, col_tiles = (a.n + kT - 1) / kT;
  const int64_t tiles = row_tiles * col_tiles;

  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t rt = tile / col_tiles, ct = tile - rt * col_tiles;
    const int64_t row0 = a.row_begin + rt * kT, col0 = ct * kT;
    const bool x_ok = row0 + p < row_end, y_ok = col0 + ycol < a.n;
    const int64_t xrow = x_ok ? a.perm[row0 + p] : 0, yrow = y_ok ? a.perm[col0 + ycol] : 0;
    f2 acc[8][4];
    pair_tile<MODE>(a.x, a.dim, a.vec != 0, xrow, x_ok, yrow, y_ok, xs, ys, acc);

    // ---- the distances of the thread's 8 x 8 pairs
    float d[8][8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) d[i][j] = (j & 1) ? acc[i][j >> 1].y : acc[i][j >> 1].x;
    if (a.post == kPostSqrt) {
#pragma unroll
      for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) d[i][j] = sqrtf(d[i][j]);
    } else if (a.post == kPostCosine) {
      float nr[8], nc[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int64_t r = row0 + (i >> 2) * 64 + ty * 4 + (i & 3);
        nr[i] = r < row_end ? a.rnorm[a.perm[r]] : 1.f;
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int64_t c = col0 + j * 16 + tx;
        nc[j] = c < a.n ? a.rnorm[a.perm[c]] : 1.f;
      }
#pragma unroll
      for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) d[i][j] = 1.0f - d[i][j] / (nr[i] * nc[j]);
    }

    // ---- one fp64 partial per (row, segment): the thread's columns j ascending, then the row's 16 lanes by a butterfly
    const int s0 = a.tile_first[ct], s1 = a.tile_first[ct + 1];
    for (int s = s0; s < s1; ++s) {
      const int64_t lo = a.seg_lo[s], hi = a.seg_hi[s];
      // a segment that is the whole tile, off the diagonal: no pair is left out
      const bool whole = lo == col0 && hi == col0 + kT && (row0 + kT <= col0 || col0 + kT <= row0);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int64_t r = row0 + (i >> 2) * 64 + ty * 4 + (i & 3);
        double sum = 0.0;
        if (whole) {
#pragma unroll
          for (int j = 0; j < 8; ++j) sum += (double)d[i][j];
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const int64_t c = col0 + j * 16 + tx;
            sum += (c >= lo && c < hi && c != r) ? (double)d[i][j] : 0.0;
          }
        }
        sum += __shfl_xor(sum, 8, 64);
        sum += __shfl_xor(sum, 4, 64);
        sum += __shfl_xor(sum, 2, 64);
        sum += __shfl_xor(sum, 1, 64);
        if (tx == 0 && r < row_end) a.partial[(int64_t)s * a.rows + (r - a.row_begin)] = sum;
      }
    }
  }
}

// a thread per slab row: S of a label is the sum of the row's partials over the label's segments in segment order
__global__ __launch_bounds__(kThreads) void sil_finish_kernel(const double* __restrict__ partial, int64_t row_begin, int64_t rows,
                                                              int64_t n_segments, const int32_t* __restrict__ seg_label,
                                                              const int32_t* __restrict__ counts, const int32_t* __restrict__ perm,
                                                              const int32_t* __restrict__ sorted, double* __restrict__ s64,
                                                              float* __restrict__ scores)
{
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  const int32_t own = sorted[row_begin + r];
  double s_own = 0.0, b = INFINITY, run = 0.0;
  int32_t cur = seg_label[0];
  for (int64_t s = 0; s <= n_segments; ++s) {
    const int32_t c = s < n_segments ? seg_label[s] : -1;
    if (c != cur) {
      if (cur == own) s_own = run;
      else b = fmin(b, run / (double)counts[cur]);  // (fmin: a NaN mean is passed over, as by the twin's np.fmin)
      cur = c;
      run = 0.0;
    }
    if (s < n_segments) run += partial[s * rows + r];
  }
  const double v = H::sil_sample(s_own, (double)counts[own], b);
  const int64_t i = perm[row_begin + r];
  s64[i] = v;
  if (scores != nullptr) scores[i] = (float)v;
}

// ---------------------------------------------------------------- ranks
// flags |= 1 for an id equal to its row, |= 2 for an id outside [0, n)
__global__ __launch_bounds__(kThreads) void rank_check_kernel(const int64_t* __restrict__ nbr, int64_t n, int k, unsigned* flags)
{
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n * k) return;
  const int64_t j = nbr[e];
  if (j < 0 || j >= n) atomicOr(flags, 2u);
  else if (j == e / k) atomicOr(flags, 1u);
}

// a wave per slab row, lane q: the threshold v(i, neighbors[i][q]) by the chain, then its place among the row's k
// (threshold, id) pairs; slot[place] = q
__global__ __launch_bounds__(kThreads) void rank_prep_kernel(const float* __restrict__ x, int64_t dim, const int64_t* __restrict__ nbr, int k,
                                                             int64_t row_begin, int64_t rows, float* __restrict__ thr,
                                                             int32_t* __restrict__ ids, uint8_t* __restrict__ slot)
{
  const int lane = threadIdx.x & 63;
  const int64_t r = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;  // wave-uniform
  if (r >= rows) return;
  const int64_t i = row_begin + r;
  float t    = INFINITY;
  int32_t id = INT_MAX;
  if (lane < k) {
    const int64_t j = nbr[i * k + lane];
    const float* xi = x + i * dim;
    const float* xj = x + j * dim;
    float acc = 0.f;
    for (int64_t u = 0; u < dim; ++u) {
      const float d = xi[u] - xj[u];
      acc = fmaf(d, d, acc);
    }
    t  = acc;
    id = (int32_t)j;
  }
  int place = 0;
  for (int q = 0; q < k; ++q) {
    const float t2   = __shfl(t, q, 64);
    const int32_t i2 = __shfl(id, q, 64);
    place += (t2 < t || (t2 == t && (i2 < id || (i2 == id && q < lane)))) ? 1 : 0;
  }
  if (lane < k) {
    thr[r * k + place]  = t;
    ids[r * k + place]  = id;
    slot[r * k + place] = (uint8_t)lane;
  }
}

struct rank_args {
  const float* x;
  int64_t n, dim;
  int vec, k;
  int64_t row_begin, rows;
  const float* thr;           // [rows, k] ascending by (threshold, id)
  const int32_t* ids;
  uint32_t* bucket;           // [rows, k], zeroed by the caller
  unsigned long long* passed; // pairs past the screen
  int64_t col_tiles, run_tiles, runs;  // a unit is a row tile and a run of `run_tiles` column tiles
};

__global__ __launch_bounds__(kThreads) void rank_tile_kernel(rank_args a)
{
  __shared__ __attribute__((aligned(16))) float xs[kKB][kT];
  __shared__ __attribute__((aligned(16))) float ys[kKB][kT];
  extern __shared__ __attribute__((aligned(16))) unsigned char dyn[];
  float* sthr   = reinterpret_cast<float*>(dyn);             // [kT][k]
  int32_t* sid  = reinterpret_cast<int32_t*>(sthr + kT * a.k);
  uint32_t* sb  = reinterpret_cast<uint32_t*>(sid + kT * a.k);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tx = lane & 15, ty = wave * 4 + (lane >> 4);
  const int p = tid & (kT - 1), ycol = ycol_of(p);
  const int k = a.k;
  const int64_t row_end = a.row_begin + a.rows;
  const int64_t row_tiles = (a.rows + kT - 1) / kT, units = row_tiles * a.runs;
  unsigned long long passed = 0;

  for (int64_t unit = blockIdx.x; unit < units; unit += gridDim.x) {
    const int64_t rt = unit / a.runs, run = unit - rt * a.runs;
    const int64_t row0 = a.row_begin + rt * kT;
    __syncthreads();  // the previous unit's buckets have been flushed
    for (int e = tid; e < kT * k; e += kThreads) {
      const int64_t r = row0 + e / k;
      const bool ok   = r < row_end;
      sthr[e] = ok ? a.thr[(rt * kT) * k + e] : -1.f;  // (no chain is <= -1: a row outside the slab counts nothing)
      sid[e]  = ok ? a.ids[(rt * kT) * k + e] : 0;
      sb[e]   = 0u;
    }
    __syncthreads();
    float top[8];  // the row's largest threshold
#pragma unroll
    for (int i = 0; i < 8; ++i) top[i] = sthr[((i >> 2) * 64 + ty * 4 + (i & 3)) * k + k - 1];

    const int64_t ct_end = (run + 1) * a.run_tiles < a.col_tiles ? (run + 1) * a.run_tiles : a.col_tiles;
    for (int64_t ct = run * a.run_tiles; ct < ct_end; ++ct) {
      const int64_t col0 = ct * kT;
      const bool x_ok = row0 + p < row_end, y_ok = col0 + ycol < a.n;
      f2 acc[8][4];
      pair_tile<kSq>(a.x, a.dim, a.vec != 0, row0 + p, x_ok, col0 + ycol, y_ok, xs, ys, acc);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int rl    = (i >> 2) * 64 + ty * 4 + (i & 3);
        const int64_t r = row0 + rl;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float v   = (j & 1) ? acc[i][j >> 1].y : acc[i][j >> 1].x;
          const int64_t c = col0 + j * 16 + tx;
          if (c < a.n && c != r && v <= top[i]) {
            ++passed;
            // position = thresholds (t, id) <= (v, c): the pair counts for every later threshold
            int lo = 0, hi = k;
            while (lo < hi) {
              const int mid = (lo + hi) >> 1;
              const float t = sthr[rl * k + mid];
              if (t < v || (t == v && (int64_t)sid[rl * k + mid] <= c)) lo = mid + 1;
              else hi = mid;
            }
            if (lo < k) atomicAdd(&sb[rl * k + lo], 1u);
          }
        }
      }
    }
    __syncthreads();
    for (int e = tid; e < kT * k; e += kThreads)
      if (sb[e] != 0u) atomicAdd(&a.bucket[(rt * kT) * k + e], sb[e]);
  }
  if (passed != 0) atomicAdd(a.passed, passed);
}

// a thread per slab row: ranks from the prefix sum of the buckets, written at the caller's columns; the penalty
__global__ __launch_bounds__(kThreads) void rank_finish_kernel(const uint32_t* __restrict__ bucket, const uint8_t* __restrict__ slot, int k,
                                                               int64_t row_begin, int64_t rows, int32_t* __restrict__ ranks,
                                                               unsigned long long* penalty)
{
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  unsigned long long pen = 0;
  uint32_t run = 0;
  for (int s = 0; s < k; ++s) {
    run += bucket[r * k + s];
    const int64_t rank = 1 + (int64_t)run;
    if (ranks != nullptr) ranks[(row_begin + r) * k + slot[r * k + s]] = (int32_t)rank;
    if (rank > k) pen += (unsigned long long)(rank - k);
  }
  if (pen != 0) atomicAdd(penalty, pen);
}

// the k nearest other rows from a (k + 1)-nearest list: the entry whose id is the row's own is dropped if present, else the last
__global__ __launch_bounds__(kThreads) void trust_drop_self_kernel(const int64_t* __restrict__ knn, int64_t n, int k, int64_t* __restrict__ out)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int w = 0;
  for (int q = 0; q < k + 1 && w < k; ++q) {
    const int64_t j = knn[i * (k + 1) + q];
    if (j != i) out[i * k + w++] = j;
  }
}

// ---------------------------------------------------------------- host side
int rows_vec(const float* x, int64_t dim) { return (dim % 4 == 0 && reinterpret_cast<uintptr_t>(x) % 16 == 0) ? 1 : 0; }

unsigned persistent_grid(const resources& res, int64_t units)
{
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>(units, (int64_t)res.num_cus * kWgPerCu));
}

template <typename T>
dev_buf<T> upload(resources& res, const std::vector<T>& h)
{
  dev_buf<T> d(res, h.size());
  copy_async(res, d.data(), h.data(), h.size() * sizeof(T));
  return d;
}

double silhouette(resources& res, const float* x, int64_t n, int64_t dim, const int32_t* labels, int64_t n_labels,
                  H::metric_plan plan, int64_t batch_rows, float* scores)
{
  uint64_t* st = g_stats;
  st[0] = st[1] = st[2] = st[3] = 0;
  // ---- label counts; nothing is written before the labels are known to be in range
  dev_buf<int32_t> counts(res, (size_t)n_labels + 1);
  HIP_TRY(hipMemsetAsync(counts.data(), 0, counts.bytes(), res.stream));
  hipLaunchKernelGGL(sil_count_kernel, dim3((unsigned)std::min<int64_t>((n + kThreads - 1) / kThreads, (int64_t)res.num_cus * 8)),
                     dim3(kThreads), 0, res.stream, labels, n, n_labels, counts.data());
  HIP_TRY(hipGetLastError());
  const std::vector<int32_t> h_counts = to_host(res, counts.data(), (size_t)n_labels + 1);
  H::check_label_counts(h_counts[(size_t)n_labels], n_labels);
  const H::segments seg = H::build_segments(h_counts.data(), n_labels, n);
  const int64_t n_seg   = seg.count();

  // ---- rows sorted by label
  dev_buf<int32_t> cursor = upload(res, seg.label_first), perm(res, (size_t)n), sorted(res, (size_t)n);
  {
    dev_buf<uint16_t> place(res, (size_t)n);
    hipLaunchKernelGGL(sil_chunk_kernel, dim3(grid_blocks(n, kThreads)), dim3(kThreads), 0, res.stream, labels, n, place.data());
    if (n_labels <= kLdsLabels)
      hipLaunchKernelGGL(sil_place_kernel<true>, dim3(1), dim3(kThreads), 0, res.stream, labels, place.data(), n, n_labels, cursor.data(),
                         perm.data(), sorted.data());
    else
      hipLaunchKernelGGL(sil_place_kernel<false>, dim3(1), dim3(kThreads), 0, res.stream, labels, place.data(), n, n_labels, cursor.data(),
                         perm.data(), sorted.data());
    HIP_TRY(hipGetLastError());
  }
  dev_buf<int32_t> seg_lo = upload(res, seg.lo), seg_hi = upload(res, seg.hi), seg_label = upload(res, seg.label),
                   tile_first = upload(res, seg.tile_first);
  dev_buf<float> rnorm;
  if (plan.post == H::post_t::cosine) {
    rnorm = dev_buf<float>(res, (size_t)n);
    hipLaunchKernelGGL(sil_norm_kernel, dim3(grid_blocks(n, kThreads)), dim3(kThreads), 0, res.stream, x, n, dim, rnorm.data());
    HIP_TRY(hipGetLastError());
  }

  // ---- slabs of positions
  const int64_t slab = H::slab_rows(n, H::silhouette_row_bytes(n_seg), (int64_t)res.workspace_limit, batch_rows, res.tune.stats_slab_rows);
  dev_buf<double> partial(res, (size_t)(slab * n_seg)), s64(res, (size_t)n);
  const int64_t col_tiles = (n + kT - 1) / kT;
  for (int64_t r0 = 0; r0 < n; r0 += slab) {
    const int64_t rows = std::min(slab, n - r0);
    sil_args a{};
    a.x = x; a.perm = perm.data(); a.rnorm = rnorm.data(); a.n = n; a.dim = dim;
    a.row_begin = r0; a.rows = rows; a.vec = rows_vec(x, dim); a.post = (int)plan.post;
    a.tile_first = tile_first.data(); a.seg_lo = seg_lo.data(); a.seg_hi = seg_hi.data(); a.partial = partial.data();
    const int64_t row_tiles = (rows + kT - 1) / kT;
    const dim3 grid(persistent_grid(res, row_tiles * col_tiles));
    profile_begin(res, "sil_tile_kernel");
    if (plan.chain == H::chain_t::sq) hipLaunchKernelGGL(sil_tile_kernel<kSq>, grid, dim3(kThreads), 0, res.stream, a);
    else if (plan.chain == H::chain_t::l1) hipLaunchKernelGGL(sil_tile_kernel<kL1>, grid, dim3(kThreads), 0, res.stream, a);
    else hipLaunchKernelGGL(sil_tile_kernel<kDot>, grid, dim3(kThreads), 0, res.stream, a);
    profile_end(res, "sil_tile_kernel");
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(sil_finish_kernel, dim3(grid_blocks(rows, kThreads)), dim3(kThreads), 0, res.stream, partial.data(), r0, rows,
                       n_seg, seg_label.data(), counts.data(), perm.data(), sorted.data(), s64.data(), scores);
    HIP_TRY(hipGetLastError());
    st[0] += (uint64_t)(row_tiles * col_tiles);
    st[1] += 1;
    st[2] += (uint64_t)(row_tiles * seg.straddling);
  }
  const std::vector<double> h_s = to_host(res, s64.data(), (size_t)n);  // (the uploads above are read before this returns)
  return H::sil_mean(h_s.data(), n);
}

// ranks [n, k] (or null) and the penalty sum; the neighbour ids have not been checked yet
uint64_t neighbor_ranks(resources& res, const float* x, int64_t n, int64_t dim, const int64_t* nbr, int k, int32_t* ranks)
{
  uint64_t* st = g_stats;
  st[0] = st[1] = st[2] = st[3] = 0;
  if (n == 0) return 0;
  dev_buf<unsigned long long> words(res, 3);  // id flags, penalty, pairs past the screen
  HIP_TRY(hipMemsetAsync(words.data(), 0, words.bytes(), res.stream));
  hipLaunchKernelGGL(rank_check_kernel, dim3(grid_blocks(n * k, kThreads)), dim3(kThreads), 0, res.stream, nbr, n, k,
                     reinterpret_cast<unsigned*>(words.data()));
  HIP_TRY(hipGetLastError());
  H::check_neighbor_flags((unsigned)to_host(res, words.data(), 1)[0], n);

  const int64_t slab = H::slab_rows(n, H::ranks_row_bytes(k), (int64_t)res.workspace_limit, 0, res.tune.stats_slab_rows);
  dev_buf<float> thr(res, (size_t)(slab * k));
  dev_buf<int32_t> ids(res, (size_t)(slab * k));
  dev_buf<uint8_t> slot(res, (size_t)(slab * k));
  dev_buf<uint32_t> bucket(res, (size_t)(slab * k));
  const size_t lds = (size_t)kT * k * 12;
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(rank_tile_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const int64_t col_tiles = (n + kT - 1) / kT;
  for (int64_t r0 = 0; r0 < n; r0 += slab) {
    const int64_t rows = std::min(slab, n - r0), row_tiles = (rows + kT - 1) / kT;
    hipLaunchKernelGGL(rank_prep_kernel, dim3(grid_blocks(rows * 64, kThreads)), dim3(kThreads), 0, res.stream, x, dim, nbr, k, r0, rows,
                       thr.data(), ids.data(), slot.data());
    HIP_TRY(hipMemsetAsync(bucket.data(), 0, (size_t)(rows * k) * sizeof(uint32_t), res.stream));
    // enough units to fill the device four times over: a row tile's columns are cut into runs
    const int64_t want = (int64_t)res.num_cus * kWgPerCu * 4;
    const int64_t runs_want = std::min<int64_t>(col_tiles, std::max<int64_t>(1, (want + row_tiles - 1) / row_tiles));
    rank_args a{};
    a.x = x; a.n = n; a.dim = dim; a.vec = rows_vec(x, dim); a.k = k; a.row_begin = r0; a.rows = rows;
    a.thr = thr.data(); a.ids = ids.data(); a.bucket = bucket.data(); a.passed = words.data() + 2;
    a.col_tiles = col_tiles;
    a.run_tiles = (col_tiles + runs_want - 1) / runs_want;
    a.runs      = (col_tiles + a.run_tiles - 1) / a.run_tiles;
    profile_begin(res, "rank_tile_kernel");
    hipLaunchKernelGGL(rank_tile_kernel, dim3(persistent_grid(res, row_tiles * a.runs)), dim3(kThreads), lds, res.stream, a);
    profile_end(res, "rank_tile_kernel");
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(rank_finish_kernel, dim3(grid_blocks(rows, kThreads)), dim3(kThreads), 0, res.stream, bucket.data(), slot.data(), k,
                       r0, rows, ranks, words.data() + 1);
    HIP_TRY(hipGetLastError());
    st[0] += (uint64_t)(row_tiles * col_tiles);
    st[1] += 1;
  }
  const std::vector<unsigned long long> h = to_host(res, words.data(), 3);
  st[2] = h[2];
  return h[1];
}

const float* f32_of(DLManagedTensor* t) { return static_cast<const float*>(dl_data(t->dl_tensor)); }

}  // namespace
}  // namespace cuvs_amd

using namespace cuvs_amd;

extern "C" {

cuvsError_t cuvsAmdSilhouetteScore(cuvsResources_t res_h, DLManagedTensor* X, DLManagedTensor* labels, int64_t n_labels,
                                   cuvsDistanceType metric, int64_t batch_rows, DLManagedTensor* scores, double* mean)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& res = *as_res(res_h);
    const H::metric_plan plan = H::check_silhouette_metric((int)metric);
    int64_t n = 0, dim = 0;
    H::check_matrix(desc_of(X), "X", &n, &dim);
    H::check_vector(desc_of(labels), "labels", n, false, false);
    H::check_vector(desc_of(scores), "scores", n, true, true);
    H::check_n_labels(n_labels, n);
    if (mean == nullptr) H::refuse("mean must not be NULL");
    const double m = silhouette(res, f32_of(X), n, dim, static_cast<const int32_t*>(dl_data(labels->dl_tensor)), n_labels, plan,
                                batch_rows, scores ? static_cast<float*>(dl_data(scores->dl_tensor)) : nullptr);
    *mean = m;
  });
}

cuvsError_t cuvsAmdNeighborRanks(cuvsResources_t res_h, DLManagedTensor* X, DLManagedTensor* neighbors, DLManagedTensor* ranks,
                                 uint64_t* penalty_sum)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& res = *as_res(res_h);
    int64_t n = 0, dim = 0;
    H::check_matrix(desc_of(X), "X", &n, &dim);
    const int k = H::check_neighbors(desc_of(neighbors), n);
    H::check_ranks(desc_of(ranks), n, k);
    if (penalty_sum == nullptr) H::refuse("penalty_sum must not be NULL");
    const uint64_t t = neighbor_ranks(res, f32_of(X), n, dim, static_cast<const int64_t*>(dl_data(neighbors->dl_tensor)), k,
                                      ranks ? static_cast<int32_t*>(dl_data(ranks->dl_tensor)) : nullptr);
    *penalty_sum = t;
  });
}

cuvsError_t cuvsAmdTrustworthinessScore(cuvsResources_t res_h, DLManagedTensor* X, DLManagedTensor* X_embedded, int64_t n_neighbors,
                                        cuvsDistanceType metric, double* score)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& res = *as_res(res_h);
    H::check_trustworthiness_metric((int)metric);
    int64_t n = 0, dim = 0, ne = 0, dim_e = 0;
    H::check_matrix(desc_of(X), "X", &n, &dim);
    H::check_matrix(desc_of(X_embedded), "X_embedded", &ne, &dim_e);
    if (ne != n) H::refuse("X_embedded has %lld rows, X has %lld", (long long)ne, (long long)n);
    H::check_n_neighbors(n_neighbors, n);
    if (score == nullptr) H::refuse("score must not be NULL");
    const int k = (int)n_neighbors;
    // (a) the k + 1 nearest rows of the embedding under the brute-force search's exactness contract
    const float* e = f32_of(X_embedded);
    dev_buf<float> norms(res, (size_t)n), knn_d(res, (size_t)(n * (k + 1)));
    dev_buf<int64_t> knn_i(res, (size_t)(n * (k + 1))), nbr(res, (size_t)(n * k));
    row_norms<float>(res, e, n, dim_e, dim_e, norms.data(), false);
    bf_search_view(res, M_L2Expanded, e, n, dim_e, norms.data(), e, n, k + 1, knn_i.data(), knn_d.data(), nullptr);
    hipLaunchKernelGGL(trust_drop_self_kernel, dim3(grid_blocks(n, kThreads)), dim3(kThreads), 0, res.stream, knn_i.data(), n, k, nbr.data());
    HIP_TRY(hipGetLastError());
    // (b) their ranks among the rows of X, (c) the score
    const uint64_t t = neighbor_ranks(res, f32_of(X), n, dim, nbr.data(), k, nullptr);
    *score = H::trustworthiness(n, k, t);
  });
}

cuvsError_t cuvsAmdStatsLastStats(uint64_t out[4])
{
  return (cuvsError_t)translate_exceptions([=] {
    CUVS_EXPECTS(out != nullptr, "out is null");
    for (int i = 0; i < 4; ++i) out[i] = g_stats[i];
  });
}

}  // extern "C"
