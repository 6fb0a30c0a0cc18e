// Epsilon neighbourhood by brute force (include/cuvs_amd/eps_neighbors.h; semantics of the reference's
// cpp/src/neighbors/detail/epsilon_neighborhood.cuh and of the CSR protocols of ball_cover::eps_nn). DESIGN 3.1t.
//
// Contract: pair (i, j) is inside when acc <= eps, acc the fp32 chain acc = fmaf(d, d, acc) from 0, d = x[i][t] - y[j][t],
// t ascending, one accumulator per pair. The matrix cores do not compute this chain, so the pair tile runs on the VALU.
//
// eps_tile_kernel: a 256-thread workgroup owns a 128 x 128 block of pairs, 8 x 8 accumulators per thread, K chunks of 16 of both
// operands staged k-major in LDS and read with ds_read_b128. Thread (ty, tx) of the 16 x 16 grid owns rows
// {64 h + 4 ty + c} and columns {16 j + tx}: the ballot of one (i, j) comparison over a wave is then, for each of the wave's
// four row groups, the 16 membership bits of the columns 16 j .. 16 j + 15 in order. The y operand sits in LDS at the
// permuted position 64 (j / 4) + 4 tx + j % 4, so that the thread's eight columns are still two 16-byte reads.
// Epilogues: dense (adjacency bytes as 16-byte stores, degrees by integer atomics) and count (bit mask + per-tile counts in
// workspace, no atomics). eps_fill_kernel writes a row's ids in ascending order from the mask.
#include "common.hpp"
#include "dl_desc.hpp"
#include "eps_neighbors_host.hpp"

#include <cuvs_amd/eps_neighbors.h>

#include <algorithm>
#include <type_traits>
#include <vector>

namespace cuvs_amd {
namespace {

namespace H = eps_host;

constexpr int kT       = H::kTile;  // pairs tile edge
constexpr int kKB      = 16;        // K chunk
constexpr int kThreads = 256;
constexpr int kWgPerCu = 3;         // persistent workgroups per CU: the tile kernel holds ~160 VGPRs, three waves fit a SIMD (18 KiB LDS each)

typedef float f2 __attribute__((ext_vector_type(2)));
typedef float f4 __attribute__((ext_vector_type(4)));

thread_local uint64_t g_eps_stats[4] = {0, 0, 0, 0};

__device__ inline float eps_f32(float v) { return v; }
__device__ inline float eps_f32(__half v) { return __half2float(v); }

// eight consecutive elements k .. k + 7 of one row, widened to fp32; zero past `dim` and for a row outside the matrix.
// `vec`: rows are 16-byte aligned and dim is a multiple of the elements of 16 bytes.
template <typename T>
__device__ inline void eps_load8(const T* __restrict__ base, int64_t row, bool row_ok, int64_t dim, int64_t k, bool vec, float out[8])
{
  const T* p = base + row * dim + k;
  if (vec && row_ok && k + 8 <= dim) {
    if constexpr (sizeof(T) == 4) {
      const f4 v0 = *reinterpret_cast<const f4*>(p), v1 = *reinterpret_cast<const f4*>(p + 4);
      out[0] = v0.x; out[1] = v0.y; out[2] = v0.z; out[3] = v0.w;
      out[4] = v1.x; out[5] = v1.y; out[6] = v1.z; out[7] = v1.w;
    } else {
      union { uint4 u; __half h[8]; } v;
      v.u = *reinterpret_cast<const uint4*>(p);
#pragma unroll
      for (int c = 0; c < 8; ++c) out[c] = __half2float(v.h[c]);
    }
    return;
  }
#pragma unroll
  for (int c = 0; c < 8; ++c) out[c] = (row_ok && k + c < dim) ? eps_f32(p[c]) : 0.f;
}

enum : int { kEpiDense = 0, kEpiCount = 1 };

struct eps_tile_args {
  int64_t rows, n, dim;        // rows of x in this slab, rows of y, columns
  float eps;
  int vec_rows;                // eps_load8's `vec`
  // dense
  uint8_t* adj;                // [rows, n] or null
  void* vd;                    // [rows] degrees (VdT) or null; zeroed by the caller
  unsigned long long* total;   // edges, zeroed by the caller
  int vec_adj;                 // adj rows are 16-byte aligned
  // count
  uint32_t* mask;              // [rows, mask_stride] bit j % 32 of word j / 32 = pair (row, j)
  int64_t mask_stride;         // words per row: 4 per column tile
  uint8_t* counts;             // [rows, col_tiles]
};

template <typename T, int EPI, typename VdT>
__global__ __launch_bounds__(kThreads) void eps_tile_kernel(const T* __restrict__ x, const T* __restrict__ y, eps_tile_args a)
{
  __shared__ __attribute__((aligned(16))) float xs[kKB][kT];
  __shared__ __attribute__((aligned(16))) float ys[kKB][kT];
  __shared__ __attribute__((aligned(16))) unsigned long long sball[4][64];  // [wave][8 i + j]: the ballot of comparison (i, j)

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tx = lane & 15, ty = wave * 4 + (lane >> 4);
  // staging: LDS position p of both operands, K half kh
  const int p = tid & (kT - 1), kh = tid >> 7;
  const int ycol_of_p = (((p >> 6) << 2) | (p & 3)) * 16 + ((p & 63) >> 2);

  const int64_t row_tiles = (a.rows + kT - 1) / kT, col_tiles = (a.n + kT - 1) / kT;
  const int64_t tiles = row_tiles * col_tiles;
  unsigned long long my_edges = 0;

  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t rt = tile / col_tiles, ct = tile - rt * col_tiles;
    const int64_t row0 = rt * kT, col0 = ct * kT;

    f2 acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = (f2)(0.f);

    const int64_t xrow = row0 + p, yrow = col0 + ycol_of_p;
    const bool x_ok = xrow < a.rows, y_ok = yrow < a.n;
    float px[8], py[8];
    if (a.dim > 0) {
      eps_load8(x, xrow, x_ok, a.dim, (int64_t)kh * 8, a.vec_rows != 0, px);
      eps_load8(y, yrow, y_ok, a.dim, (int64_t)kh * 8, a.vec_rows != 0, py);
    }
    for (int64_t k0 = 0; k0 < a.dim; k0 += kKB) {
      __syncthreads();  // the previous chunk has been read
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        xs[kh * 8 + c][p] = px[c];
        ys[kh * 8 + c][p] = py[c];
      }
      __syncthreads();
      if (k0 + kKB < a.dim) {  // the next chunk is in flight while this one is computed
        eps_load8(x, xrow, x_ok, a.dim, k0 + kKB + kh * 8, a.vec_rows != 0, px);
        eps_load8(y, yrow, y_ok, a.dim, k0 + kKB + kh * 8, a.vec_rows != 0, py);
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
            const f2 d = (f2)(av[i]) - bv[j];                      // v_pk_add_f32 (one fp32 subtraction per pair)
            acc[i][j]  = __builtin_elementwise_fma(d, d, acc[i][j]);  // v_pk_fma_f32 (one chain per pair)
          }
      }
    }

    // ---- membership: the ballot of comparison (i, j), a wave-uniform 64-bit value, goes to LDS through lane 0. A tile
    // inside the matrix needs no masks; at the matrix edge the pairs of rows and columns outside it are masked off.
    __syncthreads();  // the previous tile's epilogue has read sball (dim == 0 has no other barrier)
    auto membership = [&](auto inside_tag) {
      constexpr bool kInside = decltype(inside_tag)::value;
      bool ok_r[8], ok_c[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) ok_r[i] = kInside || row0 + (i >> 2) * 64 + ty * 4 + (i & 3) < a.rows;
#pragma unroll
      for (int j = 0; j < 8; ++j) ok_c[j] = kInside || col0 + j * 16 + tx < a.n;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        unsigned long long ball[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float v = (j & 1) ? acc[i][j >> 1].y : acc[i][j >> 1].x;
          ball[j] = __ballot(ok_r[i] && ok_c[j] && v <= a.eps);  // false for NaN
        }
        if (lane == 0) {
#pragma unroll
          for (int j = 0; j < 8; ++j) sball[wave][i * 8 + j] = ball[j];
        }
      }
    };
    if (row0 + kT <= a.rows && col0 + kT <= a.n) membership(std::true_type{});
    else membership(std::false_type{});
    __syncthreads();
    // the 16 bits of tile row r, columns 16 j .. 16 j + 15
    const unsigned short* s16 = reinterpret_cast<const unsigned short*>(&sball[0][0]);
    auto piece = [&](int r, int j) -> unsigned {
      const int rty = (r & 63) >> 2, ri = ((r >> 6) << 2) | (r & 3);
      return s16[((((rty >> 2) * 64) + ri * 8 + j) << 2) + (rty & 3)];
    };

    if constexpr (EPI == kEpiDense) {
      if (a.adj != nullptr) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int id = tid + kThreads * u, r = id >> 3, j = id & 7;
          const int64_t row = row0 + r, col = col0 + j * 16;
          if (row < a.rows && col < a.n) {
            const unsigned bits = piece(r, j);
            uint8_t* o = a.adj + row * a.n + col;
            if (a.vec_adj && col + 16 <= a.n) {
              uint4 v;  // bit c of a nibble -> byte c of a word
              v.x = (((bits >> 0) & 15u) * 0x00204081u) & 0x01010101u;
              v.y = (((bits >> 4) & 15u) * 0x00204081u) & 0x01010101u;
              v.z = (((bits >> 8) & 15u) * 0x00204081u) & 0x01010101u;
              v.w = (((bits >> 12) & 15u) * 0x00204081u) & 0x01010101u;
              *reinterpret_cast<uint4*>(o) = v;
            } else {
              for (int c = 0; c < 16; ++c)
                if (col + c < a.n) o[c] = (uint8_t)((bits >> c) & 1u);
            }
          }
        }
      }
      if (tid < kT) {
        int cnt = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) cnt += __popc(piece(tid, j));
        if (cnt != 0) {  // (rows outside the slab have no bits)
          if (a.vd != nullptr) atomicAdd(static_cast<VdT*>(a.vd) + row0 + tid, (VdT)cnt);
          my_edges += (unsigned)cnt;
        }
      }
    } else {
      if (tid < kT && row0 + tid < a.rows) {
        uint4 w;
        w.x = piece(tid, 0) | (piece(tid, 1) << 16);
        w.y = piece(tid, 2) | (piece(tid, 3) << 16);
        w.z = piece(tid, 4) | (piece(tid, 5) << 16);
        w.w = piece(tid, 6) | (piece(tid, 7) << 16);
        const int64_t row = row0 + tid;
        *reinterpret_cast<uint4*>(a.mask + row * a.mask_stride + ct * 4) = w;
        a.counts[row * col_tiles + ct] = (uint8_t)(__popc(w.x) + __popc(w.y) + __popc(w.z) + __popc(w.w));
      }
    }
  }
  if constexpr (EPI == kEpiDense) {
    if (my_edges != 0) atomicAdd(a.total, my_edges);
  }
}

template <typename VdT>
__global__ void eps_set_total_kernel(VdT* out, const unsigned long long* total) { *out = (VdT)*total; }

// degree of every slab row: a wave per row over its tile counts
__global__ __launch_bounds__(kThreads) void eps_degree_kernel(const uint8_t* __restrict__ counts, int64_t rows, int64_t col_tiles,
                                                              int64_t* __restrict__ deg)
{
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t row = wave; row < rows; row += waves) {
    long long s = 0;
    for (int64_t t = lane; t < col_tiles; t += 64) s += counts[row * col_tiles + t];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    if (lane == 0) deg[row] = s;
  }
}

// ids (and distances) of the slab's rows at their exact positions: row r keeps at most off[r + 1] - off[r] ids, the first in
// ascending order, from indices[off[r]] on. A wave per row: the tile counts are scanned 64 tiles at a time, and each tile
// that holds an edge is expanded from its two 64-bit mask words, a lane per column, position = offset + mbcnt of the word.
template <typename T>
__global__ __launch_bounds__(kThreads) void eps_fill_kernel(const T* __restrict__ x, const T* __restrict__ y, int64_t rows, int64_t n,
                                                            int64_t dim, const uint32_t* __restrict__ mask, int64_t mask_stride,
                                                            const uint8_t* __restrict__ counts, const int64_t* __restrict__ off,
                                                            int64_t* __restrict__ indices, float* __restrict__ distances)
{
  const int lane = threadIdx.x & 63;
  const int64_t col_tiles = (n + kT - 1) / kT;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t row = wave; row < rows; row += waves) {  // wave-uniform
    const int64_t base = off[row], cap = off[row + 1] - base;
    int64_t run = 0;  // edges of the tiles before t0
    for (int64_t t0 = 0; t0 < col_tiles && run < cap; t0 += 64) {
      const int c = t0 + lane < col_tiles ? (int)counts[row * col_tiles + t0 + lane] : 0;
      int incl = c;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(incl, o, 64);
        if (lane >= o) incl += v;
      }
      unsigned long long todo = __ballot(c > 0);
      while (todo != 0) {  // wave-uniform
        const int t = __builtin_ctzll(todo);
        todo &= todo - 1;
        int64_t pos = run + (__shfl(incl, t, 64) - __shfl(c, t, 64));
        const unsigned long long* mw = reinterpret_cast<const unsigned long long*>(mask + row * mask_stride + (t0 + t) * 4);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const unsigned long long w = mw[h];
          const int64_t mine = pos + __builtin_amdgcn_mbcnt_hi((unsigned)(w >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)w, 0u));
          if (((w >> lane) & 1ull) != 0 && mine < cap) {
            const int64_t col   = (t0 + t) * kT + h * 64 + lane;
            indices[base + mine] = col;
            if (distances != nullptr) {
              const T* xr = x + row * dim;
              const T* yr = y + col * dim;
              float acc = 0.f;
              for (int64_t k = 0; k < dim; ++k) {
                const float d = eps_f32(xr[k]) - eps_f32(yr[k]);
                acc = fmaf(d, d, acc);
              }
              distances[base + mine] = acc;
            }
          }
          pos += __popcll(w);
        }
      }
      run += __shfl(incl, 63, 64);
    }
  }
}

// ---------------------------------------------------------------- host side
struct eps_rows {
  const void* x;
  const void* y;
  H::rows_t type;
  int64_t m, n, dim;
};

eps_rows rows_of(DLManagedTensor* x, DLManagedTensor* y)
{
  eps_rows r{};
  r.type = H::check_rows(desc_of(x), desc_of(y), &r.m, &r.n, &r.dim);
  r.x    = dl_data(x->dl_tensor);
  r.y    = dl_data(y->dl_tensor);
  return r;
}

template <typename T>
int rows_vec(const eps_rows& r, int64_t row_begin)
{
  const int64_t per16 = 16 / (int64_t)sizeof(T);
  const uintptr_t xa = reinterpret_cast<uintptr_t>(static_cast<const T*>(r.x) + row_begin * r.dim);
  return (r.dim % per16 == 0 && xa % 16 == 0 && reinterpret_cast<uintptr_t>(r.y) % 16 == 0) ? 1 : 0;
}

unsigned tile_grid(const resources& res, int64_t rows, int64_t n)
{
  const int64_t tiles = ((rows + kT - 1) / kT) * ((n + kT - 1) / kT);
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>(tiles, (int64_t)res.num_cus * kWgPerCu));
}

template <typename T, typename VdT>
void launch_dense(resources& res, const eps_rows& r, int64_t r0, int64_t rows, float eps, uint8_t* adj, VdT* vd, unsigned long long* total)
{
  eps_tile_args a{};
  a.rows = rows; a.n = r.n; a.dim = r.dim; a.eps = eps;
  a.vec_rows = rows_vec<T>(r, r0);
  a.adj      = adj ? adj + r0 * r.n : nullptr;
  a.vd       = vd ? static_cast<void*>(vd + r0) : nullptr;
  a.total    = total;
  a.vec_adj  = (adj != nullptr && r.n % 16 == 0 && reinterpret_cast<uintptr_t>(adj) % 16 == 0) ? 1 : 0;
  profile_begin(res, "eps_tile_kernel_dense");
  hipLaunchKernelGGL((eps_tile_kernel<T, kEpiDense, VdT>), dim3(tile_grid(res, rows, r.n)), dim3(kThreads), 0, res.stream,
                     static_cast<const T*>(r.x) + r0 * r.dim, static_cast<const T*>(r.y), a);
  profile_end(res, "eps_tile_kernel_dense");
  HIP_TRY(hipGetLastError());
}

template <typename T>
void launch_count(resources& res, const eps_rows& r, int64_t r0, int64_t rows, float eps, uint32_t* mask, int64_t mask_stride,
                  uint8_t* counts, int64_t* deg)
{
  eps_tile_args a{};
  a.rows = rows; a.n = r.n; a.dim = r.dim; a.eps = eps;
  a.vec_rows    = rows_vec<T>(r, r0);
  a.mask        = mask;
  a.mask_stride = mask_stride;
  a.counts      = counts;
  profile_begin(res, "eps_tile_kernel_count");
  hipLaunchKernelGGL((eps_tile_kernel<T, kEpiCount, int>), dim3(tile_grid(res, rows, r.n)), dim3(kThreads), 0, res.stream,
                     static_cast<const T*>(r.x) + r0 * r.dim, static_cast<const T*>(r.y), a);
  profile_end(res, "eps_tile_kernel_count");
  const unsigned blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>((rows + 3) / 4, (int64_t)res.num_cus * 8));
  hipLaunchKernelGGL(eps_degree_kernel, dim3(blocks), dim3(kThreads), 0, res.stream, counts, rows, (r.n + kT - 1) / kT, deg);
  HIP_TRY(hipGetLastError());
}

template <typename T>
void launch_fill(resources& res, const eps_rows& r, int64_t r0, int64_t rows, const uint32_t* mask, int64_t mask_stride,
                 const uint8_t* counts, const int64_t* off, int64_t* indices, float* distances)
{
  const unsigned blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>((rows + 3) / 4, (int64_t)res.num_cus * 8));
  profile_begin(res, "eps_fill_kernel");
  hipLaunchKernelGGL(eps_fill_kernel<T>, dim3(blocks), dim3(kThreads), 0, res.stream, static_cast<const T*>(r.x) + r0 * r.dim,
                     static_cast<const T*>(r.y), rows, r.n, r.dim, mask, mask_stride, counts, off, indices, distances);
  profile_end(res, "eps_fill_kernel");
  HIP_TRY(hipGetLastError());
}

int64_t tiles_of(int64_t rows, int64_t n) { return ((rows + kT - 1) / kT) * ((n + kT - 1) / kT); }

template <typename T, typename VdT>
void eps_dense(resources& res, const eps_rows& r, uint8_t* adj, VdT* vd, float eps)
{
  uint64_t* st = g_eps_stats;
  st[0] = st[1] = st[2] = st[3] = 0;
  if (vd != nullptr) HIP_TRY(hipMemsetAsync(vd, 0, (size_t)(r.m + 1) * sizeof(VdT), res.stream));
  if (r.m == 0 || r.n == 0 || (adj == nullptr && vd == nullptr)) return;
  dev_buf<unsigned long long> total(res, 1);
  HIP_TRY(hipMemsetAsync(total.data(), 0, sizeof(unsigned long long), res.stream));
  const int64_t slab = res.tune.eps_slab_rows > 0 ? std::min<int64_t>(r.m, res.tune.eps_slab_rows) : r.m;
  for (int64_t r0 = 0; r0 < r.m; r0 += slab) {
    const int64_t rows = std::min(slab, r.m - r0);
    launch_dense<T, VdT>(res, r, r0, rows, eps, adj, vd, total.data());
    st[0] += (uint64_t)tiles_of(rows, r.n);
    st[1] += 1;
  }
  if (vd != nullptr) {
    hipLaunchKernelGGL(eps_set_total_kernel<VdT>, dim3(1), dim3(1), 0, res.stream, vd + r.m, total.data());
    HIP_TRY(hipGetLastError());
  }
  st[2] = to_host(res, total.data(), 1)[0];
}

template <typename T>
void eps_csr(resources& res, const eps_rows& r, int64_t* indptr, int64_t* indices, int64_t indices_len, float* distances,
             int64_t distances_len, int64_t* vd, float eps, int64_t* max_k)
{
  uint64_t* st = g_eps_stats;
  st[0] = st[1] = st[2] = st[3] = 0;
  const bool one_call = max_k != nullptr, fill = indices != nullptr;
  const int64_t m = r.m, cap = one_call ? *max_k : -1;
  std::vector<int64_t> h_indptr;
  if (one_call) {
    H::check_max_k(cap, m, indices_len, distances_len, distances != nullptr);
  } else if (fill) {
    h_indptr = to_host(res, indptr, (size_t)m + 1);
    H::check_fill(h_indptr.data(), m, indices_len, distances_len, distances != nullptr);
  }
  std::vector<int64_t> h_deg((size_t)m + 1, 0), h_off;
  const int64_t col_tiles = (r.n + kT - 1) / kT, mask_stride = col_tiles * 4;
  if (m > 0 && r.n > 0) {
    const int64_t slab = H::slab_rows(m, r.n, (int64_t)res.workspace_limit, res.tune.eps_slab_rows);
    dev_buf<uint32_t> mask(res, (size_t)(slab * mask_stride));
    dev_buf<uint8_t> counts(res, (size_t)(slab * col_tiles));
    dev_buf<int64_t> deg(res, (size_t)slab), d_off;
    if (one_call) d_off = dev_buf<int64_t>(res, (size_t)slab + 1);
    int64_t carry = 0;
    for (int64_t r0 = 0; r0 < m; r0 += slab) {
      const int64_t rows = std::min(slab, m - r0);
      launch_count<T>(res, r, r0, rows, eps, mask.data(), mask_stride, counts.data(), deg.data());
      copy_async(res, h_deg.data() + r0, deg.data(), (size_t)rows * sizeof(int64_t));
      sync(res);
      st[0] += (uint64_t)tiles_of(rows, r.n);
      st[1] += 1;
      if (!fill) continue;
      const int64_t* off = indptr + r0;  // the caller's offsets (a row never gets more ids than its range holds)
      if (one_call) {
        h_off.resize((size_t)rows + 1);
        carry = H::offsets_from_counts(h_deg.data() + r0, rows, cap, carry, h_off.data());
        copy_async(res, d_off.data(), h_off.data(), ((size_t)rows + 1) * sizeof(int64_t));
        copy_async(res, indptr + r0, d_off.data(), ((size_t)rows + 1) * sizeof(int64_t));
        off = d_off.data();
      }
      launch_fill<T>(res, r, r0, rows, mask.data(), mask_stride, counts.data(), off, indices, distances);
      sync(res);  // (h_off and the slab buffers are reused)
    }
  }
  int64_t edges = 0;
  for (int64_t i = 0; i < m; ++i) edges += h_deg[(size_t)i];
  st[2] = (uint64_t)edges;
  if (!fill || (one_call && (m == 0 || r.n == 0))) {  // offsets of the count call (and of a one-call form that ran no slab)
    h_off.resize((size_t)m + 1);
    H::offsets_from_counts(h_deg.data(), m, cap, 0, h_off.data());
    copy_async(res, indptr, h_off.data(), ((size_t)m + 1) * sizeof(int64_t));
  }
  if (vd != nullptr) {
    h_deg[(size_t)m] = edges;
    copy_async(res, vd, h_deg.data(), ((size_t)m + 1) * sizeof(int64_t));
  }
  sync(res);
  if (one_call) *max_k = H::largest_degree(h_deg.data(), m);
}

}  // namespace
}  // namespace cuvs_amd

using namespace cuvs_amd;

extern "C" {

cuvsError_t cuvsAmdEpsNeighbors(cuvsResources_t res_h, DLManagedTensor* x, DLManagedTensor* y, DLManagedTensor* adj,
                                DLManagedTensor* vd, float eps, cuvsDistanceType metric)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& res = *as_res(res_h);
    H::check_metric((int)metric);
    const eps_rows r = rows_of(x, y);
    H::check_adj(desc_of(adj), r.m, r.n);
    const int vd_bytes = H::check_row_vector(desc_of(vd), r.m, "vd", true, r.n);
    uint8_t* adj_p = adj ? static_cast<uint8_t*>(dl_data(adj->dl_tensor)) : nullptr;
    void* vd_p     = vd ? dl_data(vd->dl_tensor) : nullptr;
    if (r.type == H::rows_t::f32) {
      if (vd_bytes == 4) eps_dense<float, int>(res, r, adj_p, static_cast<int*>(vd_p), eps);
      else               eps_dense<float, unsigned long long>(res, r, adj_p, static_cast<unsigned long long*>(vd_p), eps);
    } else {
      if (vd_bytes == 4) eps_dense<__half, int>(res, r, adj_p, static_cast<int*>(vd_p), eps);
      else               eps_dense<__half, unsigned long long>(res, r, adj_p, static_cast<unsigned long long*>(vd_p), eps);
    }
  });
}

cuvsError_t cuvsAmdEpsNeighborsCsr(cuvsResources_t res_h, DLManagedTensor* x, DLManagedTensor* y, DLManagedTensor* indptr,
                                   DLManagedTensor* indices, DLManagedTensor* distances, DLManagedTensor* vd, float eps,
                                   cuvsDistanceType metric, int64_t* max_k)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& res = *as_res(res_h);
    H::check_metric((int)metric);
    const eps_rows r = rows_of(x, y);
    if (indptr == nullptr) H::refuse("indptr must not be NULL");
    H::check_row_vector(desc_of(indptr), r.m, "indptr", false, r.n);
    H::check_row_vector(desc_of(vd), r.m, "vd", false, r.n);
    if (indices == nullptr && max_k != nullptr) H::refuse("the max_k form needs indices");
    if (indices == nullptr && distances != nullptr) H::refuse("distances need indices");
    const int64_t ilen = indices ? H::check_list(desc_of(indices), "indices", false) : 0;
    const int64_t dlen = distances ? H::check_list(desc_of(distances), "distances", true) : 0;
    int64_t* ip = static_cast<int64_t*>(dl_data(indptr->dl_tensor));
    int64_t* ix = indices ? static_cast<int64_t*>(dl_data(indices->dl_tensor)) : nullptr;
    float* ds   = distances ? static_cast<float*>(dl_data(distances->dl_tensor)) : nullptr;
    int64_t* vp = vd ? static_cast<int64_t*>(dl_data(vd->dl_tensor)) : nullptr;
    if (r.type == H::rows_t::f32) eps_csr<float>(res, r, ip, ix, ilen, ds, dlen, vp, eps, max_k);
    else                          eps_csr<__half>(res, r, ip, ix, ilen, ds, dlen, vp, eps, max_k);
  });
}

cuvsError_t cuvsAmdEpsNeighborsLastStats(uint64_t out[4])
{
  return (cuvsError_t)translate_exceptions([=] {
    CUVS_EXPECTS(out != nullptr, "out is null");
    for (int i = 0; i < 4; ++i) out[i] = g_eps_stats[i];
  });
}

}  // extern "C"
