// Sparse (CSR) pairwise distances and sparse brute-force kNN (include/cuvs_amd/sparse.h; semantics of the reference's
// cpp/src/distance/sparse_distance.cuh + detail/sparse/* and cpp/src/neighbors/detail/sparse_knn.cuh). DESIGN 3.1x.
//
// Contract: one fp32 accumulator per pair (i, j), a sequential chain from 0 over the columns where both rows are non-zero
// (intersection family) or where at least one is (union family), in ascending column order; a stored 0.0 is an absent entry.
// A row of y with more than kSplit stored entries is cut after every kSplit-th one: every piece is a chain of its own from 0
// over the columns up to and including its last one, and the pieces are combined in order. No float atomics: a pair is owned
// by one thread, so two runs give the same bits.
//
// A 256-thread workgroup owns kTA = 4 rows of x and a tile of virtual rows of y (VR per thread, four accumulators each).
// Columns are processed in ranges that hold at least one entry of the four x rows:
//   sp_isect_kernel: the x entries of the range are scattered into a dense LDS image [kRangeI][4]; a thread walks its y row
//     up to the end of the range and reads the four x values of a column with one 16-byte LDS read. The image is cleared by
//     un-scattering the same entries.
//   sp_union_kernel: the x entries of the range are staged as four sorted (column, value) lists; a thread merges its y row
//     against the four lists at once (y-only, x-only and shared columns in column order).
// Both rows being sorted, the ascending chain falls out of the loop order for any n_cols. The epilogue is fused: finished
// values go straight to out (lanes hold consecutive y rows: a wave's store covers contiguous runs of a row of out); pieces of
// split rows go to a scratch matrix and sp_combine_kernel folds them.
// How a thread reads its y row is walk_row's business: one entry per load, or through a stage in LDS that the wave fills
// together; choose_form picks by shape from what was measured, cuvsAmdSparseSetForm forces a form.
#include "common.hpp"
#include "dl_desc.hpp"
#include "ops.hpp"
#include "sparse_distance_host.hpp"

#include <cuvs_amd/sparse.h>

#include <algorithm>
#include <climits>
#include <map>
#include <mutex>
#include <vector>

namespace cuvs_amd {
namespace {

namespace H = sparse_host;

constexpr int kThreads = H::kThreads;
constexpr int kTA      = H::kTA;

typedef float f4 __attribute__((ext_vector_type(4)));

thread_local uint64_t g_sparse_stats[4] = {0, 0, 0, 0};

struct csr_dev {
  const int* indptr;    // [rows + 1]; may point into a larger matrix: the positions are absolute
  const int* indices;
  const float* data;
  int64_t rows;
};
struct stats_dev {
  const float* sq;    // chain fmaf(v, v, sq)
  const float* sum;   // chain sum + v
  const float* ones;  // number of v == 1.0f
};

inline csr_dev slice(const csr_dev& c, int64_t r0, int64_t rows) { return csr_dev{c.indptr + r0, c.indices, c.data, rows}; }
inline stats_dev slice(const stats_dev& s, int64_t r0) { return stats_dev{s.sq + r0, s.sum + r0, s.ones + r0}; }

// ---------------------------------------------------------------- validator
// a wave per row; reads indptr[0 .. rows] and indices[0 .. nnz) only. verdict: the smallest (row, code) key found.
__global__ __launch_bounds__(kThreads) void sp_validate_kernel(const int* __restrict__ indptr, const int* __restrict__ indices, int64_t rows,
                                                               int64_t nnz, int64_t n_cols, unsigned long long* verdict)
{
  const int lane = threadIdx.x & 63;
  const int64_t gtid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t wave = gtid >> 6, waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  if (gtid == 0) {
    if (indptr[0] != 0) atomicMin(verdict, ((unsigned long long)0 << 8) | (unsigned)H::kBadIndptr0);
    if ((int64_t)indptr[rows] != nnz) atomicMin(verdict, ((unsigned long long)rows << 8) | (unsigned)H::kBadIndptrEnd);
  }
  for (int64_t row = wave; row < rows; row += waves) {
    const int64_t b = indptr[row], e = indptr[row + 1];
    if (b < 0 || e < b || e > nnz) {
      if (lane == 0) atomicMin(verdict, ((unsigned long long)row << 8) | (unsigned)H::kBadIndptrOrder);
      continue;
    }
    int bad = 0;
    for (int64_t p = b + lane; p < e; p += 64) {
      const int c = indices[p];
      if (c < 0 || (int64_t)c >= n_cols) bad |= 1;
      if (p > b && indices[p - 1] >= c) bad |= 2;
    }
    if (bad != 0) atomicMin(verdict, ((unsigned long long)row << 8) | (unsigned)((bad & 1) ? H::kBadColumn : H::kBadOrder));
  }
}

// ---------------------------------------------------------------- row statistics
// a wave per row: 64 entries per coalesced load, then every lane runs the same sequential chains over them
__global__ __launch_bounds__(kThreads) void sp_row_stats_kernel(csr_dev c, float* __restrict__ sq, float* __restrict__ sum, float* __restrict__ ones)
{
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t row = wave; row < c.rows; row += waves) {
    const int b = c.indptr[row], e = c.indptr[row + 1];
    float q = 0.f, s = 0.f;
    int o = 0;
    for (int p0 = b; p0 < e; p0 += 64) {
      const float v = p0 + lane < e ? c.data[p0 + lane] : 0.f;
      const int cnt = min(64, e - p0);
      for (int t = 0; t < cnt; ++t) {
        const float u = __shfl(v, t, 64);
        q = fmaf(u, u, q);
        s = s + u;
        o += (u == 1.f) ? 1 : 0;
      }
    }
    if (lane == 0) {
      sq[row]   = q;
      sum[row]  = s;
      ones[row] = (float)o;
    }
  }
}

// ---------------------------------------------------------------- terms and epilogues
enum : int { T_DOT = 0, T_HELLINGER, T_KL, T_L1, T_L2, T_LINF, T_CANBERRA, T_LP, T_HAMMING, T_JS };

template <int T>
__device__ inline float isect_term(float a, float b, float acc)
{
  if constexpr (T == T_DOT) return fmaf(a, b, acc);
  else if constexpr (T == T_HELLINGER) return fmaf(sqrtf(a), sqrtf(b), acc);
  else return fmaf(a, logf(a / b), acc);
}

__device__ inline float flag(bool b) { return b ? 1.f : 0.f; }

template <int T>
__device__ inline float union_term(float a, float b, float acc, float p)
{
  if constexpr (T == T_L1) return acc + fabsf(a - b);
  else if constexpr (T == T_L2) {
    const float d = a - b;
    return fmaf(d, d, acc);
  } else if constexpr (T == T_LINF) return fmaxf(acc, fabsf(a - b));
  else if constexpr (T == T_CANBERRA) {  // lp_distance.cuh:162-167
    const float d = fabsf(a) + fabsf(b);
    return acc + (flag(d != 0.f) * fabsf(a - b)) / (d + flag(d == 0.f));
  } else if constexpr (T == T_LP) return acc + powf(fabsf(a - b), p);
  else if constexpr (T == T_HAMMING) return __int_as_float(__float_as_int(acc) + (a != b ? 1 : 0));  // an integer count in the accumulator's bits
  else {  // lp_distance.cuh:249-261
    const float m = 0.5f * (a + b);
    const bool a_zero = a == 0.f, b_zero = b == 0.f;
    const float x = (flag(!a_zero) * m) / (flag(a_zero) + a);
    const float y = (flag(!b_zero) * m) / (flag(b_zero) + b);
    const bool x_zero = x == 0.f, y_zero = y == 0.f;
    const float t = (-a * (flag(!x_zero) * logf(x + flag(x_zero)))) + (-b * (flag(!y_zero) * logf(y + flag(y_zero))));
    return acc + t;
  }
}

struct epi_args {
  int metric;
  float p;         // Lp
  float n_cols_f;  // (float)n_cols
  float inv_cols;  // (float)(1.0 / (double)n_cols)
};

__device__ inline float clamp_small(float v) { return fabsf(v) < 1e-4f ? 0.f : v; }  // l2_distance.cuh:75

__device__ inline float sp_epilogue(const epi_args& e, float acc, float sqa, float suma, float onea, float sqb, float sumb, float oneb)
{
  switch (e.metric) {
    case H::L2Expanded:
    case H::L2SqrtExpanded: {
      float v = -2.f * acc;
      v = v + sqa;
      v = v + sqb;
      v = clamp_small(v);
      return e.metric == H::L2Expanded ? v : sqrtf(fmaxf(v, 0.f));
    }
    case H::CosineExpanded: {  // l2_distance.cuh:376-384
      const float norms = sqrtf(sqa) * sqrtf(sqb);
      const float cs    = (flag(norms != 0.f) * acc) / (flag(norms == 0.f) + norms);
      const bool both   = sqa == 0.f && sqb == 0.f;
      return clamp_small(1.f - ((flag(!both) * cs) + flag(both)));
    }
    case H::CorrelationExpanded: {  // l2_distance.cuh:94-108
      const float n       = e.n_cols_f;
      const float numer   = n * acc - (suma * sumb);
      const float q_denom = n * sqa - (suma * suma);
      const float r_denom = n * sqb - (sumb * sumb);
      return clamp_small(1.f - (numer / sqrtf(q_denom * r_denom)));
    }
    case H::JaccardExpanded: {  // bin_distance.cuh:142-151
      const float un    = onea + oneb;
      const float denom = un - acc;
      const float jacc  = (flag(denom != 0.f) * acc) / (flag(denom == 0.f) + denom);
      const bool both   = un == 0.f;
      return 1.f - ((flag(!both) * jacc) + flag(both));
    }
    case H::DiceExpanded: {  // bin_distance.cuh:201-206; two rows without ones: 0, as Jaccard
      const float un   = onea + oneb;
      const float dice = (2.f * acc) / un;
      return un == 0.f ? 0.f : 1.f - dice;
    }
    case H::RusselRaoExpanded: return (e.n_cols_f - acc) * e.inv_cols;
    case H::HellingerExpanded: {
      const float r = 1.f - acc;
      return r > 0.f ? sqrtf(r) : 0.f;
    }
    case H::KLDivergence: return 0.5f * acc;
    case H::L2SqrtUnexpanded: return sqrtf(acc);
    case H::LpUnexpanded: return powf(acc, 1.0f / e.p);
    case H::HammingUnexpanded: return (float)__float_as_int(acc) * e.inv_cols;
    case H::JensenShannon: return sqrtf(0.5f * acc);
    default: return acc;  // InnerProduct, L1, L2Unexpanded, Linf, Canberra
  }
}

// ---------------------------------------------------------------- the pair kernels
struct pair_args {
  csr_dev x, y;
  stats_dev xs, ys;
  const H::vrow* vrows;  // virtual rows of y
  int64_t n_vrows;
  float* out;            // out[i * ldo + j]: row i of x, row j of y
  int64_t ldo;
  float* partial;        // partial[slot * ldp + i]: raw accumulators of the pieces of split rows
  int64_t ldp;
  epi_args epi;
  unsigned long long* visited;  // column ranges processed, summed over the tiles
};

template <int VR>
struct tile_ctx {
  int64_t a0;
  int cur[kTA], end[kTA];
  bool has[VR];
  int vrow[VR], vbegin[VR], vend[VR], vslot[VR];  // the thread's virtual rows (H::vrow)
};

// a tile: kTA rows of x and VR * kThreads virtual rows of y; thread tid owns the virtual rows u * kThreads + tid of it
template <int VR>
__device__ __forceinline__ tile_ctx<VR> open_tile(const pair_args& a, int64_t tile, int64_t b_tiles)
{
  tile_ctx<VR> t;
  const int64_t at = tile / b_tiles, bt = tile - at * b_tiles;
  t.a0 = at * kTA;
#pragma unroll
  for (int r = 0; r < kTA; ++r) {
    const bool ok = t.a0 + r < a.x.rows;
    t.cur[r] = ok ? a.x.indptr[t.a0 + r] : 0;
    t.end[r] = ok ? a.x.indptr[t.a0 + r + 1] : 0;
  }
#pragma unroll
  for (int u = 0; u < VR; ++u) {
    const int64_t v = (bt * VR + u) * kThreads + threadIdx.x;
    t.has[u] = v < a.n_vrows;
    const int4 w = t.has[u] ? *reinterpret_cast<const int4*>(a.vrows + v) : make_int4(0, 0, 0, -1);
    t.vrow[u] = w.x; t.vbegin[u] = w.y; t.vend[u] = w.z; t.vslot[u] = w.w;
  }
  return t;
}

// the smallest column the four x rows still hold (INT_MAX: none)
template <int VR>
__device__ __forceinline__ int next_column(const pair_args& a, const tile_ctx<VR>& t)
{
  int cmin = INT_MAX;
#pragma unroll
  for (int r = 0; r < kTA; ++r)
    if (t.cur[r] < t.end[r]) cmin = min(cmin, a.x.indices[t.cur[r]]);
  return cmin;
}

__device__ __forceinline__ void finish_vrow(const pair_args& a, int64_t a0, bool has, int row, int slot, const float acc[kTA])
{
  if (!has) return;
  const int64_t j = row;
  if (slot < 0) {
    const float sqb = a.ys.sq[j], sumb = a.ys.sum[j], oneb = a.ys.ones[j];
#pragma unroll
    for (int r = 0; r < kTA; ++r) {
      const int64_t i = a0 + r;
      if (i < a.x.rows) a.out[i * a.ldo + j] = sp_epilogue(a.epi, acc[r], a.xs.sq[i], a.xs.sum[i], a.xs.ones[i], sqb, sumb, oneb);
    }
  } else {
#pragma unroll
    for (int r = 0; r < kTA; ++r) {
      const int64_t i = a0 + r;
      if (i < a.x.rows) a.partial[(int64_t)slot * a.ldp + i] = acc[r];
    }
  }
}

// pitch of a stage row [k]: one word more than the workgroup, so that the K lanes that fill one row's entries (slots
// [0 .. K)[thread]) hit K banks instead of one
constexpr int kSlotPitch = kThreads + 1;

// ---- the walk over a thread's row of y.
// K == 0: the lane loads one entry per visit from its own row.
// K > 0: the rows of a wave are read through a stage in LDS that the wave fills together. Slot [k][thread] holds entry
// base + k of the thread's row; [base, base + n) is staged. When lanes have used up their pieces, the wave lists them
// (s_need) and loads their next K entries 64 / K rows per instruction: K consecutive lanes read K consecutive entries of one
// row, so an instruction touches 64 / K short runs instead of 64 cache lines, and a line that is fetched serves K visits. The
// stage survives the range steps of a tile. Every lane of the wave must call this (the refill is wave-wide).
template <int K, typename Visit>
__device__ __forceinline__ void walk_row(const csr_dev& y, int& p, int pend, int& base, int& n, int c_end, int* bc, float* bv,
                                         int* s_need, Visit&& visit)
{
  if constexpr (K == 0) {
    while (p < pend) {
      const int c = y.indices[p];
      if (c >= c_end) break;
      visit(c, y.data[p]);
      ++p;
    }
  } else {
    const int tid = threadIdx.x, lane = tid & 63, wbase = tid & ~63;
    bool done = false;  // the lane has reached the end of the range or of its row
    for (;;) {          // (wave-uniform)
      bool need = false;
      if (!done && p == base + n) {
        if (p >= pend) done = true;
        else need = true;
      }
      const unsigned long long m = __ballot(need);
      if (m != 0) {
        const int cnt = __popcll(m);
        if (need) s_need[wbase + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u))] = lane;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        constexpr int kRows = 64 / K;  // rows per load instruction
        for (int g = 0; g * kRows < cnt; ++g) {
          const int idx = g * kRows + lane / K, k = lane % K;
          const int rl = s_need[wbase + min(idx, cnt - 1)];  // the lane that owns the row
          const int rp = __shfl(p, rl, 64), re = __shfl(pend, rl, 64);
          if (idx < cnt) {
            const int q = min(rp + k, re - 1);
            bc[k * kSlotPitch + wbase + rl] = y.indices[q];
            bv[k * kSlotPitch + wbase + rl] = y.data[q];
          }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (need) {
          base = p;
          n    = min(K, pend - p);
        }
      }
      if (!done) {
        while (p < base + n) {
          const int c = bc[(p - base) * kSlotPitch + tid];
          if (c >= c_end) {
            done = true;
            break;
          }
          visit(c, bv[(p - base) * kSlotPitch + tid]);
          ++p;
        }
      }
      if (__ballot(!done) == 0) break;
    }
  }
}

template <int TERM, int VR, int K>
__global__ __launch_bounds__(kThreads) void sp_isect_kernel(pair_args a)
{
  constexpr int kC = H::kRangeI, kS = K > 0 ? K : 1, kSV = K > 0 ? VR : 1, kST = K > 0 ? kSlotPitch : 1;
  __shared__ __attribute__((aligned(16))) float img[kC * kTA];  // [column - c0][x row]; zero outside the scatter
  __shared__ int bufc[kSV][kS * kST];                            // the stage of the y rows (walk_row): columns, values
  __shared__ float bufv[kSV][kS * kST];
  __shared__ int s_need[kST];
  __shared__ int s_new[kTA];

  const int tid = threadIdx.x;
  for (int i = tid; i < kC * kTA; i += kThreads) img[i] = 0.f;

  const int64_t a_tiles = (a.x.rows + kTA - 1) / kTA, b_tiles = (a.n_vrows + kThreads * VR - 1) / (kThreads * VR);
  const int64_t tiles = a_tiles * b_tiles;
  unsigned long long visited = 0;

  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {  // y tiles fastest
    tile_ctx<VR> t = open_tile<VR>(a, tile, b_tiles);
    int pos[VR], bbase[VR], bn[VR];  // per virtual row: the position in the y row and its staged piece
    float acc[VR][kTA];
#pragma unroll
    for (int u = 0; u < VR; ++u) {
      pos[u]   = t.vbegin[u];
      bbase[u] = pos[u];
      bn[u]    = 0;
#pragma unroll
      for (int r = 0; r < kTA; ++r) acc[u][r] = 0.f;
    }

    for (;;) {  // (workgroup-uniform)
      const int cmin = next_column<VR>(a, t);
      if (cmin == INT_MAX) break;
      const int c0 = cmin / kC * kC, c_end = c0 > INT_MAX - kC ? INT_MAX : c0 + kC;
      __syncthreads();  // the image is clean and s_new has been read
#pragma unroll
      for (int r = 0; r < kTA; ++r)
        if (tid == r) s_new[r] = t.end[r];
      __syncthreads();
#pragma unroll
      for (int r = 0; r < kTA; ++r) {  // scatter the entries of [c0, c_end); the thread that meets the first entry past it says where
        for (int64_t p = (int64_t)t.cur[r] + tid; p < t.end[r]; p += kThreads) {
          const int c = a.x.indices[p];
          if (c >= c_end) {
            if (p == t.cur[r] || a.x.indices[p - 1] < c_end) s_new[r] = (int)p;
            break;
          }
          img[(c - c0) * kTA + r] = a.x.data[p];
        }
      }
      __syncthreads();
#pragma unroll
      for (int u = 0; u < VR; ++u) {  // the thread's y rows up to the end of the range
        walk_row<K>(a.y, pos[u], t.vend[u], bbase[u], bn[u], c_end, bufc[K > 0 ? u : 0], bufv[K > 0 ? u : 0], s_need, [&](int c, float b) {
          if (c >= c0 && b != 0.f) {
            const f4 av = *reinterpret_cast<const f4*>(&img[(c - c0) * kTA]);  // ds_read_b128
            if (av.x != 0.f) acc[u][0] = isect_term<TERM>(av.x, b, acc[u][0]);
            if (av.y != 0.f) acc[u][1] = isect_term<TERM>(av.y, b, acc[u][1]);
            if (av.z != 0.f) acc[u][2] = isect_term<TERM>(av.z, b, acc[u][2]);
            if (av.w != 0.f) acc[u][3] = isect_term<TERM>(av.w, b, acc[u][3]);
          }
        });
      }
      __syncthreads();
#pragma unroll
      for (int r = 0; r < kTA; ++r) {  // un-scatter
        const int nw = s_new[r];
        for (int64_t p = (int64_t)t.cur[r] + tid; p < nw; p += kThreads) img[(a.x.indices[p] - c0) * kTA + r] = 0.f;
        t.cur[r] = nw;
      }
      ++visited;
    }
#pragma unroll
    for (int u = 0; u < VR; ++u) finish_vrow(a, t.a0, t.has[u], t.vrow[u], t.vslot[u], acc[u]);
  }
  if (tid == 0 && visited != 0) atomicAdd(a.visited, visited);
}

template <int TERM, int VR, int K>
__global__ __launch_bounds__(kThreads) void sp_union_kernel(pair_args a)
{
  constexpr int kC = H::kRangeU, kS = K > 0 ? K : 1, kSV = K > 0 ? VR : 1, kST = K > 0 ? kSlotPitch : 1;
  __shared__ int lcol[kTA][kC];    // the x entries of the range: at most kC per row, the columns being strictly ascending
  __shared__ float lval[kTA][kC];
  __shared__ int bufc[kSV][kS * kST];  // the stage of the y rows (walk_row)
  __shared__ float bufv[kSV][kS * kST];
  __shared__ int s_need[kST];
  __shared__ int s_new[kTA];

  const int tid = threadIdx.x;
  const int64_t a_tiles = (a.x.rows + kTA - 1) / kTA, b_tiles = (a.n_vrows + kThreads * VR - 1) / (kThreads * VR);
  const int64_t tiles = a_tiles * b_tiles;
  unsigned long long visited = 0;

  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    tile_ctx<VR> t = open_tile<VR>(a, tile, b_tiles);
    int pos[VR], bbase[VR], bn[VR], lo[VR], hi[VR];  // the columns of a piece: (lo, hi]
    float acc[VR][kTA];                              // (Hamming: the bits of integer 0)
#pragma unroll
    for (int u = 0; u < VR; ++u) {
      pos[u]   = t.vbegin[u];
      bbase[u] = pos[u];
      bn[u]    = 0;
      lo[u] = -1;
      hi[u] = INT_MAX;
      if (t.has[u] && t.vslot[u] >= 0) {
        if (t.vbegin[u] != a.y.indptr[t.vrow[u]]) lo[u] = a.y.indices[t.vbegin[u] - 1];
        if (t.vend[u] != a.y.indptr[t.vrow[u] + 1]) hi[u] = a.y.indices[t.vend[u] - 1];
      }
#pragma unroll
      for (int r = 0; r < kTA; ++r) acc[u][r] = 0.f;
    }

    for (;;) {  // (workgroup-uniform); the last pass has no x entries and takes what is left of the y rows
      const int cmin = next_column<VR>(a, t);
      const bool fin = cmin == INT_MAX;
      const int c0 = fin ? INT_MAX : cmin / kC * kC, c_end = c0 > INT_MAX - kC ? INT_MAX : c0 + kC;
      __syncthreads();  // the lists and s_new have been read
#pragma unroll
      for (int r = 0; r < kTA; ++r)
        if (tid == r) s_new[r] = t.end[r];
      __syncthreads();
      if (!fin) {
#pragma unroll
        for (int r = 0; r < kTA; ++r) {
          for (int64_t p = (int64_t)t.cur[r] + tid; p < t.end[r]; p += kThreads) {
            const int c = a.x.indices[p];
            if (c >= c_end) {
              if (p == t.cur[r] || a.x.indices[p - 1] < c_end) s_new[r] = (int)p;
              break;
            }
            lcol[r][p - t.cur[r]] = c;
            lval[r][p - t.cur[r]] = a.x.data[p];
          }
        }
      }
      __syncthreads();
      int cnt[kTA];
#pragma unroll
      for (int r = 0; r < kTA; ++r) {
        cnt[r]   = s_new[r] - t.cur[r];
        t.cur[r] = s_new[r];
      }
#pragma unroll
      for (int u = 0; u < VR; ++u) {  // (a thread without a row walks nothing: begin == end)
        int ia[kTA] = {0, 0, 0, 0};
        walk_row<K>(a.y, pos[u], t.vend[u], bbase[u], bn[u], c_end, bufc[K > 0 ? u : 0], bufv[K > 0 ? u : 0], s_need, [&](int cb, float vb) {
#pragma unroll
          for (int r = 0; r < kTA; ++r) {
            int i = ia[r];
            while (i < cnt[r] && lcol[r][i] < cb) {  // columns only x holds
              const float va = lval[r][i];
              if (lcol[r][i] > lo[u] && va != 0.f) acc[u][r] = union_term<TERM>(va, 0.f, acc[u][r], a.epi.p);
              ++i;
            }
            float va = 0.f;
            if (i < cnt[r] && lcol[r][i] == cb) va = lval[r][i++];
            if (va != 0.f || vb != 0.f) acc[u][r] = union_term<TERM>(va, vb, acc[u][r], a.epi.p);
            ia[r] = i;
          }
        });
        if (t.has[u]) {
#pragma unroll
          for (int r = 0; r < kTA; ++r) {  // what the lists still hold lies below the thread's next y column
            for (int i = ia[r]; i < cnt[r]; ++i) {
              const int ca = lcol[r][i];
              if (ca > hi[u]) break;
              const float va = lval[r][i];
              if (ca > lo[u] && va != 0.f) acc[u][r] = union_term<TERM>(va, 0.f, acc[u][r], a.epi.p);
            }
          }
        }
      }
      if (fin) break;
      ++visited;
    }
#pragma unroll
    for (int u = 0; u < VR; ++u) finish_vrow(a, t.a0, t.has[u], t.vrow[u], t.vslot[u], acc[u]);
  }
  if (tid == 0 && visited != 0) atomicAdd(a.visited, visited);
}

// the pieces of a split row, folded in order; a thread per (split row, x row), x rows fastest
__global__ __launch_bounds__(kThreads) void sp_combine_kernel(const H::split_row* __restrict__ splits, int64_t n_splits, int64_t m,
                                                              const float* __restrict__ partial, int64_t ldp, int combine, stats_dev xs,
                                                              stats_dev ys, epi_args epi, float* __restrict__ out, int64_t ldo)
{
  const int64_t total = n_splits * m;
  for (int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; id < total; id += (int64_t)gridDim.x * blockDim.x) {
    const int64_t s = id / m, i = id - s * m;
    const H::split_row sr = splits[s];
    float acc = partial[(int64_t)sr.first_slot * ldp + i];
    for (int t = 1; t < sr.pieces; ++t) {
      const float seg = partial[(int64_t)(sr.first_slot + t) * ldp + i];
      if (combine == H::kCombineMax) acc = fmaxf(acc, seg);
      else if (combine == H::kCombineCount) acc = __int_as_float(__float_as_int(acc) + __float_as_int(seg));
      else acc = acc + seg;
    }
    const int64_t j = sr.row;
    out[i * ldo + j] = sp_epilogue(epi, acc, xs.sq[i], xs.sum[i], xs.ones[i], ys.sq[j], ys.sum[j], ys.ones[j]);
  }
}

__global__ void sp_zero_diagonal_kernel(float* out, int64_t ldo, int64_t k)
{
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < k; i += (int64_t)gridDim.x * blockDim.x) out[i * ldo + i] = 0.f;
}

__global__ void sp_ids_to_int32_kernel(const int64_t* __restrict__ in, int32_t* __restrict__ out, int64_t count)
{
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (int64_t)gridDim.x * blockDim.x) out[i] = (int32_t)in[i];
}

// ---------------------------------------------------------------- host side
unsigned wave_grid(const resources& res, int64_t rows)
{
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>((rows + 3) / 4, (int64_t)res.num_cus * 8));
}

struct csr_host {
  csr_dev dev;
  int64_t nnz, n_cols;
};

csr_host csr_of(DLManagedTensor* indptr, DLManagedTensor* indices, DLManagedTensor* data, int64_t rows, int64_t n_cols, const char* what)
{
  csr_host c{};
  c.nnz    = H::check_csr(desc_of(indptr), desc_of(indices), desc_of(data), rows, n_cols, what);
  c.n_cols = n_cols;
  c.dev    = csr_dev{static_cast<const int*>(dl_data(indptr->dl_tensor)), static_cast<const int*>(dl_data(indices->dl_tensor)),
                     static_cast<const float*>(dl_data(data->dl_tensor)), rows};
  return c;
}

// ends the call unless the matrix is canonical; nothing else has touched the matrix before
void validate(resources& res, const csr_host& c, const char* what)
{
  dev_buf<unsigned long long> verdict(res, 1);
  HIP_TRY(hipMemsetAsync(verdict.data(), 0xff, sizeof(unsigned long long), res.stream));
  hipLaunchKernelGGL(sp_validate_kernel, dim3(wave_grid(res, c.dev.rows)), dim3(kThreads), 0, res.stream, c.dev.indptr, c.dev.indices,
                     c.dev.rows, c.nnz, c.n_cols, verdict.data());
  HIP_TRY(hipGetLastError());
  H::check_verdict(to_host(res, verdict.data(), 1)[0], what, c.dev.rows, c.nnz, c.n_cols);
}

struct row_stats {
  dev_buf<float> buf;  // sq | sum | ones
  int64_t rows = 0;
  stats_dev dev() const { return stats_dev{buf.data(), buf.data() + rows, buf.data() + 2 * rows}; }
};

void compute_stats(resources& res, const csr_dev& c, row_stats* st, bool persistent)
{
  st->rows = c.rows;
  st->buf  = persistent ? dev_buf<float>::persistent((size_t)c.rows * 3) : dev_buf<float>(res, (size_t)c.rows * 3);
  if (c.rows == 0) return;
  const stats_dev d = st->dev();
  hipLaunchKernelGGL(sp_row_stats_kernel, dim3(wave_grid(res, c.rows)), dim3(kThreads), 0, res.stream, c, const_cast<float*>(d.sq),
                     const_cast<float*>(d.sum), const_cast<float*>(d.ones));
  HIP_TRY(hipGetLastError());
}

// the virtual rows of a slice of y, on the device; the host vectors live as long as the plan (the copies are asynchronous)
struct y_plan {
  std::vector<H::vrow> h_vrows;
  std::vector<H::split_row> h_splits;
  dev_buf<H::vrow> vrows;
  dev_buf<H::split_row> splits;
  int64_t slots = 0;
  int64_t nnz   = 0;  // stored entries of the rows the plan covers
};

void make_plan(resources& res, const int* h_indptr, int64_t r0, int64_t rows, y_plan* p, bool persistent = false)
{
  H::plan_vrows(h_indptr, r0, rows, H::kSplit, &p->h_vrows, &p->h_splits);
  p->slots  = H::total_slots(p->h_splits);
  p->nnz    = (int64_t)h_indptr[r0 + rows] - h_indptr[r0];
  p->vrows  = persistent ? dev_buf<H::vrow>::persistent(p->h_vrows.size()) : dev_buf<H::vrow>(res, p->h_vrows.size());
  p->splits = persistent ? dev_buf<H::split_row>::persistent(p->h_splits.size()) : dev_buf<H::split_row>(res, p->h_splits.size());
  copy_async(res, p->vrows.data(), p->h_vrows.data(), p->h_vrows.size() * sizeof(H::vrow));
  copy_async(res, p->splits.data(), p->h_splits.data(), p->h_splits.size() * sizeof(H::split_row));
}

// The form of the walk (walk_row): virtual rows of y per thread, entries of a row staged per refill (0: no stage).
struct walk_form {
  int vr, k;
};
constexpr walk_form kForms[5] = {{0, 0}, {8, 0}, {1, 8}, {1, 16}, {2, 8}};  // [0] = choose by shape; union: {8, 0} runs as {4, 0}
int g_form[2] = {0, 0};  // cuvsAmdSparseSetForm (comparators of the timing and of the tests): intersection, union

// by shape: the stage pays when a row has entries to stage per range step; below that, more rows per thread share the step
walk_form choose_form(bool isect, const pair_args& a, int64_t n_cols, int64_t y_nnz)
{
  const int forced = g_form[isect ? 0 : 1];
  walk_form f = kForms[forced >= 1 && forced <= 4 ? forced : 0];
  if (f.vr == 0) {
    const double per_step = (double)y_nnz / (double)std::max<int64_t>(a.n_vrows, 1) /
                            (double)std::max<int64_t>(H::n_ranges(n_cols, isect ? H::kRangeI : H::kRangeU), 1);
    // (the union kernel stays on the direct form: its staged forms lost on every shape measured)
    f = isect && per_step >= H::kStageMinPerStep ? kForms[H::kFormStaged] : kForms[H::kFormDirect];
  }
  if (!isect && f.k == 0) f.vr = 4;
  return f;
}

template <typename Kernel>
void launch_kernel(resources& res, Kernel kern, const char* name, int64_t tiles, const pair_args& a)
{
  int per_cu = 0;  // what the kernel's LDS and registers let a CU hold
  HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, kThreads, 0));
  const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(tiles, (int64_t)res.num_cus * std::max(per_cu, 1)));
  profile_begin(res, name);
  hipLaunchKernelGGL(kern, dim3(grid), dim3(kThreads), 0, res.stream, a);
  profile_end(res, name);
  HIP_TRY(hipGetLastError());
}

template <int TERM>
void launch_pairs(resources& res, bool isect, walk_form f, const pair_args& a)
{
  const int64_t tiles = H::n_tiles(a.x.rows, a.n_vrows, f.vr);
  if constexpr (TERM <= T_KL) {
    if (f.k == 0)                     launch_kernel(res, sp_isect_kernel<TERM, 8, 0>, "sp_isect_kernel", tiles, a);
    else if (f.vr == 2)               launch_kernel(res, sp_isect_kernel<TERM, 2, 8>, "sp_isect_kernel", tiles, a);
    else if (f.k == 16)               launch_kernel(res, sp_isect_kernel<TERM, 1, 16>, "sp_isect_kernel", tiles, a);
    else                              launch_kernel(res, sp_isect_kernel<TERM, 1, 8>, "sp_isect_kernel", tiles, a);
  } else {
    if (f.k == 0)                     launch_kernel(res, sp_union_kernel<TERM, 4, 0>, "sp_union_kernel", tiles, a);
    else if (f.vr == 2)               launch_kernel(res, sp_union_kernel<TERM, 2, 8>, "sp_union_kernel", tiles, a);
    else if (f.k == 16)               launch_kernel(res, sp_union_kernel<TERM, 1, 16>, "sp_union_kernel", tiles, a);
    else                              launch_kernel(res, sp_union_kernel<TERM, 1, 8>, "sp_union_kernel", tiles, a);
  }
  (void)isect;
}

// out[i * ldo + j] for the m rows of x and the rows of y the plan covers. `visited`: a device counter. st: the call's statistics.
void pair_distances(resources& res, const csr_dev& x, const stats_dev& xs, const csr_dev& y, const stats_dev& ys, const y_plan& plan,
                    int metric, float p, int64_t n_cols, float* out, int64_t ldo, unsigned long long* visited, uint64_t* st)
{
  if (x.rows == 0 || y.rows == 0) return;
  const bool isect     = H::family_of(metric) == H::kIntersection;
  const int64_t y_nnz  = plan.nnz;
  const int64_t slab   = H::slab_rows(x.rows, plan.slots, (int64_t)res.workspace_limit);
  dev_buf<float> partial(res, (size_t)(plan.slots * slab));
  epi_args epi{metric, p, (float)n_cols, n_cols > 0 ? (float)(1.0 / (double)n_cols) : 0.f};
  for (int64_t r0 = 0; r0 < x.rows; r0 += slab) {
    const int64_t rows = std::min(slab, x.rows - r0);
    pair_args a{};
    a.x = slice(x, r0, rows); a.y = y;
    a.xs = slice(xs, r0); a.ys = ys;
    a.vrows = plan.vrows.data(); a.n_vrows = (int64_t)plan.h_vrows.size();
    a.out = out + r0 * ldo; a.ldo = ldo;
    a.partial = partial.data(); a.ldp = slab;
    a.epi = epi;
    a.visited = visited;
    const walk_form f = choose_form(isect, a, n_cols, y_nnz);
    switch (metric) {
      case H::HellingerExpanded: launch_pairs<T_HELLINGER>(res, true, f, a); break;
      case H::KLDivergence: launch_pairs<T_KL>(res, true, f, a); break;
      case H::L1: launch_pairs<T_L1>(res, false, f, a); break;
      case H::L2Unexpanded:
      case H::L2SqrtUnexpanded: launch_pairs<T_L2>(res, false, f, a); break;
      case H::Linf: launch_pairs<T_LINF>(res, false, f, a); break;
      case H::Canberra: launch_pairs<T_CANBERRA>(res, false, f, a); break;
      case H::LpUnexpanded: launch_pairs<T_LP>(res, false, f, a); break;
      case H::HammingUnexpanded: launch_pairs<T_HAMMING>(res, false, f, a); break;
      case H::JensenShannon: launch_pairs<T_JS>(res, false, f, a); break;
      default: launch_pairs<T_DOT>(res, true, f, a); break;
    }
    if (plan.slots > 0) {
      const int64_t n_splits = (int64_t)plan.h_splits.size();
      hipLaunchKernelGGL(sp_combine_kernel, dim3(grid_blocks(std::min<int64_t>(n_splits * rows, int64_t(1) << 20), kThreads)), dim3(kThreads),
                         0, res.stream, plan.splits.data(), n_splits, rows, partial.data(), slab, H::combine_of(metric), a.xs, a.ys, epi,
                         a.out, ldo);
      HIP_TRY(hipGetLastError());
    }
    const int64_t tiles = H::n_tiles(rows, a.n_vrows, f.vr);
    st[1] += (uint64_t)(tiles * H::n_ranges(n_cols, isect ? H::kRangeI : H::kRangeU));  // (all ranges; the visited ones are taken off at the end)
    st[2] += (uint64_t)plan.slots;
    st[3] += (uint64_t)tiles;
  }
}

struct visit_counter {
  dev_buf<unsigned long long> d;
  explicit visit_counter(resources& res) : d(res, 1) { HIP_TRY(hipMemsetAsync(d.data(), 0, sizeof(unsigned long long), res.stream)); }
  void finish(resources& res, uint64_t* st)  // also the call's final synchronisation
  {
    st[0] = to_host(res, d.data(), 1)[0];
    st[1] -= std::min(st[1], st[0]);
  }
};

struct sparse_bf_index {
  csr_host csr{};
  int metric = 0;
  float p    = 2.f;
  row_stats stats;
  std::vector<int> h_indptr;
  // the virtual-row plans of the index batches for the batch size of the last search, kept on the device
  mutable std::mutex mu;
  mutable std::map<int64_t, std::shared_ptr<std::vector<y_plan>>> plans;
};

std::shared_ptr<std::vector<y_plan>> plans_of(resources& res, const sparse_bf_index& ix, int64_t bs_index)
{
  std::lock_guard<std::mutex> lock(ix.mu);
  if (ix.plans.count(bs_index) == 0) ix.plans.clear();  // only the plans of the last batch size are kept
  auto& slot = ix.plans[bs_index];
  if (!slot) {
    const int64_t n = ix.csr.dev.rows, n_ib = H::n_batches(n, bs_index);
    slot = std::make_shared<std::vector<y_plan>>((size_t)n_ib);
    for (int64_t ib = 0; ib < n_ib; ++ib) {
      int64_t i0, irows;
      H::batch_rows(n, bs_index, ib, &i0, &irows);
      make_plan(res, ix.h_indptr.data(), i0, irows, &(*slot)[(size_t)ib], true);
    }
    sync(res);
  }
  return slot;
}

void sparse_search(resources& res, const sparse_bf_index& ix, const csr_host& q, int64_t k, int64_t bs_index, int64_t bs_query,
                   void* neighbors, int id_bytes, float* distances)
{
  uint64_t* st = g_sparse_stats;
  st[0] = st[1] = st[2] = st[3] = 0;
  const int64_t nq = q.dev.rows, n = ix.csr.dev.rows;
  if (nq == 0) return;
  validate(res, q, "the queries");
  row_stats qs;
  compute_stats(res, q.dev, &qs, false);
  visit_counter visited(res);
  const bool smin = H::select_min(ix.metric);
  bs_index = std::min(bs_index, n);
  bs_query = std::min(bs_query, nq);
  H::cap_tile((int64_t)res.workspace_limit, &bs_index, &bs_query);  // (the batch sizes never change results)
  const int64_t n_ib = H::n_batches(n, bs_index), n_qb = H::n_batches(nq, bs_query);
  const auto plans_p = plans_of(res, ix, bs_index);
  const std::vector<y_plan>& plans = *plans_p;
  dev_buf<float> tile(res, (size_t)(bs_query * bs_index));
  dev_buf<float> buf_v[2];
  dev_buf<int64_t> buf_i[2];
  if (n_ib > 1) {
    for (int b = 0; b < 2; ++b) {
      buf_v[b] = dev_buf<float>(res, (size_t)(bs_query * 2 * k));
      buf_i[b] = dev_buf<int64_t>(res, (size_t)(bs_query * 2 * k));
    }
  }
  dev_buf<int64_t> wide(res, id_bytes == 4 ? (size_t)(bs_query * k) : 0);
  const stats_dev xs = qs.dev(), ys = ix.stats.dev();
  for (int64_t qb = 0; qb < n_qb; ++qb) {
    int64_t q0, qrows;
    H::batch_rows(nq, bs_query, qb, &q0, &qrows);
    float* out_d   = distances + q0 * k;
    int64_t* out_i = id_bytes == 8 ? static_cast<int64_t*>(neighbors) + q0 * k : wide.data();
    int cur = 0;
    for (int64_t ib = 0; ib < n_ib; ++ib) {
      int64_t i0, irows;
      H::batch_rows(n, bs_index, ib, &i0, &irows);
      pair_distances(res, slice(q.dev, q0, qrows), slice(xs, q0), slice(ix.csr.dev, i0, irows), slice(ys, i0), plans[(size_t)ib], ix.metric,
                     ix.p, ix.csr.n_cols, tile.data(), irows, visited.d.data(), st);
      if (n_ib == 1) {
        select_k<int64_t, int64_t>(res, tile.data(), nullptr, qrows, irows, irows, (int)k, out_d, out_i, smin, i0);
      } else if (ib == 0) {
        select_k<int64_t, int64_t>(res, tile.data(), nullptr, qrows, irows, irows, (int)k, buf_v[cur].data(), buf_i[cur].data(), smin, i0,
                                   2 * k, 0);
      } else {  // the batch's k best next to the k best so far (earlier rows first: ties go to the smaller id), then the k best of both
        select_k<int64_t, int64_t>(res, tile.data(), nullptr, qrows, irows, irows, (int)k, buf_v[cur].data(), buf_i[cur].data(), smin, i0,
                                   2 * k, k);
        if (ib + 1 == n_ib) {
          select_k<int64_t, int64_t>(res, buf_v[cur].data(), buf_i[cur].data(), qrows, 2 * k, 2 * k, (int)k, out_d, out_i, smin);
        } else {
          select_k<int64_t, int64_t>(res, buf_v[cur].data(), buf_i[cur].data(), qrows, 2 * k, 2 * k, (int)k, buf_v[cur ^ 1].data(),
                                     buf_i[cur ^ 1].data(), smin, 0, 2 * k, 0);
          cur ^= 1;
        }
      }
    }
    if (id_bytes == 4) {
      hipLaunchKernelGGL(sp_ids_to_int32_kernel, dim3(grid_blocks(std::min<int64_t>(qrows * k, int64_t(1) << 20), kThreads)), dim3(kThreads), 0,
                         res.stream, wide.data(), static_cast<int32_t*>(neighbors) + q0 * k, qrows * k);
      HIP_TRY(hipGetLastError());
    }
  }
  visited.finish(res, st);
}

}  // namespace
}  // namespace cuvs_amd

using namespace cuvs_amd;

extern "C" {

cuvsError_t cuvsAmdSparseCsrValidate(cuvsResources_t res_h, DLManagedTensor* indptr, DLManagedTensor* indices, DLManagedTensor* data,
                                     int64_t n_rows, int64_t n_cols)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& res = *as_res(res_h);
    validate(res, csr_of(indptr, indices, data, n_rows, n_cols, "the matrix"), "the matrix");
  });
}

cuvsError_t cuvsAmdSparsePairwiseDistance(cuvsResources_t res_h, DLManagedTensor* x_indptr, DLManagedTensor* x_indices,
                                          DLManagedTensor* x_data, int64_t m, DLManagedTensor* y_indptr, DLManagedTensor* y_indices,
                                          DLManagedTensor* y_data, int64_t n, int64_t n_cols, DLManagedTensor* out, cuvsDistanceType metric,
                                          float metric_arg)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& res    = *as_res(res_h);
    uint64_t* st = g_sparse_stats;
    st[0] = st[1] = st[2] = st[3] = 0;
    H::check_metric((int)metric, metric_arg);
    const csr_host x = csr_of(x_indptr, x_indices, x_data, m, n_cols, "x");
    const csr_host y = csr_of(y_indptr, y_indices, y_data, n, n_cols, "y");
    H::check_out(desc_of(out), m, n);
    const bool same = x.dev.indptr == y.dev.indptr && x.dev.indices == y.dev.indices && x.dev.data == y.dev.data && m == n && x.nnz == y.nnz;
    validate(res, x, "x");
    if (!same) validate(res, y, "y");
    if (m == 0 || n == 0) return;
    row_stats xs, ys_own;
    compute_stats(res, x.dev, &xs, false);
    if (!same) compute_stats(res, y.dev, &ys_own, false);
    const stats_dev ys = same ? xs.dev() : ys_own.dev();
    const std::vector<int> h_indptr = to_host(res, y.dev.indptr, (size_t)n + 1);
    y_plan plan;
    make_plan(res, h_indptr.data(), 0, n, &plan);
    visit_counter visited(res);
    float* o = static_cast<float*>(dl_data(out->dl_tensor));
    pair_distances(res, x.dev, xs.dev(), y.dev, ys, plan, (int)metric, metric_arg, n_cols, o, n, visited.d.data(), st);
    if ((int)metric == H::RusselRaoExpanded) {
      const int64_t k = std::min(m, n);
      hipLaunchKernelGGL(sp_zero_diagonal_kernel, dim3(grid_blocks(std::min<int64_t>(k, int64_t(1) << 20), kThreads)), dim3(kThreads), 0,
                         res.stream, o, n, k);
      HIP_TRY(hipGetLastError());
    }
    visited.finish(res, st);
  });
}

cuvsError_t cuvsAmdSparseBruteForceIndexCreate(cuvsAmdSparseBruteForceIndex_t* index)
{
  return (cuvsError_t)translate_exceptions([=] {
    CUVS_EXPECTS(index != nullptr, "index is null");
    *index = new cuvsAmdSparseBruteForceIndex{0};
  });
}

cuvsError_t cuvsAmdSparseBruteForceIndexDestroy(cuvsAmdSparseBruteForceIndex_t index)
{
  return (cuvsError_t)translate_exceptions([=] {
    if (index == nullptr) return;
    delete reinterpret_cast<sparse_bf_index*>(index->addr);
    delete index;
  });
}

cuvsError_t cuvsAmdSparseBruteForceBuild(cuvsResources_t res_h, DLManagedTensor* indptr, DLManagedTensor* indices, DLManagedTensor* data,
                                         int64_t n_rows, int64_t n_cols, cuvsDistanceType metric, float metric_arg,
                                         cuvsAmdSparseBruteForceIndex_t index)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& res = *as_res(res_h);
    CUVS_EXPECTS(index != nullptr, "index is null");
    H::check_metric((int)metric, metric_arg);
    auto ix    = std::make_unique<sparse_bf_index>();
    ix->csr    = csr_of(indptr, indices, data, n_rows, n_cols, "the index");
    ix->metric = (int)metric;
    ix->p      = metric_arg;
    validate(res, ix->csr, "the index");
    compute_stats(res, ix->csr.dev, &ix->stats, true);
    ix->h_indptr = to_host(res, ix->csr.dev.indptr, (size_t)n_rows + 1);
    delete reinterpret_cast<sparse_bf_index*>(index->addr);
    index->addr = reinterpret_cast<uintptr_t>(ix.release());
  });
}

cuvsError_t cuvsAmdSparseBruteForceSearch(cuvsResources_t res_h, cuvsAmdSparseBruteForceIndex_t index, DLManagedTensor* q_indptr,
                                          DLManagedTensor* q_indices, DLManagedTensor* q_data, int64_t n_queries, int64_t k,
                                          int64_t batch_size_index, int64_t batch_size_query, DLManagedTensor* neighbors,
                                          DLManagedTensor* distances)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& res = *as_res(res_h);
    CUVS_EXPECTS(index != nullptr && index->addr != 0, "the index has not been built");
    const sparse_bf_index& ix = *reinterpret_cast<const sparse_bf_index*>(index->addr);
    const csr_host q          = csr_of(q_indptr, q_indices, q_data, n_queries, ix.csr.n_cols, "the queries");
    const int id_bytes = H::check_knn(desc_of(neighbors), desc_of(distances), n_queries, k, ix.csr.dev.rows, batch_size_index, batch_size_query);
    sparse_search(res, ix, q, k, batch_size_index, batch_size_query, dl_data(neighbors->dl_tensor), id_bytes,
                  static_cast<float*>(dl_data(distances->dl_tensor)));
  });
}

// Comparator hook (not part of sparse.h): the form of the walk over the rows of y for the intersection and the union kernel,
// an index into kForms; 0 chooses by shape. Process-wide; the results never depend on it.
__attribute__((visibility("default"))) cuvsError_t cuvsAmdSparseSetForm(int intersection, int union_)
{
  return (cuvsError_t)translate_exceptions([=] {
    CUVS_EXPECTS(intersection >= 0 && intersection <= 4 && union_ >= 0 && union_ <= 4, "forms are 0 .. 4");
    g_form[0] = intersection;
    g_form[1] = union_;
  });
}

cuvsError_t cuvsAmdSparseLastStats(uint64_t out[4])
{
  return (cuvsError_t)translate_exceptions([=] {
    CUVS_EXPECTS(out != nullptr, "out is null");
    for (int i = 0; i < 4; ++i) out[i] = g_sparse_stats[i];
  });
}

}  // extern "C"
