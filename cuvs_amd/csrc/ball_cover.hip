// Random ball cover (include/cuvs_amd/ball_cover.h; semantics of the reference's cpp/include/cuvs/neighbors/ball_cover.hpp).
// DESIGN 3.1u has the contract.
//
// One __device__ distance function per metric serves the build, the landmark pass and the list scan: the L2 chain
// acc = fmaf(d, d, acc) then sqrtf, or the reference's haversine formula. Every comparison is on (distance, id): a candidate
// is the 64-bit key (distance bits << 32 | id), distances are not negative, so keys order like the pairs.
//
// bc_knn_kernel: a wave (one 64-thread workgroup) per query. The sorted top-k lives in LDS, k <= 256 keys; a lane whose
// candidate beats the k-th key (tau) hands it to the wave, which inserts it by shifting the tail (every lane moves its 64 * j +
// lane slots). The k nearest landmarks are selected the same way, their lists scanned (pass one), then every other list
// whose ball can still hold a candidate under the pass-one tau (pass two). Inside a list the rows are sorted by their
// distance to the landmark, so the rows that can still matter are a contiguous window found by a 64-ary search.
// bc_eps_kernel: the same walk with a fixed bound; the CSR fill collects (id, position) pairs of a row in list order and
// sorts them by id with a wave-level LSD radix sort before they are written.
#include "common.hpp"
#include "ball_cover_host.hpp"
#include "dl_desc.hpp"

#include <cuvs_amd/ball_cover.h>

#include <cfloat>
#include <cstring>
#include <vector>

namespace cuvs_amd {
namespace {

namespace H = eps_host;
namespace B = bc_host;

constexpr int kWave = 64;
constexpr unsigned long long kPad = ~0ull;

thread_local uint64_t g_bc_stats[4] = {0, 0, 0, 0};

struct bc_index {
  int metric  = 0;
  int64_t m = 0, dim = 0, L = 0;
  dev_buf<float> X, R, dists, radius;       // X_reordered [m, dim], R [L, dim], R_1nn_dists [m], R_radius [L]
  dev_buf<int64_t> indptr, cols, rrows;     // R_indptr [L + 1], R_1nn_cols [m], the landmarks' row ids [L]
};

// ---------------------------------------------------------------- distances
enum : int { kL2 = 0, kHav = 1 };

__device__ __forceinline__ float bc_l2_acc(const float* a, const float* b, int dim)
{
  float acc = 0.f;
  for (int t = 0; t < dim; ++t) {
    const float d = a[t] - b[t];
    acc = fmaf(d, d, acc);
  }
  return acc;
}
__device__ __forceinline__ float bc_l2(const float* a, const float* b, int dim) { return sqrtf(bc_l2_acc(a, b, dim)); }
// haversine_distance.cuh:32-36 with (x1, y1, x2, y2) = (a[0], b[0], a[1], b[1])
__device__ __forceinline__ float bc_haversine(const float* a, const float* b)
{
  const float sin_0 = sinf(0.5f * (a[0] - b[0]));
  const float sin_1 = sinf(0.5f * (a[1] - b[1]));
  const float rdist = sin_0 * sin_0 + cosf(a[0]) * cosf(b[0]) * sin_1 * sin_1;
  return 2.f * asinf(sqrtf(rdist));
}
template <int METRIC>
__device__ __forceinline__ float bc_dist(const float* a, const float* b, int dim)
{
  if constexpr (METRIC == kHav) return bc_haversine(a, b);
  else return bc_l2(a, b, dim);
}

// ---------------------------------------------------------------- pruning
// dq: query to landmark, dp: a row of the list (or the list's radius) to the landmark, bound = fmaf(c, tau, tau) + s.
// bc_below: the row is so much nearer to the landmark than the query that it is further than tau from the query;
// bc_beyond: the same with the roles swapped. Both are monotone in dp.
__device__ __forceinline__ bool bc_below(float dq, float dp, float bound, float c) { return (fmaf(-c, dq, dq) - fmaf(c, dp, dp)) > bound; }
__device__ __forceinline__ bool bc_beyond(float dq, float dp, float bound, float c) { return (fmaf(-c, dp, dp) - fmaf(c, dq, dq)) > bound; }

// first index of [0, n) at which the monotone (false ... true) predicate holds, n when it never does; wave-uniform
template <typename Pred>
__device__ __forceinline__ int64_t bc_first_true(int64_t n, int lane, Pred pred)
{
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t step = (hi - lo + kWave - 1) / kWave;
    const int64_t idx  = lo + (int64_t)(lane + 1) * step - 1;
    const bool t       = idx >= hi ? true : pred(idx);
    const unsigned long long b = __ballot(t);
    if (b == 0) return hi;
    const int j          = __builtin_ctzll(b);
    const int64_t idx_j = lo + (int64_t)(j + 1) * step - 1;
    lo = lo + (int64_t)j * step;
    hi = idx_j < hi ? idx_j : hi;
  }
  return lo;
}

// the rows [a, b) of a list of n sorted distances that the bound does not rule out
__device__ __forceinline__ void bc_window(const float* __restrict__ dists, int64_t n, int lane, float dq, float bound, float c, int64_t* a,
                                          int64_t* b)
{
  const int64_t lo = bc_first_true(n, lane, [&](int64_t i) { return !bc_below(dq, dists[i], bound, c); });
  const int64_t hi = lo + bc_first_true(n - lo, lane, [&](int64_t i) { return bc_beyond(dq, dists[lo + i], bound, c); });
  *a = lo;
  *b = hi;
}

// ---------------------------------------------------------------- the sorted top-k of a wave
// arr: 64 * KS keys in LDS, ascending, the first k in use (the rest stay kPad). One workgroup is one wave, so
// __syncthreads() orders the LDS traffic of its lanes.
template <int KS>
__device__ __forceinline__ void bc_insert(unsigned long long* arr, int k, int lane, unsigned long long key)
{
  unsigned long long cur[KS], prev[KS];
#pragma unroll
  for (int j = 0; j < KS; ++j) {
    const int i = lane + kWave * j;
    cur[j]  = arr[i];
    prev[j] = i > 0 ? arr[i - 1] : 0ull;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < KS; ++j) {
    const int i = lane + kWave * j;
    if (i < k && !(cur[j] < key)) arr[i] = (i == 0 || prev[j] < key) ? key : prev[j];
  }
  __syncthreads();
}
// every lane offers one key (kPad: none); tau is arr[k - 1]
template <int KS>
__device__ __forceinline__ void bc_push(unsigned long long* arr, int k, int lane, unsigned long long key, unsigned long long& tau)
{
  unsigned long long todo = __ballot(key < tau);
  while (todo != 0) {  // wave-uniform
    const int j = __builtin_ctzll(todo);
    todo &= todo - 1;
    const unsigned long long kj = __shfl(key, j, kWave);
    if (kj < tau) {
      bc_insert<KS>(arr, k, lane, kj);
      tau = arr[k - 1];
    }
  }
}

struct bc_knn_args {
  const float* X;          // [m, DIM] reordered
  const float* R;          // [L, DIM]
  const float* dists;      // [m]
  const float* radius;     // [L]
  const int64_t* indptr;   // [L + 1]
  const int64_t* cols;     // [m]
  const float* queries;    // [nq, DIM]
  int64_t nq, L;
  int k;
  int post_filter;
  float weight, c, s;      // the visit weight, the relative margin and the absolute slack of the pruning expressions
  int64_t* out_ids;        // [nq, k]
  float* out_dists;        // [nq, k]
  unsigned long long* stats;  // [3]: lists visited, rows scored, rows skipped by the window
};

template <int METRIC, int DIM, int KS>
__global__ __launch_bounds__(kWave) void bc_knn_kernel(bc_knn_args a)
{
  __shared__ unsigned long long best[kWave * KS];
  __shared__ unsigned long long lm[kWave * KS];
  const int lane = threadIdx.x;
  unsigned long long n_visited = 0, n_scored = 0, n_skipped = 0;

  for (int64_t qi = blockIdx.x; qi < a.nq; qi += gridDim.x) {
    float q[DIM];
#pragma unroll
    for (int t = 0; t < DIM; ++t) q[t] = a.queries[qi * DIM + t];
    __syncthreads();  // the previous query's keys have been written out
#pragma unroll
    for (int j = 0; j < KS; ++j) best[lane + kWave * j] = lm[lane + kWave * j] = kPad;
    __syncthreads();

    unsigned long long tau = kPad;
    // rows [beg, beg + n) of one list against the running top-k
    auto scan_list = [&](int64_t l, float dq) {
      const int64_t beg = a.indptr[l], n = a.indptr[l + 1] - beg;
      if (n == 0) return;  // an empty list is never visited
      const float tau_f = tau == kPad ? __builtin_inff() : __uint_as_float((unsigned)(tau >> 32));
      int64_t w0, w1;
      bc_window(a.dists + beg, n, lane, dq, fmaf(a.c, tau_f, tau_f) + a.s, a.c, &w0, &w1);
      n_visited += 1;
      n_scored += (unsigned long long)(w1 - w0);
      n_skipped += (unsigned long long)(n - (w1 - w0));
      for (int64_t i0 = w0; i0 < w1; i0 += kWave) {  // wave-uniform
        const int64_t i = i0 + lane;
        unsigned long long key = kPad;
        if (i < w1) {
          float p[DIM];
#pragma unroll
          for (int t = 0; t < DIM; ++t) p[t] = a.X[(beg + i) * DIM + t];
          const unsigned bits = __float_as_uint(bc_dist<METRIC>(q, p, DIM));
          if (bits <= (unsigned)(tau >> 32)) key = ((unsigned long long)bits << 32) | (unsigned long long)(unsigned)a.cols[beg + i];
        }
        bc_push<KS>(best, a.k, lane, key, tau);
      }
    };

    // the k nearest landmarks by (distance, landmark)
    unsigned long long lm_tau = kPad;
    for (int64_t l0 = 0; l0 < a.L; l0 += kWave) {
      const int64_t l = l0 + lane;
      unsigned long long key = kPad;
      if (l < a.L) {
        float r[DIM];
#pragma unroll
        for (int t = 0; t < DIM; ++t) r[t] = a.R[l * DIM + t];
        key = ((unsigned long long)__float_as_uint(bc_dist<METRIC>(q, r, DIM)) << 32) | (unsigned long long)(unsigned)l;
      }
      bc_push<KS>(lm, a.k, lane, key, lm_tau);
    }
    // pass one: their lists (k <= L: all k keys are landmarks)
    for (int t = 0; t < a.k; ++t) {
      const unsigned long long key = lm[t];
      scan_list((int64_t)(unsigned)key, __uint_as_float((unsigned)(key >> 32)));
    }
    // pass two: every other list whose ball the pass-one tau does not rule out
    if (a.post_filter) {
      const float tau1  = tau == kPad ? __builtin_inff() : __uint_as_float((unsigned)(tau >> 32));
      const float bound = fmaf(a.c, tau1, tau1) + a.s;
      for (int64_t l0 = 0; l0 < a.L; l0 += kWave) {
        const int64_t l = l0 + lane;
        bool visit = false;
        float dq   = 0.f;
        if (l < a.L) {
          float r[DIM];
#pragma unroll
          for (int t = 0; t < DIM; ++t) r[t] = a.R[l * DIM + t];
          dq = bc_dist<METRIC>(q, r, DIM);
          const unsigned long long key = ((unsigned long long)__float_as_uint(dq) << 32) | (unsigned long long)(unsigned)l;
          const float rad = a.radius[l];
          visit = key > lm_tau && a.indptr[l + 1] > a.indptr[l] && a.weight * (fmaf(-a.c, dq, dq) - fmaf(a.c, rad, rad)) <= bound;
        }
        unsigned long long todo = __ballot(visit);
        while (todo != 0) {  // wave-uniform
          const int j = __builtin_ctzll(todo);
          todo &= todo - 1;
          scan_list(l0 + j, __shfl(dq, j, kWave));
        }
      }
    }
#pragma unroll
    for (int j = 0; j < KS; ++j) {
      const int i = lane + kWave * j;
      if (i < a.k) {
        const unsigned long long key = best[i];
        a.out_ids[qi * a.k + i]   = key == kPad ? INT64_MAX : (int64_t)(unsigned)key;
        a.out_dists[qi * a.k + i] = key == kPad ? FLT_MAX : __uint_as_float((unsigned)(key >> 32));
      }
    }
  }
  if (lane == 0 && a.stats != nullptr) {
    atomicAdd(a.stats + 0, n_visited);
    atomicAdd(a.stats + 1, n_scored);
    atomicAdd(a.stats + 2, n_skipped);
  }
}

// ---------------------------------------------------------------- eps_nn
enum : int { kEpsCount = 0, kEpsDense = 1, kEpsCollect = 2 };

struct bc_eps_args {
  const float* X;
  const float* R;
  const float* dists;
  const float* radius;
  const int64_t* indptr;
  const int64_t* cols;
  const float* queries;    // [nq, dim], the rows of this launch
  int64_t nq, L, m;
  int dim;
  float eps, eps2, c;      // the radius, fp32(eps * eps), the margin
  int64_t* deg;            // [nq] (count, dense)
  uint8_t* adj;            // [nq, m] zeroed, or null (dense)
  // collect
  const int64_t* tmp_off;  // [nq + 1]: the rows' ranges of the scratch lists
  unsigned long long* tmp; // (id << 32 | reordered position), two buffers of tmp_off[nq] entries
  unsigned long long* tmp2;
  const int64_t* off;      // [nq + 1]: the rows' ranges of the output
  int64_t* indices;
  float* distances;        // or null
  int id_bytes;            // radix passes: the bytes of an id that can be non-zero
  unsigned long long* stats;
};

template <int MODE>
__global__ __launch_bounds__(kWave) void bc_eps_kernel(bc_eps_args a)
{
  __shared__ float qs[B::kMaxEpsDim];
  __shared__ unsigned hist[256];
  const int lane = threadIdx.x;
  const float bound = fmaf(a.c, a.eps, a.eps);
  unsigned long long n_visited = 0, n_scored = 0, n_skipped = 0;

  for (int64_t qi = blockIdx.x; qi < a.nq; qi += gridDim.x) {
    __syncthreads();  // the previous query has been read
    if (lane < a.dim) qs[lane] = a.queries[qi * a.dim + lane];
    __syncthreads();
    int64_t cnt = 0;  // members so far, wave-uniform
    const int64_t tbase = MODE == kEpsCollect ? a.tmp_off[qi] : 0;
    for (int64_t l0 = 0; l0 < a.L; l0 += kWave) {
      const int64_t l = l0 + lane;
      bool visit = false;
      float dq   = 0.f;
      if (l < a.L) {
        dq    = bc_l2(qs, a.R + l * a.dim, a.dim);
        visit = a.indptr[l + 1] > a.indptr[l] && !bc_below(dq, a.radius[l], bound, a.c);
      }
      unsigned long long todo = __ballot(visit);
      while (todo != 0) {  // wave-uniform
        const int j = __builtin_ctzll(todo);
        todo &= todo - 1;
        const float dql   = __shfl(dq, j, kWave);
        const int64_t beg = a.indptr[l0 + j], n = a.indptr[l0 + j + 1] - beg;
        int64_t w0, w1;
        bc_window(a.dists + beg, n, lane, dql, bound, a.c, &w0, &w1);
        n_visited += 1;
        n_scored += (unsigned long long)(w1 - w0);
        n_skipped += (unsigned long long)(n - (w1 - w0));
        for (int64_t i0 = w0; i0 < w1; i0 += kWave) {
          const int64_t i = i0 + lane;
          const bool in   = i < w1 && bc_l2_acc(qs, a.X + (beg + i) * a.dim, a.dim) <= a.eps2;
          const unsigned long long bal = __ballot(in);
          if (in) {
            if constexpr (MODE == kEpsDense) {
              if (a.adj != nullptr) a.adj[qi * a.m + a.cols[beg + i]] = 1;
            }
            if constexpr (MODE == kEpsCollect) {
              const int64_t at = cnt + __builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0u));
              a.tmp[tbase + at] = ((unsigned long long)a.cols[beg + i] << 32) | (unsigned long long)(unsigned)(beg + i);
            }
          }
          cnt += __popcll(bal);
        }
      }
    }
    if constexpr (MODE != kEpsCollect) {
      if (lane == 0) a.deg[qi] = cnt;
    } else {
      // the row's pairs by ascending id: LSD radix sort, a byte of the id per pass, between the two scratch buffers
      unsigned long long* src = a.tmp + tbase;
      unsigned long long* dst = a.tmp2 + tbase;
      for (int pass = 0; pass < a.id_bytes; ++pass) {
        const int shift = 32 + 8 * pass;
        __syncthreads();  // src is written
#pragma unroll
        for (int u = 0; u < 4; ++u) hist[lane * 4 + u] = 0;
        __syncthreads();
        for (int64_t i = lane; i < cnt; i += kWave) atomicAdd(&hist[(unsigned)(src[i] >> shift) & 255u], 1u);
        __syncthreads();
        unsigned c4[4], sum = 0;
#pragma unroll
        for (int u = 0; u < 4; ++u) { c4[u] = hist[lane * 4 + u]; sum += c4[u]; }
        unsigned incl = sum;
#pragma unroll
        for (int o = 1; o < kWave; o <<= 1) {
          const unsigned v = __shfl_up(incl, o, kWave);
          if (lane >= o) incl += v;
        }
        unsigned run = incl - sum;
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 4; ++u) { hist[lane * 4 + u] = run; run += c4[u]; }
        __syncthreads();
        for (int64_t i0 = 0; i0 < cnt; i0 += kWave) {  // wave-uniform; 64 pairs keep their order inside a digit
          const int64_t i = i0 + lane;
          const bool ok   = i < cnt;
          const unsigned long long e = ok ? src[i] : 0ull;
          const unsigned d = (unsigned)(e >> shift) & 255u;
          unsigned long long same = __ballot(ok);
#pragma unroll
          for (int bit = 0; bit < 8; ++bit) {
            const unsigned long long bb = __ballot(ok && ((d >> bit) & 1u));
            same &= ((d >> bit) & 1u) ? bb : ~bb;
          }
          const unsigned before = __builtin_amdgcn_mbcnt_hi((unsigned)(same >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)same, 0u));
          const unsigned total  = (unsigned)__popcll(same);
          const unsigned base   = ok ? hist[d] : 0u;
          __syncthreads();
          if (ok) {
            dst[base + before] = e;
            if (before + 1 == total) hist[d] = base + total;
          }
          __syncthreads();
        }
        unsigned long long* t = src; src = dst; dst = t;
      }
      __syncthreads();
      const int64_t obase = a.off[qi], cap = a.off[qi + 1] - obase;
      const int64_t keep  = cnt < cap ? cnt : cap;
      for (int64_t i = lane; i < keep; i += kWave) {
        const unsigned long long e = src[i];
        a.indices[obase + i] = (int64_t)(e >> 32);
        if (a.distances != nullptr) a.distances[obase + i] = bc_l2_acc(qs, a.X + (int64_t)(unsigned)e * a.dim, a.dim);
      }
    }
  }
  if (lane == 0 && a.stats != nullptr) {
    atomicAdd(a.stats + 0, n_visited);
    atomicAdd(a.stats + 1, n_scored);
    atomicAdd(a.stats + 2, n_skipped);
  }
}

// ---------------------------------------------------------------- build
__global__ void bc_gather_kernel(const float* __restrict__ src, const int64_t* __restrict__ rows, int64_t n, int64_t dim, float* __restrict__ dst)
{
  const int64_t total = n * dim;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = e / dim;
    dst[e] = src[rows[r] * dim + (e - r * dim)];
  }
}

// every row to its nearest landmark by (distance, landmark): landmarks in ascending order, a strict comparison
template <int METRIC>
__global__ __launch_bounds__(256) void bc_assign_kernel(const float* __restrict__ X, const float* __restrict__ R, int64_t m, int64_t L, int dim,
                                                        uint32_t* __restrict__ label, float* __restrict__ dist)
{
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x) {
    float x[B::kMaxEpsDim];
    for (int t = 0; t < dim; ++t) x[t] = X[i * dim + t];
    float best = __builtin_inff();
    uint32_t arg = 0;
    for (int64_t l = 0; l < L; ++l) {
      const float d = bc_dist<METRIC>(x, R + l * dim, dim);
      if (d < best) { best = d; arg = (uint32_t)l; }
    }
    label[i] = arg;
    dist[i]  = best;
  }
}

// ---------------------------------------------------------------- host side
// fp32 [rows, cols] on the device
const float* f32_rows(DLManagedTensor* t, const char* what, int64_t* rows, int64_t* cols)
{
  const H::tensor_desc d = desc_of(t);
  if (!d.present) H::refuse("ball cover: %s must not be NULL", what);
  if (d.ndim != 2) H::refuse("ball cover: %s must be a 2-D matrix", what);
  if (!(d.code == 2 && d.bits == 32 && d.lanes == 1)) H::refuse("ball cover: %s must be fp32 (fp16 and fp64 rows are not supported)", what);
  H::check_placed(d, what);
  *rows = d.shape[0];
  *cols = d.shape[1];
  return static_cast<const float*>(dl_data(t->dl_tensor));
}

void* out_matrix(DLManagedTensor* t, const char* what, int64_t rows, int64_t cols, int code, int bits)
{
  const H::tensor_desc d = desc_of(t);
  if (!d.present) H::refuse("ball cover: %s must not be NULL", what);
  if (!(d.code == code && d.bits == bits && d.lanes == 1)) H::refuse("ball cover: %s must be %s", what, code == 0 ? "int64" : "fp32");
  if (d.ndim != 2 || d.shape[0] != rows || d.shape[1] != cols)
    H::refuse("ball cover: %s must have shape [%lld, %lld]", what, (long long)rows, (long long)cols);
  H::check_placed(d, what);
  return dl_data(t->dl_tensor);
}

bc_index& get_index(cuvsAmdBallCoverIndex_t h)
{
  CUVS_EXPECTS(h != nullptr && h->addr != 0, "the ball cover index has not been built");
  return *reinterpret_cast<bc_index*>(h->addr);
}

unsigned wave_grid(const resources& res, int64_t n) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(n, (int64_t)res.num_cus * 32)); }

std::unique_ptr<bc_index> bc_build(resources& res, const cuvsAmdBallCoverIndexParams& p, DLManagedTensor* dataset)
{
  int64_t m = 0, dim = 0;
  const H::tensor_desc d = desc_of(dataset);
  if (d.present && d.ndim == 2) B::check_build((int)p.metric, d.shape[0], d.shape[1], (int64_t)p.n_landmarks);  // the metric first
  const float* X = f32_rows(dataset, "dataset", &m, &dim);
  B::check_build((int)p.metric, m, dim, (int64_t)p.n_landmarks);
  auto idx    = std::make_unique<bc_index>();
  idx->metric = (int)p.metric;
  idx->m      = m;
  idx->dim    = dim;
  idx->L      = B::landmarks_of(m, (int64_t)p.n_landmarks);
  const int64_t L = idx->L;

  const std::vector<int64_t> rrows = B::draw_landmarks(m, L, p.seed);
  idx->rrows = dev_buf<int64_t>::persistent((size_t)L);
  idx->R     = dev_buf<float>::persistent((size_t)(L * dim));
  copy_async(res, idx->rrows.data(), rrows.data(), (size_t)L * sizeof(int64_t));
  hipLaunchKernelGGL(bc_gather_kernel, dim3(wave_grid(res, (L * dim + 255) / 256)), dim3(256), 0, res.stream, X, idx->rrows.data(), L, dim,
                     idx->R.data());
  HIP_TRY(hipGetLastError());

  dev_buf<uint32_t> label(res, (size_t)m);
  dev_buf<float> dist(res, (size_t)m);
  profile_begin(res, "bc_assign_kernel");
  if (idx->metric == B::kHaversine)
    hipLaunchKernelGGL(bc_assign_kernel<kHav>, dim3(wave_grid(res, (m + 255) / 256)), dim3(256), 0, res.stream, X, idx->R.data(), m, L, (int)dim,
                       label.data(), dist.data());
  else
    hipLaunchKernelGGL(bc_assign_kernel<kL2>, dim3(wave_grid(res, (m + 255) / 256)), dim3(256), 0, res.stream, X, idx->R.data(), m, L, (int)dim,
                       label.data(), dist.data());
  profile_end(res, "bc_assign_kernel");
  HIP_TRY(hipGetLastError());
  const std::vector<uint32_t> h_label = to_host(res, label.data(), (size_t)m);
  const std::vector<float> h_dist     = to_host(res, dist.data(), (size_t)m);

  std::vector<int64_t> h_indptr((size_t)L + 1), h_cols((size_t)m);
  std::vector<float> h_sdist((size_t)m), h_radius((size_t)L);
  B::order_lists(h_label.data(), h_dist.data(), m, L, h_indptr.data(), h_cols.data(), h_sdist.data(), h_radius.data());

  idx->indptr = dev_buf<int64_t>::persistent((size_t)L + 1);
  idx->cols   = dev_buf<int64_t>::persistent((size_t)m);
  idx->dists  = dev_buf<float>::persistent((size_t)m);
  idx->radius = dev_buf<float>::persistent((size_t)L);
  idx->X      = dev_buf<float>::persistent((size_t)(m * dim));
  copy_async(res, idx->indptr.data(), h_indptr.data(), ((size_t)L + 1) * sizeof(int64_t));
  copy_async(res, idx->cols.data(), h_cols.data(), (size_t)m * sizeof(int64_t));
  copy_async(res, idx->dists.data(), h_sdist.data(), (size_t)m * sizeof(float));
  copy_async(res, idx->radius.data(), h_radius.data(), (size_t)L * sizeof(float));
  hipLaunchKernelGGL(bc_gather_kernel, dim3(wave_grid(res, (m * dim + 255) / 256)), dim3(256), 0, res.stream, X, idx->cols.data(), m, dim,
                     idx->X.data());
  HIP_TRY(hipGetLastError());
  sync(res);  // the host arrays and the caller's rows have been read
  return idx;
}

void read_stats(resources& res, const unsigned long long* d_stats, int64_t nq)
{
  const std::vector<unsigned long long> h = to_host(res, d_stats, 3);
  g_bc_stats[0] = h[0];
  g_bc_stats[1] = h[1];
  g_bc_stats[2] = h[2];
  g_bc_stats[3] = (uint64_t)nq;
}

template <int METRIC, int DIM>
void launch_knn(resources& res, const bc_knn_args& a)
{
  const dim3 grid(wave_grid(res, a.nq)), block(kWave);
  if (a.k <= 64) hipLaunchKernelGGL((bc_knn_kernel<METRIC, DIM, 1>), grid, block, 0, res.stream, a);
  else if (a.k <= 128) hipLaunchKernelGGL((bc_knn_kernel<METRIC, DIM, 2>), grid, block, 0, res.stream, a);
  else hipLaunchKernelGGL((bc_knn_kernel<METRIC, DIM, 4>), grid, block, 0, res.stream, a);
}

void bc_knn(resources& res, const bc_index& idx, const float* queries, int64_t nq, int64_t qdim, DLManagedTensor* neighbors,
            DLManagedTensor* distances, bool post_filter, float weight)
{
  const H::tensor_desc dn = desc_of(neighbors);
  const int64_t k = dn.present && dn.ndim == 2 ? dn.shape[1] : 0;
  B::check_knn(idx.metric, idx.dim, qdim, k, idx.L, weight);
  bc_knn_args a{};
  a.out_ids   = static_cast<int64_t*>(out_matrix(neighbors, "neighbors", nq, k, 0, 64));
  a.out_dists = static_cast<float*>(out_matrix(distances, "distances", nq, k, 2, 32));
  g_bc_stats[0] = g_bc_stats[1] = g_bc_stats[2] = g_bc_stats[3] = 0;
  if (nq == 0) return;
  a.X = idx.X.data(); a.R = idx.R.data(); a.dists = idx.dists.data(); a.radius = idx.radius.data();
  a.indptr = idx.indptr.data(); a.cols = idx.cols.data();
  a.queries = queries; a.nq = nq; a.L = idx.L; a.k = (int)k;
  a.post_filter = post_filter ? 1 : 0;
  a.weight = weight;
  a.c      = B::margin_of(idx.metric);
  a.s      = B::slack_of(idx.metric);
  dev_buf<unsigned long long> stats(res, 3);
  HIP_TRY(hipMemsetAsync(stats.data(), 0, 3 * sizeof(unsigned long long), res.stream));
  a.stats = stats.data();
  profile_begin(res, "bc_knn_kernel");
  if (idx.metric == B::kHaversine) launch_knn<kHav, 2>(res, a);
  else if (idx.dim == 2) launch_knn<kL2, 2>(res, a);
  else launch_knn<kL2, 3>(res, a);
  profile_end(res, "bc_knn_kernel");
  HIP_TRY(hipGetLastError());
  read_stats(res, stats.data(), nq);
}

bc_eps_args eps_args(const bc_index& idx, const float* queries, int64_t nq, float eps)
{
  bc_eps_args a{};
  a.X = idx.X.data(); a.R = idx.R.data(); a.dists = idx.dists.data(); a.radius = idx.radius.data();
  a.indptr = idx.indptr.data(); a.cols = idx.cols.data();
  a.queries = queries; a.nq = nq; a.L = idx.L; a.m = idx.m; a.dim = (int)idx.dim;
  a.eps  = eps;
  a.eps2 = eps * eps;
  a.c    = B::margin_of(idx.metric);
  int bytes = 1;
  while (bytes < 4 && ((uint64_t)(idx.m - 1) >> (8 * bytes)) != 0) ++bytes;
  a.id_bytes = bytes;
  return a;
}

// degrees of every query on the host
std::vector<int64_t> eps_degrees(resources& res, bc_eps_args a, uint8_t* adj)
{
  std::vector<int64_t> h((size_t)a.nq + 1, 0);
  if (a.nq == 0) return h;
  dev_buf<int64_t> deg(res, (size_t)a.nq);
  a.deg = deg.data();
  a.adj = adj;
  profile_begin(res, "bc_eps_kernel");
  if (adj != nullptr) hipLaunchKernelGGL(bc_eps_kernel<kEpsDense>, dim3(wave_grid(res, a.nq)), dim3(kWave), 0, res.stream, a);
  else hipLaunchKernelGGL(bc_eps_kernel<kEpsCount>, dim3(wave_grid(res, a.nq)), dim3(kWave), 0, res.stream, a);
  profile_end(res, "bc_eps_kernel");
  HIP_TRY(hipGetLastError());
  copy_async(res, h.data(), deg.data(), (size_t)a.nq * sizeof(int64_t));
  sync(res);
  return h;
}

void bc_eps_dense(resources& res, const bc_index& idx, const float* queries, int64_t nq, uint8_t* adj, void* vd, int vd_bytes, float eps)
{
  g_bc_stats[0] = g_bc_stats[1] = g_bc_stats[2] = g_bc_stats[3] = 0;
  if (adj == nullptr && vd == nullptr) return;
  bc_eps_args a = eps_args(idx, queries, nq, eps);
  dev_buf<unsigned long long> stats(res, 3);
  HIP_TRY(hipMemsetAsync(stats.data(), 0, 3 * sizeof(unsigned long long), res.stream));
  a.stats = stats.data();
  if (adj != nullptr && nq > 0) HIP_TRY(hipMemsetAsync(adj, 0, (size_t)nq * (size_t)idx.m, res.stream));
  std::vector<int64_t> h = eps_degrees(res, a, adj);
  int64_t edges = 0;
  for (int64_t i = 0; i < nq; ++i) edges += h[(size_t)i];
  h[(size_t)nq] = edges;
  if (vd != nullptr) {
    if (vd_bytes == 8) {
      copy_async(res, vd, h.data(), ((size_t)nq + 1) * sizeof(int64_t));
    } else {
      std::vector<int32_t> h32(h.begin(), h.end());
      copy_async(res, vd, h32.data(), ((size_t)nq + 1) * sizeof(int32_t));
    }
    sync(res);
  }
  read_stats(res, stats.data(), nq);
}

void bc_eps_csr(resources& res, const bc_index& idx, const float* queries, int64_t nq, int64_t* indptr, int64_t* indices, int64_t indices_len,
                float* distances, int64_t distances_len, int64_t* vd, float eps, int64_t* max_k)
{
  g_bc_stats[0] = g_bc_stats[1] = g_bc_stats[2] = g_bc_stats[3] = 0;
  const bool one_call = max_k != nullptr, fill = indices != nullptr;
  const int64_t cap = one_call ? *max_k : -1;
  std::vector<int64_t> h_indptr;
  if (one_call) {
    H::check_max_k(cap, nq, indices_len, distances_len, distances != nullptr);
  } else if (fill) {
    h_indptr = to_host(res, indptr, (size_t)nq + 1);
    H::check_fill(h_indptr.data(), nq, indices_len, distances_len, distances != nullptr);
  }
  bc_eps_args a = eps_args(idx, queries, nq, eps);
  dev_buf<unsigned long long> stats(res, 3);
  HIP_TRY(hipMemsetAsync(stats.data(), 0, 3 * sizeof(unsigned long long), res.stream));
  a.stats = stats.data();
  std::vector<int64_t> h_deg = eps_degrees(res, a, nullptr);
  read_stats(res, stats.data(), nq);  // the counters of the count pass (the fill walks the same lists again)
  a.stats = nullptr;

  if (!fill || one_call) {  // the offsets this call writes
    std::vector<int64_t> h_off((size_t)nq + 1);
    H::offsets_from_counts(h_deg.data(), nq, cap, 0, h_off.data());
    copy_async(res, indptr, h_off.data(), ((size_t)nq + 1) * sizeof(int64_t));
    sync(res);
  }
  if (fill && nq > 0) {
    std::vector<int64_t> h_tmp((size_t)nq + 1);
    for (int64_t r0 = 0; r0 < nq;) {
      const int64_t r1 = B::slab_end(h_deg.data(), nq, r0, (int64_t)res.workspace_limit), rows = r1 - r0;
      H::offsets_from_counts(h_deg.data() + r0, rows, -1, 0, h_tmp.data());
      const int64_t edges = h_tmp[(size_t)rows];
      dev_buf<int64_t> d_tmp_off(res, (size_t)rows + 1);
      dev_buf<unsigned long long> tmp(res, (size_t)std::max<int64_t>(edges, 1)), tmp2(res, (size_t)std::max<int64_t>(edges, 1));
      copy_async(res, d_tmp_off.data(), h_tmp.data(), ((size_t)rows + 1) * sizeof(int64_t));
      bc_eps_args s = a;
      s.queries   = queries + r0 * idx.dim;
      s.nq        = rows;
      s.tmp_off   = d_tmp_off.data();
      s.tmp       = tmp.data();
      s.tmp2      = tmp2.data();
      s.off       = indptr + r0;
      s.indices   = indices;
      s.distances = distances;
      profile_begin(res, "bc_eps_kernel_fill");
      hipLaunchKernelGGL(bc_eps_kernel<kEpsCollect>, dim3(wave_grid(res, rows)), dim3(kWave), 0, res.stream, s);
      profile_end(res, "bc_eps_kernel_fill");
      HIP_TRY(hipGetLastError());
      sync(res);  // (h_tmp is reused)
      r0 = r1;
    }
  }
  int64_t edges = 0;
  for (int64_t i = 0; i < nq; ++i) edges += h_deg[(size_t)i];
  if (vd != nullptr) {
    h_deg[(size_t)nq] = edges;
    copy_async(res, vd, h_deg.data(), ((size_t)nq + 1) * sizeof(int64_t));
    sync(res);
  }
  if (one_call) *max_k = H::largest_degree(h_deg.data(), nq);
}

}  // namespace
}  // namespace cuvs_amd

using namespace cuvs_amd;

extern "C" {

cuvsError_t cuvsAmdBallCoverIndexParamsCreate(cuvsAmdBallCoverIndexParams_t* params)
{
  return (cuvsError_t)translate_exceptions([=] { *params = new cuvsAmdBallCoverIndexParams{L2SqrtExpanded, 0, 0}; });
}
cuvsError_t cuvsAmdBallCoverIndexParamsDestroy(cuvsAmdBallCoverIndexParams_t params)
{
  return (cuvsError_t)translate_exceptions([=] { delete params; });
}
cuvsError_t cuvsAmdBallCoverIndexCreate(cuvsAmdBallCoverIndex_t* index)
{
  return (cuvsError_t)translate_exceptions([=] { *index = new cuvsAmdBallCoverIndex{0, DLDataType{kDLFloat, 32, 1}}; });
}
cuvsError_t cuvsAmdBallCoverIndexDestroy(cuvsAmdBallCoverIndex_t index)
{
  return (cuvsError_t)translate_exceptions([=] {
    if (!index) return;
    delete reinterpret_cast<bc_index*>(index->addr);
    delete index;
  });
}

cuvsError_t cuvsAmdBallCoverBuild(cuvsResources_t res_h, cuvsAmdBallCoverIndexParams_t params, DLManagedTensor* dataset,
                                  cuvsAmdBallCoverIndex_t index)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& res = *as_res(res_h);
    CUVS_EXPECTS(params != nullptr && index != nullptr, "params and index must not be NULL");
    std::unique_ptr<bc_index> built = bc_build(res, *params, dataset);
    delete reinterpret_cast<bc_index*>(index->addr);
    index->addr = reinterpret_cast<uintptr_t>(built.release());
  });
}

cuvsError_t cuvsAmdBallCoverKnnQuery(cuvsResources_t res_h, cuvsAmdBallCoverIndex_t index, DLManagedTensor* queries,
                                     DLManagedTensor* neighbors, DLManagedTensor* distances, bool perform_post_filtering, float weight)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& res           = *as_res(res_h);
    const bc_index& idx = get_index(index);
    int64_t nq = 0, qdim = 0;
    const float* q = f32_rows(queries, "queries", &nq, &qdim);
    bc_knn(res, idx, q, nq, qdim, neighbors, distances, perform_post_filtering, weight);
  });
}

cuvsError_t cuvsAmdBallCoverAllKnnQuery(cuvsResources_t res_h, cuvsAmdBallCoverIndexParams_t params, DLManagedTensor* dataset,
                                        DLManagedTensor* neighbors, DLManagedTensor* distances, bool perform_post_filtering, float weight,
                                        cuvsAmdBallCoverIndex_t index_out)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& res = *as_res(res_h);
    CUVS_EXPECTS(params != nullptr, "params must not be NULL");
    // the arguments of the query are checked before the build is paid for
    const H::tensor_desc dd = desc_of(dataset), dn = desc_of(neighbors);
    if (dd.present && dd.ndim == 2 && dn.present && dn.ndim == 2) {
      B::check_build((int)params->metric, dd.shape[0], dd.shape[1], (int64_t)params->n_landmarks);
      B::check_knn((int)params->metric, dd.shape[1], dd.shape[1], dn.shape[1], B::landmarks_of(dd.shape[0], (int64_t)params->n_landmarks),
                   weight);
    }
    std::unique_ptr<bc_index> built = bc_build(res, *params, dataset);
    int64_t nq = 0, qdim = 0;
    const float* q = f32_rows(dataset, "dataset", &nq, &qdim);
    bc_knn(res, *built, q, nq, qdim, neighbors, distances, perform_post_filtering, weight);
    if (index_out != nullptr) {
      delete reinterpret_cast<bc_index*>(index_out->addr);
      index_out->addr = reinterpret_cast<uintptr_t>(built.release());
    }
  });
}

cuvsError_t cuvsAmdBallCoverEpsNn(cuvsResources_t res_h, cuvsAmdBallCoverIndex_t index, DLManagedTensor* queries, DLManagedTensor* adj,
                                  DLManagedTensor* vd, float eps)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& res           = *as_res(res_h);
    const bc_index& idx = get_index(index);
    if (idx.metric == B::kHaversine) B::check_eps(idx.metric, idx.dim, idx.dim, eps);
    int64_t nq = 0, qdim = 0;
    const float* q = f32_rows(queries, "queries", &nq, &qdim);
    B::check_eps(idx.metric, idx.dim, qdim, eps);
    H::check_adj(desc_of(adj), nq, idx.m);
    const int vd_bytes = H::check_row_vector(desc_of(vd), nq, "vd", true, idx.m);
    bc_eps_dense(res, idx, q, nq, adj ? static_cast<uint8_t*>(dl_data(adj->dl_tensor)) : nullptr, vd ? dl_data(vd->dl_tensor) : nullptr,
                 vd_bytes, eps);
  });
}

cuvsError_t cuvsAmdBallCoverEpsNnCsr(cuvsResources_t res_h, cuvsAmdBallCoverIndex_t index, DLManagedTensor* queries, DLManagedTensor* indptr,
                                     DLManagedTensor* indices, DLManagedTensor* distances, DLManagedTensor* vd, float eps, int64_t* max_k)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& res           = *as_res(res_h);
    const bc_index& idx = get_index(index);
    if (idx.metric == B::kHaversine) B::check_eps(idx.metric, idx.dim, idx.dim, eps);
    int64_t nq = 0, qdim = 0;
    const float* q = f32_rows(queries, "queries", &nq, &qdim);
    B::check_eps(idx.metric, idx.dim, qdim, eps);
    if (indptr == nullptr) H::refuse("indptr must not be NULL");
    H::check_row_vector(desc_of(indptr), nq, "indptr", false, idx.m);
    H::check_row_vector(desc_of(vd), nq, "vd", false, idx.m);
    if (indices == nullptr && max_k != nullptr) H::refuse("the max_k form needs indices");
    if (indices == nullptr && distances != nullptr) H::refuse("distances need indices");
    const int64_t ilen = indices ? H::check_list(desc_of(indices), "indices", false) : 0;
    const int64_t dlen = distances ? H::check_list(desc_of(distances), "distances", true) : 0;
    bc_eps_csr(res, idx, q, nq, static_cast<int64_t*>(dl_data(indptr->dl_tensor)),
               indices ? static_cast<int64_t*>(dl_data(indices->dl_tensor)) : nullptr, ilen,
               distances ? static_cast<float*>(dl_data(distances->dl_tensor)) : nullptr, dlen,
               vd ? static_cast<int64_t*>(dl_data(vd->dl_tensor)) : nullptr, eps, max_k);
  });
}

cuvsError_t cuvsAmdBallCoverIndexGetNLandmarks(cuvsAmdBallCoverIndex_t index, int64_t* n_landmarks)
{
  return (cuvsError_t)translate_exceptions([=] { *n_landmarks = get_index(index).L; });
}
cuvsError_t cuvsAmdBallCoverIndexGetSize(cuvsAmdBallCoverIndex_t index, int64_t* m)
{
  return (cuvsError_t)translate_exceptions([=] { *m = get_index(index).m; });
}
cuvsError_t cuvsAmdBallCoverIndexGetDim(cuvsAmdBallCoverIndex_t index, int64_t* dim)
{
  return (cuvsError_t)translate_exceptions([=] { *dim = get_index(index).dim; });
}
cuvsError_t cuvsAmdBallCoverIndexGetMetric(cuvsAmdBallCoverIndex_t index, cuvsDistanceType* metric)
{
  return (cuvsError_t)translate_exceptions([=] { *metric = (cuvsDistanceType)get_index(index).metric; });
}

cuvsError_t cuvsAmdBallCoverIndexGetArray(cuvsAmdBallCoverIndex_t index, cuvsAmdBallCoverArray which, DLManagedTensor* out)
{
  return (cuvsError_t)translate_exceptions([=] {
    const bc_index& idx = get_index(index);
    const DLDataType f32{kDLFloat, 32, 1}, i64{kDLInt, 64, 1};
    int device = 0;
    HIP_TRY(hipGetDevice(&device));
    switch (which) {
      case CUVS_AMD_BALL_COVER_R_INDPTR: fill_dl_view(out, idx.indptr.data(), i64, idx.L + 1, 1, 1, device); break;
      case CUVS_AMD_BALL_COVER_R_1NN_COLS: fill_dl_view(out, idx.cols.data(), i64, idx.m, 1, 1, device); break;
      case CUVS_AMD_BALL_COVER_R_1NN_DISTS: fill_dl_view(out, idx.dists.data(), f32, idx.m, 1, 1, device); break;
      case CUVS_AMD_BALL_COVER_R_RADIUS: fill_dl_view(out, idx.radius.data(), f32, idx.L, 1, 1, device); break;
      case CUVS_AMD_BALL_COVER_R: fill_dl_view(out, idx.R.data(), f32, idx.L, idx.dim, 2, device); break;
      case CUVS_AMD_BALL_COVER_X_REORDERED: fill_dl_view(out, idx.X.data(), f32, idx.m, idx.dim, 2, device); break;
      case CUVS_AMD_BALL_COVER_R_ROWS: fill_dl_view(out, idx.rrows.data(), i64, idx.L, 1, 1, device); break;
      default: CUVS_FAIL("unknown ball cover array %d", (int)which);
    }
  });
}

cuvsError_t cuvsAmdBallCoverLastStats(uint64_t out[4])
{
  return (cuvsError_t)translate_exceptions([=] {
    CUVS_EXPECTS(out != nullptr, "out is null");
    for (int i = 0; i < 4; ++i) out[i] = g_bc_stats[i];
  });
}

}  // extern "C"
