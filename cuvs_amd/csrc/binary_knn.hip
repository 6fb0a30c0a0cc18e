// Exact Hamming kNN and Hamming distance matrices over packed bit codes (include/cuvs_amd/binary_knn.h). DESIGN 3.1zc.
//
// hamming(a, b) = popcount(a) + popcount(b) - 2 a.b, and a.b over 0/1 vectors is an exact integer product:
// v_mfma_i32_32x32x32_i8 computes it. The codes stay packed in memory; they are expanded to 0/1 bytes on the way to the matrix
// core, and the design is about what that expansion costs: 16 bits -> one operand register quad is ~14 VALU instructions, about
// the issue time of one MFMA, so every expanded operand has to feed several MFMAs.
//   * A workgroup (256 threads) owns kBQ = 128 queries and one column split of the dataset rows. Its queries are expanded ONCE
//     into the LDS (128 x up to 1024 bit-dimensions as bytes, row pitch + 16 bytes: conflict-free 16-byte operand reads) and
//     stay there while the split's rows stream past. Rows longer than the resident part (kb bytes: 128, or 64 when the top-k
//     lists need the room) are done in `stages`: the queries are then re-staged for every group of 256 rows.
//   * A wave takes kR = 2 tiles of 32 rows at a time. A lane reads 16 bytes of its row's packed code straight from global memory
//     (each code is read once per 128 queries), and per 32-dimension slice expands its 16 bits in registers (bk_expand16) into
//     the B operand. That one operand meets the four A operands of the 4 x 32 queries from the LDS: four MFMAs per expansion,
//     and every A operand read from the LDS serves both row tiles. 2 x 4 x 16 int32 accumulators per lane.
//   * Operand maps (coarse_lowp.hip): lane (li = lane & 31, h = lane >> 5) holds row li, K bytes [16 h, 16 h + 16) of a 32-byte
//     K step; accumulator register i = query (i & 3) + 8 (i >> 2) + 4 h of the 32, row li.
//   * Tails add nothing: bytes past nbytes, rows past n and query slots past m are ZERO at the load (bk_load_word), and a zero
//     0/1 byte adds nothing to a product. int8 rows are read through uint8_t pointers.
// Epilogues: d = pcq + pcx - 2 acc in int32, then
//   store: (float)d into an fp32 tile - cuvsAmdBinaryPairwiseDistance, and the tile producer of brute_force.hip's per-tile
//          select path (bf_select_tiles: BITSET / BITMAP filter, select_k per column tile, merge) for k > 64 or any filter;
//   fused: k <= 64, no filter: per-query sorted lists of 64-bit keys d << 32 | id in the LDS with the k-th key as the admission
//          bound (fused_knn.hip's queue-and-insert scheme on integer keys: Hamming distances take at most 8 nbytes + 1 values,
//          so admission compares (distance, id), never the distance alone). Keys are unique, insertion keeps a list sorted, so the
//          result does not depend on the order the waves arrive in. Column splits are merged by select_k.
#include "common.hpp"
#include "device_utils.hpp"
#include "ops.hpp"

#include <cuvs_amd/binary_knn.h>

#include <algorithm>
#include <cfloat>
#include <climits>

namespace cuvs_amd {
namespace {

typedef int bk_i32x4 __attribute__((ext_vector_type(4)));
typedef int bk_i32x16 __attribute__((ext_vector_type(16)));
typedef unsigned long long bk_key;

constexpr int kThreads    = 256;
constexpr int kBQ         = 128;              // queries of a workgroup
constexpr int kR          = 2;                // 32-row tiles a wave holds accumulators for
constexpr int kGroupRows  = 4 * kR * 32;      // dataset rows of a workgroup's step
constexpr int kChunkBytes = 64;               // K chunk: 512 bit-dimensions
constexpr int kMaxStage   = 2 * kChunkBytes;  // most bytes of a query kept expanded in the LDS
constexpr int kFusedMaxK  = 64;
constexpr int kQueueCap   = 512;
constexpr bk_key kNoKey   = ~0ull;

// 16 bits -> 16 bytes of 0 / 1 (bit i to byte i): a nibble times 0x204081 puts its bits 0..3 at bits 0, 8, 16, 24
__device__ inline bk_i32x4 bk_expand16(const uint32_t h)
{
  bk_i32x4 r;
  r[0] = (int)((((h >> 0) & 15u) * 0x204081u) & 0x01010101u);
  r[1] = (int)((((h >> 4) & 15u) * 0x204081u) & 0x01010101u);
  r[2] = (int)((((h >> 8) & 15u) * 0x204081u) & 0x01010101u);
  r[3] = (int)((((h >> 12) & 15u) * 0x204081u) & 0x01010101u);
  return r;
}

// the four bytes at p of which `avail` exist (<= 0: none); the others are zero. al4: p is 4-byte aligned
__device__ inline uint32_t bk_load_word(const uint8_t* __restrict__ p, const int avail, const bool al4)
{
  if (avail >= 4 && al4) return *reinterpret_cast<const uint32_t*>(p);
  uint32_t w = 0u;
#pragma unroll
  for (int b = 0; b < 4; ++b)
    if (b < avail) w |= (uint32_t)p[b] << (8 * b);
  return w;
}

// ---------------------------------------------------------------- 1: row popcounts (eight lanes a row)
__global__ __launch_bounds__(kThreads) void bk_popcount_kernel(const uint8_t* __restrict__ x, int64_t n, int64_t ld, int nbytes, bool al4,
                                                                int32_t* __restrict__ out)
{
  const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x, row = t >> 3;
  const int sub = (int)(t & 7);
  int c = 0;
  if (row < n)
    for (int b = sub * 4; b < nbytes; b += 32) c += __popc(bk_load_word(x + row * ld + b, nbytes - b, al4));
  c += __shfl_xor(c, 1, kWave);
  c += __shfl_xor(c, 2, kWave);
  c += __shfl_xor(c, 4, kWave);
  if (row < n && sub == 0) out[row] = c;
}

// ---------------------------------------------------------------- 2: the tile kernel
struct bk_args {
  const uint8_t *q, *x;      // queries [m] and dataset rows [n], row pitches ldq / ldx bytes
  int64_t m, n, ldq, ldx;
  int nbytes;
  int kb, stages, pitch;     // bytes of K staged at a time (a multiple of 16), their number, LDS bytes per query (8 kb + 16)
  int q_al4, x_align;        // queries 4-byte aligned; dataset rows 16-, 4- or 1-byte aligned
  const int32_t *pcq, *pcx;  // popcounts
  int64_t groups_per_split;  // kGroupRows-row steps of a column split
  float* out;                // store: [m, n] with pitch ldo
  int64_t ldo;
  int k, kp, n_splits;       // fused: list length kp (a power of two, 16..64)
  float* out_d;              // fused: [m, n_splits, k]
  int64_t* out_i;
};

__device__ inline int bk_slot(const int aq, const int i, const int h) { return aq * 32 + (i & 3) + 8 * (i >> 2) + 4 * h; }

// VEC: every row start is 16-byte aligned and nbytes is a multiple of 16 - a step's codes are one 16-byte load
template <bool FUSED, bool VEC>
__global__ __launch_bounds__(kThreads) void bk_tile_kernel(const bk_args a)
{
  extern __shared__ __attribute__((aligned(16))) uint8_t dyn[];
  uint8_t* sq     = dyn;                                                  // [kBQ][pitch] the queries as 0/1 bytes
  int32_t* s_pcq  = reinterpret_cast<int32_t*>(dyn + (size_t)kBQ * a.pitch);  // [kBQ]
  int32_t* s_thr  = s_pcq + kBQ;  // [kBQ] fused: (k-th distance) - pcq, what px - 2 acc must not exceed (INT_MAX: list not full)
  bk_key* top     = reinterpret_cast<bk_key*>(s_thr + kBQ);               // fused: [kBQ][kp] sorted keys
  bk_key* bound   = top + kBQ * a.kp;                                     // [kBQ] the k-th key
  bk_key* q_key   = bound + kBQ;                                          // [kQueueCap]
  uint32_t* q_row = reinterpret_cast<uint32_t*>(q_key + kQueueCap);       // [kQueueCap] query slot
  int* q_cnt      = reinterpret_cast<int*>(q_row + kQueueCap);            // [3][2] count, "another round" flag

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, h = lane >> 5;
  const int64_t q0        = (int64_t)blockIdx.y * kBQ;
  const int64_t row_begin = (int64_t)blockIdx.x * a.groups_per_split * kGroupRows;
  const int64_t row_end   = min(a.n, row_begin + a.groups_per_split * kGroupRows);
  const int pitch         = a.pitch;

  if (tid < kBQ) s_pcq[tid] = q0 + tid < a.m ? a.pcq[q0 + tid] : 0;
  if constexpr (FUSED) {
    for (int t = tid; t < kBQ * a.kp; t += kThreads) top[t] = kNoKey;
    if (tid < kBQ) {
      bound[tid] = kNoKey;
      s_thr[tid] = q0 + tid < a.m ? INT_MAX : INT_MIN;  // (a slot past m admits nothing)
    }
    if (tid < 6) q_cnt[tid] = 0;
  }
  int rd = 0;  // rounds of the fused epilogue so far (workgroup-uniform)

  // stage st of the workgroup's queries: a thread expands a word (32 dimensions) into two 16-byte stores
  auto stage = [&](const int st) {
    const int b0 = st * a.kb, words = a.kb >> 2;
    for (int u = tid; u < kBQ * words; u += kThreads) {
      const int q = u / words, w = u - q * words, off = b0 + 4 * w;
      const int64_t row = q0 + q;
      const uint32_t v  = row < a.m ? bk_load_word(a.q + row * a.ldq + off, a.nbytes - off, a.q_al4 != 0) : 0u;
      bk_i32x4* dst = reinterpret_cast<bk_i32x4*>(sq + (size_t)q * pitch + (size_t)w * 32);
      dst[0] = bk_expand16(v & 0xffffu);
      dst[1] = bk_expand16(v >> 16);
    }
  };

  for (int64_t g0 = row_begin; g0 < row_end; g0 += kGroupRows) {
    bk_i32x16 acc[kR][4];
    int64_t rows[kR];
    bool rv[kR];
    const uint8_t* xp[kR];
#pragma unroll
    for (int r = 0; r < kR; ++r) {
      rows[r] = g0 + (wave * kR + r) * 32 + li;
      rv[r]   = rows[r] < row_end;
      xp[r]   = a.x + (rv[r] ? rows[r] : 0) * a.ldx;
#pragma unroll
      for (int aq = 0; aq < 4; ++aq) acc[r][aq] = bk_i32x16{};
    }
    // the rows' codes in steps of 16 bytes (four slices), the next step's loads in flight under this step's products
    uint32_t wn[kR][4];
    auto fetch = [&](const int off) {
#pragma unroll
      for (int r = 0; r < kR; ++r) {
        const int avail = rv[r] ? a.nbytes - off : 0;
        if constexpr (VEC) {
          uint4 v = make_uint4(0u, 0u, 0u, 0u);
          if (rv[r]) v = *reinterpret_cast<const uint4*>(xp[r] + off);
          wn[r][0] = v.x; wn[r][1] = v.y; wn[r][2] = v.z; wn[r][3] = v.w;
        } else if (a.x_align == 16 && avail >= 16) {
          const uint4 v = *reinterpret_cast<const uint4*>(xp[r] + off);
          wn[r][0] = v.x; wn[r][1] = v.y; wn[r][2] = v.z; wn[r][3] = v.w;
        } else {
#pragma unroll
          for (int t = 0; t < 4; ++t) wn[r][t] = bk_load_word(xp[r] + off + 4 * t, avail - 4 * t, a.x_align >= 4);
        }
      }
    };
    fetch(0);
    for (int off = 0; off < a.nbytes; off += 16) {
      const int st = off / a.kb, in_stage = off - st * a.kb;
      if (in_stage == 0 && (a.stages > 1 || g0 == row_begin)) {  // (workgroup-uniform) one stage: the queries stay resident
        __syncthreads();
        stage(st);
        __syncthreads();
      }
      uint32_t w[kR][4];
#pragma unroll
      for (int r = 0; r < kR; ++r)
#pragma unroll
        for (int t = 0; t < 4; ++t) w[r][t] = wn[r][t];
      if (off + 16 < a.nbytes) fetch(off + 16);
      // all four slices without a branch: past nbytes both operands are zero (the staged part is a multiple of 16 bytes)
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const uint8_t* ap = sq + (size_t)li * pitch + (size_t)in_stage * 8 + t * 32 + h * 16;
        bk_i32x4 av[4];
#pragma unroll
        for (int aq = 0; aq < 4; ++aq) av[aq] = *reinterpret_cast<const bk_i32x4*>(ap + (size_t)aq * 32 * pitch);
#pragma unroll
        for (int r = 0; r < kR; ++r) {
          const bk_i32x4 bv = bk_expand16((w[r][t] >> (16 * h)) & 0xffffu);
#pragma unroll
          for (int aq = 0; aq < 4; ++aq) acc[r][aq] = __builtin_amdgcn_mfma_i32_32x32x32_i8(av[aq], bv, acc[r][aq], 0, 0, 0);
        }
      }
    }

    if constexpr (!FUSED) {
#pragma unroll
      for (int r = 0; r < kR; ++r) {
        if (!rv[r]) continue;
        const int px = a.pcx[rows[r]];
#pragma unroll
        for (int aq = 0; aq < 4; ++aq)
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const int qb    = aq * 32 + 8 * g + 4 * h;  // slots of registers 4 g .. 4 g + 3
            const int4 pq   = *reinterpret_cast<const int4*>(&s_pcq[qb]);
            const int pq4[4] = {pq.x, pq.y, pq.z, pq.w};
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (q0 + qb + e < a.m) a.out[(q0 + qb + e) * a.ldo + rows[r]] = (float)(pq4[e] + px - 2 * acc[r][aq][4 * g + e]);
          }
      }
    } else {
      // ---- admission against the queries' bounds, queue, insert (fused_knn.hip's scheme, one row tile after the other)
#pragma unroll
      for (int r = 0; r < kR; ++r) {
        const int px = rv[r] ? a.pcx[rows[r]] : 0;
        // screen: candidate (aq, i) <-> bit aq * 16 + i is kept while its distance does not exceed the query's k-th distance
        unsigned long long pend = 0ull;
#pragma unroll
        for (int aq = 0; aq < 4; ++aq)
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const int4 th    = *reinterpret_cast<const int4*>(&s_thr[aq * 32 + 8 * g + 4 * h]);
            const int th4[4] = {th.x, th.y, th.z, th.w};
#pragma unroll
            for (int e = 0; e < 4; ++e)
              pend |= (unsigned long long)(px - 2 * acc[r][aq][4 * g + e] <= th4[e]) << (aq * 16 + 4 * g + e);
          }
        if (!rv[r]) pend = 0ull;
        auto key_of = [&](const int aq, const int i) -> bk_key {
          const int d = s_pcq[bk_slot(aq, i, h)] + px - 2 * acc[r][aq][i];
          return ((bk_key)(uint32_t)d << 32) | (uint32_t)rows[r];
        };
        for (;;) {
          // the counters rotate over three sets: the one of the round after this is cleared before this round's barrier (its
          // last readers passed the previous barrier), so a round in which nobody submits costs a single barrier
          int* cnt_now = q_cnt + 2 * (rd % 3);
          if (tid == 0) { q_cnt[2 * ((rd + 1) % 3)] = 0; q_cnt[2 * ((rd + 1) % 3) + 1] = 0; }
          ++rd;
          // every wave submits at most kQueueCap / 4 candidates per round, so the four reservations always fit
          int mine = 0;
          if (__ballot(pend != 0ull) != 0ull) {
#pragma unroll
            for (int aq = 0; aq < 4; ++aq)
#pragma unroll
              for (int i = 0; i < 16; ++i) {
                const unsigned long long bit = 1ull << (aq * 16 + i);
                if (pend & bit) {
                  if (key_of(aq, i) > bound[bk_slot(aq, i, h)]) pend &= ~bit;  // can never enter this query's list
                  else ++mine;
                }
              }
          }
          const int incl   = wave_inclusive_scan(mine);
          const int total  = __shfl(incl, 63, kWave);
          const int submit = min(total, kQueueCap / 4);
          if (submit > 0) {
            int base = 0;
            if (lane == 0) base = atomicAdd(&cnt_now[0], submit);
            base     = __shfl(base, 0, kWave);
            int rank = incl - mine;
#pragma unroll
            for (int aq = 0; aq < 4; ++aq)
#pragma unroll
              for (int i = 0; i < 16; ++i) {
                const unsigned long long bit = 1ull << (aq * 16 + i);
                if (pend & bit) {
                  if (rank < submit) {
                    q_key[base + rank] = key_of(aq, i);
                    q_row[base + rank] = (uint32_t)bk_slot(aq, i, h);
                    pend &= ~bit;
                  }
                  ++rank;
                }
              }
          }
          if (total > submit && lane == 0) cnt_now[1] = 1;  // this wave has candidates left for another round
          __syncthreads();
          const int cnt = min(cnt_now[0], kQueueCap);
          if (cnt == 0) break;  // (workgroup-uniform; nobody has anything left either)
          const bool more = cnt_now[1] != 0;
          // ---- drain: wave w inserts the entries of the query slots with slot % 4 == w
          for (int e0 = 0; e0 < cnt; e0 += 64) {
            const int e       = e0 + lane;
            const bool have   = e < cnt && ((q_row[e < cnt ? e : 0] & 3u) == (uint32_t)wave);
            const bk_key ek   = have ? q_key[e] : 0ull;
            const uint32_t er = have ? q_row[e] : 0u;
            unsigned long long mm = __ballot(have);
            while (mm != 0ull) {
              const int src = (int)__ffsll((long long)mm) - 1;
              mm &= mm - 1ull;
              const bk_key ck = ((bk_key)(uint32_t)__builtin_amdgcn_readlane((int)(ek >> 32), src) << 32) |
                                (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)ek, src);
              const uint32_t cr = (uint32_t)__builtin_amdgcn_readlane((int)er, src);
              bk_key lk = lane < a.kp ? top[cr * a.kp + lane] : kNoKey;
              const bk_key wk = ((bk_key)(uint32_t)__builtin_amdgcn_readlane((int)(lk >> 32), a.k - 1) << 32) |
                                (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)lk, a.k - 1);
              if (ck < wk) {  // (wave-uniform)
                const int pos       = __popcll(__ballot(lk < ck));
                const uint32_t uphi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(lk >> 32), 0x138, 0xf, 0xf, false);
                const uint32_t uplo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)lk, 0x138, 0xf, 0xf, false);
                if (lane > pos) lk = ((bk_key)uphi << 32) | uplo;
                else if (lane == pos) lk = ck;
                if (lane < a.kp) top[cr * a.kp + lane] = lk;
                if (lane == a.k - 1) {
                  bound[cr] = lk;
                  if (lk != kNoKey) s_thr[cr] = (int)(uint32_t)(lk >> 32) - s_pcq[cr];
                }
              }
            }
          }
          __syncthreads();
          if (!more) break;
        }
      }
    }
  }

  if constexpr (FUSED) {
    __syncthreads();
    for (int t = tid; t < kBQ * a.k; t += kThreads) {
      const int r = t / a.k, j = t - r * a.k;
      const int64_t row = q0 + r;
      if (row >= a.m) continue;
      const bk_key key = top[r * a.kp + j];
      const size_t o   = ((size_t)row * a.n_splits + blockIdx.x) * a.k + j;
      a.out_d[o] = key == kNoKey ? FLT_MAX : (float)(uint32_t)(key >> 32);
      a.out_i[o] = key == kNoKey ? (int64_t)-1 : (int64_t)(uint32_t)key;
    }
  }
}

// slots nothing real filled (the worst value: a row the filter removed, or padding) get the id of padding
// (all: an empty dataset - every slot is padding)
__global__ __launch_bounds__(kThreads) void bk_pad_ids_kernel(float* __restrict__ d, int64_t* __restrict__ ids, int64_t count, bool all)
{
  const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (t >= count) return;
  if (all) d[t] = FLT_MAX;
  if (all || d[t] == FLT_MAX) ids[t] = -1;
}

// ---------------------------------------------------------------- host side
struct bk_rows {
  const uint8_t* p = nullptr;
  int64_t rows = 0, ld = 0;
  int nbytes = 0;
  int align() const  // what every row start is aligned to
  {
    const uintptr_t bits = reinterpret_cast<uintptr_t>(p) | (uintptr_t)ld;
    return (bits & 15) == 0 ? 16 : ((bits & 3) == 0 ? 4 : 1);
  }
};

thread_local uint64_t g_stats[4] = {0, 0, 0, 0};

size_t bk_lds_bytes(int kb, bool fused, int kp)
{
  size_t b = (size_t)kBQ * (kb * 8 + 16) + 2 * kBQ * sizeof(int32_t);
  if (fused) b += (size_t)kBQ * kp * sizeof(bk_key) + kBQ * sizeof(bk_key) + kQueueCap * (sizeof(bk_key) + sizeof(uint32_t)) + 32;
  return b;
}

void bk_popcounts(resources& res, const bk_rows& x, int32_t* out)
{
  if (x.rows == 0) return;
  hipLaunchKernelGGL(bk_popcount_kernel, dim3(grid_blocks(x.rows * 8, kThreads)), dim3(kThreads), 0, res.stream, x.p, x.rows, x.ld, x.nbytes,
                     x.align() >= 4, out);
  HIP_TRY(hipGetLastError());
}

// One launch over queries x dataset rows (at most 65535 * kBQ queries). Launch heuristic: the grid is (column splits, query
// blocks of kBQ). A split is a run of kGroupRows-row steps; splits are cut so that query blocks x splits comes to about four
// workgroups per CU (never above: a rounded-up grid would leave a tail round nearly empty), so a handful of queries still
// fills the chip, while a split stays long enough to pay for expanding the queries once per workgroup. The fused epilogue
// writes [m, splits, k] partial lists; the store epilogue writes the tile. Returns the number of splits.
int64_t bk_splits(const resources& res, int64_t m, int64_t n, int64_t* groups_per_split)
{
  const int64_t qblocks = (m + kBQ - 1) / kBQ, groups = (n + kGroupRows - 1) / kGroupRows;
  int64_t splits        = std::max<int64_t>(1, std::min<int64_t>(groups, (4 * (int64_t)res.num_cus) / qblocks));
  *groups_per_split     = (groups + splits - 1) / splits;
  return (groups + *groups_per_split - 1) / *groups_per_split;
}

template <bool FUSED>
void bk_launch(resources& res, bk_args a, const bk_rows& q, const bk_rows& x, int64_t splits)
{
  a.q = q.p; a.m = q.rows; a.ldq = q.ld; a.x = x.p; a.n = x.rows; a.ldx = x.ld; a.nbytes = x.nbytes;
  a.q_al4 = q.align() >= 4; a.x_align = x.align();
  // as much of a query as the LDS holds beside the lists stays expanded: 128 bytes, else 64 (whole 16-byte steps)
  const int padded = (int)round_up(x.nbytes, 16);
  a.kb     = bk_lds_bytes(kMaxStage, FUSED, a.kp) <= res.lds_per_block ? kMaxStage : kChunkBytes;
  a.kb     = std::min(a.kb, padded);
  a.stages = (x.nbytes + a.kb - 1) / a.kb;
  a.pitch  = a.kb * 8 + 16;
  const size_t lds = bk_lds_bytes(a.kb, FUSED, a.kp);
  auto kern = (a.x_align == 16 && x.nbytes % 16 == 0) ? bk_tile_kernel<FUSED, true> : bk_tile_kernel<FUSED, false>;
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  profile_begin(res, FUSED ? "bk_tile_kernel_fused" : "bk_tile_kernel_store");
  hipLaunchKernelGGL(kern, dim3((unsigned)splits, (unsigned)((q.rows + kBQ - 1) / kBQ)), dim3(kThreads), lds, res.stream, a);
  profile_end(res, FUSED ? "bk_tile_kernel_fused" : "bk_tile_kernel_store");
  HIP_TRY(hipGetLastError());
  g_stats[0] = (uint64_t)splits;
  g_stats[1] = FUSED ? 1 : 0;
  g_stats[2] = (uint64_t)((x.nbytes + kChunkBytes - 1) / kChunkBytes);
  g_stats[3] = (uint64_t)a.stages;
}

constexpr int64_t kSlabQueries = int64_t(65535) * kBQ;  // queries of one launch (grid.y)

// out[i][j] = hamming(q[i], x[j]) for the given rows, pitch ldo
void bk_store_tile(resources& res, const bk_rows& q, const bk_rows& x, const int32_t* pcq, const int32_t* pcx, float* out, int64_t ldo)
{
  if (q.rows == 0 || x.rows == 0) return;
  for (int64_t r0 = 0; r0 < q.rows; r0 += kSlabQueries) {
    bk_rows qs = q;
    qs.p += r0 * q.ld;
    qs.rows = std::min(kSlabQueries, q.rows - r0);
    bk_args a{};
    a.pcq = pcq + r0; a.pcx = pcx; a.out = out + r0 * ldo; a.ldo = ldo; a.kp = 0;
    const int64_t splits = bk_splits(res, qs.rows, x.rows, &a.groups_per_split);
    bk_launch<false>(res, a, qs, x, splits);
  }
}

void bk_fused_knn(resources& res, const bk_rows& q, const bk_rows& x, const int32_t* pcq, const int32_t* pcx, int k, int64_t* neighbors,
                  float* distances)
{
  for (int64_t r0 = 0; r0 < q.rows; r0 += kSlabQueries) {
    bk_rows qs = q;
    qs.p += r0 * q.ld;
    qs.rows = std::min(kSlabQueries, q.rows - r0);
    bk_args a{};
    a.pcq = pcq + r0; a.pcx = pcx; a.k = k; a.kp = std::max(16, next_pow2(k));
    const int64_t splits = bk_splits(res, qs.rows, x.rows, &a.groups_per_split);
    a.n_splits = (int)splits;
    dev_buf<float> pd;
    dev_buf<int64_t> pi;
    if (splits > 1) {
      pd = dev_buf<float>(res, (size_t)qs.rows * splits * k);
      pi = dev_buf<int64_t>(res, (size_t)qs.rows * splits * k);
      a.out_d = pd.data(); a.out_i = pi.data();
    } else {
      a.out_d = distances + r0 * k; a.out_i = neighbors + r0 * k;
    }
    bk_launch<true>(res, a, qs, x, splits);
    // a split's list is sorted by (distance, id) and the splits are in id order: select_k's "earliest position wins" is (distance, id)
    if (splits > 1)
      select_k<int64_t, int64_t>(res, pd.data(), pi.data(), qs.rows, splits * k, splits * k, k, distances + r0 * k, neighbors + r0 * k, true);
  }
}

void binary_knn(resources& res, const bk_rows& x, const bk_rows& q, int k, int64_t* neighbors, float* distances, const uint32_t* bits,
                int filter_type)
{
  g_stats[0] = g_stats[1] = g_stats[2] = g_stats[3] = 0;
  const int64_t m = q.rows, n = x.rows;
  if (m == 0 || k == 0) return;
  auto pad = [&](bool all) {
    hipLaunchKernelGGL(bk_pad_ids_kernel, dim3(grid_blocks(m * k, kThreads)), dim3(kThreads), 0, res.stream, distances, neighbors,
                       m * (int64_t)k, all);
    HIP_TRY(hipGetLastError());
  };
  if (n == 0) return pad(true);
  dev_buf<int32_t> pcq(res, (size_t)m), pcx(res, (size_t)n);
  bk_popcounts(res, q, pcq.data());
  bk_popcounts(res, x, pcx.data());
  if (k <= kFusedMaxK && filter_type == NO_FILTER) {
    bk_fused_knn(res, q, x, pcq.data(), pcx.data(), k, neighbors, distances);
    return;
  }
  // fp32 tiles through the tiled brute force's per-tile select path, every row tile
  int64_t m_tile = 0, n_tile = 0;
  bf_tile_shape(res, m, n, k, &m_tile, &n_tile);
  const int64_t n_ct = (n + n_tile - 1) / n_tile, ldo = std::min(n_tile, n);
  dev_buf<float> tile(res, (size_t)m_tile * ldo), part_v;
  dev_buf<int64_t> part_i;
  if (n_ct > 1) {
    part_v = dev_buf<float>(res, (size_t)m_tile * n_ct * k);
    part_i = dev_buf<int64_t>(res, (size_t)m_tile * n_ct * k);
  }
  const std::vector<char> every((size_t)((m + m_tile - 1) / m_tile), 1);
  bf_select_tiles(res, m, n, k, true, m_tile, n_tile, tile.data(), ldo, every, nullptr, bits, filter_type, part_v.data(), part_i.data(),
                  [&](int64_t r0, int64_t mr, int64_t c0, int64_t nc, float* out, int64_t ld, const uint32_t*) {
                    bk_rows qs = q, xs = x;
                    qs.p += r0 * q.ld; qs.rows = mr;
                    xs.p += c0 * x.ld; xs.rows = nc;
                    bk_store_tile(res, qs, xs, pcq.data() + r0, pcx.data() + c0, out, ld);
                  },
                  neighbors, distances);
  pad(false);  // a row the filter removed came through with the worst value and its own id
}

// uint8 / int8 [rows, nbytes] on the device, last stride 1, row stride >= nbytes
bk_rows bk_check_rows(const DLManagedTensor* t, const char* what)
{
  CUVS_EXPECTS(t != nullptr, "%s must not be NULL", what);
  const DLTensor& s = t->dl_tensor;
  CUVS_EXPECTS(dtype_is(s.dtype, kDLUInt, 8) || dtype_is(s.dtype, kDLInt, 8),
               "%s must hold packed bit codes as uint8 or int8 rows (dtype code %d, %d bits)", what, (int)s.dtype.code, (int)s.dtype.bits);
  CUVS_EXPECTS(s.ndim == 2, "%s must be a 2-D matrix", what);
  CUVS_EXPECTS(is_device_accessible(s), "%s must be accessible on device memory", what);
  CUVS_EXPECTS(s.shape[0] >= 0 && s.shape[1] >= 1, "%s must have at least one byte per row", what);
  CUVS_EXPECTS(s.shape[1] < (int64_t(1) << 21), "%s has %lld bytes per row: 8 * nbytes must stay below 2^24", what, (long long)s.shape[1]);
  bk_rows r;
  r.p = static_cast<const uint8_t*>(dl_data(s));
  r.rows = s.shape[0]; r.nbytes = (int)s.shape[1]; r.ld = s.shape[1];
  if (s.strides != nullptr && s.shape[0] > 0) {
    CUVS_EXPECTS(s.shape[1] == 1 || s.strides[1] == 1, "%s must be row-major: its last stride must be 1", what);
    if (s.shape[0] > 1) {
      CUVS_EXPECTS(s.strides[0] >= s.shape[1], "%s must be row-major: its row stride is below its row length", what);
      r.ld = s.strides[0];
    }
  }
  return r;
}

void bk_check_pair(const DLManagedTensor* x, const DLManagedTensor* y, const char* nx, const char* ny, const bk_rows& rx, const bk_rows& ry)
{
  CUVS_EXPECTS(x->dl_tensor.dtype.code == y->dl_tensor.dtype.code, "%s and %s must have the same dtype (uint8 or int8)", nx, ny);
  CUVS_EXPECTS(rx.nbytes == ry.nbytes, "nbytes mismatch: %s has %d bytes per row, %s has %d", nx, rx.nbytes, ny, ry.nbytes);
}

// contiguous [rows, cols] on the device of the given type
void* bk_check_out(const DLManagedTensor* t, const char* what, uint8_t code, uint8_t bits, const char* type_name, int64_t rows, int64_t cols)
{
  CUVS_EXPECTS(t != nullptr, "%s must not be NULL", what);
  const DLTensor& s = t->dl_tensor;
  CUVS_EXPECTS(dtype_is(s.dtype, code, bits), "%s must be %s", what, type_name);
  CUVS_EXPECTS(is_device_accessible(s), "%s must be accessible on device memory", what);
  CUVS_EXPECTS(s.ndim == 2 && s.shape[0] == rows && (cols < 0 || s.shape[1] == cols), "%s must have shape [%lld, %lld]", what,
               (long long)rows, (long long)(cols < 0 ? s.shape[1] : cols));
  CUVS_EXPECTS(s.shape[0] == 0 || s.shape[1] == 0 || is_c_contiguous(s), "%s must be row-major and contiguous", what);
  return dl_data(s);
}

}  // namespace
}  // namespace cuvs_amd

using namespace cuvs_amd;

extern "C" {

cuvsError_t cuvsAmdBinaryKnn(cuvsResources_t res_h, DLManagedTensor* dataset, DLManagedTensor* queries, DLManagedTensor* neighbors,
                             DLManagedTensor* distances, cuvsFilter prefilter)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& res = *as_res(res_h);
    const bk_rows x = bk_check_rows(dataset, "dataset"), q = bk_check_rows(queries, "queries");
    bk_check_pair(dataset, queries, "dataset", "queries", x, q);
    CUVS_EXPECTS(x.rows < (int64_t(1) << 32) - 1, "dataset has %lld rows: n must be below 2^32 - 1", (long long)x.rows);
    auto* nb = static_cast<int64_t*>(bk_check_out(neighbors, "neighbors", kDLInt, 64, "int64", q.rows, -1));
    const int64_t k = neighbors->dl_tensor.shape[1];
    auto* ds = static_cast<float*>(bk_check_out(distances, "distances", kDLFloat, 32, "float32", q.rows, k));
    CUVS_EXPECTS(k < (int64_t(1) << 31), "k must be below 2^31");
    const uint32_t* bits = nullptr;
    if (prefilter.type != NO_FILTER) {
      CUVS_EXPECTS(prefilter.type == BITSET || prefilter.type == BITMAP, "unsupported prefilter type");
      CUVS_EXPECTS(prefilter.addr != 0, "prefilter tensor is null");
      auto& ft = reinterpret_cast<DLManagedTensor*>(prefilter.addr)->dl_tensor;
      CUVS_EXPECTS(dtype_is(ft.dtype, kDLUInt, 32) && is_device_accessible(ft), "prefilter must be a device uint32 tensor");
      bits = static_cast<const uint32_t*>(dl_data(ft));
    }
    binary_knn(res, x, q, (int)k, nb, ds, bits, (int)prefilter.type);
  });
}

cuvsError_t cuvsAmdBinaryPairwiseDistance(cuvsResources_t res_h, DLManagedTensor* x_t, DLManagedTensor* y_t, DLManagedTensor* out)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& res = *as_res(res_h);
    const bk_rows x = bk_check_rows(x_t, "x"), y = bk_check_rows(y_t, "y");
    bk_check_pair(x_t, y_t, "x", "y", x, y);
    auto* o = static_cast<float*>(bk_check_out(out, "out", kDLFloat, 32, "float32", x.rows, y.rows));
    g_stats[0] = g_stats[1] = g_stats[2] = g_stats[3] = 0;
    if (x.rows == 0 || y.rows == 0) return;
    dev_buf<int32_t> pcx(res, (size_t)x.rows), pcy(res, (size_t)y.rows);
    bk_popcounts(res, x, pcx.data());
    bk_popcounts(res, y, pcy.data());
    bk_store_tile(res, x, y, pcx.data(), pcy.data(), o, y.rows);
  });
}

cuvsError_t cuvsAmdBinaryKnnLastStats(cuvsResources_t res_h, uint64_t out[4])
{
  return (cuvsError_t)translate_exceptions([=] {
    (void)as_res(res_h);
    CUVS_EXPECTS(out != nullptr, "out is null");
    for (int i = 0; i < 4; ++i) out[i] = g_stats[i];
  });
}

}  // extern "C"
