// IVF-RaBitQ on MI355X: index build (rotation, 1-bit codes, extended codes, factors), the two-stage search - an exact integer
// screen of the 1-bit codes against quantized queries on v_mfma_i32_32x32x32_i8, then a re-score of the survivors from the
// extended codes - the reference's file layout and the C entry points (include/cuvs_amd/ivf_rabitq.h).
//
// Reference: cpp/include/cuvs/neighbors/ivf_rabitq.hpp, cpp/src/neighbors/ivf_rabitq/gpu_index/{quantizer_gpu.cu (codes and
// factors), ivf_gpu.cu (lists, file), searcher_gpu*.cu (search)}. Its search shares a per-query threshold between blocks through
// atomics in whatever order they run and drops candidates beyond a per-block cap; this one is a pure function of (index, queries,
// params): DESIGN.md 3.1s states the contract, tests/ivf_rabitq_ref.py restates it in numpy.
//
// Layout: all lists in flat arrays, a list starts at a multiple of 32 rows. Bit codes in tiles of 32 rows, [tile][word][row] uint32
// with dimension 32 w + i at bit i of word w: lane r of a half-wave reads word w of row r (128 contiguous bytes per half-wave) and
// expands its 16 bits into the 16 operand bytes of one MFMA K step. Short factors float4 per row, extended codes in the file's
// bit stream per row, extended factors float2 per row, ids uint32.
#include "ivf_common.hpp"
#include "ivf_lists.hpp"
#include "ivf_rabitq_host.hpp"

#include <cuvs_amd/ivf_rabitq.h>

#include <cfloat>
#include <map>
#include <mutex>

namespace cuvs_amd {

struct ivf_rabitq_index {
  int metric       = 0;
  uint32_t n_lists = 0, dim = 0;
  uint32_t D = 0, W = 0;  // padded dimension (multiple of 64), 32-bit words per row
  uint32_t ex = 0;        // extended bits per dimension (bits_per_dim - 1)
  uint32_t exb = 0;       // bytes of a row's extended code (D ex / 8)
  float t = 0.f;          // scaling factor of the extended codes
  int64_t size = 0, padded_rows = 0;
  dev_buf<float> centers;           // [n_lists, dim] (a built index only)
  dev_buf<float> centers_rot;       // [n_lists, D]
  dev_buf<float> center_rot_norms;  // [n_lists] canonical |c'|^2
  dev_buf<float> rotation;          // [D, D]
  dev_buf<uint32_t> bits;           // [padded_rows / 32, W, 32]
  dev_buf<float4> short_fac;        // [padded_rows] f_add, f_rescale, f_error, 0
  dev_buf<uint8_t> ex_codes;        // [padded_rows, exb]
  dev_buf<float2> ex_fac;           // [padded_rows] f_add_ex, f_rescale_ex
  dev_buf<uint32_t> ids;            // [padded_rows], 0xffffffff in the padding
  dev_buf<uint32_t> list_sizes, list_offsets;
  std::vector<uint32_t> h_list_sizes, h_list_offsets;
};

namespace {

typedef int rbq_i32x4 __attribute__((ext_vector_type(4)));
typedef int rbq_i32x16 __attribute__((ext_vector_type(16)));

constexpr int kRbqQPB   = 32;    // queries of a screen work item: the 32 A rows of one MFMA tile
constexpr float kRbqEps = 1.9f;  // quantizer_gpu.cu: kConstEpsilon

thread_local uint64_t g_last_stats[4] = {0, 0, 0, 0};

float rbq_scaling_factor(uint32_t D, uint32_t ex)
{
  static std::mutex mu;
  static std::map<std::pair<uint32_t, uint32_t>, float> cache;
  {
    std::lock_guard<std::mutex> lock(mu);
    auto it = cache.find({D, ex});
    if (it != cache.end()) return it->second;
  }
  // computed outside the lock (D 2^ex events per vector are sorted: seconds at D = 4096, ex = 8); two threads that miss at once
  // compute the same value twice
  const float t = rabitq_host::const_scaling_factor(D, ex);
  std::lock_guard<std::mutex> lock(mu);
  cache[{D, ex}] = t;
  return t;
}

// ------------------------------------------------------------------ build
__global__ void rbq_pad_rows_kernel(const float* __restrict__ in, int64_t n, uint32_t dim, uint32_t D, float* __restrict__ out)
{
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * D) return;
  const int64_t i  = t / D;
  const uint32_t j = (uint32_t)(t % D);
  out[t] = j < dim ? in[i * dim + j] : 0.f;
}

// slot[row] = flat position of the row: its list's offset + its rank among the list's rows in input order
__global__ void rbq_slots_kernel(const uint32_t* __restrict__ perm, const uint32_t* __restrict__ labels,
                                 const uint32_t* __restrict__ grp_off, const uint32_t* __restrict__ list_off, int64_t n,
                                 uint32_t* __restrict__ slot)
{
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const uint32_t row = perm[j], L = labels[row];
  slot[row] = list_off[L] + (uint32_t)(j - (int64_t)grp_off[L]);
}

struct rbq_encode_args {
  const float* xr;           // [cnt, D] rotated rows of this batch (input order)
  const uint32_t* labels;    // [cnt]
  const uint32_t* slot;      // [cnt]
  const float* centers_rot;  // [n_lists, D]
  int64_t cnt, r0;
  uint32_t D, W, ex, exb;
  float t;
  uint32_t* bits;
  float4* short_fac;
  uint8_t* ex_codes;
  float2* ex_fac;
  uint32_t* ids;
};

// One wave per row. Every sum: lane l adds the terms of dimensions l, l + 64, ... in that order, then the 64 partials are
// combined by the xor butterfly 32, 16, ..., 1 (wave_sum). Products and sums are separate roundings (-ffp-contract=off).
__global__ __launch_bounds__(256) void rbq_encode_kernel(rbq_encode_args a)
{
  extern __shared__ __attribute__((aligned(16))) uint8_t enc_smem[];  // [4][D] unpacked extended codes
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t i = (int64_t)blockIdx.x * 4 + wave;
  if (i >= a.cnt) return;  // wave-uniform; the kernel has no workgroup barrier
  const uint32_t D = a.D, L = a.labels[i], fr = a.slot[i];
  const float* __restrict__ x = a.xr + (size_t)i * D;
  const float* __restrict__ c = a.centers_rot + (size_t)L * D;
  uint32_t* brow = a.bits + (size_t)(fr >> 5) * a.W * 32 + (fr & 31);
  float l2 = 0.f, ipr = 0.f, ipc = 0.f, xq = 0.f;
  for (uint32_t tt = 0; tt < D / 64; ++tt) {
    const uint32_t j = lane + 64 * tt;
    const float cv = c[j], r = x[j] - cv;
    const bool b   = r >= 0.f;
    const float xu = b ? 0.5f : -0.5f;
    l2  = l2 + r * r;
    ipr = ipr + r * xu;
    ipc = ipc + cv * xu;
    xq  = xq + xu * xu;
    const unsigned long long m = __ballot(b);
    if (lane == 0) {
      brow[(size_t)(2 * tt) * 32]     = (uint32_t)m;
      brow[(size_t)(2 * tt + 1) * 32] = (uint32_t)(m >> 32);
    }
  }
  l2 = wave_sum(l2); ipr = wave_sum(ipr); ipc = wave_sum(ipc); xq = wave_sum(xq);
  const float l2n = sqrtf(fmaxf(l2, 0.f));
  {
    const float denom = ipr == 0.0f ? INFINITY : ipr;
    const float fadd  = l2 + 2.f * l2 * (ipc / denom);
    const float frs   = -2.f * l2 / denom;
    const float ratio = (l2 * xq) / (denom * denom);
    float inner       = (ratio - 1.f) / fmaxf((float)(D - 1), 1.f);
    inner             = fmaxf(inner, 0.f);
    const float ferr  = 2.f * (l2n * kRbqEps * sqrtf(inner));
    if (lane == 0) {
      a.short_fac[fr] = make_float4(fadd, frs, ferr, 0.f);
      a.ids[fr]       = (uint32_t)(a.r0 + i);
    }
  }
  if (a.ex == 0) return;
  const int ex = (int)a.ex, top = (1 << ex) - 1;
  const float half_top = (float)(1 << ex) - 0.5f;
  uint8_t* sc = enc_smem + (size_t)wave * D;
  float ipn = 0.f, ipr2 = 0.f, ipc2 = 0.f;
  for (uint32_t tt = 0; tt < D / 64; ++tt) {
    const uint32_t j = lane + 64 * tt;
    const float cv = c[j], r = x[j] - cv;
    const bool b    = r >= 0.f;
    const float val = l2n > 0.f ? fabsf(r) / l2n : 0.f;
    int code        = (int)(a.t * val + 1e-5f);
    if (code > top) code = top;
    ipn = ipn + ((float)code + 0.5f) * val;
    const int cf   = b ? code : ((~code) & top);
    const float xu = (float)(cf + ((b ? 1 : 0) << ex)) - half_top;
    ipr2 = ipr2 + r * xu;
    ipc2 = ipc2 + cv * xu;
    sc[j] = (uint8_t)cf;
  }
  ipn = wave_sum(ipn); ipr2 = wave_sum(ipr2); ipc2 = wave_sum(ipc2);
  float inv = 1.0f / ipn;
  if (!isfinite(inv)) inv = 1.0f;
  const float denom2 = ipr2 == 0.0f ? INFINITY : ipr2;
  const float fadd2  = l2 + 2.f * l2 * ipc2 / denom2;
  const float frs2   = -2.f * l2n * inv;
  if (lane == 0) a.ex_fac[fr] = make_float2(fadd2, frs2);
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  // MSB-first stream of ex bits per dimension: bit p of the row is bit (ex - 1 - p % ex) of the code of dimension p / ex
  uint8_t* out = a.ex_codes + (size_t)fr * a.exb;
  for (uint32_t ob = lane; ob < a.exb; ob += 64) {
    uint32_t byte = 0;
#pragma unroll
    for (uint32_t bit = 0; bit < 8; ++bit) {
      const uint32_t p = ob * 8 + bit;
      byte |= (((uint32_t)sc[p / ex] >> (ex - 1 - p % ex)) & 1u) << (7 - bit);
    }
    out[ob] = (uint8_t)byte;
  }
}

// ------------------------------------------------------------------ search: per-query preparation
// one wave per query: S = sum of q' (the order of the encode sums), the quantized query of the mode
__global__ __launch_bounds__(256) void rbq_query_prep_kernel(const float* __restrict__ qr, int64_t nq, uint32_t D, int mode,
                                                             float* __restrict__ S, float* __restrict__ w,
                                                             int8_t* __restrict__ qhat, float* __restrict__ qlut)
{
  const int lane = threadIdx.x & 63;
  const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= nq) return;
  const float* __restrict__ v = qr + (size_t)q * D;
  float s = 0.f, mx = 0.f;
  for (uint32_t tt = 0; tt < D / 64; ++tt) {
    const float x = v[lane + 64 * tt];
    s  = s + x;
    mx = fmaxf(mx, fabsf(x));
  }
  s = wave_sum(s);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
  if (mode == CUVS_AMD_IVF_RABITQ_QUANT4 || mode == CUVS_AMD_IVF_RABITQ_QUANT8) {
    const float qmax = mode == CUVS_AMD_IVF_RABITQ_QUANT4 ? 7.f : 127.f;
    const float ww   = mx / qmax;
    for (uint32_t tt = 0; tt < D / 64; ++tt) {
      const uint32_t j = lane + 64 * tt;
      float r = ww > 0.f ? rintf(v[j] / ww) : 0.f;  // round to nearest even
      r       = fminf(fmaxf(r, -qmax), qmax);
      qhat[(size_t)q * D + j] = (int8_t)r;
    }
    if (lane == 0) w[q] = ww;
  } else {
    for (uint32_t tt = 0; tt < D / 64; ++tt) {
      const uint32_t j = lane + 64 * tt;
      qlut[(size_t)q * D + j] = mode == CUVS_AMD_IVF_RABITQ_LUT16 ? __half2float(__float2half_rn(v[j])) : v[j];
    }
    if (lane == 0) w[q] = 1.f;
  }
  if (lane == 0) S[q] = s;
}

// one thread per query: the head (the shortest prefix of the probe order that holds k rows), the first mask word of every pair in
// the query's row of the mask (a pair takes ceil(list size / 32) words), the pair labels of the screen's grouping (head pairs get
// the label n_lists: never screened), the rows of the tail for the statistics
__global__ void rbq_head_kernel(const uint32_t* __restrict__ probes, const uint32_t* __restrict__ list_sizes, int64_t nq,
                                uint32_t n_probes, uint32_t k, uint32_t n_lists, uint32_t* __restrict__ head_len,
                                uint32_t* __restrict__ seg, uint32_t* __restrict__ labels, unsigned long long* __restrict__ stats)
{
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nq) return;
  uint64_t cum = 0, tail_rows = 0, head_rows = 0;
  uint32_t off = 0, hl = n_probes;
  bool done = false;
  for (uint32_t p = 0; p < n_probes; ++p) {
    const uint32_t L = probes[q * n_probes + p], sz = list_sizes[L];
    seg[q * n_probes + p]    = off;
    labels[q * n_probes + p] = done ? L : n_lists;
    off += (sz + 31) / 32;
    if (done) tail_rows += sz;
    else {
      head_rows += sz;
      cum += sz;
      if (cum >= k) { done = true; hl = p + 1; }
    }
  }
  head_len[q] = hl;
  if (tail_rows) atomicAdd(&stats[0], (unsigned long long)tail_rows);
  if (head_rows) atomicAdd(&stats[1], (unsigned long long)head_rows);
}

// one thread per pair: the words of a head pair hold one bit per row of the list (the mask was zeroed before)
__global__ void rbq_head_mask_kernel(const uint32_t* __restrict__ probes, const uint32_t* __restrict__ list_sizes,
                                     const uint32_t* __restrict__ head_len, const uint32_t* __restrict__ seg, int64_t n_pairs,
                                     uint32_t n_probes, size_t ldw, uint32_t* __restrict__ mask)
{
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_pairs) return;
  const int64_t q = p / n_probes;
  if ((uint32_t)(p % n_probes) >= head_len[q]) return;
  const uint32_t sz = list_sizes[probes[p]];
  uint32_t* mw = mask + (size_t)q * ldw + seg[p];
  for (uint32_t wd = 0; wd * 32 < sz; ++wd) {
    const uint32_t cnt = min(32u, sz - wd * 32);
    mw[wd] = cnt == 32 ? 0xffffffffu : ((1u << cnt) - 1u);
  }
}

// one wave per query: set bits of its mask row
__global__ __launch_bounds__(256) void rbq_count_kernel(const uint32_t* __restrict__ mask, int64_t nq, size_t ldw,
                                                        uint32_t* __restrict__ counts)
{
  const int lane = threadIdx.x & 63;
  const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= nq) return;
  int c = 0;
  for (size_t i = lane; i < ldw; i += 64) c += __popc(mask[(size_t)q * ldw + i]);
  c = wave_sum_i(c);
  if (lane == 0) counts[q] = (uint32_t)c;
}

// one wave per query: the set bits of its mask row in order (probe rank, row) -> entries (flat row, pair) from offsets[q] on
__global__ __launch_bounds__(256) void rbq_fill_kernel(const uint32_t* __restrict__ mask, const uint32_t* __restrict__ probes,
                                                       const uint32_t* __restrict__ list_sizes, const uint32_t* __restrict__ list_offsets,
                                                       const uint32_t* __restrict__ seg, const uint32_t* __restrict__ offsets, int64_t nq,
                                                       uint32_t n_probes, size_t ldw, uint32_t* __restrict__ ent_row,
                                                       uint32_t* __restrict__ ent_pair)
{
  const int lane = threadIdx.x & 63;
  const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= nq) return;
  uint32_t base = offsets[q];
  for (uint32_t p = 0; p < n_probes; ++p) {
    const uint32_t pair = (uint32_t)(q * n_probes + p);
    const uint32_t L = probes[pair], nw = (list_sizes[L] + 31) / 32, lo = list_offsets[L];
    const uint32_t* mw = mask + (size_t)q * ldw + seg[pair];
    for (uint32_t w0 = 0; w0 < nw; w0 += 64) {
      const uint32_t wd = w0 + lane;
      uint32_t m        = wd < nw ? mw[wd] : 0u;
      const int c       = __popc(m);
      const int inc     = wave_inclusive_scan(c);
      uint32_t pos      = base + (uint32_t)(inc - c);
      while (m != 0u) {
        const uint32_t b = (uint32_t)__ffs((int)m) - 1u;
        m &= m - 1u;
        ent_row[pos]  = lo + wd * 32 + b;
        ent_pair[pos] = pair;
        ++pos;
      }
      base += (uint32_t)__shfl(inc, 63, 64);
    }
  }
}

// ------------------------------------------------------------------ search: the screen
struct rbq_screen_args {
  const work_item* items;
  const uint32_t* n_items;
  const uint32_t* sorted_pairs;
  const int8_t* qhat;  // [nq, D]
  const float* qlut;   // [nq, D]
  const float* w;      // [nq]
  const float* S;      // [nq]
  const float* pd;     // [n_pairs] g of the pair
  const float* T;      // [nq]
  const uint32_t* bits;
  const float4* short_fac;
  const uint32_t* list_offsets;
  const uint32_t* list_sizes;
  const uint32_t* seg;
  uint32_t* mask;
  uint32_t n_probes, D, W;
  size_t ldw;
  unsigned long long* stats;  // word 2: rows the screen read (a list's rows once per work item)
};

// the per-slot terms of a work item: [0] w, [1] S / 2, [2] g, [3] sqrt(g), [4] T as floats, [5] the first mask word of the pair,
// [6] the query; slots past the item's count hold T = -inf (nothing passes) and are never written
__device__ inline void rbq_item_terms(const rbq_screen_args& a, const work_item& item, float* par, uint32_t* mbase, uint32_t* qid)
{
  const int tid = threadIdx.x;
  if (tid < kRbqQPB) {
    const bool live  = tid < (int)item.count;
    const uint32_t p = live ? a.sorted_pairs[item.first + tid] : 0u;
    const uint32_t q = p / a.n_probes;
    const float g    = live ? fmaxf(a.pd[p], 0.f) : 0.f;
    par[0 * kRbqQPB + tid] = live ? a.w[q] : 0.f;
    par[1 * kRbqQPB + tid] = live ? 0.5f * a.S[q] : 0.f;
    par[2 * kRbqQPB + tid] = g;
    par[3 * kRbqQPB + tid] = sqrtf(g);
    par[4 * kRbqQPB + tid] = live ? a.T[q] : -INFINITY;
    mbase[tid]             = live ? (uint32_t)((size_t)q * a.ldw + a.seg[p]) : 0u;
    qid[tid]               = q;
  }
  if (tid == 0 && a.stats != nullptr) atomicAdd(&a.stats[2], (unsigned long long)a.list_sizes[item.list]);
}

// low = (f_add + g + f_rescale (ip1 - S / 2)) - f_error sqrt(g), every operation rounded on its own
__device__ inline bool rbq_passes(const float4 f, const float ip1, const float* par, const int slot)
{
  const float t2  = ip1 - par[1 * kRbqQPB + slot];
  const float est = (f.x + par[2 * kRbqQPB + slot]) + f.y * t2;
  const float low = est - f.z * par[3 * kRbqQPB + slot];
  return low < par[4 * kRbqQPB + slot];
}

// 16 bits -> 16 bytes of 0 / 1 (bit i to byte i): a nibble times 0x204081 puts its bits 0..3 at bits 0, 8, 16, 24
__device__ inline rbq_i32x4 rbq_expand16(const uint32_t h)
{
  rbq_i32x4 r;
  r[0] = (int)((((h >> 0) & 15u) * 0x204081u) & 0x01010101u);
  r[1] = (int)((((h >> 4) & 15u) * 0x204081u) & 0x01010101u);
  r[2] = (int)((((h >> 8) & 15u) * 0x204081u) & 0x01010101u);
  r[3] = (int)((((h >> 12) & 15u) * 0x204081u) & 0x01010101u);
  return r;
}

// QUANT4 / QUANT8. A work item = one list x up to 32 of the queries that probe it in their tail. The item's quantized queries are
// staged in the LDS once (row pitch D + 16 bytes); a wave takes 32-row tiles of the list: per 32 dimensions one word per lane from
// memory (each bit code is read once per item), expanded to the B operand, one v_mfma_i32_32x32x32_i8 against the A operand from
// the LDS. Accumulator register i of lane (li, h) = row li of the tile x query slot (i & 3) + 8 (i >> 2) + 4 h (the operand maps of
// coarse_lowp.hip). The epilogue applies the row's factors and the compare; a ballot per register gives the 32-row survivor words of
// two slots, each written once by the only wave that owns (pair, tile): no atomics, no dependence on the order of the waves.
__global__ __launch_bounds__(256) void rbq_screen_mfma_kernel(rbq_screen_args a)
{
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const uint32_t wi = blockIdx.x;
  if (wi >= *a.n_items) return;
  const work_item item = a.items[wi];
  const uint32_t qstride = a.D + 16;
  int8_t* sq      = reinterpret_cast<int8_t*>(smem);
  float* par      = reinterpret_cast<float*>(smem + (size_t)kRbqQPB * qstride);
  uint32_t* mbase = reinterpret_cast<uint32_t*>(par + 5 * kRbqQPB);
  uint32_t* qid   = mbase + kRbqQPB;
  const int tid   = threadIdx.x;
  rbq_item_terms(a, item, par, mbase, qid);
  __syncthreads();
  const uint32_t c16 = a.D / 16;
  for (uint32_t idx = tid; idx < kRbqQPB * c16; idx += 256) {
    const uint32_t slot = idx / c16, c = idx % c16;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (slot < item.count) v = reinterpret_cast<const uint4*>(a.qhat + (size_t)qid[slot] * a.D)[c];
    *reinterpret_cast<uint4*>(sq + (size_t)slot * qstride + (size_t)c * 16) = v;
  }
  __syncthreads();
  const int lane = tid & 63, wave = tid >> 6, li = lane & 31, h = lane >> 5;
  const uint32_t L = item.list, base_row = a.list_offsets[L], len = a.list_sizes[L];
  const uint32_t n_tile = (len + 31) / 32;
  for (uint32_t tile = wave; tile < n_tile; tile += 4) {
    const uint32_t* __restrict__ bp = a.bits + ((size_t)(base_row >> 5) + tile) * a.W * 32 + li;
    const uint4* ap = reinterpret_cast<const uint4*>(sq + (size_t)li * qstride) + h;
    rbq_i32x16 acc = {};
    for (uint32_t s = 0; s < a.W; ++s) {
      const uint32_t word = bp[(size_t)s * 32];
      const rbq_i32x4 bv  = rbq_expand16((word >> (16 * h)) & 0xffffu);
      const uint4 av      = ap[s * 2];
      acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(__builtin_bit_cast(rbq_i32x4, av), bv, acc, 0, 0, 0);
    }
    const uint32_t row = tile * 32 + li;
    const bool valid   = row < len;
    const float4 f     = a.short_fac[(size_t)base_row + (valid ? row : 0u)];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int slot  = (i & 3) + 8 * (i >> 2) + 4 * h;
      const float ip1 = par[slot] * (float)acc[i];
      const bool pass = valid && rbq_passes(f, ip1, par, slot);
      const unsigned long long m = __ballot(pass);
      if (li == 0 && slot < (int)item.count) a.mask[(size_t)mbase[slot] + tile] = (uint32_t)(m >> (32 * h));
    }
  }
}

// LUT32 / LUT16: ip1 = the fp32 sum of the query components at the row's set bits, added in dimension order (a clear bit adds 0).
// Same items, tiles and survivor words; lanes 0..31 take the even slots, lanes 32..63 the odd ones.
__global__ __launch_bounds__(256) void rbq_screen_lut_kernel(rbq_screen_args a)
{
  __shared__ float par[5 * kRbqQPB];
  __shared__ uint32_t mbase[kRbqQPB], qid[kRbqQPB];
  const uint32_t wi = blockIdx.x;
  if (wi >= *a.n_items) return;
  const work_item item = a.items[wi];
  const int tid = threadIdx.x;
  rbq_item_terms(a, item, par, mbase, qid);
  __syncthreads();
  const int lane = tid & 63, wave = tid >> 6, li = lane & 31, h = lane >> 5;
  const uint32_t L = item.list, base_row = a.list_offsets[L], len = a.list_sizes[L];
  const uint32_t n_tile = (len + 31) / 32;
  for (uint32_t tile = wave; tile < n_tile; tile += 4) {
    const uint32_t* __restrict__ bp = a.bits + ((size_t)(base_row >> 5) + tile) * a.W * 32 + li;
    const uint32_t row = tile * 32 + li;
    const bool valid   = row < len;
    const float4 f     = a.short_fac[(size_t)base_row + (valid ? row : 0u)];
    for (uint32_t it = 0; 2 * it < item.count; ++it) {
      const int slot = (int)(2 * it) + h;
      const bool act = slot < (int)item.count;
      const float* __restrict__ qv = a.qlut + (size_t)qid[act ? slot : 0] * a.D;
      float acc = 0.f;
      for (uint32_t s = 0; s < a.W; ++s) {
        const uint32_t word = bp[(size_t)s * 32];
#pragma unroll 8
        for (uint32_t i = 0; i < 32; ++i) acc = acc + (((word >> i) & 1u) ? qv[s * 32 + i] : 0.f);
      }
      const bool pass = act && valid && rbq_passes(f, acc, par, act ? slot : 0);
      const unsigned long long m = __ballot(pass);
      if (li == 0 && act) a.mask[(size_t)mbase[slot] + tile] = (uint32_t)(m >> (32 * h));
    }
  }
}

// ------------------------------------------------------------------ search: re-score and selection
struct rbq_rescore_args {
  const uint32_t* ent_row;
  const uint32_t* ent_pair;
  int64_t n_ent;
  const float* qr;  // [nq, D] rotated queries (fp32: the final distance never uses the quantized query)
  const float* S;
  const float* pd;
  const uint32_t* bits;
  const float4* short_fac;
  const uint8_t* ex_codes;
  const float2* ex_fac;
  const uint32_t* ids;
  uint32_t n_probes, D, W, ex, exb;
  float* ent_d;
  uint32_t* ent_id;
};

// one wave per candidate: dot = sum over dimensions of q'_j u_j, u_j = (b_j << ex) | code_j, in the order of the encode sums;
// distance = (f_add + g) + f_rescale (dot - (2^(ex + 1) - 1) / 2 S) with the extended factors (ex = 0: the short ones)
__global__ __launch_bounds__(256) void rbq_rescore_kernel(rbq_rescore_args a)
{
  const int lane = threadIdx.x & 63;
  const int ex = (int)a.ex, top = (1 << ex) - 1;
  const float cs = (float)((1 << (ex + 1)) - 1) * 0.5f;
  for (int64_t e = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); e < a.n_ent; e += (int64_t)gridDim.x * 4) {
    const uint32_t fr = a.ent_row[e], pair = a.ent_pair[e];
    const uint32_t q  = pair / a.n_probes;
    const float* __restrict__ qv     = a.qr + (size_t)q * a.D;
    const uint32_t* __restrict__ br  = a.bits + (size_t)(fr >> 5) * a.W * 32 + (fr & 31);
    const uint8_t* __restrict__ xrow = a.ex_codes + (size_t)fr * a.exb;
    float acc = 0.f;
    for (uint32_t tt = 0; tt < a.D / 64; ++tt) {
      const uint32_t j = lane + 64 * tt;
      uint32_t u       = (br[(size_t)(j >> 5) * 32] >> (j & 31)) & 1u;
      if (ex > 0) {
        const uint32_t bitpos = j * (uint32_t)ex, byte = bitpos >> 3, off = bitpos & 7u;
        const uint32_t win = ((uint32_t)xrow[byte] << 8) | (byte + 1 < a.exb ? (uint32_t)xrow[byte + 1] : 0u);
        u = (u << ex) | ((win >> (16 - ex - (int)off)) & (uint32_t)top);
      }
      acc = acc + qv[j] * (float)u;
    }
    acc = wave_sum(acc);
    float fa, frs;
    if (ex > 0) { const float2 f = a.ex_fac[fr]; fa = f.x; frs = f.y; }
    else        { const float4 f = a.short_fac[fr]; fa = f.x; frs = f.y; }
    const float d = (fa + fmaxf(a.pd[pair], 0.f)) + frs * (acc - cs * a.S[q]);
    if (lane == 0) {
      a.ent_d[e]  = d;
      a.ent_id[e] = a.ids[fr];
    }
  }
}

// one wave per query: the k smallest of its candidates - segment A (the head rows) and, when given, segment B (the survivors of
// the screen) - by (distance, source id). threshold != nullptr: only the k-th distance is written (+inf with fewer than k candidates).
template <int E>
__global__ __launch_bounds__(256) void rbq_select_kernel(const uint32_t* __restrict__ off_a, const float* __restrict__ d_a,
                                                         const uint32_t* __restrict__ i_a, const uint32_t* __restrict__ off_b,
                                                         const float* __restrict__ d_b, const uint32_t* __restrict__ i_b, int64_t nq,
                                                         int k, float* __restrict__ threshold, int64_t* __restrict__ neighbors,
                                                         float* __restrict__ distances, int take_sqrt)
{
  const int lane = threadIdx.x & 63;
  const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= nq) return;
  wave_top<E> top;
  top.init();
  const int kr = k - 1;
  float kd     = INFINITY;
  uint32_t ki  = 0xffffffffu;
  for (int sgm = 0; sgm < 2; ++sgm) {
    const uint32_t* off = sgm == 0 ? off_a : off_b;
    if (off == nullptr) continue;
    const float* dd    = sgm == 0 ? d_a : d_b;
    const uint32_t* ii = sgm == 0 ? i_a : i_b;
    const uint32_t b = off[q], e = off[q + 1];
    for (uint32_t i0 = b; i0 < e; i0 += 64) {
      const uint32_t i = i0 + lane;
      const bool ok    = i < e;
      const float d    = ok ? dd[i] : INFINITY;
      const uint32_t id = ok ? ii[i] : 0xffffffffu;
      unsigned long long m = __ballot(ok && ((d < kd) || (d == kd && id < ki)));
      while (m != 0ull) {
        const int src = (int)__ffsll((long long)m) - 1;
        m &= m - 1ull;
        const float cd    = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(d), src));
        const uint32_t ci = __builtin_amdgcn_readlane(id, src);
        if ((cd < kd) || (cd == kd && ci < ki)) {
          top.insert(cd, ci, lane);
          kd = top.rank_d(kr);
          ki = top.rank_i(kr);
        }
      }
    }
  }
  if (threshold != nullptr) {
    if (lane == 0) threshold[q] = kd;
    return;
  }
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int r = e * 64 + lane;
    if (r >= k) continue;
    const bool ok = top.i[e] != 0xffffffffu;
    float d       = top.d[e];
    if (take_sqrt) d = sqrtf(fmaxf(d, 0.f));
    neighbors[q * k + r] = ok ? (int64_t)top.i[e] : INT64_MAX;
    distances[q * k + r] = ok ? d : FLT_MAX;
  }
}

void rbq_select(resources& res, const uint32_t* off_a, const float* d_a, const uint32_t* i_a, const uint32_t* off_b, const float* d_b,
                const uint32_t* i_b, int64_t nq, int k, float* threshold, int64_t* neighbors, float* distances, int take_sqrt)
{
  const dim3 grid(grid_blocks(nq, 4)), block(256);
  auto go = [&](auto kern) {
    hipLaunchKernelGGL(kern, grid, block, 0, res.stream, off_a, d_a, i_a, off_b, d_b, i_b, nq, k, threshold, neighbors, distances, take_sqrt);
  };
  if (k <= 64) go(rbq_select_kernel<1>);
  else if (k <= 256) go(rbq_select_kernel<4>);
  else go(rbq_select_kernel<16>);
}

// the entries of a mask (count, scan, read the total back, fill) and their distances
struct rbq_entries {
  dev_buf<uint32_t> off, row, pair, id;
  dev_buf<float> d;
  int64_t n = 0;
};

}  // namespace

std::unique_ptr<ivf_rabitq_index> ivf_rabitq_build(resources& res, const cuvsAmdIvfRabitqIndexParams& p, const void* data, int64_t n,
                                                   int64_t dim, bool is_host)
{
  CUVS_EXPECTS(n > 0 && dim > 0, "ivf_rabitq::build: empty dataset");
  CUVS_EXPECTS(p.n_lists > 0 && n >= p.n_lists, "ivf_rabitq::build: number of rows (%ld) can't be less than n_lists (%u)", (long)n, p.n_lists);
  CUVS_EXPECTS(p.n_lists <= rabitq_host::kMaxLists, "ivf_rabitq::build: n_lists too large");
  CUVS_EXPECTS(p.bits_per_dim >= 1 && p.bits_per_dim <= 9, "ivf_rabitq::build: bits_per_dim=%u out of the valid range [1, 9]", p.bits_per_dim);
  CUVS_EXPECTS(p.metric == L2Expanded || p.metric == L2SqrtExpanded,
               "ivf_rabitq::build: unsupported metric %d (L2Expanded and L2SqrtExpanded only)", (int)p.metric);
  CUVS_EXPECTS(p.fast_quantize_flag, "ivf_rabitq::build: fast_quantize_flag = false (the per-vector search of the rescale factor) is not implemented");
  CUVS_EXPECTS(p.max_train_points_per_cluster > 0, "ivf_rabitq::build: max_train_points_per_cluster must be > 0");
  CUVS_EXPECTS(p.streaming_batch_size > 0, "ivf_rabitq::build: streaming_batch_size must be > 0");
  CUVS_EXPECTS((uint64_t)dim <= rabitq_host::kMaxDim, "ivf_rabitq::build: dim=%ld exceeds the maximum %lu", (long)dim, (unsigned long)rabitq_host::kMaxDim);
  CUVS_EXPECTS(n + 32 * (int64_t)p.n_lists < (int64_t(1) << 32), "ivf_rabitq::build: %ld rows do not fit 32-bit row ids", (long)n);
  auto idx     = std::make_unique<ivf_rabitq_index>();
  idx->metric  = (int)p.metric;
  idx->n_lists = p.n_lists;
  idx->dim     = (uint32_t)dim;
  idx->D       = (uint32_t)rabitq_host::padded_dim((uint64_t)dim);
  idx->W       = idx->D / 32;
  idx->ex      = p.bits_per_dim - 1;
  idx->exb     = idx->D * idx->ex / 8;
  idx->t       = rbq_scaling_factor(idx->D, idx->ex);
  const uint32_t D = idx->D;

  // a host dataset is streamed in batches of streaming_batch_size rows when asked to, or when 4x its size exceeds the workspace;
  // otherwise it is copied to the device once
  const bool streaming = is_host && (p.force_streaming || (size_t)n * dim * 4 > res.workspace_limit / 4);
  dev_buf<float> on_device;
  if (is_host && !streaming) {
    on_device = dev_buf<float>(res, (size_t)n * dim);
    copy_async(res, on_device.data(), data, (size_t)n * dim * sizeof(float));
    sync(res);
    data    = on_device.data();
    is_host = false;
  }

  // ---- centres: the trainset rule of the IVF-SQ build, balanced k-means
  idx->centers = dev_buf<float>::persistent((size_t)p.n_lists * dim);
  {
    const int64_t n_train = std::min<int64_t>(n, (int64_t)p.n_lists * p.max_train_points_per_cluster);
    const std::vector<uint32_t> pick = pick_train_rows(n, n_train);
    dev_buf<float> trainset(res, (size_t)n_train * dim);
    dev_buf<uint32_t> tids(res, n_train);
    copy_async(res, tids.data(), pick.data(), (size_t)n_train * sizeof(uint32_t));
    load_gather_as_float(res, data, elem_t::f32, is_host, dim, tids.data(), n_train, trainset.data());
    sync(res);
    kmeans_params kp;
    kp.n_iters = (int)p.kmeans_n_iters;
    kmeans_balanced_fit(res, trainset.data(), n_train, dim, (int)p.n_lists, kp, idx->centers.data());
  }
  dev_buf<float> center_norms(res, p.n_lists);
  row_norms<float>(res, idx->centers.data(), p.n_lists, dim, dim, center_norms.data(), false);

  // ---- rotation, rotated centres
  {
    const std::vector<float> rot = random_rotation_matrix(D, D);
    idx->rotation = dev_buf<float>::persistent((size_t)D * D);
    copy_async(res, idx->rotation.data(), rot.data(), rot.size() * sizeof(float));
    sync(res);
  }
  idx->centers_rot      = dev_buf<float>::persistent((size_t)p.n_lists * D);
  idx->center_rot_norms = dev_buf<float>::persistent(p.n_lists);
  {
    dev_buf<float> cpad(res, (size_t)p.n_lists * D);
    hipLaunchKernelGGL(rbq_pad_rows_kernel, dim3(grid_blocks((int64_t)p.n_lists * D, 256)), dim3(256), 0, res.stream, idx->centers.data(),
                       (int64_t)p.n_lists, (uint32_t)dim, D, cpad.data());
    pairwise_distance<float, float>(res, cpad.data(), p.n_lists, D, idx->rotation.data(), D, D, D, nullptr, nullptr, M_InnerProduct,
                                    idx->centers_rot.data(), D);
    row_norms<float>(res, idx->centers_rot.data(), p.n_lists, D, D, idx->center_rot_norms.data(), false);
    sync(res);
  }

  // ---- pass 1: labels
  const int64_t batch = streaming ? std::min<int64_t>(n, p.streaming_batch_size)
                                  : std::min<int64_t>(n, std::max<int64_t>(1024, (int64_t(1) << 26) / D));
  dev_buf<uint32_t> labels(res, n), slot(res, n);
  dev_buf<float> xb(res, (size_t)batch * dim);
  for (int64_t r0 = 0; r0 < n; r0 += batch) {
    const int64_t cnt = std::min(batch, n - r0);
    load_range_as_float(res, data, elem_t::f32, is_host, dim, r0, cnt, xb.data());
    fused_l2_argmin<float>(res, xb.data(), cnt, dim, idx->centers.data(), p.n_lists, dim, center_norms.data(), labels.data() + r0, nullptr);
  }
  // ---- lists: rows of a list in input order, every list starts at a multiple of 32 rows
  {
    dev_buf<uint32_t> perm(res, n), grp_off(res, p.n_lists + 1);
    group_by_label(res, labels.data(), n, p.n_lists, perm.data(), grp_off.data());
    const std::vector<uint32_t> h_off = to_host(res, grp_off.data(), p.n_lists + 1);
    idx->h_list_sizes.resize(p.n_lists);
    idx->h_list_offsets.resize(p.n_lists + 1);
    int64_t total = 0;
    for (uint32_t L = 0; L < p.n_lists; ++L) {
      idx->h_list_sizes[L]   = h_off[L + 1] - h_off[L];
      idx->h_list_offsets[L] = (uint32_t)total;
      total += round_up(idx->h_list_sizes[L], 32);
    }
    idx->h_list_offsets[p.n_lists] = (uint32_t)total;
    idx->padded_rows  = total;
    idx->list_sizes   = dev_buf<uint32_t>::persistent(p.n_lists);
    idx->list_offsets = dev_buf<uint32_t>::persistent(p.n_lists + 1);
    copy_async(res, idx->list_sizes.data(), idx->h_list_sizes.data(), p.n_lists * sizeof(uint32_t));
    copy_async(res, idx->list_offsets.data(), idx->h_list_offsets.data(), (p.n_lists + 1) * sizeof(uint32_t));
    hipLaunchKernelGGL(rbq_slots_kernel, dim3(grid_blocks(n, 256)), dim3(256), 0, res.stream, perm.data(), labels.data(), grp_off.data(),
                       idx->list_offsets.data(), n, slot.data());
    sync(res);
  }
  const size_t rows = (size_t)idx->padded_rows;
  idx->bits      = dev_buf<uint32_t>::persistent(rows * idx->W);
  idx->short_fac = dev_buf<float4>::persistent(rows);
  idx->ex_codes  = dev_buf<uint8_t>::persistent(rows * idx->exb);
  idx->ex_fac    = dev_buf<float2>::persistent(rows);
  idx->ids       = dev_buf<uint32_t>::persistent(rows);
  HIP_TRY(hipMemsetAsync(idx->bits.data(), 0, idx->bits.bytes(), res.stream));
  HIP_TRY(hipMemsetAsync(idx->short_fac.data(), 0, idx->short_fac.bytes(), res.stream));
  if (idx->ex_codes.bytes()) HIP_TRY(hipMemsetAsync(idx->ex_codes.data(), 0, idx->ex_codes.bytes(), res.stream));
  HIP_TRY(hipMemsetAsync(idx->ex_fac.data(), 0, idx->ex_fac.bytes(), res.stream));
  HIP_TRY(hipMemsetAsync(idx->ids.data(), 0xff, idx->ids.bytes(), res.stream));

  // ---- pass 2: rotate and encode
  {
    dev_buf<float> xpad(res, (size_t)batch * D), xr(res, (size_t)batch * D);
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(rbq_encode_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(4 * D)));
    for (int64_t r0 = 0; r0 < n; r0 += batch) {
      const int64_t cnt = std::min(batch, n - r0);
      load_range_as_float(res, data, elem_t::f32, is_host, dim, r0, cnt, xb.data());
      hipLaunchKernelGGL(rbq_pad_rows_kernel, dim3(grid_blocks(cnt * D, 256)), dim3(256), 0, res.stream, xb.data(), cnt, (uint32_t)dim, D,
                         xpad.data());
      pairwise_distance<float, float>(res, xpad.data(), cnt, D, idx->rotation.data(), D, D, D, nullptr, nullptr, M_InnerProduct, xr.data(), D);
      rbq_encode_args a{};
      a.xr = xr.data(); a.labels = labels.data() + r0; a.slot = slot.data() + r0; a.centers_rot = idx->centers_rot.data();
      a.cnt = cnt; a.r0 = r0; a.D = D; a.W = idx->W; a.ex = idx->ex; a.exb = idx->exb; a.t = idx->t;
      a.bits = idx->bits.data(); a.short_fac = idx->short_fac.data(); a.ex_codes = idx->ex_codes.data(); a.ex_fac = idx->ex_fac.data();
      a.ids = idx->ids.data();
      hipLaunchKernelGGL(rbq_encode_kernel, dim3(grid_blocks(cnt, 4)), dim3(256), 4 * D, res.stream, a);
      HIP_TRY(hipGetLastError());
      sync(res);
    }
  }
  idx->size = n;
  sync(res);
  return idx;
}

namespace {

// entries of the set bits of `mask`: count per query, exclusive scan, the total read back (the arrays are sized from it: no
// candidate is ever dropped), fill, re-score
void rbq_collect(resources& res, const ivf_rabitq_index& idx, const uint32_t* mask, size_t ldw, const uint32_t* probes, const uint32_t* seg,
                 int64_t nq, uint32_t n_probes, const float* qr, const float* S, const float* pd, dev_buf<uint32_t>& counts, rbq_entries& out)
{
  out.off = dev_buf<uint32_t>(res, nq + 1);
  hipLaunchKernelGGL(rbq_count_kernel, dim3(grid_blocks(nq, 4)), dim3(256), 0, res.stream, mask, nq, ldw, counts.data());
  hipLaunchKernelGGL(pair_scan_kernel, dim3(1), dim3(1024), 0, res.stream, counts.data(), (int)nq, out.off.data());
  HIP_TRY(hipGetLastError());
  out.n = (int64_t)read_word(res, out.off.data() + nq);
  const size_t cap = (size_t)std::max<int64_t>(out.n, 1);
  out.row  = dev_buf<uint32_t>(res, cap);
  out.pair = dev_buf<uint32_t>(res, cap);
  out.id   = dev_buf<uint32_t>(res, cap);
  out.d    = dev_buf<float>(res, cap);
  if (out.n == 0) return;
  hipLaunchKernelGGL(rbq_fill_kernel, dim3(grid_blocks(nq, 4)), dim3(256), 0, res.stream, mask, probes, idx.list_sizes.data(),
                     idx.list_offsets.data(), seg, out.off.data(), nq, n_probes, ldw, out.row.data(), out.pair.data());
  rbq_rescore_args a{};
  a.ent_row = out.row.data(); a.ent_pair = out.pair.data(); a.n_ent = out.n; a.qr = qr; a.S = S; a.pd = pd;
  a.bits = idx.bits.data(); a.short_fac = idx.short_fac.data(); a.ex_codes = idx.ex_codes.data(); a.ex_fac = idx.ex_fac.data();
  a.ids = idx.ids.data(); a.n_probes = n_probes; a.D = idx.D; a.W = idx.W; a.ex = idx.ex; a.exb = idx.exb;
  a.ent_d = out.d.data(); a.ent_id = out.id.data();
  const unsigned grid = (unsigned)std::min<int64_t>((out.n + 3) / 4, 1 << 20);
  profile_begin(res, "rbq_rescore_kernel");
  hipLaunchKernelGGL(rbq_rescore_kernel, dim3(grid), dim3(256), 0, res.stream, a);
  profile_end(res, "rbq_rescore_kernel");
  HIP_TRY(hipGetLastError());
}

}  // namespace

void ivf_rabitq_search(resources& res, const ivf_rabitq_index& idx, uint32_t n_probes, int mode, const float* queries, int64_t n_queries,
                       int k, int64_t* neighbors, float* distances)
{
  if (k == 0 || n_queries == 0 || n_probes == 0) return;
  CUVS_EXPECTS(k > 0, "ivf_rabitq::search: k must not be negative");
  CUVS_EXPECTS(k <= 1024, "ivf_rabitq::search: k=%d exceeds the maximum 1024", k);
  CUVS_EXPECTS(n_probes <= idx.n_lists, "ivf_rabitq::search: n_probes (%u) must not exceed n_lists (%u)", n_probes, idx.n_lists);
  CUVS_EXPECTS(mode >= CUVS_AMD_IVF_RABITQ_LUT16 && mode <= CUVS_AMD_IVF_RABITQ_QUANT8, "ivf_rabitq::search: unknown mode %d", mode);
  const bool quant  = mode == CUVS_AMD_IVF_RABITQ_QUANT4 || mode == CUVS_AMD_IVF_RABITQ_QUANT8;
  const uint32_t D  = idx.D;
  // a query's mask row: ceil(size / 32) words for each of its probes - at most those of the n_probes largest lists
  size_t ldw = 0, ld_rows = 0;
  {
    std::vector<uint32_t> s(idx.h_list_sizes);
    std::partial_sort(s.begin(), s.begin() + n_probes, s.end(), std::greater<uint32_t>());
    for (uint32_t i = 0; i < n_probes; ++i) { ldw += (s[i] + 31) / 32; ld_rows += s[i]; }
    ldw = std::max<size_t>(ldw, 1);
  }
  int64_t max_batch = 1 << 15;
  {
    const int64_t per_q = (int64_t)idx.n_lists * 4 + (int64_t)ldw * 4 + (int64_t)D * 16 + (int64_t)n_probes * 32 + (int64_t)ld_rows * 16 + 64;
    max_batch = std::min(max_batch, std::max<int64_t>(1, (int64_t)res.ivf_batch_limit / per_q));
    max_batch = std::min(max_batch, std::max<int64_t>(1, ((int64_t(1) << 31) - 1) / (int64_t)std::max<size_t>(ld_rows, 1)));
    max_batch = std::min(max_batch, std::max<int64_t>(1, ((int64_t(1) << 32) - 1) / (int64_t)ldw));
    max_batch = balanced_batch(n_queries, max_batch);
  }
  const int64_t bs = std::min<int64_t>(max_batch, n_queries), np_max = bs * n_probes;
  dev_buf<float> qpad(res, (size_t)bs * D), qr(res, (size_t)bs * D), qn(res, bs), dist(res, (size_t)bs * idx.n_lists), pd(res, np_max),
    S(res, bs), w(res, bs), T(res, bs), qlut(res, quant ? 0 : (size_t)bs * D);
  dev_buf<int8_t> qhat(res, quant ? (size_t)bs * D : 0);
  dev_buf<uint32_t> probes(res, np_max), head_len(res, bs), seg(res, np_max), labels(res, np_max), mask(res, (size_t)bs * ldw), counts(res, bs),
    sorted_pairs(res, np_max), pair_off(res, idx.n_lists + 2), item_off(res, idx.n_lists + 2);
  const size_t max_items = (size_t)(np_max / kRbqQPB + idx.n_lists + 2);
  dev_buf<work_item> items(res, max_items);
  dev_buf<unsigned long long> stats(res, 3);
  HIP_TRY(hipMemsetAsync(stats.data(), 0, stats.bytes(), res.stream));
  uint64_t n_survivors = 0;
  const size_t screen_smem = (size_t)kRbqQPB * (D + 16) + 7 * kRbqQPB * 4;
  if (quant)
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(rbq_screen_mfma_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)screen_smem));

  for (int64_t q0 = 0; q0 < n_queries; q0 += max_batch) {
    const int64_t nq = std::min(max_batch, n_queries - q0), n_pairs = nq * n_probes;
    // q' = rotate(pad(q)); the probes: the n_probes nearest rotated centres by fp32 L2, ties to the smaller list id
    hipLaunchKernelGGL(rbq_pad_rows_kernel, dim3(grid_blocks(nq * D, 256)), dim3(256), 0, res.stream, queries + q0 * idx.dim, nq, idx.dim, D,
                       qpad.data());
    pairwise_distance<float, float>(res, qpad.data(), nq, D, idx.rotation.data(), D, D, D, nullptr, nullptr, M_InnerProduct, qr.data(), D);
    row_norms<float>(res, qr.data(), nq, D, D, qn.data(), false);
    pairwise_distance<float, float>(res, qr.data(), nq, D, idx.centers_rot.data(), idx.n_lists, D, D, qn.data(), idx.center_rot_norms.data(),
                                    M_L2Expanded, dist.data(), idx.n_lists);
    select_k<uint32_t, uint32_t>(res, dist.data(), nullptr, nq, idx.n_lists, idx.n_lists, (int)n_probes, pd.data(), probes.data(), true);
    hipLaunchKernelGGL(rbq_query_prep_kernel, dim3(grid_blocks(nq, 4)), dim3(256), 0, res.stream, qr.data(), nq, D, mode, S.data(), w.data(),
                       qhat.data(), qlut.data());
    hipLaunchKernelGGL(rbq_head_kernel, dim3(grid_blocks(nq, 256)), dim3(256), 0, res.stream, probes.data(), idx.list_sizes.data(), nq, n_probes,
                       (uint32_t)k, idx.n_lists, head_len.data(), seg.data(), labels.data(), stats.data());
    // ---- the head: every row is a candidate; T = the k-th smallest final distance among them
    HIP_TRY(hipMemsetAsync(mask.data(), 0, (size_t)nq * ldw * sizeof(uint32_t), res.stream));
    hipLaunchKernelGGL(rbq_head_mask_kernel, dim3(grid_blocks(n_pairs, 256)), dim3(256), 0, res.stream, probes.data(), idx.list_sizes.data(),
                       head_len.data(), seg.data(), n_pairs, n_probes, ldw, mask.data());
    rbq_entries head;
    rbq_collect(res, idx, mask.data(), ldw, probes.data(), seg.data(), nq, n_probes, qr.data(), S.data(), pd.data(), counts, head);
    rbq_select(res, head.off.data(), head.d.data(), head.id.data(), nullptr, nullptr, nullptr, nq, k, T.data(), nullptr, nullptr, 0);
    // ---- the tail: screen (low < T), survivors re-scored
    HIP_TRY(hipMemsetAsync(mask.data(), 0, (size_t)nq * ldw * sizeof(uint32_t), res.stream));
    build_work_items(res, labels.data(), n_pairs, idx.n_lists + 1, kRbqQPB, sorted_pairs.data(), pair_off.data(), item_off.data(), items.data(),
                     -1, 0, nullptr, idx.n_lists);
    rbq_screen_args a{};
    a.items = items.data(); a.n_items = item_off.data() + idx.n_lists; a.sorted_pairs = sorted_pairs.data(); a.qhat = qhat.data();
    a.qlut = qlut.data(); a.w = w.data(); a.S = S.data(); a.pd = pd.data(); a.T = T.data(); a.bits = idx.bits.data();
    a.short_fac = idx.short_fac.data(); a.list_offsets = idx.list_offsets.data(); a.list_sizes = idx.list_sizes.data(); a.seg = seg.data();
    a.mask = mask.data(); a.n_probes = n_probes; a.D = D; a.W = idx.W; a.ldw = ldw; a.stats = stats.data();
    const unsigned grid = (unsigned)(n_pairs / kRbqQPB + idx.n_lists + 1);
    profile_begin(res, "rbq_screen_kernel");
    if (quant) hipLaunchKernelGGL(rbq_screen_mfma_kernel, dim3(grid), dim3(256), screen_smem, res.stream, a);
    else       hipLaunchKernelGGL(rbq_screen_lut_kernel, dim3(grid), dim3(256), 0, res.stream, a);
    profile_end(res, "rbq_screen_kernel");
    HIP_TRY(hipGetLastError());
    rbq_entries tail;
    rbq_collect(res, idx, mask.data(), ldw, probes.data(), seg.data(), nq, n_probes, qr.data(), S.data(), pd.data(), counts, tail);
    n_survivors += (uint64_t)tail.n;
    // ---- the k smallest of head rows and survivors by (distance, source id)
    rbq_select(res, head.off.data(), head.d.data(), head.id.data(), tail.off.data(), tail.d.data(), tail.id.data(), nq, k, nullptr,
               neighbors + q0 * k, distances + q0 * k, idx.metric == M_L2SqrtExpanded ? 1 : 0);
    HIP_TRY(hipGetLastError());
    sync(res);  // (head / tail entries are freed on the stream; the next batch reuses the scratch)
  }
  const std::vector<unsigned long long> h_stats = to_host(res, stats.data(), 3);
  g_last_stats[0] = h_stats[0];
  g_last_stats[1] = n_survivors;
  g_last_stats[2] = h_stats[1];
  g_last_stats[3] = h_stats[2] * ((uint64_t)idx.W * 4 + 16);
}

namespace {

// the whole index on the host in the file's encodings, rows in list order
struct rbq_host_arrays {
  std::vector<float> centers_rot, rotation, short_fac, ex_fac;
  std::vector<uint32_t> ids, bit_codes;
  std::vector<uint8_t> ex_codes;
};

rbq_host_arrays rbq_download(resources& res, const ivf_rabitq_index& idx)
{
  rbq_host_arrays h;
  const size_t n = (size_t)idx.size, W = idx.W, exb = idx.exb;
  h.centers_rot = to_host(res, idx.centers_rot.data(), idx.centers_rot.size());
  h.rotation    = to_host(res, idx.rotation.data(), idx.rotation.size());
  const std::vector<uint32_t> bits = to_host(res, idx.bits.data(), idx.bits.size());
  const std::vector<float4> sf     = to_host(res, idx.short_fac.data(), idx.short_fac.size());
  const std::vector<uint8_t> exc   = to_host(res, idx.ex_codes.data(), idx.ex_codes.size());
  const std::vector<float2> ef     = to_host(res, idx.ex_fac.data(), idx.ex_fac.size());
  const std::vector<uint32_t> ids  = to_host(res, idx.ids.data(), idx.ids.size());
  h.ids.resize(n); h.bit_codes.resize(n * W); h.short_fac.resize(n * 3); h.ex_codes.resize(n * exb); h.ex_fac.resize(n * 2);
  size_t o = 0;
  for (uint32_t L = 0; L < idx.n_lists; ++L) {
    for (uint32_t r = 0; r < idx.h_list_sizes[L]; ++r, ++o) {
      const size_t fr = (size_t)idx.h_list_offsets[L] + r;
      h.ids[o] = ids[fr];
      for (size_t wd = 0; wd < W; ++wd) h.bit_codes[o * W + wd] = rabitq_host::reverse_bits(bits[((fr >> 5) * W + wd) * 32 + (fr & 31)]);
      h.short_fac[o * 3] = sf[fr].x; h.short_fac[o * 3 + 1] = sf[fr].y; h.short_fac[o * 3 + 2] = sf[fr].z;
      if (exb) memcpy(&h.ex_codes[o * exb], &exc[fr * exb], exb);
      h.ex_fac[o * 2] = ef[fr].x; h.ex_fac[o * 2 + 1] = ef[fr].y;
    }
  }
  return h;
}

void rbq_write(resources& res, const char* filename, const ivf_rabitq_index& idx)
{
  CUVS_EXPECTS(filename != nullptr, "filename is null");
  const rbq_host_arrays h = rbq_download(res, idx);
  FILE* f = fopen(filename, "wb");
  CUVS_EXPECTS(f != nullptr, "Cannot open file %s", filename);
  bool ok = true;
  auto put = [&](const void* p, size_t bytes) { ok = ok && (bytes == 0 || fwrite(p, 1, bytes, f) == bytes); };
  const uint64_t head[4] = {(uint64_t)idx.size, idx.dim, idx.n_lists, idx.ex};
  const bool legacy = true;
  const float two[2] = {idx.t, idx.metric == M_L2SqrtExpanded ? 1.0f : 0.0f};
  put(head, sizeof(head)); put(&legacy, 1); put(two, sizeof(two));
  std::vector<uint64_t> sizes(idx.h_list_sizes.begin(), idx.h_list_sizes.end());
  put(sizes.data(), sizes.size() * 8);
  put(h.rotation.data(), h.rotation.size() * 4);
  put(h.centers_rot.data(), h.centers_rot.size() * 4);
  put(h.bit_codes.data(), h.bit_codes.size() * 4);
  put(h.short_fac.data(), h.short_fac.size() * 4);
  put(h.ex_codes.data(), h.ex_codes.size());
  put(h.ex_fac.data(), h.ex_fac.size() * 4);
  put(h.ids.data(), h.ids.size() * 4);
  ok = (fclose(f) == 0) && ok;
  CUVS_EXPECTS(ok, "write failed to %s", filename);
}

struct file_closer {
  FILE* f;
  ~file_closer() { if (f) fclose(f); }
};

std::unique_ptr<ivf_rabitq_index> rbq_read(resources& res, const char* filename)
{
  CUVS_EXPECTS(filename != nullptr, "filename is null");
  FILE* f = fopen(filename, "rb");
  CUVS_EXPECTS(f != nullptr, "Cannot open file %s", filename);
  file_closer closer{f};
  CUVS_EXPECTS(fseek(f, 0, SEEK_END) == 0, "cannot seek in %s", filename);
  const long file_bytes = ftell(f);
  CUVS_EXPECTS(file_bytes >= 0 && fseek(f, 0, SEEK_SET) == 0, "cannot seek in %s", filename);
  const rabitq_host::file_header h = rabitq_host::read_header(f, (uint64_t)file_bytes);  // every length checked against the file
  auto idx = std::make_unique<ivf_rabitq_index>();
  idx->metric  = h.metric == 1 ? (int)M_L2SqrtExpanded : (int)M_L2Expanded;
  idx->n_lists = (uint32_t)h.n_lists; idx->dim = (uint32_t)h.dim; idx->D = (uint32_t)h.D; idx->W = idx->D / 32;
  idx->ex = (uint32_t)h.ex_bits; idx->exb = (uint32_t)h.ex_row_bytes(); idx->t = h.t; idx->size = (int64_t)h.n;
  const size_t n = (size_t)h.n, W = idx->W, exb = idx->exb;
  auto get = [&](void* p, size_t bytes) { CUVS_EXPECTS(bytes == 0 || fread(p, 1, bytes, f) == bytes, "unexpected end of file in %s", filename); };
  std::vector<float> rotation((size_t)h.D * h.D), centers_rot((size_t)h.n_lists * h.D), short_fac(n * 3), ex_fac(n * 2);
  std::vector<uint32_t> bit_codes(n * W), ids(n);
  std::vector<uint8_t> ex_codes(n * exb);
  get(rotation.data(), rotation.size() * 4); get(centers_rot.data(), centers_rot.size() * 4); get(bit_codes.data(), bit_codes.size() * 4);
  get(short_fac.data(), short_fac.size() * 4); get(ex_codes.data(), ex_codes.size()); get(ex_fac.data(), ex_fac.size() * 4);
  get(ids.data(), ids.size() * 4);
  rabitq_host::check_ids(ids.data(), n);
  idx->h_list_sizes.resize(idx->n_lists);
  idx->h_list_offsets.resize(idx->n_lists + 1);
  int64_t total = 0;
  for (uint32_t L = 0; L < idx->n_lists; ++L) {
    idx->h_list_sizes[L]   = (uint32_t)h.sizes[L];
    idx->h_list_offsets[L] = (uint32_t)total;
    total += round_up((int64_t)h.sizes[L], 32);
  }
  CUVS_EXPECTS(total < (int64_t(1) << 32), "ivf_rabitq::deserialize: index too large for 32-bit row offsets");
  idx->h_list_offsets[idx->n_lists] = (uint32_t)total;
  idx->padded_rows = total;
  const size_t rows = (size_t)total;
  std::vector<uint32_t> bits(rows * W, 0u), pids(rows, 0xffffffffu);
  std::vector<float4> sf(rows, make_float4(0.f, 0.f, 0.f, 0.f));
  std::vector<float2> ef(rows, make_float2(0.f, 0.f));
  std::vector<uint8_t> exc(rows * exb, 0);
  size_t o = 0;
  for (uint32_t L = 0; L < idx->n_lists; ++L) {
    for (uint32_t r = 0; r < idx->h_list_sizes[L]; ++r, ++o) {
      const size_t fr = (size_t)idx->h_list_offsets[L] + r;
      pids[fr] = ids[o];
      for (size_t wd = 0; wd < W; ++wd) bits[((fr >> 5) * W + wd) * 32 + (fr & 31)] = rabitq_host::reverse_bits(bit_codes[o * W + wd]);
      sf[fr] = make_float4(short_fac[o * 3], short_fac[o * 3 + 1], short_fac[o * 3 + 2], 0.f);
      if (exb) memcpy(&exc[fr * exb], &ex_codes[o * exb], exb);
      ef[fr] = make_float2(ex_fac[o * 2], ex_fac[o * 2 + 1]);
    }
  }
  auto upload = [&](auto& dst, const auto& src) {
    using T = typename std::remove_reference_t<decltype(src)>::value_type;
    dst = dev_buf<T>::persistent(src.size());
    copy_async(res, dst.data(), src.data(), src.size() * sizeof(T));
  };
  upload(idx->rotation, rotation); upload(idx->centers_rot, centers_rot); upload(idx->bits, bits); upload(idx->short_fac, sf);
  upload(idx->ex_codes, exc); upload(idx->ex_fac, ef); upload(idx->ids, pids); upload(idx->list_sizes, idx->h_list_sizes);
  upload(idx->list_offsets, idx->h_list_offsets);
  idx->center_rot_norms = dev_buf<float>::persistent(idx->n_lists);
  row_norms<float>(res, idx->centers_rot.data(), idx->n_lists, idx->D, idx->D, idx->center_rot_norms.data(), false);
  sync(res);
  return idx;
}

ivf_rabitq_index& get_rbq(cuvsAmdIvfRabitqIndex_t index)
{
  CUVS_EXPECTS(index != nullptr && index->addr != 0, "IVF-RaBitQ index is not built");
  return *reinterpret_cast<ivf_rabitq_index*>(index->addr);
}

}  // namespace
}  // namespace cuvs_amd

using namespace cuvs_amd;

extern "C" {

cuvsError_t cuvsAmdIvfRabitqIndexParamsCreate(cuvsAmdIvfRabitqIndexParams_t* params)
{
  return (cuvsError_t)translate_exceptions(
    [=] { *params = new cuvsAmdIvfRabitqIndexParams{L2Expanded, 1024, 3, 20, 256, true, 100000, false}; });
}
cuvsError_t cuvsAmdIvfRabitqIndexParamsDestroy(cuvsAmdIvfRabitqIndexParams_t params)
{
  return (cuvsError_t)translate_exceptions([=] { delete params; });
}
cuvsError_t cuvsAmdIvfRabitqSearchParamsCreate(cuvsAmdIvfRabitqSearchParams_t* params)
{
  return (cuvsError_t)translate_exceptions([=] { *params = new cuvsAmdIvfRabitqSearchParams{20, CUVS_AMD_IVF_RABITQ_QUANT4}; });
}
cuvsError_t cuvsAmdIvfRabitqSearchParamsDestroy(cuvsAmdIvfRabitqSearchParams_t params)
{
  return (cuvsError_t)translate_exceptions([=] { delete params; });
}
cuvsError_t cuvsAmdIvfRabitqIndexCreate(cuvsAmdIvfRabitqIndex_t* index)
{
  return (cuvsError_t)translate_exceptions([=] { *index = new cuvsAmdIvfRabitqIndex{0, DLDataType{kDLFloat, 32, 1}}; });
}
cuvsError_t cuvsAmdIvfRabitqIndexDestroy(cuvsAmdIvfRabitqIndex_t index)
{
  return (cuvsError_t)translate_exceptions([=] {
    if (!index) return;
    delete reinterpret_cast<ivf_rabitq_index*>(index->addr);
    delete index;
  });
}
cuvsError_t cuvsAmdIvfRabitqIndexGetNLists(cuvsAmdIvfRabitqIndex_t index, int64_t* n_lists)
{
  return (cuvsError_t)translate_exceptions([=] { *n_lists = get_rbq(index).n_lists; });
}
cuvsError_t cuvsAmdIvfRabitqIndexGetDim(cuvsAmdIvfRabitqIndex_t index, int64_t* dim)
{
  return (cuvsError_t)translate_exceptions([=] { *dim = get_rbq(index).dim; });
}
cuvsError_t cuvsAmdIvfRabitqIndexGetSize(cuvsAmdIvfRabitqIndex_t index, int64_t* size)
{
  return (cuvsError_t)translate_exceptions([=] { *size = get_rbq(index).size; });
}
cuvsError_t cuvsAmdIvfRabitqIndexGetBitsPerDim(cuvsAmdIvfRabitqIndex_t index, int64_t* bits_per_dim)
{
  return (cuvsError_t)translate_exceptions([=] { *bits_per_dim = get_rbq(index).ex + 1; });
}

cuvsError_t cuvsAmdIvfRabitqBuild(cuvsResources_t res_h, cuvsAmdIvfRabitqIndexParams_t params, DLManagedTensor* dataset_tensor,
                                  cuvsAmdIvfRabitqIndex_t index)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& res = *as_res(res_h);
    CUVS_EXPECTS(params && dataset_tensor && index, "null argument");
    auto& ds = dataset_tensor->dl_tensor;
    CUVS_EXPECTS(dtype_is(ds.dtype, kDLFloat, 32), "ivf_rabitq::build: dataset must be float32 (DLtensor dtype %d, bits %d)", (int)ds.dtype.code,
                 (int)ds.dtype.bits);
    CUVS_EXPECTS(ds.ndim == 2 && is_c_contiguous(ds), "dataset must be a row-major matrix");
    auto idx = ivf_rabitq_build(res, *params, dl_data(ds), ds.shape[0], ds.shape[1], !is_device_accessible(ds));
    delete reinterpret_cast<ivf_rabitq_index*>(index->addr);
    index->addr = reinterpret_cast<uintptr_t>(idx.release());
  });
}

cuvsError_t cuvsAmdIvfRabitqSearch(cuvsResources_t res_h, cuvsAmdIvfRabitqSearchParams_t params, cuvsAmdIvfRabitqIndex_t index_c,
                                   DLManagedTensor* queries_tensor, DLManagedTensor* neighbors_tensor, DLManagedTensor* distances_tensor)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& res = *as_res(res_h);
    auto& idx = get_rbq(index_c);
    CUVS_EXPECTS(params && queries_tensor && neighbors_tensor && distances_tensor, "null argument");
    auto& queries   = queries_tensor->dl_tensor;
    auto& neighbors = neighbors_tensor->dl_tensor;
    auto& distances = distances_tensor->dl_tensor;
    CUVS_EXPECTS(is_device_accessible(queries), "queries should have device compatible memory");
    CUVS_EXPECTS(is_device_accessible(neighbors), "neighbors should have device compatible memory");
    CUVS_EXPECTS(is_device_accessible(distances), "distances should have device compatible memory");
    CUVS_EXPECTS(dtype_is(neighbors.dtype, kDLInt, 64), "neighbors should be of type int64_t");
    CUVS_EXPECTS(dtype_is(distances.dtype, kDLFloat, 32), "distances should be of type float32");
    CUVS_EXPECTS(dtype_is(queries.dtype, kDLFloat, 32), "ivf_rabitq::search: queries must be float32");
    CUVS_EXPECTS(queries.ndim == 2 && neighbors.ndim == 2 && distances.ndim == 2, "tensors must be 2-D");
    CUVS_EXPECTS(queries.shape[1] == idx.dim, "queries dim %ld != index dim %u", (long)queries.shape[1], idx.dim);
    const int64_t m = queries.shape[0], k = neighbors.shape[1];
    CUVS_EXPECTS(neighbors.shape[0] == m && distances.shape[0] == m && distances.shape[1] == k, "neighbors/distances shape mismatch");
    if (m == 0 || k == 0 || params->n_probes == 0) return;  // nothing to do: the outputs are not touched
    CUVS_EXPECTS(is_c_contiguous(queries) && is_c_contiguous(neighbors) && is_c_contiguous(distances), "tensors must be C-contiguous");
    ivf_rabitq_search(res, idx, params->n_probes, (int)params->mode, static_cast<const float*>(dl_data(queries)), m, (int)k,
                      static_cast<int64_t*>(dl_data(neighbors)), static_cast<float*>(dl_data(distances)));
  });
}

cuvsError_t cuvsAmdIvfRabitqSerialize(cuvsResources_t res_h, const char* filename, cuvsAmdIvfRabitqIndex_t index)
{
  return (cuvsError_t)translate_exceptions([=] { rbq_write(*as_res(res_h), filename, get_rbq(index)); });
}
cuvsError_t cuvsAmdIvfRabitqDeserialize(cuvsResources_t res_h, const char* filename, cuvsAmdIvfRabitqIndex_t index)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& res = *as_res(res_h);
    CUVS_EXPECTS(index != nullptr, "index is null");
    auto idx = rbq_read(res, filename);
    delete reinterpret_cast<ivf_rabitq_index*>(index->addr);
    index->addr = reinterpret_cast<uintptr_t>(idx.release());
  });
}

cuvsError_t cuvsAmdIvfRabitqExport(cuvsResources_t res_h, cuvsAmdIvfRabitqIndex_t index, float* centers_rot, float* rotation,
                                   uint32_t* list_sizes, uint32_t* ids, uint32_t* bit_codes, float* short_factors, uint8_t* ex_codes,
                                   float* ex_factors, float* t)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& res = *as_res(res_h);
    auto& idx = get_rbq(index);
    const rbq_host_arrays h = rbq_download(res, idx);
    auto put = [](void* dst, const auto& v) {
      if (dst != nullptr && !v.empty()) memcpy(dst, v.data(), v.size() * sizeof(v[0]));
    };
    put(centers_rot, h.centers_rot); put(rotation, h.rotation); put(list_sizes, idx.h_list_sizes); put(ids, h.ids);
    put(bit_codes, h.bit_codes); put(short_factors, h.short_fac); put(ex_codes, h.ex_codes); put(ex_factors, h.ex_fac);
    if (t != nullptr) *t = idx.t;
  });
}

cuvsError_t cuvsAmdIvfRabitqExportCenters(cuvsResources_t res_h, cuvsAmdIvfRabitqIndex_t index, float* centers)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& res = *as_res(res_h);
    auto& idx = get_rbq(index);
    CUVS_EXPECTS(idx.centers.data() != nullptr, "an IVF-RaBitQ index loaded from a file holds only the rotated centres");
    CUVS_EXPECTS(centers != nullptr, "centers is null");
    copy_async(res, centers, idx.centers.data(), idx.centers.bytes());
    sync(res);
  });
}

cuvsError_t cuvsAmdIvfRabitqScalingFactor(uint32_t padded_dim, uint32_t ex_bits, float* t)
{
  return (cuvsError_t)translate_exceptions([=] {
    CUVS_EXPECTS(t != nullptr, "t is null");
    CUVS_EXPECTS(padded_dim > 0 && padded_dim % 64 == 0 && padded_dim <= rabitq_host::kMaxDim, "padded_dim must be a multiple of 64 up to %lu",
                 (unsigned long)rabitq_host::kMaxDim);
    CUVS_EXPECTS(ex_bits <= 8, "ex_bits must be at most 8");
    *t = rbq_scaling_factor(padded_dim, ex_bits);
  });
}

cuvsError_t cuvsAmdIvfRabitqLastSearchStats(uint64_t out[4])
{
  return (cuvsError_t)translate_exceptions([=] {
    CUVS_EXPECTS(out != nullptr, "out is null");
    for (int i = 0; i < 4; ++i) out[i] = g_last_stats[i];
  });
}

}  // extern "C"
