// HNSW on the host: the index, its search, its insert and its files - what <cuvs/neighbors/hnsw.h> serves once a
// CAGRA graph has left the device. Pure C++17, no HIP include: hnsw.hip, tests/cpp/hnsw_host_test.cpp (under the sanitizers)
// and nothing else include it. Written against the published algorithm (Malkov & Yashunin) and hnswlib's saveIndex layout as
// the reference documents it (cagra_serialize.cuh:98-258, detail/hnsw.hpp:375-700, cmake/patches/hnswlib.diff for the
// base-layer-only seeding); hnswlib itself is not used. tests/hnsw_ref.py restates every rule below in numpy.
//
// Memory: level 0 is kept as the file keeps it, one record {uint32 count, uint32 links[maxM0], row, uint64 label} per row
// (records are not padded: for odd dims of 1- and 2-byte rows the words are unaligned and go through memcpy); the levels above
// are one block {uint32 count, uint32 links[maxM]} per level and row.
//
// Order: every comparison is on the pair (distance, id), so neither the heap implementation nor the thread count shows in a
// result. Distances: fp32 / fp16 rows in fp32 summed in index order without contraction, int8 / uint8 rows in exact int32;
// inner product is 1 - sum.
//
// Insert (extend, CPU hierarchy): sequential, in id order; num_threads of the C structs is accepted and unused.
//   level(i)  = #{k >= 1 : h(i) < T_k}, T_k = floor(2^32 M^-k) by repeated division in double, h a fixed 32-bit hash of (100, i)
//   greedy    : through the levels above the row's own, scanning a list in stored order, moving on strictly smaller distance
//   per level : W = search_layer(ef_construction); the row's list = heuristic(W, M); every chosen neighbour gets the row
//               appended, or, its list being full, its list and the row re-pruned by the heuristic at the list's cap
//               (maxM0 = 2 M at level 0, M above); the next level starts from W's nearest
//   heuristic : candidates ascending; one is kept unless a kept one is strictly nearer to it than the base is
//   entry     : a row whose level is at least the top level becomes the entry point (the largest id on the top level)
#pragma once
#include "mix_hash.hpp"

#include <algorithm>
#include <atomic>
#include <cfloat>
#include <cstdarg>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <queue>
#include <stdexcept>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#if defined(__HIPCC__)
#define CUVS_AMD_HNSW_HD __host__ __device__
#else
#define CUVS_AMD_HNSW_HD
#endif

namespace cuvs_amd {
namespace hnsw {

enum : int { H_NONE = 0, H_CPU = 1, H_GPU = 2 };          // cuvsHnswHierarchy
enum : int { T_F32 = 0, T_F16 = 1, T_I8 = 2, T_U8 = 3 };  // the order of elem_t (common.hpp)
enum : int { METRIC_L2 = 0, METRIC_IP = 6 };              // L2Expanded, InnerProduct
constexpr uint32_t kLevelSeed   = 100;
constexpr int kMaxLevels        = 32;
constexpr int kBaseSeeds        = 32;  // starts of a base-layer-only search (hnswlib.diff: num_seeds)
constexpr size_t kHeaderBytes   = 96;
constexpr double kBaseOnlyMult  = 0.42424242;  // what cuvsCagraSerializeToHnswlib writes (cagra_serialize.cuh)
constexpr size_t kBaseOnlyEfCon = 500;

[[noreturn]] inline void hfail(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
inline void hfail(const char* fmt, ...)
{
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  throw std::runtime_error(buf);
}

// ---------------------------------------------------------------- levels
// (the finalizer of MurmurHash3 over i + seed * golden ratio: mix_hash.hpp, shared with the ball cover's landmark draw)
CUVS_AMD_HNSW_HD inline uint32_t level_hash(uint32_t seed, uint32_t i) { return mix_hash(seed, i); }
struct level_rule {
  uint32_t t[kMaxLevels];  // T_1 .. T_count, strictly decreasing, all > 0
  int count;
};
inline level_rule make_level_rule(size_t M)
{
  level_rule r{};
  if (M < 2) return r;  // a flat index
  double t = 4294967296.0;
  while (r.count < kMaxLevels) {
    t /= (double)M;
    const double f = std::floor(t);
    if (f < 1.0) break;
    r.t[r.count++] = (uint32_t)f;
  }
  return r;
}
CUVS_AMD_HNSW_HD inline int level_of(const level_rule& r, uint32_t i)
{
  const uint32_t h = level_hash(kLevelSeed, i);
  int l = 0;
  while (l < r.count && h < r.t[l]) ++l;
  return l;
}

// ---------------------------------------------------------------- distances
inline float half_to_float(uint16_t h)
{
  const uint32_t sign = (uint32_t)(h & 0x8000u) << 16;
  uint32_t exp = (h >> 10) & 0x1Fu, man = h & 0x3FFu, bits;
  if (exp == 0) {
    if (man == 0) {
      bits = sign;
    } else {  // subnormal: normalise
      int e = -1;
      do { ++e; man <<= 1; } while ((man & 0x400u) == 0);
      bits = sign | ((uint32_t)(127 - 15 - e) << 23) | ((man & 0x3FFu) << 13);
    }
  } else if (exp == 31) {
    bits = sign | 0x7F800000u | (man << 13);
  } else {
    bits = sign | ((exp + 127 - 15) << 23) | (man << 13);
  }
  float f;
  memcpy(&f, &bits, 4);
  return f;
}
struct f16 { uint16_t v; };
inline float as_float(float x) { return x; }
inline float as_float(f16 x) { return half_to_float(x.v); }

template <typename T>
float dist_l2_f(const void* a, const void* b, size_t dim)
{
  const T* x = static_cast<const T*>(a);
  const T* y = static_cast<const T*>(b);
  float s = 0.f;
  for (size_t i = 0; i < dim; ++i) {
    const float t = as_float(x[i]) - as_float(y[i]);
    const float p = t * t;
    s += p;
  }
  return s;
}
template <typename T>
float dist_ip_f(const void* a, const void* b, size_t dim)
{
  const T* x = static_cast<const T*>(a);
  const T* y = static_cast<const T*>(b);
  float s = 0.f;
  for (size_t i = 0; i < dim; ++i) {
    const float p = as_float(x[i]) * as_float(y[i]);
    s += p;
  }
  return 1.0f - s;
}
template <typename T>
float dist_l2_i(const void* a, const void* b, size_t dim)
{
  const T* x = static_cast<const T*>(a);
  const T* y = static_cast<const T*>(b);
  int32_t s = 0;
  for (size_t i = 0; i < dim; ++i) {
    const int32_t t = (int32_t)x[i] - (int32_t)y[i];
    s += t * t;
  }
  return (float)s;
}
template <typename T>
float dist_ip_i(const void* a, const void* b, size_t dim)
{
  const T* x = static_cast<const T*>(a);
  const T* y = static_cast<const T*>(b);
  int32_t s = 0;
  for (size_t i = 0; i < dim; ++i) s += (int32_t)x[i] * (int32_t)y[i];
  return 1.0f - (float)s;
}
using dist_fn = float (*)(const void*, const void*, size_t);
inline dist_fn pick_dist(int dtype, int metric)
{
  if (metric != METRIC_L2 && metric != METRIC_IP) hfail("Unsupported metric type was used");
  const bool l2 = metric == METRIC_L2;
  switch (dtype) {
    case T_F32: return l2 ? dist_l2_f<float> : dist_ip_f<float>;
    case T_F16: return l2 ? dist_l2_f<f16> : dist_ip_f<f16>;
    case T_I8: return l2 ? dist_l2_i<int8_t> : dist_ip_i<int8_t>;
    case T_U8: return l2 ? dist_l2_i<uint8_t> : dist_ip_i<uint8_t>;
    default: hfail("Unsupported dtype: %d", dtype);
  }
}
inline size_t dtype_size(int dtype) { return dtype == T_F32 ? 4 : (dtype == T_F16 ? 2 : 1); }

// ---------------------------------------------------------------- index
inline uint32_t ld32(const char* p) { uint32_t v; memcpy(&v, p, 4); return v; }
inline void st32(char* p, uint32_t v) { memcpy(p, &v, 4); }

struct index {
  int dtype = T_F32, metric = METRIC_L2, hierarchy = H_NONE;
  size_t dim = 0, n = 0, max_elements = 0;
  size_t M = 0, maxM = 0, maxM0 = 0, ef_construction = 0;
  double mult   = 0;
  int maxlevel  = 0;   // as the file holds it (1 in a base-layer-only file, whose rows all have level 0)
  uint32_t entry = 0;
  size_t per_elem = 0, offset_data = 0, label_offset = 0;
  dist_fn dist = nullptr;
  std::vector<char> level0;                  // [n, per_elem]
  std::vector<int32_t> levels;               // [n]
  std::vector<std::vector<uint32_t>> upper;  // row i: levels[i] blocks of 1 + maxM words

  void set_shape()
  {
    offset_data  = 4 * maxM0 + 4;
    per_elem     = offset_data + dim * dtype_size(dtype) + 8;
    label_offset = per_elem - 8;
    dist         = pick_dist(dtype, metric);
  }
  const char* rec(size_t i) const { return level0.data() + i * per_elem; }
  char* rec(size_t i) { return level0.data() + i * per_elem; }
  const void* row(size_t i) const { return rec(i) + offset_data; }
  uint64_t label(size_t i) const { uint64_t v; memcpy(&v, rec(i) + label_offset, 8); return v; }
  size_t cap(int level) const { return level == 0 ? maxM0 : maxM; }
  // the list of row i at `level`: count, then the ids (through ld32: a level-0 record may be unaligned)
  const char* list(size_t i, int level) const
  {
    return level == 0 ? rec(i) : reinterpret_cast<const char*>(upper[i].data() + (size_t)(level - 1) * (maxM + 1));
  }
  char* list(size_t i, int level) { return const_cast<char*>(static_cast<const index*>(this)->list(i, level)); }
  void set_list(size_t i, int level, const uint32_t* ids, size_t count)
  {
    char* p = list(i, level);
    st32(p, (uint32_t)count);
    for (size_t j = 0; j < cap(level); ++j) st32(p + 4 + 4 * j, j < count ? ids[j] : 0u);
  }
};

// an index of n rows over a graph of `degree` links per row, its records still to be filled (make_record or a copy of packed
// records into level0); the levels follow the rule unless the hierarchy is NONE
inline std::unique_ptr<index> make_index(int dtype, int metric, int hierarchy, size_t dim, size_t n, size_t degree,
                                         size_t ef_construction)
{
  auto ix = std::make_unique<index>();
  ix->dtype = dtype; ix->metric = metric; ix->hierarchy = hierarchy;
  ix->dim = dim; ix->n = n; ix->max_elements = n;
  if (hierarchy == H_NONE) {  // the header of cuvsCagraSerializeToHnswlib
    ix->M = ix->maxM = degree / 2;
    ix->maxM0 = degree;
    ix->mult = kBaseOnlyMult;
    ix->ef_construction = kBaseOnlyEfCon;
    ix->maxlevel = 1;
    ix->entry = (uint32_t)(n / 2);
  } else {
    ix->M = ix->maxM = (degree + 1) / 2;
    ix->maxM0 = 2 * ix->M;
    ix->mult = ix->M >= 2 ? 1.0 / std::log((double)ix->M) : 0.0;
    ix->ef_construction = ef_construction;
    ix->maxlevel = -1;  // set by finish_levels / the inserts
  }
  ix->set_shape();
  ix->level0.assign(n * ix->per_elem, 0);
  ix->levels.assign(n, 0);
  ix->upper.resize(n);
  return ix;
}
inline void make_record(index& ix, size_t i, const uint32_t* links, size_t count, const void* row)
{
  ix.set_list(i, 0, links, count);
  memcpy(ix.rec(i) + ix.offset_data, row, ix.dim * dtype_size(ix.dtype));
  const uint64_t label = i;
  memcpy(ix.rec(i) + ix.label_offset, &label, 8);
}
// levels by the rule for rows [first, n), their (empty) upper blocks
inline void assign_levels(index& ix, size_t first)
{
  const level_rule r = make_level_rule(ix.M);
  for (size_t i = first; i < ix.n; ++i) {
    ix.levels[i] = level_of(r, (uint32_t)i);
    ix.upper[i].assign((size_t)ix.levels[i] * (ix.maxM + 1), 0u);
  }
}
// entry point and top level of a finished hierarchy: the largest id on the highest level
inline void set_entry_from_levels(index& ix)
{
  ix.maxlevel = 0; ix.entry = 0;
  for (size_t i = 0; i < ix.n; ++i)
    if (ix.levels[i] >= ix.maxlevel) { ix.maxlevel = ix.levels[i]; ix.entry = (uint32_t)i; }
}

// ---------------------------------------------------------------- search
using cand_t = std::pair<float, uint32_t>;  // compared as (distance, id)

struct visited_list {
  std::vector<uint32_t> stamp;
  uint32_t epoch = 0;
  void begin(size_t n)
  {
    if (stamp.size() < n) { stamp.assign(n, 0u); epoch = 0; }
    if (++epoch == 0) { std::fill(stamp.begin(), stamp.end(), 0u); epoch = 1; }
  }
  bool test_and_set(uint32_t i)
  {
    if (stamp[i] == epoch) return true;
    stamp[i] = epoch;
    return false;
  }
};

inline void greedy_step(const index& ix, const void* q, int level, uint32_t& cur, float& curd)
{
  bool changed = true;
  while (changed) {
    changed = false;
    const char* l = ix.list(cur, level);
    const uint32_t cnt = ld32(l);
    for (uint32_t j = 0; j < cnt; ++j) {
      const uint32_t c = ld32(l + 4 + 4 * j);
      const float d = ix.dist(q, ix.row(c), ix.dim);
      if (d < curd) { curd = d; cur = c; changed = true; }
    }
  }
}

// best-first search of one level from one entry; out: at most ef rows, ascending
inline void search_layer(const index& ix, const void* q, uint32_t ep, float epd, size_t ef, int level, visited_list& vis,
                         std::vector<cand_t>& out)
{
  std::priority_queue<cand_t> top;
  std::priority_queue<cand_t, std::vector<cand_t>, std::greater<cand_t>> cand;
  vis.begin(ix.n);
  vis.test_and_set(ep);
  top.emplace(epd, ep);
  cand.emplace(epd, ep);
  while (!cand.empty()) {
    const cand_t c = cand.top();
    if (top.size() >= ef && c > top.top()) break;
    cand.pop();
    const char* l = ix.list(c.second, level);
    const uint32_t cnt = ld32(l);
    for (uint32_t j = 0; j < cnt; ++j) {
      const uint32_t e = ld32(l + 4 + 4 * j);
      if (vis.test_and_set(e)) continue;
      const cand_t p(ix.dist(q, ix.row(e), ix.dim), e);
      if (top.size() < ef || p < top.top()) {
        cand.push(p);
        top.push(p);
        if (top.size() > ef) top.pop();
      }
    }
  }
  out.resize(top.size());
  for (size_t i = top.size(); i-- > 0;) { out[i] = top.top(); top.pop(); }
}

inline void search_one(const index& ix, const void* q, size_t k, size_t ef, visited_list& vis, std::vector<cand_t>& w,
                       uint64_t* ids, float* dists)
{
  uint32_t cur = ix.entry;
  float curd   = ix.dist(q, ix.row(cur), ix.dim);
  if (ix.hierarchy == H_NONE) {
    for (int i = 0; i < kBaseSeeds; ++i) {
      const size_t s = (size_t)i * (ix.max_elements / kBaseSeeds);
      if (s >= ix.n) continue;
      const float d = ix.dist(q, ix.row(s), ix.dim);
      if (d < curd) { curd = d; cur = (uint32_t)s; }
    }
  } else {
    for (int l = ix.maxlevel; l >= 1; --l) greedy_step(ix, q, l, cur, curd);
  }
  search_layer(ix, q, cur, curd, std::max(ef, k), 0, vis, w);
  for (size_t j = 0; j < k; ++j) {
    if (j < w.size()) { ids[j] = ix.label(w[j].second); dists[j] = w[j].first; }
    else { ids[j] = UINT64_MAX; dists[j] = FLT_MAX; }
  }
}

inline int resolve_threads(int num_threads)
{
  if (num_threads > 0) return num_threads;
  if (const char* e = getenv("OMP_NUM_THREADS")) {
    const int v = atoi(e);
    if (v > 0) return v;
  }
  const unsigned hc = std::thread::hardware_concurrency();
  return hc > 0 ? (int)hc : 1;
}

// queries [nq, dim] of the index's dtype; ids [nq, k], dists [nq, k]. Reads the index only: concurrent calls are safe.
inline void search(const index& ix, const void* queries, size_t nq, size_t k, size_t ef, int num_threads, uint64_t* ids,
                   float* dists)
{
  if (ix.n == 0) hfail("the HNSW index is empty");
  if (k == 0 || nq == 0) return;
  const size_t qbytes = ix.dim * dtype_size(ix.dtype);
  const int nt = (int)std::min<size_t>((size_t)resolve_threads(num_threads), nq);
  std::atomic<size_t> next{0};
  auto work = [&] {
    visited_list vis;
    std::vector<cand_t> w;
    for (;;) {
      const size_t q0 = next.fetch_add(8);
      if (q0 >= nq) break;
      for (size_t i = q0; i < std::min(nq, q0 + 8); ++i)
        search_one(ix, static_cast<const char*>(queries) + i * qbytes, k, ef, vis, w, ids + i * k, dists + i * k);
    }
  };
  if (nt <= 1) { work(); return; }
  std::vector<std::thread> pool;
  for (int t = 0; t < nt; ++t) pool.emplace_back(work);
  for (auto& t : pool) t.join();
}

// ---------------------------------------------------------------- insert
inline void heuristic(const index& ix, const std::vector<cand_t>& c, size_t cap, std::vector<uint32_t>& out)
{
  out.clear();
  for (const cand_t& p : c) {
    if (out.size() >= cap) break;
    bool keep = true;
    for (uint32_t r : out)
      if (ix.dist(ix.row(p.second), ix.row(r), ix.dim) < p.first) { keep = false; break; }
    if (keep) out.push_back(p.second);
  }
}

struct inserter {
  visited_list vis;
  std::vector<cand_t> w, c;
  std::vector<uint32_t> sel, sel2;
};

// links row q (its record, level and empty upper blocks in place) into the levels min_level .. levels[q]
inline void insert(index& ix, uint32_t q, int min_level, inserter& s)
{
  const int L = ix.levels[q];
  if (ix.maxlevel < 0) {  // the first row of a hierarchy
    ix.maxlevel = L; ix.entry = q;
    return;
  }
  const void* qrow = ix.row(q);
  uint32_t cur = ix.entry;
  float curd   = ix.dist(qrow, ix.row(cur), ix.dim);
  for (int l = ix.maxlevel; l > L; --l) greedy_step(ix, qrow, l, cur, curd);
  for (int l = std::min(L, ix.maxlevel); l >= min_level; --l) {
    search_layer(ix, qrow, cur, curd, std::max<size_t>(ix.ef_construction, 1), l, s.vis, s.w);
    heuristic(ix, s.w, ix.M, s.sel);
    ix.set_list(q, l, s.sel.data(), s.sel.size());
    for (uint32_t nb : s.sel) {
      char* lst = ix.list(nb, l);
      const uint32_t cnt = ld32(lst);
      if (cnt < ix.cap(l)) {
        st32(lst + 4 + 4 * (size_t)cnt, q);
        st32(lst, cnt + 1);
        continue;
      }
      s.c.clear();
      for (uint32_t j = 0; j < cnt; ++j) {
        const uint32_t e = ld32(lst + 4 + 4 * (size_t)j);
        s.c.emplace_back(ix.dist(ix.row(nb), ix.row(e), ix.dim), e);
      }
      s.c.emplace_back(ix.dist(ix.row(nb), qrow, ix.dim), q);
      std::sort(s.c.begin(), s.c.end());
      heuristic(ix, s.c, ix.cap(l), s.sel2);
      ix.set_list(nb, l, s.sel2.data(), s.sel2.size());
    }
    cur = s.w[0].second; curd = s.w[0].first;
  }
  if (L >= ix.maxlevel) { ix.maxlevel = L; ix.entry = q; }
}

// the CPU hierarchy: level 0 is given (the CAGRA graph); rows of level >= 1 are inserted into the levels >= 1 only, in id order
inline void build_cpu_hierarchy(index& ix)
{
  assign_levels(ix, 0);
  ix.maxlevel = -1;
  inserter s;
  for (size_t i = 0; i < ix.n; ++i)
    if (ix.levels[i] >= 1) insert(ix, (uint32_t)i, 1, s);
  if (ix.maxlevel < 0) set_entry_from_levels(ix);  // no row above level 0
}

// m more rows of the index's dtype, linked into every level
inline void extend(index& ix, const void* rows, size_t m)
{
  if (ix.hierarchy == H_NONE) hfail("cuvsHnswExtend: a base-layer-only index (hierarchy NONE) is immutable and cannot be extended");
  if (ix.n + m >= 0xFFFFFFFFull) hfail("cuvsHnswExtend: at most 2^32 - 2 rows");
  const size_t n0 = ix.n, rb = ix.dim * dtype_size(ix.dtype);
  ix.n = n0 + m;
  ix.max_elements = std::max(ix.max_elements, ix.n);
  ix.level0.resize(ix.n * ix.per_elem, 0);
  ix.levels.resize(ix.n, 0);
  ix.upper.resize(ix.n);
  for (size_t i = n0; i < ix.n; ++i) make_record(ix, i, nullptr, 0, static_cast<const char*>(rows) + (i - n0) * rb);
  assign_levels(ix, n0);
  inserter s;
  for (size_t i = n0; i < ix.n; ++i) insert(ix, (uint32_t)i, 0, s);
}

// ---------------------------------------------------------------- files (hnswlib saveIndex)
struct file_closer {
  FILE* f;
  ~file_closer() { if (f) fclose(f); }
};

inline void save(const index& ix, const char* filename)
{
  if (filename == nullptr) hfail("filename is null");
  FILE* f = fopen(filename, "wb");
  if (f == nullptr) hfail("Cannot open file %s", filename);
  file_closer guard{f};
  auto put = [&](const void* p, size_t bytes) {
    if (bytes && fwrite(p, 1, bytes, f) != bytes) hfail("Error writing HNSW file %s", filename);
  };
  const size_t hdr[6] = {0, ix.max_elements, ix.n, ix.per_elem, ix.label_offset, ix.offset_data};
  put(hdr, sizeof(hdr));
  const int32_t maxlevel = ix.maxlevel, entry = (int32_t)ix.entry;
  put(&maxlevel, 4);
  put(&entry, 4);
  const size_t m[3] = {ix.maxM, ix.maxM0, ix.M};
  put(m, sizeof(m));
  put(&ix.mult, 8);
  put(&ix.ef_construction, 8);
  put(ix.level0.data(), ix.n * ix.per_elem);
  std::vector<uint32_t> buf;
  for (size_t i = 0; i < ix.n; ++i) {  // uint32 bytes of the row's upper blocks, then the blocks
    buf.push_back((uint32_t)(ix.upper[i].size() * 4));
    buf.insert(buf.end(), ix.upper[i].begin(), ix.upper[i].end());
    if (buf.size() >= (1u << 18) || i + 1 == ix.n) { put(buf.data(), buf.size() * 4); buf.clear(); }
  }
  const int rc = fclose(f);
  guard.f = nullptr;
  if (rc != 0) hfail("Error writing output %s", filename);
}

// The file is untrusted: every size, count and id is checked before it is used.
inline std::unique_ptr<index> load(const char* filename, int dim, int metric, int dtype, int hierarchy)
{
  if (filename == nullptr) hfail("filename is null");
  if (dim <= 0) hfail("cuvsHnswDeserialize: dim must be positive (got %d)", dim);
  if (hierarchy != H_NONE && hierarchy != H_CPU && hierarchy != H_GPU) hfail("cuvsHnswDeserialize: unknown hierarchy %d", hierarchy);
  (void)pick_dist(dtype, metric);
  FILE* f = fopen(filename, "rb");
  if (f == nullptr) hfail("Cannot open file %s", filename);
  file_closer guard{f};
  if (fseek(f, 0, SEEK_END) != 0) hfail("HNSW file %s: cannot seek", filename);
  const long end = ftell(f);
  if (end < 0 || fseek(f, 0, SEEK_SET) != 0) hfail("HNSW file %s: cannot seek", filename);
  size_t left = (size_t)end;
  auto get = [&](void* p, size_t bytes) {
    if (bytes > left) hfail("HNSW file %s has the wrong length: it ends %zu bytes early", filename, bytes - left);
    if (bytes && fread(p, 1, bytes, f) != bytes) hfail("Error reading HNSW file %s", filename);
    left -= bytes;
  };
  if (left < kHeaderBytes) hfail("HNSW file %s has the wrong length: %zu bytes, the header alone takes %zu", filename, left, kHeaderBytes);
  size_t hdr[6], m[3], efc;
  int32_t maxlevel, entry;
  double mult;
  get(hdr, sizeof(hdr));
  get(&maxlevel, 4);
  get(&entry, 4);
  get(m, sizeof(m));
  get(&mult, 8);
  get(&efc, 8);
  auto ix = std::make_unique<index>();
  ix->dtype = dtype; ix->metric = metric; ix->hierarchy = hierarchy; ix->dim = (size_t)dim;
  ix->max_elements = hdr[1]; ix->n = hdr[2];
  ix->maxM = m[0]; ix->maxM0 = m[1]; ix->M = m[2];
  ix->mult = mult; ix->ef_construction = efc;
  if (ix->maxM0 > (1u << 16) || ix->maxM > (1u << 16) || ix->M > (1u << 16))
    hfail("HNSW file %s: link list caps %zu / %zu / %zu are out of range", filename, ix->maxM, ix->maxM0, ix->M);
  ix->set_shape();
  if (hdr[0] != 0 || hdr[3] != ix->per_elem || hdr[4] != ix->label_offset || hdr[5] != ix->offset_data)
    hfail("HNSW file %s: a record of %zu bytes (links at %zu, row at %zu, label at %zu) does not fit dim %d of %zu-byte elements and "
          "%zu links, which take %zu",
          filename, hdr[3], hdr[0], hdr[5], hdr[4], dim, dtype_size(dtype), ix->maxM0, ix->per_elem);
  if (ix->n == 0 || ix->n >= 0xFFFFFFFFull || ix->n > ix->max_elements)
    hfail("HNSW file %s: %zu rows of at most %zu is out of range", filename, ix->n, ix->max_elements);
  if (ix->n > left / ix->per_elem) hfail("HNSW file %s has the wrong length: %zu bytes left for %zu records of %zu", filename, left, ix->n, ix->per_elem);
  if (maxlevel < 0 || maxlevel > kMaxLevels) hfail("HNSW file %s: top level %d is out of range", filename, (int)maxlevel);
  if (entry < 0 || (size_t)entry >= ix->n) hfail("HNSW file %s: entry point %d is out of range (%zu rows)", filename, (int)entry, ix->n);
  ix->maxlevel = maxlevel; ix->entry = (uint32_t)entry;
  ix->level0.resize(ix->n * ix->per_elem);
  get(ix->level0.data(), ix->level0.size());
  const size_t n = ix->n;
  auto check_list = [&](const char* l, size_t cap, size_t row, int level) {
    const uint32_t cnt = ld32(l);
    if (cnt > cap) hfail("HNSW file %s: row %zu lists %u links at level %d, the cap is %zu", filename, row, cnt, level, cap);
    for (uint32_t j = 0; j < cnt; ++j)
      if (ld32(l + 4 + 4 * (size_t)j) >= n) hfail("HNSW file %s: row %zu links to %u at level %d, the index has %zu rows", filename, row, ld32(l + 4 + 4 * (size_t)j), level, n);
  };
  for (size_t i = 0; i < n; ++i) check_list(ix->rec(i), ix->maxM0, i, 0);
  ix->levels.assign(n, 0);
  ix->upper.resize(n);
  const size_t block = 4 * ix->maxM + 4;
  for (size_t i = 0; i < n; ++i) {
    uint32_t bytes;
    get(&bytes, 4);
    if (bytes % block != 0 || bytes / block > (size_t)maxlevel)
      hfail("HNSW file %s: row %zu holds %u bytes of upper links, which is no level in 0..%d of %zu-byte blocks", filename, i, bytes, (int)maxlevel, block);
    if (bytes > left) hfail("HNSW file %s has the wrong length: it ends %zu bytes early", filename, bytes - left);
    ix->levels[i] = (int32_t)(bytes / block);
    ix->upper[i].resize(bytes / 4);
    get(ix->upper[i].data(), bytes);
  }
  if (left != 0) hfail("HNSW file %s has the wrong length: %zu bytes follow the last row", filename, left);
  for (size_t i = 0; i < n; ++i)
    for (int l = 1; l <= ix->levels[i]; ++l) {
      const char* lst = ix->list(i, l);
      check_list(lst, ix->maxM, i, l);
      for (uint32_t j = 0; j < ld32(lst); ++j) {
        const uint32_t e = ld32(lst + 4 + 4 * (size_t)j);
        if (ix->levels[e] < l) hfail("HNSW file %s: row %zu links at level %d to row %u of level %d", filename, i, l, e, (int)ix->levels[e]);
      }
    }
  if (hierarchy != H_NONE && ix->levels[ix->entry] < ix->maxlevel)
    hfail("HNSW file %s: entry point %u has level %d, the top level is %d (a base-layer-only file is read with hierarchy NONE)",
          filename, ix->entry, (int)ix->levels[ix->entry], ix->maxlevel);
  return ix;
}

}  // namespace hnsw
}  // namespace cuvs_amd
