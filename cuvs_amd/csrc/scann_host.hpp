// Host-only parts of the ScaNN index build (scann.hip): the parameter checks, the sizes of the samples and batches, the code
// unpacking, the label interleaving, the writer of the index files, and the checks and the list builder of the search
// (scann_search.hip). No HIP and no DLPack types in here:
// tests/cpp/scann_host_test.cpp builds this header alone under the sanitizers. The .npy records are byte for byte those of
// npy_writer::header (npy_io.hpp), restated so that this header stays free of the HIP runtime.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

namespace cuvs_amd {
namespace scann_host {

[[noreturn]] inline void refuse(const char* fmt, ...)
{
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  throw std::invalid_argument(buf);
}

constexpr int64_t kMaxBatchRows   = 65536;   // rows staged and processed at a time (scann_build.cuh:70)
constexpr int64_t kMaxPqTrainRows = 100000;  // scann_build.cuh:151
constexpr int32_t kSerializationVersion = 1;
constexpr int kMaxNoiseShapingRounds    = 10;

// scann.hpp:40-85 (names and defaults)
struct params {
  int metric                  = 0;
  float metric_arg            = 2.0f;
  uint32_t n_leaves           = 1000;
  int64_t kmeans_n_rows_train = 100000;
  uint32_t kmeans_n_iters     = 24;
  float partitioning_eta      = 1.0f;
  float soar_lambda           = 1.0f;
  uint32_t pq_dim             = 8;  // the WIDTH of a subspace: dim / pq_dim subspaces
  uint32_t pq_bits            = 8;
  int64_t pq_n_rows_train     = 100000;
  uint32_t pq_train_iters     = 10;
  bool reordering_bf16        = false;
  float reordering_noise_shaping_threshold = NAN;
};

inline void check_eta(float eta)
{
  if (!(eta > 0.0f) || !std::isfinite(eta)) refuse("partitioning_eta must be positive and finite, got %g", (double)eta);
}
inline void check_lambda(float lambda)
{
  if (!(lambda >= 0.0f) || !std::isfinite(lambda)) refuse("soar_lambda must be non-negative and finite, got %g", (double)lambda);
}

// scann.hpp:179-183 and the checks of this library
inline void check_params(const params& p, int64_t n_rows, int64_t dim)
{
  if (dim < 1) refuse("dataset must have at least one column");
  if (!(p.pq_bits == 4 || p.pq_bits == 8)) refuse("pq_bits must be 4 or 8, got %u", p.pq_bits);
  if (p.pq_dim < 1 || dim % p.pq_dim != 0)
    refuse("the dataset dimension (%lld) must be a multiple of pq_dim (%u)", (long long)dim, p.pq_dim);
  check_eta(p.partitioning_eta);
  check_lambda(p.soar_lambda);
  if (p.n_leaves < 1) refuse("n_leaves must be at least 1");
  if (n_rows < (int64_t)p.n_leaves) refuse("n_rows (%lld) must not be smaller than n_leaves (%u)", (long long)n_rows, p.n_leaves);
  if (p.kmeans_n_rows_train < (int64_t)p.n_leaves)
    refuse("kmeans_n_rows_train (%lld) must not be smaller than n_leaves (%u)", (long long)p.kmeans_n_rows_train, p.n_leaves);
  if (p.kmeans_n_iters < 1) refuse("kmeans_n_iters must be positive");
  if (p.pq_train_iters < 1) refuse("pq_train_iters must be positive");
  const int64_t book = int64_t(1) << p.pq_bits;
  if (std::min<int64_t>(p.pq_n_rows_train, n_rows) < book)
    refuse("pq_n_rows_train and n_rows must not be smaller than the %lld entries of a codebook", (long long)book);
}

inline int64_t kmeans_train_rows(const params& p, int64_t n_rows) { return std::min<int64_t>(p.kmeans_n_rows_train, n_rows); }
inline int64_t pq_train_rows(const params& p, int64_t n_rows)
{
  return std::min<int64_t>(std::min<int64_t>(p.pq_n_rows_train, kMaxPqTrainRows), n_rows);
}
// sample i of m is row i * (n / m): the strided rule of the product quantizer's trainsets (pq_quantize.hip pq_subsample)
inline int64_t sample_row(int64_t i, int64_t n, int64_t m) { return i * (n / m); }

// leaves whose dim x dim Gram matrices share the workspace at a time
inline int64_t avq_leaf_batch(int64_t n_leaves, int64_t dim, size_t workspace_bytes)
{
  const int64_t fit = (int64_t)(workspace_bytes / ((size_t)dim * (size_t)dim * sizeof(float)));
  return std::max<int64_t>(1, std::min<int64_t>(n_leaves, fit));
}
// the factorisation runs in LDS while the matrix and two vectors fit
inline bool avq_solve_in_lds(int64_t dim, size_t lds_bytes) { return (size_t)(dim * dim + 2 * dim) * sizeof(float) <= lds_bytes; }

// packed codes (code j in bits [j * bits, (j + 1) * bits) of the row, little endian) -> one byte per subspace
// (scann_quantize.cuh:74-95)
inline void unpack_codes(const uint8_t* packed, int64_t n, int64_t n_sub, int bits, uint8_t* out)
{
  const int64_t row_bytes = (n_sub * bits + 7) / 8;
  if (bits == 8) {
    for (int64_t i = 0; i < n * n_sub; ++i) out[i] = packed[i];
    return;
  }
  for (int64_t i = 0; i < n; ++i)
    for (int64_t j = 0; j < n_sub; ++j) {
      const uint8_t b     = packed[i * row_bytes + (j >> 1)];
      out[i * n_sub + j] = (j & 1) ? (uint8_t)(b >> 4) : (uint8_t)(b & 15);
    }
}

// datapoint_to_token: primary and SOAR label interleaved, SOAR = -1 where both agree (scann_serialize.cuh:64-96)
inline std::vector<int32_t> interleave_labels(const uint32_t* labels, const uint32_t* soar, int64_t n)
{
  std::vector<int32_t> out((size_t)(2 * n));
  for (int64_t i = 0; i < n; ++i) {
    out[2 * i]     = (int32_t)labels[i];
    out[2 * i + 1] = soar[i] == labels[i] ? -1 : (int32_t)soar[i];
  }
  return out;
}

// ---------------------------------------------------------------- .npy records
class npy_file {
 public:
  explicit npy_file(const std::string& name) : name_(name)
  {
    f_ = fopen(name.c_str(), "wb");
    if (f_ == nullptr) refuse("Cannot open file %s", name.c_str());
  }
  ~npy_file() { if (f_) fclose(f_); }
  npy_file(const npy_file&)            = delete;
  npy_file& operator=(const npy_file&) = delete;
  void record(char kind, uint32_t itemsize, const std::vector<int64_t>& shape, const void* data)
  {
    std::string d = std::string("{'descr': '") + (itemsize > 1 ? '<' : '|') + kind + std::to_string(itemsize) +
                    "', 'fortran_order': False, 'shape': (";
    size_t count = 1;
    for (size_t i = 0; i < shape.size(); i++) {
      d += std::to_string(shape[i]);
      if (shape.size() == 1) d += ",";
      else if (i + 1 < shape.size()) d += ", ";
      count *= (size_t)shape[i];
    }
    d += "), }";
    const size_t preamble = 6 + 2 + 2 + d.size() + 1;
    d.append((64 - preamble % 64) % 64, ' ');
    d += '\n';
    const unsigned char magic[8] = {0x93, 'N', 'U', 'M', 'P', 'Y', 1, 0};
    const uint16_t len           = (uint16_t)d.size();
    raw(magic, 8);
    raw(&len, 2);
    raw(d.data(), d.size());
    raw(data, count * itemsize);
  }
  void close()
  {
    const int rc = fclose(f_);
    f_           = nullptr;
    if (rc != 0) refuse("Error writing %s", name_.c_str());
  }

 private:
  void raw(const void* p, size_t n)
  {
    if (n && fwrite(p, 1, n, f_) != n) refuse("short write to %s", name_.c_str());
  }
  FILE* f_ = nullptr;
  std::string name_;
};

// every array of an index, on the host
struct host_index {
  int64_t n_rows = 0, dim = 0, n_leaves = 0, n_sub = 0, book_n = 0;
  uint32_t pq_dim = 0;
  const float* centers     = nullptr;  // [n_leaves, dim]
  const uint32_t* labels   = nullptr;  // [n_rows]
  const uint32_t* soar     = nullptr;  // [n_rows]
  const float* codebook    = nullptr;  // [book_n, dim]
  const uint8_t* codes     = nullptr;  // [n_rows, n_sub]
  const uint8_t* soar_codes = nullptr; // [n_rows, n_sub]
  const int16_t* bf16      = nullptr;  // [n_rows, dim] or nullptr
};

// the files of scann_serialize.cuh:107-142; `dir` must exist
inline void write_files(const std::string& dir, const host_index& h)
{
  if (dir.empty()) refuse("the directory name is empty");
  const std::string base = dir.back() == '/' ? dir : dir + "/";
  {
    npy_file f(base + "cuvs_metadata.bin");
    const int32_t version = kSerializationVersion;
    const uint32_t dim = (uint32_t)h.dim, pq_dim = h.pq_dim;
    f.record('i', 4, {}, &version);
    f.record('u', 4, {}, &dim);
    f.record('u', 4, {}, &pq_dim);
    f.close();
  }
  auto one = [&](const char* name, char kind, uint32_t itemsize, const std::vector<int64_t>& shape, const void* data) {
    npy_file f(base + name);
    f.record(kind, itemsize, shape, data);
    f.close();
  };
  one("centers.npy", 'f', 4, {h.n_leaves, h.dim}, h.centers);
  const std::vector<int32_t> tokens = interleave_labels(h.labels, h.soar, h.n_rows);
  one("datapoint_to_token.npy", 'i', 4, {2 * h.n_rows}, tokens.data());
  one("pq_codebook.npy", 'f', 4, {h.book_n, h.dim}, h.codebook);
  one("hashed_dataset.npy", 'u', 1, {h.n_rows, h.n_sub}, h.codes);
  one("hashed_dataset_soar.npy", 'u', 1, {h.n_rows, h.n_sub}, h.soar_codes);
  if (h.bf16 != nullptr) one("bf16_dataset.npy", 'i', 2, {h.n_rows, h.dim}, h.bf16);
}

// ---------------------------------------------------------------- search-side lists (scann_search.hip)
constexpr int kTileEntries      = 32;          // entries of a code tile: one matrix-core operand
constexpr uint32_t kNoRow       = 0xffffffffu; // row id of a padding entry
constexpr uint32_t kMaxReorder  = 4096;
constexpr int64_t kMaxSearchDim = 2048;        // the 32 staged query rows have to fit LDS

inline uint16_t bf16_rne_bits(float f)
{
  uint32_t u;
  std::memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}

inline void check_search(int metric, uint32_t n_probes, uint32_t n_reorder, int64_t k, bool has_bf16, int64_t dim, int64_t query_dim)
{
  if (!(metric == 0 || metric == 6)) refuse("ScaNN search serves L2Expanded and InnerProduct, the index records metric %d", metric);
  if (query_dim != dim) refuse("queries have %lld columns, the index has dim %lld", (long long)query_dim, (long long)dim);
  if (dim > kMaxSearchDim) refuse("ScaNN search serves up to %lld dimensions, the index has %lld", (long long)kMaxSearchDim, (long long)dim);
  if (n_probes < 1) refuse("n_probes must be positive");
  if (k < 1) refuse("k must be positive");
  if (n_reorder > kMaxReorder) refuse("n_reorder (%u) must not exceed %u", n_reorder, kMaxReorder);
  if (n_reorder > 0 && !has_bf16) refuse("n_reorder > 0 needs an index built with reordering_bf16 (cuvsRefine re-ranks against the caller's rows)");
  if (n_reorder > 0 && k > (int64_t)n_reorder) refuse("k (%lld) must not exceed n_reorder (%u)", (long long)k, n_reorder);
  if (n_reorder == 0 && k > (int64_t)kMaxReorder) refuse("k (%lld) must not exceed %u", (long long)k, kMaxReorder);
}

// Leaf j: an entry with the primary codes for every row whose label is j and one with the SOAR codes for every row whose SOAR
// label is j and differs from its label, in ascending row id. A leaf starts at a whole tile of 32 entries; entry p of a leaf is
// slot (tile_off[j] + p / 32) * 32 + p % 32 of ids and t, and its codes are byte s % 4 of words[(tile * n_words + s / 4) * 32 + p % 32]
// for subspace s: a tile's lanes read consecutive words. Subspaces past the last one (dimensions up to dim_pad) hold code 0 and
// meet the zero padding of the codebook rows.
struct search_lists {
  int64_t dim_pad = 0, n_words = 0, n_tiles = 0, n_spilled = 0;
  std::vector<uint32_t> leaf_size, tile_off;  // [n_leaves], [n_leaves + 1]
  std::vector<uint32_t> ids, words;           // [n_tiles * 32], [n_tiles * n_words * 32]
  std::vector<float> t;                       // [n_tiles * 32]: 2 <centre, r~> + |r~|^2 (L2; fp64 sums, rounded once), else 0
  std::vector<uint16_t> book_bf16;            // [book_n, dim_pad], zero-padded
};

inline search_lists build_search_lists(const host_index& h, bool l2)
{
  if (h.n_rows >= (int64_t)kNoRow) refuse("ScaNN search serves fewer than 2^32 - 1 rows");
  search_lists s;
  const int64_t W = h.pq_dim;
  s.dim_pad       = (h.dim + 15) / 16 * 16;
  s.n_words       = ((s.dim_pad - 1) / W) / 4 + 1;
  s.leaf_size.assign((size_t)h.n_leaves, 0);
  for (int64_t i = 0; i < h.n_rows; ++i) {
    if (h.labels[i] >= h.n_leaves || h.soar[i] >= h.n_leaves) refuse("row %lld has a label outside the %lld leaves", (long long)i, (long long)h.n_leaves);
    ++s.leaf_size[h.labels[i]];
    if (h.soar[i] != h.labels[i]) { ++s.leaf_size[h.soar[i]]; ++s.n_spilled; }
  }
  s.tile_off.assign((size_t)h.n_leaves + 1, 0);
  for (int64_t j = 0; j < h.n_leaves; ++j) s.tile_off[j + 1] = s.tile_off[j] + (s.leaf_size[j] + kTileEntries - 1) / kTileEntries;
  s.n_tiles = s.tile_off[h.n_leaves];
  s.ids.assign((size_t)s.n_tiles * kTileEntries, kNoRow);
  s.t.assign((size_t)s.n_tiles * kTileEntries, 0.0f);
  s.words.assign((size_t)(s.n_tiles * s.n_words) * kTileEntries, 0u);
  s.book_bf16.assign((size_t)(h.book_n * s.dim_pad), 0);
  for (int64_t e = 0; e < h.book_n; ++e)
    for (int64_t d = 0; d < h.dim; ++d) s.book_bf16[e * s.dim_pad + d] = bf16_rne_bits(h.codebook[e * h.dim + d]);
  std::vector<uint32_t> cursor((size_t)h.n_leaves, 0);
  auto put = [&](int64_t row, uint32_t leaf, const uint8_t* codes) {
    const uint32_t p    = cursor[leaf]++;
    const int64_t tile  = s.tile_off[leaf] + p / kTileEntries;
    const int64_t lane  = p % kTileEntries;
    s.ids[tile * kTileEntries + lane] = (uint32_t)row;
    double cr = 0.0, rr = 0.0;
    for (int64_t j = 0; j < h.n_sub; ++j) {
      if (codes[j] >= h.book_n) refuse("row %lld has a code outside the %lld entries of the codebook", (long long)row, (long long)h.book_n);
      s.words[(tile * s.n_words + j / 4) * kTileEntries + lane] |= (uint32_t)codes[j] << (8 * (j % 4));
      for (int64_t d = j * W; d < (j + 1) * W; ++d) {
        const double r = h.codebook[(int64_t)codes[j] * h.dim + d];
        cr += (double)h.centers[(int64_t)leaf * h.dim + d] * r;
        rr += r * r;
      }
    }
    if (l2) s.t[tile * kTileEntries + lane] = (float)(2.0 * cr + rr);
  };
  for (int64_t i = 0; i < h.n_rows; ++i) {
    put(i, h.labels[i], h.codes + i * h.n_sub);
    if (h.soar[i] != h.labels[i]) put(i, h.soar[i], h.soar_codes + i * h.n_sub);
  }
  return s;
}

}  // namespace scann_host
}  // namespace cuvs_amd
