// Host-only parts of the ScaNN index build (scann.hip): the parameter checks, the sizes of the samples and batches, the code
// unpacking, the label interleaving and the writer of the index files. No HIP and no DLPack types in here:
// tests/cpp/scann_host_test.cpp builds this header alone under the sanitizers. The .npy records are byte for byte those of
// npy_writer::header (npy_io.hpp), restated so that this header stays free of the HIP runtime.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
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

}  // namespace scann_host
}  // namespace cuvs_amd
