// Host-only parts of IVF-RaBitQ (no HIP headers: a stand-alone program can compile this file with a sanitizer and run it over
// damaged files): the file header's parsing and validation, the section sizes, the bit-stream conversions between the file and
// the in-memory layout, and the constant scaling factor t of the extended codes. DESIGN.md 3.1s.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

namespace cuvs_amd {
namespace rabitq_host {

constexpr uint64_t kMaxLists = uint64_t(1) << 24;
constexpr uint64_t kMaxDim   = 4096;  // the screen stages 32 quantized queries of the padded dimension in the LDS

[[noreturn]] inline void bad_file(const std::string& what) { throw std::runtime_error("ivf_rabitq::deserialize: " + what); }

inline uint64_t padded_dim(uint64_t dim) { return (dim + 63) / 64 * 64; }

// File layout (the reference's IVFGPU::save): four size_t n, dim, n_lists, ex_bits; one bool; two floats; n_lists size_t list
// sizes; rotation [D, D] fp32; rotated centres [n_lists, D] fp32; bit codes [n, D / 32] uint32 (dimension 32 w + i at bit 31 - i);
// short factors [n, 3] fp32; ex codes [n, D ex / 8] bytes (MSB-first); ex factors [n, 2] fp32; ids [n] uint32. Rows in list order.
// The two floats: the scaling factor t of the extended codes, and the metric (0: L2Expanded, 1: L2SqrtExpanded) - the reference
// keeps two query scaling constants there that this library has no use for; a file of the reference therefore loads as L2Expanded
// (any second float other than 1), and its first float is taken for t, which only a build uses.
struct file_header {
  uint64_t n = 0, dim = 0, n_lists = 0, ex_bits = 0;
  uint64_t D = 0;
  float t = 0.f;
  int metric = 0;
  std::vector<uint64_t> sizes;
  // byte offsets of the sections that follow the list sizes
  uint64_t off_rotation = 0, off_centers = 0, off_bits = 0, off_short = 0, off_ex = 0, off_exfac = 0, off_ids = 0, end = 0;
  uint64_t ex_row_bytes() const { return D * ex_bits / 8; }
};

constexpr uint64_t kFixedHeaderBytes = 4 * 8 + 1 + 2 * 4;

// Reads and checks the header of `f` (positioned at 0) against the file's size: every check of the reference's load_transposed
// (dim > 0, ex_bits < 9, 0 < n_lists <= max, n * D without overflow, sizes summing to n) and every section length against the
// bytes that are actually there - before the caller allocates anything.
inline file_header read_header(FILE* f, uint64_t file_bytes)
{
  file_header h;
  if (file_bytes < kFixedHeaderBytes) bad_file("file too short for the header (" + std::to_string(file_bytes) + " bytes)");
  unsigned char raw[kFixedHeaderBytes];
  if (fread(raw, 1, sizeof(raw), f) != sizeof(raw)) bad_file("unexpected end of file in the header");
  memcpy(&h.n, raw, 8);
  memcpy(&h.dim, raw + 8, 8);
  memcpy(&h.n_lists, raw + 16, 8);
  memcpy(&h.ex_bits, raw + 24, 8);
  float two[2];
  memcpy(two, raw + 33, 8);
  if (h.dim == 0) bad_file("dim=0");
  if (h.dim > kMaxDim) bad_file("dim=" + std::to_string(h.dim) + " exceeds the maximum " + std::to_string(kMaxDim));
  if (h.ex_bits >= 9) bad_file("ex_bits=" + std::to_string(h.ex_bits) + " out of the valid range [0, 9)");
  if (h.n_lists == 0 || h.n_lists > kMaxLists) bad_file("n_lists=" + std::to_string(h.n_lists) + " out of the valid range (0, 2^24]");
  if (h.n >= (uint64_t(1) << 32)) bad_file("n=" + std::to_string(h.n) + " does not fit 32-bit row ids");
  h.D = padded_dim(h.dim);
  h.t = two[0];
  h.metric = two[1] == 1.0f ? 1 : 0;  // anything else (a file of the reference keeps a query scaling constant here): L2Expanded
  // with n < 2^32, D <= 4096 and n_lists <= 2^24 no product below can overflow 64 bits
  uint64_t pos = kFixedHeaderBytes;
  auto section = [&](uint64_t bytes, const char* name) {
    if (bytes > file_bytes - pos) bad_file(std::string("file too short for ") + name + " (" + std::to_string(bytes) + " bytes at offset " +
                                           std::to_string(pos) + ", file has " + std::to_string(file_bytes) + ")");
    const uint64_t at = pos;
    pos += bytes;
    return at;
  };
  const uint64_t off_sizes = section(h.n_lists * 8, "the list sizes");
  (void)off_sizes;
  h.sizes.resize((size_t)h.n_lists);
  if (fread(h.sizes.data(), 8, (size_t)h.n_lists, f) != (size_t)h.n_lists) bad_file("unexpected end of file in the list sizes");
  uint64_t total = 0;
  for (uint64_t s : h.sizes) {
    if (s > h.n) bad_file("a list size exceeds n");
    total += s;  // (n_lists * n < 2^56)
  }
  if (total != h.n) bad_file("list sizes (" + std::to_string(total) + ") do not sum to n (" + std::to_string(h.n) + ")");
  h.off_rotation = section(h.D * h.D * 4, "the rotation matrix");
  h.off_centers  = section(h.n_lists * h.D * 4, "the centroids");
  h.off_bits     = section(h.n * (h.D / 32) * 4, "the bit codes");
  h.off_short    = section(h.n * 12, "the short factors");
  h.off_ex       = section(h.n * h.ex_row_bytes(), "the extended codes");
  h.off_exfac    = section(h.n * 8, "the extended factors");
  h.off_ids      = section(h.n * 4, "the ids");
  h.end          = pos;
  if (h.end != file_bytes) bad_file("trailing bytes after the ids (" + std::to_string(file_bytes - h.end) + ")");
  return h;
}

// ids must name rows of the index (the search hands them out as they are)
inline void check_ids(const uint32_t* ids, uint64_t n)
{
  for (uint64_t i = 0; i < n; ++i)
    if (ids[i] == 0xffffffffu) bad_file("row id 0xffffffff is reserved");
}

// bit words: the file keeps dimension 32 w + i at bit 31 - i, the kernels at bit i
inline uint32_t reverse_bits(uint32_t v)
{
  v = ((v >> 1) & 0x55555555u) | ((v & 0x55555555u) << 1);
  v = ((v >> 2) & 0x33333333u) | ((v & 0x33333333u) << 2);
  v = ((v >> 4) & 0x0f0f0f0fu) | ((v & 0x0f0f0f0fu) << 4);
  v = ((v >> 8) & 0x00ff00ffu) | ((v & 0x00ff00ffu) << 8);
  return (v >> 16) | (v << 16);
}

// ------------------------------------------------------------------ the constant scaling factor t
// t(D, ex) = mean over 100 pseudo-random unit vectors of the rescale factor that maximises the cosine between |o| and its
// quantized image (the reference's get_const_scaling_factors / best_rescale_factor). The vectors come from this library's own
// generator - splitmix64, twelve 32-bit uniforms summed per component (Irwin-Hall: a normal shape from exact arithmetic, no libm) -
// and every sum below runs in index order, so that tests/ivf_rabitq_ref.py reproduces the value bit for bit.
inline uint64_t splitmix64(uint64_t i, uint64_t seed)
{
  uint64_t z = seed + (i + 1) * 0x9e3779b97f4a7c15ull;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

constexpr double kTightStart[9] = {0, 0.15, 0.20, 0.52, 0.59, 0.71, 0.75, 0.77, 0.81};

inline double best_rescale_factor(const double* o, size_t dim, unsigned ex_bits)
{
  const int top = (1 << ex_bits) - 1;
  double max_o  = 0;
  for (size_t i = 0; i < dim; ++i) max_o = std::max(max_o, o[i]);
  const double t_end   = (double)(top + 10) / max_o;
  const double t_start = t_end * kTightStart[ex_bits];
  double den = (double)dim * 0.25, num = 0;
  std::vector<std::pair<double, uint32_t>> events;  // (t at which component i steps up, i); the level follows from the order
  std::vector<int> level(dim);
  for (size_t i = 0; i < dim; ++i) {
    const int cur = (int)(t_start * o[i] + 1e-5);
    level[i]      = cur;
    den += (double)(cur * cur + cur);
    num += ((double)cur + 0.5) * o[i];
    // the first step of a component always counts; later ones while the level stays below the top and t below t_end
    for (int u = cur + 1;; ++u) {
      const double tu = (double)u / o[i];
      if (u != cur + 1 && !(u <= top && tu < t_end)) break;
      events.emplace_back(tu, (uint32_t)i);
    }
  }
  std::sort(events.begin(), events.end());
  double best = 0, t = 0;
  for (const auto& e : events) {
    const int u = ++level[e.second];
    den += 2.0 * u;
    num += o[e.second];
    const double ip = num / std::sqrt(den);
    if (ip > best) {
      best = ip;
      t    = e.first;
    }
  }
  return t;
}

inline float const_scaling_factor(uint32_t D, uint32_t ex_bits)
{
  if (ex_bits == 0) return 0.0f;
  constexpr int kRows = 100;
  const uint64_t seed = 0x7261626974710000ull + (uint64_t)D * 16 + ex_bits;
  std::vector<double> o(D);
  double sum = 0;
  for (int r = 0; r < kRows; ++r) {
    double nrm2 = 0;
    for (uint32_t j = 0; j < D; ++j) {
      uint64_t s = 0;
      for (int u = 0; u < 12; ++u) s += splitmix64(((uint64_t)r * D + j) * 12 + u, seed) >> 32;
      const double v = (double)s / 4294967296.0 - 6.0;
      o[j]           = std::fabs(v);
      nrm2 += v * v;
    }
    const double nrm = std::sqrt(nrm2);
    for (uint32_t j = 0; j < D; ++j) o[j] = o[j] / nrm;
    sum += best_rescale_factor(o.data(), D, ex_bits);
  }
  return (float)(sum / kRows);
}

}  // namespace rabitq_host
}  // namespace cuvs_amd
