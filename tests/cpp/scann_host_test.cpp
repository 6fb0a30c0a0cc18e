// Host-only parts of the ScaNN build (cuvs_amd/csrc/scann_host.hpp) on their own, meant to be built with
// -fsanitize=address,undefined (tests/test_scann_cpu.py): the parameter checks, and the writer of the index files fed with raw
// arrays that the test wrote:
//   scann_host_test IN_DIR OUT_DIR n_rows dim n_leaves pq_dim pq_bits has_bf16
// IN_DIR holds centers.f32, labels.u32, soar.u32, codebook.f32, codes.u8 and soar_codes.u8 (packed rows) and bf16.i16.
#include "scann_host.hpp"

#include <cstdlib>
#include <cstring>

namespace H = cuvs_amd::scann_host;

template <typename T>
static std::vector<T> slurp(const std::string& name, size_t count)
{
  std::vector<T> v(count);
  FILE* f = fopen(name.c_str(), "rb");
  if (f == nullptr) H::refuse("cannot open %s", name.c_str());
  const size_t got = count ? fread(v.data(), sizeof(T), count, f) : 0;
  fclose(f);
  if (got != count) H::refuse("%s is too short", name.c_str());
  return v;
}

template <typename Fn>
static bool refused(Fn&& fn, const char* word)
{
  try {
    fn();
  } catch (const std::invalid_argument& e) {
    return strstr(e.what(), word) != nullptr;
  }
  return false;
}

static int check_params_cases()
{
  int bad = 0;
  H::params p;
  p.n_leaves = 32;
  H::check_params(p, 4096, 64);  // the defaults pass
  auto expect = [&](bool ok, const char* what) {
    if (!ok) { printf("FAILED: %s\n", what); ++bad; }
  };
  { H::params q = p; q.pq_bits = 5; expect(refused([&] { H::check_params(q, 4096, 64); }, "pq_bits"), "pq_bits 5"); }
  { H::params q = p; q.pq_dim = 7; expect(refused([&] { H::check_params(q, 4096, 64); }, "multiple of pq_dim"), "dim % pq_dim"); }
  { H::params q = p; q.partitioning_eta = 0.f; expect(refused([&] { H::check_params(q, 4096, 64); }, "partitioning_eta"), "eta 0"); }
  { H::params q = p; q.soar_lambda = -1.f; expect(refused([&] { H::check_params(q, 4096, 64); }, "soar_lambda"), "lambda < 0"); }
  { H::params q = p; q.n_leaves = 0; expect(refused([&] { H::check_params(q, 4096, 64); }, "n_leaves"), "n_leaves 0"); }
  { H::params q = p; q.n_leaves = 5000; expect(refused([&] { H::check_params(q, 4096, 64); }, "n_rows"), "n_rows < n_leaves"); }
  expect(H::pq_train_rows(p, 4096) == 4096 && H::pq_train_rows(p, 1 << 20) == 100000, "pq_train_rows");
  expect(H::sample_row(3, 10, 4) == 6, "sample_row");
  expect(H::avq_leaf_batch(1000, 128, size_t(2) << 30) == 1000 && H::avq_leaf_batch(1000, 520, 4 * 520 * 520 * 3) == 3 &&
           H::avq_leaf_batch(10, 520, 16) == 1,
         "avq_leaf_batch");
  expect(H::avq_solve_in_lds(130, 160 * 1024) && !H::avq_solve_in_lds(520, 160 * 1024), "avq_solve_in_lds");
  const uint8_t packed[4] = {0x21, 0x03, 0xba, 0x0c};  // two rows of three 4-bit codes: the odd nibble
  uint8_t out[6];
  H::unpack_codes(packed, 2, 3, 4, out);
  const uint8_t want[6] = {1, 2, 3, 10, 11, 12};
  expect(memcmp(out, want, 6) == 0, "unpack_codes");
  const uint32_t l[3] = {0, 4, 2}, s[3] = {1, 4, 0};
  const std::vector<int32_t> t = H::interleave_labels(l, s, 3);
  expect(t == std::vector<int32_t>({0, 1, 4, -1, 2, 0}), "interleave_labels");
  return bad;
}

int main(int argc, char** argv)
{
  try {
    int bad = check_params_cases();
    if (argc == 9) {
      const std::string in = std::string(argv[1]) + "/";
      const int64_t n = atoll(argv[3]), dim = atoll(argv[4]), n_leaves = atoll(argv[5]), pq_dim = atoll(argv[6]), bits = atoll(argv[7]);
      const bool has_bf16 = atoi(argv[8]) != 0;
      const int64_t n_sub = dim / pq_dim, book_n = int64_t(1) << bits, cb = (n_sub * bits + 7) / 8;
      const auto centers  = slurp<float>(in + "centers.f32", (size_t)(n_leaves * dim));
      const auto labels   = slurp<uint32_t>(in + "labels.u32", (size_t)n);
      const auto soar     = slurp<uint32_t>(in + "soar.u32", (size_t)n);
      const auto codebook = slurp<float>(in + "codebook.f32", (size_t)(book_n * dim));
      const auto packed   = slurp<uint8_t>(in + "codes.u8", (size_t)(n * cb));
      const auto packed_s = slurp<uint8_t>(in + "soar_codes.u8", (size_t)(n * cb));
      std::vector<int16_t> bf16;
      if (has_bf16) bf16 = slurp<int16_t>(in + "bf16.i16", (size_t)(n * dim));
      std::vector<uint8_t> codes((size_t)(n * n_sub)), codes_s((size_t)(n * n_sub));
      H::unpack_codes(packed.data(), n, n_sub, (int)bits, codes.data());
      H::unpack_codes(packed_s.data(), n, n_sub, (int)bits, codes_s.data());
      H::host_index h;
      h.n_rows = n; h.dim = dim; h.n_leaves = n_leaves; h.n_sub = n_sub; h.book_n = book_n; h.pq_dim = (uint32_t)pq_dim;
      h.centers = centers.data(); h.labels = labels.data(); h.soar = soar.data(); h.codebook = codebook.data();
      h.codes = codes.data(); h.soar_codes = codes_s.data(); h.bf16 = has_bf16 ? bf16.data() : nullptr;
      H::write_files(argv[2], h);
      if (!refused([&] { H::write_files(std::string(argv[2]) + "/missing/dir", h); }, "Cannot open")) { printf("FAILED: missing dir\n"); ++bad; }
    }
    if (bad) return 1;
    printf("scann host OK\n");
    return 0;
  } catch (const std::exception& e) {
    printf("exception: %s\n", e.what());
    return 2;
  }
}
