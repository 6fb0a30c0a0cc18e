// Stand-alone check of the host-only parts of IVF-RaBitQ (cuvs_amd/csrc/ivf_rabitq_host.hpp) for a sanitizer build:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -Icuvs_amd/csrc \
//       scripts/ivf_rabitq_file_check.cpp -o ivf_rabitq_file_check && ./ivf_rabitq_file_check
// It writes a small valid file, reads its header back, then feeds read_header every truncation of the file and thousands of
// corrupted copies (random bytes of the header and of the list sizes overwritten, extreme values in every header field): each must
// either be accepted with section offsets inside the file or be refused with an exception - never read or allocate out of bounds.
// After the header it reads every section the way the loader does. Also runs the scaling factor and the bit reversal.
#include "ivf_rabitq_host.hpp"

#include <cstdlib>
#include <random>

using namespace cuvs_amd::rabitq_host;

static std::vector<unsigned char> make_file(uint64_t dim, uint64_t ex, const std::vector<uint64_t>& sizes)
{
  uint64_t n = 0;
  for (auto s : sizes) n += s;
  const uint64_t D = padded_dim(dim);
  std::vector<unsigned char> f;
  auto put = [&](const void* p, size_t b) { f.insert(f.end(), (const unsigned char*)p, (const unsigned char*)p + b); };
  const uint64_t head[4] = {n, dim, sizes.size(), ex};
  put(head, 32);
  const unsigned char flag = 1;
  put(&flag, 1);
  const float two[2] = {3.25f, 1.0f};
  put(two, 8);
  put(sizes.data(), sizes.size() * 8);
  f.resize(f.size() + D * D * 4 + sizes.size() * D * 4 + n * (D / 32) * 4 + n * 12 + n * D * ex / 8 + n * 8, 0x5a);
  for (uint64_t i = 0; i < n; ++i) {
    const uint32_t id = (uint32_t)i;
    put(&id, 4);
  }
  return f;
}

// what the loader does with a file: header, then every section into a buffer of the header's size
static bool try_load(const std::vector<unsigned char>& bytes, const char* path)
{
  FILE* f = fopen(path, "wb");
  if (!f) abort();
  if (!bytes.empty() && fwrite(bytes.data(), 1, bytes.size(), f) != bytes.size()) abort();
  fclose(f);
  f = fopen(path, "rb");
  if (!f) abort();
  bool ok = false;
  try {
    const file_header h = read_header(f, bytes.size());
    if (h.end != bytes.size() || h.off_ids + h.n * 4 != h.end || h.off_rotation != kFixedHeaderBytes + h.n_lists * 8) abort();
    std::vector<float> rotation((size_t)(h.D * h.D)), centers((size_t)(h.n_lists * h.D)), sf((size_t)h.n * 3), ef((size_t)h.n * 2);
    std::vector<uint32_t> bits((size_t)(h.n * (h.D / 32))), ids((size_t)h.n);
    std::vector<uint8_t> exc((size_t)(h.n * h.ex_row_bytes()));
    auto get = [&](void* p, size_t b) { if (b && fread(p, 1, b, f) != b) abort(); };  // the header promised these bytes
    get(rotation.data(), rotation.size() * 4); get(centers.data(), centers.size() * 4); get(bits.data(), bits.size() * 4);
    get(sf.data(), sf.size() * 4); get(exc.data(), exc.size()); get(ef.data(), ef.size() * 4); get(ids.data(), ids.size() * 4);
    check_ids(ids.data(), h.n);
    ok = true;
  } catch (const std::exception& e) {
    if (std::string(e.what()).find("ivf_rabitq::deserialize") != 0) abort();  // every refusal carries a message
  }
  fclose(f);
  return ok;
}

int main()
{
  const char* path = "ivf_rabitq_file_check.tmp";
  const std::vector<unsigned char> good = make_file(10, 2, {3, 0, 40, 7});
  if (!try_load(good, path)) { fprintf(stderr, "the valid file was refused\n"); return 1; }
  if (!try_load(make_file(64, 0, {1}), path) || !try_load(make_file(65, 8, {2, 2}), path)) return 1;
  size_t refused = 0, accepted = 0;
  for (size_t cut = 0; cut < good.size(); cut += (cut < 200 ? 1 : 97)) {  // every truncation of the header, a sweep beyond
    std::vector<unsigned char> t(good.begin(), good.begin() + cut);
    if (try_load(t, path)) { fprintf(stderr, "a truncated file (%zu bytes) was accepted\n", cut); return 1; }
    ++refused;
  }
  std::mt19937_64 rng(5);
  const uint64_t extremes[] = {0, 1, 8, 9, 63, 64, 65, 4096, 4097, 1ull << 24, (1ull << 24) + 1, 1ull << 31, 1ull << 32, (1ull << 32) - 1,
                               1ull << 40, 1ull << 62, ~0ull, ~0ull - 63};
  for (int field = 0; field < 4; ++field)
    for (uint64_t v : extremes) {
      std::vector<unsigned char> t = good;
      memcpy(t.data() + 8 * field, &v, 8);
      (try_load(t, path) ? accepted : refused)++;
    }
  for (int it = 0; it < 4000; ++it) {
    std::vector<unsigned char> t = good;
    const int nb = 1 + (int)(rng() % 4);
    for (int b = 0; b < nb; ++b) t[rng() % (kFixedHeaderBytes + 4 * 8)] = (unsigned char)rng();
    if (it % 5 == 0) t.resize(rng() % (good.size() + 64), 0);
    (try_load(t, path) ? accepted : refused)++;
  }
  {  // ids: the reserved value is refused
    std::vector<unsigned char> t = good;
    memset(t.data() + t.size() - 4, 0xff, 4);
    if (try_load(t, path)) return 1;
  }
  remove(path);
  if (reverse_bits(1u) != 0x80000000u || reverse_bits(0x80000001u) != 0x80000001u || reverse_bits(0x0000f00fu) != 0xf00f0000u) return 1;
  const float t1 = const_scaling_factor(64, 1), t8 = const_scaling_factor(128, 8), t0 = const_scaling_factor(64, 0);
  if (!(t1 > 0 && t8 > t1 && t0 == 0.0f)) return 1;
  printf("ivf_rabitq_file_check: %zu files refused, %zu accepted, t(64,1)=%.6f t(128,8)=%.4f: OK\n", refused, accepted, t1, t8);
  return 0;
}
