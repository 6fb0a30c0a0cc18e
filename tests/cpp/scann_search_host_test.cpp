// The host-only list builder of the ScaNN search (cuvs_amd/csrc/scann_host.hpp), built alone under the sanitizers:
//   scann_search_host_test <n_rows> <dim> <n_leaves> <pq_dim> <bits>
// Builds the lists of a small index made here, reads every entry back through the word layout the scan kernel uses and compares
// ids, codes and t with a direct restatement; then the refusals.
#include "scann_host.hpp"

#include <cstdlib>
#include <random>

namespace H = cuvs_amd::scann_host;

int main(int argc, char** argv)
{
  if (argc != 6) return 2;
  const int64_t n = atoll(argv[1]), dim = atoll(argv[2]), n_leaves = atoll(argv[3]), W = atoll(argv[4]), bits = atoll(argv[5]);
  const int64_t n_sub = dim / W, book_n = int64_t(1) << bits;
  std::mt19937 rng(7);
  std::uniform_real_distribution<float> u(-1.f, 1.f);
  std::vector<float> centers((size_t)(n_leaves * dim)), book((size_t)(book_n * dim));
  for (float& v : centers) v = u(rng);
  for (float& v : book) v = u(rng);
  std::vector<uint32_t> labels((size_t)n), soar((size_t)n);
  std::vector<uint8_t> codes((size_t)(n * n_sub)), soar_codes((size_t)(n * n_sub));
  for (int64_t i = 0; i < n; ++i) {
    labels[i] = rng() % (n_leaves - 1);  // the last leaf stays empty
    soar[i]   = i % 3 == 0 ? labels[i] : rng() % (n_leaves - 1);
  }
  for (uint8_t& c : codes) c = (uint8_t)(rng() % book_n);
  for (uint8_t& c : soar_codes) c = (uint8_t)(rng() % book_n);
  H::host_index h;
  h.n_rows = n; h.dim = dim; h.n_leaves = n_leaves; h.n_sub = n_sub; h.book_n = book_n; h.pq_dim = (uint32_t)W;
  h.centers = centers.data(); h.labels = labels.data(); h.soar = soar.data(); h.codebook = book.data();
  h.codes = codes.data(); h.soar_codes = soar_codes.data();
  const H::search_lists s = H::build_search_lists(h, true);

  int64_t total = 0, two = 0;
  for (int64_t i = 0; i < n; ++i) two += soar[i] != labels[i];
  if (s.n_spilled != two || s.leaf_size[n_leaves - 1] != 0 || s.dim_pad % 16 != 0 || s.dim_pad < dim) return 3;
  for (int64_t j = 0; j < n_leaves; ++j) {
    uint32_t prev = 0;
    for (uint32_t p = 0; p < s.leaf_size[j]; ++p, ++total) {
      const int64_t tile = s.tile_off[j] + p / 32, lane = p % 32;
      const uint32_t row = s.ids[tile * 32 + lane];
      if (row >= n || (p > 0 && row <= prev)) return 4;  // ascending row id
      prev = row;
      const bool primary    = labels[row] == (uint32_t)j;
      const uint8_t* expect = primary ? &codes[row * n_sub] : &soar_codes[row * n_sub];
      if (!primary && (soar[row] != (uint32_t)j)) return 5;
      double cr = 0, rr = 0;
      for (int64_t sub = 0; sub < n_sub; ++sub) {
        const uint32_t c = (s.words[(tile * s.n_words + sub / 4) * 32 + lane] >> (8 * (sub % 4))) & 255u;
        if (c != expect[sub]) return 6;
        for (int64_t d = sub * W; d < (sub + 1) * W; ++d) {
          cr += (double)centers[j * dim + d] * book[c * dim + d];
          rr += (double)book[c * dim + d] * book[c * dim + d];
        }
      }
      if (s.t[tile * 32 + lane] != (float)(2.0 * cr + rr)) return 7;
    }
    for (uint32_t p = s.leaf_size[j]; p < (s.tile_off[j + 1] - s.tile_off[j]) * 32; ++p)
      if (s.ids[(int64_t)s.tile_off[j] * 32 + p] != H::kNoRow) return 8;  // the padding of the last tile
  }
  if (total != n + two) return 9;
  for (int64_t e = 0; e < book_n; ++e)
    for (int64_t d = 0; d < s.dim_pad; ++d) {
      const uint16_t want = d < dim ? H::bf16_rne_bits(book[e * dim + d]) : 0;
      if (s.book_bf16[e * s.dim_pad + d] != want) return 10;
    }
  if (H::bf16_rne_bits(1.00390625f) != 0x3f80 || H::bf16_rne_bits(1.01171875f) != 0x3f82) return 11;  // ties to even

  int refused = 0;
  auto refuses = [&](auto&& fn) { try { fn(); } catch (const std::invalid_argument&) { ++refused; } };
  refuses([&] { labels[0] = (uint32_t)n_leaves; H::build_search_lists(h, true); });
  labels[0] = 0;
  refuses([&] { H::check_search(2, 20, 0, 10, false, dim, dim); });     // cosine
  refuses([&] { H::check_search(0, 20, 100, 10, false, dim, dim); });   // re-rank without bf16 rows
  refuses([&] { H::check_search(0, 20, 5, 10, true, dim, dim); });      // k > n_reorder
  refuses([&] { H::check_search(0, 20, 0, 10, false, dim, dim + 1); }); // dim mismatch
  refuses([&] { H::check_search(6, 20, 0, 4097, false, dim, dim); });   // k > 4096
  H::check_search(6, 20, 4096, 4096, true, dim, dim);
  if (refused != 6) return 12;
  printf("scann search host OK\n");
  return 0;
}
