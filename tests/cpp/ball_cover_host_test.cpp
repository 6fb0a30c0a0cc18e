// Stand-alone test of cuvs_amd/csrc/ball_cover_host.hpp (built with -fsanitize=address,undefined by
// tests/test_ball_cover_cpu.py): the landmark draw, the order of the lists, the slabs of the CSR fill and the argument
// checks, against hand-written cases. With an argument it prints the landmarks of (m, n, seed) for the twin to compare.
#include "ball_cover_host.hpp"

#include <cstdio>
#include <cstdlib>
#include <functional>
#include <set>
#include <vector>

using namespace cuvs_amd::bc_host;

static int g_failed = 0;
#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);   \
      ++g_failed;                                                  \
    }                                                              \
  } while (0)

static std::string refusal(const std::function<void()>& fn)
{
  try {
    fn();
  } catch (const std::invalid_argument& e) {
    return e.what();
  }
  return "";
}
static bool has(const std::string& s, const char* part) { return s.find(part) != std::string::npos; }

static void test_landmarks()
{
  CHECK(isqrt(1) == 1 && isqrt(3) == 1 && isqrt(4) == 2 && isqrt(65535) == 255 && isqrt(65536) == 256 && isqrt(999999) == 999);
  CHECK(isqrt((int64_t(1) << 32) - 1) == 65535);
  CHECK(landmarks_of(1, 0) == 1 && landmarks_of(3000, 0) == 54 && landmarks_of(3000, 7) == 7);
  for (int64_t m : {1, 2, 3, 63, 64, 65, 1000}) {
    for (int64_t n : {int64_t(1), landmarks_of(m, 0), m}) {
      const std::vector<int64_t> a = draw_landmarks(m, n, 5), b = draw_landmarks(m, n, 5), c = draw_landmarks(m, n, 6);
      CHECK((int64_t)a.size() == n && a == b);
      CHECK(std::set<int64_t>(a.begin(), a.end()).size() == (size_t)n);  // without replacement
      for (int64_t r : a) CHECK(r >= 0 && r < m);
      if (m == 1000 && n > 1 && n < m) CHECK(a != c);
      // a prefix of the draw of more landmarks
      const std::vector<int64_t> all = draw_landmarks(m, m, 5);
      CHECK(std::equal(a.begin(), a.end(), all.begin()));
    }
  }
}

static void test_order()
{
  // rows 0..7, three lists; list 1 is empty; ties inside list 0 go by row id
  const std::vector<uint32_t> label = {2, 0, 0, 2, 0, 0, 2, 0};
  const std::vector<float> dist     = {1.5f, 2.f, 0.f, 0.5f, 2.f, 1.f, 0.5f, 0.f};
  std::vector<int64_t> indptr(4, -1), cols(8, -1);
  std::vector<float> sd(8, -1.f), radius(3, -1.f);
  order_lists(label.data(), dist.data(), 8, 3, indptr.data(), cols.data(), sd.data(), radius.data());
  CHECK((indptr == std::vector<int64_t>{0, 5, 5, 8}));
  CHECK((cols == std::vector<int64_t>{2, 7, 5, 1, 4, 3, 6, 0}));
  CHECK((sd == std::vector<float>{0.f, 0.f, 1.f, 2.f, 2.f, 0.5f, 0.5f, 1.5f}));
  CHECK((radius == std::vector<float>{2.f, 0.f, 1.5f}));
}

static void test_slabs()
{
  const std::vector<int64_t> deg = {3, 0, 10, 2, 2};
  CHECK(slab_end(deg.data(), 5, 0, 16 * 100) == 5);
  CHECK(slab_end(deg.data(), 5, 0, 16 * 12) == 2);   // 3 + 0, then 10 does not fit
  CHECK(slab_end(deg.data(), 5, 2, 16 * 12) == 4);   // 10 + 2
  CHECK(slab_end(deg.data(), 5, 2, 16) == 3);        // a row larger than the budget goes alone
  CHECK(slab_end(deg.data(), 5, 4, 16 * 12) == 5);
}

static void test_checks()
{
  CHECK(refusal([] { check_build(kL2Sqrt, 1, 1, 0); }).empty());
  CHECK(refusal([] { check_build(kL2SqrtUnexpanded, 10, 32, 10); }).empty());
  CHECK(refusal([] { check_build(kHaversine, 10, 2, 3); }).empty());
  for (int metric : {0, 4}) CHECK(has(refusal([=] { check_build(metric, 10, 2, 0); }), "squared L2 forms are not metrics"));
  CHECK(has(refusal([] { check_build(kHaversine, 10, 3, 0); }), "Haversine needs dim == 2"));
  CHECK(has(refusal([] { check_build(kL2Sqrt, 10, 33, 0); }), "dim must be in [1, 32]"));
  CHECK(has(refusal([] { check_build(kL2Sqrt, 0, 2, 0); }), "at least one row"));
  CHECK(has(refusal([] { check_build(kL2Sqrt, int64_t(1) << 32, 2, 0); }), "below 2^32"));
  CHECK(has(refusal([] { check_build(kL2Sqrt, 10, 2, 11); }), "n_landmarks (11) must not exceed"));

  CHECK(refusal([] { check_knn(kL2Sqrt, 3, 3, 256, 256, 1.f); }).empty());
  CHECK(refusal([] { check_knn(kHaversine, 2, 2, 1, 1, 0.5f); }).empty());
  CHECK(has(refusal([] { check_knn(kL2Sqrt, 4, 4, 1, 10, 1.f); }), "k-NN needs dim 2 or 3"));
  CHECK(has(refusal([] { check_knn(kL2Sqrt, 2, 3, 1, 10, 1.f); }), "queries have 3 columns, the index has 2"));
  CHECK(has(refusal([] { check_knn(kL2Sqrt, 2, 2, 257, 1000, 1.f); }), "k must be in [1, 256]"));
  CHECK(has(refusal([] { check_knn(kL2Sqrt, 2, 2, 0, 1000, 1.f); }), "k must be in [1, 256]"));
  CHECK(has(refusal([] { check_knn(kL2Sqrt, 2, 2, 11, 10, 1.f); }), "k (11) must not exceed n_landmarks (10)"));
  CHECK(has(refusal([] { check_knn(kL2Sqrt, 2, 2, 1, 10, -1.f); }), "weight"));
  CHECK(has(refusal([] { check_knn(kL2Sqrt, 2, 2, 1, 10, std::nanf("")); }), "weight"));

  CHECK(refusal([] { check_eps(kL2Sqrt, 32, 32, 0.f); }).empty());
  CHECK(has(refusal([] { check_eps(kHaversine, 2, 2, 1.f); }), "eps_nn needs an L2 index"));
  CHECK(has(refusal([] { check_eps(kL2Sqrt, 2, 2, -1.f); }), "eps"));
  CHECK(has(refusal([] { check_eps(kL2Sqrt, 2, 3, 1.f); }), "columns"));
  CHECK(margin_of(kL2Sqrt) == 0x1p-17f && margin_of(kHaversine) == 0x1p-8f && slack_of(kL2Sqrt) == 0.f && slack_of(kHaversine) == 0x1p-16f);
}

int main(int argc, char** argv)
{
  if (argc == 4) {
    for (int64_t r : draw_landmarks(std::atoll(argv[1]), std::atoll(argv[2]), (uint32_t)std::atoll(argv[3]))) std::printf("%lld\n", (long long)r);
    return 0;
  }
  test_landmarks();
  test_order();
  test_slabs();
  test_checks();
  if (g_failed != 0) return 1;
  std::printf("ball cover host OK\n");
  return 0;
}
