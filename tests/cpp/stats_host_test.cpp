// Stand-alone test of cuvs_amd/csrc/stats_host.hpp (built with -fsanitize=address,undefined by tests/test_stats_cpu.py): the
// argument checks and every refusal, the column segments of label-sorted rows, the slab size against a workspace limit and the
// score formulas, against hand-written cases.
#include "stats_host.hpp"

#include <cstdio>
#include <cstring>
#include <functional>
#include <vector>

using namespace cuvs_amd::stats_host;

static int g_failed = 0;
#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);   \
      ++g_failed;                                                  \
    }                                                              \
  } while (0)

// the message of the refusal `fn` must raise ("" when it raises none)
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

static tensor_desc mat(int64_t r, int64_t c, int code = 2, int bits = 32)
{
  tensor_desc t;
  t.present = true; t.ndim = 2; t.shape[0] = r; t.shape[1] = c; t.code = code; t.bits = bits;
  return t;
}
static tensor_desc vec(int64_t len, int code = 0, int bits = 32)
{
  tensor_desc t;
  t.present = true; t.ndim = 1; t.shape[0] = len; t.code = code; t.bits = bits;
  return t;
}

static void test_metrics()
{
  for (int m : {0, 4}) CHECK(check_silhouette_metric(m).chain == chain_t::sq && check_silhouette_metric(m).post == post_t::none);
  for (int m : {1, 5}) CHECK(check_silhouette_metric(m).chain == chain_t::sq && check_silhouette_metric(m).post == post_t::sqrt);
  CHECK(check_silhouette_metric(3).chain == chain_t::l1 && check_silhouette_metric(3).post == post_t::none);
  CHECK(check_silhouette_metric(2).chain == chain_t::dot && check_silhouette_metric(2).post == post_t::cosine);
  for (int m : {6, 7, 8, 20, -1}) CHECK(has(refusal([=] { check_silhouette_metric(m); }), "is not supported by the silhouette score"));
  for (int m : {0, 1, 4, 5}) CHECK(refusal([=] { check_trustworthiness_metric(m); }).empty());
  for (int m : {2, 3, 6, 20}) CHECK(has(refusal([=] { check_trustworthiness_metric(m); }), "is not supported by the trustworthiness score"));
}

static void test_argument_checks()
{
  int64_t n = -1, dim = -1;
  check_matrix(mat(5, 3), "X", &n, &dim);
  CHECK(n == 5 && dim == 3);
  auto m = [&](const tensor_desc& t) { return refusal([&] { check_matrix(t, "X", &n, &dim); }); };
  CHECK(has(m(tensor_desc{}), "X must not be NULL"));
  CHECK(has(m(vec(5, 2, 32)), "X must be a 2-D matrix"));
  CHECK(has(m(mat(5, 3, 2, 64)), "X must be fp32"));
  CHECK(has(m(mat(5, 3, 2, 16)), "X must be fp32"));
  CHECK(has(m(mat(5, 3, 0, 32)), "X must be fp32"));
  tensor_desc t = mat(5, 3);
  t.contiguous  = false;
  CHECK(has(m(t), "X must be row-major and contiguous"));
  t = mat(5, 3);
  t.on_device = false;
  CHECK(has(m(t), "X must be accessible on device memory"));
  CHECK(has(m(mat(int64_t(1) << 31, 1)), "n must be below 2^31"));
  CHECK(m(mat((int64_t(1) << 31) - 1, 1)).empty());

  CHECK(refusal([] { check_vector(vec(5), "labels", 5, false, false); }).empty());
  CHECK(refusal([] { check_vector(tensor_desc{}, "scores", 5, true, true); }).empty());
  CHECK(has(refusal([] { check_vector(tensor_desc{}, "labels", 5, false, false); }), "labels must not be NULL"));
  CHECK(has(refusal([] { check_vector(vec(5, 0, 64), "labels", 5, false, false); }), "labels must be int32"));
  CHECK(has(refusal([] { check_vector(vec(4), "labels", 5, false, false); }), "labels must have shape [5]"));
  CHECK(has(refusal([] { check_vector(mat(5, 1, 0, 32), "labels", 5, false, false); }), "labels must have shape [5]"));
  CHECK(has(refusal([] { check_vector(vec(5, 2, 64), "scores", 5, true, true); }), "scores must be fp32"));
  CHECK(has(refusal([] { check_vector(vec(6, 2, 32), "scores", 5, true, true); }), "scores must have shape [5]"));
  t = vec(5, 2, 32);
  t.on_device = false;
  CHECK(has(refusal([&] { check_vector(t, "scores", 5, true, true); }), "scores must be accessible on device memory"));

  CHECK(refusal([] { check_n_labels(2, 3); }).empty());
  CHECK(refusal([] { check_n_labels(299, 300); }).empty());
  CHECK(has(refusal([] { check_n_labels(1, 300); }), "n_labels must be in [2, n - 1]: n_labels is 1, n is 300"));
  CHECK(has(refusal([] { check_n_labels(300, 300); }), "n_labels must be in [2, n - 1]"));
  CHECK(has(refusal([] { check_n_labels(2, 2); }), "n_labels must be in [2, n - 1]"));
  CHECK(refusal([] { check_label_counts(0, 5); }).empty());
  CHECK(has(refusal([] { check_label_counts(3, 5); }), "labels holds 3 values outside [0, 5)"));

  CHECK(check_neighbors(mat(9, 1, 0, 64), 9) == 1 && check_neighbors(mat(9, 64, 0, 64), 9) == 64);
  CHECK(has(refusal([] { check_neighbors(mat(9, 65, 0, 64), 9); }), "k = 65 columns: k must be in [1, 64]"));
  CHECK(has(refusal([] { check_neighbors(mat(9, 0, 0, 64), 9); }), "k must be in [1, 64]"));
  CHECK(has(refusal([] { check_neighbors(mat(9, 5, 0, 32), 9); }), "neighbors must be int64"));
  CHECK(has(refusal([] { check_neighbors(mat(8, 5, 0, 64), 9); }), "neighbors must have shape [9, k]"));
  CHECK(has(refusal([] { check_neighbors(tensor_desc{}, 9); }), "neighbors must not be NULL"));
  CHECK(refusal([] { check_ranks(tensor_desc{}, 9, 5); }).empty());
  CHECK(refusal([] { check_ranks(mat(9, 5, 0, 32), 9, 5); }).empty());
  CHECK(has(refusal([] { check_ranks(mat(9, 5, 0, 64), 9, 5); }), "ranks must be int32"));
  CHECK(has(refusal([] { check_ranks(mat(9, 4, 0, 32), 9, 5); }), "ranks must have shape [9, 5]"));
  CHECK(refusal([] { check_neighbor_flags(0, 9); }).empty());
  CHECK(has(refusal([] { check_neighbor_flags(1, 9); }), "a row's own id"));
  CHECK(has(refusal([] { check_neighbor_flags(2, 9); }), "an id outside [0, 9)"));
  CHECK(has(refusal([] { check_neighbor_flags(3, 9); }), "outside"));

  CHECK(refusal([] { check_n_neighbors(5, 11); }).empty());
  CHECK(has(refusal([] { check_n_neighbors(5, 10); }), "n_neighbors = 5 must be less than n / 2 (n is 10)"));
  CHECK(has(refusal([] { check_n_neighbors(0, 10); }), "positive"));
  CHECK(has(refusal([] { check_n_neighbors(65, 1000); }), "at most 64"));
  CHECK(refusal([] { check_n_neighbors(64, 129); }).empty());
}

static void test_segments()
{
  // 300 rows: label 0 ends exactly on a tile edge, label 1 is a singleton, label 2 is empty, 3 and 4 straddle
  const std::vector<int32_t> counts = {128, 1, 0, 100, 71};
  const segments s = build_segments(counts.data(), 5, 300);
  CHECK((s.lo == std::vector<int32_t>{0, 128, 129, 229, 256}));
  CHECK((s.hi == std::vector<int32_t>{128, 129, 229, 256, 300}));
  CHECK((s.label == std::vector<int32_t>{0, 1, 3, 4, 4}));
  CHECK((s.tile_first == std::vector<int32_t>{0, 1, 4, 5}));
  CHECK((s.label_first == std::vector<int32_t>{0, 128, 129, 129, 229}));
  CHECK(s.straddling == 1 && s.count() == 5);
  // every row its own label but one pair: n - 1 labels
  std::vector<int32_t> ones(299, 1);
  ones[7] = 2;
  const segments u = build_segments(ones.data(), 299, 300);
  CHECK(u.count() == 299 && u.straddling == 3 && u.tile_first.back() == 299 && u.lo[8] == 9 && u.hi[7] == 9);
  // one label over many tiles
  const std::vector<int32_t> two = {1000, 24};
  const segments w = build_segments(two.data(), 2, 1024);
  CHECK(w.count() == 9 && w.straddling == 1 && w.lo[7] == 896 && w.hi[7] == 1000 && w.label[8] == 1);
  CHECK(has(refusal([&] { build_segments(two.data(), 2, 1000); }), "add up to more than n"));
  CHECK(has(refusal([&] { build_segments(two.data(), 2, 1100); }), "add up to 1024, n is 1100"));
}

static void test_slabs()
{
  CHECK(silhouette_row_bytes(9) == 72 && ranks_row_bytes(64) == 832);
  CHECK(slab_rows(0, 72, 1 << 20, 0, 0) == 0);
  CHECK(slab_rows(257, 72, int64_t(1) << 30, 0, 0) == 257);    // everything fits
  CHECK(slab_rows(257, 72, int64_t(1) << 30, 100, 0) == 100);  // the caller's batch
  CHECK(slab_rows(257, 72, int64_t(1) << 30, 1, 0) == 1);
  CHECK(slab_rows(257, 72, int64_t(1) << 30, 0, 64) == 64);    // the test hook
  CHECK(slab_rows(257, 72, int64_t(1) << 30, 100, 64) == 64);
  CHECK(slab_rows(100000, 8000, 1, 0, 0) == 128);              // never below one tile
  const int64_t segs = 782 + 999, limit = int64_t(2) << 30;    // n = 100k, 1000 labels
  const int64_t rows = slab_rows(1000000, silhouette_row_bytes(segs), limit, 0, 0);
  CHECK(rows % 128 == 0 && rows * silhouette_row_bytes(segs) <= limit && (rows + 128) * silhouette_row_bytes(segs) > limit);
}

static void test_formulas()
{
  const double inf = std::numeric_limits<double>::infinity();
  CHECK(sil_sample(10.0, 1.0, 3.0) == 0.0);                 // a singleton
  CHECK(sil_sample(6.0, 3.0, 3.0) == 0.0);                  // a == b
  CHECK(sil_sample(6.0, 3.0, inf) == 0.0);                  // no other label has a row
  CHECK(sil_sample(6.0, 3.0, 4.0) == 0.25);                 // a = 3, b = 4
  CHECK(sil_sample(8.0, 3.0, 1.0) == -0.75);                // a = 4, b = 1
  CHECK(sil_sample(0.0, 3.0, 5.0) == 1.0);
  const std::vector<double> s = {0.25, -0.75, 1.0, 0.0};
  CHECK(sil_mean(s.data(), 4) == 0.125);
  // sklearn's example values: n = 50, k = 5, t = 1362 gives the reference test's window
  CHECK(trustworthiness(50, 5, 0) == 1.0);
  const double tw = trustworthiness(50, 5, 1362);
  CHECK(tw == 1.0 - ((2.0 / (250.0 * 84.0)) * 1362.0));
  // n * k past 2^31 (an int product would overflow): n = 2^26, k = 64
  const int64_t n = int64_t(1) << 26;
  const double big = trustworthiness(n, 64, uint64_t(1) << 40);
  const double want = 1.0 - ((2.0 / ((67108864.0 * 64.0) * ((2.0 * 67108864.0) - 192.0 - 1.0))) * 1099511627776.0);
  CHECK(big == want && big > 0.0 && big < 1.0);
}

int main()
{
  test_metrics();
  test_argument_checks();
  test_segments();
  test_slabs();
  test_formulas();
  if (g_failed != 0) return 1;
  std::printf("stats host OK\n");
  return 0;
}
