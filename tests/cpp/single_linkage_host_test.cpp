// Stand-alone test of cuvs_amd/csrc/single_linkage_host.hpp (built with -fsanitize=address,undefined by
// tests/test_single_linkage_cpu.py): the union-find of the dendrogram, the label roots of a cut, build_k, the round bound and
// the argument checks, against hand-written cases.
#include "single_linkage_host.hpp"

#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

using namespace cuvs_amd::sl_host;

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

static tensor_desc mat(int64_t r, int64_t c, int code = 2, int bits = 32)
{
  tensor_desc t;
  t.present = true; t.ndim = 2; t.shape[0] = r; t.shape[1] = c; t.code = code; t.bits = bits;
  return t;
}
static tensor_desc vec(int64_t len, int code = 0, int bits = 64)
{
  tensor_desc t;
  t.present = true; t.ndim = 1; t.shape[0] = len; t.code = code; t.bits = bits;
  return t;
}

template <typename IdxT>
static void test_dendrogram()
{
  // a chain 0 - 1 - 2 - 3 - 4 merged from the far end: every merge joins the growing node with a leaf
  {
    const std::vector<IdxT> src = {3, 2, 1, 0}, dst = {4, 3, 2, 1};
    const std::vector<float> w = {1.f, 2.f, 3.f, 4.f};
    std::vector<IdxT> ch(8, -7), size(4, -7);
    std::vector<float> delta(4, -7.f);
    build_dendrogram<IdxT>(src.data(), dst.data(), w.data(), 4, ch.data(), delta.data(), size.data());
    CHECK((ch == std::vector<IdxT>{3, 4, 2, 5, 1, 6, 0, 7}));
    CHECK((size == std::vector<IdxT>{2, 3, 4, 5}));
    CHECK(delta == w);
    CHECK((label_roots<IdxT>(ch.data(), 5, 2) == std::vector<int64_t>{7, 0}));
    CHECK((label_roots<IdxT>(ch.data(), 5, 3) == std::vector<int64_t>{6, 1, 0}));
    CHECK((label_roots<IdxT>(ch.data(), 5, 5) == std::vector<int64_t>{4, 3, 2, 1, 0}));
  }
  // a star around 2, then two pairs joined last
  {
    const std::vector<IdxT> src = {2, 2, 2}, dst = {0, 1, 3};
    const std::vector<float> w = {1.f, 1.f, 5.f};
    std::vector<IdxT> ch(6), size(3);
    std::vector<float> delta(3);
    build_dendrogram<IdxT>(src.data(), dst.data(), w.data(), 3, ch.data(), delta.data(), size.data());
    CHECK((ch == std::vector<IdxT>{2, 0, 4, 1, 5, 3}));
    CHECK((size == std::vector<IdxT>{2, 3, 4}));
  }
  {
    const std::vector<IdxT> src = {0, 2, 1}, dst = {1, 3, 2};
    const std::vector<float> w = {1.f, 2.f, 9.f};
    std::vector<IdxT> ch(6), size(3);
    std::vector<float> delta(3);
    build_dendrogram<IdxT>(src.data(), dst.data(), w.data(), 3, ch.data(), delta.data(), size.data());
    CHECK((ch == std::vector<IdxT>{0, 1, 2, 3, 4, 5}));
    CHECK((size == std::vector<IdxT>{2, 2, 4}));
    CHECK((label_roots<IdxT>(ch.data(), 4, 2) == std::vector<int64_t>{5, 4}));
    CHECK((label_roots<IdxT>(ch.data(), 4, 3) == std::vector<int64_t>{4, 3, 2}));
  }
  // no spanning tree
  {
    const std::vector<IdxT> src = {0, 0}, dst = {1, 1};
    const std::vector<float> w = {1.f, 2.f};
    std::vector<IdxT> ch(4), size(2);
    std::vector<float> delta(2);
    CHECK(has(refusal([&] { build_dendrogram<IdxT>(src.data(), dst.data(), w.data(), 2, ch.data(), delta.data(), size.data()); }),
              "closes a cycle"));
    const std::vector<IdxT> far = {1, 7};
    CHECK(has(refusal([&] { build_dendrogram<IdxT>(src.data(), far.data(), w.data(), 2, ch.data(), delta.data(), size.data()); }),
              "outside"));
  }
  // a long chain in ascending order: find() walks and compresses n levels
  {
    const int64_t m = 5000;
    std::vector<IdxT> src((size_t)m), dst((size_t)m), ch((size_t)(2 * m)), size((size_t)m);
    std::vector<float> w((size_t)m, 1.f), delta((size_t)m);
    for (int64_t e = 0; e < m; ++e) { src[(size_t)e] = (IdxT)e; dst[(size_t)e] = (IdxT)(e + 1); }
    build_dendrogram<IdxT>(src.data(), dst.data(), w.data(), m, ch.data(), delta.data(), size.data());
    CHECK(size[(size_t)m - 1] == (IdxT)(m + 1));
    CHECK(ch[(size_t)(2 * m - 2)] == (IdxT)(2 * m - 1) && ch[(size_t)(2 * m - 1)] == (IdxT)m);
  }
}

static void test_k_and_rounds()
{
  CHECK(build_k(2, 15) == 2);
  CHECK(build_k(10, -1) == 2);
  CHECK(build_k(100, -4) == 2);
  CHECK(build_k(100, 5) == 11);
  CHECK(build_k(1000000, 15) == 34);
  CHECK(build_k(8, 100) == 8);
  CHECK(floor_log2(1) == 0 && floor_log2(2) == 1 && floor_log2(3) == 1 && floor_log2(1024) == 10 && floor_log2(1025) == 10);
  CHECK(max_dense_rounds(2) == 2 && max_dense_rounds(3) == 3 && max_dense_rounds(1024) == 11 && max_dense_rounds(1025) == 12);
}

static void test_checks()
{
  CHECK(!check_metric(0) && check_metric(1) && !check_metric(4) && check_metric(5));
  const std::string m = refusal([] { check_metric(2); });
  CHECK(has(m, "L2Expanded") && has(m, "L2SqrtExpanded") && has(m, "L2Unexpanded") && has(m, "L2SqrtUnexpanded"));
  CHECK(has(refusal([] { check_linkage(2); }), "PAIRWISE"));
  CHECK(has(refusal([] { check_space(2); }), "MUTUAL_REACHABILITY"));

  int64_t n = 0, dim = 0;
  check_x(mat(10, 3), &n, &dim);
  CHECK(n == 10 && dim == 3);
  CHECK(has(refusal([&] { check_x(tensor_desc{}, &n, &dim); }), "must not be NULL"));
  CHECK(has(refusal([&] { check_x(vec(10, 2, 32), &n, &dim); }), "2-D"));
  CHECK(has(refusal([&] { check_x(mat(10, 3, 2, 16), &n, &dim); }), "must be fp32"));
  CHECK(has(refusal([&] { check_x(mat(10, 3, 2, 64), &n, &dim); }), "must be fp32"));
  tensor_desc host = mat(10, 3);
  host.on_device   = false;
  CHECK(has(refusal([&] { check_x(host, &n, &dim); }), "device memory"));
  tensor_desc gaps = mat(10, 3);
  gaps.contiguous  = false;
  CHECK(has(refusal([&] { check_x(gaps, &n, &dim); }), "contiguous"));
  CHECK(has(refusal([&] { check_x(mat(1, 3), &n, &dim); }), "n >= 2"));
  CHECK(has(refusal([&] { check_x(mat(int64_t(1) << 30, 3), &n, &dim); }), "n < 2^30"));
  CHECK(has(refusal([&] { check_x(mat(10, 0), &n, &dim); }), "at least one column"));

  int bytes = 0;
  check_index(mat(9, 2, 0, 32), 9, 2, "dendrogram", true, &bytes);
  CHECK(bytes == 4);
  CHECK(has(refusal([&] { check_index(vec(10, 0, 64), 10, 0, "labels", true, &bytes); }), "one type"));
  check_index(vec(10, 0, 32), 10, 0, "labels", true, &bytes);
  CHECK(has(refusal([&] { check_index(vec(11, 0, 32), 10, 0, "labels", true, &bytes); }), "shape [10]"));
  CHECK(has(refusal([&] { check_index(mat(9, 3, 0, 32), 9, 2, "dendrogram", true, &bytes); }), "shape [9, 2]"));
  CHECK(has(refusal([&] { check_index(vec(10, 2, 32), 10, 0, "labels", true, &bytes); }), "int32 or int64"));
  CHECK(has(refusal([&] { check_index(tensor_desc{}, 10, 0, "labels", true, &bytes); }), "must not be NULL"));
  check_index(tensor_desc{}, 10, 0, "labels", false, &bytes);

  check_f32_vector(vec(10, 2, 32), 10, "core_dists", true);
  CHECK(has(refusal([] { check_f32_vector(tensor_desc{}, 10, "core_dists", true); }), "must not be NULL"));
  CHECK(has(refusal([] { check_f32_vector(vec(10, 2, 64), 10, "core_dists", true); }), "must be fp32"));
  CHECK(has(refusal([] { check_f32_vector(vec(9, 2, 32), 10, "core_dists", true); }), "shape [10]"));

  check_n_clusters(1, 10);
  check_n_clusters(10, 10);
  CHECK(has(refusal([] { check_n_clusters(0, 10); }), "n_clusters must be in [1, n]"));
  CHECK(has(refusal([] { check_n_clusters(11, 10); }), "n_clusters must be in [1, n]"));
  check_min_samples(2, 10);
  check_min_samples(10, 10);
  CHECK(has(refusal([] { check_min_samples(1, 10); }), "min_samples must be in [2, n]"));
  CHECK(has(refusal([] { check_min_samples(11, 10); }), "min_samples must be in [2, n]"));
}

int main()
{
  test_dendrogram<int32_t>();
  test_dendrogram<int64_t>();
  test_k_and_rounds();
  test_checks();
  if (g_failed == 0) std::printf("single linkage host OK\n");
  return g_failed == 0 ? 0 : 1;
}
