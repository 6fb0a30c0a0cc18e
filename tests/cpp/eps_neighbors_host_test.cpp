// Stand-alone test of cuvs_amd/csrc/eps_neighbors_host.hpp (built with -fsanitize=address,undefined by
// tests/test_eps_neighbors_cpu.py): CSR offsets from degrees, the max_k truncation, the slab size and the argument checks,
// against hand-written cases.
#include "eps_neighbors_host.hpp"

#include <cstdio>
#include <cstring>
#include <functional>
#include <vector>

using namespace cuvs_amd::eps_host;

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
static tensor_desc vec(int64_t len, int code = 0, int bits = 64)
{
  tensor_desc t;
  t.present = true; t.ndim = 1; t.shape[0] = len; t.code = code; t.bits = bits;
  return t;
}

static void test_offsets()
{
  const std::vector<int64_t> deg = {3, 0, 0, 5, 1, 0};  // empty rows at the front of a run, in the middle and at the end
  std::vector<int64_t> off(deg.size() + 1, -7);
  // no cap
  CHECK(offsets_from_counts(deg.data(), 6, -1, 0, off.data()) == 9);
  CHECK((off == std::vector<int64_t>{0, 3, 3, 3, 8, 9, 9}));
  // max_k 0: every list is empty
  CHECK(offsets_from_counts(deg.data(), 6, 0, 0, off.data()) == 0);
  CHECK((off == std::vector<int64_t>{0, 0, 0, 0, 0, 0, 0}));
  // max_k 1
  CHECK(offsets_from_counts(deg.data(), 6, 1, 0, off.data()) == 3);
  CHECK((off == std::vector<int64_t>{0, 1, 1, 1, 2, 3, 3}));
  // max_k 3 cuts only the row of 5
  CHECK(offsets_from_counts(deg.data(), 6, 3, 0, off.data()) == 7);
  CHECK((off == std::vector<int64_t>{0, 3, 3, 3, 6, 7, 7}));
  // max_k above every degree == no cap
  CHECK(offsets_from_counts(deg.data(), 6, 6, 0, off.data()) == 9);
  CHECK((off == std::vector<int64_t>{0, 3, 3, 3, 8, 9, 9}));
  // two slabs with a carry give the offsets of one
  std::vector<int64_t> a(4), b(4);
  const int64_t carry = offsets_from_counts(deg.data(), 3, 3, 0, a.data());
  CHECK(carry == 3);
  CHECK(offsets_from_counts(deg.data() + 3, 3, 3, carry, b.data()) == 7);
  CHECK((a == std::vector<int64_t>{0, 3, 3, 3}) && (b == std::vector<int64_t>{3, 6, 7, 7}));
  // no rows: only offsets[0]
  int64_t one = -1;
  CHECK(offsets_from_counts(nullptr, 0, -1, 0, &one) == 0 && one == 0);
  CHECK(largest_degree(deg.data(), 6) == 5 && largest_degree(nullptr, 0) == 0);
  CHECK(kept(5, -1) == 5 && kept(5, 0) == 0 && kept(5, 5) == 5 && kept(5, 9) == 5 && kept(0, 3) == 0);
}

static void test_fill_checks()
{
  const std::vector<int64_t> indptr = {0, 3, 3, 3, 8, 9, 9};
  CHECK(refusal([&] { check_fill(indptr.data(), 6, 9, 0, false); }).empty());   // exactly nnz
  CHECK(refusal([&] { check_fill(indptr.data(), 6, 12, 9, true); }).empty());
  CHECK(has(refusal([&] { check_fill(indptr.data(), 6, 8, 0, false); }), "indices holds 8 entries but indptr[m] is 9"));  // one short
  CHECK(has(refusal([&] { check_fill(indptr.data(), 6, 9, 8, true); }), "distances holds 8 entries"));
  const std::vector<int64_t> down = {0, 3, 2}, neg = {-1, 0};
  CHECK(has(refusal([&] { check_fill(down.data(), 2, 100, 0, false); }), "not ascending at row 1"));
  CHECK(has(refusal([&] { check_fill(neg.data(), 1, 100, 0, false); }), "negative"));
  const int64_t zero = 0;
  CHECK(refusal([&] { check_fill(&zero, 0, 0, 0, false); }).empty());  // m == 0
  // the one-call form
  CHECK(refusal([&] { check_max_k(0, 6, 0, 0, false); }).empty());
  CHECK(refusal([&] { check_max_k(2, 6, 12, 12, true); }).empty());
  CHECK(has(refusal([&] { check_max_k(2, 6, 11, 0, false); }), "indices holds 11 entries but m * max_k is 12"));
  CHECK(has(refusal([&] { check_max_k(2, 6, 12, 11, true); }), "distances holds 11"));
  CHECK(has(refusal([&] { check_max_k(-1, 6, 12, 0, false); }), "negative"));
  CHECK(has(refusal([&] { check_max_k(INT64_MAX / 2, 6, 12, 0, false); }), "overflows"));
}

static void test_argument_checks()
{
  int64_t m = -1, n = -1, dim = -1;
  CHECK(check_rows(mat(5, 3), mat(7, 3), &m, &n, &dim) == rows_t::f32 && m == 5 && n == 7 && dim == 3);
  CHECK(check_rows(mat(0, 0, 2, 16), mat(4, 0, 2, 16), &m, &n, &dim) == rows_t::f16 && m == 0 && n == 4 && dim == 0);
  auto rows = [&](const tensor_desc& x, const tensor_desc& y) { return refusal([&] { check_rows(x, y, &m, &n, &dim); }); };
  CHECK(has(rows(mat(5, 3, 2, 64), mat(7, 3, 2, 64)), "fp64 rows are not supported"));
  CHECK(has(rows(mat(5, 3, 2, 32), mat(7, 3, 2, 16)), "same dtype"));
  CHECK(has(rows(mat(5, 3, 0, 8), mat(7, 3, 0, 8)), "fp32 or fp16"));
  CHECK(has(rows(mat(5, 3), mat(7, 4)), "dim mismatch: x has 3 columns, y has 4"));
  CHECK(has(rows(mat(5, 3), tensor_desc{}), "NULL"));
  CHECK(has(rows(vec(5, 2, 32), mat(7, 3)), "2-D"));
  tensor_desc t = mat(5, 3);
  t.contiguous  = false;
  CHECK(has(rows(t, mat(7, 3)), "x must be row-major and contiguous"));
  t = mat(7, 3);
  t.on_device = false;
  CHECK(has(rows(mat(5, 3), t), "y must be accessible on device memory"));

  CHECK(refusal([] { check_metric(4); }).empty());
  for (int metric : {0, 1, 2, 5, 6}) CHECK(has(refusal([=] { check_metric(metric); }), "Currently only L2Unexpanded distance metric is supported"));

  CHECK(refusal([] { check_adj(tensor_desc{}, 5, 7); }).empty());  // NULL: degrees only
  CHECK(refusal([] { check_adj(mat(5, 7, 1, 8), 5, 7); }).empty());
  CHECK(refusal([] { check_adj(mat(5, 7, 6, 8), 5, 7); }).empty());
  CHECK(has(refusal([] { check_adj(mat(5, 7, 2, 32), 5, 7); }), "bool or uint8"));
  CHECK(has(refusal([] { check_adj(mat(7, 5, 1, 8), 5, 7); }), "adj must have shape [5, 7]"));
  CHECK(has(refusal([] { check_adj(vec(35, 1, 8), 5, 7); }), "adj must have shape [5, 7]"));

  CHECK(check_row_vector(tensor_desc{}, 5, "vd", true, 7) == 0);
  CHECK(check_row_vector(vec(6), 5, "vd", true, 7) == 8);
  CHECK(check_row_vector(vec(6, 0, 32), 5, "vd", true, 7) == 4);
  CHECK(has(refusal([] { check_row_vector(vec(5), 5, "vd", true, 7); }), "vd must have shape [6] (m + 1)"));
  CHECK(has(refusal([] { check_row_vector(vec(6, 0, 32), 5, "indptr", false, 7); }), "indptr must be int64"));
  CHECK(has(refusal([] { check_row_vector(vec(6, 2, 32), 5, "vd", true, 7); }), "int32 or int64"));
  // int32 degrees: m * n below 2^31 only
  CHECK(check_row_vector(vec(32769, 0, 32), 32768, "vd", true, 65535) == 4);
  CHECK(has(refusal([] { check_row_vector(vec(32769, 0, 32), 32768, "vd", true, 65536); }), "vd must be int64 when m * n >= 2^31"));
  CHECK(has(refusal([] { check_row_vector(vec(4, 0, 32), 3, "vd", true, INT64_MAX / 2); }), "2^31"));
  CHECK(check_row_vector(vec(32769), 32768, "vd", true, 65536) == 8);

  CHECK(check_list(vec(9), "indices", false) == 9 && check_list(vec(9, 2, 32), "distances", true) == 9);
  CHECK(has(refusal([] { check_list(vec(9, 0, 32), "indices", false); }), "indices must be int64"));
  CHECK(has(refusal([] { check_list(vec(9), "distances", true); }), "distances must be fp32"));
  CHECK(has(refusal([] { check_list(mat(3, 3, 0, 64), "indices", false); }), "vector"));
}

static void test_slabs()
{
  CHECK(slab_row_bytes(1) == 17 + 8 && slab_row_bytes(128) == 25 && slab_row_bytes(129) == 42);
  CHECK(slab_rows(0, 100, 1 << 20, 0) == 0);
  CHECK(slab_rows(257, 300, 1 << 20, 100) == 100);   // forced
  CHECK(slab_rows(50, 300, 1 << 20, 100) == 50);
  CHECK(slab_rows(257, 300, int64_t(1) << 30, 0) == 257);  // everything fits
  CHECK(slab_rows(100000, 100000, 1, 0) == 128);     // never below one tile
  const int64_t rows = slab_rows(1000000, 100000, int64_t(2) << 30, 0);
  CHECK(rows % 128 == 0 && rows * slab_row_bytes(100000) <= (int64_t(2) << 30) && (rows + 128) * slab_row_bytes(100000) > (int64_t(2) << 30));
}

int main()
{
  test_offsets();
  test_fill_checks();
  test_argument_checks();
  test_slabs();
  if (g_failed != 0) return 1;
  std::printf("eps neighbors host OK\n");
  return 0;
}
