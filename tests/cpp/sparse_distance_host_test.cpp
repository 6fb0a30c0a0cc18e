// Stand-alone test of cuvs_amd/csrc/sparse_distance_host.hpp (built with -fsanitize=address,undefined by
// tests/test_sparse_distance_cpu.py): the metric-to-family table, batch arithmetic, the plan of virtual rows, the slab size,
// the validator's verdicts and the refusals, against hand-written cases.
#include "sparse_distance_host.hpp"

#include <cstdio>
#include <cstring>
#include <functional>
#include <vector>

using namespace cuvs_amd::sparse_host;

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

static tensor_desc vec(int64_t len, int code, int bits)
{
  tensor_desc t;
  t.present = true; t.ndim = 1; t.shape[0] = len; t.code = code; t.bits = bits;
  return t;
}
static tensor_desc mat(int64_t r, int64_t c, int code, int bits)
{
  tensor_desc t;
  t.present = true; t.ndim = 2; t.shape[0] = r; t.shape[1] = c; t.code = code; t.bits = bits;
  return t;
}

static void test_metric_table()
{
  int isect = 0, uni = 0;
  for (int m = -1; m <= 25; ++m) {
    const int f = family_of(m);
    isect += f == kIntersection;
    uni += f == kUnion;
  }
  CHECK(isect == 10 && uni == 8);  // the 18 metrics of the reference's dispatch
  CHECK(family_of(Haversine) == kNone && family_of(BrayCurtis) == kNone && family_of(BitwiseHamming) == kNone);
  CHECK(family_of(InnerProduct) == kIntersection && family_of(KLDivergence) == kIntersection && family_of(JensenShannon) == kUnion);
  CHECK(!select_min(InnerProduct) && select_min(CosineExpanded) && select_min(L1));
  CHECK(combine_of(Linf) == kCombineMax && combine_of(HammingUnexpanded) == kCombineCount && combine_of(L1) == kCombineAdd);
  CHECK(has(refusal([] { check_metric(Haversine, 0.f); }), "Haversine"));
  CHECK(has(refusal([] { check_metric(BrayCurtis, 0.f); }), "BrayCurtis"));
  CHECK(has(refusal([] { check_metric(77, 0.f); }), "77"));
  CHECK(has(refusal([] { check_metric(LpUnexpanded, 0.f); }), "p"));
  CHECK(has(refusal([] { check_metric(LpUnexpanded, -1.f); }), "p"));
  CHECK(has(refusal([] { check_metric(LpUnexpanded, std::nanf("")); }), "p"));
  CHECK(refusal([] { check_metric(LpUnexpanded, 1.5f); }).empty());
  CHECK(refusal([] { check_metric(L1, 0.f); }).empty());  // metric_arg matters to Lp only
}

static void test_csr_checks()
{
  const tensor_desc ip = vec(5, 0, 32), ix = vec(9, 0, 32), dv = vec(9, 2, 32);
  CHECK(check_csr(ip, ix, dv, 4, 10, "x") == 9);
  CHECK(has(refusal([&] { check_csr(ip, ix, dv, 5, 10, "x"); }), "rows + 1"));
  CHECK(has(refusal([&] { check_csr(vec(5, 0, 64), ix, dv, 4, 10, "x"); }), "indptr must be int32"));
  CHECK(has(refusal([&] { check_csr(ip, vec(9, 0, 64), dv, 4, 10, "x"); }), "indices must be int32"));
  CHECK(has(refusal([&] { check_csr(ip, ix, vec(9, 2, 64), 4, 10, "x"); }), "data must be fp32"));
  CHECK(has(refusal([&] { check_csr(ip, ix, vec(9, 2, 16), 4, 10, "x"); }), "data must be fp32"));
  CHECK(has(refusal([&] { check_csr(ip, ix, vec(8, 2, 32), 4, 10, "x"); }), "entries"));
  CHECK(has(refusal([&] { check_csr(ip, vec(int64_t(1) << 31, 0, 32), vec(int64_t(1) << 31, 2, 32), 4, 10, "x"); }), "2^31"));
  CHECK(has(refusal([&] { check_csr(ip, ix, dv, 4, -1, "x"); }), "negative"));
  tensor_desc host = ix;
  host.on_device = false;
  CHECK(has(refusal([&] { check_csr(ip, host, dv, 4, 10, "x"); }), "device"));
  tensor_desc none;
  CHECK(has(refusal([&] { check_csr(none, ix, dv, 4, 10, "x"); }), "NULL"));
  CHECK(has(refusal([&] { check_csr(ip, mat(3, 3, 0, 32), dv, 4, 10, "x"); }), "vectors"));
  // out
  CHECK(refusal([&] { check_out(mat(4, 7, 2, 32), 4, 7); }).empty());
  CHECK(has(refusal([&] { check_out(mat(4, 7, 2, 64), 4, 7); }), "fp32"));
  CHECK(has(refusal([&] { check_out(mat(7, 4, 2, 32), 4, 7); }), "shape"));
  tensor_desc host_out = mat(4, 7, 2, 32);
  host_out.on_device = false;
  CHECK(has(refusal([&] { check_out(host_out, 4, 7); }), "device"));
  // kNN outputs
  CHECK(check_knn(mat(6, 3, 0, 64), mat(6, 3, 2, 32), 6, 3, 10, 4, 4) == 8);
  CHECK(check_knn(mat(6, 3, 0, 32), mat(6, 3, 2, 32), 6, 3, 3, 4, 4) == 4);
  CHECK(has(refusal([&] { check_knn(mat(6, 3, 0, 64), mat(6, 3, 2, 32), 6, 3, 2, 4, 4); }), "larger than the number of index rows"));
  CHECK(has(refusal([&] { check_knn(mat(6, 0, 0, 64), mat(6, 0, 2, 32), 6, 0, 2, 4, 4); }), "positive"));
  CHECK(has(refusal([&] { check_knn(mat(6, 3, 1, 32), mat(6, 3, 2, 32), 6, 3, 10, 4, 4); }), "int64 or int32"));
  CHECK(has(refusal([&] { check_knn(mat(6, 3, 0, 64), mat(6, 3, 2, 16), 6, 3, 10, 4, 4); }), "fp32"));
  CHECK(has(refusal([&] { check_knn(mat(6, 2, 0, 64), mat(6, 3, 2, 32), 6, 3, 10, 4, 4); }), "shape"));
  CHECK(has(refusal([&] { check_knn(mat(6, 3, 0, 64), mat(6, 3, 2, 32), 6, 3, 10, 0, 4); }), "batch_size"));
  CHECK(has(refusal([&] { check_knn(mat(6, 3, 0, 64), mat(6, 3, 2, 32), 6, 3, 10, 4, -2); }), "batch_size"));
}

static void test_batches()
{
  CHECK(n_batches(0, 5) == 0 && n_batches(1, 5) == 1 && n_batches(5, 5) == 1 && n_batches(6, 5) == 2 && n_batches(300, 64) == 5);
  int64_t covered = 0, b0, cnt;
  for (int64_t b = 0; b < n_batches(300, 64); ++b) {
    batch_rows(300, 64, b, &b0, &cnt);
    CHECK(b0 == covered && cnt > 0 && cnt <= 64);
    covered += cnt;
  }
  CHECK(covered == 300);
  batch_rows(9, 2, 4, &b0, &cnt);
  CHECK(b0 == 8 && cnt == 1);
  // the distance tile under the workspace budget
  int64_t bi = 32768, bq = 32768;
  cap_tile(int64_t(2) << 30, &bi, &bq);
  CHECK(bi == 32768 && bq == 16384 && bi * bq * 4 <= (int64_t(2) << 30));
  bi = 300; bq = 70;
  cap_tile(int64_t(2) << 30, &bi, &bq);
  CHECK(bi == 300 && bq == 70);
  bi = 1000; bq = 1000;
  cap_tile(4 * 500, &bi, &bq);
  CHECK(bi == 500 && bq == 1);
  CHECK(n_tiles(5, 300, 1) == 4 && n_tiles(5, 300, 2) == 2 && n_tiles(5, 300, 8) == 2 && n_tiles(8, kThreads * 4 + 1, 4) == 4 && n_tiles(0, 10, 1) == 0);
  CHECK(n_ranges(0, kRangeI) == 0 && n_ranges(1, kRangeI) == 1 && n_ranges(kRangeI, kRangeI) == 1 && n_ranges(kRangeI + 1, kRangeI) == 2);
}

static void test_plan()
{
  // rows of 0, 3, split, split + 1, 2 * split + 5 and 0 stored entries, behind an offset of 7
  const int lens[] = {0, 3, 8, 9, 21, 0};
  std::vector<int> indptr = {7};
  for (int l : lens) indptr.push_back(indptr.back() + l);
  std::vector<vrow> v;
  std::vector<split_row> s;
  plan_vrows(indptr.data(), 0, 6, 8, &v, &s);
  CHECK(v.size() == 4 + 2 + 3 && s.size() == 2 && total_slots(s) == 5);
  CHECK(s[0].row == 3 && s[0].first_slot == 0 && s[0].pieces == 2 && s[1].row == 4 && s[1].first_slot == 2 && s[1].pieces == 3);
  // every stored entry belongs to exactly one virtual row, in order; unsplit rows have no slot
  int pos = 7, slot = 0;
  for (const vrow& r : v) {
    CHECK(r.begin == pos || r.begin == r.end);
    CHECK(r.end - r.begin <= 8 && r.begin >= indptr[r.row] && r.end <= indptr[r.row + 1]);
    if (r.end - r.begin == indptr[r.row + 1] - indptr[r.row]) CHECK(r.slot == -1);
    else CHECK(r.slot == slot++);
    pos = r.begin == r.end ? pos : r.end;
  }
  CHECK(pos == indptr.back() && slot == 5);
  CHECK(v[3].begin == 18 && v[3].end == 26 && v[4].begin == 26 && v[4].end == 27);  // the row just past the threshold: 8 + 1
  // a slice: rows relative to r0, positions absolute
  plan_vrows(indptr.data(), 3, 2, 8, &v, &s);
  CHECK(v.size() == 5 && v[0].row == 0 && v[0].begin == 18 && v[2].row == 1 && s[1].row == 1 && s[1].first_slot == 2);
  // a long row that ends at nnz = 2^31 - 1: the piece ends are computed in 64 bits
  const std::vector<int> top = {INT_MAX - 20, INT_MAX};
  plan_vrows(top.data(), 0, 1, 8, &v, &s);
  CHECK(v.size() == 3 && v[0].begin == INT_MAX - 20 && v[1].begin == INT_MAX - 12 && v[2].begin == INT_MAX - 4 && v[2].end == INT_MAX);
  CHECK(s.size() == 1 && s[0].pieces == 3);
  plan_vrows(indptr.data(), 0, 0, 8, &v, &s);
  CHECK(v.empty() && s.empty() && total_slots(s) == 0);
  // slabs
  CHECK(slab_rows(0, 5, 1 << 20) == 0 && slab_rows(100, 0, 1 << 20) == 100);
  CHECK(slab_rows(100, 5, 4 * 5 * 40) == 40 && slab_rows(100, 5, 4 * 5 * 43) == 40 && slab_rows(100, 5, 1) == kTA);
  CHECK(slab_rows(3, 5, 1 << 30) == 3);
}

static void test_verdicts()
{
  CHECK(refusal([] { check_verdict(kValid, "x", 4, 9, 10); }).empty());
  CHECK(has(refusal([] { check_verdict(verdict_key(0, kBadIndptr0), "x", 4, 9, 10); }), "indptr[0]"));
  CHECK(has(refusal([] { check_verdict(verdict_key(2, kBadIndptrOrder), "x", 4, 9, 10); }), "row 2"));
  CHECK(has(refusal([] { check_verdict(verdict_key(4, kBadIndptrEnd), "x", 4, 9, 10); }), "indptr[4] is not nnz (9)"));
  CHECK(has(refusal([] { check_verdict(verdict_key(3, kBadColumn), "x", 4, 9, 10); }), "row 3 holds a column outside [0, 10)"));
  CHECK(has(refusal([] { check_verdict(verdict_key(1, kBadOrder), "x", 4, 9, 10); }), "row 1 are not strictly ascending"));
  CHECK(verdict_key(1, kBadOrder) < verdict_key(2, kBadIndptrOrder));  // the first bad row wins
}

int main()
{
  test_metric_table();
  test_csr_checks();
  test_batches();
  test_plan();
  test_verdicts();
  if (g_failed != 0) return 1;
  std::printf("sparse distance host OK\n");
  return 0;
}
