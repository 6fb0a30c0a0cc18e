// The C++ surface of include/cuvs_amd/stats.hpp on the inputs tests/test_stats_gpu.py writes to a file: it prints what
// cuvs::stats::* returns, and the test compares that with the Python functions and the C calls. Built and run by that test.
// File: int64 n, dim, dim_e, n_labels, k, chunk; X fp32 [n, dim]; X_embedded fp32 [n, dim_e]; labels int32 [n]; neighbors int64 [n, k].
#include <cuvs_amd/stats.hpp>

#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

#define HIPCHECK(e) do { if ((e) != hipSuccess) { std::printf("HIP error line %d\n", __LINE__); return 2; } } while (0)

template <typename T>
static bool read_all(std::FILE* f, std::vector<T>& v) { return std::fread(v.data(), sizeof(T), v.size(), f) == v.size(); }

int main(int argc, char** argv)
{
  if (argc != 2) return 3;
  std::FILE* f = std::fopen(argv[1], "rb");
  if (f == nullptr) return 3;
  int64_t h[6];
  if (std::fread(h, 8, 6, f) != 6) return 3;
  const int64_t n = h[0], dim = h[1], dim_e = h[2], n_labels = h[3], k = h[4], chunk = h[5];
  std::vector<float> x(n * dim), e(n * dim_e);
  std::vector<int32_t> y(n);
  std::vector<int64_t> nb(n * k);
  if (!read_all(f, x) || !read_all(f, e) || !read_all(f, y) || !read_all(f, nb)) return 3;
  std::fclose(f);
  float *dx, *de, *ds;
  int32_t *dy, *dr;
  int64_t* dn;
  HIPCHECK(hipMalloc((void**)&dx, x.size() * 4)); HIPCHECK(hipMalloc((void**)&de, e.size() * 4));
  HIPCHECK(hipMalloc((void**)&ds, n * 4)); HIPCHECK(hipMalloc((void**)&dy, n * 4));
  HIPCHECK(hipMalloc((void**)&dr, n * k * 4)); HIPCHECK(hipMalloc((void**)&dn, n * k * 8));
  HIPCHECK(hipMemcpy(dx, x.data(), x.size() * 4, hipMemcpyHostToDevice));
  HIPCHECK(hipMemcpy(de, e.data(), e.size() * 4, hipMemcpyHostToDevice));
  HIPCHECK(hipMemcpy(dy, y.data(), n * 4, hipMemcpyHostToDevice));
  HIPCHECK(hipMemcpy(dn, nb.data(), n * k * 8, hipMemcpyHostToDevice));
  try {
    cuvs::resources res;
    auto X  = cuvs::make_device_matrix_view<const float>(dx, n, dim);
    auto E  = cuvs::make_device_matrix_view<const float>(de, n, dim_e);
    auto NB = cuvs::make_device_matrix_view<const int64_t>(dn, n, k);
    auto R  = cuvs::make_device_matrix_view<int32_t>(dr, n, k);
    namespace st = cuvs::stats;
    const float plain   = st::silhouette_score(res, X, dy, ds, n_labels, L2SqrtUnexpanded);
    std::vector<float> s(n);
    HIPCHECK(hipMemcpy(s.data(), ds, n * 4, hipMemcpyDeviceToHost));
    const float batched = st::silhouette_score_batched(res, X, dy, nullptr, n_labels, chunk, L2SqrtUnexpanded);
    const double mean   = st::silhouette_score_f64(res, X, dy, nullptr, n_labels, chunk, L2SqrtUnexpanded);
    if (plain != batched || plain != (float)mean) return 1;
    std::printf("silhouette %a\n", mean);
    double sum = 0.0;
    for (float v : s) sum += (double)v;
    std::printf("scores_sum %a\n", sum);
    const uint64_t penalty = st::neighbor_ranks(res, X, NB, R);
    std::vector<int32_t> r(n * k);
    HIPCHECK(hipMemcpy(r.data(), dr, n * k * 4, hipMemcpyDeviceToHost));
    long long rank_sum = 0;
    for (int32_t v : r) rank_sum += v;
    if (st::neighbor_ranks(res, X, NB, cuvs::device_matrix_view<int32_t>{}) != penalty) return 1;
    std::printf("penalty %llu\nrank_sum %lld\n", (unsigned long long)penalty, rank_sum);
    std::printf("trustworthiness %a\n", st::trustworthiness_score(res, X, E, (int)k));
    // a refusal arrives as an exception that carries the library's message
    try {
      st::silhouette_score(res, X, dy, ds, 1);
      return 1;
    } catch (const std::exception& ex) {
      std::printf("refusal %s\n", ex.what());
    }
  } catch (const std::exception& ex) {
    std::printf("exception: %s\n", ex.what());
    return 1;
  }
  std::printf("stats api OK\n");
  return 0;
}
