// C++ surface over the C ABI of include/cuvs_amd/binary_knn.h: exact Hamming kNN and Hamming distance matrices over packed bit
// codes. Header-only, C++17, no HIP headers; views, resources and errors are those of neighbors.hpp. T is uint8_t or int8_t;
// the views are contiguous (a row pitch beyond nbytes needs the C entry points and their strides).
#pragma once
#include <cuvs_amd/binary_knn.h>
#include <cuvs_amd/neighbors.hpp>

namespace cuvs {
namespace neighbors {
namespace binary_brute_force {

// neighbors int64 [m, k], distances fp32 [m, k]: the k rows of dataset with the smallest (Hamming distance, id) per query
template <typename T>
void knn(const resources& res, device_matrix_view<const T> dataset, device_matrix_view<const T> queries,
         device_matrix_view<int64_t> neighbors, device_matrix_view<float> distances)
{
  detail::tensor<const T> d(dataset), q(queries);
  detail::tensor<int64_t> n(neighbors);
  detail::tensor<float> o(distances);
  cuvsFilter none{0, NO_FILTER};
  check(cuvsAmdBinaryKnn(res.get(), d.get(), q.get(), n.get(), o.get(), none), "cuvsAmdBinaryKnn");
}
// the same among the rows whose bit of the filter is set
template <typename T>
void knn(const resources& res, device_matrix_view<const T> dataset, device_matrix_view<const T> queries,
         device_matrix_view<int64_t> neighbors, device_matrix_view<float> distances, const filtering::bitset_filter& sample_filter)
{
  detail::tensor<const T> d(dataset), q(queries);
  detail::tensor<int64_t> n(neighbors);
  detail::tensor<float> o(distances);
  detail::tensor<const uint32_t> f(device_matrix_view<const uint32_t>{sample_filter.words, 1, (sample_filter.n_bits + 31) / 32, false});
  cuvsFilter flt{reinterpret_cast<uintptr_t>(f.get()), BITSET};
  check(cuvsAmdBinaryKnn(res.get(), d.get(), q.get(), n.get(), o.get(), flt), "cuvsAmdBinaryKnn");
}

// out fp32 [m, n]: hamming(x[i], y[j])
template <typename T>
void pairwise_distance(const resources& res, device_matrix_view<const T> x, device_matrix_view<const T> y, device_matrix_view<float> out)
{
  detail::tensor<const T> tx(x), ty(y);
  detail::tensor<float> o(out);
  check(cuvsAmdBinaryPairwiseDistance(res.get(), tx.get(), ty.get(), o.get()), "cuvsAmdBinaryPairwiseDistance");
}

}  // namespace binary_brute_force
}  // namespace neighbors
}  // namespace cuvs
