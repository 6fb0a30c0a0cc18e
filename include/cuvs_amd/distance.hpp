// C++ surface over the C ABI of include/cuvs_amd/masked_nn.h: cuvs::distance::masked_l2_nn (cpp/src/distance/masked_nn.cuh) and
// cuvs::neighbors::cross_component_nn (cpp/src/sparse/neighbors/cross_component_nn.cuh). Header-only, C++17, no HIP and no RAFT
// headers; views, resources and errors are those of neighbors.hpp. fp32 rows only (masked_nn.h has the contract).
#pragma once
#include <cuvs_amd/masked_nn.h>
#include <cuvs_amd/neighbors.hpp>

namespace cuvs {
namespace distance {

struct masked_l2_nn_params {
  bool sqrt            = false;
  bool init_out_buffer = true;  // false: reduce into the values out_idx / out_dist already hold
};

// adj bool [m, n_groups]; group_idxs int64 [n_groups]: the end index of every group of rows of y; x_norm / y_norm may be null
inline void masked_l2_nn(const resources& res, const masked_l2_nn_params& params, device_matrix_view<const float> x,
                         device_matrix_view<const float> y, const float* x_norm, const float* y_norm, device_matrix_view<const bool> adj,
                         const int64_t* group_idxs, int64_t* out_idx, float* out_dist)
{
  detail::tensor<const float> tx(x), ty(y);
  detail::tensor<const bool> ta(adj);
  detail::vector_tensor<const float> txn(x_norm, x.extent(0)), tyn(y_norm, y.extent(0)), td(out_dist, x.extent(0));
  detail::vector_tensor<const int64_t> tg(group_idxs, adj.extent(1)), ti(out_idx, x.extent(0));
  check(cuvsAmdMaskedL2NN(res.get(), tx.get(), ty.get(), txn.get(), tyn.get(), ta.get(), &tg.m, params.sqrt, params.init_out_buffer,
                          ti.get(), td.get()),
        "cuvsAmdMaskedL2NN");
}

}  // namespace distance

namespace neighbors {

// row_nn_idx / row_nn_dist [n] may be null; edge_src, edge_dst, edge_weight [n_components]
inline void cross_component_nn(const resources& res, device_matrix_view<const float> x, const int32_t* colors, int64_t n_components,
                               int64_t* row_nn_idx, float* row_nn_dist, int64_t* edge_src, int64_t* edge_dst, float* edge_weight,
                               bool sqrt = false)
{
  detail::tensor<const float> tx(x);
  detail::vector_tensor<const int32_t> tc(colors, x.extent(0));
  detail::vector_tensor<int64_t> ti(row_nn_idx, x.extent(0)), ts(edge_src, n_components), tt(edge_dst, n_components);
  detail::vector_tensor<float> td(row_nn_dist, x.extent(0)), tw(edge_weight, n_components);
  check(cuvsAmdCrossComponentNN(res.get(), tx.get(), tc.get(), n_components, sqrt, ti.get(), td.get(), ts.get(), tt.get(), tw.get()),
        "cuvsAmdCrossComponentNN");
}

}  // namespace neighbors
}  // namespace cuvs
