// C++ surface over the C ABI of include/cuvs_amd/single_linkage.h: cuvs::cluster::agglomerative::{single_linkage,
// helpers::build_linkage, helpers::build_dendrogram} with the reference's names (cpp/include/cuvs/cluster/agglomerative.hpp).
// Header-only, C++17, no HIP and no RAFT headers; views, resources and errors are those of neighbors.hpp.
#pragma once
#include <cuvs_amd/neighbors.hpp>
#include <cuvs_amd/single_linkage.h>

#include <variant>

namespace cuvs {
namespace cluster {
namespace agglomerative {

enum Linkage { PAIRWISE = 0, KNN_GRAPH = 1 };

// dendrogram [n - 1, 2] and labels [n] on the device, IdxT int32_t or int64_t
template <typename IdxT>
void single_linkage(const resources& res, device_matrix_view<const float> X, device_matrix_view<IdxT> dendrogram, IdxT* labels,
                    cuvsDistanceType metric, int64_t n_clusters, Linkage linkage = KNN_GRAPH, int c = 15)
{
  detail::tensor<const float> tx(X);
  detail::tensor<IdxT> td(dendrogram);
  detail::vector_tensor<IdxT> tl(labels, X.extent(0));
  check(cuvsAmdSingleLinkage(res.get(), tx.get(), td.get(), tl.get(), metric, n_clusters, (cuvsAmdLinkage)linkage, c),
        "cuvsAmdSingleLinkage");
}

namespace helpers {

namespace linkage_graph_params {
struct distance_params {
  int c           = 15;
  Linkage dist_linkage = KNN_GRAPH;
};
struct mutual_reachability_params {
  int min_samples = 5;
  float alpha     = 1.0f;
  cuvsAllNeighborsIndexParams_t all_neighbors_params = nullptr;  // borrowed; nullptr: brute force
};
}  // namespace linkage_graph_params

using linkage_params = std::variant<linkage_graph_params::distance_params, linkage_graph_params::mutual_reachability_params>;

// out_mst_* [n - 1], dendrogram [n - 1, 2], out_distances and out_sizes [n - 1], core_dists [n] (mutual reachability only);
// null pointers leave an output out
template <typename IdxT>
void build_linkage(const resources& res, device_matrix_view<const float> X, const linkage_params& params, cuvsDistanceType metric,
                   IdxT* out_mst_src, IdxT* out_mst_dst, float* out_mst_weights, device_matrix_view<IdxT> dendrogram,
                   float* out_distances, IdxT* out_sizes, float* core_dists = nullptr)
{
  using c_params = detail::c_params<cuvsAmdLinkageParams_t, cuvsAmdLinkageParamsCreate, cuvsAmdLinkageParamsDestroy>;
  c_params cp;
  if (const auto* d = std::get_if<linkage_graph_params::distance_params>(&params)) {
    cp.p->space   = CUVS_AMD_LINKAGE_SPACE_DISTANCE;
    cp.p->c       = d->c;
    cp.p->linkage = (cuvsAmdLinkage)d->dist_linkage;
  } else {
    const auto& m = std::get<linkage_graph_params::mutual_reachability_params>(params);
    cp.p->space                = CUVS_AMD_LINKAGE_SPACE_MUTUAL_REACHABILITY;
    cp.p->min_samples          = m.min_samples;
    cp.p->alpha                = m.alpha;
    cp.p->all_neighbors_params = m.all_neighbors_params;
  }
  const int64_t n = X.extent(0);
  detail::tensor<const float> tx(X);
  detail::tensor<IdxT> td(dendrogram);
  detail::vector_tensor<IdxT> ts(out_mst_src, n - 1), tt(out_mst_dst, n - 1), tz(out_sizes, n - 1);
  detail::vector_tensor<float> tw(out_mst_weights, n - 1), tdist(out_distances, n - 1), tc(core_dists, n);
  check(cuvsAmdBuildLinkage(res.get(), tx.get(), cp.p, metric, ts.get(), tt.get(), tw.get(), dendrogram.ptr ? td.get() : nullptr,
                            tdist.get(), tz.get(), tc.get()),
        "cuvsAmdBuildLinkage");
}

// rows, cols, data: the n - 1 edges of a spanning tree in merge order, on the device
template <typename IdxT>
void build_dendrogram(const resources& res, const IdxT* rows, const IdxT* cols, const float* data, int64_t nnz,
                      device_matrix_view<IdxT> children, float* out_delta, IdxT* out_size)
{
  detail::vector_tensor<const IdxT> tr(rows, nnz), tc(cols, nnz);
  detail::vector_tensor<const float> tv(data, nnz);
  detail::tensor<IdxT> tch(children);
  detail::vector_tensor<float> td(out_delta, nnz);
  detail::vector_tensor<IdxT> ts(out_size, nnz);
  check(cuvsAmdBuildDendrogram(res.get(), tr.get(), tc.get(), tv.get(), tch.get(), td.get(), ts.get()), "cuvsAmdBuildDendrogram");
}

}  // namespace helpers
}  // namespace agglomerative
}  // namespace cluster
}  // namespace cuvs
