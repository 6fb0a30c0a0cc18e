// Host-side steps shared by the IVF indexes (ivf_lists.hip): the fp32 coarse search (IVF-Flat, IVF-SQ, IVF-PQ), and for the
// indexes that keep their rows in the 64-row-interleaved list store (IVF-Flat, IVF-SQ) the store itself, list assignment
// and list growth. The scan kernels, the pack kernels and the serialisers stay with their index.
#pragma once
#include "ops.hpp"

#include <functional>
#include <vector>

namespace cuvs_amd {

// n_probes nearest centres of every query: probes [nq, n_probes] and their coarse distances pd, ordered best first
// (ivf_flat_search.cuh:104-187, ivf_pq_search.cuh:60-168). metric: inner product, cosine, anything else is L2.
// centers [n_lists, dim] with row pitch ld_centers; norms_sq = |c|^2 (L2), norms_sqrt = |c| (cosine).
// qn [nq]: |q|^2 after an L2 search, |q| after a cosine search, untouched for inner product.
// dist: the [batch_cap, n_lists] matrix of the plain form, allocated by the first call that does not take the grouped form.
void coarse_search(resources& res, const float* centers, int64_t ld_centers, uint32_t n_lists, uint32_t dim,
                   const float* norms_sq, const float* norms_sqrt, int metric, const float* qf, int64_t nq,
                   uint32_t n_probes, int64_t batch_cap, float* qn, dev_buf<float>& dist, float* pd, uint32_t* probes);

// All lists in one flat allocation, rows interleaved in groups of 64: [padded_rows / 64, n_chunks, 64, 16 bytes]. Every
// list starts at a multiple of 64 rows; in-list order is the order of arrival.
struct ivf_lists {
  uint32_t n_lists = 0;
  uint32_t n_chunks = 0;  // 16-byte chunks per row
  int64_t size = 0, padded_rows = 0;
  dev_buf<uint8_t> data;
  dev_buf<int64_t> indices;  // [padded_rows] source ids
  dev_buf<uint32_t> list_sizes, list_offsets;
  std::vector<uint32_t> h_list_sizes, h_list_offsets;
};

// List labels with the index metric, like the k-means that trained the centres (ivf_flat_build.cuh:179-200, :438): L2
// argmin; inner product -> the centre with the largest dot product (argmin of |c|^2 - 2 x.c with the |c|^2 term dropped),
// which is also how the search ranks the probes; cosine -> L2 on unit-length copies.
// centers [n_lists, dim] with their canonical |c|^2; x: fp32 device rows [n, dim], normalised IN PLACE for cosine.
void ivf_assign_lists(resources& res, int metric, const float* centers, const float* center_norms, uint32_t n_lists,
                      uint32_t dim, float* x, int64_t n, uint32_t* labels);
// rows of any element type, host or device: converted and labelled in batches
void ivf_assign_lists(resources& res, int metric, const float* centers, const float* center_norms, uint32_t n_lists,
                      uint32_t dim, const void* data, elem_t et, bool is_host, int64_t n, uint32_t* labels);

// What a pack launch needs besides its rows: new row j of the (list, row)-sorted order is source row perm[j], goes to
// list L = labels[perm[j]] at flat row list_off[L] + old_sizes[L] + (j - new_off[L]) of data / indices and gets the id
// new_ids[row] (nullptr: id_base + row).
struct ivf_pack_dest {
  const uint32_t *perm, *labels, *new_off, *old_sizes, *list_off;
  const int64_t* new_ids;
  int64_t id_base;
  uint8_t* data;
  int64_t* indices;
};
// pack(dest, j0, batch, src, src_is_batch): launch the index's pack kernel for sorted rows [j0, j0 + batch).
// src_is_batch 0: src is the whole device array; 1: src holds exactly these rows in sorted order (host staging).
using ivf_pack_fn = std::function<void(const ivf_pack_dest&, int64_t, int64_t, const void*, int)>;

// Appends n_new labelled rows (row_bytes each, host or device) to their lists in input order: new sizes and offsets, a
// new store with the old lists moved over, the pack launches, and the index fields published. new_ids: optional source
// ids, host or device.
void ivf_lists_grow(resources& res, ivf_lists& idx, const uint32_t* labels, const void* data, size_t row_bytes,
                    int64_t n_new, bool is_host, const int64_t* new_ids, bool ids_on_host, const ivf_pack_fn& pack);

// canonical |c|^2 of the centres; cosine: |c| as well
void ivf_set_center_norms(resources& res, int metric, const float* centers, uint32_t n_lists, uint32_t dim,
                          dev_buf<float>& norms_sq, dev_buf<float>& norms_sqrt);

// training sample of the IVF-SQ and IVF-RaBitQ builds: n_train distinct rows of n chosen by a seeded shuffle (all rows
// when n_train >= n), in ascending order
std::vector<uint32_t> pick_train_rows(int64_t n, int64_t n_train);

}  // namespace cuvs_amd
