/* Entry points of libcuvs_c.so that the reference's C headers do not declare. Everything a binding needs for the
 * reference's API lives in <cuvs/...>; these are additions in the same conventions (cuvsError_t, DLPack tensors).
 */
#pragma once
#include <cuvs/core/c_api.h>
#include <cuvs/core/export.h>
#include <cuvs/neighbors/all_neighbors.h>
#include <cuvs/neighbors/cagra.h>
#include <cuvs/neighbors/common.h>
#include <cuvs/neighbors/ivf_pq.h>
#include <cuvs/neighbors/tiered_index.h>
#include <cuvs/neighbors/vamana.h>
#include <cuvs/preprocessing/quantize/binary.h>
#include <cuvs/preprocessing/quantize/pq.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* IVF-PQ search with a pre-filter. The reference has this only in C++ - cuvs::neighbors::ivf_pq::search(..., const
 * filtering::base_filter& sample_filter), cpp/include/cuvs/neighbors/ivf_pq.hpp:1818-1828; kernel side
 * cpp/src/neighbors/ivf_pq/detail/jit_lto_kernels/compute_distances_impl.cuh:78-80 - its C entry point
 * cuvsIvfPqSearch (c/include/cuvs/neighbors/ivf_pq.h:536-541) takes no filter. Same argument convention as
 * cuvsIvfFlatSearch: filter.type NO_FILTER or BITSET, filter.addr = DLManagedTensor* of uint32 words on the device,
 * bit i = 1 keeps source id i. */
CUVS_EXPORT cuvsError_t cuvsAmdIvfPqSearchFiltered(cuvsResources_t res, cuvsIvfPqSearchParams_t search_params,
                                                   cuvsIvfPqIndex_t index, DLManagedTensor* queries,
                                                   DLManagedTensor* neighbors, DLManagedTensor* distances,
                                                   cuvsFilter filter);

/* Measured work of the CAGRA graph walks run on `res` (the hot path's algorithmic bytes per query are n_dist * dim *
 * sizeof(T) + n_iter * graph_degree * 4 with n_dist, n_iter measured; the reference keeps per-phase clock counters,
 * cpp/src/neighbors/detail/cagra/search_single_cta_jit.cuh:91-103,425-451). enable != 0 zeroes the counters and starts
 * counting; enable == 0 stops and fills out = {rows whose distance was computed, graph rows read, walkers (waves)}. */
CUVS_EXPORT cuvsError_t cuvsAmdCagraWorkCounters(cuvsResources_t res, int enable, uint64_t out[3]);

/* cagra::index_params::guarantee_connectivity (cpp/include/cuvs/neighbors/cagra.hpp:193; the spanning-forest pass of
 * graph::optimize, cpp/src/neighbors/detail/cagra/graph_core.cuh:1186-1581,1747-1760) is C++-only in the reference: the C
 * struct cuvsCagraIndexParams has no such field. The switch is kept on the handle and applies to every cuvsCagraBuild
 * made with it. */
CUVS_EXPORT cuvsError_t cuvsAmdCagraSetGuaranteeConnectivity(cuvsResources_t res, int on);

/* cuvs::neighbors::cagra::helpers::optimize (cpp/include/cuvs/neighbors/cagra_optimize.hpp): kNN graph [n, K] uint32 ->
 * search graph [n, degree] uint32 (prune by 2-hop detours, reverse edges, optional connectivity guarantee). Either
 * tensor may live on the host or on the device. */
CUVS_EXPORT cuvsError_t cuvsAmdCagraOptimize(cuvsResources_t res, DLManagedTensor* knn_graph, DLManagedTensor* graph,
                                             int guarantee_connectivity);

/* The intermediate kNN graph that cuvsCagraBuild optimises, made by params->build_algo for params->metric: uint32 [n, K] on
 * the device, K < n. Exposes the graph step alone (for BitwiseHamming: NN-descent, or the exact graph of
 * ITERATIVE_CAGRA_SEARCH / AUTO up to 200000 rows). */
CUVS_EXPORT cuvsError_t cuvsAmdCagraBuildKnnGraph(cuvsResources_t res, cuvsCagraIndexParams_t params, DLManagedTensor* dataset,
                                                  DLManagedTensor* knn_graph);

/* The VPQ dataset of a CAGRA index built with cuvsCagraIndexParams::compression or loaded from a file that holds one (the
 * reference exposes it through its C++ index only). cuvsAmdCagraIndexGetVpqInfo: out = {vq_n_centers,
 * pq_n_centers, pq_len, encoded row length in bytes, dim}; an error for an index that is not compressed.
 * cuvsAmdCagraIndexGetVpq fills caller-allocated device tensors: vq_book fp16 [vq_n_centers, dim], pq_book fp16 [256, pq_len],
 * codes uint8 [n, row length] in the reference's row layout: [uint32 VQ label][pq_dim code bytes][zero padding to 4 bytes]. */
CUVS_EXPORT cuvsError_t cuvsAmdCagraIndexGetVpqInfo(cuvsCagraIndex_t index, uint32_t out[5]);
CUVS_EXPORT cuvsError_t cuvsAmdCagraIndexGetVpq(cuvsResources_t res, cuvsCagraIndex_t index, DLManagedTensor* vq_book,
                                                DLManagedTensor* pq_book, DLManagedTensor* codes);

/* index.codes_layout() of the reference's C++ index (cpp/include/cuvs/neighbors/ivf_pq.hpp:40-90; the C ABI sets the layout in
 * cuvsIvfPqIndexParams but has no getter): 0 = CUVS_IVF_PQ_LIST_LAYOUT_FLAT, 1 = CUVS_IVF_PQ_LIST_LAYOUT_INTERLEAVED. */
CUVS_EXPORT cuvsError_t cuvsAmdIvfPqIndexGetCodesLayout(cuvsIvfPqIndex_t index, int* layout);

/* The trained thresholds of a binary quantizer (cuvs::preprocessing::quantize::binary::quantizer<T>::threshold; the C ABI
 * has no getter): copied into `out`, a 1-D tensor of the quantizer's dtype and length dim on the host or the device. A ZERO
 * quantizer holds no thresholds: out must then have length 0. */
CUVS_EXPORT cuvsError_t cuvsAmdBinaryQuantizerGetThreshold(cuvsResources_t res, cuvsBinaryQuantizer_t quantizer,
                                                           DLManagedTensor* out);

/* A product quantizer over caller-supplied codebooks (no reference counterpart; books trained elsewhere, and the tests' way
 * to pin the encoder without k-means). pq_codebook: device fp32 [pq_dim * 2^pq_bits, pq_len] when params->use_subspaces,
 * else [2^pq_bits, pq_len]; params->pq_dim must be set. vq_codebook: device fp32 [vq_n_centers, pq_dim * pq_len] or NULL
 * (then use_vq is off whatever params says). The books are copied. */
CUVS_EXPORT cuvsError_t cuvsAmdProductQuantizerFromCodebooks(cuvsResources_t res, cuvsProductQuantizerParams_t params,
                                                             DLManagedTensor* pq_codebook, DLManagedTensor* vq_codebook,
                                                             cuvsProductQuantizer_t quantizer);
/* Encoder launches since the library was loaded (the tests' proof of which path ran): out = {default encoder, plain encoder,
 * default encoder with more than one row per lane (taken when ceil(n / (256 R)) >= 2 * compute units; R = 4 up to pq_len 8,
 * 2 up to pq_len 32)}; out[2] is part of out[0]. */
CUVS_EXPORT void cuvsAmdPqEncodeCounters(unsigned long long out[3]);

/* The two steps of a batched cuvsAllNeighborsBuild on their own (no reference counterpart; how the tests pin the batched
 * build to a restatement). cuvsAmdAllNeighborsPartition: the clustering step, same code path as the build and deterministic -
 * dataset_host fp32 [n, dim] on the host; centroids_out fp32 [n_clusters, dim] (host or device); nearest_clusters_out int64
 * [n, overlap_factor] on the host, row i = the clusters row i is assigned to, nearest first. */
CUVS_EXPORT cuvsError_t cuvsAmdAllNeighborsPartition(cuvsResources_t res, cuvsAllNeighborsIndexParams_t params,
                                                     DLManagedTensor* dataset_host, DLManagedTensor* centroids_out,
                                                     DLManagedTensor* nearest_clusters_out);
/* cuvsAmdAllNeighborsMerge: one launch of the remap-merge kernel. All tensors on the device: inverted_indices int64 [m] (the
 * cluster's global row ids), batch_indices int64 [m, k] LOCAL ids, batch_distances fp32 [m, k]; global_indices int64 [n, k]
 * and global_distances fp32 [n, k] are updated in place. select_min 0: larger distances are better (inner product). */
CUVS_EXPORT cuvsError_t cuvsAmdAllNeighborsMerge(cuvsResources_t res, DLManagedTensor* inverted_indices,
                                                 DLManagedTensor* batch_indices, DLManagedTensor* batch_distances,
                                                 DLManagedTensor* global_indices, DLManagedTensor* global_distances,
                                                 int select_min);

/* Tiered index (cuvsTieredIndex*). cuvsAmdTieredIndexGetInfo: rows held, rows served by the ANN tier (0: no
 * ANN tier), rows the storage has room for, row width; any out pointer may be NULL. cuvsAmdTieredIndexCompact: the reference's
 * C++ tiered_index::compact (its C ABI has none) - rebuilds the ANN tier over all rows with the stored build parameters when
 * the tail is not empty. */
CUVS_EXPORT cuvsError_t cuvsAmdTieredIndexGetInfo(cuvsTieredIndex_t index, int64_t* size, int64_t* ann_rows, int64_t* capacity,
                                                  int64_t* dim);
CUVS_EXPORT cuvsError_t cuvsAmdTieredIndexCompact(cuvsResources_t res, cuvsTieredIndex_t index);
/* The two inputs of a tiered search's merge for the same call (arguments as cuvsTieredIndexSearch; all four outputs [m, k] on the
 * device, int64 / fp32): ann_* = what the ANN tier's own search returns, with that tier's own padding for missing slots; tail_* =
 * the exact top-k of the tail rows with global ids, INT64_MAX / FLT_MAX (-FLT_MAX for inner product) in the slots the tail cannot
 * fill. An absent tier's outputs are all padding (INT64_MAX and the worst distance). */
CUVS_EXPORT cuvsError_t cuvsAmdTieredIndexSearchTiers(cuvsResources_t res, void* search_params, cuvsTieredIndex_t index,
                                                      DLManagedTensor* queries, DLManagedTensor* ann_neighbors,
                                                      DLManagedTensor* ann_distances, DLManagedTensor* tail_neighbors,
                                                      DLManagedTensor* tail_distances, cuvsFilter prefilter);
/* The tail phase of a tiered search on its own (how the tests pin the kernels to a restatement): seed_neighbors int64 / seed_distances
 * fp32 [m, k] play the ANN result over rows [0, ann_rows) (padding recognised by id), tail fp32 [n_tail, dim] holds the rows with
 * global ids ann_rows + j, bitset (NULL or uint32 words over the global ids, 1 keeps) filters the tail; neighbors / distances [m, k]
 * receive the merged result. All tensors on the device. path 0: the library's choice, 1: the composed path (threshold append + merge
 * kernel), 2: the single-launch small-batch kernel (refused beyond its shapes). */
CUVS_EXPORT cuvsError_t cuvsAmdTieredTailSearch(cuvsResources_t res, cuvsDistanceType metric, DLManagedTensor* tail, int64_t ann_rows,
                                                DLManagedTensor* queries, DLManagedTensor* seed_neighbors,
                                                DLManagedTensor* seed_distances, DLManagedTensor* bitset, int path,
                                                DLManagedTensor* neighbors, DLManagedTensor* distances);
/* One launch of the tiered merge kernel: A int64 / fp32 [m, k] (an ANN result over rows [0, ann_rows), padding recognised by id) and
 * B int64 / fp32 [m, kb] (entries with id INT64_MAX are padding) -> the first k of the union by (distance, id), inner product by
 * (-distance, id), into out_* [m, k]; the slots that remain hold INT64_MAX / the worst distance. All tensors on the device. */
CUVS_EXPORT cuvsError_t cuvsAmdTieredMerge(cuvsResources_t res, DLManagedTensor* a_neighbors, DLManagedTensor* a_distances,
                                           DLManagedTensor* b_neighbors, DLManagedTensor* b_distances, int64_t ann_rows,
                                           int select_min, DLManagedTensor* out_neighbors, DLManagedTensor* out_distances);
/* Launch counts since the library was loaded (the tests' proof of which path ran): out = {composed tail phases, single-launch tail
 * phases, single-launch tail phases redone because an append buffer overflowed}. */
CUVS_EXPORT void cuvsAmdTieredCounters(unsigned long long out[3]);

/* Vamana (cuvsVamana*). The reference's C ABI cannot read the graph back. cuvsAmdVamanaIndexGetGraph copies it
 * into `out`, uint32 [n, graph_degree] on the host or the device (unused slots 0xFFFFFFFF, behind the used ones; the rows can
 * be handed to cuvsCagraIndexFromArgs once those slots are replaced). cuvsAmdVamanaIndexGetMedoid: the entry node. */
CUVS_EXPORT cuvsError_t cuvsAmdVamanaIndexGetGraph(cuvsResources_t res, cuvsVamanaIndex_t index, DLManagedTensor* out);
CUVS_EXPORT cuvsError_t cuvsAmdVamanaIndexGetMedoid(cuvsVamanaIndex_t index, uint32_t* medoid);
/* One launch of the build's search kernel on a GIVEN graph (how the tests pin the kernel to a restatement). All tensors on the
 * device: dataset [n, dim] float32 / int8 / uint8, graph uint32 [n, params->graph_degree], query_ids uint32 [m] (rows of the
 * dataset); out_ids uint32 / out_dists fp32 [m, visited_size] (visited_size after rounding) receive the expanded nodes of each
 * walk from `medoid`, nearest first, without the query row itself, padded with 0xFFFFFFFF / FLT_MAX. */
CUVS_EXPORT cuvsError_t cuvsAmdVamanaGreedySearch(cuvsResources_t res, cuvsVamanaIndexParams_t params, DLManagedTensor* dataset,
                                                  DLManagedTensor* graph, uint32_t medoid, DLManagedTensor* query_ids,
                                                  DLManagedTensor* out_ids, DLManagedTensor* out_dists);
/* One launch of the build's prune kernel: for node_ids[i] the candidates cand_ids / cand_dists [m, visited_size] (padding
 * 0xFFFFFFFF; cand_dists as cuvsAmdVamanaGreedySearch gives them) are merged with the node's row of `graph` and pruned to
 * out_ids uint32 [m, graph_degree], padded with 0xFFFFFFFF. All tensors on the device; `graph` is not written. */
CUVS_EXPORT cuvsError_t cuvsAmdVamanaRobustPrune(cuvsResources_t res, cuvsVamanaIndexParams_t params, DLManagedTensor* dataset,
                                                 DLManagedTensor* graph, DLManagedTensor* node_ids, DLManagedTensor* cand_ids,
                                                 DLManagedTensor* cand_dists, DLManagedTensor* out_ids);
/* The sector-aligned SSD layout of DiskANN (the reference's C++ serialize(..., sector_aligned = true)): `<filename>_disk.index`
 * holds a 4096-byte sector with the nine uint64 metadata words, then the nodes (row, uint32 count, ids) packed per sector, or one
 * node over several sectors when it does not fit one. With include_dataset also `<filename>.data`. No PQ output. */
CUVS_EXPORT cuvsError_t cuvsAmdVamanaSerializeSectorAligned(cuvsResources_t res, const char* filename, cuvsVamanaIndex_t index,
                                                            bool include_dataset);

/* Measurement helpers of bench.py (no reference counterpart). cuvsAmdProfileEnable / cuvsAmdProfileCollect: HIP events
 * around the named kernels on the handle's stream (Collect sums and resets the records of `name`, returns the launch count).
 * cuvsAmdIvfPqLastFilterStats: counters of the last IVF-PQ search made by a handle created under CUVS_AMD_SCAN_DEBUG=1024
 * (behind CUVS_AMD_DEBUG_SWITCHES=1): out = {(row, query) pairs screened by the matrix-core filter, survivors re-scored,
 * 32-row subtiles decoded, work units}. */
CUVS_EXPORT int cuvsAmdDebugSwitchesCompiledIn(void); /* 0: built with -DCUVS_AMD_NO_DEBUG_SWITCHES (make PRODUCTION=1) */
CUVS_EXPORT void cuvsAmdProfileEnable(int on);
CUVS_EXPORT int cuvsAmdProfileCollect(const char* name, double* total_ms);
CUVS_EXPORT void cuvsAmdIvfPqLastFilterStats(unsigned long long out[4]);
/* the same + out[4] = (query, probe) pairs handed back to the LUT scan kernels, out[5] = candidates that went through the
 * shared overflow list */
CUVS_EXPORT void cuvsAmdIvfPqLastFilterStats6(unsigned long long out[6]);
/* Test hook over the functions that hand the matrix-core filter's work units to its waves: out = {cost key of a unit of `rows`
 * rows and `groups` groups of 32 queries when row chunks have up to `unit_rows` rows (0: no rows, placed last), units in the
 * share of XCD `xcd` out of `n_units`, array position of that share's ticket `t`} - strided != 0: the shares of the cost order. */
CUVS_EXPORT void cuvsAmdIvfPqUnitOrderHook(uint32_t rows, uint32_t groups, uint32_t unit_rows, uint32_t n_units, uint32_t xcd,
                                           uint32_t t, int strided, uint32_t out[3]);

/* Sweeps of the Jacobi eigensolver that the calling thread's last cuvsPcaFit / cuvsPcaFitTransform ran (a sweep that rotated
 * nothing is not counted). Test and tuning hook for cuvsPcaParams::tol and n_iterations. */
CUVS_EXPORT cuvsError_t cuvsAmdPcaLastSweeps(int* sweeps);

#ifdef __cplusplus
}
#endif
