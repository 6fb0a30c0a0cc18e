/* ScaNN index build (reference: cpp/include/cuvs/neighbors/scann.hpp, C++ only and build-only there): balanced k-means
 * partitions, centres adjusted by anisotropic vector quantization (AVQ), a second "spilled" partition per row (SOAR), product
 * quantization of both residuals, an optional bf16 copy of the rows, and the .npy files that open-source ScaNN searches.
 * These entry points are extensions in the conventions of the cuvs* C layer. Implemented by cuvs_amd/csrc/scann.hip;
 * DESIGN.md 3.1z has the arithmetic, the deviations from what the reference executes and the kernels.
 *
 * Rows are fp32, row-major and contiguous, on the device or on the host (host rows are streamed in batches of at most 65536
 * and give the same index bit for bit). Finite inputs are the caller's responsibility. There is no search and no reader.
 */
#pragma once
#include <cuvs/core/c_api.h>
#include <cuvs/core/export.h>
#include <cuvs/distance/distance.h>
#include <dlpack/dlpack.h>
#include <stdbool.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* scann.hpp:40-85. pq_dim is the WIDTH of a subspace (dim % pq_dim == 0; dim / pq_dim codes per row), not their number. */
struct cuvsAmdScannIndexParams {
  cuvsDistanceType metric;      /* L2Expanded; recorded only */
  float metric_arg;             /* 2.0; recorded only */
  uint32_t n_leaves;            /* 1000 */
  int64_t kmeans_n_rows_train;  /* 100000 */
  uint32_t kmeans_n_iters;      /* 24 */
  float partitioning_eta;       /* 1: AVQ's eta for the centres, > 0 (1 = plain means) */
  float soar_lambda;            /* 1: SOAR's lambda, >= 0 */
  uint32_t pq_dim;              /* 8 */
  uint32_t pq_bits;             /* 8: 4 or 8 */
  int64_t pq_n_rows_train;      /* 100000: capped at 100000 */
  uint32_t pq_train_iters;      /* 10 */
  bool reordering_bf16;         /* false: keep a bf16 copy of the rows */
  float reordering_noise_shaping_threshold; /* NaN: round to nearest even; T: AVQ noise shaping of rows with |x| > T */
};
typedef struct cuvsAmdScannIndexParams* cuvsAmdScannIndexParams_t;

CUVS_EXPORT cuvsError_t cuvsAmdScannIndexParamsCreate(cuvsAmdScannIndexParams_t* params);
CUVS_EXPORT cuvsError_t cuvsAmdScannIndexParamsDestroy(cuvsAmdScannIndexParams_t params);

typedef struct {
  uintptr_t addr;
} cuvsAmdScannIndex;
typedef cuvsAmdScannIndex* cuvsAmdScannIndex_t;

CUVS_EXPORT cuvsError_t cuvsAmdScannIndexCreate(cuvsAmdScannIndex_t* index);
CUVS_EXPORT cuvsError_t cuvsAmdScannIndexDestroy(cuvsAmdScannIndex_t index);

/* dataset fp32 [n_rows, dim] on the device or on the host, n_rows >= n_leaves. Invalid parameters return CUVS_ERROR with a
 * text before anything is launched. */
CUVS_EXPORT cuvsError_t cuvsAmdScannBuild(cuvsResources_t res, cuvsAmdScannIndexParams_t params, DLManagedTensor* dataset,
                                          cuvsAmdScannIndex_t index);

/* Writes cuvs_metadata.bin, centers.npy, datapoint_to_token.npy, pq_codebook.npy, hashed_dataset.npy,
 * hashed_dataset_soar.npy and, with reordering_bf16, bf16_dataset.npy into the existing directory `dir`
 * (scann_serialize.cuh:107-142). */
CUVS_EXPORT cuvsError_t cuvsAmdScannSerialize(cuvsResources_t res, const char* dir, cuvsAmdScannIndex_t index);

CUVS_EXPORT cuvsError_t cuvsAmdScannIndexGetSize(cuvsAmdScannIndex_t index, int64_t* n_rows);
CUVS_EXPORT cuvsError_t cuvsAmdScannIndexGetDim(cuvsAmdScannIndex_t index, int64_t* dim);
CUVS_EXPORT cuvsError_t cuvsAmdScannIndexGetNLeaves(cuvsAmdScannIndex_t index, int64_t* n_leaves);
CUVS_EXPORT cuvsError_t cuvsAmdScannIndexGetPqDim(cuvsAmdScannIndex_t index, int64_t* pq_dim);
CUVS_EXPORT cuvsError_t cuvsAmdScannIndexGetPqBits(cuvsAmdScannIndex_t index, int64_t* pq_bits);
CUVS_EXPORT cuvsError_t cuvsAmdScannIndexHasBf16(cuvsAmdScannIndex_t index, bool* has_bf16);

/* Non-owning views (valid while the index lives); the caller supplies the DLManagedTensor and calls its deleter.
 * Device: centers fp32 [n_leaves, dim], labels and SOAR labels uint32 [n_rows], codebook fp32 [2^pq_bits, dim] (row e is
 * the concatenation over the subspaces of entry e). */
CUVS_EXPORT cuvsError_t cuvsAmdScannIndexGetCenters(cuvsAmdScannIndex_t index, DLManagedTensor* centers);
CUVS_EXPORT cuvsError_t cuvsAmdScannIndexGetLabels(cuvsAmdScannIndex_t index, DLManagedTensor* labels);
CUVS_EXPORT cuvsError_t cuvsAmdScannIndexGetSoarLabels(cuvsAmdScannIndex_t index, DLManagedTensor* soar_labels);
CUVS_EXPORT cuvsError_t cuvsAmdScannIndexGetPqCodebook(cuvsAmdScannIndex_t index, DLManagedTensor* codebook);
/* Host: codes of the primary and of the SOAR residual, uint8 [n_rows, dim / pq_dim], one byte per subspace whatever pq_bits;
 * the bf16 rows as int16 [n_rows, dim] (an error without reordering_bf16). */
CUVS_EXPORT cuvsError_t cuvsAmdScannIndexGetCodes(cuvsAmdScannIndex_t index, DLManagedTensor* codes);
CUVS_EXPORT cuvsError_t cuvsAmdScannIndexGetSoarCodes(cuvsAmdScannIndex_t index, DLManagedTensor* soar_codes);
CUVS_EXPORT cuvsError_t cuvsAmdScannIndexGetBf16Dataset(cuvsAmdScannIndex_t index, DLManagedTensor* bf16);

/* The three stages on their own. All tensors on the device, row-major and contiguous; labels are uint32 (or int32) [n_rows]
 * with values below n_leaves.
 *
 * AvqCenters: centers_inout fp32 [n_leaves, dim] holds the k-means centres and receives, for every leaf with members,
 *   eta * inverse(S I + (eta - 1) sum w3_i x_i x_i^T) * sum w1_i x_i, w1 = |x|^(eta - 1), w3 = |x|^(eta - 3), S = sum w1_i,
 *   members in ascending row id, then times one scalar: (sum_c <sum_{i in c} x_i, centre_c>) / (sum_c n_c |centre_c|^2)
 *   (1 when that is not finite or its denominator is 0). A zero row has weights 0; a leaf without weight keeps its centre.
 * SoarLabels: soar_labels_out uint32 [n_rows]: argmin_j ((a_j - p)^2 lambda - 2 b_j) + |c_j|^2 with r = x - c[label],
 *   rh = r / |r| (zeros when |r| = 0), p = <rh, x>, a_j = <rh, c_j>, b_j = <x, c_j>; every dot product one fp32 fma chain in
 *   ascending k, the lowest j on a tie, the primary leaf not excluded.
 * QuantizeBf16: out int16 [n_rows, dim]: the bf16 bits of every coordinate, rounded to nearest even (threshold NaN) or chosen
 *   by AVQ noise shaping for rows with |x| > threshold. */
CUVS_EXPORT cuvsError_t cuvsAmdScannAvqCenters(cuvsResources_t res, DLManagedTensor* dataset, DLManagedTensor* labels,
                                               DLManagedTensor* centers_inout, float eta);
CUVS_EXPORT cuvsError_t cuvsAmdScannSoarLabels(cuvsResources_t res, DLManagedTensor* dataset, DLManagedTensor* centers,
                                               DLManagedTensor* labels, float lambda, DLManagedTensor* soar_labels_out);
CUVS_EXPORT cuvsError_t cuvsAmdScannQuantizeBf16(cuvsResources_t res, DLManagedTensor* dataset, float threshold,
                                                 DLManagedTensor* out);

#ifdef __cplusplus
}
#endif
