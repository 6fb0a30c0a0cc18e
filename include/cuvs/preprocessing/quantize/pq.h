/*
 * Product quantizer entry points — drop-in for c/include/cuvs/preprocessing/quantize/pq.h.
 * Struct field order and sizes are ABI: callers mutate fields directly.
 * Implemented by cuvs_amd/csrc/pq_quantize.hip.
 *
 * A row [dim] is cut into pq_dim pieces of pq_len = dim / pq_dim columns; each piece (minus the row's VQ centre when
 * use_vq) is replaced by the index of its nearest codebook entry. Code j of a row occupies bits
 * [j * pq_bits, (j + 1) * pq_bits) of the row's bytes, little endian.
 */
#pragma once
#include <cuvs/cluster/kmeans.h>
#include <cuvs/core/c_api.h>
#include <cuvs/core/export.h>
#include <dlpack/dlpack.h>
#include <stdbool.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

struct cuvsProductQuantizerParams {
  uint32_t pq_bits;        /* 8: bits per code, in [4, 16] */
  uint32_t pq_dim;         /* 0: codes per row; dim % pq_dim == 0; 0 -> ceil(dim / 4) */
  bool use_subspaces;      /* true: one codebook per piece; false: one codebook shared by all pieces */
  bool use_vq;             /* false; true: rows are first replaced by their residual to a k-means centre */
  uint32_t vq_n_centers;   /* 0 -> sqrt(n_rows) rounded up to a multiple of 8 */
  uint32_t kmeans_n_iters; /* 25: k-means iterations, VQ and PQ */
  cuvsKMeansType pq_kmeans_type;            /* CUVS_KMEANS_TYPE_KMEANS_BALANCED: the k-means that trains the PQ codebooks */
  uint32_t max_train_points_per_pq_code;    /* 256: PQ trains on min(n_rows, this * 2^pq_bits) rows */
  uint32_t max_train_points_per_vq_cluster; /* 1024: VQ trains on min(n_rows, this * vq_n_centers) rows */
};
typedef struct cuvsProductQuantizerParams* cuvsProductQuantizerParams_t;
CUVS_EXPORT cuvsError_t cuvsProductQuantizerParamsCreate(cuvsProductQuantizerParams_t* params);
CUVS_EXPORT cuvsError_t cuvsProductQuantizerParamsDestroy(cuvsProductQuantizerParams_t params);

/* dtype: the element type of the training data (float32) */
typedef struct {
  uintptr_t addr;
  DLDataType dtype;
} cuvsProductQuantizer;
typedef cuvsProductQuantizer* cuvsProductQuantizer_t;
CUVS_EXPORT cuvsError_t cuvsProductQuantizerCreate(cuvsProductQuantizer_t* quantizer);
CUVS_EXPORT cuvsError_t cuvsProductQuantizerDestroy(cuvsProductQuantizer_t quantizer);

/* dataset host or device, fp32, row-major [n, dim] */
CUVS_EXPORT cuvsError_t cuvsProductQuantizerBuild(cuvsResources_t res,
                                                  cuvsProductQuantizerParams_t params,
                                                  DLManagedTensor* dataset,
                                                  cuvsProductQuantizer_t quantizer);

/* dataset host or device fp32 [n, dim]; codes_out device uint8 [n, ceil(pq_dim * pq_bits / 8)]; vq_labels device uint32 [n]
 * or NULL (written only when the quantizer uses VQ) */
CUVS_EXPORT cuvsError_t cuvsProductQuantizerTransform(cuvsResources_t res,
                                                      cuvsProductQuantizer_t quantizer,
                                                      DLManagedTensor* dataset,
                                                      DLManagedTensor* codes_out,
                                                      DLManagedTensor* vq_labels);

/* pq_codes device uint8 [n, encoded_dim]; out device fp32 [n, dim]; vq_labels device uint32 [n], required with VQ */
CUVS_EXPORT cuvsError_t cuvsProductQuantizerInverseTransform(cuvsResources_t res,
                                                             cuvsProductQuantizer_t quantizer,
                                                             DLManagedTensor* pq_codes,
                                                             DLManagedTensor* out,
                                                             DLManagedTensor* vq_labels);

CUVS_EXPORT cuvsError_t cuvsProductQuantizerGetPqBits(cuvsProductQuantizer_t quantizer, uint32_t* pq_bits);
CUVS_EXPORT cuvsError_t cuvsProductQuantizerGetPqDim(cuvsProductQuantizer_t quantizer, uint32_t* pq_dim);
/* non-owning device views: fp32 [pq_dim * 2^pq_bits, pq_len] (use_subspaces) or [2^pq_bits, pq_len]; the VQ codebook is
 * fp32 [vq_n_centers, dim], empty when VQ is off. They live as long as the quantizer. */
CUVS_EXPORT cuvsError_t cuvsProductQuantizerGetPqCodebook(cuvsProductQuantizer_t quantizer, DLManagedTensor* pq_codebook);
CUVS_EXPORT cuvsError_t cuvsProductQuantizerGetVqCodebook(cuvsProductQuantizer_t quantizer, DLManagedTensor* vq_codebook);
/* bytes per encoded row: ceil(pq_dim * pq_bits / 8) */
CUVS_EXPORT cuvsError_t cuvsProductQuantizerGetEncodedDim(cuvsProductQuantizer_t quantizer, uint32_t* encoded_dim);
CUVS_EXPORT cuvsError_t cuvsProductQuantizerGetUseVq(cuvsProductQuantizer_t quantizer, bool* use_vq);
#ifdef __cplusplus
}
#endif
