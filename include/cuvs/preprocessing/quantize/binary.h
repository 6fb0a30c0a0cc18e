/*
 * Binary quantizer entry points — drop-in for c/include/cuvs/preprocessing/quantize/binary.h.
 * Struct field order and sizes are ABI: callers mutate fields directly.
 * Implemented by cuvs_amd/csrc/binary_quantize.hip.
 */
#pragma once
#include <cuvs/core/c_api.h>
#include <cuvs/core/export.h>
#include <dlpack/dlpack.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* bit j of output byte b is set when x[8b + j] > threshold[8b + j]; MEAN and SAMPLING_MEDIAN are per dimension */
enum cuvsBinaryQuantizerThreshold { ZERO = 0, MEAN = 1, SAMPLING_MEDIAN = 2 };

struct cuvsBinaryQuantizerParams {
  enum cuvsBinaryQuantizerThreshold threshold; /* MEAN */
  float sampling_ratio;                        /* 0.1: share of the rows SAMPLING_MEDIAN sorts, in (0, 1] */
};
typedef struct cuvsBinaryQuantizerParams* cuvsBinaryQuantizerParams_t;
CUVS_EXPORT cuvsError_t cuvsBinaryQuantizerParamsCreate(cuvsBinaryQuantizerParams_t* params);
CUVS_EXPORT cuvsError_t cuvsBinaryQuantizerParamsDestroy(cuvsBinaryQuantizerParams_t params);

/* dtype: the element type of the training data (thresholds are stored in it) */
typedef struct {
  uintptr_t addr;
  DLDataType dtype;
} cuvsBinaryQuantizer;
typedef cuvsBinaryQuantizer* cuvsBinaryQuantizer_t;
CUVS_EXPORT cuvsError_t cuvsBinaryQuantizerCreate(cuvsBinaryQuantizer_t* quantizer);
CUVS_EXPORT cuvsError_t cuvsBinaryQuantizerDestroy(cuvsBinaryQuantizer_t quantizer);

/* dataset host or device, fp16/fp32/fp64, row-major [n, dim] */
CUVS_EXPORT cuvsError_t cuvsBinaryQuantizerTrain(cuvsResources_t res,
                                                 cuvsBinaryQuantizerParams_t params,
                                                 DLManagedTensor* dataset,
                                                 cuvsBinaryQuantizer_t quantizer);

/* threshold ZERO; out uint8 [>= n, >= ceil(dim / 8)] in the same kind of memory as the dataset */
CUVS_EXPORT cuvsError_t cuvsBinaryQuantizerTransform(cuvsResources_t res, DLManagedTensor* dataset, DLManagedTensor* out);

/* the trained thresholds; the dataset dtype must be the quantizer's */
CUVS_EXPORT cuvsError_t cuvsBinaryQuantizerTransformWithParams(cuvsResources_t res,
                                                               cuvsBinaryQuantizer_t quantizer,
                                                               DLManagedTensor* dataset,
                                                               DLManagedTensor* out);
#ifdef __cplusplus
}
#endif
