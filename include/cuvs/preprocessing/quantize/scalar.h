/*
 * Scalar quantizer entry points — drop-in for c/include/cuvs/preprocessing/quantize/scalar.h.
 * Struct field order and sizes are ABI: callers read and write fields directly.
 * Implemented by cuvs_amd/csrc/scalar_quantize.hip.
 *
 * Host tensors are processed on the host and need no device: `res` may then be 0.
 *
 * x -> int8: -128 at or below min_, 127 at or above max_, round(255 (x - min_) / (max_ - min_) - 128) between.
 */
#pragma once
#include <cuvs/core/c_api.h>
#include <cuvs/core/export.h>
#include <dlpack/dlpack.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

struct cuvsScalarQuantizerParams {
  float quantile; /* 0.99: share of the sampled elements inside [min_, max_], centred; in (0, 1] */
};
typedef struct cuvsScalarQuantizerParams* cuvsScalarQuantizerParams_t;
CUVS_EXPORT cuvsError_t cuvsScalarQuantizerParamsCreate(cuvsScalarQuantizerParams_t* params);
CUVS_EXPORT cuvsError_t cuvsScalarQuantizerParamsDestroy(cuvsScalarQuantizerParams_t params);

typedef struct {
  double min_;
  double max_;
} cuvsScalarQuantizer;
typedef cuvsScalarQuantizer* cuvsScalarQuantizer_t;
CUVS_EXPORT cuvsError_t cuvsScalarQuantizerCreate(cuvsScalarQuantizer_t* quantizer);
CUVS_EXPORT cuvsError_t cuvsScalarQuantizerDestroy(cuvsScalarQuantizer_t quantizer);

/* dataset host or device, fp16/fp32/fp64, row-major [n, dim], free of NaN (the quantile is an order statistic: NaN has no
 * place in the order, as in the reference's sort) */
CUVS_EXPORT cuvsError_t cuvsScalarQuantizerTrain(cuvsResources_t res,
                                                 cuvsScalarQuantizerParams_t params,
                                                 DLManagedTensor* dataset,
                                                 cuvsScalarQuantizer_t quantizer);

/* out int8 [n, dim] in the same kind of memory as the dataset */
CUVS_EXPORT cuvsError_t cuvsScalarQuantizerTransform(cuvsResources_t res,
                                                     cuvsScalarQuantizer_t quantizer,
                                                     DLManagedTensor* dataset,
                                                     DLManagedTensor* out);

/* dataset int8 [n, dim]; out fp16/fp32/fp64 [n, dim] in the same kind of memory */
CUVS_EXPORT cuvsError_t cuvsScalarQuantizerInverseTransform(cuvsResources_t res,
                                                            cuvsScalarQuantizer_t quantizer,
                                                            DLManagedTensor* dataset,
                                                            DLManagedTensor* out);
#ifdef __cplusplus
}
#endif
