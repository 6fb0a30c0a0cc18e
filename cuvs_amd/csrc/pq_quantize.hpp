// What pq_quantize.hip offers to the rest of the library: the product quantizer behind cuvsProductQuantizer*, its training and
// its encoder (canonical arithmetic in the file header of pq_quantize.hip). CAGRA's VPQ compression (cagra.hip) is built on it.
#pragma once
#include "common.hpp"

#include <cuvs/preprocessing/quantize/pq.h>

#include <memory>

namespace cuvs_amd {

struct product_quantizer {
  cuvsProductQuantizerParams p{};  // filled: pq_dim and vq_n_centers are the values in use
  int64_t dim     = 0;
  int64_t pq_len  = 0;
  int64_t book_n  = 0;             // 2^pq_bits
  int64_t vq_n    = 0;             // 0: no VQ
  dev_buf<float> pq_book;          // [pq_dim * book_n, pq_len] (use_subspaces) or [book_n, pq_len]
  dev_buf<float> vq_book;          // [vq_n, dim]
  int64_t code_bytes() const { return ((int64_t)p.pq_dim * p.pq_bits + 7) / 8; }
};

struct f32_rows {
  const float* data;
  int64_t n, dim;
  bool device;
};

// trains the VQ centres (use_vq) and the PQ codebook(s) on strided subsamples of `ds`
std::unique_ptr<product_quantizer> pq_build(resources& res, const cuvsProductQuantizerParams& params, const f32_rows& ds);
// codes [n, code_bytes] of the device rows x [n, dim] with row pitch ld; labels [n]: the VQ centre of every row (with VQ)
void pq_encode(resources& res, const product_quantizer& q, const float* x, int64_t ld, int64_t n, const uint32_t* labels,
               uint8_t* codes);

}  // namespace cuvs_amd
