// The ScaNN index as scann.hip builds it and scann_search.hip searches it.
#pragma once
#include "common.hpp"
#include "scann_host.hpp"

#include <cuvs_amd/scann.h>

#include <memory>
#include <mutex>
#include <vector>

namespace cuvs_amd {

struct scann_search_lists;  // scann_search.hip: built by the first search, under search_mu

struct scann_index {
  scann_host::params p;
  int64_t n = 0, dim = 0, n_leaves = 0, n_sub = 0, book_n = 0;
  dev_buf<float> centers, codebook;
  dev_buf<uint32_t> labels, soar_labels;
  std::vector<uint8_t> codes, soar_codes;
  std::vector<int16_t> bf16;
  int device = 0;
  std::mutex search_mu;
  std::shared_ptr<scann_search_lists> search;
};

inline scann_index& index_of(cuvsAmdScannIndex_t index)
{
  if (index == nullptr || index->addr == 0) scann_host::refuse("the ScaNN index is not built");
  return *reinterpret_cast<scann_index*>(index->addr);
}

}  // namespace cuvs_amd
