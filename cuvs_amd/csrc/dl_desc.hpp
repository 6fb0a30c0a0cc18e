// What the host-only argument checks (eps_neighbors_host.hpp, ball_cover_host.hpp) need to know of a DLTensor.
#pragma once

#include "common.hpp"
#include "eps_neighbors_host.hpp"

namespace cuvs_amd {

inline eps_host::tensor_desc desc_of(const DLManagedTensor* t)
{
  eps_host::tensor_desc d;
  if (t == nullptr) return d;
  const DLTensor& s = t->dl_tensor;
  d.present    = true;
  d.ndim       = s.ndim;
  for (int i = 0; i < 2 && i < s.ndim; ++i) d.shape[i] = s.shape[i];
  bool empty = false;
  for (int i = 0; i < s.ndim; ++i) empty = empty || s.shape[i] == 0;
  d.contiguous = empty || is_c_contiguous(s);  // (no element: the strides say nothing)
  d.on_device  = is_device_accessible(s);
  d.code       = s.dtype.code;
  d.bits       = s.dtype.bits;
  d.lanes      = s.dtype.lanes;
  return d;
}

}  // namespace cuvs_amd
