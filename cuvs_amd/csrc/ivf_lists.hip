// Host-side steps shared by the IVF indexes: see ivf_lists.hpp.
#include "ivf_lists.hpp"

#include <algorithm>
#include <cstring>
#include <numeric>
#include <random>

namespace cuvs_amd {

namespace {

// one workgroup per list: its ids and its whole 64-row groups to the list's place in the new store
__global__ void relocate_lists_kernel(const uint8_t* __restrict__ old_data, const int64_t* __restrict__ old_ids,
                                      const uint32_t* __restrict__ old_off, const uint32_t* __restrict__ old_sizes,
                                      const uint32_t* __restrict__ new_off, uint32_t n_chunks,
                                      uint8_t* __restrict__ data, int64_t* __restrict__ ids)
{
  const uint32_t L  = blockIdx.x;
  const uint32_t sz = old_sizes[L];
  const int64_t so = old_off[L], dn = new_off[L];
  for (uint32_t i = threadIdx.x; i < sz; i += blockDim.x) ids[dn + i] = old_ids[so + i];
  const size_t n16 = (size_t)((sz + 63) / 64) * n_chunks * 64;
  const uint4* s = reinterpret_cast<const uint4*>(old_data + (size_t)(so >> 6) * n_chunks * 1024);
  uint4* d       = reinterpret_cast<uint4*>(data + (size_t)(dn >> 6) * n_chunks * 1024);
  for (size_t i = threadIdx.x; i < n16; i += blockDim.x) d[i] = s[i];
}

// inner product: the |c|^2 term of the argmin is dropped - a zeroed array stands in for the centre norms
const float* label_norms(resources& res, int metric, const float* center_norms, uint32_t n_lists, dev_buf<float>& zero_norms)
{
  if (metric != M_InnerProduct) return center_norms;
  zero_norms = dev_buf<float>(res, n_lists);
  HIP_TRY(hipMemsetAsync(zero_norms.data(), 0, zero_norms.bytes(), res.stream));
  return zero_norms.data();
}

void assign_batch(resources& res, int metric, const float* centers, const float* norms, uint32_t n_lists, uint32_t dim,
                  float* x, int64_t cnt, uint32_t* labels)
{
  if (metric == M_CosineExpanded) normalize_rows(res, x, cnt, dim);  // rows are assigned on unit-length copies
  fused_l2_argmin<float>(res, x, cnt, dim, centers, n_lists, dim, norms, labels, nullptr);
}

}  // namespace

void coarse_search(resources& res, const float* centers, int64_t ld_centers, uint32_t n_lists, uint32_t dim,
                   const float* norms_sq, const float* norms_sqrt, int metric, const float* qf, int64_t nq,
                   uint32_t n_probes, int64_t batch_cap, float* qn, dev_buf<float>& dist, float* pd, uint32_t* probes)
{
  const bool ipm = metric == M_InnerProduct, cosm = metric == M_CosineExpanded;
  // 1 - q.c / (|q| |c|): the same ranking as the reference's -q.c / (|q| |c|) (ivf_flat_search.cuh:130-175)
  const int family    = ipm ? (int)M_InnerProduct : (cosm ? (int)M_CosineExpanded : (int)M_L2Expanded);
  const float* cnorms = ipm ? nullptr : (cosm ? norms_sqrt : norms_sq);
  // Common shapes: distances in grouped layout + the best key of every 16-centre group, selection from the keys and the
  // qualifying groups only (ops.hpp: pairwise_distance_grouped / select_k_grouped) - the values, their order
  // and the tie rule are those of the plain form below
  if (res.tune.coarse_grouped != 0 && select_k_grouped_ok(n_lists, (int)n_probes)) {
    const int64_t ldo = round_up((int64_t)n_lists, 128);
    dev_buf<float> gdist(res, (size_t)nq * ldo);
    dev_buf<uint32_t> gkeys(res, (size_t)nq * (ldo / 16));
    if (!ipm) row_norms<float>(res, qf, nq, dim, dim, qn, cosm);
    if (pairwise_distance_grouped(res, qf, nq, dim, centers, n_lists, ld_centers, dim, ipm ? nullptr : qn, cnorms, family,
                                  gdist.data(), ldo, gkeys.data(), ldo / 16)) {
      select_k_grouped(res, gdist.data(), ldo, gkeys.data(), ldo / 16, nq, n_lists, (int)n_probes, pd, probes, !ipm);
      return;
    }
  }
  if (dist.data() == nullptr) dist = dev_buf<float>(res, (size_t)batch_cap * n_lists);
  if (!ipm) row_norms<float>(res, qf, nq, dim, dim, qn, cosm);
  pairwise_distance<float, float>(res, qf, nq, dim, centers, n_lists, ld_centers, dim, ipm ? nullptr : qn, cnorms, family,
                                  dist.data(), n_lists);
  select_k<uint32_t, uint32_t>(res, dist.data(), nullptr, nq, n_lists, n_lists, (int)n_probes, pd, probes, !ipm);
}

void ivf_assign_lists(resources& res, int metric, const float* centers, const float* center_norms, uint32_t n_lists,
                      uint32_t dim, float* x, int64_t n, uint32_t* labels)
{
  dev_buf<float> zero_norms;
  assign_batch(res, metric, centers, label_norms(res, metric, center_norms, n_lists, zero_norms), n_lists, dim, x, n, labels);
}

void ivf_assign_lists(resources& res, int metric, const float* centers, const float* center_norms, uint32_t n_lists,
                      uint32_t dim, const void* data, elem_t et, bool is_host, int64_t n, uint32_t* labels)
{
  dev_buf<float> zero_norms;
  const float* norms       = label_norms(res, metric, center_norms, n_lists, zero_norms);
  const int64_t batch_rows = std::max<int64_t>(1024, std::min<int64_t>(n, (int64_t(1) << 28) / dim));
  dev_buf<float> xb(res, (size_t)std::min(batch_rows, n) * dim);
  for (int64_t r0 = 0; r0 < n; r0 += batch_rows) {
    const int64_t cnt = std::min(batch_rows, n - r0);
    load_range_as_float(res, data, et, is_host, dim, r0, cnt, xb.data());
    assign_batch(res, metric, centers, norms, n_lists, dim, xb.data(), cnt, labels + r0);
  }
}

void ivf_lists_grow(resources& res, ivf_lists& idx, const uint32_t* labels, const void* data, size_t row_bytes,
                    int64_t n_new, bool is_host, const int64_t* new_ids, bool ids_on_host, const ivf_pack_fn& pack)
{
  dev_buf<int64_t> ids_dev;
  if (new_ids && ids_on_host) {
    ids_dev = dev_buf<int64_t>(res, n_new);
    copy_async(res, ids_dev.data(), new_ids, n_new * sizeof(int64_t));
    new_ids = ids_dev.data();
  }
  // rows appended to their lists in input order: perm = rows ordered by (label, row)
  dev_buf<uint32_t> perm(res, n_new), new_off(res, idx.n_lists + 1);
  group_by_label(res, labels, n_new, idx.n_lists, perm.data(), new_off.data());
  std::vector<uint32_t> h_new_off = to_host(res, new_off.data(), idx.n_lists + 1);
  std::vector<uint32_t> sizes(idx.n_lists), offs(idx.n_lists + 1);
  int64_t total = 0;
  for (uint32_t L = 0; L < idx.n_lists; ++L) {
    sizes[L] = idx.h_list_sizes[L] + (h_new_off[L + 1] - h_new_off[L]);
    offs[L]  = (uint32_t)total;
    total += round_up(sizes[L], 64);
  }
  offs[idx.n_lists] = (uint32_t)total;
  auto ndata    = dev_buf<uint8_t>::persistent((size_t)total * idx.n_chunks * 16);
  auto nindices = dev_buf<int64_t>::persistent((size_t)total);
  HIP_TRY(hipMemsetAsync(ndata.data(), 0, ndata.bytes(), res.stream));
  HIP_TRY(hipMemsetAsync(nindices.data(), 0xff, nindices.bytes(), res.stream));
  dev_buf<uint32_t> d_list_off(res, idx.n_lists + 1);
  copy_async(res, d_list_off.data(), offs.data(), offs.size() * sizeof(uint32_t));
  if (idx.size > 0) {
    hipLaunchKernelGGL(relocate_lists_kernel, dim3(idx.n_lists), dim3(256), 0, res.stream, idx.data.data(),
                       idx.indices.data(), idx.list_offsets.data(), idx.list_sizes.data(), d_list_off.data(),
                       idx.n_chunks, ndata.data(), nindices.data());
  }
  ivf_pack_dest dest;
  dest.perm = perm.data(); dest.labels = labels; dest.new_off = new_off.data(); dest.old_sizes = idx.list_sizes.data();
  dest.list_off = d_list_off.data(); dest.new_ids = new_ids; dest.id_base = idx.size;
  dest.data = ndata.data(); dest.indices = nindices.data();
  if (!is_host) {
    const int64_t pb = int64_t(1) << 22;  // rows per pack launch
    for (int64_t j0 = 0; j0 < n_new; j0 += pb) pack(dest, j0, std::min(pb, n_new - j0), data, 0);
  } else {
    // host rows: permuted into sorted order on the host, staged and packed batch by batch
    std::vector<uint32_t> h_perm = to_host(res, perm.data(), n_new);
    const int64_t hb = std::max<int64_t>(1, std::min<int64_t>(n_new, (int64_t(1) << 28) / (int64_t)row_bytes));
    std::vector<char> host((size_t)hb * row_bytes);
    dev_buf<char> stage(res, host.size());
    const char* src = static_cast<const char*>(data);
    for (int64_t j0 = 0; j0 < n_new; j0 += hb) {
      const int64_t cnt = std::min(hb, n_new - j0);
      for (int64_t i = 0; i < cnt; ++i)
        memcpy(host.data() + (size_t)i * row_bytes, src + (size_t)h_perm[j0 + i] * row_bytes, row_bytes);
      copy_async(res, stage.data(), host.data(), (size_t)cnt * row_bytes);
      pack(dest, j0, cnt, stage.data(), 1);
      sync(res);
    }
  }
  HIP_TRY(hipGetLastError());
  sync(res);
  idx.data    = std::move(ndata);
  idx.indices = std::move(nindices);
  copy_async(res, idx.list_sizes.data(), sizes.data(), sizes.size() * sizeof(uint32_t));
  copy_async(res, idx.list_offsets.data(), offs.data(), offs.size() * sizeof(uint32_t));
  sync(res);
  idx.h_list_sizes   = sizes;
  idx.h_list_offsets = offs;
  idx.size += n_new;
  idx.padded_rows = total;
}

void ivf_set_center_norms(resources& res, int metric, const float* centers, uint32_t n_lists, uint32_t dim,
                          dev_buf<float>& norms_sq, dev_buf<float>& norms_sqrt)
{
  norms_sq = dev_buf<float>::persistent(n_lists);
  row_norms<float>(res, centers, n_lists, dim, dim, norms_sq.data(), false);
  if (metric == M_CosineExpanded) {
    norms_sqrt = dev_buf<float>::persistent(n_lists);
    row_norms<float>(res, centers, n_lists, dim, dim, norms_sqrt.data(), true);
  }
}

std::vector<uint32_t> pick_train_rows(int64_t n, int64_t n_train)
{
  std::vector<uint32_t> pick((size_t)n);
  std::iota(pick.begin(), pick.end(), 0u);
  if (n_train < n) {
    std::mt19937_64 rng(137);
    for (int64_t i = 0; i < n_train; ++i) {
      const int64_t j = i + (int64_t)(rng() % (uint64_t)(n - i));
      std::swap(pick[i], pick[j]);
    }
    pick.resize((size_t)n_train);
    std::sort(pick.begin(), pick.end());
  }
  return pick;
}

}  // namespace cuvs_amd
