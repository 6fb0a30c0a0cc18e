// Core C-ABI: resources, stream, allocation, last-error text, matrix copy/slice.
// Replaces c/src/core/c_api.cpp of the reference (same symbols, same error convention).
#include <cuvs/version_config.h>
#include "common.hpp"

#include <cuvs/core/c_api.h>

#include "scratch_cache.hpp"

#include <algorithm>
#include <cstdlib>
#include <mutex>
#include <vector>

namespace cuvs_amd {

std::string& last_error_text()
{
  thread_local std::string text;
  return text;
}

namespace {

void* raw_alloc(resources& res, size_t bytes, bool* failed)
{
  void* p = nullptr;
  hipError_t e = res.pool != nullptr ? hipMallocFromPoolAsync(&p, bytes, res.pool, res.stream)
                                     : hipMallocAsync(&p, bytes, res.stream);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    if (failed != nullptr) { *failed = true; return nullptr; }
    // pool exhausted or unsupported: fall back to a synchronous allocation
    HIP_TRY(hipStreamSynchronize(res.stream));
    HIP_TRY(hipMalloc(&p, bytes));
  }
  return p;
}

void raw_free(void* stream_v, void* p)
{
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  hipError_t e = hipFreeAsync(p, stream);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    (void)hipStreamSynchronize(stream);
    (void)hipFree(p);
  }
}

}  // namespace

unsigned long long g_pq3_last_stats[6] = {0, 0, 0, 0, 0, 0};  // cuvsAmdIvfPqLastFilterStats (written by ivf_pq_search.hip)

// scratch_cache.hpp: freed scratch blocks are kept by the handle and re-used by exact size on the same stream
// Kept blocks back to the runtime OUTSIDE a call (stream change, handle destruction, another thread's failed allocation): on the
// handle's own stream stream-ordered; on a stream the CALLER owns - which may already be destroyed (legal: the reference's setter
// never touches the old stream) - after ONE device-wide drain, synchronously (every flush site, one sync for all blocks)
static void flush_cache(scratch_cache& c)
{
  if (!c.caller_stream) { c.flush(raw_free); return; }
  bool drained = false;
  c.flush([&](void*, void* p) {
    if (!drained) { (void)hipDeviceSynchronize(); drained = true; }
    (void)hipFree(p);
    (void)hipGetLastError();
  });
}
void scratch_cache_flush(resources& res)
{
  if (res.cache != nullptr) flush_cache(*res.cache);
}

// every live cache of the process: a PERSISTENT allocation (an index buffer: plain hipMalloc, no handle in sight) that fails
// gives all kept scratch blocks back before it tries again
namespace {
std::mutex g_caches_mu;
std::vector<scratch_cache*> g_caches;
}  // namespace
void scratch_cache_register(scratch_cache* c, bool add)
{
  std::lock_guard<std::mutex> lk(g_caches_mu);
  if (add) g_caches.push_back(c);
  else g_caches.erase(std::remove(g_caches.begin(), g_caches.end(), c), g_caches.end());
}
void scratch_cache_flush_all()
{
  {
    std::lock_guard<std::mutex> lk(g_caches_mu);
    for (scratch_cache* c : g_caches) flush_cache(*c);
  }
  (void)hipDeviceSynchronize();  // the frees are stream-ordered: the memory is back once the streams have drained
  (void)hipGetLastError();
}

void ensure_aux_stream(resources& res)
{
  if (res.aux_stream != nullptr) return;
  int lo = 0, hi = 0;  // (numerically lower = higher priority)
  HIP_TRY(hipDeviceGetStreamPriorityRange(&lo, &hi));
  HIP_TRY(hipStreamCreateWithPriority(&res.aux_stream, hipStreamNonBlocking, hi));
  for (auto& ev : res.aux_events) HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
}

void* device_alloc(resources& res, size_t bytes)
{
  if (res.cache == nullptr) return raw_alloc(res, bytes, nullptr);
  return res.cache->alloc(
    res.stream, bytes, [&](size_t n, bool* failed) { return raw_alloc(res, n, failed); }, raw_free);
}

void device_free(resources& res, void* p)
{
  if (!p) return;
  if (res.cache == nullptr) raw_free(res.stream, p);
  else res.cache->release(res.stream, p, raw_free);
}

void fill_dl_view(DLManagedTensor* out, void* data, DLDataType dt, int64_t rows, int64_t cols,
                  int ndim, int device_id)
{
  CUVS_EXPECTS(out != nullptr, "output DLManagedTensor is null");
  out->dl_tensor.data        = data;
  out->dl_tensor.device      = DLDevice{kDLCUDA, device_id};  // what unmodified bindings expect
  out->dl_tensor.ndim        = ndim;
  out->dl_tensor.dtype       = dt;
  out->dl_tensor.shape       = new int64_t[2]{rows, cols};
  out->dl_tensor.strides     = nullptr;
  out->dl_tensor.byte_offset = 0;
  out->manager_ctx           = nullptr;
  out->deleter               = [](DLManagedTensor* self) {
    delete[] self->dl_tensor.shape;
    self->dl_tensor.shape = nullptr;
  };
}

static int g_log_level = CUVS_LOG_LEVEL_INFO;

// ---- per-kernel HIP-event timing (off unless enabled)
struct prof_rec {
  std::string name;
  hipEvent_t start, stop;
};
static bool g_prof_on = false;
static std::vector<prof_rec> g_prof;
static std::mutex g_prof_mu;

void profile_begin(resources& res, const char* name)
{
  if (!g_prof_on) return;
  std::lock_guard<std::mutex> lk(g_prof_mu);
  prof_rec r;
  r.name = name;
  HIP_TRY(hipEventCreate(&r.start));
  HIP_TRY(hipEventCreate(&r.stop));
  HIP_TRY(hipEventRecord(r.start, res.stream));
  g_prof.push_back(r);
}
void profile_end(resources& res, const char* name)
{
  if (!g_prof_on) return;
  std::lock_guard<std::mutex> lk(g_prof_mu);
  for (auto it = g_prof.rbegin(); it != g_prof.rend(); ++it)
    if (it->name == name) { HIP_TRY(hipEventRecord(it->stop, res.stream)); return; }
}

// ONE gate in front of every kernel-selection / ablation switch: without CUVS_AMD_DEBUG_SWITCHES=1 in the environment of the
// process that creates the handle, none of the CUVS_AMD_* variables below is even looked at - a caller of the drop-in
// library cannot change its behaviour by accident (tests/conftest.py and the bench / profiling scripts set the gate).
// A build with -DCUVS_AMD_NO_DEBUG_SWITCHES (make PRODUCTION=1) has no gate to open: the variables are never read. The default
// build keeps them - bench.py's own evidence (the LUT-scan comparator of `scan3_equals_lut_scan`, the filter's survivor counters)
// and the comparator tests need a second kernel selection inside one process; tests/conftest.py and bench.py set the gate only
// while they create such a comparator handle, every other handle runs the production configuration.
static bool debug_switches_on()
{
#ifdef CUVS_AMD_NO_DEBUG_SWITCHES
  return false;
#else
  const char* g = getenv("CUVS_AMD_DEBUG_SWITCHES");
  return g != nullptr && g[0] == '1';
#endif
}

tuning load_tuning_from_env()
{
  tuning t;
  if (!debug_switches_on()) return t;
  auto geti = [](const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; };
  auto set  = [](const char* name) { return getenv(name) != nullptr; };
  t.pq_head_probes   = geti("CUVS_AMD_PQ_HEAD_PROBES", -1);
  t.pq_scan2         = geti("CUVS_AMD_PQ_SCAN2", 1);
  t.pq_scan3         = geti("CUVS_AMD_PQ_SCAN3", 1);
  t.pq_filter4       = geti("CUVS_AMD_PQ_FILTER4", 1);
  t.coarse_grouped   = geti("CUVS_AMD_COARSE_GROUPED", 1);
  t.pq_overlap       = geti("CUVS_AMD_PQ_OVERLAP", 1);
  t.pq_unit_order    = geti("CUVS_AMD_PQ_UNIT_ORDER", t.pq_unit_order);
  t.pq_head_rows     = geti("CUVS_AMD_PQ_HEAD_ROWS", -1);
  t.coarse_lowp      = geti("CUVS_AMD_COARSE_LOWP", 1);
  t.flat_scan3       = geti("CUVS_AMD_FLAT_SCAN3", 1);
  t.flat_filter2     = geti("CUVS_AMD_FLAT_FILTER2", 1);
  t.flat_bound_head  = geti("CUVS_AMD_FLAT_BOUND_HEAD", 1);
  t.pq_wide          = geti("CUVS_AMD_PQ_WIDE", 1);
  t.pq_wide_heads    = geti("CUVS_AMD_PQ_WIDE_HEADS", 0);
  t.pq_wide_blocks   = geti("CUVS_AMD_PQ_WIDE_BLOCKS", 1);
  if (const char* e = getenv("CUVS_AMD_PQ_ENCODE")) t.pq_encode_plain = strcmp(e, "plain") == 0;
  t.pq3_surv_cap     = geti("CUVS_AMD_PQ3_SURV_CAP", 0);
  t.pq_qcap          = geti("CUVS_AMD_PQ_QCAP", 0);
  t.scan_debug       = geti("CUVS_AMD_SCAN_DEBUG", 0);
  t.alloc_cache      = geti("CUVS_AMD_ALLOC_CACHE", 1);
  t.shard_coarse_replicated = set("CUVS_AMD_SHARD_COARSE_REPLICATED");
  t.bf_fused           = set("CUVS_AMD_BF_FUSED");
  t.bf_no_threshold    = set("CUVS_AMD_BF_NO_THRESHOLD");
  t.bf_no_fused_filter = set("CUVS_AMD_BF_NO_FUSED_FILTER");
  t.bf_host_flags = set("CUVS_AMD_BF_HOST_FLAGS");
  t.dist_old           = set("CUVS_AMD_DIST_OLD");
  t.tile_dbg           = geti("CUVS_AMD_TILE_DBG", 0);
  t.flat_head_probes   = geti("CUVS_AMD_FLAT_HEAD_PROBES", -1);
  t.cagra_pq_lists     = geti("CUVS_AMD_CAGRA_PQ_LISTS", 0);
  t.cagra_pq_probes    = geti("CUVS_AMD_CAGRA_PQ_PROBES", 0);
  t.cagra_kpq          = geti("CUVS_AMD_CAGRA_KPQ", 0);
  t.cagra_rank_chunk   = geti("CUVS_AMD_CAGRA_RANK_CHUNK", 0);
  t.prune_dbg          = geti("CUVS_AMD_PRUNE_DBG", 0);
  if (const char* e = getenv("CUVS_AMD_CAGRA_AUTO")) t.cagra_auto_multi = e[0] == 'm';
  if (const char* e = getenv("CUVS_AMD_TIERED_PATH")) t.tiered_path = strcmp(e, "composed") == 0 ? 1 : (strcmp(e, "fused") == 0 ? 2 : 0);
  if (const char* e = getenv("CUVS_AMD_NATIVE_FORMAT")) t.native_format = e[0] == '1';
  t.hnsw_pack_rows   = geti("CUVS_AMD_HNSW_PACK_ROWS", 0);
  t.hnsw_pack_host   = geti("CUVS_AMD_HNSW_PACK_HOST", 0);
  t.eps_slab_rows    = geti("CUVS_AMD_EPS_SLAB_ROWS", 0);
  t.stats_slab_rows  = geti("CUVS_AMD_STATS_SLAB_ROWS", 0);
  return t;
}

}  // namespace cuvs_amd

using namespace cuvs_amd;

extern "C" {

const char* cuvsGetLastErrorText()
{
  auto& t = last_error_text();
  return t.empty() ? nullptr : t.c_str();
}

void cuvsSetLastErrorText(const char* error) { last_error_text() = error ? error : ""; }

cuvsLogLevel_t cuvsGetLogLevel() { return (cuvsLogLevel_t)g_log_level; }
void cuvsSetLogLevel(cuvsLogLevel_t l) { g_log_level = (int)l; }

cuvsError_t cuvsResourcesCreate(cuvsResources_t* res)
{
  return (cuvsError_t)translate_exceptions([=] {
    CUVS_EXPECTS(res != nullptr, "res is null");
    auto* r = new resources();
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    r->device = dev;
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, dev));
    r->num_cus       = prop.multiProcessorCount;
    r->lds_per_block = prop.sharedMemPerBlock;
    // A blocking stream, like the per-thread default stream behind the reference's handle: work issued on the legacy
    // default stream (a plain hipMemcpy of the results, as the reference's C examples do right after a search) is
    // ordered after the work queued here. A non-blocking stream would let such callers read results too early.
    HIP_TRY(hipStreamCreateWithFlags(&r->stream, hipStreamDefault));
    r->owns_stream = true;
    r->tune = load_tuning_from_env();
    // the scratch of one internal batch of an IVF search: at most a quarter of what is free on the device right now (a nearly
    // full or a smaller device splits the batch instead of failing with out-of-memory), never below 256 MiB
    {
      size_t free_b = 0, total_b = 0;
      if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b > 0)
        r->ivf_batch_limit = std::max<size_t>(size_t(256) << 20, std::min<size_t>(r->ivf_batch_limit, free_b / 4));
      else
        (void)hipGetLastError();
    }
    // test hook: shrink the temporary-tile budget so tiling/merge logic runs on small inputs
    // (the reference has max_row_tile_size/max_col_tile_size hooks, knn_brute_force.cuh:90-93)
    if (const char* ws = debug_switches_on() ? getenv("CUVS_AMD_WORKSPACE_MB") : nullptr) {
      long mb = atol(ws);
      if (mb > 0) r->workspace_limit = r->ivf_batch_limit = (size_t)mb << 20;
    }
    // Scratch buffers come from a pool of the handle's own that keeps freed blocks (search allocates the same
    // temporaries every batch). The device's default pool is left alone: raising ITS release threshold would keep
    // gigabytes cached away from every other user of hipMallocAsync in the process. Freed with the handle.
    hipMemPoolProps props{};
    props.allocType     = hipMemAllocationTypePinned;
    props.handleTypes   = hipMemHandleTypeNone;
    props.location.type = hipMemLocationTypeDevice;
    props.location.id   = dev;
    if (hipMemPoolCreate(&r->pool, &props) == hipSuccess) {
      uint64_t thresh = UINT64_MAX;
      (void)hipMemPoolSetAttribute(r->pool, hipMemPoolAttrReleaseThreshold, &thresh);
    } else {
      r->pool = nullptr;  // no private pools on this runtime: plain hipMallocAsync from the default pool
    }
    (void)hipGetLastError();
    if (r->tune.alloc_cache != 0) {
      r->cache         = new scratch_cache();
      scratch_cache_register(r->cache, true);
      r->cache->stream = r->stream;
      size_t free_b = 0, total_b = 0;
      if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); total_b = size_t(64) << 30; }
      r->cache->cap_bytes = std::min<size_t>(total_b / 8, size_t(16) << 30);
      if (const char* mb = debug_switches_on() ? getenv("CUVS_AMD_ALLOC_CACHE_MB") : nullptr) r->cache->cap_bytes = (size_t)std::max(0L, atol(mb)) << 20;
    }
    *res = reinterpret_cast<uintptr_t>(r);
  });
}

// Handles are created and destroyed by the threads that use them (benchmark.hpp:296-307: one copy of the handle per bench thread).
// Tearing down the runtime objects of several handles at once - pools that still give blocks back, streams, events - is
// serialised: tests/test_concurrent_search_gpu.py had three threads die inside this call (round 6).
static std::mutex g_handle_teardown_mu;

cuvsError_t cuvsResourcesDestroy(cuvsResources_t res)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto* r = as_res(res);
    (void)hipStreamSynchronize(r->stream);
    std::lock_guard<std::mutex> teardown(g_handle_teardown_mu);
    if (r->aux_stream != nullptr) {
      (void)hipStreamSynchronize(r->aux_stream);
      (void)hipStreamDestroy(r->aux_stream);
      for (auto& e : r->aux_events) if (e != nullptr) (void)hipEventDestroy(e);
    }
    if (r->cagra_work != nullptr) (void)hipFree(r->cagra_work);
    if (r->host_word != nullptr) (void)hipHostFree(r->host_word);
    if (r->cache != nullptr) {
      scratch_cache_flush(*r);
      (void)hipStreamSynchronize(r->stream);
      scratch_cache_register(r->cache, false);
      delete r->cache;
      r->cache = nullptr;
    }
    if (r->pool != nullptr) (void)hipMemPoolDestroy(r->pool);
    if (r->owns_stream && r->stream) (void)hipStreamDestroy(r->stream);
    delete r;
  });
}

cuvsError_t cuvsStreamSet(cuvsResources_t res, cudaStream_t stream)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto* r = as_res(res);
    if (r->cache != nullptr) {
      // kept blocks are ordered on the old stream: give them back before it goes. A stream the CALLER owns may already
      // be destroyed (legal: the reference's setter never touches the old stream), so nothing here may fail on it: the
      // kept blocks are then freed synchronously after a device-wide drain
      scratch_cache_flush(*r);  // (own stream: stream-ordered frees; caller's stream: one drain, then synchronous frees)
      if (r->owns_stream) HIP_TRY(hipStreamSynchronize(r->stream));
    }
    if (r->owns_stream && r->stream) {
      HIP_TRY(hipStreamSynchronize(r->stream));
      HIP_TRY(hipStreamDestroy(r->stream));
    }
    r->stream      = reinterpret_cast<hipStream_t>(stream);
    r->owns_stream = false;
    if (r->cache != nullptr) {
      std::lock_guard<std::mutex> lk(r->cache->mu);
      r->cache->stream        = r->stream;
      r->cache->caller_stream = true;
    }
  });
}

cuvsError_t cuvsStreamGet(cuvsResources_t res, cudaStream_t* stream)
{
  return (cuvsError_t)translate_exceptions([=] {
    CUVS_EXPECTS(stream != nullptr, "stream is null");
    *stream = reinterpret_cast<cudaStream_t>(as_res(res)->stream);
  });
}

cuvsError_t cuvsStreamSync(cuvsResources_t res)
{
  return (cuvsError_t)translate_exceptions([=] { sync(*as_res(res)); });
}

cuvsError_t cuvsDeviceIdGet(cuvsResources_t res, int* device_id)
{
  return (cuvsError_t)translate_exceptions([=] {
    CUVS_EXPECTS(device_id != nullptr, "device_id is null");
    *device_id = as_res(res)->device;
  });
}

// Single-process multi-GPU handle: records the participating devices. The sharded search path
// itself runs one process per GPU over RCCL (see cuvs_amd/mg.py); this handle exists so that
// bindings that create it keep working (reference: c_api.cpp:38-75).
cuvsError_t cuvsMultiGpuResourcesCreate(cuvsResources_t* res)
{
  cuvsError_t e = cuvsResourcesCreate(res);
  if (e != CUVS_SUCCESS) return e;
  return (cuvsError_t)translate_exceptions([=] {
    int n = 0;
    HIP_TRY(hipGetDeviceCount(&n));
    auto* r = as_res(*res);
    for (int i = 0; i < n; ++i) r->mg_devices.push_back(i);
  });
}

cuvsError_t cuvsMultiGpuResourcesCreateWithDeviceIds(cuvsResources_t* res, DLManagedTensor* device_ids)
{
  cuvsError_t e = cuvsResourcesCreate(res);
  if (e != CUVS_SUCCESS) return e;
  e = (cuvsError_t)translate_exceptions([=] {
    CUVS_EXPECTS(device_ids != nullptr, "device_ids is null");
    auto& t = device_ids->dl_tensor;
    CUVS_EXPECTS(dtype_is(t.dtype, kDLInt, 32) && t.ndim == 1 && is_host_accessible(t),
                 "device_ids must be a host int32 vector");
    auto* r   = as_res(*res);
    auto* ids = static_cast<const int32_t*>(dl_data(t));
    for (int64_t i = 0; i < t.shape[0]; ++i) r->mg_devices.push_back(ids[i]);
  });
  if (e != CUVS_SUCCESS) {  // do not leak the handle when validation fails (the error text is kept)
    const std::string msg = last_error_text();
    (void)cuvsResourcesDestroy(*res);
    *res = 0;
    last_error_text() = msg;
  }
  return e;
}

cuvsError_t cuvsMultiGpuResourcesDestroy(cuvsResources_t res) { return cuvsResourcesDestroy(res); }

cuvsError_t cuvsMultiGpuResourcesSetMemoryPool(cuvsResources_t res, int percent_of_free_memory)
{
  return (cuvsError_t)translate_exceptions([=] {
    (void)as_res(res);
    CUVS_EXPECTS(percent_of_free_memory >= 0 && percent_of_free_memory <= 100, "bad percentage");
  });
}

cuvsError_t cuvsRMMAlloc(cuvsResources_t res, void** ptr, size_t bytes)
{
  return (cuvsError_t)translate_exceptions([=] {
    CUVS_EXPECTS(ptr != nullptr, "ptr is null");
    *ptr = device_alloc(*as_res(res), bytes);
  });
}

cuvsError_t cuvsRMMFree(cuvsResources_t res, void* ptr, size_t)
{
  return (cuvsError_t)translate_exceptions([=] { device_free(*as_res(res), ptr); });
}

cuvsError_t cuvsRMMPoolMemoryResourceEnable(int initial_pool_size_percent, int max_pool_size_percent, bool)
{
  // The HIP stream-ordered pool is always on; record nothing, validate arguments.
  return (cuvsError_t)translate_exceptions([=] {
    CUVS_EXPECTS(initial_pool_size_percent >= 0 && max_pool_size_percent <= 100 &&
                   initial_pool_size_percent <= max_pool_size_percent,
                 "invalid pool percentages");
  });
}

cuvsError_t cuvsRMMMemoryResourceReset() { return CUVS_SUCCESS; }

cuvsError_t cuvsRMMHostAlloc(void** ptr, size_t bytes)
{
  return (cuvsError_t)translate_exceptions([=] {
    CUVS_EXPECTS(ptr != nullptr, "ptr is null");
    HIP_TRY(hipHostMalloc(ptr, bytes, hipHostMallocDefault));
  });
}

cuvsError_t cuvsRMMHostFree(void* ptr, size_t)
{
  return (cuvsError_t)translate_exceptions([=] { HIP_TRY(hipHostFree(ptr)); });
}

// extension (not in the reference ABI): counters of the last IVF-PQ search whose handle was created under
// CUVS_AMD_SCAN_DEBUG=1024 - [0] (row, query) pairs screened by the matrix-core filter, [1] survivors re-scored, [2] 32-row
// subtiles decoded, [3] work units (bench.py: survivors per pair of a corpus)
// 1: this build reads the CUVS_AMD_* switches behind the CUVS_AMD_DEBUG_SWITCHES=1 gate; 0: compiled out (make PRODUCTION=1)
__attribute__((visibility("default"))) int cuvsAmdDebugSwitchesCompiledIn(void)
{
#ifdef CUVS_AMD_NO_DEBUG_SWITCHES
  return 0;
#else
  return 1;
#endif
}
__attribute__((visibility("default"))) void cuvsAmdIvfPqLastFilterStats(unsigned long long* out)
{
  for (int i = 0; i < 4; ++i) out[i] = cuvs_amd::g_pq3_last_stats[i];
}
// the same six-fold: + [4] (query, probe) pairs handed back to the LUT scan kernels (queries the filter could not serve),
// [5] candidates that went through the shared overflow list (their query's pool was full)
__attribute__((visibility("default"))) void cuvsAmdIvfPqLastFilterStats6(unsigned long long* out)
{
  for (int i = 0; i < 6; ++i) out[i] = cuvs_amd::g_pq3_last_stats[i];
}
// extension (not in the reference ABI): kernel timing for bench.py
__attribute__((visibility("default"))) void cuvsAmdProfileEnable(int on) { g_prof_on = on != 0; }
// sums the elapsed ms of every recorded launch called `name`; returns the launch count; resets those records
__attribute__((visibility("default"))) int cuvsAmdProfileCollect(const char* name, double* total_ms)
{
  std::lock_guard<std::mutex> lk(g_prof_mu);
  int count = 0;
  double total = 0;
  std::vector<prof_rec> keep;
  for (auto& r : g_prof) {
    if (r.name == name) {
      if (hipEventSynchronize(r.stop) == hipSuccess) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, r.start, r.stop) == hipSuccess) { total += ms; ++count; }
      }
      (void)hipEventDestroy(r.start);
      (void)hipEventDestroy(r.stop);
    } else {
      keep.push_back(r);
    }
  }
  g_prof.swap(keep);
  if (total_ms) *total_ms = total;
  return count;
}

cuvsError_t cuvsVersionGet(uint16_t* major, uint16_t* minor, uint16_t* patch)
{
  return (cuvsError_t)translate_exceptions([=] {
    CUVS_EXPECTS(major && minor && patch, "null output");
    *major = CUVS_VERSION_MAJOR; *minor = CUVS_VERSION_MINOR; *patch = CUVS_VERSION_PATCH;  // reference VERSION 26.08.00
  });
}

cuvsError_t cuvsMatrixCopy(cuvsResources_t res, DLManagedTensor* src_m, DLManagedTensor* dst_m)
{
  return (cuvsError_t)translate_exceptions([=] {
    auto& r   = *as_res(res);
    auto& src = src_m->dl_tensor;
    auto& dst = dst_m->dl_tensor;
    CUVS_EXPECTS(src.ndim == 2 && dst.ndim == 2, "cuvsMatrixCopy: tensors must be 2-D");
    CUVS_EXPECTS(src.shape[0] == dst.shape[0] && src.shape[1] == dst.shape[1],
                 "cuvsMatrixCopy: shape mismatch");
    CUVS_EXPECTS(src.dtype.code == dst.dtype.code && src.dtype.bits == dst.dtype.bits,
                 "cuvsMatrixCopy: dtype mismatch");
    size_t esz     = (src.dtype.bits + 7) / 8;
    int64_t rows   = src.shape[0], cols = src.shape[1];
    int64_t s_ld   = src.strides ? src.strides[0] : cols;
    int64_t d_ld   = dst.strides ? dst.strides[0] : cols;
    CUVS_EXPECTS((!src.strides || src.strides[1] == 1) && (!dst.strides || dst.strides[1] == 1),
                 "cuvsMatrixCopy: inner stride must be 1");
    HIP_TRY(hipMemcpy2DAsync(dl_data(dst), d_ld * esz, dl_data(src), s_ld * esz, cols * esz, rows,
                             hipMemcpyDefault, r.stream));
  });
}

cuvsError_t cuvsMatrixSliceRows(cuvsResources_t res, DLManagedTensor* src_m, int64_t start, int64_t end,
                                DLManagedTensor* dst)
{
  return (cuvsError_t)translate_exceptions([=] {
    (void)as_res(res);
    auto& src = src_m->dl_tensor;
    CUVS_EXPECTS(src.ndim == 2, "cuvsMatrixSliceRows: tensor must be 2-D");
    CUVS_EXPECTS(start >= 0 && end >= start && end <= src.shape[0], "cuvsMatrixSliceRows: bad range");
    int64_t ld  = src.strides ? src.strides[0] : src.shape[1];
    size_t esz  = (src.dtype.bits + 7) / 8;
    dst->dl_tensor            = src;
    dst->dl_tensor.data       = static_cast<char*>(dl_data(src)) + start * ld * esz;
    dst->dl_tensor.byte_offset = 0;
    dst->dl_tensor.shape      = new int64_t[2]{end - start, src.shape[1]};
    dst->dl_tensor.strides    = new int64_t[2]{ld, 1};
    dst->manager_ctx          = nullptr;
    dst->deleter              = [](DLManagedTensor* self) {
      delete[] self->dl_tensor.shape;
      delete[] self->dl_tensor.strides;
    };
  });
}

}  // extern "C"
