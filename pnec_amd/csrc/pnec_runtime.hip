// pnec_runtime.hip -- process-wide state of the ABI layer: the per-thread error message, the device-memory cache, the
// stream / event pools and the refinement's pass counters (declared in pnec_internal.hpp).
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "pnec_internal.hpp"

namespace pnec_hip {

thread_local std::string g_last_error;

int fail(int code, const std::string &msg) {
  g_last_error = msg;
  return code;
}
int fail_hip(hipError_t e, const char *what) {
  return fail(PNEC_HIP_ERR_HIP_RUNTIME, std::string(what) + ": " + hipGetErrorString(e));
}

}  // namespace pnec_hip

using namespace pnec_hip;

namespace {

// ---- device memory with a small cache --------------------------------------------------------
// Batches come and go in pipelines (create -> select -> destroy every frame set, or one batch per frame
// when the odometry calls PNEC::Solve), and hipMalloc / hipFree cost tens of microseconds for a small
// buffer and up to hundreds of ms for GB-sized ones on some boxes.  Freed blocks are kept (per device, up
// to PNEC_HIP_CACHE_MB, default 16384, and kMaxCachedBlocks blocks) and handed out again to requests of
// [size/2, size] -- requests below 1 MiB are rounded up to a power of two (>= 4 KiB) so that the small
// arrays of same-shaped batches always match; pnec_hip_release_cache() returns them to the driver.  A
// block is only cached after the device has drained (what hipFree does implicitly), so a new owner never
// races an old kernel; a batch's destructor drains once for all of its blocks (dev_free_drained).
struct DevBlock {
  void *ptr;
  size_t bytes;
  int device;
};
constexpr size_t kRoundBelowBytes = 1u << 20;  // requests below this are rounded up to a power of two
constexpr size_t kMaxCachedBlocks = 4096;
std::mutex g_mem_mutex;
std::unordered_map<void *, DevBlock> g_live;  // every block handed out
std::vector<DevBlock> g_cache;               // free blocks kept for reuse
size_t g_cached_bytes = 0;
uint64_t g_n_hip_malloc = 0, g_n_cache_hit = 0;   // pnec_hip_alloc_counters

size_t cache_limit_bytes() {
  static const size_t limit = [] {
    const char *e = std::getenv("PNEC_HIP_CACHE_MB");
    return (size_t)(e && *e ? std::strtoull(e, nullptr, 10) : 16384ull) << 20;
  }();
  return limit;
}

void release_cache_locked(int device /* -1: all */) {
  for (size_t i = 0; i < g_cache.size();) {
    if (device < 0 || g_cache[i].device == device) {
      (void)hipFree(g_cache[i].ptr);
      g_cached_bytes -= g_cache[i].bytes;
      g_cache[i] = g_cache.back();
      g_cache.pop_back();
    } else {
      ++i;
    }
  }
}

}  // namespace

hipError_t pnec_hip::dev_alloc_bytes(void **out, size_t bytes) {
  *out = nullptr;
  if (bytes < kRoundBelowBytes) {
    size_t r = 4096;
    while (r < bytes) r <<= 1;
    bytes = r;
  }
  int device = 0;
  hipError_t e = hipGetDevice(&device);
  if (e != hipSuccess) return e;
  std::lock_guard<std::mutex> lock(g_mem_mutex);
  size_t best = g_cache.size();
  for (size_t i = 0; i < g_cache.size(); ++i)
    if (g_cache[i].device == device && g_cache[i].bytes >= bytes && g_cache[i].bytes <= 2 * bytes &&
        (best == g_cache.size() || g_cache[i].bytes < g_cache[best].bytes))
      best = i;
  DevBlock b{nullptr, bytes, device};
  if (best != g_cache.size()) {
    b = g_cache[best];
    g_cached_bytes -= b.bytes;
    g_cache[best] = g_cache.back();
    g_cache.pop_back();
    ++g_n_cache_hit;
  } else {
    ++g_n_hip_malloc;
    e = hipMalloc(&b.ptr, bytes);
    if (e != hipSuccess) {  // out of memory: give the cache back and try once more
      (void)hipGetLastError();
      release_cache_locked(device);
      e = hipMalloc(&b.ptr, bytes);
      if (e != hipSuccess) return e;
    }
  }
  g_live[b.ptr] = b;
  *out = b.ptr;
  return hipSuccess;
}

namespace {

// drained: the caller has synchronised the block's device since the last work that touched it
hipError_t dev_free_impl(void *ptr, bool drained) {
  if (!ptr) return hipSuccess;
  std::lock_guard<std::mutex> lock(g_mem_mutex);
  auto it = g_live.find(ptr);
  if (it == g_live.end()) return hipFree(ptr);
  const DevBlock b = it->second;
  g_live.erase(it);
  if (g_cache.size() < kMaxCachedBlocks && g_cached_bytes + b.bytes <= cache_limit_bytes()) {
    hipError_t e = hipSuccess;
    if (!drained) {
      int prev = -1;
      (void)hipGetDevice(&prev);
      (void)hipSetDevice(b.device);
      e = hipDeviceSynchronize();
      if (prev >= 0) (void)hipSetDevice(prev);
    }
    if (e == hipSuccess) {
      g_cache.push_back(b);
      g_cached_bytes += b.bytes;
      return hipSuccess;
    }
  }
  return hipFree(ptr);
}
// ---- side streams and events with a pool -----------------------------------------------------
// hipStreamCreate / hipStreamDestroy cost milliseconds on some boxes (measured: a batch per frame that forked one
// side stream spent 2.7 of its 3.1 ms creating and destroying it).  Streams and events a batch no longer needs
// go back to a per-device pool (the owner drains before it lets go, like the memory blocks) and are handed out
// again; pnec_hip_release_cache() destroys them.
struct PooledStream {
  hipStream_t st;
  int device;
};
struct PooledEvent {
  hipEvent_t ev;
  int device;
};
std::vector<PooledStream> g_stream_pool;
std::vector<PooledEvent> g_event_pool;
constexpr size_t kMaxPooledStreams = 64, kMaxPooledEvents = 256;

void release_stream_pool_locked(int device /* -1: all */) {
  for (size_t i = 0; i < g_stream_pool.size();) {
    if (device < 0 || g_stream_pool[i].device == device) {
      (void)hipStreamDestroy(g_stream_pool[i].st);
      g_stream_pool[i] = g_stream_pool.back();
      g_stream_pool.pop_back();
    } else {
      ++i;
    }
  }
  for (size_t i = 0; i < g_event_pool.size();) {
    if (device < 0 || g_event_pool[i].device == device) {
      (void)hipEventDestroy(g_event_pool[i].ev);
      g_event_pool[i] = g_event_pool.back();
      g_event_pool.pop_back();
    } else {
      ++i;
    }
  }
}

// the refinement's pass counters (PNEC_HIP_OPT_COUNT_PASSES): two 64-bit sums per device, allocated on first use
unsigned long long *g_solve_work[64] = {nullptr};

}  // namespace

namespace pnec_hip {

hipError_t dev_free(void *ptr) { return dev_free_impl(ptr, false); }
hipError_t dev_free_drained(void *ptr) { return dev_free_impl(ptr, true); }

hipError_t pool_stream_get(hipStream_t *out) {
  int device = 0;
  hipError_t e = hipGetDevice(&device);
  if (e != hipSuccess) return e;
  {
    std::lock_guard<std::mutex> lock(g_mem_mutex);
    for (size_t i = 0; i < g_stream_pool.size(); ++i)
      if (g_stream_pool[i].device == device) {
        *out = g_stream_pool[i].st;
        g_stream_pool[i] = g_stream_pool.back();
        g_stream_pool.pop_back();
        return hipSuccess;
      }
  }
  return hipStreamCreateWithFlags(out, hipStreamNonBlocking);
}
void pool_stream_put(hipStream_t st, int device) {
  if (!st) return;
  {
    std::lock_guard<std::mutex> lock(g_mem_mutex);
    if (g_stream_pool.size() < kMaxPooledStreams) {
      g_stream_pool.push_back({st, device});
      return;
    }
  }
  (void)hipStreamDestroy(st);
}
hipError_t pool_event_get(hipEvent_t *out) {
  int device = 0;
  hipError_t e = hipGetDevice(&device);
  if (e != hipSuccess) return e;
  {
    std::lock_guard<std::mutex> lock(g_mem_mutex);
    for (size_t i = 0; i < g_event_pool.size(); ++i)
      if (g_event_pool[i].device == device) {
        *out = g_event_pool[i].ev;
        g_event_pool[i] = g_event_pool.back();
        g_event_pool.pop_back();
        return hipSuccess;
      }
  }
  return hipEventCreateWithFlags(out, hipEventDisableTiming);
}
void pool_event_put(hipEvent_t ev, int device) {
  if (!ev) return;
  {
    std::lock_guard<std::mutex> lock(g_mem_mutex);
    if (g_event_pool.size() < kMaxPooledEvents) {
      g_event_pool.push_back({ev, device});
      return;
    }
  }
  (void)hipEventDestroy(ev);
}

int solve_work_buffer(int device, unsigned long long **out) {
  if (device < 0 || device >= 64) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "device index out of range");
  std::lock_guard<std::mutex> lock(g_mem_mutex);
  if (!g_solve_work[device]) {
    unsigned long long *w = nullptr;
    PNEC_HIP_TRY(hipMalloc(&w, 2 * sizeof(unsigned long long)));
    PNEC_HIP_TRY(hipMemset(w, 0, 2 * sizeof(unsigned long long)));
    g_solve_work[device] = w;
  }
  *out = g_solve_work[device];
  return 0;
}

}  // namespace pnec_hip

extern "C" {

const char *pnec_hip_last_error(void) { return g_last_error.c_str(); }

int pnec_hip_work_counters(int device, int reset, uint64_t *out16, int32_t *compiled_in) {
  if (!out16) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "out16 is NULL");
  DeviceGuard guard(device);
  if (!guard.ok) return fail(PNEC_HIP_ERR_HIP_RUNTIME, "hipSetDevice failed (no such device?)");
  unsigned long long c[16];
  int in = 0;
  PNEC_HIP_TRY(frontend_work_counters(reset, c, &in));
  for (int i = 0; i < 16; ++i) out16[i] = (uint64_t)c[i];
  if (compiled_in) *compiled_in = in;
  // [13], [14]: correspondence-passes the refinement executed in full / cost-only, for calls made with
  // PNEC_HIP_OPT_COUNT_PASSES set (any build)
  if (device >= 0 && device < 64 && g_solve_work[device]) {
    unsigned long long w[2] = {0, 0};
    PNEC_HIP_TRY(hipDeviceSynchronize());
    PNEC_HIP_TRY(hipMemcpy(w, g_solve_work[device], sizeof(w), hipMemcpyDeviceToHost));
    out16[13] = w[0];
    out16[14] = w[1];
    if (reset) PNEC_HIP_TRY(hipMemset(g_solve_work[device], 0, sizeof(w)));
  }
  return 0;
}

int pnec_hip_alloc_counters(uint64_t *out4) {
  if (!out4) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "out is NULL");
  std::lock_guard<std::mutex> lock(g_mem_mutex);
  out4[0] = g_n_hip_malloc;
  out4[1] = g_n_cache_hit;
  out4[2] = (uint64_t)g_live.size();
  out4[3] = (uint64_t)g_cached_bytes;
  return 0;
}

int64_t pnec_hip_release_cache(int device) {
  std::lock_guard<std::mutex> lock(g_mem_mutex);
  const size_t before = g_cached_bytes;
  release_cache_locked(device);
  release_stream_pool_locked(device);
  return (int64_t)(before - g_cached_bytes);
}

}  // extern "C"
