// pnec_internal.hpp -- what the translation units of the ABI layer share (host side; not part of the public ABI):
// the batch object, error reporting, the device-memory cache and the stream / event pools (pnec_runtime.hip), the
// helpers of the batch layer (pnec_capi.hip) the sub-APIs call, the staging of host-space calls, and the launchers
// the kernels' translation units define.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>
#include <optional>
#include <string>
#include <type_traits>
#include <vector>

#include "pnec_call_plan.hpp"
#include "pnec_hip.h"

// ------------------------------------------------------------------------------------------
// HBM layout of a batch ("problem"):
//   data:  for pair p, a block of NC planes, each `stride_p = round_up(count_p, 64)` doubles:
//          f1x f1y f1z | f2x f2y f2z | cov xx xy xz yy yz zz | cov_host xx .. zz (SYM)
//          block_offset[p] = first double of the block; padding entries are 0.
//   A wavefront reading plane c touches 64 consecutive doubles (512 B) per load: fully coalesced.
struct pnec_hip_problem {
  int device = 0;
  int mode = 0;
  int nc = 0;
  int64_t n_pairs = 0;
  int64_t n_corr = 0;
  int32_t n_max = 0;
  int64_t data_doubles = 0;
  // A batch made with pnec_hip_problem_create_capacity is re-shaped in place (pnec_hip_problem_reshape): room for
  // cap_pairs pairs / cap_doubles doubles of planes, the index arrays laid out for cap_pairs.  0 = the shape it
  // was created with is all it can hold.  layout_gen counts the shapes it has had (views cache by it).
  int64_t cap_pairs = 0, cap_doubles = 0;
  uint64_t layout_gen = 0, view_src_gen = ~0ull;
  std::vector<int64_t> block_offset_host;  // reshape: the block layout of the current shape
  std::vector<int64_t> meta_host;      // reshape: the index arrays as uploaded (alive until the copy has run)
  hipEvent_t meta_uploaded = nullptr;  // reshape: recorded behind the upload
  std::vector<int64_t> offsets;       // host copy, [n_pairs+1]
  double *d_data = nullptr;           // SoA payload
  int64_t *d_block_offset = nullptr;  // [n_pairs]
  int64_t *d_offsets = nullptr;       // [n_pairs+1] AoS offsets (ingest only)
  int32_t *d_count = nullptr;         // [n_pairs]
  void *d_meta = nullptr;             // pnec_hip_problem_create: ONE block holding the three arrays above (one upload)
  // staging for host-space solves (grown on demand, reused)
  double *d_stage = nullptr;
  int64_t stage_doubles = 0;
  int32_t *d_stage_i = nullptr;
  int64_t stage_ints = 0;
  // pnec_hip_relative_scale without out_ratio: the ratios between the pass and the selection (grown on demand, kept)
  double *d_ratio = nullptr;
  int64_t ratio_doubles = 0;
  // scratch of the front stages (sums, starts and results of the batched eigenvalue minimisation)
  double *d_front = nullptr;
  int32_t *d_front_i = nullptr;
  int64_t front_pairs = 0;
  // which iteration the eigenvalue minimisations of the stage calls run (pnec_hip_problem_set_eigensolver_scheme)
  int es_scheme = 0;
  int ransac_flags = 0;   // PNEC_HIP_RANSAC_*: what pnec_hip_ransac_eigensolver on this batch runs with
  // capacity-shaped batches (filled again and again): the host-space fill's AoS staging, kept and grown on demand
  double *d_fill = nullptr;
  int64_t fill_doubles = 0;
  // launch-order hint of the RANSAC stage (pnec_hip_problem_launch_order_hint): the last run's hypothesis counts and
  // the order made from them; order_pairs = the number of pairs d_order is a permutation of (0: none yet)
  bool order_hint = false;
  int32_t *d_hint_its = nullptr, *d_order = nullptr;
  int64_t hint_cap = 0, order_pairs = 0;
  // ragged batches: pairs grouped by the smallest launch geometry that holds them (built lazily)
  struct Bucket {
    int cpl, wpp, ldsk;
    bool resident;
    int64_t count;
    int64_t first;  // offset into d_bucket_pairs
  };
  std::vector<Bucket> buckets;
  int32_t *d_bucket_pairs = nullptr;
  // ragged batches: the launches of the geometries in use run side by side (fork / join around them), so that
  // the long tail of one (solves of up to 50 iterations) is filled by the others' wavefronts
  std::vector<hipStream_t> side_streams;
  std::vector<hipEvent_t> side_done;
  hipEvent_t fork_event = nullptr;
  std::vector<int32_t> host_counts;
  // A batch produced by InlierExtraction on the device (pnec_hip_problem_select, the pipeline): it keeps
  // the source's block layout (capacity) and its real pair sizes exist only in d_count until somebody
  // asks for host-side numbers.  While `lazy`, host_counts / n_max / n_corr / offsets hold the SOURCE's
  // values, i.e. upper bounds -- all the launch selection needs.
  // A capacity batch filled by pnec_hip_problem_fill_keypoints_ragged is lazy in the same way: its shape (the last
  // pnec_hip_problem_reshape) gives the bounds, the device-side offsets of the call the sizes.  bound_offsets keeps that
  // shape (empty: no such call since the last reshape) so that a call after materialize() finds the bounds again;
  // d_bound [cap_pairs] holds the bound per pair for the kernel, uploaded from bound_counts by the first call after a
  // reshape (bound_uploaded: recorded behind that copy).
  bool lazy = false;
  hipStream_t lazy_stream = nullptr;   // the stream the device-side sizes were produced on
  std::vector<int64_t> bound_offsets;
  std::vector<int32_t> bound_counts;
  int32_t *d_bound = nullptr;
  hipEvent_t bound_uploaded = nullptr;
  bool owns_data = true;               // false: a re-typed view of another batch's buffers (NEC view of a TARGET batch)
  pnec_hip_problem *sel_view = nullptr;  // pipeline: cached InlierExtraction target (same capacity, reused)
  pnec_hip_problem *nec_view = nullptr;  // pipeline: this batch's bearings as a NEC-family batch (no copy)
  // pipeline, large batches: contiguous ranges of the pairs as batches of their own (views: no data of their own,
  // index arrays = slices of this batch's), each with its scratch and its stream, and the same for the InlierExtraction
  // target -- the chain runs on them side by side (pnec_pipeline.hip)
  std::vector<pnec_hip_problem *> chunk_views, chunk_sel_views;
  std::vector<hipStream_t> chunk_streams;
  std::vector<hipEvent_t> chunk_done;
  uint8_t *d_mask = nullptr;             // pipeline: inlier mask [n_corr]
  int64_t mask_bytes = 0;
};

namespace pnec_hip {

struct SolveArgs;  // pnec_solve_kernel.hpp

// ---- errors (pnec_runtime.hip): the message pnec_hip_last_error returns, per thread --------
extern thread_local std::string g_last_error;
int fail(int code, const std::string &msg);
int fail_hip(hipError_t e, const char *what);
#define PNEC_HIP_TRY(expr)                                      \
  do {                                                          \
    hipError_t e_ = (expr);                                     \
    if (e_ != hipSuccess) return ::pnec_hip::fail_hip(e_, #expr); \
  } while (0)

// ---- device memory with a small cache, pooled streams and events (pnec_runtime.hip) --------
hipError_t dev_alloc_bytes(void **out, size_t bytes);
template <typename T>
inline hipError_t dev_alloc(T **out, size_t bytes) {
  void *ptr = nullptr;
  const hipError_t e = dev_alloc_bytes(&ptr, bytes);
  *out = static_cast<T *>(ptr);
  return e;
}
hipError_t dev_free(void *ptr);
// drained: the caller has synchronised the block's device since the last work that touched it
hipError_t dev_free_drained(void *ptr);
hipError_t pool_stream_get(hipStream_t *out);
void pool_stream_put(hipStream_t st, int device);
hipError_t pool_event_get(hipEvent_t *out);
void pool_event_put(hipEvent_t ev, int device);
// the refinement's pass counters (PNEC_HIP_OPT_COUNT_PASSES): two 64-bit sums per device, allocated on first use
int solve_work_buffer(int device, unsigned long long **out);

struct DeviceGuard {
  int prev = -1;
  bool ok = true;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    ok = (hipSetDevice(dev) == hipSuccess);
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

// ---- the batch layer's helpers the sub-APIs call (pnec_capi.hip) ---------------------------
struct Geometry {
  int cpl, wpp, ldsk;
  bool resident;
};
int geometry_ladder(int mode, const int (**order)[3], bool planes = true);
int ensure_stage(pnec_hip_problem *p, int64_t doubles, int64_t ints);
int ensure_side_streams(pnec_hip_problem *p, size_t n);
int ensure_order_hint(pnec_hip_problem *p);
int ensure_front(pnec_hip_problem *p);
int materialize(const pnec_hip_problem *cp);
int problem_reshape_impl(pnec_hip_problem *p, int64_t n_pairs, const int64_t *offsets, hipStream_t stream, bool upload);
int alloc_like(pnec_hip_problem *src, hipStream_t stream, pnec_hip_problem **out);
int select_prepare(pnec_hip_problem *src, hipStream_t stream, pnec_hip_problem *dst);
int select_finish(pnec_hip_problem *src, hipStream_t stream, pnec_hip_problem *dst, bool scan = true);

// ---- the arrays of one ABI call, in either memory space --------------------------------------
// An entry point names each array once -- in(), in_bytes(), out(), scratch() with the field of its argument struct, the
// caller's pointer and the length -- then commit()s, launches, and returns finish().
//   DEVICE space: the fields get the caller's pointers; nothing is allocated, copied or waited for (scratch() aside).
//   HOST space: commit() sizes the owner's d_stage / d_stage_i once from the list (CallPlan, pnec_call_plan.hpp), points
//   the fields into them and queues the uploads on the call's stream; finish() queues the copies back, in the order of
//   the out() calls, and waits for the stream.
// The staging buffers are the batch's, or, for a call without a batch (the image entry points), the call's own.  The
// object also makes the batch's (the given) device the current one for as long as it lives; that the given device
// could not be selected is commit()'s first error.
class CallArrays {
 public:
  CallArrays(pnec_hip_problem *owner, int space, hipStream_t stream)
      : guard_(owner->device), p_(owner), host_(space == PNEC_HIP_MEM_HOST), stream_(stream) {}
  CallArrays(int device, int space, hipStream_t stream)
      : guard_(device), host_(space == PNEC_HIP_MEM_HOST), stream_(stream) {
    own_.emplace();
    own_->device = device;
    p_ = &*own_;
  }
  ~CallArrays() {
    if (own_ && own_->d_stage) (void)dev_free(own_->d_stage);
    if (own_ && own_->d_stage_i) (void)dev_free(own_->d_stage_i);
  }
  CallArrays(const CallArrays &) = delete;
  CallArrays &operator=(const CallArrays &) = delete;

  bool host() const { return host_; }
  // n doubles, 64-bit or 32-bit integers; a NULL array gives nullptr and takes no room
  template <typename F, typename T>
  void in(F &field, const T *caller, int64_t n) {
    static_assert(sizeof(T) == 8 || sizeof(T) == 4, "doubles, int64_t or int32_t");
    if (!host_) field = caller;
    else note(field, caller, plan_.in(caller != nullptr, n, sizeof(T)));
  }
  // n bytes of anything (pixels)
  template <typename F>
  void in_bytes(F &field, const void *caller, int64_t n) {
    if (!host_) field = caller;
    else note(field, caller, plan_.in(caller != nullptr, n, 1));
  }
  // an output of n doubles, 64-bit or 32-bit integers or bytes; a NULL one gives nullptr unless kKeep; kPreload: the
  // caller's content travels up first, so that what the kernel leaves alone comes back as it was
  template <typename F, typename T>
  void out(F &field, T *caller, int64_t n, unsigned flags = 0) {
    static_assert(sizeof(T) == 8 || sizeof(T) == 4 || sizeof(T) == 1, "doubles, int64_t, int32_t or bytes");
    if (!host_) field = caller;
    else note(field, caller, plan_.out(caller != nullptr, n, sizeof(T), flags));
  }
  // n doubles or 32-bit integers the call's kernels use among themselves, in either space
  template <typename T>
  void scratch(T *&field, int64_t n) {
    static_assert(sizeof(T) == 8 || sizeof(T) == 4, "doubles or int32_t");
    note(field, nullptr, plan_.scratch(n, sizeof(T)));
  }
  int commit() {
    if (own_ && !guard_.ok) return fail(PNEC_HIP_ERR_HIP_RUNTIME, "hipSetDevice failed (no such device?)");
    if (slots_.empty()) return 0;
    if (int rc = ensure_stage(p_, plan_.doubles, plan_.ints)) return rc;
    for (size_t i = 0; i < slots_.size(); ++i) {
      const CallPlan::Entry &e = plan_.entries[i];
      Slot &s = slots_[i];
      if (e.room) s.dev = e.ints ? static_cast<void *>(p_->d_stage_i + e.offset) : static_cast<void *>(p_->d_stage + e.offset);
      std::memcpy(s.field, &s.dev, sizeof(void *));
      if (e.up && err_ == hipSuccess) err_ = hipMemcpyAsync(s.dev, s.caller, e.bytes, hipMemcpyHostToDevice, stream_);
    }
    return status();
  }
  int finish() {
    if (!host_) return 0;
    for (size_t i = 0; i < slots_.size(); ++i)
      if (plan_.entries[i].back && err_ == hipSuccess)
        err_ = hipMemcpyAsync(slots_[i].caller, slots_[i].dev, plan_.entries[i].bytes, hipMemcpyDeviceToHost, stream_);
    if (err_ == hipSuccess) err_ = hipStreamSynchronize(stream_);
    return status();
  }

 private:
  struct Slot {
    void *field;   // the pointer of the argument struct that commit() sets
    void *caller;
    void *dev;
  };
  // slots_[i] goes with plan_.entries[i]
  template <typename F>
  void note(F &field, const void *caller, const CallPlan::Entry &) {
    static_assert(std::is_pointer<F>::value, "a field is a pointer");
    slots_.push_back({&field, const_cast<void *>(caller), nullptr});
  }
  int status() const { return err_ == hipSuccess ? 0 : fail_hip(err_, "host staging copy"); }
  DeviceGuard guard_;
  std::optional<pnec_hip_problem> own_;  // a call without a batch: the holder of its staging buffers
  pnec_hip_problem *p_ = nullptr;
  bool host_;
  hipStream_t stream_;
  hipError_t err_ = hipSuccess;
  CallPlan plan_;
  std::vector<Slot> slots_;
};

// ---- launchers defined by the kernels' translation units ------------------------------------
// one translation unit per residual family (pnec_solve_<family>.hip)
hipError_t launch_solve_mode_0(int, int, int, bool, const SolveArgs &, hipStream_t);
hipError_t launch_solve_mode_1(int, int, int, bool, const SolveArgs &, hipStream_t);
hipError_t launch_solve_mode_2(int, int, int, bool, const SolveArgs &, hipStream_t);
hipError_t launch_solve_mode_3(int, int, int, bool, const SolveArgs &, hipStream_t);
// the multi-hypothesis form (pnec_solve_group_kernel.hpp): one block per (pair, group of hypotheses)
hipError_t launch_solve_group_mode_0(int, int, int, const SolveArgs &, hipStream_t);
hipError_t launch_solve_group_mode_1(int, int, int, const SolveArgs &, hipStream_t);
hipError_t launch_solve_group_mode_2(int, int, int, const SolveArgs &, hipStream_t);
hipError_t launch_solve_group_mode_3(int, int, int, const SolveArgs &, hipStream_t);

// pnec_stream_<family>.hip: the same kernels reading the reference's AoS arrays (streaming handle)
hipError_t launch_solve_aos_mode_0(int, int, int, const SolveArgs &, hipStream_t);
hipError_t launch_solve_aos_mode_1(int, int, int, const SolveArgs &, hipStream_t);
hipError_t launch_solve_aos_mode_2(int, int, int, const SolveArgs &, hipStream_t);
hipError_t launch_solve_aos_mode_3(int, int, int, const SolveArgs &, hipStream_t);

// pnec_frontend.hip
hipError_t launch_ransac_eigensolver(const double *, const int64_t *, const int64_t *, const int32_t *, int64_t,
                                     const double *, unsigned long long, unsigned long long, int, int, double, double *, double *,
                                     uint8_t *, int32_t *, int32_t *, double *, int32_t *, hipStream_t, hipStream_t,
                                     hipEvent_t, hipEvent_t, int, double *, const int64_t *, int32_t *, int64_t *, const int32_t *, int, int);
hipError_t launch_ransac_order(const int32_t *, int64_t, int32_t *, hipStream_t);
hipError_t frontend_work_counters(int, unsigned long long *, int *);
hipError_t launch_select(int, const double *, const int64_t *, const int64_t *, const int32_t *, const uint8_t *,
                         double *, const int64_t *, const int32_t *, int32_t *, int64_t *, int64_t, hipStream_t);
hipError_t launch_nec_eigensolver(const double *, const int64_t *, const int32_t *, int64_t, const double *,
                                  double *, double *, int32_t *, double *, int32_t *, hipStream_t, int);
hipError_t launch_weighted_eigensolver(int, const double *, const int64_t *, const int32_t *, int64_t, int,
                                       const double *, const double *, double, int, double *, double *,
                                       int32_t *, double *, int32_t *, hipStream_t, int);
hipError_t launch_frontend_selftest(double *, hipStream_t);

}  // namespace pnec_hip
