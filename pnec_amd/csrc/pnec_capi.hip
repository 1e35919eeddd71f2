// pnec_capi.hip -- the batch part of the C ABI declared in include/pnec_hip.h: batch storage in HBM, ingest, launch
// selection, the refinement and the stages in front of it, InlierExtraction.  (The kernels it launches live in
// pnec_batch_kernels.hip and the kernels' own units; the cache and the pools in pnec_runtime.hip.)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "pnec_batch_kernels.hpp"
#include "pnec_device.hpp"
#include "pnec_detect.hpp"
#include "pnec_front_shared.hpp"
#include "pnec_internal.hpp"
#include "pnec_keyframe.hpp"
#include "pnec_patch_cov.hpp"
#include "pnec_patch_store.hpp"
#include "pnec_patch_track.hpp"
#include "pnec_pose_cov.hpp"
#include "pnec_residuals.hpp"
#include "pnec_sensitivity.hpp"
#include "pnec_eight_point.hpp"
#include "pnec_essential_minimal.hpp"
#include "pnec_essential_ransac.hpp"
#include "pnec_undistort.hpp"
#include "pnec_trajectory.hpp"
#include "pnec_relative_scale.hpp"
#include "pnec_tracks.hpp"
#include "pnec_tracks_link.hpp"
#include "pnec_triangulate.hpp"
#include "pnec_solve_kernel.hpp"
#include "pnec_solve_group_kernel.hpp"

using namespace pnec_hip;

namespace {

// ---- launch geometry --------------------------------------------------------------------
bool geometry_exists(int mode, int cpl, int wpp, int ldsk) {
#define PNEC_GEOMETRY_MATCH(CPL, WPP, LDSK) \
  if (cpl == CPL && wpp == WPP && ldsk == LDSK) return geometry_ok(mode, cpl, wpp, ldsk);
  PNEC_FOR_EACH_GEOMETRY(PNEC_GEOMETRY_MATCH)
#undef PNEC_GEOMETRY_MATCH
  return false;
}

}  // namespace

namespace pnec_hip {

// The auto-tuner's ladder for a residual family (smallest capacity first).
// planes = true: the batch path, which reads the SoA planes in HBM and has the tail form (12, 1, 3) for pairs of
// 513..768 -- one wavefront, 512 correspondences resident, the tail re-read from L2 every pass -- whose results are
// bit for bit those of (8, 2, 3); the AoS-source kernels of the streaming handle (planes = false) are not built for it
// and run such pairs on (8, 2, 3), to the same bits.
int geometry_ladder(int mode, const int (**order)[3], bool planes) {
  static const int order12t[][3] = {{1, 1, 0}, {2, 1, 0}, {4, 1, 0}, {8, 1, 3}, {12, 1, 3},
                                    {8, 2, 3}, {8, 4, 3}, {8, 8, 3}};
  static const int order6t[][3] = {{1, 1, 0}, {2, 1, 0}, {4, 1, 0}, {8, 1, 0}, {12, 1, 3},
                                   {8, 2, 3}, {8, 4, 3}, {8, 8, 3}};
  if (planes && mode != PNEC_HIP_MODE_SYM) {
    *order = (mode == PNEC_HIP_MODE_NEC) ? order6t : order12t;
    return 8;
  }
  static const int order12[][3] = {{1, 1, 0}, {2, 1, 0}, {4, 1, 0}, {8, 1, 3},
                                   {8, 2, 3}, {8, 4, 3}, {8, 8, 3}};
  // 18-plane payload: 512 correspondences fit ONE wavefront at one wavefront per SIMD (288 payload
  // registers, AGPRs included) and that beats two wavefronts per solve: 19.0 vs 15.7 M solves/s
  static const int order18[][3] = {{1, 1, 0}, {2, 1, 0}, {4, 1, 0}, {8, 1, 0}, {4, 4, 0}, {4, 8, 0}};
  // 6-plane NEC payload: 8 correspondences per lane are 96 registers, so 512 fit one wavefront at two
  // per SIMD without the LDS slots: 41.7 vs 38.8 M solves/s
  static const int order6[][3] = {{1, 1, 0}, {2, 1, 0}, {4, 1, 0}, {8, 1, 0},
                                  {8, 2, 3}, {8, 4, 3}, {8, 8, 3}};
  if (mode == PNEC_HIP_MODE_SYM) { *order = order18; return 6; }
  *order = (mode == PNEC_HIP_MODE_NEC) ? order6 : order12;
  return 7;
}

}  // namespace pnec_hip

namespace {

// On-chip resident whenever the largest pair fits 64*CPL*WPP slots.  Preference: as few
// wavefronts per solve as possible (the serial part of an LM iteration is paid once per
// wavefront) at two wavefronts per SIMD; 12-plane payloads use the (8,W,3) family (5 of a
// lane's 8 correspondences in registers, 3 in LDS), the 18-plane SYM payload (8,1,0) up to 512
// correspondences and the (4,W,0) family beyond.
int choose_geometry(const pnec_hip_problem *p, const pnec_hip_options *opt, Geometry *g) {
  const int n = std::max<int32_t>(p->n_max, 1);
  if (opt && (opt->corr_per_lane > 0 || opt->waves_per_pair > 0)) {
    const int cpl = opt->corr_per_lane, wpp = opt->waves_per_pair ? opt->waves_per_pair : 1;
    const int ldsk = opt->lds_corr_per_lane;
    if (cpl < 0 || wpp < 0 || ldsk < 0) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "negative launch tuning");
    if (cpl == 0) {  // streaming with the fixed block shape
      *g = {1, kStreamWaves, 0, false};
      return 0;
    }
    if (!geometry_exists(p->mode, cpl, wpp, ldsk))
      return fail(PNEC_HIP_ERR_UNSUPPORTED,
                  "launch geometry (corr_per_lane, waves_per_pair, lds_corr_per_lane) not built");
    if ((int64_t)kWave * cpl * wpp < n)
      return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "launch geometry too small for the largest pair");
    *g = {cpl, wpp, ldsk, true};
    return 0;
  }
  const int (*order)[3];
  const int count = geometry_ladder(p->mode, &order);
  for (int i = 0; i < count; ++i) {
    if ((int64_t)kWave * order[i][0] * order[i][1] >= n) {
      *g = {order[i][0], order[i][1], order[i][2], true};
      return 0;
    }
  }
  *g = {1, kStreamWaves, 0, false};
  return 0;
}

// Ragged batches: one launch per geometry actually needed, each over the pairs that fit it, so a
// few large pairs do not force every small pair into a many-wavefront geometry.
int ensure_buckets(pnec_hip_problem *p) {
  if (!p->buckets.empty() || p->n_pairs == 0) return 0;
  const int (*order)[3];
  const int count = geometry_ladder(p->mode, &order);
  std::vector<std::vector<int32_t>> lists((size_t)count + 1);
  for (int64_t i = 0; i < p->n_pairs; ++i) {
    const int n = std::max<int32_t>(p->host_counts[(size_t)i], 1);
    int b = count;  // streaming
    for (int k = 0; k < count; ++k)
      if ((int64_t)kWave * order[k][0] * order[k][1] >= n) {
        b = k;
        break;
      }
    lists[(size_t)b].push_back((int32_t)i);
  }
  std::vector<int32_t> flat;
  std::vector<pnec_hip_problem::Bucket> buckets;
  flat.reserve((size_t)p->n_pairs);
  for (int b = 0; b <= count; ++b) {
    if (lists[(size_t)b].empty()) continue;
    pnec_hip_problem::Bucket bk;
    if (b < count) {
      bk = {order[b][0], order[b][1], order[b][2], true, (int64_t)lists[(size_t)b].size(), (int64_t)flat.size()};
    } else {
      bk = {1, kStreamWaves, 0, false, (int64_t)lists[(size_t)b].size(), (int64_t)flat.size()};
    }
    buckets.push_back(bk);
    flat.insert(flat.end(), lists[(size_t)b].begin(), lists[(size_t)b].end());
  }
  if (buckets.size() == 1) {  // one geometry serves every pair: the launch indexes pairs directly, no table
    p->buckets = std::move(buckets);
    return 0;
  }
  int32_t *d_pairs = nullptr;
  PNEC_HIP_TRY(dev_alloc(&d_pairs, sizeof(int32_t) * flat.size()));
  const hipError_t e = hipMemcpy(d_pairs, flat.data(), sizeof(int32_t) * flat.size(), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)dev_free(d_pairs);
    return fail_hip(e, "hipMemcpy(bucket pairs)");
  }
  // published only now: a failed attempt leaves the problem as it was (no buckets, no table)
  p->d_bucket_pairs = d_pairs;
  p->buckets = std::move(buckets);
  return 0;
}

}  // namespace

namespace pnec_hip {

int ensure_stage(pnec_hip_problem *p, int64_t doubles, int64_t ints) {
  if (doubles > p->stage_doubles) {
    if (p->d_stage) (void)dev_free(p->d_stage);
    p->d_stage = nullptr;
    p->stage_doubles = 0;
    PNEC_HIP_TRY(dev_alloc(&p->d_stage, sizeof(double) * doubles));
    p->stage_doubles = doubles;
  }
  if (ints > p->stage_ints) {
    if (p->d_stage_i) (void)dev_free(p->d_stage_i);
    p->d_stage_i = nullptr;
    p->stage_ints = 0;
    PNEC_HIP_TRY(dev_alloc(&p->d_stage_i, sizeof(int32_t) * ints));
    p->stage_ints = ints;
  }
  return 0;
}

// at least `n` side streams (+ their "done" events) and the fork event of the batch
int ensure_side_streams(pnec_hip_problem *p, size_t n) {
  while (p->side_streams.size() < n) {
    hipStream_t st = nullptr;
    hipEvent_t ev = nullptr;
    hipError_t e = pool_stream_get(&st);
    if (e == hipSuccess) e = pool_event_get(&ev);
    if (e != hipSuccess) {
      pool_stream_put(st, p->device);
      return fail_hip(e, "side stream");
    }
    p->side_streams.push_back(st);
    p->side_done.push_back(ev);
  }
  if (!p->fork_event) PNEC_HIP_TRY(pool_event_get(&p->fork_event));
  return 0;
}

// The launch-order hint's arrays (two int32 per pair), grown on demand.
int ensure_order_hint(pnec_hip_problem *p) {
  if (!p->order_hint || p->hint_cap >= p->n_pairs) return 0;
  if (p->d_hint_its) (void)dev_free(p->d_hint_its);
  if (p->d_order) (void)dev_free(p->d_order);
  p->d_hint_its = p->d_order = nullptr;
  p->hint_cap = p->order_pairs = 0;
  const int64_t want = std::max<int64_t>(p->n_pairs, p->cap_pairs);
  PNEC_HIP_TRY(dev_alloc(&p->d_hint_its, sizeof(int32_t) * (size_t)want));
  PNEC_HIP_TRY(dev_alloc(&p->d_order, sizeof(int32_t) * (size_t)want));
  p->hint_cap = want;
  return 0;
}

int ensure_front(pnec_hip_problem *p) {
  const int64_t P = std::max<int64_t>(p->n_pairs, 1);
  if (P > p->front_pairs) {
    if (p->d_front) (void)dev_free(p->d_front);
    if (p->d_front_i) (void)dev_free(p->d_front_i);
    p->d_front = nullptr;
    p->d_front_i = nullptr;
    p->front_pairs = 0;
    PNEC_HIP_TRY(dev_alloc(&p->d_front, sizeof(double) * (size_t)kFrontDoublesPerPair * P));
    PNEC_HIP_TRY(dev_alloc(&p->d_front_i, sizeof(int32_t) * ((size_t)kFrontIntsPerPair * P + kFrontCounterInts)));
    p->front_pairs = P;
  }
  return 0;
}

// Host-side sizes of a batch whose real pair sizes so far exist only on the device (a batch made by
// InlierExtraction): wait for the producing stream, fetch the counts, rebuild offsets / totals.
int materialize(const pnec_hip_problem *cp) {
  pnec_hip_problem *p = const_cast<pnec_hip_problem *>(cp);
  if (!p || !p->lazy) return 0;
  DeviceGuard guard(p->device);
  PNEC_HIP_TRY(hipStreamSynchronize(p->lazy_stream));
  if (p->n_pairs > 0)
    PNEC_HIP_TRY(hipMemcpy(p->host_counts.data(), p->d_count, sizeof(int32_t) * p->n_pairs, hipMemcpyDeviceToHost));
  p->n_max = 0;
  for (int64_t i = 0; i < p->n_pairs; ++i) {
    p->offsets[(size_t)i + 1] = p->offsets[(size_t)i] + p->host_counts[(size_t)i];
    p->n_max = std::max(p->n_max, p->host_counts[(size_t)i]);
  }
  p->n_corr = p->offsets[(size_t)p->n_pairs];
  p->lazy = false;
  // the geometry buckets were chosen from the source's sizes (upper bounds): rebuild them from the real ones
  p->buckets.clear();
  if (p->d_bucket_pairs) (void)dev_free(p->d_bucket_pairs);
  p->d_bucket_pairs = nullptr;
  return 0;
}

}  // namespace pnec_hip

namespace {

// the block layout of a shape: block_offset / count per pair, total doubles, the largest pair
int shape_layout(int nc, int64_t n_pairs, const int64_t *offsets, std::vector<int64_t> &block_offset,
                 std::vector<int32_t> &count, int64_t *total_out, int32_t *n_max_out) {
  if (n_pairs < 0 || !offsets) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "bad n_pairs/offsets");
  if (offsets[0] != 0) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "offsets[0] must be 0");
  block_offset.resize((size_t)n_pairs);
  count.resize((size_t)n_pairs);
  int64_t total = 0;
  int32_t n_max = 0;
  for (int64_t p = 0; p < n_pairs; ++p) {
    const int64_t n = offsets[p + 1] - offsets[p];
    if (n < 0 || n > (int64_t)1 << 30)
      return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "offsets must be non-decreasing (pair sizes < 2^30)");
    const int64_t stride = (n + kWave - 1) & ~(int64_t)(kWave - 1);
    block_offset[(size_t)p] = total;
    count[(size_t)p] = (int32_t)n;
    total += stride * nc;
    n_max = std::max<int32_t>(n_max, (int32_t)n);
  }
  *total_out = total;
  *n_max_out = n_max;
  return 0;
}

// block_offset [C] | offsets [C+1] | count [C] (C = the pair capacity) in one device block, filled by one copy (a
// batch per frame pays every blocking copy in full: three of them were a tenth of the one-pair PNEC::Solve)
int upload_meta(pnec_hip_problem *p, const std::vector<int64_t> &block_offset, const int64_t *offsets,
                const std::vector<int32_t> &count, hipStream_t stream, bool blocking) {
  const int64_t n_pairs = (int64_t)count.size();
  const size_t C1 = (size_t)std::max<int64_t>(std::max(p->cap_pairs, n_pairs), 1);
  const size_t words = C1 + (C1 + 1);  // int64 entries
  // an asynchronous upload reads this buffer when the stream gets there: it lives in the batch, and the next
  // upload waits for the previous one before it overwrites it
  if (p->meta_uploaded) PNEC_HIP_TRY(hipEventSynchronize(p->meta_uploaded));
  std::vector<int64_t> &meta = p->meta_host;
  meta.assign(words + (C1 + 1) / 2, 0);
  std::copy(block_offset.begin(), block_offset.end(), meta.begin());
  std::copy(offsets, offsets + n_pairs + 1, meta.begin() + (ptrdiff_t)C1);
  std::memcpy(meta.data() + words, count.data(), sizeof(int32_t) * count.size());
  if (!p->d_meta) {
    int64_t *d_meta = nullptr;
    hipError_t e = dev_alloc(&d_meta, sizeof(int64_t) * meta.size());
    if (e != hipSuccess) return fail_hip(e, "hipMalloc(meta)");
    p->d_meta = d_meta;
    p->d_block_offset = d_meta;
    p->d_offsets = d_meta + C1;
    p->d_count = reinterpret_cast<int32_t *>(d_meta + words);
  }
  // the used prefix of each array is what changes; for the small capacities of per-frame handles one copy
  // of the whole block is cheaper than three
  hipError_t e;
  if (blocking) {
    e = hipMemcpy(p->d_meta, meta.data(), sizeof(int64_t) * meta.size(), hipMemcpyHostToDevice);
  } else if (C1 <= 4096) {
    e = hipMemcpyAsync(p->d_meta, meta.data(), sizeof(int64_t) * meta.size(), hipMemcpyHostToDevice, stream);
  } else {
    e = hipMemcpyAsync(p->d_block_offset, meta.data(), sizeof(int64_t) * (size_t)std::max<int64_t>(n_pairs, 1),
                       hipMemcpyHostToDevice, stream);
    if (e == hipSuccess)
      e = hipMemcpyAsync(p->d_offsets, meta.data() + C1, sizeof(int64_t) * (size_t)(n_pairs + 1), hipMemcpyHostToDevice,
                         stream);
    if (e == hipSuccess)
      e = hipMemcpyAsync(p->d_count, meta.data() + words, sizeof(int32_t) * (size_t)std::max<int64_t>(n_pairs, 1),
                         hipMemcpyHostToDevice, stream);
  }
  if (e != hipSuccess) return fail_hip(e, "hipMemcpy(meta)");
  if (!blocking) {
    if (!p->meta_uploaded) PNEC_HIP_TRY(pool_event_get(&p->meta_uploaded));
    PNEC_HIP_TRY(hipEventRecord(p->meta_uploaded, stream));
  }
  return 0;
}

}  // namespace

namespace pnec_hip {

// upload = false: the caller's next kernel on the stream writes the device-side index arrays itself (the frame
// handle's ingest kernel does, for its single pair)
int problem_reshape_impl(pnec_hip_problem *p, int64_t n_pairs, const int64_t *offsets, hipStream_t stream,
                         bool upload) {
  if (!p) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "problem is NULL");
  // (d_meta: the index arrays in ONE block, which only pnec_hip_problem_create[_capacity] makes -- an InlierExtraction
  // target has capacity too, but its index arrays are separate allocations that upload_meta would leak and replace)
  if (p->cap_pairs <= 0 || !p->owns_data || !p->d_meta)
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "not a capacity-shaped batch (pnec_hip_problem_create_capacity)");
  std::vector<int64_t> block_offset;
  std::vector<int32_t> count;
  int64_t total = 0;
  int32_t n_max = 0;
  if (int rc = shape_layout(p->nc, n_pairs, offsets, block_offset, count, &total, &n_max)) return rc;
  if (n_pairs > p->cap_pairs || total > p->cap_doubles)
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "shape exceeds the batch's capacity");
  DeviceGuard guard(p->device);
  if (upload)
    if (int rc = upload_meta(p, block_offset, offsets, count, stream, /*blocking*/ false)) return rc;
  p->n_pairs = n_pairs;
  p->n_corr = offsets[n_pairs];
  p->n_max = n_max;
  p->host_counts = count;
  p->data_doubles = total;
  p->offsets.assign(offsets, offsets + n_pairs + 1);
  p->lazy = false;
  p->bound_offsets.clear();  // (an exact shape again: pnec_hip_problem_fill_keypoints_ragged takes its bounds from this one)
  p->buckets.clear();
  if (p->d_bucket_pairs) (void)dev_free(p->d_bucket_pairs);  // (drains: only ragged multi-geometry shapes have one)
  p->d_bucket_pairs = nullptr;
  // views cache the block layout by generation: a new one only when it really changed (the frame handle's single
  // pair always starts at 0, so its InlierExtraction target never re-copies anything)
  if (block_offset != p->block_offset_host) {
    p->block_offset_host = block_offset;
    ++p->layout_gen;
  }
  return 0;
}

// A batch with the capacity (block layout) of `src` and no contents yet: the target of InlierExtraction.
int alloc_like(pnec_hip_problem *src, hipStream_t stream, pnec_hip_problem **out) {
  *out = nullptr;
  pnec_hip_problem *d = new (std::nothrow) pnec_hip_problem();
  if (!d) return fail(PNEC_HIP_ERR_HIP_RUNTIME, "out of host memory");
  d->device = src->device;
  d->mode = src->mode;
  d->nc = src->nc;
  d->es_scheme = src->es_scheme;
  d->n_pairs = src->n_pairs;
  d->n_corr = src->n_corr;          // upper bounds until materialize()
  d->n_max = src->n_max;
  d->host_counts = src->host_counts;
  d->offsets = src->offsets;
  d->data_doubles = src->data_doubles;
  // as roomy as the source can ever get, so that a cached view survives the source's re-shaping
  d->cap_pairs = std::max(src->cap_pairs, src->n_pairs);
  d->cap_doubles = std::max(src->cap_doubles, src->data_doubles);
  const int64_t P = std::max<int64_t>(d->cap_pairs, 1);
  hipError_t e = dev_alloc(&d->d_data, sizeof(double) * (std::max<int64_t>(d->cap_doubles, 1) + kDataSlackDoubles));
  if (e == hipSuccess) e = dev_alloc(&d->d_block_offset, sizeof(int64_t) * P);
  if (e == hipSuccess) e = dev_alloc(&d->d_offsets, sizeof(int64_t) * (P + 1));
  if (e == hipSuccess) e = dev_alloc(&d->d_count, sizeof(int32_t) * P);
  if (e == hipSuccess && src->n_pairs > 0)
    e = hipMemcpyAsync(d->d_block_offset, src->d_block_offset, sizeof(int64_t) * src->n_pairs,
                       hipMemcpyDeviceToDevice, stream);
  d->view_src_gen = src->layout_gen;
  if (e != hipSuccess) {
    pnec_hip_problem_destroy(d);
    return fail_hip(e, "InlierExtraction target allocation");
  }
  *out = d;
  return 0;
}

// PNEC::InlierExtraction on the device, nothing read back: counts by ballot, offsets by a scan, the kept
// correspondences compacted pair by pair into dst (which has src's capacity).  All on `stream`.
// known_counts (optional, device): the inliers per pair when the producer of the mask counted them already (RANSAC
// does): the counting launch is skipped
// select_prepare: dst follows the source's current shape (block layout by generation); select_finish: the offsets of the
// kept correspondences + the host-side bookkeeping.  Between the two something fills dst's planes and counts: the copy
// kernel below (select_into), or the RANSAC stage itself (the chain: InlierExtraction fused into a pair's last pass).
int select_prepare(pnec_hip_problem *src, hipStream_t stream, pnec_hip_problem *dst) {
  const int64_t P = src->n_pairs;
  if (dst->view_src_gen != src->layout_gen) {  // the source has been re-shaped since dst copied its block layout
    if (P > 0)
      PNEC_HIP_TRY(hipMemcpyAsync(dst->d_block_offset, src->d_block_offset, sizeof(int64_t) * P, hipMemcpyDeviceToDevice,
                                  stream));
    dst->view_src_gen = src->layout_gen;
    dst->n_pairs = P;
    dst->data_doubles = src->data_doubles;
    dst->buckets.clear();
    if (dst->d_bucket_pairs) (void)dev_free(dst->d_bucket_pairs);
    dst->d_bucket_pairs = nullptr;
    dst->lazy = false;  // (so that select_finish re-installs the source's bounds)
    dst->offsets = src->offsets;
  }
  return 0;
}
int select_finish(pnec_hip_problem *src, hipStream_t stream, pnec_hip_problem *dst, bool scan) {
  const int64_t P = src->n_pairs;
  if (scan && P > 1) {
    const hipError_t e = launch_offsets_scan(dst->d_count, dst->d_offsets, P, stream);
    if (e != hipSuccess) return fail_hip(e, "offsets_scan_kernel");
  }
  if (!dst->lazy) {  // it had been given exact sizes: back to the source's bounds, buckets included
    dst->buckets.clear();
    if (dst->d_bucket_pairs) (void)dev_free(dst->d_bucket_pairs);
    dst->d_bucket_pairs = nullptr;
    dst->offsets = src->offsets;
  }
  dst->lazy = true;
  dst->lazy_stream = stream;
  dst->n_corr = src->n_corr;
  dst->n_max = src->n_max;
  dst->n_pairs = P;
  dst->data_doubles = src->data_doubles;  // (also when the block layout is unchanged but the pair's size is not)
  if (dst->host_counts != src->host_counts) {  // a re-shaped source: the launch geometries follow its new bounds
    dst->host_counts = src->host_counts;
    dst->offsets = src->offsets;
    dst->buckets.clear();
    if (dst->d_bucket_pairs) (void)dev_free(dst->d_bucket_pairs);
    dst->d_bucket_pairs = nullptr;
  }
  return 0;
}

}  // namespace pnec_hip

// ---- argument checks several entry points share; `name` is the entry point's, for the message ----------------------
namespace {

// prefix: "name: ", or "" where the entry point reports this one bare
int check_space(const std::string &prefix, int space) {
  if (space != PNEC_HIP_MEM_DEVICE && space != PNEC_HIP_MEM_HOST)
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, prefix + "bad memory space");
  return 0;
}

// the batch and the poses of a call that works on (pair, pose) slots
int check_pose_args(const char *name, const pnec_hip_problem *p, const double *q, const double *t, int32_t n_hyp) {
  const std::string pre = std::string(name) + ": ";
  if (!p) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "problem is NULL");
  if (!q || !t) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "q or t is NULL");
  if (n_hyp < 1) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "n_hyp must be >= 1");
  return 0;
}

// *S = the (pair, pose) slots of the call; 0: nothing to do.  what: "poses" / "solves"
int pose_slots(const pnec_hip_problem *p, int32_t n_hyp, const char *what, int64_t *S) {
  *S = p->n_pairs * (int64_t)n_hyp;
  if (*S > 0x7fffffffLL) return fail(PNEC_HIP_ERR_UNSUPPORTED, std::string("more than 2^31-1 ") + what + " in one call");
  return 0;
}

// (kernels that address a pair's planes with 32-bit byte offsets)
int check_planes_fit(const char *name, const pnec_hip_problem *b) {
  if ((int64_t)num_components(b->mode) * (((int64_t)b->n_max + kWave - 1) & ~(int64_t)(kWave - 1)) * 8 > 0xffffffffLL)
    return fail(PNEC_HIP_ERR_UNSUPPORTED, std::string(name) + ": a pair of 4 GiB of planes or more");
  return 0;
}

size_t pixel_bytes(int pixel_type) {
  switch (pixel_type) {
    case PNEC_HIP_PIXEL_U8: return 1;
    case PNEC_HIP_PIXEL_U16: return 2;
    case PNEC_HIP_PIXEL_F32: return 4;
    default: return 0;
  }
}

// n_images images of `rows` rows, `pitch` elements apart, as one block
int check_images_fit(const char *name, int64_t n_images, int64_t rows, int64_t pitch, size_t elem) {
  if (n_images > 0x7fffffffLL || (double)n_images * (double)rows * (double)pitch * (double)elem > 9.0e18)
    return fail(PNEC_HIP_ERR_UNSUPPORTED, std::string(name) + ": the images do not fit a 64-bit byte count");
  return 0;
}
// (its bytes: the last row of the last image need not be padded)
int64_t image_block_bytes(size_t elem, int64_t n_images, int64_t rows, int64_t pitch, int64_t width) {
  return (int64_t)elem * ((n_images * rows - 1) * pitch + width);
}

// HOST space only (the array is read): offsets[0 .. n] run from 0 to total without a step down
int check_offsets(const char *name, const char *array, const int64_t *offsets, int64_t n, int64_t total,
                  const char *total_name) {
  bool ok = offsets[0] == 0 && offsets[n] == total;
  for (int64_t f = 0; ok && f < n; ++f) ok = offsets[f] <= offsets[f + 1];
  if (!ok)
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT,
                std::string(name) + ": " + array + " must be non-decreasing from 0 to " + total_name);
  return 0;
}

}  // namespace

// ==========================================================================================
extern "C" {


int pnec_hip_abi_version(void) { return PNEC_HIP_ABI_VERSION; }

int pnec_hip_problem_launch_order_hint(pnec_hip_problem *p, int32_t enable) {
  if (!p) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "NULL problem");
  p->order_hint = enable != 0;
  if (!p->order_hint) p->order_pairs = 0;
  return 0;
}

int pnec_hip_device_count(int *count) {
  if (!count) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "count is NULL");
  *count = 0;
  PNEC_HIP_TRY(hipGetDeviceCount(count));
  return 0;
}

void pnec_hip_default_options(pnec_hip_options *o) {
  if (!o) return;
  std::memset(o, 0, sizeof(*o));
  o->max_num_iterations = 50;
  o->max_num_consecutive_invalid_steps = 5;
  o->jacobi_scaling = 1;
  o->check_convergence = 1;
  o->corr_per_lane = 0;
  o->waves_per_pair = 0;
  o->lds_corr_per_lane = 0;
  o->flags = 0;
  o->function_tolerance = 1e-6;
  o->gradient_tolerance = 1e-10;
  o->parameter_tolerance = 1e-8;
  o->initial_trust_region_radius = 1e4;
  o->max_trust_region_radius = 1e16;
  o->min_trust_region_radius = 1e-32;
  o->min_relative_decrease = 1e-3;
  o->min_lm_diagonal = 1e-6;
  o->max_lm_diagonal = 1e32;
}

static int problem_create_impl(int device, int mode, int64_t cap_pairs, int64_t cap_doubles, int64_t n_pairs,
                               const int64_t *offsets, pnec_hip_problem **out) {
  if (!out) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "out is NULL");
  *out = nullptr;
  if (mode < PNEC_HIP_MODE_NEC || mode > PNEC_HIP_MODE_SYM)
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "unknown mode");
  std::vector<int64_t> block_offset;
  std::vector<int32_t> count;
  const int nc = num_components(mode);
  int64_t total = 0;
  int32_t n_max = 0;
  if (int rc = shape_layout(nc, n_pairs, offsets, block_offset, count, &total, &n_max)) return rc;
  DeviceGuard guard(device);
  if (!guard.ok) return fail(PNEC_HIP_ERR_HIP_RUNTIME, "hipSetDevice failed (no such device?)");
  pnec_hip_problem *p = new (std::nothrow) pnec_hip_problem();
  if (!p) return fail(PNEC_HIP_ERR_HIP_RUNTIME, "out of host memory");
  p->device = device;
  p->mode = mode;
  p->nc = nc;
  p->n_pairs = n_pairs;
  p->n_corr = offsets[n_pairs];
  p->n_max = n_max;
  p->host_counts = count;
  p->data_doubles = total;
  p->cap_pairs = cap_pairs;
  p->cap_doubles = cap_doubles;
  p->offsets.assign(offsets, offsets + n_pairs + 1);
  hipError_t e;
  // (+ kDataSlackDoubles: the weighted stage's 16-byte table loads may read 512 bytes past the last pair's last plane)
  if ((e = dev_alloc(&p->d_data, sizeof(double) * (std::max<int64_t>(std::max(total, cap_doubles), 1) + kDataSlackDoubles))) != hipSuccess) {
    pnec_hip_problem_destroy(p);
    return fail_hip(e, "hipMalloc(data)");
  }
  if (int rc = upload_meta(p, block_offset, offsets, count, nullptr, /*blocking*/ true)) {
    const std::string msg = g_last_error;
    pnec_hip_problem_destroy(p);
    g_last_error = msg;
    return rc;
  }
  *out = p;
  return 0;
}

int pnec_hip_problem_create(int device, int mode, int64_t n_pairs, const int64_t *offsets,
                            pnec_hip_problem **out) {
  return problem_create_impl(device, mode, 0, 0, n_pairs, offsets, out);
}

int pnec_hip_problem_create_capacity(int device, int mode, int64_t max_pairs, int64_t max_corr,
                                     pnec_hip_problem **out) {
  if (!out) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "out is NULL");
  *out = nullptr;
  if (mode < PNEC_HIP_MODE_NEC || mode > PNEC_HIP_MODE_SYM) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "unknown mode");
  if (max_pairs < 1 || max_corr < 0 || max_corr > (int64_t)1 << 40)
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "need max_pairs >= 1, max_corr >= 0");
  // every pair's planes are padded to a multiple of 64 correspondences: at most 63 extra per pair
  const int64_t cap_doubles = (int64_t)num_components(mode) * ((max_corr + 63 * max_pairs + kWave - 1) & ~(int64_t)(kWave - 1));
  const int64_t zero = 0;
  return problem_create_impl(device, mode, max_pairs, cap_doubles, 0, &zero, out);
}

int pnec_hip_problem_reshape(pnec_hip_problem *p, int64_t n_pairs, const int64_t *offsets, void *stream_) {
  return problem_reshape_impl(p, n_pairs, offsets, (hipStream_t)stream_, true);
}

int pnec_hip_problem_destroy(pnec_hip_problem *p) {
  if (!p) return 0;
  DeviceGuard guard(p->device);
  // one drain for all of the batch's blocks (and its views'): nothing launched on them is still running
  // when they go back to the cache
  const bool drained = hipDeviceSynchronize() == hipSuccess;
  auto release = [&](void *ptr) { (void)(drained ? dev_free_drained(ptr) : dev_free(ptr)); };
  for (pnec_hip_problem *v : p->chunk_views) pnec_hip_problem_destroy(v);
  for (pnec_hip_problem *v : p->chunk_sel_views) pnec_hip_problem_destroy(v);
  if (p->sel_view) pnec_hip_problem_destroy(p->sel_view);
  if (p->nec_view) pnec_hip_problem_destroy(p->nec_view);
  release(p->d_mask);
  if (p->owns_data) {
    release(p->d_data);
    if (p->d_meta) {
      release(p->d_meta);
    } else {
      release(p->d_block_offset);
      release(p->d_offsets);
      release(p->d_count);
    }
  }
  release(p->d_stage);
  release(p->d_stage_i);
  release(p->d_ratio);
  release(p->d_front);
  release(p->d_front_i);
  release(p->d_hint_its);
  release(p->d_order);
  // (the device has drained: nothing is pending on these, so the next owner starts clean)
  for (hipStream_t st : p->side_streams) {
    if (drained) pool_stream_put(st, p->device); else (void)hipStreamDestroy(st);
  }
  for (hipEvent_t ev : p->side_done) {
    if (drained) pool_event_put(ev, p->device); else (void)hipEventDestroy(ev);
  }
  for (hipStream_t st : p->chunk_streams) {
    if (drained) pool_stream_put(st, p->device); else (void)hipStreamDestroy(st);
  }
  for (hipEvent_t ev : p->chunk_done) {
    if (drained) pool_event_put(ev, p->device); else (void)hipEventDestroy(ev);
  }
  if (p->fork_event) {
    if (drained) pool_event_put(p->fork_event, p->device); else (void)hipEventDestroy(p->fork_event);
  }
  if (p->meta_uploaded) {
    if (drained) pool_event_put(p->meta_uploaded, p->device); else (void)hipEventDestroy(p->meta_uploaded);
  }
  if (p->bound_uploaded) {
    if (drained) pool_event_put(p->bound_uploaded, p->device); else (void)hipEventDestroy(p->bound_uploaded);
  }
  release(p->d_bound);
  release(p->d_bucket_pairs);
  release(p->d_fill);
  delete p;
  return 0;
}

int pnec_hip_problem_fill(pnec_hip_problem *p, int64_t first_pair, int64_t n_pairs,
                          const double *bvs1, const double *bvs2, const double *covs,
                          const double *covs_host, int space, void *stream_) {
  if (!p) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "problem is NULL");
  if (first_pair < 0 || n_pairs < 0 || first_pair + n_pairs > p->n_pairs)
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "pair range out of bounds");
  if (n_pairs == 0) return 0;
  if (int rc = materialize(p)) return rc;
  const int64_t m = p->offsets[(size_t)(first_pair + n_pairs)] - p->offsets[(size_t)first_pair];
  if (m > 0 && (!bvs1 || !bvs2)) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "bvs1/bvs2 is NULL");
  if (m > 0 && p->nc >= 12 && !covs)
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "covs is NULL for a PNEC-mode problem");
  if (m > 0 && p->nc >= 18 && !covs_host)
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "covs_host is NULL for a SYM-mode problem");
  DeviceGuard guard(p->device);
  hipStream_t stream = (hipStream_t)stream_;

  const double *d_b1 = bvs1, *d_b2 = bvs2, *d_c = covs, *d_ch = covs_host;
  double *tmp = nullptr;
  bool persistent_stage = false;
  if (space == PNEC_HIP_MEM_HOST && m > 0) {
    const int64_t per = 6 + (p->nc >= 12 ? 9 : 0) + (p->nc >= 18 ? 9 : 0);
    // a batch that is re-filled keeps its staging (nothing allocated per call: the per-frame and streaming handles) --
    // up to 256 MB; beyond that the staging is ~1.25 x the payload (6 GB for 100k x 512) and is borrowed from the
    // library's buffer cache per call instead, so that it is shared by every batch on the device, not held by each
    if (p->cap_pairs > 0 && per * m * (int64_t)sizeof(double) <= (256ll << 20)) {
      if (per * m > p->fill_doubles) {
        if (p->d_fill) (void)dev_free(p->d_fill);
        p->d_fill = nullptr;
        p->fill_doubles = 0;
        PNEC_HIP_TRY(dev_alloc(&p->d_fill, sizeof(double) * per * m));
        p->fill_doubles = per * m;
      }
      persistent_stage = true;
      tmp = p->d_fill;
    } else {
      PNEC_HIP_TRY(dev_alloc(&tmp, sizeof(double) * per * m));
    }
    double *w = tmp;
    auto up = [&](const double *src, int64_t k, const double **dst) -> hipError_t {
      *dst = w;
      hipError_t e = hipMemcpyAsync(w, src, sizeof(double) * k * m, hipMemcpyHostToDevice, stream);
      w += k * m;
      return e;
    };
    hipError_t e = up(bvs1, 3, &d_b1);
    if (e == hipSuccess) e = up(bvs2, 3, &d_b2);
    if (e == hipSuccess && p->nc >= 12) e = up(covs, 9, &d_c);
    if (e == hipSuccess && p->nc >= 18) e = up(covs_host, 9, &d_ch);
    if (e != hipSuccess) {
      if (!persistent_stage) (void)dev_free(tmp);
      return fail_hip(e, "hipMemcpyAsync(H2D)");
    }
  } else if (space != PNEC_HIP_MEM_DEVICE && space != PNEC_HIP_MEM_HOST) {
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "bad memory space");
  }

  hipError_t e = launch_pack(p->nc, p->n_max, p->d_data, p->d_block_offset, p->d_offsets, p->d_count, first_pair, n_pairs,
                             d_b1, d_b2, d_c, d_ch, stream);
  if (tmp) {
    if (e == hipSuccess) e = hipStreamSynchronize(stream);   // (the caller may reuse its arrays; the staging may be refilled)
    if (!persistent_stage) (void)dev_free(tmp);
  }
  if (e != hipSuccess) return fail_hip(e, "pack_kernel");
  return 0;
}

int pnec_hip_problem_fill_keypoints(pnec_hip_problem *p, int64_t first_pair, int64_t n_pairs, const double *pts1,
                                    const double *pts2, const double *cov2, const double *cov1, const double *K_inv,
                                    double kappa, int camera_model, int space, void *stream_) {
  if (!p) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "problem is NULL");
  if (first_pair < 0 || n_pairs < 0 || first_pair + n_pairs > p->n_pairs)
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "pair range out of bounds");
  if (camera_model != 1)
    return fail(PNEC_HIP_ERR_UNSUPPORTED, "keypoint ingest is pinhole only (KeyPoint::Unproject, keypoints.cc:59-60)");
  if (space != PNEC_HIP_MEM_DEVICE && space != PNEC_HIP_MEM_HOST)
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "bad memory space");
  if (!K_inv) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "K_inv is NULL");
  if (n_pairs == 0) return 0;
  if (int rc = materialize(p)) return rc;
  const int64_t m = p->offsets[(size_t)(first_pair + n_pairs)] - p->offsets[(size_t)first_pair];
  if (m > 0 && (!pts1 || !pts2)) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "pts1/pts2 is NULL");
  if (m > 0 && p->nc >= 12 && !cov2) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "cov2 is NULL for a PNEC-mode problem");
  if (m > 0 && p->nc >= 18 && !cov1) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "cov1 is NULL for a SYM-mode problem");
  DeviceGuard guard(p->device);
  hipStream_t stream = (hipStream_t)stream_;
  const double *d_p1 = pts1, *d_p2 = pts2, *d_c2 = cov2, *d_c1 = cov1, *d_K = K_inv;
  double *tmp = nullptr;
  if (space == PNEC_HIP_MEM_HOST) {
    const int64_t per = 4 + (p->nc >= 12 ? 3 : 0) + (p->nc >= 18 ? 3 : 0);
    PNEC_HIP_TRY(dev_alloc(&tmp, sizeof(double) * (per * m + 9)));
    double *w = tmp;
    auto up = [&](const double *src, int64_t k, const double **dst) -> hipError_t {
      *dst = w;
      hipError_t e = k ? hipMemcpyAsync(w, src, sizeof(double) * k, hipMemcpyHostToDevice, stream) : hipSuccess;
      w += k;
      return e;
    };
    hipError_t e = up(K_inv, 9, &d_K);
    if (e == hipSuccess) e = up(pts1, 2 * m, &d_p1);
    if (e == hipSuccess) e = up(pts2, 2 * m, &d_p2);
    if (e == hipSuccess && p->nc >= 12) e = up(cov2, 3 * m, &d_c2);
    if (e == hipSuccess && p->nc >= 18) e = up(cov1, 3 * m, &d_c1);
    if (e != hipSuccess) {
      (void)dev_free(tmp);
      return fail_hip(e, "hipMemcpyAsync(H2D)");
    }
  }
  hipError_t e = launch_ingest_keypoints(p->nc, p->n_max, p->d_data, p->d_block_offset, p->d_offsets, p->d_count, first_pair,
                                         n_pairs, d_p1, d_p2, d_c2, d_c1, d_K, kappa, stream);
  if (tmp) {
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    (void)dev_free(tmp);
  }
  if (e != hipSuccess) return fail_hip(e, "ingest_keypoints_kernel");
  return 0;
}

int pnec_hip_problem_fill_keypoints_ragged(pnec_hip_problem *p, const int64_t *offsets, int64_t n_rows, const double *pts1,
                                           const double *pts2, const double *cov2, const double *cov1, const double *K_inv,
                                           double kappa, int camera_model, int32_t *out_dropped, int space, void *stream_) {
  const char *name = "pnec_hip_problem_fill_keypoints_ragged";
  const std::string pre = std::string(name) + ": ";
  if (!p) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "problem is NULL");
  if (p->cap_pairs <= 0 || !p->owns_data || !p->d_meta)
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "not a capacity-shaped batch (pnec_hip_problem_create_capacity)");
  if (camera_model != 1)
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "keypoint ingest is pinhole only: camera_model must be 1");
  if (int rc = check_space(pre, space)) return rc;
  if (!offsets || !K_inv) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "offsets or K_inv is NULL");
  if (n_rows < 0 || n_rows > 0x7fffffffLL) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "n_rows must be 0 .. 2^31-1");
  if (n_rows > 0 && (!pts1 || !pts2)) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "pts1/pts2 is NULL");
  // (whether a covariance array belongs does not depend on the rows offered: the sizes are the device's)
  if ((p->nc >= 12) != (cov2 != nullptr))
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "cov2 goes with TARGET, HOST and SYM batches and with no other");
  if ((p->nc >= 18) != (cov1 != nullptr))
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "cov1 goes with SYM batches and with no other");
  const int64_t P = p->n_pairs;
  if (P == 0) return 0;
  if (space == PNEC_HIP_MEM_HOST) {
    bool ok = offsets[0] >= 0 && offsets[P] <= n_rows;
    for (int64_t k = 0; ok && k < P; ++k) ok = offsets[k] <= offsets[k + 1];
    if (!ok) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "offsets must be non-decreasing within 0 .. n_rows");
  }
  hipStream_t stream = (hipStream_t)stream_;
  struct {
    const int64_t *offsets;
    const double *pts1, *pts2, *cov2, *cov1, *K_inv;
    int32_t *dropped;
  } d;
  CallArrays io(p, space, stream);
  io.in(d.offsets, offsets, P + 1);
  io.in(d.pts1, pts1, 2 * n_rows);
  io.in(d.pts2, pts2, 2 * n_rows);
  io.in(d.cov2, cov2, 3 * n_rows);
  io.in(d.cov1, cov1, 3 * n_rows);
  io.in(d.K_inv, K_inv, 9);
  io.out(d.dropped, out_dropped, P);
  // ---- the bounds: the shape pnec_hip_problem_reshape gave, on the host and (first call since) on the device
  if (p->bound_offsets.empty()) {
    if (!p->d_bound) PNEC_HIP_TRY(dev_alloc(&p->d_bound, sizeof(int32_t) * (size_t)p->cap_pairs));
    if (p->bound_uploaded) PNEC_HIP_TRY(hipEventSynchronize(p->bound_uploaded));  // (the last upload has read bound_counts)
    else PNEC_HIP_TRY(pool_event_get(&p->bound_uploaded));
    p->bound_counts = p->host_counts;
    PNEC_HIP_TRY(hipMemcpyAsync(p->d_bound, p->bound_counts.data(), sizeof(int32_t) * (size_t)P, hipMemcpyHostToDevice, stream));
    PNEC_HIP_TRY(hipEventRecord(p->bound_uploaded, stream));
    p->bound_offsets = p->offsets;
  } else if (!p->lazy) {  // somebody asked for host-side sizes (materialize): back to the bounds, buckets included
    p->offsets = p->bound_offsets;
    p->host_counts = p->bound_counts;
    p->n_corr = p->offsets[(size_t)P];
    p->n_max = 0;
    for (int32_t c : p->host_counts) p->n_max = std::max(p->n_max, c);
    p->buckets.clear();
    if (p->d_bucket_pairs) (void)dev_free(p->d_bucket_pairs);
    p->d_bucket_pairs = nullptr;
  }
  if (int rc = io.commit()) return rc;
  hipError_t e = launch_ingest_keypoints_ragged(p->nc, p->n_max, p->d_data, p->d_block_offset, d.offsets, p->d_bound, p->d_count,
                                                d.dropped, P, n_rows, d.pts1, d.pts2, d.cov2, d.cov1, d.K_inv, kappa, stream);
  if (e != hipSuccess) return fail_hip(e, "ingest_keypoints_ragged_kernel");
  // the batch's own offsets: those of the rows kept
  e = launch_offsets_scan(p->d_count, p->d_offsets, P, stream);
  if (e != hipSuccess) return fail_hip(e, "offsets_scan_kernel");
  p->lazy = true;
  p->lazy_stream = stream;
  return io.finish();
}

// keypoint undistortion, the step before the two ingests above: pnec_undistort.hip.  No batch: HOST space stages in
// buffers that live for the call only.
int pnec_hip_undistort_keypoints(int device, int64_t n_rows, const double *pts1, const double *pts2, const double *cov2,
                                 const double *cov1, const double *camera, int32_t fixed_iterations,
                                 int32_t newton_iterations, uint32_t flags, double *out_pts1, double *out_pts2,
                                 double *out_cov2, double *out_cov1, uint8_t *out_status1, uint8_t *out_status2, int space,
                                 void *stream_) {
  const std::string pre = "undistort_keypoints: ";
  const bool newton = (flags & PNEC_HIP_UNDISTORT_NEWTON) != 0;
  if (flags & ~(PNEC_HIP_UNDISTORT_NEWTON | PNEC_HIP_UNDISTORT_PROPAGATE_COV))
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "unknown bit in flags");
  if (fixed_iterations < 0 || fixed_iterations > 64)
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "fixed_iterations must be 0 .. 64");
  if (newton && (newton_iterations < 0 || newton_iterations > 64))
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "newton_iterations must be 0 .. 64");
  if (n_rows < 0 || n_rows > 0x7fffffffLL) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "n_rows must be 0 .. 2^31-1");
  if (!camera) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "camera is NULL");
  if (int rc = check_space(pre, space)) return rc;
  if (n_rows == 0) return 0;   // (an array of no rows says nothing: a caller's empty array may have no address)
  if ((pts1 != nullptr) != (out_pts1 != nullptr) || (pts2 != nullptr) != (out_pts2 != nullptr) ||
      (cov2 != nullptr) != (out_cov2 != nullptr) || (cov1 != nullptr) != (out_cov1 != nullptr))
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "an input and its output are given or NULL together");
  if ((out_status1 && !pts1) || (out_status2 && !pts2))
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "a status array without its points");
  if ((cov1 && !pts1) || (cov2 && !pts2)) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "a covariance without its points");
  if (!pts1 && !pts2) return 0;
  hipStream_t stream = (hipStream_t)stream_;
  CallArrays io(device, space, stream);
  UndistortArgs a{};
  a.n_rows = n_rows;
  a.fixed_iterations = fixed_iterations;
  a.newton_iterations = newton ? newton_iterations : 0;
  a.flags = flags;
  io.in(a.pts[0], pts1, 2 * n_rows);
  io.in(a.pts[1], pts2, 2 * n_rows);
  io.in(a.cov[1], cov2, 3 * n_rows);
  io.in(a.cov[0], cov1, 3 * n_rows);
  io.in(a.camera, camera, 9);
  io.out(a.out_pts[0], out_pts1, 2 * n_rows);
  io.out(a.out_pts[1], out_pts2, 2 * n_rows);
  io.out(a.out_cov[1], out_cov2, 3 * n_rows);
  io.out(a.out_cov[0], out_cov1, 3 * n_rows);
  io.out(a.out_status[0], out_status1, n_rows);
  io.out(a.out_status[1], out_status2, n_rows);
  if (int rc = io.commit()) return rc;
  PNEC_HIP_TRY(launch_undistort_keypoints(a, stream));
  return io.finish();
}

// trajectory evaluation: pnec_trajectory.hip.  No batch: HOST space stages in buffers that live for the call only.
namespace {
int check_trajectory_shape(const std::string &pre, int64_t n_seq, const int64_t *offsets, int64_t n_rows, int space) {
  if (n_seq < 1 || n_seq > 0x7fffffffLL) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "n_seq must be 1 .. 2^31-1");
  if (n_rows < 0 || n_rows > 0x7fffffffLL) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "n_rows must be 0 .. 2^31-1");
  if (!offsets) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "offsets is NULL");
  if (int rc = check_space(pre, space)) return rc;
  if (space == PNEC_HIP_MEM_HOST) {
    bool ok = offsets[0] == 0 && offsets[n_seq] <= n_rows;
    for (int64_t f = 0; ok && f < n_seq; ++f) ok = offsets[f] <= offsets[f + 1];
    if (!ok) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "offsets must be non-decreasing from 0 within n_rows");
  }
  return 0;
}
// an output that is also an input, or given twice
bool trajectory_alias(std::initializer_list<const void *> outs, std::initializer_list<const void *> ins) {
  for (const void *const *o = outs.begin(); o != outs.end(); ++o) {
    if (!*o) continue;
    for (const void *i : ins)
      if (*o == i) return true;
    for (const void *const *other = outs.begin(); other != o; ++other)
      if (*o == *other) return true;
  }
  return false;
}
}  // namespace

int pnec_hip_trajectory_compose(int device, int64_t n_seq, const int64_t *offsets, int64_t n_rows, const double *rel_q,
                                const double *rel_t, const double *scale, const double *q0, const double *p0,
                                double *out_q, double *out_p, uint8_t *out_valid, int space, void *stream_) {
  const std::string pre = "trajectory_compose: ";
  if (int rc = check_trajectory_shape(pre, n_seq, offsets, n_rows, space)) return rc;
  if ((scale || p0) && !rel_t) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "scale and p0 need rel_t");
  if ((rel_t != nullptr) != (out_p != nullptr))
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "out_p is given exactly when rel_t is");
  if (n_rows > 0 && (!rel_q || !out_q)) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "rel_q or out_q is NULL");
  if (trajectory_alias({out_q, out_p, out_valid}, {offsets, rel_q, rel_t, scale, q0, p0}))
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "an output is also an input or another output");
  if (n_rows == 0) return 0;
  hipStream_t stream = (hipStream_t)stream_;
  CallArrays io(device, space, stream);
  TrajectoryComposeArgs a{};
  a.n_seq = n_seq;
  a.n_rows = n_rows;
  io.in(a.offsets, offsets, n_seq + 1);
  io.in(a.rel_q, rel_q, 4 * n_rows);
  io.in(a.rel_t, rel_t, 3 * n_rows);
  io.in(a.scale, scale, n_rows);
  io.in(a.q0, q0, 4 * n_seq);
  io.in(a.p0, p0, 3 * n_seq);
  // (HOST space: rows of no sequence are not written, so the caller's content travels up first)
  io.out(a.out_q, out_q, 4 * n_rows, kPreload);
  io.out(a.out_p, out_p, 3 * n_rows, kPreload);
  io.out(a.out_valid, out_valid, n_rows, kPreload);
  if (int rc = io.commit()) return rc;
  PNEC_HIP_TRY(launch_trajectory_compose(a, stream));
  return io.finish();
}

int pnec_hip_trajectory_metrics(int device, int64_t n_seq, const int64_t *offsets, int64_t n_rows, const double *est_q,
                                const double *gt_q, const double *est_p, const double *gt_p, double *out_metrics,
                                double *out_err_q, double *out_rmse_d, double *out_l1_d, double *out_angle1,
                                double *out_rt1, int space, void *stream_) {
  const std::string pre = "trajectory_metrics: ";
  if (int rc = check_trajectory_shape(pre, n_seq, offsets, n_rows, space)) return rc;
  if (!out_metrics) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "out_metrics is NULL");
  if (n_rows > 0 && (!est_q || !gt_q || !out_err_q || !out_rmse_d || !out_l1_d))
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "est_q, gt_q, out_err_q, out_rmse_d or out_l1_d is NULL");
  if ((est_p != nullptr) != (gt_p != nullptr))
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "est_p and gt_p are given or NULL together");
  if (out_rt1 && !est_p) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "out_rt1 needs the positions");
  if (trajectory_alias({out_metrics, out_err_q, out_rmse_d, out_l1_d, out_angle1, out_rt1},
                       {offsets, est_q, gt_q, est_p, gt_p}))
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "an output is also an input or another output");
  hipStream_t stream = (hipStream_t)stream_;
  CallArrays io(device, space, stream);
  TrajectoryMetricsArgs a{};
  a.n_seq = n_seq;
  a.n_rows = n_rows;
  io.in(a.offsets, offsets, n_seq + 1);
  io.in(a.est_q, est_q, 4 * n_rows);
  io.in(a.gt_q, gt_q, 4 * n_rows);
  io.in(a.est_p, est_p, 3 * n_rows);
  io.in(a.gt_p, gt_p, 3 * n_rows);
  io.out(a.out_metrics, out_metrics, 5 * n_seq);
  io.out(a.out_err_q, out_err_q, 4 * n_rows);
  io.out(a.out_rmse_d, out_rmse_d, n_rows, kPreload);
  io.out(a.out_l1_d, out_l1_d, n_rows, kPreload);
  io.out(a.out_angle1, out_angle1, n_rows, kPreload);
  io.out(a.out_rt1, out_rt1, n_rows, kPreload);
  if (int rc = io.commit()) return rc;
  PNEC_HIP_TRY(launch_trajectory_metrics(a, stream));
  return io.finish();
}

int pnec_hip_trajectory_advance(int device, int64_t n_seq, const double *rel_q, const double *rel_t, const int32_t *count,
                                int32_t min_count, const double *scale3, const int32_t *n_used, int32_t min_used,
                                const double *s, const double *q, const double *p, double *next_s, double *next_q,
                                double *next_p, int32_t *out_status, int space, void *stream_) {
  const std::string pre = "trajectory_advance: ";
  if (n_seq < 1 || n_seq > 0x7fffffffLL) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "n_seq must be 1 .. 2^31-1");
  if (!rel_q || !rel_t) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "rel_q or rel_t is NULL");
  if (!s || !q || !p || !next_s || !next_q || !next_p)
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "a state array (s, q, p, next_s, next_q, next_p) is NULL");
  if (min_count < 0 || min_used < 1) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "min_count must be >= 0, min_used >= 1");
  if (n_used && !scale3) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "n_used needs scale3");
  if (trajectory_alias({next_s, next_q, next_p, out_status}, {rel_q, rel_t, count, scale3, n_used, s, q, p}))
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "an output is also an input or another output (the state is double-buffered)");
  if (int rc = check_space(pre, space)) return rc;
  hipStream_t stream = (hipStream_t)stream_;
  CallArrays io(device, space, stream);
  TrajectoryAdvanceArgs a{};
  a.n_seq = n_seq;
  a.min_count = min_count;
  a.min_used = min_used;
  io.in(a.rel_q, rel_q, 4 * n_seq);
  io.in(a.rel_t, rel_t, 3 * n_seq);
  io.in(a.count, count, n_seq);
  io.in(a.scale3, scale3, 3 * n_seq);
  io.in(a.n_used, n_used, n_seq);
  io.in(a.s, s, n_seq);
  io.in(a.q, q, 4 * n_seq);
  io.in(a.p, p, 3 * n_seq);
  io.out(a.next_s, next_s, n_seq);
  io.out(a.next_q, next_q, 4 * n_seq);
  io.out(a.next_p, next_p, 3 * n_seq);
  io.out(a.out_status, out_status, n_seq);
  if (int rc = io.commit()) return rc;
  PNEC_HIP_TRY(launch_trajectory_advance(a, stream));
  return io.finish();
}

int64_t pnec_hip_problem_payload_doubles(const pnec_hip_problem *p) { return p ? p->data_doubles : 0; }

int pnec_hip_problem_export_payload(const pnec_hip_problem *p, double *out, int space, void *stream_) {
  if (!p || !out) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
  if (space != PNEC_HIP_MEM_DEVICE && space != PNEC_HIP_MEM_HOST)
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "bad memory space");
  if (p->data_doubles == 0) return 0;
  DeviceGuard guard(p->device);
  hipStream_t stream = (hipStream_t)stream_;
  PNEC_HIP_TRY(hipMemcpyAsync(out, p->d_data, sizeof(double) * p->data_doubles,
                              space == PNEC_HIP_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, stream));
  if (space == PNEC_HIP_MEM_HOST) PNEC_HIP_TRY(hipStreamSynchronize(stream));
  return 0;
}

int64_t pnec_hip_problem_num_pairs(const pnec_hip_problem *p) { return p ? p->n_pairs : 0; }
int64_t pnec_hip_problem_num_correspondences(const pnec_hip_problem *p) {
  return p && materialize(p) == 0 ? p->n_corr : 0;
}
int64_t pnec_hip_problem_max_correspondences(const pnec_hip_problem *p) {
  return p && materialize(p) == 0 ? p->n_max : 0;
}
int64_t pnec_hip_problem_payload_bytes(const pnec_hip_problem *p) {
  return p && materialize(p) == 0 ? p->n_corr * p->nc * (int64_t)sizeof(double) : 0;
}
int pnec_hip_problem_offsets(const pnec_hip_problem *p, int64_t *out) {
  if (!p || !out) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
  if (int rc = materialize(p)) return rc;
  std::memcpy(out, p->offsets.data(), sizeof(int64_t) * p->offsets.size());
  return 0;
}
int pnec_hip_problem_mode(const pnec_hip_problem *p) { return p ? p->mode : -1; }
int pnec_hip_problem_device(const pnec_hip_problem *p) { return p ? p->device : -1; }

int pnec_hip_describe_launch(const pnec_hip_problem *p, const pnec_hip_options *opt,
                             int32_t *corr_per_lane, int32_t *waves_per_pair,
                             int32_t *lds_corr_per_lane, int32_t *threads_per_block,
                             int32_t *resident) {
  if (!p) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "problem is NULL");
  Geometry g;
  if (int rc = choose_geometry(p, opt, &g)) return rc;
  if (corr_per_lane) *corr_per_lane = g.cpl;
  if (waves_per_pair) *waves_per_pair = g.wpp;
  if (lds_corr_per_lane) *lds_corr_per_lane = g.ldsk;
  if (threads_per_block) *threads_per_block = kWave * g.wpp;
  if (resident) *resident = g.resident ? 1 : 0;
  return 0;
}

int pnec_hip_solve(pnec_hip_problem *p, const double *init_q, const double *init_t, int32_t n_hyp,
                   const double *hyp_t, double reg, const pnec_hip_options *opt_in, double *out_q,
                   double *out_t, double *out_cost, int32_t *out_iterations, int32_t *out_status,
                   int space, void *stream_) {
  if (!p) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "problem is NULL");
  if (!init_q) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "init_q is NULL");
  if (!hyp_t) n_hyp = 1;
  if (n_hyp < 1) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "n_hyp must be >= 1");
  if (!hyp_t && !init_t) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "init_t and hyp_t are both NULL");
  if (int rc = check_space("", space)) return rc;
  pnec_hip_options opt;
  if (opt_in)
    opt = *opt_in;
  else
    pnec_hip_default_options(&opt);
  if (opt.max_num_iterations < 0) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "max_num_iterations < 0");
  if (opt.flags & ~(PNEC_HIP_OPT_COUNT_PASSES | PNEC_HIP_OPT_JACOBIAN_NUMERIC_CENTRAL))
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "pnec_hip_options.flags: undefined bit set");
  const bool numeric = (opt.flags & PNEC_HIP_OPT_JACOBIAN_NUMERIC_CENTRAL) != 0;
  if (numeric) {   // verification mode: the streaming form, whatever the tuning fields say
    opt.corr_per_lane = 0;
    opt.waves_per_pair = kStreamWaves;
    opt.lds_corr_per_lane = 0;
  }
  int64_t S;
  if (int rc = pose_slots(p, n_hyp, "solves", &S)) return rc;
  if (S == 0) return 0;
  Geometry g;
  if (int rc = choose_geometry(p, &opt, &g)) return rc;

  hipStream_t stream = (hipStream_t)stream_;
  CallArrays io(p, space, stream);
  SolveArgs a;
  std::memset(&a, 0, sizeof(a));
  a.data = p->d_data;
  a.block_offset = p->d_block_offset;
  a.count = p->d_count;
  a.n_solves = S;
  a.n_hyp = n_hyp;
  a.reg = reg;
  a.opt = opt;
  finish_args(a);
  a.numeric_jacobian = numeric ? 1 : 0;
  if (opt.flags & PNEC_HIP_OPT_COUNT_PASSES) {   // diagnostics: count the passes this call executes (pnec_hip_work_counters)
    if (int rc = solve_work_buffer(p->device, &a.work)) return rc;
  }

  // (every output is staged, wanted or not)
  const int64_t P = p->n_pairs;
  io.in(a.init_q, init_q, 4 * P);
  io.in(a.init_t, init_t, 3 * P);
  io.in(a.hyp_t, hyp_t, 3 * S);
  io.out(a.out_q, out_q, 4 * S, kKeep);
  io.out(a.out_t, out_t, 3 * S, kKeep);
  io.out(a.out_cost, out_cost, S, kKeep);
  io.out(a.out_iterations, out_iterations, S, kKeep);
  io.out(a.out_status, out_status, S, kKeep);
  if (int rc = io.commit()) return rc;

  // several hypotheses per pair on a several-wavefront geometry: the block-per-(pair, group of hypotheses) form -- the
  // pair's payload loaded once per group, one LM step for the whole group (bit-identical results).  PNEC_SOLVE_GROUPS=0
  // keeps the one-solve-per-block launch (A/B, and the bit-identity test).
  static const bool use_groups = [] {
    const char *ev = std::getenv("PNEC_SOLVE_GROUPS");
    return !(ev && *ev == '0');
  }();
  auto launch_on = [&](const Geometry &gg, const SolveArgs &aa, hipStream_t st) -> hipError_t {
    if (use_groups && aa.n_hyp > 1 && gg.resident && !aa.trace && !aa.numeric_jacobian &&
        (gg.wpp >= 2 ? group_geometry_ok(p->mode, gg.cpl, gg.wpp, gg.ldsk)
                     : pairhyp_geometry_ok(p->mode, gg.cpl, gg.wpp, gg.ldsk))) {
      switch (p->mode) {
        case PNEC_HIP_MODE_NEC: return launch_solve_group_mode_0(gg.cpl, gg.wpp, gg.ldsk, aa, st);
        case PNEC_HIP_MODE_TARGET: return launch_solve_group_mode_1(gg.cpl, gg.wpp, gg.ldsk, aa, st);
        case PNEC_HIP_MODE_HOST: return launch_solve_group_mode_2(gg.cpl, gg.wpp, gg.ldsk, aa, st);
        default: return launch_solve_group_mode_3(gg.cpl, gg.wpp, gg.ldsk, aa, st);
      }
    }
    switch (p->mode) {
      case PNEC_HIP_MODE_NEC: return launch_solve_mode_0(gg.cpl, gg.wpp, gg.ldsk, gg.resident, aa, st);
      case PNEC_HIP_MODE_TARGET: return launch_solve_mode_1(gg.cpl, gg.wpp, gg.ldsk, gg.resident, aa, st);
      case PNEC_HIP_MODE_HOST: return launch_solve_mode_2(gg.cpl, gg.wpp, gg.ldsk, gg.resident, aa, st);
      default: return launch_solve_mode_3(gg.cpl, gg.wpp, gg.ldsk, gg.resident, aa, st);
    }
  };
  auto launch = [&](const Geometry &gg, const SolveArgs &aa) -> hipError_t { return launch_on(gg, aa, stream); };
  // PNEC_HIP_TRACE=<file>: per-workgroup phase timestamps of every launch (diagnostics; adds a
  // device synchronisation, so never set it for timed runs)
  const char *trace_path = std::getenv("PNEC_HIP_TRACE");
  unsigned long long *d_trace = nullptr;
  const bool forced = opt.corr_per_lane > 0 || opt.waves_per_pair > 0;
  if (!forced) {
    if (int rc = ensure_buckets(p)) return rc;
  }
  if (trace_path && *trace_path) {
    PNEC_HIP_TRY(dev_alloc(&d_trace, sizeof(unsigned long long) * 4 * S));
    const hipError_t te = hipMemsetAsync(d_trace, 0, sizeof(unsigned long long) * 4 * S, stream);
    if (te != hipSuccess) {
      (void)dev_free(d_trace);
      return fail_hip(te, "hipMemsetAsync(trace)");
    }
    a.trace = d_trace;
  }
  hipError_t e = hipSuccess;
  if (forced || p->buckets.size() <= 1) {
    e = launch(g, a);
  } else {
    // ragged batch: one launch per geometry in use, over the pairs that fit it -- side by side: the first on
    // the caller's stream, the others on streams of the batch's own that fork from it and join it again
    const size_t n_side = p->buckets.size() - 1;
    if (int rc = ensure_side_streams(p, n_side)) {
      if (d_trace) (void)dev_free(d_trace);
      return rc;
    }
    e = hipEventRecord(p->fork_event, stream);
    for (size_t b = 0; b < p->buckets.size() && e == hipSuccess; ++b) {
      const auto &bk = p->buckets[b];
      SolveArgs ab = a;
      ab.pair_index = p->d_bucket_pairs + bk.first;
      ab.n_solves = bk.count * (int64_t)n_hyp;
      if (ab.trace) ab.trace += 4 * (size_t)(bk.first * (int64_t)n_hyp);  // records are indexed by blockIdx per launch
      const Geometry gb = {bk.cpl, bk.wpp, bk.ldsk, bk.resident};
      if (b == 0) {
        e = launch_on(gb, ab, stream);
      } else {
        hipStream_t st = p->side_streams[b - 1];
        e = hipStreamWaitEvent(st, p->fork_event, 0);
        if (e == hipSuccess) e = launch_on(gb, ab, st);
        if (e == hipSuccess) e = hipEventRecord(p->side_done[b - 1], st);
        if (e == hipSuccess) e = hipStreamWaitEvent(stream, p->side_done[b - 1], 0);
      }
    }
  }
  if (d_trace) {
    std::vector<unsigned long long> h(4 * (size_t)S);
    hipError_t te = hipStreamSynchronize(stream);
    if (te == hipSuccess) te = hipMemcpy(h.data(), d_trace, sizeof(unsigned long long) * h.size(), hipMemcpyDeviceToHost);
    (void)dev_free(d_trace);
    if (te == hipSuccess) {
      if (FILE *f = std::fopen(trace_path, "ab")) {
        std::fwrite(h.data(), sizeof(unsigned long long), h.size(), f);
        std::fclose(f);
      }
    }
  }
  if (e != hipSuccess) return fail_hip(e, "lm_solve_kernel launch");

  return io.finish();
}

int pnec_hip_select_best(int64_t n_pairs, int32_t n_hyp, const double *cost, int32_t *best_index,
                         int space, int device, void *stream_) {
  if (n_pairs < 0 || n_hyp < 1 || !cost || !best_index)
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "bad arguments");
  if (n_pairs == 0) return 0;
  DeviceGuard guard(device);
  if (!guard.ok) return fail(PNEC_HIP_ERR_HIP_RUNTIME, "hipSetDevice failed");
  hipStream_t stream = (hipStream_t)stream_;
  const double *d_cost = cost;
  int32_t *d_best = best_index;
  double *tmp_c = nullptr;
  int32_t *tmp_b = nullptr;
  if (space == PNEC_HIP_MEM_HOST) {
    PNEC_HIP_TRY(dev_alloc(&tmp_c, sizeof(double) * n_pairs * n_hyp));
    hipError_t e = dev_alloc(&tmp_b, sizeof(int32_t) * n_pairs);
    if (e == hipSuccess)
      e = hipMemcpyAsync(tmp_c, cost, sizeof(double) * n_pairs * n_hyp, hipMemcpyHostToDevice, stream);
    if (e != hipSuccess) {
      (void)dev_free(tmp_c);
      if (tmp_b) (void)dev_free(tmp_b);
      return fail_hip(e, "select_best staging");
    }
    d_cost = tmp_c;
    d_best = tmp_b;
  }
  hipError_t e = launch_select_best(n_pairs, (int)n_hyp, d_cost, d_best, stream);
  if (space == PNEC_HIP_MEM_HOST) {
    if (e == hipSuccess)
      e = hipMemcpyAsync(best_index, tmp_b, sizeof(int32_t) * n_pairs, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    (void)dev_free(tmp_c);
    (void)dev_free(tmp_b);
  }
  if (e != hipSuccess) return fail_hip(e, "select_best_kernel");
  return 0;
}

int pnec_hip_cost_function(pnec_hip_problem *p, const double *q, const double *t, double *out,
                           int space, void *stream_) {
  if (!p || !q || !t || !out) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
  if (p->mode != PNEC_HIP_MODE_TARGET)
    return fail(PNEC_HIP_ERR_UNSUPPORTED, "cost_function needs a TARGET-mode problem");
  if (p->n_pairs == 0) return 0;
  hipStream_t stream = (hipStream_t)stream_;
  const double *d_q, *d_t;
  double *d_out;
  const int64_t P = p->n_pairs;
  CallArrays io(p, space, stream);
  io.in(d_q, q, 4 * P);
  io.in(d_t, t, 3 * P);
  io.out(d_out, out, P);
  if (int rc = io.commit()) return rc;
  PNEC_HIP_TRY(launch_cost_function(P, p->d_data, p->d_block_offset, p->d_count, d_q, d_t, d_out, stream));
  return io.finish();
}

// J'J, its lifted inverse, J'r and the cost of every (pair, pose) slot: pnec_pose_cov.hip
int pnec_hip_pose_covariance(pnec_hip_problem *p, const double *q, const double *t, int32_t n_hyp, double reg,
                             double *out_info, double *out_cov, double *out_grad, double *out_cost,
                             int32_t *out_status, int space, void *stream_) {
  if (int rc = check_pose_args("pose_covariance", p, q, t, n_hyp)) return rc;
  if (!out_info && !out_cov && !out_grad && !out_cost && !out_status)
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "pose_covariance: every output is NULL");
  if (int rc = check_space("", space)) return rc;
  int64_t S;
  if (int rc = pose_slots(p, n_hyp, "poses", &S)) return rc;
  if (S == 0) return 0;
  hipStream_t stream = (hipStream_t)stream_;
  CallArrays io(p, space, stream);
  PoseCovArgs a;
  a.data = p->d_data;
  a.block_offset = p->d_block_offset;
  a.count = p->d_count;
  a.n_hyp = n_hyp;
  a.reg = reg;
  io.in(a.q, q, 4 * S);
  io.in(a.t, t, 3 * S);
  io.out(a.out_cov, out_cov, 36 * S);
  io.out(a.out_info, out_info, 15 * S);
  io.out(a.out_grad, out_grad, 5 * S);
  io.out(a.out_cost, out_cost, S);
  io.out(a.out_status, out_status, S);
  if (int rc = io.commit()) return rc;
  // n_max of a batch whose sizes still live on the device (select) is the source's: an upper bound, which is all the
  // block size needs (the wavefronts a pair uses follow from its own count)
  PNEC_HIP_TRY(launch_pose_covariance(p->mode, S, cov_waves(p->n_max), a, stream));
  return io.finish();
}

// r_i, its variance and the gate's verdict per correspondence, chi-square sums per (pair, pose) slot: pnec_residuals.hip
int pnec_hip_residuals(pnec_hip_problem *p, const double *q, const double *t, int32_t n_hyp, double reg, double gate,
                       double *out_residual, double *out_variance, uint8_t *out_mask, double *out_chi2,
                       double *out_gated_chi2, int32_t *out_gated_count, double *out_max_abs, int space, void *stream_) {
  if (int rc = check_pose_args("residuals", p, q, t, n_hyp)) return rc;
  if (!(gate >= 0.0)) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "residuals: gate must be >= 0 (sigmas; +inf allowed)");
  if (!out_residual && !out_variance && !out_mask && !out_chi2 && !out_gated_chi2 && !out_gated_count && !out_max_abs)
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "residuals: every output is NULL");
  if (int rc = check_space("residuals: ", space)) return rc;
  int64_t S;
  if (int rc = pose_slots(p, n_hyp, "poses", &S)) return rc;
  if (S == 0) return 0;
  hipStream_t stream = (hipStream_t)stream_;
  CallArrays io(p, space, stream);
  ResidualArgs a;
  a.data = p->d_data;
  a.block_offset = p->d_block_offset;
  a.count = p->d_count;
  a.offsets = p->d_offsets;
  a.n_hyp = n_hyp;
  a.reg = reg;
  a.gate = gate;
  // HOST space: the lengths of the caller's arrays are the batch's own totals, so a batch made by select waits for its
  // sizes here.  (DEVICE space needs no host-side number: the kernel reads the batch's offsets.)
  if (io.host())
    if (int rc = materialize(p)) return rc;
  const int64_t M = p->n_corr * (int64_t)n_hyp;   // entries of a per-correspondence array
  io.in(a.q, q, 4 * S);
  io.in(a.t, t, 3 * S);
  io.out(a.out_chi2, out_chi2, S);
  io.out(a.out_gated_chi2, out_gated_chi2, S);
  io.out(a.out_max_abs, out_max_abs, S);
  io.out(a.out_residual, out_residual, M);
  io.out(a.out_variance, out_variance, M);
  io.out(a.out_mask, out_mask, M);
  io.out(a.out_gated_count, out_gated_count, S);
  if (int rc = io.commit()) return rc;
  // n_max of a batch whose sizes still live on the device (select) is the source's: an upper bound, which is all the
  // block size needs (the wavefronts a pair uses follow from its own count)
  PNEC_HIP_TRY(launch_residuals(p->mode, S, cov_waves(p->n_max), a, stream));
  return io.finish();
}

// input gradients of the minimiser at every (pair, pose) slot: pnec_sensitivity.hip
int pnec_hip_pose_sensitivity(pnec_hip_problem *p, const double *q, const double *t, const double *grad_pose,
                              int32_t n_hyp, double reg, int32_t flags, double *out_grad_bvs1, double *out_grad_bvs2,
                              double *out_grad_covs, double *out_grad_covs_host, double *out_lambda,
                              double *out_hessian, double *out_grad, double *out_newton, int32_t *out_status,
                              int space, void *stream_) {
  if (int rc = check_pose_args("pose_sensitivity", p, q, t, n_hyp)) return rc;
  if (!grad_pose) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "pose_sensitivity: grad_pose is NULL");
  if (flags & ~(PNEC_HIP_SENS_GAUSS_NEWTON | PNEC_HIP_SENS_ZERO_ON_FAILURE))
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "pose_sensitivity: unknown bit in flags");
  if (!out_grad_bvs1 && !out_grad_bvs2 && !out_grad_covs && !out_grad_covs_host && !out_lambda && !out_hessian &&
      !out_grad && !out_newton && !out_status)
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "pose_sensitivity: every output is NULL");
  if (out_grad_covs && p->mode == PNEC_HIP_MODE_NEC)
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "pose_sensitivity: out_grad_covs on a NEC batch (it has no covariances)");
  if (out_grad_covs_host && p->mode != PNEC_HIP_MODE_SYM)
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "pose_sensitivity: out_grad_covs_host needs a SYM batch");
  if (int rc = check_space("pose_sensitivity: ", space)) return rc;
  int64_t S;
  if (int rc = pose_slots(p, n_hyp, "poses", &S)) return rc;
  if (S == 0) return 0;
  hipStream_t stream = (hipStream_t)stream_;
  CallArrays io(p, space, stream);
  SensitivityArgs a;
  a.data = p->d_data;
  a.block_offset = p->d_block_offset;
  a.count = p->d_count;
  a.offsets = p->d_offsets;
  a.n_hyp = n_hyp;
  a.flags = flags;
  a.reg = reg;
  // HOST space: the lengths of the caller's arrays are the batch's own totals, so a batch made by select waits for its
  // sizes here.  (DEVICE space needs no host-side number: the kernel reads the batch's offsets.)
  if (io.host())
    if (int rc = materialize(p)) return rc;
  const int64_t M = p->n_corr * (int64_t)n_hyp;   // rows of a per-correspondence array
  io.in(a.q, q, 4 * S);
  io.in(a.t, t, 3 * S);
  io.in(a.grad_pose, grad_pose, 6 * S);
  io.out(a.out_lambda, out_lambda, 5 * S);
  io.out(a.out_hessian, out_hessian, 15 * S);
  io.out(a.out_grad, out_grad, 5 * S);
  io.out(a.out_newton, out_newton, 5 * S);
  io.out(a.out_grad_bvs1, out_grad_bvs1, 3 * M);
  io.out(a.out_grad_bvs2, out_grad_bvs2, 3 * M);
  io.out(a.out_grad_covs, out_grad_covs, 9 * M);
  io.out(a.out_grad_covs_host, out_grad_covs_host, 9 * M);
  io.out(a.out_status, out_status, S);
  if (int rc = io.commit()) return rc;
  // n_max of a batch whose sizes still live on the device (select) is the source's: an upper bound, which is all the
  // block size needs (the wavefronts a pair uses follow from its own count)
  PNEC_HIP_TRY(launch_pose_sensitivity(p->mode, S, cov_waves(p->n_max), a, stream));
  return io.finish();
}

// depths, points, parallax and depth variance per correspondence, the cheirality vote per (pair, pose) slot:
// pnec_triangulate.hip
int pnec_hip_triangulate(pnec_hip_problem *p, const double *q, const double *t, int32_t n_hyp, int32_t flags,
                         double *out_point, double *out_depth1, double *out_depth2, double *out_parallax,
                         double *out_depth1_var, uint8_t *out_front, int32_t *out_n_front, int32_t *out_n_back,
                         int32_t *out_sign, double *out_t_oriented, double *out_parallax_mean, int space, void *stream_) {
  if (int rc = check_pose_args("triangulate", p, q, t, n_hyp)) return rc;
  if (flags & ~PNEC_HIP_TRI_ORIENT) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "triangulate: unknown bit in flags");
  if (!out_point && !out_depth1 && !out_depth2 && !out_parallax && !out_depth1_var && !out_front && !out_n_front &&
      !out_n_back && !out_sign && !out_t_oriented && !out_parallax_mean)
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "triangulate: every output is NULL");
  if (int rc = check_space("triangulate: ", space)) return rc;
  int64_t S;
  if (int rc = pose_slots(p, n_hyp, "poses", &S)) return rc;
  if (S == 0) return 0;
  if (int rc = check_planes_fit("triangulate", p)) return rc;
  hipStream_t stream = (hipStream_t)stream_;
  CallArrays io(p, space, stream);
  TriangulateArgs a;
  a.data = p->d_data;
  a.block_offset = p->d_block_offset;
  a.count = p->d_count;
  a.offsets = p->d_offsets;
  a.n_hyp = n_hyp;
  a.flags = flags;
  // HOST space: the lengths of the caller's arrays are the batch's own totals, so a batch made by select waits for its
  // sizes here.  (DEVICE space needs no host-side number: the kernel reads the batch's offsets.)
  if (io.host())
    if (int rc = materialize(p)) return rc;
  const int64_t M = p->n_corr * (int64_t)n_hyp;   // entries of a per-correspondence array
  io.in(a.q, q, 4 * S);
  io.in(a.t, t, 3 * S);
  io.out(a.out_t_oriented, out_t_oriented, 3 * S);
  io.out(a.out_parallax_mean, out_parallax_mean, S);
  io.out(a.out_point, out_point, 3 * M);
  io.out(a.out_depth1, out_depth1, M);
  io.out(a.out_depth2, out_depth2, M);
  io.out(a.out_parallax, out_parallax, M);
  io.out(a.out_depth1_var, out_depth1_var, M);
  io.out(a.out_front, out_front, M);
  io.out(a.out_n_front, out_n_front, S);
  io.out(a.out_n_back, out_n_back, S);
  io.out(a.out_sign, out_sign, S);
  if (int rc = io.commit()) return rc;
  // n_max of a batch whose sizes still live on the device (select) is the source's: an upper bound, which is all the
  // block size needs (the wavefronts a pair uses follow from its own count)
  PNEC_HIP_TRY(launch_triangulate(p->mode, S, cov_waves(p->n_max), a, stream));
  return io.finish();
}

// essential matrix and pose of every pair from its correspondences alone: pnec_eight_point.hip
int pnec_hip_eight_point(pnec_hip_problem *p, int32_t flags, double *out_q, double *out_t, double *out_E,
                         double *out_singular, double *out_gap, double *out_quality, int32_t *out_choice,
                         int32_t *out_status, int space, void *stream_) {
  if (!p) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "eight_point: problem is NULL");
  if (flags & ~PNEC_HIP_EP_QUALITY_ALL) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "eight_point: unknown bit in flags");
  if (!out_q && !out_t && !out_E && !out_singular && !out_gap && !out_quality && !out_choice && !out_status)
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "eight_point: every output is NULL");
  if (int rc = check_space("eight_point: ", space)) return rc;
  const int64_t P = p->n_pairs;
  if (P > 0x7fffffffLL) return fail(PNEC_HIP_ERR_UNSUPPORTED, "more than 2^31-1 pairs in one call");
  if (P == 0) return 0;
  hipStream_t stream = (hipStream_t)stream_;
  CallArrays io(p, space, stream);
  EightPointArgs a;
  a.data = p->d_data;
  a.block_offset = p->d_block_offset;
  a.count = p->d_count;
  a.flags = flags;
  io.out(a.out_q, out_q, 4 * P);
  io.out(a.out_t, out_t, 3 * P);
  io.out(a.out_E, out_E, 9 * P);
  io.out(a.out_singular, out_singular, 3 * P);
  io.out(a.out_gap, out_gap, P);
  io.out(a.out_quality, out_quality, 4 * P);
  io.out(a.out_choice, out_choice, P);
  io.out(a.out_status, out_status, P);
  if (int rc = io.commit()) return rc;
  PNEC_HIP_TRY(launch_eight_point(P, a, stream));
  return io.finish();
}

// every solution of the five-point / seven-point solver and the chosen pose of every pair: pnec_essential_minimal.hip
int pnec_hip_essential_minimal(pnec_hip_problem *p, int32_t algorithm, int32_t flags, double *out_q, double *out_t,
                               double *out_E, double *out_singular, double *out_gap, int32_t *out_n_solutions,
                               double *out_E_all, double *out_quality, int32_t *out_choice, int32_t *out_status,
                               int space, void *stream_) {
  if (!p) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "essential_minimal: problem is NULL");
  if (algorithm != PNEC_HIP_EM_NISTER && algorithm != PNEC_HIP_EM_SEVENPT)
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "essential_minimal: algorithm is neither NISTER nor SEVENPT");
  if (flags & ~PNEC_HIP_EM_QUALITY_ALL) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "essential_minimal: unknown bit in flags");
  if (!out_q && !out_t && !out_E && !out_singular && !out_gap && !out_n_solutions && !out_E_all && !out_quality &&
      !out_choice && !out_status)
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "essential_minimal: every output is NULL");
  if (int rc = check_space("essential_minimal: ", space)) return rc;
  const int64_t P = p->n_pairs;
  if (P > 0x7fffffffLL) return fail(PNEC_HIP_ERR_UNSUPPORTED, "more than 2^31-1 pairs in one call");
  if (P == 0) return 0;
  hipStream_t stream = (hipStream_t)stream_;
  CallArrays io(p, space, stream);
  EssentialMinimalArgs a;
  a.data = p->d_data;
  a.block_offset = p->d_block_offset;
  a.count = p->d_count;
  a.algorithm = algorithm;
  a.flags = flags;
  io.out(a.out_q, out_q, 4 * P);
  io.out(a.out_t, out_t, 3 * P);
  io.out(a.out_E, out_E, 9 * P);
  io.out(a.out_singular, out_singular, 3 * P);
  io.out(a.out_gap, out_gap, P);
  io.out(a.out_n_solutions, out_n_solutions, P);
  io.out(a.out_E_all, out_E_all, 9 * PNEC_HIP_EM_MAX_SOLUTIONS * P);
  io.out(a.out_quality, out_quality, 4 * PNEC_HIP_EM_MAX_SOLUTIONS * P);
  io.out(a.out_choice, out_choice, P);
  io.out(a.out_status, out_status, P);
  if (int rc = io.commit()) return rc;
  PNEC_HIP_TRY(launch_essential_minimal(P, a, stream));
  return io.finish();
}

// the RANSAC forms of the five-, seven- and eight-point baselines, pose and inlier mask of every pair:
// pnec_essential_ransac.hip
int pnec_hip_essential_ransac(pnec_hip_problem *p, int32_t algorithm, uint64_t seed, int64_t first_pair_id,
                              int32_t max_iterations, double threshold, double *out_q, double *out_t, double *out_E,
                              double *out_singular, uint8_t *out_inlier_mask, int32_t *out_inlier_count,
                              int32_t *out_iterations, int32_t *out_attempts, int32_t *out_best_attempt,
                              int32_t *out_status, int space, void *stream_) {
  if (!p) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "essential_ransac: problem is NULL");
  if (algorithm != PNEC_HIP_EM_NISTER && algorithm != PNEC_HIP_EM_SEVENPT && algorithm != PNEC_HIP_EM_EIGHTPT)
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "essential_ransac: algorithm is none of NISTER, SEVENPT, EIGHTPT");
  if (max_iterations < 0) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "essential_ransac: max_iterations < 0");
  if (!std::isfinite(threshold) || !(threshold > 0.0))
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "essential_ransac: threshold is not finite and positive");
  if (first_pair_id < 0) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "essential_ransac: first_pair_id < 0");
  if (!out_q && !out_t && !out_E && !out_singular && !out_inlier_mask && !out_inlier_count && !out_iterations &&
      !out_attempts && !out_best_attempt && !out_status)
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "essential_ransac: every output is NULL");
  if (int rc = check_space("essential_ransac: ", space)) return rc;
  const int64_t P = p->n_pairs;
  if (P > 0x7fffffffLL) return fail(PNEC_HIP_ERR_UNSUPPORTED, "more than 2^31-1 pairs in one call");
  if (P == 0) return 0;
  hipStream_t stream = (hipStream_t)stream_;
  CallArrays io(p, space, stream);
  // HOST space: the mask's length is the batch's own total, so a batch made by select waits for its sizes here.
  // (DEVICE space needs no host-side number: the kernel reads the batch's offsets.)
  if (io.host() && out_inlier_mask)
    if (int rc = materialize(p)) return rc;
  EssentialRansacArgs a;
  a.data = p->d_data;
  a.block_offset = p->d_block_offset;
  a.offsets = p->d_offsets;
  a.count = p->d_count;
  a.algorithm = algorithm;
  a.max_iterations = max_iterations;
  a.seed = seed;
  a.first_pair_id = (uint64_t)first_pair_id;
  a.threshold = threshold;
  io.out(a.out_q, out_q, 4 * P);
  io.out(a.out_t, out_t, 3 * P);
  io.out(a.out_E, out_E, 9 * P);
  io.out(a.out_singular, out_singular, 3 * P);
  io.out(a.out_inlier_mask, out_inlier_mask, p->n_corr);
  io.out(a.out_inlier_count, out_inlier_count, P);
  io.out(a.out_iterations, out_iterations, P);
  io.out(a.out_attempts, out_attempts, P);
  io.out(a.out_best_attempt, out_best_attempt, P);
  io.out(a.out_status, out_status, P);
  if (int rc = io.commit()) return rc;
  PNEC_HIP_TRY(launch_essential_ransac(P, a, stream));
  return io.finish();
}

// the ratio of every pair's baseline to its previous pair's from the tracks they share, and three exact order
// statistics of it per pair: pnec_relative_scale.hip
int pnec_hip_relative_scale(pnec_hip_problem *cur, pnec_hip_problem *prev, const int64_t *prev_pair, const int32_t *link,
                            const double *q_cur, const double *t_cur, const double *q_prev, const double *t_prev,
                            double min_parallax, double *out_ratio, uint8_t *out_used, double *out_scale,
                            int32_t *out_n_linked, int32_t *out_n_used, int space, void *stream_) {
  if (!cur || !prev) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "relative_scale: cur or prev problem is NULL");
  if (!prev_pair || !link) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "relative_scale: prev_pair or link is NULL");
  if (!q_cur || !t_cur || !q_prev || !t_prev)
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "relative_scale: a pose pointer (q_cur, t_cur, q_prev, t_prev) is NULL");
  if (!(min_parallax >= 0.0) || !std::isfinite(min_parallax))
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "relative_scale: min_parallax must be >= 0 and finite (radians)");
  if (!out_ratio && !out_used && !out_scale && !out_n_linked && !out_n_used)
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "relative_scale: every output is NULL");
  if (int rc = check_space("relative_scale: ", space)) return rc;
  if (cur->device != prev->device)
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "relative_scale: cur and prev live on different devices");
  const int64_t P = cur->n_pairs, Pp = prev->n_pairs;
  if (P == 0) return 0;
  if (P > 0x7fffffffLL) return fail(PNEC_HIP_ERR_UNSUPPORTED, "more than 2^31-1 pairs in one call");
  if (int rc = check_planes_fit("relative_scale", cur)) return rc;
  if (int rc = check_planes_fit("relative_scale", prev)) return rc;
  hipStream_t stream = (hipStream_t)stream_;
  CallArrays io(cur, space, stream);
  RelativeScaleArgs a;
  a.data = cur->d_data;
  a.block_offset = cur->d_block_offset;
  a.count = cur->d_count;
  a.offsets = cur->d_offsets;
  a.prev_data = prev->d_data;
  a.prev_block_offset = prev->d_block_offset;
  a.prev_count = prev->d_count;
  a.n_prev_pairs = Pp;
  // sin^2 orders angles only below 90 degrees, which the gate's a10 > 0 enforces: from pi/2 on nothing passes
  const double sn = std::sin(min_parallax);
  a.sin2_min = min_parallax >= 1.5707963267948966 ? 2.0 : sn * sn;
  a.gate_a10 = min_parallax > 0.0 ? 1 : 0;
  // HOST space: the lengths of the caller's arrays are the batch's own totals, so a batch made by select waits for its
  // sizes here.  (DEVICE space needs no host-side number: the kernel reads the batch's offsets, and n_corr of such a batch
  // is the source's, an upper bound.)
  if (io.host())
    if (int rc = materialize(cur)) return rc;
  const int64_t M = cur->n_corr;
  io.in(a.q, q_cur, 4 * P);
  io.in(a.t, t_cur, 3 * P);
  io.in(a.q_prev, q_prev, 4 * Pp);
  io.in(a.t_prev, t_prev, 3 * Pp);
  io.in(a.prev_pair, prev_pair, P);
  io.out(a.out_scale, out_scale, 3 * P);
  io.out(a.ratio, out_ratio, M, kKeep);   // (the pass writes the ratios whether or not the caller wants them)
  io.out(a.out_used, out_used, M);
  io.in(a.link, link, M);
  io.out(a.out_n_linked, out_n_linked, P);
  io.out(a.out_n_used, out_n_used, P);
  if (int rc = io.commit()) return rc;
  if (!io.host() && !out_ratio) {   // DEVICE space without out_ratio: the batch keeps the ratios between the pass and the selection
    const int64_t need = std::max<int64_t>(M, 1);
    if (need > cur->ratio_doubles) {
      if (cur->d_ratio) (void)dev_free(cur->d_ratio);
      cur->d_ratio = nullptr;
      cur->ratio_doubles = 0;
      PNEC_HIP_TRY(dev_alloc(&cur->d_ratio, sizeof(double) * (size_t)need));
      cur->ratio_doubles = need;
    }
    a.ratio = cur->d_ratio;
  }
  // n_max of a batch whose sizes still live on the device (select) is the source's: an upper bound, which is all the
  // block size needs (the wavefronts a pair uses follow from its own count)
  PNEC_HIP_TRY(launch_relative_scale(P, cov_waves(cur->n_max), a, stream));
  return io.finish();
}

// the 2x2 image covariance of keypoints from their image patches: pnec_patch_cov.hip.  No batch is involved: a HOST-space
// call stages in buffers that live for the call only (CallArrays made from the device).
int pnec_hip_patch_covariance(const void *images, int pixel_type, int64_t n_images, int32_t height, int32_t width,
                              int64_t pitch, const int64_t *offsets, int64_t n_points, const double *pts,
                              const double *pattern, int32_t n_pattern, double scaling, const double *angle,
                              double *out_cov, double *out_hessian, double *out_mean, int32_t *out_n_valid,
                              int32_t *out_status, int space, int device, void *stream_) {
  if (!images || !offsets || !pattern || (!pts && n_points > 0))
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "patch_covariance: images, offsets, pts or pattern is NULL");
  if (!out_cov && !out_hessian && !out_mean && !out_n_valid && !out_status)
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "patch_covariance: every output is NULL");
  if (n_pattern < 1 || n_pattern > PNEC_HIP_PATCH_MAX_POINTS)
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "patch_covariance: n_pattern must be 1 .. 64");
  const size_t elem = pixel_bytes(pixel_type);
  if (!elem) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "patch_covariance: unknown pixel_type");
  if (n_images < 1 || height < 1 || width < 1 || n_points < 0)
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "patch_covariance: n_images, height, width must be >= 1, n_points >= 0");
  if (pitch < width) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "patch_covariance: pitch (in elements) is below width");
  if (!(scaling > 0.0) || !std::isfinite(scaling))
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "patch_covariance: scaling must be positive and finite");
  if (int rc = check_space("patch_covariance: ", space)) return rc;
  if (int rc = check_images_fit("patch_covariance", n_images, height, pitch, elem)) return rc;
  if (space == PNEC_HIP_MEM_HOST)
    if (int rc = check_offsets("patch_covariance", "offsets", offsets, n_images, n_points, "n_points")) return rc;
  if (n_points == 0) return 0;
  hipStream_t stream = (hipStream_t)stream_;
  CallArrays io(device, space, stream);
  PatchCovArgs a;
  a.w = width;
  a.h = height;
  a.pitch = pitch;
  a.n_images = n_images;
  a.n_points = n_points;
  a.n_pattern = n_pattern;
  a.scaling = scaling;
  const int64_t M = n_points;
  io.in_bytes(a.images, images, image_block_bytes(elem, n_images, height, pitch, width));
  io.in(a.offsets, offsets, n_images + 1);
  io.in(a.pts, pts, 2 * M);
  io.in(a.pattern, pattern, 2 * (int64_t)n_pattern);
  io.in(a.angle, angle, M);
  io.out(a.out_cov, out_cov, 3 * M);
  io.out(a.out_hessian, out_hessian, 6 * M);
  io.out(a.out_mean, out_mean, M);
  io.out(a.out_n_valid, out_n_valid, M);
  io.out(a.out_status, out_status, M);
  if (int rc = io.commit()) return rc;
  PNEC_HIP_TRY(launch_patch_covariance(pixel_type, a, stream));
  return io.finish();
}

// the pyramid's halving step and the tracker: pnec_patch_track.hip.  Staged like the patch covariances.
int pnec_hip_image_pyramid_level(const void *in, void *out, int pixel_type, int64_t n_images, int32_t height,
                                 int32_t width, int64_t pitch_in, int64_t pitch_out, int space, int device,
                                 void *stream_) {
  if (!in || !out) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "image_pyramid_level: in or out is NULL");
  const size_t elem = pixel_bytes(pixel_type);
  if (!elem) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "image_pyramid_level: unknown pixel_type");
  if (n_images < 1 || height < 4 || width < 4)
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "image_pyramid_level: n_images must be >= 1, height and width >= 4");
  if (pitch_in < width || pitch_out < width / 2)
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "image_pyramid_level: a pitch (in elements) is below its width");
  if (int rc = check_space("image_pyramid_level: ", space)) return rc;
  if (int rc = check_images_fit("image_pyramid_level", n_images, height, pitch_in, elem)) return rc;
  if (int rc = check_images_fit("image_pyramid_level", n_images, height / 2, pitch_out, elem)) return rc;
  hipStream_t stream = (hipStream_t)stream_;
  CallArrays io(device, space, stream);
  PyramidLevelArgs a;
  a.w = width;
  a.h = height;
  a.pitch_in = pitch_in;
  a.pitch_out = pitch_out;
  a.n_images = n_images;
  io.in_bytes(a.in, in, image_block_bytes(elem, n_images, height, pitch_in, width));
  // (the whole output block travels up first: the padding between its rows comes back as the caller had it)
  io.out(a.out, static_cast<uint8_t *>(out), image_block_bytes(elem, n_images, height / 2, pitch_out, width / 2), kPreload);
  if (int rc = io.commit()) return rc;
  PNEC_HIP_TRY(launch_image_pyramid_level(pixel_type, a, stream));
  return io.finish();
}

// pnec_hip_patch_track (tmpl_image NULL, n_tmpl_images = n_images), pnec_hip_patch_track_indexed and
// pnec_hip_patch_track_stored (store given: tmpl is absent, tmpl_image is the slot column): one body
static int check_set_offsets(const std::string &pre, const char *array, const int64_t *offsets, int64_t n, int64_t rows,
                             const char *rows_name);
static int run_patch_track(const char *name, bool stored, const double *store, int64_t n_slots, const void *const *tmpl, const int64_t *tmpl_pitch, const void *const *prev,
                           const int64_t *prev_pitch, const void *const *next, const int64_t *next_pitch,
                           int32_t n_levels, int pixel_type, int64_t n_images, int64_t n_tmpl_images, int32_t height,
                           int32_t width, const int64_t *offsets, int64_t n_points, const double *tmpl_pts,
                           const int32_t *tmpl_image, const double *init_pts, const double *init_angle, double shift_x,
                           double shift_y, const double *pattern, int32_t n_pattern, int32_t max_iterations,
                           double max_recovered_dist2, uint32_t flags, double scaling, double *out_pts,
                           double *out_angle, double *out_cov, double *out_dist2, int32_t *out_status,
                           int32_t *out_lost_level, int space, int device, void *stream_) {
  const std::string pre = std::string(name) + ": ";
  const bool prev_given = prev != nullptr;
  if (stored) {
    if (!store || !tmpl_image || !prev || !prev_pitch)
      return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "store, slot, prev or its pitch array is NULL");
    if (n_slots < 1 || n_slots > 0x7fffffffLL)
      return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "n_slots must be 1 .. 2^31 - 1");
    for (void *o : {(void *)out_pts, (void *)out_angle, (void *)out_cov, (void *)out_dist2, (void *)out_status,
                    (void *)out_lost_level})
      if (o && (o == (const void *)store || o == (const void *)tmpl_image))
        return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "an output is an input (the store or the slot column)");
    // (no template pyramid: the checks below see the previous frame in its place)
    tmpl = prev;
    tmpl_pitch = prev_pitch;
    n_tmpl_images = n_images;
  }
  if (!prev) {
    prev = tmpl;
    prev_pitch = tmpl_pitch;
  }
  if (!tmpl || !tmpl_pitch || !prev_pitch || !next || !next_pitch || !offsets || !pattern || (!tmpl_pts && n_points > 0))
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT,
                pre + "tmpl, next, a pitch array, offsets, tmpl_pts or pattern is NULL");
  if (!out_pts && !out_angle && !out_cov && !out_dist2 && !out_status && !out_lost_level)
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "every output is NULL");
  if (n_levels < 1 || n_levels > PNEC_HIP_TRACK_MAX_LEVELS)
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "n_levels must be 1 .. 8");
  if (max_iterations < 1 || max_iterations > 255)
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "max_iterations must be 1 .. 255");
  if (n_pattern < 1 || n_pattern > PNEC_HIP_PATCH_MAX_POINTS)
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "n_pattern must be 1 .. 64");
  const size_t elem = pixel_bytes(pixel_type);
  if (!elem) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "unknown pixel_type");
  if (flags & ~PNEC_HIP_TRACK_NO_BACKWARD) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "unknown flags");
  if (n_images < 1 || n_points < 0)
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "n_images must be >= 1, n_points >= 0");
  // (the plain call passes n_tmpl_images = n_images and no tmpl_image: none of the three can fire for it)
  if (n_tmpl_images < 1) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "n_tmpl_images must be >= 1");
  if (!tmpl_image && n_tmpl_images != n_images)
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "without tmpl_image, n_tmpl_images must equal n_images");
  if (tmpl_image && !stored && !prev_given)
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "with tmpl_image, prev must be given (tmpl is a stack of other images)");
  if (height < 1 || width < 1 || (height >> (n_levels - 1)) < 4 || (width >> (n_levels - 1)) < 4)
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "the smallest level is below 4 pixels in height or width");
  for (int l = 0; l < n_levels; ++l) {
    if (!tmpl[l] || !prev[l] || !next[l]) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "a level pointer is NULL");
    if (tmpl_pitch[l] < (width >> l) || prev_pitch[l] < (width >> l) || next_pitch[l] < (width >> l))
      return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "a pitch (in elements) is below its level's width");
  }
  if (!(max_recovered_dist2 >= 0.0))
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "max_recovered_dist2 must be >= 0");
  if (!std::isfinite(shift_x) || !std::isfinite(shift_y))
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "shift must be finite");
  if (!(scaling > 0.0) || !std::isfinite(scaling))
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "scaling must be positive and finite");
  if (int rc = check_space(pre, space)) return rc;
  for (int l = 0; l < n_levels; ++l)
    for (const int64_t pitch : {tmpl_pitch[l], prev_pitch[l], next_pitch[l]})
      if (int rc = check_images_fit(name, std::max(n_images, n_tmpl_images), height >> l, pitch, elem)) return rc;
  if (space == PNEC_HIP_MEM_HOST && stored) {
    // (a track set: rows at and beyond offsets[n_images] are padding, whose slot is -1)
    if (int rc = check_set_offsets(pre, "offsets", offsets, n_images, n_points, "n_points")) return rc;
    for (int64_t k = 0; k < offsets[n_images]; ++k)
      if (tmpl_image[k] < 0 || tmpl_image[k] >= n_slots)
        return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "a slot entry below offsets[n_images] lies outside 0 .. n_slots - 1");
  }
  if (space == PNEC_HIP_MEM_HOST && !stored)
    if (int rc = check_offsets(name, "offsets", offsets, n_images, n_points, "n_points")) return rc;
  if (space == PNEC_HIP_MEM_HOST && tmpl_image && !stored)
    for (int64_t k = 0; k < n_points; ++k)
      if (tmpl_image[k] < 0 || tmpl_image[k] >= n_tmpl_images)
        return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "a tmpl_image entry lies outside 0 .. n_tmpl_images - 1");
  if (n_points == 0) return 0;
  hipStream_t stream = (hipStream_t)stream_;
  CallArrays io(device, space, stream);
  PatchTrackArgs a{};
  a.n_levels = n_levels;
  a.w = width;
  a.h = height;
  a.n_images = n_images;
  a.n_points = n_points;
  a.shift_x = shift_x;
  a.shift_y = shift_y;
  a.n_pattern = n_pattern;
  a.max_iterations = max_iterations;
  a.max_recovered_dist2 = max_recovered_dist2;
  a.backward = (flags & PNEC_HIP_TRACK_NO_BACKWARD) ? 0 : 1;
  a.scaling = scaling;
  for (int l = 0; l < n_levels; ++l) {
    a.tmpl.pitch[l] = tmpl_pitch[l];
    a.prev.pitch[l] = prev_pitch[l];
    a.next.pitch[l] = next_pitch[l];
  }
  const int64_t M = n_points;
  auto level_bytes = [&](int l, int64_t pitch, int64_t n = -1) {
    return image_block_bytes(elem, n < 0 ? n_images : n, height >> l, pitch, width >> l);
  };
  // a level that two pyramids share (prev = tmpl) is staged once
  auto shared = [&](int l) { return !tmpl_image && prev[l] == tmpl[l] && prev_pitch[l] == tmpl_pitch[l]; };
  for (int l = 0; l < n_levels; ++l) {
    if (!stored) io.in_bytes(a.tmpl.level[l], tmpl[l], level_bytes(l, tmpl_pitch[l], n_tmpl_images));
    io.in_bytes(a.next.level[l], next[l], level_bytes(l, next_pitch[l]));
    if (!shared(l)) io.in_bytes(a.prev.level[l], prev[l], level_bytes(l, prev_pitch[l]));
  }
  io.in(a.offsets, offsets, n_images + 1);
  io.in(a.tmpl_pts, tmpl_pts, 2 * M);
  io.in(a.init_pts, init_pts, 2 * M);
  io.in(a.init_angle, init_angle, M);
  const int32_t *d_tmpl_image = nullptr;
  io.in(d_tmpl_image, tmpl_image, M);
  const double *d_store = nullptr;
  if (stored) io.in(d_store, store, n_slots * store_slot_doubles(n_levels));
  io.in(a.pattern, pattern, 2 * (int64_t)n_pattern);
  io.out(a.out_pts, out_pts, 2 * M);
  io.out(a.out_angle, out_angle, M);
  io.out(a.out_cov, out_cov, 3 * M);
  io.out(a.out_dist2, out_dist2, M);
  io.out(a.out_status, out_status, M);
  io.out(a.out_lost_level, out_lost_level, M);
  if (int rc = io.commit()) return rc;
  for (int l = 0; l < n_levels; ++l)
    if (shared(l)) a.prev.level[l] = a.tmpl.level[l];
  if (stored) PNEC_HIP_TRY(launch_patch_track_stored(pixel_type, a, d_store, n_slots, d_tmpl_image, stream));
  else if (tmpl_image) PNEC_HIP_TRY(launch_patch_track_indexed(pixel_type, a, d_tmpl_image, n_tmpl_images, stream));
  else PNEC_HIP_TRY(launch_patch_track(pixel_type, a, stream));
  return io.finish();
}

int pnec_hip_patch_track(const void *const *tmpl, const int64_t *tmpl_pitch, const void *const *prev,
                         const int64_t *prev_pitch, const void *const *next, const int64_t *next_pitch,
                         int32_t n_levels, int pixel_type, int64_t n_images, int32_t height, int32_t width,
                         const int64_t *offsets, int64_t n_points, const double *tmpl_pts, const double *init_pts,
                         const double *init_angle, double shift_x, double shift_y, const double *pattern,
                         int32_t n_pattern, int32_t max_iterations, double max_recovered_dist2, uint32_t flags,
                         double scaling, double *out_pts, double *out_angle, double *out_cov, double *out_dist2,
                         int32_t *out_status, int32_t *out_lost_level, int space, int device, void *stream_) {
  return run_patch_track("patch_track", false, nullptr, 0, tmpl, tmpl_pitch, prev, prev_pitch, next, next_pitch, n_levels, pixel_type,
                         n_images, n_images, height, width, offsets, n_points, tmpl_pts, nullptr, init_pts, init_angle,
                         shift_x, shift_y, pattern, n_pattern, max_iterations, max_recovered_dist2, flags, scaling,
                         out_pts, out_angle, out_cov, out_dist2, out_status, out_lost_level, space, device, stream_);
}

int pnec_hip_patch_track_indexed(const void *const *tmpl, const int64_t *tmpl_pitch, int64_t n_tmpl_images,
                                 const void *const *prev, const int64_t *prev_pitch, const void *const *next,
                                 const int64_t *next_pitch, int32_t n_levels, int pixel_type, int64_t n_images,
                                 int32_t height, int32_t width, const int64_t *offsets, int64_t n_points,
                                 const double *tmpl_pts, const int32_t *tmpl_image, const double *init_pts,
                                 const double *init_angle, double shift_x, double shift_y, const double *pattern,
                                 int32_t n_pattern, int32_t max_iterations, double max_recovered_dist2, uint32_t flags,
                                 double scaling, double *out_pts, double *out_angle, double *out_cov,
                                 double *out_dist2, int32_t *out_status, int32_t *out_lost_level, int space, int device,
                                 void *stream_) {
  return run_patch_track("patch_track_indexed", false, nullptr, 0, tmpl, tmpl_pitch, prev, prev_pitch, next, next_pitch, n_levels,
                         pixel_type, n_images, n_tmpl_images, height, width, offsets, n_points, tmpl_pts, tmpl_image,
                         init_pts, init_angle, shift_x, shift_y, pattern, n_pattern, max_iterations, max_recovered_dist2,
                         flags, scaling, out_pts, out_angle, out_cov, out_dist2, out_status, out_lost_level, space,
                         device, stream_);
}

int pnec_hip_patch_track_stored(const double *store, int64_t n_slots, const void *const *prev, const int64_t *prev_pitch,
                                const void *const *next, const int64_t *next_pitch, int32_t n_levels, int pixel_type,
                                int64_t n_images, int32_t height, int32_t width, const int64_t *offsets, int64_t n_points,
                                const double *tmpl_pts, const int32_t *slot, const double *init_pts,
                                const double *init_angle, double shift_x, double shift_y, const double *pattern,
                                int32_t n_pattern, int32_t max_iterations, double max_recovered_dist2, uint32_t flags,
                                double scaling, double *out_pts, double *out_angle, double *out_cov, double *out_dist2,
                                int32_t *out_status, int32_t *out_lost_level, int space, int device, void *stream_) {
  return run_patch_track("patch_track_stored", true, store, n_slots, nullptr, nullptr, prev, prev_pitch, next, next_pitch,
                         n_levels, pixel_type, n_images, 0, height, width, offsets, n_points, tmpl_pts, slot, init_pts,
                         init_angle, shift_x, shift_y, pattern, n_pattern, max_iterations, max_recovered_dist2, flags,
                         scaling, out_pts, out_angle, out_cov, out_dist2, out_status, out_lost_level, space, device,
                         stream_);
}

// stored patches: pnec_patch_store.hip.  Staged like the tracker.
int64_t pnec_hip_patch_store_slot_bytes(int32_t n_levels) {
  if (n_levels < 1 || n_levels > PNEC_HIP_TRACK_MAX_LEVELS) return 0;
  return 8 * store_slot_doubles(n_levels);
}

int pnec_hip_patch_store_add(const void *const *cur, const int64_t *cur_pitch, int32_t n_levels, int pixel_type,
                             int64_t n_images, int32_t height, int32_t width, const int64_t *carried_offsets,
                             const int64_t *offsets, int64_t n_rows, const double *tmpl_pts, int32_t *slot,
                             int64_t per_image_capacity, const double *pattern, int32_t n_pattern, double *store,
                             int64_t n_slots, int space, int device, void *stream_) {
  const std::string pre = "patch_store_add: ";
  if (!cur || !cur_pitch || !offsets || !pattern || !store || (n_rows > 0 && (!tmpl_pts || !slot)))
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "cur, its pitch array, offsets, tmpl_pts, slot, pattern or store is NULL");
  if (n_levels < 1 || n_levels > PNEC_HIP_TRACK_MAX_LEVELS)
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "n_levels must be 1 .. 8");
  if (n_pattern < 1 || n_pattern > PNEC_HIP_PATCH_MAX_POINTS)
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "n_pattern must be 1 .. 64");
  const size_t elem = pixel_bytes(pixel_type);
  if (!elem) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "unknown pixel_type");
  if (n_images < 1 || n_rows < 0) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "n_images must be >= 1, n_rows >= 0");
  if (height < 1 || width < 1 || (height >> (n_levels - 1)) < 4 || (width >> (n_levels - 1)) < 4)
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "the smallest level is below 4 pixels in height or width");
  for (int l = 0; l < n_levels; ++l) {
    if (!cur[l]) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "a level pointer is NULL");
    if (cur_pitch[l] < (width >> l))
      return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "a pitch (in elements) is below its level's width");
  }
  if (per_image_capacity < 1) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "per_image_capacity must be >= 1");
  if (per_image_capacity > kStoreMaxCapacity)
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT,
                pre + "per_image_capacity is above 65536 (PNEC_HIP_PATCH_STORE_MAX_CAPACITY: the assignment's occupancy map)");
  if ((__int128)n_images * per_image_capacity > 0x7fffffffLL)
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "n_images * per_image_capacity does not fit int32 (a slot is an int32)");
  if (n_slots < n_images * per_image_capacity)
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "n_slots is below n_images * per_image_capacity");
  if (n_slots > 0x7fffffffLL) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "n_slots must fit int32");
  if (n_rows > (int64_t)1 << 40) return fail(PNEC_HIP_ERR_UNSUPPORTED, pre + "too many rows");
  const void *ins[] = {carried_offsets, offsets, tmpl_pts, pattern};
  for (const void *i : ins)
    if (i && (i == (const void *)slot || i == (const void *)store))
      return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "an output is an input (slot and store are written)");
  if (slot && (const void *)slot == (const void *)store)
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "an output is an input (slot and store are two arrays)");
  if (int rc = check_space(pre, space)) return rc;
  for (int l = 0; l < n_levels; ++l)
    if (int rc = check_images_fit("patch_store_add", n_images, height >> l, cur_pitch[l], elem)) return rc;
  if (space == PNEC_HIP_MEM_HOST) {
    if (int rc = check_set_offsets(pre, "offsets", offsets, n_images, n_rows, "n_rows")) return rc;
    if (carried_offsets) {
      bool ok = carried_offsets[0] == 0;
      for (int64_t f = 0; ok && f < n_images; ++f) ok = carried_offsets[f] <= carried_offsets[f + 1];
      if (!ok) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "carried_offsets must be non-decreasing from 0");
    }
    for (int64_t f = 0; f < n_images; ++f) {
      int64_t lo, c, take;
      store_counts(carried_offsets, offsets, n_rows, f, lo, c, take);
      for (int64_t r = 0; r < take; ++r)
        if (store_local_slot(slot[lo + r], f, per_image_capacity) < 0)
          return fail(PNEC_HIP_ERR_INVALID_ARGUMENT,
                      pre + "a carried row's slot lies outside its image's f * C .. f * C + C - 1");
    }
  }
  if (n_rows == 0) return 0;
  hipStream_t stream = (hipStream_t)stream_;
  CallArrays io(device, space, stream);
  PatchStoreAssignArgs s{};
  s.n_images = n_images;
  s.n_rows = n_rows;
  s.capacity = per_image_capacity;
  PatchStoreBuildArgs a{};
  a.n_levels = n_levels;
  a.w = width;
  a.h = height;
  a.n_images = n_images;
  a.n_rows = n_rows;
  a.n_pattern = n_pattern;
  a.n_slots = n_slots;
  for (int l = 0; l < n_levels; ++l) {
    a.cur.pitch[l] = cur_pitch[l];
    io.in_bytes(a.cur.level[l], cur[l], image_block_bytes(elem, n_images, height >> l, cur_pitch[l], width >> l));
  }
  io.in(s.carried_offsets, carried_offsets, n_images + 1);
  io.in(s.offsets, offsets, n_images + 1);
  io.in(a.tmpl_pts, tmpl_pts, 2 * n_rows);
  io.in(a.pattern, pattern, 2 * (int64_t)n_pattern);
  io.out(s.slot, slot, n_rows, kPreload);
  // (the whole store travels up first: the slots the call leaves alone come back as the caller had them)
  io.out(a.store, store, n_slots * store_slot_doubles(n_levels), kPreload);
  if (int rc = io.commit()) return rc;
  a.carried_offsets = s.carried_offsets;
  a.offsets = s.offsets;
  a.slot = s.slot;
  PNEC_HIP_TRY(launch_patch_store_assign(s, stream));
  PNEC_HIP_TRY(launch_patch_store_build(pixel_type, a, stream));
  return io.finish();
}

// the bookkeeping of tracks across frames: pnec_tracks.hip.  No batch and no images: staged like the patch covariances.
// HOST space only (the array is read): a set's offsets run from 0 up to at most n_rows without a step down.
static int check_set_offsets(const std::string &pre, const char *array, const int64_t *offsets, int64_t n, int64_t rows,
                             const char *rows_name) {
  bool ok = offsets[0] == 0 && offsets[n] <= rows;
  for (int64_t f = 0; ok && f < n; ++f) ok = offsets[f] <= offsets[f + 1];
  if (!ok)
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT,
                pre + array + " must be non-decreasing from 0 to at most " + rows_name);
  return 0;
}

int pnec_hip_tracks_retain(int64_t n_images, const int64_t *offsets, int64_t n_rows, const int64_t *id,
                           const int32_t *tmpl_image, const double *tmpl_pts, const int32_t *age, const double *pts,
                           const double *cov, const double *trk_pts, const double *trk_angle, const double *trk_cov,
                           const int32_t *trk_status, int32_t max_age, int64_t *out_offsets, int64_t *out_id,
                           int32_t *out_tmpl_image, double *out_tmpl_pts, int32_t *out_age, double *out_pts,
                           double *out_angle, double *out_cov, double *out_prev_pts, double *out_prev_cov,
                           int64_t *out_src, int space, int device, void *stream_) {
  const std::string pre = "tracks_retain: ";
  if (n_images < 1 || n_rows < 0) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "n_images must be >= 1, n_rows >= 0");
  if (!offsets || !out_offsets) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "offsets or out_offsets is NULL");
  if (n_rows > 0 && (!id || !tmpl_image || !tmpl_pts || !age || !pts || !trk_pts || !trk_angle || !trk_status))
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT,
                pre + "id, tmpl_image, tmpl_pts, age, pts, trk_pts, trk_angle or trk_status is NULL");
  if (n_rows > 0 && (!out_id || !out_tmpl_image || !out_tmpl_pts || !out_age || !out_pts || !out_angle))
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT,
                pre + "out_id, out_tmpl_image, out_tmpl_pts, out_age, out_pts or out_angle is NULL");
  const int n_cov = (cov ? 1 : 0) + (trk_cov ? 1 : 0) + (out_cov ? 1 : 0) + (out_prev_cov ? 1 : 0);
  if (n_cov != 0 && n_cov != 4)
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "cov, trk_cov, out_cov and out_prev_cov are given or NULL together");
  if (max_age < 0) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "max_age must be >= 0");
  if (n_images > 0x7fffffffLL || n_rows > (int64_t)1 << 40)
    return fail(PNEC_HIP_ERR_UNSUPPORTED, pre + "too many images or rows");
  const void *ins[] = {offsets, id, tmpl_image, tmpl_pts, age, pts, cov, trk_pts, trk_angle, trk_cov, trk_status};
  void *outs[] = {out_offsets, out_id, out_tmpl_image, out_tmpl_pts, out_age, out_pts, out_angle, out_cov,
                  out_prev_pts, out_prev_cov, out_src};
  for (void *o : outs)
    for (const void *i : ins)
      if (o && o == i) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "an output is an input (the outputs are fresh arrays)");
  if (int rc = check_space(pre, space)) return rc;
  if (space == PNEC_HIP_MEM_HOST)
    if (int rc = check_set_offsets(pre, "offsets", offsets, n_images, n_rows, "n_rows")) return rc;
  hipStream_t stream = (hipStream_t)stream_;
  CallArrays io(device, space, stream);
  TracksRetainArgs a{};
  a.n_images = n_images;
  a.in.n_rows = n_rows;
  a.max_age = max_age;
  const int64_t N = n_rows;
  io.in(a.in.offsets, offsets, n_images + 1);
  io.in(a.in.id, id, N);
  io.in(a.in.tmpl_image, tmpl_image, N);
  io.in(a.in.tmpl_pts, tmpl_pts, 2 * N);
  io.in(a.in.age, age, N);
  io.in(a.in.pts, pts, 2 * N);
  io.in(a.in.cov, cov, 3 * N);
  io.in(a.trk_pts, trk_pts, 2 * N);
  io.in(a.trk_angle, trk_angle, N);
  io.in(a.trk_cov, trk_cov, 3 * N);
  io.in(a.trk_status, trk_status, N);
  io.out(a.out.offsets, out_offsets, n_images + 1);
  io.out(a.out.id, out_id, N);
  io.out(a.out.tmpl_image, out_tmpl_image, N);
  io.out(a.out.tmpl_pts, out_tmpl_pts, 2 * N);
  io.out(a.out.age, out_age, N);
  io.out(a.out.pts, out_pts, 2 * N);
  io.out(a.out.angle, out_angle, N);
  io.out(a.out.cov, out_cov, 3 * N);
  io.out(a.out_prev_pts, out_prev_pts, 2 * N);
  io.out(a.out_prev_cov, out_prev_cov, 3 * N);
  io.out(a.out_src, out_src, N);
  if (int rc = io.commit()) return rc;
  PNEC_HIP_TRY(launch_tracks_retain(a, stream));
  return io.finish();
}

int pnec_hip_tracks_append(int64_t n_images, const int64_t *offsets, int64_t n_rows, const int64_t *id,
                           const int32_t *tmpl_image, const double *tmpl_pts, const int32_t *age, const double *pts,
                           const double *angle, const double *cov, const int64_t *det_offsets, int64_t n_det,
                           const double *det_pts, const double *det_cov, int32_t tmpl_image_base,
                           int64_t per_image_capacity, int64_t *next_id, int64_t n_out, int64_t *out_offsets,
                           int64_t *out_id, int32_t *out_tmpl_image, double *out_tmpl_pts, int32_t *out_age,
                           double *out_pts, double *out_angle, double *out_cov, int64_t *out_dropped, int space,
                           int device, void *stream_) {
  const std::string pre = "tracks_append: ";
  if (n_images < 1 || n_rows < 0 || n_det < 0 || n_out < 0)
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "n_images must be >= 1, n_rows, n_det and n_out >= 0");
  const bool no_set = !offsets;
  if (no_set && (n_rows != 0 || id || tmpl_image || tmpl_pts || age || pts || angle || cov))
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "without offsets (no set) every set pointer is NULL and n_rows is 0");
  if (!no_set && n_rows > 0 && (!id || !tmpl_image || !tmpl_pts || !age || !pts || !angle))
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "id, tmpl_image, tmpl_pts, age, pts or angle is NULL");
  if (!det_offsets || (!det_pts && n_det > 0))
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "det_offsets or det_pts is NULL");
  if (!next_id || !out_offsets) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "next_id or out_offsets is NULL");
  if (n_out > 0 && (!out_id || !out_tmpl_image || !out_tmpl_pts || !out_age || !out_pts || !out_angle))
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT,
                pre + "out_id, out_tmpl_image, out_tmpl_pts, out_age, out_pts or out_angle is NULL");
  if (per_image_capacity < 1) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "per_image_capacity must be >= 1");
  if (n_images > 0x7fffffffLL || n_rows > (int64_t)1 << 40 || n_det > (int64_t)1 << 40 || n_out > (int64_t)1 << 40)
    return fail(PNEC_HIP_ERR_UNSUPPORTED, pre + "too many images or rows");
  if (tmpl_image_base < 0 || (int64_t)tmpl_image_base + n_images - 1 > 0x7fffffffLL)
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "tmpl_image_base must be >= 0 and tmpl_image_base + n_images - 1 fit int32");
  // (an image takes at most every row there is: with the capacity cut there, n_images * capacity stays below 2^73)
  const int64_t total_in = n_rows + n_det;
  const __int128 all_full = (__int128)n_images * std::min(per_image_capacity, total_in);
  if ((__int128)n_out < std::min(all_full, (__int128)total_in))
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "n_out is below min(n_images * per_image_capacity, n_rows + n_det)");
  const void *ins[] = {offsets, id, tmpl_image, tmpl_pts, age, pts, angle, cov, det_offsets, det_pts, det_cov};
  void *outs[] = {out_offsets, out_id, out_tmpl_image, out_tmpl_pts, out_age, out_pts, out_angle, out_cov, out_dropped,
                  next_id};
  for (void *o : outs)
    for (const void *i : ins)
      if (o && o == i) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "an output is an input (the outputs are fresh arrays)");
  if (int rc = check_space(pre, space)) return rc;
  if (space == PNEC_HIP_MEM_HOST) {
    if (!no_set)
      if (int rc = check_set_offsets(pre, "offsets", offsets, n_images, n_rows, "n_rows")) return rc;
    if (int rc = check_set_offsets(pre, "det_offsets", det_offsets, n_images, n_det, "n_det")) return rc;
    int64_t total = 0;
    for (int64_t f = 0; f < n_images; ++f) {
      int64_t take_a, take_d;
      tracks_take(no_set ? 0 : offsets[f + 1] - offsets[f], det_offsets[f + 1] - det_offsets[f], per_image_capacity,
                  take_a, take_d);
      total += take_a + take_d;
    }
    if (n_out < total) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "n_out is below the rows the call produces");
  }
  hipStream_t stream = (hipStream_t)stream_;
  CallArrays io(device, space, stream);
  TracksAppendArgs a{};
  a.n_images = n_images;
  a.in.n_rows = n_rows;
  a.n_det = n_det;
  a.tmpl_image_base = tmpl_image_base;
  a.capacity = per_image_capacity;
  a.n_out = n_out;
  const int64_t N = n_rows, D = n_det, O = n_out;
  io.in(a.in.offsets, offsets, n_images + 1);
  io.in(a.in.id, id, N);
  io.in(a.in.tmpl_image, tmpl_image, N);
  io.in(a.in.tmpl_pts, tmpl_pts, 2 * N);
  io.in(a.in.age, age, N);
  io.in(a.in.pts, pts, 2 * N);
  io.in(a.in.angle, angle, N);
  io.in(a.in.cov, cov, 3 * N);
  io.in(a.det_offsets, det_offsets, n_images + 1);
  io.in(a.det_pts, det_pts, 2 * D);
  io.in(a.det_cov, det_cov, 3 * D);
  io.out(a.next_id, next_id, n_images, kPreload);
  io.out(a.out.offsets, out_offsets, n_images + 1);
  io.out(a.out.id, out_id, O);
  io.out(a.out.tmpl_image, out_tmpl_image, O);
  io.out(a.out.tmpl_pts, out_tmpl_pts, 2 * O);
  io.out(a.out.age, out_age, O);
  io.out(a.out.pts, out_pts, 2 * O);
  io.out(a.out.angle, out_angle, O);
  io.out(a.out.cov, out_cov, 3 * O);
  io.out(a.out_dropped, out_dropped, n_images);
  if (int rc = io.commit()) return rc;
  PNEC_HIP_TRY(launch_tracks_append(a, stream));
  return io.finish();
}

// the join of two sets on their ids: pnec_tracks_link.hip.  Staged like the two calls above.
int pnec_hip_tracks_link(int64_t n_images, const int64_t *cur_offsets, int64_t n_cur, const int64_t *cur_id,
                         const int64_t *prev_offsets, int64_t n_prev, const int64_t *prev_id, int32_t *out_link,
                         int32_t *out_n_linked, int space, int device, void *stream_) {
  const std::string pre = "tracks_link: ";
  if (n_images < 1 || n_images > 0x7fffffffLL) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "n_images must be 1 .. 2^31-1");
  if (n_cur < 0 || n_cur > 0x7fffffffLL || n_prev < 0 || n_prev > 0x7fffffffLL)
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "n_cur and n_prev must be 0 .. 2^31-1");
  if (!cur_offsets || !prev_offsets || !out_link)
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "cur_offsets, prev_offsets or out_link is NULL");
  if ((n_cur > 0 && !cur_id) || (n_prev > 0 && !prev_id))
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "cur_id or prev_id is NULL");
  const void *ins[] = {cur_offsets, cur_id, prev_offsets, prev_id};
  for (const void *i : ins)
    if (i && (i == out_link || i == out_n_linked))
      return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "an output is an input (the outputs are fresh arrays)");
  if ((const void *)out_link == (const void *)out_n_linked)
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "out_link and out_n_linked are the same array");
  if (int rc = check_space(pre, space)) return rc;
  if (space == PNEC_HIP_MEM_HOST) {
    if (int rc = check_set_offsets(pre, "cur_offsets", cur_offsets, n_images, n_cur, "n_cur")) return rc;
    if (int rc = check_set_offsets(pre, "prev_offsets", prev_offsets, n_images, n_prev, "n_prev")) return rc;
  }
  hipStream_t stream = (hipStream_t)stream_;
  if (n_cur == 0) {   // no row: the counts alone
    if (!out_n_linked) return 0;
    if (space == PNEC_HIP_MEM_HOST) {
      std::memset(out_n_linked, 0, (size_t)n_images * sizeof(int32_t));
      return 0;
    }
    DeviceGuard guard(device);
    if (!guard.ok) return fail(PNEC_HIP_ERR_HIP_RUNTIME, "hipSetDevice failed (no such device?)");
    PNEC_HIP_TRY(hipMemsetAsync(out_n_linked, 0, (size_t)n_images * sizeof(int32_t), stream));
    return 0;
  }
  CallArrays io(device, space, stream);
  TracksLinkArgs a{};
  a.n_images = n_images;
  a.n_cur = n_cur;
  a.n_prev = n_prev;
  io.in(a.cur_offsets, cur_offsets, n_images + 1);
  io.in(a.cur_id, cur_id, n_cur);
  io.in(a.prev_offsets, prev_offsets, n_images + 1);
  io.in(a.prev_id, prev_id, n_prev);
  io.out(a.out_link, out_link, n_cur);
  io.out(a.out_n_linked, out_n_linked, n_images);
  if (int rc = io.commit()) return rc;
  PNEC_HIP_TRY(launch_tracks_link(a, stream));
  return io.finish();
}

// keyframe pairs: pnec_keyframe.hip.  Staged like the two calls above.
int pnec_hip_tracks_keyframe(int64_t n_images, const int64_t *offsets, int64_t n_rows, const double *pts,
                             const double *cov, const int64_t *src, const int64_t *new_offsets, int64_t n_new,
                             const double *new_pts, const double *new_cov, int64_t n_key_rows, const double *key_pts,
                             const double *key_cov, const int32_t *span, double min_displacement, int32_t max_span,
                             int64_t *out_offsets, double *out_key_pts, double *out_pts, double *out_cov,
                             double *out_key_cov, int64_t *out_row, uint8_t *out_accepted, double *out_mean,
                             int32_t *out_n_matches, double *next_key_pts, double *next_key_cov, int32_t *next_span,
                             int space, int device, void *stream_) {
  const std::string pre = "tracks_keyframe: ";
  if (n_images < 1 || n_rows < 0 || n_new < 0 || n_key_rows < 0)
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "n_images must be >= 1, n_rows, n_new and n_key_rows >= 0");
  const bool no_set = !offsets;
  if (no_set && (n_rows != 0 || pts || cov || src))
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT,
                pre + "a retained set given in part: without offsets (no set) pts, cov and src are NULL and n_rows is 0");
  if (!no_set && n_rows > 0 && (!pts || !src))
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "a retained set given in part: pts or src is NULL");
  // the state: wanted with a retained set, optional (and not read) without one
  const bool state = !no_set || key_pts || key_cov || span || n_key_rows > 0;
  if (state && (!span || (n_key_rows > 0 && !key_pts) || (key_cov && !key_pts)))
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "the state given in part: span or key_pts is NULL");
  if (!new_offsets || (n_new > 0 && !new_pts))
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "new_offsets or new_pts is NULL");
  if (!out_offsets) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "out_offsets is NULL");
  if (!next_span || (n_new > 0 && !next_key_pts))
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "a next-state array (next_key_pts, next_span) is NULL");
  if (n_rows > 0 && (!out_key_pts || !out_pts || !out_row))
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "out_key_pts, out_pts or out_row is NULL");
  {
    // (an array of no rows says nothing: a caller's empty array may have no address)
    int given = 0, absent = 0;
    auto note = [&](const void *ptr, int64_t rows) { (ptr ? given : absent) += rows > 0; };
    note(new_cov, n_new);
    note(next_key_cov, n_new);
    if (!no_set) {
      note(cov, n_rows);
      note(out_cov, n_rows);
      note(out_key_cov, n_rows);
      note(key_cov, n_key_rows);
    }
    if (given && absent)
      return fail(PNEC_HIP_ERR_INVALID_ARGUMENT,
                  pre + "cov, new_cov, key_cov, out_cov, out_key_cov and next_key_cov are given or NULL together");
  }
  if (!(min_displacement >= 0.0) || std::isinf(min_displacement))
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "min_displacement must be finite and >= 0");
  if (max_span < 1) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "max_span must be >= 1");
  if (n_images > 0x7fffffffLL || n_rows > (int64_t)1 << 40 || n_new > (int64_t)1 << 40 || n_key_rows > (int64_t)1 << 40)
    return fail(PNEC_HIP_ERR_UNSUPPORTED, pre + "too many images or rows");
  const void *ins[] = {offsets, pts, cov, src, new_offsets, new_pts, new_cov, key_pts, key_cov, span};
  void *outs[] = {out_offsets, out_key_pts, out_pts, out_cov, out_key_cov, out_row, out_accepted, out_mean,
                  out_n_matches, next_key_pts, next_key_cov, next_span};
  for (void *o : outs)
    for (const void *i : ins)
      if (o && o == i) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, pre + "an output is an input (the outputs are fresh arrays)");
  if (int rc = check_space(pre, space)) return rc;
  if (space == PNEC_HIP_MEM_HOST) {
    if (!no_set)
      if (int rc = check_set_offsets(pre, "offsets", offsets, n_images, n_rows, "n_rows")) return rc;
    if (int rc = check_set_offsets(pre, "new_offsets", new_offsets, n_images, n_new, "n_new")) return rc;
  }
  hipStream_t stream = (hipStream_t)stream_;
  CallArrays io(device, space, stream);
  KeyframeArgs a{};
  a.n_images = n_images;
  a.n_rows = n_rows;
  a.n_new = n_new;
  a.n_key_rows = no_set ? 0 : n_key_rows;
  a.min_displacement = min_displacement;
  a.max_span = max_span;
  const int64_t N = n_rows, A = n_new, S = a.n_key_rows;
  io.in(a.offsets, offsets, n_images + 1);
  io.in(a.pts, pts, 2 * N);
  io.in(a.cov, cov, 3 * N);
  io.in(a.src, src, N);
  io.in(a.new_offsets, new_offsets, n_images + 1);
  io.in(a.new_pts, new_pts, 2 * A);
  io.in(a.new_cov, new_cov, 3 * A);
  io.in(a.key_pts, no_set ? nullptr : key_pts, 2 * S);   // (the first-frame form reads no state)
  io.in(a.key_cov, no_set ? nullptr : key_cov, 3 * S);
  io.in(a.span, no_set ? nullptr : span, n_images);
  io.out(a.out_offsets, out_offsets, n_images + 1);
  io.out(a.out_key_pts, out_key_pts, 2 * N);
  io.out(a.out_pts, out_pts, 2 * N);
  io.out(a.out_cov, no_set ? nullptr : out_cov, 3 * N);
  io.out(a.out_key_cov, no_set ? nullptr : out_key_cov, 3 * N);
  io.out(a.out_row, out_row, N);
  io.out(a.out_accepted, out_accepted, n_images);
  io.out(a.out_mean, out_mean, n_images);
  io.out(a.out_n_matches, out_n_matches, n_images);
  io.out(a.next_key_pts, next_key_pts, 2 * A);
  io.out(a.next_key_cov, next_key_cov, 3 * A);
  io.out(a.next_span, next_span, n_images);
  if (int rc = io.commit()) return rc;
  PNEC_HIP_TRY(launch_tracks_keyframe(a, stream));
  return io.finish();
}

// keypoint detection: pnec_detect.hip.  Staged like the patch covariances; the outputs travel up first, so that what
// lies beyond out_offsets[n_images] comes back as the caller had it.
int pnec_hip_detect_keypoints(const void *images, int pixel_type, int64_t n_images, int32_t height, int32_t width,
                              int64_t pitch, int32_t grid, int32_t points_per_cell, int32_t min_threshold, int32_t edge,
                              const int64_t *cur_offsets, int64_t n_cur, const double *cur_pts, int32_t *out_cell,
                              int64_t *out_offsets, double *out_pts, int32_t *out_score, int32_t *out_cell_index,
                              int space, int device, void *stream_) {
  if (!images || !out_cell || !out_offsets || !out_pts)
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "detect_keypoints: images, out_cell, out_offsets or out_pts is NULL");
  if (pixel_type == PNEC_HIP_PIXEL_F32)
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT,
                "detect_keypoints: pixel_type F32 has no declared range to quantise to 8 bits (U8 or U16 only)");
  const size_t elem = pixel_bytes(pixel_type);
  if (!elem) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "detect_keypoints: unknown pixel_type");
  if (grid < kDetectMinGrid || grid > kDetectMaxGrid)
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "detect_keypoints: grid must be 8 .. 64");
  if (points_per_cell < 1 || points_per_cell > kDetectMaxPerCell)
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "detect_keypoints: points_per_cell must be 1 .. 4");
  if (min_threshold < 0 || min_threshold > kDetectMaxThreshold)
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "detect_keypoints: min_threshold must be 0 .. 254");
  if (edge < 0) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "detect_keypoints: edge must be >= 0");
  if (n_images < 1) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "detect_keypoints: n_images must be >= 1");
  if (height < grid || width < grid)
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "detect_keypoints: height and width must be at least one grid cell");
  if (pitch < width) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "detect_keypoints: pitch (in elements) is below width");
  if (n_cur < 0) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "detect_keypoints: n_cur must be >= 0");
  if (cur_pts && !cur_offsets)
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "detect_keypoints: cur_pts without cur_offsets");
  if (cur_offsets && !cur_pts && n_cur > 0)
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "detect_keypoints: cur_offsets and n_cur > 0 without cur_pts (NULL)");
  if (int rc = check_space("detect_keypoints: ", space)) return rc;
  if (int rc = check_images_fit("detect_keypoints", n_images, height, pitch, elem)) return rc;
  const bool have_cur = cur_offsets && cur_pts && n_cur > 0;
  if (space == PNEC_HIP_MEM_HOST && cur_offsets)
    if (int rc = check_offsets("detect_keypoints", "cur_offsets", cur_offsets, n_images, n_cur, "n_cur")) return rc;
  DetectArgs a{};
  a.w = width;
  a.h = height;
  a.pitch = pitch;
  a.n_images = n_images;
  a.grid = grid;
  a.per_cell = points_per_cell;
  a.thr = min_threshold;
  a.edge = edge;
  a.nx = width / grid;
  a.ny = height / grid;
  a.x_start = (width % grid) / 2;
  a.y_start = (height % grid) / 2;
  a.n_cur = have_cur ? n_cur : 0;
  const int64_t n_cells = (int64_t)a.nx * a.ny;
  if (n_cells > 0x7fffffffLL / kDetectMaxPerCell || (double)n_images * (double)n_cells * kDetectMaxPerCell > 4.0e18)
    return fail(PNEC_HIP_ERR_UNSUPPORTED, "detect_keypoints: too many cells");
  const int64_t cap = n_images * n_cells * points_per_cell;
  hipStream_t stream = (hipStream_t)stream_;
  CallArrays io(device, space, stream);
  io.in_bytes(a.images, images, image_block_bytes(elem, n_images, height, pitch, width));
  io.in(a.cur_offsets, have_cur ? cur_offsets : nullptr, n_images + 1);
  io.in(a.cur_pts, have_cur ? cur_pts : nullptr, 2 * n_cur);
  io.out(a.out_cell, out_cell, n_images * n_cells);
  io.out(a.out_offsets, out_offsets, n_images + 1);
  io.out(a.out_pts, out_pts, 2 * cap, kPreload);
  io.out(a.out_score, out_score, cap, kPreload);
  io.out(a.out_cell_index, out_cell_index, cap, kPreload);
  if (int rc = io.commit()) return rc;
  PNEC_HIP_TRY(launch_detect_keypoints(pixel_type, a, stream));
  return io.finish();
}

// shared driver of the two eigensolver stages (host or device pointers)
static int run_front_stage(pnec_hip_problem *p, bool weighted, const double *init_q, const double *init_t,
                           double reg, int weighted_iterations, double *out_q, double *out_t, int space,
                           void *stream_) {
  if (!p || !init_q || !out_q || !out_t || (weighted && !init_t))
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
  if (weighted && p->mode != PNEC_HIP_MODE_TARGET)
    return fail(PNEC_HIP_ERR_UNSUPPORTED, "the weighted eigensolver needs a TARGET-mode problem");
  if (int rc = check_space("", space)) return rc;
  if (p->n_pairs == 0) return 0;
  hipStream_t stream = (hipStream_t)stream_;
  const int64_t P = p->n_pairs;
  const double *d_q, *d_t;
  double *d_oq, *d_ot;
  CallArrays io(p, space, stream);
  io.in(d_q, init_q, 4 * P);
  io.in(d_t, init_t, 3 * P);   // (NULL for the unweighted stage, which has no use for it)
  io.out(d_oq, out_q, 4 * P);
  io.out(d_ot, out_t, 3 * P);
  if (int rc = io.commit()) return rc;
  if (int rc = ensure_front(p)) return rc;
  hipError_t e = weighted
                     ? launch_weighted_eigensolver(p->device, p->d_data, p->d_block_offset, p->d_count, P, p->n_max, d_q,
                                                   d_t, reg, weighted_iterations, d_oq, d_ot, nullptr, p->d_front,
                                                   p->d_front_i, stream, p->es_scheme)
                     : launch_nec_eigensolver(p->d_data, p->d_block_offset, p->d_count, P, d_q, d_oq, d_ot,
                                              nullptr, p->d_front, p->d_front_i, stream, p->es_scheme);
  if (e != hipSuccess) return fail_hip(e, weighted ? "weighted_eigensolver_kernel" : "nec_eigensolver_kernel");
  return io.finish();
}

int pnec_hip_problem_set_eigensolver_scheme(pnec_hip_problem *p, int32_t scheme) {
  if (!p) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "problem is NULL");
  if (scheme < PNEC_HIP_ES_NEWTON || scheme > PNEC_HIP_ES_LM)
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "eigensolver scheme: 0 (Newton), 1 (descent) or 2 (LM)");
  p->es_scheme = scheme;
  if (p->sel_view) p->sel_view->es_scheme = scheme;   // a view handed out earlier follows its source
  return 0;
}
int pnec_hip_problem_eigensolver_scheme(const pnec_hip_problem *p) { return p ? p->es_scheme : 0; }

int pnec_hip_problem_set_ransac_flags(pnec_hip_problem *p, int32_t flags) {
  if (!p) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "problem is NULL");
  if (flags & ~PNEC_HIP_RANSAC_CHAINED_STARTS) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "unknown RANSAC flag");
  p->ransac_flags = flags;
  return 0;
}
int pnec_hip_problem_ransac_flags(const pnec_hip_problem *p) { return p ? p->ransac_flags : 0; }

int pnec_hip_nec_eigensolver(pnec_hip_problem *p, const double *init_q, double *out_q, double *out_t,
                             int space, void *stream) {
  return run_front_stage(p, false, init_q, nullptr, 0.0, 0, out_q, out_t, space, stream);
}

int pnec_hip_weighted_eigensolver(pnec_hip_problem *p, const double *init_q, const double *init_t,
                                  double reg, int32_t weighted_iterations, double *out_q, double *out_t,
                                  int space, void *stream) {
  if (weighted_iterations < 0) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "weighted_iterations < 0");
  // DESCENT moves the rotation in every round and keeps a minimiser per round (kEsMaxRounds of them); NEWTON and LM
  // chain calls only while one ends at its evaluation cap, and freeze a pair's rotation after kEsMaxRounds such calls
  if (p && p->es_scheme == PNEC_HIP_ES_DESCENT && weighted_iterations - 1 > kEsMaxRounds)
    return fail(PNEC_HIP_ERR_UNSUPPORTED, "eigensolver scheme 1 (descent) holds at most 16 weighted_iterations");
  return run_front_stage(p, true, init_q, init_t, reg, weighted_iterations, out_q, out_t, space, stream);
}

int pnec_hip_ransac_eigensolver(pnec_hip_problem *p, const double *init_q, uint64_t seed,
                                int32_t max_iterations, int32_t sample_size, double threshold, double *out_q,
                                double *out_t, uint8_t *out_inlier_mask, int32_t *out_inlier_count,
                                int32_t *out_ransac_iterations, int space, void *stream_) {
  if (!p || !init_q || !out_q || !out_t) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
  if (max_iterations < 0 || sample_size < 1) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "bad RANSAC parameters");
  if (sample_size > PNEC_HIP_MAX_RANSAC_SAMPLE)
    return fail(PNEC_HIP_ERR_UNSUPPORTED, "ransac sample_size > 16 is not built (a hypothesis keeps its sample in registers)");
  if (int rc = check_space("", space)) return rc;
  if (p->n_pairs == 0) return 0;
  if (space == PNEC_HIP_MEM_HOST)  // host-side per-correspondence arrays need the exact sizes
    if (int rc = materialize(p)) return rc;
  hipStream_t stream = (hipStream_t)stream_;
  const int64_t P = p->n_pairs, M = p->n_corr;
  const double *d_q;
  double *d_oq, *d_ot;
  uint8_t *d_mask;
  int32_t *d_cnt, *d_it;
  CallArrays io(p, space, stream);
  io.in(d_q, init_q, 4 * P);
  io.out(d_oq, out_q, 4 * P);
  io.out(d_ot, out_t, 3 * P);
  io.out(d_mask, out_inlier_mask, M);
  io.out(d_cnt, out_inlier_count, P, kKeep);   // (the stage fills both counts, wanted or not)
  io.out(d_it, out_ransac_iterations, P, kKeep);
  if (int rc = io.commit()) return rc;
  if (int rc = ensure_front(p)) return rc;
  if (int rc = ensure_order_hint(p)) return rc;
  if (p->order_hint && !d_it) d_it = p->d_hint_its;
  hipError_t e = launch_ransac_eigensolver(p->d_data, p->d_block_offset, p->d_offsets, p->d_count, P, d_q, seed,
                                           /*first_pair_id*/ 0ull, max_iterations, sample_size, threshold, d_oq, d_ot, d_mask, d_cnt, d_it,
                                           p->d_front, p->d_front_i, stream, nullptr, nullptr, nullptr, 0, nullptr, nullptr,
                                           nullptr, nullptr,
                                           p->order_hint && p->order_pairs == P ? p->d_order : nullptr, p->es_scheme,
                                           p->ransac_flags);
  if (e == hipSuccess && p->order_hint) {   // the next call's launch order from this call's counts
    e = launch_ransac_order(d_it, P, p->d_order, stream);
    p->order_pairs = P;
  }
  if (e != hipSuccess) return fail_hip(e, "ransac_eigensolver_kernel");
  return io.finish();
}

static int select_into(pnec_hip_problem *src, const uint8_t *d_mask, hipStream_t stream, pnec_hip_problem *dst,
                       const int32_t *known_counts = nullptr) {
  const int64_t P = src->n_pairs;
  if (int rc = select_prepare(src, stream, dst)) return rc;
  if (P > 0) {
    hipError_t e = hipSuccess;
    if (known_counts) {
      // (the copy kernel also installs the counts in dst and, for a batch of one pair, its AoS offsets; the scan
      // of a larger batch's counts follows it: nothing in the copy needs the new offsets)
      e = launch_select(src->nc, src->d_data, src->d_block_offset, src->d_offsets, src->d_count, d_mask, dst->d_data,
                        dst->d_block_offset, known_counts, dst->d_count, P == 1 ? dst->d_offsets : (int64_t *)nullptr, P,
                        stream);
      if (e == hipSuccess && P > 1) e = launch_offsets_scan(dst->d_count, dst->d_offsets, P, stream);
    } else {
      e = launch_mask_count(P, d_mask, src->d_offsets, src->d_count, dst->d_count,
                            P == 1 ? dst->d_offsets : (int64_t *)nullptr, stream);
      if (e == hipSuccess && P > 1) e = launch_offsets_scan(dst->d_count, dst->d_offsets, P, stream);
      if (e == hipSuccess)
        e = launch_select(src->nc, src->d_data, src->d_block_offset, src->d_offsets, src->d_count, d_mask, dst->d_data,
                          dst->d_block_offset, dst->d_count, dst->d_count, nullptr, P, stream);
    }
    if (e != hipSuccess) return fail_hip(e, "select_kernel");
  }
  return select_finish(src, stream, dst, /*scan*/ false);  // (the scans are among the launches above)
}

int pnec_hip_problem_select(pnec_hip_problem *src, const uint8_t *mask, int space, void *stream_,
                            pnec_hip_problem **out) {
  if (!src || !mask || !out) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
  if (space != PNEC_HIP_MEM_DEVICE && space != PNEC_HIP_MEM_HOST)
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "bad memory space");
  *out = nullptr;
  DeviceGuard guard(src->device);
  hipStream_t stream = (hipStream_t)stream_;
  // a host mask is in the caller's correspondence order: its length is the source's exact total
  if (space == PNEC_HIP_MEM_HOST)
    if (int rc = materialize(src)) return rc;
  pnec_hip_problem *dst = nullptr;
  if (int rc = alloc_like(src, stream, &dst)) return rc;
  const uint8_t *d_mask = mask;
  if (space == PNEC_HIP_MEM_HOST) {
    dst->mask_bytes = std::max<int64_t>(src->n_corr, 1);
    hipError_t e = dev_alloc(&dst->d_mask, (size_t)dst->mask_bytes);
    if (e == hipSuccess && src->n_corr > 0)
      e = hipMemcpyAsync(dst->d_mask, mask, (size_t)src->n_corr, hipMemcpyHostToDevice, stream);
    if (e != hipSuccess) {
      pnec_hip_problem_destroy(dst);
      return fail_hip(e, "mask upload");
    }
    d_mask = dst->d_mask;
  }
  if (int rc = select_into(src, d_mask, stream, dst)) {
    pnec_hip_problem_destroy(dst);
    return rc;
  }
  if (space == PNEC_HIP_MEM_HOST) {  // HOST space calls block (the caller may reuse `mask` right away)
    const hipError_t e = hipStreamSynchronize(stream);
    if (e != hipSuccess) {
      pnec_hip_problem_destroy(dst);
      return fail_hip(e, "select_kernel");
    }
  }
  *out = dst;
  return 0;
}

int pnec_hip_problem_select_view(pnec_hip_problem *src, const uint8_t *mask, int space, void *stream_,
                                 pnec_hip_problem **out) {
  if (!src || !mask || !out) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
  if (space != PNEC_HIP_MEM_DEVICE && space != PNEC_HIP_MEM_HOST)
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "bad memory space");
  *out = nullptr;
  DeviceGuard guard(src->device);
  hipStream_t stream = (hipStream_t)stream_;
  if (space == PNEC_HIP_MEM_HOST)
    if (int rc = materialize(src)) return rc;  // a host mask is sized by the source's exact total
  if (!src->sel_view || src->sel_view->cap_doubles < src->data_doubles || src->sel_view->cap_pairs < src->n_pairs) {
    if (src->sel_view) pnec_hip_problem_destroy(src->sel_view);
    src->sel_view = nullptr;
    if (int rc = alloc_like(src, stream, &src->sel_view)) return rc;
  }
  const uint8_t *d_mask = mask;
  if (space == PNEC_HIP_MEM_HOST) {
    const int64_t M = std::max<int64_t>(src->n_corr, 1);
    if (src->mask_bytes < M) {
      if (src->d_mask) (void)dev_free(src->d_mask);
      src->d_mask = nullptr;
      src->mask_bytes = 0;
      const int64_t want = std::max<int64_t>(M, src->cap_doubles / std::max(src->nc, 1));
      PNEC_HIP_TRY(dev_alloc(&src->d_mask, (size_t)want));
      src->mask_bytes = want;
    }
    if (src->n_corr > 0)
      PNEC_HIP_TRY(hipMemcpyAsync(src->d_mask, mask, (size_t)src->n_corr, hipMemcpyHostToDevice, stream));
    d_mask = src->d_mask;
  }
  if (int rc = select_into(src, d_mask, stream, src->sel_view)) return rc;
  // the view runs the stages the way its source would NOW (the scheme may have been changed since the view was made)
  src->sel_view->es_scheme = src->es_scheme;
  if (space == PNEC_HIP_MEM_HOST) PNEC_HIP_TRY(hipStreamSynchronize(stream));  // (the caller may reuse `mask`)
  *out = src->sel_view;
  return 0;
}

int pnec_hip_unscented_transform(int64_t n, const double *mu, const double *covs, const double *K_inv,
                                 double kappa, int camera_model, double *out_bvs, double *out_covs,
                                 int space, int device, void *stream_) {
  if (n < 0 || (n > 0 && (!mu || !covs || !out_covs)) || !K_inv)
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "NULL argument");
  if (camera_model != 0 && camera_model != 1) return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "camera_model must be 0 or 1");
  if (n == 0) return 0;
  DeviceGuard guard(device);
  if (!guard.ok) return fail(PNEC_HIP_ERR_HIP_RUNTIME, "hipSetDevice failed (no such device?)");
  hipStream_t stream = (hipStream_t)stream_;
  const double *d_mu = mu, *d_cov = covs, *d_K = K_inv;
  double *d_ob = out_bvs, *d_oc = out_covs, *tmp = nullptr;
  if (space == PNEC_HIP_MEM_HOST) {
    PNEC_HIP_TRY(dev_alloc(&tmp, sizeof(double) * (24 * n + 9)));
    double *w = tmp;
    hipError_t e = hipMemcpyAsync(w, mu, sizeof(double) * 3 * n, hipMemcpyHostToDevice, stream);
    d_mu = w; w += 3 * n;
    if (e == hipSuccess) e = hipMemcpyAsync(w, covs, sizeof(double) * 9 * n, hipMemcpyHostToDevice, stream);
    d_cov = w; w += 9 * n;
    if (e == hipSuccess) e = hipMemcpyAsync(w, K_inv, sizeof(double) * 9, hipMemcpyHostToDevice, stream);
    d_K = w; w += 9;
    d_oc = w; w += 9 * n;
    d_ob = out_bvs ? w : nullptr;
    if (e != hipSuccess) {
      (void)dev_free(tmp);
      return fail_hip(e, "unscented_transform staging");
    }
  } else if (space != PNEC_HIP_MEM_DEVICE) {
    return fail(PNEC_HIP_ERR_INVALID_ARGUMENT, "bad memory space");
  }
  hipError_t e = launch_unscented(n, d_mu, d_cov, d_K, kappa, camera_model, d_ob, d_oc, stream);
  if (tmp) {
    if (e == hipSuccess) e = hipMemcpyAsync(out_covs, d_oc, sizeof(double) * 9 * n, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess && out_bvs)
      e = hipMemcpyAsync(out_bvs, d_ob, sizeof(double) * 3 * n, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    (void)dev_free(tmp);
  }
  if (e != hipSuccess) return fail_hip(e, "unscented_kernel");
  return 0;
}

int pnec_hip_selftest(int device) {
  DeviceGuard guard(device);
  if (!guard.ok) return fail(PNEC_HIP_ERR_HIP_RUNTIME, "hipSetDevice failed");
  {  // the front stages' smallest-eigenpair route against the Jacobi sweeps
    double *d = nullptr;
    PNEC_HIP_TRY(dev_alloc(&d, sizeof(double) * 192));
    double h[192];
    hipError_t e = launch_frontend_selftest(d, 0);
    if (e == hipSuccess) e = hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost);
    (void)dev_free(d);
    if (e != hipSuccess) return fail_hip(e, "eig_selftest_kernel");
    for (int i = 0; i < kWave; ++i) {
      char buf[160];
      if (!(h[i] < 1e-14)) {
        std::snprintf(buf, sizeof(buf), "smallest eigenpair: residual %.3g |M| in lane %d", h[i], i);
        return fail(PNEC_HIP_ERR_HIP_RUNTIME, buf);
      }
      if (!(h[64 + i] < 1e-14)) {
        std::snprintf(buf, sizeof(buf), "smallest eigenpair: eigenvalue %.3g |M| above the sweeps' smallest in lane %d", h[64 + i], i);
        return fail(PNEC_HIP_ERR_HIP_RUNTIME, buf);
      }
    }
  }
  double *d = nullptr;
  PNEC_HIP_TRY(dev_alloc(&d, sizeof(double) * kSelftestDoubles));
  double h[kSelftestDoubles];
  hipError_t e = launch_selftest(d, 0);
  if (e == hipSuccess) e = hipMemcpy(h, d, sizeof(double) * kSelftestDoubles, hipMemcpyDeviceToHost);
  (void)dev_free(d);
  if (e != hipSuccess) return fail_hip(e, "selftest_kernel");
  for (int i = 0; i < kWave; ++i)
    if (h[i] != 89440.0) {
      char buf[128];
      std::snprintf(buf, sizeof(buf), "wave_allreduce_sum: lane %d holds %.17g, expected 89440", i, h[i]);
      return fail(PNEC_HIP_ERR_HIP_RUNTIME, buf);
    }
  if (!(h[64] >= 0.0 && h[64] < 1e-12)) return fail(PNEC_HIP_ERR_HIP_RUNTIME, "chol_solve5 residual too large");
  for (int i = 0; i < kWave; ++i) {
    char buf[160];
    if (!(h[216 + i] >= 0.0 && h[216 + i] < 1e-13)) {
      std::snprintf(buf, sizeof(buf), "gj_solve5_rows: lane %d deviates from chol_solve5 by %.3g (relative)", i, h[216 + i]);
      return fail(PNEC_HIP_ERR_HIP_RUNTIME, buf);
    }
    if (h[280 + i] != 1011.0 + 16.0 * (i / 16)) {
      std::snprintf(buf, sizeof(buf), "bcast_row<11>: lane %d holds %.17g", i, h[280 + i]);
      return fail(PNEC_HIP_ERR_HIP_RUNTIME, buf);
    }
  }
  if (!(std::abs(h[65]) < 1e-15)) return fail(PNEC_HIP_ERR_HIP_RUNTIME, "fast_rsqrt inaccurate");
  if (!(std::abs(h[66]) < 1e-15)) return fail(PNEC_HIP_ERR_HIP_RUNTIME, "fast_rcp inaccurate");
  for (int j = 0; j < kNumAcc; ++j)
    if (h[67 + j] != 2080.0 * (j + 1) + 64.0 * j) {
      char buf[128];
      std::snprintf(buf, sizeof(buf), "wave_reduce21: sum %d is %.17g, expected %.17g", j, h[67 + j],
                    2080.0 * (j + 1) + 64.0 * j);
      return fail(PNEC_HIP_ERR_HIP_RUNTIME, buf);
    }
  for (int i = 0; i < kWave; ++i)
    if (!(h[88 + i] < 4e-16)) {
      char buf[128];
      std::snprintf(buf, sizeof(buf), "sincos_bounded deviates from libm by %.3g", h[88 + i]);
      return fail(PNEC_HIP_ERR_HIP_RUNTIME, buf);
    }
  for (int i = 0; i < kWave; ++i)
    if (!(h[152 + i] < 9e-16)) {
      char buf[128];
      std::snprintf(buf, sizeof(buf), "acos_lean / atan2_lean deviate from libm by %.3g", h[152 + i]);
      return fail(PNEC_HIP_ERR_HIP_RUNTIME, buf);
    }
  for (int i = 0; i < kAtan2Edges + kAcosEdges; ++i) {
    const bool is_atan2 = i < kAtan2Edges;
    const double want = is_atan2 ? std::atan2(kAtan2EdgeY[i], kAtan2EdgeX[i]) : std::acos(kAcosEdge[i - kAtan2Edges]);
    const double got = h[kEdgeOut + i];
    if (std::signbit(got) != std::signbit(want) || !(std::abs(got - want) <= 9e-16 * std::abs(want))) {
      char buf[192];
      if (is_atan2)
        std::snprintf(buf, sizeof(buf), "atan2_c(%.17g, %.17g) = %.17g, libm %.17g", kAtan2EdgeY[i], kAtan2EdgeX[i],
                      got, want);
      else
        std::snprintf(buf, sizeof(buf), "acos_lean(%.17g) = %.17g, libm %.17g", kAcosEdge[i - kAtan2Edges], got, want);
      return fail(PNEC_HIP_ERR_HIP_RUNTIME, buf);
    }
  }
  return 0;
}

}  // extern "C"
