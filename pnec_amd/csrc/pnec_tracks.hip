// pnec_tracks.hip -- the bookkeeping of tracks across frames: the surviving tracks of a tracking step, compacted
// (pnec_hip_tracks_retain), and the refill with new detections (pnec_hip_tracks_append); include/pnec_hip.h has the
// definitions, pnec_tracks.hpp the rules and the row copies.  A translation unit of its own.
//
// No allocation, no atomics, nothing read back: a row's position follows from counts and prefix sums, so the output is a
// function of the inputs alone.
//   retain  count   one wavefront per image walks its rows 64 at a time; the population count of the ballot of the
//                   retention rule is summed into out.offsets[f + 1].
//           scan    one block turns out.offsets into the exclusive scan over images (as pnec_detect.hip does).
//           emit    one wavefront per image walks its rows again: a retained row's position is out.offsets[f] + the
//                   running base + the number of retained lanes below it; the base grows by the ballot's count.
//           pad     one lane per row at and beyond out.offsets[n_images].
//   append  scan    the counts come from the two offset arrays alone: one block scans take_a + take_d into out.offsets
//                   and writes out_dropped.
//           emit    one lane per output row: its image by bisection of out.offsets, then a set row, a detection or padding.
//           bump    next_id[f] += take_d (its own kernel: emit reads next_id).
// Every ballot and barrier runs with all lanes of the wavefront (block) active: a lane without a row carries a false
// predicate, a wavefront past the last image walks nothing.  No kernel reads a word that a lane of the same kernel writes.
#include <hip/hip_runtime.h>

#include "pnec_tracks.hpp"

namespace pnec_hip {

__global__ __launch_bounds__(kTracksBlock) void tracks_retain_count_kernel(const TracksRetainArgs a) {
  const int wave = threadIdx.x / kTracksLanes, lane = threadIdx.x & (kTracksLanes - 1);
  const int64_t f = (int64_t)blockIdx.x * kTracksWaves + wave;
  const bool inside = f < a.n_images;
  int64_t lo = 0, hi = 0;
  if (inside) tracks_range(a.in.offsets, f, a.in.n_rows, lo, hi);   // (wavefront-uniform)
  int64_t sum = 0;
  for (int64_t base = lo; base < hi; base += kTracksLanes) {
    const int64_t k = base + lane;
    const bool keep = k < hi && tracks_keep(a.in.id[k], a.trk_status[k], a.in.age[k], a.max_age);
    sum += tracks_popcount(__builtin_amdgcn_ballot_w64(keep));
  }
  if (inside && lane == 0) a.out.offsets[f + 1] = sum;
}

__global__ __launch_bounds__(256) void tracks_retain_scan_kernel(const TracksRetainArgs a) {
  const int64_t *counts = a.out.offsets;   // (each count is read by the lane that then overwrites it)
  tracks_block_scan(a.out.offsets, a.n_images, [&](int64_t f) { return counts[f + 1]; });
}

__global__ __launch_bounds__(kTracksBlock) void tracks_retain_emit_kernel(const TracksRetainArgs a) {
  const int wave = threadIdx.x / kTracksLanes, lane = threadIdx.x & (kTracksLanes - 1);
  const int64_t f = (int64_t)blockIdx.x * kTracksWaves + wave;
  const bool inside = f < a.n_images;
  int64_t lo = 0, hi = 0;
  if (inside) tracks_range(a.in.offsets, f, a.in.n_rows, lo, hi);
  int64_t at0 = inside ? a.out.offsets[f] : 0;   // the running base
  for (int64_t base = lo; base < hi; base += kTracksLanes) {
    const int64_t k = base + lane;
    const bool keep = k < hi && tracks_keep(a.in.id[k], a.trk_status[k], a.in.age[k], a.max_age);
    const uint64_t ballot = __builtin_amdgcn_ballot_w64(keep);
    const int64_t at = at0 + tracks_rank(ballot, lane);
    // (at < n_rows whenever the images' ranges do not overlap; DEVICE space does not check that they do not)
    if (keep && at < a.in.n_rows) tracks_retain_row(a, k, at);
    at0 += tracks_popcount(ballot);
  }
}

__global__ __launch_bounds__(256) void tracks_retain_pad_kernel(const TracksRetainArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.in.n_rows || i < a.out.offsets[a.n_images]) return;
  tracks_pad_retained(a, i);
}

hipError_t launch_tracks_retain(const TracksRetainArgs &a, hipStream_t stream) {
  const int64_t image_blocks = (a.n_images + kTracksWaves - 1) / kTracksWaves, row_blocks = (a.in.n_rows + 255) / 256;
  if (image_blocks > 0x7fffffffLL || row_blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  const dim3 images((unsigned)image_blocks), wide((unsigned)kTracksBlock);
  hipLaunchKernelGGL(tracks_retain_count_kernel, images, wide, 0, stream, a);
  hipLaunchKernelGGL(tracks_retain_scan_kernel, dim3(1), dim3(256), 0, stream, a);
  hipLaunchKernelGGL(tracks_retain_emit_kernel, images, wide, 0, stream, a);
  if (row_blocks > 0) hipLaunchKernelGGL(tracks_retain_pad_kernel, dim3((unsigned)row_blocks), dim3(256), 0, stream, a);
  return hipGetLastError();
}

__global__ __launch_bounds__(256) void tracks_append_scan_kernel(const TracksAppendArgs a) {
  tracks_block_scan(a.out.offsets, a.n_images, [&](int64_t f) {
    int64_t lo_a, lo_d, n_a, n_d, take_a, take_d;
    tracks_append_counts(a, f, lo_a, lo_d, n_a, n_d, take_a, take_d);
    if (a.out_dropped) a.out_dropped[f] = (n_a - take_a) + (n_d - take_d);
    return take_a + take_d;
  });
}

__global__ __launch_bounds__(256) void tracks_append_emit_kernel(const TracksAppendArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n_out) return;
  tracks_append_row(a, i);
}

__global__ __launch_bounds__(256) void tracks_append_bump_kernel(const TracksAppendArgs a) {
  const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (f >= a.n_images) return;
  int64_t lo_a, lo_d, n_a, n_d, take_a, take_d;
  tracks_append_counts(a, f, lo_a, lo_d, n_a, n_d, take_a, take_d);
  a.next_id[f] += take_d;
}

hipError_t launch_tracks_append(const TracksAppendArgs &a, hipStream_t stream) {
  const int64_t image_blocks = (a.n_images + 255) / 256, row_blocks = (a.n_out + 255) / 256;
  if (image_blocks > 0x7fffffffLL || row_blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(tracks_append_scan_kernel, dim3(1), dim3(256), 0, stream, a);
  if (row_blocks > 0) hipLaunchKernelGGL(tracks_append_emit_kernel, dim3((unsigned)row_blocks), dim3(256), 0, stream, a);
  hipLaunchKernelGGL(tracks_append_bump_kernel, dim3((unsigned)image_blocks), dim3(256), 0, stream, a);
  return hipGetLastError();
}

}  // namespace pnec_hip
