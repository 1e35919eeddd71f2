// pnec_keyframe.hip -- keyframe pairs (pnec_hip_tracks_keyframe): which images moved enough against their key frame,
// their matches compacted, and the per-track state of the next step; include/pnec_hip.h has the definition,
// pnec_keyframe.hpp the rules and the row copies.  A translation unit of its own.
//
// No allocation, no atomics, nothing read back: a row's position follows from counts and prefix sums, and the
// displacement sum has a fixed order, so the output is a function of the inputs alone.
//   count        one wavefront per image walks its retained rows 64 at a time: the population count of the ballot of the
//                match predicate, and per lane the sum of its matches' displacements (rows lane, lane + 64, ...); a tree
//                over the lanes (32, 16, .. 1) gives the sum.  Lane 0 writes n_matches, mean, accepted, next_span and the
//                image's pair count into out_offsets[f + 1].
//   scan         one block turns out_offsets into the exclusive scan over images.
//   emit         one wavefront per accepted image walks its rows again: a match's position is out_offsets[f] + the running
//                base + the number of matching lanes below it.  A skipped image walks nothing.
//   state + pad  one lane per row of A' writes the next state (its image by bisection of A's offsets), and one lane per
//                pair row at and beyond out_offsets[n_images] the padding.
// Every ballot, lane exchange and barrier runs with all lanes of the wavefront (block) active: a lane without a row
// carries a false predicate, a wavefront past the last image walks nothing.  No kernel reads a word that a lane of the
// same kernel writes: `accepted` travels as next_span == 0, written by count and read by the launches after it.
#include <hip/hip_runtime.h>

#include "pnec_keyframe.hpp"

namespace pnec_hip {

__global__ __launch_bounds__(kTracksBlock) void tracks_keyframe_count_kernel(const KeyframeArgs a) {
  const int wave = threadIdx.x / kTracksLanes, lane = threadIdx.x & (kTracksLanes - 1);
  const int64_t f = (int64_t)blockIdx.x * kTracksWaves + wave;
  const bool inside = f < a.n_images;
  int64_t lo = 0, hi = 0;
  if (inside) tracks_range(a.offsets, f, a.n_rows, lo, hi);   // (wavefront-uniform)
  int64_t n = 0;
  double part = 0.0;
  for (int64_t base = lo; base < hi; base += kTracksLanes) {
    const int64_t k = base + lane;
    double d = 0.0;
    const bool match = k < hi && keyframe_match(a, k, d);
    n += tracks_popcount(__builtin_amdgcn_ballot_w64(match));
    if (match) part += d;
  }
  for (int s = kTracksLanes / 2; s >= 1; s >>= 1) {
    // (lane + s > 63 reads itself: keyframe_tree_peer)
    const double other = __shfl(part, keyframe_tree_peer(lane, s), kTracksLanes);
    part = keyframe_tree_step(part, other);
  }
  if (inside && lane == 0) keyframe_decide(a, f, n, part);
}

__global__ __launch_bounds__(256) void tracks_keyframe_scan_kernel(const KeyframeArgs a) {
  const int64_t *counts = a.out_offsets;   // (each count is read by the lane that then overwrites it)
  tracks_block_scan(a.out_offsets, a.n_images, [&](int64_t f) { return counts[f + 1]; });
}

__global__ __launch_bounds__(kTracksBlock) void tracks_keyframe_emit_kernel(const KeyframeArgs a) {
  const int wave = threadIdx.x / kTracksLanes, lane = threadIdx.x & (kTracksLanes - 1);
  const int64_t f = (int64_t)blockIdx.x * kTracksWaves + wave;
  const bool inside = f < a.n_images;
  int64_t lo = 0, hi = 0;
  if (inside && keyframe_accepted(a, f)) tracks_range(a.offsets, f, a.n_rows, lo, hi);
  int64_t at0 = inside ? a.out_offsets[f] : 0;   // the running base
  for (int64_t base = lo; base < hi; base += kTracksLanes) {
    const int64_t k = base + lane;
    double d = 0.0;
    const bool match = k < hi && keyframe_match(a, k, d);
    const uint64_t ballot = __builtin_amdgcn_ballot_w64(match);
    const int64_t at = at0 + tracks_rank(ballot, lane);
    // (at < n_rows whenever the images' ranges do not overlap; DEVICE space does not check that they do not)
    if (match && at >= 0 && at < a.n_rows) keyframe_pair_row(a, k, at);
    at0 += tracks_popcount(ballot);
  }
}

__global__ __launch_bounds__(256) void tracks_keyframe_state_kernel(const KeyframeArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < a.n_new) keyframe_state_row(a, i);
  if (i < a.n_rows && i >= a.out_offsets[a.n_images]) keyframe_pad_pair(a, i);
}

hipError_t launch_tracks_keyframe(const KeyframeArgs &a, hipStream_t stream) {
  const int64_t rows = a.n_new > a.n_rows ? a.n_new : a.n_rows;
  const int64_t image_blocks = (a.n_images + kTracksWaves - 1) / kTracksWaves, row_blocks = (rows + 255) / 256;
  if (image_blocks > 0x7fffffffLL || row_blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  const dim3 images((unsigned)image_blocks), wide((unsigned)kTracksBlock);
  hipLaunchKernelGGL(tracks_keyframe_count_kernel, images, wide, 0, stream, a);
  hipLaunchKernelGGL(tracks_keyframe_scan_kernel, dim3(1), dim3(256), 0, stream, a);
  if (a.n_rows > 0) hipLaunchKernelGGL(tracks_keyframe_emit_kernel, images, wide, 0, stream, a);
  if (row_blocks > 0) hipLaunchKernelGGL(tracks_keyframe_state_kernel, dim3((unsigned)row_blocks), dim3(256), 0, stream, a);
  return hipGetLastError();
}

}  // namespace pnec_hip
