// pnec_tracks_link.hip -- the join of two track sets on their ids (pnec_hip_tracks_link): for every row of the current
// set the row, within the same image's range of the previous set, that holds the same id.  include/pnec_hip.h has the
// definition, pnec_tracks_link.hpp the row's work.  A translation unit of its own.
//
//   rows    one lane per row of the current set.  The lane finds its image by bisection of the cut offsets (at most 31
//           reads of an array that stays in L1 / L2), then bisects its image's previous ids: ceil(log2(Lp + 1)) dependent
//           8-byte reads plus the one that confirms the hit.  The ids of an image (a few KB to 16 KB) are read from
//           cache by every lane of that image; they are not staged in LDS: a block of 256 rows would load the whole
//           range to use 256 x 12 words of it, and neighbouring lanes' probes already share lines for the first steps.
//           Rows outside every image (padding) get -1.
//   counts  one wavefront per image walks its rows of out_link 64 at a time and adds the population counts of the
//           ballots: no atomic, an order fixed by the image's own rows.  Launched only when out_n_linked is wanted.
// No allocation, nothing read back, plain vector stores.  Every ballot runs with all lanes of the wavefront active.
#include <hip/hip_runtime.h>

#include "pnec_tracks_link.hpp"

namespace pnec_hip {

__global__ __launch_bounds__(kTracksLinkBlock) void tracks_link_rows_kernel(const TracksLinkArgs a) {
  const int64_t k = (int64_t)blockIdx.x * kTracksLinkBlock + threadIdx.x;
  if (k >= a.n_cur) return;
  a.out_link[k] = tracks_link_row(a, k);
}

__global__ __launch_bounds__(kTracksBlock) void tracks_link_count_kernel(const TracksLinkArgs a) {
  const int wave = threadIdx.x / kTracksLanes, lane = threadIdx.x & (kTracksLanes - 1);
  const int64_t f = (int64_t)blockIdx.x * kTracksWaves + wave;
  const bool inside = f < a.n_images;
  int64_t lo = 0, hi = 0;
  if (inside) tracks_range(a.cur_offsets, f, a.n_cur, lo, hi);   // (wavefront-uniform)
  int64_t sum = 0;
  for (int64_t base = lo; base < hi; base += kTracksLanes) {
    const int64_t k = base + lane;
    const bool linked = k < hi && a.out_link[k] >= 0;
    sum += tracks_popcount(__builtin_amdgcn_ballot_w64(linked));
  }
  if (inside && lane == 0) a.out_n_linked[f] = (int32_t)sum;   // (sum <= n_cur <= 2^31 - 1)
}

hipError_t launch_tracks_link(const TracksLinkArgs &a, hipStream_t stream) {
  const int64_t row_blocks = (a.n_cur + kTracksLinkBlock - 1) / kTracksLinkBlock;
  const int64_t image_blocks = (a.n_images + kTracksWaves - 1) / kTracksWaves;
  if (a.n_cur < 1 || row_blocks > 0x7fffffffLL || image_blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(tracks_link_rows_kernel, dim3((unsigned)row_blocks), dim3(kTracksLinkBlock), 0, stream, a);
  if (a.out_n_linked)
    hipLaunchKernelGGL(tracks_link_count_kernel, dim3((unsigned)image_blocks), dim3(kTracksBlock), 0, stream, a);
  return hipGetLastError();
}

}  // namespace pnec_hip
