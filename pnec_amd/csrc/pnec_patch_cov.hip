// pnec_patch_cov.hip -- patch covariances: the 2x2 image covariance of every keypoint from the image patch around it
// (pnec_hip_patch_covariance; include/pnec_hip.h has the definition, pnec_patch_cov.hpp the arithmetic).  A translation
// unit of its own.
//
// Geometry: 16 lanes -- one DPP row -- per keypoint, four keypoints per wavefront, 16 per block of 256 threads.  Pattern
// point i belongs to lane i mod 16 of the row, slot i / 16 (four slots: 64 points).  Why not one lane per point and a
// wavefront per keypoint: both forms keep 52 of 64 point-lanes busy on Pattern52 and issue the same gathers, but nine
// sums per keypoint (S, Gx, Gy, then the six of H) cross lanes, and a 64-lane sum is six levels, two of them
// v_permlane*_swap, per KEYPOINT, where the row form adds three of four points inside the lane for free and then runs
// four DPP levels (row_allreduce_sum) for FOUR keypoints at once: a sixth of the cross-lane instructions.  A row's sums
// never leave the row, so a keypoint's bits do not depend on its neighbours in the wavefront.
//
// Two phases, values held in registers (12 doubles per lane): phase 1 gathers the twelve pixels of each of the lane's
// points (plain per-lane vector loads; neighbouring pattern points share cache lines, nothing is coalesced across
// keypoints) and sums d, gx, gy and the count; phase 2 forms g'_i, which needs S and G, and sums the six products.  Every
// lane of the row then holds the same nine sums and runs the epilogue redundantly (it is SIMD either way); lanes 0..5
// store.  No LDS, no barrier, no atomics.  Lanes past the last keypoint compute on the last keypoint and store nothing,
// so every cross-lane move runs with all lanes active.
//
// The image of a keypoint: offsets[f] <= k < offsets[f+1].  One probe at f = k * n_images / n_points (exact when the
// images have equally many keypoints), a binary search otherwise; the result is clamped to the images there are.
#include <hip/hip_runtime.h>

#include "pnec_device.hpp"
#include "pnec_patch_cov.hpp"

namespace pnec_hip {

constexpr int kPatchBlock = 256;

__device__ __forceinline__ int row_allreduce_sum_i(int x) {
  x += __builtin_amdgcn_mov_dpp(x, 0xB1, 0xF, 0xF, true);    // quad_perm [1,0,3,2]
  x += __builtin_amdgcn_mov_dpp(x, 0x4E, 0xF, 0xF, true);    // quad_perm [2,3,0,1]
  x += __builtin_amdgcn_mov_dpp(x, 0x141, 0xF, 0xF, true);   // row_half_mirror
  x += __builtin_amdgcn_mov_dpp(x, 0x140, 0xF, 0xF, true);   // row_mirror
  return x;
}

template <typename T>
__global__ __launch_bounds__(kPatchBlock) void patch_covariance_kernel(const PatchCovArgs a) {
  const int64_t g = ((int64_t)blockIdx.x * kPatchBlock + threadIdx.x) / kPatchLanes;
  const int j = threadIdx.x & (kPatchLanes - 1);
  const bool live = g < a.n_points;
  const int64_t k = live ? g : a.n_points - 1;   // (n_points >= 1: the ABI layer launches nothing otherwise)

  // which image
  const int64_t F = a.n_images;
  int64_t f = (int64_t)((double)k * (double)F / (double)a.n_points);
  f = f < 0 ? 0 : (f > F - 1 ? F - 1 : f);
  if (!(a.offsets[f] <= k && k < a.offsets[f + 1])) {
    int64_t lo = 0, hi = F - 1;   // the last f in [0, F-1] with offsets[f] <= k
    while (lo < hi) {
      const int64_t mid = (lo + hi + 1) >> 1;
      if (a.offsets[mid] <= k) lo = mid; else hi = mid - 1;
    }
    f = lo;
  }
  const T *img = reinterpret_cast<const T *>(a.images) + f * (int64_t)a.h * a.pitch;
  const double px = a.pts[2 * k], py = a.pts[2 * k + 1];

  // phase 1
  double d[kPatchSlots], gx[kPatchSlots], gy[kPatchSlots], patx[kPatchSlots], paty[kPatchSlots];
  bool valid[kPatchSlots];
  double S = 0.0, Gx = 0.0, Gy = 0.0;
  int cnt = 0;
#pragma unroll
  for (int s = 0; s < kPatchSlots; ++s) {
    const int i = j + kPatchLanes * s;
    const bool has = i < a.n_pattern;
    patx[s] = has ? a.pattern[2 * i] : 0.0;
    paty[s] = has ? a.pattern[2 * i + 1] : 0.0;
    valid[s] = false;
    d[s] = 0.0;
    gx[s] = 0.0;
    gy[s] = 0.0;
    if (has) valid[s] = patch_point(img, a.pitch, a.w, a.h, px + patx[s], py + paty[s], d[s], gx[s], gy[s]);
    S += d[s];
    Gx += gx[s];
    Gy += gy[s];
    cnt += valid[s] ? 1 : 0;
  }
  S = row_allreduce_sum(S);
  Gx = row_allreduce_sum(Gx);
  Gy = row_allreduce_sum(Gy);
  const int n = row_allreduce_sum_i(cnt);

  // phase 2
  const double nd = (double)n;
  double H[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int s = 0; s < kPatchSlots; ++s) {
    const double gpx = valid[s] ? patch_normalised_gradient(nd, gx[s], S, Gx, d[s]) : 0.0;
    const double gpy = valid[s] ? patch_normalised_gradient(nd, gy[s], S, Gy, d[s]) : 0.0;
    patch_accumulate(gpx, gpy, patx[s], paty[s], H);
  }
#pragma unroll
  for (int c = 0; c < 6; ++c) H[c] = row_allreduce_sum(H[c]);

  double cs = 1.0, sn = 0.0;
  if (a.angle) sincos_bounded(a.angle[k], sn, cs);
  double cov[3], Hs[6], mean;
  const int status = patch_epilogue(n, S, H, a.scaling, cs, sn, cov, Hs, mean);

  if (live) {
    if (a.out_cov && j < 3) a.out_cov[3 * k + j] = j == 0 ? cov[0] : (j == 1 ? cov[1] : cov[2]);
    if (a.out_hessian && j < 6) {
      const double v01 = j == 0 ? Hs[0] : Hs[1], v23 = j == 2 ? Hs[2] : Hs[3], v45 = j == 4 ? Hs[4] : Hs[5];
      a.out_hessian[6 * k + j] = j < 2 ? v01 : (j < 4 ? v23 : v45);
    }
    if (j == 0) {
      if (a.out_mean) a.out_mean[k] = mean;
      if (a.out_n_valid) a.out_n_valid[k] = n;
      if (a.out_status) a.out_status[k] = status;
    }
  }
}

hipError_t launch_patch_covariance(int pixel_type, const PatchCovArgs &a, hipStream_t stream) {
  const int64_t blocks = (a.n_points * kPatchLanes + kPatchBlock - 1) / kPatchBlock;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  const dim3 grid((unsigned)blocks), block((unsigned)kPatchBlock);
  switch (pixel_type) {
    case PNEC_HIP_PIXEL_U8: hipLaunchKernelGGL(patch_covariance_kernel<uint8_t>, grid, block, 0, stream, a); break;
    case PNEC_HIP_PIXEL_U16: hipLaunchKernelGGL(patch_covariance_kernel<uint16_t>, grid, block, 0, stream, a); break;
    case PNEC_HIP_PIXEL_F32: hipLaunchKernelGGL(patch_covariance_kernel<float>, grid, block, 0, stream, a); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace pnec_hip
