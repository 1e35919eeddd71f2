// pnec_patch_track.hip -- patch tracking: the pyramidal SE(2) KLT iteration with its forward-backward check
// (pnec_hip_patch_track) and the pyramid's halving step (pnec_hip_image_pyramid_level); include/pnec_hip.h has the
// definitions, pnec_patch_track.hpp and pnec_patch_cov.hpp the arithmetic.  A translation unit of its own.
//
// The tracker keeps pnec_patch_cov.hip's geometry: 16 lanes -- one DPP row -- per keypoint, four keypoints per wavefront,
// 16 per block of 256 threads, pattern point i in lane i mod 16 of the row, slot i / 16.  Every sum is a
// row_allreduce_sum, so a keypoint's bits do not depend on its neighbours.  No LDS, no barrier, no atomics.
//
// Per (direction, level) the row rebuilds the template from the template pyramid (48 pixel loads per lane, as the
// covariance kernel's two phases) and keeps, per slot, the normalised value data_i and the gain K_i = H^-1 J_i' (24
// doubles per lane); the iterations then gather four pixels per point and run five row sums (S2, the two counts share
// one integer sum each, and the three components of the step).  The trip counts do not depend on the data except for
// loss: a lost row keeps running with its transform frozen and its stores masked, so that every DPP move runs with all
// lanes active, and the wavefront leaves its loops early only on a ballot that none of its four rows is alive.  Lanes past
// the last keypoint compute on the last keypoint and store nothing.
//
// The pyramid step is a plain streaming kernel: one output pixel per lane, lanes along x.
#include <hip/hip_runtime.h>

#include "pnec_device.hpp"
#include "pnec_patch_track.hpp"

namespace pnec_hip {

constexpr int kPyrBlock = 256;

template <typename T>
__global__ __launch_bounds__(kPyrBlock) void image_pyramid_level_kernel(const PyramidLevelArgs a) {
  const int32_t w2 = a.w / 2, h2 = a.h / 2;
  const int64_t idx = (int64_t)blockIdx.x * kPyrBlock + threadIdx.x;
  if (idx >= a.n_images * (int64_t)h2 * w2) return;
  const int32_t x = (int32_t)(idx % w2);
  const int64_t row = idx / w2;   // f * h2 + y
  const int32_t y = (int32_t)(row % h2);
  const int64_t f = row / h2;
  const T *img = reinterpret_cast<const T *>(a.in) + f * (int64_t)a.h * a.pitch_in;
  reinterpret_cast<T *>(a.out)[row * a.pitch_out + x] = pyr_pixel(img, a.pitch_in, a.w, a.h, x, y);
}

hipError_t launch_image_pyramid_level(int pixel_type, const PyramidLevelArgs &a, hipStream_t stream) {
  const int64_t pixels = a.n_images * (int64_t)(a.h / 2) * (a.w / 2);
  const int64_t blocks = (pixels + kPyrBlock - 1) / kPyrBlock;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  const dim3 grid((unsigned)blocks), block((unsigned)kPyrBlock);
  switch (pixel_type) {
    case PNEC_HIP_PIXEL_U8: hipLaunchKernelGGL(image_pyramid_level_kernel<uint8_t>, grid, block, 0, stream, a); break;
    case PNEC_HIP_PIXEL_U16: hipLaunchKernelGGL(image_pyramid_level_kernel<uint16_t>, grid, block, 0, stream, a); break;
    case PNEC_HIP_PIXEL_F32: hipLaunchKernelGGL(image_pyramid_level_kernel<float>, grid, block, 0, stream, a); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

template <typename T>
__global__ __launch_bounds__(kTrackBlock) void patch_track_kernel(const PatchTrackArgs a) {
#define PNEC_TRACK_TMPL_IMAGE f
#include "pnec_patch_track_kernel.inl"
#undef PNEC_TRACK_TMPL_IMAGE
}

// the index clamped to the images there are (DEVICE space checks nothing; HOST space has refused a bad one)
__device__ __forceinline__ int64_t track_tmpl_image(int32_t i, int64_t n) {
  return i < 0 ? 0 : ((int64_t)i > n - 1 ? n - 1 : (int64_t)i);
}

template <typename T>
__global__ __launch_bounds__(kTrackBlock) void patch_track_indexed_kernel(const PatchTrackArgs a,
                                                                          const int32_t *tmpl_image,
                                                                          const int64_t n_tmpl_images) {
#define PNEC_TRACK_TMPL_IMAGE track_tmpl_image(tmpl_image[k], n_tmpl_images)
#include "pnec_patch_track_kernel.inl"
#undef PNEC_TRACK_TMPL_IMAGE
}

hipError_t launch_patch_track(int pixel_type, const PatchTrackArgs &a, hipStream_t stream) {
  const int64_t blocks = (a.n_points * kPatchLanes + kTrackBlock - 1) / kTrackBlock;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  const dim3 grid((unsigned)blocks), block((unsigned)kTrackBlock);
  switch (pixel_type) {
    case PNEC_HIP_PIXEL_U8: hipLaunchKernelGGL(patch_track_kernel<uint8_t>, grid, block, 0, stream, a); break;
    case PNEC_HIP_PIXEL_U16: hipLaunchKernelGGL(patch_track_kernel<uint16_t>, grid, block, 0, stream, a); break;
    case PNEC_HIP_PIXEL_F32: hipLaunchKernelGGL(patch_track_kernel<float>, grid, block, 0, stream, a); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_patch_track_indexed(int pixel_type, const PatchTrackArgs &a, const int32_t *tmpl_image,
                                      int64_t n_tmpl_images, hipStream_t stream) {
  const int64_t blocks = (a.n_points * kPatchLanes + kTrackBlock - 1) / kTrackBlock;
  if (blocks > 0x7fffffffLL || !tmpl_image || n_tmpl_images < 1) return hipErrorInvalidValue;
  const dim3 grid((unsigned)blocks), block((unsigned)kTrackBlock);
  switch (pixel_type) {
    case PNEC_HIP_PIXEL_U8:
      hipLaunchKernelGGL(patch_track_indexed_kernel<uint8_t>, grid, block, 0, stream, a, tmpl_image, n_tmpl_images);
      break;
    case PNEC_HIP_PIXEL_U16:
      hipLaunchKernelGGL(patch_track_indexed_kernel<uint16_t>, grid, block, 0, stream, a, tmpl_image, n_tmpl_images);
      break;
    case PNEC_HIP_PIXEL_F32:
      hipLaunchKernelGGL(patch_track_indexed_kernel<float>, grid, block, 0, stream, a, tmpl_image, n_tmpl_images);
      break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace pnec_hip
