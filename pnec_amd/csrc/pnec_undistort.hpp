// pnec_undistort.hpp -- launch interface of the keypoint undistortion kernel (pnec_undistort.hip), shared with the ABI
// layer.  include/pnec_hip.h (pnec_hip_undistort_keypoints) has the definition in six numbered steps: normalise, the
// fixed-point inversion of the radial-tangential model, the Newton polish, back to pixels, the covariance, and the
// all-zero camera.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pnec_hip {

struct UndistortArgs {
  int64_t n_rows;
  // side 0 is frame 1 (pts1, cov1), side 1 is frame 2 (pts2, cov2); a NULL pts leaves its side out, a NULL cov its
  // covariance.  An output may be its own input (a row is read whole before it is written, by the lane that writes it).
  const double *pts[2];        // [n_rows,2] raw pixels
  const double *cov[2];        // [n_rows,3] (xx, xy, yy)
  const double *camera;        // [9] fx fy cx cy k1 k2 p1 p2 k3
  int32_t fixed_iterations, newton_iterations;
  uint32_t flags;              // PNEC_HIP_UNDISTORT_NEWTON | PNEC_HIP_UNDISTORT_PROPAGATE_COV
  double *out_pts[2];
  double *out_cov[2];
  uint8_t *out_status[2];      // [n_rows] or NULL
};

// one lane per row, 256 lanes a block; n_rows >= 1
hipError_t launch_undistort_keypoints(const UndistortArgs &a, hipStream_t stream);

constexpr double kUndistortStop = 0x1p-46;   // the Newton stop: rho <= kUndistortStop * max(1, |(x0, y0)|)

}  // namespace pnec_hip
