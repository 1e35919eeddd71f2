// pnec_undistort.hip -- keypoint undistortion (pnec_hip_undistort_keypoints): the radial-tangential lens model inverted
// per tracked point, between the tracker and the keypoint ingest; include/pnec_hip.h has the definition in six steps and
// this file follows their operation order.  A translation unit of its own.
//
// One lane per row: the lane reads the row's two points and their covariances (two and three 8-byte loads at strides of
// 16 and 24 bytes: a wavefront's loads of one array cover one contiguous run of 1 KiB / 1.5 KiB between them, so every
// cache line fetched is used whole), inverts the model for each point and writes the row.  The camera's nine doubles are
// read at a uniform address.  Plain vector stores, no atomics, no LDS.
//
// A row's bits depend on the row, the camera and the call's scalars alone:
//   * floating-point contraction is off in this file, so every product and sum is rounded where the header writes it
//     and no fused multiply-add is formed -- the numpy checker of the tests follows the same order;
//   * the fixed-point and Newton loops have wavefront-uniform trip counts; a lane that has finished (outside the model,
//     converged, singular Jacobian, no row) keeps its values by select and goes on computing values nobody reads.  The
//     Newton loop leaves early only when every lane of the wavefront has finished, which changes no lane's values.
// Every ballot runs with all 64 lanes active: no lane returns early, a lane beyond n_rows loads and stores nothing.
#include <hip/hip_runtime.h>

#include "pnec_hip.h"
#include "pnec_undistort.hpp"

#pragma clang fp contract(off)

namespace pnec_hip {
namespace {

constexpr int kUndistortBlock = 256;

struct UndistortCamera {
  double fx, fy, cx, cy, k1, k2, p1, p2, k3;
};

// the forward model at (x, y): the distorted point, and with J the analytic Jacobian (j00 j01; j10 j11)
template <bool kJacobian>
__device__ __forceinline__ void undistort_forward(const UndistortCamera &c, double x, double y, double &xd, double &yd,
                                                  double *J) {
  const double xx = x * x, yy = y * y, xy = x * y;
  const double r2 = xx + yy;
  const double cdist = 1.0 + ((c.k3 * r2 + c.k2) * r2 + c.k1) * r2;
  const double a1 = 2.0 * xy, a2 = r2 + 2.0 * xx, a3 = r2 + 2.0 * yy;
  xd = x * cdist + (c.p1 * a1 + c.p2 * a2);
  yd = y * cdist + (c.p1 * a3 + c.p2 * a1);
  if constexpr (kJacobian) {
    const double dc = (3.0 * c.k3 * r2 + 2.0 * c.k2) * r2 + c.k1;   // d cdist / d r2
    const double cross = 2.0 * xy * dc + (2.0 * c.p1 * x + 2.0 * c.p2 * y);
    J[0] = cdist + 2.0 * xx * dc + (2.0 * c.p1 * y + 6.0 * c.p2 * x);
    J[1] = cross;
    J[2] = cross;
    J[3] = cdist + 2.0 * yy * dc + (6.0 * c.p1 * y + 2.0 * c.p2 * x);
  }
}

__device__ __forceinline__ bool undistort_finite(double x) { return __builtin_fabs(x) <= 0x1.fffffffffffffp1023; }

}  // namespace

__global__ __launch_bounds__(kUndistortBlock) void undistort_keypoints_kernel(const UndistortArgs a) {
  const int64_t i = (int64_t)blockIdx.x * kUndistortBlock + threadIdx.x;
  const bool live = i < a.n_rows;
  const double *__restrict__ cam = a.camera;
  const UndistortCamera c{cam[0], cam[1], cam[2], cam[3], cam[4], cam[5], cam[6], cam[7], cam[8]};
  // step 6 (wavefront-uniform: the camera is the call's)
  const bool identity = c.k1 == 0.0 && c.k2 == 0.0 && c.p1 == 0.0 && c.p2 == 0.0 && c.k3 == 0.0;
  const bool newton = (a.flags & PNEC_HIP_UNDISTORT_NEWTON) != 0, propagate = (a.flags & PNEC_HIP_UNDISTORT_PROPAGATE_COV) != 0;

  for (int side = 0; side < 2; ++side) {
    const double *pts = a.pts[side], *cov = a.cov[side];
    if (!pts) continue;
    double u = 0.0, v = 0.0, sxx = 0.0, sxy = 0.0, syy = 0.0;
    if (live) {
      u = pts[2 * i];
      v = pts[2 * i + 1];
      if (cov) {
        sxx = cov[3 * i];
        sxy = cov[3 * i + 1];
        syy = cov[3 * i + 2];
      }
    }
    double ou = u, ov = v, oxx = sxx, oxy = sxy, oyy = syy;
    uint8_t status = PNEC_HIP_UNDISTORT_OK;
    if (!identity) {
      // 1 normalise
      const bool finite = undistort_finite(u) && undistort_finite(v);
      const double x0 = (u - c.cx) / c.fx, y0 = (v - c.cy) / c.fy;
      // 2 fixed point
      double x = x0, y = y0;
      bool outside = false;
      for (int it = 0; it < a.fixed_iterations; ++it) {
        const double xx = x * x, yy = y * y, xy = x * y;
        const double r2 = xx + yy;
        const double icdist = 1.0 / (1.0 + ((c.k3 * r2 + c.k2) * r2 + c.k1) * r2);
        outside = outside || icdist < 0.0;
        const double a1 = 2.0 * xy, a2 = r2 + 2.0 * xx, a3 = r2 + 2.0 * yy;
        const double dx = c.p1 * a1 + c.p2 * a2, dy = c.p1 * a3 + c.p2 * a1;
        const double xn = (x0 - dx) * icdist, yn = (y0 - dy) * icdist;
        x = outside ? x0 : xn;
        y = outside ? y0 : yn;
      }
      status = outside ? PNEC_HIP_UNDISTORT_OUTSIDE : PNEC_HIP_UNDISTORT_OK;
      // 3 Newton
      if (newton) {
        const double n0 = __builtin_sqrt(x0 * x0 + y0 * y0);
        const double bound = kUndistortStop * (n0 > 1.0 ? n0 : 1.0);
        double xn = x, yn = y;
        bool ended = !live || !finite || outside, converged = false;
        for (int it = 0;; ++it) {
          double xd, yd, J[4];
          undistort_forward<true>(c, xn, yn, xd, yd, J);
          const double e0 = xd - x0, e1 = yd - y0;
          const double rho = __builtin_sqrt(e0 * e0 + e1 * e1);
          const bool stop = !ended && rho <= bound;
          converged = converged || stop;
          ended = ended || stop;
          if (it >= a.newton_iterations) break;                        // (uniform)
          if (__builtin_amdgcn_ballot_w64(!ended) == 0) break;         // (uniform: every lane has finished)
          const double det = J[0] * J[3] - J[1] * J[2];
          ended = ended || det == 0.0 || !undistort_finite(det);
          const double sx = (J[3] * e0 - J[1] * e1) / det, sy = (J[0] * e1 - J[2] * e0) / det;
          xn = ended ? xn : xn - sx;
          yn = ended ? yn : yn - sy;
        }
        x = converged ? xn : x;
        y = converged ? yn : y;
        if (!outside && !converged) status = PNEC_HIP_UNDISTORT_NOT_CONVERGED;
      }
      // 4 back to pixels
      ou = c.fx * x + c.cx;
      ov = c.fy * y + c.cy;
      if (!finite) {
        ou = ov = __builtin_nan("");
        status = PNEC_HIP_UNDISTORT_NOT_FINITE;
      }
      // 5 covariance
      if (propagate && cov) {
        double xd, yd, J[4];
        undistort_forward<true>(c, x, y, xd, yd, J);
        const double det = J[0] * J[3] - J[1] * J[2];
        const double a00 = J[3] / det, a01 = -J[1] / det * c.fx / c.fy;
        const double a10 = -J[2] / det * c.fy / c.fx, a11 = J[0] / det;
        const double m00 = a00 * sxx + a01 * sxy, m01 = a00 * sxy + a01 * syy;
        const double m10 = a10 * sxx + a11 * sxy, m11 = a10 * sxy + a11 * syy;
        const bool carry = status == PNEC_HIP_UNDISTORT_OK && det != 0.0 && undistort_finite(det);
        oxx = carry ? m00 * a00 + m01 * a01 : sxx;
        oxy = carry ? m00 * a10 + m01 * a11 : sxy;
        oyy = carry ? m10 * a10 + m11 * a11 : syy;
      }
    }
    if (live) {
      double *out_pts = a.out_pts[side], *out_cov = a.out_cov[side];
      uint8_t *out_status = a.out_status[side];
      out_pts[2 * i] = ou;
      out_pts[2 * i + 1] = ov;
      if (cov) {
        out_cov[3 * i] = oxx;
        out_cov[3 * i + 1] = oxy;
        out_cov[3 * i + 2] = oyy;
      }
      if (out_status) out_status[i] = status;
    }
  }
}

hipError_t launch_undistort_keypoints(const UndistortArgs &a, hipStream_t stream) {
  const int64_t blocks = (a.n_rows + kUndistortBlock - 1) / kUndistortBlock;
  if (blocks < 1 || blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(undistort_keypoints_kernel, dim3((unsigned)blocks), dim3(kUndistortBlock), 0, stream, a);
  return hipGetLastError();
}

}  // namespace pnec_hip
