// pnec_patch_cov.hpp -- patch covariances (pnec_hip_patch_covariance): launch interface of pnec_patch_cov.hip, shared
// with the ABI layer, and the two functions that hold the arithmetic -- one pattern point (interpolation + gradient) and
// one keypoint's epilogue (Hessian -> covariance) -- written so that they also compile for the host
// (tools/patch_cov_host.cc runs them under the address sanitizer on images without slack before any device does).
// include/pnec_hip.h has the definition.
#pragma once

#include <math.h>
#include <stdint.h>

#include "pnec_hip.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PNEC_PATCH_HD __host__ __device__ __forceinline__
#else
#define PNEC_PATCH_HD inline
#endif
// No product is fused into a following sum in these functions: which products the compiler would fuse differs between
// the kernel's three instances (one per pixel type), and a keypoint's bits must not depend on the pixel type its image
// is stored in, nor on the compiler's mood.  (The statement opens each function body; other compilers do not fuse
// without being told to.)
#if defined(__clang__)
#define PNEC_PATCH_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define PNEC_PATCH_NO_CONTRACT
#endif

namespace pnec_hip {

// Geometry: 16 lanes -- one DPP row -- per keypoint, four keypoints per wavefront, four pattern points per lane
// (point i sits in lane i mod 16, slot i / 16): 16 x 4 = PNEC_HIP_PATCH_MAX_POINTS.
constexpr int kPatchLanes = 16;
constexpr int kPatchSlots = 4;
static_assert(kPatchLanes * kPatchSlots == PNEC_HIP_PATCH_MAX_POINTS, "a row of lanes holds a whole pattern");

// One pattern point at p = (px, py) of an image whose first pixel is `img` (rows `pitch` elements apart): value and
// central-difference gradient of the bilinear interpolant (basalt's interpGrad [EXT]).  False -- and zeros -- when the
// point is not valid; a valid point reads the twelve pixels of rows iy-1 .. iy+2, columns ix-1 .. ix+2 without the four
// corners, and 2 <= p < size - 3 keeps all of them at least one pixel inside the image.
template <typename T>
PNEC_PATCH_HD bool patch_point(const T *img, int64_t pitch, int32_t w, int32_t h, double px, double py, double &d,
                               double &gx, double &gy) {
  PNEC_PATCH_NO_CONTRACT
  d = 0.0;
  gx = 0.0;
  gy = 0.0;
  // (written so that a NaN fails)
  if (!(px >= 2.0 && px < (double)w - 3.0 && py >= 2.0 && py < (double)h - 3.0)) return false;
  const double fx = floor(px), fy = floor(py);
  const int32_t ix = (int32_t)fx, iy = (int32_t)fy;
  const double dx = px - fx, dy = py - fy, ddx = 1.0 - dx, ddy = 1.0 - dy;
  const double w00 = ddx * ddy, w01 = ddx * dy, w10 = dx * ddy, w11 = dx * dy;
  const T *r0 = img + ((int64_t)(iy - 1) * pitch + ix);   // (ix, iy-1)
  const T *r1 = r0 + pitch, *r2 = r1 + pitch, *r3 = r2 + pitch;
  const double a0 = (double)r0[0], a1 = (double)r0[1];
  const double bm = (double)r1[-1], b0 = (double)r1[0], b1 = (double)r1[1], b2 = (double)r1[2];
  const double cm = (double)r2[-1], c0 = (double)r2[0], c1 = (double)r2[1], c2 = (double)r2[2];
  const double e0 = (double)r3[0], e1 = (double)r3[1];
  // B(u, v) = ((w00 I(u,v) + w01 I(u,v+1)) + w10 I(u+1,v)) + w11 I(u+1,v+1)
  d = ((w00 * b0 + w01 * c0) + w10 * b1) + w11 * c1;
  const double bxp = ((w00 * b1 + w01 * c1) + w10 * b2) + w11 * c2;
  const double bxm = ((w00 * bm + w01 * cm) + w10 * b0) + w11 * c0;
  const double byp = ((w00 * c0 + w01 * e0) + w10 * c1) + w11 * e1;
  const double bym = ((w00 * a0 + w01 * b0) + w10 * a1) + w11 * b1;
  gx = 0.5 * (bxp - bxm);
  gy = 0.5 * (byp - bym);
  return true;
}

// g'_i = n (g_i S - G d_i) / S^2 (pnec_patch.h:114-115), one component
PNEC_PATCH_HD double patch_normalised_gradient(double n, double g, double S, double G, double d) {
  PNEC_PATCH_NO_CONTRACT
  return n * (g * S - G * d) / (S * S);
}

// Adds J_i' J_i of one point to the six sums (00 01 02 11 12 22); J_i = (gpx, gpy, -pat_y gpx + pat_x gpy)
PNEC_PATCH_HD void patch_accumulate(double gpx, double gpy, double pat_x, double pat_y, double (&H)[6]) {
  PNEC_PATCH_NO_CONTRACT
  const double r = -pat_y * gpx + pat_x * gpy;
  H[0] += gpx * gpx;
  H[1] += gpx * gpy;
  H[2] += gpx * r;
  H[3] += gpy * gpy;
  H[4] += gpy * r;
  H[5] += r * r;
}

// One keypoint's epilogue.  n valid points, S = sum d, H the six sums; (c, s) = (cos, sin) of the angle, (1, 0) for none.
// Writes cov (xx, xy, yy) = (H^-1)[0:2,0:2] / scaling rotated, Hs = H * scaling, mean = S / n; returns the status.
// The inverse comes from the Cholesky factor of the Jacobi-scaled matrix diag(H)^-1/2 H diag(H)^-1/2 (unit diagonal: the
// pivots are those of a correlation matrix whatever the contrast of the patch); a zero or negative diagonal makes its
// scale infinite or NaN, the pivot NaN, and `pivot > 0` false; fewer than three valid points are singular by count.
// With (c, s) = (1, 0) the rotation returns its input's bits (x * 1 - y * 0 is x for finite x, y, fused or not).
PNEC_PATCH_HD int patch_epilogue(int n, double S, const double (&H)[6], double scaling, double c, double s,
                                 double (&cov)[3], double (&Hs)[6], double &mean) {
  PNEC_PATCH_NO_CONTRACT
  const double nan = (double)NAN;
  for (int k = 0; k < 6; ++k) Hs[k] = H[k] * scaling;
  mean = S / (double)n;
  cov[0] = nan;
  cov[1] = nan;
  cov[2] = nan;
  if (n == 0 || !(S > 0.0) || !(S <= 1.7976931348623157e308)) return PNEC_HIP_PATCH_EMPTY;
  const double s0 = 1.0 / sqrt(H[0]), s1 = 1.0 / sqrt(H[3]), s2 = 1.0 / sqrt(H[5]);
  // A = D H D, L L' = A, row by row
  const double p0 = (H[0] * s0) * s0;
  bool ok = n >= 3 && p0 > 0.0;   // (fewer than three points: H has rank below three whatever the rounding says)
  const double i0 = 1.0 / sqrt(p0);
  const double l10 = ((H[1] * s0) * s1) * i0, l20 = ((H[2] * s0) * s2) * i0;
  const double p1 = (H[3] * s1) * s1 - l10 * l10;
  ok = ok && p1 > 0.0;
  const double i1 = 1.0 / sqrt(p1);
  const double l21 = (((H[4] * s1) * s2) - l20 * l10) * i1;
  const double p2 = ((H[5] * s2) * s2 - l20 * l20) - l21 * l21;
  ok = ok && p2 > 0.0;
  const double i2 = 1.0 / sqrt(p2);
  // M = L^-1 (lower triangular): the entries the top-left 2x2 of A^-1 = M' M needs
  const double m10 = -(l10 * i0) * i1;
  const double m21 = -(l21 * i1) * i2;
  const double m20 = -(l20 * i0 + l21 * m10) * i2;
  const double a00 = (i0 * i0 + m10 * m10) + m20 * m20;
  const double a01 = m10 * i1 + m20 * m21;
  const double a11 = i1 * i1 + m21 * m21;
  const double xx = ((a00 * s0) * s0) / scaling, xy = ((a01 * s0) * s1) / scaling, yy = ((a11 * s1) * s1) / scaling;
  const double z = (xx * 0.0 + xy * 0.0) + yy * 0.0;   // 0 iff all three are finite
  if (!ok || !(z == 0.0)) return PNEC_HIP_PATCH_SINGULAR;
  // Sigma' = R Sigma R',  R = [c -s; s c]
  const double ra = c * xx - s * xy, rb = c * xy - s * yy;   // first row of R Sigma
  const double re = s * xx + c * xy, rf = s * xy + c * yy;   // second row
  cov[0] = ra * c - rb * s;
  cov[1] = ra * s + rb * c;
  cov[2] = re * s + rf * c;
  return PNEC_HIP_PATCH_OK;
}

#if defined(__HIPCC__)
struct PatchCovArgs {
  const void *images;
  int32_t w, h;
  int64_t pitch;        // elements between rows; image f starts at element f * h * pitch
  int64_t n_images;
  const int64_t *offsets;   // [n_images + 1]
  int64_t n_points;
  const double *pts;        // [n_points, 2]
  const double *pattern;    // [n_pattern, 2]
  int32_t n_pattern;
  double scaling;
  const double *angle;      // [n_points] or NULL
  double *out_cov;          // [n_points, 3] or NULL
  double *out_hessian;      // [n_points, 6] or NULL
  double *out_mean;         // [n_points]    or NULL
  int32_t *out_n_valid;     // [n_points]    or NULL
  int32_t *out_status;      // [n_points]    or NULL
};

// 16 keypoints per block of 256 threads
hipError_t launch_patch_covariance(int pixel_type, const PatchCovArgs &a, hipStream_t stream);
#endif

}  // namespace pnec_hip
