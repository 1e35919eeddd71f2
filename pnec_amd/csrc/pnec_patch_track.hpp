// pnec_patch_track.hpp -- patch tracking (pnec_hip_patch_track) and the pyramid's halving step
// (pnec_hip_image_pyramid_level): launch interface of pnec_patch_track.hip, shared with the ABI layer, and the functions
// that hold the tracker's arithmetic beside those of pnec_patch_cov.hpp -- the four-pixel interpolant, the full inverse of
// the template's Hessian, one point's gain, the SE(2) step, and the pyramid's filter -- written so that they also compile
// for the host (tools/patch_track_host.cc runs them under the address sanitizer on images without slack before any device
// does).  include/pnec_hip.h has the definition.
#pragma once

#include "pnec_patch_cov.hpp"

namespace pnec_hip {

// One pattern point at p = (px, py): the bilinear interpolant alone (basalt's interp [EXT]), four pixels -- (ix, iy),
// (ix+1, iy), (ix, iy+1), (ix+1, iy+1) -- in patch_point's order of operations, so that on the same point it returns
// patch_point's value bit for bit.  False -- and zero -- when the point is not valid (patch_point's rule).
template <typename T>
PNEC_PATCH_HD bool patch_value(const T *img, int64_t pitch, int32_t w, int32_t h, double px, double py, double &v) {
  PNEC_PATCH_NO_CONTRACT
  v = 0.0;
  if (!(px >= 2.0 && px < (double)w - 3.0 && py >= 2.0 && py < (double)h - 3.0)) return false;
  const double fx = floor(px), fy = floor(py);
  const int32_t ix = (int32_t)fx, iy = (int32_t)fy;
  const double dx = px - fx, dy = py - fy, ddx = 1.0 - dx, ddy = 1.0 - dy;
  const double w00 = ddx * ddy, w01 = ddx * dy, w10 = dx * ddy, w11 = dx * dy;
  const T *r1 = img + ((int64_t)iy * pitch + ix);
  const T *r2 = r1 + pitch;
  const double b0 = (double)r1[0], b1 = (double)r1[1], c0 = (double)r2[0], c1 = (double)r2[1];
  v = ((w00 * b0 + w01 * c0) + w10 * b1) + w11 * c1;
  return true;
}

// InBounds(t, 2) of a transform's translation: patch_point's rule on the point itself
PNEC_PATCH_HD bool track_in_bounds(int32_t w, int32_t h, double x, double y) {
  return x >= 2.0 && x < (double)w - 3.0 && y >= 2.0 && y < (double)h - 3.0;
}

// The template's full inverse.  n valid points, S = sum d, H the six sums (00 01 02 11 12 22); writes Hi, the upper
// triangle of H^-1 in the same layout, and returns pnec_hip_patch_status by patch_epilogue's rules: the same Jacobi-scaled
// Cholesky factor, term by term (so the pivots, and with them the verdict, are patch_epilogue's), and the inverse must be
// finite in all six entries.
PNEC_PATCH_HD int patch_inverse3(int n, double S, const double (&H)[6], double (&Hi)[6]) {
  PNEC_PATCH_NO_CONTRACT
  const double nan = (double)NAN;
  for (int k = 0; k < 6; ++k) Hi[k] = nan;
  if (n == 0 || !(S > 0.0) || !(S <= 1.7976931348623157e308)) return PNEC_HIP_PATCH_EMPTY;
  const double s0 = 1.0 / sqrt(H[0]), s1 = 1.0 / sqrt(H[3]), s2 = 1.0 / sqrt(H[5]);
  const double p0 = (H[0] * s0) * s0;
  bool ok = n >= 3 && p0 > 0.0;
  const double i0 = 1.0 / sqrt(p0);
  const double l10 = ((H[1] * s0) * s1) * i0, l20 = ((H[2] * s0) * s2) * i0;
  const double p1 = (H[3] * s1) * s1 - l10 * l10;
  ok = ok && p1 > 0.0;
  const double i1 = 1.0 / sqrt(p1);
  const double l21 = (((H[4] * s1) * s2) - l20 * l10) * i1;
  const double p2 = ((H[5] * s2) * s2 - l20 * l20) - l21 * l21;
  ok = ok && p2 > 0.0;
  const double i2 = 1.0 / sqrt(p2);
  // M = L^-1 (lower triangular), A^-1 = M' M
  const double m10 = -(l10 * i0) * i1;
  const double m21 = -(l21 * i1) * i2;
  const double m20 = -(l20 * i0 + l21 * m10) * i2;
  const double a00 = (i0 * i0 + m10 * m10) + m20 * m20;
  const double a01 = m10 * i1 + m20 * m21;
  const double a02 = m20 * i2;
  const double a11 = i1 * i1 + m21 * m21;
  const double a12 = m21 * i2;
  const double a22 = i2 * i2;
  const double h00 = (a00 * s0) * s0, h01 = (a01 * s0) * s1, h02 = (a02 * s0) * s2;
  const double h11 = (a11 * s1) * s1, h12 = (a12 * s1) * s2, h22 = (a22 * s2) * s2;
  const double z = ((((h00 * 0.0 + h01 * 0.0) + h02 * 0.0) + h11 * 0.0) + h12 * 0.0) + h22 * 0.0;   // 0 iff all finite
  if (!ok || !(z == 0.0)) return PNEC_HIP_PATCH_SINGULAR;
  Hi[0] = h00;
  Hi[1] = h01;
  Hi[2] = h02;
  Hi[3] = h11;
  Hi[4] = h12;
  Hi[5] = h22;
  return PNEC_HIP_PATCH_OK;
}

// K_i = H^-1 J_i' of one template point: J_i = (gpx, gpy, -pat_y gpx + pat_x gpy), patch_accumulate's
PNEC_PATCH_HD void track_gain(const double (&Hi)[6], double gpx, double gpy, double pat_x, double pat_y,
                              double (&K)[3]) {
  PNEC_PATCH_NO_CONTRACT
  const double r = -pat_y * gpx + pat_x * gpy;
  K[0] = (Hi[0] * gpx + Hi[1] * gpy) + Hi[2] * r;
  K[1] = (Hi[1] * gpx + Hi[3] * gpy) + Hi[4] * r;
  K[2] = (Hi[2] * gpx + Hi[4] * gpy) + Hi[5] * r;
}

// where pattern point (pat_x, pat_y) lies under the transform (t, R(theta)), (c, s) = (cos, sin) theta
PNEC_PATCH_HD void track_warp(double c, double s, double tx, double ty, double pat_x, double pat_y, double &px,
                              double &py) {
  PNEC_PATCH_NO_CONTRACT
  px = (c * pat_x - s * pat_y) + tx;
  py = (s * pat_x + c * pat_y) + ty;
}

// (n v) / S: the template's data_i and the first term of r_i = (n2 v_i) / S2 - data_i, in one order of operations, so
// that a patch looked at where it was built has residuals that are exactly zero
PNEC_PATCH_HD double track_normalised_value(double n, double v, double S) {
  PNEC_PATCH_NO_CONTRACT
  return (n * v) / S;
}

// adds K_i r_i of one point to the three sums of -inc
PNEC_PATCH_HD void track_accumulate(const double (&K)[3], double r, double (&acc)[3]) {
  PNEC_PATCH_NO_CONTRACT
  acc[0] += K[0] * r;
  acc[1] += K[1] * r;
  acc[2] += K[2] * r;
}

// T <- T exp(inc): t += R(theta) V(d) (inc0, inc1), theta += d with d = inc2 and V(d) = [a -b; b a], a = sin d / d,
// b = (1 - cos d) / d, below |d| < 1e-10 the series a = 1 - d^2 / 6, b = d / 2.  (c, s) = (cos, sin) theta of the
// transform, (cd, sd) = (cos, sin) d.
PNEC_PATCH_HD void track_step(double c, double s, double cd, double sd, double inc0, double inc1, double d, double &tx,
                              double &ty, double &theta) {
  PNEC_PATCH_NO_CONTRACT
  const bool tiny = fabs(d) < 1e-10;
  const double a = tiny ? 1.0 - (d * d) / 6.0 : sd / d;
  const double b = tiny ? 0.5 * d : (1.0 - cd) / d;
  const double ux = a * inc0 - b * inc1, uy = b * inc0 + a * inc1;
  tx = tx + (c * ux - s * uy);
  ty = ty + (s * ux + c * uy);
  theta = theta + d;
}

// The pyramid's filter.  r(i, n): the reflection about the border pixels that does not repeat them (n >= 4, -2 <= i <= n+1)
PNEC_PATCH_HD int32_t pyr_reflect(int32_t i, int32_t n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

PNEC_PATCH_HD uint32_t pyr_taps(uint32_t a, uint32_t b, uint32_t c, uint32_t d, uint32_t e) {
  return (((a + 4u * b) + 6u * c) + 4u * d) + e;
}
PNEC_PATCH_HD double pyr_taps(double a, double b, double c, double d, double e) {
  PNEC_PATCH_NO_CONTRACT
  return (((a + 4.0 * b) + 6.0 * c) + 4.0 * d) + e;
}
template <typename T>
struct PyrAcc {
  typedef uint32_t type;
  static PNEC_PATCH_HD T finish(uint32_t s) { return (T)((s + 128u) >> 8); }
};
template <>
struct PyrAcc<float> {
  typedef double type;
  static PNEC_PATCH_HD float finish(double s) { return (float)(s / 256.0); }
};

// one output pixel (x, y) of the half-size image from the h x w image `img`
template <typename T>
PNEC_PATCH_HD T pyr_pixel(const T *img, int64_t pitch, int32_t w, int32_t h, int32_t x, int32_t y) {
  typedef typename PyrAcc<T>::type A;
  const int32_t c0 = pyr_reflect(2 * x - 2, w), c1 = pyr_reflect(2 * x - 1, w), c2 = 2 * x, c3 = pyr_reflect(2 * x + 1, w),
                c4 = pyr_reflect(2 * x + 2, w);
  A row[5];
  for (int j = 0; j < 5; ++j) {
    const T *r = img + (int64_t)pyr_reflect(2 * y + j - 2, h) * pitch;
    row[j] = pyr_taps((A)r[c0], (A)r[c1], (A)r[c2], (A)r[c3], (A)r[c4]);
  }
  return PyrAcc<T>::finish(pyr_taps(row[0], row[1], row[2], row[3], row[4]));
}

#if defined(__HIPCC__)
// (shared with pnec_patch_store.hip, which compiles the tracker's body a third time)
constexpr int kTrackBlock = 256;

// the integer sum over the 16 lanes of a DPP row, in every lane
__device__ __forceinline__ int track_row_sum_i(int x) {
  x += __builtin_amdgcn_mov_dpp(x, 0xB1, 0xF, 0xF, true);    // quad_perm [1,0,3,2]
  x += __builtin_amdgcn_mov_dpp(x, 0x4E, 0xF, 0xF, true);    // quad_perm [2,3,0,1]
  x += __builtin_amdgcn_mov_dpp(x, 0x141, 0xF, 0xF, true);   // row_half_mirror
  x += __builtin_amdgcn_mov_dpp(x, 0x140, 0xF, 0xF, true);   // row_mirror
  return x;
}

struct PyramidLevelArgs {
  const void *in;
  void *out;
  int32_t w, h;            // of the input; the output is (h / 2) x (w / 2)
  int64_t pitch_in, pitch_out;   // elements between rows; image f starts at element f * height * pitch
  int64_t n_images;
};

struct TrackPyramid {
  const void *level[PNEC_HIP_TRACK_MAX_LEVELS];
  int64_t pitch[PNEC_HIP_TRACK_MAX_LEVELS];
};

struct PatchTrackArgs {
  TrackPyramid tmpl, prev, next;
  int32_t n_levels;
  int32_t w, h;             // of level 0
  int64_t n_images;
  const int64_t *offsets;   // [n_images + 1]
  int64_t n_points;
  const double *tmpl_pts;   // [n_points, 2]
  const double *init_pts;   // [n_points, 2] or NULL
  const double *init_angle; // [n_points] or NULL
  double shift_x, shift_y;
  const double *pattern;    // [n_pattern, 2]
  int32_t n_pattern;
  int32_t max_iterations;
  double max_recovered_dist2;
  int32_t backward;         // 0 with PNEC_HIP_TRACK_NO_BACKWARD
  double scaling;
  double *out_pts;          // [n_points, 2] or NULL
  double *out_angle;        // [n_points]    or NULL
  double *out_cov;          // [n_points, 3] or NULL
  double *out_dist2;        // [n_points]    or NULL
  int32_t *out_status;      // [n_points]    or NULL
  int32_t *out_lost_level;  // [n_points]    or NULL
};

hipError_t launch_image_pyramid_level(int pixel_type, const PyramidLevelArgs &a, hipStream_t stream);
// 16 keypoints per block of 256 threads
hipError_t launch_patch_track(int pixel_type, const PatchTrackArgs &a, hipStream_t stream);
// the same with a.tmpl a stack of n_tmpl_images images per level and keypoint k's templates built in image tmpl_image[k]
hipError_t launch_patch_track_indexed(int pixel_type, const PatchTrackArgs &a, const int32_t *tmpl_image,
                                      int64_t n_tmpl_images, hipStream_t stream);
#endif

}  // namespace pnec_hip
