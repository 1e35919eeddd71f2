// pnec_triangulate.hpp -- launch interface of the triangulation / cheirality kernel (pnec_triangulate.hip), shared
// with the ABI layer, and the device function that triangulates one correspondence.
//
// Pose.  R maps frame-2 vectors into frame 1 and x1 = R x2 + t: camera 1 sits at the origin, camera 2 at t.  The pose
// is pose_setup's (pnec_pose_pass.hpp): q is normalised inside, t is used as a DIRECTION (so the baseline is 1 and
// every length below is in baselines), and t = 0 is read as (0, 0, 1).
//
// Midpoint triangulation (the system of reprojection_score in pnec_frontend.hip, bearings not assumed unit).  With
// u = R f2:
//   a00 = f1.f1   a10 = f1.u   a11 = u.u   b0 = f1.t   b1 = u.t
//   D      = a00 a11 - a10^2                  (= sin^2 psi for unit bearings)
//   depth1 = (a11 b0 - a10 b1) / D            along f1, from camera 1
//   depth2 = (a10 b0 - a00 b1) / D            along u,  from camera 2
//   point  = 1/2 (depth1 f1 + t + depth2 u)   in frame 1
//   psi    = atan2(|f1 x u|, f1.u)            parallax, radians, in [0, pi]
//   front  = depth1 > 0 and depth2 > 0 (both finite)
//   back   = depth1 < 0 and depth2 < 0 (both finite)   -- "in front" under -t
// depth1, depth2 and point are linear in t: every operation below that carries t is a product, an FMA or a sum whose
// operands all change sign with t, so at -t they are the exact IEEE negations of their values at t, and front and back
// swap.
//
// Depth variance: the first-order propagation of the resident covariances to depth1.
//   d depth1 / d u  = ( 2 b0 u - b1 f1 - a10 t  -  depth1 (2 a00 u - 2 a10 f1) ) / D  =: gu
//   d depth1 / d f1 = ( a11 t - b1 u            -  depth1 (2 a11 f1 - 2 a10 u) ) / D  =: g1
//   TARGET: (R' gu)' Sigma2 (R' gu)       HOST: g1' Sigma1 g1       SYM: both summed       NEC: NaN
// Sigma2 is the covariance of f2 in frame 2 (planes 6..11 of TARGET and SYM), Sigma1 that of f1 in frame 1 (planes
// 6..11 of HOST, 12..17 of SYM).  No `reg` is added.  gu and g1 are odd in t, the variance is even.
//
// Degenerate inputs (the result is the same whatever else the pair holds):
//   D not a positive finite number (parallel rays, a zero bearing, a padding slot): depth1 = depth2 = +inf, point and
//     variance NaN, psi as the atan2 gives it (0 for parallel rays), front 0, counted in neither vote;
//   a NaN in a bearing: every per-correspondence output NaN, front 0, counted in neither vote, left out of the
//     parallax mean.
// D is formed from two rounded products; a D at or below its own rounding error (2^-49 a00 a11) is read as 0, so that
// rays that are parallel before R f2 is rounded are parallel after.  The division is an IEEE division of a D known
// to be positive and finite (a select feeds it 1 otherwise).
//
// Vote, always at t as given: n_front / n_back count the front / back correspondences; sign = +1 if n_front >= n_back
// (a tie, an empty pair included), else -1; t_oriented = sign * t / |t|.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pnec_device.hpp"
#include "pnec_pose_pass.hpp"   // cov_waves: the wavefronts of a pair follow from its own count; pose_setup

namespace pnec_hip {

struct TriangulateArgs {
  const double *data;
  const int64_t *block_offset;
  const int32_t *count;
  const int64_t *offsets;      // [n_pairs+1] the batch's correspondence offsets (device)
  const double *q;             // [S,4] xyzw
  const double *t;             // [S,3]
  int32_t n_hyp;
  int32_t flags;               // PNEC_HIP_TRI_ORIENT
  // per correspondence, entry n_hyp * offsets[p] + h * N_p + i; each may be NULL
  double *out_point;           // [M,3]
  double *out_depth1;
  double *out_depth2;
  double *out_parallax;
  double *out_depth1_var;
  uint8_t *out_front;
  // per slot [S]; each may be NULL
  int32_t *out_n_front;
  int32_t *out_n_back;
  int32_t *out_sign;
  double *out_t_oriented;      // [S,3]
  double *out_parallax_mean;
};

// one block of `waves` wavefronts per slot (pair * n_hyp + h)
hipError_t launch_triangulate(int mode, int64_t n_slots, int waves, const TriangulateArgs &a, hipStream_t stream);

// D <= 2^-49 a00 a11 (sin^2 psi below 1.8e-15: psi below 4.2e-8 rad, where no digit of a depth is left) counts as
// "D not positive": parallel rays stay parallel after R f2 has been rounded
constexpr double kTriRelZero = 0x1p-49;

// the two depths of one correspondence and what the rest of the pass needs of the 2x2 system
struct TriSystem {
  double ux, uy, uz;           // u = R f2
  double a00, a10, a11, b0, b1;
  double inv;                  // 1 / D where ok, else 1
  double depth1, depth2;       // +inf where not ok
  bool ok;                     // D is a positive finite number
  bool isnan;                  // a NaN in f1 or f2
  bool front, back;
};

__device__ __forceinline__ void tri_depths(const double (&f)[6], const double (&R)[9], const double (&t)[3],
                                           TriSystem &s) {
  const double f1x = f[0], f1y = f[1], f1z = f[2];
  const double f2x = f[3], f2y = f[4], f2z = f[5];
  s.ux = R[0] * f2x + R[1] * f2y + R[2] * f2z;
  s.uy = R[3] * f2x + R[4] * f2y + R[5] * f2z;
  s.uz = R[6] * f2x + R[7] * f2y + R[8] * f2z;
  s.a00 = f1x * f1x + f1y * f1y + f1z * f1z;
  s.a10 = f1x * s.ux + f1y * s.uy + f1z * s.uz;
  s.a11 = s.ux * s.ux + s.uy * s.uy + s.uz * s.uz;
  s.b0 = f1x * t[0] + f1y * t[1] + f1z * t[2];
  s.b1 = s.ux * t[0] + s.uy * t[1] + s.uz * t[2];
  // both products rounded, not fused: for parallel rays (a00 = a10 = a11 up to rounding) a fused form returns the
  // rounding residual of a10^2, of either sign.  A D at or below its own rounding error is read as 0.
  const double a0011 = __dmul_rn(s.a00, s.a11);
  const double D = __dsub_rn(a0011, __dmul_rn(s.a10, s.a10));
  s.isnan = (f1x != f1x) | (f1y != f1y) | (f1z != f1z) | (f2x != f2x) | (f2y != f2y) | (f2z != f2z);
  s.ok = D > kTriRelZero * a0011 && finite_d(D);
  s.inv = 1.0 / (s.ok ? D : 1.0);
  const double n1 = __builtin_fma(s.a11, s.b0, -(s.a10 * s.b1));
  const double n2 = __builtin_fma(s.a10, s.b0, -(s.a00 * s.b1));
  const double inf = __builtin_inf();
  s.depth1 = s.ok ? n1 * s.inv : inf;
  s.depth2 = s.ok ? n2 * s.inv : inf;
  const bool fin = s.ok && !s.isnan && finite_d(s.depth1) && finite_d(s.depth2);
  s.front = fin && s.depth1 > 0.0 && s.depth2 > 0.0;
  s.back = fin && s.depth1 < 0.0 && s.depth2 < 0.0;
}

// x' Sigma x, Sigma = six planes (xx, xy, xz, yy, yz, zz) starting at c[0]
__device__ __forceinline__ double tri_quad_form(const double *c, double x, double y, double z) {
  const double sx = c[0] * x + c[1] * y + c[2] * z;
  const double sy = c[1] * x + c[3] * y + c[4] * z;
  const double sz = c[2] * x + c[4] * y + c[5] * z;
  return x * sx + y * sy + z * sz;
}

// atan2(y, x) for y >= 0, in [0, pi]: atan_lean's argument reduction and polynomial (pnec_device.hpp) with the
// quotient of each range written over a common denominator, so the ranges are selects and there is ONE division;
// atan2(0, 0) is 0 (a padding slot), a NaN argument gives NaN.
__device__ __forceinline__ double tri_atan2_pos(double y, double x) {
  const double kPi = 3.14159265358979311600e+00, kPiLo = 1.2246467991473531772e-16;
  const double ax = fabs(x);
  double num = y, den = ax, hi = 0.0, lo = 0.0;
  const bool reduced = y >= 0.4375 * ax;
  if (reduced) {
    hi = 4.63647609000806093515e-01; lo = 2.26987774529616870924e-17;
    num = 2.0 * y - ax; den = 2.0 * ax + y;
  }
  if (y >= 0.6875 * ax) {
    hi = 7.85398163397448278999e-01; lo = 3.06161699786838301793e-17;
    num = y - ax; den = ax + y;
  }
  if (y >= 1.1875 * ax) {
    hi = 9.82793723247329054082e-01; lo = 1.39033110312309984516e-17;
    num = y - 1.5 * ax; den = ax + 1.5 * y;
  }
  if (y >= 2.4375 * ax) {
    hi = 1.57079632679489655800e+00; lo = 6.12323399573676603587e-17;
    num = -ax; den = y;
  }
  const bool origin = den == 0.0;   // y = x = 0 only
  if (origin) den = 1.0;
  const double r = num / den;
  const double z = r * r, w = z * z;
  double s1 = __builtin_fma(w, 1.62858201153657823623e-02, 4.97687799461593236017e-02);
  s1 = __builtin_fma(w, s1, 6.66107313738753120669e-02);
  s1 = __builtin_fma(w, s1, 9.09088713343650656196e-02);
  s1 = __builtin_fma(w, s1, 1.42857142725034663711e-01);
  s1 = z * __builtin_fma(w, s1, 3.33333333333329318027e-01);
  double s2 = __builtin_fma(w, -3.65315727442169155270e-02, -5.83357013379057348645e-02);
  s2 = __builtin_fma(w, s2, -7.69187620504482999495e-02);
  s2 = __builtin_fma(w, s2, -1.11111104054623557880e-01);
  s2 = w * __builtin_fma(w, s2, -1.99999999998764832476e-01);
  const double a = reduced ? hi - ((r * (s1 + s2) - lo) - r) : r - r * (s1 + s2);
  const double res = x < 0.0 ? kPi - (a - kPiLo) : a;
  return origin ? 0.0 : res;
}

struct TriCorr {
  double depth1, depth2, px, py, pz, psi, var;
  bool front, back, isnan;
};

// One correspondence at (R, t): d[] holds its planes (0..2 f1 | 3..5 f2 | the covariances); the covariance planes are
// read only if want_var (wave-uniform).
template <int MODE>
__device__ __forceinline__ void triangulate_corr(const double (&d)[num_components(MODE)], const double (&R)[9],
                                                 const double (&t)[3], bool want_var, TriCorr &o) {
  const double f[6] = {d[0], d[1], d[2], d[3], d[4], d[5]};
  TriSystem s;
  tri_depths(f, R, t, s);
  const double nan = __builtin_nan("");
  const double cx = f[1] * s.uz - f[2] * s.uy;
  const double cy = f[2] * s.ux - f[0] * s.uz;
  const double cz = f[0] * s.uy - f[1] * s.ux;
  const double psi = tri_atan2_pos(sqrt(cx * cx + cy * cy + cz * cz), s.a10);
  const bool good = s.ok && !s.isnan;
  o.isnan = s.isnan;
  o.front = s.front;
  o.back = s.back;
  o.depth1 = s.isnan ? nan : s.depth1;
  o.depth2 = s.isnan ? nan : s.depth2;
  o.psi = s.isnan ? nan : psi;
  o.px = good ? 0.5 * __builtin_fma(s.depth1, f[0], __builtin_fma(s.depth2, s.ux, t[0])) : nan;
  o.py = good ? 0.5 * __builtin_fma(s.depth1, f[1], __builtin_fma(s.depth2, s.uy, t[1])) : nan;
  o.pz = good ? 0.5 * __builtin_fma(s.depth1, f[2], __builtin_fma(s.depth2, s.uz, t[2])) : nan;
  o.var = nan;
  if constexpr (MODE != PNEC_HIP_MODE_NEC) {
    if (want_var) {
      double v = 0.0;
      const double d1 = s.depth1;
      if constexpr (MODE == PNEC_HIP_MODE_TARGET || MODE == PNEC_HIP_MODE_SYM) {
        const double k = 2.0 * s.b0 - 2.0 * d1 * s.a00;   // of u
        const double l = 2.0 * d1 * s.a10 - s.b1;         // of f1
        const double gx = (k * s.ux + l * f[0] - s.a10 * t[0]) * s.inv;
        const double gy = (k * s.uy + l * f[1] - s.a10 * t[1]) * s.inv;
        const double gz = (k * s.uz + l * f[2] - s.a10 * t[2]) * s.inv;
        const double wx = R[0] * gx + R[3] * gy + R[6] * gz;
        const double wy = R[1] * gx + R[4] * gy + R[7] * gz;
        const double wz = R[2] * gx + R[5] * gy + R[8] * gz;
        v = tri_quad_form(&d[6], wx, wy, wz);
      }
      if constexpr (MODE == PNEC_HIP_MODE_HOST || MODE == PNEC_HIP_MODE_SYM) {
        constexpr int o1 = (MODE == PNEC_HIP_MODE_SYM) ? 12 : 6;
        const double k = 2.0 * d1 * s.a10 - s.b1;         // of u
        const double l = -2.0 * d1 * s.a11;               // of f1
        const double gx = (s.a11 * t[0] + k * s.ux + l * f[0]) * s.inv;
        const double gy = (s.a11 * t[1] + k * s.uy + l * f[1]) * s.inv;
        const double gz = (s.a11 * t[2] + k * s.uz + l * f[2]) * s.inv;
        v += tri_quad_form(&d[o1], gx, gy, gz);
      }
      o.var = good ? v : nan;
    }
  }
}

}  // namespace pnec_hip
