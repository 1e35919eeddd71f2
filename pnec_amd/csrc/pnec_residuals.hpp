// pnec_residuals.hpp -- launch interface of the per-correspondence residual / chi-square gate kernel
// (pnec_residuals.hip), shared with the ABI layer.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pnec_device.hpp"
#include "pnec_pose_pass.hpp"   // cov_waves: the wavefronts of a pair follow from its own count

namespace pnec_hip {

struct ResidualArgs {
  const double *data;
  const int64_t *block_offset;
  const int32_t *count;
  const int64_t *offsets;      // [n_pairs+1] the batch's correspondence offsets (device)
  const double *q;             // [S,4] xyzw
  const double *t;             // [S,3]
  int32_t n_hyp;
  double reg;
  double gate;                 // in sigmas: inside iff |r| <= gate
  // per correspondence, entry n_hyp * offsets[p] + h * N_p + i; each may be NULL
  double *out_residual;
  double *out_variance;
  uint8_t *out_mask;
  // per slot [S]; each may be NULL
  double *out_chi2;
  double *out_gated_chi2;
  int32_t *out_gated_count;
  double *out_max_abs;
};

// one block of `waves` wavefronts per slot (pair * n_hyp + h)
hipError_t launch_residuals(int mode, int64_t n_slots, int waves, const ResidualArgs &a, hipStream_t stream);

// eval_cost's sibling: the residual with the same operations in the same order (so r carries the bits of the solve's
// cost pass), and the propagated variance it was whitened by -- den as the sum gives it, BEFORE the kTinyDen clamp
// (a zero covariance with reg = 0 reports variance 0 while r = n / sqrt(kTinyDen)); exactly 1 for NEC.
template <int MODE>
__device__ __forceinline__ void eval_residual(const double (&d)[num_components(MODE)], const PassUniforms &U,
                                              double reg, double &r, double &den) {
  const double f1x = d[0], f1y = d[1], f1z = d[2];
  const double f2x = d[3], f2y = d[4], f2z = d[5];
  const double *R = U.R;
  const double mx = U.t[1] * f1z - U.t[2] * f1y;
  const double my = U.t[2] * f1x - U.t[0] * f1z;
  const double mz = U.t[0] * f1y - U.t[1] * f1x;
  const double gx = R[0] * mx + R[3] * my + R[6] * mz;
  const double gy = R[1] * mx + R[4] * my + R[7] * mz;
  const double gz = R[2] * mx + R[5] * my + R[8] * mz;
  const double n = f2x * gx + f2y * gy + f2z * gz;
  if constexpr (MODE == PNEC_HIP_MODE_NEC) {
    r = n;
    den = 1.0;
  } else if constexpr (MODE == PNEC_HIP_MODE_TARGET) {
    const double sgx = d[6] * gx + d[7] * gy + d[8] * gz;
    const double sgy = d[7] * gx + d[9] * gy + d[10] * gz;
    const double sgz = d[8] * gx + d[10] * gy + d[11] * gz;
    den = gx * sgx + gy * sgy + gz * sgz + reg;
    const double y = fast_rsqrt(fmax(den, kTinyDen));
    r = n * y;
  } else {
    constexpr bool kSym = (MODE == PNEC_HIP_MODE_SYM);
    const double ax = kSym ? f2x : f1x, ay = kSym ? f2y : f1y, az = kSym ? f2z : f1z;
    const double px = R[0] * ax + R[1] * ay + R[2] * az;
    const double py = R[3] * ax + R[4] * ay + R[5] * az;
    const double pz = R[6] * ax + R[7] * ay + R[8] * az;
    const double qx = U.t[1] * pz - U.t[2] * py;
    const double qy = U.t[2] * px - U.t[0] * pz;
    const double qz = U.t[0] * py - U.t[1] * px;
    constexpr int o = kSym ? 12 : 6;
    const double shx = d[o + 0] * qx + d[o + 1] * qy + d[o + 2] * qz;
    const double shy = d[o + 1] * qx + d[o + 3] * qy + d[o + 4] * qz;
    const double shz = d[o + 2] * qx + d[o + 4] * qy + d[o + 5] * qz;
    den = qx * shx + qy * shy + qz * shz + reg;
    if constexpr (kSym) {
      const double sgx = d[6] * gx + d[7] * gy + d[8] * gz;
      const double sgy = d[7] * gx + d[9] * gy + d[10] * gz;
      const double sgz = d[8] * gx + d[10] * gy + d[11] * gz;
      den += gx * sgx + gy * sgy + gz * sgz;
    }
    const double y = fast_rsqrt(fmax(den, kTinyDen));
    r = n * y;
  }
}

// max over the 64 lanes, in every lane (fmax: a NaN operand is ignored -- the kernel carries NaN as a flag)
__device__ __forceinline__ double wave_allreduce_max(double x) {
  x = fmax(x, dpp_perm<0xB1>(x));   // quad_perm [1,0,3,2]
  x = fmax(x, dpp_perm<0x4E>(x));   // quad_perm [2,3,0,1]
  x = fmax(x, dpp_perm<0x141>(x));  // row_half_mirror
  x = fmax(x, dpp_perm<0x140>(x));  // row_mirror
  {
    const unsigned lo = (unsigned)__double2loint(x), hi = (unsigned)__double2hiint(x);
    const auto a = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
    const auto b = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
    x = fmax(make_double((int)b[0], (int)a[0]), make_double((int)b[1], (int)a[1]));
  }
  const unsigned lo = (unsigned)__double2loint(x), hi = (unsigned)__double2hiint(x);
  const auto a = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
  const auto b = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
  return fmax(make_double((int)b[0], (int)a[0]), make_double((int)b[1], (int)a[1]));
}

}  // namespace pnec_hip
