// pnec_sensitivity.hip -- input gradients of a solved pose: the derivative of a loss of the refinement's minimiser with
// respect to every bearing vector and covariance of its pair, by the implicit-function theorem at the pose the caller
// passes in (pnec_hip_pose_sensitivity, include/pnec_hip.h).  A translation unit of its own: the solve / stream /
// front-stage / pose-pass objects do not see it.  Blocks, wavefronts, the pose, the output offset and the exchange of
// the wavefronts' sums: pnec_pose_pass.hpp.  The arithmetic: pnec_sensitivity.hpp.
//
// Three phases per slot, in a fixed order, so a slot's bits depend on its own pair and pose only:
//   (a) every wavefront of the pair walks its share of the zero-padded planes and sums r^2, g = J'r and the full Hessian
//       H = J'J + sum r grad^2 r of the chart (J'J alone with PNEC_HIP_SENS_GAUSS_NEWTON); 21 sums through wave_reduce21
//       and combine_waves, in wave order;
//   (b) thread 0 factors the Jacobi-scaled H, solves for lambda = H^-1 v (v: the caller's cotangent in the chart) and the
//       Newton step x_N = -H^-1 g, writes the slot's outputs and parks lambda in LDS;
//   (c) the wavefronts walk the planes again (the pair was just read: L2) and each lane writes its correspondence's rows
//       -d(lambda . grad_x r^2/2)/d(f1, f2, S) with plain stores.  A lane's row is 24 or 72 bytes and consecutive lanes
//       write consecutive rows, so a wavefront's store instruction covers one contiguous range.
// No atomics, no device allocation, no scratch.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "pnec_device.hpp"
#include "pnec_sensitivity.hpp"

namespace pnec_hip {

namespace {

// one wavefront's 21 sums
struct SensSums {
  double v[kNumAcc];
  __device__ __forceinline__ void add(const SensSums &o) {
#pragma unroll
    for (int j = 0; j < kNumAcc; ++j) v[j] += o.v[j];
  }
};

// the 3x3 symmetric matrix of six unique entries (xx, xy, xz, yy, yz, zz), row i of the [M,9] output
__device__ __forceinline__ void store_sym9(double *out, int64_t i, const double (&G)[6]) {
  double *o = out + i * 9;
  o[0] = G[0]; o[1] = G[1]; o[2] = G[2];
  o[3] = G[1]; o[4] = G[3]; o[5] = G[4];
  o[6] = G[2]; o[7] = G[4]; o[8] = G[5];
}

// A lane's sums with the Hessian's fifteen in LDS: column `tid` of a [15][kCovMaxWaves * kWave] table (conflict-free,
// and only its own lane ever touches a column: no barrier).  For the kernel whose pass does not fit the registers
// with all 21 in them.
struct SensAccLds {
  double v[6];
  double *h;
  __device__ __forceinline__ void add(int j, double x) {
    if (j < 6) v[j] += x;
    else h[(j - 6) * (kCovMaxWaves * kWave)] += x;
  }
};

}  // namespace

static_assert(kSensSums == kNumAcc, "the sums go through wave_reduce21");

// FULL: the Hessian with its second-derivative term; false: J'J (PNEC_HIP_SENS_GAUSS_NEWTON).  A kernel of its own each:
// with the choice left to a branch the SYM kernel does not fit its registers.
template <int MODE, bool FULL>
__global__ __launch_bounds__(kCovMaxWaves *kWave) void pose_sensitivity_kernel(const SensitivityArgs a) {
  using T = SensTraits<MODE>;
  constexpr int NC = num_components(MODE);
  static_assert(NC == T::NC, "plane count");
  __shared__ SensSums part[kCovMaxWaves];
  __shared__ double lam_s[5];
  __shared__ int32_t failed_s;

  const PoseSlot g = pose_slot(a.count, a.offsets, a.n_hyp);
  const int64_t s = g.s, ob = g.ob;
  const int lane = g.lane, wave = g.wave, n = g.n, stride = g.stride, W = g.W;
  const double *base = a.data + a.block_offset[g.p];

  // the pose goes to scalar registers: every lane holds the same bits, and every term below reads it
  SensPose P;
  {
    double R[9], st, ct, cp, sp;
    pose_setup(a.q + 4 * s, a.t + 3 * s, R, st, ct, cp, sp);
    SensPose V;
    sens_pose(R, st, ct, cp, sp, V);
#pragma unroll
    for (int i = 0; i < 9; ++i) P.R[i] = to_sgpr(V.R[i]);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      P.t[i] = to_sgpr(V.t[i]);
      P.B[0][i] = to_sgpr(V.B[0][i]);
      P.B[1][i] = to_sgpr(V.B[1][i]);
    }
  }

  // (a) the planes are padded with zeros to `stride`, and a zero slot contributes exactly 0
  // (SYM with the full Hessian: 18 planes and the second derivatives of two quadratic forms leave no room for 21
  // accumulators; the Hessian's fifteen stay in LDS during the walk)
  constexpr bool kLdsAcc = T::kSym && FULL;
  __shared__ double hacc[kLdsAcc ? 15 * kCovMaxWaves * kWave : 1];
  std::conditional_t<kLdsAcc, SensAccLds, SensAccArray> lane_acc;
#pragma unroll
  for (int j = 0; j < (kLdsAcc ? 6 : kNumAcc); ++j) lane_acc.v[j] = 0.0;
  if constexpr (kLdsAcc) {
    lane_acc.h = hacc + threadIdx.x;
#pragma unroll
    for (int j = 0; j < 15; ++j) lane_acc.h[j * (kCovMaxWaves * kWave)] = 0.0;
  }
  if (wave < W) {
    for (int i = wave * kWave + lane; i < stride; i += W * kWave) {
      double d[NC];
#pragma unroll
      for (int c = 0; c < NC; ++c) d[c] = base[(int64_t)c * stride + i];
      sens_accumulate<MODE, FULL>(d, P, a.reg, lane_acc);
    }
  }
  double acc[kNumAcc];
#pragma unroll
  for (int j = 0; j < kNumAcc; ++j) {
    if constexpr (kLdsAcc) acc[j] = j < 6 ? lane_acc.v[j] : lane_acc.h[(j - 6) * (kCovMaxWaves * kWave)];
    else acc[j] = lane_acc.v[j];
  }
  SensSums total;
  wave_reduce21(acc, total.v);
  combine_waves(g, part, total);

  // (b)
  if (threadIdx.x == 0) {
    double H[15], gr[5], lam[5], xn[5];
    const int status = sens_finish(total.v, P, a.grad_pose + 6 * s, n, a.flags, H, gr, lam, xn);
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      lam_s[i] = lam[i];
      if (a.out_lambda) a.out_lambda[s * 5 + i] = lam[i];
      if (a.out_newton) a.out_newton[s * 5 + i] = xn[i];
      if (a.out_grad) a.out_grad[s * 5 + i] = gr[i];
    }
    if (a.out_hessian) {
#pragma unroll
      for (int i = 0; i < 15; ++i) a.out_hessian[s * 15 + i] = H[i];
    }
    if (a.out_status) a.out_status[s] = status;
    failed_s = status != PNEC_HIP_SENS_OK;
  }
  __syncthreads();

  // (c)
  if (!a.out_grad_bvs1 && !a.out_grad_bvs2 && !a.out_grad_covs && !a.out_grad_covs_host) return;
  if (wave >= W) return;
  double lam[5];
#pragma unroll
  for (int i = 0; i < 5; ++i) lam[i] = to_sgpr(lam_s[i]);
  const bool failed = to_sgpr((int)failed_s) != 0;
  for (int i = wave * kWave + lane; i < n; i += W * kWave) {
    double gf1[3], gf2[3], Gg[6], Gh[6];
    if (failed) {   // (a failed slot's lambda is the fill value: every row is that value)
#pragma unroll
      for (int j = 0; j < 3; ++j) gf1[j] = gf2[j] = lam[0];
#pragma unroll
      for (int j = 0; j < 6; ++j) Gg[j] = Gh[j] = lam[0];
    } else {
      double d[NC];
#pragma unroll
      for (int c = 0; c < NC; ++c) d[c] = base[(int64_t)c * stride + i];
      sens_gradients<MODE>(d, P, a.reg, lam, gf1, gf2, Gg, Gh);
    }
    const int64_t e = ob + i;
    if (a.out_grad_bvs1) {
#pragma unroll
      for (int j = 0; j < 3; ++j) a.out_grad_bvs1[e * 3 + j] = gf1[j];
    }
    if (a.out_grad_bvs2) {
#pragma unroll
      for (int j = 0; j < 3; ++j) a.out_grad_bvs2[e * 3 + j] = gf2[j];
    }
    // the planes 6..11 are S_g in TARGET and SYM, S_h in HOST; SYM's planes 12..17 are S_h
    if constexpr (MODE != PNEC_HIP_MODE_NEC) {
      if (a.out_grad_covs) store_sym9(a.out_grad_covs, e, T::kG ? Gg : Gh);
    }
    if constexpr (T::kSym) {
      if (a.out_grad_covs_host) store_sym9(a.out_grad_covs_host, e, Gh);
    }
  }
}

template <int MODE>
struct PoseSensitivityKernel {
  static constexpr auto run = &pose_sensitivity_kernel<MODE, true>;
};
template <int MODE>
struct PoseSensitivityGnKernel {
  static constexpr auto run = &pose_sensitivity_kernel<MODE, false>;
};

hipError_t launch_pose_sensitivity(int mode, int64_t n_slots, int waves, const SensitivityArgs &a, hipStream_t stream) {
  if (a.flags & PNEC_HIP_SENS_GAUSS_NEWTON) return launch_by_mode<PoseSensitivityGnKernel>(mode, n_slots, waves, a, stream);
  return launch_by_mode<PoseSensitivityKernel>(mode, n_slots, waves, a, stream);
}

}  // namespace pnec_hip
