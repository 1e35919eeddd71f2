// pnec_pose_pass.hpp -- what the passes at a pose the caller passes in have in common, one copy of each:
// pose_covariance_kernel (pnec_pose_cov.hip), residuals_kernel (pnec_residuals.hip), triangulate_kernel
// (pnec_triangulate.hip) and relative_scale_kernel (pnec_relative_scale.hip).  Everything is __forceinline__: a kernel
// that calls a piece gets the statements it would have written out.
//
// Geometry.  One block per slot s = pair * n_hyp + h (the relative scale: per pair, n_hyp = 1), launched with
// cov_waves(n_max) wavefronts of which a pair of n correspondences uses W = cov_waves(n); correspondence i goes to
// wavefront (i / 64) mod W, a wavefront walks  for (i = wave * 64 + lane; i < stride; i += W * 64)  over planes padded
// with zeros to stride = n rounded up to 64.  Per-correspondence outputs of slot s start at entry
// n_hyp * offsets[p] + h * n (offsets relative to the batch's first pair).
//   pose_slot      the slot's numbers from blockIdx.x, count, offsets and n_hyp
//   pose_setup     R and the sines and cosines of t's angles from the slot's q and t -- the one definition of what the
//                  four calls of include/pnec_hip.h agree on.  Builds for the host too (tools/relative_scale_link_host.hip),
//                  so which values go to scalar registers is the caller's business
//   load_plane     one plane entry by scalar base and 32-bit byte offset
//   combine_waves  the wavefronts' partials through LDS to thread 0, in wave order
//   launch_by_mode the launch of a kernel template by residual family
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pnec_device.hpp"

namespace pnec_hip {

// How many wavefronts sum one pair: one per 512 correspondences (eight per lane, the one-wavefront solve's share),
// at most eight.  A function of the PAIR's own count, not of the launch: the block is sized for the batch's largest
// pair and the wavefronts a smaller pair does not need only meet the barrier, so a pair's sums are added in the same
// order -- have the same bits -- whatever batch it sits in.
constexpr int kCovCorrPerWave = 512;
constexpr int kCovMaxWaves = 8;
__host__ __device__ constexpr int cov_waves(int n) {
  const int w = (n + kCovCorrPerWave - 1) / kCovCorrPerWave;
  return w < 1 ? 1 : (w > kCovMaxWaves ? kCovMaxWaves : w);
}

struct PoseSlot {
  int64_t s, p, h;   // slot = p * n_hyp + h
  int lane, wave;    // wave is in a scalar register
  int n, stride, W;
  int64_t ob;        // the slot's first per-correspondence output entry
};

// a call without per-correspondence outputs (ob stays 0)
__device__ __forceinline__ PoseSlot pose_slot(const int32_t *count, int n_hyp) {
  PoseSlot g;
  g.s = blockIdx.x;
  g.p = g.s / n_hyp;
  g.h = g.s - g.p * n_hyp;
  g.lane = threadIdx.x & (kWave - 1);
  g.wave = to_sgpr((int)(threadIdx.x >> 6));
  g.n = count[g.p];
  g.stride = (g.n + kWave - 1) & ~(kWave - 1);
  // (the block is sized for the batch's largest pair, so the bound below never binds; it keeps a wrong size harmless)
  g.W = min(cov_waves(g.n), (int)(blockDim.x >> 6));
  g.ob = 0;
  return g;
}
__device__ __forceinline__ PoseSlot pose_slot(const int32_t *count, const int64_t *offsets, int n_hyp) {
  PoseSlot g = pose_slot(count, n_hyp);
  g.ob = (int64_t)n_hyp * (offsets[g.p] - offsets[0]) + g.h * (int64_t)g.n;
  return g;
}

// The pose of a slot: q (xyzw) normalised as pnec_hip_cost_function does, R from it; t as a DIRECTION through
// (theta, phi) of AnglesFromVec (common.cc:103-116) -- as sines and cosines straight from the components, which keeps
// sin(theta)'s relative accuracy at the pole where acos loses it.  t = 0 is read as +z; theta < 1e-10 (and t = 0)
// -> phi = 0.  The direction is (st * cp, st * sp, ct).
__device__ __forceinline__ void pose_setup(const double *qp, const double *tp, double (&R)[9], double &st, double &ct,
                                           double &cp, double &sp) {
  double q[4] = {qp[0], qp[1], qp[2], qp[3]};
  const double qn = 1.0 / sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
#pragma unroll
  for (int k = 0; k < 4; ++k) q[k] *= qn;
  const double tx = tp[0], ty = tp[1], tz = tp[2];
  const double nrm = sqrt(tx * tx + ty * ty + tz * tz), rho = sqrt(tx * tx + ty * ty);
  st = rho / nrm;
  ct = tz / nrm;
  cp = tx / rho;
  sp = ty / rho;
  if (nrm == 0.0) {
    st = 0.0;
    ct = 1.0;
  }
  if (rho == 0.0 || (st < 1e-10 && ct > 0.0)) {
    cp = 1.0;
    sp = 0.0;
  }
  rot_from_quat(q, R);
}

// Entry i of plane c: one scalar base and a 32-bit byte offset per load (as the solve kernels' plane loads) -- a 64-bit
// index per plane costs scalar registers.  The ABI layer refuses a batch whose largest pair has 4 GiB of planes or more.
__device__ __forceinline__ double load_plane(const char *base, unsigned plane_bytes, int c, int i) {
  return *reinterpret_cast<const double *>(base + ((unsigned)c * plane_bytes + (unsigned)i * 8u));
}

// The block's exchange of the wavefronts' partials.  P holds what one wavefront found (the same in all its lanes, or
// at least in lane 0) and has  void add(const P &).  Lane 0 of wavefronts 1..W-1 parks its P in LDS, a barrier follows
// only if the block has more than one wavefront (uniform: the launch's block size), and thread 0 adds them to its own
// in wave order -- that order is what makes a slot's bits independent of the batch it sits in.  Only thread 0's `mine`
// is the slot's afterwards.
template <class P>
__device__ __forceinline__ void combine_waves(const PoseSlot &g, P (&parked)[kCovMaxWaves], P &mine) {
  if (blockDim.x > kWave) {
    if (g.lane == 0 && g.wave > 0 && g.wave < g.W) parked[g.wave] = mine;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
#pragma unroll 1   // (a dependent chain of at most seven trips, once per block)
    for (int w = 1; w < g.W; ++w) mine.add(parked[w]);
  }
}

// Launches Kernel<MODE>::run, MODE the residual family, with one block of `waves` wavefronts per slot.  Kernel names a
// __global__ template:  template <int MODE> struct K { static constexpr auto run = &some_kernel<MODE>; };
template <template <int> class Kernel, class Args>
hipError_t launch_by_mode(int mode, int64_t n_slots, int waves, const Args &a, hipStream_t stream) {
  const dim3 grid((unsigned)n_slots), block((unsigned)(waves * kWave));
  switch (mode) {
    case PNEC_HIP_MODE_NEC:
      hipLaunchKernelGGL(Kernel<PNEC_HIP_MODE_NEC>::run, grid, block, 0, stream, a);
      break;
    case PNEC_HIP_MODE_TARGET:
      hipLaunchKernelGGL(Kernel<PNEC_HIP_MODE_TARGET>::run, grid, block, 0, stream, a);
      break;
    case PNEC_HIP_MODE_HOST:
      hipLaunchKernelGGL(Kernel<PNEC_HIP_MODE_HOST>::run, grid, block, 0, stream, a);
      break;
    case PNEC_HIP_MODE_SYM:
      hipLaunchKernelGGL(Kernel<PNEC_HIP_MODE_SYM>::run, grid, block, 0, stream, a);
      break;
    default:
      return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace pnec_hip
