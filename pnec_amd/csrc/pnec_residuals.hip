// pnec_residuals.hip -- per-correspondence residuals and a chi-square inlier gate at a pose the caller passes in.  One
// pass over the pair's resident SoA planes, a translation unit of its own (the solve / stream / front-stage objects do
// not see it).
//
// The residuals of the probabilistic families are whitened by the propagated variance (r_i = n_i / sqrt(den_i)), so
// under the model r_i ~ N(0, 1) and r_i^2 is a chi-square statistic with one degree of freedom: |r_i| <= gate is "within
// `gate` sigmas of the pose".  The pass writes r_i, den_i and that verdict per correspondence, and per slot sum r^2, the
// same sum and the count over the gated set, and max |r|.  It classifies AT the pose it is given; it estimates nothing.
//
// r_i is eval_residual (pnec_residuals.hpp): eval_cost's operations in eval_cost's order.  The slot sums go lane by lane
// through the stride of the pose-covariance pass (correspondence i in wavefront (i / 64) mod W, W = cov_waves(n)), the
// tree of wave_reduce21 for accumulator 0 and the wavefronts' partials in wave order: no atomics, and a slot's bits
// depend on its own pair and pose only.
#include <hip/hip_runtime.h>

#include "pnec_device.hpp"
#include "pnec_residuals.hpp"

namespace pnec_hip {

template <int MODE>
__global__ __launch_bounds__(kCovMaxWaves *kWave) void residuals_kernel(const ResidualArgs a) {
  constexpr int NC = num_components(MODE);
  __shared__ double part[kCovMaxWaves][3];   // chi2 | gated chi2 | max |r|
  __shared__ int32_t parti[kCovMaxWaves][2]; // gated count | a NaN residual seen

  const int64_t s = blockIdx.x;
  const int64_t p = s / a.n_hyp;
  const int64_t h = s - p * a.n_hyp;
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = to_sgpr((int)(threadIdx.x >> 6));
  const int n = a.count[p];
  const int stride = (n + kWave - 1) & ~(kWave - 1);
  const double *base = a.data + a.block_offset[p];
  // (the block is sized for the batch's largest pair, so the bound below never binds; it keeps a wrong size harmless)
  const int W = min(cov_waves(n), (int)(blockDim.x >> 6));
  // where this slot's correspondences go: n_hyp * offsets[p] + h * N_p  (offsets relative to the batch's first pair)
  const int64_t ob = (int64_t)a.n_hyp * (a.offsets[p] - a.offsets[0]) + h * (int64_t)n;

  // pose: exactly pose_covariance_kernel's (q normalised; the sines and cosines of AnglesFromVec's angles straight
  // from the components of t).  eval_residual reads R and t only.
  double q[4] = {a.q[4 * s], a.q[4 * s + 1], a.q[4 * s + 2], a.q[4 * s + 3]};
  const double qn = 1.0 / sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
#pragma unroll
  for (int k = 0; k < 4; ++k) q[k] *= qn;
  const double tx = a.t[3 * s], ty = a.t[3 * s + 1], tz = a.t[3 * s + 2];
  const double nrm = sqrt(tx * tx + ty * ty + tz * tz), rho = sqrt(tx * tx + ty * ty);
  double st = rho / nrm, ct = tz / nrm, cp = tx / rho, sp = ty / rho;
  if (nrm == 0.0) {
    st = 0.0;
    ct = 1.0;
  }
  if (rho == 0.0 || (st < 1e-10 && ct > 0.0)) {
    cp = 1.0;
    sp = 0.0;
  }
  PassUniforms U;
  {
    double R[9];
    rot_from_quat(q, R);
#pragma unroll
    for (int i = 0; i < 9; ++i) U.R[i] = to_sgpr(R[i]);
  }
  st = to_sgpr(st);
  U.t[0] = to_sgpr(st * cp);   U.t[1] = to_sgpr(st * sp);   U.t[2] = to_sgpr(ct);
  U.bth[0] = 0.0; U.bth[1] = 0.0; U.bth[2] = 0.0;   // (the chart: not read by the residual)
  U.bph[0] = 0.0; U.bph[1] = 0.0; U.bph[2] = 0.0;

  // the pass: the planes are padded with zeros to `stride`, and a zero slot has r exactly 0 -- it adds 0 to both sums
  // and to the maximum; only the count and the stores need to know where the pair ends
  double chi2 = 0.0, gchi2 = 0.0, mx = 0.0;
  int cnt = 0, nan_seen = 0;   // wave-uniform
  if (wave < W) {
    for (int i = wave * kWave + lane; i < stride; i += W * kWave) {
      double d[NC];
#pragma unroll
      for (int c = 0; c < NC; ++c) d[c] = base[(int64_t)c * stride + i];
      double r, den;
      eval_residual<MODE>(d, U, a.reg, r, den);
      const double ar = fabs(r);
      const bool inside = finite_d(r) && ar <= a.gate;
      const bool real = i < n;
      chi2 = __builtin_fma(r, r, chi2);
      gchi2 = inside ? __builtin_fma(r, r, gchi2) : gchi2;
      mx = fmax(mx, ar);
      cnt += __popcll(__builtin_amdgcn_ballot_w64(inside && real));
      nan_seen |= (__builtin_amdgcn_ballot_w64(r != r) != 0ull) ? 1 : 0;
      if (real) {
        if (a.out_residual) a.out_residual[ob + i] = r;
        if (a.out_variance) a.out_variance[ob + i] = den;
        if (a.out_mask) a.out_mask[ob + i] = inside ? 1 : 0;
      }
    }
  }
  // chi2 through accumulator 0's tree, the gated sum through accumulator 11's (the other half of the same swaps):
  // after the two swap levels row 0 holds chi2's columns and row 2 the gated sum's
  const double c0 = row_allreduce_sum(swap_add16(swap_add32(chi2, gchi2), 0.0));
  double sum_chi2 = read_lane<0>(c0), sum_g = read_lane<32>(c0);
  double mxw = read_lane<0>(wave_allreduce_max(mx));
  if (blockDim.x > kWave) {   // (uniform: the launch's block size)
    if (lane == 0 && wave > 0 && wave < W) {
      part[wave][0] = sum_chi2;
      part[wave][1] = sum_g;
      part[wave][2] = mxw;
      parti[wave][0] = cnt;
      parti[wave][1] = nan_seen;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    for (int w = 1; w < W; ++w) {
      sum_chi2 += part[w][0];
      sum_g += part[w][1];
      mxw = fmax(mxw, part[w][2]);
      cnt += parti[w][0];
      nan_seen |= parti[w][1];
    }
    if (a.out_chi2) a.out_chi2[s] = sum_chi2;
    if (a.out_gated_chi2) a.out_gated_chi2[s] = sum_g;
    if (a.out_gated_count) a.out_gated_count[s] = cnt;
    if (a.out_max_abs) a.out_max_abs[s] = nan_seen ? __builtin_nan("") : mxw;
  }
}

hipError_t launch_residuals(int mode, int64_t n_slots, int waves, const ResidualArgs &a, hipStream_t stream) {
  const dim3 grid((unsigned)n_slots), block((unsigned)(waves * kWave));
  switch (mode) {
    case PNEC_HIP_MODE_NEC:
      hipLaunchKernelGGL(residuals_kernel<PNEC_HIP_MODE_NEC>, grid, block, 0, stream, a);
      break;
    case PNEC_HIP_MODE_TARGET:
      hipLaunchKernelGGL(residuals_kernel<PNEC_HIP_MODE_TARGET>, grid, block, 0, stream, a);
      break;
    case PNEC_HIP_MODE_HOST:
      hipLaunchKernelGGL(residuals_kernel<PNEC_HIP_MODE_HOST>, grid, block, 0, stream, a);
      break;
    case PNEC_HIP_MODE_SYM:
      hipLaunchKernelGGL(residuals_kernel<PNEC_HIP_MODE_SYM>, grid, block, 0, stream, a);
      break;
    default:
      return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace pnec_hip
