// pnec_residuals.hip -- per-correspondence residuals and a chi-square inlier gate at a pose the caller passes in.  One
// pass over the pair's resident SoA planes, a translation unit of its own (the solve / stream / front-stage objects do
// not see it).
//
// The residuals of the probabilistic families are whitened by the propagated variance (r_i = n_i / sqrt(den_i)), so
// under the model r_i ~ N(0, 1) and r_i^2 is a chi-square statistic with one degree of freedom: |r_i| <= gate is "within
// `gate` sigmas of the pose".  The pass writes r_i, den_i and that verdict per correspondence, and per slot sum r^2, the
// same sum and the count over the gated set, and max |r|.  It classifies AT the pose it is given; it estimates nothing.
//
// r_i is eval_residual (pnec_residuals.hpp): eval_cost's operations in eval_cost's order.  Blocks, wavefronts, the pose
// and the output offset: pnec_pose_pass.hpp.  The slot sums go lane by lane through that header's stride, the tree of
// wave_reduce21 for accumulator 0 and the wavefronts' partials in wave order: no atomics, and a slot's bits depend on its
// own pair and pose only.
#include <hip/hip_runtime.h>

#include "pnec_device.hpp"
#include "pnec_residuals.hpp"

namespace pnec_hip {

// what one wavefront found
struct ResidualSums {
  double chi2, gated, max_abs;
  int32_t count, nan_seen;   // gated count | a NaN residual seen
  __device__ __forceinline__ void add(const ResidualSums &o) {
    chi2 += o.chi2;
    gated += o.gated;
    max_abs = fmax(max_abs, o.max_abs);
    count += o.count;
    nan_seen |= o.nan_seen;
  }
};

template <int MODE>
__global__ __launch_bounds__(kCovMaxWaves *kWave) void residuals_kernel(const ResidualArgs a) {
  constexpr int NC = num_components(MODE);
  __shared__ ResidualSums part[kCovMaxWaves];

  const PoseSlot g = pose_slot(a.count, a.offsets, a.n_hyp);
  const int64_t s = g.s, ob = g.ob;
  const int lane = g.lane, wave = g.wave, n = g.n, stride = g.stride, W = g.W;
  const double *base = a.data + a.block_offset[g.p];

  // the pose goes to scalar registers, as in the covariance pass.  eval_residual reads R and t only.
  double st, ct, cp, sp;
  PassUniforms U;
  {
    double R[9];
    pose_setup(a.q + 4 * s, a.t + 3 * s, R, st, ct, cp, sp);
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
  ResidualSums total = {read_lane<0>(c0), read_lane<32>(c0), read_lane<0>(wave_allreduce_max(mx)), cnt, nan_seen};
  combine_waves(g, part, total);
  if (threadIdx.x == 0) {
    if (a.out_chi2) a.out_chi2[s] = total.chi2;
    if (a.out_gated_chi2) a.out_gated_chi2[s] = total.gated;
    if (a.out_gated_count) a.out_gated_count[s] = total.count;
    if (a.out_max_abs) a.out_max_abs[s] = total.nan_seen ? __builtin_nan("") : total.max_abs;
  }
}

template <int MODE>
struct ResidualsKernel {
  static constexpr auto run = &residuals_kernel<MODE>;
};

hipError_t launch_residuals(int mode, int64_t n_slots, int waves, const ResidualArgs &a, hipStream_t stream) {
  return launch_by_mode<ResidualsKernel>(mode, n_slots, waves, a, stream);
}

}  // namespace pnec_hip
