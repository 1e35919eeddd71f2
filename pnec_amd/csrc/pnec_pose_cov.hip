// pnec_pose_cov.hip -- pose covariance: the Gauss-Newton information J'J of a pair at a pose the caller passes in, and
// its inverse lifted to a 6x6 covariance of (rotation vector, translation direction).  One pass over the pair's
// resident SoA planes, a translation unit of its own (the solve / stream objects do not see it).  Blocks, wavefronts, the
// pose and the exchange of the wavefronts' sums: pnec_pose_pass.hpp.
//
// The residuals of the probabilistic families are whitened by the propagated variance, so J'J at the solution is the
// inverse of the posterior covariance (Laplace approximation; what ceres::Covariance returns for the reference's
// problem, src/optimization/pnec_ceres.cc:70-111).
//
// Chart.  The reference's translation chart (theta, phi) is singular at t = (0, 0, 1): |dt/dphi| = sin(theta), and
// forward motion sits there.  The pass therefore runs in the orthonormal chart
//   x = (tau_1, tau_2, omega_x, omega_y, omega_z):   t <- normalize(t + tau_1 b_theta + tau_2 e_phi),  R <- Exp(omega) R
// with b_theta = dt/dtheta (unit) and e_phi = (-sin phi, cos phi, 0) = (dt/dphi) / sin(theta) -- for eval_corr that is a
// change of PassUniforms::bph, nothing else.  H_x = sum J_x' J_x stays well conditioned at the pole.  From it, exactly:
//   Ceres tangent space (theta, phi, delta_xyz; delta = omega / 2):  H_c = D H_x D,  D = diag(1, sin theta, 2, 2, 2)
//   covariance:  Sigma_x = H_x^-1 (Cholesky of the Jacobi-scaled matrix),
//                Sigma_6 = L Sigma_x L',  L = blockdiag(I_3 on omega, [b_theta e_phi])   (order: omega, t)
#include <hip/hip_runtime.h>

#include "pnec_device.hpp"
#include "pnec_pose_cov.hpp"

namespace pnec_hip {

namespace {

// what one block leaves in LDS for its coalesced stores: cov 36 | info 15 | grad 5 | cost 1
constexpr int kOutCov = 0, kOutInfo = 36, kOutGrad = 51, kOutCost = 56, kOutDoubles = 57;

// Upper triangle (tri order) of the inverse of the SPD 5x5 whose upper triangle is H, through the Cholesky factor of
// the Jacobi-scaled matrix diag(H)^-1/2 H diag(H)^-1/2 (unit diagonal: the pivots are those of a correlation matrix,
// whatever the units of the columns).  The LM step's scale 1 / (1 + sqrt(H_aa)) exists for columns that may be zero;
// here a zero column means "singular" either way.  False when a pivot is not positive or a result is not finite.
__device__ __forceinline__ bool spd_inverse5(const double (&H)[15], double (&S)[15]) {
  double sc[5];
#pragma unroll
  for (int a = 0; a < 5; ++a) sc[a] = fast_rsqrt(H[tri(a, a)]);
  double L[15];  // L(i,j), i >= j, at tri(j,i)
  double inv[5];
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    double dj = (H[tri(j, j)] * sc[j]) * sc[j];
#pragma unroll
    for (int k = 0; k < j; ++k) dj = __builtin_fma(-L[tri(k, j)], L[tri(k, j)], dj);
    ok = ok && (dj > 0.0);
    const double iv = fast_rsqrt(dj);
    inv[j] = iv;
    L[tri(j, j)] = dj * iv;
#pragma unroll
    for (int i = j + 1; i < 5; ++i) {
      double s = (H[tri(j, i)] * sc[j]) * sc[i];
#pragma unroll
      for (int k = 0; k < j; ++k) s = __builtin_fma(-L[tri(k, i)], L[tri(k, j)], s);
      L[tri(j, i)] = s * iv;
    }
  }
  // M = L^-1 (lower triangular), M(i,j) at tri(j,i)
  double M[15];
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    M[tri(j, j)] = inv[j];
#pragma unroll
    for (int i = j + 1; i < 5; ++i) {
      double s = 0.0;
#pragma unroll
      for (int k = j; k < i; ++k) s = __builtin_fma(L[tri(k, i)], M[tri(j, k)], s);
      M[tri(j, i)] = -s * inv[i];
    }
  }
  // inverse = M' M, scaled back
  double z = 0.0;
#pragma unroll
  for (int a = 0; a < 5; ++a)
#pragma unroll
    for (int b = a; b < 5; ++b) {
      double s = 0.0;
#pragma unroll
      for (int k = b; k < 5; ++k) s = __builtin_fma(M[tri(a, k)], M[tri(b, k)], s);
      S[tri(a, b)] = (s * sc[a]) * sc[b];
      z = __builtin_fma(S[tri(a, b)], 0.0, z);
    }
  return ok && (z == 0.0);
}

// one wavefront's 21 sums
struct CovSums {
  double v[kNumAcc];
  __device__ __forceinline__ void add(const CovSums &o) {
#pragma unroll
    for (int j = 0; j < kNumAcc; ++j) v[j] += o.v[j];
  }
};

}  // namespace

template <int MODE>
__global__ __launch_bounds__(kCovMaxWaves *kWave) void pose_covariance_kernel(const PoseCovArgs a) {
  constexpr int NC = num_components(MODE);
  __shared__ CovSums part[kCovMaxWaves];
  __shared__ double outbuf[kOutDoubles];
  __shared__ int32_t out_st;

  const PoseSlot g = pose_slot(a.count, a.n_hyp);
  const int64_t s = g.s;
  const int lane = g.lane, wave = g.wave, n = g.n, stride = g.stride, W = g.W;
  const double *base = a.data + a.block_offset[g.p];

  // the pose goes to scalar registers: every lane holds the same bits, and eval_corr reads it in every term
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
  U.bth[0] = to_sgpr(ct * cp); U.bth[1] = to_sgpr(ct * sp); U.bth[2] = to_sgpr(-st);
  U.bph[0] = to_sgpr(-sp);     U.bph[1] = to_sgpr(cp);      U.bph[2] = 0.0;   // e_phi: unit, where the solve has dt/dphi

  // the pass: the planes are padded with zeros to `stride`, and a zero slot contributes exactly 0 (eval_corr)
  double acc[kNumAcc];
#pragma unroll
  for (int j = 0; j < kNumAcc; ++j) acc[j] = 0.0;
  if (wave < W) {
    for (int i = wave * kWave + lane; i < stride; i += W * kWave) {
      double d[NC];
#pragma unroll
      for (int c = 0; c < NC; ++c) d[c] = base[(int64_t)c * stride + i];
      double r, J[5];
      eval_corr<MODE>(d, U, a.reg, r, J);
      accumulate(r, J, acc);
    }
  }
  CovSums total;
  wave_reduce21(acc, total.v);
  combine_waves(g, part, total);

  if (threadIdx.x == 0) {
    const double (&sum)[kNumAcc] = total.v;
    double z = 0.0;
#pragma unroll
    for (int j = 0; j < kNumAcc; ++j) z = __builtin_fma(sum[j], 0.0, z);
    const bool finite = (z == 0.0);

    // Ceres tangent space: phi column x sin(theta), delta columns x 2
    const double D[5] = {1.0, st, 2.0, 2.0, 2.0};
    outbuf[kOutCost] = 0.5 * sum[0];
#pragma unroll
    for (int i = 0; i < 5; ++i) outbuf[kOutGrad + i] = sum[1 + i] * D[i];
    double H[15];
#pragma unroll
    for (int i = 0; i < 5; ++i)
#pragma unroll
      for (int j = i; j < 5; ++j) {
        H[tri(i, j)] = sum[6 + tri(i, j)];
        outbuf[kOutInfo + tri(i, j)] = (H[tri(i, j)] * D[i]) * D[j];
      }

    double S[15];
    const bool ok = spd_inverse5(H, S);
    const int status = !finite ? PNEC_HIP_COV_NONFINITE : ((n < 5 || !ok) ? PNEC_HIP_COV_SINGULAR : PNEC_HIP_COV_OK);
    out_st = status;
    // lift: rows / columns 0..2 omega, 3..5 t;  dt = b_theta tau_1 + e_phi tau_2
    const double *bt = U.bth, *be = U.bph;
    double C[6][6];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = i; j < 3; ++j) {
        C[i][j] = S[tri(2 + i, 2 + j)];
        C[3 + i][3 + j] = bt[i] * bt[j] * S[tri(0, 0)] + (bt[i] * be[j] + be[i] * bt[j]) * S[tri(0, 1)] +
                          be[i] * be[j] * S[tri(1, 1)];
      }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) C[i][3 + j] = S[tri(0, 2 + i)] * bt[j] + S[tri(1, 2 + i)] * be[j];
    const double nan = __builtin_nan("");
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = i; j < 6; ++j) {
        const double v = status == PNEC_HIP_COV_OK ? C[i][j] : nan;
        outbuf[kOutCov + 6 * i + j] = v;   // one triangle, stored twice: exactly symmetric
        outbuf[kOutCov + 6 * j + i] = v;
      }
  }
  __syncthreads();

  // coalesced stores: lane k of the first wavefront owns entry k of the block's results
  const int k = threadIdx.x;
  if (k < kOutInfo) {
    if (a.out_cov) a.out_cov[s * 36 + k] = outbuf[k];
  } else if (k < kOutGrad) {
    if (a.out_info) a.out_info[s * 15 + (k - kOutInfo)] = outbuf[k];
  } else if (k < kOutCost) {
    if (a.out_grad) a.out_grad[s * 5 + (k - kOutGrad)] = outbuf[k];
  } else if (k == kOutCost) {
    if (a.out_cost) a.out_cost[s] = outbuf[k];
  } else if (k == kOutDoubles) {
    if (a.out_status) a.out_status[s] = out_st;
  }
}

template <int MODE>
struct PoseCovKernel {
  static constexpr auto run = &pose_covariance_kernel<MODE>;
};

hipError_t launch_pose_covariance(int mode, int64_t n_slots, int waves, const PoseCovArgs &a, hipStream_t stream) {
  return launch_by_mode<PoseCovKernel>(mode, n_slots, waves, a, stream);
}

}  // namespace pnec_hip
