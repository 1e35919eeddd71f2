// pnec_eight_point.hip -- the eight-point baseline: essential matrix and pose of every pair from its correspondences
// alone, in one pass.  A translation unit of its own (the solve / stream / front-stage objects do not see it).
// include/pnec_hip.h has the definitions; this file says how the wavefront is used.
//
// One block of one wavefront per pair, as the front stages' sums kernel.  Four phases, every branch wave-uniform; the
// first three are the functions of pnec_essential_shared.hpp, which the minimal solvers' kernel calls too:
//   sums    es_sums: lane l takes correspondences l, l + 64, ...: nine products f1_a f2_b and 45 FMAs into 45
//           accumulators; each accumulator then goes through wave_allreduce_sum (the DPP / permlane butterfly of
//           pnec_device.hpp), always the same tree.  This phase is all of the memory traffic: the six bearing planes,
//           read once.
//   Jacobi  es_jacobi: the 9x9 matrix and the 9x9 eigenvector matrix lie stacked in LDS as one 18x9 array, rows on lanes;
//           no lane waits for another one's arithmetic, nothing is indexed dynamically in registers.
//   SVD     es_decompose: of the 3x3 E through the Jacobi eigen-decomposition of E'E, in registers, every lane the
//           same.
//   choice  sample: lane = 16 * candidate + k triangulates correspondence k < min(9, N) at its candidate (es_term), a DPP
//           row sum per 16 lanes gives the four qualities.  PNEC_HIP_EP_QUALITY_ALL: the lanes stride over all
//           correspondences with four accumulators and the butterfly of the sums reduces them.
// Lane 0 stores the pair's outputs with plain vector stores (es_store_pose and the four qualities).  No atomics; a pair's
// bits depend on its own rows and on `flags` only.
#include <hip/hip_runtime.h>

#include "pnec_device.hpp"
#include "pnec_eight_point.hpp"
#include "pnec_essential_shared.hpp"

namespace pnec_hip {

__global__ __launch_bounds__(kWave) void eight_point_kernel(const EightPointArgs a) {
  __shared__ double M[kEsRows * kEsDim];   // rows 0..8: A'A (full, symmetric), rows 9..17: its eigenvectors as columns

  const int64_t pair = blockIdx.x;
  const int lane = threadIdx.x;
  const int n = to_sgpr(a.count[pair]);
  const EsPair pr = {a.data + a.block_offset[pair], ((int64_t)n + kWave - 1) & ~(int64_t)(kWave - 1)};

  const double nan = __builtin_nan("");
  int status = n < 8 ? PNEC_HIP_EP_TOO_FEW : PNEC_HIP_EP_OK;
  int choice = -1;
  double E[9], sing[3], quality[4], Rc[9], tc[3];
  double gap = nan;
#pragma unroll
  for (int k = 0; k < 9; ++k) E[k] = Rc[k] = nan;
#pragma unroll
  for (int k = 0; k < 3; ++k) sing[k] = tc[k] = nan;
#pragma unroll
  for (int k = 0; k < 4; ++k) quality[k] = nan;

  double trace = 0.0;
  if (status == PNEC_HIP_EP_OK) {
    trace = es_sums(pr, n, lane, M);
    if (!finite_d(trace)) status = PNEC_HIP_EP_NOT_FINITE;
  }
  __syncthreads();

  if (status == PNEC_HIP_EP_OK) {
    es_jacobi(M, trace, lane);

    // ---- the null vector and the gap -----------------------------------------------------------------------------------
    double d[kEsDim];
#pragma unroll
    for (int k = 0; k < kEsDim; ++k) d[k] = M[k * kEsDim + k];
    int imin = 0;
    double lam0 = d[0], lam8 = d[0];
#pragma unroll
    for (int k = 1; k < kEsDim; ++k) {
      if (d[k] < lam0) {
        lam0 = d[k];
        imin = k;
      }
      lam8 = d[k] > lam8 ? d[k] : lam8;
    }
    double lam1 = __builtin_inf();
#pragma unroll
    for (int k = 0; k < kEsDim; ++k) lam1 = (k != imin && d[k] < lam1) ? d[k] : lam1;
    gap = (lam1 - lam0) / lam8;
#pragma unroll
    for (int k = 0; k < 9; ++k) E[k] = M[(kEsDim + k) * kEsDim + imin];
    {
      double nn = 0.0;
#pragma unroll
      for (int k = 0; k < 9; ++k) nn = __builtin_fma(E[k], E[k], nn);
      const double sc = es_sign(E) / sqrt(nn);
#pragma unroll
      for (int k = 0; k < 9; ++k) E[k] *= sc;
    }

    // ---- SVD of E through E'E, the two rotations ----------------------------------------------------------------------
    double u2[3], Ra[9], Rb[9];
    es_decompose(E, sing, u2, Ra, Rb);
    es_signed_rotation(Ra);
    es_signed_rotation(Rb);

    // ---- the choice among (Ra, ta), (Rb, ta), (Ra, -ta), (Rb, -ta) -----------------------------------------------------
    const double tn[3] = {-u2[0], -u2[1], -u2[2]};
    if (a.flags & PNEC_HIP_EP_QUALITY_ALL) {
      double qa[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
      for (int i0_ = 0; i0_ < n; i0_ += kWave) {
        const int i = i0_ + lane;
        const bool in = i < n;
        double f[6];
        pr.load6(in ? i : n - 1, f);
        const double e0 = es_term(f, Ra, u2), e1 = es_term(f, Rb, u2), e2 = es_term(f, Ra, tn), e3 = es_term(f, Rb, tn);
        qa[0] += in ? e0 : 0.0;
        qa[1] += in ? e1 : 0.0;
        qa[2] += in ? e2 : 0.0;
        qa[3] += in ? e3 : 0.0;
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) quality[c] = to_sgpr(wave_allreduce_sum(qa[c]));
    } else {
      const int cand = lane >> 4, k = lane & 15;
      const bool in = k < (n < kEpSample ? n : kEpSample);
      double f[6], R[9], t[3];
      pr.load6(in ? k : 0, f);
#pragma unroll
      for (int j = 0; j < 9; ++j) R[j] = (cand & 1) ? Rb[j] : Ra[j];
#pragma unroll
      for (int j = 0; j < 3; ++j) t[j] = (cand & 2) ? tn[j] : u2[j];
      const double e = es_term(f, R, t);
      const double rs = row_allreduce_sum(in ? e : 0.0);
      quality[0] = read_lane<0>(rs);
      quality[1] = read_lane<16>(rs);
      quality[2] = read_lane<32>(rs);
      quality[3] = read_lane<48>(rs);
    }
    double best = kEsStartQuality;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      quality[c] = finite_d(quality[c]) ? quality[c] : __builtin_inf();
      if (quality[c] < best) {
        best = quality[c];
        choice = c;
      }
    }
    if (choice < 0) {
      status = PNEC_HIP_EP_NO_CANDIDATE;
#pragma unroll
      for (int k = 0; k < 9; ++k) E[k] = nan;
    } else {
#pragma unroll
      for (int k = 0; k < 9; ++k) Rc[k] = (choice & 1) ? Rb[k] : Ra[k];
#pragma unroll
      for (int k = 0; k < 3; ++k) tc[k] = (choice & 2) ? tn[k] : u2[k];
    }
  }

  if (lane == 0) {
    es_store_pose(a, pair, status == PNEC_HIP_EP_OK, Rc, tc, E, sing, gap, choice, status);
    if (a.out_quality) {
#pragma unroll
      for (int k = 0; k < 4; ++k) a.out_quality[4 * pair + k] = quality[k];
    }
  }
}

hipError_t launch_eight_point(int64_t n_pairs, const EightPointArgs &a, hipStream_t stream) {
  hipLaunchKernelGGL(eight_point_kernel, dim3((unsigned)n_pairs), dim3(kWave), 0, stream, a);
  return hipGetLastError();
}

}  // namespace pnec_hip
