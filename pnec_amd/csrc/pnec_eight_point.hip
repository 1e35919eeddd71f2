// pnec_eight_point.hip -- the eight-point baseline: essential matrix and pose of every pair from its correspondences
// alone, in one pass.  A translation unit of its own (the solve / stream / front-stage objects do not see it).
// include/pnec_hip.h has the definitions; this file says how the wavefront is used.
//
// One block of one wavefront per pair, as the front stages' sums kernel.  Four phases, every branch wave-uniform; the
// first is es_sums of pnec_essential_shared.hpp, the other three are ep_model of pnec_essential_model.hpp, which the
// RANSAC kernel calls once per attempt:
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
#include "pnec_essential_model.hpp"
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
    const bool all = a.flags & PNEC_HIP_EP_QUALITY_ALL;
    const int K = all ? n : (n < kEpSample ? n : kEpSample);
    status = model::ep_model(pr, K, all, lane, M, trace, gap, choice, quality, E, sing, Rc, tc);
    if (status != PNEC_HIP_EP_OK) {
#pragma unroll
      for (int k = 0; k < 9; ++k) E[k] = nan;
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
