// pnec_essential_ransac.hpp -- launch interface of the RANSAC forms of the essential-matrix baselines
// (pnec_essential_ransac.hip), shared with the ABI layer.  include/pnec_hip.h (pnec_hip_essential_ransac) has the
// definitions: a counter-based sample per attempt, the model of pnec_hip_essential_minimal / pnec_hip_eight_point on the
// sample, the midpoint score of every correspondence, opengv's sequential rule.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pnec_hip {

struct EssentialRansacArgs {
  const double *data;
  const int64_t *block_offset;
  const int64_t *offsets;      // the caller's correspondence order: where a pair's rows of the mask begin
  const int32_t *count;
  int32_t algorithm;           // PNEC_HIP_EM_NISTER / PNEC_HIP_EM_SEVENPT / PNEC_HIP_EM_EIGHTPT
  int32_t max_iterations;
  uint64_t seed;
  uint64_t first_pair_id;
  double threshold;
  // per pair; each may be NULL
  double *out_q;               // [P,4] xyzw
  double *out_t;               // [P,3] unit
  double *out_E;               // [P,9] the best attempt's chosen solution
  double *out_singular;        // [P,3]
  uint8_t *out_inlier_mask;    // [sum N]
  int32_t *out_inlier_count;   // [P]
  int32_t *out_iterations;     // [P]
  int32_t *out_attempts;       // [P]
  int32_t *out_best_attempt;   // [P]
  int32_t *out_status;         // [P]
};

// one block of one wavefront per pair
hipError_t launch_essential_ransac(int64_t n_pairs, const EssentialRansacArgs &a, hipStream_t stream);

constexpr int kErMaxSample = 9;          // the largest S: 7 + 2 and 8 + 1
constexpr int kErRowStride = 16;         // the gathered sample in LDS: six planes of sixteen
constexpr int kErSkipFactor = 10;        // opengv's max_skip = 10 max_iterations
constexpr double kErProbability = 0.99;  // opengv's probability_

}  // namespace pnec_hip
