// pnec_pose_cov.hpp -- launch interface of the pose-covariance kernel (pnec_pose_cov.hip), shared with the ABI layer.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

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

struct PoseCovArgs {
  const double *data;
  const int64_t *block_offset;
  const int32_t *count;
  const double *q;       // [S,4] xyzw
  const double *t;       // [S,3]
  int32_t n_hyp;
  double reg;
  double *out_info;      // [S,15] or NULL
  double *out_cov;       // [S,36] or NULL
  double *out_grad;      // [S,5]  or NULL
  double *out_cost;      // [S]    or NULL
  int32_t *out_status;   // [S]    or NULL
};

// one block of `waves` wavefronts per solve slot
hipError_t launch_pose_covariance(int mode, int64_t n_slots, int waves, const PoseCovArgs &a, hipStream_t stream);

}  // namespace pnec_hip
