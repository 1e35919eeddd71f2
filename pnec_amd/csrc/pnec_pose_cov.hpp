// pnec_pose_cov.hpp -- launch interface of the pose-covariance kernel (pnec_pose_cov.hip), shared with the ABI layer.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pnec_pose_pass.hpp"   // cov_waves: the wavefronts of a pair follow from its own count

namespace pnec_hip {

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
