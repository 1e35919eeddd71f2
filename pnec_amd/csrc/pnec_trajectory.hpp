// pnec_trajectory.hpp -- launch interface of the trajectory kernels (pnec_trajectory.hip), shared with the ABI layer.
// include/pnec_hip.h has the definitions: pnec_hip_trajectory_compose (relative poses to a trajectory per sequence) and
// pnec_hip_trajectory_metrics (RPE_1, RPE_n, L1RPE_1, L1RPE_n, r_t of a trajectory against ground truth).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pnec_hip {

// rows are sequence-major; sequence f is rows lo .. hi of the cut lo = clamp(offsets[f], 0, n_rows),
// hi = clamp(offsets[f + 1], lo, n_rows)
struct TrajectoryComposeArgs {
  int64_t n_seq, n_rows;
  const int64_t *offsets;   // [n_seq + 1]
  const double *rel_q;      // [n_rows,4] xyzw
  const double *rel_t;      // [n_rows,3] or NULL
  const double *scale;      // [n_rows] or NULL (needs rel_t)
  const double *q0;         // [n_seq,4] or NULL
  const double *p0;         // [n_seq,3] or NULL (needs rel_t)
  double *out_q;            // [n_rows,4]
  double *out_p;            // [n_rows,3], exactly when rel_t
  uint8_t *out_valid;       // [n_rows] or NULL
};

struct TrajectoryMetricsArgs {
  int64_t n_seq, n_rows;
  const int64_t *offsets;        // [n_seq + 1]
  const double *est_q, *gt_q;    // [n_rows,4] xyzw
  const double *est_p, *gt_p;    // [n_rows,3], both or neither
  double *out_metrics;           // [n_seq,5]
  double *out_err_q;             // [n_rows,4]
  double *out_rmse_d, *out_l1_d; // [n_rows]
  double *out_angle1, *out_rt1;  // [n_rows] or NULL
};

// one wavefront per sequence; n_seq >= 1, n_rows >= 1
hipError_t launch_trajectory_compose(const TrajectoryComposeArgs &a, hipStream_t stream);
// three launches: the error rotations (one lane per row), the distances (one wavefront per row), the metrics (one
// wavefront per sequence); n_seq >= 1, n_rows >= 0 (no rows: the last launch alone, which writes NaN)
hipError_t launch_trajectory_metrics(const TrajectoryMetricsArgs &a, hipStream_t stream);

constexpr int kTrajectoryWave = 64;   // a lane's chunk in the composition is ceil(L / 64) rows; a diagonal is walked 64 pairs at a time

}  // namespace pnec_hip
