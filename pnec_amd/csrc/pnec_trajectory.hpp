// pnec_trajectory.hpp -- launch interface of the trajectory kernels (pnec_trajectory.hip), shared with the ABI layer.
// include/pnec_hip.h has the definitions: pnec_hip_trajectory_compose (relative poses to a trajectory per sequence) and
// pnec_hip_trajectory_metrics (RPE_1, RPE_n, L1RPE_1, L1RPE_n, r_t of a trajectory against ground truth), and
// pnec_hip_trajectory_advance (one frame's step of a running scale and pose).
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

// one frame's step of the running scale and pose of n_seq sequences (pnec_hip_trajectory_advance)
struct TrajectoryAdvanceArgs {
  int64_t n_seq;
  const double *rel_q;      // [n_seq,4] xyzw
  const double *rel_t;      // [n_seq,3]
  const int32_t *count;     // [n_seq] or NULL
  int32_t min_count;
  const double *scale3;     // [n_seq,3] or NULL: quartile, median, quartile; the median is read
  const int32_t *n_used;    // [n_seq] or NULL (needs scale3)
  int32_t min_used;
  const double *s, *q, *p;  // the state: [n_seq], [n_seq,4], [n_seq,3]
  double *next_s, *next_q, *next_p;
  int32_t *out_status;      // [n_seq] or NULL
};

// one lane per sequence; n_seq >= 1
hipError_t launch_trajectory_advance(const TrajectoryAdvanceArgs &a, hipStream_t stream);

// one wavefront per sequence; n_seq >= 1, n_rows >= 1
hipError_t launch_trajectory_compose(const TrajectoryComposeArgs &a, hipStream_t stream);
// three launches: the error rotations (one lane per row), the distances (one wavefront per row), the metrics (one
// wavefront per sequence); n_seq >= 1, n_rows >= 0 (no rows: the last launch alone, which writes NaN)
hipError_t launch_trajectory_metrics(const TrajectoryMetricsArgs &a, hipStream_t stream);

constexpr int kTrajectoryWave = 64;   // a lane's chunk in the composition is ceil(L / 64) rows; a diagonal is walked 64 pairs at a time

}  // namespace pnec_hip
