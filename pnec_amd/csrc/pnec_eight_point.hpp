// pnec_eight_point.hpp -- launch interface of the eight-point kernel (pnec_eight_point.hip), shared with the ABI layer.
// include/pnec_hip.h (pnec_hip_eight_point) has the definitions: the 45 sums of A'A, the null vector by cyclic Jacobi, the
// decomposition of E into four poses and the choice among them by reprojection of triangulated points.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pnec_hip {

struct EightPointArgs {
  const double *data;
  const int64_t *block_offset;
  const int32_t *count;
  int32_t flags;               // PNEC_HIP_EP_QUALITY_ALL
  // per pair; each may be NULL
  double *out_q;               // [P,4] xyzw
  double *out_t;               // [P,3] unit
  double *out_E;               // [P,9] row-major
  double *out_singular;        // [P,3]
  double *out_gap;             // [P]
  double *out_quality;         // [P,4]
  int32_t *out_choice;         // [P]
  int32_t *out_status;         // [P]
};

// one block of one wavefront per pair
hipError_t launch_eight_point(int64_t n_pairs, const EightPointArgs &a, hipStream_t stream);

// (the Jacobi iteration's constants and the start quality: pnec_essential_shared.hpp)
constexpr int kEpSample = 9;              // the reference's sampleSize for EIGHTPT: 8 + 1 (common.cc:378)

}  // namespace pnec_hip
