// pnec_batch_kernels.hpp -- launch interface of the batch layer's utility kernels (pnec_batch_kernels.hip), shared with
// the ABI layer.  Every launcher queues one kernel on `stream` and returns hipGetLastError().
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pnec_hip {

// ingest of pairs [first_pair, first_pair + n_pairs): reference AoS (bvs 3, covs 9 column-major) -> SoA planes; nc = 6,
// 12 or 18 planes, n_max = the largest pair (sizes the grid)
hipError_t launch_pack(int nc, int32_t n_max, double *data, const int64_t *block_offset, const int64_t *offsets,
                       const int32_t *count, int64_t first_pair, int64_t n_pairs, const double *bvs1, const double *bvs2,
                       const double *covs, const double *covs_host, hipStream_t stream);
// the same from both frames' keypoints (pixel positions + 2x2 image covariances), pinhole
hipError_t launch_ingest_keypoints(int nc, int32_t n_max, double *data, const int64_t *block_offset, const int64_t *offsets,
                                   const int32_t *count, int64_t first_pair, int64_t n_pairs, const double *pts1,
                                   const double *pts2, const double *cov2, const double *cov1, const double *K_inv,
                                   double kappa, hipStream_t stream);
// the same shaped on the device, all n_pairs pairs: pair p takes the first min(rows, bound[p]) of the rows
// [src_offsets[p], src_offsets[p + 1]) (cut to [0, n_rows]) and the kernel writes count[p] and out_dropped[p] (may be
// null); n_max = the largest bound (sizes the grid).  n_pairs >= 1.
hipError_t launch_ingest_keypoints_ragged(int nc, int32_t n_max, double *data, const int64_t *block_offset,
                                          const int64_t *src_offsets, const int32_t *bound, int32_t *count,
                                          int32_t *out_dropped, int64_t n_pairs, int64_t n_rows, const double *pts1,
                                          const double *pts2, const double *cov2, const double *cov1, const double *K_inv,
                                          double kappa, hipStream_t stream);
hipError_t launch_unscented(int64_t n, const double *mu, const double *covs, const double *K_inv, double kappa,
                            int camera_model, double *out_bvs, double *out_covs, hipStream_t stream);
// pnec::common::CostFunction of every pair of a TARGET-family batch at its pose
hipError_t launch_cost_function(int64_t n_pairs, const double *data, const int64_t *block_offset, const int32_t *count,
                                const double *qs, const double *ts, double *out, hipStream_t stream);
hipError_t launch_select_best(int64_t n_pairs, int n_hyp, const double *cost, int32_t *best, hipStream_t stream);
// inliers per pair from a correspondence mask (single_offsets: null, or the new batch's offsets when it has ONE pair)
hipError_t launch_mask_count(int64_t n_pairs, const uint8_t *mask, const int64_t *offsets, const int32_t *count,
                             int32_t *out, int64_t *single_offsets, hipStream_t stream);
// exclusive prefix sum of n pair sizes -> AoS offsets [n + 1]
hipError_t launch_offsets_scan(const int32_t *count, int64_t *offsets, int64_t n, hipStream_t stream);

// ---- device self-test (cross-lane reduction, 5x5 solve, lean trigonometry) ------------------
// edge arguments of atan2_c / acos_lean (start_angles' start poses on the axes and the seam); the kernel's results for
// them start at out[kEdgeOut]
constexpr int kAtan2Edges = 26, kAcosEdges = 6, kEdgeOut = 344;
constexpr int kSelftestDoubles = kEdgeOut + kAtan2Edges + kAcosEdges;
__host__ __device__ constexpr double kAtan2EdgeY[kAtan2Edges] = {
    0.0, -0.0, 0.0, -0.0, 0.0, -0.0, 0.0, -0.0, 1.0, 1.0, -1.0, -1.0, 0.0, -0.0, 1e-300, -1e-300,
    1.2246467991473532e-16, -1.2246467991473532e-16, 1.0, -1.0, 1.0, -1.0, 1e-12, -1e-12, 0.0, -0.0};
__host__ __device__ constexpr double kAtan2EdgeX[kAtan2Edges] = {
    0.0, 0.0, -0.0, -0.0, -1.0, -1.0, 1.0, 1.0, 0.0, -0.0, 0.0, -0.0, -2.5, -0.3, -1.0, -1.0,
    -1.0, -1.0, -1.0, -1.0, 1.0, 1.0, -1.0, -1.0, 1e-300, -1e-300};
__host__ __device__ constexpr double kAcosEdge[kAcosEdges] = {1.0, -1.0, 0.0, -0.0, 1.0 - 0x1p-53, -1.0 + 0x1p-53};
// one wavefront; out: kSelftestDoubles doubles
hipError_t launch_selftest(double *out, hipStream_t stream);

}  // namespace pnec_hip
