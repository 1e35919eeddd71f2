// pnec_batch_kernels.hip -- the batch layer's utility kernels: ingest (reference AoS -> SoA planes, from bearings or
// from keypoints), covariance propagation, CostFunction, best hypothesis, mask counts, offsets scan, device self-test;
// and their launchers (pnec_batch_kernels.hpp).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "pnec_batch_kernels.hpp"
#include "pnec_solve_kernel.hpp"   // (the self-test exercises its lean trigonometry)

using namespace pnec_hip;

namespace {

// ---- ingest: reference AoS (bvs 3, covs 9 column-major) -> SoA planes --------------------
template <int NC>
__global__ __launch_bounds__(256) void pack_kernel(double *__restrict__ data,
                                                   const int64_t *__restrict__ block_offset,
                                                   const int64_t *__restrict__ offsets,
                                                   const int32_t *__restrict__ count,
                                                   int64_t first_pair, int64_t n_pairs,
                                                   const double *__restrict__ bvs1,
                                                   const double *__restrict__ bvs2,
                                                   const double *__restrict__ covs,
                                                   const double *__restrict__ covs_host) {
  const int64_t src0 = offsets[first_pair];
  for (int64_t p = first_pair + blockIdx.y; p < first_pair + n_pairs; p += gridDim.y) {
    const int n = count[p];
    const int stride = (n + kWave - 1) & ~(kWave - 1);
    double *blk = data + block_offset[p];
    const int64_t src = offsets[p] - src0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < stride; i += gridDim.x * blockDim.x) {
      const bool in = i < n;
      const int64_t j = src + i;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        blk[(int64_t)c * stride + i] = in ? bvs1[3 * j + c] : 0.0;
        blk[(int64_t)(3 + c) * stride + i] = in ? bvs2[3 * j + c] : 0.0;
      }
      if constexpr (NC >= 12) {
        // symmetric part of the column-major 3x3: (r,c) at 3*c + r
        const double *C = covs + 9 * j;
        blk[(int64_t)6 * stride + i] = in ? C[0] : 0.0;
        blk[(int64_t)7 * stride + i] = in ? 0.5 * (C[1] + C[3]) : 0.0;
        blk[(int64_t)8 * stride + i] = in ? 0.5 * (C[2] + C[6]) : 0.0;
        blk[(int64_t)9 * stride + i] = in ? C[4] : 0.0;
        blk[(int64_t)10 * stride + i] = in ? 0.5 * (C[5] + C[7]) : 0.0;
        blk[(int64_t)11 * stride + i] = in ? C[8] : 0.0;
      }
      if constexpr (NC >= 18) {
        const double *C = covs_host + 9 * j;
        blk[(int64_t)12 * stride + i] = in ? C[0] : 0.0;
        blk[(int64_t)13 * stride + i] = in ? 0.5 * (C[1] + C[3]) : 0.0;
        blk[(int64_t)14 * stride + i] = in ? 0.5 * (C[2] + C[6]) : 0.0;
        blk[(int64_t)15 * stride + i] = in ? C[4] : 0.0;
        blk[(int64_t)16 * stride + i] = in ? 0.5 * (C[5] + C[7]) : 0.0;
        blk[(int64_t)17 * stride + i] = in ? C[8] : 0.0;
      }
    }
  }
}

// ---- best hypothesis per pair ------------------------------------------------------------
__global__ void select_best_kernel(int64_t n_pairs, int n_hyp, const double *__restrict__ cost,
                                   int32_t *__restrict__ best) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_pairs) return;
  int bi = 0;
  double bc = cost[p * n_hyp];
  for (int h = 1; h < n_hyp; ++h) {
    const double c = cost[p * n_hyp + h];
    // NaN never wins; first NaN-free minimum wins ties
    if (c < bc || (bc != bc && c == c)) {
      bc = c;
      bi = h;
    }
  }
  best[p] = bi;
}

// ---- pnec::common::CostFunction (common.cc:237-259), one wavefront per pair ---------------
__global__ __launch_bounds__(kWave) void cost_function_kernel(const double *__restrict__ data,
                                                              const int64_t *__restrict__ block_offset,
                                                              const int32_t *__restrict__ count,
                                                              const double *__restrict__ qs,
                                                              const double *__restrict__ ts,
                                                              double *__restrict__ out) {
  const int64_t p = blockIdx.x;
  const int lane = threadIdx.x;
  const int n = count[p];
  const int stride = (n + kWave - 1) & ~(kWave - 1);
  const double *base = data + block_offset[p];
  double q[4] = {qs[4 * p], qs[4 * p + 1], qs[4 * p + 2], qs[4 * p + 3]};
  const double qn = 1.0 / sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
#pragma unroll
  for (int k = 0; k < 4; ++k) q[k] *= qn;
  double R[9];
  rot_from_quat(q, R);
  const double tx = ts[3 * p], ty = ts[3 * p + 1], tz = ts[3 * p + 2];
  double acc = 0.0;
  for (int i = lane; i < n; i += kWave) {
    double d[12];
#pragma unroll
    for (int c = 0; c < 12; ++c) d[c] = base[(int64_t)c * stride + i];
    const double mx = ty * d[2] - tz * d[1], my = tz * d[0] - tx * d[2], mz = tx * d[1] - ty * d[0];
    const double gx = R[0] * mx + R[3] * my + R[6] * mz;
    const double gy = R[1] * mx + R[4] * my + R[7] * mz;
    const double gz = R[2] * mx + R[5] * my + R[8] * mz;
    const double nn = d[3] * gx + d[4] * gy + d[5] * gz;
    const double sgx = d[6] * gx + d[7] * gy + d[8] * gz;
    const double sgy = d[7] * gx + d[9] * gy + d[10] * gz;
    const double sgz = d[8] * gx + d[10] * gy + d[11] * gz;
    acc += nn * nn / (gx * sgx + gy * sgy + gz * sgz);
  }
  acc = wave_allreduce_sum(acc);
  if (lane == 0) out[p] = acc / (double)n;
}

// ---- covariance propagation: pnec::common::UnscentedTransform + Unproject -----------------
// (src/common/common.cc:460-525; 5 sigma points, kappa-weighted).  All matrices column-major like
// Eigen.  camera_model: 0 omnidirectional, 1 pinhole.  One function shared by the stand-alone kernel and
// the fused keypoint ingest, compiled WITHOUT floating-point contraction so that both produce the same
// bits whatever code surrounds the call (the ingest test compares them bitwise).
//   m:  the image point (x, y, 1) [or (x, y, f) with K_inv = I];  c0, c1: the two columns added to /
//   subtracted from it (columns of the covariance's Cholesky factor).
__device__ __forceinline__ void unscented_core(const double (&m)[3], const double (&c0)[3], const double (&c1)[3],
                                               const double (&K)[9], double kappa, int camera_model,
                                               double (&bearing)[3], double (&S)[9]) {
#pragma clang fp contract(off)
  const double w0 = kappa / (2.0 + kappa), wi = 0.5 / (2.0 + kappa);
  double tp[5][3], mean[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int p = 0; p < 5; ++p) {
    const double sg = (p == 0) ? 0.0 : (p <= 2 ? 1.0 : -1.0);
    const double *col = (p == 1 || p == 3) ? c0 : c1;
    const double x = m[0] + sg * col[0], y = m[1] + sg * col[1], z = m[2] + sg * col[2];
    double tx = x, ty = y, tz = z;
    if (camera_model != 0) {
      tx = K[0] * x + K[3] * y + K[6] * z;
      ty = K[1] * x + K[4] * y + K[7] * z;
      tz = K[2] * x + K[5] * y + K[8] * z;
    }
    const double nn = 1.0 / sqrt(tx * tx + ty * ty + tz * tz);
    tp[p][0] = tx * nn; tp[p][1] = ty * nn; tp[p][2] = tz * nn;
    const double w = (p == 0) ? w0 : wi;
#pragma unroll
    for (int k = 0; k < 3; ++k) mean[k] += w * tp[p][k];
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) S[k] = 0.0;
#pragma unroll
  for (int p = 0; p < 5; ++p) {
    const double w = (p == 0) ? w0 : wi;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) S[3 * c + r] += w * (tp[p][r] - mean[r]) * (tp[p][c] - mean[c]);
  }
  // (w a_r) a_c and (w a_c) a_r round differently unless w is a power of two: both mirror entries get their mean, so that
  // the matrix handed out is exactly symmetric.  The mean is what the ingest kernels' 0.5 * (S_rc + S_cr) stored anyway.
  S[1] = S[3] = 0.5 * (S[1] + S[3]);
  S[2] = S[6] = 0.5 * (S[2] + S[6]);
  S[5] = S[7] = 0.5 * (S[5] + S[7]);
#pragma unroll
  for (int k = 0; k < 3; ++k) bearing[k] = tp[0][k];  // normalised (K^-1) mu = Unproject
}
// the pinhole branch's sigma-point offsets: columns of the lower Cholesky factor of the image-plane
// covariance [[a, b], [b, d]] (common.cc:488-489)
__device__ __forceinline__ void pinhole_columns(double a, double b, double d, double (&c0)[3], double (&c1)[3]) {
#pragma clang fp contract(off)
  const double l00 = sqrt(a), l10 = b / l00, l11 = sqrt(d - l10 * l10);
  c0[0] = l00; c0[1] = l10; c0[2] = 0.0;
  c1[0] = 0.0; c1[1] = l11; c1[2] = 0.0;
}

__global__ __launch_bounds__(256) void unscented_kernel(int64_t n, const double *__restrict__ mu,
                                                        const double *__restrict__ covs,
                                                        const double *__restrict__ K_inv_, double kappa,
                                                        int camera_model, double *__restrict__ out_bvs,
                                                        double *__restrict__ out_covs) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double K[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) K[k] = K_inv_[k];
  const double m[3] = {mu[3 * i], mu[3 * i + 1], mu[3 * i + 2]};
  const double *C9 = covs + 9 * i;
  double c0[3], c1[3];  // the two columns added to / subtracted from mu
  if (camera_model == 0) {
    // rotation taking (0,0,1) to the bearing (RotationBetweenPoints, common.cc:118-124)
    const double nm = fast_rsqrt(m[0] * m[0] + m[1] * m[1] + m[2] * m[2]);
    const double vx = m[0] * nm, vy = m[1] * nm, vz = m[2] * nm;
    const double cx = -vy, cy = vx;  // (0,0,1) x v = (-vy, vx, 0)
    double R[9];                     // column-major
    const double f = 1.0 / (1.0 + vz);
    // K = skew(c) = [[0,0,cy],[0,0,-cx],[-cy,cx,0]];  R = I + K + K^2 f
    R[0] = 1.0 - cy * cy * f; R[3] = cx * cy * f;       R[6] = cy;
    R[1] = cx * cy * f;       R[4] = 1.0 - cx * cx * f; R[7] = -cx;
    R[2] = -cy;               R[5] = cx;                R[8] = 1.0 - (cx * cx + cy * cy) * f;
    // local = (R' cov R) top-left 2x2
    double T[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) T[3 * c + r] = C9[r] * R[3 * c] + C9[3 + r] * R[3 * c + 1] + C9[6 + r] * R[3 * c + 2];
    const double a = R[0] * T[0] + R[1] * T[1] + R[2] * T[2];
    const double b = R[3] * T[0] + R[4] * T[1] + R[5] * T[2];
    const double d = R[3] * T[3] + R[4] * T[4] + R[5] * T[5];
    const double l00 = sqrt(a), l10 = b / l00, l11 = sqrt(d - l10 * l10);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      c0[r] = R[r] * l00 + R[3 + r] * l10;
      c1[r] = R[3 + r] * l11;
    }
  } else {
    pinhole_columns(C9[0], C9[1], C9[4], c0, c1);
  }
  double bearing[3], S[9];
  unscented_core(m, c0, c1, K, kappa, camera_model, bearing, S);
#pragma unroll
  for (int k = 0; k < 9; ++k) out_covs[9 * i + k] = S[k];
  if (out_bvs) {
#pragma unroll
    for (int k = 0; k < 3; ++k) out_bvs[3 * i + k] = bearing[k];
  }
}

// ---- fused keypoint ingest: KeyPoint::Unproject (src/frames/keypoints.cc:49-62) for both frames'
// keypoints -- bearing = normalised K^-1 (u, v, 1), covariance = UnscentedTransform of the 2x2 image
// covariance, kappa = 1, pinhole -- written straight into the batch's SoA planes.  Per correspondence the
// device reads 56 B (two pixel positions, one symmetric 2x2) instead of the 120 B of ready-made bearings
// + 3x3 covariance, and the AoS covariances never exist in HBM.  Same bits as unscented_kernel followed
// by pack_kernel (both call unscented_core; the 3x3 it returns is exactly symmetric, so pack_kernel's
// symmetrisation is the identity on it).
template <int NC>
__global__ __launch_bounds__(256) void ingest_keypoints_kernel(double *__restrict__ data,
                                                               const int64_t *__restrict__ block_offset,
                                                               const int64_t *__restrict__ offsets,
                                                               const int32_t *__restrict__ count, int64_t first_pair,
                                                               int64_t n_pairs, const double *__restrict__ pts1,
                                                               const double *__restrict__ pts2,
                                                               const double *__restrict__ cov2,
                                                               const double *__restrict__ cov1,
                                                               const double *__restrict__ K_inv_, double kappa) {
  double K[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) K[k] = K_inv_[k];
  const int64_t src0 = offsets[first_pair];
  const double zero3[3] = {0.0, 0.0, 0.0};
  for (int64_t p = first_pair + blockIdx.y; p < first_pair + n_pairs; p += gridDim.y) {
    const int n = count[p];
    const int stride = (n + kWave - 1) & ~(kWave - 1);
    double *blk = data + block_offset[p];
    const int64_t src = offsets[p] - src0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < stride; i += gridDim.x * blockDim.x) {
      const bool in = i < n;
      const int64_t j = in ? src + i : src;  // a valid address for the padding lanes
      double b1[3], b2[3], S2[9], S1[9];
      {
        const double m[3] = {pts2[2 * j], pts2[2 * j + 1], 1.0};
        double c0[3], c1[3];
        if constexpr (NC >= 12) pinhole_columns(cov2[3 * j], cov2[3 * j + 1], cov2[3 * j + 2], c0, c1);
        else { c0[0] = c0[1] = c0[2] = c1[0] = c1[1] = c1[2] = 0.0; }
        unscented_core(m, c0, c1, K, kappa, 1, b2, S2);
      }
      {
        const double m[3] = {pts1[2 * j], pts1[2 * j + 1], 1.0};
        if constexpr (NC >= 18) {
          double c0[3], c1[3];
          pinhole_columns(cov1[3 * j], cov1[3 * j + 1], cov1[3 * j + 2], c0, c1);
          unscented_core(m, c0, c1, K, kappa, 1, b1, S1);
        } else {
          unscented_core(m, zero3, zero3, K, kappa, 1, b1, S1);  // only the bearing is kept
        }
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        blk[(int64_t)c * stride + i] = in ? b1[c] : 0.0;
        blk[(int64_t)(3 + c) * stride + i] = in ? b2[c] : 0.0;
      }
      if constexpr (NC >= 12) {
        blk[(int64_t)6 * stride + i] = in ? S2[0] : 0.0;
        blk[(int64_t)7 * stride + i] = in ? 0.5 * (S2[1] + S2[3]) : 0.0;
        blk[(int64_t)8 * stride + i] = in ? 0.5 * (S2[2] + S2[6]) : 0.0;
        blk[(int64_t)9 * stride + i] = in ? S2[4] : 0.0;
        blk[(int64_t)10 * stride + i] = in ? 0.5 * (S2[5] + S2[7]) : 0.0;
        blk[(int64_t)11 * stride + i] = in ? S2[8] : 0.0;
      }
      if constexpr (NC >= 18) {
        blk[(int64_t)12 * stride + i] = in ? S1[0] : 0.0;
        blk[(int64_t)13 * stride + i] = in ? 0.5 * (S1[1] + S1[3]) : 0.0;
        blk[(int64_t)14 * stride + i] = in ? 0.5 * (S1[2] + S1[6]) : 0.0;
        blk[(int64_t)15 * stride + i] = in ? S1[4] : 0.0;
        blk[(int64_t)16 * stride + i] = in ? 0.5 * (S1[5] + S1[7]) : 0.0;
        blk[(int64_t)17 * stride + i] = in ? S1[8] : 0.0;
      }
    }
  }
}

// ---- the same ingest shaped on the device: pair p's rows are [src_offsets[p], src_offsets[p + 1]) of the caller's
// arrays, cut to [0, n_rows] (as pnec_tracks.hpp's tracks_range cuts a set's), and the pair keeps the first
// min(rows, bound[p]) of them inside the block its bound reserved.  It differs from ingest_keypoints_kernel in three
// things: the source offsets are the caller's (the batch's own compact offsets come from the scan that follows), the
// count is computed here, and one lane per pair stores it and what the bound turned away.  Every block derives the count
// from src_offsets and bound: `count` and `out_dropped` are written and never read, so no lane reads a word that a lane
// of this launch writes.  No wavefront-wide operation: lanes diverge freely.
template <int NC>
__global__ __launch_bounds__(256) void ingest_keypoints_ragged_kernel(double *__restrict__ data,
                                                                      const int64_t *__restrict__ block_offset,
                                                                      const int64_t *__restrict__ src_offsets,
                                                                      const int32_t *__restrict__ bound,
                                                                      int32_t *__restrict__ count,
                                                                      int32_t *__restrict__ out_dropped, int64_t n_pairs,
                                                                      int64_t n_rows, const double *__restrict__ pts1,
                                                                      const double *__restrict__ pts2,
                                                                      const double *__restrict__ cov2,
                                                                      const double *__restrict__ cov1,
                                                                      const double *__restrict__ K_inv_, double kappa) {
  double K[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) K[k] = K_inv_[k];
  const double zero3[3] = {0.0, 0.0, 0.0};
  for (int64_t p = blockIdx.y; p < n_pairs; p += gridDim.y) {
    int64_t lo = src_offsets[p], hi = src_offsets[p + 1];
    lo = lo < 0 ? 0 : (lo > n_rows ? n_rows : lo);
    hi = hi < lo ? lo : (hi > n_rows ? n_rows : hi);
    const int64_t room = bound[p] > 0 ? bound[p] : 0;
    const int n = (int)(hi - lo < room ? hi - lo : room);
    const int stride = (n + kWave - 1) & ~(kWave - 1);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      count[p] = n;
      if (out_dropped) out_dropped[p] = (int32_t)(hi - lo - n);
    }
    double *blk = data + block_offset[p];
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < stride; i += gridDim.x * blockDim.x) {
      const bool in = i < n;
      const int64_t j = in ? lo + i : lo;  // a valid address for the padding lanes (n > 0 here, so lo < n_rows)
      double b1[3], b2[3], S2[9], S1[9];
      {
        const double m[3] = {pts2[2 * j], pts2[2 * j + 1], 1.0};
        double c0[3], c1[3];
        if constexpr (NC >= 12) pinhole_columns(cov2[3 * j], cov2[3 * j + 1], cov2[3 * j + 2], c0, c1);
        else { c0[0] = c0[1] = c0[2] = c1[0] = c1[1] = c1[2] = 0.0; }
        unscented_core(m, c0, c1, K, kappa, 1, b2, S2);
      }
      {
        const double m[3] = {pts1[2 * j], pts1[2 * j + 1], 1.0};
        if constexpr (NC >= 18) {
          double c0[3], c1[3];
          pinhole_columns(cov1[3 * j], cov1[3 * j + 1], cov1[3 * j + 2], c0, c1);
          unscented_core(m, c0, c1, K, kappa, 1, b1, S1);
        } else {
          unscented_core(m, zero3, zero3, K, kappa, 1, b1, S1);  // only the bearing is kept
        }
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        blk[(int64_t)c * stride + i] = in ? b1[c] : 0.0;
        blk[(int64_t)(3 + c) * stride + i] = in ? b2[c] : 0.0;
      }
      if constexpr (NC >= 12) {
        blk[(int64_t)6 * stride + i] = in ? S2[0] : 0.0;
        blk[(int64_t)7 * stride + i] = in ? 0.5 * (S2[1] + S2[3]) : 0.0;
        blk[(int64_t)8 * stride + i] = in ? 0.5 * (S2[2] + S2[6]) : 0.0;
        blk[(int64_t)9 * stride + i] = in ? S2[4] : 0.0;
        blk[(int64_t)10 * stride + i] = in ? 0.5 * (S2[5] + S2[7]) : 0.0;
        blk[(int64_t)11 * stride + i] = in ? S2[8] : 0.0;
      }
      if constexpr (NC >= 18) {
        blk[(int64_t)12 * stride + i] = in ? S1[0] : 0.0;
        blk[(int64_t)13 * stride + i] = in ? 0.5 * (S1[1] + S1[3]) : 0.0;
        blk[(int64_t)14 * stride + i] = in ? 0.5 * (S1[2] + S1[6]) : 0.0;
        blk[(int64_t)15 * stride + i] = in ? S1[4] : 0.0;
        blk[(int64_t)16 * stride + i] = in ? 0.5 * (S1[5] + S1[7]) : 0.0;
        blk[(int64_t)17 * stride + i] = in ? S1[8] : 0.0;
      }
    }
  }
}

// ---- inliers per pair from a correspondence mask ----------------------------------------------
__global__ __launch_bounds__(kWave) void mask_count_kernel(const uint8_t *__restrict__ mask,
                                                           const int64_t *__restrict__ offsets,
                                                           const int32_t *__restrict__ count,
                                                           int32_t *__restrict__ out,
                                                           int64_t *__restrict__ single_offsets /* null, or the
                                                           new batch's offsets when it has ONE pair: the scan of one
                                                           count is the count (a launch less per frame) */) {
  const int64_t p = blockIdx.x;
  const int n = count[p];
  int c = 0;
  for (int i = threadIdx.x; i < n; i += kWave) c += mask[offsets[p] + i] != 0;
  c = (int)wave_allreduce_sum((double)c);
  if (threadIdx.x == 0) {
    out[p] = c;
    if (single_offsets) {
      single_offsets[0] = 0;
      single_offsets[1] = c;
    }
  }
}

// exclusive prefix sum of the pair sizes -> AoS offsets [n+1] (one workgroup; n is at most a few 1e5).  Segments of
// 32 x 1024 pairs: each thread takes up to 32 consecutive sizes, ALL of them requested before the first is used; the 1024
// partial sums are scanned by shuffles inside the sixteen wavefronts + one scan of their totals.  (Until round 6: one
// dependent load after the other per thread, twice, and thread 0 walking the 1024 partial sums alone -- ~40 us on the
// chain's critical path in every call.)
__global__ __launch_bounds__(1024) void offsets_scan_kernel(const int32_t *__restrict__ count,
                                                            int64_t *__restrict__ offsets, int64_t n) {
  constexpr int kPer = 32;
  __shared__ long long wave_tot[17];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  long long carry = 0;
  for (int64_t seg = 0; seg < n; seg += (int64_t)kPer * 1024) {
    const int64_t m = std::min<int64_t>(n - seg, (int64_t)kPer * 1024);
    const int64_t per = (m + 1023) / 1024, a = seg + std::min<int64_t>(m, per * t), b = seg + std::min<int64_t>(m, per * (t + 1));
    int32_t c[kPer];
#pragma unroll
    for (int k = 0; k < kPer; ++k) c[k] = (a + k < b) ? count[a + k] : 0;
    long long sacc = 0;
#pragma unroll
    for (int k = 0; k < kPer; ++k) sacc += c[k];
    long long inc = sacc;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const long long o = __shfl_up(inc, d, 64);
      if (lane >= d) inc += o;
    }
    __syncthreads();   // (the previous segment's totals have been read)
    if (lane == 63) wave_tot[wave] = inc;
    __syncthreads();
    if (wave == 0) {
      const long long w = lane < 16 ? wave_tot[lane] : 0ll;
      long long winc = w;
#pragma unroll
      for (int d = 1; d < 16; d <<= 1) {
        const long long o = __shfl_up(winc, d, 64);
        if (lane >= d) winc += o;
      }
      if (lane < 16) wave_tot[lane] = winc - w;
      if (lane == 15) wave_tot[16] = winc;
    }
    __syncthreads();
    long long run = carry + wave_tot[wave] + inc - sacc;
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
      if (a + k < b) offsets[a + k] = run;
      run += c[k];
    }
    carry += wave_tot[16];
  }
  if (t == 0) offsets[n] = carry;
}

// ---- device self-test kernels (cross-lane reduction, 5x5 solve) ---------------------------
__global__ void selftest_kernel(double *out) {
  const int lane = threadIdx.x;
  // sum of (lane+1)^2 over 64 lanes = 89440; every lane must hold it
  const double v = wave_allreduce_sum((double)((lane + 1) * (lane + 1)));
  out[lane] = v;
  if (lane == 0) {
    // A = M M' + I for a fixed M; solve A y = b and report the residual norm
    double P[15], b[5], y[5];
    double M[5][5];
    for (int i = 0; i < 5; ++i)
      for (int j = 0; j < 5; ++j) M[i][j] = sin(1.0 + i * 1.7 + j * 0.9);
    for (int i = 0; i < 5; ++i)
      for (int j = i; j < 5; ++j) {
        double sacc = (i == j) ? 1.0 : 0.0;
        for (int k = 0; k < 5; ++k) sacc += M[i][k] * M[j][k];
        P[tri(i, j)] = sacc;
      }
    for (int i = 0; i < 5; ++i) b[i] = 1.0 + i;
    const bool ok = chol_solve5(P, b, y);
    double res = 0.0;
    for (int i = 0; i < 5; ++i) {
      double sacc = -b[i];
      for (int j = 0; j < 5; ++j) sacc += P[sym(i, j)] * y[j];
      res += sacc * sacc;
    }
    out[64] = ok ? sqrt(res) : -1.0;
    out[65] = fast_rsqrt(2.0) - 0.70710678118654752440;
    out[66] = fast_rcp(3.0) - 0.33333333333333333333;
  }
  {
    // the same system solved across lanes (gj_solve5_rows: lane i of every 16-lane row owns row i) with a damped
    // diagonal, against chol_solve5 on the damped matrix; and the 64-bit row broadcast on its own
    double P[15], bb[5], y[5];
    double M[5][5];
    for (int i = 0; i < 5; ++i)
      for (int j = 0; j < 5; ++j) M[i][j] = sin(1.0 + i * 1.7 + j * 0.9);
    for (int i = 0; i < 5; ++i)
      for (int j = i; j < 5; ++j) {
        double sacc = (i == j) ? 1.0 : 0.0;
        for (int k = 0; k < 5; ++k) sacc += M[i][k] * M[j][k];
        P[tri(i, j)] = sacc;
      }
    for (int i = 0; i < 5; ++i) bb[i] = 1.0 + i;
    const int li = lane & 15;
    double A[5], rhs = 0.0, damp = 0.0;
    for (int k = 0; k < 5; ++k) A[k] = 0.0;
    for (int i = 0; i < 5; ++i)
      if (li == i) {
        for (int k = 0; k < 5; ++k) A[k] = P[sym(i, k)];
        rhs = bb[i];
        damp = 0.25 * (i + 1);
      }
    for (int i = 0; i < 5; ++i) P[tri(i, i)] += 0.25 * (i + 1);
    const bool ok_rows = gj_solve5_rows(A, damp, rhs, li);
    const bool ok_chol = chol_solve5(P, bb, y);
    double dev = 0.0;
    for (int i = 0; i < 5; ++i)
      if (li == i) dev = fabs(rhs - y[i]) / fabs(y[i]);
    out[216 + lane] = (ok_rows && ok_chol && li < 5) ? dev : ((ok_rows && ok_chol) ? 0.0 : -1.0);
    out[280 + lane] = bcast_row<11>(1000.0 + lane);  // must be 1011 + 16 * (lane / 16)
  }
  // 21-way swap-halving reduction: acc[j] = (lane+1)(j+1) + j  ->  2080 (j+1) + 64 j
  double acc[kNumAcc], sums[kNumAcc];
  for (int j = 0; j < kNumAcc; ++j) acc[j] = (double)((lane + 1) * (j + 1) + j);
  wave_reduce21(acc, sums);
  if (lane == 0)
    for (int j = 0; j < kNumAcc; ++j) out[67 + j] = sums[j];
  // lean acos / atan2 against libm: a grid over the circle and over [-1, 1] with dense ends
  {
    double worst_a = 0.0;
    for (int k = 0; k < 64; ++k) {
      const int i = lane * 64 + k;
      const double ang = -3.14159 + 6.28318 * i / 4095.0;
      const double yy = sin(ang) * (1.0 + (i % 7)), xx = cos(ang) * (1.0 + (i % 7));
      worst_a = fmax(worst_a, fabs(atan2_lean(yy, xx) - atan2(yy, xx)));
      const double u = (double)i / 4095.0;
      const double c = (i & 1) ? 1.0 - u * u * u * u : -1.0 + u * u * u * u;   // clusters at +-1
      const double ref = acos(c);
      worst_a = fmax(worst_a, fabs(acos_lean(c) - ref) / fmax(ref, 1e-300));
    }
    out[152 + lane] = worst_a;
  }
  // atan2_c / acos_lean at the signed zeros, the axes and the +-pi seam, where C fixes the sign of the result too
  // (the host compares value AND sign bit with its own libm: pnec_hip_selftest)
  if (lane < kAtan2Edges) out[kEdgeOut + lane] = atan2_c(kAtan2EdgeY[lane], kAtan2EdgeX[lane]);
  else if (lane < kAtan2Edges + kAcosEdges) out[kEdgeOut + lane] = acos_lean(kAcosEdge[lane - kAtan2Edges]);
  // bounded sincos against libm over [-40, 40]
  double worst = 0.0;
  for (int k = 0; k < 64; ++k) {
    const double x = -40.0 + 80.0 * (lane * 64 + k) / 4095.0;
    double s1, c1, s2, c2;
    sincos_bounded(x, s1, c1);
    sincos(x, &s2, &c2);
    worst = fmax(worst, fmax(fabs(s1 - s2), fabs(c1 - c2)));
  }
  out[88 + lane] = worst;
}

}  // namespace

namespace pnec_hip {

// the two ingest kernels: x over a pair's (padded) correspondences, y over the pairs
static dim3 ingest_grid(int32_t n_max, int64_t n_pairs) {
  n_max = std::max<int32_t>(n_max, 1);
  return dim3((unsigned)std::min<int64_t>((n_max + 255) / 256, 64), (unsigned)std::min<int64_t>(n_pairs, 32768));
}

hipError_t launch_pack(int nc, int32_t n_max, double *data, const int64_t *block_offset, const int64_t *offsets,
                       const int32_t *count, int64_t first_pair, int64_t n_pairs, const double *bvs1, const double *bvs2,
                       const double *covs, const double *covs_host, hipStream_t stream) {
  const dim3 block(256), grid = ingest_grid(n_max, n_pairs);
  switch (nc) {
    case 6:
      hipLaunchKernelGGL(pack_kernel<6>, grid, block, 0, stream, data, block_offset, offsets, count, first_pair, n_pairs,
                         bvs1, bvs2, covs, covs_host);
      break;
    case 12:
      hipLaunchKernelGGL(pack_kernel<12>, grid, block, 0, stream, data, block_offset, offsets, count, first_pair, n_pairs,
                         bvs1, bvs2, covs, covs_host);
      break;
    default:
      hipLaunchKernelGGL(pack_kernel<18>, grid, block, 0, stream, data, block_offset, offsets, count, first_pair, n_pairs,
                         bvs1, bvs2, covs, covs_host);
      break;
  }
  return hipGetLastError();
}

hipError_t launch_ingest_keypoints(int nc, int32_t n_max, double *data, const int64_t *block_offset, const int64_t *offsets,
                                   const int32_t *count, int64_t first_pair, int64_t n_pairs, const double *pts1,
                                   const double *pts2, const double *cov2, const double *cov1, const double *K_inv,
                                   double kappa, hipStream_t stream) {
  const dim3 block(256), grid = ingest_grid(n_max, n_pairs);
  switch (nc) {
    case 6:
      hipLaunchKernelGGL(ingest_keypoints_kernel<6>, grid, block, 0, stream, data, block_offset, offsets, count, first_pair,
                         n_pairs, pts1, pts2, cov2, cov1, K_inv, kappa);
      break;
    case 12:
      hipLaunchKernelGGL(ingest_keypoints_kernel<12>, grid, block, 0, stream, data, block_offset, offsets, count, first_pair,
                         n_pairs, pts1, pts2, cov2, cov1, K_inv, kappa);
      break;
    default:
      hipLaunchKernelGGL(ingest_keypoints_kernel<18>, grid, block, 0, stream, data, block_offset, offsets, count, first_pair,
                         n_pairs, pts1, pts2, cov2, cov1, K_inv, kappa);
      break;
  }
  return hipGetLastError();
}

hipError_t launch_ingest_keypoints_ragged(int nc, int32_t n_max, double *data, const int64_t *block_offset,
                                          const int64_t *src_offsets, const int32_t *bound, int32_t *count,
                                          int32_t *out_dropped, int64_t n_pairs, int64_t n_rows, const double *pts1,
                                          const double *pts2, const double *cov2, const double *cov1, const double *K_inv,
                                          double kappa, hipStream_t stream) {
  const dim3 block(256), grid = ingest_grid(n_max, n_pairs);
  switch (nc) {
    case 6:
      hipLaunchKernelGGL(ingest_keypoints_ragged_kernel<6>, grid, block, 0, stream, data, block_offset, src_offsets, bound,
                         count, out_dropped, n_pairs, n_rows, pts1, pts2, cov2, cov1, K_inv, kappa);
      break;
    case 12:
      hipLaunchKernelGGL(ingest_keypoints_ragged_kernel<12>, grid, block, 0, stream, data, block_offset, src_offsets, bound,
                         count, out_dropped, n_pairs, n_rows, pts1, pts2, cov2, cov1, K_inv, kappa);
      break;
    default:
      hipLaunchKernelGGL(ingest_keypoints_ragged_kernel<18>, grid, block, 0, stream, data, block_offset, src_offsets, bound,
                         count, out_dropped, n_pairs, n_rows, pts1, pts2, cov2, cov1, K_inv, kappa);
      break;
  }
  return hipGetLastError();
}

hipError_t launch_unscented(int64_t n, const double *mu, const double *covs, const double *K_inv, double kappa,
                            int camera_model, double *out_bvs, double *out_covs, hipStream_t stream) {
  hipLaunchKernelGGL(unscented_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, n, mu, covs, K_inv, kappa,
                     camera_model, out_bvs, out_covs);
  return hipGetLastError();
}

hipError_t launch_cost_function(int64_t n_pairs, const double *data, const int64_t *block_offset, const int32_t *count,
                                const double *qs, const double *ts, double *out, hipStream_t stream) {
  hipLaunchKernelGGL(cost_function_kernel, dim3((unsigned)n_pairs), dim3(kWave), 0, stream, data, block_offset, count, qs,
                     ts, out);
  return hipGetLastError();
}

hipError_t launch_select_best(int64_t n_pairs, int n_hyp, const double *cost, int32_t *best, hipStream_t stream) {
  hipLaunchKernelGGL(select_best_kernel, dim3((unsigned)((n_pairs + 255) / 256)), dim3(256), 0, stream, n_pairs, n_hyp,
                     cost, best);
  return hipGetLastError();
}

hipError_t launch_mask_count(int64_t n_pairs, const uint8_t *mask, const int64_t *offsets, const int32_t *count,
                             int32_t *out, int64_t *single_offsets, hipStream_t stream) {
  hipLaunchKernelGGL(mask_count_kernel, dim3((unsigned)n_pairs), dim3(kWave), 0, stream, mask, offsets, count, out,
                     single_offsets);
  return hipGetLastError();
}

hipError_t launch_offsets_scan(const int32_t *count, int64_t *offsets, int64_t n, hipStream_t stream) {
  hipLaunchKernelGGL(offsets_scan_kernel, dim3(1), dim3(1024), 0, stream, count, offsets, n);
  return hipGetLastError();
}

hipError_t launch_selftest(double *out, hipStream_t stream) {
  static_assert(kAtan2Edges + kAcosEdges <= kWave, "one edge case per lane");
  hipLaunchKernelGGL(selftest_kernel, dim3(1), dim3(kWave), 0, stream, out);
  return hipGetLastError();
}

}  // namespace pnec_hip
