// pnec_trajectory.hip -- trajectory evaluation (pnec_hip_trajectory_compose, pnec_hip_trajectory_metrics): relative poses
// composed into a trajectory per sequence, and the five metrics the reference judges a run by (RPE_1, RPE_n, L1RPE_1,
// L1RPE_n, r_t) of a trajectory against ground truth.  include/pnec_hip.h has both definitions; this file follows their
// steps.  A translation unit of its own, all arithmetic FP64.
//
// compose: one wavefront per sequence.  Lane k owns the chunk of ceil(L / 64) consecutive rows k * chunk ..; it multiplies
// its steps in order (lane 0 starts from the sequence's left factor), an inclusive scan over the 64 chunk totals follows
// (six shuffle steps, left operand from the lower lane: the product does not commute), and each lane walks its chunk a
// second time from the total of the lanes below it and writes the poses.  The steps are read twice, the second time from
// cache; nothing is kept between the passes but seven doubles.
//
// advance (pnec_hip_trajectory_advance): the online form, one frame's step of the running scale and pose with the state
// held by the caller; one lane per sequence, the product and the rotation of compose.
//
// metrics: three launches on the call's stream.
//   error rotations   one lane per row, e = est * conj(gt), whatever sequence the row is in
//   distances         one wavefront per row lo + d: the wavefront finds its sequence by bisection of the cut offsets,
//                     walks the diagonal d 64 pairs at a time (two coalesced 32-byte rows per lane: e_i and e_{i+d}),
//                     each lane adding its angles in the order of i, and ends in a six-step butterfly
//   metrics           one wavefront per sequence over the rmse_d / l1_d rows, the consecutive angles and r_t
// Every sum is a per-lane sum in the order of the index followed by the butterfly, so its order is fixed by L (and d)
// alone.  No atomics, no LDS, plain vector stores.  The O(L^2) traffic is the 32-byte rows of e, at most a few hundred KB
// a sequence: it stays in L2, and the pair's cost is its FP64 instructions (one asin among them).
#include <hip/hip_runtime.h>

#include "pnec_hip.h"
#include "pnec_trajectory.hpp"

// every product and sum is rounded where it is written: the exact zero of quat_mul below needs it, and the numpy checker
// of the tests follows the same order
#pragma clang fp contract(off)

namespace pnec_hip {
namespace {

constexpr int kWaveLanes = kTrajectoryWave;
constexpr int kRowBlock = 256;   // the row kernels: four wavefronts a block

struct Quat {
  double x, y, z, w;
};
struct Vec3 {
  double x, y, z;
};
struct Pose {
  Quat q;
  Vec3 p;
};

__device__ __forceinline__ bool traj_finite(double x) { return __builtin_fabs(x) <= 0x1.fffffffffffffp1023; }

__device__ __forceinline__ Quat load_quat(const double *__restrict__ base, int64_t row) {
  const double *p = base + 4 * row;
  return Quat{p[0], p[1], p[2], p[3]};
}
__device__ __forceinline__ Vec3 load_vec3(const double *__restrict__ base, int64_t row) {
  const double *p = base + 3 * row;
  return Vec3{p[0], p[1], p[2]};
}
__device__ __forceinline__ void store_quat(double *__restrict__ base, int64_t row, const Quat &q) {
  double *p = base + 4 * row;
  p[0] = q.x;
  p[1] = q.y;
  p[2] = q.z;
  p[3] = q.w;
}

__device__ __forceinline__ double quat_norm2(const Quat &q) { return q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w; }
// q / |q|: a zero or non-finite q gives NaN
__device__ __forceinline__ Quat quat_normalise(const Quat &q) {
  const double n = __builtin_sqrt(quat_norm2(q));
  return Quat{q.x / n, q.y / n, q.z / n, q.w / n};
}
__device__ __forceinline__ Quat quat_conj(const Quat &q) { return Quat{-q.x, -q.y, -q.z, q.w}; }
// the Hamilton product: R(a b) = R(a) R(b).  The vector part is summed in pairs that cancel exactly for b = conj(a)
// (no fused multiply-add in this file), so an estimate equal to the ground truth gives e = (0, 0, 0, 1) and every angle 0.
__device__ __forceinline__ Quat quat_mul(const Quat &a, const Quat &b) {
  return Quat{(a.w * b.x + a.x * b.w) + (a.y * b.z - a.z * b.y), (a.w * b.y + a.y * b.w) + (a.z * b.x - a.x * b.z),
              (a.w * b.z + a.z * b.w) + (a.x * b.y - a.y * b.x), (a.w * b.w - a.x * b.x) - (a.y * b.y + a.z * b.z)};
}
// R(q) v for a unit q: v + w t + u x t with t = 2 (u x v), u the vector part
__device__ __forceinline__ Vec3 quat_rotate(const Quat &q, const Vec3 &v) {
  const double tx = 2.0 * (q.y * v.z - q.z * v.y), ty = 2.0 * (q.z * v.x - q.x * v.z), tz = 2.0 * (q.x * v.y - q.y * v.x);
  return Vec3{v.x + q.w * tx + (q.y * tz - q.z * ty), v.y + q.w * ty + (q.z * tx - q.x * tz),
              v.z + q.w * tz + (q.x * ty - q.y * tx)};
}

// (q_a, p_a) (q_b, p_b) = (q_a q_b, p_a + R(q_a) p_b)
__device__ __forceinline__ Pose pose_mul(const Pose &a, const Pose &b, bool positions) {
  Pose r;
  r.q = quat_mul(a.q, b.q);
  r.p = a.p;
  if (positions) {
    const Vec3 t = quat_rotate(a.q, b.p);
    r.p = Vec3{a.p.x + t.x, a.p.y + t.y, a.p.z + t.z};
  }
  return r;
}
__device__ __forceinline__ Pose pose_identity() { return Pose{Quat{0.0, 0.0, 0.0, 1.0}, Vec3{0.0, 0.0, 0.0}}; }

__device__ __forceinline__ Pose pose_shfl_up(const Pose &a, int delta) {
  Pose r;
  r.q.x = __shfl_up(a.q.x, delta, kWaveLanes);
  r.q.y = __shfl_up(a.q.y, delta, kWaveLanes);
  r.q.z = __shfl_up(a.q.z, delta, kWaveLanes);
  r.q.w = __shfl_up(a.q.w, delta, kWaveLanes);
  r.p.x = __shfl_up(a.p.x, delta, kWaveLanes);
  r.p.y = __shfl_up(a.p.y, delta, kWaveLanes);
  r.p.z = __shfl_up(a.p.z, delta, kWaveLanes);
  return r;
}

// the sum over the wavefront in a fixed order; every lane gets it
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int m = kWaveLanes / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m, kWaveLanes);
  return v;
}

__device__ __forceinline__ int64_t clamp64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }
// the rows of sequence f, cut as pnec_hip_problem_fill_keypoints_ragged cuts them
__device__ __forceinline__ void sequence_rows(const int64_t *__restrict__ offsets, int64_t f, int64_t n_rows, int64_t &lo,
                                              int64_t &hi) {
  lo = clamp64(offsets[f], 0, n_rows);
  hi = clamp64(offsets[f + 1], lo, n_rows);
}

// row r as a step: the unit rotation and the scaled translation of a present row, the identity (and false) otherwise
__device__ __forceinline__ bool load_step(const TrajectoryComposeArgs &a, int64_t r, Pose &s) {
  const Quat q = load_quat(a.rel_q, r);
  const double n2 = quat_norm2(q);
  bool present = traj_finite(q.x) && traj_finite(q.y) && traj_finite(q.z) && traj_finite(q.w) && n2 > 0.0 && traj_finite(n2);
  Vec3 t{0.0, 0.0, 0.0};
  if (a.rel_t) {
    t = load_vec3(a.rel_t, r);
    present = present && traj_finite(t.x) && traj_finite(t.y) && traj_finite(t.z);
    if (a.scale) {
      const double sc = a.scale[r];
      present = present && traj_finite(sc);
      t = Vec3{sc * t.x, sc * t.y, sc * t.z};
      present = present && traj_finite(t.x) && traj_finite(t.y) && traj_finite(t.z);
    }
  }
  const double n = __builtin_sqrt(n2);
  s = present ? Pose{Quat{q.x / n, q.y / n, q.z / n, q.w / n}, t} : pose_identity();
  return present;
}

// 4 asin(min(1, |a - s b| / 2)), s the sign of <a, b>: the angle of the rotation a conj(b), in [0, pi]
__device__ __forceinline__ double quat_angle(const Quat &a, const Quat &b) {
  const double dot = a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w;
  const double s = dot >= 0.0 ? 1.0 : -1.0;
  const double dx = a.x - s * b.x, dy = a.y - s * b.y, dz = a.z - s * b.z, dw = a.w - s * b.w;
  double c = 0.5 * __builtin_sqrt(dx * dx + dy * dy + dz * dz + dw * dw);
  c = c > 1.0 ? 1.0 : c;   // (a NaN stays a NaN)
  return 4.0 * asin(c);
}

// the direction of the step k-1 -> k in the frame of k-1: R(q_{k-1})' (p_k - p_{k-1}), normalised (a zero step: NaN)
__device__ __forceinline__ Vec3 step_direction(const double *__restrict__ q, const double *__restrict__ p, int64_t row) {
  const Quat g = quat_normalise(load_quat(q, row - 1));
  const Vec3 a = load_vec3(p, row - 1), b = load_vec3(p, row);
  const Vec3 u = quat_rotate(quat_conj(g), Vec3{b.x - a.x, b.y - a.y, b.z - a.z});
  const double n = __builtin_sqrt(u.x * u.x + u.y * u.y + u.z * u.z);
  return Vec3{u.x / n, u.y / n, u.z / n};
}
// 2 asin(min(1, |u - s v| / 2)): the angle between the lines of u and v, in [0, pi/2]
__device__ __forceinline__ double line_angle(const Vec3 &u, const Vec3 &v) {
  const double dot = u.x * v.x + u.y * v.y + u.z * v.z;
  const double s = dot >= 0.0 ? 1.0 : -1.0;
  const double dx = u.x - s * v.x, dy = u.y - s * v.y, dz = u.z - s * v.z;
  double c = 0.5 * __builtin_sqrt(dx * dx + dy * dy + dz * dz);
  c = c > 1.0 ? 1.0 : c;
  return 2.0 * asin(c);
}

}  // namespace

// ---- compose ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kWaveLanes) void trajectory_compose_kernel(const TrajectoryComposeArgs a) {
  const int64_t f = blockIdx.x;
  const int lane = threadIdx.x;
  int64_t lo, hi;
  sequence_rows(a.offsets, f, a.n_rows, lo, hi);
  const int64_t L = hi - lo;
  if (L == 0) return;   // (uniform)
  const bool positions = a.rel_t != nullptr;
  const int64_t chunk = (L + kWaveLanes - 1) / kWaveLanes;
  const int64_t first = lane * chunk < L ? lane * chunk : L, last = (lane + 1) * chunk < L ? (lane + 1) * chunk : L;

  // the sequence's left factor
  Pose start = pose_identity();
  if (a.q0) start.q = quat_normalise(load_quat(a.q0, f));
  if (a.p0) start.p = load_vec3(a.p0, f);

  // the chunk's product, in the order of the rows; lane 0's carries the left factor
  Pose total = lane == 0 ? start : pose_identity();
  for (int64_t k = first; k < last; ++k) {
    Pose s;
    (void)load_step(a, lo + k, s);
    total = pose_mul(total, s, positions);
  }
  // inclusive scan of the 64 totals: after the step of distance d a lane holds the product of up to 2 d totals ending
  // at its own
#pragma unroll
  for (int d = 1; d < kWaveLanes; d <<= 1) {
    const Pose left = pose_shfl_up(total, d);
    const Pose both = pose_mul(left, total, positions);
    if (lane >= d) total = both;
  }
  Pose pose = pose_shfl_up(total, 1);   // everything before this lane's chunk
  if (lane == 0) pose = start;
  for (int64_t k = first; k < last; ++k) {
    Pose s;
    const bool present = load_step(a, lo + k, s);
    pose = pose_mul(pose, s, positions);
    store_quat(a.out_q, lo + k, quat_normalise(pose.q));
    if (positions) {
      double *o = a.out_p + 3 * (lo + k);
      o[0] = pose.p.x;
      o[1] = pose.p.y;
      o[2] = pose.p.z;
    }
    if (a.out_valid) a.out_valid[lo + k] = present ? 1 : 0;
  }
}

hipError_t launch_trajectory_compose(const TrajectoryComposeArgs &a, hipStream_t stream) {
  if (a.n_seq < 1 || a.n_seq > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(trajectory_compose_kernel, dim3((unsigned)a.n_seq), dim3(kWaveLanes), 0, stream, a);
  return hipGetLastError();
}

// ---- advance ------------------------------------------------------------------------------------------------------
// One lane per sequence: 14 doubles and two integers in, 8 doubles and a status out, a few dozen dependent FP64
// operations with one square root and two divisions' worth of normalisation.  Nothing is shared between lanes.
__global__ __launch_bounds__(kRowBlock) void trajectory_advance_kernel(const TrajectoryAdvanceArgs a) {
  const int64_t i = (int64_t)blockIdx.x * kRowBlock + threadIdx.x;
  if (i >= a.n_seq) return;
  const Quat rq = load_quat(a.rel_q, i);
  const Vec3 rt = load_vec3(a.rel_t, i);
  const double n2 = quat_norm2(rq);
  const bool present = traj_finite(rq.x) && traj_finite(rq.y) && traj_finite(rq.z) && traj_finite(rq.w) && traj_finite(rt.x) &&
                       traj_finite(rt.y) && traj_finite(rt.z) && n2 > 0.0 && traj_finite(n2) &&
                       (!a.count || a.count[i] >= a.min_count);
  const double s = a.s[i];
  const Quat q = load_quat(a.q, i);
  const Vec3 p = load_vec3(a.p, i);
  double *np = a.next_p + 3 * i;
  if (!present) {   // the state as it is, bit for bit
    a.next_s[i] = s;
    store_quat(a.next_q, i, q);
    np[0] = p.x;
    np[1] = p.y;
    np[2] = p.z;
    if (a.out_status) a.out_status[i] = PNEC_HIP_TRAJ_ABSENT;
    return;
  }
  double next_s = 1.0;
  int32_t status = PNEC_HIP_TRAJ_STARTED;
  if (traj_finite(s) && s > 0.0) {
    next_s = s;
    status = PNEC_HIP_TRAJ_HELD;
    if (a.scale3) {
      const double r = a.scale3[3 * i + 1], sr = s * r;
      if (traj_finite(r) && r > 0.0 && (!a.n_used || a.n_used[i] >= a.min_used) && traj_finite(sr) && sr > 0.0) {
        next_s = sr;
        status = PNEC_HIP_TRAJ_MEASURED;
      }
    }
  }
  const double n = __builtin_sqrt(n2);
  const Quat step{rq.x / n, rq.y / n, rq.z / n, rq.w / n};
  const Vec3 d = quat_rotate(q, Vec3{next_s * rt.x, next_s * rt.y, next_s * rt.z});
  a.next_s[i] = next_s;
  store_quat(a.next_q, i, quat_normalise(quat_mul(q, step)));
  np[0] = p.x + d.x;
  np[1] = p.y + d.y;
  np[2] = p.z + d.z;
  if (a.out_status) a.out_status[i] = status;
}

hipError_t launch_trajectory_advance(const TrajectoryAdvanceArgs &a, hipStream_t stream) {
  if (a.n_seq < 1 || a.n_seq > 0x7fffffffLL) return hipErrorInvalidValue;
  const int64_t blocks = (a.n_seq + kRowBlock - 1) / kRowBlock;
  hipLaunchKernelGGL(trajectory_advance_kernel, dim3((unsigned)blocks), dim3(kRowBlock), 0, stream, a);
  return hipGetLastError();
}

// ---- metrics ------------------------------------------------------------------------------------------------------
// step 1: e = normalise(normalise(est) conj(normalise(gt))) for every row
__global__ __launch_bounds__(kRowBlock) void trajectory_error_kernel(const TrajectoryMetricsArgs a) {
  const int64_t r = (int64_t)blockIdx.x * kRowBlock + threadIdx.x;
  if (r >= a.n_rows) return;
  const Quat e = quat_normalise(load_quat(a.est_q, r)), g = quat_normalise(load_quat(a.gt_q, r));
  store_quat(a.out_err_q, r, quat_normalise(quat_mul(e, quat_conj(g))));
}

// steps 2 and 3: row lo + d gets rmse_d and l1_d.  One wavefront per row.
__global__ __launch_bounds__(kRowBlock) void trajectory_distance_kernel(const TrajectoryMetricsArgs a) {
  const int lane = threadIdx.x % kWaveLanes;
  const int64_t r = (int64_t)blockIdx.x * (kRowBlock / kWaveLanes) + threadIdx.x / kWaveLanes;
  if (r >= a.n_rows) return;   // (uniform over the wavefront, as is everything up to the loop)
  // the last sequence whose first row is not beyond r; the ones that share its first row and come before it are empty
  int64_t f = 0, above = a.n_seq;
  while (above - f > 1) {
    const int64_t mid = f + (above - f) / 2;
    if (clamp64(a.offsets[mid], 0, a.n_rows) <= r) f = mid;
    else above = mid;
  }
  int64_t lo, hi;
  sequence_rows(a.offsets, f, a.n_rows, lo, hi);
  if (r < lo || r >= hi) return;   // a row of no sequence
  const int64_t d = r - lo, n = hi - lo - d;
  double sum1 = 0.0, sum2 = 0.0;
  if (d > 0) {
    const double *__restrict__ e = a.out_err_q;
    for (int64_t i = lane; i < n; i += kWaveLanes) {
      const double angle = quat_angle(load_quat(e, lo + i), load_quat(e, lo + i + d));
      sum1 += angle;
      sum2 += angle * angle;
    }
    sum1 = wave_sum(sum1);
    sum2 = wave_sum(sum2);
  }
  if (lane == 0) {
    a.out_rmse_d[r] = d > 0 ? __builtin_sqrt(sum2 / (double)n) : 0.0;
    a.out_l1_d[r] = d > 0 ? sum1 / (double)n : 0.0;
  }
}

// steps 4 to 7: the consecutive angles, r_t and the five metrics.  One wavefront per sequence.
__global__ __launch_bounds__(kWaveLanes) void trajectory_metrics_kernel(const TrajectoryMetricsArgs a) {
  const int64_t f = blockIdx.x;
  const int lane = threadIdx.x;
  int64_t lo, hi;
  sequence_rows(a.offsets, f, a.n_rows, lo, hi);
  const int64_t L = hi - lo;
  const double nan = __builtin_nan("");
  double *m = a.out_metrics + 5 * f;
  const bool positions = a.est_p != nullptr;
  if (lane == 0 && L >= 1) {
    if (a.out_angle1) a.out_angle1[lo] = 0.0;
    if (a.out_rt1) a.out_rt1[lo] = 0.0;
  }
  if (L < 2) {   // (uniform)
    if (lane < 5) m[lane] = nan;
    return;
  }
  double sum_rmse = 0.0, sum_l1 = 0.0, sum_rt = 0.0;
  for (int64_t k = 1 + lane; k < L; k += kWaveLanes) {
    sum_rmse += a.out_rmse_d[lo + k];
    sum_l1 += a.out_l1_d[lo + k];
    if (a.out_angle1) a.out_angle1[lo + k] = quat_angle(load_quat(a.out_err_q, lo + k - 1), load_quat(a.out_err_q, lo + k));
    if (positions) {
      const double rt = line_angle(step_direction(a.gt_q, a.gt_p, lo + k), step_direction(a.est_q, a.est_p, lo + k));
      if (a.out_rt1) a.out_rt1[lo + k] = rt;
      sum_rt += rt;
    }
  }
  sum_rmse = wave_sum(sum_rmse);
  sum_l1 = wave_sum(sum_l1);
  sum_rt = wave_sum(sum_rt);
  if (lane == 0) {
    m[0] = a.out_rmse_d[lo + 1];
    m[1] = sum_rmse / (double)L;
    m[2] = a.out_l1_d[lo + 1];
    m[3] = sum_l1 / (double)L;
    m[4] = positions ? sum_rt / (double)(L - 1) : nan;
  }
}

hipError_t launch_trajectory_metrics(const TrajectoryMetricsArgs &a, hipStream_t stream) {
  if (a.n_seq < 1 || a.n_seq > 0x7fffffffLL || a.n_rows < 0 || a.n_rows > 0x7fffffffLL) return hipErrorInvalidValue;
  if (a.n_rows > 0) {
    const int64_t lanes = (a.n_rows + kRowBlock - 1) / kRowBlock;
    hipLaunchKernelGGL(trajectory_error_kernel, dim3((unsigned)lanes), dim3(kRowBlock), 0, stream, a);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    const int64_t per_block = kRowBlock / kWaveLanes, waves = (a.n_rows + per_block - 1) / per_block;
    hipLaunchKernelGGL(trajectory_distance_kernel, dim3((unsigned)waves), dim3(kRowBlock), 0, stream, a);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(trajectory_metrics_kernel, dim3((unsigned)a.n_seq), dim3(kWaveLanes), 0, stream, a);
  return hipGetLastError();
}

}  // namespace pnec_hip
