// pnec_eight_point.hip -- the eight-point baseline: essential matrix and pose of every pair from its correspondences
// alone, in one pass.  A translation unit of its own (the solve / stream / front-stage objects do not see it).
// include/pnec_hip.h has the definitions; this file says how the wavefront is used.
//
// One block of one wavefront per pair, as the front stages' sums kernel.  Four phases, every branch wave-uniform:
//   sums    lane l takes correspondences l, l + 64, ...: nine products f1_a f2_b and 45 FMAs into 45 accumulators; each
//           accumulator then goes through wave_allreduce_sum (the DPP / permlane butterfly of pnec_device.hpp), always
//           the same tree.  This phase is all of the memory traffic: the six bearing planes, read once.
//   Jacobi  the 9x9 matrix and the 9x9 eigenvector matrix lie stacked in LDS as one 18x9 array.  A rotation (p, q) is a
//           column operation on both: lane r < 18 updates entries (r, p) and (r, q) of its own row; lanes p and q of the
//           upper half write the 2x2 block in closed form, the other seven mirror their two entries into rows p and q
//           (the matrix stays symmetric bit for bit).  The angle is computed by every lane from three broadcast reads:
//           no lane waits for another one's arithmetic, nothing is indexed dynamically in registers.
//   SVD     of the 3x3 E through the Jacobi eigen-decomposition of E'E, in registers, every lane the same.
//   choice  sample: lane = 16 * candidate + k triangulates correspondence k < min(9, N) at its candidate, a DPP row sum
//           per 16 lanes gives the four qualities.  PNEC_HIP_EP_QUALITY_ALL: the lanes stride over all correspondences
//           with four accumulators and the butterfly of the sums reduces them.
// Lane 0 stores the pair's outputs with plain vector stores.  No atomics; a pair's bits depend on its own rows and on
// `flags` only.
#include <hip/hip_runtime.h>

#include "pnec_device.hpp"
#include "pnec_eight_point.hpp"
#include "pnec_triangulate.hpp"   // tri_depths: the midpoint system

namespace pnec_hip {

namespace {

constexpr int kEpDim = 9;
constexpr int kEpRows = 2 * kEpDim;   // the matrix on top of its eigenvectors

// one Jacobi rotation of a symmetric 3x3 (full storage) in registers, V accumulates the eigenvectors as columns
template <int P, int Q>
__device__ __forceinline__ void ep_rotate3(double (&A)[9], double (&V)[9]) {
  constexpr int R = 3 - P - Q;
  const double apq = A[3 * P + Q];
  const bool nz = apq != 0.0;
  const double theta = (A[4 * Q] - A[4 * P]) / (2.0 * (nz ? apq : 1.0));
  double t = copysign(1.0, theta) / (fabs(theta) + sqrt(__builtin_fma(theta, theta, 1.0)));
  t = nz ? t : 0.0;
  const double c = 1.0 / sqrt(__builtin_fma(t, t, 1.0)), s = t * c;
  A[4 * P] = __builtin_fma(-t, apq, A[4 * P]);
  A[4 * Q] = __builtin_fma(t, apq, A[4 * Q]);
  A[3 * P + Q] = A[3 * Q + P] = 0.0;
  const double arp = A[3 * R + P], arq = A[3 * R + Q];
  A[3 * R + P] = A[3 * P + R] = c * arp - s * arq;
  A[3 * R + Q] = A[3 * Q + R] = s * arp + c * arq;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double vp = V[3 * k + P], vq = V[3 * k + Q];
    V[3 * k + P] = c * vp - s * vq;
    V[3 * k + Q] = s * vp + c * vq;
  }
}

__device__ __forceinline__ double ep_pick3(const double (&x)[9], int row, int col) {
  const double a = x[3 * row], b = x[3 * row + 1], c = x[3 * row + 2];
  return col == 0 ? a : (col == 1 ? b : c);
}

__device__ __forceinline__ void ep_cross(const double (&a)[3], const double (&b)[3], double (&c)[3]) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

__device__ __forceinline__ void ep_normalise(double (&v)[3]) {
  const double inv = 1.0 / sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
  v[0] *= inv;
  v[1] *= inv;
  v[2] *= inv;
}

// the sign that makes the entry of largest magnitude positive (the lowest index wins a tie)
template <int N>
__device__ __forceinline__ double ep_sign(const double (&v)[N]) {
  double big = v[0];
#pragma unroll
  for (int k = 1; k < N; ++k) big = fabs(v[k]) > fabs(big) ? v[k] : big;
  return big < 0.0 ? -1.0 : 1.0;
}

__device__ __forceinline__ double ep_det3(const double (&R)[9]) {
  return R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
}

// (1 - f1.r1) + (1 - f2.r2): the point of the midpoint system seen from both cameras against the bearings
__device__ __forceinline__ double ep_term(const double (&f)[6], const double (&R)[9], const double (&t)[3]) {
  TriSystem ts;
  tri_depths(f, R, t, ts);
  const double px = 0.5 * __builtin_fma(ts.depth1, f[0], __builtin_fma(ts.depth2, ts.ux, t[0]));
  const double py = 0.5 * __builtin_fma(ts.depth1, f[1], __builtin_fma(ts.depth2, ts.uy, t[1]));
  const double pz = 0.5 * __builtin_fma(ts.depth1, f[2], __builtin_fma(ts.depth2, ts.uz, t[2]));
  const double n1 = 1.0 / sqrt(px * px + py * py + pz * pz);
  const double wx = px - t[0], wy = py - t[1], wz = pz - t[2];
  const double x2 = R[0] * wx + R[3] * wy + R[6] * wz;
  const double y2 = R[1] * wx + R[4] * wy + R[7] * wz;
  const double z2 = R[2] * wx + R[5] * wy + R[8] * wz;
  const double n2 = 1.0 / sqrt(x2 * x2 + y2 * y2 + z2 * z2);
  const double e1 = 1.0 - (f[0] * px + f[1] * py + f[2] * pz) * n1;
  const double e2 = 1.0 - (f[3] * x2 + f[4] * y2 + f[5] * z2) * n2;
  return e1 + e2;
}

// xyzw of a rotation matrix (row-major), unit norm
__device__ __forceinline__ void ep_quat(const double (&R)[9], double (&q)[4]) {
  const double tr = R[0] + R[4] + R[8];
  double x, y, z, w;
  if (tr > 0.0) {
    w = 1.0 + tr;
    x = R[7] - R[5];
    y = R[2] - R[6];
    z = R[3] - R[1];
  } else if (R[0] >= R[4] && R[0] >= R[8]) {
    x = 1.0 + R[0] - R[4] - R[8];
    y = R[1] + R[3];
    z = R[2] + R[6];
    w = R[7] - R[5];
  } else if (R[4] >= R[8]) {
    x = R[1] + R[3];
    y = 1.0 - R[0] + R[4] - R[8];
    z = R[5] + R[7];
    w = R[2] - R[6];
  } else {
    x = R[2] + R[6];
    y = R[5] + R[7];
    z = 1.0 - R[0] - R[4] + R[8];
    w = R[3] - R[1];
  }
  const double inv = 1.0 / sqrt(x * x + y * y + z * z + w * w);
  q[0] = x * inv;
  q[1] = y * inv;
  q[2] = z * inv;
  q[3] = w * inv;
}

}  // namespace

__global__ __launch_bounds__(kWave) void eight_point_kernel(const EightPointArgs a) {
  __shared__ double M[kEpRows * kEpDim];   // rows 0..8: A'A (full, symmetric), rows 9..17: its eigenvectors as columns

  const int64_t pair = blockIdx.x;
  const int lane = threadIdx.x;
  const int n = to_sgpr(a.count[pair]);
  const int64_t stride = ((int64_t)n + kWave - 1) & ~(int64_t)(kWave - 1);
  const double *base = a.data + a.block_offset[pair];
  // correspondence i of the pair, i < n (callers clamp: nothing outside the pair's own rows is ever addressed)
  auto load6 = [&](int i, double (&f)[6]) {
#pragma unroll
    for (int c = 0; c < 6; ++c) f[c] = base[(int64_t)c * stride + i];
  };

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
    // ---- the 45 sums --------------------------------------------------------------------------------------------------
    double acc[45];
#pragma unroll
    for (int k = 0; k < 45; ++k) acc[k] = 0.0;
#pragma unroll 1
    for (int i0 = 0; i0 < n; i0 += kWave) {
      const int i = i0 + lane;
      const bool in = i < n;
      double f[6];
      load6(in ? i : n - 1, f);
      double r[9];
#pragma unroll
      for (int k = 0; k < 9; ++k) r[k] = in ? f[k / 3] * f[3 + k % 3] : 0.0;
      int k = 0;
#pragma unroll
      for (int x = 0; x < 9; ++x)
#pragma unroll
        for (int y = x; y < 9; ++y) {
          acc[k] = __builtin_fma(r[x], r[y], acc[k]);
          ++k;
        }
    }
    {
      int k = 0;
#pragma unroll
      for (int x = 0; x < 9; ++x)
#pragma unroll
        for (int y = x; y < 9; ++y) {
          const double s = wave_allreduce_sum(acc[k]);
          ++k;
          if (x == y) trace += s;
          if (lane == 0) {
            M[x * kEpDim + y] = s;
            M[y * kEpDim + x] = s;
          }
        }
    }
    for (int x = lane; x < kEpDim * kEpDim; x += kWave) M[kEpDim * kEpDim + x] = (x / kEpDim == x % kEpDim) ? 1.0 : 0.0;
    trace = to_sgpr(trace);
    // a NaN or an infinity in a bearing reaches three of the nine products, and through their squares the diagonal
    if (!finite_d(trace)) status = PNEC_HIP_EP_NOT_FINITE;
  }
  __syncthreads();

  if (status == PNEC_HIP_EP_OK) {
    // ---- cyclic Jacobi on the 9x9, rows of the stacked 18x9 array to lanes ---------------------------------------------
    const double off_limit = (kEpOffTol * trace) * (kEpOffTol * trace), skip_limit = kEpSkipTol * trace;
    const int row = lane < kEpRows ? lane : 0;
    const bool upper = lane < kEpDim, active = lane < kEpRows;
#pragma unroll 1
    for (int sweep = 0; sweep < kEpMaxSweeps; ++sweep) {
      double o = 0.0;
#pragma unroll
      for (int j = 0; j < kEpDim; ++j) {
        const double v = M[row * kEpDim + j];
        o = __builtin_fma((upper && j != lane) ? v : 0.0, v, o);
      }
      const double off2 = to_sgpr(wave_allreduce_sum(o));
      if (!(off2 > off_limit)) break;
#pragma unroll 1
      for (int p = 0; p < kEpDim - 1; ++p)
#pragma unroll 1
        for (int q = p + 1; q < kEpDim; ++q) {
          const double app = to_sgpr(M[p * kEpDim + p]), aqq = to_sgpr(M[q * kEpDim + q]), apq = to_sgpr(M[p * kEpDim + q]);
          const double x = M[row * kEpDim + p], y = M[row * kEpDim + q];   // (issued with the three broadcasts)
          if (!(fabs(apq) > skip_limit)) continue;
          // The two reciprocals, the root and the reciprocal root come from the hardware seeds with Newton steps
          // (pnec_device.hpp), not from the IEEE sequences: a rotation that is orthogonal to an ulp or two is all the
          // iteration needs (the updates round at that level anyway), and four IEEE divisions and roots were most of
          // the chain a rotation is.  |theta| <= 2^89 -- the pivot is above 2^-90 trace, the diagonal within the trace
          // -- so nothing below overflows.
          const double theta = 0.5 * (aqq - app) * fast_rcp(apq);
          const double t = copysign(fast_rcp(fabs(theta) + fast_sqrt(__builtin_fma(theta, theta, 1.0))), theta);
          const double c = fast_rsqrt(__builtin_fma(t, t, 1.0)), s = t * c;
          const double nx = c * x - s * y, ny = s * x + c * y;
          __syncthreads();   // every lane has read before any lane writes
          if (active) {
            const bool isp = upper && lane == p, isq = upper && lane == q;
            M[row * kEpDim + p] = isp ? __builtin_fma(-t, apq, app) : (isq ? 0.0 : nx);
            M[row * kEpDim + q] = isq ? __builtin_fma(t, apq, aqq) : (isp ? 0.0 : ny);
            if (upper && !isp && !isq) {
              M[p * kEpDim + row] = nx;
              M[q * kEpDim + row] = ny;
            }
          }
          __syncthreads();
        }
    }

    // ---- the null vector and the gap -----------------------------------------------------------------------------------
    double d[kEpDim];
#pragma unroll
    for (int k = 0; k < kEpDim; ++k) d[k] = M[k * kEpDim + k];
    int imin = 0;
    double lam0 = d[0], lam8 = d[0];
#pragma unroll
    for (int k = 1; k < kEpDim; ++k) {
      if (d[k] < lam0) {
        lam0 = d[k];
        imin = k;
      }
      lam8 = d[k] > lam8 ? d[k] : lam8;
    }
    double lam1 = __builtin_inf();
#pragma unroll
    for (int k = 0; k < kEpDim; ++k) lam1 = (k != imin && d[k] < lam1) ? d[k] : lam1;
    gap = (lam1 - lam0) / lam8;
#pragma unroll
    for (int k = 0; k < 9; ++k) E[k] = M[(kEpDim + k) * kEpDim + imin];
    {
      double nn = 0.0;
#pragma unroll
      for (int k = 0; k < 9; ++k) nn = __builtin_fma(E[k], E[k], nn);
      const double sc = ep_sign(E) / sqrt(nn);
#pragma unroll
      for (int k = 0; k < 9; ++k) E[k] *= sc;
    }

    // ---- SVD of E through E'E ------------------------------------------------------------------------------------------
    double B[9], V[9];
#pragma unroll
    for (int x = 0; x < 3; ++x)
#pragma unroll
      for (int y = x; y < 3; ++y) B[3 * x + y] = B[3 * y + x] = E[x] * E[y] + E[3 + x] * E[3 + y] + E[6 + x] * E[6 + y];
#pragma unroll
    for (int k = 0; k < 9; ++k) V[k] = (k % 4 == 0) ? 1.0 : 0.0;
    {
      const double tr3 = B[0] + B[4] + B[8];
      const double lim3 = (kEpOffTol * tr3) * (kEpOffTol * tr3);
#pragma unroll 1
      for (int sweep = 0; sweep < kEpMaxSweeps; ++sweep) {
        const double off2 = 2.0 * (B[1] * B[1] + B[2] * B[2] + B[5] * B[5]);
        if (!(to_sgpr(off2) > lim3)) break;
        ep_rotate3<0, 1>(B, V);
        ep_rotate3<0, 2>(B, V);
        ep_rotate3<1, 2>(B, V);
      }
    }
    // descending: i0 the largest (the lowest index wins a tie), i2 the smallest of the other two (the highest wins)
    const double w0 = B[0], w1 = B[4], w2 = B[8];
    const int i0 = (w0 >= w1 && w0 >= w2) ? 0 : (w1 >= w2 ? 1 : 2);
    const int ja = i0 == 0 ? 1 : 0, jb = i0 == 2 ? 1 : 2;   // the other two, ja < jb
    const double wa = ja == 0 ? w0 : w1, wb = jb == 1 ? w1 : w2;
    const int i2 = wb <= wa ? jb : ja, i1 = 3 - i0 - i2;
    const double lam[3] = {i0 == 0 ? w0 : (i0 == 1 ? w1 : w2), i1 == 0 ? w0 : (i1 == 1 ? w1 : w2),
                           i2 == 0 ? w0 : (i2 == 1 ? w1 : w2)};
#pragma unroll
    for (int k = 0; k < 3; ++k) sing[k] = sqrt(lam[k] > 0.0 ? lam[k] : 0.0);
    double v0[3], v1[3], v2[3], u0[3], u1[3], u2[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      v0[k] = ep_pick3(V, k, i0);
      v1[k] = ep_pick3(V, k, i1);
      v2[k] = ep_pick3(V, k, i2);
    }
    {
      const double sg = ep_sign(v2);
#pragma unroll
      for (int k = 0; k < 3; ++k) v2[k] *= sg;
      double cr[3];
      ep_cross(v1, v2, cr);
      const double det = v0[0] * cr[0] + v0[1] * cr[1] + v0[2] * cr[2];
      const double s1 = det < 0.0 ? -1.0 : 1.0;
#pragma unroll
      for (int k = 0; k < 3; ++k) v1[k] *= s1;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      u0[k] = E[3 * k] * v0[0] + E[3 * k + 1] * v0[1] + E[3 * k + 2] * v0[2];
      u1[k] = E[3 * k] * v1[0] + E[3 * k + 1] * v1[1] + E[3 * k + 2] * v1[2];
    }
    ep_normalise(u0);
    ep_normalise(u1);
    ep_cross(u0, u1, u2);
    ep_normalise(u2);
    // Ra = U W V' = u1 v0' - u0 v1' + u2 v2',  Rb = U W' V' = -u1 v0' + u0 v1' + u2 v2'
    double Ra[9], Rb[9];
#pragma unroll
    for (int x = 0; x < 3; ++x)
#pragma unroll
      for (int y = 0; y < 3; ++y) {
        const double m = u1[x] * v0[y] - u0[x] * v1[y], z = u2[x] * v2[y];
        Ra[3 * x + y] = z + m;
        Rb[3 * x + y] = z - m;
      }
    {
      const double sa = ep_det3(Ra) < 0.0 ? -1.0 : 1.0, sb = ep_det3(Rb) < 0.0 ? -1.0 : 1.0;
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        Ra[k] *= sa;
        Rb[k] *= sb;
      }
    }

    // ---- the choice among (Ra, ta), (Rb, ta), (Ra, -ta), (Rb, -ta) -----------------------------------------------------
    const double tn[3] = {-u2[0], -u2[1], -u2[2]};
    if (a.flags & PNEC_HIP_EP_QUALITY_ALL) {
      double qa[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
      for (int i0_ = 0; i0_ < n; i0_ += kWave) {
        const int i = i0_ + lane;
        const bool in = i < n;
        double f[6];
        load6(in ? i : n - 1, f);
        const double e0 = ep_term(f, Ra, u2), e1 = ep_term(f, Rb, u2), e2 = ep_term(f, Ra, tn), e3 = ep_term(f, Rb, tn);
        qa[0] += in ? e0 : 0.0;
        qa[1] += in ? e1 : 0.0;
        qa[2] += in ? e2 : 0.0;
        qa[3] += in ? e3 : 0.0;
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) quality[c] = to_sgpr(wave_allreduce_sum(qa[c]));
    } else {
      const int cand = lane >> 4, k = lane & 15;
      const bool in = k < (n < kEpSample ? n : kEpSample);
      double f[6], R[9], t[3];
      load6(in ? k : 0, f);
#pragma unroll
      for (int j = 0; j < 9; ++j) R[j] = (cand & 1) ? Rb[j] : Ra[j];
#pragma unroll
      for (int j = 0; j < 3; ++j) t[j] = (cand & 2) ? tn[j] : u2[j];
      const double e = ep_term(f, R, t);
      const double rs = row_allreduce_sum(in ? e : 0.0);
      quality[0] = read_lane<0>(rs);
      quality[1] = read_lane<16>(rs);
      quality[2] = read_lane<32>(rs);
      quality[3] = read_lane<48>(rs);
    }
    double best = kEpStartQuality;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      quality[c] = finite_d(quality[c]) ? quality[c] : __builtin_inf();
      if (quality[c] < best) {
        best = quality[c];
        choice = c;
      }
    }
    if (choice < 0) {
      status = PNEC_HIP_EP_NO_CANDIDATE;
#pragma unroll
      for (int k = 0; k < 9; ++k) E[k] = nan;
    } else {
#pragma unroll
      for (int k = 0; k < 9; ++k) Rc[k] = (choice & 1) ? Rb[k] : Ra[k];
#pragma unroll
      for (int k = 0; k < 3; ++k) tc[k] = (choice & 2) ? tn[k] : u2[k];
    }
  }

  if (lane == 0) {
    if (a.out_q) {
      double q[4] = {nan, nan, nan, nan};
      if (status == PNEC_HIP_EP_OK) ep_quat(Rc, q);
#pragma unroll
      for (int k = 0; k < 4; ++k) a.out_q[4 * pair + k] = q[k];
    }
    if (a.out_t) {
#pragma unroll
      for (int k = 0; k < 3; ++k) a.out_t[3 * pair + k] = tc[k];
    }
    if (a.out_E) {
#pragma unroll
      for (int k = 0; k < 9; ++k) a.out_E[9 * pair + k] = E[k];
    }
    if (a.out_singular) {
#pragma unroll
      for (int k = 0; k < 3; ++k) a.out_singular[3 * pair + k] = sing[k];
    }
    if (a.out_gap) a.out_gap[pair] = gap;
    if (a.out_quality) {
#pragma unroll
      for (int k = 0; k < 4; ++k) a.out_quality[4 * pair + k] = quality[k];
    }
    if (a.out_choice) a.out_choice[pair] = choice;
    if (a.out_status) a.out_status[pair] = status;
  }
}

hipError_t launch_eight_point(int64_t n_pairs, const EightPointArgs &a, hipStream_t stream) {
  hipLaunchKernelGGL(eight_point_kernel, dim3((unsigned)n_pairs), dim3(kWave), 0, stream, a);
  return hipGetLastError();
}

}  // namespace pnec_hip
