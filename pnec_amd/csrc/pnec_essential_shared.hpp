// pnec_essential_shared.hpp -- the phases that the essential-matrix kernels (pnec_eight_point.hip,
// pnec_essential_minimal.hip) have in common, one copy of each.  Device code only, everything __forceinline__: a kernel
// that calls a phase gets the statements it would have written out.  One wavefront per pair in both kernels:
//   es_sums       the 45 sums of A'A by the fixed butterfly, A'A and the identity into the stacked 18x9 LDS array
//   es_jacobi     the cyclic Jacobi iteration on that array, rows on lanes
//   es_decompose  singular values, u2 and the two rotations of a 3x3 E through the eigen-decomposition of E'E, one E
//                 per wavefront; what follows its sweep loop is es_order3, es_right_vectors, es_left_vectors and
//                 es_rotations, which the minimal solvers' kernel calls after a sweep loop of its own (one E per lane)
//   es_term       the midpoint quality term of one correspondence at one candidate pose
//   es_store_pose the lane-0 stores of the outputs both calls have
// The status codes, the barrier between es_sums and es_jacobi and everything a call has alone stay with the kernels.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pnec_device.hpp"
#include "pnec_triangulate.hpp"   // tri_depths: the midpoint system

namespace pnec_hip {

constexpr int kEsDim = 9;
constexpr int kEsRows = 2 * kEsDim;   // the matrix on top of its eigenvectors

// the cyclic Jacobi iteration on A'A: it stops when the Frobenius norm of the off-diagonal part is at or below
// kEsOffTol * trace, after kEsMaxSweeps sweeps at the latest; a rotation whose pivot is at or below kEsSkipTol * trace
// is left out (it would change nothing that the stop looks at)
constexpr int kEsMaxSweeps = 16;
constexpr double kEsOffTol = 0x1p-58;
constexpr double kEsSkipTol = 0x1p-90;
constexpr double kEsStartQuality = 1e6;   // the reference's bestQuality (src/common/common.cc:273)

// the six bearing planes of one pair
struct EsPair {
  const double *base;
  int64_t stride;
  // correspondence i of the pair, i < n (callers clamp: nothing outside the pair's own rows is ever addressed)
  __device__ __forceinline__ void load6(int i, double (&f)[6]) const {
#pragma unroll
    for (int c = 0; c < 6; ++c) f[c] = base[(int64_t)c * stride + i];
  }
};

// ---- 3-vectors and 3x3 matrices (row-major) in registers ------------------------------------------------------------
// one Jacobi rotation of a symmetric 3x3 (full storage) in registers, V accumulates the eigenvectors as columns
template <int P, int Q>
__device__ __forceinline__ void es_rotate3(double (&A)[9], double (&V)[9]) {
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

__device__ __forceinline__ double es_pick3(const double (&x)[9], int row, int col) {
  const double a = x[3 * row], b = x[3 * row + 1], c = x[3 * row + 2];
  return col == 0 ? a : (col == 1 ? b : c);
}

__device__ __forceinline__ void es_cross(const double (&a)[3], const double (&b)[3], double (&c)[3]) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

__device__ __forceinline__ void es_normalise(double (&v)[3]) {
  const double inv = 1.0 / sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
  v[0] *= inv;
  v[1] *= inv;
  v[2] *= inv;
}

// the sign that makes the entry of largest magnitude positive (the lowest index wins a tie)
template <int N>
__device__ __forceinline__ double es_sign(const double (&v)[N]) {
  double big = v[0];
#pragma unroll
  for (int k = 1; k < N; ++k) big = fabs(v[k]) > fabs(big) ? v[k] : big;
  return big < 0.0 ? -1.0 : 1.0;
}

__device__ __forceinline__ double es_det3(const double (&R)[9]) {
  return R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
}

// R or -R, whichever has the positive determinant: what turns es_decompose's Ra / Rb into rotations
__device__ __forceinline__ void es_signed_rotation(double (&R)[9]) {
  const double sd = es_det3(R) < 0.0 ? -1.0 : 1.0;
#pragma unroll
  for (int k = 0; k < 9; ++k) R[k] *= sd;
}

// (1 - f1.r1) + (1 - f2.r2): the point of the midpoint system seen from both cameras against the bearings
__device__ __forceinline__ double es_term(const double (&f)[6], const double (&R)[9], const double (&t)[3]) {
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
__device__ __forceinline__ void es_quat(const double (&R)[9], double (&q)[4]) {
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

// ---- the 45 sums ----------------------------------------------------------------------------------------------------
// Lane l takes correspondences l, l + 64, ... of the pair (n >= 1): nine products f1_a f2_b and 45 FMAs into 45
// accumulators, each then through wave_allreduce_sum, always the same tree.  Leaves A'A (full, symmetric) in rows 0..8 of
// M and the identity in rows 9..17; the caller's barrier comes after.  -> the trace, wave-uniform: a NaN or an infinity
// in a bearing reaches three of the nine products, and through their squares the diagonal.
__device__ __forceinline__ double es_sums(const EsPair &pr, int n, int lane, double *M) {
  double trace = 0.0;
  double acc[45];
#pragma unroll
  for (int k = 0; k < 45; ++k) acc[k] = 0.0;
#pragma unroll 1
  for (int i0 = 0; i0 < n; i0 += kWave) {
    const int i = i0 + lane;
    const bool in = i < n;
    double f[6];
    pr.load6(in ? i : n - 1, f);
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
          M[x * kEsDim + y] = s;
          M[y * kEsDim + x] = s;
        }
      }
  }
  for (int x = lane; x < kEsDim * kEsDim; x += kWave) M[kEsDim * kEsDim + x] = (x / kEsDim == x % kEsDim) ? 1.0 : 0.0;
  return to_sgpr(trace);
}

// ---- cyclic Jacobi on the 9x9, rows of the stacked 18x9 array to lanes ------------------------------------------------
// A rotation (p, q) is a column operation on the matrix and on its eigenvectors: lane r < 18 updates entries (r, p) and
// (r, q) of its own row; lanes p and q of the upper half write the 2x2 block in closed form, the other seven mirror their
// two entries into rows p and q (the matrix stays symmetric bit for bit).  The angle is computed by every lane from
// three broadcast reads.  Holds barriers: the whole wavefront calls it or none of it does (both kernels call it under a
// wave-uniform test of their status), and every branch around a barrier below is on wave-uniform values.
__device__ __forceinline__ void es_jacobi(double *M, double trace, int lane) {
  const double off_limit = (kEsOffTol * trace) * (kEsOffTol * trace), skip_limit = kEsSkipTol * trace;
  const int row = lane < kEsRows ? lane : 0;
  const bool upper = lane < kEsDim, active = lane < kEsRows;
#pragma unroll 1
  for (int sweep = 0; sweep < kEsMaxSweeps; ++sweep) {
    double o = 0.0;
#pragma unroll
    for (int j = 0; j < kEsDim; ++j) {
      const double v = M[row * kEsDim + j];
      o = __builtin_fma((upper && j != lane) ? v : 0.0, v, o);
    }
    const double off2 = to_sgpr(wave_allreduce_sum(o));
    if (!(off2 > off_limit)) break;
#pragma unroll 1
    for (int p = 0; p < kEsDim - 1; ++p)
#pragma unroll 1
      for (int q = p + 1; q < kEsDim; ++q) {
        const double app = to_sgpr(M[p * kEsDim + p]), aqq = to_sgpr(M[q * kEsDim + q]), apq = to_sgpr(M[p * kEsDim + q]);
        const double x = M[row * kEsDim + p], y = M[row * kEsDim + q];   // (issued with the three broadcasts)
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
          M[row * kEsDim + p] = isp ? __builtin_fma(-t, apq, app) : (isq ? 0.0 : nx);
          M[row * kEsDim + q] = isq ? __builtin_fma(t, apq, aqq) : (isp ? 0.0 : ny);
          if (upper && !isp && !isq) {
            M[p * kEsDim + row] = nx;
            M[q * kEsDim + row] = ny;
          }
        }
        __syncthreads();
      }
  }
}

// the eigenvalues of E'E in descending order: i0 the largest (the lowest index wins a tie), i2 the smallest of the
// other two (the highest wins)
__device__ __forceinline__ void es_order3(double w0, double w1, double w2, int &i0, int &i1, int &i2) {
  i0 = (w0 >= w1 && w0 >= w2) ? 0 : (w1 >= w2 ? 1 : 2);
  const int ja = i0 == 0 ? 1 : 0, jb = i0 == 2 ? 1 : 2;   // the other two, ja < jb
  const double wa = ja == 0 ? w0 : w1, wb = jb == 1 ? w1 : w2;
  i2 = wb <= wa ? jb : ja;
  i1 = 3 - i0 - i2;
}

// the right singular vectors: columns i0, i1, i2 of V; v2 with its largest entry positive, v1 so that (v0, v1, v2) is
// right-handed
__device__ __forceinline__ void es_right_vectors(const double (&V)[9], int i0, int i1, int i2, double (&v0)[3],
                                                 double (&v1)[3], double (&v2)[3]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    v0[k] = es_pick3(V, k, i0);
    v1[k] = es_pick3(V, k, i1);
    v2[k] = es_pick3(V, k, i2);
  }
  const double sg = es_sign(v2);
#pragma unroll
  for (int k = 0; k < 3; ++k) v2[k] *= sg;
  double cr[3];
  es_cross(v1, v2, cr);
  const double det = v0[0] * cr[0] + v0[1] * cr[1] + v0[2] * cr[2];
  const double s1 = det < 0.0 ? -1.0 : 1.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) v1[k] *= s1;
}

// the left singular vectors: u0 = E v0, u1 = E v1 normalised, u2 = u0 x u1 normalised
__device__ __forceinline__ void es_left_vectors(const double (&E)[9], const double (&v0)[3], const double (&v1)[3],
                                                double (&u0)[3], double (&u1)[3], double (&u2)[3]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    u0[k] = E[3 * k] * v0[0] + E[3 * k + 1] * v0[1] + E[3 * k + 2] * v0[2];
    u1[k] = E[3 * k] * v1[0] + E[3 * k + 1] * v1[1] + E[3 * k + 2] * v1[2];
  }
  es_normalise(u0);
  es_normalise(u1);
  es_cross(u0, u1, u2);
  es_normalise(u2);
}

// Ra = U W V' = u1 v0' - u0 v1' + u2 v2',  Rb = U W' V' = -u1 v0' + u0 v1' + u2 v2', before the sign that makes them
// rotations (es_signed_rotation)
__device__ __forceinline__ void es_rotations(const double (&u0)[3], const double (&u1)[3], const double (&u2)[3],
                                             const double (&v0)[3], const double (&v1)[3], const double (&v2)[3],
                                             double (&Ra)[9], double (&Rb)[9]) {
#pragma unroll
  for (int x = 0; x < 3; ++x)
#pragma unroll
    for (int y = 0; y < 3; ++y) {
      const double m = u1[x] * v0[y] - u0[x] * v1[y], z = u2[x] * v2[y];
      Ra[3 * x + y] = z + m;
      Rb[3 * x + y] = z - m;
    }
}

// ---- the 3x3 decomposition: SVD of E through E'E, every lane the same E ------------------------------------------------
// -> the singular values descending, u2 (the translation up to its sign) and Ra = U W V', Rb = U W' V' before the sign
// that makes them rotations (es_signed_rotation).  The sweeps end on a scalar test.  (The minimal solvers' kernel has one
// E per lane, ends its sweeps by ballot and freezes converged lanes: that loop is in pnec_essential_minimal.hip, followed
// by the same four functions as here.)
__device__ __forceinline__ void es_decompose(const double (&E)[9], double (&sing)[3], double (&u2)[3], double (&Ra)[9],
                                             double (&Rb)[9]) {
  double B[9], V[9];
#pragma unroll
  for (int x = 0; x < 3; ++x)
#pragma unroll
    for (int y = x; y < 3; ++y) B[3 * x + y] = B[3 * y + x] = E[x] * E[y] + E[3 + x] * E[3 + y] + E[6 + x] * E[6 + y];
#pragma unroll
  for (int k = 0; k < 9; ++k) V[k] = (k % 4 == 0) ? 1.0 : 0.0;
  {
    const double tr3 = B[0] + B[4] + B[8];
    const double lim3 = (kEsOffTol * tr3) * (kEsOffTol * tr3);
#pragma unroll 1
    for (int sweep = 0; sweep < kEsMaxSweeps; ++sweep) {
      const double off2 = 2.0 * (B[1] * B[1] + B[2] * B[2] + B[5] * B[5]);
      if (!(to_sgpr(off2) > lim3)) break;
      es_rotate3<0, 1>(B, V);
      es_rotate3<0, 2>(B, V);
      es_rotate3<1, 2>(B, V);
    }
  }
  const double w0 = B[0], w1 = B[4], w2 = B[8];
  int i0, i1, i2;
  es_order3(w0, w1, w2, i0, i1, i2);
  const double lam[3] = {i0 == 0 ? w0 : (i0 == 1 ? w1 : w2), i1 == 0 ? w0 : (i1 == 1 ? w1 : w2),
                         i2 == 0 ? w0 : (i2 == 1 ? w1 : w2)};
#pragma unroll
  for (int k = 0; k < 3; ++k) sing[k] = sqrt(lam[k] > 0.0 ? lam[k] : 0.0);
  double v0[3], v1[3], v2[3], u0[3], u1[3];
  es_right_vectors(V, i0, i1, i2, v0, v1, v2);
  es_left_vectors(E, v0, v1, u0, u1, u2);
  es_rotations(u0, u1, u2, v0, v1, v2, Ra, Rb);
}

// ---- the outputs both calls have, by the lane that calls it (lane 0), plain vector stores -------------------------------
// Args: EightPointArgs or EssentialMinimalArgs; every output may be NULL.  `ok`: the pair has a pose, Rc is a rotation.
template <class Args>
__device__ __forceinline__ void es_store_pose(const Args &a, int64_t pair, bool ok, const double (&Rc)[9],
                                              const double (&tc)[3], const double (&E)[9], const double (&sing)[3],
                                              double gap, int choice, int status) {
  if (a.out_q) {
    const double nan = __builtin_nan("");
    double q[4] = {nan, nan, nan, nan};
    if (ok) es_quat(Rc, q);
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
  if (a.out_choice) a.out_choice[pair] = choice;
  if (a.out_status) a.out_status[pair] = status;
}

}  // namespace pnec_hip
