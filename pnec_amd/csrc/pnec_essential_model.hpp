// pnec_essential_model.hpp -- a pose from rows: what the essential-matrix kernels do between the sums of A'A and the
// chosen candidate, callable on any rows.  Device code only, everything __forceinline__, one wavefront per call.
//   em_model   steps 1-4 of pnec_hip_essential_minimal after es_sums: Jacobi, null space, Nister's ten cubics / the
//              seven-point's cubic, Sturm chain, roots, polish, order, decomposition, the forty qualities, the choice
//   em_chosen  the chosen solution's rotation, translation, E and singular values out of em_model's LDS arrays
//   ep_model   steps 2-4 of pnec_hip_eight_point after es_sums: Jacobi, null vector, decomposition, the four qualities,
//              the choice
// `Rows` is anything with load6(i, f): the pair's own planes (EsPair on global memory) or a gathered sample (EsPair on
// LDS).  The rows of the sums and the rows of the quality are counted separately: the caller has run es_sums (and the
// barrier behind it) on the first, the functions here read the first K of the second.  Two kernels call them:
// eight_point_kernel once per pair on the pair's own rows, essential_ransac_kernel once per attempt on its sample.
// essential_minimal_kernel holds the statements of em_model and of the helpers below written out under its own names:
// rewired onto this header it no longer gave its recorded bits (tests/test_essential_bits_gpu.py), and DESIGN.md 9q says
// what moves them and what paying that debt takes.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pnec_device.hpp"
#include "pnec_eight_point.hpp"
#include "pnec_essential_minimal.hpp"
#include "pnec_essential_shared.hpp"

namespace pnec_hip {
namespace model {

constexpr int kCand = 24;   // doubles per solution in LDS: Ra, Rb, ta, singular values

// the LDS a call of em_model works in (the caller declares the arrays; M holds A'A from es_sums on entry)
struct EmLds {
  double *M;    // [kEsRows * kEsDim]  rows 0..8: A'A, rows 9..17: its eigenvectors as columns
  double *T;    // [10 * 20]           the ten cubics, row-major
  double *S;    // [11 * 11]           the Sturm chain, polynomial k at S[11 k]
  double *Es;   // [kEmMaxSolutions * 9]      the solutions in their order
  double *C;    // [kEmMaxSolutions * kCand]  the candidates of every solution
};

// ---- lanes ---------------------------------------------------------------------------------------------------------------
// the value lane `src` holds, src wave-uniform (a constant where the caller's loop is unrolled)
__device__ __forceinline__ double lane_value(double x, int src) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(x), src);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(x), src);
  return make_double(hi, lo);
}
// the value of any lane, src per lane; issued by the whole wavefront
__device__ __forceinline__ double gather(double x, int src) {
  const int lo = __builtin_amdgcn_ds_bpermute(src << 2, __double2loint(x));
  const int hi = __builtin_amdgcn_ds_bpermute(src << 2, __double2hiint(x));
  return make_double(hi, lo);
}
__device__ __forceinline__ double wave_max(double x) {
#pragma unroll
  for (int m = 1; m < kWave; m <<= 1) x = fmax(x, gather(x, (int)threadIdx.x ^ m));
  return x;
}
__device__ __forceinline__ double wave_min(double x) {
#pragma unroll
  for (int m = 1; m < kWave; m <<= 1) x = fmin(x, gather(x, (int)threadIdx.x ^ m));
  return x;
}

// ---- polynomials in (x, y, z) ------------------------------------------------------------------------------------------
// linear: x y z 1.  quadratic: the products (a, b), a <= b, of the linear monomials in the order of q2.  cubic:
// Nister's order  x3 y3 x2y xy2 x2z x2 y2z y2 xyz xy | xz2 xz x yz2 yz y z3 z2 z 1.
// (no recursion for the swapped pair: inside the attempts' loop the compiler turned a tail call into a loop at run time
// and the quadratic's ten registers into scratch)
constexpr int q2_ordered(int a, int b) { return a * 4 - a * (a - 1) / 2 + (b - a); }
constexpr int q2(int a, int b) { return a <= b ? q2_ordered(a, b) : q2_ordered(b, a); }
constexpr int qa(int i) { return i < 4 ? 0 : (i < 7 ? 1 : (i < 9 ? 2 : 3)); }
constexpr int qb(int i) { return i < 4 ? i : (i < 7 ? i - 3 : (i < 9 ? i - 5 : 3)); }
constexpr int cnt(int v, int a, int b, int c) { return (a == v) + (b == v) + (c == v); }
constexpr int c3e(int ex, int ey, int ez) {
  return ex == 3 ? 0 : ey == 3 ? 1 : (ex == 2 && ey == 1) ? 2 : (ex == 1 && ey == 2) ? 3 : (ex == 2 && ez == 1) ? 4
       : ex == 2 ? 5 : (ey == 2 && ez == 1) ? 6 : ey == 2 ? 7 : (ex == 1 && ey == 1 && ez == 1) ? 8
       : (ex == 1 && ey == 1) ? 9 : (ex == 1 && ez == 2) ? 10 : (ex == 1 && ez == 1) ? 11 : ex == 1 ? 12
       : (ey == 1 && ez == 2) ? 13 : (ey == 1 && ez == 1) ? 14 : ey == 1 ? 15 : ez == 3 ? 16 : ez == 2 ? 17 : ez == 1 ? 18 : 19;
}
constexpr int c3(int q, int l) {
  return c3e(cnt(0, qa(q), qb(q), l), cnt(1, qa(q), qb(q), l), cnt(2, qa(q), qb(q), l));
}

// q += s a b
__device__ __forceinline__ void fma_ll(const double (&a)[4], const double (&b)[4], double s, double (&q)[10]) {
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) q[q2(i, j)] = __builtin_fma(s * a[i], b[j], q[q2(i, j)]);
}
// c += q l
__device__ __forceinline__ void fma_ql(const double (&q)[10], const double (&l)[4], double (&c)[20]) {
#pragma unroll
  for (int i = 0; i < 10; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) c[c3(i, j)] = __builtin_fma(q[i], l[j], c[c3(i, j)]);
}
// c += s a b, polynomials in z with ascending coefficients
template <int NA, int NB>
__device__ __forceinline__ void fma_zz(const double (&a)[NA], const double (&b)[NB], double s, double (&c)[NA + NB - 1]) {
#pragma unroll
  for (int i = 0; i < NA; ++i)
#pragma unroll
    for (int j = 0; j < NB; ++j) c[i + j] = __builtin_fma(s * a[i], b[j], c[i + j]);
}
template <int N>
__device__ __forceinline__ double horner(const double (&c)[N], double z) {
  double v = c[N - 1];
#pragma unroll
  for (int k = N - 2; k >= 0; --k) v = __builtin_fma(v, z, c[k]);
  return v;
}

// the doubles in their order as integers (-0 and +0 share a key)
__device__ __forceinline__ long long key(double x) {
  const long long b = __double_as_longlong(x);
  return b < 0 ? -(b & 0x7fffffffffffffffLL) : b;
}
__device__ __forceinline__ double unkey(long long k) {
  return __longlong_as_double(k < 0 ? ((-k) | (long long)0x8000000000000000ULL) : k);
}

// 3x3 row-major
__device__ __forceinline__ void mul33(const double (&A)[9], const double (&B)[9], double (&C)[9]) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}
// A B'
__device__ __forceinline__ void mul33_nt(const double (&A)[9], const double (&B)[9], double (&C)[9]) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) C[3 * i + j] = A[3 * i] * B[3 * j] + A[3 * i + 1] * B[3 * j + 1] + A[3 * i + 2] * B[3 * j + 2];
}
// A' B
__device__ __forceinline__ void mul33_tn(const double (&A)[9], const double (&B)[9], double (&C)[9]) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) C[3 * i + j] = A[i] * B[j] + A[3 + i] * B[3 + j] + A[6 + i] * B[6 + j];
}
// the rows of E crossed: c[k] is column k of adj(E), so d det(E + s D) / ds = sum_k c[k] . row k of D
__device__ __forceinline__ void cofactors(const double (&E)[9], double (&c)[9]) {
  const double r0[3] = {E[0], E[1], E[2]}, r1[3] = {E[3], E[4], E[5]}, r2[3] = {E[6], E[7], E[8]};
  double c0[3], c1[3], c2[3];
  es_cross(r1, r2, c0);
  es_cross(r2, r0, c1);
  es_cross(r0, r1, c2);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    c[k] = c0[k];
    c[3 + k] = c1[k];
    c[6 + k] = c2[k];
  }
}
__device__ __forceinline__ double dot9(const double (&a)[9], const double (&b)[9]) {
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < 9; ++k) s = __builtin_fma(a[k], b[k], s);
  return s;
}

// the ten constraints at E: r[0] = det E, r[1..9] = 2 E E'E - tr(E E') E; G = E E', H = E'E, cof, tr for the derivative
struct Point {
  double G[9], H[9], cof[9], tr;
};
__device__ __forceinline__ void residual(const double (&E)[9], Point &w, double (&r)[10]) {
  mul33_nt(E, E, w.G);
  mul33_tn(E, E, w.H);
  cofactors(E, w.cof);
  w.tr = w.G[0] + w.G[4] + w.G[8];
  r[0] = E[0] * w.cof[0] + E[1] * w.cof[1] + E[2] * w.cof[2];
  double GE[9];
  mul33(w.G, E, GE);
#pragma unroll
  for (int k = 0; k < 9; ++k) r[1 + k] = __builtin_fma(2.0, GE[k], -w.tr * E[k]);
}
// the derivative of the ten along D: tr(adj(E) D) and 2 (D E'E + E D'E + E E'D) - 2 tr(E D') E - tr(E E') D
__device__ __forceinline__ void derivative(const double (&E)[9], const Point &w, const double (&D)[9], double (&j)[10]) {
  j[0] = dot9(w.cof, D);
  double DH[9], P[9], PE[9], GD[9];
  mul33(D, w.H, DH);
  mul33_nt(E, D, P);
  mul33(P, E, PE);
  mul33(w.G, D, GD);
  const double ted = dot9(E, D);
#pragma unroll
  for (int k = 0; k < 9; ++k) j[1 + k] = 2.0 * (DH[k] + PE[k] + GD[k]) - 2.0 * ted * E[k] - w.tr * D[k];
}

// ---- the minimal solvers: from A'A in L.M to the choice ------------------------------------------------------------------
// Called by the whole wavefront under a wave-uniform test (it holds barriers), after es_sums and the barrier behind it.
// `trace`: what es_sums returned, finite.  `rows`, K: the quality of every candidate is the sum of es_term over
// rows.load6(0..K-1).  -> PNEC_HIP_EM_OK, NO_SOLUTION or NO_CANDIDATE, wave-uniform, as are n_sol, gap and choice
// (4 i + j, or -1).  e: lane i < n_sol holds solution i (NaN elsewhere); quality: lane 4 i + j that candidate's (NaN
// elsewhere).  L.Es and L.C hold the solutions and their candidates until the next call: em_chosen reads them.
template <class Rows>
__device__ __forceinline__ int em_model(const Rows &rows, int K, bool nister, int lane, const EmLds &L, double trace,
                                        int &n_sol, double &gap, int &choice, double &quality, double (&e)[9]) {
  double *const M = L.M, *const T = L.T, *const S = L.S, *const Es = L.Es, *const C = L.C;
  const double nan = __builtin_nan("");
  int status = PNEC_HIP_EM_OK;
  choice = -1;
  n_sol = 0;
  quality = nan;
#pragma unroll
  for (int k = 0; k < 9; ++k) e[k] = nan;

  es_jacobi(M, trace, lane);

  // ---- the null space: the eigenvalues ranked, the lowest index first among equals --------------------------------------
  const int nb = nister ? 4 : 2;
  double d[kEsDim];
#pragma unroll
  for (int k = 0; k < kEsDim; ++k) d[k] = M[k * kEsDim + k];
  int col[4] = {0, 0, 0, 0};
  double lam_lo = 0.0, lam_hi = 0.0, lam8 = d[0];
#pragma unroll
  for (int k = 0; k < kEsDim; ++k) {
    int rank = 0;
#pragma unroll
    for (int j = 0; j < kEsDim; ++j) rank += (j != k && (d[j] < d[k] || (d[j] == d[k] && j < k))) ? 1 : 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) col[b] = rank == b ? k : col[b];
    lam_lo = rank == nb - 1 ? d[k] : lam_lo;
    lam_hi = rank == nb ? d[k] : lam_hi;
    lam8 = d[k] > lam8 ? d[k] : lam8;
  }
  gap = (lam_hi - lam_lo) / lam8;
  // Bv[m]: the coefficient of (x, y, z, 1)[m] in E -- NISTER X = v3, Y = v2, Z = v1, W = v0; SEVENPT X = v1, W = v0
  double Bv[4][9];
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const int c = nister ? col[3 - m] : (m == 0 ? col[1] : col[0]);
    const bool used = nister || m == 0 || m == 3;
#pragma unroll
    for (int k = 0; k < 9; ++k) Bv[m][k] = used ? M[(kEsDim + k) * kEsDim + c] : 0.0;
  }

  // ---- p(z), ascending coefficients; the rows of B(z) stay for the null vector -------------------------------------------
  double pz[11];
#pragma unroll
  for (int k = 0; k < 11; ++k) pz[k] = 0.0;
  double bx[3][4], by[3][4], b1[3][5];
#pragma unroll
  for (int s = 0; s < 3; ++s) {
#pragma unroll
    for (int k = 0; k < 4; ++k) bx[s][k] = by[s][k] = 0.0;
#pragma unroll
    for (int k = 0; k < 5; ++k) b1[s][k] = 0.0;
  }
  if (nister) {
    // the ten cubics, one per lane
    double row20[20];
#pragma unroll
    for (int k = 0; k < 20; ++k) row20[k] = 0.0;
    {
      double El[9][4];
#pragma unroll
      for (int k = 0; k < 9; ++k)
#pragma unroll
        for (int m = 0; m < 4; ++m) El[k][m] = Bv[m][k];
      // lane r < 9: entry (ri, rj) of 2 E E'E - tr(E E') E = sum_k L(ri, k) E(k, rj), L = 2 E E' - tr(E E') I
      const int r9 = lane < 9 ? lane : 0, ri = r9 / 3, rj = r9 % 3;
      double tr[10];
#pragma unroll
      for (int k = 0; k < 10; ++k) tr[k] = 0.0;
      double Lrow[3][10];
#pragma unroll
      for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int m = 0; m < 10; ++m) Lrow[k][m] = 0.0;
#pragma unroll
      for (int x = 0; x < 3; ++x)
#pragma unroll
        for (int y = x; y < 3; ++y) {
          double g[10];
#pragma unroll
          for (int m = 0; m < 10; ++m) g[m] = 0.0;
#pragma unroll
          for (int k = 0; k < 3; ++k) fma_ll(El[3 * x + k], El[3 * y + k], 1.0, g);
          if (x == y) {
#pragma unroll
            for (int m = 0; m < 10; ++m) tr[m] += g[m];
          }
          // G(x, y) = G(y, x) is entry y of row x and entry x of row y
#pragma unroll
          for (int m = 0; m < 10; ++m) {
            Lrow[y][m] = ri == x ? 2.0 * g[m] : Lrow[y][m];
            if (x != y) Lrow[x][m] = ri == y ? 2.0 * g[m] : Lrow[x][m];
          }
        }
#pragma unroll
      for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int m = 0; m < 10; ++m) Lrow[k][m] -= ri == k ? tr[m] : 0.0;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        double ecol[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) ecol[m] = rj == 0 ? El[3 * k][m] : (rj == 1 ? El[3 * k + 1][m] : El[3 * k + 2][m]);
        fma_ql(Lrow[k], ecol, row20);
      }
      // det E = sum_k E(0, k) (E(1, k+1) E(2, k+2) - E(1, k+2) E(2, k+1))
      double detc[20];
#pragma unroll
      for (int k = 0; k < 20; ++k) detc[k] = 0.0;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int k1 = (k + 1) % 3, k2 = (k + 2) % 3;
        double minor[10];
#pragma unroll
        for (int m = 0; m < 10; ++m) minor[m] = 0.0;
        fma_ll(El[3 + k1], El[6 + k2], 1.0, minor);
        fma_ll(El[3 + k2], El[6 + k1], -1.0, minor);
        fma_ql(minor, El[k], detc);
      }
#pragma unroll
      for (int k = 0; k < 20; ++k) row20[k] = lane == 9 ? detc[k] : row20[k];
    }
    if (lane < 10) {
#pragma unroll
      for (int k = 0; k < 20; ++k) T[lane * 20 + k] = row20[k];
    }
    __syncthreads();
    // lane c < 20: column c.  Gauss-Jordan on the first ten columns, partial pivoting, the lowest row wins a tie
    double cl[10];
    {
      const int c = lane < 20 ? lane : 19;
#pragma unroll
      for (int r = 0; r < 10; ++r) cl[r] = T[r * 20 + c];
    }
#pragma unroll
    for (int p = 0; p < 10; ++p) {
      double pc[10];            // column p, wave-uniform
#pragma unroll
      for (int r = 0; r < 10; ++r) pc[r] = lane_value(cl[r], p);
      int piv = p;
      double big = fabs(pc[p]);
#pragma unroll
      for (int r = p + 1; r < 10; ++r) {
        const bool more = fabs(pc[r]) > big;
        big = more ? fabs(pc[r]) : big;
        piv = more ? r : piv;
      }
#pragma unroll
      for (int r = p + 1; r < 10; ++r) {
        const bool sw = piv == r;
        const double mine = cl[r], theirs = cl[p];
        cl[p] = sw ? mine : theirs;
        cl[r] = sw ? theirs : mine;
        const double um = pc[r], ut = pc[p];
        pc[p] = sw ? um : ut;
        pc[r] = sw ? ut : um;
      }
      cl[p] = cl[p] / pc[p];
#pragma unroll
      for (int r = 0; r < 10; ++r)
        if (r != p) cl[r] = __builtin_fma(-pc[r], cl[p], cl[r]);
    }
    // rows 4..9 = <x2z> <x2> <y2z> <y2> <xyz> <xy>, columns 10..19 = xz2 xz x yz2 yz y z3 z2 z 1
#pragma unroll
    for (int s = 0; s < 3; ++s) {
      double ra[10], rb[10];
#pragma unroll
      for (int c = 0; c < 10; ++c) {
        ra[c] = lane_value(cl[4 + 2 * s], 10 + c);
        rb[c] = lane_value(cl[5 + 2 * s], 10 + c);
      }
      bx[s][0] = ra[2];
      bx[s][1] = ra[1] - rb[2];
      bx[s][2] = ra[0] - rb[1];
      bx[s][3] = -rb[0];
      by[s][0] = ra[5];
      by[s][1] = ra[4] - rb[5];
      by[s][2] = ra[3] - rb[4];
      by[s][3] = -rb[3];
      b1[s][0] = ra[9];
      b1[s][1] = ra[8] - rb[9];
      b1[s][2] = ra[7] - rb[8];
      b1[s][3] = ra[6] - rb[7];
      b1[s][4] = -rb[6];
    }
    // det B(z) along its third column
#pragma unroll
    for (int s = 0; s < 3; ++s) {
      const int s1 = (s + 1) % 3, s2 = (s + 2) % 3;
      double minor[7];
#pragma unroll
      for (int k = 0; k < 7; ++k) minor[k] = 0.0;
      fma_zz<4, 4>(bx[s1], by[s2], 1.0, minor);
      fma_zz<4, 4>(by[s1], bx[s2], -1.0, minor);
      fma_zz<5, 7>(b1[s], minor, 1.0, pz);
    }
  } else {
    // det(W + aX) = det W + tr(adj(W) X) a + tr(adj(X) W) a2 + det X a3
    double cw[9], cx[9];
    cofactors(Bv[3], cw);
    cofactors(Bv[0], cx);
    pz[0] = Bv[3][0] * cw[0] + Bv[3][1] * cw[1] + Bv[3][2] * cw[2];
    pz[1] = dot9(cw, Bv[0]);
    pz[2] = dot9(cx, Bv[3]);
    pz[3] = Bv[0][0] * cx[0] + Bv[0][1] * cx[1] + Bv[0][2] * cx[2];
  }

  // ---- the Sturm chain, coefficient j on lane j ----------------------------------------------------------------------------
  // scale a polynomial by its largest coefficient and find its actual degree; not finite or all zero: the zero polynomial
  auto settle = [&](double &c, int &deg) {
    const bool bad = __builtin_amdgcn_ballot_w64(!finite_d(c)) != 0;
    const double m = wave_max(fabs(c));
    c = (bad || !(m > 0.0)) ? 0.0 : c / m;
    const unsigned long long nz = __builtin_amdgcn_ballot_w64(c != 0.0);
    deg = nz ? 63 - __builtin_clzll(nz) : -1;
  };
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 11; ++k) S[k] = pz[k];
  }
  __syncthreads();
  double chain[11];
  int deg[11];
  chain[0] = lane < 11 ? S[lane] : 0.0;
  __syncthreads();
  settle(chain[0], deg[0]);
  {
    const double up = gather(chain[0], lane < 63 ? lane + 1 : lane);   // (by every lane: an idle lane would send 0)
    chain[1] = lane < 10 ? (double)(lane + 1) * up : 0.0;
  }
  settle(chain[1], deg[1]);
#pragma unroll
  for (int k = 1; k < 10; ++k) {
    double r = 0.0;
    int dr = -1;
    const int dA = deg[k - 1], dB = deg[k];
    if (dB >= 1) {
      r = chain[k - 1];
      const double lead = lane_value(chain[k], dB);
#pragma unroll 1
      for (int i = dA; i >= dB; --i) {
        const double f = lane_value(r, i) / lead;
        const int sh = i - dB;
        const double b = gather(chain[k], lane >= sh ? lane - sh : lane);
        r = __builtin_fma(-f, lane >= sh ? b : 0.0, r);
        r = lane >= i ? 0.0 : r;
      }
      r = -r;
      settle(r, dr);
    }
    chain[k + 1] = r;
    deg[k + 1] = dr;
  }
  if (lane < 11) {
#pragma unroll
    for (int k = 0; k < 11; ++k) S[11 * k + lane] = chain[k];
  }
  __syncthreads();
  double sc[66];   // polynomial k: 11 - k coefficients at sc[k (23 - k) / 2]
#pragma unroll
  for (int k = 0; k < 11; ++k)
#pragma unroll
    for (int j = 0; j < 11 - k; ++j) sc[k * (23 - k) / 2 + j] = S[11 * k + j];
  auto variations = [&](double z) {
    int v = 0, last = 0;
#pragma unroll
    for (int k = 0; k < 11; ++k) {
      double val = sc[k * (23 - k) / 2 + 10 - k];
#pragma unroll
      for (int j = 9 - k; j >= 0; --j) val = __builtin_fma(val, z, sc[k * (23 - k) / 2 + j]);
      const int s = val > 0.0 ? 1 : (val < 0.0 ? -1 : 0);
      v += (s != 0 && last != 0 && s != last) ? 1 : 0;
      last = s != 0 ? s : last;
    }
    return v;
  };

  // ---- the real roots: all of them lie within Cauchy's bound; lane i bisects for the i-th ----------------------------------
  double root = 0.0;
  {
    const int d0 = deg[0];
    double bound = 0.0;
    if (d0 >= 1) {
      const double lead = lane_value(chain[0], d0);
      bound = 1.0 + wave_max(lane < d0 ? fabs(chain[0] / lead) : 0.0);
    }
    bound = to_sgpr(bound);
    int v_lo = 0;
    if (d0 >= 1 && finite_d(bound)) {
      v_lo = to_sgpr(variations(-bound));
      n_sol = v_lo - to_sgpr(variations(bound));
      n_sol = n_sol < 0 ? 0 : (n_sol > d0 ? d0 : n_sol);
    }
    long long lo = key(-bound), hi = key(bound);
    if (n_sol > 0) {
#pragma unroll 1
      for (int it = 0; it < kEmBisections; ++it) {
        const long long mid = lo + (long long)(((unsigned long long)hi - (unsigned long long)lo) >> 1);
        const bool below = v_lo - variations(unkey(mid)) >= lane + 1;   // at least lane + 1 roots in (-bound, mid]
        hi = below ? mid : hi;
        lo = below ? lo : mid;
      }
    }
    root = unkey(hi);
  }
  const bool valid = lane < n_sol;
  if (n_sol <= 0) return PNEC_HIP_EM_NO_SOLUTION;

  // ---- per solution: the point, the polish, norm and sign --------------------------------------------------------------------
  double E[9];
  if (nister) {
    double Bz[3][3];
#pragma unroll
    for (int s = 0; s < 3; ++s) {
      Bz[s][0] = horner(bx[s], root);
      Bz[s][1] = horner(by[s], root);
      Bz[s][2] = horner(b1[s], root);
    }
    // (x, y, 1) spans the null space of B(z): the cross product of two rows, the pair whose product is longest
    double c01[3], c02[3], c12[3];
    es_cross(Bz[0], Bz[1], c01);
    es_cross(Bz[0], Bz[2], c02);
    es_cross(Bz[1], Bz[2], c12);
    const double n01 = c01[0] * c01[0] + c01[1] * c01[1] + c01[2] * c01[2];
    const double n02 = c02[0] * c02[0] + c02[1] * c02[1] + c02[2] * c02[2];
    const double n12 = c12[0] * c12[0] + c12[1] * c12[1] + c12[2] * c12[2];
    const bool t01 = n01 >= n02 && n01 >= n12, t02 = !t01 && n02 >= n12;
    double cv[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) cv[k] = t01 ? c01[k] : (t02 ? c02[k] : c12[k]);
    double xyz[3] = {cv[0] / cv[2], cv[1] / cv[2], root};
#pragma unroll 1
    for (int step = 0; step < kEmPolishNister; ++step) {
#pragma unroll
      for (int k = 0; k < 9; ++k)
        E[k] = __builtin_fma(xyz[0], Bv[0][k], __builtin_fma(xyz[1], Bv[1][k], __builtin_fma(xyz[2], Bv[2][k], Bv[3][k])));
      Point w;
      double r[10], J[3][10];
      residual(E, w, r);
#pragma unroll
      for (int m = 0; m < 3; ++m) derivative(E, w, Bv[m], J[m]);
      // the normal equations, 3x3, by the adjugate
      double A[9], g[3];
#pragma unroll
      for (int x = 0; x < 3; ++x) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < 10; ++k) s = __builtin_fma(J[x][k], r[k], s);
        g[x] = s;
#pragma unroll
        for (int y = x; y < 3; ++y) {
          double t = 0.0;
#pragma unroll
          for (int k = 0; k < 10; ++k) t = __builtin_fma(J[x][k], J[y][k], t);
          A[3 * x + y] = A[3 * y + x] = t;
        }
      }
      double cof[9];
      cofactors(A, cof);   // A symmetric: its adjugate is the cofactor matrix
      const double det = A[0] * cof[0] + A[1] * cof[1] + A[2] * cof[2];
      const double inv = 1.0 / det;
#pragma unroll
      for (int x = 0; x < 3; ++x)
        xyz[x] -= (cof[x] * g[0] + cof[3 + x] * g[1] + cof[6 + x] * g[2]) * inv;
    }
#pragma unroll
    for (int k = 0; k < 9; ++k)
      E[k] = __builtin_fma(xyz[0], Bv[0][k], __builtin_fma(xyz[1], Bv[1][k], __builtin_fma(xyz[2], Bv[2][k], Bv[3][k])));
  } else {
    double al = root;
#pragma unroll 1
    for (int step = 0; step < kEmPolishSevenpt; ++step) {
#pragma unroll
      for (int k = 0; k < 9; ++k) E[k] = __builtin_fma(al, Bv[0][k], Bv[3][k]);
      double cof[9];
      cofactors(E, cof);
      al -= (E[0] * cof[0] + E[1] * cof[1] + E[2] * cof[2]) / dot9(cof, Bv[0]);
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) E[k] = __builtin_fma(al, Bv[0][k], Bv[3][k]);
  }
  {
    double nn = 0.0;
#pragma unroll
    for (int k = 0; k < 9; ++k) nn = __builtin_fma(E[k], E[k], nn);
    const double scl = es_sign(E) / sqrt(nn);
#pragma unroll
    for (int k = 0; k < 9; ++k) E[k] = valid ? E[k] * scl : nan;
  }

  // ---- the order: ascending e[0], then e[1], ...; equal vectors keep the order of their roots ---------------------------
  int rank = 0;
#pragma unroll
  for (int j = 0; j < kEmMaxSolutions; ++j) {
    if (j < n_sol) {
      bool less = false, decided = false;
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        const double o = lane_value(E[k], j);
        less = (!decided && o < E[k]) ? true : less;
        decided = decided || o != E[k];
      }
      rank += (less || (!decided && j < lane)) ? 1 : 0;
    }
  }
  if (valid) {
#pragma unroll
    for (int k = 0; k < 9; ++k) Es[rank * 9 + k] = E[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 9; ++k) e[k] = valid ? Es[lane * 9 + k] : nan;

  // ---- SVD of every E through E'E, one E per lane: the sweeps end by ballot, the rest is es_decompose's pieces ------------
  double B[9], V[9];
#pragma unroll
  for (int x = 0; x < 3; ++x)
#pragma unroll
    for (int y = x; y < 3; ++y) B[3 * x + y] = B[3 * y + x] = e[x] * e[y] + e[3 + x] * e[3 + y] + e[6 + x] * e[6 + y];
#pragma unroll
  for (int k = 0; k < 9; ++k) V[k] = (k % 4 == 0) ? 1.0 : 0.0;
  {
    const double tr3 = B[0] + B[4] + B[8];
    const double lim3 = (kEsOffTol * tr3) * (kEsOffTol * tr3);
#pragma unroll 1
    for (int sweep = 0; sweep < kEsMaxSweeps; ++sweep) {
      const double off2 = 2.0 * (B[1] * B[1] + B[2] * B[2] + B[5] * B[5]);
      const bool more = off2 > lim3;
      if (__builtin_amdgcn_ballot_w64(more) == 0) break;
      double Bn[9], Vn[9];
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        Bn[k] = B[k];
        Vn[k] = V[k];
      }
      es_rotate3<0, 1>(Bn, Vn);
      es_rotate3<0, 2>(Bn, Vn);
      es_rotate3<1, 2>(Bn, Vn);
#pragma unroll
      for (int k = 0; k < 9; ++k) {   // a lane that has converged keeps what it has
        B[k] = more ? Bn[k] : B[k];
        V[k] = more ? Vn[k] : V[k];
      }
    }
  }
  const double w0 = B[0], w1 = B[4], w2 = B[8];
  int i0, i1, i2;
  es_order3(w0, w1, w2, i0, i1, i2);
  const double lam[3] = {i0 == 0 ? w0 : (i0 == 1 ? w1 : w2), i1 == 0 ? w0 : (i1 == 1 ? w1 : w2),
                         i2 == 0 ? w0 : (i2 == 1 ? w1 : w2)};
  double sing[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) sing[k] = sqrt(lam[k] > 0.0 ? lam[k] : 0.0);
  double v0[3], v1[3], v2[3], u0[3], u1[3], u2[3];
  es_right_vectors(V, i0, i1, i2, v0, v1, v2);
  es_left_vectors(e, v0, v1, u0, u1, u2);
  if (lane < kEmMaxSolutions) {
    double Ra[9], Rb[9];   // before their sign
    es_rotations(u0, u1, u2, v0, v1, v2, Ra, Rb);
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      C[lane * kCand + k] = Ra[k];
      C[lane * kCand + 9 + k] = Rb[k];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      C[lane * kCand + 18 + k] = u2[k];
      C[lane * kCand + 21 + k] = sing[k];
    }
  }
  __syncthreads();

  // ---- the forty qualities: lane 4 i + j, candidate j of solution i ----------------------------------------------------------
  const int ci = lane < 4 * kEmMaxSolutions ? lane >> 2 : 0, cj = lane & 3;
  const bool cand = lane < 4 * n_sol;
  double R[9], t[3];
#pragma unroll
  for (int k = 0; k < 9; ++k) R[k] = C[ci * kCand + ((cj & 1) ? 9 : 0) + k];
  es_signed_rotation(R);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double u = C[ci * kCand + 18 + k];
    t[k] = (cj & 2) ? -u : u;
  }
  {
    double qs = 0.0;
#pragma unroll 1
    for (int k = 0; k < K; ++k) {
      double f[6];
      rows.load6(k, f);
      qs += es_term(f, R, t);
    }
    qs = finite_d(qs) ? qs : __builtin_inf();
    quality = cand ? qs : nan;
    const double mine = cand ? qs : __builtin_inf();
    const double best = wave_min(mine);
    if (best < kEsStartQuality) {
      const unsigned long long at = __builtin_amdgcn_ballot_w64(cand && mine == best);
      choice = at ? (int)__builtin_ctzll(at) : -1;
    }
  }
  if (choice < 0) status = PNEC_HIP_EM_NO_CANDIDATE;
  return status;
}

// the chosen candidate of em_model (choice >= 0) out of its LDS arrays; every lane that calls it gets the same values
__device__ __forceinline__ void em_chosen(const EmLds &L, int choice, double (&Rc)[9], double (&tc)[3], double (&Ec)[9],
                                          double (&sing)[3]) {
  const int ci = choice >> 2;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    Rc[k] = L.C[ci * kCand + ((choice & 1) ? 9 : 0) + k];
    Ec[k] = L.Es[ci * 9 + k];
  }
  es_signed_rotation(Rc);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double u = L.C[ci * kCand + 18 + k];
    tc[k] = (choice & 2) ? -u : u;
    sing[k] = L.C[ci * kCand + 21 + k];
  }
}

// ---- the eight-point: from A'A in M to the choice ---------------------------------------------------------------------------
// Called as em_model is.  The four qualities are sums over rows.load6(0..K-1).  `all` false, K <= 16: lane
// 16 * candidate + k takes row k, a DPP row sum per 16 lanes adds them up.  `all` true (PNEC_HIP_EP_QUALITY_ALL), K >= 1:
// the lanes stride over the K rows with four accumulators and the butterfly of the sums reduces them.  -> PNEC_HIP_EP_OK
// or NO_CANDIDATE; everything returned is wave-uniform.  E and sing are set either way, Rc and tc with a choice only.
template <class Rows>
__device__ __forceinline__ int ep_model(const Rows &rows, int K, bool all, int lane, double *M, double trace, double &gap,
                                        int &choice, double (&quality)[4], double (&E)[9], double (&sing)[3],
                                        double (&Rc)[9], double (&tc)[3]) {
  choice = -1;
  es_jacobi(M, trace, lane);

  // ---- the null vector and the gap -----------------------------------------------------------------------------------
  double d[kEsDim];
#pragma unroll
  for (int k = 0; k < kEsDim; ++k) d[k] = M[k * kEsDim + k];
  int imin = 0;
  double lam0 = d[0], lam8 = d[0];
#pragma unroll
  for (int k = 1; k < kEsDim; ++k) {
    if (d[k] < lam0) {
      lam0 = d[k];
      imin = k;
    }
    lam8 = d[k] > lam8 ? d[k] : lam8;
  }
  double lam1 = __builtin_inf();
#pragma unroll
  for (int k = 0; k < kEsDim; ++k) lam1 = (k != imin && d[k] < lam1) ? d[k] : lam1;
  gap = (lam1 - lam0) / lam8;
#pragma unroll
  for (int k = 0; k < 9; ++k) E[k] = M[(kEsDim + k) * kEsDim + imin];
  {
    double nn = 0.0;
#pragma unroll
    for (int k = 0; k < 9; ++k) nn = __builtin_fma(E[k], E[k], nn);
    const double sc = es_sign(E) / sqrt(nn);
#pragma unroll
    for (int k = 0; k < 9; ++k) E[k] *= sc;
  }

  // ---- SVD of E through E'E, the two rotations ----------------------------------------------------------------------
  double u2[3], Ra[9], Rb[9];
  es_decompose(E, sing, u2, Ra, Rb);
  es_signed_rotation(Ra);
  es_signed_rotation(Rb);

  // ---- the choice among (Ra, ta), (Rb, ta), (Ra, -ta), (Rb, -ta) -----------------------------------------------------
  const double tn[3] = {-u2[0], -u2[1], -u2[2]};
  if (all) {
    double qa[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
    for (int i0_ = 0; i0_ < K; i0_ += kWave) {
      const int i = i0_ + lane;
      const bool in = i < K;
      double f[6];
      rows.load6(in ? i : K - 1, f);
      const double e0 = es_term(f, Ra, u2), e1 = es_term(f, Rb, u2), e2 = es_term(f, Ra, tn), e3 = es_term(f, Rb, tn);
      qa[0] += in ? e0 : 0.0;
      qa[1] += in ? e1 : 0.0;
      qa[2] += in ? e2 : 0.0;
      qa[3] += in ? e3 : 0.0;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) quality[c] = to_sgpr(wave_allreduce_sum(qa[c]));
  } else {
    const int cand = lane >> 4, k = lane & 15;
    const bool in = k < K;
    double f[6], R[9], t[3];
    rows.load6(in ? k : 0, f);
#pragma unroll
    for (int j = 0; j < 9; ++j) R[j] = (cand & 1) ? Rb[j] : Ra[j];
#pragma unroll
    for (int j = 0; j < 3; ++j) t[j] = (cand & 2) ? tn[j] : u2[j];
    const double e = es_term(f, R, t);
    const double rs = row_allreduce_sum(in ? e : 0.0);
    quality[0] = read_lane<0>(rs);
    quality[1] = read_lane<16>(rs);
    quality[2] = read_lane<32>(rs);
    quality[3] = read_lane<48>(rs);
  }
  double best = kEsStartQuality;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    quality[c] = finite_d(quality[c]) ? quality[c] : __builtin_inf();
    if (quality[c] < best) {
      best = quality[c];
      choice = c;
    }
  }
  if (choice < 0) return PNEC_HIP_EP_NO_CANDIDATE;
#pragma unroll
  for (int k = 0; k < 9; ++k) Rc[k] = (choice & 1) ? Rb[k] : Ra[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) tc[k] = (choice & 2) ? tn[k] : u2[k];
  return PNEC_HIP_EP_OK;
}

}  // namespace model
}  // namespace pnec_hip
