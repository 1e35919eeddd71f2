// pnec_sensitivity.hpp -- input gradients of a solved pose (pnec_hip_pose_sensitivity, include/pnec_hip.h): the
// per-correspondence arithmetic, the 5x5 solve, and the launch interface of pnec_sensitivity.hip.
//
// The arithmetic is written once, for the device AND for a host compiler (tools/sensitivity_host.cc builds this header
// with g++: no HIP header is pulled in there, and 1/sqrt is IEEE's).  It does not use eval_corr: the second derivatives
// need the pieces eval_corr folds together.
//
// Chart at the pose (R, t):  x = (tau_1, tau_2, omega),  t(x) = normalize(t + tau_1 B_0 + tau_2 B_1),  R(x) = Exp(omega) R,
// B_0 = b_theta, B_1 = e_phi.  To second order  t(x) = t + B tau - |tau|^2 t / 2  and  Exp(omega) = I + [omega]x +
// [omega]x^2 / 2, which is all a Hessian at x = 0 sees.  With
//   m = t x f1,  g = R'm,  n = f2.g,  p = R a,  h = t x p      (a = f1: HOST, f2: SYM)
//   D = g'S_g g + h'S_h h + reg,  y = D^-1/2,  r = n y         (NEC: r = n;  TARGET: no h;  HOST: no g'S_g g)
// the derivatives of g and h along the chart's directions a, b (k, l = the omega components, rho_k = row k of R) are
//   g_tau_a = R'(B_a x f1)            g_omega_k = g x rho_k
//   g_tau_a tau_b = -delta_ab g       g_tau_a omega_k = g_tau_a x rho_k     g_omega_k omega_l = (rho_l m_k + rho_k m_l)/2 - delta_kl g
//   h_tau_a = B_a x p                 h_omega_k = e_k (t.p) - t_k p
//   h_tau_a tau_b = -delta_ab h       h_tau_a omega_k = e_k (B_a.p) - B_a[k] p   h_omega_k omega_l = t x ((e_l p_k + e_k p_l)/2 - delta_kl p)
// (the tau tau terms are the chart's curvature: `reg` breaks the homogeneity in t, so they do not cancel; the omega omega
// terms are symmetric because Exp's second-order term symmetrises the generator products), and
//   r_a  = y (n_a - c D_a / 2),  c = n / D
//   r_ab = y n_ab - y^3 (n_a D_b + n_b D_a + n D_ab) / 2 + 3 n y^5 D_a D_b / 4
//   D_a = 2 (g_a'S_g g + h_a'S_h h),   D_ab = 2 (g_ab'S_g g + g_a'S_g g_b + h_ab'S_h h + h_a'S_h h_b).
#pragma once

#include <math.h>
#include <stdint.h>

#include "pnec_hip.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

#include "pnec_pose_pass.hpp"
#define PNEC_SENS_HD __host__ __device__ __forceinline__
#define PNEC_SENS_CONSTEXPR __host__ __device__ constexpr
#define PNEC_SENS_UNROLL _Pragma("unroll")
#else
#define PNEC_SENS_HD inline
#define PNEC_SENS_CONSTEXPR constexpr
#define PNEC_SENS_UNROLL
#endif
// Device code: the scheduler may not move instructions across this point.  The Hessian sweep is fifteen independent
// chains; interleaved for instruction-level parallelism they hold more values than a lane has registers for.
#if defined(__HIP_DEVICE_COMPILE__)
#define PNEC_SENS_FENCE() __builtin_amdgcn_sched_barrier(0)
#else
#define PNEC_SENS_FENCE() ((void)0)
#endif

namespace pnec_hip {

constexpr int kSensSums = 21;             // sum r^2 | g (5) | upper triangle of H (15): the layout of wave_reduce21
constexpr double kSensTinyDen = 1e-300;   // kTinyDen of pnec_device.hpp: a padding slot's D is `reg`, which may be 0

PNEC_SENS_CONSTEXPR int sens_tri(int a, int b) { return a * 5 - a * (a - 1) / 2 + (b - a); }   // a <= b

template <int MODE>
struct SensTraits {
  static constexpr bool kG = MODE == PNEC_HIP_MODE_TARGET || MODE == PNEC_HIP_MODE_SYM;   // D has g'S_g g (planes 6..11)
  static constexpr bool kH = MODE == PNEC_HIP_MODE_HOST || MODE == PNEC_HIP_MODE_SYM;     // D has h'S_h h
  static constexpr bool kSym = MODE == PNEC_HIP_MODE_SYM;
  static constexpr int kHOff = kSym ? 12 : 6;                                              // S_h's planes
  static constexpr int NC = MODE == PNEC_HIP_MODE_NEC ? 6 : (kSym ? 18 : 12);
};

PNEC_SENS_HD double sens_rsqrt(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return fast_rsqrt(x);
#else
  return 1.0 / sqrt(x);
#endif
}

// the pose of a slot as the arithmetic reads it (the kernel keeps it in scalar registers)
struct SensPose {
  double R[9];      // row-major
  double t[3];      // unit
  double B[2][3];   // b_theta, e_phi
};
// from what pose_setup (pnec_pose_pass.hpp) returns
PNEC_SENS_HD void sens_pose(const double (&R)[9], double st, double ct, double cp, double sp, SensPose &P) {
  PNEC_SENS_UNROLL
  for (int i = 0; i < 9; ++i) P.R[i] = R[i];
  P.t[0] = st * cp;    P.t[1] = st * sp;    P.t[2] = ct;
  P.B[0][0] = ct * cp; P.B[0][1] = ct * sp; P.B[0][2] = -st;
  P.B[1][0] = -sp;     P.B[1][1] = cp;      P.B[1][2] = 0.0;
}

PNEC_SENS_HD void sens_cross(const double (&a)[3], const double (&b)[3], double (&c)[3]) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}
PNEC_SENS_HD double sens_dot(const double (&a)[3], const double (&b)[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
// R v and R'v
PNEC_SENS_HD void sens_rot(const double (&R)[9], const double (&v)[3], double (&o)[3]) {
  PNEC_SENS_UNROLL
  for (int i = 0; i < 3; ++i) o[i] = R[3 * i] * v[0] + R[3 * i + 1] * v[1] + R[3 * i + 2] * v[2];
}
PNEC_SENS_HD void sens_rot_t(const double (&R)[9], const double (&v)[3], double (&o)[3]) {
  PNEC_SENS_UNROLL
  for (int i = 0; i < 3; ++i) o[i] = R[i] * v[0] + R[3 + i] * v[1] + R[6 + i] * v[2];
}
// S v, S = six planes (xx, xy, xz, yy, yz, zz)
PNEC_SENS_HD void sens_symv(const double *S, const double (&v)[3], double (&o)[3]) {
  o[0] = S[0] * v[0] + S[1] * v[1] + S[2] * v[2];
  o[1] = S[1] * v[0] + S[3] * v[1] + S[4] * v[2];
  o[2] = S[2] * v[0] + S[4] * v[1] + S[5] * v[2];
}

// what both passes need of one correspondence.  d[] = its planes: 0..2 f1 | 3..5 f2 | 6..11 cov | 12..17 cov_host (SYM).
// A padding slot (every plane 0) has n = 0 and a finite y, so everything made of it below is exactly 0.
struct SensCorr {
  double f1[3], f2[3], m[3], g[3], p[3], h[3], Sg[3], Sh[3];
  double n, y, r, c;   // c = n / D
};
template <int MODE>
PNEC_SENS_HD void sens_corr(const double (&d)[SensTraits<MODE>::NC], const SensPose &P, double reg, SensCorr &c) {
  using T = SensTraits<MODE>;
  PNEC_SENS_UNROLL
  for (int j = 0; j < 3; ++j) {
    c.f1[j] = d[j];
    c.f2[j] = d[3 + j];
    c.p[j] = c.h[j] = c.Sg[j] = c.Sh[j] = 0.0;
  }
  sens_cross(P.t, c.f1, c.m);
  sens_rot_t(P.R, c.m, c.g);
  c.n = sens_dot(c.f2, c.g);
  if constexpr (MODE == PNEC_HIP_MODE_NEC) {
    c.y = 1.0;
    c.r = c.n;
    c.c = c.n;
  } else {
    double D = reg;
    if constexpr (T::kH) {
      sens_rot(P.R, T::kSym ? c.f2 : c.f1, c.p);
      sens_cross(P.t, c.p, c.h);
      sens_symv(d + T::kHOff, c.h, c.Sh);
      D += sens_dot(c.h, c.Sh);
    }
    if constexpr (T::kG) {
      sens_symv(d + 6, c.g, c.Sg);
      D += sens_dot(c.g, c.Sg);
    }
    c.y = sens_rsqrt(D > kSensTinyDen ? D : kSensTinyDen);
    c.r = c.n * c.y;
    c.c = c.r * c.y;
  }
}

// Pass (a): adds one correspondence's r^2, r J and J J' (+ r hess r when FULL) to the 21 sums.
// One sweep over the columns b of the chart; column b's g_b and h_b are made where they are used, the entries (a, b),
// a <= b, are finished inside it, and the products g_a'S_g g_b + h_a'S_h h_b go through triple products with the pose's
// own vectors:  g_tau_a . v = B_a . (f1 x R v),  g_omega_k . v = rho_k . (v x g),  h_tau_a . v = B_a . (p x v),
// h_omega_k . v = (t.p) v_k - t_k (p.v)  -- so that no column but the two g_tau_a (the mixed second derivatives read
// them) outlives its sweep step: the SYM kernel has no registers for them.
// Acc holds a lane's 21 sums:  void add(int j, double x)  adds x to sum j (SensAccArray; the SYM kernel keeps the
// Hessian's fifteen in LDS).
struct SensAccArray {
  double v[kSensSums];
  PNEC_SENS_HD void add(int j, double x) { v[j] += x; }
};
template <int MODE, bool FULL, class Acc>
PNEC_SENS_HD void sens_accumulate(const double (&d)[SensTraits<MODE>::NC], const SensPose &P, double reg, Acc &acc) {
  using T = SensTraits<MODE>;
  constexpr bool kNec = MODE == PNEC_HIP_MODE_NEC;
  SensCorr c;
  sens_corr<MODE>(d, P, reg, c);

  double ga[2][3], na[5], Da[5], J[5];
  double rho[3][3];
  PNEC_SENS_UNROLL
  for (int k = 0; k < 3; ++k)
    PNEC_SENS_UNROLL
    for (int j = 0; j < 3; ++j) rho[k][j] = P.R[3 * k + j];
  const double tp = T::kH ? sens_dot(P.t, c.p) : 0.0;
  const double y3 = c.y * c.y * c.y, y5 = y3 * c.y * c.y;
  const double quad = T::kG || T::kH ? sens_dot(c.g, c.Sg) + sens_dot(c.h, c.Sh) : 0.0;   // D - reg
  acc.add(0, c.r * c.r);
  PNEC_SENS_UNROLL
  for (int b = 0; b < 5; ++b) {
    double gb[3], hb[3] = {0.0, 0.0, 0.0};
    if (b < 2) {
      double w[3];
      sens_cross(P.B[b], c.f1, w);
      sens_rot_t(P.R, w, gb);
      PNEC_SENS_UNROLL
      for (int j = 0; j < 3; ++j) ga[b][j] = gb[j];
      if constexpr (T::kH) sens_cross(P.B[b], c.p, hb);
    } else {
      sens_cross(c.g, rho[b - 2], gb);
      if constexpr (T::kH) {
        PNEC_SENS_UNROLL
        for (int j = 0; j < 3; ++j) hb[j] = (j == b - 2 ? tp : 0.0) - P.t[b - 2] * c.p[j];
      }
    }
    na[b] = sens_dot(c.f2, gb);
    double D = 0.0, X[3], Y[3], V[3], Shb[3] = {0.0, 0.0, 0.0}, pS = 0.0;
    if constexpr (T::kG) {
      D += sens_dot(gb, c.Sg);
      if constexpr (FULL) {
        double Sgb[3], RS[3];
        sens_symv(d + 6, gb, Sgb);
        sens_cross(Sgb, c.g, X);
        sens_rot(P.R, Sgb, RS);
        sens_cross(c.f1, RS, Y);
      }
    }
    if constexpr (T::kH) {
      D += sens_dot(hb, c.Sh);
      if constexpr (FULL) {
        sens_symv(d + T::kHOff, hb, Shb);
        pS = sens_dot(c.p, Shb);
        sens_cross(c.p, Shb, V);
      }
    }
    PNEC_SENS_FENCE();
    Da[b] = 2.0 * D;
    J[b] = kNec ? na[b] : c.y * (na[b] - 0.5 * c.c * Da[b]);
    acc.add(1 + b, J[b] * c.r);

    PNEC_SENS_UNROLL
    for (int a = 0; a <= b; ++a) {
      if constexpr (!FULL) {
        acc.add(6 + sens_tri(a, b), J[a] * J[b]);
      } else {
        // second derivatives of g and h along (a, b):  nab = f2 . g_ab,  Dab = g_ab'S_g g + h_ab'S_h h (+ Q_ab below)
        double nab, Dab = 0.0;
        if (b < 2) {
          nab = a == b ? -c.n : 0.0;
          Dab = a == b ? -quad : 0.0;
        } else {
          double gab[3], hab[3] = {0.0, 0.0, 0.0};
          if (a < 2) {
            const int k = b - 2;
            sens_cross(ga[a], rho[k], gab);
            if constexpr (T::kH) {
              const double bp = sens_dot(P.B[a], c.p);
              PNEC_SENS_UNROLL
              for (int j = 0; j < 3; ++j) hab[j] = (j == k ? bp : 0.0) - P.B[a][k] * c.p[j];
            }
          } else {
            const int k = a - 2, l = b - 2;
            PNEC_SENS_UNROLL
            for (int j = 0; j < 3; ++j) gab[j] = 0.5 * (rho[l][j] * c.m[k] + rho[k][j] * c.m[l]) - (k == l ? c.g[j] : 0.0);
            if constexpr (T::kH) {
              double w[3];
              PNEC_SENS_UNROLL
              for (int j = 0; j < 3; ++j)
                w[j] = 0.5 * ((j == l ? c.p[k] : 0.0) + (j == k ? c.p[l] : 0.0)) - (k == l ? c.p[j] : 0.0);
              sens_cross(P.t, w, hab);
            }
          }
          nab = sens_dot(c.f2, gab);
          if constexpr (T::kG) Dab += sens_dot(gab, c.Sg);
          if constexpr (T::kH) Dab += sens_dot(hab, c.Sh);
        }
        double rab;
        if constexpr (kNec) {
          rab = nab;
        } else {
          if (a < 2) {   // Q_ab
            if constexpr (T::kG) Dab += sens_dot(P.B[a], Y);
            if constexpr (T::kH) Dab += sens_dot(P.B[a], V);
          } else {
            if constexpr (T::kG) Dab += sens_dot(rho[a - 2], X);
            if constexpr (T::kH) Dab += tp * Shb[a - 2] - P.t[a - 2] * pS;
          }
          Dab *= 2.0;
          rab = c.y * nab - 0.5 * y3 * (na[a] * Da[b] + na[b] * Da[a] + c.n * Dab) + 0.75 * c.n * y5 * Da[a] * Da[b];
        }
        acc.add(6 + sens_tri(a, b), J[a] * J[b] + c.r * rab);
        PNEC_SENS_FENCE();
      }
    }
  }
}

// Pass (c): the gradient of  phi = lambda . grad_x (r^2 / 2) = n nd / D - n^2 Dd / (2 D^2)  with respect to the
// correspondence's inputs, negated; nd, Dd = the derivatives of n and D along lambda.  Reverse sweep over
//   md = td x f1,  gd = R'(md - om x m),  nd = f2.gd,  pd = om x p,  hd = td x p + t x pd,  Dd = 2 (gd'S_g g + hd'S_h h)
// with td = lambda_0 B_0 + lambda_1 B_1 and om = lambda_2..4.  G_g / G_h: the six unique entries of the symmetric
// gradient with respect to S_g (planes 6..11 of TARGET and SYM) and S_h (planes 6..11 of HOST, 12..17 of SYM).
template <int MODE>
PNEC_SENS_HD void sens_gradients(const double (&d)[SensTraits<MODE>::NC], const SensPose &P, double reg,
                                 const double (&lam)[5], double (&gf1)[3], double (&gf2)[3], double (&Gg)[6],
                                 double (&Gh)[6]) {
  using T = SensTraits<MODE>;
  SensCorr c;
  sens_corr<MODE>(d, P, reg, c);
  double td[3], om[3] = {lam[2], lam[3], lam[4]};
  PNEC_SENS_UNROLL
  for (int j = 0; j < 3; ++j) td[j] = lam[0] * P.B[0][j] + lam[1] * P.B[1][j];

  double md[3], w[3], gd[3], hd[3] = {0.0, 0.0, 0.0};
  sens_cross(td, c.f1, md);
  sens_cross(om, c.m, w);
  PNEC_SENS_UNROLL
  for (int j = 0; j < 3; ++j) w[j] = md[j] - w[j];
  sens_rot_t(P.R, w, gd);
  const double nd = sens_dot(c.f2, gd);
  double Dd = 0.0;
  if constexpr (T::kG) Dd += sens_dot(gd, c.Sg);
  if constexpr (T::kH) {
    double pd[3], u[3];
    sens_cross(om, c.p, pd);
    sens_cross(td, c.p, hd);
    sens_cross(P.t, pd, u);
    PNEC_SENS_UNROLL
    for (int j = 0; j < 3; ++j) hd[j] += u[j];
    Dd += sens_dot(hd, c.Sh);
  }
  Dd *= 2.0;

  // the partials of phi
  double phi_n, phi_nd, phi_D = 0.0, phi_Dd = 0.0;
  if constexpr (MODE == PNEC_HIP_MODE_NEC) {
    phi_n = nd;
    phi_nd = c.n;
  } else {
    const double iD = c.y * c.y;
    phi_nd = c.c;
    phi_n = nd * iD - c.c * Dd * iD;
    phi_D = c.c * c.c * Dd * iD - c.c * nd * iD;
    phi_Dd = -0.5 * c.c * c.c;
  }

  double gbar[3], gdbar[3], f1bar[3], f2bar[3];
  PNEC_SENS_UNROLL
  for (int j = 0; j < 3; ++j) {
    gbar[j] = phi_n * c.f2[j];
    gdbar[j] = phi_nd * c.f2[j];
    f2bar[j] = phi_n * c.g[j] + phi_nd * gd[j];
  }
  PNEC_SENS_UNROLL
  for (int j = 0; j < 6; ++j) Gg[j] = Gh[j] = 0.0;
  if constexpr (T::kG) {
    double Sgd[3];
    sens_symv(d + 6, gd, Sgd);
    PNEC_SENS_UNROLL
    for (int j = 0; j < 3; ++j) {
      gbar[j] += 2.0 * (phi_D * c.Sg[j] + phi_Dd * Sgd[j]);
      gdbar[j] += 2.0 * phi_Dd * c.Sg[j];
    }
    int e = 0;
    PNEC_SENS_UNROLL
    for (int i = 0; i < 3; ++i)
      PNEC_SENS_UNROLL
      for (int j = i; j < 3; ++j) Gg[e++] = -(phi_D * c.g[i] * c.g[j] + phi_Dd * (gd[i] * c.g[j] + c.g[i] * gd[j]));
  }
  // g = R'm,  gd = R'(md - om x m),  m = t x f1,  md = td x f1
  double u[3], mbar[3], x[3];
  sens_rot(P.R, gdbar, u);      // = mdbar
  sens_rot(P.R, gbar, mbar);
  sens_cross(om, u, x);
  PNEC_SENS_UNROLL
  for (int j = 0; j < 3; ++j) mbar[j] += x[j];
  sens_cross(mbar, P.t, f1bar);
  sens_cross(u, td, x);
  PNEC_SENS_UNROLL
  for (int j = 0; j < 3; ++j) f1bar[j] += x[j];
  if constexpr (T::kH) {
    double Shd[3], hbar[3], hdbar[3], pbar[3], pdbar[3], abar[3];
    sens_symv(d + T::kHOff, hd, Shd);
    PNEC_SENS_UNROLL
    for (int j = 0; j < 3; ++j) {
      hbar[j] = 2.0 * (phi_D * c.Sh[j] + phi_Dd * Shd[j]);
      hdbar[j] = 2.0 * phi_Dd * c.Sh[j];
    }
    int e = 0;
    PNEC_SENS_UNROLL
    for (int i = 0; i < 3; ++i)
      PNEC_SENS_UNROLL
      for (int j = i; j < 3; ++j) Gh[e++] = -(phi_D * c.h[i] * c.h[j] + phi_Dd * (hd[i] * c.h[j] + c.h[i] * hd[j]));
    // h = t x p,  hd = td x p + t x pd,  pd = om x p,  p = R a
    sens_cross(hbar, P.t, pbar);
    sens_cross(hdbar, td, x);
    sens_cross(hdbar, P.t, pdbar);
    PNEC_SENS_UNROLL
    for (int j = 0; j < 3; ++j) pbar[j] += x[j];
    sens_cross(pdbar, om, x);
    PNEC_SENS_UNROLL
    for (int j = 0; j < 3; ++j) pbar[j] += x[j];
    sens_rot_t(P.R, pbar, abar);
    PNEC_SENS_UNROLL
    for (int j = 0; j < 3; ++j) {
      if (T::kSym) f2bar[j] += abar[j];
      else f1bar[j] += abar[j];
    }
  }
  PNEC_SENS_UNROLL
  for (int j = 0; j < 3; ++j) {
    gf1[j] = -f1bar[j];
    gf2[j] = -f2bar[j];
  }
}

// lambda = H^-1 v and x_N = -H^-1 g through the Cholesky factor of the Jacobi-scaled matrix diag(H)^-1/2 H diag(H)^-1/2
// (unit diagonal: the pivots are those of a correlation matrix, whatever the units of the columns).  False when a
// diagonal entry or a pivot is not positive, or a result is not finite.  H: packed upper triangle.
PNEC_SENS_HD bool sens_solve5(const double (&H)[15], const double (&v)[5], const double (&g)[5], double (&lam)[5],
                              double (&xn)[5]) {
  double sc[5], L[15], inv[5];   // L(i,j), i >= j, at tri(j,i)
  bool ok = true;
  PNEC_SENS_UNROLL
  for (int a = 0; a < 5; ++a) {
    ok = ok && (H[sens_tri(a, a)] > 0.0);
    sc[a] = sens_rsqrt(H[sens_tri(a, a)]);
  }
  PNEC_SENS_UNROLL
  for (int j = 0; j < 5; ++j) {
    double dj = (H[sens_tri(j, j)] * sc[j]) * sc[j];
    PNEC_SENS_UNROLL
    for (int k = 0; k < j; ++k) dj -= L[sens_tri(k, j)] * L[sens_tri(k, j)];
    ok = ok && (dj > 0.0);
    const double iv = sens_rsqrt(dj);
    inv[j] = iv;
    L[sens_tri(j, j)] = dj * iv;
    PNEC_SENS_UNROLL
    for (int i = j + 1; i < 5; ++i) {
      double s = (H[sens_tri(j, i)] * sc[j]) * sc[i];
      PNEC_SENS_UNROLL
      for (int k = 0; k < j; ++k) s -= L[sens_tri(k, i)] * L[sens_tri(k, j)];
      L[sens_tri(j, i)] = s * iv;
    }
  }
  double z = 0.0;
  PNEC_SENS_UNROLL
  for (int which = 0; which < 2; ++which) {
    double b[5], w[5], o[5];
    PNEC_SENS_UNROLL
    for (int i = 0; i < 5; ++i) b[i] = (which == 0 ? v[i] : -g[i]) * sc[i];
    PNEC_SENS_UNROLL
    for (int i = 0; i < 5; ++i) {
      double s = b[i];
      PNEC_SENS_UNROLL
      for (int k = 0; k < i; ++k) s -= L[sens_tri(k, i)] * w[k];
      w[i] = s * inv[i];
    }
    PNEC_SENS_UNROLL
    for (int i = 4; i >= 0; --i) {
      double s = w[i];
      PNEC_SENS_UNROLL
      for (int k = i + 1; k < 5; ++k) s -= L[sens_tri(i, k)] * o[k];
      o[i] = s * inv[i];
    }
    PNEC_SENS_UNROLL
    for (int i = 0; i < 5; ++i) {
      const double x = o[i] * sc[i];
      z += x * 0.0;   // 0 for finite, NaN otherwise
      if (which == 0) lam[i] = x;
      else xn[i] = x;
    }
  }
  return ok && (z == 0.0);
}

// Phase (b), one slot: from the 21 sums and the caller's cotangent gp = (dL/d omega, dL/d t) to H, g, lambda, x_N and the
// status.  A failed slot's lambda and x_N are NaN, or 0 with PNEC_HIP_SENS_ZERO_ON_FAILURE; H and g are what was summed.
PNEC_SENS_HD int sens_finish(const double (&sum)[kSensSums], const SensPose &P, const double *gp, int n, int flags,
                             double (&H)[15], double (&gr)[5], double (&lam)[5], double (&xn)[5]) {
  double z = 0.0;
  PNEC_SENS_UNROLL
  for (int j = 0; j < kSensSums; ++j) z += sum[j] * 0.0;   // 0 for finite, NaN otherwise
  PNEC_SENS_UNROLL
  for (int i = 0; i < 5; ++i) gr[i] = sum[1 + i];
  PNEC_SENS_UNROLL
  for (int i = 0; i < 15; ++i) H[i] = sum[6 + i];
  double v[5];
  v[0] = P.B[0][0] * gp[3] + P.B[0][1] * gp[4] + P.B[0][2] * gp[5];
  v[1] = P.B[1][0] * gp[3] + P.B[1][1] * gp[4] + P.B[1][2] * gp[5];
  v[2] = gp[0];
  v[3] = gp[1];
  v[4] = gp[2];
  const bool ok = sens_solve5(H, v, gr, lam, xn);
  const int status = !(z == 0.0) ? PNEC_HIP_SENS_NONFINITE : ((n < 5 || !ok) ? PNEC_HIP_SENS_SINGULAR : PNEC_HIP_SENS_OK);
  const double fill = (flags & PNEC_HIP_SENS_ZERO_ON_FAILURE) ? 0.0 : NAN;
  PNEC_SENS_UNROLL
  for (int i = 0; i < 5; ++i) {
    lam[i] = status == PNEC_HIP_SENS_OK ? lam[i] : fill;
    xn[i] = status == PNEC_HIP_SENS_OK ? xn[i] : fill;
  }
  return status;
}

#if defined(__HIPCC__)
struct SensitivityArgs {
  const double *data;
  const int64_t *block_offset;
  const int32_t *count;
  const int64_t *offsets;
  const double *q;           // [S,4] xyzw
  const double *t;           // [S,3]
  const double *grad_pose;   // [S,6] (dL/d omega, dL/d t)
  int32_t n_hyp;
  int32_t flags;             // PNEC_HIP_SENS_*
  double reg;
  double *out_grad_bvs1;       // [M,3] or NULL
  double *out_grad_bvs2;       // [M,3] or NULL
  double *out_grad_covs;       // [M,9] or NULL
  double *out_grad_covs_host;  // [M,9] or NULL (SYM)
  double *out_lambda;          // [S,5]  or NULL
  double *out_hessian;         // [S,15] or NULL
  double *out_grad;            // [S,5]  or NULL
  double *out_newton;          // [S,5]  or NULL
  int32_t *out_status;         // [S]    or NULL
};

// one block of `waves` wavefronts per slot
hipError_t launch_pose_sensitivity(int mode, int64_t n_slots, int waves, const SensitivityArgs &a, hipStream_t stream);
#endif

}  // namespace pnec_hip
