// sensitivity_host.cc -- the arithmetic of pnec_hip_pose_sensitivity on the host: pnec_amd/csrc/pnec_sensitivity.hpp
// built with a host compiler (no HIP), one slot at a time, with the sums added in the order one block of the kernel adds
// them: correspondence i in lane i % 64 of wavefront (i / 64) % W, a lane's share summed in walk order over the
// zero-padded planes, the lanes through the tree of wave_reduce21, the wavefronts in wave order.  1 / sqrt is IEEE's
// here, so the results agree with the device to rounding, not to the bit.
//
//   g++ -O2 -std=c++17 -Iinclude -Ipnec_amd/csrc tools/sensitivity_host.cc -o sensitivity_host
//   sensitivity_host in.bin out.bin
//
// in.bin (little endian):  int32 K, then K problems, each
//   int32 mode, n, flags, 0 | double reg, q[4] (xyzw), t[3], grad_pose[6] | double planes[NC][n]  (NC = 6, 12 or 18:
//   f1 xyz, f2 xyz, cov xx xy xz yy yz zz, cov_host ...; NOT padded)
// out.bin:  per problem  int32 status, 0 | double H[15], g[5], lambda[5], x_N[5] | double grad_bvs1[n][3],
//   grad_bvs2[n][3], grad_covs[n][9], grad_covs_host[n][9]  (an array the family does not have is all 0)
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "pnec_sensitivity.hpp"

using namespace pnec_hip;

namespace {

constexpr int kLanes = 64, kPerWave = 512, kMaxWaves = 8;   // kWave, kCovCorrPerWave, kCovMaxWaves of pnec_pose_pass.hpp

int waves_of(int n) {
  const int w = (n + kPerWave - 1) / kPerWave;
  return w < 1 ? 1 : (w > kMaxWaves ? kMaxWaves : w);
}

// pose_setup of pnec_pose_pass.hpp
void pose_of(const double *qp, const double *tp, SensPose &P) {
  double q[4] = {qp[0], qp[1], qp[2], qp[3]};
  const double qn = 1.0 / std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  for (double &v : q) v *= qn;
  const double tx = tp[0], ty = tp[1], tz = tp[2];
  const double nrm = std::sqrt(tx * tx + ty * ty + tz * tz), rho = std::sqrt(tx * tx + ty * ty);
  double st = rho / nrm, ct = tz / nrm, cp = tx / rho, sp = ty / rho;
  if (nrm == 0.0) {
    st = 0.0;
    ct = 1.0;
  }
  if (rho == 0.0 || (st < 1e-10 && ct > 0.0)) {
    cp = 1.0;
    sp = 0.0;
  }
  const double x2 = 2.0 * q[0], y2 = 2.0 * q[1], z2 = 2.0 * q[2];
  const double twx = x2 * q[3], twy = y2 * q[3], twz = z2 * q[3];
  const double txx = x2 * q[0], txy = y2 * q[0], txz = z2 * q[0];
  const double tyy = y2 * q[1], tyz = z2 * q[1], tzz = z2 * q[2];
  const double R[9] = {1.0 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1.0 - (txx + tzz),
                       tyz - twx,         txz - twy, tyz + twx, 1.0 - (txx + tyy)};
  sens_pose(R, st, ct, cp, sp, P);
}

// the 64 lanes' values of one sum through the tree of wave_reduce21: lanes l and l + 32, rows r and r ^ 1, then inside a
// row of 16 lanes  l ^ 1,  l ^ 2,  the half row mirrored,  the row mirrored
double lane_tree(const double (&x)[kLanes]) {
  double a[32], b[16], c[16];
  for (int l = 0; l < 32; ++l) a[l] = x[l] + x[l + 32];
  for (int l = 0; l < 16; ++l) b[l] = a[l] + a[l + 16];
  for (int l = 0; l < 16; ++l) c[l] = b[l] + b[l ^ 1];
  for (int l = 0; l < 16; ++l) b[l] = c[l] + c[l ^ 2];
  for (int l = 0; l < 16; ++l) c[l] = b[l] + b[(l & 8) | (7 - (l & 7))];
  return c[0] + c[15];
}

struct Problem {
  int32_t mode, n, flags;
  double reg, q[4], t[3], gp[6];
  std::vector<double> planes;
};

template <int MODE>
void run(const Problem &pr, std::FILE *out) {
  constexpr int NC = SensTraits<MODE>::NC;
  const int n = pr.n, stride = (n + kLanes - 1) / kLanes * kLanes, W = waves_of(n);
  SensPose P;
  pose_of(pr.q, pr.t, P);
  auto load = [&](int i, double (&d)[NC]) {
    for (int c = 0; c < NC; ++c) d[c] = i < n ? pr.planes[(size_t)c * n + i] : 0.0;
  };
  const bool full = !(pr.flags & PNEC_HIP_SENS_GAUSS_NEWTON);
  double sum[kSensSums];
  for (int w = 0; w < W; ++w) {
    std::vector<SensAccArray> lanes(kLanes);
    for (SensAccArray &a : lanes)
      for (double &v : a.v) v = 0.0;
    for (int l = 0; l < kLanes; ++l)
      for (int i = w * kLanes + l; i < stride; i += W * kLanes) {
        double d[NC];
        load(i, d);
        if (full) sens_accumulate<MODE, true>(d, P, pr.reg, lanes[l]);
        else sens_accumulate<MODE, false>(d, P, pr.reg, lanes[l]);
      }
    for (int j = 0; j < kSensSums; ++j) {
      double x[kLanes];
      for (int l = 0; l < kLanes; ++l) x[l] = lanes[l].v[j];
      const double s = lane_tree(x);
      sum[j] = w == 0 ? s : sum[j] + s;
    }
  }
  double H[15], g[5], lam[5], xn[5];
  const int32_t head[2] = {sens_finish(sum, P, pr.gp, n, pr.flags, H, g, lam, xn), 0};
  std::fwrite(head, sizeof head, 1, out);
  std::fwrite(H, sizeof H, 1, out);
  std::fwrite(g, sizeof g, 1, out);
  std::fwrite(lam, sizeof lam, 1, out);
  std::fwrite(xn, sizeof xn, 1, out);

  std::vector<double> o1((size_t)n * 3, 0.0), o2((size_t)n * 3, 0.0), oc((size_t)n * 9, 0.0), oh((size_t)n * 9, 0.0);
  auto sym9 = [](const double (&G)[6], double *o) {
    const int at[9] = {0, 1, 2, 1, 3, 4, 2, 4, 5};
    for (int k = 0; k < 9; ++k) o[k] = G[at[k]];
  };
  for (int i = 0; i < n; ++i) {
    double gf1[3], gf2[3], Gg[6], Gh[6];
    if (head[0] != PNEC_HIP_SENS_OK) {
      for (double &v : gf1) v = lam[0];
      for (double &v : gf2) v = lam[0];
      for (double &v : Gg) v = lam[0];
      for (double &v : Gh) v = lam[0];
    } else {
      double d[NC];
      load(i, d);
      sens_gradients<MODE>(d, P, pr.reg, lam, gf1, gf2, Gg, Gh);
    }
    for (int j = 0; j < 3; ++j) {
      o1[(size_t)i * 3 + j] = gf1[j];
      o2[(size_t)i * 3 + j] = gf2[j];
    }
    if (MODE != PNEC_HIP_MODE_NEC) sym9(SensTraits<MODE>::kG ? Gg : Gh, &oc[(size_t)i * 9]);
    if (SensTraits<MODE>::kSym) sym9(Gh, &oh[(size_t)i * 9]);
  }
  for (const std::vector<double> *v : {&o1, &o2, &oc, &oh})
    if (!v->empty()) std::fwrite(v->data(), sizeof(double), v->size(), out);
}

bool get(std::FILE *f, void *p, size_t bytes) { return bytes == 0 || std::fread(p, bytes, 1, f) == 1; }

}  // namespace

int main(int argc, char **argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]);
    return 2;
  }
  std::FILE *in = std::fopen(argv[1], "rb"), *out = std::fopen(argv[2], "wb");
  if (!in || !out) {
    std::fprintf(stderr, "cannot open the files\n");
    return 2;
  }
  int32_t K = 0;
  bool ok = get(in, &K, sizeof K) && K >= 0;
  for (int32_t k = 0; ok && k < K; ++k) {
    Problem pr;
    int32_t head[4];
    ok = get(in, head, sizeof head) && head[0] >= 0 && head[0] <= 3 && head[1] >= 0 && head[1] <= (1 << 24);
    if (!ok) break;
    pr.mode = head[0], pr.n = head[1], pr.flags = head[2];
    ok = get(in, &pr.reg, sizeof pr.reg) && get(in, pr.q, sizeof pr.q) && get(in, pr.t, sizeof pr.t) && get(in, pr.gp, sizeof pr.gp);
    const int nc = pr.mode == PNEC_HIP_MODE_NEC ? 6 : (pr.mode == PNEC_HIP_MODE_SYM ? 18 : 12);
    pr.planes.resize((size_t)nc * pr.n);
    ok = ok && get(in, pr.planes.data(), pr.planes.size() * sizeof(double));
    if (!ok) break;
    switch (pr.mode) {
      case PNEC_HIP_MODE_NEC: run<PNEC_HIP_MODE_NEC>(pr, out); break;
      case PNEC_HIP_MODE_TARGET: run<PNEC_HIP_MODE_TARGET>(pr, out); break;
      case PNEC_HIP_MODE_HOST: run<PNEC_HIP_MODE_HOST>(pr, out); break;
      default: run<PNEC_HIP_MODE_SYM>(pr, out); break;
    }
  }
  std::fclose(in);
  if (std::fclose(out) != 0) ok = false;
  if (!ok) {
    std::fprintf(stderr, "malformed input\n");
    return 1;
  }
  std::printf("sensitivity_host: %d problem(s)\n", K);
  return 0;
}
