// undistort_host.cc -- what pnec::common::Undistort (pnec_amd/csrc/host/pnec_host.h) and pnec_hip_undistort_keypoints do
// before any device is touched, as a stand-alone host program for the address / undefined-behaviour sanitizers:
//   * UndistortCamera: 4 or 5 coefficients, K upper triangular with zero skew and last row (0, 0, 1), else
//     std::invalid_argument; the nine doubles in the ABI's order;
//   * the reference's rule dist_coef[0] == 0.0 (common.cc:74-76): points and covariances come back bit for bit with
//     status OK, whatever k2, p1, p2 are, for one point and for a vector; an empty vector; covs of another length;
//   * every refusal of the C ABI call comes back as PNEC_HIP_ERR_INVALID_ARGUMENT.
// tests/test_undistort_cpu.py builds it with pnec_host.cc under -fsanitize=address,undefined against libpnec_hip.so and
// runs it.  Prints one line per group; exit status 1 on the first failure.
#include <cstdio>
#include <cstring>
#include <limits>
#include <stdexcept>

#include "pnec_host.h"

namespace {

int g_failures = 0;
void expect(bool ok, const char *what) {
  if (ok) return;
  std::printf("FAIL %s\n", what);
  ++g_failures;
}

template <typename F>
bool throws_invalid(F &&f) {
  try {
    f();
  } catch (const std::invalid_argument &) {
    return true;
  }
  return false;
}

pnec::Matrix3d camera_matrix(double fx, double fy, double cx, double cy) {
  pnec::Matrix3d K;
  K(0, 0) = fx;
  K(1, 1) = fy;
  K(0, 2) = cx;
  K(1, 2) = cy;
  K(2, 2) = 1.0;
  return K;
}

void camera_cases() {
  using pnec::common::UndistortCamera;
  const pnec::Matrix3d K = camera_matrix(458.654, 457.296, 367.215, 248.375);
  const std::array<double, 9> c4 = UndistortCamera(K, {-0.28, 0.07, 1e-4, 2e-5});
  const double want4[9] = {458.654, 457.296, 367.215, 248.375, -0.28, 0.07, 1e-4, 2e-5, 0.0};
  expect(std::memcmp(c4.data(), want4, sizeof want4) == 0, "camera from four coefficients");
  const std::array<double, 9> c5 = UndistortCamera(K, {0.26, -0.95, -0.005, 0.003, 1.16});
  expect(c5[8] == 1.16 && c5[4] == 0.26, "camera from five coefficients");
  expect(throws_invalid([&] { UndistortCamera(K, {0.1, 0.2, 0.3}); }), "three coefficients are refused");
  expect(throws_invalid([&] { UndistortCamera(K, {0.1, 0.2, 0.3, 0.4, 0.5, 0.6}); }), "six coefficients are refused");
  expect(throws_invalid([&] { UndistortCamera(K, {}); }), "no coefficients are refused");
  pnec::Matrix3d skew = K;
  skew(0, 1) = 1e-3;
  expect(throws_invalid([&] { UndistortCamera(skew, {0.1, 0, 0, 0}); }), "skew is refused");
  pnec::Matrix3d lower = K;
  lower(1, 0) = 1e-3;
  expect(throws_invalid([&] { UndistortCamera(lower, {0.1, 0, 0, 0}); }), "a lower-triangle entry is refused");
  pnec::Matrix3d last = K;
  last(2, 2) = 2.0;
  expect(throws_invalid([&] { UndistortCamera(last, {0.1, 0, 0, 0}); }), "a last row other than (0, 0, 1) is refused");
  std::printf("%s camera: argument handling\n", g_failures ? "FAIL" : "ok  ");
}

void quirk_cases() {
  using namespace pnec::common;
  const int before = g_failures;
  const pnec::Matrix3d K = camera_matrix(700.0, 700.0, 320.0, 240.0);
  const std::vector<double> quirk = {0.0, 0.3, 1e-3, -5e-4};   // k1 == 0, the rest not
  const double nan = std::numeric_limits<double>::quiet_NaN();
  std::vector<Vector2d> pts = {{1.5, 2.5}, {639.0, 479.0}, {nan, -0.0}};
  std::vector<Covariance2d> covs = {{0.5, 0.1, 0.25}, {1.0, -0.2, 2.0}, {nan, 0.0, 1.0}};
  const std::vector<Vector2d> pts0 = pts;
  const std::vector<Covariance2d> covs0 = covs;
  UndistortOptions both;
  both.newton = both.propagate_cov = true;
  const std::vector<uint8_t> st = Undistort(pts, &covs, K, quirk, both);
  expect(st.size() == 3 && st[0] == PNEC_HIP_UNDISTORT_OK && st[1] == PNEC_HIP_UNDISTORT_OK && st[2] == PNEC_HIP_UNDISTORT_OK,
         "k1 == 0: every status OK");
  expect(std::memcmp(pts.data(), pts0.data(), sizeof(Vector2d) * 3) == 0, "k1 == 0: the points are the input's bits");
  expect(std::memcmp(covs.data(), covs0.data(), sizeof(Covariance2d) * 3) == 0, "k1 == 0: the covariances are the input's bits");
  const Vector2d one = Undistort(Vector2d{12.25, 400.5}, K, quirk);
  expect(one[0] == 12.25 && one[1] == 400.5, "k1 == 0: the single point comes back");
  std::vector<Vector2d> none;
  expect(Undistort(none, nullptr, K, {-0.05, 0.01, 0, 0}).empty() && none.empty(), "no points: no status, no device");
  std::vector<Covariance2d> two(2);
  expect(throws_invalid([&] { Undistort(pts, &two, K, {-0.05, 0.01, 0, 0}); }), "covs of another length are refused");
  expect(throws_invalid([&] { Undistort(pts, nullptr, K, {-0.05, 0.01}); }), "two coefficients are refused");
  std::printf("%s facade: the reference's k1 == 0 rule and the sizes\n", g_failures == before ? "ok  " : "FAIL");
}

void abi_refusals() {
  const int before = g_failures;
  double pts[4] = {1, 2, 3, 4}, cov[6] = {1, 0, 1, 1, 0, 1}, cam[9] = {700, 700, 320, 240, -0.05, 0.01, 0, 0, 0};
  double opts[4], ocov[6];
  uint8_t st[2];
  const int dev = 0, H = PNEC_HIP_MEM_HOST;
  const int bad = PNEC_HIP_ERR_INVALID_ARGUMENT;
  auto call = [&](int64_t n, const double *p1, const double *p2, const double *c2, const double *c1, const double *camera,
                  int32_t fixed, int32_t newton, uint32_t flags, double *o1, double *o2, double *oc2, double *oc1, uint8_t *s1,
                  uint8_t *s2, int space) {
    return pnec_hip_undistort_keypoints(dev, n, p1, p2, c2, c1, camera, fixed, newton, flags, o1, o2, oc2, oc1, s1, s2, space,
                                        nullptr);
  };
  const uint32_t N = PNEC_HIP_UNDISTORT_NEWTON;
  expect(call(2, pts, 0, 0, 0, cam, -1, 20, 0, opts, 0, 0, 0, st, 0, H) == bad, "fixed_iterations -1");
  expect(call(2, pts, 0, 0, 0, cam, 65, 20, 0, opts, 0, 0, 0, st, 0, H) == bad, "fixed_iterations 65");
  expect(call(2, pts, 0, 0, 0, cam, 5, -1, N, opts, 0, 0, 0, st, 0, H) == bad, "newton_iterations -1 with NEWTON");
  expect(call(2, pts, 0, 0, 0, cam, 5, 65, N, opts, 0, 0, 0, st, 0, H) == bad, "newton_iterations 65 with NEWTON");
  expect(call(2, pts, 0, 0, 0, cam, 5, 20, 4u, opts, 0, 0, 0, st, 0, H) == bad, "an unknown flag bit");
  expect(call(-1, pts, 0, 0, 0, cam, 5, 20, 0, opts, 0, 0, 0, st, 0, H) == bad, "n_rows -1");
  expect(call((int64_t)1 << 31, pts, 0, 0, 0, cam, 5, 20, 0, opts, 0, 0, 0, st, 0, H) == bad, "n_rows 2^31");
  expect(call(2, pts, 0, 0, 0, nullptr, 5, 20, 0, opts, 0, 0, 0, st, 0, H) == bad, "camera NULL");
  expect(call(2, pts, 0, 0, 0, cam, 5, 20, 0, nullptr, 0, 0, 0, 0, 0, H) == bad, "pts1 without out_pts1");
  expect(call(2, 0, 0, 0, 0, cam, 5, 20, 0, opts, 0, 0, 0, 0, 0, H) == bad, "out_pts1 without pts1");
  expect(call(2, pts, pts, 0, 0, cam, 5, 20, 0, opts, nullptr, 0, 0, 0, 0, H) == bad, "pts2 without out_pts2");
  expect(call(2, pts, 0, 0, cov, cam, 5, 20, 0, opts, 0, 0, nullptr, 0, 0, H) == bad, "cov1 without out_cov1");
  expect(call(2, pts, 0, 0, 0, cam, 5, 20, 0, opts, 0, 0, ocov, 0, 0, H) == bad, "out_cov1 without cov1");
  expect(call(2, pts, 0, cov, 0, cam, 5, 20, 0, opts, 0, ocov, 0, 0, 0, H) == bad, "cov2 without pts2");
  expect(call(2, 0, pts, 0, cov, cam, 5, 20, 0, 0, opts, 0, ocov, 0, 0, H) == bad, "cov1 without pts1");
  expect(call(2, pts, 0, 0, 0, cam, 5, 20, 0, opts, 0, 0, 0, 0, st, H) == bad, "out_status2 without pts2");
  expect(call(2, pts, 0, 0, 0, cam, 5, 20, 0, opts, 0, 0, 0, st, 0, 7) == bad, "a bad space");
  expect(call(0, 0, 0, 0, 0, cam, 5, 20, 0, 0, 0, 0, 0, 0, 0, H) == 0, "n_rows 0 returns 0");
  expect(call(0, 0, 0, 0, 0, cam, 5, 99, 0, 0, 0, 0, 0, 0, 0, H) == 0, "newton_iterations is not looked at without NEWTON");
  std::printf("%s abi: every refusal before a device is touched\n", g_failures == before ? "ok  " : "FAIL");
}

}  // namespace

int main() {
  camera_cases();
  quirk_cases();
  abi_refusals();
  if (g_failures) {
    std::printf("%d check(s) failed\n", g_failures);
    return 1;
  }
  std::printf("undistort host: every case held\n");
  return 0;
}
