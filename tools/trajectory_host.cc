// trajectory_host.cc -- what pnec::odometry::ComposeTrajectory / TrajectoryMetrics (pnec_amd/csrc/host/pnec_host.h) and
// pnec_hip_trajectory_compose / pnec_hip_trajectory_metrics do before any device is touched, as a stand-alone host program
// for the address / undefined-behaviour sanitizers:
//   * the facade: no poses give no poses (and no device), trajectories of different sizes throw std::invalid_argument, no
//     frames score NaN;
//   * every refusal of the two C ABI calls comes back as PNEC_HIP_ERR_INVALID_ARGUMENT, in both memory spaces where the
//     rule does not read an array, with a device number that does not exist; no rows is not a refusal.
// tests/test_trajectory_cpu.py builds it with pnec_host.cc under -fsanitize=address,undefined against libpnec_hip.so and
// runs it.  Prints one line per group; exit status 1 on the first failure.
#include <cmath>
#include <cstdio>
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

void facade_cases() {
  using namespace pnec::odometry;
  std::vector<uint8_t> valid = {7, 7};
  const std::vector<pnec::SE3d> none;
  expect(ComposeTrajectory(none, pnec::SE3d(), &valid).empty() && valid.empty(), "no relative poses: no poses, no device");
  expect(ComposeTrajectory(none).empty(), "no relative poses and no valid array");
  const std::vector<pnec::SE3d> two(2), three(3);
  expect(throws_invalid([&] { TrajectoryMetrics(two, three); }), "trajectories of different sizes are refused");
  const TrajectoryScore s = TrajectoryMetrics(none, none);
  expect(std::isnan(s.RPE_1) && std::isnan(s.RPE_n) && std::isnan(s.L1RPE_1) && std::isnan(s.L1RPE_n) && std::isnan(s.r_t) &&
             s.rmse_d.empty() && s.l1_d.empty() && s.angle1.empty() && s.rt1.empty(),
         "no frames: NaN, no device");
  std::printf("%s facade: sizes and the empty trajectory\n", g_failures ? "FAIL" : "ok  ");
}

const int kNoDevice = 1 << 20;
const int bad = PNEC_HIP_ERR_INVALID_ARGUMENT;

void compose_refusals() {
  const int before = g_failures;
  const int H = PNEC_HIP_MEM_HOST, D = PNEC_HIP_MEM_DEVICE;
  int64_t off[3] = {0, 2, 3};
  double q[12] = {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1}, t[9] = {}, sc[3] = {1, 1, 1}, q0[8] = {0, 0, 0, 1, 0, 0, 0, 1}, p0[6] = {};
  double oq[12], op[9];
  uint8_t ov[3];
  auto call = [&](int64_t n_seq, const int64_t *offsets, int64_t n_rows, const double *rq, const double *rt, const double *s,
                  const double *a0, const double *b0, double *out_q, double *out_p, uint8_t *out_valid, int space) {
    return pnec_hip_trajectory_compose(kNoDevice, n_seq, offsets, n_rows, rq, rt, s, a0, b0, out_q, out_p, out_valid, space,
                                       nullptr);
  };
  for (int space : {H, D}) {
    expect(call(0, off, 3, q, t, sc, q0, p0, oq, op, ov, space) == bad, "compose: n_seq 0");
    expect(call(-1, off, 3, q, t, sc, q0, p0, oq, op, ov, space) == bad, "compose: n_seq -1");
    expect(call(2, off, -1, q, t, sc, q0, p0, oq, op, ov, space) == bad, "compose: n_rows -1");
    expect(call(2, off, (int64_t)1 << 31, q, t, sc, q0, p0, oq, op, ov, space) == bad, "compose: n_rows 2^31");
    expect(call(2, nullptr, 3, q, t, sc, q0, p0, oq, op, ov, space) == bad, "compose: offsets NULL");
    expect(call(2, off, 3, nullptr, t, sc, q0, p0, oq, op, ov, space) == bad, "compose: rel_q NULL");
    expect(call(2, off, 3, q, t, sc, q0, p0, nullptr, op, ov, space) == bad, "compose: out_q NULL");
    expect(call(2, off, 3, q, nullptr, sc, q0, nullptr, oq, nullptr, ov, space) == bad, "compose: scale without rel_t");
    expect(call(2, off, 3, q, nullptr, nullptr, q0, p0, oq, nullptr, ov, space) == bad, "compose: p0 without rel_t");
    expect(call(2, off, 3, q, t, sc, q0, p0, oq, nullptr, ov, space) == bad, "compose: rel_t without out_p");
    expect(call(2, off, 3, q, nullptr, nullptr, q0, nullptr, oq, op, ov, space) == bad, "compose: out_p without rel_t");
    expect(call(2, off, 3, q, t, sc, q0, p0, q, op, ov, space) == bad, "compose: out_q is rel_q");
    expect(call(2, off, 3, q, t, sc, q0, p0, oq, t, ov, space) == bad, "compose: out_p is rel_t");
    expect(call(2, off, 3, q, t, sc, q0, p0, oq, oq, ov, space) == bad, "compose: out_p is out_q");
  }
  expect(call(2, off, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, D) == 0,
         "compose: no rows return 0 (DEVICE space: the offsets are not read)");
  expect(call(2, off, 3, q, t, sc, q0, p0, oq, op, ov, 7) == bad, "compose: a bad space");
  // HOST space reads the offsets: from 0, non-decreasing, within n_rows
  int64_t from1[3] = {1, 2, 3}, down[3] = {0, 3, 2}, beyond[3] = {0, 2, 4}, zero[3] = {0, 0, 0};
  expect(call(2, from1, 3, q, t, sc, q0, p0, oq, op, ov, H) == bad, "compose: offsets that do not start at 0");
  expect(call(2, down, 3, q, t, sc, q0, p0, oq, op, ov, H) == bad, "compose: offsets that step down");
  expect(call(2, beyond, 3, q, t, sc, q0, p0, oq, op, ov, H) == bad, "compose: offsets beyond n_rows");
  expect(call(2, zero, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, H) == 0,
         "compose: no rows return 0");
  std::printf("%s abi compose: every refusal before a device is touched\n", g_failures == before ? "ok  " : "FAIL");
}

void metrics_refusals() {
  const int before = g_failures;
  const int H = PNEC_HIP_MEM_HOST, D = PNEC_HIP_MEM_DEVICE;
  int64_t off[3] = {0, 2, 3};
  double eq[12] = {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1}, gq[12] = {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1}, ep[9] = {}, gp[9] = {};
  double m[10], e[12], r[3], l[3], a1[3], rt[3];
  auto call = [&](int64_t n_seq, const int64_t *offsets, int64_t n_rows, const double *est_q, const double *gt_q,
                  const double *est_p, const double *gt_p, double *om, double *oe, double *orm, double *ol, double *oa,
                  double *ort, int space) {
    return pnec_hip_trajectory_metrics(kNoDevice, n_seq, offsets, n_rows, est_q, gt_q, est_p, gt_p, om, oe, orm, ol, oa, ort,
                                       space, nullptr);
  };
  for (int space : {H, D}) {
    expect(call(0, off, 3, eq, gq, ep, gp, m, e, r, l, a1, rt, space) == bad, "metrics: n_seq 0");
    expect(call(2, off, -1, eq, gq, ep, gp, m, e, r, l, a1, rt, space) == bad, "metrics: n_rows -1");
    expect(call(2, off, (int64_t)1 << 31, eq, gq, ep, gp, m, e, r, l, a1, rt, space) == bad, "metrics: n_rows 2^31");
    expect(call(2, nullptr, 3, eq, gq, ep, gp, m, e, r, l, a1, rt, space) == bad, "metrics: offsets NULL");
    expect(call(2, off, 3, nullptr, gq, ep, gp, m, e, r, l, a1, rt, space) == bad, "metrics: est_q NULL");
    expect(call(2, off, 3, eq, nullptr, ep, gp, m, e, r, l, a1, rt, space) == bad, "metrics: gt_q NULL");
    expect(call(2, off, 3, eq, gq, ep, gp, nullptr, e, r, l, a1, rt, space) == bad, "metrics: out_metrics NULL");
    expect(call(2, off, 0, eq, gq, ep, gp, nullptr, e, r, l, a1, rt, space) == bad, "metrics: out_metrics NULL without rows");
    expect(call(2, off, 3, eq, gq, ep, gp, m, nullptr, r, l, a1, rt, space) == bad, "metrics: out_err_q NULL");
    expect(call(2, off, 3, eq, gq, ep, gp, m, e, nullptr, l, a1, rt, space) == bad, "metrics: out_rmse_d NULL");
    expect(call(2, off, 3, eq, gq, ep, gp, m, e, r, nullptr, a1, rt, space) == bad, "metrics: out_l1_d NULL");
    expect(call(2, off, 3, eq, gq, ep, nullptr, m, e, r, l, a1, nullptr, space) == bad, "metrics: est_p without gt_p");
    expect(call(2, off, 3, eq, gq, nullptr, gp, m, e, r, l, a1, nullptr, space) == bad, "metrics: gt_p without est_p");
    expect(call(2, off, 3, eq, gq, nullptr, nullptr, m, e, r, l, a1, rt, space) == bad, "metrics: out_rt1 without positions");
    expect(call(2, off, 3, eq, gq, ep, gp, m, eq, r, l, a1, rt, space) == bad, "metrics: out_err_q is est_q");
    expect(call(2, off, 3, eq, gq, ep, gp, m, e, r, l, a1, gp, space) == bad, "metrics: out_rt1 is gt_p");
    expect(call(2, off, 3, eq, gq, ep, gp, m, e, r, r, a1, rt, space) == bad, "metrics: out_l1_d is out_rmse_d");
  }
  expect(call(2, off, 3, eq, gq, ep, gp, m, e, r, l, a1, rt, -1) == bad, "metrics: a bad space");
  int64_t from1[3] = {1, 2, 3}, down[3] = {0, 3, 2}, beyond[3] = {0, 2, 4};
  expect(call(2, from1, 3, eq, gq, ep, gp, m, e, r, l, a1, rt, H) == bad, "metrics: offsets that do not start at 0");
  expect(call(2, down, 3, eq, gq, ep, gp, m, e, r, l, a1, rt, H) == bad, "metrics: offsets that step down");
  expect(call(2, beyond, 3, eq, gq, ep, gp, m, e, r, l, a1, rt, H) == bad, "metrics: offsets beyond n_rows");
  std::printf("%s abi metrics: every refusal before a device is touched\n", g_failures == before ? "ok  " : "FAIL");
}

}  // namespace

int main() {
  facade_cases();
  compose_refusals();
  metrics_refusals();
  if (g_failures) {
    std::printf("%d check(s) failed\n", g_failures);
    return 1;
  }
  std::printf("trajectory host: every case held\n");
  return 0;
}
