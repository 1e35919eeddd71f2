// pypnec.cpp -- the reference's pybind module surface for the hot path (python/pypnec.cpp:50-82,
// 244-258): pypnec.pyceres / pypnec.pyceresnec with the same call signatures, served by the
// MI355X solver through the host facade.  The KLT / image toy functions of the reference module
// are out of scope (image domain, hard-coded author paths at pypnec.cpp:95-99).
//
//   pyceres(host_bvs, target_bvs, host_covariances, target_covariances, init_pose, regularization) -> 4x4
//   pyceresnec(host_bvs, target_bvs, init_pose) -> 4x4
// host_bvs/target_bvs: sequence of 3-vectors (or an [N,3] array); covariances: sequence of 3x3
// (or [N,3,3]); init_pose: 4x4.  Addition: ceres_solver_batch over ragged lists of pairs.
#include <cstring>
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <array>
#include <string>
#include <vector>

#include "pnec_host.h"

namespace py = pybind11;
using arr = py::array_t<double, py::array::c_style | py::array::forcecast>;

namespace {

std::vector<pnec::Vector3d> ToBearings(const arr &a, const char *name) {
  if (a.ndim() != 2 || a.shape(1) != 3) throw std::invalid_argument(std::string(name) + " must be [N,3]");
  std::vector<pnec::Vector3d> out((size_t)a.shape(0));
  auto r = a.unchecked<2>();
  for (py::ssize_t i = 0; i < a.shape(0); ++i) out[(size_t)i] = pnec::Vector3d(r(i, 0), r(i, 1), r(i, 2));
  return out;
}

std::vector<pnec::Matrix3d> ToCovariances(const arr &a, const char *name) {
  if (a.ndim() != 3 || a.shape(1) != 3 || a.shape(2) != 3)
    throw std::invalid_argument(std::string(name) + " must be [N,3,3]");
  std::vector<pnec::Matrix3d> out((size_t)a.shape(0));
  auto r = a.unchecked<3>();
  for (py::ssize_t i = 0; i < a.shape(0); ++i)
    for (int row = 0; row < 3; ++row)
      for (int col = 0; col < 3; ++col) out[(size_t)i](row, col) = r(i, row, col);
  return out;
}

// Sophus::SE3d(Quaterniond(R).normalized().toRotationMatrix(), t)   (pypnec.cpp:56-59)
pnec::SE3d ToPose(const arr &m) {
  if (m.ndim() != 2 || m.shape(0) != 4 || m.shape(1) != 4) throw std::invalid_argument("init_pose must be 4x4");
  auto r = m.unchecked<2>();
  pnec::Matrix3d R;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) R(i, j) = r(i, j);
  return pnec::SE3d(pnec::Quaterniond(R).normalized().toRotationMatrix(),
                    pnec::Vector3d(r(0, 3), r(1, 3), r(2, 3)));
}

arr FromPose(const pnec::SE3d &T) {
  arr out({4, 4});
  const pnec::Matrix4d M = T.matrix();
  auto w = out.mutable_unchecked<2>();
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) w(i, j) = M[4 * i + j];
  return out;
}

arr pyceres(arr host_bvs, arr target_bvs, arr host_covariances, arr target_covariances, arr init_pose,
            double regularization) {
  const auto b1 = ToBearings(host_bvs, "host_bvs"), b2 = ToBearings(target_bvs, "target_bvs");
  const auto c1 = ToCovariances(host_covariances, "host_covariances");
  const auto c2 = ToCovariances(target_covariances, "target_covariances");
  const pnec::SE3d init = ToPose(init_pose);
  pnec::SE3d result;
  {
    py::gil_scoped_release release;
    pnec::optimization::PNECCeres optimizer;
    optimizer.InitValues(pnec::Quaterniond(init.rotationMatrix()), init.translation());
    optimizer.Optimize(b1, b2, c1, c2, regularization);
    result = optimizer.Result();
  }
  return FromPose(result);
}

arr pyceresnec(arr host_bvs, arr target_bvs, arr init_pose) {
  const auto b1 = ToBearings(host_bvs, "host_bvs"), b2 = ToBearings(target_bvs, "target_bvs");
  const pnec::SE3d init = ToPose(init_pose);
  pnec::SE3d result;
  {
    py::gil_scoped_release release;
    pnec::optimization::NECCeres optimizer;
    optimizer.InitValues(pnec::Quaterniond(init.rotationMatrix()), init.translation());
    optimizer.Optimize(b1, b2);
    result = optimizer.Result();
  }
  return FromPose(result);
}

// PNEC::CeresSolver (target-frame covariances, pnec.cc:350-370) over a list of pairs, one launch.
py::list ceres_solver_batch(py::list bvs1, py::list bvs2, py::list covs, py::list init_poses,
                            double regularization, std::vector<int> devices) {
  const size_t B = bvs1.size();
  if (bvs2.size() != B || covs.size() != B || init_poses.size() != B)
    throw std::invalid_argument("all lists must have one entry per frame pair");
  std::vector<pnec::rel_pose_estimation::FramePair> pairs(B);
  for (size_t p = 0; p < B; ++p) {
    pairs[p].bvs1 = ToBearings(bvs1[p].cast<arr>(), "bvs1[i]");
    pairs[p].bvs2 = ToBearings(bvs2[p].cast<arr>(), "bvs2[i]");
    pairs[p].projected_covs = ToCovariances(covs[p].cast<arr>(), "covs[i]");
    pairs[p].initial_pose = ToPose(init_poses[p].cast<arr>());
  }
  pnec::rel_pose_estimation::Options options;
  options.regularization_ = regularization;
  std::vector<pnec::SE3d> poses;
  {
    py::gil_scoped_release release;
    pnec::rel_pose_estimation::PNEC solver(options);
    poses = devices.empty() ? solver.CeresSolverBatch(pairs) : solver.CeresSolverBatch(pairs, devices);
  }
  py::list out;
  for (const auto &T : poses) out.append(FromPose(T));
  return out;
}

// PNEC::Solve with the reference's default Options (or the flags given) for a list of pairs: every
// stage one launch over the batch.  Returns (poses, inliers).
py::tuple solve_batch(py::list bvs1, py::list bvs2, py::list covs, py::list init_poses, bool use_ransac,
                      bool use_nec, bool use_ceres, int weighted_iterations, double regularization,
                      std::vector<int> devices, int eigensolver_scheme) {
  const size_t B = bvs1.size();
  if (bvs2.size() != B || covs.size() != B || init_poses.size() != B)
    throw std::invalid_argument("all lists must have one entry per frame pair");
  std::vector<pnec::rel_pose_estimation::FramePair> pairs(B);
  for (size_t p = 0; p < B; ++p) {
    pairs[p].bvs1 = ToBearings(bvs1[p].cast<arr>(), "bvs1[i]");
    pairs[p].bvs2 = ToBearings(bvs2[p].cast<arr>(), "bvs2[i]");
    pairs[p].projected_covs = ToCovariances(covs[p].cast<arr>(), "covs[i]");
    pairs[p].initial_pose = ToPose(init_poses[p].cast<arr>());
  }
  pnec::rel_pose_estimation::Options options;
  options.use_ransac_ = use_ransac;
  options.use_nec_ = use_nec;
  options.use_ceres_ = use_ceres;
  options.weighted_iterations_ = (size_t)weighted_iterations;
  options.regularization_ = regularization;
  options.eigensolver_scheme_ = eigensolver_scheme;
  std::vector<pnec::SE3d> poses;
  std::vector<std::vector<int>> inliers;
  {
    py::gil_scoped_release release;
    pnec::rel_pose_estimation::PNEC solver(options);
    poses = devices.empty() ? solver.SolveBatch(pairs, &inliers) : solver.SolveBatch(pairs, devices, &inliers);
  }
  py::list out, inl;
  for (const auto &T : poses) out.append(FromPose(T));
  for (const auto &v : inliers) inl.append(py::cast(v));
  return py::make_tuple(out, inl);
}

// additions used by the tests: the small pnec::common helpers of the facade
arr compose_m(arr bvs1, arr bvs2, arr rotation) {
  const auto b1 = ToBearings(bvs1, "bvs1"), b2 = ToBearings(bvs2, "bvs2");
  auto r = rotation.unchecked<2>();
  pnec::Matrix3d R;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) R(i, j) = r(i, j);
  const pnec::Matrix3d M = pnec::common::ComposeM(b1, b2, R);
  arr out({3, 3});
  auto w = out.mutable_unchecked<2>();
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) w(i, j) = M(i, j);
  return out;
}
arr translation_from_m(arr M) {
  auto r = M.unchecked<2>();
  pnec::Matrix3d Mm;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) Mm(i, j) = r(i, j);
  const pnec::Vector3d t = pnec::common::TranslationFromM(Mm);
  arr out({3});
  auto w = out.mutable_unchecked<1>();
  for (int i = 0; i < 3; ++i) w(i) = t[i];
  return out;
}

pnec::Matrix3d ToMatrix3(const arr &a, const char *name) {
  if (a.ndim() != 2 || a.shape(0) != 3 || a.shape(1) != 3) throw std::invalid_argument(std::string(name) + " must be 3x3");
  auto r = a.unchecked<2>();
  pnec::Matrix3d M;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) M(i, j) = r(i, j);
  return M;
}
pnec::Vector3d ToVector3(const arr &a, const char *name) {
  if (a.ndim() != 1 || a.shape(0) != 3) throw std::invalid_argument(std::string(name) + " must be a 3-vector");
  auto r = a.unchecked<1>();
  return pnec::Vector3d(r(0), r(1), r(2));
}
// pnec::common metric helpers of the facade (common.cc:210-259), degrees
double rotational_difference(arr R1, arr R2) {
  return pnec::common::RotationalDifference(ToMatrix3(R1, "rotation_1"), ToMatrix3(R2, "rotation_2"));
}
double translational_difference(arr t1, arr t2, bool both_directions) {
  return pnec::common::TranslationalDifference(ToVector3(t1, "translation_1"), ToVector3(t2, "translation_2"),
                                               both_directions);
}
double cost_function(arr bvs1, arr bvs2, arr covs, arr pose) {
  return pnec::common::CostFunction(ToBearings(bvs1, "bvs_1"), ToBearings(bvs2, "bvs_2"),
                                    ToCovariances(covs, "covs"), ToPose(pose));
}

py::array_t<double> pose_covariance(arr bvs1, arr bvs2, arr covs, arr pose, double regularization) {
  const pnec::Matrix6d C = pnec::common::PoseCovariance(ToBearings(bvs1, "bvs_1"), ToBearings(bvs2, "bvs_2"),
                                                        ToCovariances(covs, "covs"), ToPose(pose), regularization);
  py::array_t<double> out({6, 6});
  auto o = out.mutable_unchecked<2>();
  for (int r = 0; r < 6; ++r)
    for (int c = 0; c < 6; ++c) o(r, c) = C(r, c);
  return out;
}

// (grad_bvs1 [N,3], grad_bvs2 [N,3], grad_covs [N,3,3], lambda [5], newton [5], status) at `pose`
py::tuple pose_sensitivity(arr bvs1, arr bvs2, arr covs, arr pose, arr grad_pose, double regularization) {
  if (grad_pose.ndim() != 1 || grad_pose.shape(0) != 6) throw std::invalid_argument("grad_pose must be a 6-vector");
  std::array<double, 6> gp;
  for (int i = 0; i < 6; ++i) gp[i] = grad_pose.unchecked<1>()(i);
  const pnec::rel_pose_estimation::PoseSensitivityResult r = pnec::rel_pose_estimation::PoseSensitivity(
      ToBearings(bvs1, "bvs_1"), ToBearings(bvs2, "bvs_2"), ToCovariances(covs, "covs"), ToPose(pose), gp, regularization);
  const py::ssize_t n = (py::ssize_t)r.grad_bvs_1.size();
  py::array_t<double> g1({n, (py::ssize_t)3}), g2({n, (py::ssize_t)3}), gc({n, (py::ssize_t)3, (py::ssize_t)3}), lam(5), xn(5);
  auto o1 = g1.mutable_unchecked<2>(), o2 = g2.mutable_unchecked<2>();
  auto oc = gc.mutable_unchecked<3>();
  for (py::ssize_t i = 0; i < n; ++i)
    for (int j = 0; j < 3; ++j) {
      o1(i, j) = r.grad_bvs_1[i][j];
      o2(i, j) = r.grad_bvs_2[i][j];
      for (int k = 0; k < 3; ++k) oc(i, j, k) = r.grad_covs[i](j, k);
    }
  for (int i = 0; i < 5; ++i) {
    lam.mutable_unchecked<1>()(i) = r.lambda[i];
    xn.mutable_unchecked<1>()(i) = r.newton[i];
  }
  return py::make_tuple(g1, g2, gc, lam, xn, r.status);
}

// covs_host (optional): the covariances of frame 1 -> the symmetric residual's two-covariance overloads
py::array_t<double> residuals(arr bvs1, arr bvs2, arr covs, arr pose, double regularization, py::object covs_host) {
  const std::vector<double> r =
      covs_host.is_none()
          ? pnec::common::Residuals(ToBearings(bvs1, "bvs_1"), ToBearings(bvs2, "bvs_2"), ToCovariances(covs, "covs"),
                                    ToPose(pose), regularization)
          : pnec::common::Residuals(ToBearings(bvs1, "bvs_1"), ToBearings(bvs2, "bvs_2"),
                                    ToCovariances(covs_host.cast<arr>(), "covs_host"), ToCovariances(covs, "covs"),
                                    ToPose(pose), regularization);
  py::array_t<double> out((py::ssize_t)r.size());
  auto o = out.mutable_unchecked<1>();
  for (size_t i = 0; i < r.size(); ++i) o((py::ssize_t)i) = r[i];
  return out;
}

std::vector<int> gate_inliers(arr bvs1, arr bvs2, arr covs, arr pose, double gate, double regularization,
                              py::object covs_host) {
  if (covs_host.is_none())
    return pnec::common::GateInliers(ToBearings(bvs1, "bvs_1"), ToBearings(bvs2, "bvs_2"), ToCovariances(covs, "covs"),
                                     ToPose(pose), gate, regularization);
  return pnec::common::GateInliers(ToBearings(bvs1, "bvs_1"), ToBearings(bvs2, "bvs_2"),
                                   ToCovariances(covs_host.cast<arr>(), "covs_host"), ToCovariances(covs, "covs"),
                                   ToPose(pose), gate, regularization);
}

// (points [N,3], depth1 [N], depth2 [N], front [N] uint8) at `pose` as given, lengths in baselines
py::tuple triangulate(arr bvs1, arr bvs2, arr pose) {
  std::vector<double> d1, d2;
  std::vector<uint8_t> front;
  const std::vector<pnec::Vector3d> pts =
      pnec::common::Triangulate(ToBearings(bvs1, "bvs_1"), ToBearings(bvs2, "bvs_2"), ToPose(pose), &d1, &d2, &front);
  const py::ssize_t n = (py::ssize_t)pts.size();
  py::array_t<double> P({n, (py::ssize_t)3}), D1(n), D2(n);
  py::array_t<uint8_t> F(n);
  auto p = P.mutable_unchecked<2>();
  auto a = D1.mutable_unchecked<1>();
  auto b = D2.mutable_unchecked<1>();
  auto f = F.mutable_unchecked<1>();
  for (py::ssize_t i = 0; i < n; ++i) {
    for (int k = 0; k < 3; ++k) p(i, k) = pts[(size_t)i][k];
    a(i) = d1[(size_t)i];
    b(i) = d2[(size_t)i];
    f(i) = front[(size_t)i];
  }
  return py::make_tuple(P, D1, D2, F);
}

arr orient_translation(arr bvs1, arr bvs2, arr pose) {
  return FromPose(pnec::common::OrientTranslation(ToBearings(bvs1, "bvs_1"), ToBearings(bvs2, "bvs_2"), ToPose(pose)));
}

// EMPoseEstimation(bvs1, bvs2, identity, EIGHTPT, ransac = false): 4x4, the translation of length s0
arr eight_point(arr bvs1, arr bvs2) {
  const auto b1 = ToBearings(bvs1, "bvs_1"), b2 = ToBearings(bvs2, "bvs_2");
  pnec::SE3d result;
  {
    py::gil_scoped_release release;
    result = pnec::rel_pose_estimation::EMPoseEstimation(b1, b2, pnec::SE3d(), pnec::rel_pose_estimation::EIGHTPT, false);
  }
  return FromPose(result);
}

// pnec::common::Undistort, batched: (points [n,2], covs [n,3] or None, status uint8 [n])
py::tuple undistort(arr points, arr K, std::vector<double> dist, py::object covs, bool newton, bool propagate_cov) {
  if (points.ndim() != 2 || points.shape(1) != 2) throw std::invalid_argument("points must be [N,2]");
  const size_t n = (size_t)points.shape(0);
  std::vector<pnec::common::Vector2d> pts(n);
  auto r = points.unchecked<2>();
  for (size_t i = 0; i < n; ++i) pts[i] = {r((py::ssize_t)i, 0), r((py::ssize_t)i, 1)};
  std::vector<pnec::common::Covariance2d> cv;
  const bool with_cov = !covs.is_none();
  if (with_cov) {
    const arr c = covs.cast<arr>();
    if (c.ndim() != 2 || c.shape(1) != 3 || (size_t)c.shape(0) != n)
      throw std::invalid_argument("covs must be [N,3]: (xx, xy, yy) per point");
    auto rc = c.unchecked<2>();
    cv.resize(n);
    for (size_t i = 0; i < n; ++i) cv[i] = {rc((py::ssize_t)i, 0), rc((py::ssize_t)i, 1), rc((py::ssize_t)i, 2)};
  }
  pnec::common::UndistortOptions options;
  options.newton = newton;
  options.propagate_cov = propagate_cov;
  const pnec::Matrix3d Km = ToMatrix3(K, "K");
  std::vector<uint8_t> status;
  {
    py::gil_scoped_release release;
    status = pnec::common::Undistort(pts, with_cov ? &cv : nullptr, Km, dist, options);
  }
  arr out_pts({(py::ssize_t)n, (py::ssize_t)2});
  py::array_t<uint8_t> out_status((py::ssize_t)n);
  auto wp = out_pts.mutable_unchecked<2>();
  auto ws = out_status.mutable_unchecked<1>();
  for (size_t i = 0; i < n; ++i) {
    wp((py::ssize_t)i, 0) = pts[i][0];
    wp((py::ssize_t)i, 1) = pts[i][1];
    ws((py::ssize_t)i) = status[i];
  }
  py::object out_cov = py::none();
  if (with_cov) {
    arr oc({(py::ssize_t)n, (py::ssize_t)3});
    auto wc = oc.mutable_unchecked<2>();
    for (size_t i = 0; i < n; ++i)
      for (int k = 0; k < 3; ++k) wc((py::ssize_t)i, k) = cv[i][(size_t)k];
    out_cov = oc;
  }
  return py::make_tuple(out_pts, out_cov, out_status);
}

// poses [N,4,4] -> SE3d; a pose that is not finite stays so (ToPose would normalise a NaN rotation just the same)
std::vector<pnec::SE3d> ToPoses(const arr &a, const char *name) {
  if (a.ndim() != 3 || a.shape(1) != 4 || a.shape(2) != 4) throw std::invalid_argument(std::string(name) + " must be [N,4,4]");
  std::vector<pnec::SE3d> out((size_t)a.shape(0));
  auto r = a.unchecked<3>();
  for (py::ssize_t i = 0; i < a.shape(0); ++i) {
    pnec::Matrix3d R;
    for (int row = 0; row < 3; ++row)
      for (int col = 0; col < 3; ++col) R(row, col) = r(i, row, col);
    out[(size_t)i] = pnec::SE3d(R, pnec::Vector3d(r(i, 0, 3), r(i, 1, 3), r(i, 2, 3)));
  }
  return out;
}

arr FromDoubles(const std::vector<double> &v) {
  arr out((py::ssize_t)v.size());
  auto w = out.mutable_unchecked<1>();
  for (size_t i = 0; i < v.size(); ++i) w((py::ssize_t)i) = v[i];
  return out;
}

// pnec::odometry::ComposeTrajectory: (poses [N,4,4], valid uint8 [N])
py::tuple compose_trajectory(arr relative_poses, py::object correction) {
  const std::vector<pnec::SE3d> rel = ToPoses(relative_poses, "relative_poses");
  const pnec::SE3d left = correction.is_none() ? pnec::SE3d() : ToPose(correction.cast<arr>());
  std::vector<pnec::SE3d> poses;
  std::vector<uint8_t> valid;
  {
    py::gil_scoped_release release;
    poses = pnec::odometry::ComposeTrajectory(rel, left, &valid);
  }
  const py::ssize_t n = (py::ssize_t)poses.size();
  arr out({n, (py::ssize_t)4, (py::ssize_t)4});
  py::array_t<uint8_t> out_valid(n);
  auto w = out.mutable_unchecked<3>();
  auto wv = out_valid.mutable_unchecked<1>();
  for (py::ssize_t i = 0; i < n; ++i) {
    const pnec::Matrix4d M = poses[(size_t)i].matrix();
    for (int r = 0; r < 4; ++r)
      for (int c = 0; c < 4; ++c) w(i, r, c) = M[4 * r + c];
    wv(i) = valid[(size_t)i];
  }
  return py::make_tuple(out, out_valid);
}

// pnec::odometry::TrajectoryMetrics: a dict of the five metrics (radians) and the per-distance / per-step arrays
py::dict trajectory_metrics(arr estimated, arr ground_truth) {
  const std::vector<pnec::SE3d> est = ToPoses(estimated, "estimated"), gt = ToPoses(ground_truth, "ground_truth");
  pnec::odometry::TrajectoryScore s;
  {
    py::gil_scoped_release release;
    s = pnec::odometry::TrajectoryMetrics(est, gt);
  }
  py::dict d;
  d["RPE_1"] = s.RPE_1;
  d["RPE_n"] = s.RPE_n;
  d["L1RPE_1"] = s.L1RPE_1;
  d["L1RPE_n"] = s.L1RPE_n;
  d["r_t"] = s.r_t;
  d["rmse_d"] = FromDoubles(s.rmse_d);
  d["l1_d"] = FromDoubles(s.l1_d);
  d["angle1"] = FromDoubles(s.angle1);
  d["rt1"] = FromDoubles(s.rt1);
  return d;
}

using iarr64 = py::array_t<int64_t, py::array::c_style | py::array::forcecast>;
using iarr32 = py::array_t<int32_t, py::array::c_style | py::array::forcecast>;

// pnec::features::LinkTracks: int32 [len(cur_ids)]
iarr32 link_tracks(iarr64 prev_ids, iarr64 cur_ids) {
  if (prev_ids.ndim() != 1 || cur_ids.ndim() != 1) throw std::invalid_argument("prev_ids and cur_ids must be one-dimensional");
  const std::vector<int64_t> prev(prev_ids.data(), prev_ids.data() + prev_ids.size()),
      cur(cur_ids.data(), cur_ids.data() + cur_ids.size());
  std::vector<int32_t> link;
  {
    py::gil_scoped_release release;
    link = pnec::features::LinkTracks(prev, cur);
  }
  iarr32 out((py::ssize_t)link.size());
  if (!link.empty()) std::memcpy(out.mutable_data(), link.data(), link.size() * sizeof(int32_t));
  return out;
}

// pnec::odometry::AdvanceTrajectory: (s [n], q [n,4], p [n,3], status int32 [n])
py::tuple advance_trajectory(arr s, arr q, arr p, arr rel_q, arr rel_t, py::object count, int min_count, py::object scale3,
                             py::object n_used, int min_used) {
  const size_t n = (size_t)s.size();
  if (s.ndim() != 1 || q.ndim() != 2 || q.shape(0) != (py::ssize_t)n || q.shape(1) != 4 || p.ndim() != 2 ||
      p.shape(0) != (py::ssize_t)n || p.shape(1) != 3)
    throw std::invalid_argument("the state is s [n], q [n,4], p [n,3]");
  if (rel_q.ndim() != 2 || rel_q.shape(0) != (py::ssize_t)n || rel_q.shape(1) != 4 || rel_t.ndim() != 2 ||
      rel_t.shape(0) != (py::ssize_t)n || rel_t.shape(1) != 3)
    throw std::invalid_argument("rel_q must be [n,4] (xyzw), rel_t [n,3]");
  auto doubles = [](const arr &a) { return std::vector<double>(a.data(), a.data() + a.size()); };
  auto ints = [](const iarr32 &a) { return std::vector<int32_t>(a.data(), a.data() + a.size()); };
  pnec::odometry::TrajectoryState state(n), next(n);
  state.s = doubles(s);
  state.q = doubles(q);
  state.p = doubles(p);
  const std::vector<double> rq = doubles(rel_q), rt = doubles(rel_t);
  std::vector<int32_t> cnt, used;
  std::vector<double> sc;
  if (!count.is_none()) cnt = ints(count.cast<iarr32>());
  if (!n_used.is_none()) used = ints(n_used.cast<iarr32>());
  if (!scale3.is_none()) sc = doubles(scale3.cast<arr>());
  std::vector<int32_t> status;
  {
    py::gil_scoped_release release;
    status = pnec::odometry::AdvanceTrajectory(state, rq, rt, &next, count.is_none() ? nullptr : &cnt, min_count,
                                               scale3.is_none() ? nullptr : &sc, n_used.is_none() ? nullptr : &used, min_used);
  }
  arr out_q({(py::ssize_t)n, (py::ssize_t)4}), out_p({(py::ssize_t)n, (py::ssize_t)3});
  iarr32 out_status((py::ssize_t)n);
  if (n) {
    std::memcpy(out_q.mutable_data(), next.q.data(), 4 * n * sizeof(double));
    std::memcpy(out_p.mutable_data(), next.p.data(), 3 * n * sizeof(double));
    std::memcpy(out_status.mutable_data(), status.data(), n * sizeof(int32_t));
  }
  return py::make_tuple(FromDoubles(next.s), out_q, out_p, out_status);
}

// MinimalEMPoseEstimation(bvs1, bvs2, identity, NISTER | SEVENPT): 4x4, the translation of length s0
arr minimal_pose(arr bvs1, arr bvs2, pnec::rel_pose_estimation::algorithm_t algorithm) {
  const auto b1 = ToBearings(bvs1, "bvs_1"), b2 = ToBearings(bvs2, "bvs_2");
  pnec::SE3d result;
  {
    py::gil_scoped_release release;
    result = pnec::rel_pose_estimation::MinimalEMPoseEstimation(b1, b2, pnec::SE3d(), algorithm);
  }
  return FromPose(result);
}
arr five_point(arr bvs1, arr bvs2) { return minimal_pose(bvs1, bvs2, pnec::rel_pose_estimation::NISTER); }
arr seven_point(arr bvs1, arr bvs2) { return minimal_pose(bvs1, bvs2, pnec::rel_pose_estimation::SEVENPT); }

// RansacEMPoseEstimation(bvs1, bvs2, identity, algorithm, ...): (4x4, inlier indices)
py::tuple essential_ransac(arr bvs1, arr bvs2, const std::string &algorithm, int max_iterations, double threshold,
                           uint64_t seed) {
  namespace rp = pnec::rel_pose_estimation;
  rp::algorithm_t alg;
  if (algorithm == "nister") alg = rp::NISTER;
  else if (algorithm == "sevenpt") alg = rp::SEVENPT;
  else if (algorithm == "eightpt") alg = rp::EIGHTPT;
  else throw std::invalid_argument("algorithm must be \"nister\", \"sevenpt\" or \"eightpt\"");
  const auto b1 = ToBearings(bvs1, "bvs_1"), b2 = ToBearings(bvs2, "bvs_2");
  pnec::SE3d result;
  std::vector<int> inliers;
  {
    py::gil_scoped_release release;
    result = rp::RansacEMPoseEstimation(b1, b2, pnec::SE3d(), alg, &inliers, max_iterations, threshold, seed);
  }
  py::array_t<int> idx((py::ssize_t)inliers.size());
  auto w = idx.mutable_unchecked<1>();
  for (py::ssize_t i = 0; i < (py::ssize_t)inliers.size(); ++i) w(i) = inliers[(size_t)i];
  return py::make_tuple(FromPose(result), idx);
}

// (scale, q25, q75, n_used, ratio [N]) of one frame against the previous one
py::tuple relative_scale(arr bvs_prev1, arr bvs_prev2, arr pose_prev, arr bvs1, arr bvs2, arr pose,
                         const std::vector<int> &link, double min_parallax) {
  double q25 = 0.0, q75 = 0.0;
  int n_used = 0;
  std::vector<double> ratios;
  const double scale = pnec::common::RelativeScale(ToBearings(bvs_prev1, "bvs_prev_1"), ToBearings(bvs_prev2, "bvs_prev_2"),
                                                   ToPose(pose_prev), ToBearings(bvs1, "bvs_1"), ToBearings(bvs2, "bvs_2"),
                                                   ToPose(pose), link, min_parallax, &q25, &q75, &n_used, &ratios);
  py::array_t<double> R((py::ssize_t)ratios.size());
  auto r = R.mutable_unchecked<1>();
  for (py::ssize_t i = 0; i < (py::ssize_t)ratios.size(); ++i) r(i) = ratios[(size_t)i];
  return py::make_tuple(scale, q25, q75, n_used, R);
}

// (cov [N,3] = xx, xy, yy; status [N]) of the keypoints `points` [N,2] (x = column, y = row) of one image
py::tuple patch_covariance(py::array image, arr points, double scaling) {
  if (image.ndim() != 2) throw std::invalid_argument("image must be [h,w]");
  pnec_hip_pixel_type type;
  if (image.dtype().is(py::dtype::of<uint8_t>())) type = PNEC_HIP_PIXEL_U8;
  else if (image.dtype().is(py::dtype::of<uint16_t>())) type = PNEC_HIP_PIXEL_U16;
  else if (image.dtype().is(py::dtype::of<float>())) type = PNEC_HIP_PIXEL_F32;
  else throw std::invalid_argument("image must be uint8, uint16 or float32");
  const py::ssize_t es = image.itemsize();
  if (image.strides(1) != es || image.strides(0) % es != 0 || image.strides(0) < image.shape(1) * es)
    throw std::invalid_argument("image rows must be contiguous (a row pitch is allowed)");
  if (points.ndim() != 2 || points.shape(1) != 2) throw std::invalid_argument("points must be [N,2]");
  const py::ssize_t n = points.shape(0);
  std::vector<std::array<double, 2>> pts((size_t)n);
  auto r = points.unchecked<2>();
  for (py::ssize_t i = 0; i < n; ++i) pts[(size_t)i] = {r(i, 0), r(i, 1)};
  std::vector<int> status;
  const auto cov = pnec::features::PatchCovariances(image.data(), type, (int)image.shape(0), (int)image.shape(1),
                                                    (int64_t)(image.strides(0) / es), pts, scaling, nullptr, &status);
  py::array_t<double> C({n, (py::ssize_t)3});
  py::array_t<int32_t> S(n);
  auto c = C.mutable_unchecked<2>();
  auto s = S.mutable_unchecked<1>();
  for (py::ssize_t i = 0; i < n; ++i) {
    for (int k = 0; k < 3; ++k) c(i, k) = cov[(size_t)i][(size_t)k];
    s(i) = status[(size_t)i];
  }
  return py::make_tuple(C, S);
}

static pnec_hip_pixel_type pixel_type_of(const py::array &image) {
  if (image.dtype().is(py::dtype::of<uint8_t>())) return PNEC_HIP_PIXEL_U8;
  if (image.dtype().is(py::dtype::of<uint16_t>())) return PNEC_HIP_PIXEL_U16;
  if (image.dtype().is(py::dtype::of<float>())) return PNEC_HIP_PIXEL_F32;
  throw std::invalid_argument("image must be uint8, uint16 or float32");
}

static pnec::features::Pyramid pyramid_of(const py::array &image, int levels) {
  if (image.ndim() != 2) throw std::invalid_argument("image must be [h,w]");
  const pnec_hip_pixel_type type = pixel_type_of(image);
  const py::ssize_t es = image.itemsize();
  if (image.strides(1) != es || image.strides(0) % es != 0 || image.strides(0) < image.shape(1) * es)
    throw std::invalid_argument("image rows must be contiguous (a row pitch is allowed)");
  return pnec::features::ImagePyramid(image.data(), type, (int)image.shape(0), (int)image.shape(1),
                                      (int64_t)(image.strides(0) / es), levels);
}

// the levels of one image's pyramid as a list of arrays of the image's dtype
py::list image_pyramid(py::array image, int levels) {
  const pnec::features::Pyramid p = pyramid_of(image, levels);
  py::list out;
  for (size_t l = 0; l < p.levels.size(); ++l) {
    py::array a(image.dtype(), std::vector<py::ssize_t>{(py::ssize_t)(p.height >> l), (py::ssize_t)(p.width >> l)});
    std::memcpy(a.mutable_data(), p.levels[l].data(), p.levels[l].size());
    out.append(a);
  }
  return out;
}

// (pts [N,2], angle [N], cov [N,3], dist2 [N], status [N], lost_level [N]) of the patches at `points` of `image1`
// tracked into `image2` and back
py::tuple patch_track(py::array image1, py::array image2, arr points, int levels, int max_iterations,
                      double max_recovered_dist2, bool backward, double scaling, double shift_x, double shift_y) {
  if (points.ndim() != 2 || points.shape(1) != 2) throw std::invalid_argument("points must be [N,2]");
  const pnec::features::Pyramid p1 = pyramid_of(image1, levels), p2 = pyramid_of(image2, levels);
  const py::ssize_t n = points.shape(0);
  std::vector<std::array<double, 2>> pts((size_t)n);
  auto r = points.unchecked<2>();
  for (py::ssize_t i = 0; i < n; ++i) pts[(size_t)i] = {r(i, 0), r(i, 1)};
  pnec::features::TrackOptions o;
  o.max_iterations = max_iterations;
  o.max_recovered_dist2 = max_recovered_dist2;
  o.backward = backward;
  o.scaling = scaling;
  o.shift = {shift_x, shift_y};
  const pnec::features::PatchTracks t = pnec::features::TrackPatches(p1, p2, pts, o);
  py::array_t<double> P({n, (py::ssize_t)2}), A(n), Cv({n, (py::ssize_t)3}), D(n);
  py::array_t<int32_t> S(n), Lv(n);
  auto pp = P.mutable_unchecked<2>();
  auto cc = Cv.mutable_unchecked<2>();
  auto aa = A.mutable_unchecked<1>();
  auto dd = D.mutable_unchecked<1>();
  auto ss = S.mutable_unchecked<1>();
  auto ll = Lv.mutable_unchecked<1>();
  for (py::ssize_t i = 0; i < n; ++i) {
    for (int k = 0; k < 2; ++k) pp(i, k) = t.points[(size_t)i][(size_t)k];
    for (int k = 0; k < 3; ++k) cc(i, k) = t.covariances[(size_t)i][(size_t)k];
    aa(i) = t.angles[(size_t)i];
    dd(i) = t.dist2[(size_t)i];
    ss(i) = t.status[(size_t)i];
    ll(i) = t.lost_level[(size_t)i];
  }
  return py::make_tuple(P, A, Cv, D, S, Lv);
}

using iarr64 = py::array_t<int64_t, py::array::c_style | py::array::forcecast>;
using iarr32 = py::array_t<int32_t, py::array::c_style | py::array::forcecast>;

template <size_t W>
std::vector<std::array<double, W>> rows_of(const arr &a, const char *what) {
  if (a.ndim() != 2 || a.shape(1) != (py::ssize_t)W) throw std::invalid_argument(std::string(what) + " has the wrong shape");
  std::vector<std::array<double, W>> v((size_t)a.shape(0));
  auto r = a.unchecked<2>();
  for (py::ssize_t i = 0; i < a.shape(0); ++i)
    for (size_t k = 0; k < W; ++k) v[(size_t)i][k] = r(i, (py::ssize_t)k);
  return v;
}
template <size_t W>
py::array_t<double> array_of(const std::vector<std::array<double, W>> &v) {
  py::array_t<double> a({(py::ssize_t)v.size(), (py::ssize_t)W});
  auto w = a.mutable_unchecked<2>();
  for (size_t i = 0; i < v.size(); ++i)
    for (size_t k = 0; k < W; ++k) w((py::ssize_t)i, (py::ssize_t)k) = v[i][k];
  return a;
}
template <typename T, typename V>
py::array_t<T> vector_of(const V &v) {
  py::array_t<T> a((py::ssize_t)v.size());
  auto w = a.template mutable_unchecked<1>();
  for (size_t i = 0; i < v.size(); ++i) w((py::ssize_t)i) = (T)v[i];
  return a;
}

pnec::features::Tracks tracks_of(iarr64 id, iarr32 tmpl_image, arr tmpl_pts, iarr32 age, arr pts, py::object angle,
                                 py::object cov) {
  pnec::features::Tracks t;
  t.id.assign(id.data(), id.data() + id.size());
  t.tmpl_image.assign(tmpl_image.data(), tmpl_image.data() + tmpl_image.size());
  t.age.assign(age.data(), age.data() + age.size());
  t.tmpl_points = rows_of<2>(tmpl_pts, "tmpl_pts");
  t.points = rows_of<2>(pts, "pts");
  if (!angle.is_none()) {
    arr a = angle.cast<arr>();
    t.angles.assign(a.data(), a.data() + a.size());
  }
  if (!cov.is_none()) t.covariances = rows_of<3>(cov.cast<arr>(), "cov");
  return t;
}

// one image's surviving tracks: (id, tmpl_image, tmpl_pts, age, pts, angle, cov or None, prev_pts, prev_cov or None,
// src), trimmed to the retained rows -- the first offsets[1] rows of pnec_amd.retain_tracks
py::tuple retain_tracks(iarr64 id, iarr32 tmpl_image, arr tmpl_pts, iarr32 age, arr pts, py::object cov, arr trk_pts,
                        arr trk_angle, py::object trk_cov, iarr32 trk_status, int max_age) {
  if (cov.is_none() != trk_cov.is_none()) throw std::invalid_argument("cov and trk_cov are given or None together");
  const pnec::features::Tracks t = tracks_of(id, tmpl_image, tmpl_pts, age, pts, py::none(), cov);
  pnec::features::PatchTracks r;
  r.points = rows_of<2>(trk_pts, "trk_pts");
  r.angles.assign(trk_angle.data(), trk_angle.data() + trk_angle.size());
  if (!trk_cov.is_none()) r.covariances = rows_of<3>(trk_cov.cast<arr>(), "trk_cov");
  r.status.assign(trk_status.data(), trk_status.data() + trk_status.size());
  const pnec::features::Tracks o = pnec::features::RetainTracks(t, r, max_age);
  const bool c = !cov.is_none();
  return py::make_tuple(vector_of<int64_t>(o.id), vector_of<int32_t>(o.tmpl_image), array_of<2>(o.tmpl_points),
                        vector_of<int32_t>(o.age), array_of<2>(o.points), vector_of<double>(o.angles),
                        c ? py::object(array_of<3>(o.covariances)) : py::object(py::none()), array_of<2>(o.prev_points),
                        c ? py::object(array_of<3>(o.prev_covariances)) : py::object(py::none()), vector_of<int64_t>(o.src));
}

// one image's refill: ((id, tmpl_image, tmpl_pts, age, pts, angle, cov or None), next_id after, dropped); `tracks` is
// None or the tuple (id, tmpl_image, tmpl_pts, age, pts, angle, cov or None)
py::tuple append_tracks(py::object tracks, arr det_pts, py::object det_cov, int tmpl_image, int64_t capacity, int64_t next_id) {
  pnec::features::Tracks t;
  const bool have = !tracks.is_none();
  if (have) {
    py::tuple s = tracks.cast<py::tuple>();
    if (s.size() != 7) throw std::invalid_argument("tracks must be (id, tmpl_image, tmpl_pts, age, pts, angle, cov or None)");
    t = tracks_of(s[0].cast<iarr64>(), s[1].cast<iarr32>(), s[2].cast<arr>(), s[3].cast<iarr32>(), s[4].cast<arr>(), s[5], s[6]);
  }
  pnec::features::Keypoints k;
  k.points = rows_of<2>(det_pts, "det_pts");
  std::vector<std::array<double, 3>> dc;
  if (!det_cov.is_none()) dc = rows_of<3>(det_cov.cast<arr>(), "det_cov");
  int64_t dropped = 0;
  const pnec::features::Tracks o = pnec::features::AppendTracks(have ? &t : nullptr, k, det_cov.is_none() ? nullptr : &dc,
                                                                tmpl_image, capacity, &next_id, &dropped);
  const bool c = !o.covariances.empty() || (o.id.empty() && !det_cov.is_none());
  return py::make_tuple(py::make_tuple(vector_of<int64_t>(o.id), vector_of<int32_t>(o.tmpl_image), array_of<2>(o.tmpl_points),
                                       vector_of<int32_t>(o.age), array_of<2>(o.points), vector_of<double>(o.angles),
                                       c ? py::object(array_of<3>(o.covariances)) : py::object(py::none())),
                        next_id, dropped);
}

// (pts [N,2], score [N], cell_index [N], cell [n_cells]) of the grid FAST-9 corners of one uint8 / uint16 image
py::tuple detect_keypoints(py::array image, int grid, int points_per_cell, int min_threshold, int edge, py::object current) {
  if (image.ndim() != 2) throw std::invalid_argument("image must be [h,w]");
  const pnec_hip_pixel_type type = pixel_type_of(image);
  if (type == PNEC_HIP_PIXEL_F32) throw std::invalid_argument("image must be uint8 or uint16");
  const py::ssize_t es = image.itemsize();
  if (image.strides(1) != es || image.strides(0) % es != 0 || image.strides(0) < image.shape(1) * es)
    throw std::invalid_argument("image rows must be contiguous (a row pitch is allowed)");
  std::vector<std::array<double, 2>> cur;
  if (!current.is_none()) {
    arr c = current.cast<arr>();
    if (c.ndim() != 2 || c.shape(1) != 2) throw std::invalid_argument("current must be [n,2]");
    auto r = c.unchecked<2>();
    cur.resize((size_t)c.shape(0));
    for (py::ssize_t i = 0; i < c.shape(0); ++i) cur[(size_t)i] = {r(i, 0), r(i, 1)};
  }
  pnec::features::DetectOptions o;
  o.grid = grid;
  o.points_per_cell = points_per_cell;
  o.min_threshold = min_threshold;
  o.edge = edge;
  const pnec::features::Keypoints k = pnec::features::DetectKeypoints(
      image.data(), type, (int)image.shape(0), (int)image.shape(1), (int64_t)(image.strides(0) / es), o,
      cur.empty() ? nullptr : &cur);
  const py::ssize_t n = (py::ssize_t)k.points.size(), nc = (py::ssize_t)k.cell.size();
  py::array_t<double> P({n, (py::ssize_t)2});
  py::array_t<int32_t> S(n), I(n), Cl(nc);
  auto pp = P.mutable_unchecked<2>();
  auto ss = S.mutable_unchecked<1>();
  auto ii = I.mutable_unchecked<1>();
  auto cc = Cl.mutable_unchecked<1>();
  for (py::ssize_t i = 0; i < n; ++i) {
    pp(i, 0) = k.points[(size_t)i][0];
    pp(i, 1) = k.points[(size_t)i][1];
    ss(i) = k.score[(size_t)i];
    ii(i) = k.cell_index[(size_t)i];
  }
  for (py::ssize_t i = 0; i < nc; ++i) cc(i) = k.cell[(size_t)i];
  return py::make_tuple(P, S, I, Cl);
}

// PNEC::Solve for ONE frame pair through the overload asked for (pnec.cc:69-75, :77-124, :126-134,
// :135-208): overload 0 = (bvs1, bvs2, covs, init), 1 = (+ inliers), 2 = (+ timing), 3 = (+ inliers,
// timing).  Returns (pose 4x4, inliers or None, timing dict or None).
py::tuple solve(arr bvs1, arr bvs2, arr covs, arr init_pose, int overload, bool use_ransac, bool use_nec,
                bool use_ceres, int weighted_iterations, double regularization, int eigensolver_scheme,
                bool ransac_chained_starts) {
  const auto b1 = ToBearings(bvs1, "bvs1"), b2 = ToBearings(bvs2, "bvs2");
  const auto cv = ToCovariances(covs, "covs");
  const pnec::SE3d init = ToPose(init_pose);
  pnec::rel_pose_estimation::Options options;
  options.use_ransac_ = use_ransac;
  options.use_nec_ = use_nec;
  options.use_ceres_ = use_ceres;
  options.weighted_iterations_ = (size_t)weighted_iterations;
  options.regularization_ = regularization;
  options.eigensolver_scheme_ = eigensolver_scheme;
  options.ransac_chained_starts_ = ransac_chained_starts;
  if (overload < 0 || overload > 3) throw std::invalid_argument("overload must be 0..3");
  pnec::SE3d pose;
  std::vector<int> inliers;
  pnec::common::FrameTiming timing(7);
  // sentinels: the timed overloads only write the fields the reference writes (pnec.cc:135-208)
  timing.nec_es_ = timing.it_es_ = timing.avg_it_es_ = timing.ceres_ = -1;
  {
    py::gil_scoped_release release;
    pnec::rel_pose_estimation::PNEC solver(options);
    switch (overload) {
      case 0: pose = solver.Solve(b1, b2, cv, init); break;
      case 1: pose = solver.Solve(b1, b2, cv, init, inliers); break;
      case 2: pose = solver.Solve(b1, b2, cv, init, timing); break;
      default: pose = solver.Solve(b1, b2, cv, init, inliers, timing); break;
    }
  }
  py::object inl = py::none(), tim = py::none();
  if (overload == 1 || overload == 3) inl = py::cast(inliers);
  if (overload >= 2) {
    py::dict d;
    d["id"] = timing.id_;
    d["nec_es"] = timing.nec_es_;
    d["it_es"] = timing.it_es_;
    d["avg_it_es"] = timing.avg_it_es_;
    d["ceres"] = timing.ceres_;
    d["frame_loading"] = timing.frame_loading_;
    d["feature_creation"] = timing.feature_creation_;
    d["optimization"] = timing.OptimizationTime();
    d["total"] = timing.TotalTime();
    d["header"] = pnec::common::FrameTiming::TimingHeader();
    // the microsecond twins (this library's addition: a whole Solve is a fraction of a millisecond here)
    d["nec_es_us"] = timing.nec_es_us_;
    d["it_es_us"] = timing.it_es_us_;
    d["avg_it_es_us"] = timing.avg_it_es_us_;
    d["ceres_us"] = timing.ceres_us_;
    d["optimization_us"] = timing.OptimizationTimeUs();
    d["row_us"] = timing.TimingRowUs();
    d["header_us"] = pnec::common::FrameTiming::TimingHeaderUs();
    tim = d;
  }
  return py::make_tuple(FromPose(pose), inl, tim);
}

int add(int i, int j) { return i + j; }  // the reference module's smoke function (pypnec.cpp:34)

}  // namespace

PYBIND11_MODULE(pypnec, m) {
  m.doc() = "PNEC least-squares refinement on AMD MI355X (drop-in for tum-vision/pnec's pypnec)";
  m.def("add", &add, "A function that adds two numbers");
  m.def("pyceres", &pyceres, py::arg("host_bvs"), py::arg("target_bvs"), py::arg("host_covariances"),
        py::arg("target_covariances"), py::arg("init_pose"), py::arg("regularization"),
        "Symmetric PNEC refinement (PNECCeres::Optimize with covariances in both frames)");
  m.def("pyceresnec", &pyceresnec, py::arg("host_bvs"), py::arg("target_bvs"), py::arg("init_pose"),
        "NEC refinement (NECCeres::Optimize)");
  m.def("compose_m", &compose_m, "pnec::common::ComposeM (loop from i = 1, like the reference)");
  m.def("translation_from_m", &translation_from_m, "pnec::common::TranslationFromM");
  m.def("rotational_difference", &rotational_difference, "pnec::common::RotationalDifference (degrees)");
  m.def("translational_difference", &translational_difference, py::arg("translation_1"), py::arg("translation_2"),
        py::arg("both_directions") = true, "pnec::common::TranslationalDifference (degrees)");
  m.def("cost_function", &cost_function, "pnec::common::CostFunction (device)");
  m.def("pose_covariance", &pose_covariance, py::arg("bvs1"), py::arg("bvs2"), py::arg("covs"), py::arg("pose"),
        py::arg("regularization") = 1e-13,
        "pnec::common::PoseCovariance (addition; device): 6x6 covariance of (omega_xyz [left perturbation, rad], t_xyz "
        "[unit direction]) at `pose` -- include/pnec_hip.h pnec_hip_pose_covariance");
  m.def("pose_sensitivity", &pose_sensitivity, py::arg("bvs1"), py::arg("bvs2"), py::arg("covs"), py::arg("pose"),
        py::arg("grad_pose"), py::arg("regularization") = 1e-13,
        "pnec::rel_pose_estimation::PoseSensitivity (addition; device): (grad_bvs1, grad_bvs2, grad_covs, lambda, newton, "
        "status), the gradient of a loss of the refined pose with respect to the pair's inputs; grad_pose = (dL/d omega, "
        "dL/d t) at `pose` -- include/pnec_hip.h pnec_hip_pose_sensitivity");
  m.def("residuals", &residuals, py::arg("bvs1"), py::arg("bvs2"), py::arg("covs"), py::arg("pose"),
        py::arg("regularization") = 1e-13, py::arg("covs_host") = py::none(),
        "pnec::common::Residuals (addition; device): the whitened PNEC residual of every correspondence at `pose` -- "
        "include/pnec_hip.h pnec_hip_residuals.  covs: frame 2 (target); covs_host: frame 1, given -> the symmetric residual");
  m.def("gate_inliers", &gate_inliers, py::arg("bvs1"), py::arg("bvs2"), py::arg("covs"), py::arg("pose"),
        py::arg("gate") = 3.0, py::arg("regularization") = 1e-13, py::arg("covs_host") = py::none(),
        "pnec::common::GateInliers (addition; device): indices of the correspondences with |residual| <= gate (sigmas) "
        "at `pose`, a pose already near the truth");
  m.def("triangulate", &triangulate, py::arg("bvs1"), py::arg("bvs2"), py::arg("pose"),
        "pnec::common::Triangulate (addition; device): (points [N,3] in frame 1, depth1, depth2, front) by midpoint "
        "triangulation at `pose` as given, lengths in baselines -- include/pnec_hip.h pnec_hip_triangulate");
  m.def("orient_translation", &orient_translation, py::arg("bvs1"), py::arg("bvs2"), py::arg("pose"),
        "pnec::common::OrientTranslation (addition; device): `pose` with its translation multiplied by the cheirality "
        "vote's sign, so that the structure lies in front of both cameras");
  m.def("eight_point", &eight_point, py::arg("bvs1"), py::arg("bvs2"),
        "pnec::rel_pose_estimation::EMPoseEstimation(bvs1, bvs2, identity, EIGHTPT, ransac = false) (device): the 4x4 pose "
        "of the eight-point baseline, translation of length s0; the identity when the pair gives no pose -- "
        "include/pnec_hip.h pnec_hip_eight_point");
  m.def("undistort", &undistort, py::arg("points"), py::arg("K"), py::arg("dist"), py::arg("covs") = py::none(),
        py::arg("newton") = false, py::arg("propagate_cov") = false,
        "pnec::common::Undistort, batched (device): cv::undistortPoints with K, dist = k1 k2 p1 p2 [k3] and P = K for "
        "points [N,2] and optionally their covariances [N,3] (xx, xy, yy); returns (points, covs or None, status uint8 [N]). "
        "newton polishes the five fixed-point steps, propagate_cov carries the covariances through the map (neither is in the "
        "reference).  As in the reference, dist[0] == 0 returns the input -- include/pnec_hip.h pnec_hip_undistort_keypoints");
  m.def("compose_trajectory", &compose_trajectory, py::arg("relative_poses"), py::arg("correction") = py::none(),
        "pnec::odometry::ComposeTrajectory (device): the relative poses [N,4,4] of one run chained into absolute poses, the "
        "first being a pose itself, with `correction` (4x4) as the left factor -- evaluate_run.py:118-129.  Returns (poses "
        "[N,4,4], valid uint8 [N]); a relative pose that is not finite carries the pose before it and gets valid 0 -- "
        "include/pnec_hip.h pnec_hip_trajectory_compose");
  m.def("trajectory_metrics", &trajectory_metrics, py::arg("estimated"), py::arg("ground_truth"),
        "pnec::odometry::TrajectoryMetrics (device): RPE_1, RPE_n, L1RPE_1, L1RPE_n, r_t in radians of the matched absolute "
        "poses estimated / ground_truth [N,4,4], with rmse_d, l1_d, angle1, rt1 [N], as a dict; an exact estimate scores 0 "
        "where the reference gives NaN -- include/pnec_hip.h pnec_hip_trajectory_metrics");
  m.def("link_tracks", &link_tracks, py::arg("prev_ids"), py::arg("cur_ids"),
        "pnec::features::LinkTracks (device): for every track id of cur_ids the row of the same id in prev_ids (strictly "
        "ascending), -1 where there is none; int32 [len(cur_ids)] -- include/pnec_hip.h pnec_hip_tracks_link");
  m.def("advance_trajectory", &advance_trajectory, py::arg("s"), py::arg("q"), py::arg("p"), py::arg("rel_q"),
        py::arg("rel_t"), py::arg("count") = py::none(), py::arg("min_count") = 0, py::arg("scale3") = py::none(),
        py::arg("n_used") = py::none(), py::arg("min_used") = 1,
        "pnec::odometry::AdvanceTrajectory (device): one frame's step of the running scale s [n] and pose q [n,4] xyzw, "
        "p [n,3] by the relative pose rel_q, rel_t and the baseline ratio's median scale3[:, 1]; returns (s, q, p, status "
        "int32 [n]: 0 measured, 1 held, 2 started, 3 absent) -- include/pnec_hip.h pnec_hip_trajectory_advance");
  m.def("five_point", &five_point, py::arg("bvs1"), py::arg("bvs2"),
        "pnec::rel_pose_estimation::MinimalEMPoseEstimation(bvs1, bvs2, identity, NISTER) (device): the 4x4 pose of "
        "Nister's five-point solver, translation of length s0; the identity when the pair gives no pose -- "
        "include/pnec_hip.h pnec_hip_essential_minimal");
  m.def("seven_point", &seven_point, py::arg("bvs1"), py::arg("bvs2"),
        "pnec::rel_pose_estimation::MinimalEMPoseEstimation(bvs1, bvs2, identity, SEVENPT) (device): the same of the "
        "seven-point solver");
  m.def("essential_ransac", &essential_ransac, py::arg("bvs1"), py::arg("bvs2"), py::arg("algorithm"),
        py::arg("max_iterations") = 5000, py::arg("threshold") = 1e-6, py::arg("seed") = 1,
        "pnec::rel_pose_estimation::RansacEMPoseEstimation(bvs1, bvs2, identity, algorithm, ...) (device): RANSAC around "
        "the \"nister\", \"sevenpt\" or \"eightpt\" solver; returns (the 4x4 pose, translation of length s0, and the indices "
        "of its inliers); the identity and no inliers when the pair gives no model -- include/pnec_hip.h "
        "pnec_hip_essential_ransac");
  m.def("relative_scale", &relative_scale, py::arg("bvs_prev1"), py::arg("bvs_prev2"), py::arg("pose_prev"),
        py::arg("bvs1"), py::arg("bvs2"), py::arg("pose"), py::arg("link"), py::arg("min_parallax") = 0.0,
        "pnec::common::RelativeScale (addition; device): (scale, q25, q75, n_used, ratio [N]) -- the baseline of `pose` in "
        "units of the baseline of `pose_prev` from the tracks `link` ties to the previous pair -- include/pnec_hip.h "
        "pnec_hip_relative_scale");
  m.def("image_pyramid", &image_pyramid, py::arg("image"), py::arg("levels"),
        "pnec::features::ImagePyramid (addition; device): the levels of one image's pyramid, level 0 first -- "
        "include/pnec_hip.h pnec_hip_image_pyramid_level");
  m.def("patch_track", &patch_track, py::arg("image1"), py::arg("image2"), py::arg("points"), py::arg("levels") = 5,
        py::arg("max_iterations") = 40, py::arg("max_recovered_dist2") = 0.04, py::arg("backward") = true,
        py::arg("scaling") = 10.0, py::arg("shift_x") = 0.0, py::arg("shift_y") = 0.0,
        "pnec::features::TrackPatches (addition; device): (pts [N,2], angle [N], cov [N,3], dist2 [N], status [N], "
        "lost_level [N]) of the Pattern52 patches at `points` of image1 tracked into image2 and back, in double -- "
        "include/pnec_hip.h pnec_hip_patch_track");
  m.def("retain_tracks", &retain_tracks, py::arg("id"), py::arg("tmpl_image"), py::arg("tmpl_pts"), py::arg("age"),
        py::arg("pts"), py::arg("cov"), py::arg("trk_pts"), py::arg("trk_angle"), py::arg("trk_cov"), py::arg("trk_status"),
        py::arg("max_age") = 0,
        "(id, tmpl_image, tmpl_pts, age, pts, angle, cov, prev_pts, prev_cov, src) of one image's tracks that came back OK "
        "(and young enough), compacted in order; include/pnec_hip.h pnec_hip_tracks_retain");
  m.def("append_tracks", &append_tracks, py::arg("tracks"), py::arg("det_pts"), py::arg("det_cov"), py::arg("tmpl_image"),
        py::arg("capacity"), py::arg("next_id"),
        "((id, tmpl_image, tmpl_pts, age, pts, angle, cov), next_id, dropped): one image's tracks refilled with detections "
        "up to `capacity`; include/pnec_hip.h pnec_hip_tracks_append");
  m.def("detect_keypoints", &detect_keypoints, py::arg("image"), py::arg("grid") = 30, py::arg("points_per_cell") = 1,
        py::arg("min_threshold") = 5, py::arg("edge") = 19, py::arg("current") = py::none(),
        "pnec::features::DetectKeypoints (addition; device): (pts [N,2], score [N], cell_index [N], cell [n_cells]) -- the "
        "grid FAST-9 corners of one uint8 / uint16 image, skipping the cells the `current` points [n,2] occupy -- "
        "include/pnec_hip.h pnec_hip_detect_keypoints");
  m.def("patch_covariance", &patch_covariance, py::arg("image"), py::arg("points"), py::arg("scaling") = 10.0,
        "pnec::features::PatchCovariances (addition; device): (cov [N,3] as xx, xy, yy, status [N]) -- the 2x2 image "
        "covariance of the keypoints `points` [N,2] of one uint8 / uint16 / float32 image from their Pattern52 patches, in "
        "double; no tracking -- include/pnec_hip.h pnec_hip_patch_covariance");
  m.def("solve", &solve, py::arg("bvs1"), py::arg("bvs2"), py::arg("covs"), py::arg("init_pose"),
        py::arg("overload") = 1, py::arg("use_ransac") = true, py::arg("use_nec") = false,
        py::arg("use_ceres") = true, py::arg("weighted_iterations") = 10, py::arg("regularization") = 1e-13,
        py::arg("eigensolver_scheme") = 2, py::arg("ransac_chained_starts") = false,
        "PNEC::Solve for one frame pair through one of its four overloads (eigensolver_scheme: which iteration stands in "
        "for opengv's eigenvalue minimisation; ransac_chained_starts: PNEC_HIP_RANSAC_CHAINED_STARTS -- include/pnec_hip.h)");
  m.def("solve_batch", &solve_batch, py::arg("bvs1"), py::arg("bvs2"), py::arg("covs"), py::arg("init_poses"),
        py::arg("use_ransac") = true, py::arg("use_nec") = false, py::arg("use_ceres") = true,
        py::arg("weighted_iterations") = 10, py::arg("regularization") = 1e-13, py::arg("devices") = std::vector<int>{},
        py::arg("eigensolver_scheme") = 2,
        "PNEC::Solve for a list of frame pairs, every stage one device launch over the batch (addition); devices: the "
        "GPUs to shard the pairs over from this process (empty: the default device)");
  m.def("ceres_solver_batch", &ceres_solver_batch, py::arg("bvs1"), py::arg("bvs2"), py::arg("covs"),
        py::arg("init_poses"), py::arg("regularization") = 1e-13, py::arg("devices") = std::vector<int>{},
        "PNEC::CeresSolver for a list of frame pairs in one device launch (addition); devices: the GPUs to shard the pairs "
        "over from this process (empty: the default device)");
}
