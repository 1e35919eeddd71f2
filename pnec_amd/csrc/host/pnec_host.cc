// pnec_host.cc -- implementation of the host facade over the C ABI.  See pnec_host.h.
#include "pnec_host.h"

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <limits>

namespace pnec {
namespace {

void Check(int rc) {
  if (rc != 0) throw HipError(rc, std::string("libpnec_hip: ") + pnec_hip_last_error());
}

// RAII over pnec_hip_problem
struct Problem {
  pnec_hip_problem *p = nullptr;
  Problem(int device, int mode, const std::vector<int64_t> &offsets) {
    Check(pnec_hip_problem_create(device, mode, (int64_t)offsets.size() - 1, offsets.data(), &p));
  }
  ~Problem() { pnec_hip_problem_destroy(p); }
  Problem(const Problem &) = delete;
  Problem &operator=(const Problem &) = delete;
};

Vector3d TranslationFromAngles(double theta, double phi) {
  return Vector3d(std::sin(theta) * std::cos(phi), std::sin(theta) * std::sin(phi), std::cos(theta));
}

// The per-thread streaming handle of a device (pnec_hip_stream: pinned staging + one HIP stream, created
// once): what makes a single Optimize() call cost one memcpy + one kernel launch instead of a batch
// object's create / fill / solve / destroy.  Grown (re-created) when a pair exceeds its capacity.
struct ThreadStream {
  pnec_hip_stream *s = nullptr;
  int device = -1;
  int32_t max_corr = 0;
  ~ThreadStream() { pnec_hip_stream_destroy(s); }
  pnec_hip_stream *Get(int dev, int64_t n) {
    if (!s || dev != device || n > max_corr) {
      pnec_hip_stream_destroy(s);
      s = nullptr;
      int32_t cap = 4096;
      while (cap < n) cap *= 2;
      Check(pnec_hip_stream_create(dev, cap, 1, 4, nullptr, &s));
      device = dev;
      max_corr = cap;
    }
    return s;
  }
};
thread_local ThreadStream g_stream;

// One solve through the ABI: host arrays in the reference's layout in, pose + summary out.
void SolveOne(int mode, const optimization::SolverOptions &options, const std::vector<Vector3d> &b1,
              const std::vector<Vector3d> &b2, const std::vector<Matrix3d> *covs,
              const std::vector<Matrix3d> *covs_host, double reg, Quaterniond &q, double &theta,
              double &phi, optimization::Summary &summary) {
  if (b1.size() != b2.size()) throw std::invalid_argument("bvs_1 and bvs_2 differ in size");
  if (covs && covs->size() != b1.size()) throw std::invalid_argument("covs and bvs differ in size");
  if (covs_host && covs_host->size() != b1.size()) throw std::invalid_argument("covs_1 and bvs differ in size");
  const int64_t offsets[2] = {0, (int64_t)b1.size()};
  pnec_hip_stream *stream = g_stream.Get(options.device, offsets[1]);
  const Vector3d t0 = TranslationFromAngles(theta, phi);
  const pnec_hip_options o = options.ToHip();
  int64_t ticket = 0;
  Check(pnec_hip_stream_submit(stream, mode, 1, offsets, b1.empty() ? nullptr : b1[0].data(),
                               b2.empty() ? nullptr : b2[0].data(),
                               covs && !covs->empty() ? (*covs)[0].data() : nullptr,
                               covs_host && !covs_host->empty() ? (*covs_host)[0].data() : nullptr, q.coeffs(),
                               t0.data(), reg, &o, &ticket));
  double out_q[4], out_t[3], cost = 0.0;
  int32_t it = 0, st = 0;
  Check(pnec_hip_stream_wait(stream, ticket, out_q, out_t, &cost, &it, &st));
  q = Quaterniond(out_q[3], out_q[0], out_q[1], out_q[2]);
  common::AnglesFromVec(Vector3d(out_t[0], out_t[1], out_t[2]), theta, phi);
  summary.final_cost = cost;
  summary.iterations = it;
  summary.termination = st;
}

}  // namespace

// ------------------------------------------------------------------------------------ common
namespace common {

Matrix3d SkewFromVector(const Vector3d &v) {
  Matrix3d S;
  S(0, 1) = -v[2]; S(0, 2) = v[1];
  S(1, 0) = v[2];  S(1, 2) = -v[0];
  S(2, 0) = -v[1]; S(2, 1) = v[0];
  return S;
}

void AnglesFromVec(const Vector3d &vector, double &theta, double &phi) {
  const double n = vector.norm();
  if (n == 0.0) {
    theta = 0.0;
    phi = 0.0;
    return;
  }
  theta = std::acos(vector[2] / n);
  phi = (std::fabs(theta) < 1e-10) ? 0.0 : std::atan2(vector[1] / n, vector[0] / n);
}

double RotationalDifference(const Matrix3d &rotation_1, const Matrix3d &rotation_2) {
  const Quaterniond q = Quaterniond(rotation_1.transpose() * rotation_2).normalized();
  const double n = std::sqrt(q.x() * q.x() + q.y() * q.y() + q.z() * q.z());
  const double theta = (q.w() < 0.0) ? 2.0 * std::atan2(-n, -q.w()) : 2.0 * std::atan2(n, q.w());
  return std::fabs(theta) * 180.0 / M_PI;
}

double TranslationalDifference(const Vector3d &translation_1, const Vector3d &translation_2,
                               bool both_directions) {
  const double n1 = translation_1.norm(), n2 = translation_2.norm();
  if (n1 < 1e-10) return 90.0;  // the reference tests translation_1 twice (common.cc:220)
  const double c = translation_1.dot(translation_2) / (n1 * n2);
  double error = std::acos(c);
  if (both_directions) error = std::min(error, std::acos(-c));
  return error * 180.0 / M_PI;
}

Matrix3d ComposeM(const bearingVectors_t &bvs_1, const bearingVectors_t &bvs_2, const Matrix3d &rotation) {
  Matrix3d M;
  for (size_t i = 1; i < bvs_1.size(); ++i) {  // sic: the reference's loop starts at 1
    const Vector3d n = bvs_1[i].cross(rotation * bvs_2[i]);
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) M(r, c) += n[r] * n[c];
  }
  return M;
}

// unit eigenvector of the smallest eigenvalue (cyclic Jacobi); largest-magnitude component positive
Vector3d TranslationFromM(const Matrix3d &M) {
  double A[3][3], V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) A[r][c] = 0.5 * (M(r, c) + M(c, r));
  for (int sweep = 0; sweep < 12; ++sweep) {
    const double off = A[0][1] * A[0][1] + A[0][2] * A[0][2] + A[1][2] * A[1][2];
    const double dg = A[0][0] * A[0][0] + A[1][1] * A[1][1] + A[2][2] * A[2][2];
    if (off <= 1e-34 * dg || off == 0.0) break;
    const int P[3] = {0, 0, 1}, Q[3] = {1, 2, 2};
    for (int k = 0; k < 3; ++k) {
      const int p = P[k], q = Q[k];
      if (A[p][q] == 0.0) continue;
      const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
      const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
      const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
      for (int r = 0; r < 3; ++r) {
        const double arp = A[r][p], arq = A[r][q];
        A[r][p] = c * arp - s * arq;
        A[r][q] = s * arp + c * arq;
      }
      for (int r = 0; r < 3; ++r) {
        const double apr = A[p][r], aqr = A[q][r];
        A[p][r] = c * apr - s * aqr;
        A[q][r] = s * apr + c * aqr;
      }
      for (int r = 0; r < 3; ++r) {
        const double vrp = V[r][p], vrq = V[r][q];
        V[r][p] = c * vrp - s * vrq;
        V[r][q] = s * vrp + c * vrq;
      }
    }
  }
  int j = 0;
  if (A[1][1] < A[j][j]) j = 1;
  if (A[2][2] < A[j][j]) j = 2;
  Vector3d v(V[0][j], V[1][j], V[2][j]);
  int big = 0;
  for (int r = 1; r < 3; ++r)
    if (std::fabs(v[r]) > std::fabs(v[big])) big = r;
  if (v[big] < 0.0) v = -v;
  return v.normalized();
}

double Weight(const Vector3d &f1, const Vector3d &f2, const Vector3d &translation, const Matrix3d &rotation,
              const Matrix3d &covariance, double regularization, bool host_frame) {
  const Vector3d v = host_frame ? translation.cross(rotation * f2) : rotation.transpose() * translation.cross(f1);
  const double q = v.dot(covariance * v);
  return host_frame ? 1.0 / q : 1.0 / (q + regularization);
}

Vector3d Unproject(const double img_pt[2], const Matrix3d &K_inv) {
  return (K_inv * Vector3d(img_pt[0], img_pt[1], 1.0)).normalized();
}

std::vector<Matrix3d> UnscentedTransform(const std::vector<Vector3d> &mus, const std::vector<Matrix3d> &covs,
                                         const Matrix3d &K_inv, double kappa, CameraModel camera_model) {
  if (mus.size() != covs.size()) return covs;  // the reference warns and returns the input (common.cc:532-537)
  std::vector<Matrix3d> out(mus.size());
  if (!mus.empty())
    Check(pnec_hip_unscented_transform((int64_t)mus.size(), mus[0].data(), covs[0].data(), K_inv.data(), kappa,
                                       camera_model == Pinhole ? 1 : 0, nullptr, out[0].data(),
                                       PNEC_HIP_MEM_HOST, optimization::SolverOptions().device, nullptr));
  return out;
}

Matrix3d UnscentedTransform(const Vector3d &mu, const Matrix3d &cov, const Matrix3d &K_inv, double kappa,
                            CameraModel camera_model) {
  return UnscentedTransform(std::vector<Vector3d>{mu}, std::vector<Matrix3d>{cov}, K_inv, kappa, camera_model)[0];
}

std::array<double, 9> UndistortCamera(const Matrix3d &K, const std::vector<double> &dist_coef) {
  if (dist_coef.size() != 4 && dist_coef.size() != 5)
    throw std::invalid_argument("Undistort: dist_coef takes 4 or 5 coefficients: k1 k2 p1 p2 [k3]");
  if (K(0, 1) != 0.0 || K(1, 0) != 0.0 || K(2, 0) != 0.0 || K(2, 1) != 0.0 || K(2, 2) != 1.0)
    throw std::invalid_argument("Undistort: K must be upper triangular with zero skew and last row (0, 0, 1)");
  return {K(0, 0), K(1, 1), K(0, 2), K(1, 2), dist_coef[0], dist_coef[1], dist_coef[2], dist_coef[3],
          dist_coef.size() == 5 ? dist_coef[4] : 0.0};
}

std::vector<uint8_t> Undistort(std::vector<Vector2d> &points, std::vector<Covariance2d> *covs, const Matrix3d &K,
                               const std::vector<double> &dist_coef, const UndistortOptions &options) {
  const std::array<double, 9> camera = UndistortCamera(K, dist_coef);
  if (covs && covs->size() != points.size()) throw std::invalid_argument("Undistort: points and covs differ in size");
  std::vector<uint8_t> status(points.size(), (uint8_t)PNEC_HIP_UNDISTORT_OK);
  if (dist_coef[0] == 0.0 || points.empty()) return status;  // (the reference's rule, common.cc:74-76)
  const uint32_t flags = (options.newton ? PNEC_HIP_UNDISTORT_NEWTON : 0u) |
                         (options.propagate_cov ? PNEC_HIP_UNDISTORT_PROPAGATE_COV : 0u);
  double *pts = points[0].data(), *cov = covs ? (*covs)[0].data() : nullptr;
  // (frame 1's slots: in place, an output being its own input)
  Check(pnec_hip_undistort_keypoints(optimization::SolverOptions().device, (int64_t)points.size(), pts, nullptr, nullptr, cov,
                                     camera.data(), options.fixed_iterations, options.newton_iterations, flags, pts, nullptr,
                                     nullptr, cov, status.data(), nullptr, PNEC_HIP_MEM_HOST, nullptr));
  return status;
}

Vector2d Undistort(const Vector2d &point, const Matrix3d &K, const std::vector<double> &dist_coef) {
  std::vector<Vector2d> points{point};
  Undistort(points, nullptr, K, dist_coef);
  return points[0];
}

double CostFunction(const bearingVectors_t &bvs_1, const bearingVectors_t &bvs_2,
                    const std::vector<Matrix3d> &covs, const SE3d &camera_pose) {
  if (bvs_1.size() != bvs_2.size() || bvs_1.size() != covs.size())
    throw std::invalid_argument("bvs_1, bvs_2 and covs differ in size");
  // empty input: the reference divides 0.0 by size() == 0 (common.cc:258) -> NaN
  if (bvs_1.empty()) return std::nan("");
  const std::vector<int64_t> offsets = {0, (int64_t)bvs_1.size()};
  Problem prob(optimization::SolverOptions().device, PNEC_HIP_MODE_TARGET, offsets);
  Check(pnec_hip_problem_fill(prob.p, 0, 1, bvs_1[0].data(), bvs_2[0].data(), covs[0].data(), nullptr,
                              PNEC_HIP_MEM_HOST, nullptr));
  const Quaterniond q(camera_pose.rotationMatrix());
  double out = 0.0;
  Check(pnec_hip_cost_function(prob.p, q.coeffs(), camera_pose.translation().data(), &out,
                               PNEC_HIP_MEM_HOST, nullptr));
  return out;
}

namespace {
Matrix6d PoseCovarianceImpl(int mode, const bearingVectors_t &bvs_1, const bearingVectors_t &bvs_2,
                            const std::vector<Matrix3d> &covs, const std::vector<Matrix3d> *covs_host,
                            const SE3d &camera_pose, double regularization) {
  if (bvs_1.size() != bvs_2.size() || bvs_1.size() != covs.size() || (covs_host && covs_host->size() != covs.size()))
    throw std::invalid_argument("bvs_1, bvs_2 and covs differ in size");
  Matrix6d out;
  if (bvs_1.empty()) {   // no information at all
    for (double &v : out.m) v = std::nan("");
    return out;
  }
  const std::vector<int64_t> offsets = {0, (int64_t)bvs_1.size()};
  Problem prob(optimization::SolverOptions().device, mode, offsets);
  Check(pnec_hip_problem_fill(prob.p, 0, 1, bvs_1[0].data(), bvs_2[0].data(), covs[0].data(),
                              covs_host ? (*covs_host)[0].data() : nullptr, PNEC_HIP_MEM_HOST, nullptr));
  const Quaterniond q(camera_pose.rotationMatrix());
  // (symmetric: the ABI's row-major 6x6 is the column-major one)
  Check(pnec_hip_pose_covariance(prob.p, q.coeffs(), camera_pose.translation().data(), 1, regularization, nullptr,
                                 out.data(), nullptr, nullptr, nullptr, PNEC_HIP_MEM_HOST, nullptr));
  return out;
}
}  // namespace

Matrix6d PoseCovariance(const bearingVectors_t &bvs_1, const bearingVectors_t &bvs_2, const std::vector<Matrix3d> &covs,
                        const SE3d &camera_pose, double regularization) {
  return PoseCovarianceImpl(PNEC_HIP_MODE_TARGET, bvs_1, bvs_2, covs, nullptr, camera_pose, regularization);
}
Matrix6d PoseCovariance(const bearingVectors_t &bvs_1, const bearingVectors_t &bvs_2, const std::vector<Matrix3d> &covs_1,
                        const std::vector<Matrix3d> &covs_2, const SE3d &camera_pose, double regularization) {
  return PoseCovarianceImpl(PNEC_HIP_MODE_SYM, bvs_1, bvs_2, covs_2, &covs_1, camera_pose, regularization);
}

namespace {
// pnec_hip_residuals for one pair; the residuals and / or the gate's mask (either may be NULL)
void ResidualsImpl(int mode, const bearingVectors_t &bvs_1, const bearingVectors_t &bvs_2,
                   const std::vector<Matrix3d> &covs, const std::vector<Matrix3d> *covs_host, const SE3d &camera_pose,
                   double gate, double regularization, std::vector<double> *residuals, std::vector<uint8_t> *mask) {
  if (bvs_1.size() != bvs_2.size() || bvs_1.size() != covs.size() || (covs_host && covs_host->size() != covs.size()))
    throw std::invalid_argument("bvs_1, bvs_2 and covs differ in size");
  if (residuals) residuals->assign(bvs_1.size(), 0.0);
  if (mask) mask->assign(bvs_1.size(), 0);
  if (bvs_1.empty()) return;
  const std::vector<int64_t> offsets = {0, (int64_t)bvs_1.size()};
  Problem prob(optimization::SolverOptions().device, mode, offsets);
  Check(pnec_hip_problem_fill(prob.p, 0, 1, bvs_1[0].data(), bvs_2[0].data(), covs[0].data(),
                              covs_host ? (*covs_host)[0].data() : nullptr, PNEC_HIP_MEM_HOST, nullptr));
  const Quaterniond q(camera_pose.rotationMatrix());
  Check(pnec_hip_residuals(prob.p, q.coeffs(), camera_pose.translation().data(), 1, regularization, gate,
                           residuals ? residuals->data() : nullptr, nullptr, mask ? mask->data() : nullptr, nullptr,
                           nullptr, nullptr, nullptr, PNEC_HIP_MEM_HOST, nullptr));
}
std::vector<int> MaskToIndices(const std::vector<uint8_t> &mask) {
  std::vector<int> out;
  for (size_t i = 0; i < mask.size(); ++i)
    if (mask[i]) out.push_back((int)i);
  return out;
}
}  // namespace

std::vector<double> Residuals(const bearingVectors_t &bvs_1, const bearingVectors_t &bvs_2,
                              const std::vector<Matrix3d> &covs, const SE3d &camera_pose, double regularization) {
  std::vector<double> r;
  ResidualsImpl(PNEC_HIP_MODE_TARGET, bvs_1, bvs_2, covs, nullptr, camera_pose, 0.0, regularization, &r, nullptr);
  return r;
}
std::vector<double> Residuals(const bearingVectors_t &bvs_1, const bearingVectors_t &bvs_2,
                              const std::vector<Matrix3d> &covs_1, const std::vector<Matrix3d> &covs_2,
                              const SE3d &camera_pose, double regularization) {
  std::vector<double> r;
  ResidualsImpl(PNEC_HIP_MODE_SYM, bvs_1, bvs_2, covs_2, &covs_1, camera_pose, 0.0, regularization, &r, nullptr);
  return r;
}
std::vector<int> GateInliers(const bearingVectors_t &bvs_1, const bearingVectors_t &bvs_2,
                             const std::vector<Matrix3d> &covs, const SE3d &camera_pose, double gate,
                             double regularization) {
  std::vector<uint8_t> m;
  ResidualsImpl(PNEC_HIP_MODE_TARGET, bvs_1, bvs_2, covs, nullptr, camera_pose, gate, regularization, nullptr, &m);
  return MaskToIndices(m);
}
std::vector<int> GateInliers(const bearingVectors_t &bvs_1, const bearingVectors_t &bvs_2,
                             const std::vector<Matrix3d> &covs_1, const std::vector<Matrix3d> &covs_2,
                             const SE3d &camera_pose, double gate, double regularization) {
  std::vector<uint8_t> m;
  ResidualsImpl(PNEC_HIP_MODE_SYM, bvs_1, bvs_2, covs_2, &covs_1, camera_pose, gate, regularization, nullptr, &m);
  return MaskToIndices(m);
}

namespace {
// pnec_hip_triangulate for one pair (a NEC-mode batch: bearings only) at the pose as given; any output may be NULL
void TriangulateImpl(const bearingVectors_t &bvs_1, const bearingVectors_t &bvs_2, const SE3d &camera_pose,
                     double *points, double *depths_1, double *depths_2, uint8_t *front, int32_t *sign) {
  if (bvs_1.size() != bvs_2.size()) throw std::invalid_argument("bvs_1 and bvs_2 differ in size");
  if (sign) *sign = 1;
  if (bvs_1.empty()) return;
  const std::vector<int64_t> offsets = {0, (int64_t)bvs_1.size()};
  Problem prob(optimization::SolverOptions().device, PNEC_HIP_MODE_NEC, offsets);
  Check(pnec_hip_problem_fill(prob.p, 0, 1, bvs_1[0].data(), bvs_2[0].data(), nullptr, nullptr, PNEC_HIP_MEM_HOST,
                              nullptr));
  const Quaterniond q(camera_pose.rotationMatrix());
  Check(pnec_hip_triangulate(prob.p, q.coeffs(), camera_pose.translation().data(), 1, 0, points, depths_1, depths_2,
                             nullptr, nullptr, front, nullptr, nullptr, sign, nullptr, nullptr, PNEC_HIP_MEM_HOST,
                             nullptr));
}
}  // namespace

std::vector<Vector3d> Triangulate(const bearingVectors_t &bvs_1, const bearingVectors_t &bvs_2, const SE3d &camera_pose,
                                  std::vector<double> *depths_1, std::vector<double> *depths_2,
                                  std::vector<uint8_t> *front) {
  const size_t n = bvs_1.size();
  std::vector<Vector3d> points(n);
  if (depths_1) depths_1->assign(n, 0.0);
  if (depths_2) depths_2->assign(n, 0.0);
  if (front) front->assign(n, 0);
  static_assert(sizeof(Vector3d) == 3 * sizeof(double), "Vector3d is three packed doubles");
  TriangulateImpl(bvs_1, bvs_2, camera_pose, n ? points[0].data() : nullptr, depths_1 ? depths_1->data() : nullptr,
                  depths_2 ? depths_2->data() : nullptr, front ? front->data() : nullptr, nullptr);
  return points;
}

SE3d OrientTranslation(const bearingVectors_t &bvs_1, const bearingVectors_t &bvs_2, const SE3d &camera_pose) {
  int32_t sign = 1;
  TriangulateImpl(bvs_1, bvs_2, camera_pose, nullptr, nullptr, nullptr, nullptr, &sign);
  return SE3d(camera_pose.rotationMatrix(), camera_pose.translation() * (double)sign);
}

double RelativeScale(const bearingVectors_t &bvs_prev_1, const bearingVectors_t &bvs_prev_2, const SE3d &pose_prev,
                     const bearingVectors_t &bvs_1, const bearingVectors_t &bvs_2, const SE3d &camera_pose,
                     const std::vector<int> &link, double min_parallax, double *q25, double *q75, int *n_used,
                     std::vector<double> *ratios) {
  if (bvs_prev_1.size() != bvs_prev_2.size()) throw std::invalid_argument("bvs_prev_1 and bvs_prev_2 differ in size");
  if (bvs_1.size() != bvs_2.size()) throw std::invalid_argument("bvs_1 and bvs_2 differ in size");
  if (link.size() != bvs_1.size()) throw std::invalid_argument("link must have one entry per current correspondence");
  const double nan = std::nan("");
  const size_t n = bvs_1.size();
  double scale[3] = {nan, nan, nan};
  int32_t used = 0;
  if (ratios) ratios->assign(n, nan);
  if (n > 0 && !bvs_prev_1.empty()) {
    const int device = optimization::SolverOptions().device;
    Problem prev(device, PNEC_HIP_MODE_NEC, {0, (int64_t)bvs_prev_1.size()});
    Problem cur(device, PNEC_HIP_MODE_NEC, {0, (int64_t)n});
    Check(pnec_hip_problem_fill(prev.p, 0, 1, bvs_prev_1[0].data(), bvs_prev_2[0].data(), nullptr, nullptr,
                                PNEC_HIP_MEM_HOST, nullptr));
    Check(pnec_hip_problem_fill(cur.p, 0, 1, bvs_1[0].data(), bvs_2[0].data(), nullptr, nullptr, PNEC_HIP_MEM_HOST,
                                nullptr));
    const Quaterniond qc(camera_pose.rotationMatrix()), qp(pose_prev.rotationMatrix());
    const int64_t prev_pair = 0;
    const std::vector<int32_t> link32(link.begin(), link.end());
    Check(pnec_hip_relative_scale(cur.p, prev.p, &prev_pair, link32.data(), qc.coeffs(),
                                  camera_pose.translation().data(), qp.coeffs(), pose_prev.translation().data(),
                                  min_parallax, ratios ? ratios->data() : nullptr, nullptr, scale, nullptr, &used,
                                  PNEC_HIP_MEM_HOST, nullptr));
  }
  if (q25) *q25 = scale[0];
  if (q75) *q75 = scale[2];
  if (n_used) *n_used = (int)used;
  return scale[1];
}

std::ostream &operator<<(std::ostream &os, const FrameTiming &ft) {
  const long fields[] = {(long)ft.id_,    ft.frame_loading_, ft.feature_creation_,      ft.nec_es_,
                         ft.it_es_,       ft.avg_it_es_,     ft.ceres_,
                         (long)ft.OptimizationTime(),        (long)ft.TotalTime()};
  const char *sep = "";
  for (long v : fields) {
    os << sep << v;
    sep = " ";
  }
  return os;
}

std::string FrameTiming::TimingRowUs() const {
  char buf[192];
  std::snprintf(buf, sizeof(buf), "%d %.1f %.1f %.1f %.1f %.1f", id_, nec_es_us_, it_es_us_, avg_it_es_us_, ceres_us_,
                OptimizationTimeUs());
  return buf;
}

std::ostream &operator<<(std::ostream &os, const Timing &timing) {
  os << FrameTiming::TimingHeader() << std::endl;
  for (const FrameTiming &ft : timing.frame_timings_) os << ft << std::endl;
  return os;
}

bool Timing::Save(const std::string &path) const {
  std::ofstream out(path, std::ios_base::trunc);
  if (!out) return false;
  out << *this;
  return (bool)out;
}

}  // namespace common

namespace features {

const std::vector<std::array<double, 2>> &Pattern52() {
  static const std::vector<std::array<double, 2>> pattern = [] {
    std::vector<std::array<double, 2>> p;
    const int half_width[8] = {3, 5, 7, 7, 7, 7, 5, 3};
    for (int row = 0; row < 8; ++row)
      for (int x = -half_width[row]; x <= half_width[row]; x += 2) p.push_back({0.5 * x, 0.5 * (7 - 2 * row)});
    return p;
  }();
  return pattern;
}

std::vector<std::array<double, 3>> PatchCovariances(const void *image, pnec_hip_pixel_type pixel_type, int height,
                                                    int width, int64_t pitch,
                                                    const std::vector<std::array<double, 2>> &points, double scaling,
                                                    const std::vector<double> *angles, std::vector<int> *status,
                                                    const std::vector<std::array<double, 2>> *pattern) {
  if (angles && angles->size() != points.size()) throw std::invalid_argument("angles must have one entry per keypoint");
  const std::vector<std::array<double, 2>> &pat = pattern ? *pattern : Pattern52();
  const size_t n = points.size();
  const double nan = std::nan("");
  std::vector<std::array<double, 3>> cov(n, std::array<double, 3>{nan, nan, nan});
  std::vector<int32_t> st(n, PNEC_HIP_PATCH_EMPTY);
  const int64_t offsets[2] = {0, (int64_t)n};
  static_assert(sizeof(std::array<double, 2>) == 2 * sizeof(double) && sizeof(std::array<double, 3>) == 3 * sizeof(double),
                "std::array<double, N> is N packed doubles");
  if (n > 0)
    Check(pnec_hip_patch_covariance(image, (int)pixel_type, 1, height, width, pitch > 0 ? pitch : width, offsets,
                                    (int64_t)n, points[0].data(), pat.empty() ? nullptr : pat[0].data(), (int32_t)pat.size(),
                                    scaling, angles ? angles->data() : nullptr, cov[0].data(), nullptr, nullptr, nullptr,
                                    st.data(), PNEC_HIP_MEM_HOST, optimization::SolverOptions().device, nullptr));
  if (status) status->assign(st.begin(), st.end());
  return cov;
}

static size_t PixelBytes(pnec_hip_pixel_type t) { return t == PNEC_HIP_PIXEL_U8 ? 1 : (t == PNEC_HIP_PIXEL_U16 ? 2 : 4); }

Pyramid ImagePyramid(const void *image, pnec_hip_pixel_type pixel_type, int height, int width, int64_t pitch, int levels) {
  if (!image) throw std::invalid_argument("image is NULL");
  if (levels < 1 || levels > PNEC_HIP_TRACK_MAX_LEVELS) throw std::invalid_argument("levels must be 1 .. 8");
  if (pixel_type != PNEC_HIP_PIXEL_U8 && pixel_type != PNEC_HIP_PIXEL_U16 && pixel_type != PNEC_HIP_PIXEL_F32)
    throw std::invalid_argument("unknown pixel type");
  if (height < 1 || width < 1 || (pitch > 0 && pitch < width)) throw std::invalid_argument("bad image shape");
  const size_t es = PixelBytes(pixel_type);
  const int64_t in_pitch = pitch > 0 ? pitch : width;
  Pyramid p;
  p.pixel_type = pixel_type;
  p.height = height;
  p.width = width;
  p.levels.resize((size_t)levels);
  p.levels[0].resize((size_t)height * (size_t)width * es);
  for (int y = 0; y < height; ++y)
    std::memcpy(p.levels[0].data() + (size_t)y * (size_t)width * es,
                static_cast<const unsigned char *>(image) + (size_t)y * (size_t)in_pitch * es, (size_t)width * es);
  for (int l = 1; l < levels; ++l) {
    const int h = height >> (l - 1), w = width >> (l - 1);
    p.levels[(size_t)l].resize((size_t)(h / 2) * (size_t)(w / 2) * es);
    Check(pnec_hip_image_pyramid_level(p.levels[(size_t)l - 1].data(), p.levels[(size_t)l].data(), (int)pixel_type, 1, h, w,
                                       w, w / 2, PNEC_HIP_MEM_HOST, optimization::SolverOptions().device, nullptr));
  }
  return p;
}

PatchTracks TrackPatches(const Pyramid &tmpl, const Pyramid &next, const std::vector<std::array<double, 2>> &points,
                         const TrackOptions &options, const Pyramid *prev,
                         const std::vector<std::array<double, 2>> *init_points, const std::vector<double> *init_angles,
                         const std::vector<std::array<double, 2>> *pattern) {
  const size_t n = points.size(), L = tmpl.levels.size();
  if (L < 1 || L > PNEC_HIP_TRACK_MAX_LEVELS) throw std::invalid_argument("a pyramid must have 1 .. 8 levels");
  for (const Pyramid *p : {&next, prev})
    if (p && (p->levels.size() != L || p->height != tmpl.height || p->width != tmpl.width || p->pixel_type != tmpl.pixel_type))
      throw std::invalid_argument("the pyramids must have the same levels, size and pixel type");
  if ((init_points && init_points->size() != n) || (init_angles && init_angles->size() != n))
    throw std::invalid_argument("init_points / init_angles must have one entry per keypoint");
  const std::vector<std::array<double, 2>> &pat = pattern ? *pattern : Pattern52();
  const double nan = std::nan("");
  PatchTracks out;
  out.points.assign(n, std::array<double, 2>{nan, nan});
  out.angles.assign(n, nan);
  out.covariances.assign(n, std::array<double, 3>{nan, nan, nan});
  out.dist2.assign(n, nan);
  std::vector<int32_t> st(n, PNEC_HIP_TRACK_BAD_TEMPLATE), lv(n, -1);
  if (n > 0) {
    const void *tp[PNEC_HIP_TRACK_MAX_LEVELS], *np[PNEC_HIP_TRACK_MAX_LEVELS], *pp[PNEC_HIP_TRACK_MAX_LEVELS];
    int64_t pitch[PNEC_HIP_TRACK_MAX_LEVELS];
    const size_t es = PixelBytes(tmpl.pixel_type);
    for (size_t l = 0; l < L; ++l) {
      pitch[l] = tmpl.width >> l;
      const size_t bytes = (size_t)(tmpl.height >> l) * (size_t)(tmpl.width >> l) * es;
      for (const Pyramid *p : {&tmpl, &next, prev})
        if (p && p->levels[l].size() != bytes) throw std::invalid_argument("a pyramid level has the wrong size");
      tp[l] = tmpl.levels[l].data();
      np[l] = next.levels[l].data();
      pp[l] = prev ? prev->levels[l].data() : nullptr;
    }
    const int64_t offsets[2] = {0, (int64_t)n};
    Check(pnec_hip_patch_track(tp, pitch, prev ? pp : nullptr, prev ? pitch : nullptr, np, pitch, (int32_t)L,
                               (int)tmpl.pixel_type, 1, tmpl.height, tmpl.width, offsets, (int64_t)n, points[0].data(),
                               init_points ? (*init_points)[0].data() : nullptr, init_angles ? init_angles->data() : nullptr,
                               options.shift[0], options.shift[1], pat.empty() ? nullptr : pat[0].data(), (int32_t)pat.size(),
                               options.max_iterations, options.max_recovered_dist2,
                               options.backward ? 0u : PNEC_HIP_TRACK_NO_BACKWARD, options.scaling, out.points[0].data(),
                               out.angles.data(), out.covariances[0].data(), out.dist2.data(), st.data(), lv.data(),
                               PNEC_HIP_MEM_HOST, optimization::SolverOptions().device, nullptr));
  }
  out.status.assign(st.begin(), st.end());
  out.lost_level.assign(lv.begin(), lv.end());
  return out;
}

Keypoints DetectKeypoints(const void *image, pnec_hip_pixel_type pixel_type, int height, int width, int64_t pitch,
                          const DetectOptions &options, const std::vector<std::array<double, 2>> *current) {
  if (!image) throw std::invalid_argument("image is NULL");
  if (options.grid < 8 || options.grid > 64) throw std::invalid_argument("grid must be 8 .. 64");
  if (options.points_per_cell < 1 || options.points_per_cell > 4) throw std::invalid_argument("points_per_cell must be 1 .. 4");
  if (height < options.grid || width < options.grid) throw std::invalid_argument("the image is smaller than one grid cell");
  Keypoints out;
  out.nx = width / options.grid;
  out.ny = height / options.grid;
  const size_t n_cells = (size_t)out.nx * (size_t)out.ny, cap = n_cells * (size_t)options.points_per_cell;
  std::vector<int32_t> cell(n_cells, 0), score(cap, 0), index(cap, 0);
  std::vector<std::array<double, 2>> pts(cap);
  int64_t offsets[2] = {0, 0};
  const int64_t n_cur = current ? (int64_t)current->size() : 0;
  const int64_t cur_offsets[2] = {0, n_cur};
  Check(pnec_hip_detect_keypoints(image, (int)pixel_type, 1, height, width, pitch > 0 ? pitch : width, options.grid,
                                  options.points_per_cell, options.min_threshold, options.edge,
                                  n_cur > 0 ? cur_offsets : nullptr, n_cur, n_cur > 0 ? (*current)[0].data() : nullptr,
                                  cell.data(), offsets, pts[0].data(), score.data(), index.data(), PNEC_HIP_MEM_HOST,
                                  optimization::SolverOptions().device, nullptr));
  const size_t n = (size_t)offsets[1];
  out.points.assign(pts.begin(), pts.begin() + (std::ptrdiff_t)n);
  out.score.assign(score.begin(), score.begin() + (std::ptrdiff_t)n);
  out.cell_index.assign(index.begin(), index.begin() + (std::ptrdiff_t)n);
  out.cell.assign(cell.begin(), cell.end());
  return out;
}

Tracks RetainTracks(const Tracks &t, const PatchTracks &r, int max_age) {
  const size_t n = t.id.size();
  const bool cov = !t.covariances.empty() || n == 0;
  if (t.tmpl_image.size() != n || t.age.size() != n || t.tmpl_points.size() != n || t.points.size() != n ||
      (!t.covariances.empty() && t.covariances.size() != n))
    throw std::invalid_argument("the arrays of a track set must have one entry per track");
  if (r.points.size() != n || r.angles.size() != n || r.status.size() != n || (cov && r.covariances.size() != n))
    throw std::invalid_argument("the track result must have one entry per track");
  Tracks out;
  if (n == 0) return out;
  const double nan = std::nan("");
  std::vector<int32_t> ti(t.tmpl_image.begin(), t.tmpl_image.end()), age(t.age.begin(), t.age.end()),
      st(r.status.begin(), r.status.end()), o_ti(n), o_age(n);
  out.id.assign(n, -1);
  out.src.assign(n, -1);
  out.tmpl_points.assign(n, {nan, nan});
  out.points.assign(n, {nan, nan});
  out.prev_points.assign(n, {nan, nan});
  out.angles.assign(n, nan);
  if (cov) {
    out.covariances.assign(n, {nan, nan, nan});
    out.prev_covariances.assign(n, {nan, nan, nan});
  }
  const int64_t offsets[2] = {0, (int64_t)n};
  int64_t o_off[2] = {0, 0};
  Check(pnec_hip_tracks_retain(1, offsets, (int64_t)n, t.id.data(), ti.data(), t.tmpl_points[0].data(), age.data(),
                               t.points[0].data(), cov ? t.covariances[0].data() : nullptr, r.points[0].data(),
                               r.angles.data(), cov ? r.covariances[0].data() : nullptr, st.data(), max_age, o_off,
                               out.id.data(), o_ti.data(), out.tmpl_points[0].data(), o_age.data(), out.points[0].data(),
                               out.angles.data(), cov ? out.covariances[0].data() : nullptr, out.prev_points[0].data(),
                               cov ? out.prev_covariances[0].data() : nullptr, out.src.data(), PNEC_HIP_MEM_HOST,
                               optimization::SolverOptions().device, nullptr));
  const size_t m = (size_t)o_off[1];
  out.id.resize(m);
  out.src.resize(m);
  out.tmpl_points.resize(m);
  out.points.resize(m);
  out.prev_points.resize(m);
  out.angles.resize(m);
  if (cov) {
    out.covariances.resize(m);
    out.prev_covariances.resize(m);
  }
  out.tmpl_image.assign(o_ti.begin(), o_ti.begin() + (std::ptrdiff_t)m);
  out.age.assign(o_age.begin(), o_age.begin() + (std::ptrdiff_t)m);
  return out;
}

Tracks AppendTracks(const Tracks *t, const Keypoints &det, const std::vector<std::array<double, 3>> *det_cov, int tmpl_image,
                    int64_t capacity, int64_t *next_id, int64_t *dropped) {
  if (!next_id) throw std::invalid_argument("next_id is NULL");
  if (capacity < 1) throw std::invalid_argument("capacity must be >= 1");
  const size_t n = t ? t->id.size() : 0, d = det.points.size();
  if (t && (t->tmpl_image.size() != n || t->age.size() != n || t->tmpl_points.size() != n || t->points.size() != n ||
            t->angles.size() != n || (!t->covariances.empty() && t->covariances.size() != n)))
    throw std::invalid_argument("the arrays of a track set must have one entry per track");
  if (det_cov && det_cov->size() != d) throw std::invalid_argument("det_covariances must have one entry per detection");
  const bool set = t && n > 0, set_cov = set && !t->covariances.empty(), cov = det_cov || set_cov;
  const size_t rows = std::min<size_t>((size_t)std::min<int64_t>(capacity, (int64_t)(n + d)), n + d);
  const double nan = std::nan("");
  Tracks out;
  std::vector<int32_t> ti, age, o_ti(rows), o_age(rows);
  if (set) {
    ti.assign(t->tmpl_image.begin(), t->tmpl_image.end());
    age.assign(t->age.begin(), t->age.end());
  }
  out.id.assign(rows, -1);
  out.tmpl_points.assign(rows, {nan, nan});
  out.points.assign(rows, {nan, nan});
  out.angles.assign(rows, nan);
  if (cov) out.covariances.assign(rows, {nan, nan, nan});
  const int64_t offsets[2] = {0, (int64_t)n}, det_offsets[2] = {0, (int64_t)d};
  int64_t o_off[2] = {0, 0}, drop = 0;
  const std::array<double, 2> none2 = {nan, nan};
  Check(pnec_hip_tracks_append(1, set ? offsets : nullptr, set ? (int64_t)n : 0, set ? t->id.data() : nullptr,
                               set ? ti.data() : nullptr, set ? t->tmpl_points[0].data() : nullptr, set ? age.data() : nullptr,
                               set ? t->points[0].data() : nullptr, set ? t->angles.data() : nullptr,
                               set_cov ? t->covariances[0].data() : nullptr, det_offsets, (int64_t)d,
                               d > 0 ? det.points[0].data() : none2.data(), det_cov && d > 0 ? (*det_cov)[0].data() : nullptr,
                               tmpl_image, capacity, next_id, (int64_t)rows, o_off, rows ? out.id.data() : nullptr,
                               o_ti.data(), rows ? out.tmpl_points[0].data() : nullptr, o_age.data(),
                               rows ? out.points[0].data() : nullptr, out.angles.data(),
                               cov && rows ? out.covariances[0].data() : nullptr, &drop, PNEC_HIP_MEM_HOST,
                               optimization::SolverOptions().device, nullptr));
  out.tmpl_image.assign(o_ti.begin(), o_ti.end());
  out.age.assign(o_age.begin(), o_age.end());
  if (dropped) *dropped = drop;
  return out;
}

PatchTracks TrackPatches(const std::vector<const Pyramid *> &stack, const std::vector<int> &tmpl_image, const Pyramid &prev,
                         const Pyramid &next, const std::vector<std::array<double, 2>> &points, const TrackOptions &options,
                         const std::vector<std::array<double, 2>> *init_points, const std::vector<double> *init_angles,
                         const std::vector<std::array<double, 2>> *pattern) {
  const size_t n = points.size(), L = next.levels.size(), S = stack.size();
  if (L < 1 || L > PNEC_HIP_TRACK_MAX_LEVELS) throw std::invalid_argument("a pyramid must have 1 .. 8 levels");
  if (S < 1) throw std::invalid_argument("the template stack is empty");
  if (tmpl_image.size() != n) throw std::invalid_argument("tmpl_image must have one entry per keypoint");
  std::vector<const Pyramid *> all(stack);
  all.push_back(&prev);
  for (const Pyramid *p : all)
    if (!p || p->levels.size() != L || p->height != next.height || p->width != next.width || p->pixel_type != next.pixel_type)
      throw std::invalid_argument("the pyramids must have the same levels, size and pixel type");
  if ((init_points && init_points->size() != n) || (init_angles && init_angles->size() != n))
    throw std::invalid_argument("init_points / init_angles must have one entry per keypoint");
  const std::vector<std::array<double, 2>> &pat = pattern ? *pattern : Pattern52();
  const double nan = std::nan("");
  PatchTracks out;
  out.points.assign(n, std::array<double, 2>{nan, nan});
  out.angles.assign(n, nan);
  out.covariances.assign(n, std::array<double, 3>{nan, nan, nan});
  out.dist2.assign(n, nan);
  std::vector<int32_t> st(n, PNEC_HIP_TRACK_BAD_TEMPLATE), lv(n, -1), ti(tmpl_image.begin(), tmpl_image.end());
  if (n > 0) {
    // the stack as one block of S images per level
    std::vector<std::vector<unsigned char>> block(L);
    const void *tp[PNEC_HIP_TRACK_MAX_LEVELS], *np[PNEC_HIP_TRACK_MAX_LEVELS], *pp[PNEC_HIP_TRACK_MAX_LEVELS];
    int64_t pitch[PNEC_HIP_TRACK_MAX_LEVELS];
    const size_t es = PixelBytes(next.pixel_type);
    for (size_t l = 0; l < L; ++l) {
      pitch[l] = next.width >> l;
      const size_t bytes = (size_t)(next.height >> l) * (size_t)(next.width >> l) * es;
      all.push_back(&next);
      for (const Pyramid *p : all)
        if (p->levels[l].size() != bytes) throw std::invalid_argument("a pyramid level has the wrong size");
      all.pop_back();
      block[l].resize(bytes * S);
      for (size_t i = 0; i < S; ++i) std::memcpy(block[l].data() + i * bytes, stack[i]->levels[l].data(), bytes);
      tp[l] = block[l].data();
      np[l] = next.levels[l].data();
      pp[l] = prev.levels[l].data();
    }
    const int64_t offsets[2] = {0, (int64_t)n};
    Check(pnec_hip_patch_track_indexed(tp, pitch, (int64_t)S, pp, pitch, np, pitch, (int32_t)L, (int)next.pixel_type, 1,
                                       next.height, next.width, offsets, (int64_t)n, points[0].data(), ti.data(),
                                       init_points ? (*init_points)[0].data() : nullptr,
                                       init_angles ? init_angles->data() : nullptr, options.shift[0], options.shift[1],
                                       pat.empty() ? nullptr : pat[0].data(), (int32_t)pat.size(), options.max_iterations,
                                       options.max_recovered_dist2, options.backward ? 0u : PNEC_HIP_TRACK_NO_BACKWARD,
                                       options.scaling, out.points[0].data(), out.angles.data(), out.covariances[0].data(),
                                       out.dist2.data(), st.data(), lv.data(), PNEC_HIP_MEM_HOST,
                                       optimization::SolverOptions().device, nullptr));
  }
  out.status.assign(st.begin(), st.end());
  out.lost_level.assign(lv.begin(), lv.end());
  return out;
}

std::vector<int32_t> LinkTracks(const std::vector<int64_t> &prev_ids, const std::vector<int64_t> &cur_ids) {
  std::vector<int32_t> link(cur_ids.size(), -1);
  if (cur_ids.empty()) return link;
  const int64_t cur_offsets[2] = {0, (int64_t)cur_ids.size()}, prev_offsets[2] = {0, (int64_t)prev_ids.size()};
  Check(pnec_hip_tracks_link(1, cur_offsets, (int64_t)cur_ids.size(), cur_ids.data(), prev_offsets, (int64_t)prev_ids.size(),
                             prev_ids.empty() ? nullptr : prev_ids.data(), link.data(), nullptr, PNEC_HIP_MEM_HOST,
                             optimization::SolverOptions().device, nullptr));
  return link;
}

}  // namespace features

// -------------------------------------------------------------------------------- optimization
namespace optimization {

pnec_hip_options SolverOptions::ToHip() const {
  pnec_hip_options o;
  pnec_hip_default_options(&o);
  o.max_num_iterations = max_num_iterations;
  o.max_num_consecutive_invalid_steps = max_num_consecutive_invalid_steps;
  o.jacobi_scaling = jacobi_scaling ? 1 : 0;
  o.function_tolerance = function_tolerance;
  o.gradient_tolerance = gradient_tolerance;
  o.parameter_tolerance = parameter_tolerance;
  o.initial_trust_region_radius = initial_trust_region_radius;
  o.max_trust_region_radius = max_trust_region_radius;
  o.min_trust_region_radius = min_trust_region_radius;
  o.min_relative_decrease = min_relative_decrease;
  o.min_lm_diagonal = min_lm_diagonal;
  o.max_lm_diagonal = max_lm_diagonal;
  return o;
}

PNECCeres::PNECCeres() : orientation_(1.0, 0.0, 0.0, 0.0), theta_(0.0), phi_(0.0) {}
PNECCeres::PNECCeres(const SE3d &init, const SolverOptions &options) : options_(options) {
  orientation_ = init.unit_quaternion();
  common::AnglesFromVec(init.translation(), theta_, phi_);
}
// (the reference drops `options` in this overload, pnec_ceres.cc:57-59; kept here)
PNECCeres::PNECCeres(const Quaterniond &orientation, double theta, double phi,
                     const SolverOptions &options)
    : orientation_(orientation), theta_(theta), phi_(phi), options_(options) {}
PNECCeres::PNECCeres(const Quaterniond &orientation, const Vector3d &translation,
                     const SolverOptions &options)
    : orientation_(orientation), options_(options) {
  common::AnglesFromVec(translation, theta_, phi_);
}
PNECCeres::~PNECCeres() {}

void PNECCeres::Run(int mode, const std::vector<Vector3d> &b1, const std::vector<Vector3d> &b2,
                    const std::vector<Matrix3d> *covs, const std::vector<Matrix3d> *covs_host,
                    double reg) {
  SolveOne(mode, options_, b1, b2, covs, covs_host, reg, orientation_, theta_, phi_, summary_);
}

void PNECCeres::Optimize(const std::vector<Vector3d> &bvs_1, const std::vector<Vector3d> &bvs_2,
                         const std::vector<Matrix3d> &covs, double regularization,
                         common::NoiseFrame noise_frame) {
  Run(noise_frame == common::Host ? PNEC_HIP_MODE_HOST : PNEC_HIP_MODE_TARGET, bvs_1, bvs_2, &covs,
      nullptr, regularization);
}

void PNECCeres::Optimize(const std::vector<Vector3d> &bvs_1, const std::vector<Vector3d> &bvs_2,
                         const std::vector<Matrix3d> &covs_1, const std::vector<Matrix3d> &covs_2,
                         double regularization) {
  // PNECSymmetrical(bv_1, bv_2, cov_1, cov_2): cov_2 rides with R Sigma R', cov_1 with [R f2]x
  Run(PNEC_HIP_MODE_SYM, bvs_1, bvs_2, &covs_2, &covs_1, regularization);
}

void PNECCeres::InitValues(const Quaterniond orientation, double theta, double phi) {
  orientation_ = orientation;
  theta_ = theta;
  phi_ = phi;
}
void PNECCeres::InitValues(const SE3d &init) {
  orientation_ = init.unit_quaternion();
  common::AnglesFromVec(init.translation(), theta_, phi_);
}
void PNECCeres::InitValues(const Quaterniond &orientation, const Vector3d &translation) {
  orientation_ = orientation;
  common::AnglesFromVec(translation, theta_, phi_);
}
void PNECCeres::SetOptions(const SolverOptions &options) { options_ = options; }
Matrix3d PNECCeres::Orientation() const { return orientation_.normalized().toRotationMatrix(); }
Vector3d PNECCeres::Translation() const { return TranslationFromAngles(theta_, phi_); }
SE3d PNECCeres::Result() const { return SE3d(Orientation(), Translation()); }

NECCeres::NECCeres() : orientation_(1.0, 0.0, 0.0, 0.0), theta_(0.0), phi_(0.0) {}
NECCeres::NECCeres(const SE3d &init, const SolverOptions &options) : options_(options) {
  orientation_ = init.unit_quaternion();
  common::AnglesFromVec(init.translation(), theta_, phi_);
}
NECCeres::NECCeres(const Quaterniond &orientation, double theta, double phi, const SolverOptions &options)
    : orientation_(orientation), theta_(theta), phi_(phi), options_(options) {}
NECCeres::NECCeres(const Quaterniond &orientation, const Vector3d &translation,
                   const SolverOptions &options)
    : orientation_(orientation), options_(options) {
  common::AnglesFromVec(translation, theta_, phi_);
}
NECCeres::~NECCeres() {}
void NECCeres::Optimize(const std::vector<Vector3d> &bvs_1, const std::vector<Vector3d> &bvs_2) {
  SolveOne(PNEC_HIP_MODE_NEC, options_, bvs_1, bvs_2, nullptr, nullptr, 0.0, orientation_, theta_,
           phi_, summary_);
}
void NECCeres::InitValues(const Quaterniond orientation, double theta, double phi) {
  orientation_ = orientation;
  theta_ = theta;
  phi_ = phi;
}
void NECCeres::InitValues(const SE3d &init) {
  orientation_ = init.unit_quaternion();
  common::AnglesFromVec(init.translation(), theta_, phi_);
}
void NECCeres::InitValues(const Quaterniond &orientation, const Vector3d &translation) {
  orientation_ = orientation;
  common::AnglesFromVec(translation, theta_, phi_);
}
void NECCeres::SetOptions(const SolverOptions &options) { options_ = options; }
Matrix3d NECCeres::Orientation() const { return orientation_.normalized().toRotationMatrix(); }
Vector3d NECCeres::Translation() const { return TranslationFromAngles(theta_, phi_); }
SE3d NECCeres::Result() const { return SE3d(Orientation(), Translation()); }

}  // namespace optimization

// -------------------------------------------------------------------------- rel_pose_estimation
namespace rel_pose_estimation {

PNEC::PNEC(const Options &options) : options_(options) {}

SE3d PNEC::Solve(const bearingVectors_t &bvs1, const bearingVectors_t &bvs2,
                 const std::vector<Matrix3d> &projected_covs, const SE3d &initial_pose) {
  std::vector<int> inliers;
  return Solve(bvs1, bvs2, projected_covs, initial_pose, inliers);
}

namespace {
// The per-thread frame handle of a device (pnec_hip_frame: pinned staging, a capacity-shaped one-pair batch with
// its cached scratch, one HIP stream -- all created once): PNEC::Solve is called once per frame pair by the
// odometry (frame2frame.cc:122-141), and a batch object per call cost more than the chain's kernels take.
// Grown (re-created) when a pair exceeds its capacity.
struct ThreadFrame {
  pnec_hip_frame *f = nullptr;
  int device = -1;
  ~ThreadFrame() { pnec_hip_frame_destroy(f); }
  pnec_hip_frame *Get(int dev, int64_t n) {
    if (!f || dev != device || n > pnec_hip_frame_capacity(f)) {
      pnec_hip_frame_destroy(f);
      f = nullptr;
      int64_t cap = 2048;
      while (cap < n) cap *= 2;
      Check(pnec_hip_frame_create(dev, cap, nullptr, &f));
      device = dev;
    }
    return f;
  }
};
thread_local ThreadFrame g_frame;

// one pair resident on the device (the thread's frame handle's batch), shared by the stages of Solve
struct PairOnDevice {
  struct {
    pnec_hip_problem *p = nullptr;
  } prob;
  pnec_hip_frame *frame = nullptr;
  PairOnDevice(int device, const bearingVectors_t &b1, const bearingVectors_t &b2,
               const std::vector<Matrix3d> &covs) {
    if (b1.size() != b2.size() || b1.size() != covs.size())
      throw std::invalid_argument("bvs1, bvs2 and projected_covs differ in size");
    frame = g_frame.Get(device, (int64_t)b1.size());
    Check(pnec_hip_frame_load(frame, (int64_t)b1.size(), b1.empty() ? nullptr : b1[0].data(),
                              b2.empty() ? nullptr : b2[0].data(), covs.empty() ? nullptr : covs[0].data(), &prob.p));
  }
};

// the Options fields PNEC::Solve reads (pnec.cc:87,96,97,105,109,116,239,246,249,300,327,367); the
// refinement uses default solver options whatever Options::ceres_options_ says (quirk C1, pnec.cc:355)
pnec_hip_pipeline_options ToPipeline(const Options &o) {
  pnec_hip_pipeline_options p;
  pnec_hip_default_pipeline_options(&p);
  p.use_ransac = o.use_ransac_ ? 1 : 0;
  p.use_nec = o.use_nec_ ? 1 : 0;
  p.use_ceres = o.use_ceres_ ? 1 : 0;
  p.weighted_iterations = (int32_t)o.weighted_iterations_;
  p.max_ransac_iterations = o.max_ransac_iterations_;
  p.ransac_sample_size = o.ransac_sample_size_;
  p.regularization = o.regularization_;
  p.solver = optimization::SolverOptions().ToHip();
  p.eigensolver_scheme = o.eigensolver_scheme_;
  p.ransac_flags = o.ransac_chained_starts_ ? PNEC_HIP_RANSAC_CHAINED_STARTS : 0;
  return p;
}

SE3d PoseFromQT(const double q[4], const double t[3]) {
  return SE3d(Quaterniond(q[3], q[0], q[1], q[2]).toRotationMatrix(), Vector3d(t[0], t[1], t[2]));
}
}  // namespace

SE3d PNEC::Solve(const bearingVectors_t &bvs1, const bearingVectors_t &bvs2,
                 const std::vector<Matrix3d> &projected_covs, const SE3d &initial_pose,
                 std::vector<int> &inliers) {
  return SolveImpl(bvs1, bvs2, projected_covs, initial_pose, inliers, nullptr);
}
SE3d PNEC::Solve(const bearingVectors_t &bvs1, const bearingVectors_t &bvs2,
                 const std::vector<Matrix3d> &projected_covs, const SE3d &initial_pose,
                 common::FrameTiming &timing) {
  std::vector<int> inliers;
  return SolveImpl(bvs1, bvs2, projected_covs, initial_pose, inliers, &timing);
}
SE3d PNEC::Solve(const bearingVectors_t &bvs1, const bearingVectors_t &bvs2,
                 const std::vector<Matrix3d> &projected_covs, const SE3d &initial_pose,
                 std::vector<int> &inliers, common::FrameTiming &timing) {
  return SolveImpl(bvs1, bvs2, projected_covs, initial_pose, inliers, &timing);
}

SE3d PNEC::SolveImpl(const bearingVectors_t &bvs1, const bearingVectors_t &bvs2,
                     const std::vector<Matrix3d> &projected_covs, const SE3d &initial_pose,
                     std::vector<int> &inliers, common::FrameTiming *timing) {
  // pnec.cc:77-124 (timed twin :135-208), stage by stage on the device.
  using clock = std::chrono::high_resolution_clock;
  // (one reading per stage: the millisecond field is the microsecond reading truncated, as duration_cast does)
  auto us_since = [](clock::time_point t0) { return std::chrono::duration<double, std::micro>(clock::now() - t0).count(); };
  auto tic = clock::now();
  const Quaterniond q0(initial_pose.rotationMatrix());
  double q[4], t[3];
  if (!timing) {
    // the untimed overloads: the whole chain in one call on the thread's frame handle -- arrays in through
    // pinned staging, stages chained on the device, pose and inlier mask written straight back
    if (bvs1.size() != bvs2.size() || bvs1.size() != projected_covs.size())
      throw std::invalid_argument("bvs1, bvs2 and projected_covs differ in size");
    const pnec_hip_pipeline_options po = ToPipeline(options_);
    std::vector<uint8_t> mask(bvs1.size() ? bvs1.size() : 1, 0);
    pnec_hip_frame *frame = g_frame.Get(optimization::SolverOptions().device, (int64_t)bvs1.size());
    Check(pnec_hip_frame_solve(frame, (int64_t)bvs1.size(), bvs1.empty() ? nullptr : bvs1[0].data(),
                               bvs2.empty() ? nullptr : bvs2[0].data(),
                               projected_covs.empty() ? nullptr : projected_covs[0].data(), q0.coeffs(),
                               initial_pose.translation().data(), &po, q, t, mask.data(), nullptr));
    inliers.clear();
    if (options_.use_ransac_)
      for (size_t i = 0; i < bvs1.size(); ++i)
        if (mask[i]) inliers.push_back((int)i);
    return PoseFromQT(q, t);
  }
  // the timed overloads run stage by stage (each stage's wall time is what FrameTiming reports)
  PairOnDevice dev(optimization::SolverOptions().device, bvs1, bvs2, projected_covs);
  void *const st = pnec_hip_frame_stream(dev.frame);   // the ingest is queued there: the stages follow it
  pnec_hip_problem *stage = dev.prob.p;   // the batch the later stages run on (inliers under RANSAC)
  pnec_hip_problem *selected = nullptr;   // the handle's cached InlierExtraction target: nothing to destroy
  Check(pnec_hip_problem_set_eigensolver_scheme(dev.prob.p, options_.eigensolver_scheme_));
  Check(pnec_hip_problem_set_ransac_flags(dev.prob.p, options_.ransac_chained_starts_ ? PNEC_HIP_RANSAC_CHAINED_STARTS : 0));
  // ES_solution = Eigensolver(bvs1, bvs2, initial_pose, inliers)
  inliers.clear();
  if (options_.use_ransac_) {
    std::vector<uint8_t> mask(bvs1.size() ? bvs1.size() : 1);
    Check(pnec_hip_ransac_eigensolver(dev.prob.p, q0.coeffs(), /*seed*/ 1, options_.max_ransac_iterations_,
                                      options_.ransac_sample_size_, /*threshold pnec.cc:248*/ 1.0e-6, q, t,
                                      mask.data(), nullptr, nullptr, PNEC_HIP_MEM_HOST, st));
    for (size_t i = 0; i < bvs1.size(); ++i)
      if (mask[i]) inliers.push_back((int)i);
    // InlierExtraction (pnec.cc:210-229)
    Check(pnec_hip_problem_select_view(dev.prob.p, mask.data(), PNEC_HIP_MEM_HOST, st, &selected));
    Check(pnec_hip_problem_set_eigensolver_scheme(selected, options_.eigensolver_scheme_));
    stage = selected;
  } else {
    Check(pnec_hip_nec_eigensolver(dev.prob.p, q0.coeffs(), q, t, PNEC_HIP_MEM_HOST, st));
  }
  if (timing) { timing->nec_es_us_ = us_since(tic); timing->nec_es_ = (long)(timing->nec_es_us_ / 1000.0); }
  const pnec_hip_options o = optimization::SolverOptions().ToHip();
  double oq[4], ot[3];
  if (options_.use_nec_) {
    if (timing) timing->ceres_ = 0;
    if (!options_.use_ceres_) return PoseFromQT(q, t);
    tic = clock::now();
    // NECCeresSolver on the (inlier) bearings: the NEC residual ignores the covariance planes, but
    // the kernel family is fixed by the batch, so the inlier bearings go into a NEC batch
    std::vector<Vector3d> b1, b2;
    if (options_.use_ransac_) {
      for (int i : inliers) { b1.push_back(bvs1[(size_t)i]); b2.push_back(bvs2[(size_t)i]); }
    } else {
      b1 = bvs1; b2 = bvs2;
    }
    const SE3d nec = NECCeresSolver(b1, b2, PoseFromQT(q, t));
    if (timing) { timing->ceres_us_ = us_since(tic); timing->ceres_ = (long)(timing->ceres_us_ / 1000.0); }
    return nec;
  }
  double qi[4], ti[3];
  // it_es_ is written in every branch, avg_it_es_ only when the weighted stage runs (pnec.cc:178-195)
  if (timing) timing->it_es_ = 0;
  if (options_.weighted_iterations_ > 1) {
    tic = clock::now();
    Check(pnec_hip_weighted_eigensolver(stage, q, t, options_.regularization_,
                                        (int32_t)options_.weighted_iterations_, qi, ti, PNEC_HIP_MEM_HOST,
                                        st));
    if (timing) {
      timing->it_es_us_ = us_since(tic);
      timing->it_es_ = (long)(timing->it_es_us_ / 1000.0);
      timing->avg_it_es_ = timing->it_es_ / (long)options_.weighted_iterations_;
      timing->avg_it_es_us_ = timing->it_es_us_ / (double)options_.weighted_iterations_;
    }
  } else if (options_.weighted_iterations_ == 1) {
    std::memcpy(qi, q, sizeof(qi));
    std::memcpy(ti, t, sizeof(ti));
  } else {
    std::memcpy(qi, q0.coeffs(), sizeof(qi));
    std::memcpy(ti, initial_pose.translation().data(), sizeof(ti));
  }
  if (timing) timing->ceres_ = 0;
  if (!options_.use_ceres_) return PoseFromQT(qi, ti);
  // CeresSolver: default-constructed optimiser, Target frame (pnec.cc:355,366)
  tic = clock::now();
  Check(pnec_hip_solve(stage, qi, ti, 1, nullptr, options_.regularization_, &o, oq, ot, nullptr, nullptr,
                       nullptr, PNEC_HIP_MEM_HOST, st));
  if (timing) { timing->ceres_us_ = us_since(tic); timing->ceres_ = (long)(timing->ceres_us_ / 1000.0); }
  return PoseFromQT(oq, ot);
}

SE3d PNEC::Eigensolver(const bearingVectors_t &bvs1, const bearingVectors_t &bvs2,
                       const SE3d &initial_pose, std::vector<int> &inliers) {
  inliers.clear();
  const std::vector<int64_t> offsets = {0, (int64_t)bvs1.size()};
  Problem prob(optimization::SolverOptions().device, PNEC_HIP_MODE_NEC, offsets);
  if (!bvs1.empty())
    Check(pnec_hip_problem_fill(prob.p, 0, 1, bvs1[0].data(), bvs2[0].data(), nullptr, nullptr,
                                PNEC_HIP_MEM_HOST, nullptr));
  Check(pnec_hip_problem_set_eigensolver_scheme(prob.p, options_.eigensolver_scheme_));
  Check(pnec_hip_problem_set_ransac_flags(prob.p, options_.ransac_chained_starts_ ? PNEC_HIP_RANSAC_CHAINED_STARTS : 0));
  const Quaterniond q0(initial_pose.rotationMatrix());
  double q[4], t[3];
  if (options_.use_ransac_) {
    std::vector<uint8_t> mask(bvs1.size() ? bvs1.size() : 1);
    Check(pnec_hip_ransac_eigensolver(prob.p, q0.coeffs(), 1, options_.max_ransac_iterations_,
                                      options_.ransac_sample_size_, 1.0e-6, q, t, mask.data(), nullptr, nullptr,
                                      PNEC_HIP_MEM_HOST, nullptr));
    for (size_t i = 0; i < bvs1.size(); ++i)
      if (mask[i]) inliers.push_back((int)i);
  } else {
    Check(pnec_hip_nec_eigensolver(prob.p, q0.coeffs(), q, t, PNEC_HIP_MEM_HOST, nullptr));
  }
  return PoseFromQT(q, t);
}

SE3d PNEC::WeightedEigensolver(const bearingVectors_t &bvs1, const bearingVectors_t &bvs2,
                               const std::vector<Matrix3d> &projected_covariances,
                               const SE3d &initial_pose) {
  PairOnDevice dev(optimization::SolverOptions().device, bvs1, bvs2, projected_covariances);
  Check(pnec_hip_problem_set_eigensolver_scheme(dev.prob.p, options_.eigensolver_scheme_));
  const Quaterniond q0(initial_pose.rotationMatrix());
  double q[4], t[3];
  Check(pnec_hip_weighted_eigensolver(dev.prob.p, q0.coeffs(), initial_pose.translation().data(),
                                      options_.regularization_, (int32_t)options_.weighted_iterations_, q, t,
                                      PNEC_HIP_MEM_HOST, pnec_hip_frame_stream(dev.frame)));
  return PoseFromQT(q, t);
}

SE3d PNEC::CeresSolver(const bearingVectors_t &bvs1, const bearingVectors_t &bvs2,
                       const std::vector<Matrix3d> &projected_covariances, const SE3d &initial_pose) {
  return CeresSolverFull(bvs1, bvs2, projected_covariances, options_.regularization_, initial_pose);
}

SE3d PNEC::CeresSolverFull(const bearingVectors_t &bvs1, const bearingVectors_t &bvs2,
                           const std::vector<Matrix3d> &projected_covariances, double regularization,
                           const SE3d &initial_pose) {
  // default-constructed optimiser and Target frame, like the reference (pnec.cc:355,366: it ignores
  // Options::ceres_options_ and noise_frame_)
  optimization::PNECCeres optimizer;
  optimizer.InitValues(Quaterniond(initial_pose.rotationMatrix()), initial_pose.translation());
  optimizer.Optimize(bvs1, bvs2, projected_covariances, regularization);
  return optimizer.Result();
}

SE3d PNEC::NECCeresSolver(const bearingVectors_t &bvs1, const bearingVectors_t &bvs2,
                          const SE3d &initial_pose) {
  optimization::NECCeres optimizer;
  optimizer.InitValues(Quaterniond(initial_pose.rotationMatrix()), initial_pose.translation());
  optimizer.Optimize(bvs1, bvs2);
  return optimizer.Result();
}

namespace {
// a ragged batch on the host, flattened the way pnec_hip_problem_fill ingests it
struct FlatBatch {
  std::vector<int64_t> offsets;
  std::vector<Vector3d> b1, b2;
  std::vector<Matrix3d> cv;
  std::vector<double> q0, t0;
  explicit FlatBatch(const std::vector<FramePair> &pairs) {
    const int64_t B = (int64_t)pairs.size();
    offsets.assign(B + 1, 0);
    for (int64_t p = 0; p < B; ++p) {
      if (pairs[p].bvs1.size() != pairs[p].bvs2.size() || pairs[p].bvs1.size() != pairs[p].projected_covs.size())
        throw std::invalid_argument("FramePair arrays differ in size");
      offsets[p + 1] = offsets[p] + (int64_t)pairs[p].bvs1.size();
    }
    b1.reserve(offsets[B]); b2.reserve(offsets[B]); cv.reserve(offsets[B]);
    q0.resize(4 * B); t0.resize(3 * B);
    for (int64_t p = 0; p < B; ++p) {
      b1.insert(b1.end(), pairs[p].bvs1.begin(), pairs[p].bvs1.end());
      b2.insert(b2.end(), pairs[p].bvs2.begin(), pairs[p].bvs2.end());
      cv.insert(cv.end(), pairs[p].projected_covs.begin(), pairs[p].projected_covs.end());
      const Quaterniond q(pairs[p].initial_pose.rotationMatrix());
      std::memcpy(&q0[4 * p], q.coeffs(), 4 * sizeof(double));
      std::memcpy(&t0[3 * p], pairs[p].initial_pose.translation().data(), 3 * sizeof(double));
    }
  }
};
}  // namespace

std::vector<SE3d> PNEC::SolveBatch(const std::vector<FramePair> &pairs, std::vector<std::vector<int>> *inliers) {
  // pnec.cc:77-124 for every pair: one upload, every stage one launch over the batch with the results
  // handed on in HBM (pnec_hip_solve_pipeline), one download
  const int64_t B = (int64_t)pairs.size();
  std::vector<SE3d> out(B);
  if (inliers) inliers->assign(B, {});
  if (B == 0) return out;
  const FlatBatch h(pairs);
  const int64_t total = h.offsets[B];
  const optimization::SolverOptions so;
  Problem prob(so.device, PNEC_HIP_MODE_TARGET, h.offsets);
  if (total > 0)
    Check(pnec_hip_problem_fill(prob.p, 0, B, h.b1[0].data(), h.b2[0].data(), h.cv[0].data(), nullptr,
                                PNEC_HIP_MEM_HOST, nullptr));
  const pnec_hip_pipeline_options po = ToPipeline(options_);
  std::vector<double> q(4 * B), t(3 * B);
  std::vector<uint8_t> mask;
  if (inliers && options_.use_ransac_) mask.assign(total ? total : 1, 0);
  Check(pnec_hip_solve_pipeline(prob.p, h.q0.data(), h.t0.data(), &po, q.data(), t.data(),
                                mask.empty() ? nullptr : mask.data(), nullptr, PNEC_HIP_MEM_HOST, nullptr));
  if (!mask.empty())
    for (int64_t p = 0; p < B; ++p)
      for (int64_t i = h.offsets[p]; i < h.offsets[p + 1]; ++i)
        if (mask[i]) (*inliers)[p].push_back((int)(i - h.offsets[p]));
  for (int64_t p = 0; p < B; ++p) out[p] = PoseFromQT(&q[4 * p], &t[3 * p]);
  return out;
}

std::vector<SE3d> PNEC::SolveBatch(const std::vector<FramePair> &pairs, const std::vector<int> &devices,
                                   std::vector<std::vector<int>> *inliers) {
  const int64_t B = (int64_t)pairs.size();
  std::vector<SE3d> out(B);
  if (inliers) inliers->assign(B, {});
  if (B == 0) return out;
  if (devices.empty()) throw std::invalid_argument("SolveBatch: empty device list");
  const FlatBatch h(pairs);
  const int64_t total = h.offsets[B];
  const pnec_hip_pipeline_options po = ToPipeline(options_);
  std::vector<double> q(4 * B), t(3 * B);
  std::vector<uint8_t> mask;
  if (inliers && options_.use_ransac_) mask.assign(total ? total : 1, 0);
  std::vector<int32_t> devs(devices.begin(), devices.end());
  Check(pnec_hip_solve_pipeline_multi((int32_t)devs.size(), devs.data(), B, h.offsets.data(),
                                      total ? h.b1[0].data() : nullptr, total ? h.b2[0].data() : nullptr,
                                      total ? h.cv[0].data() : nullptr, h.q0.data(), h.t0.data(), &po, q.data(), t.data(),
                                      mask.empty() ? nullptr : mask.data(), nullptr));
  if (!mask.empty())
    for (int64_t p = 0; p < B; ++p)
      for (int64_t i = h.offsets[p]; i < h.offsets[p + 1]; ++i)
        if (mask[i]) (*inliers)[p].push_back((int)(i - h.offsets[p]));
  for (int64_t p = 0; p < B; ++p) out[p] = PoseFromQT(&q[4 * p], &t[3 * p]);
  return out;
}

std::vector<SE3d> PNEC::CeresSolverBatch(const std::vector<FramePair> &pairs,
                                         std::vector<optimization::Summary> *summaries) {
  const int64_t B = (int64_t)pairs.size();
  const FlatBatch h(pairs);
  const std::vector<int64_t> &offsets = h.offsets;
  const auto &b1 = h.b1, &b2 = h.b2;
  const auto &cv = h.cv;
  const auto &q0 = h.q0, &t0 = h.t0;
  const optimization::SolverOptions so;  // defaults, as CeresSolver does
  Problem prob(so.device, PNEC_HIP_MODE_TARGET, offsets);
  if (offsets[B] > 0)
    Check(pnec_hip_problem_fill(prob.p, 0, B, b1[0].data(), b2[0].data(), cv[0].data(), nullptr,
                                PNEC_HIP_MEM_HOST, nullptr));
  std::vector<double> oq(4 * B), ot(3 * B), oc(B);
  std::vector<int32_t> oi(B), os(B);
  const pnec_hip_options o = so.ToHip();
  if (B > 0)
    Check(pnec_hip_solve(prob.p, q0.data(), t0.data(), 1, nullptr, options_.regularization_, &o, oq.data(),
                         ot.data(), oc.data(), oi.data(), os.data(), PNEC_HIP_MEM_HOST, nullptr));
  std::vector<SE3d> out(B);
  if (summaries) summaries->resize(B);
  for (int64_t p = 0; p < B; ++p) {
    out[p] = SE3d(Quaterniond(oq[4 * p + 3], oq[4 * p], oq[4 * p + 1], oq[4 * p + 2]).toRotationMatrix(),
                  Vector3d(ot[3 * p], ot[3 * p + 1], ot[3 * p + 2]));
    if (summaries) (*summaries)[p] = {oc[p], oi[p], os[p]};
  }
  return out;
}

PNEC::~PNEC() {
  if (multi_) pnec_hip_multi_destroy(multi_);
}

std::vector<SE3d> PNEC::CeresSolverBatch(const std::vector<FramePair> &pairs, const std::vector<int> &devices,
                                         std::vector<optimization::Summary> *summaries) {
  const int64_t B = (int64_t)pairs.size();
  std::vector<SE3d> out(B);
  if (summaries) summaries->resize(B);
  if (B == 0) return out;
  if (devices.empty()) throw std::invalid_argument("CeresSolverBatch: empty device list");
  const FlatBatch h(pairs);
  const int64_t total = h.offsets[B];
  int64_t max_pair = 0;
  for (int64_t p = 0; p < B; ++p) max_pair = std::max(max_pair, h.offsets[p + 1] - h.offsets[p]);
  if (!multi_ || multi_devices_ != devices || B > multi_pairs_ || total > multi_corr_ || max_pair > multi_pair_corr_) {
    if (multi_) pnec_hip_multi_destroy(multi_);
    multi_ = nullptr;
    std::vector<int32_t> devs(devices.begin(), devices.end());
    // (some head-room, so that a stream of similar batches keeps the handle)
    multi_pairs_ = B + B / 8; multi_corr_ = total + total / 8; multi_pair_corr_ = max_pair + max_pair / 8;
    Check(pnec_hip_multi_create((int32_t)devs.size(), devs.data(), PNEC_HIP_MODE_TARGET, multi_pairs_, multi_corr_,
                                multi_pair_corr_, &multi_));
    multi_devices_ = devices;
  }
  Check(pnec_hip_multi_fill(multi_, B, h.offsets.data(), total ? h.b1[0].data() : nullptr, total ? h.b2[0].data() : nullptr,
                            total ? h.cv[0].data() : nullptr, nullptr));
  std::vector<double> oq(4 * B), ot(3 * B), oc(B);
  std::vector<int32_t> oi(B), os(B);
  const pnec_hip_options o = optimization::SolverOptions().ToHip();   // defaults, as CeresSolver does (quirk C1)
  Check(pnec_hip_multi_solve(multi_, h.q0.data(), h.t0.data(), 1, nullptr, options_.regularization_, &o, oq.data(), ot.data(),
                             oc.data(), oi.data(), os.data()));
  for (int64_t p = 0; p < B; ++p) {
    out[p] = PoseFromQT(&oq[4 * p], &ot[3 * p]);
    if (summaries) (*summaries)[p] = {oc[p], oi[p], os[p]};
  }
  return out;
}

SE3d EMPoseEstimation(const bearingVectors_t &bvs1, const bearingVectors_t &bvs2, const SE3d &initial_pose,
                      algorithm_t algorithm, bool ransac) {
  static const char *const names[] = {"STEWENIUS", "NISTER", "SEVENPT", "EIGHTPT"};
  if (algorithm < STEWENIUS || algorithm > EIGHTPT) throw std::invalid_argument("EMPoseEstimation: unknown algorithm");
  if (algorithm != EIGHTPT)
    throw std::invalid_argument(std::string("EMPoseEstimation: ") + names[algorithm] +
                                " is not built (only EIGHTPT with ransac = false is)");
  if (ransac)
    throw std::invalid_argument("EMPoseEstimation: ransac = true (opengv's CentralRelativePoseSacProblem) is not built "
                                "(only EIGHTPT with ransac = false is)");
  if (bvs1.size() != bvs2.size()) throw std::invalid_argument("bvs1 and bvs2 differ in size");
  if (bvs1.empty()) return initial_pose;
  Problem batch(optimization::SolverOptions().device, PNEC_HIP_MODE_NEC, {0, (int64_t)bvs1.size()});
  Check(pnec_hip_problem_fill(batch.p, 0, 1, bvs1[0].data(), bvs2[0].data(), nullptr, nullptr, PNEC_HIP_MEM_HOST, nullptr));
  double q[4], t[3], singular[3];
  int32_t status = PNEC_HIP_EP_OK;
  Check(pnec_hip_eight_point(batch.p, 0, q, t, nullptr, singular, nullptr, nullptr, nullptr, &status, PNEC_HIP_MEM_HOST,
                             nullptr));
  if (status != PNEC_HIP_EP_OK) return initial_pose;
  // (q comes back with unit norm: no second normalisation, so the matrix is a function of the call's bits alone)
  return SE3d(Quaterniond(q[3], q[0], q[1], q[2]).toRotationMatrix(), Vector3d(t[0], t[1], t[2]) * singular[0]);
}

SE3d MinimalEMPoseEstimation(const bearingVectors_t &bvs1, const bearingVectors_t &bvs2, const SE3d &initial_pose,
                             algorithm_t algorithm) {
  if (algorithm != NISTER && algorithm != SEVENPT)
    throw std::invalid_argument("MinimalEMPoseEstimation: the algorithm is neither NISTER nor SEVENPT");
  if (bvs1.size() != bvs2.size()) throw std::invalid_argument("bvs1 and bvs2 differ in size");
  if (bvs1.empty()) return initial_pose;
  Problem batch(optimization::SolverOptions().device, PNEC_HIP_MODE_NEC, {0, (int64_t)bvs1.size()});
  Check(pnec_hip_problem_fill(batch.p, 0, 1, bvs1[0].data(), bvs2[0].data(), nullptr, nullptr, PNEC_HIP_MEM_HOST, nullptr));
  double q[4], t[3], singular[3];
  int32_t status = PNEC_HIP_EM_OK;
  Check(pnec_hip_essential_minimal(batch.p, algorithm == NISTER ? PNEC_HIP_EM_NISTER : PNEC_HIP_EM_SEVENPT, 0, q, t,
                                   nullptr, singular, nullptr, nullptr, nullptr, nullptr, nullptr, &status,
                                   PNEC_HIP_MEM_HOST, nullptr));
  if (status != PNEC_HIP_EM_OK) return initial_pose;
  return SE3d(Quaterniond(q[3], q[0], q[1], q[2]).toRotationMatrix(), Vector3d(t[0], t[1], t[2]) * singular[0]);
}

SE3d RansacEMPoseEstimation(const bearingVectors_t &bvs1, const bearingVectors_t &bvs2, const SE3d &initial_pose,
                            algorithm_t algorithm, std::vector<int> *inliers, int max_iterations, double threshold,
                            uint64_t seed) {
  if (algorithm == STEWENIUS)
    throw std::invalid_argument("RansacEMPoseEstimation: STEWENIUS is not built (NISTER, SEVENPT and EIGHTPT are)");
  if (algorithm != NISTER && algorithm != SEVENPT && algorithm != EIGHTPT)
    throw std::invalid_argument("RansacEMPoseEstimation: unknown algorithm");
  if (bvs1.size() != bvs2.size()) throw std::invalid_argument("bvs1 and bvs2 differ in size");
  if (inliers) inliers->clear();
  if (bvs1.empty()) return initial_pose;
  Problem batch(optimization::SolverOptions().device, PNEC_HIP_MODE_NEC, {0, (int64_t)bvs1.size()});
  Check(pnec_hip_problem_fill(batch.p, 0, 1, bvs1[0].data(), bvs2[0].data(), nullptr, nullptr, PNEC_HIP_MEM_HOST, nullptr));
  double q[4], t[3], singular[3];
  int32_t status = PNEC_HIP_ER_OK;
  std::vector<uint8_t> mask(bvs1.size());
  // (algorithm_t's values are the ABI's: NISTER 1, SEVENPT 2, EIGHTPT 3)
  Check(pnec_hip_essential_ransac(batch.p, (int32_t)algorithm, seed, 0, max_iterations, threshold, q, t, nullptr, singular,
                                  mask.data(), nullptr, nullptr, nullptr, nullptr, &status, PNEC_HIP_MEM_HOST, nullptr));
  if (status != PNEC_HIP_ER_OK) return initial_pose;
  if (inliers)
    for (size_t i = 0; i < mask.size(); ++i)
      if (mask[i]) inliers->push_back((int)i);
  return SE3d(Quaterniond(q[3], q[0], q[1], q[2]).toRotationMatrix(), Vector3d(t[0], t[1], t[2]) * singular[0]);
}

PoseSensitivityResult PoseSensitivity(const bearingVectors_t &bvs_1, const bearingVectors_t &bvs_2,
                                      const std::vector<Matrix3d> &covs, const SE3d &camera_pose,
                                      const std::array<double, 6> &grad_pose, double regularization) {
  if (bvs_1.size() != bvs_2.size() || bvs_1.size() != covs.size())
    throw std::invalid_argument("bvs_1, bvs_2 and covs differ in size");
  PoseSensitivityResult out;
  const double nan = std::nan("");
  out.lambda.fill(nan);
  out.newton.fill(nan);
  if (bvs_1.empty()) return out;   // no information at all: singular
  out.grad_bvs_1.resize(bvs_1.size());
  out.grad_bvs_2.resize(bvs_1.size());
  out.grad_covs.resize(bvs_1.size());
  const std::vector<int64_t> offsets = {0, (int64_t)bvs_1.size()};
  Problem prob(optimization::SolverOptions().device, PNEC_HIP_MODE_TARGET, offsets);
  Check(pnec_hip_problem_fill(prob.p, 0, 1, bvs_1[0].data(), bvs_2[0].data(), covs[0].data(), nullptr, PNEC_HIP_MEM_HOST,
                              nullptr));
  const Quaterniond q(camera_pose.rotationMatrix());
  int32_t status = PNEC_HIP_SENS_SINGULAR;
  // (symmetric: the ABI's row-major 3x3 is the column-major one)
  Check(pnec_hip_pose_sensitivity(prob.p, q.coeffs(), camera_pose.translation().data(), grad_pose.data(), 1, regularization,
                                  0, out.grad_bvs_1[0].data(), out.grad_bvs_2[0].data(), out.grad_covs[0].data(), nullptr,
                                  out.lambda.data(), nullptr, nullptr, out.newton.data(), &status, PNEC_HIP_MEM_HOST,
                                  nullptr));
  out.status = status;
  return out;
}

}  // namespace rel_pose_estimation

namespace odometry {
namespace {
// rows of the C ABI from poses: xyzw of the rotation (Shepperd, as Eigen) and the translation
void PoseRows(const std::vector<SE3d> &poses, std::vector<double> &q, std::vector<double> &p) {
  q.resize(4 * poses.size());
  p.resize(3 * poses.size());
  for (size_t i = 0; i < poses.size(); ++i) {
    const Quaterniond r = poses[i].unit_quaternion();
    for (int k = 0; k < 4; ++k) q[4 * i + (size_t)k] = r.coeffs()[k];
    for (int k = 0; k < 3; ++k) p[3 * i + (size_t)k] = poses[i].translation()[k];
  }
}
}  // namespace

std::vector<SE3d> ComposeTrajectory(const std::vector<SE3d> &relative_poses, const SE3d &correction,
                                    std::vector<uint8_t> *valid) {
  const size_t n = relative_poses.size();
  std::vector<SE3d> out(n);
  if (valid) valid->assign(n, 0);
  if (n == 0) return out;
  std::vector<double> q, t, q0, p0, out_q(4 * n), out_p(3 * n);
  std::vector<uint8_t> present(n);
  PoseRows(relative_poses, q, t);
  PoseRows({correction}, q0, p0);
  const int64_t offsets[2] = {0, (int64_t)n};
  Check(pnec_hip_trajectory_compose(optimization::SolverOptions().device, 1, offsets, (int64_t)n, q.data(), t.data(), nullptr,
                                    q0.data(), p0.data(), out_q.data(), out_p.data(), present.data(), PNEC_HIP_MEM_HOST,
                                    nullptr));
  for (size_t i = 0; i < n; ++i) {
    const double *r = &out_q[4 * i];
    Vector3d p;
    for (int k = 0; k < 3; ++k) p[k] = out_p[3 * i + (size_t)k];
    out[i] = SE3d(Quaterniond(r[3], r[0], r[1], r[2]), p);
  }
  if (valid) *valid = present;
  return out;
}

TrajectoryScore TrajectoryMetrics(const std::vector<SE3d> &estimated, const std::vector<SE3d> &ground_truth) {
  if (estimated.size() != ground_truth.size())
    throw std::invalid_argument("TrajectoryMetrics: estimated and ground_truth differ in size (match the frames first)");
  const size_t n = estimated.size();
  const double nan = std::numeric_limits<double>::quiet_NaN();
  TrajectoryScore s{nan, nan, nan, nan, nan, std::vector<double>(n), std::vector<double>(n), std::vector<double>(n),
                    std::vector<double>(n)};
  if (n == 0) return s;
  std::vector<double> eq, ep, gq, gp, err_q(4 * n);
  PoseRows(estimated, eq, ep);
  PoseRows(ground_truth, gq, gp);
  const int64_t offsets[2] = {0, (int64_t)n};
  double m[5];
  Check(pnec_hip_trajectory_metrics(optimization::SolverOptions().device, 1, offsets, (int64_t)n, eq.data(), gq.data(),
                                    ep.data(), gp.data(), m, err_q.data(), s.rmse_d.data(), s.l1_d.data(), s.angle1.data(),
                                    s.rt1.data(), PNEC_HIP_MEM_HOST, nullptr));
  s.RPE_1 = m[0];
  s.RPE_n = m[1];
  s.L1RPE_1 = m[2];
  s.L1RPE_n = m[3];
  s.r_t = m[4];
  return s;
}

TrajectoryState::TrajectoryState(size_t n)
    : s(n, std::numeric_limits<double>::quiet_NaN()), q(4 * n, 0.0), p(3 * n, 0.0) {
  for (size_t i = 0; i < n; ++i) q[4 * i + 3] = 1.0;
}

std::vector<int32_t> AdvanceTrajectory(const TrajectoryState &state, const std::vector<double> &rel_q,
                                       const std::vector<double> &rel_t, TrajectoryState *next,
                                       const std::vector<int32_t> *count, int min_count, const std::vector<double> *scale3,
                                       const std::vector<int32_t> *n_used, int min_used) {
  const size_t n = state.s.size();
  if (!next || next == &state) throw std::invalid_argument("AdvanceTrajectory: next must be another object than state");
  if (state.q.size() != 4 * n || state.p.size() != 3 * n || rel_q.size() != 4 * n || rel_t.size() != 3 * n ||
      (count && count->size() != n) || (scale3 && scale3->size() != 3 * n) || (n_used && n_used->size() != n))
    throw std::invalid_argument("AdvanceTrajectory: every array holds one row per sequence of the state");
  next->s.resize(n);
  next->q.resize(4 * n);
  next->p.resize(3 * n);
  std::vector<int32_t> status(n);
  if (n == 0) return status;
  Check(pnec_hip_trajectory_advance(optimization::SolverOptions().device, (int64_t)n, rel_q.data(), rel_t.data(),
                                    count ? count->data() : nullptr, min_count, scale3 ? scale3->data() : nullptr,
                                    n_used ? n_used->data() : nullptr, min_used, state.s.data(), state.q.data(),
                                    state.p.data(), next->s.data(), next->q.data(), next->p.data(), status.data(),
                                    PNEC_HIP_MEM_HOST, nullptr));
  return status;
}

}  // namespace odometry
}  // namespace pnec
