// pnec_host.h -- host C++ facade: the reference's class / method names for the hot path, on top
// of the C ABI (include/pnec_hip.h).  No arithmetic of the optimisation lives here: every
// Optimize()/Solve() is a pnec_hip_* call that runs on the MI355X; there is NO CPU fallback (a
// missing device or library is a thrown std::runtime_error, loudly).
//
// Mirrors (reference file:line):
//   pnec::common::{NoiseFrame, SkewFromVector, AnglesFromVec, RotationalDifference,
//                  TranslationalDifference, CostFunction}      include/common/common.h:57-120
//   pnec::optimization::PNECCeres                               include/optimization/pnec_ceres.h:48-89
//   pnec::optimization::NECCeres                                include/optimization/nec_ceres.h:46-79
//   pnec::rel_pose_estimation::{Options, PNEC}                  include/rel_pose_estimation/pnec_config.h:46-65,
//                                                               include/rel_pose_estimation/pnec.h:48-114
// Batch entry points (SolveBatch / OptimizeBatch) are additions: the reference solves one pair per
// call; thousands of pairs per call is what the device is for.
#pragma once

#include <array>
#include <cstdint>
#include <ostream>
#include <stdexcept>
#include <string>
#include <vector>

#include "pnec_hip.h"
#include "pnec_types.h"

namespace pnec {
namespace common {

enum NoiseFrame { Host, Target, Both };  // common.h:60

Matrix3d SkewFromVector(const Vector3d &vector);                       // common.cc:96-101
void AnglesFromVec(const Vector3d &vector, double &theta, double &phi);  // common.cc:103-116
double RotationalDifference(const Matrix3d &rotation_1, const Matrix3d &rotation_2);  // common.cc:210-214 (deg)
double TranslationalDifference(const Vector3d &translation_1, const Vector3d &translation_2,
                               bool both_directions = true);           // common.cc:216-235 (deg)
// common.cc:127-136 (the loop starts at i = 1, as in the reference), :157-181, :183-208
Matrix3d ComposeM(const bearingVectors_t &bvs_1, const bearingVectors_t &bvs_2, const Matrix3d &rotation);
Vector3d TranslationFromM(const Matrix3d &M);
double Weight(const Vector3d &bearing_vector_1, const Vector3d &bearing_vector_2, const Vector3d &translation,
              const Matrix3d &rotation, const Matrix3d &covariance, double regularization, bool host_frame);
// common.cc:460-525, evaluated on the device (batch overload :527-550)
enum CameraModel { Omnidirectional, Pinhole };  // common.h:62
Vector3d Unproject(const double img_pt[2], const Matrix3d &K_inv);
Matrix3d UnscentedTransform(const Vector3d &mu, const Matrix3d &cov, const Matrix3d &K_inv, double kappa,
                            CameraModel camera_model);
std::vector<Matrix3d> UnscentedTransform(const std::vector<Vector3d> &mus, const std::vector<Matrix3d> &covs,
                                         const Matrix3d &K_inv, double kappa, CameraModel camera_model);

// common.cc:67-93: cv::undistortPoints with the camera's K, dist_coef and P = K, evaluated on the device
// (pnec_hip_undistort_keypoints; include/pnec_hip.h has the definition).  The reference reads K and dist_coef from its
// Camera singleton; here they are arguments.  K: upper triangular, zero skew, last row (0, 0, 1); dist_coef: k1 k2 p1 p2
// and optionally k3 -- anything else throws std::invalid_argument.
// THE REFERENCE'S QUIRK, reproduced by both overloads: dist_coef[0] == 0.0 returns the input untouched (common.cc:74-76),
// whatever k2, p1 and p2 are.  The C ABI does not have it: there only all five coefficients zero mean "no distortion".
typedef std::array<double, 2> Vector2d;  // layout of Eigen::Vector2d
typedef std::array<double, 3> Covariance2d;  // (xx, xy, yy) of a 2x2 image covariance
struct UndistortOptions {
  bool newton = false;          // polish the five fixed-point steps by Newton steps on the forward model (not in the reference)
  bool propagate_cov = false;   // covs become A cov A' (not in the reference, which hands them on unchanged)
  int fixed_iterations = 5, newton_iterations = 20;
};
// fx fy cx cy k1 k2 p1 p2 k3 for the C ABI; throws as described above.  No device.
std::array<double, 9> UndistortCamera(const Matrix3d &K, const std::vector<double> &dist_coef);
Vector2d Undistort(const Vector2d &point, const Matrix3d &K, const std::vector<double> &dist_coef);
// points (and covs, when not NULL: one per point, else std::invalid_argument) are undistorted in place; returns one
// pnec_hip_undistort_status per point (all OK where the quirk above returns the input)
std::vector<uint8_t> Undistort(std::vector<Vector2d> &points, std::vector<Covariance2d> *covs, const Matrix3d &K,
                               const std::vector<double> &dist_coef, const UndistortOptions &options = UndistortOptions());

// include/common/timing.h:48-67: per-frame stage timers in milliseconds
struct FrameTiming {
  explicit FrameTiming(int id) : id_(id) {}
  static std::string TimingHeader() {
    return "ID FrameLoading FeatureCreation NEC-ES IT-ES AVG-IT-ES CERES OPTIMIZATION TOTAL";
  }
  int OptimizationTime() const { return (int)(nec_es_ + it_es_ + ceres_); }
  int TotalTime() const { return (int)(frame_loading_ + feature_creation_) + OptimizationTime(); }
  int id_;
  long frame_loading_ = 0, feature_creation_ = 0, nec_es_ = 0, it_es_ = 0, avg_it_es_ = 0, ceres_ = 0;  // ms
  // The same stage timers in MICROSECONDS (not in the reference: its millisecond counts were made for a solver that
  // takes tens of milliseconds per frame; here a whole PNEC::Solve is ~0.2 ms and every field above rounds to 0).
  // Filled by the timed PNEC::Solve overloads next to the millisecond fields; the row operator<< streams -- the
  // reference's timing.txt format -- does not show them, TimingRowUs() does.
  double nec_es_us_ = 0.0, it_es_us_ = 0.0, avg_it_es_us_ = 0.0, ceres_us_ = 0.0;
  double OptimizationTimeUs() const { return nec_es_us_ + it_es_us_ + ceres_us_; }
  // "id nec-es it-es avg-it-es ceres optimization", microseconds with one decimal
  std::string TimingRowUs() const;
  static std::string TimingHeaderUs() { return "ID NEC-ES[us] IT-ES[us] AVG-IT-ES[us] CERES[us] OPTIMIZATION[us]"; }
};
// src/common/timing.cc:49-58: one row of timing.txt -- "id loading features nec-es it-es avg-it-es ceres
// optimization total", blank separated.  Every field is an integral millisecond count there
// (std::chrono::milliseconds::count() and two int sums), so the std::scientific / setprecision(8) the
// reference sets on the stream never shows in a row: the fields print as plain integers.
std::ostream &operator<<(std::ostream &os, const FrameTiming &frame_timing);

// include/common/timing.h:69-80, src/common/timing.cc:60-66: the rows of a run; streams as the header line
// followed by one row per frame (what pnec_vo.cc:273-276 writes to <results>/timing.txt)
class Timing {
 public:
  void push_back(const FrameTiming &frame_timing) { frame_timings_.push_back(frame_timing); }
  size_t size() const { return frame_timings_.size(); }
  friend std::ostream &operator<<(std::ostream &os, const Timing &timing);
  // pnec_vo.cc:273-276: open <path> truncating, stream the table; false if the file cannot be written
  bool Save(const std::string &path) const;

 private:
  std::vector<FrameTiming> frame_timings_;
};
std::ostream &operator<<(std::ostream &os, const Timing &timing);

// common.cc:237-259, evaluated on the device
double CostFunction(const bearingVectors_t &bvs_1, const bearingVectors_t &bvs_2,
                    const std::vector<Matrix3d> &covs, const SE3d &camera_pose);

// Addition (the reference has no such function): the 6x6 covariance of camera_pose given the correspondences --
// pnec_hip_pose_covariance for one pair, include/pnec_hip.h has the conventions: rows / columns (omega_x, omega_y,
// omega_z, t_x, t_y, t_z), omega the rotation vector of a LEFT perturbation R <- Exp(omega) R in radians, t the unit
// translation direction (rank 5: the length of t is not observable).  The inverse of the Gauss-Newton information of
// the PNEC residual (pnec_residual.h:50-150, target-frame covariances) at the pose; what ceres::Covariance would
// give for PNECCeres' problem.  Fewer than 5 correspondences or a singular information matrix: all NaN.
Matrix6d PoseCovariance(const bearingVectors_t &bvs_1, const bearingVectors_t &bvs_2, const std::vector<Matrix3d> &covs,
                        const SE3d &camera_pose, double regularization = 1e-13);
// the symmetric residual (pnec_residual.h:111-150): covariances of both frames
Matrix6d PoseCovariance(const bearingVectors_t &bvs_1, const bearingVectors_t &bvs_2, const std::vector<Matrix3d> &covs_1,
                        const std::vector<Matrix3d> &covs_2, const SE3d &camera_pose, double regularization = 1e-13);

// Addition (the reference returns a pose and no per-correspondence verdict): the whitened PNEC residual of every
// correspondence at camera_pose -- pnec_hip_residuals for one pair; what ceres::Problem::Evaluate would return per
// residual block for PNECCeres' problem.  Under the model each is N(0, 1).
std::vector<double> Residuals(const bearingVectors_t &bvs_1, const bearingVectors_t &bvs_2,
                              const std::vector<Matrix3d> &covs, const SE3d &camera_pose, double regularization = 1e-13);
// the symmetric residual: covariances of both frames
std::vector<double> Residuals(const bearingVectors_t &bvs_1, const bearingVectors_t &bvs_2,
                              const std::vector<Matrix3d> &covs_1, const std::vector<Matrix3d> &covs_2,
                              const SE3d &camera_pose, double regularization = 1e-13);
// The indices of the correspondences within `gate` sigmas of camera_pose (|residual| <= gate), in the shape of the
// `inliers` vector PNEC::Solve fills.  It classifies at a pose that is already near the truth (PNEC::Solve's result);
// it is not a robust estimator.
std::vector<int> GateInliers(const bearingVectors_t &bvs_1, const bearingVectors_t &bvs_2,
                             const std::vector<Matrix3d> &covs, const SE3d &camera_pose, double gate = 3.0,
                             double regularization = 1e-13);
std::vector<int> GateInliers(const bearingVectors_t &bvs_1, const bearingVectors_t &bvs_2,
                             const std::vector<Matrix3d> &covs_1, const std::vector<Matrix3d> &covs_2,
                             const SE3d &camera_pose, double gate = 3.0, double regularization = 1e-13);

// Addition (the reference scores a translation with TranslationalDifference(..., both_directions = true) and never
// decides between t and -t): midpoint triangulation of every correspondence at camera_pose AS GIVEN --
// pnec_hip_triangulate for one pair without PNEC_HIP_TRI_ORIENT, include/pnec_hip.h has the definitions.  Returns the
// points in frame 1; lengths are in units of the baseline (the translation is used as a direction).  depths_1 along
// bvs_1 from camera 1, depths_2 along R bvs_2 from camera 2, front[i] = 1 iff both depths are positive.  Parallel rays:
// depths +inf, point NaN, front 0.
std::vector<Vector3d> Triangulate(const bearingVectors_t &bvs_1, const bearingVectors_t &bvs_2, const SE3d &camera_pose,
                                  std::vector<double> *depths_1 = nullptr, std::vector<double> *depths_2 = nullptr,
                                  std::vector<uint8_t> *front = nullptr);
// camera_pose with its translation multiplied by the cheirality vote's sign: -1 if more correspondences triangulate
// behind both cameras than in front of both, else +1 (a tie, no correspondences included).  Rotation and the
// translation's magnitude are untouched.
SE3d OrientTranslation(const bearingVectors_t &bvs_1, const bearingVectors_t &bvs_2, const SE3d &camera_pose);

// Addition (every pose of the reference carries its translation as a direction; nothing in it relates the baseline of one
// frame pair to the next): the length of camera_pose's baseline in units of pose_prev's, from the tracks the two pairs
// share -- pnec_hip_relative_scale for one frame, include/pnec_hip.h has the definitions.  (bvs_prev_1, bvs_prev_2,
// pose_prev) is the previous pair, whose SECOND camera is the first camera of (bvs_1, bvs_2, camera_pose); link[i] is
// the index in the previous pair of the track of current correspondence i, -1 if it is not there.  Both translations
// must carry the sign that puts the structure in front (OrientTranslation).  Returns the lower median of the used links'
// ratios (NaN if none is used); q25 / q75 its lower / upper quartile, n_used the number of links used, ratios the
// per-correspondence values (NaN where not used).  min_parallax (radians) leaves out links of smaller parallax.
double RelativeScale(const bearingVectors_t &bvs_prev_1, const bearingVectors_t &bvs_prev_2, const SE3d &pose_prev,
                     const bearingVectors_t &bvs_1, const bearingVectors_t &bvs_2, const SE3d &camera_pose,
                     const std::vector<int> &link, double min_parallax = 0.0, double *q25 = nullptr,
                     double *q75 = nullptr, int *n_used = nullptr, std::vector<double> *ratios = nullptr);

}  // namespace common

// Addition (the reference computes these inside its KLT tracker, in float: POpticalFlowPatch::setFromImage,
// include/features/tracking/pnec_patch.h:78-137, scaled and rotated by KLTPatchOpticalFlow; basalt's image.h /
// patterns.h are not in its tree [EXT]): the 2x2 image covariance of keypoints from the patches around them --
// pnec_hip_patch_covariance for one image, in double, include/pnec_hip.h has the definitions.  No tracking happens here.
namespace features {
// basalt's Pattern52: 52 offsets (x, y) in pixels, 0.5 * the raw integer pattern, rows from y = 3.5 down to -3.5
const std::vector<std::array<double, 2>> &Pattern52();
// One image of height x width pixels (`pitch` elements per row, 0 = width) of pixel_type, keypoints (x = column, y = row).
// Returns (xx, xy, yy) per keypoint, what KeyPoint::img_covariance_ holds; NaN where status is not PNEC_HIP_PATCH_OK
// (PNEC_HIP_PATCH_EMPTY: no pattern point inside the image or a patch without intensity; PNEC_HIP_PATCH_SINGULAR: a
// constant patch or a ramp).  scaling is the reference's uncertainty_scaling; angles (one per keypoint, radians) rotate
// the covariance as the tracked transform does.
std::vector<std::array<double, 3>> PatchCovariances(const void *image, pnec_hip_pixel_type pixel_type, int height,
                                                    int width, int64_t pitch,
                                                    const std::vector<std::array<double, 2>> &points,
                                                    double scaling = 10.0, const std::vector<double> *angles = nullptr,
                                                    std::vector<int> *status = nullptr,
                                                    const std::vector<std::array<double, 2>> *pattern = nullptr);

// Addition: the tracker itself -- KLTPatchOpticalFlow::trackPoints / trackPoint / trackPointAtLevel
// (klt_patch_optical_flow.h:195-342) and POpticalFlowPatch::residual (pnec_patch.h:139-170) on basalt's image pyramid
// [EXT] -- for one image pair, in double: pnec_hip_image_pyramid_level and pnec_hip_patch_track, include/pnec_hip.h has
// the definitions.  Detection is DetectKeypoints, ids and bookkeeping RetainTracks / AppendTracks; the view graph is the
// caller's.
struct Pyramid {
  pnec_hip_pixel_type pixel_type = PNEC_HIP_PIXEL_U8;
  int height = 0, width = 0;                  // of level 0; level l is (height >> l) x (width >> l), rows packed
  std::vector<std::vector<unsigned char>> levels;
};
// `levels` levels (1 .. PNEC_HIP_TRACK_MAX_LEVELS) of one image (`pitch` elements per row, 0 = width); level 0 is a copy
Pyramid ImagePyramid(const void *image, pnec_hip_pixel_type pixel_type, int height, int width, int64_t pitch, int levels);
struct TrackOptions {
  int max_iterations = 40;                    // per level (optical_flow_max_iterations)
  double max_recovered_dist2 = 0.04;          // optical_flow_max_recovered_dist2
  bool backward = true;                       // the forward-backward check
  double scaling = 10.0;                      // uncertainty_scaling
  std::array<double, 2> shift = {0.0, 0.0};   // the reference's `offset`
};
struct PatchTracks {
  std::vector<std::array<double, 2>> points;        // the tracked translations in `next`
  std::vector<double> angles;                       // the tracked rotations: PatchCovariances' `angles`
  std::vector<std::array<double, 3>> covariances;   // (xx, xy, yy); NaN unless status is PNEC_HIP_TRACK_OK
  std::vector<double> dist2;
  std::vector<int> status, lost_level;              // pnec_hip_track_status; the level of a loss or -1
};
// Tracks the patches built at `points` in `tmpl` into `next` and back into `prev` (nullptr: tmpl); init_points /
// init_angles are the transform in prev (nullptr: points / 0).
PatchTracks TrackPatches(const Pyramid &tmpl, const Pyramid &next, const std::vector<std::array<double, 2>> &points,
                         const TrackOptions &options = TrackOptions(), const Pyramid *prev = nullptr,
                         const std::vector<std::array<double, 2>> *init_points = nullptr,
                         const std::vector<double> *init_angles = nullptr,
                         const std::vector<std::array<double, 2>> *pattern = nullptr);

// Addition: the detector that feeds the tracker -- what KLTPatchOpticalFlow::addPoints (klt_patch_optical_flow.h:344-385)
// gets from basalt's detectKeypoints [EXT]: grid FAST-9 corners of one uint8 / uint16 image, integer arithmetic --
// pnec_hip_detect_keypoints, include/pnec_hip.h has the definition.  Keypoint ids and the track bookkeeping: RetainTracks /
// AppendTracks below.
struct DetectOptions {
  int grid = 30;                              // optical_flow_detection_grid_size (8 .. 64)
  int points_per_cell = 1;                    // 1 .. 4; the reference passes 1
  int min_threshold = 5;                      // the last threshold of the reference's loop
  int edge = 19;                              // EDGE_THRESHOLD
};
struct Keypoints {
  std::vector<std::array<double, 2>> points;  // x, y: what TrackPatches takes as `points`
  std::vector<int> score, cell_index;         // cv::FAST's score (m - 1) and the cell cx * ny + cy, per point
  std::vector<int> cell;                      // per cell: points produced, -1 for a cell a current point occupies
  int nx = 0, ny = 0;
};
// `current` (nullptr: none): the points already tracked in this image; their cells are not searched
Keypoints DetectKeypoints(const void *image, pnec_hip_pixel_type pixel_type, int height, int width, int64_t pitch,
                          const DetectOptions &options = DetectOptions(),
                          const std::vector<std::array<double, 2>> *current = nullptr);

// Addition: the bookkeeping of KLTPatchOpticalFlow::processFrame (klt_patch_optical_flow.h:121-191) for one image --
// pnec_hip_tracks_retain, pnec_hip_tracks_append and pnec_hip_patch_track_indexed, include/pnec_hip.h has the definitions.
// A track keeps the image it was born in as its template (tmpl_image: an index into a stack of pyramids the caller
// keeps).  DEVIATION when that stack is a ring: the reference keeps a patch for ever, a ring of R frames retires a track
// when its age would reach R - 1 (max_age = R - 2), which costs the pair that track's correspondence on that step.
struct Tracks {
  std::vector<int64_t> id;                          // unique, >= 0
  std::vector<int> tmpl_image, age;                 // the birth image in the caller's stack; frames since birth
  std::vector<std::array<double, 2>> tmpl_points;   // where the patch was built
  std::vector<std::array<double, 2>> points;        // the transform in the set's frame
  std::vector<double> angles;
  std::vector<std::array<double, 3>> covariances;   // (xx, xy, yy); empty: none
  // a retained set: the same track in the set it was retained from -- (prev_points, points, covariances) are the
  // correspondences of the pair -- and the row it had there
  std::vector<std::array<double, 2>> prev_points;
  std::vector<std::array<double, 3>> prev_covariances;
  std::vector<int64_t> src;
};
// the tracks of `tracks` that `result` (TrackPatches' output for its rows) brought back with PNEC_HIP_TRACK_OK and, with
// max_age > 0, whose age + 1 stays <= max_age: in their order, age + 1, the tracked transform and covariance
Tracks RetainTracks(const Tracks &tracks, const PatchTracks &result, int max_age = 0);
// `tracks` (nullptr: none yet) cut to `capacity` rows and refilled with as many of `detections` as still fit: ids from
// *next_id (advanced), tmpl_image, age 0, identity transform, det_covariances (nullptr: NaN).  *dropped: what did not fit.
Tracks AppendTracks(const Tracks *tracks, const Keypoints &detections,
                    const std::vector<std::array<double, 3>> *det_covariances, int tmpl_image, int64_t capacity,
                    int64_t *next_id, int64_t *dropped = nullptr);
// The indexed form of TrackPatches: keypoint k builds its templates in pyramid tmpl_image[k] of `tmpl_stack` (all of one
// size and pixel type) and is tracked from `prev` (where init_points / init_angles hold) into `next` and back.
PatchTracks TrackPatches(const std::vector<const Pyramid *> &tmpl_stack, const std::vector<int> &tmpl_image,
                         const Pyramid &prev, const Pyramid &next, const std::vector<std::array<double, 2>> &tmpl_points,
                         const TrackOptions &options = TrackOptions(),
                         const std::vector<std::array<double, 2>> *init_points = nullptr,
                         const std::vector<double> *init_angles = nullptr,
                         const std::vector<std::array<double, 2>> *pattern = nullptr);
// Addition: the join of two track sets of one image on their ids (pnec_hip_tracks_link): for every id of `cur_ids` the
// row of the same id in `prev_ids`, -1 where there is none or the id is negative -- the `link` a relative scale between
// the two pairs takes.  prev_ids must ascend strictly, as the ids RetainTracks / AppendTracks produce do.
std::vector<int32_t> LinkTracks(const std::vector<int64_t> &prev_ids, const std::vector<int64_t> &cur_ids);
}  // namespace features

namespace optimization {

// The ceres::Solver::Options fields this path honours (Ceres 2.x defaults).
struct SolverOptions {
  int max_num_iterations = 50;
  double function_tolerance = 1e-6;
  double gradient_tolerance = 1e-10;
  double parameter_tolerance = 1e-8;
  double initial_trust_region_radius = 1e4;
  double max_trust_region_radius = 1e16;
  double min_trust_region_radius = 1e-32;
  double min_relative_decrease = 1e-3;
  double min_lm_diagonal = 1e-6;
  double max_lm_diagonal = 1e32;
  bool jacobi_scaling = true;
  int max_num_consecutive_invalid_steps = 5;
  int device = 0;  // which GPU
  pnec_hip_options ToHip() const;
};

// What ceres::Solver::Summary would have told (the reference stores it and never reads it).
struct Summary {
  double final_cost = 0.0;  // 1/2 sum r^2
  int iterations = 0;
  int termination = PNEC_HIP_TERM_MAX_ITERATIONS;  // pnec_hip_termination
};

class PNECCeres {
 public:
  PNECCeres();
  PNECCeres(const SE3d &init, const SolverOptions &options = SolverOptions());
  PNECCeres(const Quaterniond &orientation, double theta, double phi,
            const SolverOptions &options = SolverOptions());
  PNECCeres(const Quaterniond &orientation, const Vector3d &translation,
            const SolverOptions &options = SolverOptions());
  ~PNECCeres();

  void Optimize(const std::vector<Vector3d> &bvs_1, const std::vector<Vector3d> &bvs_2,
                const std::vector<Matrix3d> &covs, double regularization,
                common::NoiseFrame noise_frame = common::Target);
  void Optimize(const std::vector<Vector3d> &bvs_1, const std::vector<Vector3d> &bvs_2,
                const std::vector<Matrix3d> &covs_1, const std::vector<Matrix3d> &covs_2,
                double regularization);

  void InitValues(const Quaterniond orientation, double theta, double phi);
  void InitValues(const SE3d &init);
  void InitValues(const Quaterniond &orientation, const Vector3d &translation);
  void SetOptions(const SolverOptions &options);

  Matrix3d Orientation() const;
  Vector3d Translation() const;
  SE3d Result() const;
  const Summary &summary() const { return summary_; }

 private:
  void Run(int mode, const std::vector<Vector3d> &b1, const std::vector<Vector3d> &b2,
           const std::vector<Matrix3d> *covs, const std::vector<Matrix3d> *covs_host, double reg);
  Quaterniond orientation_;
  double theta_, phi_;
  SolverOptions options_;
  Summary summary_;
};

class NECCeres {
 public:
  NECCeres();
  NECCeres(const SE3d &init, const SolverOptions &options = SolverOptions());
  NECCeres(const Quaterniond &orientation, double theta, double phi,
           const SolverOptions &options = SolverOptions());
  NECCeres(const Quaterniond &orientation, const Vector3d &translation,
           const SolverOptions &options = SolverOptions());
  ~NECCeres();

  void Optimize(const std::vector<Vector3d> &bvs_1, const std::vector<Vector3d> &bvs_2);
  void InitValues(const Quaterniond orientation, double theta, double phi);
  void InitValues(const SE3d &init);
  void InitValues(const Quaterniond &orientation, const Vector3d &translation);
  void SetOptions(const SolverOptions &options);
  Matrix3d Orientation() const;
  Vector3d Translation() const;
  SE3d Result() const;
  const Summary &summary() const { return summary_; }

 private:
  Quaterniond orientation_;
  double theta_, phi_;
  SolverOptions options_;
  Summary summary_;
};

}  // namespace optimization

namespace rel_pose_estimation {

struct Options {  // pnec_config.h:46-65, same names and defaults
  bool use_nec_ = false;
  common::NoiseFrame noise_frame_ = common::Target;
  double regularization_ = 1.0e-13;
  size_t weighted_iterations_ = 10;
  bool use_scf_ = true;
  bool use_ceres_ = true;
  optimization::SolverOptions ceres_options_ = optimization::SolverOptions();
  bool use_ransac_ = true;
  int max_ransac_iterations_ = 5000;
  int ransac_sample_size_ = 10;
  int min_matches_ = 30;
  int min_inliers_ = 10;
  int min_matches_further_ = 20;
  // NOT in the reference: which iteration stands in for opengv::relative_pose::eigensolver's eigenvalue minimisation
  // (pnec.cc:239-258,274,315; opengv is not in the reference tree) -- pnec_hip_eigensolver_scheme in include/pnec_hip.h:
  // 0 damped Newton, 1 normalised descent [EXT], 2 Eigen's Levenberg-Marquardt on the reduced-Cayley gradient [EXT].
  // This facade stands in for the reference's classes, so it defaults to the restatement believed to be what opengv runs
  // (2; 1.8x the cost of 0 on the whole chain) -- the C ABI's own default is 0.  INTEGRATION.md 6 has the evidence.
  int eigensolver_scheme_ = 2;
  // NOT in the reference either: opengv's RANSAC starts hypothesis h + 1 from the last model it SCORED (a side effect of
  // EigensolverSacProblem::getSelectedDistancesToModel on the adapter [EXT, recalled]) -- PNEC_HIP_RANSAC_CHAINED_STARTS.
  // Off: a round's sixteen hypotheses run side by side from the initial rotation (inside the noise of opengv's rand());
  // on: one hypothesis per round, ~3x the RANSAC stage.
  bool ransac_chained_starts_ = false;
};

// One frame pair of a batch, in the reference's argument shapes.
struct FramePair {
  bearingVectors_t bvs1, bvs2;
  std::vector<Matrix3d> projected_covs;
  SE3d initial_pose;
};

class PNEC {
 public:
  PNEC() {}
  explicit PNEC(const Options &options);
  ~PNEC();

  // pnec.cc:69-124: NEC eigensolver (+ RANSAC, inlier extraction) -> weighted eigensolver + SCF ->
  // least-squares refinement, every stage on the device, driven by the same Options fields the
  // reference reads.  RANSAC draws come from a counter-based hash (seed 1), not rand().
  SE3d Solve(const bearingVectors_t &bvs1, const bearingVectors_t &bvs2,
             const std::vector<Matrix3d> &projected_covs, const SE3d &initial_pose);
  SE3d Solve(const bearingVectors_t &bvs1, const bearingVectors_t &bvs2,
             const std::vector<Matrix3d> &projected_covs, const SE3d &initial_pose,
             std::vector<int> &inliers);
  // the timed twins (pnec.cc:126-208): same result, stage times filled in
  SE3d Solve(const bearingVectors_t &bvs1, const bearingVectors_t &bvs2,
             const std::vector<Matrix3d> &projected_covs, const SE3d &initial_pose,
             common::FrameTiming &timing);
  SE3d Solve(const bearingVectors_t &bvs1, const bearingVectors_t &bvs2,
             const std::vector<Matrix3d> &projected_covs, const SE3d &initial_pose,
             std::vector<int> &inliers, common::FrameTiming &timing);

  SE3d Eigensolver(const bearingVectors_t &bvs1, const bearingVectors_t &bvs2,
                   const SE3d &initial_pose, std::vector<int> &inliers);          // pnec.cc:231-281
  SE3d WeightedEigensolver(const bearingVectors_t &bvs1, const bearingVectors_t &bvs2,
                           const std::vector<Matrix3d> &projected_covariances,
                           const SE3d &initial_pose);                            // pnec.cc:283-348
  SE3d CeresSolver(const bearingVectors_t &bvs1, const bearingVectors_t &bvs2,
                   const std::vector<Matrix3d> &projected_covariances,
                   const SE3d &initial_pose);                                    // pnec.cc:350-370
  SE3d CeresSolverFull(const bearingVectors_t &bvs1, const bearingVectors_t &bvs2,
                       const std::vector<Matrix3d> &projected_covariances, double regularization,
                       const SE3d &initial_pose);                                // pnec.cc:372-392
  SE3d NECCeresSolver(const bearingVectors_t &bvs1, const bearingVectors_t &bvs2,
                      const SE3d &initial_pose);                                 // pnec.cc:394-411

  // Addition: Solve() for many frame pairs at once (ragged sizes allowed) -- every stage is one
  // launch over the whole batch, which is where the device earns its keep.  Same Options handling
  // and the same per-pair results as calling Solve() pair by pair (RANSAC draws are a function of
  // the pair's index in the batch: pair i of a batch reproduces Solve() only for i = 0).
  std::vector<SE3d> SolveBatch(const std::vector<FramePair> &pairs,
                               std::vector<std::vector<int>> *inliers = nullptr);
  // Addition: the same over several GPUs of the node from this one process (the reference fans out by process:
  // scripts/parallel_kitti.sh:60-69).  `devices` lists the GPUs (a device may appear twice); the pairs are split
  // into contiguous ranges balanced by correspondence count, one host thread + batch + stream per entry
  // (pnec_hip_solve_pipeline_multi).  Same results as the single-device call whatever the list.
  std::vector<SE3d> SolveBatch(const std::vector<FramePair> &pairs, const std::vector<int> &devices,
                               std::vector<std::vector<int>> *inliers = nullptr);
  // Addition: CeresSolver for many pairs in one device launch (ragged sizes allowed).
  std::vector<SE3d> CeresSolverBatch(const std::vector<FramePair> &pairs,
                                     std::vector<optimization::Summary> *summaries = nullptr);
  // Addition: ... over several GPUs of the node from this one process -- the path the benchmark shards (independent frame
  // pairs, no data-path exchange) -- through the persistent multi-device handle (pnec_hip_multi_*): the handle lives in
  // this object and is reused while the device list and the shapes fit, so a loop of calls allocates nothing.
  std::vector<SE3d> CeresSolverBatch(const std::vector<FramePair> &pairs, const std::vector<int> &devices,
                                     std::vector<optimization::Summary> *summaries = nullptr);
  PNEC(const PNEC &o) : options_(o.options_) {}   // (the cached device handle is not shared: a copy makes its own)
  PNEC &operator=(const PNEC &o) { options_ = o.options_; return *this; }

 private:
  SE3d SolveImpl(const bearingVectors_t &bvs1, const bearingVectors_t &bvs2,
                 const std::vector<Matrix3d> &projected_covs, const SE3d &initial_pose,
                 std::vector<int> &inliers, common::FrameTiming *timing);
  Options options_;
  // CeresSolverBatch(pairs, devices): the cached multi-device handle and what it was made for
  struct pnec_hip_multi *multi_ = nullptr;
  std::vector<int> multi_devices_;
  int64_t multi_pairs_ = 0, multi_corr_ = 0, multi_pair_corr_ = 0;
};

// essential_matrix_methods.h: the closed-form baselines of `run_simulation -e`.  algorithm_t stands in for
// opengv::sac_problems::relative_pose::CentralRelativePoseSacProblem::algorithm_t (same names, same order).
enum algorithm_t { STEWENIUS = 0, NISTER = 1, SEVENPT = 2, EIGHTPT = 3 };
// EMPoseEstimation (essential_matrix_methods.cc:45-126).  Built: EIGHTPT with ransac == false -- opengv's eightpt and
// PoseFromEssentialMatrix (common.cc:262-457) on the device, pnec_hip_eight_point.  The rotation takes frame-2 vectors
// into frame 1; the translation has the length of E's largest singular value, as the reference's has.  Returns
// initial_pose when the call finds no pose (fewer than 8 correspondences, a non-finite bearing, no candidate), as
// essential_matrix_methods.cc:118-124 does.  Every other combination (STEWENIUS, NISTER, SEVENPT, or ransac == true:
// opengv's CentralRelativePoseSacProblem) throws std::invalid_argument naming what is not built.
SE3d EMPoseEstimation(const bearingVectors_t &bvs1, const bearingVectors_t &bvs2, const SE3d &initial_pose,
                      algorithm_t algorithm, bool ransac = true);
// The minimal baselines without RANSAC, under a name of their own (EMPoseEstimation keeps throwing for them): NISTER is
// opengv's fivept_nister, SEVENPT its sevenpt, each followed by PoseFromEssentialMatrix over every solution, on the
// device -- pnec_hip_essential_minimal.  Rotation, translation (of length s0 of the chosen solution) and the return of
// initial_pose where the call finds no pose as EMPoseEstimation; any other algorithm throws std::invalid_argument.
SE3d MinimalEMPoseEstimation(const bearingVectors_t &bvs1, const bearingVectors_t &bvs2, const SE3d &initial_pose,
                             algorithm_t algorithm);
// The RANSAC forms, again under a name of their own (EMPoseEstimation(..., ransac = true) keeps throwing): the
// ransac == true branch of essential_matrix_methods.cc:56-75 for NISTER, SEVENPT and EIGHTPT on the device --
// pnec_hip_essential_ransac, opengv's CentralRelativePoseSacProblem and Ransac restated, its rand() a hash of `seed`.
// max_iterations and threshold default to the reference's.  `inliers`, when given, receives the indices of the best
// model's inliers in ascending order.  Rotation and translation (of length s0 of the chosen solution) as above;
// initial_pose (and no inliers) where the call finds no model or has fewer correspondences than a sample.  STEWENIUS
// throws std::invalid_argument saying that it is not built.
SE3d RansacEMPoseEstimation(const bearingVectors_t &bvs1, const bearingVectors_t &bvs2, const SE3d &initial_pose,
                            algorithm_t algorithm, std::vector<int> *inliers = nullptr, int max_iterations = 5000,
                            double threshold = 1e-6, uint64_t seed = 1);

// Addition (the reference only dumps training data for learned covariances, src/uncertainty_extraction.cc; the gradient
// itself it leaves to other code): the gradient of a loss of the refined pose with respect to every bearing vector and
// covariance -- pnec_hip_pose_sensitivity for one pair of the PNEC residual (target-frame covariances), include/pnec_hip.h
// has the definitions.  grad_pose = (dL/d omega [3], dL/d t [3]) at camera_pose, omega the rotation vector of a LEFT
// perturbation.  status is a pnec_hip_sens_status: when it is not PNEC_HIP_SENS_OK (fewer than 5 correspondences, or
// camera_pose is not a minimiser: the Hessian there is not positive definite) every gradient is NaN.
struct PoseSensitivityResult {
  std::vector<Vector3d> grad_bvs_1, grad_bvs_2;
  std::vector<Matrix3d> grad_covs;    // symmetric: dL = sum_jk G_jk dS_jk
  std::array<double, 5> lambda{}, newton{};   // in the chart (tau_1, tau_2, omega); newton: the step to the minimiser
  int status = PNEC_HIP_SENS_SINGULAR;
};
PoseSensitivityResult PoseSensitivity(const bearingVectors_t &bvs_1, const bearingVectors_t &bvs_2,
                                      const std::vector<Matrix3d> &covs, const SE3d &camera_pose,
                                      const std::array<double, 6> &grad_pose, double regularization = 1e-13);

}  // namespace rel_pose_estimation

namespace odometry {

// Trajectory evaluation on the device over HOST space (pnec_hip_trajectory_compose, pnec_hip_trajectory_metrics;
// include/pnec_hip.h has the definitions), one sequence per call.
// ComposeTrajectory is scripts/pnec/visual_odometry/io/evaluate_run.py:118-129: poses[i] = poses[i-1] * poses[i], the first
// relative pose being a pose itself, then correction * pose for every pose.  A relative pose that is not finite is an
// identity step: the pose before it is carried, and `valid` (when not NULL: one byte per pose) says 0 there.
std::vector<SE3d> ComposeTrajectory(const std::vector<SE3d> &relative_poses, const SE3d &correction = SE3d(),
                                    std::vector<uint8_t> *valid = nullptr);
// The five numbers of the reference's metrics.yaml (scripts/pnec/metrics), in RADIANS, and what they are made of.  The
// two vectors hold matched frames and have one size, else std::invalid_argument.  Fewer than two frames: NaN.
// DEVIATION: an exact estimate scores 0 (the reference: NaN).
struct TrajectoryScore {
  double RPE_1, RPE_n, L1RPE_1, L1RPE_n, r_t;
  std::vector<double> rmse_d, l1_d;   // [d]: the RMSE / the mean of the angle over all pairs at distance d; [0] is 0
  std::vector<double> angle1, rt1;    // [k]: rotation / translation error of the step k-1 -> k; [0] is 0
};
TrajectoryScore TrajectoryMetrics(const std::vector<SE3d> &estimated, const std::vector<SE3d> &ground_truth);

// Addition: the online form (pnec_hip_trajectory_advance): a running scale and pose per sequence, one frame's step a call.
// s [n]: the last pair's baseline in units of the first pair's (NaN: no pair yet); q [n,4] xyzw and p [n,3]: the pose
// of the last frame.
struct TrajectoryState {
  std::vector<double> s, q, p;
  explicit TrajectoryState(size_t n = 0);   // fresh: s = NaN, q = (0, 0, 0, 1), p = 0
};
// One step for the n sequences of `state`: rel_q [n,4] xyzw, rel_t [n,3] (the oriented direction); count / min_count: the
// pair's correspondences and the least that make a pose; scale3 [n,3] / n_used [n] / min_used: the three quantiles of the
// baseline ratios (the median, entry 1, is read), the links behind them and the least that make a measurement.  nullptr:
// not given.  Writes *next (another object than `state`) and returns the statuses, PNEC_HIP_TRAJ_* [n].
std::vector<int32_t> AdvanceTrajectory(const TrajectoryState &state, const std::vector<double> &rel_q,
                                       const std::vector<double> &rel_t, TrajectoryState *next,
                                       const std::vector<int32_t> *count = nullptr, int min_count = 0,
                                       const std::vector<double> *scale3 = nullptr,
                                       const std::vector<int32_t> *n_used = nullptr, int min_used = 1);

}  // namespace odometry

// thrown when the HIP side reports an error (no device, bad argument, launch failure)
struct HipError : std::runtime_error {
  int code;
  HipError(int c, const std::string &what) : std::runtime_error(what), code(c) {}
};

}  // namespace pnec
