/*
 * pnec_hip.h -- C ABI of the MI355X-native PNEC pose solver (libpnec_hip.so).
 *
 * This is the drop-in boundary for the reference's rel_pose_estimation + optimization hot path.
 * The reference has no FFI layer; its seams are C++ classes and one pybind module.  Every entry
 * point below names the reference interface it replaces (paths relative to the reference repo):
 *
 *   reference seam                                              replaced by
 *   ----------------------------------------------------------  ---------------------------------
 *   PNECCeres::Optimize(bvs1,bvs2,covs,reg,frame)               pnec_hip_problem_create/upload +
 *     src/optimization/pnec_ceres.cc:70-111                       pnec_hip_solve (mode TARGET/HOST)
 *   PNECCeres::Optimize(bvs1,bvs2,covs1,covs2,reg)              ... mode SYM
 *     src/optimization/pnec_ceres.cc:113-168  (pypnec.pyceres, python/pypnec.cpp:50-66)
 *   NECCeres::Optimize(bvs1,bvs2)                               ... mode NEC
 *     src/optimization/nec_ceres.cc:73-101    (pypnec.pyceresnec, python/pypnec.cpp:68-82)
 *   PNECCeres::InitValues(q,t) / Result()                       init_q/init_t in, out_q/out_t out
 *     src/optimization/pnec_ceres.cc:182-186,201-207
 *   PNEC::CeresSolver / CeresSolverFull / NECCeresSolver        pnec_hip_solve over a batch of pairs
 *     src/rel_pose_estimation/pnec.cc:350-411
 *   ceres::Solver::Options (default-constructed, pnec_ceres.cc:47)   pnec_hip_options
 *   pnec::common::CostFunction  src/common/common.cc:237-259    pnec_hip_cost_function
 *   pnec::common::UnscentedTransform / Unproject  common.cc:460-525   pnec_hip_unscented_transform
 *   pnec::common::Undistort  common.cc:67-93 (cv::undistortPoints [EXT])   pnec_hip_undistort_keypoints
 *   matches_from_poses  scripts/pnec/visual_odometry/io/evaluate_run.py:118-129      pnec_hip_trajectory_compose
 *    (the chain of relative poses and the pose correction)
 *   rmse, l1_error, rpe_n, l1_rpe_n, r_t  in scripts/pnec/metrics                      pnec_hip_trajectory_metrics
 *   (no counterpart: what ceres::Covariance would give for the        pnec_hip_pose_covariance
 *    problems of pnec_ceres.cc / nec_ceres.cc)
 *   (no counterpart: the per-residual values ceres::Problem::Evaluate  pnec_hip_residuals
 *    would return for the problems of pnec_ceres.cc / nec_ceres.cc)
 *   (no counterpart: the structure a pose implies and the sign of t,   pnec_hip_triangulate
 *    which TranslationalDifference(..., both_directions = true) hides)
 *   EMPoseEstimation(bvs1, bvs2, initial_pose, EIGHTPT, false) +     pnec_hip_eight_point
 *    PoseFromEssentialMatrix  essential_matrix_methods.cc:45-126, common.cc:262-457
 *   opengv's fivept_nister / sevenpt [EXT] + PoseFromEssentialMatrix  pnec_hip_essential_minimal
 *    (EMPoseEstimation(..., NISTER | SEVENPT, false))
 *   (no counterpart: the length of one pair's baseline in units of    pnec_hip_relative_scale
 *    the previous pair's, from the tracks both see)
 *   POpticalFlowPatch::setFromImage (Cov) + KLTPatchOpticalFlow's     pnec_hip_patch_covariance
 *    scaling and rotation  include/features/tracking/pnec_patch.h:78-137,
 *    klt_patch_optical_flow.h:244-252  (the covariance only: no tracking; double, not the reference's float)
 *   KLTPatchOpticalFlow::trackPoints / trackPoint / trackPointAtLevel  pnec_hip_patch_track,
 *    klt_patch_optical_flow.h:195-342 + POpticalFlowPatch::residual     pnec_hip_image_pyramid_level
 *    pnec_patch.h:139-170  (the iteration and the pyramid: no detection, no ids; double, not the reference's float)
 *   KLTPatchOpticalFlow::addPoints  klt_patch_optical_flow.h:344-385       pnec_hip_detect_keypoints
 *    (basalt's detectKeypoints on a grid + cv::FAST [EXT]: the detector only)
 *   KLTPatchOpticalFlow::processFrame klt_patch_optical_flow.h:121-191      pnec_hip_tracks_retain, pnec_hip_tracks_append,
 *    (ids, the surviving tracks, the refill, a template image per track)     pnec_hip_patch_track_indexed
 *   OpticalFlowPatch kept per track klt_patch_optical_flow.h:344-385, :228     pnec_hip_patch_store_add,
 *    (a slot per track filled at birth, the tracker reading its templates)   pnec_hip_patch_track_stored
 *   PNEC::Eigensolver (no RANSAC) / WeightedEigensolver  pnec.cc:231-348   pnec_hip_nec_eigensolver /
 *                                                               pnec_hip_weighted_eigensolver
 *
 * Conventions (same as the reference):
 *   - bearing vectors: 3 doubles each, unit norm; frame 1 = "host", frame 2 = "target".
 *   - covariances: 9 doubles each in Eigen column-major order (std::vector<Eigen::Matrix3d>);
 *     only the symmetric part matters.
 *   - quaternions: x,y,z,w (Eigen coeffs() order).  R takes frame-2 vectors into frame 1.
 *   - a batch holds n_pairs independent frame pairs; pair p owns correspondences
 *     [offsets[p], offsets[p+1]) of the concatenated arrays (ragged sizes allowed).
 *   - a "solve" is one (pair, hypothesis): s = pair * n_hyp + hypothesis.
 *
 * Plain pointers and sizes only; no C++ or torch types.  All functions return 0 on success or a
 * negative pnec_hip_status; pnec_hip_last_error() gives the message for the calling thread.
 * A handle (problem) is not thread-safe; distinct handles are independent.
 */
#ifndef PNEC_HIP_H_
#define PNEC_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PNEC_HIP_ABI_VERSION 8
#define PNEC_HIP_MAX_RANSAC_SAMPLE 16 /* largest Options::ransac_sample_size_ the RANSAC kernel is built for */

typedef enum pnec_hip_status {
  PNEC_HIP_OK = 0,
  PNEC_HIP_ERR_INVALID_ARGUMENT = -1,
  PNEC_HIP_ERR_HIP_RUNTIME = -2,   /* a hip* call failed (no device, OOM, launch failure ...) */
  PNEC_HIP_ERR_UNSUPPORTED = -3,
  PNEC_HIP_ERR_BUSY = -4           /* streaming handle: every slot holds a ticket that has not been collected */
} pnec_hip_status;

/* residual family == which reference functor the device evaluates */
typedef enum pnec_hip_mode {
  PNEC_HIP_MODE_NEC = 0,    /* include/optimization/nec_residual.h:51-63   */
  PNEC_HIP_MODE_TARGET = 1, /* include/optimization/pnec_residual.h:86-104 */
  PNEC_HIP_MODE_HOST = 2,   /* include/optimization/pnec_residual.h:55-72  */
  PNEC_HIP_MODE_SYM = 3     /* include/optimization/pnec_residual.h:120-142 */
} pnec_hip_mode;

/* per-solve termination code (out_status); what ceres::Solver::Summary would have said */
typedef enum pnec_hip_termination {
  PNEC_HIP_TERM_FUNCTION_TOL = 0,
  PNEC_HIP_TERM_PARAMETER_TOL = 1,
  PNEC_HIP_TERM_GRADIENT_TOL = 2,
  PNEC_HIP_TERM_MAX_ITERATIONS = 3,
  PNEC_HIP_TERM_MIN_RADIUS = 4,
  PNEC_HIP_TERM_INVALID_STEPS = 5,
  PNEC_HIP_TERM_BAD_INITIAL = 6 /* non-finite cost/Jacobian (e.g. NaN input); last iterate returned */
} pnec_hip_termination;

typedef enum pnec_hip_memspace {
  PNEC_HIP_MEM_HOST = 0,  /* pointer arguments are host memory; the call blocks until done */
  PNEC_HIP_MEM_DEVICE = 1 /* pointer arguments are device memory; the call is asynchronous on `stream` */
} pnec_hip_memspace;

/* The ceres::Solver::Options fields the reference's default-constructed optimiser relies on
 * (defaults = Ceres 2.x defaults), plus launch tuning.  Fill with pnec_hip_default_options(). */
typedef struct pnec_hip_options {
  int32_t max_num_iterations;                /* 50 */
  int32_t max_num_consecutive_invalid_steps; /* 5 */
  int32_t jacobi_scaling;                    /* 1 */
  int32_t check_convergence;                 /* 1; 0 = exactly max_num_iterations LM iterations */
  int32_t corr_per_lane;                     /* 0 = auto; launch tuning: correspondences held per lane */
  int32_t waves_per_pair;                    /* 0 = auto; launch tuning: wavefronts cooperating on one solve */
  int32_t lds_corr_per_lane;                 /* launch tuning: how many of corr_per_lane live in LDS */
  int32_t flags;                             /* 0; a set of PNEC_HIP_OPT_* bits (below); an undefined bit:
                                                PNEC_HIP_ERR_INVALID_ARGUMENT.  (ABI <= 5 called this field `reserved`
                                                and defined bit 0 only.) */
  double function_tolerance;                 /* 1e-6 */
  double gradient_tolerance;                 /* 1e-10 */
  double parameter_tolerance;                /* 1e-8 */
  double initial_trust_region_radius;        /* 1e4 */
  double max_trust_region_radius;            /* 1e16 */
  double min_trust_region_radius;            /* 1e-32 */
  double min_relative_decrease;              /* 1e-3 */
  double min_lm_diagonal;                    /* 1e-6 */
  double max_lm_diagonal;                    /* 1e32 */
} pnec_hip_options;

/* pnec_hip_options.flags */
#define PNEC_HIP_OPT_COUNT_PASSES 1 /* diagnostics: add the correspondence-passes this call executes -- in full /
                                        cost-only -- to pnec_hip_work_counters()[13] / [14] */
#define PNEC_HIP_OPT_JACOBIAN_NUMERIC_CENTRAL 2
/* VERIFICATION mode (ABI 6): differentiate the way the reference does -- ceres::NumericDiffCostFunction<Functor, CENTRAL,
 * 1, 1, 1, 4> (src/optimization/pnec_ceres.cc:84-97; nec_ceres.cc:82-93): per AMBIENT parameter x_j of (theta, phi, qx, qy,
 * qz, qw) the residual at x_j +- h, h = max(sqrt(eps), 1e-6 |x_j|), J_j = (r+ - r-) / (2 h), the quaternion perturbed
 * component-wise WITHOUT renormalisation (toRotationMatrix of a non-unit quaternion), then the 1x4 block through
 * EigenQuaternionManifold::PlusJacobian (4x3) [EXT] -- instead of the closed-form Jacobian.  Thirteen residual evaluations
 * per correspondence and pass, streamed from HBM (no on-chip residency, one 8-wavefront block per solve): ~20x slower
 * than the production kernel, and not meant to be anything else.  It exists so that the device can follow the reference's
 * TRAJECTORY on solves that are not converged when they stop (fixed iteration counts from far-off starts), where the
 * rounding of the difference quotient -- not the derivative -- decides the last digits of every step.  pnec_hip_solve
 * only (the streaming handle returns PNEC_HIP_ERR_UNSUPPORTED). */

typedef struct pnec_hip_problem pnec_hip_problem; /* opaque: a batch of pairs resident in HBM */

/* Which iteration stands in for opengv::relative_pose::eigensolver's eigenvalue minimisation -- called at
 * src/rel_pose_estimation/pnec.cc:274 (plain), :239-258 (RANSAC hypotheses + optimizeModelCoefficients) and :315 (the
 * weighted stage's rounds).  opengv is NOT in the reference tree: all three are restatements, the last two from memory
 * of its source (oracle/pnec_oracle_opengv.c says what is remembered and how surely; INTEGRATION.md 6 which to pick).
 *   NEWTON  damped Newton on lambda_min(M(R(v))) to ~1e-12 rad (rounds 1-4's only form; the fastest).
 *   DESCENT [EXT] normalised steepest descent, step 0.01 doubled up to 0.08 in the first iteration, halved while the
 *           value does not improve, stop at step < 1e-5 or 50 iterations: ends ~1e-5 rad short of the minimiser.
 *   LM      [EXT] Eigen/MINPACK Levenberg-Marquardt (ftol 5e-5, xtol 10 eps, maxfev 100) on the gradient of lambda_min
 *           of M composed with opengv's REDUCED Cayley rotation (no 1 / (1 + |v|^2)), forward-difference Jacobian: the
 *           root of that gradient -- 1e-9 (KITTI-like motion) .. 1e-5 rad (|v| ~ 0.3) from NEWTON's minimiser.
 * Under DESCENT and LM every RANSAC hypothesis is scored (no iteration cap that voids a model), and the weighted
 * stage runs the eigensolver in every round under DESCENT (each call moves the rotation a little further). */
typedef enum pnec_hip_eigensolver_scheme {
  PNEC_HIP_ES_NEWTON = 0,
  PNEC_HIP_ES_DESCENT = 1,
  PNEC_HIP_ES_LM = 2
} pnec_hip_eigensolver_scheme;

int pnec_hip_abi_version(void);
const char *pnec_hip_last_error(void);
int pnec_hip_device_count(int *count);
void pnec_hip_default_options(pnec_hip_options *opt);

/* Allocate HBM for a batch.  offsets: HOST int64[n_pairs+1], non-decreasing, offsets[0]==0.
 * mode fixes which arrays the batch carries: NEC bvs only; TARGET/HOST bvs + one covariance
 * array; SYM bvs + both. */
int pnec_hip_problem_create(int device, int mode, int64_t n_pairs, const int64_t *offsets,
                            pnec_hip_problem **out);
int pnec_hip_problem_destroy(pnec_hip_problem *p);

/* A batch that is shaped again and again without allocating: room for up to max_pairs pairs holding up to
 * max_corr correspondences in total; created empty (0 pairs).  pnec_hip_problem_reshape gives it a shape --
 * offsets as in pnec_hip_problem_create -- on `stream` (the index arrays are uploaded asynchronously; work
 * queued earlier on that stream still sees the old shape); the planes then hold garbage until filled.  Shapes
 * beyond the capacity return PNEC_HIP_ERR_INVALID_ARGUMENT.  What the per-frame callers of the reference need
 * (one PNEC::Solve per frame pair, frame2frame.cc:122-141): see pnec_hip_frame_* below, which is built on it. */
int pnec_hip_problem_create_capacity(int device, int mode, int64_t max_pairs, int64_t max_corr,
                                     pnec_hip_problem **out);
int pnec_hip_problem_reshape(pnec_hip_problem *p, int64_t n_pairs, const int64_t *offsets, void *stream);

/* Fill pairs [first_pair, first_pair+n_pairs) from arrays in the REFERENCE layout (AoS: bvs
 * 3 doubles, covs 9 doubles column-major per correspondence), pointing at the first
 * correspondence of `first_pair`.  `covs` is the single array of Optimize(bvs1,bvs2,covs,..)
 * [frame 2 for TARGET, frame 1 for HOST] or covs_2 of the symmetric overload; `covs_host` is
 * covs_1 of the symmetric overload (NULL otherwise).  space = where those arrays live.
 * HOST space stages the arrays in HBM first (15 / 24 doubles per correspondence on top of the 12 / 18 of the planes): a
 * capacity-shaped batch keeps that staging between calls while it is <= 256 MB (per-frame handles: nothing allocated per
 * call); larger stagings are borrowed from the library's buffer cache for the call (pnec_hip_release_cache frees it). */
int pnec_hip_problem_fill(pnec_hip_problem *p, int64_t first_pair, int64_t n_pairs,
                          const double *bvs1, const double *bvs2, const double *covs,
                          const double *covs_host, int space, void *stream);

/* Fused keypoint ingest: KeyPoint::Unproject (src/frames/keypoints.cc:49-62) for the keypoints of both
 * frames -- bearing = normalised K^-1 (u, v, 1); bearing covariance = UnscentedTransform(mu, 2x2 image
 * covariance, K^-1, kappa, Pinhole) (src/common/common.cc:460-525) -- written straight into the batch's
 * SoA planes: 56 B per correspondence cross the bus instead of 120 B, and no AoS 3x3 covariance is ever
 * stored.  Same bits as pnec_hip_unscented_transform followed by pnec_hip_problem_fill.
 *   pts1, pts2 [M,2]   pixel coordinates (KeyPoint::point_) of frame 1 / frame 2
 *   cov2 [M,3]         frame-2 image covariance (xx, xy, yy) (KeyPoint::img_covariance_); NULL for NEC batches
 *   cov1 [M,3]         frame-1 image covariance, SYM batches only (else NULL)
 *   K_inv [9] column-major, kappa (1.0 in the reference), camera_model must be 1 (Pinhole)
 * M = correspondences of pairs [first_pair, first_pair + n_pairs), pointing at the first of them. */
int pnec_hip_problem_fill_keypoints(pnec_hip_problem *p, int64_t first_pair, int64_t n_pairs, const double *pts1,
                                    const double *pts2, const double *cov2, const double *cov1, const double *K_inv,
                                    double kappa, int camera_model, int space, void *stream);

/* The same ingest, shaped by offsets that may live on the device (added within ABI 8: a pure addition,
 * PNEC_HIP_ABI_VERSION is unchanged): what a tracker that reads nothing back hands over -- rows of keypoints, ragged by
 * an offsets array only the device knows -- becomes a batch without the host ever learning the pair sizes.
 *   p        a capacity batch (pnec_hip_problem_create_capacity).  Its current shape -- the last
 *            pnec_hip_problem_reshape -- is read as BOUNDS: pair k may hold up to bound_k = (that shape's) offsets[k+1] -
 *            offsets[k] correspondences, and its block keeps that room.  The bounds stay until the next reshape.
 *   offsets  int64 [n_pairs + 1], in `space` like the other arrays: rows [offsets[k], offsets[k+1]) of pts1 / pts2 /
 *            cov2 / cov1 are pair k's correspondences.  The range is cut to [0, n_rows] first (lo = clamp(offsets[k], 0,
 *            n_rows), hi = clamp(offsets[k+1], lo, n_rows)); the pair takes its first cnt_k = min(hi - lo, bound_k) rows.
 *            It must not be the batch's own offsets array.
 *   n_rows   the rows of pts1, pts2 [n_rows,2], cov2, cov1 [n_rows,3]; at most 2^31-1
 *   cov2 / cov1, K_inv, kappa, camera_model   as for pnec_hip_problem_fill_keypoints; cov2 must be NULL for a NEC batch
 *            and given otherwise, cov1 given for a SYM batch and NULL otherwise, whatever the sizes turn out to be
 *   out_dropped  int32 [n_pairs] or NULL: (hi - lo) - cnt_k, the rows the bound turned away
 * It writes, per pair, the count cnt_k, the batch's own offsets (the exclusive scan of the counts: the positions the
 * per-correspondence outputs of the other calls use) and the SoA planes with stride round_up(cnt_k, 64) at the start of
 * the pair's bound-sized block, padding lanes zero: what pnec_hip_problem_fill_keypoints writes for the same rows, bit
 * for bit.  The batch is then in the state pnec_hip_problem_select leaves its result in: launch geometries follow the
 * bounds, the real sizes exist on the device only, and every DEVICE-space stage takes it as it is; the first call that
 * needs host-side sizes (pnec_hip_problem_offsets, _num_correspondences, a HOST-space mask, ...) waits for `stream` and
 * fetches them.  pnec_hip_problem_reshape makes it an exact batch again.
 * DEVICE space: asynchronous on `stream`, no host synchronisation, and nothing is allocated after the first call (the
 * first call after a reshape uploads the bounds and waits for the previous such upload, as reshape itself does); nothing
 * but the cut above is validated.  HOST space: staged like the other calls, waits for the stream; offsets that decrease,
 * start below 0 or end beyond n_rows are refused.  Refusals are PNEC_HIP_ERR_INVALID_ARGUMENT: a batch without capacity,
 * NULL offsets or K_inv, a covariance array missing or present against the mode, a bad space, camera_model != 1. */
int pnec_hip_problem_fill_keypoints_ragged(pnec_hip_problem *p, const int64_t *offsets, int64_t n_rows, const double *pts1,
                                           const double *pts2, const double *cov2, const double *cov1, const double *K_inv,
                                           double kappa, int camera_model, int32_t *out_dropped, int space, void *stream);

/* Keypoint undistortion: the radial-tangential ("plumb bob") lens model inverted per tracked point (added within ABI 8: a
 * pure addition, PNEC_HIP_ABI_VERSION is unchanged).  The ingest above is pinhole only; a tracker follows patches in the
 * raw image, so its points and 2x2 covariances are in distorted pixels.  This call stands between the two: rows in the
 * layout of pnec_hip_problem_fill_keypoints_ragged come in, rows in that layout go out.  It is what the reference does
 * per observation, pnec::common::Undistort (src/common/common.cc:67-93, called from converter.cc:75-92): a call of
 * cv::undistortPoints with Camera.k1, k2, p1, p2 and P = K.
 *
 *   pts1, pts2 [n_rows,2]   raw pixels of frame 1 / frame 2; either may be NULL (that frame is left out)
 *   cov2, cov1 [n_rows,3]   (xx, xy, yy) of pts2 / pts1, or NULL; a covariance needs its points
 *   camera [9]              fx fy cx cy k1 k2 p1 p2 k3, in `space` like the other arrays
 *   out_pts1, out_pts2, out_cov2, out_cov1   given exactly where their input is given
 *   out_status1, out_status2  uint8 [n_rows] or NULL (NULL where the points are NULL): pnec_hip_undistort_status
 *
 * The forward model, distort(x, y), in normalised coordinates:
 *     r2 = x x + y y,  cdist = 1 + ((k3 r2 + k2) r2 + k1) r2,
 *     dx = p1 (2 x y) + p2 (r2 + 2 x x),  dy = p1 (r2 + 2 y y) + p2 (2 x y),
 *     distort(x, y) = (x cdist + dx, y cdist + dy)
 * and its Jacobian J, with dc = (3 k3 r2 + 2 k2) r2 + k1 (the derivative of cdist by r2):
 *     j00 = cdist + 2 x x dc + (2 p1 y + 6 p2 x),   j11 = cdist + 2 y y dc + (6 p1 y + 2 p2 x),
 *     j01 = j10 = 2 x y dc + (2 p1 x + 2 p2 y).
 * Per point (u, v), every operation in FP64, rounded one by one in the order written (no fused multiply-add):
 *  1 Normalise.  x0 = (u - cx) / fx, y0 = (v - cy) / fy.  A u or v that is not finite gives NaN for both output
 *    coordinates, status NOT_FINITE, and its covariance is copied.
 *  2 Fixed point ([EXT]: cv::undistortPoints restated from memory, OpenCV is not in the reference tree; 5 steps are its
 *    default termination).  Start at (x, y) = (x0, y0).  Repeat fixed_iterations times: r2 = x x + y y;
 *    icdist = 1 / (1 + ((k3 r2 + k2) r2 + k1) r2); if icdist < 0 the point becomes (x0, y0), the status OUTSIDE, and the
 *    iteration stops; else, with dx, dy as above at (x, y): x = (x0 - dx) icdist, y = (y0 - dy) icdist.
 *  3 Newton, with PNEC_HIP_UNDISTORT_NEWTON (not in the reference) and only where step 2 did not end OUTSIDE.  Start
 *    from step 2's result.  Before each of up to newton_iterations steps the forward residual e = distort(x, y) - (x0, y0)
 *    and rho = sqrt(e0 e0 + e1 e1) are computed; rho <= 2^-46 max(1, sqrt(x0 x0 + y0 y0)) stops the iteration with OK.
 *    Otherwise det = j00 j11 - j01 j10; a det that is zero or not finite ends the iteration; else
 *    x -= (j11 e0 - j01 e1) / det, y -= (j00 e1 - j10 e0) / det.  rho is looked at once more after the last step.  If the
 *    iteration ended without the stop, the status is NOT_CONVERGED and the point is step 2's result: never worse than
 *    the reference's answer.
 *  4 Back to pixels with the same K (the reference passes P = K): u' = fx x + cx, v' = fy y + cy.
 *  5 Covariance.  Without PNEC_HIP_UNDISTORT_PROPAGATE_COV (the reference), or where the status is not OK, the three
 *    doubles are copied bit for bit.  With it, J is taken at the returned (x, y), and with D = diag(fx, fy) the linear
 *    map of pixels is A = D J^-1 D^-1: a00 = j11 / det, a01 = ((-j01 / det) fx) / fy, a10 = ((-j10 / det) fy) / fx,
 *    a11 = j00 / det.  M = A S, S' = M A': xx' = m00 a00 + m01 a01, xy' = m00 a10 + m01 a11, yy' = m10 a10 + m11 a11.
 *    (A det that is zero or not finite copies the covariance; the status stays OK.)
 *  6 All five coefficients zero (compared with == 0.0): points and covariances are copied bit for bit with status OK,
 *    whatever the flags and whatever the points hold; this is looked at first.  The kernel decides it from the camera
 *    array, since in DEVICE space the host never sees it: "distortion given but zero" equals "no distortion".
 * A row's bits depend on the row, the camera and the scalar arguments alone: not on n_rows, on the row's position or on
 * the other rows.  Rows whose status is not OK pass through with their status, as in OpenCV; nothing is dropped.
 *
 * Aliasing: an output may be the very same pointer as its input (in place).  Any other overlap among the arrays is
 * undefined.  DEVICE space: asynchronous on `stream`, no host wait, nothing allocated.  HOST space: staged on `device`
 * like the other calls, waits for the stream.
 * Refused with PNEC_HIP_ERR_INVALID_ARGUMENT before any device is touched: fixed_iterations or newton_iterations outside
 * 0 .. 64 (newton_iterations is not looked at without the NEWTON flag), an unknown flag bit, n_rows < 0 or > 2^31-1,
 * camera NULL, a bad space; and for n_rows > 0 an input without its output, an output (a status included) without its
 * input, a covariance without its points.  n_rows == 0 returns 0. */
#define PNEC_HIP_UNDISTORT_NEWTON 1u         /* polish the fixed-point result by Newton steps on the forward model */
#define PNEC_HIP_UNDISTORT_PROPAGATE_COV 2u  /* out_cov = A cov A', else out_cov = cov bit for bit (the reference) */
typedef enum pnec_hip_undistort_status {
  PNEC_HIP_UNDISTORT_OK = 0,
  PNEC_HIP_UNDISTORT_OUTSIDE = 1,
  PNEC_HIP_UNDISTORT_NOT_CONVERGED = 2,
  PNEC_HIP_UNDISTORT_NOT_FINITE = 3
} pnec_hip_undistort_status;
int pnec_hip_undistort_keypoints(int device, int64_t n_rows, const double *pts1, const double *pts2, const double *cov2,
                                 const double *cov1, const double *camera, int32_t fixed_iterations,
                                 int32_t newton_iterations, uint32_t flags, double *out_pts1, double *out_pts2,
                                 double *out_cov2, double *out_cov1, uint8_t *out_status1, uint8_t *out_status2, int space,
                                 void *stream);

/* Trajectory evaluation (added within ABI 8: a pure addition, PNEC_HIP_ABI_VERSION is unchanged): the relative poses of a
 * run composed into a trajectory, and the five numbers the reference judges a run by.  Both calls take rows that are
 * sequence-major and ragged by `offsets` int64 [n_seq + 1], in `space` like the other arrays; sequence f is the rows
 * lo .. hi of the cut pnec_hip_problem_fill_keypoints_ragged makes: lo = clamp(offsets[f], 0, n_rows),
 * hi = clamp(offsets[f + 1], lo, n_rows), L = hi - lo.  Rows of no sequence are neither read nor written (out_err_q
 * aside, which is written for every row).  Quaternions are x, y, z, w; all arithmetic is FP64.
 *
 * Rules of both calls.  DEVICE space: asynchronous on `stream`, no host wait, nothing allocated, `offsets` is not read
 * back; the launches are sized by n_rows and n_seq alone; the offsets must not step down after the cut (else the
 * outputs are unspecified; every access stays inside the arrays).  No floating-point atomics: every sum runs in an order
 * fixed by L, so the bits of a sequence's outputs depend on its own rows (and q0, p0) and on L alone, not on n_seq, on
 * the sequence's position or on its neighbours.  HOST space: the arrays are staged on `device`, the offsets are checked
 * (from 0, non-decreasing, within n_rows), and the call waits for the stream.
 * Refused with PNEC_HIP_ERR_INVALID_ARGUMENT before any device is touched: n_seq < 1 or > 2^31-1, n_rows < 0 or
 * > 2^31-1, offsets NULL, a bad space, an output that is also an input or another output (the same pointer; arrays that overlap
 * otherwise are undefined), and what each call lists.
 *
 * pnec_hip_trajectory_compose: evaluate_run.py:118-120 (poses[i] = poses[i-1] * poses[i]) and :122-129 (the pose
 * correction, a left factor) per sequence.
 *   rel_q [n_rows,4]         the relative rotation of each row
 *   rel_t [n_rows,3] | NULL  its translation
 *   scale [n_rows] | NULL    multiplies rel_t (the output of pnec_hip_relative_scale chained); needs rel_t
 *   q0 [n_seq,4] | NULL      the left factor's rotation per sequence (NULL: the identity); normalised as read
 *   p0 [n_seq,3] | NULL      the left factor's position (NULL: zero); needs rel_t
 *   out_q [n_rows,4]         the absolute rotations
 *   out_p [n_rows,3]         the absolute positions, given exactly when rel_t is
 *   out_valid [n_rows] uint8 | NULL   1 where the row was present
 *  1 A row is present when every value given for it (rel_q, rel_t, scale, and the scaled translation) is finite and
 *    |rel_q|^2 = x x + y y + z z + w w, as computed, is finite and > 0.  Its step is (rel_q / |rel_q|, scale rel_t).
 *  2 A row that is not present acts as the identity step and gets out_valid 0: a frame the keyframe rule skipped or a
 *    pair without correspondences, whose pose the odometry reports as NaN, carries the pose before it -- bit for bit
 *    inside a lane's chunk of step 5, and to that step's rounding where the row is a chunk's first: the two rows then
 *    come from products associated differently.
 *  3 The first row of a sequence is a pose itself (the reference writes SE3() there): P_lo = (q0, p0) step_lo,
 *    P_k = P_{k-1} step_k, with (q_a, p_a) (q_b, p_b) = (q_a q_b, p_a + R(q_a) p_b).
 *  4 out_q is the product normalised once, where it is written; the running product is not normalised.  Its sign is
 *    the product's: compare up to sign.  A q0 that is zero or not finite gives NaN for its sequence.
 *  5 The definition is the sequential product from the left.  The kernel associates differently (the product is
 *    associative): one wavefront per sequence, each lane multiplies ceil(L / 64) consecutive steps, a scan in a fixed
 *    order joins the 64 partial products.  Against the sequential product in exact arithmetic: |dq| <= 8 (L + 2) u up
 *    to sign and |dp| <= 16 (L + 2) u x (path length), u = 2^-53.
 * Refused besides: rel_q or out_q NULL (n_rows > 0), scale or p0 without rel_t, out_p given without rel_t or missing
 * with it.  n_rows == 0 returns 0. */
int pnec_hip_trajectory_compose(int device, int64_t n_seq, const int64_t *offsets, int64_t n_rows, const double *rel_q,
                                const double *rel_t, const double *scale, const double *q0, const double *p0,
                                double *out_q, double *out_p, uint8_t *out_valid, int space, void *stream);

/* pnec_hip_trajectory_metrics: RPE_1, RPE_n, L1RPE_1, L1RPE_n (scripts/pnec/metrics/rmse.py, l1_error.py, rpe_n.py,
 * l1_rpe_n.py) and r_t (r_t.py:24-40) per sequence, in radians.
 *   est_q, gt_q [n_rows,4]         absolute rotations, estimate and ground truth, in the reference's convention: the
 *                                  relative pose of frames i, j is P_i^-1 P_j
 *   est_p, gt_p [n_rows,3] | NULL  absolute positions, both or neither
 *   out_metrics [n_seq,5]          RPE_1, RPE_n, L1RPE_1, L1RPE_n, r_t
 *   out_err_q [n_rows,4], out_rmse_d [n_rows], out_l1_d [n_rows]   required: results, and the storage the call's
 *                                  kernels hand on to one another, so that the call allocates nothing
 *   out_angle1, out_rt1 [n_rows] | NULL   the angle and the translation error of consecutive rows; out_rt1 needs the
 *                                  positions
 *  1 e_i = normalise(normalise(est_i) conj(normalise(gt_i))) -> out_err_q, for every row.  The product a b has the vector
 *    part (a_w b_x + a_x b_w) + (a_y b_z - a_z b_y) and its cyclic fellows and the scalar part (a_w b_w - a_x b_x) -
 *    (a_y b_y + a_z b_z), every operation rounded on its own (no fused multiply-add): est_i == gt_i gives (0, 0, 0, 1).
 *  2 angle(i, j) = 4 asin(min(1, |e_i - s e_j| / 2)), s = +1 if <e_i, e_j> >= 0, else -1.  It lies in [0, pi] and is the
 *    reference's arccos((trace(rel) - 1) / 2) (rmse.py:19-25) of rel = (Est_j' Est_i)(Gt_i' Gt_j): the trace is cyclic,
 *    so rel's angle is that of E_i' E_j with E = Est Gt'.
 *  3 For d = 1 .. L-1: rmse_d = sqrt(sum_i angle(i, i+d)^2 / (L - d)), l1_d = sum_i angle(i, i+d) / (L - d), i = 0 ..
 *    L-d-1, written at row lo + d; row lo gets 0.
 *  4 out_angle1[lo + k] = angle(k-1, k); row lo gets 0.
 *  5 RPE_1 = rmse_1, RPE_n = (sum_d rmse_d) / L, L1RPE_1 = l1_1, L1RPE_n = (sum_d l1_d) / L.  The divisor is L, not
 *    L - 1: the reference's (rpe_n.py:39, l1_rpe_n.py:34).
 *  6 r_t, for k = 1 .. L-1: u = R(gt_{k-1})' (p_gt,k - p_gt,k-1), normalised (gt_{k-1} normalised first), v likewise from
 *    the estimate; rt_k = 2 asin(min(1, |u - s v| / 2)), s as in step 2: in [0, pi/2], the reference's
 *    min(arccos(c), arccos(-c)).  A step of length zero gives NaN, as in the reference.  out_rt1[lo + k] = rt_k, row lo
 *    gets 0; r_t is the mean of rt_k, and NaN without positions.
 *  7 L < 2 gives NaN for all five metrics.  A row that is not finite (or a zero quaternion) gives NaN wherever it
 *    enters, as in the reference; a caller drops such frames from both sides first, as the reference's join on
 *    timestamps with dropna() does, so that the distance d counts matched rows.
 * DEVIATION from the reference: an estimate that is exact gives 0 here, where arccos of a trace rounded past 3 gives
 * NaN there; and small angles keep their digits (arccos loses half of them).
 * Against exact arithmetic, u = 2^-53: out_err_q 16 u; any angle 64 u + 8 u angle; rmse_d, l1_d 64 u + (L - d + 8) u
 * value; the _n metrics 64 u + (2 L + 8) u value.
 * Refused besides: out_metrics NULL; for n_rows > 0 est_q, gt_q, out_err_q, out_rmse_d or out_l1_d NULL; one of est_p,
 * gt_p without the other; out_rt1 without positions.  n_rows == 0 writes NaN to all of out_metrics and returns 0. */
int pnec_hip_trajectory_metrics(int device, int64_t n_seq, const int64_t *offsets, int64_t n_rows, const double *est_q,
                                const double *gt_q, const double *est_p, const double *gt_p, double *out_metrics,
                                double *out_err_q, double *out_rmse_d, double *out_l1_d, double *out_angle1,
                                double *out_rt1, int space, void *stream);

/* pnec_hip_trajectory_advance: one frame's step of the running scale and pose of n_seq sequences in lockstep -- the
 * online form of pnec_hip_relative_scale's chain and of pnec_hip_trajectory_compose (added within ABI 8: a pure
 * addition, PNEC_HIP_ABI_VERSION is unchanged).  The state is per sequence and the caller's: s [n_seq] the baseline of
 * the last pair in units of the first one, q [n_seq,4] xyzw and p [n_seq,3] the pose of the last frame.  A fresh state is
 * s = NaN, q = (0, 0, 0, 1), p = 0.  The call reads (s, q, p) and writes (next_s, next_q, next_p): other arrays, the
 * state is double-buffered.
 *   rel_q [n_seq,4], rel_t [n_seq,3]   the pair's relative pose; rel_t as given (a direction: pass the oriented one,
 *                                      out_t_oriented of pnec_hip_triangulate)
 *   count int32 [n_seq] | NULL, min_count >= 0    the pair's correspondences and the least that make a pose
 *   scale3 [n_seq,3] | NULL            pnec_hip_relative_scale's out_scale as it stands; entry 1, the lower median, is read
 *   n_used int32 [n_seq] | NULL, min_used >= 1    that call's out_n_used and the least that make a ratio; needs scale3
 *   out_status int32 [n_seq] | NULL    PNEC_HIP_TRAJ_*
 *  1 The pair is PRESENT iff every word of rel_q and rel_t is finite, |rel_q|^2 = x x + y y + z z + w w, as computed, is
 *    finite and > 0, and count is NULL or count >= min_count: rule 1 of pnec_hip_trajectory_compose and the count.
 *  2 The state scale is VALID iff s is finite and > 0.
 *  3 Not present: next = state, bit for bit; PNEC_HIP_TRAJ_ABSENT.
 *  4 Present, state scale not valid: next_s = 1; PNEC_HIP_TRAJ_STARTED.
 *  5 Present, state scale valid: r = scale3[1] is MEASURED iff scale3 is given, r is finite and > 0, n_used is NULL or
 *    n_used >= min_used, and s * r is finite and > 0.  Measured: next_s = s * r, PNEC_HIP_TRAJ_MEASURED; otherwise
 *    next_s = s (the last baseline is kept), PNEC_HIP_TRAJ_HELD.
 *  6 The pose of a present pair: next_q = normalise(q (rel_q / |rel_q|)), next_p = p + R(q) (next_s rel_t), the product
 *    and the rotation of pnec_hip_trajectory_compose step 3, every operation rounded on its own.  The state is
 *    normalised once a step, where it is written; q is read as it stands (R(q) is a rotation for a unit q: a state this
 *    call wrote, or a fresh one).  A product next_s rel_t that overflows gives a position that is not finite.
 *  7 Against exact arithmetic on the same inputs over L steps, u = 2^-53: |dq| <= 12 (L + 2) u up to sign and
 *    |dp| <= 26 (L + 2) u x (path length), the path being the sum of |next_s rel_t| over the present steps:
 *    pnec_hip_trajectory_compose's 8 u a step and 4 u for the normalisation; twice that as the angle by which a step of
 *    the path is turned, and 2 u a step for the rounding of the scale and of the sum (DESIGN.md 9r has the derivation).
 * One lane per sequence: a sequence's outputs depend on its own inputs alone, not on n_seq, its position or `space`.
 * DEVICE space: asynchronous on `stream`, nothing allocated, nothing read back.  HOST space: staged on `device`, the call
 * blocks.  Refused with PNEC_HIP_ERR_INVALID_ARGUMENT before any device is touched: n_seq < 1 or > 2^31-1, a NULL rel_q,
 * rel_t, s, q, p, next_s, next_q or next_p, min_count < 0, min_used < 1, n_used without scale3, an output that is an input
 * or another output, a bad `space`. */
#define PNEC_HIP_TRAJ_MEASURED 0
#define PNEC_HIP_TRAJ_HELD 1
#define PNEC_HIP_TRAJ_STARTED 2
#define PNEC_HIP_TRAJ_ABSENT 3
int pnec_hip_trajectory_advance(int device, int64_t n_seq, const double *rel_q, const double *rel_t, const int32_t *count,
                                int32_t min_count, const double *scale3, const int32_t *n_used, int32_t min_used,
                                const double *s, const double *q, const double *p, double *next_s, double *next_q,
                                double *next_p, int32_t *out_status, int space, void *stream);

/* The batch's SoA planes as stored in HBM (pair blocks of round_up(N_p, 64)-double planes; the layout in
 * pnec_internal.hpp / DESIGN.md): size in doubles, and a copy out (tests, debugging). */
int64_t pnec_hip_problem_payload_doubles(const pnec_hip_problem *p);
int pnec_hip_problem_export_payload(const pnec_hip_problem *p, double *out, int space, void *stream);

int64_t pnec_hip_problem_num_pairs(const pnec_hip_problem *p);
int64_t pnec_hip_problem_num_correspondences(const pnec_hip_problem *p);
int64_t pnec_hip_problem_max_correspondences(const pnec_hip_problem *p);
/* bytes of bearing/covariance payload the solver reads per pass over the batch (algorithmic) */
int64_t pnec_hip_problem_payload_bytes(const pnec_hip_problem *p);
/* The batch's correspondence offsets, HOST int64[n_pairs+1] (what problem_create was given; for a
 * batch made by pnec_hip_problem_select: the offsets of the kept correspondences). */
int pnec_hip_problem_offsets(const pnec_hip_problem *p, int64_t *out);
int pnec_hip_problem_mode(const pnec_hip_problem *p);
int pnec_hip_problem_device(const pnec_hip_problem *p);
/* The scheme the STAGE calls on this batch use (pnec_hip_nec_eigensolver, pnec_hip_ransac_eigensolver,
 * pnec_hip_weighted_eigensolver; default NEWTON).  pnec_hip_solve_pipeline takes its own from the options.  Under
 * DESCENT weighted_iterations is limited to 16 (a minimiser is kept per round; more: PNEC_HIP_ERR_UNSUPPORTED).  NEWTON
 * and LM run a further minimisation only while the previous one stopped at its evaluation cap (the weights never change
 * from round to round, pnec.cc:297-300), at most 15 of them per pair: a pair still at the cap then keeps that rotation
 * for the remaining rounds.  A batch handed out by pnec_hip_problem_select_view follows its source's scheme. */
int pnec_hip_problem_set_eigensolver_scheme(pnec_hip_problem *p, int32_t scheme);
int pnec_hip_problem_eigensolver_scheme(const pnec_hip_problem *p);

/* RANSAC variants (ABI 7): a set of bits for pnec_hip_pipeline_options.ransac_flags (the chain) and
 * pnec_hip_problem_set_ransac_flags (what pnec_hip_ransac_eigensolver on the batch runs with; default 0).
 *   PNEC_HIP_RANSAC_CHAINED_STARTS  [EXT, recalled: opengv is not in the reference tree]  opengv's
 *     EigensolverSacProblem::getSelectedDistancesToModel leaves the model it scores in the adapter
 *     (_adapter.setR12(model.rotation)), and computeModelCoefficients starts from _adapter.getR12() + jitter: hypothesis
 *     h + 1 starts from the rotation of the last model scored, not from the initial rotation the call site hands over once
 *     (src/rel_pose_estimation/pnec.cc:235-252).  A sequential dependence between hypotheses: with this bit a round is
 *     ONE hypothesis per pair (sixteen side by side without) and the stage costs 20-60x (600 pairs x 256, 25 % gross
 *     mismatches: 1.4 -> 30 ms under scheme 0, 2.2 -> 131 ms under scheme 2); the draws (sample, jitter) of hypothesis h
 *     are the same either way, the hypothesis counts grow (a contaminated sample's minimum is a poor start for the next
 *     one).  A FIDELITY switch, checked against the CPU checker's same switch (tests/test_opengv_schemes.py: masks and
 *     counts identical for 97-99 % of the pairs over chains of 100+ dependent hypotheses); off by default because the
 *     difference is inside the noise of opengv's rand(). */
#define PNEC_HIP_RANSAC_CHAINED_STARTS 1
int pnec_hip_problem_set_ransac_flags(pnec_hip_problem *p, int32_t flags);
int pnec_hip_problem_ransac_flags(const pnec_hip_problem *p);

/* Run InitValues + Optimize + Result for every solve of the batch, entirely on the device.
 *   init_q  [n_pairs,4] xyzw     starting orientation per pair (used as given)
 *   init_t  [n_pairs,3]          starting translation per pair (any non-zero vector; ignored if hyp_t)
 *   n_hyp, hyp_t [n_pairs*n_hyp,3]  optional multi-hypothesis starts sharing init_q (hyp_t NULL -> n_hyp=1)
 *   reg                         regularisation (Options::regularization_, 1e-13 in the reference)
 *   out_q [S,4] normalised, out_t [S,3] unit, out_cost [S] (= 1/2 sum r^2 at the result),
 *   out_iterations [S], out_status [S] (pnec_hip_termination); S = n_pairs*n_hyp; any out may be NULL
 *   space: where init and out arrays live (HOST: blocking; DEVICE: async on stream).  A HOST-space call runs on
 *   `stream` too and returns after everything queued on THAT stream before it; made with stream = NULL it is not ordered
 *   after work on a non-blocking stream.  A caller who filled the batch on a side stream synchronises that stream first
 *   (or passes it).  The same holds for every call that takes `space`.
 * With n_hyp > 1 the hypotheses of a pair share its payload on chip: pairs of up to 512 correspondences run two
 * hypotheses per wavefront (both LM steps at once), larger ones one block per pair and group of 2 / 4 / 8 hypotheses (the
 * group's LM steps at the same time) -- the same bits as n_hyp separate calls, 1.2x .. 1.6x their rate.  */
int pnec_hip_solve(pnec_hip_problem *p, const double *init_q, const double *init_t, int32_t n_hyp,
                   const double *hyp_t, double reg, const pnec_hip_options *opt, double *out_q,
                   double *out_t, double *out_cost, int32_t *out_iterations, int32_t *out_status,
                   int space, void *stream);

/* For each pair keep the hypothesis with the lowest out_cost (ties: lowest index).
 * best_index [n_pairs] int32 receives the hypothesis index.  DEVICE or HOST pointers per `space`. */
int pnec_hip_select_best(int64_t n_pairs, int32_t n_hyp, const double *cost, int32_t *best_index,
                         int space, int device, void *stream);

/* pnec::common::CostFunction (src/common/common.cc:237-259) for every pair: mean over the
 * pair's correspondences of n^2 / (g' Sigma g), no regularisation; pose given as q (xyzw,
 * normalised inside) and t.  Only for TARGET-mode problems.  out [n_pairs].  A pair without correspondences gets
 * 0 / 0 = NaN (the mean of nothing), as the reference's function returns for empty input. */
int pnec_hip_cost_function(pnec_hip_problem *p, const double *q, const double *t, double *out,
                           int space, void *stream);

/* Pose covariance: the uncertainty of a relative pose, from one pass over the pair at a pose the caller passes in
 * (usually pnec_hip_solve's out_q / out_t; a RANSAC, eigensolver or ground-truth pose works the same way).
 *
 * Definition.  With r_i the residuals of the problem's family at (q, t) and J their Jacobian, the Gauss-Newton
 * information matrix is H = J'J.  The probabilistic residuals (TARGET, HOST, SYM) are whitened by the propagated
 * variance, so at the minimum H^-1 is the posterior covariance of the pose (Laplace approximation; what
 * ceres::Covariance returns for the reference's problem).  The NEC residual is NOT whitened: its out_cov is the
 * covariance for unit residual variance and means something only after the caller multiplies it by the variance
 * factor 2 out_cost / (n - 5).  The call never applies that factor.
 *
 * Poses.  q [n_pairs * n_hyp, 4] xyzw (normalised inside, as pnec_hip_cost_function does), t [n_pairs * n_hyp, 3]
 * (any length > 0; used as a direction), slot s = pair * n_hyp + h is evaluated on pair s / n_hyp.  The spherical
 * angles of t are those of AnglesFromVec (src/common/common.cc:103-116): theta = acos(t_z / |t|), phi = atan2(t_y,
 * t_x), and phi = 0 where theta < 1e-10 or t_x = t_y = 0.  `reg` is the regularisation of the residual (the value
 * given to pnec_hip_solve).
 *
 * Charts.  With b_theta = dt/dtheta = (cos th cos ph, cos th sin ph, -sin th) and e_phi = (-sin ph, cos ph, 0) -- an
 * orthonormal basis of the tangent plane of the unit sphere at t -- the pass differentiates in
 *     x = (tau_1, tau_2, omega_x, omega_y, omega_z):  t <- normalize(t + tau_1 b_theta + tau_2 e_phi),
 *                                                     R <- Exp(omega) R   (LEFT perturbation, radians)
 * which, unlike the reference's (theta, phi), is not singular for forward motion t ~ (0, 0, 1).
 *
 * Outputs, per slot; every pointer may be NULL (not wanted), not all of them:
 *   out_info [15]   upper triangle, row by row ((0,0) (0,1) .. (0,4) (1,1) .. (4,4)), of J'J in the CERES TANGENT
 *                   SPACE of the reference's problem: (theta, phi, delta_x, delta_y, delta_z) with the manifolds of
 *                   pnec_ceres.cc -- t = (sin th cos ph, sin th sin ph, cos th), EigenQuaternionManifold's delta =
 *                   omega / 2.  It is D H_x D with D = diag(1, sin theta, 2, 2, 2): exactly 0 in row / column phi at
 *                   theta = 0.
 *   out_cov  [36]   row-major symmetric 6x6 covariance of (omega_x, omega_y, omega_z, t_x, t_y, t_z): the rotation
 *                   vector of a left perturbation R <- Exp(omega) R in radians, and the unit translation direction as
 *                   a vector of R^3.  Sigma_6 = L H_x^-1 L', L = blockdiag(I_3, [b_theta e_phi]): rank 5, t spans its
 *                   null space (the length of t is not observable).
 *   out_grad [5]    J'r in the Ceres tangent space (first-order optimality at the passed pose).
 *   out_cost [1]    1/2 sum r^2.
 *   out_status [1]  pnec_hip_cov_status.  PNEC_HIP_COV_SINGULAR: fewer than 5 correspondences or a non-positive pivot
 *                   in the factorisation -- out_cov is all NaN, the other outputs are written as usual;
 *                   PNEC_HIP_COV_NONFINITE: a sum is Inf / NaN (NaN input) -- out_cov all NaN, the others hold what
 *                   the arithmetic gave.  A slot's outputs depend on its own pair and pose only.
 *
 * All four problem modes; batches made by pnec_hip_problem_select(_view) and reshaped capacity batches included.
 * `space` as in pnec_hip_cost_function: HOST pointers are staged and the call blocks, DEVICE pointers make the call
 * asynchronous on `stream`.  NULL problem / q / t, n_hyp < 1 or all outputs NULL: PNEC_HIP_ERR_INVALID_ARGUMENT
 * before any device is touched. */
typedef enum pnec_hip_cov_status {
  PNEC_HIP_COV_OK = 0,
  PNEC_HIP_COV_SINGULAR = 1,
  PNEC_HIP_COV_NONFINITE = 2
} pnec_hip_cov_status;
int pnec_hip_pose_covariance(pnec_hip_problem *p, const double *q, const double *t, int32_t n_hyp, double reg,
                             double *out_info, double *out_cov, double *out_grad, double *out_cost,
                             int32_t *out_status, int space, void *stream);

/* Per-correspondence residuals and a chi-square inlier gate at a pose the caller passes in (added within ABI 8: a pure
 * addition, PNEC_HIP_ABI_VERSION is unchanged).
 *
 * Definition.  r_i is the residual of the problem's family at (q, t), with the operations of the solve's cost pass in
 * the same order, so it carries the bits the solve sums.  The probabilistic residuals (TARGET, HOST, SYM) are whitened:
 * r_i = n_i / sqrt(den_i), n_i the normal epipolar error and den_i the variance propagated from the correspondence's
 * covariance(s) plus `reg` (TARGET: g' Sigma g + reg).  Under the model r_i ~ N(0, 1), r_i^2 is a chi-square statistic
 * with one degree of freedom, and |r_i| <= gate means "within `gate` sigmas of this pose".  For NEC r_i = n_i, den_i is
 * exactly 1 and `gate` is in the residual's own units.
 *
 * What it is not.  The gate classifies AT the pose it is given: a pose already near the truth (the chain's result, a
 * RANSAC pose, ground truth).  It is not a robust estimator: at a least-squares pose pulled away by gross outliers it
 * rejects the clean correspondences.
 *
 * Poses: q [n_pairs * n_hyp, 4] xyzw, t [n_pairs * n_hyp, 3], slot s = pair * n_hyp + h, `reg` -- all exactly as in
 * pnec_hip_pose_covariance.  `gate` >= 0 in sigmas; +inf is allowed (every finite residual passes).
 *
 * Outputs; every pointer may be NULL (not wanted), not all of them.
 *  per correspondence, n_hyp * sum N entries each; the entry of (pair p, hypothesis h, correspondence i) is
 *  n_hyp * offsets[p] + h * N_p + i, i in the batch's own correspondence order -- with n_hyp == 1 out_mask is what
 *  pnec_hip_problem_select / _select_view take.  Nothing else is written:
 *   out_residual  double   r_i, signed
 *   out_variance  double   den_i as summed, before the solve's clamp: r_i = n_i / sqrt(max(den_i, 1e-300)), so a zero
 *                          covariance with reg = 0 reports variance 0 and a finite (huge) residual
 *   out_mask      uint8    1 iff r_i is finite and |r_i| <= gate
 *  per slot [n_pairs * n_hyp], from a deterministic reduction (a slot's bits depend on its own pair and pose only):
 *   out_chi2         sum r_i^2   (twice pnec_hip_pose_covariance's out_cost)
 *   out_gated_chi2   sum of r_i^2 over the correspondences with mask 1
 *   out_gated_count  int32, the number of those
 *   out_max_abs      max |r_i|; NaN if any r_i is NaN; 0 for a pair without correspondences
 *  The variance factor of a slot is out_chi2 / (N_p - 5).
 *
 * All four problem modes; batches made by pnec_hip_problem_select(_view) and reshaped capacity batches included.  For a
 * batch made by select the positions follow THAT batch's offsets (pnec_hip_problem_offsets).  DEVICE space: the offsets
 * are read on the device, nothing waits, and arrays sized for the source batch are always large enough.  HOST space: the
 * call first resolves the batch's sizes, which waits for the stream that produced them.
 * HOST space also stages the per-correspondence outputs on the device: the handle's staging buffer grows to
 * 17 bytes * n_hyp * sum N (0.87 GB for 100 000 x 512) and, like every staging buffer of a handle, is kept until the handle
 * is destroyed; a caller of that size should pass DEVICE pointers.
 * `space` as in pnec_hip_pose_covariance: HOST pointers are staged and the call blocks, DEVICE pointers make the call
 * asynchronous on `stream`.  NULL problem / q / t, n_hyp < 1, gate < 0 or NaN, all outputs NULL or a bad `space`:
 * PNEC_HIP_ERR_INVALID_ARGUMENT before the handle is read or any device is touched. */
int pnec_hip_residuals(pnec_hip_problem *p, const double *q, const double *t, int32_t n_hyp, double reg, double gate,
                       double *out_residual, double *out_variance, uint8_t *out_mask,
                       double *out_chi2, double *out_gated_chi2, int32_t *out_gated_count, double *out_max_abs,
                       int space, void *stream);

/* Pose sensitivity: the gradient of a loss of the SOLVED pose with respect to every input of the pair -- what a
 * training loop needs to push a pose error back through the refinement onto learned covariances (added within ABI 8: a
 * pure addition, PNEC_HIP_ABI_VERSION is unchanged).  No iteration is unrolled: the pose the refinement returns is a
 * minimiser, so its derivative follows from the implicit-function theorem at that pose, one 5x5 solve per slot and one
 * pass per correspondence.
 *
 * Poses: q, t, slot s = pair * n_hyp + h and `reg` exactly as in pnec_hip_pose_covariance.
 *
 * Chart.  The one of pnec_hip_pose_covariance: x = (tau_1, tau_2, omega), t(x) = normalize(t + tau_1 b_theta + tau_2
 * e_phi), R(x) = Exp(omega) R.
 *
 * Cost.  E(x; theta) = 1/2 sum_i r_i^2 with r_i the residual of the batch's family, `reg` included:
 *     m = t x f1,  g = R'm,  n = f2.g,  h = t x (R a)   (a = f1 for HOST, f2 for SYM)
 *     NEC r = n;  TARGET r = n / sqrt(g'S2 g + reg);  HOST r = n / sqrt(h'S h + reg);  SYM r = n / sqrt(g'S2 g + h'S1 h + reg)
 * theta_i are correspondence i's inputs as the planes hold them: f1 [3], f2 [3], the covariance (symmetric 3x3: S2 of
 * TARGET and SYM, S of HOST) and for SYM the host covariance S1.  f1 and f2 are used as written -- nothing normalises
 * them inside -- and the gradients are plain partials in R^3.
 *     g = grad_x E at x = 0,   H = hess_x E at x = 0 = J'J + sum_i r_i hess_x r_i IN THIS CHART (the curvature of both
 *     manifolds included);  with PNEC_HIP_SENS_GAUSS_NEWTON  H = J'J (1 - 40 % off at 37 - 200 correspondences).
 *
 * Cotangent.  grad_pose [n_pairs * n_hyp, 6] = (dL/d omega [3], dL/d t [3]), in the order of out_cov's rows:
 *     v = (b_theta . dL/dt, e_phi . dL/dt, dL/d omega),   lambda = H^-1 v
 * (Cholesky factor of the Jacobi-scaled H, as pnec_hip_pose_covariance inverts its matrix).
 *
 * Result per correspondence.  dL/d theta_i = - d/d theta_i [ lambda . grad_x (r_i^2 / 2) ] at x = 0.  For a covariance it
 * is the symmetric matrix G with dL = sum_jk G_jk dS_jk: an off-diagonal entry holds half the derivative with respect to
 * the stored plane value.  This is the derivative of the minimiser when g = 0; at any other pose it is exact for the
 * Newton-corrected pose to first order in x_N = -H^-1 g, which the call returns so that a caller can see how converged
 * the pose was.
 *
 * Outputs; every pointer may be NULL (not wanted), not all of them.
 *  per correspondence, M = n_hyp * sum N rows each, the row of (pair p, hypothesis h, correspondence i) is
 *  n_hyp * offsets[p] + h * N_p + i as in pnec_hip_residuals:
 *   out_grad_bvs1 [M,3]  out_grad_bvs2 [M,3]
 *   out_grad_covs [M,9]       row-major symmetric G of the batch's `covs` input; not for NEC
 *   out_grad_covs_host [M,9]  the same for `covs_host`; SYM only
 *  per slot:
 *   out_lambda [5]    lambda
 *   out_hessian [15]  upper triangle of H, row by row, in x (NOT the Ceres tangent space of out_info)
 *   out_grad [5]      g in x
 *   out_newton [5]    x_N
 *   out_status        pnec_hip_sens_status.  PNEC_HIP_SENS_SINGULAR: fewer than 5 correspondences, a non-positive
 *                     diagonal entry or pivot (H is not positive definite: the pose is not a minimiser);
 *                     PNEC_HIP_SENS_NONFINITE: a sum is Inf / NaN.  A failed slot's lambda, x_N and per-correspondence
 *                     rows are NaN, or exactly 0 with PNEC_HIP_SENS_ZERO_ON_FAILURE; H and g are written as computed;
 *                     other slots are unaffected.  A slot's outputs depend on its own pair, pose and cotangent only.
 *
 * All four problem modes; batches made by pnec_hip_problem_select(_view) and reshaped capacity batches included.  `space`
 * as in pnec_hip_residuals (HOST space resolves a selected batch's sizes first and stages every array; DEVICE space is
 * asynchronous on `stream`).  NULL problem / q / t / grad_pose, n_hyp < 1, an unknown bit in flags, all outputs NULL, a
 * covariance output the family has no input for, or a bad `space`: PNEC_HIP_ERR_INVALID_ARGUMENT before the handle's
 * device is touched. */
typedef enum pnec_hip_sens_status {
  PNEC_HIP_SENS_OK = 0,
  PNEC_HIP_SENS_SINGULAR = 1,
  PNEC_HIP_SENS_NONFINITE = 2
} pnec_hip_sens_status;
enum { PNEC_HIP_SENS_GAUSS_NEWTON = 1, PNEC_HIP_SENS_ZERO_ON_FAILURE = 2 };
int pnec_hip_pose_sensitivity(pnec_hip_problem *p, const double *q, const double *t, const double *grad_pose,
                              int32_t n_hyp, double reg, int32_t flags, double *out_grad_bvs1, double *out_grad_bvs2,
                              double *out_grad_covs, double *out_grad_covs_host, double *out_lambda,
                              double *out_hessian, double *out_grad, double *out_newton, int32_t *out_status,
                              int space, void *stream);

/* Triangulation at a pose the caller passes in: depths, points, parallax, depth variance and the cheirality vote that
 * fixes the sign of t (added within ABI 8: a pure addition, PNEC_HIP_ABI_VERSION is unchanged).  Every energy the
 * solvers minimise is even in t; this call is what decides between t and -t.
 *
 * Pose.  R (from q, normalised inside) maps frame-2 vectors into frame 1 and x1 = R x2 + t: camera 1 sits at the origin,
 * camera 2 at t.  t is used as a DIRECTION exactly as in pnec_hip_residuals, so the baseline is 1 and every length
 * below is in baselines; t = 0 is read as (0, 0, 1).  Poses: q [n_pairs * n_hyp, 4] xyzw, t [n_pairs * n_hyp, 3], slot
 * s = pair * n_hyp + h.
 *
 * Midpoint triangulation, bearings not assumed unit.  With u = R f2:
 *   a00 = f1.f1   a10 = f1.u   a11 = u.u   b0 = f1.t   b1 = u.t
 *   D      = a00 a11 - a10^2                  (= sin^2 psi for unit bearings)
 *   depth1 = (a11 b0 - a10 b1) / D            along f1, from camera 1
 *   depth2 = (a10 b0 - a00 b1) / D            along u,  from camera 2
 *   point  = 1/2 (depth1 f1 + t + depth2 u)   in frame 1
 *   psi    = atan2(|f1 x u|, f1.u)            parallax, radians, in [0, pi]
 *   front  = depth1 > 0 and depth2 > 0 (both finite)
 *   back   = depth1 < 0 and depth2 < 0 (both finite)   -- "in front" under -t
 * depth1, depth2 and point are linear in t: at -t they are the exact IEEE negations of their values at t, and front and
 * back swap.
 *
 * Depth variance: the first-order propagation of the resident covariances to depth1.
 *   d depth1 / d u  = ( 2 b0 u - b1 f1 - a10 t  -  depth1 (2 a00 u - 2 a10 f1) ) / D  =: gu
 *   d depth1 / d f1 = ( a11 t - b1 u            -  depth1 (2 a11 f1 - 2 a10 u) ) / D  =: g1
 *   TARGET: (R' gu)' Sigma2 (R' gu)       HOST: g1' Sigma1 g1       SYM: both summed       NEC: NaN
 * Sigma2 is the covariance of f2 in frame 2, Sigma1 that of f1 in frame 1.  No regularisation is added.  Even in t.
 *
 * Degenerate inputs (the result is the same whatever else the pair holds).  D not a positive finite number (parallel
 * rays, a zero bearing): depth1 = depth2 = +inf, point and variance NaN, psi as the atan2 gives it (0 for parallel
 * rays), front 0, counted in neither vote.  A NaN in a bearing: every per-correspondence output NaN, front 0, counted in
 * neither vote, left out of the parallax mean.  D is formed from two rounded products and a D at or below its own rounding
 * error, 2^-49 a00 a11 (a parallax below 4.2e-8 rad, where no digit of a depth is left), is read as 0.
 *
 * Vote, always at t as given: n_front / n_back count the front / back correspondences; sign = +1 if n_front >= n_back
 * (a tie, a pair without correspondences included), else -1; t_oriented = sign * t / |t|.
 *
 * flags: PNEC_HIP_TRI_ORIENT evaluates the per-correspondence outputs at t_oriented instead of t (out_front is then
 * relative to t_oriented; the three vote outputs stay relative to t as given).
 *
 * Outputs; every pointer may be NULL (not wanted), not all of them.  M = n_hyp * sum N; the entry of (pair p,
 * hypothesis h, correspondence i) is n_hyp * offsets[p] + h * N_p + i, the layout of pnec_hip_residuals -- with
 * n_hyp == 1 out_front is what pnec_hip_problem_select / _select_view take.
 *   out_point [M,3] row-major   out_depth1, out_depth2, out_parallax, out_depth1_var [M]   out_front uint8 [M]
 *   out_n_front, out_n_back, out_sign int32 [S]   out_t_oriented [S,3] unit   out_parallax_mean [S]: the mean of psi
 *   over the pair's correspondences that have one (0 if there is none)
 * A slot's bits depend on its own pair and pose only (no atomics, fixed reduction order).
 *
 * All four problem modes; batches made by pnec_hip_problem_select(_view) and reshaped capacity batches included, with
 * the positions following THAT batch's offsets.  DEVICE space: the offsets are read on the device, nothing waits, the
 * call is asynchronous on `stream`.  HOST space: the call first resolves the batch's sizes (which waits for the stream
 * that produced them), stages the outputs on the device and blocks: the handle's staging buffer grows to
 * 57 bytes * n_hyp * sum N (2.9 GB for 100 000 x 512) and is kept until the handle is destroyed; a caller of that size
 * should pass DEVICE pointers.
 * A batch whose largest pair holds 4 GiB of planes or more (29 million correspondences in SYM mode): PNEC_HIP_ERR_UNSUPPORTED.
 * NULL problem / q / t, n_hyp < 1, a flag bit other than PNEC_HIP_TRI_ORIENT, all outputs NULL or a bad `space`:
 * PNEC_HIP_ERR_INVALID_ARGUMENT before the handle is read or any device is touched. */
#define PNEC_HIP_TRI_ORIENT 1
int pnec_hip_triangulate(pnec_hip_problem *p, const double *q, const double *t, int32_t n_hyp, int32_t flags,
                         double *out_point, double *out_depth1, double *out_depth2, double *out_parallax,
                         double *out_depth1_var, uint8_t *out_front, int32_t *out_n_front, int32_t *out_n_back,
                         int32_t *out_sign, double *out_t_oriented, double *out_parallax_mean, int space, void *stream);

/* The eight-point baseline: essential matrix and pose of every pair from its correspondences alone, no start pose
 * (added within ABI 8: a pure addition, PNEC_HIP_ABI_VERSION is unchanged).  It is the closed-form estimator behind the
 * reference's `run_simulation -e`: EMPoseEstimation(..., EIGHTPT, ransac = false).  Conventions as everywhere here: R
 * takes frame-2 vectors into frame 1, t is a direction in frame 1, the constraint is f1' E f2 = 0 with E = [t]x R.
 *
 * Steps 1-2 restate opengv::relative_pose::eightpt from memory ([EXT]: opengv is not in the reference tree); steps 3-5
 * restate PoseFromEssentialMatrix, src/common/common.cc:262-457.  Per pair with N correspondences:
 *  1 Normal matrix.  Row i of A holds the nine products f1_a f2_b in the row-major order of E; G = A'A is 9x9 symmetric
 *    (45 distinct sums).  Bearings are used as stored: no Hartley normalisation (eightpt has none).
 *  2 Null vector.  The eigenvector of G's smallest eigenvalue by cyclic Jacobi (rotations (0,1), (0,2), ... (7,8) per
 *    sweep; stop when the Frobenius norm of the off-diagonal part is at or below 2^-58 trace, 16 sweeps at most).  e has
 *    unit norm and the sign that makes its entry of largest magnitude positive (the lowest index wins a tie); E is e
 *    row-major.  gap = (lambda_1 - lambda_0) / lambda_8 of G's ascending eigenvalues: small for a planar scene or a pure
 *    rotation, where the null vector is not unique -- what a caller gates on.
 *  3 Decomposition (common.cc:280-325).  E = U S V' through the Jacobi eigen-decomposition of E'E: its eigenvalues in
 *    descending order are the squares of the singular values s0 >= s1 >= s2, its eigenvectors v0, v1, v2; v2 gets the
 *    sign that makes its entry of largest magnitude positive (lowest index on a tie) and v1 the sign that makes
 *    (v0, v1, v2) right-handed; u0 = E v0 / |E v0|, u1 = E v1 / |E v1|, u2 = u0 x u1 (so s2 ~ 0 costs nothing).  With
 *    W = [[0,-1,0],[1,0,0],[0,0,1]]: Ra = U W V', Rb = U W' V', each negated if its determinant is negative; ta = u2.
 *    The candidates are (Ra, ta), (Rb, ta), (Ra, -ta), (Rb, -ta), in that order.  The SET of candidates does not depend
 *    on the sign of e, on the signs of the singular vectors or on the rotation of (v0, v1) within their plane when
 *    s0 = s1 (only U and V enter; the singular values do not); the sign rules above fix their ORDER, so that out_choice
 *    means the same on every implementation.  t comes back as a unit direction; the reference's `scale` is out_singular[0].
 *  4 Choice (common.cc:342-406).  The first K = min(9, N) correspondences of the pair (the reference's sampleSize 8 + 1)
 *    are triangulated at each candidate by the midpoint system of pnec_hip_triangulate (opengv's triangulate2); the point
 *    is normalised in frame 1 (r1) and R'(point - t) in frame 2 (r2); quality = sum (1 - f1.r1) + (1 - f2.r2).  The
 *    candidate of lowest quality wins by strict < from a start value of 1e6 (the lowest index wins a tie).  A non-finite
 *    term (parallel rays: no midpoint) makes that candidate's quality +inf.  PNEC_HIP_EP_QUALITY_ALL sums over all N
 *    instead: an extension, for batches whose first nine rows may be outliers.
 *  5 Status, pnec_hip_ep_status.  TOO_FEW: N < 8.  NOT_FINITE: a NaN or an infinity in a bearing the pair holds (or
 *    bearings so long that the sums overflow).  NO_CANDIDATE: no quality below 1e6.  A status other than OK writes NaN to
 *    q, t and E and -1 to out_choice; TOO_FEW and NOT_FINITE write NaN to the other double outputs too.
 *
 * Outputs for P pairs; every pointer may be NULL (not wanted), not all of them.
 *   out_q [P,4] xyzw   out_t [P,3] unit   out_E [P,9] row-major, sign and norm of step 2   out_singular [P,3]
 *   out_gap [P]   out_quality [P,4]   out_choice, out_status int32 [P]
 * A pair's bits depend on its own rows and on `flags` only (no atomics, fixed reduction order).
 *
 * All four problem modes (only the six bearing planes are read); batches made by pnec_hip_problem_select(_view) and
 * reshaped capacity batches included.  DEVICE space: the pair sizes are read on the device, nothing waits, nothing is
 * allocated, the call is asynchronous on `stream`.  HOST space: the outputs are staged on the device (24 doubles and two
 * ints per pair) and the call blocks.
 * NULL problem, all outputs NULL, a flag bit other than PNEC_HIP_EP_QUALITY_ALL or a bad `space`:
 * PNEC_HIP_ERR_INVALID_ARGUMENT before the handle is read or any device is touched. */
#define PNEC_HIP_EP_QUALITY_ALL 1
typedef enum pnec_hip_ep_status {
  PNEC_HIP_EP_OK = 0,
  PNEC_HIP_EP_TOO_FEW = 1,
  PNEC_HIP_EP_NOT_FINITE = 2,
  PNEC_HIP_EP_NO_CANDIDATE = 3
} pnec_hip_ep_status;
int pnec_hip_eight_point(pnec_hip_problem *p, int32_t flags, double *out_q, double *out_t, double *out_E,
                         double *out_singular, double *out_gap, double *out_quality, int32_t *out_choice,
                         int32_t *out_status, int space, void *stream);

/* The minimal baselines: Nister's five-point and the seven-point solver, every solution and the chosen pose of every
 * pair (added within ABI 8: a pure addition, PNEC_HIP_ABI_VERSION is unchanged).  They are the `Nister5pt` and `7pt`
 * columns of the reference's `run_simulation -e`: EMPoseEstimation(..., NISTER | SEVENPT, ransac = false).  Steps 1-2
 * restate opengv's fivept_nister and sevenpt from memory ([EXT], as eightpt was); the conventions and steps 3-4 are those
 * of pnec_hip_eight_point.  Per pair with N correspondences:
 *  1 Sums and eigenvectors.  G = A'A and its cyclic Jacobi exactly as in the eight-point (same order, same stop, same
 *    skip rule).  The eigenvalues ascend as lambda_0..lambda_8 (the lowest index first among equal ones) with
 *    eigenvectors v0..v8.  NISTER: W = v0, Z = v1, Y = v2, X = v3, gap = (lambda_4 - lambda_3) / lambda_8.  SEVENPT:
 *    W = v0, X = v1, gap = (lambda_2 - lambda_1) / lambda_8.  W is the smallest eigenvalue's vector, as opengv's constant
 *    term is the last column of V: for noise-free pairs with N above the minimal count the true E lies in the span of the
 *    zero eigenvalues, and the parametrisation below would put it at infinity if W were the last vector of the basis.
 *  2a NISTER.  E(x, y, z) = xX + yY + zZ + W.  The ten cubics det E = 0 and the nine entries of 2 E E'E - tr(E E') E = 0
 *    give a 10 x 20 matrix in Nister's monomial order
 *      x3 y3 x2y xy2 x2z x2 y2z y2 xyz xy | xz2 xz x yz2 yz y z3 z2 z 1
 *    (rows: the nine entries row-major, then det E).  Gauss-Jordan with partial pivoting on the first ten columns, the
 *    lowest row wins a tie.  The rows k = <x2z> - z <x2>, l = <y2z> - z <y2>, m = <xyz> - z <xy> form the 3 x 3 matrix
 *    B(z) on (x, y, 1), entries of degree 3, 3, 4; p(z) = det B(z) has degree 10.  Its real roots come from a Sturm chain
 *    (p, p', negated remainders, each scaled by its largest coefficient; a polynomial whose leading coefficients are
 *    zero is taken at its actual degree): the roots lie within Cauchy's bound 1 + max |p_i / p_n|, their count is the
 *    difference of the sign changes at the two ends, root i is isolated by bisection on the count, 64 halvings in the
 *    integer order of the doubles.  x and y are the null vector of B(z): the cross product of two rows, the pair whose
 *    product is longest.  Polish: five Gauss-Newton steps on the ten cubics in (x, y, z), evaluated from E directly -- the
 *    derivative of det E along X is tr(adj(E) X), that of the nine entries 2 (X E'E + E X'E + E E'X) - 2 tr(E X') E -
 *    tr(E E') X; the 3 x 3 normal equations are solved by the adjugate.
 *  2b SEVENPT.  E(a) = W + aX, det E(a) = det W + tr(adj(W) X) a + tr(adj(X) W) a2 + det X a3; the real roots of the
 *    cubic by the same Sturm chain, each polished by two Newton steps on det.  1 or 3 solutions; they are fundamental
 *    matrices (s0 != s1), which the reference decomposes all the same.
 *  2c Every solution: e of unit norm with the sign that makes its entry of largest magnitude positive; the solutions in
 *    ascending order of e[0], then e[1], and so on (this does not depend on the basis of the null space, which is
 *    arbitrary when N is the minimal count).  out_n_solutions is their count, at most PNEC_HIP_EM_MAX_SOLUTIONS.
 *  3-4 Every solution i is decomposed as in step 3 of the eight-point into candidates j = 0..3; the quality of each over
 *    the first K = min(S, N) correspondences, S = 8 for NISTER and 9 for SEVENPT (common.cc:352-373), or over all N with
 *    PNEC_HIP_EM_QUALITY_ALL.  The lowest quality wins by strict < from 1e6 in the order (i, j); out_choice = 4 i + j.
 *  5 Status, pnec_hip_em_status.  TOO_FEW: N < 5 (NISTER), N < 7 (SEVENPT).  NOT_FINITE: as in the eight-point.
 *    NO_SOLUTION: no real root.  NO_CANDIDATE: no quality below 1e6.  A status other than OK writes NaN to q, t, E and
 *    singular and -1 to out_choice; TOO_FEW and NOT_FINITE write NaN to the other double outputs too and NO_SOLUTION to
 *    all but the gap; out_n_solutions is 0 for those three.
 *
 * Outputs for P pairs; every pointer may be NULL (not wanted), not all of them.
 *   out_q [P,4] xyzw   out_t [P,3] unit   out_E [P,9] the chosen solution   out_singular [P,3] of the chosen solution
 *   out_gap [P]   out_n_solutions int32 [P]   out_E_all [P,10,9], NaN beyond n_solutions
 *   out_quality [P,10,4], NaN beyond   out_choice int32 [P] = 4 i + j, or -1   out_status int32 [P]
 * A pair's bits depend on its own rows, on `algorithm` and on `flags` only (no atomics, fixed reduction order).
 *
 * All four problem modes, batches made by pnec_hip_problem_select(_view) and reshaped capacity batches included.  DEVICE
 * space: nothing waits, nothing is allocated, the call is asynchronous on `stream`.  HOST space: the outputs are staged
 * on the device (150 doubles and three ints per pair) and the call blocks.
 * NULL problem, an `algorithm` other than the two, a flag bit other than PNEC_HIP_EM_QUALITY_ALL, all outputs NULL or a
 * bad `space`: PNEC_HIP_ERR_INVALID_ARGUMENT before the handle is read or any device is touched. */
#define PNEC_HIP_EM_NISTER 1
#define PNEC_HIP_EM_SEVENPT 2
#define PNEC_HIP_EM_MAX_SOLUTIONS 10
#define PNEC_HIP_EM_QUALITY_ALL 1
typedef enum pnec_hip_em_status {
  PNEC_HIP_EM_OK = 0,
  PNEC_HIP_EM_TOO_FEW = 1,
  PNEC_HIP_EM_NOT_FINITE = 2,
  PNEC_HIP_EM_NO_CANDIDATE = 3,
  PNEC_HIP_EM_NO_SOLUTION = 4
} pnec_hip_em_status;
int pnec_hip_essential_minimal(pnec_hip_problem *p, int32_t algorithm, int32_t flags, double *out_q, double *out_t,
                               double *out_E, double *out_singular, double *out_gap, int32_t *out_n_solutions,
                               double *out_E_all, double *out_quality, int32_t *out_choice, int32_t *out_status,
                               int space, void *stream);

/* The RANSAC forms of the three closed-form baselines: a pose and an inlier mask per pair from its correspondences
 * alone, no start rotation (added within ABI 8: a pure addition, PNEC_HIP_ABI_VERSION is unchanged).  This is the
 * `ransac = true` branch of the reference's EMPoseEstimation (src/rel_pose_estimation/essential_matrix_methods.cc:56-75)
 * for NISTER, SEVENPT and EIGHTPT.  opengv's CentralRelativePoseSacProblem and sac::Ransac::computeModel are restated
 * from memory ([EXT]), with the constants of pnec_hip_ransac_eigensolver; rand() is that call's counter-based hash.
 * Per pair p with N correspondences, (m, S) = (5, 8) NISTER, (7, 9) SEVENPT, (8, 9) EIGHTPT (the reference's sample
 * sizes 5 + 3, 7 + 2, 8 + 1, common.cc:352-380):
 *  1 Sample of attempt a = 0, 1, 2, ...: the first S distinct indices min(floor(u N), N - 1) with
 *    u = rng_uniform(seed, first_pair_id + p, a, draw), draw = 0, 1, 2, ... -- the hash and the draw-until-distinct loop
 *    of pnec_hip_ransac_eigensolver; all 64 bits of `seed` enter.
 *  2 Model of an attempt.  Steps 1-3 of pnec_hip_essential_minimal (of pnec_hip_eight_point for EIGHTPT) on the sample's
 *    rows 0..m-1; step 4, the choice over the four candidates of every solution, sums the quality over all S rows of the
 *    sample in sample order.  The model is the chosen (R, unit t), R taking frame-2 vectors into frame 1.  An attempt has
 *    no model if its sums are not finite (a sample row holds a NaN or an infinity), if there is no real solution, or if
 *    no candidate's quality is below 1e6.
 *  3 Score.  A correspondence's score at a model is the quality term (1 - f1.r1) + (1 - f2.r2) of the midpoint
 *    triangulation (step 4 of pnec_hip_eight_point; opengv's reprojection error of CentralRelativePoseSacProblem [EXT]).
 *    Inlier iff score < threshold; a score that is not finite is no inlier.
 *  4 The sequential rule [EXT].  it = 0, a = 0, skipped = 0, k = 1, best = -1.  While it < k and
 *    skipped < 10 max_iterations: take attempt a, ++a; no model: ++skipped and go on (not an iteration -- unlike
 *    pnec_hip_ransac_eigensolver, where a capped hypothesis scores zero: here the first attempt may fail while k is 1);
 *    otherwise count its inliers c over all N rows; c > best: the attempt becomes the best, best = c, w = c / N,
 *    p_no = min(max(1 - w^S, 2^-52), 1 - 2^-52) (w^S by squaring), k = log(1 - 0.99) / log(p_no); ++it; it >
 *    max_iterations: stop.  No refit follows (essential_matrix_methods.cc:72-75 returns model_coefficients_ as it is).
 *  5 Status, pnec_hip_er_status.  TOO_FEW: N < S.  NO_MODEL: the rule ended with best = -1.  Both write NaN to the
 *    doubles, -1 to out_best_attempt and zeros to the mask and the count; TOO_FEW also 0 to out_iterations and
 *    out_attempts, NO_MODEL what the rule counted.
 *
 * Outputs for P pairs; every pointer may be NULL (not wanted), not all of them.
 *   out_q [P,4] xyzw, out_t [P,3] unit: the best attempt's model   out_E [P,9]: its chosen solution
 *   out_singular [P,3]: that solution's singular values
 *   out_inlier_mask uint8 [sum N], in the caller's correspondence order as pnec_hip_ransac_eigensolver writes it
 *   out_inlier_count int32 [P]: the mask's sum   out_iterations int32 [P]: it   out_attempts int32 [P]: a
 *   out_best_attempt int32 [P]: the index a of the winning attempt   out_status int32 [P]
 * A pair's bits depend on its own rows, `algorithm`, `seed`, first_pair_id + p, `max_iterations` and `threshold` only:
 * not on the batch around it and not on the memory space (no atomics, fixed reduction order).
 *
 * All four problem modes (only the six bearing planes are read); batches made by pnec_hip_problem_select(_view) and
 * reshaped capacity batches included.  DEVICE space: nothing waits, nothing is allocated, the call is asynchronous on
 * `stream`.  HOST space: the outputs are staged on the device and the call blocks.
 * NULL problem, an `algorithm` other than the three, max_iterations < 0, a threshold that is not finite and positive,
 * first_pair_id < 0, all outputs NULL or a bad `space`: PNEC_HIP_ERR_INVALID_ARGUMENT before the handle is read or any
 * device is touched. */
#define PNEC_HIP_EM_EIGHTPT 3 /* beside PNEC_HIP_EM_NISTER 1, PNEC_HIP_EM_SEVENPT 2: the values of algorithm_t */
typedef enum pnec_hip_er_status {
  PNEC_HIP_ER_OK = 0,
  PNEC_HIP_ER_TOO_FEW = 1,
  PNEC_HIP_ER_NO_MODEL = 2
} pnec_hip_er_status;
int pnec_hip_essential_ransac(pnec_hip_problem *p, int32_t algorithm, uint64_t seed, int64_t first_pair_id,
                              int32_t max_iterations, double threshold, double *out_q, double *out_t, double *out_E,
                              double *out_singular, uint8_t *out_inlier_mask, int32_t *out_inlier_count,
                              int32_t *out_iterations, int32_t *out_attempts, int32_t *out_best_attempt,
                              int32_t *out_status, int space, void *stream);

/* Relative scale between consecutive pairs from linked tracks (added within ABI 8: a pure addition,
 * PNEC_HIP_ABI_VERSION is unchanged).  Every pose carries t as a direction, so each pair is reconstructed with a
 * baseline of 1; a track seen in three consecutive frames has a depth from the shared middle camera in both
 * reconstructions, and the quotient of the two is the ratio of the baselines.
 *
 * `cur` holds the P pairs whose baseline is wanted, `prev` the pairs they are compared with: the same handle (a sequence
 * stored as consecutive pairs of one batch) or another handle on the same device; the modes need not be equal, only the
 * six bearing planes of either are read.  prev_pair int64 [P]: entry p is the pair of `prev` whose SECOND camera is pair
 * p's FIRST camera, or -1 if there is none (a value at or above prev's number of pairs is read as -1).  link int32
 * [sum N of cur], laid out by cur's own offsets: for correspondence i of pair p the index, within pair prev_pair[p] of
 * `prev`, of the same physical track; an entry below 0 or at / above that pair's count is "not linked"; duplicates are
 * allowed.  Poses: q_cur [P,4] / t_cur [P,3] one per pair of cur, q_prev / t_prev one per pair of prev, with the
 * conventions of pnec_hip_triangulate (q xyzw normalised inside, t a direction, t = 0 read as (0, 0, 1)); there is no
 * n_hyp.  The SIGN of t matters and this call does not vote: pass translations that put the structure in front, i.e.
 * out_t_oriented of pnec_hip_triangulate.
 *
 * Per link, with c the midpoint system (pnec_hip_triangulate's) of the correspondence in the current pair and r that of
 * the linked correspondence in the previous pair:
 *   ratio = (r.depth2 * sqrt(r.a11)) / (c.depth1 * sqrt(c.a00))        = |baseline_cur| / |baseline_prev|
 * (the depths multiply bearings that are not assumed unit: the square roots make both terms metric distances from the
 * shared camera).  A link is USED iff both systems are `front` at the poses given, both pass the parallax gate and
 * ratio is a positive finite number.  Parallax gate: min_parallax in radians, >= 0 and finite; 0 switches it off.  It
 * compares sin^2 psi = D / (a00 a11) with sin^2(min_parallax), as D >= sin^2(min_parallax) * (a00 a11) with D formed
 * from two rounded products as in pnec_hip_triangulate; and ONLY IF min_parallax > 0 it additionally requires a10 > 0
 * (a parallax below 90 degrees, without which sin^2 does not order angles).  min_parallax >= pi/2 leaves no link.
 *
 * Outputs; every pointer may be NULL (not wanted), not all of them.
 *   out_ratio double [sum N cur]   the value of a used link, NaN otherwise
 *   out_used  uint8  [sum N cur]   1 for a used link, else 0
 *   out_n_linked int32 [P]         links within range        out_n_used int32 [P]   links used (m below)
 *   out_scale double [P,3]         with the m used ratios in ascending order x_0 <= ... <= x_(m-1): the elements of rank
 *                                  (m-1)/4, (m-1)/2 and 3(m-1)/4 (integer division): lower quartile, lower median (THE
 *                                  SCALE) and upper quartile, each an element of the set, never an interpolation; NaN
 *                                  for m = 0.  log(q75 / q25) / 1.349 is a robust sigma of the scale's logarithm.
 * The order statistics are exact: a most-significant-digit-first radix selection over the 64-bit patterns (positive
 * finite doubles order as their patterns), no atomics on global memory, no sort.  A pair's outputs depend only on its
 * own data, its linked pair's data and the two poses: not on the batch it sits in, on `space`, or on prev == cur.
 * When out_ratio is NULL the ratios live in a workspace of 8 bytes * sum N that `cur` owns and keeps until it is
 * destroyed; calls on one handle that overlap in time must therefore pass out_ratio.
 *
 * Batches made by pnec_hip_problem_select(_view) and reshaped capacity batches are accepted on either side, positions
 * following each batch's own offsets and sizes.  DEVICE space: offsets and sizes are read on the device, nothing waits,
 * the call is asynchronous on `stream`.  HOST space: the call first resolves cur's sizes, stages in cur's staging buffer
 * (13 bytes per correspondence) and blocks.  A batch whose largest pair holds 4 GiB of planes or more:
 * PNEC_HIP_ERR_UNSUPPORTED.
 * NULL cur / prev / prev_pair / link / q_cur / t_cur / q_prev / t_prev, a negative, NaN or infinite min_parallax, all
 * outputs NULL or a bad `space`: PNEC_HIP_ERR_INVALID_ARGUMENT before a handle is read or any device is touched; after
 * that, two handles on different devices: PNEC_HIP_ERR_INVALID_ARGUMENT. */
int pnec_hip_relative_scale(pnec_hip_problem *cur, pnec_hip_problem *prev, const int64_t *prev_pair, const int32_t *link,
                            const double *q_cur, const double *t_cur, const double *q_prev, const double *t_prev,
                            double min_parallax, double *out_ratio, uint8_t *out_used, double *out_scale,
                            int32_t *out_n_linked, int32_t *out_n_used, int space, void *stream);

/* PNEC::Eigensolver with use_ransac_ = false (src/rel_pose_estimation/pnec.cc:273-278) for every
 * pair: rotation by opengv-style eigenvalue minimisation (Kneip-Lynen; opengv is not in the
 * reference tree, so the published algorithm is restated) started at init_q, translation by
 * TranslationFromM(ComposeM(...)) (src/common/common.cc:127-136,157-181, including ComposeM's
 * skipped first correspondence).  init_q [n_pairs,4] xyzw -> out_q [n_pairs,4], out_t [n_pairs,3]. */
int pnec_hip_nec_eigensolver(pnec_hip_problem *p, const double *init_q, double *out_q, double *out_t,
                             int space, void *stream);

/* PNEC::Eigensolver with use_ransac_ = true (src/rel_pose_estimation/pnec.cc:239-272): RANSAC over
 * eigensolver hypotheses from `sample_size` random correspondences (Options::ransac_sample_size_ = 10),
 * at most `max_iterations` (Options::max_ransac_iterations_ = 5000) with the adaptive bound for 99 %
 * confidence, inlier threshold on the midpoint-triangulation reprojection score (1e-6 in the
 * reference, pnec.cc:248), eigensolver re-run on the inliers, translation by
 * TranslationFromM(ComposeM(inliers)).  opengv::sac::Ransac is restated (opengv is not in the tree);
 * its rand() draws are replaced by a counter-based hash of (seed, pair, hypothesis, draw).
 * out_inlier_mask [sum N] (1 = inlier, in the caller's correspondence order), out_inlier_count
 * [n_pairs], out_ransac_iterations [n_pairs] may each be NULL.  Pairs with fewer than sample_size
 * correspondences fall back to the plain eigensolver with every correspondence an inlier.
 * sample_size > PNEC_HIP_MAX_RANSAC_SAMPLE (16) returns PNEC_HIP_ERR_UNSUPPORTED. */
int pnec_hip_ransac_eigensolver(pnec_hip_problem *p, const double *init_q, uint64_t seed,
                                int32_t max_iterations, int32_t sample_size, double threshold, double *out_q,
                                double *out_t, uint8_t *out_inlier_mask, int32_t *out_inlier_count,
                                int32_t *out_ransac_iterations, int space, void *stream);

/* PNEC::InlierExtraction (src/rel_pose_estimation/pnec.cc:210-229): a new batch holding, pair by pair
 * and in order, the correspondences whose mask byte is non-zero.  Done on the device: DEVICE-space calls
 * are asynchronous on `stream` and nothing is read back -- the new batch keeps the source's capacity and
 * its pair sizes stay in HBM until a host-side number is asked for (pnec_hip_problem_offsets /
 * _num_correspondences / _max_correspondences / _payload_bytes wait for the stream and fetch them).
 * HOST-space calls block (the caller may reuse `mask` on return). */
int pnec_hip_problem_select(pnec_hip_problem *src, const uint8_t *mask, int space, void *stream,
                            pnec_hip_problem **out);

/* The same InlierExtraction into the batch's CACHED target (the one pnec_hip_solve_pipeline compacts into): nothing is
 * allocated after the first call on `src`, nothing is to be destroyed.  *out is owned by `src` and valid until the next
 * select_view / solve_pipeline on `src`, a re-shape that outgrows it, or src's destruction.  For callers that run the
 * stages of PNEC::Solve one by one per frame (the timed overloads, pnec.cc:135-208) on a persistent batch. */
int pnec_hip_problem_select_view(pnec_hip_problem *src, const uint8_t *mask, int space, void *stream,
                                 pnec_hip_problem **out);

/* PNEC::WeightedEigensolver (src/rel_pose_estimation/pnec.cc:283-348) for every pair of a
 * TARGET-mode problem: (weighted_iterations - 1) rounds of { weights from the INITIAL pose x 1e-8,
 * eigensolver on the weighted bearings, 500-direction Fibonacci search of obj_fun
 * (src/optimization/scf.cc:43-72), 10 scf steps (scf.cc:128-148) }.  Options::weighted_iterations_
 * is 10 in the reference. */
int pnec_hip_weighted_eigensolver(pnec_hip_problem *p, const double *init_q, const double *init_t,
                                  double reg, int32_t weighted_iterations, double *out_q, double *out_t,
                                  int space, void *stream);

/* ---- the whole PNEC::Solve chain, device-resident ------------------------------------------------
 * pnec::rel_pose_estimation::Options as PNEC::Solve reads it (include/rel_pose_estimation/pnec_config.h:
 * 46-65; pnec.cc:87,96,97,105,109,116,239,246,249,300,327,367).  Fill with
 * pnec_hip_default_pipeline_options() (the reference's defaults). */
typedef struct pnec_hip_pipeline_options {
  int32_t use_ransac;            /* 1     Options::use_ransac_ */
  int32_t use_nec;               /* 0     Options::use_nec_ */
  int32_t use_ceres;             /* 1     Options::use_ceres_ */
  int32_t weighted_iterations;   /* 10    Options::weighted_iterations_ */
  int32_t max_ransac_iterations; /* 5000  Options::max_ransac_iterations_ */
  int32_t ransac_sample_size;    /* 10    Options::ransac_sample_size_ (<= PNEC_HIP_MAX_RANSAC_SAMPLE) */
  int64_t first_pair_id;         /* 0     RANSAC draws: pair p of the batch samples as pair first_pair_id + p, so a
                                          rank that solves pairs [a, b) of a larger set passes a and the results do
                                          not depend on how the set was sharded (>= 0; ABI 2 had reserved[2] here) */
  double regularization;         /* 1e-13 Options::regularization_ */
  double ransac_threshold;       /* 1e-6  pnec.cc:248 */
  uint64_t ransac_seed;          /* 1     counter-based draws (see pnec_hip_ransac_eigensolver) */
  pnec_hip_options solver;       /* the refinement's ceres::Solver::Options; PNEC::CeresSolver and
                                    NECCeresSolver default-construct theirs (pnec.cc:355,399) */
  int32_t eigensolver_scheme;    /* 0     pnec_hip_eigensolver_scheme: which iteration every eigenvalue minimisation of
                                          the chain runs (ABI 5) */
  int32_t ransac_flags;          /* 0     PNEC_HIP_RANSAC_* bits (ABI 7; `reserved` until ABI 6); an undefined bit:
                                          PNEC_HIP_ERR_INVALID_ARGUMENT */
} pnec_hip_pipeline_options;
void pnec_hip_default_pipeline_options(pnec_hip_pipeline_options *opt);

/* PNEC::Solve (src/rel_pose_estimation/pnec.cc:77-124) for every pair of a batch: Eigensolver (with
 * RANSAC when use_ransac) -> InlierExtraction -> NECCeresSolver (use_nec) or WeightedEigensolver +
 * CeresSolver, each stage one launch over the batch on `stream`, the stages handing their results to
 * each other in HBM (no host round trip, no allocation after the first call on a batch).
 *   init_q [n_pairs,4] xyzw, init_t [n_pairs,3]   initial_pose per pair
 *   out_q [n_pairs,4], out_t [n_pairs,3]          the pose Solve returns
 *   out_inlier_mask [sum N] / out_inlier_count [n_pairs]  the `inliers` of the four-argument overload
 *                                                 (all zero without RANSAC: inliers.clear()); may be NULL
 * TARGET-mode problems (use_nec also accepts NEC-mode ones).  space as in pnec_hip_solve. */
int pnec_hip_solve_pipeline(pnec_hip_problem *p, const double *init_q, const double *init_t,
                            const pnec_hip_pipeline_options *opt, double *out_q, double *out_t,
                            uint8_t *out_inlier_mask, int32_t *out_inlier_count, int space, void *stream);

/* Launch-order hint of the RANSAC stage (opt-in, scheduling only: results never depend on it).  A launch ends with
 * its slowest wavefronts: the pairs that need a second and third round of hypotheses (about a tenth at 10 % outliers)
 * run two to three times as long as the rest and end the launch late when they are dispatched late.  With the hint
 * enabled the batch remembers every pair's RANSAC hypothesis count of the last call that ran RANSAC on it
 * (pnec_hip_ransac_eigensolver, pnec_hip_solve_pipeline) and the next call on the same number of pairs dispatches
 * the pairs that went beyond one round first, each sharing its wavefront with one that did not.  Meaningful when
 * pair i of the next call is pair i of this one again (other start poses, other seeds, a benchmark loop) or its
 * successor in a stream of frames (sequence i's next frame pair: outlier ratios persist from frame to frame); a
 * stale hint costs nothing but the gain.  The reference has no counterpart (opengv's RANSAC runs one pair at a
 * time, pnec.cc:231-281). */
int pnec_hip_problem_launch_order_hint(pnec_hip_problem *p, int32_t enable);

/* ---- several GPUs of one node, one process ----------------------------------------------------------------
 * The reference fans out at process level (scripts/run_simulation.sh:52-67, scripts/parallel_kitti.sh:60-69: one
 * process per experiment / sequence).  Frame pairs are independent, so a batch shards with no data-path exchange:
 * pnec_hip_partition gives contiguous ranges of pairs balanced by correspondence count (bounds[n_parts + 1]; part r
 * owns pairs [bounds[r], bounds[r+1]) -- the rule the multi-process bench uses, pnec_amd/distributed.py::partition);
 * pnec_hip_solve_pipeline_multi runs PNEC::Solve (as pnec_hip_solve_pipeline) on one batch per entry of `devices`,
 * one host thread and one stream each, from HOST arrays in the reference layout (as pnec_hip_problem_fill: bvs 3
 * doubles, covs 9 doubles column-major per correspondence, NULL covs = NEC-only data for use_nec) and writes every
 * pair's result into the caller's arrays; it returns when all shards are done.  A device may be listed more than
 * once.  RANSAC draws belong to the GLOBAL pair index, so the results do not depend on the device list. */
int pnec_hip_partition(int64_t n_pairs, const int64_t *offsets, int32_t n_parts, int64_t *bounds);
int pnec_hip_solve_pipeline_multi(int32_t n_devices, const int32_t *devices, int64_t n_pairs, const int64_t *offsets,
                                  const double *bvs1, const double *bvs2, const double *covs, const double *init_q,
                                  const double *init_t, const pnec_hip_pipeline_options *opt, double *out_q,
                                  double *out_t, uint8_t *out_inlier_mask, int32_t *out_inlier_count);

/* The persistent form (ABI 5): a handle that keeps one capacity-shaped batch and one stream per listed device alive, for
 * callers that solve batch after batch -- the one-shot call above creates, fills and destroys a batch per device per
 * call.  What north_star shards is the refinement (PNECCeres::Optimize over independent frame pairs), so the handle has
 * it (pnec_hip_multi_solve = pnec_hip_solve per shard, multi-hypothesis starts included) next to the whole chain
 * (pnec_hip_multi_solve_pipeline = pnec_hip_solve_pipeline per shard).
 *   create  devices[n_devices] (a device may be listed more than once); mode as pnec_hip_problem_create; the handle holds
 *           up to max_pairs pairs / max_corr correspondences in total, no pair larger than max_pair_corr (each device's
 *           batch is sized for max_corr / n_devices + max_pair_corr: what a partition balanced by correspondence count
 *           can give it).
 *   fill    HOST arrays in the reference layout (as pnec_hip_problem_fill); partitions the pairs (pnec_hip_partition),
 *           re-shapes the device batches in place and uploads every shard from a host thread of its own.
 *   solve / solve_pipeline   HOST arrays; every shard on its device and stream, side by side; return when all are done.
 *           Results do not depend on the device list (RANSAC draws belong to the GLOBAL pair index).
 * After the first call of each kind nothing is allocated (pnec_hip_alloc_counters counts the library's hipMalloc calls).
 * Not thread-safe: one handle per calling thread. */
typedef struct pnec_hip_multi pnec_hip_multi;
int pnec_hip_multi_create(int32_t n_devices, const int32_t *devices, int mode, int64_t max_pairs, int64_t max_corr,
                          int64_t max_pair_corr, pnec_hip_multi **out);
int pnec_hip_multi_destroy(pnec_hip_multi *m);
int32_t pnec_hip_multi_num_devices(const pnec_hip_multi *m);
int pnec_hip_multi_bounds(const pnec_hip_multi *m, int64_t *bounds /* [n_devices + 1]: the current partition */);
int pnec_hip_multi_fill(pnec_hip_multi *m, int64_t n_pairs, const int64_t *offsets, const double *bvs1, const double *bvs2,
                        const double *covs, const double *covs_host);
int pnec_hip_multi_solve(pnec_hip_multi *m, const double *init_q, const double *init_t, int32_t n_hyp, const double *hyp_t,
                         double reg, const pnec_hip_options *opt, double *out_q, double *out_t, double *out_cost,
                         int32_t *out_iterations, int32_t *out_status);
int pnec_hip_multi_solve_pipeline(pnec_hip_multi *m, const double *init_q, const double *init_t,
                                  const pnec_hip_pipeline_options *opt, double *out_q, double *out_t,
                                  uint8_t *out_inlier_mask, int32_t *out_inlier_count);

/* ---- streaming: one frame pair (or a few) per call, as the reference's odometry calls the solver ----
 * (Frame2Frame::PNECAlign -> PNEC::Solve once per frame, src/rel_pose_estimation/frame2frame.cc:122-141;
 * PNECCeres::Optimize once per pybind call, python/pypnec.cpp:55-65.)  A handle owns `slots` staging
 * slots in pinned, device-mapped host memory and one HIP stream; nothing is allocated per call.
 *   submit  copies the caller's reference-layout arrays (as in pnec_hip_problem_fill; offsets[n_pairs+1]
 *           with offsets[0] == 0) and start poses into a free slot and launches ONE kernel that reads
 *           them over PCIe, runs InitValues + Optimize + Result on chip and writes the result records
 *           back into the slot; returns a ticket at once.  Up to `slots` tickets may be outstanding; with
 *           every slot holding an uncollected ticket submit returns PNEC_HIP_ERR_BUSY (collect the oldest
 *           with wait first: nothing is ever dropped).  Pairs beyond the register-resident geometries (> 4096 correspondences; > 2048
 *           for SYM) are staged through a batch owned by the handle instead.
 *   poll    done = 1 once the ticket's results are in host memory (never blocks).
 *   wait    blocks (polling a flag the kernel raises -- no stream synchronisation), copies the results
 *           out (any pointer may be NULL) and frees the slot.  Tickets must be collected with wait.
 * max_corr / max_pairs bound ONE submit.  stream: NULL = a stream of the handle's own.
 * A handle is not thread-safe; use one per thread. */
typedef struct pnec_hip_stream pnec_hip_stream;
int pnec_hip_stream_create(int device, int32_t max_corr, int32_t max_pairs, int32_t slots, void *stream,
                           pnec_hip_stream **out);
int pnec_hip_stream_destroy(pnec_hip_stream *s);
int pnec_hip_stream_submit(pnec_hip_stream *s, int mode, int64_t n_pairs, const int64_t *offsets,
                           const double *bvs1, const double *bvs2, const double *covs, const double *covs_host,
                           const double *init_q, const double *init_t, double reg, const pnec_hip_options *opt,
                           int64_t *ticket);
int pnec_hip_stream_poll(pnec_hip_stream *s, int64_t ticket, int32_t *done);
int pnec_hip_stream_wait(pnec_hip_stream *s, int64_t ticket, double *out_q, double *out_t, double *out_cost,
                         int32_t *out_iterations, int32_t *out_status);

/* ---- per-frame PNEC::Solve: the WHOLE chain for one frame pair per call, nothing allocated per call ----
 * (Frame2Frame::PNECAlign -> PNEC::Solve, src/rel_pose_estimation/frame2frame.cc:122-141 -> pnec.cc:77-124.)
 * A handle owns a pinned, device-mapped staging block, a capacity-shaped batch of one pair (TARGET family) with
 * its cached scratch / InlierExtraction target / side stream, and one HIP stream.
 *   solve   bvs1, bvs2 [n,3], covs [n,9] column-major (may be NULL with use_nec), start pose (q xyzw, t) in HOST
 *           memory -> pose out, inlier mask [n] and count (either may be NULL; zeros without RANSAC).  Runs
 *           pnec_hip_solve_pipeline on the handle's batch -- the same launches as the batch call, so the result
 *           is bit-identical to pnec_hip_solve_pipeline on a one-pair batch -- and returns when it is done.
 *   load    only the ingest (arrays -> SoA planes of the handle's batch, asynchronous on the handle's stream);
 *           *problem is the handle's batch, valid until the next load / solve / destroy, for callers that run the
 *           stages one by one (the timed PNEC::Solve overloads, pnec.cc:135-208) on pnec_hip_frame_stream().
 *           The caller's arrays are copied into the handle's pinned staging block before load returns (they may be
 *           reused at once); load first waits for everything queued earlier on the handle's stream, because the
 *           previous ingest reads that staging block when it executes -- two loads in a row are safe, not overlapped.
 * n <= max_corr (pnec_hip_frame_capacity).  Not thread-safe: one handle per thread. */
typedef struct pnec_hip_frame pnec_hip_frame;
int pnec_hip_frame_create(int device, int64_t max_corr, void *stream, pnec_hip_frame **out);
int pnec_hip_frame_destroy(pnec_hip_frame *f);
int64_t pnec_hip_frame_capacity(const pnec_hip_frame *f);
void *pnec_hip_frame_stream(const pnec_hip_frame *f);
int pnec_hip_frame_load(pnec_hip_frame *f, int64_t n, const double *bvs1, const double *bvs2, const double *covs,
                        pnec_hip_problem **problem);
int pnec_hip_frame_solve(pnec_hip_frame *f, int64_t n, const double *bvs1, const double *bvs2, const double *covs,
                         const double *init_q, const double *init_t, const pnec_hip_pipeline_options *opt,
                         double *out_q, double *out_t, uint8_t *out_inlier_mask, int32_t *out_inlier_count);

/* Input side of the path: pnec::common::UnscentedTransform (src/common/common.cc:467-525) and
 * pnec::common::Unproject (:460-465) for n keypoints at once -- what KeyPoint::Unproject
 * (src/frames/keypoints.cc:49-62) and the simulator's GetFeatures (src/simulation/sim_common.cc:72-107)
 * do per point.  mu [n,3] image points (x, y, 1) [or (x, y, f) with K_inv = I], covs [n,9]
 * column-major 3x3 whose top-left 2x2 is the image-plane covariance (omnidirectional: the
 * tangent-plane covariance rotated to the bearing), K_inv [9] column-major, kappa (1.0 in the
 * reference), camera_model 0 = Omnidirectional, 1 = Pinhole (enum CameraModel, common.h:62).
 * out_covs [n,9] bearing covariances, exactly symmetric (mirror entries carry the same bits); out_bvs [n,3] unit
 * bearings or NULL. */
int pnec_hip_unscented_transform(int64_t n, const double *mu, const double *covs, const double *K_inv,
                                 double kappa, int camera_model, double *out_bvs, double *out_covs,
                                 int space, int device, void *stream);

/* Patch covariances: the 2x2 image covariance of keypoints from the image patches around them (added within ABI 8: a
 * pure addition, PNEC_HIP_ABI_VERSION is unchanged) -- the cov2 / cov1 input of pnec_hip_problem_fill_keypoints, in its
 * layout.  It is the quantity POpticalFlowPatch::setFromImage keeps as `Cov` (include/features/tracking/pnec_patch.h:
 * 78-137: the top-left 2x2 block of the inverse of the patch's SE(2) Gauss-Newton Hessian) after KLTPatchOpticalFlow has
 * divided it by uncertainty_scaling and rotated it by the tracked transform (klt_patch_optical_flow.h:244-252,375-382).
 * This is NOT tracking: no KLT iteration, no pyramid, no detection; positions come from the caller's tracker, or from
 * pnec_hip_patch_track below, which is.  Level 0
 * only (the reference's min_level): for another level pass the downsampled image and the scaled positions.
 * ALL ARITHMETIC IS DOUBLE.  The reference computes in float; its float bits are not reproduced and not claimed.
 * [EXT] basalt's image.h / patterns.h are not in the reference tree: interpGrad, InBounds and Pattern52 below are
 * restated from the published code, and what follows is this library's own definition.
 *
 * Input.
 *   images      n_images images of height x width pixels, row-major, `pitch` ELEMENTS from one row to the next
 *               (pitch >= width), image f starting at element f * height * pitch; the last row of the last image
 *               need only hold `width` elements.  pixel_type: pnec_hip_pixel_type.
 *   offsets     int64 [n_images + 1], non-decreasing, offsets[0] = 0, offsets[n_images] = n_points: keypoints
 *               [offsets[f], offsets[f+1]) lie in image f (ragged; an image may have none).
 *   pts         double [n_points, 2]: x = column, y = row, pixel centres at integers.
 *   pattern     double [n_pattern, 2] offsets in pixels, 1 <= n_pattern <= PNEC_HIP_PATCH_MAX_POINTS (64).  The
 *               reference's is Pattern52 [EXT]: 0.5 * raw, raw rows y = 7, 5 .. -7, x ascending in steps of 2 over
 *               +-3, +-5, +-7, +-7, +-7, +-7, +-5, +-3 (52 points; pnec_amd.PATTERN52, pnec::features::Pattern52()).
 *   scaling     > 0 (the reference's uncertainty_scaling is 10).
 *   angle       double [n_points] or NULL: rotation of the tracked transform in radians, |angle| < 1e6.
 *
 * Per pattern point i: p = pos + pattern[i].  The point is VALID iff 2 <= p.x < width - 3 and 2 <= p.y < height - 3
 * (InBounds(p, 2) for floating coordinates; a NaN coordinate is invalid).  With ix = floor(p.x), dx = p.x - ix,
 * ddx = 1 - dx (the same in y) and B(u, v) = ((ddx ddy I(u,v) + ddx dy I(u,v+1)) + dx ddy I(u+1,v)) + dx dy I(u+1,v+1):
 *   d_i = B(ix, iy),  gx_i = 0.5 (B(ix+1, iy) - B(ix-1, iy)),  gy_i = 0.5 (B(ix, iy+1) - B(ix, iy-1))
 * -- twelve distinct pixels, all inside the image by the validity rule.
 * Per keypoint (pnec_patch.h:101-135 term by term): n = number of valid points, S = sum d_i, G = sum g_i,
 *   g'_i = n (g_i S - G d_i) / S^2 for a valid point, 0 for an invalid one;  r_i = -pat_y g'x_i + pat_x g'y_i;
 *   J_i = (g'x_i, g'y_i, r_i);  H = sum J_i' J_i (3x3);  Sigma = (H^-1)[0:2, 0:2] / scaling, and with an angle
 *   Sigma <- R(angle) Sigma R(angle)', R = [c -s; s c].
 * H^-1 as pnec_hip_pose_covariance does it: the Cholesky factor of the Jacobi-scaled matrix diag(H)^-1/2 H diag(H)^-1/2.
 * Order of every sum, fixed by the pattern's order alone: pattern point i belongs to position i mod 16; a position adds
 * its points in ascending i; the 16 positions are then added pairwise: j with j^1, then with j^2, then with 7 - j inside
 * each half, then with 15 - j.  No atomics: a keypoint's bits depend on its own image, position, pattern, scaling and
 * angle only -- not on the call it sits in, nor on `space`.
 *
 * Outputs, per keypoint; every pointer may be NULL (not wanted), not all of them.
 *   out_cov     double [n_points, 3]  Sigma as (xx, xy, yy): what pnec_hip_problem_fill_keypoints takes as cov2 / cov1
 *   out_hessian double [n_points, 6]  H * scaling, upper triangle (00 01 02 11 12 22)
 *   out_mean    double [n_points]     S / n
 *   out_n_valid int32  [n_points]     n
 *   out_status  int32  [n_points]     pnec_hip_patch_status: 0; PNEC_HIP_PATCH_EMPTY when n = 0 or S is not positive and
 *               finite; PNEC_HIP_PATCH_SINGULAR on a non-positive pivot (a constant image, a ramp), a non-finite
 *               inverse or n < 3 (H then has rank below 3, whatever sign rounding gives the last pivot).  In both error
 *               cases out_cov is NaN and out_hessian holds what the arithmetic gave.
 * DEVICE space: every pointer (images, offsets, pts, pattern, angle, outputs) is device memory of `device`, nothing
 * waits, the call is asynchronous on `stream`, and an offsets array that breaks the rules above cannot make the kernel
 * read outside the images (the image index is clamped).  HOST space: the arrays are staged, offsets are checked, the
 * call blocks.  n_points = 0 returns at once.
 * PNEC_HIP_ERR_INVALID_ARGUMENT: NULL images / offsets / pts / pattern, all outputs NULL, n_pattern outside 1..64, an
 * unknown pixel_type, n_images < 1, width or height < 1, pitch < width, n_points < 0, scaling not positive and finite,
 * a bad `space`; in HOST space also offsets that break the rules above. */
#define PNEC_HIP_PATCH_MAX_POINTS 64
typedef enum pnec_hip_pixel_type {
  PNEC_HIP_PIXEL_U8 = 0,
  PNEC_HIP_PIXEL_U16 = 1,
  PNEC_HIP_PIXEL_F32 = 2
} pnec_hip_pixel_type;
typedef enum pnec_hip_patch_status {
  PNEC_HIP_PATCH_OK = 0,
  PNEC_HIP_PATCH_EMPTY = 1,
  PNEC_HIP_PATCH_SINGULAR = 2
} pnec_hip_patch_status;
int pnec_hip_patch_covariance(const void *images, int pixel_type, int64_t n_images, int32_t height, int32_t width,
                              int64_t pitch, const int64_t *offsets, int64_t n_points, const double *pts,
                              const double *pattern, int32_t n_pattern, double scaling, const double *angle,
                              double *out_cov, double *out_hessian, double *out_mean, int32_t *out_n_valid,
                              int32_t *out_status, int space, int device, void *stream);

/* Patch tracking: the pyramidal SE(2) KLT iteration of KLTPatchOpticalFlow with its forward-backward check, and the
 * halving step of the image pyramid it runs on (added within ABI 8: pure additions, PNEC_HIP_ABI_VERSION is unchanged).
 * This is the producer of pnec_hip_patch_covariance's positions and of its `angle`: trackPoints / trackPoint /
 * trackPointAtLevel (include/features/tracking/klt_patch_optical_flow.h:195-342) and POpticalFlowPatch::residual
 * (pnec_patch.h:139-170) on top of setFromImage as restated above.  The view graph and stereo filtering are NOT here;
 * FAST detection on the grid is pnec_hip_detect_keypoints, keypoint ids and the tracks' bookkeeping pnec_hip_tracks_* below.  ALL ARITHMETIC IS DOUBLE; the
 * reference's float bits are not reproduced and not claimed.  [EXT] basalt's image.h (interp, InBounds), image_pyr.h (the pyramid) and Sophus (SE2::exp) are not in the
 * reference tree: they are restated from the published code, and what follows is this library's own definition.
 *
 * --- pnec_hip_image_pyramid_level: one halving step.
 * in: n_images images of height x width pixels in pnec_hip_patch_covariance's layout (pitch_in elements per row); out:
 * n_images images of (height / 2) x (width / 2) pixels (floor), pitch_out elements per row, image f at element
 * f * (height / 2) * pitch_out.  height, width >= 4.  With k = [1 4 6 4 1] and r(i, n) the reflection about the border
 * pixels that does not repeat them (-1 -> 1, -2 -> 2, n -> n - 2, n + 1 -> n - 3):
 *   out(x, y) = sum_j k_j ( sum_i k_i I(r(2x + i - 2, width), r(2y + j - 2, height)) ) / 256,   i, j = 0 .. 4,
 * the inner sum first, both sums in ascending index.  U8 and U16 in integer arithmetic, (sum + 128) >> 8; F32 sums in
 * double (every product is exact, so a fused multiply-add gives the same bits), divides by 256 and rounds once to float.
 * DEVICE space: asynchronous on `stream`; HOST space: staged, the call blocks.
 * PNEC_HIP_ERR_INVALID_ARGUMENT: NULL in / out, an unknown pixel_type, n_images < 1, height or width < 4, a pitch below
 * its width, a bad `space`.
 *
 * --- pnec_hip_patch_track.
 * Input.
 *   tmpl, prev, next   three pyramids: where the patches are built, and the two images of the track (forward in `next`,
 *               backward in `prev`).  Each is a HOST array of n_levels pointers, 1 <= n_levels <=
 *               PNEC_HIP_TRACK_MAX_LEVELS (8), with a HOST array of n_levels pitches in elements; the buffers the
 *               pointers name live in `space`.  Level l holds n_images images of (height >> l) x (width >> l) pixels in
 *               pnec_hip_patch_covariance's layout; the smallest level must still be 4 pixels in each direction.  prev
 *               (and prev_pitch) may be NULL, meaning tmpl.
 *   offsets     as in pnec_hip_patch_covariance.
 *   tmpl_pts    double [n_points, 2]: where the patch is built, in level-0 pixels; level l uses tmpl_pts / 2^l
 *               (klt_patch_optical_flow.h:365-368).
 *   init_pts, init_angle   double [n_points, 2] / [n_points]: the transform in `prev` (translation in level-0 pixels,
 *               rotation in radians, |angle| < 1e6); NULL means tmpl_pts / 0.
 *   shift_x, shift_y   the reference's `offset`, added to the start of the forward track.
 *   pattern, n_pattern, scaling   as in pnec_hip_patch_covariance.
 *   max_iterations   1 .. 255 per level (the reference's configurations use 40, with 4 + 1 levels).
 *   max_recovered_dist2   >= 0, in square pixels (the reference's 0.04).
 *   flags       PNEC_HIP_TRACK_NO_BACKWARD: the forward track alone.
 *
 * The template of a keypoint at level l is pnec_hip_patch_covariance's patch of tmpl's level l at q = tmpl_pts / 2^l,
 * sums and order as stated there: validity t_i, d_i, n1, S1, g'_i, J_i, H.  In addition data_i = (n1 d_i) / S1 and
 * K_i = H^-1 J_i' with the FULL 3x3 inverse from the same Cholesky factor of the Jacobi-scaled H; K_i = 0 for a point
 * that is not valid.  A template that pnec_hip_patch_covariance would call EMPTY or SINGULAR (or whose inverse is not
 * finite in all entries) is BAD.
 * One iteration at level l (size w_l x h_l) from the transform (t, theta), t in that level's pixels:
 *   p_i = (c pat_x - s pat_y + t_x, s pat_x + c pat_y + t_y), (c, s) = (cos, sin) theta; p_i is valid by the rule above
 *   v_i = B(floor p_i) as above (four pixels) for a valid point, 0 otherwise;  n2 = number valid;  S2 = sum v_i
 *   r_i = (n2 v_i) / S2 - data_i where t_i and p_i is valid, 0 otherwise;  m = the number of such points
 *   the track is LOST, the transform unchanged, if m <= n_pattern / 2 (integer division) or S2 is not positive and finite
 *   inc = -sum_i K_i r_i;   d = inc_2;   a = sin d / d, b = (1 - cos d) / d, for |d| < 1e-10 a = 1 - d^2 / 6, b = d / 2
 *   u = (a inc_0 - b inc_1, b inc_0 + a inc_1);   t += (c u_x - s u_y, s u_x + c u_y);   theta += d       [T <- T exp(inc)]
 *   the track is LOST, the transform updated, if not (2 <= t_x < w_l - 3 and 2 <= t_y < h_l - 3) or |d| or |theta| has
 *   reached 1e6 (the domain of the library's sine and cosine; no reference track comes near it).
 * Every sum over the pattern runs in pnec_hip_patch_covariance's order.
 * One direction: for l = n_levels - 1 .. 0: if the template of level l is BAD, stop with BAD_TEMPLATE at level l;
 * t /= 2^l; max_iterations iterations (there is no convergence test: the reference has none); t *= 2^l -- also after a
 * loss at that level, which ends the direction.
 * Per keypoint: forward from (init_pts + shift, init_angle) in `next`; its result is the OUTPUT transform.  Unless
 * NO_BACKWARD: backward from (output - shift, output angle) in `prev` with the same templates, then
 * dist2 = (init_x - rec_x)^2 + (init_y - rec_y)^2 and the track is RECOVERED_TOO_FAR unless dist2 < max_recovered_dist2
 * (strict, klt_patch_optical_flow.h:238-242).  The first event in this order decides the status.
 *
 * Outputs, per keypoint; every pointer may be NULL (not wanted), not all of them.
 *   out_pts     double [n_points, 2]  the output transform's translation: where the forward track stood last, also when
 *   out_angle   double [n_points]     lost (a track lost backward keeps its forward result) -- and its rotation
 *   out_cov     double [n_points, 3]  R(out_angle) Sigma_0 R' / scaling of the level-0 template; NaN unless the status
 *               is OK.  Bit for bit what pnec_hip_patch_covariance(tmpl level 0, tmpl_pts, angle = out_angle) returns.
 *   out_dist2   double [n_points]     dist2; NaN when the backward track was not run to its end
 *   out_status  int32  [n_points]     pnec_hip_track_status
 *   out_lost_level int32 [n_points]   the level of BAD_TEMPLATE, LOST_FORWARD or LOST_BACKWARD; -1 otherwise
 * A keypoint's bits depend on its own images, positions, pattern and parameters only -- not on the call it sits in, nor
 * on `space`, nor on the pixel type the same values are stored in.
 * DEVICE space: the level buffers and every array but the pointer and pitch arrays are device memory of `device`,
 * nothing waits, the call is asynchronous on `stream` (the pointer and pitch arrays are read before it returns), and
 * the image index is clamped as in pnec_hip_patch_covariance.  HOST space: everything is staged, offsets are checked,
 * the call blocks.  n_points = 0 returns at once.
 * PNEC_HIP_ERR_INVALID_ARGUMENT: NULL tmpl / next / a pitch array / a level pointer / offsets / tmpl_pts / pattern, all
 * outputs NULL, n_levels outside 1..8, max_iterations outside 1..255, n_pattern outside 1..64, an unknown pixel_type or
 * flag, n_images < 1, n_points < 0, a level smaller than 4 pixels, a pitch below its level's width, max_recovered_dist2
 * negative or NaN, shift or scaling not finite (scaling not positive), a bad `space`; in HOST space also bad offsets. */
#define PNEC_HIP_TRACK_MAX_LEVELS 8
#define PNEC_HIP_TRACK_NO_BACKWARD 1u
typedef enum pnec_hip_track_status {
  PNEC_HIP_TRACK_OK = 0,
  PNEC_HIP_TRACK_BAD_TEMPLATE = 1,
  PNEC_HIP_TRACK_LOST_FORWARD = 2,
  PNEC_HIP_TRACK_LOST_BACKWARD = 3,
  PNEC_HIP_TRACK_RECOVERED_TOO_FAR = 4
} pnec_hip_track_status;
int pnec_hip_image_pyramid_level(const void *in, void *out, int pixel_type, int64_t n_images, int32_t height,
                                 int32_t width, int64_t pitch_in, int64_t pitch_out, int space, int device,
                                 void *stream);
int pnec_hip_patch_track(const void *const *tmpl, const int64_t *tmpl_pitch, const void *const *prev,
                         const int64_t *prev_pitch, const void *const *next, const int64_t *next_pitch,
                         int32_t n_levels, int pixel_type, int64_t n_images, int32_t height, int32_t width,
                         const int64_t *offsets, int64_t n_points, const double *tmpl_pts, const double *init_pts,
                         const double *init_angle, double shift_x, double shift_y, const double *pattern,
                         int32_t n_pattern, int32_t max_iterations, double max_recovered_dist2, uint32_t flags,
                         double scaling, double *out_pts, double *out_angle, double *out_cov, double *out_dist2,
                         int32_t *out_status, int32_t *out_lost_level, int space, int device, void *stream);

/* Keypoint detection: grid FAST-9 corners (added within ABI 8: a pure addition, PNEC_HIP_ABI_VERSION is unchanged).
 * This is the producer of pnec_hip_patch_track's tmpl_pts: what KLTPatchOpticalFlow::addPoints
 * (include/features/tracking/klt_patch_optical_flow.h:344-385) gets from basalt's detectKeypoints(level image, kd,
 * optical_flow_detection_grid_size, 1, current points), called for the first frame (:145) and after every tracking step
 * (:180) to refill the grid cells whose tracks were lost.  Keypoint ids and the bookkeeping of tracks across frames are
 * pnec_hip_tracks_retain / _append below; stereo filtering and the view graph are NOT here.  INTEGER ARITHMETIC ON 8-BIT PIXELS: every output is exact.
 * [EXT] basalt's keypoints.cpp and OpenCV's cv::FAST, which it calls, are not in the reference tree: they are restated
 * from the published code, and what follows is this library's own definition.
 *
 * Input.
 *   images      n_images images of height x width pixels in pnec_hip_patch_covariance's layout, `pitch` elements per row.
 *   pixel_type  PNEC_HIP_PIXEL_U8, or PNEC_HIP_PIXEL_U16 read as v >> 8 (the reference's quantisation of its 16-bit
 *               pyramid; the low byte does not matter).  PNEC_HIP_PIXEL_F32 is refused: a float image has no declared
 *               range to quantise.
 *   grid        the cell size G, 8 <= G <= 64 (the reference's configurations use 20, 30 and 50); width, height >= G.
 *   points_per_cell   K, 1 <= K <= 4 (the reference always passes 1).
 *   min_threshold     T, 0 <= T <= 254 (the reference's loop ends at 5).
 *   edge        E >= 0 (the reference's EDGE_THRESHOLD is 19).
 *   cur_offsets, n_cur, cur_pts   int64 [n_images + 1], double [n_cur, 2]: the points already tracked in each image,
 *               ragged, in the image's own pixel coordinates.  Either pointer may be NULL (with n_cur = 0): none.
 *
 * Cells.  x_start = (width % G) / 2, nx = width / G; cell column cx covers x_start + cx G .. x_start + cx G + G - 1; the
 * same in y.  n_cells = nx ny, cell index c = cx ny + cy (the reference's loop order, x outer).
 * Occupied cells.  A current point p with x_start <= p.x < x_start + nx G, and the same in y, marks cell
 * ((int)((p.x - x_start) / G), (int)((p.y - y_start) / G)) in double arithmetic; a NaN coordinate marks nothing.  An
 * occupied cell is not searched.
 * Corner measure.  The detector sees each cell as a G x G image of its own, as the reference does: pixels within 3 of a
 * cell's border are never corners and nothing outside the cell is read.  For an interior pixel p of value I and the 16
 * ring pixels I_k at (0,-3) (1,-3) (2,-2) (3,-1) (3,0) (3,1) (2,2) (1,3) (0,3) (-1,3) (-2,2) (-3,1) (-3,0) (-3,-1) (-2,-2)
 * (-1,-3):  m(p) = the largest value, over the 16 arcs of 9 contiguous ring pixels and both signs, of the minimum over
 * the arc of +-(I_k - I), floored at 0.  p is a FAST-9 corner at threshold t iff m > t; cv::FAST's score is m - 1.
 * Selection.  A candidate has m > T, m strictly greater than m at all 8 neighbours (a neighbour on the 3-pixel border has
 * m = 0), and an image position with E <= x < width - E - 1 and E <= y < height - E - 1 (basalt's InBounds).  The cell's
 * output is its up to K candidates by descending m, then ascending y, then ascending x.  For K = 1 this is what the
 * reference's loop returns (cv::FAST with non-maximum suppression at thresholds 40, 20, 10, 5; the best in-bounds point
 * of the first round that has one).  Two deviations: ties are broken by raster order (the reference's std::sort leaves
 * them open), and for K > 1 the points are distinct (the reference's loop would add the same point again in the next
 * round).
 *
 * Outputs, cap = n_images n_cells K entries provided by the caller.
 *   out_cell        int32 [n_images, n_cells]  the number of points the cell produced, 0 .. K; -1 for an occupied cell.
 *                   Required (it is the occupancy map while the call runs).
 *   out_offsets     int64 [n_images + 1]       points [out_offsets[f], out_offsets[f+1]) lie in image f.  Required.
 *   out_pts         double [cap, 2]            x, y: integers in doubles, what pnec_hip_patch_track / _patch_covariance
 *                   take as tmpl_pts / pts.  Required.
 *   out_score       int32 [cap]                m - 1.  May be NULL.
 *   out_cell_index  int32 [cap]                c.  May be NULL.
 * Points are compacted image by image, cell by cell in index order, rank by rank; entries at and beyond
 * out_offsets[n_images] are left untouched.  Order and content are a function of the inputs alone (no atomic decides a
 * position), and a cell's points depend on its own pixels and parameters only -- not on the call it sits in, nor on
 * `space`, nor on the pixel type the same values are stored in.
 * DEVICE space: every array is device memory of `device`, nothing is allocated, nothing waits, the call is asynchronous
 * on `stream`, and the image index of a current point is clamped as in pnec_hip_patch_covariance.  HOST space:
 * everything is staged, cur_offsets is checked, the call blocks.
 * PNEC_HIP_ERR_INVALID_ARGUMENT: NULL images / out_cell / out_offsets / out_pts, grid, points_per_cell or min_threshold
 * outside its range, edge < 0, width or height < grid, pitch < width, n_images < 1, n_cur < 0, F32 or an unknown
 * pixel_type, cur_pts without cur_offsets (or cur_offsets with n_cur > 0 without cur_pts), a bad `space`; in HOST space
 * also cur_offsets that do not run from 0 to n_cur without decreasing. */
int pnec_hip_detect_keypoints(const void *images, int pixel_type, int64_t n_images, int32_t height, int32_t width,
                              int64_t pitch, int32_t grid, int32_t points_per_cell, int32_t min_threshold, int32_t edge,
                              const int64_t *cur_offsets, int64_t n_cur, const double *cur_pts, int32_t *out_cell,
                              int64_t *out_offsets, double *out_pts, int32_t *out_score, int32_t *out_cell_index,
                              int space, int device, void *stream);

/* Tracks across frames: the bookkeeping of KLTPatchOpticalFlow::processFrame
 * (include/features/tracking/klt_patch_optical_flow.h:121-191) on the device, and the tracker with a template image per
 * track (added within ABI 8: pure additions, PNEC_HIP_ABI_VERSION is unchanged).  After trackPoints the reference keeps
 * the tracks that came back valid in id order (`observations` is a std::map, :198-212, :282-283), hands their positions
 * to addPoints as the occupied cells (:344-355) and gives every new corner the next id and an identity transform
 * (:359-385); a track's patches are built in the frame it was born in (:361-369) and tracked for its whole life (:228).
 * Stereo filtering and the view graph are NOT here.
 *
 * --- A track set.  Ragged over n_images images (sequences in lockstep): offsets int64 [n_images + 1] and arrays of
 * n_rows rows; rows [offsets[f], offsets[f+1]) belong to image f, rows at and beyond offsets[n_images] are padding.
 *   id          int64  [n_rows]     unique per image, >= 0                                     padding -1
 *   tmpl_image  int32  [n_rows]     index of the birth image in a stack of template images     padding 0
 *   tmpl_pts    double [n_rows, 2]  where the patch was built                                  padding NaN
 *   age         int32  [n_rows]     frames since birth                                         padding 0
 *   pts, angle  double [n_rows, 2], [n_rows]   the transform in the set's frame                padding NaN
 *   cov         double [n_rows, 3]  the 2x2 covariance there (xx, xy, yy)                      padding NaN
 * Both calls below write the padding themselves, to the end of the arrays, so the next pnec_hip_patch_track_indexed /
 * _detect_keypoints / _patch_covariance call can be given the full n_rows as its n_points without reading a size back:
 * a NaN template is BAD_TEMPLATE, a NaN current point marks no cell, a NaN point is an EMPTY patch.
 * Positions come from counts and prefix sums, never from an atomic: the outputs are a function of the inputs alone, and
 * an image's rows do not depend on the other images of the call, nor on `space`.
 * DEVICE space: every array is device memory of `device`, nothing is allocated, nothing waits, the calls are
 * asynchronous on `stream`; offsets are not checked (a row range is cut to the rows there are).  HOST space: everything
 * is staged, the offsets are checked (from 0, non-decreasing, at most n_rows / n_det), the call blocks.
 * Outputs are fresh arrays: none may be an input of the same call.
 *
 * --- pnec_hip_tracks_retain: the surviving tracks of one tracking step, compacted.
 * Input: a set (its `angle` is not needed) and pnec_hip_patch_track's outputs for its rows, trk_pts / trk_angle / trk_cov
 * / trk_status; max_age >= 0.  Row k is retained iff k < offsets[n_images], id[k] >= 0, trk_status[k] ==
 * PNEC_HIP_TRACK_OK, and max_age == 0 or age[k] + 1 <= max_age.
 * Output: a set of the same n_rows.  Per image the retained rows in their input order (stable: the reference's id order);
 * id, tmpl_image, tmpl_pts copied; age + 1, saturating; pts / angle / cov = the track's outputs; out_prev_pts /
 * out_prev_cov = the input set's pts / cov of the same track; out_src int64 = the input row (-1 in padding).  May be
 * NULL: cov, trk_cov, out_cov and out_prev_cov (together), out_prev_pts, out_src.  The retained set is the
 * correspondence list of the pair (previous frame, this frame): pnec_hip_problem_fill_keypoints takes out_prev_pts,
 * out_pts, out_cov with out_offsets as they stand.
 * PNEC_HIP_ERR_INVALID_ARGUMENT: n_images < 1, n_rows < 0, NULL offsets / out_offsets, with n_rows > 0 a NULL required
 * array, the four covariance arrays not given together, max_age < 0, an output that is an input, a bad `space`; in HOST
 * space also bad offsets.
 *
 * --- pnec_hip_tracks_append: addPoints' bookkeeping.
 * Input: a set (absent on the first frame: offsets and all its pointers NULL, n_rows = 0; `cov` may be NULL);
 * detections det_offsets [n_images + 1], det_pts [n_det, 2], det_cov [n_det, 3] or NULL (pnec_hip_detect_keypoints'
 * outputs as they stand, n_det its capacity, and pnec_hip_patch_covariance there); tmpl_image_base >= 0 with
 * tmpl_image_base + n_images - 1 fitting int32; per_image_capacity C >= 1; next_id int64 [n_images], read and written.
 * For image f with a = offsets[f+1] - offsets[f] and d = det_offsets[f+1] - det_offsets[f]: take_a = min(a, C), take_d =
 * min(d, C - take_a); its output rows are the first take_a set rows unchanged, then the first take_d detections, where
 * detection r gets id = next_id[f] + r, tmpl_image = tmpl_image_base + f, tmpl_pts = pts = det_pts, age = 0, angle = 0,
 * cov = det_cov or NaN; then next_id[f] += take_d, and out_dropped[f] = (a - take_a) + (d - take_d) (may be NULL).
 * n_out rows are provided by the caller: at least min(n_images C, n_rows + n_det) -- checked from the arguments alone;
 * HOST space also checks it against the rows the call produces.  Padding is written to n_out.  Ids are 64-bit throughout.
 * PNEC_HIP_ERR_INVALID_ARGUMENT: n_images < 1, a negative count, a set given in part, NULL det_offsets / det_pts /
 * next_id / out_offsets / (n_out > 0) a required output, C < 1, tmpl_image_base out of range, n_out too small, an output
 * that is an input, a bad `space`; in HOST space also bad offsets.
 *
 * --- pnec_hip_patch_track_indexed: pnec_hip_patch_track with a template image per keypoint.
 * pnec_hip_patch_track's arguments plus n_tmpl_images and tmpl_image int32 [n_points]: `tmpl` holds n_tmpl_images images
 * per level, and keypoint k builds its templates -- and its out_cov -- in image tmpl_image[k] of `tmpl`; prev and next
 * stay indexed by the keypoint's own image.  Everything else is pnec_hip_patch_track's definition, bit for bit: a call
 * whose tmpl_image names, for every keypoint, an image with the pixels of its own image in a plain call returns the plain
 * call's bits.  tmpl_image == NULL requires n_tmpl_images == n_images, means "the keypoint's own image" and runs
 * pnec_hip_patch_track's kernel.  With tmpl_image, prev must not be NULL.  DEVICE space: the index is clamped to
 * [0, n_tmpl_images - 1]; HOST space: an index outside that range is PNEC_HIP_ERR_INVALID_ARGUMENT.
 *
 * The frame loop (pnec_amd.Tracker): a ring of R >= 3 pyramids as one stack of R n_images images per level, frame n in
 * slot n % R; per frame pyramid -> patch_track_indexed (tmpl = the stack, prev / next = two slots, init = the set) ->
 * tracks_retain (max_age = R - 2) -> detect_keypoints (current = the retained set) -> patch_covariance ->
 * tracks_append (tmpl_image_base = slot * n_images), none of which reads anything back.  DEVIATION: the reference keeps a
 * track's patch for ever; here a track is retired when its age would reach R - 1, the step before its birth frame's slot
 * is overwritten, and the pair loses that track's correspondence on that step.  The stored form below
 * (pnec_hip_patch_store_add, pnec_hip_patch_track_stored; pnec_amd.Tracker(templates="patches")) lifts it. */
int pnec_hip_tracks_retain(int64_t n_images, const int64_t *offsets, int64_t n_rows, const int64_t *id,
                           const int32_t *tmpl_image, const double *tmpl_pts, const int32_t *age, const double *pts,
                           const double *cov, const double *trk_pts, const double *trk_angle, const double *trk_cov,
                           const int32_t *trk_status, int32_t max_age, int64_t *out_offsets, int64_t *out_id,
                           int32_t *out_tmpl_image, double *out_tmpl_pts, int32_t *out_age, double *out_pts,
                           double *out_angle, double *out_cov, double *out_prev_pts, double *out_prev_cov,
                           int64_t *out_src, int space, int device, void *stream);
int pnec_hip_tracks_append(int64_t n_images, const int64_t *offsets, int64_t n_rows, const int64_t *id,
                           const int32_t *tmpl_image, const double *tmpl_pts, const int32_t *age, const double *pts,
                           const double *angle, const double *cov, const int64_t *det_offsets, int64_t n_det,
                           const double *det_pts, const double *det_cov, int32_t tmpl_image_base,
                           int64_t per_image_capacity, int64_t *next_id, int64_t n_out, int64_t *out_offsets,
                           int64_t *out_id, int32_t *out_tmpl_image, double *out_tmpl_pts, int32_t *out_age,
                           double *out_pts, double *out_angle, double *out_cov, int64_t *out_dropped, int space,
                           int device, void *stream);
int pnec_hip_patch_track_indexed(const void *const *tmpl, const int64_t *tmpl_pitch, int64_t n_tmpl_images,
                                 const void *const *prev, const int64_t *prev_pitch, const void *const *next,
                                 const int64_t *next_pitch, int32_t n_levels, int pixel_type, int64_t n_images,
                                 int32_t height, int32_t width, const int64_t *offsets, int64_t n_points,
                                 const double *tmpl_pts, const int32_t *tmpl_image, const double *init_pts,
                                 const double *init_angle, double shift_x, double shift_y, const double *pattern,
                                 int32_t n_pattern, int32_t max_iterations, double max_recovered_dist2, uint32_t flags,
                                 double scaling, double *out_pts, double *out_angle, double *out_cov,
                                 double *out_dist2, int32_t *out_status, int32_t *out_lost_level, int space, int device,
                                 void *stream);

/* --- pnec_hip_tracks_keyframe: keyframe pairs -- skip frames that moved too little (added within ABI 8: a pure
 * addition, PNEC_HIP_ABI_VERSION is unchanged).  The reference does not turn every frame into a pose:
 * FrameProcessing::ProcessFrame (frame_processing.cc:87-93) asks TrackingMatcher::FindMatches (tracking_matcher.cc:68-85)
 * for the mean pixel distance between the host frame's and the new frame's matched keypoints and skips the frame when
 * that mean is below min_local_rad (5.0 at every caller); a skipped frame never enters the view graph, the next frame is
 * matched by track id against the same host frame.  This call is that rule for n_images sequences in lockstep, after one
 * step of the frame loop above, without a read-back.
 *
 * Per-track STATE, carried from call to call: key_pts double [n_key_rows, 2] and key_cov [n_key_rows, 3] hold where each
 * row of the current set (the set after the last refill) was seen in its sequence's KEY FRAME, the last accepted frame --
 * NaN for a track born after the key frame --, and span int32 [n_images] the number of frames between the key frame and
 * the previous frame (0: the previous frame is the key frame; a negative span counts as 0).
 * Inputs of one step:
 *   the retained set B   offsets [n_images + 1], n_rows, pts [n_rows, 2], cov [n_rows, 3], src int64 [n_rows]:
 *                        pnec_hip_tracks_retain's out_offsets, out_pts, out_cov, out_src -- src is the row of the set the
 *                        track was retained from, which is the row of the state
 *   the refilled set A'  new_offsets [n_images + 1], n_new, new_pts [n_new, 2], new_cov [n_new, 3]:
 *                        pnec_hip_tracks_append's out_offsets, out_pts, out_cov when given B
 *   the state, min_displacement >= 0 (finite), max_span >= 1.
 * Row ranges of both sets are cut as everywhere: lo = clamp(offsets[f], 0, rows), hi = clamp(offsets[f+1], lo, rows).
 * Per image f: a retained row k of its range is a MATCH iff 0 <= src[k] < n_key_rows, both words of key_pts[src[k]] are
 * finite and both words of pts[k] are finite.  n_matches[f] is the count of matches; mean[f] the sum over the matches of
 * sqrt(dx*dx + dy*dy), (dx, dy) = pts[k] - key_pts[src[k]], divided by n_matches -- NaN for n_matches == 0.
 * THE ORDER OF THE SUM is fixed: with lo the first row of the image, lane l of 64 adds the displacements of the matches
 * among rows lo + l, lo + l + 64, ... in that order, starting from +0.0; then six tree steps s = 32, 16, 8, 4, 2, 1, each
 * v[l] += v[l + s] for l < s; the sum is v[0].  It is a function of the image's rows alone: not of the batch, of `space`,
 * or of an atomic.
 *   accepted[f] = !(mean < min_displacement) || span[f] + 1 >= max_span
 * The first clause is the reference's comparison; a NaN mean (no match) is accepted, which moves the key frame on after
 * every track was lost.  The second clause forces acceptance (DEVIATION below).
 * PAIR outputs, arrays of n_rows rows: for an accepted image its matches in row order, compacted; for a skipped image
 * nothing.  out_offsets int64 [n_images + 1] = the exclusive scan of accepted ? n_matches : 0; out_key_pts = key_pts[src],
 * out_pts = pts, out_cov = cov, out_key_cov = key_cov[src] (for HOST / SYM batches), out_row int64 = the retained row k;
 * rows at and beyond out_offsets[n_images] are padding, written to n_rows: NaN (0x7ff8000000000000) and out_row -1.
 * pnec_hip_problem_fill_keypoints_ragged(offsets = out_offsets, pts1 = out_key_pts, pts2 = out_pts, cov2 = out_cov) takes
 * them as they stand.  Per image, each may be NULL: out_accepted uint8 [n_images], out_mean double [n_images],
 * out_n_matches int32 [n_images].
 * NEXT STATE, laid out by A' (n_new rows; distinct arrays: double-buffer the state as the sets are): for image f,
 * take = min(count_B[f], count_A'[f]) (pnec_hip_tracks_append's take_a, for every capacity).  Local row l < take of A' is
 * retained row B.offsets[f] + l: of an accepted image it gets new_pts / new_cov of its own row, else key_pts[src] /
 * key_cov[src] of that retained row, NaN for an src outside [0, n_key_rows).  Local row l >= take is a new detection: of
 * an accepted image its own new_pts / new_cov, else NaN.  Rows at and beyond new_offsets[n_images] get NaN.
 * next_span[f] = accepted ? 0 : span[f] + 1, saturating.
 * FIRST-FRAME FORM: the retained set is absent (offsets, pts, cov, src NULL, n_rows == 0; key_pts, key_cov, span may be
 * NULL and are not read).  Every image is accepted with n_matches 0 and mean NaN, all out_offsets are 0, the next state
 * is A''s own new_pts / new_cov, next_span is 0.
 * The covariance arrays cov, new_cov, key_cov, out_cov, out_key_cov, next_key_cov are given or NULL together (first-frame
 * form: new_cov and next_key_cov); an array of no rows counts for neither side.
 * DEVICE space: no allocation, no atomic, no wait; asynchronous on `stream`; offsets are not checked, only cut.  HOST
 * space: staged, both offsets arrays are checked (from 0, non-decreasing, within their rows), the call blocks.
 * PNEC_HIP_ERR_INVALID_ARGUMENT, before a device is touched: n_images < 1, a negative count, a retained set or a state
 * given in part, the covariance arrays not given together, NULL new_offsets / new_pts / out_offsets / (n_rows > 0) a pair
 * array, a NULL next-state array, min_displacement negative, NaN or infinite, max_span < 1, an output that is an input, a
 * bad `space`; in HOST space also bad offsets.
 * DEVIATION: pnec_amd.Tracker's ring retires a track at age R - 2, so a pair that spans more than R - 2 frames has no
 * match: the caller caps the span (pnec_amd.KeyframeTracker: max_span defaults to R - 2 and more is refused), and a pair
 * that spans s frames also lacks the tracks born before the key frame that aged out.  The reference keeps a track's
 * patches for ever and has no such cap.  The stored form below lifts it: with pnec_amd.KeyframeTracker(templates=
 * "patches") a track lives as long as it is tracked, any max_span >= 1 is taken and none forces no acceptance. */
int pnec_hip_tracks_keyframe(int64_t n_images, const int64_t *offsets, int64_t n_rows, const double *pts,
                             const double *cov, const int64_t *src, const int64_t *new_offsets, int64_t n_new,
                             const double *new_pts, const double *new_cov, int64_t n_key_rows, const double *key_pts,
                             const double *key_cov, const int32_t *span, double min_displacement, int32_t max_span,
                             int64_t *out_offsets, double *out_key_pts, double *out_pts, double *out_cov,
                             double *out_key_cov, int64_t *out_row, uint8_t *out_accepted, double *out_mean,
                             int32_t *out_n_matches, double *next_key_pts, double *next_key_cov, int32_t *next_span,
                             int space, int device, void *stream);

/* pnec_hip_tracks_link: the join of two track sets on their ids (added within ABI 8: a pure addition,
 * PNEC_HIP_ABI_VERSION is unchanged) -- for every row of the current set the row of the same track in the previous set,
 * WITHIN its image's range there: the `link` pnec_hip_relative_scale takes when both sets filled a batch each.
 *   cur_offsets int64 [n_images + 1], cur_id int64 [n_cur]      the current set's ranges and ids
 *   prev_offsets int64 [n_images + 1], prev_id int64 [n_prev]   the previous set's
 *   out_link int32 [n_cur]; out_n_linked int32 [n_images] | NULL
 * Both sets' ranges are cut as in every track call: lo = clamp(offsets[f], 0, rows), hi = clamp(offsets[f + 1], lo, rows);
 * Lp is the previous range's length, plo its first row.  For row k of image f with id = cur_id[k]: id < 0 gives -1;
 * otherwise the lower bound by the bisection a = 0, b = Lp; while a < b: m = a + (b - a) / 2, if prev_id[plo + m] < id then
 * a = m + 1 else b = m; and out_link[k] = a if a < Lp and prev_id[plo + a] == id, else -1.  For previous ids that ascend
 * strictly within an image -- what pnec_hip_tracks_retain and pnec_hip_tracks_append produce: they keep the order of ids
 * and new ids are larger -- that is the row holding the id, or -1 where there is none; for other input the result is
 * the bisection's, and every access stays inside the arrays.  All compares are 64-bit.  Rows at and beyond the cut
 * cur_offsets[n_images] (padding) get -1, up to n_cur.  out_n_linked[f] is the number of rows of image f with a link >= 0.
 * DEVICE space: asynchronous on `stream`, two launches sized by n_cur and n_images alone, nothing allocated, nothing
 * waited for, no atomic on global memory, the offsets are not read back (rows that unchecked offsets leave in no image
 * get -1); an image's outputs depend on its own rows and its previous range alone, not on its neighbours or on `space`.
 * HOST space: staged on `device`, both offset arrays are checked (from 0, non-decreasing, within their rows), the call
 * blocks.  n_cur == 0 writes zeros to out_n_linked and returns 0.
 * PNEC_HIP_ERR_INVALID_ARGUMENT, before a device is touched: n_images < 1 or > 2^31-1, n_cur or n_prev negative or
 * > 2^31-1, NULL cur_offsets, prev_offsets or out_link, cur_id NULL with n_cur > 0, prev_id NULL with n_prev > 0, an
 * output that is an input or the other output, a bad `space`. */
int pnec_hip_tracks_link(int64_t n_images, const int64_t *cur_offsets, int64_t n_cur, const int64_t *cur_id,
                         const int64_t *prev_offsets, int64_t n_prev, const int64_t *prev_id, int32_t *out_link,
                         int32_t *out_n_linked, int space, int device, void *stream);

/* Stored patches: a track keeps its templates for as long as it lives (added within ABI 8: pure additions,
 * PNEC_HIP_ABI_VERSION is unchanged).  The reference (klt_patch_optical_flow.h:344-385) builds an OpticalFlowPatch per
 * pyramid level when a point is added -- the mean-normalised intensities `data`, the gain H_se2_inv_J_se2_T, the level's
 * Hessian -- and keeps them until the track is lost (:228, :256-280).  A PATCH STORE is device (or, in HOST space, host)
 * memory of n_slots slots of pnec_hip_patch_store_slot_bytes(n_levels) bytes each, one slot per track, filled when the
 * track is born; the set's tmpl_image column then holds the track's slot instead of an image index, and
 * pnec_hip_tracks_retain / _append carry it along unchanged.
 *
 * --- pnec_hip_patch_store_slot_bytes: the size of one slot, 8 (32 + 256 n_levels); 0 for n_levels outside 1 .. 8.
 * Callers only allocate n_slots * slot_bytes (8-byte aligned; 256-byte aligned makes every plane start on a 128-byte line).
 * The layout is the library's own, in 64-bit words:
 *   word 0 int64 n, word 1 double S, words 2 .. 7 double H[6] (00 01 02 11 12 22): the level-0 template's sums, which the
 *   covariance epilogue needs; word 8 + l int64 level l's template status (pnec_hip_patch_status of the template's full
 *   inverse); word 16 + l uint64 level l's validity, bit i pattern point i's; words 24 .. 31 zero; then per level l, from
 *   word 32 + 256 l, four planes of 64 doubles: the normalised value (n v_i) / S of each pattern point and the three
 *   components of its gain K_i = H^-1 J_i'.  Storage is double: the tracker's bits are those of the rebuilt template.
 *
 * --- pnec_hip_patch_store_add: gives every new row of a refilled set a slot and fills it.
 * Input: the current frame's pyramid cur / cur_pitch (n_levels levels in pnec_hip_patch_track's layout, pixel_type,
 * n_images, height, width); carried_offsets int64 [n_images + 1], the offsets of the retained set the refill started from,
 * or NULL on the first frame; the refilled set's offsets int64 [n_images + 1], n_rows, tmpl_pts [n_rows, 2] and its
 * tmpl_image column `slot` int32 [n_rows], READ AND WRITTEN IN PLACE; per_image_capacity C; pattern / n_pattern; the
 * store and n_slots >= n_images C.
 * With a_f the count of image f in carried_offsets (0 when NULL; a negative one counts as 0) and c_f its count in offsets,
 * take_f = min(a_f, c_f) (pnec_hip_tracks_append's take_a).  Rows with local index < take_f are CARRIED: their slot is
 * read and left alone.  The others are NEW.  The occupied local slots of image f are slot[r] - f C over its carried rows;
 * a value outside [0, C) is ignored in DEVICE space and refused in HOST space.  The i-th new row, in row order, gets the
 * global slot f C + (the i-th smallest free local slot); a new row for which no slot is free (only when c_f > C) gets -1
 * and no patch; rows at and beyond offsets[n_images] (padding) get -1.  The assignment is a function of the image's rows
 * alone: no atomic on device memory decides a slot, nothing is allocated, nothing waits.
 * Then, for every new row that has a slot, the templates of all levels are built at tmpl_pts / 2^l in the row's own image
 * of `cur` and written into the slot: the terms pnec_hip_patch_track computes for a template, in its order of operations.
 * Other slots of the store are not touched.
 * DEVICE space: asynchronous on `stream`, offsets are not checked, only cut to the rows there are.  HOST space:
 * everything is staged (the whole store travels up and back), offsets and carried slots are checked, the call blocks.
 * n_rows = 0 returns at once.
 * PNEC_HIP_ERR_INVALID_ARGUMENT, before a device is touched: NULL cur / cur_pitch / a level pointer / offsets / pattern /
 * store / (n_rows > 0) tmpl_pts or slot, n_levels outside 1 .. 8, n_pattern outside 1 .. 64, an unknown pixel_type,
 * n_images < 1, n_rows < 0, a level smaller than 4 pixels, a pitch below its level's width, C < 1,
 * C > PNEC_HIP_PATCH_STORE_MAX_CAPACITY (65536: the assignment keeps an image's occupancy map in LDS), n_images C not
 * fitting int32, n_slots < n_images C or not fitting int32, an output (slot, store) that is an input, a bad `space`; in
 * HOST space also offsets or carried_offsets that do not run from 0 without decreasing (offsets: to at most n_rows) and
 * a carried row whose slot is not one of its image's.
 *
 * --- pnec_hip_patch_track_stored: pnec_hip_patch_track with the templates read from the store.
 * pnec_hip_patch_track_indexed's arguments with store, n_slots in place of tmpl, tmpl_pitch, n_tmpl_images, and slot int32
 * [n_points] in place of tmpl_image; prev is required.  Everything that is not the template is pnec_hip_patch_track's
 * definition, bit for bit, and a call whose slots were filled by pnec_hip_patch_store_add from the image, the point and
 * the pattern an indexed call would build its templates from returns the indexed call's bits in every output.  The
 * pattern must be the one the slots were built with (it still places the points in prev and next).  A row whose slot lies
 * outside [0, n_slots) comes back as a template that is bad at the top level: status PNEC_HIP_TRACK_BAD_TEMPLATE,
 * lost_level n_levels - 1, out_pts the start + shift, out_angle the start angle, out_cov and out_dist2 NaN -- what the
 * indexed call returns for a set's NaN padding rows.  The row-to-image map is that of a track set: rows at and beyond
 * offsets[n_images] are padding.  HOST space: offsets run from 0 to at most n_points without decreasing, and a slot
 * outside [0, n_slots) on a row below offsets[n_images] is PNEC_HIP_ERR_INVALID_ARGUMENT; the store is staged whole.
 * PNEC_HIP_ERR_INVALID_ARGUMENT: pnec_hip_patch_track's list, and NULL store / slot / prev, n_slots outside 1 .. 2^31 - 1,
 * an output that is the store or the slot column.
 *
 * The frame loop with stored patches (pnec_amd.Tracker(templates="patches")): two pyramids suffice; per frame pyramid ->
 * patch_track_stored (prev / next = the two pyramids, init = the set) -> tracks_retain (max_age = 0) -> detect_keypoints
 * -> patch_covariance -> tracks_append -> patch_store_add (cur = this frame, carried_offsets = the retained set's), seven
 * calls, none of which reads anything back.  A track keeps its slot until it is lost; the slot is free from the next
 * patch_store_add on. */
#define PNEC_HIP_PATCH_STORE_MAX_CAPACITY 65536
int64_t pnec_hip_patch_store_slot_bytes(int32_t n_levels);
int pnec_hip_patch_store_add(const void *const *cur, const int64_t *cur_pitch, int32_t n_levels, int pixel_type,
                             int64_t n_images, int32_t height, int32_t width, const int64_t *carried_offsets,
                             const int64_t *offsets, int64_t n_rows, const double *tmpl_pts, int32_t *slot,
                             int64_t per_image_capacity, const double *pattern, int32_t n_pattern, double *store,
                             int64_t n_slots, int space, int device, void *stream);
int pnec_hip_patch_track_stored(const double *store, int64_t n_slots, const void *const *prev, const int64_t *prev_pitch,
                                const void *const *next, const int64_t *next_pitch, int32_t n_levels, int pixel_type,
                                int64_t n_images, int32_t height, int32_t width, const int64_t *offsets, int64_t n_points,
                                const double *tmpl_pts, const int32_t *slot, const double *init_pts,
                                const double *init_angle, double shift_x, double shift_y, const double *pattern,
                                int32_t n_pattern, int32_t max_iterations, double max_recovered_dist2, uint32_t flags,
                                double scaling, double *out_pts, double *out_angle, double *out_cov, double *out_dist2,
                                int32_t *out_status, int32_t *out_lost_level, int space, int device, void *stream);

/* Name and launch geometry the auto-tuner would pick for this problem (for logs / profiles). */
int pnec_hip_describe_launch(const pnec_hip_problem *p, const pnec_hip_options *opt,
                             int32_t *corr_per_lane, int32_t *waves_per_pair,
                             int32_t *lds_corr_per_lane, int32_t *threads_per_block,
                             int32_t *resident);

/* Device-side unit checks of the cross-lane reduction (DPP + v_permlane*_swap), the 5x5 Cholesky,
 * the reciprocal / reciprocal-square-root refinements, the lean trigonometry and the front stages'
 * smallest-eigenpair route (characteristic-polynomial start + Rayleigh-quotient iteration against the
 * Jacobi sweeps, on generic, nearly degenerate, rank-deficient and badly scaled matrices).  0 = all good. */
int pnec_hip_selftest(int device);

/* Work counters of the front stages, for roofline accounting: how many evaluations of the eigenvalue function, scored
 * tiles, table builds, ... the launches since the last reset held (the indices: enum kWk* in pnec_frontend.hip; the
 * numbers depend on the data, not on the timing).  Only a library built with -DPNEC_WORK_COUNT counts
 * (tools/count_chain_work.py builds and runs one); the production build compiles the counting out and reports
 * *compiled_in = 0 and zeros.  Entries [13] and [14] work in every build: the correspondence-passes the refinement
 * executed in full (residual, weight, Jacobian, normal equations) and cost-only (after a rejected step and at the iteration
 * cap) in the pnec_hip_solve calls made with PNEC_HIP_OPT_COUNT_PASSES in pnec_hip_options.flags.  Waits for the device. */
int pnec_hip_work_counters(int device, int reset, uint64_t *out16, int32_t *compiled_in);

/* The library keeps freed device buffers for reuse (batches are created and destroyed per frame or per
 * frame set in a pipeline; hipMalloc/hipFree cost tens of microseconds for small buffers and far more for
 * GB-sized ones).  Cap: environment
 * variable PNEC_HIP_CACHE_MB (default 16384, 0 disables).  This call returns the cached buffers
 * of `device` (-1: all devices) to the driver; returns the number of bytes released. */
int64_t pnec_hip_release_cache(int device);
/* out4: hipMalloc calls made by the library's allocator so far | requests served from its cache | blocks handed out and
 * not yet freed | bytes sitting in the cache (all devices; for "nothing is allocated after warm-up" tests) */
int pnec_hip_alloc_counters(uint64_t *out4);

#ifdef __cplusplus
}
#endif
#endif /* PNEC_HIP_H_ */
