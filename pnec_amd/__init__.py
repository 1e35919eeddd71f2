"""pnec_amd -- MI355X-native PNEC relative-pose solver (hot path of tum-vision/pnec).

Layout:
  csrc/            HIP kernels + the C ABI (include/pnec_hip.h) + host C++ facade + pybind module
  capi.py          ctypes binding of libpnec_hip.so (no fallback: raises if the library is missing)
  batch.py         batches of frame pairs in HBM; numpy (host space) or torch.cuda (device space)
  autograd.py      differentiable_solve: the refinement as a torch.autograd.Function (gradients by pose_sensitivity)
  patches.py       2x2 keypoint covariances from image patches (the cov input of Batch.fill_keypoints)
  tracker.py       tracks across frames: retain, refill, and the frame loop over F sequences in lockstep
  patch_store.py   stored patches: a slot per track that keeps its templates for as long as it lives
  keyframes.py     keyframe pairs: skip frames that moved too little against the last accepted frame
  undistort.py     keypoint undistortion: the radial-tangential lens model inverted per tracked point
  trajectory.py    trajectory evaluation: relative poses composed per sequence, RPE_1 / RPE_n / L1RPE_1 / L1RPE_n / r_t
  evaluate.py      python -m pnec_amd.evaluate: a pose file against KITTI ground truth, the reference's metrics row
  odometry.py      images in, poses out: the tracker, a batch shaped from its device offsets, and the chain
  scaled_odometry.py  images in, a trajectory out: tracks linked on their ids, a running scale and pose per sequence
  simulation.py    synthetic inputs following the reference simulator's distributions (harness)
  distributed.py   one-process-per-GPU sharding of independent pair batches + one RCCL gather
"""
from . import capi  # noqa: F401
from .batch import (Batch, EightPoint, EssentialRansac, MinimalPose, PoseCovariance, PoseSensitivity, RelativeScale, ResidualReport, SolveResult, Triangulation, gate_sigma,  # noqa: F401
                    select_best)
from .keyframes import KeyframePairs, KeyframeState, KeyframeTracker, keyframe_pairs  # noqa: F401
from .odometry import Odometry, OdometryResult  # noqa: F401
from .patches import (PATTERN52, Keypoints, PatchCovariance, PatchTrack, detect_keypoints, image_pyramid,  # noqa: F401
                      patch_covariance, patch_track)
from .scaled_odometry import (ScaledOdometry, ScaledOdometryResult, TrajectoryState, advance_trajectory, link_tracks,  # noqa: F401
                              new_trajectory_state)
from .tracker import Tracker, TrackSet, append_tracks, retain_tracks  # noqa: F401
from .patch_store import PatchStore, add_patches, new_patch_store, patch_track_stored  # noqa: F401
from .tracks import chain_scales  # noqa: F401
from .undistort import Undistorted, camera_array, undistort_keypoints  # noqa: F401
from .trajectory import (Trajectory, TrajectoryMetrics, compose_trajectory, matched, stack_steps,  # noqa: F401
                         trajectory_metrics)


def differentiable_solve(*args, **kwargs):
    """pnec_amd.autograd.differentiable_solve (imported on first use: the package itself does not need torch)."""
    from .autograd import differentiable_solve as f
    return f(*args, **kwargs)


__all__ = ["capi", "Batch", "EightPoint", "EssentialRansac", "KeyframePairs", "KeyframeState", "KeyframeTracker", "Keypoints", "MinimalPose", "Odometry", "OdometryResult", "PATTERN52", "PatchCovariance", "PatchStore", "PatchTrack", "PoseCovariance", "PoseSensitivity", "RelativeScale", "ResidualReport", "ScaledOdometry", "ScaledOdometryResult", "SolveResult",
           "TrackSet", "Tracker", "Trajectory", "TrajectoryMetrics", "TrajectoryState", "Triangulation", "Undistorted", "add_patches", "advance_trajectory", "append_tracks", "camera_array", "chain_scales", "compose_trajectory", "detect_keypoints", "differentiable_solve", "gate_sigma", "image_pyramid", "keyframe_pairs", "link_tracks", "matched", "new_patch_store", "new_trajectory_state", "patch_covariance", "patch_track", "patch_track_stored", "retain_tracks", "select_best", "stack_steps", "trajectory_metrics", "undistort_keypoints"]
