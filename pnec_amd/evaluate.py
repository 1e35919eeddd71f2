"""``python -m pnec_amd.evaluate EST GT TIMES [--name NAME]``: the reference's run evaluation
(scripts/pnec/visual_odometry/io/evaluate_run.py:85-132) on the device.

EST is a relative-pose file as the odometry writes it (timestamp tx ty tz qx qy qz qw per line, io_formats.read_pose_file),
GT a KITTI ground-truth file (a 3x4 matrix per line) and TIMES its times.txt.  The relative poses are composed into a
trajectory (pnec_hip_trajectory_compose) whose left factor is the reference's pose correction -- the ground truth's first
pose times the inverse of the estimate's first -- the frames are joined on timestamps truncated to milliseconds, and the
matched frames are scored (pnec_hip_trajectory_metrics).  Prints the header and the row of the reference's metrics.yaml.
"""
from __future__ import annotations

import argparse

import numpy as np

from . import io_formats
from .trajectory import compose_trajectory, trajectory_metrics


def millisecond_keys(timestamps):
    """The join key of evaluate_run.py:45-46: datetime.fromtimestamp(t) printed with microseconds, the last three digits
    cut -- the timestamp rounded to whole microseconds, then truncated to whole milliseconds.  int64."""
    us = np.rint(np.asarray(timestamps, dtype=np.float64) * 1e6).astype(np.int64)
    return us // 1000


def join_timestamps(est_times, gt_times):
    """(est_index, gt_index): for every ground-truth frame, in order, whose millisecond key some estimated frame has, the
    two row numbers -- pandas' ground_truth.join(estimated.set_index('timestamp'), on='timestamp').dropna().  Two
    estimated frames with one key are refused: the reference would score the frame twice."""
    ek, gk = millisecond_keys(est_times), millisecond_keys(gt_times)
    where = {}
    for i, k in enumerate(ek.tolist()):
        if k in where:
            raise ValueError(f"estimated frames {where[k]} and {i} share the millisecond {k}")
        where[k] = i
    pairs = [(where[k], j) for j, k in enumerate(gk.tolist()) if k in where]
    idx = np.array(pairs, dtype=np.int64).reshape(-1, 2)
    return idx[:, 0], idx[:, 1]


def read_kitti_poses(path):
    """-> (R [M,3,3], p [M,3]) of a KITTI ground-truth file: 12 numbers a line, a 3x4 matrix row by row"""
    a = np.loadtxt(path, ndmin=2).reshape(-1, 3, 4)
    return a[:, :, :3].copy(), a[:, :, 3].copy()


def rotations_to_quaternions(R):
    """xyzw of rotation matrices [M,3,3] (Shepperd), unit"""
    import torch

    from .simulation import matrix_to_quaternion_xyzw
    q = matrix_to_quaternion_xyzw(torch.as_tensor(np.asarray(R, dtype=np.float64))).numpy()
    return q / np.linalg.norm(q, axis=-1, keepdims=True)


def _rotate(q, v):
    u = q[:3]
    t = 2.0 * np.cross(u, v)
    return v + q[3] * t + np.cross(u, t)


def pose_correction(gt_q0, gt_p0, est_q0, est_p0):
    """gt_0 * est_0^-1 (evaluate_run.py:125-126) as (q [4], p [3])"""
    x, y, z, w = est_q0 / np.linalg.norm(est_q0)
    inv = np.array([-x, -y, -z, w])
    a = gt_q0
    q = np.array([a[3] * inv[0] + a[0] * inv[3] + a[1] * inv[2] - a[2] * inv[1],
                  a[3] * inv[1] - a[0] * inv[2] + a[1] * inv[3] + a[2] * inv[0],
                  a[3] * inv[2] + a[0] * inv[1] - a[1] * inv[0] + a[2] * inv[3],
                  a[3] * inv[3] - a[0] * inv[0] - a[1] * inv[1] - a[2] * inv[2]])
    return q, gt_p0 - _rotate(q, est_p0)


def evaluate(est_path, gt_path, times_path, name="run"):
    """The metrics of one run: a TrajectoryMetrics of one sequence (numpy; the arrays are staged on device 0)."""
    times, rel_t, rel_q = io_formats.read_pose_file(est_path)
    keep = ~np.isnan(np.column_stack([times, rel_t, rel_q])).any(axis=1)   # (read_poses drops such rows, :58)
    times, rel_t, rel_q = times[keep], rel_t[keep], rel_q[keep]
    gt_R, gt_p = read_kitti_poses(gt_path)
    gt_times = np.loadtxt(times_path, ndmin=1)
    if gt_times.shape[0] != gt_R.shape[0]:
        raise ValueError(f"{gt_R.shape[0]} ground-truth poses but {gt_times.shape[0]} times")
    if times.shape[0] == 0 or gt_R.shape[0] == 0:
        raise ValueError("no estimated or no ground-truth poses")
    gt_q = rotations_to_quaternions(gt_R)
    q0, p0 = pose_correction(gt_q[0], gt_p[0], rel_q[0], rel_t[0])
    n = times.shape[0]
    traj = compose_trajectory(np.array([0, n], dtype=np.int64), rel_q, rel_t, q0=q0[None], p0=p0[None])
    ei, gi = join_timestamps(times, gt_times)
    m = len(ei)
    return trajectory_metrics(np.array([0, m], dtype=np.int64), traj.q[ei], gt_q[gi], traj.p[ei], gt_p[gi])


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m pnec_amd.evaluate", description=__doc__.split("\n\n")[0])
    ap.add_argument("est", help="relative poses: timestamp tx ty tz qx qy qz qw per line")
    ap.add_argument("gt", help="KITTI ground truth: a 3x4 matrix per line")
    ap.add_argument("times", help="the ground truth's times.txt")
    ap.add_argument("--name", default="run", help="the row's name (the reference: the method)")
    args = ap.parse_args(argv)
    for line in evaluate(args.est, args.gt, args.times).rows([args.name]):
        print(line)


if __name__ == "__main__":
    main()
