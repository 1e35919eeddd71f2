#!/usr/bin/env python3
"""Generate tests/golden/trajectory_metrics_golden.npz by IMPORTING the reference's metric functions.

Run from the repo root:   python tests/golden/make_trajectory_golden.py
Needs the reference tree (make_golden.REF; the script does nothing without it -> the .npz is committed, this script is
only its provenance).  Nothing of the reference's text is stored: the fixture holds seeded trajectories made here
(tests/trajectory_cases.traj) and the numbers the reference's functions return for them.

Reference functions exercised (scripts/pnec/metrics): rpe_1.rpe_1 (rmse at distance 1), rpe_n.rpe_n, l1_rpe_1.rpe_1,
l1_rpe_n.rpe_n and r_t.r_t.  They take a pandas frame with the columns poses_gt / poses_est holding sophus SE3 objects;
sophus is not needed for that: the small Pose class below has the four methods they call.

Per trajectory of trajectory_cases.GOLDEN_CASES the file holds the inputs (est_q, est_p, gt_q, gt_p, and the estimate's
relative steps rel_q, rel_t), `ref` [5] (RPE_1, RPE_n, L1RPE_1, L1RPE_n, r_t in radians) and `ref_err` [5]:
|reference - long-double checker|, the reference's own distance from the truth, which the tests add to their bound.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import trajectory_cases as tc  # noqa: E402
from make_golden import REF  # noqa: E402


class Pose:
    """what the reference's metric functions ask of an SE3: rotationMatrix(), translation(), inverse(), *"""

    def __init__(self, R, t):
        self.R, self.t = np.asarray(R, dtype=np.float64), np.asarray(t, dtype=np.float64)

    def rotationMatrix(self):
        return self.R

    def translation(self):
        return self.t

    def inverse(self):
        return Pose(self.R.T, -self.R.T @ self.t)

    def __mul__(self, other):
        return Pose(self.R @ other.R, self.t + self.R @ other.t)


def main():
    if not os.path.isdir(REF):
        print("reference tree not found: nothing generated")
        return
    sys.path.insert(0, REF)
    import pandas as pd
    from pnec.metrics import l1_rpe_1, l1_rpe_n, r_t, rpe_1, rpe_n

    out = {"cases": np.array(tc.GOLDEN_CASES, dtype=np.float64)}
    for i, (L, noise, step, seed) in enumerate(tc.GOLDEN_CASES):
        t = tc.traj(L, noise, seed, step)
        frame = pd.DataFrame({"poses_gt": [Pose(R, p) for R, p in zip(tc.qmat(t.gt_q), t.gt_p)],
                              "poses_est": [Pose(R, p) for R, p in zip(tc.qmat(t.est_q), t.est_p)]})
        stdout = sys.stdout
        sys.stdout = open(os.devnull, "w")   # (rpe_n draws a progress bar)
        try:
            ref = np.array([rpe_1.rpe_1(frame), rpe_n.rpe_n(frame), l1_rpe_1.rpe_1(frame), l1_rpe_n.rpe_n(frame),
                            r_t.r_t(frame)], dtype=np.float64)
        finally:
            sys.stdout.close()
            sys.stdout = stdout
        assert np.isfinite(ref).all(), (L, ref)
        exact = tc.metrics_np([0, L], t.est_q, t.gt_q, t.est_p, t.gt_p, dtype=np.longdouble).metrics[0]
        err = np.abs(ref.astype(np.longdouble) - exact).astype(np.float64)
        print(f"L={L}: ref {ref}  |ref - longdouble| relative {err / np.abs(ref)}")
        for name in tc.Traj._fields[1:]:
            out[f"{name}_{i}"] = getattr(t, name)
        out[f"ref_{i}"] = ref
        out[f"ref_err_{i}"] = err
    path = os.path.join(HERE, "trajectory_metrics_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
