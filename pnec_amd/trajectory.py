"""Trajectory evaluation: ``compose_trajectory`` (``pnec_hip_trajectory_compose``) chains the relative poses of a run into
a trajectory per sequence, and ``trajectory_metrics`` (``pnec_hip_trajectory_metrics``) scores a trajectory against ground
truth with the five numbers the reference reports for every run: RPE_1, RPE_n, L1RPE_1, L1RPE_n and r_t
(scripts/pnec/visual_odometry/io/evaluate_run.py:85-129 and scripts/pnec/metrics).  include/pnec_hip.h has both
definitions.  Rows are sequence-major and ragged by ``offsets`` [n_seq + 1]; quaternions are x, y, z, w.

``stack_steps`` turns the steps of ``Odometry.process`` into those rows, ``matched`` drops the frames without a pose from
both sides before they are scored, so that images -> poses -> the paper's table stays on the device.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from . import capi
from .patches import _is_torch
from .tracker import _where

METRIC_NAMES = ("RPE_1", "RPE_n", "L1RPE_1", "L1RPE_n", "r_t")


@dataclass
class Trajectory:
    """pnec_hip_trajectory_compose's outputs; numpy or torch.cuda, matching the input."""
    q: object       # [n,4] xyzw absolute rotations, unit; the sign is the product's
    p: object       # [n,3] absolute positions, or None (no rel_t)
    valid: object   # uint8 [n]: 1 where the row was present, 0 where it carried the pose before it


@dataclass
class TrajectoryMetrics:
    """pnec_hip_trajectory_metrics' outputs, in radians; numpy or torch.cuda, matching the input."""
    RPE_1: object     # [n_seq]
    RPE_n: object     # [n_seq]
    L1RPE_1: object   # [n_seq]
    L1RPE_n: object   # [n_seq]
    r_t: object       # [n_seq], NaN without positions
    rmse_d: object    # [n]: row lo + d of a sequence holds the RMSE over all pairs at distance d, row lo holds 0
    l1_d: object      # [n]: the mean angle at distance d likewise
    err_q: object     # [n,4]: est * conj(gt) per row
    angle1: object    # [n]: the angle between consecutive rows, 0 at a sequence's first row
    rt1: object       # [n]: the translation error of consecutive rows, or None (no positions)
    metrics: object = None   # [n_seq,5]: the array the five views above are columns of

    def degrees(self):
        """The five metrics in degrees: float64 numpy [n_seq,5] (waits for the device)."""
        m = self.metrics
        m = m.detach().cpu().numpy() if _is_torch(m) else np.asarray(m)
        return m * (180.0 / math.pi)

    def rows(self, names):
        """The reference's metrics.yaml: the header line, then one line `name, RPE_1, RPE_n, L1RPE_1, L1RPE_n, r_t` per
        sequence, in degrees, '%.3f' (evaluate_run.py:99-100: to_csv(sep=',', float_format='%.3f'))."""
        deg = self.degrees()
        names = [names] if isinstance(names, str) else list(names)
        if len(names) != deg.shape[0]:
            raise ValueError(f"{deg.shape[0]} sequences need {deg.shape[0]} names")
        cell = lambda v: "" if math.isnan(v) else "%.3f" % v
        return [",".join(("name",) + METRIC_NAMES)] + [",".join([str(n)] + [cell(float(v)) for v in row])
                                                       for n, row in zip(names, deg)]


def _kit(ref, on):
    """(as_input(array, dtype name), new(shape, dtype name), pointer) in ref's memory space"""
    space, device, stream, dev = _where(ref, on)
    if on:
        import torch
        kinds = {"f64": torch.float64, "i64": torch.int64, "u8": torch.uint8}
        as_in = lambda a, k="f64": None if a is None else (
            a.to(device=dev, dtype=kinds[k]).contiguous() if _is_torch(a) else torch.as_tensor(np.array(a), dtype=kinds[k], device=dev))
        new = lambda shape, k="f64": torch.empty(shape, dtype=kinds[k], device=dev)
        ptr = lambda a: None if a is None else a.data_ptr()
    else:
        kinds = {"f64": np.float64, "i64": np.int64, "u8": np.uint8}
        as_in = lambda a, k="f64": None if a is None else np.ascontiguousarray(a.cpu().numpy() if _is_torch(a) else a, dtype=kinds[k])
        new = lambda shape, k="f64": np.empty(shape, dtype=kinds[k])
        ptr = lambda a: None if a is None else a.ctypes.data
    return space, device, stream, as_in, new, ptr


def _shape(a, want, name):
    if a is not None and tuple(a.shape) != tuple(want):
        raise ValueError(f"{name} must be {list(want)}, not {list(a.shape)}")


def _fits(o, want, on, name):
    if o is None or tuple(o.shape) != tuple(want) or (_is_torch(o) and o.is_cuda) != on or \
            not (o.is_contiguous() if _is_torch(o) else o.flags["C_CONTIGUOUS"]):
        raise ValueError(f"`out` must hold the call's shapes in its memory space ({name})")


def compose_trajectory(offsets, rel_q, rel_t=None, scale=None, q0=None, p0=None, out: Trajectory = None) -> Trajectory:
    """Compose the relative poses rel_q [n,4] (rel_t [n,3], times scale [n]) of every sequence -- rows
    offsets[f] .. offsets[f+1] -- into absolute poses: P_first = (q0, p0)[f] * step_first, P_k = P_{k-1} * step_k.  A row
    with a value that is not finite, or a zero quaternion, is an identity step and gets valid 0.  q0 [n_seq,4] and
    p0 [n_seq,3] default to the identity and zero.  torch.cuda in -> torch.cuda out, asynchronous on torch's current
    stream, nothing read back, and with `out` (a previous result) nothing allocated; numpy in -> staged, numpy out."""
    on = _is_torch(rel_q) and rel_q.is_cuda
    space, device, stream, as_in, new, ptr = _kit(rel_q, on)
    off, q, t, s, a0, b0 = as_in(offsets, "i64"), as_in(rel_q), as_in(rel_t), as_in(scale), as_in(q0), as_in(p0)
    if off.ndim != 1 or off.shape[0] < 2:
        raise ValueError("offsets must be [n_seq + 1] with n_seq >= 1")
    n_seq, n = int(off.shape[0]) - 1, int(q.shape[0])
    _shape(q, (n, 4), "rel_q"), _shape(t, (n, 3), "rel_t"), _shape(s, (n,), "scale")
    _shape(a0, (n_seq, 4), "q0"), _shape(b0, (n_seq, 3), "p0")
    if out is None:
        out = Trajectory(new((n, 4)), new((n, 3)) if t is not None else None, new((n,), "u8"))
    else:
        _fits(out.q, (n, 4), on, "q"), _fits(out.valid, (n,), on, "valid")
        if t is not None:
            _fits(out.p, (n, 3), on, "p")
    out_p = out.p if t is not None else None
    capi.check(capi.lib().pnec_hip_trajectory_compose(device, n_seq, ptr(off), n, ptr(q), ptr(t), ptr(s), ptr(a0), ptr(b0),
                                                      ptr(out.q), ptr(out_p), ptr(out.valid), space, stream))
    return Trajectory(out.q, out_p, out.valid)


def new_trajectory_metrics(n_seq: int, rows: int, on_device: bool, device=None, positions: bool = True) -> TrajectoryMetrics:
    """Uninitialised outputs for `rows` rows in `n_seq` sequences: what `out=` of trajectory_metrics takes."""
    if on_device:
        import torch
        new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=device)
    else:
        new = lambda *shape: np.empty(shape, dtype=np.float64)
    m = new(int(n_seq), 5)
    n = int(rows)
    return TrajectoryMetrics(m[:, 0], m[:, 1], m[:, 2], m[:, 3], m[:, 4], new(n), new(n), new(n, 4), new(n),
                             new(n) if positions else None, m)


def trajectory_metrics(offsets, est_q, gt_q, est_p=None, gt_p=None, out: TrajectoryMetrics = None) -> TrajectoryMetrics:
    """RPE_1, RPE_n, L1RPE_1, L1RPE_n and r_t (radians) of the absolute rotations est_q against gt_q [n,4] (and positions
    est_p, gt_p [n,3], for r_t) per sequence of `offsets`, with the per-distance errors they are made of.  Rows are
    matched frames: drop the frames without a pose from both sides first (`matched`).  An exact estimate scores 0 (the
    reference: NaN).  Memory spaces and `out` as in compose_trajectory."""
    on = _is_torch(est_q) and est_q.is_cuda
    space, device, stream, as_in, new, ptr = _kit(est_q, on)
    off, eq, gq, ep, gp = as_in(offsets, "i64"), as_in(est_q), as_in(gt_q), as_in(est_p), as_in(gt_p)
    if off.ndim != 1 or off.shape[0] < 2:
        raise ValueError("offsets must be [n_seq + 1] with n_seq >= 1")
    if (ep is None) != (gp is None):
        raise ValueError("est_p and gt_p go together")
    n_seq, n = int(off.shape[0]) - 1, int(eq.shape[0])
    _shape(eq, (n, 4), "est_q"), _shape(gq, (n, 4), "gt_q"), _shape(ep, (n, 3), "est_p"), _shape(gp, (n, 3), "gt_p")
    if out is None:
        out = new_trajectory_metrics(n_seq, n, on, eq.device if on else None, ep is not None)
    else:
        _fits(out.metrics, (n_seq, 5), on, "metrics"), _fits(out.err_q, (n, 4), on, "err_q")
        for name in ("rmse_d", "l1_d", "angle1") + (("rt1",) if ep is not None else ()):
            _fits(getattr(out, name), (n,), on, name)
    rt1 = out.rt1 if ep is not None else None
    capi.check(capi.lib().pnec_hip_trajectory_metrics(device, n_seq, ptr(off), n, ptr(eq), ptr(gq), ptr(ep), ptr(gp),
                                                      ptr(out.metrics), ptr(out.err_q), ptr(out.rmse_d), ptr(out.l1_d),
                                                      ptr(out.angle1), ptr(rt1), space, stream))
    m = out.metrics
    return TrajectoryMetrics(m[:, 0], m[:, 1], m[:, 2], m[:, 3], m[:, 4], out.rmse_d, out.l1_d, out.err_q, out.angle1, rt1, m)


def stack_steps(results):
    """The steps of one run -- a list of OdometryResult, each q [F,4] and t [F,3] for F sequences in lockstep -- as
    sequence-major rows: (offsets int64 [F+1], rel_q [F * (S+1), 4], rel_t [F * (S+1), 3]) with S = len(results).  Every
    sequence starts with an identity row, the pose of its first frame (the reference writes SE3() first,
    frame2frame.cc:134-137); a step without a pose stays NaN and compose_trajectory carries the pose over it.  Pure
    torch on the steps' device: no wait."""
    import torch
    if not results:
        raise ValueError("stack_steps needs at least one step")
    q = torch.stack([r.q for r in results], dim=1).to(torch.float64)   # [F,S,4]
    t = torch.stack([r.t for r in results], dim=1).to(torch.float64)
    F, S = int(q.shape[0]), int(q.shape[1])
    first_q = torch.zeros((F, 1, 4), dtype=torch.float64, device=q.device)
    first_q[:, :, 3] = 1.0
    first_t = torch.zeros((F, 1, 3), dtype=torch.float64, device=q.device)
    rel_q = torch.cat([first_q, q], dim=1).reshape(F * (S + 1), 4).contiguous()
    rel_t = torch.cat([first_t, t], dim=1).reshape(F * (S + 1), 3).contiguous()
    offsets = torch.arange(F + 1, dtype=torch.int64, device=q.device) * (S + 1)
    return offsets, rel_q, rel_t


def matched(offsets, traj: Trajectory, gt_q, gt_p=None):
    """Drop the rows with valid == 0 from the trajectory and from the ground truth, as the reference's join on
    timestamps with dropna() does: -> (offsets', est_q, est_p, gt_q', gt_p'), the inputs of trajectory_metrics.  torch
    (any device) or numpy.  Boolean indexing sizes its result from the data, so on a device this WAITS for the stream:
    it is meant for the end of a run, not for the frame loop."""
    if _is_torch(traj.q):
        import torch
        keep = traj.valid != 0
        off = torch.as_tensor(offsets, dtype=torch.int64, device=keep.device) if not _is_torch(offsets) else \
            offsets.to(device=keep.device, dtype=torch.int64)
        cum = torch.cat([torch.zeros(1, dtype=torch.int64, device=keep.device), torch.cumsum(keep.to(torch.int64), 0)])
        gq = gt_q if _is_torch(gt_q) else torch.as_tensor(np.asarray(gt_q), dtype=torch.float64, device=keep.device)
        gp = None if gt_p is None else (gt_p if _is_torch(gt_p) else
                                        torch.as_tensor(np.asarray(gt_p), dtype=torch.float64, device=keep.device))
        new_off = cum[off.clamp(0, keep.shape[0])]
    else:
        keep = np.asarray(traj.valid) != 0
        cum = np.concatenate([[0], np.cumsum(keep, dtype=np.int64)])
        gq, gp = np.asarray(gt_q), None if gt_p is None else np.asarray(gt_p)
        new_off = cum[np.clip(np.asarray(offsets, dtype=np.int64), 0, keep.shape[0])]
    pick = lambda a: None if a is None else a[keep]
    return new_off, pick(traj.q), pick(traj.p), pick(gq), pick(gp)
