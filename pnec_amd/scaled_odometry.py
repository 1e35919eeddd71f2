"""Scaled odometry: images in, a trajectory out, and still nothing read back.

``Odometry.process`` returns a relative rotation and a translation DIRECTION per frame.  ``ScaledOdometry`` adds what is
left between that and a trajectory, on the device: the pair's tracks are joined with the previous pair's on their ids
(``link_tracks``, ``pnec_hip_tracks_link``), the linked tracks give the ratio of the two baselines
(``pnec_hip_relative_scale``), and a running scale and pose per sequence take one step (``advance_trajectory``,
``pnec_hip_trajectory_advance``).  include/pnec_hip.h has the definitions.

The scale is relative to each sequence's FIRST solved pair (its baseline is the unit); the pose is that of the current
frame in the frame of the sequence's first, with the conventions of ``compose_trajectory``.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import capi
from .batch import Batch
from .odometry import Odometry, OdometryResult
from .patches import _is_torch
from .tracker import _where
from .trajectory import _fits, _shape

STATUS_NAMES = capi.TRAJ_NAMES


@dataclass
class TrajectoryState:
    """The running state of pnec_hip_trajectory_advance, one row per sequence; numpy or torch.cuda."""
    s: object   # [n] the last pair's baseline in units of the first pair's; NaN before the first pair
    q: object   # [n,4] xyzw, the pose of the last frame: rotation, unit
    p: object   # [n,3] and position


@dataclass
class ScaledOdometryResult:
    """One step of ScaledOdometry.process, everything torch.cuda.  `step` is Odometry's result (its `pairs` is the
    tracker's buffer); every other field is a fresh tensor the caller may keep."""
    step: OdometryResult
    t_oriented: object   # [F,3] step.t with the sign that puts the structure in front (pnec_hip_triangulate)
    scale: object        # [F] the running scale s after this step
    ratio3: object       # [F,3] lower quartile, lower median, upper quartile of the baseline ratios against the previous pair
    n_linked: object     # int32 [F] tracks this pair shares with the previous one
    n_used: object       # int32 [F] of which gave a ratio
    abs_q: object        # [F,4] the frame's rotation in its sequence's first frame
    abs_p: object        # [F,3] and position, in units of the sequence's first baseline
    status: object       # int32 [F] capi.TRAJ_MEASURED / TRAJ_HELD / TRAJ_STARTED / TRAJ_ABSENT


def _kit(on, ref):
    space, device, stream, dev = _where(ref, on)
    if on:
        import torch
        kinds = {"f64": torch.float64, "i64": torch.int64, "i32": torch.int32}
        as_in = lambda a, k="f64": None if a is None else (
            a.to(device=dev, dtype=kinds[k]).contiguous() if _is_torch(a) else torch.as_tensor(np.array(a), dtype=kinds[k], device=dev))
        new = lambda shape, k="f64": torch.empty(shape, dtype=kinds[k], device=dev)
        ptr = lambda a: None if a is None else a.data_ptr()
    else:
        kinds = {"f64": np.float64, "i64": np.int64, "i32": np.int32}
        as_in = lambda a, k="f64": None if a is None else np.ascontiguousarray(a.cpu().numpy() if _is_torch(a) else a, dtype=kinds[k])
        new = lambda shape, k="f64": np.empty(shape, dtype=kinds[k])
        ptr = lambda a: None if a is None else a.ctypes.data
    return space, device, stream, as_in, new, ptr


def _is_i32(a):
    return str(a.dtype).replace("torch.", "") == "int32"


def link_tracks(cur_offsets, cur_id, prev_offsets, prev_id, out=None, n_linked=None):
    """For every row of the current set (cur_offsets int64 [F+1], cur_id int64 [n]) the row, within the same image's
    range of the previous set (prev_offsets, prev_id), that holds the same track id; -1 where there is none, for a
    negative id and in padding: the `link` of Batch.relative_scale.  The previous ids must ascend within an image, as
    a tracker's do.  Returns (link int32 [n], n_linked int32 [F]).  torch.cuda in -> torch.cuda out, asynchronous on
    torch's current stream, nothing read back, and with `out` / `n_linked` nothing allocated; numpy in -> staged,
    numpy out."""
    on = _is_torch(cur_id) and cur_id.is_cuda
    space, device, stream, as_in, new, ptr = _kit(on, cur_id)
    co, ci, po, pi = as_in(cur_offsets, "i64"), as_in(cur_id, "i64"), as_in(prev_offsets, "i64"), as_in(prev_id, "i64")
    if co.ndim != 1 or co.shape[0] < 2 or tuple(po.shape) != tuple(co.shape):
        raise ValueError("cur_offsets and prev_offsets must both be [F + 1] with F >= 1")
    if ci.ndim != 1 or pi.ndim != 1:
        raise ValueError("cur_id and prev_id must be one-dimensional")
    F, n, m = int(co.shape[0]) - 1, int(ci.shape[0]), int(pi.shape[0])
    if out is None:
        out = new((n,), "i32")
    else:
        _fits(out, (n,), on, "link")
    if n_linked is None:
        n_linked = new((F,), "i32")
    else:
        _fits(n_linked, (F,), on, "n_linked")
    if not (_is_i32(out) and _is_i32(n_linked)):
        raise ValueError("`out` and `n_linked` must be int32")
    if n == 0:     # (an array without rows has no address to pass: what the call writes for n_cur == 0)
        n_linked[...] = 0
        return out, n_linked
    capi.check(capi.lib().pnec_hip_tracks_link(F, ptr(co), n, ptr(ci) if n else None, ptr(po), m, ptr(pi) if m else None,
                                               ptr(out), ptr(n_linked), space, device, stream))
    return out, n_linked


def new_trajectory_state(n: int, on_device: bool, device=None) -> TrajectoryState:
    """A fresh state of n sequences: s = NaN (no pair yet), q = (0, 0, 0, 1), p = 0."""
    n = int(n)
    if on_device:
        import torch
        f64 = dict(dtype=torch.float64, device=device)
        s, q, p = torch.full((n,), float("nan"), **f64), torch.zeros((n, 4), **f64), torch.zeros((n, 3), **f64)
    else:
        s, q, p = np.full(n, np.nan), np.zeros((n, 4)), np.zeros((n, 3))
    q[:, 3] = 1.0
    return TrajectoryState(s, q, p)


def advance_trajectory(state: TrajectoryState, rel_q, rel_t, count=None, min_count: int = 0, scale3=None, n_used=None,
                       min_used: int = 1, out=None):
    """One frame's step of the running scale and pose (pnec_hip_trajectory_advance): a pair that is present -- rel_q
    [n,4] and rel_t [n,3] finite, a quaternion that is not zero, `count` [n] (if given) at least min_count -- multiplies
    the scale by the lower median scale3[:, 1] of RelativeScale's three quantiles where that is measured (finite, > 0,
    `n_used` at least min_used), keeps the scale where it is not, starts it at 1 on a fresh state, and moves the pose
    by (rel_q, scale * rel_t); a pair that is not present leaves the state as it is.  Returns (the next state,
    status int32 [n]): capi.TRAJ_MEASURED, TRAJ_HELD, TRAJ_STARTED, TRAJ_ABSENT.  `out`: (a TrajectoryState, a status
    array) to write, other arrays than `state`.  Memory spaces as in link_tracks."""
    on = _is_torch(rel_q) and rel_q.is_cuda
    space, device, stream, as_in, new, ptr = _kit(on, rel_q)
    rq, rt = as_in(rel_q), as_in(rel_t)
    n = int(rq.shape[0])
    cnt, sc, nu = as_in(count, "i32"), as_in(scale3), as_in(n_used, "i32")
    s, q, p = as_in(state.s), as_in(state.q), as_in(state.p)
    _shape(rq, (n, 4), "rel_q"), _shape(rt, (n, 3), "rel_t"), _shape(cnt, (n,), "count"), _shape(sc, (n, 3), "scale3")
    _shape(nu, (n,), "n_used"), _shape(s, (n,), "state.s"), _shape(q, (n, 4), "state.q"), _shape(p, (n, 3), "state.p")
    if nu is not None and sc is None:
        raise ValueError("n_used needs scale3")
    if out is None:
        nxt, status = TrajectoryState(new((n,)), new((n, 4)), new((n, 3))), new((n,), "i32")
    else:
        nxt, status = out
        _fits(nxt.s, (n,), on, "s"), _fits(nxt.q, (n, 4), on, "q"), _fits(nxt.p, (n, 3), on, "p"), _fits(status, (n,), on, "status")
        if not _is_i32(status):
            raise ValueError("the status array must be int32")
    capi.check(capi.lib().pnec_hip_trajectory_advance(device, n, ptr(rq), ptr(rt), ptr(cnt), int(min_count), ptr(sc), ptr(nu),
                                                      int(min_used), ptr(s), ptr(q), ptr(p), ptr(nxt.s), ptr(nxt.q),
                                                      ptr(nxt.p), ptr(status), space, stream))
    return nxt, status


class ScaledOdometry(Odometry):
    """Odometry with a running scale and pose per sequence; Odometry's arguments, and keyword-only:

    min_parallax  radians, pnec_hip_relative_scale's gate (0: off)
    min_links     the used links a ratio needs to count as measured (advance's min_used)
    min_corr      the correspondences a pair needs for its pose to count (advance's min_count; 0: any finite pose)

    ``process(images)`` returns None for the first frame, then a ScaledOdometryResult.  A step is Odometry.process,
    pnec_hip_triangulate (for the translation's sign), pnec_hip_tracks_link, pnec_hip_relative_scale against the previous
    pair's batch, pnec_hip_trajectory_advance, and two copies that keep the pair's ids for the next step.  Everything is
    allocated here: two capacity batches used in turn (``batch`` names the current one), the link, ratio and kept-id
    buffers of F * capacity rows, both pairs' oriented translations, two states.  No call of process reads anything back
    or waits, and the library allocates nothing after the second pair.

    Keyframe pairs (min_displacement > 0) are refused: a sequence that skips a frame needs the last ACCEPTED pair's
    batch and ids kept per sequence, which two batches used in lockstep cannot hold."""

    def __init__(self, n_sequences: int, height: int, width: int, K_inv, mode: int = capi.MODE_TARGET,
                 pipeline_options: capi.PipelineOptions | None = None, min_displacement: float = 0.0, max_span: int = None,
                 *, min_parallax: float = 0.0, min_links: int = 1, min_corr: int = 0, **kwargs):
        if float(min_displacement) > 0.0:
            raise ValueError("ScaledOdometry does not take keyframe pairs (min_displacement > 0): the previous pair must "
                             "be the previous frame's")
        if not (float(min_parallax) >= 0.0) or not np.isfinite(float(min_parallax)):
            raise ValueError("min_parallax must be >= 0 and finite (radians)")
        if int(min_links) < 1 or int(min_corr) < 0:
            raise ValueError("min_links must be >= 1 and min_corr >= 0")
        import torch
        super().__init__(n_sequences, height, width, K_inv, mode, pipeline_options, 0.0, max_span, **kwargs)
        self.min_parallax, self.min_links, self.min_corr = float(min_parallax), int(min_links), int(min_corr)
        F, cap, dev = self.n_sequences, self.capacity, self.device
        with torch.cuda.device(dev):
            other = Batch.with_capacity(self.mode, F, F * cap, device=dev.index)
            other.reshape(np.arange(F + 1, dtype=np.int64) * cap)
        self._batches = [self.batch, other]
        self._turn = 0
        N = F * cap
        f64, i32, i64 = (dict(dtype=d, device=dev) for d in (torch.float64, torch.int32, torch.int64))
        self._link = torch.full((N,), -1, **i32)
        self._ratio = torch.empty((N,), **f64)
        self._prev_id = torch.full((N,), -1, **i64)           # the previous pair's ids and ranges: none yet
        self._prev_offsets = torch.zeros((F + 1,), **i64)
        self._t_oriented = [torch.zeros((F, 3), **f64), torch.zeros((F, 3), **f64)]
        self._scale3 = torch.empty((F, 3), **f64)
        self._n_linked, self._n_used, self._status = (torch.zeros((F,), **i32) for _ in range(3))
        self._states = [new_trajectory_state(F, True, dev), new_trajectory_state(F, True, dev)]
        self._state = 0                                        # which of _states is current
        self.prev_pair = torch.arange(F, **i64)
        self._no_prev_pair = torch.full((F,), -1, **i64)
        self._pairs_done = 0

    @property
    def state(self) -> TrajectoryState:
        """the current running state (the library's own buffers: the step after next overwrites them)"""
        return self._states[self._state]

    def process(self, images):
        import torch
        turn = self._turn
        self.batch = cur = self._batches[turn]
        q_prev = self._prev_q            # the previous pair's rotation (None before the first pair)
        step = super().process(images)
        if step is None:
            return None
        first = self._pairs_done == 0
        prev = cur if first else self._batches[1 - turn]
        t_cur, t_prev = self._t_oriented[turn], self._t_oriented[1 - turn]
        F, N = self.n_sequences, self.n_sequences * self.capacity
        lib, p = capi.lib(), (lambda a: None if a is None else a.data_ptr())
        device = self.device.index
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(device).cuda_stream
            capi.check(lib.pnec_hip_triangulate(cur._h, p(step.q), p(step.t), 1, capi.TRI_ORIENT, None, None, None, None, None,
                                                None, None, None, None, p(t_cur), None, capi.MEM_DEVICE, stream))
            pairs = step.pairs
            capi.check(lib.pnec_hip_tracks_link(F, p(pairs.offsets), N, p(pairs.id), p(self._prev_offsets), N, p(self._prev_id),
                                                p(self._link), None, capi.MEM_DEVICE, device, stream))
            capi.check(lib.pnec_hip_relative_scale(
                cur._h, prev._h, p(self._no_prev_pair if first else self.prev_pair), p(self._link), p(step.q), p(t_cur),
                p(self._identity if q_prev is None else q_prev), p(t_prev), self.min_parallax, p(self._ratio), None,
                p(self._scale3), p(self._n_linked), p(self._n_used), capi.MEM_DEVICE, stream))
            old, new = self._states[self._state], self._states[1 - self._state]
            capi.check(lib.pnec_hip_trajectory_advance(
                device, F, p(step.q), p(t_cur), p(step.n_corr), self.min_corr, p(self._scale3), p(self._n_used),
                self.min_links, p(old.s), p(old.q), p(old.p), p(new.s), p(new.q), p(new.p), p(self._status),
                capi.MEM_DEVICE, stream))
            self._prev_id.copy_(pairs.id, non_blocking=True)
            self._prev_offsets.copy_(pairs.offsets, non_blocking=True)
        self._state = 1 - self._state
        self._turn = 1 - turn
        self._pairs_done += 1
        return ScaledOdometryResult(step, t_cur.clone(), new.s.clone(), self._scale3.clone(), self._n_linked.clone(),
                                    self._n_used.clone(), new.q.clone(), new.p.clone(), self._status.clone())

    def close(self):
        for b in self._batches:
            b.close()
