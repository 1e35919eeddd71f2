"""Images in, poses out: ``Odometry`` runs ``Tracker`` -> ``Batch.fill_keypoints_ragged`` -> ``Batch.solve_pipeline`` for F
image sequences in lockstep, and no call of ``process`` reads anything back or waits.

The tracker's correspondences are ragged by an offsets array only the device knows.  The batch is a capacity batch
shaped ONCE, to the uniform bounds ``arange(F + 1) * capacity`` (a track set holds at most `capacity` rows per image);
every frame the device-side offsets shape it inside those bounds (pnec_hip_problem_fill_keypoints_ragged), and the
chain's launch geometries follow the bounds.

The start pose of a pair is the reference's (frame_processing.cc:97-102): the previous pair's rotation with zero
translation, the identity for the first pair -- and the identity wherever the previous result is not finite (an empty
pair has no pose).

With ``min_displacement > 0`` the pairs are keyframe pairs (keyframes.py): a sequence whose frame moved too little
against its key frame is skipped -- its pose is NaN, its n_corr 0 -- and the chain of a later pair starts from the last
ACCEPTED pair's rotation (the reference's PrevRelRotation).

With ``distortion`` the pair's rows go through ``undistort_keypoints`` (undistort.py) on their way from the tracker to
the ingest; the tracker itself goes on from its raw positions.  DEVIATION from the reference, which measures the
keyframe displacement after undistortion (its keypoints are undistorted when they are made): here it is measured in raw
pixels, before this step.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import capi
from .batch import Batch
from .keyframes import KeyframeTracker
from .tracker import Tracker, TrackSet
from .undistort import camera_array, new_undistorted, undistort_keypoints


@dataclass
class OdometryResult:
    """One step of Odometry.process, everything torch.cuda on the tracker's device.  q, t, n_corr and init_q are fresh
    tensors (the caller may keep them); `pairs` is the tracker's own buffer, overwritten by the next step."""
    q: object        # [F,4] xyzw, the relative rotation of the pair (previous frame, this frame)
    t: object        # [F,3] unit translation direction
    n_corr: object   # int32 [F] correspondences per pair as the batch holds them: gate poses of empty or tiny pairs on it
    pairs: TrackSet  # the correspondences (prev_pts, pts, cov, ragged by offsets): Tracker.process's result
    init_q: object   # [F,4] the start rotation the chain was given
    # keyframes on (min_displacement > 0) only; `pairs` is then the KeyframePairs, and q / t of a skipped sequence are NaN
    accepted: object = None           # uint8 [F]
    mean_displacement: object = None  # [F] mean pixel distance of the matches against the key frame, NaN without a match
    span: object = None               # int32 [F] frames between the key frame and this frame after the step (0: accepted)


def start_rotation(prev_q, identity):
    """The rotation a pair's chain starts from: the previous pair's where every component is finite, else the identity.
    prev_q [F,4] or None (the first pair), identity [F,4]; torch."""
    import torch
    if prev_q is None:
        return identity.clone()
    return torch.where(torch.isfinite(prev_q).all(dim=-1, keepdim=True), prev_q, identity)


def _camera_from(K_inv, distortion):
    """camera_array from K_inv [3,3] (host) and 4 or 5 distortion coefficients; ValueError unless K_inv is upper
    triangular with zero skew and last row (0, 0, 1)."""
    d = [float(x) for x in distortion]
    if len(d) not in (4, 5):
        raise ValueError("distortion takes 4 or 5 coefficients: k1 k2 p1 p2 [k3]")
    a, b = K_inv[0, 0], K_inv[1, 1]
    if K_inv[0, 1] != 0.0 or K_inv[1, 0] != 0.0 or K_inv[2, 0] != 0.0 or K_inv[2, 1] != 0.0 or K_inv[2, 2] != 1.0 or \
            not (np.isfinite(K_inv).all() and a != 0.0 and b != 0.0):
        raise ValueError("with a distortion K_inv must be upper triangular with zero skew and last row (0, 0, 1)")
    return camera_array(1.0 / a, 1.0 / b, -K_inv[0, 2] / a, -K_inv[1, 2] / b, *d)


class Odometry:
    """Tracker + one capacity Batch, all allocated in the constructor.

    ``process(images)`` takes the next frame of every sequence ([F,h,w] torch.cuda) and returns None for the first frame,
    then an OdometryResult per frame.  mode: capi.MODE_TARGET (the PNEC chain, covariances from the tracker) or
    capi.MODE_NEC (bearings only; needs pipeline_options with use_nec).  K_inv [3,3]: host array or CUDA tensor.
    tracker_kwargs go to Tracker (levels, ring, grid, capacity, ...).  Asynchronous on torch's current stream.

    min_displacement > 0 turns keyframes on (KeyframeTracker: ring >= 4, max_span in 1 .. ring - 2, default ring - 2); with
    the default 0 every consecutive pair is solved, as before, and nothing of the keyframe machinery is created.
    templates="patches" among the tracker_kwargs runs both on stored patches (no age limit, ring >= 2, any max_span).

    distortion: None (an ideal pinhole camera: nothing is created and process makes the calls it always made) or the 4 or
    5 coefficients k1 k2 p1 p2 [k3] of the radial-tangential model.  K is then recovered from K_inv, which must be upper
    triangular with zero skew and last row (0, 0, 1).  Each pair's rows are undistorted (the reference's five fixed-point
    steps; undistort_newton polishes them, undistort_propagate_cov carries the covariances through the map) into buffers
    made here, never in place; `undistorted` holds the rows and statuses of the last step, `OdometryResult.pairs` stays the
    raw tracker result.  The keyframe displacement is measured in raw pixels (the reference: after undistortion)."""

    def __init__(self, n_sequences: int, height: int, width: int, K_inv, mode: int = capi.MODE_TARGET,
                 pipeline_options: capi.PipelineOptions | None = None, min_displacement: float = 0.0, max_span: int = None,
                 *, distortion=None, undistort_newton: bool = False, undistort_propagate_cov: bool = False,
                 **tracker_kwargs):
        import torch
        if mode not in (capi.MODE_TARGET, capi.MODE_NEC):
            raise ValueError("Odometry takes MODE_TARGET or MODE_NEC (what a tracker's covariances can fill)")
        if mode == capi.MODE_NEC and (pipeline_options is None or not pipeline_options.use_nec):
            raise ValueError("a MODE_NEC batch needs pipeline_options with use_nec")
        if not float(min_displacement) >= 0.0:
            raise ValueError("min_displacement must be >= 0")
        K_inv_host = np.asarray(K_inv.cpu() if hasattr(K_inv, "cpu") else K_inv, dtype=np.float64)
        if tuple(K_inv_host.shape) != (3, 3):
            raise ValueError("K_inv must be [3,3]")
        camera = None
        if distortion is not None:
            camera = _camera_from(K_inv_host, distortion)
        self.keyframes = None
        if float(min_displacement) > 0.0:
            self.keyframes = KeyframeTracker(n_sequences, height, width, min_displacement, max_span, **tracker_kwargs)
            self.tracker = self.keyframes.tracker
        else:
            self.tracker = Tracker(n_sequences, height, width, **tracker_kwargs)
        F, cap, dev = self.tracker.n_sequences, self.tracker.capacity, self.tracker.device
        self.n_sequences, self.capacity, self.mode, self.device = F, cap, int(mode), dev
        self.pipeline_options = pipeline_options
        with torch.cuda.device(dev):
            self.batch = Batch.with_capacity(mode, F, F * cap, device=dev.index)
            self.batch.reshape(np.arange(F + 1, dtype=np.int64) * cap)
        f64 = dict(dtype=torch.float64, device=dev)
        self._K_inv = torch.as_tensor(K_inv_host, **f64)
        self.undistorted = None   # the undistorted rows and statuses of the last step (distortion given)
        self._camera = None
        if camera is not None:
            self._camera = torch.as_tensor(camera, **f64)
            self._newton, self._propagate = bool(undistort_newton), bool(undistort_propagate_cov)
            self._und = new_undistorted(F * cap, True, dev, cov2=mode == capi.MODE_TARGET)
        self._identity = torch.zeros((F, 4), **f64)
        self._identity[:, 3] = 1.0
        self._zero_t = torch.zeros((F, 3), **f64)
        self._prev_q = None

    def _fill(self, offsets, pts1, pts2, cov):
        """The pair's rows into the batch, through undistort_keypoints where a distortion was given."""
        cov = cov if self.mode == capi.MODE_TARGET else None
        if self._camera is not None:
            u = self.undistorted = undistort_keypoints(self._camera, pts1, pts2, cov, newton=self._newton,
                                                       propagate_cov=self._propagate, out=self._und)
            pts1, pts2, cov = u.pts1, u.pts2, u.cov2
        self.batch.fill_keypoints_ragged(offsets, pts1, pts2, cov, K_inv=self._K_inv)

    def _process_keyframes(self, images):
        import torch
        pairs = self.keyframes.process(images)
        if pairs is None:
            return None
        with torch.cuda.device(self.device):
            self._fill(pairs.offsets, pairs.key_pts, pairs.pts, pairs.cov)
            init_q = start_rotation(self._prev_q, self._identity)
            q, t = self.batch.solve_pipeline(init_q, self._zero_t, self.pipeline_options)
        accepted = pairs.accepted.to(torch.bool)[:, None]
        nan = torch.full_like(q[:, :1], float("nan"))
        # the next chain starts from the last accepted pair's rotation (NaN before any: start_rotation's identity)
        self._prev_q = torch.where(accepted, q, nan if self._prev_q is None else self._prev_q)
        n_corr = torch.diff(pairs.offsets).clamp(0, self.capacity).to(torch.int32)
        return OdometryResult(torch.where(accepted, q, nan), torch.where(accepted, t, nan), n_corr, pairs, init_q,
                              pairs.accepted.clone(), pairs.mean_displacement.clone(), self.keyframes.state.span.clone())

    def process(self, images):
        import torch
        if self.keyframes is not None:
            return self._process_keyframes(images)
        pairs = self.tracker.process(images)
        if pairs is None:
            return None
        with torch.cuda.device(self.device):
            self._fill(pairs.offsets, pairs.prev_pts, pairs.pts, pairs.cov)
            init_q = start_rotation(self._prev_q, self._identity)
            q, t = self.batch.solve_pipeline(init_q, self._zero_t, self.pipeline_options)
        n_corr = torch.diff(pairs.offsets).clamp(0, self.capacity).to(torch.int32)
        self._prev_q = q
        return OdometryResult(q, t, n_corr, pairs, init_q)

    def close(self):
        self.batch.close()
