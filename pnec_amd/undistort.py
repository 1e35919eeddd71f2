"""Keypoint undistortion: ``undistort_keypoints`` (``pnec_hip_undistort_keypoints``) takes tracked points and their 2x2
covariances from raw, distorted pixels to the pixels of the ideal pinhole camera with the same K -- the step the reference
runs per observation before a keypoint becomes a bearing (pnec::common::Undistort, common.cc:67-93: cv::undistortPoints
with k1, k2, p1, p2).  The rows are those of ``Batch.fill_keypoints_ragged``, so the outputs go straight into it.
include/pnec_hip.h has the definition in six steps.

Two things the reference's step does not do are offered and off by default: ``newton=True`` polishes the five fixed-point
steps of OpenCV (which leave tenths of a pixel at the corners of a wide-angle image) down to rounding, and
``propagate_cov=True`` carries the covariance through the map, S' = A S A', where the reference hands it on unchanged.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import capi
from .patches import _is_torch
from .tracker import _where


@dataclass
class Undistorted:
    """pnec_hip_undistort_keypoints' outputs; numpy or torch.cuda, matching the input.  A side that was not given is
    None.  status: uint8 per row, capi.UNDISTORT_OK / _OUTSIDE / _NOT_CONVERGED / _NOT_FINITE (capi.UNDISTORT_NAMES)."""
    pts1: object      # [n,2]
    pts2: object      # [n,2] or None
    cov2: object      # [n,3] (xx, xy, yy) of pts2, or None
    cov1: object      # [n,3] of pts1, or None
    status1: object   # uint8 [n]
    status2: object   # uint8 [n] or None


def camera_array(fx, fy, cx, cy, k1=0.0, k2=0.0, p1=0.0, p2=0.0, k3=0.0):
    """The nine doubles pnec_hip_undistort_keypoints reads: fx fy cx cy k1 k2 p1 p2 k3 (numpy, float64)."""
    return np.array([fx, fy, cx, cy, k1, k2, p1, p2, k3], dtype=np.float64)


def _new(shape, u8, on, dev):
    if on:
        import torch
        return torch.empty(shape, dtype=torch.uint8 if u8 else torch.float64, device=dev)
    return np.empty(shape, dtype=np.uint8 if u8 else np.float64)


def new_undistorted(rows: int, on_device: bool, device=None, pts2: bool = True, cov2: bool = True,
                    cov1: bool = False) -> Undistorted:
    """Uninitialised outputs for `rows` rows: what `out=` of undistort_keypoints takes."""
    n = lambda cols, want=True: (_new((int(rows), cols) if cols else (int(rows),), not cols, on_device, device)
                                 if want else None)
    return Undistorted(n(2), n(2, pts2), n(3, cov2), n(3, cov1), n(0), n(0, pts2))


def undistort_keypoints(camera, pts1, pts2=None, cov2=None, cov1=None, *, fixed_iterations: int = 5, newton: bool = False,
                        newton_iterations: int = 20, propagate_cov: bool = False, out: Undistorted = None) -> Undistorted:
    """Undistort the rows pts1 [n,2] (and pts2 [n,2], cov2 [n,3] of pts2, cov1 [n,3] of pts1) with `camera`
    (camera_array's nine doubles; array or CUDA tensor).  fixed_iterations=5 and no flag is the reference's
    cv::undistortPoints; `newton` polishes that result by up to newton_iterations Newton steps on the forward model;
    `propagate_cov` writes A S A' in place of a copy of S.  torch.cuda in -> torch.cuda out, asynchronous on torch's
    current stream, nothing read back, and with `out` nothing allocated; numpy in -> staged, numpy out.
    `out`: an Undistorted of the call's shapes (a previous result, new_undistorted) to write in place of new arrays.  An
    output may be its own input (in place); any other overlap is undefined."""
    on = _is_torch(pts1) and pts1.is_cuda
    space, device, stream, dev = _where(pts1, on)
    if on:
        import torch
        as_in = lambda a: None if a is None else (a.to(device=dev, dtype=torch.float64).contiguous() if _is_torch(a) else
                                                  torch.as_tensor(np.array(a), dtype=torch.float64, device=dev))
        ptr = lambda a: None if a is None else a.data_ptr()
    else:
        as_in = lambda a: None if a is None else np.ascontiguousarray(a.cpu().numpy() if _is_torch(a) else a,
                                                                      dtype=np.float64)
        ptr = lambda a: None if a is None else a.ctypes.data
    cam, p1, p2, c2, c1 = as_in(camera), as_in(pts1), as_in(pts2), as_in(cov2), as_in(cov1)
    if tuple(cam.shape) != (9,):
        raise ValueError("camera must hold 9 values: fx fy cx cy k1 k2 p1 p2 k3 (camera_array)")
    n = int(p1.shape[0])
    for a, cols, name in ((p1, 2, "pts1"), (p2, 2, "pts2"), (c2, 3, "cov2"), (c1, 3, "cov1")):
        if a is not None and tuple(a.shape) != (n, cols):
            raise ValueError(f"{name} must be [{n},{cols}]")
    if c2 is not None and p2 is None:
        raise ValueError("cov2 is the covariance of pts2: it needs pts2")
    if out is None:
        out = new_undistorted(n, on, dev, p2 is not None, c2 is not None, c1 is not None)
    else:
        for a, o, u8, name in ((p1, out.pts1, False, "pts1"), (p2, out.pts2, False, "pts2"), (c2, out.cov2, False, "cov2"),
                               (c1, out.cov1, False, "cov1"), (p1, out.status1, True, "status1"),
                               (p2, out.status2, True, "status2")):
            want = None if a is None else ((n,) if u8 else tuple(a.shape))
            if a is not None and (o is None or tuple(o.shape) != want or (_is_torch(o) and o.is_cuda) != on or
                                  not (o.is_contiguous() if _is_torch(o) else o.flags["C_CONTIGUOUS"])):
                raise ValueError(f"`out` must be an Undistorted of the call's shapes and memory space ({name})")
    g = lambda a, o: None if a is None else o
    flags = (capi.UNDISTORT_NEWTON if newton else 0) | (capi.UNDISTORT_PROPAGATE_COV if propagate_cov else 0)
    capi.check(capi.lib().pnec_hip_undistort_keypoints(
        device, n, ptr(p1), ptr(p2), ptr(c2), ptr(c1), ptr(cam), int(fixed_iterations), int(newton_iterations), flags,
        ptr(g(p1, out.pts1)), ptr(g(p2, out.pts2)), ptr(g(c2, out.cov2)), ptr(g(c1, out.cov1)), ptr(g(p1, out.status1)),
        ptr(g(p2, out.status2)), space, stream))
    return Undistorted(out.pts1, g(p2, out.pts2), g(c2, out.cov2), g(c1, out.cov1), out.status1, g(p2, out.status2))
