"""Patch covariances: the 2x2 image covariance of keypoints from the image patches around them
(``pnec_hip_patch_covariance``; include/pnec_hip.h has the definition) -- the ``cov2`` / ``cov1`` input of
``Batch.fill_keypoints``, computed on the device from images and keypoint positions.

This is the covariance POpticalFlowPatch::setFromImage keeps (include/features/tracking/pnec_patch.h:78-137) after
KLTPatchOpticalFlow's scaling and rotation.  It is not tracking (positions come from the caller's tracker) and it is
double arithmetic, not the reference's float: no float parity is claimed.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import capi

PATCH_OK, PATCH_EMPTY, PATCH_SINGULAR = 0, 1, 2      # pnec_hip_patch_status
PATCH_NAMES = {PATCH_OK: "ok", PATCH_EMPTY: "empty_patch", PATCH_SINGULAR: "singular_hessian"}
PIXEL_U8, PIXEL_U16, PIXEL_F32 = 0, 1, 2             # pnec_hip_pixel_type
PATCH_MAX_POINTS = 64


def _pattern52() -> np.ndarray:
    """basalt's Pattern52 [EXT] (patterns.h is not in the reference tree; restated): 0.5 * raw, raw rows from y = 7 down
    to -7 in steps of 2, x ascending in steps of 2 over +-3, +-5, +-7, +-7, +-7, +-7, +-5, +-3."""
    raw = [(x, y) for y, r in zip(range(7, -9, -2), (3, 5, 7, 7, 7, 7, 5, 3)) for x in range(-r, r + 1, 2)]
    p = 0.5 * np.asarray(raw, dtype=np.float64)
    p.setflags(write=False)
    return p


PATTERN52 = _pattern52()


@dataclass
class PatchCovariance:
    """pnec_hip_patch_covariance's outputs, one row per keypoint; numpy or torch, matching the input."""
    cov: object        # [M,3] (xx, xy, yy): what Batch.fill_keypoints takes as cov2 / cov1; NaN unless status == 0
    hessian: object    # [M,6] upper triangle (00 01 02 11 12 22) of the SE(2) Hessian * scaling
    mean: object       # [M] mean patch intensity S / n
    n_valid: object    # [M] int32, pattern points inside the image
    status: object     # [M] int32: PATCH_OK, PATCH_EMPTY, PATCH_SINGULAR
    offsets: object = None       # int64 [F+1], numpy or torch like the rest

    def ok(self):
        return self.status == PATCH_OK


def _is_torch(a) -> bool:
    return type(a).__module__.split(".")[0] == "torch"


def _pixel_type(dtype_name: str) -> int:
    try:
        return {"uint8": PIXEL_U8, "uint16": PIXEL_U16, "float32": PIXEL_F32}[dtype_name]
    except KeyError:
        raise TypeError(f"images must be uint8, uint16 or float32, not {dtype_name}") from None


def patch_covariance(images, pts, offsets=None, pattern=PATTERN52, scaling: float = 10.0, angle=None,
                     outputs=("cov", "hessian", "mean", "n_valid", "status")) -> PatchCovariance:
    """Covariances of the keypoints `pts` [M,2] (x = column, y = row) of `images` [F,h,w] (or one image [h,w]), uint8 /
    uint16 / float32; keypoints [offsets[f], offsets[f+1]) lie in image f (offsets may be left out for one image).
    `pattern` [P,2] (P <= 64) are the patch's offsets in pixels, `scaling` divides the covariance (the reference's
    uncertainty_scaling = 10), `angle` [M] rotates it (the tracked transform's rotation, radians).  torch.cuda images ->
    everything stays on the device, asynchronous on torch's current stream, torch.cuda tensors out (rows of a strided
    image batch are read in place when each image's rows are evenly pitched and the images follow one another);
    numpy (or CPU tensors) in -> staged, numpy out."""
    on_device = _is_torch(images) and images.is_cuda
    if _is_torch(images) and not on_device:
        images = images.numpy()
    if images.ndim == 2:
        images = images[None]
    if images.ndim != 3:
        raise ValueError("images must be [F,h,w] or [h,w]")
    F, h, w = (int(x) for x in images.shape)
    if on_device:
        import torch
        ptype = _pixel_type(str(images.dtype).replace("torch.", ""))
        st = images.stride()
        if st[2] != 1 or st[1] < w or (F > 1 and st[0] != h * st[1]):
            images = images.contiguous()
            st = images.stride()
        pitch, dev = int(st[1]), images.device
        f64 = dict(dtype=torch.float64, device=dev)
        # (np.array copies: torch refuses to wrap a read-only array such as PATTERN52 without a warning)
        as_dev = lambda a, dt: a.to(device=dev, dtype=dt).contiguous() if _is_torch(a) else \
            torch.as_tensor(np.array(a), dtype=dt, device=dev)
        pts = as_dev(pts, torch.float64)
        M = int(pts.shape[0])
        offsets_d = as_dev(np.array([0, M], dtype=np.int64) if offsets is None else offsets, torch.int64)
        pattern_d = as_dev(pattern, torch.float64)
        angle_d = None if angle is None else as_dev(angle, torch.float64)
        new = {"cov": lambda: torch.empty((M, 3), **f64), "hessian": lambda: torch.empty((M, 6), **f64),
               "mean": lambda: torch.empty((M,), **f64),
               "n_valid": lambda: torch.empty((M,), dtype=torch.int32, device=dev),
               "status": lambda: torch.empty((M,), dtype=torch.int32, device=dev)}
        p = lambda a: None if a is None else a.data_ptr()
        device = dev.index if dev.index is not None else torch.cuda.current_device()
        space, stream = capi.MEM_DEVICE, torch.cuda.current_stream(device).cuda_stream
    else:
        images = np.asarray(images)
        ptype = _pixel_type(images.dtype.name)
        es = images.dtype.itemsize
        st = images.strides
        if st[2] != es or st[1] % es or st[1] < w * es or (F > 1 and st[0] != h * st[1]):
            images = np.ascontiguousarray(images)
            st = images.strides
        pitch = st[1] // es
        pts = np.ascontiguousarray(pts.cpu().numpy() if _is_torch(pts) else pts, dtype=np.float64)
        M = int(pts.shape[0])
        offsets_d = np.array([0, M], dtype=np.int64) if offsets is None else np.ascontiguousarray(offsets, dtype=np.int64)
        pattern_d = np.ascontiguousarray(pattern, dtype=np.float64)
        angle_d = None if angle is None else np.ascontiguousarray(angle, dtype=np.float64)
        new = {"cov": lambda: np.empty((M, 3)), "hessian": lambda: np.empty((M, 6)), "mean": lambda: np.empty(M),
               "n_valid": lambda: np.empty(M, dtype=np.int32), "status": lambda: np.empty(M, dtype=np.int32)}
        p = lambda a: None if a is None else a.ctypes.data
        device, space, stream = 0, capi.MEM_HOST, None
    if tuple(pts.shape) != (M, 2):
        raise ValueError("pts must be [M,2] (x = column, y = row)")
    if tuple(offsets_d.shape) != (F + 1,):
        raise ValueError("offsets must be [F+1] (one image: [0, M], or leave it out)")
    if pattern_d.ndim != 2 or pattern_d.shape[1] != 2:
        raise ValueError("pattern must be [P,2]")
    if angle_d is not None and tuple(angle_d.shape) != (M,):
        raise ValueError("angle must be [M]")
    unknown = set(outputs) - set(new)
    if unknown:
        raise ValueError(f"unknown outputs {sorted(unknown)}")
    out = {k: (new[k]() if k in outputs else None) for k in new}
    # (the image pointer is the first pixel of the first image as viewed: a cropped view starts at its own corner)
    capi.check(capi.lib().pnec_hip_patch_covariance(
        p(images), ptype, F, h, w, pitch, p(offsets_d), M, p(pts), p(pattern_d), int(pattern_d.shape[0]), float(scaling),
        p(angle_d), p(out["cov"]), p(out["hessian"]), p(out["mean"]), p(out["n_valid"]), p(out["status"]), space, device,
        stream))
    return PatchCovariance(out["cov"], out["hessian"], out["mean"], out["n_valid"], out["status"], offsets_d)
