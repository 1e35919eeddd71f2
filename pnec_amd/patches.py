"""Patch covariances: the 2x2 image covariance of keypoints from the image patches around them
(``pnec_hip_patch_covariance``; include/pnec_hip.h has the definition) -- the ``cov2`` / ``cov1`` input of
``Batch.fill_keypoints``, computed on the device from images and keypoint positions.

This is the covariance POpticalFlowPatch::setFromImage keeps (include/features/tracking/pnec_patch.h:78-137) after
KLTPatchOpticalFlow's scaling and rotation.  It is double arithmetic, not the reference's float: no float parity is
claimed.

Patch tracking: ``image_pyramid`` (``pnec_hip_image_pyramid_level``) and ``patch_track`` (``pnec_hip_patch_track``), the
pyramidal SE(2) KLT iteration with its forward-backward check (klt_patch_optical_flow.h:195-342) -- the producer of the
positions and of ``angle`` above.  Keypoint ids and the bookkeeping of tracks across frames are tracker.py's; the view
graph is not here.

Keypoint detection: ``detect_keypoints`` (``pnec_hip_detect_keypoints``), grid FAST-9 corners as
KLTPatchOpticalFlow::addPoints gets them (klt_patch_optical_flow.h:344-385) -- the producer of ``tmpl_pts``.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import capi

PATCH_OK, PATCH_EMPTY, PATCH_SINGULAR = 0, 1, 2      # pnec_hip_patch_status
PATCH_NAMES = {PATCH_OK: "ok", PATCH_EMPTY: "empty_patch", PATCH_SINGULAR: "singular_hessian"}
PIXEL_U8, PIXEL_U16, PIXEL_F32 = 0, 1, 2             # pnec_hip_pixel_type
PATCH_MAX_POINTS = 64
TRACK_OK, TRACK_BAD_TEMPLATE, TRACK_LOST_FORWARD, TRACK_LOST_BACKWARD, TRACK_RECOVERED_TOO_FAR = range(5)  # pnec_hip_track_status
TRACK_NAMES = {TRACK_OK: "ok", TRACK_BAD_TEMPLATE: "bad_template", TRACK_LOST_FORWARD: "lost_forward",
               TRACK_LOST_BACKWARD: "lost_backward", TRACK_RECOVERED_TOO_FAR: "recovered_too_far"}
TRACK_MAX_LEVELS = 8
TRACK_NO_BACKWARD = 1
DETECT_MIN_GRID, DETECT_MAX_GRID, DETECT_MAX_PER_CELL, DETECT_MAX_THRESHOLD = 8, 64, 4, 254


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


@dataclass
class PatchTrack:
    """pnec_hip_patch_track's outputs, one row per keypoint; numpy or torch, matching the input."""
    pts: object          # [M,2] the tracked translation in `next` (where the forward track stood last, also when lost)
    angle: object        # [M] the tracked rotation, radians: patch_covariance's `angle`
    cov: object          # [M,3] (xx, xy, yy) of the level-0 template, rotated and scaled; NaN unless status == 0
    dist2: object        # [M] squared forward-backward distance; NaN when the backward track did not finish
    status: object       # [M] int32: TRACK_OK, TRACK_BAD_TEMPLATE, TRACK_LOST_FORWARD, TRACK_LOST_BACKWARD, TRACK_RECOVERED_TOO_FAR
    lost_level: object   # [M] int32: the level of a bad template or a loss, -1 otherwise
    offsets: object = None

    def ok(self):
        return self.status == TRACK_OK


def _as_batch(images):
    """images as ([F,h,w] array or tensor with unit pixel stride and evenly pitched images, on_device)"""
    on_device = _is_torch(images) and images.is_cuda
    if _is_torch(images) and not on_device:
        images = images.numpy()
    if not on_device:
        images = np.asarray(images)
    if images.ndim == 2:
        images = images[None]
    if images.ndim != 3:
        raise ValueError("images must be [F,h,w] or [h,w]")
    F, h, w = (int(x) for x in images.shape)
    if on_device:
        _pixel_type(str(images.dtype).replace("torch.", ""))
        st = images.stride()
        if st[2] != 1 or st[1] < w or (F > 1 and st[0] != h * st[1]):
            images = images.contiguous()
    else:
        _pixel_type(images.dtype.name)
        es, st = images.dtype.itemsize, images.strides
        if st[2] != es or st[1] % es or st[1] < w * es or (F > 1 and st[0] != h * st[1]):
            images = np.ascontiguousarray(images)
    return images, on_device


def _pitch(images, on_device) -> int:
    return int(images.stride()[1]) if on_device else images.strides[1] // images.dtype.itemsize


def _ptype(images, on_device) -> int:
    return _pixel_type(str(images.dtype).replace("torch.", "") if on_device else images.dtype.name)


def _where(images, on_device):
    """(space, device, stream) of a call on `images`"""
    if not on_device:
        return capi.MEM_HOST, 0, None
    import torch
    dev = images.device
    device = dev.index if dev.index is not None else torch.cuda.current_device()
    return capi.MEM_DEVICE, device, torch.cuda.current_stream(device).cuda_stream


def image_pyramid(images, levels: int) -> list:
    """The `levels` levels (1 .. 8) of the pyramid of `images` [F,h,w] (or one image [h,w]), uint8 / uint16 / float32:
    a list whose entry 0 is the input (as a [F,h,w] batch, not copied when its rows are evenly pitched) and whose entry l
    is entry l - 1 halved by pnec_hip_image_pyramid_level (5-tap binomial filter, reflected borders, sizes floored).
    torch.cuda in -> device tensors out, asynchronous on torch's current stream; numpy in -> numpy out."""
    if not 1 <= int(levels) <= TRACK_MAX_LEVELS:
        raise ValueError(f"levels must be 1 .. {TRACK_MAX_LEVELS}")
    images, on_device = _as_batch(images)
    space, device, stream = _where(images, on_device)
    ptype = _ptype(images, on_device)
    out = [images]
    for _ in range(1, int(levels)):
        src = out[-1]
        F, h, w = (int(x) for x in src.shape)
        if on_device:
            import torch
            dst = torch.empty((F, h // 2, w // 2), dtype=src.dtype, device=src.device)
            ps, pd = src.data_ptr(), dst.data_ptr()
        else:
            dst = np.empty((F, h // 2, w // 2), dtype=src.dtype)
            ps, pd = src.ctypes.data, dst.ctypes.data
        capi.check(capi.lib().pnec_hip_image_pyramid_level(ps, pd, ptype, F, h, w, _pitch(src, on_device), w // 2, space,
                                                          device, stream))
        out.append(dst)
    return out


def patch_track(tmpl, next, tmpl_pts, offsets=None, prev=None, init_pts=None, init_angle=None, shift=(0.0, 0.0),
                pattern=PATTERN52, max_iterations: int = 40, max_recovered_dist2: float = 0.04, backward: bool = True,
                scaling: float = 10.0, outputs=("pts", "angle", "cov", "dist2", "status", "lost_level"),
                tmpl_image=None) -> PatchTrack:
    """Tracks the patches built at `tmpl_pts` [M,2] (level-0 pixels, x = column, y = row) in the pyramid `tmpl` into the
    pyramid `next`, and back into `prev` (None: `tmpl`) for the forward-backward check.  A pyramid is a list of [F,h_l,w_l]
    batches as image_pyramid returns it; keypoints [offsets[f], offsets[f+1]) lie in image f.  `init_pts` / `init_angle`
    are the transform in `prev` (None: tmpl_pts / 0), `shift` is added to the forward start.  All pyramids in torch.cuda
    tensors -> everything stays on the device, asynchronous on torch's current stream, torch.cuda tensors out; numpy in
    -> staged, numpy out.

    `tmpl_image` int32 [M] (``pnec_hip_patch_track_indexed``): `tmpl` is then a stack of any number of images per level
    and keypoint k builds its templates, and its `cov`, in image tmpl_image[k] of it; `prev` must be given, and `prev` /
    `next` stay indexed by the keypoint's own image.  None: the keypoint's own image, `pnec_hip_patch_track` as before."""
    if tmpl_image is not None and prev is None:
        raise ValueError("with tmpl_image, prev must be given: tmpl is a stack of other images")
    pyrs = {"tmpl": tmpl, "next": next, "prev": prev}
    levels = len(tmpl)
    norm, on = {}, None
    for name, pyr in pyrs.items():
        if pyr is None:
            continue
        if len(pyr) != levels:
            raise ValueError("the pyramids must have the same number of levels")
        got = [_as_batch(lv) for lv in pyr]
        if any(d != got[0][1] for _, d in got) or (on is not None and got[0][1] != on):
            raise ValueError("the pyramids must all be on the device or all on the host")
        on = got[0][1]
        norm[name] = [a for a, _ in got]
    if not 1 <= levels <= TRACK_MAX_LEVELS:
        raise ValueError(f"a pyramid must have 1 .. {TRACK_MAX_LEVELS} levels")
    base = norm["tmpl"][0]
    Ft, h, w = (int(x) for x in base.shape)
    F = Ft if tmpl_image is None else int(norm["next"][0].shape[0])
    ptype = _ptype(base, on)
    for name, pyr in norm.items():
        n = Ft if name == "tmpl" else F
        for l, lv in enumerate(pyr):
            if tuple(int(x) for x in lv.shape) != (n, h >> l, w >> l) or _ptype(lv, on) != ptype:
                raise ValueError(f"level {l} of {name} must be [{n},{h >> l},{w >> l}] of the pyramid's pixel type")
    space, device, stream = _where(base, on)
    if on:
        import torch
        dev = base.device
        f64 = dict(dtype=torch.float64, device=dev)
        as_in = lambda a, dt: a.to(device=dev, dtype=dt).contiguous() if _is_torch(a) else \
            torch.as_tensor(np.array(a), dtype=dt, device=dev)
        F64, I64 = torch.float64, torch.int64
        p = lambda a: None if a is None else a.data_ptr()
        M = int(tmpl_pts.shape[0])
        new = {"pts": lambda: torch.empty((M, 2), **f64), "angle": lambda: torch.empty((M,), **f64),
               "cov": lambda: torch.empty((M, 3), **f64), "dist2": lambda: torch.empty((M,), **f64),
               "status": lambda: torch.empty((M,), dtype=torch.int32, device=dev),
               "lost_level": lambda: torch.empty((M,), dtype=torch.int32, device=dev)}
    else:
        as_in = lambda a, dt: np.ascontiguousarray(a.cpu().numpy() if _is_torch(a) else a, dtype=dt)
        F64, I64 = np.float64, np.int64
        p = lambda a: None if a is None else a.ctypes.data
        M = int(np.shape(tmpl_pts)[0])
        new = {"pts": lambda: np.empty((M, 2)), "angle": lambda: np.empty(M), "cov": lambda: np.empty((M, 3)),
               "dist2": lambda: np.empty(M), "status": lambda: np.empty(M, dtype=np.int32),
               "lost_level": lambda: np.empty(M, dtype=np.int32)}
    tmpl_pts = as_in(tmpl_pts, F64)
    offsets_d = as_in(np.array([0, M], dtype=np.int64) if offsets is None else offsets, I64)
    init_pts = None if init_pts is None else as_in(init_pts, F64)
    init_angle = None if init_angle is None else as_in(init_angle, F64)
    pattern_d = as_in(pattern, F64)
    if tmpl_image is not None:
        tmpl_image = as_in(tmpl_image, torch.int32 if on else np.int32)
        if tuple(tmpl_image.shape) != (M,):
            raise ValueError("tmpl_image must be [M]")
    if tuple(tmpl_pts.shape) != (M, 2) or (init_pts is not None and tuple(init_pts.shape) != (M, 2)):
        raise ValueError("tmpl_pts and init_pts must be [M,2] (x = column, y = row)")
    if init_angle is not None and tuple(init_angle.shape) != (M,):
        raise ValueError("init_angle must be [M]")
    if tuple(offsets_d.shape) != (F + 1,):
        raise ValueError("offsets must be [F+1] (one image: [0, M], or leave it out)")
    if pattern_d.ndim != 2 or pattern_d.shape[1] != 2:
        raise ValueError("pattern must be [P,2]")
    unknown = set(outputs) - set(new)
    if unknown:
        raise ValueError(f"unknown outputs {sorted(unknown)}")
    out = {k: (new[k]() if k in outputs else None) for k in new}

    import ctypes as C

    def table(pyr):
        if pyr is None:
            return None, None
        ptrs = (C.c_void_p * levels)(*[p(lv) for lv in pyr])
        pitches = (C.c_int64 * levels)(*[_pitch(lv, on) for lv in pyr])
        return ptrs, pitches
    tp, tq = table(norm["tmpl"])
    pp, pq = table(norm.get("prev"))
    np_, nq = table(norm["next"])
    if tmpl_image is not None:
        capi.check(capi.lib().pnec_hip_patch_track_indexed(
            tp, tq, Ft, pp, pq, np_, nq, levels, ptype, F, h, w, p(offsets_d), M, p(tmpl_pts), p(tmpl_image), p(init_pts),
            p(init_angle), float(shift[0]), float(shift[1]), p(pattern_d), int(pattern_d.shape[0]), int(max_iterations),
            float(max_recovered_dist2), 0 if backward else TRACK_NO_BACKWARD, float(scaling), p(out["pts"]),
            p(out["angle"]), p(out["cov"]), p(out["dist2"]), p(out["status"]), p(out["lost_level"]), space, device, stream))
        return PatchTrack(out["pts"], out["angle"], out["cov"], out["dist2"], out["status"], out["lost_level"], offsets_d)
    capi.check(capi.lib().pnec_hip_patch_track(
        tp, tq, pp, pq, np_, nq, levels, ptype, F, h, w, p(offsets_d), M, p(tmpl_pts), p(init_pts), p(init_angle),
        float(shift[0]), float(shift[1]), p(pattern_d), int(pattern_d.shape[0]), int(max_iterations),
        float(max_recovered_dist2), 0 if backward else TRACK_NO_BACKWARD, float(scaling), p(out["pts"]), p(out["angle"]),
        p(out["cov"]), p(out["dist2"]), p(out["status"]), p(out["lost_level"]), space, device, stream))
    return PatchTrack(out["pts"], out["angle"], out["cov"], out["dist2"], out["status"], out["lost_level"], offsets_d)


@dataclass
class Keypoints:
    """pnec_hip_detect_keypoints' outputs; numpy or torch, matching the input.  Trimmed to offsets[-1] rows, or (the
    `capacity` form) all F * n_cells * K rows of which the first offsets[-1] are written."""
    offsets: object      # int64 [F+1]: points [offsets[f], offsets[f+1]) lie in image f
    pts: object          # [N,2] x = column, y = row: integers in doubles, patch_track's tmpl_pts
    score: object        # [N] int32: cv::FAST's score, m - 1
    cell_index: object   # [N] int32: cx * ny + cy
    cell: object         # [F, n_cells] int32: points per cell, -1 for a cell a current point occupies
    grid_shape: tuple = None     # (nx, ny)
    grid_origin: tuple = None    # (x_start, y_start)


def detect_keypoints(images, grid: int = 30, points_per_cell: int = 1, min_threshold: int = 5, edge: int = 19,
                     current=None, capacity: bool = False, out: Keypoints = None) -> Keypoints:
    """Grid FAST-9 corners of `images` [F,h,w] (or one image [h,w]), uint8 or uint16 (read as v >> 8): in every
    `grid` x `grid` cell that none of the `current` points lies in, the up to `points_per_cell` strongest corners above
    `min_threshold` that are 3 x 3 maxima and at least `edge` pixels inside the image (include/pnec_hip.h has the
    definition).  `current` = the tuple (offsets [F+1], pts [n,2]) or, for one image, pts [n,2] (an array or a tensor).

    torch.cuda images -> everything stays on the device, asynchronous on torch's current stream, torch.cuda tensors out;
    numpy (or CPU tensors) in -> staged, numpy out.  The arrays are trimmed to offsets[-1] rows: on the device THIS IS THE
    ONE PLACE A SIZE IS READ BACK (one 8-byte copy that waits for the stream).  capacity=True returns the untrimmed arrays
    -- F * n_cells * points_per_cell rows, the first offsets[-1] written -- without any wait, so a caller in a frame loop
    never synchronises; `out` (a capacity-form result of the same shapes) is written in place of new arrays."""
    images, on_device = _as_batch(images)
    ptype = _ptype(images, on_device)
    if ptype == PIXEL_F32:
        raise TypeError("detect_keypoints takes uint8 or uint16 images: a float image has no declared range to quantise")
    F, h, w = (int(x) for x in images.shape)
    G, K = int(grid), int(points_per_cell)
    if not DETECT_MIN_GRID <= G <= DETECT_MAX_GRID:
        raise ValueError(f"grid must be {DETECT_MIN_GRID} .. {DETECT_MAX_GRID}")
    if not 1 <= K <= DETECT_MAX_PER_CELL:
        raise ValueError(f"points_per_cell must be 1 .. {DETECT_MAX_PER_CELL}")
    if h < G or w < G:
        raise ValueError("the images must be at least one grid cell in height and width")
    nx, ny = w // G, h // G
    n_cells, cap = nx * ny, F * nx * ny * K
    space, device, stream = _where(images, on_device)
    if on_device:
        import torch
        dev = images.device
        as_in = lambda a, dt: a.to(device=dev, dtype=dt).contiguous() if _is_torch(a) else \
            torch.as_tensor(np.array(a), dtype=dt, device=dev)
        F64, I64 = torch.float64, torch.int64
        p = lambda a: None if a is None else a.data_ptr()
        new = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
        I32 = torch.int32
    else:
        as_in = lambda a, dt: np.ascontiguousarray(a.cpu().numpy() if _is_torch(a) else a, dtype=dt)
        F64, I64, I32 = np.float64, np.int64, np.int32
        p = lambda a: None if a is None else a.ctypes.data
        new = lambda shape, dt: np.empty(shape, dtype=dt)
    cur_offsets = cur_pts = None
    n_cur = 0
    if current is not None:
        if isinstance(current, tuple) and len(current) == 2:
            cur_offsets, cur_pts = as_in(current[0], I64), as_in(current[1], F64)
        else:
            if F != 1:
                raise ValueError("current points of several images come as (offsets, pts)")
            cur_pts = as_in(current, F64)
            cur_offsets = as_in(np.array([0, int(cur_pts.shape[0])], dtype=np.int64), I64)
        if cur_pts.ndim != 2 or cur_pts.shape[1] != 2 or tuple(cur_offsets.shape) != (F + 1,):
            raise ValueError("current must be (offsets [F+1], pts [n,2])")
        n_cur = int(cur_pts.shape[0])
    if out is None:
        out = Keypoints(new((F + 1,), I64), new((cap, 2), F64), new((cap,), I32), new((cap,), I32), new((F, n_cells), I32))
    elif (tuple(out.offsets.shape), tuple(out.pts.shape), tuple(out.score.shape), tuple(out.cell_index.shape),
          tuple(out.cell.shape)) != ((F + 1,), (cap, 2), (cap,), (cap,), (F, n_cells)):
        raise ValueError("`out` must be a capacity-form result of the same images, grid and points_per_cell")
    capi.check(capi.lib().pnec_hip_detect_keypoints(
        p(images), ptype, F, h, w, _pitch(images, on_device), G, K, int(min_threshold), int(edge), p(cur_offsets), n_cur,
        p(cur_pts), p(out.cell), p(out.offsets), p(out.pts), p(out.score), p(out.cell_index), space, device, stream))
    shape, origin = (nx, ny), ((w % G) // 2, (h % G) // 2)
    if capacity:
        return Keypoints(out.offsets, out.pts, out.score, out.cell_index, out.cell, shape, origin)
    n = int(out.offsets[-1])     # (on the device: the read-back)
    return Keypoints(out.offsets, out.pts[:n], out.score[:n], out.cell_index[:n], out.cell, shape, origin)
