"""Tracks across frames: the bookkeeping of KLTPatchOpticalFlow::processFrame (klt_patch_optical_flow.h:121-191) on the
device -- ``retain_tracks`` (``pnec_hip_tracks_retain``), ``append_tracks`` (``pnec_hip_tracks_append``) -- and
``Tracker``, the frame loop over them for F sequences in lockstep: images in, correspondences with covariances out, and
no host wait in the loop.  include/pnec_hip.h has the definitions.

DEVIATION from the reference, which keeps a track's patch for ever: ``Tracker`` keeps a ring of R pyramids, a track's
template is the frame it was born in, and a track is retired when its age would reach R - 1 (the step before its birth
frame's slot is overwritten).  The pair loses that track's correspondence on the step it is retired.
``Tracker(..., templates="patches")`` (stored patches, pnec_amd/patch_store.py) lifts it: a track keeps its templates for
as long as it is tracked.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import capi
from .patches import PATTERN52, Keypoints, PatchTrack, _is_torch, _ptype, detect_keypoints


@dataclass
class TrackSet:
    """A track set, ragged over F images: rows [offsets[f], offsets[f+1]) belong to image f, rows at and beyond offsets[F]
    are padding (id -1, tmpl_image 0, age 0, NaN).  numpy or torch, matching the input."""
    offsets: object      # int64 [F+1]
    id: object           # int64 [N], unique per image, >= 0
    tmpl_image: object   # int32 [N], the birth image in a stack of template images
    tmpl_pts: object     # [N,2] where the patch was built
    age: object          # int32 [N], frames since birth
    pts: object          # [N,2] the transform in the set's frame
    angle: object        # [N]
    cov: object = None   # [N,3] the 2x2 covariance there
    prev_pts: object = None   # retained sets: the same track's pts / cov in the set it was retained from,
    prev_cov: object = None   # and the row it had there (-1 in padding)
    src: object = None

    @property
    def rows(self) -> int:
        return int(self.id.shape[0])

    def fields(self):
        return (self.offsets, self.id, self.tmpl_image, self.tmpl_pts, self.age, self.pts, self.angle, self.cov)


def _kit(on_device, dev=None):
    """(new(shape, kind), as_in(a, kind), ptr(a)) for device tensors or numpy arrays; kind in 'f64', 'i64', 'i32'"""
    if on_device:
        import torch
        dt = {"f64": torch.float64, "i64": torch.int64, "i32": torch.int32}
        new = lambda shape, kind: torch.empty(shape, dtype=dt[kind], device=dev)
        as_in = lambda a, kind: a.to(device=dev, dtype=dt[kind]).contiguous() if _is_torch(a) else \
            torch.as_tensor(np.array(a), dtype=dt[kind], device=dev)
        ptr = lambda a: None if a is None else a.data_ptr()
    else:
        dt = {"f64": np.float64, "i64": np.int64, "i32": np.int32}
        new = lambda shape, kind: np.empty(shape, dtype=dt[kind])
        as_in = lambda a, kind: np.ascontiguousarray(a.cpu().numpy() if _is_torch(a) else a, dtype=dt[kind])
        ptr = lambda a: None if a is None else a.ctypes.data
    return new, as_in, ptr


def _where(ref, on_device):
    if not on_device:
        return capi.MEM_HOST, 0, None, None
    import torch
    dev = ref.device
    device = dev.index if dev.index is not None else torch.cuda.current_device()
    return capi.MEM_DEVICE, device, torch.cuda.current_stream(device).cuda_stream, dev


def new_track_set(n_images: int, rows: int, on_device: bool, device=None, cov: bool = True, retained: bool = False) -> TrackSet:
    """Uninitialised arrays of a set of `rows` rows (a retained one: with prev_pts, prev_cov and src)."""
    new, _, _ = _kit(on_device, device)
    N = int(rows)
    s = TrackSet(new((n_images + 1,), "i64"), new((N,), "i64"), new((N,), "i32"), new((N, 2), "f64"), new((N,), "i32"),
                 new((N, 2), "f64"), new((N,), "f64"), new((N, 3), "f64") if cov else None)
    if retained:
        s.prev_pts, s.src = new((N, 2), "f64"), new((N,), "i64")
        s.prev_cov = new((N, 3), "f64") if cov else None
    return s


def _set_in(tracks: TrackSet, as_in):
    c = lambda a, kind: None if a is None else as_in(a, kind)
    return TrackSet(c(tracks.offsets, "i64"), c(tracks.id, "i64"), c(tracks.tmpl_image, "i32"), c(tracks.tmpl_pts, "f64"),
                    c(tracks.age, "i32"), c(tracks.pts, "f64"), c(tracks.angle, "f64"), c(tracks.cov, "f64"))


def retain_tracks(tracks: TrackSet, track_result: PatchTrack, max_age: int = 0, out: TrackSet = None) -> TrackSet:
    """The tracks of `tracks` that `track_result` (patch_track's outputs for its rows) brought back with TRACK_OK --
    and, with max_age > 0, whose age + 1 stays <= max_age -- compacted per image in their order, age + 1, the track's
    pts / angle / cov, and prev_pts / prev_cov / src from the input set: the correspondences of the pair, in the form
    Batch(mode, offsets).fill_keypoints(prev_pts, pts, cov) takes.  The result has the rows of the input, padding written
    to the end.  torch.cuda in -> torch.cuda out, asynchronous on torch's current stream, nothing read back; numpy in ->
    staged, numpy out.  `out`: a retained set of the same shapes to write in place of new arrays."""
    on = _is_torch(tracks.id) and tracks.id.is_cuda
    space, device, stream, dev = _where(tracks.id, on)
    new, as_in, p = _kit(on, dev)
    t = _set_in(tracks, as_in)
    F, N = int(t.offsets.shape[0]) - 1, int(t.id.shape[0])
    r_pts, r_angle, r_status = as_in(track_result.pts, "f64"), as_in(track_result.angle, "f64"), as_in(track_result.status, "i32")
    with_cov = t.cov is not None and track_result.cov is not None
    r_cov = as_in(track_result.cov, "f64") if with_cov else None
    if tuple(r_pts.shape) != (N, 2) or tuple(r_angle.shape) != (N,) or tuple(r_status.shape) != (N,):
        raise ValueError("track_result must hold one row per row of the set")
    if out is None:
        out = new_track_set(F, N, on, dev, cov=with_cov, retained=True)
    elif out.rows != N or int(out.offsets.shape[0]) != F + 1 or (out.cov is None) != (not with_cov) or out.src is None:
        raise ValueError("`out` must be a retained set of the same shapes")
    capi.check(capi.lib().pnec_hip_tracks_retain(
        F, p(t.offsets), N, p(t.id), p(t.tmpl_image), p(t.tmpl_pts), p(t.age), p(t.pts), p(t.cov) if with_cov else None,
        p(r_pts), p(r_angle), p(r_cov), p(r_status), int(max_age), p(out.offsets), p(out.id), p(out.tmpl_image),
        p(out.tmpl_pts), p(out.age), p(out.pts), p(out.angle), p(out.cov), p(out.prev_pts), p(out.prev_cov), p(out.src),
        space, device, stream))
    return out


def append_tracks(tracks, keypoints: Keypoints, det_cov, tmpl_image_base: int, capacity: int, next_id, rows: int = None,
                  out: TrackSet = None, dropped=None):
    """`tracks` (a TrackSet, or None on the first frame) refilled with the detections `keypoints` (detect_keypoints'
    result, trimmed or in capacity form) and their covariances `det_cov` [n,3] (or None: NaN): per image the first
    min(a, capacity) set rows unchanged, then as many detections as still fit, each with the next id of `next_id` int64 [F]
    (updated in place), tmpl_image = tmpl_image_base + f, tmpl_pts = pts = the corner, age 0, angle 0.  Returns (the set
    of `rows` rows -- default min(F * capacity, rows in + detections in) --, dropped int64 [F]).  torch.cuda in -> torch.cuda
    out, asynchronous on torch's current stream, nothing read back; numpy in -> staged, numpy out.  `next_id` must be of
    the kind of the rest (it is written).  `out` / `dropped`: arrays to write in place of new ones."""
    ref = keypoints.pts
    on = _is_torch(ref) and ref.is_cuda
    space, device, stream, dev = _where(ref, on)
    new, as_in, p = _kit(on, dev)
    d_off, d_pts = as_in(keypoints.offsets, "i64"), as_in(keypoints.pts, "f64")
    d_cov = None if det_cov is None else as_in(det_cov, "f64")
    F, D = int(d_off.shape[0]) - 1, int(d_pts.shape[0])
    if d_cov is not None and tuple(d_cov.shape) != (D, 3):
        raise ValueError("det_cov must be [n,3], one row per row of keypoints.pts")
    if tracks is None:
        t, N = TrackSet(None, None, None, None, None, None, None, None), 0
    else:
        t = _set_in(tracks, as_in)
        N = int(t.id.shape[0])
        if int(t.offsets.shape[0]) != F + 1:
            raise ValueError("the set and the detections must cover the same images")
    if (on and not (_is_torch(next_id) and next_id.is_cuda)) or (not on and not isinstance(next_id, np.ndarray)):
        raise TypeError("next_id is written: a torch.cuda tensor with device inputs, a numpy array with host inputs")
    if str(next_id.dtype).replace("torch.", "") != "int64" or tuple(next_id.shape) != (F,) or \
            not (next_id.is_contiguous() if on else next_id.flags.c_contiguous):
        raise ValueError("next_id must be a contiguous int64 [F]")
    C = int(capacity)
    O = min(F * C, N + D) if rows is None else int(rows)
    with_cov = d_cov is not None or t.cov is not None
    if out is None:
        out = new_track_set(F, O, on, dev, cov=with_cov)
    elif out.rows != O or int(out.offsets.shape[0]) != F + 1:
        raise ValueError("`out` must be a set of `rows` rows")
    if dropped is None:
        dropped = new((F,), "i64")
    capi.check(capi.lib().pnec_hip_tracks_append(
        F, p(t.offsets), N, p(t.id), p(t.tmpl_image), p(t.tmpl_pts), p(t.age), p(t.pts), p(t.angle), p(t.cov), p(d_off), D,
        p(d_pts), p(d_cov), int(tmpl_image_base), C, p(next_id), O, p(out.offsets), p(out.id), p(out.tmpl_image),
        p(out.tmpl_pts), p(out.age), p(out.pts), p(out.angle), p(out.cov), p(dropped), space, device, stream))
    return out, dropped


class Tracker:
    """The device form of KLTPatchOpticalFlow::processFrame for `n_sequences` image sequences in lockstep.

    ``process(images)`` takes the next frame of every sequence ([F,h,w] torch.cuda, the pixel type of `dtype`) and returns
    the retained TrackSet -- the correspondences of the pair (previous frame, this frame): prev_pts, pts, cov, ragged by
    offsets, ready for ``Batch.fill_keypoints`` -- or None for the first frame.  ``tracks`` is the set after the refill,
    ``dropped`` int64 [F] what the last refill could not take, ``last_track`` the raw outputs of the last tracking call.

    A ring of `ring` = R >= 3 pyramids is kept as one stack of R * F images per level, frame n in slot n % R.  The first
    call runs pyramid, detect_keypoints, patch_covariance, tracks_append; every later call the six device calls pyramid ->
    patch_track_indexed (tmpl = the stack, prev / next = two slots, start = the set) -> tracks_retain (max_age = R - 2) ->
    detect_keypoints (current = the retained set, capacity form) -> patch_covariance -> tracks_append (tmpl_image_base =
    slot * F).  Every array is allocated here, in the constructor; NO CALL OF process READS ANYTHING BACK or waits: it is
    asynchronous on torch's current stream.  The sets it returns are the tracker's own buffers: the next call overwrites
    them.

    DEVIATION: the reference keeps a patch for ever; a track here is retired when its age would reach R - 1 (its birth
    frame's slot is about to be overwritten), which costs the pair that track's correspondence on that step.
    `templates="patches"` lifts it: the constructor allocates a PatchStore of F * capacity slots (``store``), `ring` may be
    2 (only the previous and this frame's pyramids are read), and every later call makes seven device calls: pyramid ->
    patch_track_stored (the templates from the store) -> tracks_retain (max_age = 0: no age limit) -> detect_keypoints ->
    patch_covariance -> tracks_append -> patch_store_add (a free slot and the templates for every new track).  Still
    nothing is read back or allocated in process.  The sets' `tmpl_image` column is then the track's slot.
    `templates="ring"`, the default, is the object described above in every respect."""

    def __init__(self, n_sequences: int, height: int, width: int, levels: int = 5, ring: int = 4, grid: int = 30,
                 capacity: int = None, points_per_cell: int = 1, min_threshold: int = 5, edge: int = 19,
                 max_iterations: int = 40, max_recovered_dist2: float = 0.04, scaling: float = 10.0, pattern=PATTERN52,
                 dtype=None, device=None, templates: str = "ring"):
        import torch
        F, h, w, L, R = int(n_sequences), int(height), int(width), int(levels), int(ring)
        if templates not in ("ring", "patches"):
            raise ValueError('templates must be "ring" or "patches"')
        if templates == "patches":
            if F < 1 or R < 2:
                raise ValueError("n_sequences must be >= 1 and ring >= 2")
        elif F < 1 or R < 3:
            raise ValueError("n_sequences must be >= 1 and ring >= 3")
        self.templates = templates
        if not 1 <= L <= 8 or (h >> (L - 1)) < 4 or (w >> (L - 1)) < 4:
            raise ValueError("levels must be 1 .. 8 and the smallest level at least 4 pixels in each direction")
        G, K = int(grid), int(points_per_cell)
        n_cells = (w // G) * (h // G)
        if n_cells < 1:
            raise ValueError("the images must be at least one grid cell in height and width")
        self.n_sequences, self.height, self.width, self.levels, self.ring = F, h, w, L, R
        self.grid, self.points_per_cell, self.min_threshold, self.edge = G, K, int(min_threshold), int(edge)
        self.capacity = n_cells * K if capacity is None else int(capacity)
        if self.capacity < 1:
            raise ValueError("capacity must be >= 1")
        self.max_iterations, self.max_recovered_dist2, self.scaling = int(max_iterations), float(max_recovered_dist2), float(scaling)
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        dtype = torch.uint8 if dtype is None else dtype
        if dtype not in (torch.uint8, getattr(torch, "uint16", torch.uint8)):
            raise TypeError("Tracker takes uint8 or uint16 images (detect_keypoints' pixel types)")
        self.device, self.dtype = dev, dtype
        self._stack = [torch.zeros((R * F, h >> l, w >> l), dtype=dtype, device=dev) for l in range(L)]
        N = F * self.capacity
        self._N = N
        self._sets = [new_track_set(F, N, True, dev), new_track_set(F, N, True, dev)]
        self._retained = new_track_set(F, N, True, dev, retained=True)
        f64 = dict(dtype=torch.float64, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        self.last_track = PatchTrack(torch.empty((N, 2), **f64), torch.empty((N,), **f64), torch.empty((N, 3), **f64),
                                     torch.empty((N,), **f64), torch.empty((N,), **i32), torch.empty((N,), **i32))
        cap = F * n_cells * K
        self._det = Keypoints(torch.zeros((F + 1,), dtype=torch.int64, device=dev),
                              torch.full((cap, 2), float("nan"), **f64), torch.zeros((cap,), **i32),
                              torch.zeros((cap,), **i32), torch.zeros((F, n_cells), **i32))
        self._det_cov = torch.empty((cap, 3), **f64)
        self._pattern = torch.as_tensor(np.array(pattern), **f64).contiguous()
        self.store = None
        if templates == "patches":
            from .patch_store import new_patch_store
            self.store = new_patch_store(F, self.capacity, L, dev)
        self.next_id = torch.zeros((F,), dtype=torch.int64, device=dev)
        self.dropped = torch.zeros((F,), dtype=torch.int64, device=dev)
        self.frame = 0          # the number of frames processed
        self._cur = 0           # which of _sets is `tracks`
        self.tracks = None
        import ctypes as C
        self._C = C

    def _slot(self, n: int):
        F = self.n_sequences
        s = n % self.ring
        return [lv[s * F:(s + 1) * F] for lv in self._stack]

    def _tables(self, pyr):
        C = self._C
        return ((C.c_void_p * self.levels)(*[lv.data_ptr() for lv in pyr]),
                (C.c_int64 * self.levels)(*[int(lv.stride()[1]) for lv in pyr]))

    def process(self, images) -> TrackSet:
        import torch
        F, h, w, L = self.n_sequences, self.height, self.width, self.levels
        if not (_is_torch(images) and images.is_cuda) or tuple(images.shape) != (F, h, w) or images.dtype != self.dtype:
            raise ValueError(f"images must be a torch.cuda [{F},{h},{w}] batch of {self.dtype}")
        lib = capi.lib()
        device = self.device.index
        stream = torch.cuda.current_stream(device).cuda_stream
        n = self.frame
        cur = self._slot(n)
        ptype = _ptype(cur[0], True)
        cur[0].copy_(images, non_blocking=True)
        for l in range(1, L):
            capi.check(lib.pnec_hip_image_pyramid_level(cur[l - 1].data_ptr(), cur[l].data_ptr(), ptype, F, h >> (l - 1),
                                                        w >> (l - 1), w >> (l - 1), w >> l, capi.MEM_DEVICE, device, stream))
        p = lambda a: None if a is None else a.data_ptr()
        N, pat = self._N, self._pattern
        retained = None
        if n > 0:
            A, T, B = self._sets[self._cur], self.last_track, self._retained
            pp, pq = self._tables(self._slot(n - 1))
            np_, nq = self._tables(cur)
            if self.store is not None:
                capi.check(lib.pnec_hip_patch_track_stored(
                    p(self.store.data), self.store.n_slots, pp, pq, np_, nq, L, ptype, F, h, w, p(A.offsets), N, p(A.tmpl_pts),
                    p(A.tmpl_image), p(A.pts), p(A.angle), 0.0, 0.0, p(pat), int(pat.shape[0]), self.max_iterations,
                    self.max_recovered_dist2, 0, self.scaling, p(T.pts), p(T.angle), p(T.cov), p(T.dist2), p(T.status),
                    p(T.lost_level), capi.MEM_DEVICE, device, stream))
            else:
                tp, tq = self._tables(self._stack)
                capi.check(lib.pnec_hip_patch_track_indexed(
                    tp, tq, self.ring * F, pp, pq, np_, nq, L, ptype, F, h, w, p(A.offsets), N, p(A.tmpl_pts), p(A.tmpl_image),
                    p(A.pts), p(A.angle), 0.0, 0.0, p(pat), int(pat.shape[0]), self.max_iterations, self.max_recovered_dist2, 0,
                    self.scaling, p(T.pts), p(T.angle), p(T.cov), p(T.dist2), p(T.status), p(T.lost_level), capi.MEM_DEVICE,
                    device, stream))
            T.offsets = A.offsets
            retained = retain_tracks(A, T, max_age=0 if self.store is not None else self.ring - 2, out=B)
        det = detect_keypoints(cur[0], self.grid, self.points_per_cell, self.min_threshold, self.edge,
                               current=None if retained is None else (retained.offsets, retained.pts), capacity=True,
                               out=self._det)
        D = int(det.pts.shape[0])
        capi.check(lib.pnec_hip_patch_covariance(
            cur[0].data_ptr(), ptype, F, h, w, w, p(det.offsets), D, p(det.pts), p(pat), int(pat.shape[0]), self.scaling,
            None, p(self._det_cov), None, None, None, None, capi.MEM_DEVICE, device, stream))
        nxt = self._sets[1 - self._cur]
        append_tracks(retained, det, self._det_cov, (n % self.ring) * F, self.capacity, self.next_id, rows=N, out=nxt,
                      dropped=self.dropped)
        if self.store is not None:
            cp, cq = self._tables(cur)
            capi.check(lib.pnec_hip_patch_store_add(
                cp, cq, L, ptype, F, h, w, None if retained is None else p(retained.offsets), p(nxt.offsets), N,
                p(nxt.tmpl_pts), p(nxt.tmpl_image), self.capacity, p(pat), int(pat.shape[0]), p(self.store.data),
                self.store.n_slots, capi.MEM_DEVICE, device, stream))
        self._cur = 1 - self._cur
        self.tracks = nxt
        self.frame = n + 1
        return retained
