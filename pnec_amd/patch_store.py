"""Stored patches: a track keeps its templates for as long as it lives, as the reference's OpticalFlowPatch does
(klt_patch_optical_flow.h:344-385, :228) -- ``PatchStore`` / ``new_patch_store``, ``add_patches``
(``pnec_hip_patch_store_add``) and ``patch_track_stored`` (``pnec_hip_patch_track_stored``).  include/pnec_hip.h has the
definitions.

A store holds one slot per track, filled from the frame the track was born in; the track set's ``tmpl_image`` column is
then the track's slot, which ``retain_tracks`` and ``append_tracks`` carry along as they carry an image index.
``Tracker(..., templates="patches")`` is the frame loop over it: no ring of pyramids, no age limit.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import capi
from .patches import (PATTERN52, TRACK_MAX_LEVELS, TRACK_NO_BACKWARD, PatchTrack, _as_batch, _is_torch, _pitch, _ptype)
from .tracker import TrackSet, _kit, _where


@dataclass
class PatchStore:
    """`data`: uint8 [n_slots, slot_bytes] (torch.cuda or numpy), one slot per track: slot f * per_image_capacity + i is
    image f's i-th.  The layout of a slot is the library's own (include/pnec_hip.h)."""
    data: object
    n_levels: int
    per_image_capacity: int

    @property
    def n_slots(self) -> int:
        return int(self.data.shape[0])


def slot_bytes(n_levels: int) -> int:
    """pnec_hip_patch_store_slot_bytes: the size of one slot; 0 for n_levels outside 1 .. 8"""
    return int(capi.lib().pnec_hip_patch_store_slot_bytes(int(n_levels)))


def new_patch_store(n_images: int, per_image_capacity: int, n_levels: int, device=None) -> PatchStore:
    """A store of n_images * per_image_capacity zeroed slots for pyramids of `n_levels` levels, on `device` (None: torch's
    current CUDA device; "cpu": a numpy store for HOST-space calls)."""
    F, cap, L = int(n_images), int(per_image_capacity), int(n_levels)
    size = slot_bytes(L)
    if F < 1 or cap < 1 or size == 0:
        raise ValueError("n_images and per_image_capacity must be >= 1 and n_levels 1 .. 8")
    if F * cap > 2 ** 31 - 1:
        raise ValueError("n_images * per_image_capacity must fit int32 (a slot is an int32)")
    if device is not None and str(device) == "cpu":
        return PatchStore(np.zeros((F * cap, size), dtype=np.uint8), L, cap)
    import torch
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    return PatchStore(torch.zeros((F * cap, size), dtype=torch.uint8, device=dev), L, cap)


def _store_ptr(store: PatchStore, on: bool):
    d = store.data
    if on != (_is_torch(d) and d.is_cuda):
        raise ValueError("the store must be where the pyramid and the set are (torch.cuda with device inputs, numpy with host inputs)")
    if tuple(d.shape) != (store.n_slots, slot_bytes(store.n_levels)) or not (d.is_contiguous() if on else d.flags.c_contiguous):
        raise ValueError("store.data must be a contiguous uint8 [n_slots, slot_bytes]")
    return d.data_ptr() if on else d.ctypes.data


def _pyramid(pyr, name, levels, on=None, shape=None, ptype=None):
    """the levels of `pyr` as batches -> (list, on_device, (F, h, w), pixel type)"""
    if len(pyr) != levels:
        raise ValueError(f"{name} must have the store's {levels} levels")
    got = [_as_batch(lv) for lv in pyr]
    if any(d != got[0][1] for _, d in got) or (on is not None and got[0][1] != on):
        raise ValueError("the pyramids must all be on the device or all on the host")
    on = got[0][1]
    lv = [a for a, _ in got]
    F, h, w = (int(x) for x in lv[0].shape)
    pt = _ptype(lv[0], on)
    if (shape is not None and shape != (F, h, w)) or (ptype is not None and ptype != pt):
        raise ValueError(f"{name} must have the shape and the pixel type of the other pyramid")
    for l, a in enumerate(lv):
        if tuple(int(x) for x in a.shape) != (F, h >> l, w >> l) or _ptype(a, on) != pt:
            raise ValueError(f"level {l} of {name} must be [{F},{h >> l},{w >> l}] of the pyramid's pixel type")
    return lv, on, (F, h, w), pt


def _table(pyr, on):
    n = len(pyr)
    return ((C.c_void_p * n)(*[(lv.data_ptr() if on else lv.ctypes.data) for lv in pyr]),
            (C.c_int64 * n)(*[_pitch(lv, on) for lv in pyr]))


def add_patches(store: PatchStore, pyramid, tracks: TrackSet, carried_offsets=None, pattern=PATTERN52) -> TrackSet:
    """Gives every new row of `tracks` -- the set append_tracks made from a retained set whose offsets are
    `carried_offsets` (None: the first frame, every row is new) -- a free slot of its image, builds its templates at
    tracks.tmpl_pts in `pyramid` (the frame the rows were detected in, image_pyramid's list) and writes them there.
    `tracks.tmpl_image` is read (the carried rows' slots) and WRITTEN IN PLACE (the new rows' slots, -1 in padding); it
    must be a contiguous int32 array of the kind of the rest.  Returns `tracks`.  torch.cuda in -> asynchronous on torch's
    current stream, nothing read back (give `pattern` as a device tensor: a host one is copied up first); numpy in ->
    staged."""
    L = int(store.n_levels)
    pyr, on, (F, h, w), ptype = _pyramid(pyramid, "pyramid", L)
    space, device, stream, dev = _where(pyr[0], on)
    _, as_in, p = _kit(on, dev)
    slot = tracks.tmpl_image
    ok_kind = (_is_torch(slot) and slot.is_cuda) if on else isinstance(slot, np.ndarray)
    if not ok_kind or str(slot.dtype).replace("torch.", "") != "int32" or not (slot.is_contiguous() if on else slot.flags.c_contiguous):
        raise TypeError("tracks.tmpl_image is written: a contiguous int32 torch.cuda tensor with device inputs, numpy with host inputs")
    offsets, tmpl_pts = as_in(tracks.offsets, "i64"), as_in(tracks.tmpl_pts, "f64")
    carried = None if carried_offsets is None else as_in(carried_offsets, "i64")
    N = int(slot.shape[0])
    if tuple(offsets.shape) != (F + 1,) or tuple(tmpl_pts.shape) != (N, 2) or (carried is not None and tuple(carried.shape) != (F + 1,)):
        raise ValueError("offsets and carried_offsets must be [F+1] for the pyramid's F images, tmpl_pts [N,2]")
    pat = as_in(pattern, "f64")
    if pat.ndim != 2 or pat.shape[1] != 2:
        raise ValueError("pattern must be [P,2]")
    tp, tq = _table(pyr, on)
    capi.check(capi.lib().pnec_hip_patch_store_add(
        tp, tq, L, ptype, F, h, w, p(carried), p(offsets), N, p(tmpl_pts), p(slot), int(store.per_image_capacity), p(pat),
        int(pat.shape[0]), _store_ptr(store, on), store.n_slots, space, device, stream))
    return tracks


def patch_track_stored(store: PatchStore, prev, next, tracks_or_arrays, shift=(0.0, 0.0), pattern=PATTERN52,
                       max_iterations: int = 40, max_recovered_dist2: float = 0.04, backward: bool = True,
                       scaling: float = 10.0, outputs=("pts", "angle", "cov", "dist2", "status", "lost_level")) -> PatchTrack:
    """patch_track with the templates read from `store`: tracks the rows of a TrackSet whose tmpl_image column holds
    slots (add_patches) from the pyramid `prev`, where they stand at tracks.pts / tracks.angle, into the pyramid `next`,
    and back.  `tracks_or_arrays`: a TrackSet, or a tuple (offsets, tmpl_pts, slot[, init_pts[, init_angle]]).  A row
    whose slot is outside the store (the -1 of padding) comes back TRACK_BAD_TEMPLATE at the top level.  `pattern` must be
    the one the slots were built with.  Everything else is patch_track's; torch.cuda in -> torch.cuda out, asynchronous on
    torch's current stream; numpy in -> staged, numpy out."""
    L = int(store.n_levels)
    if not 1 <= L <= TRACK_MAX_LEVELS:
        raise ValueError(f"a store has 1 .. {TRACK_MAX_LEVELS} levels")
    pv, on, shape, ptype = _pyramid(prev, "prev", L)
    nx, _, _, _ = _pyramid(next, "next", L, on, shape, ptype)
    F, h, w = shape
    space, device, stream, dev = _where(pv[0], on)
    new, as_in, p = _kit(on, dev)
    if isinstance(tracks_or_arrays, TrackSet):
        t = tracks_or_arrays
        arrays = (t.offsets, t.tmpl_pts, t.tmpl_image, t.pts, t.angle)
    else:
        arrays = tuple(tracks_or_arrays) + (None,) * (5 - len(tracks_or_arrays))
        if len(arrays) != 5:
            raise ValueError("arrays must be (offsets, tmpl_pts, slot[, init_pts[, init_angle]])")
    c = lambda a, kind: None if a is None else as_in(a, kind)
    offsets, tmpl_pts, slot = as_in(arrays[0], "i64"), as_in(arrays[1], "f64"), as_in(arrays[2], "i32")
    init_pts, init_angle = c(arrays[3], "f64"), c(arrays[4], "f64")
    M = int(tmpl_pts.shape[0])
    if tuple(offsets.shape) != (F + 1,) or tuple(tmpl_pts.shape) != (M, 2) or tuple(slot.shape) != (M,) or \
            (init_pts is not None and tuple(init_pts.shape) != (M, 2)) or (init_angle is not None and tuple(init_angle.shape) != (M,)):
        raise ValueError("offsets must be [F+1], tmpl_pts and init_pts [M,2], slot and init_angle [M]")
    pat = as_in(pattern, "f64")
    if pat.ndim != 2 or pat.shape[1] != 2:
        raise ValueError("pattern must be [P,2]")
    shapes = {"pts": ((M, 2), "f64"), "angle": ((M,), "f64"), "cov": ((M, 3), "f64"), "dist2": ((M,), "f64"),
              "status": ((M,), "i32"), "lost_level": ((M,), "i32")}
    unknown = set(outputs) - set(shapes)
    if unknown:
        raise ValueError(f"unknown outputs {sorted(unknown)}")
    out = {k: (new(*shapes[k]) if k in outputs else None) for k in shapes}
    pp, pq = _table(pv, on)
    np_, nq = _table(nx, on)
    capi.check(capi.lib().pnec_hip_patch_track_stored(
        _store_ptr(store, on), store.n_slots, pp, pq, np_, nq, L, ptype, F, h, w, p(offsets), M, p(tmpl_pts), p(slot),
        p(init_pts), p(init_angle), float(shift[0]), float(shift[1]), p(pat), int(pat.shape[0]), int(max_iterations),
        float(max_recovered_dist2), 0 if backward else TRACK_NO_BACKWARD, float(scaling), p(out["pts"]), p(out["angle"]),
        p(out["cov"]), p(out["dist2"]), p(out["status"]), p(out["lost_level"]), space, device, stream))
    return PatchTrack(out["pts"], out["angle"], out["cov"], out["dist2"], out["status"], out["lost_level"], offsets)
