"""Keyframe pairs: the reference's "did the frame move enough" rule (FrameProcessing::ProcessFrame,
frame_processing.cc:87-93; TrackingMatcher::FindMatches, tracking_matcher.cc:68-85) on the device --
``keyframe_pairs`` (``pnec_hip_tracks_keyframe``) -- and ``KeyframeTracker``, a ``Tracker`` with the per-track state of
that rule carried from frame to frame.  include/pnec_hip.h has the definition.

A sequence's KEY FRAME is its last accepted frame.  A frame whose tracks moved, on average, less than `min_displacement`
pixels against the key frame is skipped: it gives no pair, and the next frame is matched against the same key frame.

DEVIATION from the reference, which keeps a track's patch for ever and so matches against a key frame of any age:
``Tracker`` retires a track at age ring - 2, so a pair spanning more frames has no match.  `max_span` (default and at
most ring - 2) forces acceptance when the pair would span that many frames; a pair that spans s frames also lacks the
tracks born before the key frame that aged out on the way.  ``KeyframeTracker(..., templates="patches")`` (stored
patches) lifts it: a track lives as long as it is tracked, any max_span >= 1 is taken, and None forces no acceptance.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import capi
from .patches import _is_torch
from .tracker import Tracker, TrackSet, _kit, _where


@dataclass
class KeyframePairs:
    """The pairs (key frame, this frame) of one step, ragged over F images: rows [offsets[f], offsets[f+1]) are image f's
    matches -- none for a skipped image --, rows at and beyond offsets[F] are padding (NaN, row -1).  The arrays have the
    rows of the retained set.  numpy or torch, matching the input."""
    offsets: object            # int64 [F+1]
    key_pts: object            # [N,2] the track in the key frame
    pts: object                # [N,2] the track in this frame
    cov: object                # [N,3] its covariance in this frame, or None
    key_cov: object            # [N,3] its covariance in the key frame, or None
    row: object                # int64 [N] the row of the retained set
    accepted: object           # uint8 [F]
    mean_displacement: object  # [F] NaN without a match
    n_matches: object          # int32 [F] matches against the key frame, accepted or not


@dataclass
class KeyframeState:
    """Where each row of the current track set was seen in its sequence's key frame (NaN: born after it), and how many
    frames lie between the key frame and the frame of the set."""
    key_pts: object   # [N,2]
    key_cov: object   # [N,3] or None
    span: object      # int32 [F]


def _new(shape, kind, on, dev):
    if on:
        import torch
        dt = {"f64": torch.float64, "i64": torch.int64, "i32": torch.int32, "u8": torch.uint8}
        return torch.empty(shape, dtype=dt[kind], device=dev)
    return np.empty(shape, dtype={"f64": np.float64, "i64": np.int64, "i32": np.int32, "u8": np.uint8}[kind])


def new_keyframe_pairs(n_images: int, rows: int, on_device: bool, device=None, cov: bool = True) -> KeyframePairs:
    """Uninitialised arrays of the pairs of a retained set of `rows` rows."""
    n = lambda shape, kind: _new(shape, kind, on_device, device)
    F, N = int(n_images), int(rows)
    return KeyframePairs(n((F + 1,), "i64"), n((N, 2), "f64"), n((N, 2), "f64"), n((N, 3), "f64") if cov else None,
                         n((N, 3), "f64") if cov else None, n((N,), "i64"), n((F,), "u8"), n((F,), "f64"), n((F,), "i32"))


def new_keyframe_state(n_images: int, rows: int, on_device: bool, device=None, cov: bool = True) -> KeyframeState:
    """Uninitialised arrays of the state of a track set of `rows` rows."""
    n = lambda shape, kind: _new(shape, kind, on_device, device)
    return KeyframeState(n((int(rows), 2), "f64"), n((int(rows), 3), "f64") if cov else None, n((int(n_images),), "i32"))


def keyframe_pairs(retained, appended: TrackSet, state, min_displacement: float, max_span: int, out=None):
    """One step of the keyframe rule.  `retained`: the retained set of the step (retain_tracks' result, with `src`), or
    None on the first frame; `appended`: the set append_tracks made from it; `state`: the KeyframeState that goes with the
    set `retained` was retained from (None on the first frame).  Returns (KeyframePairs, the next KeyframeState -- the one
    that goes with `appended`).  An image is accepted when the mean displacement of its matches is not below
    `min_displacement`, or when state.span + 1 >= max_span; pnec_hip_tracks_keyframe in include/pnec_hip.h is the
    definition.  The pairs are in the form Batch.fill_keypoints_ragged(offsets, key_pts, pts, cov) takes.  torch.cuda in ->
    torch.cuda out, asynchronous on torch's current stream, nothing read back; numpy in -> staged, numpy out.
    `out`: a (KeyframePairs, KeyframeState) of the same shapes to write in place of new arrays; the state must not be
    `state` itself."""
    ref = appended.pts
    on = _is_torch(ref) and ref.is_cuda
    space, device, stream, dev = _where(ref, on)
    _, as_in, p = _kit(on, dev)
    c = lambda a, kind: None if a is None else as_in(a, kind)
    a_off, a_pts, a_cov = as_in(appended.offsets, "i64"), as_in(appended.pts, "f64"), c(appended.cov, "f64")
    F, A = int(a_off.shape[0]) - 1, int(a_pts.shape[0])
    with_cov = a_cov is not None
    if retained is None:
        b_off = b_pts = b_cov = b_src = k_pts = k_cov = k_span = None
        N = S = 0
    else:
        if retained.src is None or state is None:
            raise ValueError("a retained set needs its `src` and the state of the set it was retained from")
        b_off, b_pts, b_src = as_in(retained.offsets, "i64"), as_in(retained.pts, "f64"), as_in(retained.src, "i64")
        b_cov = c(retained.cov, "f64") if with_cov else None
        k_pts, k_span = as_in(state.key_pts, "f64"), as_in(state.span, "i32")
        k_cov = c(state.key_cov, "f64") if with_cov else None
        N, S = int(b_pts.shape[0]), int(k_pts.shape[0])
        if int(b_off.shape[0]) != F + 1 or tuple(k_span.shape) != (F,):
            raise ValueError("the retained set, the refilled set and the state must cover the same images")
        if with_cov and (b_cov is None or k_cov is None):
            raise ValueError("covariances must be given for the retained set, the refilled set and the state, or for none")
    if out is None:
        pairs = new_keyframe_pairs(F, N, on, dev, cov=with_cov)
        nxt = new_keyframe_state(F, A, on, dev, cov=with_cov)
    else:
        pairs, nxt = out
        if int(pairs.key_pts.shape[0]) < N or int(pairs.offsets.shape[0]) != F + 1 or int(nxt.key_pts.shape[0]) != A or \
                tuple(nxt.span.shape) != (F,) or (retained is not None and int(pairs.key_pts.shape[0]) != N) or \
                (with_cov and (nxt.key_cov is None or pairs.cov is None or pairs.key_cov is None)):
            raise ValueError("`out` must be a (KeyframePairs, KeyframeState) of the call's shapes")
    capi.check(capi.lib().pnec_hip_tracks_keyframe(
        F, p(b_off), N, p(b_pts), p(b_cov), p(b_src), p(a_off), A, p(a_pts), p(a_cov), S, p(k_pts), p(k_cov), p(k_span),
        float(min_displacement), int(max_span), p(pairs.offsets), p(pairs.key_pts), p(pairs.pts),
        p(pairs.cov) if with_cov else None, p(pairs.key_cov) if with_cov else None, p(pairs.row), p(pairs.accepted),
        p(pairs.mean_displacement), p(pairs.n_matches), p(nxt.key_pts), p(nxt.key_cov) if with_cov else None, p(nxt.span),
        space, device, stream))
    return pairs, nxt


class KeyframeTracker:
    """A ``Tracker`` whose pairs are (key frame, this frame) instead of (previous frame, this frame).

    ``process(images)`` runs ``Tracker.process`` and then ``keyframe_pairs`` on the tracker's retained set and
    ``tracker.tracks``; it returns None for the first frame (which sets the state), then a KeyframePairs per frame --
    empty (accepted 0) for a sequence whose frame was skipped.  ``state`` is the KeyframeState that goes with
    ``tracker.tracks``.  The tracker, the pairs and the two state buffers are allocated here, in the constructor; no call
    of process reads anything back or waits.  The pairs are this object's own buffer: the next call overwrites it.

    It needs ring >= 4 (default 4), and max_span must lie in 1 .. ring - 2 (default ring - 2): a track is retired at age
    ring - 2, so a pair spanning more frames has no match -- see the module's DEVIATION.  With templates="patches" among
    the tracker's keywords there is no such limit: ring >= 2, any max_span >= 1, and max_span None means that no
    acceptance is forced (the call gets 2**31 - 1)."""

    def __init__(self, n_sequences: int, height: int, width: int, min_displacement: float = 5.0, max_span: int = None,
                 **tracker_kwargs):
        ring = int(tracker_kwargs.get("ring", 4))
        if tracker_kwargs.get("templates", "ring") == "patches":
            max_span = 2 ** 31 - 1 if max_span is None else int(max_span)
            if not 1 <= max_span <= 2 ** 31 - 1:
                raise ValueError("max_span must be >= 1 (and fit int32)")
        else:
            if ring < 4:
                raise ValueError("KeyframeTracker needs ring >= 4 (a pair must be able to span two frames)")
            max_span = ring - 2 if max_span is None else int(max_span)
            if not 1 <= max_span <= ring - 2:
                raise ValueError("max_span must lie in 1 .. ring - 2 (a track is retired at age ring - 2)")
        min_displacement = float(min_displacement)
        if not (min_displacement >= 0.0 and np.isfinite(min_displacement)):
            raise ValueError("min_displacement must be finite and >= 0")
        self.min_displacement, self.max_span = min_displacement, max_span
        self.tracker = Tracker(n_sequences, height, width, **tracker_kwargs)
        F, N, dev = self.tracker.n_sequences, self.tracker._N, self.tracker.device
        self._pairs = new_keyframe_pairs(F, N, True, dev)
        self._states = [new_keyframe_state(F, N, True, dev), new_keyframe_state(F, N, True, dev)]
        self._cur = 0
        self.state = None

    def process(self, images):
        retained = self.tracker.process(images)
        nxt = self._states[1 - self._cur]
        pairs, self.state = keyframe_pairs(retained, self.tracker.tracks, self.state, self.min_displacement, self.max_span,
                                           out=(self._pairs, nxt))
        self._cur = 1 - self._cur
        return None if retained is None else pairs
