#!/usr/bin/env python3
"""What carrying tracks across frames costs: F sequences of 1241 x 376 uint8 (smoothed noise; frame n is frame 0 rolled by
3 n pixels), grid 30 with 4 points per cell and a capacity of 2 000 tracks per image (the patch tracker's workload of
DESIGN 9f), 5 levels, a ring of 3, everything device-resident.  One process, the arms alternated after warm-up, each timed
with device events around `inner` back-to-back calls:
   retain    pnec_hip_tracks_retain on the tracker's set and its last tracking result
   append    pnec_hip_tracks_append of the retained set and the detections
   plain     pnec_hip_patch_track, all templates in the previous frame
   indexed   pnec_hip_patch_track_indexed on identical inputs (tmpl = the ring's stack, tmpl_image = the previous slot)
   pyramid / detect / cov   the other three stages of a step, as Tracker.process calls them
   step      one Tracker.process
   torch     the same step with torch boolean indexing between the plain calls (its read-backs included; timed on the
             host clock around a device-wide wait, since it waits for the stream by itself)
There is no acceptance figure: nobody had measured any of it.  Prints one JSON object and, with an output path, writes it
there (profiles/tracks.json).  Runs on the GPU box.
   python tools/bench_tracks.py [F] [repeats] [out.json]"""
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from pnec_amd import (Tracker, append_tracks, capi, detect_keypoints, image_pyramid, patch_covariance, patch_track,
                      retain_tracks)
from pnec_amd.tracker import new_track_set

F = int(sys.argv[1]) if len(sys.argv) > 1 else 256
REPEATS = int(sys.argv[2]) if len(sys.argv) > 2 else 11
OUT = sys.argv[3] if len(sys.argv) > 3 else None
H, W, INNER, G, K, C, LEVELS, RING = 376, 1241, 3, 30, 4, 2000, 5, 3
dev = torch.device("cuda:0")

gen = torch.Generator(device=dev)
gen.manual_seed(13)
a = torch.rand((F, H + 6, W + 6), device=dev, generator=gen)
for _ in range(3):
    a = 0.25 * a[:, :-2] + 0.5 * a[:, 1:-1] + 0.25 * a[:, 2:]
    a = 0.25 * a[:, :, :-2] + 0.5 * a[:, :, 1:-1] + 0.25 * a[:, :, 2:]
lo, hi = a.amin(dim=(1, 2), keepdim=True), a.amax(dim=(1, 2), keepdim=True)
img0 = (24.0 + 206.0 * (a - lo) / (hi - lo)).round().to(torch.uint8).contiguous()
del a, lo, hi
frames = [torch.roll(img0, shifts=3 * n, dims=2).contiguous() for n in range(4)]

trk = Tracker(F, H, W, levels=LEVELS, ring=RING, grid=G, points_per_cell=K, capacity=C)
trk.process(frames[0])
torch.cuda.synchronize()
born = int(trk.tracks.offsets[-1])
N = F * C
L = capi.lib()
pat = trk._pattern


def _stream():
    return torch.cuda.current_stream(0).cuda_stream


# the state after frame 0: every track was born in slot 0, so the plain call (tmpl = slot 0) sees identical inputs
A = trk.tracks
slot0, slot1 = trk._slot(0), trk._slot(1)
slot1[0].copy_(frames[1])
for l in range(1, LEVELS):
    capi.check(L.pnec_hip_image_pyramid_level(slot1[l - 1].data_ptr(), slot1[l].data_ptr(), 0, F, H >> (l - 1), W >> (l - 1),
                                              W >> (l - 1), W >> l, capi.MEM_DEVICE, 0, _stream()))
T = trk.last_track
p = lambda t: None if t is None else t.data_ptr()
tabs = {k: trk._tables(v) for k, v in (("stack", trk._stack), ("s0", slot0), ("s1", slot1))}


def track(indexed):
    (tp, tq), (pp, pq), (np_, nq) = tabs["stack" if indexed else "s0"], tabs["s0"], tabs["s1"]
    tail = (0.0, 0.0, p(pat), int(pat.shape[0]), 40, 0.04, 0, 10.0, p(T.pts), p(T.angle), p(T.cov), p(T.dist2), p(T.status),
            p(T.lost_level), capi.MEM_DEVICE, 0, _stream())
    if indexed:
        capi.check(L.pnec_hip_patch_track_indexed(tp, tq, RING * F, pp, pq, np_, nq, LEVELS, 0, F, H, W, p(A.offsets), N,
                                                  p(A.tmpl_pts), p(A.tmpl_image), p(A.pts), p(A.angle), *tail))
    else:
        capi.check(L.pnec_hip_patch_track(tp, tq, pp, pq, np_, nq, LEVELS, 0, F, H, W, p(A.offsets), N, p(A.tmpl_pts), p(A.pts),
                                          p(A.angle), *tail))


track(False)
torch.cuda.synchronize()
plain_bits = [getattr(T, k).clone() for k in ("pts", "angle", "cov", "status")]
track(True)
torch.cuda.synchronize()
same_bits = all(torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a,
                            b.view(torch.int64) if b.dtype == torch.float64 else b)
                for a, b in zip(plain_bits, [getattr(T, k) for k in ("pts", "angle", "cov", "status")]))
B = new_track_set(F, N, True, dev, retained=True)
T.offsets = A.offsets
retain_tracks(A, T, RING - 2, out=B)
det = detect_keypoints(slot1[0], G, K, 5, 19, current=(B.offsets, B.pts), capacity=True, out=trk._det)
det_cov = trk._det_cov
nxt = new_track_set(F, N, True, dev)
nid, dropped = trk.next_id.clone(), torch.zeros(F, dtype=torch.int64, device=dev)
torch.cuda.synchronize()
kept = int(B.offsets[-1])
found = int(det.offsets[-1])


def run_pyramid():
    for l in range(1, LEVELS):
        capi.check(L.pnec_hip_image_pyramid_level(slot1[l - 1].data_ptr(), slot1[l].data_ptr(), 0, F, H >> (l - 1), W >> (l - 1),
                                                  W >> (l - 1), W >> l, capi.MEM_DEVICE, 0, _stream()))


def run_cov():
    capi.check(L.pnec_hip_patch_covariance(slot1[0].data_ptr(), 0, F, H, W, W, p(det.offsets), int(det.pts.shape[0]), p(det.pts),
                                           p(pat), int(pat.shape[0]), 10.0, None, p(det_cov), None, None, None, None,
                                           capi.MEM_DEVICE, 0, _stream()))


# (a tracker of its own: the arms above keep working on the first one's set as it stood after frame 0)
trk2 = Tracker(F, H, W, levels=LEVELS, ring=RING, grid=G, points_per_cell=K, capacity=C)
trk2.process(frames[0])
state = {"n": 1}


def run_step():
    trk2.process(frames[state["n"] % 4])
    state["n"] += 1


def run_torch():
    """the step between two plain calls done with torch: boolean indexing, a bincount for the offsets, a stable sort to
    interleave the refill per image"""
    prev_pyr, cur_pyr = image_pyramid(frames[0], LEVELS), image_pyramid(frames[1], LEVELS)
    n = int(A.offsets[-1])                                                   # read-back
    tr = patch_track(prev_pyr, cur_pyr, A.tmpl_pts[:n], A.offsets, init_pts=A.pts[:n], init_angle=A.angle[:n], pattern=pat)
    image = torch.searchsorted(A.offsets[1:].contiguous(), torch.arange(n, device=dev), right=True)
    ok = tr.status == 0
    keep_img = image[ok]                                                     # (a size read back inside)
    offs = torch.zeros(F + 1, dtype=torch.int64, device=dev)
    offs[1:] = torch.cumsum(torch.bincount(keep_img, minlength=F), 0)
    pts = tr.pts[ok].contiguous()
    kp = detect_keypoints(cur_pyr[0], G, K, 5, 19, current=(offs, pts))     # read-back: the trimmed form
    cov = patch_covariance(cur_pyr[0], kp.pts, kp.offsets, pattern=pat, outputs=("cov",)).cov
    d_img = torch.searchsorted(kp.offsets[1:].contiguous(), torch.arange(kp.pts.shape[0], device=dev), right=True)
    order = torch.argsort(torch.cat([keep_img, d_img]), stable=True)
    out = (torch.cat([pts, kp.pts])[order], torch.cat([tr.cov[ok], cov])[order], torch.cat([A.id[:n][ok], torch.arange(
        kp.pts.shape[0], device=dev)])[order])
    return out


ARMS = (("retain", lambda: retain_tracks(A, T, RING - 2, out=B)),
        ("append", lambda: append_tracks(B, det, det_cov, F, C, nid, rows=N, out=nxt, dropped=dropped)),
        ("plain", lambda: track(False)), ("indexed", lambda: track(True)), ("pyramid", run_pyramid),
        ("detect", lambda: detect_keypoints(slot1[0], G, K, 5, 19, current=(B.offsets, B.pts), capacity=True, out=trk._det)),
        ("cov", run_cov), ("step", run_step))


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(INNER):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / INNER


def timed_host(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(INNER):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / INNER


for _, fn in ARMS:
    fn()
run_torch()
torch.cuda.synchronize()
ms = {k: [] for k, _ in ARMS}
ms["torch"], ms["step_host_clock"] = [], []
for _ in range(REPEATS):
    for key, fn in ARMS:
        ms[key].append(timed(fn))
    ms["torch"].append(timed_host(run_torch))
    ms["step_host_clock"].append(timed_host(run_step))


def stat(x):
    x = np.asarray(x)
    return {"median_ms": float(np.median(x)), "min_ms": float(x.min()), "max_ms": float(x.max()),
            "spread_rel": float((x.max() - x.min()) / np.median(x))}


med = {k: float(np.median(v)) for k, v in ms.items()}
# a retained row: read id, tmpl_image, tmpl_pts, age, pts, cov, trk_pts, trk_angle, trk_cov, status (124 B; id, age and
# status once more by the count: 16 B), written id .. cov, prev_pts, prev_cov, src (128 B); an appended row: 80 B in, 80 B out
retain_bytes = 124 + 16 + 128
append_bytes = 2 * (8 + 4 + 16 + 4 + 16 + 8 + 24)
stages = ("pyramid", "indexed", "retain", "detect", "cov", "append")
line = {"images": F, "height": H, "width": W, "levels": LEVELS, "ring": RING, "grid": G, "points_per_cell": K,
        "capacity_per_image": C, "rows": N, "tracks_born_in_frame_0": born, "retained_after_frame_1": kept,
        "detections_in_frame_1": found, "repeats": REPEATS, "calls_per_timing": INNER,
        "timing": "device events around back-to-back calls, arms alternated; torch and step_host_clock on the host clock",
        **{k: stat(v) for k, v in ms.items()},
        "indexed_minus_plain_ms": med["indexed"] - med["plain"],
        "indexed_minus_plain_range_ms": [min(ms["indexed"]) - max(ms["plain"]), max(ms["indexed"]) - min(ms["plain"])],
        "indexed_has_plain_bits": bool(same_bits),
        "retain_bytes_per_row": retain_bytes, "append_bytes_per_row": append_bytes,
        "retain_rows_per_s": N / (med["retain"] * 1e-3), "retain_bytes_per_s": N * retain_bytes / (med["retain"] * 1e-3),
        "append_rows_per_s": N / (med["append"] * 1e-3), "append_bytes_per_s": N * append_bytes / (med["append"] * 1e-3),
        "stage_share_of_their_sum": {k: med[k] / sum(med[s] for s in stages) for k in stages},
        "sum_of_stages_ms": sum(med[s] for s in stages),
        "torch_over_step": med["torch"] / med["step_host_clock"],
        "lib_sha256": hashlib.sha256(open(capi.LIB_PATH, "rb").read()).hexdigest()}
print(json.dumps(line), flush=True)
if OUT:
    with open(OUT, "w") as f:
        json.dump(line, f, indent=1)
        f.write("\n")
