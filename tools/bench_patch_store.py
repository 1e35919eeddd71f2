#!/usr/bin/env python3
"""What stored patches cost and save: F sequences of 1241 x 376 uint8 (tools/bench_tracks.py's images: smoothed noise,
frame n is frame 0 rolled by 3 n pixels), grid 30 with 4 points per cell and a capacity of 2 000 tracks per image, 5
levels, everything device-resident.  One process, the arms alternated after warm-up, each timed with device events around
`inner` back-to-back calls (tools/bench_tracks.py's method):
   indexed    pnec_hip_patch_track_indexed: frame 0 -> frame 1, every template rebuilt from the ring's stack
   stored     pnec_hip_patch_track_stored on the same rows, the templates read from the store
   add_all    pnec_hip_patch_store_add with every row new (the first frame)
   add_5pct   the same with the first 95 % of every image's rows carried
   step_ring / step_patches   one Tracker.process with ring=4 / with templates="patches", ring=2
and the store's bytes.  There is no acceptance figure: nobody had measured whether loading about 2 KB per level beats
rebuilding the template.  Prints one JSON object and, with an output path, writes it there (profiles/patch_store.json).
Runs on the GPU box.
   python tools/bench_patch_store.py [F] [repeats] [out.json]"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from pnec_amd import Tracker, capi

F = int(sys.argv[1]) if len(sys.argv) > 1 else 256
REPEATS = int(sys.argv[2]) if len(sys.argv) > 2 else 11
OUT = sys.argv[3] if len(sys.argv) > 3 else None
H, W, INNER, G, K, C, LEVELS, RING = 376, 1241, 3, 30, 4, 2000, 5, 4
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

kw = dict(levels=LEVELS, grid=G, points_per_cell=K, capacity=C)
ring = Tracker(F, H, W, ring=RING, **kw)
stor = Tracker(F, H, W, ring=2, templates="patches", **kw)
ring.process(frames[0])
stor.process(frames[0])
torch.cuda.synchronize()
N = F * C
L = capi.lib()
pat = ring._pattern
A, S = ring.tracks, stor.tracks                     # the same rows: image indices in A.tmpl_image, slots in S.tmpl_image
born = int(A.offsets[-1])
assert torch.equal(A.offsets, S.offsets) and torch.equal(A.tmpl_pts[:born], S.tmpl_pts[:born])


def _stream():
    return torch.cuda.current_stream(0).cuda_stream


slot0, slot1 = ring._slot(0), ring._slot(1)
slot1[0].copy_(frames[1])
for l in range(1, LEVELS):
    capi.check(L.pnec_hip_image_pyramid_level(slot1[l - 1].data_ptr(), slot1[l].data_ptr(), 0, F, H >> (l - 1), W >> (l - 1),
                                              W >> (l - 1), W >> l, capi.MEM_DEVICE, 0, _stream()))
p = lambda t: None if t is None else t.data_ptr()
tabs = {k: ring._tables(v) for k, v in (("stack", ring._stack), ("s0", slot0), ("s1", slot1))}
T = ring.last_track
KEYS = ("pts", "angle", "cov", "dist2", "status", "lost_level")


def track(stored):
    (tp, tq), (pp, pq), (np_, nq) = tabs["stack"], tabs["s0"], tabs["s1"]
    tail = (0.0, 0.0, p(pat), int(pat.shape[0]), 40, 0.04, 0, 10.0, p(T.pts), p(T.angle), p(T.cov), p(T.dist2), p(T.status),
            p(T.lost_level), capi.MEM_DEVICE, 0, _stream())
    if stored:
        capi.check(L.pnec_hip_patch_track_stored(p(stor.store.data), stor.store.n_slots, pp, pq, np_, nq, LEVELS, 0, F, H, W,
                                                 p(S.offsets), N, p(S.tmpl_pts), p(S.tmpl_image), p(S.pts), p(S.angle), *tail))
    else:
        capi.check(L.pnec_hip_patch_track_indexed(tp, tq, RING * F, pp, pq, np_, nq, LEVELS, 0, F, H, W, p(A.offsets), N,
                                                  p(A.tmpl_pts), p(A.tmpl_image), p(A.pts), p(A.angle), *tail))


bits = lambda t: t.view(torch.int64) if t.dtype == torch.float64 else t
track(False)
torch.cuda.synchronize()
indexed_bits = [getattr(T, k).clone() for k in KEYS]
track(True)
torch.cuda.synchronize()
same_bits = all(torch.equal(bits(x), bits(getattr(T, k))) for x, k in zip(indexed_bits, KEYS))

slots = S.tmpl_image.clone()
counts = torch.diff(S.offsets)
carried95 = torch.zeros_like(S.offsets)
carried95[1:] = torch.cumsum((counts * 95) // 100, 0)
new_5pct = int((counts - (counts * 95) // 100).sum())
cp, cq = ring._tables(slot0)


def add(carried):
    # (the rows' slots as the first frame left them: a carried row keeps its own, a new one gets the one it had)
    slots.copy_(S.tmpl_image)
    capi.check(L.pnec_hip_patch_store_add(cp, cq, LEVELS, 0, F, H, W, p(carried), p(S.offsets), N, p(S.tmpl_pts), p(slots), C,
                                          p(pat), int(pat.shape[0]), p(stor.store.data), stor.store.n_slots, capi.MEM_DEVICE, 0,
                                          _stream()))


# (trackers of their own: the arms above keep working on the sets as they stood after frame 0)
ring2 = Tracker(F, H, W, ring=RING, **kw)
stor2 = Tracker(F, H, W, ring=2, templates="patches", **kw)
ring2.process(frames[0])
stor2.process(frames[0])
state = {"ring": 1, "patches": 1}


def step(which, trk):
    trk.process(frames[state[which] % 4])
    state[which] += 1


ARMS = (("indexed", lambda: track(False)), ("stored", lambda: track(True)), ("add_all", lambda: add(None)),
        ("add_5pct", lambda: add(carried95)), ("step_ring", lambda: step("ring", ring2)),
        ("step_patches", lambda: step("patches", stor2)))


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(INNER):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / INNER


for _, fn in ARMS:
    fn()
torch.cuda.synchronize()
store_unchanged = bool(torch.equal(slots, S.tmpl_image))
ms = {k: [] for k, _ in ARMS}
for _ in range(REPEATS):
    for key, fn in ARMS:
        ms[key].append(timed(fn))
torch.cuda.synchronize()


def stat(x):
    x = np.asarray(x)
    return {"median_ms": float(np.median(x)), "min_ms": float(x.min()), "max_ms": float(x.max()),
            "spread_rel": float((x.max() - x.min()) / np.median(x))}


med = {k: float(np.median(v)) for k, v in ms.items()}
slot_bytes = int(L.pnec_hip_patch_store_slot_bytes(LEVELS))
line = {"images": F, "height": H, "width": W, "levels": LEVELS, "ring": RING, "grid": G, "points_per_cell": K,
        "capacity_per_image": C, "rows": N, "tracks_born_in_frame_0": born, "new_rows_in_add_5pct": new_5pct,
        "repeats": REPEATS, "calls_per_timing": INNER, "timing": "device events around back-to-back calls, arms alternated",
        **{k: stat(v) for k, v in ms.items()},
        "stored_minus_indexed_ms": med["stored"] - med["indexed"],
        "stored_minus_indexed_range_ms": [min(ms["stored"]) - max(ms["indexed"]), max(ms["stored"]) - min(ms["indexed"])],
        "stored_over_indexed": med["stored"] / med["indexed"],
        "step_patches_over_step_ring": med["step_patches"] / med["step_ring"],
        "stored_has_indexed_bits": bool(same_bits), "add_reassigns_the_same_slots": store_unchanged,
        "slot_bytes": slot_bytes, "store_bytes": slot_bytes * N,
        "ring_stack_bytes": int(sum(lv.numel() * lv.element_size() for lv in ring._stack)),
        "patches_stack_bytes": int(sum(lv.numel() * lv.element_size() for lv in stor._stack)),
        "store_bytes_read_per_stored_call": born * slot_bytes * 2,
        "lib_sha256": hashlib.sha256(open(capi.LIB_PATH, "rb").read()).hexdigest()}
print(json.dumps(line), flush=True)
if OUT:
    with open(OUT, "w") as f:
        json.dump(line, f, indent=1)
        f.write("\n")
