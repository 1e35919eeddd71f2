#!/usr/bin/env python3
"""What the keyframe rule costs: 256 sequences x capacity 2 000 of 1241 x 376 uint8 (smoothed noise; frame n is frame 0
rolled by 3 n pixels; grid 30, 4 points per cell, 5 levels, a ring of 4; min_displacement 5, max_span 2), one process:
   the call alone   pnec_hip_tracks_keyframe against pnec_hip_tracks_retain on the rows of the same tracker step, device
                    events around `inner` back-to-back calls, the two arms alternated
   the step         one Odometry.process step with keyframes on (min_displacement = 5) against off (0), alternated after
                    warm-up; device events, and the host clock until the last call returned
Median with min - max over the repeats.  There is no acceptance figure: nobody had measured any of it.  The two Odometry
arms do NOT solve the same pairs -- with keyframes on a skipped sequence hands the chain an empty pair -- so their
difference is the rule's cost minus the solves it saves on this workload, not the cost of the call.
Prints one JSON object and, with an output path, writes it there (profiles/keyframes.json).  Runs on the GPU box.
   python tools/bench_keyframes.py [repeats] [out.json] [sequences]"""
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from pnec_amd import KeyframeTracker, Odometry, capi, keyframe_pairs, retain_tracks
from pnec_amd.keyframes import new_keyframe_pairs, new_keyframe_state
from pnec_amd.tracker import new_track_set

REPEATS = int(sys.argv[1]) if len(sys.argv) > 1 else 11
OUT = sys.argv[2] if len(sys.argv) > 2 and sys.argv[2] != "-" else None
F = int(sys.argv[3]) if len(sys.argv) > 3 else 256
H, W, INNER, G, K, LEVELS, RING, C = 376, 1241, 3, 30, 4, 5, 4, 2000
MIN_DISPLACEMENT, MAX_SPAN = 5.0, 2
dev = torch.device("cuda:0")
K_INV = np.linalg.inv(np.array([[718.856, 0.0, 607.1928], [0.0, 718.856, 185.2157], [0.0, 0.0, 1.0]]))
TRACKER = dict(levels=LEVELS, ring=RING, grid=G, points_per_cell=K, capacity=C)


def make_frames():
    gen = torch.Generator(device=dev)
    gen.manual_seed(13)
    a = torch.rand((F, H + 6, W + 6), device=dev, generator=gen)
    for _ in range(3):
        a = 0.25 * a[:, :-2] + 0.5 * a[:, 1:-1] + 0.25 * a[:, 2:]
        a = 0.25 * a[:, :, :-2] + 0.5 * a[:, :, 1:-1] + 0.25 * a[:, :, 2:]
    lo, hi = a.amin(dim=(1, 2), keepdim=True), a.amax(dim=(1, 2), keepdim=True)
    img0 = (24.0 + 206.0 * (a - lo) / (hi - lo)).round().to(torch.uint8).contiguous()
    return [torch.roll(img0, shifts=3 * n, dims=2).contiguous() for n in range(4)]


def stat(x):
    x = np.asarray(x)
    return {"median_ms": float(np.median(x)), "min_ms": float(x.min()), "max_ms": float(x.max()),
            "spread_rel": float((x.max() - x.min()) / np.median(x))}


def difference(d, a, b):
    return {"median_of_medians": float(np.median(d[a]) - np.median(d[b])), "range": [min(d[a]) - max(d[b]), max(d[a]) - min(d[b])]}


frames = make_frames()

# ---- the call alone, on the rows of a tracker step
kft = KeyframeTracker(F, H, W, MIN_DISPLACEMENT, MAX_SPAN, **TRACKER)
for n in range(3):
    kft.process(frames[n])
trk = kft.tracker
before, retained, appended = trk._sets[1 - trk._cur], trk._retained, trk.tracks
old_state = kft._states[1 - kft._cur]
N = trk._N
out_k = (new_keyframe_pairs(F, N, True, dev), new_keyframe_state(F, N, True, dev))
out_r = new_track_set(F, N, True, dev, retained=True)
calls = {"tracks_keyframe": lambda: keyframe_pairs(retained, appended, old_state, MIN_DISPLACEMENT, MAX_SPAN, out=out_k),
         "tracks_retain": lambda: retain_tracks(before, trk.last_track, max_age=RING - 2, out=out_r)}
for fn in calls.values():
    fn()
torch.cuda.synchronize()
call_ms = {k: [] for k in calls}
for _ in range(REPEATS):
    for k, fn in calls.items():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(INNER):
            fn()
        b.record()
        b.synchronize()
        call_ms[k].append(a.elapsed_time(b) / INNER)
rows = {"retained_rows": int(retained.offsets[-1]), "pair_rows": int(out_k[0].offsets[-1]),
        "accepted_sequences": int(out_k[0].accepted.sum()), "set_rows": int(appended.offsets[-1])}
del kft, trk, before, retained, appended, old_state, out_k, out_r, calls
torch.cuda.empty_cache()

# ---- one Odometry step, keyframes on against off
arms = {"keyframes_on": Odometry(F, H, W, K_INV, min_displacement=MIN_DISPLACEMENT, max_span=MAX_SPAN, **TRACKER),
        "keyframes_off": Odometry(F, H, W, K_INV, **TRACKER)}
count = {k: 0 for k in arms}
accepted = []


def step(k):
    r = arms[k].process(frames[count[k] % 4])
    count[k] += 1
    return r


for k in arms:                                                # warm-up: first frame, allocations, table uploads
    for _ in range(5):
        step(k)
torch.cuda.synchronize()
ev, ret = ({k: [] for k in arms} for _ in range(2))
for _ in range(REPEATS):
    for k in arms:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        for _ in range(INNER):
            r = step(k)
            if k == "keyframes_on":
                accepted.append(r.accepted)
        b.record()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        ev[k].append(a.elapsed_time(b) / INNER)
        ret[k].append((t1 - t0) * 1e3 / INNER)
share = float(torch.stack(accepted).to(torch.float64).mean())
for a in arms.values():
    a.close()

line = {"height": H, "width": W, "sequences": F, "capacity_per_image": C, "rows": F * C, "levels": LEVELS, "ring": RING, "grid": G,
        "points_per_cell": K, "min_displacement": MIN_DISPLACEMENT, "max_span": MAX_SPAN, "repeats": REPEATS,
        "steps_per_timing": INNER,
        "timing": "arms alternated after warm-up; device events, and the host clock until the last call returned; median "
                  "(min - max) over the repeats",
        "call_alone_rows": rows,
        "call_alone_device_events": {k: stat(v) for k, v in call_ms.items()},
        "keyframe_minus_retain_ms": difference(call_ms, "tracks_keyframe", "tracks_retain"),
        "step_device_events": {k: stat(v) for k, v in ev.items()},
        "step_host_clock_until_returned": {k: stat(v) for k, v in ret.items()},
        "step_on_minus_off_device_ms": difference(ev, "keyframes_on", "keyframes_off"),
        "accepted_share_of_the_timed_steps": share,
        "lib_sha256": hashlib.sha256(open(capi.LIB_PATH, "rb").read()).hexdigest()}
print(json.dumps(line), flush=True)
if OUT:
    with open(OUT, "w") as f:
        json.dump(line, f, indent=1)
        f.write("\n")
