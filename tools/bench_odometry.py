#!/usr/bin/env python3
"""What the device-side hand-over from the tracker to the solver is worth: one Odometry.process step (Tracker ->
fill_keypoints_ragged on the device's offsets -> solve_pipeline) against the same step with the read-back form of
INTEGRATION 3j (the offsets fetched with .cpu(), which waits for the whole tracker step; then a batch shaped on the
host), at two sizes of 1241 x 376 uint8 sequences (smoothed noise; frame n is frame 0 rolled by 3 n pixels; grid 30, 4
points per cell, 5 levels, a ring of 3):
   large   256 sequences, capacity 2 000 per image  (the tracker benchmark's workload, tools/bench_tracks.py)
   small   8 sequences, capacity 500                (the wait is not hidden behind a long tracker step)
One process; per size the arms are alternated after warm-up:
   device      Odometry.process
   readback    Tracker.process, offsets.cpu(), Batch(mode, offsets), fill_keypoints, solve_pipeline   (3j as it was printed)
   reshape     the same with ONE capacity batch re-shaped from the fetched offsets                    (3j without the allocation)
each timed three ways over `inner` back-to-back steps: device events (what the GPU spends), the host clock around the
steps and a final wait (what a caller with nothing else to do sees), and the host clock until the last call has RETURNED
(what a caller with other work sees: the read-back arms cannot return before the tracker step has run).
The new call alone, against pnec_hip_problem_fill_keypoints on the same rows (an exact batch of the fetched offsets):
device events around `inner` back-to-back calls.
There is no acceptance figure: nobody had measured any of it.  Prints one JSON object and, with an output path, writes it
there (profiles/odometry.json).  Runs on the GPU box.
   python tools/bench_odometry.py [repeats] [out.json] [large_F]"""
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from pnec_amd import Batch, Odometry, Tracker, capi
from pnec_amd.odometry import start_rotation

REPEATS = int(sys.argv[1]) if len(sys.argv) > 1 else 11
OUT = sys.argv[2] if len(sys.argv) > 2 and sys.argv[2] != "-" else None
LARGE_F = int(sys.argv[3]) if len(sys.argv) > 3 else 256
H, W, INNER, G, K, LEVELS, RING = 376, 1241, 3, 30, 4, 5, 3
dev = torch.device("cuda:0")
K_INV = np.linalg.inv(np.array([[718.856, 0.0, 607.1928], [0.0, 718.856, 185.2157], [0.0, 0.0, 1.0]]))
MODE = capi.MODE_TARGET


def make_frames(F):
    gen = torch.Generator(device=dev)
    gen.manual_seed(13)
    a = torch.rand((F, H + 6, W + 6), device=dev, generator=gen)
    for _ in range(3):
        a = 0.25 * a[:, :-2] + 0.5 * a[:, 1:-1] + 0.25 * a[:, 2:]
        a = 0.25 * a[:, :, :-2] + 0.5 * a[:, :, 1:-1] + 0.25 * a[:, :, 2:]
    lo, hi = a.amin(dim=(1, 2), keepdim=True), a.amax(dim=(1, 2), keepdim=True)
    img0 = (24.0 + 206.0 * (a - lo) / (hi - lo)).round().to(torch.uint8).contiguous()
    return [torch.roll(img0, shifts=3 * n, dims=2).contiguous() for n in range(4)]


class ReadBack:
    """the step of INTEGRATION 3j: the host fetches the offsets (and waits for the tracker step) to shape the batch"""

    def __init__(self, F, C, reshape):
        self.trk = Tracker(F, H, W, levels=LEVELS, ring=RING, grid=G, points_per_cell=K, capacity=C)
        self.cap = Batch.with_capacity(MODE, F, F * C) if reshape else None
        self.identity = torch.zeros((F, 4), dtype=torch.float64, device=dev)
        self.identity[:, 3] = 1.0
        self.zero_t = torch.zeros((F, 3), dtype=torch.float64, device=dev)
        self.prev_q = None
        self.last = None

    def process(self, images):
        pairs = self.trk.process(images)
        if pairs is None:
            return None
        off = pairs.offsets.cpu().numpy()                     # <- waits for the whole tracker step
        m = int(off[-1])
        if self.cap is not None:
            batch = self.cap.reshape(off)
        else:
            if self.last is not None:
                self.last.close()
            batch = self.last = Batch(MODE, off)
        batch.fill_keypoints(pairs.prev_pts[:m], pairs.pts[:m], pairs.cov[:m], K_inv=K_INV)
        q, t = batch.solve_pipeline(start_rotation(self.prev_q, self.identity), self.zero_t)
        self.prev_q = q
        return q, t


def stat(x):
    x = np.asarray(x)
    return {"median_ms": float(np.median(x)), "min_ms": float(x.min()), "max_ms": float(x.max()),
            "spread_rel": float((x.max() - x.min()) / np.median(x))}


def measure(F, C):
    frames = make_frames(F)
    arms = {"device": Odometry(F, H, W, K_INV, mode=MODE, levels=LEVELS, ring=RING, grid=G, points_per_cell=K, capacity=C),
            "readback": ReadBack(F, C, False), "reshape": ReadBack(F, C, True)}
    count = {k: 0 for k in arms}

    def step(k):
        r = arms[k].process(frames[count[k] % 4])
        count[k] += 1
        return r

    for k in arms:                                            # warm-up: first frame, allocations, table uploads
        for _ in range(5):
            step(k)
    torch.cuda.synchronize()
    ev, host, ret = ({k: [] for k in arms} for _ in range(3))
    for _ in range(REPEATS):
        for k in arms:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            a.record()
            for _ in range(INNER):
                step(k)
            b.record()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            ev[k].append(a.elapsed_time(b) / INNER)
            ret[k].append((t1 - t0) * 1e3 / INNER)
            host[k].append((t2 - t0) * 1e3 / INNER)
    # the poses of the three arms after the same number of steps from the same frames: the same bits
    torch.cuda.synchronize()
    assert len(set(count.values())) == 1
    q_dev = arms["device"]._prev_q
    same = all(torch.equal(q_dev.view(torch.int64), arms[k].prev_q.view(torch.int64)) for k in ("readback", "reshape"))

    # ---- the call alone, on the rows of a tracker step
    trk = Tracker(F, H, W, levels=LEVELS, ring=RING, grid=G, points_per_cell=K, capacity=C)
    trk.process(frames[0])
    pairs = trk.process(frames[1])
    off_d = pairs.offsets.clone()
    p1, p2, cv = pairs.prev_pts.clone(), pairs.pts.clone(), pairs.cov.clone()
    torch.cuda.synchronize()
    off_h = off_d.cpu().numpy()
    m = int(off_h[-1])
    ragged = Batch.with_capacity(MODE, F, F * C).reshape(np.arange(F + 1, dtype=np.int64) * C)
    exact = Batch(MODE, off_h)
    Kd = torch.as_tensor(K_INV, device=dev)
    fills = {"fill_keypoints_ragged": lambda: ragged.fill_keypoints_ragged(off_d, p1, p2, cv, K_inv=Kd),
             "fill_keypoints": lambda: exact.fill_keypoints(p1[:m], p2[:m], cv[:m], K_inv=Kd)}
    for fn in fills.values():
        fn()
    torch.cuda.synchronize()
    fill_ms = {k: [] for k in fills}
    for _ in range(REPEATS):
        for k, fn in fills.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(INNER):
                fn()
            b.record()
            b.synchronize()
            fill_ms[k].append(a.elapsed_time(b) / INNER)
    med = lambda d, k: float(np.median(d[k]))
    out = {"sequences": F, "capacity_per_image": C, "rows": F * C, "correspondences_of_the_timed_fill": m,
           "three_arms_same_pose_bits": bool(same),
           "device_events": {k: stat(v) for k, v in ev.items()},
           "host_clock_with_final_wait": {k: stat(v) for k, v in host.items()},
           "host_clock_until_returned": {k: stat(v) for k, v in ret.items()},
           "fill_alone_device_events": {k: stat(v) for k, v in fill_ms.items()}}
    for other in ("readback", "reshape"):
        out[f"{other}_minus_device_host_ms"] = {"median_of_medians": med(host, other) - med(host, "device"),
                                                "range": [min(host[other]) - max(host["device"]),
                                                          max(host[other]) - min(host["device"])]}
    out["ragged_minus_exact_fill_ms"] = {"median_of_medians": med(fill_ms, "fill_keypoints_ragged") - med(fill_ms, "fill_keypoints"),
                                         "range": [min(fill_ms["fill_keypoints_ragged"]) - max(fill_ms["fill_keypoints"]),
                                                   max(fill_ms["fill_keypoints_ragged"]) - min(fill_ms["fill_keypoints"])]}
    for a in arms.values():
        (a if hasattr(a, "close") else a.cap or a.last).close()
    ragged.close()
    exact.close()
    del arms, frames
    torch.cuda.empty_cache()
    return out


line = {"height": H, "width": W, "levels": LEVELS, "ring": RING, "grid": G, "points_per_cell": K, "repeats": REPEATS,
        "steps_per_timing": INNER,
        "timing": "arms alternated after warm-up; device events, the host clock around the steps + a final wait, and the "
                  "host clock until the last step's call returned; median (min - max) over the repeats",
        "large": measure(LARGE_F, 2000), "small": measure(8, 500),
        "lib_sha256": hashlib.sha256(open(capi.LIB_PATH, "rb").read()).hexdigest()}
print(json.dumps(line), flush=True)
if OUT:
    with open(OUT, "w") as f:
        json.dump(line, f, indent=1)
        f.write("\n")
