#!/usr/bin/env python3
"""What the running scale and pose cost on top of the poses: one ScaledOdometry.process step (Odometry.process, then
triangulate for the sign, tracks_link, relative_scale, trajectory_advance and two copies) against one Odometry.process
step in the same run, at the two sizes of tools/bench_odometry.py (1241 x 376 uint8 smoothed noise, frame n = frame 0
rolled by 3 n pixels; grid 30, 4 points per cell, 5 levels, a ring of 4 so that consecutive pairs share tracks):
   large   256 sequences, capacity 2 000 per image
   small   8 sequences, capacity 500
The arms are alternated after warm-up, each timed over `inner` back-to-back steps by device events, by the host clock
with a final wait, and by the host clock until the last call has returned.
The two new calls alone, device events around `inner` back-to-back calls:
   tracks_link         256 x 2 000 rows, every image's ids ascending, about 3 of 4 linked, against a device copy of the
                       bytes the call moves (both id arrays and both offset arrays in, the links out)
   trajectory_advance  256 and 65 536 sequences
There is no acceptance figure: nobody had measured any of it.  Prints one JSON object and, with an output path, writes it
there (profiles/scaled_odometry.json).  Runs on the GPU box.
   python tools/bench_scaled_odometry.py [repeats] [out.json] [large_F]"""
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from pnec_amd import Odometry, ScaledOdometry, advance_trajectory, capi, link_tracks, new_trajectory_state

REPEATS = int(sys.argv[1]) if len(sys.argv) > 1 else 11
OUT = sys.argv[2] if len(sys.argv) > 2 and sys.argv[2] != "-" else None
LARGE_F = int(sys.argv[3]) if len(sys.argv) > 3 else 256
H, W, INNER, G, K, LEVELS, RING = 376, 1241, 3, 30, 4, 5, 4
dev = torch.device("cuda:0")
K_INV = np.linalg.inv(np.array([[718.856, 0.0, 607.1928], [0.0, 718.856, 185.2157], [0.0, 0.0, 1.0]]))


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


def stat(x):
    x = np.asarray(x)
    return {"median_ms": float(np.median(x)), "min_ms": float(x.min()), "max_ms": float(x.max()),
            "spread_rel": float((x.max() - x.min()) / np.median(x))}


def events(fn, inner=INNER):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def measure_steps(F, C):
    frames = make_frames(F)
    kw = dict(levels=LEVELS, ring=RING, grid=G, points_per_cell=K, capacity=C)
    arms = {"odometry": Odometry(F, H, W, K_INV, **kw), "scaled": ScaledOdometry(F, H, W, K_INV, min_corr=8, min_links=8, **kw)}
    count = {k: 0 for k in arms}
    last = {}

    def step(k):
        last[k] = arms[k].process(frames[count[k] % 4])
        count[k] += 1

    for k in arms:
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
    torch.cuda.synchronize()
    r = last["scaled"]
    same = torch.equal(r.step.q.view(torch.int64), last["odometry"].q.view(torch.int64))
    status = r.status.cpu().numpy()
    out = {"sequences": F, "capacity_per_image": C, "same_pose_bits_in_both_arms": bool(same),
           "last_step": {"status_counts": {capi.TRAJ_NAMES[s]: int((status == s).sum()) for s in range(4)},
                         "n_corr_mean": float(r.step.n_corr.double().mean()), "n_linked_mean": float(r.n_linked.double().mean()),
                         "n_used_mean": float(r.n_used.double().mean())},
           "device_events": {k: stat(v) for k, v in ev.items()},
           "host_clock_with_final_wait": {k: stat(v) for k, v in host.items()},
           "host_clock_until_returned": {k: stat(v) for k, v in ret.items()}}
    med = lambda d, k: float(np.median(d[k]))
    out["scaled_minus_odometry_device_ms"] = {"median_of_medians": med(ev, "scaled") - med(ev, "odometry"),
                                              "range": [min(ev["scaled"]) - max(ev["odometry"]), max(ev["scaled"]) - min(ev["odometry"])]}
    for a in arms.values():
        a.close()
    del arms, frames, last
    torch.cuda.empty_cache()
    return out


def measure_link(F, C):
    rng = np.random.default_rng(3)
    prev = np.cumsum(rng.integers(1, 4, (F, C)), axis=1).astype(np.int64)              # ascending within an image
    keep = rng.random((F, C)) < 0.75
    cur = np.where(keep, prev, prev + 10 ** 9)
    cur = np.sort(cur, axis=1)
    off = torch.arange(F + 1, dtype=torch.int64, device=dev) * C
    ci, pi = torch.as_tensor(cur.reshape(-1), device=dev), torch.as_tensor(prev.reshape(-1), device=dev)
    link = torch.empty((F * C,), dtype=torch.int32, device=dev)
    n_linked = torch.empty((F,), dtype=torch.int32, device=dev)
    src = torch.empty((2 * F * C + 2 * (F + 1)) * 8 + F * C * 4, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    arms = {"tracks_link": lambda: link_tracks(off, ci, off, pi, out=link, n_linked=n_linked),
            "device_copy_of_the_same_bytes": lambda: dst.copy_(src)}
    for fn in arms.values():
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for _ in range(REPEATS):
        for k, fn in arms.items():
            ms[k].append(events(fn, 10))
    return {"images": F, "rows": F * C, "bytes": int(src.numel()), "linked_fraction": float((link >= 0).double().mean()),
            "device_events": {k: stat(v) for k, v in ms.items()}}


def measure_advance(n):
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)
    f = lambda *shape: torch.randn(shape, dtype=torch.float64, device=dev, generator=gen)
    rq, rt, s3 = f(n, 4), f(n, 3), f(n, 3).abs() + 0.5
    cnt = torch.full((n,), 50, dtype=torch.int32, device=dev)
    a, b = new_trajectory_state(n, True, dev), new_trajectory_state(n, True, dev)
    status = torch.empty((n,), dtype=torch.int32, device=dev)
    fn = lambda: advance_trajectory(a, rq, rt, cnt, 8, s3, cnt, 8, out=(b, status))
    fn()
    torch.cuda.synchronize()
    return {"sequences": n, "device_events": stat([events(fn, 10) for _ in range(REPEATS)])}


line = {"height": H, "width": W, "levels": LEVELS, "ring": RING, "grid": G, "points_per_cell": K, "repeats": REPEATS,
        "steps_per_timing": INNER,
        "timing": "arms alternated after warm-up; device events, the host clock around the steps + a final wait, and the "
                  "host clock until the last step's call returned; median (min - max) over the repeats; the calls alone: "
                  "device events around 10 back-to-back calls",
        "large": measure_steps(LARGE_F, 2000), "small": measure_steps(8, 500),
        "tracks_link": measure_link(LARGE_F, 2000),
        "trajectory_advance": [measure_advance(256), measure_advance(65536)],
        "lib_sha256": hashlib.sha256(open(capi.LIB_PATH, "rb").read()).hexdigest()}
print(json.dumps(line), flush=True)
if OUT:
    with open(OUT, "w") as f:
        json.dump(line, f, indent=1)
        f.write("\n")
