#!/usr/bin/env python3
"""What keypoint undistortion costs: pnec_hip_undistort_keypoints under each flag combination next to a device-to-device
copy of the same bytes (the read-once, write-once floor) and next to pnec_hip_problem_fill_keypoints_ragged on the same
rows, and one Odometry step with and without a distortion.  Device-resident inputs, one process; after warm-up the arms
alternate, each timed with device events around 5 back-to-back calls, medians over the repeats:
   U0 U1 U2 U3   undistort_keypoints(pts1, pts2, cov2) with flags 0 (the reference), NEWTON, PROPAGATE_COV, both;
                 EuRoC-like camera, points spread over 752 x 480, all outputs and both statuses into preallocated tensors
   C             one copy of 7 doubles a row and one of 2 bytes a row: what the call reads once and writes once
   F             fill_keypoints_ragged of the same rows into a capacity batch (TARGET mode)
on 256 x 2000 rows and 20 000 x 512 rows; then Odometry.process at 256 sequences of 1241 x 376 with distortion=None
against the mild coefficients (device events and the host clock until the call returned).  Nothing is fixed in advance.
Prints one JSON object and, with an output path, writes it there (profiles/undistort.json).  Runs on the GPU box.
   python tools/bench_undistort.py [repeats] [out.json] [sequences]"""
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from pnec_amd import Batch, Odometry, camera_array, capi, undistort_keypoints
from pnec_amd.undistort import new_undistorted

REPEATS = int(sys.argv[1]) if len(sys.argv) > 1 else 15
OUT = sys.argv[2] if len(sys.argv) > 2 and sys.argv[2] != "-" else None
F = int(sys.argv[3]) if len(sys.argv) > 3 else 256
INNER = 5
dev = torch.device("cuda:0")
f64 = dict(dtype=torch.float64, device=dev)
EUROC = camera_array(458.654, 457.296, 367.215, 248.375, -0.28340811, 0.07395907, 0.00019359, 1.76187114e-05)
MILD = [-0.05, 0.01, 1e-3, -5e-4]


def stat(x):
    x = np.asarray(x)
    return {"median_ms": float(np.median(x)), "min_ms": float(x.min()), "max_ms": float(x.max()),
            "spread_rel": float((x.max() - x.min()) / np.median(x))}


def timed(fn):
    a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(INNER):
        fn()
    z.record()
    z.synchronize()
    return a.elapsed_time(z) / INNER


def rows_case(n_pairs, n_corr):
    n = n_pairs * n_corr
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    size = torch.tensor([752.0, 480.0], **f64)
    pts1 = torch.rand((n, 2), generator=gen, **f64) * size
    pts2 = torch.rand((n, 2), generator=gen, **f64) * size
    s = 0.1 + 0.9 * torch.rand((n, 2), generator=gen, **f64)
    cov2 = torch.stack([s[:, 0] ** 2, 0.3 * s[:, 0] * s[:, 1], s[:, 1] ** 2], dim=1).contiguous()
    cam = torch.as_tensor(EUROC, **f64)
    out = new_undistorted(n, True, dev)
    flat_in, flat_out = torch.empty(7 * n, **f64), torch.empty(7 * n, **f64)
    byte_in, byte_out = (torch.zeros(2 * n, dtype=torch.uint8, device=dev) for _ in range(2))
    batch = Batch.with_capacity(capi.MODE_TARGET, n_pairs, n, device=0)
    batch.reshape(np.arange(n_pairs + 1, dtype=np.int64) * n_corr)
    offsets = torch.arange(n_pairs + 1, dtype=torch.int64, device=dev) * n_corr
    k_inv = torch.as_tensor(np.linalg.inv(np.array([[EUROC[0], 0, EUROC[2]], [0, EUROC[1], EUROC[3]], [0, 0, 1.0]])), **f64)

    def und(newton, propagate):
        return lambda: undistort_keypoints(cam, pts1, pts2, cov2, newton=newton, propagate_cov=propagate, out=out)

    def copy():
        flat_out.copy_(flat_in)
        byte_out.copy_(byte_in)

    arms = {"U0_reference": und(False, False), "U1_newton": und(True, False), "U2_propagate_cov": und(False, True),
            "U3_newton_propagate_cov": und(True, True), "C_copy_of_the_same_bytes": copy,
            "F_fill_keypoints_ragged": lambda: batch.fill_keypoints_ragged(offsets, pts1, pts2, cov2, K_inv=k_inv)}
    for fn in arms.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    arms["U1_newton"]()
    torch.cuda.synchronize()
    status = torch.bincount(torch.cat([out.status1, out.status2]).to(torch.int64), minlength=4).tolist()
    ms = {k: [] for k in arms}
    for _ in range(REPEATS):
        for k, fn in arms.items():
            ms[k].append(timed(fn))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    moved = 2 * (7 * 8 * n) + 2 * 2 * n
    res = {"rows": n, "shape": f"{n_pairs} x {n_corr}", "bytes_read_plus_written": moved,
           "status_counts_newton": {capi.UNDISTORT_NAMES[k]: status[k] for k in range(4)},
           **{k: stat(v) for k, v in ms.items()},
           "over_copy": {k: med[k] / med["C_copy_of_the_same_bytes"] for k in med if k[0] == "U"},
           "over_fill_keypoints_ragged": {k: med[k] / med["F_fill_keypoints_ragged"] for k in med if k[0] == "U"},
           "GBps": {k: moved / (med[k] * 1e-3) / 1e9 for k in med if k[0] in "UC"}}
    batch.close()
    return res


def make_frames(H, W):
    gen = torch.Generator(device=dev)
    gen.manual_seed(13)
    a = torch.rand((F, H + 6, W + 6), device=dev, generator=gen)
    for _ in range(3):
        a = 0.25 * a[:, :-2] + 0.5 * a[:, 1:-1] + 0.25 * a[:, 2:]
        a = 0.25 * a[:, :, :-2] + 0.5 * a[:, :, 1:-1] + 0.25 * a[:, :, 2:]
    lo, hi = a.amin(dim=(1, 2), keepdim=True), a.amax(dim=(1, 2), keepdim=True)
    img0 = (24.0 + 206.0 * (a - lo) / (hi - lo)).round().to(torch.uint8).contiguous()
    return [torch.roll(img0, shifts=3 * n, dims=2).contiguous() for n in range(4)]


def odometry_case():
    H, W = 376, 1241
    k_inv = np.linalg.inv(np.array([[718.856, 0.0, 607.1928], [0.0, 718.856, 185.2157], [0.0, 0.0, 1.0]]))
    tracker = dict(levels=5, ring=4, grid=30, points_per_cell=4, capacity=2000)
    frames = make_frames(H, W)
    arms = {"distortion_none": Odometry(F, H, W, k_inv, **tracker),
            "distortion_mild": Odometry(F, H, W, k_inv, distortion=MILD, **tracker),
            "distortion_mild_newton_propagate": Odometry(F, H, W, k_inv, distortion=MILD, undistort_newton=True,
                                                         undistort_propagate_cov=True, **tracker)}
    count = {k: 0 for k in arms}

    def step(k):
        arms[k].process(frames[count[k] % 4])
        count[k] += 1

    for k in arms:
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
            for _ in range(3):
                step(k)
            b.record()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            ev[k].append(a.elapsed_time(b) / 3)
            ret[k].append((t1 - t0) * 1e3 / 3)
    for o in arms.values():
        o.close()
    return {"sequences": F, "height": H, "width": W, "rows": F * 2000, "steps_per_timing": 3,
            "step_device_events": {k: stat(v) for k, v in ev.items()},
            "step_host_clock_until_returned": {k: stat(v) for k, v in ret.items()},
            "mild_minus_none_device_ms": float(np.median(ev["distortion_mild"]) - np.median(ev["distortion_none"]))}


out = {"repeats": REPEATS, "calls_per_timing": INNER,
       "timing": "device events around back-to-back calls, arms alternating after warm-up; median (min - max) over the repeats",
       "lib_sha256": hashlib.sha256(open(capi.LIB_PATH, "rb").read()).hexdigest()}
out["rows_256x2000"] = rows_case(256, 2000)
torch.cuda.empty_cache()
out["rows_20000x512"] = rows_case(20_000, 512)
torch.cuda.empty_cache()
out["odometry_step"] = odometry_case()
out["measured"] = ["the call under the four flag combinations", "a device-to-device copy of the same bytes",
                   "fill_keypoints_ragged on the same rows", "one Odometry step with and without a distortion"]
out["not_measured"] = ["a wave-wide contiguous read of the covariance rows re-dealt through LDS (not built)",
                       "a reciprocal faster than the IEEE division (not built)", "HOST space"]
print(json.dumps(out), flush=True)
if OUT:
    with open(OUT, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
