#!/usr/bin/env python3
"""What keypoint detection costs: F images of 1241 x 376 uint8 (smoothed noise, the patch tracker's workload), cell size
G = 30, one point per cell, everything device-resident.  One process, alternating D D2 P after warm-up, each timed with
device events around `inner` back-to-back calls:
   D   pnec_hip_detect_keypoints with no current points (the first frame: every cell is searched)
   D2  the same with `C` current points per image at random places (most cells occupied: a tracker's steady state)
   P   one pnec_hip_image_pyramid_level on the same images: a streaming kernel that reads the same pixels once
There is no acceptance ratio: nobody had measured any of it.  Recorded: medians and ranges, D / P, D2 / D, pixels and
cells per second, the share of occupied cells and the points found.  One image of each form is compared with the numpy
statement of the definition (tests/test_detect_keypoints_cpu.py) before anything is timed.
Prints one JSON object and, with an output path, writes it there (profiles/detect_keypoints.json).  Runs on the GPU box.
   python tools/bench_detect_keypoints.py [F] [C] [repeats] [out.json]"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

from pnec_amd import capi, patches

F = int(sys.argv[1]) if len(sys.argv) > 1 else 256
CUR = int(sys.argv[2]) if len(sys.argv) > 2 else 2000
REPEATS = int(sys.argv[3]) if len(sys.argv) > 3 else 15
OUT = sys.argv[4] if len(sys.argv) > 4 else None
H, W, INNER, G, K, T, E = 376, 1241, 5, 30, 1, 5, 19
dev = torch.device("cuda:0")

gen = torch.Generator(device=dev)
gen.manual_seed(13)
a = torch.rand((F, H + 6, W + 6), device=dev, generator=gen)
for _ in range(3):
    a = 0.25 * a[:, :-2] + 0.5 * a[:, 1:-1] + 0.25 * a[:, 2:]
    a = 0.25 * a[:, :, :-2] + 0.5 * a[:, :, 1:-1] + 0.25 * a[:, :, 2:]
lo, hi = a.amin(dim=(1, 2), keepdim=True), a.amax(dim=(1, 2), keepdim=True)
img = (24.0 + 206.0 * (a - lo) / (hi - lo)).round().to(torch.uint8).contiguous()
del a, lo, hi
cur = torch.stack([torch.rand(F * CUR, device=dev, generator=gen, dtype=torch.float64) * W,
                   torch.rand(F * CUR, device=dev, generator=gen, dtype=torch.float64) * H], 1).contiguous()
cur_offsets = (torch.arange(F + 1, device=dev, dtype=torch.int64) * CUR).contiguous()
nx, ny = W // G, H // G
n_cells, cap = nx * ny, F * nx * ny * K
i32 = dict(dtype=torch.int32, device=dev)
o_cell, o_off = torch.empty((F, n_cells), **i32), torch.empty((F + 1,), dtype=torch.int64, device=dev)
o_pts, o_sc, o_ci = torch.empty((cap, 2), dtype=torch.float64, device=dev), torch.empty((cap,), **i32), torch.empty((cap,), **i32)
half = torch.empty((F, H // 2, W // 2), dtype=torch.uint8, device=dev)
L = capi.lib()


def _stream():
    return torch.cuda.current_stream(0).cuda_stream


def detect(with_current):
    capi.check(L.pnec_hip_detect_keypoints(img.data_ptr(), patches.PIXEL_U8, F, H, W, W, G, K, T, E,
                                           cur_offsets.data_ptr() if with_current else None, F * CUR if with_current else 0,
                                           cur.data_ptr() if with_current else None, o_cell.data_ptr(), o_off.data_ptr(),
                                           o_pts.data_ptr(), o_sc.data_ptr(), o_ci.data_ptr(), capi.MEM_DEVICE, 0, _stream()))


def run_d():
    detect(False)


def run_d2():
    detect(True)


def run_p():
    capi.check(L.pnec_hip_image_pyramid_level(img.data_ptr(), half.data_ptr(), patches.PIXEL_U8, F, H, W, W, W // 2,
                                              capi.MEM_DEVICE, 0, _stream()))


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(INNER):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / INNER


# one image of each form against the numpy statement of the definition, before anything is timed
from test_detect_keypoints_cpu import detect_np  # noqa: E402

found, occupied, notes = {}, {}, {}
for key, with_current in (("D", False), ("D2", True)):
    detect(with_current)
    torch.cuda.synchronize()
    found[key] = int(o_off[-1])
    occupied[key] = float((o_cell < 0).double().mean())
    f = F // 2
    ref = detect_np(img[f].cpu().numpy(), G, K, T, E,
                    (np.array([0, CUR]), cur[f * CUR:(f + 1) * CUR].cpu().numpy()) if with_current else None)
    lo_, hi_ = int(o_off[f]), int(o_off[f + 1])
    same = (np.array_equal(o_cell[f].cpu().numpy(), ref["cell"][0]) and np.array_equal(o_pts[lo_:hi_].cpu().numpy(), ref["pts"])
            and np.array_equal(o_sc[lo_:hi_].cpu().numpy(), ref["score"])
            and np.array_equal(o_ci[lo_:hi_].cpu().numpy(), ref["cell_index"]))
    notes[key] = "equal to numpy" if same else "DIFFERS from numpy"

FORMS = (("D", run_d), ("D2", run_d2), ("P", run_p))
for _, fn in FORMS:
    for _ in range(2):
        fn()
torch.cuda.synchronize()
ms = {k: [] for k, _ in FORMS}
for _ in range(REPEATS):
    for key, fn in FORMS:
        ms[key].append(timed(fn))


def stat(x):
    x = np.asarray(x)
    return {"median_ms": float(np.median(x)), "min_ms": float(x.min()), "max_ms": float(x.max()),
            "spread_rel": float((x.max() - x.min()) / np.median(x))}


D_, D2_, P_ = (float(np.median(ms[k])) for k in ("D", "D2", "P"))
line = {"images": F, "height": H, "width": W, "pixel_type": "uint8", "grid": G, "points_per_cell": K, "min_threshold": T,
        "edge": E, "cells_per_image": n_cells, "current_points_per_image_D2": CUR, "repeats": REPEATS,
        "calls_per_timing": INNER, "timing": "device events around back-to-back calls, D D2 P alternated",
        "D_detect_no_current_points": stat(ms["D"]), "D2_detect_with_current_points": stat(ms["D2"]),
        "P_one_pyramid_level": stat(ms["P"]),
        "D_over_P": D_ / P_, "D_over_P_range": [min(ms["D"]) / max(ms["P"]), max(ms["D"]) / min(ms["P"])],
        "D2_over_D": D2_ / D_, "D2_over_D_range": [min(ms["D2"]) / max(ms["D"]), max(ms["D2"]) / min(ms["D"])],
        "D_pixels_per_s": F * H * W / (D_ * 1e-3), "P_pixels_per_s": F * H * W / (P_ * 1e-3),
        "D_cells_per_s": F * n_cells / (D_ * 1e-3), "D_ns_per_cell": D_ * 1e6 / (F * n_cells),
        "points_found": found, "occupied_cell_share": occupied, "one_image_check": notes,
        "lib_sha256": hashlib.sha256(open(capi.LIB_PATH, "rb").read()).hexdigest()}
print(json.dumps(line), flush=True)
if OUT:
    with open(OUT, "w") as f:
        json.dump(line, f, indent=1)
        f.write("\n")
