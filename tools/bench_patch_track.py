#!/usr/bin/env python3
"""What patch tracking costs: F image pairs of 1241 x 376 uint8 (smoothed noise; the second image is the first moved by
a few pixels) with K keypoints each, Pattern52, five levels, 40 iterations per level, everything device-resident.  One
process, alternating T F P C after warm-up, each timed with device events around `inner` back-to-back calls:
   T  pnec_hip_patch_track with the backward track (all six outputs)
   F  the same, forward only (PNEC_HIP_TRACK_NO_BACKWARD)
   P  building the two five-level pyramids (2 x 4 calls of pnec_hip_image_pyramid_level)
   C  pnec_hip_patch_covariance, covariance and status only: the parent's kernel, one template's worth of work
There is no acceptance ratio: nobody had measured any of it.  Recorded: medians and ranges, T / C, F / T, keypoints per
second, and the share of each status.  A sample of keypoints is compared with the numpy statement of the definition
(tests/test_patch_track_cpu.py) before anything is timed.
Prints one JSON object and, with an output path, writes it there (profiles/patch_track.json).  Runs on the GPU box.
   python tools/bench_patch_track.py [F] [K] [repeats] [out.json]"""
import ctypes as C
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
K = int(sys.argv[2]) if len(sys.argv) > 2 else 2000
REPEATS = int(sys.argv[3]) if len(sys.argv) > 3 else 15
OUT = sys.argv[4] if len(sys.argv) > 4 else None
H, W, INNER, LEVELS, ITERATIONS = 376, 1241, 5, 5, 40
MOVE = (3, -2)                     # image 2 is image 1 moved by (dx, dy) pixels
dev = torch.device("cuda:0")
M = F * K

gen = torch.Generator(device=dev)
gen.manual_seed(13)
a = torch.rand((F, H + 6 + 8, W + 6 + 8), device=dev, generator=gen)
for _ in range(3):
    a = 0.25 * a[:, :-2] + 0.5 * a[:, 1:-1] + 0.25 * a[:, 2:]
    a = 0.25 * a[:, :, :-2] + 0.5 * a[:, :, 1:-1] + 0.25 * a[:, :, 2:]
lo, hi = a.amin(dim=(1, 2), keepdim=True), a.amax(dim=(1, 2), keepdim=True)
big = (24.0 + 206.0 * (a - lo) / (hi - lo)).round().to(torch.uint8)
img1 = big[:, 4:4 + H, 4:4 + W].contiguous()
img2 = big[:, 4 - MOVE[1]:4 - MOVE[1] + H, 4 - MOVE[0]:4 - MOVE[0] + W].contiguous()    # I2(p) = I1(p - MOVE)
del a, lo, hi, big
# keypoints whose patch fits the top level (77 x 23 pixels) with the motion to spare
pts = torch.stack([torch.rand(M, device=dev, generator=gen, dtype=torch.float64) * 1000.0 + 104.0,
                   torch.rand(M, device=dev, generator=gen, dtype=torch.float64) * 140.0 + 100.0], 1).contiguous()
offsets = (torch.arange(F + 1, device=dev, dtype=torch.int64) * K).contiguous()
pattern = torch.from_numpy(np.array(patches.PATTERN52)).to(dev)
f64 = dict(dtype=torch.float64, device=dev)
i32 = dict(dtype=torch.int32, device=dev)
o_pts, o_ang, o_cov, o_d2 = torch.empty((M, 2), **f64), torch.empty((M,), **f64), torch.empty((M, 3), **f64), torch.empty((M,), **f64)
o_st, o_lv = torch.empty((M,), **i32), torch.empty((M,), **i32)
L = capi.lib()


def _stream():
    return torch.cuda.current_stream(0).cuda_stream


def new_pyramid():
    return [torch.empty((F, H >> l, W >> l), dtype=torch.uint8, device=dev) for l in range(LEVELS)]


pyr1, pyr2 = new_pyramid(), new_pyramid()
pyr1[0], pyr2[0] = img1, img2


def table(pyr):
    return (C.c_void_p * LEVELS)(*[t.data_ptr() for t in pyr]), (C.c_int64 * LEVELS)(*[int(t.shape[2]) for t in pyr])


T1, Q1 = table(pyr1)
T2, Q2 = table(pyr2)


def run_p():
    for pyr in (pyr1, pyr2):
        for l in range(1, LEVELS):
            capi.check(L.pnec_hip_image_pyramid_level(pyr[l - 1].data_ptr(), pyr[l].data_ptr(), patches.PIXEL_U8, F, H >> (l - 1),
                                                      W >> (l - 1), W >> (l - 1), W >> l, capi.MEM_DEVICE, 0, _stream()))


def track(flags):
    capi.check(L.pnec_hip_patch_track(T1, Q1, None, None, T2, Q2, LEVELS, patches.PIXEL_U8, F, H, W, offsets.data_ptr(), M,
                                      pts.data_ptr(), None, None, 0.0, 0.0, pattern.data_ptr(), 52, ITERATIONS, 0.04, flags,
                                      10.0, o_pts.data_ptr(), o_ang.data_ptr(), o_cov.data_ptr(), o_d2.data_ptr(),
                                      o_st.data_ptr(), o_lv.data_ptr(), capi.MEM_DEVICE, 0, _stream()))


def run_t():
    track(0)


def run_f():
    track(patches.TRACK_NO_BACKWARD)


c_cov, c_st = torch.empty((M, 3), **f64), torch.empty((M,), **i32)


def run_c():
    capi.check(L.pnec_hip_patch_covariance(img1.data_ptr(), patches.PIXEL_U8, F, H, W, W, offsets.data_ptr(), M,
                                           pts.data_ptr(), pattern.data_ptr(), 52, 10.0, None, c_cov.data_ptr(), None, None,
                                           None, c_st.data_ptr(), capi.MEM_DEVICE, 0, _stream()))


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(INNER):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / INNER


run_p()
run_t()
torch.cuda.synchronize()
status = o_st.cpu().numpy()
shares = {patches.TRACK_NAMES[s]: float((status == s).mean()) for s in range(5)}
moved = (o_pts - pts)[o_st == 0]
median_motion = [float(moved[:, 0].median()), float(moved[:, 1].median())] if moved.numel() else [float("nan")] * 2
# a sample against the numpy statement of the definition, before anything is timed
from test_patch_track_cpu import check_track_against_np, patch_track_np  # noqa: E402

sample = np.arange(0, M, max(1, M // 32))[:32]
parts = []
for k in sample:
    f = int(k // K)
    parts.append(patch_track_np([p[f].cpu().numpy() for p in pyr1], [p[f].cpu().numpy() for p in pyr2],
                                pts[k:k + 1].cpu().numpy(), max_iterations=ITERATIONS))
ref = {key: np.concatenate([r[key] for r in parts]) for key in parts[0]}
got = dict(pts=o_pts[sample].cpu().numpy(), angle=o_ang[sample].cpu().numpy(), dist2=o_d2[sample].cpu().numpy(),
           status=o_st[sample].cpu().numpy(), lost_level=o_lv[sample].cpu().numpy())
try:     # (a gate for the tests, a record here: a wandering track on this texture would say so in the profile)
    worst_p, worst_a, worst_d = check_track_against_np(got, ref, "sample of 32 keypoints")
    sample_note = "within the tests' bounds"
except AssertionError as e:
    worst_p = worst_a = worst_d = float("nan")
    sample_note = "OUTSIDE the tests' bounds: " + str(e)[:300]

FORMS = (("T", run_t), ("F", run_f), ("P", run_p), ("C", run_c))
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


T_, F_, P_, C_ = (float(np.median(ms[k])) for k in ("T", "F", "P", "C"))
line = {"images": F, "height": H, "width": W, "pixel_type": "uint8", "keypoints_per_image": K, "keypoints": M,
        "pattern_points": 52, "levels": LEVELS, "max_iterations": ITERATIONS, "image_motion_px": list(MOVE),
        "repeats": REPEATS, "calls_per_timing": INNER,
        "timing": "device events around back-to-back calls, T F P C alternated",
        "T_track_forward_backward": stat(ms["T"]), "F_track_forward_only": stat(ms["F"]),
        "P_two_pyramids_of_five_levels": stat(ms["P"]), "C_patch_covariance_cov_and_status": stat(ms["C"]),
        "T_over_C": T_ / C_, "T_over_C_range": [min(ms["T"]) / max(ms["C"]), max(ms["T"]) / min(ms["C"])],
        "F_over_T": F_ / T_, "F_over_T_range": [min(ms["F"]) / max(ms["T"]), max(ms["F"]) / min(ms["T"])],
        "P_over_T": P_ / T_,
        "T_keypoints_per_s": M / (T_ * 1e-3), "F_keypoints_per_s": M / (F_ * 1e-3),
        "iterations_per_keypoint_T": 2 * LEVELS * ITERATIONS,
        "T_ns_per_keypoint_iteration": T_ * 1e6 / (M * 2 * LEVELS * ITERATIONS),
        "P_pixels_per_s": 2 * F * H * W / (P_ * 1e-3),
        "status_shares": shares, "median_motion_found_px": median_motion,
        "sample_worst_position_error_over_bound": worst_p, "sample_worst_angle_error_over_bound": worst_a,
        "sample_worst_dist2_error_over_bound": worst_d, "sample_check": sample_note,
        "lib_sha256": hashlib.sha256(open(capi.LIB_PATH, "rb").read()).hexdigest()}
print(json.dumps(line), flush=True)
if OUT:
    with open(OUT, "w") as f:
        json.dump(line, f, indent=1)
        f.write("\n")
