#!/usr/bin/env python3
"""What the patch-covariance pass costs, next to the keypoint ingest it feeds: F images of 1241 x 376 uint8 (smoothed
noise) with K keypoints each, everything device-resident; the same F * K keypoints as a TARGET batch of F pairs x K
correspondences for the fused keypoint ingest.  One process, alternating C I C I after warm-up, each timed with device
events around `inner` back-to-back calls:
   C  pnec_hip_patch_covariance, covariance and status only (what the ingest needs), Pattern52, scaling 10, no angle
   A  the same with all five outputs and an angle per keypoint
   I  pnec_hip_problem_fill_keypoints (Unproject + UnscentedTransform into the SoA planes) with C's covariances
There is no acceptance ratio: nobody had measured either.  Recorded: medians and ranges, C / I with the run's spread,
keypoints per second, and the pixel traffic the gathers ask for (52 points x 12 pixels per keypoint, by instruction, not
by cache line) over C's time.  The covariances of a sample of keypoints are compared with the numpy statement of the
definition (tests/test_patch_covariance_cpu.py) before anything is timed.
Prints one JSON object and, with an output path, writes it there (profiles/patch_covariance.json).  Runs on the GPU box.
   python tools/bench_patch_covariance.py [F] [K] [repeats] [out.json]"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

from pnec_amd import Batch, capi, patches

F = int(sys.argv[1]) if len(sys.argv) > 1 else 256
K = int(sys.argv[2]) if len(sys.argv) > 2 else 2000
REPEATS = int(sys.argv[3]) if len(sys.argv) > 3 else 15
OUT = sys.argv[4] if len(sys.argv) > 4 else None
H, W, INNER = 376, 1241, 5
dev = torch.device("cuda:0")
M = F * K

gen = torch.Generator(device=dev)
gen.manual_seed(11)
# smoothed noise, made on the device: white noise under three passes of the 1-2-1 filter per axis, stretched to 24 .. 230
a = torch.rand((F, H + 6, W + 6), device=dev, generator=gen)
for _ in range(3):
    a = 0.25 * a[:, :-2] + 0.5 * a[:, 1:-1] + 0.25 * a[:, 2:]
    a = 0.25 * a[:, :, :-2] + 0.5 * a[:, :, 1:-1] + 0.25 * a[:, :, 2:]
lo, hi = a.amin(dim=(1, 2), keepdim=True), a.amax(dim=(1, 2), keepdim=True)
images = (24.0 + 206.0 * (a - lo) / (hi - lo)).round().to(torch.uint8).contiguous()
del a, lo, hi
# keypoints anywhere a tracker would keep them: the whole patch inside the image
pts = torch.stack([torch.rand(M, device=dev, generator=gen, dtype=torch.float64) * (W - 12.0) + 5.5,
                   torch.rand(M, device=dev, generator=gen, dtype=torch.float64) * (H - 12.0) + 5.5], 1).contiguous()
pts1 = (pts + torch.randn((M, 2), device=dev, generator=gen, dtype=torch.float64) * 5.0).contiguous()
angle = ((torch.rand(M, device=dev, generator=gen, dtype=torch.float64) - 0.5) * 0.4).contiguous()
offsets = (torch.arange(F + 1, device=dev, dtype=torch.int64) * K).contiguous()
pattern = torch.from_numpy(np.array(patches.PATTERN52)).to(dev)
f64 = dict(dtype=torch.float64, device=dev)
i32 = dict(dtype=torch.int32, device=dev)
o_cov, o_hes, o_mean = torch.empty((M, 3), **f64), torch.empty((M, 6), **f64), torch.empty((M,), **f64)
o_nv, o_st = torch.empty((M,), **i32), torch.empty((M,), **i32)
L = capi.lib()
Kmat = np.array([[718.856, 0, 607.1928], [0, 718.856, 185.2157], [0, 0, 1.0]])
Kinv = np.linalg.inv(Kmat)
batch = Batch.uniform(capi.MODE_TARGET, F, K)


def _stream():
    return torch.cuda.current_stream(0).cuda_stream


def run_c():
    capi.check(L.pnec_hip_patch_covariance(images.data_ptr(), patches.PIXEL_U8, F, H, W, W, offsets.data_ptr(), M,
                                           pts.data_ptr(), pattern.data_ptr(), 52, 10.0, None, o_cov.data_ptr(), None, None,
                                           None, o_st.data_ptr(), capi.MEM_DEVICE, 0, _stream()))


def run_a():
    capi.check(L.pnec_hip_patch_covariance(images.data_ptr(), patches.PIXEL_U8, F, H, W, W, offsets.data_ptr(), M,
                                           pts.data_ptr(), pattern.data_ptr(), 52, 10.0, angle.data_ptr(), o_cov.data_ptr(),
                                           o_hes.data_ptr(), o_mean.data_ptr(), o_nv.data_ptr(), o_st.data_ptr(),
                                           capi.MEM_DEVICE, 0, _stream()))


def run_i():
    batch.fill_keypoints(pts1, pts, cov_in, K_inv=Kinv)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(INNER):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / INNER


run_c()
torch.cuda.synchronize()
n_ok = int((o_st == 0).sum())
cov_in = o_cov.clone()
# a sample against the numpy statement of the definition, before anything is timed
from test_patch_covariance_cpu import check_against_np, patch_cov_np  # noqa: E402

run_a()
torch.cuda.synchronize()
sample = np.arange(0, M, max(1, M // 64))[:64]
frames = sample // K
ref_parts = [patch_cov_np(images[f].cpu().numpy(), pts[k:k + 1].cpu().numpy(), angle=angle[k:k + 1].cpu().numpy())
             for f, k in zip(frames, sample)]
ref = {key: np.concatenate([r[key] for r in ref_parts]) for key in ref_parts[0]}
got = dict(cov=o_cov[sample].cpu().numpy(), hessian=o_hes[sample].cpu().numpy(), mean=o_mean[sample].cpu().numpy(),
           n_valid=o_nv[sample].cpu().numpy(), status=o_st[sample].cpu().numpy())
worst_h, worst_c, worst_m = check_against_np(got, ref, "sample of 64 keypoints")

FORMS = (("C", run_c), ("A", run_a), ("I", run_i))
for _, fn in FORMS:
    for _ in range(5):
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


C_, A_, I_ = (float(np.median(ms[k])) for k in ("C", "A", "I"))
line = {"images": F, "height": H, "width": W, "pixel_type": "uint8", "keypoints_per_image": K, "keypoints": M,
        "pattern_points": 52, "repeats": REPEATS, "calls_per_timing": INNER,
        "timing": "device events around back-to-back calls, C A I alternated",
        "C_patch_covariance_cov_and_status": stat(ms["C"]), "A_patch_covariance_all_outputs_with_angle": stat(ms["A"]),
        "I_fill_keypoints": stat(ms["I"]),
        "C_over_I": C_ / I_, "C_over_I_range": [min(ms["C"]) / max(ms["I"]), max(ms["C"]) / min(ms["I"])],
        "A_over_C": A_ / C_,
        "C_keypoints_per_s": M / (C_ * 1e-3), "A_keypoints_per_s": M / (A_ * 1e-3), "I_keypoints_per_s": M / (I_ * 1e-3),
        "pixel_loads_per_keypoint": 52 * 12, "C_pixel_loads_per_s": M * 52 * 12 / (C_ * 1e-3),
        "image_bytes": F * H * W, "share_status_ok": n_ok / M,
        "sample_worst_hessian_error": worst_h, "sample_worst_covariance_error_over_bound": worst_c,
        "sample_worst_mean_error": worst_m,
        "lib_sha256": hashlib.sha256(open(capi.LIB_PATH, "rb").read()).hexdigest()}
print(json.dumps(line), flush=True)
if OUT:
    with open(OUT, "w") as f:
        json.dump(line, f, indent=1)
        f.write("\n")
