#!/usr/bin/env python3
"""What trajectory evaluation costs: pnec_hip_trajectory_metrics and pnec_hip_trajectory_compose on the KITTI-like
lengths (4541, 1101, 4661, 801, 271, 2761, 1101, 1101, 4071, 1591, 1201 frames: 23 201 rows, 37.4 M frame pairs),
device-resident inputs, outputs into preallocated tensors, one process.  After warm-up the arms alternate, each timed with device events
around back-to-back calls, medians over the repeats:
   M     trajectory_metrics of the eleven sequences in one call
   M1    trajectory_metrics of the 4541-frame sequence alone (10.3 M pairs)
   T1    the straightforward torch port of the reference on the same GPU for that sequence: rotation matrices, and per
         distance one batched matmul chain, trace, arccos, RMSE and mean (scripts/pnec/metrics/rmse.py, l1_error.py); one
         call a timing, fewer repeats -- it is 4540 x ~10 launches
   C     trajectory_compose of the eleven sequences (rel_q, rel_t -> q, p, valid)
   Cc    a device-to-device copy of the bytes C reads once and writes once
Reports pairs/s and, with the FP64 instructions a pair costs in the distance kernel's loop (counted in the ISA listing),
the fraction of the FP64 vector rate of the datasheet (78.6 TFLOP/s = 39.3 T lane-instructions/s at the peak clock; the
traffic of a pair is two 32-byte rows out of L2).  The loop has 59 FP64 instructions on the path every pair takes and 50
more in asin's branch for arguments above 0.5, which a wavefront enters only when one of its 64 angles exceeds 2.09 rad:
this workload's angles stay far below that, so the fraction is given for the 59 (FP64_PER_PAIR) and, as the figure for
data with large angles, for all 109.  Nothing is fixed in advance.
Prints one JSON object and, with an output path, writes it there (profiles/trajectory_metrics.json).  Runs on the GPU box.
   python tools/bench_trajectory.py [repeats] [out.json]"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from pnec_amd import Trajectory, capi, compose_trajectory, trajectory_metrics
from pnec_amd.trajectory import new_trajectory_metrics

REPEATS = int(sys.argv[1]) if len(sys.argv) > 1 else 15
OUT = sys.argv[2] if len(sys.argv) > 2 and sys.argv[2] != "-" else None
INNER = 5
LENGTHS = [4541, 1101, 4661, 801, 271, 2761, 1101, 1101, 4071, 1591, 1201]
FP64_PER_PAIR = 59                     # v_*_f64 in the loop of trajectory_distance_kernel on the path every pair takes
FP64_PER_PAIR_LARGE_ANGLES = 109       # ... with asin's branch for arguments above 0.5 (angles above 2.09 rad)
FP64_LANE_INSTRUCTIONS_PER_S = 39.3e12  # datasheet: 78.6 TFLOP/s FP64 vector, two flops a fused multiply-add
dev = torch.device("cuda:0")
f64 = dict(dtype=torch.float64, device=dev)


def stat(x):
    x = np.asarray(x)
    return {"median_ms": float(np.median(x)), "min_ms": float(x.min()), "max_ms": float(x.max()),
            "spread_rel": float((x.max() - x.min()) / np.median(x))}


def timed(fn, inner=INNER):
    a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    z.record()
    z.synchronize()
    return a.elapsed_time(z) / inner


def steps(n, sigma, gen):
    """unit quaternions exp(N(0, sigma^2)) and unit translations"""
    w = torch.randn((n, 3), generator=gen, **f64) * sigma
    th = w.norm(dim=1, keepdim=True)
    q = torch.cat([torch.sin(th / 2) / th * w, torch.cos(th / 2)], dim=1)
    t = torch.randn((n, 3), generator=gen, **f64)
    return q.contiguous(), (t / t.norm(dim=1, keepdim=True)).contiguous()


def qmul(a, b):
    ax, ay, az, aw = a.unbind(-1)
    bx, by, bz, bw = b.unbind(-1)
    return torch.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                        aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz], dim=-1)


def rotation_matrices(q):
    x, y, z, w = q.unbind(-1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=-1).reshape(-1, 3, 3)


def torch_port(est_q, gt_q, out):
    """rmse.py / l1_error.py per distance, rpe_n.py / l1_rpe_n.py over them: (RPE_1, RPE_n, L1RPE_1, L1RPE_n) -> out"""
    est, gt = rotation_matrices(est_q), rotation_matrices(gt_q)
    L = est.shape[0]
    rmse, l1 = torch.empty(L - 1, **f64), torch.empty(L - 1, **f64)
    for d in range(1, L):
        rel_gt = torch.matmul(gt[:-d].transpose(1, 2), gt[d:])
        rel_est_inv = torch.matmul(est[d:].transpose(1, 2), est[:-d])
        rel = torch.matmul(rel_est_inv, rel_gt)
        angles = torch.arccos((rel.diagonal(dim1=1, dim2=2).sum(dim=1) - 1.0) / 2.0)
        rmse[d - 1] = torch.sqrt(torch.square(angles).sum() / (L - d))
        l1[d - 1] = angles.mean()
    out[0], out[1], out[2], out[3] = rmse[0], rmse.sum() / L, l1[0], l1.sum() / L


gen = torch.Generator(device=dev)
gen.manual_seed(11)
n = sum(LENGTHS)
offsets = torch.as_tensor(np.concatenate([[0], np.cumsum(LENGTHS)]), dtype=torch.int64, device=dev)
gt_rel_q, gt_rel_t = steps(n, 0.02, gen)
noise_q, _ = steps(n, 5e-3, gen)
est_rel_q = qmul(gt_rel_q, noise_q).contiguous()
est_rel_t = gt_rel_t + 0.05 * torch.randn((n, 3), generator=gen, **f64)
est_rel_t = (est_rel_t / est_rel_t.norm(dim=1, keepdim=True)).contiguous()
gt = compose_trajectory(offsets, gt_rel_q, gt_rel_t)
est = compose_trajectory(offsets, est_rel_q, est_rel_t)
L0 = LENGTHS[0]
off1 = torch.as_tensor([0, L0], dtype=torch.int64, device=dev)
est1_q, est1_p, gt1_q, gt1_p = (a[:L0].contiguous() for a in (est.q, est.p, gt.q, gt.p))
out_all, out_one = new_trajectory_metrics(len(LENGTHS), n, True, dev), new_trajectory_metrics(1, L0, True, dev)
out_c = Trajectory(torch.empty_like(est.q), torch.empty_like(est.p), torch.empty_like(est.valid))
port = torch.empty(4, **f64)
flat_in, flat_out = torch.empty(7 * n, **f64), torch.empty(7 * n, **f64)
byte_in, byte_out = (torch.zeros(n, dtype=torch.uint8, device=dev) for _ in range(2))


def copy():
    flat_out.copy_(flat_in)
    byte_out.copy_(byte_in)


arms = {"M_metrics_eleven_sequences": lambda: trajectory_metrics(offsets, est.q, gt.q, est.p, gt.p, out=out_all),
        "M1_metrics_4541": lambda: trajectory_metrics(off1, est1_q, gt1_q, est1_p, gt1_p, out=out_one),
        "C_compose_eleven_sequences": lambda: compose_trajectory(offsets, est_rel_q, est_rel_t, out=out_c),
        "Cc_copy_of_the_same_bytes": copy}
for fn in arms.values():
    for _ in range(3):
        fn()
torch_port(est1_q, gt1_q, port)
torch.cuda.synchronize()
agree = (port - out_one.metrics[0, :4]).abs().tolist()
ms = {k: [] for k in arms}
ms["T1_torch_port_4541"] = []
for r in range(REPEATS):
    for k, fn in arms.items():
        ms[k].append(timed(fn))
    if r < 3:
        ms["T1_torch_port_4541"].append(timed(lambda: torch_port(est1_q, gt1_q, port), inner=1))
med = {k: float(np.median(v)) for k, v in ms.items()}
pairs_all, pairs_one = sum(L * (L - 1) // 2 for L in LENGTHS), L0 * (L0 - 1) // 2
rate = lambda pairs, k: pairs / (med[k] * 1e-3)
moved = 2 * 7 * 8 * n + 2 * n
out = {"repeats": REPEATS, "calls_per_timing": INNER, "lengths": LENGTHS, "rows": n,
       "timing": "device events around back-to-back calls, arms alternating after warm-up; median (min - max) over the "
                 "repeats; the torch port: one call a timing, three repeats",
       "lib_sha256": hashlib.sha256(open(capi.LIB_PATH, "rb").read()).hexdigest(),
       **{k: stat(v) for k, v in ms.items()},
       "frame_pairs": {"eleven_sequences": pairs_all, "4541": pairs_one},
       "pairs_per_s": {"M_metrics_eleven_sequences": rate(pairs_all, "M_metrics_eleven_sequences"),
                       "M1_metrics_4541": rate(pairs_one, "M1_metrics_4541"), "T1_torch_port_4541": rate(pairs_one, "T1_torch_port_4541")},
       "fp64_instructions_per_pair": FP64_PER_PAIR,
       "fp64_instructions_per_pair_with_asin_branch_above_half": FP64_PER_PAIR_LARGE_ANGLES,
       "largest_angle_rad": {"rmse_d_max": float(out_all.rmse_d.max()), "angle1_max": float(out_all.angle1.max())},
       "fraction_of_fp64_vector_rate_datasheet": {
           k: rate(p, k) * FP64_PER_PAIR / FP64_LANE_INSTRUCTIONS_PER_S
           for k, p in (("M_metrics_eleven_sequences", pairs_all), ("M1_metrics_4541", pairs_one))},
       "fraction_if_every_wavefront_took_asins_branch_above_half": {
           k: rate(p, k) * FP64_PER_PAIR_LARGE_ANGLES / FP64_LANE_INSTRUCTIONS_PER_S
           for k, p in (("M_metrics_eleven_sequences", pairs_all), ("M1_metrics_4541", pairs_one))},
       "torch_port_over_M1": med["T1_torch_port_4541"] / med["M1_metrics_4541"],
       "torch_port_minus_device_abs": dict(zip(("RPE_1", "RPE_n", "L1RPE_1", "L1RPE_n"), agree)),
       "compose_over_copy": med["C_compose_eleven_sequences"] / med["Cc_copy_of_the_same_bytes"],
       "compose_bytes_read_plus_written": moved,
       "measured": ["both calls on the eleven KITTI-like lengths", "the metrics of the 4541-frame sequence alone",
                    "the torch port of the reference for that sequence on the same GPU", "a copy of compose's bytes"],
       "not_measured": ["the error rotations staged in LDS per wavefront (not built: a diagonal reads each row once per "
                        "wavefront, and the rows come from L2)", "the three launches of the metrics call one by one",
                        "HOST space", "the clock the device held (the roof is the datasheet's peak clock)"]}
print(json.dumps(out), flush=True)
if OUT:
    with open(OUT, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
