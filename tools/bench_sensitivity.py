#!/usr/bin/env python3
"""What a backward pass through the refinement costs, next to the forward solve: B pairs x 512 correspondences, TARGET,
device-resident inputs, one process, alternating A B C D after warm-up, each timed with device events around `inner`
back-to-back calls:
   A  pnec_hip_pose_sensitivity at the solved poses, all outputs into preallocated tensors
   B  A with the per-correspondence outputs NULL (the reduce phase and the 5x5 solve alone)
   C  pnec_hip_pose_covariance, all outputs
   D  the headline launch: pnec_hip_solve, 10 fixed iterations
   copy  torch's copy_ of the bytes A moves per correspondence: 96 read (12 planes) + 120 written (3 + 3 + 9 doubles)
A should sit near copy + C; A / D is what a training step costs on top of the forward solve.
Prints one JSON object and, with an output path, writes it there (profiles/sensitivity.json).  Runs on the GPU box.
   python tools/bench_sensitivity.py [B] [repeats] [out.json]"""
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from pnec_amd import Batch, capi
from pnec_amd import simulation as sim

B = int(sys.argv[1]) if len(sys.argv) > 1 else 20_000
REPEATS = int(sys.argv[2]) if len(sys.argv) > 2 else 15
OUT = sys.argv[3] if len(sys.argv) > 3 else None
N, INNER = 512, 5
dev = torch.device("cuda:0")
M = B * N

batch = Batch.uniform(capi.MODE_TARGET, B, N)
qs, ts = [], []
for c0 in range(0, B, 10_000):
    m = min(10_000, B - c0)
    g = sim.generate(m, N, seed=1 + c0, device=dev)
    batch.fill(g.bvs1.reshape(-1, 3), g.bvs2.reshape(-1, 3), g.covs2.reshape(-1, 3, 3), first_pair=c0, n_pairs=m)
    qs.append(g.init_q), ts.append(g.init_t)
    del g
q0, t0 = torch.cat(qs), torch.cat(ts)
ten = capi.default_options(max_num_iterations=10, check_convergence=0)
solved = batch.solve(q0, t0, options=capi.default_options())   # converged poses: where a training step differentiates
q1, t1 = solved.q.clone(), solved.t.clone()

f64 = dict(dtype=torch.float64, device=dev)
gp = torch.randn((B, 6), generator=torch.Generator(device=dev).manual_seed(3), **f64)
g1, g2, gc = torch.empty((M, 3), **f64), torch.empty((M, 3), **f64), torch.empty((M, 9), **f64)
lam, hes, grd, nwt = torch.empty((B, 5), **f64), torch.empty((B, 15), **f64), torch.empty((B, 5), **f64), torch.empty((B, 5), **f64)
status = torch.empty((B,), dtype=torch.int32, device=dev)
o_info, o_cov, o_cost = torch.empty((B, 15), **f64), torch.empty((B, 36), **f64), torch.empty((B,), **f64)
src, dst = torch.empty((M * 12,), **f64), torch.empty((M * 15,), **f64)
out_d = None


def sens(per):
    p = lambda a: a.data_ptr() if per else None
    capi.check(capi.lib().pnec_hip_pose_sensitivity(
        batch._h, q1.data_ptr(), t1.data_ptr(), gp.data_ptr(), 1, 1e-13, 0, p(g1), p(g2), p(gc), None, lam.data_ptr(),
        hes.data_ptr(), grd.data_ptr(), nwt.data_ptr(), status.data_ptr(), capi.MEM_DEVICE, torch.cuda.current_stream(0).cuda_stream))


def run_c():
    capi.check(capi.lib().pnec_hip_pose_covariance(batch._h, q1.data_ptr(), t1.data_ptr(), 1, 1e-13, o_info.data_ptr(),
                                                   o_cov.data_ptr(), grd.data_ptr(), o_cost.data_ptr(), status.data_ptr(),
                                                   capi.MEM_DEVICE, torch.cuda.current_stream(0).cuda_stream))


def run_d():
    global out_d
    out_d = batch.solve(q0, t0, options=ten, out=out_d)


def run_copy():
    dst[:M * 12].copy_(src)      # 96 B read + 96 B written per correspondence ...
    dst[M * 12:].zero_()         # ... + 24 B written: 120 B written in all


runs = (("A", lambda: sens(True)), ("B", lambda: sens(False)), ("C", run_c), ("D", run_d), ("copy", run_copy))


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(INNER):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / INNER


for _, fn in runs:
    for _ in range(3):
        fn()
torch.cuda.synchronize()
sens(True)
torch.cuda.synchronize()
n_ok = int((status == 0).sum())
assert n_ok > 0.99 * B and bool(torch.isfinite(gc.reshape(B, -1)[status == 0]).all()), n_ok
ms = {k: [] for k, _ in runs}
for _ in range(REPEATS):
    for key, fn in runs:
        ms[key].append(timed(fn))


def stat(x):
    x = np.asarray(x)
    return {"median_ms": float(np.median(x)), "min_ms": float(x.min()), "max_ms": float(x.max()),
            "spread_rel": float((x.max() - x.min()) / np.median(x))}


med = {k: float(np.median(v)) for k, v in ms.items()}
line = {"pairs": B, "corr": N, "mode": "TARGET", "repeats": REPEATS, "calls_per_timing": INNER,
        "timing": "device events around back-to-back calls", "slots_ok": n_ok,
        "A_pose_sensitivity_all_outputs": stat(ms["A"]), "B_slot_outputs_only": stat(ms["B"]), "C_pose_covariance": stat(ms["C"]),
        "D_solve_10_iterations": stat(ms["D"]), "copy_216_bytes_per_correspondence": stat(ms["copy"]),
        "A_over_copy_plus_C": med["A"] / (med["copy"] + med["C"]), "A_over_D": med["A"] / med["D"], "B_over_C": med["B"] / med["C"],
        "A_bytes_GBps": 216.0 * M / (med["A"] * 1e-3) / 1e9,
        "lib_sha256": hashlib.sha256(open(capi.LIB_PATH, "rb").read()).hexdigest()}
print(json.dumps(line), flush=True)
if OUT:
    with open(OUT, "w") as f:
        json.dump(line, f, indent=1)
        f.write("\n")
