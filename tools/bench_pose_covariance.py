#!/usr/bin/env python3
"""What the pose covariance costs, next to the solve: B pairs x 512 correspondences, TARGET, device-resident inputs, in
one process, alternating A B C A B C after warm-up, each timed with device events around `inner` back-to-back calls:
   A  pnec_hip_pose_covariance, all five outputs into preallocated tensors, at the solved poses
      (A_py: the same through Batch.pose_covariance, which allocates its outputs and expands the information to 5x5)
   B  pnec_hip_solve with max_num_iterations = 1 (the same payload read once, two evaluation passes and a step)
   C  the headline launch: pnec_hip_solve, 10 fixed iterations
Prints one JSON object and, with an output path, writes it there (profiles/pose_covariance.json).  Runs on the GPU box.
   python tools/bench_pose_covariance.py [B] [repeats] [out.json]"""
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from pnec_amd import Batch, capi
from pnec_amd import simulation as sim

B = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000
REPEATS = int(sys.argv[2]) if len(sys.argv) > 2 else 15
OUT = sys.argv[3] if len(sys.argv) > 3 else None
N, INNER = 512, 5
dev = torch.device("cuda:0")

batch = Batch.uniform(capi.MODE_TARGET, B, N)
qs, ts = [], []
for c0 in range(0, B, 10_000):
    m = min(10_000, B - c0)
    g = sim.generate(m, N, seed=1 + c0, device=dev)
    batch.fill(g.bvs1.reshape(-1, 3), g.bvs2.reshape(-1, 3), g.covs2.reshape(-1, 3, 3), first_pair=c0, n_pairs=m)
    qs.append(g.init_q), ts.append(g.init_t)
    del g
q0, t0 = torch.cat(qs), torch.cat(ts)
one = capi.default_options(max_num_iterations=1, check_convergence=0)
ten = capi.default_options(max_num_iterations=10, check_convergence=0)
solved = batch.solve(q0, t0, options=ten)
q1, t1 = solved.q.clone(), solved.t.clone()
out_b = out_c = None


f64 = dict(dtype=torch.float64, device=dev)
o_info, o_cov, o_grad, o_cost = torch.empty((B, 15), **f64), torch.empty((B, 36), **f64), torch.empty((B, 5), **f64), torch.empty((B,), **f64)
o_status = torch.empty((B,), dtype=torch.int32, device=dev)


def run_a():
    capi.check(capi.lib().pnec_hip_pose_covariance(batch._h, q1.data_ptr(), t1.data_ptr(), 1, 1e-13, o_info.data_ptr(),
                                                   o_cov.data_ptr(), o_grad.data_ptr(), o_cost.data_ptr(), o_status.data_ptr(),
                                                   capi.MEM_DEVICE, torch.cuda.current_stream(0).cuda_stream))


def run_a_py():
    return batch.pose_covariance(q1, t1)


def run_b():
    global out_b
    out_b = batch.solve(q0, t0, options=one, out=out_b)


def run_c():
    global out_c
    out_c = batch.solve(q0, t0, options=ten, out=out_c)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(INNER):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / INNER


for fn in (run_a, run_a_py, run_b, run_c):
    for _ in range(5):
        fn()
torch.cuda.synchronize()
pc = run_a_py()
assert int((pc.status != 0).sum()) == 0 and bool(torch.isfinite(pc.cov).all())
assert torch.equal(pc.cov.reshape(B, 36), o_cov) and int((o_status != 0).sum()) == 0
ms = {"A": [], "B": [], "C": [], "A_py": []}
for _ in range(REPEATS):
    for key, fn in (("A", run_a), ("B", run_b), ("C", run_c), ("A_py", run_a_py)):
        ms[key].append(timed(fn))


def stat(x):
    x = np.asarray(x)
    return {"median_ms": float(np.median(x)), "min_ms": float(x.min()), "max_ms": float(x.max()),
            "spread_rel": float((x.max() - x.min()) / np.median(x))}


A, Bm, Cm = (float(np.median(ms[k])) for k in "ABC")
line = {"pairs": B, "corr": N, "mode": "TARGET", "repeats": REPEATS, "calls_per_timing": INNER,
        "timing": "device events around back-to-back calls",
        "A_pose_covariance_all_outputs": stat(ms["A"]), "A_py_batch_method": stat(ms["A_py"]), "B_solve_1_iteration": stat(ms["B"]),
        "C_solve_10_iterations": stat(ms["C"]), "A_over_B": A / Bm, "A_over_C": A / Cm,
        "accept_A_le_1p1_B": bool(A <= 1.1 * Bm),
        "payload_bytes": batch.payload_bytes, "A_payload_GBps": batch.payload_bytes / (A * 1e-3) / 1e9,
        "launch_10_iterations": batch.describe_launch(ten),
        "lib_sha256": hashlib.sha256(open(capi.LIB_PATH, "rb").read()).hexdigest()}
print(json.dumps(line), flush=True)
if OUT:
    with open(OUT, "w") as f:
        json.dump(line, f, indent=1)
        f.write("\n")
