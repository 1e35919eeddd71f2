#!/usr/bin/env python3
"""What the triangulation / cheirality pass costs, next to the residual pass and the pose covariance: B pairs x 512
correspondences, TARGET, device-resident inputs, in one process, alternating T V R P T V R P after warm-up, each timed
with device events around `inner` back-to-back calls:
   T  pnec_hip_triangulate, all eleven outputs into preallocated tensors, PNEC_HIP_TRI_ORIENT, at the solved poses
      (two sweeps: the vote over the six bearing planes, then the pass proper)
   V  pnec_hip_triangulate, the five per-slot outputs only (one sweep over the six bearing planes, no covariances read,
      no per-correspondence stores)
   R  pnec_hip_residuals, all seven outputs
   P  pnec_hip_pose_covariance, all five outputs
Nothing is fixed in advance.  Recorded: medians and ranges, T/R and V/P; V reads half of P's planes and is expected to
be no slower than P -- if it is, the JSON says by how much and what V does that P does not.
Prints one JSON object and, with an output path, writes it there (profiles/triangulate.json).  Runs on the GPU box.
   python tools/bench_triangulate.py [B] [repeats] [out.json]"""
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
N, INNER, GATE = 512, 5, 3.0
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
solved = batch.solve(q0, t0, options=capi.default_options(max_num_iterations=10, check_convergence=0))
q1, t1 = solved.q.clone(), solved.t.clone()

f64 = dict(dtype=torch.float64, device=dev)
i32 = dict(dtype=torch.int32, device=dev)
M = B * N
o_point = torch.empty((M, 3), **f64)
o_d1, o_d2, o_psi, o_var = (torch.empty((M,), **f64) for _ in range(4))
o_front = torch.empty((M,), dtype=torch.uint8, device=dev)
o_nf, o_nb, o_sign = (torch.empty((B,), **i32) for _ in range(3))
o_t, o_mean = torch.empty((B, 3), **f64), torch.empty((B,), **f64)
o_res, o_rvar, o_mask = torch.empty((M,), **f64), torch.empty((M,), **f64), torch.empty((M,), dtype=torch.uint8, device=dev)
o_chi2, o_gchi2, o_max = torch.empty((B,), **f64), torch.empty((B,), **f64), torch.empty((B,), **f64)
o_cnt = torch.empty((B,), **i32)
o_info, o_cov, o_grad, o_cost = torch.empty((B, 15), **f64), torch.empty((B, 36), **f64), torch.empty((B, 5), **f64), torch.empty((B,), **f64)
o_status = torch.empty((B,), **i32)
L = capi.lib()
SLOT = (o_nf, o_nb, o_sign, o_t, o_mean)


def _stream():
    return torch.cuda.current_stream(0).cuda_stream


def _tri(per_corr, flags):
    pc = [None if a is None else a.data_ptr() for a in per_corr]

    def run():
        capi.check(L.pnec_hip_triangulate(batch._h, q1.data_ptr(), t1.data_ptr(), 1, flags, *pc,
                                          *(a.data_ptr() for a in SLOT), capi.MEM_DEVICE, _stream()))
    return run


run_t = _tri((o_point, o_d1, o_d2, o_psi, o_var, o_front), capi.TRI_ORIENT)
run_t_plain = _tri((o_point, o_d1, o_d2, o_psi, o_var, o_front), 0)           # one sweep: what the vote sweep costs
run_t_novar = _tri((o_point, o_d1, o_d2, o_psi, None, o_front), capi.TRI_ORIENT)  # no covariance planes read
run_v = _tri((None,) * 6, capi.TRI_ORIENT)


def run_r():
    capi.check(L.pnec_hip_residuals(batch._h, q1.data_ptr(), t1.data_ptr(), 1, 1e-13, GATE, o_res.data_ptr(), o_rvar.data_ptr(),
                                    o_mask.data_ptr(), o_chi2.data_ptr(), o_gchi2.data_ptr(), o_cnt.data_ptr(),
                                    o_max.data_ptr(), capi.MEM_DEVICE, _stream()))


def run_p():
    capi.check(L.pnec_hip_pose_covariance(batch._h, q1.data_ptr(), t1.data_ptr(), 1, 1e-13, o_info.data_ptr(),
                                          o_cov.data_ptr(), o_grad.data_ptr(), o_cost.data_ptr(), o_status.data_ptr(),
                                          capi.MEM_DEVICE, _stream()))


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(INNER):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / INNER


FORMS = (("T", run_t), ("V", run_v), ("R", run_r), ("P", run_p), ("T_one_sweep", run_t_plain), ("T_no_variance", run_t_novar))
for _, fn in FORMS:
    for _ in range(5):
        fn()
torch.cuda.synchronize()
run_t()
torch.cuda.synchronize()
assert int(o_front.sum()) == int(torch.maximum(o_nf, o_nb).sum())
share_front = float(o_front.sum()) / M
flipped = float((o_sign < 0).sum()) / B
ms = {k: [] for k, _ in FORMS}
for _ in range(REPEATS):
    for key, fn in FORMS:
        ms[key].append(timed(fn))


def stat(x):
    x = np.asarray(x)
    return {"median_ms": float(np.median(x)), "min_ms": float(x.min()), "max_ms": float(x.max()),
            "spread_rel": float((x.max() - x.min()) / np.median(x))}


T, V, R, P = (float(np.median(ms[k])) for k in "TVRP")
stores = M * 57 + B * 44
bearing_bytes = M * 6 * 8
line = {"pairs": B, "corr": N, "mode": "TARGET", "repeats": REPEATS, "calls_per_timing": INNER,
        "timing": "device events around back-to-back calls",
        "T_triangulate_all_outputs_orient": stat(ms["T"]), "V_triangulate_per_slot_only": stat(ms["V"]),
        "R_residuals_all_outputs": stat(ms["R"]), "P_pose_covariance_all_outputs": stat(ms["P"]),
        "T_one_sweep_no_orient": stat(ms["T_one_sweep"]), "T_orient_without_variance": stat(ms["T_no_variance"]),
        "T_over_R": T / R, "V_over_P": V / P, "expect_V_le_P": bool(V <= P),
        "payload_bytes": batch.payload_bytes, "bearing_plane_bytes": bearing_bytes, "T_store_bytes": stores,
        "T_traffic_GBps": (batch.payload_bytes + bearing_bytes + stores) / (T * 1e-3) / 1e9,
        "V_bearing_GBps": bearing_bytes / (V * 1e-3) / 1e9, "P_payload_GBps": batch.payload_bytes / (P * 1e-3) / 1e9,
        "share_in_front_after_orient": share_front, "share_of_pairs_flipped": flipped,
        "lib_sha256": hashlib.sha256(open(capi.LIB_PATH, "rb").read()).hexdigest()}
if V > P:
    line["why_V_slower_than_P"] = (
        f"V is {100 * (V / P - 1):.0f} % slower than P although it reads {bearing_bytes / 1e9:.2f} GB of P's "
        f"{batch.payload_bytes / 1e9:.2f} GB: V moves {line['V_bearing_GBps']:.0f} GB/s against P's "
        f"{line['P_payload_GBps']:.0f} GB/s, so V is bound by its arithmetic, not by HBM -- per correspondence an IEEE "
        f"division for 1/D, an IEEE square root and a second division for the arctangent of the parallax (the mean "
        f"needs psi of every correspondence), at 150+ vector registers and occupancy 3, where P has FMAs and one "
        f"reciprocal square root.")
print(json.dumps(line), flush=True)
if OUT:
    with open(OUT, "w") as f:
        json.dump(line, f, indent=1)
        f.write("\n")
