#!/usr/bin/env python3
"""What the residual / chi-square gate pass costs, next to the pose covariance and the solve: B pairs x 512
correspondences, TARGET, device-resident inputs, in one process, alternating R S P B R S P B after warm-up, each timed with
device events around `inner` back-to-back calls:
   R  pnec_hip_residuals, all seven outputs into preallocated tensors, at the solved poses, gate 3
      (R_py: the same through Batch.residuals, which allocates its outputs)
   S  pnec_hip_residuals, the four per-slot summaries only (no per-correspondence stores)
   P  pnec_hip_pose_covariance, all five outputs
   B  pnec_hip_solve with max_num_iterations = 1
Nothing is fixed in advance; the expectation recorded against is "R no slower than P in this same run" (R does strictly
less arithmetic and adds 17 B of stores per correspondence to 96 B of loads).
Prints one JSON object and, with an output path, writes it there (profiles/residuals.json).  Runs on the GPU box.
   python tools/bench_residuals.py [B] [repeats] [out.json]"""
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
one = capi.default_options(max_num_iterations=1, check_convergence=0)
ten = capi.default_options(max_num_iterations=10, check_convergence=0)
solved = batch.solve(q0, t0, options=ten)
q1, t1 = solved.q.clone(), solved.t.clone()
out_b = None

f64 = dict(dtype=torch.float64, device=dev)
M = B * N
o_res, o_var, o_mask = torch.empty((M,), **f64), torch.empty((M,), **f64), torch.empty((M,), dtype=torch.uint8, device=dev)
o_chi2, o_gchi2, o_max = torch.empty((B,), **f64), torch.empty((B,), **f64), torch.empty((B,), **f64)
o_cnt = torch.empty((B,), dtype=torch.int32, device=dev)
o_info, o_cov, o_grad, o_cost = torch.empty((B, 15), **f64), torch.empty((B, 36), **f64), torch.empty((B, 5), **f64), torch.empty((B,), **f64)
o_status = torch.empty((B,), dtype=torch.int32, device=dev)
L = capi.lib()


def run_r():
    capi.check(L.pnec_hip_residuals(batch._h, q1.data_ptr(), t1.data_ptr(), 1, 1e-13, GATE, o_res.data_ptr(), o_var.data_ptr(),
                                    o_mask.data_ptr(), o_chi2.data_ptr(), o_gchi2.data_ptr(), o_cnt.data_ptr(),
                                    o_max.data_ptr(), capi.MEM_DEVICE, torch.cuda.current_stream(0).cuda_stream))


def run_s():
    capi.check(L.pnec_hip_residuals(batch._h, q1.data_ptr(), t1.data_ptr(), 1, 1e-13, GATE, None, None, None,
                                    o_chi2.data_ptr(), o_gchi2.data_ptr(), o_cnt.data_ptr(), o_max.data_ptr(),
                                    capi.MEM_DEVICE, torch.cuda.current_stream(0).cuda_stream))


def _one(res, var, mask):
    """the summaries + ONE of the per-correspondence arrays: what each store stream costs on top of S"""
    def run():
        capi.check(L.pnec_hip_residuals(batch._h, q1.data_ptr(), t1.data_ptr(), 1, 1e-13, GATE, res, var, mask,
                                        o_chi2.data_ptr(), o_gchi2.data_ptr(), o_cnt.data_ptr(), o_max.data_ptr(),
                                        capi.MEM_DEVICE, torch.cuda.current_stream(0).cuda_stream))
    return run


run_sr, run_sv, run_sm = _one(o_res.data_ptr(), None, None), _one(None, o_var.data_ptr(), None), _one(None, None, o_mask.data_ptr())
run_srv = _one(o_res.data_ptr(), o_var.data_ptr(), None)


def run_r_py():
    return batch.residuals(q1, t1, gate=GATE)


def run_p():
    capi.check(L.pnec_hip_pose_covariance(batch._h, q1.data_ptr(), t1.data_ptr(), 1, 1e-13, o_info.data_ptr(),
                                          o_cov.data_ptr(), o_grad.data_ptr(), o_cost.data_ptr(), o_status.data_ptr(),
                                          capi.MEM_DEVICE, torch.cuda.current_stream(0).cuda_stream))


def run_b():
    global out_b
    out_b = batch.solve(q0, t0, options=one, out=out_b)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(INNER):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / INNER


for fn in (run_r, run_s, run_sr, run_sv, run_sm, run_srv, run_r_py, run_p, run_b):
    for _ in range(5):
        fn()
torch.cuda.synchronize()
rep = run_r_py()
run_r(), run_p()
torch.cuda.synchronize()
assert torch.equal(rep.residual, o_res) and torch.equal(rep.mask, o_mask) and torch.equal(rep.chi2, o_chi2)
assert bool(torch.isfinite(o_chi2).all()) and int(o_cnt.sum()) == int(o_mask.sum())
inside = float(o_mask.sum()) / M
ms = {k: [] for k in ("R", "S", "P", "B", "R_py", "S_res", "S_var", "S_mask", "S_res_var")}
for _ in range(REPEATS):
    for key, fn in (("R", run_r), ("S", run_s), ("P", run_p), ("B", run_b), ("R_py", run_r_py), ("S_res", run_sr),
                    ("S_var", run_sv), ("S_mask", run_sm), ("S_res_var", run_srv)):
        ms[key].append(timed(fn))


def stat(x):
    x = np.asarray(x)
    return {"median_ms": float(np.median(x)), "min_ms": float(x.min()), "max_ms": float(x.max()),
            "spread_rel": float((x.max() - x.min()) / np.median(x))}


R, S, P, Bm = (float(np.median(ms[k])) for k in "RSPB")
stores = M * 17 + B * 28
line = {"pairs": B, "corr": N, "mode": "TARGET", "gate": GATE, "repeats": REPEATS, "calls_per_timing": INNER,
        "timing": "device events around back-to-back calls",
        "R_residuals_all_outputs": stat(ms["R"]), "S_residuals_summaries_only": stat(ms["S"]),
        "R_py_batch_method": stat(ms["R_py"]), "P_pose_covariance_all_outputs": stat(ms["P"]),
        "B_solve_1_iteration": stat(ms["B"]),
        "store_streams_on_top_of_S": {"summaries_plus_residual_8B": stat(ms["S_res"]), "summaries_plus_variance_8B": stat(ms["S_var"]),
                                      "summaries_plus_mask_1B": stat(ms["S_mask"]),
                                      "summaries_plus_residual_and_variance_16B": stat(ms["S_res_var"])},
        "R_over_P": R / P, "S_over_P": S / P, "R_over_B": R / Bm,
        "expect_R_le_P": bool(R <= P),
        "payload_bytes": batch.payload_bytes, "R_store_bytes": stores,
        "R_traffic_GBps": (batch.payload_bytes + stores) / (R * 1e-3) / 1e9,
        "S_payload_GBps": batch.payload_bytes / (S * 1e-3) / 1e9,
        "share_inside_gate": inside, "median_variance_factor": float(torch.median(o_chi2 / (N - 5))),
        "lib_sha256": hashlib.sha256(open(capi.LIB_PATH, "rb").read()).hexdigest()}
if R > P:
    med = lambda k: float(np.median(ms[k]))
    bytes_only = S * (batch.payload_bytes + stores) / batch.payload_bytes
    line["why_R_slower_than_P"] = (
        f"R is {100 * (R / P - 1):.0f} % slower than P.  P and S (this pass without per-correspondence stores, {S:.3f} ms) "
        f"both run at the rate of the {batch.payload_bytes / 1e9:.2f} GB payload read, so nothing that also writes can match "
        f"P: R writes {stores / 1e9:.2f} GB more, which at S's rate would be {bytes_only:.3f} ms "
        f"(+{100 * (bytes_only / S - 1):.0f} %).  Measured per store stream on top of S, same run: residual (8 B) "
        f"+{med('S_res') - S:.3f} ms, variance (8 B) +{med('S_var') - S:.3f} ms, mask (1 B) +{med('S_mask') - S:.3f} ms, "
        f"residual and variance together +{med('S_res_var') - S:.3f} ms, all three +{R - S:.3f} ms.")
print(json.dumps(line), flush=True)
if OUT:
    with open(OUT, "w") as f:
        json.dump(line, f, indent=1)
        f.write("\n")
