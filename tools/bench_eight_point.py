#!/usr/bin/env python3
"""What the eight-point baseline costs: pnec_hip_eight_point next to pnec_hip_nec_eigensolver on the same batch and
next to the read-once floor of the six bearing planes.  NEC mode, device-resident inputs, one process; after warm-up the
arms alternate E A N E A N ..., each timed with device events around `inner` back-to-back calls, medians over repeats:
   E  pnec_hip_eight_point, all eight outputs into preallocated tensors, the reference's sample of nine
   A  the same with PNEC_HIP_EP_QUALITY_ALL (a second sweep over the planes, four triangulations per correspondence)
   N  pnec_hip_nec_eigensolver from the simulator's start rotations
on three batches:
   uniform   B x 512
   kitti     the 23 190-pair KITTI-like ragged set (265..700 correspondences)
   fixed     B x 8: the phases whose cost does not depend on N (Jacobi, decomposition, choice) almost alone
Nothing is fixed in advance.  Recorded: medians and ranges, E / N, the bearing planes' bytes over E's time against the
HBM rate, and the share of E on the uniform batch that the fixed phases account for -- which phase binds the kernel.
Prints one JSON object and, with an output path, writes it there (profiles/eight_point.json).  Runs on the GPU box.
   python tools/bench_eight_point.py [B] [repeats] [out.json]"""
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
INNER = 5
dev = torch.device("cuda:0")
L = capi.lib()
f64 = dict(dtype=torch.float64, device=dev)
i32 = dict(dtype=torch.int32, device=dev)


def _stream():
    return torch.cuda.current_stream(0).cuda_stream


def uniform(n_pairs, n_corr, seed):
    b = Batch.uniform(capi.MODE_NEC, n_pairs, n_corr)
    qs = []
    for c0 in range(0, n_pairs, 10_000):
        m = min(10_000, n_pairs - c0)
        g = sim.generate(m, n_corr, seed=seed + c0, device=dev)
        b.fill(g.bvs1.reshape(-1, 3), g.bvs2.reshape(-1, 3), first_pair=c0, n_pairs=m)
        qs.append(g.init_q)
        del g
    return b, torch.cat(qs)


def kitti():
    offsets, f1, f2, _, _, _, q0, _ = sim.generate_kitti_like(23190, mean_corr=500, seed=11, device=dev)
    off = offsets.cpu().numpy() if hasattr(offsets, "cpu") else np.asarray(offsets)
    b = Batch(capi.MODE_NEC, off)
    b.fill(f1, f2)
    return b, q0


def arms(b, q0):
    P = b.n_pairs
    o = [torch.empty((P, w), **f64) for w in (4, 3, 9, 3)] + [torch.empty((P,), **f64), torch.empty((P, 4), **f64),
                                                                torch.empty((P,), **i32), torch.empty((P,), **i32)]
    ptr = [a.data_ptr() for a in o]
    nq, nt = torch.empty((P, 4), **f64), torch.empty((P, 3), **f64)

    def run_e():
        capi.check(L.pnec_hip_eight_point(b._h, 0, *ptr, capi.MEM_DEVICE, _stream()))

    def run_a():
        capi.check(L.pnec_hip_eight_point(b._h, capi.EP_QUALITY_ALL, *ptr, capi.MEM_DEVICE, _stream()))

    def run_n():
        capi.check(L.pnec_hip_nec_eigensolver(b._h, q0.data_ptr(), nq.data_ptr(), nt.data_ptr(), capi.MEM_DEVICE, _stream()))

    return (("E", run_e), ("A", run_a), ("N", run_n)), o


def timed(fn):
    a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(INNER):
        fn()
    z.record()
    z.synchronize()
    return a.elapsed_time(z) / INNER


def stat(x):
    x = np.asarray(x)
    return {"median_ms": float(np.median(x)), "min_ms": float(x.min()), "max_ms": float(x.max()),
            "spread_rel": float((x.max() - x.min()) / np.median(x))}


def measure(name, b, q0):
    forms, o = arms(b, q0)
    for _, fn in forms:
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    forms[0][1]()
    torch.cuda.synchronize()
    status = o[7].cpu().numpy()
    ms = {k: [] for k, _ in forms}
    for _ in range(REPEATS):
        for key, fn in forms:
            ms[key].append(timed(fn))
    n_corr = int(b.num_correspondences)
    plane_bytes = n_corr * 6 * 8
    E, A, N = (float(np.median(ms[k])) for k in "EAN")
    return {"batch": name, "pairs": b.n_pairs, "correspondences": n_corr, "bearing_plane_bytes": plane_bytes,
            "E_eight_point_sample": stat(ms["E"]), "A_eight_point_quality_all": stat(ms["A"]),
            "N_nec_eigensolver": stat(ms["N"]), "E_over_N": E / N, "A_over_E": A / E,
            "E_bearing_GBps": plane_bytes / (E * 1e-3) / 1e9, "E_us_per_pair": E * 1e3 / b.n_pairs,
            "status_counts": {capi.EP_NAMES[k]: int((status == k).sum()) for k in capi.EP_NAMES}}


out = {"repeats": REPEATS, "calls_per_timing": INNER, "mode": "NEC",
       "timing": "device events around back-to-back calls, arms alternating E A N",
       "lib_sha256": hashlib.sha256(open(capi.LIB_PATH, "rb").read()).hexdigest()}
b, q0 = uniform(B, 512, 1)
out["uniform"] = measure(f"{B} x 512", b, q0)
b.close()
b, q0 = kitti()
out["kitti"] = measure("23 190 ragged pairs, KITTI-like", b, q0)
b.close()
b, q0 = uniform(B, 8, 3)
out["fixed"] = measure(f"{B} x 8", b, q0)
b.close()
u, f = out["uniform"], out["fixed"]
share = f["E_eight_point_sample"]["median_ms"] / u["E_eight_point_sample"]["median_ms"]
out["fixed_phases_share_of_uniform_E"] = share
out["binding_phase"] = (
    f"{B} x 8 holds the Jacobi sweeps, the decomposition and the choice almost alone (8 correspondences: one "
    f"iteration of the sums loop); it takes {100 * share:.0f} % of the time of {B} x 512, so "
    + ("the phases that do not depend on N bind the kernel, not the sums and not HBM" if share > 0.5 else
       "the 45-sum pass over the correspondences binds the kernel")
    + f"; the bearing planes stream at {u['E_bearing_GBps']:.0f} GB/s during E.")
print(json.dumps(out), flush=True)
if OUT:
    with open(OUT, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
