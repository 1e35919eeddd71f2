#!/usr/bin/env python3
"""What the minimal solvers cost: pnec_hip_essential_minimal (NISTER, SEVENPT) next to pnec_hip_eight_point on the same
batch in the same run.  NEC mode, device-resident inputs, one process; after warm-up the arms alternate 5 7 8 5 7 8 ...,
each timed with device events around `inner` back-to-back calls, medians over repeats:
   5  pnec_hip_essential_minimal, PNEC_HIP_EM_NISTER, all ten outputs into preallocated tensors, the sample of eight
   7  the same with PNEC_HIP_EM_SEVENPT, the sample of nine
   8  pnec_hip_eight_point, all eight outputs
on four batches:
   uniform   B x 512
   kitti     the 23 190-pair KITTI-like ragged set (265..700 correspondences)
   fixed8    B x 8: the phases whose cost does not depend on N almost alone
   fixed5    B x 5: the same at the five-point's minimal count (the other two arms answer TOO_FEW there: their times are
             those of a kernel that returns after reading one count, recorded for completeness)
Nothing is fixed in advance.  Recorded: medians and ranges, the ratios 5 / 8 and 7 / 8 of the same run, the status and
solution counts, and what the B x 5 batch says about the five-point's own phases: its time less the eight-point's time
on B x 8 (sums of one stride and the Jacobi, which both kernels share) is the algebra -- cubics, elimination, Sturm
chain, bisection, polish, ten decompositions, forty qualities.
Prints one JSON object and, with an output path, writes it there (profiles/minimal_solvers.json).  Runs on the GPU box.
   python tools/bench_minimal_solvers.py [B] [repeats] [out.json]"""
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
    for c0 in range(0, n_pairs, 10_000):
        m = min(10_000, n_pairs - c0)
        g = sim.generate(m, n_corr, seed=seed + c0, device=dev)
        b.fill(g.bvs1.reshape(-1, 3), g.bvs2.reshape(-1, 3), first_pair=c0, n_pairs=m)
        del g
    return b


def kitti():
    offsets, f1, f2 = sim.generate_kitti_like(23190, mean_corr=500, seed=11, device=dev)[:3]
    off = offsets.cpu().numpy() if hasattr(offsets, "cpu") else np.asarray(offsets)
    b = Batch(capi.MODE_NEC, off)
    b.fill(f1, f2)
    return b


def arms(b):
    P, S = b.n_pairs, capi.EM_MAX_SOLUTIONS
    em = [torch.empty((P, w), **f64) for w in (4, 3, 9, 3)] + [
        torch.empty((P,), **f64), torch.empty((P,), **i32), torch.empty((P, S, 9), **f64), torch.empty((P, S, 4), **f64),
        torch.empty((P,), **i32), torch.empty((P,), **i32)]
    ep = [torch.empty((P, w), **f64) for w in (4, 3, 9, 3)] + [torch.empty((P,), **f64), torch.empty((P, 4), **f64),
                                                                 torch.empty((P,), **i32), torch.empty((P,), **i32)]
    em_ptr, ep_ptr = [a.data_ptr() for a in em], [a.data_ptr() for a in ep]

    def run_5():
        capi.check(L.pnec_hip_essential_minimal(b._h, capi.EM_NISTER, 0, *em_ptr, capi.MEM_DEVICE, _stream()))

    def run_7():
        capi.check(L.pnec_hip_essential_minimal(b._h, capi.EM_SEVENPT, 0, *em_ptr, capi.MEM_DEVICE, _stream()))

    def run_8():
        capi.check(L.pnec_hip_eight_point(b._h, 0, *ep_ptr, capi.MEM_DEVICE, _stream()))

    return (("5", run_5), ("7", run_7), ("8", run_8)), em, ep


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


def counts(forms, em, ep):
    out = {}
    for key, fn in forms:
        fn()
        torch.cuda.synchronize()
        o, names = (ep, capi.EP_NAMES) if key == "8" else (em, capi.EM_NAMES)
        status = o[-1].cpu().numpy()
        out[key] = {"status": {names[k]: int((status == k).sum()) for k in names}}
        if key != "8":
            n = em[5].cpu().numpy()
            out[key]["n_solutions"] = {str(k): int((n == k).sum()) for k in range(capi.EM_MAX_SOLUTIONS + 1) if (n == k).any()}
    return out


def measure(name, b):
    forms, em, ep = arms(b)
    for _, fn in forms:
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    seen = counts(forms, em, ep)
    ms = {k: [] for k, _ in forms}
    for _ in range(REPEATS):
        for key, fn in forms:
            ms[key].append(timed(fn))
    t5, t7, t8 = (float(np.median(ms[k])) for k in "578")
    return {"batch": name, "pairs": b.n_pairs, "correspondences": int(b.num_correspondences),
            "5_nister": stat(ms["5"]), "7_sevenpt": stat(ms["7"]), "8_eight_point": stat(ms["8"]),
            "nister_over_eight_point": t5 / t8, "sevenpt_over_eight_point": t7 / t8,
            "nister_us_per_pair": t5 * 1e3 / b.n_pairs, "sevenpt_us_per_pair": t7 * 1e3 / b.n_pairs, "counts": seen}


out = {"repeats": REPEATS, "calls_per_timing": INNER, "mode": "NEC",
       "timing": "device events around back-to-back calls, arms alternating 5 7 8",
       "lib_sha256": hashlib.sha256(open(capi.LIB_PATH, "rb").read()).hexdigest()}
for key, make, name in (("uniform", lambda: uniform(B, 512, 1), f"{B} x 512"),
                        ("kitti", kitti, "23 190 ragged pairs, KITTI-like"),
                        ("fixed8", lambda: uniform(B, 8, 3), f"{B} x 8"),
                        ("fixed5", lambda: uniform(B, 5, 5), f"{B} x 5")):
    b = make()
    out[key] = measure(name, b)
    b.close()
    print(key, json.dumps(out[key]), flush=True)
shared = out["fixed8"]["8_eight_point"]["median_ms"]
five = out["fixed5"]["5_nister"]["median_ms"]
algebra = five - shared
out["nister_algebra_ms"] = algebra
out["nister_algebra_share_of_fixed5"] = algebra / five
out["binding_phase"] = (
    f"{B} x 5 takes the five-point {five:.3f} ms; the eight-point's {B} x 8 -- one stride of sums, the Jacobi, one "
    f"decomposition -- takes {shared:.3f} ms in the same run, so {algebra:.3f} ms ({100 * algebra / five:.0f} %) is what the "
    "eight-point does not have: cubics, elimination, Sturm chain, bisection, polish, ten decompositions, forty "
    "qualities.  " + ("The algebra binds the five-point, not the Jacobi." if algebra > shared else
                      "The Jacobi still binds: the five-point costs the eight-point plus the algebra."))
print(json.dumps(out), flush=True)
if OUT:
    with open(OUT, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
