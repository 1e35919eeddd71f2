#!/usr/bin/env python3
"""What the RANSAC forms of the essential-matrix baselines cost: pnec_hip_essential_ransac (NISTER, SEVENPT, EIGHTPT)
with the reference's defaults (5000 iterations at most, threshold 1e-6) on batches with 10 % planted outliers, next to two
yardsticks measured in the same run:
   E  pnec_hip_ransac_eigensolver on the same batch (sample of ten, same bounds, identity start rotation)
   S  the batch's total number of attempts times the per-pair time of the existing non-RANSAC call on a B x m batch
      (pnec_hip_essential_minimal on B x 5 / B x 7, pnec_hip_eight_point on B x 8): what the solves alone would cost.
      The ratio of a RANSAC time to S says what the loop, the gathers and the scoring add on top of the solves.
NEC mode, device-resident inputs, one process; after warm-up the arms alternate, each timed with device events around
`inner` back-to-back calls, medians and spreads over repeats, as tools/bench_minimal_solvers.py.  Two batches:
   uniform   B x 512
   kitti     23 190 ragged pairs with the KITTI-like sizes of pnec_amd.simulation (265..700 correspondences)
Scenes as the tests': points in a box in front of both cameras, a rotation of up to 0.1 rad, a unit baseline, noise of
1e-4 on f2, a tenth of the rows' f2 replaced by random directions.  Nothing is fixed in advance.  Also recorded: the
distribution of attempts and iterations per pair, the inlier share, the status counts.
Prints one JSON object and, with an output path, writes it there (profiles/essential_ransac.json).  Runs on the GPU box.
   python tools/bench_essential_ransac.py [B] [repeats] [out.json]"""
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
REPEATS = int(sys.argv[2]) if len(sys.argv) > 2 else 9
OUT = sys.argv[3] if len(sys.argv) > 3 else None
INNER = 3
MAX_ITERATIONS, THRESHOLD, SEED = 5000, 1e-6, 1
SHARE, NOISE = 0.10, 1e-4
ALGS = (("nister", capi.EM_NISTER, 5), ("sevenpt", capi.EM_SEVENPT, 7), ("eightpt", capi.EM_EIGHTPT, 8))
dev = torch.device("cuda:0")
L = capi.lib()
f64 = dict(dtype=torch.float64, device=dev)
i32 = dict(dtype=torch.int32, device=dev)


def _stream():
    return torch.cuda.current_stream(0).cuda_stream


def scenes(counts, seed, share):
    """(offsets, f1 [M,3], f2 [M,3]) of one scene per pair, numpy."""
    rng = np.random.default_rng(seed)
    counts = np.asarray(counts, dtype=np.int64)
    P, M = len(counts), int(counts.sum())
    pid = np.repeat(np.arange(P), counts)
    k = rng.normal(size=(P, 3))
    k /= np.linalg.norm(k, axis=1)[:, None]
    th = rng.uniform(0.0, 0.1, size=P)
    K = np.zeros((P, 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -k[:, 2], k[:, 1], k[:, 2], -k[:, 0], -k[:, 1], k[:, 0]
    R = np.eye(3)[None] + np.sin(th)[:, None, None] * K + (1.0 - np.cos(th))[:, None, None] * (K @ K)
    t = rng.normal(size=(P, 3))
    t /= np.linalg.norm(t, axis=1)[:, None]
    x1 = np.column_stack([rng.uniform(-2.0, 2.0, M), rng.uniform(-2.0, 2.0, M), rng.uniform(4.0, 8.0, M)])
    d = x1 - t[pid]
    x2 = np.stack([sum(d[:, j] * R[pid, j, c] for j in range(3)) for c in range(3)], axis=1)   # (x1 - t) R, row by row
    f1 = x1 / np.linalg.norm(x1, axis=1)[:, None]
    f2 = x2 / np.linalg.norm(x2, axis=1)[:, None] + rng.normal(scale=NOISE, size=(M, 3))
    out = rng.random(M) < share
    f2[out] = rng.normal(size=(int(out.sum()), 3))
    f2 /= np.linalg.norm(f2, axis=1)[:, None]
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), f1, f2


def batch_of(counts, seed, share=SHARE):
    off, f1, f2 = scenes(counts, seed, share)
    b = Batch(capi.MODE_NEC, off)
    b.fill(torch.as_tensor(f1, device=dev), torch.as_tensor(f2, device=dev))
    return b


def kitti_counts():
    offsets = sim.generate_kitti_like(23190, mean_corr=500, seed=11, device=dev)[0]
    off = offsets.cpu().numpy() if hasattr(offsets, "cpu") else np.asarray(offsets)
    return np.diff(off)


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


def alternate(forms):
    for _, fn in forms:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k, _ in forms}
    for _ in range(REPEATS):
        for key, fn in forms:
            ms[key].append(timed(fn))
    return {k: stat(v) for k, v in ms.items()}


def quantiles(x):
    x = np.asarray(x, dtype=np.float64)
    return {"mean": float(x.mean()), "p50": float(np.median(x)), "p90": float(np.quantile(x, 0.9)),
            "p99": float(np.quantile(x, 0.99)), "max": float(x.max()), "total": float(x.sum())}


def solve_yardstick():
    """ms per pair of the non-RANSAC calls on B x m batches without outliers."""
    out, forms, keep = {}, [], []
    for name, alg, m in ALGS:
        b = batch_of(np.full(B, m), 100 + m, share=0.0)
        P = b.n_pairs
        o = [torch.empty((P, w), **f64) for w in (4, 3, 9, 3)] + [torch.empty((P,), **i32)]
        if alg == capi.EM_EIGHTPT:
            ptr = [o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr(), None, None, None, o[4].data_ptr()]
            fn = lambda b=b, ptr=ptr: capi.check(L.pnec_hip_eight_point(b._h, 0, *ptr, capi.MEM_DEVICE, _stream()))
        else:
            ptr = [o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr(), None, None, None, None, None,
                   o[4].data_ptr()]
            fn = lambda b=b, ptr=ptr, alg=alg: capi.check(
                L.pnec_hip_essential_minimal(b._h, alg, 0, *ptr, capi.MEM_DEVICE, _stream()))
        forms.append((name, fn))
        keep.append((b, o))
    st = alternate(forms)
    for (name, _, m), (b, o) in zip(ALGS, keep):
        status = o[4].cpu().numpy()
        out[name] = dict(st[name], batch=f"{B} x {m}", ok=int((status == 0).sum()),
                         us_per_pair=st[name]["median_ms"] * 1e3 / B)
        b.close()
    return out


def measure(name, b, per_solve):
    P, M = b.n_pairs, int(b.num_correspondences)
    o = [torch.empty((P, w), **f64) for w in (4, 3, 9, 3)] + [torch.empty((max(M, 1),), dtype=torch.uint8, device=dev)] + \
        [torch.empty((P,), **i32) for _ in range(5)]
    ptr = [a.data_ptr() for a in o]
    q0 = torch.zeros((P, 4), **f64)
    q0[:, 3] = 1.0
    e = [torch.empty((P, 4), **f64), torch.empty((P, 3), **f64), torch.empty((max(M, 1),), dtype=torch.uint8, device=dev),
         torch.empty((P,), **i32), torch.empty((P,), **i32)]
    forms = [(n, lambda alg=alg: capi.check(L.pnec_hip_essential_ransac(
        b._h, alg, SEED, 0, MAX_ITERATIONS, THRESHOLD, *ptr, capi.MEM_DEVICE, _stream()))) for n, alg, _ in ALGS]
    forms.append(("eigensolver", lambda: capi.check(L.pnec_hip_ransac_eigensolver(
        b._h, q0.data_ptr(), SEED, MAX_ITERATIONS, 10, THRESHOLD, *[a.data_ptr() for a in e], capi.MEM_DEVICE, _stream()))))
    seen = {}
    for (n, alg, _), (_, fn) in zip(ALGS, forms):
        fn()
        torch.cuda.synchronize()
        status, att, it, cnt = (o[k].cpu().numpy() for k in (9, 7, 6, 5))
        seen[n] = {"status": {capi.ER_NAMES[k]: int((status == k).sum()) for k in capi.ER_NAMES},
                   "attempts": quantiles(att), "iterations": quantiles(it), "inlier_share": float(cnt.sum()) / max(M, 1)}
    st = alternate(forms)
    out = {"batch": name, "pairs": P, "correspondences": M, "eigensolver_ransac": st["eigensolver"]}
    for n, _, _ in ALGS:
        solves = seen[n]["attempts"]["total"] * per_solve[n]["us_per_pair"] * 1e-3
        out[n] = dict(st[n], counts=seen[n], over_eigensolver_ransac=st[n]["median_ms"] / st["eigensolver"]["median_ms"],
                      solves_alone_ms=solves, over_solves_alone=st[n]["median_ms"] / solves,
                      us_per_attempt=st[n]["median_ms"] * 1e3 / seen[n]["attempts"]["total"])
    return out


out = {"repeats": REPEATS, "calls_per_timing": INNER, "mode": "NEC", "max_iterations": MAX_ITERATIONS,
       "threshold": THRESHOLD, "planted_outliers": SHARE, "noise": NOISE,
       "timing": "device events around back-to-back calls, arms alternating nister sevenpt eightpt eigensolver",
       "lib_sha256": hashlib.sha256(open(capi.LIB_PATH, "rb").read()).hexdigest()}
out["solves"] = solve_yardstick()
print("solves", json.dumps(out["solves"]), flush=True)
for key, counts, name in (("uniform", lambda: np.full(B, 512), f"{B} x 512"),
                          ("kitti", kitti_counts, "23 190 ragged pairs, KITTI-like sizes")):
    b = batch_of(counts(), 7 if key == "uniform" else 9)
    out[key] = measure(name, b, out["solves"])
    b.close()
    print(key, json.dumps(out[key]), flush=True)
print(json.dumps(out), flush=True)
if OUT:
    with open(OUT, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
