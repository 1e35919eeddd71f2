#!/usr/bin/env python3
"""What the relative-scale pass costs, next to the triangulation pass it is built from: B pairs x 512 correspondences,
TARGET, device-resident inputs, stored as ONE batch read as a sequence (prev == cur, prev_pair = k - 1), every
correspondence linked to a random row of the previous pair except 30 % that are not linked; poses = a 10-iteration solve,
translations oriented by pnec_hip_triangulate.  One process, alternating S L V S L V after warm-up, each timed with device
events around `inner` back-to-back calls:
   S  pnec_hip_relative_scale, the per-pair outputs only (scale, n_linked, n_used; the ratios go to the handle's workspace)
   L  pnec_hip_relative_scale, all five outputs
   V  pnec_hip_triangulate, the five per-slot outputs only (one sweep over the six bearing planes, no gather, no
      selection) -- the triangulation kernel is the parent commit's, instruction for instruction
There is no acceptance ratio: S does a gather and three selections that V does not.  Recorded: medians and ranges, S/V
and L/V with the run's spread, and S with the selection's input emptied (min_parallax = 2: no link is used, no round
runs), recorded as measured: on the first run it was SLOWER than S, so it does not split the pass from the rounds.  (The pairs are independent simulator pairs, so the ratios mean nothing here;
the work is that of a real sequence with the same share of used links.)
Prints one JSON object and, with an output path, writes it there (profiles/relative_scale.json).  Runs on the GPU box.
   python tools/bench_relative_scale.py [B] [repeats] [out.json]"""
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
solved = batch.solve(torch.cat(qs), torch.cat(ts), options=capi.default_options(max_num_iterations=10, check_convergence=0))
q1 = solved.q.clone()
t1 = batch.triangulate(q1, solved.t, orient=True).t.clone()      # the sign that puts the structure in front

f64 = dict(dtype=torch.float64, device=dev)
i32 = dict(dtype=torch.int32, device=dev)
M = B * N
gen = torch.Generator(device=dev)
gen.manual_seed(7)
link = torch.argsort(torch.rand((B, N), device=dev, generator=gen), dim=1).to(torch.int32)   # a permutation per pair
link[torch.rand((B, N), device=dev, generator=gen) < 0.3] = -1
link = link.reshape(-1).contiguous()
prev_pair = torch.arange(-1, B - 1, dtype=torch.int64, device=dev)
o_ratio, o_used = torch.empty((M,), **f64), torch.empty((M,), dtype=torch.uint8, device=dev)
o_scale, o_nl, o_nu = torch.empty((B, 3), **f64), torch.empty((B,), **i32), torch.empty((B,), **i32)
o_nf, o_nb, o_sign = (torch.empty((B,), **i32) for _ in range(3))
o_t, o_mean = torch.empty((B, 3), **f64), torch.empty((B,), **f64)
L = capi.lib()


def _stream():
    return torch.cuda.current_stream(0).cuda_stream


def _rs(per_link, min_parallax):
    pl = (o_ratio.data_ptr(), o_used.data_ptr()) if per_link else (None, None)

    def run():
        capi.check(L.pnec_hip_relative_scale(batch._h, batch._h, prev_pair.data_ptr(), link.data_ptr(), q1.data_ptr(),
                                             t1.data_ptr(), q1.data_ptr(), t1.data_ptr(), min_parallax, *pl,
                                             o_scale.data_ptr(), o_nl.data_ptr(), o_nu.data_ptr(), capi.MEM_DEVICE, _stream()))
    return run


run_s, run_l, run_s_empty = _rs(False, 0.0), _rs(True, 0.0), _rs(False, 2.0)


def run_v():
    capi.check(L.pnec_hip_triangulate(batch._h, q1.data_ptr(), t1.data_ptr(), 1, capi.TRI_ORIENT, *(None,) * 6,
                                      o_nf.data_ptr(), o_nb.data_ptr(), o_sign.data_ptr(), o_t.data_ptr(), o_mean.data_ptr(),
                                      capi.MEM_DEVICE, _stream()))


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(INNER):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / INNER


FORMS = (("S", run_s), ("L", run_l), ("V", run_v), ("S_nothing_used", run_s_empty))
for _, fn in FORMS:
    for _ in range(5):
        fn()
torch.cuda.synchronize()
run_l()
torch.cuda.synchronize()
assert int(o_used.sum()) == int(o_nu.sum()) and int(o_nl.sum()) == int((link.reshape(B, N)[1:] >= 0).sum())
share_linked, share_used = float(o_nl.sum()) / M, float(o_nu.sum()) / M
ms = {k: [] for k, _ in FORMS}
for _ in range(REPEATS):
    for key, fn in FORMS:
        ms[key].append(timed(fn))


def stat(x):
    x = np.asarray(x)
    return {"median_ms": float(np.median(x)), "min_ms": float(x.min()), "max_ms": float(x.max()),
            "spread_rel": float((x.max() - x.min()) / np.median(x))}


S, Lm, V, S0 = (float(np.median(ms[k])) for k in ("S", "L", "V", "S_nothing_used"))
bearing_bytes = M * 6 * 8
line = {"pairs": B, "corr": N, "mode": "TARGET", "repeats": REPEATS, "calls_per_timing": INNER,
        "timing": "device events around back-to-back calls",
        "S_relative_scale_per_pair_only": stat(ms["S"]), "L_relative_scale_all_outputs": stat(ms["L"]),
        "V_triangulate_per_slot_only": stat(ms["V"]), "S_with_no_link_used_no_selection_rounds": stat(ms["S_nothing_used"]),
        "S_over_V": S / V, "L_over_V": Lm / V,
        "S_over_V_range": [min(ms["S"]) / max(ms["V"]), max(ms["S"]) / min(ms["V"])],
        "L_over_V_range": [min(ms["L"]) / max(ms["V"]), max(ms["L"]) / min(ms["V"])],
        "S_minus_S_with_no_link_used_ms": S - S0, "S_minus_V_ms": S - V,
        "bearing_plane_bytes": bearing_bytes, "link_bytes": M * 4, "ratio_bytes": M * 8,
        "V_bearing_GBps": bearing_bytes / (V * 1e-3) / 1e9,
        "share_linked": share_linked, "share_used": share_used,
        "lib_sha256": hashlib.sha256(open(capi.LIB_PATH, "rb").read()).hexdigest()}
print(json.dumps(line), flush=True)
if OUT:
    with open(OUT, "w") as f:
        json.dump(line, f, indent=1)
        f.write("\n")
