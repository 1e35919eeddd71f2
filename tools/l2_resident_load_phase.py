#!/usr/bin/env python3
"""What an L2-resident payload is worth to a solve wavefront's load phase (NOTES/solve-payload-prefetch.md).

H hypotheses per pair, one block per solve (PNEC_SOLVE_GROUPS=0, and the trace keeps the launch on lm_solve_kernel):
the hypotheses of a pair are consecutive solve slots, i.e. consecutive rows of ONE XCD (xcd_contiguous_index), started a
fraction of a microsecond apart.  Hypothesis 0 reads the pair's payload from HBM; the later ones find the very same
bytes in that XCD's L2.  The load phase (s_memtime at start -> payload on chip, PNEC_HIP_TRACE) per hypothesis index is
therefore the measurement of "the same loads, as L2 hits" -- the ceiling of anything that moves the payload into L2
ahead of its wavefront.

    python tools/l2_resident_load_phase.py [pairs] [hypotheses] [corr]      (on a GPU; default 1600 x 64 x 512)
"""
import os
import sys
import tempfile

os.environ["PNEC_SOLVE_GROUPS"] = "0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from pnec_amd import Batch, capi, simulation as sim  # noqa: E402

P = int(sys.argv[1]) if len(sys.argv) > 1 else 1600
H = int(sys.argv[2]) if len(sys.argv) > 2 else 64
N = int(sys.argv[3]) if len(sys.argv) > 3 else 512
S = P * H
dev = torch.device("cuda:0")
g = sim.generate(P, N, noise_type="anisotropic_inhomogeneous", noise_level=1.0, seed=1, device=dev)
batch = Batch.uniform(capi.MODE_TARGET, P, N, device=0)
batch.fill(g.bvs1.reshape(-1, 3), g.bvs2.reshape(-1, 3), g.covs2.reshape(-1, 3, 3))
gen = torch.Generator(device=dev)
gen.manual_seed(7)
hyp = g.init_t.repeat_interleave(H, dim=0) + 0.02 * torch.randn(S, 3, generator=gen, dtype=torch.float64, device=dev)
hyp = (hyp / hyp.norm(dim=1, keepdim=True)).contiguous()
opts = capi.default_options(max_num_iterations=10, check_convergence=0)
for _ in range(3):
    batch.solve(g.init_q, g.init_t, options=opts, hyp_t=hyp, n_hyp=H)
torch.cuda.synchronize()
path = os.path.join(tempfile.gettempdir(), f"pnec_l2_resident_{os.getpid()}.bin")
os.environ["PNEC_HIP_TRACE"] = path
batch.solve(g.init_q, g.init_t, options=opts, hyp_t=hyp, n_hyp=H)
torch.cuda.synchronize()
del os.environ["PNEC_HIP_TRACE"]
a = np.fromfile(path, dtype=np.uint64).reshape(-1, 4)[-S:]
os.remove(path)
# block -> solve slot as the kernel maps itself (xcd_contiguous_index), slot -> hypothesis of its pair
b = np.arange(S, dtype=np.int64)
xcd, q, r = b & 7, S >> 3, S & 7
slot = np.where(xcd < r, xcd * (q + 1), r * (q + 1) + (xcd - r) * q) + (b >> 3)
h = slot % H
t0, t1, t2 = (a[:, i].astype(np.int64) for i in range(3))
load, life = t1 - t0, t2 - t0
steady = b >= 8192   # past the first wavefronts of every SIMD, which all load at once
print(f"{S} blocks = {P} pairs x {H} hypotheses x {N} correspondences; s_memtime ticks")
groups = [("hypothesis 0 (HBM)", h == 0), ("1..3", (h >= 1) & (h <= 3)), ("4..15", (h >= 4) & (h <= 15)), (f"16..{H - 1} (L2)", h >= 16)]
for name, m in groups:
    m = m & steady
    if not m.any():
        continue
    p10, p50, p90 = np.percentile(load[m], [10, 50, 90])
    print(f"{name:20s} n {int(m.sum()):6d}  load p10/p50/p90 {p10:6.0f} {p50:6.0f} {p90:6.0f} mean {load[m].mean():6.0f}   "
          f"lifetime p50 {np.median(life[m]):7.0f}  load/lifetime {load[m].sum() / life[m].sum():.4f}")
