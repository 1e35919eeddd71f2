#!/usr/bin/env python3
"""Headline benchmark: PNEC frame-pair solves/s (512 correspondences, 10 LM iterations).

  python bench.py --gpus N --steps K --warmup W [--workload sim100k|kitti_all] [--tracks file.npz]
                  [--dump-outputs DIR] [--full]

A plain run sets up, warms up, times the K steps and prints the line (metric, value, unit, higher_is_better, dtype,
ms_per_step).  --full also measures and checks everything beyond that headline, after the timed steps: the roofline
blocks (with one counted launch), the CPU baseline and its parity, the chain's stage times and one-at-a-time rate, and on
sim100k with one GPU the `secondary` array (BASELINE configs 3, 4, 5 and the whole chain).  --dump-outputs DIR writes
the per-pair results of the last timed step as DIR/<name>.npy (float64; a fixed sample of rows beyond 64 MB).

One process per GPU.  Launched under torch.distributed.run (RANK / LOCAL_RANK / WORLD_SIZE /
MASTER_* in the environment) it joins that job; launched plainly with --gpus N > 1 it SPAWNS the N
ranks itself (one per GPU, RCCL over xGMI, rendezvous on 127.0.0.1 at a free port) -- the analogue of
the reference's own fan-out scripts (scripts/run_simulation.sh:52-67, scripts/parallel_kitti.sh:60-69),
which start one process per experiment / sequence.

A "step" = one pass of the hot path over one batch: every rank solves its own shard of independent
frame pairs on the device, then the fixed-size result records are gathered on rank 0 with ONE
collective, issued on a side stream so that it overlaps the next step's solve.  Inputs are resident
in HBM before the timed region.  Rank 0 prints ONE JSON line.

Workloads:
  sim100k   (default; BASELINE configs[1], the headline) 100k simulated pairs x 512 anisotropic-
            covariance correspondences PER GPU, exactly 10 LM iterations -> weak scaling.
  kitti_all (BASELINE configs[4]) every frame pair of KITTI odometry 00-10 (23 190 ragged pairs),
            partitioned over the ranks in contiguous ranges balanced by correspondence count
            (pnec_amd.distributed.partition), Ceres-default termination -> strong scaling.  Real tracks
            come from --tracks <file.npz> (format: pnec_amd/tracks.py); without it a labelled
            SYNTHETIC KITTI-like stand-in with the real sequence lengths is generated.

  kitti_all --chain   the same pairs (10 % gross mismatches added) through the WHOLE chain of PNEC::Solve
            (pnec.cc:77-124, reference-default Options) in one pnec_hip_solve_pipeline call per step: ~10x the
            device time per pair of the refinement alone, i.e. the config-5 workload that has something to scale.

--share-gpu puts every rank on cuda:0 (boxes with one GPU): real solver, real partition, the gather's device
side (events, side stream, double buffering, per-rank sizes) with world > 1; the collective itself is gloo over
pinned host records, because RCCL does not accept two ranks on one device.  Its line says so ("shared_gpu").

--dry-run-cpu replaces the device solve by a stub that fabricates records (gloo on CPU): it exists so
that the spawn / partition / gather path can be exercised where there is no GPU (tests); its JSON
line says so and carries no throughput claim.
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0         # MI355X HBM3E spec (MI355X_MICROARCH.md); ~6300 achievable
FP64_VALU_PEAK_TFLOPS = 78.6  # vector FP64 (256 CU x 4 SIMD x 16 lanes x 2 flop x 2.4 GHz)
# FP64 work the kernel issues per correspondence per pass (TARGET residual; counted from
# pnec_device.hpp eval_corr<TARGET> + accumulate): 62 FMA + 28 MUL + 1 v_rsq = 91 VALU instructions,
# 62*2 + 28 + 1 = 153 flop.  The FP64 roof above prices every issue slot as an FMA (2 flop), so the
# flop fraction (153) and the issue-slot fraction (91 slots) are reported side by side.
VALU_INSTR_PER_CORR_PASS = 91
FLOP_PER_CORR_PASS = 153
# the pass that follows the last allowed iteration only needs the candidate's cost (eval_cost<TARGET>: residual and
# weight, no Jacobian, no normal equations): 24 FMA + 17 MUL + 1 max + 1 rsq = 43 instructions, 67 flop
VALU_INSTR_PER_CORR_COST_PASS = 43
FLOP_PER_CORR_COST_PASS = 67
# ---- the chain's front stages: algorithmic FP64 flop per unit of work (counted from the algebra of pnec_frontend.hip, an
# FMA = 2 flop; DESIGN.md 5b has the derivations).  The NUMBER of units a launch holds depends on the data (Newton
# iterations per hypothesis, where a model is dropped); it is counted once by a -DPNEC_WORK_COUNT build of the library
# (tools/count_chain_work.py -> profiles/chain_work_latest.json) and combined here with the live stage times.
# One evaluation of the eigenvalue function at ONE point (es_value_grad): the rotation from the Cayley vector 47, M from the
# 36 sums 339 (compose_m, round 6: M = S + S', six blocks x 18 FMA + three x 18 FMA + 9 halvings + 6 additions; the block
# form until then took 411), the smallest eigenpair by Rayleigh-quotient iteration ~274 (2.9 steps on average, counted in
# round 4), the gradient 292 = e x r_l 27 + three q_k = (sum_l G_kl y_l) x e 189 + 1 / (1 + |v|^2) 13 + the contraction
# with dR/dv 63.  Cross-check against the compiled code: tools/isa_front_regions.py counts the FP64 instructions of the
# pieces as kernels of their own -- rotation 51, M 339, gradient (evaluation with minus without) 327 flop: the
# straight-line pieces within 6 % of the model's 678 (tests/test_bench_launch_cpu.py holds it there).
FLOP_ES_POINT = 47 + 339 + 274 + 292
FLOP_ES_QUAD_EVAL = 4 * FLOP_ES_POINT + 160   # a quad's trip: four points + the iteration's head
FLOP_SCORE_CORR = 117                # reprojection score of one correspondence against one model
FLOP_INLIER_CORR = 117 + 84          # ... + its 36 sums when it is an inlier
FLOP_SAMPLE_CORR = 84                # a sampled correspondence's share of the 36 sums
FLOP_SUMS36W_CORR = 145              # weight + 36 weighted sums
FLOP_WES_TABLE_CORR = 129            # n = f1 x R f2 and B = f1hat R Sigma R' f1hat' + reg I
FLOP_WES_COST_CORR = 28              # (t.n)^2 / t'Bt
FLOP_WES_SCF_CORR = 36               # A_i / t'B_i t into the 3x3 sum
FLOP_WES_BOUND_CORR = 18             # n n' / trace(B)


def chain_stage_rooflines(counts, stage_ms, payload_bytes, inlier_payload_bytes, refinement):
    """Roofline block per stage of the chain: VALU-bound stages by algorithmic flop (committed work counts x the flop
    model above) against the FP64 vector peak, the bandwidth-bound ones by the bytes they must move against HBM."""
    out = []
    if counts:
        r, w = counts["ransac_stage"], counts["weighted_stage"]
        ss = 10
        fl = (r.get("ransac_quad_evaluations", 0) + r.get("es_on_inliers_quad_evaluations", 0)) * FLOP_ES_QUAD_EVAL \
            + r.get("ransac_scored_tiles", 0) * 64 * FLOP_SCORE_CORR + r.get("ransac_inlier_pass_corr", 0) * FLOP_INLIER_CORR \
            + r.get("ransac_hypotheses", 0) * ss * FLOP_SAMPLE_CORR
        t = stage_ms["ransac_es"] * 1e-3
        out.append({"stage": "RANSAC eigensolver + InlierExtraction (ransac*_eigensolver_kernel, es_batch_kernel<1>)",
                    "bound": "valu_fp64", "achieved": fl / t / 1e12, "peak": FP64_VALU_PEAK_TFLOPS, "unit": "TFLOP/s",
                    "frac": fl / t / 1e12 / FP64_VALU_PEAK_TFLOPS, "ms": stage_ms["ransac_es"], "algorithmic_gflop": fl / 1e9,
                    "work": {k: r[k] for k in r}, "hbm_bytes_min": payload_bytes + inlier_payload_bytes,
                    "hbm_frac_if_it_were_the_bound": (payload_bytes + inlier_payload_bytes) / t / 1e9 / HBM_PEAK_GBS})
        fl = (w.get("es_first_quad_evaluations", 0) + w.get("weighted_inkernel_quad_evaluations", 0)) * FLOP_ES_QUAD_EVAL \
            + w.get("sums36_weighted_corr", 0) * FLOP_SUMS36W_CORR + w.get("weighted_table_corr", 0) * FLOP_WES_TABLE_CORR \
            + w.get("weighted_cost_corr", 0) * FLOP_WES_COST_CORR + w.get("weighted_scf_corr", 0) * FLOP_WES_SCF_CORR \
            + w.get("weighted_bound_corr", 0) * FLOP_WES_BOUND_CORR
        t = stage_ms["weighted_es"] * 1e-3
        out.append({"stage": "weighted eigensolver + SCF (sums36_kernel<true>, es_batch_kernel<0>, weighted_eigensolver_kernel)",
                    "bound": "valu_fp64", "achieved": fl / t / 1e12, "peak": FP64_VALU_PEAK_TFLOPS, "unit": "TFLOP/s",
                    "frac": fl / t / 1e12 / FP64_VALU_PEAK_TFLOPS, "ms": stage_ms["weighted_es"], "algorithmic_gflop": fl / 1e9,
                    "work": {k: w[k] for k in w}, "hbm_bytes_min": 2 * inlier_payload_bytes,
                    "hbm_frac_if_it_were_the_bound": 2 * inlier_payload_bytes / t / 1e9 / HBM_PEAK_GBS})
    else:
        for k, name in (("ransac_es", "RANSAC eigensolver + InlierExtraction"), ("weighted_es", "weighted eigensolver + SCF")):
            out.append({"stage": name, "bound": "valu_fp64", "achieved": None, "peak": FP64_VALU_PEAK_TFLOPS, "unit": "TFLOP/s",
                        "frac": None, "ms": stage_ms[k],
                        "note": "no committed work counts for this workload (tools/count_chain_work.py)"})
    out.append(refinement)
    return out


# the front stages' device code: what the flop model above was counted from and what the committed work counts were taken on
FRONT_KERNEL_SOURCES = ("pnec_frontend.hip", "pnec_es_schemes.inl", "pnec_device.hpp", "pnec_front_shared.hpp")
# sha256 (front_sources_sha256) of the sources the FLOP_* table above was last derived from / cross-checked against
# (tools/isa_front_regions.py); tests/test_bench_launch_cpu.py fails when the sources move on without it
FRONT_FLOP_MODEL_STAMP = "27df01740a57074aa8fbcea9692d2fcf70cb7e05a0852e0a592793667e1aab93"


def front_sources_sha256():
    """Identity of the front stages' device code (comments and layout stripped), like kernel_sources_sha256."""
    d = os.path.join(ROOT, "pnec_amd", "csrc")
    h = hashlib.sha256()
    for f in FRONT_KERNEL_SOURCES:
        h.update(f.encode())
        h.update(_strip_comments(open(os.path.join(d, f), "r").read()).encode())
    return h.hexdigest()


def load_chain_counts(name, pairs, corr):
    """The committed work counts of a bench workload -- only if they were taken on THIS front-stage code and workload."""
    try:
        j = json.load(open(os.path.join(ROOT, "profiles", "chain_work_latest.json")))
        if j.get("frontend_sources_sha256") != front_sources_sha256():
            return None
        c = j["workloads"][name]
        return c if (c["pairs"], c["correspondences"]) == (pairs, corr) else None
    except (OSError, KeyError, ValueError):
        return None


def executed_passes(batch, q0, t0, opts, capi, **solve_kw):
    """How many correspondence-passes ONE launch of the refinement over `batch` executes, in full and cost-only: one extra,
    untimed launch with the diagnostics flag set (PNEC_HIP_OPT_COUNT_PASSES in pnec_hip_options.flags -> pnec_hip_work_counters[13], [14]).
    The kernel skips the Jacobian of a candidate whose step it expects to be rejected and evaluates a solve's last
    candidate at the iteration cap cost-only, so the number of full passes is a property of the data; with the same
    inputs the counted launch executes exactly what the timed ones do."""
    import ctypes as C

    import torch
    L = capi.lib()
    out = np.zeros(16, dtype=np.uint64)
    flag = C.c_int32(0)
    torch.cuda.synchronize()
    capi.check(L.pnec_hip_work_counters(batch.device, 1, out.ctypes.data, C.byref(flag)))
    o2 = capi.Options.from_buffer_copy(bytes(opts))
    o2.flags = 1
    batch.solve(q0, t0, options=o2, **solve_kw)
    torch.cuda.synchronize()
    capi.check(L.pnec_hip_work_counters(batch.device, 1, out.ctypes.data, C.byref(flag)))
    return int(out[13]), int(out[14])


def refinement_roofline(batch, res, kernel_ms, ragged, capi, launch=None, passes_executed=None, primary="hbm"):
    """The roofline block of one launch of lm_solve_kernel<TARGET> over `batch` (result `res`): read-once HBM bytes and
    algorithmic FP64 flop (153 per correspondence and full pass, 67 for the cost-only pass of a solve that ends at the
    iteration cap) against the two roofs."""
    import torch
    my_pairs = int(res.iterations.numel())
    payload = batch.payload_bytes
    iters_done = res.iterations.to(torch.float64)
    passes = float(iters_done.mean()) + 1.0 if my_pairs else 0.0
    sizes = torch.as_tensor(np.diff(batch.offsets), dtype=torch.float64, device=iters_done.device)
    n_hyp = my_pairs // max(1, len(sizes))
    if n_hyp > 1:
        sizes = sizes.repeat_interleave(n_hyp)
    corr_passes = float(((iters_done + 1.0) * sizes).sum()) if my_pairs else 0.0
    capped = res.status == capi.TERM_MAX_ITERATIONS
    cost_corr = float((capped.to(torch.float64) * sizes).sum()) if my_pairs else 0.0
    full_corr = corr_passes - cost_corr
    counted = passes_executed is not None
    if counted:   # what the kernel executed (a counted launch on the same inputs): cost-only passes after rejected steps too
        full_corr, cost_corr = float(passes_executed[0]), float(passes_executed[1])
    t = kernel_ms * 1e-3
    flops = FLOP_PER_CORR_PASS * full_corr + FLOP_PER_CORR_COST_PASS * cost_corr
    gbs = payload / t / 1e9
    if primary == "valu_fp64":
        # several hypotheses per pair: the payload is read once per pair (and group of hypotheses) and evaluated n_hyp times --
        # HBM is not what such a launch is priced against (19 GB/s of 8 TB/s said nothing); the FP64 vector roof is
        tf = flops / t / 1e12
        return {"stage": "refinement, multi-hypothesis (lm_solve_group_kernel<TARGET>)", "bound": "valu_fp64", "achieved": tf,
                "peak": FP64_VALU_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": tf / FP64_VALU_PEAK_TFLOPS, "ms": kernel_ms,
                "algorithmic_flop_per_launch": flops, "passes": passes,
                "correspondence_passes_executed": {"full": full_corr, "cost_only": cost_corr,
                                                   "source": "counted launch (pnec_hip_work_counters)" if counted else
                                                             "iterations + 1 per solve, the last one cost-only at the cap"},
                "hbm": {"achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": gbs / HBM_PEAK_GBS,
                        "algorithmic_bytes_per_launch": payload,
                        "note": "read once per pair; the hypotheses of a pair share it (L2 / on-chip)"},
                "binding_frac": tf / FP64_VALU_PEAK_TFLOPS, "launch": launch}
    return {"stage": "refinement (lm_solve_kernel<TARGET>)", "bound": "hbm", "bound_binding": "valu_fp64",
            "achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": gbs / HBM_PEAK_GBS, "ms": kernel_ms,
            "algorithmic_bytes_per_launch": payload, "passes": passes,
            "correspondence_passes_executed": {"full": full_corr, "cost_only": cost_corr,
                                               "source": "counted launch (pnec_hip_work_counters)" if counted else
                                                         "iterations + 1 per solve, the last one cost-only at the cap"},
            "valu": {"achieved": flops / t / 1e12, "peak": FP64_VALU_PEAK_TFLOPS, "unit": "TFLOP/s",
                     "frac": flops / t / 1e12 / FP64_VALU_PEAK_TFLOPS},
            "binding_frac": flops / t / 1e12 / FP64_VALU_PEAK_TFLOPS, "launch": launch}


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=20, help="untimed steps; ~20 of these 3.5 ms steps bring the GPU to its steady clocks")
    ap.add_argument("--workload", choices=("sim100k", "kitti_all"), default="sim100k")
    ap.add_argument("--tracks", default=None, help="kitti_all: .npz of real tracks (pnec_amd/tracks.py)")
    ap.add_argument("--pairs", type=int, default=100_000, help="sim100k: frame pairs per GPU")
    ap.add_argument("--corr", type=int, default=512, help="sim100k: correspondences per pair")
    ap.add_argument("--iters", type=int, default=10, help="sim100k: LM iterations per solve (fixed count)")
    ap.add_argument("--cpl", type=int, default=0, help="launch tuning: correspondences per lane")
    ap.add_argument("--wpp", type=int, default=0, help="launch tuning: wavefronts per solve")
    ap.add_argument("--ldsk", type=int, default=0, help="launch tuning: correspondences per lane kept in LDS")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also measure and check everything beyond the headline: rooflines, CPU "
                         "baseline + parity, the chain's stage times, the `secondary` array (off: the plain, lean run)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's per-pair results as DIR/<name>.npy (float64, at most 64 MB)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline (and the secondary array)")
    ap.add_argument("--no-secondary", action="store_true",
                    help="--full, sim100k on one GPU: skip the `secondary` array (BASELINE configs 3, 4, 5 and the whole chain, "
                         "measured in the same process after the headline)")
    ap.add_argument("--quick-secondary", action="store_true", help="fewer steps / a shorter stream in the secondary runs (tests)")
    ap.add_argument("--cpu-sample", type=int, default=0, help="--full: pairs in the CPU baseline sample (0 = auto)")
    ap.add_argument("--sync-gather", action="store_true", help="gather on the solve's stream (A/B of the overlap)")
    ap.add_argument("--single-process", action="store_true",
                    help="sim100k: drive all --gpus devices from THIS process through the persistent multi-device handle "
                         "(pnec_hip_multi_*: one host thread, batch and stream per device, no collective) instead of one rank "
                         "per GPU + an RCCL gather -- the comparison line for a SCALE run; with --share-gpu every entry of "
                         "the device list is cuda:0")
    ap.add_argument("--dry-run-cpu", action="store_true", help="gloo + stubbed solve: exercises spawn/partition/gather without a GPU")
    ap.add_argument("--share-gpu", action="store_true",
                    help="all ranks on cuda:0 (single-GPU boxes): the real solver and the device side of the gather "
                         "(events, side stream, per-rank sizes) with world > 1; the collective is gloo over pinned "
                         "host records because RCCL refuses two ranks on one device")
    ap.add_argument("--chain", action="store_true",
                    help="kitti_all: the whole PNEC::Solve chain per pair (pnec_hip_solve_pipeline: RANSAC eigensolver, "
                         "inlier extraction, weighted eigensolver + SCF, refinement) instead of the refinement alone")
    ap.add_argument("--outliers", type=float, default=0.10, help="--chain: share of gross mismatches in the synthetic set")
    ap.add_argument("--es-scheme", type=int, default=2, choices=(0, 1, 2),
                    help="--chain: which iteration minimises the eigenvalue (include/pnec_hip.h pnec_hip_eigensolver_scheme); "
                         "2 = the C++ facade's default (the restatement believed to be opengv's), 0 = the C ABI's (damped Newton)")
    ap.add_argument("--in-flight", type=int, default=3,
                    help="--chain: steps kept in flight, each on its own stream and its own copy of the batch (the chain's "
                         "kernels end in tails of a few long pairs; the next step's work fills them).  1 = one at a time")
    return ap.parse_args(argv)


# ---------------------------------------------------------------------------------------------------
# launch: join torchrun's job, or spawn the ranks ourselves
def free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def spawn_ranks(n: int, argv) -> int:
    """Start n copies of this script, one per GPU; rank 0 inherits stdout (it prints the JSON line)."""
    port = free_port()
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), PNEC_BENCH_SPAWNED="1")
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC (RCCL between processes on this driver)
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + list(argv), env=env,
                                      stdout=None if r == 0 else subprocess.DEVNULL))
    rc = 0
    deadline = None
    while procs:
        for p in list(procs):
            code = p.poll()
            if code is None:
                continue
            procs.remove(p)
            if code != 0 and rc == 0:
                rc = code
                deadline = time.time() + 30.0  # a rank died: give the others a moment, then stop them
        if deadline is not None and time.time() > deadline:
            for p in procs:
                p.kill()
        time.sleep(0.05)
    return rc


# ---------------------------------------------------------------------------------------------------
# workloads: each returns a Shard (this rank's pairs in HBM) + the global partition
class Shard:
    pass


def build_sim100k(args, rank, world, device):
    """Synthetic shard, generated on the GPU in chunks straight into the solver's SoA layout."""
    import torch

    from pnec_amd import Batch, capi
    from pnec_amd import simulation as sim
    sh = Shard()
    sh.sizes = [args.pairs] * world                       # weak scaling: same work on every rank
    sh.total_pairs = args.pairs * world
    sh.scaling = "weak"
    sh.data = "synthetic"
    sh.opts = dict(max_num_iterations=args.iters, check_convergence=0)
    sh.workload = ("configs[1]: batch of 100k simulated frame pairs x 512 anisotropic-covariance "
                   "correspondences per GPU")
    if args.dry_run_cpu:
        sh.batch, sh.q0, sh.t0, sh.sample = None, None, None, None
        return sh
    batch = Batch.uniform(capi.MODE_TARGET, args.pairs, args.corr, device=device.index)
    chunk = 10_000
    qs, ts, sample = [], [], None
    for c, first in enumerate(range(0, args.pairs, chunk)):
        m = min(chunk, args.pairs - first)
        g = sim.generate(m, args.corr, noise_type="anisotropic_inhomogeneous", noise_level=1.0,
                         seed=1 + 1000 * rank + c, device=device)
        batch.fill(g.bvs1.reshape(-1, 3), g.bvs2.reshape(-1, 3), g.covs2.reshape(-1, 3, 3),
                   first_pair=first, n_pairs=m)
        qs.append(g.init_q)
        ts.append(g.init_t)
        if sample is None:  # first chunk doubles as the CPU-baseline / parity sample
            k = min(m, 4096)
            sample = (np.arange(k + 1, dtype=np.int64) * args.corr, g.bvs1[:k].reshape(-1, 3),
                      g.bvs2[:k].reshape(-1, 3), g.covs2[:k].reshape(-1, 3, 3), g.init_q[:k], g.init_t[:k])
        del g
    sh.batch, sh.q0, sh.t0, sh.sample = batch, torch.cat(qs), torch.cat(ts), sample
    return sh


def build_kitti_all(args, rank, world, device):
    """Config 5: all pairs of the 11 sequences, contiguous ranges balanced by correspondence count."""
    from pnec_amd import tracks as tk
    from pnec_amd.distributed import partition
    sh = Shard()
    sizes = tk.sizes_of(args.tracks) if args.tracks else tk.kitti_all_sizes()
    bounds = partition(sizes, world)
    sh.bounds = bounds
    sh.sizes = [int(bounds[r + 1] - bounds[r]) for r in range(world)]
    sh.total_pairs = int(len(sizes))
    sh.shard_corr = [int(sizes[bounds[r]:bounds[r + 1]].sum()) for r in range(world)]
    sh.scaling = "strong"
    sh.opts = dict()                                       # Ceres-default termination (what the VO runs)
    sh.workload = ("configs[4]: all KITTI 00-10 frame pairs (23 190 ragged pairs) sharded as independent "
                   "batches, contiguous ranges balanced by correspondence count")
    sh.data = f"tracks:{os.path.basename(args.tracks)}" if args.tracks else "synthetic"
    if args.chain:
        sh.workload += (f"; whole PNEC::Solve chain per pair (reference-default Options"
                        + ("" if args.tracks else f", {args.outliers:.0%} gross mismatches added") + ")")
    sh.pair_sizes = sizes
    if args.dry_run_cpu:
        sh.batch, sh.q0, sh.t0, sh.sample = None, None, None, None
        return sh
    import torch

    from pnec_amd import Batch, capi
    a, b = int(bounds[rank]), int(bounds[rank + 1])
    tr = tk.load_tracks(args.tracks, a, b) if args.tracks else \
        tk.kitti_all_shard(a, b, device=device, outlier_frac=args.outliers if args.chain else 0.0)
    as_dev = lambda x: x if hasattr(x, "is_cuda") and x.is_cuda else torch.as_tensor(np.asarray(x), device=device)
    batch = Batch(capi.MODE_TARGET, tr.offsets, device=device.index)
    if tr.n_pairs:
        batch.fill(as_dev(tr.bvs1), as_dev(tr.bvs2), as_dev(tr.covs))
    sh.batch, sh.q0, sh.t0 = batch, as_dev(tr.init_q).contiguous(), as_dev(tr.init_t).contiguous()
    sh.batches = [batch]
    for _ in range(max(1, args.in_flight) - 1 if args.chain else 0):   # one copy of the shard per step in flight
        extra = Batch(capi.MODE_TARGET, tr.offsets, device=device.index)
        if tr.n_pairs:
            extra.fill(as_dev(tr.bvs1), as_dev(tr.bvs2), as_dev(tr.covs))
        sh.batches.append(extra)
    k = min(tr.n_pairs, 2048)
    m = int(tr.offsets[k])
    sh.sample = (tr.offsets[:k + 1], as_dev(tr.bvs1)[:m], as_dev(tr.bvs2)[:m], as_dev(tr.covs)[:m], sh.q0[:k], sh.t0[:k])
    return sh


# ---------------------------------------------------------------------------------------------------
def host_cpu_facts():
    """What the process may use of this host: logical CPUs OpenMP sees, the scheduler affinity, the cgroup CPU quota."""
    facts = {"cores_logical": os.cpu_count()}
    try:
        facts["cores_affinity"] = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        facts["cores_affinity"] = None
    quota = None
    for f in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            txt = open(f).read().split()
            if f.endswith("cpu.max"):
                quota = None if txt[0] == "max" else float(txt[0]) / float(txt[1])
            else:
                q = float(txt[0])
                quota = None if q <= 0 else q / float(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            facts["cgroup_cpu_quota_file"] = f
            break
        except (OSError, ValueError, IndexError):
            continue
    facts["cgroup_cpu_quota_cpus"] = quota
    return facts


def cpu_baseline(sample, n_sample, opts_hip, gpu_q):
    """The oracle (reference-faithful port: central differences + Ceres LM policy) timed on this
    box's host cores over a bounded sample of the same workload; also the parity figure."""
    from oracle import pnec_oracle as po
    # the same sources compiled for THIS host (-O3 -march=native) when the box has a compiler; else the portable build
    native = po.build_native()
    if native:
        po.use_library(native)
    march = "native (built on this box: oracle/Makefile `native`)" if native else "x86-64-v3 (portable build: no compiler on this box)"
    threads_all = po.max_threads()
    offsets, b1, b2, cv, iq, it = sample
    offsets = np.asarray(offsets[:n_sample + 1], dtype=np.int64)
    m = int(offsets[-1])
    f1, f2 = b1[:m].cpu().numpy(), b2[:m].cpu().numpy()
    c9 = po.covs_to_colmajor9(cv[:m].cpu().numpy())
    q0, t0 = iq[:n_sample].cpu().numpy(), it[:n_sample].cpu().numpy()
    o = po.default_options(jacobian_mode=po.JAC_NUMERIC_CENTRAL,
                           max_num_iterations=opts_hip.max_num_iterations,
                           check_convergence=opts_hip.check_convergence)
    po.lib().pnec_oracle_lm_diagnostics(0)   # (test tooling of the checker: not in the timed baseline)
    # single thread (the reference's real execution model) on a small slice
    n1 = max(8, min(64, n_sample))
    t = time.perf_counter()
    po.solve_batch(po.MODE_TARGET, offsets[:n1 + 1], f1, f2, c9, None, 1e-13, q0, t0, options=o, num_threads=1)
    single = n1 / (time.perf_counter() - t)
    # How the box scales -- 8, 16, 32, 64, all threads -- and the baseline = the BEST of them: omp_get_max_threads() reports
    # every logical CPU of the host, but a container may hold a cgroup CPU quota far below that (the round-5 GPU boxes:
    # 256 logical CPUs, cpu.max = 16 CPUs), and 128 threads time-slicing a 16-CPU quota are slower than 32.
    facts = host_cpu_facts()
    scaling = {"1": single}
    q = tt = cost = its = st = None
    best_th, rate = 1, single
    cands = sorted({th for th in (8, 16, 32, 64, threads_all) if th <= threads_all})
    for th in cands:
        rates = []
        for _ in range(3 if th == cands[-1] or th in (16, 32) else 1):
            t = time.perf_counter()
            r_ = po.solve_batch(po.MODE_TARGET, offsets, f1, f2, c9, None, 1e-13, q0, t0, options=o, num_threads=th)
            rates.append(n_sample / (time.perf_counter() - t))
        q, tt, cost, its, st = r_
        scaling[str(th)] = float(np.median(rates))
        if scaling[str(th)] > rate:
            best_th, rate = th, scaling[str(th)]
    gq = gpu_q[:n_sample].cpu().numpy()   # parity of the GPU result on the same pairs
    dots = np.clip(np.abs(np.sum(gq * q, axis=1)), 0.0, 1.0)
    dq = np.stack([
        gq[:, 3] * q[:, 0] - gq[:, 0] * q[:, 3] - gq[:, 1] * q[:, 2] + gq[:, 2] * q[:, 1],
        gq[:, 3] * q[:, 1] + gq[:, 0] * q[:, 2] - gq[:, 1] * q[:, 3] - gq[:, 2] * q[:, 0],
        gq[:, 3] * q[:, 2] - gq[:, 0] * q[:, 1] + gq[:, 1] * q[:, 0] - gq[:, 2] * q[:, 3]], 1)
    ang = 2.0 * np.arctan2(np.linalg.norm(dq, axis=1), dots)  # small-angle safe
    sizes = np.diff(offsets)
    base = {"value": rate, "unit": "solves/s", "cores": best_th, "kind": "port",
            "cores_note": "`cores` = the OpenMP thread count that gave the best rate (`value`) among those tried "
                          "(`scaling_solves_per_s_by_threads`); `cores_effective` = value / single_thread_value is what they "
                          "amount to on this box -- SMT siblings, throttling and the cgroup quota included",
            "cores_effective": rate / single if single > 0 else None, "omp_max_threads": threads_all,
            "single_thread_value": single, "scaling_solves_per_s_by_threads": scaling, "march": march, **facts,
            "sample": f"{n_sample} of the benchmark's own pairs ({int(sizes.min())}..{int(sizes.max())} corr, "
                      f"{'Ceres-default termination' if opts_hip.check_convergence else str(opts_hip.max_num_iterations) + ' LM iterations'}, "
                      f"central-difference Jacobian + Ceres LM policy, OpenMP over pairs, median of 3)"}
    parity = {"max_rot_err_rad": float(ang.max()), "median_rot_err_rad": float(np.median(ang)),
              "n_pairs": int(n_sample), "against": "oracle (reference-faithful port), same inputs, same options",
              "tolerance_rad": 1e-6}
    return base, parity


# everything that is compiled into lm_solve_kernel -- the kernel the profiled counters belong to: the kernel and
# its device helpers, the launcher and its translation units, the build recipe (flags) and the ABI structs
SOLVE_KERNEL_SOURCES = ("pnec_solve_kernel.hpp", "pnec_device.hpp", "pnec_solve_launch.inl", "pnec_solve_nec.hip",
                        "pnec_solve_target.hip", "pnec_solve_host.hip", "pnec_solve_sym.hip", "Makefile")


def _strip_comments(text: str) -> str:
    import re
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    return " ".join(text.split())


def kernel_sources_sha256():
    """Identity of the device code of the benchmarked kernel: sha256 over its sources (comments and layout
    stripped), the build recipe and the one ABI struct the kernel reads (pnec_hip_options) -- stable across
    rebuilds on another box and across edits that cannot change the kernel (comments, other ABI entries)."""
    import re
    d = os.path.join(ROOT, "pnec_amd", "csrc")
    h = hashlib.sha256()
    for f in SOLVE_KERNEL_SOURCES:
        text = open(os.path.join(d, f), "r").read()
        h.update(f.encode())
        if f == "Makefile":
            # the build recipe of the kernels: compiler, target and flags (incl. their continuation lines) -- not the
            # lists of sources / headers / host targets, which cannot change the device code of this kernel
            keep, cont = [], False
            for ln in text.splitlines():
                if cont or re.match(r"\s*(HIPCC|ARCH|CXXFLAGS|CXXBASE|SCHED_\w+)\s*[?:+]?=", ln):
                    keep.append(" ".join(ln.split()))
                    cont = ln.rstrip().endswith("\\")
                else:
                    cont = False
            text = "\n".join(keep)
        h.update((text if f == "Makefile" else _strip_comments(text)).encode())
    header = open(os.path.join(ROOT, "include", "pnec_hip.h"), "r").read()
    m = re.search(r"typedef struct pnec_hip_options\s*\{.*?\}\s*pnec_hip_options;", header, flags=re.S)
    h.update(_strip_comments(m.group(0) if m else header).encode())
    return h.hexdigest()


def profiled_counters(lib_path, key):
    """HBM traffic / VALU-busy of the dominant kernel from the committed rocprofv3 PMC passes -- only if
    they were taken on THIS device code (sha256 of the kernel sources, or of the built library) and on
    this workload + geometry; otherwise None: a kernel change must not leave a stale counter in the line."""
    try:
        tj = json.load(open(os.path.join(ROOT, "profiles", "traffic_latest.json")))
        same_code = tj.get("kernel_sources_sha256") == kernel_sources_sha256() or \
            tj.get("lib_sha256") == hashlib.sha256(open(lib_path, "rb").read()).hexdigest()
        w = tj["workload"]
        if same_code and [w["name"], w["pairs"], w["corr"], w["iters"], w["geometry"]] == key:
            return tj["hbm_bytes_per_launch"], tj.get("valu_busy_frac"), None
        return None, None, "profiles/traffic_latest.json was measured on other device code or another workload"
    except (OSError, KeyError, ValueError):
        return None, None, "no committed PMC record"


# ---------------------------------------------------------------------------------------------------
# N > 1: pre-flight + the first collective under a watchdog.  The multi-GPU path has never met more than one device on
# the builder's boxes; whatever goes wrong the first time it does (a communicator that cannot form, IPC handles the
# driver refuses, a rank that never arrives) must come out as ONE JSON line with an "error", not as a hang.
def _fail_line(args, what, detail):
    print(json.dumps({"metric": "PNEC pose solves/sec (512 corr, 10 GN iters)" if args.workload == "sim100k" else "PNEC (kitti_all)",
                      "value": None, "unit": "solves/s", "n_gpus": args.gpus, "steps": args.steps, "warmup": args.warmup,
                      "error": what, "detail": detail}), flush=True)


def join_job(args, world, rank, device, cpu):
    import datetime
    import threading

    import torch
    import torch.distributed as dist
    backend = "gloo" if (cpu or args.share_gpu) else "nccl"
    info = {"backend": backend, "world_size": world, "rank": rank, "master": f"{os.environ.get('MASTER_ADDR')}:{os.environ.get('MASTER_PORT')}",
            "HSA_ENABLE_IPC_MODE_LEGACY": os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY"),
            "NCCL_DEBUG": os.environ.get("NCCL_DEBUG"), "torch": torch.__version__}
    if not cpu:
        info["visible_devices"] = torch.cuda.device_count()
        info["device"] = str(device)
        try:
            info["rccl_version"] = ".".join(str(x) for x in torch.cuda.nccl.version())
        except Exception as e:   # noqa: BLE001
            info["rccl_version"] = f"unavailable ({e})"
    if rank == 0:
        print(json.dumps({"preflight": info}), file=sys.stderr, flush=True)
    limit = float(os.environ.get("PNEC_BENCH_JOIN_TIMEOUT_S", "180"))
    stage = ["init_process_group"]

    def watchdog():
        if rank == 0:
            _fail_line(args, f"multi-GPU start-up did not finish within {limit:.0f} s (stuck in {stage[0]})", info)
        else:
            print(json.dumps({"rank": rank, "error": f"stuck in {stage[0]}", "preflight": info}), file=sys.stderr, flush=True)
        os._exit(3)

    timer = threading.Timer(limit, watchdog)
    timer.daemon = True
    timer.start()
    try:
        if backend == "gloo":
            dist.init_process_group("gloo", timeout=datetime.timedelta(seconds=limit))
        else:
            dist.init_process_group("nccl", device_id=device, timeout=datetime.timedelta(seconds=limit))
        stage[0] = "the first collective (all_reduce of one number per rank)"
        probe = torch.ones(1, dtype=torch.float64, device="cpu" if backend == "gloo" else device)
        dist.all_reduce(probe)
        if not cpu:
            torch.cuda.synchronize()
        if int(probe.item()) != world:
            raise RuntimeError(f"all_reduce over {world} ranks returned {probe.item()}")
    except Exception as e:   # noqa: BLE001
        timer.cancel()
        if rank == 0:
            _fail_line(args, f"{stage[0]} failed: {type(e).__name__}: {e}", info)
        raise SystemExit(3)
    timer.cancel()


# ---------------------------------------------------------------------------------------------------
# the other BASELINE configs, measured in the same process after the headline (the `secondary` array of the line)
def _quat_angles(a, b):
    a, b = np.asarray(a), np.asarray(b)
    d = np.abs(np.sum(a * b, axis=1)).clip(0, 1)
    v = np.stack([a[:, 3] * b[:, 0] - a[:, 0] * b[:, 3] - a[:, 1] * b[:, 2] + a[:, 2] * b[:, 1],
                  a[:, 3] * b[:, 1] + a[:, 0] * b[:, 2] - a[:, 1] * b[:, 3] - a[:, 2] * b[:, 0],
                  a[:, 3] * b[:, 2] - a[:, 0] * b[:, 1] + a[:, 1] * b[:, 0] - a[:, 2] * b[:, 3]], 1)
    return 2.0 * np.arctan2(np.linalg.norm(v, axis=1), d)


def chain_stage_times(batch, q0, t0, reps=3):
    """The chain stage by stage (the same launches as the one call, bit-identical results) with events between the
    stages: ms per stage, mean of `reps` after one warm-up."""
    import torch
    acc = {"ransac_es": 0.0, "inlier_extraction": 0.0, "weighted_es": 0.0, "refinement": 0.0}
    res = None
    for r in range(reps + 1):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        ev[0].record()
        qr, tr, mask, cnt, its = batch.ransac_eigensolver(q0, seed=1)
        ev[1].record()
        sel = batch.select(mask, view=True)
        ev[2].record()
        qw, tw = sel.weighted_eigensolver(qr, tr, 1e-13, 10)
        ev[3].record()
        res = sel.solve(qw, tw)
        ev[4].record()
        torch.cuda.synchronize()
        if r:
            for k, (a, b) in zip(acc, zip(ev[:-1], ev[1:])):
                acc[k] += a.elapsed_time(b) / reps
    sel_payload = int(cnt.sum()) * 96
    return acc, res, sel, sel_payload


def lockstep_sequences(device, capi, tk, quick=False, check_steps=12, scheme=2):
    """The KITTI-like set's sequences advanced side by side: -> dict(wall_s, steps, sequences, pairs, q [P,4] in the set's
    pair order, bitwise_equal_to_one_call_per_frame, n_compared)."""
    import torch

    from pnec_amd import Batch
    from pnec_amd.frame import FrameSolver
    frames = tk.KITTI_FRAMES if not quick else tuple(max(2, f // 12) for f in tk.KITTI_FRAMES)
    sizes = tk.kitti_all_sizes(frames=frames)
    P = int(len(sizes))
    tr = tk.kitti_all_shard(0, P, device=device, frames=frames, outlier_frac=0.10)
    seq = np.asarray(tr.sequence)
    lens = np.array([f - 1 for f in frames])
    order = np.argsort(-lens, kind="stable")                   # longest sequence first: the running ones are a prefix
    start = np.concatenate([[0], np.cumsum(lens)])
    T = int(lens.max())
    step_pairs = [np.array([start[s] + k for s in order if lens[s] > k], dtype=np.int64) for k in range(T)]
    off = np.asarray(tr.offsets, dtype=np.int64)
    # the correspondences regrouped step by step (a gather on the device, once): step k's pairs are contiguous
    flat = np.concatenate(step_pairs)
    cnt = np.diff(off)[flat]
    src = torch.as_tensor(np.concatenate([np.arange(off[p], off[p + 1]) for p in flat]), device=device)
    f1, f2, cv = tr.bvs1[src].contiguous(), tr.bvs2[src].contiguous(), tr.covs[src].contiguous()
    step_off = np.concatenate([[0], np.cumsum([len(sp) for sp in step_pairs])])
    corr_off = np.concatenate([[0], np.cumsum(cnt)])
    S = len(frames)
    q_out = torch.zeros(P, 4, dtype=torch.float64, device=device)
    flat_t = torch.as_tensor(flat, device=device)
    popts = capi.default_pipeline_options(eigensolver_scheme=scheme)
    wall = None
    with Batch.with_capacity(capi.MODE_TARGET, S, int(S * (np.diff(off).max() + 64)), device=device.index) as b:
        for rep in range(2):                                   # the first pass warms the batch's scratch
            q_prev = torch.zeros(S, 4, dtype=torch.float64, device=device)
            q_prev[:, 3] = 1.0
            t_prev = torch.zeros(S, 3, dtype=torch.float64, device=device)
            t_prev[:, 2] = 1.0
            outs = []
            torch.cuda.synchronize()
            t_0 = time.perf_counter()
            for k in range(T):
                a, e = int(step_off[k]), int(step_off[k + 1])
                n = e - a
                ca, ce = int(corr_off[a]), int(corr_off[e])
                b.reshape(np.concatenate([[0], np.cumsum(cnt[a:e])]))
                b.fill(f1[ca:ce], f2[ca:ce], cv[ca:ce])
                popts.first_pair_id = a                        # RANSAC draws keyed by the pair's place in this order
                q_prev, t_prev = b.solve_pipeline(q_prev[:n].contiguous(), t_prev[:n].contiguous(), options=popts)
                outs.append(q_prev)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t_0
        q_steps = torch.cat(outs)
    q_out[flat_t] = q_steps
    # the same frames one call per frame, for the first steps of every sequence: same start poses, same pair ids
    equal, n_cmp = True, 0
    q_steps_h = q_steps.cpu().numpy()
    f1h, f2h = f1.cpu().numpy(), f2.cpu().numpy()
    c9 = np.ascontiguousarray(np.transpose(cv.cpu().numpy(), (0, 2, 1)).reshape(-1, 9))
    with FrameSolver(max_corr=int(np.diff(off).max()), device=device.index) as fs:
        o1 = capi.default_pipeline_options(eigensolver_scheme=scheme)
        oq, ot, mask = np.zeros(4), np.zeros(3), np.zeros(int(np.diff(off).max()), dtype=np.uint8)
        prev = {}
        for k in range(min(check_steps, T)):
            a, e = int(step_off[k]), int(step_off[k + 1])
            for i in range(e - a):
                j = a + i
                qi, ti = prev.get(i, (np.array([0.0, 0.0, 0.0, 1.0]), np.array([0.0, 0.0, 1.0])))
                o1.first_pair_id = j
                ca, ce = int(corr_off[j]), int(corr_off[j + 1])
                fs.solve_raw(ce - ca, f1h[ca:ce], f2h[ca:ce], c9[ca:ce], qi, ti, o1, oq, ot, mask)
                equal = equal and bool(np.array_equal(oq, q_steps_h[j]))
                prev[i] = (oq.copy(), ot.copy())
                n_cmp += 1
    return {"wall_s": wall, "steps": T, "sequences": S, "pairs": P, "q": q_out, "bitwise_equal_to_one_call_per_frame": equal,
            "n_compared": n_cmp}


def secondary_lines(device, capi, quick=False):
    """BASELINE configs 3, 4, 5 and the whole PNEC::Solve chain on this GPU, each {workload, value, unit, ms_per_step,
    roofline, parity}; an entry that fails reports its error instead of taking the headline down with it."""
    import torch

    from oracle import pnec_oracle as po
    from pnec_amd import Batch, select_best
    from pnec_amd import simulation as sim
    from pnec_amd import tracks as tk
    out = []
    cores = po.usable_threads()   # (capped by the cgroup quota: 128 OpenMP threads on a 16-CPU quota run slower than 32)

    def guarded(fn):
        try:
            out.append(fn())
        except Exception as e:   # noqa: BLE001 -- the line must come out
            out.append({"workload": fn.__name__, "error": f"{type(e).__name__}: {e}"})
        torch.cuda.synchronize()

    def timed(fn, steps, warm):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        best = None
        for _ in range(2):   # twice, the quieter run counts (a host hiccup inside a ten-step loop is a third of it)
            e0 = [torch.cuda.Event(enable_timing=True) for _ in range(steps)]
            e1 = [torch.cuda.Event(enable_timing=True) for _ in range(steps)]
            t0 = time.perf_counter()
            r = None
            for i in range(steps):
                e0[i].record()
                r = fn()
                e1[i].record()
            torch.cuda.synchronize()
            wall = (time.perf_counter() - t0) / steps * 1e3
            dev = float(np.mean([a.elapsed_time(b) for a, b in zip(e0, e1)]))
            if best is None or wall < best[1]:
                best = (r, wall, dev)
        return best

    sizes = tk.kitti_all_sizes()
    P = int(len(sizes))

    def kitti_all_refinement():
        tr = tk.kitti_all_shard(0, P, device=device)
        with Batch(capi.MODE_TARGET, tr.offsets, device=device.index) as b:
            b.fill(tr.bvs1, tr.bvs2, tr.covs)
            q0, t0 = tr.init_q.contiguous(), tr.init_t.contiguous()
            opts = capi.default_options()
            res, wall, kms = timed(lambda: b.solve(q0, t0, reg=1e-13, options=opts), 10 if quick else 30, 5)
            roof = refinement_roofline(b, res, kms, True, capi, b.describe_launch(opts),
                                       executed_passes(b, q0, t0, opts, capi, reg=1e-13))
            k = 256
            m = int(tr.offsets[k])
            oq = po.solve_batch(po.MODE_TARGET, np.asarray(tr.offsets[:k + 1]), tr.bvs1[:m].cpu().numpy(), tr.bvs2[:m].cpu().numpy(),
                                po.covs_to_colmajor9(tr.covs[:m].cpu().numpy()), None, 1e-13, q0[:k].cpu().numpy(),
                                t0[:k].cpu().numpy(), options=po.default_options(jacobian_mode=po.JAC_NUMERIC_CENTRAL),
                                num_threads=cores)
            ang = _quat_angles(res.q[:k].cpu().numpy(), oq[0])
            its_eq = int((res.iterations[:k].cpu().numpy() == oq[3]).sum())
        return {"workload": "configs[4] on one GPU: all KITTI 00-10 frame pairs (23 190 ragged pairs, synthetic KITTI-like stand-in), "
                            "refinement with Ceres-default termination", "value": P / (wall * 1e-3), "unit": "solves/s",
                "ms_per_step": wall, "kernel_ms": kms, "lm_iterations_mean": float(res.iterations.double().mean()),
                "roofline": roof, "parity": {"max_rot_err_rad": float(ang.max()), "median_rot_err_rad": float(np.median(ang)),
                                             "n_pairs": k, "iteration_counts_equal": its_eq, "tolerance_rad": 1e-6,
                                             "against": "oracle (central differences + Ceres LM policy), same inputs"}}

    def kitti_all_chain():
        # The eigensolver scheme of the headline entry is the FACADE's default (2: MINPACK-style LM on the reduced-Cayley
        # gradient, the restatement believed to be what opengv runs -- what a drop-in user of pnec::rel_pose_estimation::PNEC
        # gets); the C ABI's default (0: damped Newton, the fastest) and scheme 1 follow under `other_eigensolver_schemes`.
        MAIN = 2
        tr = tk.kitti_all_shard(0, P, device=device, outlier_frac=0.10)
        q0, t0 = tr.init_q.contiguous(), tr.init_t.contiguous()
        batches = []
        for _ in range(3):
            b = Batch(capi.MODE_TARGET, tr.offsets, device=device.index)
            b.fill(tr.bvs1, tr.bvs2, tr.covs)
            batches.append(b)
        k = 512
        m = int(tr.offsets[k])
        chk = (np.asarray(tr.offsets[:k + 1]), tr.bvs1[:m].cpu().numpy(), tr.bvs2[:m].cpu().numpy(),
               tr.covs[:m].cpu().numpy(), q0[:k].cpu().numpy())
        offs = chk[0]

        def checker(sch):
            po.set_eigensolver_scheme(sch)
            try:
                return po.solve_chain_batch(*chk, seed=1, num_threads=cores)
            finally:
                po.set_eigensolver_scheme(0)

        def parity_of(sch, qd, md):
            o = checker(sch)
            a_s = _quat_angles(qd[:k].cpu().numpy(), o["q"])
            same = np.array([(md[offs[i]:offs[i + 1]].cpu().numpy().astype(bool) == o["mask"][offs[i]:offs[i + 1]]).all()
                             for i in range(k)])
            return a_s, same
        try:
            po_main = capi.default_pipeline_options(eigensolver_scheme=MAIN)
            one = lambda: batches[0].solve_pipeline(q0, t0, options=po_main, want_inliers=True)
            (q, t, mask, cnt), wall1, dev1 = timed(one, 6 if quick else 12, 3)
            streams = [torch.cuda.Stream(device=device) for _ in range(3)]
            steps = 9 if quick else 18
            for i in range(3):
                with torch.cuda.stream(streams[i]):
                    batches[i].solve_pipeline(q0, t0, options=po_main, want_inliers=True)
            torch.cuda.synchronize()
            t_0 = time.perf_counter()
            for i in range(steps):
                with torch.cuda.stream(streams[i % 3]):
                    batches[i % 3].solve_pipeline(q0, t0, options=po_main, want_inliers=True)
            torch.cuda.synchronize()
            wall3 = (time.perf_counter() - t_0) / steps * 1e3
            # opt-in launch-order hint: the previous call solved the same batch, so the hint is perfect (an upper bound)
            batches[0].launch_order_hint(True)
            one()
            (qh, th, _mh, _ch), wall1h, _ = timed(one, 6 if quick else 12, 2)
            batches[0].launch_order_hint(False)
            hint_equal = bool(torch.equal(qh, q) and torch.equal(th, t))
            batches[0].set_eigensolver_scheme(MAIN)          # (the stage-by-stage calls take the batch's scheme)
            stage_ms, res, sel, sel_payload = chain_stage_times(batches[0], q0, t0)
            assert torch.equal(res.q, q)                       # the stages one by one == the one call, bit for bit
            counts = load_chain_counts("kitti_all_chain" + ("" if MAIN == 0 else f"_scheme{MAIN}"), P, int(sizes.sum()))
            roofs = chain_stage_rooflines(counts, {"ransac_es": stage_ms["ransac_es"] + stage_ms["inlier_extraction"],
                                                   "weighted_es": stage_ms["weighted_es"]},
                                          batches[0].payload_bytes // 2, sel_payload,
                                          refinement_roofline(sel, res, stage_ms["refinement"], True, capi))
            batches[0].set_eigensolver_scheme(0)
            ang, same = parity_of(MAIN, q, mask)
            # Scheme 2's LM-on-the-gradient stalls on a flat valley of |grad| where M's two smallest eigenvalues lie close
            # (~1 % of pairs): device and checker then end at points their rounding picks (tests/test_chain_scale_gpu.py
            # checks at 20 000 pairs that every such pair IS a stall on the checker's side).  The line's tolerance applies
            # to the pairs with identical inlier masks up to the 99th percentile; the rest is counted and printed.
            a_ok = ang[same]
            p99 = float(np.percentile(a_ok, 99)) if a_ok.size else 0.0
            n_over = int((a_ok > 1e-6).sum())
            gate = bool(same.mean() >= 0.99 and p99 <= 1e-8 and n_over <= max(2, k // 100))
            # the other two restatements of opengv's eigenvalue minimisation, each against the checker running the same scheme
            schemes = {}
            for sch, name in ((0, "damped Newton (the C ABI's default)"), (1, "descent [EXT]")):
                po_s = capi.default_pipeline_options(eigensolver_scheme=sch)
                call = lambda: batches[0].solve_pipeline(q0, t0, options=po_s, want_inliers=True)
                (qs_, ts_, ms_, cs_), wall_s, _ = timed(call, 4 if quick else 8, 2)
                a_s, same_s = parity_of(sch, qs_, ms_)
                schemes[str(sch)] = {"eigenvalue_minimisation": name, "pairs_per_s_one_call_at_a_time": P / (wall_s * 1e-3),
                                     "ms_per_step_one_call_at_a_time": wall_s,
                                     "parity": {"n_pairs": k, "inlier_masks_identical": int(same_s.sum()),
                                                "max_rot_err_rad_pairs_with_identical_masks": float(a_s[same_s].max()) if same_s.any() else None,
                                                "p99_rot_err_rad": float(np.percentile(a_s, 99)),
                                                "against": "the oracle's chain running the same scheme, same inputs and draws"}}
        finally:
            for b in batches:
                b.close()
        return {"workload": "PNEC::Solve, whole chain with the reference's default Options (RANSAC eigensolver, InlierExtraction, "
                            "weighted eigensolver + SCF, refinement) over all KITTI 00-10 frame pairs (23 190 ragged pairs, "
                            "synthetic stand-in, 10 % gross mismatches), one pnec_hip_solve_pipeline call per step, eigensolver "
                            "scheme 2 (the C++ facade's default)",
                "value": P / (wall3 * 1e-3), "unit": "pairs/s", "ms_per_step": wall3, "steps_in_flight": 3,
                "pairs_per_s_one_call_at_a_time": P / (wall1 * 1e-3), "ms_per_step_one_call_at_a_time": wall1,
                "pairs_per_s_one_call_with_launch_order_hint": P / (wall1h * 1e-3),
                "launch_order_hint_note": "opt-in (pnec_hip_problem_launch_order_hint): pairs that needed more than one round of "
                                          "hypotheses in the previous call go first; here the previous call solved the same batch "
                                          "(a perfect hint); results bitwise equal: " + str(hint_equal),
                "stage_ms_stage_by_stage": stage_ms, "roofline": roofs,
                "inlier_share_mean": float((cnt.double() / torch.as_tensor(sizes, dtype=torch.float64, device=device)).mean()),
                "eigensolver_scheme": MAIN, "eigenvalue_minimisation": "lm on the reduced-Cayley gradient [EXT]",
                "other_eigensolver_schemes": schemes,
                # the plain maximum over the mask-identical pairs when it is within the tolerance (the usual case on this sample);
                # otherwise the 99th percentile, with the stalled pairs counted below -- or, when a gate fails, the worst pair
                "parity": {"max_rot_err_rad": (float(a_ok.max()) if (gate and a_ok.size and float(a_ok.max()) <= 1e-6)
                                               else (p99 if gate else float(ang.max()))),
                           "max_rot_err_rad_is": ("the maximum over the pairs with identical inlier masks"
                                                  if (gate and a_ok.size and float(a_ok.max()) <= 1e-6) else
                                                  "the 99th percentile over the pairs with identical inlier masks (the rest: counted "
                                                  "below; an iteration that stalls ends where its rounding puts it)"),
                           "max_rot_err_rad_pairs_with_identical_masks": float(a_ok.max()) if a_ok.size else None,
                           "n_pairs_over_1e-6_rad_with_identical_masks": n_over,
                           "median_rot_err_rad": float(np.median(ang)), "n_pairs": k,
                           "inlier_masks_identical": bool(same.mean() >= 0.99), "n_inlier_masks_identical": int(same.sum()),
                           "tolerance_rad": 1e-6, "gates_passed": gate,
                           "against": "the oracle's chain (pnec_oracle_solve_chain_batch) running scheme 2, same inputs and draws"}}

    def multi_hypothesis():
        Bp, N, H = 64, 4096, 64
        g = sim.generate(Bp, N, seed=9, device=device)
        gen = torch.Generator(device=device)
        gen.manual_seed(5)
        hyp = torch.randn(Bp * H, 3, generator=gen, dtype=torch.float64, device=device)
        hyp = hyp / hyp.norm(dim=1, keepdim=True)
        hyp[::H] = g.init_t
        opts = capi.default_options(max_num_iterations=10, check_convergence=0)
        with Batch.uniform(capi.MODE_TARGET, Bp, N, device=device.index) as b:
            b.fill(g.bvs1.reshape(-1, 3), g.bvs2.reshape(-1, 3), g.covs2.reshape(-1, 3, 3))

            def go():
                r = b.solve(g.init_q, None, options=opts, hyp_t=hyp, n_hyp=H)
                select_best(r.cost, H)
                return r
            res, wall, kms = timed(go, 5 if quick else 10, 2)
            roof = refinement_roofline(b, res, kms, False, capi, b.describe_launch(opts),
                                       executed_passes(b, g.init_q, None, opts, capi, hyp_t=hyp, n_hyp=H), primary="valu_fp64")
            # Parity sample: one hypothesis of every pair, 64 solves.  A random t-hat start can be 180 degrees off, and ten LM
            # iterations from there are not converged: such a trajectory amplifies the ROUNDING of the reference's central
            # difference quotient (eps |r| / h ~ 1e-8 of the Jacobian) to 1e-6 .. 1e-2 rad at iteration ten.  The CPU path
            # shows it by itself: run again with its difference step h scaled by a factor in [0.5, 2] -- the same derivative
            # to 1e-15 -- it lands that far from its own first result on about ten of the 64 solves
            # (`reference_path_self_distance`; tools/verify_numeric_jacobian.py, profiles/r06_numeric_jacobian_config4.jsonl).
            # So: the north star's tolerance is applied where the reference path reproduces itself (self-distance <= 1e-7);
            # on the others the device must be no further from the reference path than twice that path's own self-distance;
            # iteration counts and termination codes must agree on ALL, the analytic twin within 1e-5 on ALL; and every
            # number, the unreproducible solves' included, is printed.
            kw10 = dict(max_num_iterations=10, check_convergence=0)
            picks = [(pp, (7 * pp + 3) % H) for pp in range(Bp)]
            idx = torch.tensor([pp * H + h for pp, h in picks], device=device)
            hs = hyp[idx].contiguous()
            rn = b.solve(g.init_q, None, options=capi.default_options(flags=capi.OPT_JACOBIAN_NUMERIC_CENTRAL, **kw10), hyp_t=hs, n_hyp=1)
            torch.cuda.synchronize()
            offs = np.arange(Bp + 1, dtype=np.int64) * N
            cpu_in = (po.MODE_TARGET, offs, g.bvs1.reshape(-1, 3).cpu().numpy(), g.bvs2.reshape(-1, 3).cpu().numpy(),
                      po.covs_to_colmajor9(g.covs2.reshape(-1, 3, 3).cpu().numpy()), None, 1e-13, g.init_q.cpu().numpy(), None)

            def cpu(jm, scale=1.0):
                po.set_numeric_step_scale(scale)
                try:
                    o_ = po.solve_batch(*cpu_in, n_hyp=1, hyp_t=hs.cpu().numpy(), options=po.default_options(jacobian_mode=jm, **kw10),
                                        num_threads=cores)
                finally:
                    po.set_numeric_step_scale(1.0)
                return o_[0], o_[3], o_[4]
            ref_q, ref_it, ref_st = cpu(po.JAC_NUMERIC_CENTRAL)
            twin_q = cpu(po.JAC_ANALYTIC)[0]
            scales = (1.0 + 2.0 ** -10, 1.0 - 2.0 ** -10, 1.0 + 2.0 ** -7, 2.0, 0.5)
            self_d = np.max(np.stack([_quat_angles(ref_q, cpu(po.JAC_NUMERIC_CENTRAL, sc)[0]) for sc in scales]), axis=0)
            dq = res.q[idx].cpu().numpy()
            d_ref, d_twin = _quat_angles(dq, ref_q), _quat_angles(dq, twin_q)
            d_num = _quat_angles(rn.q.cpu().numpy(), ref_q)
            repro = self_d <= 1e-7
            its_ok = bool((res.iterations[idx].cpu().numpy() == ref_it).all() and (res.status[idx].cpu().numpy() == ref_st).all())
            within_self = bool((d_ref[~repro] <= 2.0 * self_d[~repro]).all())
            worst = float(d_ref[repro].max()) if repro.any() else 0.0
            gate_ok = bool(its_ok and within_self and worst <= 1e-6 and float(d_twin.max()) <= 1e-5 and int((~repro).sum()) <= Bp // 3)
            if not gate_ok:
                worst = max(worst, float(d_ref.max()))     # a failed gate must fail the line's tolerance check
        return {"workload": "configs[3]: multi-hypothesis, 64 pairs x 4096 correspondences x 64 random t-hat starts sharing the pair's "
                            "payload (4096 solves per launch; one 8-wavefront block per pair and group of 8 hypotheses: the payload "
                            "on chip once per group, all 8 LM steps at the same time), 10 LM iterations, + select_best",
                "value": Bp * H / (wall * 1e-3), "unit": "solves/s", "ms_per_step": wall, "kernel_ms": kms, "roofline": roof,
                "parity": {"max_rot_err_rad": worst, "n_solves": len(picks), "iteration_counts_equal": its_ok, "tolerance_rad": 1e-6,
                           "tolerance_applies_to": "the solves whose reference path reproduces itself (self-distance <= 1e-7 rad)",
                           "n_solves_whose_reference_path_reproduces_itself": int(repro.sum()),
                           "max_rot_err_rad_all_solves": float(d_ref.max()),
                           "reference_path_self_distance": {
                               "what": "the CPU reference path (central differences + Ceres LM policy) run again with its difference "
                                       "step scaled by " + ", ".join(f"{x:.6g}" for x in scales) + " (the same derivative to 1e-15): "
                                       "max distance of those runs from the unscaled one, per solve",
                               "max_rad": float(self_d.max()), "n_above_1e-7": int((~repro).sum()), "n_above_1e-6": int((self_d > 1e-6).sum())},
                           "unreproducible_solves": {"n": int((~repro).sum()),
                                                     "device_within_twice_the_reference_paths_self_distance": within_self,
                                                     "max_rot_err_rad": float(d_ref[~repro].max()) if (~repro).any() else 0.0,
                                                     "max_ratio_to_self_distance": float((d_ref[~repro] / self_d[~repro]).max()) if (~repro).any() else 0.0},
                           "max_rot_err_rad_vs_analytic_twin_all_solves": float(d_twin.max()),
                           "device_numeric_jacobian_mode_vs_reference_path": {
                               "what": "PNEC_HIP_OPT_JACOBIAN_NUMERIC_CENTRAL (the reference's own differentiation on the device, verification only)",
                               "max_rot_err_rad_reproducible_solves": float(d_num[repro].max()) if repro.any() else 0.0,
                               "max_rot_err_rad_all_solves": float(d_num.max()),
                               "iteration_counts_equal": bool((rn.iterations.cpu().numpy() == ref_it).all())},
                           "gates_passed": gate_ok,
                           "against": "oracle (central differences + Ceres LM policy), sampled (pair, hypothesis) solves"}}

    def kitti00_streamed():
        from pnec_amd.streaming import Stream
        Ps = 1000 if quick else 4541
        offsets, f1, f2, c2, R_gt, t_gt, q0, t0 = sim.generate_kitti_like(Ps, mean_corr=500, seed=3)
        f1, f2, c2, q0, t0 = (x.numpy() for x in (f1, f2, c2, q0, t0))
        with Batch(capi.MODE_TARGET, offsets, device=device.index) as b:
            b.fill(f1, f2, c2)
            ref = b.solve(q0, t0)
        gq = np.zeros((Ps, 4))
        with Stream(max_corr=int(np.diff(offsets).max()), slots=8, device=device.index) as st:
            for rep in range(2):                       # the first pass warms the handle
                tickets, nxt = [], 0
                t_0 = time.perf_counter()
                for pp in range(Ps):
                    a, e = offsets[pp], offsets[pp + 1]
                    tickets.append(st.submit(capi.MODE_TARGET, f1[a:e], f2[a:e], c2[a:e], None, q0[pp], t0[pp]))
                    if len(tickets) == 8:
                        gq[nxt] = st.wait(tickets.pop(0)).q[0]
                        nxt += 1
                while tickets:
                    gq[nxt] = st.wait(tickets.pop(0)).q[0]
                    nxt += 1
                wall = time.perf_counter() - t_0
        return {"workload": f"configs[2]: a KITTI-00-like sequence of {Ps} consecutive frame pairs (synthetic stand-in, ~500 ragged "
                            "correspondences) STREAMED one pair per call (pnec_hip_stream_*: host arrays in, pose out, 8 in flight), "
                            "refinement with Ceres-default termination; includes the host-side copies and the Python loop",
                "value": Ps / wall, "unit": "pairs/s", "ms_per_step": wall / Ps * 1e3,
                "roofline": {"bound": "latency", "note": "one pair per launch: bounded by the submit path (memcpy into pinned staging + one "
                                                         "launch + flag poll), not by a device roof; the same pairs as one batch: see the "
                                                         "kitti_all entry"},
                "parity": {"bitwise_equal_to_the_batched_call": bool(np.array_equal(gq, np.asarray(ref.q))), "n_pairs": Ps}}

    def kitti00_per_frame_chain():
        # The reference's ACTUAL call pattern (VERDICT r5 "missing" 5): one PNEC::Solve -- the whole chain -- per frame, each
        # start pose depending on the previous frame's result (FrameProcessing::ProcessFrame, src/odometry/frame_processing.cc:
        # 57-145: prev_rel_rotation -> Frame2Frame::Align -> PNECAlign, frame2frame.cc:122-141 -> PNEC::Solve): nothing of
        # frame k + 1 can start before frame k's pose is back on the host.  pnec_hip_frame_solve on a persistent handle.
        from pnec_amd.frame import FrameSolver
        Ps = 400 if quick else 4541
        offsets, f1, f2, c2, R_gt, t_gt, q0, t0 = sim.generate_kitti_like(Ps, mean_corr=500, seed=3)
        f1, f2, c2 = (x.numpy() for x in (f1, f2, c2))
        offsets = np.asarray(offsets, dtype=np.int64)
        # the caller's arrays as the reference holds them (std::vector<Eigen::Matrix3d>: column-major 3x3), made once
        c9 = np.ascontiguousarray(np.transpose(c2, (0, 2, 1)).reshape(-1, 9))
        out = {}
        for name, kw in (("default", dict()), ("odometry", dict(use_nec=1, use_ceres=0))):
            inits_q, inits_t, gq = np.zeros((Ps, 4)), np.zeros((Ps, 3)), np.zeros((Ps, 4))
            with FrameSolver(max_corr=int(np.diff(offsets).max()), device=device.index) as fs:
                o = capi.default_pipeline_options(eigensolver_scheme=2, **kw)
                mask_buf = np.zeros(int(np.diff(offsets).max()), dtype=np.uint8)
                gt = np.zeros((Ps, 3))
                for rep in range(2):                   # the first pass warms the handle
                    inits_q[0], inits_t[0] = (0.0, 0.0, 0.0, 1.0), (0.0, 0.0, 1.0)
                    t_0 = time.perf_counter()
                    for pp in range(Ps):
                        a, e = int(offsets[pp]), int(offsets[pp + 1])
                        # (RANSAC draws as pair pp of the sequence, so that the batched call below draws the same)
                        o.first_pair_id = pp
                        fs.solve_raw(e - a, f1[a:e], f2[a:e], c9[a:e], inits_q[pp], inits_t[pp], o, gq[pp], gt[pp], mask_buf)
                        if pp + 1 < Ps:                # the next frame starts from this frame's result
                            inits_q[pp + 1], inits_t[pp + 1] = gq[pp], gt[pp]
                    wall = time.perf_counter() - t_0
            # the same frames, with the start poses the sequence produced, as ONE batched call: bit for bit the same poses
            with Batch(capi.MODE_TARGET, offsets, device=device.index) as b:
                b.fill(f1, f2, c2)
                bq, _bt = b.solve_pipeline(inits_q, inits_t, options=capi.default_pipeline_options(eigensolver_scheme=2, **kw))
            gt_err = _quat_angles(gq, np.stack([po.quat_from_rot(R) for R in R_gt.numpy()]))
            out[name] = {"frames_per_s": Ps / wall, "us_per_frame": wall / Ps * 1e6,
                         "bitwise_equal_to_the_batched_call": bool(np.array_equal(gq, np.asarray(bq))),
                         "median_rot_err_rad_vs_ground_truth": float(np.median(gt_err))}
        d = out["default"]
        return {"workload": f"configs[2], the reference's call pattern: a KITTI-00-like sequence of {Ps} consecutive frames "
                            "(synthetic stand-in, ~500 ragged correspondences), ONE PNEC::Solve (whole chain, reference-default "
                            "Options, eigensolver scheme 2) per frame through pnec_hip_frame_solve, every start pose = the "
                            "previous frame's result (sequentially dependent: frame_processing.cc:57-145); host arrays in, pose "
                            "out, includes the Python loop",
                "value": d["frames_per_s"], "unit": "pairs/s", "ms_per_step": d["us_per_frame"] * 1e-3,
                "us_per_frame": d["us_per_frame"],
                "odometry_options": {"what": "use_nec, no refinement -- what Frame2Frame forces (frame2frame.cc:127-128)", **out["odometry"]},
                "roofline": {"bound": "latency", "note": "one frame = one wavefront's worth of sequential work per stage (RANSAC "
                                                         "hypotheses' minimisations one trip after the other); bounded by dependent-"
                                                         "instruction latency and four launches, not by a device roof"},
                "parity": {"bitwise_equal_to_the_batched_call": bool(d["bitwise_equal_to_the_batched_call"] and
                                                                     out["odometry"]["bitwise_equal_to_the_batched_call"]),
                           "n_pairs": Ps, "median_rot_err_rad_vs_ground_truth": d["median_rot_err_rad_vs_ground_truth"],
                           "note": "the batched call's parity against the oracle's chain: the chain entry above and "
                                   "tests/test_chain_scale_gpu.py"}}

    def kitti_all_sequences_in_lockstep():
        # configs[4] the way an odometry would run it on ONE device: the eleven sequences advance side by side -- the
        # reference fans them out as processes (scripts/parallel_kitti.sh:60-69) -- one batched PNEC::Solve per time step over
        # the sequences still running, and every start pose is the previous step's result of the same sequence
        # (frame_processing.cc:57-145) WITHOUT leaving the device: step k + 1's call takes step k's output tensors as its
        # init poses, everything is enqueued on one stream, the host never waits for a pose.
        res = lockstep_sequences(device, capi, tk, quick)
        return {"workload": "configs[4] as eleven odometry runs in lockstep on one GPU: all KITTI 00-10 frame pairs (23 190, synthetic "
                            "stand-in, 10 % gross mismatches), one batched whole-chain PNEC::Solve (scheme 2) per time step over the "
                            "sequences still running, every start pose = the previous step's result of that sequence, chained ON THE "
                            "DEVICE (no host round trip between steps)",
                "value": res["pairs"] / res["wall_s"], "unit": "pairs/s", "ms_per_step": res["wall_s"] / res["steps"] * 1e3,
                "time_steps": res["steps"], "sequences": res["sequences"], "pairs": res["pairs"],
                "roofline": {"bound": "latency", "note": "a time step is a batch of <= 11 pairs: one wavefront per pair and stage, five "
                                                         "dependent launches; bounded by a stage's sequential trips, not by a device roof"},
                "parity": {"bitwise_equal_to_one_call_per_frame": res["bitwise_equal_to_one_call_per_frame"],
                           "n_pairs_compared": res["n_compared"],
                           "note": "the first steps of every sequence re-run one frame per call (pnec_hip_frame_solve) with the same "
                                   "start poses and RANSAC pair ids"}}

    for fn in (kitti_all_refinement, kitti_all_chain, multi_hypothesis, kitti00_streamed, kitti00_per_frame_chain,
               kitti_all_sequences_in_lockstep):
        guarded(fn)
    return out


# ---------------------------------------------------------------------------------------------------
# --dump-outputs: what the timed path computed in its last step, so that two builds can be compared output for output
DUMP_LIMIT_BYTES = 64 * 10**6


def record_arrays(rec, chain=False):
    """The per-pair results a caller of the timed path receives, from the [P, 10] records of pack_records (q, t, cost,
    iterations, status); --chain steps carry the inlier count in the iterations column and nothing in the others."""
    rec = np.asarray(rec.detach().cpu() if hasattr(rec, "detach") else rec, dtype=np.float64)
    out = {"q": rec[:, 0:4], "t": rec[:, 4:7]}
    if chain:
        out["inlier_count"] = rec[:, 8]
    else:
        out.update(cost=rec[:, 7], iterations=rec[:, 8], status=rec[:, 9])
    return out


def dump_outputs(path, arrays, limit=DUMP_LIMIT_BYTES):
    """Every array as <path>/<name>.npy in float64.  Beyond `limit` bytes in all, the same fixed, seeded sample of rows of
    each, sorted, and the rows' indices as row_index.npy."""
    arrays = {k: np.ascontiguousarray(v, dtype=np.float64) for k, v in arrays.items()}
    n = len(next(iter(arrays.values())))
    if sum(a.nbytes for a in arrays.values()) > limit:
        row = sum(a.nbytes for a in arrays.values()) // max(n, 1) + 8
        idx = np.sort(np.random.default_rng(0).choice(n, size=(limit - 4096) // row, replace=False))   # (room for the headers)
        arrays = {k: np.ascontiguousarray(a[idx]) for k, a in arrays.items()}
        arrays["row_index"] = idx.astype(np.float64)
    os.makedirs(path, exist_ok=True)
    for k, a in arrays.items():
        np.save(os.path.join(path, k + ".npy"), a)


# ---------------------------------------------------------------------------------------------------
def run(args):
    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != max(1, args.gpus):
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    cpu = args.dry_run_cpu
    if not cpu:
        if not torch.cuda.is_available():
            raise SystemExit("bench.py needs a GPU: the solver has no CPU fallback")
        if args.share_gpu:
            local_rank = 0
        if torch.cuda.device_count() <= local_rank:
            raise SystemExit(f"rank {rank}: no GPU {local_rank} ({torch.cuda.device_count()} visible)")
        device = torch.device("cuda", local_rank)
        torch.cuda.set_device(device)
    else:
        device = torch.device("cpu")
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        join_job(args, world, rank, device, cpu)
        assert dist.get_world_size() == args.gpus, (dist.get_world_size(), args.gpus)
    n_ranks = dist.get_world_size() if world > 1 else 1

    from pnec_amd.distributed import RecordGather
    sh = (build_kitti_all if args.workload == "kitti_all" else build_sim100k)(args, rank, world, device)
    my_pairs = sh.sizes[rank]
    first_global = sum(sh.sizes[:rank])
    if args.chain and args.workload != "kitti_all":
        raise SystemExit("--chain goes with --workload kitti_all")
    in_flight = max(1, args.in_flight) if (args.chain and not cpu) else 1
    gather = RecordGather(world, rank, sizes=sh.sizes, device=None if (cpu or args.sync_gather) else device,
                          host_staged=args.share_gpu, slots=in_flight + 1)
    host_collective = world > 1 and not cpu and (args.share_gpu and args.sync_gather)
    outs = [None] * gather.SLOTS
    which = [0]   # the copy of the batch (and the stream) the next step runs on

    if cpu:
        from pnec_amd.batch import SolveResult
        opts = launch = None
        step_no = [0]

        def solve(slot):
            # stub: records a real solve would produce in shape, with the GLOBAL pair index as "cost" so
            # that rank 0 can check the gathered order; no arithmetic of the solver is imitated
            idx = torch.arange(first_global, first_global + my_pairs, dtype=torch.float64)
            q = torch.zeros(my_pairs, 4, dtype=torch.float64)
            q[:, 3] = 1.0
            t = torch.zeros(my_pairs, 3, dtype=torch.float64)
            t[:, 2] = 1.0
            step_no[0] += 1
            return SolveResult(q, t, idx, torch.full((my_pairs,), step_no[0], dtype=torch.int32),
                               torch.full((my_pairs,), rank, dtype=torch.int32))
    else:
        from pnec_amd import capi
        opts = capi.default_options(corr_per_lane=args.cpl, waves_per_pair=args.wpp,
                                    lds_corr_per_lane=args.ldsk, **sh.opts)
        launch = sh.batch.describe_launch(opts)

        if args.chain:
            from pnec_amd.batch import SolveResult

            # pair p of this shard draws its RANSAC samples as pair first_global + p of the whole set: the records do
            # not depend on the number of ranks
            popts = capi.default_pipeline_options(first_pair_id=first_global, eigensolver_scheme=args.es_scheme)

            def solve(slot):
                # one pnec_hip_solve_pipeline call; the record's "iterations" column carries the inlier count
                q, t, _, cnt = sh.batches[which[0]].solve_pipeline(sh.q0, sh.t0, options=popts, want_inliers=True)
                outs[slot] = SolveResult(q, t, torch.zeros(my_pairs, dtype=torch.float64, device=device), cnt,
                                         torch.zeros(my_pairs, dtype=torch.int32, device=device))
                return outs[slot]
        else:
            def solve(slot):
                outs[slot] = sh.batch.solve(sh.q0, sh.t0, reg=1e-13, options=opts, out=outs[slot])
                return outs[slot]

    ev0 = ev1 = None
    if not cpu:
        ev0 = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps)]
        ev1 = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps)]

    streams = [torch.cuda.Stream(device=device) for _ in range(in_flight)] if in_flight > 1 else None

    def step(i=None, overlap=True):
        import contextlib
        ctx = contextlib.nullcontext()
        if streams is not None and overlap:   # this step's launches (and its events, and its gather) on its own stream
            which[0] = (which[0] + 1) % in_flight
            ctx = torch.cuda.stream(streams[which[0]])
        with ctx:
            slot = gather.acquire()
            if i is not None and ev0:
                ev0[i].record()
            res = solve(slot)
            if i is not None and ev1:
                ev1[i].record()
            if host_collective:   # --share-gpu --sync-gather: gloo moves host tensors only
                from pnec_amd.batch import SolveResult as _SR
                gather.submit(slot, _SR(*(x.cpu() for x in (res.q, res.t, res.cost, res.iterations, res.status))))
            else:
                gather.submit(slot, res)
        return res

    def fence():
        if not cpu:
            torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
            if not cpu:
                torch.cuda.synchronize()

    # setup: the first ~10 launches after an idle period run ~4 % slower (clock ramp).  Bring the
    # GPU to its steady clocks before the contract's W untimed warm-up steps, whatever W is.
    setup_launches = 0 if cpu else max(0, 20 - args.warmup)
    for _ in range(setup_launches):
        solve(0)
    if world > 1:   # bring the communicator up outside the timed region whatever W is (first collective = RCCL init)
        step()
        gather.drain()
    for _ in range(args.warmup):
        step()
    gather.drain()
    fence()
    t_start = time.perf_counter()
    res = None
    for i in range(args.steps):
        res = step(i)
    gathered = gather.drain()
    fence()
    elapsed = time.perf_counter() - t_start
    if args.dump_outputs and rank == 0:   # the gathered records of the last timed step, every rank's pairs in order
        dump_outputs(args.dump_outputs, record_arrays(gathered, chain=args.chain))
    per_rank = None
    if world > 1:
        tmax = torch.tensor([elapsed], dtype=torch.float64, device="cpu" if args.share_gpu else device)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        # every rank's own numbers, for the line (after the timed region): wall time of its K steps, device time of one step's
        # launches (events on its stream), device time of the side stream's pack + collective per step, its pairs
        mine = torch.tensor([elapsed,
                             float(np.mean([a.elapsed_time(b) for a, b in zip(ev0, ev1)])) if ev0 else float("nan"),
                             gather.device_ms_per_collective() or float("nan"), float(my_pairs)],
                            dtype=torch.float64, device=tmax.device)
        allr = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(allr, mine)
        per_rank = torch.stack(allr).cpu().numpy()
        elapsed = float(tmax.item())
    one_at_a_time = None
    if args.full and in_flight > 1 and world == 1:   # the same steps one after the other on one stream, for the record
        which[0] = 0
        t1 = time.perf_counter()
        for _ in range(args.steps):
            step(None, overlap=False)
        gather.drain()
        fence()
        one_at_a_time = sh.total_pairs * args.steps / (time.perf_counter() - t1)

    if rank == 0:
        value = sh.total_pairs * args.steps / elapsed
        assert gathered.shape == (sh.total_pairs, 10), (tuple(gathered.shape), sh.total_pairs)
        assert bool(torch.isfinite(gathered[:, :8]).all())
        line = {
            "metric": "PNEC pose solves/sec (512 corr, 10 GN iters)" if args.workload == "sim100k"
                      else ("PNEC::Solve frame pairs/sec, whole chain (all KITTI 00-10 pairs, ragged, reference-default Options)"
                            if args.chain else
                            "PNEC pose solves/sec (all KITTI 00-10 pairs, ragged, Ceres-default termination)"),
            "value": value, "unit": "pairs/s" if args.chain else "solves/s",
            "n_gpus": 1 if (args.share_gpu and not cpu) else n_ranks, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3,
            "higher_is_better": True, "scaling": sh.scaling, "vs_baseline": None, "dtype": "f64",
            "data": sh.data,
            "config": {"workload": sh.workload, "pairs_total": sh.total_pairs, "pairs_per_rank": sh.sizes,
                       "launcher": "torch.distributed.run" if not os.environ.get("PNEC_BENCH_SPAWNED") and world > 1
                                   else ("self-spawned ranks" if world > 1 else "single process"),
                       "sharding": f"independent pairs, {n_ranks} rank(s), one "
                                   f"{'gloo' if (cpu or args.share_gpu) else 'RCCL'} gather of "
                                   f"80-B result records per step" + ("" if args.sync_gather or cpu else
                                                                      ", on a side stream (overlaps the next step)")},
        }
        # digest of the gathered records of the last step (q, t, cost, iterations, status per pair, in pair order):
        # equal across rank counts for the strong-scaling workloads, whose pairs do not depend on the sharding
        line["records_sha256"] = hashlib.sha256(gathered.detach().cpu().contiguous().numpy().tobytes()).hexdigest()
        if per_rank is not None:
            # a SCALE run diagnoses itself: `value` is the slowest rank's wall time; here is every rank's
            line["per_rank"] = {"wall_ms_per_step": [float(x) / args.steps * 1e3 for x in per_rank[:, 0]],
                                "kernel_ms": [None if np.isnan(x) else float(x) for x in per_rank[:, 1]],
                                "gather_ms": [None if np.isnan(x) else float(x) for x in per_rank[:, 2]],
                                "pairs": [int(x) for x in per_rank[:, 3]],
                                "note": "kernel_ms: device time of one step's launches (events on the rank's stream); gather_ms: "
                                        "device time of the side stream's pack + collective of one step (it overlaps the next "
                                        "step's launches); wall_ms_per_step: the rank's own clock around its K steps"}
        if args.share_gpu and not cpu:
            line["shared_gpu"] = {"ranks": n_ranks, "note": "every rank on cuda:0 (plumbing run on a one-GPU box: real "
                                  "solver, partition and device-side gather with world > 1; gloo over pinned host records "
                                  "because RCCL refuses two ranks on one device) -- NOT a scaling measurement",
                                  "collectives_issued": gather.collectives,
                                  # where a step's wall time goes on rank 0 (all steps incl. warm-up, per collective): the
                                  # gloo gather itself (which also waits for the other rank to arrive) and the wait for
                                  # the step's records to reach pinned memory (= for this rank's kernels to have run:
                                  # two processes on one device do not run their kernels side by side, the device is
                                  # time-sliced between their queues)
                                  "host_collective_ms_per_collective": 1e3 * gather.host_collective_s / max(1, gather.collectives),
                                  "wait_for_own_records_ms_per_collective": 1e3 * gather.host_copy_wait_s / max(1, gather.collectives)}
        if cpu:
            # the gathered "cost" column must be the global pair index, in order, from the LAST step
            assert torch.equal(gathered[:, 7], torch.arange(sh.total_pairs, dtype=torch.float64))
            assert bool((gathered[:, 8] == args.warmup + args.steps + (1 if world > 1 else 0)).all())  # + the set-up step
            want_rank = torch.repeat_interleave(torch.arange(world), torch.tensor(sh.sizes)).to(torch.float64)
            assert torch.equal(gathered[:, 9], want_rank)
            line.update({"metric": "DRY RUN (stubbed solve, no GPU): launch/partition/gather plumbing only",
                         "value": None, "dry_run": True, "records_in_order": True})
            if args.workload == "kitti_all":
                line["config"]["corr_per_rank"] = sh.shard_corr
        elif args.chain:
            line["config"].update({"corr_per_rank": sh.shard_corr,
                                   "corr_min_mean_max": [int(sh.pair_sizes.min()), float(sh.pair_sizes.mean()),
                                                         int(sh.pair_sizes.max())],
                                   "options": "reference defaults: RANSAC eigensolver (5000 its max, 10-point samples), "
                                              "weighted_iterations 10 + SCF, Ceres-default refinement"})
            line["config"]["steps_in_flight"] = in_flight
            line["config"]["eigensolver_scheme"] = args.es_scheme
            if args.full:
                # the chain is a handful of kernels of different character: one roofline block per STAGE.
                # Also reported: the device time of this rank's shard per step and the inlier statistics of the last step.
                dev_ms = float(np.mean([a.elapsed_time(b) for a, b in zip(ev0, ev1)]))
                inl = gathered[:, 8].detach().cpu()
                sh.batches[0].set_eigensolver_scheme(args.es_scheme)     # (the stage-by-stage calls take the batch's scheme)
                stage_ms, sres, ssel, sel_payload = chain_stage_times(sh.batches[0], sh.q0, sh.t0)
                counts = load_chain_counts("kitti_all_chain" + ("" if args.es_scheme == 0 else f"_scheme{args.es_scheme}"),
                                           sh.total_pairs, int(sh.pair_sizes.sum())) \
                    if (world == 1 and not args.tracks and args.outliers == 0.10) else None
                line["roofline"] = chain_stage_rooflines(
                    counts, {"ransac_es": stage_ms["ransac_es"] + stage_ms["inlier_extraction"], "weighted_es": stage_ms["weighted_es"]},
                    sh.batches[0].payload_bytes // 2, sel_payload, refinement_roofline(ssel, sres, stage_ms["refinement"], True, capi))
                line["chain"] = {"device_ms_per_step_rank0": dev_ms, "stage_ms_stage_by_stage_rank0": stage_ms,
                                 "steps_in_flight": in_flight,
                                 "pairs_per_s_one_step_at_a_time": one_at_a_time,
                                 "in_flight_note": "each step in flight runs on its own stream and its own copy of the batch; "
                                                   "device_ms_per_step is one step's span while the others run beside it",
                                 "inlier_share_mean": float((inl / torch.as_tensor(sh.pair_sizes, dtype=torch.float64)).mean()),
                                 "note": "one pnec_hip_solve_pipeline call per step and rank; `roofline` has one block per stage "
                                         "(stage times from the same chain run stage by stage on rank 0; algorithmic flop from the "
                                         "committed work counts, profiles/chain_work_latest.json); stage kernels: "
                                         "profiles/r06_full_pipeline_kernels_scheme2.md"}
        else:
            iters_done = res.iterations.to(torch.float64)
            line["config"].update({
                "lm_iterations_done_min_mean_max": [float(iters_done.min()), float(iters_done.mean()),
                                                    float(iters_done.max())] if my_pairs else None,
                "residual": "PNEC target frame", "launch": launch,
                "setup_launches_before_warmup": setup_launches})
            if args.workload == "sim100k":
                line["config"].update({"pairs_per_gpu": args.pairs, "correspondences": args.corr,
                                       "lm_iterations": args.iters})
            else:
                line["config"].update({"corr_per_rank": sh.shard_corr,
                                       "corr_min_mean_max": [int(sh.pair_sizes.min()), float(sh.pair_sizes.mean()),
                                                             int(sh.pair_sizes.max())]})
            if args.full:
                step_ms = [a.elapsed_time(b) for a, b in zip(ev0, ev1)]
                kernel_ms = float(np.mean(step_ms))
                batch = sh.batch
                payload = batch.payload_bytes                      # bytes the kernel must read once
                passes = float(iters_done.mean()) + 1.0 if my_pairs else 0.0   # iteration zero + one per LM iteration
                achieved_gbs = payload / (kernel_ms * 1e-3) / 1e9
                corr_passes = batch.num_correspondences * passes
                if args.workload == "kitti_all" and my_pairs:      # ragged: weight each pair's passes by its size
                    w = torch.as_tensor(np.diff(batch.offsets), dtype=torch.float64, device=iters_done.device)
                    corr_passes = float(((iters_done + 1.0) * w).sum())
                # a solve that runs into the iteration cap ends with ONE cost-only pass (fixed-count mode: every solve)
                capped = res.status == capi.TERM_MAX_ITERATIONS
                cost_corr = 0.0
                if my_pairs:
                    wts = (torch.as_tensor(np.diff(batch.offsets), dtype=torch.float64, device=iters_done.device)
                           if args.workload == "kitti_all" else
                           torch.full_like(iters_done, batch.num_correspondences / max(my_pairs, 1)))
                    cost_corr = float((capped.to(torch.float64) * wts).sum())
                full_corr = corr_passes - cost_corr
                # what the kernel EXECUTED: it evaluates a candidate cost-only when it expects the step to be rejected (Ceres'
                # own order: residuals first, the Jacobian once the step is accepted) -- one counted launch on the same inputs
                passes_full_if_all_speculated = full_corr
                full_corr, cost_corr = (float(x) for x in executed_passes(batch, sh.q0, sh.t0, opts, capi, reg=1e-13))
                valu_tflops = (FLOP_PER_CORR_PASS * full_corr + FLOP_PER_CORR_COST_PASS * cost_corr) / (kernel_ms * 1e-3) / 1e12
                issue_tflops_equiv = 2 * (VALU_INSTR_PER_CORR_PASS * full_corr + VALU_INSTR_PER_CORR_COST_PASS * cost_corr) \
                    / (kernel_ms * 1e-3) / 1e12
                key = [args.workload, args.pairs if args.workload == "sim100k" else sh.total_pairs,
                       args.corr if args.workload == "sim100k" else 0, args.iters if args.workload == "sim100k" else 0,
                       [launch["corr_per_lane"], launch["waves_per_pair"], launch["lds_corr_per_lane"]]]
                traffic, valu_busy, why = profiled_counters(capi.LIB_PATH, key)
                line["roofline"] = {
                    # the contract's block prices the kernel against HBM (bytes it must read once / its duration);
                    # the roof that BINDS this register-resident kernel is FP64 VALU issue: see bound_binding / 'valu'
                    "bound": "hbm", "bound_binding": "valu_fp64",
                    "binding_frac": valu_tflops / FP64_VALU_PEAK_TFLOPS,
                    "kernel": "lm_solve_kernel<TARGET>", "rank": 0,
                    "achieved": achieved_gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                    "frac": achieved_gbs / HBM_PEAK_GBS, "traffic": traffic, "traffic_note": why,
                    "kernel_ms": kernel_ms,
                    # the spread over the K timed launches: a box whose clocks move shows here (round 6: two boxes at 2.72 ms, one at
                    # 3.03 ms mean whose rocprofv3 trace of the same command read 2.72 min / 2.90 mean); `achieved` / `frac` use the
                    # MEAN, as the contract says
                    "kernel_ms_min_median_max": [float(np.min(step_ms)), float(np.median(step_ms)), float(np.max(step_ms))],
                    "algorithmic_bytes_per_launch": payload,
                    "note": "register-resident design: the payload (96 B/correspondence) is read from HBM "
                            "once per solve, not once per pass, so the kernel is FP64-VALU-bound, not "
                            "HBM-bound; see 'valu' for the binding roof and DESIGN.md",
                    # SURVEY.md 8(d) quotes the streaming model (N x 96 B x passes per solve); against it:
                    "streaming_equivalent_GBs": achieved_gbs * passes,
                    "streaming_equivalent_frac": achieved_gbs * passes / HBM_PEAK_GBS,
                    "valu": {"bound": "valu_fp64", "achieved": valu_tflops, "peak": FP64_VALU_PEAK_TFLOPS,
                             "unit": "TFLOP/s", "frac": valu_tflops / FP64_VALU_PEAK_TFLOPS,
                             "flop_per_corr_pass": FLOP_PER_CORR_PASS, "passes": passes,
                             "cost_only_passes_per_solve": (cost_corr / batch.num_correspondences) if batch.num_correspondences else 0.0,
                             "flop_per_corr_cost_only_pass": FLOP_PER_CORR_COST_PASS,
                             "flop_note": "62 FMA + 28 MUL + 1 rsq per correspondence per full pass = 153 flop in 91 issue slots; "
                                          "a cost-only pass (after a rejected step, at the iteration cap): 67 flop in 43 slots; "
                                          "the flop counted are those of the passes the kernel executed (a counted launch)",
                             "correspondence_passes_executed": {"full": full_corr, "cost_only": cost_corr,
                                                                "full_if_every_candidate_got_its_jacobian": passes_full_if_all_speculated},
                             # the same work priced in issue slots (every VALU instruction = one FMA-sized slot)
                             "issue_slot_frac_useful": issue_tflops_equiv / FP64_VALU_PEAK_TFLOPS,
                             # share of cycles the vector ALU was issuing (any FP64/integer/cross-lane
                             # instruction, useful or bookkeeping), from the committed rocprofv3 SQ counters
                             "issue_busy_frac_profiled": valu_busy},
                }
                if not args.no_cpu_baseline and world == 1 and sh.sample is not None:
                    from oracle import pnec_oracle as po
                    cores = po.max_threads()
                    avail = len(sh.sample[0]) - 1
                    n_sample = args.cpu_sample or int(min(avail, max(64, 32 * cores)))
                    base, parity = cpu_baseline(sh.sample, n_sample, opts, res.q)
                    line["cpu_baseline"] = base
                    line["parity"] = parity
                if args.workload == "sim100k" and world == 1 and not args.no_secondary and not args.no_cpu_baseline:
                    # the other configs + the chain, on this GPU, after the headline's timed region (the headline's batch is
                    # released first: nothing of it is timed any more)
                    sh.batch.close()
                    t_sec = time.perf_counter()
                    line["secondary"] = secondary_lines(device, capi, quick=args.quick_secondary)
                    line["secondary_wall_s"] = time.perf_counter() - t_sec
        print(json.dumps(line), flush=True)

    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def run_single_process(args):
    """One process, N devices, the persistent multi-device handle (include/pnec_hip.h pnec_hip_multi_*): the sim100k
    workload with `--pairs` pairs PER DEVICE (weak scaling, as the rank-per-GPU form), filled once; a step = one
    pnec_hip_multi_solve over all shards (start poses and result records cross PCIe in every step: 136 B per pair --
    the handle's entry points take host arrays; the payload stays resident)."""
    import torch

    from pnec_amd import capi
    from pnec_amd import simulation as sim
    from pnec_amd.multi import MultiBatch, alloc_counters
    N = args.gpus
    devices = [0] * N if args.share_gpu else list(range(N))
    dev = torch.device("cuda:0")
    if args.workload == "kitti_all":
        # the strong-scaling workload through the handle: the SAME pairs, start poses, options and record layout as the
        # rank-per-GPU form gathers, so that `records_sha256` of the two launchers can be compared on the day an N-GPU box
        # runs both (the results do not depend on the device list: tests/test_distributed_gpu.py)
        from pnec_amd import tracks as tk
        sizes = tk.kitti_all_sizes()
        Pk = int(len(sizes))
        tr = tk.kitti_all_shard(0, Pk, device=dev, outlier_frac=args.outliers if args.chain else 0.0)
        f1, f2, cv = tr.bvs1.cpu().numpy(), tr.bvs2.cpu().numpy(), tr.covs.cpu().numpy()
        q0, t0 = tr.init_q.cpu().numpy(), tr.init_t.cpu().numpy()
        off = np.asarray(tr.offsets, dtype=np.int64)
        del tr
        popts = capi.default_pipeline_options(eigensolver_scheme=args.es_scheme)
        ropts = capi.default_options()
        with MultiBatch(devices, capi.MODE_TARGET, Pk, int(off[-1]), int(sizes.max())) as mb:
            mb.fill(off, f1, f2, cv)

            def one():
                if args.chain:
                    q, t, _m, cnt = mb.solve_pipeline(q0, t0, options=popts, want_inliers=True)
                    return np.concatenate([q, t, np.zeros((Pk, 1)), cnt[:, None].astype(np.float64), np.zeros((Pk, 1))], axis=1)
                r = mb.solve(q0, t0, reg=1e-13, options=ropts)
                return np.concatenate([r["q"], r["t"], r["cost"][:, None], r["iterations"][:, None].astype(np.float64),
                                       r["status"][:, None].astype(np.float64)], axis=1)
            for _ in range(max(args.warmup, 2)):
                rec = one()
            t_0 = time.perf_counter()
            for _ in range(args.steps):
                rec = one()
            wall = (time.perf_counter() - t_0) / args.steps * 1e3
            if args.dump_outputs:
                dump_outputs(args.dump_outputs, record_arrays(rec, chain=args.chain))
            bounds = mb.bounds.tolist()
        line = {"metric": ("PNEC::Solve frame pairs/sec, whole chain (all KITTI 00-10 pairs, ragged, reference-default Options)" if args.chain
                           else "PNEC pose solves/sec (all KITTI 00-10 pairs, ragged, Ceres-default termination)"),
                "value": Pk / (wall * 1e-3), "unit": "pairs/s" if args.chain else "solves/s", "n_gpus": 1 if args.share_gpu else N,
                "steps": args.steps, "warmup": args.warmup, "ms_per_step": wall, "higher_is_better": True, "scaling": "strong",
                "vs_baseline": None, "dtype": "f64", "data": "synthetic KITTI-like (no KITTI data in this environment)",
                "config": {"workload": "configs[4]: all KITTI 00-10 frame pairs (23 190 ragged pairs, synthetic stand-in)" +
                                       (f", whole chain, eigensolver scheme {args.es_scheme}" if args.chain else ", refinement"),
                           "parallelism": f"single process, {N} devices (pnec_hip_multi_*: one host thread + batch + stream per "
                                          "device, no collective; host arrays in and out)", "devices": devices, "shard_bounds": bounds},
                "records_sha256": hashlib.sha256(np.ascontiguousarray(rec).tobytes()).hexdigest(),
                "records_note": "the digest of the per-pair records [q t cost iterations status] in pair order: the same "
                                "number `bench.py --gpus N --workload kitti_all [--chain]` prints for its gathered records"}
        print(json.dumps(line), flush=True)
        return 0
    P, C = args.pairs * N, args.corr
    f1, f2, cv, q0, t0 = [], [], [], [], []
    for c0 in range(0, P, 10000):                        # generated on device 0 in chunks, handed over as host arrays
        m = min(10000, P - c0)
        g = sim.generate(m, C, seed=1 + c0, device=dev)
        f1.append(g.bvs1.reshape(-1, 3).cpu().numpy()); f2.append(g.bvs2.reshape(-1, 3).cpu().numpy())
        cv.append(g.covs2.reshape(-1, 3, 3).cpu().numpy()); q0.append(g.init_q.cpu().numpy()); t0.append(g.init_t.cpu().numpy())
        del g
    f1, f2, cv, q0, t0 = (np.concatenate(x) for x in (f1, f2, cv, q0, t0))
    off = np.arange(P + 1, dtype=np.int64) * C
    opts = capi.default_options(max_num_iterations=args.iters, check_convergence=0)
    with MultiBatch(devices, capi.MODE_TARGET, P, P * C, C) as mb:
        mb.fill(off, f1, f2, cv)
        for _ in range(max(args.warmup, 2)):
            res = mb.solve(q0, t0, options=opts)
        a0 = alloc_counters()
        t_0 = time.perf_counter()
        for _ in range(args.steps):
            res = mb.solve(q0, t0, options=opts)
        wall = (time.perf_counter() - t_0) / args.steps * 1e3
        a1 = alloc_counters()
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, {k: res[k] for k in ("q", "t", "cost", "iterations", "status")})
        bounds = mb.bounds.tolist()
    line = {"metric": "PNEC pose solves/sec (512 corr, 10 GN iters)", "value": P / (wall * 1e-3), "unit": "solves/s", "n_gpus": N, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": wall, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f64", "data": "synthetic",
            "config": {"workload": f"configs[1]: {args.pairs} simulated frame pairs x {C} anisotropic-covariance correspondences per "
                                   f"GPU, {args.iters} LM iterations", "parallelism": f"single process, {N} devices "
                       "(pnec_hip_multi_solve: one host thread + batch + stream per device, no collective)",
                       "devices": devices, "shard_bounds": bounds,
                       "per_step_pcie_bytes": P * 136, "note": "start poses in and result records out cross PCIe in every "
                       "step (host-array entry point); the payload is resident; NOT the rank-per-GPU headline form",
                       "hip_malloc_calls_during_timed_steps": a1["hip_malloc_calls"] - a0["hip_malloc_calls"]},
            "all_iterations_done": bool((res["iterations"] == args.iters).all())}
    print(json.dumps(line), flush=True)
    return 0


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    args = parse_args(argv)
    if args.single_process:
        if args.chain and args.workload != "kitti_all":
            sys.exit("--chain goes with --workload kitti_all")
        sys.exit(run_single_process(args))
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(spawn_ranks(args.gpus, argv))
    run(args)


if __name__ == "__main__":
    main()
