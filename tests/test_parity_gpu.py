"""GPU parity suite (-m gpu): the HIP path, called through the C ABI, against the CPU oracle on
the same seeded inputs, against the committed golden vectors, and -- at BASELINE's full size --
through size-independent properties.

Tolerance (BASELINE.json north_star): rotations within 1e-6 rad of the reference-faithful CPU
path (central-difference Jacobian + Ceres LM policy).  Against the oracle's analytic-Jacobian
variant (the same algorithm the kernel runs) the bar is 1e-9 rad.
"""
import math
import os
import sys

import numpy as np
import pytest
import torch

from pnec_amd import Batch, capi, select_best
from pnec_amd import simulation as sim

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_lm_edges_gpu import _oracle_opts  # noqa: E402  (one helper: every field the two option structs share)

pytestmark = pytest.mark.gpu

ROT_TOL_REFERENCE = 1e-6   # rad, vs reference-faithful oracle (north_star)
ROT_TOL_SAME_ALGO = 1e-9   # rad, vs oracle running the kernel's own algorithm


def _rot_err(oracle, Ra, Rb):
    return math.radians(oracle.rotational_difference_deg(Ra, Rb))


def _covs_for(mode, S2):
    """(covs, covs_host) for a residual family, derived deterministically from S2 [n,3,3]"""
    if mode == capi.MODE_NEC:
        return None, None
    if mode == capi.MODE_SYM:
        return S2, np.roll(S2, 1, axis=0) * 0.8
    return S2, None


def _oracle_batch(oracle, mode, offsets, f1, f2, c2, c1, reg, q0, t0, opts, **kw):
    c2_9 = None if c2 is None else oracle.covs_to_colmajor9(c2)
    c1_9 = None if c1 is None else oracle.covs_to_colmajor9(c1)
    return oracle.solve_batch(mode, offsets, f1, f2, c2_9, c1_9, reg, q0, t0, options=opts, **kw)


def _quat_to_R(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def test_device_selftest():
    capi.check(capi.lib().pnec_hip_selftest(0))


def test_objective_matches_reference_goldens(golden_dir):
    """max_num_iterations = 0 returns cost = 1/2 sum r^2 at the start pose: compare the DEVICE's
    residual evaluation with the numbers scripts/pnec/common.py produced."""
    z = np.load(f"{golden_dir}/energy_golden.npz")
    from oracle import pnec_oracle as po
    opts = capi.default_options(max_num_iterations=0)
    checked = 0
    for i in range(int(z["n_cases"])):
        k = f"case{i:03d}_"
        f1, f2, S = z[k + "f1"], z[k + "f2"], z[k + "sigmas"]
        reg = float(z[k + "reg"])
        rots = z[k + "rotations"].reshape(4, 3, 3)
        n = len(f1)
        for mode, key in ((capi.MODE_TARGET, "pnec_energy_rotations"), (capi.MODE_NEC, "nec_energy_rotations")):
            want = z[k + key].reshape(4)
            with Batch.uniform(mode, 4, n) as b:
                b.fill(np.tile(f1, (4, 1)), np.tile(f2, (4, 1)),
                       None if mode == capi.MODE_NEC else np.tile(S, (4, 1, 1)))
                q0 = np.stack([po.quat_from_rot(R) for R in rots])
                t0 = np.tile(z[k + "t"], (4, 1))
                res = b.solve(q0, t0, reg=reg if mode != capi.MODE_NEC else 0.0, options=opts)
            np.testing.assert_allclose(2.0 * res.cost, want, rtol=1e-10)
            assert (res.iterations == 0).all()
            checked += 4
    assert checked == 36 * 8


def test_host_and_symmetric_objectives_match_numbers_the_reference_python_returned(golden_dir):
    """The DEVICE's 1/2 sum r^2 for the Host and Symmetrical functors (max_num_iterations = 0 returns the cost at the start
    pose) against tests/golden/residual_forms_golden.npz -- numbers scripts/pnec/common.py returned for the transformed
    inputs at which its target energy is those functors' (tests/golden/make_golden.py)."""
    from oracle import pnec_oracle as po
    z = np.load(f"{golden_dir}/residual_forms_golden.npz")
    opts = capi.default_options(max_num_iterations=0)
    n = int(z["n_cases"])
    for i in range(n):
        k = f"form{i:03d}_"
        f1, f2, c1, c2, R, t = (z[k + a] for a in ("f1", "f2", "cov1", "cov2", "R", "t"))
        reg = float(z[k + "reg"])
        q0, t0 = po.quat_from_rot(R)[None], t[None]
        off = np.array([0, len(f1)], dtype=np.int64)
        with Batch(capi.MODE_HOST, off) as b:
            b.fill(f1, f2, c1)
            res = b.solve(q0, t0, reg=reg, options=opts)
        np.testing.assert_allclose(2.0 * res.cost, [float(z[k + "host_energy"])], rtol=1e-9)
        with Batch(capi.MODE_SYM, off) as b:
            b.fill(f1, f2, c2, c1)
            res = b.solve(q0, t0, reg=reg, options=opts)
        np.testing.assert_allclose(2.0 * res.cost, [float(z[k + "sym_r2"].sum())], rtol=1e-9)
    assert n == 24


@pytest.mark.parametrize("mode", [capi.MODE_NEC, capi.MODE_TARGET, capi.MODE_HOST, capi.MODE_SYM])
@pytest.mark.parametrize("n_corr", [10, 100, 512])
def test_lm_parity_with_oracle(oracle, mode, n_corr):
    B = 24
    g = sim.generate(B, n_corr, seed=100 + n_corr)
    f1 = g.bvs1.reshape(-1, 3).numpy()
    f2 = g.bvs2.reshape(-1, 3).numpy()
    c2, c1 = _covs_for(mode, g.covs2.reshape(-1, 3, 3).numpy())
    offsets = np.arange(B + 1, dtype=np.int64) * n_corr
    reg = 1e-13
    opts = capi.default_options()
    with Batch(mode, offsets) as b:
        b.fill(f1, f2, c2, c1)
        res = b.solve(g.init_q.numpy(), g.init_t.numpy(), reg=reg, options=opts)
    for jm, tol in ((oracle.JAC_ANALYTIC, ROT_TOL_SAME_ALGO), (oracle.JAC_NUMERIC_CENTRAL, ROT_TOL_REFERENCE)):
        q, t, cost, it, st = _oracle_batch(oracle, mode, offsets, f1, f2, c2, c1, reg,
                                           g.init_q.numpy(), g.init_t.numpy(),
                                           _oracle_opts(oracle, opts, jm))
        worst = max(_rot_err(oracle, _quat_to_R(res.q[p]), _quat_to_R(q[p])) for p in range(B))
        assert worst <= tol, (jm, worst)
        np.testing.assert_array_equal(res.iterations, it)
        np.testing.assert_array_equal(res.status, st)
        np.testing.assert_allclose(res.cost, cost, rtol=1e-9)
        tdot = np.abs(np.sum(res.t * t, axis=1))
        assert (tdot > 1 - 1e-10).all()
    # the optimiser did something and ended near the ground truth
    gt_err = max(_rot_err(oracle, _quat_to_R(res.q[p]), g.R_gt[p].numpy()) for p in range(B))
    assert gt_err < 0.02


def test_fixed_iteration_mode_matches_oracle(oracle):
    """the throughput configuration: exactly 10 LM iterations, convergence tests off"""
    B, N = 16, 512
    g = sim.generate(B, N, seed=7)
    f1, f2 = g.bvs1.reshape(-1, 3).numpy(), g.bvs2.reshape(-1, 3).numpy()
    c2 = g.covs2.reshape(-1, 3, 3).numpy()
    offsets = np.arange(B + 1, dtype=np.int64) * N
    opts = capi.default_options(max_num_iterations=10, check_convergence=0)
    with Batch(capi.MODE_TARGET, offsets) as b:
        b.fill(f1, f2, c2)
        res = b.solve(g.init_q.numpy(), g.init_t.numpy(), options=opts)
    assert (res.iterations == 10).all() and (res.status == 3).all()
    q, t, cost, it, st = _oracle_batch(oracle, capi.MODE_TARGET, offsets, f1, f2, c2, None, 1e-13,
                                       g.init_q.numpy(), g.init_t.numpy(),
                                       _oracle_opts(oracle, opts, oracle.JAC_NUMERIC_CENTRAL))
    assert (it == 10).all()
    worst = max(_rot_err(oracle, _quat_to_R(res.q[p]), _quat_to_R(q[p])) for p in range(B))
    assert worst <= ROT_TOL_REFERENCE


def _ragged_case(oracle, counts, seed):
    counts = np.asarray(counts, dtype=np.int64)
    offsets = np.concatenate([[0], np.cumsum(counts)])
    B, M = len(counts), int(offsets[-1])
    g = sim.generate(1, M, seed=seed)
    f1, f2 = g.bvs1[0].numpy(), g.bvs2[0].numpy()
    c2 = g.covs2[0].numpy()
    q0 = np.tile(g.init_q[0].numpy(), (B, 1))
    t0 = np.tile(g.init_t[0].numpy(), (B, 1))
    opts = capi.default_options()
    with Batch(capi.MODE_TARGET, offsets) as b:
        assert b.max_correspondences == counts.max()
        launch = b.describe_launch()
        b.fill(f1, f2, c2)
        res = b.solve(q0, t0, options=opts)
    q, t, cost, it, st = _oracle_batch(oracle, capi.MODE_TARGET, offsets, f1, f2, c2, None, 1e-13,
                                       q0, t0, _oracle_opts(oracle, opts, oracle.JAC_ANALYTIC))
    for p in range(B):
        if counts[p] >= 63:   # well-posed pairs (tiny ones are rank-deficient: any LM wanders)
            assert res.status[p] == st[p] and res.iterations[p] == it[p], counts[p]
            assert _rot_err(oracle, _quat_to_R(res.q[p]), _quat_to_R(q[p])) <= 1e-8, counts[p]
    assert np.isfinite(res.q).all() and np.isfinite(res.t).all()
    return launch, res, st, q0


def test_ragged_batch_with_empty_and_tiny_pairs(oracle):
    """ragged sizes inside one on-chip-resident launch (largest pair 2500 -> 8 wavefronts x 8
    correspondences per lane); the empty pair stops at iteration 0 on the gradient tolerance
    (zero cost, zero gradient) and returns its start pose"""
    launch, res, st, q0 = _ragged_case(
        oracle, [0, 1, 5, 63, 64, 65, 127, 300, 512, 700, 1025, 2048, 2500], seed=31)
    # describe_launch reports the geometry of the LARGEST pair; smaller pairs of a ragged batch run
    # in their own, smaller-geometry launches (bucketing) with identical results
    assert launch["resident"] is True and launch["threads_per_block"] == 512
    assert res.status[0] == st[0] == 2 and res.iterations[0] == 0
    np.testing.assert_allclose(res.q[0], q0[0] / np.linalg.norm(q0[0]), atol=1e-15)


def test_pairs_larger_than_on_chip_capacity_stream(oracle):
    """> 4096 correspondences: the streaming kernel re-reads the payload every pass"""
    launch, res, st, q0 = _ragged_case(oracle, [4097, 100, 6000], seed=33)
    assert launch["resident"] is False


@pytest.mark.parametrize("n_corr,geometries", [
    (512, [(8, 1, 3), (8, 1, 0), (4, 2, 0), (1, 8, 0), (8, 2, 3), (4, 4, 0), (0, 0, 0)]),
    (100, [(2, 1, 0), (4, 1, 0), (8, 1, 3), (1, 8, 0)]),
    (2000, [(8, 4, 3), (4, 8, 0), (8, 8, 3), (0, 0, 0)]),
])
def test_launch_geometries_agree(n_corr, geometries):
    """on-chip-resident geometries (registers / registers + LDS, 1..8 wavefronts per solve) and
    the streaming kernel are the same computation"""
    B = 6
    g = sim.generate(B, n_corr, seed=n_corr)
    ref = None
    with Batch.uniform(capi.MODE_TARGET, B, n_corr) as b:
        b.fill(g.bvs1.reshape(-1, 3).numpy(), g.bvs2.reshape(-1, 3).numpy(),
               g.covs2.reshape(-1, 3, 3).numpy())
        for cpl, wpp, ldsk in geometries:
            if cpl == 0:   # streaming: corr_per_lane 0 with an explicit wavefront count
                opts = capi.default_options(corr_per_lane=0, waves_per_pair=8)
            else:
                opts = capi.default_options(corr_per_lane=cpl, waves_per_pair=wpp,
                                            lds_corr_per_lane=ldsk)
            d = b.describe_launch(opts)
            assert d["resident"] == (cpl != 0)
            res = b.solve(g.init_q.numpy(), g.init_t.numpy(), options=opts)
            if ref is None:
                ref = res
                continue
            np.testing.assert_array_equal(res.iterations, ref.iterations)
            np.testing.assert_array_equal(res.status, ref.status)
            np.testing.assert_allclose(res.q, ref.q, atol=1e-11)
            np.testing.assert_allclose(res.cost, ref.cost, rtol=1e-10)
        with pytest.raises(capi.PnecHipError):   # too small for the pair
            b.solve(g.init_q.numpy(), g.init_t.numpy(),
                    options=capi.default_options(corr_per_lane=1, waves_per_pair=1))
        with pytest.raises(capi.PnecHipError):   # a geometry that is not built
            b.solve(g.init_q.numpy(), g.init_t.numpy(),
                    options=capi.default_options(corr_per_lane=8, waves_per_pair=8, lds_corr_per_lane=1))


def test_multi_hypothesis_shares_payload(oracle):
    """64 t-hat restarts per pair (BASELINE config 4 shape, small): every hypothesis equals an
    independent oracle solve from that start; select_best picks the lowest cost."""
    B, N, H = 3, 1024, 16
    g = sim.generate(B, N, seed=41)
    rng = np.random.default_rng(3)
    hyp = rng.normal(size=(B * H, 3))
    hyp /= np.linalg.norm(hyp, axis=1, keepdims=True)
    hyp[::H] = g.init_t.numpy()       # hypothesis 0 = the good start
    f1, f2 = g.bvs1.reshape(-1, 3).numpy(), g.bvs2.reshape(-1, 3).numpy()
    c2 = g.covs2.reshape(-1, 3, 3).numpy()
    offsets = np.arange(B + 1, dtype=np.int64) * N
    opts = capi.default_options()
    with Batch(capi.MODE_TARGET, offsets) as b:
        b.fill(f1, f2, c2)
        res = b.solve(g.init_q.numpy(), None, options=opts, hyp_t=hyp, n_hyp=H)
    q, t, cost, it, st = _oracle_batch(oracle, capi.MODE_TARGET, offsets, f1, f2, c2, None, 1e-13,
                                       g.init_q.numpy(), g.init_t.numpy(),
                                       _oracle_opts(oracle, opts, oracle.JAC_ANALYTIC),
                                       n_hyp=H, hyp_t=hyp)
    np.testing.assert_array_equal(res.iterations, it)
    np.testing.assert_array_equal(res.status, st)
    for s in range(B * H):
        assert _rot_err(oracle, _quat_to_R(res.q[s]), _quat_to_R(q[s])) <= 1e-7
    best = select_best(res.cost, H)
    np.testing.assert_array_equal(best, np.argmin(cost.reshape(B, H), axis=1))


def test_device_space_equals_host_space():
    B, N = 10, 256
    g = sim.generate(B, N, seed=51, device="cuda:0")
    with Batch.uniform(capi.MODE_TARGET, B, N) as b:
        b.fill(g.bvs1.reshape(-1, 3), g.bvs2.reshape(-1, 3), g.covs2.reshape(-1, 3, 3))
        dev = b.solve(g.init_q, g.init_t)
        torch.cuda.synchronize()
        cf_dev = b.cost_function(dev.q, dev.t)
        host = b.solve(g.init_q.cpu().numpy(), g.init_t.cpu().numpy())
        cf_host = b.cost_function(host.q, host.t)
    np.testing.assert_array_equal(dev.q.cpu().numpy(), host.q)
    np.testing.assert_array_equal(dev.t.cpu().numpy(), host.t)
    np.testing.assert_array_equal(dev.iterations.cpu().numpy(), host.iterations)
    np.testing.assert_array_equal(cf_dev.cpu().numpy(), cf_host)


def test_cost_function_metric(oracle):
    B, N = 4, 77
    g = sim.generate(B, N, seed=61)
    with Batch.uniform(capi.MODE_TARGET, B, N) as b:
        b.fill(g.bvs1.reshape(-1, 3).numpy(), g.bvs2.reshape(-1, 3).numpy(),
               g.covs2.reshape(-1, 3, 3).numpy())
        got = b.cost_function(g.init_q.numpy(), g.init_t.numpy())
    for p in range(B):
        want = oracle.cost_function(g.bvs1[p].numpy(), g.bvs2[p].numpy(), g.covs2[p].numpy(),
                                    g.init_R[p].numpy(), g.init_t[p].numpy())
        assert got[p] == pytest.approx(want, rel=1e-10)


def test_nan_input_is_reported_not_hidden():
    B, N = 3, 64
    g = sim.generate(B, N, seed=71)
    f1 = g.bvs1.reshape(-1, 3).numpy().copy()
    f1[N + 5, 1] = np.nan
    with Batch.uniform(capi.MODE_TARGET, B, N) as b:
        b.fill(f1, g.bvs2.reshape(-1, 3).numpy(), g.covs2.reshape(-1, 3, 3).numpy())
        res = b.solve(g.init_q.numpy(), g.init_t.numpy())
    assert res.status[1] == 6 and res.iterations[1] == 0
    assert res.status[0] != 6 and res.status[2] != 6
    assert np.isfinite(res.q).all()   # the last iterate (= the start) is returned, as the reference would


def test_kitti_like_forward_motion_near_chart_singularity(oracle):
    """t ~ +z is where the (theta,phi) chart degenerates (Appendix C12); parity must hold there."""
    offsets, f1, f2, c2, R_gt, t_gt, q0, t0 = sim.generate_kitti_like(40, mean_corr=480, seed=5)
    f1, f2, c2, q0, t0 = (x.numpy() for x in (f1, f2, c2, q0, t0))
    opts = capi.default_options()
    with Batch(capi.MODE_TARGET, offsets) as b:
        b.fill(f1, f2, c2)
        res = b.solve(q0, t0, options=opts)
    q, t, cost, it, st = _oracle_batch(oracle, capi.MODE_TARGET, offsets, f1, f2, c2, None, 1e-13,
                                       q0, t0, _oracle_opts(oracle, opts, oracle.JAC_NUMERIC_CENTRAL))
    worst = max(_rot_err(oracle, _quat_to_R(res.q[p]), _quat_to_R(q[p])) for p in range(40))
    assert worst <= ROT_TOL_REFERENCE, worst
    np.testing.assert_array_equal(res.status, st)


def test_full_size_batch_properties(oracle):
    """BASELINE config 2 (100k pairs x 512 anisotropic correspondences) through properties that
    do not need a CPU solve of the whole batch: finite results, cost never above the start cost,
    idempotence (re-solving from the result moves < 1e-6 rad), plus oracle parity on a sample."""
    B, N = 100_000, 512
    chunk = 10_000
    batch = Batch.uniform(capi.MODE_TARGET, B, N)
    qs, ts, keep = [], [], {}
    for c in range(B // chunk):
        g = sim.generate(chunk, N, seed=1000 + c, device="cuda:0")
        batch.fill(g.bvs1.reshape(-1, 3), g.bvs2.reshape(-1, 3), g.covs2.reshape(-1, 3, 3),
                   first_pair=c * chunk, n_pairs=chunk)
        qs.append(g.init_q)
        ts.append(g.init_t)
        keep[c] = (g.bvs1[:4].cpu().numpy(), g.bvs2[:4].cpu().numpy(), g.covs2[:4].cpu().numpy())
        del g
    q0, t0 = torch.cat(qs), torch.cat(ts)
    start = batch.solve(q0, t0, options=capi.default_options(max_num_iterations=0))
    res = batch.solve(q0, t0)
    again = batch.solve(res.q, res.t)
    torch.cuda.synchronize()
    assert torch.isfinite(res.q).all() and torch.isfinite(res.cost).all()
    assert (res.cost <= start.cost * (1 + 1e-12)).all()
    # Ceres-default termination: nearly every solve stops on a tolerance; a handful (~3e-4 of this
    # distribution) crawl to the 50-iteration cap -- the oracle does exactly the same on them
    converged = res.status <= 2
    assert float(converged.double().mean()) > 0.999
    assert int(res.iterations.max()) <= 50
    # idempotence of converged solves: re-solving from the result moves less than the tolerance
    # ball of the stopping rule (function_tolerance 1e-6 ~ a few 1e-6 rad here), never far
    dq = (res.q * again.q).sum(-1).abs().clamp(max=1.0)
    ang = 2 * torch.acos(dq)
    assert float(ang[converged].max()) < 2e-5
    assert float((ang[converged] < 1e-6).double().mean()) > 0.99
    assert int(again.iterations[converged].max()) <= 50
    # oracle parity on 4 pairs of every chunk (reference-faithful numeric Jacobian)
    worst = 0.0
    rq = res.q.cpu().numpy()
    for c, (f1, f2, c2) in keep.items():
        for j in range(4):
            p = c * chunk + j
            s = oracle.solve(oracle.MODE_TARGET, f1[j], f2[j], c2[j], None, 1e-13,
                             q0[p].cpu().numpy(), t0[p].cpu().numpy(), oracle.default_options())
            worst = max(worst, _rot_err(oracle, _quat_to_R(rq[p]), s.R))
            assert int(res.iterations[p]) == s.iterations
    assert worst <= ROT_TOL_REFERENCE, worst

    # ---- the BENCH mode on the same 100k x 512 batch: exactly 10 LM iterations, no convergence tests
    # (bench.py's timed configuration), against the central-difference oracle run the same way
    fixed = capi.default_options(max_num_iterations=10, check_convergence=0)
    r10 = batch.solve(q0, t0, options=fixed)
    torch.cuda.synchronize()
    assert torch.isfinite(r10.q).all() and torch.isfinite(r10.cost).all()
    assert int(r10.iterations.min()) == 10 and int(r10.iterations.max()) == 10
    assert bool((r10.status == 3).all())                       # PNEC_HIP_TERM_MAX_ITERATIONS
    assert (r10.cost <= start.cost * (1 + 1e-12)).all()
    assert float(((r10.q * r10.q).sum(-1) - 1).abs().max()) < 1e-12
    o10 = _oracle_opts(oracle, fixed, oracle.JAC_NUMERIC_CENTRAL)
    rq10, rc10 = r10.q.cpu().numpy(), r10.cost.cpu().numpy()
    worst10 = 0.0
    for c, (f1, f2, c2) in keep.items():
        for j in range(4):
            p = c * chunk + j
            s = oracle.solve(oracle.MODE_TARGET, f1[j], f2[j], c2[j], None, 1e-13,
                             q0[p].cpu().numpy(), t0[p].cpu().numpy(), o10)
            worst10 = max(worst10, _rot_err(oracle, _quat_to_R(rq10[p]), s.R))
            assert s.iterations == 10
            assert rc10[p] == pytest.approx(s.cost, rel=1e-6)
    assert worst10 <= ROT_TOL_REFERENCE, worst10
    batch.close()


def test_config4_full_size_multi_hypothesis(oracle):
    """BASELINE config 4 at its stated size: 64 pairs x 4096 correspondences x 64 random t-hat starts
    (4096 solves sharing 64 payloads, the (8,8,3) geometry: 8 wavefronts per solve).  Properties on all
    4096 solves; reference-faithful oracle parity on sampled (pair, hypothesis) solves."""
    Bp, N, H = 64, 4096, 64
    dev = torch.device("cuda:0")
    g = sim.generate(Bp, N, seed=9, device=dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)
    hyp = torch.randn(Bp * H, 3, generator=gen, dtype=torch.float64, device=dev)
    hyp = hyp / hyp.norm(dim=1, keepdim=True)
    hyp[::H] = g.init_t                                        # hypothesis 0 = the good start
    with Batch.uniform(capi.MODE_TARGET, Bp, N) as b:
        b.fill(g.bvs1.reshape(-1, 3), g.bvs2.reshape(-1, 3), g.covs2.reshape(-1, 3, 3))
        assert b.describe_launch()["waves_per_pair"] == 8 and b.describe_launch()["resident"]
        for opts in (capi.default_options(max_num_iterations=10, check_convergence=0), capi.default_options()):
            start = b.solve(g.init_q, None, options=capi.default_options(max_num_iterations=0), hyp_t=hyp, n_hyp=H)
            res = b.solve(g.init_q, None, options=opts, hyp_t=hyp, n_hyp=H)
            torch.cuda.synchronize()
            assert res.q.shape == (Bp * H, 4)
            assert torch.isfinite(res.q).all() and torch.isfinite(res.t).all() and torch.isfinite(res.cost).all()
            assert float(((res.q * res.q).sum(-1) - 1).abs().max()) < 1e-12
            assert float(((res.t * res.t).sum(-1) - 1).abs().max()) < 1e-12
            assert (res.cost <= start.cost * (1 + 1e-12)).all()          # LM never ends above its start
            best = select_best(res.cost, H)
            assert torch.equal(best.long(), res.cost.reshape(Bp, H).argmin(dim=1))
            # the good start wins or ties, and its rotation is the ground truth to the noise level
            cost = res.cost.reshape(Bp, H)
            assert bool((cost[:, 0] <= cost.min(dim=1).values * (1 + 1e-6)).all())
            R = res.rotation_matrices().reshape(Bp, H, 3, 3)[:, 0].cpu().numpy()
            for p in range(0, Bp, 8):
                assert _rot_err(oracle, R[p], g.R_gt[p].cpu().numpy()) < 0.01
            # sampled oracle parity (central differences + Ceres LM policy, the same options)
            oo = _oracle_opts(oracle, opts, oracle.JAC_NUMERIC_CENTRAL)
            rng = np.random.default_rng(17)
            samples = [(0, 0), (63, 63)] + [(int(rng.integers(Bp)), int(rng.integers(H))) for _ in range(8)]
            rq, rit, rst = res.q.cpu().numpy(), res.iterations.cpu().numpy(), res.status.cpu().numpy()
            for (p, h) in samples:
                s = oracle.solve(oracle.MODE_TARGET, g.bvs1[p].cpu().numpy(), g.bvs2[p].cpu().numpy(),
                                 g.covs2[p].cpu().numpy(), None, 1e-13, g.init_q[p].cpu().numpy(),
                                 hyp[p * H + h].cpu().numpy(), oo)
                assert rit[p * H + h] == s.iterations, (p, h, rit[p * H + h], s.iterations)
                assert rst[p * H + h] == s.status, (p, h)
                assert _rot_err(oracle, _quat_to_R(rq[p * H + h]), s.R) <= ROT_TOL_REFERENCE, (p, h)


def test_unscented_transform_device_vs_oracle_and_goldens(oracle, golden_dir):
    """input-side row: UnscentedTransform + Unproject for a batch of keypoints"""
    from pnec_amd import frontend
    z = np.load(f"{golden_dir}/math_golden.npz")
    bvs, covs = frontend.unscented_transform(z["ut_points"], z["ut_covs"])
    np.testing.assert_allclose(covs, z["ut_out"], rtol=1e-10, atol=1e-22)
    np.testing.assert_allclose(bvs, z["ut_points"] / np.linalg.norm(z["ut_points"], axis=1, keepdims=True), atol=1e-15)
    # the omnidirectional branch against the reference's Python (round-4 goldens: tangent-diagonal covariances)
    bo, co = frontend.unscented_transform(z["omni_points"], z["omni_covs"], np.eye(3), 1.0, frontend.CAMERA_OMNIDIRECTIONAL)
    np.testing.assert_allclose(co, z["omni_out"], rtol=1e-9, atol=1e-20)
    np.testing.assert_allclose(bo, z["omni_points"] / np.linalg.norm(z["omni_points"], axis=1, keepdims=True), atol=1e-15)
    rng = np.random.default_rng(8)
    n = 5000
    K = np.array([[718.856, 0, 607.19], [0, 718.856, 185.22], [0, 0, 1.0]])
    Kinv = np.linalg.inv(K)
    pts = np.stack([rng.uniform(0, 1241, n), rng.uniform(0, 376, n), np.ones(n)], 1)
    A = rng.normal(size=(n, 2, 2)) * 0.3
    cov = np.zeros((n, 3, 3))
    cov[:, :2, :2] = A @ np.transpose(A, (0, 2, 1)) + 0.01 * np.eye(2)
    for model, mu, cv, Ki in ((frontend.CAMERA_PINHOLE, pts, cov, Kinv),
                              (frontend.CAMERA_OMNIDIRECTIONAL, None, None, None)):
        if model == frontend.CAMERA_OMNIDIRECTIONAL:
            v = rng.normal(size=(n, 3))
            v /= np.linalg.norm(v, axis=1, keepdims=True)
            v[:, 2] = np.abs(v[:, 2]) * 0.9 + 0.05   # away from the antipode of +z
            mu = v / np.linalg.norm(v, axis=1, keepdims=True) * 800.0
            Rb = sim.rotation_between_z_and(torch.from_numpy(mu / 800.0)).numpy()
            cv = Rb @ cov @ np.transpose(Rb, (0, 2, 1))
            Ki = np.eye(3)
        b_dev, c_dev = frontend.unscented_transform(mu, cv, Ki, 1.0, model)
        for i in range(0, n, 97):
            want = oracle.unscented_transform(mu[i], cv[i], Ki, 1.0, model)
            np.testing.assert_allclose(c_dev[i], want, rtol=1e-9, atol=1e-20)
        # device space == host space
        bt, ct = frontend.unscented_transform(torch.from_numpy(mu).cuda(), torch.from_numpy(cv).cuda(),
                                              torch.from_numpy(Ki).cuda(), 1.0, model)
        np.testing.assert_array_equal(ct.cpu().numpy(), c_dev)
        np.testing.assert_array_equal(bt.cpu().numpy(), b_dev)


def test_nec_eigensolver_device_vs_oracle(oracle):
    """SURVEY 8f row 2 (without RANSAC): PNEC::Eigensolver = eigenvalue minimisation + TranslationFromM"""
    counts = np.array([64, 100, 256, 512, 700, 37], dtype=np.int64)
    offsets = np.concatenate([[0], np.cumsum(counts)])
    g = sim.generate(1, int(offsets[-1]), seed=91)
    poses = sim.generate(len(counts), 4, seed=92)
    f1, f2 = g.bvs1[0].numpy(), g.bvs2[0].numpy()
    q0 = np.tile(g.init_q[0].numpy(), (len(counts), 1))
    with Batch(capi.MODE_NEC, offsets) as b:
        b.fill(f1, f2)
        q, t = b.nec_eigensolver(q0)
    R0 = g.init_R[0].numpy()
    for p, n in enumerate(counts):
        sl = slice(offsets[p], offsets[p + 1])
        Ro, to = oracle.nec_eigensolver(f1[sl], f2[sl], R0)
        assert _rot_err(oracle, _quat_to_R(q[p]), Ro) <= 1e-8, n
        assert abs(abs(t[p] @ to) - 1) < 1e-9, n
        assert t[p][np.argmax(np.abs(t[p]))] > 0            # deterministic eigenvector sign
    del poses


# Declared deviation of the weighted stage: the device keeps the rotation once an
# eigensolver call has converged and stops the SCF at its fixed point; the reference (and the oracle)
# re-run the eigensolver in all 9 rounds and always take 10 SCF steps.  Measured over 2 048 pairs
# (tools/verify_frontend_literal.py -> profiles/r02_literal.json): device vs literal oracle max 5.5e-9 rad
# (p99 2e-11); the early exits alone (oracle twin vs literal oracle) 2.6e-11.
WEIGHTED_EARLY_EXIT_BOUND = 1e-7   # rad, device vs the LITERAL oracle (18x the measured worst case)


def test_weighted_eigensolver_device_vs_oracle(oracle):
    """PNEC::WeightedEigensolver (weights, eigensolver, Fibonacci search, scf) against the
    literal oracle (every round re-runs the eigensolver, 10 SCF steps) within the declared bound, and
    against the oracle's early-exit twin (same control flow as the kernel) tightly"""
    B, N = 6, 512
    g = sim.generate(B, N, seed=93)
    f1, f2 = g.bvs1.reshape(-1, 3).numpy(), g.bvs2.reshape(-1, 3).numpy()
    c2 = g.covs2.reshape(-1, 3, 3).numpy()
    with Batch.uniform(capi.MODE_TARGET, B, N) as b:
        b.fill(f1, f2, c2)
        qn, tn = b.nec_eigensolver(g.init_q.numpy())
        for iters in (10, 2, 1):
            qw, tw = b.weighted_eigensolver(qn, tn, 1e-13, iters)
            for p in range(B):
                sl = slice(p * N, (p + 1) * N)
                Rn = _quat_to_R(qn[p])
                Ro, to = oracle.weighted_eigensolver(f1[sl], f2[sl], c2[sl], Rn, tn[p], 1e-13, iters)
                assert _rot_err(oracle, _quat_to_R(qw[p]), Ro) <= WEIGHTED_EARLY_EXIT_BOUND, (iters, p)
                assert abs(abs(tw[p] @ to) - 1) < 1e-8, (iters, p)
                Rt, tt = oracle.weighted_eigensolver(f1[sl], f2[sl], c2[sl], Rn, tn[p], 1e-13, iters,
                                                     device_early_exits=True)
                assert _rot_err(oracle, _quat_to_R(qw[p]), Rt) <= 1e-8, (iters, p)
                assert abs(abs(tw[p] @ tt) - 1) < 1e-8, (iters, p)
        # device space, and the whole PNEC::Solve chain (no RANSAC): ES -> weighted ES -> refinement
        qd, td = b.weighted_eigensolver(torch.from_numpy(qn).cuda(), torch.from_numpy(tn).cuda(), 1e-13, 10)
        res = b.solve(qd, td)
        torch.cuda.synchronize()
        qw10, tw10 = b.weighted_eigensolver(qn, tn, 1e-13, 10)
        np.testing.assert_allclose(qd.cpu().numpy(), qw10, atol=1e-14)
    for p in range(B):
        assert _rot_err(oracle, _quat_to_R(res.q[p].cpu().numpy()), g.R_gt[p].numpy()) < 0.01


def test_weighted_eigensolver_ragged_batch_forms_device_vs_oracle(oracle):
    """a ragged batch picks the weighted stage's form PER PAIR: <= 512 correspondences resident on one wavefront,
    up to 1024 on two, 2048 on four, 4096 on eight (every sum exchanged between them), more streaming -- all of
    them against the literal oracle and its early-exit twin, in one launch"""
    sizes = [300, 512, 513, 640, 1000, 1024, 1025, 1500, 2048, 2049, 3000, 4096, 4100]
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    g = sim.generate(len(sizes), max(sizes), seed=97)
    f1 = np.concatenate([g.bvs1[p].numpy()[:n] for p, n in enumerate(sizes)])
    f2 = np.concatenate([g.bvs2[p].numpy()[:n] for p, n in enumerate(sizes)])
    c2 = np.concatenate([g.covs2[p].numpy()[:n] for p, n in enumerate(sizes)])
    with Batch(capi.MODE_TARGET, offsets) as b:
        b.fill(f1, f2, c2)
        qn, tn = b.nec_eigensolver(g.init_q.numpy())
        qw, tw = b.weighted_eigensolver(qn, tn, 1e-13, 10)
    for p, n in enumerate(sizes):
        sl = slice(offsets[p], offsets[p + 1])
        Rn = _quat_to_R(qn[p])
        Ro, to = oracle.weighted_eigensolver(f1[sl], f2[sl], c2[sl], Rn, tn[p], 1e-13, 10)
        assert _rot_err(oracle, _quat_to_R(qw[p]), Ro) <= WEIGHTED_EARLY_EXIT_BOUND, (n, "literal")
        assert abs(abs(tw[p] @ to) - 1) < 1e-8, n
        Rt, tt = oracle.weighted_eigensolver(f1[sl], f2[sl], c2[sl], Rn, tn[p], 1e-13, 10, device_early_exits=True)
        assert _rot_err(oracle, _quat_to_R(qw[p]), Rt) <= 1e-8, (n, "twin")
        assert abs(abs(tw[p] @ tt) - 1) < 1e-8, n


def test_weighted_stage_launch_order_and_chained_minimisations_on_degenerate_pairs(oracle, monkeypatch):
    """Round 5: (a) every eigenvalue minimisation of the weighted stage runs before the weighted kernel, chained (a call
    that ended at the iteration cap is followed by another from its result); (b) the kernel takes the pairs in an order
    made from the flatness of their minimum, long pairs first.  Neither may change a bit of what comes out.  The set:
    1 200 pairs of 5..11 correspondences, noise up to 0.5, starts up to |v| ~ 1 (about one in ten first calls ends at the
    cap there) -- far outside the use case, where a Newton iteration's end depends on the last bits of its start, so the
    agreement with the checker's sequential twin is exact-to-rounding only for the near starts and a share for the far."""
    rng = np.random.default_rng(5)
    F1, F2, C2, sizes, Q, T, VS = [], [], [], [], [], [], []
    for _ in range(1200):
        n = int(rng.integers(5, 12))
        f1 = rng.normal(size=(n, 3)); f1[:, 2] = abs(f1[:, 2]) + 1; f1 /= np.linalg.norm(f1, axis=1, keepdims=True)
        f2 = f1 + rng.normal(size=(n, 3)) * rng.choice([1e-3, 1e-2, 1e-1, 0.5]); f2 /= np.linalg.norm(f2, axis=1, keepdims=True)
        vs = rng.choice([0.01, 0.3, 1.0])
        A = rng.normal(size=(n, 3, 3)) * 1e-3
        t = rng.normal(size=3)
        F1.append(f1); F2.append(f2); C2.append(A @ A.transpose(0, 2, 1) + 1e-7 * np.eye(3)); sizes.append(n); VS.append(vs)
        Q.append(oracle.quat_from_rot(oracle.cayley_to_rot(rng.normal(size=3) * vs))); T.append(t / np.linalg.norm(t))
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    f1, f2, c2, q0, t0, VS = np.concatenate(F1), np.concatenate(F2), np.concatenate(C2), np.array(Q), np.array(T), np.array(VS)
    res = {}
    for index_order in ("0", "1"):
        monkeypatch.setenv("PNEC_WES_INDEX_ORDER", index_order)   # (read at every launch: "1" = blocks take pairs in index order)
        with Batch(capi.MODE_TARGET, off) as b:
            b.fill(f1, f2, c2)
            res[index_order] = b.weighted_eigensolver(q0, t0, 1e-13, 10)
    monkeypatch.delenv("PNEC_WES_INDEX_ORDER")
    np.testing.assert_array_equal(res["0"][0], res["1"][0])
    np.testing.assert_array_equal(res["0"][1], res["1"][1])
    qw, tw = res["0"]
    err = np.empty(len(sizes))
    for p in range(len(sizes)):
        sl = slice(off[p], off[p + 1])
        Rt, _ = oracle.weighted_eigensolver(f1[sl], f2[sl], c2[sl], oracle.rot_from_quat(q0[p]), t0[p], 1e-13, 10, device_early_exits=True)
        err[p] = _rot_err(oracle, _quat_to_R(qw[p]), Rt)
    assert np.isfinite(err).all()
    assert err[VS == 0.01].max() <= 1e-6 and np.quantile(err[VS == 0.01], 0.99) <= 1e-8   # (5 points, noise 0.5: ill-conditioned)
    assert (err[VS == 0.3] <= 1e-8).mean() >= 0.9 and (err[VS == 1.0] <= 1e-8).mean() >= 0.7


def test_ransac_eigensolver_and_inlier_selection_device_vs_oracle(oracle):
    """SURVEY 8f row 2 with RANSAC (pnec.cc:239-272) + InlierExtraction (pnec.cc:210-229): same
    counter-based draws on both sides -> same inlier sets, same rotations"""
    counts = np.array([300, 512, 128, 8, 40], dtype=np.int64)
    offsets = np.concatenate([[0], np.cumsum(counts)])
    B = len(counts)
    g = sim.generate(B, 512, seed=95)
    rng = np.random.default_rng(2)
    f1 = np.concatenate([g.bvs1[p].numpy()[:n] for p, n in enumerate(counts)])
    f2 = np.concatenate([g.bvs2[p].numpy()[:n] for p, n in enumerate(counts)])
    c2 = np.concatenate([g.covs2[p].numpy()[:n] for p, n in enumerate(counts)])
    for p in range(B):                       # 20 % gross outliers in every pair
        sl = np.arange(offsets[p], offsets[p + 1])
        bad = rng.choice(sl, len(sl) // 5, replace=False)
        v = rng.normal(size=(len(bad), 3))
        f2[bad] = v / np.linalg.norm(v, axis=1, keepdims=True)
    with Batch(capi.MODE_TARGET, offsets) as b:
        b.fill(f1, f2, c2)
        q, t, mask, cnt, its = b.ransac_eigensolver(g.init_q.numpy(), seed=11, max_iterations=5000,
                                                    sample_size=10, threshold=1e-6)
        for p in range(B):
            sl = slice(offsets[p], offsets[p + 1])
            Ro, to, mo, ito = oracle.ransac_eigensolver(f1[sl], f2[sl], g.init_R[p].numpy(), seed=11, pair_id=p)
            assert its[p] == ito, (p, its[p], ito)
            np.testing.assert_array_equal(mask[sl].astype(bool), mo)
            assert cnt[p] == mo.sum()
            # the eigensolver stops at |grad| <= 1e-14 (1 + |lambda|) n, which leaves the iterate free
            # within ~1e-8 rad: device and oracle may stop one Newton step apart
            assert _rot_err(oracle, _quat_to_R(q[p]), Ro) <= 1e-7
            assert abs(abs(t[p] @ to) - 1) < 1e-7
        # InlierExtraction: the selected batch holds exactly the inliers, in order
        sel = b.select(mask)
        assert sel.num_correspondences == int(mask.sum())
        qs, ts = sel.nec_eigensolver(q)
        for p in range(B):
            sl = slice(offsets[p], offsets[p + 1])
            m = mask[sl].astype(bool)
            Ro, to = oracle.nec_eigensolver(f1[sl][m], f2[sl][m], _quat_to_R(q[p]))
            assert _rot_err(oracle, _quat_to_R(qs[p]), Ro) <= 1e-7   # same stopping-tolerance slack
        # the reference's whole default pipeline on the inliers: weighted ES + SCF, then refinement
        qw, tw = sel.weighted_eigensolver(q, t, 1e-13, 10)
        res = sel.solve(qw, tw)
        for p in (0, 1, 2):
            assert _rot_err(oracle, _quat_to_R(res.q[p]), g.R_gt[p].numpy()) < 0.01
        sel.close()


@pytest.mark.parametrize("outliers", [0.15, 0.45])
def test_ransac_scoring_tile_boundaries_and_early_drop_vs_oracle(oracle, outliers):
    """RANSAC scores its models one after the other over tiles of 64 correspondences -- eight tiles in registers, the
    rest of a larger pair streamed -- and drops a model once it cannot beat the best so far (pnec_frontend.hip
    model_inliers_until_beaten).  Exactness of that drop and every tile boundary, against the oracle's full counts:
    identical masks, counts and iteration numbers for sizes around 64 k, 512 (registers | stream) and beyond;
    45 % outliers make the rule run for several rounds of sixteen hypotheses (pnec.cc:239-272)."""
    sizes = [64, 65, 100, 127, 128, 129, 300, 448, 449, 511, 512, 513, 575, 576, 577, 700, 1100]
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    rng = np.random.default_rng(17)
    f1s, f2s, cvs, Rs, qs = [], [], [], [], []
    for p, n in enumerate(sizes):
        g = sim.generate(1, n, seed=400 + p)
        f2 = g.bvs2[0].numpy().copy()
        bad = rng.choice(n, int(outliers * n), replace=False)
        v = rng.normal(size=(len(bad), 3))
        f2[bad] = v / np.linalg.norm(v, axis=1, keepdims=True)
        f1s.append(g.bvs1[0].numpy()); f2s.append(f2); cvs.append(g.covs2[0].numpy())
        Rs.append(g.init_R[0].numpy()); qs.append(g.init_q[0].numpy())
    f1, f2, c2 = np.concatenate(f1s), np.concatenate(f2s), np.concatenate(cvs)
    with Batch(capi.MODE_TARGET, offsets) as b:
        b.fill(f1, f2, c2)
        q, t, mask, cnt, its = b.ransac_eigensolver(np.stack(qs), seed=5)
    rounds = 0
    for p, n in enumerate(sizes):
        sl = slice(offsets[p], offsets[p + 1])
        Ro, to, mo, ito = oracle.ransac_eigensolver(f1[sl], f2[sl], Rs[p], seed=5, pair_id=p)
        assert its[p] == ito, (n, its[p], ito)
        np.testing.assert_array_equal(mask[sl].astype(bool), mo, err_msg=str(n))
        assert cnt[p] == mo.sum(), n
        rounds += (ito + 15) // 16
    if outliers > 0.4:
        assert rounds > 3 * len(sizes)   # the sequential rule ran across rounds, not just inside the first


TWO_PAIR_HARD = r'''
import os, sys
sys.path.insert(0, os.environ["PNEC_ROOT"])
import numpy as np
from oracle import pnec_oracle as oracle
from pnec_amd import Batch, capi
from pnec_amd import simulation as sim
sizes = [64, 100, 129, 300, 448, 511, 512, 513, 576, 700, 1100, 37, 5, 256, 384] * 3   # 45 pairs (odd: a wavefront with one)
offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
rng = np.random.default_rng(23)
f1s, f2s, cvs, Rs, qs = [], [], [], [], []
for p, n in enumerate(sizes):
    g = sim.generate(1, n, seed=700 + p)
    f2 = g.bvs2[0].numpy().copy()
    bad = rng.choice(n, int((0.25 + 0.25 * (p % 3 == 0)) * n), replace=False)     # 25 % / 50 % gross outliers
    v = rng.normal(size=(len(bad), 3))
    f2[bad] = v / np.linalg.norm(v, axis=1, keepdims=True)
    f1s.append(g.bvs1[0].numpy()); f2s.append(f2); cvs.append(g.covs2[0].numpy())
    Rs.append(g.init_R[0].numpy()); qs.append(g.init_q[0].numpy())
f1, f2, c2 = np.concatenate(f1s), np.concatenate(f2s), np.concatenate(cvs)
with Batch(capi.MODE_TARGET, offsets) as b:
    b.fill(f1, f2, c2)
    q, t, mask, cnt, its = b.ransac_eigensolver(np.stack(qs), seed=9)
long_pairs = 0
for p, n in enumerate(sizes):
    sl = slice(offsets[p], offsets[p + 1])
    Ro, to, mo, ito = oracle.ransac_eigensolver(f1[sl], f2[sl], Rs[p], seed=9, pair_id=p)
    assert its[p] == ito, (p, n, its[p], ito)
    assert (mask[sl].astype(bool) == mo).all(), (p, n)
    assert cnt[p] == mo.sum(), (p, n)
    long_pairs += ito > 48
assert long_pairs >= 10, long_pairs     # pairs that ran for rounds with the wavefront to themselves
print("TWO_PAIR_HARD_OK", long_pairs)
'''


def test_two_pair_ransac_with_a_lent_slot_on_hard_pairs_vs_oracle():
    """The two-pair RANSAC kernel (normally from 4 096 pairs up; forced here) on 45 ragged pairs with 25 % and 50 % gross
    outliers: the pairs that need many rounds outlive their partners and run their rounds over BOTH slot groups (the
    finished partner parked in LDS, pnec_frontend.hip).  Masks, counts and iteration numbers equal the oracle's."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PNEC_ROOT=root, PNEC_RANSAC_FORM="2")
    r = subprocess.run([sys.executable, "-c", TWO_PAIR_HARD], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "TWO_PAIR_HARD_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def test_device_buffer_cache_reuses_and_releases():
    """batches created and destroyed in a loop reuse cached device buffers; release_cache returns them"""
    L = capi.lib()
    L.pnec_hip_release_cache(-1)
    offsets = np.arange(4001, dtype=np.int64) * 64          # 4000 pairs x 64 corr: a ~25 MB payload
    g = sim.generate(4, 64, seed=3)
    for _ in range(3):
        with Batch(capi.MODE_TARGET, offsets) as b:
            b.fill(np.tile(g.bvs1.reshape(-1, 3).numpy(), (1000, 1)), np.tile(g.bvs2.reshape(-1, 3).numpy(), (1000, 1)),
                   np.tile(g.covs2.reshape(-1, 3, 3).numpy(), (1000, 1, 1)))
            res = b.solve(np.tile(g.init_q.numpy(), (1000, 1)), np.tile(g.init_t.numpy(), (1000, 1)))
            assert np.isfinite(res.q).all()
    released = L.pnec_hip_release_cache(-1)
    assert released >= 20 * 1024 * 1024          # the payload buffer was being kept
    assert L.pnec_hip_release_cache(-1) == 0


# how often the "one stopping decision inside rounding per batch" allowance below is actually used: filled by the
# trials, written out by test_randomised_batches_allowance_bookkeeping (gpurun_out/iteration_allowance.json; the
# committed copy of a run is profiles/r03_iteration_allowance.json)
_ALLOWANCE = {"trials": 0, "solves": 0, "fired": []}


@pytest.mark.parametrize("trial", range(8))
def test_randomised_batches_against_oracle(oracle, trial):
    """random residual family, batch size, ragged counts up to a random maximum (all launch geometries incl.
    the streaming one), random iteration cap or Ceres-default termination: rotations, iteration counts"""
    rng = np.random.default_rng(900 + trial)
    mode = [capi.MODE_NEC, capi.MODE_TARGET, capi.MODE_HOST, capi.MODE_SYM][trial % 4]
    B = int(rng.integers(1, 120))
    nmax = int(rng.choice([17, 64, 100, 256, 400, 512, 600, 1024, 2048, 3000, 4096, 5000]))
    counts = rng.integers(6, nmax + 1, size=B).astype(np.int64)
    counts[rng.integers(0, B)] = nmax
    offsets = np.concatenate([[0], np.cumsum(counts)])
    g = sim.generate(B, nmax, seed=2000 + trial)
    f1 = np.concatenate([g.bvs1[p].numpy()[:n] for p, n in enumerate(counts)])
    f2 = np.concatenate([g.bvs2[p].numpy()[:n] for p, n in enumerate(counts)])
    S2 = np.concatenate([g.covs2[p].numpy()[:n] for p, n in enumerate(counts)])
    c2, c1 = _covs_for(mode, S2)
    kw = dict(check_convergence=int(rng.integers(0, 2)))
    if not kw["check_convergence"]:
        kw["max_num_iterations"] = int(rng.integers(1, 12))
    opts = capi.default_options(**kw)
    reg = 1e-13
    with Batch(mode, offsets) as b:
        b.fill(f1, f2, c2, c1)
        res = b.solve(g.init_q.numpy(), g.init_t.numpy(), reg=reg, options=opts)
    q, t, cost, it, st = _oracle_batch(oracle, mode, offsets, f1, f2, c2, c1, reg, g.init_q.numpy(),
                                       g.init_t.numpy(), _oracle_opts(oracle, opts, oracle.JAC_ANALYTIC))
    worst = max(_rot_err(oracle, _quat_to_R(res.q[p]), _quat_to_R(q[p])) for p in range(B))
    assert worst <= 10 * ROT_TOL_SAME_ALGO, worst   # pairs of 6..20 correspondences are weakly constrained
    # iteration counts and termination codes are EQUAL; the only admissible difference is a stopping or
    # acceptance test decided inside rounding of its threshold, which shows as both runs ending in the
    # same tolerance ball -- every such pair is checked, and there may be at most one per batch
    diff = np.flatnonzero((res.iterations != it) | (res.status != st))
    _ALLOWANCE["trials"] += 1
    _ALLOWANCE["solves"] += int(B)
    for p in diff:
        _ALLOWANCE["fired"].append({"trial": int(trial), "mode": int(mode), "pair": int(p), "corr": int(counts[p]),
                                    "iterations_device_oracle": [int(res.iterations[p]), int(it[p])],
                                    "status_device_oracle": [int(res.status[p]), int(st[p])]})
    assert len(diff) <= 1, (diff, res.iterations[diff], it[diff])
    for p in diff:
        assert abs(int(res.iterations[p]) - int(it[p])) == 1, (p, res.iterations[p], it[p])
        assert abs(res.cost[p] - cost[p]) <= 2e-6 * abs(cost[p]), (p, res.cost[p], cost[p])


def test_randomised_batches_allowance_bookkeeping():
    """Record of how often test_randomised_batches_against_oracle's allowance (at most one solve per batch whose
    iteration count or termination code differs by a stopping test decided inside rounding) was used in this run."""
    import json
    if _ALLOWANCE["trials"] == 0:
        pytest.skip("the randomised trials did not run in this session")
    rec = dict(_ALLOWANCE, fired_count=len(_ALLOWANCE["fired"]))
    print("iteration allowance:", json.dumps(rec))
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out")
    try:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "iteration_allowance.json"), "w") as f:
            json.dump(rec, f)
    except OSError:
        pass
    assert len(_ALLOWANCE["fired"]) <= _ALLOWANCE["trials"]


@pytest.mark.parametrize("mode", [capi.MODE_TARGET, capi.MODE_HOST, capi.MODE_NEC])
def test_tail_geometry_is_bitwise_the_two_wavefront_geometry(oracle, mode):
    """Pairs of 513..768 correspondences run on ONE wavefront -- geometry (12, 1, 3): 512 correspondences resident on
    chip, the tail re-read from L2 in every pass -- instead of (8, 2, 3)'s two wavefronts and two barriers per pass.
    The tail's sums are accumulated, reduced and added exactly the way the second wavefront's are, so every output
    (pose, cost, iteration count, termination code) must equal the forced (8, 2, 3) solve BIT FOR BIT -- which is also
    what the streaming handle's AoS kernels (not built for the tail form) produce for such pairs.  Sizes on every
    boundary of the tail's slot pairs; Ceres-default termination and a fixed iteration count; sampled oracle parity."""
    sizes = [513, 514, 575, 576, 577, 639, 640, 641, 642, 700, 703, 704, 705, 767, 768, 520, 600, 650, 750, 768]
    B = len(sizes)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    g = sim.generate(B, 768, seed=4242)
    f1 = np.concatenate([g.bvs1[p].numpy()[:n] for p, n in enumerate(sizes)])
    f2 = np.concatenate([g.bvs2[p].numpy()[:n] for p, n in enumerate(sizes)])
    S2 = np.concatenate([g.covs2[p].numpy()[:n] for p, n in enumerate(sizes)])
    c2, c1 = _covs_for(mode, S2)
    reg = 0.0 if mode == capi.MODE_NEC else 1e-13
    for kw in (dict(), dict(max_num_iterations=7, check_convergence=0)):
        with Batch(mode, offsets) as b:
            b.fill(f1, f2, c2, c1)
            auto = capi.default_options(**kw)
            assert b.describe_launch(auto)["corr_per_lane"] == 12 and b.describe_launch(auto)["waves_per_pair"] == 1
            res = b.solve(g.init_q.numpy(), g.init_t.numpy(), reg=reg, options=auto)
            two = b.solve(g.init_q.numpy(), g.init_t.numpy(), reg=reg,
                          options=capi.default_options(corr_per_lane=8, waves_per_pair=2, lds_corr_per_lane=3, **kw))
        for name in ("q", "t", "cost", "iterations", "status"):
            assert np.array_equal(getattr(res, name), getattr(two, name)), (name, kw)
        q, t, cost, it, st = _oracle_batch(oracle, mode, offsets, f1, f2, c2, c1, reg, g.init_q.numpy(),
                                           g.init_t.numpy(), _oracle_opts(oracle, auto, oracle.JAC_NUMERIC_CENTRAL))
        worst = max(_rot_err(oracle, _quat_to_R(res.q[p]), _quat_to_R(q[p])) for p in range(B))
        assert worst <= ROT_TOL_REFERENCE, worst
        np.testing.assert_array_equal(res.iterations, it)


def test_cost_only_pass_after_a_rejected_step_counts_and_changes_no_bit(oracle):
    """Round 4: a candidate that follows a rejected step (or whose model promises less than the cost can resolve) is
    evaluated cost-only first -- Ceres' own order: residuals, then the Jacobian once the step is accepted -- and in full
    only if its step turns out accepted.  Results must be those of the reference-faithful oracle (iteration counts and
    codes equal: every decision is the same), and the pass counters (PNEC_HIP_OPT_COUNT_PASSES ->
    pnec_hip_work_counters[13], [14]) must show that fewer than iterations + 1 full passes per solve ran in the
    fixed-iteration mode, where the solves sit at their noise floor for most of their ten iterations."""
    import ctypes as C
    P, N = 2000, 512
    g = sim.generate(P, N, seed=1, device="cuda:0")
    L = capi.lib()
    cnt = np.zeros(16, dtype=np.uint64)
    flag = C.c_int32(0)
    with Batch.uniform(capi.MODE_TARGET, P, N) as b:
        b.fill(g.bvs1.reshape(-1, 3), g.bvs2.reshape(-1, 3), g.covs2.reshape(-1, 3, 3))
        for conv, mi in ((0, 10), (1, 50)):
            opts = capi.default_options(max_num_iterations=mi, check_convergence=conv)
            plain = b.solve(g.init_q, g.init_t, options=opts)
            capi.check(L.pnec_hip_work_counters(0, 1, cnt.ctypes.data, C.byref(flag)))
            counted_opts = capi.default_options(max_num_iterations=mi, check_convergence=conv, flags=1)
            counted = b.solve(g.init_q, g.init_t, options=counted_opts)
            torch.cuda.synchronize()
            capi.check(L.pnec_hip_work_counters(0, 1, cnt.ctypes.data, C.byref(flag)))
            assert torch.equal(plain.q, counted.q) and torch.equal(plain.iterations, counted.iterations)
            full, cost = int(cnt[13]), int(cnt[14])
            its = plain.iterations.cpu().numpy().astype(np.int64)
            assert full % N == 0 and cost % N == 0
            # every solve: iteration zero + one pass per iteration at least; a cost-first candidate that is accepted runs twice
            assert full + cost >= N * int((its + 1).sum()) and full + cost <= N * int((2 * its + 1).sum())
            if conv == 0:
                assert full < 0.8 * N * int((its + 1).sum()), (full, cost)        # the speculation is switched off where it loses
                assert cost > 0.25 * N * int(its.sum())
            else:
                assert cost <= 0.05 * (full + cost)                                # Ceres-default termination: next to nothing rejected
            # parity with the oracle, decisions included
            oo = _oracle_opts(oracle, opts, oracle.JAC_ANALYTIC if hasattr(oracle, "JAC_ANALYTIC") else oracle.JAC_NUMERIC_CENTRAL)
            rq, rit, rst = plain.q.cpu().numpy(), its, plain.status.cpu().numpy()
            for p in range(0, P, 97):
                s = oracle.solve(oracle.MODE_TARGET, g.bvs1[p].cpu().numpy(), g.bvs2[p].cpu().numpy(), g.covs2[p].cpu().numpy(), None,
                                 1e-13, g.init_q[p].cpu().numpy(), g.init_t[p].cpu().numpy(), oo)
                assert rit[p] == s.iterations and rst[p] == s.status, p
                assert _rot_err(oracle, _quat_to_R(rq[p]), s.R) <= 1e-8, p


@pytest.mark.parametrize("mode,n_corr,H", [(capi.MODE_TARGET, 4096, 19), (capi.MODE_TARGET, 3000, 8), (capi.MODE_TARGET, 1500, 5),
                                           (capi.MODE_TARGET, 900, 7), (capi.MODE_NEC, 2100, 6), (capi.MODE_HOST, 1100, 3),
                                           (capi.MODE_SYM, 700, 9), (capi.MODE_SYM, 2048, 10),
                                           # one wavefront per pair: two hypotheses of the pair per wavefront (lm_solve_pairhyp_kernel)
                                           (capi.MODE_TARGET, 512, 7), (capi.MODE_TARGET, 100, 4), (capi.MODE_TARGET, 40, 3),
                                           (capi.MODE_NEC, 512, 5), (capi.MODE_HOST, 300, 2), (capi.MODE_SYM, 450, 3)])
def test_multi_hypothesis_group_form_is_bitwise_the_one_solve_per_block_form(mode, n_corr, H):
    """n_hyp > 1 on a several-wavefront geometry runs lm_solve_group_kernel: one block per (pair, group of WPP hypotheses),
    the payload loaded once, the group's LM steps at the same time (one per wavefront); on a one-wavefront geometry
    lm_solve_pairhyp_kernel: two hypotheses of the pair per wavefront, both steps at once in two quads.  Same arithmetic in the
    same order per solve, so every (pair, hypothesis) must come out BIT FOR BIT as the same solve made alone (n_hyp = 1: the
    one-solve-per-block kernel) -- poses, costs, iteration counts, termination codes; with H not a multiple of the group
    size (short last group), in the throughput configuration and with Ceres' convergence tests (hypotheses of one group
    end at different iterations), and from starts 180 degrees off."""
    P = 5
    g = sim.generate(P, n_corr, seed=4000 + n_corr, device="cuda:0")
    c2, c1 = (None, None) if mode == capi.MODE_NEC else (g.covs2.reshape(-1, 3, 3), None)
    if mode == capi.MODE_SYM:
        c1 = (g.covs2.roll(1, dims=1) * 0.8).reshape(-1, 3, 3).contiguous()
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(11)
    hyp = torch.randn(P * H, 3, generator=gen, dtype=torch.float64, device="cuda:0")
    hyp = hyp / hyp.norm(dim=1, keepdim=True)
    hyp[::H] = g.init_t
    with Batch.uniform(mode, P, n_corr) as b:
        b.fill(g.bvs1.reshape(-1, 3), g.bvs2.reshape(-1, 3), c2, c1)
        for kw in (dict(max_num_iterations=10, check_convergence=0), dict(), dict(max_num_iterations=0)):
            opts = capi.default_options(**kw)
            launch = b.describe_launch(opts)
            assert (launch["waves_per_pair"] >= 2) == (n_corr > 768 or (mode == capi.MODE_SYM and n_corr > 512)), launch
            res = b.solve(g.init_q, None, options=opts, hyp_t=hyp, n_hyp=H)
            torch.cuda.synchronize()
            for h in range(H):
                one = b.solve(g.init_q, None, options=opts, hyp_t=hyp[h::H].contiguous(), n_hyp=1)
                for name in ("q", "t", "cost", "iterations", "status"):
                    got, want = getattr(res, name)[h::H], getattr(one, name)
                    assert torch.equal(got, want), (kw, h, name, got, want)
            if kw == dict():
                assert len(set(res.iterations.cpu().numpy().tolist())) > 1     # the groups did hold solves of different lengths


def test_multi_hypothesis_on_a_ragged_batch_runs_every_form_side_by_side():
    """A ragged batch is solved as one launch per geometry in use (side streams, a table of the pairs each launch covers).
    With several starts per pair that means, in ONE call: two hypotheses per wavefront on the small pairs
    (lm_solve_pairhyp_kernel), the one-solve-per-block kernel on the pairs of 513..768 (the tail form (12, 1, 3) has no
    multi-hypothesis twin), and a block per pair and group of 2 / 4 / 8 hypotheses on the larger ones
    (lm_solve_group_kernel) -- every (pair, hypothesis) bit for bit the same solve made alone."""
    sizes = np.array([40, 64, 100, 300, 512, 513, 700, 768, 769, 1024, 1500, 2048, 2100, 4096, 17, 511, 3000, 640], dtype=np.int64)
    P, H = len(sizes), 5
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    g = sim.generate(P, int(sizes.max()), seed=777, device="cuda:0")
    keep = torch.arange(int(sizes.max()), device="cuda:0")[None, :] < torch.as_tensor(sizes, device="cuda:0")[:, None]
    f1, f2, cv = g.bvs1[keep], g.bvs2[keep], g.covs2[keep]
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(3)
    hyp = torch.randn(P * H, 3, generator=gen, dtype=torch.float64, device="cuda:0")
    hyp = hyp / hyp.norm(dim=1, keepdim=True)
    hyp[::H] = g.init_t
    with Batch(capi.MODE_TARGET, off) as b:
        b.fill(f1, f2, cv)
        for kw in (dict(max_num_iterations=10, check_convergence=0), dict()):
            opts = capi.default_options(**kw)
            res = b.solve(g.init_q, None, options=opts, hyp_t=hyp, n_hyp=H)
            torch.cuda.synchronize()
            for h in range(H):
                one = b.solve(g.init_q, None, options=opts, hyp_t=hyp[h::H].contiguous(), n_hyp=1)
                for name in ("q", "t", "cost", "iterations", "status"):
                    assert torch.equal(getattr(res, name)[h::H], getattr(one, name)), (kw, h, name)
            assert torch.isfinite(res.q).all()
