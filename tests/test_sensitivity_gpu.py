"""Pose sensitivity (pnec_hip_pose_sensitivity, Batch.pose_sensitivity, pnec_amd.differentiable_solve) on the device.

The yardstick is the float64 torch-CPU reference of test_sensitivity_cpu.py (written from the formulas of
include/pnec_hip.h, pinned to the oracle there) at the same (q, t) that is handed to the device -- never a device result.
Each test asserts its precondition (the reference's Hessian positive definite, or indefinite) before looking at the device.

Bounds (test_sensitivity_cpu.check_slot): H and g 1e-10 normalised by the reference's J'J; lambda and x_N 2 kappa 1e-10 and
the per-correspondence arrays (2 kappa + 1) 1e-10 of the array's largest entry in the slot.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from pnec_amd import Batch, capi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_sensitivity_cpu import (FAMILIES, FAMILY_IDS, GAUSS_NEWTON, GRAD_POSE, HOST, NEC, NONFINITE, OK, REG, ROOT, SINGULAR,  # noqa: E402
                                  SYM, TARGET, TOL, W_Q, W_T, Pair, Reference, check_slot, fd_case, fd_gaps, grad_pose_of,
                                  make_pair, oracle_pose, perpendicular)

pytestmark = pytest.mark.gpu

SLOT = ("lam", "hessian", "grad", "newton", "status")
PER = ("grad_bvs1", "grad_bvs2", "grad_covs", "grad_covs_host")


def _batch(pairs):
    mode = pairs[0].mode
    off = np.concatenate([[0], np.cumsum([p.n for p in pairs])]).astype(np.int64)
    b = Batch(mode, off)
    cat = lambda xs: None if xs[0] is None else np.concatenate(xs)
    if off[-1] > 0:
        b.fill(cat([p.f1 for p in pairs]), cat([p.f2 for p in pairs]), cat([p.c2 for p in pairs]), cat([p.c1 for p in pairs]))
    return b


def _device(pairs, q, t, gp=None, **kw):
    S = len(np.asarray(q, float).reshape(-1, 4))
    gp = np.tile(GRAD_POSE, (S, 1)) if gp is None else np.asarray(gp, float).reshape(-1, 6)
    with _batch(pairs) as b:
        return b.pose_sensitivity(np.asarray(q, float).reshape(-1, 4), np.asarray(t, float).reshape(-1, 3), gp, reg=REG, **kw)


def _np(x):
    return None if x is None else (x.cpu().numpy() if torch.is_tensor(x) else x)


def _slot(dev, s, pairs):
    """slot s of a call with n_hyp == 1, in the shape check_slot reads"""
    a = sum(p.n for p in pairs[:s])
    rows = lambda x: np.zeros((pairs[s].n, 3, 3)) if x is None else _np(x)[a:a + pairs[s].n]
    return dict(status=int(_np(dev.status)[s]), H=_np(dev.hessian)[s], g=_np(dev.grad)[s], lam=_np(dev.lam)[s],
                newton=_np(dev.newton)[s], grads=[rows(dev.grad_bvs1), rows(dev.grad_bvs2), rows(dev.grad_covs), rows(dev.grad_covs_host)])


def _same(a, b, names=SLOT + PER, rows=None, what=""):
    for name in names:
        x, y = _np(getattr(a, name)), _np(getattr(b, name))
        if x is None and y is None:
            continue
        if rows is not None and name in PER:
            x, y = x[rows[0]], y[rows[1]]
        assert np.array_equal(x, y, equal_nan=True), (what, name)


# ---- 1, 2, 5: values on a count ladder, bits, the Gauss-Newton flag ------------------------------------------------------
# partial wavefront (8, 37), a full one, one row into a second trip, the one-wavefront share, one row into a second
# wavefront, three wavefronts odd, past eight wavefronts' single trip
COUNTS = [8, 37, 64, 65, 512, 513, 1100, 4097]
AT_MINIMISER = [True, False, True, False, False, True, False, True]
_ladders = {}


def _ladder(oracle, mode):
    if mode not in _ladders:
        pairs, qs, ts = [], [], []
        for i, (n, at_min) in enumerate(zip(COUNTS, AT_MINIMISER)):
            pr, q, t = make_pair(mode, n, seed=300 + i)
            if at_min:
                q, t, _ = oracle_pose(oracle, pr, q, t)
            pairs.append(pr), qs.append(q), ts.append(t)
        _ladders[mode] = (pairs, np.array(qs), np.array(ts))
    return _ladders[mode]


@pytest.mark.parametrize("mode", FAMILIES, ids=FAMILY_IDS)
def test_every_output_matches_the_reference_on_a_count_ladder(oracle, mode):
    pairs, qs, ts = _ladder(oracle, mode)
    refs = [Reference(pr, q, t, GRAD_POSE) for pr, q, t in zip(pairs, qs, ts)]
    for pr, ref in zip(pairs, refs):
        assert ref.ok, f"precondition: the reference's H is positive definite at n={pr.n} (least eigenvalue {ref.min_eig:.3e})"
    dev = _device(pairs, qs, ts)          # one ragged batch: block sized for the largest pair
    report = []
    for s, (pr, ref) in enumerate(zip(pairs, refs)):
        check_slot(ref, _slot(dev, s, pairs), f"{FAMILY_IDS[mode]} n={pr.n} {'minimiser' if AT_MINIMISER[s] else 'ground truth'}", report)
        H = dev.hessian[s]
        assert np.array_equal(H, H.T)
        for G in (dev.grad_covs, dev.grad_covs_host):
            if G is not None:
                assert np.array_equal(G, np.transpose(G, (0, 2, 1)))
    print("largest errors:", " ".join(f"{max(r[k] for r in report):.2e}" for k in range(1, 6)))
    # the same pairs alone in a batch (block sized for that pair): the same bits
    for s in (0, 3):
        alone = _device([pairs[s]], qs[s], ts[s])
        a = sum(p.n for p in pairs[:s])
        for name in SLOT:
            assert np.array_equal(getattr(alone, name)[0], getattr(dev, name)[s]), (s, name)
        _same(alone, dev, PER, (slice(None), slice(a, a + pairs[s].n)), f"pair {s} alone")


@pytest.mark.parametrize("mode", FAMILIES, ids=FAMILY_IDS)
def test_gauss_newton_flag_is_the_references_jtj_variant(oracle, mode):
    pairs, qs, ts = _ladder(oracle, mode)
    pick = [1, 5, 6]     # 37 (ground truth), 513 (minimiser), 1100 (ground truth)
    sub = [pairs[i] for i in pick]
    refs = [Reference(pairs[i], qs[i], ts[i], GRAD_POSE, gauss_newton=True) for i in pick]
    assert all(r.ok for r in refs)
    dev = _device(sub, qs[pick], ts[pick], gauss_newton=True)
    for s, ref in enumerate(refs):
        check_slot(ref, _slot(dev, s, sub), f"{FAMILY_IDS[mode]} n={sub[s].n} J'J")
    # and it is another matrix than the full one
    full = _device(sub, qs[pick], ts[pick])
    assert not np.array_equal(full.hessian, dev.hessian)


# ---- 3: hypotheses, spaces, views ------------------------------------------------------------------------------------------
def _sim(mode, B, n, seed):
    out = [make_pair(mode, n, seed=seed + i) for i in range(B)]
    return [o[0] for o in out], np.array([o[1] for o in out]), np.array([o[2] for o in out])


def test_hypotheses_device_space_and_views_are_bit_identical():
    pairs, q0, t0 = _sim(SYM, 4, 300, seed=80)
    rng = np.random.default_rng(1)
    q3 = np.repeat(q0, 3, axis=0) + rng.normal(size=(12, 4)) * 1e-5
    t3 = np.repeat(t0, 3, axis=0) + rng.normal(size=(12, 3)) * 1e-5
    gp3 = rng.normal(size=(12, 6))
    with _batch(pairs) as b:
        three = b.pose_sensitivity(q3, t3, gp3, n_hyp=3)
        assert np.all(three.status == OK)
        for h in range(3):
            one = b.pose_sensitivity(q3[h::3], t3[h::3], gp3[h::3])
            for name in SLOT:
                assert np.array_equal(getattr(three, name)[h::3], getattr(one, name)), (h, name)
            for p in range(4):      # row n_hyp * offsets[p] + h * N_p + i
                _same(three, one, PER, (slice(3 * 300 * p + 300 * h, 3 * 300 * p + 300 * (h + 1)), slice(300 * p, 300 * (p + 1))), (h, p))
        # device space == host space
        cu = lambda a: torch.as_tensor(a, device="cuda:0")
        d = b.pose_sensitivity(cu(q3), cu(t3), cu(gp3), n_hyp=3)
        assert d.grad_covs.is_cuda and d.hessian.shape == (12, 5, 5) and d.grad_covs_host.shape == (3600, 3, 3)
        _same(d, three, what="device space")
        # a select(view=True) batch == the same correspondences in a fresh batch
        mask = (rng.uniform(size=4 * 300) < 0.7).astype(np.uint8)
        v = b.select(mask, view=True)
        view = v.pose_sensitivity(q0, t0, gp3[:4])
    kept = []
    for p, m in zip(pairs, mask.reshape(4, 300).astype(bool)):
        k = Pair(SYM, p.f1[m], p.f2[m], p.c2[m])
        k.c1 = p.c1[m]
        kept.append(k)
    _same(view, _device(kept, q0, t0, gp3[:4]), what="view")


def test_reshaped_capacity_batch():
    pairs, q0, t0 = _sim(TARGET, 2, 150, seed=90)
    want = _device(pairs, q0, t0)
    with Batch.with_capacity(TARGET, 8, 4000) as b:
        b.reshape([0, 700, 1400]).fill(np.zeros((1400, 3)), np.zeros((1400, 3)), np.zeros((1400, 3, 3)))
        b.reshape([0, 150, 300])
        b.fill(np.concatenate([p.f1 for p in pairs]), np.concatenate([p.f2 for p in pairs]), np.concatenate([p.c2 for p in pairs]))
        got = b.pose_sensitivity(q0, t0, np.tile(GRAD_POSE, (2, 1)))
    _same(got, want, what="capacity batch")


# ---- 4: statuses -----------------------------------------------------------------------------------------------------------
def test_too_few_correspondences_and_an_empty_pair_in_the_middle():
    full, q, t = make_pair(TARGET, 40, seed=3)
    pairs = [full.head(k) for k in (0, 1, 4)] + [full, full.head(0), full]
    dev = _device(pairs, np.tile(q, (6, 1)), np.tile(t, (6, 1)))
    assert list(dev.status) == [SINGULAR] * 3 + [OK, SINGULAR, OK]
    assert np.all(np.isnan(dev.lam[:3])) and np.all(np.isnan(dev.newton[[0, 1, 2, 4]])) and np.all(np.isnan(dev.grad_bvs1[:5]))
    assert np.all(dev.hessian[0] == 0.0) and np.all(dev.grad[4] == 0.0)
    for name in SLOT:
        assert np.array_equal(getattr(dev, name)[3], getattr(dev, name)[5]), name
    assert np.array_equal(dev.grad_covs[5:45], dev.grad_covs[45:]) and np.all(np.isfinite(dev.grad_covs[5:]))


def test_nan_input_is_reported_for_its_pair_only():
    pairs, q0, t0 = _sim(TARGET, 5, 200, seed=100)
    clean = _device(pairs, q0, t0)
    assert np.all(clean.status == OK)
    bad = Pair(TARGET, pairs[2].f1.copy(), pairs[2].f2.copy(), pairs[2].c2)
    bad.f2[17, 1] = np.nan
    for kw, filled in ((dict(), np.isnan), (dict(zero_on_failure=True), lambda a: a == 0.0)):
        dev = _device(pairs[:2] + [bad] + pairs[3:], q0, t0, **kw)
        assert list(dev.status) == [0, 0, NONFINITE, 0, 0]
        assert np.all(filled(dev.lam[2])) and np.all(filled(dev.grad_bvs2[400:600])) and np.all(filled(dev.grad_covs[400:600]))
        keep = np.r_[0:400, 600:1000]
        for name in SLOT:
            assert np.array_equal(getattr(dev, name)[[0, 1, 3, 4]], getattr(clean, name)[[0, 1, 3, 4]]), name
        for name in PER[:3]:
            assert np.array_equal(getattr(dev, name)[keep], getattr(clean, name)[keep]), name


def test_a_pose_that_is_no_minimiser_is_singular():
    pairs, q0, t0 = _sim(TARGET, 3, 130, seed=110)
    t = t0.copy()
    t[1] = perpendicular(t0[1])
    ref = Reference(pairs[1], q0[1], t[1], GRAD_POSE)
    assert not ref.positive and ref.min_eig < 0.0, ref.min_eig     # the precondition: indefinite on the reference
    good = _device(pairs, q0, t0)
    nan = _device(pairs, q0, t)
    zero = _device(pairs, q0, t, zero_on_failure=True)
    for dev, filled in ((nan, np.isnan), (zero, lambda a: a == 0.0)):
        assert list(dev.status) == [OK, SINGULAR, OK]
        for a in (dev.lam[1], dev.newton[1], dev.grad_bvs1[130:260], dev.grad_bvs2[130:260], dev.grad_covs[130:260]):
            assert np.all(filled(a))
        sc = np.sqrt(np.outer(np.diag(ref.G), np.diag(ref.G)))
        assert (np.abs(dev.hessian[1] - ref.H) / sc).max() <= TOL     # H and g are written as computed
        for name in SLOT:
            assert np.array_equal(getattr(dev, name)[[0, 2]], getattr(good, name)[[0, 2]]), name


# ---- 6: end to end, against finite differences of the oracle's solve -----------------------------------------------------------
def test_device_gradient_against_finite_differences_of_the_solve(oracle):
    pr, q, t, gp, fds = fd_case(oracle)
    ref = Reference(pr, q, t, gp)
    assert ref.ok
    g_fd = max(fd_gaps(fds, ref.grads[1], ref.grads[2]))     # the differencing error, measured on the CPU
    assert g_fd <= 1e-3, g_fd
    dev = _device([pr], q, t, gp)
    assert dev.status[0] == OK
    gap = max(fd_gaps(fds, dev.grad_bvs2, dev.grad_covs))
    print(f"analytic-vs-FD gap g_fd = {g_fd:.3e}, device-vs-FD {gap:.3e}")
    assert gap <= 10 * g_fd, f"device vs finite differences {gap:.3e}, allowed 10 g_fd, g_fd = {g_fd:.3e}"


# ---- 7, 8: autograd, streams ---------------------------------------------------------------------------------------------------
def _cuda_inputs(pairs, q0, t0):
    cu = lambda a: torch.tensor(a, dtype=torch.float64, device="cuda:0")
    cat = lambda xs: cu(np.concatenate(xs))
    off = np.concatenate([[0], np.cumsum([p.n for p in pairs])]).astype(np.int64)
    return off, cat([p.f1 for p in pairs]), cat([p.f2 for p in pairs]), cat([p.c2 for p in pairs]), cu(q0), cu(t0)


def test_differentiable_solve_backpropagates_through_the_minimiser():
    import pnec_amd
    pairs, q0, t0 = _sim(TARGET, 3, 200, seed=120)
    off, f1, f2, c0, iq, it = _cuda_inputs(pairs, q0, t0)
    wq, wt = torch.tensor(W_Q, device="cuda:0"), torch.tensor(W_T, device="cuda:0")
    s = torch.zeros(600, dtype=torch.float64, device="cuda:0", requires_grad=True)
    f1.requires_grad_(True), f2.requires_grad_(True), iq.requires_grad_(True), it.requires_grad_(True)
    covs = torch.exp(s)[:, None, None] * c0
    covs.retain_grad()
    q, t, info = pnec_amd.differentiable_solve(TARGET, off, f1, f2, covs, init_q=iq, init_t=it, reg=REG)
    assert q.requires_grad and t.requires_grad and not any(v.requires_grad for v in info.values())
    assert set(info) == {"cost", "iterations", "status", "sens_status", "newton"}
    ((wq * q).sum() + (wt * t).sum()).backward()
    assert iq.grad is None and it.grad is None
    assert np.all(info["sens_status"].cpu().numpy() == OK)

    # bitwise the batch call at the returned pose, with the cotangent made by the same operations
    qd, td = q.detach(), t.detach()
    gq, gt = wq.expand(3, 4), wt.expand(3, 3)
    g_omega = 0.5 * (qd[:, 3:] * gq[:, :3] + torch.linalg.cross(qd[:, :3], gq[:, :3]) - gq[:, 3:] * qd[:, :3])
    gp = torch.cat([g_omega, gt], dim=1).contiguous()
    with Batch(TARGET, off) as b:
        b.fill(f1.detach(), f2.detach(), c0)
        direct = b.pose_sensitivity(qd, td, gp, reg=REG, zero_on_failure=True)
        torch.cuda.synchronize()
    assert torch.equal(f1.grad, direct.grad_bvs1) and torch.equal(f2.grad, direct.grad_bvs2) and torch.equal(covs.grad, direct.grad_covs)
    assert torch.equal(info["newton"], direct.newton)
    # the quaternion formula is the one the CPU test differentiates with
    assert np.allclose(gp[0].cpu().numpy(), grad_pose_of(qd[0].cpu().numpy(), W_Q, W_T), rtol=1e-14, atol=0)

    # the reference, within the bounds, and its chain onto s
    qn, tn, gpn = qd.cpu().numpy(), td.cpu().numpy(), gp.cpu().numpy()
    want_s = []
    for p, pr in enumerate(pairs):
        ref = Reference(pr, qn[p], tn[p], gpn[p])
        assert ref.ok
        rows = slice(200 * p, 200 * (p + 1))
        dev = dict(status=OK, H=ref.H, g=ref.g, lam=ref.lam, newton=ref.newton,     # (the slot outputs are test 1's business)
                   grads=[f1.grad[rows].cpu().numpy(), f2.grad[rows].cpu().numpy(), covs.grad[rows].cpu().numpy(), np.zeros((200, 3, 3))])
        check_slot(ref, dev, f"autograd pair {p}")
        want_s.append((ref.grads[2] * pr.c2).sum((1, 2)))
    want_s = np.concatenate(want_s)
    err = np.abs(s.grad.cpu().numpy() - want_s).max() / np.abs(want_s).max()
    print(f"s.grad against the reference's chain: {err:.3e}")
    assert err <= 1e-8


def test_side_stream_equals_the_default_stream():
    pairs, q0, t0 = _sim(HOST, 3, 700, seed=130)
    off, f1, f2, c2, iq, it = _cuda_inputs(pairs, q0, t0)
    gp = torch.tensor(np.tile(GRAD_POSE, (3, 1)), device="cuda:0")

    def run():
        with Batch(HOST, off) as b:
            b.fill(f1, f2, c2)
            res = b.solve(iq, it, reg=REG)
            out = res.sensitivity(gp)
            torch.cuda.current_stream().synchronize()
            return res, out
    res0, want = run()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        res1, got = run()
    assert torch.equal(res0.q, res1.q)
    _same(got, want, what="side stream")
    assert np.all(_np(want.status) == OK)


# ---- 9: surface ------------------------------------------------------------------------------------------------------------------
def test_solve_result_sensitivity_is_the_batch_call_at_its_own_pose():
    pairs, q0, t0 = _sim(TARGET, 3, 256, seed=140)
    gp = np.tile(GRAD_POSE, (3, 1))
    with _batch(pairs) as b:
        res = b.solve(q0, t0, reg=1e-12)
        a, c = res.sensitivity(gp), b.pose_sensitivity(res.q, res.t, gp, reg=1e-12)
        a2, c2 = res.sensitivity(gp, gauss_newton=True), b.pose_sensitivity(res.q, res.t, gp, reg=1e-12, gauss_newton=True)
    _same(a, c), _same(a2, c2)
    assert np.all(a.status == OK) and not np.array_equal(a.lam, a2.lam)


def test_pybind_and_facade_equal_the_batch_call(oracle):
    import pnec_amd.pypnec as pypnec
    pr, _, t = make_pair(TARGET, 180, seed=150)
    # the facade takes a rotation MATRIX and makes its own quaternion of it.  Identity rotation: that quaternion is
    # (0, 0, 0, 1) whatever the conversion, so the facade runs the batch call's very inputs -> the same bits.  (No
    # minimiser: the call may say SINGULAR, and then both say it with the same NaNs.)
    qi = np.array([0.0, 0.0, 0.0, 1.0])
    T = np.eye(4)
    T[:3, 3] = t
    g1, g2, gc, lam, xn, status = pypnec.pose_sensitivity(pr.f1, pr.f2, pr.c2, T, GRAD_POSE, 1e-13)
    want = _device([pr], qi, t)
    assert status == want.status[0]
    for got, name in ((g1, "grad_bvs1"), (g2, "grad_bvs2"), (gc, "grad_covs"), (lam[None], "lam"), (xn[None], "newton")):
        assert np.array_equal(got, getattr(want, name), equal_nan=True), name
    # a general pose, at the oracle's minimiser: the quaternion is the conversion's, equal to rounding
    pr, q, t = make_pair(TARGET, 180, seed=151)
    q, t, _ = oracle_pose(oracle, pr, q, t)
    T[:3, :3] = oracle.rot_from_quat(q)
    T[:3, 3] = t
    g1, g2, gc, lam, xn, status = pypnec.pose_sensitivity(pr.f1, pr.f2, pr.c2, T, GRAD_POSE)
    want = _device([pr], q, t)
    assert status == OK == want.status[0]
    assert np.abs(gc - want.grad_covs).max() <= 1e-8 * np.abs(want.grad_covs).max()
    assert np.abs(g2 - want.grad_bvs2).max() <= 1e-8 * np.abs(want.grad_bvs2).max()
    # the demo walks the facade: it prints how far its solve stopped from the minimiser
    out = subprocess.run([os.path.join(ROOT, "pnec_amd", "pnec_host_demo")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    f = dict(kv.split("=") for kv in out.stdout.split())
    assert int(f["sens_status"]) == OK and 0.0 <= float(f["newton_step"]) < 1e-2, out.stdout
