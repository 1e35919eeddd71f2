"""Pose covariance (pnec_hip_pose_covariance) against the CPU oracle.

The yardstick is always the oracle's ANALYTIC evaluation (`evaluate(mode, JAC_ANALYTIC, ...)`, Ceres tangent space
(theta, phi, delta_xyz)) at the same (q, t) that is handed to the device -- never a device result.

Bounds:
* information / gradient / cost: 1e-10, entries of J'J normalised by sqrt(H_aa H_bb) -- the project's bar for
  device-vs-oracle sums (test_parity_gpu).
* covariance: 2 kappa 1e-10 per entry, kappa = condition number of the Jacobi-scaled information in the orthonormal
  chart the test builds itself: the first-order perturbation bound of an inverse whose argument is off by 1e-10,
  factor 2 for the higher-order terms.  Entries are compared in the frame (omega, b_theta, e_phi | t): the 5x5 part
  normalised by sqrt(Sigma_aa Sigma_bb), the row / column along t absolutely against 1e-10 max|Sigma_tt|.
"""
import math
import os
import subprocess

import numpy as np
import pytest

from pnec_amd import Batch, capi
from pnec_amd import simulation as sim
from pnec_amd.batch import chart_basis

pytestmark = pytest.mark.gpu

NEC, TARGET, HOST, SYM = capi.MODE_NEC, capi.MODE_TARGET, capi.MODE_HOST, capi.MODE_SYM
FAMILIES = [NEC, TARGET, HOST, SYM]
FAMILY_IDS = ["NEC", "TARGET", "HOST", "SYM"]
REG = 1e-13
TOL = 1e-10
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- helpers ------------------------------------------------------------------------------------------------------
def _covs_for(mode, S2):
    if mode == NEC:
        return None, None
    if mode == SYM:
        return S2, np.roll(S2, 1, axis=0) * 0.8
    return S2, None


def _angles(t):
    """(theta, phi) of a direction, accurate at the poles (atan2, not acos); phi = 0 on the axis"""
    rho = math.hypot(t[0], t[1])
    return math.atan2(rho, t[2]), (math.atan2(t[1], t[0]) if rho > 0 else 0.0)


def _vec(theta, phi):
    return np.array([math.sin(theta) * math.cos(phi), math.sin(theta) * math.sin(phi), math.cos(theta)])


def _basis(theta, phi):
    bth = np.array([math.cos(theta) * math.cos(phi), math.cos(theta) * math.sin(phi), -math.sin(theta)])
    return bth, np.array([-math.sin(phi), math.cos(phi), 0.0])


def _lift(Sx, bth, eph):
    L = np.zeros((6, 5))
    L[3:, 0], L[3:, 1] = bth, eph
    L[:3, 2:] = np.eye(3)
    return L @ Sx @ L.T


def _kappa(Hx):
    d = 1.0 / np.sqrt(np.diag(Hx))
    return np.linalg.cond(Hx * np.outer(d, d))


def _inv_spd(Hx):
    d = 1.0 / np.sqrt(np.diag(Hx))
    return np.linalg.inv(Hx * np.outer(d, d)) * np.outer(d, d)


class Pair:
    """one pair of a family, numpy arrays"""

    def __init__(self, mode, f1, f2, S2):
        self.mode, self.f1, self.f2 = mode, np.ascontiguousarray(f1), np.ascontiguousarray(f2)
        self.c2, self.c1 = _covs_for(mode, np.ascontiguousarray(S2))
        self.n = len(self.f1)

    def evaluate(self, oracle, q, theta, phi, reg=REG):
        return oracle.evaluate(self.mode, oracle.JAC_ANALYTIC, self.f1, self.f2, self.c2, self.c1, reg, theta, phi, q)

    def reference(self, oracle, q, t, reg=REG):
        """-> dict(H, grad, cost, Hx, kappa, cov) from the oracle's analytic J at (q, angles of t)"""
        theta, phi = _angles(t)
        r, J, cost = self.evaluate(oracle, q, theta, phi, reg)
        out = dict(H=J.T @ J, grad=J.T @ r, cost=cost, theta=theta, phi=phi)
        if abs(math.sin(theta)) > 1e-8 and self.n >= 5:
            Jx = J / np.array([1.0, math.sin(theta), 2.0, 2.0, 2.0])
            Hx = Jx.T @ Jx
            bth, eph = _basis(theta, phi)
            out.update(Hx=Hx, kappa=_kappa(Hx), cov=_lift(_inv_spd(Hx), bth, eph), bth=bth, eph=eph)
        return out


def _sim_pairs(mode, B, n, seed):
    g = sim.generate(B, n, seed=seed)
    pairs = [Pair(mode, g.bvs1[p].numpy(), g.bvs2[p].numpy(), g.covs2[p].numpy()) for p in range(B)]
    return pairs, g.init_q.numpy(), g.init_t.numpy()


def _oracle_pose(oracle, pr, q0, t0):
    """the oracle's own solve (analytic Jacobian) -> (q, unit t)"""
    s = oracle.solve(pr.mode, pr.f1, pr.f2, pr.c2, pr.c1, REG, q0, t0, oracle.default_options(jacobian_mode=oracle.JAC_ANALYTIC))
    return s.q, _vec(s.theta, s.phi)


def _batch(pairs):
    mode = pairs[0].mode
    off = np.concatenate([[0], np.cumsum([p.n for p in pairs])]).astype(np.int64)
    b = Batch(mode, off)
    cat = lambda xs: None if xs[0] is None else np.concatenate(xs)
    if off[-1] > 0:
        b.fill(cat([p.f1 for p in pairs]), cat([p.f2 for p in pairs]), cat([p.c2 for p in pairs]), cat([p.c1 for p in pairs]))
    return b


def _device(pairs, q, t, n_hyp=1, reg=REG):
    with _batch(pairs) as b:
        return b.pose_covariance(np.asarray(q, float).reshape(-1, 4), np.asarray(t, float).reshape(-1, 3), reg=reg, n_hyp=n_hyp)


def _check_info(dev, s, ref, what):
    H, Hd = ref["H"], dev.info[s]
    sc = np.sqrt(np.outer(np.diag(H), np.diag(H)))
    err = np.abs(Hd - H) / sc
    print(f"{what}: info max normalised error {err.max():.3e}")
    assert np.array_equal(Hd, Hd.T), what
    assert err.max() <= TOL, f"{what}: information off by {err.max():.3e} (normalised), bound {TOL}"
    gsc = np.sqrt(np.diag(H) * 2.0 * ref["cost"])   # |J_a'r| <= |J_a| |r|
    gerr = np.abs(dev.grad[s] - ref["grad"]) / gsc
    print(f"{what}: grad max normalised error {gerr.max():.3e}, cost rel {abs(dev.cost[s] - ref['cost']) / ref['cost']:.3e}")
    assert gerr.max() <= TOL, f"{what}: gradient off by {gerr.max():.3e}"
    assert dev.cost[s] == pytest.approx(ref["cost"], rel=TOL, abs=0.0), what


def _frame(C, bth, eph, t):
    T = np.zeros((6, 6))
    T[:3, :3] = np.eye(3)
    T[3, 3:], T[4, 3:], T[5, 3:] = bth, eph, t
    return T @ C @ T.T


def _cov_gap(C, Cref, bth, eph, t):
    """(largest normalised difference of the 5x5 tangent part, largest absolute entry along t / max|Sigma_tt|)"""
    G, Gr = _frame(C, bth, eph, t), _frame(Cref, bth, eph, t)
    d = np.sqrt(np.diag(Gr)[:5])
    tang = (np.abs(G[:5, :5] - Gr[:5, :5]) / np.outer(d, d)).max()
    along = max(np.abs(G[5, :]).max(), np.abs(G[:, 5]).max()) / np.abs(Cref[3:, 3:]).max()
    return tang, along


def _check_cov(dev, s, ref, t, what, bound=None):
    C = dev.cov[s]
    assert dev.status[s] == capi.COV_OK, f"{what}: status {dev.status[s]}"
    assert np.all(np.isfinite(C)), what
    assert np.array_equal(C, C.T), f"{what}: out_cov is not exactly symmetric"
    bound = 2.0 * ref["kappa"] * TOL if bound is None else bound
    tn = np.asarray(t) / np.linalg.norm(t)
    tang, along = _cov_gap(C, ref["cov"], ref["bth"], ref["eph"], tn)
    print(f"{what}: kappa {ref['kappa']:.3e}, covariance normalised error {tang:.3e} (bound {bound:.3e}), along t {along:.3e}")
    assert tang <= bound, f"{what}: covariance off by {tang:.3e} (normalised), bound {bound:.3e}, kappa {ref['kappa']:.3e}"
    assert along <= TOL, f"{what}: component along t {along:.3e} of max|Sigma_tt|"
    assert np.abs(C @ np.concatenate([np.zeros(3), tn])).max() <= TOL * np.abs(C).max(), f"{what}: Sigma_6 t != 0"


# ---- 1 + 2: information and covariance, every family, counts on every kind of ladder rung ---------------------------
# one-wavefront partial fill, a multiple of 64, 512, beyond 512 (two wavefronts), odd count of several wavefronts,
# beyond on-chip capacity of the solve (4096; SYM 2048): the pairs the solve streams
COUNTS = [37, 128, 512, 777, 2049, 5097]


@pytest.mark.parametrize("mode", FAMILIES, ids=FAMILY_IDS)
def test_information_and_covariance_match_oracle(oracle, mode):
    pairs, qs, ts = [], [], []
    for i, n in enumerate(COUNTS):
        (pr,), q0, t0 = _sim_pairs(mode, 1, n, seed=100 + i)
        q, t = _oracle_pose(oracle, pr, q0[0], t0[0])
        pairs.append(pr), qs.append(q), ts.append(t)
    dev = _device(pairs, qs, ts)          # one ragged batch: block sized for the largest pair
    for s, pr in enumerate(pairs):
        what = f"{FAMILY_IDS[mode]} n={pr.n}"
        ref = pr.reference(oracle, qs[s], ts[s])
        _check_info(dev, s, ref, what)
        _check_cov(dev, s, ref, ts[s], what)
    # the same pairs alone in a batch (block sized for that pair): the same bits
    for s in (0, 3):
        alone = _device([pairs[s]], qs[s], ts[s])
        assert np.array_equal(alone.cov[0], dev.cov[s]) and np.array_equal(alone.info[0], dev.info[s])


# ---- 3: independent of the chart algebra ----------------------------------------------------------------------------
def _make_pair(mode, n, t_dir, seed, sigma=2e-4):
    """a pair with a chosen translation direction: points in front of both cameras, Gaussian bearing noise in
    frame 2 with the covariance the pair carries -> (Pair, q_gt, t_gt)"""
    rng = np.random.default_rng(seed)
    ang = rng.uniform(-0.1, 0.1, 3)
    a, k = np.linalg.norm(ang), ang / np.linalg.norm(ang)
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    R = np.eye(3) + math.sin(a) * K + (1.0 - math.cos(a)) * K @ K          # Rodrigues
    q = np.append(k * math.sin(a / 2), math.cos(a / 2))
    t = np.asarray(t_dir, float) / np.linalg.norm(t_dir) * 0.5
    P = np.stack([rng.uniform(-3, 3, n), rng.uniform(-2, 2, n), rng.uniform(4, 12, n)], -1)
    f1 = P / np.linalg.norm(P, axis=1, keepdims=True)
    P2 = (P - t) @ R                      # R' (P - t)
    f2 = P2 / np.linalg.norm(P2, axis=1, keepdims=True)
    A = rng.normal(size=(n, 3, 3)) * sigma
    S2 = A @ np.transpose(A, (0, 2, 1)) + (0.1 * sigma) ** 2 * np.eye(3)
    f2 = f2 + np.einsum("nij,nj->ni", np.linalg.cholesky(S2), rng.normal(size=(n, 3)))
    f2 /= np.linalg.norm(f2, axis=1, keepdims=True)
    return Pair(mode, f1, f2, S2), q, t / np.linalg.norm(t)


def _quat_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


def _fd_cov(oracle, pr, q, t, h=1e-6):
    """Sigma_6 from a 5-column central-difference Jacobian of oracle.residual in the chart
    (Exp(omega) R, normalize(t + B tau)), B = any orthonormal basis of t-perp: shares no formula with the device"""
    t = t / np.linalg.norm(t)
    a = np.cross(t, [1.0, 0.0, 0.0] if abs(t[0]) < 0.9 else [0.0, 1.0, 0.0])
    a /= np.linalg.norm(a)
    B = np.stack([a, np.cross(t, a)], 1)

    def residuals(x):
        w = x[2:]
        ang = np.linalg.norm(w)
        dq = np.append(w / ang * math.sin(ang / 2), math.cos(ang / 2)) if ang > 0 else np.array([0.0, 0, 0, 1])
        qq = _quat_mul(dq, q)
        tt = t + B @ x[:2]
        th, ph = _angles(tt / np.linalg.norm(tt))
        return np.array([oracle.residual(pr.mode, pr.f1[i], pr.f2[i], None if pr.c2 is None else pr.c2[i],
                                         None if pr.c1 is None else pr.c1[i], REG, th, ph, qq) for i in range(pr.n)])
    J = np.zeros((pr.n, 5))
    for k in range(5):
        e = np.zeros(5)
        e[k] = h
        J[:, k] = (residuals(e) - residuals(-e)) / (2 * h)
    L = np.zeros((6, 5))
    L[3:, :2] = B
    L[:3, 2:] = np.eye(3)
    return L @ _inv_spd(J.T @ J) @ L.T


@pytest.mark.parametrize("mode", [TARGET, SYM], ids=["TARGET", "SYM"])
@pytest.mark.parametrize("t_dir,theta_max", [((1.0, 0.2, 0.1), None), ((0.015, 0.0, 1.0), 0.03), ((0.0007, 0.0007, 1.0), 4e-3)],
                         ids=["sideways", "theta0.015", "theta1e-3"])
def test_covariance_against_finite_differences_of_the_residual(oracle, mode, t_dir, theta_max):
    pr, q_gt, t_gt = _make_pair(mode, 200, t_dir, seed=7)
    q, t = _oracle_pose(oracle, pr, q_gt, t_gt)
    ref = pr.reference(oracle, q, t)
    if theta_max is not None:
        assert ref["theta"] < theta_max, ref["theta"]
    C_fd = _fd_cov(oracle, pr, q, t)
    g = max(_cov_gap(ref["cov"], C_fd, ref["bth"], ref["eph"], t))   # the differencing error, measured on the CPU
    dev = _device([pr], q, t)
    assert dev.status[0] == capi.COV_OK
    gap = max(_cov_gap(dev.cov[0], C_fd, ref["bth"], ref["eph"], t))
    print(f"theta {ref['theta']:.3e}: analytic-vs-FD gap g = {g:.3e}, device-vs-FD {gap:.3e}")
    assert gap <= 10 * g, f"theta {ref['theta']:.3e}: device vs finite differences {gap:.3e}, allowed 10 g, g = {g:.3e}"


# ---- 4: at the pole ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sign", [1.0, -1.0], ids=["+z", "-z"])
def test_translation_exactly_at_the_pole(oracle, sign):
    pr, q, _ = _make_pair(TARGET, 300, (0.0, 0.0, sign), seed=11)
    t = np.array([0.0, 0.0, sign])
    dev = _device([pr], q, t)
    assert dev.status[0] == capi.COV_OK and np.all(np.isfinite(dev.cov[0]))
    # reference in the orthonormal chart: e_phi = (0, 1, 0) is d t / d theta at phi = pi/2 (up to the sign of
    # cos theta): both columns come from the oracle's theta column, at the same t
    theta = 0.0 if sign > 0 else math.pi
    _, J0, _ = pr.evaluate(oracle, q, theta, 0.0)
    _, J1, _ = pr.evaluate(oracle, q, theta, math.pi / 2)
    Jx = np.column_stack([J0[:, 0], sign * J1[:, 0], J0[:, 2:] / 2.0])
    Hx = Jx.T @ Jx
    bth, eph = np.array([sign, 0.0, 0.0]), np.array([0.0, 1.0, 0.0])
    np.testing.assert_allclose(np.stack(chart_basis(t)[:2]), np.stack([bth, eph]), atol=1e-15)
    ref = dict(kappa=_kappa(Hx), cov=_lift(_inv_spd(Hx), bth, eph), bth=bth, eph=eph)
    _check_cov(dev, 0, ref, t, f"t = (0, 0, {sign:+.0f})")
    H = dev.info[0]
    if sign > 0:
        assert np.all(H[1, :] == 0.0) and np.all(H[:, 1] == 0.0), H
    else:
        assert np.all(np.abs(H[1, :]) <= 1e-15 * np.sqrt(np.abs(np.diag(H)) * H[0, 0]) + 0.0), H
    keep = [0, 2, 3, 4]
    Href = (J0.T @ J0)[np.ix_(keep, keep)]
    err = np.abs(H[np.ix_(keep, keep)] - Href) / np.sqrt(np.outer(np.diag(Href), np.diag(Href)))
    assert err.max() <= TOL, err.max()


# ---- 5: edges ---------------------------------------------------------------------------------------------------------
def test_too_few_correspondences_are_singular_not_a_fault(oracle):
    (full,), q0, t0 = _sim_pairs(TARGET, 1, 40, seed=3)
    pairs = [Pair(TARGET, full.f1[:k], full.f2[:k], full.c2[:k]) for k in (0, 1, 4, 5)]
    dev = _device(pairs, np.tile(q0[0], (4, 1)), np.tile(t0[0], (4, 1)))
    assert list(dev.status) == [capi.COV_SINGULAR] * 3 + [capi.COV_OK]
    assert np.all(np.isnan(dev.cov[:3])) and np.all(np.isfinite(dev.cov[3]))
    assert np.all(dev.info[0] == 0.0) and dev.cost[0] == 0.0
    for s in (1, 2, 3):   # the information is written all the same
        _check_info(dev, s, pairs[s].reference(oracle, q0[0], t0[0]), f"n={pairs[s].n}")


def test_nan_input_is_reported_for_its_pair_only():
    pairs, q0, t0 = _sim_pairs(TARGET, 5, 200, seed=4)
    clean = _device(pairs, q0, t0)
    bad = Pair(TARGET, pairs[2].f1.copy(), pairs[2].f2.copy(), pairs[2].c2)
    bad.f2[17, 1] = np.nan
    dev = _device(pairs[:2] + [bad] + pairs[3:], q0, t0)
    assert list(dev.status) == [0, 0, capi.COV_NONFINITE, 0, 0]
    assert np.all(np.isnan(dev.cov[2]))
    for s in (0, 1, 3, 4):
        for name in ("cov", "info", "grad", "cost"):
            assert np.array_equal(getattr(dev, name)[s], getattr(clean, name)[s]), (s, name)


def test_ragged_batch_with_an_empty_pair_in_the_middle(oracle):
    pairs, q0, t0 = _sim_pairs(HOST, 3, 90, seed=6)
    pairs[1] = Pair(HOST, pairs[1].f1[:0], pairs[1].f2[:0], pairs[1].c2[:0])
    dev = _device(pairs, q0, t0)
    assert list(dev.status) == [0, capi.COV_SINGULAR, 0]
    for s in (0, 2):
        ref = pairs[s].reference(oracle, q0[s], t0[s])
        _check_info(dev, s, ref, f"pair {s}")
        _check_cov(dev, s, ref, t0[s], f"pair {s}")


def test_hypotheses_device_space_and_views_are_bit_identical():
    torch = pytest.importorskip("torch")
    pairs, q0, t0 = _sim_pairs(TARGET, 4, 300, seed=8)
    rng = np.random.default_rng(1)
    q3 = np.repeat(q0, 3, axis=0) + rng.normal(size=(12, 4)) * 1e-3
    t3 = np.repeat(t0, 3, axis=0) + rng.normal(size=(12, 3)) * 1e-3
    names = ("cov", "info", "grad", "cost", "status")
    with _batch(pairs) as b:
        three = b.pose_covariance(q3, t3, n_hyp=3)
        for h in range(3):
            one = b.pose_covariance(q3[h::3], t3[h::3])
            for name in names:
                assert np.array_equal(getattr(three, name)[h::3], getattr(one, name)), (h, name)
        # device space == host space
        d = b.pose_covariance(torch.as_tensor(q3, device="cuda:0"), torch.as_tensor(t3, device="cuda:0"), n_hyp=3)
        assert d.cov.is_cuda and d.info.shape == (12, 5, 5)
        for name in names:
            assert np.array_equal(getattr(d, name).cpu().numpy(), getattr(three, name)), name
        # a select(view=True) batch == the same correspondences in a fresh batch
        mask = (rng.uniform(size=4 * 300) < 0.7).astype(np.uint8)
        v = b.select(mask, view=True)
        view = v.pose_covariance(q0, t0)
    kept = [Pair(TARGET, p.f1[m], p.f2[m], p.c2[m]) for p, m in zip(pairs, mask.reshape(4, 300).astype(bool))]
    fresh = _device(kept, q0, t0)
    for name in names:
        assert np.array_equal(getattr(view, name), getattr(fresh, name)), name


def test_reshaped_capacity_batch():
    pairs, q0, t0 = _sim_pairs(TARGET, 2, 150, seed=9)
    want = _device(pairs, q0, t0)
    with Batch.with_capacity(TARGET, 8, 4000) as b:
        b.reshape([0, 700, 1400]).fill(np.zeros((1400, 3)), np.zeros((1400, 3)), np.zeros((1400, 3, 3)))
        b.reshape([0, 150, 300])
        b.fill(np.concatenate([p.f1 for p in pairs]), np.concatenate([p.f2 for p in pairs]), np.concatenate([p.c2 for p in pairs]))
        got = b.pose_covariance(q0, t0)
    assert np.array_equal(got.cov, want.cov) and np.array_equal(got.info, want.info)


# ---- 6: surface -------------------------------------------------------------------------------------------------------
def test_solve_result_covariance_is_the_batch_call_at_its_own_pose():
    pairs, q0, t0 = _sim_pairs(TARGET, 3, 256, seed=12)
    with _batch(pairs) as b:
        res = b.solve(q0, t0, reg=1e-12)
        a, c = res.covariance(), b.pose_covariance(res.q, res.t, reg=1e-12)
        hyp = np.repeat(t0, 2, axis=0)
        res2 = b.solve(q0, None, hyp_t=hyp, n_hyp=2)
        a2, c2 = res2.covariance(), b.pose_covariance(res2.q, res2.t, n_hyp=2)
    for x, y in ((a, c), (a2, c2)):
        assert np.array_equal(x.cov, y.cov) and np.array_equal(x.info, y.info) and np.array_equal(x.status, y.status)
    assert a2.cov.shape == (6, 6, 6) and np.all(a.status == 0)


def _pose44(q, t, oracle):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = oracle.rot_from_quat(q), t
    return T


def test_pybind_and_facade_equal_the_batch_call(oracle):
    import pnec_amd.pypnec as pypnec
    (pr,), q0, t0 = _sim_pairs(TARGET, 1, 180, seed=13)
    # the facade takes a rotation MATRIX and makes its own quaternion of it.  Identity rotation: that quaternion is
    # (0, 0, 0, 1) whatever the conversion, so the facade runs the batch call's very inputs -> the same bits
    qi = np.array([0.0, 0.0, 0.0, 1.0])
    got = pypnec.pose_covariance(pr.f1, pr.f2, pr.c2, _pose44(qi, t0[0], oracle), 1e-13)
    assert got.shape == (6, 6)
    assert np.array_equal(got, _device([pr], qi, t0[0]).cov[0])
    # a general pose: the quaternion is the conversion's, equal to rounding
    got = pypnec.pose_covariance(pr.f1, pr.f2, pr.c2, _pose44(q0[0], t0[0], oracle), 1e-13)
    want = _device([pr], q0[0], t0[0]).cov[0]
    assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max()
    assert np.array_equal(got, got.T)
    # the demo walks the facade: it prints the 1-sigma uncertainties of its solve
    demo = os.path.join(ROOT, "pnec_amd", "pnec_host_demo")
    out = subprocess.run([demo], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    f = dict(kv.split("=") for kv in out.stdout.split())
    assert 0.0 < float(f["rot_sigma_deg"]) < 1.0 and 0.0 < float(f["t_sigma_deg"]) < 10.0, out.stdout


# ---- 7: scale ---------------------------------------------------------------------------------------------------------
def test_twenty_thousand_pairs_at_the_devices_solved_poses(oracle):
    torch = pytest.importorskip("torch")
    B, N, chunk = 20_000, 512, 5_000
    sample = np.linspace(0, B - 1, 200).astype(int)
    keep, qs, ts = {}, [], []
    with Batch.uniform(TARGET, B, N) as batch:
        for c in range(B // chunk):
            g = sim.generate(chunk, N, seed=2000 + c, device="cuda:0")
            batch.fill(g.bvs1.reshape(-1, 3), g.bvs2.reshape(-1, 3), g.covs2.reshape(-1, 3, 3), first_pair=c * chunk, n_pairs=chunk)
            qs.append(g.init_q), ts.append(g.init_t)
            for p in sample[(sample >= c * chunk) & (sample < (c + 1) * chunk)]:
                i = p - c * chunk
                keep[int(p)] = Pair(TARGET, g.bvs1[i].cpu().numpy(), g.bvs2[i].cpu().numpy(), g.covs2[i].cpu().numpy())
            del g
        res = batch.solve(torch.cat(qs), torch.cat(ts))
        pc = res.covariance()
        torch.cuda.synchronize()
    status, cov = pc.status.cpu().numpy(), pc.cov.cpu().numpy()
    assert np.all(status == capi.COV_OK), np.unique(status, return_counts=True)
    assert np.all(np.isfinite(cov)) and np.all(np.isfinite(pc.info.cpu().numpy()))
    d = np.diagonal(cov, axis1=1, axis2=2)
    assert np.all(d[:, :3] > 0.0) and np.all(d[:, 3:] >= 0.0)
    q, t = res.q.cpu().numpy(), res.t.cpu().numpy()

    class _Np:   # the sampled slots as numpy
        info, grad, cost = pc.info.cpu().numpy(), pc.grad.cpu().numpy(), pc.cost.cpu().numpy()
    _Np.cov, _Np.status = cov, status
    for p in sample:
        ref = keep[int(p)].reference(oracle, q[p], t[p])
        _check_info(_Np, p, ref, f"pair {p}")
        _check_cov(_Np, p, ref, t[p], f"pair {p}")
