"""Pose sensitivity (pnec_hip_pose_sensitivity) without a GPU: the arithmetic of pnec_amd/csrc/pnec_sensitivity.hpp, built
for the host by tools/sensitivity_host.cc under the address and undefined-behaviour sanitizers and run as a program of its
own, against a float64 torch reference written HERE from the formulas of include/pnec_hip.h -- never a device result.

The reference: the four residuals; R(omega) = (I + [omega]x + [omega]x^2 / 2) R (exact to second order, no 0/0 at
omega = 0); t(tau) = normalize(t + tau_1 b_theta + tau_2 e_phi); H from torch.autograd.functional.hessian (J'J from
jacobian for the Gauss-Newton variant); the mixed term from autograd.grad(..., create_graph=True).  Its residuals are
pinned to the golden-pinned oracle at 1e-9 by the first test.

Bounds (the issue's): H and g 1e-10, entries normalised by sqrt(G_aa G_bb) and sqrt(G_aa 2 cost), G the reference's J'J;
lambda and x_N 2 kappa 1e-10 of the array's largest entry in the slot, kappa the condition number of the Jacobi-scaled
reference H; per-correspondence arrays (2 kappa + 1) 1e-10 of the array's largest entry in the slot.

Finite differences of the oracle's solve (six probes, n = 200, TARGET) against the reference came out at 3e-7 .. 1.2e-4 of
the array maximum when this was written; the test asserts <= 1e-3 so that a broken yardstick cannot pass silently.
"""
import math
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

from pnec_amd import capi
from pnec_amd.batch import chart_basis

NEC, TARGET, HOST, SYM = capi.MODE_NEC, capi.MODE_TARGET, capi.MODE_HOST, capi.MODE_SYM
FAMILIES = [NEC, TARGET, HOST, SYM]
FAMILY_IDS = ["NEC", "TARGET", "HOST", "SYM"]
REG = 1e-13
TOL = 1e-10
T_DIR = (0.3, 0.1, 1.0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAUSS_NEWTON, ZERO_ON_FAILURE = 1, 2
OK, SINGULAR, NONFINITE = 0, 1, 2
F64 = torch.float64


# ---- pairs (a copy of test_pose_covariance_gpu._make_pair / _covs_for) -------------------------------------------------
def covs_for(mode, S2):
    if mode == NEC:
        return None, None
    if mode == SYM:
        return S2, np.roll(S2, 1, axis=0) * 0.8
    return S2, None


class Pair:
    def __init__(self, mode, f1, f2, S2):
        self.mode, self.f1, self.f2 = mode, np.ascontiguousarray(f1), np.ascontiguousarray(f2)
        self.c2, self.c1 = covs_for(mode, np.ascontiguousarray(S2))
        self.n = len(self.f1)

    def head(self, k):
        return Pair(self.mode, self.f1[:k], self.f2[:k], np.zeros((k, 3, 3)) if self.c2 is None else self.c2[:k])


def make_pair(mode, n, seed, t_dir=T_DIR, sigma=2e-4):
    """a pair with a chosen translation direction: points in front of both cameras, Gaussian bearing noise in frame 2
    with the covariance the pair carries -> (Pair, q_gt, t_gt)"""
    rng = np.random.default_rng(seed)
    ang = rng.uniform(-0.1, 0.1, 3)
    a, k = np.linalg.norm(ang), ang / np.linalg.norm(ang)
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    R = np.eye(3) + math.sin(a) * K + (1.0 - math.cos(a)) * K @ K
    q = np.append(k * math.sin(a / 2), math.cos(a / 2))
    t = np.asarray(t_dir, float) / np.linalg.norm(t_dir) * 0.5
    P = np.stack([rng.uniform(-3, 3, n), rng.uniform(-2, 2, n), rng.uniform(4, 12, n)], -1)
    f1 = P / np.linalg.norm(P, axis=1, keepdims=True)
    P2 = (P - t) @ R
    f2 = P2 / np.linalg.norm(P2, axis=1, keepdims=True)
    A = rng.normal(size=(n, 3, 3)) * sigma
    S2 = A @ np.transpose(A, (0, 2, 1)) + (0.1 * sigma) ** 2 * np.eye(3)
    f2 = f2 + np.einsum("nij,nj->ni", np.linalg.cholesky(S2), rng.normal(size=(n, 3)))
    f2 /= np.linalg.norm(f2, axis=1, keepdims=True)
    return Pair(mode, f1, f2, S2), q, t / np.linalg.norm(t)


def angles(t):
    rho = math.hypot(t[0], t[1])
    return math.atan2(rho, t[2]), (math.atan2(t[1], t[0]) if rho > 0 else 0.0)


def oracle_pose(oracle, pr, q0, t0, **opts):
    """the oracle's own solve (analytic Jacobian) -> (q, unit t, iterations)"""
    s = oracle.solve(pr.mode, pr.f1, pr.f2, pr.c2, pr.c1, REG, q0, t0, oracle.default_options(jacobian_mode=oracle.JAC_ANALYTIC, **opts))
    return s.q, np.array([math.sin(s.theta) * math.cos(s.phi), math.sin(s.theta) * math.sin(s.phi), math.cos(s.theta)]), s.iterations


def perpendicular(t):
    t = np.asarray(t, float) / np.linalg.norm(t)
    a = np.cross(t, [1.0, 0.0, 0.0] if abs(t[0]) < 0.9 else [0.0, 1.0, 0.0])
    return a / np.linalg.norm(a)


# ---- the reference -------------------------------------------------------------------------------------------------------
def _skew(w):
    z = torch.zeros((), dtype=F64)
    return torch.stack([torch.stack([z, -w[2], w[1]]), torch.stack([w[2], z, -w[0]]), torch.stack([-w[1], w[0], z])])


def rot_of_quat(q):
    """Eigen's toRotationMatrix of the normalised q (xyzw)"""
    x, y, z, w = torch.as_tensor(q, dtype=F64) / torch.linalg.norm(torch.as_tensor(q, dtype=F64))
    return torch.stack([torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)]),
                        torch.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)]),
                        torch.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)])])


def residuals_t(mode, f1, f2, S2, S1, reg, R, t):
    """r [n]: m = t x f1, g = R'm, n = f2.g, h = t x (R a)"""
    tt = t.expand_as(f1)
    g = torch.linalg.cross(tt, f1) @ R
    n = (f2 * g).sum(-1)
    if mode == NEC:
        return n
    quad = lambda S, v: torch.einsum("ni,nij,nj->n", v, S, v)
    if mode == TARGET:
        den = quad(S2, g)
    else:
        h = torch.linalg.cross(tt, (f2 if mode == SYM else f1) @ R.T)
        den = quad(S2, h) if mode == HOST else quad(S2, g) + quad(S1, h)
    return n / torch.sqrt(den + reg)


class Reference:
    """everything pnec_hip_pose_sensitivity defines, for one slot"""

    def __init__(self, pr, q, t, grad_pose, reg=REG, gauss_newton=False):
        self.pr = pr
        td = lambda a: None if a is None else torch.tensor(a, dtype=F64)
        self.in_ = [td(pr.f1), td(pr.f2), td(pr.c2), td(pr.c1)]
        bth, eph, _ = chart_basis(t)
        self.B = torch.tensor(np.stack([bth, eph], 1), dtype=F64)        # [3,2]
        self.t0 = torch.tensor(np.asarray(t, float) / np.linalg.norm(t), dtype=F64)
        self.R0 = rot_of_quat(q)
        self.reg = reg
        x0 = torch.zeros(5, dtype=F64)
        res = lambda x: self.residuals(x, *self.in_)
        r = res(x0)
        self.cost = 0.5 * float((r * r).sum())
        J = torch.autograd.functional.jacobian(res, x0) if pr.n else torch.zeros((0, 5), dtype=F64)
        self.G = (J.T @ J).numpy()
        self.g = (J.T @ r).numpy()
        if gauss_newton or pr.n == 0:
            self.H = self.G.copy()
        else:
            H = torch.autograd.functional.hessian(lambda x: 0.5 * (res(x) ** 2).sum(), x0).numpy()
            self.H = 0.5 * (H + H.T)
        gp = np.asarray(grad_pose, float)
        self.v = np.concatenate([[bth @ gp[3:], eph @ gp[3:]], gp[:3]])
        d = np.diag(self.H)
        self.positive = bool(np.all(d > 0))
        if self.positive:
            s = 1.0 / np.sqrt(d)
            self.scaled = self.H * np.outer(s, s)
            ev = np.linalg.eigvalsh(self.scaled)
            self.min_eig, self.kappa = ev[0], (ev[-1] / ev[0] if ev[0] > 0 else math.inf)
            self.positive = ev[0] > 0
        else:
            self.min_eig, self.kappa = -math.inf, math.inf
        self.ok = self.positive and pr.n >= 5
        if self.ok:
            self.lam = s * np.linalg.solve(self.scaled, s * self.v)
            self.newton = -s * np.linalg.solve(self.scaled, s * self.g)
            self.grads = self.input_gradients(self.lam, gauss_newton)

    def pose(self, x):
        K = _skew(x[2:])
        R = (torch.eye(3, dtype=F64) + K + 0.5 * K @ K) @ self.R0
        t = self.t0 + self.B @ x[:2]
        return R, t / torch.linalg.norm(t)

    def residuals(self, x, f1, f2, S2, S1):
        R, t = self.pose(x)
        return residuals_t(self.pr.mode, f1, f2, S2, S1, self.reg, R, t)

    def input_gradients(self, lam, gauss_newton=False):
        """-d/d theta [lambda . grad_x E] -> (grad_bvs1, grad_bvs2, grad_covs or None, grad_covs_host or None).  (The
        mixed term is the same with either H: the flag changes lambda only.)"""
        ins = [None if a is None else a.clone().requires_grad_(True) for a in self.in_]
        x = torch.zeros(5, dtype=F64, requires_grad=True)
        E = 0.5 * (self.residuals(x, *ins) ** 2).sum()
        (gx,) = torch.autograd.grad(E, x, create_graph=True)
        phi = (torch.tensor(lam, dtype=F64) * gx).sum()
        live = [a for a in ins if a is not None]
        got = iter(torch.autograd.grad(phi, live))
        return [None if a is None else -next(got).numpy() for a in ins]


def check_slot(ref, dev, what, report=None):
    """dev: dict(H [5,5], g, lam, newton, status, grads [4]) of one slot against the reference, within the bounds"""
    G = ref.G
    sc = np.sqrt(np.outer(np.diag(G), np.diag(G)))
    eH = (np.abs(dev["H"] - ref.H) / sc).max()
    eg = (np.abs(dev["g"] - ref.g) / np.sqrt(np.diag(G) * 2.0 * ref.cost)).max()
    rel = lambda a, b: np.abs(a - b).max() / np.abs(b).max()
    el, en = rel(dev["lam"], ref.lam), rel(dev["newton"], ref.newton)
    ec = [0.0 if b is None else rel(a, b) for a, b in zip(dev["grads"], ref.grads)]
    print(f"{what}: kappa {ref.kappa:.1f}  H {eH:.2e}  g {eg:.2e}  lambda {el:.2e}  x_N {en:.2e}  "
          f"bvs1 {ec[0]:.2e} bvs2 {ec[1]:.2e} covs {ec[2]:.2e} covs_host {ec[3]:.2e}")
    if report is not None:
        report.append((what, eH, eg, el, en, max(ec)))
    assert dev["status"] == OK, f"{what}: status {dev['status']}"
    assert eH <= TOL and eg <= TOL, f"{what}: H off by {eH:.3e}, g by {eg:.3e} (normalised), bound {TOL}"
    bound = 2.0 * ref.kappa * TOL
    assert el <= bound and en <= bound, f"{what}: lambda off by {el:.3e}, x_N by {en:.3e} of the maximum, bound {bound:.3e}"
    assert max(ec) <= bound + TOL, f"{what}: per-correspondence gradients off by {ec} of the maximum, bound {bound + TOL:.3e}"


# ---- the host tool ---------------------------------------------------------------------------------------------------------
def planes_of(pr):
    tri = lambda S: np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]])
    rows = [pr.f1.T, pr.f2.T]
    if pr.mode != NEC:
        rows.append(tri(pr.c2))
    if pr.mode == SYM:
        rows.append(tri(pr.c1))
    return np.ascontiguousarray(np.concatenate(rows), dtype=np.float64)


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ builds the host facade, so it is there"
    exe = str(tmp_path_factory.mktemp("sens") / "sensitivity_host")
    subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "pnec_amd", "csrc"),
                    os.path.join(ROOT, "tools", "sensitivity_host.cc"), "-o", exe], check=True)

    def run(problems):
        """problems: [(Pair, q, t, grad_pose, flags)] -> [dict] (one process for all of them)"""
        d = os.path.dirname(exe)
        with open(os.path.join(d, "in.bin"), "wb") as f:
            f.write(struct.pack("<i", len(problems)))
            for pr, q, t, gp, flags in problems:
                f.write(struct.pack("<4i", pr.mode, pr.n, flags, 0))
                f.write(np.concatenate([[REG], q, t, gp]).astype("<f8").tobytes())
                f.write(planes_of(pr).astype("<f8").tobytes())
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
        r = subprocess.run([exe, os.path.join(d, "in.bin"), os.path.join(d, "out.bin")], env=env, capture_output=True, text=True)
        assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
        raw, at, out = open(os.path.join(d, "out.bin"), "rb").read(), 0, []
        for pr, *_ in problems:
            status = struct.unpack_from("<2i", raw, at)[0]
            v = np.frombuffer(raw, "<f8", 30 + 24 * pr.n, at + 8)
            at += 8 + 8 * len(v)
            H = np.zeros((5, 5))
            H[np.triu_indices(5)] = v[:15]
            H = H + np.triu(H, 1).T
            n, per = pr.n, v[30:]
            grads = [per[:3 * n].reshape(n, 3), per[3 * n:6 * n].reshape(n, 3), per[6 * n:15 * n].reshape(n, 3, 3),
                     per[15 * n:].reshape(n, 3, 3)]
            out.append(dict(status=status, H=H, g=v[15:20], lam=v[20:25], newton=v[25:30], grads=grads))
        assert at == len(raw)
        return out
    return run


GRAD_POSE = np.array([0.7, -0.4, 0.9, 0.5, 1.1, -0.3])


# ---- tests -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", FAMILIES, ids=FAMILY_IDS)
def test_reference_residuals_are_the_oracles(oracle, mode):
    pr, q, t = make_pair(mode, 37, seed=1)
    th, ph = angles(t)
    ref = Reference(pr, q, t, GRAD_POSE)
    r = ref.residuals(torch.zeros(5, dtype=F64), *ref.in_).numpy()
    want = np.array([oracle.residual(mode, pr.f1[i], pr.f2[i], None if pr.c2 is None else pr.c2[i],
                                     None if pr.c1 is None else pr.c1[i], REG, th, ph, q) for i in range(pr.n)])
    assert np.abs(r - want).max() <= 1e-9 * np.abs(want).max()


COUNTS = [5, 8, 37, 130]


@pytest.mark.parametrize("mode", FAMILIES, ids=FAMILY_IDS)
def test_host_build_matches_the_reference(oracle, tool, mode):
    cases = []
    for i, n in enumerate(COUNTS):
        pr, q_gt, t_gt = make_pair(mode, n, seed=40 + i)
        q_min, t_min, _ = oracle_pose(oracle, pr, q_gt, t_gt)
        for where, (q, t) in (("minimiser", (q_min, t_min)), ("ground truth", (q_gt, t_gt))):
            for flags in (0, GAUSS_NEWTON):
                cases.append((f"{FAMILY_IDS[mode]} n={n} {where} {'J^TJ' if flags else 'full'}", pr, q, t, flags))
    out = tool([(pr, q, t, GRAD_POSE, flags) for _, pr, q, t, flags in cases])
    checked = 0
    for (what, pr, q, t, flags), dev in zip(cases, out):
        ref = Reference(pr, q, t, GRAD_POSE, gauss_newton=bool(flags))
        if not ref.ok:     # (n = 5 and 6 are not reliably positive definite: the verdicts must agree, nothing else is defined)
            assert dev["status"] == SINGULAR, what
            continue
        check_slot(ref, dev, what)
        checked += 1
    assert checked >= 12   # n >= 8 is positive definite at both poses


def test_statuses_follow_the_references_verdict(oracle, tool):
    full, q, t = make_pair(TARGET, 40, seed=3)
    problems, want = [], []
    for k in (0, 1, 4):
        problems.append((full.head(k), q, t, GRAD_POSE, 0))
        want.append(SINGULAR)
    for n in (8, 65):
        pr, qg, tg = make_pair(TARGET, n, seed=60 + n)
        tp = perpendicular(tg)
        ref = Reference(pr, qg, tp, GRAD_POSE)
        assert not ref.positive and ref.min_eig < 0.0, (n, ref.min_eig)    # the precondition, on the reference
        problems += [(pr, qg, tp, GRAD_POSE, 0), (pr, qg, tp, GRAD_POSE, ZERO_ON_FAILURE)]
        want += [SINGULAR, SINGULAR]
    bad = Pair(TARGET, full.f1.copy(), full.f2.copy(), full.c2)
    bad.f2[17, 1] = np.nan
    problems += [(bad, q, t, GRAD_POSE, 0), (bad, q, t, GRAD_POSE, ZERO_ON_FAILURE)]
    want += [NONFINITE, NONFINITE]
    out = tool(problems)
    assert [o["status"] for o in out] == want
    for (pr, _, _, _, flags), o in zip(problems, out):
        arrays = [o["lam"], o["newton"], o["grads"][0], o["grads"][1], o["grads"][2]]
        for a in arrays:
            assert np.all(a == 0.0) if flags & ZERO_ON_FAILURE else np.all(np.isnan(a))
    # H and g are written as computed
    ref = Reference(problems[3][0], problems[3][1], problems[3][2], GRAD_POSE)
    sc = np.sqrt(np.outer(np.diag(ref.G), np.diag(ref.G)))
    assert (np.abs(out[3]["H"] - ref.H) / sc).max() <= TOL
    assert np.all(out[0]["H"] == 0.0) and np.all(out[0]["g"] == 0.0)


# ---- finite differences of the oracle's solve: the yardstick's own yardstick -------------------------------------------------
W_Q, W_T = np.array([0.3, -0.8, 0.5, 0.2]), np.array([0.6, -0.2, 0.9])
PROBES = [("f2", 3, 0), ("f2", 77, 1), ("f2", 150, 2), ("S2", 10, (0, 0)), ("S2", 101, (0, 1)), ("S2", 199, (2, 2))]


def grad_pose_of(q, grad_q, grad_t):
    """(dL/d omega, dL/d t) from the gradient with respect to q = (v, w) xyzw, for R <- Exp(omega) R"""
    v, w, gv, gw = q[:3], q[3], grad_q[:3], grad_q[3]
    return np.concatenate([0.5 * (w * gv + np.cross(v, gv) - gw * v), grad_t])


def fd_case(oracle):
    """-> (pair, q, t, grad_pose, [(probe, finite difference, factor)]) at the oracle's tightly converged minimiser of a
    TARGET pair of 200; factor: an off-diagonal covariance probe moves both stored entries"""
    pr, q_gt, t_gt = make_pair(TARGET, 200, seed=7)
    tight = dict(function_tolerance=0.0, gradient_tolerance=0.0, parameter_tolerance=0.0, max_num_iterations=200)
    q, t, _ = oracle_pose(oracle, pr, q_gt, t_gt, **tight)

    def loss(f2, c2):
        s = oracle.solve(TARGET, pr.f1, f2, c2, None, REG, q, t, oracle.default_options(jacobian_mode=oracle.JAC_ANALYTIC, **tight))
        qq = s.q if s.q @ q > 0 else -s.q
        return W_Q @ qq + W_T @ s.t
    fds = []
    for name, i, at in PROBES:
        vals = []
        for sign in (1.0, -1.0):
            f2, c2 = pr.f2.copy(), pr.c2.copy()
            if name == "f2":
                h = 1e-6
                f2[i, at] += sign * h
            else:
                h = 1e-3 * abs(c2[i][at])
                c2[i][at] += sign * h
                if at[0] != at[1]:
                    c2[i][at[::-1]] += sign * h
            vals.append(loss(f2, c2))
        fds.append(((name, i, at), (vals[0] - vals[1]) / (2 * h), 2.0 if name == "S2" and at[0] != at[1] else 1.0))
    return pr, q, t, grad_pose_of(q, W_Q, W_T), fds


def fd_gaps(fds, grad_bvs2, grad_covs):
    """each probe's |finite difference - analytic| as a share of its array's largest entry"""
    gaps = []
    for (name, i, at), fd, factor in fds:
        arr = grad_bvs2 if name == "f2" else grad_covs
        gaps.append(abs(fd - factor * arr[i][at]) / (factor * np.abs(arr).max()))
    return gaps


def test_reference_against_finite_differences_of_the_oracles_solve(oracle):
    pr, q, t, gp, fds = fd_case(oracle)
    ref = Reference(pr, q, t, gp)
    assert ref.ok
    g_fd = fd_gaps(fds, ref.grads[1], ref.grads[2])
    print("g_fd per probe:", " ".join(f"{g:.2e}" for g in g_fd))
    assert max(g_fd) <= 1e-3, g_fd


# ---- the ABI, without a device ---------------------------------------------------------------------------------------------------
def test_abi_refusals_before_any_device():
    import ctypes as C
    L = capi.lib()
    buf = np.zeros(64)
    p = buf.ctypes.data
    # a stand-in handle: this box may have no device, and a real problem cannot be created without one.  Every refusal
    # returns before the handle's device is touched; the family checks read the handle's mode, the second int of the
    # struct (pnec_internal.hpp), which the stand-in sets
    fake = C.create_string_buffer(4096)
    h = C.cast(fake, C.c_void_p)

    def call(mode=TARGET, **kw):
        struct.pack_into("<2i", fake, 0, 0, mode)
        args = [kw.get("h", h), kw.get("q", p), kw.get("t", p), kw.get("gp", p), kw.get("n_hyp", 1), 1e-13, kw.get("flags", 0),
                None, None, kw.get("oc", None), kw.get("och", None), kw.get("lam", p), None, None, None, None,
                kw.get("space", capi.MEM_HOST), None]
        rc = L.pnec_hip_pose_sensitivity(*args)
        return rc, (L.pnec_hip_last_error() or b"").decode()

    for kw, word in ((dict(h=None), "problem"), (dict(q=None), "q or t"), (dict(t=None), "q or t"), (dict(gp=None), "grad_pose"),
                     (dict(n_hyp=0), "n_hyp"), (dict(flags=4), "flags"), (dict(flags=-1), "flags"), (dict(lam=None), "every output"),
                     (dict(mode=NEC, oc=p), "out_grad_covs"), (dict(mode=NEC, och=p), "out_grad_covs_host"),
                     (dict(mode=TARGET, och=p), "out_grad_covs_host"), (dict(mode=HOST, och=p), "out_grad_covs_host"),
                     (dict(space=7), "memory space")):
        rc, msg = call(**kw)
        assert rc == capi.ERR_INVALID_ARGUMENT == -1, (kw, rc, msg)
        assert word in msg, (kw, msg)
    assert np.all(buf == 0.0)


def test_declared_in_the_header_and_the_binding():
    assert "pnec_hip_pose_sensitivity" in capi.SYMBOLS
    header = open(os.path.join(ROOT, "include", "pnec_hip.h")).read()
    assert "int pnec_hip_pose_sensitivity(pnec_hip_problem *p" in header
    assert (capi.SENS_OK, capi.SENS_SINGULAR, capi.SENS_NONFINITE) == (0, 1, 2)
    assert (capi.SENS_GAUSS_NEWTON, capi.SENS_ZERO_ON_FAILURE) == (1, 2)
    for name, value in (("PNEC_HIP_SENS_GAUSS_NEWTON", 1), ("PNEC_HIP_SENS_ZERO_ON_FAILURE", 2), ("PNEC_HIP_SENS_SINGULAR", 1),
                        ("PNEC_HIP_SENS_NONFINITE", 2)):
        assert f"{name} = {value}" in header, name


def test_the_calls_arrays_are_counted(tmp_path):
    gxx = shutil.which("g++")
    exe = str(tmp_path / "call_arrays_host")
    subprocess.run([gxx, "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "pnec_amd", "csrc"),
                    os.path.join(ROOT, "tools", "call_arrays_host.cc"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    assert any(line.startswith("ok   pose_sensitivity(") for line in r.stdout.splitlines())
