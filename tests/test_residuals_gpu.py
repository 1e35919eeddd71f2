"""Per-correspondence residuals and the chi-square gate (pnec_hip_residuals) against the CPU oracle.

The yardstick for a residual is always the oracle's `evaluate(mode, JAC_ANALYTIC, ...)` at the same (q, t) that is handed
to the device; for the energy, the numbers the reference's own Python returned (tests/golden); for a variance, a numpy
restatement of the denominator.  Never a device result.

Bounds:
* residual: 1e-10 on |dr| / max(1, |r|) -- the project's bar for device-versus-checker values of this arithmetic
  (test_pose_covariance_gpu.TOL).
* variance: relative 1e-12 (nine products and a sum in another order); NEC exactly 1.
* energies against the goldens: relative 1e-10 (TARGET, NEC) / 1e-9 (HOST, SYM), the bounds test_parity_gpu uses.
* sums against sums of the device's own per-correspondence values: relative 1e-12 -- summation order only; n eps =
  4.5e-13 bounds the re-ordering of 4096 non-negative terms.
* mask against the CPU mask: equal, except where the oracle's |r| lies within relative 1e-9 of the gate; at most 1 such
  correspondence per 10 000 (on these inputs the oracle has none within 1e-6).

Outlier recipes (24 pairs x 400, sim.generate(seed=131), injected into bvs2 of a random quarter of each pair's tracks,
covariances left as they were, i.e. undeclared):
* gross: the bearing is replaced by a random unit vector;
* mild: the bearing is moved by 8 of its own sigmas -- by V sqrt(L) u * 8 with (L, V) the eigen-decomposition of its
  covariance and u a random unit vector of the covariance's plane -- and normalised again.
  With this injection and default_rng(7) the CPU oracle alone gives: gate 4 keeps 37 % of the mild outliers, the RANSAC
  mask 63 % (the issue's own injection, of which only "8 of its own sigmas" is written down, gave 27 % against 43 %).
"""
import math
import os

import numpy as np
import pytest

from pnec_amd import Batch, capi
from pnec_amd import simulation as sim

pytestmark = pytest.mark.gpu

NEC, TARGET, HOST, SYM = capi.MODE_NEC, capi.MODE_TARGET, capi.MODE_HOST, capi.MODE_SYM
FAMILIES = [NEC, TARGET, HOST, SYM]
FAMILY_IDS = ["NEC", "TARGET", "HOST", "SYM"]
REG = 1e-13
TOL = 1e-10
VAR_TOL = 1e-12
SUM_TOL = 1e-12
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


def _quat_to_R(q):
    x, y, z, w = np.asarray(q, float) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _quad(S, g):
    """g_i' S_i g_i as the header states it: S g first, then the dot product"""
    return np.einsum("ni,ni->n", g, np.einsum("nij,nj->ni", S, g))


class Pair:
    """one pair of a family, numpy arrays"""

    def __init__(self, mode, f1, f2, S2):
        self.mode, self.f1, self.f2 = mode, np.ascontiguousarray(f1), np.ascontiguousarray(f2)
        self.c2, self.c1 = _covs_for(mode, np.ascontiguousarray(S2))
        self.n = len(self.f1)

    def oracle_r(self, oracle, q, t, reg=REG):
        theta, phi = _angles(t)
        return oracle.evaluate(self.mode, oracle.JAC_ANALYTIC, self.f1, self.f2, self.c2, self.c1, reg, theta, phi,
                               np.asarray(q, float) / np.linalg.norm(q))[0]

    def variance(self, q, t, reg=REG):
        """the denominators of include/pnec_hip.h in numpy: g = R'(t x f1); TARGET g' S g + reg; HOST h' S h + reg with
        h = t x (R f1); SYM g' S2 g + h' S1 h + reg with h = t x (R f2); NEC 1"""
        if self.mode == NEC:
            return np.ones(self.n)
        R, tn = _quat_to_R(q), np.asarray(t, float) / np.linalg.norm(t)
        g = np.cross(tn, self.f1) @ R
        if self.mode == TARGET:
            return _quad(self.c2, g) + reg
        h = np.cross(tn, (self.f2 if self.mode == SYM else self.f1) @ R.T)
        if self.mode == HOST:
            return _quad(self.c2, h) + reg
        return _quad(self.c1, h) + reg + _quad(self.c2, g)

    def take(self, keep):
        out = Pair.__new__(Pair)
        out.mode, out.f1, out.f2 = self.mode, self.f1[keep], self.f2[keep]
        out.c2 = None if self.c2 is None else self.c2[keep]
        out.c1 = None if self.c1 is None else self.c1[keep]
        out.n = len(out.f1)
        return out


def _sim_pairs(mode, B, n, seed):
    g = sim.generate(B, n, seed=seed)
    pairs = [Pair(mode, g.bvs1[p].numpy(), g.bvs2[p].numpy(), g.covs2[p].numpy()) for p in range(B)]
    return pairs, g


def _batch(pairs):
    mode = pairs[0].mode
    off = np.concatenate([[0], np.cumsum([p.n for p in pairs])]).astype(np.int64)
    b = Batch(mode, off)
    cat = lambda xs: None if xs[0] is None else np.concatenate(xs)
    if off[-1] > 0:
        b.fill(cat([p.f1 for p in pairs]), cat([p.f2 for p in pairs]), cat([p.c2 for p in pairs]), cat([p.c1 for p in pairs]))
    return b


def _poses(q, t):
    return np.asarray(q, float).reshape(-1, 4), np.asarray(t, float).reshape(-1, 3)


def _device(pairs, q, t, gate=3.0, n_hyp=1, reg=REG):
    with _batch(pairs) as b:
        return b.residuals(*_poses(q, t), reg=reg, gate=gate, n_hyp=n_hyp)


def _random_quat(rng):
    q = rng.standard_normal(4)
    return q / np.linalg.norm(q)


def _gt_quat(oracle, g, p):
    return oracle.quat_from_rot(g.R_gt[p].numpy())


def _rel(a, b):
    return abs(a - b) / abs(b) if b != 0 else abs(a)


# ---- 1: per-correspondence parity ---------------------------------------------------------------------------------
SIZES = [1, 5, 63, 64, 65, 512, 513, 4096]


@pytest.mark.parametrize("pose", ["near", "far", "pole"])
@pytest.mark.parametrize("mode", FAMILIES, ids=FAMILY_IDS)
def test_residual_and_variance_match_the_oracle(oracle, mode, pose):
    rng = np.random.default_rng(50 + mode)
    pairs, qs, ts = [], [], []
    for i, n in enumerate(SIZES):
        (pr,), g = _sim_pairs(mode, 1, n, seed=300 + i)
        pairs.append(pr)
        if pose == "near":      # the ground truth: within the noise of the optimum
            qs.append(_gt_quat(oracle, g, 0)); ts.append(g.t_gt[0].numpy())
        elif pose == "far":     # anywhere
            qs.append(_random_quat(rng)); ts.append(rng.standard_normal(3) * 3.0)
        else:                   # forward motion, the chart's pole
            qs.append(g.init_q[0].numpy()); ts.append(np.array([0.0, 0.0, 1.0]))
    rep = _device(pairs, qs, ts)
    assert np.array_equal(rep.offsets, np.concatenate([[0], np.cumsum(SIZES)]))
    worst_r = worst_v = 0.0
    for p, pr in enumerate(pairs):
        sl = slice(rep.offsets[p], rep.offsets[p + 1])
        want = pr.oracle_r(oracle, qs[p], ts[p])
        err = (np.abs(rep.residual[sl] - want) / np.maximum(1.0, np.abs(want))).max()
        worst_r = max(worst_r, err)
        assert err <= TOL, f"n={pr.n} {pose}: residual off by {err:.3e}"
        den = pr.variance(qs[p], ts[p])
        if mode == NEC:
            assert np.array_equal(rep.variance[sl], np.ones(pr.n))
        else:
            verr = (np.abs(rep.variance[sl] - den) / den).max()
            worst_v = max(worst_v, verr)
            assert verr <= VAR_TOL, f"n={pr.n} {pose}: variance off by {verr:.3e} (relative)"
    print(f"{FAMILY_IDS[mode]} {pose}: residual max error {worst_r:.3e}, variance max relative error {worst_v:.3e}")


# ---- 2: pinned to the reference -------------------------------------------------------------------------------------
def test_chi2_equals_the_reference_pythons_energies(golden_dir, oracle):
    z = np.load(f"{golden_dir}/energy_golden.npz")
    checked = 0
    for i in range(int(z["n_cases"])):
        k = f"case{i:03d}_"
        f1, f2, S = z[k + "f1"], z[k + "f2"], z[k + "sigmas"]
        reg = float(z[k + "reg"])
        rots = z[k + "rotations"].reshape(4, 3, 3)
        n = len(f1)
        q0 = np.stack([oracle.quat_from_rot(R) for R in rots])
        t0 = np.tile(z[k + "t"], (4, 1))
        for mode, key in ((TARGET, "pnec_energy_rotations"), (NEC, "nec_energy_rotations")):
            with Batch.uniform(mode, 1, n) as b:
                b.fill(f1, f2, None if mode == NEC else S)
                rep = b.residuals(q0, t0, reg=reg if mode != NEC else 0.0, n_hyp=4)
            np.testing.assert_allclose(rep.chi2, z[k + key].reshape(4), rtol=1e-10)
            checked += 4
    assert checked == 36 * 8


def test_host_and_symmetric_chi2_equal_the_reference_pythons_numbers(golden_dir, oracle):
    z = np.load(f"{golden_dir}/residual_forms_golden.npz")
    n = int(z["n_cases"])
    for i in range(n):
        k = f"form{i:03d}_"
        f1, f2, c1, c2, R, t = (z[k + a] for a in ("f1", "f2", "cov1", "cov2", "R", "t"))
        reg = float(z[k + "reg"])
        q0, t0 = oracle.quat_from_rot(R)[None], t[None]
        off = np.array([0, len(f1)], dtype=np.int64)
        with Batch(HOST, off) as b:
            b.fill(f1, f2, c1)
            rep = b.residuals(q0, t0, reg=reg)
        np.testing.assert_allclose(rep.chi2, [float(z[k + "host_energy"])], rtol=1e-9)
        with Batch(SYM, off) as b:
            b.fill(f1, f2, c2, c1)
            rep = b.residuals(q0, t0, reg=reg)
        np.testing.assert_allclose(rep.chi2, [float(z[k + "sym_r2"].sum())], rtol=1e-9)
    assert n == 24


# ---- 3: internal consistency ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", FAMILIES, ids=FAMILY_IDS)
def test_slot_sums_are_the_sums_of_the_per_correspondence_values(oracle, mode):
    pairs, qs, ts = [], [], []
    for i, n in enumerate(SIZES):
        (pr,), g = _sim_pairs(mode, 1, n, seed=340 + i)
        pairs.append(pr); qs.append(_gt_quat(oracle, g, 0)); ts.append(g.t_gt[0].numpy())
    # NEC residuals are not whitened (~1e-4): a gate that splits them; the whitened ones are split by 1 sigma
    gate = 1.0 if mode != NEC else 2e-4
    with _batch(pairs) as b:
        q, t = _poses(qs, ts)
        rep = b.residuals(q, t, gate=gate)
        pc = b.pose_covariance(q, t)
        res = b.solve(q, t, options=capi.default_options(max_num_iterations=0))
    split = 0
    for p, pr in enumerate(pairs):
        sl = slice(rep.offsets[p], rep.offsets[p + 1])
        r, m = rep.residual[sl], rep.mask[sl].astype(bool)
        assert set(np.unique(rep.mask[sl])) <= {0, 1}
        assert np.array_equal(m, np.abs(r) <= gate)
        assert _rel(rep.chi2[p], np.sum(r * r)) <= SUM_TOL
        assert _rel(rep.gated_chi2[p], np.sum(r[m] ** 2)) <= SUM_TOL
        assert rep.gated_count[p] == m.sum()
        assert rep.max_abs[p] == np.abs(r).max()
        assert _rel(0.5 * rep.chi2[p], pc.cost[p]) <= SUM_TOL
        assert _rel(0.5 * rep.chi2[p], res.cost[p]) <= SUM_TOL
        split += int(0 < m.sum() < pr.n)
    assert split >= 4, "the gate was meant to split the larger pairs"


def test_solve_result_residuals_uses_the_solves_poses_and_reg(oracle):
    pairs, g = _sim_pairs(TARGET, 6, 300, seed=77)
    with _batch(pairs) as b:
        res = b.solve(g.init_q.numpy(), g.init_t.numpy(), reg=1e-12)
        rep = res.residuals(gate=2.0)
        want = b.residuals(res.q, res.t, reg=1e-12, gate=2.0)
    assert np.array_equal(rep.residual, want.residual) and np.array_equal(rep.mask, want.mask)
    for p in range(6):
        assert _rel(0.5 * rep.chi2[p], res.cost[p]) <= SUM_TOL
    vf = rep.variance_factor()
    print("variance factors at the solved poses:", vf)
    assert np.array_equal(vf, rep.chi2 / 295.0) and np.all(vf > 0.0)


# ---- 4 + 7: the mask is the CPU mask; what the gate is for -------------------------------------------------------------
GATE_B, GATE_N = 24, 400


def _inject(kind, f2, S, rng):
    f2o, out = f2.copy(), np.zeros(f2.shape[:2], dtype=bool)
    for p in range(f2.shape[0]):
        idx = rng.permutation(f2.shape[1])[: f2.shape[1] // 4]
        out[p, idx] = True
        if kind == "gross":
            v = rng.standard_normal((len(idx), 3))
        else:
            w, V = np.linalg.eigh(S[p, idx])        # ascending: column 0 is the bearing itself (variance ~ 0)
            u = rng.standard_normal((len(idx), 3))
            u[:, 0] = 0.0
            u /= np.linalg.norm(u, axis=1, keepdims=True)
            v = f2[p, idx] + 8.0 * np.einsum("nij,nj->ni", V, np.sqrt(np.maximum(w, 0.0)) * u)
        f2o[p, idx] = v / np.linalg.norm(v, axis=1, keepdims=True)
    return f2o, out


_gate_cases = {}


def _gate_case(oracle, kind):
    """(pairs, injected [B,N], the oracle chain's result) -- the chain (RANSAC -> weighted -> LS) runs on the CPU"""
    if kind not in _gate_cases:
        g = sim.generate(GATE_B, GATE_N, seed=131)
        f1, f2, S = g.bvs1.numpy(), g.bvs2.numpy(), g.covs2.numpy()
        out = np.zeros((GATE_B, GATE_N), dtype=bool)
        if kind != "clean":
            f2, out = _inject(kind, f2, S, np.random.default_rng(7))
        off = np.arange(GATE_B + 1, dtype=np.int64) * GATE_N
        chain = oracle.solve_chain_batch(off, f1.reshape(-1, 3), f2.reshape(-1, 3), S.reshape(-1, 3, 3), g.init_q.numpy())
        pairs = [Pair(TARGET, f1[p], f2[p], S[p]) for p in range(GATE_B)]
        _gate_cases[kind] = (pairs, out, chain)
    return _gate_cases[kind]


@pytest.mark.parametrize("kind", ["clean", "gross", "mild"])
def test_mask_equals_the_cpu_mask(oracle, kind):
    pairs, _, chain = _gate_case(oracle, kind)
    r_cpu = np.concatenate([pr.oracle_r(oracle, chain["q"][p], chain["t"][p]) for p, pr in enumerate(pairs)])
    with _batch(pairs) as b:
        for gate in (1.0, 2.0, 3.0, 4.0, math.inf):
            rep = b.residuals(chain["q"], chain["t"], gate=gate)
            want = np.abs(r_cpu) <= gate
            close = np.zeros_like(want) if math.isinf(gate) else np.abs(np.abs(r_cpu) - gate) <= 1e-9 * gate
            print(f"{kind} gate {gate}: inside {int(want.sum())} of {want.size}, within 1e-9 of the gate {int(close.sum())}")
            assert close.sum() <= want.size / 10_000
            assert np.array_equal(rep.mask.astype(bool)[~close], want[~close])
            if math.isinf(gate):
                assert rep.mask.all() and np.array_equal(rep.gated_chi2, rep.chi2)
                assert np.array_equal(rep.gated_count, np.full(GATE_B, GATE_N))


def test_gate_at_the_chains_pose_rejects_gross_outliers_and_keeps_the_clean(oracle):
    pairs, injected, chain = _gate_case(oracle, "gross")
    rep = _device(pairs, chain["q"], chain["t"], gate=4.0)
    kept = rep.mask.astype(bool).reshape(GATE_B, GATE_N)
    print(f"gate 4 keeps {kept[injected].mean():.4f} of the gross outliers, {kept[~injected].mean():.4f} of the clean")
    assert kept[injected].mean() < 0.01
    assert kept[~injected].mean() > 0.95


def test_gate_keeps_fewer_mild_outliers_than_the_ransac_mask(oracle):
    pairs, injected, chain = _gate_case(oracle, "mild")
    rep = _device(pairs, chain["q"], chain["t"], gate=4.0)
    kept = rep.mask.astype(bool).reshape(GATE_B, GATE_N)
    ransac = chain["mask"].reshape(GATE_B, GATE_N)
    print(f"mild outliers kept: gate 4 {kept[injected].mean():.4f}, RANSAC {ransac[injected].mean():.4f}")
    assert kept[injected].mean() < ransac[injected].mean()


# ---- 5: layout -----------------------------------------------------------------------------------------------------
PER_CORR = ("residual", "variance", "mask")
PER_SLOT = ("chi2", "gated_chi2", "gated_count", "max_abs")


@pytest.mark.parametrize("mode", FAMILIES, ids=FAMILY_IDS)
def test_three_hypotheses_equal_three_calls_at_the_documented_positions(oracle, mode):
    rng = np.random.default_rng(9)
    sizes = [70, 1, 600, 64, 1300]
    pairs = [_sim_pairs(mode, 1, n, seed=400 + i)[0][0] for i, n in enumerate(sizes)]
    P = len(pairs)
    q = np.stack([_random_quat(rng) for _ in range(3 * P)])
    t = rng.standard_normal((3 * P, 3))
    gate = 1.0 if mode != NEC else 0.3
    with _batch(pairs) as b:
        rep3 = b.residuals(q, t, gate=gate, n_hyp=3)
        singles = [b.residuals(q[h::3], t[h::3], gate=gate) for h in range(3)]
    off = rep3.offsets
    assert len(rep3.residual) == 3 * off[-1]
    for p in range(P):
        n = sizes[p]
        for h in range(3):
            lo = 3 * off[p] + h * n
            for name in PER_CORR:
                assert np.array_equal(getattr(rep3, name)[lo:lo + n], getattr(singles[h], name)[off[p]:off[p + 1]]), (p, h, name)
            for name in PER_SLOT:
                assert getattr(rep3, name)[3 * p + h] == getattr(singles[h], name)[p], (p, h, name)


@pytest.mark.parametrize("mode", FAMILIES, ids=FAMILY_IDS)
def test_a_pairs_outputs_do_not_depend_on_the_batch_around_it(oracle, mode):
    rng = np.random.default_rng(10)
    sizes = [513, 30, 4096, 64, 1500]
    pairs = [_sim_pairs(mode, 1, n, seed=420 + i)[0][0] for i, n in enumerate(sizes)]
    q = np.stack([_random_quat(rng) for _ in sizes])
    t = rng.standard_normal((len(sizes), 3))
    together = _device(pairs, q, t)
    for p, pr in enumerate(pairs):
        alone = _device([pr], q[p], t[p])
        sl = slice(together.offsets[p], together.offsets[p + 1])
        for name in PER_CORR:
            assert np.array_equal(getattr(together, name)[sl], getattr(alone, name)), (p, name)
        for name in PER_SLOT:
            assert getattr(together, name)[p] == getattr(alone, name)[0], (p, name)


def test_host_and_device_space_agree_bit_for_bit(oracle):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(11)
    sizes = [100, 513, 7]
    pairs = [_sim_pairs(TARGET, 1, n, seed=440 + i)[0][0] for i, n in enumerate(sizes)]
    q = np.stack([_random_quat(rng) for _ in range(2 * len(sizes))])
    t = rng.standard_normal((2 * len(sizes), 3))
    with _batch(pairs) as b:
        host = b.residuals(q, t, gate=1.5, n_hyp=2)
        dev = b.residuals(torch.from_numpy(q).cuda(), torch.from_numpy(t).cuda(), gate=1.5, n_hyp=2)
        torch.cuda.synchronize()
    for name in PER_CORR + PER_SLOT:
        d = getattr(dev, name)
        assert d.is_cuda
        assert np.array_equal(d.cpu().numpy(), getattr(host, name)), name
    assert dev.mask.dtype == torch.uint8 and dev.gated_count.dtype == torch.int32


def test_null_outputs_are_skipped_and_nothing_else_is_written(oracle):
    """the raw call, HOST and DEVICE space: sentinel-filled buffers with a guard band on both sides of the documented range"""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(12)
    sizes = [65, 3, 200]
    n_hyp, PAD = 2, 64
    pairs = [_sim_pairs(TARGET, 1, n, seed=460 + i)[0][0] for i, n in enumerate(sizes)]
    S, M = n_hyp * len(sizes), n_hyp * sum(sizes)
    q = np.stack([_random_quat(rng) for _ in range(S)])
    t = rng.standard_normal((S, 3))
    L = capi.lib()
    SENT = -123.5
    kinds = [("residual", np.float64, M), ("variance", np.float64, M), ("mask", np.uint8, M), ("chi2", np.float64, S),
             ("gated_chi2", np.float64, S), ("gated_count", np.int32, S), ("max_abs", np.float64, S)]
    sent = {np.float64: SENT, np.uint8: 77, np.int32: -9}
    with _batch(pairs) as b:
        full = b.residuals(q, t, gate=1.0, n_hyp=n_hyp)
        for skip in ([], ["residual", "mask", "chi2"], ["variance", "gated_chi2", "gated_count", "max_abs"],
                     ["residual", "variance", "mask"]):
            # HOST space: every array sits PAD entries inside a larger sentinel-filled buffer
            bufs = {name: np.full(n + 2 * PAD, sent[dt], dtype=dt) for name, dt, n in kinds}
            ptr = [None if name in skip else bufs[name].ctypes.data + PAD * bufs[name].itemsize for name, _, _ in kinds]
            capi.check(L.pnec_hip_residuals(b._h, q.ctypes.data, t.ctypes.data, n_hyp, REG, 1.0, *ptr, capi.MEM_HOST, None))
            # DEVICE space
            tq, tt = torch.from_numpy(q).cuda(), torch.from_numpy(t).cuda()
            dbufs = {name: torch.from_numpy(np.full(n + 2 * PAD, sent[dt], dtype=dt)).cuda() for name, dt, n in kinds}
            dptr = [None if name in skip else dbufs[name].data_ptr() + PAD * dbufs[name].element_size() for name, _, _ in kinds]
            capi.check(L.pnec_hip_residuals(b._h, tq.data_ptr(), tt.data_ptr(), n_hyp, REG, 1.0, *dptr, capi.MEM_DEVICE,
                                            torch.cuda.current_stream(0).cuda_stream))
            torch.cuda.synchronize()
            for name, dt, n in kinds:
                for got in (bufs[name], dbufs[name].cpu().numpy()):
                    assert np.all(got[:PAD] == sent[dt]), f"{name}: written in front of its first entry"
                    assert np.all(got[PAD + n:] == sent[dt]), f"{name}: written behind its {n} entries"
                    if name in skip:
                        assert np.all(got == sent[dt]), f"{name}: a NULL-ed output was written"
                    else:
                        assert np.array_equal(got[PAD:PAD + n], getattr(full, name)), name


def test_reshaped_capacity_batch(oracle):
    pairs = [_sim_pairs(TARGET, 1, n, seed=480 + i)[0][0] for i, n in enumerate([90, 700, 33])]
    rng = np.random.default_rng(13)
    q = np.stack([_random_quat(rng) for _ in pairs])
    t = rng.standard_normal((3, 3))
    want = _device(pairs, q, t)
    with Batch.with_capacity(TARGET, 8, 4000) as b:
        b.reshape(np.array([0, 10, 20], dtype=np.int64))       # an earlier, different shape
        b.fill(np.tile(pairs[0].f1[:10], (2, 1)), np.tile(pairs[0].f2[:10], (2, 1)), np.tile(pairs[0].c2[:10], (2, 1, 1)))
        b.reshape(want.offsets)
        b.fill(*(np.concatenate([getattr(p, a) for p in pairs]) for a in ("f1", "f2", "c2")))
        got = b.residuals(q, t)
    for name in PER_CORR + PER_SLOT:
        assert np.array_equal(getattr(got, name), getattr(want, name)), name


# ---- 6: composition with select -------------------------------------------------------------------------------------
@pytest.mark.parametrize("view", [False, True], ids=["select", "select_view"])
@pytest.mark.parametrize("space", ["numpy", "torch"])
def test_residuals_of_the_selected_batch_are_the_kept_residuals(oracle, view, space):
    torch = pytest.importorskip("torch")
    sizes = [400, 64, 9, 1000, 513]
    pairs, qs, ts = [], [], []
    for i, n in enumerate(sizes):
        (pr,), g = _sim_pairs(TARGET, 1, n, seed=500 + i)
        pairs.append(pr); qs.append(_gt_quat(oracle, g, 0)); ts.append(g.t_gt[0].numpy())
    q, t = _poses(qs, ts)
    if space == "torch":
        q, t = torch.from_numpy(q).cuda(), torch.from_numpy(t).cuda()
    host = lambda a: a.cpu().numpy() if space == "torch" else a
    with _batch(pairs) as b:
        rep = b.residuals(q, t, gate=1.0)
        sel = b.select(rep.mask, view=view)          # sizes live on the device (lazy) until somebody asks
        rep2 = sel.residuals(q, t, gate=1.0)
        if space == "torch":
            torch.cuda.synchronize()
        keep = host(rep.mask).astype(bool)
        assert 0 < keep.sum() < keep.size
        assert np.array_equal(rep2.offsets, np.concatenate([[0], np.cumsum([keep[rep.offsets[p]:rep.offsets[p + 1]].sum()
                                                                            for p in range(len(sizes))])]))
        assert np.array_equal(host(rep2.residual), host(rep.residual)[keep])
        assert np.array_equal(host(rep2.variance), host(rep.variance)[keep])
        assert host(rep2.mask).all()
        assert np.array_equal(host(rep2.gated_count), host(rep.gated_count))
        assert np.array_equal(host(rep2.max_abs), np.array([np.abs(host(rep.residual)[rep.offsets[p]:rep.offsets[p + 1]][
            keep[rep.offsets[p]:rep.offsets[p + 1]]]).max() for p in range(len(sizes))]))
        sel.close()


# ---- 8: edges -------------------------------------------------------------------------------------------------------
def test_a_pair_without_correspondences(oracle):
    pairs = [_sim_pairs(TARGET, 1, 50, seed=520)[0][0]]
    empty = pairs[0].take(np.zeros(50, dtype=bool))
    q = np.tile([0.0, 0.0, 0.0, 1.0], (3, 1))
    t = np.tile([0.3, -0.2, 0.9], (3, 1))
    rep = _device([pairs[0], empty, pairs[0]], q, t)
    assert np.array_equal(rep.offsets, [0, 50, 50, 100]) and len(rep.residual) == 100
    assert rep.chi2[1] == 0.0 and rep.gated_chi2[1] == 0.0 and rep.gated_count[1] == 0 and rep.max_abs[1] == 0.0
    assert np.array_equal(rep.residual[:50], rep.residual[50:]) and rep.chi2[0] == rep.chi2[2] > 0.0
    assert np.isnan(rep.variance_factor()[1])
    only = _device([empty], q[0], t[0])
    assert len(only.residual) == 0 and only.chi2[0] == 0.0 and only.gated_count[0] == 0 and only.max_abs[0] == 0.0


@pytest.mark.parametrize("mode", FAMILIES, ids=FAMILY_IDS)
def test_a_nan_bearing_marks_its_own_slot_only(oracle, mode):
    rng = np.random.default_rng(14)
    pairs = [_sim_pairs(mode, 1, n, seed=540 + i)[0][0] for i, n in enumerate([100, 700, 100])]
    q = np.stack([_random_quat(rng) for _ in pairs])
    t = rng.standard_normal((3, 3))
    clean = _device(pairs, q, t, gate=math.inf)
    bad = 611
    pairs[1].f2 = pairs[1].f2.copy()
    pairs[1].f2[bad, 1] = np.nan
    rep = _device(pairs, q, t, gate=math.inf)
    lo = rep.offsets[1]
    assert np.isnan(rep.residual[lo + bad]) and rep.mask[lo + bad] == 0
    assert np.isnan(rep.chi2[1]) and np.isnan(rep.max_abs[1]) and np.isfinite(rep.gated_chi2[1])
    assert rep.gated_count[1] == 699
    others = np.ones(len(rep.residual), dtype=bool)
    others[lo + bad] = False
    assert np.array_equal(rep.residual[others], clean.residual[others]) and rep.mask[others].all()
    for p in (0, 2):
        for name in PER_SLOT:
            assert getattr(rep, name)[p] == getattr(clean, name)[p], (p, name)


def test_zero_covariance_without_regularisation_gives_the_documented_value(oracle):
    """variance 0 as summed, r = n / sqrt(1e-300): finite, huge, outside every finite gate -- and no fault"""
    (pr,), g = _sim_pairs(TARGET, 1, 130, seed=560)
    pr.c2 = pr.c2.copy()
    dead = [3, 64, 129]
    pr.c2[dead] = 0.0
    q, t = _gt_quat(oracle, g, 0), g.t_gt[0].numpy()
    rep = _device([pr], q, t, gate=4.0, reg=0.0)
    ref = _device([pr], q, t, gate=4.0, reg=REG)
    R, tn = _quat_to_R(q), t / np.linalg.norm(t)
    n = np.einsum("ni,ni->n", pr.f2, np.cross(tn, pr.f1) @ R)
    live = np.ones(130, dtype=bool)
    live[dead] = False
    assert np.array_equal(rep.variance[dead], np.zeros(3))
    assert np.all(np.isfinite(rep.residual))
    assert np.allclose(rep.residual[dead], n[dead] * 1e150, rtol=1e-9, atol=0.0)
    assert not rep.mask[dead].any() and rep.max_abs[0] == np.abs(rep.residual[dead]).max()
    # the others: reg = 1e-13 against variances of 1e-8 and more moves them in the 5th digit at most
    assert np.allclose(rep.residual[live], ref.residual[live], rtol=1e-4)
    assert rep.gated_count[0] == rep.mask.sum() and _rel(rep.gated_chi2[0], np.sum(rep.residual[rep.mask.astype(bool)] ** 2)) <= SUM_TOL


# ---- 9: facade and pybind module ------------------------------------------------------------------------------------
def _pose44(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def test_pybind_and_facade_equal_the_batch_call(oracle):
    import pnec_amd.pypnec as pypnec
    (pr,), g = _sim_pairs(TARGET, 1, 180, seed=13)
    t0 = g.t_gt[0].numpy()
    # the facade takes a rotation MATRIX and makes its own quaternion of it.  Identity rotation: that quaternion is
    # (0, 0, 0, 1) whatever the conversion, so the facade runs the batch call's very inputs -> the same bits
    qi = np.array([0.0, 0.0, 0.0, 1.0])
    want = _device([pr], qi, t0, gate=2.5)
    got = pypnec.residuals(pr.f1, pr.f2, pr.c2, _pose44(np.eye(3), t0), 1e-13)
    assert got.shape == (180,) and np.array_equal(got, want.residual)
    idx = pypnec.gate_inliers(pr.f1, pr.f2, pr.c2, _pose44(np.eye(3), t0), 2.5, 1e-13)
    assert list(idx) == list(np.flatnonzero(want.mask))
    # a general pose: the quaternion is the conversion's, equal to rounding
    qg = _gt_quat(oracle, g, 0)
    want = _device([pr], qg, t0, gate=2.0)
    got = pypnec.residuals(pr.f1, pr.f2, pr.c2, _pose44(g.R_gt[0].numpy(), t0), 1e-13)
    assert (np.abs(got - want.residual) / np.maximum(1.0, np.abs(want.residual))).max() <= 1e-9
    idx = np.array(pypnec.gate_inliers(pr.f1, pr.f2, pr.c2, _pose44(g.R_gt[0].numpy(), t0), 2.0, 1e-13))
    near = np.abs(np.abs(want.residual) - 2.0) <= 1e-8
    m = np.zeros(180, dtype=bool)
    m[idx] = True
    assert 0 < len(idx) < 180 and np.array_equal(m[~near], want.mask.astype(bool)[~near])


def test_pybind_and_facade_symmetric_overloads_equal_the_batch_call(oracle):
    """covs_host given -> pnec::common::Residuals / GateInliers (bvs_1, bvs_2, covs_1, covs_2, ...): the SYM batch with
    covs as the target (frame 2) and covs_host as the host (frame 1) covariance.  The two covariance sets differ (the
    host set is the target set rolled by one and scaled), so a swap or a call sent to another family shows."""
    import pnec_amd.pypnec as pypnec
    (pr,), g = _sim_pairs(SYM, 1, 180, seed=17)
    t0 = g.t_gt[0].numpy()
    qi = np.array([0.0, 0.0, 0.0, 1.0])
    I44 = _pose44(np.eye(3), t0)
    want = _device([pr], qi, t0, gate=2.5)
    got = pypnec.residuals(pr.f1, pr.f2, pr.c2, I44, 1e-13, covs_host=pr.c1)
    assert got.shape == (180,) and np.array_equal(got, want.residual)         # identity rotation: the same bits
    idx = pypnec.gate_inliers(pr.f1, pr.f2, pr.c2, I44, 2.5, 1e-13, covs_host=pr.c1)
    assert list(idx) == list(np.flatnonzero(want.mask))
    # the checks above can tell the families and the order of the covariances apart
    swapped = Pair.__new__(Pair)
    swapped.__dict__.update(pr.__dict__)
    swapped.c2, swapped.c1 = pr.c1, pr.c2
    target = Pair(TARGET, pr.f1, pr.f2, pr.c2)
    for other in (swapped, target):
        assert not np.array_equal(_device([other], qi, t0).residual, want.residual)
    assert not np.array_equal(pypnec.residuals(pr.f1, pr.f2, pr.c2, I44, 1e-13), got)
    # a general pose: the quaternion is the conversion's, equal to rounding
    qg, Tg = _gt_quat(oracle, g, 0), _pose44(g.R_gt[0].numpy(), t0)
    want = _device([pr], qg, t0, gate=2.0)
    got = pypnec.residuals(pr.f1, pr.f2, pr.c2, Tg, 1e-13, covs_host=pr.c1)
    assert (np.abs(got - want.residual) / np.maximum(1.0, np.abs(want.residual))).max() <= 1e-9
    idx = np.array(pypnec.gate_inliers(pr.f1, pr.f2, pr.c2, Tg, 2.0, 1e-13, covs_host=pr.c1))
    near = np.abs(np.abs(want.residual) - 2.0) <= 1e-8
    m = np.zeros(180, dtype=bool)
    m[idx] = True
    assert 0 < len(idx) < 180 and np.array_equal(m[~near], want.mask.astype(bool)[~near])


def test_demo_prints_the_count_within_three_sigma_and_the_variance_factor():
    import subprocess
    demo = os.path.join(ROOT, "pnec_amd", "pnec_host_demo")
    out = subprocess.run([demo], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    f = dict(kv.split("=") for kv in out.stdout.split())
    assert 0 < int(f["within_3_sigma"]) <= int(f["inliers"]), out.stdout
    vf = float(f["variance_factor"])          # chi2 / (n - 5) of a pair with more than 5 inliers: positive and finite
    assert math.isfinite(vf) and vf > 0.0, out.stdout
