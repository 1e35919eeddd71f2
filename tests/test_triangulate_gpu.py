"""Triangulation at a pose and the cheirality vote (pnec_hip_triangulate).

The yardstick is numpy float64 written here, exact synthetic geometry, or the CPU oracle; never a device result.

Bounds:
* depths and point on exact geometry: relative 1e-13 / sin^2 psi per correspondence.  numpy's closed form on this recipe
  reaches 1.1e-15 / sin^2 psi at worst; the device gets about 100x that for its reciprocal and FMA order.
* parallax against numpy's atan2: absolute 1e-12.
* parallax_mean against the mean of the device's own per-correspondence values: relative 1e-12 (summation order only).
* depth variance against the numpy formula (tests/test_triangulate_cpu.py checks that formula against central
  differences): relative 1e-12 / sin^2 psi.
* sign symmetry and isolation: bitwise.
* oracle tie: absolute 1e-10 on the reprojection score, on correspondences with psi >= 0.01.
"""
import numpy as np
import pytest

from pnec_amd import Batch, capi
from pnec_amd import simulation as sim

pytestmark = pytest.mark.gpu

NEC, TARGET, HOST, SYM = capi.MODE_NEC, capi.MODE_TARGET, capi.MODE_HOST, capi.MODE_SYM
FAMILIES = [NEC, TARGET, HOST, SYM]
FAMILY_IDS = ["NEC", "TARGET", "HOST", "SYM"]
COUNTS = [0, 1, 5, 63, 64, 65, 512, 513, 1100, 4097]
PER_CORR = ("point", "depth1", "depth2", "parallax", "depth1_var", "front")
PER_SLOT = ("n_front", "n_back", "sign", "t", "parallax_mean")


# ---- helpers ------------------------------------------------------------------------------------------------------
def _quat_to_R(q):
    x, y, z, w = np.asarray(q, float) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _quad(S, g):
    return np.einsum("ni,ni->n", g, np.einsum("nij,nj->ni", S, g))


def _spd(rng, n, scale=1e-6):
    A = rng.standard_normal((n, 3, 3))
    return scale * (A @ A.transpose(0, 2, 1) + 0.1 * np.eye(3))


def triangulate_np(f1, f2, q, t):
    """include/pnec_hip.h's midpoint system in numpy: dict of depth1, depth2, point, psi, u, D and the system's terms"""
    R, tn = _quat_to_R(q), np.asarray(t, float) / np.linalg.norm(t)
    u = f2 @ R.T
    a00, a10, a11 = (f1 * f1).sum(1), (f1 * u).sum(1), (u * u).sum(1)
    b0, b1 = f1 @ tn, u @ tn
    D = a00 * a11 - a10 * a10
    with np.errstate(all="ignore"):
        d1, d2 = (a11 * b0 - a10 * b1) / D, (a10 * b0 - a00 * b1) / D
    point = 0.5 * (d1[:, None] * f1 + tn + d2[:, None] * u)
    psi = np.arctan2(np.linalg.norm(np.cross(f1, u), axis=1), a10)
    return dict(depth1=d1, depth2=d2, point=point, psi=psi, u=u, D=D, R=R, t=tn, a00=a00, a10=a10, a11=a11, b0=b0, b1=b1)


def variance_np(mode, f1, f2, c2, c1, q, t):
    """the depth variance of include/pnec_hip.h; c2 = planes 6..11 (TARGET, SYM: frame 2; HOST: frame 1), c1 = SYM's host"""
    if mode == NEC:
        return np.full(len(f1), np.nan)
    s = triangulate_np(f1, f2, q, t)
    u, tn, d1, D = s["u"], s["t"], s["depth1"][:, None], s["D"][:, None]
    a00, a10, a11, b0, b1 = (s[k][:, None] for k in ("a00", "a10", "a11", "b0", "b1"))
    gu = (2 * b0 * u - b1 * f1 - a10 * tn - d1 * (2 * a00 * u - 2 * a10 * f1)) / D
    g1 = (a11 * tn - b1 * u - d1 * (2 * a11 * f1 - 2 * a10 * u)) / D
    w = gu @ s["R"]   # rows R' gu
    if mode == TARGET:
        return _quad(c2, w)
    if mode == HOST:
        return _quad(c2, g1)
    return _quad(c2, w) + _quad(c1, g1)


class Pair:
    def __init__(self, f1, f2, c2=None, c1=None, truth=None):
        self.f1, self.f2, self.c2, self.c1, self.truth = f1, f2, c2, c1, truth
        self.n = len(f1)

    def take(self, keep):
        cut = lambda a: None if a is None else a[keep]
        return Pair(self.f1[keep], self.f2[keep], cut(self.c2), cut(self.c1))


def _exact_pair(rng, n):
    """n correspondences of exact geometry at a random pose: (Pair, q, t); truth = (P, s, psi)"""
    axis, ang = _unit(rng.standard_normal(3)), rng.uniform(0.0, 0.3)
    q = np.concatenate([axis * np.sin(ang / 2), [np.cos(ang / 2)]])
    R, t, s = _quat_to_R(q), _unit(rng.standard_normal(3)), rng.uniform(0.1, 2.0)
    P = np.zeros((0, 3))
    while len(P) < n:
        c = np.column_stack([rng.uniform(-2, 2, 4 * n + 64), rng.uniform(-2, 2, 4 * n + 64), rng.uniform(2, 8, 4 * n + 64)])
        x2 = (c - s * t) @ R                                            # rows R'(P - s t)
        psi = np.arctan2(np.linalg.norm(np.cross(c, c - s * t), axis=1), (c * (c - s * t)).sum(1))
        P = np.concatenate([P, c[(x2[:, 2] > 0.5) & (psi >= 0.02)]])
    P = P[:n]
    f1, f2 = _unit(P), _unit((P - s * t) @ R)
    psi = np.arctan2(np.linalg.norm(np.cross(P, P - s * t), axis=1), (P * (P - s * t)).sum(1))
    return Pair(f1, f2, _spd(rng, n), _spd(rng, n), truth=(P, s, psi)), q, t


def _batch(mode, pairs):
    off = np.concatenate([[0], np.cumsum([p.n for p in pairs])]).astype(np.int64)
    b = Batch(mode, off)
    cat = lambda xs: np.ascontiguousarray(np.concatenate(xs))
    if off[-1] > 0:
        b.fill(cat([p.f1 for p in pairs]), cat([p.f2 for p in pairs]),
               None if mode == NEC else cat([p.c2 for p in pairs]), cat([p.c1 for p in pairs]) if mode == SYM else None)
    return b


def _tri(mode, pairs, q, t, orient=False, n_hyp=1):
    with _batch(mode, pairs) as b:
        return b.triangulate(np.asarray(q, float).reshape(-1, 4), np.asarray(t, float).reshape(-1, 3), n_hyp=n_hyp,
                             orient=orient)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _negated_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a) ^ np.uint64(1 << 63), _bits(b))


@pytest.fixture(scope="module")
def ragged():
    """the ragged batch of exact geometry, shared and left unchanged: (pairs, q [P,4], t [P,3])"""
    rng = np.random.default_rng(2026)
    made = [_exact_pair(rng, n) for n in COUNTS]
    return [m[0] for m in made], np.array([m[1] for m in made]), np.array([m[2] for m in made])


@pytest.fixture(scope="module")
def noisy():
    g = sim.generate(24, 400, seed=131)
    pairs = [Pair(g.bvs1[p].numpy().copy(), g.bvs2[p].numpy().copy(), g.covs2[p].numpy().copy()) for p in range(24)]
    return pairs, g


# ---- exact geometry, all four families ----------------------------------------------------------------------------
@pytest.mark.parametrize("mode", FAMILIES, ids=FAMILY_IDS)
def test_exact_geometry_depths_points_parallax_and_vote(ragged, mode):
    pairs, q, t = ragged
    r = _tri(mode, pairs, q, t)
    off = np.asarray(r.offsets)
    assert off[-1] == sum(COUNTS) and len(r.depth1) == off[-1] and r.point.shape == (off[-1], 3)
    worst = dict(depth1=0.0, depth2=0.0, point=0.0, parallax=0.0, mean=0.0)
    for p, pr in enumerate(pairs):
        P, s, psi = pr.truth
        sl = slice(off[p], off[p + 1])
        assert r.n_front[p] == pr.n and r.n_back[p] == 0 and r.sign[p] == 1
        assert np.allclose(r.t[p], t[p], rtol=0, atol=1e-15)
        if pr.n == 0:
            assert r.parallax_mean[p] == 0.0
            continue
        s2 = np.sin(psi) ** 2
        assert np.all(r.front[sl] == 1)
        e1 = np.abs(r.depth1[sl] - np.linalg.norm(P, axis=1) / s) / (np.linalg.norm(P, axis=1) / s)
        e2 = np.abs(r.depth2[sl] - np.linalg.norm(P - s * t[p], axis=1) / s) / (np.linalg.norm(P - s * t[p], axis=1) / s)
        ep = np.linalg.norm(r.point[sl] - P / s, axis=1) / np.linalg.norm(P / s, axis=1)
        ea = np.abs(r.parallax[sl] - psi)
        mean = float(np.mean(r.parallax[sl]))
        em = abs(r.parallax_mean[p] - mean) / mean
        for k, e in (("depth1", (e1 * s2).max()), ("depth2", (e2 * s2).max()), ("point", (ep * s2).max()),
                     ("parallax", ea.max()), ("mean", em)):
            worst[k] = max(worst[k], float(e))
        assert np.all(e1 * s2 <= 1e-13) and np.all(e2 * s2 <= 1e-13) and np.all(ep * s2 <= 1e-13), (p, worst)
        assert ea.max() <= 1e-12 and em <= 1e-12, (p, worst)
    print(FAMILY_IDS[mode], "worst err * sin^2 psi and parallax errors:", worst)


@pytest.mark.parametrize("mode", FAMILIES, ids=FAMILY_IDS)
def test_depth_variance_against_the_numpy_formula(ragged, mode):
    pairs, q, t = ragged
    r = _tri(mode, pairs, q, t)
    off = np.asarray(r.offsets)
    if mode == NEC:
        assert np.all(np.isnan(r.depth1_var))
        return
    worst = 0.0
    for p, pr in enumerate(pairs):
        if pr.n == 0:
            continue
        want = variance_np(mode, pr.f1, pr.f2, pr.c2, pr.c1, q[p], t[p])
        got = r.depth1_var[off[p]:off[p + 1]]
        e = np.abs(got - want) / want * np.sin(pr.truth[2]) ** 2
        worst = max(worst, float(e.max()))
        assert np.all(want > 0) and np.all(e <= 1e-12), (p, worst)
    print(FAMILY_IDS[mode], "worst variance err * sin^2 psi:", worst)


# ---- sign symmetry ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [TARGET, SYM], ids=["TARGET", "SYM"])
def test_sign_symmetry_is_bitwise(ragged, mode):
    pairs, q, t = ragged
    a, b = _tri(mode, pairs, q, t), _tri(mode, pairs, q, -t)
    for k in ("depth1", "depth2", "point"):
        assert _negated_bits(getattr(a, k), getattr(b, k)), k
    assert _same_bits(a.depth1_var, b.depth1_var) and _same_bits(a.parallax, b.parallax)
    assert np.array_equal(a.n_front, b.n_back) and np.array_equal(a.n_back, b.n_front)
    live = np.array(COUNTS) > 0
    assert np.all(a.sign[live] == 1) and np.all(b.sign[live] == -1) and np.all(b.front == 0)
    assert np.all(a.sign[~live] == 1) and np.all(b.sign[~live] == 1)     # an empty pair: a tie, +1 both ways
    assert _same_bits(a.t[live], b.t[live]) and _negated_bits(a.t[~live], b.t[~live])
    ao, bo = _tri(mode, pairs, q, t, orient=True), _tri(mode, pairs, q, -t, orient=True)
    sl = np.ones(len(ao.depth1), dtype=bool)
    for k in PER_CORR:
        assert _same_bits(getattr(ao, k)[sl], getattr(bo, k)[sl]), k
        assert _same_bits(getattr(ao, k), getattr(a, k)), k      # at +t the flag changes nothing
    assert np.array_equal(bo.n_front, b.n_front) and np.array_equal(bo.n_back, b.n_back) and np.array_equal(bo.sign, b.sign)
    assert np.all(bo.front == 1)


# ---- oracle tie and the vote on noisy data ---------------------------------------------------------------------------
def test_points_reproduce_the_oracles_reprojection_score(noisy, oracle):
    pairs, g = noisy
    q = np.array([oracle.quat_from_rot(g.R_gt[p].numpy()) for p in range(24)])
    t = g.t_gt.numpy()
    r = _tri(TARGET, pairs, q, t)
    worst, used = 0.0, 0
    for p, pr in enumerate(pairs):
        R, tn = _quat_to_R(q[p]), t[p] / np.linalg.norm(t[p])
        pts = r.point[400 * p:400 * (p + 1)]
        p2 = (pts - tn) @ R
        score = (1 - (pr.f1 * pts).sum(1) / np.linalg.norm(pts, axis=1)) + (1 - (pr.f2 * p2).sum(1) / np.linalg.norm(p2, axis=1))
        psi = triangulate_np(pr.f1, pr.f2, q[p], t[p])["psi"]
        for i in np.flatnonzero(psi >= 0.01):
            want = oracle.reprojection_score(pr.f1[i], pr.f2[i], R, tn)
            worst = max(worst, abs(score[i] - want))
            used += 1
    print("worst score difference", worst, "over", used)
    assert used > 0.9 * 24 * 400 and worst <= 1e-10


def _vote_np(pr, q, t):
    s = triangulate_np(pr.f1, pr.f2, q, t)
    d1, d2 = s["depth1"], s["depth2"]
    # a depth within relative 1e-9 of zero (relative to the terms its numerator cancels)
    n1 = np.abs(s["a11"] * s["b0"] - s["a10"] * s["b1"]) <= 1e-9 * (np.abs(s["a11"] * s["b0"]) + np.abs(s["a10"] * s["b1"]))
    n2 = np.abs(s["a10"] * s["b0"] - s["a00"] * s["b1"]) <= 1e-9 * (np.abs(s["a10"] * s["b0"]) + np.abs(s["a00"] * s["b1"]))
    return int(np.sum((d1 > 0) & (d2 > 0))), int(np.sum((d1 < 0) & (d2 < 0))), int(np.sum(n1 | n2))


def test_vote_at_ground_truth_and_after_a_solve_from_the_wrong_sign(noisy, oracle):
    pairs, g = noisy
    t_gt = g.t_gt.numpy()
    assert np.all(np.linalg.norm(t_gt, axis=1) >= 0.12)
    q = np.array([oracle.quat_from_rot(g.R_gt[p].numpy()) for p in range(24)])
    r = _tri(TARGET, pairs, q, t_gt)
    for p, pr in enumerate(pairs):
        nf, nb, _ = _vote_np(pr, q[p], t_gt[p])
        assert nf >= 0.9975 * 400 and nb == 0                         # numpy alone
        assert r.n_front[p] >= 0.99 * 400 and r.n_back[p] == 0 and r.sign[p] == 1
    # the LM refinement keeps the sign of its start: start it from -t
    with _batch(TARGET, pairs) as b:
        res = b.solve(g.init_q.numpy(), -g.init_t.numpy())
        tri = res.triangulate()
        left_out = 0
        for p, pr in enumerate(pairs):
            nf, nb, near = _vote_np(pr, res.q[p], res.t[p])
            left_out += near
            assert abs(int(tri.n_front[p]) - nf) <= near and abs(int(tri.n_back[p]) - nb) <= near, (p, nf, nb, near)
            if abs(nf - nb) > 2 * near:
                assert tri.sign[p] == (1 if nf >= nb else -1)
            assert tri.t[p] @ t_gt[p] > 0.0, p                        # within 90 degrees of the truth
            assert np.allclose(tri.t[p], tri.sign[p] * res.t[p] / np.linalg.norm(res.t[p]), rtol=0, atol=1e-15)
            assert tri.front[400 * p:400 * (p + 1)].sum() == max(tri.n_front[p], tri.n_back[p])
        assert left_out <= 24 * 400 / 10000


# ---- isolation ----------------------------------------------------------------------------------------------------
def test_a_pair_alone_has_the_bits_it_has_in_the_batch(ragged):
    pairs, q, t = ragged
    for orient in (False, True):
        whole = _tri(SYM, pairs, q, t, orient=orient)
        off = np.asarray(whole.offsets)
        for p in (1, 5, 8, 9):
            alone = _tri(SYM, [pairs[p]], q[p], t[p], orient=orient)
            for k in PER_CORR:
                assert _same_bits(getattr(alone, k), getattr(whole, k)[off[p]:off[p + 1]]), (p, k)
            for k in PER_SLOT:
                assert _same_bits(getattr(alone, k)[0], getattr(whole, k)[p]), (p, k)


def test_three_hypotheses_equal_three_calls(ragged):
    pairs, q, t = ragged
    rng = np.random.default_rng(3)
    qs = np.stack([q, q[::-1], q], 1)                                  # [P,3,4]: slot = pair * 3 + h
    ts = np.stack([t, -t, _unit(rng.standard_normal(t.shape))], 1)
    all3 = _tri(TARGET, pairs, qs.reshape(-1, 4), ts.reshape(-1, 3), orient=True, n_hyp=3)
    off = np.asarray(all3.offsets)
    assert len(all3.depth1) == 3 * off[-1] and len(all3.sign) == 3 * len(pairs)
    for h in range(3):
        one = _tri(TARGET, pairs, qs[:, h], ts[:, h], orient=True)
        for p, pr in enumerate(pairs):
            at = 3 * off[p] + h * pr.n
            for k in PER_CORR:
                assert _same_bits(getattr(all3, k)[at:at + pr.n], getattr(one, k)[off[p]:off[p + 1]]), (h, p, k)
            for k in PER_SLOT:
                assert _same_bits(getattr(all3, k)[3 * p + h], getattr(one, k)[p]), (h, p, k)


def test_host_space_equals_device_space(ragged):
    import torch
    pairs, q, t = ragged
    with _batch(SYM, pairs) as b:
        host = b.triangulate(q, t, orient=True)
        dev = b.triangulate(torch.as_tensor(q, device="cuda:0"), torch.as_tensor(t, device="cuda:0"), orient=True)
        torch.cuda.synchronize()
        for k in PER_CORR + PER_SLOT:
            assert getattr(dev, k).is_cuda
            assert _same_bits(getattr(dev, k).cpu().numpy(), getattr(host, k)), k


def test_a_select_view_batch_writes_at_its_own_offsets(ragged):
    pairs, q, t = ragged
    rng = np.random.default_rng(5)
    masks = [rng.random(pr.n) < 0.6 for pr in pairs]
    with _batch(TARGET, pairs) as b:
        view = b.select(np.concatenate(masks).astype(np.uint8), view=True)
        got = view.triangulate(q, t, orient=True)
        off = np.asarray(got.offsets)
        assert np.array_equal(np.diff(off), [m.sum() for m in masks]) and len(got.depth1) == off[-1]
    want = _tri(TARGET, [pr.take(m) for pr, m in zip(pairs, masks)], q, t, orient=True)
    for k in PER_CORR + PER_SLOT:
        assert _same_bits(getattr(got, k), getattr(want, k)), k


# ---- degenerates ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [NEC, TARGET], ids=["NEC", "TARGET"])
def test_parallel_zero_and_nan_correspondences(ragged, mode):
    pairs, q, t = ragged
    pr, qp, tp = pairs[5], q[5], t[5]                                  # the pair of 65
    PAR, ZERO, NAN = 10, 31, 64
    f1, f2 = pr.f1.copy(), pr.f2.copy()
    f2[PAR] = _quat_to_R(qp).T @ f1[PAR]
    f1[ZERO] = 0.0
    f2[NAN, 1] = np.nan
    bad = Pair(f1, f2, pr.c2, pr.c1)
    rest = np.ones(65, dtype=bool)
    rest[[PAR, ZERO, NAN]] = False
    for orient in (False, True):
        r = _tri(mode, [bad], qp, tp, orient=orient)
        clean = _tri(mode, [pr.take(rest)], qp, tp, orient=orient)
        for k in PER_CORR:
            assert _same_bits(getattr(r, k)[rest], getattr(clean, k)), k
        assert r.n_front[0] == 62 == clean.n_front[0] and r.n_back[0] == 0 and r.sign[0] == 1
        for i in (PAR, ZERO):
            assert r.depth1[i] == np.inf and r.depth2[i] == np.inf and np.all(np.isnan(r.point[i]))
            assert np.isnan(r.depth1_var[i]) and r.front[i] == 0
        assert r.parallax[ZERO] == 0.0 and 0.0 <= r.parallax[PAR] <= 1e-7
        for k in ("depth1", "depth2", "parallax", "depth1_var"):
            assert np.isnan(getattr(r, k)[NAN]), k
        assert np.all(np.isnan(r.point[NAN])) and r.front[NAN] == 0
        keep = np.ones(65, dtype=bool)
        keep[NAN] = False
        mean = float(np.mean(r.parallax[keep]))
        assert abs(r.parallax_mean[0] - mean) <= 1e-12 * mean


# ---- facade -----------------------------------------------------------------------------------------------------
def _pose44(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def test_pybind_and_facade(ragged):
    import pnec_amd.pypnec as pypnec
    pairs, q, t = ragged
    pr = pairs[6]
    # the facade makes its own quaternion of the rotation matrix; of the identity that is (0, 0, 0, 1) whatever the
    # conversion, so the facade runs the batch call's very inputs
    qi = np.array([0.0, 0.0, 0.0, 1.0])
    want = _tri(NEC, [pr], qi, t[6], orient=False)
    pts, d1, d2, front = pypnec.triangulate(pr.f1, pr.f2, _pose44(np.eye(3), t[6]))
    assert pts.shape == (512, 3) and front.dtype == np.uint8
    assert _same_bits(pts, want.point) and _same_bits(d1, want.depth1) and _same_bits(d2, want.depth2)
    assert np.array_equal(front, want.front)
    # a pose whose translation was negated and scaled by 0.7 comes back with the same rotation and +0.7 t
    R = _quat_to_R(q[6])
    T = pypnec.orient_translation(pr.f1, pr.f2, _pose44(R, -0.7 * t[6]))
    assert np.array_equal(T[:3, 3], 0.7 * t[6]) and np.allclose(T[:3, :3], R, rtol=0, atol=1e-14)   # (through the facade's own quaternion)
    assert np.array_equal(T[3], [0, 0, 0, 1])
    T = pypnec.orient_translation(pr.f1, pr.f2, _pose44(R, 0.7 * t[6]))
    assert np.array_equal(T[:3, 3], 0.7 * t[6])
