"""The plain references of tests/test_ingest_edges_gpu.py, tested without a GPU.

`payload_np` lays out the SoA payload of a batch (DESIGN.md "Data layout", pnec_internal.hpp, include/pnec_hip.h) in numpy
float64: per pair a block of 6 / 12 / 18 planes of round_up(N_p, 64) doubles, zero padded, blocks in order.  0.5 * (a + b)
is one correctly rounded addition and an exact halving on either side, so the device's planes must have these very bits.

`unscented_hp` is the algorithm of pnec_hip_unscented_transform (common.cc:460-525: five sigma points, weights
kappa / (2 + kappa) and 0.5 / (2 + kappa), lower Cholesky factor of the 2x2 covariance, RotationBetweenPoints' tangent frame
for the omnidirectional model) in Python's `decimal` at 50 digits, rounded once to float64 at the end: the truth the GPU
tests measure the device against.

`ut_classes` are the edge inputs of the GPU test and `e_oracle` the float64 oracle's own worst error on each class against
that truth: per matrix max |X - T| / max |T|.  The GPU test allows the device 16 x max(E_oracle(class), eps).  Measured
here (x86-64, gcc -O2; printed by test_oracle_error_per_input_class):
    E_oracle(corners) = 7.3e-13   E_oracle(scales) = 2.0e-07   E_oracle(correlation) = 3.9e-13
    E_oracle(kappa)   = 3.9e-13   E_oracle(omni)   = 9.0e-11
"""
import decimal
import os
from decimal import Decimal as D

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NUM_PLANES = {0: 6, 1: 12, 2: 12, 3: 18}     # NEC, TARGET, HOST, SYM (pnec_hip_mode)
PINHOLE, OMNI = 1, 0                         # enum CameraModel (common.h:62) as the ABI numbers it
KITTI_K = np.array([[718.856, 0.0, 607.1928], [0.0, 718.856, 185.2157], [0.0, 0.0, 1.0]])
KITTI_SIZE = (1241.0, 376.0)
EPS = float(np.finfo(np.float64).eps)


# ---- the payload --------------------------------------------------------------------------------------------------------
def round_up64(n):
    return (int(n) + 63) // 64 * 64


def block_layout(mode, offsets):
    """(block_offset [P], stride [P], payload_doubles) of a batch created with these offsets"""
    counts = np.diff(np.asarray(offsets, dtype=np.int64))
    stride = np.array([round_up64(n) for n in counts], dtype=np.int64)
    size = NUM_PLANES[int(mode)] * stride
    start = np.concatenate([[0], np.cumsum(size)]).astype(np.int64)
    return start[:-1], stride, int(start[-1])


def sym6(C):
    """[M,3,3] -> [M,6]: the entries (00, 01, 02, 11, 12, 22) of 0.5 * (C + C')"""
    C = np.asarray(C, dtype=np.float64).reshape(-1, 3, 3)
    return np.stack([C[:, 0, 0], 0.5 * (C[:, 0, 1] + C[:, 1, 0]), 0.5 * (C[:, 0, 2] + C[:, 2, 0]),
                     C[:, 1, 1], 0.5 * (C[:, 1, 2] + C[:, 2, 1]), C[:, 2, 2]], -1)


def payload_np(mode, offsets, bvs1, bvs2, covs=None, covs_host=None):
    """The SoA planes of a batch filled from these arrays: bvs [M,3], covs [M,3,3] (any 3x3, the symmetric part is kept);
    `covs` is pnec_hip_problem_fill's single covariance array (planes 6-11), `covs_host` SYM's covs_1 (planes 12-17)."""
    nc = NUM_PLANES[int(mode)]
    offsets = np.asarray(offsets, dtype=np.int64)
    start, stride, total = block_layout(mode, offsets)
    rows = [np.asarray(bvs1, dtype=np.float64).reshape(-1, 3), np.asarray(bvs2, dtype=np.float64).reshape(-1, 3)]
    if nc >= 12:
        rows.append(sym6(covs))
    if nc >= 18:
        rows.append(sym6(covs_host))
    aos = np.concatenate(rows, 1)               # [M, nc]: one row per correspondence, one column per plane
    assert aos.shape == (int(offsets[-1]), nc)
    out = np.zeros(total)
    for p in range(len(offsets) - 1):
        n = int(offsets[p + 1] - offsets[p])
        blk = out[start[p]:start[p] + nc * stride[p]].reshape(nc, stride[p])
        blk[:, :n] = aos[offsets[p]:offsets[p + 1]].T
    return out


def pair_planes(mode, offsets, payload, p):
    """pair p's planes [nc, N_p] and its padding [nc, stride - N_p], read out of a payload"""
    nc = NUM_PLANES[int(mode)]
    start, stride, _ = block_layout(mode, offsets)
    n = int(offsets[p + 1] - offsets[p])
    blk = np.asarray(payload)[start[p]:start[p] + nc * stride[p]].reshape(nc, stride[p])
    return blk[:, :n], blk[:, n:]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- the unscented transform at 50 digits -------------------------------------------------------------------------------
_CTX = decimal.Context(prec=50, traps=[decimal.InvalidOperation, decimal.DivisionByZero, decimal.Overflow])


def unscented_hp(mu, cov, K_inv=None, kappa=1.0, model=PINHOLE):
    """(bearing [3], covariance [3,3]) of one point, float64 roundings of a 50-digit evaluation.  mu [3], cov [3,3]
    (its top-left 2x2 is used for the pinhole model, R' cov R's for the omnidirectional one), K_inv [3,3].  Where the
    algorithm divides by zero or takes the root of a negative number every output is NaN."""
    with decimal.localcontext(_CTX):
        try:
            m = [D(float(x)) for x in np.asarray(mu, dtype=np.float64).reshape(3)]
            C = [[D(float(x)) for x in row] for row in np.asarray(cov, dtype=np.float64).reshape(3, 3)]
            K = [[D(float(x)) for x in row] for row in (np.eye(3) if K_inv is None else np.asarray(K_inv, dtype=np.float64))]
            kap = D(float(kappa))
            zero, one = D(0), D(1)
            dot = lambda a, b: sum((x * y for x, y in zip(a, b)), zero)
            matmul = lambda A, B: [[dot(A[i], [B[k][j] for k in range(3)]) for j in range(3)] for i in range(3)]
            tr = lambda A: [[A[j][i] for j in range(3)] for i in range(3)]
            if model == OMNI:
                nm = dot(m, m).sqrt()
                v = [x / nm for x in m]
                c = [-v[1], v[0], zero]                                   # (0, 0, 1) x v
                Kx = [[zero, -c[2], c[1]], [c[2], zero, -c[0]], [-c[1], c[0], zero]]
                K2, f = matmul(Kx, Kx), one / (one + v[2])
                R = [[(one if i == j else zero) + Kx[i][j] + K2[i][j] * f for j in range(3)] for i in range(3)]
                loc = matmul(tr(R), matmul(C, R))
                a, b, d = loc[0][0], loc[1][0], loc[1][1]
            else:
                a, b, d = C[0][0], C[1][0], C[1][1]
            l00 = a.sqrt()
            l10 = b / l00
            l11 = (d - l10 * l10).sqrt()
            cols = [[l00, l10, zero], [zero, l11, zero]]                  # the columns of the lower factor
            if model == OMNI:
                cols = [[dot(R[i], col) for i in range(3)] for col in cols]
            pts = [m] + [[x + y for x, y in zip(m, col)] for col in cols] + [[x - y for x, y in zip(m, col)] for col in cols]
            w = [kap / (2 + kap)] + [D("0.5") / (2 + kap)] * 4
            tp = []
            for pt in pts:
                t = pt if model == OMNI else [dot(K[i], pt) for i in range(3)]
                n = dot(t, t).sqrt()
                tp.append([x / n for x in t])
            mean = [sum((w[i] * tp[i][k] for i in range(5)), zero) for k in range(3)]
            S = [[sum((w[i] * (tp[i][r] - mean[r]) * (tp[i][c] - mean[c]) for i in range(5)), zero) for c in range(3)]
                 for r in range(3)]
            return np.array([float(x) for x in tp[0]]), np.array([[float(x) for x in row] for row in S])
        except (decimal.InvalidOperation, decimal.DivisionByZero, decimal.Overflow):
            return np.full(3, np.nan), np.full((3, 3), np.nan)


def unscented_hp_many(mu, cov, K_inv, kappa, model):
    out = [unscented_hp(m, c, K_inv, kappa, model) for m, c in zip(mu, cov)]
    return np.array([o[0] for o in out]).reshape(-1, 3), np.array([o[1] for o in out]).reshape(-1, 3, 3)


def oracle_many(oracle, mu, cov, K_inv, kappa, model):
    return np.array([oracle.unscented_transform(m, c, K_inv, kappa, model) for m, c in zip(mu, cov)]).reshape(-1, 3, 3)


def matrix_errors(X, T):
    """per matrix: max |X - T| / max |T|"""
    X, T = np.asarray(X).reshape(-1, 9), np.asarray(T).reshape(-1, 9)
    return np.abs(X - T).max(1) / np.abs(T).max(1)


# ---- the edge inputs of the GPU test ------------------------------------------------------------------------------------
def _cov33(c2):
    return np.pad(np.asarray(c2, dtype=np.float64), ((0, 0), (0, 1), (0, 1)))


def _spd2(rng, n, sigma=0.4):
    A = rng.normal(size=(n, 2, 2)) * sigma
    return A @ np.transpose(A, (0, 2, 1)) + 0.02 * np.eye(2)


def _mid_image(rng, n):
    return np.stack([rng.uniform(50, KITTI_SIZE[0] - 50, n), rng.uniform(20, KITTI_SIZE[1] - 20, n), np.ones(n)], 1)


def rotation_from_z(v):
    """RotationBetweenPoints((0, 0, 1), v) in float64 (only to MAKE omnidirectional covariances: tangent-plane ones
    rotated to the bearing)"""
    c = np.array([-v[1], v[0], 0.0])
    Kx = np.array([[0.0, -c[2], c[1]], [c[2], 0.0, -c[0]], [-c[1], c[0], 0.0]])
    return np.eye(3) + Kx + Kx @ Kx / (1.0 + v[2])


OMNI_VZ = [1.0, 0.0] + [-1.0 + 10.0 ** -k for k in range(1, 7)]
CORRELATION_K = (2, 6, 10)
KAPPAS = (0.0, 0.5, 1.0, 3.0, 1e3)
SCALES = (1e-12, 1e-6, 1.0, 1e4)


def ut_classes():
    """{class: [group]}; a group = dict(mu [n,3], cov [n,3,3], K_inv, kappa, model): the arguments of one call"""
    rng = np.random.default_rng(20260)
    Kinv = np.linalg.inv(KITTI_K)
    g = lambda mu, c, K=Kinv, kappa=1.0, model=PINHOLE: dict(mu=np.ascontiguousarray(mu), cov=np.ascontiguousarray(c),
                                                             K_inv=K, kappa=kappa, model=model)
    out = {}
    w, h = KITTI_SIZE
    spots = np.array([[0, 0, 1], [w, 0, 1], [0, h, 1], [w, h, 1], [KITTI_K[0, 2], KITTI_K[1, 2], 1]], dtype=np.float64)
    out["corners"] = [g(np.repeat(spots, 6, 0), _cov33(_spd2(rng, 30)))]
    base = _spd2(rng, 8)
    out["scales"] = [g(_mid_image(rng, 8), _cov33(base * s)) for s in SCALES]
    groups = []
    for k in CORRELATION_K:
        a, d = rng.uniform(0.05, 4.0, 8), rng.uniform(0.05, 4.0, 8)
        rho = np.where(np.arange(8) % 2 == 0, 1.0, -1.0) * (1.0 - 10.0 ** -k)
        c2 = np.zeros((8, 2, 2))
        c2[:, 0, 0], c2[:, 1, 1] = a, d
        c2[:, 0, 1] = c2[:, 1, 0] = rho * np.sqrt(a * d)
        groups.append(g(_mid_image(rng, 8), _cov33(c2)))
    out["correlation"] = groups
    out["kappa"] = [g(_mid_image(rng, 6), _cov33(_spd2(rng, 6)), kappa=kap) for kap in KAPPAS]
    groups = []
    for norm in (1.0, 800.0):
        mu, cov = [], []
        for vz in OMNI_VZ:
            for az in rng.uniform(0.0, 2 * np.pi, 3):
                s = np.sqrt(max(0.0, 1.0 - vz * vz))
                v = np.array([s * np.cos(az), s * np.sin(az), vz])
                Rb = rotation_from_z(v)
                mu.append(v * norm)
                cov.append(Rb @ (_cov33(_spd2(rng, 1))[0] * (norm / 800.0) ** 2) @ Rb.T)
        groups.append(g(np.array(mu), np.array(cov), K=np.eye(3), model=OMNI))
    out["omni"] = groups
    return out


_cases = {}


def ut_cases(oracle):
    """{class: [case]}, computed once: case = dict(args = the group, bearing_hp, cov_hp = unscented_hp's outputs,
    cov_oracle = the float64 oracle's).  The correlation class keeps only the k for which unscented_hp and the oracle
    both return finite numbers."""
    if not _cases:
        for name, groups in ut_classes().items():
            cases = []
            for grp in groups:
                bv, hp = unscented_hp_many(**grp)
                orc = oracle_many(oracle, **grp)
                if name == "correlation" and not (np.isfinite(hp).all() and np.isfinite(orc).all()):
                    continue
                cases.append(dict(args=grp, bearing_hp=bv, cov_hp=hp, cov_oracle=orc))
            _cases[name] = cases
    return _cases


def e_oracle(oracle):
    """{class: E_oracle(class)}: the float64 oracle's worst matrix error against unscented_hp"""
    return {name: max(float(matrix_errors(c["cov_oracle"], c["cov_hp"]).max()) for c in cases)
            for name, cases in ut_cases(oracle).items()}


# ---- tests --------------------------------------------------------------------------------------------------------------
def _ragged(rng, sizes):
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    M = int(offsets[-1])
    return offsets, rng.normal(size=(M, 3)), rng.normal(size=(M, 3)), rng.normal(size=(M, 3, 3)), rng.normal(size=(M, 3, 3))


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_payload_np_round_trips_a_ragged_batch(mode):
    rng = np.random.default_rng(5)
    sizes = [0, 1, 63, 64, 65, 0, 130]
    offsets, b1, b2, c, ch = _ragged(rng, sizes)
    nc = NUM_PLANES[mode]
    pay = payload_np(mode, offsets, b1, b2, c if nc >= 12 else None, ch if nc >= 18 else None)
    assert pay.shape == (nc * sum(round_up64(n) for n in sizes),) == (block_layout(mode, offsets)[2],)
    used = 0
    for p, n in enumerate(sizes):
        planes, pad = pair_planes(mode, offsets, pay, p)
        rows = slice(offsets[p], offsets[p + 1])
        assert planes.shape == (nc, n) and pad.shape == (nc, round_up64(n) - n)
        assert np.array_equal(bits(pad), np.zeros(pad.shape, dtype=np.uint64))          # +0.0, not -0.0
        assert np.array_equal(planes[0:3].T, b1[rows]) and np.array_equal(planes[3:6].T, b2[rows])
        for first, cov in ((6, c), (12, ch)):
            if nc >= first + 6:
                S = 0.5 * (cov[rows] + np.transpose(cov[rows], (0, 2, 1)))
                want = np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]])
                assert np.array_equal(planes[first:first + 6], want)
        used += planes.size + pad.size
    assert used == pay.size                      # the blocks tile the payload: an empty pair contributes nothing
    if nc >= 12:                                 # the symmetrisation matters on these inputs
        assert not np.array_equal(c, np.transpose(c, (0, 2, 1)))


def test_payload_np_keeps_the_first_covariance_array_for_host_mode_and_both_for_sym():
    rng = np.random.default_rng(6)
    offsets, b1, b2, c, ch = _ragged(rng, [3, 70])
    tgt, host, sym = (payload_np(m, offsets, b1, b2, c, ch if m == 3 else None) for m in (1, 2, 3))
    assert np.array_equal(tgt, host)
    for p in range(2):
        assert np.array_equal(pair_planes(3, offsets, sym, p)[0][:12], pair_planes(1, offsets, tgt, p)[0])
        assert np.array_equal(pair_planes(3, offsets, sym, p)[0][12:], sym6(ch[offsets[p]:offsets[p + 1]]).T)


def test_unscented_hp_agrees_with_the_oracle_and_the_goldens(oracle, golden_dir):
    z = np.load(os.path.join(golden_dir, "math_golden.npz"))
    for pts, covs, want, model, rtol, atol in ((z["ut_points"], z["ut_covs"], z["ut_out"], PINHOLE, 1e-10, 1e-22),
                                               (z["omni_points"], z["omni_covs"], z["omni_out"], OMNI, 1e-9, 1e-20)):
        bv, hp = unscented_hp_many(pts, covs, np.eye(3), 1.0, model)
        # (the tolerances of tests/test_oracle_golden.py, which pins the oracle to the same goldens)
        np.testing.assert_allclose(hp, want, rtol=rtol, atol=atol)
        np.testing.assert_allclose(hp, oracle_many(oracle, pts, covs, np.eye(3), 1.0, model), rtol=rtol, atol=atol)
        np.testing.assert_allclose(bv, pts / np.linalg.norm(pts, axis=1, keepdims=True), rtol=0, atol=2 * EPS)
        assert np.array_equal(hp, np.transpose(hp, (0, 2, 1)))
        err = matrix_errors(oracle_many(oracle, pts, covs, np.eye(3), 1.0, model), hp)
        print(f"oracle vs unscented_hp on the goldens' points (model {model}): worst matrix error {err.max():.2e}")


def test_unscented_hp_is_nan_where_the_algorithm_divides_by_zero():
    cov = np.diag([1e-6, 1e-6, 0.0])
    bv, S = unscented_hp([0.0, 0.0, -1.0], cov, None, 1.0, OMNI)
    assert np.isnan(bv).all() and np.isnan(S).all()
    bv, S = unscented_hp([0.3, 0.1, 1.0], np.diag([1.0, -1.0, 0.0]), None, 1.0, PINHOLE)   # root of a negative number
    assert np.isnan(S).all()


def test_oracle_error_per_input_class(oracle):
    """E_oracle(class) of the GPU test's bounds, measured and printed; each class has a few dozen points, the truth is
    finite on all of them, and the oracle is not wrong by more than rounding amplified by the class's cancellation."""
    classes = ut_cases(oracle)
    E = e_oracle(oracle)
    assert set(E) == {"corners", "scales", "correlation", "kappa", "omni"}
    for name, groups in classes.items():
        n = sum(len(c["cov_hp"]) for c in groups)
        assert 24 <= n <= 64, (name, n)
        for c in groups:
            assert np.isfinite(c["cov_hp"]).all() and np.isfinite(c["bearing_hp"]).all(), name
        print(f"E_oracle({name}) = {E[name]:.2e} over {n} points in {len(groups)} calls")
        assert 0.0 <= E[name] < 1e-5, name
    assert len(classes["correlation"]) >= 2      # (k = 2 and 6 are harmless in float64)
    assert [c["args"]["kappa"] for c in classes["kappa"]] == list(KAPPAS)
