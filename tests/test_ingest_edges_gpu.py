"""The batch layer's utility kernels (pnec_amd/csrc/pnec_batch_kernels.hip) at their edges, each against a plain reference
that never saw a device: pack_kernel and ingest_keypoints_kernel against `payload_np` bit for bit (every mode, both memory
spaces, ragged sizes through the second trip of either grid-stride loop, partial fills), unscented_kernel against the
50-digit `unscented_hp`, cost_function_kernel against the oracle and numpy longdouble, select_best_kernel against its
contract in numpy, mask_count_kernel + InlierExtraction against numpy's count and `payload_np` of the kept rows.
The references live in tests/test_ingest_reference_cpu.py, which tests them without a GPU.

The unscented transform's bound is derived, not chosen: per input class the device's worst error against unscented_hp (per
matrix, max |X - T| / max |T|) may be 16 x max(E_oracle(class), eps), E_oracle being the float64 oracle's own worst error
on the class.  16 covers another, equally valid order of operations (fast_rsqrt's refinement included).  E_oracle and the
bound as measured with the oracle built by gcc -O2 on x86-64; the test prints them beside the device's error and the
bearing's worst distance in ulps (test_unscented_transform_at_the_edges_against_50_digits, run with -s).  The device's
column is not recorded yet: a float64 emulation of the kernel's operation order in numpy gives 8.0e-13, 2.0e-07,
3.9e-13, 3.9e-13 and 9.0e-11, which is NOT a measurement on an MI355X.
    class         E_oracle   bound = 16 x max(E_oracle, eps)
    corners       7.3e-13    1.2e-11
    scales        2.0e-07    3.1e-06
    correlation   3.9e-13    6.3e-12
    kappa         3.9e-13    6.2e-12
    omni          9.0e-11    1.4e-09
(scales: sigma points 1e-6 px apart move the bearing by 1e-9, and the covariance is made of differences of unit vectors;
omni: 1 / (1 + vz) at vz = -1 + 1e-6 amplifies the rounding of vz a million times.  Both are the algorithm's, in any
float64 implementation.)

A batch made by InlierExtraction keeps its source's block layout (DESIGN.md "Data layout"): pair p's planes start where the
source's did, with the stride of the kept count; what lies between a shrunken block's end and the next block is capacity
and is not compared.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_ingest_reference_cpu import (EPS, KITTI_K, KITTI_SIZE, NUM_PLANES, OMNI, PINHOLE, bits, block_layout,  # noqa: E402
                                       e_oracle, matrix_errors, payload_np, round_up64, ut_cases)

from pnec_amd import Batch, capi, frontend, select_best  # noqa: E402

pytestmark = pytest.mark.gpu

MODES = [capi.MODE_NEC, capi.MODE_TARGET, capi.MODE_HOST, capi.MODE_SYM]
SPACES = ["numpy", "torch"]
SIZES = [0, 1, 63, 64, 65, 0, 513, 16385]          # 16 385: one past 64 blocks x 256 threads (the x-loop's second trip)
SPLITS = [(0, 3), (3, 3), (5, 1), (6, 2), (7, 1)]  # (first_pair, n_pairs); (5, 1) is an empty pair
KINV = np.linalg.inv(KITTI_K)


def _offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def _c9(c):
    """[M,3,3] -> [M,9] column-major, what pnec_hip_problem_fill reads"""
    return None if c is None else np.ascontiguousarray(np.transpose(c, (0, 2, 1)).reshape(-1, 9))


def _to(space, a):
    if a is None or space == "numpy":
        return a
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _covs_for(mode, c, ch):
    nc = NUM_PLANES[mode]
    return (c if nc >= 12 else None), (ch if nc >= 18 else None)


def _fill(batch, mode, space, b1, b2, c, ch, **kw):
    c, ch = _covs_for(mode, c, ch)
    batch.fill(_to(space, b1), _to(space, b2), _to(space, _c9(c)), _to(space, _c9(ch)), **kw)


def _fill_keypoints(batch, mode, space, p1, p2, c2, c1, **kw):
    c2, c1 = _covs_for(mode, c2, c1)
    batch.fill_keypoints(_to(space, p1), _to(space, p2), _to(space, c2), _to(space, c1), K_inv=KINV, **kw)


def _assert_same_bits(got, want, what=""):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(bits(got) != bits(want))
    assert bad.size == 0, f"{what}: {bad.size} doubles differ, first at {bad[:5]}: {got[bad[:5]]} != {want[bad[:5]]}"


class _Data:
    """random bearings and NON-symmetric 3x3 'covariances' (so that 0.5 * (C + C') matters), different in covs and
    covs_host; keypoints with 2x2 image covariances; a sentinel of recognisable constants"""

    def __init__(self, sizes, seed):
        rng = np.random.default_rng(seed)
        self.offsets = _offsets(sizes)
        M = self.M = int(self.offsets[-1])
        self.b1, self.b2 = rng.normal(size=(M, 3)), rng.normal(size=(M, 3))
        self.c, self.ch = rng.normal(size=(M, 3, 3)), rng.normal(size=(M, 3, 3))
        self.p1 = np.stack([rng.uniform(0, KITTI_SIZE[0], M), rng.uniform(0, KITTI_SIZE[1], M)], 1)
        self.p2 = self.p1 + rng.normal(size=(M, 2)) * 5
        A, B = rng.normal(size=(M, 2, 2)) * 0.4, rng.normal(size=(M, 2, 2)) * 0.4
        self.k2 = A @ np.transpose(A, (0, 2, 1)) + 0.02 * np.eye(2)
        self.k1 = B @ np.transpose(B, (0, 2, 1)) + 0.02 * np.eye(2)
        self.sentinel = (np.full((M, 3), 7.25), np.full((M, 3), -7.25), np.full((M, 3, 3), -3.5), np.full((M, 3, 3), 1.75))

    def rows(self, first, n):
        return slice(int(self.offsets[first]), int(self.offsets[first + n]))

    def unscented(self, rows=slice(None)):
        """the two-step path's first step on the device: (b1, b2, S2, S1) of the keypoints"""
        mu = lambda p: np.concatenate([p, np.ones((len(p), 1))], 1)
        c33 = lambda c: np.pad(c, ((0, 0), (0, 1), (0, 1)))
        b2, S2 = frontend.unscented_transform(mu(self.p2[rows]), c33(self.k2[rows]), KINV, 1.0, PINHOLE)
        b1, S1 = frontend.unscented_transform(mu(self.p1[rows]), c33(self.k1[rows]), KINV, 1.0, PINHOLE)
        return b1, b2, S2, S1


@pytest.fixture(scope="module")
def data():
    return _Data(SIZES, 41)


def _dirty(mode, offsets):
    """leave recognisable non-zero doubles where the next batch of this size will have its padding lanes (the library's
    buffer cache hands the block out again): a batch of the same payload size whose pairs have no padding"""
    sizes = [round_up64(n) for n in np.diff(offsets)]
    M = sum(sizes)
    with Batch(mode, _offsets(sizes)) as b:
        c, ch = _covs_for(mode, np.full((M, 9), 3.25), np.full((M, 9), 4.25))
        b.fill(np.full((M, 3), 5.25), np.full((M, 3), 6.25), c, ch)


# ---- a. pack against numpy, bit for bit ---------------------------------------------------------------------------------
@pytest.mark.parametrize("space", SPACES)
@pytest.mark.parametrize("mode", MODES)
def test_pack_is_bitwise_the_documented_layout(data, mode, space):
    d = data
    want = payload_np(mode, d.offsets, d.b1, d.b2, *_covs_for(mode, d.c, d.ch))
    _dirty(mode, d.offsets)
    with Batch(mode, d.offsets) as b:
        _fill(b, mode, space, d.b1, d.b2, d.c, d.ch)
        got = b.export_payload()
        assert b.num_correspondences == d.M and b.max_correspondences == max(SIZES)
    assert got.size == want.size == NUM_PLANES[mode] * sum(round_up64(n) for n in SIZES)
    _assert_same_bits(got, want, "pack_kernel")      # (padding lanes +0.0 included: -0.0 has another bit pattern)


# ---- b. partial fills ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("space", SPACES)
@pytest.mark.parametrize("mode", MODES)
def test_partial_fill_writes_its_pair_range_and_nothing_else(data, mode, space):
    d = data
    start, _, total = block_layout(mode, d.offsets)
    edges = np.concatenate([start, [total]])
    sentinel = payload_np(mode, d.offsets, *d.sentinel[:2], *_covs_for(mode, *d.sentinel[2:]))
    fresh = payload_np(mode, d.offsets, d.b1, d.b2, *_covs_for(mode, d.c, d.ch))
    with Batch(mode, d.offsets) as b:
        for first, n in SPLITS:
            _fill(b, mode, space, *d.sentinel)
            _assert_same_bits(b.export_payload(), sentinel, "sentinel fill")
            r = d.rows(first, n)
            _fill(b, mode, space, d.b1[r], d.b2[r], d.c[r], d.ch[r], first_pair=first, n_pairs=n)
            want = sentinel.copy()
            want[edges[first]:edges[first + n]] = fresh[edges[first]:edges[first + n]]
            _assert_same_bits(b.export_payload(), want, f"fill of pairs [{first}, {first + n})")


@pytest.mark.parametrize("space", SPACES)
@pytest.mark.parametrize("mode", MODES)
def test_partial_keypoint_fill_is_bitwise_unscented_transform_plus_fill_on_the_range(data, mode, space):
    d = data
    start, _, total = block_layout(mode, d.offsets)
    edges = np.concatenate([start, [total]])
    sentinel = payload_np(mode, d.offsets, *d.sentinel[:2], *_covs_for(mode, *d.sentinel[2:]))
    with Batch(mode, d.offsets) as fused, Batch(mode, d.offsets) as two_step:
        for first, n in SPLITS:
            r = d.rows(first, n)
            for b in (fused, two_step):
                _fill(b, mode, space, *d.sentinel)
            _fill_keypoints(fused, mode, space, d.p1[r], d.p2[r], d.k2[r], d.k1[r], first_pair=first, n_pairs=n)
            b1, b2, S2, S1 = d.unscented(r)
            _fill(two_step, mode, space, b1, b2, S2, S1, first_pair=first, n_pairs=n)
            got, want = fused.export_payload(), two_step.export_payload()
            _assert_same_bits(got, want, f"fill_keypoints of pairs [{first}, {first + n})")
            outside = np.ones(total, dtype=bool)
            outside[edges[first]:edges[first + n]] = False
            _assert_same_bits(got[outside], sentinel[outside], "outside the range")
            if n > 0 and r.stop > r.start:     # the range itself is the unscented transform's output in the plain layout
                sub = _offsets(np.diff(d.offsets[first:first + n + 1]))
                _assert_same_bits(got[edges[first]:edges[first + n]],
                                  payload_np(mode, sub, b1, b2, *_covs_for(mode, S2, S1)), "inside the range")


# ---- c. more than 32 768 pairs: the y-loop's second trip ----------------------------------------------------------------
@pytest.fixture(scope="module")
def many_pairs():
    sizes = np.tile([1, 0, 0, 2, 0, 65, 0, 0], 4097)[:32770].copy()
    sizes[0], sizes[32768], sizes[32769] = 1, 3, 2       # first trip's pair 0 and second trip's pair 0: sizes differ
    return _Data(sizes, 43)


def test_fill_of_more_than_32768_pairs(many_pairs):
    d = many_pairs
    assert len(d.offsets) - 1 == 32770
    want = payload_np(capi.MODE_NEC, d.offsets, d.b1, d.b2)
    assert want.size * 8 < 64 << 20
    for space in SPACES:
        with Batch(capi.MODE_NEC, d.offsets) as b:
            _fill(b, capi.MODE_NEC, space, *d.sentinel)
            _fill(b, capi.MODE_NEC, space, d.b1, d.b2, None, None)
            _assert_same_bits(b.export_payload(), want, f"pack_kernel, 32 770 pairs, {space}")


def test_keypoint_fill_of_more_than_32768_pairs(many_pairs):
    d = many_pairs
    b1, b2, _, _ = d.unscented()
    want = payload_np(capi.MODE_NEC, d.offsets, b1, b2)
    for space in SPACES:
        with Batch(capi.MODE_NEC, d.offsets) as b:
            _fill(b, capi.MODE_NEC, space, *d.sentinel)
            _fill_keypoints(b, capi.MODE_NEC, space, d.p1, d.p2, None, None)
            _assert_same_bits(b.export_payload(), want, f"ingest_keypoints_kernel, 32 770 pairs, {space}")


# ---- d. the unscented transform at the edges ----------------------------------------------------------------------------
def _device_ut(args):
    return frontend.unscented_transform(args["mu"], args["cov"], args["K_inv"], args["kappa"], args["model"])


def _bearing_ulps(args, bearing, bearing_hp):
    """|bearing - truth| in ulps.  A component of K_inv mu is a sum of three products; where they cancel (the principal
    point) its float64 value cannot be good to ulps of the SUM, only of the terms: the ulp is that of
    max(|b_k|, sum_j |K_inv[k, j] mu_j| / |K_inv mu|).  For the omnidirectional model (no K_inv) it is the component's own."""
    mu = args["mu"]
    if args["model"] == PINHOLE:
        terms = np.abs(mu) @ np.abs(args["K_inv"]).T
        norm = np.linalg.norm(mu @ args["K_inv"].T, axis=1, keepdims=True)
    else:
        terms, norm = np.abs(mu), np.linalg.norm(mu, axis=1, keepdims=True)
    unit = np.spacing(np.maximum(np.abs(bearing_hp), terms / norm))
    return np.abs(bearing - bearing_hp) / unit


def test_unscented_transform_at_the_edges_against_50_digits(oracle):
    E = e_oracle(oracle)
    failures = []
    for name, cases in ut_cases(oracle).items():
        dev_err, ulps = 0.0, 0.0
        for case in cases:
            bearing, S = _device_ut(case["args"])
            assert np.isfinite(S).all() and np.isfinite(bearing).all(), name
            assert np.array_equal(bits(S), bits(np.transpose(S, (0, 2, 1)))), f"{name}: an output matrix is not symmetric"
            dev_err = max(dev_err, float(matrix_errors(S, case["cov_hp"]).max()))
            ulps = max(ulps, float(_bearing_ulps(case["args"], bearing, case["bearing_hp"]).max()))
        bound = 16.0 * max(E[name], EPS)
        print(f"{name:12s} E_oracle {E[name]:.2e}   device {dev_err:.2e}   bound {bound:.2e}   bearing {ulps:.2f} ulp")
        if not dev_err <= bound:
            failures.append(f"{name}: device error {dev_err:.3e} > 16 x max(E_oracle, eps) = {bound:.3e}")
        if not ulps <= 4.0:
            failures.append(f"{name}: bearing off by {ulps:.2f} ulp > 4")
    assert not failures, failures


def test_unscented_transform_at_the_antipode_returns_and_leaves_its_neighbours_alone():
    """exactly at vz = -1 the algorithm divides by zero (1 / (1 + vz)): the call returns, the rows around are unaffected"""
    cov = np.diag([1e-6, 1e-6, 0.0])
    good = np.array([[0.6, 0.0, 0.8], [0.0, 480.0, 640.0], [0.0, -0.8, -0.6]])
    mu = np.array([good[0], [0.0, 0.0, -1.0], good[1], [0.0, 0.0, -800.0], good[2]])
    covs = np.array([cov, cov, cov * 800.0 ** 2, cov * 800.0 ** 2, cov])
    bearing, S = frontend.unscented_transform(mu, covs, np.eye(3), 1.0, OMNI)
    alone_b, alone_S = frontend.unscented_transform(mu[[0, 2, 4]], covs[[0, 2, 4]], np.eye(3), 1.0, OMNI)
    assert np.array_equal(bits(bearing[[0, 2, 4]]), bits(alone_b)) and np.array_equal(bits(S[[0, 2, 4]]), bits(alone_S))
    assert np.isfinite(alone_S).all() and np.abs(alone_S).max() > 0


# ---- e. cost_function ----------------------------------------------------------------------------------------------------
COST_SIZES = [1, 63, 64, 65, 0, 129, 700]


def _quat_to_R(q, dtype=np.float64):
    x, y, z, w = np.asarray(q, dtype=dtype) / np.sqrt((np.asarray(q, dtype=dtype) ** 2).sum())
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]], dtype=dtype)


def _cost_longdouble(f1, f2, cov, q, t):
    """include/pnec_hip.h: mean of n^2 / (g' Sigma g), n = t . (f1 x R f2), g = R' (t x f1), in numpy longdouble"""
    ld = np.longdouble
    f1, f2, cov, t = f1.astype(ld), f2.astype(ld), cov.astype(ld), np.asarray(t).astype(ld)
    R = _quat_to_R(q, ld)
    g = np.cross(t[None, :], f1) @ R
    num = (f2 * g).sum(1)
    den = np.einsum("ni,nij,nj->n", g, cov, g)
    with np.errstate(all="ignore"):
        return float((num * num / den).sum() / ld(len(f1)))


def test_cost_function_at_the_lane_loop_edges(oracle):
    rng = np.random.default_rng(47)
    offsets = _offsets(COST_SIZES)
    M, P = int(offsets[-1]), len(COST_SIZES)
    unit = lambda v: v / np.linalg.norm(v, axis=-1, keepdims=True)
    f1, f2 = unit(rng.normal(size=(M, 3))), unit(rng.normal(size=(M, 3)))
    A = rng.normal(size=(M, 3, 3)) * 1e-3
    cov = A @ np.transpose(A, (0, 2, 1)) + 1e-8 * np.eye(3)
    q, t = rng.normal(size=(P, 4)), unit(rng.normal(size=(P, 3)))      # (q is normalised inside)
    with Batch(capi.MODE_TARGET, offsets) as b:
        b.fill(f1, f2, _c9(cov))
        got = b.cost_function(q, t)
        got_dev = b.cost_function(torch.from_numpy(q).cuda(), torch.from_numpy(t).cuda()).cpu().numpy()
    assert np.array_equal(bits(got), bits(got_dev))
    for p, n in enumerate(COST_SIZES):
        r = slice(offsets[p], offsets[p + 1])
        if n == 0:      # the header: 0 / 0 = NaN, as the reference's function returns for empty input
            assert np.isnan(got[p]) and np.isnan(oracle.cost_function(f1[r], f2[r], cov[r], _quat_to_R(q[p]), t[p]))
            continue
        want = oracle.cost_function(f1[r], f2[r], cov[r], _quat_to_R(q[p]), t[p])
        exact = _cost_longdouble(f1[r], f2[r], cov[r], q[p], t[p])
        print(f"pair {p} (n = {n}): device {abs(got[p] - exact) / exact:.2e}, oracle {abs(want - exact) / exact:.2e} "
              f"from the longdouble value")
        assert abs(want - exact) <= 1e-10 * exact        # the oracle itself is inside the bound on these inputs
        assert got[p] == pytest.approx(want, rel=1e-10)
        assert got[p] == pytest.approx(exact, rel=1e-10)


@pytest.mark.parametrize("mode", [capi.MODE_NEC, capi.MODE_HOST, capi.MODE_SYM])
def test_cost_function_refuses_every_mode_but_target(mode):
    q, t, out = np.array([[0.0, 0.0, 0.0, 1.0]] * 2), np.array([[0.0, 0.0, 1.0]] * 2), np.full(2, -7.25)
    with Batch.uniform(mode, 2, 5) as b:
        rc = capi.lib().pnec_hip_cost_function(b._h, q.ctypes.data, t.ctypes.data, out.ctypes.data, capi.MEM_HOST, None)
        assert rc == capi.ERR_UNSUPPORTED == -3
        assert b"TARGET" in capi.lib().pnec_hip_last_error()
        with pytest.raises(capi.PnecHipError) as e:
            b.cost_function(q, t)
        assert e.value.code == capi.ERR_UNSUPPORTED
    assert np.all(out == -7.25)


# ---- f. select_best -----------------------------------------------------------------------------------------------------
def select_best_np(cost):
    """the contract: the first index of the minimum over the non-NaN entries; 0 if all are NaN"""
    best = np.zeros(len(cost), dtype=np.int32)
    for p, row in enumerate(cost):
        ok = ~np.isnan(row)
        if ok.any():
            best[p] = np.flatnonzero(ok & (row == row[ok].min()))[0]
    return best


_TINY, _SUB = 5e-324, 2.5e-310          # the smallest denormal, and a larger one
_PALETTE = np.array([1.0, 1.0, 2.0, np.nan, np.inf, -0.0, 0.0, _TINY, 2 * _TINY, _SUB, -_SUB, 1.0 + EPS, 1.0 - EPS / 2])


def _pattern(k, H, rng):
    row = rng.choice(_PALETTE[[0, 2, 4, 9, 11]], H)
    if k == 0:                                   # exact ties: the first minimum wins
        row[:] = 2.0
        row[rng.integers(0, H, 2)] = 1.0
    elif k == 1:                                 # a NaN first
        row[0] = np.nan
    elif k == 2:                                 # a NaN last
        row[-1] = np.nan
    elif k == 3:                                 # all NaN
        row[:] = np.nan
    elif k == 4:                                 # +inf everywhere, or behind NaNs: inf beats NaN, the first inf wins
        row[:] = np.inf
        row[:H // 2] = np.nan
    elif k == 5:                                 # -0.0 against +0.0: equal, the first wins
        row[:] = np.where(np.arange(H) % 2 == 0, 0.0, -0.0) if H % 2 else np.where(np.arange(H) % 2 == 0, -0.0, 0.0)
    elif k == 6:                                 # denormals are ordered, not flushed
        row[:] = rng.choice([_TINY, 2 * _TINY, _SUB, 1.0], H)
        if H > 1:
            row[-1] = -_SUB
    else:
        row = rng.choice(_PALETTE, H)
    return row


@pytest.mark.parametrize("n_hyp", [1, 2, 3, 8])
@pytest.mark.parametrize("n_pairs", [1, 255, 256, 257, 1000])
def test_select_best_contract(n_pairs, n_hyp):
    rng = np.random.default_rng(1000 * n_pairs + n_hyp)
    tables = []
    if n_pairs == 1:                             # every pattern on its own
        tables = [_pattern(k, n_hyp, rng)[None, :] for k in range(8)]
    else:
        tables = [np.stack([_pattern(p % 12, n_hyp, rng) for p in range(n_pairs)])]
        last = tables[0].copy()                  # the minimum in the last hypothesis of the last pair (a block's last thread)
        last[-1] = 3.0
        last[-1, -1] = -1.0
        tables.append(last)
    for cost in tables:
        cost = np.ascontiguousarray(cost)
        want = select_best_np(cost)
        got = select_best(cost.reshape(-1), n_hyp)
        got_dev = select_best(torch.from_numpy(cost.reshape(-1)).cuda(), n_hyp).cpu().numpy()
        assert got.dtype == np.int32 and got.shape == (n_pairs,)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (bad[:5], cost[bad[:5]], got[bad[:5]], want[bad[:5]])
        assert np.array_equal(got_dev, want)


def test_select_best_reference_is_the_contract():
    nan, inf = np.nan, np.inf
    cost = np.array([[2.0, 1.0, 1.0], [nan, 3.0, 3.0], [3.0, 2.0, nan], [nan, nan, nan], [nan, inf, inf], [0.0, -0.0, 0.0],
                     [-0.0, 0.0, -_TINY], [2 * _TINY, _TINY, _TINY]])
    assert select_best_np(cost).tolist() == [1, 1, 1, 0, 1, 0, 2, 1]


# ---- g. mask counts through select and select_view ----------------------------------------------------------------------
MASK_SIZES = [0, 1, 64, 65, 513]


def _masks(offsets, rng):
    M = int(offsets[-1])
    first, last = offsets[:-1][np.diff(offsets) > 0], offsets[1:][np.diff(offsets) > 0] - 1
    one = lambda idx: np.bincount(np.asarray(idx, dtype=np.int64), minlength=M).astype(np.uint8)
    return {"all zero": np.zeros(M, dtype=np.uint8), "all one": np.ones(M, dtype=np.uint8),
            "one at the first": one(first), "one at the last": one(last),
            "one at position 63": one([o + 63 for o, n in zip(offsets[:-1], np.diff(offsets)) if n > 63]),
            "one at position 64": one([o + 64 for o, n in zip(offsets[:-1], np.diff(offsets)) if n > 64]),
            "random": (rng.random(M) < 0.5).astype(np.uint8),
            "bytes 0 1 2 255": rng.choice(np.array([0, 1, 2, 255], dtype=np.uint8), M)}


@pytest.mark.parametrize("view", [False, True])
@pytest.mark.parametrize("space", SPACES)
def test_select_counts_and_compacts_by_mask(space, view):
    rng = np.random.default_rng(53)
    d = _Data(MASK_SIZES, 59)
    mode, nc = capi.MODE_TARGET, 12
    src_start, _, src_total = block_layout(mode, d.offsets)
    with Batch(mode, d.offsets) as b:
        _fill(b, mode, "numpy", d.b1, d.b2, d.c, None)
        for name, mask in _masks(d.offsets, rng).items():
            keep = mask != 0
            counts = np.array([keep[d.offsets[p]:d.offsets[p + 1]].sum() for p in range(len(MASK_SIZES))])
            new_offsets = _offsets(counts)
            sel = b.select(_to(space, mask), view=view)
            try:
                assert np.array_equal(sel.offsets, new_offsets), name
                assert sel.num_correspondences == int(keep.sum())
                got = sel.export_payload()
            finally:
                sel.close()
            want = payload_np(mode, new_offsets, d.b1[keep], d.b2[keep], d.c[keep])
            new_start, new_stride, _ = block_layout(mode, new_offsets)
            assert got.size == src_total                       # the source's block layout is kept
            for p in range(len(MASK_SIZES)):
                size = nc * int(new_stride[p])
                _assert_same_bits(got[src_start[p]:src_start[p] + size], want[new_start[p]:new_start[p] + size],
                                  f"{name}: pair {p}")
        _assert_same_bits(b.export_payload(), payload_np(mode, d.offsets, d.b1, d.b2, d.c), "the source, afterwards")
