"""pnec_hip_trajectory_compose and pnec_hip_trajectory_metrics on the device against the long-double checker of
tests/trajectory_cases.py, against the reference's recorded metrics (tests/golden/trajectory_metrics_golden.npz), and
against themselves bit for bit (a sequence alone, among others, twice, in HOST space, into reused buffers).

Every tolerance is trajectory_cases' bound, derived in include/pnec_hip.h for FP64 (u = 2^-53); each test prints the worst
fraction of the bound it saw.  Statuses, NaN placement, `valid` and everything compared under "bits" are exact.  Lengths:
0, 1, 2, 3 (the short paths), 63 / 64 / 65 (a wavefront: the composition's 64 chunks and the 64-pair stride of a diagonal),
129, 257 (just above the 256-lane block of the row kernels), 1025 (chunks of 17 rows).
"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trajectory_cases as tc  # noqa: E402

import pnec_amd  # noqa: E402
from pnec_amd import Trajectory, compose_trajectory, matched, stack_steps, trajectory_metrics  # noqa: E402
from pnec_amd.trajectory import new_trajectory_metrics  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trajectory_metrics_golden.npz")
LENGTHS = (0, 1, 2, 3, 63, 64, 65, 129, 257, 1025)
FLAVOURS = {"golden": (1e-2, 0.05), "wide": (0.3, 0.5), "tiny": (1e-7, 0.05)}   # (noise, step); wide: angles up to pi


def _torch():
    import torch
    return torch


def _dev(a, dtype=None):
    torch = _torch()
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda:0")


def _np(t):
    return None if t is None else (t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t))


@functools.lru_cache(maxsize=None)
def case(L, flavour="golden", seed=100):
    noise, step = FLAVOURS[flavour]
    return tc.traj(L, noise, seed + L, step)


@functools.lru_cache(maxsize=None)
def exact(L, flavour="golden", seed=100):
    """the long-double checker on case(...): computed once, shared, never written to"""
    t = case(L, flavour, seed)
    return tc.metrics_np([0, L], t.est_q, t.gt_q, t.est_p, t.gt_p, dtype=np.longdouble)


def _same_nan(a, b, what):
    assert np.array_equal(np.isnan(a), np.isnan(np.asarray(b, dtype=np.float64))), f"{what}: NaN placement"


def check_scored(got, want, offsets, n_rows, what):
    """device outputs (numpy) against the long-double checker, sequence by sequence; returns the worst fractions"""
    frac = {}

    def note(name, diff, bound):
        diff, bound = np.asarray(diff, dtype=np.float64), np.asarray(bound, dtype=np.float64)
        ok = ~np.isnan(diff)
        if ok.any():
            f = float((diff[ok] / bound[ok] if bound.ndim else diff[ok] / bound).max())
            frac[name] = max(frac.get(name, 0.0), f)
            assert f <= 1.0, f"{what}: {name} is {f:.2f} of its bound"

    f64 = lambda a: np.asarray(a, dtype=np.float64)
    _same_nan(got.err_q, want.err_q, what + " err_q")
    note("err_q", np.sqrt(((got.err_q - want.err_q) ** 2).sum(axis=1)), tc.BOUND_ERR_Q)
    for f in range(len(offsets) - 1):
        lo, hi = tc.cut(offsets, f, n_rows)
        L = hi - lo
        m = np.array([float(getattr(got, k)[f]) for k in tc.METRICS])
        _same_nan(m, want.metrics[f], f"{what} metrics of sequence {f}")
        if L < 1:
            continue
        for name in ("rmse_d", "l1_d", "angle1", "rt1"):
            if getattr(want, name) is None:
                assert getattr(got, name) is None
                continue
            g, w = getattr(got, name)[lo:hi], getattr(want, name)[lo:hi]
            _same_nan(g, w, f"{what} {name} of sequence {f}")
            assert g[0] == 0.0
            if name in ("rmse_d", "l1_d"):
                note(name, np.abs(g - w), tc.bound_distance(L, np.arange(L), f64(w)))
            else:
                note(name, np.abs(g - w), tc.bound_angle(f64(w)))
        if L >= 2:
            note("metrics", np.abs(m - want.metrics[f]), tc.bound_metrics(L, np.nan_to_num(f64(want.metrics[f]))))
    return frac


def score_device(off, d, positions=True, out=None):
    torch = _torch()
    s = trajectory_metrics(_dev(off, torch.int64), _dev(d["est_q"]), _dev(d["gt_q"]),
                           _dev(d["est_p"]) if positions else None, _dev(d["gt_p"]) if positions else None, out=out)
    torch.cuda.synchronize()
    return s


def to_numpy(s):
    return type(s)(*[_np(getattr(s, k.name)) for k in s.__dataclass_fields__.values()])


# ------------------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("L", LENGTHS)
def test_metrics_of_one_sequence_against_the_long_double_checker(L):
    t = case(L)
    off, d = tc.concat([t])
    got = to_numpy(score_device(off, d))
    frac = check_scored(got, exact(L), off, L, f"L={L}")
    print(f"L={L}: worst fraction of each bound {frac}")
    assert got.metrics.shape == (1, 5) and got.rmse_d.shape == (L,) and got.err_q.shape == (L, 4)
    if L < 2:
        assert np.isnan(got.metrics).all()
    # without positions: r_t is NaN, rt1 is not there, the rest has the same bits
    bare = to_numpy(score_device(off, d, positions=False))
    assert bare.rt1 is None and np.isnan(bare.r_t).all()
    for k in ("RPE_1", "RPE_n", "L1RPE_1", "L1RPE_n", "rmse_d", "l1_d", "err_q", "angle1"):
        assert np.array_equal(getattr(bare, k), getattr(got, k), equal_nan=True), k


@pytest.mark.parametrize("flavour,L", [("wide", 257), ("wide", 65), ("tiny", 257), ("tiny", 3)])
def test_metrics_at_angles_up_to_pi_and_at_1e_minus_7(flavour, L):
    t = case(L, flavour)
    off, d = tc.concat([t])
    got = to_numpy(score_device(off, d))
    want = exact(L, flavour)
    frac = check_scored(got, want, off, L, f"{flavour} L={L}")
    print(f"{flavour} L={L}: largest angle {float(np.nanmax(got.angle1)):.3e}, rmse_d up to {float(got.rmse_d.max()):.3e}; "
          f"worst fraction of each bound {frac}")
    if flavour == "wide":
        assert got.rmse_d.max() > 2.0 and got.angle1.max() <= np.pi
    else:
        assert 1e-8 < got.RPE_1[0] < 1e-6


def test_an_exact_estimate_scores_zero():
    t = case(130)
    off = np.array([0, 130])
    s = to_numpy(score_device(off, dict(est_q=t.gt_q, gt_q=t.gt_q, est_p=t.gt_p, gt_p=t.gt_p)))
    assert np.array_equal(s.metrics, np.zeros((1, 5))) and not s.rmse_d.any() and not s.angle1.any() and not s.rt1.any()
    assert np.array_equal(s.err_q, np.tile([0.0, 0.0, 0.0, 1.0], (130, 1)))


def test_rows_that_are_not_finite_and_steps_of_no_length():
    t = case(65)
    est_q, est_p = t.est_q.copy(), t.est_p.copy()
    est_q[7, 2] = np.nan
    est_q[20] = 0.0          # a zero quaternion normalises to NaN
    est_p[41] = est_p[40]    # a step of length zero
    off = np.array([0, 65])
    d = dict(est_q=est_q, gt_q=t.gt_q, est_p=est_p, gt_p=t.gt_p)
    got = to_numpy(score_device(off, d))
    want = tc.metrics_np(off, est_q, t.gt_q, est_p, t.gt_p, dtype=np.longdouble)
    check_scored(got, want, off, 65, "non-finite rows")
    assert np.isnan(got.metrics).all() and np.isnan(got.rt1[41]) and np.isnan(got.angle1[[7, 8, 20, 21]]).all()
    assert np.isfinite(got.angle1[[1, 6, 9, 19, 22, 64]]).all()
    # a distance takes the NaN of row 7 as long as the pair (7, 7 + d) exists; beyond it no pair holds row 7 or row 20
    assert np.isnan(got.rmse_d[1:58]).all() and np.isfinite(got.rmse_d[58:]).all() and np.isfinite(got.l1_d[58:]).all()


# ----------------------------------------------------------------------------------------------------------- batches
@functools.lru_cache(maxsize=None)
def seventy():
    trajs = [case(L, seed=300) for L in range(70)]
    off, d = tc.concat(trajs)
    want = tc.metrics_np(off, d["est_q"], d["gt_q"], d["est_p"], d["gt_p"], dtype=np.longdouble)
    return off, d, want


def test_metrics_of_three_sequences_with_an_empty_one_in_the_middle():
    off, d = tc.concat([case(65), case(0), case(257)])
    assert off.tolist() == [0, 65, 65, 322]
    got = to_numpy(score_device(off, d))
    want = tc.metrics_np(off, d["est_q"], d["gt_q"], d["est_p"], d["gt_p"], dtype=np.longdouble)
    print("worst fraction of each bound", check_scored(got, want, off, 322, "(65, 0, 257)"))
    assert np.isnan(got.metrics[1]).all() and np.isfinite(got.metrics[[0, 2]]).all()


def test_metrics_of_seventy_sequences_of_lengths_0_to_69():
    off, d, want = seventy()
    got = to_numpy(score_device(off, d))
    print("worst fraction of each bound", check_scored(got, want, off, int(off[-1]), "70 sequences"))
    assert np.isnan(got.metrics[:2]).all() and np.isfinite(got.metrics[2:]).all()


def test_offsets_that_need_the_cut():
    """DEVICE space takes offsets as they are: lo = clamp(offsets[f], 0, n), hi = clamp(offsets[f+1], lo, n)"""
    torch = _torch()
    t = case(129)
    off = np.array([-5, 40, 40, 1000, 2000], dtype=np.int64)   # -> [0, 40), empty, [40, 129), empty
    d = dict(est_q=t.est_q, gt_q=t.gt_q, est_p=t.est_p, gt_p=t.gt_p)
    got = to_numpy(score_device(off, d))
    want = tc.metrics_np(off, t.est_q, t.gt_q, t.est_p, t.gt_p, dtype=np.longdouble)
    check_scored(got, want, off, 129, "cut offsets")
    clean = to_numpy(score_device(np.array([0, 40, 40, 129, 129]), d))
    for k in ("metrics", "rmse_d", "l1_d", "err_q", "angle1", "rt1"):
        assert np.array_equal(getattr(got, k), getattr(clean, k), equal_nan=True), k
    # rows of no sequence keep what the buffers held (err_q aside), in both calls
    off = np.array([3, 50], dtype=np.int64)
    out = new_trajectory_metrics(1, 129, True, torch.device("cuda:0"))
    for a in (out.rmse_d, out.l1_d, out.angle1, out.rt1):
        a.fill_(-7.25)
    got = to_numpy(score_device(off, d, out=out))
    for a in (got.rmse_d, got.l1_d, got.angle1, got.rt1):
        assert np.all(a[:3] == -7.25) and np.all(a[50:] == -7.25) and np.all(a[3:50] != -7.25)
    alone = to_numpy(score_device(np.array([0, 47]), {k: v[3:50] for k, v in d.items()}))
    assert np.array_equal(got.metrics, alone.metrics) and np.array_equal(got.rmse_d[3:50], alone.rmse_d)
    q = torch.full((129, 4), -7.25, dtype=torch.float64, device="cuda:0")
    p = torch.full((129, 3), -7.25, dtype=torch.float64, device="cuda:0")
    v = torch.full((129,), 9, dtype=torch.uint8, device="cuda:0")
    c = compose_trajectory(_dev(off), _dev(t.rel_q), _dev(t.rel_t), out=Trajectory(q, p, v))
    cq, cv = _np(c.q), _np(c.valid)
    assert np.all(cq[:3] == -7.25) and np.all(cq[50:] == -7.25) and np.all(cv[:3] == 9) and np.all(cv[3:50] == 1)
    alone = compose_trajectory(_dev(np.array([0, 47])), _dev(t.rel_q[3:50]), _dev(t.rel_t[3:50]))
    assert np.array_equal(cq[3:50], _np(alone.q)) and np.array_equal(_np(c.p)[3:50], _np(alone.p))


# ------------------------------------------------------------------------------------------------------- the golden
def test_the_references_recorded_metrics():
    """|device - reference| <= recorded |reference - longdouble| + the bound, for all five metrics"""
    g = np.load(GOLDEN)
    for i, (L, *_rest) in enumerate(tc.GOLDEN_CASES):
        d = {k: g[f"{k}_{i}"] for k in ("est_q", "est_p", "gt_q", "gt_p")}
        got = to_numpy(score_device(np.array([0, L]), d))
        ref, ref_err = g[f"ref_{i}"], g[f"ref_err_{i}"]
        diff, bound = np.abs(got.metrics[0] - ref), tc.bound_metrics(L, ref)
        print(f"L={L}: |device - reference| {diff}; recorded reference error {ref_err}; bound {bound}")
        assert np.all(diff <= ref_err + bound), (L, diff, ref_err, bound)
        rows = got.rows([f"seq{i}"])
        assert rows[1] == f"seq{i}," + ",".join("%.3f" % np.degrees(v) for v in ref)


# ------------------------------------------------------------------------------------------------------------- bits
def test_a_sequences_bits_do_not_depend_on_its_neighbours_or_its_position():
    off70, d70, _ = seventy()
    all70 = to_numpy(score_device(off70, d70))
    torch = _torch()
    c70 = compose_trajectory(_dev(off70), _dev(d70["rel_q"]), _dev(d70["rel_t"]))
    torch.cuda.synchronize()
    for f in (2, 37, 69):
        lo, hi = int(off70[f]), int(off70[f + 1])
        one = {k: v[lo:hi] for k, v in d70.items()}
        alone = to_numpy(score_device(np.array([0, hi - lo]), one))
        assert np.array_equal(alone.metrics[0], all70.metrics[f])
        for k in ("rmse_d", "l1_d", "err_q", "angle1", "rt1"):
            assert np.array_equal(getattr(alone, k), getattr(all70, k)[lo:hi]), (f, k)
        ca = compose_trajectory(_dev(np.array([0, hi - lo])), _dev(one["rel_q"]), _dev(one["rel_t"]))
        assert np.array_equal(_np(ca.q), _np(c70.q)[lo:hi]) and np.array_equal(_np(ca.p), _np(c70.p)[lo:hi])
    # first, last and in the middle of others
    t = case(69, seed=300)
    for order in ((69, 5, 64), (5, 69, 64), (5, 64, 69)):
        off, d = tc.concat([case(L, seed=300) for L in order])
        s = to_numpy(score_device(off, d))
        f = order.index(69)
        assert np.array_equal(s.metrics[f], all70.metrics[69]), order
        assert np.array_equal(s.rmse_d[off[f]:off[f + 1]], all70.rmse_d[off70[69]:off70[70]])
    assert t.L == 69


def test_twice_the_same_call_host_space_and_reused_buffers():
    torch = _torch()
    off, d = tc.concat([case(65), case(0), case(257)])
    a = score_device(off, d)
    b = score_device(off, d)
    fields = ("metrics", "rmse_d", "l1_d", "err_q", "angle1", "rt1")
    for k in fields:
        assert torch.equal(getattr(a, k).view(torch.int64), getattr(b, k).view(torch.int64)), k
    # HOST space: numpy in, numpy out
    h = trajectory_metrics(off, d["est_q"], d["gt_q"], d["est_p"], d["gt_p"])
    assert isinstance(h.rmse_d, np.ndarray)
    for k in fields:
        assert np.array_equal(getattr(h, k), _np(getattr(a, k)), equal_nan=True), k
    # out=: the same buffers come back, holding the same bits
    out = new_trajectory_metrics(3, 322, True, torch.device("cuda:0"))
    for k in fields:
        getattr(out, k).fill_(float("nan"))
    c = score_device(off, d, out=out)
    for k in fields:
        assert getattr(c, k).data_ptr() == getattr(out, k).data_ptr()
        assert torch.equal(getattr(c, k).view(torch.int64), getattr(a, k).view(torch.int64)), k
    # compose likewise
    args = (d["rel_q"], d["rel_t"])
    ca = compose_trajectory(_dev(off), *map(_dev, args))
    cb = compose_trajectory(_dev(off), *map(_dev, args), out=Trajectory(torch.empty_like(ca.q), torch.empty_like(ca.p),
                                                                         torch.empty_like(ca.valid)))
    ch = compose_trajectory(off, *args)
    for k in ("q", "p", "valid"):
        assert np.array_equal(_np(getattr(ca, k)), _np(getattr(cb, k))) and np.array_equal(_np(getattr(ca, k)), getattr(ch, k)), k
    with pytest.raises(ValueError, match="out"):
        score_device(off, d, out=new_trajectory_metrics(3, 321, True, torch.device("cuda:0")))


# ---------------------------------------------------------------------------------------------------------- compose
def check_composed(got, off, rel_q, rel_t=None, scale=None, q0=None, p0=None, what=""):
    n = len(rel_q)
    want = tc.compose_np(off, rel_q, rel_t, scale, q0, p0, dtype=np.longdouble)
    worst = [0.0, 0.0]
    assert np.array_equal(_np(got.valid)[want.valid != 255], want.valid[want.valid != 255]), what + ": valid"
    for f in range(len(off) - 1):
        lo, hi = tc.cut(off, f, n)
        L = hi - lo
        if L == 0:
            continue
        gq = _np(got.q)[lo:hi]
        assert np.allclose(np.linalg.norm(gq, axis=1), 1.0, rtol=0, atol=4 * tc.U), what + ": out_q is normalised"
        fq = tc.sign_aligned_diff(gq, want.q[lo:hi]) / tc.bound_compose_q(L)
        worst[0] = max(worst[0], float(fq.max()))
        if rel_t is not None:
            st = np.asarray(rel_t, dtype=np.float64)[lo:hi] * (1.0 if scale is None else np.asarray(scale)[lo:hi, None])
            path = np.linalg.norm(np.where(np.isfinite(st), st, 0.0), axis=1).sum() + (0.0 if p0 is None else np.linalg.norm(p0[f]))
            dp = np.linalg.norm((_np(got.p)[lo:hi] - want.p[lo:hi]).astype(np.float64), axis=1)
            worst[1] = max(worst[1], float(dp.max() / tc.bound_compose_p(L, path)) if path > 0 else float(dp.max() > 0))
        else:
            assert got.p is None
    assert worst[0] <= 1.0 and worst[1] <= 1.0, (what, worst)
    return worst


@pytest.mark.parametrize("L", [L for L in LENGTHS if L > 0])
def test_compose_one_sequence_with_and_without_each_optional_array(L):
    t = case(L)
    rng = np.random.default_rng(L)
    off = np.array([0, L])
    scale = rng.uniform(0.5, 2.0, L)
    q0 = rng.normal(size=(1, 4)) * 3.0     # not unit: the call normalises it
    p0 = rng.normal(size=(1, 3))
    worst = {}
    for name, kw in (("q", {}), ("q t", dict(rel_t=t.rel_t)), ("q t scale", dict(rel_t=t.rel_t, scale=scale)),
                     ("q q0", dict(q0=q0)), ("all", dict(rel_t=t.rel_t, scale=scale, q0=q0, p0=p0))):
        got = compose_trajectory(_dev(off), _dev(t.rel_q), **{k: _dev(v) for k, v in kw.items()})
        worst[name] = check_composed(got, off, t.rel_q, what=f"L={L} {name}", **kw)
        assert _np(got.valid).all()
    print(f"L={L}: worst fractions of the (q, p) bounds {worst}")
    # the first row is a pose itself
    got = compose_trajectory(_dev(off), _dev(t.rel_q), _dev(t.rel_t))
    assert tc.sign_aligned_diff(_np(got.q)[:1], t.rel_q[:1])[0] <= 4 * tc.U and np.array_equal(_np(got.p)[0], t.rel_t[0])


def test_compose_carries_the_pose_over_absent_rows():
    L = 1025                           # chunks of 17 rows: row 17 k is a chunk's first, 17 k + 16 its last
    t = case(L)
    rel_q, rel_t, scale = t.rel_q.copy(), t.rel_t.copy(), np.ones(L)
    absent = [0, 16, 17, 25, 34, 500, 501, 502, 510, 1007, 1024]
    rel_q[0] = np.nan                  # first
    rel_q[16, 3] = np.inf              # a chunk's last row
    rel_t[17, 0] = np.nan              # a chunk's first row
    rel_q[25] = 0.0                    # mid-chunk: a zero quaternion
    rel_q[34] = np.nan                 # the first row of lane 2's chunk and of lane 30's: the pose before it comes from the
    rel_t[510, 1] = np.inf             # lane below walking its chunk, this row's from the scan -- another association
    scale[500] = np.nan
    rel_q[501] = np.nan
    rel_t[502] = np.inf
    scale[1007] = np.inf
    rel_q[1024] = np.nan               # last
    off = np.array([0, L])
    got = compose_trajectory(_dev(off), _dev(rel_q), _dev(rel_t), _dev(scale))
    v = _np(got.valid)
    assert np.flatnonzero(v == 0).tolist() == absent and set(v.tolist()) == {0, 1}
    q, p = _np(got.q), _np(got.p)
    assert np.isfinite(q).all() and np.isfinite(p).all()
    assert np.array_equal(q[0], [0.0, 0.0, 0.0, 1.0]) and not p[0].any()
    path = float(np.linalg.norm(np.where(np.isfinite(rel_t), rel_t, 0.0), axis=1).sum())
    for r in absent[1:]:
        if r % 17 == 0 and r // 17 >= 2:   # carried to the composition's rounding
            assert tc.sign_aligned_diff(q[r:r + 1], q[r - 1:r])[0] <= tc.bound_compose_q(L), r
            assert np.linalg.norm(p[r] - p[r - 1]) <= tc.bound_compose_p(L, path), r
        else:                              # carried bit for bit
            assert np.array_equal(q[r], q[r - 1]) and np.array_equal(p[r], p[r - 1]), r
    print("worst fractions of the (q, p) bounds", check_composed(got, off, rel_q, rel_t, scale, what="absent rows"))
    # in a batch: sequences that are all absent, empty, and one row long
    off = np.array([0, 1, 1, 3, 20])
    rq = t.rel_q[:20].copy()
    rq[0] = np.nan
    rq[1:3] = 0.0
    got = compose_trajectory(_dev(off), _dev(rq))
    assert _np(got.valid).tolist() == [0, 0, 0] + [1] * 17 and np.array_equal(_np(got.q)[:3], np.tile([0.0, 0.0, 0.0, 1.0], (3, 1)))
    check_composed(got, off, rq, what="batch with absent sequences")


def test_compose_seventy_sequences():
    off, d, _ = seventy()
    rng = np.random.default_rng(70)
    q0, p0 = tc.qnorm(rng.normal(size=(70, 4))), rng.normal(size=(70, 3))
    got = compose_trajectory(_dev(off), _dev(d["rel_q"]), _dev(d["rel_t"]), q0=_dev(q0), p0=_dev(p0))
    print("worst fractions of the (q, p) bounds", check_composed(got, off, d["rel_q"], d["rel_t"], q0=q0, p0=p0, what="70"))


# ------------------------------------------------------------------------------------------------------- end to end
def test_compose_then_matched_then_metrics_on_the_goldens_steps():
    """The estimate composed on the device, two frames dropped, scored against the same rows of the ground truth, equals
    the score of the checker-composed estimate within the sum of both bounds: the metric's own, plus what the composition's
    bound can move it by -- an angle of two error rotations moves by at most 2 * 2 * |dq| per rotation (chord to angle:
    a factor below 2 sqrt 2 for each of the two), taken here as 8 |dq|; r_t's directions move by |dp| / |step| each."""
    g = np.load(GOLDEN)
    i, L = 4, 257
    rel_q, rel_t = g[f"rel_q_{i}"].copy(), g[f"rel_t_{i}"].copy()
    gt_q, gt_p = g[f"gt_q_{i}"], g[f"gt_p_{i}"]
    rel_q[[40, 200]] = np.nan
    off = np.array([0, L])
    traj = compose_trajectory(_dev(off), _dev(rel_q), _dev(rel_t))
    o2, eq, ep, gq, gp = matched(_dev(off), traj, _dev(gt_q), _dev(gt_p))
    assert _np(o2).tolist() == [0, L - 2] and eq.shape == (L - 2, 4) and gq.is_cuda
    got = to_numpy(trajectory_metrics(o2, eq, gq, ep, gp))
    c = tc.compose_np(off, rel_q, rel_t, dtype=np.longdouble)
    keep = c.valid == 1
    want = tc.metrics_np([0, L - 2], c.q[keep], gt_q[keep], c.p[keep], gt_p[keep], dtype=np.longdouble)
    m = want.metrics[0].astype(np.float64)
    slack_q = 8.0 * tc.bound_compose_q(L)
    steps = np.linalg.norm(np.diff(c.p[keep].astype(np.float64), axis=0), axis=1)
    slack_t = 2.0 * 2.0 * tc.bound_compose_p(L, float(L)) / steps.min() + slack_q
    bound = tc.bound_metrics(L - 2, m) + np.array([slack_q] * 4 + [slack_t])
    diff = np.abs(got.metrics[0] - m)
    print(f"|device chain - checker chain| {diff}, bound {bound}")
    assert np.all(diff <= bound)


def test_an_odometry_run_scores_zero_against_itself_and_allocates_nothing_per_call():
    from pnec_amd import Odometry
    from pnec_amd.multi import alloc_counters
    from test_odometry_gpu import K_INV, TRACKER, _frames
    from test_patch_track_cpu import H0, W0
    from test_tracks_cpu import SEQ_F
    torch = _torch()
    frames = _frames()
    odo = Odometry(SEQ_F, H0, W0, K_INV, **TRACKER)
    assert odo.process(frames[0]) is None
    steps = [odo.process(frames[n]) for n in range(1, 4)]
    off, rel_q, rel_t = stack_steps(steps)
    assert off.tolist() == [4 * f for f in range(SEQ_F + 1)] and rel_q.is_cuda
    traj = compose_trajectory(off, rel_q, rel_t)
    o2, eq, ep, gq, gp = matched(off, traj, traj.q, traj.p)
    s = trajectory_metrics(o2, eq, gq, ep, gp)
    torch.cuda.synchronize()
    m = _np(s.metrics)
    L = np.diff(_np(o2))
    assert np.array_equal(m[L >= 2][:, :4], np.zeros((int((L >= 2).sum()), 4))) and np.isnan(m[L < 2]).all()
    assert (L >= 2).any() and np.isfinite(_np(eq)).all()
    # the second call into the first call's buffers: no allocation
    a0 = alloc_counters()
    compose_trajectory(off, rel_q, rel_t, out=traj)
    trajectory_metrics(o2, eq, gq, ep, gp, out=s)
    torch.cuda.synchronize()
    assert alloc_counters()["hip_malloc_calls"] == a0["hip_malloc_calls"]
    odo.close()


# ------------------------------------------------------------------------------------------------------ stream order
def test_device_space_calls_respect_stream_order():
    from test_stream_order_gpu import Entry, check
    torch = _torch()
    trajs = lambda seed: tc.concat([case(L, seed=seed) for L in (65, 0, 257, 1)])
    (off, good), (_, decoy) = trajs(500), trajs(600)
    off_d = _dev(off)
    n = int(off[-1])
    keys = ("est_q", "gt_q", "est_p", "gt_p")
    out = new_trajectory_metrics(4, n, True, torch.device("cuda:0"))

    def call_metrics(bufs):
        s = trajectory_metrics(off_d, *[bufs[k] for k in keys], out=out)
        return [s.metrics, s.rmse_d, s.l1_d, s.err_q, s.angle1, s.rt1], None

    check(Entry({k: _dev(good[k]) for k in keys}, {k: _dev(decoy[k]) for k in keys}, call_metrics,
                sentinels=[out.metrics, out.rmse_d, out.l1_d, out.err_q, out.angle1, out.rt1]), "trajectory_metrics")
    tr = Trajectory(torch.empty((n, 4), dtype=torch.float64, device="cuda:0"),
                    torch.empty((n, 3), dtype=torch.float64, device="cuda:0"),
                    torch.empty((n,), dtype=torch.uint8, device="cuda:0"))

    def call_compose(bufs):
        c = compose_trajectory(off_d, bufs["rel_q"], bufs["rel_t"], out=tr)
        return [c.q, c.p, c.valid], None

    check(Entry({k: _dev(good[k]) for k in ("rel_q", "rel_t")}, {k: _dev(decoy[k]) for k in ("rel_q", "rel_t")}, call_compose,
                sentinels=[tr.q, tr.p, tr.valid]), "trajectory_compose")


# ------------------------------------------------------------------------------------------------- pnec_amd.evaluate
def test_evaluate_scores_a_pose_file_against_kitti_ground_truth(tmp_path):
    """The files of one run -- relative poses with one frame missing, KITTI 3x4 ground truth, times.txt -- through
    pnec_amd.evaluate, against the checker on the same rows (bounds as in the end-to-end test above)."""
    from pnec_amd import evaluate
    g = np.load(GOLDEN)
    i, L = 2, 65
    rel_q, rel_t, gt_q, gt_p = (g[f"{k}_{i}"] for k in ("rel_q", "rel_t", "gt_q", "gt_p"))
    times = 1.5e9 + 0.1036 * np.arange(L)
    have = np.arange(L) != 10
    # (a missing frame's step is lost with it, as in the reference: the file holds steps between the frames it has)
    np.savetxt(tmp_path / "est.txt", np.column_stack([times, rel_t, rel_q])[have], fmt="%.17g")
    np.savetxt(tmp_path / "gt.txt", np.concatenate([tc.qmat(gt_q), gt_p[:, :, None]], axis=2).reshape(L, 12), fmt="%.17g")
    np.savetxt(tmp_path / "times.txt", times, fmt="%.17g")
    s = evaluate.evaluate(tmp_path / "est.txt", tmp_path / "gt.txt", tmp_path / "times.txt")
    gq = evaluate.rotations_to_quaternions(evaluate.read_kitti_poses(tmp_path / "gt.txt")[0])
    q0, p0 = evaluate.pose_correction(gq[0], gt_p[0], rel_q[0], rel_t[0])
    n = int(have.sum())
    c = tc.compose_np([0, n], rel_q[have], rel_t[have], q0=q0[None], p0=p0[None], dtype=np.longdouble)
    want = tc.metrics_np([0, n], c.q, gq[have], c.p, gt_p[have], dtype=np.longdouble).metrics[0].astype(np.float64)
    steps = np.linalg.norm(np.diff(c.p.astype(np.float64), axis=0), axis=1)
    path = float(np.linalg.norm(rel_t[have], axis=1).sum() + np.linalg.norm(p0))
    slack_q = 8.0 * tc.bound_compose_q(n)
    bound = tc.bound_metrics(n, want) + np.array([slack_q] * 4 + [4.0 * tc.bound_compose_p(n, path) / steps.min() + slack_q])
    diff = np.abs(s.metrics[0] - want)
    print(f"|evaluate - checker| {diff}, bound {bound}")
    assert s.metrics.shape == (1, 5) and np.all(diff <= bound)
    assert s.rows(["pnec"])[1].startswith("pnec,") and len(s.rows(["pnec"])[1].split(",")) == 6


# ------------------------------------------------------------------------------------------- the facade through pypnec
def test_pypnec_composes_and_scores_like_the_python_calls():
    """pypnec.compose_trajectory / trajectory_metrics (pnec::odometry::ComposeTrajectory / TrajectoryMetrics below them) on
    a golden trajectory as [N,4,4] poses against pnec_amd's calls on the quaternions.  The facade goes through rotation
    matrices: a quaternion to a matrix here and back by Shepperd's form there moves it by a few u -- 16 u is taken per
    pose -- and an angle of two error rotations by at most 8 |dq| (as in the end-to-end test), a matrix entry by 4 |dq|."""
    import pnec_amd.pypnec as pypnec
    g = np.load(GOLDEN)
    i, L = 2, 65
    rel_q, rel_t, est_q, est_p, gt_q, gt_p = (g[f"{k}_{i}"] for k in ("rel_q", "rel_t", "est_q", "est_p", "gt_q", "gt_p"))

    def poses(q, p):
        M = np.tile(np.eye(4), (len(q), 1, 1))
        M[:, :3, :3], M[:, :3, 3] = tc.qmat(q), p
        return M

    dq = 16.0 * tc.U
    rel = poses(rel_q, rel_t)
    rel[21] = np.nan                                   # a frame without a pose (the second row of a lane's chunk of two)
    rq, rt = rel_q.copy(), rel_t.copy()
    rq[21] = np.nan
    q0 = tc.qnorm(np.array([[0.3, -0.1, 0.2, 0.9]]))   # the correction: a left factor, not a right one
    p0 = np.array([[0.5, -1.0, 2.0]])
    got, valid = pypnec.compose_trajectory(rel, poses(q0, p0)[0])
    want = compose_trajectory(np.array([0, L]), rq, rt, q0=q0, p0=p0)
    assert got.shape == (L, 4, 4) and valid.dtype == np.uint8 and np.array_equal(valid, want.valid) and valid[21] == 0
    assert np.array_equal(got[:, 3], np.tile([0.0, 0.0, 0.0, 1.0], (L, 1)))
    slack = 4.0 * (dq * (L + 2) + tc.bound_compose_q(L))
    assert np.abs(got[:, :3, :3] - tc.qmat(want.q)).max() <= slack
    assert np.abs(got[:, :3, 3] - want.p).max() <= slack * (L + np.linalg.norm(p0))
    assert np.array_equal(got[21], got[20])
    plain, _ = pypnec.compose_trajectory(poses(rel_q, rel_t))
    assert np.abs(plain[0] - poses(rel_q, rel_t)[0]).max() <= 4.0 * dq   # no correction: the first pose is itself
    # the metrics
    s = pypnec.trajectory_metrics(poses(est_q, est_p), poses(gt_q, gt_p))
    w = trajectory_metrics(np.array([0, L]), est_q, gt_q, est_p, gt_p)
    m = np.array([s[k] for k in tc.METRICS])
    bound = tc.bound_metrics(L, w.metrics[0]) + 8.0 * 2.0 * dq
    print(f"|pypnec - python| {np.abs(m - w.metrics[0])}, bound {bound}")
    assert np.all(np.abs(m - w.metrics[0]) <= bound)
    for k in ("rmse_d", "l1_d", "angle1", "rt1"):
        assert s[k].shape == (L,) and s[k][0] == 0.0
        assert np.abs(s[k] - getattr(w, k)).max() <= tc.bound_distance(L, 1, getattr(w, k).max()) + 8.0 * 2.0 * dq, k
