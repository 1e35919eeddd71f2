"""Trajectory evaluation without a GPU: pnec_hip_trajectory_compose and pnec_hip_trajectory_metrics are declared, bound and
exported within ABI 8, their argument checks refuse before a device is touched, and the numpy checker of
tests/trajectory_cases.py -- the yardstick of the GPU tests -- agrees with the reference's five metric functions on the
golden trajectories and has the properties the GPU tests rely on.  stack_steps, matched and the timestamp join of
pnec_amd.evaluate run on CPU tensors and a temporary file.  The facade's argument handling and the two new CallArrays
lists run as stand-alone host programs under the address and undefined-behaviour sanitizers; nothing is loaded into
Python under one.
"""
import ctypes as C
import dataclasses
import inspect
import os
import re
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import pnec_amd
from pnec_amd import capi, evaluate, trajectory

import trajectory_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "trajectory_metrics_golden.npz")


def golden_case(g, i):
    return SimpleNamespace(L=int(g["cases"][i][0]), ref=g[f"ref_{i}"], ref_err=g[f"ref_err_{i}"],
                           **{name: g[f"{name}_{i}"] for name in tc.Traj._fields[1:]})


# ------------------------------------------------------------------------------------------------------- the ABI
def test_symbols_are_declared_bound_and_exported_within_abi_8():
    L = capi.lib()
    header = open(os.path.join(ROOT, "include", "pnec_hip.h")).read()
    assert capi.ABI_VERSION == 8 and L.pnec_hip_abi_version() == 8 and "#define PNEC_HIP_ABI_VERSION 8" in header
    for name, count in (("pnec_hip_trajectory_compose", 14), ("pnec_hip_trajectory_metrics", 16)):
        assert name in capi.SYMBOLS and getattr(L, name) is not None
        decl = re.search(r"int " + name + r"\(([^;]*)\);", header)
        assert decl, "the header declares the call"
        params = [p.strip() for p in decl.group(1).replace("\n", " ").split(",")]
        assert params[:4] == ["int device", "int64_t n_seq", "const int64_t *offsets", "int64_t n_rows"]
        assert params[-2:] == ["int space", "void *stream"]
        at = getattr(L, name).argtypes
        assert len(params) == count == len(at)
        assert at[0] is C.c_int and at[1] is C.c_int64 and at[3] is C.c_int64 and at[-2] is C.c_int
    assert "DEVIATION" in header[header.index("pnec_hip_trajectory_metrics: RPE_1"):]


def test_every_refusal_comes_back_before_a_device_is_touched():
    SENT = -7.25
    n, F = 3, 2
    off = np.array([0, 2, 3], dtype=np.int64)
    q, eq, gq = (np.tile([0.0, 0.0, 0.0, 1.0], (n, 1)) for _ in range(3))
    t, ep, gp = (np.zeros((n, 3)) for _ in range(3))
    sc, q0, p0 = np.ones(n), np.tile([0.0, 0.0, 0.0, 1.0], (F, 1)), np.zeros((F, 3))
    oq, op, ov = np.full((n, 4), SENT), np.full((n, 3), SENT), np.full(n, 9, dtype=np.uint8)
    om, oe = np.full((F, 5), SENT), np.full((n, 4), SENT)
    orm, ol, oa, ort = (np.full(n, SENT) for _ in range(4))
    p = lambda a: None if a is None else a.ctypes.data
    L = capi.lib()
    NO_DEVICE = 1 << 20   # exists nowhere: a check that came after the device was touched would fail otherwise

    full_c = dict(n_seq=F, off=off, n=n, q=q, t=t, sc=sc, q0=q0, p0=p0, oq=oq, op=op, ov=ov, space=capi.MEM_HOST)

    def compose(**change):
        a = dict(full_c, **change)
        rc = L.pnec_hip_trajectory_compose(NO_DEVICE, a["n_seq"], p(a["off"]), a["n"], p(a["q"]), p(a["t"]), p(a["sc"]),
                                           p(a["q0"]), p(a["p0"]), p(a["oq"]), p(a["op"]), p(a["ov"]), a["space"], None)
        return rc, (L.pnec_hip_last_error() or b"").decode()

    full_m = dict(n_seq=F, off=off, n=n, eq=eq, gq=gq, ep=ep, gp=gp, om=om, oe=oe, orm=orm, ol=ol, oa=oa, ort=ort,
                  space=capi.MEM_HOST)

    def metrics(**change):
        a = dict(full_m, **change)
        rc = L.pnec_hip_trajectory_metrics(NO_DEVICE, a["n_seq"], p(a["off"]), a["n"], p(a["eq"]), p(a["gq"]), p(a["ep"]),
                                           p(a["gp"]), p(a["om"]), p(a["oe"]), p(a["orm"]), p(a["ol"]), p(a["oa"]), p(a["ort"]),
                                           a["space"], None)
        return rc, (L.pnec_hip_last_error() or b"").decode()

    i64 = lambda *v: np.array(v, dtype=np.int64)
    shared = [(dict(n_seq=0), "n_seq"), (dict(n_seq=-1), "n_seq"), (dict(n_seq=1 << 31), "n_seq"), (dict(n=-1), "n_rows"),
              (dict(n=1 << 31), "n_rows"), (dict(off=None), "offsets"), (dict(space=7), "memory space"),
              (dict(space=-1), "memory space"), (dict(off=i64(1, 2, 3)), "offsets"), (dict(off=i64(0, 3, 2)), "offsets"),
              (dict(off=i64(0, 2, 4)), "offsets")]
    compose_only = [(dict(q=None), "NULL"), (dict(oq=None), "NULL"), (dict(t=None, op=None, p0=None), "rel_t"),
                    (dict(t=None, op=None, sc=None), "rel_t"), (dict(op=None), "out_p"),
                    (dict(t=None, sc=None, p0=None), "out_p"), (dict(oq=q), "also an input"), (dict(op=t), "also an input"),
                    (dict(op=oq), "another output")]
    metrics_only = [(dict(eq=None), "NULL"), (dict(gq=None), "NULL"), (dict(om=None), "out_metrics"),
                    (dict(om=None, n=0, off=i64(0, 0, 0)), "out_metrics"), (dict(oe=None), "NULL"), (dict(orm=None), "NULL"),
                    (dict(ol=None), "NULL"), (dict(gp=None, ort=None), "together"), (dict(ep=None, ort=None), "together"),
                    (dict(ep=None, gp=None), "out_rt1"), (dict(oe=eq), "also an input"), (dict(ort=gp), "also an input"),
                    (dict(ol=orm), "another output"), (dict(ort=oa), "another output")]
    for call, cases in ((compose, shared + compose_only), (metrics, shared + metrics_only)):
        for change, word in cases:
            for space in ((capi.MEM_HOST, capi.MEM_DEVICE) if "off" not in change and "space" not in change else (None,)):
                ch = dict(change) if space is None else dict(change, space=space)
                rc, msg = call(**ch)
                assert rc == capi.ERR_INVALID_ARGUMENT == -1, (ch, rc, msg)
                assert word in msg, (ch, msg)
    # no rows is not a refusal of compose (nothing to write), whatever the row arrays
    assert compose(n=0, off=i64(0, 0, 0))[0] == 0
    assert compose(n=0, off=i64(0, 0, 0), q=None, t=None, sc=None, q0=None, p0=None, oq=None, op=None, ov=None)[0] == 0
    for a in (oq, op, om, oe, orm, ol, oa, ort):
        assert np.all(a == SENT)
    assert np.all(ov == 9)


def test_python_names_and_defaults():
    names = {"compose_trajectory", "trajectory_metrics", "stack_steps", "matched", "Trajectory", "TrajectoryMetrics"}
    assert names <= set(pnec_amd.__all__)
    assert pnec_amd.compose_trajectory is trajectory.compose_trajectory
    assert [f.name for f in dataclasses.fields(pnec_amd.Trajectory)] == ["q", "p", "valid"]
    assert [f.name for f in dataclasses.fields(pnec_amd.TrajectoryMetrics)][:10] == [
        "RPE_1", "RPE_n", "L1RPE_1", "L1RPE_n", "r_t", "rmse_d", "l1_d", "err_q", "angle1", "rt1"]
    assert list(inspect.signature(pnec_amd.compose_trajectory).parameters) == ["offsets", "rel_q", "rel_t", "scale", "q0", "p0", "out"]
    assert list(inspect.signature(pnec_amd.trajectory_metrics).parameters) == ["offsets", "est_q", "gt_q", "est_p", "gt_p", "out"]
    import pnec_amd.pypnec as pypnec
    assert {"compose_trajectory", "trajectory_metrics"} <= set(dir(pypnec))
    facade = open(os.path.join(ROOT, "pnec_amd", "csrc", "host", "pnec_host.h")).read()
    assert "std::vector<SE3d> ComposeTrajectory(const std::vector<SE3d> &relative_poses" in facade
    assert "TrajectoryScore TrajectoryMetrics(const std::vector<SE3d> &estimated" in facade
    assert "wait" in trajectory.matched.__doc__.lower()


def test_rows_are_the_references_metrics_yaml():
    m = np.array([[np.radians(1.23456), np.radians(10.0), 0.0, np.nan, np.radians(0.0004)], [0.1, 0.2, 0.3, 0.4, 0.5]])
    s = trajectory.TrajectoryMetrics(*m.T, None, None, None, None, None, m)
    assert np.allclose(s.degrees()[0, :2], [1.23456, 10.0], rtol=1e-15)
    rows = s.rows(["a", "b"])
    assert rows[0] == "name,RPE_1,RPE_n,L1RPE_1,L1RPE_n,r_t"
    assert rows[1] == "a,1.235,10.000,0.000,,0.000"
    assert rows[2].startswith("b,5.730,11.459,")
    with pytest.raises(ValueError):
        s.rows(["only one"])


# ------------------------------------------------------------------------------------------ the checker and the golden
def test_checker_agrees_with_the_reference_on_the_golden():
    """|float64 checker - reference| <= recorded |reference - longdouble| + the bound, for all five metrics."""
    g = np.load(GOLDEN)
    assert [tuple(r) for r in g["cases"].tolist()] == [tuple(float(v) for v in c) for c in tc.GOLDEN_CASES]
    worst = 0.0
    for i in range(len(tc.GOLDEN_CASES)):
        c = golden_case(g, i)
        assert np.isfinite(c.ref).all()
        t = tc.traj(*[tc.GOLDEN_CASES[i][k] for k in (0, 1, 3, 2)])
        for name in tc.Traj._fields[1:]:   # the generator still makes the recorded inputs
            assert np.allclose(getattr(t, name), getattr(c, name), rtol=0, atol=1e-12), name
        s = tc.metrics_np([0, c.L], c.est_q, c.gt_q, c.est_p, c.gt_p)
        bound = tc.bound_metrics(c.L, c.ref)
        diff = np.abs(s.metrics[0] - c.ref)
        print(f"L={c.L}: |checker - reference| {diff}, recorded reference error {c.ref_err}, bound {bound}")
        assert np.all(diff <= c.ref_err + bound), (c.L, diff, c.ref_err, bound)
        exact = tc.metrics_np([0, c.L], c.est_q, c.gt_q, c.est_p, c.gt_p, dtype=np.longdouble)
        frac = np.abs(s.metrics[0] - exact.metrics[0]).astype(np.float64) / bound
        worst = max(worst, float(frac.max()))
        assert np.all(frac <= 1.0)
    print(f"float64 checker against long double: worst fraction of the bound {worst:.3f}")


def test_trace_identity_on_random_rotations():
    """angle((Est_j' Est_i)(Gt_i' Gt_j)) is the angle between E_i = Est_i Gt_i' and E_j, and the chord form gives it"""
    rng = np.random.default_rng(5)
    est, gt = (tc.qnorm(rng.normal(size=(200, 4))) for _ in range(2))
    Re, Rg = tc.qmat(est), tc.qmat(gt)
    i, j = np.arange(0, 100), np.arange(100, 200)
    rel = (np.swapaxes(Re[j], -1, -2) @ Re[i]) @ (np.swapaxes(Rg[i], -1, -2) @ Rg[j])
    want = np.arccos(np.clip((np.trace(rel, axis1=1, axis2=2) - 1) / 2, -1, 1))
    e = tc.qnorm(tc.qmul(est, tc.qconj(gt)))
    got = tc.chord_angle(e[i], e[j], np.float64)
    assert np.all((got >= 0) & (got <= np.pi))
    assert np.allclose(got, want, rtol=0, atol=1e-7)   # (arccos near 0 and pi keeps half the digits)
    mid = (want > 0.5) & (want < 2.6)
    assert mid.sum() > 20 and np.allclose(got[mid], want[mid], rtol=0, atol=1e-13)
    assert np.allclose(tc.reference_angle(e[i], e[j])[mid], want[mid], rtol=0, atol=1e-13)


def test_an_exact_estimate_scores_zero_where_the_reference_form_gives_nan():
    t = tc.traj(40, 0.0, 3, 0.05)
    s = tc.metrics_np([0, 40], t.gt_q, t.gt_q, t.gt_p, t.gt_p)
    assert np.array_equal(s.metrics[0], np.zeros(5)) and np.all(s.rmse_d == 0) and np.all(s.angle1 == 0)
    assert np.all(s.err_q == [0.0, 0.0, 0.0, 1.0]) and np.all(s.rt1 == 0)
    # the reference's form on rotations that differ by rounding only: arccos of a trace past 3 is NaN for some
    rng = np.random.default_rng(9)
    q = tc.qnorm(rng.normal(size=(2000, 4)))
    R = tc.qmat(q)
    tr = np.trace(np.swapaxes(R, -1, -2) @ R, axis1=1, axis2=2)
    with np.errstate(invalid="ignore"):
        assert np.isnan(np.arccos((tr - 1.0) / 2.0)).any()


def test_small_angles_keep_their_digits():
    t = tc.traj(65, 1e-7, 21, 0.05)
    a = tc.metrics_np([0, 65], t.est_q, t.gt_q, t.est_p, t.gt_p)
    b = tc.metrics_np([0, 65], t.est_q, t.gt_q, t.est_p, t.gt_p, dtype=np.longdouble)
    assert 1e-8 < a.metrics[0, 0] < 1e-6
    assert np.all(np.abs(a.angle1 - b.angle1) <= tc.bound_angle(b.angle1.astype(np.float64)))
    assert np.all(np.abs(a.metrics[0] - b.metrics[0]) <= tc.bound_metrics(65, a.metrics[0]))
    # the reference's form loses them: its relative error at these angles is far above the bound
    e = a.err_q
    ref = tc.reference_angle(e[:-1], e[1:])
    with np.errstate(invalid="ignore"):
        rel = np.abs(ref - b.angle1[1:].astype(np.float64)) / b.angle1[1:].astype(np.float64)
    assert np.nanmedian(rel) > 1e-6 or np.isnan(ref).any()


def test_short_sequences_and_the_divisor():
    t = tc.traj(5, 1e-2, 4, 0.05)
    for L in (0, 1):
        s = tc.metrics_np([0, L], t.est_q[:L], t.gt_q[:L], t.est_p[:L], t.gt_p[:L])
        assert np.isnan(s.metrics).all() and s.metrics.shape == (1, 5)
        assert s.rmse_d.tolist() == [0.0] * L and s.rt1.tolist() == [0.0] * L
    s = tc.metrics_np([0, 5], t.est_q, t.gt_q, t.est_p, t.gt_p)
    assert s.metrics[0, 1] == s.rmse_d[1:].sum() / 5 and s.metrics[0, 3] == s.l1_d[1:].sum() / 5   # L, not L - 1
    assert s.metrics[0, 0] == s.rmse_d[1] and s.metrics[0, 2] == s.l1_d[1]
    assert s.metrics[0, 4] == s.rt1[1:].sum() / 4
    assert np.isnan(tc.metrics_np([0, 5], t.est_q, t.gt_q).metrics[0, 4])
    # a row that is not finite gives NaN where it enters, and a zero-length step NaN in r_t
    bad = t.est_q.copy()
    bad[2, 1] = np.nan
    s = tc.metrics_np([0, 5], bad, t.gt_q, t.est_p, t.gt_p)
    assert np.isnan(s.metrics[0, :4]).all() and np.isnan(s.angle1[2:4]).all() and np.isfinite(s.angle1[[1, 4]]).all()
    still = t.est_p.copy()
    still[3] = still[2]
    s = tc.metrics_np([0, 5], t.est_q, t.gt_q, still, t.gt_p)
    assert np.isnan(s.rt1[3]) and np.isnan(s.metrics[0, 4]) and np.isfinite(s.metrics[0, :4]).all()


def test_checker_compose_carries_the_pose_over_an_absent_row():
    t = tc.traj(9, 1e-2, 6, 0.05)
    rel_q, rel_t = t.rel_q.copy(), t.rel_t.copy()
    rel_q[3] = np.nan
    rel_t[5, 2] = np.inf
    rel_q[7] = 0.0
    c = tc.compose_np([0, 9], rel_q, rel_t)
    assert c.valid.tolist() == [1, 1, 1, 0, 1, 0, 1, 0, 1]
    for r in (3, 5, 7):
        assert np.array_equal(c.q[r], c.q[r - 1]) and np.array_equal(c.p[r], c.p[r - 1])
    keep = c.valid == 1
    d = tc.compose_np([0, 6], rel_q[keep], rel_t[keep])
    assert np.array_equal(d.q, c.q[keep]) and np.array_equal(d.p, c.p[keep])
    # the left factor, and the first row being a pose itself
    q0 = tc.qnorm(np.array([[0.1, -0.2, 0.3, 0.9]]))
    p0 = np.array([[1.0, 2.0, 3.0]])
    e = tc.compose_np([0, 9], t.rel_q, t.rel_t, q0=q0, p0=p0)
    plain = tc.compose_np([0, 9], t.rel_q, t.rel_t)
    assert np.allclose(tc.sign_aligned_diff(e.q, tc.qmul(q0, plain.q)), 0, atol=tc.bound_compose_q(9))
    assert np.allclose(e.p, p0 + tc.qrot(q0, plain.p), atol=1e-14)
    assert np.allclose(plain.q[0], t.rel_q[0]) and np.allclose(plain.p[0], t.rel_t[0])
    # traj's absolute poses are this product
    assert np.allclose(tc.sign_aligned_diff(plain.q, t.est_q), 0, atol=tc.bound_compose_q(9))


# ------------------------------------------------------------------------------------------ stack_steps, matched, join
def test_stack_steps_and_matched_on_cpu_tensors():
    F, S = 3, 4
    rng = np.random.default_rng(2)
    steps = []
    for s in range(S):
        q = torch.as_tensor(tc.qnorm(rng.normal(size=(F, 4))))
        t = torch.as_tensor(rng.normal(size=(F, 3)))
        if s == 2:
            q[1] = float("nan")
            t[1] = float("nan")
        steps.append(SimpleNamespace(q=q, t=t))
    off, rel_q, rel_t = trajectory.stack_steps(steps)
    assert off.tolist() == [0, 5, 10, 15] and off.dtype == torch.int64
    assert rel_q.shape == (15, 4) and rel_t.shape == (15, 3) and rel_q.is_contiguous()
    for f in range(F):
        assert rel_q[5 * f].tolist() == [0.0, 0.0, 0.0, 1.0] and rel_t[5 * f].tolist() == [0.0, 0.0, 0.0]
        for s in range(S):
            assert torch.equal(rel_q[5 * f + 1 + s].isnan(), steps[s].q[f].isnan())
            if not (s == 2 and f == 1):
                assert torch.equal(rel_q[5 * f + 1 + s], steps[s].q[f]) and torch.equal(rel_t[5 * f + 1 + s], steps[s].t[f])
    with pytest.raises(ValueError):
        trajectory.stack_steps([])
    # matched: the checker's composition stands in for the device's
    c = tc.compose_np(off.numpy(), rel_q.numpy(), rel_t.numpy())
    assert c.valid.tolist() == [1] * 5 + [1, 1, 1, 0, 1] + [1] * 5
    gt_q, gt_p = rng.normal(size=(15, 4)), rng.normal(size=(15, 3))
    for conv in (lambda a: a, torch.as_tensor):
        traj = trajectory.Trajectory(conv(c.q), conv(c.p), conv(c.valid))
        o2, eq, ep, gq, gp = trajectory.matched(conv(off.numpy()), traj, conv(gt_q), conv(gt_p))
        assert np.asarray(o2).tolist() == [0, 5, 9, 14]
        keep = c.valid == 1
        assert np.array_equal(np.asarray(eq), c.q[keep]) and np.array_equal(np.asarray(ep), c.p[keep])
        assert np.array_equal(np.asarray(gq), gt_q[keep]) and np.array_equal(np.asarray(gp), gt_p[keep])
    o2, eq, ep, gq, gp = trajectory.matched(off.numpy(), trajectory.Trajectory(c.q, None, c.valid), gt_q, None)
    assert ep is None and gp is None and len(eq) == 14


def test_the_timestamp_join_of_evaluate(tmp_path):
    # truncated to milliseconds after rounding to microseconds, as datetime.fromtimestamp(...).strftime(...)[:-3] does
    assert evaluate.millisecond_keys([1.0004999, 1.0005001, 2.9999996, 0.0]).tolist() == [1000, 1000, 3000, 0]
    gt_times = np.array([0.0, 0.1036, 0.2072, 0.3108, 0.4144])
    est_times = np.array([0.10364, 0.0, 0.31089, 0.5])   # out of order, one gt frame missing, one est frame unmatched
    ei, gi = evaluate.join_timestamps(est_times, gt_times)
    assert ei.tolist() == [1, 0, 2] and gi.tolist() == [0, 1, 3]
    with pytest.raises(ValueError, match="share"):
        evaluate.join_timestamps([0.1, 0.1000004], gt_times)
    ei, gi = evaluate.join_timestamps([7.0], gt_times)
    assert ei.shape == (0,) and gi.shape == (0,)
    # the files: a KITTI ground truth of 3x4 rows and a pose file
    t = tc.traj(6, 1e-2, 8, 0.05)
    gt = np.concatenate([tc.qmat(t.gt_q), t.gt_p[:, :, None]], axis=2).reshape(6, 12)
    np.savetxt(tmp_path / "gt.txt", gt, fmt="%.17g")
    R, p = evaluate.read_kitti_poses(tmp_path / "gt.txt")
    assert np.array_equal(R, tc.qmat(t.gt_q)) and np.array_equal(p, t.gt_p)
    q = evaluate.rotations_to_quaternions(R)
    assert np.all(tc.sign_aligned_diff(q, t.gt_q) <= 8 * tc.U)
    # the pose correction makes the first estimated pose the first ground-truth pose
    q0, p0 = evaluate.pose_correction(t.gt_q[0], t.gt_p[0], t.rel_q[0], t.rel_t[0])
    c = tc.compose_np([0, 6], t.rel_q, t.rel_t, q0=q0[None], p0=p0[None])
    assert tc.sign_aligned_diff(c.q[:1], t.gt_q[:1])[0] <= 16 * tc.U and np.allclose(c.p[0], t.gt_p[0], atol=1e-15)


# ---------------------------------------------------------------------------------------------- the facade, on the host
def test_facade_argument_handling_and_the_new_call_arrays_lists_under_the_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ builds the host facade, so it is there"
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    san = ["-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    lib_dir = os.path.join(ROOT, "pnec_amd")
    exe = str(tmp_path / "trajectory_host")
    subprocess.run([gxx, *san, "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "pnec_amd", "csrc", "host"),
                    os.path.join(ROOT, "tools", "trajectory_host.cc"), os.path.join(ROOT, "pnec_amd", "csrc", "host", "pnec_host.cc"),
                    "-o", exe, "-L" + lib_dir, "-lpnec_hip", "-Wl,-rpath," + lib_dir], check=True)
    r = subprocess.run([exe], env=env, capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    assert "trajectory host: every case held" in r.stdout and "FAIL" not in r.stdout
    assert sum(line.startswith("ok   ") for line in r.stdout.splitlines()) == 3
    exe = str(tmp_path / "call_arrays_host")
    subprocess.run([gxx, *san, "-I" + os.path.join(ROOT, "pnec_amd", "csrc"), os.path.join(ROOT, "tools", "call_arrays_host.cc"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], env=env, capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "FAIL" not in r.stdout
    for name, optional in (("trajectory_compose(", 5), ("trajectory_metrics(", 3)):
        lines = [line for line in r.stdout.splitlines() if line.startswith("ok   " + name)]
        assert lines and all(f"{optional} optional arrays" in line for line in lines), r.stdout[-2000:]
