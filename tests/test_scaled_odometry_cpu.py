"""Scaled odometry without a GPU: the ABI of pnec_hip_tracks_link and pnec_hip_trajectory_advance (declared, bound,
exported, every refusal in HOST space before a device is touched), the numpy checkers of tests/scaled_odometry_cases.py
against what they must agree with -- link_np against tracks.link_pairs on strictly ascending ids, advance_np against
every status by hand, against the exact sequential product within the header's bound, and against compose_trajectory's
checker -- the Python surface, the host facade's names, and the two new lists of tools/call_arrays_host.cc under the
sanitizers.
"""
import dataclasses
import inspect
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scaled_odometry_cases as sc  # noqa: E402
import trajectory_cases as tc  # noqa: E402

import pnec_amd  # noqa: E402
from pnec_amd import capi  # noqa: E402
from pnec_amd import scaled_odometry as so  # noqa: E402
from pnec_amd import tracks as trk  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pnec_hip_tracks_link", "pnec_hip_trajectory_advance")


# ---- 1: the ABI --------------------------------------------------------------------------------------------------------
def test_both_symbols_are_declared_bound_and_exported_within_abi_8():
    L = capi.lib()
    header = open(os.path.join(ROOT, "include", "pnec_hip.h")).read()
    assert "#define PNEC_HIP_ABI_VERSION 8" in header and capi.ABI_VERSION == 8 and L.pnec_hip_abi_version() == 8
    assert "int pnec_hip_tracks_link(int64_t n_images, const int64_t *cur_offsets, int64_t n_cur, const int64_t *cur_id," in header
    assert "int pnec_hip_trajectory_advance(int device, int64_t n_seq, const double *rel_q, const double *rel_t, const int32_t *count," in header
    for name, n_args in zip(NAMES, (12, 18)):
        assert name in capi.SYMBOLS and len(getattr(L, name).argtypes) == n_args, name
    for k, v in (("MEASURED", 0), ("HELD", 1), ("STARTED", 2), ("ABSENT", 3)):
        assert f"#define PNEC_HIP_TRAJ_{k} {v}" in header and getattr(capi, "TRAJ_" + k) == v
    assert (sc.MEASURED, sc.HELD, sc.STARTED, sc.ABSENT) == (0, 1, 2, 3)
    for words in ("m = a + (b - a) / 2", "12 (L + 2) u", "26 (L + 2) u"):
        assert words in header, words


# ---- 2: refusals ---------------------------------------------------------------------------------------------------------
def _err():
    return (capi.lib().pnec_hip_last_error() or b"").decode()


def test_tracks_link_refuses_bad_arguments_in_host_space_before_a_device_is_touched():
    L = capi.lib()
    co, po = np.array([0, 2], dtype=np.int64), np.array([0, 3], dtype=np.int64)
    ci, pi = np.array([5, 7], dtype=np.int64), np.array([5, 6, 7], dtype=np.int64)
    link, nl = np.full(2, 77, dtype=np.int32), np.full(1, 77, dtype=np.int32)
    d = lambda a: a.ctypes.data
    good = [1, d(co), 2, d(ci), d(po), 3, d(pi), d(link), d(nl), capi.MEM_HOST, 0, None]

    def call(word, **change):
        a = list(good)
        for k, v in change.items():
            a[int(k[1:])] = v
        rc = L.pnec_hip_tracks_link(*a)
        msg = _err()
        assert rc == capi.ERR_INVALID_ARGUMENT == -1, (change, rc, msg)
        assert "tracks_link" in msg and word in msg, msg

    call("n_images", _0=0)
    call("n_images", _0=2 ** 31)
    call("n_cur and n_prev", _2=-1)
    call("n_cur and n_prev", _2=2 ** 31)
    call("n_cur and n_prev", _5=-1)
    call("n_cur and n_prev", _5=2 ** 31)
    call("NULL", _1=None)
    call("NULL", _4=None)
    call("NULL", _7=None)
    call("cur_id or prev_id", _3=None)
    call("cur_id or prev_id", _6=None)
    call("an output is an input", _7=d(ci))          # (the types differ; the pointer is what is compared)
    call("an output is an input", _8=d(po))
    call("same array", _8=d(link))
    call("memory space", _9=7)
    call("memory space", _9=-1)
    # HOST space checks both offset arrays: from 0, non-decreasing, within their rows
    for bad in ([1, 2], [0, 3], [0, -1]):
        call("cur_offsets", _1=d(np.array(bad, dtype=np.int64)))
    for bad in ([1, 3], [0, 4]):
        call("prev_offsets", _4=d(np.array(bad, dtype=np.int64)))
    two = np.array([0, 2, 1], dtype=np.int64)
    call("cur_offsets", _0=2, _1=d(two), _4=d(np.array([0, 1, 3], dtype=np.int64)))
    assert np.all(link == 77) and nl[0] == 77
    # no row: zeros to out_n_linked, success, still no device
    a = list(good)
    a[1], a[2], a[3] = d(np.zeros(2, dtype=np.int64)), 0, None
    assert L.pnec_hip_tracks_link(*a) == 0, _err()
    assert nl[0] == 0 and np.all(link == 77)


def test_trajectory_advance_refuses_bad_arguments_in_host_space_before_a_device_is_touched():
    L = capi.lib()
    n = 2
    f = lambda *shape: np.zeros(shape)
    rq, rt, s3, s, q, p = f(n, 4), f(n, 3), f(n, 3), f(n), f(n, 4), f(n, 3)
    cnt, nu = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    ns, nq, npos = np.full(n, 7.5), np.full((n, 4), 7.5), np.full((n, 3), 7.5)
    st = np.full(n, 9, dtype=np.int32)
    d = lambda a: a.ctypes.data
    good = [0, n, d(rq), d(rt), d(cnt), 0, d(s3), d(nu), 1, d(s), d(q), d(p), d(ns), d(nq), d(npos), d(st), capi.MEM_HOST, None]

    def call(word, **change):
        a = list(good)
        for k, v in change.items():
            a[int(k[1:])] = v
        rc = L.pnec_hip_trajectory_advance(*a)
        msg = _err()
        assert rc == capi.ERR_INVALID_ARGUMENT == -1, (change, rc, msg)
        assert "trajectory_advance" in msg and word in msg, msg

    call("n_seq", _1=0)
    call("n_seq", _1=2 ** 31)
    for i in (2, 3):
        call("rel_q or rel_t", **{f"_{i}": None})
    for i in (9, 10, 11, 12, 13, 14):
        call("state array", **{f"_{i}": None})
    call("min_count", _5=-1)
    call("min_used", _8=0)
    call("n_used needs scale3", _6=None)
    call("also an input", _12=d(s))                  # the state is double-buffered
    call("also an input", _13=d(q))
    call("also an input", _14=d(p))
    call("also an input", _15=d(cnt))
    call("also an input", _13=d(rq))
    call("another output", _14=d(nq))
    call("memory space", _16=5)
    call("memory space", _16=-1)
    assert np.all(ns == 7.5) and np.all(nq == 7.5) and np.all(npos == 7.5) and np.all(st == 9)


# ---- 3: the join ---------------------------------------------------------------------------------------------------------
def test_link_np_is_link_pairs_on_strictly_ascending_ids():
    rng = np.random.default_rng(7)
    sizes = (0, 1, 2, 63, 64, 65)
    seen = dict(first=False, last=False, below=False, between=False, above=False, negative=False, low_word=False)
    for n_prev in sizes:
        for n_cur in sizes:
            prev, cur = sc.id_case(n_prev, n_cur, rng)
            assert len(prev) == n_prev and len(cur) == n_cur
            assert np.all(np.diff(prev) > 0)
            want = trk.link_pairs(prev, cur)
            want[cur < 0] = -1
            got, n_linked = sc.link_np([0, len(cur)], cur, [0, len(prev)], prev)
            assert got.dtype == np.int32 and np.array_equal(got, want), (n_prev, n_cur)
            assert n_linked.tolist() == [int((want >= 0).sum())]
            if n_prev:
                seen["first"] |= bool((got == 0).any())
                seen["last"] |= bool((got == n_prev - 1).any())
                miss = cur[(got < 0) & (cur >= 0)]
                seen["below"] |= bool((miss < prev[0]).any())
                seen["above"] |= bool((miss > prev[-1]).any())
                seen["between"] |= bool(((miss > prev[0]) & (miss < prev[-1])).any())
                low = set((prev & 0xffffffff).tolist())
                seen["low_word"] |= any(int(x) & 0xffffffff in low for x in miss) and len(low) < n_prev
            seen["negative"] |= bool((cur < 0).any())
    assert all(seen.values()), seen
    # the first and the last row by hand, and ids that differ above bit 32 only
    prev = np.array([3, 9, 9 + sc.BIG, 20 + sc.BIG], dtype=np.int64)
    cur = np.array([9 + sc.BIG, 3, 20 + sc.BIG, 9, 20, 3 + sc.BIG, -1, 2, 10, 21 + sc.BIG], dtype=np.int64)
    assert sc.link_np([0, 10], cur, [0, 4], prev)[0].tolist() == [2, 0, 3, 1, -1, -1, -1, -1, -1, -1]
    # ragged: two images, an offsets entry beyond the rows (the cut), padding
    co, ci, po, pi = sc.ragged_sets((3, 65), (5, 64), seed=3, pad_cur=4, pad_prev=2)
    link, nl = sc.link_np(co, ci, po, pi)
    assert np.all(link[co[-1]:] == -1) and nl.sum() == (link >= 0).sum()
    for f in range(2):
        alone, _ = sc.link_np([0, co[f + 1] - co[f]], ci[co[f]:co[f + 1]], [0, po[f + 1] - po[f]], pi[po[f]:po[f + 1]])
        assert np.array_equal(link[co[f]:co[f + 1]], alone)


# ---- 4: every status -------------------------------------------------------------------------------------------------------
def test_advance_np_reaches_every_status_by_each_of_its_causes():
    q = np.array([[0.0, 0.0, 0.0, 2.0]])       # not normalised: the step is rel_q / |rel_q|
    t = np.array([[1.0, 0.0, 0.0]])
    s3 = lambda r: np.array([[0.5 * r, r, 2.0 * r]])
    nan = float("nan")
    fresh = sc.fresh_state(1)
    (s, qq, p), st = sc.advance_np(fresh, q, t, scale3=s3(3.0))
    assert st.tolist() == [sc.STARTED] and s[0] == 1.0 and p.tolist() == [[1.0, 0.0, 0.0]] and qq.tolist() == [[0, 0, 0, 1]]
    state = (s, qq, p)
    (s2, q2, p2), st = sc.advance_np(state, q, t, scale3=s3(3.0), n_used=[4], min_used=4)
    assert st.tolist() == [sc.MEASURED] and s2[0] == 3.0 and p2.tolist() == [[4.0, 0.0, 0.0]]
    held = (dict(scale3=None), dict(scale3=s3(nan)), dict(scale3=s3(0.0)), dict(scale3=s3(-2.0)),
            dict(scale3=s3(np.inf)), dict(scale3=s3(3.0), n_used=[3], min_used=4))
    for kw in held:
        (s2, q2, p2), st = sc.advance_np(state, q, t, **kw)
        assert st.tolist() == [sc.HELD] and s2[0] == 1.0 and p2.tolist() == [[2.0, 0.0, 0.0]], kw
    big = (np.array([1e200]), qq, p)
    (s2, _, _), st = sc.advance_np(big, q, t, scale3=s3(1e200))       # s * r overflows
    assert st.tolist() == [sc.HELD] and s2[0] == 1e200
    tiny = (np.array([1e-200]), qq, p)
    (s2, _, _), st = sc.advance_np(tiny, q, t, scale3=s3(1e-200))     # s * r underflows to 0
    assert st.tolist() == [sc.HELD] and s2[0] == 1e-200
    odd = (np.array([-0.0]), np.array([[0.1, -0.2, 0.3, 0.9]]), np.array([[1.5, -2.5, nan]]))
    absent = (dict(rel_q=np.array([[nan, 0, 0, 1.0]])), dict(rel_q=np.array([[0, 0, np.inf, 1.0]])),
              dict(rel_q=np.zeros((1, 4))), dict(rel_t=np.array([[0.0, nan, 0.0]])), dict(rel_q=np.full((1, 4), 1e200)),
              dict(count=[4], min_count=5))
    for kw in absent:
        for st_in in (state, odd, fresh):
            args = dict(rel_q=q, rel_t=t, scale3=s3(3.0))
            args.update(kw)
            nxt, st = sc.advance_np(st_in, **args)
            assert st.tolist() == [sc.ABSENT], kw
            for a, b in zip(nxt, st_in):
                assert np.asarray(a).tobytes() == np.asarray(b, dtype=np.float64).tobytes(), kw    # the state's bits
    (_, _, _), st = sc.advance_np(state, q, t, count=[5], min_count=5, scale3=s3(3.0))
    assert st.tolist() == [sc.MEASURED]
    # a quarter turn about z, then a step along x: the step is taken in the frame of the state BEFORE the turn
    h = np.sqrt(0.5)
    turn = np.array([[0.0, 0.0, h, h]])
    (s, qq, p), _ = sc.advance_np(fresh, turn, t)
    assert np.allclose(p, [[1, 0, 0]]) and np.allclose(qq, turn)
    (s, qq, p), _ = sc.advance_np((s, qq, p), turn, t, scale3=s3(2.0))
    assert np.allclose(p, [[1, 2, 0]], atol=1e-15) and np.allclose(qq, [[0, 0, 1, 0]], atol=1e-15) and s[0] == 2.0


# ---- 5, 6: the bound, and compose --------------------------------------------------------------------------------------------
def _chain(L, n, seed, dtype=np.float64, statuses=None, **every):
    rel_q, rel_t, s3, n_used, count = sc.random_steps(L, n, seed, **every)
    state = sc.fresh_state(n, dtype)
    out, sts = [], []
    for k in range(L):
        state, st = sc.advance_np(state, rel_q[k], rel_t[k], count[k], 10, s3[k], n_used[k], 4, dtype=dtype,
                                  status=None if statuses is None else statuses[k])
        out.append(state)
        sts.append(st)
    return (rel_q, rel_t), out, np.array(sts)


def test_advance_np_stays_within_the_stated_bound_of_the_exact_sequential_product_over_64_steps():
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63, "the exact form needs a long double of 64 bits of mantissa"
    L, n = 64, 5
    (rel_q, rel_t), got, sts = _chain(L, n, 11, absent_every=9, held_every=7)
    _, exact, _ = _chain(L, n, 11, dtype=np.longdouble, statuses=sts, absent_every=9, held_every=7)
    assert {int(x) for x in sts.ravel()} == {0, 1, 2, 3}
    path = np.zeros(n, dtype=np.longdouble)
    worst_q = worst_p = 0.0
    for k in range(L):
        moved = sts[k] != sc.ABSENT
        path += np.where(moved, exact[k][0] * np.sqrt((np.asarray(rel_t[k], dtype=np.longdouble) ** 2).sum(-1)), 0)
        dq = sc.sign_aligned_diff(got[k][1], exact[k][1])
        dp = np.sqrt(((got[k][2].astype(np.longdouble) - exact[k][2]) ** 2).sum(-1)).astype(np.float64)
        ds = np.abs((got[k][0].astype(np.longdouble) - exact[k][0]) / exact[k][0]).astype(np.float64)
        assert np.all(dq <= sc.bound_advance_q(k + 1)), (k, dq)
        assert np.all(dp <= sc.bound_advance_p(k + 1, path.astype(np.float64))), (k, dp)
        assert np.all(ds <= (k + 1) * tc.U), (k, ds)      # one rounding a measured step
        worst_q = max(worst_q, float((dq / sc.bound_advance_q(k + 1)).max()))
        worst_p = max(worst_p, float((dp / sc.bound_advance_p(k + 1, path.astype(np.float64))).max()))
    print(f"advance_np against long double over {L} steps: |dq| at most {worst_q:.3f} of its bound, |dp| {worst_p:.3f}")


def test_the_recorded_steps_composed_by_the_trajectory_checker_give_the_same_poses():
    L, n = 64, 3
    (rel_q, rel_t), got, sts = _chain(L, n, 12, absent_every=11, held_every=5)
    assert (sts == sc.ABSENT).any()
    for i in range(n):
        s = np.array([got[k][0][i] for k in range(L)])
        rq = rel_q[:, i].copy()
        rq[sts[:, i] == sc.ABSENT] = np.nan       # (compose has no count: what advance skipped is marked not present)
        c = tc.compose_np([0, L], rq, rel_t[:, i], scale=np.where(np.isfinite(s), s, 1.0))
        assert np.array_equal(c.valid == 1, sts[:, i] != sc.ABSENT)
        moved = sts[:, i] != sc.ABSENT
        path = np.cumsum(np.where(moved, np.abs(s) * np.linalg.norm(rel_t[:, i], axis=1), 0.0))
        for k in range(L):
            if not np.isfinite(got[k][0][i]):      # before the sequence's first pair both hold the start pose
                assert np.array_equal(c.q[k], [0, 0, 0, 1]) and np.array_equal(got[k][1][i], [0, 0, 0, 1])
                continue
            dq = sc.sign_aligned_diff(got[k][1][i], c.q[k])
            dp = np.linalg.norm(got[k][2][i] - c.p[k])
            assert dq <= sc.bound_advance_q(k + 1) + tc.bound_compose_q(k + 1), (i, k, dq)
            assert dp <= sc.bound_advance_p(k + 1, path[k]) + tc.bound_compose_p(k + 1, path[k]), (i, k, dp)


# ---- 7, 8: the Python surface and the facade -----------------------------------------------------------------------------------
def test_python_names_defaults_and_fields():
    names = {"ScaledOdometry", "ScaledOdometryResult", "TrajectoryState", "link_tracks", "new_trajectory_state", "advance_trajectory"}
    assert names <= set(pnec_amd.__all__) and all(getattr(pnec_amd, k) is getattr(so, k) for k in names)
    assert [f.name for f in dataclasses.fields(so.TrajectoryState)] == ["s", "q", "p"]
    assert [f.name for f in dataclasses.fields(so.ScaledOdometryResult)] == [
        "step", "t_oriented", "scale", "ratio3", "n_linked", "n_used", "abs_q", "abs_p", "status"]
    sig = inspect.signature(so.link_tracks)
    assert list(sig.parameters) == ["cur_offsets", "cur_id", "prev_offsets", "prev_id", "out", "n_linked"]
    assert sig.parameters["out"].default is None and sig.parameters["n_linked"].default is None
    sig = inspect.signature(so.advance_trajectory)
    assert [(k, v.default) for k, v in sig.parameters.items()][3:] == [
        ("count", None), ("min_count", 0), ("scale3", None), ("n_used", None), ("min_used", 1), ("out", None)]
    assert list(sig.parameters)[:3] == ["state", "rel_q", "rel_t"]
    assert list(inspect.signature(so.new_trajectory_state).parameters) == ["n", "on_device", "device"]
    st = so.new_trajectory_state(3, False)
    assert np.isnan(st.s).all() and st.q.tolist() == [[0, 0, 0, 1]] * 3 and st.p.tolist() == [[0, 0, 0]] * 3
    assert issubclass(so.ScaledOdometry, pnec_amd.Odometry)
    sig = inspect.signature(so.ScaledOdometry.__init__)
    base = inspect.signature(pnec_amd.Odometry.__init__)
    own = {"min_parallax": 0.0, "min_links": 1, "min_corr": 0}
    for k, v in own.items():
        assert sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[k].default == v
    positional = lambda s: [k for k, v in s.parameters.items() if v.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD]
    assert positional(sig) == positional(base)
    # keyframe pairs are refused before anything is allocated (no device here: an allocation would fail otherwise)
    with pytest.raises(ValueError, match="keyframe"):
        so.ScaledOdometry(3, 96, 128, np.eye(3), min_displacement=5.0)
    with pytest.raises(ValueError, match="min_links"):
        so.ScaledOdometry(3, 96, 128, np.eye(3), min_links=0)


def test_facade_declarations_and_pybind_names():
    facade = open(os.path.join(ROOT, "pnec_amd", "csrc", "host", "pnec_host.h")).read()
    assert "std::vector<int32_t> LinkTracks(const std::vector<int64_t> &prev_ids, const std::vector<int64_t> &cur_ids);" in facade
    assert "std::vector<int32_t> AdvanceTrajectory(const TrajectoryState &state," in facade and "struct TrajectoryState {" in facade
    with open(os.path.join(ROOT, "pnec_amd", "libpnec_host.so"), "rb") as f:
        blob = f.read()
    assert b"LinkTracks" in blob and b"AdvanceTrajectory" in blob
    import pnec_amd.pypnec as pypnec
    assert "link_tracks" in dir(pypnec) and "advance_trajectory" in dir(pypnec)


# ---- 9: the staging lists -----------------------------------------------------------------------------------------------------
def test_the_two_new_lists_are_counted_under_the_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ builds the host facade, so it is there"
    exe = str(tmp_path / "call_arrays_host")
    subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "pnec_amd", "csrc"),
                    os.path.join(ROOT, "tools", "call_arrays_host.cc"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "FAIL" not in r.stdout
    lines = r.stdout.splitlines()
    for name in ("tracks_link", "trajectory_advance"):
        assert any(line.startswith("ok   " + name + "(") for line in lines), name


# ---- the geometry of the GPU test's scale recovery, on the numpy yardstick first ---------------------------------------------
def test_the_recovery_scene_gives_the_true_scale_and_path_through_the_numpy_checkers():
    from test_relative_scale_cpu import link_tolerance, relative_scale_np
    seqs = sc.recovery_sequences()
    F = len(seqs)
    state = sc.fresh_state(F)
    tol = np.zeros(F)
    prev = None
    for k in range(4):
        off, ids, f1, f2, q, t = sc.recovery_pair(seqs, k)
        s3, n_used = None, None
        if prev is not None:
            link, n_linked = sc.link_np(off, ids, prev[0], prev[1])
            assert np.all(n_linked > 0.5 * np.diff(off)) and np.all(n_linked < np.diff(off))      # most tracks, not all
            s3, n_used = np.zeros((F, 3)), np.zeros(F, dtype=np.int32)
            for f in range(F):
                a, b, pa, pb = off[f], off[f + 1], prev[0][f], prev[0][f + 1]
                ref = relative_scale_np(f1[a:b], f2[a:b], q[f], t[f], prev[2][pa:pb], prev[3][pa:pb], prev[4][f], prev[5][f],
                                        link[a:b], sc.RECOVERY_MIN_PARALLAX)
                s3[f], n_used[f] = ref["scale"], ref["n_used"]
                assert ref["n_used"] >= 20, (k, f, ref["n_used"])
                tol[f] += float(np.max(link_tolerance(ref)[ref["used"] == 1]))
        state, status = sc.advance_np(state, q, t, scale3=s3, n_used=n_used, min_used=20)
        assert status.tolist() == [sc.STARTED if k == 0 else sc.MEASURED] * F, (k, status)
        for f, s in enumerate(seqs):
            assert abs(state[0][f] - s.b[k] / s.b[0]) <= tol[f] * s.b[k] / s.b[0] + 4 * tc.U, (k, f)
            path = s.path[k] / s.b[0]
            assert np.linalg.norm(state[2][f] - s.abs_p[k] / s.b[0]) <= tol[f] * path + sc.bound_advance_p(k + 1, path) + \
                1e-15 * path, (k, f)      # (1e-15: the truth's own float64 composition)
            R = tc.qmat(state[1][f])
            assert np.abs(R - s.abs_R[k]).max() <= 1e-14
        prev = (off, ids, f1, f2, q, t)
    assert tol.max() < 1e-8
    print("recovery scene: summed ratio tolerance per sequence", tol)
