"""Scaled odometry on the device: pnec_hip_tracks_link against the literal bisection, exactly;
pnec_hip_trajectory_advance against its numpy checkers; the scale of exact geometry recovered through link_tracks,
relative_scale and advance_trajectory; and pnec_amd.ScaledOdometry held, BITWISE and at every step, to the pieces it is
made of -- a plain Odometry on the same images, then everything read back: tracks.link_pairs, Batch.triangulate and
Batch.relative_scale on exact batches, advance_trajectory on those."""
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scaled_odometry_cases as sc  # noqa: E402
import trajectory_cases as tc  # noqa: E402
from test_patch_track_cpu import H0, LEVELS, W0  # noqa: E402
from test_relative_scale_cpu import REL_TOL  # noqa: E402
from test_tracks_cpu import SEQ_CAPACITY, SEQ_EDGE, SEQ_F, SEQ_GRID, _warped  # noqa: E402

from pnec_amd import (Batch, Odometry, ScaledOdometry, TrajectoryState, advance_trajectory, capi, link_tracks,  # noqa: E402
                      new_trajectory_state)
from pnec_amd import tracks as trk  # noqa: E402

pytestmark = pytest.mark.gpu

K = np.array([[110.0, 0.0, 63.5], [0.0, 110.0, 47.5], [0.0, 0.0, 1.0]])      # tests/test_odometry_gpu.py's camera
K_INV = np.linalg.inv(K)
# ring 4: a track lives for two steps after its birth, so consecutive pairs share tracks (with the fixture's ring of 3 a
# track is in one pair only and nothing could ever be linked)
TRACKER = dict(levels=LEVELS, ring=4, grid=SEQ_GRID, capacity=SEQ_CAPACITY, edge=SEQ_EDGE)
N_FRAMES = 6
MIN_CORR, MIN_LINKS = 1, 1


def _torch():
    import torch
    return torch


def _dev(a):
    return _torch().as_tensor(np.ascontiguousarray(a), device="cuda:0")


def _host(a):
    return np.ascontiguousarray(a.cpu().numpy())


def _same_bits(a, b, what):
    a = _host(a) if hasattr(a, "cpu") else np.ascontiguousarray(a)
    b = _host(b) if hasattr(b, "cpu") else np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"{what}: bits differ"


# ---- 1: tracks_link -----------------------------------------------------------------------------------------------------------
def _link_both_spaces(co, ci, po, pi):
    torch = _torch()
    h_link, h_n = link_tracks(co, ci, po, pi)
    d_link, d_n = link_tracks(_dev(co), _dev(ci), _dev(po), _dev(pi))
    torch.cuda.synchronize()
    assert d_link.is_cuda and d_link.dtype == torch.int32 and h_link.dtype == np.int32
    _same_bits(d_link, h_link, "link: DEVICE against HOST")
    _same_bits(d_n, h_n, "n_linked: DEVICE against HOST")
    return h_link, h_n


def test_tracks_link_is_the_bisection_exactly_in_both_spaces():
    sizes = sc.LINK_SIZES
    # one image: every count on either side
    for n_prev in sizes:
        for n_cur in sizes:
            co, ci, po, pi = sc.ragged_sets((n_prev,), (n_cur,), seed=100 + 7 * n_prev + n_cur, pad_cur=3, pad_prev=2)
            want, want_n = sc.link_np(co, ci, po, pi)
            got, got_n = _link_both_spaces(co, ci, po, pi)
            assert np.array_equal(got, want) and np.array_equal(got_n, want_n), (n_prev, n_cur)
            assert np.all(got[co[-1]:] == -1) and got_n[0] == (got[:co[-1]] >= 0).sum()
    # three images: counts drawn from the list, an empty image on either side among them
    rng = np.random.default_rng(5)
    draws = [((0, 65, 257), (64, 0, 63)), ((257, 1, 2), (257, 65, 1))] + \
        [(tuple(rng.choice(sizes, 3)), tuple(rng.choice(sizes, 3))) for _ in range(4)]
    linked_total = 0
    for n, (sp, scur) in enumerate(draws):
        co, ci, po, pi = sc.ragged_sets(sp, scur, seed=200 + n, pad_cur=5, pad_prev=4)
        want, want_n = sc.link_np(co, ci, po, pi)
        got, got_n = _link_both_spaces(co, ci, po, pi)
        assert np.array_equal(got, want) and np.array_equal(got_n, want_n), (sp, scur)
        assert np.all(got[co[-1]:] == -1), "padding is written, up to n_cur"
        linked_total += int(got_n.sum())
        for f in range(3):
            assert got_n[f] == (got[co[f]:co[f + 1]] >= 0).sum()
            # the image alone: a call that holds nothing else
            alone, alone_n = link_tracks(_dev(np.array([0, co[f + 1] - co[f]])), _dev(ci[co[f]:co[f + 1]]),
                                         _dev(np.array([0, po[f + 1] - po[f]])), _dev(pi[po[f]:po[f + 1]]))
            assert np.array_equal(_host(alone), got[co[f]:co[f + 1]]) and int(alone_n[0]) == got_n[f], (sp, scur, f)
    assert linked_total > 100
    # the cut: offsets that run beyond the rows on either side (DEVICE space checks nothing: it clamps)
    co, ci, po, pi = sc.ragged_sets((65, 257, 64), (63, 257, 65), seed=300)
    co2, po2 = co.copy(), po.copy()
    co2[-1] += 40
    po2[-1] += 9
    n_cur, n_prev = len(ci) - 20, len(pi) - 30                    # ... and rows that end inside the last image
    want, want_n = sc.link_np(co2, ci[:n_cur], po2, pi[:n_prev])
    out = _torch().full((n_cur + 8,), 55, dtype=_torch().int32, device="cuda:0")
    got, got_n = link_tracks(_dev(co2), _dev(ci[:n_cur]), _dev(po2), _dev(pi[:n_prev]), out=out[:n_cur])
    assert np.array_equal(_host(got), want) and np.array_equal(_host(got_n), want_n)
    assert np.all(_host(out[n_cur:]) == 55), "nothing is written beyond n_cur"
    assert want_n[2] < sc.link_np(co, ci, po, pi)[1][2], "the cut took links away"
    # offsets from beyond the rows altogether, and a negative one
    co3 = np.array([-5, 10, n_cur + 3, n_cur + 90], dtype=np.int64)
    want, want_n = sc.link_np(co3, ci[:n_cur], po, pi)
    got, got_n = link_tracks(_dev(co3), _dev(ci[:n_cur]), _dev(po), _dev(pi))
    assert np.array_equal(_host(got), want) and np.array_equal(_host(got_n), want_n)
    # no rows at all
    got, got_n = link_tracks(_dev(np.zeros(4, dtype=np.int64)), _dev(np.zeros(0, dtype=np.int64)), _dev(po), _dev(pi))
    assert tuple(got.shape) == (0,) and _host(got_n).tolist() == [0, 0, 0]


# ---- 2: trajectory_advance ------------------------------------------------------------------------------------------------------
def _state_np(st):
    return tuple(_host(a) for a in (st.s, st.q, st.p))


@pytest.mark.parametrize("n_seq", [1, 63, 64, 65])
def test_trajectory_advance_follows_its_checkers_over_a_chain_of_64_calls(n_seq):
    torch = _torch()
    L = 64
    rel_q, rel_t, s3, n_used, count = sc.random_steps(L, n_seq, 40 + n_seq, absent_every=9, held_every=7)
    dev = new_trajectory_state(n_seq, True, torch.device("cuda:0"))
    host = new_trajectory_state(n_seq, False)
    exact = sc.fresh_state(n_seq, np.longdouble)
    path = np.zeros(n_seq, dtype=np.longdouble)
    seen, same_as_np, worst_q, worst_p = set(), True, 0.0, 0.0
    for k in range(L):
        before = _state_np(dev)
        want_status = sc.decide_np(before[0], rel_q[k], rel_t[k], count[k], 10, s3[k], n_used[k], 4)
        np_next, _ = sc.advance_np(before, rel_q[k], rel_t[k], count[k], 10, s3[k], n_used[k], 4)
        dev, d_status = advance_trajectory(dev, _dev(rel_q[k]), _dev(rel_t[k]), _dev(count[k]), 10, _dev(s3[k]),
                                           _dev(n_used[k]), 4)
        host, h_status = advance_trajectory(host, rel_q[k], rel_t[k], count[k], 10, s3[k], n_used[k], 4)
        exact, _ = sc.advance_np(exact, rel_q[k], rel_t[k], scale3=s3[k], dtype=np.longdouble, status=want_status)
        after = _state_np(dev)
        assert np.array_equal(_host(d_status), want_status), k
        _same_bits(d_status, h_status, f"step {k}: status, DEVICE against HOST")
        for name, a, b in zip("sqp", after, (host.s, host.q, host.p)):
            _same_bits(a, b, f"step {k}: {name}, DEVICE against HOST")
        gone = want_status == sc.ABSENT
        for a, b in zip(after, before):
            assert np.array_equal(a[gone].view(np.uint8), b[gone].view(np.uint8)), f"step {k}: an absent pair keeps the state's bits"
        same_as_np &= all(np.array_equal(a.view(np.uint8), np.ascontiguousarray(b).view(np.uint8)) for a, b in zip(after, np_next))
        path += np.where(gone, 0, exact[0] * np.sqrt((np.asarray(rel_t[k], dtype=np.longdouble) ** 2).sum(-1)))
        started = np.isfinite(after[0])
        dq = sc.sign_aligned_diff(after[1], exact[1])
        dp = np.sqrt(((after[2].astype(np.longdouble) - exact[2]) ** 2).sum(-1)).astype(np.float64)
        ds = np.abs((after[0].astype(np.longdouble) - exact[0])[started] / exact[0][started]).astype(np.float64)
        assert np.all(dq <= sc.bound_advance_q(k + 1)), (k, dq.max())
        assert np.all(dp <= sc.bound_advance_p(k + 1, path.astype(np.float64))), (k, dp.max())
        assert np.all(ds <= (k + 1) * tc.U), (k, ds)
        assert np.array_equal(np.isnan(after[0]), np.isnan(exact[0].astype(np.float64)))
        worst_q = max(worst_q, float(dq.max() / sc.bound_advance_q(k + 1)))
        worst_p = max(worst_p, float(np.max(dp[started] / sc.bound_advance_p(k + 1, path.astype(np.float64))[started], initial=0.0)))
        seen |= {int(x) for x in want_status}
    print(f"n_seq {n_seq}: |dq| at most {worst_q:.4f} of its bound, |dp| {worst_p:.4f}; bits equal advance_np's: {same_as_np}")
    assert seen == {0, 1, 2, 3} or n_seq == 1, seen
    if n_seq == 1:
        assert {sc.STARTED, sc.MEASURED, sc.ABSENT} <= seen, seen


def test_every_cause_of_held_and_absent_on_the_device():
    q = np.array([[0.0, 0.0, 0.0, 2.0]])
    t = np.array([[1.0, 0.0, 0.0]])
    s3 = lambda r: np.array([[0.5 * r, r, 2.0 * r]])
    nan = float("nan")
    cases = []     # (state s, kwargs)
    for kw in (dict(), dict(scale3=s3(nan)), dict(scale3=s3(0.0)), dict(scale3=s3(-2.0)), dict(scale3=s3(np.inf)),
               dict(scale3=s3(3.0), n_used=np.array([3], dtype=np.int32), min_used=4), dict(scale3=s3(3.0))):
        cases.append((1.0, dict(rel_q=q, rel_t=t, **kw)))
    cases.append((nan, dict(rel_q=q, rel_t=t, scale3=s3(3.0))))        # a fresh scale starts at 1 whatever the ratio
    cases.append((-1.0, dict(rel_q=q, rel_t=t)))
    cases.append((1e200, dict(rel_q=q, rel_t=t, scale3=s3(1e200))))
    cases.append((1e-200, dict(rel_q=q, rel_t=t, scale3=s3(1e-200))))
    for kw in (dict(rel_q=np.array([[nan, 0, 0, 1.0]])), dict(rel_q=np.zeros((1, 4))), dict(rel_t=np.array([[0.0, nan, 0.0]])),
               dict(rel_q=np.full((1, 4), 1e200)), dict(count=np.array([4], dtype=np.int32), min_count=5)):
        args = dict(rel_q=q, rel_t=t, scale3=s3(3.0))
        args.update(kw)
        cases.append((1.0, args))
        cases.append((nan, args))
    seen = set()
    for s0, kw in cases:
        state = (np.array([s0]), np.array([[0.1, -0.2, 0.3, 0.9]]) / np.sqrt(0.95), np.array([[1.5, -2.5, 0.25]]))
        want, want_status = sc.advance_np(state, **kw)
        dkw = {k: (_dev(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
        got, status = advance_trajectory(TrajectoryState(*(_dev(a) for a in state)), **dkw)
        assert _host(status).tolist() == want_status.tolist(), (s0, kw)
        for a, b in zip((got.s, got.q, got.p), want):
            assert np.allclose(_host(a), b, rtol=0, atol=1e-15 * max(1.0, abs(s0)) if np.isfinite(s0) else 1e-15, equal_nan=True)
        if want_status[0] == sc.ABSENT:
            for a, b in zip((got.s, got.q, got.p), state):
                _same_bits(a, b, "an absent pair keeps the state's bits")
        seen.add(int(want_status[0]))
    assert seen == {0, 1, 2, 3}


# ---- 3: the scale is recovered ----------------------------------------------------------------------------------------------------
def test_scale_and_path_of_exact_geometry_are_recovered_through_link_relative_scale_and_advance():
    torch = _torch()
    seqs = sc.recovery_sequences()
    F = len(seqs)
    state = new_trajectory_state(F, True, torch.device("cuda:0"))
    prev_pair = _dev(np.arange(F, dtype=np.int64))
    tol = np.zeros(F)
    prev = None
    batches = []
    for k in range(4):
        off, ids, f1, f2, q, t = sc.recovery_pair(seqs, k)
        b = Batch(capi.MODE_NEC, off)
        b.fill(_dev(f1), _dev(f2), None)
        batches.append(b)
        dq, dt = _dev(q), _dev(t)
        s3 = n_used = None
        if prev is not None:
            link, n_linked = link_tracks(_dev(off), _dev(ids), _dev(prev[0]), _dev(prev[1]))
            assert np.array_equal(_host(link), sc.link_np(off, ids, prev[0], prev[1])[0])
            rs = b.relative_scale(prev[2], prev_pair, link, dq, dt, prev[3], prev[4], min_parallax=sc.RECOVERY_MIN_PARALLAX)
            s3, n_used = torch.stack([rs.q25, rs.scale, rs.q75], dim=1).contiguous(), rs.n_used
            _same_bits(rs.n_linked, n_linked, "relative_scale counts the links link_tracks made")
            # the tolerance of a step: the noise-free ratio tolerance of tests/test_relative_scale_cpu.py, REL_TOL per
            # depth over its sin^2 psi, of the worst link that passed the gate: sin^2 psi >= sin^2(min_parallax) each side
            tol += 2.0 * REL_TOL / np.sin(sc.RECOVERY_MIN_PARALLAX) ** 2
        state, status = advance_trajectory(state, dq, dt, scale3=s3, n_used=n_used, min_used=20)
        got_status = _host(status).tolist()
        print(f"pair {k}: status {got_status}, scale {_host(state.s).tolist()}, n_used {None if n_used is None else _host(n_used).tolist()}")
        assert got_status == [sc.STARTED if k == 0 else sc.MEASURED] * F, (k, got_status)
        s, aq, ap = _state_np(state)
        for f, seq in enumerate(seqs):
            truth = seq.b[k] / seq.b[0]
            assert abs(s[f] - truth) <= tol[f] * truth + 4 * tc.U, (k, f, s[f], truth)
            path = seq.path[k] / seq.b[0]
            assert np.linalg.norm(ap[f] - seq.abs_p[k] / seq.b[0]) <= tol[f] * path + sc.bound_advance_p(k + 1, path) + 1e-15 * path, (k, f)
            assert np.abs(tc.qmat(aq[f]) - seq.abs_R[k]).max() <= 1e-14
        prev = (off, ids, b, dq, dt)
    torch.cuda.synchronize()
    for b in batches:
        b.close()


# ---- 4 .. 6: ScaledOdometry ---------------------------------------------------------------------------------------------------------
def _frames():
    """six frames of tests/test_tracks_cpu.py's generator for three sequences; sequence 2's frame 1 is blank altogether (the
    pairs into and out of it hold nothing), sequence 0's frame 1 in a region"""
    frames = []
    for n in range(N_FRAMES):
        img = np.stack([_warped(300 + f, n) for f in range(SEQ_F)])
        if n == 1:
            img[0, 20:70, 60:110] = 0.0
            img[2] = 0.0
        frames.append(_torch().from_numpy(np.round(img).astype(np.uint8)).cuda())
    return frames


def _exact_batch(pairs):
    """the pair's rows read back and filled into an exact batch: (batch, offsets, ids)"""
    off = _host(pairs.offsets)
    n = int(off[-1])
    b = Batch(capi.MODE_TARGET, off)
    if n > 0:
        b.fill_keypoints(_host(pairs.prev_pts)[:n], _host(pairs.pts)[:n], _host(pairs.cov)[:n], K_inv=K_INV)
    return b, off, _host(pairs.id)[:n]


def _make(**kw):
    return ScaledOdometry(SEQ_F, H0, W0, K_INV, min_corr=MIN_CORR, min_links=MIN_LINKS, **TRACKER, **kw)


def test_scaled_odometry_equals_its_pieces_bitwise_at_every_step():
    torch = _torch()
    frames = _frames()
    sco, odo = _make(), Odometry(SEQ_F, H0, W0, K_INV, **TRACKER)
    assert sco.process(frames[0]) is None and odo.process(frames[0]) is None
    F = SEQ_F
    state = new_trajectory_state(F, True, torch.device("cuda:0"))
    prev = None                  # (batch, offsets, ids, q, t_oriented) of the previous pair
    linked_seen = absent_seen = measured_seen = False
    identity = _dev(np.array([[0.0, 0.0, 0.0, 1.0]] * F))
    for n in range(1, N_FRAMES):
        out, want = sco.process(frames[n]), odo.process(frames[n])
        for k in ("q", "t", "n_corr", "init_q"):
            _same_bits(getattr(out.step, k), getattr(want, k), f"frame {n}: step.{k}")
        for k in ("offsets", "id", "prev_pts", "pts", "cov"):
            _same_bits(getattr(out.step.pairs, k), getattr(want.pairs, k), f"frame {n}: step.pairs.{k}")
        # the manual route: everything read back, exact batches
        b, off, ids = _exact_batch(want.pairs)
        tri = b.triangulate(want.q, want.t)
        _same_bits(out.t_oriented, tri.t, f"frame {n}: t_oriented")
        link = np.full(int(off[-1]), -1, dtype=np.int32)
        if prev is None:
            pb, pp, pq, pt = b, np.full(F, -1, dtype=np.int64), identity, torch.zeros((F, 3), dtype=torch.float64, device="cuda:0")
        else:
            pb, poff, pids, pq, pt = prev
            pp = np.arange(F, dtype=np.int64)
            for f in range(F):
                link[off[f]:off[f + 1]] = trk.link_pairs(pids[poff[f]:poff[f + 1]], ids[off[f]:off[f + 1]])
        rs = b.relative_scale(pb, pp, link, want.q, tri.t, pq, pt, min_parallax=0.0)
        ratio3 = torch.stack([rs.q25, rs.scale, rs.q75], dim=1).contiguous()
        _same_bits(out.n_linked, rs.n_linked, f"frame {n}: n_linked")
        _same_bits(out.n_used, rs.n_used, f"frame {n}: n_used")
        _same_bits(out.ratio3, ratio3, f"frame {n}: ratio3")
        assert _host(rs.n_linked).tolist() == [int((link[off[f]:off[f + 1]] >= 0).sum()) for f in range(F)]
        state, status = advance_trajectory(state, want.q, tri.t, count=want.n_corr, min_count=MIN_CORR, scale3=ratio3,
                                           n_used=rs.n_used, min_used=MIN_LINKS)
        _same_bits(out.status, status, f"frame {n}: status")
        _same_bits(out.scale, state.s, f"frame {n}: scale")
        _same_bits(out.abs_q, state.q, f"frame {n}: abs_q")
        _same_bits(out.abs_p, state.p, f"frame {n}: abs_p")
        st, cnt = _host(status), _host(want.n_corr)
        print(f"frame {n}: n_corr {cnt.tolist()}, n_linked {_host(rs.n_linked).tolist()}, n_used {_host(rs.n_used).tolist()}, "
              f"status {[capi.TRAJ_NAMES[int(x)] for x in st]}, scale {_host(state.s).tolist()}")
        assert np.all(st[cnt < MIN_CORR] == capi.TRAJ_ABSENT)
        linked_seen |= bool((_host(rs.n_linked) > 0).any())
        absent_seen |= bool(st[2] == capi.TRAJ_ABSENT) if n in (1, 2) else False
        measured_seen |= bool((st == capi.TRAJ_MEASURED).any())
        if n in (1, 2):
            assert cnt[2] == 0 and st[2] == capi.TRAJ_ABSENT, "the blank frame leaves its two pairs empty: ABSENT"
        if prev is not None and prev[0] is not b:
            prev[0].close()
        prev = (b, off, ids, want.q, tri.t)
    torch.cuda.synchronize()
    print("a ratio was MEASURED on the warped images:", measured_seen)
    assert linked_seen, "no pair shared a track with the pair before it: the comparison would be vacuous"
    assert absent_seen, "the blank frame must give ABSENT"
    # a sequence whose first two pairs were absent starts with its third: the state stayed fresh until then
    prev[0].close()
    sco.close()
    odo.close()


def test_no_step_allocates_in_the_library_after_the_second_pair():
    from pnec_amd.multi import alloc_counters
    torch = _torch()
    frames = _frames()
    sco = _make()
    for n in range(3):
        sco.process(frames[n])
    torch.cuda.synchronize()
    a0 = alloc_counters()
    for n in range(3, N_FRAMES):
        sco.process(frames[n])
    torch.cuda.synchronize()
    assert alloc_counters()["hip_malloc_calls"] == a0["hip_malloc_calls"]
    sco.close()


RESULT_FIELDS = ("t_oriented", "scale", "ratio3", "n_linked", "n_used", "abs_q", "abs_p", "status")


def test_process_returns_while_a_delay_queued_before_it_still_runs():
    from test_stream_order_gpu import DELAY_MS, _delay
    torch = _torch()
    frames = _frames()
    ref = _make()
    for n in range(4):
        want = ref.process(frames[n])
    want = [getattr(want, k).clone() for k in RESULT_FIELDS] + [want.step.q.clone(), want.step.t.clone()]
    sco = _make()
    for n in range(3):
        sco.process(frames[n])
    torch.cuda.synchronize()
    _delay(0)
    S = torch.cuda.Stream()
    with torch.cuda.stream(S):
        _delay(DELAY_MS)
        gate = torch.cuda.Event()
        gate.record()
        t0 = time.perf_counter()
        out = sco.process(frames[3])
        host_ms = (time.perf_counter() - t0) * 1e3
        returned_early = not gate.query()
    S.synchronize()
    print(f"ScaledOdometry.process: host side {host_ms:.3f} ms, returned_early={returned_early}")
    got = [getattr(out, k) for k in RESULT_FIELDS] + [out.step.q, out.step.t]
    for name, a, b in zip(RESULT_FIELDS + ("step.q", "step.t"), got, want):
        _same_bits(a, b, name)
    assert returned_early, f"process returned only after the work queued ahead of it had run ({host_ms:.1f} ms on the host)"
    ref.close()
    sco.close()


# ---- 7: a stream that is not the default one ------------------------------------------------------------------------------------------
def test_both_calls_give_the_same_bits_on_a_non_default_stream():
    torch = _torch()
    co, ci, po, pi = sc.ragged_sets((65, 257, 64), (63, 257, 65), seed=9, pad_cur=6)
    rel_q, rel_t, s3, n_used, count = sc.random_steps(3, 65, 77, absent_every=5, held_every=3)
    dev = torch.device("cuda:0")

    def run():
        link, n_linked = link_tracks(_dev(co), _dev(ci), _dev(po), _dev(pi))
        state, outs = new_trajectory_state(65, True, dev), []
        for k in range(3):
            state, status = advance_trajectory(state, _dev(rel_q[k]), _dev(rel_t[k]), _dev(count[k]), 10, _dev(s3[k]),
                                               _dev(n_used[k]), 4)
            outs.append(status)
        return [link, n_linked, state.s, state.q, state.p] + outs
    want = run()
    torch.cuda.synchronize()
    S = torch.cuda.Stream()
    with torch.cuda.stream(S):
        got = run()
    S.synchronize()
    for i, (a, b) in enumerate(zip(got, want)):
        _same_bits(a, b, f"output {i} on a side stream")
    assert np.array_equal(_host(want[0]), sc.link_np(co, ci, po, pi)[0])
