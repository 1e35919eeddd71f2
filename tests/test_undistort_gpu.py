"""pnec_hip_undistort_keypoints on the device against the numpy checker of tests/undistort_cases.py.

The checker restates the header's six steps operation by operation, in float64 and in numpy.longdouble
(test_undistort_cpu.py measures its own properties).  Parity: statuses equal everywhere; a coordinate within
max(4 * D, 8 ulp of the coordinate) of the float64 checker, where D is the worst distance of the float64 checker from the
longdouble one on the same inputs -- four times because a device compiler may reorder roundings in a contraction that
does not amplify them; this kernel forms no fused multiply-add, so the factors printed are expected to be 0.  Everything
else is held bitwise: copies, in place against out of place, HOST against DEVICE space, a row alone against the same row
anywhere in a batch, partial calls against the full one.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import undistort_cases as uc  # noqa: E402

import pnec_amd  # noqa: E402
from pnec_amd import Undistorted, capi, undistort_keypoints  # noqa: E402

pytestmark = pytest.mark.gpu

FLAGS = (0, uc.NEWTON, uc.PROPAGATE_COV, uc.NEWTON | uc.PROPAGATE_COV)
SIZES = (0, 1, 63, 64, 65, 257)


def _torch():
    import torch
    return torch


def _dev(a):
    return None if a is None else _torch().from_numpy(np.ascontiguousarray(a)).cuda()


def _np(u):
    f = lambda a: None if a is None else np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a)
    return Undistorted(*(f(getattr(u, k)) for k in ("pts1", "pts2", "cov2", "cov1", "status1", "status2")))


def device(cam, pts1, pts2=None, cov2=None, cov1=None, flags=0, **kw):
    u = undistort_keypoints(_dev(cam), _dev(pts1), _dev(pts2), _dev(cov2), _dev(cov1), newton=bool(flags & uc.NEWTON),
                            propagate_cov=bool(flags & uc.PROPAGATE_COV), **kw)
    _torch().cuda.synchronize()
    return _np(u)


def _bits(a, b, what):
    assert (a is None) == (b is None), what
    if a is None:
        return
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"{what}: bits differ"


def _all_bits(a, b, what, keys=("pts1", "pts2", "cov2", "cov1", "status1", "status2")):
    for k in keys:
        _bits(getattr(a, k), getattr(b, k), f"{what}: {k}")


def _ulp(x):
    return np.spacing(np.abs(np.where(np.isfinite(x), x, 1.0)))


def _compare(got, got_status, want64, wantld, keep, what):
    """-> the factor |device - float64| / D over the kept points; asserts the tolerance of the module docstring"""
    assert np.array_equal(got_status[keep], want64.status[keep]), f"{what}: statuses differ"
    factors = []
    for g, w, l in ((got, want64.pts, wantld.pts),) if want64.cov is None else \
            ((got[0], want64.pts, wantld.pts), (got[1], want64.cov, wantld.cov)):
        g, w, l = g[keep], w[keep], l[keep]
        assert np.array_equal(np.isnan(g), np.isnan(w)), f"{what}: NaN where the checker has none (or the reverse)"
        fin = ~np.isnan(w)
        D = float(np.max(np.abs(w.astype(np.longdouble) - l)[fin], initial=0.0))
        err = np.abs(g - w)[fin]
        tol = np.maximum(4.0 * D, 8.0 * _ulp(w[fin]))
        assert np.all(err <= tol), f"{what}: worst {float(err.max()):.3e} against {float(tol[np.argmax(err - tol)]):.3e}"
        factors.append(float(err.max(initial=0.0)) / D if D > 0 else float(err.max(initial=0.0) > 0))
    return max(factors)


# ---------------------------------------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("name", list(uc.CAMERAS))
def test_parity_with_the_checker(name):
    cam = uc.CAMERAS[name][0]
    worst, dropped, seen = 0.0, 0, set()
    for n in SIZES:
        pts1, cov1 = uc.spread(name, n, 100 + n)
        pts2, cov2 = uc.spread(name, n, 200 + n)
        for flags in FLAGS:
            got = device(cam, pts1, pts2, cov2, cov1, flags=flags)
            assert got.pts1.shape == (n, 2) and got.cov2.shape == (n, 3) and got.status2.shape == (n,)
            assert got.status1.dtype == np.uint8
            for side, (p, c, gp, gc, gs) in enumerate(((pts1, cov1, got.pts1, got.cov1, got.status1),
                                                       (pts2, cov2, got.pts2, got.cov2, got.status2))):
                w64 = uc.undistort_np(cam, p, c, flags=flags)
                wld = uc.undistort_np(cam, p, c, flags=flags, dtype=np.longdouble)
                keep = w64.status == wld.status
                dropped += int((~keep).sum())
                seen |= set(w64.status[keep].tolist())
                worst = max(worst, _compare((gp, gc), gs, w64, wld, keep, f"{name} n={n} flags={flags} side {side + 1}"))
    print(f"parity {name}: worst |device - float64 checker| / |float64 - longdouble checker| = {worst:.3f} (4 allowed), "
          f"{dropped} points dropped for a status the two checkers disagree on, statuses seen {sorted(seen)}")
    assert dropped == 0, "on these fixtures the two checkers agree in every status"


def test_the_status_cases_in_normalised_units():
    pts = np.array([xy for xy, _, _ in uc.STATUS_CASES] + [(0.3, -0.2), (-0.55, 0.4), (0.0, 0.0)])
    cov = uc.random_cov(len(pts), 5)
    worst = 0.0
    for flags in FLAGS:
        got = device(uc.UNIT, pts, pts[::-1].copy(), cov2=cov[::-1].copy(), cov1=cov, flags=flags)
        w64 = uc.undistort_np(uc.UNIT, pts, cov, flags=flags)
        wld = uc.undistort_np(uc.UNIT, pts, cov, flags=flags, dtype=np.longdouble)
        assert np.array_equal(w64.status, wld.status), "none of the named cases may be dropped"
        keep = np.ones(len(pts), bool)
        worst = max(worst, _compare((got.pts1, got.cov1), got.status1, w64, wld, keep, f"status cases, flags={flags}"))
        _bits(got.pts2[::-1], got.pts1, "the same points on side 2")
        _bits(got.cov2[::-1], got.cov1, "the same covariances on side 2")
        _bits(got.status2[::-1], got.status1, "the same statuses on side 2")
        for i, (xy, case_flags, want) in enumerate(uc.STATUS_CASES):
            if (case_flags & uc.NEWTON) == (flags & uc.NEWTON) or want == uc.OUTSIDE:
                assert int(got.status1[i]) == want, (xy, flags)
        # OUTSIDE returns the input, NOT_CONVERGED the fixed-point result; a covariance that is not OK's is a copy
        _bits(got.pts1[:2], pts[:2], "OUTSIDE: the point comes back")
        bad = got.status1 != uc.OK
        _bits(got.cov1[bad], cov[bad], f"flags={flags}: the covariance of a point that is not OK")
        if flags & uc.NEWTON:
            _bits(got.pts1[2], device(uc.UNIT, pts[2:3]).pts1[0], "NOT_CONVERGED: the fixed-point result")
            assert abs(got.pts1[3, 0] - 1.0) <= 2.0 ** -45 and got.pts1[3, 1] == 0.0
    print(f"status cases: worst factor {worst:.3f}")


# ------------------------------------------------------------------------------------------------------------------ bits
def _mixed(n, seed):
    """rows of the EuRoC-like camera with a NaN, an infinity and a far-outside point among them"""
    pts1, cov1 = uc.spread("euroc", n, seed)
    pts2, cov2 = uc.spread("euroc", n, seed + 7)
    pts1[n // 3] = [np.nan, 100.0]
    pts2[n // 2] = [50.0, -np.inf]
    pts2[n // 5] = [5000.0, 4000.0]
    return pts1, pts2, cov2, cov1


def test_zero_coefficients_copy_everything_under_every_flag():
    cam = uc.EUROC.copy()
    cam[4:] = [0.0, -0.0, 0.0, 0.0, -0.0]
    pts1, pts2, cov2, cov1 = _mixed(130, 11)
    for flags in FLAGS:
        got = device(cam, pts1, pts2, cov2, cov1, flags=flags)
        for a, b, k in ((got.pts1, pts1, "pts1"), (got.pts2, pts2, "pts2"), (got.cov2, cov2, "cov2"), (got.cov1, cov1, "cov1")):
            _bits(a, b, f"flags={flags}: {k}")
        assert not got.status1.any() and not got.status2.any()


def test_covariances_are_copied_without_the_flag_and_for_points_that_are_not_ok():
    pts1, pts2, cov2, cov1 = _mixed(130, 12)
    for flags in (0, uc.NEWTON):
        got = device(uc.EUROC, pts1, pts2, cov2, cov1, flags=flags)
        _bits(got.cov2, cov2, f"flags={flags}: cov2")
        _bits(got.cov1, cov1, f"flags={flags}: cov1")
    for flags in (uc.PROPAGATE_COV, uc.PROPAGATE_COV | uc.NEWTON):
        got = device(uc.EUROC, pts1, pts2, cov2, cov1, flags=flags)
        bad1, bad2 = got.status1 != uc.OK, got.status2 != uc.OK
        assert bad1.sum() >= 1 and bad2.sum() >= 1
        _bits(got.cov1[bad1], cov1[bad1], f"flags={flags}: cov1 of rows that are not OK")
        _bits(got.cov2[bad2], cov2[bad2], f"flags={flags}: cov2 of rows that are not OK")
        assert not np.array_equal(got.cov1[~bad1], cov1[~bad1])


def test_not_finite_rows_give_nan_and_leave_their_neighbours_alone():
    pts1, pts2, cov2, cov1 = _mixed(130, 13)
    clean1, clean2 = pts1.copy(), pts2.copy()
    clean1[130 // 3] = [10.0, 100.0]
    clean2[130 // 2] = [50.0, 20.0]
    for flags in FLAGS:
        got = device(uc.EUROC, pts1, pts2, cov2, cov1, flags=flags)
        ref = device(uc.EUROC, clean1, clean2, cov2, cov1, flags=flags)
        assert got.status1[130 // 3] == uc.NOT_FINITE and got.status2[130 // 2] == uc.NOT_FINITE
        assert np.isnan(got.pts1[130 // 3]).all() and np.isnan(got.pts2[130 // 2]).all()
        _bits(got.cov1[130 // 3], cov1[130 // 3], "the covariance of a NOT_FINITE row")
        others1, others2 = np.arange(130) != 130 // 3, np.arange(130) != 130 // 2
        assert (got.status1[others1] != uc.NOT_FINITE).all()
        for k, others in (("pts1", others1), ("cov1", others1), ("status1", others1), ("pts2", others2), ("cov2", others2),
                          ("status2", others2)):
            _bits(getattr(got, k)[others], getattr(ref, k)[others], f"flags={flags}: {k} of the other rows")


def test_in_place_equals_out_of_place_and_host_space_equals_device_space():
    torch = _torch()
    pts1, pts2, cov2, cov1 = _mixed(257, 14)
    for flags in FLAGS:
        kw = dict(newton=bool(flags & uc.NEWTON), propagate_cov=bool(flags & uc.PROPAGATE_COV))
        ref = device(uc.EUROC, pts1, pts2, cov2, cov1, flags=flags)
        # in place: every output is its own input
        d = [_dev(a.copy()) for a in (pts1, pts2, cov2, cov1)]
        s1, s2 = (torch.empty(257, dtype=torch.uint8, device="cuda") for _ in range(2))
        u = undistort_keypoints(_dev(uc.EUROC), *d, out=Undistorted(d[0], d[1], d[2], d[3], s1, s2), **kw)
        torch.cuda.synchronize()
        assert u.pts1.data_ptr() == d[0].data_ptr() and u.cov2.data_ptr() == d[2].data_ptr()
        _all_bits(_np(u), ref, f"flags={flags}: in place")
        # HOST space, out of place and in place
        host = undistort_keypoints(uc.EUROC, pts1, pts2, cov2, cov1, **kw)
        assert isinstance(host.pts1, np.ndarray) and host.status1.dtype == np.uint8
        _all_bits(host, ref, f"flags={flags}: HOST space")
        h = [a.copy() for a in (pts1, pts2, cov2, cov1)]
        hs = Undistorted(h[0], h[1], h[2], h[3], np.empty(257, np.uint8), np.empty(257, np.uint8))
        _all_bits(undistort_keypoints(uc.EUROC, *h, out=hs, **kw), ref, f"flags={flags}: HOST space in place")
        # `out` reuses a previous result's buffers
        first = undistort_keypoints(_dev(uc.EUROC), *[_dev(a) for a in (pts1, pts2, cov2, cov1)], **kw)
        ptrs = [first.pts1.data_ptr(), first.cov1.data_ptr(), first.status2.data_ptr()]
        again = undistort_keypoints(_dev(uc.EUROC), *[_dev(a[::-1].copy()) for a in (pts1, pts2, cov2, cov1)], out=first, **kw)
        torch.cuda.synchronize()
        assert ptrs == [again.pts1.data_ptr(), again.cov1.data_ptr(), again.status2.data_ptr()]
        _all_bits(_np(Undistorted(*(getattr(again, k).flip(0) for k in ("pts1", "pts2", "cov2", "cov1", "status1", "status2")))),
                  ref, f"flags={flags}: out= reused")


def test_a_row_gives_the_same_bits_alone_and_anywhere_in_a_batch():
    """Rows that converge in 0 .. 5 Newton steps among neighbours that never do (20 steps): a lane that has finished
    keeps its values while the wavefront's loop goes on."""
    targets = np.array([(0.3, -0.2), (0.70, 0.0), (0.65, -0.1), (0.0, 0.0), (-0.69, 0.05), (2.0, 0.0)])
    tcov = uc.random_cov(len(targets), 21)
    rng = np.random.default_rng(22)
    slow = np.stack([rng.uniform(0.705, 0.8, 4000), rng.uniform(-0.01, 0.01, 4000)], axis=1)   # beyond the fold
    # (some of these are OUTSIDE, and from some Newton finds the root on the far side of the model: the checker says which)
    slow = slow[uc.undistort_np(uc.UNIT, slow, flags=uc.NEWTON).status == uc.NOT_CONVERGED][:257]
    assert len(slow) == 257
    slow_cov = uc.random_cov(257, 23)
    for flags in FLAGS:
        alone = [device(uc.UNIT, targets[i:i + 1], targets[i:i + 1], tcov[i:i + 1], tcov[i:i + 1], flags=flags)
                 for i in range(len(targets))]
        if flags & uc.NEWTON:
            assert [int(a.status1[0]) for a in alone] == [0, 0, 0, 0, 0, uc.OUTSIDE]
        for where in ("lane 0", "lane 63", "shuffled"):
            pts, cov = slow.copy(), slow_cov.copy()
            n = 64 if where != "shuffled" else 257
            pts, cov = pts[:n], cov[:n]
            at = {"lane 0": [0] * 6, "lane 63": [63] * 6, "shuffled": rng.permutation(257)[:6].tolist()}[where]
            for i in range(len(targets)):
                if where != "shuffled":
                    pts, cov = slow[:n].copy(), slow_cov[:n].copy()
                pts[at[i]], cov[at[i]] = targets[i], tcov[i]
                if where != "shuffled" or i == len(targets) - 1:
                    got = device(uc.UNIT, pts, pts, cov, cov, flags=flags)
                    if flags & uc.NEWTON:
                        assert (got.status1 == uc.NOT_CONVERGED).sum() >= n - 6
                    for j in (range(len(targets)) if where == "shuffled" else [i]):
                        for k in ("pts1", "pts2", "cov2", "cov1", "status1", "status2"):
                            _bits(getattr(got, k)[at[j]], getattr(alone[j], k)[0], f"flags={flags}, {where}, target {j}: {k}")


def test_partial_calls_give_the_bits_of_the_full_call():
    pts1, pts2, cov2, cov1 = _mixed(130, 15)
    for flags in FLAGS:
        full = device(uc.EUROC, pts1, pts2, cov2, cov1, flags=flags)
        only1 = device(uc.EUROC, pts1, flags=flags)
        assert only1.pts2 is None and only1.cov2 is None and only1.cov1 is None and only1.status2 is None
        _all_bits(only1, full, f"flags={flags}: pts1 alone", keys=("pts1", "status1"))
        no_cov = device(uc.EUROC, pts1, pts2, flags=flags)
        _all_bits(no_cov, full, f"flags={flags}: no covariances", keys=("pts1", "pts2", "status1", "status2"))
        c2 = device(uc.EUROC, pts1, pts2, cov2, flags=flags)
        assert c2.cov1 is None
        _all_bits(c2, full, f"flags={flags}: cov2 alone", keys=("pts1", "pts2", "cov2", "status1", "status2"))
        c1 = device(uc.EUROC, pts1, None, None, cov1, flags=flags)
        _all_bits(c1, full, f"flags={flags}: pts1 and cov1", keys=("pts1", "cov1", "status1"))
    # the raw call with pts1 NULL: frame 2 alone
    torch = _torch()
    d2, dc2, cam = _dev(pts2), _dev(cov2), _dev(uc.EUROC)
    o2, oc2 = torch.empty_like(d2), torch.empty_like(dc2)
    s2 = torch.empty(130, dtype=torch.uint8, device="cuda")
    capi.check(capi.lib().pnec_hip_undistort_keypoints(0, 130, None, d2.data_ptr(), dc2.data_ptr(), None, cam.data_ptr(), 5, 20, 3,
                                                       None, o2.data_ptr(), oc2.data_ptr(), None, None, s2.data_ptr(),
                                                       capi.MEM_DEVICE, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    full = device(uc.EUROC, pts1, pts2, cov2, cov1, flags=3)
    _bits(o2.cpu().numpy(), full.pts2, "pts1 NULL: pts2")
    _bits(oc2.cpu().numpy(), full.cov2, "pts1 NULL: cov2")
    _bits(s2.cpu().numpy(), full.status2, "pts1 NULL: status2")


def test_iteration_counts_are_honoured():
    pts, _ = uc.spread("euroc", 65, 31)
    for fixed, newton_it in ((0, 20), (1, 2), (12, 0), (64, 64)):
        for flags in (0, uc.NEWTON):
            got = device(uc.EUROC, pts, flags=flags, fixed_iterations=fixed, newton_iterations=newton_it)
            want = uc.undistort_np(uc.EUROC, pts, fixed_iterations=fixed, newton_iterations=newton_it, flags=flags)
            assert np.array_equal(got.status1, want.status), (fixed, newton_it, flags)
            assert np.all(np.abs(got.pts1 - want.pts) <= 8.0 * _ulp(want.pts)), (fixed, newton_it, flags)


# ------------------------------------------------------------------------------------------------ propagated covariance
def test_propagated_covariance_stays_symmetric_positive_semidefinite():
    """Parity of the propagated covariance is test_parity_with_the_checker's; here: positive semi-definite in, positive
    semi-definite out, singular and zero matrices included.  det(S') = det(A)^2 det(S) in exact arithmetic; each of the
    three entries is a sum of four products of magnitude up to |A|^2 |S|, so the computed determinant may be short of it
    by a few roundings of trace(S')^2: 64 * 2^-52 * trace^2 is allowed below zero."""
    n = 257
    pts, cov = uc.spread("euroc", n, 41)
    cov[:40] = np.outer(np.linspace(0.01, 4.0, 40), [1.0, 1.0, 1.0])                      # rank one
    th = np.linspace(0.0, np.pi, 40)
    cov[40:80] = np.stack([np.cos(th) ** 2, np.cos(th) * np.sin(th), np.sin(th) ** 2], axis=1)   # rank one, every direction
    cov[80:90] = 0.0
    for flags in (uc.PROPAGATE_COV, uc.PROPAGATE_COV | uc.NEWTON):
        got = device(uc.EUROC, pts, pts, cov, cov, flags=flags)
        ok = got.status2 == uc.OK
        assert ok.sum() > 200
        xx, xy, yy = got.cov2[ok].T
        tr = xx + yy
        assert np.all(xx >= 0.0) and np.all(yy >= 0.0)
        assert np.all(xx * yy - xy * xy >= -64.0 * 2.0 ** -52 * tr * tr)
        assert np.all(got.cov2[80:90][ok[80:90]] == 0.0)
        # sqrt(det S / det S') = |det J|: the forward model shrinks the image towards its corners, 0.39 .. 1 on this camera
        full = ok & (np.arange(n) >= 90)
        ratio = np.sqrt((cov[full, 0] * cov[full, 2] - cov[full, 1] ** 2) /
                        (got.cov2[full, 0] * got.cov2[full, 2] - got.cov2[full, 1] ** 2))
        print(f"flags={flags}: |det J| over the image {ratio.min():.3f} .. {ratio.max():.3f}")
        assert 0.3 < ratio.min() < 0.6 and 0.9 < ratio.max() < 1.1


# ---------------------------------------------------------------------------------------------------------- stream order
def test_device_space_call_respects_stream_order():
    from test_stream_order_gpu import Entry, check
    torch = _torch()
    n = 4099
    def data(seed):
        p1, c1 = uc.spread("euroc", n, seed)
        p2, c2 = uc.spread("euroc", n, seed + 1)
        return dict(pts1=_dev(p1), pts2=_dev(p2), cov2=_dev(c2), cov1=_dev(c1), camera=_dev(uc.EUROC))
    good, decoy = data(51), data(61)
    decoy["camera"] = _dev(uc.TUM)
    out = pnec_amd.undistort.new_undistorted(n, True, torch.device("cuda:0"), cov1=True)

    def call(bufs):
        u = undistort_keypoints(bufs["camera"], bufs["pts1"], bufs["pts2"], bufs["cov2"], bufs["cov1"], newton=True,
                                propagate_cov=True, out=out)
        return [u.pts1, u.pts2, u.cov2, u.cov1, u.status1, u.status2], None

    check(Entry(good, decoy, call, sentinels=[out.pts1, out.pts2, out.cov2, out.cov1, out.status1, out.status2]),
          "undistort_keypoints")


# -------------------------------------------------------------------------------------------------------------- odometry
def _odometry_kit():
    from test_odometry_gpu import K_INV, TRACKER, _bits_equal, _frames
    from test_patch_track_cpu import H0, W0
    from test_tracks_cpu import RETAIN_KEYS, SEQ_F
    return K_INV, TRACKER, _bits_equal, _frames, H0, W0, RETAIN_KEYS, SEQ_F


@pytest.mark.parametrize("keyframes", [False, True])
def test_odometry_with_zero_distortion_equals_odometry_without(keyframes):
    from pnec_amd import Odometry
    K_INV, TRACKER, _bits_equal, _frames, H0, W0, _, SEQ_F = _odometry_kit()
    kw = dict(TRACKER, ring=4, min_displacement=2.5) if keyframes else dict(TRACKER)
    frames = _frames()
    plain = Odometry(SEQ_F, H0, W0, K_INV, **kw)
    zero = Odometry(SEQ_F, H0, W0, K_INV, distortion=[0, 0, 0, 0], undistort_newton=True, undistort_propagate_cov=True, **kw)
    assert plain.undistorted is None and plain._camera is None
    assert plain.process(frames[0]) is None and zero.process(frames[0]) is None
    for n in range(1, 4):
        a, b = plain.process(frames[n]), zero.process(frames[n])
        for k in ("q", "t", "n_corr", "init_q"):
            _bits_equal(getattr(a, k), getattr(b, k), f"frame {n}: {k}")
        assert zero.undistorted is not None and not bool(zero.undistorted.status1.any())
    plain.close()
    zero.close()


def test_odometry_with_distortion_equals_the_hand_made_chain_and_tracks_as_before():
    from pnec_amd import Batch, Odometry, Tracker
    from pnec_amd.multi import alloc_counters
    from pnec_amd.odometry import start_rotation
    torch = _torch()
    K_INV, TRACKER, _bits_equal, _frames, H0, W0, RETAIN_KEYS, SEQ_F = _odometry_kit()
    frames = _frames()
    dist = uc.MILD[4:8].tolist()
    odo = Odometry(SEQ_F, H0, W0, K_INV, distortion=dist, **TRACKER)
    plain = Odometry(SEQ_F, H0, W0, K_INV, **TRACKER)
    trk = Tracker(SEQ_F, H0, W0, **TRACKER)
    cap = trk.capacity
    K = np.linalg.inv(K_INV)
    cam = _dev(pnec_amd.camera_array(K[0, 0], K[1, 1], K[0, 2], K[1, 2], *dist))
    _bits_equal(odo._camera, _dev(pnec_amd.odometry._camera_from(K_INV, dist)), "the camera recovered from K_inv")
    assert np.allclose(odo._camera.cpu().numpy()[:4], [K[0, 0], K[1, 1], K[0, 2], K[1, 2]], rtol=1e-13)
    cam = odo._camera
    batch = Batch.with_capacity(capi.MODE_TARGET, SEQ_F, SEQ_F * cap, device=0)
    batch.reshape(np.arange(SEQ_F + 1, dtype=np.int64) * cap)
    f64 = dict(dtype=torch.float64, device="cuda:0")
    identity = torch.tensor([[0.0, 0.0, 0.0, 1.0]] * SEQ_F, **f64)
    zero_t, k_inv = torch.zeros((SEQ_F, 3), **f64), torch.as_tensor(K_INV, **f64)
    assert odo.process(frames[0]) is None and plain.process(frames[0]) is None and trk.process(frames[0]) is None
    prev_q, moved = None, False
    for n in range(1, 4):
        if n == 3:
            torch.cuda.synchronize()
            a0 = alloc_counters()
        out = odo.process(frames[n])
        if n == 3:
            torch.cuda.synchronize()
            assert alloc_counters()["hip_malloc_calls"] == a0["hip_malloc_calls"]
        raw = plain.process(frames[n])
        pairs = trk.process(frames[n])
        for k in RETAIN_KEYS:     # tracking is untouched: .pairs is the raw tracker result
            _bits_equal(getattr(out.pairs, k), getattr(raw.pairs, k), f"frame {n}: pairs.{k} against a run without distortion")
            _bits_equal(getattr(out.pairs, k), getattr(pairs, k), f"frame {n}: pairs.{k} against the tracker")
        u = undistort_keypoints(cam, pairs.prev_pts, pairs.pts, pairs.cov)
        assert u.pts1.data_ptr() != pairs.prev_pts.data_ptr() and odo.undistorted.pts1.data_ptr() != out.pairs.prev_pts.data_ptr()
        for k in ("pts1", "pts2", "cov2", "status1", "status2"):
            _bits_equal(getattr(odo.undistorted, k), getattr(u, k), f"frame {n}: undistorted.{k}")
        batch.fill_keypoints_ragged(pairs.offsets, u.pts1, u.pts2, u.cov2, K_inv=k_inv)
        init_q = start_rotation(prev_q, identity)
        q, t = batch.solve_pipeline(init_q, zero_t, None)
        torch.cuda.synchronize()
        _bits_equal(out.init_q, init_q, f"frame {n}: start rotation")
        _bits_equal(out.q, q, f"frame {n}: q")
        _bits_equal(out.t, t, f"frame {n}: t")
        rows = int(pairs.offsets[-1])
        moved |= rows > 0 and not torch.equal(u.pts2[:rows], pairs.pts[:rows])
        prev_q = q
    assert moved, "the mild camera moves the points: the comparison has power"
    for o in (odo, plain):
        o.close()
    batch.close()


# -------------------------------------------------------------------------------------------------------------- geometry
def _pose_distance(qa, ta, qb, tb):
    """|qa -+ qb| + |ta - tb|: linear in a small difference, unlike an angle from an arc cosine"""
    qa, qb = np.asarray(qa, float), np.asarray(qb, float)
    return float(min(np.linalg.norm(qa - qb), np.linalg.norm(qa + qb)) + np.linalg.norm(np.asarray(ta) - np.asarray(tb)))


def _two_views(n, seed):
    """ideal pixels of n points seen by two EuRoC-like cameras, and the pose (q xyzw, unit t): X1 = R X2 + t"""
    from oracle import pnec_oracle as po
    rng = np.random.default_rng(seed)
    cam = uc.EUROC
    rv = np.array([0.02, -0.05, 0.03])
    th = np.linalg.norm(rv)
    k = rv / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
    t = np.array([0.4, 0.05, 0.1])
    X1 = np.stack([rng.uniform(-6, 6, 4 * n), rng.uniform(-3.5, 3.5, 4 * n), rng.uniform(4, 12, 4 * n)], axis=1)
    X2 = (X1 - t) @ R            # rows of R'(X1 - t)
    px = lambda X: np.stack([cam[0] * X[:, 0] / X[:, 2] + cam[2], cam[1] * X[:, 1] / X[:, 2] + cam[3]], axis=1)
    p1, p2 = px(X1), px(X2)
    inside = lambda p: (p[:, 0] > 20) & (p[:, 0] < 732) & (p[:, 1] > 20) & (p[:, 1] < 460)
    keep = np.flatnonzero(inside(p1) & inside(p2))[:n]
    assert len(keep) == n
    return p1[keep], p2[keep], po.quat_from_rot(R), t / np.linalg.norm(t)


def test_geometry_undistorted_points_give_the_pose_of_the_ideal_pixels():
    from oracle import pnec_oracle as po
    from pnec_amd import Batch
    n = 200
    cam = uc.EUROC
    K_inv = np.linalg.inv(np.array([[cam[0], 0, cam[2]], [0, cam[1], cam[3]], [0, 0, 1.0]]))
    ideal1, ideal2, q_true, t_true = _two_views(n, 71)
    raw1, raw2 = uc.distort_pixels(cam, ideal1), uc.distort_pixels(cam, ideal2)
    cov = np.tile([0.25, 0.0, 0.25], (n, 1))
    und = device(cam, raw1, raw2, cov, flags=uc.NEWTON)
    assert not und.status1.any() and not und.status2.any()
    chk1, chk2 = (uc.undistort_np(cam, r, flags=uc.NEWTON).pts for r in (raw1, raw2))
    print(f"device against checker on the scene: {np.abs(und.pts1 - chk1).max():.3e} px; undistorted against ideal "
          f"{max(np.abs(und.pts1 - ideal1).max(), np.abs(und.pts2 - ideal2).max()):.3e} px; raw against ideal "
          f"{np.abs(raw1 - ideal1).max():.2f} px")
    # a start near the truth, the same for every solve
    init_q = np.asarray(po.quat_from_rot(po.rot_from_quat(q_true) @ po.cayley_to_rot(np.array([0.004, -0.003, 0.005]))))
    init_t = t_true + np.array([0.02, -0.03, 0.01])
    init_t /= np.linalg.norm(init_t)

    def oracle_pose(p1, p2):
        b1 = np.stack([po.unproject(p, K_inv) for p in p1])
        b2 = np.stack([po.unproject(p, K_inv) for p in p2])
        C = np.array([[0.25, 0, 0], [0, 0.25, 0], [0, 0, 0.0]])
        covs = np.stack([po.unscented_transform(np.array([p[0], p[1], 1.0]), C, K_inv) for p in p2])
        s = po.solve(po.MODE_TARGET, b1, b2, covs, None, 1e-13, init_q, init_t, po.default_options())
        return np.asarray(po.quat_from_rot(s.R)), np.asarray(s.t) / np.linalg.norm(s.t)

    def device_pose(p1, p2):
        b = Batch.uniform(capi.MODE_TARGET, 1, n, device=0)
        b.fill_keypoints(p1, p2, cov, K_inv=K_inv)
        r = b.solve(init_q[None], init_t[None], reg=1e-13)
        q, t = np.array(r.q).reshape(4), np.array(r.t).reshape(3)
        b.close()
        return q, t / np.linalg.norm(t)

    margin = 10.0 * _pose_distance(*oracle_pose(chk1, chk2), *oracle_pose(ideal1, ideal2))
    q_i, t_i = device_pose(ideal1, ideal2)
    q_u, t_u = device_pose(und.pts1, und.pts2)
    q_r, t_r = device_pose(raw1, raw2)
    d_und = _pose_distance(q_u, t_u, q_i, t_i)
    e_i, e_u, e_r = (_pose_distance(q, t, q_true, t_true) for q, t in ((q_i, t_i), (q_u, t_u), (q_r, t_r)))
    print(f"geometry: pose from undistorted against pose from ideal {d_und:.3e} (margin {margin:.3e} = 10 x the oracle's); "
          f"against the true pose: ideal {e_i:.3e}, undistorted {e_u:.3e}, raw {e_r:.3e}")
    assert d_und <= margin
    assert e_r >= 100.0 * max(e_i, e_u)
