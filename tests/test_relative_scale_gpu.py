"""Relative scale between consecutive pairs from linked tracks (pnec_hip_relative_scale) on the device.

The yardstick is numpy float64 (`relative_scale_np` of tests/test_relative_scale_cpu.py, which also makes the data) or
the exact geometry itself; never a device result -- except where the claim IS about the device's own numbers: the order
statistics must be, bit for bit, elements of the device's own used ratios.

Bounds:
* a ratio: relative 1e-13 * (1 / sin^2 psi_prev + 1 / sin^2 psi_cur), the depth bound of tests/test_triangulate_gpu.py
  once per depth (the kernel's per-link function built for the host stays 310x inside it on this batch, see
  tests/test_relative_scale_cpu.py); min_parallax = 0.02 rad, and no link's sin^2 psi lies within 1e-9 relative of the
  gate (asserted), so the used sets cannot differ by rounding;
* used, n_linked, n_used: equal to numpy's;  order statistics, isolation, spaces, handles: bitwise.

The pair "whose ratios span 1e-300 ... 1e300" cannot be made through this interface: norms of the bearings divide out
and t is a direction, so a ratio is depth_prev / depth_cur of real geometry, and a depth beyond 1e7 baselines is a
parallax below 1e-7 rad, which the triangulation reads as parallel rays.  The test makes what CAN be made -- every link
with its own two depths between 1e-9 and 1e6 baselines -- and asserts that the used ratios span more than 1e20 (the top
two bytes of the patterns differ), then checks the ranks bit for bit.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_relative_scale_cpu import (MIN_PARALLAX, ThreeView, _quat_to_R, _unit, gate_margin, link_tolerance,  # noqa: E402
                                     ragged_cases, ranks_np, relative_scale_np)

import pnec_amd  # noqa: E402
from pnec_amd import Batch, capi  # noqa: E402
from pnec_amd import simulation as sim  # noqa: E402
from pnec_amd import tracks as trk  # noqa: E402

pytestmark = pytest.mark.gpu

NEC, TARGET = capi.MODE_NEC, capi.MODE_TARGET
FIELDS = ("scale", "q25", "q75", "n_linked", "n_used", "ratio", "used")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _same(a, b, fields=FIELDS):
    return all(_same_bits(np.asarray(getattr(a, k)), np.asarray(getattr(b, k))) for k in fields)


def _fill(mode, pairs):
    """a batch of (f1, f2) pairs; TARGET batches get some covariance (relative_scale never reads it)"""
    off = np.concatenate([[0], np.cumsum([len(p[0]) for p in pairs])]).astype(np.int64)
    b = Batch(mode, off)
    cat = lambda k: np.ascontiguousarray(np.concatenate([p[k] for p in pairs]))
    if off[-1] > 0:
        b.fill(cat(0), cat(1), None if mode == NEC else np.ascontiguousarray(np.tile(1e-6 * np.eye(3), (off[-1], 1, 1))))
    return b


def _arrays(cases):
    cat = lambda k: np.concatenate([getattr(c, k) for c in cases])
    stack = lambda k: np.array([getattr(c, k) for c in cases])
    return stack("qc"), stack("tc"), stack("qp"), stack("tp"), cat("link")


def _run(cases, min_parallax=MIN_PARALLAX, per_link=True, prev_mode=TARGET, tp_sign=1.0, prev_pair=None):
    qc, tc, qp, tp, link = _arrays(cases)
    pp = np.arange(len(cases), dtype=np.int64) if prev_pair is None else np.asarray(prev_pair, dtype=np.int64)
    with _fill(NEC, [(c.f1c, c.f2c) for c in cases]) as cur, _fill(prev_mode, [(c.f1p, c.f2p) for c in cases]) as prev:
        return cur.relative_scale(prev, pp, link, qc, tc, qp, tp_sign * tp, min_parallax=min_parallax, per_link=per_link)


@pytest.fixture(scope="module")
def ragged():
    """the ragged batch of exact geometry, its numpy reference and the device's result: shared, left unchanged"""
    cases = ragged_cases()
    refs = [c.ref() for c in cases]
    return cases, refs, _run(cases)


# ---- 1. per-link ratio and counts ---------------------------------------------------------------------------------
def test_per_link_ratio_and_counts_against_numpy(ragged):
    cases, refs, r = ragged
    off = np.asarray(r.offsets)
    assert off[-1] == sum(c.n_cur for c in cases) and len(r.ratio) == off[-1] and r.used.dtype == np.uint8
    worst = 0.0
    for p, (c, ref) in enumerate(zip(cases, refs)):
        assert gate_margin(ref, MIN_PARALLAX) > 1e-9
        sl = slice(off[p], off[p + 1])
        assert r.n_linked[p] == ref["n_linked"] and r.n_used[p] == ref["n_used"], p
        assert np.array_equal(r.used[sl], ref["used"]), p
        u = ref["used"] == 1
        assert np.all(np.isnan(r.ratio[sl][~u]))
        if u.any():
            e = np.abs(r.ratio[sl][u] - ref["ratio"][u]) / ref["ratio"][u] / link_tolerance(ref)[u]
            worst = max(worst, float(e.max()))
            assert np.all(e <= 1.0), (p, worst)
    print("worst ratio error against numpy, in units of the tolerance:", worst)


# ---- 2. order statistics, bit for bit -------------------------------------------------------------------------------
def _ranks_hold(r):
    off = np.asarray(r.offsets)
    for p in range(len(off) - 1):
        sl = slice(off[p], off[p + 1])
        x = r.ratio[sl][r.used[sl] == 1]
        assert len(x) == r.n_used[p]
        got = np.array([r.q25[p], r.scale[p], r.q75[p]])
        assert _same_bits(got, ranks_np(x)), (p, got, ranks_np(x))


def test_order_statistics_are_elements_of_the_devices_own_ratios(ragged):
    cases, refs, r = ragged
    assert all(r.n_used[p] >= 1 for p in range(len(cases)))
    _ranks_hold(r)


def test_order_statistics_with_many_exact_duplicates():
    rng = np.random.default_rng(11)
    c = ThreeView(rng, 513, 400)
    rows = np.flatnonzero(c.ref()["used"] == 1)[:9]            # nine used links, each many times over
    idx = rows[rng.integers(0, len(rows), 1300)]
    c.f1c, c.f2c, c.link, c.n_cur = c.f1c[idx], c.f2c[idx], c.link[idx], len(idx)
    r = _run([c])
    assert r.n_used[0] == 1300 and len(np.unique(r.ratio)) <= 9
    _ranks_hold(r)


def test_order_statistics_over_the_widest_span_geometry_allows():
    rng = np.random.default_rng(12)
    n = 900
    c = ThreeView(rng, 4, 4)                                   # the two poses; the points are replaced below
    Rp, Rc = _quat_to_R(c.qp), _quat_to_R(c.qc)
    d = _unit(np.column_stack([rng.uniform(-0.5, 0.5, n), rng.uniform(-0.5, 0.5, n), np.ones(n)]))
    dc, dp = 10.0 ** rng.uniform(-9, 6, n), 10.0 ** rng.uniform(-9, 6, n)      # depths from B, in baselines of each pair
    c.f1c, c.f2c = d, _unit((dc[:, None] * d - c.tc) @ Rc)
    c.f1p, c.f2p = _unit((dp[:, None] * d) @ Rp.T + c.tp), d
    c.link, c.n_cur, c.n_prev = rng.permutation(n).astype(np.int32), n, n
    c.f1p, c.f2p = c.f1p[np.argsort(c.link)], c.f2p[np.argsort(c.link)]      # row link[i] of prev is track i
    r = _run([c], min_parallax=0.0)
    x = r.ratio[r.used == 1]
    assert len(x) >= n // 2 and x.max() / x.min() > 1e20, (len(x), x.min(), x.max())
    _ranks_hold(r)


# ---- 3. truth --------------------------------------------------------------------------------------------------------
def _own_tolerance(r, ref, p, off):
    """the tolerance of the link whose ratio the median is"""
    sl = slice(off[p], off[p + 1])
    i = np.flatnonzero(_bits(r.ratio[sl]) == _bits(np.array([r.scale[p]]))[0])
    assert len(i) >= 1
    return float(link_tolerance(ref)[i].max())


def test_the_median_is_the_true_ratio(ragged):
    cases, refs, r = ragged
    off = np.asarray(r.offsets)
    for p, (c, ref) in enumerate(zip(cases, refs)):
        assert r.n_used[p] >= 1
        assert abs(r.scale[p] - c.truth) / c.truth <= _own_tolerance(r, ref, p, off), p
        assert r.q25[p] <= r.scale[p] <= r.q75[p]


# ---- 4. wrong links --------------------------------------------------------------------------------------------------
def test_the_median_withstands_wrong_links_and_the_mean_does_not():
    cases = ragged_cases(wrong_frac=0.3)
    refs = [c.ref() for c in cases]
    for c, ref in zip(cases, refs):                             # numpy alone: the test is honest
        u = ref["used"] == 1
        assert (c.wrong & u).sum() < 0.45 * u.sum()
    r = _run(cases)
    off = np.asarray(r.offsets)
    for p, (c, ref) in enumerate(zip(cases, refs)):
        sl = slice(off[p], off[p + 1])
        u = r.used[sl] == 1
        assert np.array_equal(r.used[sl], ref["used"])
        tol = _own_tolerance(r, ref, p, off)
        assert abs(r.scale[p] - c.truth) / c.truth <= tol, p
        if (c.wrong & u).any():
            assert abs(np.mean(r.ratio[sl][u]) - c.truth) / c.truth > tol, p
    assert sum(int((c.wrong & (ref["used"] == 1)).any()) for c, ref in zip(cases, refs)) >= 7


# ---- 5. gates --------------------------------------------------------------------------------------------------------
def test_gates(ragged):
    cases, refs, r = ragged
    P = len(cases)
    back = _run(cases, tp_sign=-1.0)                            # the previous pose with -t: everything lies behind
    assert np.all(back.n_used == 0) and np.all(np.isnan(back.scale)) and np.all(np.isnan(back.q25))
    assert np.all(np.isnan(back.ratio)) and np.all(back.used == 0) and np.array_equal(back.n_linked, r.n_linked)
    pp = np.arange(P)
    pp[[2, 7]] = -1
    cut = _run(cases, prev_pair=pp)
    off = np.asarray(r.offsets)
    for p in range(P):
        sl = slice(off[p], off[p + 1])
        if p in (2, 7):
            assert cut.n_linked[p] == 0 and cut.n_used[p] == 0 and np.isnan(cut.scale[p]) and np.all(cut.used[sl] == 0)
        else:
            assert _same_bits(cut.ratio[sl], r.ratio[sl]) and _same_bits(cut.scale[p:p + 1], r.scale[p:p + 1])
    wide = _run(cases, min_parallax=1.2)                        # larger than every parallax
    assert np.all(wide.n_used == 0) and np.all(np.isnan(wide.scale)) and np.array_equal(wide.n_linked, r.n_linked)
    assert np.all(_run(cases, min_parallax=2.0).n_used == 0)


def test_degenerate_correspondences_are_unused_and_leave_the_rest_alone(ragged):
    cases, refs, r = ragged
    c0 = cases[4]                                               # the pair of 65
    rows = np.flatnonzero(refs[4]["used"] == 1)
    assert len(rows) >= 12
    import copy
    c = copy.deepcopy(c0)
    Rc, Rp = _quat_to_R(c.qc), _quat_to_R(c.qp)
    c.f2c[rows[0], 1] = np.nan                                  # NaN bearing, current side
    c.f1p[c.link[rows[1]], 2] = np.nan                          # ... previous side
    c.f2c[rows[2]] = Rc.T @ c.f1c[rows[2]]                      # parallel rays, current side
    c.f2p[c.link[rows[3]]] = Rp.T @ c.f1p[c.link[rows[3]]]      # ... previous side
    c.f1c[rows[4]] = 0.0                                        # zero bearing, current side
    c.f2p[c.link[rows[5]]] = 0.0                                # ... previous side
    got = _run([c])
    want = _run([c0])
    bad = rows[:6]
    rest = np.ones(65, dtype=bool)
    rest[bad] = False
    assert np.all(got.used[bad] == 0) and np.all(np.isnan(got.ratio[bad]))
    assert _same_bits(got.ratio[rest], want.ratio[rest]) and np.array_equal(got.used[rest], want.used[rest])
    assert got.n_used[0] == want.n_used[0] - 6 and got.n_linked[0] == want.n_linked[0]
    assert _same_bits(np.array([got.q25[0], got.scale[0], got.q75[0]]), ranks_np(got.ratio[got.used == 1]))


# ---- 6. independence, bitwise ----------------------------------------------------------------------------------------
def test_a_pair_alone_has_the_bits_it_has_in_the_batch(ragged):
    cases, refs, r = ragged
    off = np.asarray(r.offsets)
    for p in (0, 3, 6, 8):
        alone = _run([cases[p]], prev_mode=NEC)
        assert _same_bits(alone.ratio, r.ratio[off[p]:off[p + 1]]) and np.array_equal(alone.used, r.used[off[p]:off[p + 1]])
        for k in ("scale", "q25", "q75", "n_linked", "n_used"):
            assert _same_bits(np.asarray(getattr(alone, k)), np.asarray(getattr(r, k))[p:p + 1]), (p, k)


def test_host_space_equals_device_space_with_and_without_out_ratio(ragged):
    import torch
    cases, refs, r = ragged
    qc, tc, qp, tp, link = _arrays(cases)
    pp = np.arange(len(cases), dtype=np.int64)
    dev = lambda a: torch.as_tensor(a, device="cuda:0")
    with _fill(NEC, [(c.f1c, c.f2c) for c in cases]) as cur, _fill(TARGET, [(c.f1p, c.f2p) for c in cases]) as prev:
        d = cur.relative_scale(prev, dev(pp), dev(link), dev(qc), dev(tc), dev(qp), dev(tp), min_parallax=MIN_PARALLAX)
        # without the per-link outputs the ratios live in the handle's workspace (DEVICE) / staging (HOST)
        ds = cur.relative_scale(prev, pp, link, dev(qc), dev(tc), dev(qp), dev(tp), min_parallax=MIN_PARALLAX, per_link=False)
        hs = cur.relative_scale(prev, pp, link, qc, tc, qp, tp, min_parallax=MIN_PARALLAX, per_link=False)
        torch.cuda.synchronize()
    assert d.ratio.is_cuda and d.scale.is_cuda and ds.ratio is None and hs.used is None
    for k in FIELDS:
        assert _same_bits(getattr(d, k).cpu().numpy(), np.asarray(getattr(r, k))), k
    for k in ("scale", "q25", "q75", "n_linked", "n_used"):
        assert _same_bits(getattr(ds, k).cpu().numpy(), np.asarray(getattr(r, k))), k
        assert _same_bits(np.asarray(getattr(hs, k)), np.asarray(getattr(r, k))), k
    assert np.allclose(d.log_sigma().cpu().numpy(), r.log_sigma(), rtol=1e-15, atol=0, equal_nan=True)


def test_prev_as_the_same_handle_equals_a_separate_handle():
    # a sequence of consecutive pairs in ONE batch: pair k's previous pair is pair k - 1 of the same batch
    rng = np.random.default_rng(21)
    sizes = [300, 70, 513, 64, 1100]
    # pair k holds exact bearings at its own pose (so every track is in front); the links are random rows, a few out of
    # range: the ratios mean nothing here, their bits must not depend on which handle the previous pair is read from
    views = [ThreeView(rng, sizes[min(k + 1, 4)], sizes[k]) for k in range(4)]
    pairs = [(v.f1p, v.f2p) for v in views] + [(views[3].f1c, views[3].f2c)]
    q = np.array([v.qp for v in views] + [views[3].qc])
    t = np.array([v.tp for v in views] + [views[3].tc])
    link = np.concatenate([np.full(sizes[0], -1, dtype=np.int32)] +
                          [rng.integers(-2, sizes[k - 1] + 2, sizes[k]).astype(np.int32) for k in range(1, 5)])
    pp = np.arange(-1, 4, dtype=np.int64)
    with _fill(NEC, pairs) as seq, _fill(TARGET, pairs) as other:
        same = seq.relative_scale(seq, pp, link, q, t, q, t, min_parallax=0.0)
        sep = seq.relative_scale(other, pp, link, q, t, q, t, min_parallax=0.0)
    assert same.n_linked[0] == 0 and np.all(same.n_linked[1:] > 0) and same.n_used[4] > 100
    assert _same(same, sep)
    _ranks_hold(same)


# ---- 7. a select_view batch on the current side ----------------------------------------------------------------------
def test_a_select_view_batch_follows_its_own_offsets(ragged):
    cases, refs, r = ragged
    rng = np.random.default_rng(5)
    qc, tc, qp, tp, link = _arrays(cases)
    f1 = np.concatenate([c.f1c for c in cases])
    f2 = np.concatenate([c.f2c for c in cases])
    hit = rng.random(len(f2)) < 0.25                             # a quarter of the tracks is off by a degree
    f2[hit] = _unit(f2[hit] + 0.02 * rng.standard_normal((int(hit.sum()), 3)))
    off = np.asarray(r.offsets)
    pp = np.arange(len(cases), dtype=np.int64)
    with Batch(TARGET, off) as cur, _fill(NEC, [(c.f1p, c.f2p) for c in cases]) as prev:
        cur.fill(f1, f2, np.ascontiguousarray(np.tile(1e-8 * np.eye(3), (len(f1), 1, 1))))
        mask = np.asarray(cur.residuals(qc, tc, gate=3.0).mask).astype(bool)   # the residual gate's verdict
        assert 0.6 * len(mask) <= mask.sum() <= 0.9 * len(mask)
        view = cur.select(mask.astype(np.uint8), view=True)
        got = view.relative_scale(prev, pp, link[mask], qc, tc, qp, tp, min_parallax=MIN_PARALLAX)
        voff = np.asarray(got.offsets)
        assert np.array_equal(np.diff(voff), [mask[off[p]:off[p + 1]].sum() for p in range(len(cases))])
        fresh_pairs = [(f1[off[p]:off[p + 1]][mask[off[p]:off[p + 1]]], f2[off[p]:off[p + 1]][mask[off[p]:off[p + 1]]])
                       for p in range(len(cases))]
        with _fill(NEC, fresh_pairs) as fresh:
            want = fresh.relative_scale(prev, pp, link[mask], qc, tc, qp, tp, min_parallax=MIN_PARALLAX)
    assert len(got.ratio) == mask.sum() and _same(got, want)


# ---- 8. noisy sequences ----------------------------------------------------------------------------------------------
def _noisy_sequences(seed=77, n_seq=2, n_pairs=6, n_tracks=300):
    """two sequences of seven frames seeing 300 tracks each: bearings of frame k exact, of frame k + 1 with the simulator's
    pixel noise (anisotropic, inhomogeneous, focal 800) and its unscented covariances; the rows of every pair shuffled"""
    import torch
    rng = np.random.default_rng(seed)
    focal, rows = 800.0, []
    for s in range(n_seq):
        X = np.column_stack([rng.uniform(-3, 3, n_tracks), rng.uniform(-2, 2, n_tracks), rng.uniform(6, 14, n_tracks)])
        Rw, cw = [np.eye(3)], [np.zeros(3)]                      # camera k: x_k = Rw[k]' (X - cw[k])
        for k in range(n_pairs):
            dR = _quat_to_R(np.concatenate([rng.uniform(-0.015, 0.015, 3), [1.0]]))
            step = np.array([rng.uniform(0.2, 0.5), rng.uniform(-0.1, 0.1), rng.uniform(0.2, 0.9)])
            cw.append(cw[-1] + Rw[-1] @ step)
            Rw.append(Rw[-1] @ dR)
        for k in range(n_pairs):
            x1, x2 = (X - cw[k]) @ Rw[k], (X - cw[k + 1]) @ Rw[k + 1]
            alpha, beta, scale = rng.uniform(0, np.pi, n_tracks), rng.uniform(0.5, 1.0, n_tracks), rng.uniform(0.5, 1.5, n_tracks)
            rot = np.stack([np.cos(alpha), -np.sin(alpha), np.sin(alpha), np.cos(alpha)], -1).reshape(-1, 2, 2)
            dg = np.zeros((n_tracks, 2, 2))
            dg[:, 0, 0], dg[:, 1, 1] = beta, 1 - beta
            cov2d = scale[:, None, None] * (rot @ dg @ rot.transpose(0, 2, 1))
            noise = np.einsum("nij,nj->ni", np.linalg.cholesky(cov2d), rng.standard_normal((n_tracks, 2)))
            p2 = x2 / x2[:, 2:3] * focal
            p2[:, :2] += noise
            cov = sim.unscented_bearing_cov(torch.from_numpy(p2), torch.from_numpy(cov2d)).numpy()
            R_rel, t_rel = Rw[k].T @ Rw[k + 1], Rw[k].T @ (cw[k + 1] - cw[k])      # x_k = R_rel x_{k+1} + t_rel
            order = rng.permutation(n_tracks)
            rows.append(dict(seq=s, ids=order.astype(np.int64) + 1000 * s, b1=_unit(x1)[order], b2=_unit(p2)[order],
                             cov=cov[order], R=R_rel, t=t_rel))
    return rows


def test_noisy_sequences_through_links_solve_triangulate_and_relative_scale():
    rows = _noisy_sequences()
    P, N = len(rows), 300
    cat = lambda k: np.ascontiguousarray(np.concatenate([r[k] for r in rows]))
    init_q = np.array([sim.matrix_to_quaternion_xyzw(__import__("torch").from_numpy(r["R"])[None])[0].numpy() for r in rows])
    init_t = np.array([_unit(r["t"]) for r in rows])
    tr = trk.Tracks(np.arange(P + 1, dtype=np.int64) * N, cat("b1"), cat("b2"), cat("cov"), init_q, init_t,
                    sequence=np.array([r["seq"] for r in rows], dtype=np.int32), ids1=cat("ids"), ids2=cat("ids"))
    prev_pair, link = tr.links()
    assert prev_pair.tolist() == [-1, 0, 1, 2, 3, 4, -1, 6, 7, 8, 9, 10] and (link[N:6 * N] >= 0).all()
    with Batch(TARGET, tr.offsets) as b:
        b.fill(tr.bvs1, tr.bvs2, tr.covs)
        res = b.solve(tr.init_q, tr.init_t)
        tri = res.triangulate(orient=True)
        rs = b.relative_scale(b, prev_pair, link, res.q, tri.t, res.q, tri.t, min_parallax=0.0)
    q, t = np.asarray(res.q), np.asarray(tri.t)
    closeness = []
    for p in range(P):
        sl = slice(p * N, (p + 1) * N)
        if prev_pair[p] < 0:
            assert rs.n_linked[p] == 0 and np.isnan(rs.scale[p])
            continue
        pl = slice((p - 1) * N, p * N)
        ref = relative_scale_np(tr.bvs1[sl], tr.bvs2[sl], q[p], t[p], tr.bvs1[pl], tr.bvs2[pl], q[p - 1], t[p - 1], link[sl])
        assert rs.n_linked[p] == N and rs.n_used[p] == ref["n_used"] >= 0.95 * N
        tol = float(link_tolerance(ref)[np.flatnonzero(ref["ratio"] == ref["scale"][1])].max())   # the median link's own
        assert abs(rs.scale[p] - ref["scale"][1]) / ref["scale"][1] <= tol, p
        closeness.append(abs(rs.scale[p] * np.linalg.norm(rows[p - 1]["t"]) / np.linalg.norm(rows[p]["t"]) - 1.0))
    chain = pnec_amd.chain_scales(rs.scale, prev_pair)
    assert np.all(np.isfinite(chain)) and chain[0] == 1.0 and chain[6] == 1.0 and np.all(chain > 0)
    print("noisy sequences: |median / simulated baseline ratio - 1| worst %.3e, median %.3e; log sigma median %.3e"
          % (max(closeness), float(np.median(closeness)), float(np.nanmedian(rs.log_sigma()))))


# ---- 9. pybind and facade --------------------------------------------------------------------------------------------
def _pose44(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def test_pybind_and_facade_give_the_batch_calls_numbers(ragged):
    import pnec_amd.pypnec as pypnec
    # the facade makes its own quaternion of the rotation matrix; of the identity that is (0, 0, 0, 1) whatever the
    # conversion, so with identity rotations the facade runs the batch call's very inputs
    c = ThreeView(np.random.default_rng(31), 512, 700, max_angle=0.0)
    assert np.array_equal(c.qc, [0, 0, 0, 1]) and np.array_equal(c.qp, [0, 0, 0, 1])
    want = _run([c], prev_mode=NEC)
    assert want.n_used[0] > 100
    scale, q25, q75, n_used, ratio = pypnec.relative_scale(c.f1p, c.f2p, _pose44(np.eye(3), c.tp), c.f1c, c.f2c,
                                                           _pose44(np.eye(3), c.tc), c.link.tolist(), MIN_PARALLAX)
    assert n_used == want.n_used[0] and _same_bits(ratio, want.ratio)
    assert _same_bits(np.array([q25, scale, q75]), np.array([want.q25[0], want.scale[0], want.q75[0]]))
