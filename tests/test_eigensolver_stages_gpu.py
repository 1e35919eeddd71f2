"""The two stage calls in front of the refinement (pnec_hip_nec_eigensolver, pnec_hip_weighted_eigensolver: sums36_kernel,
es_batch_kernel / es_batch_alt_kernel, weighted_eigensolver_kernel, weighted_eigensolver_mixed_kernel<2|8>) against the
checker at every parameter the suite otherwise leaves at the reference's default: reg (a), weighted_iterations under the
three eigensolver schemes (b), the kernel form a batch's n_max picks (c), pair counts around the sixteen pairs a
minimising wavefront holds (d), memory spaces, residual families and refusals (e), the whole size ladder with a start per
pair (f).

Every pair is compared; none is left out.  The bounds are the suite's existing ones:
  twin (the checker with the kernel's two early exits), NEWTON / LM   rotation <= 1e-8 rad, |abs(t . t') - 1| < 1e-8
  literal loop (the reference), NEWTON / LM                            WEIGHTED_EARLY_EXIT_BOUND (1e-7 rad)
  twin, DESCENT, pairs stable on the CPU                               <= 1e-8 rad
  twin, DESCENT, the other pairs                                       <= 1e-6 rad (test_opengv_schemes: chained descents)
  plain stage against the checker                                      <= 1e-8 rad, |abs(t . t') - 1| < 1e-9
What makes them fair demands -- every pair stable under NEWTON and LM, the stable mask under DESCENT, reg and the DESCENT
round count visible far above the bounds, one pose from two rounds on under NEWTON and LM -- is established for these very
inputs by test_eigensolver_stages_cpu.py from the checker alone.  Under DESCENT the twin's rotation IS the literal loop's
(the descent has no rotation exit), so the literal loop is held to the twin's bound there."""
import os
import sys

import numpy as np
import pytest

from pnec_amd import Batch, capi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eigensolver_stage_cases as ec  # noqa: E402
from test_parity_gpu import WEIGHTED_EARLY_EXIT_BOUND  # noqa: E402

pytestmark = pytest.mark.gpu

TWIN_TOL = 1e-8           # rad, and |abs(t . t') - 1|
DESCENT_LOOSE_TOL = 1e-6  # rad: a DESCENT pair that is not stable on the CPU
PLAIN_T_TOL = 1e-9        # test_parity_gpu.test_nec_eigensolver_device_vs_oracle's


def _quat_to_R(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _batch(pairs, mode=capi.MODE_TARGET):
    x = ec.inputs(pairs)
    b = Batch(mode, x.offsets)
    if mode == capi.MODE_NEC:
        b.fill(x.f1, x.f2)
    elif mode == capi.MODE_SYM:
        b.fill(x.f1, x.f2, x.c2, np.roll(x.c2, 1, axis=0) * 0.8)
    else:
        b.fill(x.f1, x.f2, x.c2)       # (TARGET: frame 2's covariances; HOST: the same numbers as frame 1's)
    return b


def _weighted(b, case, pairs=None):
    """the weighted stage of `case` on batch b, which holds `pairs` (the case's own unless given)"""
    b.set_eigensolver_scheme(case.scheme)
    q, t = ec.weighted_starts(case.pairs if pairs is None else pairs, case.scheme)
    return b.weighted_eigensolver(q, t, case.reg, case.iterations)


def _same_bits(a, b):
    return all(x.dtype == y.dtype and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def _compare_weighted(case, out, label="", pairs=None):
    """every pair of (q, t) against the twin and the literal loop; prints the worst distances"""
    q, t = out
    pairs = case.pairs if pairs is None else pairs
    name = label or case.name
    worst = dict(twin=0.0, twin_t=0.0, literal=0.0)
    for p, pair in enumerate(pairs):
        r = ec.weighted_reference(pair, case.scheme, case.reg, case.iterations)
        where = (name, p, pair.n)
        assert np.isfinite(q[p]).all() and abs(np.linalg.norm(q[p]) - 1) < 1e-12, where + (q[p],)
        R = _quat_to_R(q[p])
        e_twin, e_t, e_lit = ec.rot_angle(R, r.R), ec.t_distance(t[p], r.t), ec.rot_angle(R, r.literal_R)
        worst = dict(twin=max(worst["twin"], e_twin), twin_t=max(worst["twin_t"], e_t), literal=max(worst["literal"], e_lit))
        if case.scheme == ec.DESCENT:
            tol = TWIN_TOL if r.stable else DESCENT_LOOSE_TOL
            assert e_twin <= tol and e_t < tol and e_lit <= tol, where + (r.stable, e_twin, e_t, e_lit)
        else:
            assert r.stable, where                                   # the inputs (test_eigensolver_stages_cpu.py)
            assert e_twin <= TWIN_TOL and e_t < TWIN_TOL, where + (e_twin, e_t)
            assert e_lit <= WEIGHTED_EARLY_EXIT_BOUND, where + (e_lit,)
    print(f"{name}: device against twin at most {worst['twin']:.3e} rad, t {worst['twin_t']:.1e}; against the literal loop "
          f"{worst['literal']:.3e} rad; {len(pairs)} pairs")
    return worst


def _compare_plain(pairs, scheme, out, label):
    q, t = out
    worst, worst_t = 0.0, 0.0
    for p, pair in enumerate(pairs):
        r = ec.plain_reference(pair, scheme)
        assert r.stable, (label, p, pair.n)
        e, e_t = ec.rot_angle(_quat_to_R(q[p]), r.R), ec.t_distance(t[p], r.t)
        worst, worst_t = max(worst, e), max(worst_t, e_t)
        assert e <= TWIN_TOL and e_t < PLAIN_T_TOL, (label, p, pair.n, e, e_t)
        assert t[p][np.argmax(np.abs(t[p]))] > 0, (label, p)          # the eigenvector's sign convention
    print(f"{label}: plain stage against the checker at most {worst:.3e} rad, t {worst_t:.1e}; {len(pairs)} pairs")


# ---- a: reg ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ec.CASES_REG, ids=lambda c: c.name)
def test_reg_ladder(case):
    """a: reg 0, 1e-13, 1e-10, 1e-6, 1e-2 under NEWTON and 1e-6 under LM and DESCENT, twelve pairs of 8 ... 700, each
    against the checker run at the same reg (1e-13 and 1e-6 lie 7e-5 ... 1e-3 rad apart on these pairs; at 1e-2 the
    rotation is the plain stage's and only t moves)"""
    with _batch(case.pairs) as b:
        out = _weighted(b, case)
    _compare_weighted(case, out)


def test_chain_hands_its_regularization_to_the_weighted_stage():
    """a: solve_pipeline without RANSAC and refinement at regularization = 1e-6 is, bit for bit, nec_eigensolver followed
    by weighted_eigensolver at reg = 1e-6 -- and not what the stages give at the default"""
    x = ec.inputs(ec.TO_700_PAIRS)
    opts = capi.default_pipeline_options(use_ransac=0, use_ceres=0, regularization=1e-6)
    with _batch(ec.TO_700_PAIRS) as b:
        chain = b.solve_pipeline(x.q0, x.t0, options=opts)
        qn, tn = b.nec_eigensolver(x.q0)
        stages = b.weighted_eigensolver(qn, tn, 1e-6, 10)
        default = b.weighted_eigensolver(qn, tn, 1e-13, 10)
    assert _same_bits(chain, stages)
    apart = [ec.rot_angle(_quat_to_R(a), _quat_to_R(b_)) for a, b_ in zip(stages[0], default[0])]
    print(f"a-chain: reg 1e-6 against 1e-13 on the device: {min(apart):.1e} ... {max(apart):.1e} rad")
    assert np.mean(np.array(apart) > 1e-6) >= 0.5, apart


# ---- b: weighted_iterations --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", [ec.NEWTON, ec.LM], ids=lambda s: ec.SCHEME_NAMES[s])
def test_rounds_ladder_newton_and_lm(scheme):
    """b: 0, 1, 2, 3, 10, 16, 17, 40 rounds.  0 and 1 return the start pose (normalised: compared with the checker, which
    returns it); every count is within tolerance of the checker at that count; and every count from 2 on has the BITS of
    count 2 -- the rotation is final after the first converged call and a translation round that changes nothing ends the
    rest (beyond 16 launch_weighted_eigensolver clips the rounds it prepares; nothing may change there either)."""
    cases = {c.iterations: c for c in ec.CASES_ROUNDS[scheme]}
    with _batch(ec.TO_700_PAIRS) as b:
        out = {k: _weighted(b, c) for k, c in cases.items()}
    for k, c in cases.items():
        _compare_weighted(c, out[k])
    for k in ec.ROUNDS_NEWTON_LM[3:]:
        assert _same_bits(out[k], out[2]), (ec.SCHEME_NAMES[scheme], k, np.abs(out[k][0] - out[2][0]).max(),
                                            np.abs(out[k][1] - out[2][1]).max())
    assert _same_bits(out[0], out[1])


def test_rounds_ladder_descent_and_its_refusal():
    """b, DESCENT: 0, 1, 2, 3, 9, 16 rounds, each against the checker at that count (neighbouring counts lie more than
    1e-7 rad apart on these pairs); 17 is refused as unsupported, and the call after the refusal repeats its bits"""
    cases = {c.iterations: c for c in ec.CASES_ROUNDS[ec.DESCENT]}
    with _batch(ec.TO_700_PAIRS) as b:
        out = {k: _weighted(b, c) for k, c in cases.items()}
        q, t = ec.weighted_starts(ec.TO_700_PAIRS, ec.DESCENT)
        with pytest.raises(capi.PnecHipError) as e:
            b.weighted_eigensolver(q, t, 1e-13, ec.ROUNDS_DESCENT_REFUSED)
        assert e.value.code == capi.ERR_UNSUPPORTED, e.value.code
        again = {k: _weighted(b, cases[k]) for k in (16, 3)}
    for k, c in cases.items():
        _compare_weighted(c, out[k])
    assert _same_bits(again[16], out[16]) and _same_bits(again[3], out[3])
    assert _same_bits(out[0], out[1])


# ---- c: kernel forms ---------------------------------------------------------------------------------------------------
def test_weighted_stage_gives_a_pair_the_same_bits_under_every_kernel_form():
    """c: pairs of 64, 300, 512, 513, 700 and 1 024 correspondences alone (n_max = n: the one-wavefront kernel up to 512,
    mixed<2> above), in a batch whose largest pair has 1 024 (mixed<2>) and in one whose largest has 1 025 (mixed<8>): the
    same bits in all three, each within tolerance of the twin"""
    case = ec.CASE_LADDER
    in_1024 = case.pairs[:-1]
    assert max(p.n for p in in_1024) == 1024 and case.pairs[-1].n == 1025
    with _batch(case.pairs) as b:
        assert b.max_correspondences == 1025
        out_1025 = _weighted(b, case)
    with _batch(in_1024) as b:
        assert b.max_correspondences == 1024
        out_1024 = _weighted(b, case, in_1024)
    _compare_weighted(case, out_1025, "c-in-1025")
    _compare_weighted(case, out_1024, "c-in-1024", in_1024)
    for n in ec.FORM_SIZES:
        i = case.sizes.index(n)
        with _batch(case.pairs[i:i + 1]) as b:
            assert b.max_correspondences == n
            alone = _weighted(b, case, case.pairs[i:i + 1])
        _compare_weighted(case, alone, f"c-alone-{n}", case.pairs[i:i + 1])
        for k in (0, 1):
            assert alone[k][0].tobytes() == out_1024[k][i].tobytes() == out_1025[k][i].tobytes(), (n, "qt"[k])


def test_plain_stage_gives_a_pair_the_same_bits_alone_and_in_a_batch():
    """c: nec_eigensolver has no forms; the same pairs alone against in the ladder's batch"""
    pairs = ec.LADDER_PAIRS
    x = ec.inputs(pairs)
    with _batch(pairs) as b:
        batch = b.nec_eigensolver(x.q0)
    _compare_plain(pairs, ec.NEWTON, batch, "c-plain-in-batch")
    for n in ec.FORM_SIZES:
        i = ec.SIZE_LADDER.index(n)
        with _batch(pairs[i:i + 1]) as b:
            alone = b.nec_eigensolver(x.q0[i:i + 1])
        for k in (0, 1):
            assert alone[k][0].tobytes() == batch[k][i].tobytes(), (n, "qt"[k])


@pytest.mark.parametrize("view", [False, True], ids=["select", "select_view"])
def test_selected_batch_under_its_sources_n_max_equals_a_fresh_batch(view):
    """c: InlierExtraction leaves the target's sizes on the device and its n_max at the source's (1 025: mixed<8>) while
    every pair has shrunk below 512; a fresh batch of the same rows runs the one-wavefront kernel.  Same bits -- before the
    target's sizes have been fetched and after (fetching them lowers its n_max to the real one)."""
    pairs = ec.LADDER_PAIRS[8:]                    # 513, 700, 1 024, 1 025
    keep = (250, 64, 511, 450)
    x = ec.inputs(pairs)
    mask = np.zeros(int(x.offsets[-1]), dtype=np.uint8)
    for p, k in enumerate(keep):
        mask[x.offsets[p]:x.offsets[p + 1]][::2][:k] = 1       # every second row, k of them
    rows = mask.astype(bool)
    q, t = ec.weighted_starts(pairs, ec.NEWTON)
    with Batch(capi.MODE_TARGET, np.concatenate([[0], np.cumsum(keep)]).astype(np.int64)) as fresh:
        fresh.fill(x.f1[rows], x.f2[rows], x.c2[rows])
        assert fresh.max_correspondences == 511
        want_w, want_n = fresh.weighted_eigensolver(q, t, 1e-13, 10), fresh.nec_eigensolver(x.q0)
    with _batch(pairs) as b:
        sel = b.select(mask, view=view)
        got_w, got_n = sel.weighted_eigensolver(q, t, 1e-13, 10), sel.nec_eigensolver(x.q0)
        assert sel.max_correspondences == 511 and list(np.diff(sel.offsets)) == list(keep)
        after_w = sel.weighted_eigensolver(q, t, 1e-13, 10)
        sel.close()
    assert _same_bits(got_w, want_w) and _same_bits(after_w, want_w) and _same_bits(got_n, want_n)
    assert np.isfinite(want_w[0]).all() and np.isfinite(want_n[0]).all()


# ---- d: pair counts ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", ec.PAIR_COUNTS)
def test_pair_counts_around_sixteen_per_wavefront(count):
    """d: 1, 15, 16, 17, 33 pairs of 64 ... 100 correspondences, every pair its own scene and start: the weighted stage and
    the plain stage under all three schemes against the checker pair by pair; the batch in reverse order gives the
    reversed outputs bit for bit (a pair's answer does not depend on its quad, its wavefront or its neighbours)"""
    pairs = ec.COUNT_PAIRS[:count]
    case = ec.Case(f"d-{count}pairs", pairs)
    x, xr = ec.inputs(pairs), ec.inputs(pairs[::-1])
    with _batch(pairs) as b, _batch(pairs[::-1]) as br:
        weighted, weighted_r = _weighted(b, case), _weighted(br, case, pairs[::-1])
        plain, plain_r = {}, {}
        for s in (ec.NEWTON, ec.DESCENT, ec.LM):
            b.set_eigensolver_scheme(s); br.set_eigensolver_scheme(s)
            plain[s], plain_r[s] = b.nec_eigensolver(x.q0), br.nec_eigensolver(xr.q0)
    _compare_weighted(case, weighted)
    assert _same_bits([a[::-1] for a in weighted_r], weighted)
    for s in (ec.NEWTON, ec.DESCENT, ec.LM):
        _compare_plain(pairs, s, plain[s], f"d-{count}pairs-{ec.SCHEME_NAMES[s]}")
        assert _same_bits([a[::-1] for a in plain_r[s]], plain[s]), ec.SCHEME_NAMES[s]


# ---- e: memory spaces, residual families, refusals ---------------------------------------------------------------------
def test_host_space_and_device_space_give_the_same_bytes_in_both_stages():
    import torch
    case = ec.CASE_SPACES
    x = ec.inputs(case.pairs)
    q, t = ec.weighted_starts(case.pairs, case.scheme)
    with _batch(case.pairs) as b:
        host = b.nec_eigensolver(x.q0) + b.weighted_eigensolver(q, t, case.reg, case.iterations)
        dev = b.nec_eigensolver(torch.from_numpy(x.q0.copy()).to("cuda:0")) + b.weighted_eigensolver(
            torch.from_numpy(q.copy()).to("cuda:0"), torch.from_numpy(t.copy()).to("cuda:0"), case.reg, case.iterations)
        torch.cuda.synchronize()
    dev = tuple(v.cpu().numpy() for v in dev)
    assert _same_bits(host, dev)
    _compare_plain(case.pairs, ec.NEWTON, dev[:2], "e-device-space")
    _compare_weighted(case, dev[2:], "e-device-space")


def test_plain_stage_on_every_residual_family():
    """e: nec_eigensolver on NEC, TARGET, HOST and SYM batches filled with the same bearings: each within 1e-8 rad of the
    checker -- and the same BITS in all four: sums36_kernel and the translation epilogue read the six bearing planes
    f1x f1y f1z f2x f2y f2z, which every family keeps first in a pair's block at the same stride round_up(n, 64), in the
    same order (pass_sums36); the covariance planes behind them are never touched by the plain stage."""
    pairs = ec.TO_700_PAIRS
    x = ec.inputs(pairs)
    out = {}
    for name, mode in (("NEC", capi.MODE_NEC), ("TARGET", capi.MODE_TARGET), ("HOST", capi.MODE_HOST), ("SYM", capi.MODE_SYM)):
        with _batch(pairs, mode) as b:
            out[name] = b.nec_eigensolver(x.q0)
        _compare_plain(pairs, ec.NEWTON, out[name], f"e-{name}")
    for name in ("TARGET", "HOST", "SYM"):
        assert _same_bits(out[name], out["NEC"]), name


def test_refusals_leave_the_batch_usable():
    """e: the weighted stage on NEC / HOST / SYM batches is unsupported; weighted_iterations = -1 and a NULL init_t are
    invalid arguments; after every refusal the batch answers as before"""
    pairs = ec.TO_700_PAIRS
    x = ec.inputs(pairs)
    q, t = ec.weighted_starts(pairs, ec.NEWTON)
    for mode in (capi.MODE_NEC, capi.MODE_HOST, capi.MODE_SYM):
        with _batch(pairs, mode) as b:
            before = b.nec_eigensolver(x.q0)
            with pytest.raises(capi.PnecHipError) as e:
                b.weighted_eigensolver(q, t, 1e-13, 10)
            assert e.value.code == capi.ERR_UNSUPPORTED, (mode, e.value.code)
            assert _same_bits(b.nec_eigensolver(x.q0), before), mode
    with _batch(pairs) as b:
        before = b.weighted_eigensolver(q, t, 1e-13, 10)
        for args in ((q, t, 1e-13, -1), (q, None, 1e-13, 10)):
            with pytest.raises(capi.PnecHipError) as e:
                b.weighted_eigensolver(*args)
            assert e.value.code == capi.ERR_INVALID_ARGUMENT, e.value.code
            assert _same_bits(b.weighted_eigensolver(q, t, 1e-13, 10), before)
    _compare_weighted(ec.CASE_SPACES, before, "e-after-refusals")


# ---- f: the size ladder once -------------------------------------------------------------------------------------------
def test_size_ladder_with_a_start_per_pair():
    """f: 8, 37, 63, 64, 65, 300, 511, 512, 513, 700, 1 024, 1 025 correspondences in one ragged batch, a scene and a start
    rotation per pair, both stages under the default scheme against the checker"""
    case = ec.CASE_LADDER
    x = ec.inputs(case.pairs)
    with _batch(case.pairs) as b:
        plain, weighted = b.nec_eigensolver(x.q0), _weighted(b, case)
    _compare_plain(case.pairs, ec.NEWTON, plain, case.name)
    _compare_weighted(case, weighted)
