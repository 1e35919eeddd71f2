"""Every field of pnec_hip_options that lm_advance reads, moved off the Ceres default on the device, against the oracle
run with the same options; and every termination code the options can produce.

The option sets, the inputs and the rule that decides which solves are compared (`kept`: the oracle's analytic and
central-difference paths agree on count and code, so the decision is not one of rounding) live in
test_lm_options_cpu.py, which proves on the CPU that the table keeps at least 6 of 8 solves everywhere, that every set
changes something, and that codes 0 .. 4 all occur.  Here each set runs over its kept solves on every form of the solve
kernel: the one-wavefront rungs the tuner picks for 10 and 100 correspondences, the family's multi-wavefront geometry
forced at 600, and the streaming kernel forced at 100 and 600.

Bars: test_lm_edges_gpu's (equal iteration counts and codes, rotation <= 1e-9 rad, cost rtol 1e-9,
|t . t_oracle| > 1 - 1e-10 against the analytic path; 1e-6 rad with equal counts and codes against the
central-difference path on one kept solve per case).
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_lm_edges_gpu import FAMILIES, FAMILY_IDS, LADDER, MULTI_WAVE, TARGET, Case, _agree, _rot_err, \
    _stream_handle_is_bitwise  # noqa: E402
from test_lm_options_cpu import EDGE, HYP_SETS, MIXED_SIZES, MULTI, N_HYP, NUMERIC_ROT_BAR, NUMERIC_SETS, NUMERIC_SIZES, SMALL, \
    TABLE, hyp_run, inputs, mixed_run, mixed_set, options, settled, table_run  # noqa: E402

from pnec_amd import Batch, capi  # noqa: E402
from pnec_amd import simulation as sim  # noqa: E402

pytestmark = pytest.mark.gpu

FIELDS = ("q", "t", "cost", "iterations", "status")


def _forms(mode):
    """(n, forced geometry or None, what describe_launch must report)"""
    return [(SMALL[0], None, LADDER[mode][0]), (SMALL[1], None, LADDER[mode][1]),
            (MULTI, MULTI_WAVE[mode], MULTI_WAVE[mode]), (SMALL[1], "stream", "stream"), (MULTI, "stream", "stream")]


def _set_opts(name, mode):
    """the set's options as keywords for Case.device"""
    return TABLE[name][1](mode)


def _central_bar(oracle, res, central, solve, what):
    q, _, _, it, st = central
    assert res.iterations[solve] == it[solve] and res.status[solve] == st[solve], (what, "central", solve)
    assert _rot_err(oracle, res.q[solve], q[solve]) <= 1e-6, (what, "central", solve)


def _bitwise(a, b, what, solves=None):
    for name in FIELDS:
        x, y = np.asarray(getattr(a, name)), np.asarray(getattr(b, name))
        if solves is not None:
            x, y = x[solves], y[solves]
        np.testing.assert_array_equal(x, y, err_msg=f"{what}: {name}")


@pytest.mark.parametrize("mode", FAMILIES, ids=FAMILY_IDS)
def test_every_option_set_on_every_launch_form(oracle, mode):
    """Each set of the table over its kept solves, on each form of the kernel, at the module's bars; the code the table
    fixes (ptol 1, gtol 2, r_capped 3 at the cap, minrad_at0 4 at iteration 0 with the start returned).  Then
    liveness on the device itself: per family every set changes count or code of a kept solve against the device's own
    default-options run of the same launch, and the edge values (1 / 0 and 1 / inf in make_args) change no bit."""
    defaults = {}
    live = {name: False for name in TABLE}
    for n, geom, expect in _forms(mode):
        for name, (start, _, code) in TABLE.items():
            case, mask, ref, central = table_run(oracle, name, mode, n)
            keep = np.flatnonzero(mask)
            what = f"{FAMILY_IDS[mode]} {name} n={n} {expect}"
            res, o = case.device(geometry=geom, expect=expect, **_set_opts(name, mode))
            _agree(oracle, res, ref, what, solves=keep)
            _central_bar(oracle, res, central, keep[0], what)
            if code is not None:
                assert (res.status[keep] == code).all(), (what, res.status)
            if name == "minrad_at0":
                assert (res.iterations[keep] == 0).all(), (what, res.iterations)
                q0 = case.q0 / np.linalg.norm(case.q0, axis=1, keepdims=True)
                # write_result: q0 * fast_rsqrt(|q0|^2), a reciprocal square root within an ulp of 1 and a product
                np.testing.assert_allclose(res.q[keep], q0[keep], rtol=0, atol=4e-16, err_msg=what)
            if (n, geom, start) not in defaults:
                defaults[(n, geom, start)] = case.device(geometry=geom, expect=expect)[0]
            dflt = defaults[(n, geom, start)]
            if name == EDGE:
                _bitwise(res, dflt, what + " against the default options")
            else:
                live[name] = live[name] or bool(((res.iterations != dflt.iterations) | (res.status != dflt.status))[keep].any())
    assert all(live[name] for name in TABLE if name != EDGE), (FAMILY_IDS[mode], live)


@pytest.mark.parametrize("mode", FAMILIES, ids=FAMILY_IDS)
def test_three_hypotheses_per_pair_with_options(oracle, mode):
    """n_hyp = 3 (the start and two translations within ~0.3 of it) under ptol, far_minrad and r0_small: the
    hypotheses of one block end after different counts and, under far_minrad, with different codes.  The
    pair-hypothesis kernel on a one-wavefront rung, the group kernel on the multi-wavefront geometry; against the
    oracle's own n_hyp / hyp_t solve over the solves kept for these starts."""
    for n, geom, expect in ((SMALL[1], None, LADDER[mode][1]), (MULTI, MULTI_WAVE[mode], MULTI_WAVE[mode])):
        for name in HYP_SETS:
            case, hyp, mask, ref, central = hyp_run(oracle, name, mode, n)
            keep = np.flatnonzero(mask)
            what = f"{FAMILY_IDS[mode]} {name} n_hyp=3 n={n} {expect}"
            res, o = case.device(geometry=geom, expect=expect, hyp_t=hyp, n_hyp=N_HYP, **_set_opts(name, mode))
            _agree(oracle, res, ref, what, solves=keep)
            _central_bar(oracle, res, central, keep[0], what)
            if TABLE[name][2] is not None:
                assert (res.status[keep] == TABLE[name][2]).all(), (what, res.status)


@pytest.mark.parametrize("mode", FAMILIES, ids=FAMILY_IDS)
def test_mixed_fates_in_one_launch(oracle, mode):
    """Sixteen solves in one launch (the near and the far starts of eight pairs) that end, side by side, converged (0),
    on the parameter tolerance (1), at the iteration cap (3) and below the minimum radius (4), at different
    iterations: against the oracle over the kept solves, and every solve -- kept or not -- with the bits it has when it
    is solved alone in a batch of one.  A wavefront that ends early disturbs neither its neighbours nor the block's
    exit."""
    for n, geom, expect in ((MIXED_SIZES[0], None, LADDER[mode][1]), (MIXED_SIZES[1], MULTI_WAVE[mode], MULTI_WAVE[mode]),
                            (MIXED_SIZES[0], "stream", "stream")):
        case, mask, ref, central = mixed_run(oracle, mode, n)
        keep = np.flatnonzero(mask)
        what = f"{FAMILY_IDS[mode]} mixed fates n={n} {expect}"
        kw = mixed_set(mode)
        res, o = case.device(geometry=geom, expect=expect, **kw)
        _agree(oracle, res, ref, what, solves=keep)
        _central_bar(oracle, res, central, keep[0], what)
        for fate in ({0}, {1, 2}, {3}, {4}):
            assert np.isin(res.status[keep], list(fate)).any(), (what, fate, res.status)
        for p in range(case.B):
            sl = slice(p * n, (p + 1) * n)
            one = Case(mode, case.f1[sl], case.f2[sl], None if case.c2 is None else case.c2[sl],
                       None if case.c1 is None else case.c1[sl], case.q0[p:p + 1], case.t0[p:p + 1], n)
            alone, _ = one.device(geometry=geom, expect=expect, **kw)
            for name in FIELDS:
                np.testing.assert_array_equal(np.asarray(getattr(alone, name))[0], np.asarray(getattr(res, name))[p],
                                              err_msg=f"{what}: solve {p} alone, {name}")


@pytest.mark.parametrize("mode", FAMILIES, ids=FAMILY_IDS)
def test_stream_handle_passes_the_options_through(oracle, mode):
    """pnec_hip_stream_submit with ptol, far_minrad and noscale: the batch path's bits (which
    test_every_option_set_on_every_launch_form holds to the oracle), so the handle hands the whole struct on"""
    for name in ("ptol", "far_minrad", "noscale"):
        for n in (SMALL[1], MULTI):
            case = inputs(mode, n, TABLE[name][0])
            res, o = case.device(**_set_opts(name, mode))
            dflt, _ = case.device()
            assert ((res.iterations != dflt.iterations) | (res.status != dflt.status)).any(), (name, n)
            _stream_handle_is_bitwise(case, res, o, f"{FAMILY_IDS[mode]} {name} n={n}")


def test_pipeline_passes_its_embedded_solve_options_through(oracle):
    """pnec_hip_solve_pipeline with ptol, far_minrad and noscale in pnec_hip_pipeline_options.solver: the bits of the
    stage-by-stage chain whose last stage runs with the same options (the pattern of test_streaming_gpu's
    test_pipeline_equals_the_stage_by_stage_chain_and_never_needs_host_sizes), on 6 pairs of about 200
    correspondences with a fifth of them outliers.  The refinement starts at the weighted eigensolver's pose there, so
    the sets that need a far start change little: ptol must change the result, which shows the comparison can fail."""
    sizes = [200, 193, 256, 129, 211, 180]
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    P = len(sizes)
    g = sim.generate(P, max(sizes), seed=595)
    rng = np.random.default_rng(12)
    f1 = np.concatenate([g.bvs1[p].numpy()[:n] for p, n in enumerate(sizes)])
    f2 = np.concatenate([g.bvs2[p].numpy()[:n] for p, n in enumerate(sizes)])
    c2 = np.concatenate([g.covs2[p].numpy()[:n] for p, n in enumerate(sizes)])
    for p in range(P):
        sl = np.arange(offsets[p], offsets[p + 1])
        bad = rng.choice(sl, len(sl) // 5, replace=False)
        v = rng.normal(size=(len(bad), 3))
        f2[bad] = v / np.linalg.norm(v, axis=1, keepdims=True)
    q0, t0 = g.init_q.numpy(), g.init_t.numpy()
    with Batch(TARGET, offsets) as b:
        b.fill(f1, f2, c2)
        qr, tr, mask, cnt, its = b.ransac_eigensolver(q0, seed=1)
        sel = b.select(mask)
        qw, tw = sel.weighted_eigensolver(qr, tr, 1e-13, 10)
        plain = sel.solve(qw, tw)
        for name in ("ptol", "far_minrad", "noscale"):
            o = options(name, TARGET)
            want = sel.solve(qw, tw, options=o)
            q, t = b.solve_pipeline(q0, t0, capi.default_pipeline_options(solver=o))
            np.testing.assert_array_equal(q, want.q, err_msg=name)
            np.testing.assert_array_equal(t, want.t, err_msg=name)
            if name == "ptol":
                assert ((want.status != plain.status) | (want.iterations != plain.iterations)).any(), (want.status, plain.status)
                assert not np.array_equal(want.q, plain.q)
        sel.close()


def test_numeric_jacobian_mode_with_options(oracle):
    """PNEC_HIP_OPT_JACOBIAN_NUMERIC_CENTRAL together with ptol and far_minrad (TARGET): the verification kernel runs
    the same lm_advance, so it follows the oracle's central-difference path under these options as it does under the
    defaults -- test_lm_branches' bar: equal counts and codes on every kept solve, rotation <= 1e-8 rad and the cost
    on the settled ones (test_lm_options_cpu.settled: the oracle's own two paths end within that bar of each other).
    At 100 and 600 correspondences: with 10 the pose two or three steps from a far start is too weakly determined for
    two difference quotients to agree on it (measured 1.04e-8 rad)."""
    for name in NUMERIC_SETS:
        for n in NUMERIC_SIZES:
            case, mask, ref, central = table_run(oracle, name, TARGET, n)
            keep = np.flatnonzero(mask)
            res, o = case.device(flags=capi.OPT_JACOBIAN_NUMERIC_CENTRAL, **_set_opts(name, TARGET))
            np.testing.assert_array_equal(res.iterations[keep], central[3][keep], err_msg=f"{name} n={n}")
            np.testing.assert_array_equal(res.status[keep], central[4][keep], err_msg=f"{name} n={n}")
            keep = np.flatnonzero(mask & settled(oracle, ref, central))
            print(f"numeric central {name} n={n}: solves {keep.tolist()}, worst cost difference "
                  f"{np.max(np.abs(res.cost[keep] / central[2][keep] - 1)):.2e} relative, worst rotation "
                  f"{max(_rot_err(oracle, res.q[s], central[0][s]) for s in keep):.2e} rad")
            # far_minrad ends mid-descent, where the cost is not stationary: what the two difference quotients leave of
            # a difference in the pose (1.7e-9 rad) shows in the cost at first order (measured 1.07e-8 relative, n = 100,
            # ended by code 4 at iteration 8 with cost 1.8e5); the converged ptol solves agree to 2.0e-10
            _agree(oracle, res, central, f"numeric central {name} n={n}", rot_tol=NUMERIC_ROT_BAR,
                   cost_rtol=1e-7 if name == "far_minrad" else 1e-9, solves=keep)
