"""The table of LM option sets that tests/test_lm_options_gpu.py runs on the device, and the proof -- on the CPU oracle
alone -- that the table is fit to be a device test.

lm_advance (pnec_solve_kernel.hpp) reads thirteen fields of pnec_hip_options.  Each set below moves some of them off
the Ceres defaults; the device is compared with the oracle solve by solve, on equal iteration counts and termination
codes.  Such a comparison is only fair where the LM decisions do not sit at rounding level: two correct implementations
then take different paths.  So a solve belongs to a set only if it is ROBUST -- the oracle's analytic-Jacobian path and
its central-difference path (two implementations whose Jacobians differ by ~1e-9 relative) give the same iteration
count and the same code on it -- and this module asserts, as conditions on the table:

  robust   at most 2 of the 8 solves of a (set, family, size) are dropped; for the two far_minrad sets the analytic
           path must also keep code and count with the start translation moved by one ulp in every component;
  live     every set but the edge values changes count or code of at least one kept solve per family against the
           default options on the same inputs (an option the kernel ignored would be seen); the edge values (a zero
           minimum radius, infinite maxima: 1 / 0 and 1 / inf in make_args) change nothing at all;
  codes    over the kept solves every family ends in each of codes 0, 1, 2, 3 and 4, code 4 also after iteration 0.

`kept` is the one function that decides what is kept; the device module calls it too.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_lm_edges_gpu import FAMILIES, FAMILY_IDS, NEC, TARGET, Case, _axis_angle, _rot_err  # noqa: E402

from pnec_amd import capi  # noqa: E402
from pnec_amd import simulation as sim  # noqa: E402

INF = float("inf")
B = 8
# 10 and 100: one wavefront ((1, 1, 0) and (2, 1, 0) on every family's ladder); 600: MULTI_WAVE forced
SMALL, MULTI = (10, 100), 600
SIZES = SMALL + (MULTI,)
MAX_DROPPED = 2
MIN_RADIUS = 4   # PNEC_HIP_TERM_MIN_RADIUS


def _gtol(mode):
    # the gradient of the covariance families is ~1e6 times NEC's (residuals divided by sigma ~ 1e-3)
    return dict(function_tolerance=0.0, parameter_tolerance=0.0, gradient_tolerance=1e-3 if mode == NEC else 1.0)


# name -> (start, options(mode), the code every kept solve must end in or None)
TABLE = {
    "ftol": ("near", lambda m: dict(function_tolerance=1e-3), None),
    "ptol": ("near", lambda m: dict(function_tolerance=0.0, parameter_tolerance=1e-4), 1),
    "gtol": ("near", _gtol, 2),
    "r0_small": ("near", lambda m: dict(initial_trust_region_radius=1e-2), None),
    # a radius that can never grow: damped steps crawl; the first pair to converge needs 43 iterations, so all reach 40
    "r_capped": ("near", lambda m: dict(initial_trust_region_radius=1.0, max_trust_region_radius=1.0,
                                        max_num_iterations=40), 3),
    "minrad_at0": ("near", lambda m: dict(initial_trust_region_radius=1e-2, min_trust_region_radius=1.0), MIN_RADIUS),
    # 0.6 of the start radius: the first rejected step (radius / 2) ends the solve
    "far_minrad": ("far", lambda m: dict(min_trust_region_radius=6e3), None),
    "far_minrad1e3": ("far", lambda m: dict(min_trust_region_radius=1e3), None),
    "far_mrd": ("far", lambda m: dict(min_relative_decrease=0.5), None),
    "far_maxrad": ("far", lambda m: dict(max_trust_region_radius=1e4), None),
    "clamp_min": ("near", lambda m: dict(min_lm_diagonal=1.0), None),
    "clamp_max": ("near", lambda m: dict(max_lm_diagonal=1e-3), None),
    # without the scaling diag(J'J) is ~1e2 (NEC) to ~1e8; with it s^2 H_ii = H_ii / (1 + sqrt(H_ii))^2 < 1, so a
    # maximum of 1 bites only when jacobi_scaling = 0 is honoured
    "noscale": ("far", lambda m: dict(jacobi_scaling=0, max_lm_diagonal=1.0), None),
    "edge_values": ("near", lambda m: dict(min_trust_region_radius=0.0, max_trust_region_radius=INF,
                                           max_lm_diagonal=INF), None),
}
# the fates of one launch, side by side: near and far starts of the same pairs in one batch of 16, a first rejected
# step ends a solve (4), a parameter tolerance between the default's and ptol's splits the converging ones into 0 and
# 1, and the cap is low enough to stop the slow ones (3).  The cap is the family's own: NEC's slow pairs are done by
# iteration 8, TARGET's first rejected step at n = 600 comes at iteration 8
MIXED = "mixed_fates"
MIXED_SIZES = (100, MULTI)


def mixed_set(mode):
    return dict(min_trust_region_radius=6e3, parameter_tolerance=1e-7, max_num_iterations=10 if mode == TARGET else 7)


EDGE = "edge_values"
HYP_SETS = ("ptol", "far_minrad", "r0_small")
N_HYP = 3
ULP_SETS = ("far_minrad", "far_minrad1e3")

_cases, _runs = {}, {}


def inputs(mode, n, start):
    """sim.generate(8, n, seed=500 + n) as a Case of the family; "far": init_q turned by 0.3 rad about a seeded random
    axis, init_t + 0.8 N(0, I) renormalised"""
    key = (mode, n, start)
    if key not in _cases:
        case = Case.sim(mode, B, n, seed=500 + n)
        if start == "far":
            rng = np.random.default_rng(1500 + n)
            q0 = np.empty_like(case.q0)
            for p in range(B):
                r, q = _axis_angle(rng.normal(size=3), 0.3), case.q0[p]
                q0[p] = [*(r[3] * q[:3] + q[3] * r[:3] + np.cross(r[:3], q[:3])), r[3] * q[3] - r[:3] @ q[:3]]
            t0 = case.t0 + 0.8 * rng.normal(size=(B, 3))
            case.q0, case.t0 = q0, t0 / np.linalg.norm(t0, axis=1, keepdims=True)
        _cases[key] = case
    return _cases[key]


def mixed_inputs(mode, n):
    """the near and the far starts of inputs(mode, n, .) as one batch of 16"""
    key = (mode, n, MIXED)
    if key not in _cases:
        a, b = inputs(mode, n, "near"), inputs(mode, n, "far")
        cat = lambda x, y: None if x is None else np.concatenate([x, y])  # noqa: E731
        _cases[key] = Case(mode, cat(a.f1, b.f1), cat(a.f2, b.f2), cat(a.c2, b.c2), cat(a.c1, b.c1), cat(a.q0, b.q0),
                           cat(a.t0, b.t0), n)
    return _cases[key]


def hypotheses(case, n):
    """three start translations per pair: the start itself and two within ~0.3 of it"""
    rng = np.random.default_rng(2500 + n)
    hyp = np.repeat(case.t0, N_HYP, axis=0) + 0.3 * rng.normal(size=(N_HYP * case.B, 3))
    hyp /= np.linalg.norm(hyp, axis=1, keepdims=True)
    hyp[::N_HYP] = case.t0
    return hyp


def options(name, mode, **more):
    """the set's device options (pnec_hip_default_options is host code: no GPU is needed to fill the struct)"""
    return capi.default_options(**TABLE[name][1](mode), **more)


def kept(oracle, case, o, ulp=False, hyp_t=None, n_hyp=1):
    """-> (mask [solves] of the robust solves, the analytic path's solve_batch tuple, the central path's).  Robust: the oracle's analytic and
    central-difference paths end after the same number of iterations with the same code; with `ulp`, the analytic
    path also does from the start translations one ulp up and one ulp down in every component."""
    ref = case.oracle(oracle, o, oracle.JAC_ANALYTIC, hyp_t=hyp_t, n_hyp=n_hyp)
    runs = [case.oracle(oracle, o, oracle.JAC_NUMERIC_CENTRAL, hyp_t=hyp_t, n_hyp=n_hyp)]
    if ulp:
        for toward in (INF, -INF):
            if hyp_t is None:
                runs.append(case.oracle(oracle, o, oracle.JAC_ANALYTIC, t0=np.nextafter(case.t0, toward)))
            else:
                runs.append(case.oracle(oracle, o, oracle.JAC_ANALYTIC, hyp_t=np.nextafter(hyp_t, toward), n_hyp=n_hyp))
    mask = np.ones(len(ref[3]), dtype=bool)
    for r in runs:
        mask &= (r[3] == ref[3]) & (r[4] == ref[4])
    return mask, ref, runs[0]


NUMERIC_SETS, NUMERIC_SIZES, NUMERIC_ROT_BAR = ("ptol", "far_minrad"), (100, MULTI), 1e-8


def settled(oracle, ref, central, bar=NUMERIC_ROT_BAR):
    """mask of the solves on which the oracle's own two paths end within `bar` rad of each other.  Their Jacobians
    differ by ~1e-9 relative, as those of any two difference quotients do; a solve that ends mid-descent after a
    trajectory that amplifies this beyond the bar (1.3e-6 rad on one far_minrad pair at n = 600, equal counts and
    codes) cannot be held to the bar between the device's quotient and the oracle's either."""
    return np.array([_rot_err(oracle, ref[0][s], central[0][s]) <= bar for s in range(len(ref[3]))])


def table_run(oracle, name, mode, n):
    """(case, mask, analytic reference, central reference) of one (set, family, size), computed once per session"""
    key = (name, mode, n)
    if key not in _runs:
        case = inputs(mode, n, TABLE[name][0])
        mask, ref, central = kept(oracle, case, options(name, mode), ulp=name in ULP_SETS)
        _runs[key] = (case, mask, ref, central)
    return _runs[key]


def mixed_run(oracle, mode, n):
    key = (MIXED, mode, n)
    if key not in _runs:
        case = mixed_inputs(mode, n)
        _runs[key] = (case,) + kept(oracle, case, capi.default_options(**mixed_set(mode)), ulp=True)
    return _runs[key]


def hyp_run(oracle, name, mode, n):
    """(case, hyp_t, mask, analytic reference, central reference) of a set run from three hypotheses per pair"""
    key = ("hyp", name, mode, n)
    if key not in _runs:
        case = inputs(mode, n, TABLE[name][0])
        hyp = hypotheses(case, n)
        _runs[key] = (case, hyp) + kept(oracle, case, options(name, mode), ulp=name in ULP_SETS, hyp_t=hyp, n_hyp=N_HYP)
    return _runs[key]


def default_run(oracle, mode, n, start):
    key = ("default", mode, n, start)
    if key not in _runs:
        case = inputs(mode, n, start)
        _runs[key] = case.oracle(oracle, capi.default_options(), oracle.JAC_ANALYTIC)
    return _runs[key]


@pytest.mark.parametrize("mode", FAMILIES, ids=FAMILY_IDS)
def test_every_set_keeps_at_least_six_of_eight_solves(oracle, mode):
    for name in TABLE:
        for n in SIZES:
            _, mask, ref, _ = table_run(oracle, name, mode, n)
            assert B - int(mask.sum()) <= MAX_DROPPED, (name, FAMILY_IDS[mode], n, mask, ref[3], ref[4])


@pytest.mark.parametrize("mode", FAMILIES, ids=FAMILY_IDS)
def test_every_set_changes_a_kept_solve_and_the_edge_values_change_nothing(oracle, mode):
    for name, (start, _, _) in TABLE.items():
        live = False
        for n in SIZES:
            _, mask, ref, _ = table_run(oracle, name, mode, n)
            dflt = default_run(oracle, mode, n, start)
            if name == EDGE:
                assert mask.all(), (FAMILY_IDS[mode], n, mask)
                for a, b in zip(ref, dflt):
                    np.testing.assert_array_equal(a, b, err_msg=f"{FAMILY_IDS[mode]} n={n}")
            else:
                live = live or bool((((ref[3] != dflt[3]) | (ref[4] != dflt[4])) & mask).any())
        assert live or name == EDGE, (name, FAMILY_IDS[mode])


@pytest.mark.parametrize("mode", FAMILIES, ids=FAMILY_IDS)
def test_the_kept_solves_end_in_every_code_and_in_the_code_the_table_fixes(oracle, mode):
    seen, late_min_radius = set(), False
    for name, (_, _, code) in TABLE.items():
        for n in SIZES:
            _, mask, ref, _ = table_run(oracle, name, mode, n)
            it, st = ref[3][mask], ref[4][mask]
            seen |= set(int(s) for s in st)
            late_min_radius = late_min_radius or bool(((st == MIN_RADIUS) & (it > 0)).any())
            if code is not None:
                assert (st == code).all(), (name, FAMILY_IDS[mode], n, st)
            if name == "minrad_at0":
                assert (it == 0).all(), (FAMILY_IDS[mode], n, it)
                # nothing moved: q is the normalised start
                q0 = inputs(mode, n, "near").q0
                np.testing.assert_allclose(ref[0][mask], (q0 / np.linalg.norm(q0, axis=1, keepdims=True))[mask], rtol=0,
                                           atol=2e-16)
            if name == "r_capped":
                assert (it == 40).all(), (FAMILY_IDS[mode], n, it)
    assert seen >= {0, 1, 2, 3, 4}, (FAMILY_IDS[mode], seen)
    assert late_min_radius, FAMILY_IDS[mode]


def test_the_screen_drops_what_is_decided_by_rounding(oracle):
    """The screen is not vacuous: with all three tolerances at 0 the solve runs on until a step no longer changes
    the cost's bits, which no two implementations decide alike -- such a set would not be kept."""
    o = capi.default_options(function_tolerance=0.0, gradient_tolerance=0.0, parameter_tolerance=0.0)
    dropped = sum(B - int(kept(oracle, inputs(mode, n, "near"), o)[0].sum()) for mode in FAMILIES for n in SIZES)
    assert dropped > MAX_DROPPED * len(FAMILIES) * len(SIZES), dropped


@pytest.mark.parametrize("mode", FAMILIES, ids=FAMILY_IDS)
def test_mixed_fates_and_hypotheses_are_robust_and_mixed(oracle, mode):
    for n in MIXED_SIZES:
        _, mask, ref, _ = mixed_run(oracle, mode, n)
        assert 2 * B - int(mask.sum()) <= 2 * MAX_DROPPED, (FAMILY_IDS[mode], n, mask)
        st = ref[4][mask]
        for fate in ({0}, {1, 2}, {3}, {4}):
            assert np.isin(st, list(fate)).any(), (FAMILY_IDS[mode], n, fate, ref[4], mask)
        for name in HYP_SETS:
            _, _, hmask, href, _ = hyp_run(oracle, name, mode, n)
            assert N_HYP * B - int(hmask.sum()) <= N_HYP * MAX_DROPPED, (name, FAMILY_IDS[mode], n, hmask)
            if name == "far_minrad":   # the hypotheses of one block end differently
                st3 = np.where(hmask, href[4], -1).reshape(B, N_HYP)
                assert any(len(set(row[row >= 0])) > 1 for row in st3), (FAMILY_IDS[mode], n, st3)


def test_the_numeric_mode_cases_are_settled_on_the_oracle(oracle):
    """The solves the device's numeric-Jacobian mode is compared on: kept, and the oracle's analytic and central
    paths end within the comparison's own bar of each other.  At most 2 of 8 go, and far_minrad keeps solves that end
    below the minimum radius mid-solve."""
    for name in NUMERIC_SETS:
        for n in NUMERIC_SIZES:
            _, mask, ref, central = table_run(oracle, name, TARGET, n)
            keep = mask & settled(oracle, ref, central)
            assert B - int(keep.sum()) <= MAX_DROPPED, (name, n, keep)
            if name == "far_minrad":
                assert ((ref[4] == MIN_RADIUS) & (ref[3] > 0) & keep).any(), (n, ref[4], keep)
