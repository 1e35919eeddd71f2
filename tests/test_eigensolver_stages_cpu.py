"""Preconditions of test_eigensolver_stages_gpu.py, from the checker alone (no GPU).  The GPU tests ask the device for the
checker's pose at tight bounds, for the same bits at different round counts, and rely on a parameter changing the answer;
each of those is only a fair demand of the INPUTS where the checker itself

  * is stable: its early-exit twin, started from a quaternion moved by 1e-12, ends within 1e-10 rad and 1e-10 in
    1 - |t . t'| of where it ends from the nominal start.  Asked of every pair under NEWTON and LM, and of at least 60 % of
    a case's pairs under DESCENT (nine or fifteen chained descents creep on at the rounding level of M; the share is
    test_opengv_schemes.test_ransac_and_weighted_stage_device_vs_checker's).  The GPU tests take the mask from here: it
    chooses the bound a DESCENT pair is held to, it excuses no pair;
  * shows the parameter: reg and the DESCENT round count move the rotation by far more than the bound the device is held
    to, and under NEWTON and LM the round count from two on does not move it at all;
  * agrees with itself: the literal loop and the twin lie within the declared early-exit bound.

None of these is a tolerance on the device.  A case that fails one needs another data seed (eigensolver_stage_cases), never
an excused pair."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eigensolver_stage_cases as ec  # noqa: E402
from test_parity_gpu import WEIGHTED_EARLY_EXIT_BOUND  # noqa: E402  (1e-7 rad, declared next to its measurement there)

VISIBLE_REG = 1e-6           # rad between reg = 1e-13 and reg = 1e-6: a hundred times the device's bound against the twin
VISIBLE_ROUND = 1e-7         # rad between neighbouring DESCENT round counts: ten times that bound
# NEWTON and LM from two rounds on: the twin keeps the rotation of its first converged call (the same Cayley vector, so
# the same bits) and only repeats the translation's fixed-point iteration, which stops at a step of 4e-15 per component
SAME_T = 1e-14

ANOTHER_SEED = "pick another data seed for this case in eigensolver_stage_cases.py"


def _share(mask):
    return f"{int(np.sum(mask))}/{len(mask)}"


@pytest.mark.parametrize("pairs,scheme", ec.PLAIN_SETS,
                         ids=[f"{len(p)}pairs-to{max(x.n for x in p)}-{ec.SCHEME_NAMES[s]}" for p, s in ec.PLAIN_SETS])
def test_plain_stage_is_stable_on_every_pair(pairs, scheme):
    refs = [ec.plain_reference(p, scheme) for p in pairs]
    print(f"plain stage, {len(pairs)} pairs, {ec.SCHEME_NAMES[scheme]}: stable {_share([r.stable for r in refs])}, the "
          f"answer moves by at most {max(r.rotation_moves for r in refs):.2e} rad, {max(r.t_moves for r in refs):.1e} in t")
    for p, r in zip(pairs, refs):
        assert r.stable, (ec.SCHEME_NAMES[scheme], p, r.rotation_moves, r.t_moves, ANOTHER_SEED)


@pytest.mark.parametrize("case", ec.ALL_CASES, ids=lambda c: c.name)
def test_weighted_stage_is_stable(case):
    ref = ec.reference(case)
    stable = ec.stable_mask(case)
    print(f"{case.name}: stable {_share(stable)}, the twin's answer moves by at most "
          f"{max(r.rotation_moves for r in ref):.2e} rad, {max(r.t_moves for r in ref):.1e} in t; not stable: "
          f"{[(p.n, float(f'{r.rotation_moves:.1e}')) for p, r in zip(case.pairs, ref) if not r.stable]}")
    if case.scheme == ec.DESCENT:
        assert stable.mean() >= ec.DESCENT_STABLE_SHARE, (case.name, _share(stable), ANOTHER_SEED)
    else:
        for p, r in zip(case.pairs, ref):
            assert r.stable, (case.name, p, r.rotation_moves, r.t_moves, ANOTHER_SEED)


@pytest.mark.parametrize("case", ec.ALL_CASES, ids=lambda c: c.name)
def test_literal_loop_and_twin_agree_within_the_declared_bound(case):
    ref = ec.reference(case)
    print(f"{case.name}: literal loop against twin at most {max(r.literal_apart for r in ref):.2e} rad, "
          f"{max(ec.t_distance(r.t, r.literal_t) for r in ref):.1e} in t")
    for p, r in zip(case.pairs, ref):
        assert r.literal_apart <= WEIGHTED_EARLY_EXIT_BOUND, (case.name, p, r.literal_apart, ANOTHER_SEED)


def test_reg_is_visible_in_the_rotation_and_large_reg_leaves_only_the_translation():
    """reg = 1e-13 against 1e-6: the rotations differ by more than VISIBLE_REG on at least half the pairs -- a kernel that
    dropped reg cannot pass both.  reg = 1e-2 swamps every weight's own term, the weights become equal and the rotation
    stays where the plain stage put it (<= 1e-12 rad: the start IS that minimiser) while the translation moves -- a kernel
    that added reg somewhere else than to the weight's denominator and B's diagonal would not show that."""
    by_reg = {c.reg: ec.reference(c) for c in ec.CASES_REG[:len(ec.REG_LADDER)]}
    pairs = ec.CASES_REG[0].pairs
    apart = np.array([ec.rot_angle(a.R, b.R) for a, b in zip(by_reg[1e-13], by_reg[1e-6])])
    print(f"a: rotation between reg 1e-13 and 1e-6: {apart.min():.1e} ... {apart.max():.1e} rad, above {VISIBLE_REG:g} in "
          f"{_share(apart > VISIBLE_REG)}")
    assert (apart > VISIBLE_REG).mean() >= 0.5, (apart, ANOTHER_SEED)
    for lo, hi in zip(ec.REG_LADDER[1:-1], ec.REG_LADDER[2:]):
        step = np.array([ec.rot_angle(a.R, b.R) for a, b in zip(by_reg[lo], by_reg[hi])])
        print(f"a: rotation between reg {lo:g} and {hi:g}: {step.min():.1e} ... {step.max():.1e} rad")
    stays = np.array([ec.rot_angle(r.R, ec.plain_reference(p, ec.NEWTON).R) for p, r in zip(pairs, by_reg[1e-2])])
    t_moves = np.array([ec.t_distance(r.t, ec.plain_reference(p, ec.NEWTON).t) for p, r in zip(pairs, by_reg[1e-2])])
    print(f"a: reg 1e-2 against the plain stage: rotation at most {stays.max():.1e} rad, t {t_moves.min():.1e} ... "
          f"{t_moves.max():.1e}")
    assert stays.max() <= 1e-12, (stays, ANOTHER_SEED)
    assert (t_moves > 1e-12).mean() >= 0.5, (t_moves, ANOTHER_SEED)


def test_every_descent_round_is_visible():
    """b, DESCENT: between neighbouring counts of the ladder (2|3, 3|9, 9|16) at least a third of the pairs that are
    stable at both counts differ by more than VISIBLE_ROUND -- a round too few or too many shows.  (0|1: both return the
    start; 1|2: the first round, far above every bound.)"""
    cases = {c.iterations: c for c in ec.CASES_ROUNDS[ec.DESCENT]}
    for lo, hi in ((2, 3), (3, 9), (9, 16)):
        both = ec.stable_mask(cases[lo]) & ec.stable_mask(cases[hi])
        apart = np.array([ec.rot_angle(a.R, b.R) for a, b in zip(ec.reference(cases[lo]), ec.reference(cases[hi]))])
        print(f"b-descent {lo}|{hi}: {apart.min():.1e} ... {apart.max():.1e} rad, above {VISIBLE_ROUND:g} in "
              f"{_share(apart[both] > VISIBLE_ROUND)} of the pairs stable at both")
        assert both.sum() >= 3 and (apart[both] > VISIBLE_ROUND).mean() >= 1.0 / 3.0, (lo, hi, apart, both, ANOTHER_SEED)


@pytest.mark.parametrize("scheme", [ec.NEWTON, ec.DESCENT, ec.LM], ids=lambda s: ec.SCHEME_NAMES[s])
def test_counts_zero_and_one_return_the_start_and_the_first_round_moves_it(scheme):
    cases = {c.iterations: c for c in ec.CASES_ROUNDS[scheme]}
    q0, t0 = ec.weighted_starts(cases[0].pairs, scheme)
    with ec.checker_scheme(scheme) as oracle:
        R0 = [oracle.rot_from_quat(q) for q in q0]
    for k in (0, 1):
        for p, r in enumerate(ec.reference(cases[k])):
            assert np.array_equal(r.R, R0[p]) and np.array_equal(r.t, t0[p]), (cases[k].name, p)
            assert np.array_equal(r.literal_R, R0[p]) and np.array_equal(r.literal_t, t0[p]), (cases[k].name, p)
    first = np.array([ec.rot_angle(a.R, b.R) for a, b in zip(ec.reference(cases[1]), ec.reference(cases[2]))])
    print(f"b-{ec.SCHEME_NAMES[scheme]} 1|2: the first round moves the rotation by {first.min():.1e} ... {first.max():.1e} rad")
    assert first.min() > VISIBLE_REG, (first, ANOTHER_SEED)


@pytest.mark.parametrize("scheme", [ec.NEWTON, ec.LM], ids=lambda s: ec.SCHEME_NAMES[s])
def test_newton_and_lm_return_one_pose_from_two_rounds_on(scheme):
    """b, NEWTON / LM: every pair's first call converges, so the twin's rotation at every count from 2 to 40 has the bits
    of count 2 and its translation lies within SAME_T -- which is why the device is asked for equal BITS between counts
    there, not for a distance; the literal loop stays within the declared bound of it."""
    cases = {c.iterations: c for c in ec.CASES_ROUNDS[scheme]}
    two = ec.reference(cases[2])
    for k in ec.ROUNDS_NEWTON_LM[3:]:
        ref = ec.reference(cases[k])
        t_apart = max(ec.t_distance(a.t, b.t) for a, b in zip(two, ref))
        lit = max(ec.rot_angle(a.R, b.literal_R) for a, b in zip(two, ref))
        print(f"b-{ec.SCHEME_NAMES[scheme]} 2|{k}: rotation "
              f"{max(ec.rot_angle(a.R, b.R) for a, b in zip(two, ref)):.1e} rad, t {t_apart:.1e}; literal loop {lit:.1e} rad")
        for p, (a, b) in enumerate(zip(two, ref)):
            assert np.array_equal(a.R, b.R), (cases[k].name, p, ANOTHER_SEED)
            assert ec.t_distance(a.t, b.t) <= SAME_T, (cases[k].name, p, ANOTHER_SEED)
        assert lit <= WEIGHTED_EARLY_EXIT_BOUND, (cases[k].name, lit)
