"""The device's RANSAC (pnec_hip_ransac_eigensolver, and the RANSAC stage of pnec_hip_solve_pipeline) against the checker
at every RANSAC parameter the suite otherwise leaves at its default: sample_size (the register-held sample, the
duplicate-rejecting draw loop, the adaptive bound k = log(0.01) / log(1 - w^ss)), threshold (every count, best_count, k
and the number of rounds), max_iterations (the sequential rule ending inside a round of sixteen), seeds beyond 2^32, the
zero-inlier ending, n around the sample size, the two-pair kernel form, both memory spaces, the chain's options, refusals.

Iteration numbers, masks and counts are compared for EQUALITY.  That demand is fair because of what
test_ransac_options_cpu.py establishes for these very inputs from the checker alone: stable under one-ulp changes of the
bearings, and no compared score within REQUIRED_MARGIN of the threshold or within REQUIRED_RATIO error bounds of it; it
is asserted again here for every pair.  Poses get the slack
test_parity_gpu.test_ransac_eigensolver_and_inlier_selection_device_vs_oracle grants the eigensolver's stopping rule
(1e-7 rad), where the checker's own rotation moves less than 1e-9 rad under those one-ulp changes and there is an inlier
at all; elsewhere a finite unit quaternion and a finite unit t.

The translation is compared where, in addition, the inliers determine one.  It is the eigenvector of the smallest
eigenvalue of M = sum n n' over the inliers BUT THE FIRST (the reference's ComposeM, quirk C7): with one inlier M is the
zero matrix, with two it has rank one, and "the" eigenvector is whatever vector of a two- or three-dimensional null space
an eigen-decomposition happens to return -- the checker's Jacobi sweeps return a coordinate axis, the device something
else, both rightly.  From three inliers on M has rank two and the direction is the data's
(test_ransac_options_cpu.test_translation_is_the_datas_from_three_inliers_on holds the checker to that).

How many poses and translations each configuration must compare is written down (POSES_COMPARED): inputs that change so
that a configuration compares fewer fail the test rather than empty it."""
import os
import subprocess
import sys

import numpy as np
import pytest

from pnec_amd import Batch, capi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ransac_option_cases as rc  # noqa: E402
from test_ransac_options_cpu import REQUIRED_MARGIN, REQUIRED_RATIO  # noqa: E402  (derived next to the constants there)

pytestmark = pytest.mark.gpu

POSE_TOL = 1e-7           # rad, and |abs(t . t_o) - 1|: the stopping-rule slack of the existing RANSAC parity test
POSE_STABLE = 1e-9        # rad: the pose is compared where the checker's own rotation moves less than this under one ulp
T_DETERMINED = 3          # inliers from which M (composed without the first) has rank two: a translation exists
# (rotations, translations) each configuration compares, of its 16 pairs unless it has fewer: the pairs with an inlier and
# a rotation that holds still, and those of them with three inliers.  Counted from the checker's answers.
POSES_COMPARED = {"a-ss16": (15, 14), "b-thr3": (15, 15), "b-thr0": (0, 0), "c-max0": (6, 2), "c-max1": (11, 5),
                  "c-max15": (16, 9), "c-max16": (16, 9), "c-max17": (16, 9), "c-max31": (16, 9), "c-max32": (16, 9),
                  "c-max33": (16, 9), "d-ss16-thr1e-5": (3, 2), "e-ss5": (3, 2), "e-ss16": (3, 2), "h-ss16-max17": (15, 11),
                  "h-ss16-max33": (15, 11), "h-ss16-max40": (15, 11)}


def _quat_to_R(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _device(case):
    x = rc.inputs(case)
    with Batch(capi.MODE_TARGET, x.offsets) as b:
        b.fill(x.f1, x.f2, x.c2)
        return b.ransac_eigensolver(x.q0, seed=case.seed, **case.params)


def _compare(case, out, label=""):
    """every pair of the case against the checker -> the largest device-to-checker rotation difference among the pairs
    whose pose is compared (rad)"""
    q, t, mask, cnt, its = out
    x, ref = rc.inputs(case), rc.reference(case)
    worst, compared, t_compared = 0.0, 0, 0
    for p, r in enumerate(ref):
        where = (label or case.name, p, r.n)
        assert r.stable and r.margin >= REQUIRED_MARGIN and r.margin_ratio >= REQUIRED_RATIO, where  # the inputs
        sl = x.pair(p)
        assert its[p] == r.iterations, where + (int(its[p]), r.iterations)
        np.testing.assert_array_equal(mask[sl].astype(bool), r.mask, err_msg=str(where))
        assert cnt[p] == r.mask.sum(), where
        if cnt[p] > 0 and r.rotation_moves < POSE_STABLE:
            err = rc.rot_angle(_quat_to_R(q[p]), r.R)
            worst, compared = max(worst, err), compared + 1
            assert err <= POSE_TOL, where + (err,)
        else:
            assert np.isfinite(q[p]).all() and abs(np.linalg.norm(q[p]) - 1) < 1e-12, where + (q[p],)
        if cnt[p] >= T_DETERMINED and r.rotation_moves < POSE_STABLE:
            t_compared += 1
            assert abs(abs(t[p] @ r.t) - 1) < POSE_TOL, where + (t[p], r.t)
        else:
            assert np.isfinite(t[p]).all() and abs(np.linalg.norm(t[p]) - 1) < 1e-12, where + (t[p],)
    print(f"{label or case.name}: smallest margin {min(r.margin for r in ref):.3e} (ratio to the error bound "
          f"{min(r.margin_ratio for r in ref):.3g}), largest rotation difference {worst:.3e} rad over {compared} of "
          f"{len(ref)} pairs, t compared in {t_compared}, iterations {[r.iterations for r in ref]}")
    assert (compared, t_compared) == POSES_COMPARED.get(case.name, (16, 16)), (label or case.name, compared, t_compared)
    return worst


@pytest.mark.parametrize("case", rc.CASES_A, ids=lambda c: c.name)
def test_sample_size(case):
    """a: sample_size 5, 6, 8, 12, 16 at 25 % outliers; 12 and 16 capped at 300 iterations, where some pairs end"""
    _compare(case, _device(case))
    if case.sample_size == 16:
        assert any(r.iterations == case.max_iterations + 1 for r in rc.reference(case))


@pytest.mark.parametrize("case", rc.CASES_B, ids=lambda c: c.name)
def test_threshold(case):
    """b: thresholds through the inliers' own scores (1e-7 ... 1e-4), one that accepts everything (3.0), and 0.0: no
    inlier ever, best_count stays where the first model's zero put it, the ending with an empty inlier set"""
    _compare(case, _device(case))
    if case.threshold == 0.0:
        ref = rc.reference(case)
        assert all(r.iterations == case.max_iterations + 1 and not r.mask.any() for r in ref)


@pytest.mark.parametrize("case", rc.CASES_C, ids=lambda c: c.name)
def test_max_iterations_ends_the_rule_inside_a_round(case):
    """c: 45 % outliers keep the rule asking for more; max_iterations stops it at, just before and just after the end of
    a round of sixteen hypotheses (0, 1 | 15, 16, 17 | 31, 32, 33).  The expected number is the checker's."""
    _compare(case, _device(case))
    assert all(r.iterations == case.max_iterations + 1 for r in rc.reference(case))


@pytest.mark.parametrize("case", rc.CASES_D, ids=lambda c: c.name)
def test_largest_sample_with_few_inliers(case):
    """d: sample_size 16 at 45 % outliers: w^16 of a handful of inliers underflows towards the clamp of p_no"""
    _compare(case, _device(case))


@pytest.mark.parametrize("case", rc.CASES_E, ids=lambda c: c.name)
def test_pairs_around_the_sample_size(case):
    """e: n = ss - 1 (no sample can be drawn: it = 0, every point an inlier), ss (one possible sample: the draw loop
    rejects duplicates until it has all of them), ss + 1, an empty pair between them, and a pair of 1 100"""
    out = _device(case)
    _compare(case, out)
    ref = rc.reference(case)
    assert ref[0].iterations == 0 and ref[0].mask.all() and out[4][0] == 0 and out[3][0] == case.sample_size - 1
    assert out[3][2] == 0 and out[4][2] == 0                       # the empty pair


@pytest.mark.parametrize("case", rc.CASES_F, ids=lambda c: c.name)
def test_all_64_bits_of_the_seed_reach_the_hash(case):
    """f: seeds 0, 2^32 + 5 and 2^64 - 1 at sample_size 8"""
    _compare(case, _device(case))


def test_seeds_that_differ_only_above_bit_31_give_different_draws():
    """(f, the other way round: were the seed cut to 32 bits somewhere, 5 and 2^32 + 5 would draw alike -- on both sides
    if the checker cut it too)"""
    a, b = rc.CASES_F[1], rc.CASE_F_LOW
    assert any(ra.iterations != rb.iterations or (ra.mask != rb.mask).any()
               for ra, rb in zip(rc.reference(a), rc.reference(b)))
    _compare(b, _device(b))


def test_host_space_and_device_space_give_the_same_bytes():
    """g: configuration a at sample_size 6 through MEM_HOST (numpy) and MEM_DEVICE (torch tensors)"""
    import torch
    case = rc.CASE_G
    x = rc.inputs(case)
    with Batch(capi.MODE_TARGET, x.offsets) as b:
        b.fill(x.f1, x.f2, x.c2)
        host = b.ransac_eigensolver(x.q0, seed=case.seed, **case.params)
        dev = b.ransac_eigensolver(torch.from_numpy(x.q0.copy()).to("cuda:0"), seed=case.seed, **case.params)
        torch.cuda.synchronize()
        dev = tuple(v.cpu().numpy() for v in dev)
    for h, d in zip(host, dev):
        assert h.dtype == d.dtype and h.tobytes() == d.tobytes()
    _compare(case, dev, "g-device-space")


TWO_PAIR_CHILD = r'''
import os, sys
sys.path.insert(0, os.environ["PNEC_ROOT"])
sys.path.insert(0, os.path.join(os.environ["PNEC_ROOT"], "tests"))
import ransac_option_cases as rc
import test_ransac_options_gpu as tg
for case in rc.CASES_H:
    tg._compare(case, tg._device(case))
    its = [r.iterations for r in rc.reference(case)]
    assert its[0::2] == [case.max_iterations + 1] * 8 and max(its[1::2]) < 16, its   # partner done in round one
print("TWO_PAIR_OPTIONS_OK")
'''


def test_two_pair_form_with_a_lent_slot_stopped_by_max_iterations():
    """h: the two-pair kernel form (normally from 4 096 pairs up; forced for a fresh process).  Every second pair is clean
    and done within its first round, so its partner (45 % outliers) runs its second round over both slot groups: slot 0
    holds hypotheses 16 ... 31, the lent slot 1 holds 32 ... 47.  max_iterations = 17 ends the rule inside slot 0's sixteen
    (the lent slot's models must go unconsumed); 33 and 40 end it inside the LENT slot's, whose iteration number, stop
    and -- at 40 -- best model are handed back to the pair.  sample_size 5 and 16."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PNEC_ROOT=root, PNEC_RANSAC_FORM="2")
    r = subprocess.run([sys.executable, "-c", TWO_PAIR_CHILD], env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "TWO_PAIR_OPTIONS_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def test_chain_takes_its_ransac_options(oracle):
    """i: solve_pipeline with ransac_sample_size 6, ransac_threshold 1e-5, max_ransac_iterations 40, ransac_seed 2^40 + 1,
    first_pair_id 7 against oracle.solve_chain_batch given the same values: mask and count equal, the final rotation
    within test_frame_gpu's bound for the chain (1e-6 rad)."""
    case = rc.CASE_I
    x, ref = rc.inputs(case), rc.reference(case)
    opts = capi.default_pipeline_options(ransac_sample_size=case.sample_size, ransac_threshold=case.threshold,
                                         max_ransac_iterations=case.max_iterations, ransac_seed=case.seed,
                                         first_pair_id=case.first_pair_id)
    with Batch(capi.MODE_TARGET, x.offsets) as b:
        b.fill(x.f1, x.f2, x.c2)
        q, t, mask, cnt = b.solve_pipeline(x.q0, x.t0, options=opts, want_inliers=True)
    o = oracle.solve_chain_batch(x.offsets, x.f1, x.f2, x.c2, x.q0, seed=case.seed, first_pair_id=case.first_pair_id,
                                 max_ransac_iterations=case.max_iterations, sample_size=case.sample_size,
                                 threshold=case.threshold)
    worst = 0.0
    for p, r in enumerate(ref):
        assert r.stable and r.margin >= REQUIRED_MARGIN and r.margin_ratio >= REQUIRED_RATIO, p
        sl = x.pair(p)
        np.testing.assert_array_equal(o["mask"][sl], r.mask)               # the chain's checker is the stage's checker
        assert o["ransac_iterations"][p] == r.iterations
        np.testing.assert_array_equal(mask[sl].astype(bool), o["mask"][sl], err_msg=str((p, r.n)))
        assert cnt[p] == o["inlier_count"][p] == r.mask.sum(), (p, r.n)
        err = rc.rot_angle(_quat_to_R(q[p]), _quat_to_R(o["q"][p]))
        worst = max(worst, err)
        assert err <= 1e-6, (p, r.n, err)
    assert any(r.iterations < case.max_iterations for r in ref) and not all(r.mask.all() for r in ref)
    print(f"{case.name}: smallest margin {min(r.margin for r in ref):.3e} (ratio to the error bound "
          f"{min(r.margin_ratio for r in ref):.3g}), largest final rotation difference {worst:.3e} rad")


def test_refused_parameters_leave_the_batch_usable():
    """j: sample_size 0 and max_iterations -1 are invalid arguments, sample_size 17 is not built; a valid call on the same
    batch afterwards agrees with the checker"""
    case = rc.CASE_J
    x = rc.inputs(case)
    with Batch(capi.MODE_TARGET, x.offsets) as b:
        b.fill(x.f1, x.f2, x.c2)
        for kw, code in ((dict(sample_size=0), capi.ERR_INVALID_ARGUMENT), (dict(sample_size=17), capi.ERR_UNSUPPORTED),
                         (dict(max_iterations=-1), capi.ERR_INVALID_ARGUMENT)):
            with pytest.raises(capi.PnecHipError) as e:
                b.ransac_eigensolver(x.q0, seed=case.seed, **dict(case.params, **kw))
            assert e.value.code == code, (kw, e.value.code)
        out = b.ransac_eigensolver(x.q0, seed=case.seed, **case.params)
    _compare(case, out, "j-after-refusals")
