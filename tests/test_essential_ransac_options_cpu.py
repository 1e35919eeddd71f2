"""The conditions under which test_essential_ransac_options_gpu.py compares the device with the checker, asserted on the
checker itself and without a GPU.  For every algorithm and every case of tests/essential_ransac_option_cases.py: the
checker's two routes to the null space give the same run on every compared pair (so a device that differs adds something
beyond rounding); no row of a compared pair scores within 1e-12 of the threshold at the winning model (so no mask hangs on
a rounding); the cases reach what they are there for -- pairs ended by the cap and pairs ended by k, a winner without
inliers, a rule that ends before its first attempt; the checker obeys the call's own contract; and a seed or a pair id
cut to 32 bits draws another first sample on every pair of `seed64` (so the device test can see a truncation)."""
import numpy as np
import pytest

import essential_ransac_cases as rc
import essential_ransac_option_cases as oc

ALGORITHMS = pytest.mark.parametrize("algorithm", list(rc.ALGORITHMS), ids=[rc.NAMES[a] for a in rc.ALGORITHMS])
CASES = pytest.mark.parametrize("name", list(oc.CASE_NAMES))
LOW = 0xFFFFFFFF


# ---- 1. the inputs ----------------------------------------------------------------------------------------------------
@ALGORITHMS
def test_the_inputs_are_the_16_pairs_and_the_six_cases_of_the_description(algorithm):
    S, ps = rc.SAMPLE[algorithm], oc.pairs(algorithm)
    assert [p.n for p in ps] == [S, 63, 64, 65, 128, 129, 1000, 4097] * 2
    assert [p.share for p in ps] == [0.0] * 8 + [0.25] * 8
    for p in ps:
        assert int(p.planted.sum()) == int(round(p.share * p.n))
        assert np.all(np.isfinite(p.f1)) and np.all(np.isfinite(p.f2))
    table = {n: (c.threshold, c.max_iterations, c.seed, c.first_pair_id) for n, c in oc.CASES.items()}
    assert table == {"tight": (oc.TIGHT_THRESHOLD, 40, 1, 0), "loose": (1e-4, 40, 1, 0),
                     "seed64": (1e-6, 40, 2 ** 63 + 2 ** 40 + 5, 2 ** 33 + 7), "it1": (1e-6, 1, 1, 0),
                     "it3": (1e-6, 3, 3, 0), "it0": (1e-6, 0, 1, 0)}
    assert 4e-9 <= oc.TIGHT_THRESHOLD <= 6e-9      # about 5e-9: inside the inliers' scores
    assert oc.CASES["seed64"].seed > LOW and oc.CASES["seed64"].first_pair_id > LOW
    assert [p.n for p in oc.rotation_pairs(algorithm)] == [S, 40, 65, 300] == [p.n for p in oc.repeated_pairs(algorithm)]
    for p in oc.rotation_pairs(algorithm):
        # no baseline: f2 is R' f1 up to the noise
        assert np.abs(p.f2 - p.f1 @ p.R).max() <= 6.0 * rc.NOISE and np.allclose(np.linalg.norm(p.f2, axis=1), 1.0)
    for p in oc.repeated_pairs(algorithm):
        assert len(np.unique(np.hstack([p.f1, p.f2]), axis=0)) <= 3


# ---- 2. the two routes, the margin at the threshold, the contract ---------------------------------------------------------
@ALGORITHMS
@CASES
def test_both_routes_give_the_same_run_no_row_sits_at_the_threshold_and_the_contract_holds(algorithm, name):
    case, ps = oc.CASES[name], oc.pairs(algorithm)
    xs, ys = oc.expected(algorithm, name), oc.expected(algorithm, name, "svd")
    same = near = 0
    for i, (p, x, y) in enumerate(zip(ps, xs, ys)):
        ok = oc.same_run(x, y)
        same += ok
        if not ok:
            print(f"{rc.NAMES[algorithm]} {name} pair {i} (N = {p.n}): eigh {[x[k] for k in oc.DISCRETE]}, "
                  f"svd {[y[k] for k in oc.DISCRETE]}")
        if x["status"] != rc.ER_OK:
            continue
        at = oc.rows_at_the_threshold(p, x["R"], x["t"], case.threshold)
        if at:
            print(f"{rc.NAMES[algorithm]} {name} pair {i} (N = {p.n}): {at} rows within 1e-12 of the threshold")
        near += at
        rc.check_contract(p, algorithm, case.first_pair_id + i, x, x["R"], max_iterations=case.max_iterations,
                          threshold=case.threshold, seed=case.seed)
    print(f"{rc.NAMES[algorithm]} {name}: {same} of 16 pairs the same by both routes, {near} rows at the threshold")
    assert same == oc.N_PAIRS and near == 0


# ---- 3. what each case is there for ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(oc.CAPPED_CASES))
def test_the_cap_ends_some_pairs_and_k_ends_others(name):
    """Per algorithm the cap ends at least one pair of the case, and k at least one pair of `loose` and `seed64`.  In
    `tight` the seven- and eight-point models keep so few rows that the cap ends all their 16 pairs: there k ends a pair
    of the five-point solver."""
    case, ended_by_k = oc.CASES[name], 0
    for algorithm in rc.ALGORITHMS:
        ps, xs = oc.pairs(algorithm), oc.expected(algorithm, name)
        capped = [i for i, x in enumerate(xs) if oc.capped(x, case)]
        by_k = [i for i, (p, x) in enumerate(zip(ps, xs)) if oc.ended_by_k(x, p, algorithm, case)]
        print(f"{rc.NAMES[algorithm]} {name}: the cap ends pairs {capped}, k ends pairs {by_k}")
        assert all(x["status"] == rc.ER_OK for x in xs) and sorted(capped + by_k) == list(range(oc.N_PAIRS))
        assert len(capped) >= 1 and (len(by_k) >= 1 or name == "tight")
        ended_by_k += len(by_k)
        if name == "tight":
            # a large share of the rows on either side of the threshold: somewhere a winner keeps between a quarter and
            # three quarters of a long pair
            shares = [x["count"] / p.n for p, x in zip(ps, xs) if p.n >= 63]
            assert any(0.25 <= s <= 0.75 for s in shares), shares
    assert ended_by_k >= 1


def test_a_first_model_without_inliers_still_wins_at_one_iteration():
    zero = {a: [i for i, x in enumerate(oc.expected(a, "it1")) if x["status"] == rc.ER_OK and x["count"] == 0]
            for a in rc.ALGORITHMS}
    print("it1: ER_OK with count = 0 on pairs", {rc.NAMES[a]: v for a, v in zero.items()})
    assert sum(len(v) for v in zero.values()) >= 1
    for a, rows in zero.items():
        for i in rows:
            x = oc.expected(a, "it1")[i]
            assert not x["mask"].any() and 0 <= x["best_attempt"] < x["attempts"] and np.all(np.isfinite(x["R"]))


@ALGORITHMS
def test_the_caps_of_one_and_three_iterations_are_reached(algorithm):
    for name in ("it1", "it3"):
        case, xs = oc.CASES[name], oc.expected(algorithm, name)
        its = [int(x["iterations"]) for x in xs]
        print(f"{rc.NAMES[algorithm]} {name}: iterations {its}")
        assert all(x["status"] == rc.ER_OK for x in xs) and max(its) == case.max_iterations + 1 and min(its) >= 1


@ALGORITHMS
def test_no_iteration_allowed_means_no_attempt_and_no_model(algorithm):
    for p, x in zip(oc.pairs(algorithm), oc.expected(algorithm, "it0")):
        assert x["status"] == rc.ER_NO_MODEL and x["iterations"] == 0 and x["attempts"] == 0 and x["best_attempt"] == -1
        assert x["count"] == 0 and x["mask"].shape == (p.n,) and not x["mask"].any()
        assert all(np.isnan(x[k]).all() for k in ("R", "t", "E", "singular"))


# ---- 4. the seed and the pair id ------------------------------------------------------------------------------------------
@ALGORITHMS
def test_a_seed_or_a_pair_id_cut_to_32_bits_draws_another_first_sample_on_every_pair(algorithm):
    case, S = oc.CASES["seed64"], rc.SAMPLE[algorithm]
    for i, (p, x) in enumerate(zip(oc.pairs(algorithm), oc.expected(algorithm, "seed64"))):
        pid = case.first_pair_id + i
        for attempt in (0, int(x["best_attempt"])):
            full = rc.sample_of(case.seed, pid, attempt, p.n, S)
            # (N = S: every sample is a permutation of all rows, so it is the order that changes)
            assert full != rc.sample_of(case.seed & LOW, pid, attempt, p.n, S), (i, attempt)
            assert full != rc.sample_of(case.seed, pid & LOW, attempt, p.n, S), (i, attempt)
            assert full != rc.sample_of(case.seed & LOW, pid & LOW, attempt, p.n, S), (i, attempt)
            assert full != rc.sample_of(case.seed, i, attempt, p.n, S), (i, attempt)      # first_pair_id dropped
    # the high half alone is no seed either
    assert rc.sample_of(case.seed, case.first_pair_id, 0, 4097, S) != rc.sample_of(case.seed >> 32, case.first_pair_id, 0, 4097, S)


# ---- 5. pure rotation and repeated rows -----------------------------------------------------------------------------------
@ALGORITHMS
def test_pure_rotation_gives_the_same_run_by_both_routes_and_obeys_the_contract(algorithm):
    ps = oc.rotation_pairs(algorithm)
    xs, ys = oc.rotation_expected(algorithm), oc.rotation_expected(algorithm, "svd")
    for i, (p, x, y) in enumerate(zip(ps, xs, ys)):
        print(f"{rc.NAMES[algorithm]} pure rotation N = {p.n}: eigh {[x[k] for k in oc.DISCRETE]}, "
              f"svd {[y[k] for k in oc.DISCRETE]}")
        assert oc.same_run(x, y), i
        assert x["status"] == rc.ER_OK and oc.rows_at_the_threshold(p, x["R"], x["t"], rc.THRESHOLD) == 0
        rc.check_contract(p, algorithm, rc.FIRST_PAIR_ID + i, x, x["R"])


@ALGORITHMS
def test_the_checker_ends_on_repeated_rows_within_the_bounds_the_header_fixes(algorithm):
    """The two routes need not agree here (every sample is rank deficient: the null space is wider than the solver
    takes it to be), which is why the device test does not consult the checker on these pairs; what the header fixes for
    any input holds by either route."""
    for i, p in enumerate(oc.repeated_pairs(algorithm)):
        for route in ("eigh", "svd"):
            x = oc._ransac([p], algorithm, oc.DEFAULT, route)[0]
            assert x["status"] in (rc.ER_OK, rc.ER_NO_MODEL)
            assert x["attempts"] - x["iterations"] <= rc.SKIP_FACTOR * rc.MAX_ITERATIONS
            assert x["iterations"] <= rc.MAX_ITERATIONS + 1 and x["count"] == int(x["mask"].sum())
            if x["status"] == rc.ER_NO_MODEL:
                assert x["best_attempt"] == -1 and np.isnan(x["t"]).all()
