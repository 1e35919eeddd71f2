"""pnec_hip_essential_ransac away from the parameters of essential_ransac_cases: the inputs, the cases and the checker's
answers that test_essential_ransac_options_cpu.py and test_essential_ransac_options_gpu.py share.  Everything that
computes comes from essential_ransac_cases (draw, Pair, ransac_np, check_contract, sample_of, batch_arrays).

Per algorithm 16 pairs, N cycling through S (the sample itself), 63, 64, 65 (around one stride of the wavefront), 128,
129 (two strides and a rest), 1000 and 4097 (sixty-five trips of the scoring loop), eight without and eight with 25 % of
planted gross outliers.  A case is one launch of the 16 pairs with one parameter set:

  tight    a threshold inside the inliers' scores (some 5e-9 at noise of 1e-4): rows on both sides of it in every
           ballot, a small best share, k large -- the cap ends the rule
  loose    a threshold of 1e-4, which planted outliers pass too
  seed64   a seed and a first pair id that do not fit in 32 bits
  it1 it3  the cap after one and three iterations (`iterations` may be max_iterations + 1); a first model without
           inliers still wins
  it0      skip_limit = 10 max_iterations = 0: the rule ends before its first attempt, NO_MODEL with no attempt made

and two sets of pairs that are no generic two-view scene, at the parameters of essential_ransac_cases: pure rotation
(f2 = R' f1 with noise: no baseline, the essential matrix is undetermined) and repeated rows (every row one of three
distinct correspondences: every sample is rank deficient).  The checker's two routes to the null space disagree on
repeated rows, so those pairs are never compared with it.
"""
import functools
from dataclasses import dataclass

import numpy as np

import eight_point_cases as ec
import essential_ransac_cases as rc
import minimal_solver_cases as mc

DATA_SEED, ROTATION_SEED, REPEATED_SEED = 30301, 30302, 30303
N_PAIRS = 16
OUTLIER_SHARES = (0.0, 0.25)
LONG = (63, 64, 65, 128, 129, 1000, 4097)
DISCRETE = ("status", "iterations", "attempts", "best_attempt", "count")
MARGIN = 1e-12                    # check_contract's: a row this close to the threshold may fall on either side
# 5e-9, the middle of the inliers' scores, leaves one row of a SEVENPT pair within 1e-12 of the threshold at the
# checker's winning model, and 6e-9 one of SEVENPT and one of NISTER; at 4e-9 no row of any pair of the three is so close
TIGHT_THRESHOLD = 4e-9


@dataclass(frozen=True)
class Case:
    name: str
    threshold: float = rc.THRESHOLD
    max_iterations: int = rc.MAX_ITERATIONS
    seed: int = rc.SEED
    first_pair_id: int = rc.FIRST_PAIR_ID

    @property
    def params(self):
        return dict(seed=self.seed, max_iterations=self.max_iterations, threshold=self.threshold,
                    first_pair_id=self.first_pair_id)


CASES = {c.name: c for c in (
    Case("tight", threshold=TIGHT_THRESHOLD),
    Case("loose", threshold=1e-4),
    Case("seed64", seed=2 ** 63 + 2 ** 40 + 5, first_pair_id=2 ** 33 + 7),
    Case("it1", max_iterations=1),
    Case("it3", max_iterations=3, seed=3),
    Case("it0", max_iterations=0),
)}
CASE_NAMES = tuple(CASES)
DEFAULT = Case("default")         # the parameters of essential_ransac_cases: pure rotation and repeated rows run at them
CAPPED_CASES = ("tight", "loose", "seed64")     # each holds a pair ended by the cap and one ended by k


def sizes(algorithm):
    return (rc.SAMPLE[algorithm],) + LONG


def rotation_sizes(algorithm):
    return (rc.SAMPLE[algorithm], 40, 65, 300)


# ---- the inputs ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pairs(algorithm):
    return tuple(rc.draw(np.random.default_rng([DATA_SEED, algorithm, i]), sizes(algorithm)[i % 8],
                         OUTLIER_SHARES[i // 8]) for i in range(N_PAIRS))


@functools.lru_cache(maxsize=None)
def rotation_pairs(algorithm):
    """Four pairs without a baseline: the bearings and the rotation of ec.draw_pair, f2 = normalize(R' f1 + noise)."""
    out = []
    for i, n in enumerate(rotation_sizes(algorithm)):
        rng = np.random.default_rng([ROTATION_SEED, algorithm, i])
        f1, _, R, _ = ec.draw_pair(rng, n, 0.0)
        f2 = f1 @ R + rng.normal(scale=rc.NOISE, size=f1.shape)
        f2 /= np.linalg.norm(f2, axis=1)[:, None]
        out.append(rc.Pair(f1, f2, R, np.zeros(3)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def repeated_pairs(algorithm):
    """Four pairs whose rows are three distinct correspondences of a generic scene, repeated."""
    out = []
    for i, n in enumerate(rotation_sizes(algorithm)):
        rng = np.random.default_rng([REPEATED_SEED, algorithm, i])
        three = rc.draw(rng, 3, 0.0)
        idx = rng.integers(0, 3, n)
        out.append(rc.Pair(three.f1[idx], three.f2[idx], three.R, three.t))
    return tuple(out)


# ---- the checker's answers, once per process ---------------------------------------------------------------------------------
def _route(name):
    return {"eigh": mc.null_space_eigh, "svd": mc.null_space_svd}[name]


def _ransac(pair_list, algorithm, case, route):
    return tuple(rc.ransac_np(p.f1, p.f2, algorithm, seed=case.seed, pair_id=case.first_pair_id + i,
                              max_iterations=case.max_iterations, threshold=case.threshold, null_space=_route(route))
                 for i, p in enumerate(pair_list))


@functools.lru_cache(maxsize=None)
def expected(algorithm, name, route="eigh"):
    """ransac_np of the 16 pairs at the case `name`; route "svd" is the checker's second route (the CPU test's)."""
    return _ransac(pairs(algorithm), algorithm, CASES[name], route)


@functools.lru_cache(maxsize=None)
def rotation_expected(algorithm, route="eigh"):
    return _ransac(rotation_pairs(algorithm), algorithm, DEFAULT, route)


# ---- comparisons -------------------------------------------------------------------------------------------------------------
def same_run(x, y):
    """Whether two results of a pair agree in every discrete output and in the mask."""
    return all(int(x[k]) == int(y[k]) for k in DISCRETE) and np.array_equal(np.asarray(x["mask"]), np.asarray(y["mask"]))


def rows_at_the_threshold(p, R, t, threshold):
    """How many rows of the pair score within MARGIN of the threshold at the model (R, t)."""
    with np.errstate(invalid="ignore"):
        return int((np.abs(rc.scores_of(p.f1, p.f2, R, np.asarray(t)) - threshold) <= MARGIN).sum())


def capped(x, case):
    return int(x["iterations"]) == case.max_iterations + 1


def ended_by_k(x, p, algorithm, case):
    return (int(x["status"]) == rc.ER_OK and not capped(x, case)
            and int(x["iterations"]) >= rc.k_of(int(x["count"]), p.n, rc.SAMPLE[algorithm]))
