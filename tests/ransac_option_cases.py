"""Shared inputs and checker results of the RANSAC-option tests (test_ransac_options_cpu.py, test_ransac_options_gpu.py).

A case is one ragged TARGET batch with one RANSAC parameter set.  Pair p of a case holds `sizes[p]` correspondences of
sim.generate(1, n, seed=data_seed + p) with a share of gross outliers (frame-2 bearings replaced by uniform directions,
drawn as test_parity_gpu.test_ransac_scoring_tile_boundaries_and_early_drop_vs_oracle draws them), and is run by the
checker as pair_id first_pair_id + p.  The checker's answers are computed once per process and case and shared."""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass

import numpy as np

from pnec_amd import simulation as sim

# around the scoring tiles of 64, the 512 a wavefront keeps in registers, and beyond; 16 and 17 around the largest sample
SIZES = (16, 17, 40, 63, 64, 65, 100, 128, 129, 300, 511, 512, 513, 700, 1100, 33)
DEFAULT = dict(sample_size=10, threshold=1e-6, max_iterations=5000)


@dataclass(frozen=True)
class Case:
    name: str
    sizes: tuple = SIZES
    outliers: tuple | float = 0.25        # one share for every pair, or one per pair
    sample_size: int = 10
    threshold: float = 1e-6
    max_iterations: int = 5000
    seed: int = 3
    first_pair_id: int = 0
    data_seed: int = 900                  # (another one where a seed failed a precondition: said at the case)

    @property
    def params(self):
        return dict(sample_size=self.sample_size, threshold=self.threshold, max_iterations=self.max_iterations)


def _edge_sizes(ss):
    """config e: n = ss - 1 (no sample: the fallback), ss, ss + 1, an empty pair in the middle, one large pair"""
    return (ss - 1, ss, 0, ss + 1, 1100)


# ---- the configurations, by letter (a ... j) -----------------------------------------------------------------------
CASES_A = tuple(Case(f"a-ss{ss}", sample_size=ss, max_iterations=300 if ss >= 12 else 5000) for ss in (5, 6, 8, 12, 16))
# (seeds 4 at 1e-7 and 20 at 0.0 instead of 3: seed 3 failed a precondition there; test_ransac_options_cpu.py says which)
CASES_B = tuple(Case(f"b-thr{thr:g}", threshold=thr, max_iterations=300, seed=4 if thr == 1e-7 else 3)
                for thr in (1e-7, 1e-5, 1e-4, 3.0)) + (Case("b-thr0", threshold=0.0, max_iterations=20, seed=20),)
CASES_C = tuple(Case(f"c-max{m}", outliers=0.45, max_iterations=m) for m in (0, 1, 15, 16, 17, 31, 32, 33))
CASES_D = (Case("d-ss16-thr1e-5", sizes=SIZES[:4], outliers=0.45, sample_size=16, threshold=1e-5, max_iterations=200),)
CASES_E = tuple(Case(f"e-ss{ss}", sizes=_edge_sizes(ss), sample_size=ss, max_iterations=300) for ss in (5, 16))
CASES_F = tuple(Case(f"f-seed{s}", sample_size=8, seed=s) for s in (0, 2 ** 32 + 5, 2 ** 64 - 1))
CASE_F_LOW = Case("f-seed5", sample_size=8, seed=5)   # 2^32 + 5 cut to 32 bits: must NOT draw alike
# h: the two-pair kernel form.  Every second pair is clean and ends within its first round (hypotheses 0 ... 15); its
# partner in the wavefront (45 % outliers) runs its second round over both slot groups: slot 0 holds hypotheses 16 ... 31,
# the lent slot 1 holds 32 ... 47, consumed after slot 0's.
#   max_iterations = 17: the rule stops at it = 18, inside SLOT 0's sixteen; the lent slot's models are computed and must
#                        not be consumed (slot 0's stop suppresses slot 1).
#   max_iterations = 33: the rule stops at it = 34, on the second hypothesis of the LENT slot's sixteen; iteration number
#                        and stop are handed back from slot 1 to the pair (the best model is still slot 0's).
#   max_iterations = 40: it = 41, the lent slot's ninth; in pairs 0 and 6 (sample size 5) and 14 (16) the best model is one
#                        of hypotheses 32 ... 40 -- the lent slot's winner is handed back too
#                        (test_ransac_options_cpu.py checks that against the same inputs capped at 31).
CASES_H = tuple(Case(f"h-ss{ss}-max{m}", outliers=tuple(0.45 if p % 2 == 0 else 0.0 for p in range(len(SIZES))),
                     sample_size=ss, max_iterations=m) for ss in (5, 16) for m in (17, 33, 40))
# i: the chain's RANSAC options (solve_pipeline: ransac_sample_size, ransac_threshold, max_ransac_iterations, ransac_seed,
# first_pair_id)
CASE_I = Case("i-chain", sample_size=6, threshold=1e-5, max_iterations=40, seed=2 ** 40 + 1, first_pair_id=7)
CASE_G = CASES_A[1]                       # host space against device space: configuration a at sample_size 6
CASE_J = CASES_A[2]                       # the valid call after the refusals
ALL_CASES = CASES_A + CASES_B + CASES_C + CASES_D + CASES_E + CASES_F + (CASE_F_LOW,) + CASES_H + (CASE_I,)


@dataclass
class Inputs:
    offsets: np.ndarray    # [P + 1] int64
    f1: np.ndarray         # [M, 3]
    f2: np.ndarray
    c2: np.ndarray         # [M, 3, 3]
    R0: np.ndarray         # [P, 3, 3]
    q0: np.ndarray         # [P, 4] xyzw
    t0: np.ndarray         # [P, 3]

    def pair(self, p):
        return slice(int(self.offsets[p]), int(self.offsets[p + 1]))


@functools.lru_cache(maxsize=None)
def inputs(case: Case) -> Inputs:
    rng = np.random.default_rng(17)
    shares = case.outliers if isinstance(case.outliers, tuple) else (case.outliers,) * len(case.sizes)
    f1s, f2s, cvs, Rs, qs, ts = [], [], [], [], [], []
    for p, n in enumerate(case.sizes):
        g = sim.generate(1, max(n, 1), seed=case.data_seed + p)
        f2 = g.bvs2[0, :n].numpy().copy()
        bad = rng.choice(n, int(shares[p] * n), replace=False) if n else np.zeros(0, dtype=np.int64)
        v = rng.normal(size=(len(bad), 3))
        f2[bad] = v / np.linalg.norm(v, axis=1, keepdims=True)
        f1s.append(g.bvs1[0, :n].numpy().copy()); f2s.append(f2); cvs.append(g.covs2[0, :n].numpy().copy())
        Rs.append(g.init_R[0].numpy()); qs.append(g.init_q[0].numpy()); ts.append(g.init_t[0].numpy())
    out = Inputs(np.concatenate([[0], np.cumsum(case.sizes)]).astype(np.int64), np.concatenate(f1s), np.concatenate(f2s),
                 np.concatenate(cvs), np.stack(Rs), np.stack(qs), np.stack(ts))
    for a in (out.offsets, out.f1, out.f2, out.c2, out.R0, out.q0, out.t0):
        a.setflags(write=False)
    return out


def one_ulp_perturbations(f1, f2):
    """every bearing component moved to its neighbouring double: f1 up, f2 up, f2 down"""
    return ((np.nextafter(f1, 2.0), f2), (f1, np.nextafter(f2, 2.0)), (f1, np.nextafter(f2, -2.0)))


def rot_angle(Ra, Rb):
    """angle of Ra' Rb in rad, from the skew part (exact to first order where arccos of the trace loses eight digits)"""
    D = Ra.T @ Rb
    s = 0.5 * math.sqrt((D[2, 1] - D[1, 2]) ** 2 + (D[0, 2] - D[2, 0]) ** 2 + (D[1, 0] - D[0, 1]) ** 2)
    return math.atan2(s, 0.5 * (np.trace(D) - 1.0))


@dataclass
class PairReference:
    n: int
    R: np.ndarray
    t: np.ndarray
    mask: np.ndarray           # [n] bool
    iterations: int
    margin: float              # the checker's read-out: min |score - threshold| over everything the call compared
    margin_ratio: float        # ... as min |score - threshold| / (2 x the score's error bound)
    model_R: np.ndarray        # the model the final pass scored
    model_t: np.ndarray
    stable: bool               # mask and iteration number identical under the three one-ulp perturbations
    rotation_moves: float      # the largest change of the checker's own rotation under them, rad
    t_moves: float             # ... and of its translation, as |abs(t . t') - 1|


@functools.lru_cache(maxsize=None)
def reference(case: Case):
    """the checker on every pair of the case, and on its three one-ulp perturbations -> tuple of PairReference"""
    from oracle import pnec_oracle as oracle
    x = inputs(case)
    out = []
    for p, n in enumerate(case.sizes):
        sl = x.pair(p)
        kw = dict(seed=case.seed, pair_id=case.first_pair_id + p, **case.params)
        oracle.set_ransac_margin_tracking(True)     # (for the unperturbed run only: the bounds double its cost)
        try:
            R, t, mask, its = oracle.ransac_eigensolver(x.f1[sl], x.f2[sl], x.R0[p], **kw)
            margin, ratio = oracle.ransac_last_margin(), oracle.ransac_last_margin_ratio()
        finally:
            oracle.set_ransac_margin_tracking(False)
        mR, mt = oracle.ransac_last_model()
        stable, moves, t_moves = True, 0.0, 0.0
        for g1, g2 in (one_ulp_perturbations(x.f1[sl], x.f2[sl]) if n else ()):
            Rp, tp, mp, ip = oracle.ransac_eigensolver(g1, g2, x.R0[p], **kw)
            stable = stable and ip == its and bool((mp == mask).all())
            moves = max(moves, rot_angle(R, Rp))
            t_moves = max(t_moves, abs(abs(float(t @ tp)) - 1.0))
        out.append(PairReference(n, R, t, mask, its, margin, ratio, mR, mt, stable, moves, t_moves))
    return tuple(out)
