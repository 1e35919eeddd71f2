"""Shared inputs and checker answers of the eigensolver-stage tests (test_eigensolver_stages_cpu.py,
test_eigensolver_stages_gpu.py).

A pair is one outlier-free scene sim.generate(1, n, seed): every pair has its own scene, its own ground truth and its own
start rotation.  A case is a tuple of pairs run as one ragged batch with one parameter set of the weighted stage:
eigensolver scheme, reg, weighted_iterations.

The plain stage (nec_eigensolver) starts at the scene's start rotation.  The weighted stage starts where the checker's
plain stage ended under the same scheme (its rotation as a quaternion, its translation) -- the chain's order, and a start
that is the same array for the checker and for the device.

The checker's answers are computed once per process and (pair, parameter set) and shared: a pair that stands in several
batches (alone, among 15, among 33, ...) has one answer, which is what lets the GPU tests ask for the same pose wherever
the pair stands."""
from __future__ import annotations

import contextlib
import functools
import math
from dataclasses import dataclass

import numpy as np

from pnec_amd import simulation as sim

NEWTON, DESCENT, LM = 0, 1, 2                 # capi.ES_NEWTON / ES_DESCENT / ES_LM = the checker's scheme numbers
SCHEME_NAMES = {NEWTON: "newton", DESCENT: "descent", LM: "lm"}

STABLE_START_STEP = 1e-12                     # the start quaternion moves by this much ...
STABLE_BOUND = 1e-10                          # ... and a stable pair's answer by less than this (rad, and 1 - |t . t'|)
DESCENT_STABLE_SHARE = 0.6                    # of a case's pairs (test_opengv_schemes' share for chained descents)

# ---- the ladders -----------------------------------------------------------------------------------------------------
# sizes: below one wavefront's 64 lanes, around it, around the 512 a wavefront keeps resident, around the 1 024 of two;
# 1 025 is the one pair that makes a batch's n_max exceed 1 024
SIZE_LADDER = (8, 37, 63, 64, 65, 300, 511, 512, 513, 700, 1024, 1025)
PAIR_COUNTS = (1, 15, 16, 17, 33)             # around the sixteen pairs a minimising wavefront holds, and two of them + 1
REG_LADDER = (0.0, 1e-13, 1e-10, 1e-6, 1e-2)
ROUNDS_NEWTON_LM = (0, 1, 2, 3, 10, 16, 17, 40)
ROUNDS_DESCENT = (0, 1, 2, 3, 9, 16)          # (17 is refused: the descent keeps a minimiser per round, fifteen of them)
ROUNDS_DESCENT_REFUSED = 17


@dataclass(frozen=True)
class Pair:
    n: int
    seed: int


@dataclass(frozen=True)
class Case:
    name: str
    pairs: tuple
    scheme: int = NEWTON
    reg: float = 1e-13
    iterations: int = 10

    @property
    def sizes(self):
        return tuple(p.n for p in self.pairs)


def _pairs(sizes, data_seed):
    return tuple(Pair(n, data_seed + i) for i, n in enumerate(sizes))


# (data seeds: another one where a seed failed a precondition of test_eigensolver_stages_cpu.py -- said at the case)
LADDER_PAIRS = _pairs(SIZE_LADDER, 9300)                         # f, and c's three settings
TO_700_PAIRS = LADDER_PAIRS[:10] + _pairs((100, 200), 9320)      # a, b, e: twelve pairs spanning the ladder up to 700
COUNT_PAIRS = _pairs(tuple(64 + (7 * i) % 37 for i in range(33)), 9400)   # d: 33 pairs of 64 ... 100 correspondences
FORM_SIZES = (64, 300, 512, 513, 700, 1024)                      # c: the pairs followed through the three settings

CASES_REG = tuple(Case(f"a-reg{reg:g}", TO_700_PAIRS, reg=reg) for reg in REG_LADDER) + tuple(
    Case(f"a-reg1e-06-{SCHEME_NAMES[s]}", TO_700_PAIRS, scheme=s, reg=1e-6) for s in (LM, DESCENT))
CASES_ROUNDS = {s: tuple(Case(f"b-{SCHEME_NAMES[s]}-it{k}", TO_700_PAIRS, scheme=s, iterations=k)
                         for k in (ROUNDS_DESCENT if s == DESCENT else ROUNDS_NEWTON_LM)) for s in (NEWTON, DESCENT, LM)}
CASE_LADDER = Case("f-ladder", LADDER_PAIRS)                     # (c reads its pairs' answers from this one)
CASE_COUNTS = Case("d-counts", COUNT_PAIRS)
CASE_SPACES = CASES_REG[1]                                       # e: the defaults on the twelve pairs
ALL_CASES = CASES_REG + CASES_ROUNDS[NEWTON] + CASES_ROUNDS[DESCENT] + CASES_ROUNDS[LM] + (CASE_LADDER, CASE_COUNTS)
# the plain stage: (pairs, scheme) it runs on
PLAIN_SETS = tuple((COUNT_PAIRS, s) for s in (NEWTON, DESCENT, LM)) + ((LADDER_PAIRS, NEWTON), (TO_700_PAIRS, NEWTON))


def _oracle():
    from oracle import pnec_oracle as oracle
    return oracle


@contextlib.contextmanager
def checker_scheme(scheme):
    """the checker's scheme is process-wide: set for the block, back to the default after it"""
    oracle = _oracle()
    oracle.set_eigensolver_scheme(scheme)
    try:
        yield oracle
    finally:
        oracle.set_eigensolver_scheme(NEWTON)


def rot_angle(Ra, Rb):
    """angle of Ra' Rb in rad, from the skew part (exact to first order where arccos of the trace loses eight digits)"""
    D = Ra.T @ Rb
    s = 0.5 * math.sqrt((D[2, 1] - D[1, 2]) ** 2 + (D[0, 2] - D[2, 0]) ** 2 + (D[1, 0] - D[0, 1]) ** 2)
    return math.atan2(s, 0.5 * (np.trace(D) - 1.0))


def t_distance(ta, tb):
    """1 - |t . t'| of two unit translations (their sign is a convention)"""
    return abs(abs(float(ta @ tb)) - 1.0)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@dataclass
class PairInputs:
    f1: np.ndarray         # [n, 3]
    f2: np.ndarray
    c2: np.ndarray         # [n, 3, 3]
    q0: np.ndarray         # [4] xyzw: the scene's start rotation
    t0: np.ndarray         # [3]


@functools.lru_cache(maxsize=None)
def pair_inputs(pair: Pair) -> PairInputs:
    g = sim.generate(1, pair.n, seed=pair.seed)
    return PairInputs(*_frozen(g.bvs1[0].numpy().copy(), g.bvs2[0].numpy().copy(), g.covs2[0].numpy().copy(),
                               g.init_q[0].numpy().copy(), g.init_t[0].numpy().copy()))


def moved_start(pair: Pair, q):
    """q moved by STABLE_START_STEP in a direction of the pair's own, normalised"""
    d = np.random.default_rng(pair.seed).normal(size=4)
    q = q + STABLE_START_STEP * d / np.linalg.norm(d)
    return q / np.linalg.norm(q)


@dataclass
class PlainReference:
    R: np.ndarray
    t: np.ndarray
    q: np.ndarray              # R as a unit quaternion xyzw: with t, the weighted stage's start
    rotation_moves: float      # the checker's own answer under the moved start, rad
    t_moves: float
    stable: bool


@functools.lru_cache(maxsize=None)
def plain_reference(pair: Pair, scheme: int) -> PlainReference:
    """the checker's plain stage on the pair from the scene's start rotation, and from the moved one"""
    x = pair_inputs(pair)
    with checker_scheme(scheme) as oracle:
        R, t = oracle.nec_eigensolver(x.f1, x.f2, oracle.rot_from_quat(x.q0))
        Rm, tm = oracle.nec_eigensolver(x.f1, x.f2, oracle.rot_from_quat(moved_start(pair, x.q0)))
        q = oracle.quat_from_rot(R)
    q = q / np.linalg.norm(q)
    dr, dt = rot_angle(R, Rm), t_distance(t, tm)
    return PlainReference(*_frozen(R, t, q), dr, dt, dr <= STABLE_BOUND and dt <= STABLE_BOUND)


@dataclass
class WeightedReference:
    R: np.ndarray              # the early-exit twin: the device's control flow
    t: np.ndarray
    literal_R: np.ndarray      # the literal loop: the reference's
    literal_t: np.ndarray
    rotation_moves: float      # the twin's own answer under the moved start, rad
    t_moves: float
    stable: bool
    literal_apart: float       # twin against literal, rad


@functools.lru_cache(maxsize=None)
def weighted_reference(pair: Pair, scheme: int, reg: float, iterations: int) -> WeightedReference:
    """the checker's weighted stage on the pair from where its plain stage ended under the same scheme: the twin, the twin
    from the moved start, the literal loop"""
    x, s = pair_inputs(pair), plain_reference(pair, scheme)
    with checker_scheme(scheme) as oracle:
        R0 = oracle.rot_from_quat(s.q)
        R, t = oracle.weighted_eigensolver(x.f1, x.f2, x.c2, R0, s.t, reg, iterations, device_early_exits=True)
        Rm, tm = oracle.weighted_eigensolver(x.f1, x.f2, x.c2, oracle.rot_from_quat(moved_start(pair, s.q)), s.t, reg,
                                             iterations, device_early_exits=True)
        Rl, tl = oracle.weighted_eigensolver(x.f1, x.f2, x.c2, R0, s.t, reg, iterations)
    dr, dt = rot_angle(R, Rm), t_distance(t, tm)
    return WeightedReference(*_frozen(R, t, Rl, tl), dr, dt, dr <= STABLE_BOUND and dt <= STABLE_BOUND, rot_angle(R, Rl))


def reference(case: Case):
    """-> tuple of WeightedReference, one per pair of the case"""
    return tuple(weighted_reference(p, case.scheme, case.reg, case.iterations) for p in case.pairs)


def stable_mask(case: Case) -> np.ndarray:
    return np.array([r.stable for r in reference(case)])


@dataclass
class Inputs:
    offsets: np.ndarray    # [P + 1] int64
    f1: np.ndarray         # [M, 3]
    f2: np.ndarray
    c2: np.ndarray         # [M, 3, 3]
    q0: np.ndarray         # [P, 4] xyzw: the scenes' start rotations
    t0: np.ndarray         # [P, 3]


@functools.lru_cache(maxsize=None)
def inputs(pairs: tuple) -> Inputs:
    xs = [pair_inputs(p) for p in pairs]
    off = np.concatenate([[0], np.cumsum([p.n for p in pairs])]).astype(np.int64)
    return Inputs(*_frozen(off, np.concatenate([x.f1 for x in xs]), np.concatenate([x.f2 for x in xs]),
                           np.concatenate([x.c2 for x in xs]), np.stack([x.q0 for x in xs]), np.stack([x.t0 for x in xs])))


def weighted_starts(pairs: tuple, scheme: int):
    """-> (q [P, 4], t [P, 3]): where the checker's plain stage ended, the weighted stage's start"""
    refs = [plain_reference(p, scheme) for p in pairs]
    return np.stack([r.q for r in refs]), np.stack([r.t for r in refs])
