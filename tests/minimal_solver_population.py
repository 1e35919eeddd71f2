"""Populations of scenes for the minimal solvers and the eight-point: cells of 48 pairs each, and the checker's answers.

tests/minimal_solver_cases.py and tests/eight_point_cases.py compare one pair per size, all from draw_pair, all filtered
to be tame.  A fault that shows on a few percent of the inputs -- a Sturm chain that miscounts near a small leading
coefficient, a root at zero or next to Cauchy's bound, a degree that drops by two -- passes there.  Here every cell is a
population from one seed: four kinds of scene (generic, forward, sideways, planar), the minimal count and the first size
with a one-dimensional null space (noise-free, so the scene's E is W itself and the wanted root sits at about 0), and
nothing is drawn again because it is hard: a pair is *kept* for the comparison with the checker when the checker's own
conditions hold (mc.conditions without `count` and `xyz`: few solutions and large |xyz| are wanted here), and the pairs
that are not kept still run in the same launch and must satisfy the structural contract of the header.

Everything here is decided by numpy alone; each cell is computed once per process (lru_cache) and shared by
test_minimal_population_cpu.py and test_minimal_population_gpu.py.  How many pairs each cell keeps, and how many of them
it compares for choice and pose, is written down (KEPT): inputs that change fail the CPU test rather than empty a cell.
"""
import dataclasses
import functools
import types

import numpy as np

import eight_point_cases as ec
import minimal_solver_cases as mc

NISTER, SEVENPT, EIGHTPT = mc.NISTER, mc.SEVENPT, 8
NAMES = {NISTER: "NISTER", SEVENPT: "SEVENPT", EIGHTPT: "EIGHTPT"}
KINDS = ("generic", "forward", "sideways", "planar")
CELL_PAIRS = 48
KEPT_MIN = 16                 # a third of a cell
KEPT_MIN_EIGHT_8 = 6          # the eight-point at N = 8, noise-free: the quality margin of 1 holds on a fifth of the pairs
ALONE = 3                     # pairs of a cell that also run alone
OFF_AXIS = 0.02               # forward / sideways: the other two components of t, times a standard normal


@dataclasses.dataclass(frozen=True)
class Cell:
    algorithm: int
    kind: str
    n: int
    noise: float
    draw: int = 0             # which population of this kind: the seed's last word

    @property
    def name(self):
        return f"{NAMES[self.algorithm]}-n{self.n}-{self.kind}"

    @property
    def seed(self):
        return [20265, self.algorithm, KINDS.index(self.kind), self.n, self.draw]

    @property
    def kept_min(self):
        return KEPT_MIN_EIGHT_8 if (self.algorithm == EIGHTPT and self.n == 8) else KEPT_MIN


CELLS = (
    Cell(NISTER, "generic", 5, 0.0), Cell(NISTER, "forward", 5, 0.0), Cell(NISTER, "sideways", 5, 0.0),
    Cell(NISTER, "planar", 5, 0.0), Cell(NISTER, "generic", 8, 0.0), Cell(NISTER, "forward", 64, 0.0),
    Cell(SEVENPT, "generic", 7, 0.0), Cell(SEVENPT, "forward", 7, 0.0), Cell(SEVENPT, "sideways", 7, 0.0),
    Cell(SEVENPT, "generic", 8, 0.0), Cell(SEVENPT, "forward", 64, 0.0),
    Cell(EIGHTPT, "generic", 64, ec.NOISE), Cell(EIGHTPT, "forward", 64, ec.NOISE), Cell(EIGHTPT, "sideways", 64, ec.NOISE),
    Cell(EIGHTPT, "generic", 8, 0.0),
)
MINIMAL_CELLS = tuple(c for c in CELLS if c.algorithm != EIGHTPT)
EIGHT_CELLS = tuple(c for c in CELLS if c.algorithm == EIGHTPT)
BY_NAME = {c.name: c for c in CELLS}

# (kept, compared for choice and pose) of the 48 pairs of every cell, counted from the checker's answers
KEPT = {
    "NISTER-n5-generic": (41, 41), "NISTER-n5-forward": (31, 31), "NISTER-n5-sideways": (44, 44),
    "NISTER-n5-planar": (22, 22), "NISTER-n8-generic": (46, 42), "NISTER-n64-forward": (47, 44),
    "SEVENPT-n7-generic": (27, 27), "SEVENPT-n7-forward": (18, 18), "SEVENPT-n7-sideways": (32, 32),
    "SEVENPT-n8-generic": (37, 37), "SEVENPT-n64-forward": (44, 44),
    "EIGHTPT-n64-generic": (48, 48), "EIGHTPT-n64-forward": (48, 48), "EIGHTPT-n64-sideways": (48, 48),
    "EIGHTPT-n8-generic": (13, 13),
}


# ---- scenes ------------------------------------------------------------------------------------------------------------
def scene(rng, kind, n, noise):
    """draw_pair's conventions (x1 = R x2 + t, a rotation of up to 0.1 rad, the box of points, unit bearings) with
    generic   draw_pair itself
    forward   t = normalise(0.02 g, 0.02 g, 1), g standard normal
    sideways  t = normalise(1, 0.02 g, 0.02 g)
    planar    a generic t, the points on the plane z = 6 + 0.1 x
    -> (f1 [n,3], f2 [n,3], R, t)."""
    if kind == "generic":
        return ec.draw_pair(rng, n, noise)
    axis = rng.normal(size=3)
    R = ec.rotation_from_vector(axis / np.linalg.norm(axis) * rng.uniform(0.0, 0.1))
    g = rng.normal(size=3)
    if kind == "forward":
        t = np.array([OFF_AXIS * g[0], OFF_AXIS * g[1], 1.0])
    elif kind == "sideways":
        t = np.array([1.0, OFF_AXIS * g[0], OFF_AXIS * g[1]])
    elif kind == "planar":
        t = g
    else:
        raise ValueError(kind)
    t = t / np.linalg.norm(t)
    x, y, z = rng.uniform(-2.0, 2.0, n), rng.uniform(-2.0, 2.0, n), rng.uniform(4.0, 8.0, n)
    if kind == "planar":
        z = 6.0 + 0.1 * x
    return bearings(np.column_stack([x, y, z]), R, t, rng, noise)


def bearings(x1, R, t, rng=None, noise=0.0):
    """The unit bearings of the points x1 (frame 1) in both frames, draw_pair's way -> (f1, f2, R, t)."""
    x2 = (x1 - t[None, :]) @ R
    f1 = x1 / np.maximum(np.linalg.norm(x1, axis=1), 1e-300)[:, None]
    f2 = x2 / np.maximum(np.linalg.norm(x2, axis=1), 1e-300)[:, None]
    if noise > 0.0 and len(x1):
        f1 = f1 + rng.normal(scale=noise, size=f1.shape)
        f2 = f2 + rng.normal(scale=noise, size=f2.shape)
        f1 /= np.linalg.norm(f1, axis=1)[:, None]
        f2 /= np.linalg.norm(f2, axis=1)[:, None]
    return f1, f2, R, t


def true_e(f1, f2, R, t):
    """The scene's essential matrix [t]x R as the header's e (f1' E f2 = 0), normalised.  The orientation is checked by
    |A e|: the transposed matrix leaves a residual of the order of the rotation, this one of the order of the rounding."""
    tx = np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])
    E = tx @ R
    A = mc.rows_of_a(f1, f2)
    r, r_t = np.linalg.norm(A @ E.reshape(9)), np.linalg.norm(A @ E.T.reshape(9))
    return mc.normalise(E.reshape(9)), float(r), float(r_t)


def transposed(sols):
    """Every e of a solution set reshaped to 3 x 3, transposed and normalised again: the set of the exchanged views."""
    sols = np.asarray(sols).reshape(-1, 9)
    return np.array([mc.normalise(e.reshape(3, 3).T.reshape(9)) for e in sols]).reshape(-1, 9)


def nearest(e, sols):
    """The distance of e from the nearest of a solution set; inf for an empty one."""
    sols = np.asarray(sols).reshape(-1, 9)
    return float(np.min(np.linalg.norm(sols - e[None, :], axis=1))) if len(sols) else np.inf


# ---- cells -------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Pair:
    case: object              # mc.Case or ec.Case: bearings, scene, the checker's answer, tol
    bad: tuple                # the violated conditions (minimal solvers) or ("well_posed",)
    kept: bool                # compared with the checker
    pose: bool                # compared for qualities, choice and pose too
    swapped: np.ndarray       # the checker's solutions (E of the eight-point) of the exchanged views (f2, f1)
    truth: np.ndarray = None  # the scene's e (noise-free cells)
    residual: tuple = None    # (|A e|, |A e'|) of the scene's E and of its transpose
    xyz_max: float = 0.0      # NISTER: the largest |xyz| of a real solution


IGNORED = ("count", "xyz")


def _minimal_pair(cell, f1, f2, R, t):
    info = {}
    x = mc.minimal_np(f1, f2, cell.algorithm, info=info)
    case = mc.Case(cell.algorithm, cell.n, cell.noise, f1, f2, R, t, 1, expected=x)
    bad = tuple(b for b in mc.conditions(case, info) if b not in IGNORED)
    kept = all(b == "margin" for b in bad)
    e, r, r_t = true_e(f1, f2, R, t)
    xyz = info.get("xyz", np.zeros((0, 3)))
    return Pair(case=case, bad=bad, kept=kept, pose=kept and not bad, truth=e, residual=(r, r_t),
                swapped=mc.minimal_np(f2, f1, cell.algorithm)["E_all"],
                xyz_max=float(np.max(np.linalg.norm(xyz, axis=1))) if len(xyz) else 0.0)


def _eight_pair(cell, f1, f2, R, t):
    case = ec.Case(cell.n, cell.noise, f1, f2, R, t, 1)
    kept = bool(ec.well_posed(case.expected))
    return Pair(case=case, bad=() if kept else ("well_posed",), kept=kept, pose=kept,
                swapped=ec.eight_point_np(f2, f1)["E"])


@functools.lru_cache(maxsize=None)
def pairs(name):
    """The 48 pairs of a cell with the checker's answers, once per process."""
    cell = BY_NAME[name]
    rng = np.random.default_rng(cell.seed)
    make = _eight_pair if cell.algorithm == EIGHTPT else _minimal_pair
    return tuple(make(cell, *scene(rng, cell.kind, cell.n, cell.noise)) for _ in range(CELL_PAIRS))


def counts(name):
    ps = pairs(name)
    return sum(p.kept for p in ps), sum(p.pose for p in ps)


def alone_rows(name):
    """Three kept pairs of a cell, with as many different solution counts among them as the cell has."""
    ps = pairs(name)
    kept = [i for i, p in enumerate(ps) if p.kept]
    rows, seen = [], set()
    for i in kept:
        s = ps[i].case.expected.get("n_solutions", 1)
        if s not in seen:
            seen.add(s)
            rows.append(i)
    rows += [i for i in kept if i not in rows]
    return sorted(rows[:ALONE])


def swapped_cases(name):
    """The cell's bearings with the two views exchanged (only what a batch is filled from)."""
    return [types.SimpleNamespace(n=p.case.n, f1=p.case.f2, f2=p.case.f1) for p in pairs(name)]


# ---- degenerate but valid inputs -----------------------------------------------------------------------------------------
def degenerate(algorithm):
    """Inputs of the documented domain (finite unit bearings, N at least the minimal count) on which the problem itself is
    degenerate: [(label, f1, f2)].  The checker is no reference here (it loses the scene's E on these)."""
    rng = np.random.default_rng([20267, algorithm])
    m = mc.MIN_N[algorithm]
    out = []

    def points(n, planar=False):
        x, y, z = rng.uniform(-2.0, 2.0, n), rng.uniform(-2.0, 2.0, n), rng.uniform(4.0, 8.0, n)
        return np.column_stack([x, y, 6.0 + 0.1 * x if planar else z])

    def pose():
        axis = rng.normal(size=3)
        t = rng.normal(size=3)
        return ec.rotation_from_vector(axis / np.linalg.norm(axis) * rng.uniform(0.02, 0.1)), t / np.linalg.norm(t)

    for n in (m, 64):
        R, t = pose()
        f1, f2, _, _ = bearings(points(n), np.eye(3), t)
        out.append((f"pure translation, N = {n}", f1, f2))
        f1, f2, _, _ = bearings(points(n), R, np.zeros(3))
        out.append((f"pure rotation, N = {n}", f1, f2))
    for n in (8, 64):
        R, t = pose()
        f1, f2, _, _ = bearings(points(n, planar=True), R, t)
        out.append((f"planar, N = {n}", f1, f2))
    R, t = pose()
    f1, f2, _, _ = bearings(points(m), R, t)
    out.append((f"{m} correspondences twice", np.concatenate([f1, f1]), np.concatenate([f2, f2])))
    f1, f2, _, _ = bearings(points(1), R, t)
    out.append(("every correspondence identical, N = 8", np.repeat(f1, 8, axis=0), np.repeat(f2, 8, axis=0)))
    f1, _, _, _ = bearings(points(8), R, t)
    out.append(("f2 == f1, N = 8", f1, f1.copy()))
    return [(label, np.ascontiguousarray(a), np.ascontiguousarray(b)) for label, a, b in out]


def degenerate_batch(algorithm):
    """The degenerate inputs with three kept pairs of the algorithm's first cell among them -> (entries with .n .f1 .f2
    .label, rows of the kept pairs, their cases)."""
    first = next(c for c in MINIMAL_CELLS if c.algorithm == algorithm).name
    ps = pairs(first)
    keep = [ps[i].case for i in alone_rows(first)]
    entries = [types.SimpleNamespace(label=label, n=len(f1), f1=f1, f2=f2) for label, f1, f2 in degenerate(algorithm)]
    at = (0, len(entries) // 2 + 1, len(entries) + 2)          # first, in the middle, last
    rows = []
    for k, c in zip(at, keep):
        entries.insert(k, types.SimpleNamespace(label="kept", n=c.n, f1=c.f1, f2=c.f2))
        rows.append(k)
    return entries, rows, keep
