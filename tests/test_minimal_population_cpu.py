"""What the checker alone decides about the populations of tests/minimal_solver_population.py, without a GPU: the scenes are
what their names say, every cell keeps the share it must and exactly the counts written down, the kept pairs of the
minimal-solver cells together cover few and many solutions and large |xyz|, and the checker itself has the three properties
the device is held to beyond the comparison with it -- it finds the scene's essential matrix (and, from eight
correspondences on, the scene's pose), its solution counts have the parity of the algorithm, and the exchanged views give
the transposed solution set.

Measured here (units of kappa 2^-52, worst kept pair of a cell): the scene's E lies within 9.7 of a checker solution
(32 allowed), the transposed set of the exchanged views within 14.2 of the set (64 allowed), the chosen pose within 8.7 of
the scene's (32 allowed), all three worst on NISTER N = 64 forward.
"""
import numpy as np
import pytest

import eight_point_cases as ec
import minimal_solver_cases as mc
import minimal_solver_population as pop

ALL_CELLS = pytest.mark.parametrize("cell", pop.CELLS, ids=lambda c: c.name)
MINIMAL = pytest.mark.parametrize("cell", pop.MINIMAL_CELLS, ids=lambda c: c.name)
EIGHT = pytest.mark.parametrize("cell", pop.EIGHT_CELLS, ids=lambda c: c.name)


# ---- 1. the scenes ----------------------------------------------------------------------------------------------------
def test_the_cells_are_those_of_the_plan():
    got = {(pop.NAMES[c.algorithm], c.n, c.kind, c.noise) for c in pop.CELLS}
    assert got == {("NISTER", 5, "generic", 0.0), ("NISTER", 5, "forward", 0.0), ("NISTER", 5, "sideways", 0.0),
                   ("NISTER", 5, "planar", 0.0), ("NISTER", 8, "generic", 0.0), ("NISTER", 64, "forward", 0.0),
                   ("SEVENPT", 7, "generic", 0.0), ("SEVENPT", 7, "forward", 0.0), ("SEVENPT", 7, "sideways", 0.0),
                   ("SEVENPT", 8, "generic", 0.0), ("SEVENPT", 64, "forward", 0.0),
                   ("EIGHTPT", 64, "generic", 1e-3), ("EIGHTPT", 64, "forward", 1e-3), ("EIGHTPT", 64, "sideways", 1e-3),
                   ("EIGHTPT", 8, "generic", 0.0)}
    assert len(pop.CELLS) == len(got) == len(pop.KEPT) and set(pop.KEPT) == {c.name for c in pop.CELLS}
    assert pop.CELL_PAIRS == 48 and pop.KEPT_MIN * 3 == pop.CELL_PAIRS and pop.KEPT_MIN_EIGHT_8 == 6
    assert mc.TOL_FACTOR == 32.0 and ec.TOL_FACTOR == 32.0


@pytest.mark.parametrize("kind", pop.KINDS)
def test_a_scene_is_what_its_kind_says(kind):
    n = 12
    f1, f2, R, t = pop.scene(np.random.default_rng([9, pop.KINDS.index(kind)]), kind, n, 0.0)
    assert f1.shape == f2.shape == (n, 3)
    assert np.allclose(np.linalg.norm(f1, axis=1), 1.0, rtol=0, atol=4 * mc.EPS)
    assert np.allclose(np.linalg.norm(f2, axis=1), 1.0, rtol=0, atol=4 * mc.EPS)
    assert abs(np.linalg.norm(t) - 1.0) <= 4 * mc.EPS and np.allclose(R @ R.T, np.eye(3), rtol=0, atol=8 * mc.EPS)
    angle = np.arccos(np.clip((np.trace(R) - 1.0) / 2.0, -1.0, 1.0))
    assert angle <= 0.1 + 1e-12
    # x1 = R x2 + t: the depths along the two bearings that meet
    for a, b in zip(f1, f2):
        d = np.linalg.lstsq(np.column_stack([a, -(R @ b)]), t, rcond=None)[0]
        x1 = d[0] * a
        assert np.linalg.norm(d[0] * a - d[1] * (R @ b) - t) <= 1e-12 and d[0] > 0 and d[1] > 0
        assert abs(x1[0]) <= 2 + 1e-9 and abs(x1[1]) <= 2 + 1e-9 and 4 - 1e-9 <= x1[2] <= 8 + 1e-9
        if kind == "planar":
            assert abs(x1[2] - (6.0 + 0.1 * x1[0])) <= 1e-9
    if kind == "forward":
        assert t[2] > 0.99 and 0 < np.hypot(t[0], t[1]) < 0.2
    if kind == "sideways":
        assert t[0] > 0.99 and 0 < np.hypot(t[1], t[2]) < 0.2
    if kind == "generic":
        g1, g2, R2, t2 = ec.draw_pair(np.random.default_rng([9, 0]), n, 0.0)
        assert np.array_equal(f1, g1) and np.array_equal(f2, g2) and np.array_equal(R, R2) and np.array_equal(t, t2)
    # noise: unit bearings that moved by about its size
    h1, h2, _, _ = pop.scene(np.random.default_rng([9, pop.KINDS.index(kind)]), kind, n, 1e-3)
    assert np.allclose(np.linalg.norm(h1, axis=1), 1.0, rtol=0, atol=4 * mc.EPS)
    assert 1e-4 < np.max(np.linalg.norm(h1 - f1, axis=1)) < 1e-2 and 1e-4 < np.max(np.linalg.norm(h2 - f2, axis=1)) < 1e-2


# ---- 2. the counts ----------------------------------------------------------------------------------------------------
@ALL_CELLS
def test_every_cell_keeps_its_share_and_exactly_the_counts_written_down(cell):
    ps = pop.pairs(cell.name)
    assert len(ps) == pop.CELL_PAIRS
    assert all(p.case.n == cell.n and p.case.f1.shape == (cell.n, 3) for p in ps)
    kept, pose = pop.counts(cell.name)
    reasons = {}
    for p in ps:
        for b in p.bad:
            reasons[b] = reasons.get(b, 0) + 1
    print(f"{cell.name}: kept {kept} of {len(ps)}, compared for choice and pose {pose}; violated: {reasons}")
    assert kept >= cell.kept_min, (cell.name, kept)
    assert (kept, pose) == pop.KEPT[cell.name], (cell.name, kept, pose)
    rows = pop.alone_rows(cell.name)
    assert len(rows) == pop.ALONE == len(set(rows)) and all(ps[i].kept for i in rows)
    for p in ps:
        if cell.algorithm == pop.EIGHTPT:
            assert p.kept == p.pose == bool(ec.well_posed(p.case.expected))
            continue
        # kept: the checker's conditions without `count` and `xyz`; `margin` gates the choice and the pose only
        info = {}
        x = mc.minimal_np(p.case.f1, p.case.f2, cell.algorithm, info=info)
        bad = [b for b in mc.conditions(p.case, info) if b not in ("count", "xyz")]
        assert p.kept == (not [b for b in bad if b != "margin"]) and p.pose == (not bad)
        if p.kept:
            assert x["status"] == mc.EM_OK and x["gap"] >= mc.GAP_MIN and p.case.kappa <= mc.KAPPA_MAX
            assert mc.min_separation(x["E_all"]) >= mc.SEPARATION_MIN and info["imag_ratio"] >= mc.IMAG_MIN
            assert p.case.tol == mc.TOL_FACTOR * p.case.kappa * mc.EPS


def test_the_kept_pairs_cover_few_and_many_solutions_and_large_xyz():
    counts = {pop.NISTER: set(), pop.SEVENPT: set()}
    xyz = []
    for cell in pop.MINIMAL_CELLS:
        for p in pop.pairs(cell.name):
            if p.kept:
                counts[cell.algorithm].add(p.case.expected["n_solutions"])
                if cell.algorithm == pop.NISTER:
                    xyz.append(p.xyz_max)
    big = sorted(v for v in xyz if v > 100.0)
    print(f"NISTER solution counts {sorted(counts[pop.NISTER])}, SEVENPT {sorted(counts[pop.SEVENPT])}; "
          f"{len(big)} kept NISTER pairs with max |xyz| > 100, the largest {big[-3:]}")
    assert {2, 4, 6} <= counts[pop.NISTER]
    assert counts[pop.SEVENPT] == {1, 3}
    assert big and big[-1] > mc.XYZ_MAX       # (beyond what minimal_solver_cases.cases admits)


# ---- 3. the checker's own truth recall, parity and swap ------------------------------------------------------------------
@MINIMAL
def test_the_checker_finds_the_scenes_essential_matrix_on_every_kept_pair(cell):
    worst = worst_pose = 0.0
    for p in pop.pairs(cell.name):
        c = p.case
        # the orientation of [t]x R: f1' E f2 vanishes to rounding, the transposed matrix leaves the rotation's size
        assert p.residual[0] <= 64 * mc.EPS * np.sqrt(c.n) and p.residual[1] >= 1e-6, p.residual
        assert abs(np.linalg.norm(p.truth) - 1.0) <= 4 * mc.EPS and mc.sign_largest(p.truth) == 1.0
        if not p.kept:
            continue
        x = c.expected
        d = pop.nearest(p.truth, x["E_all"])
        worst = max(worst, d / (c.kappa * mc.EPS))
        assert d <= c.tol, (cell.name, d, c.tol)
        if cell.n >= 8:
            dR, dt = ec.rotation_distance(x["R"], c.R), ec.translation_distance(x["t"], c.t)
            worst_pose = max(worst_pose, max(dR, dt) / (c.kappa * mc.EPS))
            assert dR <= c.tol and dt <= c.tol, (cell.name, dR, dt, c.tol)
    print(f"{cell.name}: the scene's E within {worst:.2f} kappa 2^-52 of a checker solution, the chosen pose within "
          f"{worst_pose:.2f} of the scene's (allowed {mc.TOL_FACTOR})")


@MINIMAL
def test_the_checkers_solution_counts_have_the_parity_of_the_algorithm(cell):
    want = 0 if cell.algorithm == pop.NISTER else 1
    counts = [p.case.expected["n_solutions"] for p in pop.pairs(cell.name) if p.kept]
    assert all(s % 2 == want and 1 <= s <= mc.MAX_SOLUTIONS for s in counts), counts


@MINIMAL
def test_the_checker_returns_the_transposed_set_for_the_exchanged_views(cell):
    worst = 0.0
    for p in pop.pairs(cell.name):
        if not p.kept:
            continue
        c = p.case
        assert len(p.swapped) == c.expected["n_solutions"]
        d = mc.match_sets(pop.transposed(p.swapped), c.expected["E_all"])
        worst = max(worst, d / (c.kappa * mc.EPS))
        assert d <= 2.0 * c.tol, (cell.name, d, c.tol)
    print(f"{cell.name}: exchanged views, transposed: within {worst:.2f} kappa 2^-52 (allowed {2 * mc.TOL_FACTOR})")


@EIGHT
def test_the_eight_point_checker_returns_the_transposed_e_for_the_exchanged_views(cell):
    worst = 0.0
    for p in pop.pairs(cell.name):
        if not p.kept:
            continue
        c = p.case
        d = float(np.linalg.norm(pop.transposed(p.swapped)[0] - c.expected["E"]))
        worst = max(worst, d * c.expected["gap"] / ec.EPS)
        assert d <= 2.0 * c.tol, (cell.name, d, c.tol)
    print(f"{cell.name}: exchanged views, transposed: within {worst:.3f} * 2^-52 / gap (allowed {2 * ec.TOL_FACTOR})")


# ---- 4. the degenerate inputs ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algorithm", [pop.NISTER, pop.SEVENPT], ids=["NISTER", "SEVENPT"])
def test_the_degenerate_inputs_are_inputs_of_the_documented_domain(algorithm):
    entries, rows, keep = pop.degenerate_batch(algorithm)
    labels = [e.label for e in entries]
    assert len(rows) == 3 and all(labels[r] == "kept" for r in rows) and labels.count("kept") == 3
    assert rows[0] == 0 and rows[2] == len(entries) - 1
    for r, c in zip(rows, keep):
        assert np.array_equal(entries[r].f1, c.f1) and np.array_equal(entries[r].f2, c.f2)
    for word in ("pure translation", "pure rotation", "planar, N = 8", "planar, N = 64", "twice", "identical", "f2 == f1"):
        assert any(word in s for s in labels), word
    for e in entries:
        assert e.n >= mc.MIN_N[algorithm] and e.f1.shape == e.f2.shape == (e.n, 3)
        assert np.isfinite(e.f1).all() and np.isfinite(e.f2).all()
        assert np.allclose(np.linalg.norm(e.f1, axis=1), 1.0, rtol=0, atol=4 * mc.EPS)
        assert np.allclose(np.linalg.norm(e.f2, axis=1), 1.0, rtol=0, atol=4 * mc.EPS)
        if "twice" in e.label:
            m = mc.MIN_N[algorithm]
            assert e.n == 2 * m and np.array_equal(e.f1[:m], e.f1[m:]) and np.array_equal(e.f2[:m], e.f2[m:])
        if "identical" in e.label:
            assert np.all(e.f1 == e.f1[0]) and np.all(e.f2 == e.f2[0])
        if "f2 == f1" in e.label:
            assert np.array_equal(e.f1, e.f2)
        if "pure rotation" in e.label:
            # one rotation takes every f2 to its f1
            U, _, Vt = np.linalg.svd(e.f1.T @ e.f2)
            assert np.allclose(e.f1, e.f2 @ (U @ Vt).T, rtol=0, atol=1e-12)
