"""pnec_hip_essential_minimal on the device against the numpy checker of tests/minimal_solver_cases.py, both algorithms.

The compared pairs have every size at which the kernel takes another path (the minimal count and just above, both sides
of the sample, of the 16-lane row, of one, two and many strides of the wavefront) and satisfy the conditions under which
the comparison is well posed (test_minimal_solvers_cpu.py asserts them).  Tolerance: every solution within
32 * kappa * 2^-52 of the checker's, kappa the case's own condition number (the movement of the checker's solutions
under perturbations of one ulp of the bearings).  Two numpy routes to the same null space differ by up to 2.4 (NISTER)
and 0.9 (SEVENPT) in these units on these cases (the CPU test prints it); the device gets the rest for its own summation
order, its Jacobi sweeps and its route through the degree-10 polynomial.  Measured on an MI355X: worst factor 3.6
(NISTER, N = 5) and 0.9 (SEVENPT), DESIGN.md 9o.
"""
import os

import numpy as np
import pytest

from pnec_amd import Batch, capi

import eight_point_cases as ec
import minimal_solver_cases as mc

pytestmark = pytest.mark.gpu

NEC, TARGET, HOST, SYM = capi.MODE_NEC, capi.MODE_TARGET, capi.MODE_HOST, capi.MODE_SYM
FIELDS = ("q", "t", "E", "singular", "gap", "n_solutions", "E_all", "quality", "choice", "status")
DOUBLES = ("q", "t", "E", "singular", "gap", "E_all", "quality")
ALGORITHMS = pytest.mark.parametrize("algorithm", [mc.NISTER, mc.SEVENPT], ids=["NISTER", "SEVENPT"])
SOLVE = {mc.NISTER: "five_point", mc.SEVENPT: "seven_point"}


def _torch():
    import torch
    return torch


def _np(mp):
    return {k: (getattr(mp, k).cpu().numpy() if hasattr(getattr(mp, k), "cpu") else np.asarray(getattr(mp, k)))
            for k in FIELDS}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _same_rows(a, rows_a, b, rows_b):
    """The fields of result a at rows_a equal those of b at rows_b, bit for bit (a NaN equals itself)."""
    return [k for k in FIELDS if not np.array_equal(_bits(a[k][rows_a]), _bits(b[k][rows_b]))]


def _covs(n):
    return np.ascontiguousarray(np.tile(np.diag([1e-6, 2e-6, 3e-6]), (n, 1, 1)))


def _fill(b, mode, f1, f2):
    if len(f1):
        c = None if mode == NEC else _covs(len(f1))
        b.fill(f1, f2, c, c if mode == SYM else None)
    return b


def _batch(case_list, mode=NEC):
    off, f1, f2 = mc.batch_arrays(case_list)
    return _fill(Batch(mode, off), mode, f1, f2)


def _run(algorithm, case_list, quality="sample", mode=NEC, on_device=False):
    with _batch(case_list, mode) as b:
        out = _np(getattr(b, SOLVE[algorithm])(quality, on_device=on_device))
        if on_device:
            _torch().cuda.synchronize()
    return out


def _interleaved(algorithm):
    """All the sizes, the pair one short of the minimal count after the sixth and the empty pair at the end."""
    c, s = list(mc.cases(algorithm)), list(mc.short_cases(algorithm))
    order = c[:6] + [s[0]] + c[6:] + [s[1]]
    rows = [i for i, x in enumerate(order) if x.n >= mc.MIN_N[algorithm]]
    return order, rows


_main = {}


def main_result(algorithm):
    """The ragged batch of all sizes in DEVICE space, once per algorithm for the module."""
    if algorithm not in _main:
        order, rows = _interleaved(algorithm)
        off, f1, f2 = mc.batch_arrays(order)
        torch = _torch()
        with Batch(NEC, off) as b:
            b.fill(torch.as_tensor(f1, device="cuda:0"), torch.as_tensor(f2, device="cuda:0"))
            mp = getattr(b, SOLVE[algorithm])()
            assert mp.q.is_cuda and mp.status.dtype == torch.int32 and mp.n_solutions.dtype == torch.int32
            assert tuple(mp.E_all.shape) == (len(order), 10, 9) and tuple(mp.quality.shape) == (len(order), 10, 4)
            torch.cuda.synchronize()
            _main[algorithm] = dict(order=order, rows=rows, got=_np(mp))
    return _main[algorithm]


def _compare_set(case, got, row):
    """Status, count, the NaN pattern, the solution set and its order, norm and sign, the gap
    -> the distance of the solution sets in units of kappa 2^-52."""
    x = case.expected
    S = x["n_solutions"]
    assert int(got["status"][row]) == x["status"] == mc.EM_OK, (case.n, got["status"][row])
    assert int(got["n_solutions"][row]) == S, (case.n, got["n_solutions"][row], S)
    E_all, quality = got["E_all"][row], got["quality"][row]
    assert np.isnan(E_all[S:]).all() and np.isnan(quality[S:]).all() and np.isfinite(E_all[:S]).all()
    d_set = mc.match_sets(x["E_all"], E_all[:S])
    # the order: lexicographic on the device's own vectors, and the checker's solution at every place
    assert np.array_equal(mc.lexicographic(E_all[:S]), E_all[:S])
    d_place = float(np.max(np.linalg.norm(E_all[:S] - x["E_all"], axis=1)))
    factor = d_set / (case.kappa * mc.EPS)
    choice = int(got["choice"][row])
    print(f"{mc.NAMES[case.algorithm]} N = {case.n}: {S} solutions, set {d_set:.2e}, tol {case.tol:.2e}, factor {factor:.3f}, "
          f"choice {choice} (checker {x['choice']}), gap device {got['gap'][row]:.6e} checker {x['gap']:.6e}")
    assert d_set <= case.tol and d_place <= case.tol, (case.n, d_set, d_place, case.tol)
    for i in range(S):
        assert abs(np.linalg.norm(E_all[i]) - 1.0) <= 4 * mc.EPS and mc.sign_largest(E_all[i]) == 1.0
    # Weyl, as in the eight-point test
    assert abs(got["gap"][row] - x["gap"]) <= 162 * case.n * mc.EPS
    return factor


def _compare_pose(case, got, row):
    """Qualities, choice, singular values, q and t: what is determined where the checker's quality margin holds."""
    x = case.expected
    S = x["n_solutions"]
    E_all, quality = got["E_all"][row], got["quality"][row]
    choice = int(got["choice"][row])
    assert np.all(np.isfinite(quality[:S]) == np.isfinite(x["quality"]))
    assert np.allclose(quality[:S], x["quality"], rtol=0, atol=case.quality_tol)
    assert 0 <= choice < 4 * S
    if case.tie:
        # every solution fits the sample exactly: the chosen candidate only has to be as good as the best
        assert quality[choice // 4, choice % 4] <= np.min(x["quality"]) + case.quality_tol
        R = mc.decompose(E_all[choice // 4].reshape(3, 3))
        want_R, want_t = (R[1] if choice % 2 == 0 else R[2]), (R[3] if choice % 4 < 2 else -R[3])
    else:
        assert choice == x["choice"], (case.n, choice, x["choice"], quality, x["quality"])
        want_R, want_t = x["R"], x["t"]
        assert np.allclose(got["singular"][row][:2], x["singular"][:2], rtol=0, atol=case.tol + 4 * mc.EPS)
    assert np.array_equal(_bits(got["E"][row]), _bits(E_all[choice // 4]))
    dR = ec.rotation_distance(ec.rotation_from_quaternion(got["q"][row]), want_R)
    dt = ec.translation_distance(got["t"][row], want_t)
    print(f"    rotation {dR:.2e}, translation {dt:.2e}")
    assert dR <= case.tol and dt <= case.tol, (case.n, dR, dt, case.tol)
    assert abs(np.linalg.norm(got["q"][row]) - 1.0) <= 4 * mc.EPS and abs(np.linalg.norm(got["t"][row]) - 1.0) <= 4 * mc.EPS


def _compare(case, got, row):
    """-> the distance of the solution sets in units of kappa 2^-52."""
    factor = _compare_set(case, got, row)
    _compare_pose(case, got, row)
    return factor


# ---- 1. device against the checker ------------------------------------------------------------------------------------
@ALGORITHMS
def test_device_agrees_with_the_checker_on_every_size(algorithm):
    m = main_result(algorithm)
    worst = max(_compare(m["order"][r], m["got"], r) for r in m["rows"])
    print(f"{mc.NAMES[algorithm]}: worst factor over the sizes {mc.SIZES[algorithm]}: {worst:.3f} * kappa 2^-52 "
          f"(allowed {mc.TOL_FACTOR})")


# ---- 2. short and empty pairs -----------------------------------------------------------------------------------------
@ALGORITHMS
def test_short_and_empty_pairs_are_too_few_and_leave_their_neighbours_alone(algorithm):
    m = main_result(algorithm)
    got = m["got"]
    short = [i for i, c in enumerate(m["order"]) if c.n < mc.MIN_N[algorithm]]
    assert [m["order"][i].n for i in short] == list(mc.SHORT_SIZES[algorithm])
    for i in short:
        assert int(got["status"][i]) == capi.EM_TOO_FEW and int(got["choice"][i]) == -1 and int(got["n_solutions"][i]) == 0
        for k in DOUBLES:
            assert np.isnan(got[k][i]).all(), k
    alone = _run(algorithm, list(mc.cases(algorithm)), on_device=True)
    assert _same_rows(got, m["rows"], alone, list(range(len(mc.SIZES[algorithm])))) == []


# ---- 3. non-finite input ----------------------------------------------------------------------------------------------
@ALGORITHMS
@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_a_non_finite_bearing_marks_its_own_pair_only(algorithm, bad):
    m = main_result(algorithm)
    off, f1, f2 = mc.batch_arrays(m["order"])
    victim = next(r for r in m["rows"] if m["order"][r].n == 65)      # the value sits in the second stride
    f2 = f2.copy()
    f2[off[victim] + 64, 1] = bad
    with _fill(Batch(NEC, off), NEC, f1, f2) as b:
        got = _np(getattr(b, SOLVE[algorithm])(on_device=False))
    x = mc.minimal_np(f1[off[victim]:off[victim + 1]], f2[off[victim]:off[victim + 1]], algorithm)
    assert int(got["status"][victim]) == capi.EM_NOT_FINITE == x["status"]
    assert int(got["choice"][victim]) == -1 and int(got["n_solutions"][victim]) == 0
    for k in DOUBLES:
        assert np.isnan(got[k][victim]).all(), k
    others = [r for r in range(len(m["order"])) if r != victim]
    assert _same_rows(got, others, m["got"], others) == []


# ---- 4. PNEC_HIP_EM_QUALITY_ALL ---------------------------------------------------------------------------------------
@ALGORITHMS
def test_quality_all_picks_the_true_candidate_where_the_sample_does_not(algorithm):
    sample, full = mc.outlier_case(algorithm)
    got_s, got_a = _run(algorithm, [sample], "sample"), _run(algorithm, [full], "all")
    _compare(sample, got_s, 0)
    _compare(full, got_a, 0)
    R_s, R_a = ec.rotation_from_quaternion(got_s["q"][0]), ec.rotation_from_quaternion(got_a["q"][0])
    assert not mc.true_candidate(dict(choice=int(got_s["choice"][0]), R=R_s, t=got_s["t"][0]), sample.R, sample.t)
    assert mc.true_candidate(dict(choice=int(got_a["choice"][0]), R=R_a, t=got_a["t"][0]), full.R, full.t)
    assert np.array_equal(_bits(got_s["E_all"]), _bits(got_a["E_all"]))


# ---- 5. bitwise equalities --------------------------------------------------------------------------------------------
@ALGORITHMS
def test_each_pair_alone_equals_its_row_in_the_batch(algorithm):
    m = main_result(algorithm)
    for r, c in enumerate(m["order"]):
        assert _same_rows(_run(algorithm, [c]), [0], m["got"], [r]) == [], c.n


@ALGORITHMS
def test_host_space_equals_device_space(algorithm):
    m = main_result(algorithm)
    host = _run(algorithm, m["order"], on_device=False)
    every = list(range(len(m["order"])))
    assert _same_rows(host, every, m["got"], every) == []
    a, b = _run(algorithm, m["order"], "all", on_device=False), _run(algorithm, m["order"], "all", on_device=True)
    assert _same_rows(a, every, b, every) == []


@ALGORITHMS
@pytest.mark.parametrize("mode", [TARGET, HOST, SYM], ids=["TARGET", "HOST", "SYM"])
def test_the_four_problem_modes_agree(algorithm, mode):
    m = main_result(algorithm)
    every = list(range(len(m["order"])))
    assert _same_rows(_run(algorithm, m["order"], mode=mode), every, m["got"], every) == []


@ALGORITHMS
def test_a_reshaped_capacity_batch_equals_the_plain_batch(algorithm):
    m = main_result(algorithm)
    off, f1, f2 = mc.batch_arrays(m["order"])
    every = list(range(len(m["order"])))
    with Batch.with_capacity(TARGET, len(off) + 3, int(off[-1]) + 100) as b:
        # a first shape, so that the second one finds the planes used
        b.reshape(np.array([0, 50, 50 + int(off[-1])], dtype=np.int64))
        _fill(b, TARGET, np.ones((50 + int(off[-1]), 3)), np.ones((50 + int(off[-1]), 3)))
        b.reshape(off)
        _fill(b, TARGET, f1, f2)
        got = _np(getattr(b, SOLVE[algorithm])(on_device=False))
    assert _same_rows(got, every, m["got"], every) == []


@ALGORITHMS
def test_select_then_solve_equals_the_solve_on_the_masked_arrays(algorithm):
    m = main_result(algorithm)
    off, f1, f2 = mc.batch_arrays(m["order"])
    rng = np.random.default_rng(5)
    mask = (rng.random(int(off[-1])) < 0.85).astype(np.uint8)
    torch = _torch()
    with _batch(m["order"], TARGET) as b:
        for view in (False, True):
            sel = b.select(torch.as_tensor(mask, device="cuda:0"), view=view)
            got = _np(getattr(sel, SOLVE[algorithm])())    # (nothing is read back before the call)
            torch.cuda.synchronize()
            counts = [int(mask[off[p]:off[p + 1]].sum()) for p in range(len(off) - 1)]
            assert list(np.diff(sel.offsets)) == counts
            sel.close()
            keep = mask.astype(bool)
            off2 = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
            with _fill(Batch(NEC, off2), NEC, np.ascontiguousarray(f1[keep]), np.ascontiguousarray(f2[keep])) as direct:
                want = _np(getattr(direct, SOLVE[algorithm])(on_device=False))
            every = list(range(len(counts)))
            assert _same_rows(got, every, want, every) == [], view
            assert (want["status"] == capi.EM_OK).sum() >= 8 and (want["status"] == capi.EM_TOO_FEW).sum() >= 2


# ---- 6. stream order --------------------------------------------------------------------------------------------------
def _raw(b, algorithm):
    """pnec_hip_essential_minimal with DEVICE pointers on the current stream."""
    torch = _torch()
    P = b.n_pairs
    f = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda:0")
    i = lambda n: torch.zeros((n,), dtype=torch.int32, device="cuda:0")
    outs = [f(P, 4), f(P, 3), f(P, 9), f(P, 3), f(P), i(P), f(P, 10, 9), f(P, 10, 4), i(P), i(P)]
    capi.check(capi.lib().pnec_hip_essential_minimal(b._h, algorithm, 0, *[o.data_ptr() for o in outs], capi.MEM_DEVICE,
                                                     torch.cuda.current_stream(0).cuda_stream))
    return outs


@ALGORITHMS
def test_device_space_call_respects_stream_order_and_returns_while_a_delay_still_runs(algorithm):
    from test_stream_order_gpu import Entry, check
    torch = _torch()
    order, _ = _interleaved(algorithm)
    off, f1, f2 = mc.batch_arrays(order)
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda:0")
    # the decoy: the same shapes with the two frames exchanged (valid bearings, other solutions)
    good, decoy = dict(f1=dev(f1), f2=dev(f2)), dict(f1=dev(f2), f2=dev(f1))
    b = Batch(NEC, off)

    def call(bufs):
        b.fill(bufs["f1"], bufs["f2"])
        return _raw(b, algorithm), b

    check(Entry(good, decoy, call), "essential_minimal " + mc.NAMES[algorithm])
    b.close()


# ---- 7. allocation ----------------------------------------------------------------------------------------------------
@ALGORITHMS
def test_the_device_space_call_allocates_nothing_in_the_library_on_a_second_call(algorithm):
    from pnec_amd.multi import alloc_counters
    torch = _torch()
    order, _ = _interleaved(algorithm)
    with _batch(order) as b:
        first = _raw(b, algorithm)
        torch.cuda.synchronize()
        a0 = alloc_counters()
        second = _raw(b, algorithm)
        torch.cuda.synchronize()
        assert alloc_counters()["hip_malloc_calls"] == a0["hip_malloc_calls"]
        assert all(torch.equal(x.view(torch.int64) if x.dtype == torch.float64 else x,
                               y.view(torch.int64) if y.dtype == torch.float64 else y) for x, y in zip(first, second))


# ---- 8. facade and pypnec ---------------------------------------------------------------------------------------------
@ALGORITHMS
def test_the_facade_and_pypnec_equal_the_batch_call_on_one_pair(algorithm):
    import pnec_amd.pypnec as pypnec
    solve = getattr(pypnec, SOLVE[algorithm])
    c = next(x for x in mc.cases(algorithm) if x.n == 64)
    got = _run(algorithm, [c])
    T = np.asarray(solve(c.f1, c.f2))
    assert T.shape == (4, 4) and np.array_equal(T[3], [0.0, 0.0, 0.0, 1.0])
    assert np.array_equal(_bits(T[:3, :3]), _bits(ec.rotation_from_quaternion(got["q"][0])))
    s0 = np.linalg.norm(T[:3, 3])
    assert abs(s0 - got["singular"][0][0]) <= 4 * mc.EPS
    assert np.linalg.norm(T[:3, 3] / s0 - got["t"][0]) <= 4 * mc.EPS
    # one short of the minimal count: the start pose, which this binding fixes to the identity
    k = mc.MIN_N[algorithm] - 1
    assert np.array_equal(np.asarray(solve(c.f1[:k], c.f2[:k])), np.eye(4))


# ---- 9. harness -------------------------------------------------------------------------------------------------------
def test_run_simulation_adds_the_two_columns_and_leaves_the_seven_alone(tmp_path):
    import torch
    from pnec_amd import io_formats as io
    from pnec_amd import run_simulation as rs
    from pnec_amd import simulation as sim
    from pnec_amd.frontend import CAMERA_PINHOLE, unscented_transform
    E, N = 4, 40
    rng = np.random.default_rng(31)
    pairs = [ec.draw_pair(rng, N, ec.NOISE) for _ in range(E)]
    p1 = np.stack([f1 * rng.uniform(2.0, 5.0, size=(N, 1)) for f1, _, _, _ in pairs])   # 3-D points in frame 1
    p2 = np.stack([f2 / f2[:, 2:3] for _, f2, _, _ in pairs])                            # pinhole points in frame 2
    c2 = np.zeros((E, N, 3, 3))
    s = rng.uniform(0.5, 1.5, size=(E, N)) * (1.0 / 800.0) ** 2
    c2[..., 0, 0], c2[..., 1, 1] = s, 0.6 * s
    q_gt = sim.matrix_to_quaternion_xyzw(torch.as_tensor(np.stack([R for _, _, R, _ in pairs]))).numpy()
    poses_1 = np.tile(np.array([0, 0, 0, 1, 0, 0, 0], dtype=np.float64), (E, 1))
    poses_2 = np.concatenate([q_gt, np.stack([t for _, _, _, t in pairs])], 1)
    folder = str(tmp_path / "exp")
    io.write_experiments(folder, poses_1, poses_2, p1, p2, np.zeros_like(c2), c2)

    seven = rs.run(folder, seed=3, em_methods=True)
    nine = rs.run(folder, seed=3, em_methods=True, em_minimal=True)
    assert tuple(seven) == rs.METHODS + rs.EM_METHODS
    assert tuple(nine) == rs.METHODS + rs.EM_METHODS + rs.EM_MINIMAL_METHODS == rs.METHODS + ("8pt", "7pt", "Nister5pt")
    assert tuple(rs.run(folder, seed=3, em_minimal=True)) == rs.METHODS + rs.EM_MINIMAL_METHODS
    for m in seven:
        for key in ("r_error", "t_error", "cost"):
            assert np.array_equal(_bits(np.asarray(seven[m][key], dtype=np.float64)),
                                  _bits(np.asarray(nine[m][key], dtype=np.float64))), (m, key)
    io.write_result_tables(folder, nine)
    assert open(os.path.join(folder, "r_error.csv")).readline().strip() == "index," + ",".join(rs.METHODS + ("8pt", "7pt", "Nister5pt"))
    assert rs.main([folder, "--seed", "3", "--em-methods"]) == 0
    assert open(os.path.join(folder, "r_error.csv")).readline().strip() == "index," + ",".join(rs.METHODS + ("8pt",))

    # the two columns from the checker's poses, on the bearings the harness forms from what the folder holds
    ex = io.read_experiments(folder)
    R_gt, t_gt = io.relative_poses(ex["poses_1"], ex["poses_2"])
    pts1, pts2 = np.concatenate(ex["points_1"]), np.concatenate(ex["points_2"])
    b1 = pts1 / np.linalg.norm(pts1, axis=1, keepdims=True)
    b2, _ = unscented_transform(pts2, np.concatenate(ex["covs_2"]), None, 1.0, CAMERA_PINHOLE)
    b2 = np.asarray(b2)
    for name, algorithm in (("7pt", mc.SEVENPT), ("Nister5pt", mc.NISTER)):
        for e in range(E):
            g1, g2 = b1[e * N:(e + 1) * N], b2[e * N:(e + 1) * N]
            info = {}
            x = mc.minimal_np(g1, g2, algorithm, info=info)
            c = mc.Case(algorithm, N, ec.NOISE, g1, g2, R_gt[e], t_gt[e], 1, expected=x)
            assert mc.conditions(c, info) == [], (name, e, mc.conditions(c, info))
            tol = c.tol
            want_r = rs.rotational_difference_deg(R_gt[e:e + 1], x["R"][None])[0]
            want_t = rs.translational_difference_deg(t_gt[e:e + 1], x["t"][None])[0]
            # d arccos(c) = dc / sin(angle), |dc| <= 1.23 tol (rotation: |R_gt|_F |dR|_F / 2) or tol (translation)
            bound_r = np.degrees(2.0 * tol / np.sin(np.radians(want_r)))
            bound_t = np.degrees(2.0 * tol / np.sin(np.radians(want_t)))
            got_r, got_t = nine[name]["r_error"][e], nine[name]["t_error"][e]
            print(f"{name} experiment {e}: r_error {got_r:.6e} (checker {want_r:.6e}, bound {bound_r:.1e}), "
                  f"t_error {got_t:.6e} (checker {want_t:.6e}, bound {bound_t:.1e})")
            assert want_r > 1e-3 and want_t > 1e-3      # (degrees: far from where the arccos loses its digits)
            assert abs(got_r - want_r) <= bound_r and abs(got_t - want_t) <= bound_t
            assert np.isfinite(nine[name]["cost"][e])
