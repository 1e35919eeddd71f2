"""pnec_hip_eight_point on the device against the numpy checker of tests/eight_point_cases.py.

The compared pairs have every size at which the kernel takes another path (both sides of the sample of nine, of the
16-lane row, of one, two and many strides of the wavefront) and satisfy the two conditions under which the comparison is
well posed (test_eight_point_cpu.py asserts them).  Tolerance: q and t within 32 * 2^-52 / gap of the checker, gap from
the checker's eigenvalues -- at most 7e-9 at the gap bound.  Two numpy routes to the same null vector differ by up to
0.1 * 2^-52 / gap on these cases (test_eight_point_cpu.py prints it); the device gets the rest for its own summation
order over up to 2049 terms and its Jacobi sweeps.  Measured on an MI355X: see DESIGN.md 9l.
"""
import os

import numpy as np
import pytest

from pnec_amd import Batch, capi

import eight_point_cases as ec

pytestmark = pytest.mark.gpu

NEC, TARGET, HOST, SYM = capi.MODE_NEC, capi.MODE_TARGET, capi.MODE_HOST, capi.MODE_SYM
FIELDS = ("q", "t", "E", "singular", "gap", "quality", "choice", "status")


def _torch():
    import torch
    return torch


def _np(ep):
    """An EightPoint as numpy arrays, whichever space it came from."""
    return {k: (getattr(ep, k).cpu().numpy() if hasattr(getattr(ep, k), "cpu") else np.asarray(getattr(ep, k)))
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
    off, f1, f2 = ec.batch_arrays(case_list)
    return _fill(Batch(mode, off), mode, f1, f2)


def _run(case_list, quality="sample", mode=NEC, on_device=False):
    with _batch(case_list, mode) as b:
        out = _np(b.eight_point(quality, on_device=on_device))
        if on_device:
            _torch().cuda.synchronize()
    return out


def _interleaved():
    """All the sizes, the pair of 7 after the sixth and the empty pair at the end -> (cases, rows of the compared ones)."""
    c, s = list(ec.cases()), list(ec.short_cases())
    order = c[:6] + [s[0]] + c[6:] + [s[1]]
    rows = [i for i, x in enumerate(order) if x.n >= 8]
    return order, rows


_main = {}


def main_result():
    """The ragged batch of all sizes in DEVICE space, once for the module."""
    if not _main:
        order, rows = _interleaved()
        off, f1, f2 = ec.batch_arrays(order)
        torch = _torch()
        with Batch(NEC, off) as b:
            b.fill(torch.as_tensor(f1, device="cuda:0"), torch.as_tensor(f2, device="cuda:0"))
            ep = b.eight_point()
            assert ep.q.is_cuda and ep.status.dtype == torch.int32
            torch.cuda.synchronize()
            _main.update(order=order, rows=rows, got=_np(ep))
    return _main


def _compare(case, got, row):
    """-> the largest of the E, rotation and translation differences in units of 2^-52 / gap."""
    x = case.expected
    assert int(got["status"][row]) == x["status"] == ec.EP_OK, (case.n, got["status"][row])
    assert int(got["choice"][row]) == x["choice"], (case.n, got["choice"][row], x["choice"], got["quality"][row], x["quality"])
    dE = float(np.linalg.norm(got["E"][row] - x["E"]))
    dR = ec.rotation_distance(ec.rotation_from_quaternion(got["q"][row]), x["R"])
    dt = ec.translation_distance(got["t"][row], x["t"])
    factor = max(dE, dR, dt) * x["gap"] / ec.EPS
    print(f"N = {case.n}: E {dE:.2e}, rotation {dR:.2e}, translation {dt:.2e}, tol {case.tol:.2e}, "
          f"factor {factor:.3f}, gap device {got['gap'][row]:.6e} checker {x['gap']:.6e}")
    assert dE <= case.tol and dR <= case.tol and dt <= case.tol, (case.n, dE, dR, dt, case.tol)
    assert abs(np.linalg.norm(got["q"][row]) - 1.0) <= 4 * ec.EPS and abs(np.linalg.norm(got["t"][row]) - 1.0) <= 4 * ec.EPS
    assert abs(np.linalg.norm(got["E"][row]) - 1.0) <= 4 * ec.EPS and ec.sign_largest(got["E"][row]) == 1.0
    # Weyl: an eigenvalue moves by at most |dG|_F <= 9 max |dG_kl|; a sum of N products accumulated in any order is off
    # by at most N eps sum |a_k a_l| <= N eps trace / 2, for the device's matrix and for numpy's; lambda_8 >= trace / 9
    assert abs(got["gap"][row] - x["gap"]) <= 162 * case.n * ec.EPS
    # (the singular values of two E that differ by dE differ by at most |dE|)
    assert np.allclose(got["singular"][row][:2], x["singular"][:2], rtol=0, atol=case.tol + 4 * ec.EPS)
    assert np.all(np.isfinite(got["quality"][row]) == np.isfinite(x["quality"]))
    return factor


# ---- 1. device against the checker ------------------------------------------------------------------------------------
def test_device_agrees_with_the_checker_on_every_size():
    m = main_result()
    worst = max(_compare(m["order"][r], m["got"], r) for r in m["rows"])
    print(f"worst factor over the sizes {ec.SIZES}: {worst:.3f} * 2^-52 / gap (allowed {ec.TOL_FACTOR})")


# ---- 2. short and empty pairs -----------------------------------------------------------------------------------------
def test_short_and_empty_pairs_are_too_few_and_leave_their_neighbours_alone():
    m = main_result()
    got = m["got"]
    short = [i for i, c in enumerate(m["order"]) if c.n < 8]
    assert [m["order"][i].n for i in short] == [7, 0]
    for i in short:
        assert int(got["status"][i]) == capi.EP_TOO_FEW and int(got["choice"][i]) == -1
        for k in ("q", "t", "E", "singular", "gap", "quality"):
            assert np.isnan(got[k][i]).all(), k
    alone = _run(list(ec.cases()), on_device=True)
    assert _same_rows(got, m["rows"], alone, list(range(len(ec.SIZES)))) == []


# ---- 3. non-finite input ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_a_non_finite_bearing_marks_its_own_pair_only(bad):
    m = main_result()
    off, f1, f2 = ec.batch_arrays(m["order"])
    victim = m["rows"][8]                       # 65 correspondences: the value sits in the second stride
    f2 = f2.copy()
    f2[off[victim] + 64, 1] = bad
    with _fill(Batch(NEC, off), NEC, f1, f2) as b:
        got = _np(b.eight_point(on_device=False))
    x = ec.eight_point_np(f1[off[victim]:off[victim + 1]], f2[off[victim]:off[victim + 1]])
    assert int(got["status"][victim]) == capi.EP_NOT_FINITE == x["status"] and int(got["choice"][victim]) == -1
    for k in ("q", "t", "E"):
        assert np.isnan(got[k][victim]).all()
    others = [r for r in range(len(m["order"])) if r != victim]
    assert _same_rows(got, others, m["got"], others) == []


# ---- 4. PNEC_HIP_EP_QUALITY_ALL ---------------------------------------------------------------------------------------
def test_quality_all_picks_the_true_candidate_where_the_sample_of_nine_does_not():
    sample, full = ec.outlier_case()
    got_s, got_a = _run([sample], "sample"), _run([full], "all")
    _compare(sample, got_s, 0)
    _compare(full, got_a, 0)
    R_s, R_a = ec.rotation_from_quaternion(got_s["q"][0]), ec.rotation_from_quaternion(got_a["q"][0])
    assert not ec.true_candidate(dict(choice=int(got_s["choice"][0]), R=R_s, t=got_s["t"][0]), sample.R, sample.t)
    assert ec.true_candidate(dict(choice=int(got_a["choice"][0]), R=R_a, t=got_a["t"][0]), full.R, full.t)
    assert np.array_equal(_bits(got_s["E"]), _bits(got_a["E"]))
    # the flag on the clean sizes: the checker's quality_all again, every pair
    all_got = _run(list(ec.cases()), "all", on_device=True)
    for r, c in enumerate(ec.cases()):
        x = ec.eight_point_np(c.f1, c.f2, True)
        assert ec.quality_margin(x["quality"]) >= ec.MARGIN_MIN
        assert int(all_got["choice"][r]) == x["choice"] and int(all_got["status"][r]) == ec.EP_OK
        # a pose off by tol moves a triangulated direction by at most depth / baseline (8 here) times that, twice per term
        assert np.allclose(all_got["quality"][r], x["quality"], rtol=0, atol=32 * c.tol * c.n)


# ---- 5. bitwise equalities --------------------------------------------------------------------------------------------
def test_each_pair_alone_equals_its_row_in_the_batch():
    m = main_result()
    for r, c in enumerate(m["order"]):
        assert _same_rows(_run([c]), [0], m["got"], [r]) == [], c.n


def test_host_space_equals_device_space():
    m = main_result()
    host = _run(m["order"], on_device=False)
    every = list(range(len(m["order"])))
    assert _same_rows(host, every, m["got"], every) == []
    for quality in ("all",):
        a, b = _run(m["order"], quality, on_device=False), _run(m["order"], quality, on_device=True)
        assert _same_rows(a, every, b, every) == []


@pytest.mark.parametrize("mode", [TARGET, HOST, SYM], ids=["TARGET", "HOST", "SYM"])
def test_the_four_problem_modes_agree(mode):
    m = main_result()
    every = list(range(len(m["order"])))
    assert _same_rows(_run(m["order"], mode=mode), every, m["got"], every) == []


def test_a_reshaped_capacity_batch_equals_the_plain_batch():
    m = main_result()
    off, f1, f2 = ec.batch_arrays(m["order"])
    every = list(range(len(m["order"])))
    with Batch.with_capacity(TARGET, len(off) + 3, int(off[-1]) + 100) as b:
        # a first shape, so that the second one finds the planes used
        b.reshape(np.array([0, 50, 50 + int(off[-1])], dtype=np.int64))
        _fill(b, TARGET, np.ones((50 + int(off[-1]), 3)), np.ones((50 + int(off[-1]), 3)))
        b.reshape(off)
        _fill(b, TARGET, f1, f2)
        got = _np(b.eight_point(on_device=False))
    assert _same_rows(got, every, m["got"], every) == []


def test_select_then_eight_point_equals_eight_point_on_the_masked_arrays():
    m = main_result()
    off, f1, f2 = ec.batch_arrays(m["order"])
    rng = np.random.default_rng(5)
    mask = (rng.random(int(off[-1])) < 0.85).astype(np.uint8)
    torch = _torch()
    with _batch(m["order"], TARGET) as b:
        for view in (False, True):
            sel = b.select(torch.as_tensor(mask, device="cuda:0"), view=view)
            got = _np(sel.eight_point())       # (nothing is read back before the call: the sizes live on the device)
            torch.cuda.synchronize()
            counts = [int(mask[off[p]:off[p + 1]].sum()) for p in range(len(off) - 1)]
            assert list(np.diff(sel.offsets)) == counts
            sel.close()
            keep = mask.astype(bool)
            off2 = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
            with _fill(Batch(NEC, off2), NEC, np.ascontiguousarray(f1[keep]), np.ascontiguousarray(f2[keep])) as direct:
                want = _np(direct.eight_point(on_device=False))
            every = list(range(len(counts)))
            assert _same_rows(got, every, want, every) == [], view
            assert (want["status"] == capi.EP_OK).sum() >= 8 and (want["status"] == capi.EP_TOO_FEW).sum() >= 2


# ---- 6. stream order --------------------------------------------------------------------------------------------------
def _raw(b):
    """pnec_hip_eight_point with DEVICE pointers on the current stream."""
    torch = _torch()
    P = b.n_pairs
    f = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda:0")
    i = lambda n: torch.zeros((n,), dtype=torch.int32, device="cuda:0")
    outs = [f(P, 4), f(P, 3), f(P, 9), f(P, 3), f(P), f(P, 4), i(P), i(P)]
    capi.check(capi.lib().pnec_hip_eight_point(b._h, 0, *[o.data_ptr() for o in outs], capi.MEM_DEVICE,
                                               torch.cuda.current_stream(0).cuda_stream))
    return outs


def test_device_space_call_respects_stream_order_and_returns_while_a_delay_still_runs():
    from test_stream_order_gpu import Entry, check
    torch = _torch()
    order, _ = _interleaved()
    off, f1, f2 = ec.batch_arrays(order)
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda:0")
    # the decoy: the same shapes with the two frames exchanged (valid bearings, another E)
    good, decoy = dict(f1=dev(f1), f2=dev(f2)), dict(f1=dev(f2), f2=dev(f1))
    b = Batch(NEC, off)

    def call(bufs):
        b.fill(bufs["f1"], bufs["f2"])
        return _raw(b), b

    check(Entry(good, decoy, call), "eight_point")
    b.close()


# ---- 7. allocation ----------------------------------------------------------------------------------------------------
def test_the_device_space_call_allocates_nothing_in_the_library_on_a_second_call():
    from pnec_amd.multi import alloc_counters
    torch = _torch()
    order, _ = _interleaved()
    with _batch(order) as b:
        first = _raw(b)
        torch.cuda.synchronize()
        a0 = alloc_counters()
        second = _raw(b)
        torch.cuda.synchronize()
        assert alloc_counters()["hip_malloc_calls"] == a0["hip_malloc_calls"]
        assert all(torch.equal(x.view(torch.int64) if x.dtype == torch.float64 else x,
                               y.view(torch.int64) if y.dtype == torch.float64 else y) for x, y in zip(first, second))


# ---- 8. facade and pypnec ---------------------------------------------------------------------------------------------
def test_the_facade_and_pypnec_equal_the_batch_call_on_one_pair():
    import pnec_amd.pypnec as pypnec
    c = next(x for x in ec.cases() if x.n == 64)
    got = _run([c])
    T = np.asarray(pypnec.eight_point(c.f1, c.f2))
    assert T.shape == (4, 4) and np.array_equal(T[3], [0.0, 0.0, 0.0, 1.0])
    assert np.array_equal(_bits(T[:3, :3]), _bits(ec.rotation_from_quaternion(got["q"][0])))
    s0 = np.linalg.norm(T[:3, 3])
    assert abs(s0 - got["singular"][0][0]) <= 4 * ec.EPS
    assert np.linalg.norm(T[:3, 3] / s0 - got["t"][0]) <= 4 * ec.EPS
    # fewer than eight correspondences: the start pose, which this binding fixes to the identity
    assert np.array_equal(np.asarray(pypnec.eight_point(c.f1[:7], c.f2[:7])), np.eye(4))


# ---- 9. harness -------------------------------------------------------------------------------------------------------
def test_run_simulation_adds_the_8pt_column_and_leaves_the_six_alone(tmp_path):
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

    plain = rs.run(folder, seed=3)
    with_em = rs.run(folder, seed=3, em_methods=True)
    assert tuple(plain) == rs.METHODS and tuple(with_em) == rs.METHODS + rs.EM_METHODS
    for m in rs.METHODS:
        for key in ("r_error", "t_error", "cost"):
            assert np.array_equal(_bits(np.asarray(plain[m][key], dtype=np.float64)),
                                  _bits(np.asarray(with_em[m][key], dtype=np.float64))), (m, key)
    # the tables: the column after the six; without the flag, the six alone
    io.write_result_tables(folder, with_em)
    assert open(os.path.join(folder, "r_error.csv")).readline().strip() == "index," + ",".join(rs.METHODS + ("8pt",))
    assert rs.main([folder, "--seed", "3"]) == 0
    assert open(os.path.join(folder, "r_error.csv")).readline().strip() == "index," + ",".join(rs.METHODS)

    # the 8pt column from the checker's poses, on the bearings the harness forms from what the folder holds
    ex = io.read_experiments(folder)
    R_gt, t_gt = io.relative_poses(ex["poses_1"], ex["poses_2"])
    pts1, pts2 = np.concatenate(ex["points_1"]), np.concatenate(ex["points_2"])
    b1 = pts1 / np.linalg.norm(pts1, axis=1, keepdims=True)
    b2, _ = unscented_transform(pts2, np.concatenate(ex["covs_2"]), None, 1.0, CAMERA_PINHOLE)
    b2 = np.asarray(b2)
    for e in range(E):
        x = ec.eight_point_np(b1[e * N:(e + 1) * N], b2[e * N:(e + 1) * N])
        assert ec.well_posed(x), (e, x["gap"], x["quality"])
        tol = ec.TOL_FACTOR * ec.EPS / x["gap"]
        want_r = rs.rotational_difference_deg(R_gt[e:e + 1], x["R"][None])[0]
        want_t = rs.translational_difference_deg(t_gt[e:e + 1], x["t"][None])[0]
        # d arccos(c) = dc / sin(angle), |dc| <= 1.23 tol (rotation: |R_gt|_F |dR|_F / 2) or tol (translation)
        bound_r = np.degrees(2.0 * tol / np.sin(np.radians(want_r)))
        bound_t = np.degrees(2.0 * tol / np.sin(np.radians(want_t)))
        got_r, got_t = with_em["8pt"]["r_error"][e], with_em["8pt"]["t_error"][e]
        print(f"experiment {e}: r_error {got_r:.6e} (checker {want_r:.6e}, bound {bound_r:.1e}), "
              f"t_error {got_t:.6e} (checker {want_t:.6e}, bound {bound_t:.1e})")
        assert want_r > 1e-3 and want_t > 1e-3      # (degrees: far from where the arccos loses its digits)
        assert abs(got_r - want_r) <= bound_r and abs(got_t - want_t) <= bound_t
        assert np.isfinite(with_em["8pt"]["cost"][e])
