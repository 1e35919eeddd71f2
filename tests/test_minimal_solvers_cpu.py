"""The minimal solvers without a GPU: pnec_hip_essential_minimal is declared, bound and exported within ABI 8, its
argument checks refuse before the handle is read or a device is touched, the Python, facade and harness names exist, and
the numpy checker of tests/minimal_solver_cases.py -- the yardstick of the GPU tests -- satisfies the conditions under
which the comparison is well posed, agrees with its second route, does not depend on the null-space basis and contains
the scene's essential matrix on noise-free pairs."""
import ctypes as C
import dataclasses
import inspect
import os
import re

import numpy as np
import pytest

import pnec_amd
from pnec_amd import capi

import eight_point_cases as ec
import minimal_solver_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALGORITHMS = pytest.mark.parametrize("algorithm", [mc.NISTER, mc.SEVENPT], ids=["NISTER", "SEVENPT"])


# ---- 1. the symbol ----------------------------------------------------------------------------------------------------
def test_symbol_is_declared_bound_and_exported_within_abi_8():
    assert "pnec_hip_essential_minimal" in capi.SYMBOLS
    L = capi.lib()
    assert getattr(L, "pnec_hip_essential_minimal") is not None
    assert capi.ABI_VERSION == 8 and L.pnec_hip_abi_version() == 8
    header = open(os.path.join(ROOT, "include", "pnec_hip.h")).read()
    assert "#define PNEC_HIP_ABI_VERSION 8" in header
    for name, value in (("NISTER", 1), ("SEVENPT", 2), ("MAX_SOLUTIONS", 10), ("QUALITY_ALL", 1)):
        assert f"#define PNEC_HIP_EM_{name} {value}" in header and getattr(capi, "EM_" + name) == value
    for name, value in (("OK", 0), ("TOO_FEW", 1), ("NOT_FINITE", 2), ("NO_CANDIDATE", 3), ("NO_SOLUTION", 4)):
        assert f"PNEC_HIP_EM_{name} = {value}" in header and getattr(capi, "EM_" + name) == value
        assert getattr(mc, "EM_" + name) == value
    decl = re.search(r"int pnec_hip_essential_minimal\(([^;]*)\);", header)
    assert decl, "the header declares the call"
    params = [p.strip() for p in decl.group(1).replace("\n", " ").split(",")]
    assert params[:3] == ["pnec_hip_problem *p", "int32_t algorithm", "int32_t flags"]
    assert params[-2:] == ["int space", "void *stream"]
    assert [p.split("*")[-1] for p in params[3:13]] == ["out_q", "out_t", "out_E", "out_singular", "out_gap", "out_n_solutions",
                                                        "out_E_all", "out_quality", "out_choice", "out_status"]
    # problem, algorithm, flags, ten outputs, space, stream
    assert len(params) == 15 and len(L.pnec_hip_essential_minimal.argtypes) == 15
    assert L.pnec_hip_essential_minimal.argtypes[1] is C.c_int32 and L.pnec_hip_essential_minimal.argtypes[13] is C.c_int


# ---- 2. refusals ------------------------------------------------------------------------------------------------------
def _call(p, algorithm, flags, outs, space=capi.MEM_HOST):
    L = capi.lib()
    rc = L.pnec_hip_essential_minimal(p, algorithm, flags, *outs, space, None)
    return rc, (L.pnec_hip_last_error() or b"").decode()


def test_bad_arguments_are_refused_before_the_handle_is_read():
    SENT = -7.25
    doubles = [np.full(n, SENT) for n in (4, 3, 9, 3, 1, 90, 40)]
    ints = [np.full(1, -5, dtype=np.int32) for _ in range(3)]
    q, t, E, sing, gap, E_all, qual = doubles
    nsol, choice, status = ints
    outs = tuple(a.ctypes.data for a in (q, t, E, sing, gap, nsol, E_all, qual, choice, status))
    # a stand-in handle: every check below must return before the handle is read
    fake = C.create_string_buffer(4096)
    h = C.cast(fake, C.c_void_p)
    for args, word in (((None, 1, 0, outs), "problem"),
                       ((h, 0, 0, outs), "algorithm"),
                       ((h, 3, 0, outs), "algorithm"),
                       ((h, -1, 0, outs), "algorithm"),
                       ((h, 1, 2, outs), "flags"),
                       ((h, 2, 3, outs), "flags"),
                       ((h, 2, -1, outs), "flags"),
                       ((h, 1, 0, (None,) * 10), "output"),
                       ((h, 2, 1, (None,) * 10), "output")):
        rc, msg = _call(*args)
        assert rc == capi.ERR_INVALID_ARGUMENT == -1, (rc, msg)
        assert word in msg, msg
    for space in (7, -1):
        rc, msg = _call(h, 1, 1, outs, space=space)
        assert rc == -1 and "memory space" in msg
    for a in doubles:
        assert np.all(a == SENT)
    for a in ints:
        assert np.all(a == -5)


# ---- 3. and 4. names --------------------------------------------------------------------------------------------------
def test_python_facade_and_harness_expose_the_new_names():
    assert "MinimalPose" in pnec_amd.__all__ and pnec_amd.MinimalPose is not None
    assert callable(pnec_amd.Batch.five_point) and callable(pnec_amd.Batch.seven_point)
    for f in (pnec_amd.Batch.five_point, pnec_amd.Batch.seven_point):
        p = inspect.signature(f).parameters
        assert p["quality"].default == "sample" and p["on_device"].default is None
    assert [f.name for f in dataclasses.fields(pnec_amd.MinimalPose)] == [
        "q", "t", "E", "singular", "gap", "n_solutions", "E_all", "quality", "choice", "status"]
    import pnec_amd.pypnec as pypnec
    assert "five_point" in dir(pypnec) and "seven_point" in dir(pypnec)
    facade = open(os.path.join(ROOT, "pnec_amd", "csrc", "host", "pnec_host.h")).read()
    assert re.search(r"SE3d MinimalEMPoseEstimation\(const bearingVectors_t &bvs1, const bearingVectors_t &bvs2, "
                     r"const SE3d &initial_pose,\s*algorithm_t algorithm\);", facade)
    with open(os.path.join(ROOT, "pnec_amd", "libpnec_host.so"), "rb") as f:
        assert b"MinimalEMPoseEstimation" in f.read()


def test_run_simulation_leaves_em_minimal_off_by_default():
    from pnec_amd import run_simulation as rs
    assert rs.EM_METHODS == ("8pt",)
    assert rs.EM_MINIMAL_METHODS == ("7pt", "Nister5pt")
    assert rs.parser().parse_args(["folder"]).em_minimal is False
    assert rs.parser().parse_args(["folder", "--em-minimal"]).em_minimal is True
    assert rs.parser().parse_args(["folder", "--em-minimal"]).em_methods is False
    assert inspect.signature(rs.run).parameters["em_minimal"].default is False


# ---- 5. the cases -----------------------------------------------------------------------------------------------------
@ALGORITHMS
def test_every_compared_case_satisfies_its_conditions(algorithm):
    cs = mc.cases(algorithm)
    assert tuple(c.n for c in cs) == mc.SIZES[algorithm]
    counts = set()
    for c in cs + mc.outlier_case(algorithm):
        info = {}
        x = mc.minimal_np(c.f1, c.f2, algorithm, c.quality_all, info=info)
        assert mc.conditions(c, info) == [], (c.n, mc.conditions(c, info))
        assert c.draws <= 2000 and c.noise == (0.0 if c.n <= mc.NOISE_FREE_MAX else mc.NOISE)
        assert x["status"] == mc.EM_OK and 0 <= x["choice"] < 4 * x["n_solutions"] <= 4 * mc.MAX_SOLUTIONS
        assert x["gap"] >= mc.GAP_MIN and c.kappa <= mc.KAPPA_MAX and mc.min_separation(x["E_all"]) >= mc.SEPARATION_MIN
        if algorithm == mc.NISTER:
            assert x["n_solutions"] >= 2 and np.all(np.linalg.norm(info["xyz"], axis=1) <= mc.XYZ_MAX)
        assert info["imag_ratio"] >= mc.IMAG_MIN
        if not c.tie:
            assert mc.quality_margin(x["quality"]) >= 4.0 * c.quality_tol
        counts.add(x["n_solutions"])
        print(f"{mc.NAMES[algorithm]} N = {c.n}: draw {c.draws}, {x['n_solutions']} solutions, gap {x['gap']:.3e}, "
              f"kappa {c.kappa:.1f}, tol {c.tol:.2e}, margin {mc.quality_margin(x['quality']):.3e}")
    if algorithm == mc.SEVENPT:
        assert counts == {1, 3}
    for c in mc.short_cases(algorithm):
        assert c.expected["status"] == mc.EM_TOO_FEW and c.expected["n_solutions"] == 0 and np.isnan(c.expected["E"]).all()


def test_the_outlier_case_separates_the_two_quality_rules():
    for algorithm in (mc.NISTER, mc.SEVENPT):
        sample, full = mc.outlier_case(algorithm)
        assert np.array_equal(sample.f2, full.f2) and not sample.quality_all and full.quality_all
        assert not mc.true_candidate(sample.expected, sample.R, sample.t)
        assert mc.true_candidate(full.expected, full.R, full.t)
        assert np.array_equal(sample.expected["E_all"], full.expected["E_all"])


# ---- 6. the two routes ------------------------------------------------------------------------------------------------
@ALGORITHMS
def test_eigh_of_the_normal_matrix_and_svd_of_a_agree_on_every_case(algorithm):
    worst = 0.0
    for c in mc.cases(algorithm) + mc.outlier_case(algorithm):
        x = c.expected
        y = mc.minimal_np(c.f1, c.f2, algorithm, c.quality_all, null_space=mc.null_space_svd)
        assert y["status"] == mc.EM_OK and y["n_solutions"] == x["n_solutions"]
        factor = mc.match_sets(x["E_all"], y["E_all"]) / (c.kappa * mc.EPS)
        print(f"{mc.NAMES[algorithm]} N = {c.n}: routes differ by {factor:.2f} kappa 2^-52 (kappa {c.kappa:.1f})")
        worst = max(worst, factor)
        assert factor <= mc.ROUTES_FACTOR, (c.n, factor)
        if not c.tie:
            assert y["choice"] == x["choice"]
    print(f"{mc.NAMES[algorithm]}: eigh(A'A) against svd(A): worst {worst:.2f} (allowed {mc.ROUTES_FACTOR})")


# ---- 7. basis independence --------------------------------------------------------------------------------------------
@ALGORITHMS
def test_the_solution_set_does_not_depend_on_the_null_space_basis(algorithm):
    rng = np.random.default_rng(77)
    k = mc.N_NULL[algorithm]
    for c in mc.cases(algorithm):
        basis, _ = mc.null_space_eigh(c.f1, c.f2, k)
        Q, _ = np.linalg.qr(rng.normal(size=(k, k)))
        rotated = mc.solutions_of(Q @ basis, algorithm)
        d = mc.match_sets(c.expected["E_all"], rotated)
        print(f"{mc.NAMES[algorithm]} N = {c.n}: rotated basis moves the set by {d / (c.kappa * mc.EPS):.2f} kappa 2^-52")
        assert d <= 4.0 * c.kappa * mc.EPS, (c.n, d)


# ---- 8. noise-free pairs ----------------------------------------------------------------------------------------------
@ALGORITHMS
def test_noise_free_pairs_contain_the_scenes_essential_matrix(algorithm):
    seen = 0
    for c in mc.cases(algorithm):
        if c.noise:
            continue
        seen += 1
        x = c.expected
        tx = np.array([[0.0, -c.t[2], c.t[1]], [c.t[2], 0.0, -c.t[0]], [-c.t[1], c.t[0], 0.0]])
        e = mc.normalise((tx @ c.R).reshape(9))
        d = float(np.min(np.linalg.norm(x["E_all"] - e[None, :], axis=1)))
        print(f"{mc.NAMES[algorithm]} N = {c.n}: the scene's E is {d:.2e} from a solution (tol {c.tol:.2e})")
        assert d <= c.tol
        if c.tie and not mc.true_candidate(x, c.R, c.t):
            # every solution fits the sample exactly: the chosen one only has to be as good as the scene's
            i = int(np.argmin(np.linalg.norm(x["E_all"] - e[None, :], axis=1)))
            assert np.min(x["quality"][i]) <= np.min(x["quality"]) + c.quality_tol
            continue
        assert mc.true_candidate(x, c.R, c.t)
        assert ec.rotation_distance(x["R"], c.R) <= c.tol and ec.translation_distance(x["t"], c.t) <= c.tol
    assert seen == len([n for n in mc.SIZES[algorithm] if n <= mc.NOISE_FREE_MAX])


# ---- 9. the facade ----------------------------------------------------------------------------------------------------
FACADE_PROGRAM = r"""
#include <cstdio>
#include <stdexcept>
#include "pnec_host.h"
using namespace pnec;
using namespace pnec::rel_pose_estimation;
int main() {
  const bearingVectors_t none;
  int thrown = 0;
  for (algorithm_t a : {EIGHTPT, STEWENIUS}) {
    try {
      MinimalEMPoseEstimation(none, none, SE3d(), a);
    } catch (const std::invalid_argument &) {
      ++thrown;
    }
  }
  // the two that are built, on a pair without correspondences: the start pose, no device touched
  int identity = 0;
  for (algorithm_t a : {NISTER, SEVENPT}) {
    const SE3d back = MinimalEMPoseEstimation(none, none, SE3d(), a);
    identity += back.rotationMatrix()(0, 0) == 1.0 && back.translation()[0] == 0.0;
  }
  // EMPoseEstimation keeps refusing them
  for (algorithm_t a : {NISTER, SEVENPT}) {
    try {
      EMPoseEstimation(none, none, SE3d(), a, false);
    } catch (const std::invalid_argument &) {
      ++thrown;
    }
  }
  std::printf("thrown %d identity %d\n", thrown, identity);
  return 0;
}
"""


def test_the_facade_throws_for_the_others_and_returns_the_start_pose_on_an_empty_pair(tmp_path):
    import shutil
    import subprocess
    gxx = shutil.which("g++")
    assert gxx, "g++ builds the host facade, so it is there"
    src, exe = tmp_path / "em_minimal_facade.cc", str(tmp_path / "em_minimal_facade")
    src.write_text(FACADE_PROGRAM)
    lib_dir = os.path.join(ROOT, "pnec_amd")
    subprocess.run([gxx, "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "pnec_amd", "csrc", "host"), str(src), "-o", exe, "-L" + lib_dir,
                    "-lpnec_host", "-lpnec_hip", "-Wl,-rpath," + lib_dir], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "thrown 4 identity 2" in r.stdout, r.stdout
