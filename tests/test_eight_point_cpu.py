"""The eight-point baseline without a GPU: pnec_hip_eight_point is declared, bound and exported within ABI 8, its
argument checks refuse before the handle is read or a device is touched, the Python, facade and harness names exist, and
the numpy checker of tests/eight_point_cases.py -- the yardstick of the GPU tests -- returns the true pose on noise-free
pairs and agrees with a second numpy route to the same null vector on every case."""
import ctypes as C
import dataclasses
import os
import re

import numpy as np
import pytest

import pnec_amd
from pnec_amd import capi

import eight_point_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_is_declared_bound_and_exported_within_abi_8():
    assert "pnec_hip_eight_point" in capi.SYMBOLS
    L = capi.lib()
    assert getattr(L, "pnec_hip_eight_point") is not None
    assert capi.ABI_VERSION == 8 and L.pnec_hip_abi_version() == 8
    header = open(os.path.join(ROOT, "include", "pnec_hip.h")).read()
    assert "#define PNEC_HIP_ABI_VERSION 8" in header
    assert "#define PNEC_HIP_EP_QUALITY_ALL 1" in header and capi.EP_QUALITY_ALL == 1
    for name, value in (("OK", 0), ("TOO_FEW", 1), ("NOT_FINITE", 2), ("NO_CANDIDATE", 3)):
        assert f"PNEC_HIP_EP_{name} = {value}" in header and getattr(capi, "EP_" + name) == value
    decl = re.search(r"int pnec_hip_eight_point\(([^;]*)\);", header)
    assert decl, "the header declares the call"
    params = [p.strip() for p in decl.group(1).replace("\n", " ").split(",")]
    assert params[0] == "pnec_hip_problem *p" and params[1] == "int32_t flags"
    assert params[-2:] == ["int space", "void *stream"]
    # problem, flags, eight outputs, space, stream
    assert len(params) == 12 and len(L.pnec_hip_eight_point.argtypes) == 12
    assert L.pnec_hip_eight_point.argtypes[1] is C.c_int32 and L.pnec_hip_eight_point.argtypes[10] is C.c_int


def _call(p, flags, outs, space=capi.MEM_HOST):
    L = capi.lib()
    rc = L.pnec_hip_eight_point(p, flags, *outs, space, None)
    return rc, (L.pnec_hip_last_error() or b"").decode()


def test_bad_arguments_are_refused_before_the_handle_is_read():
    SENT = -7.25
    q, t, E, sing, gap, qual = (np.full(n, SENT) for n in (4, 3, 9, 3, 1, 4))
    choice, status = (np.full(1, -5, dtype=np.int32) for _ in range(2))
    outs = tuple(a.ctypes.data for a in (q, t, E, sing, gap, qual, choice, status))
    # a stand-in handle: every check below must return before the handle is read (this box may have no device, and a
    # real problem cannot be created without one)
    fake = C.create_string_buffer(4096)
    h = C.cast(fake, C.c_void_p)
    for args, word in (((None, 0, outs), "problem"),
                       ((h, 2, outs), "flags"),
                       ((h, 3, outs), "flags"),
                       ((h, -1, outs), "flags"),
                       ((h, 0, (None,) * 8), "output"),
                       ((h, 1, (None,) * 8), "output")):
        rc, msg = _call(*args)
        assert rc == capi.ERR_INVALID_ARGUMENT == -1, (rc, msg)
        assert word in msg, msg
    for space in (7, -1):
        rc, msg = _call(h, 1, outs, space=space)
        assert rc == -1 and "memory space" in msg
    for a in (q, t, E, sing, gap, qual):
        assert np.all(a == SENT)
    assert np.all(choice == -5) and np.all(status == -5)


def test_python_facade_and_harness_expose_the_new_names():
    assert "EightPoint" in pnec_amd.__all__ and pnec_amd.EightPoint is not None
    assert callable(pnec_amd.Batch.eight_point)
    assert [f.name for f in dataclasses.fields(pnec_amd.EightPoint)] == [
        "q", "t", "E", "singular", "gap", "quality", "choice", "status"]
    import pnec_amd.pypnec as pypnec
    assert "eight_point" in dir(pypnec)
    facade = open(os.path.join(ROOT, "pnec_amd", "csrc", "host", "pnec_host.h")).read()
    assert "SE3d EMPoseEstimation(const bearingVectors_t &bvs1, const bearingVectors_t &bvs2, const SE3d &initial_pose," in facade
    assert "algorithm_t algorithm, bool ransac = true);" in facade
    for name in ("STEWENIUS", "NISTER", "SEVENPT", "EIGHTPT"):
        assert re.search(r"enum algorithm_t \{[^}]*\b" + name + r"\b", facade), name
    with open(os.path.join(ROOT, "pnec_amd", "libpnec_host.so"), "rb") as f:
        assert b"EMPoseEstimation" in f.read()


def test_run_simulation_leaves_the_em_methods_off_by_default():
    from pnec_amd import run_simulation as rs
    assert rs.METHODS == ("NEC", "NEC-LS", "NEC PNEC-LS", "PNEC only LS", "PNEC w/o LS", "PNEC")
    assert rs.EM_METHODS == ("8pt",)
    assert rs.parser().parse_args(["folder"]).em_methods is False
    assert rs.parser().parse_args(["folder", "--em-methods"]).em_methods is True
    import inspect
    assert inspect.signature(rs.run).parameters["em_methods"].default is False


FACADE_PROGRAM = r"""
#include <cstdio>
#include <stdexcept>
#include <string>
#include "pnec_host.h"
using namespace pnec;
using namespace pnec::rel_pose_estimation;
int main() {
  const bearingVectors_t none;
  int thrown = 0;
  const struct { algorithm_t a; bool ransac; const char *word; } combos[] = {
      {STEWENIUS, false, "STEWENIUS"}, {NISTER, false, "NISTER"}, {SEVENPT, false, "SEVENPT"},
      {STEWENIUS, true, "STEWENIUS"},  {NISTER, true, "NISTER"},  {SEVENPT, true, "SEVENPT"}, {EIGHTPT, true, "ransac"}};
  for (const auto &c : combos) {
    try {
      EMPoseEstimation(none, none, SE3d(), c.a, c.ransac);
    } catch (const std::invalid_argument &e) {
      if (std::string(e.what()).find(c.word) != std::string::npos && std::string(e.what()).find("not built") != std::string::npos)
        ++thrown;
      else
        std::printf("message without its word: %s\n", e.what());
    }
  }
  // the default of `ransac` is the reference's: true
  try {
    EMPoseEstimation(none, none, SE3d(), EIGHTPT);
  } catch (const std::invalid_argument &) {
    ++thrown;
  }
  // the one combination that is built, on a pair without correspondences: the start pose, no device touched
  const SE3d back = EMPoseEstimation(none, none, SE3d(), EIGHTPT, false);
  std::printf("thrown %d identity %d\n", thrown, back.rotationMatrix()(0, 0) == 1.0 && back.translation()[0] == 0.0);
  return 0;
}
"""


def test_the_facades_unsupported_combinations_throw(tmp_path):
    import shutil
    import subprocess
    gxx = shutil.which("g++")
    assert gxx, "g++ builds the host facade, so it is there"
    src, exe = tmp_path / "em_facade.cc", str(tmp_path / "em_facade")
    src.write_text(FACADE_PROGRAM)
    lib_dir = os.path.join(ROOT, "pnec_amd")
    subprocess.run([gxx, "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "pnec_amd", "csrc", "host"), str(src), "-o", exe, "-L" + lib_dir,
                    "-lpnec_host", "-lpnec_hip", "-Wl,-rpath," + lib_dir], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "thrown 8 identity 1" in r.stdout, r.stdout


# ---- the checker ------------------------------------------------------------------------------------------------------
def test_every_compared_case_satisfies_both_conditions():
    all_cases = ec.cases() + ec.outlier_case()
    assert tuple(c.n for c in ec.cases()) == ec.SIZES
    for c in all_cases:
        x = c.expected
        assert x["status"] == ec.EP_OK and x["choice"] in (0, 1, 2, 3)
        assert x["gap"] >= ec.GAP_MIN, (c.n, x["gap"])
        assert ec.quality_margin(x["quality"]) >= ec.MARGIN_MIN, (c.n, x["quality"])
        assert c.noise == (0.0 if c.n in ec.NOISE_FREE_SIZES else ec.NOISE)
        # at most 7e-9 at the gap bound, inside the 1e-8 rad the front stages are held to
        assert c.tol <= ec.TOL_FACTOR * ec.EPS / ec.GAP_MIN < 1e-8
        print(f"N = {c.n}: draw {c.draws}, gap {x['gap']:.3e}, margin {ec.quality_margin(x['quality']):.2f}, tol {c.tol:.2e}")
    for c in ec.short_cases():
        assert c.expected["status"] == ec.EP_TOO_FEW and np.isnan(c.expected["E"]).all()


def test_the_checker_returns_the_true_pose_on_noise_free_pairs():
    for c in ec.cases():
        if c.noise:
            continue
        x = c.expected
        dr, dt = ec.rotation_distance(x["R"], c.R), ec.translation_distance(x["t"], c.t)
        print(f"N = {c.n}: rotation {dr:.2e}, translation {dt:.2e}, tol {c.tol:.2e}")
        assert dr <= c.tol and dt <= c.tol
        # f1' E f2 = 0 with E = [t]x R, up to the sign of step 2
        tx = np.array([[0.0, -c.t[2], c.t[1]], [c.t[2], 0.0, -c.t[0]], [-c.t[1], c.t[0], 0.0]])
        e = (tx @ c.R).reshape(9)
        e = e / np.linalg.norm(e) * ec.sign_largest(e)
        assert np.linalg.norm(e - x["E"]) <= c.tol


def test_eigh_of_the_normal_matrix_and_svd_of_a_agree_on_every_case():
    worst = 0.0
    for c in ec.cases() + ec.outlier_case():
        x = c.expected
        y = ec.pose_from_null_vector(ec.null_vector_svd(c.f1, c.f2), c.f1, c.f2, c.quality_all)
        assert y["choice"] == x["choice"]
        d = max(ec.rotation_distance(x["R"], y["R"]), ec.translation_distance(x["t"], y["t"]),
                float(np.linalg.norm(x["E"] - y["E"])))
        worst = max(worst, d * x["gap"] / ec.EPS)
        assert d <= c.tol, (c.n, d, c.tol)
    print(f"eigh(A'A) against svd(A): worst difference {worst:.3f} * 2^-52 / gap")


def test_the_outlier_case_separates_the_two_quality_rules():
    sample, full = ec.outlier_case()
    assert np.array_equal(sample.f2, full.f2) and not sample.quality_all and full.quality_all
    assert not ec.true_candidate(sample.expected, sample.R, sample.t)
    assert ec.true_candidate(full.expected, full.R, full.t)
    assert sample.expected["choice"] != full.expected["choice"]
    # a negated row of A is the same term of A'A: E is the clean pair's
    assert np.array_equal(sample.expected["E"], full.expected["E"])


def test_the_candidate_set_does_not_depend_on_the_sign_of_e():
    c = ec.cases()[6]
    e, _ = ec.null_vector_eigh(c.f1, c.f2)
    S1, Ra1, Rb1, t1 = ec.decompose(e.reshape(3, 3))
    S2, Ra2, Rb2, t2 = ec.decompose(-e.reshape(3, 3))
    assert np.allclose(Ra1, Rb2, atol=1e-12) and np.allclose(Rb1, Ra2, atol=1e-12) and np.allclose(t1, t2, atol=1e-12)
    for R in (Ra1, Rb1):
        assert abs(np.linalg.det(R) - 1.0) < 1e-12 and np.allclose(R @ R.T, np.eye(3), atol=1e-12)
