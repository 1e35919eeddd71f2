"""The RANSAC forms of the essential-matrix baselines without a GPU: pnec_hip_essential_ransac is declared, bound and
exported within ABI 8, its argument checks refuse before the handle is read or a device is touched, the Python, facade
and pybind names exist, the numpy sampler is the oracle's hash draw for draw, and the checker of
tests/essential_ransac_cases.py -- the yardstick of the GPU tests -- satisfies every condition those tests put on the
device: its two routes to the null space give the same iterations, attempts, best attempt and mask on all 48 pairs, it
keeps the planted outliers out and the planted inliers in, it obeys the call's own contract, and it skips attempts
without a model."""
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
import essential_ransac_cases as rc
import minimal_solver_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALGORITHMS = pytest.mark.parametrize("algorithm", list(rc.ALGORITHMS), ids=[rc.NAMES[a] for a in rc.ALGORITHMS])
OUTPUTS = ["out_q", "out_t", "out_E", "out_singular", "out_inlier_mask", "out_inlier_count", "out_iterations",
           "out_attempts", "out_best_attempt", "out_status"]


# ---- 1. the symbol ----------------------------------------------------------------------------------------------------
def test_symbol_is_declared_bound_and_exported_within_abi_8():
    assert "pnec_hip_essential_ransac" in capi.SYMBOLS
    L = capi.lib()
    assert getattr(L, "pnec_hip_essential_ransac") is not None
    assert capi.ABI_VERSION == 8 and L.pnec_hip_abi_version() == 8
    header = open(os.path.join(ROOT, "include", "pnec_hip.h")).read()
    assert "#define PNEC_HIP_ABI_VERSION 8" in header
    assert "#define PNEC_HIP_EM_EIGHTPT 3" in header and capi.EM_EIGHTPT == 3 == rc.EIGHTPT
    assert (capi.EM_NISTER, capi.EM_SEVENPT) == (rc.NISTER, rc.SEVENPT)
    for name, value in (("OK", 0), ("TOO_FEW", 1), ("NO_MODEL", 2)):
        assert f"PNEC_HIP_ER_{name} = {value}" in header and getattr(capi, "ER_" + name) == value
        assert getattr(rc, "ER_" + name) == value
    decl = re.search(r"int pnec_hip_essential_ransac\(([^;]*)\);", header)
    assert decl, "the header declares the call"
    params = [p.strip() for p in decl.group(1).replace("\n", " ").split(",")]
    assert params[:6] == ["pnec_hip_problem *p", "int32_t algorithm", "uint64_t seed", "int64_t first_pair_id",
                          "int32_t max_iterations", "double threshold"]
    assert params[-2:] == ["int space", "void *stream"]
    assert [p.split("*")[-1] for p in params[6:16]] == OUTPUTS
    assert params[10].startswith("uint8_t") and all(p.startswith("int32_t") for p in params[11:16])
    # problem, five parameters, ten outputs, space, stream
    at = L.pnec_hip_essential_ransac.argtypes
    assert len(params) == 18 and len(at) == 18
    assert (at[1], at[2], at[3], at[4], at[5], at[16]) == (C.c_int32, C.c_uint64, C.c_int64, C.c_int32, C.c_double, C.c_int)


# ---- 2. refusals ------------------------------------------------------------------------------------------------------
def _call(p, algorithm, seed, first, max_it, threshold, outs, space=capi.MEM_HOST):
    L = capi.lib()
    rc_ = L.pnec_hip_essential_ransac(p, algorithm, seed, first, max_it, threshold, *outs, space, None)
    return rc_, (L.pnec_hip_last_error() or b"").decode()


def test_bad_arguments_are_refused_before_the_handle_is_read():
    SENT = -7.25
    doubles = [np.full(n, SENT) for n in (4, 3, 9, 3)]
    mask = np.full(16, 9, dtype=np.uint8)
    ints = [np.full(1, -5, dtype=np.int32) for _ in range(5)]
    outs = tuple(a.ctypes.data for a in doubles + [mask] + ints)
    # a stand-in handle: every check below must return before the handle is read
    fake = C.create_string_buffer(4096)
    h = C.cast(fake, C.c_void_p)
    for args, word in (((None, 1, 1, 0, 40, 1e-6, outs), "problem"),
                       ((h, 0, 1, 0, 40, 1e-6, outs), "algorithm"),
                       ((h, 4, 1, 0, 40, 1e-6, outs), "algorithm"),
                       ((h, -1, 1, 0, 40, 1e-6, outs), "algorithm"),
                       ((h, 1, 1, 0, -1, 1e-6, outs), "max_iterations"),
                       ((h, 2, 1, 0, 40, 0.0, outs), "threshold"),
                       ((h, 2, 1, 0, 40, -1e-6, outs), "threshold"),
                       ((h, 3, 1, 0, 40, float("nan"), outs), "threshold"),
                       ((h, 3, 1, 0, 40, float("inf"), outs), "threshold"),
                       ((h, 1, 1, -1, 40, 1e-6, outs), "first_pair_id"),
                       ((h, 1, 1, 0, 40, 1e-6, (None,) * 10), "output"),
                       ((h, 3, 2 ** 64 - 1, 0, 0, 1e-6, (None,) * 10), "output")):
        r, msg = _call(*args)
        assert r == capi.ERR_INVALID_ARGUMENT == -1, (r, msg)
        assert word in msg, msg
    for space in (7, -1):
        r, msg = _call(h, 1, 1, 0, 40, 1e-6, outs, space=space)
        assert r == -1 and "memory space" in msg
    for a in doubles:
        assert np.all(a == SENT)
    assert np.all(mask == 9)
    for a in ints:
        assert np.all(a == -5)


# ---- 3. names ---------------------------------------------------------------------------------------------------------
def test_python_facade_and_pybind_expose_the_new_names():
    assert "EssentialRansac" in pnec_amd.__all__ and pnec_amd.EssentialRansac is not None
    p = inspect.signature(pnec_amd.Batch.essential_ransac).parameters
    assert list(p) == ["self", "algorithm", "seed", "max_iterations", "threshold", "first_pair_id", "on_device"]
    assert (p["seed"].default, p["max_iterations"].default, p["threshold"].default, p["first_pair_id"].default,
            p["on_device"].default) == (1, 5000, 1e-6, 0, None)
    assert [f.name for f in dataclasses.fields(pnec_amd.EssentialRansac)] == [
        "q", "t", "E", "singular", "mask", "count", "iterations", "attempts", "best_attempt", "status"]
    import pnec_amd.pypnec as pypnec
    assert "essential_ransac" in dir(pypnec)
    facade = open(os.path.join(ROOT, "pnec_amd", "csrc", "host", "pnec_host.h")).read()
    assert re.search(r"SE3d RansacEMPoseEstimation\(const bearingVectors_t &bvs1, const bearingVectors_t &bvs2, "
                     r"const SE3d &initial_pose,\s*algorithm_t algorithm, std::vector<int> \*inliers = nullptr, "
                     r"int max_iterations = 5000,\s*double threshold = 1e-6, uint64_t seed = 1\);", facade)
    with open(os.path.join(ROOT, "pnec_amd", "libpnec_host.so"), "rb") as f:
        assert b"RansacEMPoseEstimation" in f.read()


def test_an_unknown_algorithm_name_is_refused_in_python():
    b = pnec_amd.Batch.__new__(pnec_amd.Batch)      # no handle: the check comes first
    for bad in ("stewenius", "", 0, 4):
        with pytest.raises(ValueError):
            pnec_amd.Batch.essential_ransac(b, bad)


# ---- 4. the facade ----------------------------------------------------------------------------------------------------
FACADE_PROGRAM = r"""
#include <cstdio>
#include <stdexcept>
#include <string>
#include "pnec_host.h"
using namespace pnec;
using namespace pnec::rel_pose_estimation;
int main() {
  const bearingVectors_t none;
  int thrown = 0, not_built = 0, identity = 0, empty = 0;
  try {
    RansacEMPoseEstimation(none, none, SE3d(), STEWENIUS);
  } catch (const std::invalid_argument &e) {
    ++thrown;
    not_built += std::string(e.what()).find("not built") != std::string::npos;
  }
  // the three that are built, on a pair without correspondences: the start pose, no inliers, no device touched
  for (algorithm_t a : {NISTER, SEVENPT, EIGHTPT}) {
    std::vector<int> inliers(3, 7);
    const SE3d back = RansacEMPoseEstimation(none, none, SE3d(), a, &inliers);
    identity += back.rotationMatrix()(0, 0) == 1.0 && back.translation()[0] == 0.0;
    empty += inliers.empty();
  }
  // EMPoseEstimation keeps refusing ransac = true, for every algorithm
  for (algorithm_t a : {NISTER, SEVENPT, EIGHTPT}) {
    try {
      EMPoseEstimation(none, none, SE3d(), a, true);
    } catch (const std::invalid_argument &) {
      ++thrown;
    }
  }
  std::printf("thrown %d not_built %d identity %d empty %d\n", thrown, not_built, identity, empty);
  return 0;
}
"""


def test_the_facade_returns_the_start_pose_on_an_empty_pair_and_throws_for_stewenius(tmp_path):
    import shutil
    import subprocess
    gxx = shutil.which("g++")
    assert gxx, "g++ builds the host facade, so it is there"
    src, exe = tmp_path / "em_ransac_facade.cc", str(tmp_path / "em_ransac_facade")
    src.write_text(FACADE_PROGRAM)
    lib_dir = os.path.join(ROOT, "pnec_amd")
    subprocess.run([gxx, "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "pnec_amd", "csrc", "host"), str(src), "-o", exe, "-L" + lib_dir,
                    "-lpnec_host", "-lpnec_hip", "-Wl,-rpath," + lib_dir], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "thrown 4 not_built 1 identity 3 empty 3" in r.stdout, r.stdout


# ---- 5. the sampler ---------------------------------------------------------------------------------------------------
def test_the_numpy_sampler_is_the_oracles_hash_draw_for_draw(oracle):
    f = oracle.lib().pnec_oracle_rng_uniform
    seeds = (0, 1, 5, 2 ** 32 + 5, 2 ** 63 + 11, 2 ** 64 - 1)
    n = 0
    for seed in seeds:
        for pair in (0, 1, 47, 2 ** 40 + 3):
            for attempt in (0, 1, 329, 2 ** 20 + 1):
                for d in (0, 1, 2, 1000):
                    assert rc.rng_uniform(seed, pair, attempt, d) == f(seed, pair, attempt, d), (seed, pair, attempt, d)
                    n += 1
    assert n >= 300
    # all 64 bits of the seed enter: 5 and 2^32 + 5 do not draw alike
    a = [rc.rng_uniform(5, 0, 0, d) for d in range(16)]
    b = [rc.rng_uniform(2 ** 32 + 5, 0, 0, d) for d in range(16)]
    assert all(x != y for x, y in zip(a, b))
    assert all(0.0 <= x < 1.0 for x in a + b)
    s = rc.sample_of(1, 3, 2, 9, 9)
    assert sorted(s) == list(range(9))


# ---- 6. the inputs ----------------------------------------------------------------------------------------------------
@ALGORITHMS
def test_the_inputs_are_the_48_pairs_of_the_description(algorithm):
    ps = rc.pairs(algorithm)
    S = rc.SAMPLE[algorithm]
    assert len(ps) == 48 and [p.n for p in ps[:8]] == [S, S + 1, 24, 40, 64, 65, 100, 130]
    for i, p in enumerate(ps):
        assert p.n == rc.sizes(algorithm)[i % 8] and p.share == (0.0, 0.10, 0.25)[(i // 8) % 3]
        assert int(p.planted.sum()) == int(round(p.share * p.n))
        assert np.all(np.isfinite(p.f1)) and np.all(np.isfinite(p.f2))
        assert np.allclose(np.linalg.norm(p.f2, axis=1), 1.0) and np.allclose(np.linalg.norm(p.f1, axis=1), 1.0)
    assert (rc.THRESHOLD, rc.MAX_ITERATIONS, rc.SEED, rc.FIRST_PAIR_ID, rc.NOISE) == (1e-6, 40, 1, 0, 1e-4)


# ---- 7. the two routes ------------------------------------------------------------------------------------------------
@ALGORITHMS
def test_eigh_and_svd_null_spaces_give_the_same_run_on_all_48_pairs(algorithm):
    same = 0
    for i, (p, x) in enumerate(zip(rc.pairs(algorithm), rc.expected(algorithm))):
        y = rc.ransac_np(p.f1, p.f2, algorithm, pair_id=rc.FIRST_PAIR_ID + i, null_space=mc.null_space_svd)
        ok = (all(x[k] == y[k] for k in ("status", "iterations", "attempts", "best_attempt", "count"))
              and np.array_equal(x["mask"], y["mask"]))
        if not ok:
            print(f"{rc.NAMES[algorithm]} pair {i} (N = {p.n}): eigh {x['iterations']}, {x['attempts']}, "
                  f"{x['best_attempt']}, {x['count']}; svd {y['iterations']}, {y['attempts']}, {y['best_attempt']}, {y['count']}")
        same += ok
    print(f"{rc.NAMES[algorithm]}: {same} of 48 pairs the same by both routes")
    assert same == 48


# ---- 8. what it is for ------------------------------------------------------------------------------------------------
@ALGORITHMS
def test_the_checker_keeps_planted_outliers_out_and_planted_inliers_in(algorithm):
    seen = 0
    for i, (p, x) in enumerate(zip(rc.pairs(algorithm), rc.expected(algorithm))):
        if p.n < 40 or p.share > 0.10:
            continue
        seen += 1
        m = x["mask"].astype(bool)
        wrong, kept, inliers = int((m & p.planted).sum()), int((m & ~p.planted).sum()), int((~p.planted).sum())
        print(f"{rc.NAMES[algorithm]} pair {i} (N = {p.n}, {p.share:.0%}): {wrong} planted outliers in the mask, "
              f"{kept} of {inliers} planted inliers")
        assert x["status"] == rc.ER_OK and wrong <= 2 and kept >= 0.9 * inliers, (i, wrong, kept, inliers)
        # the eight-point over all the rows the mask keeps finds the scene's rotation
        refit = ec.eight_point_np(p.f1[m], p.f2[m], quality_all=True)
        assert refit["status"] == ec.EP_OK and ec.rotation_distance(refit["R"], p.R) <= 1e-2
    assert seen == 20


# ---- 9. the contract, on the checker ------------------------------------------------------------------------------------
@ALGORITHMS
def test_the_checker_obeys_the_calls_contract_on_every_pair(algorithm):
    for i, (p, x) in enumerate(zip(rc.pairs(algorithm), rc.expected(algorithm))):
        rc.check_contract(p, algorithm, rc.FIRST_PAIR_ID + i, x, x["R"])


# ---- 10. the skip rule and the edges ------------------------------------------------------------------------------------
@ALGORITHMS
def test_the_checker_skips_attempts_without_a_model_and_reports_the_edges(algorithm):
    short, empty, holes = rc.edge_pairs(algorithm)
    for p in (short, empty):
        x = rc.ransac_np(p.f1, p.f2, algorithm)
        assert x["status"] == rc.ER_TOO_FEW and x["iterations"] == 0 and x["attempts"] == 0 and x["best_attempt"] == -1
        assert x["count"] == 0 and not x["mask"].any() and np.isnan(x["R"]).all() and np.isnan(x["E"]).all()
    assert (short.n, empty.n, holes.n) == (rc.SAMPLE[algorithm] - 1, 0, 14)
    assert int(np.isnan(holes.f2).any(axis=1).sum()) == 4
    x = rc.ransac_np(holes.f1, holes.f2, algorithm)
    print(f"{rc.NAMES[algorithm]} N = 14 with four NaN rows: {x['attempts']} attempts, {x['iterations']} iterations, "
          f"{x['count']} inliers")
    assert x["status"] == rc.ER_OK and x["attempts"] > x["iterations"] >= 1
    assert not x["mask"][np.isnan(holes.f2).any(axis=1)].any()
    rc.check_contract(holes, algorithm, rc.FIRST_PAIR_ID, x, x["R"], skips_expected=True)
    n = rc.nan_pair()
    y = rc.ransac_np(n.f1, n.f2, algorithm, max_iterations=rc.NAN_PAIR_MAX_ITERATIONS)
    assert y["status"] == rc.ER_NO_MODEL and y["attempts"] == 30 and y["iterations"] == 0 and y["best_attempt"] == -1
    assert y["count"] == 0 and not y["mask"].any() and np.isnan(y["t"]).all()
