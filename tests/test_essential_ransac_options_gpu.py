"""pnec_hip_essential_ransac on the device away from the parameters of test_essential_ransac_gpu.py, and its facade and
pybind entry points on real pairs.  The inputs, the cases and the checker's answers are those of
tests/essential_ransac_option_cases.py; test_essential_ransac_options_cpu.py asserts on the checker every condition under
which the comparisons below are well posed.

Per (algorithm, case) one ragged batch of 16 pairs in DEVICE space, launched once for the module: N from the sample size
to 4097 rows, at most 41 iterations -- milliseconds; nothing here uses the defaults' 5000 iterations.

Against the checker the discrete outputs (status, iterations, attempts, best attempt, count, mask) may differ on at most 1
of a case's 16 pairs -- the rate test_essential_ransac_gpu.py allows, 2 in 48, rounded up; the checker's own two routes
differ on none -- and on none at max_iterations = 0, where nothing is computed.  The contract holds on every pair whether
it agrees or not.  Pairs of repeated rows are never compared with the checker (its two routes disagree there): only what
the header fixes for any input is asserted on them.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from pnec_amd import Batch, capi

import eight_point_cases as ec
import essential_ransac_cases as rc
import essential_ransac_option_cases as oc
import minimal_solver_cases as mc
from test_essential_ransac_gpu import FIELDS, _bits, _row, _run, _same_rows

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEC = capi.MODE_NEC
DOUBLES = ("q", "t", "E", "singular")
ALGORITHMS = pytest.mark.parametrize("algorithm", list(rc.ALGORITHMS), ids=[rc.NAMES[a] for a in rc.ALGORITHMS])
CASES = pytest.mark.parametrize("name", list(oc.CASE_NAMES))
MAX_DIFFERING = 1              # of a case's 16 pairs, and of the 12 pairs of pure rotation
SEED64 = 2 ** 63 + 2 ** 40 + 5


def _torch():
    import torch
    return torch


_launched = {}


def launch(algorithm, name):
    """The 16 pairs at the case `name` in DEVICE space, once per (algorithm, case) for the module."""
    if (algorithm, name) not in _launched:
        _launched[algorithm, name] = _run(algorithm, list(oc.pairs(algorithm)), **oc.CASES[name].params)
    return _launched[algorithm, name]


def rotation_launch(algorithm):
    if (algorithm, "rotation") not in _launched:
        _launched[algorithm, "rotation"] = _run(algorithm, list(oc.rotation_pairs(algorithm)), **oc.DEFAULT.params)
    return _launched[algorithm, "rotation"]


def _pose_tol(p, algorithm, seed, pair_id, best_attempt):
    """The tolerance of test_essential_ransac_gpu.py for a chosen pose, for the rows the model came from: 32 kappa 2^-52
    with the sample's own condition number, 32 * 2^-52 / gap for the eight-point."""
    idx = rc.sample_of(seed, pair_id, best_attempt, p.n, rc.SAMPLE[algorithm])[:rc.M_ROWS[algorithm]]
    s1, s2 = p.f1[idx], p.f2[idx]
    if algorithm == rc.EIGHTPT:
        w = ec.null_vector_eigh(s1, s2)[1]
        return ec.TOL_FACTOR * ec.EPS / ((w[1] - w[0]) / w[8])
    sols = mc.solutions_of(mc.null_space_eigh(s1, s2, mc.N_NULL[algorithm])[0], algorithm)
    return mc.TOL_FACTOR * mc.kappa_of(s1, s2, algorithm, sols) * mc.EPS


def _against_the_checker(algorithm, label, ps, out, off, xs, case):
    """-> the pairs whose discrete outputs differ from the checker's; the pose of every other pair is asserted."""
    differing = []
    for i, (p, x) in enumerate(zip(ps, xs)):
        g = _row(out, off, i)
        if not oc.same_run(g, x):
            differing.append(i)
            print(f"{rc.NAMES[algorithm]} {label} pair {i} (N = {p.n}, {p.share:.0%}) differs: device "
                  f"{[int(g[k]) for k in oc.DISCRETE]}, checker {[int(x[k]) for k in oc.DISCRETE]}, "
                  f"{int((g['mask'] != x['mask']).sum())} rows of the mask")
            continue
        if x["status"] != rc.ER_OK:
            assert all(np.isnan(g[k]).all() for k in DOUBLES), i
            continue
        tol = _pose_tol(p, algorithm, case.seed, case.first_pair_id + i, int(x["best_attempt"]))
        dR = ec.rotation_distance(ec.rotation_from_quaternion(g["q"]), x["R"])
        dt = ec.translation_distance(g["t"], x["t"])
        print(f"{rc.NAMES[algorithm]} {label} pair {i} (N = {p.n}): rotation {dR:.2e}, translation {dt:.2e}, tol {tol:.2e}")
        assert dR <= tol and dt <= tol, (i, dR, dt, tol)
    return differing


def _no_model(g, n):
    assert g["status"] == capi.ER_NO_MODEL and g["best_attempt"] == -1 and g["count"] == 0
    assert g["mask"].shape == (n,) and not g["mask"].any()
    assert all(np.isnan(g[k]).all() for k in DOUBLES)


def _unit(g):
    assert abs(np.linalg.norm(g["t"]) - 1.0) <= 1e-12 and abs(np.linalg.norm(g["q"]) - 1.0) <= 1e-12


# ---- 1. against the checker ---------------------------------------------------------------------------------------------
@ALGORITHMS
@CASES
def test_the_device_runs_the_checkers_rule_at_every_case(algorithm, name):
    out, off = launch(algorithm, name)
    case = oc.CASES[name]
    differing = _against_the_checker(algorithm, name, oc.pairs(algorithm), out, off, oc.expected(algorithm, name), case)
    print(f"{rc.NAMES[algorithm]} {name}: {len(differing)} of 16 pairs differ from the checker: {differing}")
    assert len(differing) <= (0 if name == "it0" else MAX_DIFFERING), differing
    if name == "it0":
        for i, p in enumerate(oc.pairs(algorithm)):
            g = _row(out, off, i)
            _no_model(g, p.n)
            assert g["iterations"] == 0 and g["attempts"] == 0


# ---- 2. the contract ----------------------------------------------------------------------------------------------------
@ALGORITHMS
@CASES
def test_every_pair_of_every_case_obeys_the_contract(algorithm, name):
    out, off = launch(algorithm, name)
    case = oc.CASES[name]
    for i, p in enumerate(oc.pairs(algorithm)):
        g = _row(out, off, i)
        if name == "it0":
            _no_model(g, p.n)
            continue
        rc.check_contract(p, algorithm, case.first_pair_id + i, g, ec.rotation_from_quaternion(g["q"]),
                          max_iterations=case.max_iterations, threshold=case.threshold, seed=case.seed)
        _unit(g)


# ---- 3. a pair alone, host space, no mask -----------------------------------------------------------------------------------
@ALGORITHMS
def test_a_pair_alone_with_its_64_bit_id_has_the_bits_it_had_in_the_batch(algorithm):
    out, off = launch(algorithm, "seed64")
    case, ps = oc.CASES["seed64"], oc.pairs(algorithm)
    assert ps[7].n == 4097
    for i in (3, 7, 12):
        alone, off_alone = _run(algorithm, [ps[i]], **dict(case.params, first_pair_id=2 ** 33 + 7 + i))
        assert _same_rows(out, off, [i], alone, off_alone, [0]) == [], i


@ALGORITHMS
@pytest.mark.parametrize("name", ["tight", "seed64", "it1"])
def test_host_space_gives_the_bits_of_device_space(algorithm, name):
    out, off = launch(algorithm, name)
    host, off_host = _run(algorithm, list(oc.pairs(algorithm)), on_device=False, **oc.CASES[name].params)
    assert _same_rows(out, off, range(oc.N_PAIRS), host, off_host, range(oc.N_PAIRS)) == []


@ALGORITHMS
def test_a_call_without_the_mask_ends_capped_pairs_with_the_same_counts_and_poses(algorithm):
    out, off = launch(algorithm, "tight")
    case, P = oc.CASES["tight"], oc.N_PAIRS
    assert int((out["iterations"] == case.max_iterations + 1).sum()) >= 1      # the early exit, at a capped pair
    torch = _torch()
    o, f1, f2 = rc.batch_arrays(list(oc.pairs(algorithm)))
    with Batch(NEC, o) as b:
        b.fill(torch.as_tensor(f1, device="cuda:0"), torch.as_tensor(f2, device="cuda:0"))
        doubles = [torch.zeros((P, w), dtype=torch.float64, device="cuda:0") for w in (4, 3, 9, 3)]
        ints = [torch.full((P,), -9, dtype=torch.int32, device="cuda:0") for _ in range(5)]
        capi.check(capi.lib().pnec_hip_essential_ransac(
            b._h, algorithm, case.seed, case.first_pair_id, case.max_iterations, case.threshold,
            *[t.data_ptr() for t in doubles], None, *[t.data_ptr() for t in ints], capi.MEM_DEVICE,
            torch.cuda.current_stream(0).cuda_stream))
        torch.cuda.synchronize()
    for t, k in zip(doubles, DOUBLES):
        assert np.array_equal(_bits(t.cpu().numpy()), _bits(out[k])), k
    for t, k in zip(ints, ("count", "iterations", "attempts", "best_attempt", "status")):
        assert np.array_equal(t.cpu().numpy(), out[k]), k


# ---- 4. pure rotation ---------------------------------------------------------------------------------------------------
def test_pure_rotation_runs_the_checkers_rule_and_obeys_the_contract():
    differing = []
    for algorithm in rc.ALGORITHMS:
        out, off = rotation_launch(algorithm)
        ps, xs = oc.rotation_pairs(algorithm), oc.rotation_expected(algorithm)
        differing += [(rc.NAMES[algorithm], i)
                      for i in _against_the_checker(algorithm, "pure rotation", ps, out, off, xs, oc.DEFAULT)]
        for i, (p, x) in enumerate(zip(ps, xs)):
            g = _row(out, off, i)
            Rg = ec.rotation_from_quaternion(g["q"])
            rc.check_contract(p, algorithm, rc.FIRST_PAIR_ID + i, g, Rg)
            _unit(g)
            print(f"{rc.NAMES[algorithm]} pure rotation N = {p.n}: the device's rotation {ec.rotation_distance(Rg, p.R):.2e} "
                  f"from the scene's, the checker's {ec.rotation_distance(x['R'], p.R):.2e}; inliers {int(g['count'])} "
                  f"and {int(x['count'])}")
    print(f"pure rotation: {len(differing)} of 12 pairs differ from the checker: {differing}")
    assert len(differing) <= MAX_DIFFERING, differing


# ---- 5. repeated rows ---------------------------------------------------------------------------------------------------
@ALGORITHMS
def test_repeated_rows_end_within_the_headers_bounds_and_leave_their_neighbours_alone(algorithm):
    first, second = oc.pairs(algorithm)[1], oc.pairs(algorithm)[5]
    rep = list(oc.repeated_pairs(algorithm))
    out, off = _run(algorithm, [first] + rep + [second])
    for j, p in enumerate(rep, start=1):
        g = _row(out, off, j)
        print(f"{rc.NAMES[algorithm]} repeated rows N = {p.n}: {[int(g[k]) for k in oc.DISCRETE]}")
        assert g["status"] in (capi.ER_OK, capi.ER_NO_MODEL)
        assert g["attempts"] - g["iterations"] <= rc.SKIP_FACTOR * rc.MAX_ITERATIONS
        assert 0 <= g["iterations"] <= rc.MAX_ITERATIONS + 1
        assert int(g["count"]) == int(g["mask"].sum())
        if g["status"] == capi.ER_NO_MODEL:
            _no_model(g, p.n)
            continue
        assert 0 <= g["best_attempt"] < g["attempts"]
        with np.errstate(invalid="ignore"):
            score = rc.scores_of(p.f1, p.f2, ec.rotation_from_quaternion(g["q"]), g["t"])
            clear = ~(np.abs(score - rc.THRESHOLD) <= oc.MARGIN)
            assert np.array_equal(g["mask"].astype(bool)[clear], (score < rc.THRESHOLD)[clear])
    # the generic pairs at either end: the bits of launches without the degenerate pairs (their ids here are 0 and 5)
    for j, p in ((0, first), (5, second)):
        alone, off_alone = _run(algorithm, [p], first_pair_id=rc.FIRST_PAIR_ID + j)
        assert alone["status"][0] == capi.ER_OK
        assert _same_rows(out, off, [j], alone, off_alone, [0]) == [], j


# ---- 6. the facade and pybind on real pairs -------------------------------------------------------------------------------
FACADE_PAIRS = (1, 5, 7)         # of the half without outliers: N = 63, 129, 4097
_KW = dict(max_iterations=rc.MAX_ITERATIONS, threshold=rc.THRESHOLD)


def _batch_of_one(algorithm, p, seed):
    out, off = _run(algorithm, [p], seed=seed, first_pair_id=0, **_KW)
    return _row(out, off, 0)


@ALGORITHMS
def test_pybind_returns_the_pose_and_the_inliers_of_the_one_pair_batch_for_both_seeds(algorithm):
    import pnec_amd.pypnec as pypnec
    seen = {}
    for seed in (1, SEED64):
        for i in FACADE_PAIRS:
            p = oc.pairs(algorithm)[i]
            T, idx = pypnec.essential_ransac(p.f1, p.f2, rc.WORDS[algorithm], seed=seed, **_KW)
            g = _batch_of_one(algorithm, p, seed)
            assert g["status"] == capi.ER_OK and g["count"] >= 1
            assert np.array_equal(np.asarray(idx), np.nonzero(g["mask"])[0])
            assert T.shape == (4, 4) and np.array_equal(T[3], [0.0, 0.0, 0.0, 1.0])
            assert np.abs(T[:3, :3] - ec.rotation_from_quaternion(g["q"])).max() <= 1e-15
            assert np.array_equal(_bits(T[:3, 3]), _bits(g["t"] * g["singular"][0]))
            seen[seed, i] = (T, np.asarray(idx))
    changed = [i for i in FACADE_PAIRS if not (np.array_equal(seen[1, i][1], seen[SEED64, i][1])
                                               and np.array_equal(seen[1, i][0], seen[SEED64, i][0]))]
    print(f"{rc.NAMES[algorithm]}: the 64-bit seed changes the inliers or the pose of pairs {changed}")
    assert len(changed) >= 1


FACADE_PROGRAM = r"""
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "pnec_host.h"
using namespace pnec;
using namespace pnec::rel_pose_estimation;
// <file: int64 n, f1 [n,3], f2 [n,3]> <algorithm> <seed> <max_iterations> <threshold>
int main(int argc, char **argv) {
  if (argc != 6) return 2;
  std::FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 3;
  int64_t n = 0;
  if (std::fread(&n, sizeof n, 1, f) != 1 || n < 0 || n > 100000) return 4;
  bearingVectors_t b1((size_t)n), b2((size_t)n);
  for (bearingVectors_t *b : {&b1, &b2})
    for (Vector3d &v : *b)
      if (std::fread(v.data(), sizeof(double), 3, f) != 3) return 5;
  std::fclose(f);
  const uint64_t seed = std::strtoull(argv[3], nullptr, 10);
  std::vector<int> inliers;
  const SE3d T = RansacEMPoseEstimation(b1, b2, SE3d(), (algorithm_t)std::atoi(argv[2]), &inliers, std::atoi(argv[4]),
                                        std::strtod(argv[5], nullptr), seed);
  std::printf("seed %" PRIu64 "\nR", seed);
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) std::printf(" %a", T.rotationMatrix()(r, c));
  std::printf("\nt");
  for (int r = 0; r < 3; ++r) std::printf(" %a", T.translation()[r]);
  std::printf("\ninliers %zu", inliers.size());
  for (int i : inliers) std::printf(" %d", i);
  std::printf("\n");
  return 0;
}
"""


@pytest.fixture(scope="module")
def facade_program(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ builds the host facade, so it is there"
    d = tmp_path_factory.mktemp("em_ransac_facade")
    src, exe = d / "em_ransac_pair.cc", str(d / "em_ransac_pair")
    src.write_text(FACADE_PROGRAM)
    lib_dir = os.path.join(ROOT, "pnec_amd")
    subprocess.run([gxx, "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "pnec_amd", "csrc", "host"), str(src), "-o", exe, "-L" + lib_dir,
                    "-lpnec_host", "-lpnec_hip", "-Wl,-rpath," + lib_dir], check=True)
    return exe


@ALGORITHMS
def test_the_cpp_facade_gives_pybinds_pose_and_inliers_with_the_64_bit_seed(algorithm, facade_program, tmp_path):
    import pnec_amd.pypnec as pypnec
    p = oc.pairs(algorithm)[5]
    T, idx = pypnec.essential_ransac(p.f1, p.f2, rc.WORDS[algorithm], seed=SEED64, **_KW)
    assert len(idx) >= 1 and not np.array_equal(T, np.eye(4))
    data = tmp_path / "pair.bin"
    data.write_bytes(np.int64(p.n).tobytes() + np.ascontiguousarray(p.f1).tobytes() + np.ascontiguousarray(p.f2).tobytes())
    # a fresh child process: the program opens the device itself
    r = subprocess.run([facade_program, str(data), str(algorithm), str(SEED64), str(rc.MAX_ITERATIONS),
                        float(rc.THRESHOLD).hex()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    lines = dict(line.split(" ", 1) for line in r.stdout.strip().splitlines())
    assert int(lines["seed"]) == SEED64
    R = np.array([float.fromhex(w) for w in lines["R"].split()]).reshape(3, 3)
    t = np.array([float.fromhex(w) for w in lines["t"].split()])
    inliers = [int(w) for w in lines["inliers"].split()]
    assert inliers[0] == len(inliers) - 1 and np.array_equal(inliers[1:], np.asarray(idx))
    assert np.array_equal(_bits(R), _bits(T[:3, :3])) and np.array_equal(_bits(t), _bits(T[:3, 3]))
