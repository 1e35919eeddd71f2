"""Keypoint undistortion without a GPU: pnec_hip_undistort_keypoints is declared, bound and exported within ABI 8, its
argument checks refuse before a device is touched, the Python names exist with their defaults, Odometry keeps its first
nine parameters, and the numpy checker of tests/undistort_cases.py -- the yardstick of the GPU tests -- has the properties
the GPU tests rely on (measured here, on the three cameras and the 97 x 61 grid).  The facade's argument handling runs as
a stand-alone host program under the address and undefined-behaviour sanitizers; nothing is loaded into Python under one.
"""
import ctypes as C
import dataclasses
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import pnec_amd
from pnec_amd import capi

import undistort_cases as uc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_is_declared_bound_and_exported_within_abi_8():
    assert "pnec_hip_undistort_keypoints" in capi.SYMBOLS
    L = capi.lib()
    assert getattr(L, "pnec_hip_undistort_keypoints") is not None
    assert capi.ABI_VERSION == 8 and L.pnec_hip_abi_version() == 8
    header = open(os.path.join(ROOT, "include", "pnec_hip.h")).read()
    assert "#define PNEC_HIP_ABI_VERSION 8" in header
    assert re.search(r"#define PNEC_HIP_UNDISTORT_NEWTON\s+1u", header) and capi.UNDISTORT_NEWTON == uc.NEWTON == 1
    assert re.search(r"#define PNEC_HIP_UNDISTORT_PROPAGATE_COV\s+2u", header)
    assert capi.UNDISTORT_PROPAGATE_COV == uc.PROPAGATE_COV == 2
    for name, value in (("OK", 0), ("OUTSIDE", 1), ("NOT_CONVERGED", 2), ("NOT_FINITE", 3)):
        assert f"PNEC_HIP_UNDISTORT_{name} = {value}" in header
        assert getattr(capi, "UNDISTORT_" + name) == value == getattr(uc, name)
    decl = re.search(r"int pnec_hip_undistort_keypoints\(([^;]*)\);", header)
    assert decl, "the header declares the call"
    params = [p.strip() for p in decl.group(1).replace("\n", " ").split(",")]
    assert params[:2] == ["int device", "int64_t n_rows"] and params[-2:] == ["int space", "void *stream"]
    assert params[7:10] == ["int32_t fixed_iterations", "int32_t newton_iterations", "uint32_t flags"]
    at = L.pnec_hip_undistort_keypoints.argtypes
    assert len(params) == 18 and len(at) == 18
    assert at[0] is C.c_int and at[1] is C.c_int64 and at[7] is C.c_int32 and at[8] is C.c_int32 and at[9] is C.c_uint32
    assert at[16] is C.c_int


def test_every_refusal_comes_back_before_a_device_is_touched():
    SENT = -7.25
    n = 3
    pts1, pts2, o1, o2 = (np.full((n, 2), SENT) for _ in range(4))
    c2, c1, oc2, oc1 = (np.full((n, 3), SENT) for _ in range(4))
    s1, s2 = (np.full(n, 9, dtype=np.uint8) for _ in range(2))
    cam = uc.MILD.copy()
    p = lambda a: None if a is None else a.ctypes.data
    full = dict(n_rows=n, pts1=pts1, pts2=pts2, cov2=c2, cov1=c1, camera=cam, fixed=5, newton=20, flags=0, o1=o1, o2=o2,
                oc2=oc2, oc1=oc1, s1=s1, s2=s2, space=capi.MEM_HOST)

    def call(**change):
        a = dict(full, **change)
        L = capi.lib()
        # device 1 << 20 does not exist anywhere: a check that came after the device was touched would fail otherwise
        rc = L.pnec_hip_undistort_keypoints(1 << 20, a["n_rows"], p(a["pts1"]), p(a["pts2"]), p(a["cov2"]), p(a["cov1"]),
                                            p(a["camera"]), a["fixed"], a["newton"], a["flags"], p(a["o1"]), p(a["o2"]),
                                            p(a["oc2"]), p(a["oc1"]), p(a["s1"]), p(a["s2"]), a["space"], None)
        return rc, (L.pnec_hip_last_error() or b"").decode()

    refusals = [
        (dict(fixed=-1), "fixed_iterations"), (dict(fixed=65), "fixed_iterations"),
        (dict(newton=-1, flags=1), "newton_iterations"), (dict(newton=65, flags=3), "newton_iterations"),
        (dict(flags=4), "flags"), (dict(flags=0x80000001), "flags"),
        (dict(n_rows=-1), "n_rows"), (dict(n_rows=1 << 31), "n_rows"),
        (dict(camera=None), "camera"),
        (dict(o1=None), "output"), (dict(pts1=None, cov1=None, oc1=None, s1=None), "output"),
        (dict(o2=None), "output"), (dict(pts2=None, cov2=None, oc2=None, s2=None), "output"),
        (dict(oc2=None), "output"), (dict(cov2=None), "output"), (dict(oc1=None), "output"), (dict(cov1=None), "output"),
        (dict(pts1=None, o1=None, cov1=None, oc1=None), "status"), (dict(pts2=None, o2=None, cov2=None, oc2=None), "status"),
        (dict(pts2=None, o2=None, s2=None), "covariance"), (dict(pts1=None, o1=None, s1=None), "covariance"),
        (dict(space=7), "memory space"), (dict(space=-1), "memory space"),
    ]
    for change, word in refusals:
        rc, msg = call(**change)
        assert rc == capi.ERR_INVALID_ARGUMENT == -1, (change, rc, msg)
        assert word in msg, (change, msg)
    # not refusals: no rows (whatever the pointers), and iteration counts nobody looks at
    assert call(n_rows=0)[0] == 0
    assert call(n_rows=0, pts1=None, o2=None, cov2=None)[0] == 0
    assert call(n_rows=0, newton=99, flags=capi.UNDISTORT_PROPAGATE_COV)[0] == 0
    for a in (o1, o2, oc2, oc1):
        assert np.all(a == SENT)
    assert np.all(s1 == 9) and np.all(s2 == 9)


def test_python_names_and_defaults():
    assert {"undistort_keypoints", "camera_array", "Undistorted"} <= set(pnec_amd.__all__)
    assert pnec_amd.undistort_keypoints is pnec_amd.undistort.undistort_keypoints
    assert [f.name for f in dataclasses.fields(pnec_amd.Undistorted)] == ["pts1", "pts2", "cov2", "cov1", "status1", "status2"]
    sig = inspect.signature(pnec_amd.undistort_keypoints)
    assert list(sig.parameters) == ["camera", "pts1", "pts2", "cov2", "cov1", "fixed_iterations", "newton",
                                    "newton_iterations", "propagate_cov", "out"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["pts2"], d["cov2"], d["cov1"], d["fixed_iterations"], d["newton"], d["newton_iterations"], d["propagate_cov"],
            d["out"]) == (None, None, None, 5, False, 20, False, None)
    for k in ("fixed_iterations", "newton", "newton_iterations", "propagate_cov", "out"):
        assert sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY
    cam = pnec_amd.camera_array(1.0, 2.0, 3.0, 4.0)
    assert cam.dtype == np.float64 and cam.tolist() == [1.0, 2.0, 3.0, 4.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    assert pnec_amd.camera_array(1, 2, 3, 4, 5, 6, 7, 8, 9).tolist() == [1, 2, 3, 4, 5, 6, 7, 8, 9]
    assert list(inspect.signature(pnec_amd.camera_array).parameters) == ["fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3"]
    import pnec_amd.pypnec as pypnec
    assert "undistort" in dir(pypnec)
    facade = open(os.path.join(ROOT, "pnec_amd", "csrc", "host", "pnec_host.h")).read()
    assert "Vector2d Undistort(const Vector2d &point, const Matrix3d &K, const std::vector<double> &dist_coef);" in facade
    assert "std::vector<uint8_t> Undistort(std::vector<Vector2d> &points, std::vector<Covariance2d> *covs," in facade


def test_odometry_keeps_its_first_nine_parameters_and_takes_three_keyword_only_ones():
    params = inspect.signature(pnec_amd.Odometry.__init__).parameters
    assert list(params)[:9] == ["self", "n_sequences", "height", "width", "K_inv", "mode", "pipeline_options",
                                "min_displacement", "max_span"]
    assert list(params)[9:] == ["distortion", "undistort_newton", "undistort_propagate_cov", "tracker_kwargs"]
    for name, default in (("distortion", None), ("undistort_newton", False), ("undistort_propagate_cov", False)):
        assert params[name].kind is inspect.Parameter.KEYWORD_ONLY and params[name].default is default
    assert params["tracker_kwargs"].kind is inspect.Parameter.VAR_KEYWORD


def test_a_skewed_K_inv_with_a_distortion_is_refused():
    K = np.array([[110.0, 0.3, 63.5], [0.0, 110.0, 47.5], [0.0, 0.0, 1.0]])
    with pytest.raises(ValueError, match="upper triangular"):
        pnec_amd.Odometry(3, 96, 128, np.linalg.inv(K), distortion=[-0.05, 0.01, 1e-3, -5e-4])
    good = np.linalg.inv(np.array([[110.0, 0.0, 63.5], [0.0, 120.0, 47.5], [0.0, 0.0, 1.0]]))
    with pytest.raises(ValueError, match="4 or 5"):
        pnec_amd.Odometry(3, 96, 128, good, distortion=[-0.05, 0.01, 1e-3])
    bad_row = good.copy()
    bad_row[2, 0] = 1e-6
    with pytest.raises(ValueError, match="upper triangular"):
        pnec_amd.Odometry(3, 96, 128, bad_row, distortion=[-0.05, 0.01, 1e-3, -5e-4, 0.0])
    cam = pnec_amd.odometry._camera_from(good, [-0.05, 0.01, 1e-3, -5e-4])
    assert np.allclose(cam[:4], [110.0, 120.0, 63.5, 47.5], rtol=1e-14) and cam[4:].tolist() == [-0.05, 0.01, 1e-3, -5e-4, 0.0]


# ---------------------------------------------------------------------------------------------- the checker's own facts
@pytest.mark.parametrize("name", list(uc.CAMERAS))
def test_checker_newton_converges_everywhere_and_inverts_the_forward_model(name):
    cam, w, h = uc.CAMERAS[name]
    g = uc.grid(w, h)
    assert g.shape == (97 * 61, 2)
    r = uc.undistort_np(cam, g, flags=uc.NEWTON)
    rl = uc.undistort_np(cam, g, flags=uc.NEWTON, dtype=np.longdouble)
    r5 = uc.undistort_np(cam, g)
    r5l = uc.undistort_np(cam, g, dtype=np.longdouble)
    f = max(cam[0], cam[1])
    print(f"{name}: Newton steps at most {int(r.steps.max())}, forward residual {float(r.residual.max()) * f:.3e} px; five "
          f"fixed-point steps leave {float(r5.residual.max()) * f:.4f} px; float64 against longdouble "
          f"{float(np.abs(r.pts - rl.pts).max()):.3e} px (Newton), {float(np.abs(r5.pts - r5l.pts).max()):.3e} px (five steps)")
    assert np.all(r.status == uc.OK) and np.all(r5.status == uc.OK)
    assert int(r.steps.max()) <= 6
    # the forward model of the output returns the input within the stop rule
    x0, y0 = (g[:, 0] - cam[2]) / cam[0], (g[:, 1] - cam[3]) / cam[1]
    xd, yd = uc.forward(cam, (r.pts[:, 0] - cam[2]) / cam[0], (r.pts[:, 1] - cam[3]) / cam[1])
    rho = np.hypot(xd - x0, yd - y0)
    # (the pixel round trip of step 4 adds a rounding of its own to the stop rule's 2^-46)
    assert np.all(rho <= (uc.STOP + 8 * 2.0 ** -52) * np.maximum(1.0, np.hypot(x0, y0)))
    assert np.all(r.residual <= uc.STOP * np.maximum(1.0, np.hypot(x0, y0)))
    assert np.array_equal(r.status, rl.status) and np.array_equal(r5.status, r5l.status)
    if name == "euroc":
        assert float(r5.residual.max()) * f > 0.1, "the reason the NEWTON flag exists"


def test_checker_status_cases():
    at = {}
    for (xy, flags, want) in uc.STATUS_CASES:
        for dtype in (np.float64, np.longdouble):
            r = uc.undistort_np(uc.UNIT, [xy], flags=flags, dtype=dtype)
            assert int(r.status[0]) == want, (xy, dtype)
        r = uc.undistort_np(uc.UNIT, [xy], flags=flags)
        at[xy] = (int(r.outside_at[0]), int(r.steps[0]), r.pts[0].tolist())
    assert at[(2.0, 0.0)][0] == 1 and at[(2.0, 0.0)][2] == [2.0, 0.0]
    assert at[(0.9, 0.0)][0] == 4 and at[(0.9, 0.0)][2] == [0.9, 0.0]
    assert at[(0.71, 0.0)][1] == 20
    # NOT_CONVERGED returns the fixed-point result, which is what the call gives without the flag
    assert at[(0.71, 0.0)][2] == uc.undistort_np(uc.UNIT, [(0.71, 0.0)]).pts[0].tolist()
    assert abs(at[(0.70, 0.0)][2][0] - 1.0) <= 2.0 ** -45 and at[(0.70, 0.0)][2][1] == 0.0
    # a point that is not finite, and the all-zero camera
    r = uc.undistort_np(uc.MILD, [(np.nan, 1.0), (1.0, np.inf), (5.0, 6.0)], cov=[(1.0, 0.0, 1.0)] * 3, flags=3)
    assert r.status.tolist() == [uc.NOT_FINITE, uc.NOT_FINITE, uc.OK] and np.isnan(r.pts[:2]).all()
    assert np.array_equal(r.cov[:2], [[1.0, 0.0, 1.0]] * 2) and not np.array_equal(r.cov[2], [1.0, 0.0, 1.0])
    zero = uc.MILD.copy()
    zero[4:] = 0.0
    r = uc.undistort_np(zero, [(np.nan, 1.0), (5.0, 6.0)], cov=[(1.0, 0.5, 1.0)] * 2, flags=3)
    assert r.status.tolist() == [0, 0] and np.isnan(r.pts[0, 0]) and r.pts[1].tolist() == [5.0, 6.0]
    assert np.array_equal(r.cov, [[1.0, 0.5, 1.0]] * 2)


def test_checker_propagated_covariance_is_the_jacobian_of_the_map():
    """A by central differences of the checker's own (Newton) map, EuRoC-like camera: the analytic A S A' agrees."""
    cam = uc.EUROC
    pts, cov = uc.spread("euroc", 40, 3)
    r = uc.undistort_np(cam, pts, cov, flags=3)
    h = 1e-3
    f = lambda p: uc.undistort_np(cam, p, flags=uc.NEWTON, dtype=np.longdouble).pts.astype(np.float64)
    du = (f(pts + [h, 0.0]) - f(pts - [h, 0.0])) / (2 * h)
    dv = (f(pts + [0.0, h]) - f(pts - [0.0, h])) / (2 * h)
    for i in range(len(pts)):
        A = np.array([[du[i, 0], dv[i, 0]], [du[i, 1], dv[i, 1]]])
        S = np.array([[cov[i, 0], cov[i, 1]], [cov[i, 1], cov[i, 2]]])
        want = A @ S @ A.T
        got = np.array([[r.cov[i, 0], r.cov[i, 1]], [r.cov[i, 1], r.cov[i, 2]]])
        assert np.allclose(got, want, rtol=1e-5, atol=1e-9), i


# ---------------------------------------------------------------------------------------------- the facade, on the host
def test_facade_argument_handling_and_the_new_call_arrays_list_under_the_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ builds the host facade, so it is there"
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    san = ["-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    lib_dir = os.path.join(ROOT, "pnec_amd")
    exe = str(tmp_path / "undistort_host")
    subprocess.run([gxx, *san, "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "pnec_amd", "csrc", "host"),
                    os.path.join(ROOT, "tools", "undistort_host.cc"), os.path.join(ROOT, "pnec_amd", "csrc", "host", "pnec_host.cc"),
                    "-o", exe, "-L" + lib_dir, "-lpnec_hip", "-Wl,-rpath," + lib_dir], check=True)
    r = subprocess.run([exe], env=env, capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    assert "undistort host: every case held" in r.stdout and "FAIL" not in r.stdout
    assert sum(line.startswith("ok   ") for line in r.stdout.splitlines()) == 3
    # the list of the new entry point among CallArrays' lists
    exe = str(tmp_path / "call_arrays_host")
    subprocess.run([gxx, *san, "-I" + os.path.join(ROOT, "pnec_amd", "csrc"), os.path.join(ROOT, "tools", "call_arrays_host.cc"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], env=env, capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "FAIL" not in r.stdout
    lines = [line for line in r.stdout.splitlines() if line.startswith("ok   undistort_keypoints(")]
    assert lines and all("6 optional arrays" in line for line in lines), r.stdout[-2000:]
