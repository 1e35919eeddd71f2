"""Triangulation and the cheirality vote without a GPU: pnec_hip_triangulate is declared, bound and exported within ABI 8,
its argument checks refuse before the handle is read or a device is touched, the Python and facade names exist, and the
numpy statement of the depth Jacobians that the GPU tests use as their yardstick agrees with central differences."""
import ctypes as C
import os

import numpy as np

import pnec_amd
from pnec_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_is_declared_bound_and_exported_within_abi_8():
    assert "pnec_hip_triangulate" in capi.SYMBOLS
    L = capi.lib()
    assert getattr(L, "pnec_hip_triangulate") is not None
    assert capi.ABI_VERSION == 8 and L.pnec_hip_abi_version() == 8
    header = open(os.path.join(ROOT, "include", "pnec_hip.h")).read()
    assert "#define PNEC_HIP_ABI_VERSION 8" in header
    assert "int pnec_hip_triangulate(pnec_hip_problem *p" in header
    assert "#define PNEC_HIP_TRI_ORIENT 1" in header and capi.TRI_ORIENT == 1


def _call(p, q, t, n_hyp, flags, outs, space=capi.MEM_HOST):
    L = capi.lib()
    rc = L.pnec_hip_triangulate(p, q, t, n_hyp, flags, *outs, space, None)
    return rc, (L.pnec_hip_last_error() or b"").decode()


def test_bad_arguments_are_refused_before_the_handle_is_read():
    q = np.array([0.0, 0.0, 0.0, 1.0])
    t = np.array([0.0, 0.0, 1.0])
    SENT = -7.25
    point = np.full(12, SENT)
    d1, d2, psi, var, mean = (np.full(4, SENT) for _ in range(5))
    to = np.full(12, SENT)
    front = np.full(4, 9, dtype=np.uint8)
    nf, nb, sign = (np.full(4, -5, dtype=np.int32) for _ in range(3))
    outs = tuple(a.ctypes.data for a in (point, d1, d2, psi, var, front, nf, nb, sign, to, mean))
    # a stand-in handle: every check below must return before the handle is read (this box may have no device, and a
    # real problem cannot be created without one)
    fake = C.create_string_buffer(4096)
    h = C.cast(fake, C.c_void_p)
    qp, tp = q.ctypes.data, t.ctypes.data
    for args, word in (((None, qp, tp, 1, 0, outs), "problem"),
                       ((h, None, tp, 1, 0, outs), "q or t"),
                       ((h, qp, None, 1, 0, outs), "q or t"),
                       ((h, qp, tp, 0, 0, outs), "n_hyp"),
                       ((h, qp, tp, -2, 1, outs), "n_hyp"),
                       ((h, qp, tp, 1, 2, outs), "flags"),
                       ((h, qp, tp, 1, 3, outs), "flags"),
                       ((h, qp, tp, 1, -1, outs), "flags"),
                       ((h, qp, tp, 1, 1, (None,) * 11), "output")):
        rc, msg = _call(*args)
        assert rc == capi.ERR_INVALID_ARGUMENT == -1, (rc, msg)
        assert word in msg, msg
    for space in (7, -1):
        rc, msg = _call(h, qp, tp, 1, 1, outs, space=space)
        assert rc == -1 and "memory space" in msg
    for a in (point, d1, d2, psi, var, to, mean):
        assert np.all(a == SENT)
    assert np.all(front == 9) and all(np.all(a == -5) for a in (nf, nb, sign))


def test_python_and_facade_expose_the_new_names():
    assert "Triangulation" in pnec_amd.__all__ and pnec_amd.Triangulation is not None
    assert callable(pnec_amd.Batch.triangulate) and callable(pnec_amd.SolveResult.triangulate)
    import dataclasses
    assert [f.name for f in dataclasses.fields(pnec_amd.Triangulation)][:11] == [
        "point", "depth1", "depth2", "parallax", "depth1_var", "front", "n_front", "n_back", "sign", "t", "parallax_mean"]
    import pnec_amd.pypnec as pypnec
    assert {"triangulate", "orient_translation"} <= set(dir(pypnec))
    facade = open(os.path.join(ROOT, "pnec_amd", "csrc", "host", "pnec_host.h")).read()
    assert "std::vector<Vector3d> Triangulate(" in facade and "SE3d OrientTranslation(" in facade
    with open(os.path.join(ROOT, "pnec_amd", "libpnec_host.so"), "rb") as f:
        blob = f.read()
    assert b"Triangulate" in blob and b"OrientTranslation" in blob


# ---- the yardstick of the GPU variance tests: depth1 and its Jacobians in numpy --------------------------------------
def depth1_np(f1, u, t):
    a00, a10, a11 = f1 @ f1, f1 @ u, u @ u
    b0, b1 = f1 @ t, u @ t
    return (a11 * b0 - a10 * b1) / (a00 * a11 - a10 * a10)


def depth1_jacobians_np(f1, u, t):
    """(gu, g1) = (d depth1 / d u, d depth1 / d f1) as include/pnec_hip.h states them."""
    a00, a10, a11 = f1 @ f1, f1 @ u, u @ u
    b0, b1 = f1 @ t, u @ t
    D = a00 * a11 - a10 * a10
    d1 = (a11 * b0 - a10 * b1) / D
    gu = (2 * b0 * u - b1 * f1 - a10 * t - d1 * (2 * a00 * u - 2 * a10 * f1)) / D
    g1 = (a11 * t - b1 * u - d1 * (2 * a11 * f1 - 2 * a10 * u)) / D
    return gu, g1


def test_numpy_depth_jacobians_agree_with_central_differences():
    rng = np.random.default_rng(20)
    h, done, worst = 1e-6, 0, 0.0
    while done < 200:
        f1, u = rng.normal(size=3), rng.normal(size=3)
        f1 /= np.linalg.norm(f1)
        u /= np.linalg.norm(u)
        # (bearings not assumed unit: a length of 0.7 .. 1.3 each)
        f1 *= rng.uniform(0.7, 1.3)
        u *= rng.uniform(0.7, 1.3)
        psi = np.arctan2(np.linalg.norm(np.cross(f1, u)), f1 @ u)
        if psi < 0.05:
            continue
        t = rng.normal(size=3)
        t /= np.linalg.norm(t)
        gu, g1 = depth1_jacobians_np(f1, u, t)
        nu, n1 = np.zeros(3), np.zeros(3)
        for k in range(3):
            e = np.zeros(3)
            e[k] = h
            nu[k] = (depth1_np(f1, u + e, t) - depth1_np(f1, u - e, t)) / (2 * h)
            n1[k] = (depth1_np(f1 + e, u, t) - depth1_np(f1 - e, u, t)) / (2 * h)
        for g, n in ((gu, nu), (g1, n1)):
            rel = np.linalg.norm(g - n) / np.linalg.norm(g)
            worst = max(worst, rel)
            assert rel <= 1e-6, (rel, psi)
        done += 1
    print("worst relative difference", worst)
