"""Pose covariance without a GPU: the argument checks of pnec_hip_pose_covariance (refused before any device is
touched), the ABI version, and the pure-Python helpers -- the 15 -> 5x5 expansion and the documented conversion between
the 6x6 covariance and the Ceres tangent space, on the oracle's numbers."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from pnec_amd import capi
from pnec_amd import simulation as sim
from pnec_amd.batch import ceres_chart_to_cov6, chart_basis, cov6_to_ceres_chart, expand_info


def test_abi_version_and_symbol():
    assert capi.ABI_VERSION == 8
    assert capi.lib().pnec_hip_abi_version() == 8
    assert "pnec_hip_pose_covariance" in capi.SYMBOLS
    assert (capi.COV_OK, capi.COV_SINGULAR, capi.COV_NONFINITE) == (0, 1, 2)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pnec_hip.h")).read()
    assert "#define PNEC_HIP_ABI_VERSION 8" in header and "pnec_hip_pose_covariance" in header


def _call(p, q, t, n_hyp, outs, space=capi.MEM_HOST):
    L = capi.lib()
    rc = L.pnec_hip_pose_covariance(p, q, t, n_hyp, 1e-13, *outs, space, None)
    return rc, (L.pnec_hip_last_error() or b"").decode()


def test_bad_arguments_are_refused_before_any_device_is_touched():
    q = np.array([0.0, 0.0, 0.0, 1.0])
    t = np.array([0.0, 0.0, 1.0])
    cov = np.zeros(36)
    outs = (None, cov.ctypes.data, None, None, None)
    # a stand-in handle: every check below must return before the handle is read (this box may have no device, and a
    # real problem cannot be created without one)
    fake = C.create_string_buffer(4096)
    h = C.cast(fake, C.c_void_p)
    for args, word in (((None, q.ctypes.data, t.ctypes.data, 1, outs), "problem"),
                       ((h, None, t.ctypes.data, 1, outs), "q or t"),
                       ((h, q.ctypes.data, None, 1, outs), "q or t"),
                       ((h, q.ctypes.data, t.ctypes.data, 0, outs), "n_hyp"),
                       ((h, q.ctypes.data, t.ctypes.data, -3, outs), "n_hyp"),
                       ((h, q.ctypes.data, t.ctypes.data, 1, (None,) * 5), "output")):
        rc, msg = _call(*args)
        assert rc == capi.ERR_INVALID_ARGUMENT == -1, (rc, msg)
        assert word in msg, msg
    rc, msg = _call(h, q.ctypes.data, t.ctypes.data, 1, outs, space=7)
    assert rc == -1 and "memory space" in msg
    assert np.all(cov == 0.0)


def test_expand_info_follows_the_packed_order():
    packed = np.arange(15.0) + 1.0
    full = expand_info(packed)
    assert full.shape == (5, 5) and np.array_equal(full, full.T)
    k = 0
    for a in range(5):
        for b in range(a, 5):
            assert full[a, b] == packed[k]
            k += 1
    batch = expand_info(np.stack([packed, 2 * packed]))
    assert batch.shape == (2, 5, 5) and np.array_equal(batch[1], 2 * full)


@pytest.mark.parametrize("theta,phi", [(1.3, 0.4), (0.015, -2.0), (1.6e-3, 2.5)])
def test_cov6_and_ceres_chart_round_trip_on_the_oracles_information(oracle, theta, phi):
    """Sigma_6 built from the oracle's Ceres-chart J'J maps back onto (J'J)^-1 and forth again; t is its null vector."""
    g = sim.generate(1, 200, seed=21)
    f1, f2, c2 = g.bvs1[0].numpy(), g.bvs2[0].numpy(), g.covs2[0].numpy()
    _, J, _ = oracle.evaluate(oracle.MODE_TARGET, oracle.JAC_ANALYTIC, f1, f2, c2, None, 1e-13, theta, phi, g.init_q[0].numpy())
    t = np.array([math.sin(theta) * math.cos(phi), math.sin(theta) * math.sin(phi), math.cos(theta)])
    bth, eph, st = chart_basis(t)
    assert st == pytest.approx(math.sin(theta), rel=1e-12)
    assert abs(bth @ t) < 1e-15 and abs(eph @ t) < 1e-15 and abs(bth @ eph) < 1e-15
    # invert in the orthonormal chart (the Ceres chart's own matrix is ill-conditioned near theta = 0)
    D = np.array([1.0, st, 2.0, 2.0, 2.0])
    Hx = (J / D).T @ (J / D)
    d = 1.0 / np.sqrt(np.diag(Hx))
    cov5 = (np.linalg.inv(Hx * np.outer(d, d)) * np.outer(d, d)) / np.outer(D, D)     # covariance of (theta, phi, delta)
    cov6 = ceres_chart_to_cov6(cov5, t)
    assert np.abs(cov6 @ np.concatenate([np.zeros(3), t])).max() <= 1e-12 * np.abs(cov6).max()
    back = cov6_to_ceres_chart(cov6, t)
    s = np.sqrt(np.outer(np.diag(cov5), np.diag(cov5)))
    assert (np.abs(back - cov5) / s).max() <= 1e-10
    # ... and it is the inverse of the oracle's information
    H = J.T @ J
    hs = np.sqrt(np.diag(H))
    resid = (back * np.outer(hs, hs)) @ (H / np.outer(hs, hs)) - np.eye(5)
    assert np.abs(resid).max() <= 1e-10 * np.linalg.cond(H / np.outer(hs, hs))


def test_chart_basis_at_the_poles():
    for t, bth in (((0.0, 0.0, 1.0), (1.0, 0.0, 0.0)), ((0.0, 0.0, -1.0), (-1.0, 0.0, 0.0)), ((0.0, 0.0, 0.0), (1.0, 0.0, 0.0))):
        b, e, st = chart_basis(t)
        assert np.allclose(b, bth, atol=0) and np.array_equal(e, [0.0, 1.0, 0.0]) and st == 0.0
