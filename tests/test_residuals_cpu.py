"""Residuals and the chi-square gate without a GPU: pnec_hip_residuals is declared, bound and exported within ABI 8, its
argument checks refuse before the handle is read or a device is touched, and the pure-Python helpers (gate_sigma,
ResidualReport.variance_factor) give the numbers their definitions give."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import pnec_amd
from pnec_amd import ResidualReport, capi, gate_sigma

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_is_declared_bound_and_exported_within_abi_8():
    assert "pnec_hip_residuals" in capi.SYMBOLS
    L = capi.lib()
    assert getattr(L, "pnec_hip_residuals") is not None
    assert capi.ABI_VERSION == 8 and L.pnec_hip_abi_version() == 8
    header = open(os.path.join(ROOT, "include", "pnec_hip.h")).read()
    assert "#define PNEC_HIP_ABI_VERSION 8" in header
    assert "int pnec_hip_residuals(pnec_hip_problem *p" in header and "added within ABI 8" in header


def _call(p, q, t, n_hyp, gate, outs, space=capi.MEM_HOST):
    L = capi.lib()
    rc = L.pnec_hip_residuals(p, q, t, n_hyp, 1e-13, gate, *outs, space, None)
    return rc, (L.pnec_hip_last_error() or b"").decode()


def test_bad_arguments_are_refused_before_the_handle_is_read():
    q = np.array([0.0, 0.0, 0.0, 1.0])
    t = np.array([0.0, 0.0, 1.0])
    SENT = -7.25
    res, var, chi2, gchi2, mx = (np.full(4, SENT) for _ in range(5))
    mask = np.full(4, 9, dtype=np.uint8)
    cnt = np.full(4, -5, dtype=np.int32)
    outs = tuple(a.ctypes.data for a in (res, var, mask, chi2, gchi2, cnt, mx))
    # a stand-in handle: every check below must return before the handle is read (this box may have no device, and a
    # real problem cannot be created without one)
    fake = C.create_string_buffer(4096)
    h = C.cast(fake, C.c_void_p)
    qp, tp = q.ctypes.data, t.ctypes.data
    for args, word in (((None, qp, tp, 1, 3.0, outs), "problem"),
                       ((h, None, tp, 1, 3.0, outs), "q or t"),
                       ((h, qp, None, 1, 3.0, outs), "q or t"),
                       ((h, qp, tp, 0, 3.0, outs), "n_hyp"),
                       ((h, qp, tp, -2, 3.0, outs), "n_hyp"),
                       ((h, qp, tp, 1, -1.0, outs), "gate"),
                       ((h, qp, tp, 1, -math.inf, outs), "gate"),
                       ((h, qp, tp, 1, math.nan, outs), "gate"),
                       ((h, qp, tp, 1, 3.0, (None,) * 7), "output")):
        rc, msg = _call(*args)
        assert rc == capi.ERR_INVALID_ARGUMENT == -1, (rc, msg)
        assert word in msg, msg
    rc, msg = _call(h, qp, tp, 1, 3.0, outs, space=7)
    assert rc == -1 and "memory space" in msg
    for a in (res, var, chi2, gchi2, mx):
        assert np.all(a == SENT)
    assert np.all(mask == 9) and np.all(cnt == -5)


@pytest.mark.parametrize("c", [0.5, 0.6827, 0.9, 0.95, 0.9973, 0.999999])
def test_gate_sigma_round_trips_through_erf(c):
    g = gate_sigma(c)
    assert math.erf(g / math.sqrt(2.0)) == pytest.approx(c, rel=1e-12, abs=0.0)   # P(|N(0,1)| <= g) = erf(g / sqrt 2)


def test_gate_sigma_values_and_domain():
    assert gate_sigma(0.9973) == pytest.approx(3.0, abs=5e-3)
    assert gate_sigma(0.6826894921370859) == pytest.approx(1.0, rel=1e-12)
    for bad in (0.0, 1.0, -0.1, 1.5, math.nan):
        with pytest.raises(ValueError):
            gate_sigma(bad)


def test_variance_factor_on_hand_made_numbers():
    offsets = np.array([0, 15, 20, 23, 23, 29], dtype=np.int64)     # n = 15, 5, 3, 0, 6
    chi2 = np.array([20.0, 4.0, 1.0, 0.0, 3.0])
    z = np.zeros(0)
    rep = ResidualReport(z, z, z.astype(np.uint8), chi2, chi2, np.zeros(5, np.int32), chi2, offsets)
    vf = rep.variance_factor()
    assert vf[0] == 2.0 and vf[4] == 3.0
    assert np.isnan(vf[1]) and np.isnan(vf[2]) and np.isnan(vf[3])      # n <= 5: no redundancy
    assert np.array_equal(rep.variance_factor(dof=0)[[0, 1, 2, 4]], chi2[[0, 1, 2, 4]] / np.array([15.0, 5.0, 3.0, 6.0]))
    # hypothesis-minor slots: every hypothesis of a pair divides by that pair's n - dof
    rep2 = ResidualReport(z, z, z.astype(np.uint8), np.array([10.0, 20.0, 1.0, 2.0]), None, None, None,
                          np.array([0, 15, 20], dtype=np.int64), n_hyp=2)
    vf2 = rep2.variance_factor()
    assert vf2[0] == 1.0 and vf2[1] == 2.0 and np.isnan(vf2[2]) and np.isnan(vf2[3])


def test_python_and_facade_expose_the_new_names():
    assert {"ResidualReport", "gate_sigma"} <= set(pnec_amd.__all__)
    assert callable(pnec_amd.Batch.residuals) and callable(pnec_amd.SolveResult.residuals)
    import pnec_amd.pypnec as pypnec
    assert {"residuals", "gate_inliers"} <= set(dir(pypnec))
    facade = open(os.path.join(ROOT, "pnec_amd", "csrc", "host", "pnec_host.h")).read()
    assert "std::vector<double> Residuals(" in facade and "std::vector<int> GateInliers(" in facade
    # ... and the facade library exports both (mangled names carry them)
    with open(os.path.join(ROOT, "pnec_amd", "libpnec_host.so"), "rb") as f:
        blob = f.read()
    assert b"Residuals" in blob and b"GateInliers" in blob
