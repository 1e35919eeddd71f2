"""Relative scale between consecutive pairs without a GPU: pnec_hip_relative_scale is declared, bound and exported within
ABI 8, its argument checks refuse before a handle is read or a device is touched, the Python, facade and pybind names
exist, the numpy join on track ids and the chaining of scales do what they say, and the numpy yardstick of the GPU tests
(`relative_scale_np`) returns the true baseline ratio on exact three-view geometry.

The last test compiles the kernel's own per-link function (relative_scale_link with tri_depths, built for the host from
tools/relative_scale_link_host.hip) and runs it on the GPU tests' batch.  The GPU tests allow each ratio the propagated
depth bound of tests/test_triangulate_gpu.py, one per depth: relative 1e-13 * (1 / sin^2 psi_prev + 1 / sin^2 psi_cur).
Measured here with the host build: worst relative error * (1 / sin^2 psi_prev + 1 / sin^2 psi_cur)^-1 = 3.2e-16, 310x
inside that bound (at least 10x is asked for); numpy's own statement reaches 4.2e-16.
"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import pnec_amd
from pnec_amd import capi
from pnec_amd import tracks as trk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- the data and the yardstick the GPU tests share ------------------------------------------------------------------
CUR_SIZES = [1, 4, 63, 64, 65, 512, 513, 1100, 4200]
PREV_SIZES = [3, 9, 50, 100, 64, 700, 400, 1500, 3900]
MIN_PARALLAX = 0.02
SEED = 2027
REL_TOL = 1e-13          # per depth, over sin^2 psi: the bound of tests/test_triangulate_gpu.py


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _quat_to_R(q):
    x, y, z, w = np.asarray(q, float) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def triangulate_np(f1, f2, q, t):
    """include/pnec_hip.h's midpoint system in numpy (as tests/test_triangulate_gpu.py::triangulate_np)"""
    R, tn = _quat_to_R(q), np.asarray(t, float) / np.linalg.norm(t)
    u = f2 @ R.T
    a00, a10, a11 = (f1 * f1).sum(1), (f1 * u).sum(1), (u * u).sum(1)
    b0, b1 = f1 @ tn, u @ tn
    D = a00 * a11 - a10 * a10
    with np.errstate(all="ignore"):
        d1, d2 = (a11 * b0 - a10 * b1) / D, (a10 * b0 - a00 * b1) / D
        ok = (D > 2.0 ** -49 * (a00 * a11)) & np.isfinite(D)
        front = ok & np.isfinite(d1) & np.isfinite(d2) & (d1 > 0) & (d2 > 0)
        sin2 = D / (a00 * a11)
    return dict(depth1=d1, depth2=d2, D=D, a00=a00, a10=a10, a11=a11, front=front, sin2=sin2)


def ranks_np(x):
    """the elements of rank (m-1)//4, (m-1)//2, 3(m-1)//4 of x in ascending order; NaN for an empty x"""
    x = np.sort(np.asarray(x, dtype=np.float64))
    m = len(x)
    return x[[(m - 1) // 4, (m - 1) // 2, (3 * (m - 1)) // 4]] if m else np.full(3, np.nan)


def relative_scale_np(f1c, f2c, qc, tc, f1p, f2p, qp, tp, link, min_parallax=0.0):
    """pnec_hip_relative_scale for ONE pair in numpy: triangulation of both sides, the ratio, the gates, the ranks by
    np.sort.  (f1p, f2p) is the whole previous pair, `link` indexes it."""
    link = np.asarray(link)
    n_prev = len(f1p)
    linked = (link >= 0) & (link < n_prev)
    j = np.where(linked, link, 0)
    g1 = f1p[j] if n_prev else np.zeros((len(link), 3))
    g2 = f2p[j] if n_prev else np.zeros((len(link), 3))
    c, r = triangulate_np(f1c, f2c, qc, tc), triangulate_np(g1, g2, qp, tp)
    s2 = np.sin(min_parallax) ** 2 if min_parallax < np.pi / 2 else 2.0
    with np.errstate(all="ignore"):
        ratio = (r["depth2"] * np.sqrt(r["a11"])) / (c["depth1"] * np.sqrt(c["a00"]))
        gate = lambda s: (s["D"] >= s2 * (s["a00"] * s["a11"])) & ((s["a10"] > 0) if min_parallax > 0 else True)
        used = linked & c["front"] & r["front"] & gate(c) & gate(r) & (ratio > 0) & np.isfinite(ratio)
    ratio = np.where(used, ratio, np.nan)
    return dict(ratio=ratio, used=used.astype(np.uint8), n_linked=int(linked.sum()), n_used=int(used.sum()),
                scale=ranks_np(ratio[used]), linked=linked, sin2_cur=c["sin2"], sin2_prev=r["sin2"])


def gate_margin(ref, min_parallax):
    """the smallest relative distance of a linked correspondence's sin^2 psi (either side) from the gate"""
    s2 = np.sin(min_parallax) ** 2
    both = np.concatenate([ref["sin2_cur"][ref["linked"]], ref["sin2_prev"][ref["linked"]]])
    both = both[np.isfinite(both)]
    return float(np.min(np.abs(both - s2) / s2)) if len(both) else np.inf


def link_tolerance(ref):
    """relative tolerance of each ratio: REL_TOL per depth, each over its own sin^2 psi"""
    with np.errstate(all="ignore"):
        return REL_TOL * (1.0 / ref["sin2_prev"] + 1.0 / ref["sin2_cur"])


class ThreeView:
    """One current pair (B, C) and its previous pair (A, B) of exact geometry; `truth` = |BC| / |AB|."""

    def __init__(self, rng, n_cur, n_prev, link_frac=0.7, wrong_frac=0.0, max_angle=0.3):
        def pose():
            axis, ang = _unit(rng.standard_normal(3)), rng.uniform(0.0, max_angle)
            return np.concatenate([axis * np.sin(ang / 2), [np.cos(ang / 2)]]), _unit(rng.standard_normal(3)), rng.uniform(0.3, 1.5)
        self.qp, self.tp, self.sp = pose()     # x_A = Rp x_B + sp tp : camera B sits at sp tp in frame A
        self.qc, self.tc, self.sc = pose()     # x_B = Rc x_C + sc tc : camera C sits at sc tc in frame B
        Rp, Rc = _quat_to_R(self.qp), _quat_to_R(self.qc)
        self.truth = self.sc / self.sp

        def points(k):   # in frame B, in front of all three cameras
            P = np.zeros((0, 3))
            while len(P) < k:
                m = 4 * k + 64
                X = np.column_stack([rng.uniform(-2, 2, m), rng.uniform(-2, 2, m), rng.uniform(2, 8, m)])
                xa, xc = X @ Rp.T + self.sp * self.tp, (X - self.sc * self.tc) @ Rc
                P = np.concatenate([P, X[(xa[:, 2] > 0.5) & (xc[:, 2] > 0.5)]])
            return P[:k]
        Pc, Pp = points(n_cur), points(n_prev)
        n_link = min(int(round(link_frac * n_cur)), n_prev)
        rows_c, rows_p = rng.permutation(n_cur)[:n_link], rng.permutation(n_prev)[:n_link]
        link = np.full(n_cur, -1, dtype=np.int32)
        link[rows_c] = rows_p
        Pp[rows_p] = Pc[rows_c]
        free = np.flatnonzero(link < 0)
        if len(free) >= 3:                     # a few out of range
            link[free[:3]] = [n_prev, n_prev + 7, -5]
        self.wrong = np.zeros(n_cur, dtype=bool)
        if wrong_frac > 0 and n_prev > 1:      # re-point a share of the links at other tracks
            bad = rows_c[:int(round(wrong_frac * n_link))]
            link[bad] = (link[bad] + 1 + rng.integers(0, n_prev - 1, len(bad))) % n_prev
            self.wrong[bad] = True
        self.link = link
        self.f1c, self.f2c = _unit(Pc), _unit((Pc - self.sc * self.tc) @ Rc)
        self.f1p, self.f2p = _unit(Pp @ Rp.T + self.sp * self.tp), _unit(Pp)
        self.n_cur, self.n_prev = n_cur, n_prev

    def ref(self, min_parallax=MIN_PARALLAX, tp=None):
        return relative_scale_np(self.f1c, self.f2c, self.qc, self.tc, self.f1p, self.f2p, self.qp,
                                 self.tp if tp is None else tp, self.link, min_parallax)


def ragged_cases(wrong_frac=0.0, seed=SEED):
    """the GPU tests' ragged batch: one ThreeView per size class"""
    rng = np.random.default_rng(seed)
    return [ThreeView(rng, n, m, wrong_frac=wrong_frac) for n, m in zip(CUR_SIZES, PREV_SIZES)]


# ---- the ABI ---------------------------------------------------------------------------------------------------------
def test_symbol_is_declared_bound_and_exported_within_abi_8():
    assert "pnec_hip_relative_scale" in capi.SYMBOLS
    L = capi.lib()
    assert getattr(L, "pnec_hip_relative_scale") is not None
    assert capi.ABI_VERSION == 8 and L.pnec_hip_abi_version() == 8
    header = open(os.path.join(ROOT, "include", "pnec_hip.h")).read()
    assert "#define PNEC_HIP_ABI_VERSION 8" in header
    assert "int pnec_hip_relative_scale(pnec_hip_problem *cur, pnec_hip_problem *prev, const int64_t *prev_pair" in header
    for words in ("ratio = (r.depth2 * sqrt(r.a11)) / (c.depth1 * sqrt(c.a00))", "additionally requires a10 > 0",
                  "(m-1)/4, (m-1)/2 and 3(m-1)/4", "never an interpolation"):
        assert words in header, words


def _call(cur, prev, pp, link, qc, tc, qp, tp, mp, outs, space=capi.MEM_HOST):
    L = capi.lib()
    rc = L.pnec_hip_relative_scale(cur, prev, pp, link, qc, tc, qp, tp, mp, *outs, space, None)
    return rc, (L.pnec_hip_last_error() or b"").decode()


def test_bad_arguments_are_refused_before_a_handle_is_read():
    q = np.array([0.0, 0.0, 0.0, 1.0])
    t = np.array([0.0, 0.0, 1.0])
    pp = np.zeros(1, dtype=np.int64)
    link = np.zeros(4, dtype=np.int32)
    SENT = -7.25
    ratio, scale = np.full(4, SENT), np.full(3, SENT)
    used = np.full(4, 9, dtype=np.uint8)
    nl, nu = (np.full(1, -5, dtype=np.int32) for _ in range(2))
    outs = tuple(a.ctypes.data for a in (ratio, used, scale, nl, nu))
    # stand-in handles: every check below must return before a handle is read (this box may have no device, and a real
    # problem cannot be created without one)
    fake1, fake2 = C.create_string_buffer(4096), C.create_string_buffer(4096)
    h, g = C.cast(fake1, C.c_void_p), C.cast(fake2, C.c_void_p)
    P, K, Q, T = pp.ctypes.data, link.ctypes.data, q.ctypes.data, t.ctypes.data
    for args, word in (((None, g, P, K, Q, T, Q, T, 0.0, outs), "cur or prev"),
                       ((h, None, P, K, Q, T, Q, T, 0.0, outs), "cur or prev"),
                       ((h, g, None, K, Q, T, Q, T, 0.0, outs), "prev_pair or link"),
                       ((h, g, P, None, Q, T, Q, T, 0.0, outs), "prev_pair or link"),
                       ((h, g, P, K, None, T, Q, T, 0.0, outs), "pose pointer"),
                       ((h, g, P, K, Q, None, Q, T, 0.0, outs), "pose pointer"),
                       ((h, g, P, K, Q, T, None, T, 0.0, outs), "pose pointer"),
                       ((h, g, P, K, Q, T, Q, None, 0.0, outs), "pose pointer"),
                       ((h, g, P, K, Q, T, Q, T, -0.01, outs), "min_parallax"),
                       ((h, g, P, K, Q, T, Q, T, float("nan"), outs), "min_parallax"),
                       ((h, g, P, K, Q, T, Q, T, float("inf"), outs), "min_parallax"),
                       ((h, h, P, K, Q, T, Q, T, 0.02, (None,) * 5), "output")):
        rc, msg = _call(*args)
        assert rc == capi.ERR_INVALID_ARGUMENT == -1, (rc, msg)
        assert "relative_scale" in msg and word in msg, msg
    for space in (7, -1):
        rc, msg = _call(h, g, P, K, Q, T, Q, T, 0.02, outs, space=space)
        assert rc == -1 and "memory space" in msg
    assert np.all(ratio == SENT) and np.all(scale == SENT) and np.all(used == 9) and nl[0] == -5 and nu[0] == -5
    assert fake1.raw == bytes(4096) and fake2.raw == bytes(4096)


def test_python_facade_and_pybind_expose_the_new_names():
    import dataclasses
    assert {"RelativeScale", "chain_scales"} <= set(pnec_amd.__all__)
    assert callable(pnec_amd.Batch.relative_scale) and callable(pnec_amd.chain_scales)
    assert [f.name for f in dataclasses.fields(pnec_amd.RelativeScale)][:7] == [
        "scale", "q25", "q75", "n_linked", "n_used", "ratio", "used"]
    rs = pnec_amd.RelativeScale(np.array([2.0]), np.array([1.0]), np.array([np.e]), None, None)
    assert abs(rs.log_sigma()[0] - 1.0 / 1.349) <= 1e-15
    assert callable(trk.link_pairs) and callable(trk.Tracks.links) and trk.chain_scales is pnec_amd.chain_scales
    import pnec_amd.pypnec as pypnec
    assert "relative_scale" in dir(pypnec)
    facade = open(os.path.join(ROOT, "pnec_amd", "csrc", "host", "pnec_host.h")).read()
    assert "double RelativeScale(" in facade
    with open(os.path.join(ROOT, "pnec_amd", "libpnec_host.so"), "rb") as f:
        assert b"RelativeScale" in f.read()


# ---- links and chains ------------------------------------------------------------------------------------------------
def test_link_pairs_joins_on_track_ids_first_row_wins():
    prev = np.array([10, 11, 12, 11, 40], dtype=np.int64)          # id 11 twice: the FIRST row (1) wins
    cur = np.array([12, 99, 11, 10, 11, 40, -3], dtype=np.int64)   # 99 and -3 are absent; 11 twice links both rows
    link = trk.link_pairs(prev, cur)
    assert link.dtype == np.int32 and link.tolist() == [2, -1, 1, 0, 1, 4, -1]
    assert trk.link_pairs(np.zeros(0, dtype=np.int64), cur).tolist() == [-1] * 7
    assert trk.link_pairs(prev, np.zeros(0, dtype=np.int64)).shape == (0,)


def _tracks(ids1, ids2, offsets, sequence):
    M, P = int(offsets[-1]), len(offsets) - 1
    z = np.zeros
    return trk.Tracks(np.asarray(offsets, dtype=np.int64), z((M, 3)), z((M, 3)), z((M, 3, 3)), z((P, 4)), z((P, 3)),
                      sequence=sequence, ids1=ids1, ids2=ids2)


def test_tracks_links_follow_sequences_and_ids():
    # four pairs, two sequences of two; a track id sits in the same row of ids1 and ids2 (the format's rule)
    ids = np.array([1, 2, 3,   3, 7, 1, 8,   5, 6,   6, 9, 5], dtype=np.int64)
    off = [0, 3, 7, 9, 12]
    prev_pair, link = _tracks(ids, ids.copy(), off, np.array([0, 0, 4, 4], dtype=np.int32)).links()
    assert prev_pair.dtype == np.int64 and prev_pair.tolist() == [-1, 0, -1, 2]       # -1 at each sequence's start
    assert link.dtype == np.int32 and link.tolist() == [-1, -1, -1,   2, -1, 0, -1,   -1, -1,   1, -1, 0]
    # without `sequence` the file is one sequence: pair 2 now follows pair 1 (and shares no track with it)
    prev_pair, link = _tracks(ids, ids.copy(), off, None).links()
    assert prev_pair.tolist() == [-1, 0, 1, 2] and link[7:9].tolist() == [-1, -1]
    # without ids nothing is linked
    prev_pair, link = _tracks(None, None, off, None).links()
    assert prev_pair.tolist() == [-1] * 4 and link.tolist() == [-1] * 12


def test_chain_scales_is_a_cumulative_product_and_nan_goes_forward():
    scale = np.array([np.nan, 2.0, 0.5, 3.0,   7.0, 4.0, np.nan, 2.0, 5.0])
    prev_pair = np.array([-1, 0, 1, 2,   -1, 4, 5, 6, -1])
    got = pnec_amd.chain_scales(scale, prev_pair)
    # (the scale of a chain's first pair is not used: it has no previous pair)
    assert np.array_equal(got[:6], [1.0, 2.0, 1.0, 3.0, 1.0, 4.0])
    assert np.isnan(got[6]) and np.isnan(got[7]) and got[8] == 1.0
    with pytest.raises(ValueError):
        pnec_amd.chain_scales(np.ones(2), np.array([1, -1]))


# ---- the yardstick -----------------------------------------------------------------------------------------------------
def test_numpy_yardstick_gives_the_true_ratio_on_exact_geometry():
    worst = 0.0
    for case in ragged_cases():
        ref = case.ref()
        assert gate_margin(ref, MIN_PARALLAX) > 1e-9
        in_range = (case.link >= 0) & (case.link < case.n_prev)
        assert ref["n_linked"] == in_range.sum() and 0.6 * case.n_cur <= ref["n_linked"] <= 0.75 * case.n_cur + 1
        assert ref["n_used"] >= 0.5 * ref["n_linked"] and np.all(ref["used"][~in_range] == 0)
        u = ref["used"] == 1
        assert np.all(np.isnan(ref["ratio"][~u]))
        if ref["n_used"] == 0:
            assert np.all(np.isnan(ref["scale"]))
            continue
        err = np.abs(ref["ratio"][u] - case.truth) / case.truth
        assert np.all(err <= link_tolerance(ref)[u])
        worst = max(worst, float(np.max(err / link_tolerance(ref)[u])) * REL_TOL)
        x = np.sort(ref["ratio"][u])
        assert ref["scale"][0] <= ref["scale"][1] <= ref["scale"][2] and ref["scale"][1] == x[(len(x) - 1) // 2]
    assert len({round(c.truth, 6) for c in ragged_cases()}) == len(CUR_SIZES)      # the truth differs from pair to pair
    print("numpy: worst relative error / (1/sin^2 psi_prev + 1/sin^2 psi_cur) =", worst)


def test_ranks_are_elements_of_the_set():
    assert ranks_np([5.0]).tolist() == [5.0, 5.0, 5.0]
    assert ranks_np([4.0, 1.0]).tolist() == [1.0, 1.0, 1.0]
    assert ranks_np([3.0, 1.0, 2.0, 5.0, 4.0]).tolist() == [2.0, 3.0, 4.0]
    assert ranks_np(np.arange(8.0)[::-1]).tolist() == [1.0, 3.0, 5.0]
    assert np.all(np.isnan(ranks_np([])))


def test_the_kernels_per_link_function_built_for_the_host_stays_10x_inside_the_gpu_tolerance(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    lib = str(tmp_path / "librs_link_host.so")
    subprocess.run([hipcc, "--offload-host-only", "-O2", "-std=c++17", "-fPIC", "-shared", "-mfma",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "pnec_amd", "csrc"),
                    os.path.join(ROOT, "tools", "relative_scale_link_host.hip"), "-o", lib], check=True)
    fn = C.CDLL(lib).rs_link_host
    vp = C.c_void_p
    fn.argtypes = [C.c_int64, vp, vp, vp, vp, vp, vp, C.c_double, C.c_int, vp, vp]
    fn.restype = None
    worst, total = 0.0, 0
    for case in ragged_cases():
        ref = case.ref()
        lk = ref["linked"]
        j = np.where(lk, case.link, 0)
        fc = np.ascontiguousarray(np.hstack([case.f1c, case.f2c]))
        fp = np.ascontiguousarray(np.where(lk[:, None], np.hstack([case.f1p[j], case.f2p[j]]), 0.0))
        ratio, used = np.empty(case.n_cur), np.empty(case.n_cur, dtype=np.uint8)
        fn(case.n_cur, fc.ctypes.data, case.qc.ctypes.data, case.tc.ctypes.data, fp.ctypes.data, case.qp.ctypes.data,
           case.tp.ctypes.data, np.sin(MIN_PARALLAX) ** 2, 1, ratio.ctypes.data, used.ctypes.data)
        assert np.array_equal(used, ref["used"])           # (an unlinked row is all zeros on the previous side: not used)
        u = used == 1
        assert np.all(np.isnan(ratio[~u]))
        if u.any():
            scaled = np.abs(ratio[u] - case.truth) / case.truth / (1.0 / ref["sin2_prev"][u] + 1.0 / ref["sin2_cur"][u])
            worst = max(worst, float(scaled.max()))
            total += int(u.sum())
    print("host build of relative_scale_link: worst relative error / (1/sin^2 psi_prev + 1/sin^2 psi_cur) =", worst,
          "over", total, "links")
    assert total > 3000 and worst <= REL_TOL / 10
