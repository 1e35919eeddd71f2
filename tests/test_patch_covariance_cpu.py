"""Patch covariances without a GPU.

`patch_cov_np` below is the plain-numpy statement of the definition in include/pnec_hip.h (pnec_hip_patch_covariance):
the yardstick of tests/test_patch_covariance_gpu.py, tested here on its own -- exactness of the interpolant on affine
images, invariance under a power-of-two intensity scale, the statuses of constant and ramp images -- together with
Pattern52, the new symbol's declaration, binding and export (which fails on the parent commit), the argument checks (which
return before any device is touched) and the Python / facade / pybind names.

The last test builds the kernel's own arithmetic for the host (tools/patch_cov_host.cc: the functions of
pnec_amd/csrc/pnec_patch_cov.hpp, summed in the kernel's order) with the address and undefined-behaviour sanitizers, as a
stand-alone program, and runs it on every position of the GPU tests' edge case on an image that is read into a heap block
without a byte of slack: an index error shows there, not on a device.  Its output is compared with `patch_cov_np` under
the GPU tests' own bounds.
"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import pnec_amd
from pnec_amd import capi, patches

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-10     # the project's bar for sums of products (tests/test_pose_covariance_gpu.py); covariance: 2 kappa TOL


# ---- the yardstick ---------------------------------------------------------------------------------------------------
def interp_grad_np(img, px, py):
    """value, d/dx, d/dy of the bilinear interpolant of `img` [h,w] (float64) at valid points (px, py) [..]"""
    ix, iy = np.floor(px).astype(np.int64), np.floor(py).astype(np.int64)
    dx, dy = px - ix, py - iy
    ddx, ddy = 1.0 - dx, 1.0 - dy

    def B(u, v):
        return ((ddx * ddy * img[v, u] + ddx * dy * img[v + 1, u]) + dx * ddy * img[v, u + 1]) + dx * dy * img[v + 1, u + 1]
    return B(ix, iy), 0.5 * (B(ix + 1, iy) - B(ix - 1, iy)), 0.5 * (B(ix, iy + 1) - B(ix, iy - 1))


def patch_cov_np(images, pts, offsets=None, pattern=patches.PATTERN52, scaling=10.0, angle=None):
    """include/pnec_hip.h's definition in numpy: images [F,h,w] or [h,w] of any dtype (taken as float64 values),
    pts [M,2], offsets [F+1].  Sums run over the pattern in its own order.  Returns a dict: cov [M,3] (xx, xy, yy),
    hessian [M,6] (H * scaling, upper triangle), mean [M], n_valid [M], status [M] and kappa [M] (the condition number
    of the Jacobi-scaled H; inf where it does not exist)."""
    images = np.asarray(images)
    if images.ndim == 2:
        images = images[None]
    F, h, w = images.shape
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 2)
    M = pts.shape[0]
    offsets = np.array([0, M]) if offsets is None else np.asarray(offsets)
    pattern = np.asarray(pattern, dtype=np.float64)
    out = dict(cov=np.full((M, 3), np.nan), hessian=np.zeros((M, 6)), mean=np.zeros(M), n_valid=np.zeros(M, np.int32),
               status=np.zeros(M, np.int32), kappa=np.full(M, np.inf))
    for f in range(F):
        img = images[f].astype(np.float64)
        for k in range(int(offsets[f]), int(offsets[f + 1])):
            p = pts[k] + pattern
            with np.errstate(invalid="ignore"):
                valid = (p[:, 0] >= 2) & (p[:, 0] < w - 3) & (p[:, 1] >= 2) & (p[:, 1] < h - 3)
            n = int(valid.sum())
            d, gx, gy = (np.zeros(len(pattern)) for _ in range(3))
            if n:
                d[valid], gx[valid], gy[valid] = interp_grad_np(img, p[valid, 0], p[valid, 1])
            S = Gx = Gy = 0.0
            for i in range(len(pattern)):
                S, Gx, Gy = S + d[i], Gx + gx[i], Gy + gy[i]
            H = np.zeros((3, 3))
            with np.errstate(all="ignore"):
                for i in range(len(pattern)):
                    if not valid[i]:
                        continue
                    gpx = n * (gx[i] * S - Gx * d[i]) / (S * S)
                    gpy = n * (gy[i] * S - Gy * d[i]) / (S * S)
                    J = np.array([gpx, gpy, -pattern[i, 1] * gpx + pattern[i, 0] * gpy])
                    H += np.outer(J, J)
                out["mean"][k] = np.float64(S) / np.float64(n) if n else np.nan
            out["n_valid"][k] = n
            out["hessian"][k] = (H * scaling)[np.triu_indices(3)]
            if n == 0 or not (S > 0 and np.isfinite(S)):
                out["status"][k] = patches.PATCH_EMPTY
                continue
            # Jacobi scaling, then Cholesky: a pivot that is not positive means singular (fewer than three points
            # leave H with rank below three whatever the rounding says)
            with np.errstate(all="ignore"):
                sc = 1.0 / np.sqrt(np.diag(H))
                A = H * np.outer(sc, sc)
            ok = n >= 3 and bool(np.all(np.isfinite(A)))
            if ok:
                try:
                    np.linalg.cholesky(A)
                except np.linalg.LinAlgError:
                    ok = False
            if ok:
                Ainv = np.linalg.inv(A)
                Sigma = (Ainv * np.outer(sc, sc))[:2, :2] / scaling
                ok = bool(np.all(np.isfinite(Sigma)))
            if not ok:
                out["status"][k] = patches.PATCH_SINGULAR
                continue
            out["kappa"][k] = np.linalg.cond(A)
            if angle is not None:
                c, s = np.cos(angle[k]), np.sin(angle[k])
                R = np.array([[c, -s], [s, c]])
                Sigma = R @ Sigma @ R.T
            out["cov"][k] = (Sigma[0, 0], Sigma[0, 1], Sigma[1, 1])
    return out


def check_against_np(got, ref, what=""):
    """The GPU tests' comparison: n_valid and status equal; Hessian within TOL after normalising by sqrt(H_aa H_bb);
    covariance within 2 kappa TOL after normalising by sqrt(S_aa S_bb) where the status is OK, NaN elsewhere; mean within
    TOL relative.  Prints the worst figure of each kind and returns them."""
    n_valid, status = np.asarray(got["n_valid"]), np.asarray(got["status"])
    assert np.array_equal(n_valid, ref["n_valid"]), (what, np.flatnonzero(n_valid != ref["n_valid"]))
    assert np.array_equal(status, ref["status"]), (what, np.flatnonzero(status != ref["status"]))
    H, Hr = np.asarray(got["hessian"]), ref["hessian"]
    ok = ref["status"] == patches.PATCH_OK
    worst_h = worst_c = worst_m = 0.0
    idx = {(0, 0): 0, (0, 1): 1, (0, 2): 2, (1, 1): 3, (1, 2): 4, (2, 2): 5}
    for (a, b), c in idx.items():
        den = np.sqrt(Hr[ok, idx[(a, a)]] * Hr[ok, idx[(b, b)]])
        worst_h = max(worst_h, float(np.max(np.abs(H[ok, c] - Hr[ok, c]) / den, initial=0.0)))
    cov, cr = np.asarray(got["cov"]), ref["cov"]
    assert np.all(np.isnan(cov[~ok])), what
    assert np.all(np.isfinite(cov[ok])), what
    for c, (a, b) in enumerate(((0, 0), (0, 2), (2, 2))):
        den = np.sqrt(cr[ok, a] * cr[ok, b]) * (2.0 * ref["kappa"][ok] * TOL)
        worst_c = max(worst_c, float(np.max(np.abs(cov[ok, c] - cr[ok, c]) / den, initial=0.0)))
    some = ref["n_valid"] > 0
    finite = some & np.isfinite(ref["mean"]) & (ref["mean"] != 0)
    worst_m = float(np.max(np.abs(np.asarray(got["mean"])[finite] - ref["mean"][finite]) / np.abs(ref["mean"][finite]),
                           initial=0.0))
    print(f"{what}: Hessian {worst_h:.3e} (bound {TOL:.0e}), covariance {worst_c:.3e} of its bound 2 kappa {TOL:.0e} "
          f"(kappa up to {np.max(ref['kappa'][ok], initial=0.0):.3e}), mean {worst_m:.3e}")
    assert worst_h <= TOL, (what, worst_h)
    assert worst_c <= 1.0, (what, worst_c)
    assert worst_m <= TOL, (what, worst_m)
    return worst_h, worst_c, worst_m


# ---- the data the GPU tests share ------------------------------------------------------------------------------------
def texture(h, w, seed, lo=24.0, hi=230.0):
    """smoothed noise in [lo, hi], float64 [h,w]: white noise under three passes of the 1-2-1 filter per axis"""
    rng = np.random.default_rng(seed)
    a = rng.random((h + 6, w + 6))
    for _ in range(3):
        a = 0.25 * a[:-2] + 0.5 * a[1:-1] + 0.25 * a[2:]
        a = 0.25 * a[:, :-2] + 0.5 * a[:, 1:-1] + 0.25 * a[:, 2:]
    a = (a - a.min()) / (a.max() - a.min())
    return lo + (hi - lo) * a


EDGE_H, EDGE_W, EDGE_PITCH, EDGE_SEED = 24, 32, 40, 11


def edge_image():
    """the 24 x 32 float32 image of GPU test 1 in a [24, 40] buffer (pitch 40; the padding holds a value no valid read
    may return)"""
    buf = np.full((EDGE_H, EDGE_PITCH), -1.0e6, dtype=np.float32)
    buf[:, :EDGE_W] = texture(EDGE_H, EDGE_W, EDGE_SEED).astype(np.float32)
    return buf


def n_valid_np(pts, h=EDGE_H, w=EDGE_W, pattern=patches.PATTERN52):
    p = np.asarray(pts, dtype=np.float64)[:, None, :] + pattern[None]
    with np.errstate(invalid="ignore"):
        return ((p[..., 0] >= 2) & (p[..., 0] < w - 3) & (p[..., 1] >= 2) & (p[..., 1] < h - 3)).sum(1)


def edge_points(h=EDGE_H, w=EDGE_W):
    """Every position of GPU test 1 -> (pts [M,2], labels).  Interior keypoints (integer and fractional); for each of the
    four borders one keypoint per number of valid points that border can produce with Pattern52, from 1 up to 48 (found on
    a grid of positions around the border, corners included; the outermost column or row of Pattern52 holds four points,
    so 49, 50 and 51 cannot occur with it: `skew_points` covers every count from 1 to 51); pattern points exactly at
    x = 2, at x = w - 3 and just below it, the same in y; a centre outside the image and a NaN."""
    pts, labels = [], []

    def add(x, y, label):
        pts.append((x, y))
        labels.append(label)
    for x, y in ((12.0, 10.0), (16.0, 12.0), (13.37, 11.61), (9.999, 8.25), (20.5, 16.75), (5.5, 5.5)):
        add(x, y, "interior")
    below = lambda v: float(np.nextafter(v, -np.inf))
    # Pattern52 reaches 3.5 to each side: its outermost column sits exactly on x = 2 for a centre at 5.5 (valid) and on
    # x = w - 3 for a centre at w - 6.5 (not valid; the double just below is)
    for x, label in ((5.5, "x=2"), (below(5.5), "x<2"), (w - 6.5, "x=w-3"), (below(w - 6.5), "x<w-3")):
        add(x, 11.25, label)
    for y, label in ((5.5, "y=2"), (below(5.5), "y<2"), (h - 6.5, "y=h-3"), (below(h - 6.5), "y<h-3")):
        add(14.75, y, label)
    gx = np.arange(-2.0, w + 2.0, 0.25) + 0.0625
    gy = np.arange(-2.0, h + 2.0, 0.25) + 0.03125
    X, Y = np.meshgrid(gx, gy)
    cand = np.stack([X.ravel(), Y.ravel()], 1)
    nv = n_valid_np(cand, h, w)
    border = {"left": cand[:, 0] < 5.5, "right": cand[:, 0] >= w - 6.5, "top": cand[:, 1] < 5.5, "bottom": cand[:, 1] >= h - 6.5}
    for name, near in border.items():
        for n in range(1, 52):
            hit = np.flatnonzero(near & (nv == n))
            if hit.size:
                k = hit[hit.size // 2]
                add(float(cand[k, 0]), float(cand[k, 1]), f"{name}:{n}")
    add(-10.0, 5.0, "outside")
    add(float(w) + 40.0, float(h) + 3.0, "outside")
    add(float("nan"), 8.0, "nan")
    return np.asarray(pts, dtype=np.float64), labels


# Pattern52 sheared a little: all 52 abscissae differ and all 52 ordinates differ, so a border removes the points one at
# a time and every count from 1 to 51 occurs at each of the four borders
PATTERN_SKEW = np.ascontiguousarray(patches.PATTERN52 @ np.array([[1.0, 0.017], [0.013, 1.0]]))


def skew_points(h=EDGE_H, w=EDGE_W):
    """For PATTERN_SKEW: per border and per n = 1 .. 51 a keypoint with exactly n valid points, the border's threshold
    halfway between the n-th and the (n+1)-th pattern point -> (pts [204,2], counts [204])."""
    px, py = np.sort(PATTERN_SKEW[:, 0]), np.sort(PATTERN_SKEW[:, 1])
    pts, counts = [], []
    for n in range(1, 52):
        pts.append((2.0 - 0.5 * (px[52 - n] + px[51 - n]), 11.3))           # left: the n largest abscissae stay
        pts.append(((w - 3.0) - 0.5 * (px[n - 1] + px[n]), 12.6))          # right: the n smallest stay
        pts.append((15.2, 2.0 - 0.5 * (py[52 - n] + py[51 - n])))           # top
        pts.append((16.7, (h - 3.0) - 0.5 * (py[n - 1] + py[n])))          # bottom
        counts += [n] * 4
    return np.asarray(pts, dtype=np.float64), np.asarray(counts)


# ---- the yardstick itself --------------------------------------------------------------------------------------------
def test_value_and_gradient_are_exact_on_an_affine_image():
    a, b, c = 7.0, 3.0, -2.0
    yy, xx = np.mgrid[0:24, 0:32]
    img = a + b * xx + c * yy                       # small integers: every product and sum below is exact
    px = np.array([2.0, 5.25, 17.5, 28.875, 11.0])
    py = np.array([2.0, 9.75, 3.125, 20.5, 20.96875])
    v, gx, gy = interp_grad_np(img.astype(np.float64), px, py)
    assert np.array_equal(v, a + b * px + c * py)
    assert np.array_equal(gx, np.full(5, b)) and np.array_equal(gy, np.full(5, c))


def test_a_power_of_two_intensity_scale_keeps_the_bits_of_cov_and_hessian():
    img = np.round(texture(40, 48, 3))              # integers, so that 256 * img is exact in every pixel type
    pts = np.array([[20.0, 18.0], [23.4, 21.7], [6.2, 30.1], [44.0, 3.0], [3.0, 3.0]])
    ang = np.array([0.3, -1.1, 2.0, 0.0, 0.7])
    one = patch_cov_np(img, pts, angle=ang)
    big = patch_cov_np(256.0 * img, pts, angle=ang)
    assert np.array_equal(one["status"], big["status"]) and np.array_equal(one["n_valid"], big["n_valid"])
    assert (one["status"] == patches.PATCH_OK).sum() >= 3
    assert np.array_equal(one["cov"], big["cov"], equal_nan=True)
    assert np.array_equal(one["hessian"], big["hessian"])
    assert np.array_equal(256.0 * one["mean"], big["mean"], equal_nan=True)


def test_pattern52():
    p = patches.PATTERN52
    assert p.shape == (52, 2) and p.dtype == np.float64 and not p.flags.writeable
    assert len({(x, y) for x, y in p}) == 52
    assert {(x, y) for x, y in p} == {(-x, -y) for x, y in p}
    assert np.max(np.hypot(p[:, 0], p[:, 1])) < 4.0
    assert np.array_equal(p[0], (-1.5, 3.5)) and np.array_equal(p[3], (1.5, 3.5)) and np.array_equal(p[4], (-2.5, 2.5))
    assert np.array_equal(p[-1], (1.5, -3.5)) and np.all(np.diff(p[:, 1]) <= 0)
    rows = [int((p[:, 1] == y).sum()) for y in np.arange(3.5, -4.0, -1.0)]
    assert rows == [4, 6, 8, 8, 8, 8, 6, 4]


def test_constant_and_ramp_images_are_singular_and_empty_patches_empty():
    yy, xx = np.mgrid[0:30, 0:30].astype(np.float64)
    pts = np.array([[14.0, 15.0], [12.5, 13.25]])
    for img in (10.0 + 2.0 * xx, np.full((30, 30), 77.0), 5.0 + 1.5 * yy):
        r = patch_cov_np(img, pts)
        assert np.all(r["status"] == patches.PATCH_SINGULAR) and np.all(np.isnan(r["cov"])) and np.all(r["n_valid"] == 52)
    r = patch_cov_np(np.zeros((30, 30)), pts)
    assert np.all(r["status"] == patches.PATCH_EMPTY) and np.all(np.isnan(r["cov"]))
    r = patch_cov_np(10.0 + 2.0 * xx, np.array([[-20.0, 3.0]]))
    assert r["status"][0] == patches.PATCH_EMPTY and r["n_valid"][0] == 0 and np.all(r["hessian"] == 0)


def test_a_textured_patch_gives_a_positive_definite_covariance_that_rotates_with_the_angle():
    img = texture(40, 48, 5)
    pts = np.array([[20.0, 18.0], [25.3, 20.9]])
    r0 = patch_cov_np(img, pts)
    r1 = patch_cov_np(img, pts, angle=np.array([np.pi / 2, np.pi / 2]))
    assert np.all(r0["status"] == 0) and np.all(r0["kappa"] < 1e6)
    xx, xy, yy = r0["cov"].T
    assert np.all(xx > 0) and np.all(xx * yy - xy * xy > 0)
    # a quarter turn swaps the axes
    assert np.allclose(r1["cov"][:, 0], yy, rtol=1e-12) and np.allclose(r1["cov"][:, 2], xx, rtol=1e-12)
    assert np.allclose(r1["cov"][:, 1], -xy, rtol=1e-9, atol=1e-18)
    # scaling divides the covariance and multiplies the Hessian
    r5 = patch_cov_np(img, pts, scaling=5.0)
    assert np.allclose(r5["cov"], 2.0 * r0["cov"], rtol=1e-14) and np.allclose(2.0 * r5["hessian"], r0["hessian"], rtol=1e-14)


def test_the_edge_case_covers_what_it_claims():
    pts, labels = edge_points()
    nv = n_valid_np(pts)
    by = dict(zip(labels, nv))
    assert by["x=2"] == 52 and by["x<2"] == 48 and by["x=w-3"] == 48 and by["x<w-3"] == 52
    assert by["y=2"] == 52 and by["y<2"] == 48 and by["y=h-3"] == 48 and by["y<h-3"] == 52
    assert by["outside"] == 0 and by["nan"] == 0
    for name in ("left", "right", "top", "bottom"):
        got = sorted(int(l.split(":")[1]) for l in labels if l.startswith(name + ":"))
        assert got[0] == 1 and got[-1] == 48 and len(got) >= 20, (name, got)
        for l, n in zip(labels, nv):
            if l.startswith(name + ":"):
                assert n == int(l.split(":")[1])
    # the sheared pattern: every count from 1 to 51 at each of the four borders
    assert len({tuple(r) for r in np.round(PATTERN_SKEW[:, :1], 12)}) == 52 == len({tuple(r) for r in np.round(PATTERN_SKEW[:, 1:], 12)})
    spts, counts = skew_points()
    assert np.array_equal(n_valid_np(spts, pattern=PATTERN_SKEW), counts) and len(spts) == 4 * 51
    sref = patch_cov_np(edge_image()[:, :EDGE_W], spts, pattern=PATTERN_SKEW)
    sok = sref["status"] == patches.PATCH_OK
    print(f"sheared pattern: {sok.sum()} of {len(spts)} OK, kappa up to {np.max(sref['kappa'][sok]):.3e}")
    assert np.all(sref["kappa"][sok] < 1e6) and np.all(sref["n_valid"][~sok] < 3)
    ref = patch_cov_np(edge_image()[:, :EDGE_W], pts)
    ok = ref["status"] == patches.PATCH_OK
    assert ok.sum() >= 100 and np.all(ref["kappa"][ok] < 1e6), np.max(ref["kappa"][ok])
    # nothing but a count below three, or no point at all, is refused on this texture
    assert np.all(ref["n_valid"][ref["status"] == patches.PATCH_SINGULAR] < 3)
    assert np.all(ref["n_valid"][ref["status"] == patches.PATCH_EMPTY] == 0)


# ---- the ABI ---------------------------------------------------------------------------------------------------------
def test_symbol_is_declared_bound_and_exported_within_abi_8():
    assert "pnec_hip_patch_covariance" in capi.SYMBOLS
    L = capi.lib()
    assert getattr(L, "pnec_hip_patch_covariance") is not None
    assert len(L.pnec_hip_patch_covariance.argtypes) == 21
    assert capi.ABI_VERSION == 8 and L.pnec_hip_abi_version() == 8
    header = open(os.path.join(ROOT, "include", "pnec_hip.h")).read()
    assert "#define PNEC_HIP_ABI_VERSION 8" in header
    assert "int pnec_hip_patch_covariance(const void *images, int pixel_type, int64_t n_images" in header
    for words in ("ALL ARITHMETIC IS DOUBLE", "[EXT]", "This is NOT tracking", "2 <= p.x < width - 3",
                  "g'_i = n (g_i S - G d_i) / S^2", "PNEC_HIP_PATCH_EMPTY", "PNEC_HIP_PATCH_SINGULAR", "No atomics"):
        assert words in header, words
    assert (patches.PATCH_OK, patches.PATCH_EMPTY, patches.PATCH_SINGULAR) == (0, 1, 2)
    for name, value in (("PNEC_HIP_PATCH_EMPTY", 1), ("PNEC_HIP_PATCH_SINGULAR", 2), ("PNEC_HIP_PIXEL_U16", 1),
                        ("PNEC_HIP_PIXEL_F32", 2)):
        assert f"{name} = {value}" in header


def test_bad_arguments_are_refused_before_a_device_is_touched():
    L = capi.lib()
    img = np.zeros((24, 40), dtype=np.float32)
    offs = np.array([0, 2], dtype=np.int64)
    pts = np.array([[10.0, 10.0], [12.0, 11.0]])
    pat = np.ascontiguousarray(np.tile(patches.PATTERN52, (2, 1)))     # 104 rows: room for P = 65
    SENT = -7.25
    cov, hes, mean = np.full((2, 3), SENT), np.full((2, 6), SENT), np.full(2, SENT)
    nv, st = (np.full(2, -5, dtype=np.int32) for _ in range(2))
    outs = tuple(a.ctypes.data for a in (cov, hes, mean, nv, st))
    I, O, P, A = img.ctypes.data, offs.ctypes.data, pts.ctypes.data, pat.ctypes.data

    def call(images=I, ptype=2, F=1, h=24, w=32, pitch=40, offsets=O, M=2, p=P, pattern=A, n_pat=52, scaling=10.0,
             outputs=outs, space=capi.MEM_HOST):
        rc = L.pnec_hip_patch_covariance(images, ptype, F, h, w, pitch, offsets, M, p, pattern, n_pat, scaling, None,
                                         *outputs, space, 0, None)
        return rc, (L.pnec_hip_last_error() or b"").decode()
    for kw, word in ((dict(n_pat=65), "n_pattern"), (dict(n_pat=0), "n_pattern"), (dict(pitch=31), "pitch"),
                     (dict(ptype=3), "pixel_type"), (dict(ptype=-1), "pixel_type"), (dict(images=None), "NULL"),
                     (dict(offsets=None), "NULL"), (dict(p=None), "NULL"), (dict(pattern=None), "NULL"),
                     (dict(outputs=(None,) * 5), "output"), (dict(scaling=0.0), "scaling"),
                     (dict(scaling=float("nan")), "scaling"), (dict(F=0), "n_images"), (dict(h=0), "height"),
                     (dict(M=-1), "n_points"), (dict(space=5), "memory space"), (dict(M=3), "offsets")):
        rc, msg = call(**kw)
        assert rc == capi.ERR_INVALID_ARGUMENT == -1, (kw, rc, msg)
        assert "patch_covariance" in msg and word in msg, (kw, msg)
    # DEVICE space refuses the same things (the offsets, which it cannot read, aside)
    rc, msg = call(n_pat=65, space=capi.MEM_DEVICE)
    assert rc == -1 and "n_pattern" in msg
    assert np.all(cov == SENT) and np.all(hes == SENT) and np.all(mean == SENT) and np.all(nv == -5) and np.all(st == -5)
    # nothing to do is not an error, and touches no device either
    rc, msg = call(M=0, offsets=np.array([0, 0], dtype=np.int64).ctypes.data)
    assert rc == 0, msg


def test_python_facade_and_pybind_expose_the_new_names():
    import dataclasses
    assert {"patch_covariance", "PatchCovariance", "PATTERN52"} <= set(pnec_amd.__all__)
    assert pnec_amd.patch_covariance is patches.patch_covariance and pnec_amd.PATTERN52 is patches.PATTERN52
    assert [f.name for f in dataclasses.fields(pnec_amd.PatchCovariance)][:5] == ["cov", "hessian", "mean", "n_valid", "status"]
    import inspect
    sig = inspect.signature(patches.patch_covariance)
    assert list(sig.parameters)[:6] == ["images", "pts", "offsets", "pattern", "scaling", "angle"]
    assert sig.parameters["scaling"].default == 10.0 and sig.parameters["pattern"].default is patches.PATTERN52
    with pytest.raises(TypeError):
        patches.patch_covariance(np.zeros((8, 8), dtype=np.float64), np.zeros((1, 2)))
    import pnec_amd.pypnec as pypnec
    assert "patch_covariance" in dir(pypnec)
    facade = open(os.path.join(ROOT, "pnec_amd", "csrc", "host", "pnec_host.h")).read()
    assert "PatchCovariances(" in facade and "Pattern52()" in facade
    with open(os.path.join(ROOT, "pnec_amd", "libpnec_host.so"), "rb") as f:
        blob = f.read()
    assert b"PatchCovariances" in blob and b"Pattern52" in blob


# ---- the kernel's arithmetic on the host, under the sanitizers -------------------------------------------------------
def test_the_kernels_arithmetic_built_for_the_host_reads_no_pixel_outside_and_meets_the_gpu_bounds(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ builds the host facade, so it is there"
    exe = str(tmp_path / "patch_cov_host")
    subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "pnec_amd", "csrc"),
                    os.path.join(ROOT, "tools", "patch_cov_host.cc"), "-o", exe], check=True)
    pts, _ = edge_points()
    spts, _ = skew_points()
    buf = edge_image()
    flat = buf.reshape(-1)[: (EDGE_H - 1) * EDGE_PITCH + EDGE_W]            # not one pixel behind the last
    ang = np.linspace(-3.0, 3.0, len(pts))
    (tmp_path / "pts.bin").write_bytes(pts.tobytes())
    (tmp_path / "pat.bin").write_bytes(np.ascontiguousarray(patches.PATTERN52).tobytes())
    (tmp_path / "spts.bin").write_bytes(spts.tobytes())
    (tmp_path / "spat.bin").write_bytes(PATTERN_SKEW.tobytes())
    (tmp_path / "ang.bin").write_bytes(ang.tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    u8 = np.round(buf[:, :EDGE_W]).astype(np.uint8)
    u8p = np.zeros((EDGE_H, EDGE_PITCH), dtype=np.uint8)
    u8p[:, :EDGE_W] = u8
    cases = (("f32", flat, buf[:, :EDGE_W], None, False), ("f32", flat, buf[:, :EDGE_W], ang, False),
             ("u8", u8p.reshape(-1)[: flat.size], u8, None, False),
             ("u16", (u8p.astype(np.uint16) << 8).reshape(-1)[: flat.size], u8.astype(np.uint16) << 8, None, False),
             ("f32", flat, buf[:, :EDGE_W], None, True))
    results = {}
    for tag, (typ, pixels, image, angle, skew) in enumerate(cases):
        (tmp_path / "img.bin").write_bytes(np.ascontiguousarray(pixels).tobytes())
        args = [exe, typ, str(EDGE_H), str(EDGE_W), str(EDGE_PITCH), str(tmp_path / "img.bin"),
                str(tmp_path / ("spts.bin" if skew else "pts.bin")), str(tmp_path / ("spat.bin" if skew else "pat.bin")),
                "10.0", str(tmp_path / "out.bin")]
        if angle is not None:
            args.append(str(tmp_path / "ang.bin"))
        r = subprocess.run(args, env=env, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        assert "without slack" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
        o = np.frombuffer((tmp_path / "out.bin").read_bytes(), dtype=np.float64).reshape(-1, 12)
        got = dict(cov=o[:, :3], hessian=o[:, 3:9], mean=o[:, 9], n_valid=o[:, 10].astype(np.int32),
                   status=o[:, 11].astype(np.int32))
        ref = patch_cov_np(image, spts, pattern=PATTERN_SKEW) if skew else patch_cov_np(image, pts, angle=angle)
        check_against_np(got, ref, f"host build, {typ}{' + angle' if angle is not None else ''}{', sheared pattern' if skew else ''}")
        results[tag] = got
    # the same picture as uint8 and as uint16 << 8: identical bits of covariance and Hessian, the mean scales
    assert np.array_equal(results[2]["cov"], results[3]["cov"], equal_nan=True)
    assert np.array_equal(results[2]["hessian"], results[3]["hessian"], equal_nan=True)
    assert np.array_equal(256.0 * results[2]["mean"], results[3]["mean"], equal_nan=True)
