"""Patch tracking without a GPU.

`pyramid_np` and `patch_track_np` below are the plain-numpy statements of the definitions in include/pnec_hip.h
(pnec_hip_image_pyramid_level, pnec_hip_patch_track), every sum in the pattern's own order: the yardsticks of
tests/test_patch_track_gpu.py, tested here on their own -- the pyramid on a constant, a ramp and impulses at the borders,
the SE(2) step against a matrix exponential, the template's gain against numpy.linalg.solve, the pyramid doing the work on
the main fixture -- together with the new symbols' declaration, binding and export (which fails on the parent commit), the
argument checks (which return before any device is touched), the Python / facade / pybind names, and the fixtures' own
claims (every status, every level, no decision on a knife's edge).

The last tests build the kernel's own arithmetic for the host (tools/patch_track_host.cc: the functions of
pnec_amd/csrc/pnec_patch_track.hpp and pnec_patch_cov.hpp in the kernel's control flow and order of sums) with the address
and undefined-behaviour sanitizers, as a stand-alone program, and run it over every keypoint of the GPU fixtures with each
pyramid level in a heap block without a byte of slack: an index error shows there, not on a device.  Its output is
compared with `patch_track_np` under the GPU tests' own bounds.
"""
import ctypes as C
import functools
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_patch_covariance_cpu import interp_grad_np  # noqa: E402

import pnec_amd  # noqa: E402
from pnec_amd import capi, patches  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-10     # the project's bar for sums of products (tests/test_patch_covariance_cpu.py); positions: 2 kappa TOL px
KERNEL5 = np.array([1, 4, 6, 4, 1])
OK, BAD, LOSTF, LOSTB, FAR = (patches.TRACK_OK, patches.TRACK_BAD_TEMPLATE, patches.TRACK_LOST_FORWARD,
                              patches.TRACK_LOST_BACKWARD, patches.TRACK_RECOVERED_TOO_FAR)


# ---- the yardsticks --------------------------------------------------------------------------------------------------
def _reflect(i, n):
    i = np.where(i < 0, -i, i)
    return np.where(i >= n, 2 * n - 2 - i, i)


def pyramid_np(images):
    """one halving step of [F,h,w] (or [h,w]) images, dtype kept: include/pnec_hip.h's definition"""
    images = np.asarray(images)
    single = images.ndim == 2
    if single:
        images = images[None]
    F, h, w = images.shape
    cols = _reflect(2 * np.arange(w // 2)[:, None] + np.arange(5)[None] - 2, w)      # [w2,5]
    rows = _reflect(2 * np.arange(h // 2)[:, None] + np.arange(5)[None] - 2, h)      # [h2,5]
    acc = images.astype(np.float64 if images.dtype == np.float32 else np.int64)
    inner = 0
    for i in range(5):                                    # ascending index, inner sum first
        inner = inner + KERNEL5[i] * acc[:, :, cols[:, i]]                           # [F,h,w2]
    outer = 0
    for j in range(5):
        outer = outer + KERNEL5[j] * inner[:, rows[:, j], :]                         # [F,h2,w2]
    out = (outer / 256.0).astype(np.float32) if images.dtype == np.float32 else ((outer + 128) >> 8).astype(images.dtype)
    return out[0] if single else out


def pyramid_levels_np(images, levels):
    out = [np.asarray(images)]
    for _ in range(1, levels):
        out.append(pyramid_np(out[-1]))
    return out


def _seq(x):
    """the sum of x in its own order (accumulate is sequential)"""
    return float(np.add.accumulate(np.asarray(x, dtype=np.float64))[-1])


def _valid(px, py, w, h):
    with np.errstate(invalid="ignore"):
        return (px >= 2) & (px < w - 3) & (py >= 2) & (py < h - 3)


def _edge(px, py, w, h):
    """how far the coordinates are from the thresholds of the validity rule (NaN coordinates decide nothing by rounding)"""
    d = np.concatenate([np.abs(np.ravel(px) - 2), np.abs(np.ravel(px) - (w - 3)), np.abs(np.ravel(py) - 2),
                        np.abs(np.ravel(py) - (h - 3))])
    d = d[np.isfinite(d)]
    return float(d.min()) if d.size else np.inf


def template_np(img, q, pattern):
    """the template of one keypoint at one level: dict(status, valid, data, K [P,3], H [3,3], n, S, kappa, edge)"""
    h, w = img.shape
    px, py = q[0] + pattern[:, 0], q[1] + pattern[:, 1]
    valid = _valid(px, py, w, h)
    P = len(pattern)
    d, gx, gy = np.zeros(P), np.zeros(P), np.zeros(P)
    n = int(valid.sum())
    if n:
        d[valid], gx[valid], gy[valid] = interp_grad_np(img, px[valid], py[valid])
    S, Gx, Gy = _seq(d), _seq(gx), _seq(gy)
    out = dict(valid=valid, n=n, S=S, kappa=np.inf, edge=_edge(px, py, w, h), status=patches.PATCH_OK,
               data=np.zeros(P), K=np.zeros((P, 3)), H=np.zeros((3, 3)))
    if n == 0 or not (S > 0 and np.isfinite(S)):
        out["status"] = patches.PATCH_EMPTY
        return out
    with np.errstate(all="ignore"):
        gpx = np.where(valid, n * (gx * S - Gx * d) / (S * S), 0.0)
        gpy = np.where(valid, n * (gy * S - Gy * d) / (S * S), 0.0)
        J = np.stack([gpx, gpy, -pattern[:, 1] * gpx + pattern[:, 0] * gpy], 1)
        H = np.zeros((3, 3))
        for i in range(P):
            H += np.outer(J[i], J[i])
        sc = 1.0 / np.sqrt(np.diag(H))
        A = H * np.outer(sc, sc)
    out["H"] = H
    ok = n >= 3 and bool(np.all(np.isfinite(A)))
    if ok:
        try:
            np.linalg.cholesky(A)
        except np.linalg.LinAlgError:
            ok = False
    if ok:
        Hinv = np.linalg.inv(A) * np.outer(sc, sc)
        ok = bool(np.all(np.isfinite(Hinv)))
    if not ok:
        out["status"] = patches.PATCH_SINGULAR
        return out
    out["kappa"] = float(np.linalg.cond(A))
    out["data"] = (n * d) / S
    out["K"] = J @ Hinv            # rows K_i' = J_i H^-1 (H^-1 is symmetric)
    out["Hinv"] = Hinv
    return out


def se2_step_np(t, theta, inc):
    """T <- T exp(inc), as include/pnec_hip.h states it"""
    d = inc[2]
    if abs(d) < 1e-10:
        a, b = 1.0 - d * d / 6.0, 0.5 * d
    else:
        a, b = np.sin(d) / d, (1.0 - np.cos(d)) / d
    u = np.array([a * inc[0] - b * inc[1], b * inc[0] + a * inc[1]])
    c, s = np.cos(theta), np.sin(theta)
    return t + np.array([c * u[0] - s * u[1], s * u[0] + c * u[1]]), theta + d


def _value_np(img, px, py):
    ix, iy = np.floor(px).astype(np.int64), np.floor(py).astype(np.int64)
    dx, dy = px - ix, py - iy
    ddx, ddy = 1.0 - dx, 1.0 - dy
    return ((ddx * ddy * img[iy, ix] + ddx * dy * img[iy + 1, ix]) + dx * ddy * img[iy, ix + 1]) + dx * dy * img[iy + 1, ix + 1]


def _direction_np(pyr, tmpls, f, t, theta, pattern, max_iterations, edge):
    """one direction over the levels L-1 .. 0 -> (t, theta, lost_level or -1, bad_template)"""
    P = len(pattern)
    for l in range(len(pyr) - 1, -1, -1):
        tm = tmpls[l]
        if tm["status"] != patches.PATCH_OK:
            return t, theta, l, True
        img = pyr[l][f]
        h, w = img.shape
        scale = float(1 << l)
        t = t / scale
        lost = False
        for _ in range(max_iterations):
            c, s = np.cos(theta), np.sin(theta)
            px = (c * pattern[:, 0] - s * pattern[:, 1]) + t[0]
            py = (s * pattern[:, 0] + c * pattern[:, 1]) + t[1]
            val = _valid(px, py, w, h)
            edge[0] = min(edge[0], _edge(px, py, w, h))
            v = np.zeros(P)
            if val.any():
                v[val] = _value_np(img, px[val], py[val])
            n2, S2 = int(val.sum()), _seq(v)
            both = val & tm["valid"]
            if int(both.sum()) <= P // 2 or not (S2 > 0 and np.isfinite(S2)):
                lost = True
                break
            r = np.where(both, (n2 * v) / S2 - tm["data"], 0.0)
            inc = -np.array([_seq(tm["K"][:, a] * r) for a in range(3)])
            with np.errstate(all="ignore"):
                t, theta = se2_step_np(t, theta, inc)
            edge[0] = min(edge[0], _edge(t[0], t[1], w, h))
            if not (bool(_valid(t[0], t[1], w, h)) and abs(inc[2]) < 1e6 and abs(theta) < 1e6):
                lost = True
                break
        t = t * scale
        if lost:
            return t, theta, l, False
    return t, theta, -1, False


def patch_track_np(tmpl, next, tmpl_pts, offsets=None, prev=None, init_pts=None, init_angle=None, shift=(0.0, 0.0),
                   pattern=patches.PATTERN52, max_iterations=40, max_recovered_dist2=0.04, backward=True, scaling=10.0):
    """include/pnec_hip.h's definition in numpy.  Pyramids: lists of [F,h_l,w_l] arrays of any dtype (taken as float64
    values).  Returns a dict: pts [M,2], angle [M], cov [M,3], dist2 [M], status [M], lost_level [M], rec [M,2] (where the
    backward track ended), kappa [M] (the largest condition number of the Jacobi-scaled H over the levels with a usable
    template; 0 when no level has one: that transform never moves) and edge [M]: the smallest distance of any coordinate the track compared with a threshold of the
    validity rule from that threshold, and of dist2 from max_recovered_dist2 where that comparison can go either way."""
    tmpl = [np.asarray(a, dtype=np.float64) for a in tmpl]
    nxt = [np.asarray(a, dtype=np.float64) for a in next]
    prv = tmpl if prev is None else [np.asarray(a, dtype=np.float64) for a in prev]
    tmpl, nxt, prv = ([a[None] if a.ndim == 2 else a for a in p] for p in (tmpl, nxt, prv))
    tmpl_pts = np.asarray(tmpl_pts, dtype=np.float64).reshape(-1, 2)
    M, F = len(tmpl_pts), tmpl[0].shape[0]
    offsets = np.array([0, M]) if offsets is None else np.asarray(offsets)
    init_pts = tmpl_pts if init_pts is None else np.asarray(init_pts, dtype=np.float64)
    init_angle = np.zeros(M) if init_angle is None else np.asarray(init_angle, dtype=np.float64)
    pattern = np.asarray(pattern, dtype=np.float64)
    shift = np.asarray(shift, dtype=np.float64)
    out = dict(pts=np.zeros((M, 2)), angle=np.zeros(M), cov=np.full((M, 3), np.nan), dist2=np.full(M, np.nan),
               status=np.zeros(M, np.int32), lost_level=np.full(M, -1, np.int32), rec=np.full((M, 2), np.nan),
               kappa=np.zeros(M), edge=np.full(M, np.inf))
    for f in range(F):
        for k in range(int(offsets[f]), int(offsets[f + 1])):
            tmpls = [template_np(tmpl[l][f], tmpl_pts[k] / float(1 << l), pattern) for l in range(len(tmpl))]
            # (over the levels whose template is usable -- the others are never tracked on; 0 when there is none)
            out["kappa"][k] = max([tm["kappa"] for tm in tmpls if np.isfinite(tm["kappa"])], default=0.0)
            edge = [min(tm["edge"] for tm in tmpls)]
            t, theta, lost, bad = _direction_np(nxt, tmpls, f, init_pts[k] + shift, init_angle[k], pattern, max_iterations,
                                                edge)
            out["pts"][k], out["angle"][k] = t, theta
            status = OK
            if lost >= 0:
                status = BAD if bad else LOSTF
            elif backward:
                rec, _, lost, bad = _direction_np(prv, tmpls, f, t - shift, theta, pattern, max_iterations, edge)
                if lost >= 0:
                    status = BAD if bad else LOSTB
                else:
                    e = init_pts[k] - rec
                    d2 = e[0] * e[0] + e[1] * e[1]
                    out["rec"][k], out["dist2"][k] = rec, d2
                    if not d2 < max_recovered_dist2:
                        status = FAR
                    if max_recovered_dist2 > 0:     # (dist2 < 0 is false whatever the rounding: a sum of squares)
                        edge[0] = min(edge[0], abs(d2 - max_recovered_dist2))
            out["status"][k], out["lost_level"][k], out["edge"][k] = status, lost, edge[0]
            if status == OK:
                tm = tmpls[0]
                c, s = np.cos(theta), np.sin(theta)
                R = np.array([[c, -s], [s, c]])
                Sigma = R @ (tm["Hinv"][:2, :2] / scaling) @ R.T
                out["cov"][k] = (Sigma[0, 0], Sigma[0, 1], Sigma[1, 1])
    return out


PATTERN_RADIUS = float(np.max(np.hypot(patches.PATTERN52[:, 0], patches.PATTERN52[:, 1])))


def check_track_against_np(got, ref, what="", radius=PATTERN_RADIUS):
    """The GPU tests' comparison, on ALL keypoints: status and lost_level equal; positions within 2 kappa TOL px, angles
    within that over the pattern's radius (kappa = 0: no usable template, the transform never moved and must be equal);
    dist2 within the first-order propagation of the position bound, 2 (|e_x| + |e_y|) b + 2 b^2; NaN where the reference
    has NaN.  Prints the worst figures as fractions of their bounds and returns them."""
    status, level = np.asarray(got["status"]), np.asarray(got["lost_level"])
    assert np.array_equal(status, ref["status"]), (what, np.flatnonzero(status != ref["status"]), status, ref["status"])
    assert np.array_equal(level, ref["lost_level"]), (what, np.flatnonzero(level != ref["lost_level"]))
    pts, ang, d2 = np.asarray(got["pts"]), np.asarray(got["angle"]), np.asarray(got["dist2"])
    bad = ref["kappa"] == 0
    same = lambda a, b: np.array_equal(a, b, equal_nan=True)
    assert same(pts[bad], ref["pts"][bad]) and same(ang[bad], ref["angle"][bad]), what
    fin = ~bad & np.all(np.isfinite(ref["pts"]), 1) & np.isfinite(ref["angle"])
    assert same(np.isnan(pts[~bad]), np.isnan(ref["pts"][~bad])) and same(np.isnan(ang[~bad]), np.isnan(ref["angle"][~bad])), what
    bound = 2.0 * ref["kappa"][fin] * TOL
    worst_p = float(np.max(np.max(np.abs(pts[fin] - ref["pts"][fin]), 1) / bound, initial=0.0))
    worst_a = float(np.max(np.abs(ang[fin] - ref["angle"][fin]) / (bound / radius), initial=0.0))
    has = np.isfinite(ref["dist2"])
    assert np.all(np.isnan(d2[~has])) and np.all(np.isfinite(d2[has])), what
    b = 2.0 * ref["kappa"][has] * TOL
    bound_d = 2.0 * np.sqrt(2.0 * ref["dist2"][has]) * b + 2.0 * b * b               # |e_x| + |e_y| <= sqrt(2) |e|
    worst_d = float(np.max(np.abs(d2[has] - ref["dist2"][has]) / bound_d, initial=0.0))
    print(f"{what}: positions {worst_p:.3e}, angles {worst_a:.3e}, dist2 {worst_d:.3e} of their bounds "
          f"(2 kappa {TOL:.0e} px, kappa up to {np.max(ref['kappa'][fin], initial=0.0):.3g}; {int(fin.sum())} of {len(status)} "
          f"keypoints with a finite transform, none excluded)")
    assert worst_p <= 1.0, (what, worst_p)
    assert worst_a <= 1.0, (what, worst_a)
    assert worst_d <= 1.0, (what, worst_d)
    return worst_p, worst_a, worst_d


# ---- the data the GPU tests share ------------------------------------------------------------------------------------
H0, W0, LEVELS = 96, 128, 3                 # 24 x 32 at the top: the smallest at which a Pattern52 patch still fits
TRUE_SHIFT, TRUE_ANGLE = np.array([5.3, -3.7]), 0.03


def analytic(x, y, seed):
    """a smooth texture in [24, 230]: ten sinusoids, wavelengths 9 .. 40 px"""
    rng = np.random.default_rng(seed)
    lam, phi, psi = rng.uniform(9.0, 40.0, 10), rng.uniform(0.0, np.pi, 10), rng.uniform(0.0, 2 * np.pi, 10)
    amp = rng.uniform(0.5, 1.0, 10)
    z = sum(a * np.sin(2 * np.pi * (x * np.cos(p) + y * np.sin(p)) / l + q) for a, l, p, q in zip(amp, lam, phi, psi))
    return 127.0 + 103.0 * z / amp.sum()


def warp_truth(p):
    """where a point of image 1 lies in image 2: a rotation by TRUE_ANGLE about the centre and TRUE_SHIFT"""
    c, s = np.cos(TRUE_ANGLE), np.sin(TRUE_ANGLE)
    ctr = np.array([(W0 - 1) / 2.0, (H0 - 1) / 2.0])
    return (np.asarray(p) - ctr) @ np.array([[c, -s], [s, c]]).T + ctr + TRUE_SHIFT


@functools.lru_cache(maxsize=None)
def main_fixture():
    """-> dict: img1, img2 [3,96,128] uint8 (image 2 is image 1's function at the warped coordinates), pts [40,2],
    offsets [4] (the middle image has no keypoints), truth [40,2], and the uint8 pyramids p1, p2 (pyramid_np)"""
    yy, xx = np.mgrid[0:H0, 0:W0].astype(np.float64)
    c, s = np.cos(TRUE_ANGLE), np.sin(TRUE_ANGLE)
    ctr = np.array([(W0 - 1) / 2.0, (H0 - 1) / 2.0])
    ux, uy = xx - ctr[0] - TRUE_SHIFT[0], yy - ctr[1] - TRUE_SHIFT[1]       # the inverse warp of the pixel grid
    bx, by = c * ux + s * uy + ctr[0], -s * ux + c * uy + ctr[1]
    img1 = np.stack([np.round(analytic(xx, yy, 100 + f)) for f in range(3)]).astype(np.uint8)
    img2 = np.stack([np.round(analytic(bx, by, 100 + f)) for f in range(3)]).astype(np.uint8)
    rng = np.random.default_rng(2)
    pts = np.stack([rng.uniform(30.0, 92.0, 40), rng.uniform(32.0, 62.0, 40)], 1)
    for a in (img1, img2, pts):
        a.setflags(write=False)
    return dict(img1=img1, img2=img2, pts=pts, offsets=np.array([0, 22, 22, 40], dtype=np.int64), truth=warp_truth(pts),
                p1=pyramid_levels_np(img1, LEVELS), p2=pyramid_levels_np(img2, LEVELS))


@functools.lru_cache(maxsize=None)
def main_reference():
    fx = main_fixture()
    return patch_track_np(fx["p1"], fx["p2"], fx["pts"], fx["offsets"])


def status_cases():
    """The status fixture: a list of (name, kwargs of patch_track / patch_track_np).  Built on the main fixture's
    pyramids, with whole levels of single images blanked (a zero image has S2 = 0: lost at that level and no other) or
    made constant (a singular template at that level)."""
    fx = main_fixture()
    p1, p2 = fx["p1"], fx["p2"]

    def with_level(pyr, image_level_value):
        out = [a.copy() for a in pyr]
        for f, l, v in image_level_value:
            out[l][f] = v
        return out
    pts = fx["pts"][[0, 1, 2, 3, 4, 5, 22, 23, 24, 25, 26, 27]]           # six in image 0, six in image 2
    three = np.array([0, 4, 8, 12], dtype=np.int64)                        # the same twelve over three images
    pts3 = np.concatenate([fx["pts"][0:4], fx["pts"][4:8], fx["pts"][22:26]])
    # A: forward.  image 0 untouched, next blank at level 0 in image 1 and at level 1 in image 2; keypoint 1 starts far
    # outside (lost at the top), keypoint 2 starts at a NaN, keypoint 3's template position is a NaN
    init = pts3.copy()
    init[1] = (-50.0, 40.0)
    init[2] = (np.nan, 30.0)
    tp = pts3.copy()
    tp[3] = (50.0, np.nan)
    a_next = with_level(p2, [(1, 0, 0), (2, 1, 0)])
    A = dict(tmpl=p1, next=a_next, tmpl_pts=tp, offsets=three, init_pts=init)
    # B: templates.  tmpl constant at level 0 in image 1, at level 1 in image 2, at the top in image 0
    b_tmpl = with_level(p1, [(0, 2, 77), (1, 0, 77), (2, 1, 77)])
    B = dict(tmpl=b_tmpl, next=p2, tmpl_pts=pts3, offsets=three)
    # C: backward only.  prev differs from tmpl: blank at the top in image 0, at level 0 in image 1, at level 1 in image 2
    c_prev = with_level(p1, [(0, 2, 0), (1, 0, 0), (2, 1, 0)])
    Cc = dict(tmpl=p1, next=p2, tmpl_pts=pts3, offsets=three, prev=c_prev)
    # D: A with max_recovered_dist2 = 0 -- every survivor is too far, since < is strict
    D = dict(A, max_recovered_dist2=0.0)
    # E: one pattern point.  (A one-point template has rank one: BAD_TEMPLATE at the top level, before the count rule
    # m <= n_pattern / 2 = 0 is ever asked.)
    E = dict(tmpl=p1, next=p2, tmpl_pts=pts, offsets=np.array([0, 6, 6, 12], dtype=np.int64),
             pattern=np.ascontiguousarray(patches.PATTERN52[:1]))
    return [("forward", A), ("templates", B), ("backward", Cc), ("strict", D), ("one point", E)]


@functools.lru_cache(maxsize=None)
def status_references():
    return {name: patch_track_np(**kw) for name, kw in status_cases()}


# ---- the yardsticks themselves ---------------------------------------------------------------------------------------
def test_pyramid_of_a_constant_a_ramp_and_impulses_at_the_borders():
    for dt in (np.uint8, np.uint16, np.float32):
        c = np.full((9, 13), 77, dtype=dt)
        assert np.array_equal(pyramid_np(c), np.full((4, 6), 77, dtype=dt))
    # a ramp is reproduced away from the borders (the filter is symmetric)
    yy, xx = np.mgrid[0:12, 0:16]
    r = pyramid_np((3 * xx + 10).astype(np.float32))
    assert np.array_equal(r[:, 1:7], np.broadcast_to((6 * np.arange(1, 7) + 10).astype(np.float32), (6, 6)))
    r = pyramid_np((5 * yy + 1).astype(np.uint16))
    assert np.array_equal(r[1:5, :], np.broadcast_to((10 * np.arange(1, 5) + 1)[:, None], (4, 8)))
    # reflection, by a one-pixel impulse of 256 in row 4 (output row 2 sees it through its middle tap, 6): the first output
    # pixel has taps -2 .. 2 -> pixels 2 1 0 1 2; the last of an even width n has taps n-4 .. n -> n-4 n-3 n-2 n-1 n-2
    def response(n, pos, axis):
        w = np.zeros((n, n), dtype=np.float32)
        w[(4, pos) if axis == 1 else (pos, 4)] = 256.0
        o = pyramid_np(w)
        return (o[2, :] if axis == 1 else o[:, 2]) / 6.0
    for axis in (0, 1):
        assert [response(8, pos, axis)[0] for pos in range(4)] == [6.0, 8.0, 2.0, 0.0]          # k2 | k1 + k3 | k0 + k4
        assert [response(8, pos, axis)[3] for pos in range(3, 8)] == [0.0, 1.0, 4.0, 7.0, 4.0]  # k0 | k1 | k2 + k4 | k3
        assert [response(9, pos, axis)[3] for pos in range(3, 9)] == [0.0, 1.0, 4.0, 6.0, 4.0, 1.0]   # odd: nothing reflected
    assert [int(_reflect(np.array(i), 8)) for i in (-1, -2, 8, 9)] == [1, 2, 6, 5]
    # integers round to nearest, halves up
    u = np.zeros((8, 8), dtype=np.uint8)
    u[4, 4] = 21                          # 36 * 21 = 756 -> (756 + 128) >> 8 = 3
    assert pyramid_np(u)[2, 2] == 3 and pyramid_np(u).dtype == np.uint8
    assert pyramid_np(np.zeros((97, 129), np.uint16)).shape == (48, 64)


def test_se2_step_is_the_matrix_exponential():
    def expm(A):
        out, term = np.eye(3), np.eye(3)
        for k in range(1, 40):
            term = term @ A / k
            out = out + term
        return out
    rng = np.random.default_rng(3)
    for inc in list(rng.normal(0, 0.4, (6, 3))) + [np.array([0.3, -0.2, 1e-12]), np.array([0.1, 0.2, 0.0])]:
        t0, th0 = rng.normal(0, 5, 2), rng.uniform(-3, 3)
        T = np.array([[np.cos(th0), -np.sin(th0), t0[0]], [np.sin(th0), np.cos(th0), t0[1]], [0, 0, 1]])
        G = np.array([[0, -inc[2], inc[0]], [inc[2], 0, inc[1]], [0, 0, 0]])
        T1 = T @ expm(G)
        t1, th1 = se2_step_np(t0, th0, inc)
        assert np.allclose(t1, T1[:2, 2], rtol=0, atol=1e-13) and np.allclose([np.cos(th1), np.sin(th1)], T1[:2, 0], atol=1e-13)


def test_template_gain_against_linalg_solve():
    fx = main_fixture()
    for l in range(LEVELS):
        img = fx["p1"][l][0].astype(np.float64)
        tm = template_np(img, fx["pts"][3] / (1 << l), patches.PATTERN52)
        assert tm["status"] == patches.PATCH_OK and tm["n"] == 52 and tm["kappa"] < 1e4
        # J from the definition, once more
        p = fx["pts"][3] / (1 << l) + patches.PATTERN52
        d, gx, gy = interp_grad_np(img, p[:, 0], p[:, 1])
        S, n = d.sum(), 52
        g = n * (np.stack([gx, gy], 1) * S - np.array([gx.sum(), gy.sum()]) * d[:, None]) / (S * S)
        J = np.column_stack([g, -patches.PATTERN52[:, 1] * g[:, 0] + patches.PATTERN52[:, 0] * g[:, 1]])
        K = np.linalg.solve(J.T @ J, J.T).T
        assert np.allclose(tm["K"], K, rtol=1e-9, atol=1e-12 * np.abs(K).max())
        assert np.allclose(tm["data"], d * n / S, rtol=1e-14) and abs(tm["data"].mean() - 1.0) < 1e-12


def test_the_pyramid_does_the_work_on_the_main_fixture():
    fx, ref = main_fixture(), main_reference()
    err3 = np.hypot(*(ref["pts"] - fx["truth"]).T)
    one = patch_track_np(fx["p1"][:1], fx["p2"][:1], fx["pts"], fx["offsets"])
    err1 = np.hypot(*(one["pts"] - fx["truth"]).T)
    print(f"median error against the truth: three levels {np.median(err3):.4f} px, level 0 alone {np.median(err1):.3f} px; "
          f"statuses {np.bincount(ref['status'], minlength=5)}; kappa up to {ref['kappa'].max():.3g}; angle error "
          f"{np.median(np.abs(ref['angle'] - TRUE_ANGLE)):.2e} rad")
    # (the displacement is 6.5 px: a tracker that stays near its start errs by pixels, one that follows by a fraction of one)
    assert np.median(err3) < 0.5 < 2.0 < np.median(err1)
    assert (ref["status"] == OK).sum() >= 30 and ref["kappa"].min() >= 1 and ref["kappa"].max() < 1e6
    assert np.all(ref["dist2"][ref["status"] == OK] < 0.04)
    # the iteration is not chaotic: a start moved by 1e-11 px ends within the comparison's bound, on every keypoint
    moved = patch_track_np(fx["p1"], fx["p2"], fx["pts"], fx["offsets"], init_pts=fx["pts"] + 1e-11)
    assert np.array_equal(moved["status"], ref["status"])
    assert np.max(np.abs(moved["pts"] - ref["pts"])) < 1e-10
    # nor does it amplify the rounding of its own sums: with the pattern in reverse order (the same set of points, every
    # sum in another order) forward and backward results stay far inside the comparison's bound, so device and numpy can
    # be compared on ALL keypoints.  (A fixture with a track that wanders fails here: its backward result moved by
    # thousands of bounds.)
    rev = patch_track_np(fx["p1"], fx["p2"], fx["pts"], fx["offsets"], pattern=patches.PATTERN52[::-1])
    bound = 2.0 * ref["kappa"] * TOL
    assert np.array_equal(rev["status"], ref["status"])
    assert np.max(np.abs(rev["pts"] - ref["pts"]).max(1) / bound) < 0.01
    assert np.max(np.abs(rev["rec"] - ref["rec"]).max(1) / bound) < 0.01


def test_the_status_fixture_covers_every_status_and_level_and_sits_on_no_edge():
    refs = status_references()
    seen = set()
    for name, r in refs.items():
        seen |= set(zip(r["status"].tolist(), r["lost_level"].tolist()))
        # no decision within 1e-6 of its threshold: bounds of every pattern point and transform, dist2
        assert r["edge"].min() > 1e-6, (name, r["edge"].min())
        print(name, r["status"], r["lost_level"])
    want = {(OK, -1), (FAR, -1)} | {(s, l) for s in (BAD, LOSTF, LOSTB) for l in range(LEVELS)}
    assert want <= seen, want - seen
    a, d = refs["forward"], refs["strict"]
    assert np.all(d["status"][a["status"] == OK] == FAR) and (a["status"] == OK).sum() >= 1
    assert np.array_equal(d["status"][a["status"] != OK], a["status"][a["status"] != OK])
    assert np.all(refs["one point"]["status"] == BAD) and np.all(refs["one point"]["lost_level"] == LEVELS - 1)
    assert (refs["backward"]["status"] == LOSTB).sum() >= 6
    # (the counts themselves are integers: m <= n_pattern / 2 cannot be near its threshold without a point being near a bound)
    assert main_reference()["edge"].min() > 1e-6


# ---- the ABI ---------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_bound_and_exported_within_abi_8():
    for name, n_args in (("pnec_hip_image_pyramid_level", 11), ("pnec_hip_patch_track", 33)):
        assert name in capi.SYMBOLS
        L = capi.lib()
        assert getattr(L, name) is not None and len(getattr(L, name).argtypes) == n_args
    assert capi.ABI_VERSION == 8 and L.pnec_hip_abi_version() == 8
    header = open(os.path.join(ROOT, "include", "pnec_hip.h")).read()
    assert "#define PNEC_HIP_ABI_VERSION 8" in header
    for words in ("int pnec_hip_image_pyramid_level(const void *in, void *out, int pixel_type",
                  "int pnec_hip_patch_track(const void *const *tmpl, const int64_t *tmpl_pitch", "#define PNEC_HIP_TRACK_MAX_LEVELS 8",
                  "#define PNEC_HIP_TRACK_NO_BACKWARD 1u", "ALL ARITHMETIC IS DOUBLE", "(sum + 128) >> 8", "T <- T exp(inc)",
                  "m <= n_pattern / 2", "dist2 < max_recovered_dist2"):
        assert words in header, words
    for value, name in enumerate(("OK", "BAD_TEMPLATE", "LOST_FORWARD", "LOST_BACKWARD", "RECOVERED_TOO_FAR")):
        assert f"PNEC_HIP_TRACK_{name} = {value}" in header and getattr(patches, f"TRACK_{name}") == value
    assert patches.TRACK_NO_BACKWARD == 1 and patches.TRACK_MAX_LEVELS == 8


def test_bad_arguments_are_refused_before_a_device_is_touched():
    L = capi.lib()
    img = [np.zeros((96 >> l, 128 >> l), dtype=np.uint8) for l in range(4)]       # level 3 is 12 x 16
    ptr = lambda n=3: (C.c_void_p * 9)(*([a.ctypes.data for a in img[:min(n, 4)]] + [img[3].ctypes.data] * (9 - min(n, 4))))
    pit = lambda first=128: (C.c_int64 * 9)(*([first, 64, 32, 16] + [16] * 5))
    offs = np.array([0, 2], dtype=np.int64)
    pts = np.array([[40.0, 40.0], [60.0, 50.0]])
    pat = np.ascontiguousarray(np.tile(patches.PATTERN52, (2, 1)))
    SENT = -7.25
    o_pts, o_ang, o_cov, o_d2 = np.full((2, 2), SENT), np.full(2, SENT), np.full((2, 3), SENT), np.full(2, SENT)
    o_st, o_lv = (np.full(2, -5, dtype=np.int32) for _ in range(2))
    outs = tuple(a.ctypes.data for a in (o_pts, o_ang, o_cov, o_d2, o_st, o_lv))

    def call(tmpl=ptr(), tq=pit(), prev=None, pq=None, nxt=ptr(), nq=pit(), levels=3, ptype=0, F=1, h=96, w=128,
             offsets=offs.ctypes.data, M=2, tp=pts.ctypes.data, pattern=pat.ctypes.data, n_pat=52, iters=40, d2=0.04, flags=0,
             scaling=10.0, outputs=outs, space=capi.MEM_HOST):
        rc = L.pnec_hip_patch_track(tmpl, tq, prev, pq, nxt, nq, levels, ptype, F, h, w, offsets, M, tp, None, None, 0.0,
                                    0.0, pattern, n_pat, iters, d2, flags, scaling, *outputs, space, 0, None)
        return rc, (L.pnec_hip_last_error() or b"").decode()
    holes = ptr()
    holes[1] = None
    for kw, word in ((dict(tmpl=None), "NULL"), (dict(nxt=None), "NULL"), (dict(tq=None), "NULL"), (dict(nq=None), "NULL"),
                     (dict(offsets=None), "NULL"), (dict(tp=None), "NULL"), (dict(pattern=None), "NULL"),
                     (dict(tmpl=holes), "level pointer"), (dict(outputs=(None,) * 6), "output"),
                     (dict(levels=0), "n_levels"), (dict(levels=9), "n_levels"), (dict(iters=0), "max_iterations"),
                     (dict(iters=256), "max_iterations"), (dict(n_pat=0), "n_pattern"), (dict(n_pat=65), "n_pattern"),
                     (dict(tq=pit(127)), "pitch"), (dict(nq=pit(100)), "pitch"),
                     (dict(levels=6, tmpl=ptr(6), nxt=ptr(6)), "below 4 pixels"), (dict(h=7, w=128, levels=2), "below 4 pixels"),
                     (dict(d2=-1e-9), "max_recovered_dist2"), (dict(d2=float("nan")), "max_recovered_dist2"),
                     (dict(ptype=3), "pixel_type"), (dict(flags=2), "flags"), (dict(F=0), "n_images"), (dict(M=-1), "n_points"),
                     (dict(scaling=0.0), "scaling"), (dict(space=5), "memory space"), (dict(M=3), "offsets")):
        rc, msg = call(**kw)
        assert rc == capi.ERR_INVALID_ARGUMENT == -1, (kw, rc, msg)
        assert "patch_track" in msg and word in msg, (kw, msg)
    rc, msg = call(levels=9, space=capi.MEM_DEVICE)
    assert rc == -1 and "n_levels" in msg
    assert all(np.all(a == SENT) for a in (o_pts, o_ang, o_cov, o_d2)) and np.all(o_st == -5) and np.all(o_lv == -5)
    rc, msg = call(M=0, offsets=np.array([0, 0], dtype=np.int64).ctypes.data)
    assert rc == 0, msg

    src, dst = np.zeros((8, 12), dtype=np.uint8), np.full((4, 6), 9, dtype=np.uint8)

    def pyr(a=src.ctypes.data, b=dst.ctypes.data, ptype=0, F=1, h=8, w=12, pin=12, pout=6, space=capi.MEM_HOST):
        rc = L.pnec_hip_image_pyramid_level(a, b, ptype, F, h, w, pin, pout, space, 0, None)
        return rc, (L.pnec_hip_last_error() or b"").decode()
    for kw, word in ((dict(a=None), "NULL"), (dict(b=None), "NULL"), (dict(ptype=5), "pixel_type"), (dict(F=0), "n_images"),
                     (dict(h=3), "height"), (dict(w=3), "width"), (dict(pin=11), "pitch"), (dict(pout=5), "pitch"),
                     (dict(space=7), "memory space")):
        rc, msg = pyr(**kw)
        assert rc == -1 and "image_pyramid_level" in msg and word in msg, (kw, rc, msg)
    assert np.all(dst == 9)


def test_python_facade_and_pybind_expose_the_new_names():
    import dataclasses
    import inspect
    assert {"patch_track", "PatchTrack", "image_pyramid"} <= set(pnec_amd.__all__)
    assert pnec_amd.patch_track is patches.patch_track and pnec_amd.image_pyramid is patches.image_pyramid
    assert [f.name for f in dataclasses.fields(pnec_amd.PatchTrack)][:6] == ["pts", "angle", "cov", "dist2", "status", "lost_level"]
    sig = inspect.signature(patches.patch_track)
    assert list(sig.parameters)[:4] == ["tmpl", "next", "tmpl_pts", "offsets"]
    assert sig.parameters["max_iterations"].default == 40 and sig.parameters["max_recovered_dist2"].default == 0.04
    assert sig.parameters["scaling"].default == 10.0 and sig.parameters["pattern"].default is patches.PATTERN52
    assert list(inspect.signature(patches.image_pyramid).parameters) == ["images", "levels"]
    with pytest.raises(ValueError):
        patches.image_pyramid(np.zeros((16, 16), dtype=np.uint8), 0)
    with pytest.raises(TypeError):
        patches.image_pyramid(np.zeros((16, 16), dtype=np.float64), 2)
    import pnec_amd.pypnec as pypnec
    assert "patch_track" in dir(pypnec) and "image_pyramid" in dir(pypnec)
    facade = open(os.path.join(ROOT, "pnec_amd", "csrc", "host", "pnec_host.h")).read()
    assert "ImagePyramid(" in facade and "TrackPatches(" in facade
    with open(os.path.join(ROOT, "pnec_amd", "libpnec_host.so"), "rb") as f:
        blob = f.read()
    assert b"ImagePyramid" in blob and b"TrackPatches" in blob


# ---- the kernel's arithmetic on the host, under the sanitizers -------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _host_program():
    import tempfile
    gxx = shutil.which("g++")
    assert gxx, "g++ builds the host facade, so it is there"
    exe = os.path.join(tempfile.mkdtemp(prefix="patch_track_host_"), "patch_track_host")
    subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "pnec_amd", "csrc"),
                    os.path.join(ROOT, "tools", "patch_track_host.cc"), "-o", exe], check=True)
    return exe


ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


def run_host_track(tmp_path, tmpl, next, tmpl_pts, offsets=None, prev=None, init_pts=None, init_angle=None, shift=(0.0, 0.0),
                   pattern=patches.PATTERN52, max_iterations=40, max_recovered_dist2=0.04, backward=True, scaling=10.0,
                   pad=0):
    """writes the job (every level with rows `pad` pixels longer than the image, the last row not padded), runs the
    sanitized host build, returns its outputs as a dict"""
    dt = np.asarray(tmpl[0]).dtype
    ptype = {"uint8": 0, "uint16": 1, "float32": 2}[dt.name]
    F, h, w = np.asarray(tmpl[0]).shape
    L, M = len(tmpl), len(tmpl_pts)
    offsets = np.array([0, M], dtype=np.int64) if offsets is None else offsets
    pattern = np.ascontiguousarray(pattern, dtype=np.float64)
    blob = [np.array([ptype, F, h, w, L, M, len(pattern), max_iterations, 0 if backward else 1, prev is not None,
                      init_pts is not None, init_angle is not None], dtype=np.int64).tobytes(),
            np.array([shift[0], shift[1], max_recovered_dist2, scaling], dtype=np.float64).tobytes()]
    pitches = np.array([[(w >> l) + pad for l in range(L)]] * 3, dtype=np.int64)
    blob += [pitches.tobytes(), np.ascontiguousarray(offsets, dtype=np.int64).tobytes(),
             np.ascontiguousarray(tmpl_pts, dtype=np.float64).tobytes()]
    if init_pts is not None:
        blob.append(np.ascontiguousarray(init_pts, dtype=np.float64).tobytes())
    if init_angle is not None:
        blob.append(np.ascontiguousarray(init_angle, dtype=np.float64).tobytes())
    blob.append(pattern.tobytes())
    for pyr in (tmpl, prev, next):
        if pyr is None:
            continue
        for l, lv in enumerate(pyr):
            lv = np.asarray(lv)
            buf = np.full((F * (h >> l), (w >> l) + pad), 255 if dt != np.float32 else -1.0e6, dtype=dt)
            buf[:, :w >> l] = lv.reshape(F * (h >> l), w >> l)
            blob.append(buf.reshape(-1)[: buf.size - pad].tobytes())
    (tmp_path / "job.bin").write_bytes(b"".join(blob))
    r = subprocess.run([_host_program(), "track", str(tmp_path / "job.bin"), str(tmp_path / "out.bin")], env=ENV,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "without slack" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    o = np.frombuffer((tmp_path / "out.bin").read_bytes(), dtype=np.float64).reshape(-1, 9)
    return dict(pts=o[:, :2], angle=o[:, 2], cov=o[:, 3:6], dist2=o[:, 6], status=o[:, 7].astype(np.int32),
                lost_level=o[:, 8].astype(np.int32))


def test_the_trackers_arithmetic_built_for_the_host_reads_no_pixel_outside_and_meets_the_gpu_bounds(tmp_path):
    fx, ref = main_fixture(), main_reference()
    results = {}
    for name, conv, pad in (("uint8", lambda a: a, 0), ("uint16 << 8", lambda a: a.astype(np.uint16) << 8, 3),
                            ("float32", lambda a: a.astype(np.float32), 5)):
        got = run_host_track(tmp_path, [conv(a) for a in fx["p1"]], [conv(a) for a in fx["p2"]], fx["pts"], fx["offsets"],
                             pad=pad)
        check_track_against_np(got, ref, f"host build, main fixture, {name}")
        ok = ref["status"] == OK
        assert np.all(np.isnan(got["cov"][~ok])) and np.allclose(got["cov"][ok], ref["cov"][ok], rtol=1e-6)
        results[name] = got
    for name in ("uint16 << 8", "float32"):       # the same values in another pixel type: the same bits
        for key in ("pts", "angle", "cov", "dist2"):
            assert np.array_equal(results["uint8"][key], results[name][key], equal_nan=True), (name, key)
    fwd = run_host_track(tmp_path, fx["p1"], fx["p2"], fx["pts"], fx["offsets"], backward=False)
    assert np.array_equal(fwd["pts"], results["uint8"]["pts"]) and np.array_equal(fwd["angle"], results["uint8"]["angle"])
    for name, kw in status_cases():
        got = run_host_track(tmp_path, **kw)
        check_track_against_np(got, status_references()[name], f"host build, status fixture '{name}'")


def test_the_pyramids_arithmetic_built_for_the_host_reads_no_pixel_outside_and_equals_numpy(tmp_path):
    rng = np.random.default_rng(5)
    for typ, dt in (("u8", np.uint8), ("u16", np.uint16), ("f32", np.float32)):
        for h, w, pin, pout in ((96, 128, 128, 64), (97, 129, 133, 70), (4, 4, 4, 2), (5, 7, 9, 3)):
            img = (rng.random((h, w)) * (255 if dt == np.uint8 else 65535)).astype(dt)
            buf = np.zeros((h, pin), dtype=dt)
            buf[:, :w] = img
            (tmp_path / "in.bin").write_bytes(buf.reshape(-1)[: (h - 1) * pin + w].tobytes())
            r = subprocess.run([_host_program(), "pyr", typ, str(h), str(w), str(pin), str(pout), str(tmp_path / "in.bin"),
                                str(tmp_path / "out.bin")], env=ENV, capture_output=True, text=True)
            assert r.returncode == 0, r.stderr[-3000:]
            assert "without slack" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
            flat = np.frombuffer((tmp_path / "out.bin").read_bytes(), dtype=dt)
            out = np.concatenate([flat, np.zeros(pout - w // 2, dtype=dt)]).reshape(h // 2, pout)[:, : w // 2]
            assert np.array_equal(out, pyramid_np(img)), (typ, h, w)
