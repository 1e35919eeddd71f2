"""The checker of pnec_hip_undistort_keypoints and the fixtures of its tests.

undistort_np restates the six steps of include/pnec_hip.h in numpy, one rounded operation after the other in the order
the header writes them, for all points at once; it runs in float64 (the yardstick of the device, which forms no fused
multiply-add either) and in numpy.longdouble (the yardstick of the yardstick: the distance of the two is the rounding
error a correct float64 implementation may show).  No GPU here.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

OK, OUTSIDE, NOT_CONVERGED, NOT_FINITE = 0, 1, 2, 3
NEWTON, PROPAGATE_COV = 1, 2
STOP = 2.0 ** -46

# fx fy cx cy k1 k2 p1 p2 k3
EUROC = np.array([458.654, 457.296, 367.215, 248.375, -0.28340811, 0.07395907, 0.00019359, 1.76187114e-05, 0.0])
TUM = np.array([517.3, 516.5, 318.6, 255.3, 0.2624, -0.9531, -0.0054, 0.0026, 1.1633])
MILD = np.array([700.0, 700.0, 320.0, 240.0, -0.05, 0.01, 1e-3, -5e-4, 0.0])
CAMERAS = {"euroc": (EUROC, 752, 480), "tum": (TUM, 640, 480), "mild": (MILD, 640, 480)}
# normalised units: K = I, radial only; the model folds at x = 0.7027 (1 - 0.9 x^2 = 0 at x = 1.054 undistorted)
UNIT = np.array([1.0, 1.0, 0.0, 0.0, -0.3, 0.0, 0.0, 0.0, 0.0])


def grid(width, height, nx=97, ny=61):
    """nx x ny points over the image, corners included: [nx * ny, 2]"""
    u, v = np.meshgrid(np.linspace(0.0, width - 1.0, nx), np.linspace(0.0, height - 1.0, ny))
    return np.stack([u.ravel(), v.ravel()], axis=1)


def forward(cam, x, y, jacobian=False):
    """distort(x, y) in normalised coordinates, and J = (j00, j01, j10, j11)"""
    fx, fy, cx, cy, k1, k2, p1, p2, k3 = cam
    xx, yy, xy = x * x, y * y, x * y
    r2 = xx + yy
    cdist = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
    a1, a2, a3 = 2 * xy, r2 + 2 * xx, r2 + 2 * yy
    xd = x * cdist + (p1 * a1 + p2 * a2)
    yd = y * cdist + (p1 * a3 + p2 * a1)
    if not jacobian:
        return xd, yd
    dc = (3 * k3 * r2 + 2 * k2) * r2 + k1
    cross = 2 * xy * dc + (2 * p1 * x + 2 * p2 * y)
    j00 = cdist + 2 * xx * dc + (2 * p1 * y + 6 * p2 * x)
    j11 = cdist + 2 * yy * dc + (6 * p1 * y + 2 * p2 * x)
    return xd, yd, (j00, cross, cross, j11)


@dataclass
class Result:
    pts: np.ndarray      # [n,2]
    cov: np.ndarray      # [n,3] or None
    status: np.ndarray   # uint8 [n]
    steps: np.ndarray    # Newton steps taken per point
    outside_at: np.ndarray  # the fixed-point step (1-based) that found icdist < 0, 0 where none did
    residual: np.ndarray    # the forward residual rho of the returned point, normalised units


def undistort_np(camera, pts, cov=None, fixed_iterations=5, newton_iterations=20, flags=0, dtype=np.float64):
    """One side of pnec_hip_undistort_keypoints: pts [n,2] and their cov [n,3] or None."""
    T = dtype
    cam = np.asarray(camera, dtype=np.float64).astype(T)
    fx, fy, cx, cy, k1, k2, p1, p2, k3 = cam
    pts64 = np.asarray(pts, dtype=np.float64).reshape(-1, 2)
    n = pts64.shape[0]
    cov64 = None if cov is None else np.asarray(cov, dtype=np.float64).reshape(-1, 3)
    zeros = np.zeros(n, dtype=np.int64)
    if k1 == 0 and k2 == 0 and p1 == 0 and p2 == 0 and k3 == 0:   # step 6
        return Result(pts64.astype(T), None if cov64 is None else cov64.astype(T), np.zeros(n, np.uint8), zeros, zeros,
                      np.zeros(n, T))
    with np.errstate(all="ignore"):
        u, v = pts64[:, 0].astype(T), pts64[:, 1].astype(T)
        finite = np.isfinite(u) & np.isfinite(v)
        x0, y0 = (u - cx) / fx, (v - cy) / fy                                     # 1
        x, y = x0.copy(), y0.copy()
        outside = np.zeros(n, bool)
        outside_at = zeros.copy()
        for it in range(int(fixed_iterations)):                                   # 2
            xx, yy, xy = x * x, y * y, x * y
            r2 = xx + yy
            icdist = 1 / (1 + ((k3 * r2 + k2) * r2 + k1) * r2)
            first = ~outside & (icdist < 0)
            outside_at[first] = it + 1
            outside |= first
            a1, a2, a3 = 2 * xy, r2 + 2 * xx, r2 + 2 * yy
            dx, dy = p1 * a1 + p2 * a2, p1 * a3 + p2 * a1
            x = np.where(outside, x0, (x0 - dx) * icdist)
            y = np.where(outside, y0, (y0 - dy) * icdist)
        status = np.where(outside, OUTSIDE, OK).astype(np.uint8)
        steps = zeros.copy()
        if flags & NEWTON:                                                        # 3
            n0 = np.sqrt(x0 * x0 + y0 * y0)
            bound = T(STOP) * np.where(n0 > 1, n0, T(1))
            xn, yn = x.copy(), y.copy()
            ended, converged = ~finite | outside, np.zeros(n, bool)
            it = 0
            while True:
                xd, yd, (j00, j01, j10, j11) = forward(cam, xn, yn, True)
                e0, e1 = xd - x0, yd - y0
                rho = np.sqrt(e0 * e0 + e1 * e1)
                stop = ~ended & (rho <= bound)
                converged |= stop
                ended |= stop
                if it >= int(newton_iterations):
                    break
                det = j00 * j11 - j01 * j10
                ended |= (det == 0) | ~np.isfinite(det)
                sx, sy = (j11 * e0 - j01 * e1) / det, (j00 * e1 - j10 * e0) / det
                steps += ~ended
                xn = np.where(ended, xn, xn - sx)
                yn = np.where(ended, yn, yn - sy)
                it += 1
            x, y = np.where(converged, xn, x), np.where(converged, yn, y)
            status[~outside & ~converged] = NOT_CONVERGED
        ou, ov = fx * x + cx, fy * y + cy                                         # 4
        ou[~finite] = np.nan
        ov[~finite] = np.nan
        status[~finite] = NOT_FINITE
        xd, yd, (j00, j01, j10, j11) = forward(cam, x, y, True)
        residual = np.sqrt((xd - x0) ** 2 + (yd - y0) ** 2)
        out_cov = None
        if cov64 is not None:                                                     # 5
            sxx, sxy, syy = (cov64[:, k].astype(T) for k in range(3))
            out_cov = np.stack([sxx, sxy, syy], axis=1)
            if flags & PROPAGATE_COV:
                det = j00 * j11 - j01 * j10
                a00, a01 = j11 / det, -j01 / det * fx / fy
                a10, a11 = -j10 / det * fy / fx, j00 / det
                m00, m01 = a00 * sxx + a01 * sxy, a00 * sxy + a01 * syy
                m10, m11 = a10 * sxx + a11 * sxy, a10 * sxy + a11 * syy
                carry = (status == OK) & (det != 0) & np.isfinite(det)
                new = np.stack([m00 * a00 + m01 * a01, m00 * a10 + m01 * a11, m10 * a10 + m11 * a11], axis=1)
                out_cov = np.where(carry[:, None], new, out_cov)
    return Result(np.stack([ou, ov], axis=1), out_cov, status, steps, outside_at, residual)


def distort_pixels(camera, pts):
    """The forward model in pixels: where the ideal pinhole pixel `pts` [n,2] lands in the raw image (float64)."""
    fx, fy, cx, cy = camera[:4]
    xd, yd = forward(camera, (pts[:, 0] - cx) / fx, (pts[:, 1] - cy) / fy)
    return np.stack([fx * xd + cx, fy * yd + cy], axis=1)


# the status cases, normalised units, camera UNIT: (x, y), flags, the status, and what else is known of them
STATUS_CASES = [
    ((2.0, 0.0), 0, OUTSIDE),             # icdist < 0 at the first step
    ((0.9, 0.0), 0, OUTSIDE),             # ... at the fourth
    ((0.71, 0.0), NEWTON, NOT_CONVERGED),  # beyond the fold at 0.7027: no preimage
    ((0.70, 0.0), NEWTON, OK),            # x = 1.0 exactly: 1.0 (1 - 0.3) = 0.7
]


def random_cov(n, seed):
    """n positive definite 2x2 covariances as (xx, xy, yy), standard deviations of 0.1 .. 1 px"""
    rng = np.random.default_rng(seed)
    s1, s2 = rng.uniform(0.1, 1.0, n), rng.uniform(0.1, 1.0, n)
    th = rng.uniform(0.0, np.pi, n)
    c, s = np.cos(th), np.sin(th)
    return np.stack([c * c * s1 ** 2 + s * s * s2 ** 2, c * s * (s1 ** 2 - s2 ** 2), s * s * s1 ** 2 + c * c * s2 ** 2], axis=1)


def spread(camera_name, n, seed):
    """n points spread over the camera's image (a little beyond its border too), with covariances"""
    cam, w, h = CAMERAS[camera_name]
    rng = np.random.default_rng(seed)
    pts = np.stack([rng.uniform(-8.0, w + 8.0, n), rng.uniform(-8.0, h + 8.0, n)], axis=1)
    return pts, random_cov(n, seed + 1)
