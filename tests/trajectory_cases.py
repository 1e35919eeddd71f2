"""The numpy checker of the trajectory calls and the trajectories their tests share.

compose_np and metrics_np are pnec_hip_trajectory_compose and pnec_hip_trajectory_metrics written operation by operation
from include/pnec_hip.h, in float64 or np.longdouble (`dtype`); compose_np is the sequential product the header defines.
traj(L, noise, seed, step) builds a ground-truth trajectory and a noisy estimate of it; the golden file
(tests/golden/make_trajectory_golden.py) records the reference's five metrics on five of them.

The bounds are the header's, derived for FP64 with u = 2^-53 (a product of unit quaternions errs by about 4 u a step under
any association order); none of them is measured.
"""
from collections import namedtuple

import numpy as np

U = 2.0 ** -53
METRICS = ("RPE_1", "RPE_n", "L1RPE_1", "L1RPE_n", "r_t")

# the golden's trajectories: (L, noise, step, seed)
GOLDEN_CASES = ((2, 1e-2, 0.05, 11), (3, 1e-2, 0.05, 12), (65, 1e-2, 0.05, 13), (130, 1e-3, 0.05, 14), (257, 5e-3, 0.02, 15))


# ---------------------------------------------------------------------------------------------------- the bounds
def bound_compose_q(L):
    return 8.0 * (L + 2) * U


def bound_compose_p(L, path):
    return 16.0 * (L + 2) * U * path


BOUND_ERR_Q = 16.0 * U


def bound_angle(angle):
    return 64.0 * U + 8.0 * U * np.abs(angle)


def bound_distance(L, d, value):
    return 64.0 * U + (L - d + 8) * U * np.abs(value)


def bound_n(L, value):
    return 64.0 * U + (2 * L + 8) * U * np.abs(value)


def bound_metrics(L, m):
    """the bounds of the five metrics of one sequence (m [5]): RPE_1 and L1RPE_1 are rmse_1 / l1_1, r_t a mean of L - 1
    angles"""
    m = np.abs(np.asarray(m, dtype=np.float64))
    return np.array([bound_distance(L, 1, m[0]), bound_n(L, m[1]), bound_distance(L, 1, m[2]), bound_n(L, m[3]),
                     bound_distance(L, 1, m[4])])


# ---------------------------------------------------------------------------------------------------- quaternions
def qmul(a, b):
    """Hamilton product, xyzw, [...,4]; the vector part in pairs that cancel exactly for b = conj(a)"""
    ax, ay, az, aw = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    bx, by, bz, bw = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    return np.stack([(aw * bx + ax * bw) + (ay * bz - az * by), (aw * by + ay * bw) + (az * bx - ax * bz),
                     (aw * bz + az * bw) + (ax * by - ay * bx), (aw * bw - ax * bx) - (ay * by + az * bz)], axis=-1)


def qconj(q):
    return q * np.array([-1, -1, -1, 1], dtype=q.dtype)


def qnorm(q):
    with np.errstate(invalid="ignore", divide="ignore"):
        return q / np.sqrt((q * q).sum(axis=-1, keepdims=True))


def qrot(q, v):
    """R(q) v: v + w t + u x t, t = 2 (u x v)"""
    u = q[..., :3]
    t = 2 * np.cross(u, v)
    return v + q[..., 3:4] * t + np.cross(u, t)


def qexp(w, dtype=np.longdouble):
    """exp of the rotation vectors w [...,3]"""
    w = np.asarray(w, dtype=dtype)
    th = np.sqrt((w * w).sum(axis=-1, keepdims=True))
    half = th / 2
    k = np.where(th > 0, np.sin(half) / np.where(th > 0, th, 1), dtype(0.5))
    return np.concatenate([k * w, np.cos(half)], axis=-1)


def qmat(q):
    """the rotation matrix of unit quaternions [...,4] -> [...,3,3]"""
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], axis=-1),
                     np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], axis=-1),
                     np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], axis=-1)], axis=-2)


def cut(offsets, f, n_rows):
    lo = min(max(int(offsets[f]), 0), n_rows)
    hi = min(max(int(offsets[f + 1]), lo), n_rows)
    return lo, hi


# ---------------------------------------------------------------------------------------------------- compose
Composed = namedtuple("Composed", "q p valid")


def compose_np(offsets, rel_q, rel_t=None, scale=None, q0=None, p0=None, dtype=np.float64, fill=np.nan):
    """pnec_hip_trajectory_compose, the sequential form.  Rows of no sequence hold `fill` (valid: 255)."""
    rel_q = np.asarray(rel_q, dtype=dtype).reshape(-1, 4)
    n = rel_q.shape[0]
    n_seq = len(offsets) - 1
    pos = rel_t is not None
    t_all = np.asarray(rel_t, dtype=dtype).reshape(-1, 3) if pos else None
    out_q = np.full((n, 4), fill, dtype=dtype)
    out_p = np.full((n, 3), fill, dtype=dtype) if pos else None
    valid = np.full(n, 255, dtype=np.uint8)
    for f in range(n_seq):
        lo, hi = cut(offsets, f, n)
        q = np.array([0, 0, 0, 1], dtype=dtype) if q0 is None else qnorm(np.asarray(q0, dtype=dtype)[f])
        p = np.zeros(3, dtype=dtype) if p0 is None else np.asarray(p0, dtype=dtype)[f].copy()
        for r in range(lo, hi):
            sq = rel_q[r]
            n2 = (sq * sq).sum()
            present = bool(np.isfinite(sq).all() and np.isfinite(n2) and n2 > 0)
            st = np.zeros(3, dtype=dtype)
            if pos:
                st = t_all[r]
                present = present and bool(np.isfinite(st).all())
                if scale is not None:
                    sc = dtype(np.asarray(scale, dtype=dtype)[r])
                    with np.errstate(invalid="ignore", over="ignore"):
                        st = sc * st
                    present = present and bool(np.isfinite(sc)) and bool(np.isfinite(st).all())
            if present:
                if pos:
                    p = p + qrot(q, st)
                q = qmul(q, sq / np.sqrt(n2))
            out_q[r] = qnorm(q)
            if pos:
                out_p[r] = p
            valid[r] = 1 if present else 0
    return Composed(out_q, out_p, valid)


# ---------------------------------------------------------------------------------------------------- metrics
Scored = namedtuple("Scored", "metrics err_q rmse_d l1_d angle1 rt1")


def chord_angle(a, b, dtype):
    """k asin(min(1, |a - s b| / 2)) with k = 4 for quaternions and 2 for directions; s the sign of <a, b>"""
    dot = (a * b).sum(axis=-1, keepdims=True)
    s = np.where(dot >= 0, dtype(1), dtype(-1))
    d = a - s * b
    c = np.sqrt((d * d).sum(axis=-1)) / 2
    c = np.where(c > 1, dtype(1), c)
    return (4 if a.shape[-1] == 4 else 2) * np.arcsin(c)


def step_directions(q, p, lo, hi):
    g = qnorm(q[lo:hi - 1])
    u = qrot(qconj(g), p[lo + 1:hi] - p[lo:hi - 1])
    with np.errstate(invalid="ignore", divide="ignore"):
        return u / np.sqrt((u * u).sum(axis=-1, keepdims=True))


def metrics_np(offsets, est_q, gt_q, est_p=None, gt_p=None, dtype=np.float64, fill=np.nan):
    """pnec_hip_trajectory_metrics.  Rows of no sequence hold `fill` (err_q is written for every row)."""
    est_q, gt_q = np.asarray(est_q, dtype=dtype).reshape(-1, 4), np.asarray(gt_q, dtype=dtype).reshape(-1, 4)
    n = est_q.shape[0]
    n_seq = len(offsets) - 1
    pos = est_p is not None
    if pos:
        est_p, gt_p = np.asarray(est_p, dtype=dtype).reshape(-1, 3), np.asarray(gt_p, dtype=dtype).reshape(-1, 3)
    e = qnorm(qmul(qnorm(est_q), qconj(qnorm(gt_q))))
    metrics = np.full((n_seq, 5), np.nan, dtype=dtype)
    rmse_d, l1_d, angle1 = (np.full(n, fill, dtype=dtype) for _ in range(3))
    rt1 = np.full(n, fill, dtype=dtype) if pos else None
    for f in range(n_seq):
        lo, hi = cut(offsets, f, n)
        L = hi - lo
        if L >= 1:
            rmse_d[lo] = l1_d[lo] = angle1[lo] = 0
            if pos:
                rt1[lo] = 0
        if L < 2:
            continue
        for d in range(1, L):
            a = chord_angle(e[lo:hi - d], e[lo + d:hi], dtype)
            rmse_d[lo + d] = np.sqrt((a * a).sum() / dtype(L - d))
            l1_d[lo + d] = a.sum() / dtype(L - d)
        angle1[lo + 1:hi] = chord_angle(e[lo:hi - 1], e[lo + 1:hi], dtype)
        metrics[f, 0] = rmse_d[lo + 1]
        metrics[f, 1] = rmse_d[lo + 1:hi].sum() / dtype(L)
        metrics[f, 2] = l1_d[lo + 1]
        metrics[f, 3] = l1_d[lo + 1:hi].sum() / dtype(L)
        if pos:
            rt1[lo + 1:hi] = chord_angle(step_directions(gt_q, gt_p, lo, hi), step_directions(est_q, est_p, lo, hi), dtype)
            metrics[f, 4] = rt1[lo + 1:hi].sum() / dtype(L - 1)
    return Scored(metrics, e, rmse_d, l1_d, angle1, rt1)


def reference_angle(ei, ej):
    """the reference's form: arccos((trace(rel) - 1) / 2) of rel = (Est_j' Est_i)(Gt_i' Gt_j), from E = Est Gt' per frame
    (what the trace identity says it equals): float64"""
    rel = np.swapaxes(qmat(ei), -1, -2) @ qmat(ej)
    with np.errstate(invalid="ignore"):
        return np.arccos((np.trace(rel, axis1=-2, axis2=-1) - 1.0) / 2.0)


# ---------------------------------------------------------------------------------------------------- trajectories
Traj = namedtuple("Traj", "L rel_q rel_t est_q est_p gt_q gt_p")


def traj(L, noise, seed, step):
    """A trajectory of L frames.  Ground truth: rel_k = exp(N(0, step^2)) and a unit translation step; the estimate's step
    is rel_k exp(N(0, noise^2)) with the translation direction disturbed by 0.05.  Row 0 is a pose itself, like every
    other row.  rel_q, rel_t: the estimate's steps (float64); est_*, gt_*: the absolute poses, composed in long double and
    rounded to float64."""
    rng = np.random.default_rng(seed)
    w = rng.normal(0.0, step, (L, 3))
    dw = rng.normal(0.0, noise, (L, 3))
    t = rng.normal(0.0, 1.0, (L, 3))
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    te = t + 0.05 * rng.normal(0.0, 1.0, (L, 3))
    te /= np.linalg.norm(te, axis=1, keepdims=True)
    gt_rel = qexp(w)
    est_rel = qnorm(qmul(gt_rel, qexp(dw))).astype(np.float64)
    off = [0, L]
    gt = compose_np(off, gt_rel, t, dtype=np.longdouble)
    est = compose_np(off, est_rel, te, dtype=np.longdouble)
    f = lambda a: np.ascontiguousarray(a.astype(np.float64))
    return Traj(L, est_rel.reshape(L, 4), f(te).reshape(L, 3), f(est.q).reshape(L, 4), f(est.p).reshape(L, 3),
                f(gt.q).reshape(L, 4), f(gt.p).reshape(L, 3))


def concat(trajs):
    """several trajectories as one ragged set: (offsets, dict of stacked arrays)"""
    off = np.concatenate([[0], np.cumsum([t.L for t in trajs])]).astype(np.int64)
    cat = lambda name, cols: np.concatenate([getattr(t, name).reshape(-1, cols) for t in trajs]) if trajs else np.zeros((0, cols))
    return off, {name: cat(name, 4 if name.endswith("q") else 3) for name in Traj._fields[1:]}


def sign_aligned_diff(a, b):
    """|a - s b| per row with s the sign of <a, b>: quaternions compared up to sign"""
    a, b = np.asarray(a, dtype=np.longdouble), np.asarray(b, dtype=np.longdouble)
    s = np.where((a * b).sum(axis=-1, keepdims=True) >= 0, 1, -1)
    return np.sqrt(((a - s * b) ** 2).sum(axis=-1)).astype(np.float64)
