"""The numpy checkers of pnec_hip_tracks_link and pnec_hip_trajectory_advance and the cases their tests share.

link_np is the header's bisection, literally, image by image.  advance_np is one step of the header's definition written
operation by operation, in float64 or np.longdouble (`dtype`); with `status` given it takes the decisions as made and only
does the arithmetic, which is how the exact form follows a float64 run.  The bounds are the header's (DESIGN.md 9r has
the derivation); none of them is measured.
"""
import numpy as np

from trajectory_cases import U, qmul, qnorm, qrot

MEASURED, HELD, STARTED, ABSENT = 0, 1, 2, 3
LINK_SIZES = (0, 1, 2, 63, 64, 65, 257)      # per-image counts: around a wavefront, and more than a block of 256 rows


def bound_advance_q(L):
    return 12.0 * (L + 2) * U


def bound_advance_p(L, path):
    return 26.0 * (L + 2) * U * path


# ---------------------------------------------------------------------------------------------------- tracks_link
def cut(offsets, f, rows):
    lo = min(max(int(offsets[f]), 0), rows)
    hi = min(max(int(offsets[f + 1]), lo), rows)
    return lo, hi


def find_np(prev_id, plo, Lp, ident):
    """the lower bound of `ident` among prev_id[plo : plo + Lp] by the header's bisection; the row, or -1"""
    ident = int(ident)
    if ident < 0:
        return -1
    a, b = 0, Lp
    while a < b:
        m = a + (b - a) // 2
        if int(prev_id[plo + m]) < ident:
            a = m + 1
        else:
            b = m
    return a if a < Lp and int(prev_id[plo + a]) == ident else -1


def link_np(cur_offsets, cur_id, prev_offsets, prev_id):
    """pnec_hip_tracks_link: (link int32 [n_cur], n_linked int32 [F]); rows of no image get -1"""
    cur_id, prev_id = np.asarray(cur_id, dtype=np.int64), np.asarray(prev_id, dtype=np.int64)
    F, n, m = len(cur_offsets) - 1, len(cur_id), len(prev_id)
    link = np.full(n, -1, dtype=np.int32)
    n_linked = np.zeros(F, dtype=np.int32)
    for f in range(F):
        lo, hi = cut(cur_offsets, f, n)
        plo, phi = cut(prev_offsets, f, m)
        for k in range(lo, hi):
            link[k] = find_np(prev_id, plo, phi - plo, cur_id[k])
        n_linked[f] = int((link[lo:hi] >= 0).sum())
    return link, n_linked


BIG = 1 << 32


def id_case(n_prev, n_cur, rng):
    """(prev ids, cur ids) of one image.  The previous ids ascend strictly, lie above 2^32 in part, and two of them agree in
    their low 32 bits; the current ids hold the previous set's first and last id, ids absent below, between and above, a
    negative id, and an id that agrees with a previous one in the low 32 bits only."""
    if n_prev:
        gaps = rng.integers(2, 9, n_prev).astype(np.int64)      # gaps >= 2: there are absent ids in between
        prev = 5 + np.cumsum(gaps)
        prev[n_prev // 2:] += BIG                                # the upper half lies above 2^32 ...
        if n_prev >= 2:
            prev[n_prev // 2] = prev[0] + BIG                    # ... its first with the low word of the set's first id
    else:
        prev = np.zeros(0, dtype=np.int64)
    special = [-3, 0, 4]                                         # negative; absent below (the previous ids start above 5)
    if n_prev:
        # the first and the last row; absent between and above; absent with the low word of a present id, both ways
        special += [int(prev[0]), int(prev[-1]), int(prev[-1]) + 1, int(prev[0]) + 1, int(prev[0]) + 2 * BIG,
                    int(prev[-1]) + BIG]
        if n_prev >= 2:
            special += [int(prev[-1]) - BIG, int(prev[n_prev // 2])]
    take = rng.permutation(n_prev)[:max(0, n_cur // 2)]
    pool = np.concatenate([np.array(special, dtype=np.int64), prev[take], prev[take] + 1])
    cur = pool[rng.permutation(len(pool))][:n_cur] if n_cur <= len(pool) else \
        np.concatenate([pool, rng.integers(0, 3 * BIG, n_cur - len(pool))])
    return prev.astype(np.int64), np.asarray(cur, dtype=np.int64)


def ragged_sets(sizes_prev, sizes_cur, seed, pad_cur=0, pad_prev=0):
    """two track sets over len(sizes_cur) images: (cur_offsets, cur_id, prev_offsets, prev_id); pad_* rows of padding
    (id -1) follow the last image"""
    rng = np.random.default_rng(seed)
    prevs, curs = zip(*[id_case(p, c, rng) for p, c in zip(sizes_prev, sizes_cur)])
    off = lambda parts: np.concatenate([[0], np.cumsum([len(x) for x in parts])]).astype(np.int64)
    cat = lambda parts, pad: np.concatenate(list(parts) + [np.full(pad, -1, dtype=np.int64)])
    return off(curs), cat(curs, pad_cur), off(prevs), cat(prevs, pad_prev)


# ---------------------------------------------------------------------------------------------------- trajectory_advance
def fresh_state(n, dtype=np.float64):
    q = np.zeros((n, 4), dtype=dtype)
    q[:, 3] = 1
    return np.full(n, np.nan, dtype=dtype), q, np.zeros((n, 3), dtype=dtype)


def decide_np(s, rel_q, rel_t, count=None, min_count=0, scale3=None, n_used=None, min_used=1):
    """the statuses of one step, in float64 as the kernel decides them"""
    s, rel_q, rel_t = (np.asarray(a, dtype=np.float64) for a in (s, rel_q, rel_t))
    n = len(s)
    status = np.empty(n, dtype=np.int32)
    for i in range(n):
        with np.errstate(all="ignore"):
            n2 = ((rel_q[i, 0] * rel_q[i, 0] + rel_q[i, 1] * rel_q[i, 1]) + rel_q[i, 2] * rel_q[i, 2]) + rel_q[i, 3] * rel_q[i, 3]
            present = bool(np.isfinite(rel_q[i]).all() and np.isfinite(rel_t[i]).all() and np.isfinite(n2) and n2 > 0)
            if count is not None:
                present = present and int(count[i]) >= int(min_count)
            if not present:
                status[i] = ABSENT
            elif not (np.isfinite(s[i]) and s[i] > 0):
                status[i] = STARTED
            else:
                status[i] = HELD
                if scale3 is not None:
                    r = np.float64(scale3[i][1])
                    sr = s[i] * r
                    if np.isfinite(r) and r > 0 and (n_used is None or int(n_used[i]) >= int(min_used)) and \
                            np.isfinite(sr) and sr > 0:
                        status[i] = MEASURED
    return status


def advance_np(state, rel_q, rel_t, count=None, min_count=0, scale3=None, n_used=None, min_used=1, dtype=np.float64,
               status=None):
    """pnec_hip_trajectory_advance: ((next_s, next_q, next_p), status).  `status` given: the decisions are taken from it."""
    s, q, p = (np.array(a, dtype=dtype) for a in state)
    rq, rt = np.asarray(rel_q, dtype=dtype), np.asarray(rel_t, dtype=dtype)
    if status is None:
        status = decide_np(s, rel_q, rel_t, count, min_count, scale3, n_used, min_used)
    ns, nq, npos = s.copy(), q.copy(), p.copy()
    for i in range(len(s)):
        if status[i] == ABSENT:
            continue
        if status[i] == STARTED:
            ns[i] = 1
        elif status[i] == MEASURED:
            ns[i] = s[i] * dtype(scale3[i][1])
        x = rq[i]
        n2 = ((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]) + x[3] * x[3]
        step = x / np.sqrt(n2)
        with np.errstate(over="ignore", invalid="ignore"):
            npos[i] = p[i] + qrot(q[i], ns[i] * rt[i])
        nq[i] = qnorm(qmul(q[i], step))
    return (ns, nq, npos), np.asarray(status, dtype=np.int32)


def random_steps(L, n, seed, absent_every=0, held_every=0):
    """L steps for n sequences: rel_q [L,n,4] (not normalised), rel_t [L,n,3] unit, scale3 [L,n,3], n_used [L,n],
    count [L,n]; with absent_every / held_every > 0 every such step of a sequence has a NaN pose / too few links"""
    rng = np.random.default_rng(seed)
    w = rng.normal(0.0, 0.1, (L, n, 3))
    th = np.linalg.norm(w, axis=-1, keepdims=True)
    rel_q = np.concatenate([np.sin(th / 2) * w / th, np.cos(th / 2)], axis=-1) * rng.uniform(0.5, 2.0, (L, n, 1))
    rel_t = rng.normal(0.0, 1.0, (L, n, 3))
    rel_t /= np.linalg.norm(rel_t, axis=-1, keepdims=True)
    med = np.exp(rng.normal(0.0, 0.3, (L, n)))
    scale3 = np.stack([0.9 * med, med, 1.1 * med], axis=-1)
    n_used = rng.integers(5, 50, (L, n)).astype(np.int32)
    count = rng.integers(20, 90, (L, n)).astype(np.int32)
    for k in range(L):
        for i in range(n):
            if absent_every and (k + i) % absent_every == absent_every - 1:
                rel_q[k, i, (k + i) % 4] = np.nan if k % 2 else 0.0
                if k % 2 == 0:
                    count[k, i] = 3
            if held_every and (k + 2 * i) % held_every == held_every - 1:
                n_used[k, i] = 2
    return rel_q, rel_t, scale3, n_used, count


def sign_aligned_diff(a, b):
    a, b = np.asarray(a, dtype=np.longdouble), np.asarray(b, dtype=np.longdouble)
    sgn = np.where((a * b).sum(axis=-1, keepdims=True) >= 0, 1, -1)
    return np.sqrt(((a - sgn * b) ** 2).sum(axis=-1)).astype(np.float64)


# ---------------------------------------------------------------------------------------------------- scale recovery
BASELINES = (1.0, 0.5, 2.0, 1.5)      # the pairs' true baselines, times a factor per sequence
RECOVERY_MIN_PARALLAX = 0.02


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _quat_to_R(q):
    x, y, z, w = np.asarray(q, float) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


class FiveFrames:
    """One sequence of five cameras on exact geometry, after ThreeView of tests/test_relative_scale_cpu.py: pair k is
    (frame k, frame k + 1) with x_k = R_k x_{k+1} + b_k t_k, b_k = factor * BASELINES[k].  A track is a scene point seen by
    all five cameras and its id is the point's number; every pair holds a random share of the tracks in the order of their
    ids, so two consecutive pairs share most tracks but not all, in different rows.
    pairs[k] = (ids int64, f1, f2); q[k], t[k] the pair's true pose; abs_q[k], abs_p[k] the pose of frame k + 1 in frame 0."""

    def __init__(self, rng, n_points, factor, share=0.8, max_angle=0.12):
        self.b = factor * np.array(BASELINES)
        self.q, self.t = [], []
        for _ in BASELINES:
            axis, ang = _unit(rng.standard_normal(3)), rng.uniform(0.02, max_angle)
            self.q.append(np.concatenate([axis * np.sin(ang / 2), [np.cos(ang / 2)]]))
            d = _unit(rng.standard_normal(3) * np.array([1.0, 1.0, 0.3]))    # mostly sideways: parallax
            self.t.append(d)
        frames = np.zeros((5, 0, 3))
        while frames.shape[1] < n_points:
            m = 4 * n_points
            X = np.column_stack([rng.uniform(-4, 4, m), rng.uniform(-4, 4, m), rng.uniform(6, 14, m)]) * factor
            views = [X]
            for k in range(4):
                views.append((views[-1] - self.b[k] * self.t[k]) @ _quat_to_R(self.q[k]))     # x_{k+1} = R_k' (x_k - b_k t_k)
            views = np.stack(views)
            frames = np.concatenate([frames, views[:, (views[:, :, 2] > 0.5 * factor).all(axis=0)]], axis=1)
        frames = frames[:, :n_points]
        self.pairs = []
        for k in range(4):
            ids = np.sort(rng.permutation(n_points)[:int(round(share * n_points))]).astype(np.int64)
            self.pairs.append((ids, _unit(frames[k][ids]), _unit(frames[k + 1][ids])))
        R, p = np.eye(3), np.zeros(3)
        self.abs_R, self.abs_p = [], []
        for k in range(4):
            p = p + R @ (self.b[k] * self.t[k])
            R = R @ _quat_to_R(self.q[k])
            self.abs_R.append(R)
            self.abs_p.append(p)
        self.path = np.cumsum(self.b)


def recovery_sequences(seed=2031, sizes=(90, 130, 257), factors=(1.0, 0.4, 3.0)):
    rng = np.random.default_rng(seed)
    return [FiveFrames(rng, n, f) for n, f in zip(sizes, factors)]


def recovery_pair(seqs, k):
    """pair k of every sequence as one ragged set: (offsets, ids, f1, f2, q [F,4], t [F,3])"""
    off = np.concatenate([[0], np.cumsum([len(s.pairs[k][0]) for s in seqs])]).astype(np.int64)
    cat = lambda j: np.ascontiguousarray(np.concatenate([s.pairs[k][j] for s in seqs]))
    return off, cat(0), cat(1), cat(2), np.array([s.q[k] for s in seqs]), np.array([s.t[k] for s in seqs])
