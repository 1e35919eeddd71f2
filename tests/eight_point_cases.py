"""The eight-point baseline in plain numpy, and the inputs its tests share.

eight_point_np restates steps 1-5 of pnec_hip_eight_point (include/pnec_hip.h) with numpy.linalg.eigh and
numpy.linalg.svd in place of the device's Jacobi iterations.  The cases are synthetic pairs of every size at which the
kernel takes another path -- both sides of the sample of nine, of the 16-lane row, of one, two and many strides of the
wavefront -- drawn from a fixed seed and kept only if they satisfy the two conditions under which the comparison is well
posed: a relative eigenvalue gap of at least GAP_MIN (the null vector is determined) and a difference of at least
MARGIN_MIN between the best and the second-best quality (the choice is determined).
"""
import functools

import numpy as np

SIZES = (8, 9, 10, 15, 16, 17, 63, 64, 65, 129, 513, 2049)
SHORT_SIZES = (7, 0)
NOISE_FREE_SIZES = SIZES[:3]
NOISE = 1e-3
GAP_MIN = 1e-6
MARGIN_MIN = 1.0
START_QUALITY = 1e6
SAMPLE = 9
EPS = 2.0 ** -52
TOL_FACTOR = 32.0          # q and t within TOL_FACTOR * EPS / gap of the checker
EP_OK, EP_TOO_FEW, EP_NOT_FINITE, EP_NO_CANDIDATE = 0, 1, 2, 3


def sign_largest(v):
    """+1 or -1: the sign that makes the entry of largest magnitude positive (the lowest index wins a tie)."""
    return -1.0 if v[int(np.argmax(np.abs(v)))] < 0.0 else 1.0


def rows_of_a(f1, f2):
    """Row i: the nine products f1_a f2_b in the row-major order of E."""
    return (f1[:, :, None] * f2[:, None, :]).reshape(len(f1), 9)


def null_vector_eigh(f1, f2):
    """(e, eigenvalues ascending) from eigh(A'A); e before the sign rule."""
    A = rows_of_a(f1, f2)
    w, V = np.linalg.eigh(A.T @ A)
    return V[:, 0], w


def null_vector_svd(f1, f2):
    """The same null vector from svd(A): the second numpy route, which never forms A'A."""
    A = rows_of_a(f1, f2)
    return np.linalg.svd(A, full_matrices=True)[2][8]


def decompose(E):
    """Step 3: (singular values, Ra, Rb, ta) with the sign rules that fix the order of the candidates."""
    _, S, Vt = np.linalg.svd(E)
    v0, v1, v2 = Vt[0].copy(), Vt[1].copy(), Vt[2].copy()
    v2 *= sign_largest(v2)
    if v0 @ np.cross(v1, v2) < 0.0:
        v1 = -v1
    with np.errstate(all="ignore"):
        u0 = E @ v0
        u0 = u0 / np.linalg.norm(u0)
        u1 = E @ v1
        u1 = u1 / np.linalg.norm(u1)
        u2 = np.cross(u0, u1)
        u2 = u2 / np.linalg.norm(u2)
    m = np.outer(u1, v0) - np.outer(u0, v1)
    z = np.outer(u2, v2)
    Ra, Rb = z + m, z - m
    if np.linalg.det(Ra) < 0.0:
        Ra = -Ra
    if np.linalg.det(Rb) < 0.0:
        Rb = -Rb
    return S, Ra, Rb, u2


def quality_terms(f1, f2, R, t):
    """(1 - f1.r1) + (1 - f2.r2) per correspondence: the midpoint of pnec_hip_triangulate's system seen from both
    cameras.  NaN where there is no midpoint."""
    with np.errstate(all="ignore"):
        u = f2 @ R.T
        a00, a10, a11 = np.sum(f1 * f1, 1), np.sum(f1 * u, 1), np.sum(u * u, 1)
        b0, b1 = f1 @ t, u @ t
        D = a00 * a11 - a10 * a10
        ok = (D > 2.0 ** -49 * a00 * a11) & np.isfinite(D)
        d1 = (a11 * b0 - a10 * b1) / D
        d2 = (a10 * b0 - a00 * b1) / D
        point = 0.5 * (d1[:, None] * f1 + t[None, :] + d2[:, None] * u)
        r1 = point / np.linalg.norm(point, axis=1)[:, None]
        p2 = (point - t[None, :]) @ R
        r2 = p2 / np.linalg.norm(p2, axis=1)[:, None]
        term = (1.0 - np.sum(f1 * r1, 1)) + (1.0 - np.sum(f2 * r2, 1))
    term[~ok] = np.nan
    return term


def pose_from_null_vector(e, f1, f2, quality_all=False):
    """Steps 2 (norm and sign) to 4 from a null vector: dict with E, singular, R, t, quality, choice."""
    e = e / np.linalg.norm(e)
    e = e * sign_largest(e)
    E = e.reshape(3, 3)
    S, Ra, Rb, ta = decompose(E)
    K = len(f1) if quality_all else min(SAMPLE, len(f1))
    cands = ((Ra, ta), (Rb, ta), (Ra, -ta), (Rb, -ta))
    quality = np.empty(4)
    for c, (R, t) in enumerate(cands):
        s = np.sum(quality_terms(f1[:K], f2[:K], R, t))
        quality[c] = s if np.isfinite(s) else np.inf
    best, choice = START_QUALITY, -1
    for c in range(4):
        if quality[c] < best:
            best, choice = quality[c], c
    out = dict(E=e.copy(), singular=S, quality=quality, choice=choice, R=None, t=None)
    if choice >= 0:
        out["R"], out["t"] = cands[choice][0], cands[choice][1]
    return out


def eight_point_np(f1, f2, quality_all=False):
    """Steps 1-5.  dict: status, choice, E [9], singular [3], gap, eigenvalues [9], quality [4], R [3,3], t [3]; what a
    status other than OK leaves undefined is NaN."""
    f1, f2 = np.asarray(f1, dtype=np.float64).reshape(-1, 3), np.asarray(f2, dtype=np.float64).reshape(-1, 3)
    nan = np.nan
    out = dict(status=EP_OK, choice=-1, E=np.full(9, nan), singular=np.full(3, nan), gap=nan, eigenvalues=np.full(9, nan),
               quality=np.full(4, nan), R=np.full((3, 3), nan), t=np.full(3, nan))
    if len(f1) < 8:
        out["status"] = EP_TOO_FEW
        return out
    if not (np.all(np.isfinite(f1)) and np.all(np.isfinite(f2))):
        out["status"] = EP_NOT_FINITE
        return out
    e, w = null_vector_eigh(f1, f2)
    with np.errstate(all="ignore"):
        out["gap"] = (w[1] - w[0]) / w[8]
    out["eigenvalues"] = w
    r = pose_from_null_vector(e, f1, f2, quality_all)
    out["singular"], out["quality"] = r["singular"], r["quality"]
    if r["choice"] < 0:
        out["status"] = EP_NO_CANDIDATE
        return out
    out["choice"], out["E"], out["R"], out["t"] = r["choice"], r["E"], r["R"], r["t"]
    return out


# ---- distances and conversions ---------------------------------------------------------------------------------------
def rotation_distance(R1, R2):
    """|R1 - R2|_F / sqrt 2: the angle between the two for small angles, without the arccos that bottoms out at 4e-8."""
    return float(np.linalg.norm(R1 - R2) / np.sqrt(2.0))


def translation_distance(t1, t2):
    return float(np.linalg.norm(np.asarray(t1) - np.asarray(t2)))


def rotation_from_quaternion(q):
    """xyzw, taken as unit: the formula, operation for operation, of the host facade's Quaterniond::toRotationMatrix."""
    x, y, z, w = (float(v) for v in q)
    return np.array([[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)],
                     [2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x)],
                     [2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)]])


def rotation_from_vector(v):
    th = np.linalg.norm(v)
    if th == 0.0:
        return np.eye(3)
    k = v / th
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(th) * K + (1.0 - np.cos(th)) * (K @ K)


# ---- the scene ---------------------------------------------------------------------------------------------------------
def draw_pair(rng, n, noise):
    """n points in a box in front of both cameras, a rotation of up to 0.1 rad, a unit baseline.
    -> (f1 [n,3], f2 [n,3], R, t) with x1 = R x2 + t."""
    axis = rng.normal(size=3)
    R = rotation_from_vector(axis / np.linalg.norm(axis) * rng.uniform(0.0, 0.1))
    t = rng.normal(size=3)
    t /= np.linalg.norm(t)
    x1 = np.column_stack([rng.uniform(-2.0, 2.0, n), rng.uniform(-2.0, 2.0, n), rng.uniform(4.0, 8.0, n)])
    x2 = (x1 - t[None, :]) @ R
    f1 = x1 / np.maximum(np.linalg.norm(x1, axis=1), 1e-300)[:, None]
    f2 = x2 / np.maximum(np.linalg.norm(x2, axis=1), 1e-300)[:, None]
    if noise > 0.0 and n > 0:
        f1 = f1 + rng.normal(scale=noise, size=(n, 3))
        f2 = f2 + rng.normal(scale=noise, size=(n, 3))
        f1 /= np.linalg.norm(f1, axis=1)[:, None]
        f2 /= np.linalg.norm(f2, axis=1)[:, None]
    return f1, f2, R, t


def quality_margin(quality):
    s = np.sort(quality)
    return float(s[1] - s[0])


def well_posed(res):
    return (res["status"] == EP_OK and res["gap"] >= GAP_MIN and quality_margin(res["quality"]) >= MARGIN_MIN)


class Case:
    def __init__(self, n, noise, f1, f2, R, t, draws, quality_all=False):
        self.n, self.noise, self.f1, self.f2, self.R, self.t, self.draws = n, noise, f1, f2, R, t, draws
        self.quality_all = quality_all
        self.expected = eight_point_np(f1, f2, quality_all) if n else eight_point_np(np.zeros((0, 3)), np.zeros((0, 3)))

    @property
    def tol(self):
        """TOL_FACTOR * EPS / gap of this case, gap from the checker's eigenvalues."""
        return TOL_FACTOR * EPS / self.expected["gap"]


def _draw_well_posed(n, noise, seed):
    rng = np.random.default_rng(seed)
    for draws in range(1, 2001):
        f1, f2, R, t = draw_pair(rng, n, noise)
        if well_posed(eight_point_np(f1, f2)):
            return Case(n, noise, f1, f2, R, t, draws)
    raise AssertionError(f"no well-posed pair of {n} in 2000 draws")


@functools.lru_cache(maxsize=None)
def cases():
    """One case per size of SIZES, every one satisfying both conditions (deterministic rejection from a fixed seed)."""
    return tuple(_draw_well_posed(n, 0.0 if n in NOISE_FREE_SIZES else NOISE, [20241, n]) for n in SIZES)


@functools.lru_cache(maxsize=None)
def short_cases():
    """The pairs of 7 and of 0 correspondences."""
    out = []
    for n in SHORT_SIZES:
        f1, f2, R, t = draw_pair(np.random.default_rng([20242, n]), n, 0.0)
        out.append(Case(n, 0.0, f1, f2, R, t, 1))
    return tuple(out)


def true_candidate(res, R, t, tol=0.05):
    """Whether the pose a result chose is the scene's (within `tol`: the other three are a baseline flip or a twist of
    pi away)."""
    return (res["choice"] >= 0 and rotation_distance(res["R"], R) < tol and translation_distance(res["t"], t) < tol)


@functools.lru_cache(maxsize=None)
def outlier_case():
    """65 correspondences whose first nine are gross outliers: their f2 is negated (180 degrees off: the point lies
    behind the second camera).  A negated row of A is the same term of A'A, so E is that of the clean pair, but the sample
    of nine now prefers a candidate other than the scene's, and the sum over all 65 rows does not.  -> (sample, all):
    two Cases over the same bearings."""
    rng = np.random.default_rng([20243, 65])
    for draws in range(1, 2001):
        f1, f2, R, t = draw_pair(rng, 65, NOISE)
        f2 = f2.copy()
        f2[:SAMPLE] = -f2[:SAMPLE]
        a, b = eight_point_np(f1, f2, False), eight_point_np(f1, f2, True)
        if well_posed(a) and well_posed(b) and not true_candidate(a, R, t) and true_candidate(b, R, t):
            return Case(65, NOISE, f1, f2, R, t, draws, False), Case(65, NOISE, f1, f2, R, t, draws, True)
    raise AssertionError("no outlier case in 2000 draws")


def batch_arrays(case_list):
    """(offsets int64 [P+1], f1 [sum N,3], f2 [sum N,3]) of a ragged batch of cases."""
    offsets = np.concatenate([[0], np.cumsum([c.n for c in case_list])]).astype(np.int64)
    f1 = np.concatenate([c.f1.reshape(-1, 3) for c in case_list]) if len(case_list) else np.zeros((0, 3))
    f2 = np.concatenate([c.f2.reshape(-1, 3) for c in case_list]) if len(case_list) else np.zeros((0, 3))
    return offsets, np.ascontiguousarray(f1), np.ascontiguousarray(f2)
