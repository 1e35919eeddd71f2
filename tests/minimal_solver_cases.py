"""The minimal essential-matrix solvers (Nister five-point, seven-point) in plain numpy, and the inputs their tests share.

minimal_np restates pnec_hip_essential_minimal (include/pnec_hip.h) by a route other than the device's.  The null space
comes from numpy.linalg.eigh (a second route: numpy.linalg.svd of A).  NISTER: the ten cubics are eliminated in graded
order, the 10 x 10 action matrix of the multiplication by x is formed and its real eigenvalues give the solutions -- no
hidden variable, no degree-10 polynomial, no Sturm chain.  SEVENPT: numpy.roots on the cubic.  Polish, normalisation,
order and choice are the device's.

Every case carries its own condition number `kappa`: the largest movement of any solution's e, in units of 2^-52, when
the checker is run again on bearings whose every component is multiplied by 1 +- 2^-52 (signs from a fixed seed, 16
trials).  A device solution must lie within TOL_FACTOR * kappa * 2^-52 of the checker's.
"""
import functools
import itertools

import numpy as np

import eight_point_cases as ec
from eight_point_cases import decompose, draw_pair, quality_terms, rows_of_a, sign_largest  # noqa: F401

NISTER, SEVENPT = 1, 2
MIN_N = {NISTER: 5, SEVENPT: 7}
SAMPLE = {NISTER: 8, SEVENPT: 9}          # common.cc:352-373: sampleSize of NISTER 5 + 3, of SEVENPT 7 + 2
N_NULL = {NISTER: 4, SEVENPT: 2}
MAX_SOLUTIONS = 10
SIZES = {NISTER: (5, 6, 7, 8, 9, 10, 15, 16, 17, 63, 64, 65, 129, 513, 2049),
         SEVENPT: (7, 8, 9, 10, 15, 16, 17, 63, 64, 65, 129, 513, 2049)}
SHORT_SIZES = {NISTER: (4, 0), SEVENPT: (6, 0)}
NOISE_FREE_MAX = 7
NOISE = 1e-3
EPS = 2.0 ** -52
TOL_FACTOR = 32.0
ROUTES_FACTOR = 4.0
GAP_MIN = 1e-6
KAPPA_MAX = 1e5
SEPARATION_MIN = 1e-3
XYZ_MAX = 1e3
IMAG_MIN = 1e-3
KAPPA_TRIALS = 16
START_QUALITY = 1e6
EM_OK, EM_TOO_FEW, EM_NOT_FINITE, EM_NO_CANDIDATE, EM_NO_SOLUTION = 0, 1, 2, 3, 4
NAMES = {NISTER: "NISTER", SEVENPT: "SEVENPT"}


# ---- null spaces -------------------------------------------------------------------------------------------------------
def null_space_eigh(f1, f2, k):
    """(basis [k,9]: rows v0..v(k-1) of the k smallest eigenvalues, eigenvalues ascending) from eigh(A'A)."""
    A = rows_of_a(f1, f2)
    w, V = np.linalg.eigh(A.T @ A)
    return V[:, :k].T.copy(), w


def null_space_svd(f1, f2, k):
    """The same rows from svd(A): the second numpy route, which never forms A'A."""
    A = rows_of_a(f1, f2)
    if len(A) < 9:
        A = np.vstack([A, np.zeros((9 - len(A), 9))])
    Vt = np.linalg.svd(A, full_matrices=True)[2]
    w = np.linalg.svd(A, compute_uv=False)
    w = np.concatenate([w, np.zeros(9 - len(w))])[::-1] ** 2
    return Vt[::-1][:k].copy(), w


# ---- polynomials in (x, y, z) as dictionaries exponent triple -> coefficient --------------------------------------------
def _pmul(a, b):
    out = {}
    for (ka, va), (kb, vb) in itertools.product(a.items(), b.items()):
        k = (ka[0] + kb[0], ka[1] + kb[1], ka[2] + kb[2])
        out[k] = out.get(k, 0.0) + va * vb
    return out


def _padd(a, b, s=1.0):
    out = dict(a)
    for k, v in b.items():
        out[k] = out.get(k, 0.0) + s * v
    return out


_LIN = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0))
# graded order: the ten cubics first, then what spans the quotient ring
GRADED = ((3, 0, 0), (2, 1, 0), (2, 0, 1), (1, 2, 0), (1, 1, 1), (1, 0, 2), (0, 3, 0), (0, 2, 1), (0, 1, 2), (0, 0, 3),
          (2, 0, 0), (1, 1, 0), (1, 0, 1), (0, 2, 0), (0, 1, 1), (0, 0, 2), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0))


def cubic_constraints(X, Y, Z, W, order=GRADED):
    """The 10 x 20 coefficient matrix of det E = 0 and 2 E E'E - tr(E E') E = 0 for E = xX + yY + zZ + W."""
    B = [X.reshape(3, 3), Y.reshape(3, 3), Z.reshape(3, 3), W.reshape(3, 3)]
    E = [[{_LIN[m]: B[m][i, j] for m in range(4)} for j in range(3)] for i in range(3)]
    EEt = [[functools.reduce(_padd, [_pmul(E[i][k], E[j][k]) for k in range(3)]) for j in range(3)] for i in range(3)]
    tr = functools.reduce(_padd, [EEt[i][i] for i in range(3)])
    rows = []
    det = {}
    for (i, j, k), s in (((0, 1, 2), 1), ((1, 2, 0), 1), ((2, 0, 1), 1), ((0, 2, 1), -1), ((1, 0, 2), -1), ((2, 1, 0), -1)):
        det = _padd(det, _pmul(_pmul(E[0][i], E[1][j]), E[2][k]), s)
    rows.append(det)
    for i in range(3):
        for j in range(3):
            p = functools.reduce(_padd, [_pmul(EEt[i][k], E[k][j]) for k in range(3)])
            rows.append(_padd({k: 2.0 * v for k, v in p.items()}, _pmul(tr, E[i][j]), -1.0))
    return np.array([[r.get(m, 0.0) for m in order] for r in rows])


def _gauss_jordan(M):
    M = M.copy()
    n = M.shape[0]
    for p in range(n):
        r = p + int(np.argmax(np.abs(M[p:, p])))
        M[[p, r]] = M[[r, p]]
        M[p] /= M[p, p]
        for q in range(n):
            if q != p:
                M[q] -= M[q, p] * M[p]
    return M


def nister_action_matrix(basis):
    """The solutions (x, y, z), complex, of the ten cubics on E = xX + yY + zZ + W, basis = (W, Z, Y, X) = v0..v3."""
    W, Z, Y, X = basis
    M = _gauss_jordan(cubic_constraints(X, Y, Z, W))
    R = -M[:, 10:]                      # cubic monomial i = R[i] . (x2 xy xz y2 yz z2 x y z 1)
    A = np.zeros((10, 10))
    # x * (x2 xy xz y2 yz z2) = x3 x2y x2z xy2 xyz xz2: rows 0..5 of the graded order
    for b, c in enumerate((0, 1, 2, 3, 4, 5)):
        A[b] = R[c]
    A[6, 0] = A[7, 1] = A[8, 2] = A[9, 6] = 1.0     # x * (x y z 1) = x2 xy xz x
    lam, V = np.linalg.eig(A)
    with np.errstate(all="ignore"):
        xyz = (V[6:9] / V[9]).T
    return lam, xyz


# ---- the polish ----------------------------------------------------------------------------------------------------------
def _adj(M):
    return np.array([np.cross(M[1], M[2]), np.cross(M[2], M[0]), np.cross(M[0], M[1])]).T


def _residual(E):
    EEt = E @ E.T
    return np.concatenate([[np.linalg.det(E)], (2.0 * EEt @ E - np.trace(EEt) * E).ravel()])


def _derivative(E, X):
    d = 2.0 * (X @ E.T @ E + E @ X.T @ E + E @ E.T @ X) - 2.0 * np.trace(E @ X.T) * E - np.trace(E @ E.T) * X
    return np.concatenate([[np.trace(_adj(E) @ X)], d.ravel()])


def polish_nister(xyz, basis, steps=2):
    W, Z, Y, X = (b.reshape(3, 3) for b in basis)
    xyz = np.array(xyz, dtype=np.float64)
    for _ in range(steps):
        E = xyz[0] * X + xyz[1] * Y + xyz[2] * Z + W
        J = np.column_stack([_derivative(E, X), _derivative(E, Y), _derivative(E, Z)])
        r = _residual(E)
        xyz = xyz - np.linalg.solve(J.T @ J, J.T @ r)
    return xyz


def polish_sevenpt(a, basis, steps=2):
    W, X = (b.reshape(3, 3) for b in basis)
    for _ in range(steps):
        E = W + a * X
        a = a - np.linalg.det(E) / np.trace(_adj(E) @ X)
    return a


def sevenpt_cubic(basis):
    """det(W + aX), coefficients of 1, a, a^2, a^3."""
    W, X = (b.reshape(3, 3) for b in basis)
    return np.array([np.linalg.det(W), np.trace(_adj(W) @ X), np.trace(_adj(X) @ W), np.linalg.det(X)])


# ---- solutions of a null space --------------------------------------------------------------------------------------------
def normalise(e):
    e = e / np.linalg.norm(e)
    return e * sign_largest(e)


def lexicographic(es):
    es = np.asarray(es).reshape(-1, 9)
    return es[np.lexsort(es.T[::-1])] if len(es) else es


def solutions_of(basis, algorithm, info=None):
    """[S,9]: the polished, normalised, ordered solutions of a null-space basis (rows v0.. as the header names them)."""
    if algorithm == NISTER:
        lam, xyz = nister_action_matrix(basis)
        real = np.imag(lam) == 0.0
        if info is not None:
            info["xyz"] = np.real(xyz[real])
            cz = xyz[~real]
            info["imag_ratio"] = float(np.min(np.abs(np.imag(cz[:, 2])) / (1.0 + np.abs(cz[:, 2])))) if len(cz) else np.inf
        W, Z, Y, X = basis
        out = []
        for s in np.real(xyz[real]):
            p = polish_nister(s, basis)
            out.append(normalise(p[0] * X + p[1] * Y + p[2] * Z + W))
    else:
        c = sevenpt_cubic(basis)
        r = np.roots(c[::-1])
        real = np.imag(r) == 0.0
        if info is not None:
            cz = r[~real]
            info["imag_ratio"] = float(np.min(np.abs(np.imag(cz)) / (1.0 + np.abs(cz)))) if len(cz) else np.inf
        W, X = basis
        out = [normalise(W + polish_sevenpt(a, basis) * X) for a in np.real(r[real])]
    return lexicographic(out)


def choose(sols, f1, f2, algorithm, quality_all=False):
    """Steps 3-4 over every solution: dict with quality [S,4], choice, R, t, singular (of the chosen one)."""
    K = len(f1) if quality_all else min(SAMPLE[algorithm], len(f1))
    quality = np.full((len(sols), 4), np.nan)
    best, choice, pose = START_QUALITY, -1, None
    for i, e in enumerate(sols):
        S, Ra, Rb, ta = decompose(e.reshape(3, 3))
        for j, (R, t) in enumerate(((Ra, ta), (Rb, ta), (Ra, -ta), (Rb, -ta))):
            s = np.sum(quality_terms(f1[:K], f2[:K], R, t))
            quality[i, j] = s if np.isfinite(s) else np.inf
            if quality[i, j] < best:
                best, choice, pose = quality[i, j], 4 * i + j, (R, t, S)
    return dict(quality=quality, choice=choice, pose=pose, K=K)


def minimal_np(f1, f2, algorithm, quality_all=False, null_space=null_space_eigh, info=None):
    """dict: status, n_solutions, E_all [S,9], quality [S,4], choice, E [9], singular [3], gap, R [3,3], t [3], K."""
    f1, f2 = np.asarray(f1, dtype=np.float64).reshape(-1, 3), np.asarray(f2, dtype=np.float64).reshape(-1, 3)
    nan = np.nan
    out = dict(status=EM_OK, n_solutions=0, E_all=np.zeros((0, 9)), quality=np.zeros((0, 4)), choice=-1, E=np.full(9, nan),
               singular=np.full(3, nan), gap=nan, R=np.full((3, 3), nan), t=np.full(3, nan), K=0)
    if len(f1) < MIN_N[algorithm]:
        out["status"] = EM_TOO_FEW
        return out
    if not (np.all(np.isfinite(f1)) and np.all(np.isfinite(f2))):
        out["status"] = EM_NOT_FINITE
        return out
    k = N_NULL[algorithm]
    basis, w = null_space(f1, f2, k)
    with np.errstate(all="ignore"):
        out["gap"] = (w[k] - w[k - 1]) / w[8]
    sols = solutions_of(basis, algorithm, info)
    if len(sols) == 0:
        out["status"] = EM_NO_SOLUTION
        return out
    c = choose(sols, f1, f2, algorithm, quality_all)
    out.update(n_solutions=len(sols), E_all=sols, quality=c["quality"], K=c["K"])
    if c["choice"] < 0:
        out["status"] = EM_NO_CANDIDATE
        return out
    R, t, S = c["pose"]
    out.update(choice=c["choice"], E=sols[c["choice"] // 4], singular=S, R=R, t=t)
    return out


# ---- distances between solution sets ----------------------------------------------------------------------------------------
def match_sets(a, b):
    """The largest distance of a one-to-one matching of two solution sets of equal size (greedy by nearest; the sets the
    tests compare are separated by far more than they differ).  inf where the sizes differ."""
    a, b = np.asarray(a).reshape(-1, 9), np.asarray(b).reshape(-1, 9)
    if len(a) != len(b):
        return np.inf
    left, worst = list(range(len(b))), 0.0
    for e in a:
        d = [np.linalg.norm(e - b[j]) for j in left]
        j = int(np.argmin(d))
        worst = max(worst, d[j])
        left.pop(j)
    return float(worst)


def min_separation(sols):
    sols = np.asarray(sols).reshape(-1, 9)
    d = [np.linalg.norm(a - b) for a, b in itertools.combinations(sols, 2)]
    return float(min(d)) if d else np.inf


def kappa_of(f1, f2, algorithm, base):
    """The largest movement of any solution's e in units of 2^-52 under component-wise relative perturbations of 2^-52."""
    rng = np.random.default_rng([20261, algorithm, len(f1)])
    worst = 0.0
    for _ in range(KAPPA_TRIALS):
        g1 = f1 * (1.0 + EPS * rng.choice([-1.0, 1.0], size=f1.shape))
        g2 = f2 * (1.0 + EPS * rng.choice([-1.0, 1.0], size=f2.shape))
        basis, _ = null_space_eigh(g1, g2, N_NULL[algorithm])
        worst = max(worst, match_sets(base, solutions_of(basis, algorithm)))
    return worst / EPS


def quality_margin(quality):
    s = np.sort(np.asarray(quality).ravel())
    return float(s[1] - s[0])


class Case:
    def __init__(self, algorithm, n, noise, f1, f2, R, t, draws, quality_all=False, expected=None, kappa=None):
        self.algorithm, self.n, self.noise, self.f1, self.f2, self.R, self.t, self.draws = algorithm, n, noise, f1, f2, R, t, draws
        self.quality_all = quality_all
        self.expected = expected if expected is not None else minimal_np(f1, f2, algorithm, quality_all)
        self.kappa = kappa if kappa is not None else (
            kappa_of(f1, f2, algorithm, self.expected["E_all"]) if self.expected["n_solutions"] else np.nan)

    @property
    def tol(self):
        return TOL_FACTOR * self.kappa * EPS

    @property
    def quality_tol(self):
        """A pose off by tol moves a triangulated direction by at most depth / baseline (8 here) times that, twice per
        term (the eight-point test's bound)."""
        return 32.0 * self.tol * self.expected["K"]

    @property
    def tie(self):
        """N equal to the minimal count: every solution fits the sample exactly, the reference's choice is a tie."""
        return self.n == MIN_N[self.algorithm]


def conditions(case, info):
    """The conditions of a kept case that the checker alone decides -> list of the violated ones."""
    x, alg, bad = case.expected, case.algorithm, []
    if x["status"] != EM_OK:
        return ["status"]
    if not x["gap"] >= GAP_MIN:
        bad.append("gap")
    if not case.kappa <= KAPPA_MAX:
        bad.append("kappa")
    if not min_separation(x["E_all"]) >= SEPARATION_MIN:
        bad.append("separation")
    if not info["imag_ratio"] >= IMAG_MIN:
        bad.append("imag")
    if alg == NISTER:
        if x["n_solutions"] < 2:
            bad.append("count")
        if not np.all(np.linalg.norm(info["xyz"], axis=1) <= XYZ_MAX):
            bad.append("xyz")
    if not case.tie and not quality_margin(x["quality"]) >= 4.0 * case.quality_tol:
        bad.append("margin")
    return bad


def _draw(algorithm, n, seed, want_roots=None, quality_all=False):
    rng = np.random.default_rng(seed)
    noise = 0.0 if n <= NOISE_FREE_MAX else NOISE
    for draws in range(1, 2001):
        f1, f2, R, t = draw_pair(rng, n, noise)
        info = {}
        x = minimal_np(f1, f2, algorithm, quality_all, info=info)
        if x["status"] != EM_OK or (want_roots is not None and x["n_solutions"] != want_roots):
            continue
        c = Case(algorithm, n, noise, f1, f2, R, t, draws, quality_all, expected=x)
        if not conditions(c, info):
            return c
    raise AssertionError(f"no well-posed {NAMES[algorithm]} pair of {n} in 2000 draws")


@functools.lru_cache(maxsize=None)
def cases(algorithm):
    """One case per size.  SEVENPT: the sizes alternate between three roots and one, so that both occur."""
    out = []
    for i, n in enumerate(SIZES[algorithm]):
        want = None if algorithm == NISTER else (3 if i % 2 == 0 else 1)
        out.append(_draw(algorithm, n, [20262, algorithm, n], want))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def short_cases(algorithm):
    out = []
    for n in SHORT_SIZES[algorithm]:
        f1, f2, R, t = draw_pair(np.random.default_rng([20263, algorithm, n]), n, 0.0)
        out.append(Case(algorithm, n, 0.0, f1, f2, R, t, 1))
    return tuple(out)


def true_candidate(res, R, t, tol=0.05):
    return (res["choice"] >= 0 and ec.rotation_distance(res["R"], R) < tol and ec.translation_distance(res["t"], t) < tol)


@functools.lru_cache(maxsize=None)
def outlier_case(algorithm):
    """65 correspondences whose first SAMPLE are gross outliers (f2 negated: the same term of A'A, so the solutions are
    those of the clean pair), as eight_point_cases.outlier_case: the sample prefers a candidate other than the scene's,
    the sum over all rows does not.  -> (sample, all): two Cases over the same bearings."""
    rng = np.random.default_rng([20264, algorithm, 65])
    S = SAMPLE[algorithm]
    for draws in range(1, 2001):
        f1, f2, R, t = draw_pair(rng, 65, NOISE)
        f2 = f2.copy()
        f2[:S] = -f2[:S]
        ia, ib = {}, {}
        a, b = minimal_np(f1, f2, algorithm, False, info=ia), minimal_np(f1, f2, algorithm, True, info=ib)
        if a["status"] != EM_OK or b["status"] != EM_OK or true_candidate(a, R, t) or not true_candidate(b, R, t):
            continue
        ca = Case(algorithm, 65, NOISE, f1, f2, R, t, draws, False, expected=a)
        cb = Case(algorithm, 65, NOISE, f1, f2, R, t, draws, True, expected=b, kappa=ca.kappa)
        if not conditions(ca, ia) and not conditions(cb, ib):
            return ca, cb
    raise AssertionError("no outlier case in 2000 draws")


def batch_arrays(case_list):
    return ec.batch_arrays(case_list)
