"""Batch front-end over the C ABI: a batch of frame pairs resident in HBM and its solves.

numpy arguments go through the HOST memory space of the ABI (blocking, PCIe-inclusive);
torch CUDA tensors go through the DEVICE space (asynchronous on torch's current stream).
torch is plumbing here (device memory, streams); all arithmetic is in libpnec_hip.so.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import capi


def _is_torch(x) -> bool:
    return x is not None and type(x).__module__.startswith("torch")


@dataclass
class SolveResult:
    """Per solve (pair-major, hypothesis-minor): what PNECCeres::Result() returns + summary."""
    q: object           # [S,4] xyzw, normalised
    t: object           # [S,3] unit
    cost: object        # [S]   1/2 sum r^2 at the returned point
    iterations: object  # [S]   int32
    status: object      # [S]   int32, capi.TERM_NAMES
    # the solve that produced it (Batch.solve fills these in; covariance() needs them)
    batch: object = field(default=None, repr=False, compare=False)
    reg: float = field(default=1e-13, repr=False, compare=False)
    n_hyp: int = field(default=1, repr=False, compare=False)

    def covariance(self) -> "PoseCovariance":
        """Batch.pose_covariance at this result's own poses, with the `reg` and `n_hyp` of the solve it came from."""
        if self.batch is None:
            raise ValueError("this SolveResult was not produced by Batch.solve: call Batch.pose_covariance(q, t)")
        return self.batch.pose_covariance(self.q, self.t, reg=self.reg, n_hyp=self.n_hyp)

    def residuals(self, gate: float = 3.0) -> "ResidualReport":
        """Batch.residuals at this result's own poses, with the `reg` and `n_hyp` of the solve it came from."""
        if self.batch is None:
            raise ValueError("this SolveResult was not produced by Batch.solve: call Batch.residuals(q, t)")
        return self.batch.residuals(self.q, self.t, reg=self.reg, gate=gate, n_hyp=self.n_hyp)

    def sensitivity(self, grad_pose, gauss_newton: bool = False, zero_on_failure: bool = False) -> "PoseSensitivity":
        """Batch.pose_sensitivity at this result's own poses, with the `reg` and `n_hyp` of the solve it came from: the
        gradient of a loss of these poses with respect to the pair's bearing vectors and covariances."""
        if self.batch is None:
            raise ValueError("this SolveResult was not produced by Batch.solve: call Batch.pose_sensitivity(q, t, grad_pose)")
        return self.batch.pose_sensitivity(self.q, self.t, grad_pose, reg=self.reg, n_hyp=self.n_hyp,
                                           gauss_newton=gauss_newton, zero_on_failure=zero_on_failure)

    def triangulate(self, orient: bool = True) -> "Triangulation":
        """Batch.triangulate at this result's own poses, with the `n_hyp` of the solve it came from: the structure the
        solved pose implies and, with `orient`, the sign of t that puts it in front of both cameras."""
        if self.batch is None:
            raise ValueError("this SolveResult was not produced by Batch.solve: call Batch.triangulate(q, t)")
        return self.batch.triangulate(self.q, self.t, n_hyp=self.n_hyp, orient=orient)

    def rotation_matrices(self):
        """[S,3,3] from q (numpy or torch, matching the stored arrays)."""
        q = self.q
        x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
        xp = __import__("torch") if _is_torch(q) else np
        R = xp.stack([
            xp.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
            xp.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
            xp.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1),
        ], -2)
        return R


_TRI5 = tuple((a, b) for a in range(5) for b in range(a, 5))  # the ABI's packed order of a symmetric 5x5


_FULL5 = tuple(min(a, b) * 5 - min(a, b) * (min(a, b) - 1) // 2 + abs(a - b) for a in range(5) for b in range(5))
_full5_on = {}   # torch device -> _FULL5 as an index tensor there (made once: no upload per call)
_kinv_on = {}    # (device, bytes of K_inv) -> its column-major image on that device (fill_keypoints: no upload per call)


def expand_info(packed):
    """[..., 15] packed upper triangles (pnec_hip_pose_covariance's out_info) -> [..., 5, 5] full symmetric matrices."""
    if _is_torch(packed):
        import torch
        idx = _full5_on.get(packed.device)
        if idx is None:
            idx = _full5_on[packed.device] = torch.tensor(_FULL5, device=packed.device)
        return packed.index_select(-1, idx).reshape(tuple(packed.shape[:-1]) + (5, 5))
    packed = np.asarray(packed)
    return packed[..., list(_FULL5)].reshape(packed.shape[:-1] + (5, 5))


def chart_basis(t):
    """(b_theta, e_phi, sin theta) of the translation direction t [3] as pnec_hip_pose_covariance defines them
    (include/pnec_hip.h): the orthonormal basis of t's tangent plane the 6x6 covariance is lifted with."""
    t = np.asarray(t, dtype=np.float64)
    n = np.linalg.norm(t)
    rho = np.hypot(t[0], t[1])
    st, ct = (rho / n, t[2] / n) if n > 0 else (0.0, 1.0)
    if rho == 0.0 or (st < 1e-10 and ct > 0.0):
        cp, sp = 1.0, 0.0
    else:
        cp, sp = t[0] / rho, t[1] / rho
    return np.array([ct * cp, ct * sp, -st]), np.array([-sp, cp, 0.0]), st


def cov6_to_ceres_chart(cov6, t):
    """Sigma_6 (omega, t) -> the 5x5 covariance of the Ceres tangent space (theta, phi, delta_xyz) at t: the inverse of
    `info` where sin theta != 0.  theta = b_theta . dt, phi = e_phi . dt / sin theta, delta = omega / 2."""
    bth, eph, st = chart_basis(t)
    T = np.zeros((5, 6))
    T[0, 3:] = bth
    T[1, 3:] = eph / st
    T[2:, :3] = 0.5 * np.eye(3)
    return T @ np.asarray(cov6) @ T.T


def ceres_chart_to_cov6(cov5, t):
    """The inverse map: a 5x5 covariance of (theta, phi, delta_xyz) at t -> Sigma_6 (omega, t)."""
    bth, eph, st = chart_basis(t)
    Lm = np.zeros((6, 5))
    Lm[3:, 0] = bth
    Lm[3:, 1] = eph * st
    Lm[:3, 2:] = 2.0 * np.eye(3)
    return Lm @ np.asarray(cov5) @ Lm.T


@dataclass
class PoseCovariance:
    """Per pose slot (pair-major, hypothesis-minor): pnec_hip_pose_covariance's outputs (include/pnec_hip.h has the
    chart conventions).  NEC-mode batches: `cov` is for unit residual variance; scale it by 2 cost / (n - 5)."""
    cov: object     # [S,6,6] covariance of (omega_xyz [rad, left perturbation], t_xyz [unit direction]); rank 5
    info: object    # [S,5,5] J'J in the Ceres tangent space (theta, phi, delta_xyz), full symmetric
    grad: object    # [S,5]   J'r in the same space
    cost: object    # [S]     1/2 sum r^2
    status: object  # [S]     int32, capi.COV_NAMES


@dataclass
class PoseSensitivity:
    """pnec_hip_pose_sensitivity's outputs (include/pnec_hip.h has the definitions).  Per correspondence, row
    n_hyp * offsets[p] + h * N_p + i: the gradient of the loss with respect to that correspondence's inputs; per pose
    slot (pair-major, hypothesis-minor): what the implicit-function step was made of."""
    grad_bvs1: object       # [M,3]
    grad_bvs2: object       # [M,3]
    grad_covs: object       # [M,3,3] symmetric, None for NEC batches
    grad_covs_host: object  # [M,3,3] symmetric, SYM batches only (None otherwise)
    lam: object             # [S,5]   lambda = H^-1 v in the chart (tau_1, tau_2, omega)
    hessian: object         # [S,5,5] H in the same chart, full symmetric
    grad: object            # [S,5]   g = grad_x E
    newton: object          # [S,5]   x_N = -H^-1 g: how far the pose is from the minimiser
    status: object          # [S]     int32, capi.SENS_NAMES


def gate_sigma(confidence: float) -> float:
    """The gate, in sigmas, that a share `confidence` of N(0, 1) residuals passes: the two-sided normal quantile
    (gate_sigma(0.9973) is 3.0 to 3 digits)."""
    from statistics import NormalDist
    c = float(confidence)
    if not 0.0 < c < 1.0:
        raise ValueError("confidence must lie in (0, 1)")
    return NormalDist().inv_cdf(0.5 * (1.0 + c))


@dataclass
class ResidualReport:
    """pnec_hip_residuals' outputs (include/pnec_hip.h).  Per correspondence, [n_hyp * sum N]: the entry of (pair p,
    hypothesis h, correspondence i) is n_hyp * offsets[p] + h * N_p + i; per slot (pair-major, hypothesis-minor), [S].
    The gate classifies at the pose it was given -- one already near the truth; it is not a robust estimator."""
    residual: object     # signed whitened residual r_i (NEC: the bare normal epipolar error)
    variance: object     # the propagated variance r_i was whitened by (NEC: exactly 1)
    mask: object         # uint8, 1 iff |r_i| <= gate; with n_hyp == 1 it is what Batch.select takes
    chi2: object         # [S] sum r^2  (twice the cost)
    gated_chi2: object   # [S] sum of r^2 over the mask
    gated_count: object  # [S] int32
    max_abs: object      # [S] max |r|  (NaN if a residual is NaN)
    offsets: np.ndarray  # int64 [n_pairs+1], the batch's own
    n_hyp: int = 1

    def variance_factor(self, dof: int = 5):
        """chi2 / (n - dof) per slot, NaN where n <= dof: ~1 when the covariances describe the data; what a NEC-mode
        PoseCovariance.cov is to be multiplied by."""
        n = np.repeat(np.diff(np.asarray(self.offsets, dtype=np.int64)), int(self.n_hyp)).astype(np.float64) - dof
        n[n <= 0] = np.nan
        if _is_torch(self.chi2):
            import torch
            return self.chi2 / torch.as_tensor(n, device=self.chi2.device)
        return np.asarray(self.chi2, dtype=np.float64) / n


@dataclass
class Triangulation:
    """pnec_hip_triangulate's outputs (include/pnec_hip.h has the definitions).  Per correspondence, [n_hyp * sum N], in
    ResidualReport's layout: the entry of (pair p, hypothesis h, correspondence i) is n_hyp * offsets[p] + h * N_p + i;
    per slot (pair-major, hypothesis-minor), [S].  Lengths are in baselines (t is a direction).  With `orient` the
    per-correspondence fields are evaluated at `t` below (the oriented direction), otherwise at the t passed in; the
    vote (n_front, n_back, sign) is always relative to the t passed in."""
    point: object          # [M,3] midpoint of the two rays, frame 1; NaN for parallel rays
    depth1: object         # [M] along f1 from camera 1; +inf for parallel rays
    depth2: object         # [M] along R f2 from camera 2
    parallax: object       # [M] angle between f1 and R f2, radians
    depth1_var: object     # [M] first-order variance of depth1 from the batch's covariances (NEC: NaN)
    front: object          # [M] uint8, 1 iff both depths are positive; with n_hyp == 1 it is what Batch.select takes
    n_front: object        # [S] int32, correspondences in front of both cameras at the t passed in
    n_back: object         # [S] int32, correspondences behind both (in front under -t)
    sign: object           # [S] int32, +1 if n_front >= n_back else -1
    t: object              # [S,3] sign * t / |t|
    parallax_mean: object  # [S] mean parallax of the pair, 0 if it has no correspondence
    offsets: np.ndarray = None  # int64 [n_pairs+1], the batch's own
    n_hyp: int = 1


@dataclass
class EightPoint:
    """pnec_hip_eight_point's outputs (include/pnec_hip.h has the definitions): essential matrix and pose of every pair
    from its correspondences alone.  Per pair [P]; where `status` is not capi.EP_OK, q, t and E are NaN and choice -1."""
    q: object          # [P,4] xyzw; R takes frame-2 vectors into frame 1
    t: object          # [P,3] unit direction in frame 1
    E: object          # [P,9] row-major, unit norm, entry of largest magnitude positive; f1' E f2 = 0
    singular: object   # [P,3] singular values of E, descending (the reference's scale is singular[:, 0])
    gap: object        # [P] (lambda_1 - lambda_0) / lambda_8 of A'A: small for planar scenes and pure rotations
    quality: object    # [P,4] of (Ra, ta), (Rb, ta), (Ra, -ta), (Rb, -ta); +inf where a term was not finite
    choice: object     # [P] int32, the candidate taken
    status: object     # [P] int32, capi.EP_OK / EP_TOO_FEW / EP_NOT_FINITE / EP_NO_CANDIDATE


@dataclass
class MinimalPose:
    """pnec_hip_essential_minimal's outputs (include/pnec_hip.h has the definitions): every solution of the five-point or
    the seven-point solver and the pose chosen among their decompositions.  Per pair [P]; where `status` is not
    capi.EM_OK, q, t, E and singular are NaN and choice -1."""
    q: object            # [P,4] xyzw; R takes frame-2 vectors into frame 1
    t: object            # [P,3] unit direction in frame 1
    E: object            # [P,9] the chosen solution, row-major, unit norm, entry of largest magnitude positive
    singular: object     # [P,3] singular values of the chosen solution, descending
    gap: object          # [P] the eigenvalue gap above the null space, over lambda_8
    n_solutions: object  # [P] int32, at most capi.EM_MAX_SOLUTIONS
    E_all: object        # [P,10,9] every solution in lexicographic order, NaN beyond n_solutions
    quality: object      # [P,10,4] of the four candidates of every solution; +inf where a term was not finite, NaN beyond
    choice: object       # [P] int32, 4 * solution + candidate
    status: object       # [P] int32, capi.EM_OK / EM_TOO_FEW / EM_NOT_FINITE / EM_NO_CANDIDATE / EM_NO_SOLUTION


@dataclass
class EssentialRansac:
    """pnec_hip_essential_ransac's outputs (include/pnec_hip.h has the definitions): the pose of the best five-, seven- or
    eight-point model among random samples and its inliers, from correspondences alone.  Per pair [P]; where `status` is
    not capi.ER_OK, q, t, E and singular are NaN, best_attempt is -1 and the pair's part of the mask is zero."""
    q: object             # [P,4] xyzw; R takes frame-2 vectors into frame 1
    t: object             # [P,3] unit direction in frame 1
    E: object             # [P,9] the best attempt's chosen solution, row-major, unit norm
    singular: object      # [P,3] its singular values, descending
    mask: object          # [sum N] uint8 in the batch's correspondence order: what Batch.select takes
    count: object         # [P] int32, the mask's sum per pair
    iterations: object    # [P] int32, attempts that had a model (the rule's `it`)
    attempts: object      # [P] int32, samples drawn
    best_attempt: object  # [P] int32, the index of the winning sample
    status: object        # [P] int32, capi.ER_OK / ER_TOO_FEW / ER_NO_MODEL


_ER_ALGORITHMS = {"nister": capi.EM_NISTER, "sevenpt": capi.EM_SEVENPT, "eightpt": capi.EM_EIGHTPT}


@dataclass
class RelativeScale:
    """pnec_hip_relative_scale's outputs (include/pnec_hip.h has the definitions): the ratio of each pair's baseline to
    its previous pair's, from the tracks the two pairs share.  Per pair [P]: `scale` (the lower median of the used
    ratios -- an element of the set), `q25` / `q75` (lower / upper quartile), `n_linked`, `n_used`; NaN where no link was
    used.  Per correspondence of the current batch [sum N], when asked for: `ratio` (NaN for a link that is not used) and
    `used` (uint8)."""
    scale: object          # [P] |baseline_cur| / |baseline_prev|
    q25: object            # [P]
    q75: object            # [P]
    n_linked: object       # [P] int32, links within range
    n_used: object         # [P] int32, links in front at both poses, past the parallax gate, with a positive finite ratio
    ratio: object = None   # [sum N] or None (per_link=False)
    used: object = None    # [sum N] uint8 or None
    offsets: np.ndarray = None  # int64 [P+1], the current batch's own

    def log_sigma(self):
        """log(q75 / q25) / 1.349: a robust standard deviation of log(scale) (the interquartile range of a normal
        distribution is 1.349 sigma).  numpy or torch, matching the stored arrays."""
        if _is_torch(self.q75):
            import torch
            return torch.log(self.q75 / self.q25) / 1.349
        with np.errstate(all="ignore"):
            return np.log(np.asarray(self.q75) / np.asarray(self.q25)) / 1.349


class Batch:
    """A batch of independent frame pairs in the solver's SoA layout (``pnec_hip_problem``)."""

    def __init__(self, mode: int, offsets, device: int = 0):
        self._lib = capi.lib()
        self.mode = int(mode)
        self.device = int(device)
        self._offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        if self._offsets.ndim != 1 or len(self._offsets) < 1:
            raise ValueError("offsets must be a 1-D array of length n_pairs+1")
        self.n_pairs = len(self._offsets) - 1
        h = C.c_void_p()
        capi.check(self._lib.pnec_hip_problem_create(self.device, self.mode, self.n_pairs,
                                                     self._offsets.ctypes.data, C.byref(h)))
        self._h = h

    @property
    def offsets(self) -> np.ndarray:
        """int64 [n_pairs+1]; for a batch made by select() the first access waits for the device."""
        if self._offsets is None:
            off = np.empty(self.n_pairs + 1, dtype=np.int64)
            capi.check(self._lib.pnec_hip_problem_offsets(self._h, off.ctypes.data))
            self._offsets = off
        return self._offsets

    @classmethod
    def uniform(cls, mode: int, n_pairs: int, n_corr: int, device: int = 0) -> "Batch":
        return cls(mode, np.arange(n_pairs + 1, dtype=np.int64) * n_corr, device)

    @classmethod
    def with_capacity(cls, mode: int, max_pairs: int, max_corr: int, device: int = 0) -> "Batch":
        """A batch that is shaped again and again without allocating (pnec_hip_problem_create_capacity): room for up to
        max_pairs pairs / max_corr correspondences in total, created empty; give it a shape with reshape(), then fill."""
        b = cls.__new__(cls)
        b._lib = capi.lib()
        b.mode, b.device = int(mode), int(device)
        h = C.c_void_p()
        capi.check(b._lib.pnec_hip_problem_create_capacity(b.device, b.mode, int(max_pairs), int(max_corr), C.byref(h)))
        b._h = h
        b.n_pairs = 0
        b._offsets = np.zeros(1, dtype=np.int64)
        return b

    def reshape(self, offsets) -> "Batch":
        """A new shape for a capacity batch (pnec_hip_problem_reshape), asynchronous on torch's current stream: work queued
        earlier still sees the old shape; the planes hold garbage until filled."""
        off = np.ascontiguousarray(offsets, dtype=np.int64)
        stream = None
        try:
            import torch
            if torch.cuda.is_available():
                stream = torch.cuda.current_stream(self.device).cuda_stream
        except ImportError:
            pass
        capi.check(self._lib.pnec_hip_problem_reshape(self._h, len(off) - 1, off.ctypes.data, stream))
        self._offsets = off
        self.n_pairs = len(off) - 1
        return self

    # -- lifetime ---------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            if not getattr(self, "_borrowed", False):     # (a select(view=True) result belongs to its source)
                self._lib.pnec_hip_problem_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- info -------------------------------------------------------------------------------
    @property
    def num_correspondences(self) -> int:
        return self._lib.pnec_hip_problem_num_correspondences(self._h)

    @property
    def max_correspondences(self) -> int:
        return self._lib.pnec_hip_problem_max_correspondences(self._h)

    @property
    def payload_bytes(self) -> int:
        return self._lib.pnec_hip_problem_payload_bytes(self._h)

    def describe_launch(self, options: capi.Options | None = None) -> dict:
        cpl, wpp, ldsk, tpb, res = (C.c_int32() for _ in range(5))
        capi.check(self._lib.pnec_hip_describe_launch(
            self._h, C.byref(options) if options is not None else None, C.byref(cpl),
            C.byref(wpp), C.byref(ldsk), C.byref(tpb), C.byref(res)))
        return {"corr_per_lane": cpl.value, "waves_per_pair": wpp.value,
                "lds_corr_per_lane": ldsk.value, "threads_per_block": tpb.value,
                "resident": bool(res.value)}

    # -- argument hygiene (DEVICE space: the ABI reinterprets the pointer as float64 on self.device)
    def _dev_tensor(self, a, name, shape=None, dtype=None):
        """A contiguous CUDA tensor of `dtype` (float64 by default) on this batch's GPU, or an error."""
        import torch
        if a is None:
            return None
        dtype = dtype or torch.float64
        if not _is_torch(a):
            raise TypeError(f"{name}: mixing numpy and torch arguments in one call is not supported")
        if not a.is_cuda:
            raise ValueError(f"{name}: torch arguments must be CUDA tensors (or pass numpy arrays)")
        if a.device.index != self.device:
            raise ValueError(f"{name}: tensor lives on cuda:{a.device.index}, the batch on cuda:{self.device}")
        if a.dtype != dtype:
            if dtype != torch.float64 or not a.dtype.is_floating_point:
                raise TypeError(f"{name}: expected {dtype}, got {a.dtype}")
            a = a.to(dtype)
        a = a.contiguous()
        if shape is not None and tuple(a.shape) != tuple(shape):
            raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(a.shape)}")
        return a

    def _dev_out(self, a, name, shape, dtype):
        """A caller-supplied output buffer: must already be exactly what the kernel writes."""
        if not (_is_torch(a) and a.is_cuda and a.device.index == self.device and a.dtype == dtype
                and a.is_contiguous() and tuple(a.shape) == tuple(shape)):
            raise ValueError(f"out.{name}: need a contiguous {dtype} CUDA tensor of shape {tuple(shape)} "
                             f"on cuda:{self.device}")
        return a

    # -- ingest -----------------------------------------------------------------------------
    def fill(self, bvs1, bvs2, covs=None, covs_host=None, first_pair: int = 0,
             n_pairs: int | None = None):
        """Fill pairs [first_pair, first_pair+n_pairs) from reference-layout arrays.

        bvs*: [M,3]; covs*: [M,3,3] (symmetric) or [M,9] Eigen column-major; M = the number of
        correspondences in that pair range.  numpy -> HOST space, torch.cuda -> DEVICE space.
        """
        if n_pairs is None:
            n_pairs = self.n_pairs - first_pair
        m = int(self.offsets[first_pair + n_pairs] - self.offsets[first_pair])
        arrays = [bvs1, bvs2, covs, covs_host]
        on_device = self._on_device = _is_torch(bvs1)
        ptrs, keep = [], []
        for i, a in enumerate(arrays):
            if a is None:
                ptrs.append(None)
                continue
            width = 3 if i < 2 else 9
            if on_device:
                import torch
                if not _is_torch(a) or not a.is_cuda:
                    raise ValueError("torch inputs must be CUDA tensors (or pass numpy)")
                if a.device.index != self.device:
                    raise ValueError(f"array {i}: tensor on cuda:{a.device.index}, batch on cuda:{self.device}")
                if a.dim() == 3:  # [M,3,3] symmetric == its own column-major image
                    a = a.reshape(a.shape[0], 9)
                a = a.contiguous().to(torch.float64)
                if a.numel() != m * width:
                    raise ValueError(f"array {i}: expected {m}x{width} values, got {a.numel()}")
                keep.append(a)
                ptrs.append(a.data_ptr())
            else:
                a = np.asarray(a, dtype=np.float64)
                if a.ndim == 3:
                    a = np.transpose(a, (0, 2, 1)).reshape(a.shape[0], 9)
                a = np.ascontiguousarray(a)
                if a.size != m * width:
                    raise ValueError(f"array {i}: expected {m}x{width} values, got {a.size}")
                keep.append(a)
                ptrs.append(a.ctypes.data)
        stream = None
        if on_device:
            import torch
            stream = torch.cuda.current_stream(self.device).cuda_stream
        capi.check(self._lib.pnec_hip_problem_fill(
            self._h, first_pair, n_pairs, ptrs[0], ptrs[1], ptrs[2], ptrs[3],
            capi.MEM_DEVICE if on_device else capi.MEM_HOST, stream))
        return self

    def fill_keypoints(self, pts1, pts2, cov2=None, cov1=None, K_inv=None, kappa: float = 1.0,
                       first_pair: int = 0, n_pairs: int | None = None):
        """Fused ingest from keypoints (KeyPoint::Unproject, keypoints.cc:49-62): pixel positions [M,2] of
        both frames + image-plane covariances [M,2,2] (or [M,3] = xx, xy, yy) -> bearings and bearing
        covariances computed on the device straight into the SoA planes.  numpy -> HOST space,
        torch.cuda -> DEVICE space, asynchronous on torch's current stream: K_inv [3,3] is then a CUDA tensor, or a host
        array that is uploaded the first time its value is seen (that one call waits for the stream)."""
        if n_pairs is None:
            n_pairs = self.n_pairs - first_pair
        m = int(self.offsets[first_pair + n_pairs] - self.offsets[first_pair])
        on_device = self._on_device = _is_torch(pts1)
        xp = __import__("torch") if on_device else np

        def c3(a):
            if a is None:
                return None
            if a.ndim == 3:  # [M,2,2] -> (xx, xy, yy)
                a = xp.stack([a[:, 0, 0], a[:, 1, 0], a[:, 1, 1]], -1)
            return a
        K = np.eye(3) if K_inv is None else K_inv
        arrays = [(pts1, 2), (pts2, 2), (c3(cov2), 3), (c3(cov1), 3)]
        ptrs, keep = [], []
        for a, width in arrays:
            if a is None:
                ptrs.append(None)
                continue
            if on_device:
                a = self._dev_tensor(a, "keypoint array")
                ptrs.append(a.data_ptr())
            else:
                a = np.ascontiguousarray(a, dtype=np.float64)
                ptrs.append(a.ctypes.data)
            if int(np.prod(a.shape)) != m * width:
                raise ValueError(f"expected {m}x{width} values, got {tuple(a.shape)}")
            keep.append(a)
        Kd, kp, space, stream = self._kinv_arg(K, on_device)
        capi.check(self._lib.pnec_hip_problem_fill_keypoints(self._h, first_pair, n_pairs, ptrs[0], ptrs[1], ptrs[2],
                                                             ptrs[3], kp, float(kappa), 1, space, stream))
        return self

    def _kinv_arg(self, K, on_device):
        """K_inv [3,3] (None: the identity) as the keypoint ingests take it -> (the column-major array, kept alive by the
        caller; its pointer; the memory space; the stream)."""
        K = np.eye(3) if K is None else K
        if on_device:
            import torch
            # no host round trip per call (an upload from pageable memory waits for the stream): a CUDA K_inv is
            # transposed where it is, a host one is uploaded once per value and device
            if _is_torch(K) and K.is_cuda:
                Kd = self._dev_tensor(K, "K_inv", (3, 3)).t().contiguous().reshape(9)
            else:
                K9 = np.asarray(K.cpu() if _is_torch(K) else K, dtype=np.float64).T.copy().reshape(9)
                key = (self.device, K9.tobytes())
                Kd = _kinv_on.get(key)
                if Kd is None:
                    if len(_kinv_on) >= 64:
                        _kinv_on.clear()
                    Kd = _kinv_on[key] = torch.as_tensor(K9, device=f"cuda:{self.device}")
            return Kd, Kd.data_ptr(), capi.MEM_DEVICE, torch.cuda.current_stream(self.device).cuda_stream
        Kd = np.ascontiguousarray(np.asarray(K, dtype=np.float64).T.reshape(9))
        return Kd, Kd.ctypes.data, capi.MEM_HOST, None

    def fill_keypoints_ragged(self, offsets, pts1, pts2, cov2=None, cov1=None, K_inv=None, kappa: float = 1.0,
                              dropped=None) -> "Batch":
        """fill_keypoints shaped by offsets that may live on the device (pnec_hip_problem_fill_keypoints_ragged): this
        capacity batch's current shape -- its last reshape() -- gives the BOUNDS, pair k takes the first
        min(offsets[k+1] - offsets[k], bound_k) of the rows [offsets[k], offsets[k+1]) of pts1 / pts2 [R,2], cov2 / cov1
        [R,3] (or [R,2,2]), and the batch's own offsets become the scan of those counts.  What a Tracker hands over goes
        in as it is: fill_keypoints_ragged(pairs.offsets, pairs.prev_pts, pairs.pts, pairs.cov).

        torch.cuda tensors -> DEVICE space, asynchronous on torch's current stream, nothing read back (K_inv as for
        fill_keypoints); numpy arrays -> HOST space, staged, the call waits.  `dropped`: an int32 [n_pairs] array of
        the same kind that receives the rows each bound turned away.  Afterwards the batch is what select() returns:
        solve, solve_pipeline (without want_inliers), cost_function and pose_covariance take it without a wait; `offsets`,
        num_correspondences and the calls that size per-correspondence outputs (residuals, triangulate, relative_scale,
        want_inliers) wait once for the stream and fetch the sizes.  reshape() makes it an exact batch again."""
        on_device = self._on_device = _is_torch(pts1)
        xp = __import__("torch") if on_device else np

        def c3(a):
            if a is not None and a.ndim == 3:  # [R,2,2] -> (xx, xy, yy)
                a = xp.stack([a[:, 0, 0], a[:, 1, 0], a[:, 1, 1]], -1)
            return a
        P, R = self.n_pairs, int(pts1.shape[0])
        ptrs, keep = [], []
        for a, width in ((pts1, 2), (pts2, 2), (c3(cov2), 3), (c3(cov1), 3)):
            if a is None:
                ptrs.append(None)
                continue
            if on_device:
                a = self._dev_tensor(a, "keypoint array")
                ptrs.append(a.data_ptr())
            else:
                a = np.ascontiguousarray(a, dtype=np.float64)
                ptrs.append(a.ctypes.data)
            if int(np.prod(a.shape)) != R * width:
                raise ValueError(f"expected {R}x{width} values, got {tuple(a.shape)}")
            keep.append(a)
        if on_device:
            import torch
            off = self._dev_tensor(offsets, "offsets", (P + 1,), dtype=torch.int64)
            if dropped is not None:
                self._dev_out(dropped, "dropped", (P,), torch.int32)
            po, pd = off.data_ptr(), None if dropped is None else dropped.data_ptr()
        else:
            off = np.ascontiguousarray(offsets, dtype=np.int64)
            if off.shape != (P + 1,):
                raise ValueError(f"offsets: expected shape ({P + 1},), got {off.shape}")
            if dropped is not None and not (isinstance(dropped, np.ndarray) and dropped.dtype == np.int32
                                            and dropped.shape == (P,) and dropped.flags.c_contiguous):
                raise ValueError(f"dropped: need a C-contiguous int32 array of shape ({P},)")
            po, pd = off.ctypes.data, None if dropped is None else dropped.ctypes.data
        Kd, kp, space, stream = self._kinv_arg(K_inv, on_device)
        capi.check(self._lib.pnec_hip_problem_fill_keypoints_ragged(self._h, po, R, ptrs[0], ptrs[1], ptrs[2], ptrs[3], kp,
                                                                    float(kappa), 1, pd, space, stream))
        self._offsets = None   # (the sizes are the device's: fetched from the library on first use, which waits)
        return self

    def export_payload(self) -> np.ndarray:
        """The SoA planes as they sit in HBM (float64 [payload_doubles]); for tests."""
        out = np.empty(self._lib.pnec_hip_problem_payload_doubles(self._h))
        capi.check(self._lib.pnec_hip_problem_export_payload(self._h, out.ctypes.data, capi.MEM_HOST, None))
        return out

    # -- solve ------------------------------------------------------------------------------
    def solve(self, init_q, init_t=None, reg: float = 1e-13,
              options: capi.Options | None = None, hyp_t=None, n_hyp: int = 1,
              out: SolveResult | None = None) -> SolveResult:
        """InitValues + Optimize + Result for every (pair, hypothesis) on the device."""
        on_device = _is_torch(init_q)
        n_hyp = int(n_hyp) if hyp_t is not None else 1
        if n_hyp < 1:
            raise ValueError("n_hyp must be >= 1")
        S = self.n_pairs * n_hyp
        if on_device:
            import torch
            init_q = self._dev_tensor(init_q, "init_q", (self.n_pairs, 4))
            init_t = self._dev_tensor(init_t, "init_t", (self.n_pairs, 3))
            hyp_t = self._dev_tensor(hyp_t, "hyp_t", (S, 3))
            dev = init_q.device
            f64 = dict(dtype=torch.float64, device=dev)
            if out is None:
                out = SolveResult(torch.empty((S, 4), **f64), torch.empty((S, 3), **f64),
                                  torch.empty((S,), **f64),
                                  torch.empty((S,), dtype=torch.int32, device=dev),
                                  torch.empty((S,), dtype=torch.int32, device=dev))
            else:
                self._dev_out(out.q, "q", (S, 4), torch.float64)
                self._dev_out(out.t, "t", (S, 3), torch.float64)
                self._dev_out(out.cost, "cost", (S,), torch.float64)
                self._dev_out(out.iterations, "iterations", (S,), torch.int32)
                self._dev_out(out.status, "status", (S,), torch.int32)
            p = lambda a: None if a is None else a.data_ptr()
            stream = torch.cuda.current_stream(self.device).cuda_stream
            space = capi.MEM_DEVICE
        else:
            init_q = np.ascontiguousarray(init_q, dtype=np.float64)
            init_t = None if init_t is None else np.ascontiguousarray(init_t, dtype=np.float64)
            hyp_t = None if hyp_t is None else np.ascontiguousarray(hyp_t, dtype=np.float64)
            if out is None:
                out = SolveResult(np.empty((S, 4)), np.empty((S, 3)), np.empty(S),
                                  np.empty(S, dtype=np.int32), np.empty(S, dtype=np.int32))
            else:
                for name, shape, dt in (("q", (S, 4), np.float64), ("t", (S, 3), np.float64), ("cost", (S,), np.float64),
                                        ("iterations", (S,), np.int32), ("status", (S,), np.int32)):
                    a = getattr(out, name)
                    if not (isinstance(a, np.ndarray) and a.dtype == dt and a.shape == shape and a.flags.c_contiguous):
                        raise ValueError(f"out.{name}: need a C-contiguous {np.dtype(dt).name} array of shape {shape}")
            p = lambda a: None if a is None else a.ctypes.data
            stream = None
            space = capi.MEM_HOST
        if tuple(init_q.shape) != (self.n_pairs, 4):
            raise ValueError("init_q must be [n_pairs,4] (xyzw)")
        if init_t is not None and tuple(init_t.shape) != (self.n_pairs, 3):
            raise ValueError("init_t must be [n_pairs,3]")
        if hyp_t is not None and tuple(hyp_t.shape) != (S, 3):
            raise ValueError("hyp_t must be [n_pairs*n_hyp,3]")
        capi.check(self._lib.pnec_hip_solve(
            self._h, p(init_q), p(init_t), int(n_hyp), p(hyp_t), float(reg),
            C.byref(options) if options is not None else None, p(out.q), p(out.t), p(out.cost),
            p(out.iterations), p(out.status), space, stream))
        out.batch, out.reg, out.n_hyp = self, float(reg), int(n_hyp)
        return out

    def _front(self, weighted, init_q, init_t, reg, weighted_iterations):
        on_device = _is_torch(init_q)
        if on_device:
            import torch
            keep = [self._dev_tensor(init_q, "init_q", (self.n_pairs, 4)),
                    self._dev_tensor(init_t, "init_t", (self.n_pairs, 3))]
            f64 = dict(dtype=torch.float64, device=keep[0].device)
            oq, ot = torch.empty((self.n_pairs, 4), **f64), torch.empty((self.n_pairs, 3), **f64)
            stream, space = torch.cuda.current_stream(self.device).cuda_stream, capi.MEM_DEVICE
            pq, pt = keep[0].data_ptr(), (None if keep[1] is None else keep[1].data_ptr())
        else:
            keep = [np.ascontiguousarray(init_q, dtype=np.float64),
                    None if init_t is None else np.ascontiguousarray(init_t, dtype=np.float64)]
            oq, ot = np.empty((self.n_pairs, 4)), np.empty((self.n_pairs, 3))
            stream, space = None, capi.MEM_HOST
            pq, pt = keep[0].ctypes.data, (None if keep[1] is None else keep[1].ctypes.data)
        po, pto = (oq.data_ptr(), ot.data_ptr()) if on_device else (oq.ctypes.data, ot.ctypes.data)
        if weighted:
            capi.check(self._lib.pnec_hip_weighted_eigensolver(self._h, pq, pt, float(reg),
                                                              int(weighted_iterations), po, pto, space, stream))
        else:
            capi.check(self._lib.pnec_hip_nec_eigensolver(self._h, pq, po, pto, space, stream))
        return oq, ot

    def ransac_eigensolver(self, init_q, seed: int = 1, max_iterations: int = 5000, sample_size: int = 10,
                           threshold: float = 1e-6):
        """PNEC::Eigensolver with RANSAC (pnec.cc:239-272): -> (q, t, inlier_mask [sumN] uint8,
        inlier_count [P], ransac_iterations [P])"""
        M, P = self.num_correspondences, self.n_pairs
        if _is_torch(init_q):
            import torch
            init_q = self._dev_tensor(init_q, "init_q", (P, 4))
            dev = init_q.device
            q = torch.empty((P, 4), dtype=torch.float64, device=dev)
            t = torch.empty((P, 3), dtype=torch.float64, device=dev)
            mask = torch.empty((max(M, 1),), dtype=torch.uint8, device=dev)
            cnt = torch.empty((P,), dtype=torch.int32, device=dev)
            its = torch.empty((P,), dtype=torch.int32, device=dev)
            iq = init_q.contiguous()
            capi.check(self._lib.pnec_hip_ransac_eigensolver(
                self._h, iq.data_ptr(), int(seed), int(max_iterations), int(sample_size), float(threshold),
                q.data_ptr(), t.data_ptr(), mask.data_ptr(), cnt.data_ptr(), its.data_ptr(), capi.MEM_DEVICE,
                torch.cuda.current_stream(self.device).cuda_stream))
            return q, t, mask[:M], cnt, its
        iq = np.ascontiguousarray(init_q, dtype=np.float64)
        q, t = np.empty((P, 4)), np.empty((P, 3))
        mask = np.zeros(max(M, 1), dtype=np.uint8)
        cnt, its = np.zeros(P, dtype=np.int32), np.zeros(P, dtype=np.int32)
        capi.check(self._lib.pnec_hip_ransac_eigensolver(
            self._h, iq.ctypes.data, int(seed), int(max_iterations), int(sample_size), float(threshold),
            q.ctypes.data, t.ctypes.data, mask.ctypes.data, cnt.ctypes.data, its.ctypes.data, capi.MEM_HOST, None))
        return q, t, mask[:M], cnt, its

    def launch_order_hint(self, enable: bool = True) -> None:
        """Opt in to pnec_hip_problem_launch_order_hint: the next RANSAC launch on this batch dispatches the pairs that
        needed more than one round of hypotheses in the last one first (scheduling only; results do not change)."""
        capi.check(self._lib.pnec_hip_problem_launch_order_hint(self._h, 1 if enable else 0))

    def set_eigensolver_scheme(self, scheme: int) -> None:
        """Which iteration the eigenvalue minimisations of the STAGE calls on this batch run (capi.ES_NEWTON / ES_DESCENT /
        ES_LM; include/pnec_hip.h pnec_hip_eigensolver_scheme).  solve_pipeline takes its own from the options."""
        capi.check(self._lib.pnec_hip_problem_set_eigensolver_scheme(self._h, int(scheme)))

    def set_ransac_flags(self, flags: int) -> None:
        """PNEC_HIP_RANSAC_* bits for the STAGE call ransac_eigensolver on this batch (capi.RANSAC_CHAINED_STARTS: every
        hypothesis starts from the last scored model's rotation, opengv's adapter side effect [EXT]; one hypothesis per
        round).  solve_pipeline takes its own from the options' ransac_flags."""
        capi.check(self._lib.pnec_hip_problem_set_ransac_flags(self._h, int(flags)))

    def select(self, mask, view: bool = False) -> "Batch":
        """PNEC::InlierExtraction (pnec.cc:210-229): new Batch with the masked correspondences.
        view=True: into this batch's cached target (pnec_hip_problem_select_view: nothing allocated after the first
        call, the result belongs to this batch and is replaced by the next such call)."""
        h = C.c_void_p()
        M = self.num_correspondences
        fn = self._lib.pnec_hip_problem_select_view if view else self._lib.pnec_hip_problem_select
        if _is_torch(mask):
            import torch
            m = mask if mask.dtype == torch.uint8 else (mask != 0).to(torch.uint8)
            m = self._dev_tensor(m, "mask", (M,), dtype=torch.uint8)
            capi.check(fn(self._h, m.data_ptr(), capi.MEM_DEVICE, torch.cuda.current_stream(self.device).cuda_stream,
                          C.byref(h)))
        else:
            m = np.ascontiguousarray(mask, dtype=np.uint8)
            if m.shape != (M,):
                raise ValueError(f"mask: expected shape ({M},), got {m.shape}")
            capi.check(fn(self._h, m.ctypes.data, capi.MEM_HOST, None, C.byref(h)))
        out = Batch.__new__(Batch)
        out._borrowed = bool(view)
        out._on_device = _is_torch(mask)
        out._lib, out.mode, out.device, out._h = self._lib, self.mode, self.device, h
        if view:
            # the view lives in this batch's cached target: keep the source alive as long as the view is, and retire
            # the previous view object (the library has just re-pointed the handle it held)
            out._source = self
            old = getattr(self, "_last_view", None)
            old = old() if old is not None else None
            if old is not None:
                old._h = None
            import weakref
            self._last_view = weakref.ref(out)
        out.n_pairs = self.n_pairs
        # InlierExtraction ran on the device and nothing was read back: the new batch's offsets are
        # fetched from the library on first use (that call waits for the stream)
        out._offsets = None
        return out

    def solve_pipeline(self, init_q, init_t, options: capi.PipelineOptions | None = None, want_inliers: bool = False):
        """PNEC::Solve (pnec.cc:77-124) for every pair, all stages on the device without a host round
        trip: -> (q [P,4], t [P,3]) or, with want_inliers, (q, t, inlier_mask [sumN] uint8, inlier_count [P])."""
        P = self.n_pairs
        opt = C.byref(options) if options is not None else None
        if _is_torch(init_q):
            import torch
            iq = self._dev_tensor(init_q, "init_q", (P, 4))
            it = self._dev_tensor(init_t, "init_t", (P, 3))
            q = torch.empty((P, 4), dtype=torch.float64, device=iq.device)
            t = torch.empty((P, 3), dtype=torch.float64, device=iq.device)
            mask = cnt = None
            if want_inliers:
                mask = torch.empty((max(self.num_correspondences, 1),), dtype=torch.uint8, device=iq.device)
                cnt = torch.empty((P,), dtype=torch.int32, device=iq.device)
            capi.check(self._lib.pnec_hip_solve_pipeline(
                self._h, iq.data_ptr(), it.data_ptr(), opt, q.data_ptr(), t.data_ptr(),
                None if mask is None else mask.data_ptr(), None if cnt is None else cnt.data_ptr(), capi.MEM_DEVICE,
                torch.cuda.current_stream(self.device).cuda_stream))
            return (q, t, mask[:self.num_correspondences], cnt) if want_inliers else (q, t)
        iq = np.ascontiguousarray(init_q, dtype=np.float64)
        it = np.ascontiguousarray(init_t, dtype=np.float64)
        if iq.shape != (P, 4) or it.shape != (P, 3):
            raise ValueError("init_q must be [n_pairs,4], init_t [n_pairs,3]")
        q, t = np.empty((P, 4)), np.empty((P, 3))
        mask = np.zeros(max(self.num_correspondences, 1), dtype=np.uint8) if want_inliers else None
        cnt = np.zeros(P, dtype=np.int32) if want_inliers else None
        capi.check(self._lib.pnec_hip_solve_pipeline(
            self._h, iq.ctypes.data, it.ctypes.data, opt, q.ctypes.data, t.ctypes.data,
            None if mask is None else mask.ctypes.data, None if cnt is None else cnt.ctypes.data, capi.MEM_HOST, None))
        return (q, t, mask[:self.num_correspondences], cnt) if want_inliers else (q, t)

    def nec_eigensolver(self, init_q):
        """PNEC::Eigensolver without RANSAC (pnec.cc:273-278): -> (q [P,4], t [P,3])"""
        return self._front(False, init_q, None, 0.0, 0)

    def weighted_eigensolver(self, init_q, init_t, reg: float = 1e-13, weighted_iterations: int = 10):
        """PNEC::WeightedEigensolver (pnec.cc:283-348): -> (q [P,4], t [P,3])"""
        return self._front(True, init_q, init_t, reg, weighted_iterations)

    def cost_function(self, q, t):
        """pnec::common::CostFunction per pair (TARGET-mode batches)."""
        if _is_torch(q):
            import torch
            q = self._dev_tensor(q, "q", (self.n_pairs, 4))
            t = self._dev_tensor(t, "t", (self.n_pairs, 3))
            out = torch.empty((self.n_pairs,), dtype=torch.float64, device=q.device)
            capi.check(self._lib.pnec_hip_cost_function(
                self._h, q.data_ptr(), t.data_ptr(), out.data_ptr(),
                capi.MEM_DEVICE, torch.cuda.current_stream(self.device).cuda_stream))
            return out
        q = np.ascontiguousarray(q, dtype=np.float64)
        t = np.ascontiguousarray(t, dtype=np.float64)
        out = np.empty(self.n_pairs)
        capi.check(self._lib.pnec_hip_cost_function(self._h, q.ctypes.data, t.ctypes.data,
                                                    out.ctypes.data, capi.MEM_HOST, None))
        return out


    def pose_covariance(self, q, t, reg: float = 1e-13, n_hyp: int = 1) -> PoseCovariance:
        """6x6 covariance, Ceres-chart information, gradient and cost of every pair at the poses passed in: q [S,4]
        xyzw, t [S,3], S = n_pairs * n_hyp (pnec_hip_pose_covariance).  torch.cuda tensors in -> torch.cuda tensors out,
        asynchronous on torch's current stream; numpy in -> numpy out."""
        n_hyp = int(n_hyp)
        if n_hyp < 1:
            raise ValueError("n_hyp must be >= 1")
        S = self.n_pairs * n_hyp
        if _is_torch(q):
            import torch
            q = self._dev_tensor(q, "q", (S, 4))
            t = self._dev_tensor(t, "t", (S, 3))
            f64 = dict(dtype=torch.float64, device=q.device)
            cov, info = torch.empty((S, 6, 6), **f64), torch.empty((S, 15), **f64)
            grad, cost = torch.empty((S, 5), **f64), torch.empty((S,), **f64)
            status = torch.empty((S,), dtype=torch.int32, device=q.device)
            p = lambda a: a.data_ptr()
            space, stream = capi.MEM_DEVICE, torch.cuda.current_stream(self.device).cuda_stream
        else:
            q = np.ascontiguousarray(q, dtype=np.float64)
            t = np.ascontiguousarray(t, dtype=np.float64)
            if q.shape != (S, 4) or t.shape != (S, 3):
                raise ValueError("q must be [n_pairs*n_hyp,4] (xyzw), t [n_pairs*n_hyp,3]")
            cov, info, grad, cost = np.empty((S, 6, 6)), np.empty((S, 15)), np.empty((S, 5)), np.empty(S)
            status = np.empty(S, dtype=np.int32)
            p = lambda a: a.ctypes.data
            space, stream = capi.MEM_HOST, None
        capi.check(self._lib.pnec_hip_pose_covariance(self._h, p(q), p(t), n_hyp, float(reg), p(info), p(cov), p(grad),
                                                      p(cost), p(status), space, stream))
        return PoseCovariance(cov, expand_info(info), grad, cost, status)


    def pose_sensitivity(self, q, t, grad_pose, reg: float = 1e-13, n_hyp: int = 1, gauss_newton: bool = False,
                         zero_on_failure: bool = False) -> PoseSensitivity:
        """Gradient of a loss of the solved pose with respect to every bearing vector and covariance of its pair, by the
        implicit-function theorem at the poses passed in (pnec_hip_pose_sensitivity): q [S,4] xyzw, t [S,3], grad_pose
        [S,6] = (dL/d omega, dL/d t), S = n_pairs * n_hyp.  torch.cuda tensors in -> torch.cuda tensors out, asynchronous
        on torch's current stream; numpy in -> numpy out.  `gauss_newton`: J'J in place of the full Hessian (1 - 40 % off);
        `zero_on_failure`: a slot whose Hessian is not positive definite gives zeros, not NaN.  On a batch made by
        select() the call first reads that batch's offsets to size the outputs, as residuals() does."""
        n_hyp = int(n_hyp)
        if n_hyp < 1:
            raise ValueError("n_hyp must be >= 1")
        flags = (capi.SENS_GAUSS_NEWTON if gauss_newton else 0) | (capi.SENS_ZERO_ON_FAILURE if zero_on_failure else 0)
        S = self.n_pairs * n_hyp
        M = int(self.offsets[-1]) * n_hyp     # (a batch made by select: waits for its sizes)
        has_cov, has_host = self.mode != capi.MODE_NEC, self.mode == capi.MODE_SYM
        if _is_torch(q):
            import torch
            q = self._dev_tensor(q, "q", (S, 4))
            t = self._dev_tensor(t, "t", (S, 3))
            grad_pose = self._dev_tensor(grad_pose, "grad_pose", (S, 6))
            f64 = dict(dtype=torch.float64, device=q.device)
            new = lambda *shape: torch.empty(shape, **f64)
            status = torch.empty((S,), dtype=torch.int32, device=q.device)
            p = lambda a: None if a is None else a.data_ptr()
            space, stream = capi.MEM_DEVICE, torch.cuda.current_stream(self.device).cuda_stream
        else:
            q = np.ascontiguousarray(q, dtype=np.float64)
            t = np.ascontiguousarray(t, dtype=np.float64)
            grad_pose = np.ascontiguousarray(grad_pose, dtype=np.float64)
            if q.shape != (S, 4) or t.shape != (S, 3) or grad_pose.shape != (S, 6):
                raise ValueError("q must be [n_pairs*n_hyp,4] (xyzw), t [n_pairs*n_hyp,3], grad_pose [n_pairs*n_hyp,6]")
            new = lambda *shape: np.empty(shape)
            status = np.empty(S, dtype=np.int32)
            p = lambda a: None if a is None else a.ctypes.data
            space, stream = capi.MEM_HOST, None
        g1, g2 = new(M, 3), new(M, 3)
        gc = new(M, 3, 3) if has_cov else None
        gh = new(M, 3, 3) if has_host else None
        lam, hess, grad, newton = new(S, 5), new(S, 15), new(S, 5), new(S, 5)
        capi.check(self._lib.pnec_hip_pose_sensitivity(self._h, p(q), p(t), p(grad_pose), n_hyp, float(reg), flags, p(g1),
                                                       p(g2), p(gc), p(gh), p(lam), p(hess), p(grad), p(newton), p(status),
                                                       space, stream))
        return PoseSensitivity(g1, g2, gc, gh, lam, expand_info(hess), grad, newton, status)

    def residuals(self, q, t, reg: float = 1e-13, gate: float = 3.0, n_hyp: int = 1) -> ResidualReport:
        """Whitened residual, propagated variance and chi-square gate verdict (|r| <= gate, in sigmas) of every
        correspondence at the poses passed in, and the chi-square sums per slot: q [S,4] xyzw, t [S,3], S = n_pairs *
        n_hyp (pnec_hip_residuals).  torch.cuda tensors in -> torch.cuda tensors out, asynchronous on torch's current
        stream; numpy in -> numpy out.  With n_hyp == 1, `self.select(report.mask)` keeps the gated correspondences.
        On a batch made by select() the call first reads that batch's offsets (it sizes the outputs from them and
        returns them in the report), which waits once for the stream the selection ran on -- also with torch.cuda
        inputs; the C call itself, given DEVICE pointers, does not wait."""
        n_hyp = int(n_hyp)
        if n_hyp < 1:
            raise ValueError("n_hyp must be >= 1")
        gate = float(gate)
        if not gate >= 0.0:
            raise ValueError("gate must be >= 0 (sigmas)")
        S = self.n_pairs * n_hyp
        offsets = self.offsets     # (a batch made by select: waits for its sizes)
        M = int(offsets[-1]) * n_hyp
        if _is_torch(q):
            import torch
            q = self._dev_tensor(q, "q", (S, 4))
            t = self._dev_tensor(t, "t", (S, 3))
            f64 = dict(dtype=torch.float64, device=q.device)
            res, var = torch.empty((M,), **f64), torch.empty((M,), **f64)
            mask = torch.empty((M,), dtype=torch.uint8, device=q.device)
            chi2, gchi2, mx = torch.empty((S,), **f64), torch.empty((S,), **f64), torch.empty((S,), **f64)
            cnt = torch.empty((S,), dtype=torch.int32, device=q.device)
            p = lambda a: a.data_ptr()
            space, stream = capi.MEM_DEVICE, torch.cuda.current_stream(self.device).cuda_stream
        else:
            q = np.ascontiguousarray(q, dtype=np.float64)
            t = np.ascontiguousarray(t, dtype=np.float64)
            if q.shape != (S, 4) or t.shape != (S, 3):
                raise ValueError("q must be [n_pairs*n_hyp,4] (xyzw), t [n_pairs*n_hyp,3]")
            res, var, mask = np.empty(M), np.empty(M), np.empty(M, dtype=np.uint8)
            chi2, gchi2, mx, cnt = np.empty(S), np.empty(S), np.empty(S), np.empty(S, dtype=np.int32)
            p = lambda a: a.ctypes.data
            space, stream = capi.MEM_HOST, None
        capi.check(self._lib.pnec_hip_residuals(self._h, p(q), p(t), n_hyp, float(reg), gate, p(res), p(var), p(mask),
                                                p(chi2), p(gchi2), p(cnt), p(mx), space, stream))
        return ResidualReport(res, var, mask, chi2, gchi2, cnt, mx, offsets, n_hyp)

    def triangulate(self, q, t, n_hyp: int = 1, orient: bool = True) -> Triangulation:
        """Midpoint triangulation of every correspondence at the poses passed in, the cheirality vote per slot and the
        translation direction with the sign that puts the structure in front of both cameras: q [S,4] xyzw, t [S,3],
        S = n_pairs * n_hyp (pnec_hip_triangulate).  With `orient` the per-correspondence outputs are evaluated at the
        oriented direction (PNEC_HIP_TRI_ORIENT).  torch.cuda tensors in -> torch.cuda tensors out, asynchronous on
        torch's current stream; numpy in -> numpy out.  On a batch made by select() the call first reads that batch's
        offsets, as Batch.residuals does."""
        n_hyp = int(n_hyp)
        if n_hyp < 1:
            raise ValueError("n_hyp must be >= 1")
        flags = capi.TRI_ORIENT if orient else 0
        S = self.n_pairs * n_hyp
        offsets = self.offsets     # (a batch made by select: waits for its sizes)
        M = int(offsets[-1]) * n_hyp
        if _is_torch(q):
            import torch
            q = self._dev_tensor(q, "q", (S, 4))
            t = self._dev_tensor(t, "t", (S, 3))
            f64 = dict(dtype=torch.float64, device=q.device)
            i32 = dict(dtype=torch.int32, device=q.device)
            point = torch.empty((M, 3), **f64)
            d1, d2, psi, var = (torch.empty((M,), **f64) for _ in range(4))
            front = torch.empty((M,), dtype=torch.uint8, device=q.device)
            nf, nb, sign = (torch.empty((S,), **i32) for _ in range(3))
            to, mean = torch.empty((S, 3), **f64), torch.empty((S,), **f64)
            p = lambda a: a.data_ptr()
            space, stream = capi.MEM_DEVICE, torch.cuda.current_stream(self.device).cuda_stream
        else:
            q = np.ascontiguousarray(q, dtype=np.float64)
            t = np.ascontiguousarray(t, dtype=np.float64)
            if q.shape != (S, 4) or t.shape != (S, 3):
                raise ValueError("q must be [n_pairs*n_hyp,4] (xyzw), t [n_pairs*n_hyp,3]")
            point = np.empty((M, 3))
            d1, d2, psi, var = (np.empty(M) for _ in range(4))
            front = np.empty(M, dtype=np.uint8)
            nf, nb, sign = (np.empty(S, dtype=np.int32) for _ in range(3))
            to, mean = np.empty((S, 3)), np.empty(S)
            p = lambda a: a.ctypes.data
            space, stream = capi.MEM_HOST, None
        capi.check(self._lib.pnec_hip_triangulate(self._h, p(q), p(t), n_hyp, flags, p(point), p(d1), p(d2), p(psi),
                                                  p(var), p(front), p(nf), p(nb), p(sign), p(to), p(mean), space, stream))
        return Triangulation(point, d1, d2, psi, var, front, nf, nb, sign, to, mean, offsets, n_hyp)

    def eight_point(self, quality: str = "sample", on_device: bool | None = None) -> EightPoint:
        """The eight-point baseline (pnec_hip_eight_point): essential matrix and pose of every pair from its
        correspondences alone, no start pose.  quality="sample" scores the four decompositions on the pair's first
        min(9, N) correspondences as the reference does, "all" on all of them (PNEC_HIP_EP_QUALITY_ALL).  A batch filled
        or selected from torch.cuda tensors answers with torch.cuda tensors, asynchronous on torch's current stream; one
        filled from numpy answers with numpy arrays (`on_device` overrides).  Nothing is read back to size the outputs,
        also on a batch made by select()."""
        if quality not in ("sample", "all"):
            raise ValueError('quality must be "sample" or "all"')
        flags = capi.EP_QUALITY_ALL if quality == "all" else 0
        if on_device is None:
            on_device = bool(getattr(self, "_on_device", False))
        P = self.n_pairs
        if on_device:
            import torch
            f64 = dict(dtype=torch.float64, device=f"cuda:{self.device}")
            i32 = dict(dtype=torch.int32, device=f"cuda:{self.device}")
            q, t, E, sing = (torch.empty((P, w), **f64) for w in (4, 3, 9, 3))
            gap, qual = torch.empty((P,), **f64), torch.empty((P, 4), **f64)
            choice, status = torch.empty((P,), **i32), torch.empty((P,), **i32)
            p = lambda a: a.data_ptr()
            space, stream = capi.MEM_DEVICE, torch.cuda.current_stream(self.device).cuda_stream
        else:
            q, t, E, sing = (np.empty((P, w)) for w in (4, 3, 9, 3))
            gap, qual = np.empty(P), np.empty((P, 4))
            choice, status = np.empty(P, dtype=np.int32), np.empty(P, dtype=np.int32)
            p = lambda a: a.ctypes.data
            space, stream = capi.MEM_HOST, None
        capi.check(self._lib.pnec_hip_eight_point(self._h, flags, p(q), p(t), p(E), p(sing), p(gap), p(qual), p(choice),
                                                  p(status), space, stream))
        return EightPoint(q, t, E, sing, gap, qual, choice, status)

    def _essential_minimal(self, algorithm: int, quality: str, on_device) -> MinimalPose:
        if quality not in ("sample", "all"):
            raise ValueError('quality must be "sample" or "all"')
        flags = capi.EM_QUALITY_ALL if quality == "all" else 0
        if on_device is None:
            on_device = bool(getattr(self, "_on_device", False))
        P, S = self.n_pairs, capi.EM_MAX_SOLUTIONS
        shapes = ((P, 4), (P, 3), (P, 9), (P, 3), (P,), (P,), (P, S, 9), (P, S, 4), (P,), (P,))
        ints = (5, 8, 9)
        if on_device:
            import torch
            out = [torch.empty(sh, dtype=torch.int32 if i in ints else torch.float64, device=f"cuda:{self.device}")
                   for i, sh in enumerate(shapes)]
            ptrs = [o.data_ptr() for o in out]
            space, stream = capi.MEM_DEVICE, torch.cuda.current_stream(self.device).cuda_stream
        else:
            out = [np.empty(sh, dtype=np.int32 if i in ints else np.float64) for i, sh in enumerate(shapes)]
            ptrs = [o.ctypes.data for o in out]
            space, stream = capi.MEM_HOST, None
        capi.check(self._lib.pnec_hip_essential_minimal(self._h, algorithm, flags, *ptrs, space, stream))
        return MinimalPose(*out)

    def five_point(self, quality: str = "sample", on_device: bool | None = None) -> MinimalPose:
        """Nister's five-point solver (pnec_hip_essential_minimal with PNEC_HIP_EM_NISTER): up to ten essential matrices
        per pair and the pose chosen among their forty decompositions, no start pose.  quality="sample" scores them on
        the pair's first min(8, N) correspondences as the reference does, "all" on all of them.  Spaces as eight_point:
        torch.cuda tensors, asynchronous on torch's current stream, from a batch filled or selected from them, numpy
        arrays otherwise (`on_device` overrides); nothing is read back to size the outputs."""
        return self._essential_minimal(capi.EM_NISTER, quality, on_device)

    def seven_point(self, quality: str = "sample", on_device: bool | None = None) -> MinimalPose:
        """The seven-point solver (PNEC_HIP_EM_SEVENPT): one or three fundamental matrices per pair from the cubic
        det(W + aX) = 0 and the pose chosen among their decompositions; the sample is min(9, N).  Otherwise as
        five_point."""
        return self._essential_minimal(capi.EM_SEVENPT, quality, on_device)

    def essential_ransac(self, algorithm, seed: int = 1, max_iterations: int = 5000, threshold: float = 1e-6,
                         first_pair_id: int = 0, on_device: bool | None = None) -> EssentialRansac:
        """RANSAC around the five-point, seven-point or eight-point solver (pnec_hip_essential_ransac): a pose and an
        inlier mask per pair from its correspondences alone, no start rotation.  `algorithm` is "nister", "sevenpt" or
        "eightpt" (or capi.EM_NISTER / EM_SEVENPT / EM_EIGHTPT).  Pair p draws its samples from
        (seed, first_pair_id + p), so a pair taken alone with first_pair_id set to its index has the bits it had in the
        batch.  Spaces as eight_point (`on_device` overrides); the mask's length is the batch's number of
        correspondences, which a batch made by select() waits for."""
        alg = _ER_ALGORITHMS.get(algorithm.lower(), None) if isinstance(algorithm, str) else int(algorithm)
        if alg not in _ER_ALGORITHMS.values():
            raise ValueError('algorithm must be "nister", "sevenpt" or "eightpt"')
        if on_device is None:
            on_device = bool(getattr(self, "_on_device", False))
        P, M = self.n_pairs, self.num_correspondences
        shapes = ((P, 4), (P, 3), (P, 9), (P, 3), (max(M, 1),), (P,), (P,), (P,), (P,), (P,))
        if on_device:
            import torch
            kinds = (torch.float64,) * 4 + (torch.uint8,) + (torch.int32,) * 5
            out = [torch.empty(sh, dtype=k, device=f"cuda:{self.device}") for sh, k in zip(shapes, kinds)]
            ptrs = [o.data_ptr() for o in out]
            space, stream = capi.MEM_DEVICE, torch.cuda.current_stream(self.device).cuda_stream
        else:
            kinds = (np.float64,) * 4 + (np.uint8,) + (np.int32,) * 5
            out = [np.zeros(sh, dtype=k) for sh, k in zip(shapes, kinds)]
            ptrs = [o.ctypes.data for o in out]
            space, stream = capi.MEM_HOST, None
        capi.check(self._lib.pnec_hip_essential_ransac(self._h, alg, int(seed), int(first_pair_id), int(max_iterations),
                                                       float(threshold), *ptrs, space, stream))
        out[4] = out[4][:M]
        return EssentialRansac(*out)

    def relative_scale(self, prev, prev_pair, link, q, t, q_prev, t_prev, min_parallax: float = 0.0,
                       per_link: bool = True) -> RelativeScale:
        """The ratio of every pair's baseline to that of its previous pair, from the tracks both see
        (pnec_hip_relative_scale).  `prev` is the batch of previous pairs (may be `self`); prev_pair int64 [P] names, per
        pair of this batch, the pair of `prev` whose second camera is this pair's first (-1: none); link int32 [sum N]
        gives, per correspondence, the index of the same track within that previous pair (-1: not linked) --
        pnec_amd.tracks.Tracks.links() builds both.  q [P,4] / t [P,3] are this batch's poses, q_prev / t_prev those of
        `prev`; the translations must carry the sign that puts the structure in front (Triangulation.t).  min_parallax
        (radians) leaves out links whose parallax in either pair is smaller.  per_link=False skips the two
        per-correspondence outputs.  torch.cuda tensors in -> torch.cuda tensors out, asynchronous on torch's current
        stream; numpy in -> numpy out."""
        if not isinstance(prev, Batch):
            raise TypeError("prev must be a Batch (it may be this one)")
        min_parallax = float(min_parallax)
        if not (min_parallax >= 0.0) or not np.isfinite(min_parallax):
            raise ValueError("min_parallax must be >= 0 and finite (radians)")
        P, Pp = self.n_pairs, prev.n_pairs
        offsets = self.offsets     # (a batch made by select: waits for its sizes)
        M = int(offsets[-1])
        if _is_torch(q):
            import torch
            q = self._dev_tensor(q, "q", (P, 4))
            t = self._dev_tensor(t, "t", (P, 3))
            q_prev = self._dev_tensor(q_prev, "q_prev", (Pp, 4))
            t_prev = self._dev_tensor(t_prev, "t_prev", (Pp, 3))
            dev = q.device
            as_dev = lambda a, dt: a.to(device=dev, dtype=dt).contiguous() if _is_torch(a) else \
                torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
            prev_pair, link = as_dev(prev_pair, torch.int64), as_dev(link, torch.int32)
            f64 = dict(dtype=torch.float64, device=dev)
            scale = torch.empty((P, 3), **f64)
            nl, nu = (torch.empty((P,), dtype=torch.int32, device=dev) for _ in range(2))
            ratio = torch.empty((M,), **f64) if per_link else None
            used = torch.empty((M,), dtype=torch.uint8, device=dev) if per_link else None
            p = lambda a: None if a is None else a.data_ptr()
            space, stream = capi.MEM_DEVICE, torch.cuda.current_stream(self.device).cuda_stream
        else:
            q, t, q_prev, t_prev = (np.ascontiguousarray(a, dtype=np.float64) for a in (q, t, q_prev, t_prev))
            if q.shape != (P, 4) or t.shape != (P, 3) or q_prev.shape != (Pp, 4) or t_prev.shape != (Pp, 3):
                raise ValueError("q must be [n_pairs,4] (xyzw), t [n_pairs,3]; q_prev / t_prev one per pair of prev")
            prev_pair = np.ascontiguousarray(prev_pair, dtype=np.int64)
            link = np.ascontiguousarray(link, dtype=np.int32)
            scale = np.empty((P, 3))
            nl, nu = (np.empty(P, dtype=np.int32) for _ in range(2))
            ratio = np.empty(M) if per_link else None
            used = np.empty(M, dtype=np.uint8) if per_link else None
            p = lambda a: None if a is None else a.ctypes.data
            space, stream = capi.MEM_HOST, None
        if tuple(prev_pair.shape) != (P,) or tuple(link.shape) != (M,):
            raise ValueError("prev_pair must be [n_pairs], link [sum N] (one entry per correspondence of this batch)")
        capi.check(self._lib.pnec_hip_relative_scale(self._h, prev._h, p(prev_pair), p(link), p(q), p(t), p(q_prev),
                                                     p(t_prev), min_parallax, p(ratio), p(used), p(scale), p(nl), p(nu),
                                                     space, stream))
        return RelativeScale(scale[:, 1], scale[:, 0], scale[:, 2], nl, nu, ratio, used, offsets)


def select_best(cost, n_hyp: int, device: int = 0):
    """Index of the lowest-cost hypothesis per pair."""
    L = capi.lib()
    if _is_torch(cost):
        import torch
        n_pairs = cost.numel() // n_hyp
        best = torch.empty((n_pairs,), dtype=torch.int32, device=cost.device)
        capi.check(L.pnec_hip_select_best(n_pairs, n_hyp, cost.contiguous().data_ptr(),
                                          best.data_ptr(), capi.MEM_DEVICE, device,
                                          torch.cuda.current_stream(device).cuda_stream))
        return best
    cost = np.ascontiguousarray(cost, dtype=np.float64)
    n_pairs = cost.size // n_hyp
    best = np.empty(n_pairs, dtype=np.int32)
    capi.check(L.pnec_hip_select_best(n_pairs, n_hyp, cost.ctypes.data, best.ctypes.data,
                                      capi.MEM_HOST, device, None))
    return best
