"""The refinement as a differentiable torch function: poses out, gradients back onto bearing vectors and covariances.

Forward is the device solve (Batch.fill + Batch.solve); backward is ONE pnec_hip_pose_sensitivity call at the returned
pose -- the implicit-function theorem at the minimiser, no iteration unrolled (include/pnec_hip.h has the definitions).
torch is plumbing here as everywhere: device memory, streams and the autograd graph; the arithmetic is in
libpnec_hip.so.  Nothing is read back and nothing waits for the device.
"""
from __future__ import annotations

import numpy as np
import torch

from . import capi
from .batch import Batch


class _Solve(torch.autograd.Function):
    @staticmethod
    def forward(ctx, batch, reg, options, gauss_newton, init_q, init_t, bvs1, bvs2, covs, covs_host):
        det = lambda a: None if a is None else a.detach()
        batch.fill(det(bvs1), det(bvs2), det(covs), det(covs_host))
        res = batch.solve(det(init_q), det(init_t), reg=reg, options=options)
        ctx.batch, ctx.reg, ctx.gauss_newton = batch, float(reg), bool(gauss_newton)
        ctx.cov_shapes = tuple(None if a is None else tuple(a.shape) for a in (covs, covs_host))
        ctx.save_for_backward(res.q, res.t)
        # how converged the pose is, from the sensitivity's reduce phase alone (no per-correspondence output): only where
        # a gradient can be asked for
        S = res.q.shape[0]
        if any(ctx.needs_input_grad[6:]):
            newton = torch.empty((S, 5), dtype=torch.float64, device=res.q.device)
            sens_status = torch.empty((S,), dtype=torch.int32, device=res.q.device)
            flags = capi.SENS_ZERO_ON_FAILURE | (capi.SENS_GAUSS_NEWTON if gauss_newton else 0)
            zero = torch.zeros((S, 6), dtype=torch.float64, device=res.q.device)
            capi.check(capi.lib().pnec_hip_pose_sensitivity(
                batch._h, res.q.data_ptr(), res.t.data_ptr(), zero.data_ptr(), 1, float(reg), flags, None, None, None, None,
                None, None, None, newton.data_ptr(), sens_status.data_ptr(), capi.MEM_DEVICE,
                torch.cuda.current_stream(batch.device).cuda_stream))
        else:
            newton = torch.full((S, 5), float("nan"), dtype=torch.float64, device=res.q.device)
            sens_status = torch.full((S,), -1, dtype=torch.int32, device=res.q.device)
        ctx.mark_non_differentiable(res.cost, res.iterations, res.status, sens_status, newton)
        return res.q, res.t, res.cost, res.iterations, res.status, sens_status, newton

    @staticmethod
    def backward(ctx, grad_q, grad_t, *_):
        q, t = ctx.saved_tensors
        grad_q = torch.zeros_like(q) if grad_q is None else grad_q
        grad_t = torch.zeros_like(t) if grad_t is None else grad_t
        # R <- Exp(omega) R is q <- dq(omega) * q, dq = (omega / 2, 1) to first order:  dL/d omega from dL/dq, q = (v, w)
        v, w, gv, gw = q[:, :3], q[:, 3:], grad_q[:, :3], grad_q[:, 3:]
        g_omega = 0.5 * (w * gv + torch.linalg.cross(v, gv) - gw * v)
        grad_pose = torch.cat([g_omega, grad_t], dim=1).contiguous()
        s = ctx.batch.pose_sensitivity(q, t, grad_pose, reg=ctx.reg, gauss_newton=ctx.gauss_newton, zero_on_failure=True)
        like = lambda g, shape: None if shape is None or g is None else g.reshape(shape)   # (symmetric: [M,9] is either order)
        return (None, None, None, None, None, None, s.grad_bvs1, s.grad_bvs2, like(s.grad_covs, ctx.cov_shapes[0]),
                like(s.grad_covs_host, ctx.cov_shapes[1]))


def differentiable_solve(mode, offsets, bvs1, bvs2, covs=None, covs_host=None, init_q=None, init_t=None, reg: float = 1e-13,
                         options: capi.Options | None = None, batch: Batch | None = None, gauss_newton: bool = False):
    """Batch.solve with gradients: -> (q [P,4], t [P,3], info).

    bvs1, bvs2 [M,3], covs / covs_host [M,3,3] (or [M,9]) and init_q [P,4], init_t [P,3] are float64 torch.cuda tensors;
    `offsets` [P+1] are the pairs' bounds in M (host integers).  q and t carry a grad_fn: a loss of them back-propagates
    onto bvs1, bvs2, covs and covs_host through one pose_sensitivity call at the returned pose (full Hessian; J'J with
    `gauss_newton`).  The minimiser does not depend on where the iteration started, so init_q and init_t get no gradient.
    A pair whose Hessian at the returned pose is not positive definite (the solve stopped somewhere else than at a
    minimum) contributes zero gradient and says so in info["sens_status"].

    info: cost, iterations, status (the solve's), sens_status and newton (capi.SENS_NAMES and the Newton step x_N of
    pnec_hip_pose_sensitivity at the returned pose: how converged it is; filled in only when an input requires grad).
    None of them is differentiable.

    `batch`: a Batch of this mode and these offsets to fill and solve on; by default a private one per call, which lives
    as long as the graph.  A caller's batch must keep this call's contents until backward has run.
    """
    if init_q is None or init_t is None:
        raise ValueError("init_q [P,4] and init_t [P,3] are needed: the refinement starts from a pose")
    for name, a in (("bvs1", bvs1), ("bvs2", bvs2), ("covs", covs), ("covs_host", covs_host), ("init_q", init_q), ("init_t", init_t)):
        if a is not None and not (torch.is_tensor(a) and a.is_cuda and a.dtype == torch.float64):
            raise TypeError(f"{name}: a float64 torch.cuda tensor is needed")
    if batch is None:
        batch = Batch(mode, np.asarray(offsets, dtype=np.int64), device=bvs1.device.index)
    elif batch.mode != mode:
        raise ValueError("batch: a Batch of another residual family")
    q, t, cost, iterations, status, sens_status, newton = _Solve.apply(batch, reg, options, gauss_newton, init_q, init_t, bvs1,
                                                                        bvs2, covs, covs_host)
    return q, t, dict(cost=cost, iterations=iterations, status=status, sens_status=sens_status, newton=newton)
