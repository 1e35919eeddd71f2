"""pnec_hip_patch_covariance on the device against `patch_cov_np` (tests/test_patch_covariance_cpu.py), the plain-numpy
statement of the definition in include/pnec_hip.h.

Bounds (tests/test_pose_covariance_gpu.py's): the Hessian within 1e-10 after normalising by sqrt(H_aa H_bb);
the covariance within 2 kappa 1e-10 after normalising by sqrt(S_aa S_bb), kappa the condition number of the Jacobi-scaled
H -- the first-order bound of an inverse whose argument is off by 1e-10; the textures are smoothed noise for which
kappa < 1e6 on every OK keypoint, asserted.  n_valid and status must be equal.  Where the test says "same bits" it
compares bit patterns.  Shapes are the smallest that reach every path: a 24 x 32 image holds Pattern52 with a few pixels
to spare, 16 keypoints fill a block, 65 and 130 cross blocks.

Pattern52's outermost column / row holds four points, so an image border cannot leave 49, 50 or 51 of its points valid;
test 1 therefore sweeps the borders twice: with Pattern52 (every count the grid search finds, 1 .. 48) and with a slightly
sheared copy whose 52 abscissae and ordinates all differ (every count from 1 to 51 at each of the four borders).
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_patch_covariance_cpu import (EDGE_H, EDGE_PITCH, EDGE_W, PATTERN_SKEW, check_against_np, edge_image,  # noqa: E402
                                       edge_points, patch_cov_np, skew_points, texture)

from pnec_amd import Batch, capi, patch_covariance, patches  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps


def _torch():
    import torch
    return torch


def _np(r):
    """a PatchCovariance of device tensors as a dict of numpy arrays"""
    return {k: getattr(r, k).cpu().numpy() for k in ("cov", "hessian", "mean", "n_valid", "status")}


def _same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"{what}: bits differ in {int((a != b).sum())} entries"


def _assert_kappa(ref):
    ok = ref["status"] == patches.PATCH_OK
    assert ok.any() and np.all(ref["kappa"][ok] < 1e6), float(np.max(ref["kappa"][ok]))


# ---- 1. every edge of one small image ---------------------------------------------------------------------------------
def test_edges_of_a_24x32_float32_image_with_pitch_40():
    torch = _torch()
    buf = edge_image()
    # the device buffer ends with the last pixel of the last row: no slack behind it
    flat = torch.from_numpy(buf.reshape(-1)[: (EDGE_H - 1) * EDGE_PITCH + EDGE_W].copy()).cuda()
    img = flat.as_strided((EDGE_H, EDGE_W), (EDGE_PITCH, 1))
    for pattern, (pts, _), what in ((patches.PATTERN52, edge_points(), "Pattern52"),
                                    (PATTERN_SKEW, (skew_points()[0], None), "sheared pattern")):
        ref = patch_cov_np(buf[:, :EDGE_W], pts, pattern=pattern)
        _assert_kappa(ref)
        got = patch_covariance(img, torch.from_numpy(pts).cuda(), pattern=pattern)
        assert got.cov.is_cuda and got.cov.dtype == torch.float64 and tuple(got.cov.shape) == (len(pts), 3)
        assert got.status.dtype == torch.int32 and got.n_valid.dtype == torch.int32
        check_against_np(_np(got), ref, f"edges, {what}, {len(pts)} keypoints")
        # (Pattern52's list holds a centre outside the image and a NaN: EMPTY; both hold counts below three: SINGULAR)
        want = {patches.PATCH_OK, patches.PATCH_SINGULAR} | ({patches.PATCH_EMPTY} if pattern is patches.PATTERN52 else set())
        assert set(ref["status"].tolist()) == want
    # the padding of the pitch (-1e6) and whatever lies behind the image never reached a sum
    assert float(got.mean[torch.isfinite(got.mean)].min()) > 0.0


# ---- 2. ragged batches, alone / in a batch, HOST / DEVICE ---------------------------------------------------------------
def _ragged_call(seed, counts, h=40, w=48):
    rng = np.random.default_rng(seed)
    images = np.stack([np.round(texture(h, w, seed + 10 * f)).astype(np.uint8) for f in range(len(counts))])
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    pts = np.stack([rng.uniform(-1.0, w + 1.0, offsets[-1]), rng.uniform(-1.0, h + 1.0, offsets[-1])], 1)
    pts[::3] = np.stack([rng.uniform(6.0, w - 7.0, len(pts[::3])), rng.uniform(6.0, h - 7.0, len(pts[::3]))], 1)
    ang = rng.uniform(-3.0, 3.0, offsets[-1])
    return images, offsets, pts, ang


@pytest.mark.parametrize("seed,counts", [(1, (0, 1, 63)), (2, (64, 65, 130))])
def test_ragged_batches_match_numpy_alone_and_in_the_batch_host_and_device(seed, counts):
    torch = _torch()
    images, offsets, pts, ang = _ragged_call(seed, counts)
    ref = patch_cov_np(images, pts, offsets, angle=ang)
    _assert_kappa(ref)
    dev = patch_covariance(torch.from_numpy(images).cuda(), torch.from_numpy(pts).cuda(), torch.from_numpy(offsets).cuda(),
                           angle=torch.from_numpy(ang).cuda())
    got = _np(dev)
    check_against_np(got, ref, f"ragged {counts}")
    host = patch_covariance(images, pts, offsets, angle=ang)
    assert isinstance(host.cov, np.ndarray)
    for k in ("cov", "hessian", "mean", "n_valid", "status"):
        _same_bits(getattr(host, k), got[k], f"HOST against DEVICE space, {k}")
    # a keypoint alone (its image alone) gives the bits it has inside the batch
    for f in range(len(counts)):
        for k in sorted({int(offsets[f]), int(offsets[f + 1]) - 1} if counts[f] else set()):
            one = patch_covariance(torch.from_numpy(images[f]).cuda(), torch.from_numpy(pts[k:k + 1]).cuda(),
                                   angle=torch.from_numpy(ang[k:k + 1]).cuda())
            for name, arr in _np(one).items():
                _same_bits(arr, got[name][k:k + 1], f"keypoint {k} alone, {name}")


# ---- 3. pixel types ---------------------------------------------------------------------------------------------------
def test_uint8_uint16_and_float32_give_the_same_bits():
    torch = _torch()
    images, offsets, pts, _ = _ragged_call(5, (20, 17))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    r8 = _np(patch_covariance(t(images), t(pts), t(offsets)))
    r16 = _np(patch_covariance(t(images.astype(np.uint16) << 8), t(pts), t(offsets)))
    r32 = _np(patch_covariance(t(images.astype(np.float32)), t(pts), t(offsets)))
    check_against_np(r8, patch_cov_np(images, pts, offsets), "uint8")
    assert (r8["status"] == patches.PATCH_OK).sum() >= 12
    for other, what in ((r16, "uint16 << 8"), (r32, "float32")):
        for k in ("cov", "hessian", "n_valid", "status"):
            _same_bits(other[k], r8[k], f"{what} against uint8, {k}")
    _same_bits(r32["mean"], r8["mean"], "float32 against uint8, mean")
    _same_bits(r16["mean"], 256.0 * r8["mean"], "uint16 << 8 against uint8, mean * 256")


# ---- 4. the angle -------------------------------------------------------------------------------------------------------
def test_the_angle_rotates_the_covariance_and_zero_is_no_angle():
    torch = _torch()
    images, offsets, pts, ang = _ragged_call(7, (40,))
    ang[:4] = (np.pi / 2, -np.pi, 1e-9, 2.5)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    plain = _np(patch_covariance(t(images), t(pts), t(offsets)))
    zero = _np(patch_covariance(t(images), t(pts), t(offsets), angle=t(np.zeros(len(pts)))))
    for k in plain:
        _same_bits(zero[k], plain[k], f"angle = 0 against no angle, {k}")
    rot = _np(patch_covariance(t(images), t(pts), t(offsets), angle=t(ang)))
    for k in ("hessian", "mean", "n_valid", "status"):
        _same_bits(rot[k], plain[k], f"the angle touches the covariance only, {k}")
    ok = plain["status"] == patches.PATCH_OK
    assert ok.sum() >= 12 and np.all(np.isnan(rot["cov"][~ok]))
    worst = 0.0
    for k in np.flatnonzero(ok):
        xx, xy, yy = (np.longdouble(v) for v in plain["cov"][k])
        c, s = np.cos(np.longdouble(ang[k])), np.sin(np.longdouble(ang[k]))
        S = np.array([[xx, xy], [xy, yy]], dtype=np.longdouble)
        R = np.array([[c, -s], [s, c]], dtype=np.longdouble)
        want = R @ S @ R.T
        norm = float(np.linalg.norm(S.astype(np.float64), 2))      # |Sigma|: the spectral norm
        err = max(abs(float(rot["cov"][k, 0] - want[0, 0])), abs(float(rot["cov"][k, 1] - want[0, 1])),
                  abs(float(rot["cov"][k, 2] - want[1, 1])))
        worst = max(worst, err / norm)
    print(f"rotation: worst |Sigma' - R Sigma R'| / |Sigma| = {worst / EPS:.2f} eps (bound 8 eps)")
    assert worst <= 8.0 * EPS


# ---- 5. degenerate images and pattern sizes -----------------------------------------------------------------------------
def test_constant_and_zero_images_one_pattern_point_and_too_many():
    torch = _torch()
    pts = np.array([[12.0, 11.0], [14.6, 9.3], [3.0, 3.0]])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    for image, status in ((np.full((24, 32), 77, dtype=np.uint8), patches.PATCH_SINGULAR),
                          (np.zeros((24, 32), dtype=np.uint8), patches.PATCH_EMPTY)):
        got = _np(patch_covariance(t(image), t(pts)))
        ref = patch_cov_np(image, pts)
        assert np.all(got["status"] == status) and np.all(np.isnan(got["cov"]))
        assert np.array_equal(got["n_valid"], ref["n_valid"]) and np.array_equal(got["status"], ref["status"])
    yy, xx = np.mgrid[0:24, 0:32]
    ramp = (10 + 3 * xx).astype(np.uint8)
    got = _np(patch_covariance(t(ramp), t(pts[:2])))
    assert np.all(got["status"] == patches.PATCH_SINGULAR) and np.all(np.isnan(got["cov"])) and np.all(got["hessian"][:, 3] == 0)
    # P = 1 runs: one point cannot give a covariance, the mean is the interpolated value
    image = np.round(texture(24, 32, 9)).astype(np.uint8)
    one = np.array([[0.5, -0.25]])
    got = _np(patch_covariance(t(image), t(pts), pattern=one))
    ref = patch_cov_np(image, pts, pattern=one)
    check_against_np(got, ref, "P = 1")
    assert np.all(got["n_valid"] == 1) and np.all(got["status"] == patches.PATCH_SINGULAR)
    # P = 64 runs and is right; P = 65 is refused
    rng = np.random.default_rng(3)
    p64 = rng.uniform(-3.5, 3.5, (64, 2))
    ref = patch_cov_np(image, pts, pattern=p64)
    _assert_kappa(ref)
    check_against_np(_np(patch_covariance(t(image), t(pts), pattern=p64)), ref, "P = 64")
    with pytest.raises(capi.PnecHipError) as e:
        patch_covariance(t(image), t(pts), pattern=rng.uniform(-3.5, 3.5, (65, 2)))
    assert e.value.code == capi.ERR_INVALID_ARGUMENT and "n_pattern" in str(e.value)


# ---- 6. into the keypoint ingest and a solve ------------------------------------------------------------------------------
def test_the_device_covariances_go_into_fill_keypoints_as_they_are_and_a_solve_runs():
    torch = _torch()
    rng = np.random.default_rng(17)
    h, w, n = 120, 160, 90
    K = np.array([[110.0, 0.0, 80.0], [0.0, 110.0, 60.0], [0.0, 0.0, 1.0]])
    X = np.stack([rng.uniform(-2.0, 2.0, n), rng.uniform(-1.5, 1.5, n), rng.uniform(4.0, 9.0, n)], 1)
    p1 = X @ K.T
    p1 = p1[:, :2] / p1[:, 2:]
    X2 = X - np.array([0.3, 0.02, 0.05])                                   # camera 2 moved, no rotation
    p2 = X2 @ K.T
    p2 = p2[:, :2] / p2[:, 2:]
    keep = (p2[:, 0] >= 6) & (p2[:, 0] < w - 7) & (p2[:, 1] >= 6) & (p2[:, 1] < h - 7)
    p1, p2 = np.ascontiguousarray(p1[keep]), np.ascontiguousarray(p2[keep])
    n = len(p2)
    assert n >= 40
    image2 = np.round(texture(h, w, 23)).astype(np.uint8)
    pc = patch_covariance(torch.from_numpy(image2).cuda(), torch.from_numpy(p2).cuda())
    assert bool((pc.status == patches.PATCH_OK).all()) and pc.cov.is_cuda
    check_against_np(_np(pc), patch_cov_np(image2, p2), "end to end")
    Kinv = np.linalg.inv(K)
    on_dev = Batch.uniform(capi.MODE_TARGET, 1, n)
    on_dev.fill_keypoints(torch.from_numpy(p1).cuda(), torch.from_numpy(p2).cuda(), pc.cov, K_inv=Kinv)
    torch.cuda.synchronize()
    on_host = Batch.uniform(capi.MODE_TARGET, 1, n)
    on_host.fill_keypoints(p1, p2, pc.cov.cpu().numpy(), K_inv=Kinv)
    _same_bits(on_dev.export_payload(), on_host.export_payload(), "payload from the device tensor against the host's numbers")
    q0 = torch.tensor([[0.0, 0.0, 0.0, 1.0]], dtype=torch.float64, device="cuda")
    t0 = torch.tensor([[1.0, 0.1, 0.1]], dtype=torch.float64, device="cuda")
    res = on_dev.solve(q0, t0)
    torch.cuda.synchronize()
    R = res.rotation_matrices().cpu().numpy()[0]
    tt = res.t.cpu().numpy()[0]
    assert np.all(np.isfinite(R)) and np.all(np.isfinite(tt)) and abs(np.linalg.norm(tt) - 1.0) < 1e-9
    assert np.isfinite(float(res.cost[0]))
    on_dev.close()
    on_host.close()
