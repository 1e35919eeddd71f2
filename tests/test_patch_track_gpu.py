"""pnec_hip_patch_track and pnec_hip_image_pyramid_level on the device against `patch_track_np` / `pyramid_np`
(tests/test_patch_track_cpu.py), the plain-numpy statements of the definitions in include/pnec_hip.h.

Bounds (DESIGN 9e's rule, not a new number): positions within 2 kappa 1e-10 px, angles within the same over the pattern's
radius, kappa the largest condition number of the Jacobi-scaled template Hessian over the keypoint's levels; dist2 within
the first-order propagation of the position bound.  Status and level must be equal, on ALL keypoints: none is excluded.
The pyramid must be equal to numpy's, bit for bit, in all three pixel types.  Where a test says "same bits" it compares bit
patterns.  Every fixture is 96 x 128 with three levels (24 x 32 at the top: the smallest at which a Pattern52 patch still
fits), three images, a few dozen keypoints.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_patch_track_cpu import (FAR, H0, LEVELS, OK, W0, check_track_against_np, main_fixture, main_reference,  # noqa: E402
                                  patch_track_np, pyramid_levels_np, pyramid_np, status_cases, status_references)

from pnec_amd import Batch, capi, image_pyramid, patch_covariance, patch_track, patches  # noqa: E402

pytestmark = pytest.mark.gpu

KEYS = ("pts", "angle", "cov", "dist2", "status", "lost_level")


def _torch():
    import torch
    return torch


def _t(a):
    return _torch().from_numpy(np.array(a)).cuda()        # (a copy: the fixtures are read-only)


def _np(r):
    """a PatchTrack as a dict of numpy arrays"""
    return {k: (getattr(r, k).cpu().numpy() if hasattr(getattr(r, k), "cpu") else np.asarray(getattr(r, k))) for k in KEYS}


def _same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"{what}: bits differ in {int((a != b).sum())} entries"


def _dev(kw):
    """the arguments of a case with every array on the device"""
    out = {}
    for k, v in kw.items():
        if k in ("tmpl", "next", "prev"):
            out[k] = None if v is None else [_t(a) for a in v]
        elif isinstance(v, np.ndarray):
            out[k] = _t(v)
        else:
            out[k] = v
    return out


# ---- 1. the main fixture, three pixel types ---------------------------------------------------------------------------
def test_main_fixture_in_three_pixel_types_against_numpy():
    fx, ref = main_fixture(), main_reference()
    assert fx["offsets"][1] == fx["offsets"][2]                     # ragged: the middle image has no keypoints
    got = {}
    for name, conv in (("uint8", lambda a: a), ("uint16 << 8", lambda a: a.astype(np.uint16) << 8),
                       ("float32", lambda a: a.astype(np.float32))):
        r = patch_track([_t(conv(a)) for a in fx["p1"]], [_t(conv(a)) for a in fx["p2"]], _t(fx["pts"]), _t(fx["offsets"]))
        assert r.pts.is_cuda and r.status.is_cuda
        got[name] = _np(r)
        check_track_against_np(got[name], ref, f"device, main fixture, {name}")
        ok = ref["status"] == OK
        assert np.all(np.isnan(got[name]["cov"][~ok])) and np.allclose(got[name]["cov"][ok], ref["cov"][ok], rtol=1e-6)
    for name in ("uint16 << 8", "float32"):
        for key in KEYS:
            _same_bits(got["uint8"][key], got[name][key], f"{key}: uint8 against {name}")


# ---- 2. every status, every level -------------------------------------------------------------------------------------
def test_status_fixture_against_numpy():
    refs = status_references()
    for name, kw in status_cases():
        got = _np(patch_track(**_dev(kw)))
        check_track_against_np(got, refs[name], f"device, status fixture '{name}'")
    a, d = refs["forward"], refs["strict"]
    assert np.all(d["status"][a["status"] == OK] == FAR)            # max_recovered_dist2 = 0: < is strict


# ---- 3. invariance ----------------------------------------------------------------------------------------------------
def test_alone_equals_in_the_batch_and_host_space_equals_device_space():
    fx = main_fixture()
    dev = _np(patch_track([_t(a) for a in fx["p1"]], [_t(a) for a in fx["p2"]], _t(fx["pts"]), _t(fx["offsets"])))
    host_r = patch_track(fx["p1"], fx["p2"], fx["pts"], fx["offsets"])
    assert isinstance(host_r.pts, np.ndarray)
    host = _np(host_r)
    for key in KEYS:
        _same_bits(dev[key], host[key], f"{key}: HOST space against DEVICE space")
    offs = fx["offsets"]
    for k in (0, 7, 21, 22, 39):
        f = int(np.searchsorted(offs, k, side="right") - 1)
        one = _np(patch_track([_t(a[f]) for a in fx["p1"]], [_t(a[f]) for a in fx["p2"]], _t(fx["pts"][k:k + 1])))
        for key in KEYS:
            _same_bits(one[key], dev[key][k:k + 1], f"{key}: keypoint {k} alone against inside the batch")


def test_no_backward_leaves_the_forward_outputs_bits_and_one_level_on_an_unmoved_image_returns_init():
    fx = main_fixture()
    args = ([_t(a) for a in fx["p1"]], [_t(a) for a in fx["p2"]], _t(fx["pts"]), _t(fx["offsets"]))
    both = _np(patch_track(*args))
    fwd = _np(patch_track(*args, backward=False))
    _same_bits(fwd["pts"], both["pts"], "pts without the backward track")
    _same_bits(fwd["angle"], both["angle"], "angle without the backward track")
    assert np.all(np.isnan(fwd["dist2"]))
    assert np.array_equal(fwd["status"], np.where(np.isin(both["status"], (FAR, patches.TRACK_LOST_BACKWARD)), OK, both["status"]))
    ok = both["status"] == OK
    _same_bits(fwd["cov"][ok], both["cov"][ok], "cov without the backward track")
    # one level, no shift, the same image: the residual is exactly zero at the start, so no iteration moves
    ang = np.zeros(len(fx["pts"]))
    same = _np(patch_track([_t(fx["p1"][0])], [_t(fx["p1"][0])], _t(fx["pts"]), _t(fx["offsets"]), init_angle=_t(ang)))
    assert np.all(same["status"] == OK)
    _same_bits(same["pts"], fx["pts"], "an unmoved image returns init")
    _same_bits(same["angle"], ang, "an unmoved image returns the angle")
    assert np.all(same["dist2"] == 0.0)


# ---- 4. the covariance, and into the ingest ---------------------------------------------------------------------------
def test_out_cov_has_patch_covariances_bits_and_goes_into_fill_keypoints_and_a_solve_runs():
    torch = _torch()
    fx = main_fixture()
    p1, p2 = [_t(a) for a in fx["p1"]], [_t(a) for a in fx["p2"]]
    pts, offs = _t(fx["pts"]), _t(fx["offsets"])
    tr = patch_track(p1, p2, pts, offs)
    pc = patch_covariance(p1[0], pts, offs, angle=tr.angle)
    ok = (tr.status == OK).cpu().numpy()
    assert ok.sum() >= 30 and bool((pc.status == patches.PATCH_OK).all())
    _same_bits(tr.cov.cpu().numpy()[ok], pc.cov.cpu().numpy()[ok], "out_cov against patch_covariance(angle=out_angle)")
    assert np.all(np.isnan(tr.cov.cpu().numpy()[~ok]))
    # images -> tracks -> covariances -> fill_keypoints -> solve, nothing leaves the device
    keep = torch.nonzero(tr.status == OK).flatten()
    n = int(keep.numel())
    K = np.array([[110.0, 0.0, (W0 - 1) / 2.0], [0.0, 110.0, (H0 - 1) / 2.0], [0.0, 0.0, 1.0]])
    Kinv = np.linalg.inv(K)
    on_dev = Batch.uniform(capi.MODE_TARGET, 1, n)
    on_dev.fill_keypoints(pts[keep].contiguous(), tr.pts[keep].contiguous(), tr.cov[keep].contiguous(), K_inv=Kinv)
    torch.cuda.synchronize()
    on_host = Batch.uniform(capi.MODE_TARGET, 1, n)
    on_host.fill_keypoints(pts[keep].cpu().numpy(), tr.pts[keep].cpu().numpy(), tr.cov[keep].cpu().numpy(), K_inv=Kinv)
    _same_bits(on_dev.export_payload(), on_host.export_payload(), "payload from the device tensors against the host's numbers")
    q0 = torch.tensor([[0.0, 0.0, 0.0, 1.0]], dtype=torch.float64, device="cuda")
    t0 = torch.tensor([[1.0, 0.1, 0.1]], dtype=torch.float64, device="cuda")
    res = on_dev.solve(q0, t0)
    torch.cuda.synchronize()
    R, tt = res.rotation_matrices().cpu().numpy()[0], res.t.cpu().numpy()[0]
    assert np.all(np.isfinite(R)) and np.all(np.isfinite(tt)) and abs(np.linalg.norm(tt) - 1.0) < 1e-9
    assert np.isfinite(float(res.cost[0]))
    on_dev.close()
    on_host.close()


# ---- 5. the pyramid ---------------------------------------------------------------------------------------------------
def test_pyramid_equals_numpy_in_three_types_odd_sizes_pitched_strided_and_chained():
    torch = _torch()
    rng = np.random.default_rng(31)
    for dt, top in ((np.uint8, 255), (np.uint16, 65535), (np.float32, 1000.0)):
        for h, w in ((H0, W0), (97, 129)):
            img = (rng.random((3, h, w)) * top).astype(dt)
            want = pyramid_levels_np(img, 3)                         # chained twice
            dev = image_pyramid(_t(img), 3)
            host = image_pyramid(img, 3)
            assert len(dev) == len(host) == 3 and dev[1].is_cuda and isinstance(host[1], np.ndarray)
            for l in range(3):
                assert tuple(dev[l].shape) == (3, h >> l, w >> l)
                _same_bits(dev[l].cpu().numpy(), want[l], f"{dt.__name__} {h}x{w} level {l}, device")
                _same_bits(host[l], want[l], f"{dt.__name__} {h}x{w} level {l}, host")
        # pitch > width: a view of a wider buffer whose padding holds what no output may contain; the buffer ends with
        # the image's last pixel
        h, w, pitch = 97, 129, 140
        img = (rng.random((2, h, w)) * top * 0.5).astype(dt)
        buf = np.full((2 * h, pitch), top, dtype=dt)
        buf[:, :w] = img.reshape(2 * h, w)
        flat = _t(buf.reshape(-1)[: (2 * h - 1) * pitch + w].copy())
        view = flat.as_strided((2, h, w), (h * pitch, pitch, 1))
        _same_bits(image_pyramid(view, 2)[1].cpu().numpy(), pyramid_np(img), f"{dt.__name__} pitched")
        # a strided torch view: a crop of a batch, read in place
        big = _t((rng.random((2, 60, 90)) * top).astype(dt))
        crop = big[:, 5:50, 7:80]
        assert not crop.is_contiguous()
        _same_bits(image_pyramid(crop, 2)[1].cpu().numpy(), pyramid_np(crop.cpu().numpy()), f"{dt.__name__} crop")
    # the C entry point with a pitched OUTPUT: the padding between the rows is not written
    img = (rng.random((1, 20, 30)) * 255).astype(np.uint8)
    out = torch.full((10, 21), 7, dtype=torch.uint8, device="cuda")
    src = _t(img)
    capi.check(capi.lib().pnec_hip_image_pyramid_level(src.data_ptr(), out.data_ptr(), patches.PIXEL_U8, 1, 20, 30, 30, 21,
                                                      capi.MEM_DEVICE, 0, torch.cuda.current_stream().cuda_stream))
    o = out.cpu().numpy()
    assert np.array_equal(o[:, :15], pyramid_np(img)[0]) and np.all(o[:, 15:] == 7)


# ---- 6. stream order --------------------------------------------------------------------------------------------------
def _stream_data(seed):
    fx = main_fixture()
    rng = np.random.default_rng(seed)
    img1 = np.clip(fx["img1"].astype(np.int64) + rng.integers(-6, 7, fx["img1"].shape), 0, 255).astype(np.uint8)
    img2 = np.clip(fx["img2"].astype(np.int64) + rng.integers(-6, 7, fx["img2"].shape), 0, 255).astype(np.uint8)
    return dict(img1=_t(img1), img2=_t(img2), pts=_t(fx["pts"] + rng.uniform(-0.5, 0.5, fx["pts"].shape)))


@pytest.mark.parametrize("which", ["image_pyramid", "patch_track"])
def test_device_space_call_respects_stream_order(which):
    from test_stream_order_gpu import Entry, check
    fx = main_fixture()
    offs = _t(fx["offsets"])
    pattern = _t(np.array(patches.PATTERN52))
    good, decoy = _stream_data(41), _stream_data(42)
    if which == "image_pyramid":
        def call(bufs):
            return image_pyramid(bufs["img1"], LEVELS)[1:], None
        good, decoy = dict(img1=good["img1"]), dict(img1=decoy["img1"])
    else:
        # (the pyramids are built on the default stream beforehand, in buffers the probe rewrites: the tracker alone)
        def call(bufs):
            p1 = [bufs["a0"], bufs["a1"], bufs["a2"]]
            p2 = [bufs["b0"], bufs["b1"], bufs["b2"]]
            r = patch_track(p1, p2, bufs["pts"], offs, pattern=pattern)
            return [r.pts, r.angle, r.cov, r.dist2, r.status, r.lost_level], None

        def levels(d):
            p1, p2 = image_pyramid(d["img1"], LEVELS), image_pyramid(d["img2"], LEVELS)
            out = {f"a{l}": p1[l].clone() for l in range(LEVELS)}
            out.update({f"b{l}": p2[l].clone() for l in range(LEVELS)})
            out["pts"] = d["pts"]
            return out
        good, decoy = levels(good), levels(decoy)
        _torch().cuda.synchronize()
    check(Entry(good, decoy, call), which)


# ---- 7. the facade ----------------------------------------------------------------------------------------------------
def test_pypnec_pyramid_and_track_equal_the_python_layer_on_one_image():
    import pnec_amd.pypnec as pypnec
    fx = main_fixture()
    img1, img2 = np.array(fx["img1"][0]), np.array(fx["img2"][0])
    pts = np.array(fx["pts"][:22])
    levels = pypnec.image_pyramid(img1, LEVELS)
    assert len(levels) == LEVELS
    for l in range(LEVELS):
        _same_bits(levels[l], fx["p1"][l][0], f"pypnec.image_pyramid level {l}")
    got = pypnec.patch_track(img1, img2, pts, levels=LEVELS)
    ref = _np(patch_track([a[:1] for a in fx["p1"]], [a[:1] for a in fx["p2"]], pts))
    for key, a in zip(KEYS, got):
        _same_bits(np.asarray(a), ref[key], f"pypnec.patch_track {key}")
