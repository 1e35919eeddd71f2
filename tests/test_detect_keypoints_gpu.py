"""pnec_hip_detect_keypoints on the device against `detect_np` (tests/test_detect_keypoints_cpu.py), the plain-numpy
statement of the definition in include/pnec_hip.h.  Every output array must EQUAL numpy's -- out_cell with its -1s, the
offsets, the points, the scores, the cell indices; there is no tolerance and nothing is left out -- and every entry at and
beyond out_offsets[-1] must keep the sentinel written before the call.  The fixtures are three images of 96 x 128,
97 x 131 (x_start, y_start != 0, an odd remainder) or 64 x 128 (the largest cell) with a constant image in the middle.
"""
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_detect_keypoints_cpu import (CASES, assert_equal_to_np, batch, case_args, current_points, detect_np,  # noqa: E402
                                       reference)

from pnec_amd import Batch, Keypoints, capi, detect_keypoints, image_pyramid, patch_track, patches  # noqa: E402

pytestmark = pytest.mark.gpu

KEYS = ("cell", "offsets", "pts", "score", "cell_index")
F_SENT, I_SENT = -7.25, -77


def _torch():
    import torch
    return torch


def _t(a):
    return _torch().from_numpy(np.array(a)).cuda()        # (a copy: the fixtures are read-only)


def _dev_current(cur):
    return None if cur is None else (_t(cur[0]), _t(cur[1]))


def _sentinel_out(F, h, w, G, K, device=True):
    """a capacity-form result whose arrays hold values the detector never writes"""
    n_cells = (w // G) * (h // G)
    cap = F * n_cells * K
    if device:
        torch = _torch()
        full = lambda shape, v, dt: torch.full(shape, v, dtype=dt, device="cuda")
        return Keypoints(full((F + 1,), I_SENT, torch.int64), full((cap, 2), F_SENT, torch.float64),
                         full((cap,), I_SENT, torch.int32), full((cap,), I_SENT, torch.int32),
                         full((F, n_cells), I_SENT, torch.int32))
    return Keypoints(np.full(F + 1, I_SENT, dtype=np.int64), np.full((cap, 2), F_SENT), np.full(cap, I_SENT, dtype=np.int32),
                     np.full(cap, I_SENT, dtype=np.int32), np.full((F, n_cells), I_SENT, dtype=np.int32))


def _np(r):
    return {k: (getattr(r, k).cpu().numpy() if hasattr(getattr(r, k), "cpu") else np.asarray(getattr(r, k))) for k in KEYS}


def detect_checked(images, what, ref=None, **kw):
    """runs the capacity form into sentinel-filled arrays, checks the sentinels beyond the last point, returns the
    trimmed outputs as numpy (compared with `ref` when given)"""
    on_device = hasattr(images, "is_cuda")
    shape = tuple(images.shape)
    F, h, w = (1,) + shape if len(shape) == 2 else shape
    out = _sentinel_out(F, h, w, kw["grid"], kw["points_per_cell"], on_device)
    r = detect_keypoints(images, capacity=True, out=out, **kw)
    if on_device:
        _torch().cuda.synchronize()
    got = _np(r)
    n = int(got["offsets"][-1])
    assert np.all(got["pts"][n:] == F_SENT) and np.all(got["score"][n:] == I_SENT) and np.all(got["cell_index"][n:] == I_SENT), \
        f"{what}: entries beyond the last point were written"
    got = dict(got, pts=got["pts"][:n], score=got["score"][:n], cell_index=got["cell_index"][:n])
    if ref is not None:
        assert_equal_to_np(got, ref, what)
    return got


# ---- 1. every case, device space --------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_every_output_equals_numpy(case):
    kw = case_args(case)
    kw["current"] = _dev_current(kw["current"])
    got = detect_checked(_t(batch(case[1])), case[0], reference(case[0]), **kw)
    assert got["offsets"][1] == got["offsets"][2], "the constant image has an empty range"
    # the trimmed form (the one read-back) gives the same rows
    r = detect_keypoints(_t(batch(case[1])), **kw)
    assert r.pts.is_cuda and tuple(r.pts.shape) == (len(got["pts"]), 2)
    assert_equal_to_np(_np(r), reference(case[0]), case[0] + ", trimmed")


# ---- 2. pixel types, pitch, views -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["b G16 K4 E19 cur", "b G30 K1 E19 cur", "c G64 K4 E3"])
def test_uint16_low_bits_pitch_and_a_cropped_view(name):
    case = next(c for c in CASES if c[0] == name)
    kw = case_args(case)
    kw["current"] = _dev_current(kw["current"])
    img = np.array(batch(case[1]))
    F, h, w = img.shape
    rng = np.random.default_rng(17)
    wide = (img.astype(np.uint16) << 8) | rng.integers(0, 256, img.shape).astype(np.uint16)
    for what, im, top in (("uint8", img, 255), ("uint16 with low bits", wide, 65535)):
        detect_checked(_t(im), f"{name}, {what}", reference(name), **kw)
        # pitch > width: a view of a wider buffer whose padding holds the largest value; the buffer ends with the last pixel
        pitch = w + 5
        buf = np.full((F * h, pitch), top, dtype=im.dtype)
        buf[:, :w] = im.reshape(F * h, w)
        flat = _t(buf.reshape(-1)[: (F * h - 1) * pitch + w].copy())
        view = flat.as_strided((F, h, w), (h * pitch, pitch, 1))
        detect_checked(view, f"{name}, {what}, pitched", reference(name), **kw)
    # a cropped torch view of a larger batch, read in place (columns cropped; the rows of an image stay evenly pitched)
    big = np.full((F, h, w + 13), 255, dtype=np.uint8)
    big[:, :, 6:6 + w] = img
    crop = _t(big)[:, :, 6:6 + w]
    assert not crop.is_contiguous()
    detect_checked(crop, f"{name}, crop", reference(name), **kw)


# ---- 3. alone = in the batch, HOST = DEVICE, NULL outputs -------------------------------------------------------------
def test_alone_equals_in_the_batch_and_host_space_equals_device_space():
    name = "b G16 K4 E19 cur"
    case = next(c for c in CASES if c[0] == name)
    kw = case_args(case)
    ref = reference(name)
    img = np.array(batch("b"))
    host = detect_checked(img, name + ", HOST space", ref, **kw)
    assert isinstance(detect_keypoints(img, **kw).pts, np.ndarray)
    offsets, pts = kw["current"]
    for f in range(3):
        cur = (np.array([0, offsets[f + 1] - offsets[f]], dtype=np.int64), pts[offsets[f]:offsets[f + 1]])
        one = detect_checked(_t(img[f]), f"{name}, image {f} alone", **dict(kw, current=_dev_current(cur)))
        lo, hi = int(ref["offsets"][f]), int(ref["offsets"][f + 1])
        assert np.array_equal(one["cell"][0], ref["cell"][f]) and np.array_equal(one["pts"], ref["pts"][lo:hi])
        assert np.array_equal(one["score"], ref["score"][lo:hi]) and np.array_equal(one["cell_index"], ref["cell_index"][lo:hi])
        assert np.array_equal(one["pts"], host["pts"][lo:hi])
    # one image, current points given as a plain array
    one = detect_keypoints(_t(img[0]), **dict(kw, current=_t(pts[:offsets[1]])))
    assert np.array_equal(one.pts.cpu().numpy(), ref["pts"][:ref["offsets"][1]])


def test_null_score_and_cell_index_leave_the_other_outputs_unchanged():
    torch = _torch()
    name = "a G16 K4 E19 cur"
    case = next(c for c in CASES if c[0] == name)
    kw = case_args(case)
    ref = reference(name)
    img = _t(batch("a"))
    co, cp = _dev_current(kw["current"])
    stream = torch.cuda.current_stream().cuda_stream
    for space in ("device", "host"):
        out = _sentinel_out(3, 96, 128, 16, 4, space == "device")
        if space == "device":
            p = lambda a: a.data_ptr()
            args = (p(img), patches.PIXEL_U8, 3, 96, 128, 128, 16, 4, 5, 19, p(co), int(cp.shape[0]), p(cp))
            where = (capi.MEM_DEVICE, 0, stream)
        else:
            p = lambda a: a.ctypes.data
            hi, ho, hp = np.array(batch("a")), kw["current"][0], kw["current"][1]
            args = (p(hi), patches.PIXEL_U8, 3, 96, 128, 128, 16, 4, 5, 19, p(ho), len(hp), p(hp))
            where = (capi.MEM_HOST, 0, None)
        capi.check(capi.lib().pnec_hip_detect_keypoints(*args, p(out.cell), p(out.offsets), p(out.pts), None, None, *where))
        torch.cuda.synchronize()
        got = _np(out)
        n = int(got["offsets"][-1])
        assert np.array_equal(got["cell"], ref["cell"]) and np.array_equal(got["offsets"], ref["offsets"]), space
        assert np.array_equal(got["pts"][:n], ref["pts"]) and np.all(got["pts"][n:] == F_SENT), space
        assert np.all(got["score"] == I_SENT) and np.all(got["cell_index"] == I_SENT), space


# ---- 4. stream order --------------------------------------------------------------------------------------------------
# The probe of tests/test_stream_order_gpu.py (see its docstring): the call runs on a non-blocking side stream behind a
# 50 ms device-side delay, its inputs arrive on that stream only after the delay and hold a decoy before and after; the
# outputs must have the default-stream call's bits and the call must return while the delay is still running.
DELAY_MS = 50.0
_cycles_per_ms = None
_mm = None


def _spin(n):
    torch = _torch()
    if hasattr(torch.cuda, "_sleep"):
        torch.cuda._sleep(int(n))
    else:
        for _ in range(int(n)):
            torch.mm(_mm, _mm)


def _delay(ms):
    """`ms` of device time on the current stream: torch.cuda._sleep calibrated once per module with two events (a chain
    of matrix products timed the same way where that helper is missing)."""
    torch = _torch()
    global _cycles_per_ms, _mm
    if _cycles_per_ms is None:
        if not hasattr(torch.cuda, "_sleep"):
            _mm = torch.ones((1024, 1024), device="cuda")
        unit = 2_000_000 if hasattr(torch.cuda, "_sleep") else 20
        _spin(unit)                                  # (first use)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        _spin(unit)
        b.record()
        torch.cuda.synchronize()
        _cycles_per_ms = unit / max(a.elapsed_time(b), 1e-3)
    if ms > 0:
        _spin(max(1, _cycles_per_ms * ms))


def _same(a, b):
    torch = _torch()
    bits = lambda t: t.contiguous().view(torch.int64) if t.dtype == torch.float64 else t.contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(bits(a), bits(b)))


def test_device_space_call_respects_stream_order():
    torch = _torch()
    kw = dict(grid=16, points_per_cell=4, min_threshold=5, edge=3)
    good = dict(img=_t(batch("a")), cur=_t(current_points("a", 16)[1]))
    rng = np.random.default_rng(8)
    decoy = dict(img=_t(rng.integers(0, 256, batch("a").shape).astype(np.uint8)),         # the decoy image: noise
                 cur=_t(current_points("a", 16)[1][::-1].copy()))
    co = _t(current_points("a", 16)[0])
    out = _sentinel_out(3, 96, 128, 16, 4)
    sentinels = [out.offsets, out.pts, out.score, out.cell_index, out.cell]

    def prepare():
        for s in sentinels:
            s.fill_(F_SENT if s.dtype.is_floating_point else I_SENT)
        torch.cuda.synchronize()

    def call(bufs):
        r = detect_keypoints(bufs["img"], current=(co, bufs["cur"]), capacity=True, out=out, **kw)
        return [r.offsets, r.pts, r.score, r.cell_index, r.cell]

    def on_default_stream(bufs, data):
        prepare()
        for k, v in data.items():
            bufs[k].copy_(v)
        outs = [o.clone() for o in call(bufs)]
        torch.cuda.synchronize()
        return outs

    _delay(0)                                        # (calibrates on first use, outside every timed window)
    bufs = {k: v.clone() for k, v in decoy.items()}
    want = on_default_stream(bufs, good)
    want_decoy = on_default_stream(bufs, decoy)
    assert any(not _same(a, b) for a, b in zip(want, want_decoy)), "the decoy gives the same bits: this probe proves nothing"
    assert_equal_to_np({k: v.cpu().numpy()[: int(want[0][-1])] if k in ("pts", "score", "cell_index") else v.cpu().numpy()
                        for k, v in zip(("offsets", "pts", "score", "cell_index", "cell"), want)},
                       detect_np(batch("a"), current=current_points("a", 16), **kw), "stream-order reference")
    S = torch.cuda.Stream()

    def enqueue(ms):
        prepare()
        for k, v in decoy.items():
            bufs[k].copy_(v)
        torch.cuda.synchronize()
        with torch.cuda.stream(S):
            if ms:
                _delay(ms)
            gate = torch.cuda.Event()
            gate.record()
            for k, v in good.items():
                bufs[k].copy_(v)
            t0 = time.perf_counter()
            outs = call(bufs)
            host_ms = (time.perf_counter() - t0) * 1e3
            returned_early = not gate.query()
            got = [o.clone() for o in outs]
            for k, v in decoy.items():
                bufs[k].copy_(v)
        S.synchronize()                              # S alone
        return got, outs, host_ms, returned_early

    enqueue(0)                                       # warm-up
    torch.cuda.synchronize()
    got, outs, host_ms, returned_early = enqueue(DELAY_MS)
    mismatch = [i for i, (a, b) in enumerate(zip(got, want)) if not _same(a, b)]
    torch.cuda.synchronize()
    late = [i for i, (a, b) in enumerate(zip(outs, want)) if not _same(a, b)]
    print(f"stream-order probe detect_keypoints: host side of the call {host_ms:.3f} ms, returned_early={returned_early}, "
          f"mismatching outputs {mismatch}, after a device-wide wait {late}")
    assert not mismatch, f"outputs {mismatch} differ from the default-stream call's bits"
    assert not late, f"outputs {late} were written again after the stream had drained"
    assert returned_early, f"documented as asynchronous, but the call returned only after the delay ({host_ms:.1f} ms)"


# ---- 5. the chain -----------------------------------------------------------------------------------------------------
def test_detect_pyramid_track_fill_keypoints_solve_without_leaving_the_device():
    torch = _torch()
    from test_patch_track_cpu import H0, LEVELS, OK, W0, main_fixture, patch_track_np
    fx = main_fixture()
    # (checked on the CPU with detect_np + patch_track_np: 54 points on the three images, all of them tracked)
    ref_kp = detect_np(fx["img1"], 16, 1, 5, 19)
    ref_tr = patch_track_np(fx["p1"], fx["p2"], ref_kp["pts"], ref_kp["offsets"])
    assert len(ref_kp["pts"]) >= 30 and 2 * int((ref_tr["status"] == OK).sum()) >= len(ref_kp["pts"])
    kp = detect_keypoints(_t(fx["img1"]), grid=16, points_per_cell=1, min_threshold=5, edge=19)
    assert kp.pts.is_cuda and kp.offsets.is_cuda
    assert_equal_to_np(_np(kp), ref_kp, "chain: detection")
    p1, p2 = image_pyramid(_t(fx["img1"]), LEVELS), image_pyramid(_t(fx["img2"]), LEVELS)
    tr = patch_track(p1, p2, kp.pts, kp.offsets)
    status = tr.status.cpu().numpy()
    assert np.array_equal(status, ref_tr["status"]), (status, ref_tr["status"])
    assert 2 * int((status == OK).sum()) >= len(status)
    first = tr.status[: int(kp.offsets[1])] == OK                      # the first image pair
    keep = torch.nonzero(first).flatten()
    n = int(keep.numel())
    assert n >= 5
    K = np.array([[110.0, 0.0, (W0 - 1) / 2.0], [0.0, 110.0, (H0 - 1) / 2.0], [0.0, 0.0, 1.0]])
    b = Batch.uniform(capi.MODE_TARGET, 1, n)
    b.fill_keypoints(kp.pts[keep].contiguous(), tr.pts[keep].contiguous(), tr.cov[keep].contiguous(), K_inv=np.linalg.inv(K))
    q0 = torch.tensor([[0.0, 0.0, 0.0, 1.0]], dtype=torch.float64, device="cuda")
    t0 = torch.tensor([[1.0, 0.1, 0.1]], dtype=torch.float64, device="cuda")
    res = b.solve(q0, t0)
    torch.cuda.synchronize()
    R, tt = res.rotation_matrices().cpu().numpy()[0], res.t.cpu().numpy()[0]
    assert np.all(np.isfinite(R)) and np.all(np.isfinite(tt)) and abs(np.linalg.norm(tt) - 1.0) < 1e-9
    assert np.isfinite(float(res.cost[0]))
    b.close()


# ---- 6. the facade ----------------------------------------------------------------------------------------------------
def test_pypnec_detect_keypoints_equals_the_python_layer_on_one_image():
    import pnec_amd.pypnec as pypnec
    img = np.array(batch("b")[0])
    offsets, pts = current_points("b", 16)
    cur = pts[:offsets[1]]
    for kw in (dict(grid=16, points_per_cell=4, min_threshold=5, edge=19, current=cur), dict(grid=30)):
        got = pypnec.detect_keypoints(img, **kw)
        want = detect_keypoints(_t(img), **{k: (_t(v) if k == "current" else v) for k, v in kw.items()})
        for key, a in zip(("pts", "score", "cell_index", "cell"), got):
            b = getattr(want, key).cpu().numpy()
            b = b[0] if key == "cell" else b
            assert np.asarray(a).dtype == b.dtype and np.array_equal(np.asarray(a), b), (kw, key)
        assert len(got[0]) > 0
