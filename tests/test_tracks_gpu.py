"""pnec_hip_tracks_retain, pnec_hip_tracks_append, pnec_hip_patch_track_indexed and pnec_amd.Tracker on the device
against the plain-numpy statements of their definitions (tests/test_tracks_cpu.py: retain_np, append_np, tracker_step_np).
The bookkeeping is exact: every output array must EQUAL numpy's, padding included, to the last row.  The indexed tracker
must have the bits of the plain one.  The tracker's floating-point outputs are held to check_track_against_np's bounds
(tests/test_patch_track_cpu.py) at every step, each step checked from the device's own input set, so that rounding does
not compound over the frames."""
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_patch_track_cpu import H0, LEVELS, OK, W0, check_track_against_np, main_fixture  # noqa: E402
from test_tracks_cpu import (RETAIN_KEYS, SEQ_CAPACITY, SEQ_EDGE, SEQ_F, SEQ_FRAMES, SEQ_GRID, SEQ_RING, SET_KEYS,  # noqa: E402
                             append_cases, append_reference, assert_same, retain_cases, retain_reference,
                             sequence_fixture, tracker_step_np)

from pnec_amd import (Batch, Keypoints, PatchTrack, Tracker, TrackSet, append_tracks, capi, patch_track,  # noqa: E402
                      retain_tracks)

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    return torch


def _t(a):
    return None if a is None else _torch().from_numpy(np.array(a)).cuda()        # (a copy: the fixtures are read-only)


def _n(a):
    return None if a is None else (a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a))


def _set(s, conv):
    return None if s is None else TrackSet(*[conv(s[k]) for k in SET_KEYS])


def _set_np(ts, keys=SET_KEYS):
    return {k: _n(getattr(ts, k)) for k in keys}


def _same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"{what}: bits differ in {int((a != b).sum())} entries"


def run_retain(kw, conv):
    trk = kw["trk"]
    r = PatchTrack(conv(trk["pts"]), conv(trk["angle"]), conv(trk["cov"]) if kw["with_cov"] else None, None, conv(trk["status"]),
                   None)
    out = retain_tracks(_set(kw["s"], conv), r, kw["max_age"])
    got = _set_np(out, RETAIN_KEYS)
    if not kw["with_prev_pts"]:
        got["prev_pts"] = None          # (the Python layer always asks for them; the ABI's NULL is the stream test's)
    if not kw["with_src"]:
        got["src"] = None
    return out, got


def run_append(kw, conv):
    det = kw["det"]
    kp = Keypoints(conv(det["offsets"]), conv(det["pts"]), None, None, None)
    nid = conv(kw["next_id"].copy())
    out, dropped = append_tracks(_set(kw["s"], conv), kp, conv(det["cov"]), kw["base"], kw["capacity"], nid, rows=kw["n_out"])
    got = _set_np(out)
    if not kw["with_cov"]:
        assert got["cov"] is None
    return out, got, _n(nid), _n(dropped)


# ---- 1. the bookkeeping against numpy, DEVICE and HOST space ----------------------------------------------------------
@pytest.mark.parametrize("name", [n for n, _ in retain_cases()])
def test_retain_equals_numpy_to_the_last_row(name):
    kw = dict(retain_cases())[name]
    ref = retain_reference(kw)
    if not kw["with_prev_pts"]:
        ref = dict(ref, prev_pts=None)
    out, dev = run_retain(kw, _t)
    assert out.id.is_cuda and out.offsets.is_cuda
    assert_same(dev, ref, RETAIN_KEYS, f"device, retain, {name}")
    out, host = run_retain(kw, lambda a: None if a is None else np.array(a))
    assert isinstance(out.id, np.ndarray)
    assert_same(host, ref, RETAIN_KEYS, f"host space, retain, {name}")


def test_retain_with_null_optional_arrays_through_the_abi():
    """out_prev_pts and out_src NULL, the covariance group NULL: the other outputs are unchanged"""
    torch = _torch()
    kw = dict(retain_cases())["optional arrays NULL"]
    ref = retain_reference(kw)
    s, trk = _set(kw["s"], _t), {k: _t(v) for k, v in kw["trk"].items()}
    N, F = len(kw["s"]["id"]), len(kw["s"]["offsets"]) - 1
    o = dict(offsets=torch.empty(F + 1, dtype=torch.int64, device="cuda"), id=torch.empty(N, dtype=torch.int64, device="cuda"),
             tmpl_image=torch.empty(N, dtype=torch.int32, device="cuda"), tmpl_pts=torch.empty((N, 2), dtype=torch.float64, device="cuda"),
             age=torch.empty(N, dtype=torch.int32, device="cuda"), pts=torch.empty((N, 2), dtype=torch.float64, device="cuda"),
             angle=torch.empty(N, dtype=torch.float64, device="cuda"))
    p = lambda a: a.data_ptr()
    capi.check(capi.lib().pnec_hip_tracks_retain(
        F, p(s.offsets), N, p(s.id), p(s.tmpl_image), p(s.tmpl_pts), p(s.age), p(s.pts), None, p(trk["pts"]), p(trk["angle"]),
        None, p(trk["status"]), 0, p(o["offsets"]), p(o["id"]), p(o["tmpl_image"]), p(o["tmpl_pts"]), p(o["age"]), p(o["pts"]),
        p(o["angle"]), None, None, None, None, capi.MEM_DEVICE, 0, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    got = {k: _n(v) for k, v in o.items()}
    got.update(cov=None, prev_pts=None, prev_cov=None, src=None)
    assert_same(got, ref, RETAIN_KEYS, "device, retain through the ABI with NULL optional arrays")


@pytest.mark.parametrize("name", [n for n, _ in append_cases()])
def test_append_equals_numpy_to_the_last_row(name):
    kw = dict(append_cases())[name]
    ref, ref_id, ref_dropped = append_reference(kw)
    out, dev, nid, dropped = run_append(kw, _t)
    assert out.id.is_cuda
    assert_same(dev, ref, SET_KEYS, f"device, append, {name}")
    assert np.array_equal(nid, ref_id) and np.array_equal(dropped, ref_dropped) and dropped.dtype == np.int64, name
    out, host, nid, dropped = run_append(kw, lambda a: None if a is None else np.array(a))
    assert isinstance(out.id, np.ndarray)
    assert_same(host, ref, SET_KEYS, f"host space, append, {name}")
    assert np.array_equal(nid, ref_id) and np.array_equal(dropped, ref_dropped), name


def test_an_image_alone_equals_the_same_image_inside_the_batch():
    kw = dict(retain_cases())["random statuses"]
    _, batch = run_retain(kw, _t)
    off, boff = kw["s"]["offsets"], batch["offsets"]
    for f in range(len(off) - 1):
        lo, hi = int(off[f]), int(off[f + 1])
        one = dict(kw, s={k: (np.array([0, hi - lo]) if k == "offsets" else v[lo:hi]) for k, v in kw["s"].items()},
                   trk={k: v[lo:hi] for k, v in kw["trk"].items()})
        _, alone = run_retain(one, _t)
        m = int(alone["offsets"][1])
        assert m == boff[f + 1] - boff[f]
        for k in RETAIN_KEYS[1:]:
            want = batch[k][boff[f]:boff[f + 1]]
            want = want - lo if k == "src" else want
            _same_bits(alone[k][:m], want, f"retain, image {f} alone, {k}")
    kw = dict(append_cases())["capacity 66"]
    _, batch, nid, dropped = run_append(kw, _t)
    boff = batch["offsets"]
    for f in range(len(boff) - 1):
        lo, hi = (int(x) for x in kw["s"]["offsets"][f:f + 2])
        dlo, dhi = (int(x) for x in kw["det"]["offsets"][f:f + 2])
        one = dict(kw, s={k: (np.array([0, hi - lo]) if k == "offsets" else v[lo:hi]) for k, v in kw["s"].items()},
                   det=dict(offsets=np.array([0, dhi - dlo]), pts=kw["det"]["pts"][dlo:dhi], cov=kw["det"]["cov"][dlo:dhi]),
                   base=kw["base"] + f, next_id=kw["next_id"][f:f + 1], n_out=kw["capacity"])
        _, alone, nid1, dropped1 = run_append(one, _t)
        m = int(alone["offsets"][1])
        assert m == boff[f + 1] - boff[f] and nid1[0] == nid[f] and dropped1[0] == dropped[f]
        for k in SET_KEYS[1:]:
            _same_bits(alone[k][:m], batch[k][boff[f]:boff[f + 1]], f"append, image {f} alone, {k}")


# ---- 2. the indexed tracker has the plain one's bits ------------------------------------------------------------------
TRACK_KEYS = ("pts", "angle", "cov", "dist2", "status", "lost_level")


def _track_np(r):
    return {k: _n(getattr(r, k)) for k in TRACK_KEYS}


def test_patch_track_indexed_has_the_bits_of_the_plain_call_keypoint_by_keypoint():
    fx = main_fixture()
    F = 3
    p1, p2 = fx["p1"], fx["p2"]
    alt = [a.copy() for a in p1]                          # the other half of the stack: some levels altered
    alt[0][0] = 255 - alt[0][0]
    alt[1][2] = 77                                        # (a constant level: BAD_TEMPLATE there)
    alt[2][0] = np.roll(alt[2][0], 3, axis=1)
    stack = [np.concatenate([a, b]) for a, b in zip(p1, alt)]
    pts, offs = fx["pts"], fx["offsets"]
    dp1, dp2, dalt, dstack = ([_t(a) for a in p] for p in (p1, p2, alt, stack))
    plain = _track_np(patch_track(dp1, dp2, _t(pts), _t(offs)))
    plain_alt = _track_np(patch_track(dalt, dp2, _t(pts), _t(offs), prev=dp1))
    assert any(not np.array_equal(plain[k], plain_alt[k], equal_nan=True) for k in TRACK_KEYS), "the altered half changes nothing"
    # tmpl_image = NULL: the plain call's bits, through the indexed entry point
    import ctypes as C
    torch = _torch()
    M = len(pts)
    out = dict(pts=torch.empty((M, 2), dtype=torch.float64, device="cuda"), angle=torch.empty(M, dtype=torch.float64, device="cuda"),
               cov=torch.empty((M, 3), dtype=torch.float64, device="cuda"), dist2=torch.empty(M, dtype=torch.float64, device="cuda"),
               status=torch.empty(M, dtype=torch.int32, device="cuda"), lost_level=torch.empty(M, dtype=torch.int32, device="cuda"))
    table = lambda pyr: ((C.c_void_p * LEVELS)(*[a.data_ptr() for a in pyr]), (C.c_int64 * LEVELS)(*[int(a.stride()[1]) for a in pyr]))
    # (the fixture's levels are views: a raw call wants evenly pitched images, which the Python layer makes of them)
    cp1, cp2 = [a.contiguous() for a in dp1], [a.contiguous() for a in dp2]
    (tp, tq), (np_, nq) = table(cp1), table(cp2)
    d_pts, d_offs, pat = _t(pts), _t(offs), _t(np.array(__import__("pnec_amd").PATTERN52))
    capi.check(capi.lib().pnec_hip_patch_track_indexed(
        tp, tq, F, None, None, np_, nq, LEVELS, 0, F, H0, W0, d_offs.data_ptr(), M, d_pts.data_ptr(), None, None, None, 0.0, 0.0,
        pat.data_ptr(), 52, 40, 0.04, 0, 10.0, *[out[k].data_ptr() for k in TRACK_KEYS], capi.MEM_DEVICE, 0,
        torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    for k in TRACK_KEYS:
        _same_bits(_n(out[k]), plain[k], f"{k}: indexed entry point without tmpl_image against pnec_hip_patch_track")
    # a stack of 2F images and a per-keypoint choice of half
    rng = np.random.default_rng(5)
    half = rng.integers(0, 2, M)
    image = np.searchsorted(offs, np.arange(M), side="right") - 1
    ti = (half * F + image).astype(np.int32)
    assert set(half[image == 0]) == {0, 1} and set(half[image == 2]) == {0, 1}
    want = {k: np.where((half == 0).reshape((M,) + (1,) * (plain[k].ndim - 1)), plain[k], plain_alt[k]) for k in TRACK_KEYS}
    got = _track_np(patch_track(dstack, dp2, _t(pts), _t(offs), prev=dp1, tmpl_image=_t(ti)))
    for k in TRACK_KEYS:
        _same_bits(got[k], want[k], f"{k}: indexed on a stack of 2F images against the plain calls")
    host = _track_np(patch_track(stack, p2, pts, offs, prev=p1, tmpl_image=ti))
    for k in TRACK_KEYS:
        _same_bits(host[k], want[k], f"{k}: indexed, HOST space")
    # out of range: clamped in DEVICE space, refused in HOST space
    wild = ti.copy()
    wild[half == 1] = 1000 + image[half == 1]             # -> 2F - 1
    wild[(half == 0) & (image == 0)] = -3                 # -> 0
    clamped = np.clip(wild, 0, 2 * F - 1).astype(np.int32)
    a = _track_np(patch_track(dstack, dp2, _t(pts), _t(offs), prev=dp1, tmpl_image=_t(wild)))
    b = _track_np(patch_track(dstack, dp2, _t(pts), _t(offs), prev=dp1, tmpl_image=_t(clamped)))
    for k in TRACK_KEYS:
        _same_bits(a[k], b[k], f"{k}: an index out of range is clamped")
    with pytest.raises(capi.PnecHipError) as ei:
        patch_track(stack, p2, pts, offs, prev=p1, tmpl_image=wild)
    assert ei.value.code == capi.ERR_INVALID_ARGUMENT and "tmpl_image" in str(ei.value)


# ---- 3. stream order --------------------------------------------------------------------------------------------------
# The probe of tests/test_stream_order_gpu.py (see its docstring), copied: the call runs on a non-blocking side stream
# behind a 50 ms device-side delay, its inputs arrive on that stream only after the delay and hold a decoy before and
# after; the outputs must have the default-stream call's bits and the call must return while the delay is still running.
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


def _probe(what, good, decoy, call):
    """good / decoy: dicts of device tensors of equal shapes; call(bufs) -> list of output tensors (the same objects on
    every call, written in place)"""
    torch = _torch()

    def on_default_stream(bufs, data):
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
    S = torch.cuda.Stream()

    def enqueue(ms):
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
    print(f"stream-order probe {what}: host side of the call {host_ms:.3f} ms, returned_early={returned_early}, "
          f"mismatching outputs {mismatch}")
    assert not mismatch, f"outputs {mismatch} differ from the default-stream call's bits"
    assert returned_early, f"documented as asynchronous, but the call returned only after the delay ({host_ms:.1f} ms)"


@pytest.mark.parametrize("which", ["retain", "append", "indexed"])
def test_device_space_calls_respect_stream_order(which):
    torch = _torch()
    rng = np.random.default_rng(21)
    if which == "retain":
        kw, other = dict(retain_cases())["random statuses"], dict(retain_cases())["max_age 1"]
        pack = lambda c: {**{"s_" + k: _t(v) for k, v in c["s"].items() if k != "offsets"}, **{"t_" + k: _t(v) for k, v in c["trk"].items()}}
        offs = _t(kw["s"]["offsets"])
        N = len(kw["s"]["id"])
        from pnec_amd.tracker import new_track_set
        out = new_track_set(len(kw["s"]["offsets"]) - 1, N, True, torch.device("cuda", 0), retained=True)

        def call(b):
            s = TrackSet(offs, *[b["s_" + k] for k in SET_KEYS[1:]])
            r = PatchTrack(b["t_pts"], b["t_angle"], b["t_cov"], None, b["t_status"], None)
            o = retain_tracks(s, r, 0, out=out)
            return [getattr(o, k) for k in RETAIN_KEYS]
        _probe("tracks_retain", pack(kw), pack(other), call)
    elif which == "append":
        kw, other = dict(append_cases())["capacity 66"], dict(append_cases())["capacity 60"]
        pack = lambda c: {**{"s_" + k: _t(v) for k, v in c["s"].items() if k != "offsets"},
                          "d_pts": _t(c["det"]["pts"]), "d_cov": _t(c["det"]["cov"]), "next_id": _t(c["next_id"] + (c is other))}
        offs, doffs = _t(kw["s"]["offsets"]), _t(kw["det"]["offsets"])
        from pnec_amd.tracker import new_track_set
        F = len(kw["det"]["offsets"]) - 1
        out = new_track_set(F, kw["n_out"], True, torch.device("cuda", 0))
        dropped, nid = torch.zeros(F, dtype=torch.int64, device="cuda"), torch.zeros(F, dtype=torch.int64, device="cuda")

        def call(b):
            nid.copy_(b["next_id"])
            s = TrackSet(offs, *[b["s_" + k] for k in SET_KEYS[1:]])
            o, d = append_tracks(s, Keypoints(doffs, b["d_pts"], None, None, None), b["d_cov"], kw["base"], kw["capacity"], nid,
                                 rows=kw["n_out"], out=out, dropped=dropped)
            return [getattr(o, k) for k in SET_KEYS] + [d, nid]
        _probe("tracks_append", pack(kw), pack(other), call)
    else:
        fx = main_fixture()
        F, M = 3, len(fx["pts"])
        stack = [_t(np.concatenate([a, a[::-1]])) for a in fx["p1"]]
        prev, nxt = [_t(a) for a in fx["p1"]], [_t(a) for a in fx["p2"]]
        image = np.searchsorted(fx["offsets"], np.arange(M), side="right") - 1
        good = dict(ti=_t(image.astype(np.int32)), pts=_t(fx["pts"]))
        decoy = dict(ti=_t((F + rng.integers(0, F, M)).astype(np.int32)), pts=_t(fx["pts"][::-1].copy()))
        offs, pat = _t(fx["offsets"]), _t(np.array(__import__("pnec_amd").PATTERN52))
        outs = {}

        def call(b):
            r = patch_track(stack, nxt, b["pts"], offs, prev=prev, tmpl_image=b["ti"], pattern=pat)
            for k in TRACK_KEYS:                      # (patch_track allocates: the probe wants the same tensors every time)
                if k not in outs:
                    outs[k] = torch.empty_like(getattr(r, k))
                outs[k].copy_(getattr(r, k))
            return [outs[k] for k in TRACK_KEYS]
        _probe("patch_track_indexed", good, decoy, call)


def _frames():
    return [_t(a) for a in sequence_fixture()["frames"]]


def _tracker():
    return Tracker(SEQ_F, H0, W0, levels=LEVELS, ring=SEQ_RING, grid=SEQ_GRID, capacity=SEQ_CAPACITY, edge=SEQ_EDGE)


def test_tracker_process_returns_while_a_delay_queued_before_it_still_runs():
    torch = _torch()
    frames = _frames()
    ref = _tracker()
    for n in range(3):
        want = ref.process(frames[n])
    want = [getattr(want, k).clone() for k in RETAIN_KEYS] + [getattr(ref.tracks, k).clone() for k in SET_KEYS]
    trk = _tracker()
    trk.process(frames[0])
    trk.process(frames[1])
    torch.cuda.synchronize()
    _delay(0)
    S = torch.cuda.Stream()
    with torch.cuda.stream(S):
        _delay(DELAY_MS)
        gate = torch.cuda.Event()
        gate.record()
        t0 = time.perf_counter()
        r = trk.process(frames[2])
        host_ms = (time.perf_counter() - t0) * 1e3
        returned_early = not gate.query()
    S.synchronize()
    got = [getattr(r, k) for k in RETAIN_KEYS] + [getattr(trk.tracks, k) for k in SET_KEYS]
    print(f"Tracker.process: host side {host_ms:.3f} ms, returned_early={returned_early}")
    assert all(_same(a, b) for a, b in zip(got, want)), "the step on a side stream differs from the default stream's"
    assert returned_early, f"process returned only after the delay ({host_ms:.1f} ms): something waited"


# ---- 4. the tracker over the sequence fixture -------------------------------------------------------------------------
def test_tracker_over_four_frames_each_step_from_the_devices_own_input_set():
    torch = _torch()
    frames = _frames()
    trk = _tracker()
    retained = None
    for n in range(SEQ_FRAMES):
        s_in = None if n == 0 else _set_np(trk.tracks)
        nid_in = _n(trk.next_id).copy()
        retained = trk.process(frames[n])
        torch.cuda.synchronize()
        ref = tracker_step_np(n, s_in, nid_in)
        out = _set_np(trk.tracks)
        if n == 0:
            assert retained is None
        else:
            got = {k: _n(getattr(trk.last_track, k)) for k in TRACK_KEYS}
            check_track_against_np(got, ref["trk"], f"tracker step {n}, all {len(got['status'])} rows, none excluded")
            ok = ref["trk"]["status"] == OK
            assert np.all(np.isnan(got["cov"][~ok])) and np.allclose(got["cov"][ok], ref["trk"]["cov"][ok], rtol=1e-6)
            r = _set_np(retained, RETAIN_KEYS)
            for k in ("offsets", "id", "tmpl_image", "age", "src", "tmpl_pts", "prev_pts", "prev_cov"):
                assert np.array_equal(r[k], ref["retained"][k], equal_nan=True), (n, k)
            m, src = int(r["offsets"][-1]), r["src"]
            # the statuses are equal, so the retained rows are the reference's; their numbers are the tracker's own
            for k, t in (("pts", got["pts"]), ("angle", got["angle"]), ("cov", got["cov"])):
                _same_bits(r[k][:m], t[src[:m]], f"step {n}: retained {k} is the track's output of row src")
                assert np.all(np.isnan(r[k][m:]))
            # the refill's occupancy came from the device's retained positions: the same cells as the reference's
            det = trk._det
            assert np.array_equal(_n(det.cell), ref["det"]["cell"]) and np.array_equal(_n(det.offsets), ref["det"]["offsets"])
        for k in ("offsets", "id", "tmpl_image", "age"):
            assert np.array_equal(out[k], ref["out"][k]), (n, k, out[k], ref["out"][k])
        assert np.array_equal(_n(trk.dropped), ref["dropped"]) and np.array_equal(_n(trk.next_id), ref["next_id"]), n
        new = ref["out"]["age"] == 0                         # new corners: integers and the detector's covariance
        live = np.arange(len(new)) < ref["out"]["offsets"][-1]
        assert np.array_equal(out["tmpl_pts"][new & live], ref["out"]["tmpl_pts"][new & live])
        assert np.allclose(out["cov"][new & live], ref["out"]["cov"][new & live], rtol=1e-6)
        assert np.all(np.isnan(out["pts"][~live])) and np.all(out["id"][~live] == -1)
    # the last retained set goes into the ingest as it stands, and a solve runs
    offs = _n(retained.offsets)
    assert np.all(np.diff(offs) >= 3), offs
    K = np.array([[110.0, 0.0, (W0 - 1) / 2.0], [0.0, 110.0, (H0 - 1) / 2.0], [0.0, 0.0, 1.0]])
    b = Batch(capi.MODE_TARGET, offs)
    m = int(offs[-1])
    b.fill_keypoints(retained.prev_pts[:m], retained.pts[:m], retained.cov[:m], K_inv=np.linalg.inv(K))
    q0 = torch.tensor([[0.0, 0.0, 0.0, 1.0]] * SEQ_F, dtype=torch.float64, device="cuda")
    t0 = torch.tensor([[1.0, 0.1, 0.1]] * SEQ_F, dtype=torch.float64, device="cuda")
    res = b.solve(q0, t0)
    torch.cuda.synchronize()
    R, tt = res.rotation_matrices().cpu().numpy(), res.t.cpu().numpy()
    assert np.all(np.isfinite(R)) and np.all(np.isfinite(tt)) and np.all(np.isfinite(res.cost.cpu().numpy()))
    b.close()


# ---- 5. the facade ----------------------------------------------------------------------------------------------------
def test_pypnec_retain_and_append_equal_the_python_layer_on_one_image():
    import pnec_amd.pypnec as pypnec
    kw = dict(retain_cases())["random statuses"]
    lo, hi = (int(x) for x in kw["s"]["offsets"][-2:])
    s = {k: (np.array([0, hi - lo]) if k == "offsets" else v[lo:hi]) for k, v in kw["s"].items()}
    trk = {k: v[lo:hi] for k, v in kw["trk"].items()}
    _, want = run_retain(dict(kw, s=s, trk=trk), _t)
    m = int(want["offsets"][1])
    got = pypnec.retain_tracks(s["id"], s["tmpl_image"], s["tmpl_pts"], s["age"], s["pts"], s["cov"], trk["pts"], trk["angle"],
                               trk["cov"], trk["status"], 0)
    assert 0 < m < hi - lo
    for key, a in zip(RETAIN_KEYS[1:], got):
        a = np.asarray(a)
        assert a.dtype == want[key].dtype and np.array_equal(a, want[key][:m]), key
    kw = dict(append_cases())["capacity 66"]
    f = 3
    lo, hi = (int(x) for x in kw["s"]["offsets"][f:f + 2])
    dlo, dhi = (int(x) for x in kw["det"]["offsets"][f:f + 2])
    s = {k: (np.array([0, hi - lo]) if k == "offsets" else v[lo:hi]) for k, v in kw["s"].items()}
    det = dict(offsets=np.array([0, dhi - dlo]), pts=kw["det"]["pts"][dlo:dhi], cov=kw["det"]["cov"][dlo:dhi])
    one = dict(kw, s=s, det=det, base=5, next_id=np.array([2 ** 40], np.int64), n_out=kw["capacity"])
    _, want, nid, dropped = run_append(one, _t)
    rows, nid1, dropped1 = pypnec.append_tracks(tuple(s[k] for k in SET_KEYS[1:]), det["pts"], det["cov"], 5, kw["capacity"], 2 ** 40)
    assert nid1 == nid[0] and dropped1 == dropped[0] and dropped1 > 0
    m = int(want["offsets"][1])
    for key, a in zip(SET_KEYS[1:], rows):
        a = np.asarray(a)
        assert a.dtype == want[key].dtype and np.array_equal(a, want[key][:m]), key
