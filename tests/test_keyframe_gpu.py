"""Keyframe pairs on the device: pnec_hip_tracks_keyframe against `keyframe_np` (tests/test_keyframe_cpu.py) in both memory
spaces, its stream order, KeyframeTracker and Odometry with every pair accepted against the plain forms, a sequence with
accepted, skipped and forced frames against the pieces it is made of, and the allocation / wait properties of the plain
Odometry with keyframes on.

`mean` is held to test_keyframe_cpu.MEAN_RTOL against numpy (the device may fuse dx*dx + dy*dy; at most 257 terms per
image) and is BITWISE equal between the spaces, between an image alone and in the batch, and between two calls."""
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_keyframe_cpu import (MEAN_RTOL, OUT_KEYS, THRESHOLD, assert_same, call_cases, keyframe_np, make_case,  # noqa: E402
                               margin_ok, same_bits)
from test_patch_track_cpu import H0, LEVELS, W0  # noqa: E402
from test_tracks_cpu import SEQ_CAPACITY, SEQ_EDGE, SEQ_F, SEQ_FRAMES, SEQ_GRID, _warped, sequence_fixture  # noqa: E402

import pnec_amd  # noqa: E402
from pnec_amd import Batch, KeyframeTracker, Odometry, Tracker, TrackSet, capi, keyframe_pairs  # noqa: E402
from pnec_amd.keyframes import new_keyframe_pairs, new_keyframe_state  # noqa: E402
from pnec_amd.odometry import start_rotation  # noqa: E402

pytestmark = pytest.mark.gpu

K = np.array([[110.0, 0.0, 63.5], [0.0, 110.0, 47.5], [0.0, 0.0, 1.0]])      # a synthetic camera for 128 x 96 pixels
K_INV = np.linalg.inv(K)
TRACKER4 = dict(levels=LEVELS, ring=4, grid=SEQ_GRID, capacity=SEQ_CAPACITY, edge=SEQ_EDGE)
TRACKER5 = dict(TRACKER4, ring=5)


def _torch():
    import torch
    return torch


def _dev(a):
    return None if a is None else _torch().from_numpy(np.ascontiguousarray(a)).cuda()


def _host(a):
    return None if a is None else (a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a))


def _sets(B, A, st, to=lambda a: a):
    """the dicts of test_keyframe_cpu as what keyframe_pairs takes (numpy as they are, or through `to`)"""
    from pnec_amd.keyframes import KeyframeState
    ts = lambda d: None if d is None else TrackSet(to(d["offsets"]), None, None, None, None, to(d["pts"]), None, to(d["cov"]),
                                                   src=to(d.get("src")))
    return ts(B), ts(A), None if st is None else KeyframeState(to(st["key_pts"]), to(st["key_cov"]), to(st["span"]))


def _as_dict(pairs, state):
    return dict(offsets=_host(pairs.offsets), key_pts=_host(pairs.key_pts), pts=_host(pairs.pts), cov=_host(pairs.cov),
                key_cov=_host(pairs.key_cov), row=_host(pairs.row), accepted=_host(pairs.accepted),
                mean=_host(pairs.mean_displacement), n_matches=_host(pairs.n_matches), next_key_pts=_host(state.key_pts),
                next_key_cov=_host(state.key_cov), next_span=_host(state.span))


def _bits_all(got, want, what):
    for k in OUT_KEYS:
        if want[k] is None:
            assert got[k] is None, (what, k)
        else:
            assert same_bits(got[k], want[k]), f"{what}: {k}: bits differ"


def _device_call(B, A, st, thr, max_span, out=None):
    torch = _torch()
    b, a, s = _sets(B, A, st, _dev)
    pairs, nxt = keyframe_pairs(b, a, s, thr, max_span, out=out)
    torch.cuda.synchronize()
    return pairs, nxt


RAGGED = [c for c in call_cases() if c[0].startswith("ragged")]


@pytest.mark.parametrize("case", RAGGED, ids=[c[0] for c in RAGGED])
def test_the_call_equals_numpy_in_both_spaces_alone_and_twice(case):
    torch = _torch()
    name, B, A, st, thr, max_span = case
    ref = keyframe_np(B, A, st, thr, max_span)
    assert margin_ok(ref, thr)
    F, N, n_new = len(A["offsets"]) - 1, len(B["pts"]), len(A["pts"])
    with_cov = A["cov"] is not None
    # HOST space
    host = _as_dict(*keyframe_pairs(*_sets(B, A, st), thr, max_span))
    assert_same(host, ref, f"{name}, HOST space")
    # DEVICE space, into buffers full of a sentinel: padding is written to the end of every array
    out = (new_keyframe_pairs(F, N, True, "cuda:0", cov=with_cov), new_keyframe_state(F, n_new, True, "cuda:0", cov=with_cov))
    for obj in out:
        for t in vars(obj).values():
            if t is not None:
                t.fill_(91)
    dev = _as_dict(*_device_call(B, A, st, thr, max_span, out=out))
    assert_same(dev, ref, f"{name}, DEVICE space")
    _bits_all(dev, host, f"{name}, DEVICE against HOST space")
    end = int(ref["offsets"][-1])
    assert end < N and np.isnan(dev["key_pts"][end:]).all() and np.isnan(dev["pts"][end:]).all() and (dev["row"][end:] == -1).all()
    assert np.isnan(dev["next_key_pts"][int(A["offsets"][-1]):]).all() and int(A["offsets"][-1]) < n_new
    if with_cov:
        assert np.isnan(dev["cov"][end:]).all() and np.isnan(dev["key_cov"][end:]).all()
        assert np.isnan(dev["next_key_cov"][int(A["offsets"][-1]):]).all()
    # a second call into the same buffers
    _bits_all(_as_dict(*_device_call(B, A, st, thr, max_span, out=out)), dev, f"{name}, the second call")
    # each image alone
    for f in range(F):
        lo, hi, la, ha = int(B["offsets"][f]), int(B["offsets"][f + 1]), int(A["offsets"][f]), int(A["offsets"][f + 1])
        cut = lambda d, a, b, keys: {k: (None if d[k] is None else d[k][a:b]) for k in keys}
        Bf = dict(cut(B, lo, hi, ("pts", "cov", "src")), offsets=np.array([0, hi - lo], np.int64))
        Af = dict(cut(A, la, ha, ("pts", "cov")), offsets=np.array([0, ha - la], np.int64))
        stf = dict(st, span=st["span"][f:f + 1])
        one = _as_dict(*_device_call(Bf, Af, stf, thr, max_span))
        o0, o1 = int(dev["offsets"][f]), int(dev["offsets"][f + 1])
        n = o1 - o0
        assert int(one["offsets"][1]) == n, (name, f)
        for k in ("key_pts", "pts", "cov", "key_cov"):
            assert one[k] is None and dev[k] is None or same_bits(one[k][:n], dev[k][o0:o1]), (name, f, k)
        assert np.array_equal(one["row"][:n] + lo, dev["row"][o0:o1]) and (one["row"][n:] == -1).all()
        for k in ("accepted", "mean", "n_matches", "next_span"):
            assert same_bits(one[k], dev[k][f:f + 1]), (name, f, k)
        for k in ("next_key_pts", "next_key_cov"):
            assert one[k] is None and dev[k] is None or same_bits(one[k], dev[k][la:ha]), (name, f, k)
    torch.cuda.synchronize()


def test_the_first_frame_form_and_the_small_cases():
    for name, B, A, st, thr, max_span in call_cases():
        if name.startswith("ragged"):
            continue
        ref = keyframe_np(B, A, st, thr, max_span)
        host = _as_dict(*keyframe_pairs(*_sets(B, A, st), thr, max_span))
        dev = _as_dict(*_device_call(B, A, st, thr, max_span))
        assert_same(host, ref, f"{name}, HOST space")
        assert_same(dev, ref, f"{name}, DEVICE space")
        _bits_all(dev, host, f"{name}, DEVICE against HOST space")
        if B is None:
            assert (dev["accepted"] == 1).all() and (dev["offsets"] == 0).all() and (dev["next_span"] == 0).all()
            assert np.isnan(dev["mean"]).all() and dev["key_pts"].shape == (0, 2)


# ---- stream order ----------------------------------------------------------------------------------------------------
def test_the_device_call_respects_stream_order():
    from test_stream_order_gpu import Entry, check
    counts_b, counts_a, scales, spans = (0, 1, 63, 64, 65, 257), (5, 1, 40, 64, 70, 0), (1.0, 6.0, 0.5, 0.7, 8.0, 1.0), (0, 1, 0, 1, 0, 1)

    def data(seed):
        B, A, st = make_case(seed, counts_b, counts_a, scales, spans, True)
        d = dict(b_off=B["offsets"], b_pts=B["pts"], b_cov=B["cov"], b_src=B["src"], a_off=A["offsets"], a_pts=A["pts"],
                 a_cov=A["cov"], k_pts=st["key_pts"], k_cov=st["key_cov"], span=st["span"])
        return {k: _dev(v) for k, v in d.items()}
    good, decoy = data(21), data(22)
    F, N, n_new = len(counts_b), int(good["b_pts"].shape[0]), int(good["a_pts"].shape[0])
    out = (new_keyframe_pairs(F, N, True, "cuda:0"), new_keyframe_state(F, n_new, True, "cuda:0"))
    tensors = [t for obj in out for t in vars(obj).values()]

    def call(b):
        from pnec_amd.keyframes import KeyframeState
        ret = TrackSet(b["b_off"], None, None, None, None, b["b_pts"], None, b["b_cov"], src=b["b_src"])
        app = TrackSet(b["a_off"], None, None, None, None, b["a_pts"], None, b["a_cov"])
        keyframe_pairs(ret, app, KeyframeState(b["k_pts"], b["k_cov"], b["span"]), THRESHOLD, 2, out=out)
        return tensors, None
    check(Entry(good, decoy, call, sentinels=tensors), "tracks_keyframe")


# ---- every pair accepted: the plain forms ----------------------------------------------------------------------------
def _frames():
    torch = _torch()
    return [torch.from_numpy(np.array(a)).cuda() for a in sequence_fixture()["frames"]]


def _tbits(a, b, what):
    assert same_bits(_host(a), _host(b)), f"{what}: bits differ"


def test_with_every_pair_accepted_the_pairs_and_the_poses_are_the_plain_ones():
    torch = _torch()
    frames = _frames()
    tiny = 1e-300
    kft, trk = KeyframeTracker(SEQ_F, H0, W0, min_displacement=tiny, **TRACKER4), Tracker(SEQ_F, H0, W0, **TRACKER4)
    odo_k, odo = Odometry(SEQ_F, H0, W0, K_INV, min_displacement=tiny, **TRACKER4), Odometry(SEQ_F, H0, W0, K_INV, **TRACKER4)
    assert odo.keyframes is None and odo_k.keyframes is not None and kft.max_span == 2
    assert kft.process(frames[0]) is None and trk.process(frames[0]) is None
    assert odo_k.process(frames[0]) is None and odo.process(frames[0]) is None
    for n in range(1, SEQ_FRAMES):
        pairs, want = kft.process(frames[n]), trk.process(frames[n])
        assert bool((pairs.accepted == 1).all()), n
        for got, ref, what in ((pairs.offsets, want.offsets, "offsets"), (pairs.key_pts, want.prev_pts, "prev_pts"),
                               (pairs.pts, want.pts, "pts"), (pairs.cov, want.cov, "cov"), (pairs.key_cov, want.prev_cov, "prev_cov")):
            _tbits(got, ref, f"frame {n}: {what}")
        a, b = odo_k.process(frames[n]), odo.process(frames[n])
        _tbits(a.q, b.q, f"frame {n}: q")
        _tbits(a.t, b.t, f"frame {n}: t")
        _tbits(a.init_q, b.init_q, f"frame {n}: init_q")
        _tbits(a.n_corr, b.n_corr, f"frame {n}: n_corr")
        assert b.accepted is None and bool((a.accepted == 1).all()) and bool((a.span == 0).all())
    torch.cuda.synchronize()
    odo_k.close()
    odo.close()


# ---- a sequence with accepted, skipped and forced frames -------------------------------------------------------------
SKIP_FRAMES, SKIP_MIN, SKIP_SPAN = 7, 2.5, 3
SKIP_TIMES = ([0, 1, 2, 3, 4, 5, 6],                       # the fixture's step every frame: about 5 px
              [0, 1, 2, 2, 2, 3, 4],                       # a frame repeated twice in the middle
              [0.1 * n for n in range(7)])                 # a tenth of the step: about 0.5 px per frame


def _skip_frames():
    return [np.round(np.stack([_warped(300 + f, SKIP_TIMES[f][n]) for f in range(3)])).astype(np.uint8) for n in range(SKIP_FRAMES)]


def _read_sets(trk, retained):
    B = None if retained is None else dict(offsets=_host(retained.offsets), pts=_host(retained.pts), cov=_host(retained.cov),
                                           src=_host(retained.src))
    A = dict(offsets=_host(trk.tracks.offsets), pts=_host(trk.tracks.pts), cov=_host(trk.tracks.cov))
    return B, A


def test_a_sequence_with_accepted_skipped_and_forced_frames_equals_its_pieces():
    """Three sequences of seven frames, ring 5, min_displacement 2.5, max_span 3.  Every step is held to its pieces: a
    stand-alone Tracker's sets read back, `keyframe_np` carried from step to step, a second capacity batch filled from the
    expected pairs and the chain from the last accepted rotation.  On an MI355X the means were 4.8 - 5.2 px (sequence 0),
    5.1 - 5.2 and 0.0 (sequence 1: the repeated frame) and 0.4 - 1.6 px (sequence 2, forced at frame 3 with 1.58 px);
    sequence 2's tracks of frame 0 are retired by the ring right after that forced pair, so its frame 5 is accepted
    without a match -- the deviation include/pnec_hip.h states."""
    torch = _torch()
    F, cap = 3, SEQ_CAPACITY
    frames = [torch.from_numpy(a).cuda() for a in _skip_frames()]
    odo = Odometry(F, H0, W0, K_INV, min_displacement=SKIP_MIN, max_span=SKIP_SPAN, **TRACKER5)
    trk = Tracker(F, H0, W0, **TRACKER5)
    ref_batch = Batch.with_capacity(capi.MODE_TARGET, F, F * cap, device=0)
    ref_batch.reshape(np.arange(F + 1, dtype=np.int64) * cap)
    identity = torch.tensor([[0.0, 0.0, 0.0, 1.0]] * F, dtype=torch.float64, device="cuda:0")
    zero_t = torch.zeros((F, 3), dtype=torch.float64, device="cuda:0")
    assert odo.process(frames[0]) is None and trk.process(frames[0]) is None
    _, A = _read_sets(trk, None)
    r = keyframe_np(None, A, None, SKIP_MIN, SKIP_SPAN)
    state = dict(key_pts=r["next_key_pts"], key_cov=r["next_key_cov"], span=r["next_span"])
    prev_q, seen = None, set()
    for n in range(1, SKIP_FRAMES):
        out = odo.process(frames[n])
        B, A = _read_sets(trk, trk.process(frames[n]))
        r = keyframe_np(B, A, state, SKIP_MIN, SKIP_SPAN)
        fin = np.isfinite(r["mean"])
        print(f"frame {n}: matches {r['n_matches'].tolist()}, mean {np.round(r['mean'], 3).tolist()}, accepted "
              f"{r['accepted'].tolist()}, span {r['next_span'].tolist()}")
        assert (np.abs(r["mean"][fin] - SKIP_MIN) > 0.5).all(), (n, r["mean"])
        below = r["mean"] < SKIP_MIN
        seen |= ({"accept"} if ((r["accepted"] == 1) & ~below & fin).any() else set()) | \
            ({"skip"} if (r["accepted"] == 0).any() else set()) | ({"forced"} if ((r["accepted"] == 1) & below).any() else set())
        got = _as_dict(out.pairs, odo.keyframes.state)
        assert_same(got, r, f"frame {n}")
        _tbits(out.accepted, r["accepted"], f"frame {n}: result.accepted")
        _tbits(out.span, r["next_span"], f"frame {n}: result.span")
        assert np.array_equal(_host(out.n_corr), np.diff(r["offsets"]).astype(np.int32)) and out.n_corr.dtype == torch.int32
        gm, rm = _host(out.mean_displacement), r["mean"]
        assert np.array_equal(np.isnan(gm), np.isnan(rm)) and np.all(np.abs(gm[fin] - rm[fin]) <= MEAN_RTOL * np.abs(rm[fin]))
        # the poses: a second capacity batch shaped by the expected pairs, the chain from the last accepted rotation
        init_q = start_rotation(prev_q, identity)
        _tbits(out.init_q, init_q, f"frame {n}: init_q")
        ref_batch.fill_keypoints_ragged(_dev(r["offsets"]), _dev(r["key_pts"]), _dev(r["pts"]), _dev(r["cov"]), K_inv=K_INV)
        q, t = ref_batch.solve_pipeline(init_q, zero_t, None)
        torch.cuda.synchronize()
        acc = r["accepted"].astype(bool)
        gq, gt = _host(out.q), _host(out.t)
        assert same_bits(gq[acc], _host(q)[acc]) and same_bits(gt[acc], _host(t)[acc]), f"frame {n}: poses of accepted pairs"
        assert np.isnan(gq[~acc]).all() and np.isnan(gt[~acc]).all(), f"frame {n}: poses of skipped pairs"
        keep = torch.from_numpy(acc).cuda()[:, None]
        prev_q = torch.where(keep, q, torch.full_like(q, float("nan")) if prev_q is None else prev_q)
        state = dict(key_pts=r["next_key_pts"], key_cov=r["next_key_cov"], span=r["next_span"])
    assert seen == {"accept", "skip", "forced"}, seen
    ref_batch.close()
    odo.close()


# ---- allocation and wait ---------------------------------------------------------------------------------------------
def test_the_batch_is_shaped_once_and_no_step_allocates_in_the_library():
    from pnec_amd.multi import alloc_counters
    torch = _torch()
    frames = _frames()
    odo = Odometry(SEQ_F, H0, W0, K_INV, min_displacement=SKIP_MIN, **TRACKER4)
    assert odo.batch.n_pairs == SEQ_F and odo.capacity == SEQ_CAPACITY
    for n in range(3):
        odo.process(frames[n])
    torch.cuda.synchronize()
    a0 = alloc_counters()
    odo.process(frames[3])
    torch.cuda.synchronize()
    assert alloc_counters()["hip_malloc_calls"] == a0["hip_malloc_calls"]
    odo.close()


def test_process_returns_while_a_delay_queued_before_it_still_runs():
    from test_stream_order_gpu import DELAY_MS, _delay
    torch = _torch()
    frames = _frames()
    ref = Odometry(SEQ_F, H0, W0, K_INV, min_displacement=SKIP_MIN, **TRACKER4)
    for n in range(3):
        want = ref.process(frames[n])
    want = [want.q.clone(), want.t.clone(), want.n_corr.clone(), want.accepted.clone(), want.mean_displacement.clone()]
    odo = Odometry(SEQ_F, H0, W0, K_INV, min_displacement=SKIP_MIN, **TRACKER4)
    odo.process(frames[0])
    odo.process(frames[1])
    torch.cuda.synchronize()
    _delay(0)
    S = torch.cuda.Stream()
    with torch.cuda.stream(S):
        _delay(DELAY_MS)
        gate = torch.cuda.Event()
        gate.record()
        t0 = time.perf_counter()
        out = odo.process(frames[2])
        host_ms = (time.perf_counter() - t0) * 1e3
        returned_early = not gate.query()
    S.synchronize()
    print(f"Odometry.process with keyframes: host side {host_ms:.3f} ms, returned_early={returned_early}")
    for name, a, b in zip(("q", "t", "n_corr", "accepted", "mean"), (out.q, out.t, out.n_corr, out.accepted, out.mean_displacement), want):
        _tbits(a, b, name)
    assert returned_early, f"process returned only after the work queued ahead of it had run ({host_ms:.1f} ms on the host)"
    ref.close()
    odo.close()
