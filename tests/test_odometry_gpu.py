"""pnec_amd.Odometry on the device: images in, poses out, nothing read back.

Three sequences of four frames at 96 x 128 (tests/test_tracks_cpu.py's sequence_fixture: a textured scene moved by a known
warp, one frame blank altogether -- so one pair has no correspondence, and the pair after it none either: no track
survives a blank frame).  At every step the result is held, BITWISE, to the pieces it is made of: the pairs are a
stand-alone Tracker's on the same images, n_corr their sizes, and the poses those of the manual chain -- offsets read
back, a host-shaped batch of the same bounds filled with fill_keypoints (real rows + filler) and cut down with select(),
solve_pipeline from the same start (the reference construction of tests/test_fill_ragged_gpu.py)."""
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_patch_track_cpu import H0, LEVELS, W0  # noqa: E402
from test_tracks_cpu import (RETAIN_KEYS, SEQ_CAPACITY, SEQ_EDGE, SEQ_F, SEQ_FRAMES, SEQ_GRID, SEQ_RING,  # noqa: E402
                             sequence_fixture)

from pnec_amd import Batch, Odometry, Tracker, capi  # noqa: E402
from pnec_amd.odometry import start_rotation  # noqa: E402

pytestmark = pytest.mark.gpu

K = np.array([[110.0, 0.0, 63.5], [0.0, 110.0, 47.5], [0.0, 0.0, 1.0]])      # a synthetic camera for 128 x 96 pixels
K_INV = np.linalg.inv(K)
TRACKER = dict(levels=LEVELS, ring=SEQ_RING, grid=SEQ_GRID, capacity=SEQ_CAPACITY, edge=SEQ_EDGE)


def _torch():
    import torch
    return torch


def _frames():
    torch = _torch()
    return [torch.from_numpy(np.array(a)).cuda() for a in sequence_fixture()["frames"]]


def _bits_equal(a, b, what):
    a, b = np.ascontiguousarray(a.cpu().numpy()), np.ascontiguousarray(b.cpu().numpy())
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"{what}: bits differ"


def manual_chain(pairs, init_q, options=None):
    """the section 3j form: read the offsets back, then a host-shaped batch of the bounds + select"""
    torch = _torch()
    F, cap = SEQ_F, SEQ_CAPACITY
    off = pairs.offsets.cpu().numpy()
    cnt = np.diff(off)
    assert (cnt >= 0).all() and (cnt <= cap).all()
    p1, p2, cv = (a.cpu().numpy() for a in (pairs.prev_pts, pairs.pts, pairs.cov))
    rows1, rows2 = np.full((F * cap, 2), 40.0), np.full((F * cap, 2), 41.0)          # filler: valid pixels
    rowsc = np.tile(np.array([0.5, 0.1, 0.5]), (F * cap, 1))
    mask = np.zeros(F * cap, dtype=np.uint8)
    for f in range(F):
        sl, src = slice(f * cap, f * cap + cnt[f]), slice(off[f], off[f + 1])
        rows1[sl], rows2[sl], rowsc[sl], mask[sl] = p1[src], p2[src], cv[src], 1
    src_batch = Batch(capi.MODE_TARGET, np.arange(F + 1, dtype=np.int64) * cap)
    src_batch.fill_keypoints(rows1, rows2, rowsc, K_inv=K_INV)
    sel = src_batch.select(mask)
    q, t = sel.solve_pipeline(init_q, torch.zeros((F, 3), dtype=torch.float64, device="cuda:0"), options)
    torch.cuda.synchronize()
    sel.close()
    src_batch.close()
    return q, t, cnt


def test_every_step_equals_the_tracker_and_the_manual_chain():
    torch = _torch()
    frames = _frames()
    odo = Odometry(SEQ_F, H0, W0, K_INV, **TRACKER)
    trk = Tracker(SEQ_F, H0, W0, **TRACKER)
    identity = torch.tensor([[0.0, 0.0, 0.0, 1.0]] * SEQ_F, dtype=torch.float64, device="cuda:0")
    assert odo.process(frames[0]) is None and trk.process(frames[0]) is None
    prev_q, empty_seen, fallback_seen = None, False, False
    for n in range(1, SEQ_FRAMES):
        out = odo.process(frames[n])
        want_pairs = trk.process(frames[n])
        for k in RETAIN_KEYS:
            _bits_equal(getattr(out.pairs, k), getattr(want_pairs, k), f"frame {n}: pairs.{k}")
        # the start-pose rule against its definition: the previous pair's rotation where it is finite, else the identity
        if prev_q is None:
            want_start = identity
        else:
            finite = torch.isfinite(prev_q).all(dim=1)
            want_start = prev_q.clone()
            want_start[~finite] = identity[~finite]
            fallback_seen |= bool((~finite).any())
        _bits_equal(out.init_q, want_start, f"frame {n}: start rotation")
        q, t, cnt = manual_chain(out.pairs, out.init_q)
        assert out.n_corr.dtype == torch.int32 and np.array_equal(out.n_corr.cpu().numpy(), cnt), n
        print(f"frame {n}: correspondences per pair {cnt.tolist()}, finite poses {torch.isfinite(out.q).all(dim=1).tolist()}")
        _bits_equal(out.q, q, f"frame {n}: q")
        _bits_equal(out.t, t, f"frame {n}: t")
        assert tuple(out.q.shape) == (SEQ_F, 4) and tuple(out.t.shape) == (SEQ_F, 3)
        empty_seen |= bool((cnt == 0).any())
        prev_q = out.q.clone()
    assert empty_seen, "the fixture's blank frame must give a pair without correspondences"
    # the identity fallback itself (whether the chain's pose of an empty pair is finite is the chain's business)
    bad = torch.tensor([[0.1, 0.2, 0.3, 0.9], [float("nan"), 0.0, 0.0, 1.0], [0.0, float("inf"), 0.0, 1.0]],
                       dtype=torch.float64, device="cuda:0")
    got = start_rotation(bad, identity).cpu().numpy()
    assert np.array_equal(got[0], [0.1, 0.2, 0.3, 0.9]) and np.array_equal(got[1:], [[0, 0, 0, 1]] * 2)
    assert np.array_equal(start_rotation(None, identity).cpu().numpy(), identity.cpu().numpy())
    print("identity fallback taken inside the sequence:", fallback_seen)
    odo.close()


def test_the_batch_is_shaped_once_and_no_step_allocates_in_the_library():
    from pnec_amd.multi import alloc_counters
    torch = _torch()
    frames = _frames()
    odo = Odometry(SEQ_F, H0, W0, K_INV, **TRACKER)
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
    ref = Odometry(SEQ_F, H0, W0, K_INV, **TRACKER)
    for n in range(3):
        want = ref.process(frames[n])
    want = [want.q.clone(), want.t.clone(), want.n_corr.clone()]
    odo = Odometry(SEQ_F, H0, W0, K_INV, **TRACKER)
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
    print(f"Odometry.process: host side {host_ms:.3f} ms, returned_early={returned_early}")
    for name, a, b in zip(("q", "t", "n_corr"), (out.q, out.t, out.n_corr), want):
        _bits_equal(a, b, name)
    assert returned_early, f"process returned only after the work queued ahead of it had run ({host_ms:.1f} ms on the host)"
    ref.close()
    odo.close()
