"""Stored patches on the device: Tracker(templates="patches") in lockstep with a ring tracker that never retires a track
-- every row of every set BITWISE equal, padding included, in every column but the slot / image index --, the slot
column against assign_slots_np (tests/test_patch_store_cpu.py), a sequence alone against the batch, HOST against DEVICE
space through the two calls, their stream order, keyframe pairs that span four frames against keyframe_np, Odometry's
poses, and the allocation / wait properties of process.

Equality is of bits throughout: the stored templates are the terms the indexed tracker rebuilds, in its order of
operations, in double, so no tolerance is needed or given."""
import functools
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_keyframe_cpu import assert_same as assert_same_keyframe  # noqa: E402
from test_keyframe_cpu import keyframe_np  # noqa: E402
from test_patch_store_cpu import STORE_FRAMES, assign_slots_np, store_fixture  # noqa: E402
from test_patch_track_cpu import BAD, H0, LEVELS, LOSTB, FAR, W0  # noqa: E402
from test_tracks_cpu import (RETAIN_KEYS, SEQ_CAPACITY, SEQ_EDGE, SEQ_F, SEQ_GRID, SET_KEYS, _warped,  # noqa: E402
                             sequence_fixture)

import pnec_amd  # noqa: E402
from pnec_amd import (KeyframeTracker, Odometry, PatchStore, Tracker, TrackSet, add_patches, capi,  # noqa: E402
                      new_patch_store, patch_track_stored)

pytestmark = pytest.mark.gpu

TRACK_KEYS = ("pts", "angle", "cov", "dist2", "status", "lost_level")
KW = dict(levels=LEVELS, grid=SEQ_GRID, capacity=SEQ_CAPACITY, edge=SEQ_EDGE)
K_INV = np.linalg.inv(np.array([[110.0, 0.0, 63.5], [0.0, 110.0, 47.5], [0.0, 0.0, 1.0]]))
N = SEQ_F * SEQ_CAPACITY


def _torch():
    import torch
    return torch


def _t(a):
    return None if a is None else _torch().from_numpy(np.array(a)).cuda()


def _n(a):
    return None if a is None else (a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a))


def _bits(a, b, what):
    a, b = np.ascontiguousarray(_n(a)), np.ascontiguousarray(_n(b))
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), \
        f"{what}: bits differ in rows {np.flatnonzero((a.view(np.uint8) != b.view(np.uint8)).reshape(len(a), -1).any(1))[:10]}"


def _patches(F=SEQ_F, **kw):
    return Tracker(F, H0, W0, ring=2, templates="patches", **dict(KW, **kw))


def _snap(trk, retained):
    """numpy copies of what a step left behind"""
    d = dict(tracks={k: _n(getattr(trk.tracks, k)) for k in SET_KEYS}, dropped=_n(trk.dropped), next_id=_n(trk.next_id),
             retained=None, last=None)
    if retained is not None:
        d["retained"] = {k: _n(getattr(retained, k)) for k in RETAIN_KEYS}
        d["last"] = {k: _n(getattr(trk.last_track, k)) for k in TRACK_KEYS}
    return d


def lockstep(frames, ring_ref, what):
    """a "patches" tracker and a ring tracker of `ring_ref` pyramids over `frames`; -> the patches tracker's snapshots"""
    torch = _torch()
    a, b = _patches(), Tracker(SEQ_F, H0, W0, ring=ring_ref, **KW)
    assert a.store is not None and a.store.n_slots == N and b.store is None and a.ring == 2
    snaps, prev_slot = [], None
    for n, img in enumerate(frames):
        ra, rb = a.process(_t(img)), b.process(_t(img))
        torch.cuda.synchronize()
        sa, sb = _snap(a, ra), _snap(b, rb)
        for k in SET_KEYS:
            if k != "tmpl_image":
                _bits(sa["tracks"][k], sb["tracks"][k], f"{what}, frame {n}: tracks.{k}, all {N} rows")
        _bits(sa["dropped"], sb["dropped"], f"{what}, frame {n}: dropped")
        _bits(sa["next_id"], sb["next_id"], f"{what}, frame {n}: next_id")
        assert (sa["retained"] is None) == (n == 0) == (sb["retained"] is None)
        if n > 0:
            for k in RETAIN_KEYS:
                if k != "tmpl_image":
                    _bits(sa["retained"][k], sb["retained"][k], f"{what}, frame {n}: retained.{k}, all {N} rows")
            for k in TRACK_KEYS:
                _bits(sa["last"][k], sb["last"][k], f"{what}, frame {n}: last_track.{k}, all {N} rows")
        # the slot column: the retained rows' slots carried by retain and append, the rest by the rule
        off = sa["tracks"]["offsets"]
        col = np.zeros(N, np.int32)
        coff = None
        if n > 0:
            r = sa["retained"]
            coff = r["offsets"]
            _bits(r["tmpl_image"][:coff[-1]], prev_slot[r["src"][:coff[-1]]], f"{what}, frame {n}: a retained row keeps its slot")
            for f in range(SEQ_F):
                take = min(int(coff[f + 1] - coff[f]), int(off[f + 1] - off[f]))
                col[off[f]:off[f] + take] = r["tmpl_image"][coff[f]:coff[f] + take]
        want = assign_slots_np(col, off, coff, SEQ_CAPACITY, strict=True)
        assert np.array_equal(sa["tracks"]["tmpl_image"], want), (what, n, sa["tracks"]["tmpl_image"], want)
        prev_slot = sa["tracks"]["tmpl_image"]
        snaps.append(sa)
    return snaps


@functools.lru_cache(maxsize=None)
def eight_frames():
    """the eight-frame run, once: the snapshots of the patches tracker"""
    return lockstep(store_fixture()["frames"], 10, "eight frames against ring 10")


# ---- 1., 2. in lockstep with a ring that never retires ----------------------------------------------------------------
def test_eight_frames_in_lockstep_with_a_ring_of_ten_bitwise_and_the_slots_by_the_rule():
    torch = _torch()
    snaps = eight_frames()
    short = Tracker(SEQ_F, H0, W0, ring=3, **KW)
    moved = False
    for n, img in enumerate(store_fixture()["frames"]):
        r = short.process(_t(img))
        torch.cuda.synchronize()
        if n >= 2:
            assert int(r.offsets[-1]) < int(snaps[n]["retained"]["offsets"][-1]), f"frame {n}: the ring of 3 retains as many rows"
        off = snaps[n]["tracks"]["offsets"]
        for f in range(SEQ_F):
            moved |= bool(np.any(snaps[n]["tracks"]["tmpl_image"][off[f]:off[f + 1]] - f * SEQ_CAPACITY != np.arange(off[f + 1] - off[f])))
    last = snaps[-1]["retained"]
    assert int(last["age"][:last["offsets"][-1]].max()) >= 6, "no retained row of age 6 or more at frame 7"
    assert moved, "slot == row everywhere: no freed slot was reused"


def test_the_four_frame_fixture_in_lockstep_with_a_ring_of_six():
    snaps = lockstep(sequence_fixture()["frames"], 6, "four frames against ring 6")
    live_status, pad_status, empty = set(), set(), False
    for n in range(1, len(snaps)):
        end = int(snaps[n - 1]["tracks"]["offsets"][-1])
        live_status |= set(snaps[n]["last"]["status"][:end].tolist())
        pad_status |= set(snaps[n]["last"]["status"][end:].tolist())
        empty |= bool(np.any(np.diff(snaps[n - 1]["tracks"]["offsets"]) == 0))
    assert {LOSTB, FAR} <= live_status and pad_status == {BAD} and empty


# ---- 3. a sequence alone ----------------------------------------------------------------------------------------------
def test_each_sequence_alone_has_the_bits_of_its_rows_in_the_batch():
    torch = _torch()
    snaps = eight_frames()
    for f in range(SEQ_F):
        one = _patches(F=1)
        for n, img in enumerate(store_fixture()["frames"]):
            r = one.process(_t(img[f:f + 1]))
            torch.cuda.synchronize()
            s = _snap(one, r)
            for name in ("tracks", "retained"):
                if s[name] is None:
                    continue
                batch = snaps[n][name]
                lo, hi = int(batch["offsets"][f]), int(batch["offsets"][f + 1])
                m = int(s[name]["offsets"][1])
                assert m == hi - lo, (f, n, name)
                for k in s[name]:
                    if k == "offsets":
                        continue
                    got = s[name][k][:m]
                    got = got + f * SEQ_CAPACITY if k == "tmpl_image" else (got + snaps[n - 1]["tracks"]["offsets"][f] if k == "src" else got)
                    _bits(got, batch[k][lo:hi], f"sequence {f} alone, frame {n}: {name}.{k}")


# ---- 4. HOST space through the two calls ------------------------------------------------------------------------------
def test_one_step_in_host_space_equals_the_device_step_bitwise_and_twice():
    torch = _torch()
    frames = store_fixture()["frames"]
    trk = _patches()
    for n in range(7):
        trk.process(_t(frames[n]))
    torch.cuda.synchronize()
    A = {k: _n(getattr(trk.tracks, k)) for k in SET_KEYS}                    # the set after frame 6: an image of 7 rows
    store_before = _n(trk.store.data).copy()
    prev = [_n(lv).copy() for lv in trk._slot(6)]
    retained = trk.process(_t(frames[7]))
    torch.cuda.synchronize()
    cur = [_n(lv).copy() for lv in trk._slot(7)]
    want_track = {k: _n(getattr(trk.last_track, k)) for k in TRACK_KEYS}
    want_slot, want_store = _n(trk.tracks.tmpl_image), _n(trk.store.data)
    assert not np.array_equal(want_store, store_before), "frame 7 built no patch"
    end = int(A["offsets"][-1])
    assert end < N and np.all(A["tmpl_image"][end:] == -1)

    def both(conv):
        """the tracking call and the add of step 7 with arrays made by `conv` -> (PatchTrack outputs, slot, store)"""
        st = PatchStore(conv(store_before), LEVELS, SEQ_CAPACITY)
        ts = TrackSet(*[conv(A[k]) for k in SET_KEYS])
        r = patch_track_stored(st, [conv(a) for a in prev], [conv(a) for a in cur], ts)
        # what append left: the carried rows' slots, and something else in the rows the call assigns
        B = TrackSet(*[conv(_n(getattr(trk.tracks, k))) for k in SET_KEYS])
        col = _n(B.tmpl_image).copy()
        new = np.ones(N, bool)
        off, coff = _n(B.offsets), _n(retained.offsets)
        for f in range(SEQ_F):
            new[off[f]:off[f] + min(coff[f + 1] - coff[f], off[f + 1] - off[f])] = False
        col[new] = 77
        B.tmpl_image = conv(col)
        add_patches(st, [conv(a) for a in cur], B, carried_offsets=conv(_n(retained.offsets)))
        if hasattr(B.tmpl_image, "is_cuda"):
            torch.cuda.synchronize()
        return {k: _n(getattr(r, k)) for k in TRACK_KEYS}, _n(B.tmpl_image), _n(st.data)

    for name, conv in (("HOST", lambda a: np.array(a)), ("DEVICE", _t), ("HOST, the second call", lambda a: np.array(a))):
        got_track, got_slot, got_store = both(conv)
        for k in TRACK_KEYS:
            _bits(got_track[k], want_track[k], f"{name} space: patch_track_stored {k}")
        _bits(got_slot, want_slot, f"{name} space: the slot column")
        _bits(got_store, want_store, f"{name} space: the store")
    # a padding row's slot and an out-of-range one: bad at the top level in DEVICE space, refused in HOST space
    wild = A["tmpl_image"].copy()
    wild[0], wild[1] = N, -3
    st = PatchStore(_t(store_before), LEVELS, SEQ_CAPACITY)
    ts = TrackSet(*[_t(A[k]) for k in SET_KEYS])
    ts.tmpl_image = _t(wild)
    r = patch_track_stored(st, [_t(a) for a in prev], [_t(a) for a in cur], ts)
    torch.cuda.synchronize()
    for k in (0, 1, N - 1):
        assert int(r.status[k]) == BAD and int(r.lost_level[k]) == LEVELS - 1 and bool(torch.isnan(r.cov[k]).all()) and \
            bool(torch.isnan(r.dist2[k]))
    _bits(r.pts[:2], A["pts"][:2], "a row without a slot: out_pts is the start")
    _bits(r.angle[:2], A["angle"][:2], "a row without a slot: out_angle is the start angle")
    for k in TRACK_KEYS:
        _bits(_n(getattr(r, k))[2:], want_track[k][2:], f"the other rows are not touched by a bad slot: {k}")
    with pytest.raises(capi.PnecHipError) as ei:
        patch_track_stored(PatchStore(store_before.copy(), LEVELS, SEQ_CAPACITY), prev, cur,
                           TrackSet(*[(wild if k == "tmpl_image" else A[k]) for k in SET_KEYS]))
    assert ei.value.code == capi.ERR_INVALID_ARGUMENT and "slot" in str(ei.value)


# ---- 5. stream order --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["patch_store_add", "patch_track_stored"])
def test_device_space_calls_respect_stream_order(which):
    from test_tracks_gpu import _probe
    torch = _torch()
    frames = store_fixture()["frames"]
    trk = _patches()
    for n in range(4):
        trk.process(_t(frames[n]))
    torch.cuda.synchronize()
    A = {k: getattr(trk.tracks, k).clone() for k in SET_KEYS}
    store0 = trk.store.data.clone()
    prev, cur = [lv.clone() for lv in trk._slot(3)], pnec_amd.image_pyramid(_t(frames[4]), LEVELS)
    end = int(A["offsets"][-1])
    pat = _t(np.array(pnec_amd.PATTERN52))               # (a host pattern would be copied up: a wait for the stream)
    perm = torch.cat([torch.arange(end - 1, -1, -1, device="cuda"), torch.arange(end, N, device="cuda")])
    if which == "patch_track_stored":
        st = PatchStore(store0, LEVELS, SEQ_CAPACITY)
        good = dict(slot=A["tmpl_image"], pts=A["pts"])
        decoy = dict(slot=A["tmpl_image"][perm].contiguous(), pts=A["pts"][perm].contiguous())
        outs = {}

        def call(b):
            r = patch_track_stored(st, prev, cur, (A["offsets"], A["tmpl_pts"], b["slot"], b["pts"], A["angle"]), pattern=pat)
            for k in TRACK_KEYS:                      # (the call allocates: the probe wants the same tensors every time)
                if k not in outs:
                    outs[k] = torch.empty_like(getattr(r, k))
                outs[k].copy_(getattr(r, k))
            return [outs[k] for k in TRACK_KEYS]
        _probe("patch_track_stored", good, decoy, call)
    else:
        st = PatchStore(store0.clone(), LEVELS, SEQ_CAPACITY)
        carried = A["offsets"] // 2                      # half of every image's rows carried, the rest to be assigned
        good = dict(slot=A["tmpl_image"], tmpl_pts=A["tmpl_pts"])
        decoy = dict(slot=A["tmpl_image"][perm].contiguous(), tmpl_pts=(A["tmpl_pts"][perm] + 1.0).contiguous())

        def call(b):
            st.data.copy_(store0)
            ts = TrackSet(A["offsets"], A["id"], b["slot"], b["tmpl_pts"], A["age"], A["pts"], A["angle"], A["cov"])
            add_patches(st, cur, ts, carried_offsets=carried, pattern=pat)
            return [b["slot"], st.data]
        _probe("patch_store_add", good, decoy, call)


# ---- 6. keyframe pairs that span four frames --------------------------------------------------------------------------
KEY_FRAMES, KEY_STEP, KEY_MARGIN = 9, 0.25, 0.5
# Per sequence, midway between the largest third and the smallest fourth mean after a key frame in the numpy frame loop
# without an age limit (test_patch_store_cpu.store_reference's steps on these frames), whose means per sequence are
#     frame 1  1.2068 1.2898 1.3538    frame 5  1.2518 1.2963 1.2545
#     frame 2  2.4143 2.5751 2.6330    frame 6  2.5089 2.5702 2.5962
#     frame 3  3.6688 3.8648 3.8815    frame 7  3.7829 3.8421 3.8282
#     frame 4  4.8164 5.1535 5.2155    frame 8  4.9989 5.1367 5.1909
# with 3 / 8 / 5 matches up to frame 4 and 6 / 8 / 8 after it: (3.7829 + 4.8164) / 2, (3.8648 + 5.1367) / 2,
# (3.8815 + 5.1909) / 2.  min_displacement is one number per tracker, and no single one keeps 0.5 px from every mean of
# all three sequences (sequence 0's fourth mean, 4.8164, is 0.935 px above sequence 2's third, 3.8815), so each sequence
# is held to numpy in a tracker of its own, with its own threshold; the three in lockstep are then held to those runs.
KEY_THRESHOLDS = (4.30, 4.50, 4.54)
KEY_THRESHOLD_LOCKSTEP = 4.35
PAIR_ROWS = ("key_pts", "pts", "cov", "key_cov")
PER_IMAGE = ("accepted", "mean", "n_matches", "next_span")


def _read(trk, retained):
    B = None if retained is None else dict(offsets=_n(retained.offsets), pts=_n(retained.pts), cov=_n(retained.cov), src=_n(retained.src))
    return B, dict(offsets=_n(trk.tracks.offsets), pts=_n(trk.tracks.pts), cov=_n(trk.tracks.cov))


def _pairs_dict(pairs, state):
    return dict(offsets=_n(pairs.offsets), key_pts=_n(pairs.key_pts), pts=_n(pairs.pts), cov=_n(pairs.cov), key_cov=_n(pairs.key_cov),
                row=_n(pairs.row), accepted=_n(pairs.accepted), mean=_n(pairs.mean_displacement), n_matches=_n(pairs.n_matches),
                next_key_pts=_n(state.key_pts), next_key_cov=_n(state.key_cov), next_span=_n(state.span))


def _key_frames():
    return [np.round(np.stack([_warped(300 + f, KEY_STEP * n) for f in range(SEQ_F)])).astype(np.uint8) for n in range(KEY_FRAMES)]


def test_keyframe_pairs_span_four_frames_without_a_forced_acceptance():
    """Nine frames a quarter of the fixture's step apart (about 1.25 px a frame), max_span None.  Each sequence in a
    KeyframeTracker of its own (its threshold above): every step against keyframe_np carried from step to step on a
    stand-alone "patches" tracker's sets, every mean more than 0.5 px from the threshold, the accepted pairs span 4
    frames, have matches and lie above the threshold.  Then the three sequences in lockstep in one KeyframeTracker: every
    step has, image by image, the bits of the runs alone -- the decisions, the means and the pair rows."""
    torch = _torch()
    frames = _key_frames()
    big = 2 ** 31 - 1
    alone = []
    for f, thr in enumerate(KEY_THRESHOLDS):
        kft = KeyframeTracker(1, H0, W0, min_displacement=thr, max_span=None, ring=2, templates="patches", **KW)
        trk = _patches(F=1)
        assert kft.max_span == big and kft.tracker.templates == "patches"
        first = _t(frames[0][f:f + 1])
        assert kft.process(first) is None and trk.process(first) is None
        _, A = _read(trk, None)
        r = keyframe_np(None, A, None, thr, big)
        state = dict(key_pts=r["next_key_pts"], key_cov=r["next_key_cov"], span=r["next_span"])
        spans, steps = [], [None]
        for n in range(1, KEY_FRAMES):
            img = _t(frames[n][f:f + 1])
            pairs = kft.process(img)
            B, A = _read(trk, trk.process(img))
            torch.cuda.synchronize()
            r = keyframe_np(B, A, state, thr, big)
            print(f"sequence {f}, frame {n}: matches {r['n_matches'].tolist()}, mean {np.round(r['mean'], 4).tolist()}, accepted "
                  f"{r['accepted'].tolist()}, span {state['span'].tolist()} -> {r['next_span'].tolist()}")
            assert np.all(np.isfinite(r["mean"])) and np.all(np.abs(r["mean"] - thr) > KEY_MARGIN), (f, n, r["mean"], thr)
            got = _pairs_dict(pairs, kft.state)
            assert_same_keyframe(got, r, f"sequence {f}, frame {n}")
            acc = r["accepted"].astype(bool)
            assert np.all(r["n_matches"][acc] > 0), f"sequence {f}, frame {n}: a pair accepted without a match"
            assert not np.any(r["mean"][acc] < thr), f"sequence {f}, frame {n}: a pair accepted below the threshold"
            spans += (state["span"][acc] + 1).tolist()
            state = dict(key_pts=r["next_key_pts"], key_cov=r["next_key_cov"], span=r["next_span"])
            steps.append(got)
        assert spans == [4, 4], (f, spans)
        alone.append(steps)
    # in lockstep: one threshold between every third and every fourth mean, so the decisions are those of the runs alone
    kft = KeyframeTracker(SEQ_F, H0, W0, min_displacement=KEY_THRESHOLD_LOCKSTEP, max_span=None, ring=2, templates="patches", **KW)
    assert kft.process(_t(frames[0])) is None
    for n in range(1, KEY_FRAMES):
        got = _pairs_dict(kft.process(_t(frames[n])), kft.state)
        torch.cuda.synchronize()
        off = got["offsets"]
        for f in range(SEQ_F):
            one = alone[f][n]
            m = int(one["offsets"][1])
            assert int(off[f + 1] - off[f]) == m, (n, f)
            for k in PAIR_ROWS:
                _bits(got[k][off[f]:off[f + 1]], one[k][:m], f"lockstep, frame {n}, sequence {f}: {k}")
            for k in PER_IMAGE:
                _bits(got[k][f:f + 1], one[k], f"lockstep, frame {n}, sequence {f}: {k}")
        assert got["accepted"].tolist() == ([1, 1, 1] if n in (4, 8) else [0, 0, 0]), (n, got["accepted"])


# ---- 7. Odometry ------------------------------------------------------------------------------------------------------
def test_odometry_on_stored_patches_gives_the_poses_of_a_ring_of_ten():
    torch = _torch()
    a = Odometry(SEQ_F, H0, W0, K_INV, ring=2, templates="patches", **KW)
    b = Odometry(SEQ_F, H0, W0, K_INV, ring=10, **KW)
    for n, img in enumerate(store_fixture()["frames"]):
        ra, rb = a.process(_t(img)), b.process(_t(img))
        if n == 0:
            assert ra is None and rb is None
            continue
        torch.cuda.synchronize()
        for k in ("q", "t", "n_corr"):
            _bits(getattr(ra, k), getattr(rb, k), f"frame {n}: {k}")
    assert bool(torch.isfinite(ra.q).all())
    a.close()
    b.close()


# ---- 8. allocation and wait -------------------------------------------------------------------------------------------
def test_process_allocates_nothing_in_the_library_and_returns_while_a_delay_still_runs():
    from pnec_amd.multi import alloc_counters
    from test_tracks_gpu import DELAY_MS, _delay, _same
    torch = _torch()
    frames = [_t(a) for a in store_fixture()["frames"][:4]]
    ref = _patches()
    for n in range(4):
        want = ref.process(frames[n])
    want = [getattr(want, k).clone() for k in RETAIN_KEYS] + [getattr(ref.tracks, k).clone() for k in SET_KEYS] + [ref.store.data.clone()]
    trk = _patches()
    for n in range(3):
        trk.process(frames[n])
    torch.cuda.synchronize()
    _delay(0)
    a0 = alloc_counters()
    S = torch.cuda.Stream()
    with torch.cuda.stream(S):
        _delay(DELAY_MS)
        gate = torch.cuda.Event()
        gate.record()
        t0 = time.perf_counter()
        r = trk.process(frames[3])
        host_ms = (time.perf_counter() - t0) * 1e3
        returned_early = not gate.query()
    S.synchronize()
    assert alloc_counters()["hip_malloc_calls"] == a0["hip_malloc_calls"], "a step allocated in the library"
    got = [getattr(r, k) for k in RETAIN_KEYS] + [getattr(trk.tracks, k) for k in SET_KEYS] + [trk.store.data]
    print(f"Tracker.process, stored patches: host side {host_ms:.3f} ms, returned_early={returned_early}")
    assert all(_same(x, y) for x, y in zip(got, want)), "the step on a side stream differs from the default stream's"
    assert returned_early, f"process returned only after the delay ({host_ms:.1f} ms): something waited"
