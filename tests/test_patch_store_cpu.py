"""CPU suite for the stored patches (pnec_hip_patch_store_slot_bytes, pnec_hip_patch_store_add, pnec_hip_patch_track_stored,
pnec_amd.PatchStore / add_patches / patch_track_stored, Tracker(templates="patches")): the slot rule of
include/pnec_hip.h in plain numpy -- assign_slots_np, held to hand-worked vectors --, the eight-frame fixture the GPU tests
share, the ABI (symbols, the slot size, refusals before a device is touched, the names exposed), the assignment kernel's
control flow replayed on the host under the sanitizers (tools/patch_store_host.cc), and the power of the fixture: a numpy
run of the frame loop without an age limit."""
import ctypes as C
import functools
import inspect
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import pnec_amd
from pnec_amd import capi, keyframes, patch_store, patches, tracker
from test_detect_keypoints_cpu import detect_np
from test_patch_covariance_cpu import patch_cov_np
from test_patch_track_cpu import H0, LEVELS, LOSTF, OK, W0, pyramid_levels_np
from test_tracks_cpu import (SEQ_CAPACITY, SEQ_EDGE, SEQ_F, SEQ_GRID, _warped, append_np, retain_np, track_indexed_np)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pnec_hip_patch_store_slot_bytes", "pnec_hip_patch_store_add", "pnec_hip_patch_track_stored")
STORE_FRAMES = 8


# ---- the slot rule in numpy -------------------------------------------------------------------------------------------
def assign_slots_np(slot, offsets, carried_offsets, capacity, strict=False):
    """pnec_hip_patch_store_add's assignment.  slot int32 [N] (the carried rows' entries are read), offsets [F+1],
    carried_offsets [F+1] or None -> the slot column after the call.  strict: HOST space, a carried slot that is not one of
    its image's raises."""
    slot = np.array(slot, dtype=np.int32)
    off = np.asarray(offsets, dtype=np.int64)
    F, C = len(off) - 1, int(capacity)
    for f in range(F):
        lo, c = int(off[f]), int(off[f + 1] - off[f])
        a = 0 if carried_offsets is None else max(0, int(carried_offsets[f + 1]) - int(carried_offsets[f]))
        take = min(a, c)
        occupied = set()
        for r in range(lo, lo + take):
            v = int(slot[r]) - f * C
            if 0 <= v < C:
                occupied.add(v)
            elif strict:
                raise ValueError(f"row {r}: slot {int(slot[r])} is not one of image {f}")
        free = [v for v in range(C) if v not in occupied]
        for i, r in enumerate(range(lo + take, lo + c)):
            slot[r] = f * C + free[i] if i < len(free) else -1
    slot[int(off[F]):] = -1
    return slot


def _vec(slots, counts, carried, capacity, rows=None):
    """(slot, offsets, carried_offsets) of a hand-written case: `slots` the column before the call"""
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    coff = None if carried is None else np.concatenate([[0], np.cumsum(carried)]).astype(np.int64)
    s = np.array(slots, dtype=np.int32)
    assert len(s) == (int(off[-1]) if rows is None else rows)
    return s, off, coff


X = 99   # what a new row or padding holds before the call: never read
# name -> (inputs of _vec, capacity, the column after the call), worked by hand
HAND = {
    "first frame": ((([X] * 5), (3, 2), None, 4), 4, [0, 1, 2, 4, 5]),
    "a hole in the middle reused": (([0, 1, 3, X], (4,), (3,), 4), 4, [0, 1, 3, 2]),
    "several holes taken in increasing order": (([8 + 6, 8 + 1, 8 + 4, X, X, X, X], (0, 7), (0, 3), 8), 8,
                                                [14, 9, 12, 8, 10, 11, 13]),
    "carried slot out of range": (([7, -1, 1, X, X], (5,), (3,), 4), 4, [7, -1, 1, 0, 2]),
    "an image over its capacity": (([2, X, X, X, X], (5,), (1,), 3), 3, [2, 0, 1, -1, -1]),
    "an empty image": (([1, X, X], (2, 0, 1), (1, 0, 0), 2), 2, [1, 0, 4]),
    "padding": (([1, X, X, X, X], (2, 1), (1, 0), 2, 5), 2, [1, 0, 2, -1, -1]),
    "more carried than rows": (([1, 0], (2,), (5,), 2), 2, [1, 0]),
}


def test_the_slot_rule_in_numpy_on_hand_worked_vectors():
    for name, (args, cap, want) in HAND.items():
        s, off, coff = _vec(*args)
        got = assign_slots_np(s, off, coff, cap)
        assert got.dtype == np.int32 and got.tolist() == want, (name, got.tolist(), want)
    s, off, coff = _vec(*HAND["carried slot out of range"][0])
    with pytest.raises(ValueError):
        assign_slots_np(s, off, coff, 4, strict=True)


# ---- the ABI ---------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_bound_and_exported_within_abi_8():
    L = capi.lib()
    header = open(os.path.join(ROOT, "include", "pnec_hip.h")).read()
    for name, n_args, ret in zip(NEW, (1, 20, 34), ("int64_t", "int", "int")):
        assert name in capi.SYMBOLS and getattr(L, name) is not None and len(getattr(L, name).argtypes) == n_args, name
        assert f"{ret} {name}(" in header
    assert capi.ABI_VERSION == 8 and L.pnec_hip_abi_version() == 8 and "#define PNEC_HIP_ABI_VERSION 8" in header
    assert len(L.pnec_hip_patch_track_indexed.argtypes) == 35
    plan = open(os.path.join(ROOT, "pnec_amd", "csrc", "pnec_capi.hip")).read()
    for name in NEW:
        assert name + "(" in plan
    for words in ("take_f = min(a_f, c_f)", "the i-th smallest free local slot", "PNEC_HIP_PATCH_STORE_MAX_CAPACITY 65536",
                  "bad at the top level", "DEVIATION"):
        assert words in header, words
    assert header.count("lifts it") >= 2


def test_slot_bytes_is_positive_and_aligned_for_1_to_8_levels_and_0_otherwise():
    L = capi.lib()
    sizes = [L.pnec_hip_patch_store_slot_bytes(n) for n in range(1, 9)]
    assert all(s > 0 and s % 8 == 0 for s in sizes) and all(b > a for a, b in zip(sizes, sizes[1:]))
    # what a level stores: 52 .. 64 values, three gain components each, the validity, a status
    assert all(s >= n * 64 * 4 * 8 for n, s in zip(range(1, 9), sizes))
    for n in (0, -1, 9, 2 ** 31 - 1, -2 ** 31):
        assert L.pnec_hip_patch_store_slot_bytes(n) == 0, n
    assert patch_store.slot_bytes(5) == sizes[4]


def _ptr(a):
    return None if a is None else a.ctypes.data


def test_bad_arguments_are_refused_before_a_device_is_touched():
    L = capi.lib()
    F, cap, n_levels = 2, 4, 3
    words = L.pnec_hip_patch_store_slot_bytes(n_levels) // 8
    pyr = [np.zeros((F, 96 >> l, 128 >> l), np.uint8) for l in range(n_levels)]
    ptrs = (C.c_void_p * n_levels)(*[a.ctypes.data for a in pyr])
    holed = (C.c_void_p * n_levels)(pyr[0].ctypes.data, None, pyr[2].ctypes.data)
    pitch = (C.c_int64 * n_levels)(128, 64, 32)
    short = (C.c_int64 * n_levels)(128, 63, 32)
    off, coff = np.array([0, 3, 5], np.int64), np.array([0, 2, 3], np.int64)
    pts = np.full((6, 2), 40.0)
    slot = np.array([1, 0, -5, 4, -5, -5], np.int32)
    store = np.full((F * cap, words), -5.0)
    slot0, store0 = slot.copy(), store.copy()
    pat = np.array(patches.PATTERN52)

    def add(**over):
        a = dict(cur=ptrs, pitch=pitch, levels=n_levels, ptype=0, F=F, h=96, w=128, coff=_ptr(coff), off=_ptr(off), N=6,
                 pts=_ptr(pts), slot=_ptr(slot), cap=cap, pat=_ptr(pat), n_pat=52, store=_ptr(store), n_slots=F * cap,
                 space=capi.MEM_HOST)
        a.update(over)
        rc = L.pnec_hip_patch_store_add(a["cur"], a["pitch"], a["levels"], a["ptype"], a["F"], a["h"], a["w"], a["coff"], a["off"],
                                        a["N"], a["pts"], a["slot"], a["cap"], a["pat"], a["n_pat"], a["store"], a["n_slots"],
                                        a["space"], 0, None)
        return rc, (L.pnec_hip_last_error() or b"").decode()

    bad_slot = slot.copy()
    bad_slot[3] = 3                                             # image 1's carried row with a slot of image 0
    for kw, word in ((dict(cur=None), "NULL"), (dict(pitch=None), "NULL"), (dict(off=None), "NULL"), (dict(pat=None), "NULL"),
                     (dict(store=None), "NULL"), (dict(pts=None), "NULL"), (dict(slot=None), "NULL"), (dict(cur=holed), "level pointer"),
                     (dict(levels=0), "n_levels"), (dict(levels=9), "n_levels"), (dict(n_pat=0), "n_pattern"), (dict(n_pat=65), "n_pattern"),
                     (dict(ptype=7), "pixel_type"), (dict(F=0), "n_images"), (dict(N=-1), "n_rows"), (dict(h=8), "smallest level"),
                     (dict(pitch=short), "pitch"), (dict(cap=0), "per_image_capacity"),
                     (dict(cap=65537, n_slots=2 ** 31 - 1), "PNEC_HIP_PATCH_STORE_MAX_CAPACITY"),
                     (dict(cap=65536, F=40000, n_slots=2 ** 31 - 1), "int32"), (dict(n_slots=F * cap - 1), "n_slots"),
                     (dict(n_slots=2 ** 31), "n_slots"), (dict(slot=_ptr(off)), "an output is an input"),
                     (dict(store=_ptr(pts)), "an output is an input"), (dict(store=_ptr(slot)), "an output is an input"),
                     (dict(space=5), "memory space"), (dict(off=_ptr(np.array([0, 3, 7], np.int64))), "offsets"),
                     (dict(off=_ptr(np.array([1, 3, 5], np.int64))), "offsets"), (dict(off=_ptr(np.array([0, 4, 3], np.int64))), "offsets"),
                     (dict(coff=_ptr(np.array([0, 2, 1], np.int64))), "carried_offsets"),
                     (dict(coff=_ptr(np.array([1, 2, 3], np.int64))), "carried_offsets"), (dict(slot=_ptr(bad_slot)), "carried row")):
        rc, msg = add(**kw)
        assert rc == capi.ERR_INVALID_ARGUMENT == -1 and "patch_store_add" in msg and word in msg, (kw, rc, msg)
    assert add(space=capi.MEM_DEVICE, cap=0)[0] == -1
    assert np.array_equal(slot, slot0) and np.array_equal(store, store0)

    nxt = (C.c_void_p * n_levels)(*[a[1:].ctypes.data for a in pyr])
    out_status = np.full(6, -5, np.int32)
    out_pts = np.full((6, 2), -5.0)
    good = np.array([1, 0, 2, 4, 5, -1], np.int32)               # (row 5 is padding: off[F] = 5)

    def stored(**over):
        a = dict(store=_ptr(store), n_slots=F * cap, prev=ptrs, prev_pitch=pitch, next=nxt, levels=n_levels, F=F, off=_ptr(off),
                 M=6, pts=_ptr(pts), slot=_ptr(good), iters=40, o_pts=_ptr(out_pts), o_status=_ptr(out_status), space=capi.MEM_HOST)
        a.update(over)
        rc = L.pnec_hip_patch_track_stored(a["store"], a["n_slots"], a["prev"], a["prev_pitch"], a["next"], pitch, a["levels"], 0,
                                           a["F"], 96, 128, a["off"], a["M"], a["pts"], a["slot"], None, None, 0.0, 0.0, _ptr(pat), 52,
                                           a["iters"], 0.04, 0, 10.0, a["o_pts"], None, None, None, a["o_status"], None, a["space"],
                                           0, None)
        return rc, (L.pnec_hip_last_error() or b"").decode()

    wild = good.copy()
    wild[2] = F * cap
    neg = good.copy()
    neg[4] = -1
    for kw, word in ((dict(store=None), "NULL"), (dict(slot=None), "NULL"), (dict(prev=None), "NULL"), (dict(prev_pitch=None), "NULL"),
                     (dict(n_slots=0), "n_slots"), (dict(n_slots=2 ** 31), "n_slots"), (dict(levels=9), "n_levels"), (dict(F=0), "n_images"),
                     (dict(iters=0), "max_iterations"), (dict(o_pts=None, o_status=None), "every output is NULL"),
                     (dict(o_pts=_ptr(store)), "an output is an input"), (dict(o_status=_ptr(good)), "an output is an input"),
                     (dict(space=5), "memory space"), (dict(off=_ptr(np.array([0, 3, 7], np.int64))), "offsets"),
                     (dict(slot=_ptr(wild)), "outside 0 .. n_slots - 1"), (dict(slot=_ptr(neg)), "outside 0 .. n_slots - 1")):
        rc, msg = stored(**kw)
        assert rc == -1 and "patch_track_stored" in msg and word in msg, (kw, rc, msg)
    assert np.all(out_status == -5) and np.all(out_pts == -5.0) and np.array_equal(store, store0)


def test_python_names_signatures_and_defaults():
    import dataclasses
    assert {"PatchStore", "new_patch_store", "add_patches", "patch_track_stored"} <= set(pnec_amd.__all__)
    assert pnec_amd.add_patches is patch_store.add_patches and pnec_amd.PatchStore is patch_store.PatchStore
    assert [f.name for f in dataclasses.fields(pnec_amd.PatchStore)] == ["data", "n_levels", "per_image_capacity"]
    sig = inspect.signature(pnec_amd.new_patch_store)
    assert list(sig.parameters) == ["n_images", "per_image_capacity", "n_levels", "device"] and sig.parameters["device"].default is None
    sig = inspect.signature(pnec_amd.add_patches)
    assert list(sig.parameters) == ["store", "pyramid", "tracks", "carried_offsets", "pattern"]
    assert sig.parameters["carried_offsets"].default is None and sig.parameters["pattern"].default is patches.PATTERN52
    sig = inspect.signature(pnec_amd.patch_track_stored)
    assert list(sig.parameters)[:4] == ["store", "prev", "next", "tracks_or_arrays"]
    ref = inspect.signature(patches.patch_track).parameters
    for k in ("shift", "max_iterations", "max_recovered_dist2", "backward", "scaling", "outputs"):
        assert sig.parameters[k].default == ref[k].default, k
    params = inspect.signature(tracker.Tracker.__init__).parameters
    assert list(params)[-1] == "templates" and params["templates"].default == "ring" and params["ring"].default == 4
    # a host store: what the HOST-space calls take
    st = pnec_amd.new_patch_store(2, 3, 5, device="cpu")
    assert isinstance(st.data, np.ndarray) and st.data.shape == (6, patch_store.slot_bytes(5)) and st.n_slots == 6
    assert st.data.dtype == np.uint8 and not st.data.any() and st.n_levels == 5 and st.per_image_capacity == 3
    for bad in (dict(n_images=0), dict(per_image_capacity=0), dict(n_levels=9), dict(n_images=2 ** 20, per_image_capacity=2 ** 12)):
        with pytest.raises(ValueError):
            pnec_amd.new_patch_store(**dict(dict(n_images=1, per_image_capacity=1, n_levels=1, device="cpu"), **bad))


def _past_validation(make):
    """the constructor does not refuse its arguments (without a device it fails later, on the first allocation)"""
    try:
        make()
    except ValueError as e:
        raise AssertionError(f"refused: {e}")
    except Exception:
        pass


def test_the_ring_rules_stay_and_the_patches_rules_are_the_new_ones():
    with pytest.raises(ValueError):
        pnec_amd.Tracker(1, 96, 128, ring=2)
    with pytest.raises(ValueError):
        pnec_amd.Tracker(1, 96, 128, ring=2, templates="ring")
    with pytest.raises(ValueError):
        pnec_amd.Tracker(1, 96, 128, ring=1, templates="patches")
    with pytest.raises(ValueError):
        pnec_amd.Tracker(1, 96, 128, templates="pyramids")
    _past_validation(lambda: pnec_amd.Tracker(1, 96, 128, ring=2, templates="patches"))
    # KeyframeTracker: the ring's refusals as they were ...
    for kw in (dict(ring=3), dict(ring=4, max_span=3), dict(max_span=0), dict(ring=5, max_span=4), dict(ring=2),
               dict(ring=3, templates="ring")):
        with pytest.raises(ValueError):
            pnec_amd.KeyframeTracker(1, 96, 128, **kw)
    # ... and none of them with stored patches, but max_span >= 1 and the displacement's
    for kw in (dict(max_span=0), dict(max_span=-3), dict(max_span=2 ** 31), dict(min_displacement=-1.0), dict(ring=1)):
        with pytest.raises(ValueError):
            pnec_amd.KeyframeTracker(1, 96, 128, templates="patches", **kw)
    for kw in (dict(ring=2), dict(ring=2, max_span=100), dict(ring=3, max_span=1), dict(max_span=None)):
        _past_validation(lambda: pnec_amd.KeyframeTracker(1, 96, 128, templates="patches", **kw))
    src = inspect.getsource(keyframes.KeyframeTracker.__init__)
    assert "2 ** 31 - 1" in src
    _past_validation(lambda: pnec_amd.Odometry(1, 96, 128, np.eye(3), min_displacement=4.0, ring=2, max_span=9, templates="patches"))


# ---- the assignment's control flow on the host, under the sanitizers --------------------------------------------------
@functools.lru_cache(maxsize=None)
def _host_program():
    gxx = shutil.which("g++")
    assert gxx, "g++ builds the host facade, so it is there"
    exe = os.path.join(tempfile.mkdtemp(prefix="patch_store_host_"), "patch_store_host")
    subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "pnec_amd", "csrc"),
                    os.path.join(ROOT, "tools", "patch_store_host.cc"), "-o", exe], check=True)
    return exe


ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


def run_host_assign(tmp_path, slot, off, coff, cap):
    head = np.array([len(off) - 1, cap, len(slot), 0 if coff is None else 1], np.int64)
    blob = [head.tobytes()] + ([] if coff is None else [np.asarray(coff, np.int64).tobytes()]) + \
        [np.asarray(off, np.int64).tobytes(), np.asarray(slot, np.int32).tobytes()]
    (tmp_path / "job.bin").write_bytes(b"".join(blob))
    r = subprocess.run([_host_program(), str(tmp_path / "job.bin"), str(tmp_path / "out.bin")], env=ENV, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "without slack" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    return np.frombuffer((tmp_path / "out.bin").read_bytes(), dtype=np.int32).copy()


def count_cases():
    """the wavefront and block boundaries as row counts, against capacities below, at and above them -> (name, slot, off,
    coff, cap)"""
    rng = np.random.default_rng(17)
    counts = (0, 1, 63, 64, 65, 257)
    cases = []
    for cap in (64, 257, 300, 8193, 65536):
        F = len(counts)
        carried = [int(rng.integers(0, c + 1)) for c in counts]
        carried[3] = 64                                          # an image whose rows are all carried
        off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        coff = np.concatenate([[0], np.cumsum(carried)]).astype(np.int64)
        slot = np.full(int(off[-1]) + 37, 12345, np.int32)       # 37 rows of padding
        for f in range(F):
            take = min(carried[f], counts[f])
            local = rng.permutation(cap)[:take] if take <= cap else rng.integers(0, cap, take)
            slot[off[f]:off[f] + take] = f * cap + local
        slot[off[2] + 1] = -7                                    # carried slots that are not the image's
        slot[off[5]] = 0 if carried[5] else slot[off[5]]
        cases.append((f"capacity {cap}", slot, off, coff, cap))
    cases.append(("first frame, capacity 65536", np.full(450, 5, np.int32), off, None, 65536))
    return cases


def test_the_assignment_built_for_the_host_reads_nothing_outside_and_equals_numpy(tmp_path):
    for name, (args, cap, want) in HAND.items():
        s, off, coff = _vec(*args)
        got = run_host_assign(tmp_path, s, off, coff, cap)
        assert got.tolist() == want, (name, got.tolist(), want)
    for name, slot, off, coff, cap in count_cases():
        got = run_host_assign(tmp_path, slot, off, coff, cap)
        want = assign_slots_np(slot, off, coff, cap)
        assert np.array_equal(got, want), (name, np.flatnonzero(got != want)[:10])
        live = want[:off[-1]]
        assert np.all(want[off[-1]:] == -1)
        if name == "capacity 64":
            assert np.any(live == -1) and np.any(np.diff(off) > cap)   # (an image over its capacity)
        else:
            new = np.concatenate([np.arange(off[f] + min(coff[f + 1] - coff[f], off[f + 1] - off[f]) if coff is not None else off[f],
                                            off[f + 1]) for f in range(len(off) - 1)])
            assert np.all(want[new] >= 0) and len(set(want[new].tolist())) == len(new)


# ---- the fixture and the frame loop without an age limit in numpy -----------------------------------------------------
@functools.lru_cache(maxsize=None)
def store_fixture():
    """-> dict frames [8][3,96,128] uint8: three sequences of eight frames of the `analytic` texture, each frame the previous
    one moved by test_tracks_cpu's warp, nothing blanked; pyr [8]: their pyramids (pyramid_levels_np)."""
    frames = [np.round(np.stack([_warped(300 + f, n) for f in range(SEQ_F)])).astype(np.uint8) for n in range(STORE_FRAMES)]
    for a in frames:
        a.setflags(write=False)
    return dict(frames=frames, pyr=[pyramid_levels_np(a, LEVELS) for a in frames])


def carried_slots(prev_slot, retained, out_offsets, n_out, capacity):
    """the slot column append leaves behind: per image the retained rows' slots (of the rows they came from), then
    whatever (here 0) for the rows patch_store_add assigns"""
    col = np.zeros(n_out, np.int32)
    if retained is None:
        return col
    roff = retained["offsets"]
    for f in range(len(roff) - 1):
        take = min(int(roff[f + 1] - roff[f]), capacity)
        col[out_offsets[f]:out_offsets[f] + take] = prev_slot[retained["src"][roff[f]:roff[f] + take]]
    return col


@functools.lru_cache(maxsize=None)
def store_reference():
    """The eight steps in numpy, a track's template taken from the frame it was born in for as long as it lives
    (track_indexed_np on a stack of all frames, retain_np without an age limit), and the slot column assign_slots_np gives.
    -> list of dict trk (None at 0), retained (None), out, slot, dropped"""
    fx = store_fixture()
    F, cap, N = SEQ_F, SEQ_CAPACITY, SEQ_F * SEQ_CAPACITY
    stack = [np.concatenate([fx["pyr"][m][l] for m in range(STORE_FRAMES)]) for l in range(LEVELS)]
    steps, s, slot, nid = [], None, None, np.zeros(F, np.int64)
    for n in range(STORE_FRAMES):
        cur = fx["pyr"][n]
        trk = retained = None
        if n > 0:
            trk = track_indexed_np(stack, fx["pyr"][n - 1], cur, s, F)
            retained = retain_np(s, trk, max_age=0)
        det = detect_np(cur[0], SEQ_GRID, 1, 5, SEQ_EDGE, current=None if retained is None else (retained["offsets"], retained["pts"]))
        det_cov = patch_cov_np(cur[0], det["pts"], det["offsets"])["cov"]
        s, nid, dropped = append_np(retained, det["offsets"], det["pts"], det_cov, n * F, cap, nid, N)
        slot = assign_slots_np(carried_slots(slot, retained, s["offsets"], N, cap), s["offsets"],
                               None if retained is None else retained["offsets"], cap, strict=True)
        steps.append(dict(trk=trk, retained=retained, out=s, slot=slot, dropped=dropped))
    return steps


def test_the_fixture_has_the_power_the_gpu_test_relies_on():
    steps = store_reference()
    assert (H0, W0) == (96, 128) and len(steps) == STORE_FRAMES == 8
    last = steps[-1]["retained"]
    ages = [int(last["age"][last["offsets"][f]:last["offsets"][f + 1]].max()) for f in range(SEQ_F)]
    assert ages == [6, 7, 7], ages
    lost_at = set()
    reused = moved = at_capacity = seven_rows = False
    for n, st in enumerate(steps):
        o, off = st["out"], st["out"]["offsets"]
        counts = np.diff(off)
        at_capacity |= bool(np.any((counts == SEQ_CAPACITY) & (st["dropped"] > 0)))
        seven_rows |= n == 6 and bool(np.any(counts == 7))
        live = np.arange(len(o["id"])) < off[-1]
        assert np.all(st["slot"][~live] == -1) and np.all(st["slot"][live] >= 0)
        for f in range(SEQ_F):
            rows = st["slot"][off[f]:off[f + 1]]
            assert len(set(rows.tolist())) == len(rows) and np.all(rows // SEQ_CAPACITY == f)
            moved |= bool(np.any(rows - f * SEQ_CAPACITY != np.arange(len(rows))))
        if n == 0:
            continue
        prev = steps[n - 1]
        plive = np.arange(len(prev["out"]["id"])) < prev["out"]["offsets"][-1]
        if np.any(st["trk"]["status"][plive] == LOSTF):
            lost_at.add(n)
        # a slot freed by a loss at this step and given to a track born at this step
        freed = set(prev["slot"][plive & (st["trk"]["status"] != OK)].tolist())
        reused |= bool(freed & set(st["slot"][live & (o["age"] == 0)].tolist()))
    assert {5, 6, 7} <= lost_at, lost_at
    assert reused and moved and at_capacity and seven_rows
