"""CPU suite for the tracks across frames (pnec_hip_tracks_retain, pnec_hip_tracks_append, pnec_hip_patch_track_indexed,
pnec_amd.Tracker): the definitions of include/pnec_hip.h in plain numpy -- retain_np, append_np, tracker_step_np, written
from the definitions and never calling the code under test --, the synthetic cases and the sequence fixture the GPU tests
share, the ABI (symbols, refusals before a device is touched, the names exposed), the kernels' control flow replayed on
the host under the sanitizers (tools/tracks_host.cc), and the power of the sequence fixture."""
import ctypes as C
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import pnec_amd
from pnec_amd import capi, patches, tracker
from test_detect_keypoints_cpu import detect_np
from test_patch_covariance_cpu import patch_cov_np
from test_patch_track_cpu import (BAD, FAR, H0, LEVELS, LOSTB, LOSTF, OK, W0, analytic, patch_track_np,
                                  pyramid_levels_np)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SET_KEYS = ("offsets", "id", "tmpl_image", "tmpl_pts", "age", "pts", "angle", "cov")
RETAIN_KEYS = SET_KEYS + ("prev_pts", "prev_cov", "src")
NAN = float("nan")


# ---- the definitions in numpy ----------------------------------------------------------------------------------------
def padded_set_np(F, N, cov=True):
    """a set of N rows that is all padding"""
    s = dict(offsets=np.zeros(F + 1, np.int64), id=np.full(N, -1, np.int64), tmpl_image=np.zeros(N, np.int32),
             tmpl_pts=np.full((N, 2), NAN), age=np.zeros(N, np.int32), pts=np.full((N, 2), NAN), angle=np.full(N, NAN),
             cov=np.full((N, 3), NAN) if cov else None)
    return s


def retain_np(s, trk, max_age=0, with_cov=True, with_prev_pts=True, with_src=True):
    """pnec_hip_tracks_retain.  s: a set (dict of SET_KEYS), trk: dict pts, angle, cov, status for its rows."""
    off = np.asarray(s["offsets"])
    F, N = len(off) - 1, len(s["id"])
    out = padded_set_np(F, N, with_cov)
    out["prev_pts"] = np.full((N, 2), NAN) if with_prev_pts else None
    out["prev_cov"] = np.full((N, 3), NAN) if with_cov else None
    out["src"] = np.full(N, -1, np.int64) if with_src else None
    at = 0
    for f in range(F):
        for k in range(int(off[f]), int(off[f + 1])):
            if not (s["id"][k] >= 0 and trk["status"][k] == OK and (max_age == 0 or int(s["age"][k]) + 1 <= max_age)):
                continue
            out["id"][at], out["tmpl_image"][at], out["tmpl_pts"][at] = s["id"][k], s["tmpl_image"][k], s["tmpl_pts"][k]
            out["age"][at] = min(int(s["age"][k]) + 1, 2 ** 31 - 1)
            out["pts"][at], out["angle"][at] = trk["pts"][k], trk["angle"][k]
            if with_cov:
                out["cov"][at], out["prev_cov"][at] = trk["cov"][k], s["cov"][k]
            if with_prev_pts:
                out["prev_pts"][at] = s["pts"][k]
            if with_src:
                out["src"][at] = k
            at += 1
        out["offsets"][f + 1] = at
    return out


def append_np(s, det_offsets, det_pts, det_cov, base, capacity, next_id, n_out, with_cov=True):
    """pnec_hip_tracks_append.  s: a set or None.  -> (set of n_out rows, next_id after, dropped)"""
    doff = np.asarray(det_offsets)
    F = len(doff) - 1
    out = padded_set_np(F, n_out, with_cov)
    next_id, dropped = np.array(next_id, dtype=np.int64), np.zeros(F, np.int64)
    at = 0
    for f in range(F):
        lo = 0 if s is None else int(s["offsets"][f])
        a = 0 if s is None else int(s["offsets"][f + 1]) - lo
        d = int(doff[f + 1]) - int(doff[f])
        take_a = min(a, capacity)
        take_d = min(d, capacity - take_a)
        for k in range(lo, lo + take_a):
            for key in ("id", "tmpl_image", "tmpl_pts", "age", "pts", "angle"):
                out[key][at] = s[key][k]
            if with_cov:
                out["cov"][at] = s["cov"][k] if s["cov"] is not None else NAN
            at += 1
        for r in range(take_d):
            k = int(doff[f]) + r
            out["id"][at], out["tmpl_image"][at], out["age"][at], out["angle"][at] = next_id[f] + r, base + f, 0, 0.0
            out["tmpl_pts"][at] = out["pts"][at] = det_pts[k]
            if with_cov:
                out["cov"][at] = det_cov[k] if det_cov is not None else NAN
            at += 1
        next_id[f] += take_d
        dropped[f] = (a - take_a) + (d - take_d)
        out["offsets"][f + 1] = at
    assert at <= n_out, "the case gives too few rows"
    return out, next_id, dropped


def assert_same(got, ref, keys, what):
    """every array equal to numpy's, exactly, padding included, to the last row; NaN where numpy has NaN"""
    for k in keys:
        a, b = got[k], ref[k]
        if b is None:
            assert a is None, (what, k)
            continue
        a = np.asarray(a)
        assert a.shape == b.shape and a.dtype == b.dtype, (what, k, a.shape, b.shape, a.dtype, b.dtype)
        assert np.array_equal(a, b, equal_nan=b.dtype.kind == "f"), \
            (what, k, np.flatnonzero(~((a == b) | ((a != a) & (b != b))).reshape(len(a), -1).all(1))[:10])


# ---- the synthetic cases the GPU tests and the host replay share -----------------------------------------------------
COUNTS = (0, 1, 63, 64, 65, 257)      # the wavefront (64) and block (256) boundaries, an empty image


def random_set(rng, counts, slack=0, id0=0, cov=True):
    """a set with `counts` rows per image and `slack` rows beyond offsets[F] that hold live-looking values (not padding:
    the rule k < offsets[F] must be what keeps them out)"""
    N = int(sum(counts)) + slack
    s = dict(offsets=np.concatenate([[0], np.cumsum(counts)]).astype(np.int64),
             id=(id0 + rng.permutation(N)).astype(np.int64), tmpl_image=rng.integers(0, 9, N).astype(np.int32),
             tmpl_pts=rng.uniform(0, 100, (N, 2)), age=rng.integers(0, 3, N).astype(np.int32), pts=rng.uniform(0, 100, (N, 2)),
             angle=rng.uniform(-1, 1, N), cov=rng.uniform(0, 1, (N, 3)) if cov else None)
    return s


def random_trk(rng, N, p_ok=0.6):
    status = np.where(rng.uniform(size=N) < p_ok, OK, rng.integers(1, 5, N)).astype(np.int32)
    return dict(pts=rng.uniform(0, 100, (N, 2)), angle=rng.uniform(-1, 1, N), cov=rng.uniform(0, 1, (N, 3)), status=status)


@functools.lru_cache(maxsize=None)
def retain_cases():
    """-> list of (name, dict(s, trk, max_age, with_cov, with_prev_pts, with_src))"""
    rng = np.random.default_rng(11)
    N = sum(COUNTS)
    base = dict(max_age=0, with_cov=True, with_prev_pts=True, with_src=True)
    cases = [("random statuses", dict(base, s=random_set(rng, COUNTS), trk=random_trk(rng, N))),
             ("all retained", dict(base, s=random_set(rng, COUNTS), trk=random_trk(rng, N, 1.0))),
             ("none retained", dict(base, s=random_set(rng, COUNTS), trk=random_trk(rng, N, 0.0)))]
    s = random_set(rng, COUNTS)
    s["id"][rng.uniform(size=N) < 0.3] = -1
    s["id"][[1, 64, 65, 128, 129, N - 1]] = (-1, -2, -1, -(2 ** 40), -1, -1)
    cases.append(("negative ids inside the ranges", dict(base, s=s, trk=random_trk(rng, N, 0.9))))
    s = random_set(rng, COUNTS)
    s["age"][[0, 5, 70]] = 2 ** 31 - 1
    cases.append(("max_age 0 and a saturated age", dict(base, s=s, trk=random_trk(rng, N, 0.9))))
    cases.append(("max_age 1", dict(base, s=random_set(rng, COUNTS), trk=random_trk(rng, N, 0.9), max_age=1)))
    cases.append(("optional arrays NULL", dict(s=random_set(rng, COUNTS, cov=False), trk=random_trk(rng, N), max_age=0,
                                               with_cov=False, with_prev_pts=False, with_src=False)))
    cases.append(("ids from 2^40, rows beyond offsets[F]",
                  dict(base, s=random_set(rng, COUNTS, slack=131, id0=2 ** 40), trk=random_trk(rng, N + 131, 0.8))))
    cases.append(("one image, one row", dict(base, s=random_set(rng, (1,)), trk=random_trk(rng, 1, 1.0))))
    cases.append(("no rows at all", dict(base, s=random_set(rng, (0, 0)), trk=random_trk(rng, 0))))
    return cases


def retain_reference(kw):
    return retain_np(kw["s"], kw["trk"], kw["max_age"], kw["with_cov"], kw["with_prev_pts"], kw["with_src"])


DET_COUNTS = (5, 0, 9, 70, 4, 300)


def random_det(rng, counts, slack=0, cov=True):
    D = int(sum(counts)) + slack
    return dict(offsets=np.concatenate([[0], np.cumsum(counts)]).astype(np.int64),
                pts=np.floor(rng.uniform(0, 100, (D, 2))), cov=rng.uniform(0, 1, (D, 3)) if cov else None)


@functools.lru_cache(maxsize=None)
def append_cases():
    """-> list of (name, dict(s, det, base, capacity, next_id, n_out, with_cov)).  With a = COUNTS and d = DET_COUNTS a
    capacity of 60 is below a in four images, 66 lies between a and a + d in three and above a + d in others, 1000 is above
    everything."""
    rng = np.random.default_rng(12)
    F = len(COUNTS)
    ids = np.arange(100, 100 + F, dtype=np.int64) * 1000
    full = lambda s, det: (0 if s is None else len(s["id"])) + len(det["pts"])
    cases = []
    for cap in (60, 66, 1000):
        s, det = random_set(rng, COUNTS), random_det(rng, DET_COUNTS)
        cases.append((f"capacity {cap}", dict(s=s, det=det, base=12, capacity=cap, next_id=ids, n_out=min(F * cap, full(s, det)),
                                               with_cov=True)))
    det = random_det(rng, DET_COUNTS)
    cases.append(("no input set", dict(s=None, det=det, base=0, capacity=64, next_id=np.zeros(F, np.int64),
                                       n_out=min(F * 64, full(None, det)), with_cov=True)))
    s, det = random_set(rng, COUNTS, id0=2 ** 40), random_det(rng, DET_COUNTS)
    cases.append(("ids from 2^40, int32 edge of tmpl_image", dict(s=s, det=det, base=2 ** 31 - F, capacity=300,
                                                                 next_id=2 ** 40 + ids, n_out=full(s, det), with_cov=True)))
    s, det = random_set(rng, COUNTS, slack=77), random_det(rng, DET_COUNTS, slack=55)
    cases.append(("rows beyond offsets[F] in both inputs, padding in the output",
                  dict(s=s, det=det, base=3, capacity=100, next_id=ids, n_out=F * 100, with_cov=True)))
    s, det = random_set(rng, COUNTS, cov=False), random_det(rng, DET_COUNTS, cov=False)
    cases.append(("no covariances", dict(s=s, det=det, base=3, capacity=70, next_id=ids, n_out=F * 70, with_cov=False)))
    s, det = random_set(rng, COUNTS, cov=False), random_det(rng, DET_COUNTS)
    cases.append(("set without cov, detections with", dict(s=s, det=det, base=3, capacity=70, next_id=ids, n_out=F * 70,
                                                          with_cov=True)))
    s, det = random_set(rng, (3,)), random_det(rng, (0,))
    cases.append(("one image, no detection, capacity 1", dict(s=s, det=det, base=0, capacity=1, next_id=np.array([7], np.int64),
                                                             n_out=1, with_cov=True)))
    return cases


def append_reference(kw):
    det = kw["det"]
    return append_np(kw["s"], det["offsets"], det["pts"], det["cov"], kw["base"], kw["capacity"], kw["next_id"], kw["n_out"],
                     kw["with_cov"])


def test_the_synthetic_cases_cover_what_they_claim():
    names = [n for n, _ in retain_cases()]
    refs = {n: retain_reference(kw) for n, kw in retain_cases()}
    first = retain_cases()[0][1]
    assert tuple(np.diff(first["s"]["offsets"])) == (0, 1, 63, 64, 65, 257)
    kept = np.diff(refs["random statuses"]["offsets"])
    assert 0 < kept[-1] < 257 and set(first["trk"]["status"]) == {0, 1, 2, 3, 4}
    assert np.array_equal(np.diff(refs["all retained"]["offsets"]), COUNTS) and refs["none retained"]["offsets"][-1] == 0
    assert np.all(refs["none retained"]["id"] == -1) and np.all(np.isnan(refs["none retained"]["pts"]))
    neg = dict(retain_cases())["negative ids inside the ranges"]
    assert np.any((neg["s"]["id"] < 0) & (neg["trk"]["status"] == OK))
    sat = refs["max_age 0 and a saturated age"]
    assert np.any(sat["age"] == 2 ** 31 - 1) and np.all(sat["age"] >= 0)
    one = dict(retain_cases())["max_age 1"]
    assert np.any((one["s"]["age"] >= 1) & (one["trk"]["status"] == OK) & (one["s"]["id"] >= 0)) and \
        set(refs["max_age 1"]["age"][:refs["max_age 1"]["offsets"][-1]]) == {1}
    far = dict(retain_cases())["ids from 2^40, rows beyond offsets[F]"]
    assert np.any(far["trk"]["status"][far["s"]["offsets"][-1]:] == OK) and refs[names[7]]["id"].max() >= 2 ** 40
    taken = {}
    for name, kw in append_cases():
        out, nid, dropped = append_reference(kw)
        a = np.diff(kw["s"]["offsets"]) if kw["s"] is not None else np.zeros(len(nid), np.int64)
        d, c = np.diff(kw["det"]["offsets"]), kw["capacity"]
        taken[name] = (int(np.sum(c < a)), int(np.sum((a <= c) & (c < a + d))), int(np.sum(c >= a + d)), int(dropped.sum()),
                       int(kw["n_out"] - out["offsets"][-1]))
    assert taken["capacity 60"][0] == 4 and taken["capacity 66"][1] >= 2 and taken["capacity 1000"][:2] == (0, 0)
    assert taken["capacity 60"][3] > 0 and taken["capacity 1000"][3] == 0
    assert taken["rows beyond offsets[F] in both inputs, padding in the output"][4] > 0
    assert append_reference(dict(append_cases())["ids from 2^40, int32 edge of tmpl_image"])[0]["tmpl_image"].max() == 2 ** 31 - 1


# ---- the ABI ---------------------------------------------------------------------------------------------------------
NEW = ("pnec_hip_tracks_retain", "pnec_hip_tracks_append", "pnec_hip_patch_track_indexed")


def test_symbols_are_declared_bound_and_exported_within_abi_8():
    L = capi.lib()
    header = open(os.path.join(ROOT, "include", "pnec_hip.h")).read()
    for name, n_args in zip(NEW, (28, 30, 35)):
        assert name in capi.SYMBOLS and getattr(L, name) is not None and len(getattr(L, name).argtypes) == n_args, name
        assert f"int {name}(" in header
    assert capi.ABI_VERSION == 8 and L.pnec_hip_abi_version() == 8 and "#define PNEC_HIP_ABI_VERSION 8" in header
    assert len(L.pnec_hip_patch_track.argtypes) == 33
    for words in ("k < offsets[n_images], id[k] >= 0", "age + 1, saturating", "take_a = min(a, C)", "DEVIATION",
                  "the index is clamped to\n * [0, n_tmpl_images - 1]"):
        assert words in header, words


def _ptr(a):
    return None if a is None else a.ctypes.data


def call_retain(L, s, trk, age_limit, out, space=capi.MEM_HOST, **over):
    a = dict(F=len(s["offsets"]) - 1, offsets=_ptr(s["offsets"]), N=len(s["id"]), id=_ptr(s["id"]), tmpl_image=_ptr(s["tmpl_image"]),
             tmpl_pts=_ptr(s["tmpl_pts"]), age=_ptr(s["age"]), pts=_ptr(s["pts"]), cov=_ptr(s["cov"]), trk_pts=_ptr(trk["pts"]),
             trk_angle=_ptr(trk["angle"]), trk_cov=_ptr(trk["cov"]), trk_status=_ptr(trk["status"]), max_age=age_limit,
             **{"out_" + k: _ptr(out[k]) for k in RETAIN_KEYS})
    a.update(over)
    rc = L.pnec_hip_tracks_retain(a["F"], a["offsets"], a["N"], a["id"], a["tmpl_image"], a["tmpl_pts"], a["age"], a["pts"],
                                  a["cov"], a["trk_pts"], a["trk_angle"], a["trk_cov"], a["trk_status"], a["max_age"],
                                  *[a["out_" + k] for k in RETAIN_KEYS], space, 0, None)
    return rc, (L.pnec_hip_last_error() or b"").decode()


def call_append(L, s, det, base0, cap0, next_id0, rows, out, dropped0, space=capi.MEM_HOST, **over):
    none = dict.fromkeys(SET_KEYS)
    s = none if s is None else s
    a = dict(F=len(det["offsets"]) - 1, N=0 if s["id"] is None else len(s["id"]), det_offsets=_ptr(det["offsets"]),
             D=len(det["pts"]), det_pts=_ptr(det["pts"]), det_cov=_ptr(det["cov"]), base=base0, cap=cap0, next_id=_ptr(next_id0),
             n_out=rows, dropped=_ptr(dropped0), **{k: _ptr(s[k]) for k in SET_KEYS}, **{"out_" + k: _ptr(out[k]) for k in SET_KEYS})
    a.update(over)
    rc = L.pnec_hip_tracks_append(a["F"], a["offsets"], a["N"], a["id"], a["tmpl_image"], a["tmpl_pts"], a["age"], a["pts"],
                                  a["angle"], a["cov"], a["det_offsets"], a["D"], a["det_pts"], a["det_cov"], a["base"], a["cap"],
                                  a["next_id"], a["n_out"], *[a["out_" + k] for k in SET_KEYS], a["dropped"], space, 0, None)
    return rc, (L.pnec_hip_last_error() or b"").decode()


def test_bad_arguments_are_refused_before_a_device_is_touched():
    L = capi.lib()
    rng = np.random.default_rng(3)
    s, trk = random_set(rng, (2, 3)), random_trk(rng, 5)
    out = retain_np(s, trk)
    for k in RETAIN_KEYS:
        out[k][...] = -5
    bad_off = [np.array(o, dtype=np.int64) for o in ((0, 3, 2), (1, 2, 5), (0, 2, 6))]
    for kw, word in ((dict(F=0), "n_images"), (dict(N=-1), "n_rows"), (dict(offsets=None), "NULL"), (dict(out_offsets=None), "NULL"),
                     (dict(id=None), "NULL"), (dict(tmpl_image=None), "NULL"), (dict(tmpl_pts=None), "NULL"), (dict(age=None), "NULL"),
                     (dict(pts=None), "NULL"), (dict(trk_pts=None), "NULL"), (dict(trk_angle=None), "NULL"),
                     (dict(trk_status=None), "NULL"), (dict(out_id=None), "NULL"), (dict(out_tmpl_image=None), "NULL"),
                     (dict(out_tmpl_pts=None), "NULL"), (dict(out_age=None), "NULL"), (dict(out_pts=None), "NULL"),
                     (dict(out_angle=None), "NULL"), (dict(cov=None), "together"), (dict(trk_cov=None), "together"),
                     (dict(out_cov=None), "together"), (dict(out_prev_cov=None), "together"), (dict(max_age=-1), "max_age"),
                     (dict(out_pts=_ptr(trk["pts"])), "an output is an input"), (dict(out_id=_ptr(s["id"])), "an output is an input"),
                     (dict(space=5), "memory space")) + tuple((dict(offsets=_ptr(o)), "offsets") for o in bad_off):
        rc, msg = call_retain(L, s, trk, 0, out, **kw)
        assert rc == capi.ERR_INVALID_ARGUMENT == -1 and "tracks_retain" in msg and word in msg, (kw, rc, msg)
    assert call_retain(L, s, trk, 0, out, space=capi.MEM_DEVICE, max_age=-1)[0] == -1
    assert all(np.all(out[k] == -5) for k in RETAIN_KEYS)

    det = random_det(rng, (4, 1))
    nid, dropped = np.array([10, 20], np.int64), np.full(2, -5, np.int64)
    ref, _, _ = append_np(s, det["offsets"], det["pts"], det["cov"], 0, 8, nid, 10)
    for k in SET_KEYS:
        ref[k][...] = -5
    for kw, word in ((dict(F=0), "n_images"), (dict(N=-1), "n_rows"), (dict(D=-1), "n_det"), (dict(n_out=-1), "n_out"),
                     (dict(offsets=None), "no set"), (dict(id=None), "NULL"), (dict(angle=None), "NULL"), (dict(pts=None), "NULL"),
                     (dict(det_offsets=None), "NULL"), (dict(det_pts=None), "NULL"), (dict(next_id=None), "NULL"),
                     (dict(out_offsets=None), "NULL"), (dict(out_id=None), "NULL"), (dict(out_angle=None), "NULL"),
                     (dict(cap=0), "per_image_capacity"), (dict(base=-1), "tmpl_image_base"), (dict(base=2 ** 31 - 1), "tmpl_image_base"),
                     (dict(n_out=9), "n_out"), (dict(cap=4, n_out=7), "n_out"), (dict(out_pts=_ptr(det["pts"])), "an output is an input"),
                     (dict(next_id=_ptr(s["id"])), "an output is an input"), (dict(space=5), "memory space"),
                     (dict(det_offsets=_ptr(np.array([0, 5, 4], np.int64))), "det_offsets"),
                     (dict(det_offsets=_ptr(np.array([0, 4, 6], np.int64))), "det_offsets")) + \
            tuple((dict(offsets=_ptr(o)), "offsets") for o in bad_off):
        rc, msg = call_append(L, s, det, 0, 8, nid, 10, ref, dropped, **kw)
        assert rc == capi.ERR_INVALID_ARGUMENT == -1 and "tracks_append" in msg and word in msg, (kw, rc, msg)
    # (a capacity near 2^63 does not overflow the bound)
    rc, msg = call_append(L, s, det, 0, 2 ** 62, nid, 9, ref, dropped)
    assert rc == -1 and "n_out" in msg
    assert all(np.all(ref[k] == -5) for k in SET_KEYS) and np.all(dropped == -5) and tuple(nid) == (10, 20)

    # the indexed tracker: its own refusals, and pnec_hip_patch_track's under its name
    pyr = [np.zeros((4, 96 >> l, 128 >> l), np.uint8) for l in range(3)]
    ptrs = (C.c_void_p * 3)(*[a.ctypes.data for a in pyr])
    half = (C.c_void_p * 3)(*[a[2:].ctypes.data for a in pyr])
    pitch = (C.c_int64 * 3)(128, 64, 32)
    pts, ti = np.full((3, 2), 40.0), np.array([0, 3, 1], np.int32)
    off = np.array([0, 1, 3], np.int64)
    o_st = np.full(3, -5, np.int32)

    def indexed(n_tmpl=4, prev=half, tmpl_image=ti.ctypes.data, F=2, space=capi.MEM_HOST, levels=3):
        rc = L.pnec_hip_patch_track_indexed(ptrs, pitch, n_tmpl, prev, pitch if prev is not None else None, half, pitch, levels, 0, F,
                                            96, 128, off.ctypes.data, 3, pts.ctypes.data, tmpl_image, None, None, 0.0, 0.0,
                                            patches.PATTERN52.ctypes.data, 52, 40, 0.04, 0, 10.0, None, None, None, None,
                                            o_st.ctypes.data, None, space, 0, None)
        return rc, (L.pnec_hip_last_error() or b"").decode()
    for kw, word in ((dict(n_tmpl=0), "n_tmpl_images"), (dict(tmpl_image=None), "n_tmpl_images must equal n_images"),
                     (dict(prev=None), "prev must be given"), (dict(n_tmpl=3), "outside 0 .. n_tmpl_images - 1"),
                     (dict(levels=9), "n_levels"), (dict(F=0), "n_images")):
        rc, msg = indexed(**kw)
        assert rc == -1 and "patch_track_indexed" in msg and word in msg, (kw, rc, msg)
    ti[1] = -1
    rc, msg = indexed()
    assert rc == -1 and "outside 0 .. n_tmpl_images - 1" in msg and np.all(o_st == -5)
    with pytest.raises(ValueError):
        pnec_amd.patch_track(pyr, pyr, pts, tmpl_image=ti)                       # prev missing
    with pytest.raises(ValueError):
        pnec_amd.Tracker(1, 96, 128, ring=2)


def test_python_facade_and_pybind_expose_the_new_names():
    import dataclasses
    import inspect
    assert {"TrackSet", "Tracker", "retain_tracks", "append_tracks"} <= set(pnec_amd.__all__)
    assert pnec_amd.retain_tracks is tracker.retain_tracks and pnec_amd.Tracker is tracker.Tracker
    assert [f.name for f in dataclasses.fields(pnec_amd.TrackSet)] == list(RETAIN_KEYS)
    sig = inspect.signature(patches.patch_track)
    assert sig.parameters["tmpl_image"].default is None
    assert list(inspect.signature(tracker.retain_tracks).parameters)[:3] == ["tracks", "track_result", "max_age"]
    assert list(inspect.signature(tracker.append_tracks).parameters)[:7] == \
        ["tracks", "keypoints", "det_cov", "tmpl_image_base", "capacity", "next_id", "rows"]
    params = inspect.signature(tracker.Tracker.__init__).parameters
    assert list(params)[1:4] == ["n_sequences", "height", "width"] and params["levels"].default == 5 and params["grid"].default == 30
    assert hasattr(tracker.Tracker, "process")
    import pnec_amd.pypnec as pypnec
    assert {"retain_tracks", "append_tracks"} <= set(dir(pypnec))
    facade = open(os.path.join(ROOT, "pnec_amd", "csrc", "host", "pnec_host.h")).read()
    assert "RetainTracks(" in facade and "AppendTracks(" in facade and "tmpl_image" in facade
    with open(os.path.join(ROOT, "pnec_amd", "libpnec_host.so"), "rb") as f:
        blob = f.read()
    assert b"RetainTracks" in blob and b"AppendTracks" in blob


# ---- the kernels' control flow on the host, under the sanitizers -----------------------------------------------------
@functools.lru_cache(maxsize=None)
def _host_program():
    import tempfile
    gxx = shutil.which("g++")
    assert gxx, "g++ builds the host facade, so it is there"
    exe = os.path.join(tempfile.mkdtemp(prefix="tracks_host_"), "tracks_host")
    subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "pnec_amd", "csrc"),
                    os.path.join(ROOT, "tools", "tracks_host.cc"), "-o", exe], check=True)
    return exe


ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
_DT = dict(offsets=np.int64, id=np.int64, tmpl_image=np.int32, tmpl_pts=np.float64, age=np.int32, pts=np.float64,
           angle=np.float64, cov=np.float64, prev_pts=np.float64, prev_cov=np.float64, src=np.int64)
_W = dict(tmpl_pts=2, pts=2, cov=3, prev_pts=2, prev_cov=3)


def _run_host(tmp_path, header, arrays):
    blob = [np.array(header, dtype=np.int64).tobytes()] + [np.ascontiguousarray(a).tobytes() for a in arrays if a is not None]
    (tmp_path / "job.bin").write_bytes(b"".join(blob))
    r = subprocess.run([_host_program(), str(tmp_path / "job.bin"), str(tmp_path / "out.bin")], env=ENV, capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "without slack" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    return (tmp_path / "out.bin").read_bytes()


def _unpack(raw, layout):
    """layout: list of (key, dtype, shape or None) in the order the program writes"""
    out, at = {}, 0
    for key, dt, shape in layout:
        if shape is None:
            out[key] = None
            continue
        n = int(np.prod(shape)) * np.dtype(dt).itemsize
        out[key] = np.frombuffer(raw[at:at + n], dtype=dt).reshape(shape).copy()
        at += n
    assert at == len(raw), (at, len(raw))
    return out


def _set_layout(F, N, cov, prefix=()):
    return [("offsets", np.int64, (F + 1,))] + \
        [(k, _DT[k], ((N, _W[k]) if k in _W else (N,)) if (k != "cov" or cov) else None) for k in SET_KEYS[1:]]


def run_host_retain(tmp_path, kw):
    s, trk = kw["s"], kw["trk"]
    F, N = len(s["offsets"]) - 1, len(s["id"])
    flags = (1 if kw["with_cov"] else 0) | (2 if kw["with_prev_pts"] else 0) | (4 if kw["with_src"] else 0)
    raw = _run_host(tmp_path, [0, F, N, 0, N, kw["max_age"], 0, 0, flags],
                    [s[k] for k in SET_KEYS if k != "angle"] + [trk["pts"], trk["angle"], trk["cov"] if kw["with_cov"] else None,
                                                                trk["status"]])
    layout = _set_layout(F, N, kw["with_cov"]) + [("prev_pts", np.float64, (N, 2) if kw["with_prev_pts"] else None),
                                                  ("prev_cov", np.float64, (N, 3) if kw["with_cov"] else None),
                                                  ("src", np.int64, (N,) if kw["with_src"] else None)]
    return _unpack(raw, layout)


def run_host_append(tmp_path, kw):
    s, det = kw["s"], kw["det"]
    F, N, D, O = len(det["offsets"]) - 1, 0 if s is None else len(s["id"]), len(det["pts"]), kw["n_out"]
    flags = (1 if kw["with_cov"] else 0) | (8 if s is not None else 0) | (16 if s is not None and s["cov"] is not None else 0) | \
        (32 if det["cov"] is not None else 0)
    raw = _run_host(tmp_path, [1, F, N, D, O, 0, kw["base"], kw["capacity"], flags],
                    ([s[k] for k in SET_KEYS] if s is not None else []) + [det["offsets"], det["pts"], det["cov"], kw["next_id"]])
    got = _unpack(raw, _set_layout(F, O, kw["with_cov"]) + [("next_id", np.int64, (F,)), ("dropped", np.int64, (F,))])
    return got, got["next_id"], got["dropped"]


def test_the_kernels_control_flow_built_for_the_host_reads_nothing_outside_and_equals_numpy(tmp_path):
    for name, kw in retain_cases():
        assert_same(run_host_retain(tmp_path, kw), retain_reference(kw), RETAIN_KEYS, f"host replay, retain, {name}")
    for name, kw in append_cases():
        got, nid, dropped = run_host_append(tmp_path, kw)
        ref, rnid, rdropped = append_reference(kw)
        assert_same(got, ref, SET_KEYS, f"host replay, append, {name}")
        assert np.array_equal(nid, rnid) and np.array_equal(dropped, rdropped), name


# ---- the sequence fixture and one step of the tracker in numpy -------------------------------------------------------
# (edge 27: no corner -- integers -- puts a pattern point of its coarsest template exactly on the validity threshold)
SEQ_F, SEQ_FRAMES, SEQ_RING, SEQ_GRID, SEQ_CAPACITY, SEQ_EDGE = 3, 4, 3, 30, 8, 27
SEQ_STEP_SHIFT, SEQ_STEP_ANGLE = np.array([4.1, -2.9]), 0.02


def _warped(seed, n):
    """frame n of a sequence: the texture `seed` moved n times by a rotation about the centre and a shift"""
    yy, xx = np.mgrid[0:H0, 0:W0].astype(np.float64)
    ctr = np.array([(W0 - 1) / 2.0, (H0 - 1) / 2.0])
    c, s = np.cos(n * SEQ_STEP_ANGLE), np.sin(n * SEQ_STEP_ANGLE)
    ux, uy = xx - ctr[0] - n * SEQ_STEP_SHIFT[0], yy - ctr[1] - n * SEQ_STEP_SHIFT[1]
    return analytic(c * ux + s * uy + ctr[0], -s * ux + c * uy + ctr[1], seed)


@functools.lru_cache(maxsize=None)
def sequence_fixture():
    """-> dict: frames [4][3,96,128] uint8 -- three sequences of four frames of the `analytic` texture, each frame the
    previous one moved by a known warp --, with: sequence 0's frame 1 blank in a region (tracks die there, and the corners
    of the region's border are born with a template half blank), sequence 1 carrying another texture in a region from
    frame 2 on, moving with the rest (the tracks that were there end up somewhere: too far, or lost forward or backward;
    the corners born on it are tracked like any other), sequence 2's frame 1 blank altogether (every track dies, nothing is
    detected: the image has no track at the next step).  pyr [4]: their pyramids (pyramid_levels_np)."""
    frames = []
    for n in range(SEQ_FRAMES):
        img = np.stack([_warped(300 + f, n) for f in range(SEQ_F)])
        if n == 1:
            img[0, 20:70, 60:110] = 0.0
            img[2] = 0.0
        if n >= 2:
            img[1, 10:80, 20:80] = _warped(777, n)[10:80, 20:80]
        frames.append(np.round(img).astype(np.uint8))
    for a in frames:
        a.setflags(write=False)
    return dict(frames=frames, pyr=[pyramid_levels_np(a, LEVELS) for a in frames])


def ring_stack(n):
    """the tracker's stack after frame n went in: per level [R * F, h_l, w_l], frame m in slot m % R, the newest wins"""
    fx = sequence_fixture()
    stack = [np.zeros((SEQ_RING * SEQ_F,) + lv.shape[1:], np.uint8) for lv in fx["pyr"][0]]
    for m in range(n + 1):
        s = m % SEQ_RING
        for l in range(LEVELS):
            stack[l][s * SEQ_F:(s + 1) * SEQ_F] = fx["pyr"][m][l]
    return stack


def track_indexed_np(stack, prev, nxt, s, n_images, **kw):
    """pnec_hip_patch_track_indexed on all rows of the set s, padding included (a row at or beyond offsets[F] belongs to
    the last image, as the kernels clamp it): patch_track_np, one call per (image, template image)"""
    N = len(s["id"])
    off = np.asarray(s["offsets"])
    image = np.minimum(np.searchsorted(off, np.arange(N), side="right") - 1, n_images - 1)
    keys = ("pts", "angle", "cov", "dist2", "status", "lost_level", "kappa", "edge")
    out = None
    for f, ti in sorted(set(zip(image.tolist(), s["tmpl_image"].tolist()))):
        rows = np.flatnonzero((image == f) & (s["tmpl_image"] == ti))
        r = patch_track_np([lv[ti] for lv in stack], [lv[f] for lv in nxt], s["tmpl_pts"][rows], prev=[lv[f] for lv in prev],
                           init_pts=s["pts"][rows], init_angle=s["angle"][rows], **kw)
        if out is None:
            out = {k: np.zeros((N,) + r[k].shape[1:], r[k].dtype) for k in keys}
        for k in keys:
            out[k][rows] = r[k]
    return out


def tracker_step_np(n, s, next_id, capacity=SEQ_CAPACITY, grid=SEQ_GRID, ring=SEQ_RING):
    """What Tracker.process does with frame n of the sequence fixture when its set is `s` (None for n = 0) and its id
    counters `next_id`: -> dict trk (None for n = 0), retained (None), det, det_cov, out, next_id, dropped."""
    fx = sequence_fixture()
    F, N = SEQ_F, SEQ_F * capacity
    cur = fx["pyr"][n]
    trk = retained = None
    if n > 0:
        trk = track_indexed_np(ring_stack(n), fx["pyr"][n - 1], cur, s, F)
        retained = retain_np(s, trk, max_age=ring - 2)
    det = detect_np(cur[0], grid, 1, 5, SEQ_EDGE, current=None if retained is None else (retained["offsets"], retained["pts"]))
    det_cov = patch_cov_np(cur[0], det["pts"], det["offsets"])["cov"]
    out, nid, dropped = append_np(retained, det["offsets"], det["pts"], det_cov, (n % ring) * F, capacity, next_id, N)
    return dict(trk=trk, retained=retained, det=det, det_cov=det_cov, out=out, next_id=nid, dropped=dropped)


@functools.lru_cache(maxsize=None)
def sequence_reference():
    """the four steps, each from the previous one's numpy set"""
    steps, s, nid = [], None, np.zeros(SEQ_F, np.int64)
    for n in range(SEQ_FRAMES):
        st = tracker_step_np(n, s, nid)
        steps.append(st)
        s, nid = st["out"], st["next_id"]
    return steps


def test_padding_is_inert_in_the_three_calls_that_are_given_the_full_capacity():
    """a NaN template is BAD_TEMPLATE, a NaN current point marks no cell, a NaN point is an EMPTY patch"""
    fx = sequence_fixture()
    pyr = [lv[:1] for lv in fx["pyr"][0]]
    nan2 = np.full((2, 2), NAN)
    r = patch_track_np(pyr, pyr, nan2, init_pts=nan2, init_angle=np.full(2, NAN))
    assert np.all(r["status"] == BAD) and np.all(np.isnan(r["cov"]))
    img = fx["frames"][0][:1]
    a = detect_np(img, SEQ_GRID, 1, 5, SEQ_EDGE)
    b = detect_np(img, SEQ_GRID, 1, 5, SEQ_EDGE, current=(np.array([0, 2]), nan2))
    assert np.array_equal(a["cell"], b["cell"]) and np.array_equal(a["pts"], b["pts"]) and len(a["pts"]) > 0
    c = patch_cov_np(img, nan2, np.array([0, 2]))
    assert np.all(c["status"] == patches.PATCH_EMPTY) and np.all(np.isnan(c["cov"]))


def test_the_sequence_fixture_has_the_power_the_gpu_test_relies_on():
    steps = sequence_reference()
    assert steps[0]["trk"] is None and len(steps) == SEQ_FRAMES == 4 and SEQ_RING - 2 == 1
    live_status, pad_status, edges = [], [], []
    two_frames = refilled = hit_capacity = retired_by_age = empty_image = False
    for n in range(1, SEQ_FRAMES):
        s, st = steps[n - 1]["out"], steps[n]
        off, trk = s["offsets"], st["trk"]
        live = np.arange(len(s["id"])) < off[-1]
        live_status += trk["status"][live].tolist()
        pad_status += trk["status"][~live].tolist()
        edges += trk["edge"][live].tolist()
        for f in range(SEQ_F):
            rows = slice(int(off[f]), int(off[f + 1]))
            frames_of = set((s["tmpl_image"][rows] // SEQ_F).tolist())
            assert set((s["tmpl_image"][rows] % SEQ_F).tolist()) <= {f}
            two_frames |= len(frames_of) >= 2
            empty_image |= off[f] == off[f + 1]
            retired_by_age |= bool(np.any((trk["status"][rows] == OK) & (s["age"][rows] + 1 > SEQ_RING - 2)))
        refilled |= bool(np.any(np.diff(st["det"]["offsets"]) > 0) and np.any(st["det"]["cell"] == -1))
    for st in steps:
        hit_capacity |= bool(np.any(st["dropped"] > 0) and np.any(np.diff(st["out"]["offsets"]) == SEQ_CAPACITY))
    # every status that ends a track on live rows; BAD_TEMPLATE is what the padding rows of the same calls come back with
    # (a live row's template is a detected corner of a textured image: it cannot be empty or singular here)
    assert {LOSTF, LOSTB, FAR, OK} <= set(live_status) and BAD not in live_status
    assert pad_status and set(pad_status) == {BAD}
    assert two_frames and refilled and hit_capacity and retired_by_age and empty_image
    assert min(edges) > 1e-6, min(edges)
    ids = [st["out"]["id"][:st["out"]["offsets"][-1]] for st in steps]
    for st in steps:                                            # ids unique per image, ascending within an image
        o = st["out"]
        for f in range(SEQ_F):
            row = o["id"][o["offsets"][f]:o["offsets"][f + 1]]
            assert np.all(np.diff(row) > 0)
    assert max(i.max() for i in ids) + 1 == max(st["next_id"].max() for st in steps)
