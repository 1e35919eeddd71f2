"""Keyframe pairs (pnec_hip_tracks_keyframe) without a device: the ABI and the Python names, the rule in numpy
(`keyframe_np`, a statement of the header's definition) on hand-worked cases, every refusal, and the kernels' control flow
replayed on the host under the sanitizers (tools/keyframe_host.cc, a program of its own) against `keyframe_np`.

Tolerance of `mean`: the program adds in the header's order with separate multiplies and adds where a device may fuse
them; an image of the cases has at most 257 positive terms of at most 2 ulp each, so the means agree within
600 * 2^-53 ~ 7e-14 relative: MEAN_RTOL = 1e-12.  The cases keep every mean at least MARGIN = 1e-6 from the threshold
(asserted on the numpy side), so `accepted` is exact."""
import dataclasses
import functools
import inspect
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import pnec_amd
from pnec_amd import capi, keyframes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "pnec_hip_tracks_keyframe"
MEAN_RTOL, MARGIN = 1e-12, 1e-6
PAIR_KEYS = ("offsets", "key_pts", "pts", "cov", "key_cov", "row", "accepted", "mean", "n_matches")
STATE_KEYS = ("next_key_pts", "next_key_cov", "next_span")
OUT_KEYS = PAIR_KEYS + STATE_KEYS
NAN = float("nan")


# ---- the rule in numpy -----------------------------------------------------------------------------------------------
def _range(offsets, f, rows):
    lo = min(max(int(offsets[f]), 0), rows)
    hi = min(max(int(offsets[f + 1]), lo), rows)
    return lo, hi


def ordered_sum(d_by_local_row):
    """the header's order: lane l of 64 adds its rows l, l + 64, ... in order; then the tree 32, 16, .. 1"""
    part = np.zeros(64)
    for l, d in d_by_local_row:
        part[l % 64] += d
    s = 32
    while s >= 1:
        part[:s] = part[:s] + part[s:2 * s]
        s //= 2
    return part[0]


def keyframe_np(B, A, state, min_displacement, max_span):
    """B: dict(offsets, pts, cov, src) or None (the first-frame form); A: dict(offsets, pts, cov); state: dict(key_pts,
    key_cov, span) or None.  cov entries may be None (all of them).  -> dict of OUT_KEYS."""
    F = len(A["offsets"]) - 1
    n_new = len(A["pts"])
    with_cov = A["cov"] is not None
    N = 0 if B is None else len(B["pts"])
    S = 0 if B is None else len(state["key_pts"])
    out = dict(offsets=np.zeros(F + 1, np.int64), key_pts=np.full((N, 2), NAN), pts=np.full((N, 2), NAN),
               cov=np.full((N, 3), NAN) if with_cov else None,
               key_cov=np.full((N, 3), NAN) if with_cov else None, row=np.full(N, -1, np.int64),
               accepted=np.zeros(F, np.uint8), mean=np.full(F, NAN), n_matches=np.zeros(F, np.int32),
               next_key_pts=np.full((n_new, 2), NAN), next_key_cov=np.full((n_new, 3), NAN) if with_cov else None,
               next_span=np.zeros(F, np.int32))
    at = 0
    for f in range(F):
        lo_a, hi_a = _range(A["offsets"], f, n_new)
        lo_b = hi_b = 0
        matches, terms = [], []
        if B is not None:
            lo_b, hi_b = _range(B["offsets"], f, N)
            for k in range(lo_b, hi_b):
                s = int(B["src"][k])
                if 0 <= s < S and np.isfinite(state["key_pts"][s]).all() and np.isfinite(B["pts"][k]).all():
                    dx, dy = B["pts"][k] - state["key_pts"][s]
                    matches.append(k)
                    terms.append((k - lo_b, np.sqrt(dx * dx + dy * dy)))
        n = len(matches)
        mean = ordered_sum(terms) / n if n else NAN
        span = 0 if B is None else max(int(state["span"][f]), 0)
        accepted = B is None or not (mean < min_displacement) or span + 1 >= max_span
        out["n_matches"][f], out["mean"][f], out["accepted"][f] = n, mean, accepted
        out["next_span"][f] = 0 if accepted else min(span + 1, 2 ** 31 - 1)
        if accepted:
            for k in matches:
                s = int(B["src"][k])
                out["key_pts"][at], out["pts"][at], out["row"][at] = state["key_pts"][s], B["pts"][k], k
                if with_cov:
                    out["cov"][at], out["key_cov"][at] = B["cov"][k], state["key_cov"][s]
                at += 1
        out["offsets"][f + 1] = at
        take = min(hi_b - lo_b, hi_a - lo_a)
        for i in range(lo_a, hi_a):
            l = i - lo_a
            if accepted:
                out["next_key_pts"][i] = A["pts"][i]
                if with_cov:
                    out["next_key_cov"][i] = A["cov"][i]
            elif l < take:
                s = int(B["src"][lo_b + l])
                if 0 <= s < S:
                    out["next_key_pts"][i] = state["key_pts"][s]
                    if with_cov:
                        out["next_key_cov"][i] = state["key_cov"][s]
    return out


def margin_ok(ref, min_displacement):
    m = ref["mean"][np.isfinite(ref["mean"])]
    return bool((np.abs(m - min_displacement) > MARGIN).all())


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def assert_same(got, ref, what, keys=OUT_KEYS):
    """bitwise, except `mean` (MEAN_RTOL, NaN where the reference has NaN)"""
    for k in keys:
        if ref[k] is None:
            assert got.get(k) is None, (what, k)
            continue
        if k == "mean":
            g, r = np.asarray(got[k]), ref[k]
            assert g.shape == r.shape and np.array_equal(np.isnan(g), np.isnan(r)), (what, k, g, r)
            fin = ~np.isnan(r)
            assert np.all(np.abs(g[fin] - r[fin]) <= MEAN_RTOL * np.abs(r[fin])), (what, k, g, r)
        else:
            assert same_bits(got[k], ref[k]), (what, k, got[k], ref[k])


# ---- cases -----------------------------------------------------------------------------------------------------------
def make_case(seed, counts_b, counts_a, scales, span, with_cov=True, slack_b=3, slack_a=2, n_key_rows=None, bad_src=0.1,
              nan_key=0.1):
    """A step with retained counts `counts_b`, refilled counts `counts_a`, per-image displacement scale `scales` (every
    match of image f moved by scales[f] * u, u in 0.5 .. 1.5, in a random direction: the mean is about scales[f]), random
    src -- a share `bad_src` of them -1, n_key_rows or far outside --, a share `nan_key` of the key points NaN, one pts NaN
    per image with enough rows, and slack rows at the end of both sets."""
    rng = np.random.default_rng(seed)
    F = len(counts_b)
    N, A = int(sum(counts_b)) + slack_b, int(sum(counts_a)) + slack_a
    S = max(N, 4) + 5 if n_key_rows is None else n_key_rows
    key_pts = rng.uniform(0.0, 100.0, (S, 2))
    key_pts[rng.random(S) < nan_key, rng.integers(0, 2)] = NAN
    src = rng.permutation(S)[:N].astype(np.int64) if S >= N else rng.integers(0, max(S, 1), N)
    bad = rng.random(N) < bad_src
    src[bad] = rng.choice([-1, S, S + 1000, -2 ** 40], size=int(bad.sum()))
    off_b = np.concatenate([[0], np.cumsum(counts_b)]).astype(np.int64)
    off_a = np.concatenate([[0], np.cumsum(counts_a)]).astype(np.int64)
    pts = np.full((N, 2), NAN)
    for f in range(F):
        for k in range(off_b[f], off_b[f + 1]):
            base = key_pts[src[k]] if 0 <= src[k] < S else rng.uniform(0.0, 100.0, 2)
            base = np.where(np.isfinite(base), base, 50.0)
            ang = rng.uniform(0.0, 2 * np.pi)
            pts[k] = base + scales[f] * rng.uniform(0.5, 1.5) * np.array([np.cos(ang), np.sin(ang)])
        if counts_b[f] >= 3:
            pts[off_b[f] + 1, 0] = NAN
    pts[off_b[-1]:] = rng.uniform(0.0, 100.0, (slack_b, 2))          # slack rows hold finite junk: they must not count
    src[off_b[-1]:] = rng.integers(0, max(S, 1), slack_b)
    B = dict(offsets=off_b, pts=pts, cov=rng.uniform(0.1, 1.0, (N, 3)) if with_cov else None, src=src)
    A_ = dict(offsets=off_a, pts=rng.uniform(0.0, 100.0, (A, 2)), cov=rng.uniform(0.1, 1.0, (A, 3)) if with_cov else None)
    state = dict(key_pts=key_pts, key_cov=rng.uniform(0.1, 1.0, (S, 3)) if with_cov else None,
                 span=np.array(span, dtype=np.int32))
    return B, A_, state


COUNTS_B = (0, 1, 63, 64, 65, 257)
COUNTS_A = (5, 1, 40, 64, 70, 0)          # above, equal, below, equal, above, none
SCALES = (1.0, 6.0, 0.5, 0.7, 8.0, 1.0)
SPANS = (0, 1, 0, 2, 0, 1)
THRESHOLD = 2.5


def call_cases():
    """(name, B, A, state, min_displacement, max_span)"""
    for with_cov in (True, False):
        B, A, st = make_case(11 + with_cov, COUNTS_B, COUNTS_A, SCALES, SPANS, with_cov)
        for max_span in (1, 1000):
            yield f"ragged, cov {with_cov}, max_span {max_span}", B, A, st, THRESHOLD, max_span
    B, A, st = make_case(5, (4, 0, 9), (6, 2, 3), (3.0, 1.0, 1.0), (2 ** 31 - 1, 0, 5), True, slack_b=0, slack_a=0)
    yield "no slack, a saturated span", B, A, st, THRESHOLD, 2 ** 31 - 1
    B, A, st = make_case(6, (3, 2), (3, 2), (3.0, 1.0), (0, 0), True, n_key_rows=0)
    yield "a state of no rows", B, A, st, THRESHOLD, 3
    B, A, st = make_case(7, (300,), (310,), (1.0,), (0,), False, nan_key=0.0, bad_src=0.0)
    yield "one image, zero threshold", B, A, st, 0.0, 7
    _, A, _ = make_case(8, (0, 0, 0), (4, 0, 7), (1.0,) * 3, (0,) * 3, True)
    yield "first frame", None, A, None, THRESHOLD, 2
    _, A, _ = make_case(9, (0, 0), (2, 3), (1.0,) * 2, (0,) * 2, False)
    yield "first frame without covariances", None, A, None, THRESHOLD, 2


def test_the_ragged_cases_hold_every_outcome():
    seen = set()
    for name, B, A, st, thr, max_span in call_cases():
        ref = keyframe_np(B, A, st, thr, max_span)
        assert margin_ok(ref, thr), name
        if B is None or not name.startswith("ragged"):
            continue
        below = ref["mean"] < thr
        forced = below & (ref["accepted"] == 1)
        assert not forced.any() or max_span == 1
        seen |= {"displacement"} if ((ref["accepted"] == 1) & ~below & (ref["n_matches"] > 0)).any() else set()
        seen |= {"skipped"} if (ref["accepted"] == 0).any() else set()
        seen |= {"no match"} if ((ref["accepted"] == 1) & (ref["n_matches"] == 0)).any() else set()
        seen |= {"forced"} if forced.any() else set()
        assert ref["offsets"][-1] < len(B["pts"])                      # there is padding to write
    assert seen == {"displacement", "skipped", "no match", "forced"}, seen


# ---- hand-worked ------------------------------------------------------------------------------------------------------
def hand_case():
    key_pts = np.array([[0, 0], [10, 0], [NAN, 5], [3, 4], [20, 20], [7, 7]], dtype=np.float64)
    key_cov = np.array([[100 + s, 200 + s, 300 + s] for s in range(6)], dtype=np.float64)
    span = np.array([0, 0, 2, 1, 0], dtype=np.int32)
    pts = np.array([[1, 1], [2, 2],                       # image 0: src -1 and src = n_key_rows: no match
                    [0.75, 1.0], [10, 2],                 # image 1: 1.25 and 2: mean 1.625 < 2.5, span 0: skipped
                    [5, 5], [3, 5], [20, 20],             # image 2: a NaN key point, 1 and 0: mean 0.5, span 2: forced
                    [10, 11], [NAN, 1],                   # image 3: 5 and a NaN point: mean 5: accepted
                    [9, 9], [3, 4.5],                     # image 4: src -1, 0.5: skipped
                    [NAN, NAN]], dtype=np.float64)        # slack
    src = np.array([-1, 6, 0, 1, 2, 3, 4, 5, 0, -1, 3, -1], dtype=np.int64)
    cov = np.array([[k + 0.5, k + 0.25, k + 0.125] for k in range(12)])
    B = dict(offsets=np.array([0, 2, 4, 7, 9, 11], np.int64), pts=pts, cov=cov, src=src)
    # refilled counts 3 (a new row), 1 (cut by capacity), 2 (cut), 3 (a new row), 3 (a new row); one slack row
    A = dict(offsets=np.array([0, 3, 4, 6, 9, 12], np.int64), pts=np.array([[100 + i, 200 + i] for i in range(13)], np.float64),
             cov=np.array([[i, 2 * i, 3 * i] for i in range(13)], np.float64))
    return B, A, dict(key_pts=key_pts, key_cov=key_cov, span=span)


def test_the_rule_on_hand_worked_cases():
    B, A, st = hand_case()
    r = keyframe_np(B, A, st, 2.5, 3)
    nan2, nan3 = [NAN, NAN], [NAN, NAN, NAN]
    assert r["n_matches"].tolist() == [0, 2, 2, 1, 1]
    assert np.array_equal(r["mean"], [NAN, 1.625, 0.5, 5.0, 0.5], equal_nan=True)
    assert r["accepted"].tolist() == [1, 0, 1, 1, 0] and r["next_span"].tolist() == [0, 1, 0, 0, 1]
    assert r["offsets"].tolist() == [0, 0, 0, 2, 3, 3]
    assert np.array_equal(r["key_pts"], [[3, 4], [20, 20], [7, 7]] + [nan2] * 9, equal_nan=True)
    assert np.array_equal(r["pts"], [[3, 5], [20, 20], [10, 11]] + [nan2] * 9, equal_nan=True)
    assert np.array_equal(r["cov"], [[5.5, 5.25, 5.125], [6.5, 6.25, 6.125], [7.5, 7.25, 7.125]] + [nan3] * 9, equal_nan=True)
    assert np.array_equal(r["key_cov"], [[103, 203, 303], [104, 204, 304], [105, 205, 305]] + [nan3] * 9, equal_nan=True)
    assert r["row"].tolist() == [5, 6, 7] + [-1] * 9
    want = [[100, 200], [101, 201], [102, 202],           # image 0, accepted: its own rows, the new one included
            [0, 0],                                       # image 1, skipped and cut to one row: key_pts[src[2] = 0]
            [104, 204], [105, 205],                       # image 2, forced: its own rows
            [106, 206], [107, 207], [108, 208],           # image 3
            nan2, [3, 4], nan2,                           # image 4, skipped: src -1, key_pts[3], a new row
            nan2]                                         # slack
    assert np.array_equal(r["next_key_pts"], want, equal_nan=True)
    want_cov = [[i, 2 * i, 3 * i] for i in range(3)] + [[100, 200, 300]] + [[i, 2 * i, 3 * i] for i in range(4, 9)] + \
        [nan3, [103, 203, 303], nan3, nan3]
    assert np.array_equal(r["next_key_cov"], want_cov, equal_nan=True)
    # the same step with the cap out of reach: image 2 is skipped too, and its two rows keep their key points
    r = keyframe_np(B, A, st, 2.5, 4)
    assert r["accepted"].tolist() == [1, 0, 0, 1, 0] and r["next_span"].tolist() == [0, 1, 3, 0, 1]
    assert r["offsets"].tolist() == [0, 0, 0, 0, 1, 1] and r["row"].tolist() == [7] + [-1] * 11
    assert np.array_equal(r["next_key_pts"][4:6], [[NAN, 5], [3, 4]], equal_nan=True)      # gathered as they are
    # a zero threshold accepts everything: mean < 0 never holds
    r = keyframe_np(B, A, st, 0.0, 4)
    assert r["accepted"].tolist() == [1] * 5 and r["offsets"].tolist() == [0, 0, 2, 4, 5, 6]
    # the first-frame form
    r = keyframe_np(None, A, None, 2.5, 3)
    assert r["accepted"].tolist() == [1] * 5 and r["n_matches"].tolist() == [0] * 5 and np.isnan(r["mean"]).all()
    assert r["offsets"].tolist() == [0] * 6 and r["next_span"].tolist() == [0] * 5 and r["key_pts"].shape == (0, 2)
    assert np.array_equal(r["next_key_pts"][:12], A["pts"][:12]) and np.isnan(r["next_key_pts"][12]).all()
    assert np.array_equal(r["next_key_cov"][:12], A["cov"][:12]) and np.isnan(r["next_key_cov"][12]).all()
    # the order of the sum: 65 terms, lane 0 holds two of them
    d = [(l, 1.0 + l * 2.0 ** -40) for l in range(65)]
    lanes = [d[l][1] for l in range(64)]
    lanes[0] = lanes[0] + d[64][1]
    s = 32
    while s:
        lanes = [lanes[l] + lanes[l + s] for l in range(s)]
        s //= 2
    assert ordered_sum(d) == lanes[0]


# ---- the ABI and the Python names ------------------------------------------------------------------------------------
def test_the_symbol_is_declared_bound_and_exported_within_abi_8():
    import re
    header = open(os.path.join(ROOT, "include", "pnec_hip.h")).read()
    m = re.search(r"\bint " + NAME + r"\(([^;]*)\);", header)
    assert m, "not declared in include/pnec_hip.h"
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    assert len(args) == 31 and args[0] == "int64_t n_images" and args[14] == "double min_displacement" and \
        args[15] == "int32_t max_span" and args[16] == "int64_t *out_offsets" and args[28] == "int space"
    assert re.search(r"#define PNEC_HIP_ABI_VERSION 8\b", header) and capi.ABI_VERSION == 8
    assert NAME in capi.SYMBOLS
    L = capi.lib()
    assert L.pnec_hip_abi_version() == 8 and len(getattr(L, NAME).argtypes) == 31
    for words in ("THE ORDER OF THE SUM", "accepted[f] = !(mean < min_displacement) || span[f] + 1 >= max_span", "DEVIATION",
                  "FIRST-FRAME FORM", "take = min(count_B[f], count_A'[f])"):
        assert words in header, words


def test_the_python_names_exist_with_their_defaults():
    assert {"keyframe_pairs", "KeyframePairs", "KeyframeState", "KeyframeTracker"} <= set(pnec_amd.__all__)
    assert pnec_amd.keyframe_pairs is keyframes.keyframe_pairs and pnec_amd.KeyframeTracker is keyframes.KeyframeTracker
    assert [f.name for f in dataclasses.fields(pnec_amd.KeyframePairs)] == \
        ["offsets", "key_pts", "pts", "cov", "key_cov", "row", "accepted", "mean_displacement", "n_matches"]
    assert [f.name for f in dataclasses.fields(pnec_amd.KeyframeState)] == ["key_pts", "key_cov", "span"]
    sig = inspect.signature(pnec_amd.keyframe_pairs)
    assert list(sig.parameters) == ["retained", "appended", "state", "min_displacement", "max_span", "out"]
    assert sig.parameters["out"].default is None
    sig = inspect.signature(pnec_amd.KeyframeTracker.__init__)
    assert list(sig.parameters)[:6] == ["self", "n_sequences", "height", "width", "min_displacement", "max_span"]
    assert sig.parameters["min_displacement"].default == 5.0 and sig.parameters["max_span"].default is None
    assert any(p.kind is inspect.Parameter.VAR_KEYWORD for p in sig.parameters.values())
    sig = inspect.signature(pnec_amd.Odometry.__init__)
    assert list(sig.parameters)[:9] == ["self", "n_sequences", "height", "width", "K_inv", "mode", "pipeline_options",
                                        "min_displacement", "max_span"]
    assert sig.parameters["min_displacement"].default == 0.0 and sig.parameters["max_span"].default is None
    assert sig.parameters["mode"].default == capi.MODE_TARGET and sig.parameters["pipeline_options"].default is None
    fields = dataclasses.fields(pnec_amd.OdometryResult)
    assert [f.name for f in fields] == ["q", "t", "n_corr", "pairs", "init_q", "accepted", "mean_displacement", "span"]
    assert all(f.default is None for f in fields[5:])
    # the ring's cap, checked before anything is allocated
    for kw in (dict(ring=3), dict(ring=4, max_span=3), dict(max_span=0), dict(ring=5, max_span=4), dict(min_displacement=-1.0),
               dict(min_displacement=NAN)):
        with pytest.raises(ValueError):
            pnec_amd.KeyframeTracker(1, 96, 128, **kw)


# ---- through the ABI, in HOST space -----------------------------------------------------------------------------------
def _ptr(a):
    return None if a is None else a.ctypes.data


def fresh_outputs(B, A, fill=None):
    F, N, n_new = len(A["offsets"]) - 1, 0 if B is None else len(B["pts"]), len(A["pts"])
    with_cov = A["cov"] is not None
    new = (lambda shape, dt: np.full(shape, fill, dt)) if fill is not None else (lambda shape, dt: np.empty(shape, dt))
    return dict(offsets=new(F + 1, np.int64), key_pts=new((N, 2), np.float64), pts=new((N, 2), np.float64),
                cov=new((N, 3), np.float64) if with_cov else None,
                key_cov=new((N, 3), np.float64) if with_cov else None, row=new(N, np.int64),
                accepted=new(F, np.uint8), mean=new(F, np.float64), n_matches=new(F, np.int32),
                next_key_pts=new((n_new, 2), np.float64), next_key_cov=new((n_new, 3), np.float64) if with_cov else None,
                next_span=new(F, np.int32))


def call_keyframe(L, B, A, st, thr0, max_span0, out, space=capi.MEM_HOST, **over):
    none_b, none_s = dict.fromkeys(("offsets", "pts", "cov", "src")), dict.fromkeys(("key_pts", "key_cov", "span"))
    b, s = none_b if B is None else B, none_s if st is None else st
    a = dict(F=len(A["offsets"]) - 1, offsets=_ptr(b["offsets"]), N=0 if B is None else len(B["pts"]), pts=_ptr(b["pts"]),
             cov=_ptr(b["cov"]), src=_ptr(b["src"]), new_offsets=_ptr(A["offsets"]), n_new=len(A["pts"]), new_pts=_ptr(A["pts"]),
             new_cov=_ptr(A["cov"]), S=0 if st is None else len(st["key_pts"]), key_pts=_ptr(s["key_pts"]),
             key_cov=_ptr(s["key_cov"]), span=_ptr(s["span"]), thr=thr0, max_span=max_span0,
             **{"out_" + k: _ptr(out[k]) for k in OUT_KEYS})
    a.update(over)
    rc = L.pnec_hip_tracks_keyframe(a["F"], a["offsets"], a["N"], a["pts"], a["cov"], a["src"], a["new_offsets"], a["n_new"],
                                    a["new_pts"], a["new_cov"], a["S"], a["key_pts"], a["key_cov"], a["span"], a["thr"],
                                    a["max_span"], *[a["out_" + k] for k in OUT_KEYS], space, 0, None)
    return rc, (L.pnec_hip_last_error() or b"").decode()


def test_bad_arguments_are_refused_before_a_device_is_touched():
    L = capi.lib()
    B, A, st = hand_case()
    out = fresh_outputs(B, A, fill=91)
    bad_off = [np.array(o, dtype=np.int64) for o in ((0, 3, 2, 4, 5, 6), (1, 2, 4, 7, 9, 11), (0, 2, 4, 7, 9, 14))]
    cases = [(dict(F=0), "n_images"), (dict(N=-1), "n_rows"), (dict(n_new=-1), "n_new"), (dict(S=-1), "n_key_rows"),
             (dict(offsets=None), "a retained set given in part"), (dict(pts=None), "a retained set given in part"),
             (dict(src=None), "a retained set given in part"), (dict(span=None), "the state given in part"),
             (dict(key_pts=None), "the state given in part"),
             (dict(cov=None), "together"), (dict(new_cov=None), "together"), (dict(key_cov=None), "together"),
             (dict(out_cov=None), "together"), (dict(out_key_cov=None), "together"), (dict(out_next_key_cov=None), "together"),
             (dict(new_offsets=None), "NULL"), (dict(new_pts=None), "NULL"), (dict(out_offsets=None), "out_offsets is NULL"),
             (dict(out_key_pts=None), "NULL"), (dict(out_pts=None), "NULL"), (dict(out_row=None), "NULL"),
             (dict(out_next_key_pts=None), "next-state"), (dict(out_next_span=None), "next-state"),
             (dict(thr=-0.5), "min_displacement"), (dict(thr=NAN), "min_displacement"), (dict(thr=float("inf")), "min_displacement"),
             (dict(max_span=0), "max_span"), (dict(max_span=-3), "max_span"),
             (dict(out_next_key_pts=_ptr(st["key_pts"])), "an output is an input"),
             (dict(out_next_span=_ptr(st["span"])), "an output is an input"), (dict(out_pts=_ptr(B["pts"])), "an output is an input"),
             (dict(out_offsets=_ptr(A["offsets"])), "an output is an input"), (dict(space=5), "memory space")]
    cases += [(dict(offsets=_ptr(o)), "offsets") for o in bad_off]
    cases += [(dict(new_offsets=_ptr(np.array(o, np.int64))), "new_offsets") for o in ((0, 3, 4, 6, 9, 14), (0, 3, 2, 6, 9, 12))]
    for kw, word in cases:
        rc, msg = call_keyframe(L, B, A, st, 2.5, 3, out, **kw)
        assert rc == capi.ERR_INVALID_ARGUMENT == -1 and "tracks_keyframe" in msg and word in msg, (kw, rc, msg)
    # DEVICE space refuses from the arguments alone as well
    assert call_keyframe(L, B, A, st, 2.5, 3, out, space=capi.MEM_DEVICE, max_span=0)[0] == -1
    # the first-frame form with a part of a set, or a part of a state
    o1 = fresh_outputs(None, A, fill=91)
    for kw, word in ((dict(N=3), "a retained set given in part"), (dict(src=_ptr(B["src"])), "a retained set given in part"),
                     (dict(key_pts=_ptr(st["key_pts"])), "the state given in part"), (dict(S=4), "the state given in part"),
                     (dict(out_next_key_cov=None), "together")):
        rc, msg = call_keyframe(L, None, A, None, 2.5, 3, o1, **kw)
        assert rc == -1 and "tracks_keyframe" in msg and word in msg, (kw, rc, msg)
    for o in (out, o1):
        assert all(np.all(o[k] == 91) for k in OUT_KEYS if o[k] is not None)
    # the Python layer: a retained set comes with its src and a state
    as_set = lambda d: pnec_amd.TrackSet(d["offsets"], None, None, None, None, d["pts"], None, d["cov"])
    with pytest.raises(ValueError):
        pnec_amd.keyframe_pairs(as_set(B), as_set(A), None, 2.5, 3)


# ---- the kernels' control flow on the host, under the sanitizers -----------------------------------------------------
@functools.lru_cache(maxsize=None)
def _host_program():
    import tempfile
    gxx = shutil.which("g++")
    assert gxx, "g++ builds the host facade, so it is there"
    exe = os.path.join(tempfile.mkdtemp(prefix="keyframe_host_"), "keyframe_host")
    subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "pnec_amd", "csrc"),
                    os.path.join(ROOT, "tools", "keyframe_host.cc"), "-o", exe], check=True)
    return exe


ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


def run_host(tmp_path, B, A, st, thr, max_span):
    F, N, n_new = len(A["offsets"]) - 1, 0 if B is None else len(B["pts"]), len(A["pts"])
    S = 0 if st is None else len(st["key_pts"])
    with_cov = A["cov"] is not None
    header = struct.pack("<6q", F, N, n_new, S, max_span, (1 if with_cov else 0) | (2 if B is not None else 0)) + struct.pack("<d", thr)
    arrays = ([B["offsets"], B["pts"], B["cov"], B["src"]] if B is not None else []) + [A["offsets"], A["pts"], A["cov"]] + \
        ([st["key_pts"], st["key_cov"], st["span"]] if B is not None else [])
    (tmp_path / "job.bin").write_bytes(header + b"".join(np.ascontiguousarray(a).tobytes() for a in arrays if a is not None))
    r = subprocess.run([_host_program(), str(tmp_path / "job.bin"), str(tmp_path / "out.bin")], env=ENV, capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "without slack" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    raw = (tmp_path / "out.bin").read_bytes()
    got, at = fresh_outputs(B, A), 0
    for k in OUT_KEYS:
        if got[k] is None:
            continue
        n = got[k].nbytes
        got[k] = np.frombuffer(raw[at:at + n], dtype=got[k].dtype).reshape(got[k].shape).copy()
        at += n
    assert at == len(raw), (at, len(raw))
    return got


def test_the_kernels_control_flow_built_for_the_host_reads_nothing_outside_and_equals_numpy(tmp_path):
    cases = list(call_cases()) + [("hand-worked", *hand_case(), 2.5, 3)]
    for name, B, A, st, thr, max_span in cases:
        ref = keyframe_np(B, A, st, thr, max_span)
        assert margin_ok(ref, thr), name
        assert_same(run_host(tmp_path, B, A, st, thr, max_span), ref, f"host replay, {name}")
