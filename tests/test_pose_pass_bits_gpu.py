"""pnec_hip_pose_covariance, pnec_hip_residuals, pnec_hip_triangulate and pnec_hip_relative_scale, bit for bit, against
outputs recorded on the commit BEFORE what their four kernels share -- the slot geometry, the pose set-up, the plane
load, the exchange of the wavefronts' partials and the dispatch by mode -- moved into pnec_pose_pass.hpp.
The move claims to preserve every bit of every output, so every field is held to equality of its raw words (float64
as int64: a NaN equals itself); there is no tolerance.

tools/record_pose_pass_bits.py owns the inputs (made from integer arithmetic, not stored) and the list of calls;
tests/golden/pose_pass_bits_parent.npz holds the recorded outputs: per slot raw, per correspondence raw for pairs of up
to 65 correspondences and one SHA-256 per pair and field above that.

The first three tests need no GPU: they hold the recorder's inputs to the cases the comparison is there for, and the
fixture to the recorder's list of calls.
"""
import hashlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_pose_pass_bits as rpb  # noqa: E402


def test_inputs_reach_every_branch_of_the_pose_and_every_wave_count():
    a, b = rpb.make_batch("A"), rpb.make_batch("B")
    for batch in (a, b):
        reached = set()
        for q, t in zip(batch["q"], batch["t"]):
            reached |= rpb.pose_branches(q, t)
        want = {"generic", "q not finite after normalisation", "t not finite", "rho == 0", "pole, ct > 0"}
        if batch is a:
            want |= {"nrm == 0", "pole test fails on ct < 0"}
        assert reached >= want, want - reached
    # the two ways to nrm == 0 (t = 0 and an underflow of the squares), rho == 0 on both sides, both non-finite kinds
    labels = {l.split("pose: ")[1]: rpb.pose_branches(q, t) for l, q, t in zip(a["labels"], a["q"], a["t"]) if "pose: " in l}
    assert labels["t = 0"] >= {"nrm == 0"} and labels["t * 2^-664"] >= {"nrm == 0"}
    assert labels["t = +z"] == {"rho == 0"} and labels["t = -z"] == {"rho == 0"}
    assert labels["t near +z"] == {"pole, ct > 0"} and labels["t near -z"] == {"pole test fails on ct < 0"}
    assert labels["t * 2^498"] == {"generic"} and labels["q scaled by 3"] == {"generic"}
    assert labels["NaN in t"] == {"t not finite"} and labels["inf in t"] == {"t not finite"}
    sizes_a, sizes_b = np.diff(a["offsets"]).tolist(), np.diff(b["offsets"]).tolist()
    assert set(sizes_a) >= {0, 1, 63, 64, 65, 512, 513, 1025, 3585, 4097}
    assert {rpb.cov_waves(n) for n in sizes_a} == set(range(1, 9))
    assert (4097 + 511) // 512 > 8                                  # the cap binds
    assert rpb.cov_waves(max(sizes_a)) == 8 and rpb.cov_waves(max(sizes_b)) == 1 and max(sizes_b) == 512
    assert np.isnan(a["f1"]).sum() == 1 and np.isnan(a["f2"]).sum() == 1


def test_runs_cover_the_modes_the_options_and_the_links():
    runs = rpb.runs()
    for call in ("pose_covariance", "residuals", "triangulate"):
        for mode in rpb.MODES:
            mine = [kw for c, m, _, kw in runs if c == call and m == mode]
            assert {(kw["batch"], kw["n_hyp"]) for kw in mine} >= {("A", 3), ("A", 1), ("B", 1)}, (call, mode)
            if call == "triangulate":
                for batch in "AB":
                    assert {(kw["orient"], kw["per_corr"]) for kw in mine if kw["batch"] == batch} == \
                        {(1, "var"), (1, "novar"), (0, "var"), (1, None), (0, None)}
    rs = [kw for c, _, _, kw in runs if c == "relative_scale"]
    assert {kw["min_parallax"] for kw in rs} == {0.0, 0.02} and {kw["per_link"] for kw in rs} == {0, 1}
    assert {kw["batch"] == kw["prev"] for kw in rs} == {True, False}
    data = {n: rpb.make_batch(n) for n in "AB"}
    seen = set()
    for kw in rs:
        cur, prev = data[kw["batch"]], data[kw["prev"]]
        prev_pair, link = rpb.links(cur, prev, kw["variant"])
        oc, op = cur["offsets"], prev["offsets"]
        for p, pp in enumerate(prev_pair):
            l = link[oc[p]:oc[p + 1]]
            if pp < 0:
                seen.add("prev_pair -1")
            elif pp >= len(op) - 1:
                seen.add("prev_pair out of range")
            else:
                n_prev = int(op[pp + 1] - op[pp])
                if len(l) == n_prev > 1 and sorted(l.tolist()) == list(range(n_prev)):
                    seen.add("permutation")
                if (l == -1).any():
                    seen.add("link -1")
                if (l >= n_prev).any():
                    seen.add("link past the end")
    assert seen == {"prev_pair -1", "prev_pair out of range", "permutation", "link -1", "link past the end"}, seen


@pytest.fixture(scope="module")
def recorded():
    return np.load(rpb.FIXTURE)


@pytest.fixture(scope="module")
def device():
    dev = rpb.Device()
    yield dev
    dev.close()


def test_fixture_says_which_build_made_it(recorded):
    assert len(str(recorded["recorded_on_commit"])) == 40 and len(str(recorded["recorded_lib_sha256"])) == 64
    assert os.path.getsize(rpb.FIXTURE) < 1_000_000
    want = set()
    for call, mode, label, kw in rpb.runs():
        fields = {"pose_covariance": [(f[0], "slot") for f in rpb.COV_FIELDS],
                  "residuals": [(f[0], "corr") for f in rpb.RES_CORR] + [(f[0], "slot") for f in rpb.RES_SLOT],
                  "triangulate": [(f[0], "corr") for f in rpb.TRI_CORR
                                  if kw.get("per_corr") == "var" or (kw.get("per_corr") == "novar" and f[0] != "depth1_var")]
                                 + [(f[0], "slot") for f in rpb.TRI_SLOT],
                  "relative_scale": ([("ratio", "corr"), ("used", "corr")] if kw.get("per_link") else [])
                                    + [("scale", "slot"), ("n_linked", "slot"), ("n_used", "slot")]}[call]
        for field, kind in fields:
            want |= {rpb.key(call, mode, label, field) + s for s in (("",) if kind == "slot" else ("/small", "/sha256"))}
    assert set(recorded.keys()) == want | {"recorded_on_commit", "recorded_lib_sha256"}


def _differences(call, mode, label, kw, got, z, data):
    offsets, labels, n_hyp = data["offsets"], data["labels"], kw["n_hyp"]
    sizes = np.diff(offsets)
    where = f"{call} mode={'-' if mode is None else rpb.MODE_NAMES[mode]} [{label}]"
    bad = []
    for field, (v, kind) in got.items():
        k = rpb.key(call, mode, label, field)
        a = rpb.bits(v)
        if kind == "slot":
            want = z[k]
            assert a.shape == want.shape and a.dtype == want.dtype, (where, field)
            for s in np.flatnonzero((a != want).reshape(len(a), -1).any(axis=1)):
                p, h = divmod(int(s), n_hyp)
                bad.append(f"{where} slot {s} (pair {p} '{labels[p]}', hypothesis {h}, {int(sizes[p])} correspondences) "
                           f"field {field}: got {v[s].tolist()}, recorded words {want[s].tolist()}")
            continue
        small, sha = z[k + "/small"], z[k + "/sha256"]
        at, big = 0, 0
        for p, n in enumerate(sizes):
            seg = a[n_hyp * offsets[p]:n_hyp * offsets[p + 1]]
            if n <= rpb.SMALL:
                want = small[at:at + len(seg)]
                at += len(seg)
                rows = np.flatnonzero((seg != want).reshape(len(seg), seg.shape[1]).any(axis=1))
                if len(rows):
                    h, i = divmod(int(rows[0]), int(n))
                    bad.append(f"{where} slot {p * n_hyp + h} (pair {p} '{labels[p]}', hypothesis {h}, {int(n)} correspondences) "
                               f"field {field}: {len(rows)} entries differ, the first at correspondence {i}")
            else:
                digest = np.frombuffer(hashlib.sha256(np.ascontiguousarray(seg).tobytes()).digest(), dtype=np.uint8)
                if not np.array_equal(digest, sha[big]):
                    bad.append(f"{where} slots {p * n_hyp}..{p * n_hyp + n_hyp - 1} (pair {p} '{labels[p]}', {int(n)} "
                               f"correspondences) field {field}: the SHA-256 of the pair's entries differs")
                big += 1
        assert at == len(small) and big == len(sha), (where, field)
    return bad


CALLS = [(c, m) for c in ("pose_covariance", "residuals", "triangulate") for m in rpb.MODES] + [("relative_scale", None)]


@pytest.mark.gpu
@pytest.mark.parametrize("call,mode", CALLS, ids=[f"{c}-{'-' if m is None else rpb.MODE_NAMES[m]}" for c, m in CALLS])
def test_every_output_is_bitwise_the_recorded_one(recorded, device, call, mode):
    bad = []
    for c, m, label, kw in rpb.runs():
        if (c, m) == (call, mode):
            bad += _differences(call, mode, label, kw, device.run(c, m, kw), recorded, device.data[kw["batch"]])
    assert not bad, f"{len(bad)} differences; the first: " + " | ".join(bad[:4])
