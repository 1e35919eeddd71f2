#!/usr/bin/env python3
"""Record the outputs of pnec_hip_pose_covariance, pnec_hip_residuals, pnec_hip_triangulate and pnec_hip_relative_scale,
bit for bit, as the fixture tests/golden/pose_pass_bits_parent.npz.

    python tools/record_pose_pass_bits.py --commit <sha>   # on a GPU, against a build of the commit to compare with

tests/test_pose_pass_bits_gpu.py runs the current build on the same inputs and requires every output field to be the
recorded bits.  The fixture is recorded ONCE, on the commit before the change that claims to preserve every bit of the
four kernels (what they share moved into pnec_pose_pass.hpp: DESIGN.md 9p), with that commit's library loaded through
PNEC_HIP_LIB.  NEVER re-record on the refactored build: that would compare the build with itself.

The inputs are not stored: this module makes them from integer arithmetic alone (a counter hashed by splitmix64, small
integer quaternions whose rotation matrices are integer up to a common factor, powers of two as scales), so they are
the same doubles on every machine.  Outputs per slot are stored raw; outputs per correspondence raw for pairs of up to
SMALL correspondences and as one SHA-256 per pair and field for larger pairs.

Batch "A" (blocks of eight wavefronts): pairs of SIZES_A correspondences -- both sides of one stride, of one wavefront's
512 and of every value of cov_waves up to the cap at 4097 -- then one pair of POSE_PAIR_SIZE per entry of POSE_CASES.
Batch "B" (one wavefront per block: the branch on the block's size is not taken): SIZES_B.  Slot (p, h) of a call
with n_hyp hypotheses is evaluated at the pose of pair (p + h) mod P, so with n_hyp = 3 every pose case meets three
pairs.  runs() lists the calls.
"""
import argparse
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FIXTURE = os.path.join(ROOT, "tests", "golden", "pose_pass_bits_parent.npz")
SMALL = 65
CORR_PER_WAVE, MAX_WAVES = 512, 8                      # cov_waves (pnec_amd/csrc/pnec_pose_pass.hpp)
SIZES_A = (0, 1, 63, 64, 65, 512, 513, 1025, 1537, 2049, 2561, 3073, 3585, 4097)
SIZES_B = (65, 0, 512, 1, 200)
POSE_PAIR_SIZE = 6
MODES = (0, 1, 2, 3)                                   # NEC, TARGET, HOST, SYM
MODE_NAMES = ("NEC", "TARGET", "HOST", "SYM")
REG, GATE = 1e-13, 3.0

# integer quaternions (xyzw): N R(q) is an integer matrix, N = |q|^2
QUATS = ((1, 2, 2, 4), (2, -1, 3, 6), (-1, 1, 2, 7), (3, 2, -2, 8), (0, 1, -1, 5), (1, -3, 1, 9))
T_TRUE = (48, -32, 96)                                 # in 1/128: (0.375, -0.25, 0.75)
TINY = 2.0 ** -37                                      # 7.3e-12: "within 1e-11 of the pole"


def pose_cases():
    """[(label, q, t)]: the poses that reach pose_setup's special cases, one pair of batch A each"""
    q = np.array(QUATS[0], dtype=np.float64) * 512.0 + np.array([1.0, 0.0, -1.0, 0.0])
    t = np.array(T_TRUE, dtype=np.float64) / 128.0
    z = np.array([0.0, 0.0, 1.0])
    near = np.array([0.75 * TINY, -0.5 * TINY, 0.0])
    return [("generic", q, t), ("q scaled by 3", 3.0 * q, t), ("q = 0", 0.0 * q, t), ("t = 0", q, 0.0 * t),
            ("t = +z", q, z), ("t = -z", q, -z), ("t near +z", q, z + near), ("t near -z", q, near - z),
            ("t * 2^-664", q, t * 2.0 ** -664), ("t * 2^498", q, t * 2.0 ** 498),
            ("NaN in t", q, np.array([np.nan, 0.125, 1.0])), ("inf in t", q, np.array([0.25, np.inf, 1.0]))]


def rint(tag, n, lo, hi):
    """n integers in [lo, hi), a function of (tag, index) alone (splitmix64 of a counter)"""
    with np.errstate(over="ignore"):
        x = (np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
             + np.uint64(tag) * np.uint64(0xD1B54A32D192ED03))
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        x = x ^ (x >> np.uint64(31))
    return (x >> np.uint64(11)).astype(np.int64) % (hi - lo) + lo


def int_rotation(q):
    """|q|^2 R(q) for an integer quaternion xyzw: an integer matrix"""
    x, y, z, w = (int(v) for v in q)
    return np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]], dtype=np.int64)


def make_pair(tag, n, quat):
    """(f1 [n,3], f2 [n,3], cov2 [n,3,3], cov1 [n,3,3]) of a scene in front of both cameras of the pose (quat, T_TRUE):
    f1 = X, f2 = a multiple of R'(X - t) (bearings are not unit), every 7th correspondence off its ray, every 13th
    behind the second camera."""
    X = np.stack([rint(4 * tag, n, -512, 512), rint(4 * tag + 1, n, -512, 512), rint(4 * tag + 2, n, 256, 1280)], axis=1)
    d = X - np.array(T_TRUE, dtype=np.int64)
    f2 = d @ int_rotation(quat)                         # rows: (N R)' d
    i = np.arange(n)
    f2 = f2 + (i % 7 == 3)[:, None] * np.stack([rint(4 * tag + 3, n, -4000, 4000)] * 3, axis=1) * np.array([1, -2, 1])
    f2 = np.where((i % 13 == 5)[:, None], -f2, f2)
    covs = []
    for k in (0, 1):
        A = rint(1000 + 4 * tag + k, 9 * n, -8, 8).reshape(n, 3, 3)
        covs.append((A @ A.transpose(0, 2, 1) + 4 * np.eye(3, dtype=np.int64)).astype(np.float64) * 2.0 ** -24)
    return X.astype(np.float64) / 128.0, f2.astype(np.float64) / 4096.0, covs[0], covs[1]


def make_batch(name):
    """{labels, offsets, f1, f2, cov2, cov1, q [P,4], t [P,3]} of batch "A" or "B" """
    cases = pose_cases()
    generic_t = cases[0][2]
    pairs, poses, labels = [], [], []
    sizes = SIZES_A if name == "A" else SIZES_B
    base = 0 if name == "A" else 100
    for k, n in enumerate(sizes):
        quat = QUATS[k % len(QUATS)]
        pairs.append(make_pair(base + k, n, quat))
        # near the pose the scene was made from, not at it: no residual is exactly zero
        poses.append((np.array(quat, dtype=np.float64) * 512.0 + np.array([1.0, 0.0, -1.0, 0.0]), generic_t))
        labels.append(f"N = {n}")
    if name == "A":
        for k, (label, q, t) in enumerate(cases):
            pairs.append(make_pair(50 + k, POSE_PAIR_SIZE, QUATS[0]))
            poses.append((q, t))
            labels.append(f"pose: {label}")
    else:   # the special poses on the one-wavefront block too, over the sizes it has
        for k, c in ((1, 2), (2, 6), (3, 5), (4, 10)):
            poses[k] = (cases[c][1], cases[c][2])
            labels[k] += f", pose: {cases[c][0]}"
    f1, f2, c2, c1 = (np.ascontiguousarray(np.concatenate([p[j] for p in pairs])) for j in range(4))
    if name == "A":   # a NaN bearing in the second stride of the pair of 65 and in the second wavefront of the pair of 1025
        off = np.concatenate([[0], np.cumsum(sizes)])
        f2[off[4] + 64, 1] = np.nan
        f1[off[7] + 700, 0] = np.nan
    offsets = np.concatenate([[0], np.cumsum([len(p[0]) for p in pairs])]).astype(np.int64)
    return dict(labels=labels, offsets=offsets, f1=f1, f2=f2, cov2=c2, cov1=c1,
                q=np.ascontiguousarray(np.stack([p[0] for p in poses])), t=np.ascontiguousarray(np.stack([p[1] for p in poses])))


def slot_poses(b, n_hyp):
    """(q [S,4], t [S,3]): slot (p, h) at the pose of pair (p + h) mod P"""
    P = len(b["offsets"]) - 1
    idx = (np.arange(P)[:, None] + np.arange(n_hyp)[None, :]).reshape(-1) % P
    return np.ascontiguousarray(b["q"][idx]), np.ascontiguousarray(b["t"][idx])


def links(cur, prev, variant):
    """(prev_pair int64 [P], link int32 [sum N]).  Pair p is linked to pair p - 1 + variant of `prev` (p = 0 of variant 0:
    -1, none; beyond prev's last pair: out of range, none); pair 2 to pair 2, a pair of its own size, where the link is a
    permutation.  Link i -> (5 i + 3) mod N_prev; elsewhere every 5th link -1 and every 11th past the previous pair's
    end."""
    oc, op = cur["offsets"], prev["offsets"]
    P, Pp = len(oc) - 1, len(op) - 1
    prev_pair = np.arange(P, dtype=np.int64) - 1 + variant
    prev_pair[2] = 2
    link = np.full(int(oc[-1]), -1, dtype=np.int32)
    for p in range(P):
        n, pp = int(oc[p + 1] - oc[p]), int(prev_pair[p])
        n_prev = int(op[pp + 1] - op[pp]) if 0 <= pp < Pp else 7
        i = np.arange(n)
        j = (5 * i + 3) % max(n_prev, 1)
        if not (p == 2 and n_prev == n):
            j = np.where(i % 5 == 4, -1, np.where(i % 11 == 7, n_prev + i % 3, j))
        link[oc[p]:oc[p + 1]] = j
    return prev_pair, link


# ---- the calls ------------------------------------------------------------------------------------------------------
COV_FIELDS = (("info", 15, np.float64), ("cov", 36, np.float64), ("grad", 5, np.float64), ("cost", 1, np.float64),
              ("status", 1, np.int32))
RES_CORR = (("residual", 1, np.float64), ("variance", 1, np.float64), ("mask", 1, np.uint8))
RES_SLOT = (("chi2", 1, np.float64), ("gated_chi2", 1, np.float64), ("gated_count", 1, np.int32), ("max_abs", 1, np.float64))
TRI_CORR = (("point", 3, np.float64), ("depth1", 1, np.float64), ("depth2", 1, np.float64), ("parallax", 1, np.float64),
            ("depth1_var", 1, np.float64), ("front", 1, np.uint8))
TRI_SLOT = (("n_front", 1, np.int32), ("n_back", 1, np.int32), ("sign", 1, np.int32), ("t_oriented", 3, np.float64),
            ("parallax_mean", 1, np.float64))
# (orient, per-correspondence outputs: "var" all six, "novar" all but the depth variance, None none)
TRI_CONFIGS = ((1, "var"), (1, "novar"), (0, "var"), (1, None), (0, None))


def runs():
    """[(call, mode or None, label, kwargs)] in the order they are made"""
    out = []
    for mode in MODES:
        for batch in "AB":
            for n_hyp in (1, 3):
                out.append(("pose_covariance", mode, f"{batch} n_hyp={n_hyp}", dict(batch=batch, n_hyp=n_hyp)))
                out.append(("residuals", mode, f"{batch} n_hyp={n_hyp}", dict(batch=batch, n_hyp=n_hyp)))
            for orient, per_corr in TRI_CONFIGS:
                # n_hyp = 3 (the output offset h * n) on the batch of many wavefronts, n_hyp = 1 on the other
                for n_hyp in ((3,) if batch == "A" else (1,)) + ((1,) if (batch, orient, per_corr) == ("A", 1, "var") else ()):
                    out.append(("triangulate", mode, f"{batch} n_hyp={n_hyp} orient={orient} per_corr={per_corr}",
                                dict(batch=batch, n_hyp=n_hyp, orient=orient, per_corr=per_corr)))
    for cur, prev, variant, par, per_link in (("A", "A", 0, 0.0, 1), ("A", "A", 1, 0.02, 1), ("B", "A", 2, 0.02, 1),
                                              ("B", "A", 0, 0.0, 1), ("A", "B", 0, 0.0, 0)):
        out.append(("relative_scale", None, f"cur={cur} prev={prev} variant={variant} min_parallax={par} per_link={per_link}",
                    dict(batch=cur, prev=prev, variant=variant, min_parallax=par, per_link=per_link, n_hyp=1)))
    return out


class Device:
    """the batches on the device, one per (name, mode), made when first asked for"""

    def __init__(self):
        self.data = {name: make_batch(name) for name in "AB"}
        self.batches = {}

    def batch(self, name, mode):
        from pnec_amd import Batch
        if (name, mode) not in self.batches:
            d = self.data[name]
            b = Batch(mode, d["offsets"])
            # (planes 6..11: Sigma2 of TARGET and SYM, Sigma1 of HOST; planes 12..17: Sigma1 of SYM)
            b.fill(d["f1"], d["f2"], {0: None, 1: d["cov2"], 2: d["cov1"], 3: d["cov2"]}[mode], d["cov1"] if mode == 3 else None)
            self.batches[(name, mode)] = b
        return self.batches[(name, mode)]

    def close(self):
        for b in self.batches.values():
            b.close()
        self.batches = {}

    def run(self, call, mode, kw):
        """{field: (array, "slot" | "corr")} of one call, HOST space, through the C ABI"""
        from pnec_amd import capi
        L = capi.lib()
        d = self.data[kw["batch"]]
        n_hyp = kw["n_hyp"]
        S, M = (len(d["offsets"]) - 1) * n_hyp, int(d["offsets"][-1]) * n_hyp
        q, t = slot_poses(d, n_hyp)
        new = lambda fields, rows: {k: np.full((rows, w), 7, dtype=dt) for k, w, dt in fields}
        ptr = lambda a: None if a is None else a.ctypes.data
        if call == "pose_covariance":
            o = new(COV_FIELDS, S)
            capi.check(L.pnec_hip_pose_covariance(self.batch(kw["batch"], mode)._h, ptr(q), ptr(t), n_hyp, REG,
                                                  *(ptr(o[k]) for k, _, _ in COV_FIELDS), capi.MEM_HOST, None))
            return {k: (v, "slot") for k, v in o.items()}
        if call == "residuals":
            oc, os_ = new(RES_CORR, M), new(RES_SLOT, S)
            capi.check(L.pnec_hip_residuals(self.batch(kw["batch"], mode)._h, ptr(q), ptr(t), n_hyp, REG, GATE,
                                            *(ptr(oc[k]) for k, _, _ in RES_CORR), *(ptr(os_[k]) for k, _, _ in RES_SLOT),
                                            capi.MEM_HOST, None))
            return {**{k: (v, "corr") for k, v in oc.items()}, **{k: (v, "slot") for k, v in os_.items()}}
        if call == "triangulate":
            want = {None: (), "novar": tuple(k for k, _, _ in TRI_CORR if k != "depth1_var"),
                    "var": tuple(k for k, _, _ in TRI_CORR)}[kw["per_corr"]]
            oc, os_ = new([f for f in TRI_CORR if f[0] in want], M), new(TRI_SLOT, S)
            capi.check(L.pnec_hip_triangulate(self.batch(kw["batch"], mode)._h, ptr(q), ptr(t), n_hyp,
                                              capi.TRI_ORIENT if kw["orient"] else 0,
                                              *(ptr(oc.get(k)) for k, _, _ in TRI_CORR), *(ptr(os_[k]) for k, _, _ in TRI_SLOT),
                                              capi.MEM_HOST, None))
            return {**{k: (v, "corr") for k, v in oc.items()}, **{k: (v, "slot") for k, v in os_.items()}}
        assert call == "relative_scale"
        dp = self.data[kw["prev"]]
        prev_pair, link = links(d, dp, kw["variant"])
        oc = new((("ratio", 1, np.float64), ("used", 1, np.uint8)), M) if kw["per_link"] else {}
        os_ = new((("scale", 3, np.float64), ("n_linked", 1, np.int32), ("n_used", 1, np.int32)), S)
        capi.check(L.pnec_hip_relative_scale(self.batch(kw["batch"], 0)._h, self.batch(kw["prev"], 0)._h, ptr(prev_pair),
                                             ptr(link), ptr(q), ptr(t), ptr(dp["q"]), ptr(dp["t"]), kw["min_parallax"],
                                             ptr(oc.get("ratio")), ptr(oc.get("used")), ptr(os_["scale"]), ptr(os_["n_linked"]),
                                             ptr(os_["n_used"]), capi.MEM_HOST, None))
        return {**{k: (v, "corr") for k, v in oc.items()}, **{k: (v, "slot") for k, v in os_.items()}}


def bits(a):
    """float64 as its 8-byte words, so that a NaN equals itself"""
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def pack(a, kind, offsets, n_hyp):
    """{suffix: array} as stored: a slot field raw; a per-correspondence field split by pair -- entries
    n_hyp * offsets[p] .. n_hyp * offsets[p + 1] -- the small pairs' rows raw and one SHA-256 per larger pair"""
    a = bits(a)
    if kind == "slot":
        return {"": a}
    sizes = np.diff(offsets)
    seg = [a[n_hyp * offsets[p]:n_hyp * offsets[p + 1]] for p in range(len(sizes))]
    small = [s for s, n in zip(seg, sizes) if n <= SMALL]
    sha = [np.frombuffer(hashlib.sha256(np.ascontiguousarray(s).tobytes()).digest(), dtype=np.uint8)
           for s, n in zip(seg, sizes) if n > SMALL]
    return {"/small": np.concatenate(small), "/sha256": np.stack(sha)}


def key(call, mode, label, field):
    return f"{call}/{'-' if mode is None else MODE_NAMES[mode]}/{label}/{field}"


def pose_branches(q, t):
    """Which of pose_setup's cases (pnec_amd/csrc/pnec_pose_pass.hpp) a pose takes, in numpy: a set of names"""
    with np.errstate(all="ignore"):
        qn = np.float64(1.0) / np.sqrt(np.sum(q * q))
        nrm, rho = np.sqrt(np.sum(t * t)), np.sqrt(t[0] * t[0] + t[1] * t[1])
        st, ct = rho / nrm, t[2] / nrm
    out = set()
    if nrm == 0.0:
        out.add("nrm == 0")
        st, ct = 0.0, 1.0
    if rho == 0.0:
        out.add("rho == 0")
    elif st < 1e-10 and ct > 0.0:
        out.add("pole, ct > 0")
    elif st < 1e-10 and ct < 0.0:
        out.add("pole test fails on ct < 0")
    if not np.isfinite(qn):
        out.add("q not finite after normalisation")
    if not np.all(np.isfinite(t)):
        out.add("t not finite")
    elif nrm != 0.0 and rho != 0.0 and not st < 1e-10 and np.isfinite(qn):
        out.add("generic")
    return out


def cov_waves(n):
    return min(max((n + CORR_PER_WAVE - 1) // CORR_PER_WAVE, 1), MAX_WAVES)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=FIXTURE)
    ap.add_argument("--commit", required=True, help="the commit the library (PNEC_HIP_LIB) was built from; stored in the fixture")
    a = ap.parse_args()
    from pnec_amd import capi
    arrays = {"recorded_on_commit": np.array(a.commit),
              "recorded_lib_sha256": np.array(hashlib.sha256(open(capi.LIB_PATH, "rb").read()).hexdigest())}
    dev = Device()
    for call, mode, label, kw in runs():
        got, again = dev.run(call, mode, kw), dev.run(call, mode, kw)
        offsets = dev.data[kw["batch"]]["offsets"]
        for field, (v, kind) in got.items():
            assert np.array_equal(bits(v), bits(again[field][0])), (call, mode, label, field)   # (a slot's bits are its own)
            for suffix, arr in pack(v, kind, offsets, kw["n_hyp"]).items():
                arrays[key(call, mode, label, field) + suffix] = arr
        print(call, mode, label, {f: int(np.isnan(v).sum()) for f, (v, _) in got.items() if v.dtype == np.float64})
    dev.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    np.savez_compressed(a.out, **arrays)
    print(a.out, os.path.getsize(a.out), "bytes", len(arrays), "arrays")
    assert os.path.getsize(a.out) < 1_000_000


if __name__ == "__main__":
    main()
