#!/usr/bin/env python3
"""Record the outputs of pnec_hip_eight_point and pnec_hip_essential_minimal (NISTER, SEVENPT), bit for bit, as the
fixture tests/golden/essential_bits_parent.npz.

    python tools/record_essential_bits.py --commit <sha>   # on a GPU, against a build of the commit to compare with

tests/test_essential_bits_gpu.py runs the current build on the fixture's inputs and requires every output field to be
the recorded bits.  The fixture is recorded ONCE, on the commit before the change that claims to preserve every bit of
the two kernels (their common phases moved into pnec_essential_shared.hpp: DESIGN.md 9o), with that commit's library
loaded through PNEC_HIP_LIB; recording it again on a later build would turn the test into a comparison of that build
with itself.  NEVER re-record on the refactored build.

One ragged batch per call, every call with quality="sample" and quality="all".  The inputs come from the generators of
the tests (eight_point_cases, minimal_solver_cases, minimal_solver_population) and are stored in the fixture with the
outputs, so that the test depends on no random generator's stream:
  * one pair per size of 5, 6, 7, 8, 9, 10, 15, 16, 17, 63, 64, 65, 129 as far as the algorithm accepts it: both sides of
    the minimal count, of the samples of 8 / 9, of the 16-lane row and of one wavefront stride; 129 is three trips of the
    sums loop (513 and 2049 add no path);
  * the short pair after the sixth size and the empty pair at the end (TOO_FEW);
  * the outlier pair (the sample and the sum over all rows choose different candidates);
  * the degenerate inputs of minimal_solver_population.degenerate -- pure translation, pure rotation, planar scenes,
    duplicated and identical correspondences, f2 == f1; the eight-point takes those of both algorithms.  (On the recorded
    build every one of them ends OK: 4 or 6 solutions for NISTER, 1 or 3 for SEVENPT.  NO_SOLUTION and NO_CANDIDATE are
    not among the recorded statuses.)
  * a pair of 65 with a NaN in its second stride and a pair of 17 with an infinity in its first row (NOT_FINITE);
  * NISTER only: from 20 000 noise-free pairs of five, the first on which the recorded build finds no real root
    (NO_SOLUTION) and the first with 2, with 8 and with 10 solutions, as far as they occur (rare_five_point_pairs).  On
    the recorded build 2, 8 and 10 occur; none of the 20 000 ends NO_SOLUTION.
"""
import argparse
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

FIXTURE = os.path.join(ROOT, "tests", "golden", "essential_bits_parent.npz")
MAX_SIZE = 129
CALLS = ("eight_point", "five_point", "seven_point")      # the methods of pnec_amd.Batch
QUALITIES = ("sample", "all")
EP_FIELDS = ("q", "t", "E", "singular", "gap", "quality", "choice", "status")
EM_FIELDS = EP_FIELDS + ("n_solutions", "E_all")
FIELDS = {"eight_point": EP_FIELDS, "five_point": EM_FIELDS, "seven_point": EM_FIELDS}


def _with(f, row, col, value):
    f = f.copy()
    f[row, col] = value
    return f


def make_batches():
    """{call: [(label, f1 [n,3], f2 [n,3])]} in the order of the batch"""
    import eight_point_cases as ec
    import minimal_solver_cases as mc
    import minimal_solver_population as mp
    out = {}
    for call, alg in (("eight_point", None), ("five_point", mc.NISTER), ("seven_point", mc.SEVENPT)):
        if alg is None:
            sized, short, outlier = ec.cases(), ec.short_cases(), ec.outlier_case()[0]
            degenerate = mp.degenerate(mc.NISTER) + mp.degenerate(mc.SEVENPT)
        else:
            sized, short, outlier = mc.cases(alg), mc.short_cases(alg), mc.outlier_case(alg)[0]
            degenerate = mp.degenerate(alg)
        sized = [c for c in sized if c.n <= MAX_SIZE]
        by_n = {c.n: c for c in sized}
        pairs = [(f"N = {c.n}", c.f1, c.f2) for c in sized]
        pairs.insert(6, (f"short, N = {short[0].n}", short[0].f1, short[0].f2))
        pairs.append(("outlier, N = 65", outlier.f1, outlier.f2))
        pairs += degenerate
        pairs.append(("NaN in the second stride, N = 65", by_n[65].f1, _with(by_n[65].f2, 64, 1, np.nan)))
        pairs.append(("infinity in the first row, N = 17", _with(by_n[17].f1, 0, 2, np.inf), by_n[17].f2))
        pairs.append(("empty", short[1].f1, short[1].f2))
        out[call] = [(label, np.ascontiguousarray(f1, dtype=np.float64).reshape(-1, 3),
                      np.ascontiguousarray(f2, dtype=np.float64).reshape(-1, 3)) for label, f1, f2 in pairs]
    return out


RARE_DRAWS = 20000
RARE_COUNTS = (0, 2, 8, 10)     # NO_SOLUTION and the root counts that the pairs above do not have


def rare_five_point_pairs():
    """Noise-free pairs of five from draw_pair on which the loaded library's NISTER ends with a rare number of solutions:
    the first pair of RARE_DRAWS per count of RARE_COUNTS, where there is one.  Found on the device, by the build that is
    recorded; the fixture stores the bearings like every other pair's."""
    import eight_point_cases as ec
    rng = np.random.default_rng([20268, 5])
    drawn = [ec.draw_pair(rng, 5, 0.0)[:2] for _ in range(RARE_DRAWS)]
    offsets = np.arange(RARE_DRAWS + 1, dtype=np.int64) * 5
    got = run_device("five_point", "sample", offsets, np.ascontiguousarray(np.concatenate([f1 for f1, _ in drawn])),
                     np.ascontiguousarray(np.concatenate([f2 for _, f2 in drawn])))
    out = []
    for count in RARE_COUNTS:
        rows = np.flatnonzero((got["n_solutions"] == count) & (got["status"] != 1) & (got["status"] != 2))
        if len(rows):
            out.append((f"rare: {count} solutions, N = 5", drawn[rows[0]][0], drawn[rows[0]][1]))
    return out


def batch_arrays(pairs):
    """(labels, offsets int64 [P+1], f1 [sum N,3], f2 [sum N,3])"""
    offsets = np.concatenate([[0], np.cumsum([len(f1) for _, f1, _ in pairs])]).astype(np.int64)
    return (np.array([label for label, _, _ in pairs]), offsets,
            np.ascontiguousarray(np.concatenate([f1 for _, f1, _ in pairs])),
            np.ascontiguousarray(np.concatenate([f2 for _, _, f2 in pairs])))


def run_device(call, quality, offsets, f1, f2):
    """{field: numpy array} of one call on the batch, HOST space"""
    from pnec_amd import Batch, capi
    with Batch(capi.MODE_NEC, offsets) as b:
        b.fill(f1, f2)
        r = getattr(b, call)(quality, on_device=False)
        return {k: np.ascontiguousarray(getattr(r, k)) for k in FIELDS[call]}


def bits(a):
    """float64 as its 8-byte words, so that a NaN equals itself"""
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=FIXTURE)
    ap.add_argument("--commit", required=True, help="the commit the library (PNEC_HIP_LIB) was built from; stored in the fixture")
    a = ap.parse_args()
    from pnec_amd import capi
    arrays = {"recorded_on_commit": np.array(a.commit),
              "recorded_lib_sha256": np.array(hashlib.sha256(open(capi.LIB_PATH, "rb").read()).hexdigest())}
    batches = make_batches()
    batches["five_point"][-1:-1] = rare_five_point_pairs()      # (the empty pair stays last)
    for call, pairs in batches.items():
        labels, offsets, f1, f2 = batch_arrays(pairs)
        arrays.update({f"{call}_labels": labels, f"{call}_offsets": offsets, f"{call}_f1": f1, f"{call}_f2": f2})
        for quality in QUALITIES:
            got = run_device(call, quality, offsets, f1, f2)
            again = run_device(call, quality, offsets, f1, f2)
            for k, v in got.items():
                assert np.array_equal(bits(v), bits(again[k])), (call, quality, k)   # (a pair's bits are its own rows')
                arrays[f"{call}_{quality}_{k}"] = v
            status = got["status"]
            print(call, quality, len(labels), "pairs; status", {int(s): int((status == s).sum()) for s in np.unique(status)},
                  *(["n_solutions", {int(s): int((got["n_solutions"] == s).sum()) for s in np.unique(got["n_solutions"])}]
                    if "n_solutions" in got else []))
            assert set(np.unique(status)) >= {0, 1, 2}, (call, quality)    # OK, TOO_FEW and NOT_FINITE at the least
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    np.savez_compressed(a.out, **arrays)
    print(a.out, os.path.getsize(a.out), "bytes")
    assert os.path.getsize(a.out) < 1_000_000


if __name__ == "__main__":
    main()
