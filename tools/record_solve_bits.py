#!/usr/bin/env python3
"""Record the LM solve's outputs, bit for bit, as the fixture tests/golden/solve_bits_parent.npz.

    python tools/record_solve_bits.py            # on a GPU, against a build of the commit to compare with
    python tools/record_solve_bits.py --oracle   # no GPU: what the CPU oracle makes of the same cases (choosing seeds)

tests/test_solve_bits_gpu.py solves the fixture's inputs with the current build and requires q, t, cost, iterations and
status to be the recorded bits.  The fixture is recorded ONCE, on the commit before a change that claims to preserve
every bit of the solve (the kernel that serves rejected LM steps from candidates computed ahead of time: DESIGN.md section 4);
recording it again on a later build would turn the test into a comparison of that build with itself.

The inputs (one pair per size, drawn by simulation.generate on the host from fixed seeds: anisotropic inhomogeneous
noise at noise_level 1.0, so the solves reach their noise floor and reject steps in chains; four starts per pair, the
simulator's own and three that are one to four degrees off) are stored in the fixture with the outputs, so that the
test does not depend on a random generator's stream.  The case table below is shared by this script and the test.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FIXTURE = os.path.join(ROOT, "tests", "golden", "solve_bits_parent.npz")
FAMILIES = ("TARGET", "NEC", "HOST")
N_STARTS = 4
# pair size -> forced launch geometry (corr_per_lane, waves_per_pair, lds_corr_per_lane); None = the tuner's choice,
# the small one-wavefront rungs (1, 1, 0), (2, 1, 0), (4, 1, 0)
SIZES = [(n, (8, 1, 3)) for n in (1, 5, 63, 64, 65, 128, 129, 320, 321, 511, 512)] + \
        [(n, (12, 1, 3)) for n in (513, 600, 768)] + [(1024, (8, 2, 3))] + [(n, None) for n in (5, 65, 129)]
CAPS = (1, 2, 3, 4, 5, 6, 7, 10, 25)
OPTION_SETS = [(f"cap{k}", dict(check_convergence=0, max_num_iterations=k)) for k in CAPS] + [
    ("ceres", dict()),
    ("minrad", dict(check_convergence=0, max_num_iterations=25, min_trust_region_radius=1e-3)),
]
ZERO_SETS = [(f"invalid{k}", dict(check_convergence=0, max_num_iterations=50, max_num_consecutive_invalid_steps=k))
             for k in (1, 5)]
ZERO_GEOMETRIES = ((8, 1, 3), None)
MAX_ITERATIONS, MIN_RADIUS, INVALID_STEPS = 3, 4, 5   # PNEC_HIP_TERM_*


def cases():
    """[(key of the inputs, family, geometry, option-set name, options)] in the order of the fixture's `out` rows"""
    out = []
    for fam in FAMILIES:
        for n, geom in SIZES:
            for name, kw in OPTION_SETS:
                out.append((f"n{n}", fam, geom, name, kw))
        for geom in ZERO_GEOMETRIES:
            for name, kw in ZERO_SETS:
                out.append(("zero", fam, geom, name, kw))
    return out


def zero_residual_pair():
    """tests/test_lm_branches.py's pair: f1 = f2 with small integers, R = I, t = e_z -- every residual exactly zero,
    every step invalid, Jacobian entries that are exact zeros of either sign"""
    f = np.array([[1, 2, 2], [2, -1, 2], [-2, 2, 1], [3, 0, 4], [0, 3, 4], [1, -2, 2], [2, 2, -1], [4, 0, 3]], dtype=np.float64)
    cov = np.tile(np.diag([1.0, 2.0, 4.0]) * 2.0 ** -10, (len(f), 1, 1))
    return f, f.copy(), cov, np.tile([0.0, 0.0, 0.0, 1.0], (N_STARTS, 1)), np.tile([0.0, 0.0, 1.0], (N_STARTS, 1))


def _cov6(c):
    return np.stack([c[:, 0, 0], c[:, 0, 1], c[:, 0, 2], c[:, 1, 1], c[:, 1, 2], c[:, 2, 2]], axis=1)


def cov33(c6):
    c = np.empty((len(c6), 3, 3))
    c[:, 0, 0], c[:, 0, 1], c[:, 0, 2], c[:, 1, 1], c[:, 1, 2], c[:, 2, 2] = c6.T
    c[:, 1, 0], c[:, 2, 0], c[:, 2, 1] = c[:, 0, 1], c[:, 0, 2], c[:, 1, 2]
    return c


def make_inputs():
    """{key: f1, f2, cov6, q0 [N_STARTS, 4], t0 [N_STARTS, 3]} for every size of SIZES and the zero-residual pair"""
    import torch
    from pnec_amd import simulation as sim
    d = {}
    for n in sorted({n for n, _ in SIZES}):
        g = sim.generate(1, n, seed=4100 + n, noise_level=1.0)
        rng = np.random.default_rng(900 + n)
        R_gt, t_gt = g.R_gt[0].numpy(), g.t_gt[0].numpy()
        q0, t0 = [g.init_q[0].numpy()], [g.init_t[0].numpy()]
        for _ in range(N_STARTS - 1):
            ax = rng.normal(size=3)
            ax /= np.linalg.norm(ax)
            ang = np.radians(rng.uniform(1.0, 4.0))
            R_off = sim.axis_angle_to_matrix(torch.tensor(ax)[None], torch.tensor([ang], dtype=torch.float64))[0].numpy()
            q0.append(sim.matrix_to_quaternion_xyzw(torch.tensor(R_off @ R_gt)[None])[0].numpy())
            t = R_off @ t_gt + np.radians(rng.uniform(1.0, 4.0)) * np.linalg.norm(t_gt) * ax[::-1]
            t0.append(t / np.linalg.norm(t))
        d[f"n{n}"] = (g.bvs1[0].numpy(), g.bvs2[0].numpy(), _cov6(g.covs2[0].numpy()), np.stack(q0), np.stack(t0))
    f1, f2, cov, q0, t0 = zero_residual_pair()
    d["zero"] = (f1, f2, _cov6(cov), q0, t0)
    return d


def load_inputs(z):
    return {k[3:]: tuple(z[f"{p}_{k[3:]}"] for p in ("f1", "f2", "cov6", "q0", "t0")) for k in z.files if k.startswith("f1_")}


def batch_arrays(inp, fam):
    """the pair repeated once per start: (offsets, f1, f2, covs or None, q0, t0)"""
    f1, f2, c6, q0, t0 = inp
    n = len(f1)
    covs = None if fam == "NEC" else np.tile(cov33(c6), (N_STARTS, 1, 1))
    return np.arange(N_STARTS + 1, dtype=np.int64) * n, np.tile(f1, (N_STARTS, 1)), np.tile(f2, (N_STARTS, 1)), covs, q0, t0


def solve_device(inputs, case):
    """one case on the device: [N_STARTS, 10] = q | t | cost | iterations | status"""
    from pnec_amd import Batch, capi
    key, fam, geom, _, kw = case
    offsets, f1, f2, covs, q0, t0 = batch_arrays(inputs[key], fam)
    opts = dict(kw)
    if geom is not None:
        opts.update(corr_per_lane=geom[0], waves_per_pair=geom[1], lds_corr_per_lane=geom[2])
    o = capi.default_options(**opts)
    with Batch(getattr(capi, "MODE_" + fam), offsets) as b:
        if geom is not None:
            d = b.describe_launch(o)
            assert d["resident"] and (d["corr_per_lane"], d["waves_per_pair"], d["lds_corr_per_lane"]) == geom, (case, d)
        b.fill(f1, f2, covs)
        r = b.solve(q0, t0, reg=1e-13, options=o)
    return np.concatenate([r.q, r.t, r.cost[:, None], r.iterations[:, None].astype(np.float64),
                           r.status[:, None].astype(np.float64)], axis=1)


def solve_oracle(inputs, case):
    from oracle import pnec_oracle as po
    key, fam, _, _, kw = case
    offsets, f1, f2, covs, q0, t0 = batch_arrays(inputs[key], fam)
    c9 = None if covs is None else po.covs_to_colmajor9(covs)
    q, t, cost, it, st = po.solve_batch(getattr(po, "MODE_" + fam), offsets, f1, f2, c9, None, 1e-13, q0, t0,
                                        options=po.default_options(**kw))
    return np.concatenate([q, t, np.asarray(cost)[:, None], np.asarray(it, float)[:, None], np.asarray(st, float)[:, None]], axis=1)


def longest_rejection_chain(table, out):
    """A rejected step leaves the point where it was: with the same pair and start, the result at cap k is then the
    result at cap k - 1, bit for bit.  Longest run of such k over the consecutive caps 1 .. 7, over all solves."""
    rows = {(c[0], c[1], c[2], c[3]): i for i, c in enumerate(table)}
    best = 0
    for (key, fam, geom, name), i in rows.items():
        if name != "cap1":
            continue
        run = np.zeros(N_STARTS, dtype=int)
        for k in range(2, 8):
            a, b = out[rows[(key, fam, geom, f"cap{k - 1}")]][:, :8], out[rows[(key, fam, geom, f"cap{k}")]][:, :8]
            same = (a.view(np.uint64) == b.view(np.uint64)).all(axis=1)
            run = np.where(same, run + 1, 0)
            best = max(best, int(run.max()))
    return best


def coverage(table, out):
    return {"longest_rejection_chain": longest_rejection_chain(table, out),
            "longest_rejection_chain_8_1_3": longest_rejection_chain([c for c in table if c[2] == (8, 1, 3)],
                                                                     out[[i for i, c in enumerate(table) if c[2] == (8, 1, 3)]]),
            "status_counts": {int(s): int((out[:, :, 9] == s).sum()) for s in np.unique(out[:, :, 9])}}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--oracle", action="store_true", help="solve on the CPU oracle and print the coverage; writes nothing")
    ap.add_argument("--out", default=FIXTURE)
    ap.add_argument("--commit", default="", help="the commit the library under pnec_amd/ (or PNEC_HIP_LIB) was built from; stored in the fixture")
    a = ap.parse_args()
    inputs = make_inputs()
    table = cases()
    solve = solve_oracle if a.oracle else solve_device
    out = np.ascontiguousarray(np.stack([solve(inputs, c) for c in table]))
    cov = coverage(table, out)
    print(len(table), "cases;", cov)
    assert cov["longest_rejection_chain"] >= 4, cov
    for code in (MAX_ITERATIONS, MIN_RADIUS, INVALID_STEPS):
        assert cov["status_counts"].get(code, 0) > 0, (code, cov)
    if a.oracle:
        return
    import hashlib
    from pnec_amd import capi
    # provenance: which build made the outputs
    arrays = {"out": out, "recorded_on_commit": np.array(a.commit),
              "recorded_lib_sha256": np.array(hashlib.sha256(open(capi.LIB_PATH, "rb").read()).hexdigest())}
    for k, v in inputs.items():
        for p, x in zip(("f1", "f2", "cov6", "q0", "t0"), v):
            arrays[f"{p}_{k}"] = np.ascontiguousarray(x, dtype=np.float64)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    np.savez(a.out, **arrays)
    print(a.out, os.path.getsize(a.out), "bytes")
    assert os.path.getsize(a.out) < 1_000_000


if __name__ == "__main__":
    main()
