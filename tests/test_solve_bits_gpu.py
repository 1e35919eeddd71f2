"""The LM solve, bit for bit, against outputs recorded on the commit BEFORE the kernel began to serve rejected steps from
candidates computed ahead of time in idle quads and dropped the full pass's adds of a literal zero (DESIGN.md section 4,
NOTES/lm-step-speculation.md).  Both changes claim to preserve every bit: the served candidate is made by the same
instructions on the same inputs, and the dropped adds could only turn a -0.0 Jacobian entry into +0.0 in front of sums
that cannot tell.  At the noise floor one rounding difference flips an accept / reject, so the claim is held to
np.array_equal on the raw 8-byte words of q, t and cost, and equality of iterations and status.

tests/golden/solve_bits_parent.npz holds the inputs and the recorded outputs (tools/record_solve_bits.py, which also
owns the case table):
  * pair sizes 1, 5, 63, 64, 65, 128, 129, 320, 321, 511, 512 forced on (8, 1, 3); 513, 600, 768 on the (12, 1, 3) tail;
    1024 on (8, 2, 3) and 5, 65, 129 on the rungs the tuner picks for them: (8, 1, 3) alone serves rejected steps, the
    others run the changed code with the fallbacks compiled out;
  * TARGET and NEC (their evaluation changed) and HOST (its LM step did); four starts per pair, the simulator's own and
    three that are 1 .. 4 degrees off; anisotropic noise at noise_level 1.0, so the solves reject in chains;
  * exactly k iterations for k in 1 .. 7, 10, 25 (the cap lands on a primary step and on each of the three served
    slots; 25 refills the slots after a third served fallback), Ceres-default termination, and a minimum trust-region
    radius of 1e-3, which a fallback's radius crosses;
  * the exactly-zero-residual pair of test_lm_branches.py (invalid steps in every quad, exact +-0 Jacobian entries)
    with max_num_consecutive_invalid_steps 1 and 5.
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_solve_bits as rsb  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    z = np.load(rsb.FIXTURE)
    table = rsb.cases()
    assert z["out"].shape == (len(table), rsb.N_STARTS, 10)
    return table, z["out"], rsb.load_inputs(z)


def test_fixture_reaches_the_paths_it_is_there_for(recorded):
    """the recorded outputs contain a solve with four or more consecutive rejected steps (a rejected step leaves the
    point where it was: equal bits at consecutive caps) and solves ending at the iteration cap, below the minimum
    radius and on consecutive invalid steps"""
    table, out, _ = recorded
    cov = rsb.coverage(table, out)
    assert cov["longest_rejection_chain"] >= 4, cov
    # On (8, 1, 3), the geometry that serves rejected steps: a run of five consecutive rejections inside the caps
    # 2 .. 7, every one of which is a case of its own.  The first of the five is the step computed with its three
    # fallbacks, the next three are the served slots 0, 1, 2 -- a cap lands on each -- and the fifth is computed again
    # after the third served fallback, with a cap on it too; cap 25 runs on through later refills.
    assert cov["longest_rejection_chain_8_1_3"] >= 5, cov
    # which build made the outputs
    z = np.load(rsb.FIXTURE)
    assert len(str(z["recorded_on_commit"])) == 40 and len(str(z["recorded_lib_sha256"])) == 64
    for code in (rsb.MAX_ITERATIONS, rsb.MIN_RADIUS, rsb.INVALID_STEPS):
        assert cov["status_counts"].get(code, 0) > 0, (code, cov)
    # the zero-residual pair ends on its invalid steps after exactly as many iterations as the option allows
    for i, (key, fam, geom, name, kw) in enumerate(table):
        if key == "zero":
            assert (out[i][:, 9] == rsb.INVALID_STEPS).all() and \
                (out[i][:, 8] == kw["max_num_consecutive_invalid_steps"]).all(), (fam, geom, name, out[i][:, 8:])


@pytest.mark.parametrize("family", rsb.FAMILIES)
def test_solve_is_bitwise_the_recorded_one(recorded, family):
    table, out, inputs = recorded
    bad = []
    for i, case in enumerate(table):
        if case[1] != family:
            continue
        got = rsb.solve_device(inputs, case)
        for name, cols in (("q", slice(0, 4)), ("t", slice(4, 7)), ("cost", slice(7, 8)), ("iterations", slice(8, 9)),
                           ("status", slice(9, 10))):
            a, b = np.ascontiguousarray(got[:, cols]), np.ascontiguousarray(out[i][:, cols])
            if not np.array_equal(a.view(np.uint64), b.view(np.uint64)):
                bad.append((case[0], case[2], case[3], name, got[:, 8:].tolist(), out[i][:, 8:].tolist()))
    assert not bad, (len(bad), bad[:8])
