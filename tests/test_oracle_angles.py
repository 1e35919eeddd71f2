"""The oracle's AnglesFromVec (common.cc:103-116) at the start vectors where C's acos / atan2 fix
more than a magnitude: signed zeros, the z axis, the phi = +-pi seam, tilts on both sides of the
1e-10 threshold.  The device's start pose is compared with the oracle (tests/test_lm_edges_gpu.py),
so the oracle has to be the reference's behaviour: Python's math.acos / math.atan2 are C's."""
import math

import pytest

PI = math.pi


def _reference(v):
    """common.cc:103-116 in Python floats (the same IEEE operations, C's acos / atan2)"""
    x, y, z = v
    n = math.sqrt(x * x + y * y + z * z)
    if n == 0:
        return 0.0, 0.0
    theta = math.acos(z / n)
    return theta, 0.0 if abs(theta) < 1e-10 else math.atan2(y / n, x / n)


CASES = [
    # +z: theta = 0, phi forced to 0 whatever the signs of x and y
    ((0.0, 0.0, 1.0), 0.0, 0.0), ((-0.0, 0.0, 1.0), 0.0, 0.0), ((0.0, -0.0, 1.0), 0.0, 0.0),
    ((-0.0, -0.0, 1.0), 0.0, 0.0),
    # -z: theta = pi, phi = atan2(+-0, +-0): +-0 or +-pi by the signs
    ((0.0, 0.0, -1.0), PI, 0.0), ((0.0, -0.0, -1.0), PI, -0.0), ((-0.0, 0.0, -1.0), PI, PI),
    ((-0.0, -0.0, -1.0), PI, -PI),
    # the seam: phi = +-pi by the sign of a zero y
    ((-1.0, 0.0, 0.0), PI / 2, PI), ((-1.0, -0.0, 0.0), PI / 2, -PI), ((-2.0, -0.0, 0.5), None, -PI),
    # the y axis
    ((0.0, 1.0, 0.0), PI / 2, PI / 2), ((-0.0, -1.0, 0.0), PI / 2, -PI / 2),
    # zero vector
    ((0.0, 0.0, 0.0), 0.0, 0.0), ((-0.0, -0.0, -0.0), 0.0, 0.0),
    # +-z tilted by 1e-12 / 1e-10 / 1e-8: z / n rounds to +-1 (the smallest theta a double reaches
    # is acos(1 - 2^-53) = 1.05e-8), so theta is exactly 0 or pi and phi follows the signs
    ((1e-12, 0.0, 1.0), 0.0, 0.0), ((-1e-10, -0.0, 1.0), 0.0, 0.0), ((1e-8, 1e-8, 1.0), 0.0, 0.0),
    ((1e-12, 0.0, -1.0), PI, 0.0), ((-1e-10, 0.0, -1.0), PI, PI), ((-1e-8, -0.0, -1.0), PI, -PI),
    ((0.0, -1e-10, -1.0), PI, -PI / 2),
]


@pytest.mark.parametrize("v,theta,phi", CASES, ids=[repr(c[0]) for c in CASES])
def test_oracle_angles_from_vec_follow_c(oracle, v, theta, phi):
    th, ph = oracle.angles_from_vec(v)
    rth, rph = _reference(v)
    # bit for bit, sign of zero included
    assert (th, math.copysign(1.0, th)) == (rth, math.copysign(1.0, rth)), (v, th, rth)
    assert (ph, math.copysign(1.0, ph)) == (rph, math.copysign(1.0, rph)), (v, ph, rph)
    if theta is not None:
        assert th == theta
    assert ph == phi and math.copysign(1.0, ph) == math.copysign(1.0, phi), (v, ph, phi)


def test_smallest_polar_angle_is_above_both_thresholds():
    """theta = acos(z / n) is 0 or at least acos(1 - 2^-53): no double input falls between the
    reference's 1e-10 threshold and 1e-8, so the tilted-axis cases above pin the threshold's
    behaviour completely"""
    assert math.acos(1.0 - 2.0 ** -53) > 1e-8
