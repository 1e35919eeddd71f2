"""pnec_hip_eight_point and pnec_hip_essential_minimal (NISTER, SEVENPT), bit for bit, against outputs recorded on the
commit BEFORE the two kernels' common phases -- the 45 sums, the cyclic Jacobi in LDS, the 3x3 decomposition after its
sweep loop, the quality term, the quaternion, the helpers and the lane-0 stores -- moved into pnec_essential_shared.hpp
(the sweep loop of the minimal kernel's per-lane decomposition stayed in its file because this test
failed with it moved as a template).  The move claims to preserve every bit of every output, so every field is held to
np.array_equal on its raw words (float64 as int64: a NaN equals itself).

tests/golden/essential_bits_parent.npz holds the inputs and the recorded outputs (tools/record_essential_bits.py, which
also owns the batches): per call one ragged batch of about 30 pairs -- every size from the minimal count to 129 at which
a kernel takes another path, short and empty pairs, the outlier pair, the degenerate scenes of
minimal_solver_population.degenerate, a NaN and an infinite bearing, NISTER pairs with 2, 8 and 10 solutions -- run with
quality "sample" and "all".
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_essential_bits as reb  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    return np.load(reb.FIXTURE)


def test_fixture_says_which_build_made_it_and_reaches_every_status(recorded):
    z = recorded
    assert len(str(z["recorded_on_commit"])) == 40 and len(str(z["recorded_lib_sha256"])) == 64
    assert os.path.getsize(reb.FIXTURE) < 1_000_000
    for call in reb.CALLS:
        sizes = set(np.diff(z[f"{call}_offsets"]).tolist())
        low = {"eight_point": 8, "five_point": 5, "seven_point": 7}[call]
        assert sizes >= {n for n in (5, 6, 7, 8, 9, 10, 15, 16, 17, 63, 64, 65, 129) if n >= low} | {low - 1, 0}, (call, sizes)
        for quality in reb.QUALITIES:
            status = set(z[f"{call}_{quality}_status"].tolist())
            assert status >= {0, 1, 2}, (call, quality, status)                  # OK, TOO_FEW, NOT_FINITE
    assert set(recorded["five_point_sample_n_solutions"].tolist()) >= {2, 4, 6, 8, 10}
    assert set(recorded["seven_point_sample_n_solutions"].tolist()) >= {1, 3}


@pytest.mark.parametrize("quality", reb.QUALITIES)
@pytest.mark.parametrize("call", reb.CALLS)
def test_every_output_is_bitwise_the_recorded_one(recorded, call, quality):
    z = recorded
    labels, offsets = z[f"{call}_labels"], z[f"{call}_offsets"]
    got = reb.run_device(call, quality, offsets, z[f"{call}_f1"], z[f"{call}_f2"])
    bad = []
    for field in reb.FIELDS[call]:
        want = z[f"{call}_{quality}_{field}"]
        assert got[field].shape == want.shape and got[field].dtype == want.dtype, (call, quality, field)
        a, b = reb.bits(got[field]), reb.bits(want)
        for p in range(len(labels)):
            if not np.array_equal(a[p], b[p]):
                bad.append(f"{call} quality={quality} pair {p} ({labels[p]}, {int(offsets[p + 1] - offsets[p])} "
                           f"correspondences) field {field}: got {got[field][p].tolist()}, recorded {want[p].tolist()}")
    assert not bad, f"{len(bad)} differences; the first: " + " | ".join(bad[:4])
