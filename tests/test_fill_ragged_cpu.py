"""pnec_hip_problem_fill_keypoints_ragged, Batch.fill_keypoints_ragged and pnec_amd.Odometry without a GPU: the symbol is
declared, bound and exported within ABI 8; the Python names exist with their documented defaults; the shaping rule
(include/pnec_hip.h) is stated in numpy -- `shape_np`, which tests/test_fill_ragged_gpu.py holds the device to -- and
checked on hand-made cases; the one refusal that needs no device (a NULL batch: no batch exists without a device)."""
import inspect
import os
import re

import numpy as np

import pnec_amd
from pnec_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "pnec_hip_problem_fill_keypoints_ragged"


def shape_np(offsets, n_rows, bounds):
    """The shaping rule: -> (lo [P] first row taken, cnt [P] rows taken, dropped [P] rows the bound turned away,
    own [P+1] the batch's compact offsets).  offsets int64 [P+1] as given (anything), bounds [P] >= 0."""
    offsets = np.asarray(offsets, dtype=np.int64)
    bounds = np.asarray(bounds, dtype=np.int64)
    lo = np.clip(offsets[:-1], 0, n_rows)
    hi = np.minimum(np.maximum(offsets[1:], lo), n_rows)
    cnt = np.minimum(hi - lo, np.maximum(bounds, 0))
    own = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    return lo, cnt.astype(np.int32), (hi - lo - cnt).astype(np.int32), own


def test_the_symbol_is_declared_bound_and_exported_within_abi_8():
    header = open(os.path.join(ROOT, "include", "pnec_hip.h")).read()
    m = re.search(r"\bint " + NAME + r"\(([^;]*)\);", header)
    assert m, "not declared in include/pnec_hip.h"
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    assert len(args) == 13 and args[0] == "pnec_hip_problem *p" and args[1] == "const int64_t *offsets" and \
        args[2] == "int64_t n_rows" and args[10] == "int32_t *out_dropped" and args[11] == "int space"
    assert re.search(r"#define PNEC_HIP_ABI_VERSION 8\b", header) and capi.ABI_VERSION == 8
    assert NAME in capi.SYMBOLS
    L = capi.lib()
    assert L.pnec_hip_abi_version() == 8
    f = getattr(L, NAME)
    assert len(f.argtypes) == 13


def test_the_python_names_exist_with_their_defaults():
    assert {"Odometry", "OdometryResult"} <= set(pnec_amd.__all__) and pnec_amd.Odometry is pnec_amd.odometry.Odometry
    sig = inspect.signature(pnec_amd.Batch.fill_keypoints_ragged)
    assert list(sig.parameters) == ["self", "offsets", "pts1", "pts2", "cov2", "cov1", "K_inv", "kappa", "dropped"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["cov2"], d["cov1"], d["K_inv"], d["kappa"], d["dropped"]) == (None, None, None, 1.0, None)
    sig = inspect.signature(pnec_amd.Odometry.__init__)
    assert list(sig.parameters)[:7] == ["self", "n_sequences", "height", "width", "K_inv", "mode", "pipeline_options"]
    assert sig.parameters["mode"].default == capi.MODE_TARGET and sig.parameters["pipeline_options"].default is None
    assert any(p.kind is inspect.Parameter.VAR_KEYWORD for p in sig.parameters.values())      # **tracker_kwargs
    assert callable(pnec_amd.Odometry.process)
    assert [f for f in pnec_amd.OdometryResult.__dataclass_fields__][:4] == ["q", "t", "n_corr", "pairs"]


def test_the_shaping_rule_on_hand_made_cases():
    # within the bounds: the counts are the differences, nothing dropped, the batch's own offsets are the given ones
    lo, cnt, dropped, own = shape_np([0, 0, 1, 64, 128, 193, 450], 450, [320] * 6)
    assert lo.tolist() == [0, 0, 1, 64, 128, 193] and cnt.tolist() == [0, 1, 63, 64, 65, 257]
    assert dropped.tolist() == [0] * 6 and own.tolist() == [0, 0, 1, 64, 128, 193, 450]
    # a pair beyond its bound keeps its FIRST rows; the next pair still starts at its own offset; own offsets compact
    lo, cnt, dropped, own = shape_np([0, 100, 130], 130, [64, 64])
    assert lo.tolist() == [0, 100] and cnt.tolist() == [64, 30] and dropped.tolist() == [36, 0] and own.tolist() == [0, 64, 94]
    # rows beyond n_rows do not exist: the range is cut first, the bound applies to what is left
    lo, cnt, dropped, own = shape_np([0, 100, 130, 200], 120, [64, 64, 64])
    assert lo.tolist() == [0, 100, 120] and cnt.tolist() == [64, 20, 0] and dropped.tolist() == [36, 0, 0]
    assert own.tolist() == [0, 64, 84, 84]
    # a step down, a negative start: an empty pair, never a negative count
    lo, cnt, dropped, own = shape_np([-5, 10, 4, 9], 50, [8, 8, 8])
    assert lo.tolist() == [0, 10, 4] and cnt.tolist() == [8, 0, 5] and dropped.tolist() == [2, 0, 0] and own.tolist() == [0, 8, 8, 13]
    # a zero bound takes nothing
    lo, cnt, dropped, own = shape_np([0, 3, 7], 7, [0, 4])
    assert cnt.tolist() == [0, 4] and dropped.tolist() == [3, 0] and own.tolist() == [0, 0, 4]


def test_a_null_batch_is_refused_before_any_device_is_touched():
    L = capi.lib()
    off = np.zeros(2, dtype=np.int64)
    K = np.eye(3).reshape(9)
    for space in (capi.MEM_HOST, capi.MEM_DEVICE):
        rc = L.pnec_hip_problem_fill_keypoints_ragged(None, off.ctypes.data, 0, None, None, None, None, K.ctypes.data, 1.0, 1,
                                                      None, space, None)
        assert rc == capi.ERR_INVALID_ARGUMENT and NAME.encode() in L.pnec_hip_last_error()
