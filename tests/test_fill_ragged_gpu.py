"""pnec_hip_problem_fill_keypoints_ragged on the device against existing machinery.

The reference of a device-shaped batch is a host-shaped batch of the SAME BOUNDS filled with pnec_hip_problem_fill_keypoints
-- every pair's real rows followed by filler rows up to its bound -- and then pnec_hip_problem_select with the real rows
marked: a batch with the same block layout, the same counts, the same compacted contents and the same launch geometries
(both follow the bounds).  The arithmetic per correspondence is the same function (unscented_core) and the later stages
see identical planes under identical geometries, so everything is compared BITWISE: the per-pair planes, cost_function,
solve, solve_pipeline with its inlier mask, residuals.  Which rows a pair takes is numpy's (shape_np,
tests/test_fill_ragged_cpu.py).  The oracle comparison holds the device-shaped batch's solve to the bounds
tests/test_parity_gpu.py applies to ragged batches (_ragged_case: status and iterations equal, rotations within 1e-8 rad,
for pairs of at least 63 correspondences)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_fill_ragged_cpu import shape_np  # noqa: E402
from test_ingest_reference_cpu import NUM_PLANES, block_layout, round_up64  # noqa: E402
from test_lm_edges_gpu import _oracle_opts  # noqa: E402
from test_parity_gpu import _oracle_batch, _quat_to_R, _rot_err  # noqa: E402

from pnec_amd import Batch, capi  # noqa: E402
from pnec_amd.multi import alloc_counters  # noqa: E402

pytestmark = pytest.mark.gpu

COUNTS = [0, 1, 63, 64, 65, 257]
UNIFORM = [320] * 6
MODES = [capi.MODE_NEC, capi.MODE_TARGET, capi.MODE_HOST, capi.MODE_SYM]
MODE_IDS = ["nec", "target", "host", "sym"]
K = np.array([[300.0, 0.0, 320.0], [0.0, 300.0, 240.0], [0.0, 0.0, 1.0]])
K_INV = np.linalg.inv(K)


def _torch():
    import torch
    return torch


def _t(a):
    return None if a is None else _torch().as_tensor(np.ascontiguousarray(a), device="cuda:0")


def _quat(rotvec):
    a = np.linalg.norm(rotvec)
    return np.concatenate([rotvec / a * np.sin(a / 2), [np.cos(a / 2)]]) if a > 0 else np.array([0.0, 0.0, 0.0, 1.0])


def _off(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def scene(seed, counts):
    """Keypoint rows of len(counts) frame pairs, pair after pair: a cloud in front of camera 1 seen again from a camera
    moved by (R, t) (X1 = R X2 + t), pixels with 0.3 px noise in frame 2, 2x2 covariances; and a start pose near the
    truth per pair.  -> dict of numpy arrays: p1, p2 [R,2], c2, c1 [R,3], q0 [P,4], t0 [P,3]"""
    rng = np.random.default_rng(seed)
    p1, p2, q0, t0 = [], [], [], []
    for n in counts:
        w = rng.normal(size=3) * 0.03
        R = _quat_to_R(_quat(w))
        t = rng.normal(size=3)
        t *= 0.3 / np.linalg.norm(t)
        X1 = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(4, 10, n)], -1)
        X2 = (X1 - t) @ R
        px = lambda X: (X[:, :2] / X[:, 2:]) * 300.0 + np.array([320.0, 240.0])
        p1.append(px(X1))
        p2.append(px(X2) + rng.normal(size=(n, 2)) * 0.3)
        q0.append(_quat(w + rng.normal(size=3) * 0.005))
        ts = t / np.linalg.norm(t) + rng.normal(size=3) * 0.02
        t0.append(ts / np.linalg.norm(ts))
    M = int(np.sum(counts))

    def spd():
        xx, yy = rng.uniform(0.05, 0.4, M), rng.uniform(0.05, 0.4, M)
        return np.stack([xx, rng.uniform(-0.4, 0.4, M) * np.sqrt(xx * yy), yy], -1)
    return dict(p1=np.concatenate(p1), p2=np.concatenate(p2), c2=spd(), c1=spd(), q0=np.array(q0), t0=np.array(t0))


def _covs(mode, d, rows=slice(None)):
    c2 = None if mode == capi.MODE_NEC else d["c2"][rows]
    c1 = d["c1"][rows] if mode == capi.MODE_SYM else None
    return c2, c1


def dev_batch(mode, bounds, offsets, d, on_device=True, dropped=None):
    """the device-shaped batch: capacity, ONE reshape to the bounds, the ragged fill"""
    conv = _t if on_device else (lambda a: a)
    b = Batch.with_capacity(mode, len(bounds), int(np.sum(bounds)))
    b.reshape(_off(bounds))
    c2, c1 = _covs(mode, d)
    b.fill_keypoints_ragged(conv(np.asarray(offsets, dtype=np.int64)), conv(d["p1"]), conv(d["p2"]), conv(c2), conv(c1),
                            K_inv=K_INV, dropped=dropped)
    return b


def ref_batch(mode, bounds, offsets, d, filler):
    """the reference: a host-shaped batch of the same bounds, each pair's rows (shape_np) + filler up to the bound, filled
    with fill_keypoints, then select() with the real rows marked"""
    lo, cnt, _, _ = shape_np(offsets, len(d["p1"]), bounds)
    boff = _off(bounds)
    rows = {k: np.array(filler[k][:boff[-1]]) for k in ("p1", "p2", "c2", "c1")}
    mask = np.zeros(int(boff[-1]), dtype=np.uint8)
    for p in range(len(bounds)):
        for k in rows:
            rows[k][boff[p]:boff[p] + cnt[p]] = d[k][lo[p]:lo[p] + cnt[p]]
        mask[boff[p]:boff[p] + cnt[p]] = 1
    src = Batch(mode, boff)
    c2, c1 = _covs(mode, rows)
    src.fill_keypoints(rows["p1"], rows["p2"], c2, c1, K_inv=K_INV)
    out = src.select(mask)
    src.close()
    return out


def pair_slices(mode, bounds, cnt, payload):
    start, _, total = block_layout(mode, _off(bounds))
    assert len(payload) == total
    nc = NUM_PLANES[mode]
    return [np.asarray(payload[start[p]:start[p] + nc * round_up64(cnt[p])]) for p in range(len(bounds))]


def same_bits(a, b, what):
    if hasattr(a, "cpu"):
        a = a.cpu().numpy()
    if hasattr(b, "cpu"):
        b = b.cpu().numpy()
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"{what}: bits differ in {int((a != b).sum())} entries"


def assert_batches_agree(mode, bounds, cnt, dev, ref, q0, t0, what):
    """payload per pair, then the stages while both batches are still lazy, then the calls that fetch the sizes"""
    got, want = pair_slices(mode, bounds, cnt, dev.export_payload()), pair_slices(mode, bounds, cnt, ref.export_payload())
    for p in range(len(bounds)):
        same_bits(got[p], want[p], f"{what}: planes of pair {p}")
    tq, tt = _t(q0), _t(t0)
    a, b = dev.solve(tq, tt), ref.solve(tq, tt)
    for k in ("q", "t", "cost", "iterations", "status"):
        same_bits(getattr(a, k), getattr(b, k), f"{what}: solve.{k}")
    if mode == capi.MODE_TARGET:
        same_bits(dev.cost_function(tq, tt), ref.cost_function(tq, tt), f"{what}: cost_function")
        pa, pb = dev.solve_pipeline(tq, tt, want_inliers=True), ref.solve_pipeline(tq, tt, want_inliers=True)
        for k, x, y in zip(("q", "t", "inlier_mask", "inlier_count"), pa, pb):
            same_bits(x, y, f"{what}: solve_pipeline.{k}")
    assert np.array_equal(dev.offsets, _off(cnt)) and np.array_equal(ref.offsets, _off(cnt)), what
    assert dev.num_correspondences == int(np.sum(cnt)) and dev.max_correspondences == int(np.max(cnt))
    ra, rb = dev.residuals(q0, t0), ref.residuals(q0, t0)
    for k in ("residual", "variance", "mask", "chi2", "gated_chi2", "gated_count", "max_abs", "offsets"):
        same_bits(getattr(ra, k), getattr(rb, k), f"{what}: residuals.{k}")
    return a


@pytest.fixture(scope="module")
def world():
    return dict(d=scene(101, COUNTS), filler=scene(202, UNIFORM))


@pytest.mark.parametrize("bounds", [UNIFORM, COUNTS], ids=["bound320", "bound_is_count"])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_device_shaped_batch_has_the_bits_of_fill_keypoints_and_select(world, mode, bounds):
    d = world["d"]
    offsets = _off(COUNTS)
    dev, ref = dev_batch(mode, bounds, offsets, d), ref_batch(mode, bounds, offsets, d, world["filler"])
    assert_batches_agree(mode, bounds, COUNTS, dev, ref, d["q0"], d["t0"], f"{MODE_IDS[mode]} bounds {bounds[:2]}..")
    dev.close()
    ref.close()


def test_a_pair_beyond_its_bound_and_rows_beyond_n_rows_follow_the_numpy_rule(world):
    """bound 64 with 100 rows offered, and offsets that run past n_rows: the counts, what was dropped and the planes"""
    torch = _torch()
    bounds, offsets = [64, 64, 64, 64], [0, 100, 130, 170, 400]
    d = {k: v[:200] for k, v in scene(303, [200]).items() if k in ("p1", "p2", "c2", "c1")}
    lo, cnt, dropped, own = shape_np(offsets, 200, bounds)
    assert cnt.tolist() == [64, 30, 40, 30] and dropped.tolist() == [36, 0, 0, 0]
    mode = capi.MODE_TARGET
    got_dropped = torch.full((4,), -7, dtype=torch.int32, device="cuda:0")
    dev = dev_batch(mode, bounds, offsets, d, dropped=got_dropped)
    ref = ref_batch(mode, bounds, offsets, d, world["filler"])
    assert np.array_equal(got_dropped.cpu().numpy(), dropped)
    s = scene(304, [4] * 4)
    assert_batches_agree(mode, bounds, cnt, dev, ref, s["q0"], s["t0"], "beyond the bound")
    assert np.array_equal(dev.offsets, own)
    dev.close()
    ref.close()


@pytest.mark.parametrize("mode", [capi.MODE_TARGET, capi.MODE_SYM], ids=["target", "sym"])
def test_host_space_equals_device_space(world, mode):
    d, offsets = world["d"], _off(COUNTS)
    dd, dh = np.full(6, -7, dtype=np.int32), np.full(6, -7, dtype=np.int32)
    on_dev = dev_batch(mode, UNIFORM, offsets, d, dropped=_t(dd))
    on_host = dev_batch(mode, UNIFORM, offsets, d, on_device=False, dropped=dh)
    assert (dh == 0).all()
    for p, (a, b) in enumerate(zip(pair_slices(mode, UNIFORM, COUNTS, on_dev.export_payload()),
                                   pair_slices(mode, UNIFORM, COUNTS, on_host.export_payload()))):
        same_bits(a, b, f"HOST vs DEVICE space, pair {p}")
    assert np.array_equal(on_host.offsets, on_dev.offsets)
    a, b = on_dev.solve(d["q0"], d["t0"]), on_host.solve(d["q0"], d["t0"])
    for k in ("q", "t", "cost", "iterations", "status"):
        same_bits(getattr(a, k), getattr(b, k), f"HOST vs DEVICE space: solve.{k}")
    # HOST space validates what it reads
    for bad in ([0, 5, 3, 9, 9, 9, 9], [0, 0, 1, 64, 128, 193, 451], [-1, 0, 1, 64, 128, 193, 450]):
        with pytest.raises(capi.PnecHipError) as ei:
            c2, c1 = _covs(mode, d)
            on_host.fill_keypoints_ragged(np.array(bad, dtype=np.int64), d["p1"], d["p2"], c2, c1, K_inv=K_INV)
        assert ei.value.code == capi.ERR_INVALID_ARGUMENT
    on_dev.close()
    on_host.close()


def test_refusals(world):
    d, L = world["d"], capi.lib()
    exact = Batch(capi.MODE_TARGET, _off(COUNTS))
    cap = Batch.with_capacity(capi.MODE_TARGET, 6, 2000).reshape(_off(UNIFORM))
    nec = Batch.with_capacity(capi.MODE_NEC, 6, 2000).reshape(_off(UNIFORM))
    sym = Batch.with_capacity(capi.MODE_SYM, 6, 2000).reshape(_off(UNIFORM))
    off, p1, p2, c2, c1, Kd = (_t(a) for a in (_off(COUNTS), d["p1"], d["p2"], d["c2"], d["c1"], K_INV.T.reshape(9)))
    R = len(d["p1"])
    ptr = lambda a: None if a is None else a.data_ptr()

    def rc(b, o=off, cov2=c2, cov1=None, k=Kd, model=1, space=capi.MEM_DEVICE):
        return L.pnec_hip_problem_fill_keypoints_ragged(b._h, ptr(o), R, ptr(p1), ptr(p2), ptr(cov2), ptr(cov1), ptr(k), 1.0,
                                                        model, None, space, None)
    assert rc(cap) == 0
    assert rc(exact) == capi.ERR_INVALID_ARGUMENT and b"capacity" in L.pnec_hip_last_error()
    assert rc(cap, o=None) == capi.ERR_INVALID_ARGUMENT and rc(cap, k=None) == capi.ERR_INVALID_ARGUMENT
    assert rc(cap, cov2=None) == capi.ERR_INVALID_ARGUMENT and rc(cap, cov1=c1) == capi.ERR_INVALID_ARGUMENT
    assert rc(nec) == capi.ERR_INVALID_ARGUMENT and rc(nec, cov2=None) == 0
    assert rc(sym) == capi.ERR_INVALID_ARGUMENT and rc(sym, cov1=c1) == 0
    assert rc(cap, model=0) == capi.ERR_INVALID_ARGUMENT and rc(cap, space=7) == capi.ERR_INVALID_ARGUMENT
    _torch().cuda.synchronize()
    for b in (exact, cap, nec, sym):
        b.close()


def test_one_pair_alone_equals_the_same_pair_in_the_batch(world):
    d, mode, p = world["d"], capi.MODE_TARGET, 5
    offsets = _off(COUNTS)
    whole = dev_batch(mode, UNIFORM, offsets, d)
    alone = dev_batch(mode, [UNIFORM[p]], offsets[p:p + 2], d)     # (the same rows, addressed by the pair's own offsets)
    same_bits(pair_slices(mode, [UNIFORM[p]], [COUNTS[p]], alone.export_payload())[0],
              pair_slices(mode, UNIFORM, COUNTS, whole.export_payload())[p], "planes")
    a, b = whole.solve(_t(d["q0"]), _t(d["t0"])), alone.solve(_t(d["q0"][p:p + 1]), _t(d["t0"][p:p + 1]))
    for k in ("q", "t", "cost", "iterations", "status"):
        same_bits(getattr(a, k)[p:p + 1], getattr(b, k), f"solve.{k}")
    assert alone.offsets.tolist() == [0, COUNTS[p]]
    whole.close()
    alone.close()


def test_reshape_afterwards_gives_an_exact_batch_and_a_second_call_allocates_nothing(world):
    torch = _torch()
    d, mode = world["d"], capi.MODE_TARGET
    offsets = _off(COUNTS)
    tq, tt = _t(d["q0"]), _t(d["t0"])
    other = scene(404, [64, 0, 300, 17, 1, 320])
    oo = _t(_off([64, 0, 300, 17, 1, 320]))
    dev_rows = [_t(other[k]) for k in ("p1", "p2", "c2")]
    Kd = _t(K_INV)
    b = dev_batch(mode, UNIFORM, offsets, d)
    b.solve_pipeline(tq, tt)                       # (first use of the chain's scratch, views and mask)
    b.fill_keypoints_ragged(oo, *dev_rows, K_inv=Kd)
    b.solve_pipeline(tq, tt)
    torch.cuda.synchronize()
    first = alloc_counters()
    for off_t, rows in ((_t(offsets), [_t(d[k]) for k in ("p1", "p2", "c2")]), (oo, dev_rows)):
        a0 = alloc_counters()
        b.fill_keypoints_ragged(off_t, *rows, K_inv=Kd)
        a1 = alloc_counters()             # the call itself: no hipMalloc, no block taken from or returned to the cache
        assert (a1["hip_malloc_calls"], a1["cache_hits"], a1["live_blocks"]) == \
               (a0["hip_malloc_calls"], a0["cache_hits"], a0["live_blocks"]), (a0, a1)
        q, t = b.solve_pipeline(tq, tt)
    torch.cuda.synchronize()
    assert alloc_counters()["hip_malloc_calls"] == first["hip_malloc_calls"]      # ... and none in the chain behind it
    # the second shape is what the batch now holds, compared with a fresh device-shaped batch
    fresh = dev_batch(mode, UNIFORM, _off([64, 0, 300, 17, 1, 320]), other)
    qf, tf = fresh.solve_pipeline(tq, tt)
    same_bits(q, qf, "pipeline q after re-use")
    same_bits(t, tf, "pipeline t after re-use")
    assert b.offsets.tolist() == _off([64, 0, 300, 17, 1, 320]).tolist()       # (materialises: host sizes are exact now)
    # a ragged call after the sizes were fetched finds the bounds again
    b.fill_keypoints_ragged(_t(offsets), _t(d["p1"]), _t(d["p2"]), _t(d["c2"]), K_inv=Kd)
    for p, (x, y) in enumerate(zip(pair_slices(mode, UNIFORM, COUNTS, b.export_payload()),
                                   pair_slices(mode, UNIFORM, COUNTS, dev_batch(mode, UNIFORM, offsets, d).export_payload()))):
        same_bits(x, y, f"after materialise, pair {p}")
    assert b.offsets.tolist() == offsets.tolist()
    # reshape: an exact batch again -- the host-side sizes, the planes and the solve of a batch created with that shape
    gen_probe = Batch(mode, offsets)
    gen_probe.fill_keypoints(d["p1"], d["p2"], d["c2"], K_inv=K_INV)
    b.reshape(offsets)
    assert b.num_correspondences == int(offsets[-1]) and b.max_correspondences == max(COUNTS)
    assert b.describe_launch() == gen_probe.describe_launch()
    b.fill_keypoints(d["p1"], d["p2"], d["c2"], K_inv=K_INV)
    same_bits(b.export_payload(), gen_probe.export_payload(), "payload after reshape")
    x, y = b.solve(d["q0"], d["t0"]), gen_probe.solve(d["q0"], d["t0"])
    for k in ("q", "t", "cost", "iterations", "status"):
        same_bits(getattr(x, k), getattr(y, k), f"after reshape: solve.{k}")
    px, py = b.solve_pipeline(d["q0"], d["t0"], want_inliers=True), gen_probe.solve_pipeline(d["q0"], d["t0"], want_inliers=True)
    for k, u, v in zip(("q", "t", "mask", "count"), px, py):
        same_bits(u, v, f"after reshape: pipeline.{k}")
    for z in (b, fresh, gen_probe):
        z.close()


def test_the_call_respects_stream_order_on_a_side_stream(world):
    from test_stream_order_gpu import Entry, _export_payload, check
    torch = _torch()
    mode, n_rows = capi.MODE_TARGET, int(np.sum(UNIFORM))
    b = Batch.with_capacity(mode, 6, n_rows).reshape(_off(UNIFORM))
    Kd = _t(K_INV)
    q0, t0 = _t(world["d"]["q0"]), _t(world["d"]["t0"])

    def data(seed, counts):
        s = scene(seed, counts)
        pad = n_rows - len(s["p1"])
        grow = lambda a: np.concatenate([a, np.full((pad,) + a.shape[1:], 1.0)])
        return dict(off=_t(_off(counts)), p1=_t(grow(s["p1"])), p2=_t(grow(s["p2"])), c2=_t(grow(s["c2"])))
    base = data(501, UNIFORM)                         # (fills every block to its bound: what a call leaves alone is known)
    dropped = torch.zeros((6,), dtype=torch.int32, device="cuda:0")

    def call(bufs):
        b.fill_keypoints_ragged(bufs["off"], bufs["p1"], bufs["p2"], bufs["c2"], K_inv=Kd, dropped=dropped)
        return [_export_payload(b), dropped, b.cost_function(q0, t0)], b

    def reset():
        b.fill_keypoints_ragged(base["off"], base["p1"], base["p2"], base["c2"], K_inv=Kd)
    check(Entry(data(502, COUNTS), data(503, [257, 65, 0, 64, 1, 63]), call, reset=reset, sentinels=[dropped]),
          "fill_keypoints_ragged")
    b.close()


def test_device_shaped_target_batch_agrees_with_the_oracle_on_the_same_bearings(world, oracle):
    d, mode = world["d"], capi.MODE_TARGET
    offsets = _off(COUNTS)
    dev = dev_batch(mode, UNIFORM, offsets, d)
    opts = capi.default_options()
    res = dev.solve(d["q0"], d["t0"], options=opts)
    planes = pair_slices(mode, UNIFORM, COUNTS, dev.export_payload())
    f1, f2, c2 = [], [], []
    for p, n in enumerate(COUNTS):
        blk = planes[p].reshape(12, round_up64(n))[:, :n]
        f1.append(blk[0:3].T)
        f2.append(blk[3:6].T)
        xx, xy, xz, yy, yz, zz = blk[6:12]
        c2.append(np.stack([np.stack([xx, xy, xz], -1), np.stack([xy, yy, yz], -1), np.stack([xz, yz, zz], -1)], -2))
    f1, f2, c2 = np.concatenate(f1), np.concatenate(f2), np.concatenate(c2)
    assert np.abs(np.linalg.norm(f1, axis=1) - 1).max() < 1e-14 and f1.shape == (int(offsets[-1]), 3)
    q, t, cost, it, st = _oracle_batch(oracle, mode, offsets, f1, f2, c2, None, 1e-13, d["q0"], d["t0"],
                                       _oracle_opts(oracle, opts, oracle.JAC_ANALYTIC))
    checked = 0
    for p, n in enumerate(COUNTS):
        if n >= 63:    # (test_parity_gpu._ragged_case: tiny pairs are rank-deficient, any LM wanders)
            assert res.status[p] == st[p] and res.iterations[p] == it[p], n
            assert _rot_err(oracle, _quat_to_R(res.q[p]), _quat_to_R(q[p])) <= 1e-8, n
            checked += 1
    assert checked == 4
    assert np.isfinite(res.q).all() and np.isfinite(res.t).all()
    dev.close()
