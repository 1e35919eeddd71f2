"""Stream order of every DEVICE-space entry point on a NON-DEFAULT stream.

include/pnec_hip.h documents every DEVICE-space call as "asynchronous on `stream`".  Every other GPU test calls the
library under torch's default stream -- the null stream, which every blocking stream synchronises with implicitly -- so a
launch that drops its stream argument, a forked side stream that is not joined back, scratch reset on the wrong stream or
a hidden host synchronisation changes nothing there.  Here every call runs on a non-blocking side stream `S`, held
behind a 50 ms device-side delay, with its inputs arriving ON `S` only after that delay:

  default stream   want = E(good), want_decoy = E(decoy)           (they must differ: a probe needs power)
  stream S         delay | gate | inputs <- good | E | got <- outputs | inputs <- decoy
                   ... and the host notes, right after E returns, whether the gate has fired yet

The input buffers hold the DECOY (valid data of the same shape from another seed) before and after that window, so a call
that reads early -- on another stream, or on the host -- or late -- from a fork it never joined -- computes the decoy's
result.  `got` must equal `want` BITWISE (floats compared as int64 patterns), only `S` is waited for, and a call the
header documents as asynchronous must have returned while the delay was still running.

The reference of every probe is the same call on the default stream; that call's agreement with the oracle is what
test_parity_gpu.py, test_residuals_gpu.py, test_pose_covariance_gpu.py, test_triangulate_gpu.py,
test_relative_scale_gpu.py, test_ingest_edges_gpu.py and test_patch_covariance_gpu.py pin.

The delay is not a tolerance: a correct library passes for any delay; it only has to outlast the host side of a warmed
call (under 1 ms per enqueued step by INTEGRATION.md's lockstep figure).
"""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from pnec_amd import Batch, capi
from pnec_amd import simulation as sim
from pnec_amd.batch import SolveResult, select_best

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DELAY_MS = 50.0
RAGGED = [0, 5, 37, 64, 300, 513, 1100, 2100, 4100, 5000]
SMALL = [5, 64, 513, 1100]
WIDE = [12 + i % 29 for i in range(1024)]            # 1024 pairs: the smallest batch whose chain forks the RANSAC tail
F_SENTINEL, I_SENTINEL = 12345.678, 77
RANSAC_IT = 300                                      # stage calls: hypotheses per pair (the chain keeps its default)


# ------------------------------------------------------------------------------------------------ the probe
_cycles_per_ms = None
_mm = None


def _spin(n):
    import torch
    if hasattr(torch.cuda, "_sleep"):
        torch.cuda._sleep(int(n))
    else:
        for _ in range(int(n)):
            torch.mm(_mm, _mm)


def _delay(ms):
    """`ms` of device time on the current stream: torch.cuda._sleep calibrated once per module with two events (a chain
    of matrix products timed the same way where that helper is missing)."""
    import torch
    global _cycles_per_ms, _mm
    spin = _spin
    if _cycles_per_ms is None:
        if not hasattr(torch.cuda, "_sleep"):
            _mm = torch.ones((1024, 1024), device="cuda")
        unit = 2_000_000 if hasattr(torch.cuda, "_sleep") else 20
        spin(unit)                                   # (first use)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        spin(unit)
        b.record()
        torch.cuda.synchronize()
        _cycles_per_ms = unit / max(a.elapsed_time(b), 1e-3)
        a.record()
        spin(_cycles_per_ms * DELAY_MS)
        b.record()
        torch.cuda.synchronize()
        print(f"stream-order probe: a delay of {DELAY_MS} ms asked for runs {a.elapsed_time(b):.1f} ms")
    if ms > 0:
        spin(max(1, _cycles_per_ms * ms))


def _bits(t):
    """The tensor's bit patterns where it is floating point (a NaN equals itself, payload included)."""
    import torch
    t = t.contiguous()
    if t.dtype == torch.float64:
        return t.view(torch.int64)
    if t.dtype == torch.float32:
        return t.view(torch.int32)
    return t


def _same(a, b):
    import torch
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(_bits(a), _bits(b)))


class Entry:
    """One entry point as the probe sees it.  good / decoy: dicts of device tensors (the call's device inputs);
    call(bufs) enqueues the call on the CURRENT stream with the inputs taken from `bufs` and returns (outputs, keep) --
    `keep` holds whatever must not be destroyed before the stream has drained; reset() (optional, default stream) puts
    state the call changes back; sentinels: caller-supplied output buffers, filled before each run."""

    def __init__(self, good, decoy, call, reset=None, sentinels=()):
        self.good, self.decoy, self.call, self.reset, self.sentinels = good, decoy, call, reset, list(sentinels)


class Report:
    def __init__(self):
        self.mismatch, self.late_mismatch, self.returned_early, self.host_ms = [], [], None, None
        self.got, self.live = None, None


def _prepare(entry):
    import torch
    if entry.reset is not None:
        entry.reset()
    for s in entry.sentinels:
        s.fill_(I_SENTINEL if not s.dtype.is_floating_point else F_SENTINEL)
    torch.cuda.synchronize()


def _on_default_stream(entry, bufs, data):
    import torch
    _prepare(entry)
    for k, v in data.items():
        bufs[k].copy_(v)
    outs, keep = entry.call(bufs)
    outs = [o.clone() for o in outs]
    torch.cuda.synchronize()
    del keep
    return outs


def probe(entry, want=None, delay_ms=DELAY_MS):
    """-> Report.  `want`: the reference outputs when they come from elsewhere (the forced-chunk child processes)."""
    import torch
    _delay(0)                                        # (calibrates on first use, outside every timed window)
    bufs = {k: v.clone() for k, v in entry.decoy.items()}
    # 1. warm-up and power check, default stream
    if want is None:
        want = _on_default_stream(entry, bufs, entry.good)
    want_decoy = _on_default_stream(entry, bufs, entry.decoy)
    assert len(want) == len(want_decoy) and any(not _same(a, b) for a, b in zip(want, want_decoy)), \
        "the decoy gives the same bits as the good data: this probe proves nothing"
    S = torch.cuda.Stream()

    def enqueue(ms, rep):
        _prepare(entry)
        for k, v in entry.decoy.items():             # 2. the buffers hold the decoy
            bufs[k].copy_(v)
        torch.cuda.synchronize()
        with torch.cuda.stream(S):                   # 3.
            if ms:
                _delay(ms)
            gate = torch.cuda.Event()
            gate.record()
            for k, v in entry.good.items():
                bufs[k].copy_(v)
            t0 = time.perf_counter()
            outs, keep = entry.call(bufs)
            rep.host_ms = (time.perf_counter() - t0) * 1e3
            rep.returned_early = not gate.query()
            got = [o.clone() for o in outs]
            for k, v in entry.decoy.items():
                bufs[k].copy_(v)
        S.synchronize()                              # 4. S alone
        return got, outs, keep

    warm = Report()
    got, outs, keep = enqueue(0, warm)               # first-use allocations, table uploads, stream pools
    torch.cuda.synchronize()
    del got, outs, keep
    rep = Report()
    got, outs, keep = enqueue(delay_ms, rep)
    rep.got = got
    rep.mismatch = [i for i, (a, b) in enumerate(zip(got, want)) if not _same(a, b)]   # 5.
    # what the outputs hold once EVERY stream has drained: a fork that was never joined writes them after `got` was taken
    torch.cuda.synchronize()
    rep.live = [o.clone() for o in outs]
    rep.late_mismatch = [i for i, (a, b) in enumerate(zip(rep.live, want)) if not _same(a, b)]
    torch.cuda.synchronize()
    del keep
    rep.want, rep.want_decoy = want, want_decoy
    return rep


def check(entry, name, want=None, asynchronous=True):
    rep = probe(entry, want)
    print(f"stream-order probe {name}: host side of the call {rep.host_ms:.3f} ms, returned_early={rep.returned_early}, "
          f"mismatching outputs {rep.mismatch}, after a device-wide wait {rep.late_mismatch}")
    assert not rep.mismatch, f"{name}: outputs {rep.mismatch} differ from the default-stream call's bits"
    assert not rep.late_mismatch, f"{name}: outputs {rep.late_mismatch} were written again after the stream had drained"
    if asynchronous:
        assert rep.returned_early, (f"{name}: documented as asynchronous, but the call returned only after the work queued "
                                    f"ahead of it on the stream had run ({rep.host_ms:.1f} ms on the host)")
    return rep


# ------------------------------------------------------------------------------------------------ data
def _ragged(sizes, seed, outliers):
    """Reference-layout arrays of a ragged batch from sim.generate, a share `outliers` of bvs2 replaced by random unit
    vectors (gross mismatches), and the start poses: numpy."""
    sizes = np.asarray(sizes, dtype=np.int64)
    g = sim.generate(len(sizes), int(max(sizes.max(), 1)), seed=seed)
    cat = lambda a: np.concatenate([a[p, :n].numpy() for p, n in enumerate(sizes)]).copy()
    f1, f2, cv = cat(g.bvs1), cat(g.bvs2), cat(g.covs2)
    rng = np.random.default_rng(seed)
    bad = rng.random(len(f2)) < outliers
    v = rng.normal(size=(int(bad.sum()), 3))
    f2[bad] = v / np.linalg.norm(v, axis=1, keepdims=True)
    return dict(f1=f1, f2=f2, cv=cv.reshape(-1, 9), q=g.init_q.numpy().copy(), t=g.init_t.numpy().copy())


def _dev(d):
    import torch
    return {k: torch.as_tensor(v, device="cuda:0") for k, v in d.items()}


def _offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


class World:
    """Everything the tests share: data on the device, and batches filled with the good data once."""

    def __init__(self):
        import torch
        self.off = _offsets(RAGGED)
        self.M, self.P = int(self.off[-1]), len(RAGGED)
        self.good, self.decoy = _dev(_ragged(RAGGED, 11, 0.2)), _dev(_ragged(RAGGED, 12, 0.2))
        self.prev, self.prev_decoy = _dev(_ragged(RAGGED, 13, 0.2)), _dev(_ragged(RAGGED, 14, 0.2))
        self.base = _dev(_ragged(RAGGED, 15, 0.2))                # what a batch holds before a probed fill
        self.batch = self.filled(RAGGED, self.good)               # read-only from here on (its scratch is not)
        self.woff = _offsets(WIDE)
        self.wgood, self.wdecoy = _dev(_ragged(WIDE, 21, 0.1)), _dev(_ragged(WIDE, 22, 0.1))
        self.wide = self.filled(WIDE, self.wgood)
        self.sgood, self.sdecoy = _dev(_ragged(SMALL, 41, 0.2)), _dev(_ragged(SMALL, 42, 0.2))
        self.small_batch = {}                                     # mode -> batch of the SMALL shapes holding sgood
        torch.cuda.synchronize()

    def filled(self, sizes, d, mode=capi.MODE_TARGET):
        import torch
        b = Batch(mode, _offsets(sizes))
        if mode == capi.MODE_NEC:
            b.fill(d["f1"], d["f2"])
        elif mode == capi.MODE_SYM:
            b.fill(d["f1"], d["f2"], d["cv"], d["cv"])
        else:
            b.fill(d["f1"], d["f2"], d["cv"])
        torch.cuda.synchronize()
        return b


_world = None


@pytest.fixture(scope="module")
def world():
    global _world
    if _world is None:
        _world = World()
    return _world


def _pick(d, *keys):
    return {k: d[k] for k in keys}


def _stream():
    import torch
    return torch.cuda.current_stream(0).cuda_stream


def _export_payload(b):
    """pnec_hip_problem_export_payload in DEVICE space on the current stream (Batch.export_payload is HOST space)."""
    import torch
    L = capi.lib()
    out = torch.zeros((max(int(L.pnec_hip_problem_payload_doubles(b._h)), 1),), dtype=torch.float64, device="cuda:0")
    capi.check(L.pnec_hip_problem_export_payload(b._h, out.data_ptr(), capi.MEM_DEVICE, _stream()))
    return out


def _residuals_raw(b, q, t, M, n_hyp=1, reg=1e-13, gate=3.0):
    """pnec_hip_residuals with DEVICE pointers sized for `M` correspondences (the source batch's total: always enough
    for a batch made by select) -- no host-side size is asked for, unlike Batch.residuals.  Entries past the batch's own
    total stay zero."""
    import torch
    S = b.n_pairs * n_hyp
    f = lambda n: torch.zeros((n,), dtype=torch.float64, device="cuda:0")
    res, var, chi2, gchi2, mx = f(M * n_hyp), f(M * n_hyp), f(S), f(S), f(S)
    mask = torch.zeros((M * n_hyp,), dtype=torch.uint8, device="cuda:0")
    cnt = torch.zeros((S,), dtype=torch.int32, device="cuda:0")
    capi.check(capi.lib().pnec_hip_residuals(b._h, q.data_ptr(), t.data_ptr(), n_hyp, reg, gate, res.data_ptr(),
                                             var.data_ptr(), mask.data_ptr(), chi2.data_ptr(), gchi2.data_ptr(),
                                             cnt.data_ptr(), mx.data_ptr(), capi.MEM_DEVICE, _stream()))
    return [res, var, mask, chi2, gchi2, cnt, mx]


def _triangulate_raw(b, q, t, M):
    """pnec_hip_triangulate the same way (PNEC_HIP_TRI_ORIENT)."""
    import torch
    S = b.n_pairs
    f = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda:0")
    i = lambda n: torch.zeros((n,), dtype=torch.int32, device="cuda:0")
    point, d1, d2, psi, var = f(M, 3), f(M), f(M), f(M), f(M)
    front = torch.zeros((M,), dtype=torch.uint8, device="cuda:0")
    nf, nb, sign, to, mean = i(S), i(S), i(S), f(S, 3), f(S)
    p = lambda a: a.data_ptr()
    capi.check(capi.lib().pnec_hip_triangulate(b._h, p(q), p(t), 1, capi.TRI_ORIENT, p(point), p(d1), p(d2), p(psi), p(var),
                                               p(front), p(nf), p(nb), p(sign), p(to), p(mean), capi.MEM_DEVICE, _stream()))
    return [point, d1, d2, psi, var, front, nf, nb, sign, to, mean]


def _new_result(S):
    import torch
    f64 = dict(dtype=torch.float64, device="cuda:0")
    i32 = dict(dtype=torch.int32, device="cuda:0")
    return SolveResult(torch.empty((S, 4), **f64), torch.empty((S, 3), **f64), torch.empty((S,), **f64),
                       torch.empty((S,), **i32), torch.empty((S,), **i32))


def _result_list(r):
    return [r.q, r.t, r.cost, r.iterations, r.status]


def _hyp_t(t, n_hyp, seed):
    """[P * n_hyp, 3] unit start translations around t (numpy in, numpy out)."""
    rng = np.random.default_rng(seed)
    h = np.repeat(t, n_hyp, axis=0) + 0.2 * rng.normal(size=(len(t) * n_hyp, 3))
    return h / np.linalg.norm(h, axis=1, keepdims=True)


# ------------------------------------------------------------------------------------------------ the entries
def _e_fill(w, first=0, n=None):
    n = w.P - first if n is None else n
    a, z = int(w.off[first]), int(w.off[first + n])
    b = Batch(capi.MODE_TARGET, w.off)
    cut = lambda d: {k: d[k][a:z].clone() for k in ("f1", "f2", "cv")}

    def call(bufs):
        b.fill(bufs["f1"], bufs["f2"], bufs["cv"], first_pair=first, n_pairs=n)
        return [_export_payload(b)], b

    return Entry(cut(w.good), cut(w.decoy), call, reset=lambda: b.fill(w.base["f1"], w.base["f2"], w.base["cv"]))


def _keypoints(seed, M):
    rng = np.random.default_rng(seed)
    pts = lambda: rng.uniform([20.0, 20.0], [1220.0, 356.0], size=(M, 2))
    xx, yy = rng.uniform(0.5, 2.0, M), rng.uniform(0.5, 2.0, M)
    xy = rng.uniform(-0.4, 0.4, M) * np.sqrt(xx * yy)
    return _dev(dict(p1=pts(), p2=pts(), c2=np.stack([xx, xy, yy], -1)))


K_INV = np.linalg.inv(np.array([[718.856, 0.0, 607.19], [0.0, 718.856, 185.22], [0.0, 0.0, 1.0]]))


def _e_fill_keypoints(w, k_on_device=False):
    import torch
    b = Batch(capi.MODE_TARGET, w.off)
    K_inv = torch.as_tensor(K_INV, device="cuda:0") if k_on_device else K_INV

    def call(bufs):
        b.fill_keypoints(bufs["p1"], bufs["p2"], bufs["c2"], K_inv=K_inv)
        return [_export_payload(b)], b

    return Entry(_keypoints(31, w.M), _keypoints(32, w.M), call,
                 reset=lambda: b.fill(w.base["f1"], w.base["f2"], w.base["cv"]))


def _e_reshape_fill(w):
    b = Batch.with_capacity(capi.MODE_TARGET, 16, w.M + 2000)
    other = _offsets([7, 130, 64])
    m = int(other[-1])

    def reset():
        b.reshape(other)
        b.fill(w.base["f1"][:m], w.base["f2"][:m], w.base["cv"][:m])

    def call(bufs):
        b.reshape(w.off)
        b.fill(bufs["f1"], bufs["f2"], bufs["cv"])
        return [_export_payload(b)], b

    return Entry(_pick(w.good, "f1", "f2", "cv"), _pick(w.decoy, "f1", "f2", "cv"), call, reset=reset)


def _e_solve(w, n_hyp=1, mode=capi.MODE_TARGET):
    import torch
    if mode == capi.MODE_TARGET:
        b, good, decoy = w.batch, w.good, w.decoy
    else:                                             # the other residual families on the small prefix of the shapes
        if mode not in w.small_batch:
            w.small_batch[mode] = w.filled(SMALL, w.sgood, mode)
        b, good, decoy = w.small_batch[mode], w.sgood, w.sdecoy
    S = b.n_pairs * n_hyp
    out = _new_result(S)
    if n_hyp == 1:
        g, d = _pick(good, "q", "t"), _pick(decoy, "q", "t")
        call = lambda bufs: (_result_list(b.solve(bufs["q"], bufs["t"], out=out)), b)
    else:
        mk = lambda src, seed: dict(q=src["q"], h=torch.as_tensor(_hyp_t(src["t"].cpu().numpy(), n_hyp, seed), device="cuda:0"))
        g, d = mk(good, 51), mk(decoy, 52)
        call = lambda bufs: (_result_list(b.solve(bufs["q"], None, hyp_t=bufs["h"], n_hyp=n_hyp, out=out)), b)
    return Entry(g, d, call, sentinels=_result_list(out))


def _e_select_best(w):
    import torch
    mk = lambda seed: dict(c=torch.as_tensor(np.random.default_rng(seed).uniform(0.0, 1.0, 1037 * 5), device="cuda:0"))
    return Entry(mk(61), mk(62), lambda bufs: ([select_best(bufs["c"], 5)], None))


def _e_cost_function(w):
    return Entry(_pick(w.good, "q", "t"), _pick(w.decoy, "q", "t"),
                 lambda bufs: ([w.batch.cost_function(bufs["q"], bufs["t"])], None))


def _e_pose_covariance(w):
    def call(bufs):
        c = w.batch.pose_covariance(bufs["q"], bufs["t"])
        return [c.cov, c.info, c.grad, c.cost, c.status], None
    return Entry(_pick(w.good, "q", "t"), _pick(w.decoy, "q", "t"), call)


def _e_residuals(w):
    def call(bufs):
        r = w.batch.residuals(bufs["q"], bufs["t"])
        return [r.residual, r.variance, r.mask, r.chi2, r.gated_chi2, r.gated_count, r.max_abs], None
    return Entry(_pick(w.good, "q", "t"), _pick(w.decoy, "q", "t"), call)


def _e_triangulate(w):
    def call(bufs):
        r = w.batch.triangulate(bufs["q"], bufs["t"])
        return [r.point, r.depth1, r.depth2, r.parallax, r.depth1_var, r.front, r.n_front, r.n_back, r.sign, r.t,
                r.parallax_mean], None
    return Entry(_pick(w.good, "q", "t"), _pick(w.decoy, "q", "t"), call)


def _links(w, seed):
    """prev_pair [P] and link [sum N]: every pair follows the pair of the same index of `prev`; a correspondence links to
    a track of that pair drawn at random (in range, so every link is valid), one in ten not linked."""
    import torch
    rng = np.random.default_rng(seed)
    link = np.concatenate([np.where(rng.random(n) < 0.1, -1, rng.integers(0, max(n, 1), n)) for n in RAGGED])
    return dict(pp=torch.arange(w.P, dtype=torch.int64, device="cuda:0"),
                link=torch.as_tensor(link.astype(np.int32), device="cuda:0"))


def _e_relative_scale(w):
    prev = Batch(capi.MODE_TARGET, w.off)

    def mk(cur, prv, seed):
        d = dict(q=cur["q"], t=cur["t"], qp=prv["q"], tp=prv["t"], f1=prv["f1"], f2=prv["f2"], cv=prv["cv"])
        d.update(_links(w, seed))
        return d

    def call(bufs):
        prev.fill(bufs["f1"], bufs["f2"], bufs["cv"])             # the previous pairs arrive on the same stream
        r = w.batch.relative_scale(prev, bufs["pp"], bufs["link"], bufs["q"], bufs["t"], bufs["qp"], bufs["tp"])
        return [r.scale, r.q25, r.q75, r.n_linked, r.n_used, r.ratio, r.used], prev

    return Entry(mk(w.good, w.prev, 71), mk(w.decoy, w.prev_decoy, 72), call,
                 reset=lambda: prev.fill(w.base["f1"], w.base["f2"], w.base["cv"]))


def _e_nec_eigensolver(w):
    return Entry(_pick(w.good, "q"), _pick(w.decoy, "q"), lambda bufs: (list(w.batch.nec_eigensolver(bufs["q"])), None))


def _e_ransac(w, scheme=0, batch=None, good=None, decoy=None):
    b = w.batch if batch is None else batch
    good, decoy = (w.good, w.decoy) if batch is None else (good, decoy)

    def call(bufs):
        b.set_eigensolver_scheme(scheme)
        try:
            return list(b.ransac_eigensolver(bufs["q"], seed=9, max_iterations=RANSAC_IT)), None
        finally:
            b.set_eigensolver_scheme(0)

    return Entry(_pick(good, "q"), _pick(decoy, "q"), call)


def _e_weighted(w):
    return Entry(_pick(w.good, "q", "t"), _pick(w.decoy, "q", "t"),
                 lambda bufs: (list(w.batch.weighted_eigensolver(bufs["q"], bufs["t"])), None))


def _e_select(w, view):
    import torch
    mk = lambda src, seed: dict(q=src["q"], t=src["t"], m=torch.as_tensor(
        (np.random.default_rng(seed).random(w.M) < 0.7).astype(np.uint8), device="cuda:0"))

    def call(bufs):
        sel = w.batch.select(bufs["m"], view=view)                # and straight on, no host-side size in between:
        return _residuals_raw(sel, bufs["q"], bufs["t"], w.M) + _triangulate_raw(sel, bufs["q"], bufs["t"], w.M), sel

    return Entry(mk(w.good, 81), mk(w.decoy, 82), call)


def _e_pipeline(w, batch=None, good=None, decoy=None, **kw):
    b = w.batch if batch is None else batch
    good, decoy = (w.good, w.decoy) if batch is None else (good, decoy)
    opts = capi.default_pipeline_options(**kw) if kw else None
    return Entry(_pick(good, "q", "t"), _pick(decoy, "q", "t"),
                 lambda bufs: (list(b.solve_pipeline(bufs["q"], bufs["t"], options=opts, want_inliers=True)), None))


def _ut_data(seed, n=1037):
    rng = np.random.default_rng(seed)
    mu = np.concatenate([rng.uniform(-0.6, 0.6, size=(n, 2)), np.ones((n, 1))], 1)
    cov = np.zeros((n, 3, 3))
    a = rng.normal(size=(n, 2, 2)) * 1e-3
    cov[:, :2, :2] = a @ a.transpose(0, 2, 1) + 1e-7 * np.eye(2)
    return _dev(dict(mu=mu, cov=cov))


def _e_unscented(w):
    from pnec_amd import frontend

    def call(bufs):
        bvs, covs = frontend.unscented_transform(bufs["mu"], bufs["cov"])
        return [bvs, covs], None
    return Entry(_ut_data(91), _ut_data(92), call)


def _patch_data(seed):
    import torch
    rng = np.random.default_rng(seed)
    img = (rng.uniform(20.0, 200.0, size=(4, 24, 32)) + 40.0 * np.sin(np.arange(32) / 3.0)).astype(np.float32)
    pts = rng.uniform([8.0, 8.0], [23.0, 15.0], size=(4 * 9, 2))
    return dict(img=torch.as_tensor(img, device="cuda:0"), pts=torch.as_tensor(pts, device="cuda:0"))


def _e_patch_covariance(w):
    import torch
    from pnec_amd import patches
    off = torch.arange(5, dtype=torch.int64, device="cuda:0") * 9
    pattern = torch.as_tensor(np.array(patches.PATTERN52), device="cuda:0")

    def call(bufs):
        r = patches.patch_covariance(bufs["img"], bufs["pts"], offsets=off, pattern=pattern)
        return [r.cov, r.hessian, r.mean, r.n_valid, r.status], None
    return Entry(_patch_data(95), _patch_data(96), call)


ENTRIES = {
    "fill": _e_fill,
    "fill_pair_range": lambda w: _e_fill(w, 3, 4),
    "fill_keypoints": _e_fill_keypoints,
    "fill_keypoints_device_K_inv": lambda w: _e_fill_keypoints(w, True),
    "reshape_fill_export_payload": _e_reshape_fill,
    "solve": _e_solve,
    "solve_n_hyp3": lambda w: _e_solve(w, 3),
    "solve_nec": lambda w: _e_solve(w, 1, capi.MODE_NEC),
    "solve_nec_n_hyp3": lambda w: _e_solve(w, 3, capi.MODE_NEC),
    "solve_host": lambda w: _e_solve(w, 1, capi.MODE_HOST),
    "solve_host_n_hyp3": lambda w: _e_solve(w, 3, capi.MODE_HOST),
    "solve_sym": lambda w: _e_solve(w, 1, capi.MODE_SYM),
    "solve_sym_n_hyp3": lambda w: _e_solve(w, 3, capi.MODE_SYM),
    "select_best": _e_select_best,
    "cost_function": _e_cost_function,
    "pose_covariance": _e_pose_covariance,
    "residuals": _e_residuals,
    "triangulate": _e_triangulate,
    "relative_scale": _e_relative_scale,
    "nec_eigensolver": _e_nec_eigensolver,
    "ransac_eigensolver_scheme0": lambda w: _e_ransac(w, 0),
    "ransac_eigensolver_scheme1": lambda w: _e_ransac(w, 1),
    "ransac_eigensolver_scheme2": lambda w: _e_ransac(w, 2),
    "weighted_eigensolver": _e_weighted,
    "select_then_residuals_triangulate": lambda w: _e_select(w, False),
    "select_view_then_residuals_triangulate": lambda w: _e_select(w, True),
    "solve_pipeline": _e_pipeline,
    "solve_pipeline_no_ransac": lambda w: _e_pipeline(w, use_ransac=0),
    "solve_pipeline_use_nec": lambda w: _e_pipeline(w, use_nec=1),
    "unscented_transform": _e_unscented,
    "patch_covariance": _e_patch_covariance,
    "wide_solve_pipeline": lambda w: _e_pipeline(w, w.wide, w.wgood, w.wdecoy),
    "wide_ransac_eigensolver": lambda w: _e_ransac(w, 0, w.wide, w.wgood, w.wdecoy),
}


# ------------------------------------------------------------------------------------------------ 1. the probe's teeth
def test_the_probe_flags_calls_that_break_stream_order():
    """Three stand-in entry points written in torch (valid memory only): one that clones its input on the current stream
    passes; one that clones under ANOTHER stream without waiting reads the decoy and is flagged; one that forks to another
    stream behind an event, sleeps there, clones and never joins back is flagged too -- its output is not there when the
    caller's stream gets to it, and what arrives later is the decoy's (the late read)."""
    import torch
    x = torch.arange(4096, dtype=torch.float64, device="cuda:0")
    good, decoy = dict(x=x * 1.5 + 1.0), dict(x=-x)
    T = torch.cuda.Stream()
    out = torch.empty_like(x)

    def in_order(bufs):
        out.copy_(bufs["x"] * 2.0)
        return [out], None

    def on_another_stream(bufs):
        with torch.cuda.stream(T):
            out.copy_(bufs["x"] * 2.0)
        return [out], None

    def forked_and_never_joined(bufs):
        ev = torch.cuda.Event()
        ev.record()
        with torch.cuda.stream(T):
            T.wait_event(ev)
            _delay(5.0)
            out.copy_(bufs["x"] * 2.0)
        return [out], None

    ok = check(Entry(good, decoy, in_order, sentinels=[out]), "stand-in: in order")
    assert ok.returned_early
    early = probe(Entry(good, decoy, on_another_stream, sentinels=[out]))
    assert early.mismatch == [0] and _same(early.got[0], early.want_decoy[0])         # it read the decoy, early
    # (its reference is the in-order call's result: torch's streams do not wait for the default stream either)
    late = probe(Entry(good, decoy, forked_and_never_joined, sentinels=[out]), want=ok.want)
    assert late.mismatch == [0] and late.late_mismatch == [0]
    assert bool((late.got[0] == F_SENTINEL).all())                                    # nothing there yet on the caller's stream
    assert _same(late.live[0], early.want_decoy[0])                                   # and the late read saw the decoy


# ------------------------------------------------------------------------------------------------ 2. every call, probed
def test_the_ragged_batch_uses_three_geometries_and_the_streaming_form(world):
    """Otherwise pnec_hip_solve never forks its per-geometry launches onto side streams."""
    seen = set()
    for n in RAGGED:
        with Batch(capi.MODE_TARGET, np.array([0, n], dtype=np.int64)) as b:
            d = b.describe_launch()
            seen.add((d["corr_per_lane"], d["waves_per_pair"], d["lds_corr_per_lane"], d["resident"]))
    assert len(seen) >= 3 and any(not g[3] for g in seen) and any(g[3] for g in seen), seen
    assert len(WIDE) == 1024 and min(WIDE) == 12 and max(WIDE) == 40


@pytest.mark.parametrize("name", list(ENTRIES))
def test_device_space_call_respects_stream_order(world, name):
    """The probe of the module docstring on one DEVICE-space entry point: the same bits as the call on the default
    stream, and the call returned while the work queued ahead of it on the stream was still running."""
    check(ENTRIES[name](world), name)


def test_fill_keypoints_takes_K_inv_from_the_host_or_the_device_with_the_same_bits(world):
    """Batch.fill_keypoints with torch.cuda inputs: a host K_inv (uploaded once per value, then cached) and a CUDA K_inv
    (transposed on the device) fill the same planes, bit for bit."""
    import torch
    w, kp = world, _keypoints(31, world.M)
    pay = []
    with Batch(capi.MODE_TARGET, w.off) as b:                     # (one batch: whatever its padding lanes hold stays)
        for K in (None, K_INV, torch.as_tensor(K_INV, device="cuda:0"), K_INV):
            b.fill(w.base["f1"], w.base["f2"], w.base["cv"])
            b.fill_keypoints(kp["p1"], kp["p2"], kp["c2"], K_inv=K)
            pay.append(torch.as_tensor(b.export_payload()))
    assert _same(pay[1], pay[2]) and _same(pay[1], pay[3])
    assert not _same(pay[0], pay[1])                              # (K_inv matters: the first fill used the identity)


# ------------------------------------------------------------------------------------------------ 3. several in flight
def _stage_chain(b, d, M):
    """The stage-by-stage chain as a list of steps, each enqueueing one stage on the current stream."""
    st = {}

    def ransac():
        st["rq"], st["rt"], st["mask"], st["cnt"], st["its"] = b.ransac_eigensolver(d["q"], seed=3, max_iterations=RANSAC_IT)

    def select():
        st["sel"] = b.select(st["mask"], view=True)

    def weighted():
        st["wq"], st["wt"] = st["sel"].weighted_eigensolver(st["rq"], st["rt"])

    def solve():
        st["res"] = st["sel"].solve(st["wq"], st["wt"])

    def cov():
        st["cov"] = st["sel"].pose_covariance(st["res"].q, st["res"].t)

    def residuals():
        st["r"] = _residuals_raw(st["sel"], st["res"].q, st["res"].t, M)

    def triangulate():
        st["tri"] = _triangulate_raw(st["sel"], st["res"].q, st["res"].t, M)

    def outputs():
        c = st["cov"]
        return ([st["rq"], st["rt"], st["mask"], st["cnt"], st["its"], st["wq"], st["wt"]] + _result_list(st["res"])
                + [c.cov, c.info, c.grad, c.cost, c.status] + st["r"] + st["tri"])

    return [ransac, select, weighted, solve, cov, residuals, triangulate], outputs, st


def _in_flight(batches, data, make_steps):
    """Each batch's steps alone on the default stream, then all of them round-robin across one side stream per batch,
    released together by one delay: -> (alone, together), lists of cloned output lists."""
    import torch
    alone = []
    for b, d in zip(batches, data):
        steps, outputs, st = make_steps(b, d)
        for s in steps:
            s()
        alone.append([o.clone() for o in outputs()])
        torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in batches]
    hold, release = torch.cuda.Stream(), torch.cuda.Event()
    chains = [make_steps(b, d) for b, d in zip(batches, data)]
    torch.cuda.synchronize()
    with torch.cuda.stream(hold):
        _delay(DELAY_MS)
        release.record()
    for S in streams:
        S.wait_event(release)
    for k in range(len(chains[0][0])):
        for S, (steps, _, _) in zip(streams, chains):
            with torch.cuda.stream(S):
                steps[k]()
    together = []
    for S, (_, outputs, _) in zip(streams, chains):
        with torch.cuda.stream(S):
            got = [o.clone() for o in outputs()]
        S.synchronize()
        together.append(got)
    torch.cuda.synchronize()
    return alone, together


def test_three_chains_in_flight_equal_each_alone(world):
    """Three ragged batches, each on its own side stream, the stage-by-stage chain (ransac_eigensolver -> select(view) ->
    weighted_eigensolver -> solve -> pose_covariance -> residuals -> triangulate) enqueued ROUND-ROBIN across the three
    streams behind one delay: every output equals, bitwise, the same chain run alone on the default stream.  Then three
    wide batches and solve_pipeline, the recipe INTEGRATION.md recommends.  What this catches is shared mutable state:
    device globals of the front stages, the pooled streams and events, scratch a view shares with its source."""
    w = world
    data = [w.good, _dev(_ragged(RAGGED, 16, 0.2)), _dev(_ragged(RAGGED, 17, 0.2))]
    batches = [w.batch] + [w.filled(RAGGED, d) for d in data[1:]]
    alone, together = _in_flight(batches, data, lambda b, d: _stage_chain(b, d, w.M))
    for k, (a, g) in enumerate(zip(alone, together)):
        bad = [i for i, (x, y) in enumerate(zip(a, g)) if not _same(x, y)]
        assert not bad, f"stage chain {k}: outputs {bad} differ from the chain run alone"
    assert not _same(alone[0][0], alone[1][0])                    # (three different problems)

    wdata = [w.wgood, w.wdecoy, _dev(_ragged(WIDE, 23, 0.1))]
    wbatches = [w.wide] + [w.filled(WIDE, d) for d in wdata[1:]]

    def pipeline_steps(b, d):
        st = {}

        def run():
            st["o"] = list(b.solve_pipeline(d["q"], d["t"], want_inliers=True))
        return [run], (lambda: st["o"]), st

    alone, together = _in_flight(wbatches, wdata, pipeline_steps)
    for k, (a, g) in enumerate(zip(alone, together)):
        bad = [i for i, (x, y) in enumerate(zip(a, g)) if not _same(x, y)]
        assert not bad, f"solve_pipeline {k}: outputs {bad} differ from the call alone"
    for b in batches[1:] + wbatches[1:]:
        b.close()


# ------------------------------------------------------------------------------------------------ 4. HOST space on a stream
@pytest.mark.parametrize("which", ["solve", "solve_pipeline", "residuals"])
def test_host_space_call_on_a_callers_stream_waits_for_that_streams_earlier_work(world, which):
    """A DEVICE-space fill of the good data is queued on S behind the delay; the HOST-space call that follows with
    stream = S (what pnec_host.cc does on pnec_hip_frame_stream()) returns the good data's results, bitwise those of the
    all-host call on the default stream -- and returns only after the gate has fired: "HOST: blocking" means blocking on
    that stream's earlier work too."""
    import torch
    w, L = world, capi.lib()
    P, M = len(SMALL), int(sum(SMALL))
    good, decoy = _ragged(SMALL, 41, 0.2), _ragged(SMALL, 42, 0.2)
    dgood = _dev(good)
    p = lambda a: a.ctypes.data

    def host_call(b, stream):
        q, t = np.ascontiguousarray(good["q"]), np.ascontiguousarray(good["t"])
        if which == "solve":
            o = [np.full((P, 4), F_SENTINEL), np.full((P, 3), F_SENTINEL), np.full(P, F_SENTINEL),
                 np.full(P, I_SENTINEL, dtype=np.int32), np.full(P, I_SENTINEL, dtype=np.int32)]
            capi.check(L.pnec_hip_solve(b._h, p(q), p(t), 1, None, 1e-13, None, p(o[0]), p(o[1]), p(o[2]), p(o[3]), p(o[4]),
                                        capi.MEM_HOST, stream))
        elif which == "solve_pipeline":
            o = [np.full((P, 4), F_SENTINEL), np.full((P, 3), F_SENTINEL), np.full(M, I_SENTINEL, dtype=np.uint8),
                 np.full(P, I_SENTINEL, dtype=np.int32)]
            capi.check(L.pnec_hip_solve_pipeline(b._h, p(q), p(t), None, p(o[0]), p(o[1]), p(o[2]), p(o[3]), capi.MEM_HOST,
                                                 stream))
        else:
            o = [np.full(M, F_SENTINEL), np.full(M, F_SENTINEL), np.full(M, I_SENTINEL, dtype=np.uint8), np.full(P, F_SENTINEL),
                 np.full(P, F_SENTINEL), np.full(P, I_SENTINEL, dtype=np.int32), np.full(P, F_SENTINEL)]
            capi.check(L.pnec_hip_residuals(b._h, p(q), p(t), 1, 1e-13, 3.0, *[p(a) for a in o], capi.MEM_HOST, stream))
        return o

    with Batch(capi.MODE_TARGET, _offsets(SMALL)) as b:
        b.fill(good["f1"], good["f2"], good["cv"])                # all-host, default stream
        want = host_call(b, None)
        b.fill(decoy["f1"], decoy["f2"], decoy["cv"])
        want_decoy = host_call(b, None)
        assert any(not np.array_equal(a.view(np.uint8), c.view(np.uint8)) for a, c in zip(want, want_decoy))
        S = torch.cuda.Stream()
        for ms in (0.0, DELAY_MS):                                # (a warm-up without the delay first)
            b.fill(decoy["f1"], decoy["f2"], decoy["cv"])         # a call that does not wait finds the decoy
            torch.cuda.synchronize()
            with torch.cuda.stream(S):
                if ms:
                    _delay(ms)
                gate = torch.cuda.Event()
                gate.record()
                b.fill(dgood["f1"], dgood["f2"], dgood["cv"])     # DEVICE space, on S
                got = host_call(b, S.cuda_stream)
                waited = gate.query()
            S.synchronize()
        bad = [i for i, (a, c) in enumerate(zip(got, want)) if not np.array_equal(a.view(np.uint8), c.view(np.uint8))]
        assert not bad, f"HOST-space {which} on a caller's stream: outputs {bad} differ"
        assert waited, f"HOST-space {which} returned before the work queued ahead of it on its stream had run"
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 5. handles on a caller's stream
def _frame_pair(n, seed, outliers=0.12):
    """(the `_pair` data of test_frame_gpu.py)"""
    g = sim.generate(1, max(n, 1), seed=seed)
    b1, b2, cv = g.bvs1[0, :n].numpy().copy(), g.bvs2[0, :n].numpy().copy(), g.covs2[0, :n].numpy().copy()
    rng = np.random.default_rng(seed)
    k = int(n * outliers)
    if k:
        bad = rng.choice(n, k, replace=False)
        v = rng.normal(size=(k, 3))
        b2[bad] = v / np.linalg.norm(v, axis=1, keepdims=True)
    return b1, b2, cv, g.init_q[0].numpy(), g.init_t[0].numpy()


def _stream_is_still_the_callers(S):
    import torch
    src = torch.arange(1000, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    with torch.cuda.stream(S):
        dst = src.clone()
    S.synchronize()
    assert bool(torch.equal(dst, src))


def test_frame_handle_created_on_a_callers_stream():
    """pnec_hip_frame_create(device, 2048, S): pnec_hip_frame_stream returns S, pnec_hip_frame_solve gives the bits of a
    handle with a stream of its own, and pnec_hip_frame_destroy leaves S to its owner (own_stream is false there: the
    destroy path waits for the stream and does not return it to the pool or destroy it)."""
    import torch
    from pnec_amd.frame import FrameSolver
    L = capi.lib()
    S = torch.cuda.Stream()
    h = C.c_void_p()
    capi.check(L.pnec_hip_frame_create(0, 2048, S.cuda_stream, C.byref(h)))
    on_s = FrameSolver.__new__(FrameSolver)
    on_s._lib, on_s.device, on_s._h = L, 0, h
    try:
        assert L.pnec_hip_frame_stream(h) == S.cuda_stream
        with FrameSolver(max_corr=2048) as own:
            assert L.pnec_hip_frame_stream(own._h) != S.cuda_stream
            for i, n in enumerate([512, 33, 0, 1500, 9]):
                b1, b2, cv, q0, t0 = _frame_pair(n, 100 + i)
                q, t, mask, cnt = on_s.solve(b1, b2, cv, q0, t0)
                if n == 0:
                    continue                                      # (nothing defined to compare: it must just survive)
                rq, rt, rmask, rcnt = own.solve(b1, b2, cv, q0, t0)
                assert np.array_equal(q.view(np.int64), rq.view(np.int64)) and np.array_equal(t.view(np.int64), rt.view(np.int64)), n
                assert np.array_equal(mask, rmask) and cnt == rcnt, n
    finally:
        on_s.close()
    _stream_is_still_the_callers(S)


def test_streaming_handle_created_on_a_callers_stream():
    """pnec_hip_stream_create(..., stream = S): eight submits collected with wait equal the own-stream handle's records
    bitwise, and S is usable after pnec_hip_stream_destroy."""
    import torch
    from pnec_amd.streaming import Stream
    L = capi.lib()
    S = torch.cuda.Stream()
    h = C.c_void_p()
    capi.check(L.pnec_hip_stream_create(0, 2048, 1, 8, S.cuda_stream, C.byref(h)))
    on_s = Stream.__new__(Stream)
    on_s._lib, on_s.max_corr, on_s.max_pairs, on_s.slots, on_s.device, on_s._h, on_s._pairs = L, 2048, 1, 8, 0, h, {}
    sizes = SMALL * 2
    pairs = [_frame_pair(n, 200 + i) for i, n in enumerate(sizes)]
    try:
        with Stream(max_corr=2048, max_pairs=1, slots=8) as own:
            recs = []
            for s in (on_s, own):
                tickets = [s.submit(capi.MODE_TARGET, b1, b2, cv, init_q=q0, init_t=t0) for b1, b2, cv, q0, t0 in pairs]
                recs.append([s.wait(tk) for tk in tickets])
        for n, a, b in zip(sizes, *recs):
            for x, y in zip(_result_list(a), _result_list(b)):
                assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), n
            assert np.isfinite(a.q).all() and np.isfinite(a.t).all()
    finally:
        on_s.close()
    _stream_is_still_the_callers(S)


# ------------------------------------------------------------------------------------------------ 6. forced forms, fresh processes
CHILD = r'''
import os, sys
sys.path.insert(0, os.environ["PNEC_ROOT"])
sys.path.insert(0, os.path.join(os.environ["PNEC_ROOT"], "tests"))
import numpy as np
import torch
import test_stream_order_gpu as T
w = T.World()
ref = np.load(os.environ["PNEC_STREAM_ORDER_WANT"])
for name in os.environ["PNEC_STREAM_ORDER_ENTRIES"].split(","):
    want = [torch.as_tensor(ref[f"{name}.{i}"], device="cuda:0") for i in range(sum(k.startswith(name + ".") for k in ref.files))]
    T.check(T.ENTRIES[name](w), name, want=want)
torch.cuda.synchronize()
print("STREAM_ORDER_CHILD_OK")
'''


def _child(world, tmp_path, names, env):
    import torch
    ref = {}
    for name in names:
        e = ENTRIES[name](world)
        bufs = {k: v.clone() for k, v in e.good.items()}
        for i, o in enumerate(_on_default_stream(e, bufs, e.good)):
            ref[f"{name}.{i}"] = o.cpu().numpy()
    torch.cuda.synchronize()
    path = os.path.join(str(tmp_path), "want.npz")
    np.savez(path, **ref)
    env = dict(os.environ, PNEC_ROOT=ROOT, PNEC_STREAM_ORDER_WANT=path, PNEC_STREAM_ORDER_ENTRIES=",".join(names), **env)
    r = subprocess.run([sys.executable, "-c", CHILD], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "STREAM_ORDER_CHILD_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    print(r.stdout)


def test_chunked_pipeline_forced_to_three_ranges_respects_stream_order(world, tmp_path):
    """PNEC_PIPELINE_CHUNKS=3 (read once per process: a fresh child): solve_pipeline on the ragged and on the wide batch
    under a side stream, probed as above, against the ONE-range results computed here -- "bit for bit those of one range"
    (pnec_pipeline.hip), with K whole chains on K pooled streams forked from and joined into the caller's."""
    _child(world, tmp_path, ["solve_pipeline", "wide_solve_pipeline"], dict(PNEC_PIPELINE_CHUNKS="3"))


def test_two_pair_ransac_form_forced_respects_stream_order(world, tmp_path):
    """PNEC_RANSAC_FORM=2 (two pairs per wavefront, normally from 4096 pairs up) on the ragged batch in a fresh child:
    the same bits as the one-pair form computed here, on a side stream."""
    _child(world, tmp_path, ["ransac_eigensolver_scheme0"], dict(PNEC_RANSAC_FORM="2"))
