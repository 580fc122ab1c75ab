"""bspatom_tdse_adaptive / _dev (csrc/tdse_adapt.hip: the stage and the step with their ADAPT flag, tdse_adapt_control_kernel,
tdse_adapt_commit_kernel) on the GPU against the restatement tests/tdse_adapt_ref.py and against bspatom_tdse_static.

What is exact is compared bit for bit: the controller's decisions, the interpolated field (log_f), and the guarantees of the header
(chain identity, fixed-step identity, reproducibility, continuation) with np.array_equal on the bit patterns.  The amplitudes and the
estimate are held to the yardstick of tests/test_gpu_tdse_static.py along the device's own step sequence: the restatement run in complex128
and in long double, the library within 8 times the complex128 run's own distance (tdse_ref.amp_bound / err_bound).  The decisions are
compared with those of the long-double restatement under its own controller; tests/test_tdse_adapt_cpu.py keeps every estimate of that
run 1e-3 away, relatively, from tol and tol / 64.  Never against the code under test."""
import ctypes as C
import functools
import numpy as np
import pytest
import torch                               # first: its HIP runtime is the one the process uses
from test_gpu_stages import input_from_case, note

import tdse_adapt_ref as R
import tdse_ref
import tdse_static_ref
from bspatom_amd import capi, host

pytestmark = pytest.mark.gpu
EPS = tdse_ref.EPS
LOG_CAP = 128
KEYS = [key + (scheme,) for key in R.SHAPES for scheme in (0, 1)]


@pytest.fixture(scope="module")
def prob():
    p = capi.Problem(input_from_case("tiny8"))           # the handle gives the device and the stream only
    yield p
    p.close()


def same(x, y):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    return x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8))


_runs = {}


def gpu_run(prob, nch, count, nscan, scheme, max_level=R.MAX_LEVEL_TEST, blocks=True):
    """The configuration's run with rows and snapshots on every coarse step and the whole log, once per module:
    (system, (a, err, obs, snaps, stats, (log_i, log_e, log_f)))"""
    k = (nch, count, nscan, scheme, max_level, blocks)
    if k not in _runs:
        s = R.adapt_system(nch, count, nscan, blocks)
        E, pairs, D, a0, fn, static = s
        _runs[k] = (s, prob.tdse_adaptive(E, pairs, D, a0, fn, R.DT, static, R.TOL, max_level, nsub=R.NSUB, level0=R.LEVEL0, scheme=scheme,
                                          obs_every=1, snap_every=1, log_cap=LOG_CAP))
    return _runs[k]


@functools.lru_cache(maxsize=None)
def long_log(nch, count, nscan, scheme, max_level):
    """the attempts (n, m, j, flag) of the long-double restatement under its own controller"""
    E, pairs, D, a0, fn, static = R.adapt_system(nch, count, nscan)
    log = R.run(E, pairs, D, a0, fn, R.DT, R.NSUB, static, scheme, R.TOL, max_level, R.LEVEL0, np.longdouble, np.clongdouble)[2]
    return [r[:4] for r in log]


# ---- 1 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", KEYS)
def test_parity_with_the_restatement(prob, key):
    nch, count, nscan, scheme = key
    (E, pairs, D, a0, fn, static), (a, err, obs, snaps, stats, (li, le, lf)) = gpu_run(prob, *key)
    assert a.shape == a0.shape and err.shape == (nscan,) and obs.shape == (R.NSTEPS + 1, nscan, nch, 6)
    assert snaps.shape == (R.NSTEPS, nscan, nch, count) and stats[5] == len(li) <= LOG_CAP
    # the decisions are the long-double restatement's
    assert [tuple(r) for r in li.tolist()] == long_log(*key, R.MAX_LEVEL_TEST)
    # the field of every attempt is the float64 Hermite restatement, bit for bit
    for t, (n, m, j, flag) in enumerate(li.tolist()):
        assert same(lf[t], R.attempt_field(fn, R.DT, R.NSUB, n, m, j)), (t, n, m, j)
    # a and err along the device's own sequence
    r128 = R.run(E, pairs, D, a0, fn, R.DT, R.NSUB, static, scheme, R.TOL, R.MAX_LEVEL_TEST, R.LEVEL0, sequence=li)
    rlong = R.run(E, pairs, D, a0, fn, R.DT, R.NSUB, static, scheme, R.TOL, R.MAX_LEVEL_TEST, R.LEVEL0, np.longdouble, np.clongdouble, sequence=li)
    ba, be = tdse_ref.amp_bound(r128[0], rlong[0]), tdse_ref.err_bound(r128[1], rlong[1], R.DT)
    da = float(np.max(np.abs(a.astype(np.clongdouble) - rlong[0])))
    de = float(np.max(np.abs(err.astype(np.longdouble) - rlong[1])))
    note("tdse adaptive parity %s: %d attempts, max|a - a_long| / bound = %.3g (restatement's own distance %.3g eps), |err - err_long| / bound "
         "= %.3g (err %.3g)" % (key, len(li), da / ba, ba / 8.0 / EPS, de / be, float(np.max(err))))
    assert da <= ba, (key, da, ba)
    assert de <= be, (key, de, be)
    # the estimate of every accepted attempt, per scan, against the long-double run's largest (the same yardstick, per step)
    acc = li[:, 3] > 0
    e128 = np.array([float(r[4]) for r in r128[2]])
    elong = np.array([r[4] for r in rlong[2]], dtype=np.longdouble)
    dstep = np.abs(le[acc].max(axis=1).astype(np.longdouble) - elong)
    bstep = 8.0 * np.maximum(np.abs(e128.astype(np.longdouble) - elong), EPS * R.DT)
    assert np.all(dstep <= bstep), (key, dstep, bstep)
    # rows: k = 4, 5 against the long-double definition on the run's own states, k = 0 .. 3 the bits of bspatom_tdse_observe on them
    states = np.concatenate([a0[None], snaps])
    ref = tdse_static_ref.observables(E, pairs, D, static, states, np.longdouble, np.clongdouble)
    M = tdse_static_ref.static_magnitudes(static, states)
    diff = np.abs(obs.astype(np.longdouble) - ref).reshape(-1, 6).max(axis=0)[4:]
    bound = (count * (len(static[0]) + 1) + 16) * np.longdouble(EPS) * M
    assert diff[0] <= bound[0] and diff[1] <= bound[1], (diff, bound)
    packets = states.reshape(-1, nch, count)
    o4 = prob.tdse_observe(E, pairs, D, packets, np.zeros((0, 6, len(packets)), dtype=np.complex128), R.DT, obs_every=1)[2]
    assert same(o4[0].reshape(R.NSTEPS + 1, nscan, nch, 4), obs[..., :4])
    assert same(a, snaps[-1])


# ---- 2 ----------------------------------------------------------------------------------------------------------------
def replay(prob, s, scheme, li, lf, scans=slice(None)):
    """the accepted steps of the log as a chain of bspatom_tdse_static calls of one step each, on the scans `scans`: (a, the rows at the
    coarse steps' starts, the amplitudes after every coarse step, the per-step err)"""
    E, pairs, D, a0, fn, static = s
    a = a0[scans]
    rows, snaps, errs = [], [], []
    seq = li.tolist()
    for t, (n, m, j, flag) in enumerate(seq):
        if not flag:
            continue
        a, e, o = prob.tdse_static(E, pairs, D, a, lf[t][None][:, :, scans], float(np.ldexp(R.DT, -m)), static, scheme=scheme, obs_every=1)
        errs.append(e)
        if j == 0:
            rows.append(o[0])
        if t + 1 == len(seq) or seq[t + 1][0] != n:
            snaps.append(a)
            last = o[1]
    return a, np.array(rows + [last]), np.array(snaps), np.array(errs)


@pytest.mark.parametrize("key", KEYS)
def test_chain_identity(prob, key):
    """Guarantee 1, and 3: the log follows the rule exactly."""
    nch, count, nscan, scheme = key
    s, (a, err, obs, snaps, stats, (li, le, lf)) = gpu_run(prob, *key)
    ra, rrows, rsnaps, rerrs = replay(prob, s, scheme, li, lf)
    assert same(ra, a) and same(rsnaps, snaps) and same(rrows, obs) and same(rerrs, le[li[:, 3] > 0])
    assert same(err, rerrs.max(axis=0))
    n, m, j = R.follows_rule(li, le, R.TOL, R.MAX_LEVEL_TEST, R.LEVEL0, nsteps=R.NSTEPS)
    acc = int(np.sum(li[:, 3] > 0))
    assert stats.tolist() == [acc, len(li) - acc, int(np.sum(li[:, 3] == 2)), int(li[:, 1].max()), m, len(li)]
    # the accepted steps tile the run: in units of the coarse step the starts and sizes are dyadic, so the sums are exact
    ts, hs = host.adapt_steps(li, 0.0, 1.0)
    assert ts[0] == 0.0 and np.array_equal(ts[1:], (ts + hs)[:-1]) and ts[-1] + hs[-1] == float(R.NSTEPS)


def test_chain_identity_scan_by_scan_and_without_blocks(prob):
    """Guarantee 6: given the sequence, a scan depends on itself alone -- the replay with one scan per call.  Then the system without
    static blocks at 9 scans, where the stage runs on the wide column tile as bspatom_tdse_static's kernels do."""
    s, (a, err, obs, snaps, stats, (li, le, lf)) = gpu_run(prob, 3, 15, 9, 1)
    for q in (0, 4, 8):
        ra, rrows, rsnaps, rerrs = replay(prob, s, 1, li, lf, slice(q, q + 1))
        assert same(ra[0], a[q]) and same(rsnaps[:, 0], snaps[:, q]) and same(rrows[:, 0], obs[:, q])
        assert same(rerrs[:, 0], le[li[:, 3] > 0][:, q])
    # the scan alone under its own controller takes other steps: the sequence depends on all scans
    E, pairs, D, a0, fn, static = s
    alone = prob.tdse_adaptive(E, pairs, D, a0[:1], fn[:, :, :1], R.DT, static, R.TOL, R.MAX_LEVEL_TEST, nsub=R.NSUB, level0=R.LEVEL0, log_cap=LOG_CAP)
    note("tdse adaptive scans: %d attempts for scan 0 alone, %d for the nine" % (alone[2][5], stats[5]))
    for scheme in (0, 1):
        s, (a, err, obs, snaps, stats, (li, le, lf)) = gpu_run(prob, 3, 15, 9, scheme, blocks=False)
        ra, rrows, rsnaps, rerrs = replay(prob, s, scheme, li, lf)
        assert same(ra, a) and same(rsnaps, snaps) and same(rrows, obs) and same(rerrs, le[li[:, 3] > 0])
        assert np.all(obs[..., 4:].view(np.uint64) == 0) and stats[1] >= 1
        R.follows_rule(li, le, R.TOL, R.MAX_LEVEL_TEST, R.LEVEL0, nsteps=R.NSTEPS)


@pytest.mark.parametrize("scheme", [0, 1])
@pytest.mark.parametrize("nsub", [3, 5])
def test_field_parity_with_an_odd_nsub(prob, nsub, scheme):
    """nsub = 2 leaves x_s nsub, dt / nsub and the choice of the interval exact; with 3 and 5 node intervals per coarse step every one
    of them rounds (tests/test_tdse_adapt_cpu.py shows that a fused coordinate differs there).  (3, 15, 9): log_f against the float64
    restatement bit for bit, the rule, and the chain identity, which must not care."""
    nch, count, nscan = 3, 15, 9
    s = R.adapt_system(nch, count, nscan, nsub=nsub)
    E, pairs, D, a0, fn, static = s
    assert fn.shape == (R.NSTEPS * nsub + 1, 2, nscan)
    a, err, obs, snaps, stats, (li, le, lf) = prob.tdse_adaptive(E, pairs, D, a0, fn, R.DT, static, R.TOL, R.MAX_LEVEL_TEST, nsub=nsub,
                                                                 level0=R.LEVEL0, scheme=scheme, obs_every=1, snap_every=1, log_cap=LOG_CAP)
    assert stats[5] == len(li) and tuple(li[0, :3]) == (0, R.LEVEL0, 0)
    differ = 0
    for t, (n, m, j, flag) in enumerate(li.tolist()):
        assert same(lf[t], R.attempt_field(fn, R.DT, nsub, n, m, j)), (t, n, m, j)
        differ += not np.array_equal(R.fused_u(nsub, m, j), R.plain_u(nsub, m, j))
    assert differ >= 1
    R.follows_rule(li, le, R.TOL, R.MAX_LEVEL_TEST, R.LEVEL0, nsteps=R.NSTEPS)
    ra, rrows, rsnaps, rerrs = replay(prob, s, scheme, li, lf)
    assert same(ra, a) and same(rsnaps, snaps) and same(rrows, obs) and same(rerrs, le[li[:, 3] > 0])
    note("tdse adaptive nsub %d scheme %d: %d attempts, log_f bit for bit, %d of them at positions where a fused coordinate differs"
         % (nsub, scheme, len(li), differ))


@pytest.mark.parametrize("key", KEYS)
def test_fixed_step_identity(prob, key):
    """Guarantee 2: tol = +inf from level 0 is one bspatom_tdse_static call on the coarse grid with log_f as its table."""
    nch, count, nscan, scheme = key
    E, pairs, D, a0, fn, static = R.adapt_system(nch, count, nscan)
    a, err, obs, snaps, stats, (li, le, lf) = prob.tdse_adaptive(E, pairs, D, a0, fn, R.DT, static, np.inf, R.MAX_LEVEL_TEST, nsub=R.NSUB,
                                                                 scheme=scheme, obs_every=1, snap_every=1, log_cap=LOG_CAP)
    assert stats.tolist() == [R.NSTEPS, 0, 0, 0, 0, R.NSTEPS] and li.tolist() == [[n, 0, 0, 1] for n in range(R.NSTEPS)]
    sa, serr, sobs, ssnaps = prob.tdse_static(E, pairs, D, a0, lf, R.DT, static, scheme=scheme, obs_every=1, snap_every=1)
    assert same(a, sa) and same(err, serr) and same(obs, sobs) and same(snaps, ssnaps)
    assert same(err, le.max(axis=0))


@pytest.mark.parametrize("scheme", [0, 1])
def test_reproducibility(prob, scheme):
    """Guarantee 4 on (3, 15, 9): run to run, obs_every, snap_every, log_cap (0 included), the enqueue group size, the _dev variant."""
    nch, count, nscan = 3, 15, 9
    s, (a, err, obs, snaps, stats, (li, le, lf)) = gpu_run(prob, nch, count, nscan, scheme)
    E, pairs, D, a0, fn, static = s
    kw = dict(nsub=R.NSUB, level0=R.LEVEL0, scheme=scheme)
    run = lambda **k: prob.tdse_adaptive(E, pairs, D, a0, fn, R.DT, static, R.TOL, R.MAX_LEVEL_TEST, **kw, **k)
    b = run(obs_every=1, snap_every=1, log_cap=LOG_CAP)
    assert same(b[0], a) and same(b[1], err) and same(b[2], obs) and same(b[3], snaps) and same(b[4], stats)
    assert all(same(x, y) for x, y in zip(b[5], (li, le, lf)))
    b = run(obs_every=3, snap_every=2, log_cap=5)
    assert same(b[0], a) and same(b[1], err) and same(b[2], obs[host.obs_steps(R.NSTEPS, 3)]) and same(b[3], snaps[1::2]) and same(b[4], stats)
    assert all(same(x, y[:5]) for x, y in zip(b[5], (li, le, lf)))
    b = run()
    assert len(b) == 4 and same(b[0], a) and same(b[1], err) and same(b[2], stats) and b[3][0].shape == (0, 4)
    for group in (1, 7):
        capi.set_option("tdse_adapt_group", group)
        try:
            b = run(obs_every=1, snap_every=1, log_cap=LOG_CAP)
        finally:
            capi.set_option("tdse_adapt_group", 0)
        assert same(b[0], a) and same(b[1], err) and same(b[2], obs) and same(b[3], snaps) and same(b[4], stats) and same(b[5][1], le)
    # the _dev variant on torch tensors
    dev = "cuda:0"
    t_ = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    Ed, Dd, Wd, fd, ad = t_(E), t_(D), t_(static[2]), t_(fn), t_(a0)
    sd = torch.full((R.NSTEPS, nscan, nch, count), float("nan"), dtype=torch.complex128, device=dev)
    od = torch.full((R.NSTEPS + 1, nscan, nch, 6), float("nan"), dtype=torch.float64, device=dev)
    lid = torch.zeros((LOG_CAP, 4), dtype=torch.int32, device=dev)
    led = torch.zeros((LOG_CAP, nscan), dtype=torch.float64, device=dev)
    lfd = torch.zeros((LOG_CAP, 6, nscan), dtype=torch.complex128, device=dev)
    torch.cuda.synchronize()
    errd, statsd = prob.tdse_adaptive_dev(nch, count, Ed.data_ptr(), pairs, Dd.data_ptr(), nscan, R.NSTEPS, R.DT, fd.data_ptr(), ad.data_ptr(),
                                          (static[0], static[1], Wd.data_ptr()), R.TOL, R.MAX_LEVEL_TEST, R.NSUB, R.LEVEL0, scheme, 1,
                                          od.data_ptr(), 1, sd.data_ptr(), LOG_CAP, (lid.data_ptr(), led.data_ptr(), lfd.data_ptr()))
    nl = int(statsd[5])
    assert same(ad.cpu().numpy(), a) and same(errd, err) and same(statsd, stats) and same(od.cpu().numpy(), obs) and same(sd.cpu().numpy(), snaps)
    assert same(lid.cpu().numpy()[:nl], li) and same(led.cpu().numpy()[:nl], le) and same(lfd.cpu().numpy()[:nl], lf)


def test_staging_bound(prob):
    """Guarantee 4, the staging bound: 64 scans x 4 x 65 states make a snapshot of 260 KiB, so tdse_stage_mb = 1 cuts the four coarse
    steps into two groups; the same bits as under the default bound, with the log on and off."""
    nch, count, nscan = 4, 65, 64
    E, pairs, D, a0, fn, static = R.adapt_system(nch, count, nscan)
    kw = dict(nsub=R.NSUB, level0=R.LEVEL0, scheme=1, obs_every=1, snap_every=1)
    a, err, obs, snaps, stats, log = prob.tdse_adaptive(E, pairs, D, a0, fn, R.DT, static, R.TOL, R.MAX_LEVEL_TEST, log_cap=LOG_CAP, **kw)
    capi.set_option("tdse_stage_mb", 1)
    try:
        b = prob.tdse_adaptive(E, pairs, D, a0, fn, R.DT, static, R.TOL, R.MAX_LEVEL_TEST, log_cap=LOG_CAP, **kw)
        c = prob.tdse_adaptive(E, pairs, D, a0, fn, R.DT, static, R.TOL, R.MAX_LEVEL_TEST, log_cap=0, **kw)
    finally:
        capi.set_option("tdse_stage_mb", 0)
    assert same(b[0], a) and same(b[1], err) and same(b[2], obs) and same(b[3], snaps) and same(b[4], stats)
    assert all(same(x, y) for x, y in zip(b[5], log))
    assert same(c[0], a) and same(c[1], err) and same(c[2], obs) and same(c[3], snaps) and same(c[4], stats)
    assert stats[1] >= 1 and stats[3] >= 2


@pytest.mark.parametrize("key", KEYS)
def test_continuation(prob, key):
    """Guarantee 5: two coarse steps, then two more from the snapshot with level0 = stats[4] of the shorter run."""
    nch, count, nscan, scheme = key
    s, (a, err, obs, snaps, stats, (li, le, lf)) = gpu_run(prob, *key)
    E, pairs, D, a0, fn, static = s
    half = 2 * R.NSUB
    a1, e1, st1, log1 = prob.tdse_adaptive(E, pairs, D, a0, fn[:half + 1], R.DT, static, R.TOL, R.MAX_LEVEL_TEST, nsub=R.NSUB, level0=R.LEVEL0,
                                           scheme=scheme, log_cap=LOG_CAP)
    assert same(a1, snaps[1])
    a2, e2, o2, st2, log2 = prob.tdse_adaptive(E, pairs, D, a1, fn[half:], R.DT, static, R.TOL, R.MAX_LEVEL_TEST, nsub=R.NSUB, level0=int(st1[4]),
                                               scheme=scheme, obs_every=1, log_cap=LOG_CAP)
    assert same(a2, a) and same(np.maximum(e1, e2), err) and same(o2, obs[2:])
    assert st1[5] + st2[5] == stats[5] and st2[4] == stats[4] and same(np.concatenate([log1[1], log2[1]]), le)
    assert same(np.concatenate([log1[2], log2[2]]), lf)


# ---- 3 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", KEYS)
def test_the_log_shows_the_controller_at_work(prob, key):
    s, (a, err, obs, snaps, stats, (li, le, lf)) = gpu_run(prob, *key)
    rej, coarsen, levels, forced = R.features(li.tolist())
    note("tdse adaptive log %s: %d attempts, %d rejected, %d coarsenings, levels %s, err %.3g" % (key, len(li), rej, coarsen, sorted(set(li[:, 1].tolist())),
                                                                                             float(np.max(err))))
    assert rej >= 1 and coarsen >= 1 and levels >= 3
    assert float(np.max(err)) <= R.TOL and stats[2] == 0
    # the forced configuration: max_level = 1 cannot hold tol in the middle of the pulse
    s, (a, err, obs, snaps, stats, (li, le, lf)) = gpu_run(prob, *key, max_level=R.MAX_LEVEL_FORCED)
    assert stats[2] >= 1 and float(np.max(err)) > R.TOL and int(np.sum(li[:, 3] == 2)) == stats[2]
    assert [tuple(r) for r in li.tolist()] == long_log(*key, R.MAX_LEVEL_FORCED)
    R.follows_rule(li, le, R.TOL, R.MAX_LEVEL_FORCED, R.LEVEL0, nsteps=R.NSTEPS)


# ---- 4 ----------------------------------------------------------------------------------------------------------------
def test_argument_checks(prob):
    nch, count, nscan, nsteps = 3, 15, 9, R.NSTEPS
    E, pairs, D, a0, fn, static = R.adapt_system(nch, count, nscan)
    L = capi.lib()
    ci = np.array([p[0] for p in pairs], dtype=np.int32)
    cf = np.array([p[1] for p in pairs], dtype=np.int32)
    si = np.array([p[0] for p in static[0]], dtype=np.int32)
    sf = np.array([p[1] for p in static[0]], dtype=np.int32)
    sk, W = np.array(static[1], dtype=np.int32), static[2]
    ns = len(si)
    D = np.ascontiguousarray(D)
    dev = "cuda:0"
    Ed, Dd, fd, Wd = (torch.from_numpy(x).to(dev) for x in (E, D, fn, W))
    ad = torch.from_numpy(np.ascontiguousarray(a0)).to(dev)
    sd = torch.zeros((nsteps, nscan, nch, count), dtype=torch.complex128, device=dev)
    od = torch.zeros((nsteps + 1, nscan, nch, 6), dtype=torch.float64, device=dev)
    lid = torch.zeros((8, 4), dtype=torch.int32, device=dev)
    led = torch.zeros((8, nscan), dtype=torch.float64, device=dev)
    lfd = torch.zeros((8, 6, nscan), dtype=torch.complex128, device=dev)
    torch.cuda.synchronize()
    p_ = lambda x: x.ctypes.data_as(C.c_void_p)
    d_ = lambda x: C.c_void_p(x.data_ptr())
    a, snap, err = a0.copy(), np.zeros((nsteps, nscan, nch, count), dtype=np.complex128), np.zeros(nscan)
    obs, stats = np.zeros((nsteps + 1, nscan, nch, 6)), np.zeros(6, dtype=np.int64)
    li, le, lf = np.zeros((8, 4), dtype=np.int32), np.zeros((8, nscan)), np.zeros((8, 6, nscan), dtype=np.complex128)
    host_ptrs = (p_(E), p_(D), p_(fn), p_(a), p_(snap), p_(obs), p_(W), p_(li), p_(le), p_(lf))
    dev_ptrs = (d_(Ed), d_(Dd), d_(fd), d_(ad), d_(sd), d_(od), d_(Wd), d_(lid), d_(led), d_(lfd))
    for fn_, (Ep, Dp, fp, ap, sp, op, Wp, lip, lep, lfp) in ((L.bspatom_tdse_adaptive, host_ptrs), (L.bspatom_tdse_adaptive_dev, dev_ptrs)):
        good = [prob._h, nch, count, Ep, 2, p_(ci), p_(cf), Dp, nscan, nsteps, R.DT, fp, ap, 1, sp, p_(err), 1, op, 1, ns, p_(si), p_(sf),
                p_(sk), Wp, R.NSUB, R.TOL, R.MAX_LEVEL_TEST, R.LEVEL0, p_(stats), 8, lip, lep, lfp]
        sub = lambda pos, v: [v if i == pos else x for i, x in enumerate(good)]
        assert fn_(*good) == 0
        # what bspatom_tdse_static names
        for pos in (0, 3, 5, 6, 7, 11, 12):                        # p, E, ci, cf, D, fn (nsteps > 0), a
            assert fn_(*sub(pos, None)) == -2, pos
        for pos in (1, 2, 8):                                      # nch, count, nscan < 1
            assert fn_(*sub(pos, 0)) == -2 and fn_(*sub(pos, -1)) == -2, pos
        assert fn_(*sub(9, -1)) == -2 and fn_(*sub(4, -1)) == -2   # nsteps, npairs < 0
        assert fn_(*sub(13, -1)) == -2 and fn_(*sub(13, 0)) == -2  # snap_every < 0; snap given with snap_every = 0
        assert fn_(*sub(5, p_(cf))) == -2                          # ci == cf
        for bad in (float("nan"), float("inf")):
            assert fn_(*sub(10, bad)) == -2                        # dt not finite
        assert fn_(*sub(16, -1)) == -2 and fn_(*sub(16, 0)) == -2 and fn_(*sub(17, None)) == -2          # obs_every, obs
        for bad in (-1, 2):
            assert fn_(*sub(18, bad)) == -2                        # scheme outside {0, 1}
        assert fn_(*sub(19, -1)) == -2                             # nstat < 0
        for pos in (20, 21, 22, 23):
            assert fn_(*sub(pos, None)) == -2, pos                 # nstat > 0 without si, sf, skind or W
        # its own
        for bad in (0.0, -1e-6, float("nan"), -float("inf")):
            assert fn_(*sub(25, bad)) == -2, bad                   # tol not positive or NaN
        assert fn_(*sub(26, -1)) == -2                             # max_level < 0
        for bad in (-1, R.MAX_LEVEL_TEST + 1):
            assert fn_(*sub(27, bad)) == -2                        # level0 outside 0 .. max_level
        for bad in (0, -1):
            assert fn_(*sub(24, bad)) == -2                        # nsub < 1
        assert fn_(*sub(28, None)) == -2                           # stats
        assert fn_(*sub(29, -1)) == -2                             # log_cap < 0
        for pos in (30, 31, 32):
            assert fn_(*sub(pos, None)) == -2, pos                 # log_cap > 0 with a null log array
        assert fn_(*sub(26, 17)) == -5                             # more than 16 levels: unsupported
        # allowed: tol = +inf, max_level = 16 (level0 = 1 keeps it short), no log (then no arrays), no steps (then no nodes), the plain scheme
        assert fn_(*sub(25, float("inf"))) == 0
        assert fn_(*sub(26, 16)) == 0
        assert fn_(*[None if i in (30, 31, 32) else x for i, x in enumerate(sub(29, 0))]) == 0
        assert fn_(*[None if i == 11 else x for i, x in enumerate(sub(9, 0))]) == 0 and stats.tolist() == [0, 0, 0, 0, R.LEVEL0, 0]
        assert fn_(*sub(18, 0)) == 0
        assert fn_(*[None if i in (20, 21, 22, 23) else x for i, x in enumerate(sub(19, 0))]) == 0
        assert fn_(*good) == 0 and stats[5] > 0                    # a valid call afterwards
    assert np.all(np.isfinite(a)) and np.all(np.isfinite(ad.cpu().numpy().view(np.float64)))
    assert np.all(np.isfinite(obs)) and np.all(np.isfinite(od.cpu().numpy()))


# ---- 5 ----------------------------------------------------------------------------------------------------------------
def test_end_to_end():
    """tiny8 as in tests/test_gpu_tdse_static.py: the states of (0,0), (1,0) through host.tdse_system, the absorber through
    host.tdse_absorber, the ground state under a sin^2 pulse of amplitude 0.1 lasting 10 a.u., on 25 coarse steps of 0.4 with 8 node intervals each, Lawson
    steps, tol = 1e-8.  The norm along the rows and the yield against a fixed-step bspatom_tdse_static run at the deepest level the
    controller reached, on the same interpolated field: their difference lies within accepted * tol, the sum of the local estimates."""
    p = capi.Problem(input_from_case("tiny8"))
    _, info = p.solve(0, 2)
    assert np.all(info == 0)
    channels = [(0, 0), (1, 0)]
    E, pairs, D = host.tdse_system(p, channels, 1, 8, kind_pi=1)
    static = host.tdse_absorber(p, channels, 1, 8, lambda r: host.cap_profile(r, 8.0, 0.02))
    nsteps, dt, nsub, tol, max_level = 25, 0.4, 8, 1e-8, 4
    T = nsteps * dt
    f = lambda t: 0.1 * np.sin(np.pi * t / T) ** 2 * np.cos(0.6 * t)
    fn = host.field_nodes([f], None, 0.0, dt, nsteps, nsub)
    a0 = np.zeros((1, 2, 8), dtype=np.complex128)
    a0[0, 0, 0] = 1.0
    a, err, obs, stats, (li, le, lf) = p.tdse_adaptive(E, pairs, D, a0, fn, dt, static, tol, max_level, nsub=nsub, obs_every=1, log_cap=4096)
    assert stats[5] == len(li) and stats[2] == 0 and float(err[0]) <= tol
    deep = int(stats[3])
    fine = np.array([R.attempt_field(fn, dt, nsub, n, deep, j) for n in range(nsteps) for j in range(1 << deep)])
    sa, serr, sobs = p.tdse_static(E, pairs, D, a0, fine, float(np.ldexp(dt, -deep)), static, scheme=1, obs_every=1 << deep)
    p.close()
    bound = float(stats[0]) * tol
    n_ad, n_fx = obs[..., 0].sum(axis=-1), sobs[..., 0].sum(axis=-1)
    y_ad = host.tdse_yield(obs, dt, nsteps, 1).sum(axis=-1)
    y_fx = host.tdse_yield(sobs, np.ldexp(dt, -deep), nsteps << deep, 1 << deep).sum(axis=-1)
    dn, dy, da = float(np.max(np.abs(n_ad - n_fx))), float(np.max(np.abs(y_ad - y_fx))), float(np.max(np.abs(a - sa)))
    note("tdse adaptive end to end: %d accepted of %d attempts (%d at a fixed step of level %d), levels %s; norm(T) %.9g, yield %.6g; "
         "|norm - fixed| %.3g, |yield - fixed| %.3g, |a - fixed| %.3g, bound %.3g"
         % (stats[0], stats[5], nsteps << deep, deep, sorted(set(li[:, 1].tolist())), n_ad[-1, 0], y_ad[0], dn, dy, da, bound))
    assert obs.shape == sobs.shape == (nsteps + 1, 1, 2, 6) and n_ad[0, 0] == 1.0 and 0.0 < y_ad[0] < 1.0
    assert dn <= bound and dy <= bound
