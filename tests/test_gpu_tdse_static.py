"""bspatom_tdse_static / _dev (csrc/tdse_static.hip: the stage with static entries, its observing stage 0, the reduction to rows of 6)
on the GPU against the NumPy restatement tests/tdse_static_ref.py.

The yardstick is that of tests/test_gpu_tdse.py: the restatement run twice, in complex128 and in long double, and
    max|a_gpu - a_long| <= 8 max(max|a_128 - a_long|, eps),
err[q] likewise with the floor eps dt (tdse_ref.amp_bound / err_bound).  The entries k = 4, 5 of a row are checked against the
long-double definition on the run's own snapshots with the bound tests/test_gpu_tdse_observe.py gives z_c,
    |obs_gpu - obs_long| <= (count (nstat + 1) + 16) eps M_k,
M_k the largest sum of the moduli of a row's terms; k = 0 .. 3 bit for bit against bspatom_tdse_observe on the same amplitudes.
Never against the code under test.  Every test notes its ratio."""
import ctypes as C
import functools
import numpy as np
import pytest
import torch                               # first: its HIP runtime is the one the process uses
from test_gpu_stages import input_from_case, note

import tdse_lawson_ref
import tdse_ref
import tdse_static_ref
from bspatom_amd import capi, host

pytestmark = pytest.mark.gpu
EPS = tdse_ref.EPS
DT = 0.05
SHAPES = [(2, 1, 1, 60), (2, 16, 1, 40), (3, 17, 8, 40), (3, 15, 9, 40), (4, 65, 3, 40)]


@pytest.fixture(scope="module")
def prob():
    p = capi.Problem(input_from_case("tiny8"))           # the handle gives the device and the stream only
    yield p
    p.close()


@functools.lru_cache(maxsize=None)
def system(nch, count, nscan, nsteps, driven=True):
    """(E, pairs, D, a0, field, static) computed once and shared; nobody writes into it.  (3, 17, 8) runs with the field times
    exp(0.3 i).  driven = False: the same system without its pairs, the static blocks alone."""
    phase = 0.3 if (nch, count, nscan) == (3, 17, 8) else 0.0
    E, pairs, D, a0, field = tdse_ref.system(nch, count, nscan, nsteps, dt=DT, phase=phase)
    if not driven:
        pairs, D = [], np.zeros((0, count, count))
    return E, pairs, D, a0, field, tdse_static_ref.static_system(nch, count)


@functools.lru_cache(maxsize=None)
def case(nch, count, nscan, nsteps, scheme, driven=True):
    """(system, complex128 restatement, long-double restatement)"""
    s = system(nch, count, nscan, nsteps, driven)
    r128, rlong = tdse_static_ref.both(*s[:5], DT, static=s[5], scheme=scheme)
    return s, r128, rlong


def check(tag, a, err, r128, rlong, dt=DT):
    ba, be = tdse_ref.amp_bound(r128[0], rlong[0]), tdse_ref.err_bound(r128[1], rlong[1], dt)
    da = float(np.max(np.abs(a.astype(np.clongdouble) - rlong[0])))
    de = float(np.max(np.abs(err.astype(np.longdouble) - rlong[1])))
    note("tdse static %s: max|a - a_long| / bound = %.3g (restatement's own distance %.3g eps), |err - err_long| / bound = %.3g (err %.3g)"
         % (tag, da / ba, ba / 8.0 / EPS, de / be, float(np.max(err))))
    assert da <= ba, (tag, da, ba)
    assert de <= be, (tag, de, be)
    return da / ba


def same(x, y):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    return x.shape == y.shape and np.array_equal(x.view(np.uint64), y.view(np.uint64))


def norms(obs):
    return np.asarray(obs)[..., 0].sum(axis=-1)


# ---- 1 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", [0, 1])
@pytest.mark.parametrize("key", SHAPES + [(2, 16, 1, 40, False)])
def test_parity_with_the_restatement(prob, key, scheme):
    """One state per channel, exactly one MFMA tile, one row more with 8 scans and a complex field, one row less with 9 scans (two
    column blocks), two row tiles; then the static blocks alone (npairs = 0).  The lists of tdse_static_ref.static_system: channels
    without a static block, with one kind-1 block, with a kind-0 and a kind-1 block, and a cross-channel kind-0 pair X, X^T."""
    (E, pairs, D, a0, field, static), r128, rlong = case(*key[:4], scheme, *key[4:])
    a, err = prob.tdse_static(E, pairs, D, a0, field, DT, static, scheme=scheme)
    assert a.shape == a0.shape and err.shape == (key[2],)
    check("parity %s scheme %d" % (key, scheme), a, err, r128, rlong)
    # the blocks are felt, and they absorb
    plain = (prob.tdse_lawson if scheme else prob.tdse_propagate)(E, pairs, D, a0, field, DT)[0]
    assert float(np.max(np.abs(a - plain))) > 1e-3
    assert np.all(np.sum(np.abs(a) ** 2, axis=(1, 2)) < 1.0 - 1e-3)


# ---- 2 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", [0, 1])
@pytest.mark.parametrize("key", [(2, 1, 1, 60), (3, 15, 9, 40), (4, 65, 3, 40)])
def test_rows(prob, key, scheme):
    """obs_every = 1 with snap_every = 1: the rows describe [a0, snaps[0], .., snaps[-1]] of the same run."""
    nch, count, nscan, nsteps = key
    E, pairs, D, a0, field, static = system(*key)
    a, err, obs, snaps = prob.tdse_static(E, pairs, D, a0, field, DT, static, scheme=scheme, obs_every=1, snap_every=1)
    assert obs.shape == (nsteps + 1, nscan, nch, 6) and same(a, snaps[-1])
    states = np.concatenate([a0[None], snaps])
    ref = tdse_static_ref.observables(E, pairs, D, static, states, np.longdouble, np.clongdouble)
    M = tdse_static_ref.static_magnitudes(static, states)
    diff = np.abs(obs.astype(np.longdouble) - ref).reshape(-1, 6).max(axis=0)[4:]
    bound = (count * (len(static[0]) + 1) + 16) * np.longdouble(EPS) * M
    note("tdse static rows %s scheme %d: |s - s_long| / bound = %.3g %.3g (M = %.3g %.3g)"
         % (key, scheme, float(diff[0] / bound[0]), float(diff[1] / bound[1]), float(M[0]), float(M[1])))
    assert diff[0] <= bound[0] and diff[1] <= bound[1]
    assert float(np.max(np.abs(obs[..., 4]))) > 0.0 and float(np.min(obs[..., 5])) < 0.0
    # channels no static block ends in have s = 0 exactly
    for c in set(range(nch)) - {f for _, f in static[0]}:
        assert np.all(obs[:, :, c, 4:] == 0.0)
    # k = 0 .. 3: a bspatom_tdse_observe call without steps on the same amplitudes, every state of every scan as one scan
    packets = states.reshape(-1, nch, count)
    o4 = prob.tdse_observe(E, pairs, D, packets, np.zeros((0, 6, len(packets)), dtype=np.complex128), DT, obs_every=1)[2]
    assert same(o4[0].reshape(nsteps + 1, nscan, nch, 4), obs[..., :4])
    # and a call of its own without steps gives the whole row
    a_, e_, o6 = prob.tdse_static(E, pairs, D, snaps[7], field[:0], DT, static, scheme=scheme, obs_every=1)
    assert o6.shape == (1, nscan, nch, 6) and same(o6[0], obs[8]) and same(a_, snaps[7]) and np.all(e_ == 0.0)


# ---- 3 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", [0, 1])
def test_bit_identities(prob, scheme):
    E, pairs, D, a0, field, static = system(3, 15, 9, 40)
    nch, count, nscan, nsteps = 3, 15, 9, 40
    # no static blocks: the bits of bspatom_tdse_observe / bspatom_tdse_lawson, zeros in k = 4, 5
    other = prob.tdse_lawson if scheme else prob.tdse_observe
    wa, werr, wobs, wsnaps = other(E, pairs, D, a0, field, DT, obs_every=7, snap_every=20)
    for none in (None, ([], [], np.zeros((0, count, count)))):
        a, err, obs, snaps = prob.tdse_static(E, pairs, D, a0, field, DT, none, scheme=scheme, obs_every=7, snap_every=20)
        assert same(a, wa) and same(err, werr) and same(snaps, wsnaps) and same(obs[..., :4], wobs)
        assert np.all(obs[..., 4:].view(np.uint64) == 0)
    a, err = prob.tdse_static(E, pairs, D, a0, field, DT, None, scheme=scheme)
    assert same(a, wa) and same(err, werr)
    # with the blocks: run to run
    a, err, obs, snaps = prob.tdse_static(E, pairs, D, a0, field, DT, static, scheme=scheme, obs_every=1, snap_every=20)
    a2, err2, obs2, snaps2 = prob.tdse_static(E, pairs, D, a0, field, DT, static, scheme=scheme, obs_every=1, snap_every=20)
    assert same(a, a2) and same(err, err2) and same(obs, obs2) and same(snaps, snaps2)
    assert float(np.max(err)) > 0.0 and not same(a, wa)
    # scan 4 of nine (two column blocks) and the same scan alone (one)
    aq, eq, oq = prob.tdse_static(E, pairs, D, a0[4:5], field[:, :, 4:5], DT, static, scheme=scheme, obs_every=1)
    assert same(aq[0], a[4]) and eq[0] == err[4] and same(oq[:, 0], obs[:, 4])
    # the snapshot after 20 of 40 steps is the 20-step run, the last one the result
    am, _ = prob.tdse_static(E, pairs, D, a0, field[:20], DT, static, scheme=scheme)
    assert same(am, snaps[0]) and same(a, snaps[1])
    # obs_every = 7: the rows obs_steps(40, 7) of the full run; nothing else changes; nor without rows
    a7, err7, obs7 = prob.tdse_static(E, pairs, D, a0, field, DT, static, scheme=scheme, obs_every=7)
    steps7 = host.obs_steps(nsteps, 7)
    assert same(obs7, obs[steps7]) and same(a7, a) and same(err7, err)
    a0_, err0_ = prob.tdse_static(E, pairs, D, a0, field, DT, static, scheme=scheme)
    assert same(a0_, a) and same(err0_, err)
    # the _dev variant on torch tensors
    dev = "cuda:0"
    Ed, Dd = torch.from_numpy(E).to(dev), torch.from_numpy(np.ascontiguousarray(D)).to(dev)
    Wd = torch.from_numpy(static[2]).to(dev)
    fd, ad = torch.from_numpy(field).to(dev), torch.from_numpy(np.ascontiguousarray(a0)).to(dev)
    sd = torch.full((2, nscan, nch, count), float("nan"), dtype=torch.complex128, device=dev)
    od = torch.full((len(steps7), nscan, nch, 6), float("nan"), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    errd = prob.tdse_static_dev(nch, count, Ed.data_ptr(), pairs, Dd.data_ptr(), nscan, nsteps, DT, fd.data_ptr(), ad.data_ptr(),
                                (static[0], static[1], Wd.data_ptr()), scheme, 7, od.data_ptr(), 20, sd.data_ptr())
    assert same(ad.cpu().numpy(), a) and same(errd, err) and same(od.cpu().numpy(), obs[steps7]) and same(sd.cpu().numpy(), snaps)
    note("tdse static bit identities scheme %d: nstat = 0, run to run, scan alone, snapshot, obs_every, _dev hold (max err %.3g)"
         % (scheme, float(np.max(err))))


@pytest.mark.parametrize("scheme", [0, 1])
def test_staging_bound(prob, scheme):
    """A snapshot per step of 9 scans x 4 x 65 states is 73 KiB: tdse_stage_mb = 1 cuts the 40 steps into groups; the same bits."""
    E, pairs, D, a0, field = tdse_ref.system(4, 65, 9, 40, dt=DT)
    static = tdse_static_ref.static_system(4, 65)
    a, err, obs, snaps = prob.tdse_static(E, pairs, D, a0, field, DT, static, scheme=scheme, obs_every=1, snap_every=1)
    capi.set_option("tdse_stage_mb", 1)
    try:
        a1, err1, obs1, snaps1 = prob.tdse_static(E, pairs, D, a0, field, DT, static, scheme=scheme, obs_every=1, snap_every=1)
        a3, err3, obs3, snaps3 = prob.tdse_static(E, pairs, D, a0, field, DT, static, scheme=scheme, obs_every=7, snap_every=3)
    finally:
        capi.set_option("tdse_stage_mb", 0)
    assert same(a1, a) and same(err1, err) and same(obs1, obs) and same(snaps1, snaps)
    assert same(a3, a) and same(err3, err) and same(obs3, obs[host.obs_steps(40, 7)]) and same(snaps3, snaps[2::3])


# ---- 4 ----------------------------------------------------------------------------------------------------------------
def yield_gap(obs, nsteps, obs_every):
    """|yield - (norm(0) - norm(T))| per scan from rows of 6, in the rows' own arithmetic: the trapezoid's quadrature error"""
    obs = np.asarray(obs)
    h = obs.dtype.type(DT) * obs_every
    rate = -2 * obs[..., 5]
    y = h * (rate.sum(axis=0) - (rate[0] + rate[-1]) / 2)
    n = obs[..., 0].sum(axis=-1)
    return np.abs(y.sum(axis=-1) - (n[0] - n[-1]))


@pytest.mark.parametrize("scheme", [0, 1])
def test_yield(prob, scheme):
    """(3, 17, 2, 80), absorbers on channels 1 and 2: the yield of the rows and the norm that is gone differ by the trapezoid's error,
    which the long-double restatement's own rows measure; the GPU rows stay within twice that."""
    E, pairs, D, a0, field = tdse_ref.system(3, 17, 2, 80, dt=DT)
    P = tdse_static_ref.absorbers(3, 17, range(2))
    static = ([(1, 1), (2, 2)], [1, 1], np.stack(P))
    rlong = tdse_static_ref.propagate(E, pairs, D, a0, field, DT, static=static, scheme=scheme, rdtype=np.longdouble,
                                      cdtype=np.clongdouble, obs_every=1)
    dref = yield_gap(rlong[2], 80, 1).astype(np.float64)
    a, err, obs = prob.tdse_static(E, pairs, D, a0, field, DT, static, scheme=scheme, obs_every=1)
    y = host.tdse_yield(obs, DT, 80, 1)
    n = norms(obs)
    gap = np.abs(y.sum(axis=-1) - (n[0] - n[-1]))
    note("tdse static yield scheme %d: yield %s, norm(T) %s, |yield - lost norm| %s against the restatement's %s"
         % (scheme, y.sum(-1), n[-1], gap, dref))
    assert y.shape == (2, 3) and np.all(y[:, 0] == 0.0) and np.all(y[:, 1:] > 0.0)
    assert np.all(gap <= 2.0 * dref + 64.0 * EPS)
    assert np.all(np.abs(gap - yield_gap(obs, 80, 1)) <= 64.0 * EPS)
    assert np.all(np.diff(n, axis=0) < 0.0)
    assert same(host.tdse_static_rates(obs), 2.0 * obs[..., 5])


# ---- 5 ----------------------------------------------------------------------------------------------------------------
def test_stiff_system(prob):
    """tdse_lawson_ref.stiff_system (dt max|E| = 20) with an absorber on the five moved states of every channel, Lawson steps: parity
    with the restatement, finite, and the norm only falls.  The diverging plain call is not run."""
    E, pairs, D, a0, field = tdse_lawson_ref.stiff_system()
    assert DT * float(np.max(np.abs(E))) > 19.9
    W = np.zeros((3, 17, 17))
    for c, P in enumerate(tdse_static_ref.absorbers(3, 5, range(3))):
        W[c, 12:, 12:] = P
    static = ([(c, c) for c in range(3)], [1, 1, 1], W)
    r128, rlong = tdse_static_ref.both(E, pairs, D, a0, field, DT, static=static, scheme=1)
    a, err, obs = prob.tdse_static(E, pairs, D, a0, field, DT, static, scheme=1, obs_every=1)
    check("stiff", a, err, r128, rlong)
    n = norms(obs)
    note("tdse static stiff: norm %s -> %s" % (n[0], n[-1]))
    assert np.all(np.isfinite(a)) and np.all(np.isfinite(obs)) and np.all(np.diff(n, axis=0) < 0.0)


# ---- 6 ----------------------------------------------------------------------------------------------------------------
def test_end_to_end():
    """tiny8 (nfun = 8, rb = 12): solve l = 0, 1, all 8 states of (0,0), (1,0) through host.tdse_system, the absorber
    0.02 (r - 8)^2 through host.tdse_absorber, start in the ground state, 200 Lawson steps of 0.05 under a pulse."""
    p = capi.Problem(input_from_case("tiny8"))
    assert p.lmax == 1
    _, info = p.solve(0, 2)
    assert np.all(info == 0)
    channels = [(0, 0), (1, 0)]
    E, pairs, D = host.tdse_system(p, channels, 1, 8, kind_pi=1)
    static = host.tdse_absorber(p, channels, 1, 8, lambda r: host.cap_profile(r, 8.0, 0.02))
    assert E.shape == (2, 8) and D.shape == (1, 8, 8) and static[2].shape == (2, 8, 8) and static[0] == [(0, 0), (1, 1)]
    assert float(np.max(np.abs(static[2] - static[2].transpose(0, 2, 1)))) <= 64 * EPS and np.all(np.diagonal(static[2], 0, 1, 2) > 0)
    nsteps, T = 200, 200 * DT
    pulse = lambda t: 0.1 * np.sin(np.pi * t / T) ** 2 * np.cos(0.6 * t)
    field = host.field_table([pulse], 0.0, DT, nsteps)
    a0 = np.zeros((1, 2, 8), dtype=np.complex128)
    a0[0, 0, 0] = 1.0
    a, err, obs = p.tdse_static(E, pairs, D, a0, field, DT, static, obs_every=1)
    p.close()
    r128, rlong = tdse_static_ref.both(E, pairs, D, a0, field, DT, static=static, scheme=1, obs_every=1)
    check("end to end", a, err, r128, rlong)
    y = host.tdse_yield(obs, DT, nsteps, 1).sum(axis=-1)
    n = norms(obs)
    dref = yield_gap(rlong[2], nsteps, 1).astype(np.float64)
    gap = np.abs(y + n[-1] - 1.0)
    note("tdse static end to end: yield %.6g, norm(T) %.6g, |yield + norm(T) - 1| = %.3g against the restatement's %.3g"
         % (y[0], n[-1, 0], gap[0], dref[0]))
    assert n[0, 0] == 1.0 and 0.0 < y[0] < 1.0
    assert np.all(gap <= 2.0 * dref + 64.0 * EPS)


# ---- 7 ----------------------------------------------------------------------------------------------------------------
def test_argument_checks(prob):
    E, pairs, D, a0, field, static = system(3, 15, 9, 40)
    L = capi.lib()
    nch, count, nscan, nsteps = 3, 15, 9, 4
    field = np.ascontiguousarray(field[:nsteps])
    ci = np.array([p[0] for p in pairs], dtype=np.int32)
    cf = np.array([p[1] for p in pairs], dtype=np.int32)
    si = np.array([p[0] for p in static[0]], dtype=np.int32)
    sf = np.array([p[1] for p in static[0]], dtype=np.int32)
    sk, W = np.array(static[1], dtype=np.int32), static[2]
    ns = len(si)
    D = np.ascontiguousarray(D)
    dev = "cuda:0"
    Ed, Dd, fd, Wd = (torch.from_numpy(x).to(dev) for x in (E, D, field, W))
    ad = torch.from_numpy(np.ascontiguousarray(a0)).to(dev)
    sd = torch.zeros((4, nscan, nch, count), dtype=torch.complex128, device=dev)
    od = torch.zeros((5, nscan, nch, 6), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    p_ = lambda x: x.ctypes.data_as(C.c_void_p)
    d_ = lambda x: C.c_void_p(x.data_ptr())
    a, snap, err = a0.copy(), np.zeros((4, nscan, nch, count), dtype=np.complex128), np.zeros(nscan)
    obs = np.zeros((5, nscan, nch, 6))
    for fn, (Ep, Dp, fp, ap, sp, op, Wp) in ((L.bspatom_tdse_static, (p_(E), p_(D), p_(field), p_(a), p_(snap), p_(obs), p_(W))),
                                             (L.bspatom_tdse_static_dev, (d_(Ed), d_(Dd), d_(fd), d_(ad), d_(sd), d_(od), d_(Wd)))):
        good = [prob._h, nch, count, Ep, 2, p_(ci), p_(cf), Dp, nscan, nsteps, DT, fp, ap, 1, sp, p_(err), 1, op, 1, ns, p_(si), p_(sf),
                p_(sk), Wp]
        sub = lambda pos, v: [v if i == pos else x for i, x in enumerate(good)]
        assert fn(*good) == 0
        for pos in (0, 3, 5, 6, 7, 11, 12):                        # p, E, ci, cf, D, field, a
            assert fn(*sub(pos, None)) == -2, pos
        for pos in (1, 2, 8):                                      # nch, count, nscan < 1
            assert fn(*sub(pos, 0)) == -2 and fn(*sub(pos, -1)) == -2, pos
        assert fn(*sub(9, -1)) == -2                               # nsteps < 0
        assert fn(*sub(4, -1)) == -2                               # npairs < 0
        assert fn(*sub(13, -1)) == -2                              # snap_every < 0
        assert fn(*sub(13, 0)) == -2                               # snap given with snap_every = 0
        for bad in (np.array([0, 3], dtype=np.int32), np.array([-1, 1], dtype=np.int32)):     # a channel outside 0 .. nch-1
            assert fn(*sub(5, p_(bad))) == -2 and fn(*sub(6, p_(bad))) == -2
        assert fn(*sub(5, p_(cf))) == -2                           # ci == cf: still an error among the driven pairs
        for bad in (float("nan"), float("inf"), -float("inf")):
            assert fn(*sub(10, bad)) == -2                         # dt not finite
        assert fn(*sub(16, -1)) == -2                              # obs_every < 0
        assert fn(*sub(16, 0)) == -2                               # obs given with obs_every = 0
        assert fn(*sub(17, None)) == -2                            # obs_every >= 1 without obs
        for bad in (-1, 2):
            assert fn(*sub(18, bad)) == -2                         # scheme outside {0, 1}
        assert fn(*sub(19, -1)) == -2                              # nstat < 0
        for pos in (20, 21, 22, 23):
            assert fn(*sub(pos, None)) == -2, pos                  # nstat > 0 without si, sf, skind or W
        for bad in (np.array([0, 3] + [0] * (ns - 2), dtype=np.int32), np.array([-1, 1] + [0] * (ns - 2), dtype=np.int32)):
            assert fn(*sub(20, p_(bad))) == -2 and fn(*sub(21, p_(bad))) == -2                # a channel outside 0 .. nch-1
        for bad in (np.array([2] + [0] * (ns - 1), dtype=np.int32), np.array([0] * (ns - 1) + [-1], dtype=np.int32)):
            assert fn(*sub(22, p_(bad))) == -2                     # skind outside {0, 1}
        # allowed: the plain scheme, no static blocks (then no lists either), no pairs, no steps, no snapshots and no estimate
        assert fn(*sub(18, 0)) == 0
        assert fn(*[None if i in (20, 21, 22, 23) else x for i, x in enumerate(sub(19, 0))]) == 0
        assert fn(*[None if i in (5, 6, 7) else x for i, x in enumerate(sub(4, 0))]) == 0
        assert fn(*[None if i == 11 else x for i, x in enumerate(sub(9, 0))]) == 0
        assert fn(*[None if i in (14, 15) else x for i, x in enumerate(sub(13, 0))]) == 0
        assert fn(*[None if i == 17 else x for i, x in enumerate(sub(16, 0))]) == 0
        assert fn(*good) == 0                                      # a valid call afterwards
    assert np.all(np.isfinite(a)) and np.all(np.isfinite(ad.cpu().numpy().view(np.float64)))
    assert np.all(np.isfinite(obs)) and np.all(np.isfinite(od.cpu().numpy()))
