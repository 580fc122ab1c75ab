"""bspatom_tdse_lawson / _dev (csrc/tdse.hip: the Lawson stage, observing and step kernels, tdse_phase_kernel) on the GPU against the
NumPy restatement tests/tdse_lawson_ref.py.

The yardstick is that of tests/test_gpu_tdse.py: the restatement run twice, in complex128 and in long double, and
    max|a_gpu - a_long| <= 8 max(max|a_128 - a_long|, eps),
err[q] likewise with the floor eps dt (tdse_ref.amp_bound / err_bound): the margin the project gives a different but equally stable
summation order.  The phases enter both sides from the same fp64 argument E (c_s dt); the device's sincos and NumPy's are each
within an ulp of it.  The observed rows are compared bit for bit with bspatom_tdse_observe on the same amplitudes, which
tests/test_gpu_tdse_observe.py checks against the definitions.  Never against the code under test.  Every test notes its ratio."""
import ctypes as C
import functools
import numpy as np
import pytest
import torch                               # first: its HIP runtime is the one the process uses
from test_gpu_stages import input_from_case, note

import tdse_lawson_ref
import tdse_ref
from bspatom_amd import capi, host

pytestmark = pytest.mark.gpu
EPS = tdse_ref.EPS
DT = 0.05


@pytest.fixture(scope="module")
def prob():
    p = capi.Problem(input_from_case("tiny8"))           # the handle gives the device and the stream only
    yield p
    p.close()


@functools.lru_cache(maxsize=None)
def system(nch, count, nscan, nsteps, pairs=None, phase=0.0):
    return tdse_ref.system(nch, count, nscan, nsteps, pairs=None if pairs is None else list(pairs), dt=DT, phase=phase)


@functools.lru_cache(maxsize=None)
def case(nch, count, nscan, nsteps, pairs=None, phase=0.0):
    """(system, complex128 Lawson restatement, long-double Lawson restatement), computed once and shared; nobody writes into it"""
    s = system(nch, count, nscan, nsteps, pairs, phase)
    r128, rlong = tdse_lawson_ref.both(*s, DT)
    return s, r128, rlong


def check(tag, a, err, r128, rlong, dt=DT):
    ba, be = tdse_ref.amp_bound(r128[0], rlong[0]), tdse_ref.err_bound(r128[1], rlong[1], dt)
    da = float(np.max(np.abs(a.astype(np.clongdouble) - rlong[0])))
    de = float(np.max(np.abs(err.astype(np.longdouble) - rlong[1])))
    note("tdse lawson %s: max|a - a_long| / bound = %.3g (restatement's own distance %.3g eps), |err - err_long| / bound = %.3g (err %.3g)"
         % (tag, da / ba, ba / 8.0 / EPS, de / be, float(np.max(err))))
    assert da <= ba, (tag, da, ba)
    assert de <= be, (tag, de, be)
    return da / ba


def same(x, y):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    return x.shape == y.shape and np.array_equal(x.view(np.uint64), y.view(np.uint64))


# ---- 1 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nch,count,nscan,nsteps", [(1, 20, 1, 40), (2, 1, 1, 100), (2, 16, 1, 40), (3, 17, 8, 40), (3, 15, 9, 40),
                                                    (4, 65, 3, 60)])
def test_parity_with_the_restatement(prob, nch, count, nscan, nsteps):
    """No pairs at all, one state per channel, exactly one MFMA tile, one row more, one row less with 9 scans (two column blocks,
    TN = 2), more than one row tile.  (3, 17, 8) runs with the field times exp(0.3 i): the conjugate matters."""
    phase = 0.3 if (nch, count, nscan) == (3, 17, 8) else 0.0
    (E, pairs, D, a0, field), r128, rlong = case(nch, count, nscan, nsteps, phase=phase)
    a, err = prob.tdse_lawson(E, pairs, D, a0, field, DT)
    assert a.shape == (nscan, nch, count) and err.shape == (nscan,)
    check("parity %s" % ((nch, count, nscan, nsteps),), a, err, r128, rlong)
    if nch == 1:
        exact = a0 * np.exp(-1j * E[None] * (nsteps * DT))
        got = float(np.max(np.abs(a - exact)))
        note("tdse lawson no pairs: |a - a0 exp(-i E t)| = %.3g eps, err %s" % (got / EPS, err))
        assert np.all(err == 0.0)
        assert got <= 64.0 * EPS
    else:
        assert float(np.max(np.abs(a - a0))) > 1e-3


# ---- 2 ----------------------------------------------------------------------------------------------------------------
def test_pair_lists(prob):
    """The star (0,1), (2,1), (1,3): a reversed pair and a channel with three neighbours.  Then the chain with its first pair
    given twice at half strength, and with its first pair reversed: within the bound of the plain list's restatement."""
    (E, pairs, D, a0, field), r128, rlong = case(4, 17, 2, 40, pairs=((0, 1), (2, 1), (1, 3)), phase=0.3)
    a, err = prob.tdse_lawson(E, pairs, D, a0, field, DT)
    check("star", a, err, r128, rlong)
    (E, pairs, D, a0, field), r128, rlong = case(3, 17, 2, 40)
    assert pairs == [(0, 1), (1, 2)]
    D2 = np.concatenate([D * np.array([0.5, 1.0])[:, None, None], 0.5 * D[:1]])
    a, err = prob.tdse_lawson(E, pairs + [(0, 1)], D2, a0, field, DT)
    check("repeated pair", a, err, r128, rlong)
    # real field (phase 0): the first pair in the other orientation with the transposed block is the same Hamiltonian
    a, err = prob.tdse_lawson(E, [(1, 0), (1, 2)], np.stack([D[0].T, D[1]]), a0, field, DT)
    check("reversed pair", a, err, r128, rlong)


# ---- 3 ----------------------------------------------------------------------------------------------------------------
def test_stiff_system(prob):
    """dt max|E| = 20, where the plain scheme diverges (tests/test_tdse_lawson_ref_cpu.py shows that on the CPU restatement; the
    diverging call is not run here): parity with the Lawson restatement, and the norm drifts no more than its truncation error."""
    E, pairs, D, a0, field = tdse_lawson_ref.stiff_system()
    assert DT * float(np.max(np.abs(E))) > 19.9
    r128, rlong = tdse_lawson_ref.both(E, pairs, D, a0, field, DT)
    a, err = prob.tdse_lawson(E, pairs, D, a0, field, DT)
    check("stiff", a, err, r128, rlong)
    drift = np.abs(np.sum(np.abs(a) ** 2, axis=(1, 2)) - 1.0)
    own = np.abs(np.sum(np.abs(rlong[0]) ** 2, axis=(1, 2)) - np.sum(np.abs(a0.astype(np.clongdouble)) ** 2, axis=(1, 2)))
    bound = 8.0 * float(np.max(own)) + 64.0 * EPS
    note("tdse lawson stiff: |sum |a|^2 - 1| = %.3g, bound %.3g (the long-double restatement drifts %.3g)" % (np.max(drift), bound, np.max(own)))
    assert np.all(np.isfinite(a)) and float(np.max(drift)) <= bound


# ---- 4 ----------------------------------------------------------------------------------------------------------------
def test_order_and_error_estimate(prob):
    """2 x 2 constant-field problem against the closed form: the error drops by 24 .. 40 from 50 to 100 steps, and err is within a
    factor 2 of the true error."""
    errs = []
    for nsteps in (50, 100):
        E, pairs, D, a0, field, dt, exact = tdse_ref.two_by_two(nsteps)
        a, est = prob.tdse_lawson(E, pairs, D, a0, field, dt)
        true = float(np.max(np.abs(a - exact)))
        note("tdse lawson 2 x 2, %d steps: error %.3g, err %.3g" % (nsteps, true, est[0]))
        assert 0.5 * true <= est[0] <= 2.0 * true
        errs.append(true)
    note("tdse lawson 2 x 2: error ratio %.3g" % (errs[0] / errs[1]))
    assert 24.0 <= errs[0] / errs[1] <= 40.0


# ---- 5 ----------------------------------------------------------------------------------------------------------------
def test_bit_identities(prob):
    E, pairs, D, a0, field = system(3, 15, 9, 40)
    a, err, snaps = prob.tdse_lawson(E, pairs, D, a0, field, DT, snap_every=20)
    assert snaps.shape == (2, 9, 3, 15) and float(np.max(err)) > 0.0
    # run to run
    a2, err2, snaps2 = prob.tdse_lawson(E, pairs, D, a0, field, DT, snap_every=20)
    assert same(a, a2) and same(err, err2) and same(snaps, snaps2)
    # a scan does not depend on its company (nine scans: two column blocks; alone: one)
    for q in (0, 4, 8):
        aq, eq = prob.tdse_lawson(E, pairs, D, a0[q:q + 1], field[:, :, q:q + 1], DT)
        assert same(aq[0], a[q]) and eq[0] == err[q], q
    # the snapshot after m of 2m steps is the m-step run; continuing from it gives the 2m result; the last snapshot is the result
    am, _ = prob.tdse_lawson(E, pairs, D, a0, field[:20], DT)
    assert same(am, snaps[0]) and same(a, snaps[1])
    ac, _ = prob.tdse_lawson(E, pairs, D, snaps[0], field[20:], DT)
    assert same(ac, a)
    # nsteps = 0 returns a as given
    a0_, e0_ = prob.tdse_lawson(E, pairs, D, a0, field[:0], DT)
    assert same(a0_, a0) and np.all(e0_ == 0.0)
    note("tdse lawson bit identities: run to run, scan alone, snapshot / continuation hold (max err %.3g)" % float(np.max(err)))


# ---- 6 ----------------------------------------------------------------------------------------------------------------
def test_observables(prob):
    """obs_every = 7 with snap_every = 7 on (3, 17, 2, 40): the amplitudes do not notice the observing stage 0, and every row has the
    bits of a bspatom_tdse_observe call without steps on the same amplitudes."""
    E, pairs, D, a0, field = system(3, 17, 2, 40)
    a, err, obs, snaps = prob.tdse_lawson(E, pairs, D, a0, field, DT, obs_every=7, snap_every=7)
    ap, errp, snapsp = prob.tdse_lawson(E, pairs, D, a0, field, DT, snap_every=7)
    steps = host.obs_steps(40, 7)
    assert steps == [0, 7, 14, 21, 28, 35, 40] and obs.shape == (7, 2, 3, 4) and snaps.shape == (5, 2, 3, 17)
    assert same(a, ap) and same(err, errp) and same(snaps, snapsp)
    row = lambda amp: prob.tdse_observe(E, pairs, D, amp, field[:0], DT)[2]
    for j in range(1, 6):
        r = row(snaps[j - 1])
        assert r.shape == (1, 2, 3, 4) and same(r[0], obs[j]), j
    assert same(row(a)[0], obs[6])
    assert same(row(a0)[0], obs[0])
    # a call without steps is bspatom_tdse_observe's
    a_, e_, o_ = prob.tdse_lawson(E, pairs, D, a0, field[:0], DT, obs_every=1)
    assert same(a_, a0) and np.all(e_ == 0.0) and same(o_, row(a0))
    assert float(np.max(np.abs(obs[..., 2]))) > 0.0
    note("tdse lawson observables: a, err, snaps independent of obs_every; 7 rows bit-equal to bspatom_tdse_observe on the same amplitudes")


# ---- 7 ----------------------------------------------------------------------------------------------------------------
def test_stage_bound_and_device_variant(prob):
    """A snapshot per step of 9 scans x 4 x 65 states is 73 KiB: tdse_stage_mb = 1 cuts the 60 steps into groups; the same bits.  The
    _dev variant on torch tensors equals the host variant."""
    E, pairs, D, a0, field = system(4, 65, 9, 60)
    a, err, obs, snaps = prob.tdse_lawson(E, pairs, D, a0, field, DT, obs_every=7, snap_every=1)
    assert snaps.shape == (60, 9, 4, 65) and same(snaps[-1], a)
    capi.set_option("tdse_stage_mb", 1)
    try:
        a1, err1, obs1, snaps1 = prob.tdse_lawson(E, pairs, D, a0, field, DT, obs_every=7, snap_every=1)
        a3, err3, snaps3 = prob.tdse_lawson(E, pairs, D, a0, field, DT, snap_every=7)
    finally:
        capi.set_option("tdse_stage_mb", 0)
    assert same(a1, a) and same(err1, err) and same(obs1, obs) and same(snaps1, snaps)
    assert same(a3, a) and same(err3, err) and same(snaps3, snaps[6::7])
    dev = "cuda:0"
    Ed, Dd = torch.from_numpy(E).to(dev), torch.from_numpy(np.ascontiguousarray(D)).to(dev)
    fd, ad = torch.from_numpy(field).to(dev), torch.from_numpy(np.ascontiguousarray(a0)).to(dev)
    sd = torch.full((60 // 7, 9, 4, 65), float("nan"), dtype=torch.complex128, device=dev)
    od = torch.full((len(host.obs_steps(60, 7)), 9, 4, 4), float("nan"), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    errd = prob.tdse_lawson_dev(4, 65, Ed.data_ptr(), pairs, Dd.data_ptr(), 9, 60, DT, fd.data_ptr(), ad.data_ptr(), 7, od.data_ptr(), 7,
                                sd.data_ptr())
    assert same(ad.cpu().numpy(), a) and same(errd, err) and same(sd.cpu().numpy(), snaps[6::7]) and same(od.cpu().numpy(), obs)
    ad.copy_(torch.from_numpy(np.ascontiguousarray(a0)))
    torch.cuda.synchronize()
    errd = prob.tdse_lawson_dev(4, 65, Ed.data_ptr(), pairs, Dd.data_ptr(), 9, 60, DT, fd.data_ptr(), ad.data_ptr())
    assert same(ad.cpu().numpy(), a) and same(errd, err)
    note("tdse lawson staging bound and _dev variant: bit-identical (max err %.3g)" % float(np.max(err)))


# ---- 8 ----------------------------------------------------------------------------------------------------------------
def test_end_to_end():
    """Solve l = 0 .. 2 (nfun = 64, k = 7), couple ALL 64 states of (0,0), (1,0), (2,0) through host.tdse_system, start in the ground
    state, 200 steps of 0.05 under the pulse of test_gpu_tdse.py's end-to-end test: dt max|E| is about 19.8 (the box spectrum reaches
    396), a run the plain call cannot do; against the Lawson restatement fed the same E and D."""
    p = capi.Problem(input_from_case("dip_len_lin", nfun=64, k=7, lmax=2))
    assert p.lmax == 2
    _, info = p.solve(0, 3)
    assert np.all(info == 0)
    E, pairs, D = host.tdse_system(p, [(0, 0), (1, 0), (2, 0)], 1, 64, kind_pi=1)
    assert E.shape == (3, 64) and D.shape == (2, 64, 64)
    stiff = DT * float(np.max(np.abs(E)))
    assert stiff > 4.0, stiff
    nsteps, T = 200, 200 * DT
    pulse = lambda t: 0.05 * np.sin(np.pi * t / T) ** 2 * np.cos(0.5 * t)
    field = host.field_table([pulse], 0.0, DT, nsteps)
    a0 = np.zeros((1, 3, 64), dtype=np.complex128)
    a0[0, 0, 0] = 1.0
    a, err = p.tdse_lawson(E, pairs, D, a0, field, DT)
    p.close()
    r128, rlong = tdse_lawson_ref.both(E, pairs, D, a0, field, DT)
    check("end to end (dt max|E| = %.3g)" % stiff, a, err, r128, rlong)
    excited = 1.0 - abs(a[0, 0, 0]) ** 2
    note("tdse lawson end to end: population outside the ground state %.3g, norm drift %.3g" % (excited, abs(np.sum(np.abs(a) ** 2) - 1)))
    assert 1e-6 < excited < 1.0


# ---- 9 ----------------------------------------------------------------------------------------------------------------
def test_argument_checks(prob):
    E, pairs, D, a0, field = system(3, 15, 9, 40)
    L = capi.lib()
    nch, count, nscan, nsteps = 3, 15, 9, 4
    field = np.ascontiguousarray(field[:nsteps])
    ci = np.array([p[0] for p in pairs], dtype=np.int32)
    cf = np.array([p[1] for p in pairs], dtype=np.int32)
    D = np.ascontiguousarray(D)
    dev = "cuda:0"
    Ed, Dd, fd = torch.from_numpy(E).to(dev), torch.from_numpy(D).to(dev), torch.from_numpy(field).to(dev)
    ad = torch.from_numpy(np.ascontiguousarray(a0)).to(dev)
    sd = torch.zeros((4, nscan, nch, count), dtype=torch.complex128, device=dev)
    od = torch.zeros((5, nscan, nch, 4), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    p_ = lambda x: x.ctypes.data_as(C.c_void_p)
    d_ = lambda x: C.c_void_p(x.data_ptr())
    a, snap, err = a0.copy(), np.zeros((4, nscan, nch, count), dtype=np.complex128), np.zeros(nscan)
    obs = np.zeros((5, nscan, nch, 4))
    want_a, want_err = prob.tdse_lawson(E, pairs, D, a0, field, DT)
    for fn, dvc, (Ep, Dp, fp, ap, sp, op) in ((L.bspatom_tdse_lawson, False, (p_(E), p_(D), p_(field), p_(a), p_(snap), p_(obs))),
                                              (L.bspatom_tdse_lawson_dev, True, (d_(Ed), d_(Dd), d_(fd), d_(ad), d_(sd), d_(od)))):
        good = [prob._h, nch, count, Ep, 2, p_(ci), p_(cf), Dp, nscan, nsteps, DT, fp, ap, 1, sp, p_(err), 1, op]
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
        assert fn(*sub(5, p_(cf))) == -2                           # ci == cf
        for bad in (float("nan"), float("inf"), -float("inf")):
            assert fn(*sub(10, bad)) == -2                         # dt not finite
        assert fn(*sub(16, -1)) == -2                              # obs_every < 0
        assert fn(*sub(16, 0)) == -2                               # obs given with obs_every = 0
        assert fn(*sub(17, None)) == -2                            # obs_every >= 1 without obs
        # allowed: no snapshots, no error estimate, no pairs, no steps (then no field either)
        assert fn(*[None if i in (14, 15) else x for i, x in enumerate(sub(13, 0))]) == 0
        assert fn(*[None if i in (5, 6, 7) else x for i, x in enumerate(sub(4, 0))]) == 0
        assert fn(*[None if i == 11 else x for i, x in enumerate(sub(9, 0))]) == 0
        # obs_every = 0 without obs propagates only: the bits of the run without observables
        if dvc:
            ad.copy_(torch.from_numpy(np.ascontiguousarray(a0)))
            torch.cuda.synchronize()
        else:
            a[...] = a0
        err[:] = -1.0
        assert fn(*[None if i == 17 else x for i, x in enumerate(sub(16, 0))]) == 0
        got = ad.cpu().numpy() if dvc else a
        assert same(got, want_a) and same(err, want_err)
        assert fn(*good) == 0                                      # a valid call afterwards
    assert np.all(np.isfinite(a)) and np.all(np.isfinite(ad.cpu().numpy().view(np.float64)))
    assert np.all(np.isfinite(obs)) and np.all(np.isfinite(od.cpu().numpy()))
