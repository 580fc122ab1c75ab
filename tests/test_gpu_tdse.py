"""bspatom_tdse_propagate / _dev (csrc/tdse.hip) on the GPU against the NumPy restatement tests/tdse_ref.py.

The yardstick is the restatement run twice, in complex128 and in long double (64-bit mantissa); the library must lie within
    max|a_gpu - a_long| <= 8 max(max|a_128 - a_long|, eps)
of the long-double result, and err[q] likewise with the floor eps dt: the factor 8 is for a different but equally stable summation
order (MFMA K order and FMA against NumPy's sums).  Never against the code under test.  Every test notes its measured ratio."""
import ctypes as C
import functools
import numpy as np
import pytest
import torch                               # first: its HIP runtime is the one the process uses
from test_gpu_stages import input_from_case, note

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
def case(nch, count, nscan, nsteps, pairs=None, phase=0.0):
    """(system, complex128 restatement, long-double restatement), computed once and shared; nobody writes into it"""
    s = tdse_ref.system(nch, count, nscan, nsteps, pairs=None if pairs is None else list(pairs), dt=DT, phase=phase)
    r128, rlong = tdse_ref.both(*s, DT)
    return s, r128, rlong


def check(tag, a, err, r128, rlong, dt=DT):
    ba, be = tdse_ref.amp_bound(r128[0], rlong[0]), tdse_ref.err_bound(r128[1], rlong[1], dt)
    da = float(np.max(np.abs(a.astype(np.clongdouble) - rlong[0])))
    de = float(np.max(np.abs(err.astype(np.longdouble) - rlong[1])))
    note("tdse %s: max|a - a_long| / bound = %.3g (restatement's own distance %.3g eps), |err - err_long| / bound = %.3g (err %.3g)"
         % (tag, da / ba, ba / 8.0 / EPS, de / be, float(np.max(err))))
    assert da <= ba, (tag, da, ba)
    assert de <= be, (tag, de, be)
    return da / ba


# ---- 1 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nch,count,nscan,nsteps", [(1, 20, 1, 40), (2, 1, 1, 100), (2, 16, 1, 40), (3, 17, 8, 40), (3, 15, 9, 40),
                                                    (4, 65, 3, 60)])
def test_parity_with_the_restatement(prob, nch, count, nscan, nsteps):
    """No pairs at all, one state per channel, exactly one MFMA tile, one row more, one row less with 9 scans (two column blocks),
    more than one row tile.  (3, 17, 8) runs with the field times exp(0.3 i): the conjugate matters."""
    phase = 0.3 if (nch, count, nscan) == (3, 17, 8) else 0.0
    (E, pairs, D, a0, field), r128, rlong = case(nch, count, nscan, nsteps, phase=phase)
    a, err = prob.tdse_propagate(E, pairs, D, a0, field, DT)
    assert a.shape == (nscan, nch, count) and err.shape == (nscan,)
    check("parity %s" % ((nch, count, nscan, nsteps),), a, err, r128, rlong)
    if nch == 1:
        exact = a0 * np.exp(-1j * E[None] * (nsteps * DT))
        own = float(np.max(np.abs(r128[0] - exact)))
        got = float(np.max(np.abs(a - exact)))
        note("tdse no pairs: |a - a0 exp(-i E t)| = %.3g, the restatement's %.3g" % (got, own))
        assert got <= 10.0 * own
    else:
        assert float(np.max(np.abs(a - a0))) > 1e-3


# ---- 2 ----------------------------------------------------------------------------------------------------------------
def test_pair_lists(prob):
    """The star (0,1), (2,1), (1,3): a reversed pair and a channel with three neighbours.  Then the chain with its first pair
    given twice at half strength, and with its first pair reversed: within the bound of the plain run."""
    (E, pairs, D, a0, field), r128, rlong = case(4, 17, 2, 40, pairs=((0, 1), (2, 1), (1, 3)), phase=0.3)
    a, err = prob.tdse_propagate(E, pairs, D, a0, field, DT)
    check("star", a, err, r128, rlong)
    (E, pairs, D, a0, field), r128, rlong = case(3, 17, 2, 40)
    assert pairs == [(0, 1), (1, 2)]
    D2 = np.concatenate([D * np.array([0.5, 1.0])[:, None, None], 0.5 * D[:1]])
    a, err = prob.tdse_propagate(E, pairs + [(0, 1)], D2, a0, field, DT)
    check("repeated pair", a, err, r128, rlong)
    # real field (phase 0): the first pair in the other orientation with the transposed block is the same Hamiltonian
    a, err = prob.tdse_propagate(E, [(1, 0), (1, 2)], np.stack([D[0].T, D[1]]), a0, field, DT)
    check("reversed pair", a, err, r128, rlong)


# ---- 3 ----------------------------------------------------------------------------------------------------------------
def test_order_and_error_estimate(prob):
    """2 x 2 constant-field problem against the closed form: the error drops by 24 .. 40 from 50 to 100 steps, and err is within a
    factor 2 of the true error."""
    errs = []
    for nsteps in (50, 100):
        E, pairs, D, a0, field, dt, exact = tdse_ref.two_by_two(nsteps)
        a, est = prob.tdse_propagate(E, pairs, D, a0, field, dt)
        true = float(np.max(np.abs(a - exact)))
        note("tdse 2 x 2, %d steps: error %.3g, err %.3g" % (nsteps, true, est[0]))
        assert 0.5 * true <= est[0] <= 2.0 * true
        errs.append(true)
    note("tdse 2 x 2: error ratio %.3g" % (errs[0] / errs[1]))
    assert 24.0 <= errs[0] / errs[1] <= 40.0


# ---- 4 ----------------------------------------------------------------------------------------------------------------
def test_norm(prob):
    (E, pairs, D, a0, field), r128, rlong = case(4, 65, 3, 60)
    a, _ = prob.tdse_propagate(E, pairs, D, a0, field, DT)
    drift = np.abs(np.sum(np.abs(a) ** 2, axis=(1, 2)) - 1.0)
    own = np.abs(np.sum(np.abs(rlong[0]) ** 2, axis=(1, 2)) - np.sum(np.abs(a0.astype(np.clongdouble)) ** 2, axis=(1, 2)))
    bound = 8.0 * float(np.max(own)) + 64.0 * EPS
    note("tdse norm: |sum |a|^2 - 1| = %.3g, bound %.3g (the long-double restatement drifts %.3g)" % (np.max(drift), bound, np.max(own)))
    assert float(np.max(drift)) <= bound


# ---- 5 ----------------------------------------------------------------------------------------------------------------
def same(x, y):
    return np.array_equal(np.ascontiguousarray(x).view(np.uint64), np.ascontiguousarray(y).view(np.uint64))


def test_bit_identities(prob):
    (E, pairs, D, a0, field), _, _ = case(3, 15, 9, 40)
    a, err, snaps = prob.tdse_propagate(E, pairs, D, a0, field, DT, snap_every=20)
    assert snaps.shape == (2, 9, 3, 15)
    # run to run
    a2, err2, snaps2 = prob.tdse_propagate(E, pairs, D, a0, field, DT, snap_every=20)
    assert same(a, a2) and same(err, err2) and same(snaps, snaps2)
    # a scan does not depend on its company (nine scans: two column blocks; alone: one)
    for q in (0, 4, 8):
        aq, eq = prob.tdse_propagate(E, pairs, D, a0[q:q + 1], field[:, :, q:q + 1], DT)
        assert same(aq[0], a[q]) and eq[0] == err[q], q
    # the snapshot after m of 2m steps is the m-step run; continuing from it gives the 2m result; the last snapshot is the result
    am, _ = prob.tdse_propagate(E, pairs, D, a0, field[:20], DT)
    assert same(am, snaps[0]) and same(a, snaps[1])
    ac, _ = prob.tdse_propagate(E, pairs, D, snaps[0], field[20:], DT)
    assert same(ac, a)
    # nsteps = 0 returns a as given
    a0_, e0_ = prob.tdse_propagate(E, pairs, D, a0, field[:0], DT)
    assert same(a0_, a0) and np.all(e0_ == 0.0)
    note("tdse bit identities: run to run, scan alone, snapshot / continuation hold (max err %.3g)" % float(np.max(err)))


def test_stage_bound_and_device_variant(prob):
    """A snapshot per step of 9 scans x 4 x 65 states is 73 KiB: tdse_stage_mb = 1 cuts the 60 steps into groups; the same bits.  The
    _dev variant on torch tensors equals the host variant."""
    (E, pairs, D, a0, field), _, _ = case(4, 65, 9, 60)
    a, err, snaps = prob.tdse_propagate(E, pairs, D, a0, field, DT, snap_every=1)
    assert snaps.shape == (60, 9, 4, 65) and same(snaps[-1], a)
    capi.set_option("tdse_stage_mb", 1)
    try:
        a1, err1, snaps1 = prob.tdse_propagate(E, pairs, D, a0, field, DT, snap_every=1)
        a3, err3, snaps3 = prob.tdse_propagate(E, pairs, D, a0, field, DT, snap_every=7)
    finally:
        capi.set_option("tdse_stage_mb", 0)
    assert same(a1, a) and same(err1, err) and same(snaps1, snaps)
    assert same(a3, a) and same(snaps3, snaps[6::7])
    dev = "cuda:0"
    Ed, Dd = torch.from_numpy(E).to(dev), torch.from_numpy(np.ascontiguousarray(D)).to(dev)
    fd, ad = torch.from_numpy(field).to(dev), torch.from_numpy(np.ascontiguousarray(a0)).to(dev)
    sd = torch.full((60 // 7, 9, 4, 65), float("nan"), dtype=torch.complex128, device=dev)
    torch.cuda.synchronize()
    errd = prob.tdse_propagate_dev(4, 65, Ed.data_ptr(), pairs, Dd.data_ptr(), 9, 60, DT, fd.data_ptr(), ad.data_ptr(), 7, sd.data_ptr())
    assert same(ad.cpu().numpy(), a) and same(errd, err) and same(sd.cpu().numpy(), snaps[6::7])
    note("tdse staging bound and _dev variant: bit-identical (max err %.3g)" % float(np.max(err)))


# ---- 6 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dip_len_lin", "dip_vel_lin"])
def test_end_to_end(name, tmp_path):
    """Solve l = 0 .. 2 (nfun = 64, k = 7), couple the states 1 .. 24 of (0,0), (1,0), (2,0) through host.tdse_system, start in the
    ground state, 200 steps under a sin^2 pulse (velocity gauge: f = -i A(t)); against the restatement fed the same E and D."""
    kind_pi = 1 if name == "dip_len_lin" else 2
    p = capi.Problem(input_from_case(name, nfun=64, k=7, lmax=2))
    assert p.lmax == 2
    _, info = p.solve(0, 3)
    assert np.all(info == 0)
    E, pairs, D = host.tdse_system(p, [(0, 0), (1, 0), (2, 0)], 1, 24, kind_pi=kind_pi)
    assert E.shape == (3, 24) and D.shape == (2, 24, 24) and pairs == [(1, 0), (2, 1)]
    nsteps, T = 200, 200 * DT
    pulse = lambda t: 0.05 * np.sin(np.pi * t / T) ** 2 * np.cos(0.5 * t)
    field = host.field_table([pulse if kind_pi == 1 else (lambda t: -1j * pulse(t))], 0.0, DT, nsteps)
    a0 = np.zeros((1, 3, 24), dtype=np.complex128)
    a0[0, 0, 0] = 1.0
    a, err = p.tdse_propagate(E, pairs, D, a0, field, DT)
    r128, rlong = tdse_ref.both(E, pairs, D, a0, field, DT)
    check("end to end %s" % name, a, err, r128, rlong)
    excited = 1.0 - abs(a[0, 0, 0]) ** 2
    note("tdse end to end %s: population outside the ground state %.3g, norm drift %.3g" % (name, excited, abs(np.sum(np.abs(a) ** 2) - 1)))
    assert 1e-6 < excited < 1.0
    path = str(tmp_path / "TDSE_COEFFs.dat")
    host.write_tdse_coeffs(path, a[0])
    assert same(host.read_tdse_coeffs(path, 72), a[0].reshape(-1))
    p.close()


# ---- 7 ----------------------------------------------------------------------------------------------------------------
def test_argument_checks(prob):
    (E, pairs, D, a0, field), _, _ = case(3, 15, 9, 40)
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
    torch.cuda.synchronize()
    p_ = lambda x: x.ctypes.data_as(C.c_void_p)
    d_ = lambda x: C.c_void_p(x.data_ptr())
    a, snap, err = a0.copy(), np.zeros((4, nscan, nch, count), dtype=np.complex128), np.zeros(nscan)
    for fn, (Ep, Dp, fp, ap, sp) in ((L.bspatom_tdse_propagate, (p_(E), p_(D), p_(field), p_(a), p_(snap))),
                                     (L.bspatom_tdse_propagate_dev, (d_(Ed), d_(Dd), d_(fd), d_(ad), d_(sd)))):
        good = [prob._h, nch, count, Ep, 2, p_(ci), p_(cf), Dp, nscan, nsteps, DT, fp, ap, 1, sp, p_(err)]
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
        # allowed: no snapshots, no error estimate, no pairs, no steps (then no field either)
        assert fn(*[None if i in (14, 15) else x for i, x in enumerate(sub(13, 0))]) == 0
        assert fn(*[None if i in (5, 6, 7) else x for i, x in enumerate(sub(4, 0))]) == 0
        assert fn(*[None if i == 11 else x for i, x in enumerate(sub(9, 0))]) == 0
        assert fn(*good) == 0                                      # a valid call afterwards
    assert np.all(np.isfinite(a)) and np.all(np.isfinite(ad.cpu().numpy().view(np.float64)))
