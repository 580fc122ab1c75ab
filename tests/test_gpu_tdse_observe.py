"""bspatom_tdse_observe / _dev (csrc/tdse.hip: tdse_observe_kernel, tdse_obs_reduce_kernel) on the GPU.

Two chains of trust.  The amplitudes: a, err and the snapshots are bit-equal to bspatom_tdse_propagate's (test 1), and those are
checked against the restatement by tests/test_gpu_tdse.py.  The observables: the rows of an obs_every = 1 run describe the states
[a0, snaps[0], .., snaps[-1]] of that same run; tests/tdse_obs_ref.py evaluates the definitions on them in long double, and per
component
    |obs_gpu - obs_long| <= (count (npairs + 1) + 16) eps M_k,
M_k the largest sum of the moduli of a row's terms: the worst-case rounding bound of ANY summation order with at most that many
chained additions (the MFMA chain along K over a channel's entries, count npairs at most, then the epilogue's tree: four rows, two
shuffles, the Re/Im pair, four waves, the row tiles).  An indexing, conjugation or tiling mistake misses it by ten orders of
magnitude.  Never against the code under test.  Every test notes its measured ratio."""
import ctypes as C
import functools
import numpy as np
import pytest
import torch                               # first: its HIP runtime is the one the process uses
from test_gpu_stages import input_from_case, note

import tdse_obs_ref
import tdse_ref
from bspatom_amd import capi, host

pytestmark = pytest.mark.gpu
EPS = tdse_ref.EPS
DT = 0.05
STAR = ((0, 1), (2, 1), (1, 3))
SHAPES = [(1, 20, 1, 40), (2, 1, 1, 100), (2, 16, 1, 40), (3, 17, 8, 40), (3, 15, 9, 40), (4, 65, 3, 60), (2, 129, 2, 10)]


@pytest.fixture(scope="module")
def prob():
    p = capi.Problem(input_from_case("tiny8"))           # the handle gives the device and the stream only
    yield p
    p.close()


@functools.lru_cache(maxsize=None)
def system(nch, count, nscan, nsteps, pairs=None):
    """tdse_ref.system, computed once and shared; nobody writes into it.  (3, 17, 8) and the star run with the field times exp(0.3 i)."""
    phase = 0.3 if (nch, count, nscan) == (3, 17, 8) or pairs is not None else 0.0
    return tdse_ref.system(nch, count, nscan, nsteps, pairs=None if pairs is None else list(pairs), dt=DT, phase=phase)


_RUNS = {}


def observed(prob, key):
    """(a, err, obs, snaps) of tdse_observe(obs_every = 1, snap_every = 1) on system(*key): one run per shape, shared by the tests"""
    if key not in _RUNS:
        E, pairs, D, a0, field = system(*key)
        _RUNS[key] = prob.tdse_observe(E, pairs, D, a0, field, DT, obs_every=1, snap_every=1)
    return _RUNS[key]


def same(x, y):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    return x.shape == y.shape and np.array_equal(x.view(np.uint64), y.view(np.uint64))


# ---- 1 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nch,count,nscan,nsteps", SHAPES)
def test_bits_against_propagate(prob, nch, count, nscan, nsteps):
    """The shapes of test_gpu_tdse.py's parity test and (2, 129, 2): three row tiles, the sum across workgroups."""
    E, pairs, D, a0, field = system(nch, count, nscan, nsteps)
    a, err, obs, snaps = observed(prob, (nch, count, nscan, nsteps))
    ap, errp, snapsp = prob.tdse_propagate(E, pairs, D, a0, field, DT, snap_every=1)
    assert obs.shape == (nsteps + 1, nscan, nch, 4) and snaps.shape == (nsteps, nscan, nch, count)
    assert same(a, ap) and same(err, errp) and same(snaps, snapsp)
    assert float(np.max(err)) > 0.0 and np.all(np.isfinite(obs))


# ---- 2 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", SHAPES + [(4, 17, 2, 40, STAR)])
def test_observables_against_long_double(prob, key):
    nch, count, nscan, nsteps = key[:4]
    E, pairs, D, a0, field = system(*key)
    a, err, obs, snaps = observed(prob, key)
    states = np.concatenate([a0[None], snaps])
    ref = tdse_obs_ref.observables(E, pairs, D, states, np.longdouble, np.clongdouble)
    M = tdse_obs_ref.magnitudes(E, pairs, D, states)
    assert ref.shape == obs.shape
    diff = np.abs(obs.astype(np.longdouble) - ref).reshape(-1, 4).max(axis=0)
    bound = (count * (len(pairs) + 1) + 16) * np.longdouble(EPS) * M
    ratio = [float(diff[k] / bound[k]) if bound[k] > 0 else 0.0 for k in range(4)]
    note("tdse observe %s: |obs - obs_long| / bound per component = %s (M = %s)"
         % (key, " ".join("%.3g" % r for r in ratio), " ".join("%.3g" % float(m) for m in M)))
    for k in range(4):
        assert diff[k] <= bound[k], (key, k, float(diff[k]), float(bound[k]))
    if len(pairs) == 0:
        assert np.all(obs[..., 2:] == 0.0)
    else:
        assert float(np.max(np.abs(obs[..., 2]))) > 0.0 and float(np.max(np.abs(obs[..., 3]))) > 0.0
        # the channels no pair ends in have z = 0 exactly
        for c in set(range(nch)) - {f for _, f in pairs}:
            assert np.all(obs[:, :, c, 2:] == 0.0)
    norm, h0, dre, dim = host.tdse_expectations(obs)
    assert norm.shape == (nsteps + 1, nscan) and same(norm[0], obs[0, :, :, 0].sum(axis=-1))


# ---- 3 ----------------------------------------------------------------------------------------------------------------
def test_exact_rows_end_to_end():
    """Solve l = 0 .. 2 (nfun = 64, k = 7), the states 1 .. 24 of three channels in the length gauge, start in the ground state: row 0 is
    exact; after 200 steps under the pulse of test_gpu_tdse.py's end-to-end test the populations sum to 1 and the dipole is there."""
    p = capi.Problem(input_from_case("dip_len_lin", nfun=64, k=7, lmax=2))
    _, info = p.solve(0, 3)
    assert np.all(info == 0)
    E, pairs, D = host.tdse_system(p, [(0, 0), (1, 0), (2, 0)], 1, 24, kind_pi=1)
    nsteps, T = 200, 200 * DT
    pulse = lambda t: 0.05 * np.sin(np.pi * t / T) ** 2 * np.cos(0.5 * t)
    field = host.field_table([pulse], 0.0, DT, nsteps)
    a0 = np.zeros((1, 3, 24), dtype=np.complex128)
    a0[0, 0, 0] = 1.0
    a, err, obs = p.tdse_observe(E, pairs, D, a0, field, DT, obs_every=100)
    ap, errp = p.tdse_propagate(E, pairs, D, a0, field, DT)
    p.close()
    assert obs.shape == (3, 1, 3, 4) and host.obs_steps(nsteps, 100) == [0, 100, 200]
    assert same(a, ap) and same(err, errp)
    assert same(obs[0, 0, :, 0], np.array([1.0, 0.0, 0.0]))
    assert same(obs[0, 0, :, 1], np.array([E[0, 0], 0.0, 0.0]))
    assert np.all(obs[0, 0, :, 2:] == 0.0)
    along, _ = tdse_ref.propagate(E, pairs, D, a0, field, DT, np.longdouble, np.clongdouble)
    own = float(abs(np.sum(np.abs(along) ** 2) - 1))
    bound = 8.0 * own + 64.0 * EPS
    norm, h0, dre, dim = host.tdse_expectations(obs)
    note("tdse observe end to end: |sum pop - 1| = %.3g, bound %.3g (the long-double restatement drifts %.3g); 2 Re z = %.3g at "
         "n = 100, %.3g at n = 200; <H0> %.6g -> %.6g" % (abs(norm[-1, 0] - 1.0), bound, own, dre[1, 0], dre[2, 0], h0[0, 0], h0[-1, 0]))
    assert abs(norm[-1, 0] - 1.0) <= bound
    assert dre[-1, 0] != 0.0 and dre[1, 0] != 0.0


# ---- 4 ----------------------------------------------------------------------------------------------------------------
def test_closed_form_and_sign_convention(prob):
    """The 2 x 2 problem with the constant complex field f = 1 + 0.5i: z of the last row against the exact state, and
    W = <H0> + 2 Re(f z) = <H> is conserved by the exact flow (H Hermitian); a conjugation error in z breaks both because f is complex."""
    E, pairs, D, a0, field, dt, exact = tdse_ref.two_by_two(50)
    f = complex(field[0, 0, 0])
    a, err, obs = prob.tdse_observe(E, pairs, D, a0, field, dt, obs_every=1)
    assert obs.shape == (51, 1, 2, 4)
    d = float(np.max(np.abs(a - exact)))
    z = obs[:, 0, :, 2].sum(axis=-1) + 1j * obs[:, 0, :, 3].sum(axis=-1)
    zx = 0.4 * np.conj(exact[0, 1, 0]) * exact[0, 0, 0]
    bz = 0.8 * d * (1.0 + d) + 16.0 * EPS
    W = obs[:, 0, :, 1].sum(axis=-1) + 2.0 * np.real(f * z)
    H = np.array([[E[0, 0], np.conj(f) * 0.4], [f * 0.4, E[1, 0]]])
    bw = float(np.linalg.norm(H, 2)) * (2.0 * np.sqrt(2.0) * d + 2.0 * d * d) + 64.0 * EPS
    note("tdse observe 2 x 2: d = %.3g, |z - z_exact| / bound = %.3g, |W_last - W_0| / bound = %.3g (W_0 = %.6g, z_last = %.6g%+.6gi)"
         % (d, abs(z[-1] - zx) / bz, abs(W[-1] - W[0]) / bw, W[0], z[-1].real, z[-1].imag))
    assert abs(z[-1] - zx) <= bz
    assert abs(W[-1] - W[0]) <= bw
    assert abs(zx.imag) > 1e-2 and abs(z[0] - 0.4 * np.conj(a0[0, 1, 0]) * a0[0, 0, 0]) <= 16.0 * EPS


# ---- 5 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nch,count,nscan,nsteps", [(3, 15, 9, 40), (4, 65, 9, 60)])
def test_bit_identities(prob, nch, count, nscan, nsteps):
    E, pairs, D, a0, field = system(nch, count, nscan, nsteps)
    a, err, obs, snaps = observed(prob, (nch, count, nscan, nsteps))
    # run to run
    a2, err2, obs2, snaps2 = prob.tdse_observe(E, pairs, D, a0, field, DT, obs_every=1, snap_every=1)
    assert same(a, a2) and same(err, err2) and same(obs, obs2) and same(snaps, snaps2)
    # a scan does not depend on its company (nine scans: two column blocks; alone: one)
    for q in (0, 4, 8):
        aq, eq, oq = prob.tdse_observe(E, pairs, D, a0[q:q + 1], field[:, :, q:q + 1], DT, obs_every=1)
        assert same(aq[0], a[q]) and eq[0] == err[q] and same(oq[:, 0], obs[:, q]), q
    # obs_every = 7: the rows obs_steps(nsteps, 7) of the full run; nothing else changes
    a7, err7, obs7 = prob.tdse_observe(E, pairs, D, a0, field, DT, obs_every=7)
    steps7 = host.obs_steps(nsteps, 7)
    assert obs7.shape[0] == len(steps7) and same(obs7, obs[steps7]) and same(a7, a) and same(err7, err)
    # row n: the last row of the run truncated to n steps, and row 0 of a call without steps on snaps[n - 1]
    for n in (1, 13, nsteps - 1):
        an, _, on = prob.tdse_observe(E, pairs, D, a0, field[:n], DT, obs_every=nsteps)
        assert on.shape[0] == 2 and same(on[-1], obs[n]) and same(on[0], obs[0]) and same(an, snaps[n - 1]), n
        a_, e_, o0 = prob.tdse_observe(E, pairs, D, snaps[n - 1], field[:0], DT, obs_every=1)
        assert o0.shape[0] == 1 and same(o0[0], obs[n]) and same(a_, snaps[n - 1]) and np.all(e_ == 0.0), n
    # the staging bound: a snapshot per step cuts the run into groups under 1 MiB (4 x 65 x 9: 73 KiB per step)
    capi.set_option("tdse_stage_mb", 1)
    try:
        a1, err1, obs1, snaps1 = prob.tdse_observe(E, pairs, D, a0, field, DT, obs_every=1, snap_every=1)
        a3, err3, obs3, snaps3 = prob.tdse_observe(E, pairs, D, a0, field, DT, obs_every=7, snap_every=3)
    finally:
        capi.set_option("tdse_stage_mb", 0)
    assert same(a1, a) and same(err1, err) and same(obs1, obs) and same(snaps1, snaps)
    assert same(a3, a) and same(obs3, obs[steps7]) and same(snaps3, snaps[2::3])
    # the _dev variant on torch tensors
    dev = "cuda:0"
    Ed, Dd = torch.from_numpy(E).to(dev), torch.from_numpy(np.ascontiguousarray(D)).to(dev)
    fd, ad = torch.from_numpy(field).to(dev), torch.from_numpy(np.ascontiguousarray(a0)).to(dev)
    sd = torch.full((nsteps // 3, nscan, nch, count), float("nan"), dtype=torch.complex128, device=dev)
    od = torch.full((len(steps7), nscan, nch, 4), float("nan"), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    errd = prob.tdse_observe_dev(nch, count, Ed.data_ptr(), pairs, Dd.data_ptr(), nscan, nsteps, DT, fd.data_ptr(), ad.data_ptr(), 7,
                                 od.data_ptr(), 3, sd.data_ptr())
    assert same(ad.cpu().numpy(), a) and same(errd, err) and same(od.cpu().numpy(), obs[steps7]) and same(sd.cpu().numpy(), snaps[2::3])
    # the expectation values of any blocks over any packets: every snapshot of every scan as one scan of a call without steps
    packets = snaps.reshape(nsteps * nscan, nch, count)
    ap_, ep_, op_ = prob.tdse_observe(E, pairs, D, packets, np.zeros((0, 6, nsteps * nscan), dtype=np.complex128), DT, obs_every=1)
    assert op_.shape == (1, nsteps * nscan, nch, 4) and same(op_[0].reshape(nsteps, nscan, nch, 4), obs[1:]) and same(ap_, packets)
    pd, opd = torch.from_numpy(packets).to(dev), torch.full((1, nsteps * nscan, nch, 4), float("nan"), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    prob.tdse_observe_dev(nch, count, Ed.data_ptr(), pairs, Dd.data_ptr(), nsteps * nscan, 0, DT, None, pd.data_ptr(), 1, opd.data_ptr())
    assert same(opd.cpu().numpy(), op_) and same(pd.cpu().numpy(), packets)
    note("tdse observe bit identities %s: run to run, scan alone, obs_every, truncated run, no-step call, staging bound, _dev, %d packets"
         % ((nch, count, nscan, nsteps), nsteps * nscan))


# ---- 6 ----------------------------------------------------------------------------------------------------------------
def test_argument_checks(prob):
    (E, pairs, D, a0, field) = system(3, 15, 9, 40)
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
    want_a, want_err = prob.tdse_propagate(E, pairs, D, a0, field, DT)
    for fn, dvc, (Ep, Dp, fp, ap, sp, op) in ((L.bspatom_tdse_observe, False, (p_(E), p_(D), p_(field), p_(a), p_(snap), p_(obs))),
                                              (L.bspatom_tdse_observe_dev, True, (d_(Ed), d_(Dd), d_(fd), d_(ad), d_(sd), d_(od)))):
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
        # obs_every = 0 without obs is bspatom_tdse_propagate: its bits
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
