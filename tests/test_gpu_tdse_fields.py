"""bspatom_tdse_fields / _dev (csrc/tdse_fields.hip: the stage with a pair of accumulators per field, its observing stage 0, the reduction
to rows of 4 + 2 nfield) on the GPU against the NumPy restatement tests/tdse_fields_ref.py.

The yardstick is that of tests/test_gpu_tdse_static.py: the restatement run twice, in complex128 and in long double, and
    max|a_gpu - a_long| <= 8 max(max|a_128 - a_long|, eps),
err[q] likewise with the floor eps dt (tdse_ref.amp_bound / err_bound).  The rows are checked bit for bit against bspatom_tdse_observe
and bspatom_tdse_static calls without steps on the run's own snapshots (guarantee 2 of the header).  Never against the code under test.
Every test notes its ratio."""
import functools
import math
import numpy as np
import pytest
import torch                               # first: its HIP runtime is the one the process uses
from test_gpu_stages import input_from_case, note

import tdse_fields_ref
import tdse_obs_ref
import tdse_ref
from bspatom_amd import capi, host

pytestmark = pytest.mark.gpu
EPS = tdse_ref.EPS
DT = 0.05
# (nch, count, nscan, nsteps, nfield)
SHAPES = [(2, 1, 1, 40, 2), (3, 17, 8, 40, 2), (3, 15, 9, 40, 2), (4, 65, 3, 40, 3)]
TILT = (math.sin(0.4) * math.cos(1.1), math.sin(0.4) * math.sin(1.1), math.cos(0.4))


@pytest.fixture(scope="module")
def prob():
    p = capi.Problem(input_from_case("tiny8"))           # the handle gives the device and the stream only
    yield p
    p.close()


@functools.lru_cache(maxsize=None)
def system(nch, count, nscan, nsteps, nfield):
    """(E, pairs, D, fidx, a0, field, static) computed once and shared; nobody writes into it.  (3, 17, 8) runs with every field times
    exp(0.3 i)."""
    phase = 0.3 if (nch, count, nscan) == (3, 17, 8) else 0.0
    return tdse_fields_ref.system(nch, count, nscan, nsteps, nfield, dt=DT, phase=phase)


@functools.lru_cache(maxsize=None)
def case(nch, count, nscan, nsteps, nfield, scheme):
    """(system, complex128 restatement, long-double restatement)"""
    s = system(nch, count, nscan, nsteps, nfield)
    r128, rlong = tdse_fields_ref.both(*s[:6], DT, static=s[6], scheme=scheme)
    return s, r128, rlong


def check(tag, a, err, r128, rlong, dt=DT):
    ba, be = tdse_ref.amp_bound(r128[0], rlong[0]), tdse_ref.err_bound(r128[1], rlong[1], dt)
    da = float(np.max(np.abs(a.astype(np.clongdouble) - rlong[0])))
    de = float(np.max(np.abs(err.astype(np.longdouble) - rlong[1])))
    note("tdse fields %s: max|a - a_long| / bound = %.3g (restatement's own distance %.3g eps), |err - err_long| / bound = %.3g (err %.3g)"
         % (tag, da / ba, ba / 8.0 / EPS, de / be, float(np.max(err))))
    assert da <= ba, (tag, da, ba)
    assert de <= be, (tag, de, be)
    return ba, be


def same(x, y):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    return x.shape == y.shape and np.array_equal(x.view(np.uint64), y.view(np.uint64))


# ---- 1 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", [0, 1])
@pytest.mark.parametrize("key", SHAPES)
def test_parity_with_the_restatement(prob, key, scheme):
    """One state per channel with two pairs on the same channel pair and different fields; one row past an MFMA tile with complex
    tables; two column blocks; two row tiles with three fields."""
    (E, pairs, D, fidx, a0, field, static), r128, rlong = case(*key, scheme)
    assert sorted(set(fidx)) == list(range(key[4])) and pairs[-1] == pairs[0] and fidx[-1] != fidx[0]
    a, err = prob.tdse_fields(E, pairs, D, fidx, a0, field, DT, static, scheme=scheme)
    assert a.shape == a0.shape and err.shape == (key[2],)
    check("parity %s scheme %d" % (key, scheme), a, err, r128, rlong)
    # the other fields are felt: every pair on field 0 is another run
    one = prob.tdse_static(E, pairs, D, a0, np.ascontiguousarray(field[:, :, 0, :]), DT, static, scheme=scheme)[0]
    felt = float(np.max(np.abs(a - one)))
    note("tdse fields parity %s scheme %d: distance from the run with every pair on field 0 %.3g" % (key, scheme, felt))
    assert felt > 1e-3


# ---- 2 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", [0, 1])
@pytest.mark.parametrize("key", [(3, 15, 9, 40, 2), (4, 65, 3, 40, 3)])
def test_rows(prob, key, scheme):
    """obs_every = 1 with snap_every = 1: the rows describe [a0, snaps[0], .., snaps[-1]] of the same run.  Guarantee 2: every entry has
    the bits of a call of the older entry points without steps on the same amplitudes, every state of every scan as one scan."""
    nch, count, nscan, nsteps, nfield = key
    E, pairs, D, fidx, a0, field, static = system(*key)
    RW = 4 + 2 * nfield
    a, err, obs, snaps = prob.tdse_fields(E, pairs, D, fidx, a0, field, DT, static, scheme=scheme, obs_every=1, snap_every=1)
    assert obs.shape == (nsteps + 1, nscan, nch, RW) and same(a, snaps[-1])
    states = np.concatenate([a0[None], snaps])
    packets = states.reshape(-1, nch, count)
    nof = np.zeros((0, 6, len(packets)), dtype=np.complex128)
    shape4 = (nsteps + 1, nscan, nch)
    for g in range(nfield):
        pg, Dg = tdse_fields_ref.sublist(pairs, D, fidx, g)
        assert len(pg) >= 1
        o4 = prob.tdse_observe(E, pg, Dg, packets, nof, DT, obs_every=1)[2][0].reshape(shape4 + (4,))
        k = 2 if g == 0 else 4 + 2 * g
        assert same(o4[..., 2:], obs[..., k:k + 2]), g
        assert same(o4[..., :2], obs[..., :2]), g
        assert float(np.max(np.abs(obs[..., k:k + 2]))) > 0.0
    p0, D0 = tdse_fields_ref.sublist(pairs, D, fidx, 0)
    o6 = prob.tdse_static(E, p0, D0, packets, nof, DT, static, scheme=scheme, obs_every=1)[2][0].reshape(shape4 + (6,))
    assert same(o6, obs[..., :6])
    assert float(np.min(obs[..., 5])) < 0.0
    # and against the long-double definition on the snapshots, with the bound of tests/test_gpu_tdse_observe.py per field:
    # |z - z_long| <= (count (pairs of the field + 1) + 16) eps M_k, M_k the largest sum of the moduli of a row's terms
    worst = 0.0
    for g in range(nfield):
        pg, Dg = tdse_fields_ref.sublist(pairs, D, fidx, g)
        ref = tdse_obs_ref.observables(E, pg, Dg, states, np.longdouble, np.clongdouble)[..., 2:]
        M = tdse_obs_ref.magnitudes(E, pg, Dg, states)[2:]
        k = 2 if g == 0 else 4 + 2 * g
        diff = np.abs(obs[..., k:k + 2].astype(np.longdouble) - ref).reshape(-1, 2).max(axis=0)
        bound = (count * (len(pg) + 1) + 16) * np.longdouble(EPS) * M
        worst = max(worst, float(np.max(diff / bound)))
        assert np.all(diff <= bound), (g, diff, bound)
    note("tdse fields rows %s scheme %d: the bits of the calls without steps hold; |z_g - z_g,long| / bound <= %.3g" % (key, scheme, worst))
    # and a call of its own without steps gives the whole row
    a_, e_, o1 = prob.tdse_fields(E, pairs, D, fidx, snaps[7], field[:0], DT, static, scheme=scheme, obs_every=1)
    assert o1.shape == (1, nscan, nch, RW) and same(o1[0], obs[8]) and same(a_, snaps[7]) and np.all(e_ == 0.0)


# ---- 3 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", [0, 1])
def test_bit_identities(prob, scheme):
    key = (3, 15, 9, 40, 2)
    nch, count, nscan, nsteps, nfield = key
    E, pairs, D, fidx, a0, field, static = system(*key)
    f0 = np.ascontiguousarray(field[:, :, :1, :])
    # one field: the bits of bspatom_tdse_static, with and without static blocks, fidx absent or zeros
    for st in (static, None):
        wa, werr, wobs, wsnaps = prob.tdse_static(E, pairs, D, a0, f0[:, :, 0, :], DT, st, scheme=scheme, obs_every=7, snap_every=20)
        for fx in (None, [0] * len(pairs)):
            a, err, obs, snaps = prob.tdse_fields(E, pairs, D, fx, a0, f0, DT, st, scheme=scheme, obs_every=7, snap_every=20)
            assert obs.shape[-1] == 6
            assert same(a, wa) and same(err, werr) and same(snaps, wsnaps) and same(obs, wobs)
    # two fields: run to run
    a, err, obs, snaps = prob.tdse_fields(E, pairs, D, fidx, a0, field, DT, static, scheme=scheme, obs_every=1, snap_every=20)
    a2, err2, obs2, snaps2 = prob.tdse_fields(E, pairs, D, fidx, a0, field, DT, static, scheme=scheme, obs_every=1, snap_every=20)
    assert same(a, a2) and same(err, err2) and same(obs, obs2) and same(snaps, snaps2)
    assert float(np.max(err)) > 0.0 and not same(a, wa)
    # scan 4 of nine (two column blocks) and the same scan alone (one)
    aq, eq, oq = prob.tdse_fields(E, pairs, D, fidx, a0[4:5], field[:, :, :, 4:5], DT, static, scheme=scheme, obs_every=1)
    assert same(aq[0], a[4]) and eq[0] == err[4] and same(oq[:, 0], obs[:, 4])
    # the snapshot after 20 of 40 steps is the 20-step run, the last one the result
    am, _ = prob.tdse_fields(E, pairs, D, fidx, a0, field[:20], DT, static, scheme=scheme)
    assert same(am, snaps[0]) and same(a, snaps[1])
    # obs_every = 7: the rows obs_steps(40, 7) of the full run; nothing else changes; nor without rows
    a7, err7, obs7 = prob.tdse_fields(E, pairs, D, fidx, a0, field, DT, static, scheme=scheme, obs_every=7)
    assert same(obs7, obs[host.obs_steps(nsteps, 7)]) and same(a7, a) and same(err7, err)
    a0_, err0_ = prob.tdse_fields(E, pairs, D, fidx, a0, field, DT, static, scheme=scheme)
    assert same(a0_, a) and same(err0_, err)
    # without static blocks the same kernels run on the driven entries alone: s = 0 exactly, and run to run
    an, en, on = prob.tdse_fields(E, pairs, D, fidx, a0, field, DT, None, scheme=scheme, obs_every=7)
    assert np.all(on[..., 4:6].view(np.uint64) == 0) and same(an, prob.tdse_fields(E, pairs, D, fidx, a0, field, DT, None, scheme=scheme)[0])
    # the staging bound of the host variant: a field table of 40 x 6 x 2 x 9 complex is 69 KiB, a snapshot per step 13 KiB
    capi.set_option("tdse_stage_mb", 1)
    try:
        a1, err1, obs1, snaps1 = prob.tdse_fields(E, pairs, D, fidx, a0, field, DT, static, scheme=scheme, obs_every=1, snap_every=20)
    finally:
        capi.set_option("tdse_stage_mb", 0)
    assert same(a1, a) and same(err1, err) and same(obs1, obs) and same(snaps1, snaps)
    note("tdse fields bit identities scheme %d: one field = tdse_static, run to run, scan alone, snapshot, obs_every, staging bound hold "
         "(max err %.3g)" % (scheme, float(np.max(err))))


@pytest.mark.parametrize("scheme", [0, 1])
def test_staging_bound_cuts_the_run(prob, scheme):
    """A snapshot per step of 3 scans x 4 x 65 states is 12 KiB and a step of the table 0.9 KiB: tdse_stage_mb = 1 cuts 120 steps into
    groups (three fields: the stride of the table per step is 12 nfield nscan doubles); the same bits."""
    E, pairs, D, fidx, a0, field, static = tdse_fields_ref.system(4, 65, 3, 120, 3, dt=DT)
    a, err, obs, snaps = prob.tdse_fields(E, pairs, D, fidx, a0, field, DT, static, scheme=scheme, obs_every=1, snap_every=1)
    capi.set_option("tdse_stage_mb", 1)
    try:
        a1, err1, obs1, snaps1 = prob.tdse_fields(E, pairs, D, fidx, a0, field, DT, static, scheme=scheme, obs_every=1, snap_every=1)
        a3, err3, obs3, snaps3 = prob.tdse_fields(E, pairs, D, fidx, a0, field, DT, static, scheme=scheme, obs_every=7, snap_every=3)
    finally:
        capi.set_option("tdse_stage_mb", 0)
    assert (120 * (12 * 3 * 3 + 2 * 3 * 4 * 65 + 10 * 3 * 4)) * 8 > 1 << 20                      # more than one group
    assert same(a1, a) and same(err1, err) and same(obs1, obs) and same(snaps1, snaps)
    assert same(a3, a) and same(err3, err) and same(obs3, obs[host.obs_steps(120, 7)]) and same(snaps3, snaps[2::3])


# ---- 4 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", [0, 1])
def test_dev_variant(prob, scheme):
    key = (3, 17, 8, 40, 2)
    nch, count, nscan, nsteps, nfield = key
    E, pairs, D, fidx, a0, field, static = system(*key)
    a, err, obs, snaps = prob.tdse_fields(E, pairs, D, fidx, a0, field, DT, static, scheme=scheme, obs_every=7, snap_every=20)
    steps7 = host.obs_steps(nsteps, 7)
    dev = "cuda:0"
    Ed, Dd = torch.from_numpy(E).to(dev), torch.from_numpy(np.ascontiguousarray(D)).to(dev)
    Wd = torch.from_numpy(static[2]).to(dev)
    fd, ad = torch.from_numpy(field).to(dev), torch.from_numpy(np.ascontiguousarray(a0)).to(dev)
    sd = torch.full((2, nscan, nch, count), float("nan"), dtype=torch.complex128, device=dev)
    od = torch.full((len(steps7), nscan, nch, 8), float("nan"), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    errd = prob.tdse_fields_dev(nch, count, Ed.data_ptr(), pairs, Dd.data_ptr(), fidx, nfield, nscan, nsteps, DT, fd.data_ptr(), ad.data_ptr(),
                                (static[0], static[1], Wd.data_ptr()), scheme, 7, od.data_ptr(), 20, sd.data_ptr())
    assert same(ad.cpu().numpy(), a) and same(errd, err) and same(od.cpu().numpy(), obs) and same(sd.cpu().numpy(), snaps)
    L = capi.lib()
    assert L.bspatom_tdse_fields_dev(prob._h, nch, count, Ed.data_ptr(), 0, None, None, None, nscan, 0, DT, None, ad.data_ptr(), 0, None, None,
                                     0, None, 1, 0, None, None, None, None, 4, None) == -5
    note("tdse fields _dev scheme %d: a, err, obs, snaps have the bits of the host variant" % scheme)


# ---- 5 ----------------------------------------------------------------------------------------------------------------
def shell_populations(a, channels):
    p = a.real * a.real + a.imag * a.imag
    return np.stack([sum(p[..., c, :] for c, (l, _) in enumerate(channels) if l == ll) for ll in range(3)], axis=-2)


def test_end_to_end():
    """dip_len_lin with nfun = 64, k = 7, l = 0 .. 2: the nine channels (l, m), states 1 .. 24, through host.tdse_system_pol; from the
    ground state 200 Lawson steps under 0.05 sin^2(pi t / T) cos(0.5 t) along z (scan 0) and along a tilted axis (scan 1).  The one test
    that rests on a physics identity: a rotation of the field rotates the packet, so the populations summed over m agree."""
    p = capi.Problem(input_from_case("dip_len_lin", nfun=64, k=7, lmax=2))
    assert p.lmax == 2
    _, info = p.solve(0, 3)
    assert np.all(info == 0)
    channels = [(l, m) for l in range(3) for m in range(-l, l + 1)]
    E, pairs, D, fidx = host.tdse_system_pol(p, channels, 1, 24)
    assert E.shape == (9, 24) and D.shape == (12, 24, 24) and fidx.count(0) == 4 and fidx.count(1) == 8
    nsteps, T = 200, 200 * DT
    env = lambda t: 0.05 * np.sin(np.pi * t / T) ** 2 * np.cos(0.5 * t)
    field = host.field_table_pol([lambda t: (0.0 * t, 0.0 * t, env(t)), lambda t: tuple(n * env(t) for n in TILT)], 0.0, DT, nsteps)
    a0 = np.zeros((2, 9, 24), dtype=np.complex128)
    a0[:, 0, 0] = 1.0
    a, err, obs = p.tdse_fields(E, pairs, D, fidx, a0, field, DT, None, scheme=1, obs_every=10)
    p.close()
    assert obs.shape == (21, 2, 9, 8)
    r128, rlong = tdse_fields_ref.both(E, pairs, D, fidx, a0, field, DT, scheme=1, obs_every=10)
    bounds = []
    for q in (0, 1):
        bounds.append(check("end to end scan %d" % q, a[q:q + 1], err[q:q + 1], [r[q:q + 1] for r in r128[:2]], [r[q:q + 1] for r in rlong[:2]])[0])
    # the long-double restatement: the identities to the bound of tests/test_tdse_fields_cpu.py (64 eps of double)
    spl = shell_populations(rlong[0], channels)
    dpl = float(np.max(np.abs(spl[0] - spl[1])))
    v = host.tdse_dipole_vector(rlong[2])
    dz = v[:, 0, 2]
    big = float(np.max(np.abs(dz)))
    dv = float(np.max(np.abs(v[:, 1, :] - dz[:, None] * np.array(TILT, dtype=v.dtype)[None, :])))
    assert dpl <= 64 * EPS and big > 1e-4 and dv <= 64 * EPS * big
    # the GPU: the shell populations of the two scans within the sum of the two scans' yardstick bounds
    sp = shell_populations(a, channels)
    dp = float(np.max(np.abs(sp[0] - sp[1])))
    pb = bounds[0] + bounds[1]
    moved = [c for c, (l, m) in enumerate(channels) if m != 0]
    pop_m = float(np.sum(np.abs(a[1][moved]) ** 2))
    gv = host.tdse_dipole_vector(obs)
    gdv = float(np.max(np.abs(gv[:, 1, :] - gv[:, 0, 2][:, None] * np.array(TILT)[None, :])))
    note("tdse fields end to end: shell populations of the two scans differ by %.3g (bound %.3g; long double %.3g); dipole vector "
         "identity off by %.3g on the GPU rows, %.3g in long double (largest dipole %.3g); population in m != 0 of the tilted scan %.3g; "
         "excited %.3g" % (dp, pb, dpl, gdv, dv, big, pop_m, 1.0 - float(np.abs(a[0, 0, 0]) ** 2)))
    assert dp <= bounds[0] + bounds[1]
    assert pop_m > 1e-6 and np.all(a[0][moved] == 0.0)
