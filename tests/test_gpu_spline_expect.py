"""Expectation values in the spline basis (bspatom_spline_expect / _dev, csrc/spline_expect.hip) and the same numbers along a split-step
run (bspatom_tdse_split_observe / _dev): the guarantees E1 - E6 bit for bit, every value against a long-double evaluation of the
definition (tests/spline_expect_ref.py) within a derived bound, the header's order of operations in float64 NumPy bit for bit, a
field-free beat and the second order of the dipole rows end to end, a run with 29 channels, and the argument checks.  Fixtures come
from test_gpu_resolvent_coupled._assembled, with test_gpu_tdse_split's shapes and seeding style."""
import ctypes as C
import functools
import numpy as np
import pytest
import torch                               # first: its HIP runtime is the one the process uses
from test_gpu_stages import note

import resolvent_ref as ref
import spline_expect_ref as eref
import tdse_spline_ref as sref
import tdse_split_ref as pref
import test_gpu_resolvent as single
import test_gpu_resolvent_coupled as coupled
from bspatom_amd import capi, host

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
same = single._same
DT = 0.05
NSCAN, SLOTS, GROUP, OBS_EVERY, SNAP_EVERY = 5, 2, 3, 2, 3
NEXP = 5
# (fixture, nch, nsteps): n = 8 below a wave and below the band width; one past a wave multiple; b = 8; b = 15; a single channel
SHAPES = [("tiny8", 2, 7), ("n65_k4", 3, 7), ("lin256", 4, 7), ("k16_n40", 4, 2), ("n65_k4", 1, 3)]
IDS = ["%s-nch%d" % (s[0], s[1]) for s in SHAPES]


class _Options:
    """bspatom_set_option for the duration of a with block"""
    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        for k, v in self.kw.items():
            capi.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.kw:
            capi.set_option(k, 0)


def _angular(nch, rng):
    """(Q, lam) of a random symmetric tridiagonal angular matrix; a single channel: Q = [1], lam = [0.7]"""
    if nch == 1:
        return np.ones((1, 1)), np.array([0.7])
    off = rng.uniform(0.3, 0.7, nch - 1)
    A = np.diag(rng.uniform(-0.2, 0.2, nch)) + np.diag(off, 1) + np.diag(off, -1)
    lam, Q = np.linalg.eigh(A)
    return np.ascontiguousarray(Q), lam


def _tridiagonal(nch, rng):
    off = rng.uniform(0.3, 0.7, max(nch - 1, 0))
    return np.diag(rng.uniform(0.1, 0.4, nch)) + np.diag(off, 1) + np.diag(off, -1)


def _operators(prob, SB, G2, nch, rng):
    """The five operators (B (5, nch, nch), GE (5, 2k-1, n)): a symmetric tridiagonal B with the band of r; a dense random B with the
    band of r d/dr, which is not symmetric; B = 1 with the overlap's full band; a dense B with one all-zero row and the band of d/dr;
    B = 0 with the band of r"""
    r = prob.quadrature()[0]
    rddr = prob.operator_bands(r, [1])[0]
    holed = rng.standard_normal((nch, nch))
    holed[nch // 2] = 0.0
    B = np.stack([_tridiagonal(nch, rng), rng.standard_normal((nch, nch)), np.eye(nch), holed, np.zeros((nch, nch))])
    GE = np.stack([G2[0], rddr, host.band_symmetric(SB), G2[1], G2[0]])
    assert np.max(np.abs(rddr - rddr[::-1])) > 1e-3             # not even persymmetric, let alone symmetric
    return np.ascontiguousarray(B), np.ascontiguousarray(GE)


@functools.lru_cache(maxsize=None)
def _case(name, nch, nsteps, nscan=NSCAN, tridiagonal_only=False):
    """The shared description of a case and its main run (resolvent_slots = 2, tdse_split_group = 3, obs_every = 2, snap_every = 3),
    test_gpu_tdse_split's with the operators.  Computed once, never changed."""
    prob, SB, HB, WB, G2 = coupled._assembled(name)
    n = prob.nfun
    rng = np.random.default_rng(300 + nch)
    l = [c % 2 for c in range(nch)]
    Q, lam = _angular(nch, rng)
    f = rng.uniform(0.2, 1.0, (nsteps, nscan))
    c0 = (rng.standard_normal((nscan, nch, n)) + 1j * rng.standard_normal((nscan, nch, n))) / np.sqrt(n)
    c0[0] = c0[0].real                                         # one real packet
    P = rng.standard_normal((2, nch, n)) + 1j * rng.standard_normal((2, nch, n))
    G = np.ascontiguousarray(G2[0])
    B, GE = _operators(prob, SB, G2, nch, rng)
    if tridiagonal_only:
        B, GE = B[:1], GE[:1]
    kw = dict(G=G, Q=Q, lam=lam)
    with _Options(resolvent_slots=SLOTS, tdse_split_group=GROUP):
        c, info, obs, snaps = prob.tdse_split_observe(l, c0, DT, nsteps, f=f, P=P, obs_every=OBS_EVERY, snap_every=SNAP_EVERY, expect=(B, GE), **kw)
        e0 = prob.spline_expect(c0, B, GE)
    for v in (c0, f, P, G, Q, lam, B, GE, c, info, obs, snaps, e0):
        v.setflags(write=False)
    return dict(prob=prob, SB=SB, HB=HB, G=G, Q=Q, lam=lam, n=n, k=prob.k, nch=nch, nsteps=nsteps, nscan=nscan, l=l, f=f, c0=c0, P=P, kw=kw,
                B=B, GE=GE, c=c, info=info, obs=obs, snaps=snaps, e0=e0)


def _check_accuracy(d, packets, e):
    """|e - e_ld| <= 2 (n + 2 nch + 2k + 4) eps sum |terms| for every packet (.., nch, n) and operator; the worst ratio"""
    packets = np.asarray(packets).reshape(-1, d["nch"], d["n"])
    e = np.asarray(e).reshape(packets.shape[0], -1)
    worst = 0.0
    for q in range(packets.shape[0]):
        eld, mag = eref.expect_ld(packets[q], d["B"], d["GE"])
        for o in range(e.shape[1]):
            err, bound = abs(complex(eld[o]) - e[q, o]), eref.bound(d["n"], d["nch"], d["k"], mag[o])
            assert err <= bound, (q, o, err, bound)
            if bound > 0.0:
                worst = max(worst, err / bound)
    return worst


@pytest.mark.parametrize("name,nch,nsteps", SHAPES, ids=IDS)
def test_expect_call_is_deterministic_independent_and_accurate(name, nch, nsteps):
    """E1, E2, E3 and the accuracy of bspatom_spline_expect on the five packets of a case (scan 0 real): a second run; every scan
    alone; every operator alone; one work slot, two, the default; the _dev variant on a result pre-filled with NaN -- all bit for
    bit.  A real packet gives Im e = +-0.0; B = 0 gives +0.0 in both entries; B = 1 with the overlap's band gives sum_c N_c of the row
    within the bound.  Every value against the long-double definition within m eps sum |terms|, m = 2 (n + 2 nch + 2k + 4): a leaf
    term passes through at most 3 multiplications and nch - 1 (mix) + 2k - 1 (band) + ceil(n / 64) + 6 (lane sums and tree) + nch
    (channels) + 1 (complex product) additions, together below n + 2 nch + 2k + 4; the factor 2 for the two components.  And against
    the header's order of operations in float64 NumPy (spline_expect_ref.expect_f64) bit for bit."""
    d = _case(name, nch, nsteps)
    prob, c0, B, GE, e0 = d["prob"], d["c0"], d["B"], d["GE"], d["e0"]
    assert e0.shape == (NSCAN, NEXP) and np.all(np.isfinite(e0.view(np.float64))) and np.max(np.abs(e0[:, 0])) > 1e-3
    with _Options(resolvent_slots=SLOTS):
        assert same(prob.spline_expect(c0, B, GE), e0), "second run"
        for q in range(NSCAN):
            eq = prob.spline_expect(c0[q], B, GE)
            assert eq.shape == (NEXP,) and same(eq, e0[q]), q
        for o in range(NEXP):
            assert same(prob.spline_expect(c0, B[o], GE[o])[:, 0], e0[:, o]), o
    for slots in (1, 0):
        with _Options(resolvent_slots=slots):
            assert same(prob.spline_expect(c0, B, GE), e0), slots
    put = lambda v: torch.from_numpy(np.array(v)).to("cuda:0")
    cd, Gd = put(c0), put(GE)
    ed = torch.full((NSCAN, NEXP), float("nan"), dtype=torch.complex128, device="cuda:0")
    torch.cuda.synchronize()
    prob.spline_expect_dev(NSCAN, cd.data_ptr(), B, Gd.data_ptr(), ed.data_ptr())
    assert same(ed.cpu().numpy(), e0), "_dev"
    # E3
    assert np.all(e0[0].imag == 0.0)
    zero = np.ascontiguousarray(e0[:, 4]).view(np.float64)
    assert np.all(zero == 0.0) and not np.any(np.signbit(zero))
    norms = prob.tdse_split(d["l"], c0, DT, 0, obs_every=1)[2][0].sum(-1)
    for q in range(NSCAN):
        _, mag = eref.expect_ld(c0[q], B[2], GE[2])
        assert abs(e0[q, 2].real - norms[q]) <= eref.bound(d["n"], nch, d["k"], mag[0]), q
    worst = _check_accuracy(d, c0, e0)
    print("%s nch %d: worst |e - e_ld| / bound %.3g" % (name, nch, worst))
    note("spline_expect %s nch %d: max |e - e_ld| / bound = %.3g" % (name, nch, worst))
    for q in range(NSCAN):
        assert same(eref.expect_f64(c0[q], B, GE), e0[q]), ("expect_f64", q)


@pytest.mark.parametrize("name,nch,nsteps", SHAPES, ids=IDS)
def test_observe_leaves_the_run_as_it_was(name, nch, nsteps):
    """E4: c, the snapshots, info and the first nch + 2 nproj entries of every row of tdse_split_observe equal tdse_split's with the
    same arguments, bit for bit; with nexp = 0 and with expect=None the whole obs is equal; the _dev variant equals the host's."""
    d = _case(name, nch, nsteps)
    prob, l, c0, f, P, kw, n = d["prob"], d["l"], d["c0"], d["f"], d["P"], d["kw"], d["n"]
    RW0 = nch + 4
    assert d["obs"].shape == (capi.Problem.tdse_nobs(nsteps, OBS_EVERY), NSCAN, RW0 + 2 * NEXP) and np.all(d["info"] == 0)
    args = dict(f=f, P=P, obs_every=OBS_EVERY, snap_every=SNAP_EVERY, **kw)
    with _Options(resolvent_slots=SLOTS, tdse_split_group=GROUP):
        c, info, obs, snaps = prob.tdse_split(l, c0, DT, nsteps, **args)
        none = prob.tdse_split_observe(l, c0, DT, nsteps, expect=(np.zeros((0, nch, nch)), np.zeros((0, 2 * d["k"] - 1, n))), **args)
        plain = prob.tdse_split_observe(l, c0, DT, nsteps, expect=None, **args)
    assert same(d["c"], c) and np.array_equal(d["info"], info) and same(d["snaps"], snaps) and same(d["obs"][..., :RW0], obs)
    for res in (none, plain):
        assert same(res[0], c) and np.array_equal(res[1], info) and same(res[2], obs) and same(res[3], snaps)
    put = lambda v: torch.from_numpy(np.array(v)).to("cuda:0")
    cd, Gd, Pd, fd, GEd = put(c0), put(d["G"]), put(P), put(f.astype(np.complex128)), put(d["GE"])
    od = torch.full(d["obs"].shape, float("nan"), dtype=torch.float64, device="cuda:0")
    sd = torch.full(d["snaps"].shape, float("nan"), dtype=torch.complex128, device="cuda:0")
    torch.cuda.synchronize()
    with _Options(resolvent_slots=SLOTS, tdse_split_group=GROUP):
        infod = prob.tdse_split_observe_dev(l, NSCAN, nsteps, DT, cd.data_ptr(), G_ptr=Gd.data_ptr(), Q=d["Q"], lam=d["lam"], f_ptr=fd.data_ptr(),
                                            nproj=2, P_ptr=Pd.data_ptr(), obs_every=OBS_EVERY, obs_ptr=od.data_ptr(), snap_every=SNAP_EVERY,
                                            snap_ptr=sd.data_ptr(), expect=(d["B"], GEd.data_ptr()))
    assert same(cd.cpu().numpy(), c) and np.array_equal(infod, info) and same(od.cpu().numpy(), d["obs"]) and same(sd.cpu().numpy(), snaps)


@pytest.mark.parametrize("name,nch,nsteps", SHAPES, ids=IDS)
def test_rows_are_the_expect_call_on_the_runs_packets(name, nch, nsteps):
    """E5 and the accuracy along a run: with obs_every = snap_every = 1 the new entries of row j equal spline_expect on the packet
    of step j -- c0, the snapshots, the returned c --, the last row equals a call with nsteps = 0 on the returned c, all bit for bit;
    and every entry lies within the bound of the long-double definition on that packet."""
    d = _case(name, nch, nsteps)
    prob, l, P, kw = d["prob"], d["l"], d["P"], d["kw"]
    ex = (d["B"], d["GE"])
    c, _, obs, snaps = prob.tdse_split_observe(l, d["c0"], DT, nsteps, f=d["f"], P=P, obs_every=1, snap_every=1, expect=ex, **kw)
    assert obs.shape == (nsteps + 1, NSCAN, nch + 4 + 2 * NEXP) and same(c, d["c"]) and same(snaps[-1], c)
    rows = host.split_expect_rows(obs, nch, 2)
    assert rows.shape == (nsteps + 1, NSCAN, NEXP)
    packets = np.concatenate([d["c0"][None], snaps])
    for j in range(nsteps + 1):
        assert same(rows[j], prob.spline_expect(packets[j], *ex)), j
    assert same(rows[0], d["e0"])
    c1, _, o1 = prob.tdse_split_observe(l, c, DT, 0, P=P, obs_every=1, expect=ex)
    assert same(c1, c) and o1.shape == (1, NSCAN, nch + 4 + 2 * NEXP) and same(o1[0], obs[-1])
    worst = _check_accuracy(d, packets, rows)
    print("%s nch %d: worst |e - e_ld| / bound over the rows %.3g" % (name, nch, worst))
    note("tdse_split_observe %s nch %d: max |e - e_ld| / bound over the rows = %.3g" % (name, nch, worst))


@pytest.mark.parametrize("name,nch,nsteps", SHAPES, ids=IDS)
def test_rows_do_not_depend_on_how_the_run_is_cut(name, nch, nsteps):
    """E1 and E6: the main run against a second run; tdse_split_group = 1 and the default; tdse_stage_mb = 1; one work slot;
    obs_every = 1 (the common steps); snap_every = 1 and 0; no projection and one -- the new entries, and everything else, bit for bit."""
    d = _case(name, nch, nsteps)
    prob, l, c0, f, P, kw = d["prob"], d["l"], d["c0"], d["f"], d["P"], d["kw"]
    RW0 = nch + 4
    run = lambda **over: prob.tdse_split_observe(l, c0, DT, nsteps, **{**dict(f=f, P=P, obs_every=OBS_EVERY, snap_every=SNAP_EVERY,
                                                                             expect=(d["B"], d["GE"])), **kw, **over})
    for opts in (dict(resolvent_slots=SLOTS, tdse_split_group=GROUP), dict(tdse_split_group=1), dict(), dict(tdse_split_group=GROUP, tdse_stage_mb=1),
                 dict(resolvent_slots=1)):
        with _Options(**opts):
            res = run()
        assert same(res[0], d["c"]) and same(res[2], d["obs"]) and same(res[3], d["snaps"]), opts
    o1 = run(obs_every=1)[2]
    assert same(o1[:-1][::OBS_EVERY], d["obs"][:-1]) and same(o1[-1], d["obs"][-1])
    assert same(run(snap_every=1)[2], d["obs"]) and same(run(snap_every=0)[2], d["obs"])
    o0 = run(P=None)[2]
    assert o0.shape[-1] == nch + 2 * NEXP and same(o0[..., nch:], d["obs"][..., RW0:]) and same(o0[..., :nch], d["obs"][..., :nch])
    o1p = run(P=P[:1])[2]
    assert same(o1p[..., nch + 2:], d["obs"][..., RW0:])
    for q in (0, NSCAN - 1):                                   # a scan alone
        oq = prob.tdse_split_observe(l, c0[q], DT, nsteps, f=f[:, q:q + 1], P=P, obs_every=OBS_EVERY, expect=(d["B"], d["GE"]), **kw)[2]
        assert same(oq[:, 0], d["obs"][:, q]), q


def test_many_scans_staged_step_by_step():
    """the rows where the staging bound bites: lin256 with nch = 4 and 40 scans under tdse_stage_mb = 1 -- a snapshot of all scans is
    640 KB, the host variant stages step by step --: every scan's rows equal its original's"""
    d = _case("lin256", 4, 7)
    rep = 8
    c0, f = np.tile(d["c0"], (rep, 1, 1)), np.tile(d["f"], (1, rep))
    with _Options(tdse_stage_mb=1):
        c, info, obs, snaps = d["prob"].tdse_split_observe(d["l"], c0, DT, 7, f=f, P=d["P"], obs_every=OBS_EVERY, snap_every=SNAP_EVERY,
                                                           expect=(d["B"], d["GE"]), **d["kw"])
    assert same(c, np.tile(d["c"], (rep, 1, 1))) and np.all(info == 0)
    assert same(obs, np.tile(d["obs"], (1, rep, 1))) and same(snaps, np.tile(d["snaps"], (1, rep, 1, 1)))


def test_twenty_nine_channels():
    """lin256 with nch = 29, three steps of two packets and the tridiagonal B with the band of r: every row entry meets the accuracy
    bound (the long-double side needs band-sized matrix products alone), and the rows equal spline_expect on the packets"""
    nch, nsteps, nscan = 29, 3, 2
    d = _case("lin256", nch, nsteps, nscan, True)
    prob = d["prob"]
    ex = (d["B"], d["GE"])
    assert d["B"].shape == (1, nch, nch) and np.count_nonzero(d["B"][0]) == 3 * nch - 2
    c, info, obs, snaps = prob.tdse_split_observe(d["l"], d["c0"], DT, nsteps, f=d["f"], obs_every=1, snap_every=1, expect=ex, **d["kw"])
    assert np.all(info == 0) and same(c, d["c"])
    rows = host.split_expect_rows(obs, nch, 0)
    packets = np.concatenate([d["c0"][None], snaps])
    for j in range(nsteps + 1):
        assert same(rows[j], prob.spline_expect(packets[j], *ex)), j
    worst = _check_accuracy(d, packets, rows)
    assert np.max(np.abs(rows)) > 1e-3
    note("tdse_split_observe lin256 nch 29: max |e - e_ld| / bound = %.3g" % worst)


def _hyd4():
    prob = capi.Problem(capi.make_input(**coupled.HYD4))
    E, sinfo = prob.solve(0, 2)
    assert np.all(sinfo == 0)
    return prob, E


def test_field_free_beat():
    """Hydrogen on coupled.HYD4's grid, channels l = 0, 1, c = (x_1s, x_2p) / sqrt 2 and f = 0: the scheme is exact on eigenvectors,
    every step multiplies x by rho = ((1 - i E dt/4) / (1 + i E dt/4))^2, so row n of the dipole is
        2 Re(conj(a_s) a_p (rho_p conj(rho_s))^n) A_01 x_p^T G_r x_s,   a_s = a_p = 1 / sqrt 2, A_01 = 1 / sqrt 3.
    Tolerance 8 max(delta_ref, eps nsteps), delta_ref the deviation of the dense restatement's own rows (tests/tdse_split_ref.py, the
    dipole from its packets in float64 NumPy) from the same formula."""
    prob, E = _hyd4()
    n, nsteps, dt = prob.nfun, 24, 0.25
    chans = [(0, 0), (1, 0)]
    V = prob.eigvecs_batch(0, 2, 1, 1)[:, 0]
    SB, HB = prob.assemble(0, 2)
    B, GE = host.split_expect_dipole(prob, chans)
    c0 = np.stack([V[0], V[1]]).astype(np.complex128) / np.sqrt(2.0)
    ang = host.split_angular(chans)
    c, info, obs = host.split_propagate(prob, [0, 1], c0, dt, ang, np.zeros(nsteps), obs_every=1, expect=(B, GE))
    assert np.all(info == 0)
    rows = host.split_expect_rows(obs, 2, 0)[:, 0, 0]
    Gd = ref.full_to_dense(GE[0])
    amp = B[0, 0, 1] * float(V[1] @ Gd @ V[0])
    rho = [((1 - 0.25j * dt * e) / (1 + 0.25j * dt * e)) ** 2 for e in (E[0, 0], E[1, 0])]
    closed = np.array([2.0 * (0.5 * (rho[1] * np.conj(rho[0])) ** m).real * amp for m in range(nsteps + 1)])
    _, traj, _ = pref.propagate(SB, HB, [0, 1], dt, c0, GE[0], ang[0], ang[1], np.zeros(nsteps))
    dref = np.array([np.sum(np.conj(p) * ((B[0] @ p) @ Gd.T)).real for p in np.concatenate([c0[None], traj])])
    delta_ref = float(np.max(np.abs(dref - closed)))
    dev = float(np.max(np.abs(rows.real - closed)))
    tol = 8.0 * max(delta_ref, EPS * nsteps)
    print("beat: amplitude A_01 x_p^T G_r x_s = %.12f (hydrogen 1s-2p: 128 sqrt 2 / 243 = %.12f); deviation %.3e, restatement %.3e, tolerance %.3e"
          % (abs(amp), 128.0 * np.sqrt(2.0) / 243.0, dev, delta_ref, tol))
    note("tdse_split_observe beat: deviation %.3e, restatement's %.3e, amplitude %.9f" % (dev, delta_ref, abs(amp)))
    assert np.ptp(closed) > abs(amp)                         # t = 6 is more than a third of the beat period 2 pi / 0.375
    assert np.max(np.abs(rows.imag)) <= tol and dev <= tol, (dev, delta_ref, tol)
    prob.close()


def test_dipole_rows_are_second_order():
    """test_gpu_tdse_spline's order test on the dipole rows: two channels (l = 0, 1) of n65_k4 -- the grid that test takes, so that
    ALL 130 states span the spline space --, from 1s through its pulse (sin^2 envelope, T = 12, F0 = 0.05).  Reference: tdse_lawson at
    dt = 0.0125, own err below 1e-11, <z> = -2 Re z from host.tdse_expectations (tdse_system's blocks carry the reference's phase -1,
    so the split call runs with f = -F and its <cos theta r> is minus that dipole).  The largest deviation of the dipole rows over
    the common times t = 0, 0.1, .. 12 at dt = 0.1 and at 0.05 must fall in the ratio 3.9 .. 4.1: a second-order error C dt^2 (1 +
    O(dt^2)), the window and the reasoning of the population test.  tests/test_spline_expect_cpu.py shows the dense restatement in
    the window first (4.0002 there)."""
    prob = capi.Problem(single._input("n65_k4"))
    E_, sinfo = prob.solve(0, 2)
    assert np.all(sinfo == 0)
    n, chans, T = prob.nfun, [(0, 0), (1, 0)], sref.PULSE["T"]
    E, pairs, D = host.tdse_system(prob, chans, 1, n, kind_pi=1)
    V = prob.eigvecs_batch(0, 2, 1, n)
    dtl = 0.0125
    a0 = np.zeros((1, 2, n), dtype=np.complex128); a0[0, 0, 0] = 1.0
    a, err, lobs = prob.tdse_lawson(E, pairs, D, a0, host.field_table([sref.pulse], 0.0, dtl, int(round(T / dtl))), dtl, obs_every=8)
    assert err[0] < 1e-11
    zref = -host.tdse_expectations(lobs)[2][:, 0]
    ex = host.split_expect_dipole(prob, chans)
    ang = host.split_angular(chans)
    c0 = host.spline_packet(prob, chans, 0, V[0, 0])
    errs = []
    for dt, every in ((0.1, 1), (0.05, 2)):
        ns = int(round(T / dt))
        F = -sref.pulse(host.spline_midpoints(0.0, dt, ns))
        c, info, obs = host.split_propagate(prob, [0, 1], c0, dt, ang, F, obs_every=every, expect=ex)
        z = host.split_expect_rows(obs, 2, 0)[:, 0, 0]
        assert np.all(info == 0) and z.shape == zref.shape and np.max(np.abs(z.imag)) < 1e-12
        errs.append(float(np.max(np.abs(z.real - zref))))
        print("dt %.3f: largest dipole deviation %.3e (largest |<z>| %.4e)" % (dt, errs[-1], np.max(np.abs(zref))))
    ratio = errs[0] / errs[1]
    note("tdse_split_observe dipole against tdse_lawson: %.3e (dt 0.1), %.3e (dt 0.05), ratio %.4f" % (errs[0], errs[1], ratio))
    assert 3.9 <= ratio <= 4.1, (errs, ratio)
    prob.close()


def test_argument_checks():
    prob = capi.Problem(single._input("n65_k4"))
    n, k, L = prob.nfun, prob.k, capi.lib()
    p_ = lambda x: x.ctypes.data_as(C.c_void_p)
    i32 = lambda v: np.array(v, dtype=np.int32)
    dv = lambda v: torch.from_numpy(v).to("cuda:0")
    dp = lambda t: C.c_void_p(t.data_ptr())
    nch, nscan, nsteps, nexp = 2, 2, 2, 2
    B, GE = np.ones(nexp * nch * nch), np.ones(nexp * (2 * k - 1) * n)
    c, e = np.ones(2 * nscan * nch * n), np.zeros(2 * nscan * nexp)
    GEd, cd, ed = dv(GE), dv(c), dv(e)
    # 0 p, 1 nscan, 2 nch, 3 nexp, 4 B, 5 GE, 6 c, 7 e
    for fn, ge, cc, ee in ((L.bspatom_spline_expect, p_(GE), p_(c), p_(e)), (L.bspatom_spline_expect_dev, dp(GEd), dp(cd), dp(ed))):
        good = [prob._h, nscan, nch, nexp, p_(B), ge, cc, ee]
        sub = lambda pos, v: [v if i == pos else g_ for i, g_ in enumerate(good)]
        assert fn(*good) == 0                                  # no bands needed: before any solve or assemble
        for pos in (0, 6, 7):                                  # p, c, e
            assert fn(*sub(pos, None)) == -2, pos
        for pos in (1, 2):                                     # nscan, nch below 1
            assert fn(*sub(pos, 0)) == -2 and fn(*sub(pos, -1)) == -2, pos
        assert fn(*sub(3, -1)) == -2                           # nexp < 0
        for pos in (4, 5):                                     # B, GE NULL with nexp > 0
            assert fn(*sub(pos, None)) == -2, pos
        assert fn(*[0 if i == 3 else (None if i in (4, 5) else g_) for i, g_ in enumerate(good)]) == 0    # nexp = 0 writes nothing
        assert fn(*good) == 0
    torch.cuda.synchronize()
    assert np.array_equal(ed.cpu().numpy(), e) and np.all(e.reshape(-1, 2)[:, 0] > 0.0)
    # the observing call: the checks of bspatom_tdse_split, then its own
    l, w = i32([0, 1]), i32([-1, 0])
    WB, GB = np.zeros((2 * k - 1) * n), np.ones((2 * k - 1) * n)
    Q, lam = np.array([[0.6, 0.8], [0.8, -0.6]]), np.array([-0.5, 0.5])
    f = np.array([0.1, 0.0] * (nsteps * nscan))
    P = np.ones(2 * nch * n)
    snap, obs, info = np.zeros(2 * nscan * nch * n), np.zeros(3 * nscan * (nch + 2 + 2 * nexp)), np.zeros(nscan, dtype=np.int32)
    WBd, GBd, fd, Pd, snapd, obsd = dv(WB), dv(GB), dv(f), dv(P), dv(snap), dv(obs)
    variants = ((L.bspatom_tdse_split_observe, p_(WB), p_(GB), p_(f), p_(c), p_(snap), p_(P), p_(obs), p_(GE)),
                (L.bspatom_tdse_split_observe_dev, dp(WBd), dp(GBd), dp(fd), dp(cd), dp(snapd), dp(Pd), dp(obsd), dp(GEd)))
    # 0 .. 20 as bspatom_tdse_split (19 obs, 20 info), 21 nexp, 22 B, 23 GE
    args = lambda wb, gb, fv, cv, sn, pp, ob, ge: [prob._h, nscan, nch, p_(l), 1, wb, p_(w), gb, p_(Q), p_(lam), nsteps, 0.05, fv, cv, 2, sn, 1, 1,
                                                   pp, ob, p_(info), nexp, p_(B), ge]
    for fn, *ptrs in variants:                                 # before any solve or assemble: no channel is there
        assert fn(*args(*ptrs)) == -2
    prob.assemble(0, 2)
    for fn, *ptrs in variants:
        good = args(*ptrs)
        sub = lambda pos, v: [v if i == pos else g_ for i, g_ in enumerate(good)]
        assert fn(*good) == 0
        for pos in (0, 3, 13, 20):                             # p, l, c, info
            assert fn(*sub(pos, None)) == -2, pos
        assert fn(*sub(10, -1)) == -2 and fn(*sub(16, -1)) == -2 and fn(*sub(19, None)) == -2
        assert fn(*sub(21, -1)) == -2                          # nexp < 0
        for pos in (22, 23):                                   # B, GE NULL with nexp > 0
            assert fn(*sub(pos, None)) == -2, pos
    prob.close()
    # k = 17 is refused where it is today: where its problem is created (BSPATOM_MAX_K)
    with pytest.raises(capi.BspAtomError) as ei:
        capi.Problem(capi.make_input(kind_grid=0, rb=100.0, k=17, nfun=64))
    assert ei.value.code == -5
