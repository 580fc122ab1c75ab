"""The TDSE in the spline basis (bspatom_tdse_spline / _dev, csrc/tdse_spline.hip): the guarantees S1 - S5 of its header part bit for
bit -- above all the composition S3: a step IS host.band_apply, Problem.resolvent_coupled at z = 2i/dt and two NumPy operations --, the
rows against a long-double evaluation on the run's own snapshots, then the physics end to end (an eigenvector's phase, the norm, the
second order against the eigenbasis route) and the argument checks.  The dense reference is tests/tdse_spline_ref.py; fixtures and
helpers come from test_gpu_resolvent_coupled / test_gpu_resolvent."""
import ctypes as C
import functools
import numpy as np
import pytest
import torch                               # first: its HIP runtime is the one the process uses
from test_gpu_stages import note

import resolvent_ref as ref
import tdse_spline_ref as sref
import test_gpu_resolvent as single
import test_gpu_resolvent_coupled as coupled
from bspatom_amd import capi, host

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
same = single._same
DT = 0.05
NSCAN, SLOTS, GROUP, OBS_EVERY, SNAP_EVERY = 5, 2, 3, 2, 3
# (fixture, nch, nsteps): N < 2 bw + 1; bw = 11; bw = 35; the limit bw = 63 with two steps
SHAPES = [("tiny8", 2, 7), ("n65_k4", 3, 7), ("lin256", 4, 7), ("k16_n40", 4, 2)]
CASES = [(name, nch, nsteps, absorb) for name, nch, nsteps in SHAPES for absorb in (False, True)]
IDS = ["%s-nch%d-%s" % (c[0], c[1], "cap" if c[3] else "nocap") for c in CASES]


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


@functools.lru_cache(maxsize=None)
def _case(name, nch, nsteps, absorb):
    """The shared description of a case and its main run (resolvent_slots = 2: a slot takes several of the five scans;
    tdse_spline_group = 3, obs_every = 2, snap_every = 3: none divides nsteps = 7).  Computed once, never changed."""
    prob, SB, HB, WB, G = coupled._assembled(name)
    n = prob.nfun
    rng = np.random.default_rng(100 + nch)
    l = [c % 2 for c in range(nch)]
    cp = coupled._topology(nch)
    # test_gpu_resolvent_coupled's complex coefficient pair at strength 0.3, times a real pulse value per step and scan
    F = rng.uniform(0.2, 1.0, (nsteps, NSCAN))
    coef = np.ascontiguousarray(F[:, :, None, None] * coupled._coefficients(nch, 0.3)[None, None])
    c0 = (rng.standard_normal((NSCAN, nch, n)) + 1j * rng.standard_normal((NSCAN, nch, n))) / np.sqrt(n)
    c0[0] = c0[0].real                                         # one real packet
    P = rng.standard_normal((2, nch, n)) + 1j * rng.standard_normal((2, nch, n))
    kw = dict(couplings=cp, G=G, W=WB if absorb else None, w=([0] + [-1] * (nch - 1)) if absorb else None)
    with _Options(resolvent_slots=SLOTS, tdse_spline_group=GROUP):
        c, info, obs, snaps = prob.tdse_spline(l, c0, DT, nsteps, coef=coef, P=P, obs_every=OBS_EVERY, snap_every=SNAP_EVERY, **kw)
    for v in (c0, coef, P, c, info, obs, snaps):
        v.setflags(write=False)
    return dict(prob=prob, SB=SB, HB=HB, WB=WB, G=G, n=n, nch=nch, nsteps=nsteps, l=l, cp=cp, coef=coef, c0=c0, P=P, kw=kw, c=c, info=info,
                obs=obs, snaps=snaps)


@pytest.mark.parametrize("name,nch,nsteps,absorb", CASES, ids=IDS)
def test_determinism_and_independence(name, nch, nsteps, absorb):
    """S1 and S2 bitwise: the main run against a second run; every scan alone; the default work slots and one slot; launches of one
    step and of the default length; obs_every = 1 and 0, snap_every = 1 and 0, no projections; the _dev variant on torch tensors
    pre-filled with NaN."""
    d = _case(name, nch, nsteps, absorb)
    prob, l, c0, coef, P, kw = d["prob"], d["l"], d["c0"], d["coef"], d["P"], d["kw"]
    n = d["n"]
    assert np.all(d["info"] == 0) and np.all(np.isfinite(d["c"].view(np.float64))) and np.max(np.abs(d["c"] - c0)) > 1e-3
    assert d["snaps"].shape == (nsteps // SNAP_EVERY, NSCAN, nch, n) and d["obs"].shape == (capi.Problem.tdse_nobs(nsteps, OBS_EVERY), NSCAN, nch + 4)
    run = lambda **over: prob.tdse_spline(l, c0, DT, nsteps, **{**dict(coef=coef, P=P, obs_every=OBS_EVERY, snap_every=SNAP_EVERY), **kw, **over})
    def check(res, what):
        assert same(res[0], d["c"]) and np.array_equal(res[1], d["info"]) and same(res[2], d["obs"]) and same(res[3], d["snaps"]), what
    check(run(), "second run")
    for opts in (dict(resolvent_slots=1), dict(tdse_spline_group=1), dict(resolvent_slots=SLOTS), dict(tdse_spline_group=GROUP, tdse_stage_mb=1)):
        with _Options(**opts):
            check(run(), opts)
    for q in range(NSCAN):                                     # each scan alone
        cq, iq, oq, sq = prob.tdse_spline(l, c0[q], DT, nsteps, coef=coef[:, q:q + 1], P=P, obs_every=OBS_EVERY, snap_every=SNAP_EVERY, **kw)
        assert same(cq, d["c"][q]) and iq[0] == d["info"][q] and same(oq[:, 0], d["obs"][:, q]) and same(sq[:, 0], d["snaps"][:, q]), q
    c1, _, o1, s1 = run(obs_every=1, snap_every=1)             # every step observed and kept
    assert same(c1, d["c"]) and same(o1[:-1][::OBS_EVERY], d["obs"][:-1]) and same(o1[-1], d["obs"][-1])
    assert same(s1[SNAP_EVERY - 1::SNAP_EVERY], d["snaps"])
    c2, i2 = run(obs_every=0, snap_every=0)                    # neither
    assert same(c2, d["c"]) and np.array_equal(i2, d["info"])
    _, _, o3, _ = run(P=None)                                  # no projections: the norms alone
    assert o3.shape[-1] == nch and same(o3, d["obs"][..., :nch])
    _, _, o4, _ = run(P=P[:1])
    assert same(o4, d["obs"][..., :nch + 2])
    # the _dev variant
    dev = "cuda:0"
    put = lambda v: torch.from_numpy(np.array(v)).to(dev)
    cd, Gd, Wd, Pd, coefd = put(c0), put(d["G"]), put(d["WB"]), put(P), put(coef)
    od = torch.full(d["obs"].shape, float("nan"), dtype=torch.float64, device=dev)
    sd = torch.full(d["snaps"].shape, float("nan"), dtype=torch.complex128, device=dev)
    torch.cuda.synchronize()
    infod = prob.tdse_spline_dev(l, NSCAN, nsteps, DT, cd.data_ptr(), couplings=d["cp"], nop=2, G_ptr=Gd.data_ptr(), coef_ptr=coefd.data_ptr(),
                                 nabs=1 if absorb else 0, W_ptr=Wd.data_ptr() if absorb else None, w=kw["w"], nproj=2, P_ptr=Pd.data_ptr(),
                                 obs_every=OBS_EVERY, obs_ptr=od.data_ptr(), snap_every=SNAP_EVERY, snap_ptr=sd.data_ptr())
    check((cd.cpu().numpy(), infod, od.cpu().numpy(), sd.cpu().numpy()), "_dev")


def test_many_scans_staged_step_by_step():
    """S2 where the staging bound bites: lin256 with nch = 4 and 40 scans -- the five packets of the main run eight times over -- under
    tdse_stage_mb = 1: a snapshot of all scans is 640 KB, so the host variant stages step by step.  Every scan equals its original."""
    d = _case("lin256", 4, 7, True)
    rep = 8
    c0, coef = np.tile(d["c0"], (rep, 1, 1)), np.tile(d["coef"], (1, rep, 1, 1))
    with _Options(tdse_stage_mb=1):
        c, info, obs, snaps = d["prob"].tdse_spline(d["l"], c0, DT, 7, coef=coef, P=d["P"], obs_every=OBS_EVERY, snap_every=SNAP_EVERY, **d["kw"])
    assert same(c, np.tile(d["c"], (rep, 1, 1))) and np.all(info == 0)
    assert same(obs, np.tile(d["obs"], (1, rep, 1))) and same(snaps, np.tile(d["snaps"], (1, rep, 1, 1)))


@pytest.mark.parametrize("name,nch,nsteps,absorb", CASES, ids=IDS)
def test_step_is_band_apply_coupled_solve_update(name, nch, nsteps, absorb):
    """S3, the composition, bit for bit over the whole run: b = host.band_apply on the symmetric full band of Problem.assemble's SB (an
    index shuffle; Re and Im apart), Problem.resolvent_coupled(l, 2j/dt, B = b, a = coef[n, q]), then c' = (g x_im - c_re, -(g x_re) -
    c_im) with g = 4.0/dt in NumPy: the replay reproduces c, every snapshot and info."""
    d = _case(name, nch, nsteps, absorb)
    prob, l, kw = d["prob"], d["l"], d["kw"]
    SBf = host.band_symmetric(d["SB"])
    g, z = 4.0 / DT, complex(0.0, 2.0 / DT)
    c = np.array(d["c0"])
    info = np.zeros(NSCAN, dtype=np.int64)
    for n in range(nsteps):
        for q in range(NSCAN):
            b = host.band_apply(SBf, c[q].real) + 1j * host.band_apply(SBf, c[q].imag)
            X, _, inf = prob.resolvent_coupled(l, z, b, a=d["coef"][n, q], **kw)
            x = X[0, 0]
            c[q] = (g * x.imag - c[q].real) + 1j * (-(g * x.real) - c[q].imag)
            info[q] += inf[0]
        if (n + 1) % SNAP_EVERY == 0:
            assert same(c, d["snaps"][(n + 1) // SNAP_EVERY - 1]), n
    assert same(c, d["c"]) and np.array_equal(info, d["info"])


@pytest.mark.parametrize("name,nch,nsteps,absorb", [CASES[3], CASES[4]], ids=[IDS[3], IDS[4]])
def test_snapshot_is_the_shorter_run_and_continues(name, nch, nsteps, absorb):
    """S4: the snapshot after step 3 equals the run of 3 steps; 4 more steps from it equal the run of 7."""
    d = _case(name, nch, nsteps, absorb)
    prob, l, coef, kw = d["prob"], d["l"], d["coef"], d["kw"]
    cs, _ = prob.tdse_spline(l, d["c0"], DT, SNAP_EVERY, coef=coef[:SNAP_EVERY], **kw)
    assert same(cs, d["snaps"][0])
    cl, _ = prob.tdse_spline(l, d["snaps"][0], DT, nsteps - SNAP_EVERY, coef=coef[SNAP_EVERY:], **kw)
    assert same(cl, d["c"])


@pytest.mark.parametrize("name,nch,nsteps,absorb", CASES, ids=IDS)
def test_rows_against_long_double_on_the_snapshots(name, nch, nsteps, absorb):
    """S5: with every step observed and kept, N_c and the projections of row j against a clongdouble evaluation of Re c^H S c and
    sum P (S c) on the packet the run itself returned for that step, within (nch nfun + 2) eps sum |terms| -- test_gpu_resolvent_coupled's
    bound for R --; the last row has the bits of a call with nsteps = 0 on the returned c."""
    d = _case(name, nch, nsteps, absorb)
    prob, l, P, kw, n = d["prob"], d["l"], d["P"], d["kw"], d["n"]
    c, _, obs, snaps = prob.tdse_spline(l, d["c0"], DT, nsteps, coef=d["coef"], P=P, obs_every=1, snap_every=1, **kw)
    assert obs.shape == (nsteps + 1, NSCAN, nch + 4)
    Sl = np.asarray(ref.upper_to_dense(d["SB"]), dtype=np.longdouble)
    packets = np.concatenate([d["c0"][None], snaps])
    worst = 0.0
    for j in range(nsteps + 1):
        for q in range(NSCAN):
            cl = packets[j, q].astype(np.clongdouble)
            for ch in range(nch):
                terms = np.conj(cl[ch])[:, None] * Sl * cl[ch][None, :]
                bound = (nch * n + 2) * EPS * float(np.sum(np.abs(terms)))
                err = abs(float(np.sum(terms).real) - obs[j, q, ch])
                worst = max(worst, err / bound)
                assert err <= bound, (j, q, ch, err, bound)
            for r in range(2):
                pl = P[r].astype(np.clongdouble)
                terms = np.stack([pl[ch][:, None] * Sl * cl[ch][None, :] for ch in range(nch)])
                bound = (nch * n + 2) * EPS * float(np.sum(np.abs(terms)))
                err = abs(complex(np.sum(terms)) - complex(obs[j, q, nch + 2 * r], obs[j, q, nch + 2 * r + 1]))
                worst = max(worst, err / bound)
                assert err <= bound, (j, q, r, err, bound)
    print("%s nch %d: worst row error / bound %.3g" % (name, nch, worst))
    c0, _, o0 = prob.tdse_spline(l, c, DT, 0, P=P, obs_every=1, **kw)
    assert same(c0, c) and o0.shape == (1, NSCAN, nch + 4) and same(o0[0], obs[-1])
    assert same(o0[0], d["obs"][-1])


# ---- physics, end to end -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _n65():
    """n65_k4 solved for l = 0, 1: (problem, E (2, n), all eigenvectors V (2, n, n), SB, HB)"""
    prob = capi.Problem(single._input("n65_k4"))
    E, sinfo = prob.solve(0, 2)
    assert np.all(sinfo == 0)
    V = prob.eigvecs_batch(0, 2, 1, prob.nfun)
    SB, HB = prob.assemble(0, 2)
    return prob, E, V, SB, HB


def test_eigenvector_comes_back_with_its_cayley_phase():
    """No coupling, no absorber: an eigenvector (E, phi) returns as ((1 - i tau E) / (1 + i tau E))^nsteps phi, tau = dt / 2.  States 1,
    4, 20 and the highest of l = 0 and l = 1, each in its channel of a two-channel call, 7 steps.  The deviation from the closed form
    against the dense restatement's own (tests/tdse_spline_ref.py: the same eigenvector, numpy.linalg.solve): at most 8 times it,
    floored at eps nsteps -- the project's margin for LU against LU."""
    prob, E, V, SB, HB = _n65()
    n, nsteps = prob.nfun, 7
    picks = [(ch, s) for ch in (0, 1) for s in (0, 3, 19, n - 1)]
    c0 = np.stack([host.spline_packet(prob, [(0, 0), (1, 0)], ch, V[ch, s]) for ch, s in picks])
    c, info = prob.tdse_spline([0, 1], c0, DT, nsteps)
    assert np.all(info == 0)
    worst = 0.0
    for q, (ch, s) in enumerate(picks):
        tau = 0.5 * DT
        closed = ((1 - 1j * tau * E[ch, s]) / (1 + 1j * tau * E[ch, s])) ** nsteps * c0[q]
        cref_, _, _ = sref.propagate(SB, HB, [0, 1], DT, c0[q], nsteps)
        dev, dev_ref = np.max(np.abs(c[q] - closed)), np.max(np.abs(cref_ - closed))
        print("channel %d state %d (E %.4g): deviation %.3e  restatement %.3e" % (ch, s + 1, E[ch, s], dev, dev_ref))
        worst = max(worst, dev / max(dev_ref, EPS * nsteps))
        assert dev <= 8.0 * max(dev_ref, EPS * nsteps), (ch, s, dev, dev_ref)
    note("tdse_spline eigenvector phase: max deviation / max(restatement's, eps nsteps) = %.3g" % worst)


def test_norm_is_conserved_without_absorber():
    """Hermitian couplings (stark_system's two directions times a real pulse), no absorber: sum_c N_c stays what it was.  The largest
    drift over the rows of 7 steps against the dense restatement's on the same packet: at most 8 times it, floored at eps nsteps."""
    prob, E, V, SB, HB = _n65()
    nsteps = 7
    chans = [(0, 0), (1, 0)]
    R_r = prob.dipole_bands()[0]
    pat = host.stark_system(chans, 1.0)
    F = 0.1 * np.sin(np.pi * host.spline_midpoints(0.0, DT, nsteps) / (nsteps * DT)) ** 2
    coef = host.spline_coefficients(pat, F)
    c0 = np.stack([host.spline_packet(prob, chans, 0, V[0, 0]), (V[0, 1][None] * np.array([[0.6], [0.0]]) + V[1, 2][None] * np.array([[0.0], [0.8j]]))])
    c, info, obs = prob.tdse_spline([0, 1], c0, DT, nsteps, couplings=pat[0], G=R_r, coef=coef, obs_every=1)
    assert np.all(info == 0) and np.max(np.abs(c - c0)) > 1e-4
    for q in range(2):
        _, _, rows = sref.propagate(SB, HB, [0, 1], DT, c0[q], coef[:, 0], pat[0], R_r[None])
        tot, tot_ref = obs[:, q].sum(-1), rows.sum(-1)
        drift, drift_ref = np.max(np.abs(tot - tot[0])), np.max(np.abs(tot_ref - tot_ref[0]))
        print("packet %d: norm %.15f  drift %.3e  restatement %.3e  population moved %.3e" % (q, tot[0], drift, drift_ref, abs(obs[-1, q, 0] - obs[0, q, 0])))
        assert abs(obs[-1, q, 0] - obs[0, q, 0]) > 1e-8        # the coupling did move population between the channels
        assert drift <= 8.0 * max(drift_ref, EPS * nsteps) * max(1.0, tot[0]), (q, drift, drift_ref)
        assert abs(host.spline_yield(obs)[-1, q] - (1.0 - tot[-1])) == 0.0


def test_second_order_against_the_eigenbasis_route():
    """Two channels (l = 0, 1) of n65_k4 with ALL 65 states each -- the eigenbasis then spans the spline space, both routes integrate the
    same equation --, from 1s through the pulse of tdse_spline_ref (sin^2 envelope, T = 12, about one cycle, F0 = 0.05).  Reference:
    tdse_lawson at dt = 0.0125, whose own err must be below 1e-11 (3.8e-11 at 0.025 on the CPU restatement, fifth order).  The
    populations |phi_s^T S c|^2, from the projections of the last row of the spline run with the eigenvectors as P, at dt = 0.1 and at
    0.05: the largest deviation from the reference over all 130 states must drop in the ratio 4.  Window 3.9 .. 4.1: the error of a
    second-order scheme is C dt^2 (1 + O(dt^2)), so the ratio leaves 4 by a relative O(dt^2), and 2.5 % is the room given to that term
    and to the reference's 1e-11; it excludes first order (2) and anything better than second (>= 8).  Measured once on the CPU with
    the dense restatement in place of the GPU call and DOP853 (rtol 1e-13) as the reference: 3.9982 at dt = 0.1 (errors 1.451e-05 and
    3.630e-06), 3.9928 at dt = 0.2, 3.9996 at dt = 0.05 -- dt = 0.1 sits well inside."""
    prob = capi.Problem(single._input("n65_k4"))
    E_, sinfo = prob.solve(0, 2)
    assert np.all(sinfo == 0)
    n, chans, T = prob.nfun, [(0, 0), (1, 0)], sref.PULSE["T"]
    E, pairs, D = host.tdse_system(prob, chans, 1, n, kind_pi=1)
    V = prob.eigvecs_batch(0, 2, 1, n)
    R_r = prob.dipole_bands()[0]
    dtl = 0.0125
    a0 = np.zeros((1, 2, n), dtype=np.complex128); a0[0, 0, 0] = 1.0
    a, err = prob.tdse_lawson(E, pairs, D, a0, host.field_table([sref.pulse], 0.0, dtl, int(round(T / dtl))), dtl)
    print("tdse_lawson reference: err %.3e" % err[0])
    assert err[0] < 1e-11
    pref = np.abs(a[0]) ** 2
    pat = host.stark_system(chans, -1.0)                       # the pattern of tdse_system's blocks: c0 c1, the reference's phase included
    P = np.zeros((2 * n, 2, n))
    for ch in range(2):
        P[ch * n:(ch + 1) * n, ch] = V[ch]
    c0 = host.spline_packet(prob, chans, 0, V[0, 0])
    errs = []
    for dt in (0.1, 0.05):
        ns = int(round(T / dt))
        coef = host.spline_coefficients(pat, sref.pulse(host.spline_midpoints(0.0, dt, ns)))
        c, info, obs = prob.tdse_spline([0, 1], c0, dt, ns, couplings=pat[0], G=R_r, coef=coef, P=P, obs_every=ns)
        assert np.all(info == 0) and obs.shape == (2, 1, 2 + 4 * n)
        amp = obs[-1, 0, 2::2] + 1j * obs[-1, 0, 3::2]
        pops = (np.abs(amp) ** 2).reshape(2, n)
        errs.append(float(np.max(np.abs(pops - pref))))
        print("dt %.3f: largest population error %.3e (1s %.9f, 2p %.9f; norm %.15f)" % (dt, errs[-1], pops[0, 0], pops[1, 0], obs[-1, 0, :2].sum()))
    ratio = errs[0] / errs[1]
    note("tdse_spline against tdse_lawson: population errors %.3e (dt 0.1), %.3e (dt 0.05), ratio %.4f" % (errs[0], errs[1], ratio))
    assert 3.9 <= ratio <= 4.1, (errs, ratio)
    prob.close()


def test_tdse_spline_argument_checks():
    prob = capi.Problem(single._input("n65_k4"))
    n, k, L = prob.nfun, prob.k, capi.lib()
    p_ = lambda x: x.ctypes.data_as(C.c_void_p)
    i32 = lambda v: np.array(v, dtype=np.int32)
    nch, nscan, nsteps = 2, 2, 2
    l, w = i32([0, 1]), i32([-1, 0])
    cr, cc, ctr = i32([0, 1]), i32([1, 0]), i32([0, 1])
    WB, GB = np.zeros((2 * k - 1) * n), np.ones((2 * k - 1) * n)
    coef = np.array([0.1, 0.0] * (nsteps * nscan * 2))
    c, P = np.ones(2 * nscan * nch * n), np.ones(2 * nch * n)
    snap, obs, info = np.zeros(2 * nscan * nch * n), np.zeros(3 * nscan * (nch + 2)), np.zeros(nscan, dtype=np.int32)
    dv = lambda v: torch.from_numpy(v).to("cuda:0")
    WBd, GBd, coefd, cd, Pd, snapd, obsd = dv(WB), dv(GB), dv(coef), dv(c), dv(P), dv(snap), dv(obs)
    dp = lambda t: C.c_void_p(t.data_ptr())
    variants = ((L.bspatom_tdse_spline, p_(WB), p_(GB), p_(coef), p_(c), p_(snap), p_(P), p_(obs)),
                (L.bspatom_tdse_spline_dev, dp(WBd), dp(GBd), dp(coefd), dp(cd), dp(snapd), dp(Pd), dp(obsd)))
    # 0 p, 1 nscan, 2 nch, 3 l, 4 nabs, 5 WB, 6 w, 7 ncoup, 8 cr, 9 cc, 10 ctr, 11 nop, 12 GB, 13 nsteps, 14 dt, 15 coef, 16 c, 17 snap_every,
    # 18 snap, 19 obs_every, 20 nproj, 21 P, 22 obs, 23 info
    args = lambda wb, gb, co, cv, sn, pp, ob: [prob._h, nscan, nch, p_(l), 1, wb, p_(w), 2, p_(cr), p_(cc), p_(ctr), 1, gb, nsteps, 0.05, co, cv, 2,
                                               sn, 1, 1, pp, ob, p_(info)]
    for fn, *ptrs in variants:                                 # before any solve or assemble: no channel is there
        assert fn(*args(*ptrs)) == -2
    prob.assemble(0, 2)
    for fn, *ptrs in variants:
        good = args(*ptrs)
        sub = lambda pos, v: [v if i == pos else g_ for i, g_ in enumerate(good)]
        both = lambda pa, va, pb, vb: [va if i == pa else (vb if i == pb else g_) for i, g_ in enumerate(good)]
        assert fn(*good) == 0
        for pos in (0, 3, 16, 23):                             # p, l, c, info
            assert fn(*sub(pos, None)) == -2, pos
        for pos in (1, 2):                                     # nscan, nch below 1
            assert fn(*sub(pos, 0)) == -2 and fn(*sub(pos, -1)) == -2, pos
        assert fn(*sub(13, -1)) == -2                          # nsteps < 0
        for bad in (0.0, -0.05, float("inf"), float("nan")):   # dt
            assert fn(*sub(14, bad)) == -2, bad
        assert fn(*sub(15, None)) == -2                        # coef NULL with steps and couplings
        assert fn(*both(15, None, 13, 0)) == 0                 # ... but not when there is no step
        assert fn(*sub(4, -1)) == -2 and fn(*sub(5, None)) == -2              # nabs < 0; nabs = 1 without WB
        assert fn(*sub(7, -1)) == -2                           # ncoup < 0
        for bad in ([0, 2], [-1, 0]):                          # a channel outside the bands held
            assert fn(*sub(3, p_(i32(bad)))) == -2, bad
        for bad in ([-2, 0], [-1, 1]):                         # w outside -1 .. nabs-1
            assert fn(*sub(6, p_(i32(bad)))) == -2, bad
        assert fn(*sub(6, None)) == 0                          # w NULL: absorber 0 everywhere
        for pos, bad in ((8, [0, 2]), (8, [-1, 1]), (9, [2, 0]), (9, [1, -1]), (10, [0, 2]), (10, [-1, 1])):
            assert fn(*sub(pos, p_(i32(bad)))) == -2, (pos, bad)
        for pos in (8, 9, 10, 12):                             # ncoup > 0 with cr, cc, ctr or GB NULL
            assert fn(*sub(pos, None)) == -2, pos
        assert fn(*sub(11, 0)) == -2                           # ncoup > 0 with nop < 1
        assert fn(*[0 if i in (7, 11) else (None if i in (8, 9, 10, 12, 15) else g_) for i, g_ in enumerate(good)]) == 0   # ncoup = 0 needs none
        assert fn(*sub(17, -1)) == -2 and fn(*sub(17, 0)) == -2               # snap_every < 0; snap given with snap_every = 0
        assert fn(*sub(18, None)) == 0 and fn(*both(17, 0, 18, None)) == 0     # no snapshots
        assert fn(*sub(19, -1)) == -2 and fn(*sub(19, 0)) == -2               # obs_every < 0; obs given with obs_every = 0
        assert fn(*sub(22, None)) == -2                        # obs_every >= 1 with obs NULL
        assert fn(*both(19, 0, 22, None)) == 0                 # no rows
        assert fn(*sub(20, -1)) == -2 and fn(*sub(21, None)) == -2            # nproj < 0; projections without P
        assert fn(*both(20, 0, 21, None)) == 0
        assert fn(*sub(13, 0)) == 0                            # nsteps = 0 measures
        assert fn(*good) == 0                                  # a valid call afterwards
    prob.close()
    # the limit: lin256 (k = 9) with eight channels is bw = 71
    prob = capi.Problem(single._input("lin256"))
    prob.assemble(0, 2)
    with pytest.raises(capi.BspAtomError) as ei:
        prob.tdse_spline([0, 1] * 4, np.ones((8, prob.nfun)), DT, 1)
    assert ei.value.code == -5
    c7, info7 = prob.tdse_spline([0, 1, 0, 1, 0, 1, 0], np.ones((7, prob.nfun)), DT, 1)   # seven channels, bw = 62, run
    assert info7[0] == 0 and np.all(np.isfinite(c7.view(np.float64)))
    prob.close()
