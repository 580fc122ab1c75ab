"""The split-step TDSE in the spline basis (bspatom_tdse_split / _dev, csrc/tdse_split.hip): the guarantees P1 - P4 of its header part
bit for bit, the accuracy of the final packets against the dense restatement tests/tdse_split_ref.py within 8 times that restatement's
own fp64 noise, the rows against a long-double evaluation on the run's own snapshots, the norm, a 29-channel run no other call can
make, and the argument checks.  Fixtures come from test_gpu_resolvent_coupled._assembled; the channel pattern is l = c % 2, the angular
matrix a seeded random symmetric tridiagonal with Q, lam from numpy.linalg.eigh, the field real, U(0.2, 1) per step and scan."""
import ctypes as C
import functools
import numpy as np
import pytest
import torch                               # first: its HIP runtime is the one the process uses
from test_gpu_stages import note

import resolvent_ref as ref
import tdse_split_ref as pref
import test_gpu_resolvent as single
import test_gpu_resolvent_coupled as coupled
from bspatom_amd import capi, host

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
same = single._same
DT = 0.05
NSCAN, SLOTS, GROUP, OBS_EVERY, SNAP_EVERY = 5, 2, 3, 2, 3
# (fixture, nch, nsteps): n = 8 below the window width 2b + 1; n one past a wave multiple; b = 8; b = 15, the full register window;
# a single channel; b = 9: the instances for b <= 15 with rows of the register window unused (pivot_designs.GRIDS)
SHAPES = [("tiny8", 2, 7), ("n65_k4", 3, 7), ("lin256", 4, 7), ("k16_n40", 4, 2), ("n65_k4", 1, 3), ("k10_n65", 3, 3)]
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


def _angular(nch, rng):
    """(Q, lam) of a random symmetric tridiagonal angular matrix; a single channel: Q = [1], lam = [0.7]"""
    if nch == 1:
        return np.ones((1, 1)), np.array([0.7])
    off = rng.uniform(0.3, 0.7, nch - 1)
    A = np.diag(rng.uniform(-0.2, 0.2, nch)) + np.diag(off, 1) + np.diag(off, -1)
    lam, Q = np.linalg.eigh(A)
    return np.ascontiguousarray(Q), lam


@functools.lru_cache(maxsize=None)
def _case(name, nch, nsteps, absorb, nscan=NSCAN):
    """The shared description of a case and its main run (resolvent_slots = 2: a slot takes several of the systems; tdse_split_group =
    3, obs_every = 2, snap_every = 3: none divides nsteps = 7).  Computed once, never changed."""
    prob, SB, HB, WB, G2 = coupled._assembled(name)
    n = prob.nfun
    rng = np.random.default_rng(200 + nch)
    l = [c % 2 for c in range(nch)]
    Q, lam = _angular(nch, rng)
    f = rng.uniform(0.2, 1.0, (nsteps, nscan))
    c0 = (rng.standard_normal((nscan, nch, n)) + 1j * rng.standard_normal((nscan, nch, n))) / np.sqrt(n)
    c0[0] = c0[0].real                                         # one real packet
    P = rng.standard_normal((2, nch, n)) + 1j * rng.standard_normal((2, nch, n))
    G = np.ascontiguousarray(G2[0])                            # the band of r
    kw = dict(G=G, Q=Q, lam=lam, W=WB if absorb else None, w=([0] + [-1] * (nch - 1)) if absorb else None)
    with _Options(resolvent_slots=SLOTS, tdse_split_group=GROUP):
        c, info, obs, snaps = prob.tdse_split(l, c0, DT, nsteps, f=f, P=P, obs_every=OBS_EVERY, snap_every=SNAP_EVERY, **kw)
    for v in (c0, f, P, G, Q, lam, c, info, obs, snaps):
        v.setflags(write=False)
    return dict(prob=prob, SB=SB, HB=HB, WB=WB, G=G, Q=Q, lam=lam, n=n, nch=nch, nsteps=nsteps, nscan=nscan, l=l, f=f, c0=c0, P=P, kw=kw,
                c=c, info=info, obs=obs, snaps=snaps)


@functools.lru_cache(maxsize=None)
def _reference(name, nch, nsteps, absorb, nscan=NSCAN):
    """per scan: (the dense restatement's final packet, its rows, delta_ref); computed once"""
    d = _case(name, nch, nsteps, absorb, nscan)
    WB, w = (d["WB"][None], d["kw"]["w"]) if absorb else (None, None)
    return [pref.delta_ref(d["SB"], d["HB"], d["l"], DT, d["c0"][q], d["G"], d["Q"], d["lam"], d["f"][:, q], WB, w) for q in range(nscan)]


def _accuracy(d, refs):
    """the accuracy bound on every scan of a case: ||c - c_ref||_S <= 8 max(delta_ref, eps nsteps) max(1, ||c0||_S); the worst ratio"""
    S = ref.upper_to_dense(d["SB"])
    worst = 0.0
    for q, (cref_, _, delta) in enumerate(refs):
        scale = max(1.0, pref.s_norm(S, d["c0"][q]))
        err, bound = pref.s_norm(S, d["c"][q] - cref_), 8.0 * max(delta * scale, EPS * d["nsteps"] * scale)
        print("scan %d: ||c - c_ref||_S %.3e  delta_ref %.3e  bound %.3e" % (q, err, delta, bound))
        worst = max(worst, err / bound)
        assert err <= bound, (q, err, delta, bound)
    return worst


@pytest.mark.parametrize("name,nch,nsteps,absorb", CASES, ids=IDS)
def test_determinism_and_independence(name, nch, nsteps, absorb):
    """P1 and P2 bitwise: the main run against a second run; every scan alone; the default work slots, one and two; steps waited for
    one by one, by threes and by the default; tdse_stage_mb = 1; obs_every = 1 and 0, snap_every = 1 and 0; no, one and two
    projections; the _dev variant on torch tensors pre-filled with NaN."""
    d = _case(name, nch, nsteps, absorb)
    prob, l, c0, f, P, kw = d["prob"], d["l"], d["c0"], d["f"], d["P"], d["kw"]
    n = d["n"]
    assert np.all(d["info"] == 0) and np.all(np.isfinite(d["c"].view(np.float64))) and np.max(np.abs(d["c"] - c0)) > 1e-3
    assert d["snaps"].shape == (nsteps // SNAP_EVERY, NSCAN, nch, n) and d["obs"].shape == (capi.Problem.tdse_nobs(nsteps, OBS_EVERY), NSCAN, nch + 4)
    run = lambda **over: prob.tdse_split(l, c0, DT, nsteps, **{**dict(f=f, P=P, obs_every=OBS_EVERY, snap_every=SNAP_EVERY), **kw, **over})
    def check(res, what):
        assert same(res[0], d["c"]) and np.array_equal(res[1], d["info"]) and same(res[2], d["obs"]) and same(res[3], d["snaps"]), what
    check(run(), "second run")
    for opts in (dict(resolvent_slots=1), dict(resolvent_slots=SLOTS), dict(tdse_split_group=1), dict(tdse_split_group=GROUP),
                 dict(tdse_split_group=GROUP, tdse_stage_mb=1)):
        with _Options(**opts):
            check(run(), opts)
    for q in range(NSCAN):                                     # each scan alone
        cq, iq, oq, sq = prob.tdse_split(l, c0[q], DT, nsteps, f=f[:, q:q + 1], P=P, obs_every=OBS_EVERY, snap_every=SNAP_EVERY, **kw)
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
    cd, Gd, Wd, Pd, fd = put(c0), put(d["G"]), put(d["WB"]), put(P), put(f.astype(np.complex128))
    od = torch.full(d["obs"].shape, float("nan"), dtype=torch.float64, device=dev)
    sd = torch.full(d["snaps"].shape, float("nan"), dtype=torch.complex128, device=dev)
    torch.cuda.synchronize()
    infod = prob.tdse_split_dev(l, NSCAN, nsteps, DT, cd.data_ptr(), G_ptr=Gd.data_ptr(), Q=d["Q"], lam=d["lam"], f_ptr=fd.data_ptr(),
                                nabs=1 if absorb else 0, W_ptr=Wd.data_ptr() if absorb else None, w=kw["w"], nproj=2, P_ptr=Pd.data_ptr(),
                                obs_every=OBS_EVERY, obs_ptr=od.data_ptr(), snap_every=SNAP_EVERY, snap_ptr=sd.data_ptr())
    check((cd.cpu().numpy(), infod, od.cpu().numpy(), sd.cpu().numpy()), "_dev")


def test_many_scans_staged_step_by_step():
    """P2 where the staging bound bites: lin256 with nch = 4 and 40 scans -- the five packets of the main run eight times over -- under
    tdse_stage_mb = 1: a snapshot of all scans is 640 KB, so the host variant stages step by step.  Every scan equals its original."""
    d = _case("lin256", 4, 7, True)
    rep = 8
    c0, f = np.tile(d["c0"], (rep, 1, 1)), np.tile(d["f"], (1, rep))
    with _Options(tdse_stage_mb=1):
        c, info, obs, snaps = d["prob"].tdse_split(d["l"], c0, DT, 7, f=f, P=d["P"], obs_every=OBS_EVERY, snap_every=SNAP_EVERY, **d["kw"])
    assert same(c, np.tile(d["c"], (rep, 1, 1))) and np.all(info == 0)
    assert same(obs, np.tile(d["obs"], (1, rep, 1))) and same(snaps, np.tile(d["snaps"], (1, rep, 1, 1)))


@pytest.mark.parametrize("name,nch,nsteps,absorb", CASES, ids=IDS)
def test_snapshot_is_the_shorter_run_and_continues(name, nch, nsteps, absorb):
    """P3: the snapshot after step 3 equals the run of 3 steps; the remaining steps from it equal the long run."""
    if nsteps < SNAP_EVERY:
        nsteps, every = 2, 1                                   # k16_n40's two steps: the snapshot after the first
        d = _case(name, nch, nsteps, absorb)
        _, _, snaps = d["prob"].tdse_split(d["l"], d["c0"], DT, nsteps, f=d["f"], snap_every=1, **d["kw"])
        first = snaps[0]
    else:
        every = SNAP_EVERY
        d = _case(name, nch, nsteps, absorb)
        first = d["snaps"][0]
    prob, l, f, kw = d["prob"], d["l"], d["f"], d["kw"]
    cs, _ = prob.tdse_split(l, d["c0"], DT, every, f=f[:every], **kw)
    assert same(cs, first)
    if nsteps > every:
        cl, _ = prob.tdse_split(l, first, DT, nsteps - every, f=f[every:], **kw)
        assert same(cl, d["c"])


@pytest.mark.parametrize("name,nch,nsteps,absorb", CASES, ids=IDS)
def test_accuracy_against_the_restatement(name, nch, nsteps, absorb):
    """The final packet of every scan against the dense fp64 restatement (numpy.linalg.solve on the per-channel matrices built from the
    bands a caller sees): ||c - c_ref||_S <= 8 max(delta_ref, eps nsteps) max(1, ||c0||_S), delta_ref the largest S-norm difference over
    the steps between that restatement and the same steps with scipy.linalg.solve_banded, relative to max(1, ||c0||_S): the fp64 noise
    of the scheme on the case.  8 is the margin every solver test here gives an LU against an LU."""
    d = _case(name, nch, nsteps, absorb)
    worst = _accuracy(d, _reference(name, nch, nsteps, absorb))
    note("tdse_split %s nch %d %s: max ||c - c_ref||_S / bound = %.3g" % (name, nch, "cap" if absorb else "nocap", worst))


@pytest.mark.parametrize("name,nch,nsteps,absorb", CASES, ids=IDS)
def test_rows_against_long_double_on_the_snapshots(name, nch, nsteps, absorb):
    """P4 and the rows: with every step observed and kept, N_c and the projections of row j against a clongdouble evaluation of
    Re c^H S c and sum P (S c) on the packet the run itself returned for that step, within (nch nfun + 2) eps sum |terms| --
    test_gpu_tdse_spline's bound --; the last row has the bits of a call with nsteps = 0 on the returned c."""
    d = _case(name, nch, nsteps, absorb)
    prob, l, P, kw, n = d["prob"], d["l"], d["P"], d["kw"], d["n"]
    c, _, obs, snaps = prob.tdse_split(l, d["c0"], DT, nsteps, f=d["f"], P=P, obs_every=1, snap_every=1, **kw)
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
    c0, _, o0 = prob.tdse_split(l, c, DT, 0, P=P, obs_every=1, **kw)
    assert same(c0, c) and o0.shape == (1, NSCAN, nch + 4) and same(o0[0], obs[-1])
    assert same(o0[0], d["obs"][-1])
    c00, _, o00 = prob.tdse_split(l, c, DT, 0, P=P, obs_every=1)      # a call that only measures needs no G, Q, lam, f
    assert same(c00, c) and same(o00[0], obs[-1])


@pytest.mark.parametrize("name,nch,nsteps,absorb", [c for c in CASES if not c[3]], ids=[i for c, i in zip(CASES, IDS) if not c[3]])
def test_norm_is_conserved_without_absorber(name, nch, nsteps, absorb):
    """No absorber, real f: sum_c N_c stays what it was.  The largest drift over the rows against the dense restatement's own on the
    same packet: at most 8 max(drift_ref, eps nsteps).  With more than one channel the field does move population: the first
    channel's norm changes by more than 1e-8."""
    d = _case(name, nch, nsteps, absorb)
    refs = _reference(name, nch, nsteps, absorb)
    _, _, obs = d["prob"].tdse_split(d["l"], d["c0"], DT, nsteps, f=d["f"], obs_every=1, **d["kw"])
    worst = 0.0
    for q in range(NSCAN):
        tot, tot_ref = obs[:, q].sum(-1), refs[q][1].sum(-1)
        drift, drift_ref = np.max(np.abs(tot - tot[0])), np.max(np.abs(tot_ref - tot_ref[0]))
        print("scan %d: norm %.15f  drift %.3e  restatement %.3e  population moved %.3e" % (q, tot[0], drift, drift_ref, abs(obs[-1, q, 0] - obs[0, q, 0])))
        worst = max(worst, drift / (8.0 * max(drift_ref, EPS * nsteps)))
        assert drift <= 8.0 * max(drift_ref, EPS * nsteps), (q, drift, drift_ref)
        if nch > 1:
            assert abs(obs[-1, q, 0] - obs[0, q, 0]) > 1e-8
        assert abs(host.spline_yield(obs)[-1, q] - (1.0 - tot[-1])) == 0.0
    note("tdse_split %s nch %d: max norm drift / bound = %.3g" % (name, nch, worst))


def test_twenty_nine_channels_beyond_every_other_call():
    """lin256 (k = 9) with 29 channels: the coupled matrix would have half-width 260, beyond bspatom_tdse_spline_wide's 255 --
    host.spline_propagate raises ValueError --; tdse_split runs three steps of two packets with info == 0 and meets the accuracy bound
    of test_accuracy_against_the_restatement (the restatement needs 256 x 256 solves alone)."""
    nch, nsteps, nscan = 29, 3, 2
    d = _case("lin256", nch, nsteps, False, nscan)
    assert nch * d["prob"].k - 1 == 260
    with pytest.raises(ValueError):
        host.spline_propagate(d["prob"], d["l"], d["c0"], DT, nsteps)
    assert np.all(d["info"] == 0) and np.all(np.isfinite(d["c"].view(np.float64))) and np.max(np.abs(d["c"] - d["c0"])) > 1e-3
    worst = _accuracy(d, _reference("lin256", nch, nsteps, False, nscan))
    note("tdse_split lin256 nch 29: max ||c - c_ref||_S / bound = %.3g" % worst)


def test_split_propagate_wraps_the_call():
    """host.split_propagate with split_angular's matrix and a real F_mid equals Problem.tdse_split with the same pieces, bit for bit"""
    prob = capi.Problem(capi.make_input(**coupled.HYD4))
    prob.assemble(0, 4)
    chans = [(0, 0), (1, 0), (2, 0), (3, 0)]
    ang = host.split_angular(chans)
    rng = np.random.default_rng(5)
    c0 = rng.standard_normal((4, prob.nfun)) / np.sqrt(prob.nfun)
    F = 0.1 * np.sin(0.5 * host.spline_midpoints(0.0, DT, 4))
    c, info, obs = host.split_propagate(prob, [0, 1, 2, 3], c0, DT, ang, F, obs_every=1)
    c2, info2, obs2 = prob.tdse_split([0, 1, 2, 3], c0, DT, 4, G=prob.dipole_bands()[0], Q=ang[0], lam=ang[1], f=F, obs_every=1)
    assert same(c, c2) and np.array_equal(info, info2) and same(obs, obs2) and np.all(info == 0) and obs.shape == (5, 1, 4)
    prob.close()


def test_tdse_split_argument_checks():
    prob = capi.Problem(single._input("n65_k4"))
    n, k, L = prob.nfun, prob.k, capi.lib()
    p_ = lambda x: x.ctypes.data_as(C.c_void_p)
    i32 = lambda v: np.array(v, dtype=np.int32)
    nch, nscan, nsteps = 2, 2, 2
    l, w = i32([0, 1]), i32([-1, 0])
    WB, GB = np.zeros((2 * k - 1) * n), np.ones((2 * k - 1) * n)
    Q, lam = np.array([[0.6, 0.8], [0.8, -0.6]]), np.array([-0.5, 0.5])
    f = np.array([0.1, 0.0] * (nsteps * nscan))
    c, P = np.ones(2 * nscan * nch * n), np.ones(2 * nch * n)
    snap, obs, info = np.zeros(2 * nscan * nch * n), np.zeros(3 * nscan * (nch + 2)), np.zeros(nscan, dtype=np.int32)
    dv = lambda v: torch.from_numpy(v).to("cuda:0")
    WBd, GBd, fd, cd, Pd, snapd, obsd = dv(WB), dv(GB), dv(f), dv(c), dv(P), dv(snap), dv(obs)
    dp = lambda t: C.c_void_p(t.data_ptr())
    variants = ((L.bspatom_tdse_split, p_(WB), p_(GB), p_(f), p_(c), p_(snap), p_(P), p_(obs)),
                (L.bspatom_tdse_split_dev, dp(WBd), dp(GBd), dp(fd), dp(cd), dp(snapd), dp(Pd), dp(obsd)))
    # 0 p, 1 nscan, 2 nch, 3 l, 4 nabs, 5 WB, 6 w, 7 G, 8 Q, 9 lam, 10 nsteps, 11 dt, 12 f, 13 c, 14 snap_every, 15 snap, 16 obs_every, 17 nproj,
    # 18 P, 19 obs, 20 info
    args = lambda wb, gb, fv, cv, sn, pp, ob: [prob._h, nscan, nch, p_(l), 1, wb, p_(w), gb, p_(Q), p_(lam), nsteps, 0.05, fv, cv, 2, sn, 1, 1, pp,
                                               ob, p_(info)]
    for fn, *ptrs in variants:                                 # before any solve or assemble: no channel is there
        assert fn(*args(*ptrs)) == -2
    prob.assemble(0, 2)
    for fn, *ptrs in variants:
        good = args(*ptrs)
        sub = lambda pos, v: [v if i == pos else g_ for i, g_ in enumerate(good)]
        both = lambda pa, va, pb, vb: [va if i == pa else (vb if i == pb else g_) for i, g_ in enumerate(good)]
        assert fn(*good) == 0
        for pos in (0, 3, 13, 20):                             # p, l, c, info
            assert fn(*sub(pos, None)) == -2, pos
        for pos in (1, 2):                                     # nscan, nch below 1
            assert fn(*sub(pos, 0)) == -2 and fn(*sub(pos, -1)) == -2, pos
        assert fn(*sub(10, -1)) == -2                          # nsteps < 0
        for bad in (0.0, -0.05, float("inf"), float("nan")):   # dt
            assert fn(*sub(11, bad)) == -2, bad
        for pos in (7, 8, 9, 12):                              # G, Q, lam, f NULL with steps
            assert fn(*sub(pos, None)) == -2, pos
            assert fn(*both(pos, None, 10, 0)) == 0, pos       # ... but not when there is no step
        assert fn(*[0 if i == 10 else (None if i in (7, 8, 9, 12) else g_) for i, g_ in enumerate(good)]) == 0
        assert fn(*sub(4, -1)) == -2 and fn(*sub(5, None)) == -2              # nabs < 0; nabs = 1 without WB
        for bad in ([0, 2], [-1, 0]):                          # a channel outside the bands held
            assert fn(*sub(3, p_(i32(bad)))) == -2, bad
        for bad in ([-2, 0], [-1, 1]):                         # w outside -1 .. nabs-1
            assert fn(*sub(6, p_(i32(bad)))) == -2, bad
        assert fn(*sub(6, None)) == 0                          # w NULL: absorber 0 everywhere
        assert fn(*sub(14, -1)) == -2 and fn(*sub(14, 0)) == -2               # snap_every < 0; snap given with snap_every = 0
        assert fn(*sub(15, None)) == 0 and fn(*both(14, 0, 15, None)) == 0     # no snapshots
        assert fn(*sub(16, -1)) == -2 and fn(*sub(16, 0)) == -2               # obs_every < 0; obs given with obs_every = 0
        assert fn(*sub(19, None)) == -2                        # obs_every >= 1 with obs NULL
        assert fn(*both(16, 0, 19, None)) == 0                 # no rows
        assert fn(*sub(17, -1)) == -2 and fn(*sub(18, None)) == -2            # nproj < 0; projections without P
        assert fn(*both(17, 0, 18, None)) == 0
        assert fn(*sub(10, 0)) == 0                            # nsteps = 0 measures
        assert fn(*good) == 0                                  # a valid call afterwards
    prob.close()
    # the limit k <= 16: k16_n40 runs (the cases above); a grid with k = 17 is refused with BSPATOM_ERR_UNSUPPORTED where its problem
    # is created (BSPATOM_MAX_K), so no handle with k > 16 reaches the call's own check of the one-wave window
    with pytest.raises(capi.BspAtomError) as ei:
        capi.Problem(capi.make_input(kind_grid=0, rb=100.0, k=17, nfun=64))
    assert ei.value.code == -5
