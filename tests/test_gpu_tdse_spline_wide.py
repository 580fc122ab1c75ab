"""The TDSE in the spline basis for wide bands (bspatom_tdse_spline_wide / _dev, csrc/tdse_spline_wide.hip): test_gpu_tdse_spline.py's
checks on the blocked LU -- the guarantees S1 - S5 bit for bit, above all the composition S3: a step IS host.band_apply,
Problem.resolvent_coupled_wide at z = 2i/dt and two NumPy operations --, the rows against a long-double evaluation on the run's own
snapshots, the narrow and the wide call against the dense restatement where both apply, the norm under a Hermitian coupling,
host.spline_propagate's choice, and the argument checks.  Shapes, the launch rule and the norm system: tests/tdse_spline_wide_ref.py;
the dense reference is tests/tdse_spline_ref.py; fixtures, topology and coefficients are test_gpu_resolvent_wide's."""
import ctypes as C
import functools
import numpy as np
import pytest
import torch                               # first: its HIP runtime is the one the process uses
from test_gpu_stages import note

import resolvent_ref as ref
import tdse_spline_ref as sref
import tdse_spline_wide_ref as wref
import test_gpu_resolvent as single
import test_gpu_resolvent_wide as wide
from test_gpu_tdse_spline import _Options
from bspatom_amd import capi, host

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
same = single._same
DT = wref.DT
NSCAN, SLOTS, GROUP, OBS_EVERY, SNAP_EVERY = wref.NSCAN, 2, 3, 2, 3
# bw = 11 < a panel; bw = 67 just past the old limit; N = 100 < 2 bw + 1 = 159; bw = 143: candidates over three waves; the limit bw = 255
SHAPES = [s[:3] for s in wref.SHAPES]
CASES = [(name, nch, nsteps, absorb) for name, nch, nsteps in SHAPES for absorb in (False, True)]
IDS = ["%s-nch%d-%s" % (c[0], c[1], "cap" if c[3] else "nocap") for c in CASES]
S45 = [c for c in CASES if c[:2] in (("n65_k4", 17), ("k16_n40", 9))]
S45_IDS = [i for c, i in zip(CASES, IDS) if c in S45]


@functools.lru_cache(maxsize=None)
def _grid(name):
    """test_gpu_resolvent_wide._assembled, once per fixture; the bands are never changed"""
    got = wide._assembled(name)
    for v in got[1:]:
        v.setflags(write=False)
    return got


@functools.lru_cache(maxsize=None)
def _case(name, nch, nsteps, absorb):
    """The shared description of a case and its main run (resolvent_slots = 2: a slot takes several of the five scans;
    tdse_spline_group = 3, obs_every = 2, snap_every = 3).  Computed once, never changed."""
    prob, SB, HB, WB, G = _grid(name)
    n = prob.nfun
    assert (name, nch, nsteps, prob.k, n) in wref.SHAPES
    rng = np.random.default_rng(200 + nch)
    l = [c % 2 for c in range(nch)]
    cp = wide._topology(nch)
    # test_gpu_resolvent_wide's complex coefficients at strength 0.3 (the long-range entry among them), times a real pulse value
    F = rng.uniform(0.2, 1.0, (nsteps, NSCAN))
    coef = np.ascontiguousarray(F[:, :, None, None] * wide._coefficients(nch, 0.3)[None, None])
    c0 = (rng.standard_normal((NSCAN, nch, n)) + 1j * rng.standard_normal((NSCAN, nch, n))) / np.sqrt(n)
    c0[0] = c0[0].real                                         # one real packet
    P = rng.standard_normal((2, nch, n)) + 1j * rng.standard_normal((2, nch, n))
    kw = dict(couplings=cp, G=G, W=WB if absorb else None, w=([0] + [-1] * (nch - 1)) if absorb else None)
    with _Options(resolvent_slots=SLOTS, tdse_spline_group=GROUP):
        c, info, obs, snaps = prob.tdse_spline_wide(l, c0, DT, nsteps, coef=coef, P=P, obs_every=OBS_EVERY, snap_every=SNAP_EVERY, **kw)
    for v in (c0, coef, P, c, info, obs, snaps):
        v.setflags(write=False)
    return dict(prob=prob, SB=SB, HB=HB, WB=WB, G=G, n=n, nch=nch, nsteps=nsteps, l=l, cp=cp, coef=coef, c0=c0, P=P, kw=kw, c=c, info=info,
                obs=obs, snaps=snaps)


@pytest.mark.parametrize("name,nch,nsteps,absorb", CASES, ids=IDS)
def test_determinism_and_independence(name, nch, nsteps, absorb):
    """S1 and S2 bitwise: the main run against a second run; every scan alone; the default work slots and one slot; launches of one
    step and of the default length (the launch rule's: the whole run in one launch); tdse_stage_mb = 1; obs_every = 1 and 0,
    snap_every = 1 and 0, no projections and one; the _dev variant on torch tensors pre-filled with NaN."""
    d = _case(name, nch, nsteps, absorb)
    prob, l, c0, coef, P, kw = d["prob"], d["l"], d["c0"], d["coef"], d["P"], d["kw"]
    n = d["n"]
    assert wref.launch_group(nch * n, nch * prob.k - 1, NSCAN, NSCAN) >= nsteps > 1
    assert np.all(d["info"] == 0) and np.all(np.isfinite(d["c"].view(np.float64))) and np.max(np.abs(d["c"] - c0)) > 1e-3
    assert d["snaps"].shape == (nsteps // SNAP_EVERY, NSCAN, nch, n) and d["obs"].shape == (capi.Problem.tdse_nobs(nsteps, OBS_EVERY), NSCAN, nch + 4)
    run = lambda **over: prob.tdse_spline_wide(l, c0, DT, nsteps, **{**dict(coef=coef, P=P, obs_every=OBS_EVERY, snap_every=SNAP_EVERY), **kw, **over})
    def check(res, what):
        assert same(res[0], d["c"]) and np.array_equal(res[1], d["info"]) and same(res[2], d["obs"]) and same(res[3], d["snaps"]), what
    check(run(), "second run: default slots, default launch length")
    for opts in (dict(resolvent_slots=1), dict(tdse_spline_group=1), dict(resolvent_slots=SLOTS), dict(tdse_spline_group=GROUP, tdse_stage_mb=1),
                 dict(tdse_stage_mb=1)):
        with _Options(**opts):
            check(run(), opts)
    for q in range(NSCAN):                                     # each scan alone
        cq, iq, oq, sq = prob.tdse_spline_wide(l, c0[q], DT, nsteps, coef=coef[:, q:q + 1], P=P, obs_every=OBS_EVERY, snap_every=SNAP_EVERY, **kw)
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
    infod = prob.tdse_spline_wide_dev(l, NSCAN, nsteps, DT, cd.data_ptr(), couplings=d["cp"], nop=2, G_ptr=Gd.data_ptr(), coef_ptr=coefd.data_ptr(),
                                      nabs=1 if absorb else 0, W_ptr=Wd.data_ptr() if absorb else None, w=kw["w"], nproj=2, P_ptr=Pd.data_ptr(),
                                      obs_every=OBS_EVERY, obs_ptr=od.data_ptr(), snap_every=SNAP_EVERY, snap_ptr=sd.data_ptr())
    check((cd.cpu().numpy(), infod, od.cpu().numpy(), sd.cpu().numpy()), "_dev")


@pytest.mark.parametrize("name,nch,nsteps,absorb", CASES, ids=IDS)
def test_step_is_band_apply_wide_solve_update(name, nch, nsteps, absorb):
    """S3, the composition, bit for bit over the whole run: b = host.band_apply on the symmetric full band of Problem.assemble's SB (Re
    and Im apart), Problem.resolvent_coupled_wide(l, 2j/dt, B = b, a = coef[n, q]), then c' = (g x_im - c_re, -(g x_re) - c_im) with
    g = 4.0/dt in NumPy: the replay reproduces c, every snapshot and info."""
    d = _case(name, nch, nsteps, absorb)
    prob, l, kw = d["prob"], d["l"], d["kw"]
    SBf = host.band_symmetric(d["SB"])
    g, z = 4.0 / DT, complex(0.0, 2.0 / DT)
    c = np.array(d["c0"])
    info = np.zeros(NSCAN, dtype=np.int64)
    for n in range(nsteps):
        for q in range(NSCAN):
            b = host.band_apply(SBf, c[q].real) + 1j * host.band_apply(SBf, c[q].imag)
            X, _, inf = prob.resolvent_coupled_wide(l, z, b, a=d["coef"][n, q], **kw)
            x = X[0, 0]
            c[q] = (g * x.imag - c[q].real) + 1j * (-(g * x.real) - c[q].imag)
            info[q] += inf[0]
        if (n + 1) % SNAP_EVERY == 0:
            assert same(c, d["snaps"][(n + 1) // SNAP_EVERY - 1]), n
    assert same(c, d["c"]) and np.array_equal(info, d["info"])


@pytest.mark.parametrize("name,nch,nsteps,absorb", S45, ids=S45_IDS)
def test_snapshot_is_the_shorter_run_and_continues(name, nch, nsteps, absorb):
    """S4 at bw = 67 and bw = 143: the main run's snapshot after step 3 equals the run of 3 steps, and the steps left from it give the
    long run's c; the same with the split after step 1 (a snapshot of a run with snap_every = 1), which leaves steps at bw = 143 too."""
    d = _case(name, nch, nsteps, absorb)
    prob, l, coef, kw = d["prob"], d["l"], d["coef"], d["kw"]
    cs, _ = prob.tdse_spline_wide(l, d["c0"], DT, SNAP_EVERY, coef=coef[:SNAP_EVERY], **kw)
    assert same(cs, d["snaps"][0])
    cl, _ = prob.tdse_spline_wide(l, d["snaps"][0], DT, nsteps - SNAP_EVERY, coef=coef[SNAP_EVERY:], **kw)
    assert same(cl, d["c"])
    _, _, s1 = prob.tdse_spline_wide(l, d["c0"], DT, nsteps, coef=coef, snap_every=1, **kw)
    c1, _ = prob.tdse_spline_wide(l, d["c0"], DT, 1, coef=coef[:1], **kw)
    assert same(c1, s1[0]) and same(s1[SNAP_EVERY - 1], d["snaps"][0])
    cl, _ = prob.tdse_spline_wide(l, s1[0], DT, nsteps - 1, coef=coef[1:], **kw)
    assert same(cl, d["c"])


@pytest.mark.parametrize("name,nch,nsteps,absorb", S45, ids=S45_IDS)
def test_last_row_is_the_measuring_call(name, nch, nsteps, absorb):
    """S5 at bw = 67 and bw = 143: the last row has the bits of a call with nsteps = 0 on the returned c, which leaves c alone"""
    d = _case(name, nch, nsteps, absorb)
    c0, i0, o0 = d["prob"].tdse_spline_wide(d["l"], d["c"], DT, 0, P=d["P"], obs_every=1, **d["kw"])
    assert same(c0, d["c"]) and np.all(i0 == 0) and o0.shape == (1, NSCAN, nch + 4) and same(o0[0], d["obs"][-1])
    _, _, o1 = d["prob"].tdse_spline_wide(d["l"], d["c"], DT, 0, P=d["P"], obs_every=OBS_EVERY, couplings=d["cp"], G=d["G"])
    assert same(o1[0], d["obs"][-1])                           # ... whatever the description says about couplings and the absorber


@pytest.mark.parametrize("name,nch,nsteps,absorb", CASES, ids=IDS)
def test_rows_against_long_double_on_the_snapshots(name, nch, nsteps, absorb):
    """With every step observed and kept, N_c and the projections of row j against a clongdouble evaluation of Re c^H S c and
    sum P (S c) on the packet the run itself returned for that step, within (nch nfun + 2) eps sum |terms| -- test_gpu_tdse_spline's
    bound --, and against tdse_spline_ref.row within the same bound."""
    d = _case(name, nch, nsteps, absorb)
    prob, l, P, kw, n = d["prob"], d["l"], d["P"], d["kw"], d["n"]
    c, _, obs, snaps = prob.tdse_spline_wide(l, d["c0"], DT, nsteps, coef=d["coef"], P=P, obs_every=1, snap_every=1, **kw)
    assert obs.shape == (nsteps + 1, NSCAN, nch + 4) and same(c, d["c"])
    Sl = np.asarray(ref.upper_to_dense(d["SB"]), dtype=np.longdouble)
    absS = np.abs(ref.upper_to_dense(d["SB"]))
    packets = np.concatenate([d["c0"][None], snaps])
    worst = 0.0
    for j in range(nsteps + 1):
        for q in range(NSCAN):
            cl = packets[j, q].astype(np.clongdouble)
            bl = cl @ Sl.T                                     # (nch, n): S c per channel
            row = sref.row(d["SB"], packets[j, q], P)
            for ch in range(nch):
                bound = (nch * n + 2) * EPS * float(np.abs(packets[j, q, ch]) @ absS @ np.abs(packets[j, q, ch]))
                err = abs(float(np.sum(np.conj(cl[ch]) * bl[ch]).real) - obs[j, q, ch])
                worst = max(worst, err / bound)
                assert err <= bound and abs(row[ch] - obs[j, q, ch]) <= bound, (j, q, ch, err, bound)
            for r in range(2):
                pl = P[r].astype(np.clongdouble)
                bound = (nch * n + 2) * EPS * float(sum(np.abs(P[r, ch]) @ absS @ np.abs(packets[j, q, ch]) for ch in range(nch)))
                got = complex(obs[j, q, nch + 2 * r], obs[j, q, nch + 2 * r + 1])
                err = abs(complex(np.sum(pl * bl)) - got)
                worst = max(worst, err / bound)
                assert err <= bound and abs(complex(row[nch + 2 * r], row[nch + 2 * r + 1]) - got) <= bound, (j, q, r, err, bound)
    print("%s nch %d: worst row error / bound %.3g" % (name, nch, worst))


def test_narrow_and_wide_against_the_dense_restatement():
    """Where both calls apply -- lin256, nch = 4 (bw = 35), 7 steps, the absorber on channel 0, a real and a complex packet -- they are
    not promised bit-equal; each against tdse_spline_ref.propagate (dense, float64, numpy.linalg.solve):
    max |c_wide - c_dense| <= 8 max(max |c_narrow - c_dense|, eps max |c|), 8 the factor the resolvent tests give a kernel over LAPACK."""
    prob, SB, HB, WB, G = _grid("lin256")
    n, nch, nsteps, nscan = prob.nfun, 4, 7, 2
    assert nch * prob.k - 1 == 35
    rng = np.random.default_rng(35)
    l, cp = [c % 2 for c in range(nch)], wide._topology(nch)
    F = rng.uniform(0.2, 1.0, (nsteps, nscan))
    coef = np.ascontiguousarray(F[:, :, None, None] * wide._coefficients(nch, 0.3)[None, None])
    c0 = (rng.standard_normal((nscan, nch, n)) + 1j * rng.standard_normal((nscan, nch, n))) / np.sqrt(n)
    c0[0] = c0[0].real
    w = [0] + [-1] * (nch - 1)
    cn, i_n = prob.tdse_spline(l, c0, DT, nsteps, couplings=cp, G=G, coef=coef, W=WB, w=w)
    cw, i_w = prob.tdse_spline_wide(l, c0, DT, nsteps, couplings=cp, G=G, coef=coef, W=WB, w=w)
    assert np.all(i_n == 0) and np.all(i_w == 0)
    for q in range(nscan):
        cd, _, _ = sref.propagate(SB, HB, l, DT, c0[q], coef[:, q], cp, G, WB[None], w)
        dn, dw, scale = np.max(np.abs(cn[q] - cd)), np.max(np.abs(cw[q] - cd)), np.max(np.abs(cd))
        note("tdse_spline narrow / wide against dense, lin256 nch 4 packet %d: max |c - c_dense| = %.3e (narrow) %.3e (wide), max |c| %.3g, "
             "narrow == wide: %s" % (q, dn, dw, scale, same(cn[q], cw[q])))
        assert dw <= 8.0 * max(dn, EPS * scale), (q, dn, dw)


def test_norm_is_conserved_without_absorber():
    """n65_k4, nch = 17 (bw = 67), tdse_spline_wide_ref's Hermitian system (every neighbour pair in both directions on r and d/dr, the
    second entries transposed with conjugate coefficients), no absorber, 5 steps, every step observed: the largest deviation of
    sum_ch N_ch from its start is at most 8 times the dense restatement's on the same bands and packet, floored at 8 eps -- the
    bound test_tdse_spline_wide_cpu derives and checks on the dense side."""
    prob, SB, HB, WB, G = _grid("n65_k4")
    l, cp, coef = wref.hermitian_system()
    c0 = wref.norm_packet(prob.nfun)
    c, info, obs = prob.tdse_spline_wide(l, c0, DT, wref.NORM_STEPS, couplings=cp, G=G, coef=coef, obs_every=1)
    assert np.all(info == 0) and obs.shape == (wref.NORM_STEPS + 1, 1, wref.NORM_NCH)
    drift, tot = wref.norm_drift(obs[:, 0])
    drift_ref, tot_ref = wref.norm_drift_dense(SB, HB, G)
    moved = np.max(np.abs(obs[-1, 0] - obs[0, 0]))
    note("tdse_spline_wide norm, n65_k4 nch 17: norm %.15f  drift %.3e (%.2f eps)  dense restatement %.3e  population moved %.3e"
         % (tot, drift, drift / EPS, drift_ref, moved))
    assert moved > 1e-4 and abs(tot - tot_ref) <= 16 * EPS * tot_ref
    assert drift <= max(8.0 * drift_ref, 8.0 * EPS), (drift, drift_ref)
    assert abs(host.spline_yield(obs)[-1, 0] - (1.0 - obs[-1, 0].sum())) == 0.0


def test_spline_propagate_takes_the_narrow_and_the_wide_entry(monkeypatch):
    """lin256 (k = 9): seven channels (bw = 62) go to bspatom_tdse_spline and have its bits; eight (bw = 71) go to
    bspatom_tdse_spline_wide, which the narrow call refuses"""
    prob = capi.Problem(single._input("lin256"))
    prob.assemble(0, 2)
    n = prob.nfun
    calls = []
    for name in ("tdse_spline", "tdse_spline_wide"):
        inner = getattr(prob, name)
        monkeypatch.setattr(prob, name, lambda *a, _i=inner, _n=name, **kw: (calls.append(_n), _i(*a, **kw))[1])
    rng = np.random.default_rng(9)
    for nch, want in ((7, "tdse_spline"), (8, "tdse_spline_wide")):
        l = [c % 2 for c in range(nch)]
        c0 = rng.standard_normal((nch, n)) + 1j * rng.standard_normal((nch, n))
        del calls[:]
        c, info, obs = host.spline_propagate(prob, l, c0, DT, 2, obs_every=1)
        assert calls == [want] and info[0] == 0 and obs.shape == (3, 1, nch)
        c_, _, obs_ = getattr(capi.Problem, want)(prob, l, c0, DT, 2, obs_every=1)
        assert same(c, c_) and same(obs, obs_)
    with pytest.raises(capi.BspAtomError) as ei:
        capi.Problem.tdse_spline(prob, l, c0, DT, 1)
    assert ei.value.code == -5
    with pytest.raises(ValueError):
        host.spline_propagate(prob, [0] * 29, np.ones((29, n)), DT, 1)
    prob.close()


def test_tdse_spline_wide_argument_checks():
    """test_tdse_spline_argument_checks' list on both wide variants; nch = 64 on n65_k4 (bw = 255) is accepted, nch = 65 is
    BSPATOM_ERR_UNSUPPORTED"""
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
    variants = ((L.bspatom_tdse_spline_wide, p_(WB), p_(GB), p_(coef), p_(c), p_(snap), p_(P), p_(obs)),
                (L.bspatom_tdse_spline_wide_dev, dp(WBd), dp(GBd), dp(coefd), dp(cd), dp(snapd), dp(Pd), dp(obsd)))
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
    # the limit on the same grid (k = 4): 64 channels are bw = 255 and run, 65 are bw = 259
    c64, info64 = prob.tdse_spline_wide([c % 2 for c in range(64)], np.ones((64, n)), DT, 1)
    assert info64[0] == 0 and np.all(np.isfinite(c64.view(np.float64))) and np.max(np.abs(c64 - 1.0)) > 1e-3
    for call in (prob.tdse_spline_wide, prob.tdse_spline):
        with pytest.raises(capi.BspAtomError) as ei:
            call([c % 2 for c in range(65)], np.ones((65, n)), DT, 1)
        assert ei.value.code == -5
    prob.close()
