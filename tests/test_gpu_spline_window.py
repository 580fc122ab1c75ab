"""The window operator on spline packets (bspatom_spline_window / _dev, csrc/spline_window.hip): the guarantees W1 - W6 of
include/bspatom_spline_window.h bit for bit, every value against the spectral definition under the project's accuracy rule, a
superposition of two hydrogen states and a packet after a short pulse end to end, and the argument checks.  Fixtures come from
test_gpu_resolvent._input, in test_gpu_spline_expect's seeding style; the CPU side is tests/spline_window_ref.py."""
import ctypes as C
import functools
import numpy as np
import pytest
import torch                               # first: its HIP runtime is the one the process uses
from test_gpu_stages import note

import resolvent_ref as ref
import spline_window_ref as wref
import test_gpu_resolvent as single
from bspatom_amd import capi, host

pytestmark = pytest.mark.gpu
EPS = float(np.finfo(np.float64).eps)
same = single._same
DT = 0.05
NSCAN, NE = 5, 7
GAMMAS, ORDERS = (0.05, 0.002), (1, 2, 3)
COMBOS = [(g, m) for g in GAMMAS for m in ORDERS]
# (fixture, nch): n = 8 below the window width; one past a wave multiple; b = 8; b = 9, the BT = 15 instance part used; b = 15; a
# single channel.  l = c % 2: at nch = 4 an l has ten right-hand sides, blocks of 8 + 2 by default.
SHAPES = [("tiny8", 2), ("n65_k4", 3), ("lin256", 4), ("k10_n65", 3), ("k16_n40", 4), ("n65_k4", 1)]
IDS = ["%s-nch%d" % s for s in SHAPES]


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
def _case(name, nch):
    """The shared description of a case and its main runs, one per (gamma, m).  Energies: five from the lowest CPU eigenvalue of l = 0
    minus 0.1 to plus 2.0, one EQUAL to a CPU eigenvalue, one high in the spectrum.  Computed once, never changed."""
    prob = capi.Problem(single._input(name))
    SB, HB = prob.assemble(0, 2)
    n = prob.nfun
    rng = np.random.default_rng(400 + nch)
    l = [c % 2 for c in range(nch)]
    c0 = (rng.standard_normal((NSCAN, nch, n)) + 1j * rng.standard_normal((NSCAN, nch, n))) / np.sqrt(n)
    c0[0] = c0[0].real                                         # one real packet
    S = ref.upper_to_dense(SB)
    Hd = [ref.upper_to_dense(HB[lv]) for lv in (0, 1)]
    eig = [wref.eigen(H, S) for H in Hd]
    w0 = eig[0][0]
    E = np.concatenate([np.linspace(w0[0] - 0.1, w0[0] + 2.0, 5), [w0[min(2, n - 1)], w0[(3 * n) // 4]]])
    assert E.size == NE
    SF = host.band_symmetric(SB)
    z = {gm: host.window_shifts(E, *gm) for gm in COMBOS}
    runs = {gm: prob.spline_window(l, c0, z[gm]) for gm in COMBOS}
    for v in [c0, E, SF] + list(z.values()) + [r[0] for r in runs.values()] + [r[1] for r in runs.values()]:
        v.setflags(write=False)
    return dict(prob=prob, SB=SB, HB=HB, SF=SF, S=S, Hd=Hd, eig=eig, n=n, k=prob.k, nch=nch, l=l, c0=c0, E=E, z=z, runs=runs)


@functools.lru_cache(maxsize=None)
def _composition(name, nch, gamma, m):
    """W3's right-hand side: per l and energy the chain x_{j+1} = X of Problem.resolvent(l, z[e, j], B = band_apply(S, x_j)) over the
    packets with that l, and the norm rule in float64 NumPy on every x_j: Nref[j] (nscan, nch, ne) for j = 0 .. m stages"""
    d = _case(name, nch)
    prob, l, c0, z, SF = d["prob"], d["l"], d["c0"], d["z"][(gamma, m)], d["SF"]
    Nref = np.zeros((m + 1, NSCAN, nch, NE))
    for lv in sorted(set(l)):
        chans = [c for c in range(nch) if l[c] == lv]
        x0 = np.ascontiguousarray(c0[:, chans].reshape(-1, d["n"]))
        for e in range(NE):
            x = x0
            for j in range(m + 1):
                norms = np.array([wref.norm_f64(SF, v) for v in x]).reshape(NSCAN, len(chans))
                for i, c in enumerate(chans):
                    Nref[j, :, c, e] = norms[:, i]
                if j < m:
                    X, _, info = prob.resolvent(lv, z[e, j], host.band_apply(SF, x))
                    assert np.all(info == 0)
                    x = X[0]
    Nref.setflags(write=False)
    return Nref


@pytest.mark.parametrize("name,nch", SHAPES, ids=IDS)
def test_determinism_and_independence(name, nch):
    """W1, W2, W6 for every (gamma, m): a second run; every scan alone, every channel alone, every energy alone; resolvent_slots = 1
    and 2; window_rhs = 1 and 3; resolvent_stage_mb = 1; the _dev variant on a result pre-filled with NaN -- N bit for bit, info equal
    (0: Im z != 0).  Real shifts below the spectrum (any z is legal): info 0 again whatever window_rhs and nscan."""
    d = _case(name, nch)
    prob, l, c0 = d["prob"], d["l"], d["c0"]
    put = lambda v: torch.from_numpy(np.array(v)).to("cuda:0")
    cd = put(c0)
    for gm in COMBOS:
        z, (N, info) = d["z"][gm], d["runs"][gm]
        assert N.shape == (NSCAN, nch, NE) and np.all(np.isfinite(N)) and np.all(N > 0.0) and np.all(info == 0), gm
        check = lambda res, what: (same(res[0], N) and np.array_equal(res[1], info)) or pytest.fail("%s %s" % (gm, what))
        check(prob.spline_window(l, c0, z), "second run")
        for q in range(NSCAN):
            Nq, iq = prob.spline_window(l, c0[q], z)
            assert Nq.shape == (nch, NE) and same(Nq, N[q]) and np.array_equal(iq, info), (gm, "scan", q)
        for c in range(nch):
            Nc, ic = prob.spline_window(l[c:c + 1], c0[:, c:c + 1], z)
            assert same(Nc[:, 0], N[:, c]) and np.array_equal(ic, info), (gm, "channel", c)
        for e in range(NE):
            Ne_, ie = prob.spline_window(l, c0, z[e:e + 1])
            assert same(Ne_[..., 0], N[..., e]) and ie.shape == (1,) and ie[0] == info[e], (gm, "energy", e)
        for opts in (dict(resolvent_slots=1), dict(resolvent_slots=2), dict(window_rhs=1), dict(window_rhs=3), dict(resolvent_stage_mb=1)):
            with _Options(**opts):
                check(prob.spline_window(l, c0, z), opts)
        Nd = torch.full((NSCAN, nch, NE), float("nan"), dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        infod = prob.spline_window_dev(l, NSCAN, cd.data_ptr(), z, Nd.data_ptr())
        check((Nd.cpu().numpy(), infod), "_dev")
    zr = np.ascontiguousarray(np.stack([d["E"][:1] - 0.3, d["E"][:1] - 0.2], axis=1) + 0j)   # one energy, two real stages
    Nr, ir = prob.spline_window(l, c0, zr)
    assert np.all(np.isfinite(Nr)) and np.all(ir == 0)
    for opts, cc in ((dict(window_rhs=1), c0), (dict(window_rhs=3), c0), (dict(), c0[:1])):
        with _Options(**opts):
            N1, i1 = prob.spline_window(l, cc, zr)
        assert same(N1, Nr[:cc.shape[0]]) and np.array_equal(i1, ir), opts


@pytest.mark.parametrize("name,nch", SHAPES, ids=IDS)
def test_composition_truncation_and_plain_norm(name, nch):
    """W3: N equals the norm rule in float64 NumPy (spline_window_ref.norm_f64) on the x_m of the chain of Problem.resolvent calls
    with B = host.band_apply(host.band_symmetric(SB), x_j), for every (gamma, m), bit for bit.  W4: with the first m' < 3 shifts of
    the three-stage call the result is that chain's after m' stages.  W5: no shift at all gives, for every energy, the N_ch of the
    row of a tdse_split call with nsteps = 0 (and W3's norm rule on the packets themselves)."""
    d = _case(name, nch)
    prob, l, c0 = d["prob"], d["l"], d["c0"]
    for gm in COMBOS:
        assert same(d["runs"][gm][0], _composition(name, nch, *gm)[-1]), gm
    for gamma in GAMMAS:
        Nref = _composition(name, nch, gamma, 3)
        for mp in (1, 2):
            Np, ip = prob.spline_window(l, c0, d["z"][(gamma, 3)][:, :mp])
            assert same(Np, Nref[mp]) and np.all(ip == 0), (gamma, mp)
    N0, i0 = prob.spline_window(l, c0, np.zeros((NE, 0), dtype=np.complex128))
    rows = prob.tdse_split(l, c0, DT, 0, obs_every=1)[2]
    assert rows.shape == (1, NSCAN, nch) and np.all(i0 == 0)
    for e in range(NE):
        assert same(N0[..., e], rows[0]), e
    assert same(N0, _composition(name, nch, GAMMAS[0], 3)[0])


def _cpu_spectra(d, gamma, m):
    """gamma^(2m) N by the three float64 CPU evaluations, each (nscan, nch, ne): numpy.linalg.solve's chain, scipy's solve_banded chain
    (both on all packets of an l at once: one factorisation per stage, as on the GPU) and the eigh sum"""
    import scipy.linalg as sl
    n, nch, l, c0, S, b = d["n"], d["nch"], d["l"], d["c0"], d["S"], d["k"] - 1
    z = d["z"][(gamma, m)]
    out = np.zeros((3, NSCAN, nch, NE))
    for lv in sorted(set(l)):
        chans = [c for c in range(nch) if l[c] == lv]
        H = d["Hd"][lv]
        w, X = d["eig"][lv]
        x0 = c0[:, chans].reshape(-1, n).T                                  # (n, nrhs)
        a2 = np.abs(X.T @ (S @ x0)) ** 2                                    # (n states, nrhs)
        shape = (NSCAN, len(chans))
        for e in range(NE):
            xd, xb = x0, x0
            den = np.ones(n)
            for j in range(m):
                M = H - z[e, j] * S
                xd = np.linalg.solve(M, S @ xd)
                xb = sl.solve_banded((b, b), wref._band(M, b), S @ xb)
                den = den * np.abs(w - z[e, j]) ** 2
            three = (np.real(np.sum(np.conj(xd) * (S @ xd), axis=0)), np.real(np.sum(np.conj(xb) * (S @ xb), axis=0)), np.sum(a2 / den[:, None], axis=0))
            for v, vals in enumerate(three):
                for i, c in enumerate(chans):
                    out[v, :, c, e] = vals.reshape(shape)[:, i]
    return gamma ** (2 * m) * out


@pytest.mark.parametrize("name,nch", SHAPES, ids=IDS)
def test_accuracy_against_the_spectral_definition(name, nch):
    """|gamma^(2m) N - P_spec| <= 8 max(delta_ref, eps n max_e P_spec) for every packet (q, c), energy, gamma = 0.05 and 0.002 and
    m = 1, 2, 3: P_spec the sum over scipy.linalg.eigh's pairs of |x_n^T S c|^2 gamma^(2m) / ((E_n - E)^(2m) + gamma^(2m)); delta_ref
    the largest pairwise difference, over the packet's energies, of three float64 CPU evaluations -- numpy.linalg.solve's chain,
    scipy.linalg.solve_banded's chain and that sum: the project's accuracy rule, the reference's own noise times 8.  One energy is a
    CPU eigenvalue, where the window is 1 for that state and the stage matrices are gamma away from singular.  The worst ratio
    of the deviation to the bound per shape is printed and noted.  Measured on the MI355X, worst ratio per shape: tiny8 nch 2: 0.206,
    n65_k4 nch 3: 0.163, lin256 nch 4: 0.285, k10_n65 nch 3: 0.139, k16_n40 nch 4: 0.273, n65_k4 nch 1: 0.16 (delta_ref between 1e-15 and
    4e-14, on k16_n40 up to 9e-10: there the three CPU evaluations themselves disagree that much)."""
    d = _case(name, nch)
    n = d["n"]
    worst = 0.0
    for gm in COMBOS:
        gamma, m = gm
        P = gamma ** (2 * m) * d["runs"][gm][0]
        Pd, Pb, Ps = _cpu_spectra(d, gamma, m)
        dref = np.max(np.maximum(np.maximum(np.abs(Pd - Pb), np.abs(Pd - Ps)), np.abs(Pb - Ps)), axis=-1)     # (nscan, nch)
        bound = 8.0 * np.maximum(dref, EPS * n * np.max(Ps, axis=-1))
        ratio = float(np.max(np.max(np.abs(P - Ps), axis=-1) / bound))
        print("%s nch %d gamma %g m %d: worst |P - P_spec| / bound %.3g (largest delta_ref %.3e, largest P %.3e)"
              % (name, nch, gamma, m, ratio, np.max(dref), np.max(Ps)))
        worst = max(worst, ratio)
    note("spline_window %s nch %d: max |gamma^2m N - P_spec| / (8 max(delta_ref, eps n max P)) = %.3g" % (name, nch, worst))
    assert worst <= 1.0, worst


# ---- hydrogen, the beat test's grid ---------------------------------------------------------------------------------------------
def _hydrogen():
    prob = capi.Problem(capi.make_input(**single.HYD))
    E, sinfo = prob.solve(0, 2)
    assert np.all(sinfo == 0)
    V = prob.eigvecs_batch(0, 2, 1, 1)[:, 0]
    SB, HB = prob.assemble(0, 2)
    return prob, E, V, SB, HB


def test_two_state_superposition():
    """c = (a_s x_1s, a_p x_2p) in the channels l = 0, 1, |a_s|^2 = 0.7, |a_p|^2 = 0.3 with a phase: summed over the channels, the
    window at the box eigenvalue E_1s gives |a_s|^2 plus the 2p peak's leak |a_p|^2 gamma^(2m) / ((E_2p - E_1s)^(2m) + gamma^(2m)),
    and at E_2p the other way round, for gamma = 0.05 and 0.002, m = 1, 2, 3, by the accuracy rule of the shapes' test: within
    8 max(delta_ref, eps n max P), delta_ref from the three CPU evaluations on the same packet.  Measured on the MI355X: worst ratio 0.151
    (gamma = 0.002, m = 3: deviation 2.7e-14 of a bound 1.8e-13)."""
    prob, E, V, SB, HB = _hydrogen()
    n = prob.nfun
    amp = np.array([np.sqrt(0.7), np.sqrt(0.3) * np.exp(0.4j)])
    c = np.stack([amp[0] * V[0], amp[1] * V[1]]).astype(np.complex128)
    En = np.array([E[0, 0], E[1, 0]])
    S = ref.upper_to_dense(SB)
    d = dict(n=n, nch=2, l=[0, 1], k=prob.k, S=S, Hd=[ref.upper_to_dense(HB[lv]) for lv in (0, 1)], c0=np.tile(c, (NSCAN, 1, 1)))
    d["eig"] = [wref.eigen(H, S) for H in d["Hd"]]
    Epad = np.concatenate([En, np.linspace(-0.6, 0.2, NE - 2)])             # the two peaks, then five more energies (_cpu_spectra's ne)
    worst = 0.0
    for gamma, m in COMBOS:
        z = host.window_shifts(Epad, gamma, m)
        d["z"] = {(gamma, m): z}
        P = host.window_spectrum(prob, [0, 1], c, Epad, gamma, m)
        assert P.shape == (2, NE)
        g = gamma ** (2 * m) / ((En[1] - En[0]) ** (2 * m) + gamma ** (2 * m))
        closed = np.array([0.7 + 0.3 * g, 0.3 + 0.7 * g])
        Pd, Pb, Ps = (v[0].sum(axis=0) for v in _cpu_spectra(d, gamma, m))  # summed over the channels: (ne,)
        dref = float(np.max(np.maximum(np.maximum(np.abs(Pd - Pb), np.abs(Pd - Ps)), np.abs(Pb - Ps))))
        bound = 8.0 * max(dref, EPS * n * float(np.max(Ps)))
        dev = float(np.max(np.abs(P.sum(axis=0)[:2] - closed)))
        print("gamma %g m %d: P(E_1s), P(E_2p) = %s, closed form %s, deviation %.3e, bound %.3e" % (gamma, m, P.sum(axis=0)[:2], closed, dev, bound))
        worst = max(worst, dev / bound)
    note("spline_window 1s + 2p: max |P - (|a_n|^2 + leak)| / bound = %.3g" % worst)
    assert worst <= 1.0, worst
    prob.close()


def test_spectrum_after_a_pulse_integrates_to_the_norm():
    """Hydrogen 1s through a short pulse (F0 = 0.1, omega = 0.6, sin^2 envelope, T = 10, dt = 0.05, channels l = 0, 1, no absorber: the
    box of 40 a.u. still holds the packet), then the window of order 2 and width gamma = 0.25 on the grid h = gamma / 4 from E_min - D to
    E_max + D, D = 40 gamma, which contains E = 0: the trapezoid integral of the summed density gives sum_c N_c of the run's last row,
    and window_yield above 0 plus the trapezoid integral up to 0 gives the same.  Tolerance, relative: the tail, end-point and
    trapezoid terms derived in tests/test_spline_window_cpu.py::test_density_integrates_to_the_norm (4.9e-6 together) plus the solves'
    rounding as in test_solve_chain_equals_the_spectral_sum there, 2 m n eps kappa(S) (spread + gamma) / gamma (1.3e-6)."""
    prob, E, V, SB, HB = _hydrogen()
    n, chans = prob.nfun, [(0, 0), (1, 0)]
    dt, T, F0, om = 0.05, 10.0, 0.1, 0.6
    ns = int(round(T / dt))
    t = host.spline_midpoints(0.0, dt, ns)
    F = F0 * np.sin(np.pi * t / T) ** 2 * np.cos(om * t)
    c, info, obs = host.split_propagate(prob, [0, 1], host.spline_packet(prob, chans, 0, V[0]), dt, host.split_angular(chans), F, obs_every=ns)
    assert np.all(info == 0)
    norms = obs[-1, 0, :2]
    assert norms[1] > 1e-4 and abs(norms.sum() - 1.0) < 1e-7                # the pulse moved population; Crank-Nicolson keeps the norm
    S = ref.upper_to_dense(SB)
    w = [wref.eigen(ref.upper_to_dense(HB[lv]), S)[0] for lv in (0, 1)]
    lo, hi = min(v[0] for v in w), max(v[-1] for v in w)
    gamma, m = 0.25, 2
    D, h = 40 * gamma, gamma / 4
    grid = h * np.arange(int(np.floor((lo - D) / h)), int(np.ceil((hi + D) / h)) + 1)
    i0 = int(np.flatnonzero(grid == 0.0)[0])
    P = host.window_spectrum(prob, [0, 1], c, grid, gamma, m)
    assert P.shape == (2, grid.size) and np.all(P > 0.0)
    dens = host.window_density(P, gamma, m)
    trap = lambda v, a, b: float(np.sum(0.5 * (v[a + 1:b] + v[a:b - 1]) * h))
    Im = wref.window_integral(m)
    q = np.exp(-8 * np.pi * np.sin(np.pi / (2 * m)))
    tol = ((2.0 / (2 * m - 1)) * (gamma / D) ** (2 * m - 1) / Im + 0.25 * (gamma / D) ** (2 * m) / Im + 2 * np.pi * q / ((1 - q) * Im)
           + 2 * m * n * EPS * np.linalg.cond(S) * (hi - lo + 2 * D + gamma) / gamma)
    total = sum(trap(dens[ch], 0, grid.size) for ch in range(2))
    above = host.window_yield(P, grid, gamma, m)
    split = float(above.sum()) + sum(trap(dens[ch], 0, i0 + 1) for ch in range(2))
    print("pulse: sum_c N_c %.12f, integral of the density %.12f (relative deviation %.3e), yield above 0 %.6e + below, deviation %.3e, "
          "tolerance %.3e, %d energies" % (norms.sum(), total, total / norms.sum() - 1, above.sum(), split / norms.sum() - 1, tol, grid.size))
    note("spline_window pulse: integral / norm - 1 = %.3e (tolerance %.3e), yield above 0 = %.6e" % (total / norms.sum() - 1, tol, above.sum()))
    assert abs(total - norms.sum()) <= tol * norms.sum() and abs(split - norms.sum()) <= tol * norms.sum()
    assert 0.0 < above.sum() < norms.sum()
    prob.close()


def test_argument_checks():
    prob = capi.Problem(single._input("n65_k4"))
    n, L = prob.nfun, capi.lib()
    p_ = lambda x: x.ctypes.data_as(C.c_void_p)
    dv = lambda v: torch.from_numpy(v).to("cuda:0")
    dp = lambda t: C.c_void_p(t.data_ptr())
    nscan, nch, ne, nfac = 2, 2, 3, 2
    l = np.array([0, 1], dtype=np.int32)
    z = np.ascontiguousarray(host.window_shifts([0.1, 0.2, 0.3], 0.05, nfac)).view(np.float64)
    c, N, info = np.ones(2 * nscan * nch * n), np.zeros(nscan * nch * ne), np.zeros(ne, dtype=np.int32)
    cd, Nd = dv(c), dv(N)
    # 0 p, 1 nscan, 2 nch, 3 l, 4 ne, 5 nfac, 6 z, 7 c, 8 N, 9 info
    variants = ((L.bspatom_spline_window, p_(c), p_(N)), (L.bspatom_spline_window_dev, dp(cd), dp(Nd)))
    for fn, cc, nn in variants:                                  # before any solve or assemble: no channel is there
        assert fn(prob._h, nscan, nch, p_(l), ne, nfac, p_(z), cc, nn, p_(info)) == -2
    prob.assemble(0, 2)
    for fn, cc, nn in variants:
        good = [prob._h, nscan, nch, p_(l), ne, nfac, p_(z), cc, nn, p_(info)]
        sub = lambda pos, v: [v if i == pos else g_ for i, g_ in enumerate(good)]
        assert fn(*good) == 0
        for pos in (0, 3, 6, 7, 8, 9):                             # p, l, z (nfac > 0), c, N, info
            assert fn(*sub(pos, None)) == -2, pos
        for pos in (1, 2, 4):                                      # nscan, nch, ne below 1
            assert fn(*sub(pos, 0)) == -2 and fn(*sub(pos, -1)) == -2, pos
        assert fn(*sub(5, -1)) == -2 and fn(*sub(5, capi.WINDOW_MAX_FAC + 1)) == -2
        for bad in ([0, 2], [-1, 0]):                              # a channel outside the bands
            assert fn(*sub(3, p_(np.array(bad, dtype=np.int32)))) == -2, bad
        assert fn(*[0 if i == 5 else (None if i == 6 else g_) for i, g_ in enumerate(good)]) == 0      # nfac = 0 reads no z
        assert fn(*good) == 0
    torch.cuda.synchronize()
    assert np.array_equal(Nd.cpu().numpy(), N) and np.all(N > 0.0) and np.all(info == 0)
    z8 = host.window_shifts([0.1], 0.05, capi.WINDOW_MAX_FAC)     # the largest window is a valid call
    N8, i8 = prob.spline_window([0, 1], np.ones((2, n)), z8)
    assert N8.shape == (2, 1) and np.all(np.isfinite(N8)) and np.all(N8 > 0.0) and np.all(i8 == 0)
    prob.close()
