"""The split-step TDSE's own one-wave banded LU (csrc/tdse_split.hip: sp_factor, sp_solve, and rs_forward as that file calls it) where
the physical matrices of test_gpu_tdse_split.py never take it: pivots at distance b in the atomic and in the field matrices, rows of
U that are 2 b wide, field matrices with exactly zero columns, and b = 9 in the instances compiled for b <= 15.  The matrices are
those of tests/pivot_designs.py (split_system), given to bspatom_tdse_split through its public arguments at dt = 2^-11;
test_tdse_split_pivots_cpu.py proves on the CPU that they pivot and fill as designed and that a banded LU with a cut pivot search or
dropped fill misses the criterion used here on every designed case.  Criterion, reference and helpers are test_gpu_tdse_split's own
(_accuracy, tests/tdse_split_ref.py); problems and bands are test_gpu_resolvent_pivots._assembled's, shared with that file."""
import functools
import numpy as np
import pytest
import torch                               # first: its HIP runtime is the one the process uses
from test_gpu_stages import note

import pivot_designs as pd
import tdse_split_ref as pref
import test_gpu_resolvent_pivots as pivots  # its problems and bands, assembled once per grid
import test_gpu_tdse_split as split        # its criterion (_accuracy), its option setter and its bit comparison

pytestmark = pytest.mark.gpu
same = split.same
DT, NSTEPS, NSCAN = pd.SPLIT_DT, pd.SPLIT_NSTEPS, pd.SPLIT_NSCAN
CASES = [(name, variant) for name in pd.SPLIT_GRIDS for variant in pd.SPLIT_VARIANTS]
BITWISE = ["n65_k4", "k16_n40"]


def _run(prob, sy, c0=None, nsteps=NSTEPS, f=None, **over):
    """bspatom_tdse_split on a system of pivot_designs.split_system"""
    kw = dict(G=sy["G"], Q=sy["Q"], lam=sy["lam"], f=sy["f"] if f is None else f, W=sy["W"], w=sy["w"])
    return prob.tdse_split(sy["l"], sy["c0"] if c0 is None else c0, sy["dt"], nsteps, **{**kw, **over})


@functools.lru_cache(maxsize=None)
def _case(name, variant):
    """a designed system and its main run (test_gpu_tdse_split's options: resolvent_slots = 2, tdse_split_group = 3; every step observed
    and kept), in the keys test_gpu_tdse_split._accuracy reads.  Computed once, never changed."""
    prob, SB, HB, _, G2 = pivots._assembled(name)
    sy = pd.split_system(variant, SB, HB, G2[0])
    with split._Options(resolvent_slots=split.SLOTS, tdse_split_group=split.GROUP):
        c, info, obs, snaps = _run(prob, sy, obs_every=1, snap_every=1)
    for v in [c, info, obs, snaps] + [v for v in sy.values() if isinstance(v, np.ndarray)]:
        v.setflags(write=False)
    return dict(prob=prob, SB=SB, HB=HB, sy=sy, c0=sy["c0"], nsteps=NSTEPS, c=c, info=info, obs=obs, snaps=snaps)


@functools.lru_cache(maxsize=None)
def _reference(name, variant):
    """per scan: (the dense restatement's final packet, its rows, delta_ref); computed once"""
    d = _case(name, variant)
    sy = d["sy"]
    return [pref.delta_ref(d["SB"], d["HB"], sy["l"], sy["dt"], sy["c0"][q], sy["G"], sy["Q"], sy["lam"], sy["f"][:, q], sy["W"], sy["w"])
            for q in range(NSCAN)]


@pytest.mark.parametrize("name,variant", CASES, ids=["%s-%s" % c for c in CASES])
def test_accuracy_on_designed_matrices(name, variant):
    """Two steps of three channels (l = 0, 1, 0) and three scans (one real packet) on tiny8 (b 4, n = 8 < 2 b + 1), n65_k4 (b 3),
    lin256 (b 8, the limit of the small instances), k10_n65 (b 9: the instances for b <= 15 with six register rows unused) and k16_n40
    (b 15, the full window).  atomic: the absorbers of channels 0 and 1 make M_c design (A) at t = 20 and t = 2 -- every second group of
    b columns pivots at distance b, U's rows are 2 b wide, the stored factors of tsplit_factor_kernel are read by both half steps of
    both steps --, G the band of r, f real.  field: G makes N_j = S + G design (A) in the eigenchannel lam = +1 of scan 0 (f = -2i / dt)
    and lam = -1 of scan 1 (+2i / dt); the other eigenchannels get S - G and S + G / 2; scan 2 has a real f = 0.5.  both: both.
    test_gpu_tdse_split._accuracy unchanged: ||c - c_ref||_S <= 8 max(delta_ref, eps nsteps) max(1, ||c0||_S) on every scan, delta_ref
    from the dense against the solve_banded restatement; info == 0.  On the CPU band_lu_ref meets this at 0.12 .. 0.43 of the bound
    and misses it by 47 times or more with a pivot search cut to b / 2 or U's fill dropped beyond 1.25 b.
    Measured on the MI355X, the largest ||c - c_ref||_S / bound, atomic / field / both: tiny8 0.199 / 0.179 / 0.265, n65_k4 0.208 /
    0.232 / 0.231, lin256 0.212 / 0.214 / 0.209, k10_n65 0.248 / 0.166 / 0.191, k16_n40 0.508 / 0.151 / 0.403."""
    d = _case(name, variant)
    assert np.all(d["info"] == 0), d["info"]
    assert np.all(np.isfinite(d["c"].view(np.float64))) and np.max(np.abs(d["c"] - d["c0"])) > 1e-3
    worst = split._accuracy(d, _reference(name, variant))
    note("tdse_split pivots %s %s (b %d): max ||c - c_ref||_S / bound = %.3g" % (name, variant, d["prob"].k - 1, worst))


@pytest.mark.parametrize("name", BITWISE)
def test_bitwise_guarantees_where_the_swap_branch_runs(name):
    """P1 - P3 bit for bit on the "both" case, where sp_factor's swap branch runs at every distance up to b and rs_forward exchanges
    rows b apart, at b = 3 and b = 15: a second run; every scan alone; resolvent_slots = 1 and 2; tdse_split_group = 1; the snapshot
    after step 1 against the run of one step, and the second step continued from it; the _dev variant on torch tensors with the rows
    and the snapshots pre-filled with NaN."""
    d = _case(name, "both")
    prob, sy = d["prob"], d["sy"]
    n, nch = prob.nfun, len(sy["l"])
    run = lambda **over: _run(prob, sy, **{**dict(obs_every=1, snap_every=1), **over})
    def check(res, what):
        assert same(res[0], d["c"]) and np.array_equal(res[1], d["info"]) and same(res[2], d["obs"]) and same(res[3], d["snaps"]), what
    check(run(), "second run")
    for opts in (dict(resolvent_slots=1), dict(resolvent_slots=2), dict(tdse_split_group=1)):
        with split._Options(**opts):
            check(run(), opts)
    for q in range(NSCAN):                                     # each scan alone
        cq, iq, oq, sq = run(c0=sy["c0"][q], f=sy["f"][:, q:q + 1])
        assert same(cq, d["c"][q]) and iq[0] == d["info"][q] and same(oq[:, 0], d["obs"][:, q]) and same(sq[:, 0], d["snaps"][:, q]), q
    assert d["snaps"].shape == (NSTEPS, NSCAN, nch, n) and same(d["snaps"][-1], d["c"])
    cs, _ = _run(prob, sy, nsteps=1, f=sy["f"][:1])            # P3: the snapshot is the shorter run, and continues
    assert same(cs, d["snaps"][0])
    cl, _ = _run(prob, sy, c0=d["snaps"][0], nsteps=NSTEPS - 1, f=sy["f"][1:])
    assert same(cl, d["c"])
    dev = "cuda:0"
    put = lambda v: torch.from_numpy(np.array(v)).to(dev)
    cd, Gd, Wd, fd = put(sy["c0"]), put(sy["G"]), put(sy["W"]), put(sy["f"])
    od = torch.full(d["obs"].shape, float("nan"), dtype=torch.float64, device=dev)
    sd = torch.full(d["snaps"].shape, float("nan"), dtype=torch.complex128, device=dev)
    torch.cuda.synchronize()
    infod = prob.tdse_split_dev(sy["l"], NSCAN, NSTEPS, sy["dt"], cd.data_ptr(), G_ptr=Gd.data_ptr(), Q=sy["Q"], lam=sy["lam"], f_ptr=fd.data_ptr(),
                                nabs=sy["W"].shape[0], W_ptr=Wd.data_ptr(), w=sy["w"], obs_every=1, obs_ptr=od.data_ptr(), snap_every=1,
                                snap_ptr=sd.data_ptr())
    check((cd.cpu().numpy(), infod, od.cpu().numpy(), sd.cpu().numpy()), "_dev")


@pytest.mark.parametrize("name", pd.SPLIT_ZERO_GRIDS)
def test_zero_pivots_are_replaced_and_counted(name):
    """G = minus the columns j1 = n // 3 and j2 = 2n // 3 + 1 of S, lam = [-1, 0.5, 1], two steps, three scans: the field matrix
    S + G has two exactly zero columns, in the eigenchannel lam = +1 of scan 0 (f = -2i / dt) and lam = -1 of scan 1 (+2i / dt), and a
    zero column stays exactly zero under any elimination; every other matrix of the call is regular with its pivots 1e3 times above
    the threshold (test_tdse_split_pivots_cpu.py).  So info is [4, 4, 0] exactly -- two replaced pivots per step, found at another
    pinfo[q nch + j] in scan 0 than in scan 1 --, and [2, 2, 0] with column j2 alone; every output is finite; a second run has the
    same bits; scan 2 has the bits of its run alone, next to singular neighbours.  b = 3, 8 and 9.  The atomic matrices cannot be made
    singular through the public arguments (H_l cannot be cancelled), and which of two equal pivot candidates is taken shows in the
    bits alone: neither is asked for.  Measured on the MI355X: the counts as stated; max |c| of the singular scans 1e27 .. 3e30
    (two divisions by the threshold), of scan 2 below 1."""
    prob, SB, HB, _, G2 = pivots._assembled(name)
    for variant, want in (("zeros", [4, 4, 0]), ("zero", [2, 2, 0])):
        sy = pd.split_system(variant, SB, HB, G2[0])
        c, info, obs, snaps = _run(prob, sy, obs_every=1, snap_every=1)
        print("%s %s: info %s  max |c| per scan %s" % (name, variant, info, np.max(np.abs(c), axis=(1, 2))))
        assert np.array_equal(info, want), (variant, info)
        assert all(np.all(np.isfinite(v.view(np.float64))) for v in (c, obs, snaps))
        c2, info2, obs2, snaps2 = _run(prob, sy, obs_every=1, snap_every=1)
        assert same(c2, c) and np.array_equal(info2, info) and same(obs2, obs) and same(snaps2, snaps)
        ca, ia, oa, sa = _run(prob, sy, c0=sy["c0"][2], f=sy["f"][:, 2:3], obs_every=1, snap_every=1)
        assert ia[0] == 0 and same(ca, c[2]) and same(oa[:, 0], obs[:, 2]) and same(sa[:, 0], snaps[:, 2])
        assert np.max(np.abs(c[2] - sy["c0"][2])) > 1e-3
