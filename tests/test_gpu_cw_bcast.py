"""The band reduction's four-items-per-wave kernel (csrc/crawford.hip::crawford_item4_kernel) with row I of X handed to the
reflector's FMAs as a DPP operand (option cw_bcast=1: v_fmac_f64_dpp .. row_newbcast:I, hand-written wait states) against the
same kernel with the row going round through LDS (cw_bcast=0).  The arithmetic and its order are the same, so the band and the
spectra must be equal bit for bit; a missed wait state shows as a difference on some waves of some launches, or from run to run."""
import numpy as np
import pytest
from test_gpu_stages import input_from_case
from test_gpu_solve import _Options

pytestmark = pytest.mark.gpu
from bspatom_amd import capi

# n32: the smallest n the band route takes (N = 4 blocks): wavefronts of one item, the elimination alone in a wave;
# n128: wavefronts of up to five items, a full wave and a wave of one; bc10, ka_ra, c1_lin: n is not a multiple of 8, a ragged last
# block; c3_1024_l31 with 32 channels: two stream groups (16 channels each), with 12: one group;
# k5, k3: pencils of half-width 4 and 2 built as bench.py builds its own: their 8 x 8 blocks hold structural zeros, so reflector
# steps with sig == 0 (H = I, the masked divisions) occur
MADE = {"n32": dict(kind_grid=0, ra=0.0, rb=20.0, k=9, nfun=32, n0_ini=1, l_ini=0, l_fin=3, zatom=1.0),
        "k5": dict(kind_grid=0, ra=0.0, rb=60.0, k=5, nfun=100, n0_ini=1, l_ini=0, l_fin=3, zatom=1.0),
        "k3": dict(kind_grid=0, ra=0.0, rb=40.0, k=3, nfun=67, n0_ini=1, l_ini=0, l_fin=2, zatom=1.0)}
CASES = [("n32", None), ("n128", None), ("bc10", None), ("ka_ra", None), ("c1_lin", None), ("c3_1024_l31", 32), ("c3_1024_l31", 12),
         ("k5", None), ("k3", None)]
IDS = ["%s-%s" % (c[0], c[1]) if c[1] else c[0] for c in CASES]
VARIANTS = [dict(), dict(cw_onediv=1), dict(cw_nw=4), dict(cw_ipw=1), dict(cw_ipw=2)]


def _problem(name, nl):
    prob = capi.Problem(capi.make_input(**MADE[name]) if name in MADE else input_from_case(name))
    assert prob.route() == 2
    return prob, (prob.lmax + 1 if nl is None else nl)


def _run(prob, SB, HB, nl, **kw):
    with _Options(**kw):
        AB, info = capi.stage_crawford(SB, HB)
        E, einfo = prob.solve(0, nl)
    assert info == 0 and np.all(einfo == 0), kw
    return AB, E


@pytest.mark.parametrize("name,nl", CASES, ids=IDS)
def test_dpp_broadcast_equals_the_lds_form(name, nl):
    prob, nl = _problem(name, nl)
    if name == "n32":
        assert prob.nfun == 32
    SB, HB = prob.assemble(0, nl)
    for var in VARIANTS:
        AB0, E0 = _run(prob, SB, HB, nl, cw_bcast=0, **var)
        AB1, E1 = _run(prob, SB, HB, nl, cw_bcast=1, **var)
        assert np.array_equal(AB1, AB0), (name, var, np.max(np.abs(AB1 - AB0)))
        assert np.array_equal(E1, E0), (name, var, np.max(np.abs(E1 - E0)))
    prob.close()


def test_dpp_form_does_not_change_from_run_to_run():
    prob, nl = _problem("c3_1024_l31", 32)
    SB, HB = prob.assemble(0, nl)
    runs = [_run(prob, SB, HB, nl, cw_bcast=1) for _ in range(3)]
    for AB, E in runs[1:]:
        assert np.array_equal(AB, runs[0][0]) and np.array_equal(E, runs[0][1])
    prob.close()


def test_occupancy_does_not_reach_the_bits():
    """cw_ldspad = KiB of unused LDS per workgroup: 9 leaves 8 waves per CU (18 KiB per wave of the CU's 160), 4 leaves 12; the
    default (0) has 16."""
    prob, nl = _problem("c3_1024_l31", 32)
    SB, HB = prob.assemble(0, nl)
    AB0, E0 = _run(prob, SB, HB, nl, cw_bcast=1)
    for pad in (9, 4):
        AB, E = _run(prob, SB, HB, nl, cw_bcast=1, cw_ldspad=pad)
        assert np.array_equal(AB, AB0) and np.array_equal(E, E0), pad
    prob.close()
