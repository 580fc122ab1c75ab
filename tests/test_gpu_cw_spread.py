"""The band reduction's quads on workgroups of 2 or 4 waves (csrc/crawford.hip::crawford_item4_spread_kernel, option cw_spread):
wave 0 runs the RQ loops of the quad's four items, one barrier, then every wave runs the congruences of its own item slots.  An
item's arithmetic does not depend on the wave that runs it, so the band and the spectra must equal those of one wave per quad
(cw_spread=0) bit for bit; a Q read before the barrier, an operand landing in another slot's place or a slot dealt to two waves or
to none shows as a difference on some launches, or from run to run."""
import numpy as np
import pytest
from test_gpu_stages import input_from_case
from test_gpu_solve import _Options

pytestmark = pytest.mark.gpu
from bspatom_amd import capi

# n32: N = 4 blocks: the first wavefronts have an elimination and no chase item (a quad without phase A; with 4 waves, three waves
# without an item), later ones one chase item and the elimination; n128: wavefronts of up to five items, two quads, the second with
# one item; n100 / k5 / k3: n is not a multiple of 8, a ragged last block; k5, k3: half-widths 4 and 2, reflector steps with
# sig == 0; c3_1024_l31 with 32 channels: two stream groups of 16, with 12: one group, up to eleven quads per channel
MADE = {"n32": dict(kind_grid=0, ra=0.0, rb=20.0, k=9, nfun=32, n0_ini=1, l_ini=0, l_fin=3, zatom=1.0),
        "n100": dict(kind_grid=0, ra=0.0, rb=50.0, k=9, nfun=100, n0_ini=1, l_ini=0, l_fin=3, zatom=1.0),
        "k5": dict(kind_grid=0, ra=0.0, rb=60.0, k=5, nfun=100, n0_ini=1, l_ini=0, l_fin=3, zatom=1.0),
        "k3": dict(kind_grid=0, ra=0.0, rb=40.0, k=3, nfun=67, n0_ini=1, l_ini=0, l_fin=2, zatom=1.0)}
CASES = [("n32", None), ("n128", None), ("n128", 1), ("n100", None), ("k5", None), ("k3", None), ("c3_1024_l31", 12), ("c3_1024_l31", 32)]
IDS = ["%s-%s" % (c[0], c[1]) if c[1] else c[0] for c in CASES]


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


@pytest.mark.parametrize("onediv", [0, 1])
@pytest.mark.parametrize("name,nl", CASES, ids=IDS)
def test_spread_quads_equal_one_wave_per_quad(name, nl, onediv):
    prob, nl = _problem(name, nl)
    SB, HB = prob.assemble(0, nl)
    AB0, E0 = _run(prob, SB, HB, nl, cw_spread=0, cw_onediv=onediv)
    for spread in (2, 4, 1):
        AB, E = _run(prob, SB, HB, nl, cw_spread=spread, cw_onediv=onediv)
        assert np.array_equal(AB, AB0), (name, spread, np.max(np.abs(AB - AB0)))
        assert np.array_equal(E, E0), (name, spread, np.max(np.abs(E - E0)))
    prob.close()


@pytest.mark.parametrize("onediv", [0, 1])
def test_one_solve_mixes_the_three_instances(onediv):
    """32 channels, up to eleven quads per channel: 4 waves up to two quads per channel, 2 up to six, one beyond"""
    prob, nl = _problem("c3_1024_l31", 32)
    SB, HB = prob.assemble(0, nl)
    AB0, E0 = _run(prob, SB, HB, nl, cw_spread=0, cw_onediv=onediv)
    AB, E = _run(prob, SB, HB, nl, cw_spread=1, cw_spread_cap4=2 * 32, cw_spread_cap2=6 * 32, cw_onediv=onediv)
    assert np.array_equal(AB, AB0) and np.array_equal(E, E0)
    prob.close()


@pytest.mark.parametrize("spread", [2, 4])
def test_spread_does_not_change_from_run_to_run(spread):
    prob, nl = _problem("c3_1024_l31", 32)
    SB, HB = prob.assemble(0, nl)
    runs = [_run(prob, SB, HB, nl, cw_spread=spread) for _ in range(3)]
    for AB, E in runs[1:]:
        assert np.array_equal(AB, runs[0][0]) and np.array_equal(E, runs[0][1])
    prob.close()


@pytest.mark.parametrize("keep", [dict(cw_split=50), dict(cw_nw=4), dict(cw_bcast=0)], ids=["split50", "nw4", "bcast0"])
def test_options_that_keep_one_wave_per_quad(keep):
    prob, nl = _problem("c3_1024_l31", 12)
    SB, HB = prob.assemble(0, nl)
    AB0, E0 = _run(prob, SB, HB, nl, cw_spread=0, **keep)
    for spread in (1, 4):
        AB, E = _run(prob, SB, HB, nl, cw_spread=spread, **keep)
        assert np.array_equal(AB, AB0) and np.array_equal(E, E0), (keep, spread)
    prob.close()
