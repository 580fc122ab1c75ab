"""The bits of the one-wave banded LU (csrc/band_lu_wave.h) as its two callers give them out: bspatom_resolvent and
bspatom_resolvent_chain (csrc/resolvent.hip) and bspatom_tdse_split (csrc/tdse_split.hip), both register-window instances of every
kernel (b <= 8: tiny8, n65_k4; b <= 15: k10_n65 with b = 9, k16_n40 with b = 15).  G2/G3 and C1 - C6 of include/bspatom.h and P1 - P3
of include/bspatom_tdse_split.h promise bits from run to run; this file holds them from commit to commit:
tests/golden/resolvent_bits.npz keeps the SHA-256 of every output array of every case below, recorded on the MI355X from a build of
commit ae54d7e, the parent of the commit that stated every multiply-add of these kernels in the source (DESIGN.md 4.7 "Fused
products"), with that build's libbspatom.so in place and the command below; a change to these kernels must reproduce them.  The
digests are never re-recorded from the code under test: `python tests/test_gpu_resolvent_bits.py FILE` writes them from whatever
library is built, for use on a build of the parent of a change that means to move the bits.

Cases.  resolvent, per grid: plain (two channels, complex z, no absorber), cap (absorber on, one z real inside the spectrum), real
(Im z = 0, no absorber, real B = P: G3), chain (two chains of two stages, nrhs = 2, the band of r in between, one stage with
absorber); far: design (A) of tests/pivot_designs.py in W, every second group of b columns pivots at distance b and U fills to 2 b,
by the call and by a chain of two stages.  The single-channel matrix cannot be made singular through the public arguments
(test_gpu_resolvent_pivots.py), so the replaced-pivot count of that family is recorded as the zeros it is.  split, per grid: 2 scans
x 3 channels x 3 steps with two projections, a row and a snapshot per step, without and with absorber; far: pivot_designs'
split_system "both"; zeros: its "zeros" on a grid of either instance, info [4, 4, 0] as test_gpu_tdse_split_pivots.py states."""
import hashlib
import os
import sys
import numpy as np
import pytest
import torch                               # first: its HIP runtime is the one the process uses

import pivot_designs as pd
import test_gpu_resolvent as single        # its right-hand sides (_vectors)
import test_gpu_resolvent_pivots as pivots  # its problems and bands, assembled once per grid
import test_gpu_tdse_split as split        # its angular matrices and its option setter

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resolvent_bits.npz")
GRIDS = ["tiny8", "n65_k4", "k10_n65", "k16_n40"]
FAR = ["n65_k4", "k10_n65", "k16_n40"]     # pivot_designs.SINGLE_CASES at these sizes
ZEROS = ["n65_k4", "k10_n65"]              # pivot_designs.SPLIT_ZERO_GRIDS at these sizes
DT = 0.05


def _resolvent(name, kind):
    prob, SB, HB, WB, G2 = pivots._assembled(name)
    n = prob.nfun
    B, P = single._vectors(n, 3, 2, 5)
    if kind == "plain":
        return prob.resolvent([0, 1], [0.3 + 0.05j, -0.2 - 0.3j], B, P=P)
    if kind == "cap":
        return prob.resolvent([0, 1, 1], [0.3, 0.3 - 0.05j, 1.1 + 0.05j], B, W=np.stack([WB, 0.5 * WB]), w=[0, 1, -1], P=P)
    if kind == "real":
        Br = np.random.default_rng(3).standard_normal((2, n))
        return prob.resolvent([0, 1, 1], [0.3, 0.3, -1.0], Br, P=Br)
    if kind == "chain":
        l, z, w = [[0, 1], [1, 0]], [[0.3 + 0.05j, -0.2 + 0.05j], [0.7 - 0.05j, 0.3]], [[-1, 0], [-1, 0]]
        return prob.resolvent_chain(l, z, B[:2], G=G2[:1], W=WB, w=w, P=P)
    sy = pd.design_a_single(SB, HB)
    if kind == "far":
        return prob.resolvent(sy["l"], sy["z"], B, W=sy["W"], w=sy["w"], P=P)
    assert kind == "far-chain"
    return prob.resolvent_chain(sy["l"], sy["z"], B[:2], G=G2[:1], W=sy["W"], w=sy["w"], P=P)


def _split(name, kind):
    prob, SB, HB, WB, G2 = pivots._assembled(name)
    n = prob.nfun
    with split._Options(resolvent_slots=split.SLOTS, tdse_split_group=split.GROUP):
        if kind in ("nocap", "cap"):
            nscan, nch, nsteps = 2, 3, 3
            rng = np.random.default_rng(500 + n)
            Q, lam = split._angular(nch, rng)
            f = rng.uniform(0.2, 1.0, (nsteps, nscan))
            c0 = (rng.standard_normal((nscan, nch, n)) + 1j * rng.standard_normal((nscan, nch, n))) / np.sqrt(n)
            c0[0] = c0[0].real
            P = rng.standard_normal((2, nch, n)) + 1j * rng.standard_normal((2, nch, n))
            cap = dict(W=WB, w=[0, -1, 0]) if kind == "cap" else {}
            return prob.tdse_split([0, 1, 0], c0, DT, nsteps, G=np.ascontiguousarray(G2[0]), Q=Q, lam=lam, f=f, P=P, obs_every=1, snap_every=1,
                                   **cap)
        sy = pd.split_system(dict(far="both", zeros="zeros")[kind], SB, HB, G2[0])
        return prob.tdse_split(sy["l"], sy["c0"], sy["dt"], sy["nsteps"], G=sy["G"], Q=sy["Q"], lam=sy["lam"], f=sy["f"], W=sy["W"], w=sy["w"],
                               obs_every=1, snap_every=1)


CASES = ([("resolvent", name, kind) for name in GRIDS for kind in ("plain", "cap", "real", "chain")]
         + [("resolvent", name, kind) for name in FAR for kind in ("far", "far-chain")]
         + [("split", name, kind) for name in GRIDS for kind in ("nocap", "cap")]
         + [("split", name, "far") for name in GRIDS] + [("split", name, "zeros") for name in ZEROS])
IDS = ["%s-%s-%s" % c for c in CASES]


def _digests(family, name, kind):
    """(the SHA-256 of every output array of a case, shape and type included; its info)"""
    out = (_resolvent if family == "resolvent" else _split)(name, kind)
    assert all(v is not None and np.all(np.isfinite(np.ascontiguousarray(v).view(np.float64 if v.dtype.kind in "fc" else v.dtype))) for v in out)
    info = out[2] if family == "resolvent" else out[1]
    hexes = []
    for v in out:
        v = np.ascontiguousarray(v)
        hexes.append(hashlib.sha256(("%s %s " % (v.dtype.str, v.shape)).encode() + v.tobytes()).hexdigest())
    return np.array(hexes), np.array(info)


@pytest.mark.parametrize("family,name,kind", CASES, ids=IDS)
def test_bits_are_the_recorded_ones(family, name, kind):
    """X, R, info (resolvent: the call's, the chain's) and c, info, rows, snapshots (split) of a case have the recorded digests; info is
    zero everywhere but in the zeros design, [4, 4, 0] there."""
    got, info = _digests(family, name, kind)
    with np.load(GOLDEN) as gold:
        want = gold["%s-%s-%s" % (family, name, kind)]
    print("%s %s %s: info %s" % (family, name, kind, info.ravel()))
    assert np.array_equal(info.ravel(), [4, 4, 0]) if kind == "zeros" else np.all(info == 0), info
    assert got.shape == want.shape and list(got) == list(want), [i for i in range(len(got)) if got[i] != want[i]]


if __name__ == "__main__":
    np.savez(sys.argv[1], **{i: _digests(*c)[0] for i, c in zip(IDS, CASES)})
    print("recorded %d cases into %s" % (len(CASES), sys.argv[1]))
