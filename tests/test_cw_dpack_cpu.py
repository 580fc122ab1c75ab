"""The packed records of the band reduction's diagonal blocks (csrc/crawford.hip: cw_pk, cw_up), without a GPU: the index
functions as the source states them, and the lane-level emulation of the item kernel on that layout (tools/emu_crawford.py)
against the dense statement of the reduction (tools/proto_crawford.py)."""
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
SRC = os.path.join(ROOT, "bspatom_amd", "csrc", "crawford.hip")


def _source_index_functions():
    """cw_pk and cw_up as Python functions, from the expressions in the source (integer arithmetic: / is //)"""
    text = open(SRC).read()
    fns = {}
    for name in ("cw_pk", "cw_up"):
        m = re.search(r"constexpr int %s\(int i, int j\) \{ return ([^;]+); \}" % name, text)
        assert m, name
        fns[name] = m.group(1).replace("/", "//")
    env = {}
    env["cw_pk"] = lambda i, j: eval(fns["cw_pk"], {}, {"i": i, "j": j})
    env["cw_up"] = lambda i, j: eval(fns["cw_up"], {"cw_pk": env["cw_pk"]}, {"i": i, "j": j})
    sizes = {k: int(v) for k, v in re.findall(r"constexpr int (CWD|CWU|CB|CBB) = ([^;]+);", text) if v.strip().isdigit()}
    return env["cw_pk"], env["cw_up"], sizes


def test_packed_index_is_a_bijection():
    pk, up, sizes = _source_index_functions()
    assert sizes.get("CB") == 8
    low = [pk(i, j) for i in range(8) for j in range(i + 1)]
    assert sorted(low) == list(range(36))                               # {(i, j): 8 > i >= j >= 0} onto 0 .. 35
    assert low == list(range(36))                                       # ... by rows
    upper = [up(i, j) for j in range(8) for i in range(j)]
    assert sorted(upper) == list(range(28))                             # block 0's strict upper triangle onto 0 .. 27
    # a window D_p, D_{p+1} is 2 x 36 doubles: 36 lanes of 16 bytes, and a record a multiple of 16 bytes
    assert (36 * 8) % 16 == 0 and 2 * 36 * 8 == 36 * 16
    import emu_crawford as emu
    assert all(emu.pk(i, j) == pk(i, j) for i in range(8) for j in range(i + 1))
    assert all(emu.up(i, j) == up(i, j) for j in range(8) for i in range(j))
    assert (emu.CWD, emu.CWU) == (36, 28)


def test_emulated_window_reproduces_the_dense_statement():
    """n = 32, k = 9 (four blocks: the smallest pencil with a chase item) and a ragged n = 44: the emulated kernel on packed records
    ends with the spectrum of the dense prototype's block tridiagonal matrix -- both are orthogonally similar to L^-1 H L^-T,
    computed by different reflectors, so they agree to eps cond(S) |lambda|_max (2e-14 sqrt(n), the bound of the GPU test of this
    stage), and the band is no wider than the prototype's."""
    import emu_crawford as emu
    import proto_crawford as pc
    for n, k in ((32, 9), (44, 9)):
        rng = np.random.default_rng(n)
        SB = np.zeros((k, n)); HB = np.zeros((k, n))
        SB[0] = 2.0 * k + rng.random(n)
        for d in range(1, k):
            SB[d, :n - d] = rng.standard_normal(n - d)
        for d in range(k):
            HB[d, :n - d] = rng.standard_normal(n - d)
        A = emu.run(SB, HB)                                             # original order, symmetric, from the packed D window
        S = pc.dense_from_upper_band(SB)[::-1, ::-1].copy(); H = pc.dense_from_upper_band(HB)[::-1, ::-1].copy()
        P = pc.crawford_block(S, H, k - 1)
        ev, ref = np.linalg.eigvalsh(A), np.linalg.eigvalsh((P + P.T) / 2)
        err = np.max(np.abs(ev - ref)) / np.max(np.abs(ref))
        print("n %d: emulated kernel on packed records vs dense prototype: %.2e of |lambda|_max" % (n, err))
        assert err < 2e-14 * np.sqrt(n)
        i, j = np.indices(A.shape)
        assert np.all(A[np.abs(i - j) > 2 * (k - 1) - 1] == 0.0) and np.array_equal(A, A.T)
