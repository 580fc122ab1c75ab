"""bspatom_tdse_fields without a GPU: the NumPy restatement tests/tdse_fields_ref.py against the restatement it is built on and against
the rotation invariance of a field of any direction; the host helpers of the polarised length-gauge coupling; the entry points, their
kernels in the library, and the argument checks that return before any GPU work."""
import ctypes as C
import math
import os
import sys
import numpy as np
import pytest
from conftest import ROOT

import tdse_fields_ref
import tdse_ref
import tdse_static_ref
from bspatom_amd import capi, host

EPS = tdse_ref.EPS
NAMES = ("bspatom_tdse_fields", "bspatom_tdse_fields_dev")
CHANNELS9 = [(l, m) for l in range(3) for m in range(-l, l + 1)]
TILT = (math.sin(0.4) * math.cos(1.1), math.sin(0.4) * math.sin(1.1), math.cos(0.4))


def same(x, y):
    """the same values with the same signs of zero (the bytes of a long double include padding: not compared)"""
    x, y = np.asarray(x), np.asarray(y)
    if x.shape != y.shape or x.dtype != y.dtype:
        return False
    parts = lambda z: (z.real, z.imag) if np.iscomplexobj(z) else (z,)
    return all(np.array_equal(u, v) and np.array_equal(np.signbit(u), np.signbit(v)) for u, v in zip(parts(x), parts(y)))


# ---- the restatement ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rd,cd", [(np.float64, np.complex128), (np.longdouble, np.clongdouble)])
def test_one_field_is_the_static_restatement(rd, cd):
    E, pairs, D, a0, field = tdse_ref.system(3, 5, 2, 12)
    static = tdse_static_ref.static_system(3, 5)
    for scheme in (0, 1):
        for st in (None, static):
            want = tdse_static_ref.propagate(E, pairs, D, a0, field, 0.05, static=st, scheme=scheme, rdtype=rd, cdtype=cd, snap_every=4,
                                             obs_every=5)
            got = tdse_fields_ref.propagate(E, pairs, D, [0] * len(pairs), a0, field[:, :, None, :], 0.05, static=st, scheme=scheme,
                                            rdtype=rd, cdtype=cd, snap_every=4, obs_every=5)
            assert len(got) == 4 and all(same(g, w) for g, w in zip(got, want)), (scheme, st is None)
            assert got[2].shape == (4, 2, 3, 6)


def test_one_field_split_into_two_with_the_same_table():
    """Pairs moved to a second field that carries the same table: the same equation.  The bound is the distance between the complex128
    and the long-double run of the one-field restatement (in the restatement a pair's term is one statement whatever its field, so the
    difference is expected to be 0)."""
    for scheme in (0, 1):
        E, pairs, D, fidx, a0, field, static = tdse_fields_ref.system(3, 7, 2, 30, 2)
        field[:, :, 1, :] = field[:, :, 0, :]
        one = tdse_static_ref.both(E, pairs, D, a0, np.ascontiguousarray(field[:, :, 0, :]), 0.05, static=static, scheme=scheme)
        two = tdse_fields_ref.propagate(E, pairs, D, fidx, a0, field, 0.05, static=static, scheme=scheme)
        assert sorted(set(fidx)) == [0, 1]
        own = max(float(np.max(np.abs(one[0][0].astype(np.clongdouble) - one[1][0]))), EPS)
        d = float(np.max(np.abs(two[0] - one[0][0])))
        print("split, scheme %d: |two fields - one field| = %.3g, the complex128 run's own distance %.3g" % (scheme, d, own))
        assert d <= own


def test_rows_of_the_restatement():
    """Small integers, every sum exact: z_{c,g} from the definition written as loops; k = 0 .. 5 with the pairs of field 0 alone"""
    rng = np.random.default_rng(5)
    E = rng.integers(-3, 4, size=(3, 3)).astype(np.float64)
    pairs, fidx = [(0, 1), (1, 2), (0, 1), (2, 0)], [0, 1, 2, 1]
    D = rng.integers(-3, 4, size=(4, 3, 3)).astype(np.float64)
    a = (rng.integers(-3, 4, size=(2, 3, 3)) + 1j * rng.integers(-3, 4, size=(2, 3, 3))).astype(np.complex128)
    got = tdse_fields_ref.observables(E, pairs, D, fidx, 3, None, a)
    assert got.shape == (2, 3, 10) and np.all(got[..., 4:6] == 0.0)
    want = np.zeros((2, 3, 3), dtype=np.complex128)
    for q in range(2):
        for p, (i, f) in enumerate(pairs):
            for n in range(3):
                for m in range(3):
                    want[q, f, fidx[p]] += np.conj(a[q, f, m]) * D[p, n, m] * a[q, i, n]
    for g, k in ((0, 2), (1, 6), (2, 8)):
        assert np.array_equal(got[..., k], want[..., g].real) and np.array_equal(got[..., k + 1], want[..., g].imag)
    assert np.array_equal(got[..., 0], np.sum(a.real ** 2 + a.imag ** 2, axis=-1))


# ---- the host helpers -----------------------------------------------------------------------------------------------------
def test_dipole_blocks_pol_counts_and_q0_list():
    blocks, fidx = host.dipole_blocks_pol(CHANNELS9)
    assert len(blocks) == len(fidx) == 12 and fidx.count(0) == 4 and fidx.count(1) == 8
    assert fidx == sorted(fidx)
    # the q = 0 list is dipole_blocks' without the pairs whose 3j symbol vanishes (m differs): for the nine channels, and for every pair
    nonzero = lambda chans: [b for b in host.dipole_blocks(chans, 1, 0) if b[5][0] != 0.0]
    assert [b for b, g in zip(blocks, fidx) if g == 0] == nonzero(CHANNELS9)
    for i, ca in enumerate(CHANNELS9):
        for cb in CHANNELS9[i + 1:]:
            b2, f2 = host.dipole_blocks_pol([ca, cb])
            assert [b for b, g in zip(b2, f2) if g == 0] == nonzero([ca, cb])
            assert len(nonzero([ca, cb])) == (1 if abs(ca[0] - cb[0]) == 1 and ca[1] == cb[1] else 0)
    # q = +1: m rises by one from ket to bra, both orders of l, and the angular factor is dipole_blocks' with mph = 1
    for (a_, b_, l0, lf, c0, coef), g in zip(blocks, fidx):
        if g == 1:
            (lf_, mf), (l0_, m0) = CHANNELS9[a_], CHANNELS9[b_]
            assert (lf_, l0_) == (lf, l0) and mf == m0 + 1 and abs(lf - l0) == 1 and c0 == 1.0
            ref = [b for b in host.dipole_blocks([CHANNELS9[min(a_, b_)], CHANNELS9[max(a_, b_)]], 1, 1)]
            if a_ < b_:
                assert ref and ref[0][5] == coef
    assert any(a_ > b_ for (a_, b_, *_), g in zip(blocks, fidx) if g == 1)


def test_field_table_pol_against_its_formula():
    dt, nsteps = 0.1, 5
    t = host.rk_nodes(0.5, dt, nsteps)
    Fx, Fy, Fz = np.cos(t), 0.3 * np.sin(2 * t), 0.2 + t
    tab = host.field_table_pol([lambda s: (np.cos(s), 0.3 * np.sin(2 * s), 0.2 + s), np.stack([Fx, Fy, Fz]), lambda s: (0.0, 0.0, 1.0)],
                               0.5, dt, nsteps)
    assert tab.shape == (nsteps, 6, 2, 3) and tab.dtype == np.complex128
    for q in (0, 1):
        assert np.array_equal(tab[:, :, 0, q], Fz.astype(np.complex128))
        assert np.array_equal(tab[:, :, 1, q], -(Fx - 1j * Fy) / math.sqrt(2.0))
    assert np.all(tab[:, :, 0, 2] == 1.0) and np.all(tab[:, :, 1, 2] == 0.0)
    with pytest.raises(ValueError):
        host.field_table_pol([lambda s: (np.cos(s), np.sin(s))], 0.5, dt, nsteps)


def test_dipole_vector_of_rows():
    obs = np.zeros((2, 1, 3, 8))
    obs[..., 2], obs[..., 6], obs[..., 7] = 0.5, 0.25, -1.0
    v = host.tdse_dipole_vector(obs)
    assert v.shape == (2, 1, 3)
    assert np.array_equal(v[..., 2], np.full((2, 1), 3.0))
    assert np.allclose(v[..., 0], -math.sqrt(2.0) * 0.75, rtol=1e-15) and np.allclose(v[..., 1], math.sqrt(2.0) * 3.0, rtol=1e-15)
    with pytest.raises(ValueError):
        host.tdse_dipole_vector(obs[..., :6])


def pol_system(count, seed=0):
    """The nine channels l <= 2 with all m, E by l alone, the blocks of dipole_blocks_pol on synthetic symmetric radial blocks R(l, l+1) in
    long double: (E, pairs, D, fidx)"""
    rng = np.random.default_rng(31 + seed)
    El = np.sort(rng.uniform(-0.5, 1.0, size=(3, count)), axis=1)
    R = {}
    for l in (0, 1):
        G = rng.standard_normal((count, count)) / np.sqrt(count)
        R[(l, l + 1)] = R[(l + 1, l)] = (G + G.T).astype(np.longdouble)
    E = np.stack([El[l] for l, _ in CHANNELS9])
    blocks, fidx = host.dipole_blocks_pol(CHANNELS9)
    pairs = [(b_, a_) for a_, b_, *_ in blocks]
    D = np.stack([np.longdouble(c0) * np.longdouble(coef[0]) * R[(l0, lf)] for _, _, l0, lf, c0, coef in blocks])
    return E, pairs, D, fidx


def shell_populations(a, channels):
    """|a|^2 summed over m: (..., 3, count)"""
    p = (a.real * a.real + a.imag * a.imag)
    lmax = max(l for l, _ in channels)
    return np.stack([sum(p[..., c, :] for c, (l, _) in enumerate(channels) if l == ll) for ll in range(lmax + 1)], axis=-2)


def rotation_check(tag, obs, a, channels, tilt=TILT):
    """scan 0: F along z, scan 1: the same envelope along `tilt`.  The shell populations agree and the dipole vector of scan 1 is
    tilt times the z dipole of scan 0, to 64 eps of double (scaled by the largest dipole): the runs are in long double, whose rounding
    is 2048 times finer than double's, and the 3j symbols and the field table are correct to a few eps of double."""
    sp = shell_populations(a, channels)
    dp = float(np.max(np.abs(sp[0] - sp[1])))
    v = host.tdse_dipole_vector(obs)
    dz = v[:, 0, 2]
    big = float(np.max(np.abs(dz)))
    dv = float(np.max(np.abs(v[:, 1, :] - dz[:, None] * np.array(tilt, dtype=v.dtype)[None, :])))
    stray = float(np.max(np.abs(v[:, 0, :2])))
    print("%s: shell populations differ by %.3g (%.3g eps); dipole vector off by %.3g (largest dipole %.3g, %.3g eps of it); z scan's "
          "x, y %.3g" % (tag, dp, dp / EPS, dv, big, dv / (EPS * big) if big else 0.0, stray))
    assert dp <= 64 * EPS
    assert big > 1e-4 and dv <= 64 * EPS * big and stray <= 64 * EPS * big
    return dp, dv


def test_rotation_invariance():
    count, nsteps, dt = 4, 24, 0.05
    E, pairs, D, fidx = pol_system(count)
    T = nsteps * dt
    env = lambda t: 0.8 * np.sin(np.pi * t / T) ** 2 * np.cos(2.0 * t)
    field = host.field_table_pol([lambda t: (0.0 * t, 0.0 * t, env(t)), lambda t: tuple(n * env(t) for n in TILT)], 0.0, dt, nsteps)
    a0 = np.zeros((2, 9, count), dtype=np.complex128)
    a0[:, 0, 0] = 1.0
    a, err, obs = tdse_fields_ref.propagate(E, pairs, D, fidx, a0, field, dt, scheme=1, rdtype=np.longdouble, cdtype=np.clongdouble, obs_every=1)
    assert obs.shape == (nsteps + 1, 2, 9, 8) and obs.dtype == np.longdouble
    rotation_check("rotation", obs, a, CHANNELS9)
    moved = [c for c, (l, m) in enumerate(CHANNELS9) if m != 0]
    assert float(np.max(np.abs(a[1][moved]))) > 1e-3 and np.all(a[0][moved] == 0.0)
    assert float(np.sum(np.abs(a[0, 0]) ** 2)) < 1.0 - 1e-3                                   # the pulse is felt


# ---- the library ----------------------------------------------------------------------------------------------------------
def test_entry_points_bound():
    L = capi.lib()
    header = open(os.path.join(ROOT, "include", "bspatom.h")).read()
    for name in NAMES:
        assert name in capi.EXPORTS
        assert hasattr(L, name)
        assert len(getattr(L, name).argtypes) == 26
        assert getattr(L, name).argtypes[:24] == L.bspatom_tdse_static.argtypes
        assert hasattr(capi.Problem, name[len("bspatom_"):])
        assert "int %s(" % name in header
    assert "#define BSPATOM_TDSE_MAX_FIELDS 3" in header
    assert len(L.bspatom_tdse_static.argtypes) == 24


def test_kernels_in_library_without_scratch_or_spills():
    """Six stages x two schemes x NF = 2, 3 on the narrow tile, the observing stage 0 likewise, the reductions to rows of 8 and 10"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import codeobj_notes
    ks = codeobj_notes.kernels(os.path.join(ROOT, "bspatom_amd", "libbspatom.so"))
    want = {"tdse_fields_stage_kernel": 24, "tdse_fields_observe_kernel": 4, "tdse_obs_reduce_fields_kernel": 2}
    for key, num in want.items():
        hits = [v for name, v in ks.items() if key in name]
        assert len(hits) == num, (key, [n for n in ks if "tdse" in n])
        for v in hits:
            assert (v["private_segment_fixed_size"] or 0) == 0, (key, v)
            assert (v["vgpr_spill_count"] or 0) == 0, (key, v)


def test_argument_checks_before_any_gpu_work():
    """Every error case returns before the handle is read: a block of zeros stands in for it."""
    L = capi.lib()
    nch, count, nscan, nsteps = 3, 4, 2, 2
    handle = C.create_string_buffer(1 << 16)
    p_ = lambda x: x.ctypes.data_as(C.c_void_p)
    E, D = np.zeros((nch, count)), np.zeros((2, count, count))
    ci, cf = np.array([0, 1], dtype=np.int32), np.array([1, 2], dtype=np.int32)
    field, a = np.zeros((nsteps, 6, 2, nscan), dtype=np.complex128), np.zeros((nscan, nch, count), dtype=np.complex128)
    snap, err, obs = np.zeros((2, nscan, nch, count), dtype=np.complex128), np.zeros(nscan), np.zeros((3, nscan, nch, 10))
    si, sf = np.array([0, 2], dtype=np.int32), np.array([0, 1], dtype=np.int32)
    sk, W = np.array([1, 0], dtype=np.int32), np.zeros((2, count, count))
    fidx = np.array([0, 1], dtype=np.int32)
    for fn in (L.bspatom_tdse_fields, L.bspatom_tdse_fields_dev):
        good = [C.addressof(handle), nch, count, p_(E), 2, p_(ci), p_(cf), p_(D), nscan, nsteps, 0.05, p_(field), p_(a), 1, p_(snap),
                p_(err), 1, p_(obs), 1, 2, p_(si), p_(sf), p_(sk), p_(W), 2, p_(fidx)]
        sub = lambda pos, v: [v if i == pos else x for i, x in enumerate(good)]
        for pos in (0, 3, 5, 6, 7, 11, 12):                        # p, E, ci, cf, D, field, a
            assert fn(*sub(pos, None)) == -2, pos
        for pos in (1, 2, 8):                                      # nch, count, nscan < 1
            assert fn(*sub(pos, 0)) == -2 and fn(*sub(pos, -1)) == -2, pos
        for pos in (9, 4, 13, 16):                                 # nsteps, npairs, snap_every, obs_every < 0
            assert fn(*sub(pos, -1)) == -2, pos
        assert fn(*sub(13, 0)) == -2                               # snap given with snap_every = 0
        assert fn(*sub(16, 0)) == -2                               # obs given with obs_every = 0
        assert fn(*sub(17, None)) == -2                            # obs_every >= 1 without obs
        for bad in (np.array([0, 3], dtype=np.int32), np.array([-1, 1], dtype=np.int32)):
            assert fn(*sub(5, p_(bad))) == -2 and fn(*sub(6, p_(bad))) == -2
        assert fn(*sub(5, p_(cf))) == -2                           # ci == cf stays an error for the driven pairs
        for bad in (float("nan"), float("inf")):
            assert fn(*sub(10, bad)) == -2
        for bad in (-1, 2):                                        # scheme outside {0, 1}
            assert fn(*sub(18, bad)) == -2
        assert fn(*sub(19, -1)) == -2                              # nstat < 0
        for pos in (20, 21, 22, 23):                               # nstat > 0 without si, sf, skind, W
            assert fn(*sub(pos, None)) == -2, pos
        for bad in (np.array([0, 3], dtype=np.int32), np.array([-1, 1], dtype=np.int32)):
            assert fn(*sub(20, p_(bad))) == -2 and fn(*sub(21, p_(bad))) == -2
        for bad in (np.array([1, 2], dtype=np.int32), np.array([-1, 0], dtype=np.int32)):
            assert fn(*sub(22, p_(bad))) == -2                     # skind outside {0, 1}
        # the two arguments of this call
        assert fn(*sub(24, 0)) == -2 and fn(*sub(24, -1)) == -2    # nfield < 1
        assert fn(*sub(24, 4)) == -5                               # more than BSPATOM_TDSE_MAX_FIELDS
        for bad in (np.array([0, 2], dtype=np.int32), np.array([-1, 1], dtype=np.int32)):
            assert fn(*sub(25, p_(bad))) == -2                     # fidx outside 0 .. nfield-1
        assert fn(*sub(24, 1)) == -2                               # the same fidx with one field: 1 is outside
        assert fn(*sub(25, None)) == -2                            # no fidx with two fields and pairs
