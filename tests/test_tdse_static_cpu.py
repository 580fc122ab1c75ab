"""bspatom_tdse_static without a GPU: the NumPy restatement tests/tdse_static_ref.py against the restatements it is built on, against
closed forms and against its own rows; the host helpers; the entry points, their kernels in the library, and the argument checks that
return before any GPU work."""
import ctypes as C
import os
import sys
import numpy as np
import pytest
from conftest import ROOT

import tdse_lawson_ref
import tdse_ref
import tdse_static_ref
from bspatom_amd import capi, host

EPS = tdse_ref.EPS
NAMES = ("bspatom_tdse_static", "bspatom_tdse_static_dev")


def same(x, y):
    """the same values with the same signs of zero (the bytes of a long double include padding: not compared)"""
    x, y = np.asarray(x), np.asarray(y)
    if x.shape != y.shape or x.dtype != y.dtype:
        return False
    parts = lambda z: (z.real, z.imag) if np.iscomplexobj(z) else (z,)
    return all(np.array_equal(u, v) and np.array_equal(np.signbit(u), np.signbit(v)) for u, v in zip(parts(x), parts(y)))


# ---- the restatement ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rd,cd", [(np.float64, np.complex128), (np.longdouble, np.clongdouble)])
def test_no_static_blocks_is_the_restatements_it_is_built_on(rd, cd):
    E, pairs, D, a0, field = tdse_ref.system(3, 5, 2, 12)
    for scheme, ref in ((0, tdse_ref), (1, tdse_lawson_ref)):
        want = ref.propagate(E, pairs, D, a0, field, 0.05, rd, cd, snap_every=4)
        for static in (None, ([], [], np.zeros((0, 5, 5)))):
            got = tdse_static_ref.propagate(E, pairs, D, a0, field, 0.05, static=static, scheme=scheme, rdtype=rd, cdtype=cd, snap_every=4)
            assert len(got) == 3 and all(same(g, w) for g, w in zip(got, want)), scheme
        a, err, obs = tdse_static_ref.propagate(E, pairs, D, a0, field, 0.05, scheme=scheme, rdtype=rd, cdtype=cd, obs_every=5)
        assert same(a, want[0]) and same(err, want[1])
        assert obs.shape == (4, 2, 3, 6) and np.all(obs[..., 4:] == 0.0) and obs.dtype == rd


def damped(nsteps, T=8.0):
    """Two channels of three states, no pairs, one diagonal kind-1 block diag(gamma) per channel: a(T) = a0 exp(-(i E + gamma) T)"""
    E = np.array([[-0.5, 0.1, 0.4], [0.3, 0.7, 1.0]])
    gamma = np.array([[0.1, 0.2, 0.3], [0.05, 0.15, 0.25]])
    a0 = np.array([[[0.5, 0.3j, -0.2], [0.4j, 0.5, 0.1 + 0.4j]]])
    static = ([(0, 0), (1, 1)], [1, 1], np.stack([np.diag(gamma[0]), np.diag(gamma[1])]))
    exact = a0 * np.exp(-(1j * E + gamma) * T)[None]
    return E, a0, static, np.zeros((nsteps, 6, 1), dtype=np.complex128), T / nsteps, exact


def test_diagonal_absorber_against_the_closed_form():
    """The long-double runs approach a0 exp(-(i E + gamma) t) at 5th order: from 50 to 100 steps the error of the plain scheme drops
    by 24 .. 40, the window of test_order_and_error_estimate (2^5 = 32).  The Lawson run, whose free phases are exact, converges too."""
    errs = {0: [], 1: []}
    for nsteps in (50, 100):
        E, a0, static, field, dt, exact = damped(nsteps)
        for scheme in (0, 1):
            a, est = tdse_static_ref.propagate(E, [], np.zeros((0, 3, 3)), a0, field, dt, static=static, scheme=scheme,
                                               rdtype=np.longdouble, cdtype=np.clongdouble)
            errs[scheme].append(float(np.max(np.abs(a - exact))))
            assert float(est[0]) > 0.0
    print("damped: plain errors %s ratio %.3g; lawson errors %s ratio %.3g"
          % (errs[0], errs[0][0] / errs[0][1], errs[1], errs[1][0] / errs[1][1]))
    assert 24.0 <= errs[0][0] / errs[0][1] <= 40.0
    assert errs[0][1] < 1e-7 and errs[1][1] < errs[1][0] < 1e-6
    # the population decays exactly as exp(-2 gamma t): the absorber's sign
    assert np.all(np.abs(exact) < np.abs(damped(1)[1]))


def test_diagonal_kind0_block_is_a_shift_of_the_energies():
    """E and delta on a grid of 1/64, so that E + delta is exact: the plain scheme with the block diag(delta) per channel and the plain
    scheme with E + delta integrate the same equation; the complex128 run of the former lies within the project's bound of the
    long-double run of the latter."""
    E, pairs, D, a0, field = tdse_ref.system(3, 7, 2, 40)
    rng = np.random.default_rng(3)
    E = np.round(E * 64.0) / 64.0
    delta = rng.integers(-32, 33, size=E.shape) / 64.0
    static = ([(c, c) for c in range(3)], [0, 0, 0], np.stack([np.diag(d) for d in delta]))
    r128, rlong = tdse_ref.both(E + delta, pairs, D, a0, field, 0.05)
    a, err = tdse_static_ref.propagate(E, pairs, D, a0, field, 0.05, static=static, scheme=0)
    along, errl = tdse_static_ref.propagate(E, pairs, D, a0, field, 0.05, static=static, scheme=0, rdtype=np.longdouble, cdtype=np.clongdouble)
    ba = tdse_ref.amp_bound(r128[0], rlong[0])
    da = float(np.max(np.abs(a.astype(np.clongdouble) - rlong[0])))
    dl = float(np.max(np.abs(along - rlong[0])))
    print("shift: |a_128(static) - a_long(E + delta)| / bound = %.3g, long against long %.3g eps" % (da / ba, dl / EPS))
    assert da <= ba and dl <= ba
    assert float(np.max(np.abs(err.astype(np.longdouble) - rlong[1]))) <= tdse_ref.err_bound(r128[1], rlong[1], 0.05)
    assert float(np.max(np.abs(a - tdse_ref.propagate(E, pairs, D, a0, field, 0.05)[0]))) > 1e-2          # the shift is felt


def test_norm_rate_on_the_rows():
    """d norm/dt = 2 sum_c Im s_c: the rows of a fine long-double run (dt = 0.01, every step) against the five-point central difference
    of their own norm.  Its error is dt^4 |N^(5)| / 30; every time derivative of the norm costs a factor of at most 2 ||H|| < 8 here
    (||E|| <= 2, the driven and static blocks below 1 each), the rate itself is below 2 ||W|| = 1: under 1e-8 8^4 / 30 = 1.4e-6."""
    for scheme in (0, 1):
        E, pairs, D, a0, field = tdse_ref.system(3, 6, 2, 60, dt=0.01)
        static = tdse_static_ref.static_system(3, 6)
        a, err, obs = tdse_static_ref.propagate(E, pairs, D, a0, field, 0.01, static=static, scheme=scheme, rdtype=np.longdouble,
                                                cdtype=np.clongdouble, obs_every=1)
        assert obs.shape == (61, 2, 3, 6)
        N = obs[..., 0].sum(axis=-1)
        rate = 2.0 * obs[..., 5].sum(axis=-1)
        fd = (N[:-4] - 8.0 * N[1:-3] + 8.0 * N[3:-1] - N[4:]) / (12.0 * np.longdouble(0.01))
        d = float(np.max(np.abs(fd - rate[2:-2])))
        print("norm rate, scheme %d: |five-point difference - 2 sum Im s| = %.3g (rates %.3g .. %.3g)"
              % (scheme, d, float(rate.min()), float(rate.max())))
        assert d <= 1.4e-6
        assert float(np.max(np.abs(rate))) > 1e-2
        # the Hermitian kind-0 terms (H in-channel, X with X^T) move no norm: only the kind-1 blocks are in the rate
        sp, sk, W = static
        only1 = ([p for p, k in zip(sp, sk) if k], [1] * sum(sk), W[np.array(sk) == 1])
        o1 = tdse_static_ref.observables(E, pairs, D, only1, a, np.longdouble, np.clongdouble)
        assert float(np.max(np.abs(o1[..., 5].sum(-1) - obs[-1, ..., 5].sum(-1)))) <= 64 * EPS


def test_rows_against_a_triple_loop():
    """Small integers: every sum is exact.  s_c from the definition written as loops, both kinds, in-channel and cross-channel."""
    rng = np.random.default_rng(11)
    E = rng.integers(-3, 4, size=(2, 3)).astype(np.float64)
    W = rng.integers(-3, 4, size=(3, 3, 3)).astype(np.float64)
    a = (rng.integers(-3, 4, size=(2, 2, 3)) + 1j * rng.integers(-3, 4, size=(2, 2, 3))).astype(np.complex128)
    spairs, skind = [(0, 0), (0, 1), (1, 1)], [1, 0, 1]
    got = tdse_static_ref.observables(E, [], np.zeros((0, 3, 3)), (spairs, skind, W), a)
    want = np.zeros((2, 2), dtype=np.complex128)
    for q in range(2):
        for j, (i, f) in enumerate(spairs):
            for n in range(3):
                for m in range(3):
                    want[q, f] += np.conj(a[q, f, m]) * (-1j if skind[j] else 1.0) * W[j, n, m] * a[q, i, n]
    assert got.shape == (2, 2, 6) and np.array_equal(got[..., 4], want.real) and np.array_equal(got[..., 5], want.imag)
    M = tdse_static_ref.static_magnitudes((spairs, skind, W), a)
    assert M.shape == (2,) and np.all(np.abs(got[..., 4:]).reshape(-1, 2).max(axis=0) <= M)


# ---- the host helpers -----------------------------------------------------------------------------------------------------
def test_cap_profile_rates_and_yield():
    r = np.array([0.5, 2.0, 3.0, 4.5])
    assert np.array_equal(host.cap_profile(r, 2.0, 0.5), np.array([0.0, 0.0, 0.5, 0.5 * 2.5 ** 2]))
    assert np.array_equal(host.cap_profile(r, 2.0, 2.0, power=3), np.array([0.0, 0.0, 2.0, 2.0 * 2.5 ** 3]))
    obs = np.zeros((5, 2, 3, 6))
    t = np.arange(5) * 0.2
    obs[..., 5] = -0.5 * (1.0 + t)[:, None, None] * np.array([1.0, 2.0, 0.0])[None, None, :] * np.array([1.0, 3.0])[None, :, None]
    rates = host.tdse_static_rates(obs)
    assert rates.shape == (5, 2, 3) and np.array_equal(rates, 2.0 * obs[..., 5])
    # the trapezoid is exact for a linear rate: the integral of (1 + t) over 0 .. 0.8 is 1.12
    y = host.tdse_yield(obs, 0.1, 8, 2)
    assert y.shape == (2, 3)
    assert np.allclose(y, 1.12 * np.array([[1.0, 2.0, 0.0], [3.0, 6.0, 0.0]]), rtol=1e-14, atol=0)
    assert np.array_equal(host.tdse_yield(obs[:1], 0.1, 0, 1), np.zeros((2, 3)))
    with pytest.raises(ValueError):
        host.tdse_yield(obs, 0.1, 9, 2)                      # obs_every does not divide nsteps
    with pytest.raises(ValueError):
        host.tdse_yield(obs, 0.1, 8, 0)
    with pytest.raises(ValueError):
        host.tdse_yield(obs, 0.1, 10, 2)                     # six rows belong to that run, not five
    with pytest.raises(ValueError):
        host.tdse_static_rates(obs[..., :4])                 # the rows of tdse_observe have no static entries


def test_absorber_is_one_operator_matrix_call():
    class Fake:
        calls = []

        def quadrature(self):
            r = np.linspace(0.5, 9.5, 10)
            return r, np.full(10, 1.0)

        def operator_matrix(self, pairs, G, deriv, n0_ini, count_ini, n0_fin, count_fin, a):
            self.calls.append((list(pairs), np.array(G), np.array(deriv), n0_ini, count_ini, n0_fin, count_fin, np.array(a)))
            return np.arange(len(pairs) * count_ini * count_fin, dtype=np.float64).reshape(len(pairs), count_ini, count_fin)

    p = Fake()
    g = lambda r: host.cap_profile(r, 6.0, 0.1)
    spairs, skind, W = host.tdse_absorber(p, [(0, 0), (1, 0), (2, 0)], 2, 4, g)
    assert len(p.calls) == 1
    pairs, G, deriv, n0i, ci, n0f, cf, a = p.calls[0]
    assert pairs == [(0, 0), (1, 1), (2, 2)] and (n0i, ci, n0f, cf) == (2, 4, 2, 4) and not deriv.any()
    assert np.array_equal(G[0], g(p.quadrature()[0])) and G.shape == (1, 10)
    assert spairs == [(0, 0), (1, 1), (2, 2)] and list(skind) == [1, 1, 1] and W.shape == (3, 4, 4)
    # an array on the quadrature grid serves as well
    host.tdse_absorber(p, [(1, 0)], 1, 2, g(p.quadrature()[0]))
    assert len(p.calls) == 2 and np.array_equal(p.calls[1][1], G)


# ---- the library ----------------------------------------------------------------------------------------------------------
def test_entry_points_bound():
    L = capi.lib()
    header = open(os.path.join(ROOT, "include", "bspatom.h")).read()
    for name in NAMES:
        assert name in capi.EXPORTS
        assert hasattr(L, name)
        assert len(getattr(L, name).argtypes) == 24
        assert getattr(L, name).argtypes[:18] == L.bspatom_tdse_observe.argtypes
        assert hasattr(capi.Problem, name[len("bspatom_"):])
        assert "int %s(" % name in header
    assert len(L.bspatom_tdse_lawson.argtypes) == 18 and len(L.bspatom_tdse_propagate.argtypes) == 16


def test_kernels_in_library_without_scratch_or_spills():
    """Six stages x two schemes on the narrow tile, the observing stage 0 in both schemes, the reduction to rows of 6"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import codeobj_notes
    ks = codeobj_notes.kernels(os.path.join(ROOT, "bspatom_amd", "libbspatom.so"))
    want = {"tdse_static_stage_kernel": 12, "tdse_static_observe_kernel": 2, "tdse_obs_reduce6_kernel": 1}
    for key, num in want.items():
        hits = [v for name, v in ks.items() if key in name]
        assert len(hits) == num, (key, [n for n in ks if "tdse" in n])
        for v in hits:
            assert (v["private_segment_fixed_size"] or 0) == 0, (key, v)
            assert (v["vgpr_spill_count"] or 0) == 0, (key, v)


def test_argument_checks_before_any_gpu_work():
    """Every BSPATOM_ERR_ARG case returns before the handle is read: a block of zeros stands in for it."""
    L = capi.lib()
    nch, count, nscan, nsteps = 3, 4, 2, 2
    handle = C.create_string_buffer(1 << 16)
    p_ = lambda x: x.ctypes.data_as(C.c_void_p)
    E, D = np.zeros((nch, count)), np.zeros((2, count, count))
    ci, cf = np.array([0, 1], dtype=np.int32), np.array([1, 2], dtype=np.int32)
    field, a = np.zeros((nsteps, 6, nscan), dtype=np.complex128), np.zeros((nscan, nch, count), dtype=np.complex128)
    snap, err, obs = np.zeros((2, nscan, nch, count), dtype=np.complex128), np.zeros(nscan), np.zeros((3, nscan, nch, 6))
    si, sf = np.array([0, 2], dtype=np.int32), np.array([0, 1], dtype=np.int32)
    sk, W = np.array([1, 0], dtype=np.int32), np.zeros((2, count, count))
    for fn in (L.bspatom_tdse_static, L.bspatom_tdse_static_dev):
        good = [C.addressof(handle), nch, count, p_(E), 2, p_(ci), p_(cf), p_(D), nscan, nsteps, 0.05, p_(field), p_(a), 1, p_(snap),
                p_(err), 1, p_(obs), 1, 2, p_(si), p_(sf), p_(sk), p_(W)]
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
        assert fn(*sub(5, p_(cf))) == -2                           # ci == cf stays an error for the DRIVEN pairs
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
