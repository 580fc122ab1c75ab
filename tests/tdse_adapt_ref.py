"""NumPy restatement of bspatom_tdse_adaptive (include/bspatom.h).

Three parts are exact or comparison-only arithmetic and are restated in float64 to be compared BIT FOR BIT with the library:
    the controller     decide / advance / controller: the rule on (n, m, j) from the estimate e and tol
    the stage times    stage_x, stage_times: x_s = ldexp(j + c_s, -m), t_s = t0 + dt (n + x_s)
    the field          hermite: the cubic Hermite interpolant of the node table, IEEE multiplies and adds in the header's order
The run itself, `run`, steps tdse_static_ref.propagate (one step of size h = ldexp(dt, -m) per accepted step, its (1, 6, nscan) table
from `hermite`) in a real / complex dtype of the caller's choice, either under its own controller or along a GIVEN sequence of
attempts (the device's log): the tests run it in complex128 and in long double as the other TDSE tests do.  Nothing here calls the
library."""
import numpy as np

import tdse_ref
import tdse_static_ref

C64 = np.array([float(c) for c in tdse_ref.C], dtype=np.float64)          # the doubles nearest 0, 2/9, 1/3, 3/4, 1, 5/6
MAX_LEVEL = 16


# ---- the controller -------------------------------------------------------------------------------------------------------------
def decide(e, tol, m, max_level):
    """flag of an attempt at level m with estimate e: 1 accepted, 2 forced, 0 rejected.  A NaN compares false: forced or rejected."""
    if e <= tol:
        return 1
    return 2 if m == max_level else 0


def advance(n, m, j, flag, e, tol):
    """the state after an attempt (n, m, j) with decision flag and estimate e"""
    if flag == 0:
        return n, m + 1, 2 * j
    j += 1
    if e <= tol * 0.015625 and m > 0 and j % 2 == 0:
        m, j = m - 1, j >> 1
    if j == (1 << m):
        n, j = n + 1, 0
    return n, m, j


def controller(nsteps, tol, max_level, level0, estimate):
    """Drive the rule with estimate(n, m, j) -> e until n == nsteps: the list of attempts (n, m, j, flag, e)."""
    assert 0 <= level0 <= max_level <= MAX_LEVEL
    n, m, j = 0, level0, 0
    log = []
    while n < nsteps:
        e = estimate(n, m, j)
        flag = decide(e, tol, m, max_level)
        log.append((n, m, j, flag, e))
        n, m, j = advance(n, m, j, flag, e, tol)
    return log


def stats_of(log, tol, level0=0):
    """stats[6] of a list of attempts (n, m, j, flag, e, ..): accepted, rejected, forced, deepest level, level at the end, attempts"""
    acc = sum(1 for r in log if r[3] > 0)
    end = advance(*log[-1][:5], tol)[1] if log else level0
    return [acc, len(log) - acc, sum(1 for r in log if r[3] == 2), max([r[1] for r in log], default=0), end, len(log)]


def follows_rule(log_i, log_e, tol, max_level, level0, nsteps=None):
    """Every decision and every state of a log (rows (n, m, j, flag), estimates per scan) follows from the rule, exactly.  Returns the
    state after the last logged attempt."""
    n, m, j = 0, level0, 0
    for (ln, lm, lj, lf), eq in zip(np.asarray(log_i).tolist(), np.asarray(log_e)):
        assert (ln, lm, lj) == (n, m, j), ((ln, lm, lj), (n, m, j))
        e = np.max(eq)
        assert lf == decide(e, tol, m, max_level), (lf, e, tol, m)
        n, m, j = advance(n, m, j, lf, e, tol)
    if nsteps is not None:
        assert (n, j) == (nsteps, 0)
    return n, m, j


# ---- times and the field ----------------------------------------------------------------------------------------------------------
def stage_x(m, j):
    """x_s = ldexp((double) j + c_s, -m), the six stage positions inside the coarse step"""
    return np.ldexp(np.float64(j) + C64, -int(m))


def stage_times(t0, dt, n, m, j):
    return np.float64(t0) + np.float64(dt) * (np.float64(n) + stage_x(m, j))


def hermite(fn, dt, nsub, n, x):
    """fn complex (nsteps * nsub + 1, 2, nscan), x (6,) in [0, 1] of coarse step n: complex (6, nscan) in the header's order of
    operations, float64, nothing fused (NumPy's elementwise float64 operations are single IEEE operations)."""
    fn = np.asarray(fn, dtype=np.complex128)
    x = np.asarray(x, dtype=np.float64)
    xs = x * np.float64(nsub)
    il = np.minimum(np.floor(xs).astype(np.int64), nsub - 1)
    u = (xs - il.astype(np.float64))[:, None]
    hf = np.float64(dt) / np.float64(nsub)
    omu = 1.0 - u
    omu2 = omu * omu
    u2 = u * u
    h00 = (1.0 + 2.0 * u) * omu2
    h10 = u * omu2
    h01 = u2 * (3.0 - 2.0 * u)
    h11 = u2 * (u - 1.0)
    i = n * nsub + il

    def part(v0, d0, v1, d1):
        return ((h00 * v0 + (h10 * hf) * d0) + h01 * v1) + (h11 * hf) * d1

    re = part(fn[i, 0].real, fn[i, 1].real, fn[i + 1, 0].real, fn[i + 1, 1].real)
    im = part(fn[i, 0].imag, fn[i, 1].imag, fn[i + 1, 0].imag, fn[i + 1, 1].imag)
    return re + 1j * im


def fused_u(nsub, m, j):
    """u as ONE rounding of x_s nsub - i_loc (what a contracted multiply-subtract would give), from exact rational arithmetic: the
    tests use it to show that their nsub tells the documented two roundings from the fused one"""
    from fractions import Fraction
    x = stage_x(m, j)
    il = np.minimum(np.floor(x * np.float64(nsub)).astype(np.int64), nsub - 1)
    return np.array([float(Fraction(float(xv)) * nsub - int(iv)) for xv, iv in zip(x, il)])


def plain_u(nsub, m, j):
    """u as the header defines it: rn(rn(x_s nsub) - i_loc)"""
    xs = stage_x(m, j) * np.float64(nsub)
    return xs - np.minimum(np.floor(xs).astype(np.int64), nsub - 1).astype(np.float64)


def attempt_field(fn, dt, nsub, n, m, j):
    """the (6, nscan) field values of the attempt (n, m, j): log_f's entry"""
    return hermite(fn, dt, nsub, n, stage_x(m, j))


# ---- the run ------------------------------------------------------------------------------------------------------------------------
def run(E, pairs, D, a0, fn, dt, nsub, static, scheme, tol, max_level, level0=0, rdtype=np.float64, cdtype=np.complex128, sequence=None,
        snap_every=0):
    """sequence None: the run under its own controller, the estimate taken in rdtype.  sequence = rows (n, m, j, flag): the accepted
    steps of that sequence, whatever this arithmetic would have decided.  Returns (a, err, log[, snaps]); log rows (n, m, j, flag, e,
    tol) with e the largest estimate over the scans, err (nscan,) the maximum over accepted steps per scan."""
    fn = np.asarray(fn, dtype=np.complex128)
    nsteps = (fn.shape[0] - 1) // nsub
    a = np.asarray(a0).astype(cdtype)
    err = np.zeros(a.shape[0], dtype=rdtype)
    log, snaps = [], []

    def attempt(a, n, m, j):
        f = attempt_field(fn, dt, nsub, n, m, j)[None]
        return tdse_static_ref.propagate(E, pairs, D, a, f, np.ldexp(np.float64(dt), -m), static=static, scheme=scheme, rdtype=rdtype,
                                         cdtype=cdtype)

    def accepted(a1, e1, n, n1):
        nonlocal a, err
        a, err = a1, np.maximum(err, e1)
        if snap_every and n1 != n and n1 % snap_every == 0:
            snaps.append(a.copy())

    if sequence is None:
        n, m, j = 0, level0, 0
        while n < nsteps:
            a1, e1 = attempt(a, n, m, j)
            e = np.max(e1)
            flag = decide(e, tol, m, max_level)
            log.append((n, m, j, flag, e, tol))
            n1, m1, j1 = advance(n, m, j, flag, e, tol)
            if flag:
                accepted(a1, e1, n, n1)
            n, m, j = n1, m1, j1
    else:
        seq = [tuple(int(v) for v in r[:4]) for r in sequence]
        for t, (n, m, j, flag) in enumerate(seq):
            if not flag:
                continue
            a1, e1 = attempt(a, n, m, j)
            log.append((n, m, j, flag, np.max(e1), tol))
            # a coarse step ends where the next attempt of the sequence belongs to another one (or the sequence ends)
            n1 = seq[t + 1][0] if t + 1 < len(seq) else n + 1
            accepted(a1, e1, n, n1)
    out = (a, err, log)
    return out + (np.array(snaps),) if snap_every else out


def margins(log):
    """the smallest relative distance of an estimate of the log from tol and from tol / 64"""
    worst = np.inf
    for n, m, j, flag, e, tol in log:
        for thr in (tol, tol * 0.015625):
            worst = min(worst, abs(float(e) - thr) / thr)
    return worst


def fixed_run(E, pairs, D, a0, fn, dt, nsub, static, scheme, level, rdtype=np.longdouble, cdtype=np.clongdouble):
    """the run in 2^level equal steps per coarse step (tol = +inf would coarsen: the sequence is given instead)"""
    nsteps = (np.asarray(fn).shape[0] - 1) // nsub
    seq = [(n, level, j, 1) for n in range(nsteps) for j in range(1 << level)]
    return run(E, pairs, D, a0, fn, dt, nsub, static, scheme, np.inf, level, level, rdtype, cdtype, sequence=seq)


# ---- the test system ------------------------------------------------------------------------------------------------------------------
# tdse_static_ref's system (tdse_ref.system's E, D, a0 with static_system's blocks) on NSTEPS coarse steps of DT, under a sin^2 pulse over
# the whole run whose middle is strong enough to send the controller down and whose ends let it come back.  TOL and AMP were
# chosen on the long-double restatement (tests/test_tdse_adapt_cpu.py holds them to it): every configuration of the GPU tests shows a
# rejection, a coarsening and three levels, one forced step at least with MAX_LEVEL_FORCED, and every estimate keeps a relative distance
# of 1e-3 at least from tol and tol / 64, so that the decisions do not depend on the last bits of an estimate.
NSTEPS, NSUB, DT, T0 = 4, 2, 0.4, 0.0
MAX_LEVEL_TEST, MAX_LEVEL_FORCED, LEVEL0 = 3, 1, 1
OMEGA = 1.1
TOL, AMP = 1e-5, 4.0
SHAPES = [(2, 1, 1), (3, 17, 8), (3, 15, 9), (4, 65, 3)]


def pulse(amp, phase=0.0, T=NSTEPS * DT):
    """(f, df/dt) of amp sin^2(pi t / T) cos(OMEGA t) exp(i phase)"""
    ph = np.exp(1j * phase)
    w = np.pi / T

    def f(t):
        return amp * np.sin(w * t) ** 2 * np.cos(OMEGA * t) * ph

    def df(t):
        return amp * (w * np.sin(2 * w * t) * np.cos(OMEGA * t) - OMEGA * np.sin(w * t) ** 2 * np.sin(OMEGA * t)) * ph

    return f, df


def node_table(amps, phase=0.0, nsub=NSUB):
    """fn (NSTEPS * nsub + 1, 2, nscan) of the pulses with the amplitudes amps"""
    t = T0 + np.arange(NSTEPS * nsub + 1, dtype=np.float64) * (DT / nsub)
    fn = np.zeros((len(t), 2, len(amps)), dtype=np.complex128)
    for q, amp in enumerate(amps):
        f, df = pulse(amp, phase)
        fn[:, 0, q], fn[:, 1, q] = f(t), df(t)
    return fn


def adapt_system(nch, count, nscan, blocks=True, nsub=NSUB):
    """(E, pairs, D, a0, fn, static) of a GPU test configuration, scan q driven with AMP (1 + 0.05 q); (3, 17, 8) runs with the field
    times exp(0.3 i).  blocks = False: the same system without its static blocks.  nsub: the node intervals per coarse step of fn."""
    E, pairs, D, a0, _ = tdse_ref.system(nch, count, nscan, NSTEPS, dt=DT)
    phase = 0.3 if (nch, count, nscan) == (3, 17, 8) else 0.0
    fn = node_table(AMP * (1.0 + 0.05 * np.arange(nscan)), phase, nsub)
    static = tdse_static_ref.static_system(nch, count) if blocks else None
    return E, pairs, D, a0, fn, static


def features(log):
    """(rejections, coarsenings, distinct levels, forced steps) of a list of attempts (n, m, j, flag, ..)"""
    rej = sum(1 for r in log if r[3] == 0)
    coarsen = sum(1 for x, y in zip(log, log[1:]) if x[3] > 0 and y[1] < x[1])
    return rej, coarsen, len({r[1] for r in log}), sum(1 for r in log if r[3] == 2)
