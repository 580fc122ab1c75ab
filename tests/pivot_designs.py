"""Designed matrices for the banded LU solvers (csrc/resolvent.hip, resolvent_coupled_lu.h, resolvent_wide.hip), built through the
PUBLIC arguments of the calls alone: couplings, G, a for the coupled calls, W / w for the single-channel call.  The physical matrices
of the other tests (H_l - i W - z S plus dipole couplings) pivot within about bw / 3 and fill U to about 1.15 bw; these reach what the
kernels are written for -- pivots at distance bw, rows of U that are 2 bw wide, pivots that are exactly zero:

  (A) swap pairs     a banded symmetric permutation of strength t max |M_base| on top of the physical matrix: unknown (i, c') of the
                     second half of a group of 2 (k-1) basis indices is tied to (i - (k-1), nch-1-c'), a displacement of bw - 2c in
                     the interleaved ordering.  Half of the columns pivot at distance >= bw - 2 (nch-1), the largest at bw exactly.
  (B) random blocks  every pair (cr, cc) coupled by random full bands with complex Gaussian coefficients, ten times the base.
  (C) integers       z = 0, no absorber, one l: the entry (c, c) with coefficient exactly 1 on the band of -H_l cancels the base
                     exactly (h - 0 s + 1 (-h) = 0), and small-integer bands with small-integer complex coefficients ARE the matrix;
                     the coefficients of a batch then zero one column, or two, of the same matrix: exactly singular.

A far pivot must also be NEEDED, or a kernel that never finds it goes unnoticed: on the plain physical base (z = 0.3) a search cut to
bw / 2 picks an entry of H - z S instead, and the LU it gets is only mildly unstable -- its backward error stayed under the 8 eps of the
tests' criterion on the k = 4 matrices of (A) and on nearly every matrix of (B) (band_lu_ref's mutant, measured: 0.03 .. 6.8 times eps).  So
(A) and (B) stand on the base at Im z = Y = 1e4, the matrix of a Crank-Nicolson step of 2e-4, which is -i Y S to four digits, and an
ERASER takes that part out on and below the diagonal: the overlap's lower band with the coefficient i Im z on the entries (c, c, 0)
(as -Y times it in W for the single-channel call) -- in the first halves' columns for (A), everywhere for (B), whose own bands are
also scaled by GRADE = 1e-6 within bw / 2 below the diagonal.  What a cut search finds there is 1e-4 or less of the rows it then
spreads: the mutant's backward error is 240 .. 5e5 eps on every matrix, against the criterion's 8.

Every builder returns a `system`: a dict of the call's own arguments (l, z (nmat, nch), w (nmat, nch) or None, couplings, G, a (nmat,
ncoup, nop); W (nabs, 2k-1, n) for the single-channel call).  The GPU call and dense() are given the same arrays.  The conditions the
designs must meet are asserted on LAPACK's factorisation in test_resolvent_pivots_cpu.py; the GPU cases are in
test_gpu_resolvent_pivots.py.

The split-step TDSE (csrc/tdse_split.hip) has its own one-wave LU and two kinds of matrix, both reached through bspatom_tdse_split's
public arguments at dt = SPLIT_DT = 2^-11, where everything the host derives is a power of two (4 / dt = 8192, dt / 2 = 2^-12):

  atomic   M_c = H_l - i W - (4i / dt) S is bspatom_resolvent's matrix at z = 8192 i: design (A) of the single-channel call goes into
           the call's absorbers, one per l (split_atomic).
  field    N_j = S + i (dt/2) f lam_j G.  With f = -2i / dt the factor is lam_j exactly, and lam_j = 1 makes N_j = S + G: G is (A)'s
           swap pairs at t max |S| minus the eraser of the first halves' columns, which then cancels exactly (split_field); f = +2i / dt
           puts the same matrix into the eigenchannel lam_j = -1.  A never is an argument: lam and Q are (SPLIT_LAM, split_q()).
  zeros    G = minus the columns j1 = n // 3 and j2 = 2n // 3 + 1 of S: N_j has two exactly zero columns where lam_j times the sign of
           -Im f is +1 and is regular elsewhere (split_singular).  The atomic matrix cannot be made singular through the public
           arguments (H_l cannot be cancelled), and which of two equal candidates becomes the pivot shows in the bits alone: no design
           asks for either.

split_system() puts them into the arguments of one call; test_tdse_split_pivots_cpu.py proves them, test_gpu_tdse_split_pivots.py
runs them."""
import numpy as np

import resolvent_ref as ref
import resolvent_coupled_ref as cref

# the grids of the GPU cases (test_gpu_resolvent._input / test_gpu_resolvent_wide._problem), as keyword arguments of capi.make_input
# and oracle.make_cfg
_LIN = dict(kind_grid=0, ra=0.0, l_fin=1, l_ini=0, n0_ini=1, zatom=1.0)
GRIDS = {"tiny8": dict(_LIN, rb=12.0, k=5, nfun=8), "n65_k4": dict(_LIN, rb=40.0, k=4, nfun=65),
         "lin256": dict(_LIN, rb=50.0, k=9, nfun=256), "k16_n40": dict(_LIN, rb=20.0, k=16, nfun=40),
         "k16_n20": dict(_LIN, rb=20.0, k=16, nfun=20), "k10_n65": dict(_LIN, rb=30.0, k=10, nfun=65)}
# k10_n65: b = 9, the kernels' instances for b <= 15 with rows of the register window unused
SINGLE_CASES = ["n65_k4", "lin256", "k10_n65", "k16_n40"]
NARROW_CASES = [("tiny8", 2), ("n65_k4", 3), ("lin256", 7), ("k16_n40", 4)]
WIDE_CASES = [("n65_k4", 17), ("k16_n20", 5), ("k16_n40", 9), ("k16_n40", 16)]
WIDE_C = [("n65_k4", 17), ("k16_n20", 5)]                      # the integer design on the two smaller wide cases
T_STRONG, T_WEAK = 20.0, 2.0                                   # (A): the pivot order guaranteed; the multipliers O(1)
# k16_n20: 20 functions of order 16 have an overlap of condition 1.3e8 by themselves; at t = 20 the designed matrix has 1.9e7, at 6 6.5e6
A_STRENGTHS = {"k16_n20": (6.0, T_WEAK)}
PHASE = 0.8 + 0.6j                                             # (A) on the coupled calls: a complex strength of modulus 1
Y = 1.0e4                                                      # Im z of the designs (A) and (B): the matrix of a Crank-Nicolson step of 2e-4
GRADE = 1.0e-6                                                 # (B): the factor on the bands' entries within bw // 2 below the diagonal


def base_scale(SB, HB, l, z, WB=None, w=None):
    """max |entry| of the uncoupled matrix: over the channels' blocks H_l - i W - z S"""
    s = 0.0
    for c in range(len(l)):
        Wc = WB if (WB is not None and (w is None or w[c] >= 0)) else None
        s = max(s, float(np.max(np.abs(ref.dense_matrix(SB, HB[l[c]], complex(z[c]), Wc)))))
    return s


def swap_rows(n, k):
    """the basis indices i tied to i - (k-1): the second halves of the complete groups of 2 (k-1) indices; where n holds no complete
    group (k16_n20), the one partial group's i >= k-1"""
    b = k - 1
    ng = n // (2 * b)
    if ng == 0:
        return np.arange(b, n)
    return np.concatenate([np.arange(2 * b * g + b, 2 * b * (g + 1)) for g in range(ng)])


def swap_bands(n, k):
    """(2, 2k-1, n) full bands of lo(i, i-(k-1)) = 1 and hi(i-(k-1), i) = 1 on swap_rows: lo + hi is a symmetric permutation's
    off-diagonal part"""
    b = k - 1
    rows = swap_rows(n, k)
    G = np.zeros((2, 2 * b + 1, n))
    G[0, 0, rows] = 1.0                                        # d = -(k-1) in row i
    G[1, 2 * b, rows - b] = 1.0                                # d = +(k-1) in row i - (k-1)
    return G


def full_band(UB, sign=1.0):
    """the full band (2k-1, n) of sign * the symmetric matrix whose upper band is UB (an index shuffle and a sign: exact)"""
    k, n = UB.shape
    F = np.zeros((2 * k - 1, n))
    for d in range(k):
        F[k - 1 + d, :n - d] = sign * UB[d, :n - d]
        F[k - 1 - d, d:] = sign * UB[d, :n - d]
    return F


def lower_overlap(SB, cols=None):
    """the full band of the overlap's entries S(i, j), i >= j (on and below the diagonal), of the columns `cols` (None: all) -- the
    eraser: with the coefficient i Im z on an entry (c, c, 0), or as -Im z times it in an absorber, it takes the part -i Im z S of the
    base out of those places and leaves the real part H_l - Re z S there, smaller by the factor Y"""
    k, n = SB.shape
    keep = np.ones(n, dtype=bool) if cols is None else np.isin(np.arange(n), cols)
    F = np.zeros((2 * k - 1, n))
    for d in range(k):                                         # S(j + d, j) is stored in row i = j + d at [k - 1 - d, i]
        j = np.arange(n - d)
        F[k - 1 - d, j + d] = np.where(keep[j], SB[d, j], 0.0)
    return F


def _base(nch, mats, y):
    """channels l = c % 2; per matrix (Re z of channel 0, absorber): channel c has Re z + 0.01 c (test_gpu_resolvent_coupled's rule)
    and Im z = y"""
    l = [c % 2 for c in range(nch)]
    z = np.array([[zb + 0.01 * c + 1j * y for c in range(nch)] for zb, _ in mats], dtype=np.complex128)
    w = np.array([[wm] * nch for _, wm in mats], dtype=np.int32)
    return l, z, w


def design_a(SB, HB, WB, nch, strengths=(T_STRONG, T_WEAK), phase=PHASE, mats=((0.3, -1), (-0.2, 0)), y=Y):
    """(A) on a coupled call: one matrix per strength; entries (nch-1-c, c, 0) on lo and (c, nch-1-c, 0) on hi, each with the
    coefficient t * phase * max |M_base| of its matrix; then the entries (c, c, 0) with i Im z on the eraser of the first halves'
    columns (module docstring).  mats: (Re z, absorber) per matrix.  y = 0: no eraser, a real base (the K3 test, with a real phase)."""
    k, n = SB.shape
    l, z, w = _base(nch, mats, y)
    couplings = [(nch - 1 - c, c, 0) for c in range(nch)] + [(c, nch - 1 - c, 0) for c in range(nch)] + [(c, c, 0) for c in range(nch)]
    a = np.zeros((len(mats), 3 * nch, 3), dtype=np.complex128)
    for m, t in enumerate(strengths):
        s = t * phase * base_scale(SB, HB, l, z[m], WB, w[m])
        a[m, :nch, 0] = s
        a[m, nch:2 * nch, 1] = s
        a[m, 2 * nch:, 2] = 1j * z[m].imag
    G = np.concatenate([swap_bands(n, k), lower_overlap(SB, swap_rows(n, k) - (k - 1))[None]])
    return dict(tag="A", l=l, z=z, w=w, couplings=couplings, G=G, a=a, what=["t=%g" % t for t in strengths])


def design_a_single(SB, HB, strengths=(T_STRONG, T_WEAK), mats=((0, 0.3), (1, -0.2)), y=Y):
    """(A) on the single-channel call: it goes into W, so into -i W as a large imaginary part (the pivot rule |Re| + |Im| sees it just
    the same).  Absorber m = t max |M_base| (lo + hi) - Im z * the eraser of the first halves' columns; mats: (l, Re z) per matrix."""
    k, n = SB.shape
    sw = swap_bands(n, k).sum(axis=0)
    l, z = [m[0] for m in mats], np.array([m[1] + 1j * y for m in mats], dtype=np.complex128)
    er = lower_overlap(SB, swap_rows(n, k) - (k - 1))
    W = np.stack([t * base_scale(SB, HB, [l[m]], [z[m]]) * sw - y * er for m, t in enumerate(strengths)])
    return dict(tag="A", l=l, z=z, w=list(range(len(mats))), W=W, what=["t=%g" % t for t in strengths])


def design_b(SB, HB, WB, nch, nop=3, strength=10.0, seed=1, mat=(0.3, 0), y=Y, grade=GRADE):
    """(B): all nch^2 pairs (cr, cc, 0) on nop random full bands, complex Gaussian coefficients times strength * max |M_base|; the
    bands' entries within bw // 2 below the diagonal, the diagonal included, scaled by `grade` (module docstring); the last operator is the eraser of every column, with the
    coefficient i Im z on the pairs (c, c)"""
    k, n = SB.shape
    rng = np.random.default_rng(1000 * seed + nch)
    l, z, w = _base(nch, [mat], y)
    near = ((nch * k - 1) // 2 + nch - 1) // nch               # i - j <= near: every entry within bw // 2 below the diagonal
    G = rng.standard_normal((nop, 2 * k - 1, n))
    for d in range(-(k - 1), k):                               # a full band is zero where i + d leaves the matrix
        G[:, d + k - 1, :max(0, -d)] = 0.0
        G[:, d + k - 1, n - max(0, d):] = 0.0
        if 0 <= -d <= near:
            G[:, d + k - 1] *= grade
    couplings = [(cr, cc, 0) for cr in range(nch) for cc in range(nch)]
    a = np.zeros((1, nch * nch, nop + 1), dtype=np.complex128)
    a[0, :, :nop] = strength * base_scale(SB, HB, l, z[0], WB, w[0]) * (rng.standard_normal((nch * nch, nop)) + 1j * rng.standard_normal((nch * nch, nop)))
    for c in range(nch):
        a[0, c * nch + c, nop] = 1j * z[0, c].imag
    return dict(tag="B", l=l, z=z, w=w, couplings=couplings, G=np.concatenate([G, lower_overlap(SB)[None]]), a=a, what=["nop=%d" % nop])


def design_c(SB, HB, nch, seed=1, lch=0):
    """(C): three matrices of one batch -- regular, one column zeroed, two separated columns zeroed.  Operators: -H_l (coefficient 1
    on the entries (c, c): the base cancels exactly), g1 and g4 (integers in -3 .. 3, the columns j1 and j2 empty), g2 = column j1
    alone and g3 = column j2 alone of the band g1 came from.  Coefficients: integer complex A1 on g1, g2, g3, A2 on g4, so the regular
    matrix is g (x) A1 + g4 (x) A2 in the interleaved ordering; the second matrix has coefficient 0 on g2 for the column channel c1
    (column (j1, c1) of the matrix is then zero and nothing else changes), the third also 0 on g3 for the column channel c2."""
    k, n = SB.shape
    rng = np.random.default_rng(2000 * seed + nch)
    ints = lambda shape: rng.integers(-3, 4, shape).astype(np.float64)
    g, g4 = ints((2 * k - 1, n)), ints((2 * k - 1, n))
    for d in range(-(k - 1), k):
        for q in (g, g4):
            q[d + k - 1, :max(0, -d)] = 0.0
            q[d + k - 1, n - max(0, d):] = 0.0
    g[k - 1] = np.where(g[k - 1] == 0.0, 2.0, g[k - 1])        # no zero on g's diagonal
    j1, j2 = n // 3, (2 * n) // 3 + 1
    c1, c2 = nch // 2, 0

    def column(j):
        """the band holding column j of g alone: entries g(i, j), stored at [j - i + k - 1, i]"""
        q = np.zeros_like(g)
        for i in range(max(0, j - (k - 1)), min(n, j + k)):
            q[j - i + k - 1, i] = g[j - i + k - 1, i]
        return q
    g2, g3 = column(j1), column(j2)
    g1 = g - g2 - g3
    for j in (j1, j2):
        for i in range(max(0, j - (k - 1)), min(n, j + k)):
            g4[j - i + k - 1, i] = 0.0
    cint = lambda: rng.integers(-2, 3, (nch, nch)) + 1j * rng.integers(-2, 3, (nch, nch))
    A1, A2 = cint(), cint()
    A1[np.arange(nch), np.arange(nch)] += 3.0                   # a diagonal that is not zero
    couplings = [(cr, cc, 0) for cr in range(nch) for cc in range(nch)]
    a = np.zeros((3, nch * nch, 5), dtype=np.complex128)
    for p, (cr, cc, _) in enumerate(couplings):
        a[:, p, 0] = 1.0 if cr == cc else 0.0
        a[:, p, 1:4] = A1[cr, cc]
        a[:, p, 4] = A2[cr, cc]
        if cc == c1:
            a[1:, p, 2] = 0.0
        if cc == c2:
            a[2, p, 3] = 0.0
    G = np.stack([full_band(HB[lch], -1.0), g1, g2, g3, g4])
    z = np.zeros((3, nch), dtype=np.complex128)
    return dict(tag="C", l=[lch] * nch, z=z, w=None, couplings=couplings, G=G, a=a, what=["regular", "one column", "two columns"],
                zero_columns=[(j1, c1), (j2, c2)])


def dense(sy, SB, HB, WB, m, dtype=np.complex128):
    """the channel-major dense matrix m of a coupled system, from the arrays the GPU call is given"""
    w = None if sy["w"] is None else sy["w"][m]
    Wb = WB[None] if (WB is not None and w is not None and np.any(np.asarray(w) >= 0)) else None
    return cref.dense_matrix(SB, HB, sy["l"], sy["z"][m], sy["couplings"], sy["G"], sy["a"][m], Wb, w if Wb is not None else None, dtype)


def dense_single(sy, SB, HB, m, dtype=np.complex128):
    """the dense matrix m of a single-channel system"""
    return ref.dense_matrix(SB, HB[sy["l"][m]], complex(sy["z"][m]), sy["W"][sy["w"][m]], dtype)


def interleaved(M, nch):
    """the matrix in the ordering that is factored: unknown (i, c) at position i nch + c"""
    idx = cref.interleave_index(nch, M.shape[0] // nch)
    return M[np.ix_(idx, idx)]


def coupled_systems(name, nch, SB, HB, WB, kinds):
    """the systems of a coupled case, in the order of `kinds` (a string of A, B, C); (C) alone: the regular matrix only is meant by
    the T1-style tests (matrix 0)"""
    out = []
    for kind in kinds:
        if kind == "A":
            out.append(design_a(SB, HB, WB, nch, strengths=A_STRENGTHS.get(name, (T_STRONG, T_WEAK))))
        elif kind == "B":
            out.append(design_b(SB, HB, WB, nch, nop=2 if nch >= 16 else 3))
        else:
            out.append(design_c(SB, HB, nch))
    return out


# ---- the split-step TDSE -------------------------------------------------------------------------------------------------------
SPLIT_DT = 2.0 ** -11
SPLIT_GRIDS = ["tiny8", "n65_k4", "lin256", "k10_n65", "k16_n40"]
SPLIT_VARIANTS = ["atomic", "field", "both"]
SPLIT_L, SPLIT_W = [0, 1, 0], [0, 1, -1]                       # the designed absorber m belongs to l = m; channel 2 stays physical
SPLIT_LAM = np.array([-1.0, 0.5, 1.0])                         # +-1: the designed eigenchannels of f = -+2i / dt; 0.5: the same bands at half the strength
SPLIT_NSTEPS, SPLIT_NSCAN = 2, 3
SPLIT_ZERO_GRIDS = ["n65_k4", "lin256", "k10_n65"]


def split_q():
    """a fixed orthogonal 3 x 3 matrix without a zero entry: the Q factor of a seeded Gaussian matrix"""
    Q = np.linalg.qr(np.random.default_rng(77).standard_normal((3, 3)))[0]
    assert np.min(np.abs(Q)) > 0.05
    return np.ascontiguousarray(Q)


def split_atomic(SB, HB, dt=SPLIT_DT):
    """(2, 2k-1, n): the absorbers that make M_c = H_l - i W_l - (4i / dt) S design (A) at t = 20 (l = 0) and t = 2 (l = 1)"""
    return design_a_single(SB, HB, mats=((0, 0.0), (1, 0.0)), y=4.0 / dt)["W"]


def split_field(SB, t=T_STRONG):
    """the band G with S + G = design (A) on the overlap: t max |S| (lo + hi) minus the eraser of the first halves' columns"""
    k, n = SB.shape
    return t * float(np.max(np.abs(SB))) * swap_bands(n, k).sum(axis=0) - lower_overlap(SB, swap_rows(n, k) - (k - 1))


def split_zero_columns(n):
    return n // 3, (2 * n) // 3 + 1


def split_singular(SB, cols=None):
    """the band G = minus the columns `cols` (None: both of split_zero_columns) of S's full band: S + G has those columns exactly
    zero, S - G and S + G / 2 are regular"""
    k, n = SB.shape
    F = full_band(SB)
    G = np.zeros_like(F)
    for j in (split_zero_columns(n) if cols is None else cols):
        for i in range(max(0, j - (k - 1)), min(n, j + k)):    # the entry (i, j) is stored at [j - i + k - 1, i]
            G[j - i + k - 1, i] = -F[j - i + k - 1, i]
    return G


def split_fields(dt=SPLIT_DT, nsteps=SPLIT_NSTEPS):
    """(nsteps, 3) complex: scan 0 f = -2i / dt (the factor of G is lam_j), scan 1 +2i / dt (-lam_j), scan 2 a real 0.5"""
    return np.ascontiguousarray(np.broadcast_to(np.array([-2j / dt, 2j / dt, 0.5]), (nsteps, 3)))


def split_packets(n, nch=3, nscan=SPLIT_NSCAN, seed=300):
    """(nscan, nch, n) complex Gaussian packets of norm about 1, the first real"""
    rng = np.random.default_rng(seed + n)
    c0 = (rng.standard_normal((nscan, nch, n)) + 1j * rng.standard_normal((nscan, nch, n))) / np.sqrt(n)
    c0[0] = c0[0].real
    return c0


def split_system(variant, SB, HB, RB, dt=SPLIT_DT):
    """The arguments of one bspatom_tdse_split call on three channels, two steps and three scans.  variant "atomic": the designed
    absorbers, G = RB (the band of r) and a real field U(0.2, 1) per step and scan (an imaginary f of size 2 / dt on the band of r
    would make S + lam r indefinite); "field": no absorber, G = split_field, f = split_fields; "both"; "zeros" / "zero": no absorber,
    G = split_singular with both columns / with column j2 alone, f = split_fields."""
    k, n = SB.shape
    designed_f = variant != "atomic"
    f = split_fields(dt) if designed_f else np.random.default_rng(400 + n).uniform(0.2, 1.0, (SPLIT_NSTEPS, SPLIT_NSCAN)).astype(np.complex128)
    if variant in ("zeros", "zero"):
        G = split_singular(SB, None if variant == "zeros" else split_zero_columns(n)[1:])
    else:
        G = split_field(SB) if designed_f else np.array(RB, dtype=np.float64)
    W = split_atomic(SB, HB, dt) if variant in ("atomic", "both") else None
    return dict(variant=variant, l=list(SPLIT_L), w=None if W is None else list(SPLIT_W), W=W, G=np.ascontiguousarray(G), Q=split_q(),
                lam=SPLIT_LAM.copy(), f=f, c0=split_packets(n), dt=dt, nsteps=SPLIT_NSTEPS)


def split_field_matrix(sy, SB, q, j, step=0):
    """the dense N_j of scan q at a step, as tests/tdse_split_ref.py forms it"""
    return ref.upper_to_dense(SB) + 0.5j * sy["dt"] * sy["f"][step, q] * sy["lam"][j] * ref.full_to_dense(sy["G"])
