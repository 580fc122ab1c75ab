"""Restatements of bspatom_spline_expect (csrc/spline_expect.hip, include/bspatom_spline_expect.h) for the tests:

    e(o) = sum_c conj(c_c)^T G_o (sum_c' B_o(c, c') c_c')

expect_ld: the definition on dense matrices in numpy.clongdouble, with the sum of the magnitudes of its leaf products
conj(c_c(i)) G_o(i, j) B_o(c, c') c_c'(j), what a rounding-error bound scales with.  expect_f64: the header's order of operations in
float64 NumPy -- element-wise IEEE operations, no FMA, no reassociation --, the lane-strided partial sums and the wave's tree
included.  Packets are (nch, n) complex; B (nexp, nch, nch); GE (nexp, 2k-1, n) full bands, GE[o, d + k - 1, i] = G_o(i, i + d)."""
import numpy as np

import resolvent_ref as ref


def expect_ld(c, B, GE):
    """(e (nexp,) clongdouble, sum |terms| (nexp,) float) of one packet"""
    c = np.asarray(c, dtype=np.complex128)
    nch, n = c.shape
    B = np.asarray(B, dtype=np.float64).reshape(-1, nch, nch)
    GE = np.asarray(GE, dtype=np.float64).reshape(B.shape[0], -1, n)
    cl = c.astype(np.clongdouble)
    al = np.abs(cl)
    e = np.zeros(B.shape[0], dtype=np.clongdouble)
    mag = np.zeros(B.shape[0])
    for o in range(B.shape[0]):
        Gl = np.asarray(ref.full_to_dense(GE[o]), dtype=np.longdouble)
        Ga = np.abs(Gl)
        Bl = B[o].astype(np.longdouble)
        u = Bl.astype(np.clongdouble) @ cl                                # (nch, n)
        e[o] = np.sum(np.conj(cl) * (u @ Gl.T))
        # sum over c, c', i, j of |c_c(i)| |G(i, j)| |B(c, c')| |c_c'(j)|
        mag[o] = float(np.sum(al * ((np.abs(Bl) @ al) @ Ga.T)))
    return e, mag


def wave_sum(x):
    """wave_ops.h's wave_sum of 64 lane values: the row scan with row_shr 1, 2, 4, 8 (zeros shift in), then (l15 + l31) + (l47 + l63)"""
    x = np.array(x, dtype=np.float64).reshape(4, 16)
    for s in (1, 2, 4, 8):
        sh = np.zeros_like(x)
        sh[:, s:] = x[:, :-s]
        x = x + sh
    return (x[0, 15] + x[1, 15]) + (x[2, 15] + x[3, 15])


def _lane_sums(t):
    """lane l adds t[l], t[l + 64], .. ascending, from +0.0"""
    n = t.shape[0]
    s = np.zeros(64)
    for i0 in range(0, n, 64):
        m = min(64, n - i0)
        s[:m] = s[:m] + t[i0:i0 + m]
    return s


def expect_f64(c, B, GE):
    """e (nexp,) complex128 of one packet in the header's order"""
    c = np.asarray(c, dtype=np.complex128)
    nch, n = c.shape
    B = np.asarray(B, dtype=np.float64).reshape(-1, nch, nch)
    GE = np.asarray(GE, dtype=np.float64).reshape(B.shape[0], -1, n)
    b = (GE.shape[1] - 1) // 2
    cr, ci = np.ascontiguousarray(c.real), np.ascontiguousarray(c.imag)
    e = np.zeros(B.shape[0], dtype=np.complex128)
    for o in range(B.shape[0]):
        er, ei = 0.0, 0.0
        for ch in range(nch):
            nz = [m for m in range(nch) if B[o, ch, m] != 0.0]
            if not nz:
                pr, pi = 0.0, 0.0
            else:
                ur, ui = np.zeros(n), np.zeros(n)
                for m in nz:
                    ur = ur + B[o, ch, m] * cr[m]
                    ui = ui + B[o, ch, m] * ci[m]
                yr, yi = np.zeros(n), np.zeros(n)
                for d in range(-b, b + 1):
                    lo, hi = max(0, -d), min(n, n - d)
                    if hi <= lo:
                        continue
                    g = GE[o, d + b, lo:hi]
                    yr[lo:hi] = yr[lo:hi] + g * ur[lo + d:hi + d]
                    yi[lo:hi] = yi[lo:hi] + g * ui[lo + d:hi + d]
                pr = wave_sum(_lane_sums(cr[ch] * yr + ci[ch] * yi))
                pi = wave_sum(_lane_sums(cr[ch] * yi - ci[ch] * yr))
            er, ei = er + pr, ei + pi
        e[o] = complex(er, ei)
    return e


def bound(n, nch, k, mag):
    """the accuracy bound of the tests: 2 (n + 2 nch + 2k + 4) eps sum |terms|"""
    return 2.0 * (n + 2 * nch + 2 * k + 4) * np.finfo(np.float64).eps * mag
