// resolvent_shared.h -- what the resolvent kernels (resolvent.hip, resolvent_coupled.hip, resolvent_wide.hip) share on the device: the
// zero-pivot rule and the reciprocal of a pivot, the way a right-hand side comes into a workgroup and a solution and its projections
// go out, the entry of the coupled matrix and the wave-level pieces of its pivot search.  (The one-wave LU and its substitutions,
// the forward pass that rc_solve runs among them, are band_lu_wave.h.)  One
// definition each, so that "resolvent.hip's form" and "as resolvent_coupled.hip" in the guarantees of include/bspatom.h (G2/G3,
// C1 - C6, K1 - K4) name code, not copies: the calls factor the same numbers and sum in the same order because they run the same
// statements.  (The one-wave kernels keep their own loads, stores and projections: through helpers they measured slower.)
#pragma once
#include "common.h"
#include "wave_ops.h"

namespace bsp {

constexpr int RS_PF = 8;                   // steps per prefetch block of the one-wave passes

// a wave's own global stores are complete before the pass that reads them through other lanes (eigvec.hip: y_sync<true>)
__device__ __forceinline__ void rs_sync() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// The zero-pivot threshold, invit_body's with |M_jj| measured by cabs1: dmax the largest diagonal entry, dflo the largest sum of the
// magnitudes of a diagonal entry's terms (what its rounding errors scale with when the terms cancel)
__device__ __forceinline__ double rs_pertol(double dmax, double dflo)
{
    return 2.220446049250313e-16 * fmax(fmax(dmax, 2.220446049250313e-16 * dflo), 1e-280);
}
// 1 / pivot, once per column: a pivot below the threshold is replaced by +-pertol and counted in nper; the reciprocal is scaled by
// cabs1, so that it neither overflows nor underflows.  (The replacement as selects: written as a branch it compiles to one, in the
// dependent chain of every step of the one-wave factorisation.)  The squared modulus states its fused product: the form every
// includer had compiled, with contraction on or off around it.
__device__ __forceinline__ double2 rs_pivot_recip(double pr, double pi, const double pertol, int &nper)
{
    const bool tiny = fabs(pr) + fabs(pi) < pertol;
    pr = tiny ? ((pr < 0.0) ? -pertol : pertol) : pr;
    pi = tiny ? 0.0 : pi;
    nper += tiny;
    const double sc = 1.0 / (fabs(pr) + fabs(pi));
    const double qr = pr * sc, qi = pi * sc;
    const double rd = 1.0 / __builtin_fma(qr, qr, qi * qi);
    return make_double2((qr * rd) * sc, -((qi * rd) * sc));
}

// ---- a right-hand side in, a solution and its projections out, for the coupled kernels' workgroups of NT threads: the caller's
// vectors are channel-major (entry e = c n + i), the matrix orders its unknowns basis index first (position i nch + c).  The
// caller's arrays are read and written as doubles: the ABI promises no more than their alignment.
template <int NT>
__device__ __forceinline__ void rc_load_rhs(const int n, const int nch, const double *B, double2 *y, const int tid)
{
    for (int e = tid; e < n * nch; e += NT) {
        const int c = e / n, i = e - c * n;
        y[i * nch + c] = make_double2(B[2 * e], B[2 * e + 1]);
    }
}
template <int NT>
__device__ __forceinline__ void rc_store_x(const int n, const int nch, const double2 *y, double *X, const int tid)
{
    for (int e = tid; e < n * nch; e += NT) {
        const int c = e / n, i = e - c * n;
        const double2 v = y[i * nch + c];
        X[2 * e] = v.x; X[2 * e + 1] = v.y;
    }
}
// R[q] = p_q^T y over all channels, q < nproj: bilinear, no conjugate; thread-strided partial sums in the caller's order, each
// wave's fixed tree, then the waves in ascending order.  red: NT / 64 words of LDS; called by the whole workgroup.
template <int NT>
__device__ __forceinline__ void rc_project(const int n, const int nch, const int nproj, const double *P0, const double2 *y, double *R,
                                           double2 *red, const int tid)
{
    const int N = n * nch, lane = tid & 63, wv = tid >> 6;
    for (int q = 0; q < nproj; ++q) {
        const double *P = P0 + (size_t)2 * q * N;
        double sr = 0.0, si = 0.0;
        for (int e = tid; e < N; e += NT) {
            const int c = e / n, i = e - c * n;
            const double2 xv = y[i * nch + c];
            const double pr = P[2 * e], pi = P[2 * e + 1];
            sr += pr * xv.x - pi * xv.y;
            si += pr * xv.y + pi * xv.x;
        }
        sr = wave_sum(sr); si = wave_sum(si);
        if (lane == 0) red[wv] = make_double2(sr, si);
        lds_barrier();
        if (tid == 0) {
            double tr = red[0].x, ti = red[0].y;
#pragma unroll
            for (int u = 1; u < NT / 64; ++u) { tr += red[u].x; ti += red[u].y; }
            R[2 * q] = tr; R[2 * q + 1] = ti;
        }
        lds_barrier();
    }
}

// ---- the coupled matrix
// The maximum over the 64 lanes of values that are >= 0 in lane 0 (wave_sum's scan with fmax: zeros shift in and change nothing)
__device__ __forceinline__ double rc_wave_max(double x)
{
    x = fmax(x, dpp_mov<0x111>(x)); x = fmax(x, dpp_mov<0x112>(x)); x = fmax(x, dpp_mov<0x114>(x)); x = fmax(x, dpp_mov<0x118>(x));
    return fmax(fmax(read_lane(x, 15), read_lane(x, 31)), fmax(read_lane(x, 47), read_lane(x, 63)));
}
// *p where ok, else zero: a guarded load, never a load through a selected address (that one is a FLAT load, whose wait drains the
// global loads and stores in flight as well)
__device__ __forceinline__ double2 rc_load(const double2 *p, bool ok)
{
    double2 v = make_double2(0.0, 0.0);
    if (ok) v = *p;
    return v;
}
// M(R, C), R = i nch + c, C = j nch + c2: channels, z and w of item `it`, coupling coefficients of item `ita` (the resolvent calls:
// ita = it; a time step: one record of channels, a coefficient set per step).  fl: the sum of the magnitudes of the terms (the
// pivot threshold's floor).
__device__ __forceinline__ void rc_entry(const ResolventCoupledArgs &a, int it, int ita, int R, int C, double &re, double &im, double &fl)
{
    re = 0.0; im = 0.0; fl = 0.0;
    const int n = a.n, b = a.k - 1, nch = a.nch;
    if (C < 0 || C >= n * nch) return;
    const int i = R / nch, c = R - i * nch, j = C / nch, c2 = C - j * nch;
    const int d = (i > j) ? (i - j) : (j - i);
    if (d > b) return;
    if (c == c2) {
        const int lo = (i > j) ? j : i, mc = it * nch + c;
        const double zr = a.z[2 * mc], zi = a.z[2 * mc + 1];
        const double s = a.SB[(size_t)d * n + lo], h = a.HB[((size_t)a.chan[mc] * a.k + d) * n + lo];
        re = h - zr * s;
        im = -(zi * s);
        fl = (fabs(h) + fabs(zr * s)) + fabs(zi * s);
        const int ws = a.w[mc];
        if (a.WB && ws >= 0) {
            const double wv = a.WB[((size_t)ws * (2 * b + 1) + (j - i + b)) * n + i];
            im -= wv;
            fl += fabs(wv);
        }
    }
    const size_t cs = (size_t)(2 * b + 1) * n;
    for (int p = 0; p < a.ncoup; ++p) {
        if (a.cr[p] != c || a.cc[p] != c2) continue;
        const size_t at = a.ctr[p] ? (size_t)(i - j + b) * n + j : (size_t)(j - i + b) * n + i;   // G(i, j), or G(j, i) for the transpose
        const double *co = a.acoef + ((size_t)ita * a.ncoup + p) * a.nop * 2;
        for (int o = 0; o < a.nop; ++o) {
            const double g = a.GB[(size_t)o * cs + at];
            re += co[2 * o] * g;
            im += co[2 * o + 1] * g;
            fl += (fabs(co[2 * o]) + fabs(co[2 * o + 1])) * fabs(g);
        }
    }
}

}  // namespace bsp
