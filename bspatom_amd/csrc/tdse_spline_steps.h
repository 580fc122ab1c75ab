// tdse_spline_steps.h -- what a Crank-Nicolson step in the spline basis adds to a coupled solve, for a workgroup of NT threads: the
// right-hand side b = S c (ts_rhs), the row of an observed step from it (ts_row) and the update (ts_update).  Shared by
// tdse_spline_kernel (tdse_spline.hip, on resolvent_coupled_lu.h's LU) and tdse_spline_wide_kernel (tdse_spline_wide.hip, on
// resolvent_wide_lu.h's): rules 1 and 3 of include/bspatom_tdse_spline.h are one definition each.
#pragma once
#include "common.h"
#include "wave_ops.h"
#include "resolvent_shared.h"

namespace bsp {

// b = S c of one packet (c: [nch][n] complex as doubles, channel-major) into y at position i nch + ch.  S(i, j) from the problem's
// upper band SB[|d| n + min(i, j)], the band rc_entry reads; b_re, b_im start at +0.0 and add S(i, i + d) c(i + d) for d = -(k-1) ..
// k-1 ascending, columns outside 0 .. n-1 skipped; IEEE multiplies and adds, nothing contracted.  The whole workgroup.
template <int NT>
__device__ __forceinline__ void ts_rhs(const int n, const int nch, const int b, const double *__restrict__ SB, const double *c, double2 *y,
                                       const int tid)
{
#pragma clang fp contract(off)
    for (int e = tid; e < n * nch; e += NT) {
        const int ch = e / n, i = e - ch * n;
        const double *cc = c + (size_t)2 * ch * n;
        double br = 0.0, bi = 0.0;
        for (int d = -b; d <= b; ++d) {
            const int j = i + d;
            if (j < 0 || j >= n) continue;
            const double s = SB[(size_t)(d < 0 ? -d : d) * n + (d < 0 ? j : i)];
            br = br + s * cc[2 * j];
            bi = bi + s * cc[2 * j + 1];
        }
        y[i * nch + ch] = make_double2(br, bi);
    }
}

// The row of a packet from b = S c in y (visible to the workgroup): row[ch] = Re sum_i conj(c(i, ch)) b(i, ch) -- thread-strided
// partial sums over i ascending, each wave's fixed tree, the waves in ascending order --, then rc_project's p_r^T b, Re and Im,
// r < nproj.  red: NT / 64 words of LDS; the whole workgroup.
template <int NT>
__device__ __forceinline__ void ts_row(const int n, const int nch, const int nproj, const double *P, const double *c, const double2 *y,
                                       double *row, double2 *red, const int tid)
{
#pragma clang fp contract(off)
    const int lane = tid & 63, wv = tid >> 6;
    for (int ch = 0; ch < nch; ++ch) {
        const double *cc = c + (size_t)2 * ch * n;
        double s = 0.0;
        for (int i = tid; i < n; i += NT) {
            const double2 bv = y[i * nch + ch];
            s = s + (cc[2 * i] * bv.x + cc[2 * i + 1] * bv.y);
        }
        s = wave_sum(s);
        if (lane == 0) red[wv] = make_double2(s, 0.0);
        lds_barrier();
        if (tid == 0) {
            double t = red[0].x;
#pragma unroll
            for (int u = 1; u < NT / 64; ++u) t = t + red[u].x;
            row[ch] = t;
        }
        lds_barrier();
    }
    if (nproj > 0) rc_project<NT>(n, nch, nproj, P, y, row + nch, red, tid);
}

// c' = -(4 i / dt) x - c with g = 4 / dt: c'_re = g x_im - c_re, c'_im = -(g x_re) - c_im, one multiply and one subtract each, nothing
// contracted; x in y in the matrix's ordering.  snap (or null) takes a copy.  The whole workgroup.
template <int NT>
__device__ __forceinline__ void ts_update(const int n, const int nch, const double g, const double2 *y, double *c, double *snap, const int tid)
{
#pragma clang fp contract(off)
    for (int e = tid; e < n * nch; e += NT) {
        const int ch = e / n, i = e - ch * n;
        const double2 x = y[i * nch + ch];
        const double pr = g * x.y, pi = g * x.x;
        const double nr = pr - c[2 * e], ni = -pi - c[2 * e + 1];
        c[2 * e] = nr; c[2 * e + 1] = ni;
        if (snap) { snap[2 * e] = nr; snap[2 * e + 1] = ni; }
    }
}

}  // namespace bsp
