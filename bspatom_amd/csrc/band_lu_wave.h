// band_lu_wave.h -- the pivoted complex banded LU of ONE wavefront and its two substitutions, one definition for every kernel that
// runs them: resolvent.hip (resolvent_kernel, resolvent_chain_kernel), tdse_split.hip (tsplit_factor_kernel, tsplit_atomic_kernel,
// tsplit_field_kernel), spline_window.hip (spline_window_kernel) and, for the forward pass, resolvent_coupled_lu.h::rc_solve.  This is eigvec.hip::invit_body's method for a
// complex matrix: the row window in registers, multipliers and the pivot row by readlane, the window moved by a one-lane DPP
// shift, the entering row fetched RS_PF steps ahead, no LDS and no barrier in the n dependent steps.
//
// Arithmetic: pivot by |Re| + |Im| (LAPACK's cabs1), ties to the smallest row; one reciprocal per pivot (rs_pivot_recip), kept in
// U's diagonal slot; a complex product is the four-product form.  Every function body with arithmetic here is compiled with
// contraction OFF (the pragma is scoped to the body: at file scope it would reach the code of whoever includes this), and every
// multiply-add is written out: which product of a sum of two is fused is an Arith policy's statement, not the compiler's choice by
// the code around the call.  The callers' bits (G2/G3, C1 - C6 of include/bspatom.h; P1 - P3 of
// include/bspatom_tdse_split.h) are these forms; DESIGN.md 4.7 "Fused products" has the table and where they come from.
#pragma once
#include "common.h"
#include "wave_ops.h"
#include "resolvent_shared.h"

namespace bsp {

// ---- the arithmetic policies.  a (x) b below is the rounded product; fma(a, b, c) rounds once.
// What every caller computes alike:
// (by itself a complete policy for wave_lu_forward alone, which is how rc_solve uses it)
struct WaveLuArith {
    // multiplier l = x r (x the entry below the pivot, r the pivot's reciprocal)
    static __device__ __forceinline__ void multiplier(double xr, double xi, double rr, double ri, double &lr, double &li)
    {
#pragma clang fp contract(off)
        lr = __builtin_fma(xr, rr, -(xi * ri));
        li = __builtin_fma(xr, ri, xi * rr);
    }
    // forward substitution, w -= l y
    static __device__ __forceinline__ void forward(double lr, double li, double yr, double yi, double &wr, double &wi)
    {
#pragma clang fp contract(off)
        wr = wr - __builtin_fma(lr, yr, -(li * yi));
        wi = wi - __builtin_fma(li, yr, lr * yi);
    }
    // solution x = d r (d the reduced right-hand side, r the pivot's reciprocal)
    static __device__ __forceinline__ void solution(double dr, double di, double rr, double ri, double &xr, double &xi)
    {
#pragma clang fp contract(off)
        xr = __builtin_fma(dr, rr, -(di * ri));
        xi = __builtin_fma(dr, ri, di * rr);
    }
};
// resolvent.hip's forms: the ones its kernels have computed since they exist, read off their compiled code
struct WaveLuResolvent : WaveLuArith {
    // row update of window row t, a[t] -= l a[0] where `on`, else zero: the product with one fused multiply-add per component, then a
    // subtraction.  The statements work on the rows in place with the subtraction INSIDE the conditional, as resolvent.hip always had
    // them: handed the entries by value, or with the difference formed in front of the select, the compiler gathers the readlanes of
    // a step's multipliers ahead of the updates and keeps 32 to 60 more scalar registers in vector lanes, and resolvent_chain_kernel
    // measured 2.5 to 3 % slower.
    template <int N>
    static __device__ __forceinline__ void update(bool on, double lr, double li, double (&ar)[N], double (&ai)[N], int t)
    {
#pragma clang fp contract(off)
        ar[t] = on ? ar[t] - __builtin_fma(lr, ar[0], -(li * ai[0])) : 0.0;
        ai[t] = on ? ai[t] - __builtin_fma(lr, ai[0], li * ar[0]) : 0.0;
    }
    // backward substitution's term s = u x of step `step` of a block of RS_PF: the imaginary part fuses x.re u.im ... in the first step
    // of a block and the other product in the other seven
    static __device__ __forceinline__ void term(int step, double ur, double ui, double xr, double xi, double &sr, double &si)
    {
#pragma clang fp contract(off)
        sr = __builtin_fma(ur, xr, -(ui * xi));
        si = (step == 0) ? __builtin_fma(ur, xi, ui * xr) : __builtin_fma(ui, xr, ur * xi);
    }
    // the maximum over the wave, in every lane
    static __device__ __forceinline__ double wave_max(double x)
    {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) x = fmax(x, __shfl_xor(x, off));
        return x;
    }
};
// tdse_split.hip's forms
struct WaveLuSplit : WaveLuArith {
    // a[t] -= l a[0] where `on`, else zero: four fused multiply-adds, formed in FRONT of the selects as tdse_split.hip always had them
    // (inside them tsplit_field_kernel<8> takes 191 registers for 164 and loses a wave per SIMD)
    template <int N>
    static __device__ __forceinline__ void update(bool on, double lr, double li, double (&ar)[N], double (&ai)[N], int t)
    {
#pragma clang fp contract(off)
        const double nr = __builtin_fma(li, ai[0], __builtin_fma(-lr, ar[0], ar[t]));
        const double ni = __builtin_fma(-li, ar[0], __builtin_fma(-lr, ai[0], ai[t]));
        ar[t] = on ? nr : 0.0;
        ai[t] = on ? ni : 0.0;
    }
    static __device__ __forceinline__ void term(int, double ur, double ui, double xr, double xi, double &sr, double &si)
    {
#pragma clang fp contract(off)
        sr = __builtin_fma(ur, xr, -(ui * xi));
        si = __builtin_fma(ur, xi, ui * xr);
    }
    static __device__ __forceinline__ double wave_max(double x) { return rc_wave_max(x); }
};

// The factorisation P M = L U of one matrix by one wavefront.  e: the matrix, e.entry(r, c, re, im) = M(r, c), zero outside the band
// and the matrix, and e.diag(j, mag, flo) = |M(j,j)| by cabs1 and the sum of the magnitudes of its terms (rs_pertol).  U: [n][2b+1]
// complex, row j = (1 / pivot, U(j, j+1 .. j+2b)); Lm: [n][b] complex multipliers; piv: [n] pivot rows.  b <= BT.  Returns the number
// of pivots that were replaced by pertol.
template <int BT, class Arith, class Entry>
__device__ __forceinline__ int wave_lu_factor(const int n, const int b, const Entry &e, double2 *U, double2 *Lm, int *piv, const int lane)
{
#pragma clang fp contract(off)
    constexpr int PF = RS_PF;
    // scale of the zero-pivot perturbation (rs_pertol)
    double dmax = 0.0, dflo = 0.0;
    for (int j = lane; j < n; j += 64) {
        double mag, flo;
        e.diag(j, mag, flo);
        dmax = fmax(dmax, mag);
        dflo = fmax(dflo, flo);
    }
    dmax = Arith::wave_max(dmax); dflo = Arith::wave_max(dflo);
    const double pertol = rs_pertol(dmax, dflo);

    // lane c (0 .. 2 b) holds column j + c of the rows j .. j + b: a[t] = M(j + t, j + c)
    double ar[BT + 1], ai[BT + 1];
#pragma unroll
    for (int t = 0; t <= BT; ++t) {
        ar[t] = 0.0; ai[t] = 0.0;
        if (t <= b && lane <= 2 * b) e.entry(t, lane, ar[t], ai[t]);
    }
    // the row that enters at step j (row j + b + 1), one entry per lane and step, requested a block of PF steps ahead
    double per[PF], pei[PF], pnr[PF], pni[PF];
#pragma unroll
    for (int u = 0; u < PF; ++u) {
        pnr[u] = 0.0; pni[u] = 0.0;
        if (lane <= 2 * b) e.entry(u + b + 1, u + 1 + lane, pnr[u], pni[u]);
    }
    int nper = 0;
    for (int j = 0; j < n; ++j) {
        if ((j & (PF - 1)) == 0) {
#pragma unroll
            for (int u = 0; u < PF; ++u) {
                per[u] = pnr[u]; pei[u] = pni[u];
                pnr[u] = 0.0; pni[u] = 0.0;
                if (lane <= 2 * b) e.entry(j + PF + u + b + 1, j + PF + u + 1 + lane, pnr[u], pni[u]);
            }
        }
        const int nrow = (n - 1 - j < b) ? (n - 1 - j) : b;       // rows below the pivot row
        // pivot search down lane 0's registers (column j); ties go to the smallest row
        double mxv = fabs(ar[0]) + fabs(ai[0]);
        int dpl = 0;
#pragma unroll
        for (int t = 1; t <= BT; ++t) {
            const double v = (t <= nrow) ? fabs(ar[t]) + fabs(ai[t]) : -1.0;
            if (v > mxv) { mxv = v; dpl = t; }
        }
        const int dp = __builtin_amdgcn_readfirstlane(dpl);
        if (dp != 0) {                                               // uniform: rows j and j + dp change places, in every column
#pragma unroll
            for (int t = 1; t <= BT; ++t)
                if (t == dp) {
                    const double t1 = ar[0], t2 = ai[0];
                    ar[0] = ar[t]; ai[0] = ai[t]; ar[t] = t1; ai[t] = t2;
                }
        }
        const double2 rcp = rs_pivot_recip(read_lane(ar[0], 0), read_lane(ai[0], 0), pertol, nper);
        const double rr = rcp.x, ri = rcp.y;
        double lmr = 0.0, lmi = 0.0;                                 // this lane's multiplier (row j + lane), for the store
#pragma unroll
        for (int t = 1; t <= BT; ++t) {
            double ltr, lti;
            Arith::multiplier(read_lane(ar[t], 0), read_lane(ai[t], 0), rr, ri, ltr, lti);
            ltr = (t <= nrow) ? ltr : 0.0;
            lti = (t <= nrow) ? lti : 0.0;
            lmr = (lane == t) ? ltr : lmr;
            lmi = (lane == t) ? lti : lmi;
            Arith::update(lane >= 1, ltr, lti, ar, ai, t);           // columns j + 1 .. j + 2 b; column j is eliminated
        }
        if (lane == 0) piv[j] = j + dp;
        if (lane <= 2 * b) U[(size_t)j * (2 * b + 1) + lane] = (lane == 0) ? make_double2(rr, ri) : make_double2(ar[0], ai[0]);
        if (lane >= 1 && lane <= b) Lm[(size_t)j * b + lane - 1] = make_double2(lmr, lmi);
        // slide the window: row j leaves, row j + b + 1 enters; column j leaves, column j + 2 b + 1 enters (zero above the entering row)
        double pinr = per[0], pini = pei[0];
#pragma unroll
        for (int u = 1; u < PF; ++u) {
            pinr = ((j & (PF - 1)) == u) ? per[u] : pinr;
            pini = ((j & (PF - 1)) == u) ? pei[u] : pini;
        }
#pragma unroll
        for (int t = 0; t < BT; ++t) { ar[t] = dpp_mov<0x130>(ar[t + 1]); ai[t] = dpp_mov<0x130>(ai[t + 1]); }   // wave_shl:1
        ar[BT] = 0.0; ai[BT] = 0.0;
#pragma unroll
        for (int t = 0; t <= BT; ++t)
            if (t == b) { ar[t] = pinr; ai[t] = pini; }              // uniform
    }
    return nper;
}

// y <- L^-1 P y in place on ONE wave (y: n complex in global memory, visible to the wave; Lm: [n][b] multipliers, piv: [n] pivot
// rows, b <= 63): invit_body's forward pass, lane i holds y[j + i], the b + 1 entries a step can touch in a register window, what
// enters it requested a block ahead.  On return the result is visible to every lane.
template <class Arith>
__device__ __forceinline__ void wave_lu_forward(const int n, const int b, const double2 *Lm, const int *piv, double2 *y, const int lane)
{
#pragma clang fp contract(off)
    constexpr int PF = RS_PF;
    double wr = 0.0, wi = 0.0;
    if (lane <= b && lane < n) { const double2 v = y[lane]; wr = v.x; wi = v.y; }
    double2 lvn[PF]; int pvn[PF];
#pragma unroll
    for (int u = 0; u < PF; ++u) {
        lvn[u] = (u < n && lane >= 1 && lane <= b) ? Lm[(size_t)u * b + lane - 1] : make_double2(0.0, 0.0);
        pvn[u] = (u < n) ? piv[u] : 0;
    }
    // the entering entries: one per lane (lane u: step u's), a block ahead; above every index this pass has written
    double2 yln = (lane < PF && lane + b + 1 < n) ? y[lane + b + 1] : make_double2(0.0, 0.0);
    for (int j0 = 0; j0 < n; j0 += PF) {
        double2 lv[PF]; int pvv[PF];
        const double2 yl = yln;
        yln = (lane < PF && j0 + PF + lane + b + 1 < n) ? y[j0 + PF + lane + b + 1] : make_double2(0.0, 0.0);
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            const int jn = j0 + u + PF;
            lv[u] = lvn[u]; pvv[u] = pvn[u];
            lvn[u] = (jn < n && lane >= 1 && lane <= b) ? Lm[(size_t)jn * b + lane - 1] : make_double2(0.0, 0.0);
            pvn[u] = (jn < n) ? piv[jn] : 0;
        }
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            const int j = j0 + u;
            if (j < n) {
                const int p = __builtin_amdgcn_readfirstlane(pvv[u]);
                if (p != j) {                                    // uniform: rows j and p change places (p - j <= b: inside the window)
                    const double t0r = read_lane(wr, 0), t0i = read_lane(wi, 0);
                    const double tqr = read_lane(wr, p - j), tqi = read_lane(wi, p - j);
                    wr = lane == 0 ? tqr : (lane == p - j ? t0r : wr);
                    wi = lane == 0 ? tqi : (lane == p - j ? t0i : wi);
                }
                const double yr = read_lane(wr, 0), yi = read_lane(wi, 0);
                const int nrow = (n - 1 - j < b) ? (n - 1 - j) : b;
                if (lane >= 1 && lane <= nrow) Arith::forward(lv[u].x, lv[u].y, yr, yi, wr, wi);
                if (lane == 0) y[j] = make_double2(yr, yi);
                wr = dpp_mov<0x130>(wr); wi = dpp_mov<0x130>(wi);  // wave_shl:1 -- lane i takes lane i + 1
                const double er = read_lane(yl.x, u), ei = read_lane(yl.y, u);
                if (lane == b) { wr = er; wi = ei; }
            }
        }
    }
    rs_sync();
}

// y <- U^-1 L^-1 P y in place (y: n complex in global memory, the slot's): wave_lu_forward, then the backward pass
// x_j = (y_j - sum_{c=1..2b} U[j][c] x_{j+c}) / pivot_j with lane c holding x[j + c] (zero beyond the matrix), the 2 b entries a step
// can touch in a register window, what enters it requested a block ahead.  The caller has made y visible (rs_sync); on return the
// solution is visible to every lane.
template <class Arith>
__device__ __forceinline__ void wave_lu_solve(const int n, const int b, const double2 *U, const double2 *Lm, const int *piv, double2 *y,
                                              const int lane)
{
#pragma clang fp contract(off)
    wave_lu_forward<Arith>(n, b, Lm, piv, y, lane);
    constexpr int PF = RS_PF;
    const int w = 2 * b + 1;
    double wr = 0.0, wi = 0.0;
    double2 uvn[PF], udn[PF];
#pragma unroll
    for (int u = 0; u < PF; ++u) {
        const int j = n - 1 - u;
        uvn[u] = (j >= 0 && lane >= 1 && lane <= 2 * b) ? U[(size_t)j * w + lane] : make_double2(0.0, 0.0);
        udn[u] = (j >= 0) ? U[(size_t)j * w] : make_double2(0.0, 0.0);
    }
    double2 ybn = (lane < PF && n - 1 - lane >= 0) ? y[n - 1 - lane] : make_double2(0.0, 0.0);
    for (int j0 = n - 1; j0 >= 0; j0 -= PF) {
        double2 uv[PF], ru[PF];
        const double2 yb = ybn;
        ybn = (lane < PF && j0 - PF - lane >= 0) ? y[j0 - PF - lane] : make_double2(0.0, 0.0);
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            const int jn = j0 - u - PF;
            uv[u] = uvn[u]; ru[u] = udn[u];
            uvn[u] = (jn >= 0 && lane >= 1 && lane <= 2 * b) ? U[(size_t)jn * w + lane] : make_double2(0.0, 0.0);
            udn[u] = (jn >= 0) ? U[(size_t)jn * w] : make_double2(0.0, 0.0);
        }
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            const int j = j0 - u;
            if (j >= 0) {
                double sr = 0.0, si = 0.0;
                if (lane >= 1 && lane <= 2 * b && j + lane < n) Arith::term(u, uv[u].x, uv[u].y, wr, wi, sr, si);
                sr = wave_sum32(sr); si = wave_sum32(si);
                const double dr = read_lane(yb.x, u) - sr, di = read_lane(yb.y, u) - si;
                double xr, xi;
                Arith::solution(dr, di, ru[u].x, ru[u].y, xr, xi);
                if (lane == 0) y[j] = make_double2(xr, xi);
                wr = dpp_mov<0x138>(wr); wi = dpp_mov<0x138>(wi);  // wave_shr:1 -- lane i takes lane i - 1
                if (lane == 1) { wr = xr; wi = xi; }
            }
        }
    }
    rs_sync();
}

}  // namespace bsp
