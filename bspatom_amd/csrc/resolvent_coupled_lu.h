// resolvent_coupled_lu.h -- the workgroup-level banded LU of the coupled matrix (resolvent_coupled.hip's header comment describes it):
// the shape of the workgroup, the sizes of a slot's scratch and of its LDS, the assembly of the band into U's rows with the
// zero-pivot scale (rc_assemble), the factorisation (rc_factor) and the one-wave solve (rc_solve).  Shared by
// resolvent_coupled_kernel and tdse_spline_kernel (tdse_spline.hip), so that "bspatom_resolvent_coupled's matrix, factorisation and
// solve" in the guarantees of bspatom_tdse_spline (include/bspatom_tdse_spline.h, S3) names code, not a copy: a Crank-Nicolson step and a coupled
// solve with the same matrix run the same statements.
#pragma once
#include "common.h"
#include "wave_ops.h"
#include "resolvent_shared.h"
#include "band_lu_wave.h"
#include "../../include/bspatom.h"

namespace bsp {
constexpr int RC_BMAX = 63;                // BSPATOM_COUPLED_MAX_BAND: the pivot candidates of a column fit one wavefront
constexpr int RC_NT = 512;                 // threads of the workgroup
constexpr int RC_NW = RC_NT / 64;
constexpr int RC_PANEL = 1;                // columns per panel
constexpr int RC_PFB = 4;                  // steps per prefetch block of the solves' backward pass (two U entries per lane and step)
static_assert(RC_PANEL == 1, "the step below is one column");
static_assert(RC_BMAX == BSPATOM_COUPLED_MAX_BAND, "the limit the header states");

__host__ __device__ inline size_t rc_slot_doubles(int N, int bw)
{
    const size_t piv = ((size_t)N + 1) / 2;
    return 2 * ((size_t)N * (2 * bw + 1) + (size_t)N * bw + (size_t)N) + piv + (piv & 1);
}
// LDS of a workgroup: the window, the pivot row's copy (128), the multipliers (64), the reductions' words (16), complex each
__host__ __device__ inline size_t rc_lds_bytes(int bw) { return ((size_t)(bw + 1) * (2 * bw + 1) + 128 + 64 + 16) * sizeof(double2); }

// The band of item `it` (its z, w, channels; the coefficients of item `ita`), row by row, into U's rows, by the whole workgroup;
// returns the scale of the zero-pivot perturbation from its diagonal (rs_pertol) to every thread.  red: RC_NW words of LDS.  On
// return the band is in memory and visible to the workgroup.
__device__ __forceinline__ double rc_assemble(const ResolventCoupledArgs &a, const int it, const int ita, const int N, const int bw,
                                              double2 *U, double2 *red, const int tid)
{
    const int W = 2 * bw + 1, lane = tid & 63, wv = tid >> 6;
    double dmax = 0.0, dflo = 0.0;
    for (int r = wv; r < N; r += RC_NW)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int c = lane + 64 * h;
            if (c < W) {
                double re, im, fl;
                rc_entry(a, it, ita, r, r - bw + c, re, im, fl);
                U[(size_t)r * W + c] = make_double2(re, im);
                if (c == bw) { dmax = fmax(dmax, fabs(re) + fabs(im)); dflo = fmax(dflo, fl); }
            }
        }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) { dmax = fmax(dmax, __shfl_xor(dmax, off)); dflo = fmax(dflo, __shfl_xor(dflo, off)); }
    if (lane == 0) red[wv] = make_double2(dmax, dflo);
    __syncthreads();                                             // the band is in memory (vmcnt(0) and the barrier), red is written
#pragma unroll
    for (int q = 0; q < RC_NW; ++q) { dmax = fmax(dmax, red[q].x); dflo = fmax(dflo, red[q].y); }
    return rs_pertol(dmax, dflo);
}

// The factorisation P M = L U of the assembled band in U.  U: [N][2bw+1] complex, on entry row r = M(r, r-bw .. r+bw), on return
// row j = (1 / pivot, U(j, j+1 .. j+2bw)); Lm: [N][bw] multipliers; piv: [N] pivot rows.  Returns (in wave 0) the replaced pivots.
__device__ __forceinline__ int rc_factor(const int N, const int bw, const double pertol, double2 *U, double2 *Lm, int *piv, double2 *win,
                                         double2 *prow, double2 *mult, const int tid)
{
    const int W = 2 * bw + 1, RS = bw + 1, lane = tid & 63, wv = tid >> 6;
    // the window at step 0: rows 0 .. bw, columns 0 .. 2 bw
    for (int e = tid; e < RS * W; e += RC_NT) {
        const int r = e / W, C = e - r * W;
        win[e] = rc_load(U + (size_t)r * W + (C - r + bw), r < N && C <= r + bw);
    }
    // the loaders: thread lc of the last two waves holds entry lc of the rows that enter at an even step (ent0) and at an odd one
    // (ent1); a register is loaded again right after the window has taken it, two steps ahead of its next use, and never copied
    // (a copy would wait for the load)
    const int lc = tid - (RC_NT - 128);
    const bool loader = lc >= 0 && lc < W;
    double2 ent0 = rc_load(U + (size_t)(bw + 1) * W + lc, loader && bw + 1 < N);
    double2 ent1 = rc_load(U + (size_t)(bw + 2) * W + lc, loader && bw + 2 < N);
    lds_barrier();
    int nper = 0, rbase = 0, cb = 0;                               // j mod RS, j mod W
    auto step = [&](const int j, double2 &ent) {
        const int nrow = (N - 1 - j < bw) ? (N - 1 - j) : bw;
        if (wv == 0) {
            // pivot search: lane t holds M(j + t, j); ties go to the smallest row
            int s = rbase + (lane <= bw ? lane : 0);
            s = (s >= RS) ? s - RS : s;
            const double2 v = rc_load(win + s * W + cb, lane <= nrow);
            const double mag = (lane <= nrow) ? fabs(v.x) + fabs(v.y) : -1.0;
            const double mx = rc_wave_max(mag);
            const unsigned long long hit = __ballot(mag == mx);
            const int dp = __builtin_amdgcn_readfirstlane(hit ? __ffsll((long long)hit) - 1 : 0);
            const double v0r = read_lane(v.x, 0), v0i = read_lane(v.y, 0);
            const double2 rcp = rs_pivot_recip(read_lane(v.x, dp), read_lane(v.y, dp), pertol, nper);
            const double rr = rcp.x, ri = rcp.y;
            // rows j and j + dp change places: the row now at j + t, t >= 1, is the old row j where t == dp
            const double xr = (lane == dp) ? v0r : v.x, xi = (lane == dp) ? v0i : v.y;
            const bool below = lane >= 1 && lane <= nrow;
            const double2 lm = make_double2(below ? xr * rr - xi * ri : 0.0, below ? xr * ri + xi * rr : 0.0);
            mult[lane] = lm;
            if (lane >= 1 && lane <= bw) Lm[(size_t)j * bw + lane - 1] = lm;
            if (lane == 0) piv[j] = j + dp;
            int sp = rbase + dp;
            sp = (sp >= RS) ? sp - RS : sp;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int c = lane + 64 * h;
                if (c < W) {
                    int ci = cb + c;
                    ci = (ci >= W) ? ci - W : ci;
                    const double2 pv = win[sp * W + ci];
                    if (dp != 0) win[sp * W + ci] = win[rbase * W + ci];
                    prow[c] = pv;
                    U[(size_t)j * W + c] = make_double2((c == 0) ? rr : pv.x, (c == 0) ? ri : pv.y);
                }
            }
        }
        lds_barrier();
        // the trailing update: a wave per row, a lane per column; column j is eliminated and becomes column j + 2 bw + 1
        for (int t = 1 + wv; t <= nrow; t += RC_NW) {
            int s = rbase + t;
            s = (s >= RS) ? s - RS : s;
            const double2 lm = mult[t];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int c = lane + 64 * h;
                if (c < W) {
                    int ci = cb + c;
                    ci = (ci >= W) ? ci - W : ci;
                    const double2 av = win[s * W + ci];
                    const double2 pv = prow[c];
                    const double ur = lm.x * pv.x - lm.y * pv.y, ui = lm.x * pv.y + lm.y * pv.x;
                    win[s * W + ci] = make_double2((c == 0) ? 0.0 : av.x - ur, (c == 0) ? 0.0 : av.y - ui);
                }
            }
        }
        // row j + bw + 1 enters the slot row j has left: its columns j + 1 .. j + 2 bw + 1
        if (loader && j + bw + 1 < N) {
            int ci = cb + lc + 1;
            ci = (ci >= W) ? ci - W : ci;
            win[rbase * W + ci] = ent;
        }
        ent = rc_load(U + (size_t)(j + bw + 3) * W + lc, loader && j + bw + 3 < N);
        lds_barrier();
        rbase = (rbase + 1 == RS) ? 0 : rbase + 1;
        cb = (cb + 1 == W) ? 0 : cb + 1;
    };
    for (int j = 0; j < N; j += 2) {
        step(j, ent0);
        if (j + 1 < N) step(j + 1, ent1);                          // uniform
    }
    return nper;
}

// y <- U^-1 L^-1 P y in place on ONE wave (y: N complex in global memory, visible to the wave; xs: an LDS ring of 128 complex).
// Forward: wave_lu_forward (band_lu_wave.h), the pass of the one-wave kernels, lane i holds y[j + i], i <= bw <= 63.  Backward: x_j = (y_j - sum_{c=1..2bw} U[j][c]
// x_{j+c}) / pivot_j, the 2 bw unknowns behind j in the ring, lane l takes c = l and c = 64 + l, then the wave's fixed tree.
__device__ __forceinline__ void rc_solve(const int N, const int bw, const double2 *U, const double2 *Lm, const int *piv, double2 *y,
                                         double2 *xs, const int lane)
{
    wave_lu_forward<WaveLuArith>(N, bw, Lm, piv, y, lane);
    constexpr int PF = RC_PFB;
    const int W = 2 * bw + 1;
    xs[lane] = make_double2(0.0, 0.0); xs[lane + 64] = make_double2(0.0, 0.0);
    const bool in1 = lane >= 1 && lane <= 2 * bw, in2 = lane + 64 <= 2 * bw;
    double2 u1n[PF], u2n[PF], udn[PF];
#pragma unroll
    for (int u = 0; u < PF; ++u) {
        const int j = N - 1 - u;
        u1n[u] = (j >= 0 && in1) ? U[(size_t)j * W + lane] : make_double2(0.0, 0.0);
        u2n[u] = (j >= 0 && in2) ? U[(size_t)j * W + lane + 64] : make_double2(0.0, 0.0);
        udn[u] = (j >= 0) ? U[(size_t)j * W] : make_double2(0.0, 0.0);
    }
    double2 ybn = (lane < PF && N - 1 - lane >= 0) ? y[N - 1 - lane] : make_double2(0.0, 0.0);
    for (int j0 = N - 1; j0 >= 0; j0 -= PF) {
        double2 u1[PF], u2[PF], ru[PF];
        const double2 yb = ybn;
        ybn = (lane < PF && j0 - PF - lane >= 0) ? y[j0 - PF - lane] : make_double2(0.0, 0.0);
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            const int jn = j0 - u - PF;
            u1[u] = u1n[u]; u2[u] = u2n[u]; ru[u] = udn[u];
            u1n[u] = (jn >= 0 && in1) ? U[(size_t)jn * W + lane] : make_double2(0.0, 0.0);
            u2n[u] = (jn >= 0 && in2) ? U[(size_t)jn * W + lane + 64] : make_double2(0.0, 0.0);
            udn[u] = (jn >= 0) ? U[(size_t)jn * W] : make_double2(0.0, 0.0);
        }
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            const int j = j0 - u;
            if (j >= 0) {
                double sr = 0.0, si = 0.0;
                if (in1 && j + lane < N) {
                    const double2 x = xs[(j + lane) & 127];
                    sr = u1[u].x * x.x - u1[u].y * x.y;
                    si = u1[u].x * x.y + u1[u].y * x.x;
                }
                if (in2 && j + lane + 64 < N) {
                    const double2 x = xs[(j + lane + 64) & 127];
                    sr += u2[u].x * x.x - u2[u].y * x.y;
                    si += u2[u].x * x.y + u2[u].y * x.x;
                }
                sr = wave_sum(sr); si = wave_sum(si);
                const double dr = read_lane(yb.x, u) - sr, di = read_lane(yb.y, u) - si;
                const double2 x = make_double2(dr * ru[u].x - di * ru[u].y, dr * ru[u].y + di * ru[u].x);
                if (lane == 0) { xs[j & 127] = x; y[j] = x; }
                __builtin_amdgcn_wave_barrier();
            }
        }
    }
    rs_sync();
}

}  // namespace bsp
