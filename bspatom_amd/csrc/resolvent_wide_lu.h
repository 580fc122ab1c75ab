// resolvent_wide_lu.h -- the workgroup-level BLOCKED banded LU of the coupled matrix for wide bands (resolvent_wide.hip's header comment
// describes it): the shape of the workgroup, the size of a slot's scratch, the LDS layout, the assembly of the band in ZGBTRF's
// column layout with the zero-pivot scale (rw_assemble, rw_pertol), the loop over panels with the forward elimination of the
// right-hand sides (rw_factor) and the block back-substitution (rw_backsolve).  Shared by resolvent_wide_kernel and
// tdse_spline_wide_kernel (tdse_spline_wide.hip), so that "bspatom_resolvent_coupled_wide's matrix, factorisation and solve" in the
// guarantees of bspatom_tdse_spline_wide (include/bspatom_tdse_spline.h, S3) names code, not a copy: a Crank-Nicolson step and a wide
// coupled solve with the same matrix run the same statements.
#pragma once
#include "common.h"
#include "wave_ops.h"
#include "resolvent_shared.h"
#include "../../include/bspatom.h"

namespace bsp {
constexpr int RW_BMAX = 255;               // BSPATOM_COUPLED_WIDE_MAX_BAND: the candidates of a column fit four wavefronts
constexpr int RW_NT = 512;                 // threads of the workgroup
constexpr int RW_NW = RW_NT / 64;
constexpr int RW_NB = 16;                  // columns of a panel: the 16 x 16 x 4 instruction, four k-steps
constexpr int RW_CW = 256;                 // columns of a chunk of the trailing update
static_assert(RW_BMAX == BSPATOM_COUPLED_WIDE_MAX_BAND, "the limit the header states");
static_assert(RW_BMAX + 1 <= 4 * 64 && 2 * RW_BMAX <= RW_NT && RW_BMAX + 2 * RW_NB + 1 <= RW_NT, "a thread per candidate, per row, per column");

// LDS is laid out for the limit, whatever bw is: 512 threads at up to 256 registers are one workgroup per CU anyway, and constant
// strides make every unrolled LDS access an immediate offset.
constexpr int RW_PS = RW_BMAX + 2 * RW_NB + 1;   // rows of a panel column: bw + NB, and up to 15 zero rows for the last row tile (288)
// scratch of a slot: the band [N][3bw+1] and nrhs vectors [N], complex
__host__ __device__ inline size_t rw_slot_doubles(int N, int bw, int nrhs) { return 2 * ((size_t)N * (3 * bw + 1) + (size_t)nrhs * N); }
// LDS of a workgroup: the panel and the chunk of U12 (two planes each), the window of y, the block solutions of eight right-hand
// sides, the words of the pivot search and of the projections; then the permutation, the pivots and the displaced rows (ints)
constexpr size_t RW_LDS_DOUBLES = (size_t)2 * RW_NB * RW_PS + (size_t)2 * RW_NB * RW_CW + 2 * RW_PS + 2 * RW_NW * RW_NB + 16 + 2 * RW_NW;
constexpr size_t RW_LDS_BYTES = RW_LDS_DOUBLES * sizeof(double) + (size_t)(RW_PS + 3 * RW_NB + 4) * sizeof(int);
static_assert(RW_LDS_BYTES <= 160 * 1024, "the LDS of a CU");

// The pointers into the dynamic LDS, carved once per kernel and passed BY VALUE (the phases are inlined: the pointers stay constants
// of the kernel, not a struct in memory)
struct RwLds {
    double *Pre, *Pim, *Ure, *Uim;             // the panel [NB][PS] and the chunk of U12 [NB][CW], real and imaginary planes
    double2 *ywin, *xs;                        // the window of y [PS]; the block solutions [NW][NB]
    double *red;                               // the pivot search: (maximum, row, Re, Im) of four waves
    double2 *pred;                             // NW words of the workgroup reductions (the pivot scale, rc_project, ts_row)
    int *perm, *ipiv, *dpos, *dsrc, *ndp;      // the panel's permutation [PS], its pivots, the displaced rows [NB] each, their count
};
__device__ __forceinline__ RwLds rw_lds_layout(double *base)
{
    RwLds L;
    L.Pre = base; L.Pim = L.Pre + RW_NB * RW_PS; L.Ure = L.Pim + RW_NB * RW_PS; L.Uim = L.Ure + RW_NB * RW_CW;
    L.ywin = reinterpret_cast<double2 *>(L.Uim + RW_NB * RW_CW); L.xs = L.ywin + RW_PS;
    L.red = reinterpret_cast<double *>(L.xs + RW_NW * RW_NB);
    L.pred = reinterpret_cast<double2 *>(L.red + 16);
    L.perm = reinterpret_cast<int *>(L.pred + RW_NW); L.ipiv = L.perm + RW_PS; L.dpos = L.ipiv + RW_NB; L.dsrc = L.dpos + RW_NB; L.ndp = L.dsrc + RW_NB;
    return L;
}

// M(i, c), c - 2 bw <= i <= c + bw, of the band AB with LD = 3 bw + 1
__device__ __forceinline__ double2 *rw_at(double2 *AB, const int LD, const int bw, const int i, const int c)
{
    return AB + (size_t)c * LD + (i - c + 2 * bw);
}

// The band of item `it` (its z, w, channels; the coefficients of item `ita`), column by column, into AB, by the whole workgroup; each
// wave leaves the scale of the zero-pivot perturbation from its part of the diagonal (rs_pertol's dmax, dflo) in L.pred and returns
// it.  The caller's barrier -- after it has written whatever else the factorisation reads: the right-hand sides -- puts the band in
// memory and L.pred before rw_pertol.
__device__ __forceinline__ double2 rw_assemble(const ResolventCoupledArgs &a, const int it, const int ita, const int N, const int bw,
                                               double2 *AB, const RwLds L, const int tid)
{
    const int LD = 3 * bw + 1, lane = tid & 63, wv = tid >> 6;
    double dmax = 0.0, dflo = 0.0;
    for (int c = wv; c < N; c += RW_NW)
        for (int o = lane; o < LD; o += 64) {
            const int i = c - 2 * bw + o;
            if (i >= 0 && i < N) {
                double re = 0.0, im = 0.0, fl = 0.0;
                if (o >= bw) rc_entry(a, it, ita, i, c, re, im, fl);   // above it: the room of the fill, zero
                AB[(size_t)c * LD + o] = make_double2(re, im);
                if (o == 2 * bw) { dmax = fmax(dmax, fabs(re) + fabs(im)); dflo = fmax(dflo, fl); }
            }
        }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) { dmax = fmax(dmax, __shfl_xor(dmax, off)); dflo = fmax(dflo, __shfl_xor(dflo, off)); }
    if (lane == 0) L.pred[wv] = make_double2(dmax, dflo);
    return make_double2(dmax, dflo);
}
// ... and after that barrier: the threshold, the same in every thread (part: what rw_assemble returned)
__device__ __forceinline__ double rw_pertol(const double2 part, const RwLds L)
{
    double dmax = part.x, dflo = part.y;
#pragma unroll
    for (int q = 0; q < RW_NW; ++q) { dmax = fmax(dmax, L.pred[q].x); dflo = fmax(dflo, L.pred[q].y); }
    return rs_pertol(dmax, dflo);
}

// a b - c d and a b + c d as ONE fused multiply-add on the first product and the second product rounded on its own.  Which product of
// a complex multiply is fused decides the last bit, and left to the compiler it changes with the code around the statement; the
// factorisation and the back-substitution state it for each of their complex products (the choice each has had since it was written), so
// that every kernel that inlines them rounds alike.
__device__ __forceinline__ double rw_fms(const double a, const double b, const double c, const double d)
{
#pragma clang fp contract(off)
    return __builtin_fma(a, b, -(c * d));
}
__device__ __forceinline__ double rw_fma(const double a, const double b, const double c, const double d)
{
#pragma clang fp contract(off)
    return __builtin_fma(a, b, c * d);
}

// The factorisation P M = L U of the assembled band, panel by panel, and y <- L^-1 P y of the nrhs vectors y [nrhs][N] with each panel
// (L is never stored).  On entry the band and y are in memory and visible to the workgroup; on return AB holds U (1 / pivot on the
// diagonal) and the stores of the last panel are NOT yet ordered: the caller's __syncthreads() comes before rw_backsolve.  Returns
// the replaced pivots, in every thread.  Nothing here is contracted by the compiler: the complex products are rw_fms / rw_fma, the
// subtraction from the running value is a plain one (the shared rs_pivot_recip keeps its own form).
__device__ __forceinline__ int rw_factor(const int N, const int bw, const double pertol, double2 *AB, const int nrhs, double2 *y,
                                         const RwLds L, const int tid)
{
#pragma clang fp contract(off)
    constexpr int NB = RW_NB, PS = RW_PS, CWp = RW_CW;
    const int LD = 3 * bw + 1, lane = tid & 63, wv = tid >> 6;
    double *Pre = L.Pre, *Pim = L.Pim, *Ure = L.Ure, *Uim = L.Uim, *red = L.red;
    double2 *ywin = L.ywin;
    int *perm = L.perm, *ipiv = L.ipiv, *dpos = L.dpos, *dsrc = L.dsrc, *ndp = L.ndp;
    auto at = [&](int i, int c) -> double2 * { return rw_at(AB, LD, bw, i, c); };
    int nper = 0;
    for (int j0 = 0; j0 < N; j0 += NB) {
        const int nb = (N - j0 < NB) ? N - j0 : NB;
        const int mrow = (N - j0 < nb + bw) ? N - j0 : nb + bw;  // rows j0 .. j0 + mrow - 1 of the panel
        // ---- the panel into LDS; what lies outside the band, the matrix or the panel is zero
        for (int e = tid; e < NB * PS; e += RW_NT) {
            const int t = e / PS, r = e - t * PS;
            double2 v = make_double2(0.0, 0.0);
            if (t < nb && r < mrow && r - t <= bw && t - r <= 2 * bw) v = *at(j0 + r, j0 + t);
            Pre[e] = v.x; Pim[e] = v.y;
        }
        if (tid < PS) perm[tid] = tid;
        lds_barrier();
        // ---- its factorisation, column by column
        for (int t = 0; t < nb; ++t) {
            const int nrow = (N - 1 - (j0 + t) < bw) ? N - 1 - (j0 + t) : bw;
            if (wv < 4) {
                // candidate wv * 64 + lane is row j0 + t + wv * 64 + lane; ties go to the smallest row
                const int cand = wv * 64 + lane;
                const bool ok = cand <= nrow;
                double vr = 0.0, vi = 0.0;
                if (ok) { vr = Pre[t * PS + t + cand]; vi = Pim[t * PS + t + cand]; }
                const double mag = ok ? fabs(vr) + fabs(vi) : -1.0;
                const double mx = rc_wave_max(mag);
                const unsigned long long hit = __ballot(mag == mx);
                const int dp = __builtin_amdgcn_readfirstlane(hit ? __ffsll((long long)hit) - 1 : 0);
                const double wr = read_lane(vr, dp), wi = read_lane(vi, dp);
                if (lane == 0) {
                    red[4 * wv] = (wv * 64 <= nrow) ? mx : -1.0;   // a wave without candidates never wins
                    red[4 * wv + 1] = (double)(wv * 64 + dp);
                    red[4 * wv + 2] = wr; red[4 * wv + 3] = wi;
                }
            }
            lds_barrier();
            // the waves in ascending order: a later one wins only if it is strictly larger
            double best = -1.0, pr = 0.0, pi = 0.0;
            int p = 0;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const double m = red[4 * w];
                if (m > best) { best = m; p = (int)red[4 * w + 1]; pr = red[4 * w + 2]; pi = red[4 * w + 3]; }
            }
            const double2 rcp = rs_pivot_recip(pr, pi, pertol, nper);
            const double rr = rcp.x, ri = rcp.y;
            // rows t and t + p change places in every column of the panel, L's among them
            if (p != 0 && tid < NB) {
                const int e0 = tid * PS + t, e1 = e0 + p;
                const double t0 = Pre[e0], t1 = Pim[e0];
                Pre[e0] = Pre[e1]; Pim[e0] = Pim[e1];
                Pre[e1] = t0; Pim[e1] = t1;
            }
            if (tid == 0) ipiv[t] = t + p;
            lds_barrier();
            // a thread per row below: its multiplier, then its row of the columns t + 1 .. nb - 1
            if (tid >= 1 && tid <= nrow) {
                const int r = t + tid;
                const double xr = Pre[t * PS + r], xi = Pim[t * PS + r];
                const double lr = rw_fms(xr, rr, xi, ri), li = rw_fma(xr, ri, xi, rr);
                Pre[t * PS + r] = lr; Pim[t * PS + r] = li;
                for (int s = t + 1; s < nb; ++s) {
                    const double ur = Pre[s * PS + t], ui = Pim[s * PS + t];
                    const double pr2 = rw_fms(lr, ur, li, ui), pi2 = rw_fma(li, ur, lr, ui);
                    Pre[s * PS + r] -= pr2; Pim[s * PS + r] -= pi2;
                }
            }
            if (tid == 0) { Pre[t * PS + t] = rr; Pim[t * PS + t] = ri; }   // the diagonal of U holds 1 / pivot
            lds_barrier();
        }
        // ---- the interchanges as one permutation: new row r is old row perm[r]; dpos: the rows below the block that changed
        if (tid == 0) {
            for (int t = 0; t < nb; ++t) {
                const int p = ipiv[t];
                if (p != t) { const int x = perm[t]; perm[t] = perm[p]; perm[p] = x; }
            }
            int nd = 0;
            for (int t = 0; t < nb; ++t) {
                const int p = ipiv[t];
                if (p < nb || perm[p] == p) continue;
                bool seen = false;
                for (int q = 0; q < nd; ++q) seen = seen || dpos[q] == p;
                if (!seen) { dpos[nd] = p; dsrc[nd] = perm[p]; ++nd; }
            }
            *ndp = nd;
        }
        // U11 goes back to the band
        if (tid < NB * NB) {
            const int t = tid / NB, r = tid - t * NB;
            if (t < nb && r <= t && t - r <= 2 * bw) *at(j0 + r, j0 + t) = make_double2(Pre[t * PS + r], Pim[t * PS + r]);
        }
        lds_barrier();
        // ---- the right-hand sides: y <- L^-1 P y on the panel's rows
        for (int r = 0; r < nrhs; ++r) {
            double2 *yy = y + (size_t)r * N;
            if (tid < mrow) ywin[tid] = yy[j0 + perm[tid]];
            lds_barrier();
            if (wv == 0) {
                double vr = 0.0, vi = 0.0;
                if (lane < nb) { vr = ywin[lane].x; vi = ywin[lane].y; }
#pragma unroll
                for (int s = 0; s < NB - 1; ++s) {
                    const double sr = read_lane(vr, s), si = read_lane(vi, s);
                    if (lane > s && lane < nb) {
                        const double lr = Pre[s * PS + lane], li = Pim[s * PS + lane];
                        vr -= rw_fms(lr, sr, li, si);
                        vi -= rw_fma(lr, si, li, sr);
                    }
                }
                if (lane < nb) ywin[lane] = make_double2(vr, vi);
            }
            lds_barrier();
            if (tid < mrow) {
                double2 v = ywin[tid];
                if (tid >= nb) {
#pragma unroll
                    for (int s = 0; s < NB; ++s) {
                        if (s < nb) {
                            const double lr = Pre[s * PS + tid], li = Pim[s * PS + tid];
                            const double2 x = ywin[s];
                            v.x -= rw_fms(lr, x.x, li, x.y);
                            v.y -= rw_fma(li, x.x, lr, x.y);
                        }
                    }
                }
                yy[j0 + tid] = v;
            }
            lds_barrier();
        }
        // ---- the columns to the right, in chunks: interchanges, U12 = L11^-1 A12, A22 -= L21 U12
        if (j0 + nb < N) {                                       // then nb == NB
            const int cend = (N < j0 + NB + 2 * bw) ? N : j0 + NB + 2 * bw;
            const int m2 = mrow - NB, mt = (m2 + 15) >> 4;
            for (int c0 = j0 + NB; c0 < cend; c0 += CWp) {
                const int ncol = (cend - c0 < CWp) ? cend - c0 : CWp;
                if (tid < CWp) {
                    const int c = c0 + tid;
                    const bool act = tid < ncol;
                    const int nd = *ndp;
                    double2 u[NB];
                    // every load before any store: the gather reads what the stores replace.  The rows displaced below the
                    // block wait in this thread's column of the LDS image of U12, which is written only after them
#pragma unroll
                    for (int t = 0; t < NB; ++t) {
                        const int src = j0 + perm[t];
                        u[t] = make_double2(0.0, 0.0);
                        if (act && c - src <= 2 * bw) u[t] = *at(src, c);
                    }
                    for (int q = 0; q < nd; ++q) {
                        const int src = j0 + dsrc[q];
                        double2 v = make_double2(0.0, 0.0);
                        if (act && c - src <= 2 * bw) v = *at(src, c);
                        Ure[q * CWp + tid] = v.x; Uim[q * CWp + tid] = v.y;
                    }
                    if (act)
                        for (int q = 0; q < nd; ++q) *at(j0 + dpos[q], c) = make_double2(Ure[q * CWp + tid], Uim[q * CWp + tid]);
                    // U12 = L11^-1 A12 in this thread's column of the LDS image (rolled loops: the multipliers are read as they
                    // are used), row t after the rows above it, s ascending
#pragma unroll
                    for (int t = 0; t < NB; ++t) {
                        Ure[t * CWp + tid] = act ? u[t].x : 0.0;
                        Uim[t * CWp + tid] = act ? u[t].y : 0.0;
                    }
                    if (act && c - j0 <= 2 * bw) *at(j0, c) = u[0];
#pragma unroll 1
                    for (int t = 1; t < NB; ++t) {
                        double xr = Ure[t * CWp + tid], xi = Uim[t * CWp + tid];
#pragma unroll 1
                        for (int s = 0; s < t; ++s) {
                            const double lr = Pre[s * PS + t], li = Pim[s * PS + t];
                            const double sr = Ure[s * CWp + tid], si = Uim[s * CWp + tid];
                            xr -= rw_fms(lr, sr, li, si);
                            xi -= rw_fma(li, sr, lr, si);
                        }
                        Ure[t * CWp + tid] = xr; Uim[t * CWp + tid] = xi;
                        if (act && c - (j0 + t) <= 2 * bw) *at(j0 + t, c) = make_double2(xr, xi);
                    }
                }
                __syncthreads();                                 // the displaced rows are in memory, U12 is in LDS
                const int nt = (ncol + 15) >> 4;
                for (int q = wv; q < mt * nt; q += RW_NW) {
                    const int tj = q / mt, ti = q - tj * mt;
                    const int li = NB + 16 * ti + (lane & 15), uc = 16 * tj + (lane & 15);
                    double4_t aR = {0.0, 0.0, 0.0, 0.0}, aI = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                    for (int k4 = 0; k4 < NB / 4; ++k4) {
                        const int kk = 4 * k4 + (lane >> 4);
                        const double ur = Ure[kk * CWp + uc], ui = Uim[kk * CWp + uc];
                        const double lr = Pre[kk * PS + li], lim = Pim[kk * PS + li];
                        // the product transposed (gemm_f64.hip): acc[r] is row (lane & 15), column (lane >> 4) + 4 r of the tile
                        aR = __builtin_amdgcn_mfma_f64_16x16x4f64(ur, lr, aR, 0, 0, 0);
                        aR = __builtin_amdgcn_mfma_f64_16x16x4f64(ui, -lim, aR, 0, 0, 0);
                        aI = __builtin_amdgcn_mfma_f64_16x16x4f64(ur, lim, aI, 0, 0, 0);
                        aI = __builtin_amdgcn_mfma_f64_16x16x4f64(ui, lr, aI, 0, 0, 0);
                    }
                    if (li < mrow) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int cc = 16 * tj + (lane >> 4) + 4 * r;
                            if (cc < ncol) {
                                double2 *pa = at(j0 + li, c0 + cc);
                                double2 v = *pa;
                                v.x -= aR[r]; v.y -= aI[r];
                                *pa = v;
                            }
                        }
                    }
                }
                __syncthreads();                                 // A22 is in memory before the next chunk or panel reads it
            }
        }
    }
    return nper;
}

// x <- U^-1 y in place for the nrhs vectors y [nrhs][N], block by block from the last, eight right-hand sides at a time.  On entry U
// (rw_factor's) and y are in memory and visible to the workgroup; on return so is x.  Nothing here is contracted by the compiler:
// the complex products are rw_fms / rw_fma, the subtraction from the running value is a plain one.
__device__ __forceinline__ void rw_backsolve(const int N, const int bw, double2 *AB, const int nrhs, double2 *y, const RwLds L, const int tid)
{
#pragma clang fp contract(off)
    constexpr int NB = RW_NB;
    const int LD = 3 * bw + 1, lane = tid & 63, wv = tid >> 6;
    double2 *xs = L.xs;
    auto at = [&](int i, int c) -> double2 * { return rw_at(AB, LD, bw, i, c); };
    const int nblk = (N + NB - 1) / NB;
    for (int r0 = 0; r0 < nrhs; r0 += RW_NW) {
        const int ng = (nrhs - r0 < RW_NW) ? nrhs - r0 : RW_NW;
        for (int b = nblk - 1; b >= 0; --b) {
            const int j0 = b * NB, nb = (N - j0 < NB) ? N - j0 : NB;
            if (wv < ng) {
                // the triangle on one wave: lane r holds y[j0 + r] and row r of U11
                double2 *yy = y + (size_t)(r0 + wv) * N;
                double2 uu[NB];
                double vr = 0.0, vi = 0.0, dr = 0.0, di = 0.0;
                if (lane < nb) {
                    const double2 v = yy[j0 + lane], d = *at(j0 + lane, j0 + lane);
                    vr = v.x; vi = v.y; dr = d.x; di = d.y;
                }
#pragma unroll
                for (int t = 0; t < NB; ++t) {
                    uu[t] = make_double2(0.0, 0.0);
                    if (t > lane && t < nb && t - lane <= 2 * bw) uu[t] = *at(j0 + lane, j0 + t);
                }
#pragma unroll
                for (int t = NB - 1; t >= 0; --t) {
                    if (t < nb) {                                // uniform
                        const double xr = read_lane(rw_fms(vr, dr, vi, di), t), xi = read_lane(rw_fma(vr, di, vi, dr), t);
                        if (lane == t) { vr = xr; vi = xi; }
                        if (lane < t) {
                            vr -= rw_fms(uu[t].x, xr, uu[t].y, xi);
                            vi -= rw_fma(uu[t].x, xi, uu[t].y, xr);
                        }
                    }
                }
                if (lane < nb) yy[j0 + lane] = make_double2(vr, vi);
                if (lane < NB) xs[wv * NB + lane] = make_double2(lane < nb ? vr : 0.0, lane < nb ? vi : 0.0);
            }
            __syncthreads();
            // the rows above, a thread each: y_i -= sum_t U(i, j0 + t) x_t, t ascending
            const int i = j0 - 1 - tid;
            if (tid < 2 * bw && i >= 0) {
                double2 uu[NB];
#pragma unroll
                for (int t = 0; t < NB; ++t) {
                    uu[t] = make_double2(0.0, 0.0);
                    if (t < nb && j0 + t - i <= 2 * bw) uu[t] = *at(i, j0 + t);
                }
                for (int g = 0; g < ng; ++g) {
                    double2 *yy = y + (size_t)(r0 + g) * N;
                    double2 v = yy[i];
#pragma unroll
                    for (int t = 0; t < NB; ++t) {
                        const double2 x = xs[g * NB + t];
                        v.x -= rw_fms(uu[t].x, x.x, uu[t].y, x.y);
                        v.y -= rw_fma(uu[t].x, x.y, uu[t].y, x.x);
                    }
                    yy[i] = v;
                }
            }
            __syncthreads();
        }
    }
}

}  // namespace bsp
