// tdse_split.hip -- the TDSE in the B-spline basis by split Crank-Nicolson steps (include/bspatom_tdse_split.h: bspatom_tdse_split).
//
// i S dc/dt = (sum_c (H_lc - i W_c) + f(t) A (x) G) c with ONE operator term: a constant real symmetric nch x nch angular matrix
// A = Q diag(lam) Q^T and one radial band G.  The symmetric splitting
//     exp(-i S^-1 A_c dt/2)  .  exp(-i S^-1 f lam_j G dt) in the eigenbasis of A  .  exp(-i S^-1 A_c dt/2),
// every factor in its Cayley form, is second order in dt like the unsplit step of tdse_spline.hip, and every substep is nch
// INDEPENDENT complex banded systems of half-width k - 1: the one-wave systems of resolvent.hip.  A step costs O(nch N k^2), the
// channels run side by side on the CUs, and nch has no limit.
//
//   atomic half step, channel c:   b = S c_c,  x = M_c^-1 b,  M_c = H_lc - i W_c - (4i/dt) S,   c_c <- -(8i/dt) x - c_c.
//                                  M_c does not depend on time: tsplit_factor_kernel factors it once per call and distinct (l, w),
//                                  the steps run the two substitutions alone.
//   field step, eigenchannel j:    d_j = sum_c Q(c,j) c_c,  N_j = S + i (dt/2) f lam_j G,   d_j <- 2 N_j^-1 (S d_j) - d_j.
//                                  N_j changes with the step: factored every time.
//   back:                          c_c = sum_j Q(c,j) d_j, then the atomic half step again.
//
// How: one wavefront per system -- the methods of resolvent.hip (rs_factor, rs_solve, rs_band_apply): the row window in registers,
// multipliers and the pivot row by readlane, the window moved by a one-lane DPP shift, no LDS and no barrier in the n dependent steps
// -- in statements of this file's own: this call promises no bit equality with bspatom_resolvent, and resolvent.hip's bits depend on
// the code around its loops, so nothing is moved out of it.  Shared with it through resolvent_shared.h: the pivot
// threshold, the reciprocal of a pivot, the forward substitution.  Every sum whose order the header fixes is written without FMA
// (the whole file is compiled with contraction off; the LU's multiply-adds are explicit fma calls).
//
// Scheduling: a PERSISTENT grid of single-wave workgroups takes the nscan * nch items of a substep by static stride; substeps are
// separated by kernel boundaries, three launches per step: the first atomic half step (with the rows), the field step, the second
// atomic half step (with the snapshot).  A kernel reads its scan's other channels from the buffer the previous launch wrote and
// writes the other buffer: the mixing with Q is folded into the operand loads of the field kernel and of the second atomic kernel.
// No workgroup waits on another, no atomics, no progress words.
#include "common.h"
#include "wave_ops.h"
#include "resolvent_shared.h"

#pragma clang fp contract(off)

namespace bsp {
namespace {
constexpr int SP_BMAX = 15;                // half-bandwidth limit (k <= 16): the one-wave window's

// doubles of one factorisation: U [n][2b+1], L [n][b] complex, piv [n] ints; even
__host__ __device__ inline size_t sp_factor_doubles(int n, int k)
{
    const size_t b = (size_t)k - 1, piv = ((size_t)n + 1) / 2;
    return 2 * ((size_t)n * (2 * b + 1) + (size_t)n * b) + piv + (piv & 1);
}
// doubles of one slot's scratch: v, y [n] complex, then the field step's factorisation
__host__ __device__ inline size_t sp_slot_doubles(int n, int k) { return 4 * (size_t)n + sp_factor_doubles(n, k); }

struct SpFactor {
    double2 *U, *Lm;
    int *piv;
};
__device__ __forceinline__ SpFactor sp_factor_at(double *base, int n, int b)
{
    SpFactor f;
    f.U = reinterpret_cast<double2 *>(base);
    f.Lm = f.U + (size_t)n * (2 * b + 1);
    f.piv = reinterpret_cast<int *>(f.Lm + (size_t)n * b);
    return f;
}

// The two matrices.  SB, HB upper bands [k][n] used symmetrically, WB and GB FULL bands [2k-1][n], X[(d + b) n + i] = X(i, i + d).
// entry: M(r, c), zero outside the band and the matrix; diag: |M(j,j)| by cabs1 and the sum of the magnitudes of its terms (rs_pertol)
// M_c = H - i W - (0, zi) S
struct SpAtomic {
    const double *SB, *HB, *WB;
    int n, b;
    double zi;
    __device__ __forceinline__ void entry(int r, int c, double &re, double &im) const
    {
        const int d = (r > c) ? (r - c) : (c - r);
        re = 0.0; im = 0.0;
        if (d > b || r < 0 || c < 0 || r >= n || c >= n) return;
        const int lo = (r > c) ? c : r;
        re = HB[(size_t)d * n + lo];
        im = -(zi * SB[(size_t)d * n + lo]);
        if (WB) im -= WB[(size_t)(c - r + b) * n + r];
    }
    __device__ __forceinline__ void diag(int j, double &mag, double &flo) const
    {
        const double s = SB[j], h = HB[j], wv = WB ? WB[(size_t)b * n + j] : 0.0;
        mag = fabs(h) + fabs(-(zi * s) - wv);
        flo = fabs(h) + (fabs(zi * s) + fabs(wv));
    }
};
// N_j = S + (ar, ai) G, (ar, ai) = i (dt/2) f lam_j
struct SpField {
    const double *SB, *GB;
    int n, b;
    double ar, ai;
    __device__ __forceinline__ void entry(int r, int c, double &re, double &im) const
    {
        const int d = (r > c) ? (r - c) : (c - r);
        re = 0.0; im = 0.0;
        if (d > b || r < 0 || c < 0 || r >= n || c >= n) return;
        const int lo = (r > c) ? c : r;
        const double g = GB[(size_t)(c - r + b) * n + r];
        re = SB[(size_t)d * n + lo] + ar * g;
        im = ai * g;
    }
    __device__ __forceinline__ void diag(int j, double &mag, double &flo) const
    {
        const double s = SB[j], g = GB[(size_t)b * n + j];
        mag = fabs(s + ar * g) + fabs(ai * g);
        flo = (fabs(s) + fabs(ar * g)) + fabs(ai * g);
    }
};

// The factorisation P M = L U of one matrix by one wavefront, resolvent.hip's method.  U: [n][2b+1] complex, row j = (1 / pivot,
// U(j, j+1 .. j+2b)); Lm: [n][b] complex multipliers; piv: [n] pivot rows.  Pivot by |Re| + |Im|, ties to the smallest row; the
// threshold and the reciprocal are rs_pertol and rs_pivot_recip.  Returns the number of pivots that were replaced.
template <int BT, class Entry>
__device__ __forceinline__ int sp_factor(const int n, const int b, const Entry &e, const SpFactor &f, const int lane)
{
    constexpr int PF = RS_PF;
    double dmax = 0.0, dflo = 0.0;
    for (int j = lane; j < n; j += 64) {
        double mag, flo;
        e.diag(j, mag, flo);
        dmax = fmax(dmax, mag);
        dflo = fmax(dflo, flo);
    }
    dmax = rc_wave_max(dmax); dflo = rc_wave_max(dflo);
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
        // pivot search down lane 0's registers (column j)
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
            const double xr = read_lane(ar[t], 0), xi = read_lane(ai[t], 0);
            const double ltr = (t <= nrow) ? __builtin_fma(xr, rr, -(xi * ri)) : 0.0;
            const double lti = (t <= nrow) ? __builtin_fma(xr, ri, xi * rr) : 0.0;
            lmr = (lane == t) ? ltr : lmr;
            lmi = (lane == t) ? lti : lmi;
            // a[t] -= l a[0], four fused multiply-adds
            const double nr = __builtin_fma(lti, ai[0], __builtin_fma(-ltr, ar[0], ar[t]));
            const double ni = __builtin_fma(-lti, ar[0], __builtin_fma(-ltr, ai[0], ai[t]));
            ar[t] = (lane >= 1) ? nr : 0.0;                          // columns j + 1 .. j + 2 b; column j is eliminated
            ai[t] = (lane >= 1) ? ni : 0.0;
        }
        if (lane == 0) f.piv[j] = j + dp;
        if (lane <= 2 * b) f.U[(size_t)j * (2 * b + 1) + lane] = (lane == 0) ? make_double2(rr, ri) : make_double2(ar[0], ai[0]);
        if (lane >= 1 && lane <= b) f.Lm[(size_t)j * b + lane - 1] = make_double2(lmr, lmi);
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

// y <- U^-1 L^-1 P y in place (y: n complex of the slot, visible to the wave): rs_forward, then the backward pass
// x_j = (y_j - sum_{c=1..2b} U[j][c] x_{j+c}) / pivot_j with lane c holding x[j + c], what enters requested a block ahead.  On return
// the solution is visible to every lane.
__device__ __forceinline__ void sp_solve(const int n, const int b, const SpFactor &f, double2 *y, const int lane)
{
    rs_forward(n, b, f.Lm, f.piv, y, lane);
    constexpr int PF = RS_PF;
    const int w = 2 * b + 1;
    const double2 *U = f.U;
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
                if (lane >= 1 && lane <= 2 * b && j + lane < n) {
                    sr = __builtin_fma(uv[u].x, wr, -(uv[u].y * wi));
                    si = __builtin_fma(uv[u].x, wi, uv[u].y * wr);
                }
                sr = wave_sum32(sr); si = wave_sum32(si);
                const double dr = read_lane(yb.x, u) - sr, di = read_lane(yb.y, u) - si;
                const double xr = __builtin_fma(dr, ru[u].x, -(di * ru[u].y)), xi = __builtin_fma(dr, ru[u].y, di * ru[u].x);
                if (lane == 0) y[j] = make_double2(xr, xi);
                wr = dpp_mov<0x138>(wr); wi = dpp_mov<0x138>(wi);  // wave_shr:1 -- lane i takes lane i - 1
                if (lane == 1) { wr = xr; wi = xi; }
            }
        }
    }
    rs_sync();
}

// v(i) = sum_m q[m qs] in_m(i), m = 0 .. nch-1 ascending from +0.0, multiply then add: the mixing with Q folded into a kernel's operand
// load.  in: the scan's packet [nch][n] complex; lane-strided over i, every lane its own rows.
__device__ __forceinline__ void sp_mix(const int n, const int nch, const double *q, const int qs, const double2 *in, double2 *v, const int lane)
{
    for (int i = lane; i < n; i += 64) {
        double vr = 0.0, vi = 0.0;
#pragma unroll 8
        for (int m = 0; m < nch; ++m) {
            const double qm = q[(size_t)m * qs];
            const double2 x = in[(size_t)m * n + i];
            vr = vr + qm * x.x;
            vi = vi + qm * x.y;
        }
        v[i] = make_double2(vr, vi);
    }
}

// y = S v by rule 1 of include/bspatom_tdse_spline.h: y_re(i), y_im(i) start at +0.0 and add S(i, i + d) v(i + d) for d = -(k-1) .. k-1
// ascending, columns outside 0 .. n-1 skipped.  Lane-strided over the rows; a row's loads are issued together by blocks of CH
// diagonals, every address clamped into its array and what was loaded outside dropped by a select (rs_band_apply's way).  v is
// visible to the wave.  Returns, where nrm is set, this lane's part of Re sum_i conj(v(i)) y(i), rows ascending (else zero).
template <int BT>
__device__ __forceinline__ double sp_overlap(const int n, const int b, const double *__restrict__ SB, const double2 *v, double2 *y, const bool nrm,
                                             const int lane)
{
    constexpr int CH = (2 * BT + 1 + 2) / 3;
    const int nd = 2 * b + 1;
    double s = 0.0;
    for (int i = lane; i < n; i += 64) {
        double yr = 0.0, yi = 0.0;
#pragma unroll 1
        for (int d0 = 0; d0 < nd; d0 += CH) {
            double t[CH];
            double2 xv[CH];
#pragma unroll
            for (int u = 0; u < CH; ++u) {
                const int d = d0 + u - b, ad = d < 0 ? -d : d, lo = d < 0 ? i + d : i;
                const bool in = d0 + u < nd && lo >= 0 && i + d < n;
                t[u] = SB[in ? (size_t)ad * n + lo : 0];
            }
#pragma unroll
            for (int u = 0; u < CH; ++u) {
                const int j = i + d0 + u - b;
                xv[u] = v[j < 0 ? 0 : (j >= n ? n - 1 : j)];
            }
#pragma unroll
            for (int u = 0; u < CH; ++u) {
                const int j = i + d0 + u - b;
                const bool in = d0 + u < nd && j >= 0 && j < n;
                const double ur = yr + t[u] * xv[u].x, ui = yi + t[u] * xv[u].y;
                yr = in ? ur : yr;
                yi = in ? ui : yi;
            }
        }
        y[i] = make_double2(yr, yi);
        if (nrm) {
            const double2 cv = v[i];
            s = s + (cv.x * yr + cv.y * yi);
        }
    }
    return s;
}
}  // namespace

// The atomic matrices of a call, one item per distinct (l, w): factors [nfac] of sp_factor_doubles, finfo[f] the pivots replaced.
template <int BT>
__global__ __launch_bounds__(64) void tsplit_factor_kernel(const TdseSplitArgs a)
{
    const int n = a.n, b = a.k - 1, lane = threadIdx.x;
    for (int f = blockIdx.x; f < a.nfac; f += gridDim.x) {
        const int ws = a.fw[f];
        SpAtomic e = {a.SB, a.HB + (size_t)a.fchan[f] * a.k * n, (a.WB && ws >= 0) ? a.WB + (size_t)ws * (2 * b + 1) * n : nullptr, n, b, a.zi};
        const int nper = sp_factor<BT>(n, b, e, sp_factor_at(a.fstore + (size_t)f * sp_factor_doubles(n, a.k), n, b), lane);
        if (lane == 0) a.finfo[f] = nper;
    }
}

// An atomic half step of every (scan, channel).  mix = 0: the channel's packet is read from `in` as it stands (the first half step);
// mix = 1: c_c = sum_j Q(c, j) d_j from the eigenchannels in `in` (the second).  row: the row of this step's packets from b = S c --
// N_c, and this channel's part of every projection into part, which the field kernel sums --; measure: the row alone, nothing solved
// or written (the row of the final packets).  snap: a copy of what goes to out.
template <int BT>
__global__ __launch_bounds__(64) void tsplit_atomic_kernel(const TdseSplitArgs a)
{
    const int b = a.k - 1, nch = a.nch;
    double *work = a.work + (size_t)blockIdx.x * sp_slot_doubles(a.n, a.k);
    for (int it = blockIdx.x; it < a.nscan * nch; it += gridDim.x) {
        // the operands made new values in every item, so that nothing hoisted out of the bodies stays live across the items
        int n = a.n, lane = threadIdx.x;
        double *wk = work;
        asm volatile("" : "+s"(n), "+s"(wk), "+v"(lane));
        double2 *xin = reinterpret_cast<double2 *>(wk), *y = xin + n;
        const int q = it / nch, ch = it - q * nch;
        const double2 *in = reinterpret_cast<const double2 *>(a.in) + (size_t)q * nch * n;
        const double2 *v = in + (size_t)ch * n;
        if (a.mix) {
            sp_mix(n, nch, a.Q + (size_t)ch * nch, 1, in, xin, lane);
            rs_sync();
            v = xin;
        }
        double nrm = sp_overlap<BT>(n, b, a.SB, v, y, a.row != nullptr, lane);
        if (a.row) {
            const int RW = nch + 2 * a.nproj;
            nrm = wave_sum(nrm);
            if (lane == 0) a.row[(size_t)q * RW + ch] = nrm;
            for (int r = 0; r < a.nproj; ++r) {
                // bilinear, no conjugate: lane-strided partial sums over each lane's own rows of b, then the wave's fixed tree
                const double *P = a.P + (size_t)2 * ((size_t)r * nch + ch) * n;
                double sr = 0.0, si = 0.0;
                for (int i = lane; i < n; i += 64) {
                    const double pr = P[2 * i], pi = P[2 * i + 1];
                    const double2 bv = y[i];
                    sr = sr + (pr * bv.x - pi * bv.y);
                    si = si + (pr * bv.y + pi * bv.x);
                }
                sr = wave_sum(sr); si = wave_sum(si);
                if (lane == 0) {
                    double *pt = a.part + 2 * (((size_t)q * a.nproj + r) * nch + ch);
                    pt[0] = sr; pt[1] = si;
                }
            }
        }
        rs_sync();                                                   // b is in memory
        if (a.measure) continue;
        sp_solve(n, b, sp_factor_at(a.fstore + (size_t)a.fac[ch] * sp_factor_doubles(n, a.k), n, b), y, lane);
        // c' = -(8 i / dt) x - c: one multiply and one subtract per component
        double *out = a.out + 2 * ((size_t)q * nch + ch) * n;
        double *sn = a.snap ? a.snap + 2 * ((size_t)q * nch + ch) * n : nullptr;
        for (int i = lane; i < n; i += 64) {
            const double2 x = y[i], cv = v[i];
            const double pr = a.g * x.y, pi = a.g * x.x;
            const double nr = pr - cv.x, ni = -pi - cv.y;
            out[2 * i] = nr; out[2 * i + 1] = ni;
            if (sn) { sn[2 * i] = nr; sn[2 * i + 1] = ni; }
        }
        rs_sync();                                                   // every load of the slot is back before the next item overwrites it
    }
}

// The field step of every (scan, eigenchannel): d_j = sum_c Q(c, j) c_c from `in`, N_j = S + i (dt/2) f lam_j G factored,
// d_j <- 2 N_j^-1 (S d_j) - d_j into out.  pinfo[q nch + j] gains the pivots replaced.  row: item j = 0 of a scan sums the parts of
// the scan's projections over the channels ascending, from +0.0, into the row; measure: that alone.
template <int BT>
__global__ __launch_bounds__(64) void tsplit_field_kernel(const TdseSplitArgs a)
{
    const int b = a.k - 1, nch = a.nch;
    double *work = a.work + (size_t)blockIdx.x * sp_slot_doubles(a.n, a.k);
    for (int it = blockIdx.x; it < a.nscan * nch; it += gridDim.x) {
        int n = a.n, lane = threadIdx.x;
        double *wk = work;
        asm volatile("" : "+s"(n), "+s"(wk), "+v"(lane));
        double2 *xin = reinterpret_cast<double2 *>(wk), *y = xin + n;
        const int q = it / nch, j = it - q * nch;
        if (a.row && j == 0)
            for (int r = lane; r < a.nproj; r += 64) {
                const double *pt = a.part + 2 * ((size_t)q * a.nproj + r) * nch;
                double sr = 0.0, si = 0.0;
                for (int c = 0; c < nch; ++c) { sr = sr + pt[2 * c]; si = si + pt[2 * c + 1]; }
                double *ro = a.row + (size_t)q * (nch + 2 * a.nproj) + nch + 2 * r;
                ro[0] = sr; ro[1] = si;
            }
        if (a.measure) continue;
        const double2 *in = reinterpret_cast<const double2 *>(a.in) + (size_t)q * nch * n;
        sp_mix(n, nch, a.Q + j, nch, in, xin, lane);
        rs_sync();
        sp_overlap<BT>(n, b, a.SB, xin, y, false, lane);
        // i (dt/2) mu, mu = f lam_j
        const double lam = a.lam[j], mur = a.f[2 * q] * lam, mui = a.f[2 * q + 1] * lam;
        SpField e = {a.SB, a.GB, n, b, -(a.h * mui), a.h * mur};
        const SpFactor fc = sp_factor_at(wk + 4 * (size_t)n, n, b);
        const int nper = sp_factor<BT>(n, b, e, fc, lane);
        if (lane == 0) a.pinfo[(size_t)q * nch + j] += nper;
        rs_sync();                                                   // b and the factors are in memory
        sp_solve(n, b, fc, y, lane);
        double *out = a.out + 2 * ((size_t)q * nch + j) * n;
        for (int i = lane; i < n; i += 64) {
            const double2 x = y[i], dv = xin[i];
            out[2 * i] = 2.0 * x.x - dv.x;
            out[2 * i + 1] = 2.0 * x.y - dv.y;
        }
        rs_sync();
    }
}

size_t tdse_split_factor_doubles(int n, int k) { return sp_factor_doubles(n, k); }
size_t tdse_split_slot_doubles(int n, int k) { return sp_slot_doubles(n, k); }
int tdse_split_max_k() { return SP_BMAX + 1; }

int tdse_split_slots(int k, int items, int *slots)
{
    if (k - 1 > SP_BMAX || k < 2 || items < 1) return BSP_ERR_ARG;
    if (k - 1 <= 8) return persistent_slots(tsplit_field_kernel<8>, 64, 0, items, slots);
    return persistent_slots(tsplit_field_kernel<SP_BMAX>, 64, 0, items, slots);
}

// what: 0 the atomic factorisations, 1 an atomic half step, 2 a field step
int launch_tdse_split(const TdseSplitArgs &a, int what, int slots, hipStream_t st)
{
    if (a.k - 1 > SP_BMAX || a.k < 2 || a.n < 1 || a.nch < 1 || a.nscan < 1 || slots < 1 || what < 0 || what > 2) return BSP_ERR_ARG;
    if (what == 0 && (a.nfac < 1 || !a.fstore)) return BSP_ERR_ARG;
    if (what != 0 && !a.measure && (!a.in || !a.out || !a.fstore || !a.Q || (what == 2 && (!a.GB || !a.lam || !a.f)))) return BSP_ERR_ARG;
    const bool small = a.k - 1 <= 8;
    const int grid = what == 0 ? (slots < a.nfac ? slots : a.nfac) : slots;
    if (what == 0) {
        if (small) hipLaunchKernelGGL(tsplit_factor_kernel<8>, dim3(grid), dim3(64), 0, st, a);
        else hipLaunchKernelGGL(tsplit_factor_kernel<SP_BMAX>, dim3(grid), dim3(64), 0, st, a);
    } else if (what == 1) {
        if (small) hipLaunchKernelGGL(tsplit_atomic_kernel<8>, dim3(grid), dim3(64), 0, st, a);
        else hipLaunchKernelGGL(tsplit_atomic_kernel<SP_BMAX>, dim3(grid), dim3(64), 0, st, a);
    } else {
        if (small) hipLaunchKernelGGL(tsplit_field_kernel<8>, dim3(grid), dim3(64), 0, st, a);
        else hipLaunchKernelGGL(tsplit_field_kernel<SP_BMAX>, dim3(grid), dim3(64), 0, st, a);
    }
    BSP_HIP(hipGetLastError());
    return BSP_OK;
}

}  // namespace bsp
