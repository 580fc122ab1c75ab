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
// How: one wavefront per system -- band_lu_wave.h's wave_lu_factor and wave_lu_solve, the one definition resolvent.hip runs too: the
// row window in registers, multipliers and the pivot row by readlane, the window moved by a one-lane DPP shift, no LDS and no barrier
// in the n dependent steps -- with this file's own arithmetic policy, WaveLuSplit, and its two matrices as SpAtomic and SpField:
// this call promises no bit equality with bspatom_resolvent.  The pivot threshold and the reciprocal of a pivot are
// resolvent_shared.h's.  Every sum whose order the header fixes is written without FMA (the whole file is compiled with contraction
// off; the LU's multiply-adds are explicit fma calls).
//
// Scheduling: a PERSISTENT grid of single-wave workgroups takes the nscan * nch items of a substep by static stride; substeps are
// separated by kernel boundaries, three launches per step: the first atomic half step (with the rows), the field step, the second
// atomic half step (with the snapshot).  A kernel reads its scan's other channels from the buffer the previous launch wrote and
// writes the other buffer: the mixing with Q is folded into the operand loads of the field kernel and of the second atomic kernel.
// No workgroup waits on another, no atomics, no progress words.
#include "common.h"
#include "wave_ops.h"
#include "resolvent_shared.h"
#include "band_lu_wave.h"
#include "spline_overlap.h"

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
// wave_lu_factor's argument -- entry: M(r, c), zero outside the band and the matrix; diag: |M(j,j)| by cabs1 and the sum of the
// magnitudes of its terms (rs_pertol)
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

// (b = S v with the norm, sp_overlap: spline_overlap.h, which spline_window.hip includes too)
}  // namespace

// The atomic matrices of a call, one item per distinct (l, w): factors [nfac] of sp_factor_doubles, finfo[f] the pivots replaced.
template <int BT>
__global__ __launch_bounds__(64) void tsplit_factor_kernel(const TdseSplitArgs a)
{
    const int n = a.n, b = a.k - 1, lane = threadIdx.x;
    for (int f = blockIdx.x; f < a.nfac; f += gridDim.x) {
        const int ws = a.fw[f];
        SpAtomic e = {a.SB, a.HB + (size_t)a.fchan[f] * a.k * n, (a.WB && ws >= 0) ? a.WB + (size_t)ws * (2 * b + 1) * n : nullptr, n, b, a.zi};
        const SpFactor fc = sp_factor_at(a.fstore + (size_t)f * sp_factor_doubles(n, a.k), n, b);
        const int nper = wave_lu_factor<BT, WaveLuSplit>(n, b, e, fc.U, fc.Lm, fc.piv, lane);
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
        const SpFactor fc = sp_factor_at(a.fstore + (size_t)a.fac[ch] * sp_factor_doubles(n, a.k), n, b);
        wave_lu_solve<WaveLuSplit>(n, b, fc.U, fc.Lm, fc.piv, y, lane);
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
        const int nper = wave_lu_factor<BT, WaveLuSplit>(n, b, e, fc.U, fc.Lm, fc.piv, lane);
        if (lane == 0) a.pinfo[(size_t)q * nch + j] += nper;
        rs_sync();                                                   // b and the factors are in memory
        wave_lu_solve<WaveLuSplit>(n, b, fc.U, fc.Lm, fc.piv, y, lane);
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
