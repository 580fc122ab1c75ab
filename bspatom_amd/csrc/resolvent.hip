// resolvent.hip -- solves with the banded pencil at a complex energy: (H_l - i W - z S) x = b, and projections p^T x.
//
// The stationary layers answer at the box eigenvalues only; everything of second order (dynamic polarizabilities, two-photon
// amplitudes, a Green's function between two packets) is otherwise a sum over every state of a channel.  The B-spline way is the
// perturbed function itself: one banded LU per energy, O(n k^2), the whole basis taking part, and with an absorber W the energy may
// lie anywhere in the continuum.  This is eigvec.hip::invit_body's factorisation -- one wavefront per matrix, the row window in
// registers, multipliers and pivot row by readlane, the window moved by a one-lane DPP shift, the entering row fetched a block
// ahead, no LDS and no barrier in the n dependent steps -- for the COMPLEX matrix
//     Re M(i,j) = H_l(i,j) - Re z S(i,j),     Im M(i,j) = -Im z S(i,j) - W(i,j),     |i - j| <= b = k - 1,
// with the caller's right-hand sides in place of the inverse iteration's own.
//
// Arithmetic, fixed: pivot by |Re| + |Im| (LAPACK's cabs1), ties to the smallest row; a complex product is the plain four-product
// form (ac - bd, ad + bc); one reciprocal per pivot (scaled by cabs1, so that it neither overflows nor underflows), kept in U's
// diagonal slot and multiplied with in the factorisation and in the back substitution.  The factorisation and the two substitutions
// are band_lu_wave.h's wave_lu_factor and wave_lu_solve with the policy WaveLuResolvent, the matrix comes in as RsPencil; the whole
// file is compiled with contraction off and every multiply-add is written out (DESIGN.md 4.7 "Fused products").  With Im z = 0, no absorber and real
// right-hand sides every imaginary part is a sum of products with a zero factor: +-0.0 throughout (G3 of include/bspatom.h).
// A matrix is one item, its right-hand sides are solved one after the other: nothing of an x depends on the other matrices, on the
// number of right-hand sides or projections, or on the slot that took the item (G2).
//
// Beyond second order the amplitudes are PRODUCTS of resolvents with an operator in between, p^T G(z2) A2 G(z1) A1 c: the second
// solve's right-hand side is the first one's solution.  resolvent_chain_kernel keeps such a chain on its wave: the same
// wave_lu_factor and wave_lu_solve per stage, and between the stages rs_band_apply, y = (sum_o a_o G_o) x in fixed no-FMA arithmetic (C1 - C6 of
// include/bspatom.h: a stage is bit for bit what resolvent_kernel gives for that right-hand side).  What this file shares with
// resolvent_coupled.hip and resolvent_wide.hip -- the pivot rule, the reciprocal -- is in resolvent_shared.h.
#include "common.h"
#include "wave_ops.h"
#include "resolvent_shared.h"
#include "band_lu_wave.h"
#include "resolvent_pencil.h"

#pragma clang fp contract(off)             // every multiply-add of this file is written out

namespace bsp {
namespace {
constexpr int RS_BMAX = 15;                // half-bandwidth limit (k <= 16)
// (sums of wave_ops.h: wave_sum32 over lanes 0 .. 31 -- the callers' terms are zero beyond lane 2 b <= 30 --, wave_sum over all)
// (the slot's scratch rs_slot_doubles and the matrix of an item, RsPencil: resolvent_pencil.h, which spline_window.hip includes too)

// y <- A x, A = sum_o ac[o] G_o: the right-hand side of a chain's next stage (include/bspatom.h: bspatom_resolvent_chain).  GB: nop
// full bands [2b+1][n], GB[(d + b) n + i] = G(i, i + d).  Lane-strided over the rows; an entry is t = ac[0] G_0, then t = t + ac[o] G_o
// for o ascending; y_re(i), y_im(i) start at +0.0 and add t x_re(i + d), t x_im(i + d) for d ascending, columns outside 0 .. n-1
// skipped.  IEEE multiplies and adds in the order written, NOTHING contracted (as in the whole file):
// opmat.hip::band_combine_apply_kernel's arithmetic on the two components.  x and y are distinct vectors of the slot; the caller has
// made x visible (rs_sync) and makes y visible.
// A row's loads are independent of each other and issued together by blocks of CH diagonals -- the block's entries of one operator,
// then its entries of x -- so a row costs 3 (nop + 1) memory round trips at most, not (2b + 1)(nop + 1): every address is clamped
// into its array (diagonals beyond 2b, columns outside the matrix) and what was loaded there is dropped by a select, never added.
template <int BT>
__device__ __forceinline__ void rs_band_apply(int n, int b, int nop, const double *__restrict__ GB, const double *__restrict__ ac,
                                              const double2 *x, double2 *y, const int lane)
{
    constexpr int CH = (2 * BT + 1 + 2) / 3;                   // 6 of 17 diagonals (BT = 8), 11 of 31 (BT = 15)
    const int nd = 2 * b + 1;
    const size_t cs = (size_t)nd * n;
    for (int i = lane; i < n; i += 64) {
        double yr = 0.0, yi = 0.0;
        // three blocks of diagonals, so that the loaded entries stay within the registers the factorisation needs anyway
#pragma unroll 1
        for (int d0 = 0; d0 < nd; d0 += CH) {
            double t[CH];
            double2 xv[CH];
            const double a0 = ac[0];
#pragma unroll
            for (int u = 0; u < CH; ++u) t[u] = a0 * GB[(size_t)(d0 + u < nd ? d0 + u : nd - 1) * n + i];
            for (int o = 1; o < nop; ++o) {
                const double ao = ac[o];
                const double *G = GB + (size_t)o * cs;
#pragma unroll
                for (int u = 0; u < CH; ++u) t[u] = t[u] + ao * G[(size_t)(d0 + u < nd ? d0 + u : nd - 1) * n + i];
            }
#pragma unroll
            for (int u = 0; u < CH; ++u) {
                const int j = i + d0 + u - b;
                xv[u] = x[j < 0 ? 0 : (j >= n ? n - 1 : j)];
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
    }
}
}  // namespace

// A PERSISTENT grid of single-wave workgroups, one per work slot, takes the matrices by a static stride (invit_batch_kernel's
// scheduling: bounded work per item, nobody waits for anybody -- a wrong residency estimate costs speed, never progress).
// Slot scratch: U [n][2b+1], L [n][b], y [n] complex, then piv [n] ints (resolvent_slot_doubles).
template <int BT>
__global__ __launch_bounds__(64) void resolvent_kernel(const ResolventArgs a)
{
    const int b = a.k - 1;
    double *work = a.work + (size_t)blockIdx.x * rs_slot_doubles(a.n, a.k);
    for (int it = blockIdx.x; it < a.nmat; it += gridDim.x) {
        // the operands made new values in every item, so that nothing hoisted out of the bodies stays live across the items
        // (eigvec.hip::invit_batch_kernel; the asm emits no instruction)
        int n = a.n, lane = threadIdx.x;
        const double *sb = a.SB, *hb = a.HB, *wb = a.WB;
        double *wk = work;
        asm volatile("" : "+s"(n), "+s"(sb), "+s"(hb), "+s"(wb), "+s"(wk), "+v"(lane));
        double2 *U = reinterpret_cast<double2 *>(wk), *Lm = U + (size_t)n * (2 * b + 1), *y = Lm + (size_t)n * b;
        int *piv = reinterpret_cast<int *>(y + n);
        const int wsel = a.w ? a.w[it] : -1;
        const double *wband = (wb && wsel >= 0) ? wb + (size_t)wsel * (2 * b + 1) * n : nullptr;
        const RsPencil e = {sb, hb + (size_t)a.chan[it] * a.k * n, wband, n, b, a.z[2 * it], a.z[2 * it + 1]};
        const int nper = wave_lu_factor<BT, WaveLuResolvent>(n, b, e, U, Lm, piv, lane);
        if (lane == 0) a.info[it] = nper;
        for (int r = 0; r < a.nrhs; ++r) {
            // (the caller's arrays are read and written as doubles: the ABI promises no more than their alignment)
            const double *B = a.B + (size_t)2 * r * n;
            for (int j = lane; j < n; j += 64) y[j] = make_double2(B[2 * j], B[2 * j + 1]);
            rs_sync();                                               // y, and with the first right-hand side U, L, piv, are in memory
            wave_lu_solve<WaveLuResolvent>(n, b, U, Lm, piv, y, lane);
            const size_t mr = (size_t)it * a.nrhs + r;
            if (a.X) {
                double *X = a.X + 2 * mr * n;
                for (int j = lane; j < n; j += 64) { const double2 v = y[j]; X[2 * j] = v.x; X[2 * j + 1] = v.y; }
            }
            if (a.R)
                for (int q = 0; q < a.nproj; ++q) {
                    // bilinear, no conjugate: lane-strided partial sums, then the wave's fixed tree
                    const double *P = a.P + (size_t)2 * q * n;
                    double sr = 0.0, si = 0.0;
                    for (int j = lane; j < n; j += 64) {
                        const double2 pv = make_double2(P[2 * j], P[2 * j + 1]), xv = y[j];
                        sr = sr + __builtin_fma(pv.x, xv.x, -(pv.y * xv.y));
                        si = si + __builtin_fma(pv.y, xv.x, pv.x * xv.y);
                    }
                    sr = wave_sum(sr); si = wave_sum(si);
                    if (lane == 0) { a.R[2 * (mr * a.nproj + q)] = sr; a.R[2 * (mr * a.nproj + q) + 1] = si; }
                }
            rs_sync();                                               // every load of y is back before the next right-hand side overwrites it
        }
    }
}

// Chains of resolvents, p^T G(z_s) A_s ... G(z_1) A_1 b: the same persistent grid, the CHAINS taken by the static stride, a chain
// on its wave from the first factorisation to the last projection.  A stage is resolvent_kernel's item -- wave_lu_factor, then per
// right-hand side the load of y, wave_lu_solve, X (last stage), the projections -- with y loaded from B at stage 0 and from
// rs_band_apply of the previous stage's solution otherwise; one factorisation serves the nrhs right-hand sides of its stage, so the
// slot keeps nrhs previous vectors.  Slot scratch: resolvent_kernel's (U, L, y, piv: rs_slot_doubles, even), then xp [nrhs][n] complex.
// nstage = 1 is resolvent_kernel statement for statement.
template <int BT>
__global__ __launch_bounds__(64) void resolvent_chain_kernel(const ResolventChainArgs a)
{
    const int b = a.k - 1;
    double *work = a.work + (size_t)blockIdx.x * (rs_slot_doubles(a.n, a.k) + (size_t)2 * a.nrhs * a.n);
    for (int c = blockIdx.x; c < a.nchain; c += gridDim.x)
        for (int s = 0; s < a.nstage; ++s) {
            // the operands made new values in every item, so that nothing hoisted out of the bodies stays live across the stages
            // (resolvent_kernel; the asm emits no instruction)
            int n = a.n, lane = threadIdx.x;
            const double *sb = a.SB, *hb = a.HB, *wb = a.WB, *gb = a.GB;
            double *wk = work;
            asm volatile("" : "+s"(n), "+s"(sb), "+s"(hb), "+s"(wb), "+s"(gb), "+s"(wk), "+v"(lane));
            double2 *U = reinterpret_cast<double2 *>(wk), *Lm = U + (size_t)n * (2 * b + 1), *y = Lm + (size_t)n * b;
            int *piv = reinterpret_cast<int *>(y + n);
            double2 *xp = reinterpret_cast<double2 *>(wk + rs_slot_doubles(n, a.k));
            const size_t it = (size_t)c * a.nstage + s;
            const int wsel = a.w ? a.w[it] : -1;
            const double *wband = (wb && wsel >= 0) ? wb + (size_t)wsel * (2 * b + 1) * n : nullptr;
            const RsPencil e = {sb, hb + (size_t)a.chan[it] * a.k * n, wband, n, b, a.z[2 * it], a.z[2 * it + 1]};
            const int nper = wave_lu_factor<BT, WaveLuResolvent>(n, b, e, U, Lm, piv, lane);
            if (lane == 0) a.info[it] = nper;
            const bool last = s + 1 == a.nstage;
            for (int r = 0; r < a.nrhs; ++r) {
                if (s == 0) {
                    const double *B = a.B + (size_t)2 * r * n;
                    for (int j = lane; j < n; j += 64) y[j] = make_double2(B[2 * j], B[2 * j + 1]);
                } else {
                    rs_band_apply<BT>(n, b, a.nop, gb, a.acoef + ((size_t)c * (a.nstage - 1) + (s - 1)) * a.nop, xp + (size_t)r * n, y, lane);
                }
                rs_sync();                                           // y, and with the first right-hand side U, L, piv, are in memory
                wave_lu_solve<WaveLuResolvent>(n, b, U, Lm, piv, y, lane);
                if (a.X && last) {
                    double *X = a.X + 2 * ((size_t)c * a.nrhs + r) * n;
                    for (int j = lane; j < n; j += 64) { const double2 v = y[j]; X[2 * j] = v.x; X[2 * j + 1] = v.y; }
                }
                const size_t mr = it * a.nrhs + r;
                if (a.R)
                    for (int q = 0; q < a.nproj; ++q) {
                        // bilinear, no conjugate: lane-strided partial sums, then the wave's fixed tree
                        const double *P = a.P + (size_t)2 * q * n;
                        double sr = 0.0, si = 0.0;
                        for (int j = lane; j < n; j += 64) {
                            const double2 pv = make_double2(P[2 * j], P[2 * j + 1]), xv = y[j];
                            sr = sr + __builtin_fma(pv.x, xv.x, -(pv.y * xv.y));
                            si = si + __builtin_fma(pv.y, xv.x, pv.x * xv.y);
                        }
                        sr = wave_sum(sr); si = wave_sum(si);
                        if (lane == 0) { a.R[2 * (mr * a.nproj + q)] = sr; a.R[2 * (mr * a.nproj + q) + 1] = si; }
                    }
                // x stays for the next stage: each lane's own rows, visible to the others after the wait
                if (!last)
                    for (int j = lane; j < n; j += 64) xp[(size_t)r * n + j] = y[j];
                rs_sync();                                           // every load of y is back before the next right-hand side overwrites it
            }
        }
}

size_t resolvent_slot_doubles(int n, int k) { return rs_slot_doubles(n, k); }
size_t resolvent_chain_slot_doubles(int n, int k, int nrhs) { return rs_slot_doubles(n, k) + (size_t)2 * nrhs * n; }

int resolvent_chain_slots(int k, int nchain, int *slots)
{
    if (k - 1 > RS_BMAX || k < 2 || nchain < 1) return BSP_ERR_ARG;
    if (k - 1 <= 8) return persistent_slots(resolvent_chain_kernel<8>, 64, 0, nchain, slots);
    return persistent_slots(resolvent_chain_kernel<RS_BMAX>, 64, 0, nchain, slots);
}

int launch_resolvent_chain(const ResolventChainArgs &a, int slots, hipStream_t st)
{
    if (a.k - 1 > RS_BMAX || a.k < 2 || a.n < 1 || a.nchain < 1 || a.nstage < 1 || a.nrhs < 1 || slots < 1) return BSP_ERR_ARG;
    if (a.nstage > 1 && (a.nop < 1 || !a.GB || !a.acoef)) return BSP_ERR_ARG;
    if (a.k - 1 <= 8) hipLaunchKernelGGL(resolvent_chain_kernel<8>, dim3(slots), dim3(64), 0, st, a);
    else hipLaunchKernelGGL(resolvent_chain_kernel<RS_BMAX>, dim3(slots), dim3(64), 0, st, a);
    BSP_HIP(hipGetLastError());
    return BSP_OK;
}

int resolvent_slots(int k, int nmat, int *slots)
{
    if (k - 1 > RS_BMAX || k < 2 || nmat < 1) return BSP_ERR_ARG;
    if (k - 1 <= 8) return persistent_slots(resolvent_kernel<8>, 64, 0, nmat, slots);
    return persistent_slots(resolvent_kernel<RS_BMAX>, 64, 0, nmat, slots);
}

int launch_resolvent(const ResolventArgs &a, int slots, hipStream_t st)
{
    if (a.k - 1 > RS_BMAX || a.k < 2 || a.n < 1 || a.nmat < 1 || a.nrhs < 1 || slots < 1) return BSP_ERR_ARG;
    if (a.k - 1 <= 8) hipLaunchKernelGGL(resolvent_kernel<8>, dim3(slots), dim3(64), 0, st, a);
    else hipLaunchKernelGGL(resolvent_kernel<RS_BMAX>, dim3(slots), dim3(64), 0, st, a);
    BSP_HIP(hipGetLastError());
    return BSP_OK;
}

}  // namespace bsp
