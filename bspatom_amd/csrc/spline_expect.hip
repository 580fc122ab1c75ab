// spline_expect.hip -- expectation values on wave packets in the B-spline basis (include/bspatom_spline_expect.h: bspatom_spline_expect,
// and the rows bspatom_tdse_split_observe appends).
//
//     e(q, o) = sum_c conj(c_c)^T G_o u_{o,c},   u_{o,c} = sum_c' B_o(c, c') c_c'
//
// for nexp operators B_o (x) G_o: B_o a real nch x nch angular matrix of any pattern, G_o a real full band, symmetric or not.  With
// B = the matrix of cos theta and G = the band of r this is the induced dipole <z>, with the band of dV/dr the dipole acceleration.
//
// How: one wavefront per item (scan, operator, channel), a PERSISTENT grid of single-wave workgroups that takes the items by static
// stride, as the kernels of tdse_split.hip do.  An item
//   1. mixes u = sum_c' B(c, c') c_c' over the NON-ZERO entries of row c alone -- the host compacts every row into an index/value
//      list, cos theta couples two neighbours however many channels there are -- lane-strided over i, into the slot's scratch;
//   2. forms y(i) = sum_d G(i, i + d) u(i + d) for its rows, sp_overlap's way: a row's loads issued together by blocks of CH
//      diagonals, every address clamped into its array, what was loaded outside dropped by a select;
//   3. takes conj(c_c(i)) y(i) while y is in registers -- y is never stored --, lane-strided partial sums over each lane's rows
//      ascending, then the wave's fixed tree (wave_sum);
//   4. writes ONE partial per item with a vector store.
// The sum over the channels is a second small launch, one lane per (scan, operator), ascending from +0.0: the partials of one
// (scan, operator) come from different workgroups, and a kernel boundary is the one ordering between workgroups that needs no wait, no
// atomic and no progress word.
//
// The neighbours u(i + d) come from the slot's scratch in global memory, not from LDS or DPP: the scratch holds any n (LDS would cap
// n and the waves per CU with it), the rows of a lane are 64 apart, so a DPP shift would have to carry every block of 64 rows and its
// two neighbours in registers through 2k - 2 shifts, and the reads here are coalesced 16-byte loads of 16 n bytes the wave has just
// written: they are served by the cache next to the CU.  Nothing in an item is a dependent chain of length n.
//
// Every sum whose order the header fixes is written without FMA: the file is compiled with contraction off.
#include "common.h"
#include "wave_ops.h"
#include "resolvent_shared.h"

#pragma clang fp contract(off)

namespace bsp {
namespace {
// diagonals whose loads are in flight together: 6 keeps the kernel at 53 VGPRs, eight waves per SIMD (8: 65 VGPRs, one wave fewer),
// and walks k = 9's 17 diagonals in three blocks with one idle place
constexpr int SE_CH = 6;

// u(i) = sum over the row's entries ascending of val * c_{idx}(i), from +0.0, multiply then add, Re and Im independently
__device__ __forceinline__ void se_mix(const int n, const int e0, const int e1, const int *__restrict__ cidx, const double *__restrict__ cval,
                                       const double2 *in, double2 *u, const int lane)
{
    for (int i = lane; i < n; i += 64) {
        double ur = 0.0, ui = 0.0;
        for (int e = e0; e < e1; ++e) {
            const double bv = cval[e];
            const double2 x = in[(size_t)cidx[e] * n + i];
            ur = ur + bv * x.x;
            ui = ui + bv * x.y;
        }
        u[i] = make_double2(ur, ui);
    }
}

// this lane's part of sum_i conj(cv(i)) y(i), y = G u by rule 1 of include/bspatom_tdse_spline.h on a FULL band G[(d + b) n + i] =
// G(i, i + d): d = -b .. b ascending from +0.0, columns outside 0 .. n-1 skipped.  u is visible to the wave.
__device__ __forceinline__ double2 se_band_dot(const int n, const int b, const double *__restrict__ G, const double2 *u, const double2 *cv,
                                               const int lane)
{
    const int nd = 2 * b + 1;
    double sr = 0.0, si = 0.0;
    for (int i = lane; i < n; i += 64) {
        double yr = 0.0, yi = 0.0;
#pragma unroll 1
        for (int d0 = 0; d0 < nd; d0 += SE_CH) {
            double t[SE_CH];
            double2 xv[SE_CH];
#pragma unroll
            for (int w = 0; w < SE_CH; ++w) {
                const int j = i + d0 + w - b;
                const bool in = d0 + w < nd && j >= 0 && j < n;
                t[w] = G[in ? (size_t)(d0 + w) * n + i : 0];
            }
#pragma unroll
            for (int w = 0; w < SE_CH; ++w) {
                const int j = i + d0 + w - b;
                xv[w] = u[j < 0 ? 0 : (j >= n ? n - 1 : j)];
            }
#pragma unroll
            for (int w = 0; w < SE_CH; ++w) {
                const int j = i + d0 + w - b;
                const bool in = d0 + w < nd && j >= 0 && j < n;
                const double vr = yr + t[w] * xv[w].x, vi = yi + t[w] * xv[w].y;
                yr = in ? vr : yr;
                yi = in ? vi : yi;
            }
        }
        const double2 cc = cv[i];
        sr = sr + (cc.x * yr + cc.y * yi);
        si = si + (cc.x * yi - cc.y * yr);
    }
    return make_double2(sr, si);
}
}  // namespace

// One partial per item (scan q, operator o, channel ch): part[(q nexp + o) nch + ch] = conj(c_ch)^T G_o u_{o,ch}.  A row of B with
// no non-zero entry gives (+0.0, +0.0) without reading the packets.
__global__ __launch_bounds__(64) void spline_expect_kernel(const SplineExpectArgs a)
{
    const int nch = a.nch, nexp = a.nexp, b = a.k - 1;
    const int items = a.nscan * nexp * nch;
    for (int it = blockIdx.x; it < items; it += gridDim.x) {
        const int n = a.n, lane = threadIdx.x;
        double2 *u = reinterpret_cast<double2 *>(a.work + (size_t)blockIdx.x * 2 * (size_t)n);   // spline_expect_slot_doubles
        const int qo = it / nch, ch = it - qo * nch, q = qo / nexp, o = qo - q * nexp;
        const int e0 = a.rptr[o * nch + ch], e1 = a.rptr[o * nch + ch + 1];
        double2 *out = reinterpret_cast<double2 *>(a.part) + it;
        if (e0 == e1) {                                              // uniform
            if (lane == 0) *out = make_double2(0.0, 0.0);
            continue;
        }
        const double2 *in = reinterpret_cast<const double2 *>(a.c) + (size_t)q * nch * n;
        se_mix(n, e0, e1, a.cidx, a.cval, in, u, lane);
        rs_sync();                                                   // u is in memory
        double2 s = se_band_dot(n, b, a.GE + (size_t)o * (2 * b + 1) * n, u, in + (size_t)ch * n, lane);
        s.x = wave_sum(s.x); s.y = wave_sum(s.y);
        if (lane == 0) *out = s;
        rs_sync();                                                   // every load of the slot is back before the next item overwrites it
    }
}

// e(q, o) = sum over the channels ascending, from +0.0, of the partials: one lane per (scan, operator)
__global__ __launch_bounds__(64) void spline_expect_sum_kernel(const SplineExpectArgs a)
{
    const int qo = blockIdx.x * 64 + threadIdx.x;
    if (qo >= a.nscan * a.nexp) return;
    const double2 *pt = reinterpret_cast<const double2 *>(a.part) + (size_t)qo * a.nch;
    double sr = 0.0, si = 0.0;
    for (int c = 0; c < a.nch; ++c) {
        const double2 v = pt[c];
        sr = sr + v.x;
        si = si + v.y;
    }
    a.e[2 * (size_t)qo] = sr; a.e[2 * (size_t)qo + 1] = si;       // the caller's array: doubles, the ABI promises no more than their alignment
}

// The rows of bspatom_tdse_split_observe: row r of out, rw0 + 2 nexp wide, is row r of row0 (rw0 wide, what the kernels of
// tdse_split.hip wrote) followed by row r of e (2 nexp wide).  Copies, no arithmetic.
__global__ __launch_bounds__(64) void spline_expect_rows_kernel(double *out, const double *row0, const double *e, const int rw0, const int ne2,
                                                                const int nrows)
{
    const int rw = rw0 + ne2;
    for (int r = blockIdx.x; r < nrows; r += gridDim.x)
        for (int j = threadIdx.x; j < rw; j += 64)
            out[(size_t)r * rw + j] = j < rw0 ? row0[(size_t)r * rw0 + j] : e[(size_t)r * ne2 + (j - rw0)];
}

// doubles of one slot's scratch: u [n] complex
size_t spline_expect_slot_doubles(int n) { return 2 * (size_t)n; }

int spline_expect_slots(int items, int *slots)
{
    if (items < 1) return BSP_ERR_ARG;
    return persistent_slots(spline_expect_kernel, 64, 0, items, slots);
}

// the two launches of one measurement: the partials, then the sums over the channels
int launch_spline_expect(const SplineExpectArgs &a, int slots, hipStream_t st)
{
    if (a.n < 1 || a.k < 1 || a.nch < 1 || a.nscan < 1 || a.nexp < 1 || slots < 1) return BSP_ERR_ARG;
    if (!a.GE || !a.rptr || !a.cidx || !a.cval || !a.c || !a.part || !a.e || !a.work) return BSP_ERR_ARG;
    hipLaunchKernelGGL(spline_expect_kernel, dim3(slots), dim3(64), 0, st, a);
    hipLaunchKernelGGL(spline_expect_sum_kernel, dim3((a.nscan * a.nexp + 63) / 64), dim3(64), 0, st, a);
    BSP_HIP(hipGetLastError());
    return BSP_OK;
}

int launch_spline_expect_rows(double *out, const double *row0, const double *e, int rw0, int nexp, int nrows, hipStream_t st)
{
    if (!out || !row0 || !e || rw0 < 1 || nexp < 1 || nrows < 1) return BSP_ERR_ARG;
    hipLaunchKernelGGL(spline_expect_rows_kernel, dim3(nrows < 1024 ? nrows : 1024), dim3(64), 0, st, out, row0, e, rw0, 2 * nexp, nrows);
    BSP_HIP(hipGetLastError());
    return BSP_OK;
}

}  // namespace bsp
