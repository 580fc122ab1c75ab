// spline_window.hip -- the window operator on wave packets in the B-spline basis (include/bspatom_spline_window.h:
// bspatom_spline_window): how a packet is distributed over energy, without an eigenvector.
//
//     P_m(E) = <c| gamma^(2m) / ((H - E)^(2m) + gamma^(2m)) |c> = gamma^(2m) x_m^H S x_m,    x_0 = c,   x_{j+1} = (H_l - z_j S)^-1 S x_j,
//
// z_j the m roots of the denominator in the upper half plane (the host's window_shifts; the kernel takes any z).  A stage is
// bspatom_resolvent's solve -- the matrix RsPencil without an absorber, band_lu_wave.h's wave_lu_factor and wave_lu_solve with the
// policy WaveLuResolvent -- on the right-hand side b = S x_j, which is tdse_split.hip's sp_overlap; the result is that function's
// norm, the N_ch of the spline rows.  Nothing here is arithmetic of this file's own: W3 and W5 of the header hold because the
// statements are shared.  The file is compiled with contraction off, like the two it composes.
//
// The matrices depend on (l, E, j) alone, the packets of a scan of nscan x nch are many: an ITEM is (energy e, distinct channel
// value g, block of at most window_rhs of g's right-hand sides), and the wave that takes it factors every stage ONCE for the
// block.  Between the stages the block's vectors stay in the slot.  Scheduling is resolvent_chain_kernel's: a persistent grid of
// single-wave workgroups takes the items by a static stride; nobody waits for anybody, no atomics, no LDS.
#include "common.h"
#include "wave_ops.h"
#include "resolvent_shared.h"
#include "band_lu_wave.h"
#include "resolvent_pencil.h"
#include "spline_overlap.h"

#pragma clang fp contract(off)

namespace bsp {
namespace {
constexpr int SW_BMAX = 15;                // half-bandwidth limit (k <= 16): the one-wave window's
}

// Slot scratch: resolvent_kernel's (U, L, y, piv: rs_slot_doubles, even), then x [wrhs][n] complex, the block's vectors.
// Stage s < nfac: the factorisation, then per right-hand side b = S x into y (x: the caller's packet at stage 0, the slot's vector
// after), the solve in place, y kept as the slot's vector.  "Stage" nfac measures: S x with the norm, one store per (q, c, e).
template <int BT>
__global__ __launch_bounds__(64) void spline_window_kernel(const SplineWindowArgs a)
{
    const int b = a.k - 1;
    double *work = a.work + (size_t)blockIdx.x * (rs_slot_doubles(a.n, a.k) + (size_t)2 * a.wrhs * a.n);
    for (int it = blockIdx.x; it < a.ne * a.nblk; it += gridDim.x) {
        const int e = it / a.nblk, blk = it - e * a.nblk;
        const int g = a.bg[blk], r0 = a.b0[blk], cnt = a.bn[blk];
        for (int s = 0; s <= a.nfac; ++s) {
            // the operands made new values in every stage, so that nothing hoisted out of the bodies stays live across the stages
            // (resolvent_chain_kernel; the asm emits no instruction)
            int n = a.n, lane = threadIdx.x;
            const double *sb = a.SB, *hb = a.HB;
            double *wk = work;
            asm volatile("" : "+s"(n), "+s"(sb), "+s"(hb), "+s"(wk), "+v"(lane));
            double2 *U = reinterpret_cast<double2 *>(wk), *Lm = U + (size_t)n * (2 * b + 1), *y = Lm + (size_t)n * b;
            int *piv = reinterpret_cast<int *>(y + n);
            double2 *xs = reinterpret_cast<double2 *>(wk + rs_slot_doubles(n, a.k));
            const bool measure = s == a.nfac;
            if (!measure) {
                const size_t zs = (size_t)e * a.nfac + s;
                const RsPencil m = {sb, hb + (size_t)a.gchan[g] * a.k * n, nullptr, n, b, a.z[2 * zs], a.z[2 * zs + 1]};
                const int nper = wave_lu_factor<BT, WaveLuResolvent>(n, b, m, U, Lm, piv, lane);
                // a factorisation counts once: the group's first block reports it
                if (lane == 0 && a.bhead[blk]) a.info[((size_t)e * a.ng + g) * a.nfac + s] = nper;
            }
            for (int r = 0; r < cnt; ++r) {
                const int idx = a.rhs[r0 + r];                       // q * nch + c
                const double2 *x = (s == 0) ? reinterpret_cast<const double2 *>(a.c) + (size_t)idx * n : xs + (size_t)r * n;
                double nrm = sp_overlap<BT>(n, b, sb, x, y, measure, lane);
                if (measure) {
                    nrm = wave_sum(nrm);
                    if (lane == 0) a.N[(size_t)idx * a.ne + e] = nrm;
                    continue;
                }
                rs_sync();                                           // y, and with the first right-hand side U, L, piv, are in memory
                wave_lu_solve<WaveLuResolvent>(n, b, U, Lm, piv, y, lane);
                // x stays for the next stage: each lane's own rows, visible to the others after the wait
                for (int j = lane; j < n; j += 64) xs[(size_t)r * n + j] = y[j];
                rs_sync();                                           // every load of y is back before the next right-hand side overwrites it
            }
        }
        rs_sync();                                                   // every load of the slot is back before the next item overwrites it
    }
}

size_t spline_window_slot_doubles(int n, int k, int wrhs) { return rs_slot_doubles(n, k) + (size_t)2 * wrhs * n; }

int spline_window_slots(int k, int items, int *slots)
{
    if (k - 1 > SW_BMAX || k < 2 || items < 1) return BSP_ERR_ARG;
    if (k - 1 <= 8) return persistent_slots(spline_window_kernel<8>, 64, 0, items, slots);
    return persistent_slots(spline_window_kernel<SW_BMAX>, 64, 0, items, slots);
}

int launch_spline_window(const SplineWindowArgs &a, int slots, hipStream_t st)
{
    if (a.k - 1 > SW_BMAX || a.k < 2 || a.n < 1 || a.ne < 1 || a.nblk < 1 || a.ng < 1 || a.nfac < 0 || a.wrhs < 1 || slots < 1) return BSP_ERR_ARG;
    if (a.k - 1 <= 8) hipLaunchKernelGGL(spline_window_kernel<8>, dim3(slots), dim3(64), 0, st, a);
    else hipLaunchKernelGGL(spline_window_kernel<SW_BMAX>, dim3(slots), dim3(64), 0, st, a);
    BSP_HIP(hipGetLastError());
    return BSP_OK;
}

}  // namespace bsp
