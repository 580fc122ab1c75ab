// tdse_spline_wide.hip -- the TDSE in the B-spline basis for WIDE bands: the Crank-Nicolson steps of tdse_spline.hip on the blocked
// banded LU of resolvent_wide.hip, half-width nch k - 1 up to 255 (include/bspatom_tdse_spline.h: bspatom_tdse_spline_wide).
//
// The step is tdse_spline.hip's: M_n = A_n - z S, z = 2 i / dt, c_{n+1} = -(4 i / dt) M_n^-1 (S c_n) - c_n.  Its own parts -- b = S c,
// the row of an observed step, the update -- are tdse_spline_steps.h's, the ones tdse_spline_kernel runs; the matrix, its
// factorisation and the solve are resolvent_wide_lu.h's, the ones resolvent_wide_kernel runs, with ONE right-hand side: the slot's
// vector y holds b, is eliminated with every panel and comes back as x.  tdse_spline_wide_kernel keeps a packet on ONE workgroup
// from the first step of a launch to its last: nothing goes to the host between steps, no workgroup waits for another, there are
// no atomics.
//
// A step, by a workgroup of resolvent_wide_kernel's shape on a slot of its scratch (rw_slot_doubles(N, bw, 1)):
//   1. b = S c into the slot's y (ts_rhs); on an observed step the row from b (ts_row; its reduction words are the layout's pred);
//   2. rw_assemble with the step's coefficients and the barrier that puts the band and b in memory; rw_pertol;
//   3. rw_factor with nrhs = 1, rw_backsolve;
//   4. the update (ts_update) and the snapshot when due.
// A wide step is slow -- tens to hundreds of milliseconds -- so the host keeps launches shorter than tdse_spline.hip's 64 steps
// (capi_spline.hip: the launch-length rule).
#include "common.h"
#include "wave_ops.h"
#include "resolvent_shared.h"
#include "resolvent_wide_lu.h"
#include "tdse_spline_steps.h"
#include "../../include/bspatom.h"

namespace bsp {

// A PERSISTENT grid of workgroups, one per work slot, takes the scans by static stride and runs the launch's steps of a scan one
// after the other.
__global__ __launch_bounds__(RW_NT) void tdse_spline_wide_kernel(const TdseSplineArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double tw_lds[];
    const int tid = threadIdx.x;
    const ResolventCoupledArgs &m = a.m;
    const int n = m.n, nch = m.nch, N = n * nch, bw = nch * m.k - 1, LD = 3 * bw + 1;
    const int RW = nch + 2 * m.nproj;
    const RwLds L = rw_lds_layout(tw_lds);
    double *work = m.work + (size_t)blockIdx.x * rw_slot_doubles(N, bw, 1);
    double2 *AB = reinterpret_cast<double2 *>(work), *y = AB + (size_t)N * LD;
    for (int q = blockIdx.x; q < a.nscan; q += gridDim.x) {
        double *c = a.c + (size_t)2 * q * N;
        int nper = 0;
        // step s = nst exists only in a launch that measures the packets it leaves (fin): it forms b and the row and ends there
        for (int s = 0; s < a.nst + (a.fin && a.obs ? 1 : 0); ++s) {
            const int nstep = a.n0 + s;
            const bool last = s == a.nst;
            ts_rhs<RW_NT>(n, nch, m.k - 1, m.SB, c, y, tid);
            if (last || (a.obs && nstep % a.obs_every == 0)) {
                const int j = last ? a.jfin : nstep / a.obs_every;
                __syncthreads();                                     // b is in memory
                ts_row<RW_NT>(n, nch, m.nproj, m.P, c, y, a.obs + ((size_t)(j - a.j0) * a.nscan + q) * RW, L.pred, tid);
            }
            if (last) {
                __syncthreads();                                     // every load of y is back before the next scan's b overwrites it
                break;
            }
            const double2 part = rw_assemble(m, 0, s * a.nscan + q, N, bw, AB, L, tid);
            __syncthreads();                                         // the band and b are in memory, pred is written
            const double pertol = rw_pertol(part, L);
            nper += rw_factor(N, bw, pertol, AB, 1, y, L, tid);
            __syncthreads();                                         // U and y are in memory
            rw_backsolve(N, bw, AB, 1, y, L, tid);
            __syncthreads();                                         // x is in memory; every load of the band is back before the next step assembles over it
            double *sn = nullptr;
            if (a.snap && (nstep + 1) % a.snap_every == 0)
                sn = a.snap + ((size_t)((nstep + 1) / a.snap_every - 1 - a.s0) * a.nscan + q) * 2 * N;
            ts_update<RW_NT>(n, nch, a.g, y, c, sn, tid);
            __syncthreads();                                         // the packet is in memory before the next step reads it across threads; y is free
        }
        if (tid == 0 && a.nst > 0) m.info[q] += nper;
    }
}

static int tw_allow_lds()
{
    static bool done = false;
    if (!done) {
        BSP_HIP(allow_lds(tdse_spline_wide_kernel, RW_LDS_BYTES));
        done = true;
    }
    return BSP_OK;
}

int tdse_spline_wide_slots(int k, int nch, int nscan, int *slots)
{
    if (k < 2 || nch < 1 || nscan < 1 || (long)nch * k - 1 > RW_BMAX) return BSP_ERR_ARG;
    int rc = tw_allow_lds();
    if (rc) return rc;
    return persistent_slots(tdse_spline_wide_kernel, RW_NT, RW_LDS_BYTES, nscan, slots);
}

int launch_tdse_spline_wide(const TdseSplineArgs &a, int slots, hipStream_t st)
{
    const ResolventCoupledArgs &m = a.m;
    if (m.k < 2 || m.n < 1 || m.nch < 1 || a.nscan < 1 || a.nst < 0 || slots < 1 || (long)m.nch * m.k - 1 > RW_BMAX || !a.c) return BSP_ERR_ARG;
    if (m.ncoup > 0 && (m.nop < 1 || !m.cr || !m.cc || !m.ctr || !m.GB || (a.nst > 0 && !m.acoef))) return BSP_ERR_ARG;
    if ((a.snap && a.snap_every < 1) || (a.obs && a.obs_every < 1) || (m.nproj > 0 && !m.P)) return BSP_ERR_ARG;
    int rc = tw_allow_lds();
    if (rc) return rc;
    hipLaunchKernelGGL(tdse_spline_wide_kernel, dim3(slots), dim3(RW_NT), RW_LDS_BYTES, st, a);
    BSP_HIP(hipGetLastError());
    return BSP_OK;
}

}  // namespace bsp
