// tdse_spline.hip -- the TDSE in the B-spline basis itself: Crank-Nicolson steps of i S dc/dt = (sum_c (H_lc - i W_c) + V(t)) c on the
// coupled banded LU (include/bspatom_tdse_spline.h: bspatom_tdse_spline).
//
// With tau = dt / 2 and A_n the Hamiltonian at the step's midpoint, (S + i tau A_n) c_{n+1} = (S - i tau A_n) c_n is
//
//     M_n = A_n - z S,  z = 2 i / dt:      c_{n+1} = -(4 i / dt) M_n^-1 (S c_n) - c_n,
//
// and M_n is the matrix resolvent_coupled.hip assembles and factors: the channels' own bands, an absorber, complex coefficients on
// operator bands, half-width nch k - 1 <= 63.  What a time step adds to a coupled solve is its right-hand side -- b = S c_n, the
// packet's own, the result of the step before -- and the update.  tdse_spline_kernel keeps a packet on ONE workgroup from the
// first step of a launch to its last, as resolvent_chain_kernel keeps a chain on its wave: nothing goes to the host between steps,
// no workgroup waits for another, there are no atomics.
//
// A step, by a workgroup of resolvent_coupled_kernel's shape on a slot of its scratch (resolvent_coupled_lu.h):
//   1. b = S c into the slot's y, in the matrix's ordering (ts_rhs; the chain call's rule for y = A x with A = S, nothing contracted);
//      on an observed step the row from b: N_c = Re sum_i conj(c) b per channel and the projections p_r^T b (rc_project);
//   2. rc_assemble with the step's coefficients, rc_factor, rc_solve: the statements of resolvent_coupled_kernel;
//   3. c' = (g x_im - c_re, -(g x_re) - c_im), g = 4 / dt, one multiply and one subtract each (ts_update), and the snapshot when due.
// The packet lives in the caller's (or the staging) array; the slot holds nothing between steps, so a launch of any number of steps
// continues where the one before ended, and the host keeps launches short (tdse_spline_group).
#include "common.h"
#include "wave_ops.h"
#include "resolvent_shared.h"
#include "resolvent_coupled_lu.h"
#include "tdse_spline_steps.h"
#include "../../include/bspatom.h"

namespace bsp {

// A PERSISTENT grid of workgroups, one per work slot, takes the scans by static stride and runs the launch's steps of a scan one
// after the other.  Slot scratch: resolvent_coupled_kernel's (rc_slot_doubles).
__global__ __launch_bounds__(RC_NT) void tdse_spline_kernel(const TdseSplineArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double2 ts_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const ResolventCoupledArgs &m = a.m;
    const int n = m.n, nch = m.nch, N = n * nch, bw = nch * m.k - 1, W = 2 * bw + 1;
    const int RW = nch + 2 * m.nproj;
    double2 *win = ts_lds, *prow = win + (size_t)(bw + 1) * W, *mult = prow + 128, *red = mult + 64;
    double *work = m.work + (size_t)blockIdx.x * rc_slot_doubles(N, bw);
    double2 *U = reinterpret_cast<double2 *>(work), *Lm = U + (size_t)N * W, *y = Lm + (size_t)N * bw;
    int *piv = reinterpret_cast<int *>(y + N);
    for (int q = blockIdx.x; q < a.nscan; q += gridDim.x) {
        double *c = a.c + (size_t)2 * q * N;
        int nper = 0;
        // step s = nst exists only in a launch that measures the packets it leaves (fin): it forms b and the row and ends there
        for (int s = 0; s < a.nst + (a.fin && a.obs ? 1 : 0); ++s) {
            const int nstep = a.n0 + s;
            const bool last = s == a.nst;
            ts_rhs<RC_NT>(n, nch, m.k - 1, m.SB, c, y, tid);
            if (last || (a.obs && nstep % a.obs_every == 0)) {
                const int j = last ? a.jfin : nstep / a.obs_every;
                __syncthreads();                                     // b is in memory
                ts_row<RC_NT>(n, nch, m.nproj, m.P, c, y, a.obs + ((size_t)(j - a.j0) * a.nscan + q) * RW, red, tid);
            }
            if (last) {
                __syncthreads();                                     // every load of y is back before the next scan's b overwrites it
                break;
            }
            const double pertol = rc_assemble(m, 0, s * a.nscan + q, N, bw, U, red, tid);   // its barrier: b and the band are in memory
            nper += rc_factor(N, bw, pertol, U, Lm, piv, win, prow, mult, tid);
            __syncthreads();                                         // U, L, piv are in memory
            if (wv == 0) rc_solve(N, bw, U, Lm, piv, y, prow, lane);
            __syncthreads();
            double *sn = nullptr;
            if (a.snap && (nstep + 1) % a.snap_every == 0)
                sn = a.snap + ((size_t)((nstep + 1) / a.snap_every - 1 - a.s0) * a.nscan + q) * 2 * N;
            ts_update<RC_NT>(n, nch, a.g, y, c, sn, tid);
            __syncthreads();                                         // the packet is in memory before the next step reads it across threads
        }
        if (tid == 0 && a.nst > 0) m.info[q] += nper;
    }
}

static int ts_allow_lds()
{
    static bool done = false;
    if (!done) {
        BSP_HIP(allow_lds(tdse_spline_kernel, rc_lds_bytes(RC_BMAX)));
        done = true;
    }
    return BSP_OK;
}

int tdse_spline_slots(int k, int nch, int nscan, int *slots)
{
    if (k < 2 || nch < 1 || nscan < 1 || (long)nch * k - 1 > RC_BMAX) return BSP_ERR_ARG;
    int rc = ts_allow_lds();
    if (rc) return rc;
    return persistent_slots(tdse_spline_kernel, RC_NT, rc_lds_bytes(nch * k - 1), nscan, slots);
}

int launch_tdse_spline(const TdseSplineArgs &a, int slots, hipStream_t st)
{
    const ResolventCoupledArgs &m = a.m;
    if (m.k < 2 || m.n < 1 || m.nch < 1 || a.nscan < 1 || a.nst < 0 || slots < 1 || (long)m.nch * m.k - 1 > RC_BMAX || !a.c) return BSP_ERR_ARG;
    if (m.ncoup > 0 && (m.nop < 1 || !m.cr || !m.cc || !m.ctr || !m.GB || (a.nst > 0 && !m.acoef))) return BSP_ERR_ARG;
    if ((a.snap && a.snap_every < 1) || (a.obs && a.obs_every < 1) || (m.nproj > 0 && !m.P)) return BSP_ERR_ARG;
    int rc = ts_allow_lds();
    if (rc) return rc;
    hipLaunchKernelGGL(tdse_spline_kernel, dim3(slots), dim3(RC_NT), rc_lds_bytes(m.nch * m.k - 1), st, a);
    BSP_HIP(hipGetLastError());
    return BSP_OK;
}

}  // namespace bsp
