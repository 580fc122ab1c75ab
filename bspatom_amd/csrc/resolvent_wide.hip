// resolvent_wide.hip -- the coupled-channel resolvent for WIDE bands: the system of resolvent_coupled.hip, half-width bw = nch k - 1 up
// to 255, in a BLOCKED banded LU with partial pivoting (include/bspatom.h: bspatom_resolvent_coupled_wide).
//
// resolvent_coupled.hip keeps the whole row window in LDS and the pivot candidates of a column in one wavefront: bw <= 63.  Here the
// band lives in the slot's global scratch (the active window, about (bw + NB) x (2 bw + NB) complex, stays in L2) and a workgroup
// works through it in PANELS of NB = 16 columns:
//
//   storage   LAPACK ZGBTRF's column band with kl extra superdiagonals: column c holds the rows c - 2 bw .. c + bw, contiguous,
//             M(i, c) at AB[c (3 bw + 1) + (i - c + 2 bw)].  A row interchange never leaves it.
//   panel     the at most bw + NB rows of the NB columns j0 .. j0 + NB - 1, in LDS as two real planes (the layout the matrix cores
//             read).  Factored there column by column: the pivot of a column is the largest |Re| + |Im| over ALL of its at most
//             bw + 1 <= 256 candidates, ties to the smallest row -- waves 0 .. 3 take 64 candidates each (the DPP maximum and a
//             ballot, resolvent_coupled.hip's), leave (maximum, row, value) in LDS, and every thread combines the four in ascending
//             order; one reciprocal per pivot (rs_pivot_recip, resolvent.hip's); the rows change places across the WHOLE panel, so that
//             P A = L U holds for the panel as a block; a thread per row scales its multiplier and updates its row of the panel.
//   right     the interchanges of the panel as ONE gather per column (a thread per column of the at most 2 bw to the right):
//             U12 = L11^-1 A12 on plain FMAs in registers, written back and staged in LDS; then A22 -= L21 U12 on
//             v_mfma_f64_16x16x4_f64, a wave per 16 x 16 tile, the complex product as four real ones, the contraction over the
//             panel's 16 columns in ascending order.  Columns are taken in chunks of at most 256 (the LDS image of U12).
//   vectors   the right-hand sides are eliminated WITH the panel (all of them are known up front; L is never stored): the window
//             of y in LDS, the panel's interchanges, L11^-1 on one wave, the rows below a thread each.  The backward pass runs
//             block by block over the same 16 columns: the triangle on one wave per right-hand side (eight at a time), the at most
//             2 bw rows above a thread each.  Every sum runs over the 16 columns of a block in ascending order.
//
// No workgroup waits on another: the only synchronisation is the barrier of the workgroup.  The tiles, chunks and blocks depend on
// (N, bw) alone.  Arithmetic and guarantees: K1 - K4 of include/bspatom.h, as resolvent_coupled.hip; with Im z = 0, no absorber,
// real coefficients and real B every imaginary accumulator, on the matrix cores too, sums products with a zero factor.
#include "common.h"
#include "wave_ops.h"
#include "resolvent_shared.h"
#include "resolvent_wide_lu.h"
#include "../../include/bspatom.h"

namespace bsp {

// A PERSISTENT grid of workgroups, one per work slot, takes the matrices by resolvent_kernel's static stride.  The phases are
// resolvent_wide_lu.h's, shared with tdse_spline_wide_kernel.
__global__ __launch_bounds__(RW_NT) void resolvent_wide_kernel(const ResolventCoupledArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double rw_lds[];
    const int tid = threadIdx.x;
    const int n = a.n, nch = a.nch, N = n * nch, bw = nch * a.k - 1, LD = 3 * bw + 1;
    const RwLds L = rw_lds_layout(rw_lds);
    double *work = a.work + (size_t)blockIdx.x * rw_slot_doubles(N, bw, a.nrhs);
    double2 *AB = reinterpret_cast<double2 *>(work), *y = AB + (size_t)N * LD;
    for (int it = blockIdx.x; it < a.nmat; it += gridDim.x) {
        // the band, column by column; the scale of the zero-pivot perturbation from its diagonal (rs_pertol)
        const double2 part = rw_assemble(a, it, it, N, bw, AB, L, tid);
        // the right-hand sides, into the ordering of the matrix
        for (int r = 0; r < a.nrhs; ++r) rc_load_rhs<RW_NT>(n, nch, a.B + (size_t)2 * r * N, y + (size_t)r * N, tid);
        __syncthreads();                                             // the band and the vectors are in memory, pred is written
        const double pertol = rw_pertol(part, L);
        const int nper = rw_factor(N, bw, pertol, AB, a.nrhs, y, L, tid);
        if (tid == 0) a.info[it] = nper;
        __syncthreads();
        // ---- x <- U^-1 y
        rw_backsolve(N, bw, AB, a.nrhs, y, L, tid);
        // ---- X and the projections, as resolvent_coupled.hip
        for (int r = 0; r < a.nrhs; ++r) {
            const double2 *yy = y + (size_t)r * N;
            const size_t mr = (size_t)it * a.nrhs + r;
            if (a.X) rc_store_x<RW_NT>(n, nch, yy, a.X + 2 * mr * N, tid);
            if (a.R) rc_project<RW_NT>(n, nch, a.nproj, a.P, yy, a.R + 2 * mr * a.nproj, L.pred, tid);
        }
        __syncthreads();                                             // every load of the band and of y is back before the next matrix
    }
}

int resolvent_wide_max_band() { return RW_BMAX; }
size_t resolvent_wide_slot_doubles(int n, int k, int nch, int nrhs) { return rw_slot_doubles(n * nch, nch * k - 1, nrhs); }

static int rw_allow_lds()
{
    static bool done = false;
    if (!done) {
        BSP_HIP(allow_lds(resolvent_wide_kernel, RW_LDS_BYTES));
        done = true;
    }
    return BSP_OK;
}

int resolvent_wide_slots(int k, int nch, int nmat, int *slots)
{
    if (k < 2 || nch < 1 || nmat < 1 || (long)nch * k - 1 > RW_BMAX) return BSP_ERR_ARG;
    int rc = rw_allow_lds();
    if (rc) return rc;
    return persistent_slots(resolvent_wide_kernel, RW_NT, RW_LDS_BYTES, nmat, slots);
}

int launch_resolvent_wide(const ResolventCoupledArgs &a, int slots, hipStream_t st)
{
    if (a.k < 2 || a.n < 1 || a.nch < 1 || a.nmat < 1 || a.nrhs < 1 || slots < 1 || (long)a.nch * a.k - 1 > RW_BMAX) return BSP_ERR_ARG;
    if (a.ncoup > 0 && (a.nop < 1 || !a.cr || !a.cc || !a.ctr || !a.GB || !a.acoef)) return BSP_ERR_ARG;
    int rc = rw_allow_lds();
    if (rc) return rc;
    hipLaunchKernelGGL(resolvent_wide_kernel, dim3(slots), dim3(RW_NT), RW_LDS_BYTES, st, a);
    BSP_HIP(hipGetLastError());
    return BSP_OK;
}

}  // namespace bsp
