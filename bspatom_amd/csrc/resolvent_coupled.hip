// resolvent_coupled.hip -- the coupled-channel resolvent: (sum_c (H_{l_c} - i W_c - z_c S) + V) x = b across nch channels in ONE
// banded LU (include/bspatom.h: bspatom_resolvent_coupled).
//
// resolvent.hip answers for one channel at a time and its chains multiply such answers: perturbation theory.  A coupling to all
// orders -- a static field, a Floquet block matrix, any potential that mixes l -- is one linear system whose matrix, with the
// unknowns ordered basis index first and channel second (unknown (i, c) at position i nch + c), is banded again: half-width
// bw = nch k - 1.  That is too wide for the one-wave register window of resolvent.hip (bw <= 15), so here a WORKGROUP factors a
// matrix, the row window in LDS:
//
//   rows j .. j + bw of the columns j .. j + 2 bw, (bw + 1) x (2 bw + 1) complex, as a ring in both directions (row r in slot
//   r mod (bw + 1), column c in slot c mod (2 bw + 1)): nothing is ever shifted, the slot of the row that leaves takes the row that
//   enters, the slot of the column that was eliminated is the column that comes into reach, zero but in the entering row.
//
// A step (one column; RC_PANEL of resolvent_coupled_lu.h, where the assembly, the factorisation and the solve live: tdse_spline.hip
// runs the same statements): wave 0 finds the pivot among the at most bw + 1 <= 64 candidates -- one per lane --, forms the
// reciprocal and the multipliers, copies the pivot row out (U, and a broadcast copy in LDS) and puts row j where the pivot row
// was; after a barrier all waves update the window, a wave per row, a lane per column, while the last two waves store the entering
// row, which they requested two steps ahead; a second barrier ends the step.  U rows, L multipliers and pivot indices stream
// to the slot's scratch; the solves run from there on wave 0 (forward: wave_lu_forward of band_lu_wave.h, resolvent.hip's register window on bw + 1 lanes; backward: the
// last 2 bw unknowns in an LDS ring, two per lane), one right-hand side after the other.
//
// The matrix is first ASSEMBLED, by all threads, into the rows of U itself -- row r of the band, columns r - bw .. r + bw, lies where
// U's row r will be written at step r, bw + 1 steps after the window has taken it -- so the entering row is one coalesced load and
// the generalisation of rs_entry (rc_entry: the diagonal-block formula or the sum over the block's coupling entries) runs once per
// entry, outside the dependent steps.
//
// Arithmetic, fixed (K1 - K4 of include/bspatom.h): pivot by |Re| + |Im|, ties to the smallest row; complex products in the plain
// four-product form; one reciprocal per pivot (rs_pivot_recip, resolvent.hip's); every sum in an order that depends on the matrix alone (no atomics;
// the workgroup's shape is a constant).  With Im z = 0, no absorber, real coefficients and real B every imaginary part is a sum of
// products with a zero factor.
#include "common.h"
#include "wave_ops.h"
#include "resolvent_shared.h"
#include "resolvent_coupled_lu.h"
#include "../../include/bspatom.h"

namespace bsp {

// A PERSISTENT grid of workgroups, one per work slot, takes the matrices by resolvent_kernel's static stride.
// Slot scratch: U [N][2bw+1], L [N][bw], y [N] complex, then piv [N] ints (rc_slot_doubles); N = nch n, bw = nch k - 1.
__global__ __launch_bounds__(RC_NT) void resolvent_coupled_kernel(const ResolventCoupledArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double2 rc_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int n = a.n, nch = a.nch, N = n * nch, bw = nch * a.k - 1, W = 2 * bw + 1;
    double2 *win = rc_lds, *prow = win + (size_t)(bw + 1) * W, *mult = prow + 128, *red = mult + 64;
    double *work = a.work + (size_t)blockIdx.x * rc_slot_doubles(N, bw);
    double2 *U = reinterpret_cast<double2 *>(work), *Lm = U + (size_t)N * W, *y = Lm + (size_t)N * bw;
    int *piv = reinterpret_cast<int *>(y + N);
    for (int it = blockIdx.x; it < a.nmat; it += gridDim.x) {
        const double pertol = rc_assemble(a, it, it, N, bw, U, red, tid);   // the band into U's rows, the zero-pivot scale
        const int nper = rc_factor(N, bw, pertol, U, Lm, piv, win, prow, mult, tid);
        if (tid == 0) a.info[it] = nper;
        for (int r = 0; r < a.nrhs; ++r) {
            rc_load_rhs<RC_NT>(n, nch, a.B + (size_t)2 * r * N, y, tid);
            __syncthreads();                                         // y, and with the first right-hand side U, L, piv, are in memory
            if (wv == 0) rc_solve(N, bw, U, Lm, piv, y, prow, lane);
            __syncthreads();
            const size_t mr = (size_t)it * a.nrhs + r;
            if (a.X) rc_store_x<RC_NT>(n, nch, y, a.X + 2 * mr * N, tid);
            if (a.R) rc_project<RC_NT>(n, nch, a.nproj, a.P, y, a.R + 2 * mr * a.nproj, red, tid);
            __syncthreads();                                         // every load of y is back before the next right-hand side overwrites it
        }
    }
}

int resolvent_coupled_max_band() { return RC_BMAX; }
size_t resolvent_coupled_slot_doubles(int n, int k, int nch) { return rc_slot_doubles(n * nch, nch * k - 1); }

static int rc_allow_lds()
{
    static bool done = false;
    if (!done) {
        BSP_HIP(allow_lds(resolvent_coupled_kernel, rc_lds_bytes(RC_BMAX)));
        done = true;
    }
    return BSP_OK;
}

int resolvent_coupled_slots(int k, int nch, int nmat, int *slots)
{
    if (k < 2 || nch < 1 || nmat < 1 || (long)nch * k - 1 > RC_BMAX) return BSP_ERR_ARG;
    int rc = rc_allow_lds();
    if (rc) return rc;
    return persistent_slots(resolvent_coupled_kernel, RC_NT, rc_lds_bytes(nch * k - 1), nmat, slots);
}

int launch_resolvent_coupled(const ResolventCoupledArgs &a, int slots, hipStream_t st)
{
    if (a.k < 2 || a.n < 1 || a.nch < 1 || a.nmat < 1 || a.nrhs < 1 || slots < 1 || (long)a.nch * a.k - 1 > RC_BMAX) return BSP_ERR_ARG;
    if (a.ncoup > 0 && (a.nop < 1 || !a.cr || !a.cc || !a.ctr || !a.GB || !a.acoef)) return BSP_ERR_ARG;
    int rc = rc_allow_lds();
    if (rc) return rc;
    hipLaunchKernelGGL(resolvent_coupled_kernel, dim3(slots), dim3(RC_NT), rc_lds_bytes(a.nch * a.k - 1), st, a);
    BSP_HIP(hipGetLastError());
    return BSP_OK;
}

}  // namespace bsp
