// tdse.hip -- the TDSE in the basis of the field-free eigenstates (bspatom_tdse_propagate):
//   i da_c/dt = E_c .* a_c + sum_{p: cf[p] = c} f_q(t) D_p^T a_{ci[p]} + sum_{p: ci[p] = c} conj(f_q(t)) D_p a_{cf[p]}
// for nscan wave packets at once, fixed steps of the embedded six-stage 4(5) Runge-Kutta pair of the reference (MOD_RK_PARAMS,
// Modules.f90:559-586; the state arrays zf, zdfdt, zVtij at :238-246).  Seven launches per step: one stage kernel per stage, which
// forms its operand y_s = a + dt sum_j A_sj k_j while it loads it and leaves k_s = -i H(t_n + c_s dt) y_s, then one kernel for the
// step, the error estimate and the snapshot.  bspatom_tdse_observe: on an observed step stage 0 runs as tdse_observe_kernel, which also
// measures a(t_n) (populations, E |a|^2, the coupling expectation value per channel), followed by tdse_obs_reduce_kernel: eight launches.
// bspatom_tdse_lawson: the integrating-factor form of the same tableau in the same launches (LAWSON in tdse_stage.h), after
// tdse_phase_kernel once.  The stage itself, tdse_stage_body, is in tdse_stage.h; the kernels of bspatom_tdse_static that run it with
// static blocks are in tdse_static.hip.
//
// Working layout: the amplitudes of channel c are a real matrix [count][NC], column 2q = Re, 2q + 1 = Im of scan q, NC = 2 nscan
// rounded up to 16 (zero columns); a, k_0 .. k_5 are [nch][count][NC] each.  A coupling block times these columns is a real
// product on v_mfma_f64_16x16x4_f64; the field, which differs per column, enters in the epilogue.
#include "common.h"
#include "mfma_tile.h"
#include "tdse_stage.h"
#include "tdse_launch.h"

namespace bsp {

// ---- the tableau (MOD_RK_PARAMS, Modules.f90:568-584) ----------------------------------------------------------------------
// a21 .. a65 (:568-572), c1 .. c6 (:577-578: 0, 2/9, 1/3, 3/4, 1, 5/6 -- the row sums; the field table is laid out on them),
// the 5th-order weights d1 .. d6 (:580-581) that advance the solution, the 4th-order b1 .. b5 (:574-575, b6 = 0) of the estimate
const double TDSE_A[6][5] = {{0.0, 0.0, 0.0, 0.0, 0.0},
                             {2.0 / 9.0, 0.0, 0.0, 0.0, 0.0},
                             {1.0 / 12.0, 1.0 / 4.0, 0.0, 0.0, 0.0},
                             {69.0 / 128.0, -243.0 / 128.0, 135.0 / 64.0, 0.0, 0.0},
                             {-17.0 / 12.0, 27.0 / 4.0, -27.0 / 5.0, 16.0 / 15.0, 0.0},
                             {65.0 / 432.0, -5.0 / 16.0, 13.0 / 16.0, 4.0 / 27.0, 5.0 / 144.0}};
const double TDSE_D[6] = {47.0 / 450.0, 0.0, 12.0 / 25.0, 32.0 / 225.0, 1.0 / 30.0, 6.0 / 25.0};
const double TDSE_B[6] = {1.0 / 9.0, 0.0, 9.0 / 20.0, 16.0 / 45.0, 1.0 / 12.0, 0.0};

template <int S, int TN>
__global__ __launch_bounds__(256) void tdse_stage_kernel(int count, int NC, int nscan, int tm, int tn, const int *__restrict__ cptr,
                                                        const int *__restrict__ ent, const double *__restrict__ E,
                                                        const double *__restrict__ D, const double *__restrict__ a,
                                                        double *__restrict__ K, size_t kstride, const double *__restrict__ fld,
                                                        StageCoef cf, double dt)
{
    tdse_stage_body<S, TN, false, false>(count, NC, nscan, tm, tn, cptr, ent, E, D, a, K, kstride, fld, cf, dt, nullptr, nullptr);
}

// the Lawson stage: phs = the phases of stage S (unused by stage 0); E is not read
template <int S, int TN>
__global__ __launch_bounds__(256) void tdse_lawson_stage_kernel(int count, int NC, int nscan, int tm, int tn, const int *__restrict__ cptr,
                                                               const int *__restrict__ ent, const double *__restrict__ D,
                                                               const double *__restrict__ a, double *__restrict__ K, size_t kstride,
                                                               const double *__restrict__ fld, StageCoef cf, double dt,
                                                               const double *__restrict__ phs)
{
    tdse_stage_body<S, TN, false, true>(count, NC, nscan, tm, tn, cptr, ent, nullptr, D, a, K, kstride, fld, cf, dt, nullptr, phs);
}

// stage 0 with the measuring epilogue: k_0 exactly as tdse_stage_kernel<0, TN> leaves it (fld == nullptr: no k_0, the measurement alone)
template <int TN>
__global__ __launch_bounds__(256) void tdse_observe_kernel(int count, int NC, int nscan, int tm, int tn, const int *__restrict__ cptr,
                                                          const int *__restrict__ ent, const double *__restrict__ E,
                                                          const double *__restrict__ D, const double *__restrict__ a,
                                                          double *__restrict__ K, const double *__restrict__ fld,
                                                          double *__restrict__ part)
{
    tdse_stage_body<0, TN, true, false>(count, NC, nscan, tm, tn, cptr, ent, E, D, a, K, 0, fld, StageCoef{}, 0.0, part, nullptr);
}

// the observing stage 0 of a Lawson step: the measurement of tdse_observe_kernel, k_0 as tdse_lawson_stage_kernel<0, TN> leaves it
template <int TN>
__global__ __launch_bounds__(256) void tdse_lawson_observe_kernel(int count, int NC, int nscan, int tm, int tn, const int *__restrict__ cptr,
                                                                 const int *__restrict__ ent, const double *__restrict__ E,
                                                                 const double *__restrict__ D, const double *__restrict__ a,
                                                                 double *__restrict__ K, const double *__restrict__ fld,
                                                                 double *__restrict__ part)
{
    tdse_stage_body<0, TN, true, true>(count, NC, nscan, tm, tn, cptr, ent, E, D, a, K, 0, fld, StageCoef{}, 0.0, part, nullptr);
}

// The phase table of a Lawson call, once per call: ph[((s - 1) rows + row) 2 + {0, 1}] = cos, sin of E[row] (c_s dt), s = 1 .. 5,
// both products in fp64 (cdt[s - 1] = c_s dt comes from the host: one rounding).  The entry of s = 4 (c_4 = 1) also serves the step.
struct PhaseCoef { double cdt[5]; };

__global__ __launch_bounds__(256) void tdse_phase_kernel(long long rows, const double *__restrict__ E, PhaseCoef pc, double *__restrict__ ph)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= rows) return;
    const double en = E[t];
#pragma unroll
    for (int s = 0; s < 5; ++s) {
        double sn, cs;
        sincos(en * pc.cdt[s], &sn, &cs);
        ph[((size_t)s * rows + t) * 2] = cs;
        ph[((size_t)s * rows + t) * 2 + 1] = sn;
    }
}

// One thread per (scan, channel): the row-tile partials in ascending tile order, written in the caller's layout row[(q nch + c) 4 + k]
__global__ __launch_bounds__(256) void tdse_obs_reduce_kernel(int nch, int tm, int ncq, int nscan, const double *__restrict__ part,
                                                             double *__restrict__ row)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)nscan * nch) return;
    const int q = (int)(t / nch), c = (int)(t - (long long)q * nch);
    const double *p0 = part + (((size_t)c * tm) * ncq + q) * 4;
    double s[4] = {p0[0], p0[1], p0[2], p0[3]};
    for (int im = 1; im < tm; ++im) {
        const double *pi = p0 + (size_t)im * ncq * 4;
#pragma unroll
        for (int k = 0; k < 4; ++k) s[k] += pi[k];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) row[(size_t)t * 4 + k] = s[k];
}

// ---- the step: tdse_step_body (tdse_stage.h) ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tdse_step_kernel(long long rows, int NC, int nscan, double *__restrict__ a,
                                                       const double *__restrict__ K, size_t kstride, StepCoef sc, double dt,
                                                       unsigned long long *__restrict__ err2, double *__restrict__ snap)
{
    tdse_step_body<false>(rows, NC, nscan, a, K, kstride, sc, dt, err2, snap, nullptr);
}

__global__ __launch_bounds__(256) void tdse_lawson_step_kernel(long long rows, int NC, int nscan, double *__restrict__ a,
                                                              const double *__restrict__ K, size_t kstride, StepCoef sc, double dt,
                                                              unsigned long long *__restrict__ err2, double *__restrict__ snap,
                                                              const double *__restrict__ ph4)
{
    tdse_step_body<true>(rows, NC, nscan, a, K, kstride, sc, dt, err2, snap, ph4);
}

// caller's layout a[((q nch + c) count + n) 2 + ri]  <->  working layout; pad columns are written as zeros
__global__ __launch_bounds__(256) void tdse_pack_kernel(long long rows, int NC, int nscan, const double *__restrict__ src, double *__restrict__ dst)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= rows * NC) return;
    const long long row = t / NC;
    const int col = (int)(t - row * NC), q = col >> 1;
    dst[t] = q < nscan ? src[((size_t)q * rows + row) * 2 + (col & 1)] : 0.0;
}

__global__ __launch_bounds__(256) void tdse_unpack_kernel(long long rows, int NC, int nscan, const double *__restrict__ src, double *__restrict__ dst)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= rows * 2 * nscan) return;
    const long long qr = t >> 1;
    const int ri = (int)(t & 1);
    const long long q = qr / rows, row = qr - q * rows;
    dst[t] = src[(size_t)row * NC + 2 * q + ri];
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------
int tdse_columns(int nscan) { return (2 * nscan + 15) / 16 * 16; }

template <int S>
static int launch_stage_s(const TdseDims &d, const TdseBufs &w, const double *fld, double dt, hipStream_t st)
{
    KScope ks_(KS_TDSE, st);
    if (w.nf > 1) return launch_tdse_fields_stage(S, d, w, fld, dt, st);         // several drive fields (tdse_fields.hip)
    if (w.W) return launch_tdse_static_stage(S, d, w, fld, dt, st);              // static blocks, either scheme (tdse_static.hip)
    const int TN = d.NC == 16 ? 1 : 2;
    const StageGrid g = stage_grid(d, TN);
    if (!g.ok) return BSP_ERR_UNSUPPORTED;
    if (w.ph) {
        auto kern = TN == 1 ? tdse_lawson_stage_kernel<S, 1> : tdse_lawson_stage_kernel<S, 2>;
        hipLaunchKernelGGL(kern, dim3(g.grid), dim3(256), 0, st, d.count, d.NC, d.nscan, g.tm, g.tn, w.cptr, w.ent, w.D, w.a, w.K, k_stride(d),
                           fld, stage_coef<S>(), dt, stage_phases(S, d, w));
    } else {
        auto kern = TN == 1 ? tdse_stage_kernel<S, 1> : tdse_stage_kernel<S, 2>;
        hipLaunchKernelGGL(kern, dim3(g.grid), dim3(256), 0, st, d.count, d.NC, d.nscan, g.tm, g.tn, w.cptr, w.ent, w.E, w.D, w.a, w.K,
                           k_stride(d), fld, stage_coef<S>(), dt);
    }
    BSP_HIP(hipGetLastError());
    return BSP_OK;
}

int launch_tdse_observe(const TdseDims &d, const TdseBufs &w, const double *fld, double *d_row, hipStream_t st)
{
    const int TN = d.NC == 16 ? 1 : 2;
    const StageGrid g = stage_grid(d, TN);
    {
        KScope ks_(KS_TDSE, st);
        if (!g.ok) return BSP_ERR_UNSUPPORTED;
        // a Lawson step's stage 0 leaves another k_0; a measurement alone (fld null) is the same kernel for both schemes
        const bool lawson = w.ph && fld;
        if (w.nf > 1) {
            const int rc = launch_tdse_fields_observe(d, w, fld, lawson, st);
            if (rc) return rc;
        } else if (w.W) {
            const int rc = launch_tdse_static_observe(d, w, fld, lawson, st);
            if (rc) return rc;
        } else {
            auto kern = TN == 1 ? (lawson ? tdse_lawson_observe_kernel<1> : tdse_observe_kernel<1>)
                                : (lawson ? tdse_lawson_observe_kernel<2> : tdse_observe_kernel<2>);
            hipLaunchKernelGGL(kern, dim3(g.grid), dim3(256), 0, st, d.count, d.NC, d.nscan, g.tm, g.tn, w.cptr, w.ent, w.E, w.D, w.a, w.K,
                               fld, w.part);
            BSP_HIP(hipGetLastError());
        }
    }
    if (w.nf > 1) return launch_tdse_fields_reduce(d, w, d_row, st);            // rows of 4 + 2 nf (bspatom_tdse_fields)
    if (w.ow == 6) return launch_tdse_static_reduce(d, w, d_row, st);           // rows of 6 (bspatom_tdse_static)
    const Blocks b = reduce_blocks(d);
    if (!b.ok) return BSP_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(tdse_obs_reduce_kernel, dim3(b.n), dim3(256), 0, st, d.nch, g.tm, d.NC / 2, d.nscan, w.part, d_row);
    BSP_HIP(hipGetLastError());
    return BSP_OK;
}

int launch_tdse_step(const TdseDims &d, const TdseBufs &w, const double *d_field, double dt, double *d_snap, double *d_obs, hipStream_t st)
{
    const size_t fs = (size_t)2 * d.nscan * w.nf;
    for (int S = 0; S < 6; ++S) {
        const int rc = S == 0 && d_obs ? launch_tdse_observe(d, w, d_field, d_obs, st)
                                       : dispatch_stage(S, [&](auto s) { return launch_stage_s<decltype(s)::value>(d, w, d_field + S * fs, dt, st); });
        if (rc) return rc;
    }
    const StepGrid g = step_grid(d);
    if (!g.ok) return BSP_ERR_UNSUPPORTED;
    if (w.ph)
        hipLaunchKernelGGL(tdse_lawson_step_kernel, g.grid, dim3(256), 0, st, g.rows, d.NC, d.nscan, w.a, w.K, k_stride(d), step_coef(), dt,
                           w.err2, d_snap, step_phases(d, w));
    else
        hipLaunchKernelGGL(tdse_step_kernel, g.grid, dim3(256), 0, st, g.rows, d.NC, d.nscan, w.a, w.K, k_stride(d), step_coef(), dt, w.err2,
                           d_snap);
    BSP_HIP(hipGetLastError());
    return BSP_OK;
}

int launch_tdse_phases(const TdseDims &d, const double *d_E, double dt, double *d_ph, hipStream_t st)
{
    const double c[5] = {2.0 / 9.0, 1.0 / 3.0, 3.0 / 4.0, 1.0, 5.0 / 6.0};      // c_1 .. c_5: the doubles nearest the fractions
    PhaseCoef pc;
    for (int s = 0; s < 5; ++s) pc.cdt[s] = c[s] * dt;
    const long long rows = (long long)d.nch * d.count;
    const Blocks b = blocks256(rows);
    if (!b.ok) return BSP_ERR_UNSUPPORTED;
    KScope ks_(KS_TDSE, st);
    hipLaunchKernelGGL(tdse_phase_kernel, dim3(b.n), dim3(256), 0, st, rows, d_E, pc, d_ph);
    BSP_HIP(hipGetLastError());
    return BSP_OK;
}

int launch_tdse_pack(const TdseDims &d, const double *d_user, double *d_work, hipStream_t st)
{
    const long long rows = (long long)d.nch * d.count;
    const Blocks b = blocks256(rows * d.NC);
    if (!b.ok) return BSP_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(tdse_pack_kernel, dim3(b.n), dim3(256), 0, st, rows, d.NC, d.nscan, d_user, d_work);
    BSP_HIP(hipGetLastError());
    return BSP_OK;
}

int launch_tdse_unpack(const TdseDims &d, const double *d_work, double *d_user, hipStream_t st)
{
    const long long rows = (long long)d.nch * d.count;
    const Blocks b = blocks256(rows * 2 * d.nscan);
    if (!b.ok) return BSP_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(tdse_unpack_kernel, dim3(b.n), dim3(256), 0, st, rows, d.NC, d.nscan, d_work, d_user);
    BSP_HIP(hipGetLastError());
    return BSP_OK;
}

}  // namespace bsp
