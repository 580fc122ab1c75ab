// tdse_fields.hip -- the kernels of bspatom_tdse_fields with more than one drive field: the stage of tdse_stage.h with NF = 2 or 3 pairs of
// accumulators (and its STAT flag: the static accumulator costs a call without static blocks nothing but registers), either scheme, the
// observing stage 0 with partials of 4 + 2 NF doubles, and the reduction to rows of that width.  A translation unit of its own: the code
// objects of tdse.hip and tdse_static.hip are what they were.  The launchers are called from tdse.hip's, the stage and the observing
// stage inside their timing scope (slot KS_TDSE).  A call with one field never comes here.
#include "common.h"
#include "mfma_tile.h"
#include "tdse_stage.h"
#include "tdse_launch.h"

namespace bsp {

// fld: this stage's field values [NF][nscan][2]; E is not read by a Lawson stage, phs not by a plain one, Wst only through a static entry
template <int S, int NF, bool LAWSON>
__global__ __launch_bounds__(256) void tdse_fields_stage_kernel(int count, int NC, int nscan, int tm, int tn, const int *__restrict__ cptr,
                                                               const int *__restrict__ ent, const double *__restrict__ E,
                                                               const double *__restrict__ D, const double *__restrict__ Wst,
                                                               const double *__restrict__ a, double *__restrict__ K, size_t kstride,
                                                               const double *__restrict__ fld, StageCoef cf, double dt,
                                                               const double *__restrict__ phs)
{
    tdse_stage_body<S, 1, false, LAWSON, true, NF>(count, NC, nscan, tm, tn, cptr, ent, E, D, a, K, kstride, fld, cf, dt, nullptr, phs, Wst);
}

// their observing stage 0: partials of 4 + 2 NF doubles
template <int NF, bool LAWSON>
__global__ __launch_bounds__(256) void tdse_fields_observe_kernel(int count, int NC, int nscan, int tm, int tn, const int *__restrict__ cptr,
                                                                 const int *__restrict__ ent, const double *__restrict__ E,
                                                                 const double *__restrict__ D, const double *__restrict__ Wst,
                                                                 const double *__restrict__ a, double *__restrict__ K,
                                                                 const double *__restrict__ fld, double *__restrict__ part)
{
    tdse_stage_body<0, 1, true, LAWSON, true, NF>(count, NC, nscan, tm, tn, cptr, ent, E, D, a, K, 0, fld, StageCoef{}, 0.0, part, nullptr, Wst);
}

// The rows of bspatom_tdse_fields, row[(q nch + c) RW + k]: the row-tile partials of RW doubles added in tdse_obs_reduce_kernel's order
template <int RW>
__global__ __launch_bounds__(256) void tdse_obs_reduce_fields_kernel(int nch, int tm, int ncq, int nscan, const double *__restrict__ part,
                                                                    double *__restrict__ row)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)nscan * nch) return;
    const int q = (int)(t / nch), c = (int)(t - (long long)q * nch);
    const double *p0 = part + (((size_t)c * tm) * ncq + q) * RW;
    double s[RW];
#pragma unroll
    for (int k = 0; k < RW; ++k) s[k] = p0[k];
    for (int im = 1; im < tm; ++im) {
        const double *pi = p0 + (size_t)im * ncq * RW;
#pragma unroll
        for (int k = 0; k < RW; ++k) s[k] += pi[k];
    }
#pragma unroll
    for (int k = 0; k < RW; ++k) row[(size_t)t * RW + k] = s[k];
}

// ---- launchers -----------------------------------------------------------------------------------------------------------------
// The narrow column tile (TN = 1, 8 scans per workgroup) for every nscan, as tdse_static.hip and for its reason
template <int S, int NF>
static int launch_fields_stage_sn(const TdseDims &d, const TdseBufs &w, const double *fld, double dt, hipStream_t st)
{
    const StageGrid g = stage_grid(d, 1);
    if (!g.ok) return BSP_ERR_UNSUPPORTED;
    auto kern = w.ph ? tdse_fields_stage_kernel<S, NF, true> : tdse_fields_stage_kernel<S, NF, false>;
    hipLaunchKernelGGL(kern, dim3(g.grid), dim3(256), 0, st, d.count, d.NC, d.nscan, g.tm, g.tn, w.cptr, w.ent, w.E, w.D, w.W, w.a, w.K,
                       k_stride(d), fld, stage_coef<S>(), dt, stage_phases(S, d, w));
    BSP_HIP(hipGetLastError());
    return BSP_OK;
}

int launch_tdse_fields_stage(int S, const TdseDims &d, const TdseBufs &w, const double *fld, double dt, hipStream_t st)
{
    return dispatch_stage(S, [&](auto s) {
        constexpr int S_ = decltype(s)::value;
        if (w.nf == 2) return launch_fields_stage_sn<S_, 2>(d, w, fld, dt, st);
        if (w.nf == 3) return launch_fields_stage_sn<S_, 3>(d, w, fld, dt, st);
        return (int)BSP_ERR_UNSUPPORTED;
    });
}

int launch_tdse_fields_observe(const TdseDims &d, const TdseBufs &w, const double *fld, bool lawson, hipStream_t st)
{
    const StageGrid g = stage_grid(d, 1);
    if (!g.ok || w.nf < 2 || w.nf > 3) return BSP_ERR_UNSUPPORTED;
    auto kern = w.nf == 2 ? (lawson ? tdse_fields_observe_kernel<2, true> : tdse_fields_observe_kernel<2, false>)
                          : (lawson ? tdse_fields_observe_kernel<3, true> : tdse_fields_observe_kernel<3, false>);
    hipLaunchKernelGGL(kern, dim3(g.grid), dim3(256), 0, st, d.count, d.NC, d.nscan, g.tm, g.tn, w.cptr, w.ent, w.E, w.D, w.W, w.a, w.K, fld,
                       w.part);
    BSP_HIP(hipGetLastError());
    return BSP_OK;
}

int launch_tdse_fields_reduce(const TdseDims &d, const TdseBufs &w, double *d_row, hipStream_t st)
{
    const Blocks b = reduce_blocks(d);
    if (!b.ok || w.nf < 2 || w.nf > 3) return BSP_ERR_UNSUPPORTED;
    auto kern = w.nf == 2 ? tdse_obs_reduce_fields_kernel<8> : tdse_obs_reduce_fields_kernel<10>;
    hipLaunchKernelGGL(kern, dim3(b.n), dim3(256), 0, st, d.nch, stage_grid(d, 1).tm, d.NC / 2, d.nscan, w.part, d_row);
    BSP_HIP(hipGetLastError());
    return BSP_OK;
}

}  // namespace bsp
