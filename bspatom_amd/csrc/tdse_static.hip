// tdse_static.hip -- the kernels of bspatom_tdse_static with static blocks: the stage of tdse_stage.h with its STAT flag, either scheme,
// the observing stage 0 with partials of 6 doubles, and the reduction to rows of 6.  A translation unit of its own: the code object of
// tdse.hip, the kernels of the six other TDSE entry points, is what it was.  The launchers are called from tdse.hip's, the stage and the
// observing stage inside their timing scope (slot KS_TDSE).
#include "common.h"
#include "mfma_tile.h"
#include "tdse_stage.h"
#include "tdse_launch.h"

namespace bsp {

// the stages of bspatom_tdse_static with static blocks (Wst): either scheme; E is not read by a Lawson stage, phs not by a plain one
template <int S, int TN, bool LAWSON>
__global__ __launch_bounds__(256) void tdse_static_stage_kernel(int count, int NC, int nscan, int tm, int tn, const int *__restrict__ cptr,
                                                               const int *__restrict__ ent, const double *__restrict__ E,
                                                               const double *__restrict__ D, const double *__restrict__ Wst,
                                                               const double *__restrict__ a, double *__restrict__ K, size_t kstride,
                                                               const double *__restrict__ fld, StageCoef cf, double dt,
                                                               const double *__restrict__ phs)
{
    tdse_stage_body<S, TN, false, LAWSON, true>(count, NC, nscan, tm, tn, cptr, ent, E, D, a, K, kstride, fld, cf, dt, nullptr, phs, Wst);
}

// their observing stage 0: partials of 6 doubles, the first four with the bits tdse_observe_kernel gives them
template <int TN, bool LAWSON>
__global__ __launch_bounds__(256) void tdse_static_observe_kernel(int count, int NC, int nscan, int tm, int tn, const int *__restrict__ cptr,
                                                                 const int *__restrict__ ent, const double *__restrict__ E,
                                                                 const double *__restrict__ D, const double *__restrict__ Wst,
                                                                 const double *__restrict__ a, double *__restrict__ K,
                                                                 const double *__restrict__ fld, double *__restrict__ part)
{
    tdse_stage_body<0, TN, true, LAWSON, true>(count, NC, nscan, tm, tn, cptr, ent, E, D, a, K, 0, fld, StageCoef{}, 0.0, part, nullptr, Wst);
}

// The rows of bspatom_tdse_static, row[(q nch + c) 6 + k]: partials of pw = 6 doubles (static blocks) or of 4 (none: tdse_observe_kernel's,
// k = 4, 5 are written as zeros), added in tdse_obs_reduce_kernel's order
__global__ __launch_bounds__(256) void tdse_obs_reduce6_kernel(int nch, int tm, int ncq, int nscan, int pw, const double *__restrict__ part,
                                                              double *__restrict__ row)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)nscan * nch) return;
    const int q = (int)(t / nch), c = (int)(t - (long long)q * nch);
    const double *p0 = part + (((size_t)c * tm) * ncq + q) * pw;
    double s[6] = {p0[0], p0[1], p0[2], p0[3], pw == 6 ? p0[4] : 0.0, pw == 6 ? p0[5] : 0.0};
    for (int im = 1; im < tm; ++im) {
        const double *pi = p0 + (size_t)im * ncq * pw;
#pragma unroll
        for (int k = 0; k < 4; ++k) s[k] += pi[k];
        if (pw == 6) {
            s[4] += pi[4];
            s[5] += pi[5];
        }
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) row[(size_t)t * 6 + k] = s[k];
}

// ---- launchers -----------------------------------------------------------------------------------------------------------------
// The static kernels run on the narrow column tile (TN = 1, 16 columns = 8 scans per workgroup) for every nscan: the wide tile of
// tdse.hip (TN = 2 above 8 scans) would hold 180 .. 208 registers as a static Lawson stage, two waves per SIMD, and measured 0.615
// against 0.443 ms per step at nscan = 16.
template <int S>
static int launch_static_stage_s(const TdseDims &d, const TdseBufs &w, const double *fld, double dt, hipStream_t st)
{
    const StageGrid g = stage_grid(d, 1);
    if (!g.ok) return BSP_ERR_UNSUPPORTED;
    auto kern = w.ph ? tdse_static_stage_kernel<S, 1, true> : tdse_static_stage_kernel<S, 1, false>;
    hipLaunchKernelGGL(kern, dim3(g.grid), dim3(256), 0, st, d.count, d.NC, d.nscan, g.tm, g.tn, w.cptr, w.ent, w.E, w.D, w.W, w.a, w.K,
                       k_stride(d), fld, stage_coef<S>(), dt, stage_phases(S, d, w));
    BSP_HIP(hipGetLastError());
    return BSP_OK;
}

int launch_tdse_static_stage(int S, const TdseDims &d, const TdseBufs &w, const double *fld, double dt, hipStream_t st)
{
    return dispatch_stage(S, [&](auto s) { return launch_static_stage_s<decltype(s)::value>(d, w, fld, dt, st); });
}

int launch_tdse_static_observe(const TdseDims &d, const TdseBufs &w, const double *fld, bool lawson, hipStream_t st)
{
    const StageGrid g = stage_grid(d, 1);
    if (!g.ok) return BSP_ERR_UNSUPPORTED;
    auto kern = lawson ? tdse_static_observe_kernel<1, true> : tdse_static_observe_kernel<1, false>;
    hipLaunchKernelGGL(kern, dim3(g.grid), dim3(256), 0, st, d.count, d.NC, d.nscan, g.tm, g.tn, w.cptr, w.ent, w.E, w.D, w.W, w.a, w.K, fld,
                       w.part);
    BSP_HIP(hipGetLastError());
    return BSP_OK;
}

int launch_tdse_static_reduce(const TdseDims &d, const TdseBufs &w, double *d_row, hipStream_t st)
{
    const Blocks b = reduce_blocks(d);
    if (!b.ok) return BSP_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(tdse_obs_reduce6_kernel, dim3(b.n), dim3(256), 0, st, d.nch, stage_grid(d, 1).tm, d.NC / 2, d.nscan, w.W ? 6 : 4, w.part,
                       d_row);
    BSP_HIP(hipGetLastError());
    return BSP_OK;
}

}  // namespace bsp
