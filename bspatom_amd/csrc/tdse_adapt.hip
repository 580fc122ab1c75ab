// tdse_adapt.hip -- the kernels of bspatom_tdse_adaptive: the stage and the step of tdse_stage.h with their ADAPT flag (the static stage,
// one field, either scheme, both column tiles), the reduction to the row the control block names, tdse_adapt_control_kernel, which
// judges an attempt, advances the dyadic step grid and interpolates the field of the next attempt, and tdse_adapt_commit_kernel, which
// takes an accepted candidate into a and writes its snapshot.  A translation unit of its own: the code objects of tdse.hip,
// tdse_static.hip and tdse_fields.hip are what they were.  No kernel waits for another: every launch reads the control block as the
// launch before it in the stream left it, and launches enqueued behind the end of the run return at their first instruction.
// All launches are timed in slot KS_TDSE.
#include "common.h"
#include "mfma_tile.h"
#include "tdse_stage.h"
#include "tdse_launch.h"

namespace bsp {

template <int S, int TN, bool OBS, bool LAWSON>
__global__ __launch_bounds__(256) void tdse_adapt_stage_kernel(int count, int NC, int nscan, int tm, int tn, const int *__restrict__ cptr,
                                                              const int *__restrict__ ent, const double *__restrict__ E,
                                                              const double *__restrict__ D, const double *__restrict__ Wst,
                                                              const double *__restrict__ a, double *__restrict__ K, size_t kstride,
                                                              StageCoef cf, double dt, double *__restrict__ part,
                                                              const double *__restrict__ phs, size_t phlev,
                                                              const TdseAdaptCtl *__restrict__ ctl)
{
    tdse_stage_body<S, TN, OBS, LAWSON, true, 1, true>(count, NC, nscan, tm, tn, cptr, ent, E, D, a, K, kstride, nullptr, cf, dt, part, phs,
                                                       Wst, ctl, phlev);
}

template <bool LAWSON>
__global__ __launch_bounds__(256) void tdse_adapt_step_kernel(long long rows, int NC, int nscan, double *__restrict__ a,
                                                             const double *__restrict__ K, size_t kstride, StepCoef sc, double dt,
                                                             unsigned long long *__restrict__ err2, const double *__restrict__ ph4,
                                                             size_t phlev, const TdseAdaptCtl *__restrict__ ctl,
                                                             double *__restrict__ cand)
{
    tdse_step_body<LAWSON, true>(rows, NC, nscan, a, K, kstride, sc, dt, err2, nullptr, ph4, ctl, phlev, cand);
}

// tdse_obs_reduce6_kernel on partials of 6, into row ctl->row of the group's rows (odbl doubles each); nothing without a row
__global__ __launch_bounds__(256) void tdse_adapt_reduce_kernel(int nch, int tm, int ncq, int nscan, const double *__restrict__ part,
                                                               double *__restrict__ rows, size_t odbl,
                                                               const TdseAdaptCtl *__restrict__ ctl)
{
    if (ctl->done || ctl->row < 0) return;
    double *row = rows + (size_t)ctl->row * odbl;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)nscan * nch) return;
    const int q = (int)(t / nch), c = (int)(t - (long long)q * nch);
    const double *p0 = part + (((size_t)c * tm) * ncq + q) * 6;
    double s[6] = {p0[0], p0[1], p0[2], p0[3], p0[4], p0[5]};
    for (int im = 1; im < tm; ++im) {
        const double *pi = p0 + (size_t)im * ncq * 6;
#pragma unroll
        for (int k = 0; k < 6; ++k) s[k] += pi[k];
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) row[(size_t)t * 6 + k] = s[k];
}

// attempt t was accepted: a = the candidate, and its snapshot in the caller's layout where the control block names one
__global__ __launch_bounds__(256) void tdse_adapt_commit_kernel(long long rows, int NC, int nscan, const double *__restrict__ cand,
                                                               double *__restrict__ a, double *__restrict__ snaps, size_t adbl,
                                                               const TdseAdaptCtl *__restrict__ ctl, long long t)
{
    if (ctl->acc_t != t) return;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * NC) return;
    const double v = cand[i];
    a[i] = v;
    const int sn = ctl->snap;
    if (sn < 0) return;
    const long long row = i / NC;
    const int col = (int)(i - row * NC), q = col >> 1;
    if (q < nscan) snaps[(size_t)sn * adbl + ((size_t)q * rows + row) * 2 + (col & 1)] = v;
}

// ---- the controller ------------------------------------------------------------------------------------------------------------
// The field of stage s of the attempt (n, m, j), component ri of scan q (include/bspatom.h): x_s = ldexp((double)j + c_s, -m), the
// interval i_loc = min((int)floor(x_s nsub), nsub - 1), u = x_s nsub - i_loc, then the cubic Hermite interpolant of the node table.
// IEEE multiplies and adds in the order written, NOTHING contracted from the product x_s nsub on (the pragma covers the whole body:
// a fused u = fma(x_s, nsub, -i_loc) would differ from the documented one for every nsub that is no power of two), Re and Im
// independently.  Nodes: fn[((i 2 + k) nscan + q) 2 + ri], i counted from the group's node0.
__device__ __forceinline__ double field_at(const double *__restrict__ fn, int nscan, int q, int ri, int n, int m, int j, double cs, int nsub,
                                           int node0, double dt)
{
#pragma clang fp contract(off)
    const double dsub = (double)nsub;
    const double hf = dt / dsub;
    const double xs = ldexp((double)j + cs, -m) * dsub;
    int il = (int)floor(xs);
    il = il < nsub - 1 ? il : nsub - 1;
    const double u = xs - (double)il;
    const double omu = 1.0 - u, omu2 = omu * omu, u2 = u * u;
    const double h00 = (1.0 + 2.0 * u) * omu2, h10 = u * omu2, h01 = u2 * (3.0 - 2.0 * u), h11 = u2 * (u - 1.0);
    const long long node = (long long)n * nsub + il - node0;
    const double *n0 = fn + ((size_t)node * 2 * nscan + q) * 2 + ri, *n1 = n0 + (size_t)4 * nscan;
    const double f0 = n0[0], d0 = n0[(size_t)2 * nscan], f1 = n1[0], d1 = n1[(size_t)2 * nscan];
    return ((h00 * f0 + (h10 * hf) * d0) + h01 * f1) + (h11 * hf) * d1;
}

// One workgroup per attempt, behind its step kernel: (1) e_q = |h| sqrt(err2[q]), e = max_q; (2) accepted if e <= tol, forced if not and
// m = max_level, else rejected; (3) the next (n, m, j) by the rule of the header; (4) the log entry; (5) the field at the six stage times
// of the coming attempt for every scan; (6) done at n = nend.  init: parts (5) and the row of the coming attempt alone.
__global__ __launch_bounds__(256) void tdse_adapt_control_kernel(TdseAdaptCtl *__restrict__ ctl, int nscan, TdseAdaptArgs g,
                                                                unsigned long long *__restrict__ err2, int init)
{
    __shared__ double smax[256];
    const int tid = threadIdx.x;
    if (ctl->done) return;
    double *fld = (double *)((char *)ctl + TDSE_CTL_HDR), *errmax = fld + (size_t)12 * nscan;
    int n = ctl->n, m = ctl->m, j = ctl->j;
    const int nend = ctl->nend, snap0 = ctl->snap0, row0 = ctl->row0, node0 = ctl->node0;
    long long st[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) st[k] = ctl->stats[k];
    int flag = -1, snap = -1;
    long long acc_t = ctl->acc_t;
    if (!init) {
        const double h = fabs(ldexp(g.dt, -m));
        const long long t = st[5];
        const bool logging = t < (long long)g.log_cap;
        double mx = 0.0;
        for (int q = tid; q < nscan; q += 256) {
            const double eq = h * sqrt(__longlong_as_double((long long)err2[q]));
            mx = eq > mx ? eq : mx;
            if (logging) g.log_e[(size_t)t * nscan + q] = eq;
        }
        if (logging)
            for (int i = tid; i < 12 * nscan; i += 256) g.log_f[(size_t)t * 12 * nscan + i] = fld[i];
        smax[tid] = mx;
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if (tid < s) smax[tid] = smax[tid + s] > smax[tid] ? smax[tid + s] : smax[tid];
            __syncthreads();
        }
        const double e = smax[0];
        flag = e <= g.tol ? 1 : (m == g.max_level ? 2 : 0);
        for (int q = tid; q < nscan; q += 256) {
            if (flag) {
                const double eq = h * sqrt(__longlong_as_double((long long)err2[q]));
                errmax[q] = eq > errmax[q] ? eq : errmax[q];
            }
            err2[q] = 0ull;
        }
        if (logging && tid == 0) {
            int *li = g.log_i + (size_t)t * 4;
            li[0] = n; li[1] = m; li[2] = j; li[3] = flag;
        }
        st[5] = t + 1;
        st[3] = m > st[3] ? m : st[3];
        if (flag == 0) {
            st[1] += 1;
            m += 1;
            j *= 2;
        } else {
            st[0] += 1;
            if (flag == 2) st[2] += 1;
            acc_t = t;
            j += 1;
            if (e <= g.tol * 0.015625 && m > 0 && (j & 1) == 0) { m -= 1; j >>= 1; }
            if (j == (1 << m)) {
                n += 1;
                j = 0;
                if (g.snap_every > 0 && n % g.snap_every == 0) snap = n / g.snap_every - 1 - snap0;
            }
        }
    }
    const int done = n >= nend;
    __syncthreads();                              // every thread has read the header (the init path has no other barrier)
    if (tid == 0) {
        ctl->n = n; ctl->m = m; ctl->j = j;
        ctl->flag = flag;
        ctl->done = done;
        ctl->snap = snap;
        ctl->row = (!done && g.obs_every > 0 && j == 0 && n % g.obs_every == 0) ? n / g.obs_every - row0 : -1;
        ctl->acc_t = acc_t;
        st[4] = m;
#pragma unroll
        for (int k = 0; k < 6; ++k) ctl->stats[k] = st[k];
    }
    if (done) return;
    const double cs[6] = {0.0, 2.0 / 9.0, 1.0 / 3.0, 3.0 / 4.0, 1.0, 5.0 / 6.0};
    for (int i = tid; i < 12 * nscan; i += 256) {
        const int ri = i & 1, q = (i >> 1) % nscan, s = (i >> 1) / nscan;
        fld[i] = field_at(g.fn, nscan, q, ri, n, m, j, cs[s], g.nsub, node0, g.dt);
    }
}

// ---- launchers -----------------------------------------------------------------------------------------------------------------
// The column tile is the one bspatom_tdse_static takes on the same arguments: 16 columns with static blocks (tdse_static.hip), and
// without them 16 up to 8 scans, 32 above (tdse.hip).  The sums of an element do not depend on it.
template <int S, bool OBS>
static int launch_adapt_stage_s(const TdseDims &d, const TdseBufs &w, const TdseAdaptCtl *ctl, double dt, size_t phlev, hipStream_t st)
{
    const int TN = (w.W || d.NC == 16) ? 1 : 2;
    const StageGrid g = stage_grid(d, TN);
    if (!g.ok) return BSP_ERR_UNSUPPORTED;
    auto kern = w.ph ? (TN == 1 ? tdse_adapt_stage_kernel<S, 1, OBS, true> : tdse_adapt_stage_kernel<S, 2, OBS, true>)
                     : (TN == 1 ? tdse_adapt_stage_kernel<S, 1, OBS, false> : tdse_adapt_stage_kernel<S, 2, OBS, false>);
    KScope ks_(KS_TDSE, st);
    hipLaunchKernelGGL(kern, dim3(g.grid), dim3(256), 0, st, d.count, d.NC, d.nscan, g.tm, g.tn, w.cptr, w.ent, w.E, w.D, w.W, w.a, w.K,
                       OBS ? (size_t)0 : k_stride(d), stage_coef<S>(), dt, OBS ? w.part : nullptr, stage_phases(S, d, w), phlev, ctl);
    BSP_HIP(hipGetLastError());
    return BSP_OK;
}

static int launch_adapt_control(const TdseDims &d, const TdseBufs &w, TdseAdaptCtl *ctl, const TdseAdaptArgs &g, int init, hipStream_t st)
{
    KScope ks_(KS_TDSE, st);
    hipLaunchKernelGGL(tdse_adapt_control_kernel, dim3(1), dim3(256), 0, st, ctl, d.nscan, g, w.err2, init);
    BSP_HIP(hipGetLastError());
    return BSP_OK;
}

int launch_tdse_adapt_init(const TdseDims &d, const TdseBufs &w, TdseAdaptCtl *ctl, const TdseAdaptArgs &g, hipStream_t st)
{
    return launch_adapt_control(d, w, ctl, g, 1, st);
}

int launch_tdse_adapt_attempt(const TdseDims &d, const TdseBufs &w, TdseAdaptCtl *ctl, const TdseAdaptArgs &g, long long t, double *cand,
                              size_t phlev, double *d_snap, double *d_obs, hipStream_t st)
{
    const size_t odbl = (size_t)6 * d.nscan * d.nch;
    int rc;
    if ((rc = d_obs ? launch_adapt_stage_s<0, true>(d, w, ctl, g.dt, phlev, st) : launch_adapt_stage_s<0, false>(d, w, ctl, g.dt, phlev, st)))
        return rc;
    if (d_obs) {
        const Blocks b = reduce_blocks(d);
        if (!b.ok) return BSP_ERR_UNSUPPORTED;
        KScope ks_(KS_TDSE, st);
        hipLaunchKernelGGL(tdse_adapt_reduce_kernel, dim3(b.n), dim3(256), 0, st, d.nch, stage_grid(d, 1).tm, d.NC / 2, d.nscan, w.part, d_obs,
                           odbl, ctl);
        BSP_HIP(hipGetLastError());
    }
    for (int S = 1; S < 6; ++S)
        if ((rc = dispatch_stage(S, [&](auto s) { return launch_adapt_stage_s<decltype(s)::value, false>(d, w, ctl, g.dt, phlev, st); })))
            return rc;
    const StepGrid sg = step_grid(d);
    const Blocks cb = blocks256(sg.rows * d.NC);
    if (!sg.ok || !cb.ok) return BSP_ERR_UNSUPPORTED;
    const size_t adbl = (size_t)sg.rows * d.nscan * 2;
    {
        KScope ks_(KS_TDSE, st);
        auto kern = w.ph ? tdse_adapt_step_kernel<true> : tdse_adapt_step_kernel<false>;
        hipLaunchKernelGGL(kern, sg.grid, dim3(256), 0, st, sg.rows, d.NC, d.nscan, w.a, w.K, k_stride(d), step_coef(), g.dt, w.err2,
                           step_phases(d, w), phlev, ctl, cand);
        BSP_HIP(hipGetLastError());
    }
    if ((rc = launch_adapt_control(d, w, ctl, g, 0, st))) return rc;
    KScope ks_(KS_TDSE, st);
    hipLaunchKernelGGL(tdse_adapt_commit_kernel, dim3(cb.n), dim3(256), 0, st, sg.rows, d.NC, d.nscan, cand, w.a, d_snap, adbl, ctl, t);
    BSP_HIP(hipGetLastError());
    return BSP_OK;
}

}  // namespace bsp
