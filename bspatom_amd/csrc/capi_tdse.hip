// capi_tdse.hip -- bspatom_tdse_propagate / _dev, bspatom_tdse_observe / _dev, bspatom_tdse_lawson / _dev, bspatom_tdse_static / _dev,
// bspatom_tdse_fields / _dev and bspatom_tdse_adaptive / _dev (include/bspatom.h): the argument checks, the per-channel entry lists, the working buffers and the step loop
// of tdse.hip.  One code path: propagate is observe without rows, the Lawson scheme is a flag that adds the phase table, the static call
// is either with static entries behind the driven ones and rows of 6, and the fields call is the static call whose driven entries name
// their field (one field: the static call itself).  The problem handle gives the device and the stream; nothing of a solve is read.
#include <cmath>
#include "capi_internal.h"

using namespace bsp;

namespace {
constexpr size_t TDSE_STAGE_BYTES = (size_t)256 << 20;
size_t tdse_stage_bytes() { return opts().tdse_stage_mb > 0 ? (size_t)opts().tdse_stage_mb << 20 : TDSE_STAGE_BYTES; }

bool args_ok(const bspatom_problem *p, int nch, int count, const double *E, int npairs, const int32_t *ci, const int32_t *cf,
             const double *D, int nscan, int nsteps, double dt, const double *field, const double *a, int snap_every, const double *snap)
{
    if (!p || !E || !a || nch < 1 || count < 1 || nscan < 1 || nsteps < 0 || npairs < 0 || snap_every < 0) return false;
    if (nsteps > 0 && !field) return false;
    if (npairs > 0 && (!ci || !cf || !D)) return false;
    if (snap && snap_every == 0) return false;
    if (!std::isfinite(dt)) return false;
    for (int q = 0; q < npairs; ++q)
        if (ci[q] < 0 || ci[q] >= nch || cf[q] < 0 || cf[q] >= nch || ci[q] == cf[q]) return false;
    return true;
}

// the static blocks of bspatom_tdse_static (host lists; W on the device once run_dev has it); null where a call has none by design
// nf, fidx: the drive fields of bspatom_tdse_fields and the field of every pair (null: all 0)
struct Static { int n; const int32_t *si, *sf, *kind; const double *W; int nf = 1; const int32_t *fidx = nullptr; };

// BSP_OK, or what bspatom_tdse_fields returns for its two own arguments
int fields_args_rc(int nfield, const int32_t *fidx, int npairs)
{
    if (nfield < 1) return BSP_ERR_ARG;
    if (nfield > BSPATOM_TDSE_MAX_FIELDS) return BSP_ERR_UNSUPPORTED;
    if (!fidx) return nfield > 1 && npairs > 0 ? BSP_ERR_ARG : BSP_OK;
    for (int q = 0; q < npairs; ++q)
        if (fidx[q] < 0 || fidx[q] >= nfield) return BSP_ERR_ARG;
    return BSP_OK;
}

bool static_args_ok(int nch, int scheme, int nstat, const int32_t *si, const int32_t *sf, const int32_t *skind, const double *W)
{
    if (scheme < 0 || scheme > 1 || nstat < 0) return false;
    if (nstat > 0 && (!si || !sf || !skind || !W)) return false;
    for (int j = 0; j < nstat; ++j)
        if (si[j] < 0 || si[j] >= nch || sf[j] < 0 || sf[j] >= nch || skind[j] < 0 || skind[j] > 1) return false;
    return true;
}

// everything of a call that lives on the device besides the caller's arrays
struct Plan {
    TdseDims d;
    DevArray<int> cptr, ent;
    DevArray<double> aw, K, part, ph;
    DevArray<unsigned long long> err2;
    size_t rows = 0, odbl = 0;                 // odbl: doubles of one row of observables, [nscan][nch][ow]
    bool observing = false;
    int ow = 4, nstat = 0, nf = 1;             // ow = 6: a bspatom_tdse_static call, 4 + 2 nf with nf > 1 fields; nstat: its static blocks
    // stc: null (the rows of 4 of the other calls), or the static blocks of a bspatom_tdse_static call (rows of 6, stc->n may be 0)
    // part6: partials of 6 doubles whatever the lists hold (bspatom_tdse_adaptive always runs the static stage)
    int prepare(bspatom_problem *p, int nch, int count, int nscan, int npairs, const int32_t *ci, const int32_t *cf, bool observing_,
                const Static *stc = nullptr, bool part6 = false)
    {
        d = {nch, count, nscan, tdse_columns(nscan)};
        rows = (size_t)nch * count;
        nf = stc ? stc->nf : 1;
        ow = stc ? (nf > 1 ? 4 + 2 * nf : 6) : 4;
        nstat = stc ? stc->n : 0;
        const int32_t *fidx = nf > 1 ? stc->fidx : nullptr;
        odbl = (size_t)ow * nscan * nch;
        observing = observing_;
        // channel c's entries in ascending p: (p, cf[p], 1) where ci[p] = c, (p, ci[p], 0) where cf[p] = c; behind them its static
        // entries in ascending j: (j, si[j], 2 + skind[j]) where sf[j] = c.  Several fields: a driven entry's third word gains 4 fidx[p]
        std::vector<int> cp(nch + 1, 0), en((size_t)6 * npairs + (size_t)3 * nstat + 3, 0);
        for (int q = 0; q < npairs; ++q) { ++cp[ci[q] + 1]; ++cp[cf[q] + 1]; }
        for (int j = 0; j < nstat; ++j) ++cp[stc->sf[j] + 1];
        for (int c = 0; c < nch; ++c) cp[c + 1] += cp[c];
        std::vector<int> at(cp.begin(), cp.end() - 1);
        for (int q = 0; q < npairs; ++q) {
            int *e = &en[(size_t)3 * at[ci[q]]++];
            const int g4 = fidx ? 4 * fidx[q] : 0;
            e[0] = q; e[1] = cf[q]; e[2] = 1 + g4;
            e = &en[(size_t)3 * at[cf[q]]++];
            e[0] = q; e[1] = ci[q]; e[2] = g4;
        }
        for (int j = 0; j < nstat; ++j) {
            int *e = &en[(size_t)3 * at[stc->sf[j]]++];
            e[0] = j; e[1] = stc->si[j]; e[2] = 2 + stc->kind[j];
        }
        int rc;
        if ((rc = cptr.put(cp.data(), cp.size())) || (rc = ent.put(en.data(), en.size())) || (rc = aw.alloc(rows * d.NC)) ||
            (rc = K.alloc(6 * rows * d.NC)) || (rc = err2.alloc(nscan)))
            return rc;
        // the observing kernel's partials: one of 4 doubles (6 with static blocks, 4 + 2 nf with several fields) per (channel, row tile
        // of 64 states, scan slot)
        if (observing && (rc = part.alloc((size_t)nch * ((count + 63) / 64) * (d.NC / 2) * (nf > 1 ? ow : (nstat > 0 || part6) ? 6 : 4)))) return rc;
        return HIP_RC(hipMemsetAsync(err2.p, 0, (size_t)nscan * sizeof(unsigned long long), p->st));
    }
    // the Lawson scheme: the phase table from the energies on the device, before bufs()
    int phases(bspatom_problem *p, const double *d_E, double dt)
    {
        const int rc = ph.alloc((size_t)10 * rows);
        return rc ? rc : launch_tdse_phases(d, d_E, dt, ph.p, p->st);
    }
    // d_W: the static blocks on the device (null without any: the kernels of the other calls run, whatever ow is)
    TdseBufs bufs(const double *d_E, const double *d_D, const double *d_W = nullptr) const
    {
        return {cptr.p, ent.p, d_E, d_D, aw.p, K.p, err2.p, observing ? part.p : nullptr, ph.p, nstat > 0 ? d_W : nullptr, ow, nf};
    }
    // steps n0 .. n1-1; d_field: the table from step n0 on; d_snap (or null): where snapshot number s0 (from 0) goes, the later ones behind it;
    // d_obs (or null): where row j0 goes (row j = the amplitudes before step j obs_every), the later ones behind it
    int run(bspatom_problem *p, const TdseBufs &w, int n0, int n1, double dt, const double *d_field, int snap_every, double *d_snap, int s0,
            int obs_every, double *d_obs, int j0)
    {
        for (int n = n0; n < n1; ++n) {
            double *sn = nullptr, *ob = nullptr;
            if (d_snap && (n + 1) % snap_every == 0) sn = d_snap + ((size_t)((n + 1) / snap_every - 1 - s0)) * rows * d.nscan * 2;
            if (d_obs && n % obs_every == 0) ob = d_obs + (size_t)(n / obs_every - j0) * odbl;
            const int rc = launch_tdse_step(d, w, d_field + (size_t)(n - n0) * 12 * d.nscan * nf, dt, sn, ob, p->st);
            if (rc) return rc;
        }
        return BSP_OK;
    }
    // after the stream has drained: err[q] = |dt| sqrt(max |sum_s (d_s - b_s) k_s|^2)
    int errors(double dt, double *err) const
    {
        if (!err) return BSP_OK;
        std::vector<unsigned long long> e2(d.nscan);
        const int rc = err2.get(e2.data(), e2.size());
        if (rc) return rc;
        for (int q = 0; q < d.nscan; ++q) {
            double m2;
            memcpy(&m2, &e2[q], sizeof m2);
            err[q] = std::fabs(dt) * std::sqrt(m2);
        }
        return BSP_OK;
    }
};

// obs_every = 0: no observables (obs null).  Otherwise rows for the steps 0, obs_every, .. < nsteps, then the row of the final amplitudes.
int run_dev(bspatom_problem *p, int nch, int count, const double *E_dev, int npairs, const int32_t *ci, const int32_t *cf,
            const double *D_dev, int nscan, int nsteps, double dt, const double *field_dev, double *a_dev, int snap_every,
            double *snap_dev, double *err, int obs_every, double *obs_dev, bool lawson, const Static *stc = nullptr)
{
    const bool observing = obs_every > 0;
    if (nsteps == 0 && !observing) {
        if (err) for (int q = 0; q < nscan; ++q) err[q] = 0.0;
        return BSP_OK;
    }
    BSP_HIP(hipSetDevice(p->device));
    Plan pl;
    int rc = pl.prepare(p, nch, count, nscan, npairs, ci, cf, observing, stc);
    if (!rc) rc = launch_tdse_pack(pl.d, a_dev, pl.aw.p, p->st);
    if (!rc && lawson && nsteps > 0) rc = pl.phases(p, E_dev, dt);
    const TdseBufs w = pl.bufs(E_dev, D_dev, stc ? stc->W : nullptr);
    if (!rc) rc = pl.run(p, w, 0, nsteps, dt, field_dev, snap_every, snap_dev, 0, obs_every, obs_dev, 0);
    if (!rc && observing) {
        const size_t last = nsteps > 0 ? (size_t)(nsteps - 1) / obs_every + 1 : 0;
        rc = launch_tdse_observe(pl.d, w, nullptr, obs_dev + last * pl.odbl, p->st);
    }
    if (!rc && nsteps > 0) rc = launch_tdse_unpack(pl.d, pl.aw.p, a_dev, p->st);
    if ((rc = drain(p, rc))) return rc;
    return pl.errors(dt, err);
}

int run_host(bspatom_problem *p, int nch, int count, const double *E, int npairs, const int32_t *ci, const int32_t *cf, const double *D,
             int nscan, int nsteps, double dt, const double *field, double *a, int snap_every, double *snap, double *err, int obs_every,
             double *obs, bool lawson, const Static *stc = nullptr)
{
    const bool observing = obs_every > 0;
    if (nsteps == 0 && !observing) {
        if (err) for (int q = 0; q < nscan; ++q) err[q] = 0.0;
        return BSP_OK;
    }
    BSP_HIP(hipSetDevice(p->device));
    const int nf = stc ? stc->nf : 1;
    const size_t rows = (size_t)nch * count, adbl = rows * nscan * 2, fdbl = (size_t)12 * nscan * nf;        // doubles of a snapshot, of a step's field
    const size_t odbl = (size_t)(stc ? (nf > 1 ? 4 + 2 * nf : 6) : 4) * nscan * nch;                         // of a row of observables
    // steps per group: the field of g steps, the (at most g / snap_every + 1) snapshots and the (at most (g - 1) / obs_every + 1)
    // observed steps among them within the bound, one step at least
    const bool snapping = snap && snap_every > 0;
    const size_t bound = tdse_stage_bytes() / sizeof(double);
    auto snaps_of = [&](size_t g) { return snapping ? g / snap_every + 1 : (size_t)0; };
    auto obs_of = [&](size_t g) { return observing && g > 0 ? (g - 1) / obs_every + 1 : (size_t)0; };
    auto need = [&](size_t g) { return g * fdbl + snaps_of(g) * adbl + obs_of(g) * odbl; };
    const size_t per_step = fdbl + adbl + (observing ? odbl : 0);
    size_t g = bound / fdbl;
    if (g > (size_t)nsteps) g = nsteps;
    while (g > 1 && need(g) > bound) {
        const size_t over = need(g) - bound;
        const size_t dec = over / per_step > 1 ? over / per_step : 1;
        g = g > dec ? g - dec : 1;
    }
    if (g < 1) g = 1;
    Plan pl;
    DevArray<double> dE, dD, dW, da, dfield, dsnap, dobs;
    int rc = pl.prepare(p, nch, count, nscan, npairs, ci, cf, observing, stc);
    if (!rc) rc = dE.put(E, rows);
    if (!rc && npairs > 0) rc = dD.put(D, (size_t)npairs * count * count);
    if (!rc && stc && stc->n > 0) rc = dW.put(stc->W, (size_t)stc->n * count * count);       // once per call, outside the bound like D
    if (!rc) rc = da.put(a, adbl);
    if (!rc && nsteps > 0) rc = dfield.alloc(g * fdbl);
    if (!rc && snapping) rc = dsnap.alloc(snaps_of(g) * adbl);
    if (!rc && observing) rc = dobs.alloc((obs_of(g) > 0 ? obs_of(g) : 1) * odbl);
    if (!rc) rc = launch_tdse_pack(pl.d, da.p, pl.aw.p, p->st);
    if (!rc && lawson && nsteps > 0) rc = pl.phases(p, dE.p, dt);
    const TdseBufs w = pl.bufs(dE.p, dD.p, dW.p);
    for (int n0 = 0; !rc && n0 < nsteps; n0 += (int)g) {
        const int n1 = n0 + (int)g < nsteps ? n0 + (int)g : nsteps;
        rc = HIP_RC(hipMemcpyAsync(dfield.p, field + (size_t)n0 * fdbl, (size_t)(n1 - n0) * fdbl * sizeof(double), hipMemcpyHostToDevice, p->st));
        const int s0 = snapping ? n0 / snap_every : 0, s1 = snapping ? n1 / snap_every : 0;
        // rows j0 .. j1-1: the observed steps j obs_every of n0 .. n1-1
        const int j0 = observing ? (n0 + obs_every - 1) / obs_every : 0, j1 = observing ? (n1 + obs_every - 1) / obs_every : 0;
        if (!rc) rc = pl.run(p, w, n0, n1, dt, dfield.p, snap_every, snapping ? dsnap.p : nullptr, s0, obs_every, observing ? dobs.p : nullptr, j0);
        if (!rc && s1 > s0)
            rc = HIP_RC(hipMemcpyAsync(snap + (size_t)s0 * adbl, dsnap.p, (size_t)(s1 - s0) * adbl * sizeof(double), hipMemcpyDeviceToHost, p->st));
        if (!rc && j1 > j0)
            rc = HIP_RC(hipMemcpyAsync(obs + (size_t)j0 * odbl, dobs.p, (size_t)(j1 - j0) * odbl * sizeof(double), hipMemcpyDeviceToHost, p->st));
    }
    if (!rc && observing) {
        const size_t last = nsteps > 0 ? (size_t)(nsteps - 1) / obs_every + 1 : 0;
        rc = launch_tdse_observe(pl.d, w, nullptr, dobs.p, p->st);
        if (!rc) rc = HIP_RC(hipMemcpyAsync(obs + last * odbl, dobs.p, odbl * sizeof(double), hipMemcpyDeviceToHost, p->st));
    }
    if (!rc && nsteps > 0) {
        rc = launch_tdse_unpack(pl.d, pl.aw.p, da.p, p->st);
        if (!rc) rc = HIP_RC(hipMemcpyAsync(a, da.p, adbl * sizeof(double), hipMemcpyDeviceToHost, p->st));
    }
    if ((rc = drain(p, rc))) return rc;
    return pl.errors(dt, err);
}

bool obs_args_ok(int obs_every, const double *obs) { return obs_every >= 0 && (obs_every == 0 ? obs == nullptr : obs != nullptr); }

// ---- bspatom_tdse_adaptive ------------------------------------------------------------------------------------------------------
// what the call has beyond bspatom_tdse_static's arguments
struct Adapt {
    int nsub; double tol; int max_level, level0; int64_t *stats; int log_cap; int32_t *log_i; double *log_e, *log_f;
};

// BSP_OK, BSP_ERR_ARG or BSP_ERR_UNSUPPORTED (a legal max_level above the limit)
int adapt_args_rc(const Adapt &ad, int nsteps, const double *fn)
{
    if (!(ad.tol > 0.0) || ad.max_level < 0 || ad.level0 < 0 || ad.level0 > ad.max_level || ad.nsub < 1 || !ad.stats || ad.log_cap < 0) return BSP_ERR_ARG;
    if (nsteps > 0 && !fn) return BSP_ERR_ARG;
    if (ad.log_cap > 0 && (!ad.log_i || !ad.log_e || !ad.log_f)) return BSP_ERR_ARG;
    if (ad.max_level > BSPATOM_TDSE_MAX_LEVEL) return BSP_ERR_UNSUPPORTED;
    return BSP_OK;
}

// attempts enqueued between two looks at the control block (tdse_adapt_group: the test's hook; nothing depends on it)
int adapt_group() { return opts().tdse_adapt_group > 0 ? opts().tdse_adapt_group : 16; }

// One code path for both variants.  host: every array but the lists is in host memory and fn, the snapshots and the rows are staged by
// groups of coarse steps under tdse_stage_bytes(); else they are device memory and the run is one group.
int run_adapt(bspatom_problem *p, bool host, int nch, int count, const double *E, int npairs, const int32_t *ci, const int32_t *cf,
              const double *D, int nscan, int nsteps, double dt, const double *fn, double *a, int snap_every, double *snap, double *err,
              int obs_every, double *obs, bool lawson, const Static &stc, const Adapt &ad)
{
    const bool observing = obs_every > 0, snapping = snap && snap_every > 0;
    for (int k = 0; k < 6; ++k) ad.stats[k] = 0;
    ad.stats[4] = ad.level0;
    if (nsteps == 0 && !observing) {
        if (err) for (int q = 0; q < nscan; ++q) err[q] = 0.0;
        return BSP_OK;
    }
    BSP_HIP(hipSetDevice(p->device));
    const size_t rows = (size_t)nch * count, adbl = rows * nscan * 2, odbl = (size_t)6 * nscan * nch;
    const size_t ndbl = (size_t)4 * nscan;                                 // doubles of a field node: f and df/dt of every scan
    // coarse steps per group (host): its nodes, snapshots and rows within the bound, one step at least
    auto snaps_of = [&](size_t g) { return snapping ? g / snap_every + 1 : (size_t)0; };
    auto obs_of = [&](size_t g) { return observing && g > 0 ? (g - 1) / obs_every + 1 : (size_t)0; };
    auto need = [&](size_t g) { return (g * ad.nsub + 1) * ndbl + snaps_of(g) * adbl + obs_of(g) * odbl; };
    size_t g = nsteps;
    if (host) {
        const size_t bound = tdse_stage_bytes() / sizeof(double);
        while (g > 1 && need(g) > bound) g = (g + 1) / 2;
    }
    Plan pl;
    DevArray<double> dE, dD, dW, da, dfn, dsnap, dobs, cand, dlog_e, dlog_f;
    DevArray<int> dlog_i;
    DevArray<char> dctl;
    int rc = pl.prepare(p, nch, count, nscan, npairs, ci, cf, observing, &stc, true);
    const double *E_dev = E, *D_dev = D, *W_dev = stc.W;
    double *a_dev = a;
    if (host) {
        if (!rc) rc = dE.put(E, rows);
        if (!rc && npairs > 0) rc = dD.put(D, (size_t)npairs * count * count);
        if (!rc && stc.n > 0) rc = dW.put(stc.W, (size_t)stc.n * count * count);
        if (!rc) rc = da.put(a, adbl);
        if (!rc && nsteps > 0) rc = dfn.alloc((g * ad.nsub + 1) * ndbl);
        if (!rc && snapping) rc = dsnap.alloc(snaps_of(g) * adbl);
        if (!rc && observing) rc = dobs.alloc((obs_of(g) > 0 ? obs_of(g) : 1) * odbl);
        if (!rc && ad.log_cap > 0 &&
            ((rc = dlog_i.alloc((size_t)4 * ad.log_cap)) || (rc = dlog_e.alloc((size_t)ad.log_cap * nscan)) ||
             (rc = dlog_f.alloc((size_t)ad.log_cap * 12 * nscan))))
            return drain(p, rc);
        E_dev = dE.p; D_dev = dD.p; W_dev = dW.p; a_dev = da.p;
    }
    if (rc) return drain(p, rc);                    // prepare has work on the stream
    TdseAdaptArgs ga = {ad.nsub, ad.max_level, snapping ? snap_every : 0, obs_every, ad.log_cap, dt, ad.tol, host ? dfn.p : fn,
                        host ? dlog_i.p : ad.log_i, host ? dlog_e.p : ad.log_e, host ? dlog_f.p : ad.log_f};
    if (ad.log_cap == 0) { ga.log_i = nullptr; ga.log_e = ga.log_f = nullptr; }
    rc = launch_tdse_pack(pl.d, a_dev, pl.aw.p, p->st);
    // Lawson: one phase table per level, each what tdse_phase_kernel gives for dt = ldexp(dt, -m)
    const size_t phlev = (size_t)10 * rows;
    if (!rc && lawson && nsteps > 0) {
        rc = pl.ph.alloc(phlev * (ad.max_level + 1));
        for (int m = 0; !rc && m <= ad.max_level; ++m) rc = launch_tdse_phases(pl.d, E_dev, std::ldexp(dt, -m), pl.ph.p + m * phlev, p->st);
    }
    const TdseBufs w = pl.bufs(E_dev, D_dev, W_dev);
    // the control block: the header, the field of the coming attempt, errmax = 0
    std::vector<char> blk(tdse_ctl_bytes(nscan), 0);
    TdseAdaptCtl h = {};
    h.m = ad.level0;
    h.flag = h.row = h.snap = -1;
    h.acc_t = -1;
    h.stats[4] = ad.level0;
    memcpy(blk.data(), &h, sizeof h);
    if (!rc && nsteps > 0) rc = cand.alloc(rows * pl.d.NC);
    if (!rc && nsteps > 0) rc = dctl.put(blk.data(), blk.size());
    TdseAdaptCtl *ctl = (TdseAdaptCtl *)dctl.p;
    // attempts of one coarse step: at most 2^L accepted, and a rejection either deepens the level (L - level at most beyond the
    // coarsenings) or follows a coarsening, of which there is at most one per accepted step: 2^(L+1) + L
    const long long per_step = (2LL << ad.max_level) + ad.max_level;
    for (int n0 = 0; !rc && n0 < nsteps; n0 += (int)g) {
        const int n1 = n0 + (int)g < nsteps ? n0 + (int)g : nsteps;
        const int s0 = snapping ? n0 / snap_every : 0, s1 = snapping ? n1 / snap_every : 0;
        const int j0 = observing ? (n0 + obs_every - 1) / obs_every : 0, j1 = observing ? (n1 + obs_every - 1) / obs_every : 0;
        if (host)
            rc = HIP_RC(hipMemcpyAsync(dfn.p, fn + (size_t)n0 * ad.nsub * ndbl, ((size_t)(n1 - n0) * ad.nsub + 1) * ndbl * sizeof(double),
                                       hipMemcpyHostToDevice, p->st));
        h.nend = n1; h.done = 0; h.row = h.snap = -1;
        h.row0 = j0; h.snap0 = s0; h.node0 = host ? n0 * ad.nsub : 0;
        if (!rc) rc = HIP_RC(hipMemcpyAsync(ctl, &h, sizeof h, hipMemcpyHostToDevice, p->st));
        if (!rc) rc = HIP_RC(hipStreamSynchronize(p->st));
        if (!rc) rc = launch_tdse_adapt_init(pl.d, w, ctl, ga, p->st);
        const long long tmax = h.stats[5] + (long long)(n1 - n0) * per_step;
        while (!rc && !h.done) {
            if (h.stats[5] >= tmax) {
                fprintf(stderr, "bspatom: tdse_adaptive: more than %lld attempts per coarse step (internal error)\n", per_step);
                rc = BSP_ERR_HIP;
                break;
            }
            const int ng = adapt_group();
            for (int i = 0; !rc && i < ng; ++i)
                rc = launch_tdse_adapt_attempt(pl.d, w, ctl, ga, h.stats[5] + i, cand.p, phlev, host ? dsnap.p : snap,
                                               observing ? (host ? dobs.p : obs) : nullptr, p->st);
            if (!rc) rc = HIP_RC(hipMemcpyAsync(&h, ctl, sizeof h, hipMemcpyDeviceToHost, p->st));
            if (!rc) rc = HIP_RC(hipStreamSynchronize(p->st));
        }
        if (host && !rc && s1 > s0)
            rc = HIP_RC(hipMemcpyAsync(snap + (size_t)s0 * adbl, dsnap.p, (size_t)(s1 - s0) * adbl * sizeof(double), hipMemcpyDeviceToHost, p->st));
        if (host && !rc && j1 > j0)
            rc = HIP_RC(hipMemcpyAsync(obs + (size_t)j0 * odbl, dobs.p, (size_t)(j1 - j0) * odbl * sizeof(double), hipMemcpyDeviceToHost, p->st));
        if (host && !rc) rc = HIP_RC(hipStreamSynchronize(p->st));      // the next group writes the same buffers
    }
    if (!rc && observing) {
        const size_t last = nsteps > 0 ? (size_t)(nsteps - 1) / obs_every + 1 : 0;
        rc = launch_tdse_observe(pl.d, w, nullptr, host ? dobs.p : obs + last * odbl, p->st);
        if (host && !rc) rc = HIP_RC(hipMemcpyAsync(obs + last * odbl, dobs.p, odbl * sizeof(double), hipMemcpyDeviceToHost, p->st));
    }
    if (!rc && nsteps > 0) {
        rc = launch_tdse_unpack(pl.d, pl.aw.p, a_dev, p->st);
        if (host && !rc) rc = HIP_RC(hipMemcpyAsync(a, da.p, adbl * sizeof(double), hipMemcpyDeviceToHost, p->st));
    }
    if ((rc = drain(p, rc))) return rc;
    for (int k = 0; k < 6; ++k) ad.stats[k] = h.stats[k];
    ad.stats[4] = h.m;
    if (host && ad.log_cap > 0 && nsteps > 0) {
        const size_t nl = h.stats[5] < ad.log_cap ? (size_t)h.stats[5] : (size_t)ad.log_cap;
        if (nl > 0 && ((rc = dlog_i.get(ad.log_i, 4 * nl)) || (rc = dlog_e.get(ad.log_e, nl * nscan)) || (rc = dlog_f.get(ad.log_f, nl * 12 * nscan))))
            return rc;
    }
    if (err) {
        if (nsteps > 0) BSP_HIP(hipMemcpy(err, dctl.p + TDSE_CTL_HDR + (size_t)12 * nscan * sizeof(double), nscan * sizeof(double), hipMemcpyDeviceToHost));
        else for (int q = 0; q < nscan; ++q) err[q] = 0.0;
    }
    return BSP_OK;
}
}  // namespace

extern "C" int bspatom_tdse_propagate_dev(bspatom_problem *p, int nch, int count, const double *E_dev, int npairs, const int32_t *ci,
                                          const int32_t *cf, const double *D_dev, int nscan, int nsteps, double dt,
                                          const double *field_dev, double *a_dev, int snap_every, double *snap_dev, double *err)
{
    if (!args_ok(p, nch, count, E_dev, npairs, ci, cf, D_dev, nscan, nsteps, dt, field_dev, a_dev, snap_every, snap_dev)) return BSP_ERR_ARG;
    return run_dev(p, nch, count, E_dev, npairs, ci, cf, D_dev, nscan, nsteps, dt, field_dev, a_dev, snap_every, snap_dev, err, 0, nullptr, false);
}

extern "C" int bspatom_tdse_propagate(bspatom_problem *p, int nch, int count, const double *E, int npairs, const int32_t *ci,
                                      const int32_t *cf, const double *D, int nscan, int nsteps, double dt, const double *field,
                                      double *a, int snap_every, double *snap, double *err)
{
    if (!args_ok(p, nch, count, E, npairs, ci, cf, D, nscan, nsteps, dt, field, a, snap_every, snap)) return BSP_ERR_ARG;
    return run_host(p, nch, count, E, npairs, ci, cf, D, nscan, nsteps, dt, field, a, snap_every, snap, err, 0, nullptr, false);
}

extern "C" int bspatom_tdse_observe_dev(bspatom_problem *p, int nch, int count, const double *E_dev, int npairs, const int32_t *ci,
                                        const int32_t *cf, const double *D_dev, int nscan, int nsteps, double dt, const double *field_dev,
                                        double *a_dev, int snap_every, double *snap_dev, double *err, int obs_every, double *obs_dev)
{
    if (!args_ok(p, nch, count, E_dev, npairs, ci, cf, D_dev, nscan, nsteps, dt, field_dev, a_dev, snap_every, snap_dev) ||
        !obs_args_ok(obs_every, obs_dev))
        return BSP_ERR_ARG;
    if (obs_every == 0)
        return bspatom_tdse_propagate_dev(p, nch, count, E_dev, npairs, ci, cf, D_dev, nscan, nsteps, dt, field_dev, a_dev, snap_every, snap_dev, err);
    return run_dev(p, nch, count, E_dev, npairs, ci, cf, D_dev, nscan, nsteps, dt, field_dev, a_dev, snap_every, snap_dev, err, obs_every, obs_dev, false);
}

extern "C" int bspatom_tdse_observe(bspatom_problem *p, int nch, int count, const double *E, int npairs, const int32_t *ci,
                                    const int32_t *cf, const double *D, int nscan, int nsteps, double dt, const double *field, double *a,
                                    int snap_every, double *snap, double *err, int obs_every, double *obs)
{
    if (!args_ok(p, nch, count, E, npairs, ci, cf, D, nscan, nsteps, dt, field, a, snap_every, snap) || !obs_args_ok(obs_every, obs))
        return BSP_ERR_ARG;
    if (obs_every == 0) return bspatom_tdse_propagate(p, nch, count, E, npairs, ci, cf, D, nscan, nsteps, dt, field, a, snap_every, snap, err);
    return run_host(p, nch, count, E, npairs, ci, cf, D, nscan, nsteps, dt, field, a, snap_every, snap, err, obs_every, obs, false);
}

extern "C" int bspatom_tdse_lawson_dev(bspatom_problem *p, int nch, int count, const double *E_dev, int npairs, const int32_t *ci,
                                       const int32_t *cf, const double *D_dev, int nscan, int nsteps, double dt, const double *field_dev,
                                       double *a_dev, int snap_every, double *snap_dev, double *err, int obs_every, double *obs_dev)
{
    if (!args_ok(p, nch, count, E_dev, npairs, ci, cf, D_dev, nscan, nsteps, dt, field_dev, a_dev, snap_every, snap_dev) ||
        !obs_args_ok(obs_every, obs_dev))
        return BSP_ERR_ARG;
    return run_dev(p, nch, count, E_dev, npairs, ci, cf, D_dev, nscan, nsteps, dt, field_dev, a_dev, snap_every, snap_dev, err, obs_every, obs_dev, true);
}

extern "C" int bspatom_tdse_lawson(bspatom_problem *p, int nch, int count, const double *E, int npairs, const int32_t *ci,
                                   const int32_t *cf, const double *D, int nscan, int nsteps, double dt, const double *field, double *a,
                                   int snap_every, double *snap, double *err, int obs_every, double *obs)
{
    if (!args_ok(p, nch, count, E, npairs, ci, cf, D, nscan, nsteps, dt, field, a, snap_every, snap) || !obs_args_ok(obs_every, obs))
        return BSP_ERR_ARG;
    return run_host(p, nch, count, E, npairs, ci, cf, D, nscan, nsteps, dt, field, a, snap_every, snap, err, obs_every, obs, true);
}

extern "C" int bspatom_tdse_static_dev(bspatom_problem *p, int nch, int count, const double *E_dev, int npairs, const int32_t *ci,
                                       const int32_t *cf, const double *D_dev, int nscan, int nsteps, double dt, const double *field_dev,
                                       double *a_dev, int snap_every, double *snap_dev, double *err, int obs_every, double *obs_dev,
                                       int scheme, int nstat, const int32_t *si, const int32_t *sf, const int32_t *skind, const double *W_dev)
{
    if (!args_ok(p, nch, count, E_dev, npairs, ci, cf, D_dev, nscan, nsteps, dt, field_dev, a_dev, snap_every, snap_dev) ||
        !obs_args_ok(obs_every, obs_dev) || !static_args_ok(nch, scheme, nstat, si, sf, skind, W_dev))
        return BSP_ERR_ARG;
    const Static stc = {nstat, si, sf, skind, W_dev};
    return run_dev(p, nch, count, E_dev, npairs, ci, cf, D_dev, nscan, nsteps, dt, field_dev, a_dev, snap_every, snap_dev, err, obs_every, obs_dev,
                   scheme == 1, &stc);
}

extern "C" int bspatom_tdse_static(bspatom_problem *p, int nch, int count, const double *E, int npairs, const int32_t *ci,
                                   const int32_t *cf, const double *D, int nscan, int nsteps, double dt, const double *field, double *a,
                                   int snap_every, double *snap, double *err, int obs_every, double *obs, int scheme, int nstat,
                                   const int32_t *si, const int32_t *sf, const int32_t *skind, const double *W)
{
    if (!args_ok(p, nch, count, E, npairs, ci, cf, D, nscan, nsteps, dt, field, a, snap_every, snap) || !obs_args_ok(obs_every, obs) ||
        !static_args_ok(nch, scheme, nstat, si, sf, skind, W))
        return BSP_ERR_ARG;
    const Static stc = {nstat, si, sf, skind, W};
    return run_host(p, nch, count, E, npairs, ci, cf, D, nscan, nsteps, dt, field, a, snap_every, snap, err, obs_every, obs, scheme == 1, &stc);
}

extern "C" int bspatom_tdse_fields_dev(bspatom_problem *p, int nch, int count, const double *E_dev, int npairs, const int32_t *ci,
                                       const int32_t *cf, const double *D_dev, int nscan, int nsteps, double dt, const double *field_dev,
                                       double *a_dev, int snap_every, double *snap_dev, double *err, int obs_every, double *obs_dev,
                                       int scheme, int nstat, const int32_t *si, const int32_t *sf, const int32_t *skind, const double *W_dev,
                                       int nfield, const int32_t *fidx)
{
    if (!args_ok(p, nch, count, E_dev, npairs, ci, cf, D_dev, nscan, nsteps, dt, field_dev, a_dev, snap_every, snap_dev) ||
        !obs_args_ok(obs_every, obs_dev) || !static_args_ok(nch, scheme, nstat, si, sf, skind, W_dev))
        return BSP_ERR_ARG;
    const int frc = fields_args_rc(nfield, fidx, npairs);
    if (frc) return frc;
    const Static stc = {nstat, si, sf, skind, W_dev, nfield, fidx};
    return run_dev(p, nch, count, E_dev, npairs, ci, cf, D_dev, nscan, nsteps, dt, field_dev, a_dev, snap_every, snap_dev, err, obs_every, obs_dev,
                   scheme == 1, &stc);
}

extern "C" int bspatom_tdse_fields(bspatom_problem *p, int nch, int count, const double *E, int npairs, const int32_t *ci,
                                   const int32_t *cf, const double *D, int nscan, int nsteps, double dt, const double *field, double *a,
                                   int snap_every, double *snap, double *err, int obs_every, double *obs, int scheme, int nstat,
                                   const int32_t *si, const int32_t *sf, const int32_t *skind, const double *W, int nfield, const int32_t *fidx)
{
    if (!args_ok(p, nch, count, E, npairs, ci, cf, D, nscan, nsteps, dt, field, a, snap_every, snap) || !obs_args_ok(obs_every, obs) ||
        !static_args_ok(nch, scheme, nstat, si, sf, skind, W))
        return BSP_ERR_ARG;
    const int frc = fields_args_rc(nfield, fidx, npairs);
    if (frc) return frc;
    const Static stc = {nstat, si, sf, skind, W, nfield, fidx};
    return run_host(p, nch, count, E, npairs, ci, cf, D, nscan, nsteps, dt, field, a, snap_every, snap, err, obs_every, obs, scheme == 1, &stc);
}

extern "C" int bspatom_tdse_adaptive_dev(bspatom_problem *p, int nch, int count, const double *E_dev, int npairs, const int32_t *ci,
                                         const int32_t *cf, const double *D_dev, int nscan, int nsteps, double dt, const double *fn_dev,
                                         double *a_dev, int snap_every, double *snap_dev, double *err, int obs_every, double *obs_dev,
                                         int scheme, int nstat, const int32_t *si, const int32_t *sf, const int32_t *skind,
                                         const double *W_dev, int nsub, double tol, int max_level, int level0, int64_t *stats, int log_cap,
                                         int32_t *log_i_dev, double *log_e_dev, double *log_f_dev)
{
    if (!args_ok(p, nch, count, E_dev, npairs, ci, cf, D_dev, nscan, nsteps, dt, fn_dev, a_dev, snap_every, snap_dev) ||
        !obs_args_ok(obs_every, obs_dev) || !static_args_ok(nch, scheme, nstat, si, sf, skind, W_dev))
        return BSP_ERR_ARG;
    const Adapt ad = {nsub, tol, max_level, level0, stats, log_cap, log_i_dev, log_e_dev, log_f_dev};
    const int arc = adapt_args_rc(ad, nsteps, fn_dev);
    if (arc) return arc;
    const Static stc = {nstat, si, sf, skind, W_dev};
    return run_adapt(p, false, nch, count, E_dev, npairs, ci, cf, D_dev, nscan, nsteps, dt, fn_dev, a_dev, snap_every, snap_dev, err, obs_every,
                     obs_dev, scheme == 1, stc, ad);
}

extern "C" int bspatom_tdse_adaptive(bspatom_problem *p, int nch, int count, const double *E, int npairs, const int32_t *ci,
                                     const int32_t *cf, const double *D, int nscan, int nsteps, double dt, const double *fn, double *a,
                                     int snap_every, double *snap, double *err, int obs_every, double *obs, int scheme, int nstat,
                                     const int32_t *si, const int32_t *sf, const int32_t *skind, const double *W, int nsub, double tol,
                                     int max_level, int level0, int64_t *stats, int log_cap, int32_t *log_i, double *log_e, double *log_f)
{
    if (!args_ok(p, nch, count, E, npairs, ci, cf, D, nscan, nsteps, dt, fn, a, snap_every, snap) || !obs_args_ok(obs_every, obs) ||
        !static_args_ok(nch, scheme, nstat, si, sf, skind, W))
        return BSP_ERR_ARG;
    const Adapt ad = {nsub, tol, max_level, level0, stats, log_cap, log_i, log_e, log_f};
    const int arc = adapt_args_rc(ad, nsteps, fn);
    if (arc) return arc;
    const Static stc = {nstat, si, sf, skind, W};
    return run_adapt(p, true, nch, count, E, npairs, ci, cf, D, nscan, nsteps, dt, fn, a, snap_every, snap, err, obs_every, obs, scheme == 1,
                     stc, ad);
}
