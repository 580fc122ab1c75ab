// capi_tdse.hip -- the twelve bspatom_tdse_* entry points (include/bspatom.h) over one path.  An entry point writes its arguments into
// a TdseCall, the arguments of the widest call with the neutral value where it has none (no rows, no static block, one field, no
// controller); check() holds every argument rule once, in the order the header promises; run() is the one skeleton: the per-channel entry
// lists and the working buffers (Plan), the copies of the host variant, pack, the phase tables of a Lawson run, the groups of coarse
// steps with their staging, the row of the final amplitudes, unpack, drain, the error estimate.  Only "advance this group" differs: the
// step loop of tdse.hip (Plan::steps) or the controller's attempts (Controller::advance, tdse_adapt.hip).  A _dev variant is the same
// run on the caller's device arrays as one group without copies.  The problem handle gives the device and the stream; nothing of a
// solve is read.
#include <cmath>
#include "capi_internal.h"

using namespace bsp;

namespace {
// attempts enqueued between two looks at the control block (tdse_adapt_group: the test's hook; nothing depends on it)
int adapt_group() { return opts().tdse_adapt_group > 0 ? opts().tdse_adapt_group : 16; }

// what bspatom_tdse_adaptive has beyond bspatom_tdse_static's arguments
struct Adapt {
    int nsub; double tol; int max_level, level0; int64_t *stats; int log_cap; int32_t *log_i; double *log_e, *log_f;
};

// PLAIN: rows of 4 (propagate, observe, lawson); STATIC: rows of 6, or of 4 + 2 nfield with several fields (static, fields), fixed steps
// both; ADAPTIVE: the static call with the step under the controller
enum Kind { PLAIN, STATIC, ADAPTIVE };

// the arguments of a call in the header's order; field is the node table fn of an adaptive call.  Host or device pointers as the
// variant has them; ci .. fidx, err, stats are host pointers always
struct TdseCall {
    Kind kind;
    bspatom_problem *p; int nch, count; const double *E; int npairs; const int32_t *ci, *cf; const double *D; int nscan, nsteps; double dt;
    const double *field; double *a; int snap_every; double *snap, *err;
    int obs_every = 0; double *obs = nullptr;
    int scheme = 0, nstat = 0; const int32_t *si = nullptr, *sf = nullptr, *skind = nullptr; const double *W = nullptr;
    int nfield = 1; const int32_t *fidx = nullptr;
    Adapt ad = {};
};

// doubles per (scan, channel) of a row of observables, and of the observing kernel's partials (a static call without static blocks
// runs the plain kernels: partials of 4 under rows of 6)
int row_width(const TdseCall &c) { return c.nfield > 1 ? 4 + 2 * c.nfield : c.kind == PLAIN ? 4 : 6; }
int part_width(const TdseCall &c) { return c.nfield > 1 ? row_width(c) : (c.nstat > 0 || c.kind == ADAPTIVE) ? 6 : 4; }

// BSP_OK, or what the entry point returns before the handle is read: the rules of propagate, observe, static, fields and adaptive in
// this order (a call passes those of the arguments it lacks by their neutral values)
int check(const TdseCall &c)
{
    if (!c.p || !c.E || !c.a || c.nch < 1 || c.count < 1 || c.nscan < 1 || c.nsteps < 0 || c.npairs < 0 || c.snap_every < 0) return BSP_ERR_ARG;
    if (c.nsteps > 0 && !c.field) return BSP_ERR_ARG;
    if (c.npairs > 0 && (!c.ci || !c.cf || !c.D)) return BSP_ERR_ARG;
    if (c.snap && c.snap_every == 0) return BSP_ERR_ARG;
    if (!std::isfinite(c.dt)) return BSP_ERR_ARG;
    for (int q = 0; q < c.npairs; ++q)
        if (c.ci[q] < 0 || c.ci[q] >= c.nch || c.cf[q] < 0 || c.cf[q] >= c.nch || c.ci[q] == c.cf[q]) return BSP_ERR_ARG;
    if (c.obs_every < 0 || (c.obs_every == 0) != (c.obs == nullptr)) return BSP_ERR_ARG;
    if (c.scheme < 0 || c.scheme > 1 || c.nstat < 0) return BSP_ERR_ARG;
    if (c.nstat > 0 && (!c.si || !c.sf || !c.skind || !c.W)) return BSP_ERR_ARG;
    for (int j = 0; j < c.nstat; ++j)
        if (c.si[j] < 0 || c.si[j] >= c.nch || c.sf[j] < 0 || c.sf[j] >= c.nch || c.skind[j] < 0 || c.skind[j] > 1) return BSP_ERR_ARG;
    if (c.nfield < 1) return BSP_ERR_ARG;
    if (c.nfield > BSPATOM_TDSE_MAX_FIELDS) return BSP_ERR_UNSUPPORTED;
    if (!c.fidx && c.nfield > 1 && c.npairs > 0) return BSP_ERR_ARG;
    for (int q = 0; c.fidx && q < c.npairs; ++q)
        if (c.fidx[q] < 0 || c.fidx[q] >= c.nfield) return BSP_ERR_ARG;
    if (c.kind != ADAPTIVE) return BSP_OK;
    const Adapt &ad = c.ad;
    if (!(ad.tol > 0.0) || ad.max_level < 0 || ad.level0 < 0 || ad.level0 > ad.max_level || ad.nsub < 1 || !ad.stats || ad.log_cap < 0) return BSP_ERR_ARG;
    if (ad.log_cap > 0 && (!ad.log_i || !ad.log_e || !ad.log_f)) return BSP_ERR_ARG;
    if (ad.max_level > BSPATOM_TDSE_MAX_LEVEL) return BSP_ERR_UNSUPPORTED;      // a legal level above the limit
    return BSP_OK;
}

// everything of a call that lives on the device, and the sizes of its pieces in doubles
struct Plan {
    TdseDims d;
    DevArray<int> cptr, ent;
    DevArray<double> aw, K, part, ph;
    DevArray<unsigned long long> err2;
    DevArray<double> hE, hD, hW, ha, hfld, hsnap, hobs;     // the host variant: E, D, W, a once; the field, snapshots and rows of a group
    const double *E, *D, *W, *fld;                          // on the device: the caller's arrays (_dev) or the seven above
    double *a, *snap, *obs;                                 // snap, obs: null without snapshots, rows
    size_t rows = 0, adbl = 0, odbl = 0;                    // states; doubles of a snapshot, of a row of observables [nscan][nch][ow]
    size_t fstep = 0, ftail = 0;                            // the field of g coarse steps: g fstep + ftail (the last node of an adaptive group)
    size_t phlev = 0, g = 0;                                // doubles of a phase table; coarse steps per group
    bool host = false, observing = false, snapping = false;
    int ow = 4, nstat = 0, nf = 1, snap_every = 0, obs_every = 0;

    // what n coarse steps in a row hold at most: snapshots, observed steps, doubles of the field, doubles of all three
    size_t snaps_of(size_t n) const { return snapping ? n / snap_every + 1 : (size_t)0; }
    size_t obs_of(size_t n) const { return observing && n > 0 ? (n - 1) / obs_every + 1 : (size_t)0; }
    size_t fld_of(size_t n) const { return n * fstep + ftail; }
    size_t need(size_t n) const { return fld_of(n) + snaps_of(n) * adbl + obs_of(n) * odbl; }

    // Steps per group of the host variant: the field of g steps, their snapshots and their observed steps within the bound, one step
    // at least.  The fixed step walks down by what is over; the adaptive call halves
    size_t group_steps(const TdseCall &c) const
    {
        const size_t bound = tdse_stage_bytes() / sizeof(double);
        size_t n = c.nsteps;
        if (c.kind == ADAPTIVE) {
            while (n > 1 && need(n) > bound) n = (n + 1) / 2;
            return n;
        }
        const size_t per_step = fstep + adbl + (observing ? odbl : 0);
        if (n > bound / fstep) n = bound / fstep;
        while (n > 1 && need(n) > bound) {
            const size_t over = need(n) - bound;
            const size_t dec = over / per_step > 1 ? over / per_step : 1;
            n = n > dec ? n - dec : 1;
        }
        return n < 1 ? 1 : n;
    }

    int prepare(const TdseCall &c, bool host_)
    {
        const int nch = c.nch, npairs = c.npairs, nscan = c.nscan;
        d = {nch, c.count, nscan, tdse_columns(nscan)};
        host = host_;
        observing = c.obs_every > 0;
        snapping = c.snap && c.snap_every > 0;
        snap_every = c.snap_every;
        obs_every = c.obs_every;
        nf = c.nfield;
        ow = row_width(c);
        nstat = c.nstat;
        rows = (size_t)nch * c.count;
        adbl = rows * nscan * 2;
        odbl = (size_t)ow * nscan * nch;
        phlev = (size_t)10 * rows;
        // a fixed step reads 6 values per field and scan; an adaptive coarse step has nsub nodes of f and df/dt per scan, the group one more
        fstep = c.kind == ADAPTIVE ? (size_t)c.ad.nsub * 4 * nscan : (size_t)12 * nscan * nf;
        ftail = c.kind == ADAPTIVE ? (size_t)4 * nscan : 0;
        g = host ? group_steps(c) : c.nsteps;
        const int32_t *fidx = nf > 1 ? c.fidx : nullptr;
        // channel c's entries in ascending p: (p, cf[p], 1) where ci[p] = c, (p, ci[p], 0) where cf[p] = c; behind them its static
        // entries in ascending j: (j, si[j], 2 + skind[j]) where sf[j] = c.  Several fields: a driven entry's third word gains 4 fidx[p]
        std::vector<int> cp(nch + 1, 0), en((size_t)6 * npairs + (size_t)3 * nstat + 3, 0);
        for (int q = 0; q < npairs; ++q) { ++cp[c.ci[q] + 1]; ++cp[c.cf[q] + 1]; }
        for (int j = 0; j < nstat; ++j) ++cp[c.sf[j] + 1];
        for (int ch = 0; ch < nch; ++ch) cp[ch + 1] += cp[ch];
        std::vector<int> at(cp.begin(), cp.end() - 1);
        for (int q = 0; q < npairs; ++q) {
            int *e = &en[(size_t)3 * at[c.ci[q]]++];
            const int g4 = fidx ? 4 * fidx[q] : 0;
            e[0] = q; e[1] = c.cf[q]; e[2] = 1 + g4;
            e = &en[(size_t)3 * at[c.cf[q]]++];
            e[0] = q; e[1] = c.ci[q]; e[2] = g4;
        }
        for (int j = 0; j < nstat; ++j) {
            int *e = &en[(size_t)3 * at[c.sf[j]]++];
            e[0] = j; e[1] = c.si[j]; e[2] = 2 + c.skind[j];
        }
        int rc;
        if ((rc = cptr.put(cp.data(), cp.size())) || (rc = ent.put(en.data(), en.size())) || (rc = aw.alloc(rows * d.NC)) ||
            (rc = K.alloc(6 * rows * d.NC)) || (rc = err2.alloc(nscan)))
            return rc;
        // the observing kernel's partials: part_width doubles per (channel, row tile of 64 states, scan slot)
        if (observing && (rc = part.alloc((size_t)nch * ((c.count + 63) / 64) * (d.NC / 2) * part_width(c)))) return rc;
        return HIP_RC(hipMemsetAsync(err2.p, 0, (size_t)nscan * sizeof(unsigned long long), c.p->st));
    }
    // where the kernels find the caller's arrays; the host variant copies E, D, W and a once per call (outside the bound) and
    // allocates the staging of a group
    int upload(const TdseCall &c)
    {
        E = c.E; D = c.D; W = c.W; fld = c.field; a = c.a; snap = c.snap; obs = c.obs;
        if (!host) return BSP_OK;
        const size_t blk = (size_t)c.count * c.count;
        int rc = hE.put(c.E, rows);
        if (!rc && c.npairs > 0) rc = hD.put(c.D, c.npairs * blk);
        if (!rc && nstat > 0) rc = hW.put(c.W, nstat * blk);
        if (!rc) rc = ha.put(c.a, adbl);
        if (!rc && c.nsteps > 0) rc = hfld.alloc(fld_of(g));
        if (!rc && snapping) rc = hsnap.alloc(snaps_of(g) * adbl);
        if (!rc && observing) rc = hobs.alloc((obs_of(g) > 0 ? obs_of(g) : 1) * odbl);
        E = hE.p; D = hD.p; W = hW.p; fld = hfld.p; a = ha.p; snap = hsnap.p; obs = hobs.p;
        return rc;
    }
    // the Lawson scheme: a phase table per level m, what tdse_phase_kernel gives for dt = ldexp(dt, -m) (a fixed step: level 0 alone)
    int phases(const TdseCall &c, int levels)
    {
        int rc = ph.alloc(phlev * levels);
        for (int m = 0; !rc && m < levels; ++m) rc = launch_tdse_phases(d, E, std::ldexp(c.dt, -m), ph.p + m * phlev, c.p->st);
        return rc;
    }
    // without static blocks W is null: the kernels of the other calls run, whatever ow is
    TdseBufs bufs() const { return {cptr.p, ent.p, E, D, aw.p, K.p, err2.p, observing ? part.p : nullptr, ph.p, nstat > 0 ? W : nullptr, ow, nf}; }
    // host variant: the field of the coarse steps n0 .. n1-1 into the staging buffer
    int stage_in(const TdseCall &c, int n0, int n1)
    {
        if (!host) return BSP_OK;
        return HIP_RC(hipMemcpyAsync(hfld.p, c.field + (size_t)n0 * fstep, fld_of(n1 - n0) * sizeof(double), hipMemcpyHostToDevice, c.p->st));
    }
    // host variant: the group's snapshots s0 .. s1-1 and rows j0 .. j1-1 to the caller
    int stage_out(const TdseCall &c, int s0, int s1, int j0, int j1)
    {
        int rc = BSP_OK;
        if (host && s1 > s0)
            rc = HIP_RC(hipMemcpyAsync(c.snap + (size_t)s0 * adbl, snap, (size_t)(s1 - s0) * adbl * sizeof(double), hipMemcpyDeviceToHost, c.p->st));
        if (host && !rc && j1 > j0)
            rc = HIP_RC(hipMemcpyAsync(c.obs + (size_t)j0 * odbl, obs, (size_t)(j1 - j0) * odbl * sizeof(double), hipMemcpyDeviceToHost, c.p->st));
        return rc;
    }
    // The fixed steps n0 .. n1-1 of a group that starts at snapshot number s0 (from 0) and row j0 (row j = the amplitudes before step
    // j obs_every): fld is the table from step n0 on, snap and obs where snapshot s0 and row j0 go, the later ones behind them
    int steps(const TdseCall &c, const TdseBufs &w, int n0, int n1, int s0, int j0)
    {
        for (int n = n0; n < n1; ++n) {
            double *sn = nullptr, *ob = nullptr;
            if (snap && (n + 1) % snap_every == 0) sn = snap + ((size_t)((n + 1) / snap_every - 1 - s0)) * adbl;
            if (obs && n % obs_every == 0) ob = obs + (size_t)(n / obs_every - j0) * odbl;
            const int rc = launch_tdse_step(d, w, fld + (size_t)(n - n0) * fstep, c.dt, sn, ob, c.p->st);
            if (rc) return rc;
        }
        return BSP_OK;
    }
    // the row of the final amplitudes, behind those of the observed steps
    int last_row(const TdseCall &c, const TdseBufs &w)
    {
        const size_t last = c.nsteps > 0 ? (size_t)(c.nsteps - 1) / obs_every + 1 : 0;
        const int rc = launch_tdse_observe(d, w, nullptr, host ? obs : obs + last * odbl, c.p->st);
        if (rc || !host) return rc;
        return HIP_RC(hipMemcpyAsync(c.obs + last * odbl, obs, odbl * sizeof(double), hipMemcpyDeviceToHost, c.p->st));
    }
    int unpack(const TdseCall &c)
    {
        const int rc = launch_tdse_unpack(d, aw.p, a, c.p->st);
        if (rc || !host) return rc;
        return HIP_RC(hipMemcpyAsync(c.a, a, adbl * sizeof(double), hipMemcpyDeviceToHost, c.p->st));
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

// the host side of bspatom_tdse_adaptive's controller: the control block, the candidate buffer, the log
struct Controller {
    DevArray<double> cand, hlog_e, hlog_f;
    DevArray<int> hlog_i;
    DevArray<char> dctl;
    TdseAdaptCtl h = {};
    TdseAdaptArgs ga = {};
    long long per_step = 0;

    // host variant: the log on the device
    int logs(const TdseCall &c)
    {
        const size_t cap = c.ad.log_cap;
        if (cap == 0) return BSP_OK;
        int rc = hlog_i.alloc(4 * cap);
        if (!rc) rc = hlog_e.alloc(cap * c.nscan);
        return rc ? rc : hlog_f.alloc(cap * 12 * c.nscan);
    }
    // the control block: the header, the field of the coming attempt, errmax = 0
    int start(const TdseCall &c, const Plan &pl)
    {
        const Adapt &ad = c.ad;
        const bool log = ad.log_cap > 0;
        ga = {ad.nsub, ad.max_level, pl.snapping ? c.snap_every : 0, c.obs_every, ad.log_cap, c.dt, ad.tol, pl.fld,
              log ? (pl.host ? hlog_i.p : ad.log_i) : nullptr, log ? (pl.host ? hlog_e.p : ad.log_e) : nullptr,
              log ? (pl.host ? hlog_f.p : ad.log_f) : nullptr};
        h.m = ad.level0;
        h.flag = h.row = h.snap = -1;
        h.acc_t = -1;
        h.stats[4] = ad.level0;
        // attempts of one coarse step: at most 2^L accepted, and a rejection either deepens the level (L - level at most beyond the
        // coarsenings) or follows a coarsening, of which there is at most one per accepted step: 2^(L+1) + L
        per_step = (2LL << ad.max_level) + ad.max_level;
        if (c.nsteps == 0) return BSP_OK;
        std::vector<char> blk(tdse_ctl_bytes(c.nscan), 0);
        memcpy(blk.data(), &h, sizeof h);
        const int rc = cand.alloc(pl.rows * pl.d.NC);
        return rc ? rc : dctl.put(blk.data(), blk.size());
    }
    // the coarse steps n0 .. n1-1: attempts in groups of adapt_group() until the block says done
    int advance(const TdseCall &c, const Plan &pl, const TdseBufs &w, int n0, int n1, int s0, int j0)
    {
        hipStream_t st = c.p->st;
        TdseAdaptCtl *ctl = (TdseAdaptCtl *)dctl.p;
        h.nend = n1; h.done = 0; h.row = h.snap = -1;
        h.row0 = j0; h.snap0 = s0; h.node0 = pl.host ? n0 * c.ad.nsub : 0;
        int rc = HIP_RC(hipMemcpyAsync(ctl, &h, sizeof h, hipMemcpyHostToDevice, st));
        if (!rc) rc = HIP_RC(hipStreamSynchronize(st));
        if (!rc) rc = launch_tdse_adapt_init(pl.d, w, ctl, ga, st);
        const long long tmax = h.stats[5] + (long long)(n1 - n0) * per_step;
        while (!rc && !h.done) {
            if (h.stats[5] >= tmax) {
                fprintf(stderr, "bspatom: tdse_adaptive: more than %lld attempts per coarse step (internal error)\n", per_step);
                return BSP_ERR_HIP;
            }
            const int ng = adapt_group();
            for (int i = 0; !rc && i < ng; ++i) rc = launch_tdse_adapt_attempt(pl.d, w, ctl, ga, h.stats[5] + i, cand.p, pl.phlev, pl.snap, pl.obs, st);
            if (!rc) rc = HIP_RC(hipMemcpyAsync(&h, ctl, sizeof h, hipMemcpyDeviceToHost, st));
            if (!rc) rc = HIP_RC(hipStreamSynchronize(st));
        }
        return rc;
    }
    // after the stream has drained: the counters, the host variant's log, err from the block's errmax
    int finish(const TdseCall &c, const Plan &pl)
    {
        const Adapt &ad = c.ad;
        for (int k = 0; k < 6; ++k) ad.stats[k] = h.stats[k];
        ad.stats[4] = h.m;
        if (pl.host && ad.log_cap > 0 && c.nsteps > 0) {
            const size_t nl = h.stats[5] < ad.log_cap ? (size_t)h.stats[5] : (size_t)ad.log_cap;
            int rc;
            if (nl > 0 && ((rc = hlog_i.get(ad.log_i, 4 * nl)) || (rc = hlog_e.get(ad.log_e, nl * c.nscan)) || (rc = hlog_f.get(ad.log_f, nl * 12 * c.nscan))))
                return rc;
        }
        if (c.err) {
            if (c.nsteps > 0) BSP_HIP(hipMemcpy(c.err, dctl.p + TDSE_CTL_HDR + (size_t)12 * c.nscan * sizeof(double), c.nscan * sizeof(double), hipMemcpyDeviceToHost));
            else for (int q = 0; q < c.nscan; ++q) c.err[q] = 0.0;
        }
        return BSP_OK;
    }
};

// host: every array but the lists is in host memory and the field, the snapshots and the rows are staged by groups of coarse steps
// under tdse_stage_bytes(); else they are device memory and the run is one group.  obs_every = 0: no observables (obs null); otherwise
// rows for the steps 0, obs_every, .. < nsteps, then the row of the final amplitudes
int run(const TdseCall &c, bool host)
{
    bspatom_problem *p = c.p;
    const bool adaptive = c.kind == ADAPTIVE;
    if (adaptive) {
        for (int k = 0; k < 6; ++k) c.ad.stats[k] = 0;
        c.ad.stats[4] = c.ad.level0;
    }
    if (c.nsteps == 0 && c.obs_every == 0) {
        if (c.err) for (int q = 0; q < c.nscan; ++q) c.err[q] = 0.0;
        return BSP_OK;
    }
    BSP_HIP(hipSetDevice(p->device));
    Plan pl;
    Controller ctr;
    int rc = pl.prepare(c, host);
    if (!rc) rc = pl.upload(c);
    if (!rc && adaptive && host) rc = ctr.logs(c);
    if (rc) return drain(p, rc);                    // prepare has work on the stream
    rc = launch_tdse_pack(pl.d, pl.a, pl.aw.p, p->st);
    if (!rc && c.scheme == 1 && c.nsteps > 0) rc = pl.phases(c, adaptive ? c.ad.max_level + 1 : 1);
    const TdseBufs w = pl.bufs();
    if (!rc && adaptive) rc = ctr.start(c, pl);
    for (int n0 = 0; !rc && n0 < c.nsteps; n0 += (int)pl.g) {
        const int n1 = n0 + (int)pl.g < c.nsteps ? n0 + (int)pl.g : c.nsteps;
        // the group's snapshots s0 .. s1-1 and its rows j0 .. j1-1: the observed steps j obs_every of n0 .. n1-1
        const int s0 = pl.snapping ? n0 / c.snap_every : 0, s1 = pl.snapping ? n1 / c.snap_every : 0;
        const int j0 = pl.observing ? (n0 + c.obs_every - 1) / c.obs_every : 0, j1 = pl.observing ? (n1 + c.obs_every - 1) / c.obs_every : 0;
        rc = pl.stage_in(c, n0, n1);
        if (!rc) rc = adaptive ? ctr.advance(c, pl, w, n0, n1, s0, j0) : pl.steps(c, w, n0, n1, s0, j0);
        if (!rc) rc = pl.stage_out(c, s0, s1, j0, j1);
        if (!rc && adaptive && host) rc = HIP_RC(hipStreamSynchronize(p->st));      // the controller's next group writes the same buffers
    }
    if (!rc && pl.observing) rc = pl.last_row(c, w);
    if (!rc && c.nsteps > 0) rc = pl.unpack(c);
    if ((rc = drain(p, rc))) return rc;
    return adaptive ? ctr.finish(c, pl) : pl.errors(c.dt, c.err);
}

int enter(const TdseCall &c, bool host)
{
    const int rc = check(c);
    return rc ? rc : run(c, host);
}
}  // namespace

// The definitions name their parameters alike (the header's _dev names say where an array lives): the 16 of bspatom_tdse_propagate,
// the 2 more of _observe, the 6 more of _static
#define TDSE_ARGS16 p, nch, count, E, npairs, ci, cf, D, nscan, nsteps, dt, field, a, snap_every, snap, err
#define TDSE_ARGS18 TDSE_ARGS16, obs_every, obs
#define TDSE_ARGS24 TDSE_ARGS18, scheme, nstat, si, sf, skind, W
#define TDSE_PARAMS16                                                                                                                  \
    bspatom_problem *p, int nch, int count, const double *E, int npairs, const int32_t *ci, const int32_t *cf, const double *D, int nscan, \
        int nsteps, double dt, const double *field, double *a, int snap_every, double *snap, double *err
#define TDSE_PARAMS18 TDSE_PARAMS16, int obs_every, double *obs
#define TDSE_PARAMS24 TDSE_PARAMS18, int scheme, int nstat, const int32_t *si, const int32_t *sf, const int32_t *skind, const double *W
#define TDSE_PARAMS_ADAPT \
    int nsub, double tol, int max_level, int level0, int64_t *stats, int log_cap, int32_t *log_i, double *log_e, double *log_f
#define TDSE_ARGS_ADAPT {nsub, tol, max_level, level0, stats, log_cap, log_i, log_e, log_f}

extern "C" int bspatom_tdse_propagate(TDSE_PARAMS16) { return enter({PLAIN, TDSE_ARGS16}, true); }
extern "C" int bspatom_tdse_propagate_dev(TDSE_PARAMS16) { return enter({PLAIN, TDSE_ARGS16}, false); }
// obs_every = 0 is propagate: the run without rows
extern "C" int bspatom_tdse_observe(TDSE_PARAMS18) { return enter({PLAIN, TDSE_ARGS18}, true); }
extern "C" int bspatom_tdse_observe_dev(TDSE_PARAMS18) { return enter({PLAIN, TDSE_ARGS18}, false); }
extern "C" int bspatom_tdse_lawson(TDSE_PARAMS18) { return enter({PLAIN, TDSE_ARGS18, 1}, true); }
extern "C" int bspatom_tdse_lawson_dev(TDSE_PARAMS18) { return enter({PLAIN, TDSE_ARGS18, 1}, false); }
extern "C" int bspatom_tdse_static(TDSE_PARAMS24) { return enter({STATIC, TDSE_ARGS24}, true); }
extern "C" int bspatom_tdse_static_dev(TDSE_PARAMS24) { return enter({STATIC, TDSE_ARGS24}, false); }
extern "C" int bspatom_tdse_fields(TDSE_PARAMS24, int nfield, const int32_t *fidx) { return enter({STATIC, TDSE_ARGS24, nfield, fidx}, true); }
extern "C" int bspatom_tdse_fields_dev(TDSE_PARAMS24, int nfield, const int32_t *fidx) { return enter({STATIC, TDSE_ARGS24, nfield, fidx}, false); }
extern "C" int bspatom_tdse_adaptive(TDSE_PARAMS24, TDSE_PARAMS_ADAPT) { return enter({ADAPTIVE, TDSE_ARGS24, 1, nullptr, TDSE_ARGS_ADAPT}, true); }
extern "C" int bspatom_tdse_adaptive_dev(TDSE_PARAMS24, TDSE_PARAMS_ADAPT)
{
    return enter({ADAPTIVE, TDSE_ARGS24, 1, nullptr, TDSE_ARGS_ADAPT}, false);
}
