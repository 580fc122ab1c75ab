// capi_spline.hip -- the TDSE in the B-spline basis (include/bspatom_tdse_spline.h, bspatom_tdse_split.h, bspatom_spline_expect.h) on the
// bands the problem holds on the device; all work goes on the problem's stream and the scratch of a call is freed when it returns.
//   bspatom_tdse_spline / _dev, _wide / _wide_dev: Crank-Nicolson steps on the coupled LU (tdse_spline.hip, tdse_spline_wide.hip);
//   bspatom_tdse_split / _dev, _observe / _observe_dev: split steps, nch one-wave systems per substep (tdse_split.hip);
//   bspatom_spline_expect / _dev: <c| B (x) G |c> on packets (spline_expect.hip), one measurement (ExpectPlan).
//   bspatom_spline_window / _dev: the window operator on packets (include/bspatom_spline_window.h, spline_window.hip), one launch.
// The eight stepped entry points run through one skeleton, SteppedRun: the rules of the arguments they share, the sizes, the host
// variant's staging groups, the loop over them with its copies, the last row, drain.  A flavour (tdse_spline_impl with its wide flag,
// tdse_split_impl with its nexp) makes the checks particular to it, sets up its slots, scratch and kernel arguments, and hands over
// "advance the steps of this staging group", "measure the last row" and "copy the packets and info out".
#include <cmath>
#include "capi_internal.h"

using namespace bsp;

static constexpr int SPLINE_GROUP = 64;                            // steps per launch (tdse_spline_group, tdse_split_group)
// The wide call's launch length when tdse_spline_group is unset: a wide step is slow (48 to 715 ms per matrix at
// nfun = 1024), so the largest g in 1 .. SPLINE_GROUP with
//     g * ceil(nscan / slots) * 16 N bw^2 flop <= SPLINE_WIDE_LAUNCH_FLOP = 27.6e9:
// two seconds at 13.8 Gflop/s per CU, the slowest rate measured for this LU under its model 8 N bw (2 bw).  Nothing computed depends
// on it (S2).
static constexpr double SPLINE_WIDE_LAUNCH_FLOP = 27.6e9;
static int spline_wide_group(int N, int bw, int nscan, int slots)
{
    const double per_step = (double)((nscan + slots - 1) / slots) * 16.0 * (double)N * (double)bw * (double)bw;
    int g = SPLINE_GROUP;
    while (g > 1 && (double)g * per_step > SPLINE_WIDE_LAUNCH_FLOP) --g;
    return g;
}

// One staging group as a flavour's advance sees it: the steps n0 .. n1-1, the table from step n0 on (device memory; null without one), and
// where its snapshots and rows go: snapshot s (from 0, behind step (s+1) snap_every - 1) at snap + (s - s0) snap_one, row j (the packets
// before step j obs_every) at obs + (j - j0) row_one, j0 .. j1-1 in all.  A _dev call is one group on the caller's arrays, s0 = j0 = 0.
struct StepGroup { int n0, n1, s0, j0, j1; const double *table; double *snap, *obs; };

// The stepped run: nsteps steps of nscan packets of nch channels, the per-step table (coef | f) read step by step, a snapshot every
// snap_every steps, a row of observables in front of every obs_every-th step and one of the final packets.  The host variant stages
// the table, the snapshots and the rows by groups of whole steps under tdse_stage_bytes() (one step at least); nothing computed
// depends on the groups.  It never asks which flavour runs.
struct SteppedRun {
    // the arguments the stepped entry points share, as the headers name them (table: coef | f); host or device pointers as dev says
    bspatom_problem *p; int nscan, nch; const int32_t *l; int nabs; const double *WB; const int32_t *w; int nsteps; double dt;
    const double *table; double *c; int snap_every; double *snap; int obs_every, nproj; const double *P; double *obs; int32_t *info; bool dev;
    // plan(): rows in all, steps per staging group; complex length of a packet, doubles of a step's table, of a snapshot, of a row;
    // the snapshots and rows a staging group holds at most; the host variant's staging
    bool snapping, observing;
    int nobs, sgroup;
    size_t N, table_step, snap_one, row_one, gsnaps, grows;
    DevArray<double> dtable, dsnap, dobs;

    // the rules of the shared arguments, BSP_ERR_ARG all; projections without rows are not read
    int check()
    {
        if (!p || !l || !c || !info || nscan < 1 || nch < 1 || nsteps < 0 || nabs < 0 || nproj < 0 || (nabs > 0 && !WB)) return BSP_ERR_ARG;
        if (!std::isfinite(dt) || !(dt > 0.0)) return BSP_ERR_ARG;
        if (snap_every < 0 || (snap && snap_every == 0)) return BSP_ERR_ARG;
        if (obs_every < 0 || (obs_every == 0) != (obs == nullptr) || (obs && nproj > 0 && !P)) return BSP_ERR_ARG;
        if (!obs) nproj = 0;
        return screen_channels(p, l, w, nch, nabs);
    }
    // After the flavour's limits (BSP_ERR_UNSUPPORTED comes first): the sizes for rows of row_width doubles per packet and a table of
    // table_step_ doubles per step (0: none), the staging groups -- a step counted with a snapshot and a row of its own -- and their buffers
    int plan(size_t row_width, size_t table_step_)
    {
        const int n = p->hs.nfun;
        if ((long long)nch * n > 0x3fffffffLL || (long long)nsteps * nscan > 0x3fffffffLL) return BSP_ERR_ARG;
        snapping = snap && snap_every > 0; observing = obs != nullptr;
        nobs = observing ? (nsteps == 0 ? 1 : (nsteps - 1) / obs_every + 2) : 0;
        N = (size_t)nch * n; table_step = table_step_; snap_one = 2 * N * nscan; row_one = row_width * nscan;
        BSP_HIP(hipSetDevice(p->device));
        sgroup = std::max(nsteps, 1);
        if (!dev) {
            const size_t per_step = (table_step + (snapping ? snap_one : 0) + (observing ? row_one : 0)) * sizeof(double);
            sgroup = (int)std::max<size_t>(1, std::min<size_t>(sgroup, tdse_stage_bytes() / std::max<size_t>(per_step, 1)));
        }
        gsnaps = snapping ? (size_t)sgroup / snap_every + 1 : 0; grows = observing ? (size_t)(sgroup - 1) / obs_every + 2 : 0;
        int rc = BSP_OK;
        if (!dev && table_step > 0 && nsteps > 0) rc = dtable.alloc((size_t)sgroup * table_step);
        if (!dev && !rc && snapping) rc = dsnap.alloc(gsnaps * snap_one);
        if (!dev && !rc && observing) rc = dobs.alloc(grows * row_one);
        return rc;
    }
    // advance(StepGroup): enqueue the group's steps and what the flavour does at a group's end; last_row(obs, j0): enqueue the row
    // nobs - 1 of the final packets, to obs + (nobs - 1 - j0) row_one; copy_out(): enqueue the copies of the packets and info
    template <class Advance, class LastRow, class CopyOut>
    int run(Advance advance, LastRow last_row, CopyOut copy_out)
    {
        hipStream_t st = p->st;
        int rc = BSP_OK;
        for (int n0 = 0; !rc && n0 < nsteps; n0 += sgroup) {
            const int n1 = std::min(nsteps, n0 + sgroup);
            // the group's snapshots s0 .. s1-1 and its rows j0 .. j1-1 (the observed steps j obs_every of n0 .. n1-1)
            const int s0 = snapping ? n0 / snap_every : 0, s1 = snapping ? n1 / snap_every : 0;
            const int j0 = observing ? (n0 + obs_every - 1) / obs_every : 0, j1 = observing ? (n1 + obs_every - 1) / obs_every : 0;
            StepGroup g = {n0, n1, s0, j0, j1, nullptr, snapping ? (dev ? snap : dsnap.p) : nullptr, observing ? (dev ? obs : dobs.p) : nullptr};
            if (table_step > 0) {
                g.table = dev ? table + (size_t)n0 * table_step : dtable.p;
                if (!dev) rc = HIP_RC(hipMemcpyAsync(dtable.p, table + (size_t)n0 * table_step, (size_t)(n1 - n0) * table_step * sizeof(double), hipMemcpyHostToDevice, st));
            }
            if (!rc) rc = advance(g);
            if (!rc && !dev && s1 > s0)
                rc = HIP_RC(hipMemcpyAsync(snap + (size_t)s0 * snap_one, dsnap.p, (size_t)(s1 - s0) * snap_one * sizeof(double), hipMemcpyDeviceToHost, st));
            if (!rc && !dev && j1 > j0)
                rc = HIP_RC(hipMemcpyAsync(obs + (size_t)j0 * row_one, dobs.p, (size_t)(j1 - j0) * row_one * sizeof(double), hipMemcpyDeviceToHost, st));
            if (!rc && !dev) rc = HIP_RC(hipStreamSynchronize(st));        // the staging buffers are free for the next group
        }
        if (!rc && observing) {
            rc = last_row(dev ? obs : dobs.p, dev ? 0 : nobs - 1);
            if (!rc && !dev) rc = HIP_RC(hipMemcpyAsync(obs + (size_t)(nobs - 1) * row_one, dobs.p, row_one * sizeof(double), hipMemcpyDeviceToHost, st));
        }
        if (!rc) rc = copy_out();
        return drain(p, rc);
    }
};

// bspatom_tdse_spline / _dev: every step the coupled matrix at z = 2i / dt with the step's coefficients, the packets advanced in place;
// the screening and the scratch rules of the coupled resolvent call.  The steps go out in launches of at most tdse_spline_group; the
// kernels take the group's snap and obs with its first indices.
// wide: the same arguments to tdse_spline_wide.hip, its limit, its slots, its scratch (one vector per slot) and its launch length.
static int tdse_spline_impl(SteppedRun &&r, int ncoup, const int32_t *cr, const int32_t *cc, const int32_t *ctr, int nop, const double *GB, bool wide)
{
    int rc;
    if ((rc = r.check())) return rc;
    if (ncoup < 0 || (ncoup > 0 && (nop < 1 || !cr || !cc || !ctr || !GB || (r.nsteps > 0 && !r.table)))) return BSP_ERR_ARG;
    if ((rc = screen_couplings(r.nch, ncoup, cr, cc, ctr))) return rc;
    bspatom_problem *p = r.p;
    const int n = p->hs.nfun, k = p->hs.k, nch = r.nch, nscan = r.nscan, nabs = r.nabs;
    const bool dev = r.dev, ops = ncoup > 0;
    const int max_band = wide ? resolvent_wide_max_band() : resolvent_coupled_max_band();
    if ((long long)nch * k - 1 > max_band) {
        fprintf(stderr, "bspatom_tdse_spline%s: half-width nch*k - 1 = %lld exceeds BSPATOM_COUPLED%s_MAX_BAND = %d\n", wide ? "_wide" : "",
                (long long)nch * k - 1, wide ? "_WIDE" : "", max_band);
        return BSP_ERR_UNSUPPORTED;
    }
    const size_t coef_step = (size_t)2 * nscan * ncoup * (ops ? nop : 0);
    if ((rc = r.plan((size_t)nch + 2 * r.nproj, coef_step))) return rc;
    const size_t wband = (size_t)(2 * k - 1) * n;
    int slots = 0, nproj = r.nproj;
    if ((rc = wide ? tdse_spline_wide_slots(k, nch, nscan, &slots) : tdse_spline_slots(k, nch, nscan, &slots))) return rc;
    const size_t slot_doubles = wide ? resolvent_wide_slot_doubles(n, k, nch, 1) : resolvent_coupled_slot_doubles(n, k, nch);
    slots = bounded_slots(slots, nscan, slot_doubles);
    const int group = opts().tdse_spline_group > 0 ? opts().tdse_spline_group
                                                   : (wide ? spline_wide_group(nch * n, nch * k - 1, nscan, slots) : SPLINE_GROUP);
    auto launch = [&](const TdseSplineArgs &ta) { return wide ? launch_tdse_spline_wide(ta, slots, p->st) : launch_tdse_spline(ta, slots, p->st); };
    std::vector<int> chan, wsel;
    select_channels(p, r.l, r.w, nch, nabs, chan, wsel);
    std::vector<double> z(2 * (size_t)nch, 0.0);
    for (int ch = 0; ch < nch; ++ch) z[2 * ch + 1] = 2.0 / r.dt;
    DevArray<double> work, dz, dWB, dGB, dc, dP;
    DevArray<int> dchan, dw, dinfo, dcr, dcc, dctr;
    if ((rc = work.alloc((size_t)slots * slot_doubles)) || (rc = dz.put(z.data(), z.size())) || (rc = dchan.put(chan.data(), nch)) ||
        (rc = dw.put(wsel.data(), nch)) || (rc = dinfo.alloc(nscan)) ||
        (ops && ((rc = dcr.put(cr, ncoup)) || (rc = dcc.put(cc, ncoup)) || (rc = dctr.put(ctr, ncoup))))) return rc;
    if (!dev) {
        if ((nabs > 0 && (rc = dWB.put(r.WB, (size_t)nabs * wband))) || (ops && (rc = dGB.put(GB, (size_t)nop * wband))) ||
            (rc = dc.put(r.c, 2 * r.N * nscan)) || (nproj > 0 && (rc = dP.put(r.P, 2 * r.N * nproj)))) return rc;
    }
    BSP_HIP(hipMemsetAsync(dinfo.p, 0, (size_t)nscan * sizeof(int), p->st));
    TdseSplineArgs a = {};
    ResolventCoupledArgs &m = a.m;
    m.n = n; m.k = k; m.nch = nch; m.ncoup = ncoup; m.nop = ops ? nop : 0; m.nproj = nproj;
    m.SB = p->d_SB; m.HB = p->d_HB; m.chan = dchan.p; m.z = dz.p; m.w = dw.p;
    m.WB = nabs > 0 ? (dev ? r.WB : dWB.p) : nullptr;
    m.GB = ops ? (dev ? GB : dGB.p) : nullptr;
    m.cr = dcr.p; m.cc = dcc.p; m.ctr = dctr.p;
    m.P = nproj > 0 ? (dev ? r.P : dP.p) : nullptr;
    m.info = dinfo.p; m.work = work.p;
    a.nscan = nscan; a.g = 4.0 / r.dt; a.c = dev ? r.c : dc.p;
    a.snap_every = r.snapping ? r.snap_every : 0; a.obs_every = r.observing ? r.obs_every : 0;
    return r.run(
        [&](const StepGroup &g) {
            int e = BSP_OK;
            a.snap = g.snap; a.s0 = g.s0; a.obs = g.obs; a.j0 = g.j0;
            for (int m0 = g.n0; !e && m0 < g.n1; m0 += group) {
                a.n0 = m0; a.nst = std::min(group, g.n1 - m0);
                m.acoef = ops ? g.table + (size_t)(m0 - g.n0) * coef_step : nullptr;
                e = launch(a);
            }
            return e;
        },
        [&](double *obs, int j0) {                                         // a launch that only measures
            a.n0 = r.nsteps; a.nst = 0; a.fin = 1; a.jfin = r.nobs - 1; a.snap = nullptr; m.acoef = nullptr;
            a.obs = obs; a.j0 = j0;
            return launch(a);
        },
        [&]() {
            int e = dev ? BSP_OK : HIP_RC(hipMemcpyAsync(r.c, dc.p, 2 * r.N * nscan * sizeof(double), hipMemcpyDeviceToHost, p->st));
            if (!e) e = HIP_RC(hipMemcpyAsync(r.info, dinfo.p, (size_t)nscan * sizeof(int), hipMemcpyDeviceToHost, p->st));
            return e;
        });
}

// What a measurement of nexp operators B_o (x) G_o on packets needs on the device (spline_expect.hip), built once per call: the rows of
// the angular matrices compacted to their non-zero entries -- cos theta couples two neighbours, not nch --, the bands (staged here for
// a host caller), the partials and the slots' scratch.  measure() enqueues the two launches of one measurement.
struct ExpectPlan {
    SplineExpectArgs a = {};
    int slots = 0;
    DevArray<double> work, part, dval, dGE;
    DevArray<int> drptr, didx;
    int init(const bspatom_problem *p, int nscan, int nch, int nexp, const double *B, const double *GE, bool ge_dev)
    {
        const int n = p->hs.nfun, k = p->hs.k;
        if ((long long)nscan * nexp * nch > 0x3fffffffLL || (long long)nexp * nch * nch > 0x3fffffffLL) return BSP_ERR_ARG;
        const int items = nscan * nexp * nch;
        std::vector<int> rptr(1, 0), idx;
        std::vector<double> val;
        for (size_t r = 0; r < (size_t)nexp * nch; ++r) {
            for (int cc = 0; cc < nch; ++cc)
                if (B[r * nch + cc] != 0.0) { idx.push_back(cc); val.push_back(B[r * nch + cc]); }
            rptr.push_back((int)idx.size());
        }
        int rc;
        if ((rc = spline_expect_slots(items, &slots))) return rc;
        const size_t slot_doubles = spline_expect_slot_doubles(n);
        slots = bounded_slots(slots, items, slot_doubles);
        if ((rc = work.alloc((size_t)slots * slot_doubles)) || (rc = part.alloc((size_t)2 * items)) || (rc = drptr.put(rptr.data(), rptr.size())) ||
            (rc = didx.put(idx.data(), idx.size())) || (rc = dval.put(val.data(), val.size())) ||
            (!ge_dev && (rc = dGE.put(GE, (size_t)nexp * (2 * k - 1) * n)))) return rc;
        a.n = n; a.k = k; a.nch = nch; a.nscan = nscan; a.nexp = nexp;
        a.GE = ge_dev ? GE : dGE.p;
        a.rptr = drptr.p; a.cidx = didx.p; a.cval = dval.p;
        a.part = part.p; a.work = work.p;
        return BSP_OK;
    }
    int measure(const double *c_dev, double *e_dev, hipStream_t st)
    {
        a.c = c_dev; a.e = e_dev;
        return launch_spline_expect(a, slots, st);
    }
};

// bspatom_spline_expect / _dev: one measurement on the caller's packets.  The kernels read the packets as 16-byte complex values: a
// device pointer that is not so aligned is copied first.
static int spline_expect_impl(bspatom_problem *p, int nscan, int nch, int nexp, const double *B, const double *GE, const double *c, double *e, bool dev)
{
    if (!p || !c || !e || nscan < 1 || nch < 1 || nexp < 0 || (nexp > 0 && (!B || !GE))) return BSP_ERR_ARG;
    if (nexp == 0) return BSP_OK;
    const int n = p->hs.nfun;
    if ((long long)nch * n > 0x3fffffffLL || (long long)nscan * nch > 0x3fffffffLL) return BSP_ERR_ARG;
    const size_t cdoubles = (size_t)2 * nscan * nch * n, edoubles = (size_t)2 * nscan * nexp;
    BSP_HIP(hipSetDevice(p->device));
    ExpectPlan plan;
    DevArray<double> dc, de;
    int rc;
    if ((rc = plan.init(p, nscan, nch, nexp, B, GE, dev))) return rc;
    const bool copy = !dev || (reinterpret_cast<uintptr_t>(c) & 15) != 0;
    if (copy && (rc = dc.alloc(cdoubles))) return rc;
    if (!dev && (rc = de.alloc(edoubles))) return rc;
    if (copy) rc = HIP_RC(hipMemcpyAsync(dc.p, c, cdoubles * sizeof(double), dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, p->st));
    if (!rc) rc = plan.measure(copy ? dc.p : c, dev ? e : de.p, p->st);
    if (!rc && !dev) rc = HIP_RC(hipMemcpyAsync(e, de.p, edoubles * sizeof(double), hipMemcpyDeviceToHost, p->st));
    return drain(p, rc);
}

// bspatom_spline_window / _dev: one launch over the items (energy, distinct band, block of that band's packets).  The channels' distinct
// bands in the order of their first appearance; a band's packets (q, c) with q, then c ascending, cut into blocks of window_rhs.  The
// kernel reads the packets as 16-byte complex values: a device pointer that is not so aligned is copied first.  info: the head
// blocks' counts [ne][ng][nfac], summed here per energy.
static constexpr int WINDOW_RHS = 8;                               // right-hand sides per factorisation (window_rhs)
static int spline_window_impl(bspatom_problem *p, int nscan, int nch, const int32_t *l, int ne, int nfac, const double *z, const double *c, double *N,
                              int32_t *info, bool dev)
{
    if (!p || !l || !c || !N || !info || nscan < 1 || nch < 1 || ne < 1 || nfac < 0 || nfac > BSPATOM_WINDOW_MAX_FAC || (nfac > 0 && !z)) return BSP_ERR_ARG;
    int rc;
    if ((rc = screen_channels(p, l, nullptr, nch, 0))) return rc;
    const int n = p->hs.nfun, k = p->hs.k;
    if ((long long)nch * n > 0x3fffffffLL || (long long)nscan * nch * ne > 0x3fffffffLL) return BSP_ERR_ARG;
    const int wrhs = opts().window_rhs > 0 ? opts().window_rhs : WINDOW_RHS;
    std::vector<int> chan, wsel, gchan, grp(nch), rhs, bg, b0, bn, bhead;
    select_channels(p, l, nullptr, nch, 0, chan, wsel);
    for (int ch = 0; ch < nch; ++ch) {
        size_t at = 0;
        while (at < gchan.size() && gchan[at] != chan[ch]) ++at;
        if (at == gchan.size()) gchan.push_back(chan[ch]);
        grp[ch] = (int)at;
    }
    const int ng = (int)gchan.size();
    for (int g = 0; g < ng; ++g) {
        const int first = (int)rhs.size();
        for (int q = 0; q < nscan; ++q)
            for (int ch = 0; ch < nch; ++ch)
                if (grp[ch] == g) rhs.push_back(q * nch + ch);
        for (int r0 = first; r0 < (int)rhs.size(); r0 += wrhs) {
            bg.push_back(g); b0.push_back(r0); bn.push_back(std::min(wrhs, (int)rhs.size() - r0)); bhead.push_back(r0 == first);
        }
    }
    const int nblk = (int)bg.size();
    if ((long long)ne * nblk > 0x3fffffffLL) return BSP_ERR_ARG;
    const int items = ne * nblk;
    const size_t cdoubles = (size_t)2 * nscan * nch * n, ndoubles = (size_t)nscan * nch * ne, ninfo = (size_t)ne * ng * nfac;
    BSP_HIP(hipSetDevice(p->device));
    int slots = 0;
    if ((rc = spline_window_slots(k, items, &slots))) return rc;
    const size_t slot_doubles = spline_window_slot_doubles(n, k, wrhs);
    slots = bounded_slots(slots, items, slot_doubles);
    DevArray<double> work, dz, dc, dN;
    DevArray<int> dgchan, drhs, dbg, db0, dbn, dbhead, dinfo;
    const bool copy = !dev || (reinterpret_cast<uintptr_t>(c) & 15) != 0;
    if ((rc = work.alloc((size_t)slots * slot_doubles)) || (rc = nfac > 0 ? dz.put(z, (size_t)2 * ne * nfac) : dz.alloc(1)) || (rc = dgchan.put(gchan.data(), ng)) ||
        (rc = drhs.put(rhs.data(), rhs.size())) || (rc = dbg.put(bg.data(), nblk)) || (rc = db0.put(b0.data(), nblk)) ||
        (rc = dbn.put(bn.data(), nblk)) || (rc = dbhead.put(bhead.data(), nblk)) || (rc = dinfo.alloc(ninfo)) ||
        (copy && (rc = dc.alloc(cdoubles))) || (!dev && (rc = dN.alloc(ndoubles)))) return rc;
    std::vector<int> hinfo(ninfo);
    rc = HIP_RC(hipMemsetAsync(dinfo.p, 0, std::max<size_t>(ninfo, 1) * sizeof(int), p->st));
    if (!rc && copy) rc = HIP_RC(hipMemcpyAsync(dc.p, c, cdoubles * sizeof(double), dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, p->st));
    SplineWindowArgs a = {};
    a.n = n; a.k = k; a.ne = ne; a.nfac = nfac; a.ng = ng; a.nblk = nblk; a.wrhs = wrhs;
    a.SB = p->d_SB; a.HB = p->d_HB;
    a.gchan = dgchan.p; a.rhs = drhs.p; a.bg = dbg.p; a.b0 = db0.p; a.bn = dbn.p; a.bhead = dbhead.p;
    a.z = dz.p; a.c = copy ? dc.p : c; a.N = dev ? N : dN.p; a.info = dinfo.p; a.work = work.p;
    if (!rc) rc = launch_spline_window(a, slots, p->st);
    if (!rc && !dev) rc = HIP_RC(hipMemcpyAsync(N, dN.p, ndoubles * sizeof(double), hipMemcpyDeviceToHost, p->st));
    if (!rc && ninfo > 0) rc = HIP_RC(hipMemcpyAsync(hinfo.data(), dinfo.p, ninfo * sizeof(int), hipMemcpyDeviceToHost, p->st));
    if ((rc = drain(p, rc))) return rc;
    for (int e = 0; e < ne; ++e) {
        int sum = 0;
        for (size_t i = 0; i < (size_t)ng * nfac; ++i) sum += hinfo[(size_t)e * ng * nfac + i];
        info[e] = sum;
    }
    return BSP_OK;
}

// bspatom_tdse_split / _dev: a step is three launches over the nscan * nch one-wave systems -- atomic half step, field step, atomic
// half step -- on two packet buffers that alternate; the atomic matrices are factored once, one per distinct (l, w).  The launches of
// tdse_split_group steps are enqueued, then waited for; the kernels take the place of a step's row and snapshot.  With nexp > 0
// (bspatom_tdse_split_observe) a row is nch + 2 nproj + 2 nexp wide: on an observed step the measuring launches of spline_expect.hip
// run on the buffer the step's first atomic launch reads, in front of it; the kernels of tdse_split.hip write their rows at the width
// they know into a buffer of their own, and one launch per staging group puts the two side by side.
static int tdse_split_impl(SteppedRun &&r, const double *G, const double *Q, const double *lam, int nexp, const double *EB, const double *GE)
{
    int rc;
    if ((rc = r.check())) return rc;
    if (nexp < 0 || (nexp > 0 && (!EB || !GE))) return BSP_ERR_ARG;
    if (r.nsteps > 0 && (!G || !Q || !lam || !r.table)) return BSP_ERR_ARG;
    bspatom_problem *p = r.p;
    const int n = p->hs.nfun, k = p->hs.k, nch = r.nch, nscan = r.nscan, nsteps = r.nsteps, nabs = r.nabs, nproj = r.nproj;
    const bool dev = r.dev;
    if (k > tdse_split_max_k()) {
        fprintf(stderr, "bspatom_tdse_split: k = %d exceeds the one-wave window's limit k <= %d\n", k, tdse_split_max_k());
        return BSP_ERR_UNSUPPORTED;
    }
    if ((long long)nscan * nch > 0x3fffffffLL) return BSP_ERR_ARG;
    if (!r.obs) nexp = 0;
    const bool expecting = nexp > 0;
    const int items = nscan * nch;
    // RW0: the row as the kernels of tdse_split.hip write it; the caller's row has the 2 nexp doubles of the measurements behind it
    const size_t RW0 = (size_t)nch + 2 * nproj, f_step = (size_t)2 * nscan;
    if ((rc = r.plan(RW0 + 2 * (size_t)nexp, f_step))) return rc;
    const size_t N = r.N, wband = (size_t)(2 * k - 1) * n, snap_one = r.snap_one, row_one = r.row_one, row0_one = RW0 * nscan,
                 e_one = (size_t)2 * nexp * nscan;   // doubles
    int slots = 0;
    if ((rc = tdse_split_slots(k, items, &slots))) return rc;
    const size_t slot_doubles = tdse_split_slot_doubles(n, k), fac_doubles = tdse_split_factor_doubles(n, k);
    slots = bounded_slots(slots, items, slot_doubles);
    const int group = opts().tdse_split_group > 0 ? opts().tdse_split_group : SPLINE_GROUP;
    // the channels, and the distinct (band, absorber) pairs among them in the order of their first appearance: one atomic matrix each
    std::vector<int> chan, wsel, fac(nch), fchan, fw;
    select_channels(p, r.l, r.w, nch, nabs, chan, wsel);
    for (int ch = 0; ch < nch; ++ch) {
        size_t at = 0;
        while (at < fchan.size() && (fchan[at] != chan[ch] || fw[at] != wsel[ch])) ++at;
        if (at == fchan.size()) { fchan.push_back(chan[ch]); fw.push_back(wsel[ch]); }
        fac[ch] = (int)at;
    }
    const int nfac = (int)fchan.size();
    DevArray<double> work, fstore, buf0, buf1, dQ, dlam, dpart, dWB, dG, dP, drow0, dexp;
    DevArray<int> dfac, dfchan, dfw, dfinfo, dpinfo;
    ExpectPlan plan;
    if (expecting && ((rc = plan.init(p, nscan, nch, nexp, EB, GE, dev)) || (rc = drow0.alloc(r.grows * row0_one)) || (rc = dexp.alloc(r.grows * e_one))))
        return rc;
    if ((rc = work.alloc((size_t)slots * slot_doubles)) || (rc = fstore.alloc((size_t)nfac * fac_doubles)) || (rc = buf0.alloc(2 * N * nscan)) ||
        (rc = buf1.alloc(2 * N * nscan)) || (rc = dpart.alloc((size_t)2 * nscan * nproj * nch)) ||
        (rc = dfac.put(fac.data(), nch)) || (rc = dfchan.put(fchan.data(), nfac)) ||
        (rc = dfw.put(fw.data(), nfac)) || (rc = dfinfo.alloc(nfac)) || (rc = dpinfo.alloc(items)) ||
        (nsteps > 0 && ((rc = dQ.put(Q, (size_t)nch * nch)) || (rc = dlam.put(lam, nch))))) return rc;
    if (!dev) {
        if ((nabs > 0 && (rc = dWB.put(r.WB, (size_t)nabs * wband))) || (nsteps > 0 && (rc = dG.put(G, wband))) ||
            (nproj > 0 && (rc = dP.put(r.P, 2 * N * nproj)))) return rc;
    }
    BSP_HIP(hipMemsetAsync(dfinfo.p, 0, (size_t)nfac * sizeof(int), p->st));
    BSP_HIP(hipMemsetAsync(dpinfo.p, 0, (size_t)items * sizeof(int), p->st));
    BSP_HIP(hipMemcpyAsync(buf0.p, r.c, 2 * N * nscan * sizeof(double), dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, p->st));
    TdseSplitArgs a = {};
    a.n = n; a.k = k; a.nch = nch; a.nscan = nscan; a.nproj = nproj; a.nfac = nfac;
    a.SB = p->d_SB; a.HB = p->d_HB;
    a.WB = nabs > 0 ? (dev ? r.WB : dWB.p) : nullptr;
    a.GB = nsteps > 0 ? (dev ? G : dG.p) : nullptr;
    a.fac = dfac.p; a.fchan = dfchan.p; a.fw = dfw.p;
    a.Q = dQ.p; a.lam = dlam.p;
    a.P = nproj > 0 ? (dev ? r.P : dP.p) : nullptr;
    a.g = 8.0 / r.dt; a.zi = 4.0 / r.dt; a.h = 0.5 * r.dt;
    a.part = dpart.p; a.fstore = fstore.p; a.finfo = dfinfo.p; a.pinfo = dpinfo.p; a.work = work.p;
    double *buf[2] = {buf0.p, buf1.p};
    int cur = 0;                                                       // the buffer that holds the packets
    if (nsteps > 0 && (rc = launch_tdse_split(a, 0, slots, p->st))) return drain(p, rc);
    // one launch on the packets in buf[cur]; what = 1: an atomic half step, 2: the field step
    auto launch = [&](int what, int mix, int measure, const double *fq, double *row, double *sn) {
        a.mix = mix; a.measure = measure; a.f = fq; a.row = row; a.snap = sn;
        a.in = buf[cur]; a.out = buf[cur ^ 1];
        const int e = launch_tdse_split(a, what, slots, p->st);
        if (!e && !measure) cur ^= 1;
        return e;
    };
    std::vector<int> finfo(nfac), pinfo(items);
    rc = r.run(
        [&](const StepGroup &g) {
            int e = BSP_OK;
            for (int m = g.n0; !e && m < g.n1; ++m) {
                const bool observed = r.observing && m % r.obs_every == 0;
                const size_t jr = observed ? (size_t)(m / r.obs_every - g.j0) : 0;      // the row's place in the group
                double *row = observed ? (expecting ? drow0.p + jr * row0_one : g.obs + jr * row_one) : nullptr;
                double *sn = r.snapping && (m + 1) % r.snap_every == 0 ? g.snap + (size_t)((m + 1) / r.snap_every - 1 - g.s0) * snap_one : nullptr;
                if (row && expecting) e = plan.measure(buf[cur], dexp.p + jr * e_one, p->st);
                if (!e) e = launch(1, 0, 0, nullptr, row, nullptr);
                if (!e) e = launch(2, 0, 0, g.table + (size_t)(m - g.n0) * f_step, nproj > 0 ? row : nullptr, nullptr);
                if (!e) e = launch(1, 1, 0, nullptr, nullptr, sn);
                if (!e && ((m + 1 - g.n0) % group == 0 || m + 1 == g.n1)) e = HIP_RC(hipStreamSynchronize(p->st));
            }
            if (!e && expecting && g.j1 > g.j0) e = launch_spline_expect_rows(g.obs, drow0.p, dexp.p, (int)RW0, nexp, (g.j1 - g.j0) * nscan, p->st);
            return e;
        },
        [&](double *obs, int j0) {                                         // launches that only measure
            double *wide = obs + (size_t)(r.nobs - 1 - j0) * row_one, *row = expecting ? drow0.p : wide;
            int e = expecting ? plan.measure(buf[cur], dexp.p, p->st) : BSP_OK;
            if (!e) e = launch(1, 0, 1, nullptr, row, nullptr);
            if (!e && nproj > 0) e = launch(2, 0, 1, nullptr, row, nullptr);
            if (!e && expecting) e = launch_spline_expect_rows(wide, drow0.p, dexp.p, (int)RW0, nexp, nscan, p->st);
            return e;
        },
        [&]() {
            int e = BSP_OK;
            if (nsteps > 0) e = HIP_RC(hipMemcpyAsync(r.c, buf[cur], 2 * N * nscan * sizeof(double), dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, p->st));
            if (!e) e = HIP_RC(hipMemcpyAsync(finfo.data(), dfinfo.p, (size_t)nfac * sizeof(int), hipMemcpyDeviceToHost, p->st));
            if (!e) e = HIP_RC(hipMemcpyAsync(pinfo.data(), dpinfo.p, (size_t)items * sizeof(int), hipMemcpyDeviceToHost, p->st));
            return e;
        });
    if (rc) return rc;
    // info[q]: the replaced pivots of scan q's field factorisations plus those of the call's atomic ones
    int atomic = 0;
    for (int v : finfo) atomic += v;
    for (int q = 0; q < nscan; ++q) {
        int s = nsteps > 0 ? atomic : 0;
        for (int j = 0; j < nch; ++j) s += pinfo[(size_t)q * nch + j];
        r.info[q] = s;
    }
    return BSP_OK;
}

// The definitions name their parameters alike (the headers' _dev names say where an array lives)
#define SPLINE_PARAMS                                                                                                                       \
    bspatom_problem *p, int nscan, int nch, const int32_t *l, int nabs, const double *WB, const int32_t *w, int ncoup, const int32_t *cr,      \
        const int32_t *cc, const int32_t *ctr, int nop, const double *GB, int nsteps, double dt, const double *coef, double *c, int snap_every, \
        double *snap, int obs_every, int nproj, const double *P, double *obs, int32_t *info
#define SPLINE_CALL(dev, wide)                                                                                                              \
    tdse_spline_impl({p, nscan, nch, l, nabs, WB, w, nsteps, dt, coef, c, snap_every, snap, obs_every, nproj, P, obs, info, dev}, ncoup, cr, cc, \
                     ctr, nop, GB, wide)
#define SPLIT_PARAMS                                                                                                                        \
    bspatom_problem *p, int nscan, int nch, const int32_t *l, int nabs, const double *WB, const int32_t *w, const double *G, const double *Q,  \
        const double *lam, int nsteps, double dt, const double *f, double *c, int snap_every, double *snap, int obs_every, int nproj,           \
        const double *P, double *obs, int32_t *info
#define SPLIT_CALL(dev, nexp, B, GE) \
    tdse_split_impl({p, nscan, nch, l, nabs, WB, w, nsteps, dt, f, c, snap_every, snap, obs_every, nproj, P, obs, info, dev}, G, Q, lam, nexp, B, GE)

extern "C" int bspatom_tdse_spline(SPLINE_PARAMS) { return SPLINE_CALL(false, false); }
extern "C" int bspatom_tdse_spline_dev(SPLINE_PARAMS) { return SPLINE_CALL(true, false); }
extern "C" int bspatom_tdse_spline_wide(SPLINE_PARAMS) { return SPLINE_CALL(false, true); }
extern "C" int bspatom_tdse_spline_wide_dev(SPLINE_PARAMS) { return SPLINE_CALL(true, true); }
extern "C" int bspatom_tdse_split(SPLIT_PARAMS) { return SPLIT_CALL(false, 0, nullptr, nullptr); }
extern "C" int bspatom_tdse_split_dev(SPLIT_PARAMS) { return SPLIT_CALL(true, 0, nullptr, nullptr); }
extern "C" int bspatom_tdse_split_observe(SPLIT_PARAMS, int nexp, const double *B, const double *GE) { return SPLIT_CALL(false, nexp, B, GE); }
extern "C" int bspatom_tdse_split_observe_dev(SPLIT_PARAMS, int nexp, const double *B, const double *GE) { return SPLIT_CALL(true, nexp, B, GE); }
#define EXPECT_PARAMS bspatom_problem *p, int nscan, int nch, int nexp, const double *B, const double *GE, const double *c, double *e
extern "C" int bspatom_spline_expect(EXPECT_PARAMS) { return spline_expect_impl(p, nscan, nch, nexp, B, GE, c, e, false); }
extern "C" int bspatom_spline_expect_dev(EXPECT_PARAMS) { return spline_expect_impl(p, nscan, nch, nexp, B, GE, c, e, true); }
#define WINDOW_PARAMS bspatom_problem *p, int nscan, int nch, const int32_t *l, int ne, int nfac, const double *z, const double *c, double *N, int32_t *info
extern "C" int bspatom_spline_window(WINDOW_PARAMS) { return spline_window_impl(p, nscan, nch, l, ne, nfac, z, c, N, info, false); }
extern "C" int bspatom_spline_window_dev(WINDOW_PARAMS) { return spline_window_impl(p, nscan, nch, l, ne, nfac, z, c, N, info, true); }
