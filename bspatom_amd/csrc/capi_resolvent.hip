// capi_resolvent.hip -- the resolvent entry points of include/bspatom.h: solves with the banded pencil at complex energies,
// (H_l - i W - z S) x = b.  The bands are those the problem holds on the device (the last bspatom_solve or bspatom_assemble); all
// work goes on the problem's stream and the scratch of a call is freed when it returns.
//   bspatom_resolvent / _dev: one channel per matrix, resolvent.hip's one-wave LU.
//   bspatom_resolvent_chain / _dev: chains of such solves with an operator in between, one launch for the whole batch.
//   bspatom_resolvent_coupled / _dev: several channels coupled to all orders in one banded LU (resolvent_coupled.hip).
//   bspatom_resolvent_coupled_wide / _dev: the same call on the blocked LU for wide bands (resolvent_wide.hip).
//   bspatom_tdse_spline / _dev: Crank-Nicolson steps on the coupled LU (tdse_spline.hip); a call path of its own below (every packet
//     has its own right-hand side and the steps follow each other), the screening and the scratch rules of the coupled call.
//   bspatom_tdse_spline_wide / _dev: the same call on the blocked LU for wide bands (tdse_spline_wide.hip), through the same path.
//   bspatom_tdse_split / _dev: split Crank-Nicolson steps, nch one-wave systems per substep (tdse_split.hip); a call path of its own.
//   bspatom_spline_expect / _dev: <c| B (x) G |c> on packets in the spline basis (spline_expect.hip);
//   bspatom_tdse_split_observe / _dev: the split call's path with those numbers appended to its rows.
// The eight resolvent entry points run through resolvent_call: a front function per flavour screens what is particular to it, describes the call by
// counts per ITEM (a matrix, a chain, a coupled matrix) and hands over its slot query and its launcher.
#include <algorithm>
#include <cmath>
#include "capi_internal.h"

using namespace bsp;

static constexpr size_t RESOLVENT_STAGE_BYTES = (size_t)2048 << 20;
static constexpr size_t SPLINE_STAGE_BYTES = (size_t)256 << 20;    // tdse_stage_mb's default (capi_tdse.hip)
static constexpr int SPLINE_GROUP = 64;                            // steps per launch (tdse_spline_group)
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

// A call as the shared path sees it: the caller's arrays and how much of each an item takes (single | chain | coupled)
struct ResolventCall {
    int items;                                 // nmat | nchain | nmat
    int rec;                                   // records of l, z, w per item: 1 | nstage | nch
    int ninfo;                                 // info words per item: 1 | nstage | 1
    int rrows;                                 // rows [nrhs][nproj] of R per item: 1 | nstage | 1
    size_t len;                                // complex length of a vector of B, P, X: n | n | nch*n
    size_t ncoef;                              // coefficient doubles per item: 0 | (nstage-1)*nop | 2*ncoup*nop; 0: no operator bands
    size_t slot_doubles;                       // scratch of one work slot of the flavour's kernel
    int nabs, nop, ncoup, nrhs, nproj;         // bands of WB and GB, entries of the topology arrays (coupled only), vectors of B and P
    const int32_t *l, *w, *cr, *cc, *ctr;
    const double *z, *WB, *GB, *ac, *B, *P;
    double *X, *R;
    int32_t *info;
};
// The device arrays of one group of items, each at the group's first item: what a launcher puts into its kernel's arguments
struct ResolventPtrs {
    const int *chan, *w, *cr, *cc, *ctr;
    const double *z, *WB, *GB, *acoef, *B, *P;
    double *X, *R, *work;
    int *info;
};

// The checks every flavour makes: the pointers, the counts, every record's channel among the bands and its absorber among WB's.
// (They return one code and print nothing: their order among themselves and the fronts' other BSP_ERR_ARG checks cannot be seen.)
static int resolvent_screen(const bspatom_problem *p, const ResolventCall &c)
{
    if (!p || !c.l || !c.z || !c.B || !c.info || (!c.X && !c.R)) return BSP_ERR_ARG;
    if (c.items < 1 || c.rec < 1 || c.nrhs < 1 || c.nabs < 0 || c.nproj < 0 || (c.nabs > 0 && !c.WB)) return BSP_ERR_ARG;
    if (c.R && (!c.P || c.nproj < 1)) return BSP_ERR_ARG;
    for (int m = 0; m < c.items * c.rec; ++m) {
        if (p->band_nl < 1 || c.l[m] < p->band_l0 || c.l[m] >= p->band_l0 + p->band_nl) return BSP_ERR_ARG;
        if (c.w && (c.w[m] < -1 || c.w[m] >= c.nabs)) return BSP_ERR_ARG;
    }
    return BSP_OK;
}

// What the kernels' argument structs have in common (common.h), from the problem, the call and a group's pointers
template <class Args>
static void resolvent_fill(Args &a, const bspatom_problem *p, const ResolventCall &c, const ResolventPtrs &d)
{
    a.n = p->hs.nfun; a.k = p->hs.k; a.nrhs = c.nrhs; a.nproj = c.R ? c.nproj : 0;
    a.SB = p->d_SB; a.HB = p->d_HB;
    a.chan = d.chan; a.z = d.z; a.WB = d.WB; a.w = d.w; a.B = d.B; a.P = d.P;
    a.X = d.X; a.R = d.R; a.info = d.info; a.work = d.work;
}

// The one call path, for a screened call.  query(&slots): the work slots the flavour's kernel keeps resident; launch(g, slots, d, st):
// its launcher for g items at the pointers d.  dev: the caller's WB, GB, B, P, X, R are device memory (l, z, w, the topology, the
// coefficients and info are host memory in both variants).
template <class Query, class Launch>
static int resolvent_call(bspatom_problem *p, const ResolventCall &c, bool dev, Query query, Launch launch)
{
    const int n = p->hs.nfun, k = p->hs.k, nrec = c.items * c.rec;
    const size_t wband = (size_t)(2 * k - 1) * n, stage = opts().resolvent_stage_mb > 0 ? (size_t)opts().resolvent_stage_mb << 20 : RESOLVENT_STAGE_BYTES;
    BSP_HIP(hipSetDevice(p->device));
    int rc;
    // the work slots: what is resident, within the scratch bound, one at least
    int slots = 0;
    if ((rc = query(&slots))) return rc;
    if (opts().resolvent_slots > 0) slots = std::min(opts().resolvent_slots, c.items);
    slots = (int)std::max<size_t>(1, std::min<size_t>(slots, stage / (c.slot_doubles * sizeof(double))));
    // the host variant's groups: the X of one group within the bound, one item at least
    const size_t x_item = (size_t)2 * c.nrhs * c.len, r_item = (size_t)2 * c.rrows * c.nrhs * c.nproj;   // doubles of one item's X, R
    int group = c.items;
    if (!dev && c.X) group = (int)std::max<size_t>(1, std::min<size_t>(c.items, stage / (x_item * sizeof(double))));
    std::vector<int> chan(nrec), wsel(nrec, c.nabs > 0 && !c.w ? 0 : -1);
    for (int m = 0; m < nrec; ++m) { chan[m] = c.l[m] - p->band_l0; if (c.w) wsel[m] = c.w[m]; }
    const bool ops = c.ncoef > 0;
    DevArray<double> work, dz, dac, dWB, dGB, dB, dP, dX, dR;
    DevArray<int> dchan, dw, dinfo, dcr, dcc, dctr;
    if ((rc = work.alloc((size_t)slots * c.slot_doubles)) || (rc = dz.put(c.z, (size_t)2 * nrec)) ||
        (ops && (rc = dac.put(c.ac, c.items * c.ncoef))) ||
        (c.ncoup > 0 && ((rc = dcr.put(c.cr, c.ncoup)) || (rc = dcc.put(c.cc, c.ncoup)) || (rc = dctr.put(c.ctr, c.ncoup)))) ||
        (rc = dchan.put(chan.data(), nrec)) || (rc = dw.put(wsel.data(), nrec)) || (rc = dinfo.alloc((size_t)c.items * c.ninfo))) return rc;
    if (!dev) {
        if ((c.nabs > 0 && (rc = dWB.put(c.WB, (size_t)c.nabs * wband))) || (ops && (rc = dGB.put(c.GB, (size_t)c.nop * wband))) ||
            (rc = dB.put(c.B, (size_t)2 * c.nrhs * c.len)) || (c.R && (rc = dP.put(c.P, (size_t)2 * c.nproj * c.len))) ||
            (c.X && (rc = dX.alloc((size_t)group * x_item))) || (c.R && (rc = dR.alloc(c.items * r_item))))
            return rc;
    }
    ResolventPtrs d;
    d.WB = c.nabs > 0 ? (dev ? c.WB : dWB.p) : nullptr;
    d.GB = ops ? (dev ? c.GB : dGB.p) : nullptr;
    d.cr = dcr.p; d.cc = dcc.p; d.ctr = dctr.p;
    d.B = dev ? c.B : dB.p;
    d.P = c.R ? (dev ? c.P : dP.p) : nullptr;
    d.work = work.p;
    rc = BSP_OK;
    for (int m0 = 0; !rc && m0 < c.items; m0 += group) {
        const int g = std::min(group, c.items - m0);
        const size_t r0 = (size_t)m0 * c.rec;
        d.chan = dchan.p + r0; d.z = dz.p + 2 * r0; d.w = dw.p + r0; d.info = dinfo.p + (size_t)m0 * c.ninfo;
        d.acoef = ops ? dac.p + m0 * c.ncoef : nullptr;
        d.X = c.X ? (dev ? c.X + m0 * x_item : dX.p) : nullptr;
        d.R = c.R ? (dev ? c.R : dR.p) + m0 * r_item : nullptr;
        rc = launch(g, std::min(slots, g), d, p->st);
        if (!rc && !dev && c.X) rc = HIP_RC(hipMemcpyAsync(c.X + m0 * x_item, dX.p, g * x_item * sizeof(double), hipMemcpyDeviceToHost, p->st));
    }
    if (!rc && !dev && c.R) rc = HIP_RC(hipMemcpyAsync(c.R, dR.p, c.items * r_item * sizeof(double), hipMemcpyDeviceToHost, p->st));
    if (!rc) rc = HIP_RC(hipMemcpyAsync(c.info, dinfo.p, (size_t)c.items * c.ninfo * sizeof(int), hipMemcpyDeviceToHost, p->st));
    return drain(p, rc);
}

// bspatom_resolvent / _dev: a matrix is an item of one record
static int resolvent_impl(bspatom_problem *p, int nmat, const int32_t *l, const double *z, int nabs, const double *WB, const int32_t *w,
                          int nrhs, const double *B, int nproj, const double *P, double *X, double *R, int32_t *info, bool dev)
{
    ResolventCall c = {};
    c.items = nmat; c.rec = c.ninfo = c.rrows = 1;
    c.nabs = nabs; c.nrhs = nrhs; c.nproj = nproj;
    c.l = l; c.w = w; c.z = z; c.WB = WB; c.B = B; c.P = P; c.X = X; c.R = R; c.info = info;
    int rc = resolvent_screen(p, c);
    if (rc) return rc;
    const int n = p->hs.nfun, k = p->hs.k;
    c.len = n;
    c.slot_doubles = resolvent_slot_doubles(n, k);
    return resolvent_call(p, c, dev, [&](int *slots) { return resolvent_slots(k, nmat, slots); },
                          [&](int g, int slots, const ResolventPtrs &d, hipStream_t st) {
                              ResolventArgs a;
                              resolvent_fill(a, p, c, d);
                              a.nmat = g;
                              return launch_resolvent(a, slots, st);
                          });
}

// bspatom_resolvent_chain / _dev: a chain is an item of nstage records, with a row of R and an info word per stage and the
// coefficients of the nstage - 1 operators between them; the slots are resolvent_chain_kernel's (its scratch holds nrhs more vectors)
static int resolvent_chain_impl(bspatom_problem *p, int nchain, int nstage, const int32_t *l, const double *z, int nabs, const double *WB,
                                const int32_t *w, int nop, const double *GB, const double *ac, int nrhs, const double *B, int nproj,
                                const double *P, double *X, double *R, int32_t *info, bool dev)
{
    if (nop < 0 || (nstage > 1 && (nop < 1 || !GB || !ac))) return BSP_ERR_ARG;
    if ((long long)nchain * nstage > 0x3fffffffLL) return BSP_ERR_ARG;
    ResolventCall c = {};
    c.items = nchain; c.rec = c.ninfo = c.rrows = nstage;
    c.nabs = nabs; c.nop = nop; c.nrhs = nrhs; c.nproj = nproj;
    c.l = l; c.w = w; c.z = z; c.WB = WB; c.GB = GB; c.ac = ac; c.B = B; c.P = P; c.X = X; c.R = R; c.info = info;
    int rc = resolvent_screen(p, c);
    if (rc) return rc;
    const int n = p->hs.nfun, k = p->hs.k;
    c.len = n;
    c.ncoef = (size_t)(nstage - 1) * nop;
    c.slot_doubles = resolvent_chain_slot_doubles(n, k, nrhs);
    return resolvent_call(p, c, dev, [&](int *slots) { return resolvent_chain_slots(k, nchain, slots); },
                          [&](int g, int slots, const ResolventPtrs &d, hipStream_t st) {
                              ResolventChainArgs a;
                              resolvent_fill(a, p, c, d);
                              a.nchain = g; a.nstage = nstage; a.nop = nstage > 1 ? nop : 0;
                              a.GB = d.GB; a.acoef = d.acoef;
                              return launch_resolvent_chain(a, slots, st);
                          });
}

// bspatom_resolvent_coupled / _dev: a matrix of nch coupled channels is an item of nch records and vectors of nch * n, one workgroup
// per matrix (resolvent_coupled.hip), the coupling topology and its complex coefficients beside the records.
// wide: the same arguments to resolvent_wide.hip, its limit, its slots and its scratch.
static int resolvent_coupled_impl(bspatom_problem *p, int nmat, int nch, const int32_t *l, const double *z, int nabs, const double *WB,
                                  const int32_t *w, int ncoup, const int32_t *cr, const int32_t *cc, const int32_t *ctr, int nop,
                                  const double *GB, const double *ac, int nrhs, const double *B, int nproj, const double *P, double *X,
                                  double *R, int32_t *info, bool dev, bool wide)
{
    if (ncoup < 0 || (ncoup > 0 && (nop < 1 || !cr || !cc || !ctr || !GB || !ac))) return BSP_ERR_ARG;
    if ((long long)nmat * nch > 0x3fffffffLL) return BSP_ERR_ARG;
    ResolventCall c = {};
    c.items = nmat; c.rec = nch; c.ninfo = c.rrows = 1;
    c.nabs = nabs; c.nop = nop; c.ncoup = ncoup; c.nrhs = nrhs; c.nproj = nproj;
    c.l = l; c.w = w; c.cr = cr; c.cc = cc; c.ctr = ctr; c.z = z; c.WB = WB; c.GB = GB; c.ac = ac; c.B = B; c.P = P; c.X = X; c.R = R; c.info = info;
    int rc = resolvent_screen(p, c);
    if (rc) return rc;
    for (int q = 0; q < ncoup; ++q)
        if (cr[q] < 0 || cr[q] >= nch || cc[q] < 0 || cc[q] >= nch || ctr[q] < 0 || ctr[q] > 1) return BSP_ERR_ARG;
    const int n = p->hs.nfun, k = p->hs.k;
    const int max_band = wide ? resolvent_wide_max_band() : resolvent_coupled_max_band();
    if ((long long)nch * k - 1 > max_band) {
        fprintf(stderr, "bspatom_resolvent_coupled%s: half-width nch*k - 1 = %lld exceeds BSPATOM_COUPLED%s_MAX_BAND = %d\n",
                wide ? "_wide" : "", (long long)nch * k - 1, wide ? "_WIDE" : "", max_band);
        return BSP_ERR_UNSUPPORTED;
    }
    if ((long long)nch * n > 0x3fffffffLL) return BSP_ERR_ARG;
    c.len = (size_t)nch * n;
    c.ncoef = (size_t)2 * ncoup * nop;
    c.slot_doubles = wide ? resolvent_wide_slot_doubles(n, k, nch, nrhs) : resolvent_coupled_slot_doubles(n, k, nch);
    return resolvent_call(p, c, dev,
                          [&](int *slots) { return wide ? resolvent_wide_slots(k, nch, nmat, slots) : resolvent_coupled_slots(k, nch, nmat, slots); },
                          [&](int g, int slots, const ResolventPtrs &d, hipStream_t st) {
                              ResolventCoupledArgs a;
                              resolvent_fill(a, p, c, d);
                              a.nch = nch; a.nmat = g; a.ncoup = ncoup; a.nop = ncoup > 0 ? nop : 0;
                              a.cr = d.cr; a.cc = d.cc; a.ctr = d.ctr; a.GB = d.GB; a.acoef = d.acoef;
                              return wide ? launch_resolvent_wide(a, slots, st) : launch_resolvent_coupled(a, slots, st);
                          });
}

// bspatom_tdse_spline / _dev: nsteps Crank-Nicolson steps of nscan packets, each step the coupled matrix at z = 2i / dt with the
// step's coefficients.  The steps go out in launches of at most tdse_spline_group; the host variant stages the coefficients, the
// snapshots and the rows by groups of whole steps under tdse_stage_mb (one step at least); neither changes what a step computes.
// wide: the same arguments to tdse_spline_wide.hip, its limit, its slots, its scratch (one vector per slot) and its launch length.
static int tdse_spline_impl(bspatom_problem *p, int nscan, int nch, const int32_t *l, int nabs, const double *WB, const int32_t *w, int ncoup,
                            const int32_t *cr, const int32_t *cc, const int32_t *ctr, int nop, const double *GB, int nsteps, double dt,
                            const double *coef, double *c, int snap_every, double *snap, int obs_every, int nproj, const double *P,
                            double *obs, int32_t *info, bool dev, bool wide)
{
    if (!p || !l || !c || !info || nscan < 1 || nch < 1 || nsteps < 0 || nabs < 0 || nproj < 0 || (nabs > 0 && !WB)) return BSP_ERR_ARG;
    if (!std::isfinite(dt) || !(dt > 0.0)) return BSP_ERR_ARG;
    if (ncoup < 0 || (ncoup > 0 && (nop < 1 || !cr || !cc || !ctr || !GB || (nsteps > 0 && !coef)))) return BSP_ERR_ARG;
    if (snap_every < 0 || (snap && snap_every == 0)) return BSP_ERR_ARG;
    if (obs_every < 0 || (obs_every == 0) != (obs == nullptr) || (obs && nproj > 0 && !P)) return BSP_ERR_ARG;
    for (int ch = 0; ch < nch; ++ch) {
        if (p->band_nl < 1 || l[ch] < p->band_l0 || l[ch] >= p->band_l0 + p->band_nl) return BSP_ERR_ARG;
        if (w && (w[ch] < -1 || w[ch] >= nabs)) return BSP_ERR_ARG;
    }
    for (int q = 0; q < ncoup; ++q)
        if (cr[q] < 0 || cr[q] >= nch || cc[q] < 0 || cc[q] >= nch || ctr[q] < 0 || ctr[q] > 1) return BSP_ERR_ARG;
    const int n = p->hs.nfun, k = p->hs.k;
    const int max_band = wide ? resolvent_wide_max_band() : resolvent_coupled_max_band();
    if ((long long)nch * k - 1 > max_band) {
        fprintf(stderr, "bspatom_tdse_spline%s: half-width nch*k - 1 = %lld exceeds BSPATOM_COUPLED%s_MAX_BAND = %d\n", wide ? "_wide" : "",
                (long long)nch * k - 1, wide ? "_WIDE" : "", max_band);
        return BSP_ERR_UNSUPPORTED;
    }
    if ((long long)nch * n > 0x3fffffffLL || (long long)nsteps * nscan > 0x3fffffffLL) return BSP_ERR_ARG;
    const bool snapping = snap && snap_every > 0, observing = obs != nullptr;
    if (!observing) nproj = 0;
    const size_t N = (size_t)nch * n, wband = (size_t)(2 * k - 1) * n, RW = (size_t)nch + 2 * nproj;
    const size_t coef_step = (size_t)2 * nscan * ncoup * (ncoup > 0 ? nop : 0), snap_one = 2 * N * nscan, row_one = RW * nscan;   // doubles
    BSP_HIP(hipSetDevice(p->device));
    int rc, slots = 0;
    if ((rc = wide ? tdse_spline_wide_slots(k, nch, nscan, &slots) : tdse_spline_slots(k, nch, nscan, &slots))) return rc;
    if (opts().resolvent_slots > 0) slots = std::min(opts().resolvent_slots, nscan);
    const size_t slot_doubles = wide ? resolvent_wide_slot_doubles(n, k, nch, 1) : resolvent_coupled_slot_doubles(n, k, nch);
    const size_t rstage = opts().resolvent_stage_mb > 0 ? (size_t)opts().resolvent_stage_mb << 20 : RESOLVENT_STAGE_BYTES;
    slots = (int)std::max<size_t>(1, std::min<size_t>(slots, rstage / (slot_doubles * sizeof(double))));
    const int group = opts().tdse_spline_group > 0 ? opts().tdse_spline_group
                                                   : (wide ? spline_wide_group(nch * n, nch * k - 1, nscan, slots) : SPLINE_GROUP);
    auto launch = [&](const TdseSplineArgs &ta) { return wide ? launch_tdse_spline_wide(ta, slots, p->st) : launch_tdse_spline(ta, slots, p->st); };
    // the host variant's staging groups: whole steps, a step counted with a snapshot and a row of its own (an upper bound)
    int sgroup = std::max(nsteps, 1);
    if (!dev) {
        const size_t tstage = opts().tdse_stage_mb > 0 ? (size_t)opts().tdse_stage_mb << 20 : SPLINE_STAGE_BYTES;
        const size_t per_step = (coef_step + (snapping ? snap_one : 0) + (observing ? row_one : 0)) * sizeof(double);
        sgroup = (int)std::max<size_t>(1, std::min<size_t>(sgroup, tstage / std::max<size_t>(per_step, 1)));
    }
    const size_t gsnaps = snapping ? (size_t)sgroup / snap_every + 1 : 0, grows = observing ? (size_t)(sgroup - 1) / obs_every + 2 : 0;
    std::vector<int> chan(nch), wsel(nch, nabs > 0 && !w ? 0 : -1);
    std::vector<double> z(2 * (size_t)nch);
    const double zi = 2.0 / dt, g = 4.0 / dt;
    for (int ch = 0; ch < nch; ++ch) { chan[ch] = l[ch] - p->band_l0; if (w) wsel[ch] = w[ch]; z[2 * ch] = 0.0; z[2 * ch + 1] = zi; }
    const bool ops = ncoup > 0;
    DevArray<double> work, dz, dcoef, dWB, dGB, dc, dP, dsnap, dobs;
    DevArray<int> dchan, dw, dinfo, dcr, dcc, dctr;
    if ((rc = work.alloc((size_t)slots * slot_doubles)) || (rc = dz.put(z.data(), z.size())) || (rc = dchan.put(chan.data(), nch)) ||
        (rc = dw.put(wsel.data(), nch)) || (rc = dinfo.alloc(nscan)) ||
        (ops && ((rc = dcr.put(cr, ncoup)) || (rc = dcc.put(cc, ncoup)) || (rc = dctr.put(ctr, ncoup))))) return rc;
    if (!dev) {
        if ((nabs > 0 && (rc = dWB.put(WB, (size_t)nabs * wband))) || (ops && (rc = dGB.put(GB, (size_t)nop * wband))) ||
            (rc = dc.put(c, 2 * N * nscan)) || (nproj > 0 && (rc = dP.put(P, 2 * N * nproj))) ||
            (ops && nsteps > 0 && (rc = dcoef.alloc((size_t)sgroup * coef_step))) || (snapping && (rc = dsnap.alloc(gsnaps * snap_one))) ||
            (observing && (rc = dobs.alloc(grows * row_one)))) return rc;
    }
    BSP_HIP(hipMemsetAsync(dinfo.p, 0, (size_t)nscan * sizeof(int), p->st));
    TdseSplineArgs a = {};
    ResolventCoupledArgs &m = a.m;
    m.n = n; m.k = k; m.nch = nch; m.ncoup = ncoup; m.nop = ops ? nop : 0; m.nproj = nproj;
    m.SB = p->d_SB; m.HB = p->d_HB; m.chan = dchan.p; m.z = dz.p; m.w = dw.p;
    m.WB = nabs > 0 ? (dev ? WB : dWB.p) : nullptr;
    m.GB = ops ? (dev ? GB : dGB.p) : nullptr;
    m.cr = dcr.p; m.cc = dcc.p; m.ctr = dctr.p;
    m.P = nproj > 0 ? (dev ? P : dP.p) : nullptr;
    m.info = dinfo.p; m.work = work.p;
    a.nscan = nscan; a.g = g; a.c = dev ? c : dc.p;
    a.snap_every = snapping ? snap_every : 0; a.obs_every = observing ? obs_every : 0;
    const int nobs = observing ? (nsteps == 0 ? 1 : (nsteps - 1) / obs_every + 2) : 0;
    rc = BSP_OK;
    for (int n0 = 0; !rc && n0 < nsteps; n0 += sgroup) {
        const int n1 = std::min(nsteps, n0 + sgroup);
        // the group's snapshots s0 .. s1-1 and its rows j0 .. j1-1 (the observed steps j obs_every of n0 .. n1-1)
        const int s0 = snapping ? n0 / snap_every : 0, s1 = snapping ? n1 / snap_every : 0;
        const int j0 = observing ? (n0 + obs_every - 1) / obs_every : 0, j1 = observing ? (n1 + obs_every - 1) / obs_every : 0;
        const double *gcoef = nullptr;
        if (ops) {
            if (dev) gcoef = coef + (size_t)n0 * coef_step;
            else {
                rc = HIP_RC(hipMemcpyAsync(dcoef.p, coef + (size_t)n0 * coef_step, (size_t)(n1 - n0) * coef_step * sizeof(double), hipMemcpyHostToDevice, p->st));
                gcoef = dcoef.p;
            }
        }
        a.snap = snapping ? (dev ? snap : dsnap.p) : nullptr; a.s0 = dev ? 0 : s0;
        a.obs = observing ? (dev ? obs : dobs.p) : nullptr; a.j0 = dev ? 0 : j0;
        for (int m0 = n0; !rc && m0 < n1; m0 += group) {
            a.n0 = m0; a.nst = std::min(group, n1 - m0);
            m.acoef = ops ? gcoef + (size_t)(m0 - n0) * coef_step : nullptr;
            rc = launch(a);
        }
        if (!rc && !dev && s1 > s0)
            rc = HIP_RC(hipMemcpyAsync(snap + (size_t)s0 * snap_one, dsnap.p, (size_t)(s1 - s0) * snap_one * sizeof(double), hipMemcpyDeviceToHost, p->st));
        if (!rc && !dev && j1 > j0)
            rc = HIP_RC(hipMemcpyAsync(obs + (size_t)j0 * row_one, dobs.p, (size_t)(j1 - j0) * row_one * sizeof(double), hipMemcpyDeviceToHost, p->st));
        if (!rc && !dev) rc = HIP_RC(hipStreamSynchronize(p->st));     // the staging buffers are free for the next group
    }
    if (!rc && observing) {                                            // the row of the final packets: a launch that only measures
        a.n0 = nsteps; a.nst = 0; a.fin = 1; a.jfin = nobs - 1; a.snap = nullptr; m.acoef = nullptr;
        a.obs = dev ? obs : dobs.p; a.j0 = dev ? 0 : nobs - 1;
        rc = launch(a);
        if (!rc && !dev) rc = HIP_RC(hipMemcpyAsync(obs + (size_t)(nobs - 1) * row_one, dobs.p, row_one * sizeof(double), hipMemcpyDeviceToHost, p->st));
    }
    if (!rc && !dev) rc = HIP_RC(hipMemcpyAsync(c, dc.p, 2 * N * nscan * sizeof(double), hipMemcpyDeviceToHost, p->st));
    if (!rc) rc = HIP_RC(hipMemcpyAsync(info, dinfo.p, (size_t)nscan * sizeof(int), hipMemcpyDeviceToHost, p->st));
    return drain(p, rc);
}

extern "C" int bspatom_tdse_spline(bspatom_problem *p, int nscan, int nch, const int32_t *l, int nabs, const double *WB, const int32_t *w,
                                   int ncoup, const int32_t *cr, const int32_t *cc, const int32_t *ctr, int nop, const double *GB, int nsteps,
                                   double dt, const double *coef, double *c, int snap_every, double *snap, int obs_every, int nproj,
                                   const double *P, double *obs, int32_t *info)
{
    return tdse_spline_impl(p, nscan, nch, l, nabs, WB, w, ncoup, cr, cc, ctr, nop, GB, nsteps, dt, coef, c, snap_every, snap, obs_every, nproj,
                            P, obs, info, false, false);
}
extern "C" int bspatom_tdse_spline_dev(bspatom_problem *p, int nscan, int nch, const int32_t *l, int nabs, const double *WB_dev,
                                       const int32_t *w, int ncoup, const int32_t *cr, const int32_t *cc, const int32_t *ctr, int nop,
                                       const double *GB_dev, int nsteps, double dt, const double *coef_dev, double *c_dev, int snap_every,
                                       double *snap_dev, int obs_every, int nproj, const double *P_dev, double *obs_dev, int32_t *info)
{
    return tdse_spline_impl(p, nscan, nch, l, nabs, WB_dev, w, ncoup, cr, cc, ctr, nop, GB_dev, nsteps, dt, coef_dev, c_dev, snap_every,
                            snap_dev, obs_every, nproj, P_dev, obs_dev, info, true, false);
}
extern "C" int bspatom_tdse_spline_wide(bspatom_problem *p, int nscan, int nch, const int32_t *l, int nabs, const double *WB, const int32_t *w,
                                        int ncoup, const int32_t *cr, const int32_t *cc, const int32_t *ctr, int nop, const double *GB,
                                        int nsteps, double dt, const double *coef, double *c, int snap_every, double *snap, int obs_every,
                                        int nproj, const double *P, double *obs, int32_t *info)
{
    return tdse_spline_impl(p, nscan, nch, l, nabs, WB, w, ncoup, cr, cc, ctr, nop, GB, nsteps, dt, coef, c, snap_every, snap, obs_every, nproj,
                            P, obs, info, false, true);
}
extern "C" int bspatom_tdse_spline_wide_dev(bspatom_problem *p, int nscan, int nch, const int32_t *l, int nabs, const double *WB_dev,
                                            const int32_t *w, int ncoup, const int32_t *cr, const int32_t *cc, const int32_t *ctr, int nop,
                                            const double *GB_dev, int nsteps, double dt, const double *coef_dev, double *c_dev,
                                            int snap_every, double *snap_dev, int obs_every, int nproj, const double *P_dev, double *obs_dev,
                                            int32_t *info)
{
    return tdse_spline_impl(p, nscan, nch, l, nabs, WB_dev, w, ncoup, cr, cc, ctr, nop, GB_dev, nsteps, dt, coef_dev, c_dev, snap_every,
                            snap_dev, obs_every, nproj, P_dev, obs_dev, info, true, true);
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
        if (opts().resolvent_slots > 0) slots = std::min(opts().resolvent_slots, items);
        const size_t slot_doubles = spline_expect_slot_doubles(n);
        const size_t rstage = opts().resolvent_stage_mb > 0 ? (size_t)opts().resolvent_stage_mb << 20 : RESOLVENT_STAGE_BYTES;
        slots = (int)std::max<size_t>(1, std::min<size_t>(slots, rstage / (slot_doubles * sizeof(double))));
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
static int spline_expect_impl(bspatom_problem *p, int nscan, int nch, int nexp, const double *B, const double *GE, const double *c, double *e,
                              bool dev)
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
extern "C" int bspatom_spline_expect(bspatom_problem *p, int nscan, int nch, int nexp, const double *B, const double *GE, const double *c,
                                     double *e)
{
    return spline_expect_impl(p, nscan, nch, nexp, B, GE, c, e, false);
}
extern "C" int bspatom_spline_expect_dev(bspatom_problem *p, int nscan, int nch, int nexp, const double *B, const double *GE_dev,
                                         const double *c_dev, double *e_dev)
{
    return spline_expect_impl(p, nscan, nch, nexp, B, GE_dev, c_dev, e_dev, true);
}

// bspatom_tdse_split / _dev: nsteps split Crank-Nicolson steps of nscan packets (tdse_split.hip).  A step is three launches over the
// nscan * nch one-wave systems -- atomic half step, field step, atomic half step -- on two packet buffers that alternate; the atomic
// matrices are factored once, one per distinct (l, w).  The launches of tdse_split_group steps are enqueued, then waited for; the host
// variant stages f, the snapshots and the rows by groups of whole steps under tdse_stage_mb (one step at least); neither changes what
// a step computes.  With nexp > 0 (bspatom_tdse_split_observe) a row is nch + 2 nproj + 2 nexp wide: on an observed step the measuring
// launches of spline_expect.hip run on the buffer the step's first atomic launch reads, in front of it; the kernels of tdse_split.hip
// write their rows at the width they know into a buffer of their own, and one launch per staging group puts the two side by side.
static int tdse_split_impl(bspatom_problem *p, int nscan, int nch, const int32_t *l, int nabs, const double *WB, const int32_t *w, const double *G,
                           const double *Q, const double *lam, int nsteps, double dt, const double *f, double *c, int snap_every, double *snap,
                           int obs_every, int nproj, const double *P, double *obs, int32_t *info, int nexp, const double *EB, const double *GE,
                           bool dev)
{
    if (!p || !l || !c || !info || nscan < 1 || nch < 1 || nsteps < 0 || nabs < 0 || nproj < 0 || (nabs > 0 && !WB)) return BSP_ERR_ARG;
    if (nexp < 0 || (nexp > 0 && (!EB || !GE))) return BSP_ERR_ARG;
    if (!std::isfinite(dt) || !(dt > 0.0)) return BSP_ERR_ARG;
    if (nsteps > 0 && (!G || !Q || !lam || !f)) return BSP_ERR_ARG;
    if (snap_every < 0 || (snap && snap_every == 0)) return BSP_ERR_ARG;
    if (obs_every < 0 || (obs_every == 0) != (obs == nullptr) || (obs && nproj > 0 && !P)) return BSP_ERR_ARG;
    for (int ch = 0; ch < nch; ++ch) {
        if (p->band_nl < 1 || l[ch] < p->band_l0 || l[ch] >= p->band_l0 + p->band_nl) return BSP_ERR_ARG;
        if (w && (w[ch] < -1 || w[ch] >= nabs)) return BSP_ERR_ARG;
    }
    const int n = p->hs.nfun, k = p->hs.k;
    if (k > tdse_split_max_k()) {
        fprintf(stderr, "bspatom_tdse_split: k = %d exceeds the one-wave window's limit k <= %d\n", k, tdse_split_max_k());
        return BSP_ERR_UNSUPPORTED;
    }
    if ((long long)nch * n > 0x3fffffffLL || (long long)nscan * nch > 0x3fffffffLL || (long long)nsteps * nscan > 0x3fffffffLL) return BSP_ERR_ARG;
    const bool snapping = snap && snap_every > 0, observing = obs != nullptr;
    if (!observing) { nproj = 0; nexp = 0; }
    const bool expecting = nexp > 0;
    const int items = nscan * nch;
    // RW0: the row as the kernels of tdse_split.hip write it; RW: the caller's row
    const size_t N = (size_t)nch * n, wband = (size_t)(2 * k - 1) * n, RW0 = (size_t)nch + 2 * nproj, RW = RW0 + 2 * (size_t)nexp;
    const size_t f_step = (size_t)2 * nscan, snap_one = 2 * N * nscan, row_one = RW * nscan, row0_one = RW0 * nscan,
                 e_one = (size_t)2 * nexp * nscan;   // doubles
    BSP_HIP(hipSetDevice(p->device));
    int rc, slots = 0;
    if ((rc = tdse_split_slots(k, items, &slots))) return rc;
    if (opts().resolvent_slots > 0) slots = std::min(opts().resolvent_slots, items);
    const size_t slot_doubles = tdse_split_slot_doubles(n, k), fac_doubles = tdse_split_factor_doubles(n, k);
    const size_t rstage = opts().resolvent_stage_mb > 0 ? (size_t)opts().resolvent_stage_mb << 20 : RESOLVENT_STAGE_BYTES;
    slots = (int)std::max<size_t>(1, std::min<size_t>(slots, rstage / (slot_doubles * sizeof(double))));
    const int group = opts().tdse_split_group > 0 ? opts().tdse_split_group : SPLINE_GROUP;
    // the host variant's staging groups: whole steps, a step counted with a snapshot and a row of its own (an upper bound)
    int sgroup = std::max(nsteps, 1);
    if (!dev) {
        const size_t tstage = opts().tdse_stage_mb > 0 ? (size_t)opts().tdse_stage_mb << 20 : SPLINE_STAGE_BYTES;
        const size_t per_step = (f_step + (snapping ? snap_one : 0) + (observing ? row_one : 0)) * sizeof(double);
        sgroup = (int)std::max<size_t>(1, std::min<size_t>(sgroup, tstage / per_step));
    }
    const size_t gsnaps = snapping ? (size_t)sgroup / snap_every + 1 : 0, grows = observing ? (size_t)(sgroup - 1) / obs_every + 2 : 0;
    // the channels, and the distinct (band, absorber) pairs among them in the order of their first appearance: one atomic matrix each
    std::vector<int> chan(nch), wsel(nch, nabs > 0 && !w ? 0 : -1), fac(nch), fchan, fw;
    for (int ch = 0; ch < nch; ++ch) {
        chan[ch] = l[ch] - p->band_l0;
        if (w) wsel[ch] = w[ch];
        size_t at = 0;
        while (at < fchan.size() && (fchan[at] != chan[ch] || fw[at] != wsel[ch])) ++at;
        if (at == fchan.size()) { fchan.push_back(chan[ch]); fw.push_back(wsel[ch]); }
        fac[ch] = (int)at;
    }
    const int nfac = (int)fchan.size();
    DevArray<double> work, fstore, buf0, buf1, dQ, dlam, dpart, dWB, dG, dP, df, dsnap, dobs;
    DevArray<double> drow0, dexp;
    DevArray<int> dfac, dfchan, dfw, dfinfo, dpinfo;
    ExpectPlan plan;
    if (expecting && ((rc = plan.init(p, nscan, nch, nexp, EB, GE, dev)) || (rc = drow0.alloc(grows * row0_one)) || (rc = dexp.alloc(grows * e_one))))
        return rc;
    if ((rc = work.alloc((size_t)slots * slot_doubles)) || (rc = fstore.alloc((size_t)nfac * fac_doubles)) || (rc = buf0.alloc(2 * N * nscan)) ||
        (rc = buf1.alloc(2 * N * nscan)) || (rc = dpart.alloc((size_t)2 * nscan * nproj * nch)) ||
        (rc = dfac.put(fac.data(), nch)) || (rc = dfchan.put(fchan.data(), nfac)) ||
        (rc = dfw.put(fw.data(), nfac)) || (rc = dfinfo.alloc(nfac)) || (rc = dpinfo.alloc(items)) ||
        (nsteps > 0 && ((rc = dQ.put(Q, (size_t)nch * nch)) || (rc = dlam.put(lam, nch))))) return rc;
    if (!dev) {
        if ((nabs > 0 && (rc = dWB.put(WB, (size_t)nabs * wband))) || (nsteps > 0 && (rc = dG.put(G, wband))) ||
            (nproj > 0 && (rc = dP.put(P, 2 * N * nproj))) || (nsteps > 0 && (rc = df.alloc((size_t)sgroup * f_step))) ||
            (snapping && (rc = dsnap.alloc(gsnaps * snap_one))) || (observing && (rc = dobs.alloc(grows * row_one)))) return rc;
    }
    BSP_HIP(hipMemsetAsync(dfinfo.p, 0, (size_t)nfac * sizeof(int), p->st));
    BSP_HIP(hipMemsetAsync(dpinfo.p, 0, (size_t)items * sizeof(int), p->st));
    BSP_HIP(hipMemcpyAsync(buf0.p, c, 2 * N * nscan * sizeof(double), dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, p->st));
    TdseSplitArgs a = {};
    a.n = n; a.k = k; a.nch = nch; a.nscan = nscan; a.nproj = nproj; a.nfac = nfac;
    a.SB = p->d_SB; a.HB = p->d_HB;
    a.WB = nabs > 0 ? (dev ? WB : dWB.p) : nullptr;
    a.GB = nsteps > 0 ? (dev ? G : dG.p) : nullptr;
    a.fac = dfac.p; a.fchan = dfchan.p; a.fw = dfw.p;
    a.Q = dQ.p; a.lam = dlam.p;
    a.P = nproj > 0 ? (dev ? P : dP.p) : nullptr;
    a.g = 8.0 / dt; a.zi = 4.0 / dt; a.h = 0.5 * dt;
    a.part = dpart.p; a.fstore = fstore.p; a.finfo = dfinfo.p; a.pinfo = dpinfo.p; a.work = work.p;
    double *buf[2] = {buf0.p, buf1.p};
    int cur = 0;                                                       // the buffer that holds the packets
    rc = nsteps > 0 ? launch_tdse_split(a, 0, slots, p->st) : BSP_OK;
    // one launch on the packets in buf[cur]; what = 1: an atomic half step, 2: the field step
    auto launch = [&](int what, int mix, int measure, const double *fq, double *row, double *sn) {
        a.mix = mix; a.measure = measure; a.f = fq; a.row = row; a.snap = sn;
        a.in = buf[cur]; a.out = buf[cur ^ 1];
        const int r = launch_tdse_split(a, what, slots, p->st);
        if (!r && !measure) cur ^= 1;
        return r;
    };
    const int nobs = observing ? (nsteps == 0 ? 1 : (nsteps - 1) / obs_every + 2) : 0;
    for (int n0 = 0; !rc && n0 < nsteps; n0 += sgroup) {
        const int n1 = std::min(nsteps, n0 + sgroup);
        // the group's snapshots s0 .. s1-1 and its rows j0 .. j1-1 (the observed steps j obs_every of n0 .. n1-1)
        const int s0 = snapping ? n0 / snap_every : 0, s1 = snapping ? n1 / snap_every : 0;
        const int j0 = observing ? (n0 + obs_every - 1) / obs_every : 0, j1 = observing ? (n1 + obs_every - 1) / obs_every : 0;
        const double *gf = dev ? f + (size_t)n0 * f_step : df.p;
        if (!dev) rc = HIP_RC(hipMemcpyAsync(df.p, f + (size_t)n0 * f_step, (size_t)(n1 - n0) * f_step * sizeof(double), hipMemcpyHostToDevice, p->st));
        // where the group's first snapshot and row go: the caller's arrays from their start (_dev), else the staging buffers
        double *gsnap = snapping ? (dev ? snap + (size_t)s0 * snap_one : dsnap.p) : nullptr;
        double *gobs = observing ? (dev ? obs + (size_t)j0 * row_one : dobs.p) : nullptr;
        for (int m = n0; !rc && m < n1; ++m) {
            const bool observed = observing && m % obs_every == 0;
            const size_t jr = observed ? (size_t)(m / obs_every - j0) : 0;          // the row's place in the group
            double *row = observed ? (expecting ? drow0.p + jr * row0_one : gobs + jr * row_one) : nullptr;
            double *sn = snapping && (m + 1) % snap_every == 0 ? gsnap + (size_t)((m + 1) / snap_every - 1 - s0) * snap_one : nullptr;
            if (row && expecting) rc = plan.measure(buf[cur], dexp.p + jr * e_one, p->st);
            if (!rc) rc = launch(1, 0, 0, nullptr, row, nullptr);
            if (!rc) rc = launch(2, 0, 0, gf + (size_t)(m - n0) * f_step, nproj > 0 ? row : nullptr, nullptr);
            if (!rc) rc = launch(1, 1, 0, nullptr, nullptr, sn);
            if (!rc && ((m + 1 - n0) % group == 0 || m + 1 == n1)) rc = HIP_RC(hipStreamSynchronize(p->st));
        }
        if (!rc && expecting && j1 > j0) rc = launch_spline_expect_rows(gobs, drow0.p, dexp.p, (int)RW0, nexp, (j1 - j0) * nscan, p->st);
        if (!rc && !dev && s1 > s0)
            rc = HIP_RC(hipMemcpyAsync(snap + (size_t)s0 * snap_one, dsnap.p, (size_t)(s1 - s0) * snap_one * sizeof(double), hipMemcpyDeviceToHost, p->st));
        if (!rc && !dev && j1 > j0)
            rc = HIP_RC(hipMemcpyAsync(obs + (size_t)j0 * row_one, dobs.p, (size_t)(j1 - j0) * row_one * sizeof(double), hipMemcpyDeviceToHost, p->st));
        if (!rc && !dev) rc = HIP_RC(hipStreamSynchronize(p->st));     // the staging buffers are free for the next group
    }
    if (!rc && observing) {                                            // the row of the final packets: launches that only measure
        double *wide = dev ? obs + (size_t)(nobs - 1) * row_one : dobs.p, *row = expecting ? drow0.p : wide;
        if (expecting) rc = plan.measure(buf[cur], dexp.p, p->st);
        if (!rc) rc = launch(1, 0, 1, nullptr, row, nullptr);
        if (!rc && nproj > 0) rc = launch(2, 0, 1, nullptr, row, nullptr);
        if (!rc && expecting) rc = launch_spline_expect_rows(wide, drow0.p, dexp.p, (int)RW0, nexp, nscan, p->st);
        if (!rc && !dev) rc = HIP_RC(hipMemcpyAsync(obs + (size_t)(nobs - 1) * row_one, dobs.p, row_one * sizeof(double), hipMemcpyDeviceToHost, p->st));
    }
    if (!rc && nsteps > 0)
        rc = HIP_RC(hipMemcpyAsync(c, buf[cur], 2 * N * nscan * sizeof(double), dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, p->st));
    std::vector<int> finfo(nfac), pinfo(items);
    if (!rc) rc = HIP_RC(hipMemcpyAsync(finfo.data(), dfinfo.p, (size_t)nfac * sizeof(int), hipMemcpyDeviceToHost, p->st));
    if (!rc) rc = HIP_RC(hipMemcpyAsync(pinfo.data(), dpinfo.p, (size_t)items * sizeof(int), hipMemcpyDeviceToHost, p->st));
    if ((rc = drain(p, rc))) return rc;
    int atomic = 0;
    for (int v : finfo) atomic += v;
    for (int q = 0; q < nscan; ++q) {
        int s = nsteps > 0 ? atomic : 0;
        for (int j = 0; j < nch; ++j) s += pinfo[(size_t)q * nch + j];
        info[q] = s;
    }
    return BSP_OK;
}

extern "C" int bspatom_tdse_split(bspatom_problem *p, int nscan, int nch, const int32_t *l, int nabs, const double *WB, const int32_t *w,
                                  const double *G, const double *Q, const double *lam, int nsteps, double dt, const double *f, double *c,
                                  int snap_every, double *snap, int obs_every, int nproj, const double *P, double *obs, int32_t *info)
{
    return tdse_split_impl(p, nscan, nch, l, nabs, WB, w, G, Q, lam, nsteps, dt, f, c, snap_every, snap, obs_every, nproj, P, obs, info, 0, nullptr, nullptr,
                           false);
}
extern "C" int bspatom_tdse_split_dev(bspatom_problem *p, int nscan, int nch, const int32_t *l, int nabs, const double *WB_dev,
                                      const int32_t *w, const double *G_dev, const double *Q, const double *lam, int nsteps, double dt,
                                      const double *f_dev, double *c_dev, int snap_every, double *snap_dev, int obs_every, int nproj,
                                      const double *P_dev, double *obs_dev, int32_t *info)
{
    return tdse_split_impl(p, nscan, nch, l, nabs, WB_dev, w, G_dev, Q, lam, nsteps, dt, f_dev, c_dev, snap_every, snap_dev, obs_every, nproj,
                           P_dev, obs_dev, info, 0, nullptr, nullptr, true);
}
extern "C" int bspatom_tdse_split_observe(bspatom_problem *p, int nscan, int nch, const int32_t *l, int nabs, const double *WB, const int32_t *w,
                                          const double *G, const double *Q, const double *lam, int nsteps, double dt, const double *f, double *c,
                                          int snap_every, double *snap, int obs_every, int nproj, const double *P, double *obs, int32_t *info,
                                          int nexp, const double *B, const double *GE)
{
    return tdse_split_impl(p, nscan, nch, l, nabs, WB, w, G, Q, lam, nsteps, dt, f, c, snap_every, snap, obs_every, nproj, P, obs, info, nexp, B,
                           GE, false);
}
extern "C" int bspatom_tdse_split_observe_dev(bspatom_problem *p, int nscan, int nch, const int32_t *l, int nabs, const double *WB_dev,
                                              const int32_t *w, const double *G_dev, const double *Q, const double *lam, int nsteps, double dt,
                                              const double *f_dev, double *c_dev, int snap_every, double *snap_dev, int obs_every, int nproj,
                                              const double *P_dev, double *obs_dev, int32_t *info, int nexp, const double *B,
                                              const double *GE_dev)
{
    return tdse_split_impl(p, nscan, nch, l, nabs, WB_dev, w, G_dev, Q, lam, nsteps, dt, f_dev, c_dev, snap_every, snap_dev, obs_every, nproj,
                           P_dev, obs_dev, info, nexp, B, GE_dev, true);
}

extern "C" int bspatom_resolvent_coupled(bspatom_problem *p, int nmat, int nch, const int32_t *l, const double *z, int nabs,
                                         const double *WB, const int32_t *w, int ncoup, const int32_t *cr, const int32_t *cc,
                                         const int32_t *ctr, int nop, const double *GB, const double *a, int nrhs, const double *B,
                                         int nproj, const double *P, double *X, double *R, int32_t *info)
{
    return resolvent_coupled_impl(p, nmat, nch, l, z, nabs, WB, w, ncoup, cr, cc, ctr, nop, GB, a, nrhs, B, nproj, P, X, R, info, false, false);
}
extern "C" int bspatom_resolvent_coupled_dev(bspatom_problem *p, int nmat, int nch, const int32_t *l, const double *z, int nabs,
                                             const double *WB_dev, const int32_t *w, int ncoup, const int32_t *cr, const int32_t *cc,
                                             const int32_t *ctr, int nop, const double *GB_dev, const double *a, int nrhs,
                                             const double *B_dev, int nproj, const double *P_dev, double *X_dev, double *R_dev,
                                             int32_t *info)
{
    return resolvent_coupled_impl(p, nmat, nch, l, z, nabs, WB_dev, w, ncoup, cr, cc, ctr, nop, GB_dev, a, nrhs, B_dev, nproj, P_dev,
                                  X_dev, R_dev, info, true, false);
}
extern "C" int bspatom_resolvent_coupled_wide(bspatom_problem *p, int nmat, int nch, const int32_t *l, const double *z, int nabs,
                                              const double *WB, const int32_t *w, int ncoup, const int32_t *cr, const int32_t *cc,
                                              const int32_t *ctr, int nop, const double *GB, const double *a, int nrhs, const double *B,
                                              int nproj, const double *P, double *X, double *R, int32_t *info)
{
    return resolvent_coupled_impl(p, nmat, nch, l, z, nabs, WB, w, ncoup, cr, cc, ctr, nop, GB, a, nrhs, B, nproj, P, X, R, info, false, true);
}
extern "C" int bspatom_resolvent_coupled_wide_dev(bspatom_problem *p, int nmat, int nch, const int32_t *l, const double *z, int nabs,
                                                  const double *WB_dev, const int32_t *w, int ncoup, const int32_t *cr, const int32_t *cc,
                                                  const int32_t *ctr, int nop, const double *GB_dev, const double *a, int nrhs,
                                                  const double *B_dev, int nproj, const double *P_dev, double *X_dev, double *R_dev,
                                                  int32_t *info)
{
    return resolvent_coupled_impl(p, nmat, nch, l, z, nabs, WB_dev, w, ncoup, cr, cc, ctr, nop, GB_dev, a, nrhs, B_dev, nproj, P_dev,
                                  X_dev, R_dev, info, true, true);
}

extern "C" int bspatom_resolvent_chain(bspatom_problem *p, int nchain, int nstage, const int32_t *l, const double *z, int nabs,
                                       const double *WB, const int32_t *w, int nop, const double *GB, const double *a, int nrhs,
                                       const double *B, int nproj, const double *P, double *X, double *R, int32_t *info)
{
    return resolvent_chain_impl(p, nchain, nstage, l, z, nabs, WB, w, nop, GB, a, nrhs, B, nproj, P, X, R, info, false);
}
extern "C" int bspatom_resolvent_chain_dev(bspatom_problem *p, int nchain, int nstage, const int32_t *l, const double *z, int nabs,
                                           const double *WB_dev, const int32_t *w, int nop, const double *GB_dev, const double *a,
                                           int nrhs, const double *B_dev, int nproj, const double *P_dev, double *X_dev, double *R_dev,
                                           int32_t *info)
{
    return resolvent_chain_impl(p, nchain, nstage, l, z, nabs, WB_dev, w, nop, GB_dev, a, nrhs, B_dev, nproj, P_dev, X_dev, R_dev, info, true);
}

extern "C" int bspatom_resolvent(bspatom_problem *p, int nmat, const int32_t *l, const double *z, int nabs, const double *WB,
                                 const int32_t *w, int nrhs, const double *B, int nproj, const double *P, double *X, double *R,
                                 int32_t *info)
{
    return resolvent_impl(p, nmat, l, z, nabs, WB, w, nrhs, B, nproj, P, X, R, info, false);
}
extern "C" int bspatom_resolvent_dev(bspatom_problem *p, int nmat, const int32_t *l, const double *z, int nabs, const double *WB_dev,
                                     const int32_t *w, int nrhs, const double *B_dev, int nproj, const double *P_dev, double *X_dev,
                                     double *R_dev, int32_t *info)
{
    return resolvent_impl(p, nmat, l, z, nabs, WB_dev, w, nrhs, B_dev, nproj, P_dev, X_dev, R_dev, info, true);
}
