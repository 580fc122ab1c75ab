// capi_resolvent.hip -- the resolvent entry points of include/bspatom.h: solves with the banded pencil at complex energies,
// (H_l - i W - z S) x = b.  The bands are those the problem holds on the device (the last bspatom_solve or bspatom_assemble); all
// work goes on the problem's stream and the scratch of a call is freed when it returns.
//   bspatom_resolvent / _dev: one channel per matrix, resolvent.hip's one-wave LU.
//   bspatom_resolvent_chain / _dev: chains of such solves with an operator in between, one launch for the whole batch.
//   bspatom_resolvent_coupled / _dev: several channels coupled to all orders in one banded LU (resolvent_coupled.hip).
//   bspatom_resolvent_coupled_wide / _dev: the same call on the blocked LU for wide bands (resolvent_wide.hip).
// All eight run through resolvent_call: a front function per flavour screens what is particular to it, describes the call by counts per
// ITEM (a matrix, a chain, a coupled matrix) and hands over its slot query and its launcher.  (The time steps on the same LUs are
// capi_spline.hip's.)
#include "capi_internal.h"

using namespace bsp;

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
    return screen_channels(p, c.l, c.w, c.items * c.rec, c.nabs);
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
    const size_t wband = (size_t)(2 * k - 1) * n;
    BSP_HIP(hipSetDevice(p->device));
    int rc;
    // the work slots: what is resident, within the scratch bound, one at least
    int slots = 0;
    if ((rc = query(&slots))) return rc;
    slots = bounded_slots(slots, c.items, c.slot_doubles);
    // the host variant's groups: the X of one group within the bound, one item at least
    const size_t x_item = (size_t)2 * c.nrhs * c.len, r_item = (size_t)2 * c.rrows * c.nrhs * c.nproj;   // doubles of one item's X, R
    int group = c.items;
    if (!dev && c.X) group = (int)std::max<size_t>(1, std::min<size_t>(c.items, resolvent_stage_bytes() / (x_item * sizeof(double))));
    std::vector<int> chan, wsel;
    select_channels(p, c.l, c.w, nrec, c.nabs, chan, wsel);
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
    if (!rc) rc = screen_couplings(nch, ncoup, cr, cc, ctr);
    if (rc) return rc;
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
