// capi_resolvent.hip -- bspatom_resolvent / bspatom_resolvent_dev (include/bspatom.h): solves with the banded pencil at complex
// energies, (H_l - i W - z S) x = b, by resolvent.hip's one-wave LU.  The bands are those the problem holds on the device (the
// last bspatom_solve or bspatom_assemble); all work goes on the problem's stream and the scratch of a call is freed when it returns.
// bspatom_resolvent_chain / _dev: chains of such solves with an operator in between, one launch for the whole batch.
// bspatom_resolvent_coupled / _dev: several channels coupled to all orders in one banded LU (resolvent_coupled.hip).
// bspatom_resolvent_coupled_wide / _dev: the same call on the blocked LU for wide bands (resolvent_wide.hip).
#include <algorithm>
#include "capi_internal.h"

using namespace bsp;

static constexpr size_t RESOLVENT_STAGE_BYTES = (size_t)2048 << 20;

static int resolvent_impl(bspatom_problem *p, int nmat, const int32_t *l, const double *z, int nabs, const double *WB, const int32_t *w,
                          int nrhs, const double *B, int nproj, const double *P, double *X, double *R, int32_t *info, bool dev)
{
    if (!p || !l || !z || !B || !info || (!X && !R)) return BSP_ERR_ARG;
    if (nmat < 1 || nrhs < 1 || nabs < 0 || nproj < 0 || (nabs > 0 && !WB)) return BSP_ERR_ARG;
    if (R && (!P || nproj < 1)) return BSP_ERR_ARG;
    if (!WB) nabs = 0;
    for (int m = 0; m < nmat; ++m) {
        if (p->band_nl < 1 || l[m] < p->band_l0 || l[m] >= p->band_l0 + p->band_nl) return BSP_ERR_ARG;
        if (w && (w[m] < -1 || w[m] >= nabs)) return BSP_ERR_ARG;
    }
    const HostSetup &h = p->hs;
    const int n = h.nfun, k = h.k;
    const size_t wband = (size_t)(2 * k - 1) * n, stage = opts().resolvent_stage_mb > 0 ? (size_t)opts().resolvent_stage_mb << 20 : RESOLVENT_STAGE_BYTES;
    BSP_HIP(hipSetDevice(p->device));
    int rc;
    // the work slots: what is resident, within the scratch bound, one at least
    int slots = 0;
    if ((rc = resolvent_slots(k, nmat, &slots))) return rc;
    if (opts().resolvent_slots > 0) slots = std::min(opts().resolvent_slots, nmat);
    const size_t slot_bytes = resolvent_slot_doubles(n, k) * sizeof(double);
    slots = (int)std::max<size_t>(1, std::min<size_t>(slots, stage / slot_bytes));
    // the host variant's groups: the X of one group within the bound, one matrix at least
    const size_t x_mat = (size_t)2 * nrhs * n;                       // doubles of one matrix's X
    int group = nmat;
    if (!dev && X) group = (int)std::max<size_t>(1, std::min<size_t>(nmat, stage / (x_mat * sizeof(double))));
    std::vector<int> chan(nmat), wsel(nmat, nabs > 0 && !w ? 0 : -1);
    for (int m = 0; m < nmat; ++m) { chan[m] = l[m] - p->band_l0; if (w) wsel[m] = w[m]; }
    DevArray<double> work, dz, dWB, dB, dP, dX, dR;
    DevArray<int> dchan, dw, dinfo;
    if ((rc = work.alloc((size_t)slots * resolvent_slot_doubles(n, k))) || (rc = dz.put(z, (size_t)2 * nmat)) ||
        (rc = dchan.put(chan.data(), nmat)) || (rc = dw.put(wsel.data(), nmat)) || (rc = dinfo.alloc(nmat))) return rc;
    const size_t r_all = (size_t)2 * nmat * nrhs * nproj;
    if (!dev) {
        if ((nabs > 0 && (rc = dWB.put(WB, (size_t)nabs * wband))) || (rc = dB.put(B, (size_t)2 * nrhs * n)) ||
            (R && (rc = dP.put(P, (size_t)2 * nproj * n))) || (X && (rc = dX.alloc((size_t)group * x_mat))) || (R && (rc = dR.alloc(r_all))))
            return rc;
    }
    ResolventArgs a;
    a.n = n; a.k = k; a.nrhs = nrhs; a.nproj = R ? nproj : 0;
    a.SB = p->d_SB; a.HB = p->d_HB;
    a.WB = nabs > 0 ? (dev ? WB : dWB.p) : nullptr;
    a.B = dev ? B : dB.p;
    a.P = R ? (dev ? P : dP.p) : nullptr;
    a.work = work.p;
    rc = BSP_OK;
    for (int m0 = 0; !rc && m0 < nmat; m0 += group) {
        const int g = std::min(group, nmat - m0);
        a.nmat = g;
        a.chan = dchan.p + m0; a.z = dz.p + (size_t)2 * m0; a.w = dw.p + m0; a.info = dinfo.p + m0;
        a.X = X ? (dev ? X + (size_t)m0 * x_mat : dX.p) : nullptr;
        a.R = R ? (dev ? R : dR.p) + (size_t)2 * m0 * nrhs * nproj : nullptr;
        rc = launch_resolvent(a, std::min(slots, g), p->st);
        if (!rc && !dev && X) rc = HIP_RC(hipMemcpyAsync(X + (size_t)m0 * x_mat, dX.p, (size_t)g * x_mat * sizeof(double), hipMemcpyDeviceToHost, p->st));
    }
    if (!rc && !dev && R) rc = HIP_RC(hipMemcpyAsync(R, dR.p, r_all * sizeof(double), hipMemcpyDeviceToHost, p->st));
    if (!rc) rc = HIP_RC(hipMemcpyAsync(info, dinfo.p, (size_t)nmat * sizeof(int), hipMemcpyDeviceToHost, p->st));
    return drain(p, rc);
}

// bspatom_resolvent_chain / _dev: the same plumbing with nchain * nstage matrices, the operator bands and their coefficients beside
// them, the slots sized by resolvent_chain_kernel (its scratch holds nrhs more vectors), the groups made of whole chains.
static int resolvent_chain_impl(bspatom_problem *p, int nchain, int nstage, const int32_t *l, const double *z, int nabs, const double *WB,
                                const int32_t *w, int nop, const double *GB, const double *ac, int nrhs, const double *B, int nproj,
                                const double *P, double *X, double *R, int32_t *info, bool dev)
{
    if (!p || !l || !z || !B || !info || (!X && !R)) return BSP_ERR_ARG;
    if (nchain < 1 || nstage < 1 || nrhs < 1 || nabs < 0 || nproj < 0 || nop < 0 || (nabs > 0 && !WB)) return BSP_ERR_ARG;
    if (R && (!P || nproj < 1)) return BSP_ERR_ARG;
    if (nstage > 1 && (nop < 1 || !GB || !ac)) return BSP_ERR_ARG;
    if ((long long)nchain * nstage > 0x3fffffffLL) return BSP_ERR_ARG;
    if (!WB) nabs = 0;
    const int nmat = nchain * nstage;
    for (int m = 0; m < nmat; ++m) {
        if (p->band_nl < 1 || l[m] < p->band_l0 || l[m] >= p->band_l0 + p->band_nl) return BSP_ERR_ARG;
        if (w && (w[m] < -1 || w[m] >= nabs)) return BSP_ERR_ARG;
    }
    const HostSetup &h = p->hs;
    const int n = h.nfun, k = h.k;
    const size_t wband = (size_t)(2 * k - 1) * n, stage = opts().resolvent_stage_mb > 0 ? (size_t)opts().resolvent_stage_mb << 20 : RESOLVENT_STAGE_BYTES;
    BSP_HIP(hipSetDevice(p->device));
    int rc;
    int slots = 0;
    if ((rc = resolvent_chain_slots(k, nchain, &slots))) return rc;
    if (opts().resolvent_slots > 0) slots = std::min(opts().resolvent_slots, nchain);
    const size_t slot_doubles = resolvent_chain_slot_doubles(n, k, nrhs);
    slots = (int)std::max<size_t>(1, std::min<size_t>(slots, stage / (slot_doubles * sizeof(double))));
    // the host variant's groups: the X of one group of chains within the bound, one chain at least
    const size_t x_chain = (size_t)2 * nrhs * n;                     // doubles of one chain's X
    int group = nchain;
    if (!dev && X) group = (int)std::max<size_t>(1, std::min<size_t>(nchain, stage / (x_chain * sizeof(double))));
    std::vector<int> chan(nmat), wsel(nmat, nabs > 0 && !w ? 0 : -1);
    for (int m = 0; m < nmat; ++m) { chan[m] = l[m] - p->band_l0; if (w) wsel[m] = w[m]; }
    const bool ops = nstage > 1;
    DevArray<double> work, dz, dac, dWB, dGB, dB, dP, dX, dR;
    DevArray<int> dchan, dw, dinfo;
    if ((rc = work.alloc((size_t)slots * slot_doubles)) || (rc = dz.put(z, (size_t)2 * nmat)) ||
        (ops && (rc = dac.put(ac, (size_t)nchain * (nstage - 1) * nop))) ||
        (rc = dchan.put(chan.data(), nmat)) || (rc = dw.put(wsel.data(), nmat)) || (rc = dinfo.alloc(nmat))) return rc;
    const size_t r_chain = (size_t)2 * nstage * nrhs * nproj, r_all = r_chain * nchain;
    if (!dev) {
        if ((nabs > 0 && (rc = dWB.put(WB, (size_t)nabs * wband))) || (ops && (rc = dGB.put(GB, (size_t)nop * wband))) ||
            (rc = dB.put(B, (size_t)2 * nrhs * n)) || (R && (rc = dP.put(P, (size_t)2 * nproj * n))) ||
            (X && (rc = dX.alloc((size_t)group * x_chain))) || (R && (rc = dR.alloc(r_all))))
            return rc;
    }
    ResolventChainArgs a;
    a.n = n; a.k = k; a.nstage = nstage; a.nop = ops ? nop : 0; a.nrhs = nrhs; a.nproj = R ? nproj : 0;
    a.SB = p->d_SB; a.HB = p->d_HB;
    a.WB = nabs > 0 ? (dev ? WB : dWB.p) : nullptr;
    a.GB = ops ? (dev ? GB : dGB.p) : nullptr;
    a.B = dev ? B : dB.p;
    a.P = R ? (dev ? P : dP.p) : nullptr;
    a.work = work.p;
    rc = BSP_OK;
    for (int c0 = 0; !rc && c0 < nchain; c0 += group) {
        const int g = std::min(group, nchain - c0);
        const size_t m0 = (size_t)c0 * nstage;
        a.nchain = g;
        a.chan = dchan.p + m0; a.z = dz.p + 2 * m0; a.w = dw.p + m0; a.info = dinfo.p + m0;
        a.acoef = ops ? dac.p + (size_t)c0 * (nstage - 1) * nop : nullptr;
        a.X = X ? (dev ? X + (size_t)c0 * x_chain : dX.p) : nullptr;
        a.R = R ? (dev ? R : dR.p) + (size_t)c0 * r_chain : nullptr;
        rc = launch_resolvent_chain(a, std::min(slots, g), p->st);
        if (!rc && !dev && X) rc = HIP_RC(hipMemcpyAsync(X + (size_t)c0 * x_chain, dX.p, (size_t)g * x_chain * sizeof(double), hipMemcpyDeviceToHost, p->st));
    }
    if (!rc && !dev && R) rc = HIP_RC(hipMemcpyAsync(R, dR.p, r_all * sizeof(double), hipMemcpyDeviceToHost, p->st));
    if (!rc) rc = HIP_RC(hipMemcpyAsync(info, dinfo.p, (size_t)nmat * sizeof(int), hipMemcpyDeviceToHost, p->st));
    return drain(p, rc);
}

// bspatom_resolvent_coupled / _dev: nmat matrices of nch coupled channels each, one workgroup per matrix (resolvent_coupled.hip); the
// plumbing of resolvent_impl with nmat * nch channel records, the coupling topology and its complex coefficients beside them.
// wide: the same arguments to resolvent_wide.hip, its limit, its slots and its scratch.
static int resolvent_coupled_impl(bspatom_problem *p, int nmat, int nch, const int32_t *l, const double *z, int nabs, const double *WB,
                                  const int32_t *w, int ncoup, const int32_t *cr, const int32_t *cc, const int32_t *ctr, int nop,
                                  const double *GB, const double *ac, int nrhs, const double *B, int nproj, const double *P, double *X,
                                  double *R, int32_t *info, bool dev, bool wide)
{
    if (!p || !l || !z || !B || !info || (!X && !R)) return BSP_ERR_ARG;
    if (nmat < 1 || nch < 1 || nrhs < 1 || nabs < 0 || nproj < 0 || ncoup < 0 || (nabs > 0 && !WB)) return BSP_ERR_ARG;
    if (R && (!P || nproj < 1)) return BSP_ERR_ARG;
    if (ncoup > 0 && (nop < 1 || !cr || !cc || !ctr || !GB || !ac)) return BSP_ERR_ARG;
    if ((long long)nmat * nch > 0x3fffffffLL) return BSP_ERR_ARG;
    if (!WB) nabs = 0;
    const int nrec = nmat * nch;
    for (int m = 0; m < nrec; ++m) {
        if (p->band_nl < 1 || l[m] < p->band_l0 || l[m] >= p->band_l0 + p->band_nl) return BSP_ERR_ARG;
        if (w && (w[m] < -1 || w[m] >= nabs)) return BSP_ERR_ARG;
    }
    for (int q = 0; q < ncoup; ++q)
        if (cr[q] < 0 || cr[q] >= nch || cc[q] < 0 || cc[q] >= nch || ctr[q] < 0 || ctr[q] > 1) return BSP_ERR_ARG;
    const HostSetup &h = p->hs;
    const int n = h.nfun, k = h.k;
    const int max_band = wide ? resolvent_wide_max_band() : resolvent_coupled_max_band();
    if ((long long)nch * k - 1 > max_band) {
        fprintf(stderr, "bspatom_resolvent_coupled%s: half-width nch*k - 1 = %lld exceeds BSPATOM_COUPLED%s_MAX_BAND = %d\n",
                wide ? "_wide" : "", (long long)nch * k - 1, wide ? "_WIDE" : "", max_band);
        return BSP_ERR_UNSUPPORTED;
    }
    if ((long long)nch * n > 0x3fffffffLL) return BSP_ERR_ARG;
    const size_t N = (size_t)nch * n;
    const size_t wband = (size_t)(2 * k - 1) * n, stage = opts().resolvent_stage_mb > 0 ? (size_t)opts().resolvent_stage_mb << 20 : RESOLVENT_STAGE_BYTES;
    BSP_HIP(hipSetDevice(p->device));
    int rc;
    int slots = 0;
    if ((rc = wide ? resolvent_wide_slots(k, nch, nmat, &slots) : resolvent_coupled_slots(k, nch, nmat, &slots))) return rc;
    if (opts().resolvent_slots > 0) slots = std::min(opts().resolvent_slots, nmat);
    const size_t slot_doubles = wide ? resolvent_wide_slot_doubles(n, k, nch, nrhs) : resolvent_coupled_slot_doubles(n, k, nch);
    slots = (int)std::max<size_t>(1, std::min<size_t>(slots, stage / (slot_doubles * sizeof(double))));
    // the host variant's groups: the X of one group within the bound, one matrix at least
    const size_t x_mat = (size_t)2 * nrhs * N;                       // doubles of one matrix's X
    int group = nmat;
    if (!dev && X) group = (int)std::max<size_t>(1, std::min<size_t>(nmat, stage / (x_mat * sizeof(double))));
    std::vector<int> chan(nrec), wsel(nrec, nabs > 0 && !w ? 0 : -1);
    for (int m = 0; m < nrec; ++m) { chan[m] = l[m] - p->band_l0; if (w) wsel[m] = w[m]; }
    const bool ops = ncoup > 0;
    DevArray<double> work, dz, dac, dWB, dGB, dB, dP, dX, dR;
    DevArray<int> dchan, dw, dinfo, dcr, dcc, dctr;
    if ((rc = work.alloc((size_t)slots * slot_doubles)) || (rc = dz.put(z, (size_t)2 * nrec)) ||
        (ops && ((rc = dac.put(ac, (size_t)2 * nmat * ncoup * nop)) || (rc = dcr.put(cr, ncoup)) || (rc = dcc.put(cc, ncoup)) ||
                 (rc = dctr.put(ctr, ncoup)))) ||
        (rc = dchan.put(chan.data(), nrec)) || (rc = dw.put(wsel.data(), nrec)) || (rc = dinfo.alloc(nmat))) return rc;
    const size_t r_all = (size_t)2 * nmat * nrhs * nproj;
    if (!dev) {
        if ((nabs > 0 && (rc = dWB.put(WB, (size_t)nabs * wband))) || (ops && (rc = dGB.put(GB, (size_t)nop * wband))) ||
            (rc = dB.put(B, (size_t)2 * nrhs * N)) || (R && (rc = dP.put(P, (size_t)2 * nproj * N))) ||
            (X && (rc = dX.alloc((size_t)group * x_mat))) || (R && (rc = dR.alloc(r_all))))
            return rc;
    }
    ResolventCoupledArgs a;
    a.n = n; a.k = k; a.nch = nch; a.nrhs = nrhs; a.nproj = R ? nproj : 0; a.ncoup = ncoup; a.nop = ops ? nop : 0;
    a.SB = p->d_SB; a.HB = p->d_HB;
    a.WB = nabs > 0 ? (dev ? WB : dWB.p) : nullptr;
    a.cr = ops ? dcr.p : nullptr; a.cc = ops ? dcc.p : nullptr; a.ctr = ops ? dctr.p : nullptr;
    a.GB = ops ? (dev ? GB : dGB.p) : nullptr;
    a.B = dev ? B : dB.p;
    a.P = R ? (dev ? P : dP.p) : nullptr;
    a.work = work.p;
    rc = BSP_OK;
    for (int m0 = 0; !rc && m0 < nmat; m0 += group) {
        const int g = std::min(group, nmat - m0);
        a.nmat = g;
        a.chan = dchan.p + (size_t)m0 * nch; a.z = dz.p + (size_t)2 * m0 * nch; a.w = dw.p + (size_t)m0 * nch; a.info = dinfo.p + m0;
        a.acoef = ops ? dac.p + (size_t)2 * m0 * ncoup * nop : nullptr;
        a.X = X ? (dev ? X + (size_t)m0 * x_mat : dX.p) : nullptr;
        a.R = R ? (dev ? R : dR.p) + (size_t)2 * m0 * nrhs * nproj : nullptr;
        rc = wide ? launch_resolvent_wide(a, std::min(slots, g), p->st) : launch_resolvent_coupled(a, std::min(slots, g), p->st);
        if (!rc && !dev && X) rc = HIP_RC(hipMemcpyAsync(X + (size_t)m0 * x_mat, dX.p, (size_t)g * x_mat * sizeof(double), hipMemcpyDeviceToHost, p->st));
    }
    if (!rc && !dev && R) rc = HIP_RC(hipMemcpyAsync(R, dR.p, r_all * sizeof(double), hipMemcpyDeviceToHost, p->st));
    if (!rc) rc = HIP_RC(hipMemcpyAsync(info, dinfo.p, (size_t)nmat * sizeof(int), hipMemcpyDeviceToHost, p->st));
    return drain(p, rc);
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
