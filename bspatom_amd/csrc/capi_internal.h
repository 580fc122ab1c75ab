// capi_internal.h -- what the translation units of the C ABI share (capi.hip: handle, options, solve; capi_states.hip: the
// consumers of the last solve; capi_stage.hip: the stage-level entry points).  Private to csrc.
#pragma once
#include <algorithm>
#include <cstring>
#include <vector>
#include "common.h"
#include "host_setup.h"
#include "../../include/bspatom.h"

struct bspatom_problem {
    bsp::HostSetup hs;
    int device, npad;
    hipStream_t st = nullptr;
    bsp::LaunchCtx lc;                        // what the launchers of a solve own besides the buffers below (common.h)
    // device: set-up tables
    double *d_rt = nullptr, *d_aind = nullptr, *d_xg = nullptr, *d_wg = nullptr, *d_vpot = nullptr, *d_bl = nullptr;
    double *d_ptab = nullptr; int *d_left = nullptr; int *d_status = nullptr;
    bool ptab_ready = false;
    // device: per-solve buffers (sized for cap_nl channels)
    int cap_nl = 0;
    double *d_SB = nullptr, *d_HB = nullptr, *d_UB = nullptr, *d_rdiag = nullptr;
    double *d_Y = nullptr, *d_C = nullptr, *d_AB = nullptr, *d_d = nullptr, *d_e = nullptr, *d_E = nullptr;
    void *d_work = nullptr, *d_sbctl = nullptr;
    void *d_cwork = nullptr;         // band route (crawford.hip)
    int cap_dense = 0, cap_band = 0; // channels the dense buffers (Y, C, work) / the band route's work area are sized for
    int *d_info = nullptr;
    // eigenvector / wave-function scratch
    double *d_vwork = nullptr, *d_vec = nullptr, *d_wfr = nullptr, *d_wfu = nullptr, *d_Esel = nullptr;
    int *d_chan = nullptr;
    int wf_cap = 0;
    // the eigenvector the reference consumes, Hij(:, n0_ini) of channel l_ini (matrices.f90:267), computed on a side
    // stream while the batched bisection runs; bspatom_eigvec returns it when asked for exactly that state
    hipStream_t st2 = nullptr;
    hipEvent_t evx = nullptr;
    hipStream_t stS = nullptr;                // band route: the S-only part of the reduction beside the assembly of the H_l
    hipEvent_t evS = nullptr, evC[bsp::CW_CHUNKS] = {};
    bool pre_early = false, pre_early_ok = false;   // the prefetched vector's eigenvalue came from the pencil (bandsect.hip); it passed the check
    double *d_pvec = nullptr, *d_pE = nullptr;
    int *d_pinfo = nullptr;
    int pre_l = -1, pre_n0 = -1, pre_ch = 0;
    // last solve
    int last_l0 = 0, last_nl = 0;
    int band_l0 = 0, band_nl = 0;             // channels whose bands d_HB holds (the last bspatom_solve or bspatom_assemble): bspatom_resolvent's
    hipEvent_t ev[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    double ms[6] = {0, 0, 0, 0, 0, 0};
};

namespace bsp {
inline int round_up(int x, int m) { return (x + m - 1) / m * m; }

// BSP_HIP as an expression: BSP_OK, or BSP_ERR_HIP with the error printed
#define HIP_RC(x) ([&]() -> int { BSP_HIP(x); return BSP_OK; }())

// n elements of device memory (one at least), freed when the owner leaves its scope: what was enqueued on them must be complete
// by then (drain / finish below)
template <class T>
class DevArray {
public:
    T *p = nullptr;
    DevArray() = default;
    DevArray(const DevArray &) = delete;
    ~DevArray() { hipFree(p); }
    int alloc(size_t n) { BSP_HIP(hipMalloc(reinterpret_cast<void **>(&p), (n ? n : 1) * sizeof(T))); return BSP_OK; }
    int put(const T *h, size_t n) { const int rc = alloc(n); return rc ? rc : HIP_RC(hipMemcpy(p, h, n * sizeof(T), hipMemcpyHostToDevice)); }
    int get(T *h, size_t n) const { return HIP_RC(hipMemcpy(h, p, n * sizeof(T), hipMemcpyDeviceToHost)); }
};

// the point table of the problem's grid (assemble.hip), run on the problem's stream the first time something needs it
inline int ensure_point_table(bspatom_problem *p)
{
    if (p->ptab_ready) return BSP_OK;
    const HostSetup &h = p->hs;
    const int rc = launch_point_table(h.nkp, h.k, h.ka, h.nfun, p->d_rt, p->d_aind, p->d_xg, p->d_wg, p->d_vpot, p->d_ptab, p->d_left,
                                      p->d_status, p->st);
    if (!rc) p->ptab_ready = true;
    return rc;
}

// the kernels' status word (common.h): BSP_OK or the error one of them left
inline int check_status(bspatom_problem *p)
{
    int st = 0;
    BSP_HIP(hipMemcpy(&st, p->d_status, sizeof(int), hipMemcpyDeviceToHost));
    return st;
}

// d_info after inverse iterations: 1 + index of a vector whose iterate had norm zero (eigvec.hip), else 0
inline int invit_failed(bspatom_problem *p)
{
    int v = 0;
    BSP_HIP(hipMemcpy(&v, p->d_info, sizeof(int), hipMemcpyDeviceToHost));
    return v ? BSP_ERR_UNSUPPORTED : BSP_OK;
}

// states n0 .. n0+count-1 (from 1) of channels l0 .. l0+nl-1: BSP_OK if the last solve holds them all, else BSP_ERR_ARG
inline int last_solve_window(const bspatom_problem *p, int l0, int nl, int n0, int count)
{
    return nl >= 1 && count >= 1 && n0 >= 1 && (long)n0 + count - 1 <= p->hs.nfun && l0 >= p->last_l0 &&
           (long)l0 + nl <= (long)p->last_l0 + p->last_nl ? BSP_OK : BSP_ERR_ARG;
}

// The tail of an entry point that enqueued work on p->st, called while its DevArrays are alive: EVERY path waits for the stream
// before the scratch is freed and before the call returns.  rc, the first error of the call so far, comes before the wait's own.
inline int drain(bspatom_problem *p, int rc)
{
    const hipError_t es = hipStreamSynchronize(p->st);
    return rc ? rc : HIP_RC(es);
}

// drain, then whether an inverse iteration of the call broke down
inline int finish(bspatom_problem *p, int rc) { return (rc = drain(p, rc)) ? rc : invit_failed(p); }

int ensure_vec_scratch(bspatom_problem *p);     // capi.hip: d_vwork, d_vec, d_chan, d_Esel for one vector

// The bounds of a call's device scratch (capi_resolvent.hip, capi_spline.hip, capi_tdse.hip): resolvent_stage_mb for the work slots and a
// group's X, tdse_stage_mb for what a stepped run's host variant stages (the table, the snapshots and the rows of one group of steps)
inline size_t resolvent_stage_bytes() { return (size_t)(opts().resolvent_stage_mb > 0 ? opts().resolvent_stage_mb : 2048) << 20; }
inline size_t tdse_stage_bytes() { return (size_t)(opts().tdse_stage_mb > 0 ? opts().tdse_stage_mb : 256) << 20; }

// the work slots of a call: what the kernel's occupancy query gave, or resolvent_slots (the items at most), within the bound, one at least
inline int bounded_slots(int queried, int items, size_t slot_doubles)
{
    if (opts().resolvent_slots > 0) queried = std::min(opts().resolvent_slots, items);
    return (int)std::max<size_t>(1, std::min<size_t>(queried, resolvent_stage_bytes() / (slot_doubles * sizeof(double))));
}

// nrec records (l, w): every channel among the bands the handle holds, every absorber index -1 or among the nabs of WB (w null: none given)
inline int screen_channels(const bspatom_problem *p, const int32_t *l, const int32_t *w, int nrec, int nabs)
{
    for (int m = 0; m < nrec; ++m) {
        if (p->band_nl < 1 || l[m] < p->band_l0 || l[m] >= p->band_l0 + p->band_nl) return BSP_ERR_ARG;
        if (w && (w[m] < -1 || w[m] >= nabs)) return BSP_ERR_ARG;
    }
    return BSP_OK;
}
// the coupling topology: blocks (cr, cc) among the nch channels, ctr 0 or 1
inline int screen_couplings(int nch, int ncoup, const int32_t *cr, const int32_t *cc, const int32_t *ctr)
{
    for (int q = 0; q < ncoup; ++q)
        if (cr[q] < 0 || cr[q] >= nch || cc[q] < 0 || cc[q] >= nch || ctr[q] < 0 || ctr[q] > 1) return BSP_ERR_ARG;
    return BSP_OK;
}
// what the kernels read for screened records: the channel's place among the bands, its absorber (without w the first, -1: none)
inline void select_channels(const bspatom_problem *p, const int32_t *l, const int32_t *w, int nrec, int nabs, std::vector<int> &chan, std::vector<int> &wsel)
{
    chan.resize(nrec);
    wsel.assign(nrec, nabs > 0 && !w ? 0 : -1);
    for (int m = 0; m < nrec; ++m) { chan[m] = l[m] - p->band_l0; if (w) wsel[m] = w[m]; }
}
}  // namespace bsp
