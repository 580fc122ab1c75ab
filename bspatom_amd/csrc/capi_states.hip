// capi_states.hip -- the entry points of the C ABI (include/bspatom.h) that consume the last solve of a problem: eigenvectors,
// dipole elements and matrices, wave functions.  All work goes on the problem's stream.  An entry point that enqueues work on
// scratch of its own returns through drain / finish (capi_internal.h): every path waits for the stream before the scratch is freed.
#include <algorithm>
#include <climits>
#include "capi_internal.h"

using namespace bsp;

static size_t dipole_band_doubles(const HostSetup &h) { return (size_t)3 * (2 * h.k - 1) * h.nfun; }

extern "C" int bspatom_dipole_bands(bspatom_problem *p, double *RB)
{
    if (!p || !RB) return BSP_ERR_ARG;
    const HostSetup &h = p->hs;
    BSP_HIP(hipSetDevice(p->device));
    int rc;
    if ((rc = ensure_point_table(p))) return rc;
    DevArray<double> d_RB;
    if ((rc = d_RB.alloc(dipole_band_doubles(h)))) return rc;
    rc = launch_dipole_bands(h.nfun, h.k, h.ka, h.nkp, p->d_ptab, p->d_left, d_RB.p, p->st);
    if (!rc) rc = HIP_RC(hipMemcpyAsync(RB, d_RB.p, dipole_band_doubles(h) * sizeof(double), hipMemcpyDeviceToHost, p->st));
    if ((rc = drain(p, rc))) return rc;
    return check_status(p);
}

extern "C" int bspatom_eigvec(bspatom_problem *p, int l, int n0, double *c)
{
    if (!p || !c) return BSP_ERR_ARG;
    const HostSetup &h = p->hs;
    const int n = h.nfun;
    int rc;
    if ((rc = last_solve_window(p, l, 1, n0, 1))) return rc;
    BSP_HIP(hipSetDevice(p->device));
    if (l == p->pre_l && n0 == p->pre_n0) {                  // computed beside the bisection of the last solve
        int pinfo = 0;
        BSP_HIP(hipMemcpy(&pinfo, p->d_pinfo, sizeof(int), hipMemcpyDeviceToHost));
        if (pinfo) return BSP_ERR_UNSUPPORTED;              // the inverse iteration broke down (vector of norm 0)
        BSP_HIP(hipMemcpy(c, p->d_pvec, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
        return BSP_OK;
    }
    if ((rc = ensure_vec_scratch(p))) return rc;
    const int ch = l - p->last_l0;
    BSP_HIP(hipMemcpyAsync(p->d_chan, &ch, sizeof(int), hipMemcpyHostToDevice, p->st));
    BSP_HIP(hipMemcpyAsync(p->d_Esel, p->d_E + (size_t)ch * n + (n0 - 1), sizeof(double), hipMemcpyDeviceToDevice, p->st));
    BSP_HIP(hipMemsetAsync(p->d_info, 0, sizeof(int), p->st));
    if ((rc = launch_inverse_iteration(n, h.k, 1, p->d_SB, p->d_HB, p->d_chan, p->d_Esel, p->d_vwork, p->d_vec,
                                       p->d_info, p->st))) return rc;
    BSP_HIP(hipMemcpyAsync(c, p->d_vec, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, p->st));
    BSP_HIP(hipStreamSynchronize(p->st));
    return invit_failed(p);
}

namespace {
// bspatom_eigvecs' path, kept apart from the batch kernel, which is tested against it: vectors of ONE channel of the last solve by
// launch_inverse_iteration, at most 512 per launch (the chunk bounds the scratch: invit_work_doubles(n, k) per vector)
struct EigChunks {
    int chunk = 0;
    DevArray<double> work, vec;                    // vec: [chunk][n], the vectors of run's last launch
    DevArray<int> chan;                            // [chunk]: the channel of every vector of a launch
    int prepare(bspatom_problem *p, int count)
    {
        const HostSetup &h = p->hs;
        chunk = count < 512 ? count : 512;
        int rc;
        if ((rc = work.alloc((size_t)chunk * invit_work_doubles(h.nfun, h.k))) || (rc = vec.alloc((size_t)chunk * h.nfun))) return rc;
        return chan.alloc(chunk);
    }
    // the launches that follow take channel ch; waits for the ones before, which may still read the array
    int channel(bspatom_problem *p, int ch)
    {
        BSP_HIP(hipStreamSynchronize(p->st));
        const std::vector<int> hc(chunk, ch);
        BSP_HIP(hipMemcpy(chan.p, hc.data(), (size_t)chunk * sizeof(int), hipMemcpyHostToDevice));
        return BSP_OK;
    }
    // m <= chunk vectors from state n0 on, to out[m][n]
    int launch(bspatom_problem *p, int ch, int n0, int m, double *out)
    {
        const HostSetup &h = p->hs;
        return launch_inverse_iteration(h.nfun, h.k, m, p->d_SB, p->d_HB, chan.p, p->d_E + (size_t)ch * h.nfun + (n0 - 1), work.p, out,
                                        p->d_info, p->st);
    }
    // states n0 .. n0+count-1 chunk by chunk into vec: consume(done, m) enqueues what reads the m vectors from state n0 + done on,
    // and the stream is waited for before the next chunk overwrites them
    template <class F>
    int run(bspatom_problem *p, int ch, int n0, int count, F consume)
    {
        int rc = BSP_OK;
        for (int done = 0; !rc && done < count; done += chunk) {
            const int m = std::min(chunk, count - done);
            if (!(rc = launch(p, ch, n0 + done, m, vec.p)) && !(rc = consume(done, m))) rc = HIP_RC(hipStreamSynchronize(p->st));
        }
        return rc;
    }
};

// Eigenvector blocks of runs of consecutive channels of the last solve by launch_inverse_iteration_batch (eigvec.hip::
// invit_batch_kernel, one persistent launch per run): bspatom_eigvecs' vectors bit for bit.  The scratch is one slot per resident
// wave, whatever the number of vectors.
struct EigBlocks {
    int slots = 0;
    DevArray<double> work;
    int prepare(bspatom_problem *p, int max_items)             // for launches of at most max_items vectors
    {
        const HostSetup &h = p->hs;
        int rc;
        if ((rc = invit_batch_slots(h.k, max_items, &slots))) return rc;
        return work.alloc((size_t)slots * invit_batch_slot_doubles(h.nfun, h.k));
    }
    // states n0 .. n0+count-1 of channels ch .. ch+nch-1 (counted from the first channel of the last solve) to out[nch][count][n]
    int launch(bspatom_problem *p, int ch, int nch, int n0, int count, double *out)
    {
        const HostSetup &h = p->hs;
        const int n = h.nfun, items = nch * count;
        return launch_inverse_iteration_batch(n, h.k, count, items, slots < items ? slots : items, p->d_SB, p->d_HB + (size_t)ch * h.k * n,
                                              p->d_E + (size_t)ch * n + (n0 - 1), work.p, out, p->d_info, p->st);
    }
};
}  // namespace

// channels per launch of EigBlocks for blocks of `count` vectors, nl at most: items = channels * count stays an int, and the
// channels' blocks stay within stage_bytes (0: no bound), one channel at least
static int channel_group(const bspatom_problem *p, int nl, int count, size_t stage_bytes)
{
    size_t gmax = ((size_t)1 << 30) / count;
    if (stage_bytes) gmax = std::min(gmax, stage_bytes / ((size_t)count * p->hs.nfun * sizeof(double)));
    if (gmax < 1) gmax = 1;
    return (size_t)nl < gmax ? nl : (int)gmax;
}

extern "C" int bspatom_eigvecs(bspatom_problem *p, int l, int n0, int count, double *Z)
{
    if (!p || !Z) return BSP_ERR_ARG;
    int rc;
    if ((rc = last_solve_window(p, l, 1, n0, count))) return rc;
    BSP_HIP(hipSetDevice(p->device));
    const size_t n = p->hs.nfun;
    const int ch = l - p->last_l0;
    EigChunks ec;
    if ((rc = ec.prepare(p, count)) || (rc = ec.channel(p, ch))) return rc;
    rc = HIP_RC(hipMemsetAsync(p->d_info, 0, sizeof(int), p->st));
    if (!rc) rc = ec.run(p, ch, n0, count, [&](int done, int m) {
        return HIP_RC(hipMemcpyAsync(Z + done * n, ec.vec.p, m * n * sizeof(double), hipMemcpyDeviceToHost, p->st));
    });
    return finish(p, rc);
}

// bspatom_eigvecs for the channel range l0 .. l0+nl-1 in one persistent launch per group of channels: the same vectors bit for
// bit.  Z: host memory (dev false: staged through a device buffer of at most EIGVECS_STAGE_BYTES, one channel at least) or the
// caller's device memory (dev true: written in place).
static constexpr size_t EIGVECS_STAGE_BYTES = (size_t)256 << 20;
static int eigvecs_batch_impl(bspatom_problem *p, int l0, int nl, int n0, int count, double *Z, bool dev)
{
    if (!p || !Z) return BSP_ERR_ARG;
    int rc;
    if ((rc = last_solve_window(p, l0, nl, n0, count))) return rc;
    BSP_HIP(hipSetDevice(p->device));
    const int ch0 = l0 - p->last_l0;
    const size_t per_ch = (size_t)count * p->hs.nfun;         // doubles of one channel's block
    const int group = channel_group(p, nl, count, dev ? 0 : EIGVECS_STAGE_BYTES);
    EigBlocks eb;
    DevArray<double> stage;
    if ((rc = eb.prepare(p, group * count)) || (!dev && (rc = stage.alloc((size_t)group * per_ch)))) return rc;
    rc = HIP_RC(hipMemsetAsync(p->d_info, 0, sizeof(int), p->st));
    for (int c = 0; !rc && c < nl; c += group) {
        const int g = std::min(group, nl - c);
        rc = eb.launch(p, ch0 + c, g, n0, count, dev ? Z + (size_t)c * per_ch : stage.p);
        if (!rc && !dev) rc = HIP_RC(hipMemcpyAsync(Z + (size_t)c * per_ch, stage.p, (size_t)g * per_ch * sizeof(double), hipMemcpyDeviceToHost, p->st));
    }
    return finish(p, rc);
}

extern "C" int bspatom_eigvecs_batch(bspatom_problem *p, int l0, int nl, int n0, int count, double *Z)
{
    return eigvecs_batch_impl(p, l0, nl, n0, count, Z, false);
}
extern "C" int bspatom_eigvecs_batch_dev(bspatom_problem *p, int l0, int nl, int n0, int count, double *Z_dev)
{
    return eigvecs_batch_impl(p, l0, nl, n0, count, Z_dev, true);
}

extern "C" int bspatom_dipole_elements(bspatom_problem *p, int l_ini, int n0_ini, int l_fin, int n0_fin, int count,
                                       const double a[3], double *D)
{
    if (!p || !a || !D) return BSP_ERR_ARG;
    if (last_solve_window(p, l_ini, 1, n0_ini, 1) || last_solve_window(p, l_fin, 1, n0_fin, count)) return BSP_ERR_ARG;
    const HostSetup &h = p->hs;
    const int n = h.nfun, ch_ini = l_ini - p->last_l0, ch_fin = l_fin - p->last_l0;
    BSP_HIP(hipSetDevice(p->device));
    int rc;
    if ((rc = ensure_point_table(p))) return rc;
    DevArray<double> RB, ci, v, dD;
    EigChunks ec;
    if ((rc = RB.alloc(dipole_band_doubles(h))) || (rc = ec.prepare(p, count)) || (rc = ci.alloc(n)) || (rc = v.alloc(n)) ||
        (rc = dD.alloc(ec.chunk)) || (rc = ec.channel(p, ch_ini))) return rc;
    // v = (a0 R_r + a1 R_1/r + a2 R_d/dr) c_ini
    rc = HIP_RC(hipMemsetAsync(p->d_info, 0, sizeof(int), p->st));
    if (!rc) rc = launch_dipole_bands(n, h.k, h.ka, h.nkp, p->d_ptab, p->d_left, RB.p, p->st);
    if (!rc) rc = ec.launch(p, ch_ini, n0_ini, 1, ci.p);
    if (!rc) rc = launch_band_apply(n, h.k, RB.p, a, ci.p, v.p, p->st);
    if (!rc) rc = ec.channel(p, ch_fin);
    // D(i) = c_fin(:, n0_fin + i) . v, the final states in chunks
    if (!rc) rc = ec.run(p, ch_fin, n0_fin, count, [&](int done, int m) {
        const int rd = launch_dots(n, m, ec.vec.p, v.p, dD.p, p->st);
        return rd ? rd : HIP_RC(hipMemcpyAsync(D + done, dD.p, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, p->st));
    });
    if ((rc = finish(p, rc))) return rc;
    return check_status(p);
}

// bspatom_dipole_elements for whole windows of initial and final states of many channel pairs in one call (dipole.hip):
// D[p][i][f] = c(l_fin[p], n0_fin + f)^T (a[3p] R_r + a[3p+1] R_1/r + a[3p+2] R_d/dr) c(l_ini[p], n0_ini + i).
// The pairs are taken in groups, in the order given; the device scratch of a group -- its distinct (channel, window) eigenvector
// blocks, W = A x of its distinct (operator, initial block) items, the split-K partials and, for host output, D itself --
// stays within DIPOLE_STAGE_BYTES (option dipole_stage_mb), one pair at least.  The eigenvectors are bspatom_eigvecs' bit for
// bit (one EigBlocks launch per run of consecutive channels and window); nothing of a pair's arithmetic depends on
// the other pairs or on the grouping.  The scratch of the inverse iterations is one slot per resident wave beside that.
// pair_matrix_impl is that plan for any number nco of coefficients per pair (bspatom_operator_matrix: A_p = sum_o a[p*nco + o]
// G_o); the operator bands and the apply launch are the caller's, the bands counted outside the bound.
static constexpr size_t DIPOLE_STAGE_BYTES = (size_t)2 << 30;
namespace {
struct DipItem {                                   // W item: operator (nco coefficients of the caller's array) and initial channel
    int ch, nco; const double *a;
    bool operator<(const DipItem &o) const { return ch != o.ch ? ch < o.ch : memcmp(a, o.a, (size_t)nco * sizeof(double)) < 0; }
};
struct DipRun { int ch, len, w; size_t pos; };     // channels ch .. ch+len-1, block pos .. of the list of window w (0: chA, 1: chB)
struct DipGroup {
    int p0 = 0, np = 0;
    std::vector<int> chA, chB;                     // sorted distinct channels whose initial / final window the group needs
    std::vector<DipItem> items;                    // sorted distinct W items
    std::vector<DipRun> runs;                      // one EigBlocks launch each (find_runs)
    static bool has(const std::vector<int> &v, int c) { return std::binary_search(v.begin(), v.end(), c); }
    static void add(std::vector<int> &v, int c) { if (!has(v, c)) v.insert(std::lower_bound(v.begin(), v.end(), c), c); }
    static int pos(const std::vector<int> &v, int c) { return (int)(std::lower_bound(v.begin(), v.end(), c) - v.begin()); }
    bool has_item(const DipItem &t) const { return std::binary_search(items.begin(), items.end(), t); }
    int item_pos(const DipItem &t) const { return (int)(std::lower_bound(items.begin(), items.end(), t) - items.begin()); }
    // the maximal runs of consecutive channels of chA, then of chB, of at most gmax[w] channels
    void find_runs(const int gmax[2])
    {
        for (int w = 0; w < 2; ++w) {
            const std::vector<int> &ch = w ? chB : chA;
            for (size_t i = 0, j; i < ch.size(); i = j) {
                for (j = i + 1; j < ch.size() && ch[j] == ch[j - 1] + 1 && (int)(j - i) < gmax[w]; ++j) {}
                runs.push_back({ch[i], (int)(j - i), w, i});
            }
        }
    }
};
}  // namespace

// bands(): allocates and enqueues the operator bands of the call on the problem's stream (after the point table);
// apply(nitems, d_acoef, d_xoff, d_base, d_W): the launch of W = A x for nitems items, d_acoef[nitems][nco].
template <class Bands, class Apply>
static int pair_matrix_impl(bspatom_problem *p, int nco, int npairs, const int32_t *l_ini, const int32_t *l_fin, int n0_ini,
                            int count_ini, int n0_fin, int count_fin, const double *a, double *D, bool dev, Bands bands, Apply apply)
{
    if (!p || !l_ini || !l_fin || !a || !D || npairs < 1 || nco < 1) return BSP_ERR_ARG;
    for (int q = 0; q < npairs; ++q)
        if (last_solve_window(p, l_ini[q], 1, n0_ini, count_ini) || last_solve_window(p, l_fin[q], 1, n0_fin, count_fin)) return BSP_ERR_ARG;
    const HostSetup &h = p->hs;
    const int n = h.nfun, lo = p->last_l0;
    BSP_HIP(hipSetDevice(p->device));
    int rc;
    if ((rc = ensure_point_table(p))) return rc;
    // ---- the groups ----
    const bool same = n0_ini == n0_fin && count_ini == count_fin;        // one window: a channel's block serves both roles
    const size_t mn = (size_t)count_ini * count_fin, vi = (size_t)count_ini * n, vf = (size_t)count_fin * n;
    int chunk = 0, ns = 1;
    dipole_kslices(n, count_ini, count_fin, &chunk, &ns);
    const size_t per_pair = (ns > 1 ? (size_t)ns * mn : 0) + (dev ? 0 : mn);
    const size_t limit = (opts().dipole_stage_mb > 0 ? (size_t)opts().dipole_stage_mb << 20 : DIPOLE_STAGE_BYTES) / sizeof(double);
    auto item_of = [&](int q) { return DipItem{l_ini[q] - lo, nco, a + (size_t)nco * q}; };
    auto doubles_of = [&](const DipGroup &g) {
        return g.chA.size() * vi + g.chB.size() * vf + g.items.size() * vi + (size_t)g.np * per_pair;
    };
    std::vector<DipGroup> groups;
    DipGroup cur;
    for (int q = 0; q < npairs; ++q) {
        const int ci = l_ini[q] - lo, cf = l_fin[q] - lo;
        const DipItem t = item_of(q);
        if (cur.np > 0) {
            // what the group would need with this pair in it
            size_t need = doubles_of(cur) + per_pair;
            if (!DipGroup::has(cur.chA, ci)) need += vi;
            if (same) { if (cf != ci && !DipGroup::has(cur.chA, cf)) need += vi; }
            else if (!DipGroup::has(cur.chB, cf)) need += vf;
            if (!cur.has_item(t)) need += vi;
            if (need > limit) { groups.push_back(cur); cur = DipGroup(); cur.p0 = q; }
        }
        DipGroup::add(cur.chA, ci);
        DipGroup::add(same ? cur.chA : cur.chB, cf);
        if (!cur.has_item(t)) cur.items.insert(cur.items.begin() + cur.item_pos(t), t);
        cur.np += 1;
    }
    groups.push_back(cur);
    // ---- the runs, the tables (offsets in doubles from the scratch base) and sizes ----
    const int n0w[2] = {n0_ini, n0_fin}, cntw[2] = {count_ini, count_fin};
    const int gmax[2] = {channel_group(p, INT_MAX, count_ini, 0), channel_group(p, INT_MAX, count_fin, 0)};
    size_t stage_doubles = 0, nitems_all = 0;
    int max_run_items = 1;
    for (DipGroup &g : groups) {
        stage_doubles = std::max(stage_doubles, doubles_of(g));
        nitems_all += g.items.size();
        g.find_runs(gmax);
        for (const DipRun &r : g.runs) max_run_items = std::max(max_run_items, r.len * cntw[r.w]);
    }
    std::vector<long long> tab(nitems_all + 2 * (size_t)npairs);      // [xoff of every item | (W, Z) offsets of every pair]
    std::vector<double> acoef((size_t)nco * nitems_all);
    size_t q0 = 0;                                                    // items of the groups before
    for (const DipGroup &g : groups) {
        const size_t offB = g.chA.size() * vi, offW = offB + g.chB.size() * vf;
        for (size_t t = 0; t < g.items.size(); ++t) {
            tab[q0 + t] = (long long)((size_t)DipGroup::pos(g.chA, g.items[t].ch) * vi);
            memcpy(&acoef[(size_t)nco * (q0 + t)], g.items[t].a, (size_t)nco * sizeof(double));
        }
        for (int q = g.p0; q < g.p0 + g.np; ++q) {
            const int cf = l_fin[q] - lo;
            tab[nitems_all + 2 * (size_t)q] = (long long)(offW + (size_t)g.item_pos(item_of(q)) * vi);
            tab[nitems_all + 2 * (size_t)q + 1] = same ? (long long)((size_t)DipGroup::pos(g.chA, cf) * vi)
                                                       : (long long)(offB + (size_t)DipGroup::pos(g.chB, cf) * vf);
        }
        q0 += g.items.size();
    }
    DevArray<double> stage, dA;
    DevArray<long long> dtab;
    EigBlocks eb;
    if ((rc = eb.prepare(p, max_run_items)) || (rc = stage.alloc(stage_doubles)) ||
        (rc = dA.put(acoef.data(), acoef.size())) || (rc = dtab.put(tab.data(), tab.size()))) return rc;
    // ---- group by group on the problem's stream ----
    rc = HIP_RC(hipMemsetAsync(p->d_info, 0, sizeof(int), p->st));
    if (!rc) rc = bands();
    q0 = 0;
    for (size_t gi = 0; !rc && gi < groups.size(); ++gi) {
        const DipGroup &g = groups[gi];
        const size_t offB = g.chA.size() * vi, offW = offB + g.chB.size() * vf, offP = offW + g.items.size() * vi;
        const size_t offD = offP + (ns > 1 ? (size_t)g.np * ns * mn : 0);
        for (const DipRun &r : g.runs)
            if (!rc) rc = eb.launch(p, r.ch, r.len, n0w[r.w], cntw[r.w], stage.p + (r.w ? offB + r.pos * vf : r.pos * vi));
        if (!rc) rc = apply((int)g.items.size(), dA.p + (size_t)nco * q0, dtab.p + q0, stage.p, stage.p + offW);
        double *out = dev ? D + (size_t)g.p0 * mn : stage.p + offD;
        if (!rc) rc = launch_dipole_block(n, count_ini, count_fin, g.np, dtab.p + nitems_all + 2 * (size_t)g.p0, stage.p,
                                          ns > 1 ? stage.p + offP : nullptr, out, p->st);
        if (!rc && !dev) rc = HIP_RC(hipMemcpyAsync(D + (size_t)g.p0 * mn, out, (size_t)g.np * mn * sizeof(double), hipMemcpyDeviceToHost, p->st));
        q0 += g.items.size();
    }
    if ((rc = finish(p, rc))) return rc;
    return check_status(p);
}

static int dipole_matrix_impl(bspatom_problem *p, int npairs, const int32_t *l_ini, const int32_t *l_fin, int n0_ini, int count_ini,
                              int n0_fin, int count_fin, const double *a, double *D, bool dev)
{
    DevArray<double> RB;
    return pair_matrix_impl(p, 3, npairs, l_ini, l_fin, n0_ini, count_ini, n0_fin, count_fin, a, D, dev,
        [&]() {
            const HostSetup &h = p->hs;
            const int rc = RB.alloc(dipole_band_doubles(h));
            return rc ? rc : launch_dipole_bands(h.nfun, h.k, h.ka, h.nkp, p->d_ptab, p->d_left, RB.p, p->st);
        },
        [&](int nitems, const double *d_acoef, const long long *d_xoff, const double *d_base, double *d_W) {
            return launch_band_apply_block(p->hs.nfun, p->hs.k, count_ini, nitems, RB.p, d_acoef, d_xoff, d_base, d_W, p->st);
        });
}

extern "C" int bspatom_dipole_matrix(bspatom_problem *p, int npairs, const int32_t *l_ini, const int32_t *l_fin, int n0_ini,
                                     int count_ini, int n0_fin, int count_fin, const double *a, double *D)
{
    return dipole_matrix_impl(p, npairs, l_ini, l_fin, n0_ini, count_ini, n0_fin, count_fin, a, D, false);
}
extern "C" int bspatom_dipole_matrix_dev(bspatom_problem *p, int npairs, const int32_t *l_ini, const int32_t *l_fin, int n0_ini,
                                         int count_ini, int n0_fin, int count_fin, const double *a, double *D_dev)
{
    return dipole_matrix_impl(p, npairs, l_ini, l_fin, n0_ini, count_ini, n0_fin, count_fin, a, D_dev, true);
}

// ---- caller-given radial operators g(r), g(r) d/dr (opmat.hip) -------------------------------------------------------------
namespace {
// The operator bands of a call: g (nop*nr doubles indexed like bspatom_quadrature's points; host memory is uploaded once, device
// memory is read in place), deriv and the interval table of operator_band_kernel (from wf_quadrature's rows) on the device.
struct OpBands {
    int nop = 0, nr = 0;
    DevArray<double> g_up, GB;
    DevArray<int> deriv, qfirst;
    const double *d_g = nullptr;
    double *band = nullptr;                        // [nop][2k-1][nfun]: GB, or the caller's device memory
    static bool args_ok(const bspatom_problem *p, int nop, const double *g, const int32_t *deriv)
    {
        if (!p || !g || !deriv || nop < 1) return false;
        for (int o = 0; o < nop; ++o)
            if (deriv[o] != 0 && deriv[o] != 1) return false;
        return true;
    }
    int prepare(bspatom_problem *p, int nop_, const double *g, bool g_dev, const int32_t *deriv_, double *GB_dev)
    {
        const HostSetup &h = p->hs;
        nop = nop_;
        nr = wf_quadrature(h.nkp, h.ka, h.rt.data(), h.xg.data(), h.wg.data(), nullptr, nullptr, nullptr);
        if (nr < 1) return BSP_ERR_ARG;
        std::vector<int> rows(nr), qf(h.nkp - 1, -1), dv(deriv_, deriv_ + nop);
        wf_quadrature(h.nkp, h.ka, h.rt.data(), h.xg.data(), h.wg.data(), rows.data(), nullptr, nullptr);
        for (int q = 0; q < nr; q += h.ka) qf[rows[q] / h.ka] = q;
        int rc;
        if ((rc = qfirst.put(qf.data(), qf.size())) || (rc = deriv.put(dv.data(), dv.size()))) return rc;
        if (!GB_dev && (rc = GB.alloc(doubles(h)))) return rc;
        band = GB_dev ? GB_dev : GB.p;
        if (g_dev) d_g = g;
        else { if ((rc = g_up.put(g, (size_t)nop * nr))) return rc; d_g = g_up.p; }
        return BSP_OK;
    }
    size_t doubles(const HostSetup &h) const { return (size_t)nop * (2 * h.k - 1) * h.nfun; }
    int launch(bspatom_problem *p) const
    {
        const HostSetup &h = p->hs;
        return launch_operator_bands(h.nfun, h.k, h.ka, h.nkp, nop, nr, p->d_ptab, p->d_left, qfirst.p, d_g, deriv.p, band, p->st);
    }
};
}  // namespace

static int operator_bands_impl(bspatom_problem *p, int nop, const double *g, const int32_t *deriv, double *GB, bool dev)
{
    if (!OpBands::args_ok(p, nop, g, deriv) || !GB) return BSP_ERR_ARG;
    BSP_HIP(hipSetDevice(p->device));
    int rc;
    if ((rc = ensure_point_table(p))) return rc;
    OpBands ob;
    if ((rc = ob.prepare(p, nop, g, dev, deriv, dev ? GB : nullptr))) return rc;
    rc = ob.launch(p);
    if (!rc && !dev) rc = HIP_RC(hipMemcpyAsync(GB, ob.band, ob.doubles(p->hs) * sizeof(double), hipMemcpyDeviceToHost, p->st));
    if ((rc = drain(p, rc))) return rc;
    return check_status(p);
}

extern "C" int bspatom_operator_bands(bspatom_problem *p, int nop, const double *g, const int32_t *deriv, double *GB)
{
    return operator_bands_impl(p, nop, g, deriv, GB, false);
}
extern "C" int bspatom_operator_bands_dev(bspatom_problem *p, int nop, const double *g_dev, const int32_t *deriv, double *GB_dev)
{
    return operator_bands_impl(p, nop, g_dev, deriv, GB_dev, true);
}

// bspatom_dipole_matrix's plan (pair_matrix_impl) with the bands of the caller's operators and nop coefficients per pair
static int operator_matrix_impl(bspatom_problem *p, int nop, const double *g, const int32_t *deriv, int npairs, const int32_t *l_ini,
                                const int32_t *l_fin, int n0_ini, int count_ini, int n0_fin, int count_fin, const double *a, double *D,
                                bool dev)
{
    if (!OpBands::args_ok(p, nop, g, deriv)) return BSP_ERR_ARG;
    OpBands ob;
    return pair_matrix_impl(p, nop, npairs, l_ini, l_fin, n0_ini, count_ini, n0_fin, count_fin, a, D, dev,
        [&]() {
            const int rc = ob.prepare(p, nop, g, dev, deriv, nullptr);
            return rc ? rc : ob.launch(p);
        },
        [&](int nitems, const double *d_acoef, const long long *d_xoff, const double *d_base, double *d_W) {
            return launch_band_combine_apply(p->hs.nfun, p->hs.k, nop, count_ini, nitems, ob.band, d_acoef, d_xoff, d_base, d_W, p->st);
        });
}

extern "C" int bspatom_operator_matrix(bspatom_problem *p, int nop, const double *g, const int32_t *deriv, int npairs,
                                       const int32_t *l_ini, const int32_t *l_fin, int n0_ini, int count_ini, int n0_fin,
                                       int count_fin, const double *a, double *D)
{
    return operator_matrix_impl(p, nop, g, deriv, npairs, l_ini, l_fin, n0_ini, count_ini, n0_fin, count_fin, a, D, false);
}
extern "C" int bspatom_operator_matrix_dev(bspatom_problem *p, int nop, const double *g_dev, const int32_t *deriv, int npairs,
                                           const int32_t *l_ini, const int32_t *l_fin, int n0_ini, int count_ini, int n0_fin,
                                           int count_fin, const double *a, double *D_dev)
{
    return operator_matrix_impl(p, nop, g_dev, deriv, npairs, l_ini, l_fin, n0_ini, count_ini, n0_fin, count_fin, a, D_dev, true);
}

extern "C" int bspatom_write_wf(bspatom_problem *p, const double *c, int npts, double *r, double *u)
{
    if (!p || !c || !r || !u || npts < 1) return BSP_ERR_ARG;
    const HostSetup &h = p->hs;
    BSP_HIP(hipSetDevice(p->device));
    if (p->wf_cap < npts + 1) {
        hipFree(p->d_wfr); hipFree(p->d_wfu);
        p->d_wfr = p->d_wfu = nullptr; p->wf_cap = 0;
        BSP_HIP(hipMalloc(reinterpret_cast<void **>(&p->d_wfr), (size_t)(npts + 1) * sizeof(double)));
        BSP_HIP(hipMalloc(reinterpret_cast<void **>(&p->d_wfu), (size_t)(npts + 1) * sizeof(double)));
        p->wf_cap = npts + 1;
    }
    DevArray<double> d_c;
    int rc;
    if ((rc = d_c.alloc(h.nfun))) return rc;
    rc = HIP_RC(hipMemcpyAsync(d_c.p, c, (size_t)h.nfun * sizeof(double), hipMemcpyHostToDevice, p->st));
    if (!rc) rc = HIP_RC(hipMemsetAsync(p->d_status, 0, sizeof(int), p->st));
    if (!rc) rc = launch_wf_tabulate(h.nkp, h.k, h.nfun, p->d_rt, d_c.p, h.in.ra, h.in.rb, npts, p->d_wfr, p->d_wfu, p->d_status, p->st);
    if ((rc = drain(p, rc))) return rc;
    if ((rc = check_status(p))) { hipMemset(p->d_status, 0, sizeof(int)); return rc; }
    BSP_HIP(hipMemcpy(r, p->d_wfr, (size_t)(npts + 1) * sizeof(double), hipMemcpyDeviceToHost));
    BSP_HIP(hipMemcpy(u, p->d_wfu, (size_t)(npts + 1) * sizeof(double), hipMemcpyDeviceToHost));
    return BSP_OK;
}

// ---- u(r), u'(r) of blocks of vectors (wavefn.hip; WFALL, TorusFuns.f90:193-261) -------------------------------------------

extern "C" int bspatom_quadrature(bspatom_problem *p, int *nr, double *r, double *w)
{
    if (!p || !nr) return BSP_ERR_ARG;
    const HostSetup &h = p->hs;
    *nr = wf_quadrature(h.nkp, h.ka, h.rt.data(), h.xg.data(), h.wg.data(), nullptr, r, w);
    return BSP_OK;
}

static constexpr size_t WF_STAGE_BYTES = (size_t)256 << 20;
static size_t wf_stage_bytes() { return opts().wf_stage_mb > 0 ? (size_t)opts().wf_stage_mb << 20 : WF_STAGE_BYTES; }

struct WfBasis {
    DevArray<double> tab;       // [2k][npts]
    DevArray<int> left;         // [npts]
};

// The basis table of a call on the problem's stream: r == nullptr: the quadrature grid (npts must be its size; the rows of the
// assembly's point table, which is run first if it has not been), else the caller's points, checked on the host before any launch.
// Returns with the stream drained (the uploads it made are freed here) and the kernels' status word checked.
static int wf_basis(bspatom_problem *p, int npts, const double *r, WfBasis *b)
{
    const HostSetup &h = p->hs;
    if (npts < 1) return BSP_ERR_ARG;
    std::vector<int> rows;
    if (!r) {
        if (npts != wf_quadrature(h.nkp, h.ka, h.rt.data(), h.xg.data(), h.wg.data(), nullptr, nullptr, nullptr)) return BSP_ERR_ARG;
        rows.resize(npts);
        wf_quadrature(h.nkp, h.ka, h.rt.data(), h.xg.data(), h.wg.data(), rows.data(), nullptr, nullptr);
    } else if (!wf_points_valid(h.nkp, h.rt.data(), npts, r)) return BSP_ERR_ARG;
    BSP_HIP(hipSetDevice(p->device));
    int rc;
    if ((rc = b->tab.alloc((size_t)npts * 2 * h.k)) || (rc = b->left.alloc(npts))) return rc;
    DevArray<int> d_rows;
    DevArray<double> d_r;
    if (r) {
        if (!(rc = d_r.put(r, npts)))
            rc = launch_basis_table(h.nkp, h.k, h.nfun, npts, p->d_rt, p->d_aind, d_r.p, b->tab.p, b->left.p, p->d_status, p->st);
    } else if (!(rc = ensure_point_table(p)) && !(rc = d_rows.put(rows.data(), npts)))
        rc = launch_basis_gather(h.k, npts, d_rows.p, p->d_ptab, p->d_left, b->tab.p, b->left.p, p->st);
    if ((rc = drain(p, rc))) return rc;
    if ((rc = check_status(p))) { if (r) hipMemset(p->d_status, 0, sizeof(int)); return rc; }
    return BSP_OK;
}

// vectors per pass of a host variant: U and dU of them together stay within the staging bound, one vector's rows at least
static size_t wf_stage_vectors(int npts, bool deriv, size_t nvec)
{
    size_t g = wf_stage_bytes() / ((size_t)npts * (deriv ? 2 : 1) * sizeof(double));
    if (g < 1) g = 1;
    return g < nvec ? g : nvec;
}

// nv vectors at d_Z through the stage buffer ([m][npts] values, then [m][npts] derivatives) to the host rows U, dU
static int wf_stage_out(bspatom_problem *p, const WfBasis &b, int npts, size_t nv, size_t g, const double *d_Z, double *stage,
                        double *U, double *dU)
{
    const HostSetup &h = p->hs;
    for (size_t v = 0; v < nv; v += g) {
        const size_t m = nv - v < g ? nv - v : g;
        int rc;
        if ((rc = launch_tabulate(h.k, h.nfun, npts, (int)m, b.tab.p, b.left.p, d_Z + v * h.nfun, stage, dU ? stage + m * npts : nullptr,
                                  p->st))) return rc;
        BSP_HIP(hipMemcpyAsync(U + v * npts, stage, m * npts * sizeof(double), hipMemcpyDeviceToHost, p->st));
        if (dU) BSP_HIP(hipMemcpyAsync(dU + v * npts, stage + m * npts, m * npts * sizeof(double), hipMemcpyDeviceToHost, p->st));
    }
    return BSP_OK;
}

static int tabulate_impl(bspatom_problem *p, int nvec, const double *Z, int npts, const double *r, double *U, double *dU, bool dev)
{
    if (!p || !Z || !U || nvec < 1 || npts < 1) return BSP_ERR_ARG;
    const HostSetup &h = p->hs;
    WfBasis b;
    int rc;
    if ((rc = wf_basis(p, npts, r, &b))) return rc;
    DevArray<double> stage, zc;
    const size_t g = wf_stage_vectors(npts, dU != nullptr, nvec), n = h.nfun;
    if (!dev && ((rc = stage.alloc(g * npts * (dU ? 2 : 1))) || (rc = zc.alloc(g * n)))) return rc;
    if (dev) rc = launch_tabulate(h.k, h.nfun, npts, nvec, b.tab.p, b.left.p, Z, U, dU, p->st);
    else for (size_t v = 0; !rc && v < (size_t)nvec; v += g) {
        const size_t m = std::min(g, (size_t)nvec - v);
        rc = HIP_RC(hipMemcpyAsync(zc.p, Z + v * n, m * n * sizeof(double), hipMemcpyHostToDevice, p->st));
        if (!rc) rc = wf_stage_out(p, b, npts, m, g, zc.p, stage.p, U + v * npts, dU ? dU + v * npts : nullptr);
    }
    return drain(p, rc);
}

extern "C" int bspatom_tabulate(bspatom_problem *p, int nvec, const double *Z, int npts, const double *r, double *U, double *dU)
{
    return tabulate_impl(p, nvec, Z, npts, r, U, dU, false);
}
extern "C" int bspatom_tabulate_dev(bspatom_problem *p, int nvec, const double *Z_dev, int npts, const double *r, double *U_dev,
                                    double *dU_dev)
{
    return tabulate_impl(p, nvec, Z_dev, npts, r, U_dev, dU_dev, true);
}

// The eigenvectors come from EigBlocks in groups of channels (bspatom_eigvecs_batch's launch: the same bits), one group's block
// within the staging bound (one channel at least); a group is tabulated from device memory, in place (dev) or through the stage
// buffer.
static int wavefunctions_impl(bspatom_problem *p, int l0, int nl, int n0, int count, int npts, const double *r, double *U, double *dU,
                              bool dev)
{
    if (!p || !U || npts < 1) return BSP_ERR_ARG;
    int rc;
    if ((rc = last_solve_window(p, l0, nl, n0, count))) return rc;
    const HostSetup &h = p->hs;
    WfBasis b;
    if ((rc = wf_basis(p, npts, r, &b))) return rc;
    const int ch0 = l0 - p->last_l0;
    const int group = channel_group(p, nl, count, wf_stage_bytes());
    EigBlocks eb;
    DevArray<double> zblk, stage;
    if ((rc = eb.prepare(p, group * count)) || (rc = zblk.alloc((size_t)group * count * h.nfun))) return rc;
    const size_t gv = wf_stage_vectors(npts, dU != nullptr, (size_t)group * count);
    if (!dev && (rc = stage.alloc(gv * npts * (dU ? 2 : 1)))) return rc;
    rc = HIP_RC(hipMemsetAsync(p->d_info, 0, sizeof(int), p->st));
    for (int c = 0; !rc && c < nl; c += group) {
        const int g = std::min(group, nl - c), items = g * count;
        if ((rc = eb.launch(p, ch0 + c, g, n0, count, zblk.p))) break;
        const size_t o = (size_t)c * count * npts;
        if (dev) rc = launch_tabulate(h.k, h.nfun, npts, items, b.tab.p, b.left.p, zblk.p, U + o, dU ? dU + o : nullptr, p->st);
        else rc = wf_stage_out(p, b, npts, (size_t)items, gv, zblk.p, stage.p, U + o, dU ? dU + o : nullptr);
    }
    return finish(p, rc);
}

extern "C" int bspatom_wavefunctions(bspatom_problem *p, int l0, int nl, int n0, int count, int npts, const double *r, double *U,
                                     double *dU)
{
    return wavefunctions_impl(p, l0, nl, n0, count, npts, r, U, dU, false);
}
extern "C" int bspatom_wavefunctions_dev(bspatom_problem *p, int l0, int nl, int n0, int count, int npts, const double *r,
                                         double *U_dev, double *dU_dev)
{
    return wavefunctions_impl(p, l0, nl, n0, count, npts, r, U_dev, dU_dev, true);
}
