// wavefn.hip -- u(r) = sum_j c_j B_j(r) and u'(r) = sum_j c_j B_j'(r) for blocks of coefficient vectors on many points.
//
// Replaces WFALL (reference TorusFuns.f90:193-261: fur(ir, n, l), dfur(ir, n, l) for all states of all channels at the
// quadrature points rtot, :87-104) with BSPALL (Modules.f90:71-110), bsplvb (bsplvb.f90:10-52) and interv (interv.f90:86-117)
// underneath.  The arithmetic is the reference's and nothing else: this file is compiled with -ffp-contract=off (no FMA),
// divisions are IEEE, and the sums run over the k local functions ascending from 0.0 with one multiply and one add per term
// (WFALL's order, wf_kernel's order) -- a value depends on its point and its vector alone, not on tiles, groups or the other
// vectors of the call.
//
// Basis table of a call, point index fastest: tab[j * npts + ip] = B_(left-k+1+j)(r_ip) for j < k, tab[(k + j) * npts + ip] the
// derivative; tleft[ip] = left (1-based, interv).
//   basis_table_kernel<K>    caller's points: one thread per point, interval by binary search with interv's two edge rules,
//                            both recurrences with K a compile-time constant (work arrays in registers; eigvec.hip::wf_kernel
//                            is the model)
//   basis_gather_kernel      quadrature grid: no recurrence, the rows of the assembly's point table (assemble.hip) that belong
//                            to knot intervals of positive width, transposed into the same layout
//   tabulate_kernel<K, DERIV>  grid (point tile, vector tile), one thread per point: the thread holds its K (2K) basis values
//                            in registers, walks the vectors of the tile, reads the K coefficients left-k+1 .. left -- from LDS,
//                            where the tile's windows are staged once when its points span few knot intervals (sorted points,
//                            the quadrature grid), else from global memory -- and stores U (and dU) with the point index
//                            fastest: a wave writes 512 contiguous bytes per vector and table
#include <cmath>
#include "common.h"

namespace bsp {

// ---- host: the assembly's quadrature (matrices.f90:91-97) ---------------------------------------------------------
// r = f1 + xg*f2, dr = f2*wg with f1 = (rt(i+1) + rt(i))/2, f2 = (rt(i+1) - rt(i))/2 for the intervals of positive width,
// ascending, ka per interval (point_table_kernel's expressions; this translation unit forms no FMA on the host either).
// rows (may be null): row of the device point table each point lives in.  Returns the number of points.
int wf_quadrature(int nkp, int ka, const double *rt0, const double *xg, const double *wg, int *rows, double *r, double *w)
{
    const double *rt = rt0 - 1;
    int nr = 0;
    for (int ibet = 1; ibet <= nkp - 1; ++ibet) {
        if (!(rt[ibet + 1] > rt[ibet])) continue;
        const double f1 = (rt[ibet + 1] + rt[ibet]) / 2.0;
        const double f2 = (rt[ibet + 1] - rt[ibet]) / 2.0;
        for (int g = 0; g < ka; ++g, ++nr) {
            if (rows) rows[nr] = (ibet - 1) * ka + g;
            if (r) r[nr] = f1 + xg[g] * f2;
            if (w) w[nr] = f2 * wg[g];
        }
    }
    return nr;
}

// every point finite and inside [rt(1), rt(nkp)] (outside it interv answers left = 1 and the reference's BSPLVB STOPs or
// extrapolates; the C ABI refuses such points before anything is launched)
bool wf_points_valid(int nkp, const double *rt0, int npts, const double *r)
{
    const double lo = rt0[0], hi = rt0[nkp - 1];
    for (int i = 0; i < npts; ++i)
        if (!std::isfinite(r[i]) || r[i] < lo || r[i] > hi) return false;
    return true;
}

constexpr int WF_TPB = 256;   // threads (= points) per workgroup
constexpr int WF_VT = 32;     // vectors per workgroup of tabulate_kernel

// ---- caller's points ------------------------------------------------------------------------------------------------
template <int K>
__global__ __launch_bounds__(WF_TPB) void basis_table_kernel(int nkp, int nfun, int npts, const double *__restrict__ rt0,
                                                             const double *__restrict__ aind, const double *__restrict__ rin,
                                                             double *__restrict__ tab, int *__restrict__ tleft, int *status)
{
    constexpr int k = K;
    const int ip = blockIdx.x * WF_TPB + threadIdx.x;
    if (ip >= npts) return;
    const double *t = rt0 - 1;
    const double r = rin[ip];
    // interv.f90:86-117: largest left with t(left) <= r < t(left+1); at r == t(nkp) the walk down to the last knot below it
    int left;
    if (r > t[nkp] || r < t[1]) left = 1;
    else if (r == t[nkp]) { left = nkp; while (left > 1 && !(t[left] < t[nkp])) --left; }
    else {
        int lo = 1, hi = nkp;                      // t[lo] <= r < t[hi]
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (t[mid] <= r) lo = mid; else hi = mid; }
        left = lo;
    }
    // bsplvb.f90:24-50 at orders k and k - 1 (BSPALL, Modules.f90:84-96).  deltar(j) = t(left+j) - r and deltal(j) =
    // r - t(left+1-j) are the same numbers in both calls, so they are formed once.  Knot reads stay inside 1 .. nkp
    // (a clamped read can only differ from the reference where the reference reads past its array).
    double bsp[K + 1], bsp1[K + 1], dl[K + 1], dR[K + 1];
#pragma unroll
    for (int j = 0; j <= k; ++j) { bsp[j] = 0.0; bsp1[j] = 0.0; }
    bsp[1] = 1.0;
    bsp1[1] = 1.0;
    if (k > 1) {
        if (t[left + 1] <= t[left]) { atomicExch(status, BSP_ERR_BSPLVB); return; }   // FATAL ERROR - BSPLVB (bsplvb.f90:30-34)
#pragma unroll
        for (int j = 1; j < k; ++j) {
            const int hiq = left + j < nkp ? left + j : nkp, loq = left + 1 - j > 1 ? left + 1 - j : 1;
            dR[j] = t[hiq] - r;
            dl[j] = r - t[loq];
            double saved = 0.0;
#pragma unroll
            for (int q = 1; q <= j; ++q) {
                const double term = bsp[q] / (dR[q] + dl[j + 1 - q]);
                bsp[q] = saved + dR[q] * term;
                saved = dl[j + 1 - q] * term;
            }
            bsp[j + 1] = saved;
        }
#pragma unroll
        for (int j = 1; j < k - 1; ++j) {
            double saved = 0.0;
#pragma unroll
            for (int q = 1; q <= j; ++q) {
                const double term = bsp1[q] / (dR[q] + dl[j + 1 - q]);
                bsp1[q] = saved + dR[q] * term;
                saved = dl[j + 1 - q] * term;
            }
            bsp1[j + 1] = saved;
        }
    }
    // Modules.f90:98-108: dbsp(j) = (k-1) (Aind(jp,1) bspp(j) - Aind(jp,2) bspp(j+1)), bspp(j+1) = bsp1(j), bspp(1) = bspp(k+1) = 0,
    // Aind = 0 outside 1 .. nfun
#pragma unroll
    for (int j = 1; j <= k; ++j) {
        const int jp = j + (left - k);
        double A1 = 0.0, A2 = 0.0;
        if (jp >= 1 && jp <= nfun) { A1 = aind[jp - 1]; A2 = aind[nfun + jp - 1]; }
        const double b1 = (j >= 2) ? bsp1[j - 1] : 0.0;
        const double b2 = (j <= k - 1) ? bsp1[j] : 0.0;
        tab[(size_t)(j - 1) * npts + ip] = bsp[j];
        tab[(size_t)(k + j - 1) * npts + ip] = (double)(k - 1) * (A1 * b1 - A2 * b2);
    }
    tleft[ip] = left;
}

// ---- quadrature grid: rows of the assembly's point table (2k + 3 doubles each, assemble.hip) -----------------------------
__global__ __launch_bounds__(WF_TPB) void basis_gather_kernel(int k, int npts, const int *__restrict__ rows,
                                                              const double *__restrict__ ptab, const int *__restrict__ pleft,
                                                              double *__restrict__ tab, int *__restrict__ tleft)
{
    const int ip = blockIdx.x * WF_TPB + threadIdx.x;
    if (ip >= npts) return;
    const int row = rows[ip];
    const double *e = ptab + (size_t)row * (2 * k + 3);
    for (int j = 0; j < 2 * k; ++j) tab[(size_t)j * npts + ip] = e[j];
    tleft[ip] = pleft[row];
}

// ---- the sums -------------------------------------------------------------------------------------------------------------
template <int K, bool DERIV, bool EDGE>
__device__ __forceinline__ void wf_vectors(int nfun, int npts, int ip, int j0, int v0, int v1, const double (&B)[K],
                                           const double (&D)[K], const double *__restrict__ Z, double *__restrict__ U,
                                           double *__restrict__ dU)
{
    for (int v = v0; v < v1; ++v) {
        const double *c = Z + (size_t)v * nfun;
        double s = 0.0, d = 0.0;
#pragma unroll
        for (int jf = 0; jf < K; ++jf) {
            const int j = j0 + jf;                                   // 0-based function index
            double cj;
            if (EDGE) cj = (j >= 0 && j < nfun) ? c[j] : 0.0;        // coefficients outside 1 .. nfun are zero
            else cj = c[j];
            s = s + cj * B[jf];
            if (DERIV) d = d + cj * D[jf];
        }
        const size_t o = (size_t)v * npts + ip;
        U[o] = s;
        if (DERIV) dU[o] = d;
    }
}

constexpr int WF_WIN = 64;    // widest coefficient window (functions) of a point tile that is staged in LDS

template <int K, bool DERIV>
__global__ __launch_bounds__(WF_TPB) void tabulate_kernel(int nfun, int npts, int nvec, int vt, const double *__restrict__ tab,
                                                          const int *__restrict__ tleft, const double *__restrict__ Z,
                                                          double *__restrict__ U, double *__restrict__ dU)
{
    __shared__ double cw[WF_VT][WF_WIN];
    __shared__ int lrange[2];
    const int ip = blockIdx.x * WF_TPB + threadIdx.x;
    const bool live = ip < npts;
    double B[K], D[K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
        B[j] = live ? tab[(size_t)j * npts + ip] : 0.0;
        D[j] = (DERIV && live) ? tab[(size_t)(K + j) * npts + ip] : 0.0;
    }
    const int left = live ? tleft[ip] : 0;
    const int j0 = left - K;
    const int v0 = blockIdx.y * vt;
    const int v1 = (nvec - v0 < vt) ? nvec : v0 + vt;
    // the tile's range of `left`: sorted points (the quadrature grid) span a few knot intervals, and the K-wide coefficient windows
    // of the tile's vectors are then staged in LDS once (zero outside 1 .. nfun) instead of being fetched by every lane
    if (threadIdx.x == 0) { lrange[0] = 0x7fffffff; lrange[1] = 0; }
    __syncthreads();
    if (live) { atomicMin(&lrange[0], left); atomicMax(&lrange[1], left); }
    __syncthreads();
    const int lo = lrange[0] - K, span = lrange[1] - lrange[0] + K;       // functions lo .. lo + span - 1 (0-based)
    if (span > WF_WIN) {                                                   // scattered points: every lane reads its own window
        if (!live) return;
        if (j0 >= 0 && j0 + K <= nfun) wf_vectors<K, DERIV, false>(nfun, npts, ip, j0, v0, v1, B, D, Z, U, dU);
        else wf_vectors<K, DERIV, true>(nfun, npts, ip, j0, v0, v1, B, D, Z, U, dU);
        return;
    }
    const int off = live ? j0 - lo : 0;
    for (int vb = v0; vb < v1; vb += WF_VT) {
        const int nv = (v1 - vb < WF_VT) ? v1 - vb : WF_VT;
        __syncthreads();                                                   // the previous chunk has been read
        for (int idx = threadIdx.x; idx < nv * span; idx += WF_TPB) {
            const int vv = idx / span, q = idx - vv * span, j = lo + q;
            cw[vv][q] = (j >= 0 && j < nfun) ? Z[(size_t)(vb + vv) * nfun + j] : 0.0;
        }
        __syncthreads();
        if (live) {
            for (int vv = 0; vv < nv; ++vv) {
                const double *c = &cw[vv][off];
                double s = 0.0, d = 0.0;
#pragma unroll
                for (int jf = 0; jf < K; ++jf) {
                    const double cj = c[jf];
                    s = s + cj * B[jf];
                    if (DERIV) d = d + cj * D[jf];
                }
                const size_t o = (size_t)(vb + vv) * npts + ip;
                U[o] = s;
                if (DERIV) dU[o] = d;
            }
        }
    }
}

// ---- launchers ----------------------------------------------------------------------------------------------------------------
#define WF_ALL_K(M) M(1) M(2) M(3) M(4) M(5) M(6) M(7) M(8) M(9) M(10) M(11) M(12) M(13) M(14) M(15) M(16)

int launch_basis_table(int nkp, int k, int nfun, int npts, const double *d_rt, const double *d_aind, const double *d_r, double *d_tab,
                       int *d_tleft, int *d_status, hipStream_t st)
{
    if (k > 16 || k < 1 || npts < 1) return BSP_ERR_ARG;
    const dim3 grid((npts + WF_TPB - 1) / WF_TPB), block(WF_TPB);
    switch (k) {
#define WF_CASE(K) case K: hipLaunchKernelGGL(basis_table_kernel<K>, grid, block, 0, st, nkp, nfun, npts, d_rt, d_aind, d_r, d_tab, d_tleft, d_status); break;
        WF_ALL_K(WF_CASE)
#undef WF_CASE
    }
    BSP_HIP(hipGetLastError());
    return BSP_OK;
}

int launch_basis_gather(int k, int npts, const int *d_rows, const double *d_ptab, const int *d_pleft, double *d_tab, int *d_tleft,
                        hipStream_t st)
{
    if (npts < 1) return BSP_ERR_ARG;
    hipLaunchKernelGGL(basis_gather_kernel, dim3((npts + WF_TPB - 1) / WF_TPB), dim3(WF_TPB), 0, st, k, npts, d_rows, d_ptab, d_pleft,
                       d_tab, d_tleft);
    BSP_HIP(hipGetLastError());
    return BSP_OK;
}

// U[v * npts + ip], dU likewise (d_dU null: values only) for the nvec vectors Z[v * nfun + j]
int launch_tabulate(int k, int nfun, int npts, int nvec, const double *d_tab, const int *d_tleft, const double *d_Z, double *d_U,
                    double *d_dU, hipStream_t st)
{
    if (k > 16 || k < 1 || npts < 1 || nvec < 1) return BSP_ERR_ARG;
    int vt = WF_VT;
    if ((nvec + vt - 1) / vt > 65535) vt = (nvec + 65534) / 65535;          // grid.y limit
    const dim3 grid((npts + WF_TPB - 1) / WF_TPB, (nvec + vt - 1) / vt), block(WF_TPB);
    switch (k) {
#define WF_CASE(K)                                                                                                                   \
    case K:                                                                                                                          \
        if (d_dU) hipLaunchKernelGGL((tabulate_kernel<K, true>), grid, block, 0, st, nfun, npts, nvec, vt, d_tab, d_tleft, d_Z, d_U, d_dU); \
        else hipLaunchKernelGGL((tabulate_kernel<K, false>), grid, block, 0, st, nfun, npts, nvec, vt, d_tab, d_tleft, d_Z, d_U, d_dU);     \
        break;
        WF_ALL_K(WF_CASE)
#undef WF_CASE
    }
    BSP_HIP(hipGetLastError());
    return BSP_OK;
}

}  // namespace bsp
