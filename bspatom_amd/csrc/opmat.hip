// opmat.hip -- matrix elements of caller-given radial operators g(r) and g(r) d/dr (bspatom_operator_bands / _matrix).
//
// The general case of the rij that MATRIX_SVT keeps: for KIND_PI >= 3 the reference assembles zAij (matrices.f90:114-139, 165-171),
// for every tabulated profile zIth(ibet, igl, ...) the sums  fbra * g(r_q) * fket * dr  and  fbra * g(r_q) * dfket * dr  over the
// Gauss-Legendre points, g known by its values on those points alone.  Two kernels:
//   operator_band_kernel       G_o(i, j) = sum_q B_i(r_q) g_o(q) X_j(r_q) w_q, X = B or B', full band, for blocks of operators
//   band_combine_apply_kernel  W = (sum_o a_o G_o) x for every initial vector of a group of pairs
// and the contraction D = W Z^T is dipole.hip's.  The arithmetic is fixed and nothing else: this file is compiled with
// -ffp-contract=off (no FMA), a band entry is one accumulator from 0.0 over intervals ascending and points ascending (the
// intervals common to both functions, matrices.f90:71-72), each term ((fbra * g) * x) * dr with fbra, fket, dfket, dr from the
// assembly's point table -- so with g = r, 1/r, 1 the bands are dipole_band_kernel's bit for bit, and an operator's band does
// not depend on the other operators of the call.
#include "common.h"

namespace bsp {

constexpr int OPB = 8;          // operators per item of operator_band_kernel (register block); gridDim.y chunks the rest
constexpr int OP_KMAX = 16;     // B-spline order limit (BSPATOM_MAX_K)

// Staging and items as dipole_band_kernel (assemble.hip): a workgroup owns TI rows, stages the point-table rows of its
// TI+k-1 intervals, a thread owns (row, diagonal) items.  Beside the table: gs[point][OPB], the g values of this workgroup's
// operators at the staged points (0.0 beyond nop), and qf[interval], the quadrature index of the interval's first point or
// -1 for an interval of zero width -- those carry no g value and are skipped (their terms are +-0.0 in dipole_band_kernel:
// dr = 0).  A thread reads fbra, fket, dfket, dr of a point once and updates its OPB accumulators; g multiplies in the middle
// of the product, so nothing of a term is shared between operators.
__global__ __launch_bounds__(256) void operator_band_kernel(int TI, int nfun, int k, int ka, int nkp, int nop, int nr, int o_base,
                                                           const double *__restrict__ ptab, const int *__restrict__ leftv,
                                                           const int *__restrict__ qfirst, const double *__restrict__ g,
                                                           const int *__restrict__ deriv, double *__restrict__ GB)
{
    extern __shared__ double sm[];
    const int W = 2 * k + 3, nd = 2 * k - 1;
    const int i0 = blockIdx.x * TI;
    const int ib0 = i0 + 1;
    const int o0 = o_base + blockIdx.y * OPB;
    const int on = (nop - o0 < OPB) ? (nop - o0) : OPB;
    int nint = TI + k - 1;
    if (ib0 + nint - 1 > nkp - 1) nint = nkp - 1 - ib0 + 1;
    const int npts = nint * ka, cap = (TI + k - 1) * ka;
    double *tab = sm;                                         // [cap][W]
    double *gs = sm + (size_t)cap * W;                        // [cap][OPB]
    int *lf = reinterpret_cast<int *>(gs + (size_t)cap * OPB); // [cap]
    int *qf = lf + cap;                                       // [TI + k - 1]
    for (int idx = threadIdx.x; idx < npts * W; idx += blockDim.x)
        tab[idx] = ptab[(size_t)(ib0 - 1) * ka * W + idx];
    for (int idx = threadIdx.x; idx < npts; idx += blockDim.x) lf[idx] = leftv[(ib0 - 1) * ka + idx];
    for (int idx = threadIdx.x; idx < nint; idx += blockDim.x) qf[idx] = qfirst[ib0 - 1 + idx];
    for (int idx = threadIdx.x; idx < npts * OPB; idx += blockDim.x) {
        const int u = idx / npts, pt = idx - u * npts;
        const int t = pt / ka, q = qfirst[ib0 - 1 + t];
        double v = 0.0;
        if (q >= 0 && u < on) v = g[(size_t)(o0 + u) * nr + q + (pt - t * ka)];
        gs[(size_t)pt * OPB + u] = v;
    }
    unsigned dm = 0;                                          // bit u: operator o0 + u takes B_j'
    for (int u = 0; u < on; ++u)
        if (deriv[o0 + u]) dm |= 1u << u;
    __syncthreads();
    const int nrow = (nfun - i0 < TI) ? (nfun - i0) : TI;
    for (int it = threadIdx.x; it < TI * nd; it += blockDim.x) {
        const int ii = it % TI, dd = it / TI, d = dd - (k - 1);
        if (ii >= nrow) continue;
        const int ibra = i0 + ii + 1, jket = ibra + d;        // 1-based
        double acc[OPB];
#pragma unroll
        for (int u = 0; u < OPB; ++u) acc[u] = 0.0;
        if (jket >= 1 && jket <= nfun) {
            const int ibetmin = ibra > jket ? ibra : jket;                    // matrices.f90:71
            int ibetmax = (ibra < jket ? ibra : jket) + k - 1;                // :72
            if (ibetmax > ib0 + nint - 1) ibetmax = ib0 + nint - 1;           // never for a valid knot sequence: the staged range
            for (int ibet = ibetmin; ibet <= ibetmax; ++ibet) {
                const int t = ibet - ib0;
                if (qf[t] < 0) continue;
                const double *eb = tab + (size_t)t * ka * W;
                const double *gb = gs + (size_t)t * ka * OPB;
                const int *lb = lf + t * ka;
                for (int gp = 0; gp < ka; ++gp) {
                    const double *e = eb + gp * W;
                    const int left = lb[gp];
                    int ifun = ibra - (left - k), jfun = jket - (left - k);
                    ifun = ifun < 1 ? 1 : (ifun > k ? k : ifun);
                    jfun = jfun < 1 ? 1 : (jfun > k ? k : jfun);
                    const double fbra = e[ifun - 1], fket = e[jfun - 1], dfket = e[k + jfun - 1];
                    const double dr = e[2 * k + 1];
                    const double *gv = gb + gp * OPB;
#pragma unroll
                    for (int u = 0; u < OPB; ++u) {
                        const double x = ((dm >> u) & 1u) ? dfket : fket;
                        acc[u] = acc[u] + ((fbra * gv[u]) * x) * dr;          // zAij, matrices.f90:114-139
                    }
                }
            }
        }
#pragma unroll
        for (int u = 0; u < OPB; ++u)
            if (u < on) GB[((size_t)(o0 + u) * nd + dd) * nfun + (ibra - 1)] = acc[u];
    }
}

// d_qfirst[nkp - 1]: quadrature index of the first point of every knot interval, -1 for zero width; d_g[nop][nr]; d_deriv[nop];
// d_GB[nop][2k-1][nfun].  TI as launch_dipole_bands chooses it, the g block counted in.
int launch_operator_bands(int nfun, int k, int ka, int nkp, int nop, int nr, const double *d_ptab, const int *d_left,
                          const int *d_qfirst, const double *d_g, const int *d_deriv, double *d_GB, hipStream_t st)
{
    if (nop < 1 || nr < 1 || k < 2 || k > OP_KMAX) return BSP_ERR_ARG;
    const int W = 2 * k + 3;
    int TI = 32;
    size_t lds = 0;
    for (; TI >= 4; TI /= 2) {
        const size_t cap = (size_t)(TI + k - 1) * ka;
        lds = cap * (W + OPB) * sizeof(double) + cap * sizeof(int) + (size_t)(TI + k - 1) * sizeof(int);
        if (lds <= 150 * 1024) break;
    }
    if (TI < 4) return BSP_ERR_UNSUPPORTED;
    static bool attr = false;
    if (!attr) {
        BSP_HIP(allow_lds(operator_band_kernel, 150 * 1024));
        attr = true;
    }
    KScope ks(KS_OPBAND, st);
    const int chunks = (nop + OPB - 1) / OPB, ymax = 65535;
    for (int c = 0; c < chunks; c += ymax) {
        const int ny = chunks - c < ymax ? chunks - c : ymax;
        hipLaunchKernelGGL(operator_band_kernel, dim3((nfun + TI - 1) / TI, ny), dim3(256), lds, st, TI, nfun, k, ka, nkp, nop, nr,
                           c * OPB, d_ptab, d_left, d_qfirst, d_g, d_deriv, d_GB);
        BSP_HIP(hipGetLastError());
    }
    return BSP_OK;
}

// ---- W[q][j][:] = A_q x_j,  A_q = sum_o a[q][o] G_o ---------------------------------------------------------------------
// band_apply_block_kernel (dipole.hip) with nop coefficients per item.  A workgroup owns 256 rows of one item and CA_JV of its
// vectors: a thread forms the 2k-1 entries of its row of A_q once -- s = a_0 G_0, then s = s + a_o G_o for o ascending -- keeps
// them in its own column of LDS, and applies them to each vector over diagonals ascending, columns outside 0 .. n-1 skipped.
// No FMA, and nothing of a row depends on which vectors share the workgroup.
constexpr int CA_JV = 16;
__global__ __launch_bounds__(256) void band_combine_apply_kernel(int n, int k, int nop, int count, int nblk, int nvc,
                                                                const double *__restrict__ GB, const double *__restrict__ acoef,
                                                                const long long *__restrict__ xoff, const double *__restrict__ base,
                                                                double *__restrict__ W)
{
    __shared__ double As[(2 * OP_KMAX - 1) * 256];
    int b = blockIdx.x;
    const int rb = b % nblk; b /= nblk;
    const int vc = b % nvc, q = b / nvc;
    const int i = rb * 256 + threadIdx.x;
    if (i >= n) return;
    const int nd = 2 * k - 1;
    const size_t cs = (size_t)nd * n;
    const double *ac = acoef + (size_t)q * nop;
    for (int dd = 0; dd < nd; ++dd) {
        const size_t idx = (size_t)dd * n + i;
        double s = ac[0] * GB[idx];
        for (int o = 1; o < nop; ++o) s = s + ac[o] * GB[(size_t)o * cs + idx];
        As[dd * 256 + threadIdx.x] = s;
    }
    const int j1 = (vc + 1) * CA_JV < count ? (vc + 1) * CA_JV : count;
    for (int jv = vc * CA_JV; jv < j1; ++jv) {
        const double *x = base + xoff[q] + (size_t)jv * n;
        double s = 0.0;
        for (int d = -(k - 1); d <= k - 1; ++d) {
            const int j = i + d;
            if (j < 0 || j >= n) continue;
            s = s + As[(d + k - 1) * 256 + threadIdx.x] * x[j];
        }
        W[((size_t)q * count + jv) * n + i] = s;
    }
}

int launch_band_combine_apply(int n, int k, int nop, int count, int nitems, const double *d_GB, const double *d_acoef,
                              const long long *d_xoff, const double *d_base, double *d_W, hipStream_t st)
{
    if (n < 1 || k < 1 || k > OP_KMAX || nop < 1 || count < 1 || nitems < 1) return BSP_ERR_ARG;
    const int nblk = (n + 255) / 256, nvc = (count + CA_JV - 1) / CA_JV;
    const long long grid = (long long)nblk * nvc * nitems;
    if (grid > 0x7fffffffLL) return BSP_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(band_combine_apply_kernel, dim3((unsigned)grid), dim3(256), 0, st, n, k, nop, count, nblk, nvc, d_GB, d_acoef,
                       d_xoff, d_base, d_W);
    BSP_HIP(hipGetLastError());
    return BSP_OK;
}

}  // namespace bsp
