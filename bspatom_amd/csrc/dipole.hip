// dipole.hip -- dipole matrix blocks between eigenvector windows of many channel pairs (bspatom_dipole_matrix):
//   D_p[i][f] = z_f^T (a0 R_r + a1 R_{1/r} + a2 R_{d/dr}) x_i,   x_i: initial window of pair p, z_f: its final window.
// The reference's unit of work is "all states of two channels" (matrices.f90:331 keeps ctemp(:,1:ntemp,l); PhotoIon.f90:95-107
// runs DGEMV + DDOT over it).  Two kernels per group of pairs: W = A x for every initial vector (VALU, banded), then
// D = W Z^T on the matrix cores with K = n cut into slices by a rule in (n, count_ini, count_fin) alone.
#include "common.h"
#include "mfma_tile.h"

namespace bsp {

// ---- W[q][j][:] = A_q x_j --------------------------------------------------------------------------------------------
// Item q = (operator a[3q .. 3q+2], initial block at base + xoff[q]); one thread per row of one vector, one launch for all
// items of a group.  Per row the expression and the order of band_apply_kernel (eigvec.hip): (a0 RB + a1 RB1) + a2 RB2,
// diagonals ascending, columns outside 0 .. n-1 skipped -- every column of W has the bits bspatom_dipole_elements forms.
__global__ __launch_bounds__(256) void band_apply_block_kernel(int n, int k, int count, int nblk, const double *__restrict__ RB,
                                                              const double *__restrict__ acoef, const long long *__restrict__ xoff,
                                                              const double *__restrict__ base, double *__restrict__ W)
{
    const int rb = blockIdx.x % nblk, vj = blockIdx.x / nblk;       // vj = q * count + j
    const int q = vj / count, j0 = vj - q * count;
    const int i = rb * 256 + threadIdx.x;
    if (i >= n) return;
    const double a0 = acoef[3 * q], a1 = acoef[3 * q + 1], a2 = acoef[3 * q + 2];
    const double *x = base + xoff[q] + (size_t)j0 * n;
    double *v = W + (size_t)vj * n;
    const size_t cs = (size_t)(2 * k - 1) * n;
    double s = 0.0;
    for (int d = -(k - 1); d <= k - 1; ++d) {
        const int j = i + d;
        if (j < 0 || j >= n) continue;
        const size_t idx = (size_t)(d + k - 1) * n + i;
        const double a = (a0 * RB[idx] + a1 * RB[cs + idx]) + a2 * RB[2 * cs + idx];
        s += a * x[j];
    }
    v[i] = s;
}

int launch_band_apply_block(int n, int k, int count, int nitems, const double *d_RB, const double *d_acoef, const long long *d_xoff,
                            const double *d_base, double *d_W, hipStream_t st)
{
    if (n < 1 || k < 1 || count < 1 || nitems < 1) return BSP_ERR_ARG;
    const int nblk = (n + 255) / 256;
    const long long grid = (long long)nblk * count * nitems;
    if (grid > 0x7fffffffLL) return BSP_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(band_apply_block_kernel, dim3((unsigned)grid), dim3(256), 0, st, n, k, count, nblk, d_RB, d_acoef, d_xoff, d_base, d_W);
    BSP_HIP(hipGetLastError());
    return BSP_OK;
}

// ---- D_p = W_p Z_p^T ---------------------------------------------------------------------------------------------------
// K slices of a (n, count_ini, count_fin) product: as many as bring one pair's grid to ~64 workgroups, none shorter than 256;
// the batch (pairs, groups) never enters, so a pair's bits do not depend on its company (the tsqr_max_m principle).
void dipole_kslices(int n, int count_ini, int count_fin, int *chunk, int *nslices)
{
    const long tiles = (long)((count_ini + 63) / 64) * ((count_fin + 63) / 64);
    long s = (64 + tiles - 1) / tiles;
    const long smax = n / 256 > 1 ? n / 256 : 1;
    if (s > smax) s = smax;
    int c = (int)((n + s - 1) / s);
    c = (c + 15) / 16 * 16;
    *chunk = c;
    *nslices = (n + c - 1) / c;
}

// Both operands are rows contiguous along K (vectors are stored [vector][n]): W[i][:] on the MFMA's row axis, Z[f][:] on its
// lane-fast column axis, so the 16 lanes of a DPP row store 16 consecutive f of one row of D.  One workgroup = one 64 x 64 tile
// of one pair over one K slice; 4 waves as 2 x 2, each 32 x 32 (2 x 2 MFMA tiles).  The staged tiles take the column permutation
// of gemm_f64.hip (lds_swz): a K-contiguous operand puts the lanes of a 16-lane group on rows k, k + 2, .. of one column.
// V2: n is even, every row starts on 16 bytes: double2 loads along k (K slices are multiples of 16 long); else 8-byte loads.
// The loads of step t + 1 are in registers before the MFMAs of step t.
constexpr int DBK = 16, DBT = 64, DLD = DBT + 16;

template <bool V2>
struct DipRegs { double v[V2 ? 2 * (DBT * DBK / 2 / 256) : DBT * DBK / 256]; };

template <bool V2>
__device__ __forceinline__ void dip_load(DipRegs<V2> &r, const double *__restrict__ X, int rows, int r0, int n, int k0, int kend, int tid)
{
    if (V2) {
#pragma unroll
        for (int it = 0; it < DBT * DBK / 2 / 256; ++it) {
            const int idx = tid + it * 256;
            const int mm = idx / (DBK / 2), kk = (idx % (DBK / 2)) * 2;
            const int gm = r0 + mm, gk = k0 + kk;
            const bool ok = (gm < rows) && (gk + 1 < kend);
            // unconditional load from a clamped address, the value selected afterwards (a branch around a load serialises them)
            const double2 v = *reinterpret_cast<const double2 *>(X + (ok ? ((size_t)gm * n + gk) : 0));
            r.v[2 * it] = ok ? v.x : 0.0;
            r.v[2 * it + 1] = ok ? v.y : 0.0;
        }
    } else {
#pragma unroll
        for (int it = 0; it < DBT * DBK / 256; ++it) {
            const int idx = tid + it * 256;
            const int mm = idx / DBK, kk = idx % DBK;
            const int gm = r0 + mm, gk = k0 + kk;
            const bool ok = (gm < rows) && (gk < kend);
            const double v = X[ok ? ((size_t)gm * n + gk) : 0];
            r.v[it] = ok ? v : 0.0;
        }
    }
}

template <bool V2>
__device__ __forceinline__ void dip_store(const DipRegs<V2> &r, double *Xs, int tid)
{
    if (V2) {
#pragma unroll
        for (int it = 0; it < DBT * DBK / 2 / 256; ++it) {
            const int idx = tid + it * 256;
            const int mm = idx / (DBK / 2), kk = (idx % (DBK / 2)) * 2;
            Xs[kk * DLD + (mm ^ lds_swz(kk))] = r.v[2 * it];
            Xs[(kk + 1) * DLD + (mm ^ lds_swz(kk))] = r.v[2 * it + 1];         // kk is even: the same offset
        }
    } else {
#pragma unroll
        for (int it = 0; it < DBT * DBK / 256; ++it) {
            const int idx = tid + it * 256;
            const int mm = idx / DBK, kk = idx % DBK;
            Xs[kk * DLD + (mm ^ lds_swz(kk))] = r.v[it];
        }
    }
}

// pw[2p], pw[2p+1]: offsets (doubles from base) of pair p's W block [count_ini][n] and final block [count_fin][n].
// out: pair p, slice s at out + (p * ns + s) * count_ini * count_fin, row-major [count_ini][count_fin].
template <bool V2>
__global__ __launch_bounds__(256) void dipole_block_kernel(int n, int ci, int cf, int tm, int tn, int ns, int chunk,
                                                          const long long *__restrict__ pw, const double *__restrict__ base,
                                                          double *__restrict__ out)
{
    __shared__ double As[DBK * DLD];
    __shared__ double Bs[DBK * DLD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    int b = blockIdx.x;
    const int s = b % ns; b /= ns;
    const int jn = b % tn; b /= tn;
    const int im = b % tm;
    const int p = b / tm;
    const double *Wp = base + pw[2 * p], *Zp = base + pw[2 * p + 1];
    const int m0 = im * DBT, n0 = jn * DBT;
    const int kbeg = s * chunk, kend = (kbeg + chunk < n) ? kbeg + chunk : n;

    double4_t acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = (double4_t){0.0, 0.0, 0.0, 0.0};

    DipRegs<V2> ra, rb;
    dip_load<V2>(ra, Wp, ci, m0, n, kbeg, kend, tid);
    dip_load<V2>(rb, Zp, cf, n0, n, kbeg, kend, tid);
    for (int k0 = kbeg; k0 < kend; k0 += DBK) {
        dip_store<V2>(ra, As, tid);
        dip_store<V2>(rb, Bs, tid);
        __syncthreads();
        if (k0 + DBK < kend) {
            dip_load<V2>(ra, Wp, ci, m0, n, k0 + DBK, kend, tid);
            dip_load<V2>(rb, Zp, cf, n0, n, k0 + DBK, kend, tid);
        }
#pragma unroll
        for (int k4 = 0; k4 < DBK / 4; ++k4) {
            const int kr = k4 * 4 + (lane >> 4);
            mfma_step<2, 2>(&As[kr * DLD + wm * 32], &Bs[kr * DLD + wn * 32], lane, kr, acc);
        }
        __syncthreads();
    }

    double *C = out + ((size_t)p * ns + s) * ((size_t)ci * cf);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int gi = m0 + wm * 32 + i * 16 + (lane >> 4) + 4 * r;
                const int gj = n0 + wn * 32 + j * 16 + (lane & 15);
                if (gi < ci && gj < cf) C[(size_t)gi * cf + gj] = acc[i][j][r];
            }
}

// D[p][idx] = sum over the K slices, in slice order
__global__ __launch_bounds__(256) void dipole_reduce_kernel(const double *__restrict__ part, int ns, long long mn, long long total,
                                                           double *__restrict__ D)
{
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long long)gridDim.x * 256) {
        const long long p = t / mn, idx = t - p * mn;
        const double *q = part + (size_t)p * ns * mn + idx;
        double s = 0.0;
        for (int i = 0; i < ns; ++i) s += q[(size_t)i * mn];
        D[t] = s;
    }
}

// npairs products on one grid: d_out row-major [npairs][count_ini][count_fin]; d_part (npairs * nslices * count_ini * count_fin
// doubles) is used when dipole_kslices gives more than one slice
int launch_dipole_block(int n, int count_ini, int count_fin, int npairs, const long long *d_pw, const double *d_base, double *d_part,
                        double *d_out, hipStream_t st)
{
    if (n < 1 || count_ini < 1 || count_fin < 1 || npairs < 1) return BSP_ERR_ARG;
    int chunk, ns;
    dipole_kslices(n, count_ini, count_fin, &chunk, &ns);
    if (ns > 1 && !d_part) return BSP_ERR_ARG;
    const int tm = (count_ini + DBT - 1) / DBT, tn = (count_fin + DBT - 1) / DBT;
    const long long grid = (long long)npairs * tm * tn * ns;
    if (grid > 0x7fffffffLL) return BSP_ERR_UNSUPPORTED;
    double *out = ns > 1 ? d_part : d_out;
    if (n % 2 == 0)
        hipLaunchKernelGGL(dipole_block_kernel<true>, dim3((unsigned)grid), dim3(256), 0, st, n, count_ini, count_fin, tm, tn, ns, chunk, d_pw, d_base, out);
    else
        hipLaunchKernelGGL(dipole_block_kernel<false>, dim3((unsigned)grid), dim3(256), 0, st, n, count_ini, count_fin, tm, tn, ns, chunk, d_pw, d_base, out);
    BSP_HIP(hipGetLastError());
    if (ns > 1) {
        const long long mn = (long long)count_ini * count_fin, total = mn * npairs;
        const long long blocks = (total + 255) / 256;
        hipLaunchKernelGGL(dipole_reduce_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, st, d_part, ns, mn, total, d_out);
        BSP_HIP(hipGetLastError());
    }
    return BSP_OK;
}

}  // namespace bsp
