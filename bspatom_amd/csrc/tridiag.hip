// tridiag.hip -- all eigenvalues of the symmetric tridiagonal matrices by Sturm-sequence bisection.
// Replaces DSTEQR/DSTERF inside DSYEV/DSYGV (reference call matrices.f90:248).  Batched over the
// l-channels: grid = (ceil(n/256), batch); thread m of a channel brackets eigenvalue m (0-based,
// ascending, like LAPACK's w) and bisects until the bracket cannot shrink.  d and e^2 of the
// channel are staged in LDS (2 x 8 B x n; n <= 8192 -> 128 KiB) and every thread of the
// workgroup walks them in lock-step, so each LDS read is a broadcast.
//
// count(x) = #{eigenvalues < x} from the LDL^T pivots q_i = (d_i - x) - e_{i-1}^2 / q_{i-1}
// (LAPACK dstebz/dlaebz recurrence with the pivmin safeguard).
#include <algorithm>
#include <vector>
#include "common.h"
#include "wave_ops.h"

namespace bsp {

__device__ __forceinline__ int sturm_count(const double *__restrict__ d, const double *__restrict__ e2,
                                           int n, double x, double pivmin)
{
    double q = d[0] - x;
    if (fabs(q) < pivmin) q = -pivmin;
    int cnt = (q < 0.0) ? 1 : 0;
    for (int i = 1; i < n; ++i) {
        q = (d[i] - x) - e2[i - 1] / q;
        if (fabs(q) < pivmin) q = -pivmin;
        cnt += (q < 0.0) ? 1 : 0;
    }
    return cnt;
}

// EPT eigenvalues per thread: EPT independent Sturm recurrences share every LDS read of (d_i, e_i^2)
// and hide each other's latency (the recurrence is one long dependent chain per shift).
// The quotient e^2/q uses v_rcp_f64 refined by one Newton step (error a few ulp): only the SIGN of
// each pivot enters the count, and a relative perturbation of e_i^2 of a few ulp moves every
// eigenvalue by at most a few ulp of |T| -- the same bound plain bisection has.
constexpr int EPT = 4;

__global__ __launch_bounds__(256) void bisect_kernel(int n, int ldn, const double *__restrict__ dall,
                                                    const double *__restrict__ eall, double *wall, long ldw)
{
    extern __shared__ double sm[];
    double *d = sm, *e2 = sm + n;
    __shared__ double red[8];
    const int tid = threadIdx.x;
    const size_t ch = blockIdx.y;
    const double *dg = dall + ch * (size_t)ldn, *eg = eall + ch * (size_t)ldn;
    double gl = 1e300, gu = -1e300, emax = 0.0;
    for (int i = tid; i < n; i += 256) {
        const double di = dg[i];
        const double el = (i > 0) ? fabs(eg[i - 1]) : 0.0;
        const double er = (i < n - 1) ? fabs(eg[i]) : 0.0;
        d[i] = di;
        e2[i] = (i < n - 1) ? eg[i] * eg[i] : 0.0;
        gl = fmin(gl, di - el - er);
        gu = fmax(gu, di + el + er);
        emax = fmax(emax, er * er);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        gl = fmin(gl, __shfl_xor(gl, off));
        gu = fmax(gu, __shfl_xor(gu, off));
        emax = fmax(emax, __shfl_xor(emax, off));
    }
    if ((tid & 63) == 0) { red[tid >> 6] = gl; red[4 + (tid >> 6)] = gu; }
    __syncthreads();
    gl = fmin(fmin(red[0], red[1]), fmin(red[2], red[3]));
    gu = fmax(fmax(red[4], red[5]), fmax(red[6], red[7]));
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = emax;
    __syncthreads();
    emax = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
    const double safmin = 2.2250738585072014e-308;
    const double pivmin = safmin * fmax(1.0, emax);
    const double tnorm = fmax(fabs(gl), fabs(gu));
    const double eps = 2.220446049250313e-16;
    gl = gl - 2.1 * tnorm * eps * n - 2.1 * pivmin;
    gu = gu + 2.1 * tnorm * eps * n + 2.1 * pivmin;

    const int mbase = blockIdx.x * (256 * EPT) + tid;      // eigenvalue indices mbase + 256 c
    double lo[EPT], hi[EPT];
#pragma unroll
    for (int c = 0; c < EPT; ++c) { lo[c] = gl; hi[c] = gu; }
    for (int it = 0; it < 128; ++it) {
        double mid[EPT];
        bool done[EPT];
        bool alld = true;
#pragma unroll
        for (int c = 0; c < EPT; ++c) {
            mid[c] = 0.5 * (lo[c] + hi[c]);
            done[c] = (mid[c] <= lo[c]) || (mid[c] >= hi[c]) ||
                      (hi[c] - lo[c] <= 2.0 * eps * fmax(fabs(lo[c]), fabs(hi[c])) + 2.0 * pivmin);
            alld = alld && done[c];
        }
        if (__syncthreads_and(alld)) break;
        double q[EPT];
        int cnt[EPT];
        {
            const double d0 = d[0];
#pragma unroll
            for (int c = 0; c < EPT; ++c) {
                q[c] = d0 - mid[c];
                if (fabs(q[c]) < pivmin) q[c] = -pivmin;
                cnt[c] = (q[c] < 0.0) ? 1 : 0;
            }
        }
        for (int i = 1; i < n; ++i) {
            const double di = d[i], ei = e2[i - 1];
#pragma unroll
            for (int c = 0; c < EPT; ++c) {
                double r = __builtin_amdgcn_rcp(q[c]);
                r = r * (2.0 - q[c] * r);                   // one Newton step
                q[c] = (di - mid[c]) - ei * r;
                if (fabs(q[c]) < pivmin) q[c] = -pivmin;
                cnt[c] += (q[c] < 0.0) ? 1 : 0;
            }
        }
#pragma unroll
        for (int c = 0; c < EPT; ++c) {
            if (!done[c]) {
                if (cnt[c] > mbase + 256 * c) hi[c] = mid[c]; else lo[c] = mid[c];
            }
        }
    }
#pragma unroll
    for (int c = 0; c < EPT; ++c) {
        const int m = mbase + 256 * c;
        if (m < n) wall[ch * (size_t)ldw + m] = 0.5 * (lo[c] + hi[c]);
    }
}

// ------------------------------------------------------------------------------------------------
// Division-free Sturm count.  The pivot recurrence above spends most of its time in v_rcp_f64 + Newton; the
// characteristic-polynomial form  p_i = (d_i - x) p_{i-1} - e_{i-1}^2 p_{i-2}  needs a multiply, an FMA and the
// comparison of two sign bits: count(x) = number of sign changes in p_0 = 1, p_1, ..., p_n (q_i = p_i / p_{i-1}
// are the pivots above, so the two counts agree; an exact zero may take either sign because its successor
// -e^2 p_{i-2} is opposite to its predecessor).  Safeguards:
//   * the matrix is scaled by a power of two to norm <= 1 (exact), so a step changes |p| by a factor in
//     [eps, 3]: renormalising p_i, p_{i-1} by a common power of two every 8 steps excludes over- and underflow;
//   * e^2 is floored at 1e-60 (scaled units; moves no eigenvalue by more than 1e-30 |T|), so two successive
//     exact zeros -- the only way the recurrence can die -- are impossible;
//   * rows are padded to a multiple of 8 with decoupled 1 x 1 blocks d = 2 > every scaled eigenvalue.
constexpr int RS = 8;      // steps between renormalisations

__global__ __launch_bounds__(256) void bisect2_kernel(int n, int ldn, const double *__restrict__ dall,
                                                     const double *__restrict__ eall, double *wall, long ldw)
{
    extern __shared__ double sm[];
    const int np = (n + RS - 1) / RS * RS;             // padded length (steps 1 .. np, np a multiple of RS)
    double *d = sm, *e2 = sm + np + RS;
    __shared__ double red[8];
    const int tid = threadIdx.x;
    const size_t ch = blockIdx.y;
    const double *dg = dall + ch * (size_t)ldn, *eg = eall + ch * (size_t)ldn;
    double gl = 1e300, gu = -1e300;
    for (int i = tid; i < n; i += 256) {
        const double di = dg[i];
        const double el = (i > 0) ? fabs(eg[i - 1]) : 0.0;
        const double er = (i < n - 1) ? fabs(eg[i]) : 0.0;
        gl = fmin(gl, di - el - er);
        gu = fmax(gu, di + el + er);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        gl = fmin(gl, __shfl_xor(gl, off));
        gu = fmax(gu, __shfl_xor(gu, off));
    }
    if ((tid & 63) == 0) { red[tid >> 6] = gl; red[4 + (tid >> 6)] = gu; }
    __syncthreads();
    gl = fmin(fmin(red[0], red[1]), fmin(red[2], red[3]));
    gu = fmax(fmax(red[4], red[5]), fmax(red[6], red[7]));
    const double eps = 2.220446049250313e-16;
    double tnorm = fmax(fabs(gl), fabs(gu));
    if (!(tnorm > 0.0)) tnorm = 1.0;                   // the zero matrix
    int kexp;
    (void)frexp(tnorm, &kexp);                         // tnorm = f 2^kexp, f in [0.5, 1)
    const double sc = ldexp(1.0, -kexp), isc = ldexp(1.0, kexp);
    for (int i = tid; i < np + RS; i += 256) {
        // row i of the scaled matrix; e2[i] couples rows i and i+1.  Padding rows: d = 2, coupling at the floor.
        d[i] = (i < n) ? dg[i] * sc : 2.0;
        const double ev = (i < n - 1) ? (eg[i] * sc) : 0.0;
        e2[i] = fmax(ev * ev, 1e-60);
    }
    __syncthreads();
    gl = gl * sc - 2.1 * eps * n - 1e-300;             // scaled Gershgorin interval, widened as dstebz does
    gu = gu * sc + 2.1 * eps * n + 1e-300;

    const int mbase = blockIdx.x * (256 * EPT) + tid;      // eigenvalue indices mbase + 256 c
    double lo[EPT], hi[EPT];
#pragma unroll
    for (int c = 0; c < EPT; ++c) { lo[c] = gl; hi[c] = gu; }
    for (int it = 0; it < 128; ++it) {
        double mid[EPT];
        bool done[EPT];
        bool alld = true;
#pragma unroll
        for (int c = 0; c < EPT; ++c) {
            mid[c] = 0.5 * (lo[c] + hi[c]);
            done[c] = (mid[c] <= lo[c]) || (mid[c] >= hi[c]) ||
                      (hi[c] - lo[c] <= 2.0 * eps * fmax(fabs(lo[c]), fabs(hi[c])) + 1e-300);
            alld = alld && done[c];
        }
        if (__syncthreads_and(alld)) break;
        double p0[EPT], p1[EPT];
        int cnt[EPT];
#pragma unroll
        for (int c = 0; c < EPT; ++c) { p0[c] = 1.0; p1[c] = d[0] - mid[c]; cnt[c] = (p1[c] < 0.0) ? 1 : 0; }
        // rows 1 .. np-1 in blocks of RS (row 0 is done; the block that holds row 0 starts at row 1)
        for (int ib = 0; ib < np; ib += RS) {
#pragma unroll
            for (int r = 0; r < RS; ++r) {
                const int i = ib + r + 1;                  // rows 1 .. np (row np is padding too: arrays hold np + RS)
                const double di = d[i], ei = e2[i - 1];
#pragma unroll
                for (int c = 0; c < EPT; ++c) {
                    const double pn = __builtin_fma(di - mid[c], p1[c], -(ei * p0[c]));
                    cnt[c] += (int)((unsigned)(__double2hiint(pn) ^ __double2hiint(p1[c])) >> 31);
                    p0[c] = p1[c];
                    p1[c] = pn;
                }
            }
#pragma unroll
            for (int c = 0; c < EPT; ++c) {
                int ea, eb;
                (void)frexp(p1[c], &ea);
                (void)frexp(p0[c], &eb);
                const int ex = (p1[c] == 0.0) ? eb : ((p0[c] == 0.0) ? ea : max(ea, eb));
                p1[c] = ldexp(p1[c], -ex);
                p0[c] = ldexp(p0[c], -ex);
            }
        }
#pragma unroll
        for (int c = 0; c < EPT; ++c) {
            if (!done[c]) {
                if (cnt[c] > mbase + 256 * c) hi[c] = mid[c]; else lo[c] = mid[c];
            }
        }
    }
#pragma unroll
    for (int c = 0; c < EPT; ++c) {
        const int m = mbase + 256 * c;
        if (m < n) wall[ch * (size_t)ldw + m] = 0.5 * (lo[c] + hi[c]) * isc;
    }
}

// ------------------------------------------------------------------------------------------------
// Third form: the same recurrence with less bookkeeping per row, and a shared first level.
//   * (d_i, e_{i-1}^2) are interleaved: one 16-byte LDS broadcast per row;
//   * the sign bit of every p_i is shifted into a 32-bit history word (one v_alignbit per row); the sign changes of
//     32 rows are counted at once, popcount(h ^ (h >> 1 | previous word's last bit << 31)): three instructions per
//     32 rows instead of three per row;
//   * renormalisation without the zero special cases: v_frexp_exp of 0 is 0, which at worst skips one renormalisation (the
//     block after an exact zero has none), far from the range limits (see RS above); round 4: by the exponent of p_i ALONE
//     (two instructions fewer per eight rows).  p_{i-1} may then sit up to 2^200 above 1 after a cancellation in p_i (the e^2
//     floor bounds the ratio) and p grows by at most 3^8 until the next renormalisation: nowhere near 2^1023.  A power of two
//     is exact, so every sign, every count and every eigenvalue is what it was, bit for bit;
//   * first level: the workgroup counts at 256*EPT uniformly spaced points of the Gershgorin interval in ONE
//     evaluation round and every eigenvalue starts from the grid cell that brackets it -- ten bisection levels for
//     the price of one; the search keeps the invariant count(lo) <= m < count(hi) and therefore needs no
//     monotonicity of the computed counts.
//   * stopping rule: a bracket is final when it is narrower than 2 eps |x| -- RELATIVE to the eigenvalue, nothing
//     absolute.  T comes out of two orthogonal reductions whose worst-case error is eps |T|, but on these graded
//     pencils the eigenvalues next to zero (|E| ~ 1e-8 |T| at the ionisation threshold) come out far better than
//     that bound (measured against 113-bit truth, tests/golden/truth_*.npz: ~1e-3 eps |T|, as with LAPACK), and
//     north_star's bar is 1e-10 RELATIVE; an absolute floor of eps/16 |T| (round 1) put up to 8e-7 relative error
//     on exactly those eigenvalues.
//   * the tail: the eigenvalues next to zero need up to 25 more levels than the bulk, and in a lock-step search the
//     whole workgroup would pay every one of them at the full price.  Once every thread has at most half of its
//     eigenvalues unfinished, the unfinished ones are compacted into a list in LDS and the workgroup's 256*EPT
//     evaluation slots are dealt out evenly: P = floor(256*EPT / K) points inside every remaining bracket per
//     round (multisection: log2(P+1) levels per round, more the fewer remain).  Every eigenvalue's result depends
//     only on its own bracket and on K, so the spectra stay bit-identical from run to run.
constexpr int HW = 32;     // rows per sign-history word (np is padded to a multiple of it)

// Rows 1 .. nl come from LDS (de), rows nl + 1 .. np from global memory (gt, same indexing; nl = np: no global part).  The
// global part exists for matrices whose rows do not fit the LDS (n > 8672 with 1024 slots): the loads do not depend on the
// recurrence, so the compiler issues a block's worth ahead of their use.
#define STURM_BLOCK(LOADROW)                                                                          \
    {                                                                                                 \
        _Pragma("unroll") for (int sb = 0; sb < HW / RS; ++sb) {                                      \
            _Pragma("unroll") for (int r = 0; r < RS; ++r) {                                          \
                const double2 v = LOADROW(ib + sb * RS + r + 1);                                      \
                _Pragma("unroll") for (int c = 0; c < EPT; ++c) {                                     \
                    const double pn = __builtin_fma(v.x - x[c], p1[c], -(v.y * p0[c]));               \
                    h[c] = __builtin_amdgcn_alignbit(h[c], (unsigned)__double2hiint(pn), 31);         \
                    p0[c] = p1[c];                                                                    \
                    p1[c] = pn;                                                                       \
                }                                                                                     \
            }                                                                                         \
            _Pragma("unroll") for (int c = 0; c < EPT; ++c) {                                         \
                const int ex = -__builtin_amdgcn_frexp_exp(p1[c]);   /* by p_i alone: see below */   \
                p1[c] = __builtin_amdgcn_ldexp(p1[c], ex);                                            \
                p0[c] = __builtin_amdgcn_ldexp(p0[c], ex);                                            \
                if (VAL) es[c] -= ex;                                /* p_true = p 2^es */            \
            }                                                                                         \
        }                                                                                             \
        _Pragma("unroll") for (int c = 0; c < EPT; ++c) {                                             \
            const unsigned t = __builtin_amdgcn_alignbit(hp[c], h[c], 1);                             \
            cnt[c] += __builtin_popcount(h[c] ^ t);                                                   \
            hp[c] = h[c];                                                                             \
        }                                                                                             \
    }
__device__ __forceinline__ double2 sturm_gload(const double2 *p)
{
    typedef double d2v __attribute__((ext_vector_type(2)));
    const d2v v = __builtin_nontemporal_load(reinterpret_cast<const d2v *>(p));      // served by the L2: the rows were written by this kernel
    return make_double2(v.x, v.y);
}
// VAL: also log2 |p_n(x)| (lf: the accumulated exponent of the renormalisations + log2 of the last mantissa, single precision --
// 13 bits of exponent, 11 of fraction: the secant step it feeds needs three digits of the RATIO of two such values)
template <int EPT, bool VAL = false>
__device__ __forceinline__ void sturm_counts3(const double2 *__restrict__ de, int np, const double (&x)[EPT], int (&cnt)[EPT],
                                              const double2 *__restrict__ gt = nullptr, int nl = 0x7fffffff, float *lf = nullptr)
{
    double p0[EPT], p1[EPT];
    unsigned h[EPT], hp[EPT];
    int es[EPT];
#pragma unroll
    for (int c = 0; c < EPT; ++c) es[c] = 0;
    const double d0 = de[0].x;
#pragma unroll
    for (int c = 0; c < EPT; ++c) {
        p0[c] = 1.0; p1[c] = d0 - x[c];
        hp[c] = (unsigned)__double2hiint(p1[c]) >> 31;      // p_0 = 1 > 0: a negative p_1 is the first sign change
        cnt[c] = (int)hp[c]; h[c] = 0u;
    }
    const int nlds = nl < np ? nl : np;
#define STURM_LDS(i) de[i]
#define STURM_GLB(i) sturm_gload(gt + (i))
    for (int ib = 0; ib < nlds; ib += HW) STURM_BLOCK(STURM_LDS)
    for (int ib = nlds; ib < np; ib += HW) STURM_BLOCK(STURM_GLB)
#undef STURM_LDS
#undef STURM_GLB
    if (VAL) {
#pragma unroll
        for (int c = 0; c < EPT; ++c) {
            const int e2 = __builtin_amdgcn_frexp_exp(p1[c]);
            const float mant = (float)__builtin_amdgcn_ldexp(p1[c], -e2);                    // 0.5 <= |mant| < 1, or 0
            lf[c] = (float)(es[c] + e2) + __log2f(fmaxf(fabsf(mant), 1e-30f));
        }
    }
}

// point q (0-based) of P interior points of the bracket [a, a + w]; the evaluating and the deciding thread must get
// the same bits, hence the explicit fma
__device__ __forceinline__ double msect_point(double a, double w, int q, double rp)
{
    return __builtin_fma(w, (double)(q + 1) * rp, a);
}

__device__ __forceinline__ bool bracket_final(double lo, double hi)
{
    const double mid = 0.5 * (lo + hi);
    return (mid <= lo) || (mid >= hi) || (hi - lo <= 2.0 * 2.220446049250313e-16 * fmax(fabs(lo), fabs(hi)) + 1e-300);
}

// a value that is the same in every lane, moved to scalar registers (bit for bit)

// dynamic LDS of bisect3_kernel<EPT, TPB> for n rows (ng = TPB * EPT evaluation slots)
static size_t bisect3_lds_bytes(int n, int ng)
{
    const int np = (n + HW - 1) / HW * HW;
    return (size_t)(np + 1) * 16 + (size_t)(ng / 2) * 16 + (size_t)ng * 4 + (size_t)(ng / 2) * 4;
}

// TPB threads per workgroup: 512 = two waves per SIMD sharing one LDS copy of the matrix (one wave per SIMD reaches
// only ~60 % of the fp64 vector rate: tools/microbench/mfma_f64_peak, v_fma_f64 line)
//
// pair_stride > 0: the workgroup runs TWO logical workgroups of its channel one after the other, bx = blockIdx.x and bx + pair_stride
// (the second only if it exists), on one set-up: the quarters of a spectrum do not cost the same (the one next to zero takes 1.5 x the
// rounds of the middle ones, tools/sim_bisect_rounds.py) and a grid of more workgroups than CUs left the placement of slow beside
// slow to the dispatcher.  A logical workgroup keeps its slots, its slot-to-eigenvalue map and its tail list, so every
// eigenvalue sees the same points in the same order: the spectra do not depend on pair_stride, bit for bit.
// DIAG: the instrumented instance (BSP_BISECT_DIAG; `diag` non-null): a record per logical workgroup; the other carries no stamp, no
// test for one.
//
// QUEUE (BSP_BISECT_QUEUE, launch_bisect): a 1-D grid of at most two hardware workgroups per CU, and every one of them CLAIMS its items
// -- logical workgroups (x, channel) -- from a list in global memory until none is left.  The list is in the order of the expected
// cost, costliest first: item i is channel i % batch of rank i / batch, and the ranks take x from the ends of the spectrum inwards
// (nw - 1, 0, nw - 2, 1, ..).  The first workgroup to arrive on a CU (an atomic on the CU's word of the arrival table, the CU from
// HW_REG_XCC_ID and HW_REG_HW_ID) claims from the head of the list, the second from its tail, so a CU that holds two starts a slow
// item beside a fast one whatever the dispatcher does.  The placement only decides which end a workgroup draws from: every item is
// handed out exactly once (`claimed` counts the claims, so head and tail cannot cross) wherever the workgroups sit, and no workgroup
// waits for another.  What an item computes is what it computes in the other launches; the set-up is redone when the channel changes.
constexpr int BISECT_DIAG_WORDS = 10;  // x, channel, HW_REG_XCC_ID, HW_REG_HW_ID, wall clock at its start and end, lock-step rounds, tail rounds,
                                       // the hardware workgroup, its arrival number on its CU (queue launch; else -1)
constexpr int BISECT_Q_CUS = 16 * 256; // words of the arrival table: HW_REG_XCC_ID (4 bits) x the CU, SH and SE bits of HW_REG_HW_ID (8)
constexpr int BISECT_Q_WORDS = BISECT_Q_CUS + 4;   // .. and the words `claimed`, `head`, `tail`
template <int EPT, int TPB, bool DIAG = false, bool QUEUE = false>
__global__ __launch_bounds__(TPB) void bisect3_kernel(int n, int ldn, const double *__restrict__ dall,
                                                     const double *__restrict__ eall, double *wall, long ldw, int tail,
                                                     double2 *gtail, int nl, int hybrid_arg, int pair_stride, long long *diag,
                                                     unsigned *qcnt, int items, int batch)
{
    long long dt0 = DIAG ? (long long)wall_clock64() : 0;
    // (eight eigenvalues per thread, BSP_BISECT_EPT=8, an A/B of round 1: plain bisection -- the secant rounds' state does not fit its registers)
    const int hybrid = EPT > 4 ? 0 : hybrid_arg;
    extern __shared__ double2 sde[];
    constexpr int NG = TPB * EPT;
    constexpr int NW = TPB / 64;
    constexpr int KC = NG / 2;                         // capacity of the tail list
    const int np = (n + HW - 1) / HW * HW;
    const int nlr = nl < np ? nl : np;                 // rows 0 .. nlr live in LDS, rows nlr + 1 .. np in global memory (gtail)
    double2 *de = sde;                                 // de[i] = (d_i, e_{i-1}^2), i = 0 .. nlr
    // the secant rounds hand at most NG / 4 brackets to the tail: a shorter list; the rounds themselves keep their points in the same
    // bytes (bisect3_lds_bytes: 14 NG -- a point, its log2 |p_n| and its count in 16 bits per slot; the tail 9 NG)
    const int kcap = hybrid ? NG / 4 : KC;
    double *llo = (double *)(sde + nlr + 1);           // tail list: brackets and eigenvalue numbers
    double *lhi = llo + kcap;
    int *cg = (int *)(lhi + kcap);                     // counts at the NG evaluation slots
    int *lm = cg + NG;
    __shared__ double red[2 * NW];
    __shared__ int sK;
    __shared__ int sItem, sSide;                       // QUEUE: the claimed item (-1: none left); the end of the list this workgroup claims from
    const int tid0 = threadIdx.x;
    size_t ch = blockIdx.y;
    double *wout;
    double2 *gt;
    double gl, gu, isc;
    // the set-up of a channel: Gershgorin bounds, scaling, the rows (d, e^2) to LDS (and to global memory beyond row nlr)
    const auto channel_setup = [&]() __attribute__((always_inline)) {
        const double *dg = dall + ch * (size_t)ldn, *eg = eall + ch * (size_t)ldn;
        wout = wall + ch * (size_t)ldw;
        // the rows that do not fit the LDS: every workgroup of a channel writes the same values to the channel's slice
        gt = gtail ? gtail + ch * (size_t)(np + 1) : nullptr;
        gl = 1e300; gu = -1e300;
        for (int i = tid0; i < n; i += TPB) {
            const double di = dg[i];
            const double el = (i > 0) ? fabs(eg[i - 1]) : 0.0;
            const double er = (i < n - 1) ? fabs(eg[i]) : 0.0;
            gl = fmin(gl, di - el - er);
            gu = fmax(gu, di + el + er);
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            gl = fmin(gl, __shfl_xor(gl, off));
            gu = fmax(gu, __shfl_xor(gu, off));
        }
        if ((tid0 & 63) == 0) { red[tid0 >> 6] = gl; red[NW + (tid0 >> 6)] = gu; }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < NW; ++q) { gl = fmin(gl, red[q]); gu = fmax(gu, red[NW + q]); }
        const double eps = 2.220446049250313e-16;
        double tnorm = fmax(fabs(gl), fabs(gu));
        if (!(tnorm > 0.0)) tnorm = 1.0;                   // the zero matrix
        int kexp;
        (void)frexp(tnorm, &kexp);                         // tnorm = f 2^kexp, f in [0.5, 1)
        const double sc = ldexp(1.0, -kexp), isc_v = ldexp(1.0, kexp);
        for (int i = tid0; i <= np; i += TPB) {
            // row i of the scaled matrix with its coupling to row i-1.  Padding rows: d = 2, coupling at the floor.
            const double di = (i < n) ? dg[i] * sc : 2.0;
            const double ev = (i >= 1 && i < n) ? (eg[i - 1] * sc) : 0.0;
            const double2 row = make_double2(di, fmax(ev * ev, 1e-60));
            if (i <= nlr) de[i] = row; else gt[i] = row;
        }
        if (gt) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this workgroup's stores have reached the L2 it reads them back from
        __syncthreads();
        gl = gl * sc - 2.1 * eps * n - 1e-300;             // scaled Gershgorin interval, widened as dstebz does
        gu = gu * sc + 2.1 * eps * n + 1e-300;

        // the same in every lane, and live through the items: in scalar registers
        gl = read_first_lane(gl); gu = read_first_lane(gu);
        isc = read_first_lane(isc_v);
    };
    const int nwl = (n + NG - 1) / NG;                 // logical workgroups of a channel
    int side = -1;                                     // DIAG: the workgroup's arrival number on its CU
    if (QUEUE) {
        if (tid0 == 0) {
            const unsigned xcc = __builtin_amdgcn_s_getreg((31 << 11) | 20) & 0xfu;                 // HW_REG_XCC_ID
            const unsigned cu = (__builtin_amdgcn_s_getreg((31 << 11) | 4) >> 8) & 0xffu;         // HW_REG_HW_ID: CU bits 8-11, SH 12, SE 13-15
            sSide = (int)atomicAdd(qcnt + xcc * 256 + cu, 1u);
        }
    } else
        channel_setup();
#pragma unroll 1
    for (int item = 0; QUEUE || item < 2; ++item) {
        int bx;                                            // the logical workgroup: eigenvalues bx NG .. bx NG + NG - 1
        if (QUEUE) {
            // the previous item's last reads of its tail list and of sItem are over: the slot arrays are used again
            if (item) __syncthreads();
            if (tid0 == 0) {
                int it = -1;
                if (atomicAdd(qcnt + BISECT_Q_CUS, 1u) < (unsigned)items)     // `claimed`: at most `items` claims draw from the two ends
                    it = (sSide & 1) ? items - 1 - (int)atomicAdd(qcnt + BISECT_Q_CUS + 2, 1u) : (int)atomicAdd(qcnt + BISECT_Q_CUS + 1, 1u);
                sItem = it;
            }
            __syncthreads();
            const int it = __builtin_amdgcn_readfirstlane(sItem);
            if (it < 0) break;
            if (DIAG) { dt0 = (long long)wall_clock64(); side = __builtin_amdgcn_readfirstlane(sSide); }
            const int rank = it / batch;
            bx = (rank & 1) ? (rank >> 1) : nwl - 1 - (rank >> 1);
            const size_t chn = (size_t)(it - rank * batch);
            if (item == 0 || chn != ch) { ch = chn; channel_setup(); }
        } else {
            bx = blockIdx.x + item * pair_stride;
            if (item) {
                if (pair_stride == 0 || bx >= nwl) break;
                __syncthreads();                           // the first one's last reads of its tail list: the slot arrays are used again
                if (DIAG) dt0 = (long long)wall_clock64();
            }
        }
        int drounds = 0, dtail = 0;
        // the thread's number, opaque to the compiler: the slot addresses it forms from it are the same for both items, and hoisted in front
        // of the loop they stayed live through it (20 registers: the kernel left its 128, and with them two workgroups per CU)
        int tid = tid0;
        asm volatile("" : "+v"(tid));
        const int mbase = bx * NG + tid;                   // eigenvalue indices mbase + TPB c
        double lo[EPT], hi[EPT];
        int clo[EPT], chi[EPT];                            // count(lo) <= m < count(hi): the bracket is ISOLATING when chi - clo = 1
        float lflo[EPT], lfhi[EPT];                        // log2 |p_n| at the ends (3e38: not known)
        if (!hybrid) {
            // first level: NG interior points x_j = gl + (gu - gl) (j+1)/(NG+1), j = tid + TPB c
            const double w = gu - gl;
            double xg[EPT];
            int cc[EPT];
#pragma unroll
            for (int c = 0; c < EPT; ++c) xg[c] = gl + w * ((double)(tid + TPB * c + 1) * (1.0 / (NG + 1)));
            if (DIAG) ++drounds;
            sturm_counts3<EPT>(de, np, xg, cc, gt, nlr);
#pragma unroll
            for (int c = 0; c < EPT; ++c) cg[tid + TPB * c] = cc[c];
            __syncthreads();
#pragma unroll
            for (int c = 0; c < EPT; ++c) {
                const int m = mbase + TPB * c;
                int L = -1, R = NG;                        // count(x_L) <= m < count(x_R), with x_{-1} = gl, x_NG = gu
                while (R - L > 1) {
                    const int mid = (L + R) >> 1;
                    if (cg[mid] > m) R = mid; else L = mid;
                }
                lo[c] = (L < 0) ? gl : gl + w * ((double)(L + 1) * (1.0 / (NG + 1)));
                hi[c] = (R >= NG) ? gu : gl + w * ((double)(R + 1) * (1.0 / (NG + 1)));
                clo[c] = (L < 0) ? 0 : cg[L];
                chi[c] = (R >= NG) ? n : cg[R];
            }
        }
        bool done[EPT];
        if (hybrid) {
            // Lock-step rounds with a SAFEGUARDED SECANT step (round 4).  The Sturm recurrence delivers p_n(x) with its count: once a
            // bracket holds ONE eigenvalue (chi - clo = 1) and p_n is known at both ends, the next point is the regula falsi estimate
            //   x = lo + (hi - lo) r / (1 + r),  r = |p_n(lo)| / |p_n(hi)| = 2^(lflo - lfhi),
            // in its Illinois form: an end that survives two estimates in a row has its value halved, so both ends close in on the
            // eigenvalue (superlinearly) and the bracket itself collapses.  The COUNT alone decides which end a point replaces (the
            // invariant count(lo) <= m < count(hi) never rests on the value), three rounds that have not halved the bracket between
            // them are followed by a bisection, and the stopping rule is the bisection's: the result is a point of a bracket
            // narrower than 2 eps |x|, as before -- after ~19 evaluations instead of ~49 (tools/sim_secant.py on C4's spectra: 99 %
            // within 25; single precision in log2 |p_n| costs nothing).
            //
            // SHARED POINTS: while a bracket still holds several eigenvalues of this workgroup -- numbers a .. b - 1, q = b - a of them;
            // they all carry the same bracket -- eigenvalue a + r takes point r + 1 of q + 1 equal parts of it, every point of the round
            // goes to LDS with its count and its log2 |p_n| (slot = eigenvalue number, so a bracket's points are the slots a .. b - 1, in
            // ascending order), and every one of the q eigenvalues takes the tightest bracket that ALL q counts allow: the bracket
            // shrinks q + 1 fold where the midpoint halved it.  The first level (everything in the Gershgorin interval: a uniform grid
            // of NG points) is the first round of the same rule; on the graded spectra of the B-spline pencils, where a tenth of that
            // grid's cells hold all the eigenvalues, the next two rounds do what took ten bisections (tools/sim_grid.py: 11 - 15
            // evaluations per eigenvalue instead of 17 - 19).  Any point with count <= m is a lower end for eigenvalue m and any with
            // count > m an upper end, whoever evaluated it: nothing rests on the brackets of a cell being the same or on the counts
            // being monotone -- a point is taken if it lies strictly inside the bracket the eigenvalue's OWN point has left.
            double *xs = llo;                              // the round's points, by slot (the tail's list and counts reuse the bytes)
            float *lfs = (float *)(xs + NG);
            unsigned short *cs = (unsigned short *)(lfs + NG);       // n <= 65535 (launch_bisect)
            const int m0 = bx * NG, m1 = min(m0 + NG, n);
            float wref[EPT];                              // the bracket's width when it last halved
            int st[EPT];                                  // bits 0-1: the end the last estimate replaced (1 hi, 2 lo); bits 2..: rounds since wref
#pragma unroll
            for (int c = 0; c < EPT; ++c) {
                wref[c] = 3e38f; st[c] = 0;
                lo[c] = gl; hi[c] = gu; clo[c] = 0; chi[c] = n; lflo[c] = 3e38f; lfhi[c] = 3e38f;
            }
            for (int it = 0; it < 200; ++it) {
                double x[EPT];
                bool sec[EPT];
                int rng[EPT];                             // shared point: slots s0 | s1 << 16 of the bracket's points, else 0
#pragma unroll
                for (int c = 0; c < EPT; ++c) {
                    const int m = mbase + TPB * c;
                    const double wd = hi[c] - lo[c];
                    done[c] = (m >= n) || bracket_final(lo[c], hi[c]);
                    if ((float)wd <= 0.5f * wref[c]) { wref[c] = (float)wd; st[c] &= 3; }
                    const bool slow = (st[c] >> 2) >= 3;
                    st[c] += 4;
                    x[c] = 0.5 * (lo[c] + hi[c]); sec[c] = false; rng[c] = 0;
                    const int a = max(clo[c], m0), b = min(chi[c], m1);
                    if (chi[c] - clo[c] == 1 && lflo[c] < 1e38f && lfhi[c] < 1e38f && !slow && !done[c]) {
                        const double tiny = 2.0 * 2.220446049250313e-16 * fmax(fabs(lo[c]), fabs(hi[c]));
                        const float dl = fminf(fmaxf(lflo[c] - lfhi[c], -60.0f), 60.0f);
                        const double r = (double)exp2f(dl);
                        const double xe = fmin(fmax(lo[c] + wd * (r / (1.0 + r)), lo[c] + tiny), hi[c] - tiny);
                        if (xe > lo[c] && xe < hi[c]) { x[c] = xe; sec[c] = true; }
                    } else if (b - a > 1 && m >= a && m < b && !slow && !done[c]) {
                        const double xq = msect_point(lo[c], wd, m - a, 1.0 / (double)(b - a + 1));
                        if (xq > lo[c] && xq < hi[c]) { x[c] = xq; rng[c] = (a - m0) | ((b - m0) << 16); }
                    }
                }
                // on to the multisection tail once few enough brackets are left for it to have many points in each (NG / hybrid slots:
                // the stragglers of these rounds are brackets that are still WIDE, and the tail shrinks a bracket by P + 1 per round)
                int tot = 0;
#pragma unroll
                for (int c = 0; c < EPT; ++c) tot += __syncthreads_count(!done[c]);     // (and: last round's reads of xs, cs, lfs are over)
                if (tot <= (tail ? NG / hybrid : 0)) break;
                int cnt[EPT];
                float lf[EPT];
                if (DIAG) ++drounds;
                sturm_counts3<EPT, true>(de, np, x, cnt, gt, nlr, lf);
#pragma unroll
                for (int c = 0; c < EPT; ++c) {
                    xs[tid + TPB * c] = x[c]; cs[tid + TPB * c] = (unsigned short)cnt[c]; lfs[tid + TPB * c] = lf[c];
                }
                __syncthreads();
#pragma unroll
                for (int c = 0; c < EPT; ++c) {
                    if (done[c]) continue;
                    const int m = mbase + TPB * c;
                    const bool up = cnt[c] > m;                                    // x is above eigenvalue m: it replaces hi
                    const int last = st[c] & 3;
                    if (up) {
                        hi[c] = x[c]; chi[c] = cnt[c]; lfhi[c] = lf[c];
                        if (sec[c] && last == 1 && lflo[c] < 1e38f) lflo[c] -= 1.0f;   // Illinois: lo survived two estimates
                    } else {
                        lo[c] = x[c]; clo[c] = cnt[c]; lflo[c] = lf[c];
                        if (sec[c] && last == 2 && lfhi[c] < 1e38f) lfhi[c] -= 1.0f;
                    }
                    st[c] = (st[c] & ~3) | (sec[c] ? (up ? 1 : 2) : 0);
                    if (rng[c]) {
                        // the other points of the bracket: L = the last slot before R with count <= m, R = the first found with count > m
                        // (the search's own tests guarantee both counts; -1 / s1: none)
                        const int s0 = rng[c] & 0xffff, s1 = rng[c] >> 16;
                        int L = s0 - 1, R = s1;
                        while (R - L > 1) {
                            const int mid = (L + R) >> 1;
                            if ((int)cs[mid] > m) R = mid; else L = mid;
                        }
                        if (R < s1) { const double xr = xs[R]; if (xr > lo[c] && xr < hi[c]) { hi[c] = xr; chi[c] = cs[R]; lfhi[c] = lfs[R]; } }
                        if (L >= s0) { const double xl = xs[L]; if (xl > lo[c] && xl < hi[c]) { lo[c] = xl; clo[c] = cs[L]; lflo[c] = lfs[L]; } }
                    }
                }
            }
            __syncthreads();                               // the tail's list goes where the points were
        } else
        // lock-step bisection until every thread has at most EPT/2 unfinished eigenvalues (<= KC in the workgroup)
        for (int it = 0; it < 160; ++it) {
            double mid[EPT];
            int nun = 0;
#pragma unroll
            for (int c = 0; c < EPT; ++c) {
                mid[c] = 0.5 * (lo[c] + hi[c]);
                done[c] = (mbase + TPB * c >= n) || bracket_final(lo[c], hi[c]);
                nun += done[c] ? 0 : 1;
            }
            if (!__syncthreads_or(nun > (tail ? EPT / 2 : 0))) break;
            int cnt[EPT];
            if (DIAG) ++drounds;
            sturm_counts3<EPT>(de, np, mid, cnt, gt, nlr);
#pragma unroll
            for (int c = 0; c < EPT; ++c) {
                if (!done[c]) {
                    if (cnt[c] > mbase + TPB * c) hi[c] = mid[c]; else lo[c] = mid[c];
                }
            }
        }
        // the tail: compact the unfinished into the list, store the finished
        if (tid == 0) sK = 0;
        __syncthreads();
#pragma unroll
        for (int c = 0; c < EPT; ++c) {
            const int m = mbase + TPB * c;
            done[c] = (m >= n) || bracket_final(lo[c], hi[c]);
            if (!done[c]) {
                const int pos = atomicAdd(&sK, 1);
                if (pos < kcap) { llo[pos] = lo[c]; lhi[pos] = hi[c]; lm[pos] = m; }
                else wout[m] = 0.5 * (lo[c] + hi[c]) * isc;      // cannot happen (<= EPT/2 per thread); never lose a value
            } else if (m < n) wout[m] = 0.5 * (lo[c] + hi[c]) * isc;
        }
        __syncthreads();
        for (int round = 0; round < 128; ++round) {
            const int K = min(sK, kcap);                   // uniform: written before the last barrier
            if (K == 0) break;
            const int P = NG / K;                          // >= 2 points inside every bracket
            const double rp = 1.0 / (double)(P + 1);
            double x[EPT];
            int cc[EPT];
#pragma unroll
            for (int c = 0; c < EPT; ++c) {
                const int s = tid + TPB * c, e = s / P, q = s - e * P;
                x[c] = 2.0;                                // idle slot: a point above the spectrum
                if (e < K) { const double a = llo[e]; x[c] = msect_point(a, lhi[e] - a, q, rp); }
            }
            if (DIAG) ++dtail;
            sturm_counts3<EPT>(de, np, x, cc, gt, nlr);
#pragma unroll
            for (int c = 0; c < EPT; ++c) cg[tid + TPB * c] = cc[c];
            __syncthreads();
            double nlo[EPT / 2], nhi[EPT / 2];
            int nm[EPT / 2];
            bool keep[EPT / 2];
#pragma unroll
            for (int j = 0; j < EPT / 2; ++j) {
                const int e = tid + TPB * j;
                keep[j] = false;
                if (e < K) {
                    const double a = llo[e], b = lhi[e], w = b - a;
                    const int m = lm[e];
                    const int *ce = cg + e * P;
                    int L = -1, R = P;                     // count(point L) <= m < count(point R); -1 = a, P = b
                    while (R - L > 1) {
                        const int mid = (L + R) >> 1;
                        if (ce[mid] > m) R = mid; else L = mid;
                    }
                    nlo[j] = (L < 0) ? a : msect_point(a, w, L, rp);
                    nhi[j] = (R >= P) ? b : msect_point(a, w, R, rp);
                    nm[j] = m;
                    if (bracket_final(nlo[j], nhi[j]) || !(nhi[j] - nlo[j] < w)) wout[m] = 0.5 * (nlo[j] + nhi[j]) * isc;
                    else keep[j] = true;
                }
            }
            __syncthreads();                               // every read of the list and of cg is done
            if (tid == 0) sK = 0;
            __syncthreads();
#pragma unroll
            for (int j = 0; j < EPT / 2; ++j) {
                if (keep[j]) {
                    const int pos = atomicAdd(&sK, 1);
                    llo[pos] = nlo[j]; lhi[pos] = nhi[j]; lm[pos] = nm[j];
                }
            }
            __syncthreads();
        }
        {   // round limit (not reached: every round shrinks every bracket): store what is left
            const int K = min(sK, kcap);
            for (int e = tid; e < K; e += TPB) wout[lm[e]] = 0.5 * (llo[e] + lhi[e]) * isc;
        }
        if (DIAG && tid == 0) {
            long long *rec = diag + (ch * (size_t)nwl + bx) * BISECT_DIAG_WORDS;
            rec[0] = bx; rec[1] = (long long)ch;
            rec[2] = (long long)(__builtin_amdgcn_s_getreg((31 << 11) | 20) & 0xfu);      // HW_REG_XCC_ID
            rec[3] = (long long)(unsigned)__builtin_amdgcn_s_getreg((31 << 11) | 4);     // HW_REG_HW_ID: CU bits 8-11, SH 12, SE 13-15
            rec[4] = dt0; rec[5] = (long long)wall_clock64();
            rec[6] = drounds; rec[7] = dtail;
            rec[8] = (long long)(blockIdx.x + gridDim.x * blockIdx.y); rec[9] = side;
        }
    }
}

// One eigenvalue (index m, 0-based, ascending) of one tridiagonal matrix by MULTISECTION on one wavefront: every round
// the 64 lanes count at 64 interior points of the bracket, which shrinks 65-fold (about ten rounds instead of 56
// bisections).  Used to start the inverse iteration for the eigenvector the reference consumes (Hij(:, n0_ini) of
// channel l_ini, matrices.f90:267) while the batched bisection of all channels is still running.
__global__ __launch_bounds__(64) void bisect_one_kernel(int n, const double *__restrict__ dg, const double *__restrict__ eg,
                                                       int m, double *out)
{
    extern __shared__ double sm[];
    const int np = (n + RS - 1) / RS * RS;
    double *d = sm, *e2 = sm + np + RS;
    const int lane = threadIdx.x;
    double gl = 1e300, gu = -1e300;
    for (int i = lane; i < n; i += 64) {
        const double di = dg[i];
        const double el = (i > 0) ? fabs(eg[i - 1]) : 0.0;
        const double er = (i < n - 1) ? fabs(eg[i]) : 0.0;
        gl = fmin(gl, di - el - er);
        gu = fmax(gu, di + el + er);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        gl = fmin(gl, __shfl_xor(gl, off));
        gu = fmax(gu, __shfl_xor(gu, off));
    }
    const double eps = 2.220446049250313e-16;
    double tnorm = fmax(fabs(gl), fabs(gu));
    if (!(tnorm > 0.0)) tnorm = 1.0;
    int kexp;
    (void)frexp(tnorm, &kexp);
    const double sc = ldexp(1.0, -kexp), isc = ldexp(1.0, kexp);
    for (int i = lane; i < np + RS; i += 64) {
        d[i] = (i < n) ? dg[i] * sc : 2.0;
        const double ev = (i < n - 1) ? (eg[i] * sc) : 0.0;
        e2[i] = fmax(ev * ev, 1e-60);
    }
    __syncthreads();
    double lo = gl * sc - 2.1 * eps * n - 1e-300, hi = gu * sc + 2.1 * eps * n + 1e-300;
    for (int round = 0; round < 40; ++round) {
        if (hi - lo <= 2.0 * eps * fmax(fabs(lo), fabs(hi)) + 1e-300) break;
        const double w = (hi - lo) * (1.0 / 65.0);
        const double x = lo + (lane + 1) * w;
        if (!(x > lo && x < hi)) {                         // the bracket cannot be divided any further
            const double mid = 0.5 * (lo + hi);
            if (!(mid > lo && mid < hi)) break;
        }
        double p0 = 1.0, p1 = d[0] - x;
        int cnt = (p1 < 0.0) ? 1 : 0;
        for (int ib = 0; ib < np; ib += RS) {
#pragma unroll
            for (int r = 0; r < RS; ++r) {
                const int i = ib + r + 1;
                const double pn = __builtin_fma(d[i] - x, p1, -(e2[i - 1] * p0));
                cnt += (int)((unsigned)(__double2hiint(pn) ^ __double2hiint(p1)) >> 31);
                p0 = p1; p1 = pn;
            }
            int ea, eb;
            (void)frexp(p1, &ea);
            (void)frexp(p0, &eb);
            const int ex = (p1 == 0.0) ? eb : ((p0 == 0.0) ? ea : max(ea, eb));
            p1 = ldexp(p1, -ex); p0 = ldexp(p0, -ex);
        }
        // eigenvalue m lies left of the first point whose count exceeds m
        const unsigned long long above = __ballot(cnt > m);
        const int f = above ? (__ffsll((long long)above) - 1) : 64;
        const double xl = __shfl(x, f > 0 ? f - 1 : 0), xh = __shfl(x, f < 64 ? f : 63);
        const double nlo = (f > 0) ? xl : lo, nhi = (f < 64) ? xh : hi;
        if (!(nhi - nlo < hi - lo)) break;
        lo = nlo; hi = nhi;
    }
    if (lane == 0) *out = 0.5 * (lo + hi) * isc;
}

// The same on a workgroup of 256 threads with the counting routine of bisect3_kernel: 1024 points per round (the
// bracket shrinks 1025-fold: six rounds), four independent recurrences per thread.  The one-wave kernel above took
// 12 ms next to the batched bisection (one dependent chain per lane, on a CU it shares); with the inverse iteration
// behind it the consumed eigenvector arrived 15 ms after the spectra.
__global__ __launch_bounds__(256) void bisect_one3_kernel(int n, const double *__restrict__ dg, const double *__restrict__ eg,
                                                         int m, double *out)
{
    extern __shared__ double2 sde[];
    constexpr int NG = 256 * EPT;
    const int np = (n + HW - 1) / HW * HW;
    double2 *de = sde;
    int *cg = (int *)(sde + np + 1);
    __shared__ double red[8];
    const int tid = threadIdx.x;
    double gl = 1e300, gu = -1e300;
    for (int i = tid; i < n; i += 256) {
        const double di = dg[i];
        const double el = (i > 0) ? fabs(eg[i - 1]) : 0.0;
        const double er = (i < n - 1) ? fabs(eg[i]) : 0.0;
        gl = fmin(gl, di - el - er);
        gu = fmax(gu, di + el + er);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        gl = fmin(gl, __shfl_xor(gl, off));
        gu = fmax(gu, __shfl_xor(gu, off));
    }
    if ((tid & 63) == 0) { red[tid >> 6] = gl; red[4 + (tid >> 6)] = gu; }
    __syncthreads();
    gl = fmin(fmin(red[0], red[1]), fmin(red[2], red[3]));
    gu = fmax(fmax(red[4], red[5]), fmax(red[6], red[7]));
    const double eps = 2.220446049250313e-16;
    double tnorm = fmax(fabs(gl), fabs(gu));
    if (!(tnorm > 0.0)) tnorm = 1.0;
    int kexp;
    (void)frexp(tnorm, &kexp);
    const double sc = ldexp(1.0, -kexp), isc = ldexp(1.0, kexp);
    for (int i = tid; i <= np; i += 256) {
        const double di = (i < n) ? dg[i] * sc : 2.0;
        const double ev = (i >= 1 && i < n) ? (eg[i - 1] * sc) : 0.0;
        de[i] = make_double2(di, fmax(ev * ev, 1e-60));
    }
    __syncthreads();
    double lo = gl * sc - 2.1 * eps * n - 1e-300, hi = gu * sc + 2.1 * eps * n + 1e-300;
    for (int round = 0; round < 24; ++round) {
        const double w = hi - lo;
        if (w <= 2.0 * eps * fmax(fabs(lo), fabs(hi)) + 1e-300) break;
        double x[EPT];
        int cc[EPT];
#pragma unroll
        for (int c = 0; c < EPT; ++c) x[c] = lo + w * ((double)(tid + 256 * c + 1) * (1.0 / (NG + 1)));
        sturm_counts3<EPT>(de, np, x, cc);
#pragma unroll
        for (int c = 0; c < EPT; ++c) cg[tid + 256 * c] = cc[c];
        __syncthreads();
        int L = -1, R = NG;                            // count(x_L) <= m < count(x_R); every thread does the same search
        while (R - L > 1) {
            const int mid = (L + R) >> 1;
            if (cg[mid] > m) R = mid; else L = mid;
        }
        __syncthreads();                               // cg is rewritten in the next round
        const double nlo = (L < 0) ? lo : lo + w * ((double)(L + 1) * (1.0 / (NG + 1)));
        const double nhi = (R >= NG) ? hi : lo + w * ((double)(R + 1) * (1.0 / (NG + 1)));
        if (!(nhi - nlo < w)) break;
        lo = nlo; hi = nhi;
    }
    if (tid == 0) *out = 0.5 * (lo + hi) * isc;
}

int launch_bisect_one(int n, const double *d_d, const double *d_e, int m, double *d_out, hipStream_t st)
{
    const int variant1 = opts().bisect;
    if (variant1 >= 3) {
        const size_t lds3 = (size_t)2 * (n + 3 * RS + HW) * sizeof(double) + 256 * EPT * sizeof(int);
        if (lds3 > 150 * 1024) return BSP_ERR_UNSUPPORTED;
        static bool attr3 = false;
        if (!attr3) {
            BSP_HIP(allow_lds(bisect_one3_kernel, 150 * 1024));
            attr3 = true;
        }
        hipLaunchKernelGGL(bisect_one3_kernel, dim3(1), dim3(256), lds3, st, n, d_d, d_e, m, d_out);
        BSP_HIP(hipGetLastError());
        return BSP_OK;
    }
    const size_t lds = (size_t)2 * (n + 3 * RS) * sizeof(double);
    if (lds > 150 * 1024) return BSP_ERR_UNSUPPORTED;
    static bool attr = false;
    if (!attr) {
        BSP_HIP(allow_lds(bisect_one_kernel, 150 * 1024));
        attr = true;
    }
    hipLaunchKernelGGL(bisect_one_kernel, dim3(1), dim3(64), lds, st, n, d_d, d_e, m, d_out);
    BSP_HIP(hipGetLastError());
    return BSP_OK;
}

int launch_bisect(LaunchCtx &cx, int n, int ldn, int batch, const double *d_d, const double *d_e, double *d_w, long ldw, hipStream_t st)
{
    // ONE workgroup shape for every batch size: 512 threads x 2 eigenvalues = 1024 evaluation slots and 1024 eigenvalues per
    // workgroup.  The bracket sequence of an eigenvalue depends on the first-level grid (its size = the slots) and on which
    // eigenvalues share a multisection tail, so a shape chosen by batch size (rounds 1-2: 512 x 4 for >= 256 workgroups, else
    // 256 x 4) made the last bits of a spectrum depend on how many channels were solved together.  Measured (round 3, n = 4096):
    // 128 channels 23.3 ms against 23.0 with 512 x 4; 32 channels 12.1 against 13.0; 16 channels 11.3 against 12.3 (256 x 2,
    // BSP_BISECT_EPT=21: 26.2 / 8.5 / 7.8 ms -- faster for small batches, 3 ms slower for the full one).
    // BSP_BISECT_EPT: 8 = 256 x 8 (round 1), 4 = 256 x 4, 2 = 1024 x 2, 21 = 256 x 2, 5 = 512 x 4.
    const int ept_env = opts().bisect_ept;
    int mode = (ept_env == 8) ? 8 : (ept_env == 4) ? 4 : (ept_env == 2) ? 1024 : (ept_env == 21) ? 21 : (ept_env == 5) ? 512 : 22;
    int ng = (mode == 4) ? 1024 : (mode == 21 ? 512 : (mode == 22 ? 1024 : 2048));
    if (bisect3_lds_bytes(n, ng) > 150 * 1024) { mode = 22; ng = 1024; }         // n = 8192: 146 KB with 1024 slots
    // Matrices whose rows do not fit the LDS beside the slot arrays (n > 8672 with 1024 slots): the first nl rows in LDS, the
    // rest in a global array the kernel writes and reads back through the L2 (sturm_counts3); nl a multiple of HW.
    const int np3 = (n + HW - 1) / HW * HW;
    int nl = np3;
    while (bisect3_lds_bytes(nl, ng) > 150 * 1024) nl -= HW;
    const size_t lds3 = bisect3_lds_bytes(nl, ng);
    const size_t lds = (size_t)2 * (n + 3 * RS + HW) * sizeof(double);    // variants 1 and 2
    // rows beyond the LDS (n > 8672): one scratch array of the ctx (a ctx bisects on one stream, whose launches are ordered, so it may
    // reuse its own; two problems bisecting at the same time share no rows), grown on demand
    double2 *gtail = nullptr;
    if (nl < np3) {
        const size_t need = (size_t)batch * (np3 + 1);
        if (need > cx.bis_tail_cap) {
            if (cx.bis_tail) { BSP_HIP(hipStreamSynchronize(st)); (void)hipFree(cx.bis_tail); cx.bis_tail = nullptr; cx.bis_tail_cap = 0; }
            BSP_HIP(hipMalloc(reinterpret_cast<void **>(&cx.bis_tail), need * sizeof(double2)));
            cx.bis_tail_cap = need;
        }
        gtail = cx.bis_tail;
        if (opts().bisect < 3) return BSP_ERR_UNSUPPORTED;                  // the older counting kernels keep the whole matrix in LDS
    }
    static bool attr_set = false;
    const int variant = opts().bisect;
    if (!attr_set) {
        BSP_HIP(allow_lds(bisect_kernel, 150 * 1024));
        BSP_HIP(allow_lds(bisect2_kernel, 150 * 1024));
        BSP_HIP(allow_lds(bisect3_kernel<4, 256>, 150 * 1024));
        BSP_HIP(allow_lds(bisect3_kernel<8, 256>, 150 * 1024));
        BSP_HIP(allow_lds(bisect3_kernel<4, 512>, 150 * 1024));
        BSP_HIP(allow_lds(bisect3_kernel<2, 1024>, 150 * 1024));
        BSP_HIP(allow_lds(bisect3_kernel<2, 256>, 150 * 1024));
        BSP_HIP(allow_lds(bisect3_kernel<2, 512>, 150 * 1024));
        BSP_HIP(allow_lds(bisect3_kernel<2, 512, true>, 150 * 1024));
        BSP_HIP(allow_lds(bisect3_kernel<2, 512, false, true>, 150 * 1024));
        BSP_HIP(allow_lds(bisect3_kernel<2, 512, true, true>, 150 * 1024));
        attr_set = true;
    }
    const dim3 grid((n + 256 * EPT - 1) / (256 * EPT), batch);
    if (variant == 1 || variant == 2) {
        KScope kt(KS_BISECT, st);
        if (variant == 1) hipLaunchKernelGGL(bisect_kernel, grid, dim3(256), lds, st, n, ldn, d_d, d_e, d_w, ldw);
        else hipLaunchKernelGGL(bisect2_kernel, grid, dim3(256), lds, st, n, ldn, d_d, d_e, d_w, ldw);
        BSP_HIP(hipGetLastError());
        return BSP_OK;
    }
    // Two logical workgroups per hardware workgroup, x and x + ceil(nw / 2), once there are more workgroups than CUs: they would share
    // CUs anyway, and the dispatcher deals them out so that the slow quarters of the spectra share theirs.  The rule
    // looks at the batch size -- allowed here because the schedule cannot change a bit of the result.
    // BSP_BISECT_PAIR: 1 = by this rule, 0 = never, 2 = always.
    const int cus = device_cus();
    const int nw = (n + ng - 1) / ng;
    const int pmode = opts().bisect_pair;
    // The item queue (bisect3_kernel, QUEUE): at most two hardware workgroups per CU claim the nw x batch logical workgroups from a list,
    // the first on a CU from its costly end, the second from its cheap end.  It takes the pairing rule's place where it fires, under the
    // same rule; the default workgroup shape only (the others keep their launch).
    // BSP_BISECT_QUEUE: 1 = when nw x batch exceeds the CU count, 0 = never, 2 = always.  BSP_BISECT_QUEUE_GRID (test hook): at most
    // this many hardware workgroups (0 = no cap), so that a small batch makes a workgroup run several items of several channels.
    const int qmode = opts().bisect_queue;
    const long items = (long)nw * batch;
    const bool queue = mode == 22 && items < (1L << 30) && (qmode == 2 || (qmode == 1 && items > cus));
    const int pair_stride = queue ? 0 : ((pmode == 2 || (pmode == 1 && items > cus)) ? (nw + 1) / 2 : 0);
    int qgrid = (int)std::min(items, 2L * cus);
    if (opts().bisect_queue_grid > 0) qgrid = std::min(qgrid, opts().bisect_queue_grid);
    const dim3 g3 = queue ? dim3(qgrid, 1) : dim3(pair_stride ? pair_stride : nw, batch);
    // the queue's counters (arrival table, claimed, head, tail): one small array of the ctx like the rows above, zeroed on the stream in
    // front of every launch
    unsigned *qcnt = nullptr;
    if (queue) {
        if (!cx.bis_qcnt) BSP_HIP(hipMalloc(reinterpret_cast<void **>(&cx.bis_qcnt), BISECT_Q_WORDS * sizeof(unsigned)));
        qcnt = cx.bis_qcnt;
        BSP_HIP(hipMemsetAsync(qcnt, 0, BISECT_Q_WORDS * sizeof(unsigned), st));
    }
    // (measured with BSP_BISECT_DIAG, 128 channels of n = 4096: the 256 paired workgroups land on 256 different CUs although two would fit
    // one CU's LDS -- no request for more LDS than the arrays need, profiles/r12_bisect_pairs.txt)
    const int tail = opts().bisect_tail;
    // (the secant rounds keep a point's count in 16 bits: beyond that size plain bisection)
    const int hyb = n > 65535 ? 0 : (opts().bisect_secant == 1 ? 8 : (opts().bisect_secant >= 4 ? opts().bisect_secant : (opts().bisect_secant >= 2 ? 4 : 0)));
#define BISECT3_LAUNCH_Q(E, T, D, Q, dbuf) hipLaunchKernelGGL((bisect3_kernel<E, T, D, Q>), g3, dim3(T), lds3, st, n, ldn, d_d, d_e, d_w, ldw, tail, gtail, nl, \
                                                              hyb, pair_stride, dbuf, qcnt, (int)items, batch)
#define BISECT3_LAUNCH(E, T, D, dbuf) BISECT3_LAUNCH_Q(E, T, D, false, dbuf)
    if (opts().bisect_diag) {                              // a record per logical workgroup, on stderr (tools/bisect_balance.py reads them)
        if (mode != 22) {
            fprintf(stderr, "bspatom: BSP_BISECT_DIAG is built for the default workgroup shape only (512 x 2)\n");
            return BSP_ERR_UNSUPPORTED;
        }
        const size_t words = (size_t)nw * batch * BISECT_DIAG_WORDS;
        std::vector<long long> h(words);
        long long *dbuf = nullptr;
        BSP_HIP(hipMalloc(reinterpret_cast<void **>(&dbuf), words * sizeof(long long)));
        BSP_HIP(hipMemsetAsync(dbuf, 0, words * sizeof(long long), st));
        if (queue) BISECT3_LAUNCH_Q(2, 512, true, true, dbuf);
        else BISECT3_LAUNCH(2, 512, true, dbuf);
        const hipError_t le = hipGetLastError();
        if (le != hipSuccess) { hipFree(dbuf); BSP_HIP(le); }
        BSP_HIP(hipStreamSynchronize(st));
        BSP_HIP(hipMemcpy(h.data(), dbuf, words * sizeof(long long), hipMemcpyDeviceToHost));
        hipFree(dbuf);
        int dev = 0, khz = 0;
        BSP_HIP(hipGetDevice(&dev));
        BSP_HIP(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev));
        fprintf(stderr, "bisect3 diag: n %d batch %d nw %d pair_stride %d queue %d grid %u x %u lds %zu cus %d wall_khz %d\n", n, batch, nw, pair_stride,
                queue ? 1 : 0, g3.x, g3.y, lds3, cus, khz);
        for (size_t r = 0; r < (size_t)nw * batch; ++r) {
            const long long *q = h.data() + r * BISECT_DIAG_WORDS;
            fprintf(stderr, "bisect3 wg: x %lld ch %lld xcc %lld hwid 0x%llx t0 %lld t1 %lld rounds %lld tail %lld hwg %lld side %lld\n", q[0], q[1], q[2], q[3],
                    q[4], q[5], q[6], q[7], q[8], q[9]);
        }
        return BSP_OK;
    }
    KScope kt(KS_BISECT, st);
    if (mode == 512) BISECT3_LAUNCH(4, 512, false, nullptr);
    else if (mode == 1024) BISECT3_LAUNCH(2, 1024, false, nullptr);
    else if (mode == 8) BISECT3_LAUNCH(8, 256, false, nullptr);
    else if (mode == 21) BISECT3_LAUNCH(2, 256, false, nullptr);
    else if (mode == 22 && queue) BISECT3_LAUNCH_Q(2, 512, false, true, nullptr);
    else if (mode == 22) BISECT3_LAUNCH(2, 512, false, nullptr);
    else BISECT3_LAUNCH(4, 256, false, nullptr);
#undef BISECT3_LAUNCH
#undef BISECT3_LAUNCH_Q
    BSP_HIP(hipGetLastError());
    return BSP_OK;
}

}  // namespace bsp
