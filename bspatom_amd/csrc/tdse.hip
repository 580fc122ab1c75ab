// tdse.hip -- the TDSE in the basis of the field-free eigenstates (bspatom_tdse_propagate):
//   i da_c/dt = E_c .* a_c + sum_{p: cf[p] = c} f_q(t) D_p^T a_{ci[p]} + sum_{p: ci[p] = c} conj(f_q(t)) D_p a_{cf[p]}
// for nscan wave packets at once, fixed steps of the embedded six-stage 4(5) Runge-Kutta pair of the reference (MOD_RK_PARAMS,
// Modules.f90:559-586; the state arrays zf, zdfdt, zVtij at :238-246).  Seven launches per step: one stage kernel per stage, which
// forms its operand y_s = a + dt sum_j A_sj k_j while it loads it and leaves k_s = -i H(t_n + c_s dt) y_s, then one kernel for the
// step, the error estimate and the snapshot.  bspatom_tdse_observe: on an observed step stage 0 runs as tdse_observe_kernel, which also
// measures a(t_n) (populations, E |a|^2, the coupling expectation value per channel), followed by tdse_obs_reduce_kernel: eight launches.
// bspatom_tdse_lawson: the integrating-factor form of the same tableau in the same launches (LAWSON below), after tdse_phase_kernel once.
//
// Working layout: the amplitudes of channel c are a real matrix [count][NC], column 2q = Re, 2q + 1 = Im of scan q, NC = 2 nscan
// rounded up to 16 (zero columns); a, k_0 .. k_5 are [nch][count][NC] each.  A coupling block times these columns is a real
// product on v_mfma_f64_16x16x4_f64; the field, which differs per column, enters in the epilogue.
#include "common.h"
#include "mfma_tile.h"

namespace bsp {

// ---- the tableau (MOD_RK_PARAMS, Modules.f90:568-584) ----------------------------------------------------------------------
// a21 .. a65 (:568-572), c1 .. c6 (:577-578: 0, 2/9, 1/3, 3/4, 1, 5/6 -- the row sums; the field table is laid out on them),
// the 5th-order weights d1 .. d6 (:580-581) that advance the solution, the 4th-order b1 .. b5 (:574-575, b6 = 0) of the estimate
const double TDSE_A[6][5] = {{0.0, 0.0, 0.0, 0.0, 0.0},
                             {2.0 / 9.0, 0.0, 0.0, 0.0, 0.0},
                             {1.0 / 12.0, 1.0 / 4.0, 0.0, 0.0, 0.0},
                             {69.0 / 128.0, -243.0 / 128.0, 135.0 / 64.0, 0.0, 0.0},
                             {-17.0 / 12.0, 27.0 / 4.0, -27.0 / 5.0, 16.0 / 15.0, 0.0},
                             {65.0 / 432.0, -5.0 / 16.0, 13.0 / 16.0, 4.0 / 27.0, 5.0 / 144.0}};
const double TDSE_D[6] = {47.0 / 450.0, 0.0, 12.0 / 25.0, 32.0 / 225.0, 1.0 / 30.0, 6.0 / 25.0};
const double TDSE_B[6] = {1.0 / 9.0, 0.0, 9.0 / 20.0, 16.0 / 45.0, 1.0 / 12.0, 0.0};

constexpr int TBK = 16, TBM = 64, TLDA = TBM + 16;

struct StageCoef { double w[5]; };          // A_s0 .. A_s,s-1

// y_s of one element from a and the k_j of the step, in one fixed order (the staged operand and the epilogue's E .* y agree bit for bit)
template <int S>
__device__ __forceinline__ double form_y(const double (&v)[S + 1], const StageCoef &cf, double dt)
{
    if constexpr (S == 0) {
        return v[0];
    } else {
        double s = cf.w[0] * v[1];
#pragma unroll
        for (int j = 1; j < S; ++j) s = fma(cf.w[j], v[j + 1], s);
        return fma(dt, s, v[0]);
    }
}

template <int S>
__device__ __forceinline__ void load_y(double (&v)[S + 1], const double *__restrict__ a, const double *__restrict__ K, size_t kstride,
                                       size_t idx, bool ok)
{
    // unconditional loads from a clamped address, the values selected afterwards (dipole.hip)
    const size_t at = ok ? idx : 0;
    const double x = a[at];
    v[0] = ok ? x : 0.0;
#pragma unroll
    for (int j = 0; j < S; ++j) {
        const double kx = K[(size_t)j * kstride + at];
        v[j + 1] = ok ? kx : 0.0;
    }
}

// One workgroup = 64 states of one channel x 16 TN columns; wave w owns rows 16 w .. 16 w + 15.  The channel's entries (its pairs
// in ascending p; ent[3e] = p, [3e+1] = the other channel, [3e+2] = 1 where the channel is ci[p]) are walked in order, every block
// along K ascending in steps of 16: nothing of the batch (nscan, nch, the list's length) enters the order of the sums of an element.
//   entry with cf[p] = c:  accT += D_p^T y_ci   -- the A tile is contiguous along M in memory (D_p[i][f], f = output row)
//   entry with ci[p] = c:  accN += D_p y_cf     -- contiguous along K; staged through the column permutation lds_swz
// Epilogue per scan: h = E y + f accT + conj(f) accN, k_s = -i h.
//
// OBS (stage 0 only, y_0 = a(t_n)): the epilogue also measures.  Before the field enters, accT of channel c is
// U = sum_{p: cf[p] = c} D_p^T a_ci[p], so per row f of scan q the lane pair (Re, Im) holds everything of
//   |a|^2,  E |a|^2,  conj(a) U = (y_re u_re + y_im u_im) + i (y_re u_im - y_im u_re):
// every lane forms y y, E (y y), y u and +- y u' (u' the neighbour's u; - on the Im lane) of its component, chained by fma over its
// four rows r = 0 .. 3; then lane + (lane ^ 16), + (lane ^ 32) (the rows (lane >> 4) of the wave), + (lane ^ 1) (Re + Im), the
// four waves through LDS as ((w0 + w1) + w2) + w3, and one partial of 4 doubles per (channel, row tile, scan) goes to
// part[((c tm + im) NC/2 + q) 4 + k].  The tree is fixed by count alone; rows beyond count enter as zeros; scans q >= nscan are
// not written.  fld == nullptr: measure only (the row after the last step) -- the same instructions, so the same bits.
//
// LAWSON (bspatom_tdse_lawson): the stage of the integrating-factor form.  phs[(c count + n) 2 + {0, 1}] = cos, sin of
// E[c][n] c_s dt, this stage's part of tdse_phase_kernel's table (s = 1 .. 5); R_s = cos - i sin.  The operand is y_s = R_s .* w_s, w_s what form_y
// gives: Re and Im of a state sit in neighbouring columns of the B tile, and since NB is even the column parity of idx = tid + r 256 is
// the lane's, so the partner is __shfl_xor(w, 1).  The epilogue leaves k_s = conj(R_s) .* (-i g), g = f accT + conj(f) accN without
// the E .* y term: one shuffle serves both the -i exchange and the rotation.  R_0 = 1: stage 0 rotates nothing and reads no phase, so
// the observing chains t0 .. t3 on y = a(t_n), en, u, up are those of the plain scheme, instruction for instruction.
template <int S, int TN, bool OBS, bool LAWSON>
__device__ __forceinline__ void tdse_stage_body(int count, int NC, int nscan, int tm, int tn, const int *__restrict__ cptr,
                                                const int *__restrict__ ent, const double *__restrict__ E,
                                                const double *__restrict__ D, const double *__restrict__ a,
                                                double *__restrict__ K, size_t kstride, const double *__restrict__ fld,
                                                StageCoef cf, double dt, double *__restrict__ part, const double *__restrict__ phs)
{
    static_assert(!OBS || S == 0, "only stage 0 runs on a(t_n)");
    constexpr bool ROT = LAWSON && S > 0;                                     // R_0 = 1; phs: this stage's phases [nch][count][2]
    constexpr int NB = 16 * TN, TLDB = NB + 16, BEL = TBK * NB / 256;        // B-tile elements per thread: 1 or 2
    __shared__ double As[TBK * TLDA];
    __shared__ double Bs[TBK * TLDB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int b = blockIdx.x;
    const int jn = b % tn; b /= tn;
    const int im = b % tm;
    const int c = b / tm;
    const int m0 = im * TBM, n0 = jn * NB;
    const int e0 = cptr[c], e1 = cptr[c + 1];
    const int ksteps = (count + TBK - 1) / TBK;
    const size_t blk = (size_t)count * count;

    double4_t accT[1][TN], accN[1][TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        accT[0][j] = (double4_t){0.0, 0.0, 0.0, 0.0};
        accN[0][j] = (double4_t){0.0, 0.0, 0.0, 0.0};
    }

    double ra[4], rb[BEL][S + 1];
    [[maybe_unused]] double rc[ROT ? BEL : 1], rs[ROT ? BEL : 1];                            // cos, +- sin (+ on the Re lane) of the B-tile rows
    // the loads of iteration it = (entry, k-step): A tile 64 x 16 of D_p (either orientation), B tile 16 x NB of y of the other channel
    auto load = [&](int it) {
        const int e = e0 + it / ksteps, k0 = (it % ksteps) * TBK;
        const int p = ent[3 * e], oc = ent[3 * e + 1], nrm = ent[3 * e + 2];
        const double *Dp = D + (size_t)p * blk;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int idx = tid + r * 256;
            // nrm: A(m, k) = D_p[m][k], consecutive threads along k; else A(m, k) = D_p[k][m], consecutive threads along m
            const int mm = nrm ? idx / TBK : idx % TBM, kk = nrm ? idx % TBK : idx / TBM;
            const int gm = m0 + mm, gk = k0 + kk;
            const bool ok = gm < count && gk < count;
            const double v = Dp[ok ? (nrm ? (size_t)gm * count + gk : (size_t)gk * count + gm) : 0];
            ra[r] = ok ? v : 0.0;
        }
#pragma unroll
        for (int r = 0; r < BEL; ++r) {
            const int idx = tid + r * 256;
            const int kk = idx / NB, col = n0 + idx % NB, gk = k0 + kk;
            load_y<S>(rb[r], a, K, kstride, ((size_t)oc * count + gk) * NC + col, gk < count && col < NC);
            if constexpr (ROT) {
                // the phase of row gk of channel oc, from a clamped address like load_y's
                const bool ok = gk < count;
                const double *pp = phs + (ok ? ((size_t)oc * count + gk) * 2 : 0);
                const double pc = pp[0], psn = pp[1];
                rc[r] = ok ? pc : 0.0;
                rs[r] = ok ? ((tid & 1) ? -psn : psn) : 0.0;
            }
        }
        return nrm;
    };
    auto store = [&](int nrm) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int idx = tid + r * 256;
            const int mm = nrm ? idx / TBK : idx % TBM, kk = nrm ? idx % TBK : idx / TBM;
            As[kk * TLDA + (mm ^ lds_swz(kk))] = ra[r];
        }
#pragma unroll
        for (int r = 0; r < BEL; ++r) {
            const int idx = tid + r * 256;
            const int kk = idx / NB, cc = idx % NB;
            if constexpr (ROT) {
                // y = R w: Re lane cos w_re + sin w_im, Im lane cos w_im - sin w_re
                const double wv = form_y<S>(rb[r], cf, dt);
                const double wo = __shfl_xor(wv, 1);
                Bs[kk * TLDB + (cc ^ lds_swz(kk))] = fma(rs[r], wo, rc[r] * wv);
            } else {
                Bs[kk * TLDB + (cc ^ lds_swz(kk))] = form_y<S>(rb[r], cf, dt);
            }
        }
    };

    const int nit = (e1 - e0) * ksteps;
    int nrm = 0;
    if (nit > 0) nrm = load(0);
    for (int it = 0; it < nit; ++it) {
        store(nrm);
        __syncthreads();
        const int cur = nrm;
        if (it + 1 < nit) nrm = load(it + 1);
        if (cur) {
#pragma unroll
            for (int k4 = 0; k4 < TBK / 4; ++k4) {
                const int kr = k4 * 4 + (lane >> 4);
                mfma_step<1, TN>(&As[kr * TLDA + wave * 16], &Bs[kr * TLDB], lane, kr, accN);
            }
        } else {
#pragma unroll
            for (int k4 = 0; k4 < TBK / 4; ++k4) {
                const int kr = k4 * 4 + (lane >> 4);
                mfma_step<1, TN>(&As[kr * TLDA + wave * 16], &Bs[kr * TLDB], lane, kr, accT);
            }
        }
        __syncthreads();
    }

    // epilogue: this lane holds column col (Re of scan col / 2 if even, Im if odd) of rows (lane >> 4) + 4 r; the other component of the
    // same scan is in lane ^ 1.  Every lane forms its own component of h; k_s = -i h = (Im h, -Re h) is then the neighbour's value.
    double *Ks = K + (size_t)S * kstride;
    const bool stepping = !OBS || fld != nullptr;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int col = n0 + j * 16 + (lane & 15);
        const int q = col >> 1, odd = col & 1;
        const bool cok = col < NC, fok = q < nscan;
        const double fre = stepping ? fld[fok ? 2 * q : 0] : 0.0, fim = stepping ? fld[fok ? 2 * q + 1 : 0] : 0.0;
        const double fr = fok ? fre : 0.0, fi = fok ? (odd ? fim : -fim) : 0.0;
        double t0 = 0.0, t1 = 0.0, t2 = 0.0, t3 = 0.0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int gm = m0 + wave * 16 + (lane >> 4) + 4 * r;
            const bool ok = cok && gm < count;
            const size_t idx = ((size_t)c * count + gm) * NC + col;
            [[maybe_unused]] double y = 0.0, en = 0.0;
            if constexpr (!LAWSON || OBS) {
                double v[S + 1];
                load_y<S>(v, a, K, kstride, idx, ok);
                y = form_y<S>(v, cf, dt);
                en = E[ok ? (size_t)c * count + gm : 0];
            }
            const double u = accT[0][j][r], w = accN[0][j][r];
            const double up = __shfl_xor(u, 1), wp = __shfl_xor(w, 1);
            // even lane: Re h = E y_re + (f_re u_re - f_im u_im) + (f_re w_re + f_im w_im)
            // odd lane:  Im h = E y_im + (f_re u_im + f_im u_re) + (f_re w_im - f_im w_re)
            // LAWSON: the same without E y
            double h;
            if constexpr (LAWSON) {
                h = fr * u;
            } else {
                h = en * y;
                h = fma(fr, u, h);
            }
            h = fma(fi, up, h);
            h = fma(fr, w, h);
            h = fma(-fi, wp, h);
            const double hp = __shfl_xor(h, 1);
            if constexpr (ROT) {
                // k = conj(R) (-i h) = (cos + i sin)(Im h - i Re h): Re lane cos hp + sin h, Im lane -cos hp + sin h
                const double *pp = phs + (ok ? ((size_t)c * count + gm) * 2 : 0);
                const double pc = pp[0], psn = pp[1];
                if (ok) Ks[idx] = fma(psn, h, (odd ? -pc : pc) * hp);
            } else {
                if (ok && stepping) Ks[idx] = odd ? -hp : hp;
            }
            if constexpr (OBS) {
                const double yy = y * y;
                t0 = fma(y, y, t0);
                t1 = fma(ok ? en : 0.0, yy, t1);
                t2 = fma(y, u, t2);
                t3 = fma(y, up, t3);
            }
        }
        if constexpr (OBS) {
            double t[4] = {t0, t1, t2, odd ? -t3 : t3};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                t[k] += __shfl_xor(t[k], 16);
                t[k] += __shfl_xor(t[k], 32);
                t[k] += __shfl_xor(t[k], 1);
            }
            // As is free after the last barrier of the main loop: [wave][j][scan of the block of 8][k]
            if (lane < 16 && !odd) {
#pragma unroll
                for (int k = 0; k < 4; ++k) As[((wave * TN + j) * 8 + (lane >> 1)) * 4 + k] = t[k];
            }
        }
    }
    if constexpr (OBS) {
        __syncthreads();
        if (tid < TN * 32) {
            const int j = tid >> 5, s8 = (tid >> 2) & 7, k = tid & 3;
            double s = As[((0 * TN + j) * 8 + s8) * 4 + k];
#pragma unroll
            for (int w = 1; w < 4; ++w) s += As[((w * TN + j) * 8 + s8) * 4 + k];
            const int q = ((n0 + j * 16) >> 1) + s8;
            if (q < nscan) part[(((size_t)c * tm + im) * (NC >> 1) + q) * 4 + k] = s;
        }
    }
}

template <int S, int TN>
__global__ __launch_bounds__(256) void tdse_stage_kernel(int count, int NC, int nscan, int tm, int tn, const int *__restrict__ cptr,
                                                        const int *__restrict__ ent, const double *__restrict__ E,
                                                        const double *__restrict__ D, const double *__restrict__ a,
                                                        double *__restrict__ K, size_t kstride, const double *__restrict__ fld,
                                                        StageCoef cf, double dt)
{
    tdse_stage_body<S, TN, false, false>(count, NC, nscan, tm, tn, cptr, ent, E, D, a, K, kstride, fld, cf, dt, nullptr, nullptr);
}

// the Lawson stage: phs = the phases of stage S (unused by stage 0); E is not read
template <int S, int TN>
__global__ __launch_bounds__(256) void tdse_lawson_stage_kernel(int count, int NC, int nscan, int tm, int tn, const int *__restrict__ cptr,
                                                               const int *__restrict__ ent, const double *__restrict__ D,
                                                               const double *__restrict__ a, double *__restrict__ K, size_t kstride,
                                                               const double *__restrict__ fld, StageCoef cf, double dt,
                                                               const double *__restrict__ phs)
{
    tdse_stage_body<S, TN, false, true>(count, NC, nscan, tm, tn, cptr, ent, nullptr, D, a, K, kstride, fld, cf, dt, nullptr, phs);
}

// stage 0 with the measuring epilogue: k_0 exactly as tdse_stage_kernel<0, TN> leaves it (fld == nullptr: no k_0, the measurement alone)
template <int TN>
__global__ __launch_bounds__(256) void tdse_observe_kernel(int count, int NC, int nscan, int tm, int tn, const int *__restrict__ cptr,
                                                          const int *__restrict__ ent, const double *__restrict__ E,
                                                          const double *__restrict__ D, const double *__restrict__ a,
                                                          double *__restrict__ K, const double *__restrict__ fld,
                                                          double *__restrict__ part)
{
    tdse_stage_body<0, TN, true, false>(count, NC, nscan, tm, tn, cptr, ent, E, D, a, K, 0, fld, StageCoef{}, 0.0, part, nullptr);
}

// the observing stage 0 of a Lawson step: the measurement of tdse_observe_kernel, k_0 as tdse_lawson_stage_kernel<0, TN> leaves it
template <int TN>
__global__ __launch_bounds__(256) void tdse_lawson_observe_kernel(int count, int NC, int nscan, int tm, int tn, const int *__restrict__ cptr,
                                                                 const int *__restrict__ ent, const double *__restrict__ E,
                                                                 const double *__restrict__ D, const double *__restrict__ a,
                                                                 double *__restrict__ K, const double *__restrict__ fld,
                                                                 double *__restrict__ part)
{
    tdse_stage_body<0, TN, true, true>(count, NC, nscan, tm, tn, cptr, ent, E, D, a, K, 0, fld, StageCoef{}, 0.0, part, nullptr);
}

// The phase table of a Lawson call, once per call: ph[((s - 1) rows + row) 2 + {0, 1}] = cos, sin of E[row] (c_s dt), s = 1 .. 5,
// both products in fp64 (cdt[s - 1] = c_s dt comes from the host: one rounding).  The entry of s = 4 (c_4 = 1) also serves the step.
struct PhaseCoef { double cdt[5]; };

__global__ __launch_bounds__(256) void tdse_phase_kernel(long long rows, const double *__restrict__ E, PhaseCoef pc, double *__restrict__ ph)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= rows) return;
    const double en = E[t];
#pragma unroll
    for (int s = 0; s < 5; ++s) {
        double sn, cs;
        sincos(en * pc.cdt[s], &sn, &cs);
        ph[((size_t)s * rows + t) * 2] = cs;
        ph[((size_t)s * rows + t) * 2 + 1] = sn;
    }
}

// One thread per (scan, channel): the row-tile partials in ascending tile order, written in the caller's layout row[(q nch + c) 4 + k]
__global__ __launch_bounds__(256) void tdse_obs_reduce_kernel(int nch, int tm, int ncq, int nscan, const double *__restrict__ part,
                                                             double *__restrict__ row)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)nscan * nch) return;
    const int q = (int)(t / nch), c = (int)(t - (long long)q * nch);
    const double *p0 = part + (((size_t)c * tm) * ncq + q) * 4;
    double s[4] = {p0[0], p0[1], p0[2], p0[3]};
    for (int im = 1; im < tm; ++im) {
        const double *pi = p0 + (size_t)im * ncq * 4;
#pragma unroll
        for (int k = 0; k < 4; ++k) s[k] += pi[k];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) row[(size_t)t * 4 + k] = s[k];
}

// ---- the step: a += dt sum_s d_s k_s, the error estimate, the snapshot ------------------------------------------------------
// One thread per (state row, scan): 32 rows x 8 scans per workgroup, the 16 real columns of 8 scans contiguous.  err2[q] (bit
// pattern of a non-negative double) takes the maximum of |sum_s (d_s - b_s) k_s|^2 with an integer atomic maximum: order-independent.
// snap (or null): the new amplitudes in the caller's layout [nscan][nch * count] complex.
// LAWSON: the update and the estimate from the k_s as they are, then a_{n+1} = R_4 .* (the sum), ph4 = the phases of s = 4 [rows][2];
// what is stored and what the snapshot takes is the rotated value.
struct StepCoef { double d[6], e[6]; };

template <bool LAWSON>
__device__ __forceinline__ void tdse_step_body(long long rows, int NC, int nscan, double *__restrict__ a, const double *__restrict__ K,
                                               size_t kstride, const StepCoef &sc, double dt, unsigned long long *__restrict__ err2,
                                               double *__restrict__ snap, const double *__restrict__ ph4)
{
    __shared__ double smax[4][8];
    const int tid = threadIdx.x, ql = tid & 7, lane = tid & 63, wave = tid >> 6;
    const int q = blockIdx.y * 8 + ql;
    const long long row = (long long)blockIdx.x * 32 + (tid >> 3);
    const bool ok = row < rows && 2 * q < NC;
    double m2 = 0.0;
    if (ok) {
        const size_t idx = (size_t)row * NC + 2 * q;
        double s[2], e[2];
#pragma unroll
        for (int ri = 0; ri < 2; ++ri) {
            const double k0 = K[idx + ri];
            s[ri] = sc.d[0] * k0;
            e[ri] = sc.e[0] * k0;
#pragma unroll
            for (int j = 2; j < 6; ++j) {               // the second stage has weight 0 in both formulas
                const double kj = K[(size_t)j * kstride + idx + ri];
                s[ri] = fma(sc.d[j], kj, s[ri]);
                e[ri] = fma(sc.e[j], kj, e[ri]);
            }
            s[ri] = fma(dt, s[ri], a[idx + ri]);
            if constexpr (!LAWSON) a[idx + ri] = s[ri];
        }
        if constexpr (LAWSON) {
            // (cos - i sin)(s_re + i s_im)
            const double pc = ph4[(size_t)row * 2], psn = ph4[(size_t)row * 2 + 1];
            const double re = fma(psn, s[1], pc * s[0]), im = fma(-psn, s[0], pc * s[1]);
            s[0] = re;
            s[1] = im;
            a[idx] = re;
            a[idx + 1] = im;
        }
        m2 = fma(e[0], e[0], e[1] * e[1]);
        if (snap && q < nscan) {
            double *o = snap + ((size_t)q * rows + row) * 2;
            o[0] = s[0];
            o[1] = s[1];
        }
    }
    // maximum over the 8 lanes of a wave with the same scan, then over the 4 waves.  A NaN never wins a comparison here.
#pragma unroll
    for (int sh = 8; sh < 64; sh <<= 1) {
        const double o = __shfl_xor(m2, sh);
        m2 = o > m2 ? o : m2;
    }
    if (lane < 8) smax[wave][lane] = m2;
    __syncthreads();
    if (tid < 8) {
        double m = smax[0][tid];
#pragma unroll
        for (int w = 1; w < 4; ++w) m = smax[w][tid] > m ? smax[w][tid] : m;
        const int qq = blockIdx.y * 8 + tid;
        if (qq < nscan && m > 0.0) atomicMax(&err2[qq], (unsigned long long)__double_as_longlong(m));
    }
}

__global__ __launch_bounds__(256) void tdse_step_kernel(long long rows, int NC, int nscan, double *__restrict__ a,
                                                       const double *__restrict__ K, size_t kstride, StepCoef sc, double dt,
                                                       unsigned long long *__restrict__ err2, double *__restrict__ snap)
{
    tdse_step_body<false>(rows, NC, nscan, a, K, kstride, sc, dt, err2, snap, nullptr);
}

__global__ __launch_bounds__(256) void tdse_lawson_step_kernel(long long rows, int NC, int nscan, double *__restrict__ a,
                                                              const double *__restrict__ K, size_t kstride, StepCoef sc, double dt,
                                                              unsigned long long *__restrict__ err2, double *__restrict__ snap,
                                                              const double *__restrict__ ph4)
{
    tdse_step_body<true>(rows, NC, nscan, a, K, kstride, sc, dt, err2, snap, ph4);
}

// caller's layout a[((q nch + c) count + n) 2 + ri]  <->  working layout; pad columns are written as zeros
__global__ __launch_bounds__(256) void tdse_pack_kernel(long long rows, int NC, int nscan, const double *__restrict__ src, double *__restrict__ dst)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= rows * NC) return;
    const long long row = t / NC;
    const int col = (int)(t - row * NC), q = col >> 1;
    dst[t] = q < nscan ? src[((size_t)q * rows + row) * 2 + (col & 1)] : 0.0;
}

__global__ __launch_bounds__(256) void tdse_unpack_kernel(long long rows, int NC, int nscan, const double *__restrict__ src, double *__restrict__ dst)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= rows * 2 * nscan) return;
    const long long qr = t >> 1;
    const int ri = (int)(t & 1);
    const long long q = qr / rows, row = qr - q * rows;
    dst[t] = src[(size_t)row * NC + 2 * q + ri];
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------
int tdse_columns(int nscan) { return (2 * nscan + 15) / 16 * 16; }

template <int S>
static int launch_stage_s(const TdseDims &d, const TdseBufs &w, const double *fld, double dt, hipStream_t st)
{
    StageCoef cf;
    for (int j = 0; j < 5; ++j) cf.w[j] = TDSE_A[S][j];
    const int tm = (d.count + TBM - 1) / TBM;
    const size_t ks = (size_t)d.nch * d.count * d.NC;
    KScope ks_(KS_TDSE, st);
    const int tn = d.NC == 16 ? 1 : (d.NC + 31) / 32;
    const long long grid = (long long)d.nch * tm * tn;
    if (grid > 0x7fffffffLL) return BSP_ERR_UNSUPPORTED;
    if (w.ph) {
        // Lawson: the phases of stage S (stage 0 has none)
        const double *phs = S > 0 ? w.ph + (size_t)(S - 1) * d.nch * d.count * 2 : nullptr;
        if (d.NC == 16)
            hipLaunchKernelGGL((tdse_lawson_stage_kernel<S, 1>), dim3((unsigned)grid), dim3(256), 0, st, d.count, d.NC, d.nscan, tm, tn, w.cptr,
                               w.ent, w.D, w.a, w.K, ks, fld, cf, dt, phs);
        else
            hipLaunchKernelGGL((tdse_lawson_stage_kernel<S, 2>), dim3((unsigned)grid), dim3(256), 0, st, d.count, d.NC, d.nscan, tm, tn, w.cptr,
                               w.ent, w.D, w.a, w.K, ks, fld, cf, dt, phs);
    } else if (d.NC == 16) {
        hipLaunchKernelGGL((tdse_stage_kernel<S, 1>), dim3((unsigned)grid), dim3(256), 0, st, d.count, d.NC, d.nscan, tm, tn, w.cptr, w.ent,
                           w.E, w.D, w.a, w.K, ks, fld, cf, dt);
    } else {
        hipLaunchKernelGGL((tdse_stage_kernel<S, 2>), dim3((unsigned)grid), dim3(256), 0, st, d.count, d.NC, d.nscan, tm, tn, w.cptr, w.ent,
                           w.E, w.D, w.a, w.K, ks, fld, cf, dt);
    }
    BSP_HIP(hipGetLastError());
    return BSP_OK;
}

int launch_tdse_observe(const TdseDims &d, const TdseBufs &w, const double *fld, double *d_row, hipStream_t st)
{
    const int tm = (d.count + TBM - 1) / TBM;
    {
        KScope ks_(KS_TDSE, st);
        const int tn = d.NC == 16 ? 1 : (d.NC + 31) / 32;
        const long long grid = (long long)d.nch * tm * tn;
        if (grid > 0x7fffffffLL) return BSP_ERR_UNSUPPORTED;
        // a Lawson step's stage 0 leaves another k_0; a measurement alone (fld null) is the same kernel for both schemes
        const bool lawson = w.ph && fld;
        auto kern = d.NC == 16 ? (lawson ? tdse_lawson_observe_kernel<1> : tdse_observe_kernel<1>)
                               : (lawson ? tdse_lawson_observe_kernel<2> : tdse_observe_kernel<2>);
        hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(256), 0, st, d.count, d.NC, d.nscan, tm, tn, w.cptr, w.ent, w.E, w.D, w.a, w.K, fld,
                           w.part);
        BSP_HIP(hipGetLastError());
    }
    const long long blocks = ((long long)d.nscan * d.nch + 255) / 256;
    if (blocks > 0x7fffffffLL) return BSP_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(tdse_obs_reduce_kernel, dim3((unsigned)blocks), dim3(256), 0, st, d.nch, tm, d.NC / 2, d.nscan, w.part, d_row);
    BSP_HIP(hipGetLastError());
    return BSP_OK;
}

int launch_tdse_step(const TdseDims &d, const TdseBufs &w, const double *d_field, double dt, double *d_snap, double *d_obs, hipStream_t st)
{
    const size_t fs = (size_t)2 * d.nscan;
    int rc;
    if ((rc = d_obs ? launch_tdse_observe(d, w, d_field, d_obs, st) : launch_stage_s<0>(d, w, d_field, dt, st)) ||
        (rc = launch_stage_s<1>(d, w, d_field + fs, dt, st)) ||
        (rc = launch_stage_s<2>(d, w, d_field + 2 * fs, dt, st)) || (rc = launch_stage_s<3>(d, w, d_field + 3 * fs, dt, st)) ||
        (rc = launch_stage_s<4>(d, w, d_field + 4 * fs, dt, st)) || (rc = launch_stage_s<5>(d, w, d_field + 5 * fs, dt, st)))
        return rc;
    StepCoef sc;
    for (int j = 0; j < 6; ++j) { sc.d[j] = TDSE_D[j]; sc.e[j] = TDSE_D[j] - TDSE_B[j]; }
    const long long rows = (long long)d.nch * d.count;
    const long long gx = (rows + 31) / 32;
    const int gy = (d.NC / 2 + 7) / 8;
    if (gx > 0x7fffffffLL || gy > 65535) return BSP_ERR_UNSUPPORTED;
    if (w.ph)
        hipLaunchKernelGGL(tdse_lawson_step_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, st, rows, d.NC, d.nscan, w.a, w.K,
                           (size_t)rows * d.NC, sc, dt, w.err2, d_snap, w.ph + (size_t)3 * rows * 2);
    else
        hipLaunchKernelGGL(tdse_step_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, st, rows, d.NC, d.nscan, w.a, w.K,
                           (size_t)rows * d.NC, sc, dt, w.err2, d_snap);
    BSP_HIP(hipGetLastError());
    return BSP_OK;
}

int launch_tdse_phases(const TdseDims &d, const double *d_E, double dt, double *d_ph, hipStream_t st)
{
    const double c[5] = {2.0 / 9.0, 1.0 / 3.0, 3.0 / 4.0, 1.0, 5.0 / 6.0};      // c_1 .. c_5: the doubles nearest the fractions
    PhaseCoef pc;
    for (int s = 0; s < 5; ++s) pc.cdt[s] = c[s] * dt;
    const long long rows = (long long)d.nch * d.count, blocks = (rows + 255) / 256;
    if (blocks > 0x7fffffffLL) return BSP_ERR_UNSUPPORTED;
    KScope ks_(KS_TDSE, st);
    hipLaunchKernelGGL(tdse_phase_kernel, dim3((unsigned)blocks), dim3(256), 0, st, rows, d_E, pc, d_ph);
    BSP_HIP(hipGetLastError());
    return BSP_OK;
}

int launch_tdse_pack(const TdseDims &d, const double *d_user, double *d_work, hipStream_t st)
{
    const long long rows = (long long)d.nch * d.count, total = rows * d.NC, blocks = (total + 255) / 256;
    if (blocks > 0x7fffffffLL) return BSP_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(tdse_pack_kernel, dim3((unsigned)blocks), dim3(256), 0, st, rows, d.NC, d.nscan, d_user, d_work);
    BSP_HIP(hipGetLastError());
    return BSP_OK;
}

int launch_tdse_unpack(const TdseDims &d, const double *d_work, double *d_user, hipStream_t st)
{
    const long long rows = (long long)d.nch * d.count, total = rows * 2 * d.nscan, blocks = (total + 255) / 256;
    if (blocks > 0x7fffffffLL) return BSP_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(tdse_unpack_kernel, dim3((unsigned)blocks), dim3(256), 0, st, rows, d.NC, d.nscan, d_work, d_user);
    BSP_HIP(hipGetLastError());
    return BSP_OK;
}

}  // namespace bsp
