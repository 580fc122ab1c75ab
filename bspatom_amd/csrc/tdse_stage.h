// tdse_stage.h -- the stage and the step of the TDSE (tdse.hip, tdse_static.hip, tdse_fields.hip, tdse_adapt.hip): one body each for
// every scheme, instantiated by the kernels of these files.  Device code only.
#pragma once
#include "common.h"
#include "mfma_tile.h"

namespace bsp {

constexpr int TBK = 16, TBM = 64, TLDA = TBM + 16;

struct StageCoef { double w[5]; };          // A_s0 .. A_s,s-1
template <bool STAT, int TN> struct StatAcc { double4_t v[1][TN]; };        // the accumulator of the static entries, absent without STAT
template <int TN> struct StatAcc<false, TN> {};
// the accumulator pairs of the fields 1 .. NX (bspatom_tdse_fields), absent with one field
template <int NX, int TN> struct FieldAcc { double4_t t[NX][1][TN], n[NX][1][TN]; };
template <int TN> struct FieldAcc<0, TN> {};

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
//
// STAT (bspatom_tdse_static): behind its driven entries the channel's list holds its static entries in ascending j, ent[3e] = j,
// [3e+1] = si[j], [3e+2] = 2 + skind[j]; the block is W + j count^2, walked like an entry with cf[p] = c (accS += W_j^T y_si).  Kind 1,
// -i W^T y = W^T (-i y): the B tile takes -i y = (y_im, -y_re), the neighbour column through __shfl_xor(.., 1), so both kinds run the
// same real product into the one accumulator accS, which the field never touches: h += accS where the channel has a static entry
// (a channel without one computes what the kernels without STAT compute).  OBS: two more chains t4, t5 on y and accS, reduced like
// t2, t3, are s_c = conj(a_c) . S_c; the partials are 6 doubles wide.
//
// NF > 1 (bspatom_tdse_fields, always with STAT): a driven entry carries its field in ent[3e+2] = 4 g + {0, 1} (a static entry stays 2 or
// 3; with g = 0 the list is what the other kernels read), and every field g >= 1 has its own pair accX.t[g - 1], accX.n[g - 1] beside
// accT, accN of field 0: an entry's products go into the pair of its field, so an accumulator sees its field's entries in ascending p
// as if the others were not there.  fld holds this stage's values [g][nscan][2]; the epilogue chains the fields in ascending g,
// h = ((E y + f_0 ..) + f_1 ..) + .., each field's four terms in the order above, accS behind them.  OBS: two more chains per field
// g >= 1 on y and its accT, reduced like t2, t3, are z_{c,g}; the partials are 4 + 2 NF doubles wide: [0 .. 3] as ever (z of field
// 0), [4, 5] = s_c, [4 + 2 g, 5 + 2 g] = z_{c,g}.
template <int NF> __device__ __forceinline__ int ent_kind(int kd)
{
    if constexpr (NF > 1) return kd & 3;
    else return kd;
}

//
// ADAPT (bspatom_tdse_adaptive, tdse_adapt.hip; always with STAT, NF = 1): the step size, the field and the phase table of the attempt
// come from the control block ctl: dt = ldexp(dt, -ctl->m) after one uniform load, fld = the block's six values per scan, phs moves
// phlev doubles per level, and a launch enqueued behind the end of the run returns at once.  Everything after that is the code above.
template <int S, int TN, bool OBS, bool LAWSON, bool STAT = false, int NF = 1, bool ADAPT = false>
__device__ __forceinline__ void tdse_stage_body(int count, int NC, int nscan, int tm, int tn, const int *__restrict__ cptr,
                                                const int *__restrict__ ent, const double *__restrict__ E,
                                                const double *__restrict__ D, const double *__restrict__ a,
                                                double *__restrict__ K, size_t kstride, const double *__restrict__ fld,
                                                StageCoef cf, double dt, double *__restrict__ part, const double *__restrict__ phs,
                                                const double *__restrict__ Wst = nullptr, const TdseAdaptCtl *__restrict__ ctl = nullptr,
                                                size_t phlev = 0)
{
    static_assert(!OBS || S == 0, "only stage 0 runs on a(t_n)");
    static_assert(NF == 1 || STAT, "several fields run with the static accumulator");
    static_assert(!ADAPT || (STAT && NF == 1), "the adaptive call runs the static stage with one field");
    if constexpr (ADAPT) {
        if (ctl->done) return;
        const int lev = ctl->m;
        dt = ldexp(dt, -lev);
        fld = tdse_ctl_fld(ctl) + (size_t)S * 2 * nscan;
        if constexpr (LAWSON && S > 0) phs += (size_t)lev * phlev;
    }
    constexpr int PW = NF > 1 ? 4 + 2 * NF : STAT ? 6 : 4;                    // doubles of a partial
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

    double4_t accT[1][TN], accN[1][TN];                                       // field 0; accX.t[g - 1], accX.n[g - 1]: field g >= 1
    [[maybe_unused]] StatAcc<STAT, TN> accS;
    [[maybe_unused]] FieldAcc<NF - 1, TN> accX;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        accT[0][j] = (double4_t){0.0, 0.0, 0.0, 0.0};
        accN[0][j] = (double4_t){0.0, 0.0, 0.0, 0.0};
        if constexpr (STAT) accS.v[0][j] = (double4_t){0.0, 0.0, 0.0, 0.0};
        if constexpr (NF > 1) {
#pragma unroll
            for (int g = 0; g < NF - 1; ++g) {
                accX.t[g][0][j] = (double4_t){0.0, 0.0, 0.0, 0.0};
                accX.n[g][0][j] = (double4_t){0.0, 0.0, 0.0, 0.0};
            }
        }
    }
    // the static entries come last: the channel has one exactly if its last entry is one
    [[maybe_unused]] bool has_s = false;
    if constexpr (STAT) has_s = e1 > e0 && ent_kind<NF>(ent[3 * (e1 - 1) + 2]) >= 2;

    double ra[4], rb[BEL][S + 1];
    [[maybe_unused]] double rc[ROT ? BEL : 1], rs[ROT ? BEL : 1];                            // cos, +- sin (+ on the Re lane) of the B-tile rows
    // the loads of iteration it = (entry, k-step): A tile 64 x 16 of D_p (either orientation), B tile 16 x NB of y of the other channel
    auto load = [&](int it) {
        const int e = e0 + it / ksteps, k0 = (it % ksteps) * TBK;
        const int p = ent[3 * e], oc = ent[3 * e + 1], kd = ent[3 * e + 2];
        const int nrm = STAT ? ent_kind<NF>(kd) == 1 : kd;
        const double *Dp = D + (size_t)p * blk;
        if constexpr (STAT) {
            if (ent_kind<NF>(kd) >= 2) Dp = Wst + (size_t)p * blk;
        }
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
        return kd;
    };
    auto store = [&](int kd) {
        const int nrm = STAT ? ent_kind<NF>(kd) == 1 : kd;
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
            if constexpr (STAT) {
                double yv = form_y<S>(rb[r], cf, dt);
                if constexpr (ROT) yv = fma(rs[r], __shfl_xor(yv, 1), rc[r] * yv);
                // kind 1: -i y, Re lane y_im, Im lane -y_re
                const double yo = __shfl_xor(yv, 1);
                Bs[kk * TLDB + (cc ^ lds_swz(kk))] = kd == 3 ? ((tid & 1) ? -yo : yo) : yv;
            } else if constexpr (ROT) {
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
        if constexpr (NF > 1) {
            // the accumulator of the entry's field, by uniform branches (an index would put the accumulators into scratch)
            auto mm = [&](double4_t (&acc)[1][TN]) {
#pragma unroll
                for (int k4 = 0; k4 < TBK / 4; ++k4) {
                    const int kr = k4 * 4 + (lane >> 4);
                    mfma_step<1, TN>(&As[kr * TLDA + wave * 16], &Bs[kr * TLDB], lane, kr, acc);
                }
            };
            const int kind = cur & 3, g = cur >> 2;
            if (kind >= 2) {
                mm(accS.v);
            } else {
                if (g == 0) {
                    if (kind) mm(accN);
                    else mm(accT);
                }
#pragma unroll
                for (int gg = 1; gg < NF; ++gg) {
                    if (g == gg) {
                        if (kind) mm(accX.n[gg - 1]);
                        else mm(accX.t[gg - 1]);
                    }
                }
            }
        } else if (STAT && cur >= 2) {
            if constexpr (STAT) {
#pragma unroll
                for (int k4 = 0; k4 < TBK / 4; ++k4) {
                    const int kr = k4 * 4 + (lane >> 4);
                    mfma_step<1, TN>(&As[kr * TLDA + wave * 16], &Bs[kr * TLDB], lane, kr, accS.v);
                }
            }
        } else if (cur) {
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
        // the fields g >= 1: fld[(g nscan + q) 2 + {0, 1}], selected like field 0's
        [[maybe_unused]] double frg[NF], fig[NF];
        if constexpr (NF > 1) {
#pragma unroll
            for (int g = 1; g < NF; ++g) {
                const size_t at = fok ? ((size_t)g * nscan + q) * 2 : 0;
                const double gre = stepping ? fld[at] : 0.0, gim = stepping ? fld[at + 1] : 0.0;
                frg[g] = fok ? gre : 0.0;
                fig[g] = fok ? (odd ? gim : -gim) : 0.0;
            }
        }
        double t0 = 0.0, t1 = 0.0, t2 = 0.0, t3 = 0.0;
        [[maybe_unused]] double t4 = 0.0, t5 = 0.0;
        [[maybe_unused]] double tz[NF][2];
        if constexpr (NF > 1 && OBS) {
#pragma unroll
            for (int g = 1; g < NF; ++g) tz[g][0] = tz[g][1] = 0.0;
        }
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
            if constexpr (NF > 1) {
#pragma unroll
                for (int g = 1; g < NF; ++g) {
                    const double ug = accX.t[g - 1][0][j][r], wg = accX.n[g - 1][0][j][r];
                    const double ugp = __shfl_xor(ug, 1), wgp = __shfl_xor(wg, 1);
                    h = fma(frg[g], ug, h);
                    h = fma(fig[g], ugp, h);
                    h = fma(frg[g], wg, h);
                    h = fma(-fig[g], wgp, h);
                    if constexpr (OBS) {
                        tz[g][0] = fma(y, ug, tz[g][0]);
                        tz[g][1] = fma(y, ugp, tz[g][1]);
                    }
                }
            }
            [[maybe_unused]] double sv = 0.0;
            if constexpr (STAT) {
                sv = accS.v[0][j][r];
                h = has_s ? h + sv : h;
            }
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
                if constexpr (STAT) {
                    t4 = fma(y, sv, t4);
                    t5 = fma(y, __shfl_xor(sv, 1), t5);
                }
            }
        }
        if constexpr (OBS) {
            double t[PW] = {t0, t1, t2, odd ? -t3 : t3};
            if constexpr (STAT) {
                t[4] = t4;
                t[5] = odd ? -t5 : t5;
            }
            if constexpr (NF > 1) {
#pragma unroll
                for (int g = 1; g < NF; ++g) {
                    t[4 + 2 * g] = tz[g][0];
                    t[5 + 2 * g] = odd ? -tz[g][1] : tz[g][1];
                }
            }
#pragma unroll
            for (int k = 0; k < PW; ++k) {
                t[k] += __shfl_xor(t[k], 16);
                t[k] += __shfl_xor(t[k], 32);
                t[k] += __shfl_xor(t[k], 1);
            }
            // As is free after the last barrier of the main loop: [wave][j][scan of the block of 8][k]
            if (lane < 16 && !odd) {
#pragma unroll
                for (int k = 0; k < PW; ++k) As[((wave * TN + j) * 8 + (lane >> 1)) * PW + k] = t[k];
            }
        }
    }
    if constexpr (OBS) {
        __syncthreads();
        if constexpr (STAT) {
            if (tid < TN * 8 * PW) {
                const int j = tid / (8 * PW), s8 = tid / PW % 8, k = tid % PW;
                double s = As[((0 * TN + j) * 8 + s8) * PW + k];
#pragma unroll
                for (int w = 1; w < 4; ++w) s += As[((w * TN + j) * 8 + s8) * PW + k];
                const int q = ((n0 + j * 16) >> 1) + s8;
                if (q < nscan) part[(((size_t)c * tm + im) * (NC >> 1) + q) * PW + k] = s;
            }
        } else if (tid < TN * 32) {
            const int j = tid >> 5, s8 = (tid >> 2) & 7, k = tid & 3;
            double s = As[((0 * TN + j) * 8 + s8) * 4 + k];
#pragma unroll
            for (int w = 1; w < 4; ++w) s += As[((w * TN + j) * 8 + s8) * 4 + k];
            const int q = ((n0 + j * 16) >> 1) + s8;
            if (q < nscan) part[(((size_t)c * tm + im) * (NC >> 1) + q) * 4 + k] = s;
        }
    }
}

// ---- the step: a += dt sum_s d_s k_s, the error estimate, the snapshot ------------------------------------------------------
// One thread per (state row, scan): 32 rows x 8 scans per workgroup, the 16 real columns of 8 scans contiguous.  err2[q] (bit
// pattern of a non-negative double) takes the maximum of |sum_s (d_s - b_s) k_s|^2 with an integer atomic maximum: order-independent.
// snap (or null): the new amplitudes in the caller's layout [nscan][nch * count] complex.
// LAWSON: the update and the estimate from the k_s as they are, then a_{n+1} = R_4 .* (the sum), ph4 = the phases of s = 4 [rows][2];
// what is stored and what the snapshot takes is the rotated value.
// ADAPT (bspatom_tdse_adaptive): dt = ldexp(dt, -ctl->m), ph4 moves phlev doubles per level, the new amplitudes go to the candidate
// buffer cand instead of a (tdse_adapt_commit_kernel copies them and writes the snapshot once the step is accepted), and a launch
// behind the end of the run returns at once.  The arithmetic is the one above.
struct StepCoef { double d[6], e[6]; };

template <bool LAWSON, bool ADAPT = false>
__device__ __forceinline__ void tdse_step_body(long long rows, int NC, int nscan, double *__restrict__ a, const double *__restrict__ K,
                                               size_t kstride, const StepCoef &sc, double dt, unsigned long long *__restrict__ err2,
                                               double *__restrict__ snap, const double *__restrict__ ph4,
                                               const TdseAdaptCtl *__restrict__ ctl = nullptr, size_t phlev = 0,
                                               double *__restrict__ cand = nullptr)
{
    if constexpr (ADAPT) {
        if (ctl->done) return;
        const int lev = ctl->m;
        dt = ldexp(dt, -lev);
        if constexpr (LAWSON) ph4 += (size_t)lev * phlev;
    }
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
            if constexpr (!LAWSON) {
                if constexpr (ADAPT) cand[idx + ri] = s[ri];
                else a[idx + ri] = s[ri];
            }
        }
        if constexpr (LAWSON) {
            // (cos - i sin)(s_re + i s_im)
            const double pc = ph4[(size_t)row * 2], psn = ph4[(size_t)row * 2 + 1];
            const double re = fma(psn, s[1], pc * s[0]), im = fma(-psn, s[0], pc * s[1]);
            s[0] = re;
            s[1] = im;
            if constexpr (ADAPT) {
                cand[idx] = re;
                cand[idx + 1] = im;
            } else {
                a[idx] = re;
                a[idx + 1] = im;
            }
        }
        m2 = fma(e[0], e[0], e[1] * e[1]);
        if (!ADAPT && snap && q < nscan) {
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

}  // namespace bsp
