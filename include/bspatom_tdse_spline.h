/* bspatom_tdse_spline.h -- the spline-basis TDSE entry points of libbspatom.  Part of bspatom.h, which includes it inside its
 * extern "C" block after the types it needs: include bspatom.h, not this file. */
#ifndef BSPATOM_H
#error "include bspatom.h: bspatom_tdse_spline.h is a part of it"
#endif
#ifndef BSPATOM_TDSE_SPLINE_H
#define BSPATOM_TDSE_SPLINE_H

/* The TDSE in the B-spline basis itself: Crank-Nicolson steps on the coupled banded LU (csrc/tdse_spline.hip).  The calls above
 * integrate in the basis of field-free eigenstates and see the continuum their window of states holds; this one propagates
 *     i S dc/dt = (sum_c (H_{l_c} - i W_c) + V(t)) c
 * on the banded pencil, with no eigenvector, the whole continuum of the box, any absorber and any coupling between the channels.  With
 * tau = dt/2 and A_n the right-hand operator at t_n + dt/2, the step (S + i tau A_n) c_{n+1} = (S - i tau A_n) c_n is
 *     M_n = A_n - z S,  z = 2i/dt:       c_{n+1} = -(4i/dt) M_n^-1 (S c_n) - c_n,
 * and M_n is bspatom_resolvent_coupled's matrix.  The scheme is unconditionally stable -- the spectrum of the pencil does not limit dt --
 * and conserves c^H S c exactly for a Hermitian problem.
 * The problem, shared by all scans and steps, is described as for bspatom_resolvent_coupled, one record of channels: l[c], w[c] (NULL and
 * -1 as there), WB (nabs full bands), the topology cr, cc, ctr of ncoup entries, GB (nop full bands); the ordering i*nch + c, the
 * half-width bw = nch*k - 1 <= BSPATOM_COUPLED_MAX_BAND, beyond it BSPATOM_ERR_UNSUPPORTED with the limit on stderr.
 *   coef[(((n*nscan + q)*ncoup + p)*nop + o)*2 + {0,1}]: the complex coefficient of entry p and operator o during step n of scan q: what
 *     a is to bspatom_resolvent_coupled with m = n*nscan + q.  The library never evaluates a pulse: the caller puts F(t_n + dt/2) times the
 *     angular factor there; a static entry repeats its value; a Hermitian coupling is two entries, the second transposed with the
 *     conjugate coefficient.
 *   c[((q*nch + ch)*nfun + i)*2 + {0,1}]: c(t0) of scan q on entry, c(t0 + nsteps dt) on return.
 *   snap[(((s*nscan + q)*nch + ch)*nfun + i)*2 + {0,1}], s < nsteps / snap_every: the packets after every snap_every-th step, as in the
 *     other TDSE calls; may be NULL.
 *   obs: rows for the steps n = 0, obs_every, .. < nsteps and always n = nsteps as the last (nobs as in bspatom_tdse_observe; nsteps = 0 is
 *     a real call that only measures), obs[(j*nscan + q)*(nch + 2*nproj) + k], all from b = S c_n, which the step forms anyway:
 *       k = ch < nch             N_ch = Re sum_i conj(c(i,ch)) b(i,ch): the norm per channel; its loss under an absorber is the yield;
 *       k = nch + 2r, + 2r + 1   Re, Im of sum_ch sum_i P_r(i,ch) b(i,ch), P[(r*nch + ch)*nfun + i] complex, channel-major as in the coupled
 *                                call: bilinear, no conjugate.  With P a real eigenvector placed in its channel: the amplitude in that
 *                                state along the run, without a snapshot.
 *     The dipole expectation c^H V c is not among them: it needs V c, which the step does not hold.
 *   info[q]: the pivots replaced, summed over the steps; 0 for any finite dt and W >= 0.
 * The arithmetic, fixed:
 *   1. b = S c per channel and component by bspatom_resolvent_chain's rule for y = A x with A = S: the sum starts at +0.0 and adds
 *      S(i,i+d) * x(i+d) for d = -(k-1) .. k-1 ascending, terms outside 0..nfun-1 skipped; IEEE multiply and add, no FMA, Re and Im
 *      independently; S(i,j) = SB[|d|*nfun + min(i,j)] of the problem's own upper band, the band the coupled matrix reads.
 *   2. M is bspatom_resolvent_coupled's entry with z = (0.0, 2.0/dt) on every channel -- 2.0/dt one fp64 division on the host -- and the
 *      step's coefficients; then its pivot threshold, its factorisation and its solve: the same statements (csrc/resolvent_coupled_lu.h),
 *      not copies.
 *   3. with g = 4.0/dt from the host:  c'_re = g*x_im - c_re,  c'_im = -(g*x_re) - c_im: one multiply and one subtract each, no FMA.
 * How: a persistent grid, one workgroup of the coupled kernel's shape per work slot ("resolvent_slots" applies), takes the scans by
 * static stride and runs a scan's steps one after the other: a packet stays on one workgroup, nothing goes to the host between steps, no
 * workgroup waits on another, no atomics.  Slot scratch is the coupled call's; c lives in the caller's array (or its staging copy).  The
 * host enqueues launches of at most 64 steps (bspatom_set_option("tdse_spline_group", g) sets another length), so that no launch runs
 * for seconds.  The host variant stages coef, the snapshots and the rows by groups of steps under tdse_stage_mb, one step at least.
 * Guarantees:
 *   (S1) results are bit-identical from run to run;
 *   (S2) a scan's c, snapshots, rows and info depend on its own packet and coefficients and on the shared description alone: not on nscan,
 *        the other scans, the work slots, tdse_spline_group, tdse_stage_mb, obs_every, snap_every, nproj, or host versus _dev;
 *   (S3) composition: one step equals, bit for bit in c and with info adding up, the band product b = S c of rule 1 (host.band_apply on
 *        the symmetric full band of SB), bspatom_resolvent_coupled at z = 2i/dt with B = b and a = the step's coefficients, and the two
 *        operations of rule 3;
 *   (S4) a snapshot equals the result of the shorter run, and a run continued from a snapshot equals the long run;
 *   (S5) the last row has the bits of a call with nsteps = 0 on the returned c.
 * NOT promised: the result is second order in dt, an approximation; nothing stays real (z is imaginary); it is not bit-equal to any
 * eigenbasis call -- another equation of motion in another basis, the same physics to O(dt^2) and to the window of states of the other.
 * BSPATOM_ERR_ARG: what bspatom_resolvent_coupled names for l, w, WB and the topology; nscan < 1; nsteps < 0; a dt that is not finite or
 * not positive; coef NULL with nsteps > 0 and ncoup > 0; c or info NULL; snap_every < 0; snap given with snap_every = 0; obs_every < 0; obs
 * given with obs_every = 0; obs_every >= 1 with obs NULL; nproj < 0; nproj > 0 with P NULL while rows are asked for.
 * The _dev variant: WB, GB, coef, c, snap, P, obs in device memory of the problem's device; l, w, cr, cc, ctr, info stay host pointers. */
int bspatom_tdse_spline(bspatom_problem *p, int nscan, int nch, const int32_t *l, int nabs, const double *WB, const int32_t *w, int ncoup,
                        const int32_t *cr, const int32_t *cc, const int32_t *ctr, int nop, const double *GB, int nsteps, double dt,
                        const double *coef, double *c, int snap_every, double *snap, int obs_every, int nproj, const double *P, double *obs,
                        int32_t *info);
int bspatom_tdse_spline_dev(bspatom_problem *p, int nscan, int nch, const int32_t *l, int nabs, const double *WB_dev, const int32_t *w,
                            int ncoup, const int32_t *cr, const int32_t *cc, const int32_t *ctr, int nop, const double *GB_dev, int nsteps,
                            double dt, const double *coef_dev, double *c_dev, int snap_every, double *snap_dev, int obs_every, int nproj,
                            const double *P_dev, double *obs_dev, int32_t *info);

/* The same call on the blocked LU for wide bands (csrc/tdse_spline_wide.hip): the 24 arguments, the layouts, the rows, the arithmetic
 * rules 1 and 3 and the error returns of bspatom_tdse_spline; what differs:
 *   the limit   any half-width bw = nch*k - 1 from 1 to BSPATOM_COUPLED_WIDE_MAX_BAND = 255 (28 channels at k = 9, 16 at k = 16); beyond it
 *               BSPATOM_ERR_UNSUPPORTED with that limit on stderr.  bspatom_tdse_spline is not rerouted: it keeps its limit and its bits.
 *   rule 2      M is bspatom_resolvent_coupled_wide's entry, pivot threshold, factorisation and solve with ONE right-hand side: the same
 *               statements (csrc/resolvent_wide_lu.h), not copies.  Guarantees S1 - S5 hold with "bspatom_resolvent_coupled" read as
 *               "bspatom_resolvent_coupled_wide": in S3 one step equals the band product, bspatom_resolvent_coupled_wide at z = 2i/dt with
 *               nrhs = 1, B = b and a = the step's coefficients, and the two operations of rule 3, bit for bit.
 *   how         one workgroup of the wide kernel's shape per work slot; the slot scratch is the wide call's with one vector.
 *   launches    a wide step takes tens to hundreds of milliseconds, so 64 steps per launch would run for most of a minute.  Unless
 *               "tdse_spline_group" is set, a launch takes the largest g in 1 .. 64 with
 *                   g * ceil(nscan/slots) * 16 * N * bw^2 flop <= 27.6e9,   N = nch*nfun,
 *               two seconds at 13.8 Gflop/s per CU, the slowest rate measured for this LU under its model 8 N bw (2 bw).  The option
 *               overrides it; nothing computed depends on either (S2).
 * NOT promised, beside what bspatom_tdse_spline does not promise: equality with bspatom_tdse_spline where both apply (bw <= 63) -- another
 * elimination order, the same backward error class. */
int bspatom_tdse_spline_wide(bspatom_problem *p, int nscan, int nch, const int32_t *l, int nabs, const double *WB, const int32_t *w, int ncoup,
                             const int32_t *cr, const int32_t *cc, const int32_t *ctr, int nop, const double *GB, int nsteps, double dt,
                             const double *coef, double *c, int snap_every, double *snap, int obs_every, int nproj, const double *P,
                             double *obs, int32_t *info);
int bspatom_tdse_spline_wide_dev(bspatom_problem *p, int nscan, int nch, const int32_t *l, int nabs, const double *WB_dev, const int32_t *w,
                                 int ncoup, const int32_t *cr, const int32_t *cc, const int32_t *ctr, int nop, const double *GB_dev,
                                 int nsteps, double dt, const double *coef_dev, double *c_dev, int snap_every, double *snap_dev,
                                 int obs_every, int nproj, const double *P_dev, double *obs_dev, int32_t *info);

#endif
