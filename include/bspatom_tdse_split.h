/* bspatom_tdse_split.h -- the split-step spline-basis TDSE entry points of libbspatom.  Part of bspatom.h, which includes it inside its
 * extern "C" block after the types it needs: include bspatom.h, not this file. */
#ifndef BSPATOM_H
#error "include bspatom.h: bspatom_tdse_split.h is a part of it"
#endif
#ifndef BSPATOM_TDSE_SPLIT_H
#define BSPATOM_TDSE_SPLIT_H

/* The TDSE in the B-spline basis by split Crank-Nicolson steps (csrc/tdse_split.hip).  bspatom_tdse_spline factors the whole coupled
 * matrix, of half-width nch*k - 1, on every step: O(N (nch k)^2) per step, nch capped by the half-width limit, one workgroup per packet.
 * This call propagates
 *     i S dc/dt = (sum_c (H_{l_c} - i W_c) + f(t) A (x) G) c
 * with ONE operator term -- a constant real symmetric nch x nch angular matrix A = Q diag(lam) Q^T, Q orthogonal, and one radial band G
 * -- by the symmetric splitting the grid codes use: the atomic part is block-diagonal in the channels and constant in time, the field
 * term is block-diagonal in the eigenbasis of A.  Every substep is nch independent complex banded systems of half-width k - 1, one
 * wavefront each: O(nch N k^2) per step, the channels side by side on the CUs, the atomic factorisation once per call, nch limited by
 * memory alone.  The splitting is second order in dt, like the unsplit step.
 * The channels are described as for bspatom_tdse_spline: l[c], w[c] (NULL and -1 as there), WB (nabs full bands); nscan, nsteps, dt, c,
 * snap_every, snap, obs_every, nproj, P, obs, info as there, layouts included.  New:
 *   G            one full band [2k-1][nfun], G[(d + k-1)*nfun + i] = G(i, i + d) (bspatom_dipole_bands' band of r for the length gauge)
 *   Q[c*nch + j] the mixing matrix: column j is the j-th eigenvector of A;  lam[j] its eigenvalue
 *   f[(n*nscan + q)*2 + {0,1}]   the complex field value of step n and scan q, at the step's midpoint.  The library never evaluates a pulse.
 * One step of one scan, with tau = dt/4 and A_c = H_{l_c} - i W_c:
 *   1. atomic half step, every channel c on its own: b = S c_c by rule 1 of bspatom_tdse_spline.h; x = M_c^-1 b, M_c = A_c - z S, z = 4i/dt
 *      (4.0/dt one fp64 division on the host); with g = 8.0/dt from the host c_re <- g*x_im - c_re, c_im <- -(g*x_re) - c_im, one
 *      multiply and one subtract each, no FMA: the Cayley form of exp(-i S^-1 A_c dt/2).  M_c depends on (l_c, w_c, dt) alone: it is
 *      factored once per call and distinct (l_c, w_c); the steps run the two substitutions.
 *   2. field step, every eigenchannel j on its own: d_j = sum_c Q(c,j) c_c, c ascending from +0.0, multiply then add, no FMA, Re and Im
 *      independently; mu = (f_re*lam_j, f_im*lam_j); N_j = S + i (dt/2) mu G with h = 0.5*dt from the host: Re N = S + (-(h*mu_im))*G,
 *      Im N = (h*mu_re)*G; b = S d_j by rule 1; d_j <- 2*x - d_j with x = N_j^-1 b, one multiply and one subtract, no FMA.  N_j changes
 *      with the step and is factored every time.
 *   3. back: c_c = sum_j Q(c,j) d_j, j ascending, as in 2; then the atomic half step 1 again.
 * The factorisations pivot by |Re| + |Im| with ties to the smallest row; the pivot threshold, the reciprocal and the replacement of a
 * zero pivot are bspatom_resolvent's (csrc/resolvent_shared.h).
 * Rows: the nch + 2*nproj entries of bspatom_tdse_spline, from b = S c_n of the FIRST atomic half step of step n: N_ch per channel
 * (lane-strided partial sums over i ascending, then the wave's fixed tree), the projections as the sum over the channels ascending,
 * from +0.0, of each channel's own p_r^T b.  nsteps = 0 is a real call that only measures.
 * info[q]: the pivots replaced over the run: those of the field factorisations of scan q, summed over the steps and eigenchannels,
 * plus, when nsteps > 0, those of the call's atomic factorisations; 0 for any finite dt, W >= 0 and finite f.
 * How: a persistent grid of single-wave workgroups ("resolvent_slots" applies) takes the nscan*nch systems of a substep by static
 * stride; a step is three launches -- atomic, field, atomic -- on two packet buffers that alternate, the mixing with Q folded into the
 * operand loads of the second and third; no workgroup waits on another, no atomics.  The host enqueues the launches of 64 steps
 * (bspatom_set_option("tdse_split_group", g) sets another number) and waits for them before the next.  The host variant stages f, the
 * snapshots and the rows by groups of steps under tdse_stage_mb, one step at least.
 * The limit: k <= 16, the one-wave window's as in bspatom_resolvent; beyond it BSPATOM_ERR_UNSUPPORTED with the limit on stderr.
 * Guarantees, bitwise:
 *   (P1) results are identical from run to run;
 *   (P2) a scan's c, snapshots, rows and info depend on its own packet and f and on the shared description alone: not on nscan, the other
 *        scans, the work slots, tdse_split_group, tdse_stage_mb, obs_every, snap_every, nproj, or host versus _dev;
 *   (P3) a snapshot equals the result of the shorter run, and a run continued from a snapshot equals the long run;
 *   (P4) the last row has the bits of a call with nsteps = 0 on the returned c.
 * NOT promised: equality with bspatom_tdse_spline -- another approximation of the same equation, the two differ at O(dt^2) --; equality
 * of a substep with bspatom_resolvent; unitarity for a complex f (with no absorber and a real f every factor is S-unitary and c^H S c
 * is conserved).
 * BSPATOM_ERR_ARG: what bspatom_tdse_spline names for p, l, w, nabs, WB, nscan, nch, nsteps, dt, c, info, snap_every, snap, obs_every,
 * obs, nproj, P; G, Q, lam or f NULL with nsteps > 0.
 * The _dev variant: WB, G, f, c, snap, P, obs in device memory of the problem's device; l, w, Q, lam, info stay host pointers.
 * The same call with expectation values <c| B (x) G |c> -- the dipole, the acceleration -- behind the entries of every row:
 * bspatom_tdse_split_observe in bspatom_spline_expect.h. */
int bspatom_tdse_split(bspatom_problem *p, int nscan, int nch, const int32_t *l, int nabs, const double *WB, const int32_t *w, const double *G,
                       const double *Q, const double *lam, int nsteps, double dt, const double *f, double *c, int snap_every, double *snap,
                       int obs_every, int nproj, const double *P, double *obs, int32_t *info);
int bspatom_tdse_split_dev(bspatom_problem *p, int nscan, int nch, const int32_t *l, int nabs, const double *WB_dev, const int32_t *w,
                           const double *G_dev, const double *Q, const double *lam, int nsteps, double dt, const double *f_dev, double *c_dev,
                           int snap_every, double *snap_dev, int obs_every, int nproj, const double *P_dev, double *obs_dev, int32_t *info);

#endif
