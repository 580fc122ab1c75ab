/* bspatom_spline_expect.h -- expectation values on wave packets in the B-spline basis, in a call of their own and along a split-step
 * run.  Part of bspatom.h, which includes it inside its extern "C" block after the types it needs: include bspatom.h, not this file. */
#ifndef BSPATOM_H
#error "include bspatom.h: bspatom_spline_expect.h is a part of it"
#endif
#ifndef BSPATOM_SPLINE_EXPECT_H
#define BSPATOM_SPLINE_EXPECT_H

/* bspatom_spline_expect (csrc/spline_expect.hip): for nscan packets and nexp operators B_o (x) G_o
 *     e(q, o) = sum_c conj(c_c)^T G_o u_{o,c},     u_{o,c} = sum_c' B_o(c, c') c_c'.
 * With B the matrix of cos theta between the channels and G the band of r this is the induced dipole <z>; with the band of dV/dr
 * the dipole acceleration, the one observable an absorbing box does not spoil.
 *   c    [nscan][nch][nfun] complex: the packet layout of bspatom_tdse_spline / bspatom_tdse_split
 *   GE   [nexp] full bands [2k-1][nfun], GE[(o*(2k-1) + d + k-1)*nfun + i] = G_o(i, i + d): real, symmetric or not
 *        (bspatom_dipole_bands, bspatom_operator_bands, the overlap's full band)
 *   B    [nexp][nch][nch] real angular matrices, row-major, any pattern
 *   e    [nscan][nexp][2]: Re, Im
 * The arithmetic, all plain IEEE fp64 without FMA:
 *   u(i)  starts at +0.0 and adds B_o(c, c') * c_c'(i) for c' ascending OVER THE ENTRIES WITH B_o(c, c') != 0 ONLY, multiply then add,
 *         Re and Im independently.  (The host compacts every row of B into an index/value list: the cost of a row is its non-zero
 *         entries', not nch.)
 *   y(i)  = sum_d G_o(i, i + d) u(i + d) by rule 1 of bspatom_tdse_spline.h on the full band: d = -(k-1) .. k-1 ascending from +0.0,
 *         columns outside 0 .. nfun-1 skipped, Re and Im independently.
 *   per channel  s_re = sum_i (c_re(i)*y_re(i) + c_im(i)*y_im(i)),  s_im = sum_i (c_re(i)*y_im(i) - c_im(i)*y_re(i)): lane-strided
 *         partial sums -- lane t of 64 adds its rows i = t, t + 64, .. ascending, from +0.0 -- then the wave's fixed tree.
 *   over the channels  ascending, from +0.0.
 * A row of B without a non-zero entry contributes (+0.0, +0.0) whatever the packets hold.  Hence: B_o = 0 gives exactly +0.0 in both
 * entries; a real packet gives Im e = +-0.0.
 * How: a persistent grid of single-wave workgroups takes the nscan*nexp*nch items by static stride ("resolvent_slots" applies), u
 * goes through the slot's scratch, y is consumed in registers; one partial per item, and a second small launch adds the partials of
 * the channels.  No workgroup waits on another, no atomics.
 * The limit: none of its own -- nothing is factored, the band is walked by a loop: any k a problem can have, any nfun, any nch;
 * nscan*nexp*nch and nexp*nch*nch below 2^30.
 * Guarantees, bitwise:
 *   (E1) results are identical from run to run;
 *   (E2) e(q, o) depends on packet q, B_o and G_o alone: not on nscan, the other scans, nexp, the other operators, the work slots, or
 *        host versus _dev.
 * BSPATOM_ERR_ARG: p, c or e NULL; nscan < 1 or nch < 1; nexp < 0; B or GE NULL with nexp > 0.  nexp = 0 is a valid call that
 * writes nothing.  The problem needs no bands: nfun and k are its grid's.
 * The _dev variant: GE, c, e in device memory of the problem's device; B stays a host pointer. */
int bspatom_spline_expect(bspatom_problem *p, int nscan, int nch, int nexp, const double *B, const double *GE, const double *c, double *e);
int bspatom_spline_expect_dev(bspatom_problem *p, int nscan, int nch, int nexp, const double *B, const double *GE_dev, const double *c_dev,
                              double *e_dev);

/* bspatom_tdse_split_observe: bspatom_tdse_split (bspatom_tdse_split.h) with the same numbers along the run.  The arguments are that
 * call's, followed by nexp, B, GE as above.  A row is nch + 2*nproj + 2*nexp wide: behind the entries of bspatom_tdse_split come Re, Im
 * of e(q, o), o ascending.  Row n measures the packets at t_n, before the first atomic half step of step n -- the packets N_c is
 * taken from --; the last row measures the returned packets; nsteps = 0 is a call that only measures.  The new entries have the bits
 * of bspatom_spline_expect on those packets (E1, E2), and they do not depend on tdse_split_group, tdse_stage_mb, obs_every, snap_every
 * or nproj.  Everything else the call returns -- c, the snapshots, info, the first nch + 2*nproj entries of every row -- has the bits of
 * bspatom_tdse_split with the same arguments: the measuring launches run in front of an observed step's first launch on the buffer
 * it reads, and write nothing a step reads.  With nexp = 0, or without rows (obs NULL), the call IS bspatom_tdse_split.
 * BSPATOM_ERR_ARG: what bspatom_tdse_split names; nexp < 0; B or GE NULL with nexp > 0.  The limit k <= 16 is that call's.
 * The _dev variant: what bspatom_tdse_split_dev takes in device memory, and GE; B stays a host pointer.  The host variant stages GE
 * once per call. */
int bspatom_tdse_split_observe(bspatom_problem *p, int nscan, int nch, const int32_t *l, int nabs, const double *WB, const int32_t *w,
                               const double *G, const double *Q, const double *lam, int nsteps, double dt, const double *f, double *c,
                               int snap_every, double *snap, int obs_every, int nproj, const double *P, double *obs, int32_t *info, int nexp,
                               const double *B, const double *GE);
int bspatom_tdse_split_observe_dev(bspatom_problem *p, int nscan, int nch, const int32_t *l, int nabs, const double *WB_dev, const int32_t *w,
                                   const double *G_dev, const double *Q, const double *lam, int nsteps, double dt, const double *f_dev,
                                   double *c_dev, int snap_every, double *snap_dev, int obs_every, int nproj, const double *P_dev,
                                   double *obs_dev, int32_t *info, int nexp, const double *B, const double *GE_dev);

#endif
