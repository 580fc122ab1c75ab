/* bspatom_spline_window.h -- the window operator on wave packets in the B-spline basis: how a packet is distributed over energy.
 * Part of bspatom.h, which includes it inside its extern "C" block after the types it needs: include bspatom.h, not this file. */
#ifndef BSPATOM_H
#error "include bspatom.h: bspatom_spline_window.h is a part of it"
#endif
#ifndef BSPATOM_SPLINE_WINDOW_H
#define BSPATOM_SPLINE_WINDOW_H

#define BSPATOM_WINDOW_MAX_FAC 8     /* stages (resolvent factors) of one window */

/* bspatom_spline_window (csrc/spline_window.hip): for nscan packets of nch channels and ne energies
 *     N(q, c, e) = x^H S x,     x_0 = c_{q,c},     x_{j+1} = (H_l[c] - z[e][j] S)^-1 S x_j,     x = x_nfac.
 * With the nfac = m shifts z_j = E + gamma exp(i pi (2j+1) / (2m)) -- the roots of (lambda - E)^(2m) + gamma^(2m) in the upper half
 * plane -- gamma^(2m) N is the window operator of order m,
 *     P_m(E) = <c| gamma^(2m) / ((H - E)^(2m) + gamma^(2m)) |c> = sum_n |x_n^T S c|^2 gamma^(2m) / ((E_n - E)^(2m) + gamma^(2m)),
 * the part of the packet within about gamma of E: the photoelectron spectrum of a propagated packet, on any energy grid, without an
 * eigenvector.  The library neither builds the shifts nor multiplies by gamma^(2m): ANY z is legal.  H must be Hermitian for the
 * window's meaning: the call takes no absorber.
 *   l    [nch]: the channels, among the bands the handle holds (the last bspatom_solve or bspatom_assemble)
 *   z    [ne][nfac][2]: Re, Im of the shift of stage j at energy e; not read with nfac = 0
 *   nfac 0 .. BSPATOM_WINDOW_MAX_FAC; nfac = 0 measures the plain S-norm c^H S c for every e
 *   c    [nscan][nch][nfun] complex: the packet layout of bspatom_tdse_split; not changed
 *   N    [nscan][nch][ne] real
 *   info [ne]: the pivots replaced (bspatom_resolvent's rule) at energy e, summed over the DISTINCT values of l and the stages: a
 *        factorisation counts once, however many packets it serves.  0 whenever Im z != 0.
 * The arithmetic, fixed:
 *   the matrix of a stage, its factorisation and the two substitutions are bspatom_resolvent's for (l, z) without an absorber (pivot by
 *         |Re| + |Im|, one scaled reciprocal per pivot, the four-product complex form with that call's fused products);
 *   the right-hand side of a stage, b = S x_j, by rule 1 of bspatom_tdse_spline.h on the symmetric band of S: b_re(i), b_im(i) start at
 *         +0.0 and add S(i, i + d) x(i + d) for d = -(k-1) .. k-1 ascending, columns outside 0 .. nfun-1 skipped, multiply then add;
 *   the norm is the N_ch of the spline rows: y = S x by the same rule, lane-strided partial sums -- lane t of 64 adds its rows
 *         i = t, t + 64, .. ascending from +0.0, s = s + (x_re(i)*y_re(i) + x_im(i)*y_im(i)), no FMA -- then the wave's fixed tree.
 * How: the matrices depend on (l, e, j) alone.  A work item is (energy, distinct value of l, block of at most "window_rhs"
 * right-hand sides among the packets (q, c) with that l; bspatom_set_option("window_rhs", r), default 8, 0 restores it): one wave
 * factors every stage once for its block, solves the block's right-hand sides one after the other and keeps their vectors in its
 * slot between the stages.  A persistent grid of single-wave workgroups takes the items by static stride ("resolvent_slots"
 * applies); no workgroup waits on another, no atomics, no LDS; one 8-byte store per (q, c, e).  Scratch per work slot, within
 * "resolvent_stage_mb" (one slot at least): bspatom_resolvent's slot and window_rhs vectors, 16*nfun*(3k-1) + 4*nfun +
 * 16*window_rhs*nfun bytes.  The host variant copies c in and N out once.
 * The limit: k <= 16 (the one-wave window's, BSPATOM_MAX_K); nscan*nch*ne and the items below 2^30.
 * Guarantees, bitwise:
 *   (W1) results are identical from run to run;
 *   (W2) N(q, c, e) depends on packet (q, c), l[c] and z[e][.] alone: not on nscan, nch, ne, the other scans, channels or energies,
 *        the work slots, window_rhs, resolvent_stage_mb, or host versus _dev;
 *   (W3) composition: with x_{j+1} the X of bspatom_resolvent for (l[c], z[e][j]) and the right-hand side B = S x_j formed by rule 1,
 *        N(q, c, e) is the norm rule above on x_nfac;
 *   (W4) a call with nfac' <= nfac and the first nfac' shifts of every energy returns what the nfac'-stage chain gives;
 *   (W5) nfac = 0 returns, for every e, the N_ch of the row of a bspatom_tdse_split call with nsteps = 0 on these packets;
 *   (W6) info does not depend on window_rhs or nscan.
 * BSPATOM_ERR_ARG: p, l, c, N or info NULL; z NULL with nfac > 0; nscan, nch or ne < 1; nfac outside 0 .. BSPATOM_WINDOW_MAX_FAC; a
 * channel outside the bands the handle holds; a count beyond the limit above.
 * The _dev variant: c and N in device memory of the problem's device; l, z and info stay host pointers. */
int bspatom_spline_window(bspatom_problem *p, int nscan, int nch, const int32_t *l, int ne, int nfac, const double *z, const double *c,
                          double *N, int32_t *info);
int bspatom_spline_window_dev(bspatom_problem *p, int nscan, int nch, const int32_t *l, int ne, int nfac, const double *z,
                              const double *c_dev, double *N_dev, int32_t *info);

#endif
