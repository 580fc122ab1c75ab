/*
 * bspatom.h -- C ABI of libbspatom: MI355X (gfx950) drop-in for the hot path of
 * carlosmwh1985/BspAtom: MATRIX_SVT + SOLVE_SYSTEM (reference src/matrices.f90:1-394), i.e. the
 * Gauss-Legendre assembly of the banded S, H(l) and the LAPACK DSYGV generalized eigen-solve.
 *
 * The reference has no plugin API: MATRIX_SVT / SOLVE_SYSTEM take no arguments and talk through
 * Fortran module globals (src/Modules.f90:21-203).  This header is therefore the explicit form
 * of that implicit interface; each entry point names the reference code it replaces.
 * All pointers are plain host pointers unless the name says `_dev`; the caller owns every
 * buffer it passes; the library owns the device memory of a problem between create/destroy.
 * All calls are blocking and must come from one host thread per problem.
 * Return value: 0 = ok, < 0 = BSPATOM_ERR_*, per-channel LAPACK-style codes go to `info[]`.
 */
#ifndef BSPATOM_H
#define BSPATOM_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define BSPATOM_OK 0
#define BSPATOM_ERR_HIP (-1)         /* HIP runtime error (text on stderr) */
#define BSPATOM_ERR_ARG (-2)         /* invalid argument */
#define BSPATOM_ERR_BSPLVB (-3)      /* 'FATAL ERROR - BSPLVB' STOP of bsplvb.f90:30-34 */
#define BSPATOM_ERR_NOGPU (-4)       /* no gfx950 device: there is no CPU fallback */
#define BSPATOM_ERR_UNSUPPORTED (-5)  /* a size outside this build's limits (below), or a switch combination that has no kernel */

/* Size limits of this build (bspatom_problem_create / bspatom_host_setup return BSPATOM_ERR_UNSUPPORTED beyond them, with the
 * limit on stderr).  The reference allocates everything by nfun / nkp (matrices.f90:20,222-225; bsplvb.f90:22) and has no
 * such limits, except that its Enl.dat record is I4 (matrices.f90:391): nfun <= 9999 is all it can write.
 *   BSPATOM_MAX_NFUN  functions per channel: 10048 (npad; every nfun the reference's output format allows);
 *   BSPATOM_MAX_K     B-spline order k (device tables of the assembly, band half-width of the Cholesky / inverse iteration);
 *   BSPATOM_MAX_KA    Gauss-Legendre points per interval (ka = k + 3 by default: 19 at k = 16). */
#define BSPATOM_MAX_NFUN 10048
#define BSPATOM_MAX_K 16
#define BSPATOM_MAX_KA 32

/* Namelist values of VARS_BSP / VARS_TISE (src/ReadInputs.f90:15-17) with the reference's
 * defaults (:27-36, :75-84) as the zero-initialised-then-`bspatom_input_defaults` state. */
typedef struct bspatom_input {
    int32_t kind_grid, k, ka, nfun, kind_bc1, kind_bc2;
    double ra, rb, rmax;
    int32_t n0_ini, l_ini, m_ini, l_fin, lmax, kind_pot;
    double emax_fin, zatom;
} bspatom_input;

/* Sizes derived exactly as READ_INPUTS does (src/ReadInputs.f90:39-69, :87). */
typedef struct bspatom_sizes {
    int32_t nfun, k, ka, nkp, nointv, nbc1, nbc2, lmax, nintv_exp, nintv_lin, npad;
} bspatom_sizes;

typedef struct bspatom_problem bspatom_problem;   /* opaque */

/* ---- set-up: READ_INPUTS sizes + GRID + gauleg + SELPOT tables (host), upload ------------- */
void bspatom_input_defaults(bspatom_input *in);                       /* ReadInputs.f90:27-36,75-84 */
int bspatom_device_count(void);
/* Host-only part of the set-up (no GPU needed): sizes as READ_INPUTS derives them; rt[nkp],
 * aind[2*nfun], xg[ka], wg[ka] as GRID/gauleg build them (call once with NULL arrays for the sizes). */
int bspatom_host_setup(const bspatom_input *in, bspatom_sizes *s, double *rt, double *aind, double *xg,
                       double *wg);
/* Creates the problem on HIP device `device`: derives sizes (ReadInputs.f90:39-141), builds the knot
 * sequence and Aind (grid.f90:14-91), the Gauss-Legendre rule (Modules.f90:112-153) and the
 * potential table (Modules.f90:263-295) on the host, uploads them.  One process per GPU: every problem of a
 * process must name the device of the first one (BSPATOM_ERR_UNSUPPORTED otherwise). */
int bspatom_problem_create(const bspatom_input *in, int device, bspatom_problem **out);
void bspatom_problem_destroy(bspatom_problem *p);
int bspatom_problem_sizes(const bspatom_problem *p, bspatom_sizes *s);
/* The route bspatom_solve takes for this problem under the current switches (BSP_ROUTE / option "route"): 2 = band route
 * (csrc/crawford.hip: the pencil stays banded; k - 1 <= 8), 1 = dense route (standard form, two-stage tridiagonalisation). */
int bspatom_problem_route(const bspatom_problem *p);
/* Host copies of rt[nkp], aind[2*nfun] (column-major Aind(nfun,2)), xg[ka], wg[ka]; any may be NULL. */
int bspatom_problem_grid(const bspatom_problem *p, double *rt, double *aind, double *xg, double *wg);

/* ---- the hot path --------------------------------------------------------------------------- */
/* MATRIX_SVT (matrices.f90:68-186) + `Hij = Tij + Uij(:,:,l) + Vij` (:244) for channels
 * l0 .. l0+nl-1, upper bands: SB[d*nfun + i] = S(i,i+d); HB[(l*k + d)*nfun + i] = H_l(i,i+d),
 * 0-based, d < k.  Bit-identical to the reference's dense matrices on the band.  SB/HB may be NULL
 * (results stay on the device for bspatom_solve). */
int bspatom_assemble(bspatom_problem *p, int l0, int nl, double *SB, double *HB);

/* SURVEY 8(f).2 -- the dipole matrices that MATRIX_SVT accumulates in the same quadrature loop and keeps in
 * rij for KIND_PI = 1, 2 (matrices.f90:141-144, 159-163): c = 0: int B_i r B_j dr (rij(:,:,1), length gauge),
 * c = 1: int B_i (1/r) B_j dr and c = 2: int B_i B_j' dr (rij(:,:,1), rij(:,:,2), velocity gauge).  The
 * reference fills both triangles and they are not bit-symmetric, so the FULL band is returned:
 * RB[(c*(2k-1) + (d+k-1))*nfun + i] = X_c(i, i+d), 0-based i, d = -(k-1)..k-1.  Bit-identical to the
 * reference's rij on the band (which is all of it).  RB: 3*(2k-1)*nfun doubles. */
int bspatom_dipole_bands(bspatom_problem *p, double *RB);

/* SOLVE_SYSTEM's l-loop (matrices.f90:242-265): assembly + DSYGV eigenvalues for channels
 * l0 .. l0+nl-1.  E[l*nfun + i] ascending per channel (column-major Enl(nfun,0:lmax), :230).
 * info[l]: 0 ok; nfun+i: leading minor i of S not positive definite (DSYGV convention, :250-254). */
int bspatom_solve(bspatom_problem *p, int l0, int nl, double *E, int32_t *info);
/* Same, spectra left in device memory (E_dev: nl*nfun doubles on the problem's device, e.g. a
 * torch tensor's data_ptr) so that ranks can exchange them with RCCL without a host round trip. */
int bspatom_solve_dev(bspatom_problem *p, int l0, int nl, double *E_dev, int32_t *info);

/* Eigenvector column `n0` (1-based, as n0_ini) of channel l -- the only column of DSYGV's 'V'
 * output that KIND_PI=0 consumes (matrices.f90:267): inverse iteration on the banded pencil
 * (H_l - E S), normalised c^T S c = 1; sign arbitrary (CHKPHS is commented out, :382).
 * Requires a previous bspatom_solve covering channel l.  c[nfun]. */
int bspatom_eigvec(bspatom_problem *p, int l, int n0, double *c);
/* The eigenvectors n0 .. n0+count-1 (1-based) of channel l, i.e. columns n0.. of DSYGV's 'V' output
 * Hij(:, n0:n0+count-1) at matrices.f90:248 -- what the KIND_PI >= 3 branch keeps as ctemp(:,1:ntemp,l)
 * (matrices.f90:331) and writes to Eigenvec_All.dat (:366-378, FORMAT 300 `I5,5000G20.10`): batched inverse
 * iteration on the banded pencil, each column normalised c^T S c = 1, sign arbitrary (as LAPACK's).
 * Z[j*nfun + i] = component i of eigenvector n0+j.  Requires a previous bspatom_solve covering l. */
int bspatom_eigvecs(bspatom_problem *p, int l, int n0, int count, double *Z);

/* Eigenvectors n0 .. n0+count-1 (1-based) of channels l0 .. l0+nl-1 of the last solved batch, in one call:
 * Z[((size_t)c * count + j) * nfun + i] = component i of eigenvector n0+j of channel l0+c.
 * Column for column BIT-IDENTICAL to bspatom_eigvecs(p, l0+c, n0, count, ...): the same inverse iteration on a persistent grid
 * of one wave per resident work slot (device scratch bounded by the slots, not by nl*count).  The host variant stages the
 * output through a device buffer of at most 256 MiB (one channel's block at least).  BSPATOM_ERR_ARG unless every channel
 * lies in the last solve, nl >= 1, count >= 1, n0 >= 1 and n0+count-1 <= nfun (and after bspatom_assemble);
 * BSPATOM_ERR_UNSUPPORTED if an iterate vanished. */
int bspatom_eigvecs_batch(bspatom_problem *p, int l0, int nl, int n0, int count, double *Z);
/* Same, Z_dev in device memory of the problem's device (e.g. a torch tensor's data_ptr), nl*count*nfun doubles, written in place. */
int bspatom_eigvecs_batch_dev(bspatom_problem *p, int l0, int nl, int n0, int count, double *Z_dev);

/* Dipole matrix elements between eigenvectors of the last solved batch: the DGEMV + DDOT of TRANS_AMP for the
 * plane-wave branches KIND_PI = 1, 2 (reference PhotoIon.f90:95-107):
 *   D[i] = c(l_fin, n0_fin + i)^T (a[0] R_r + a[1] R_{1/r} + a[2] R_{d/dr}) c(l_ini, n0_ini),  i = 0 .. count-1,
 * with R_r = int B_i r B_j, R_{1/r} = int B_i B_j / r, R_{d/dr} = int B_i B_j' (the rij of MATRIX_SVT,
 * matrices.f90:141-144,159-163) and S-normalised eigenvectors whose signs are this library's (first significant
 * coefficient positive).  The reference's T_fi(n) = An c0 D: the angular factors c0, a[] (THREE_J) and the density of
 * states An are host arithmetic (bspatom_amd/host.py::trans_amp).  n0_* are 1-based. */
int bspatom_dipole_elements(bspatom_problem *p, int l_ini, int n0_ini, int l_fin, int n0_fin, int count,
                            const double a[3], double *D);

/* The same elements for whole windows of initial AND final states of many channel pairs in one call -- the reference's unit
 * of work, "all states of two channels" (matrices.f90:331 keeps ctemp(:,1:ntemp,l); PhotoIon.f90:95-107 runs over it):
 *   D[((size_t)p*count_ini + i)*count_fin + f] =
 *     c(l_fin[p], n0_fin+f)^T (a[3p] R_r + a[3p+1] R_{1/r} + a[3p+2] R_{d/dr}) c(l_ini[p], n0_ini+i)
 * for p < npairs, i < count_ini, f < count_fin; 1-based state numbers, channels of the last solve.  Matrices, eigenvectors
 * (bspatom_eigvecs' bit for bit), signs and normalisation are those of bspatom_dipole_elements: row i of pair p is what
 * bspatom_dipole_elements(p, l_ini[p], n0_ini+i, l_fin[p], n0_fin, count_fin, a+3p, .) returns up to the summation order of
 * the final dot product, which here runs on the matrix cores over K slices fixed by (nfun, count_ini, count_fin) alone and
 * summed in slice order.  Pairs may repeat channels in either role and l_ini[p] == l_fin[p] is allowed.  The pairs are
 * processed in groups, in the order given; a group's device scratch (its distinct eigenvector blocks, A x of its distinct
 * initial blocks, the K-slice partials, and D for the host variant) stays within 2 GiB -- bspatom_eigvecs_batch stages through
 * 256 MiB -- or one pair's need if that is more; bspatom_set_option("dipole_stage_mb", m) sets another bound.  Results are
 * run-to-run bit-identical, and a pair's block depends neither on the other pairs of the call nor on the grouping.
 * BSPATOM_ERR_ARG: a null pointer, npairs < 1, a count < 1, a window outside 1..nfun, a channel outside the last solve (every
 * channel after bspatom_assemble); BSPATOM_ERR_UNSUPPORTED if an inverse iteration broke down. */
int bspatom_dipole_matrix(bspatom_problem *p, int npairs, const int32_t *l_ini, const int32_t *l_fin, int n0_ini, int count_ini,
                          int n0_fin, int count_fin, const double *a, double *D);
/* Same, D_dev in device memory of the problem's device (npairs*count_ini*count_fin doubles), written in place. */
int bspatom_dipole_matrix_dev(bspatom_problem *p, int npairs, const int32_t *l_ini, const int32_t *l_fin, int n0_ini,
                              int count_ini, int n0_fin, int count_fin, const double *a, double *D_dev);

/* Matrix elements of caller-given radial operators g(r) and g(r) d/dr (csrc/opmat.hip) -- the general case of the rij above: for
 * KIND_PI >= 3 MATRIX_SVT assembles zAij (matrices.f90:114-139, 165-171), for every tabulated profile zIth(ibet, igl, il, jl, comp) the
 * sums fbra * g(r_q) * fket * dr and fbra * g(r_q) * dfket * dr; FRMATINT's u_i u_j'/r^2 and u_i u_j/r^3 (TorusFunsInts.f90:286-382),
 * multipoles r^lambda, a perturbing potential are the same thing.  g is known by its values on the Gauss-Legendre points alone:
 * nr = what bspatom_quadrature returns, g holds nop*nr doubles, operator o at g + o*nr, indexed like the quadrature points;
 * deriv[o] = 0: G_o(i,j) = sum_q B_i(r_q) g_o(q) B_j(r_q) w_q, deriv[o] = 1: B_j' in place of B_j.
 *   GB[(o*(2k-1) + (d+k-1))*nfun + i] = G_o(i, i+d), 0-based i, d = -(k-1)..k-1 (the layout of bspatom_dipole_bands; zero where i+d
 *   is outside 0..nfun-1): the FULL band, both triangles computed independently, as the reference does.  GB: nop*(2k-1)*nfun doubles.
 * The arithmetic is fixed: one accumulator from 0.0, terms added over intervals ascending and points ascending across the intervals
 * common to both functions (matrices.f90:71-72), each term ((fbra * g) * fket) * dr or ((fbra * g) * dfket) * dr, IEEE multiplies
 * and adds, no FMA; fbra, fket, dfket, dr are the assembly's point table; intervals of zero width carry no g value and are skipped.
 * So: with g = (r, 1/r, 1), deriv = (0, 0, 1) and the r of bspatom_quadrature the three bands equal bspatom_dipole_bands bit for bit
 * (hence the reference's rij); a complex profile is two operators, Re g and Im g, whose bands are the real and imaginary parts of
 * the reference's complex sum bit for bit (real times complex is componentwise); an operator's band does not depend on the other
 * operators of the call.  g is not checked for finiteness: a NaN in goes to NaN out.
 * BSPATOM_ERR_ARG: a null pointer, nop < 1, a deriv value outside {0, 1}.  The _dev variant: g_dev, GB_dev in device memory of the
 * problem's device; deriv stays a host pointer. */
int bspatom_operator_bands(bspatom_problem *p, int nop, const double *g, const int32_t *deriv, double *GB);
int bspatom_operator_bands_dev(bspatom_problem *p, int nop, const double *g_dev, const int32_t *deriv, double *GB_dev);

/* bspatom_dipole_matrix for those operators:
 *   D[((size_t)p*count_ini + i)*count_fin + f] = c(l_fin[p], n0_fin+f)^T A_p c(l_ini[p], n0_ini+i),   A_p = sum_o a[p*nop + o] G_o.
 * An entry of A_p is formed as s = a_0*G_0, then s = s + a_o*G_o for o ascending; a row of A_p x over diagonals ascending; both
 * without FMA; the final product D = W Z^T is bspatom_dipole_matrix's (matrix cores, K slices by (nfun, count_ini, count_fin) alone,
 * summed in slice order).  Eigenvectors, signs and normalisation, channels of the last solve, 1-based windows, repeated channels in
 * either role and l_ini[p] == l_fin[p], the grouping under the dipole_stage_mb bound (the operator bands, nop*(2k-1)*nfun doubles,
 * and the uploaded g are counted outside it), run-to-run bit-identical results and a pair's block independent of the other pairs and
 * of the grouping: all as bspatom_dipole_matrix states them.  The host variant uploads g and deriv once per call.
 * BSPATOM_ERR_ARG: a null pointer, nop < 1, a deriv value outside {0, 1}, and what bspatom_dipole_matrix names;
 * BSPATOM_ERR_UNSUPPORTED if an inverse iteration broke down.  The _dev variant: g_dev and D_dev in device memory of the problem's
 * device; deriv, l_ini, l_fin and a stay host pointers. */
int bspatom_operator_matrix(bspatom_problem *p, int nop, const double *g, const int32_t *deriv, int npairs, const int32_t *l_ini,
                            const int32_t *l_fin, int n0_ini, int count_ini, int n0_fin, int count_fin, const double *a, double *D);
int bspatom_operator_matrix_dev(bspatom_problem *p, int nop, const double *g_dev, const int32_t *deriv, int npairs,
                                const int32_t *l_ini, const int32_t *l_fin, int n0_ini, int count_ini, int n0_fin, int count_fin,
                                const double *a, double *D_dev);

/* ---- resolvent solves on the banded pencil (csrc/resolvent.hip) ------------------------------------------------------------ */
/* The response at ANY complex energy, where the layers above answer at the box eigenvalues only: for m < nmat the banded system
 *   M_m x = b,   M_m = H_{l[m]} - i W_{w[m]} - z_m S,   z_m = z[2m] + i z[2m+1],
 * is solved for each of nrhs right-hand sides shared by all matrices, and projected on nproj left vectors:
 *   X[((size_t)m*nrhs + r)*nfun + i] = x_{m,r}(i),      R[((size_t)m*nrhs + r)*nproj + q] = sum_i P_q(i) x_{m,r}(i)
 * (bilinear: NO complex conjugate).  Complex means interleaved (Re, Im) doubles: z has 2*nmat doubles, B nrhs*nfun complex, P
 * nproj*nfun complex, X nmat*nrhs*nfun complex, R nmat*nrhs*nproj complex.  H_l and S are the bands the problem holds on the device,
 * so l[m] must be a channel of the last bspatom_solve or bspatom_assemble, whichever came last.  W: nabs caller-given FULL bands in
 * bspatom_operator_bands' layout, WB[(a*(2k-1) + (d+k-1))*nfun + i] = W_a(i, i+d), both triangles used as given (e.g. the band of
 * host.cap_profile: a complex absorbing potential); w[m] = -1: no absorber for matrix m; w == NULL: absorber 0 for every matrix
 * if WB is given, none otherwise.  With an absorber z may lie anywhere in the continuum and p^T x is a smooth function of z: the sum
 * over every state of a channel (dynamic polarizabilities, two-photon amplitudes, Green's functions) in O(nfun k^2) per energy.
 * One wavefront factors one matrix: banded LU with partial pivoting by |Re| + |Im| (ties to the smallest row), complex products in
 * the plain four-product form, one reciprocal per pivot; info[m] = number of pivots below eps * max_j |M_jj| that were replaced by
 * that bound on the real axis: 0 unless a real z sits on an eigenvalue with no absorber (the x is then huge, not wrong).
 * At least one of X and R must be non-NULL; P may be NULL when R is.  Guarantees:
 *   (G1) results are bit-identical from run to run;
 *   (G2) x_{m,r} and R[m][r][q] depend on (l[m], z_m, W_{w[m]}, B_r, P_q) alone -- not on the other matrices, on nmat, nrhs or nproj, on
 *        the number of work slots, on the grouping below, or on the host versus _dev variant;
 *   (G3) with Im z = 0, no absorber and real B every imaginary part of X is +-0.0 exactly.
 * The host variant processes the matrices in groups, in the order given, the X of one group staged through a device buffer of at
 * most 2 GiB (one matrix at least); the kernel's scratch, nfun*(6k-1) doubles per resident wave, stays within the same bound (one
 * wave at least); bspatom_set_option("resolvent_stage_mb", m) sets another bound, ("resolvent_slots", s) another number of waves.
 * The scratch of a call is freed when it returns.  BSPATOM_ERR_ARG: a null p, l, z, B or info, X and R both NULL, R given with P NULL
 * or nproj < 1, nmat < 1, nrhs < 1, nabs < 0, nabs > 0 with WB NULL, a channel outside the bands held, w[m] outside -1 .. nabs-1.
 * The _dev variant: WB, B, P, X, R in device memory of the problem's device, written in place; l, z, w, info stay host pointers. */
int bspatom_resolvent(bspatom_problem *p, int nmat, const int32_t *l, const double *z, int nabs, const double *WB, const int32_t *w,
                      int nrhs, const double *B, int nproj, const double *P, double *X, double *R, int32_t *info);
int bspatom_resolvent_dev(bspatom_problem *p, int nmat, const int32_t *l, const double *z, int nabs, const double *WB_dev,
                          const int32_t *w, int nrhs, const double *B_dev, int nproj, const double *P_dev, double *X_dev, double *R_dev,
                          int32_t *info);

/* Chains of resolvents with an operator in between (csrc/resolvent.hip: resolvent_chain_kernel) -- what lies beyond second order:
 * two-photon amplitudes above threshold, three-photon amplitudes, hyperpolarizabilities, the Cauchy moments of alpha(omega) are
 *   p^T G_{l2}(z2) A2 G_{l1}(z1) A1 c_i,      G_l(z) = (H_l - i W - z S)^-1,
 * where the right-hand side of a solve is the solution of the one before and differs for every energy.  For chain c < nchain, stage
 * s < nstage, right-hand side r < nrhs, with m = c*nstage + s:
 *   M_{c,s}   = H_{l[m]} - i W_{w[m]} - z_{c,s} S,   z_{c,s} = z[2m] + i z[2m+1]   (w == NULL, w[m] = -1 as in bspatom_resolvent)
 *   x_{c,0,r} = M_{c,0}^-1 B_r
 *   x_{c,s,r} = M_{c,s}^-1 (A_{c,s} x_{c,s-1,r}),   s >= 1,   A_{c,s} = sum_o a[(c*(nstage-1) + (s-1))*nop + o] G_o
 *   R[(((size_t)c*nstage + s)*nrhs + r)*nproj + q] = sum_i P_q(i) x_{c,s,r}(i)      (bilinear, EVERY stage)
 *   X[((size_t)c*nrhs + r)*nfun + i] = x_{c,nstage-1,r}(i)                          (the LAST stage only)
 *   info[m] = pivots replaced in M_{c,s}
 * GB: nop FULL bands in bspatom_operator_bands' layout, both triangles used as given (bspatom_dipole_bands, any
 * bspatom_operator_bands result, S itself from g = 1).  a is REAL, as in bspatom_operator_matrix: the bands are real and a real
 * combination keeps A x two independent real products (G3 below survives a chain); a phase factor on an operator is a factor on the
 * whole amplitude and the caller's business.  nstage = 1 needs neither GB nor a: nop = 0 is then allowed and both may be NULL.
 * The arithmetic of y = A x is fixed: an entry is formed as t = a_0*G_0(i,i+d), then t = t + a_o*G_o(i,i+d) for o ascending; y_re(i)
 * starts at +0.0 and adds t * x_re(i+d) for d = -(k-1) .. k-1 ascending, terms with i+d outside 0..nfun-1 skipped; y_im likewise from
 * x_im; IEEE multiplies and adds, no FMA (bspatom_operator_matrix's rule for A x, applied to the two components).  One wavefront
 * keeps a chain from its first factorisation to its last projection; a stage's factorisation serves all nrhs right-hand sides.
 * Guarantees:
 *   (C1) results are bit-identical from run to run;
 *   (C2) a chain's results depend on its own (l, z, W, a), on GB, B_r and P_q alone -- not on the other chains, on nchain, nrhs or
 *        nproj, on the work slots or the grouping, or on the host versus _dev variant;
 *   (C3) prefix: R and info of stages 0..s equal those of the same chain cut to s+1 stages, and the cut chain's X is x_{c,s}: an
 *        intermediate vector is obtained this way;
 *   (C4) nstage = 1 is bspatom_resolvent bit for bit, in X, R and info;
 *   (C5) composition: stage s equals bspatom_resolvent with nmat = 1 given A x_{s-1}, formed by the arithmetic above, as its
 *        right-hand side, bit for bit;
 *   (C6) with every Im z = 0, no absorber and real B every imaginary part of X is +-0.0 exactly.
 * The host variant processes the chains in groups under the bound of bspatom_resolvent ("resolvent_stage_mb"; the X of one group, one
 * chain at least); the kernel's scratch per resident wave is bspatom_resolvent's plus nrhs complex vectors, nfun*(6k-1 + 2 nrhs)
 * doubles, within the same bound; "resolvent_slots" applies as there.  BSPATOM_ERR_ARG: what bspatom_resolvent names, for every
 * stage; nchain < 1, nstage < 1; nop < 0; nstage > 1 with nop < 1 or GB or a NULL.  The _dev variant: WB, GB, B, P, X, R in device
 * memory of the problem's device, written in place; l, z, w, a, info stay host pointers. */
int bspatom_resolvent_chain(bspatom_problem *p, int nchain, int nstage, const int32_t *l, const double *z, int nabs, const double *WB,
                            const int32_t *w, int nop, const double *GB, const double *a, int nrhs, const double *B, int nproj,
                            const double *P, double *X, double *R, int32_t *info);
int bspatom_resolvent_chain_dev(bspatom_problem *p, int nchain, int nstage, const int32_t *l, const double *z, int nabs,
                                const double *WB_dev, const int32_t *w, int nop, const double *GB_dev, const double *a, int nrhs,
                                const double *B_dev, int nproj, const double *P_dev, double *X_dev, double *R_dev, int32_t *info);

/* Channels coupled to ALL orders in one banded LU (csrc/resolvent_coupled.hip).  bspatom_resolvent answers for one channel, a chain
 * multiplies such answers with one operator in between -- perturbation theory.  A static field (Stark shifts and widths), a
 * monochromatic field in the Floquet picture (dressed states, multiphoton rates without a time propagation), any potential that mixes
 * l is ONE linear system:  (sum_c (H_{l_c} - i W_c - z_c S) + V) x = b.  Matrix m < nmat acts on nch blocks of nfun coefficients:
 *   diagonal block c:  H_{l[m*nch+c]} - i W_{w[m*nch+c]} - z_{m,c} S,   z_{m,c} = z[2(m*nch+c)] + i z[2(m*nch+c)+1]
 *     -- every channel of every matrix has its own energy (a Floquet block carries z - n omega); l may repeat within a matrix; w as in
 *     bspatom_resolvent per (m, c): w[..] = -1: no absorber for that block; w == NULL: absorber 0 for every block if WB is given,
 *     none otherwise; WB: nabs FULL bands;
 *   coupling entry p < ncoup:  block (row channel cr[p], column channel cc[p]) gains sum_o alpha_{m,p,o} G_o, or G_o^T where
 *     ctr[p] = 1;  alpha_{m,p,o} = a[((m*ncoup+p)*nop+o)*2] + i a[((m*ncoup+p)*nop+o)*2 + 1] is COMPLEX;  GB: nop FULL bands in
 *     bspatom_operator_bands' layout, both triangles as given.  The topology (cr, cc, ctr) is shared by all matrices of the call, the
 *     coefficients are per matrix.  NO partner is added: a Hermitian coupling is two entries, the second with ctr = 1 and the
 *     conjugate coefficient (bspatom_tdse_static's convention).  cr[p] == cc[p] is allowed (an in-channel perturbation); entries on
 *     the same block add in ascending p, after the diagonal-block formula, each as re += Re alpha * G, im += Im alpha * G for o
 *     ascending.  ncoup = 0 needs neither cr, cc, ctr, GB nor a.
 * Right-hand sides, shared by all matrices, and projections are channel-major, nch*nfun complex each:
 *   B[(r*nch+c)*nfun+i],   P[(q*nch+c)*nfun+i];   X[((((size_t)m*nrhs+r)*nch+c)*nfun+i] = x_{m,r}(i, c);
 *   R[((size_t)m*nrhs+r)*nproj+q] = sum_c sum_i P_q(i, c) x_{m,r}(i, c)   (bilinear, no conjugate, over ALL channels);
 *   info[m] = number of pivots replaced, with bspatom_resolvent's meaning and threshold (eps * max |M_jj| over the whole diagonal).
 * At least one of X and R must be given; P may be NULL when R is.
 * Ordering: the matrix that is factored has unknown (i, c) at position i*nch + c; it is banded with half-width bw = nch*k - 1 (this
 *   build does not narrow bw from the topology).  The matrix is the one in that ordering: a dense solve of the same system meets the
 *   same band and, with the same pivot rule, the same growth.
 * Factorisation: one workgroup per matrix, LU with partial pivoting by |Re| + |Im|, ties to the smallest row; complex products in the
 *   plain four-product form; one reciprocal per pivot (bspatom_resolvent's).  The row window, (bw+1) x (2bw+1) complex, lives in LDS.
 * Limit: bw <= BSPATOM_COUPLED_MAX_BAND = 63: the pivot candidates of a column, at most bw + 1, then fit one wavefront, and the window,
 *   at most 64 x 127 complex = 130 KB, fits the 160 KiB of LDS.  That covers k = 9 with seven channels and k = 16 with four.  Beyond it:
 *   BSPATOM_ERR_UNSUPPORTED, the limit printed on stderr.
 * Guarantees:
 *   (K1) results are bit-identical from run to run;
 *   (K2) the results of matrix m depend on its own l, z, w, a, on the shared topology and on WB, GB, B_r, P_q alone -- not on the other
 *        matrices, on nmat, nrhs or nproj, on the work slots, on the grouping below, or on the host versus _dev variant;
 *   (K3) with every Im z = 0, no absorber, real coefficients and real B every imaginary part of X is +-0.0 exactly;
 *   (K4) an entry given with ctr = 1 equals, bit for bit, the same entry with ctr = 0 and the transposed band.
 * NOT promised: nch = 1 is not bspatom_resolvent bit for bit -- another kernel, another order of summation; it satisfies the same
 * system to the same backward error.
 * The host variant processes the matrices in groups under bspatom_resolvent's bound ("resolvent_stage_mb": the X of one group, one
 * matrix at least); "resolvent_slots" applies.  Scratch per work slot (resident workgroup), within the same bound: U, L and one
 * vector, N*(3bw+2) complex with N = nch*nfun, plus N pivot indices -- nch*nfun*(6*nch*k - 2) doubles and nch*nfun 32-bit integers.
 * BSPATOM_ERR_ARG: what bspatom_resolvent names, per (m, c); nch < 1; ncoup < 0; a channel index outside 0..nch-1; ctr outside {0, 1};
 * ncoup > 0 with nop < 1 or with any of cr, cc, ctr, GB, a NULL.  The _dev variant: WB, GB, B, P, X, R in device memory of the problem's
 * device, written in place; l, z, w, cr, cc, ctr, a, info stay host pointers. */
#define BSPATOM_COUPLED_MAX_BAND 63
int bspatom_resolvent_coupled(bspatom_problem *p, int nmat, int nch, const int32_t *l, const double *z, int nabs, const double *WB,
                              const int32_t *w, int ncoup, const int32_t *cr, const int32_t *cc, const int32_t *ctr, int nop,
                              const double *GB, const double *a, int nrhs, const double *B, int nproj, const double *P, double *X,
                              double *R, int32_t *info);
int bspatom_resolvent_coupled_dev(bspatom_problem *p, int nmat, int nch, const int32_t *l, const double *z, int nabs,
                                  const double *WB_dev, const int32_t *w, int ncoup, const int32_t *cr, const int32_t *cc,
                                  const int32_t *ctr, int nop, const double *GB_dev, const double *a, int nrhs, const double *B_dev,
                                  int nproj, const double *P_dev, double *X_dev, double *R_dev, int32_t *info);

/* The coupled system beyond half-width 63: a BLOCKED banded LU (csrc/resolvent_wide.hip).  Four l with two photons either side are
 * ten Floquet blocks, bw = 89 at k = 9; a strong static field needs l well beyond 6: bspatom_resolvent_coupled answers those with
 * BSPATOM_ERR_UNSUPPORTED.  bspatom_resolvent_coupled_wide takes the SAME arguments with the SAME meaning -- B, P, X, R channel-major
 * in the same layouts; w == NULL and w = -1; cr, cc, ctr and the complex a; info[m] = number of pivots replaced, the same threshold;
 * the ordering i*nch + c with bw = nch*k - 1, not narrowed from the topology; the same BSPATOM_ERR_ARG list -- for any bw from 1 to
 * BSPATOM_COUPLED_WIDE_MAX_BAND = 255 (bw <= 63 included): k = 9 with 28 blocks, k = 16 with 16.  Beyond it: BSPATOM_ERR_UNSUPPORTED,
 * the limit printed on stderr.  bspatom_resolvent_coupled itself is unchanged: its limit, its kernel, its bits.
 * Factorisation: one workgroup per matrix, no workgroup waits on another.  The band lies in the slot's scratch in LAPACK ZGBTRF's
 *   column layout (column c holds the rows c - 2bw .. c + bw); the workgroup factors it in panels of 16 columns.  A panel, at most
 *   bw + 16 rows, is factored in LDS column by column with bspatom_resolvent_coupled's pivot rule exactly: the largest |Re| + |Im|
 *   over ALL candidates of the column (up to 256: four wavefronts, combined in ascending order), ties to the smallest row; a pivot
 *   below the threshold is replaced and counted; one reciprocal per pivot.  Then the panel's interchanges go to the columns on its
 *   right, U12 = L11^-1 A12 on plain FMAs, and A22 -= L21 U12 on v_mfma_f64_16x16x4_f64, the complex product as four real ones, the
 *   contraction over the panel's 16 columns in ascending order.  The right-hand sides are eliminated with each panel (L is not
 *   kept); the backward pass runs over the same blocks of 16 columns.  Tiles, chunks and blocks depend on (nch*nfun, bw) alone.
 * Guarantees:
 *   (K1) results are bit-identical from run to run;
 *   (K2) the results of matrix m depend on its own l, z, w, a, on the shared topology and on WB, GB, B_r, P_q alone -- not on the other
 *        matrices, on nmat, nrhs or nproj, on the work slots, on the grouping below, or on the host versus _dev variant;
 *   (K3) with every Im z = 0, no absorber, real coefficients and real B every imaginary part of X is +-0.0 exactly (on the matrix
 *        cores too: every imaginary accumulator only ever sums products with a zero factor);
 *   (K4) an entry given with ctr = 1 equals, bit for bit, the same entry with ctr = 0 and the transposed band.
 * NOT promised: equality with bspatom_resolvent_coupled at bw <= 63 -- another kernel, another order of summation; both satisfy the
 * same system to the same backward error.
 * The host variant processes the matrices in groups under bspatom_resolvent's bound ("resolvent_stage_mb": the X of one group, one
 * matrix at least); "resolvent_slots" applies.  Scratch per work slot, within the same bound (one slot at least): the band with the
 * room of the fill and the nrhs vectors, N*(3bw + 1 + nrhs) complex with N = nch*nfun -- 2*nch*nfun*(3*nch*k - 2 + nrhs) doubles.
 * The _dev variant as bspatom_resolvent_coupled_dev. */
#define BSPATOM_COUPLED_WIDE_MAX_BAND 255
int bspatom_resolvent_coupled_wide(bspatom_problem *p, int nmat, int nch, const int32_t *l, const double *z, int nabs, const double *WB,
                                   const int32_t *w, int ncoup, const int32_t *cr, const int32_t *cc, const int32_t *ctr, int nop,
                                   const double *GB, const double *a, int nrhs, const double *B, int nproj, const double *P, double *X,
                                   double *R, int32_t *info);
int bspatom_resolvent_coupled_wide_dev(bspatom_problem *p, int nmat, int nch, const int32_t *l, const double *z, int nabs,
                                       const double *WB_dev, const int32_t *w, int ncoup, const int32_t *cr, const int32_t *cc,
                                       const int32_t *ctr, int nop, const double *GB_dev, const double *a, int nrhs,
                                       const double *B_dev, int nproj, const double *P_dev, double *X_dev, double *R_dev, int32_t *info);

/* WRITE_WF (Bsp_Atom.f90:118-146): u(r_i) = sum_j c_j B_j(r_i), r_i = ra + i*(rb-ra)/npts,
 * i = 0..npts.  Returns BSPATOM_ERR_BSPLVB where the reference STOPs. r[npts+1], u[npts+1]. */
int bspatom_write_wf(bspatom_problem *p, const double *c, int npts, double *r, double *u);

/* ---- wavefunctions and their derivatives as functions of r (csrc/wavefn.hip) --------------------------------------------- */
/* The points and weights of the assembly's Gauss-Legendre quadrature (matrices.f90:91-97: r = f1 + xg*f2, dr = f2*wg with
 * f1 = (rt(i+1) + rt(i))/2, f2 = (rt(i+1) - rt(i))/2) for the knot intervals of positive width (rt(i+1) > rt(i)), ascending, ka per
 * interval: the grid rtot of TORMAT / WFALL (TorusFuns.f90:87-104, nr = nointv*ka).  *nr = their number; r, w may be NULL (size
 * query).  ON PURPOSE these are the assembly's f1 + xg*f2, not a second gauleg(rt(i), rt(i+1)) as TORMAT calls it (:99): on the
 * assembly's own points sum_p w_p u_i(r_p) u_j(r_p) is c_i^T S c_j term for term, and likewise for the rij of MATRIX_SVT, so every
 * radial integral <f| g(r) |i>, <f| g(r) d/dr |i> formed from the tables below is the quadrature the matrices were built with.
 * Host arithmetic, no GPU work. */
int bspatom_quadrature(bspatom_problem *p, int *nr, double *r, double *w);

/* WFALL (TorusFuns.f90:193-261) for any block of coefficient vectors:
 *   U[v*npts + ip] = sum_j Z[v*nfun + j] B_j(r_ip),   dU[v*npts + ip] = sum_j Z[v*nfun + j] B_j'(r_ip)   (dU may be NULL: values only)
 * for v < nvec, ip < npts.  r is a HOST pointer in every variant; r == NULL selects the quadrature grid above (npts must then equal
 * nr; the assembly's point table is run first if it has not been and its B_j, B_j' are used).  The caller's points may be unsorted and
 * may repeat; each must be finite and lie in [rt(1), rt(nkp)] (BSPATOM_ERR_ARG otherwise, checked on the host before any launch).
 * The interval of a point is interv's (interv.f90:86-117), including the walk down at r == rt(nkp); BSPATOM_ERR_BSPLVB where the
 * reference STOPs (bsplvb.f90:30-34).  B_j, B_j' are BSPALL's (Modules.f90:71-110): two bsplvb recurrences, dbsp = (k-1) (Aind1
 * bspp(j) - Aind2 bspp(j+1)), zero coefficients outside 1..nfun; the sums run over the k local functions ascending from 0.0, one IEEE
 * multiply and one IEEE add per term, IEEE division, no FMA -- WFALL's order.  So a value is reproducible bit for bit from a CPU
 * restatement, run-to-run identical, and independent of grouping, tiling and the other vectors of the call.
 * The host variant stages U and dU together through a device buffer of at most 256 MiB (bspatom_set_option("wf_stage_mb", m) sets
 * another bound; one vector's rows at least); the _dev variant (Z_dev, U_dev, dU_dev in device memory of the problem's device) writes
 * in place, its scratch is the basis table: npts*2k doubles and npts ints.  BSPATOM_ERR_ARG: a null p, Z or U, nvec < 1, npts < 1,
 * r == NULL with npts != nr, a bad point. */
int bspatom_tabulate(bspatom_problem *p, int nvec, const double *Z, int npts, const double *r, double *U, double *dU);
int bspatom_tabulate_dev(bspatom_problem *p, int nvec, const double *Z_dev, int npts, const double *r, double *U_dev, double *dU_dev);

/* The same for the eigenvectors n0 .. n0+count-1 (1-based) of channels l0 .. l0+nl-1 of the last solve -- fur(ir, n, l), dfur(ir, n, l)
 * of WFALL (TorusFuns.f90:218, 245-246), the factors of FRMATINT's u_i u_j'/r^2 and u_i u_j/r^3 (TorusFunsInts.f90:286-382):
 *   U[((size_t)c*count + j)*npts + ip] = u(r_ip) of eigenvector n0+j of channel l0+c, dU likewise (may be NULL).
 * The eigenvectors are bspatom_eigvecs' bit for bit (signs, S-normalisation), computed in groups of channels whose block stays within
 * the bound above (one channel at least): the result equals bspatom_tabulate* applied to bspatom_eigvecs_batch's output, bit for bit.
 * Points as above.  BSPATOM_ERR_ARG as bspatom_eigvecs_batch (every channel after bspatom_assemble) and for the points;
 * BSPATOM_ERR_UNSUPPORTED if an inverse iteration broke down. */
int bspatom_wavefunctions(bspatom_problem *p, int l0, int nl, int n0, int count, int npts, const double *r, double *U, double *dU);
int bspatom_wavefunctions_dev(bspatom_problem *p, int l0, int nl, int n0, int count, int npts, const double *r, double *U_dev,
                              double *dU_dev);

/* ---- the TDSE in the basis of the field-free eigenstates (csrc/tdse.hip) ---------------------------------------------------- */
/* What the blocks above are for: the sibling TDSE programs integrate i da/dt = (E + f(t) D) a in the eigenstate basis.  The reference
 * ships the state arrays zf, zdfdt, zVtij (Modules.f90:238-246), the envelopes CHAMP (:330-396), the tableau MOD_RK_PARAMS (:559-586)
 * and the reader of the result READ_TDCOEFF (ReadInputs.f90:453-467), not the integrator.  This is it, for nscan wave packets at once.
 *   nch channels of count states: E[c*count + n]; npairs coupling blocks between channels ci[p] != cf[p] (0-based positions in E),
 *   D[(p*count + i)*count + f], i a state of channel ci[p], f of cf[p] -- bspatom_dipole_matrix's layout with count_ini = count_fin;
 *   nscan independent wave packets, scan q driven by its own complex scalar f_q(t).  For every q
 *     i d a_c/dt = E_c .* a_c + sum_{p: cf[p]=c} f_q(t) (D_p^T a_ci[p]) + sum_{p: ci[p]=c} conj(f_q(t)) (D_p a_cf[p]),
 *     (D_p^T a)[f] = sum_i D_p[i][f] a[i], (D_p a)[i] = sum_f D_p[i][f] a[f]:
 *   every block enters with its Hermitian conjugate, the Hamiltonian is Hermitian for any complex f (length gauge: f = F(t) real;
 *   velocity gauge: f = -i A(t) on the real a1/r + a2 d/dr blocks).  Pairs in any order and either orientation; a repeated pair adds.
 * Integrator: nsteps fixed steps dt of the six-stage embedded pair of MOD_RK_PARAMS: y_s = a + dt sum_{j<s} A_sj k_j,
 * k_s = -i H(t_n + c_s dt) y_s, c = (0, 2/9, 1/3, 3/4, 1, 5/6); a_{n+1} = a_n + dt sum_s d_s k_s with the 5th-order weights
 * d = (47/450, 0, 12/25, 32/225, 1/30, 6/25); err[q] = max over steps, channels, states of dt |sum_s (d_s - b_s) k_s|,
 * b = (1/9, 0, 9/20, 16/45, 1/12, 0).  No step-size control here (bspatom_tdse_adaptive below resizes the step from err); stability, dt max|E|, is the
 * caller's business (bspatom_tdse_lawson below removes that bound); amplitudes are not checked for finiteness.
 * The library never evaluates a pulse: field[((n*6 + s)*nscan + q)*2 + {0,1}] = Re, Im of f_q(t0 + (n + c_s) dt).
 *   a    [((q*nch + c)*count + n)*2 + {0,1}] (complex128 of shape (nscan, nch, count)); in: a(t0), out: a(t0 + nsteps dt)
 *   snap the amplitudes after steps snap_every, 2 snap_every, .. in the same layout one after the other (nsteps / snap_every of them);
 *        may be NULL;  err: nscan doubles, may be NULL.  nsteps = 0 returns a as given; npairs = 0 (ci, cf, D NULL) is allowed.
 * The sums of an element run over the channel's pairs in ascending p and along each block ascending, on v_mfma_f64_16x16x4_f64; no
 * split depends on nscan, nch, the pair list or the snapshots; no atomics on amplitudes: results are run-to-run bit-identical, a scan
 * does not depend on the other scans of the call, a snapshot equals the result of the shorter run.  Seven launches per step on the
 * problem's stream.  The problem gives the device and the stream only: no solve is needed.
 * The host variant stages the field table and the snapshots through device buffers of at most 256 MiB together
 * (bspatom_set_option("tdse_stage_mb", m) sets another bound; one step's worth at least); the result does not depend on the bound.
 * BSPATOM_ERR_ARG: a null p, E, a, field (nsteps > 0), ci, cf or D (npairs > 0); nch, count or nscan < 1; nsteps < 0; npairs < 0;
 * snap_every < 0; snap given with snap_every = 0; a channel index outside 0..nch-1; ci[p] == cf[p]; a dt that is not finite.
 * The _dev variant: E_dev, D_dev, field_dev, a_dev, snap_dev in device memory of the problem's device; ci, cf, err host pointers. */
int bspatom_tdse_propagate(bspatom_problem *p, int nch, int count, const double *E, int npairs, const int32_t *ci, const int32_t *cf,
                           const double *D, int nscan, int nsteps, double dt, const double *field, double *a, int snap_every,
                           double *snap, double *err);
int bspatom_tdse_propagate_dev(bspatom_problem *p, int nch, int count, const double *E_dev, int npairs, const int32_t *ci,
                               const int32_t *cf, const double *D_dev, int nscan, int nsteps, double dt, const double *field_dev,
                               double *a_dev, int snap_every, double *snap_dev, double *err);

/* The same run with its observables: populations, the field-free energy and the coupling expectation value of every channel, on
 * every obs_every-th step, without a snapshot and without another read of D.  The first 16 arguments are bspatom_tdse_propagate's.
 * Observed steps: n = 0, obs_every, 2 obs_every, .. < nsteps, and always n = nsteps as the last row:
 *   nobs = (nsteps - 1) / obs_every + 2 for nsteps >= 1, nobs = 1 for nsteps = 0; row j describes a(t0 + n_j dt); when obs_every
 *   divides nsteps the rows form a uniform time grid with both ends.  nsteps = 0 is a real call: one row for a as given, no field
 *   needed -- the expectation value of any block operator over any set of wave packets (acceleration form of the dipole: pass the
 *   snapshots as scans and blocks from bspatom_operator_matrix).
 *   obs[((j*nscan + q)*nch + c)*4 + k], sums over the count states n of channel c of scan q:
 *     k = 0     pop = sum_n |a|^2
 *     k = 1     sum_n E[c][n] |a|^2
 *     k = 2, 3  Re, Im of z_c = sum_{p: cf[p] = c} sum_{i,f} conj(a[cf[p]][f]) D_p[i][f] a[ci[p]][i]
 *   With z = sum_c z_c the interaction energy is <H_int> = 2 Re(f z): length gauge <D> = 2 Re z; a velocity-gauge drive
 *   f = -i A on the real blocks gives 2 Im z.  sum_c pop is the norm, sum_c obs[..1] is <H0>.
 * How: on an observed step the first stage runs as tdse_observe_kernel -- stage 0's operand is a(t_n), and before the field enters its
 * epilogue the accumulator of channel c holds sum_{p: cf[p] = c} D_p^T a_ci[p] -- followed by one small kernel that adds the
 * partials of the 64-state row tiles: eight launches on an observed step, seven otherwise, two after the last step.
 * Guarantees:
 *   a, snap and err are bit-identical to bspatom_tdse_propagate* on the same inputs, whatever obs_every is;
 *   a row depends on (E, D, the pair list, count) and that scan's amplitudes alone: not on nscan, the other scans, obs_every, nsteps,
 *   the snapshots or the staging bound;
 *   no floating-point atomics: every sum runs through a tree fixed by count and the channel's entry list, run-to-run bit-identical;
 *   the last row (a measurement with no step after it) has the bits that a stage-0 measurement of the same amplitudes has.
 * The host variant stages the rows with the field and the snapshots under the same bound (tdse_stage_mb).
 * BSPATOM_ERR_ARG: everything bspatom_tdse_propagate names; obs_every < 0; obs given with obs_every = 0; obs_every >= 1 with obs NULL.
 * obs_every = 0 with obs NULL is bspatom_tdse_propagate*.  The _dev variant: obs_dev in device memory, written in place. */
int bspatom_tdse_observe(bspatom_problem *p, int nch, int count, const double *E, int npairs, const int32_t *ci, const int32_t *cf,
                         const double *D, int nscan, int nsteps, double dt, const double *field, double *a, int snap_every,
                         double *snap, double *err, int obs_every, double *obs);
int bspatom_tdse_observe_dev(bspatom_problem *p, int nch, int count, const double *E_dev, int npairs, const int32_t *ci,
                             const int32_t *cf, const double *D_dev, int nscan, int nsteps, double dt, const double *field_dev,
                             double *a_dev, int snap_every, double *snap_dev, double *err, int obs_every, double *obs_dev);

/* The same run with Lawson (integrating-factor) steps of the same tableau: within a step b = exp(+i E tau) a is propagated, so the
 * free evolution is exact and the stability limit comes from |f| ||D|| alone, not from dt max|E|.  The 18 arguments, nobs, the row
 * layout, the field table, the staging under tdse_stage_mb and BSPATOM_ERR_ARG are bspatom_tdse_observe's; obs_every = 0 with obs NULL
 * propagates only.  a, snap and the rows are Schroedinger-picture amplitudes at step boundaries, as in the calls above.
 * The scheme, with A, d, b the tableau above and c = (0, 2/9, 1/3, 3/4, 1, 5/6):
 *   theta_s[c][n] = E[c][n] * (c_s * dt), both products in fp64, c_s the double nearest the fraction;
 *   R_s = cos theta_s - i sin theta_s from the device's fp64 sincos;  R_0 = 1 exactly (stage 0 rotates nothing)
 *   w_s = a_n + dt sum_{j<s} A_sj kappa_j                      (the sums of the plain scheme, in the same order)
 *   y_s = R_s .* w_s                                           (the operand of the products)
 *   g_s[c] = sum_{p: cf[p]=c} f_q(t_n + c_s dt) D_p^T y_s[ci[p]] + sum_{p: ci[p]=c} conj(f_q) D_p y_s[cf[p]]
 *   kappa_s = conj(R_s) .* (-i g_s)                            (no E .* y term)
 *   a_{n+1} = R_4 .* (a_n + dt sum_s d_s kappa_s)              (c_4 = 1: R_4 = exp(-i E dt))
 *   err[q] = max over steps, channels, states of dt |sum_s (d_s - b_s) kappa_s|
 * One small kernel builds the table of the R_s (five complex entries per state, s = 1 .. 5; the entry of s = 4 also serves the step)
 * once per call from E on the problem's stream; then seven launches per step, eight on an observed one, as above, with the same
 * products and the same reads of D; every element pays one complex rotation in the operand load and one in the epilogue.
 * Guarantees:
 *   results are run-to-run bit-identical (no floating-point atomics, no split of a sum, no summation order that depends on nscan, nch,
 *   the pair list, the snapshots, obs_every or the staging bound); a scan does not depend on the other scans of the call;
 *   a snapshot equals the result of the shorter run, and a run continued from a snapshot equals the long run;
 *   a, snap and err do not depend on obs_every or the staging bound;
 *   an observed row has the bits of a bspatom_tdse_observe call with nsteps = 0 on the same amplitudes;
 *   with npairs = 0, err is exactly 0 and |a| changes only by the rounding of the rotations;
 *   a call with nsteps = 0 returns what bspatom_tdse_observe* returns, bit for bit.
 * What the scheme does not give: accuracy still needs a dt that resolves the field and the Bohr frequencies E_i - E_j between
 * populated, coupled states.  What is removed is the stability bound from states that carry no population.  The result is not that
 * of bspatom_tdse_propagate bit for bit: both are 5th-order approximations of the same solution. */
int bspatom_tdse_lawson(bspatom_problem *p, int nch, int count, const double *E, int npairs, const int32_t *ci, const int32_t *cf,
                        const double *D, int nscan, int nsteps, double dt, const double *field, double *a, int snap_every,
                        double *snap, double *err, int obs_every, double *obs);
int bspatom_tdse_lawson_dev(bspatom_problem *p, int nch, int count, const double *E_dev, int npairs, const int32_t *ci,
                            const int32_t *cf, const double *D_dev, int nscan, int nsteps, double dt, const double *field_dev,
                            double *a_dev, int snap_every, double *snap_dev, double *err, int obs_every, double *obs_dev);

/* The same run with static blocks beside the driven couplings: terms of the Hamiltonian that the field does not multiply and that enter
 * without a conjugate partner -- a complex absorbing potential -i W(r) (in-channel blocks <n| W |n'> of bspatom_operator_matrix,
 * l_ini = l_fin), a static field, a perturbing potential, a second, constant drive.  The first 18 arguments are bspatom_tdse_observe's,
 * unchanged in meaning; scheme: 0 = the plain tableau of bspatom_tdse_propagate, 1 = the Lawson steps of bspatom_tdse_lawson.
 *   W[(j*count + i)*count + f], j < nstat: static block j, i a state of channel si[j], f of sf[j] (bspatom_operator_matrix's layout with
 *   count_ini = count_fin = count); si[j] == sf[j] is allowed and is the main case.  Block j adds to the right-hand side of i da/dt of
 *   channel sf[j] ONLY:   skind[j] = 0:  + W_j^T a_si[j]        skind[j] = 1:  - i W_j^T a_si[j],     (W^T a)[f] = sum_i W[i][f] a[i].
 *   No conjugate partner is added: a Hermitian cross-channel term is two blocks, (si, sf, W) and (sf, si, W^T).  Symmetry and sign are
 *   the caller's business and are not checked (a symmetric positive kind-1 block absorbs, its negative feeds).  Static blocks do not
 *   see the field.  Several blocks on one channel add, in ascending j, after the channel's driven entries.
 * With S(y) the sum of these terms:  plain scheme  k_s = -i (E y_s + driven terms + S(y_s));  Lawson  g_s gains S(y_s), y_s = R_s w_s,
 * kappa_s = conj(R_s) (-i g_s) as before: the free phases stay exact, and dt ||W|| joins dt |f| ||D|| as the caller's stability business
 * (for the plain scheme, beside dt max|E|).
 * Rows: nobs as in bspatom_tdse_observe, obs[((j*nscan + q)*nch + c)*6 + k]:
 *     k = 0 .. 3  as in bspatom_tdse_observe
 *     k = 4, 5    Re, Im of s_c = sum_f conj(a_c[f]) S_c[f], S_c the static right-hand side of channel c evaluated on a(t_n)
 *   sum_c Re s_c is the energy of the Hermitian static terms; d pop_c/dt from the static terms is 2 Im s_c, for a symmetric in-channel
 *   absorber -2 <W>_c: the norm lost per channel, integrated over the rows, is the ionisation yield.  nsteps = 0 is a real call, as in
 *   bspatom_tdse_observe: one row measuring a as given.
 * How: a channel's entry list carries its static entries behind the driven ones; -i W^T y = W^T (-i y), and -i y is the Re/Im column
 * exchange with a sign, done while the operand tile is staged, so both kinds run the same real product into ONE more accumulator,
 * which the epilogue adds after the driven terms.  On an observed step stage 0 also chains conj(a) . (that accumulator): s_c, from
 * what the kernel already holds, with no snapshot and no second read of W.  The launches per step are those of the scheme.
 * Guarantees:
 *   1. with nstat = 0, a, snap, err and k = 0 .. 3 of every row have the bits of bspatom_tdse_observe (scheme 0) or bspatom_tdse_lawson
 *      (scheme 1) -- the same kernels run -- and k = 4, 5 are exactly 0;
 *   2. with static blocks, k = 0 .. 3 of a row have the bits of a bspatom_tdse_observe call with nsteps = 0 on the same amplitudes;
 *   3. results are run-to-run bit-identical: no floating-point atomics, no split of a sum along K;
 *   4. the summation order of an element depends on count and on its channel's driven and static lists alone; a channel without a
 *      static entry computes what it computes in the call without static blocks;
 *   5. a scan does not depend on the other scans of the call;
 *   6. a snapshot equals the result of the shorter run;
 *   7. nothing depends on obs_every or on the staging bound (tdse_stage_mb).
 * The host variant uploads W once per call; like D it is not counted in the staging bound.
 * BSPATOM_ERR_ARG: everything bspatom_tdse_observe names; scheme outside {0, 1}; nstat < 0; nstat > 0 with a null si, sf, skind or W;
 * a channel index outside 0..nch-1; skind outside {0, 1}.  The _dev variant: W_dev in device memory; si, sf, skind host pointers. */
int bspatom_tdse_static(bspatom_problem *p, int nch, int count, const double *E, int npairs, const int32_t *ci, const int32_t *cf,
                        const double *D, int nscan, int nsteps, double dt, const double *field, double *a, int snap_every,
                        double *snap, double *err, int obs_every, double *obs, int scheme, int nstat, const int32_t *si,
                        const int32_t *sf, const int32_t *skind, const double *W);
int bspatom_tdse_static_dev(bspatom_problem *p, int nch, int count, const double *E_dev, int npairs, const int32_t *ci,
                            const int32_t *cf, const double *D_dev, int nscan, int nsteps, double dt, const double *field_dev,
                            double *a_dev, int snap_every, double *snap_dev, double *err, int obs_every, double *obs_dev, int scheme,
                            int nstat, const int32_t *si, const int32_t *sf, const int32_t *skind, const double *W_dev);

/* The same run with several drive fields, each driven block naming its own: a field with components along more than one axis (r_0 on one
 * field, r_{+1} on a second: any polarisation and direction), a non-collinear two-colour pulse, a probe along another axis or in the
 * other gauge, a multipole driven by A(t)^2.  The first 24 arguments are bspatom_tdse_static's, unchanged in meaning (scheme 0 plain,
 * 1 Lawson; the static blocks as there).
 *   nfield  the number of fields, 1 .. BSPATOM_TDSE_MAX_FIELDS (more: BSPATOM_ERR_UNSUPPORTED);
 *   fidx[p] (host pointer, also for the _dev variant) the field of pair p, 0 .. nfield-1; NULL only with nfield = 1: all 0;
 *   field[(((n*6 + s)*nfield + g)*nscan + q)*2 + {0,1}]: f_{g,q} at stage s of step n.  The host variant stages the table under
 *   tdse_stage_mb as the other calls do; one step's worth is 12*nfield*nscan doubles.
 *   i da_c/dt = E_c .* a_c + sum_{p: cf[p] = c} f_{fidx[p],q}(t) D_p^T a_ci[p] + sum_{p: ci[p] = c} conj(f_{fidx[p],q}(t)) D_p a_cf[p] + S_c(a)
 * Two pairs between the same two channels with different fidx are legal ("a repeated pair adds").
 * Rows: nobs as in bspatom_tdse_observe, RW = 4 + 2*nfield doubles wide, obs[((j*nscan + q)*nch + c)*RW + k]:
 *     k = 0, 1                 population and sum E |a|^2, as in bspatom_tdse_observe
 *     k = 2, 3                 Re, Im of z_{c,0}
 *     k = 4, 5                 Re, Im of s_c, as in bspatom_tdse_static
 *     k = 4 + 2g, 5 + 2g       Re, Im of z_{c,g}, g = 1 .. nfield-1
 *   z_{c,g} = sum over the pairs p with cf[p] = c and fidx[p] = g of conj(a_cf) . D_p^T a_ci;  <H_int> = sum_g 2 Re(f_g z_g).  With
 *   nfield = 1 this is bspatom_tdse_static's row of 6.  nsteps = 0 is a real call: the expectation values of up to
 *   BSPATOM_TDSE_MAX_FIELDS block operators over any set of packets in one call.
 * How: the field enters the stage only in its epilogue, so every field has its own pair of accumulators and an entry's products go into
 * the pair of its field: the same reads of D and the same matrix instructions as with one field, no split along K, no atomics.  The limit
 * of 3: every field costs two more accumulators of 8 registers and its epilogue values; with three fields no stage needs scratch, and
 * the stages hold 168 .. 176 registers, at the edge of three waves per SIMD (two fields: 136 .. 152, three waves).
 * Guarantees:
 *   1. with nfield = 1, a, snap, err and obs have the bits of bspatom_tdse_static on the same inputs -- the same kernels run;
 *   2. with more fields, k = 0, 1 of a row have the bits of a bspatom_tdse_observe call with nsteps = 0 on the same amplitudes; z_{c,g}
 *      has the bits of such a call given only the pairs with fidx = g, in their order; s_c has the bits of a bspatom_tdse_static call
 *      with nsteps = 0 and the same static blocks;
 *   3. results are run-to-run bit-identical;
 *   4. a scan does not depend on the other scans of the call;
 *   5. a snapshot equals the result of the shorter run;
 *   6. nothing depends on obs_every or on the staging bound (tdse_stage_mb);
 *   7. the order of an element's sums depends on count and on its channel's lists alone: the entries are walked in ascending p, each
 *      into the accumulator of its field; the epilogue adds the fields in ascending g, within a field in the order of the other calls;
 *      the static accumulator comes after that.
 * BSPATOM_ERR_ARG: everything bspatom_tdse_static names; nfield < 1; an fidx entry outside 0..nfield-1; fidx NULL with nfield > 1 and
 * npairs > 0. */
#define BSPATOM_TDSE_MAX_FIELDS 3
int bspatom_tdse_fields(bspatom_problem *p, int nch, int count, const double *E, int npairs, const int32_t *ci, const int32_t *cf,
                        const double *D, int nscan, int nsteps, double dt, const double *field, double *a, int snap_every,
                        double *snap, double *err, int obs_every, double *obs, int scheme, int nstat, const int32_t *si,
                        const int32_t *sf, const int32_t *skind, const double *W, int nfield, const int32_t *fidx);
int bspatom_tdse_fields_dev(bspatom_problem *p, int nch, int count, const double *E_dev, int npairs, const int32_t *ci,
                            const int32_t *cf, const double *D_dev, int nscan, int nsteps, double dt, const double *field_dev,
                            double *a_dev, int snap_every, double *snap_dev, double *err, int obs_every, double *obs_dev, int scheme,
                            int nstat, const int32_t *si, const int32_t *sf, const int32_t *skind, const double *W_dev, int nfield,
                            const int32_t *fidx);

/* The run of bspatom_tdse_static (one field, driven pairs, static blocks, scheme 0 plain or 1 Lawson) with step-size control on the device
 * from the embedded estimate.  The first 24 arguments are bspatom_tdse_static's with two changes of meaning: dt and nsteps describe the
 * COARSE grid t0 + n dt, and the field arrives as a node table fn that the library interpolates (the stage times are not known in advance).
 * The step grid.  The controller's state is (n, m, j): coarse step 0 <= n < nsteps, level 0 <= m <= max_level, position 0 <= j < 2^m;
 * the step is h = ldexp(dt, -m) and starts at t0 + dt (n + j / 2^m).  It starts at (0, level0, 0).  After an attempt, e = max_q err_q,
 * err_q = h max |sum_s (d_s - b_s) k_s| of that attempt (the estimate of the other calls with h in the place of dt):
 *     e <= tol                          accepted
 *     not, and m == max_level           accepted as FORCED and counted (also an e that does not compare, a NaN)
 *     otherwise                         rejected: (n, m + 1, 2 j), a untouched
 *   after an accepted step: j += 1; if e <= tol * 0.015625 and m > 0 and j is even: m -= 1, j >>= 1 (the local error scales as h^5, a
 *   doubled step multiplies it by 32; the factor 2 left over keeps a coarsened step from being rejected at once); if j == 2^m:
 *   n += 1, j = 0.  The level is carried across coarse steps.  tol = +inf never rejects.  max_level <= BSPATOM_TDSE_MAX_LEVEL.
 *   Stage times: x_s = ldexp((double)j + c_s, -m), t_s = t0 + dt * ((double)n + x_s), c_s the double nearest the fraction; IEEE operations.
 *   Attempts per coarse step: at most 2^max_level accepted; a rejection either deepens the level or follows a coarsening, of which there
 *   is at most one per accepted step: no more than 2^(max_level + 1) + max_level attempts.  A run that exceeds this is an internal error:
 *   BSPATOM_ERR_HIP with a message on stderr.
 * The field.  nsub >= 1 intervals per coarse step, node i at t0 + i dt / nsub, i = 0 .. nsteps * nsub:
 *     fn[((i*2 + k)*nscan + q)*2 + {0,1}], k = 0: f_q, k = 1: d f_q / dt.
 *   At x_s: i_loc = min((int)floor(x_s * nsub), nsub - 1), u = x_s * nsub - i_loc, hf = dt / nsub, with i = n nsub + i_loc
 *     omu = 1 - u; omu2 = omu * omu; u2 = u * u;
 *     h00 = (1 + 2 u) * omu2;  h10 = u * omu2;  h01 = u2 * (3 - 2 u);  h11 = u2 * (u - 1);
 *     f = ((h00 * f_i + (h10 * hf) * f'_i) + h01 * f_{i+1}) + (h11 * hf) * f'_{i+1}
 *   in IEEE multiplies and adds in exactly this order, no FMA, Re and Im independently.  THE EQUATION THAT IS INTEGRATED IS THE ONE WITH
 *   THIS PIECEWISE-CUBIC FIELD: it is C1 and depends on fn alone; how well it follows the caller's pulse is the caller's choice of nsub.
 * What comes back:
 *   a, snap, err as in bspatom_tdse_static; a snapshot after every snap_every-th COARSE step; err[q] the maximum over accepted steps.
 *   obs: rows of 6 for the coarse steps 0, obs_every, .. < nsteps and the final state (nobs as in bspatom_tdse_observe): a uniform time
 *   grid whatever the controller does.
 *   stats[6]: accepted, rejected, forced steps, the deepest level of an attempt, the level at the end (fed back as level0 it continues a
 *   run), attempts; all counted whether logged or not.
 *   the log of the first log_cap attempts (t = 0, 1, ..): log_i[4 t] = (n, m, j, flag), flag 0 rejected, 1 accepted, 2 forced;
 *   log_e[t*nscan + q] the estimate per scan; log_f[((t*6 + s)*nscan + q)*2 + {0,1}] the field values the attempt used.
 * How: a control block in device memory holds (n, m, j), the last decision, a done flag, the six field values per scan of the coming
 * attempt and the counters.  An attempt is a fixed sequence of launches: the six stages of the static call (tdse_stage.h with its ADAPT
 * flag: h from the block by one load and ldexp, the field from the block; stage 0 observing, with the reduction to the row the block
 * names, on every attempt when rows are asked for), the step into a CANDIDATE buffer, tdse_adapt_control_kernel (one workgroup: judges,
 * advances (n, m, j), writes the log entry, interpolates the field of the coming attempt, sets done at the end) and
 * tdse_adapt_commit_kernel, which copies an accepted candidate into a and writes its snapshot: 9 launches, 10 with rows.  No kernel waits
 * for another.  The host enqueues attempts in groups of 16 (bspatom_set_option("tdse_adapt_group", g) sets another size), copies the
 * block back, synchronises and goes on until done; launches enqueued
 * behind the end return at their first instruction.  Lawson: one phase table per level 0 .. max_level, each from tdse_phase_kernel with
 * dt = h, before the first attempt.  The host variant stages fn, the snapshots and the rows under tdse_stage_mb by groups of coarse steps.
 * Guarantees:
 *   1. chain identity: the accepted steps of the log, replayed in order as bspatom_tdse_static calls with nsteps = 1, dt = h of the step
 *      and the (1, 6, nscan) table from log_f, reproduce a, every snapshot, the per-step err (= log_e) and k = 0 .. 5 of every row bit
 *      for bit: the stage arithmetic is the static call's, the controller only chooses h;
 *   2. fixed-step identity: with tol = +inf and level0 = 0, a, snap, err and the rows equal one bspatom_tdse_static call with nsteps, dt
 *      and log_f as its table, bit for bit;
 *   3. every decision in the log follows from the logged estimate by the rule above, exactly;
 *   4. results are run-to-run bit-identical; nothing depends on obs_every, snap_every, log_cap, the enqueue group size or the staging bound;
 *   5. a run continued from a snapshot with level0 = stats[4] of the shorter run equals the long run, bit for bit;
 *   6. THE STEP SEQUENCE DEPENDS ON ALL SCANS OF THE CALL, because the worst one decides; given the sequence, a scan's amplitudes depend
 *      on that scan alone (guarantee 1 with a single scan in each replay call).
 * What it does not give: a forced step can exceed tol (stats[2] counts them: raise max_level or shorten dt); tol bounds the local
 * estimate of the 4th-order formula per step, not the global error.
 * BSPATOM_ERR_ARG: everything bspatom_tdse_static names (fn in the place of field); tol not positive or NaN; max_level < 0; level0
 * outside 0..max_level; nsub < 1; fn NULL with nsteps > 0; stats NULL; log_cap < 0; log_cap > 0 with a null log array.
 * BSPATOM_ERR_UNSUPPORTED: max_level > BSPATOM_TDSE_MAX_LEVEL.  The _dev variant: fn_dev and the three log arrays in device memory as
 * well; stats and err host pointers. */
#define BSPATOM_TDSE_MAX_LEVEL 16
int bspatom_tdse_adaptive(bspatom_problem *p, int nch, int count, const double *E, int npairs, const int32_t *ci, const int32_t *cf,
                          const double *D, int nscan, int nsteps, double dt, const double *fn, double *a, int snap_every, double *snap,
                          double *err, int obs_every, double *obs, int scheme, int nstat, const int32_t *si, const int32_t *sf,
                          const int32_t *skind, const double *W, int nsub, double tol, int max_level, int level0, int64_t *stats,
                          int log_cap, int32_t *log_i, double *log_e, double *log_f);
int bspatom_tdse_adaptive_dev(bspatom_problem *p, int nch, int count, const double *E_dev, int npairs, const int32_t *ci,
                              const int32_t *cf, const double *D_dev, int nscan, int nsteps, double dt, const double *fn_dev,
                              double *a_dev, int snap_every, double *snap_dev, double *err, int obs_every, double *obs_dev, int scheme,
                              int nstat, const int32_t *si, const int32_t *sf, const int32_t *skind, const double *W_dev, int nsub,
                              double tol, int max_level, int level0, int64_t *stats, int log_cap, int32_t *log_i_dev, double *log_e_dev,
                              double *log_f_dev);

/* The TDSE in the B-spline basis itself, Crank-Nicolson steps on the coupled banded LU: the spline-basis entry points and their
 * description are in bspatom_tdse_spline.h beside this file, which is part of this header (the twelve calls above are the eigenbasis
 * family; the spline call has another argument list, bspatom_resolvent_coupled's, and its own guarantees S1 - S5). */
#include "bspatom_tdse_spline.h"
/* The same equation with one operator term by split Crank-Nicolson steps, nch independent systems of half-width k - 1 per substep and
 * no limit on the channels: bspatom_tdse_split.h, a part of this header like the one above, with its guarantees P1 - P4. */
#include "bspatom_tdse_split.h"
/* Expectation values <c| B (x) G |c> on packets in the spline basis -- the induced dipole, the dipole acceleration -- in a call of
 * their own and as further row entries along a split-step run: bspatom_spline_expect.h, a part of this header like the two above. */
#include "bspatom_spline_expect.h"
/* How a packet in the spline basis is distributed over energy -- photoelectron spectra by the window operator, a product of resolvents
 * with the S-norm at its end --: bspatom_spline_window.h, a fourth part of this header, with its guarantees W1 - W6. */
#include "bspatom_spline_window.h"

/* The eigenvector the reference consumes (l_ini, n0_ini; matrices.f90:267) is computed during bspatom_solve when its channel is in
 * the batch.  On the band route its eigenvalue comes from the pencil's inertia right after the assembly (csrc/bandsect.hip), and the
 * solve checks it against the spectra when they are there.  state of the last solve: 0 = no early vector (other route, channel not in
 * the batch, BSP_VEC_EARLY=0), 1 = early vector kept, -1 = check failed, vector dropped (bspatom_eigvec computes it on demand). */
int bspatom_early_vector_state(const bspatom_problem *p, int32_t *state);
/* Per-stage device time of the last bspatom_solve* call, HIP events on the library's stream
 * (milliseconds): [0] point table + bands, [1] Cholesky + standard form, [2] sy2sb,
 * [3] sb2st, [4] bisection, [5] total.  Also the number of launches of the sy2sb GEMM. */
int bspatom_last_timing(const bspatom_problem *p, double ms[6]);

/* Per-kernel launch durations (measurement only; no reference counterpart).  With bspatom_set_option("ktime", 1) every launch
 * of the kernels below is bracketed by two HIP events on its own stream; this call waits for the device, sums the elapsed
 * times and launch counts per slot since the previous call into ms[] / launches[] (cap >= the slot count, which it returns)
 * and forgets them.  Slots: 0 rank-128 update (syr2k), 1 symm, 2 panel QR, 3 the small products of the panel chain,
 * 4 sb2sb_mfma_kernel, 5 sbr_rows_kernel<8> / <16> (sb16st_kernel with BSP_SB16_ROWS=0), 6 batched bisection, 7 Cholesky + standard form,
 * 8 the band route's reduction (crawford.hip), 9 operator_band_kernel (opmat.hip), 10 tdse_stage_kernel and tdse_observe_kernel, their Lawson and static variants and tdse_phase_kernel (tdse.hip, tdse_static.hip), and every kernel of bspatom_tdse_adaptive (tdse_adapt.hip: its stages, step, reduction, tdse_adapt_control_kernel, tdse_adapt_commit_kernel);
 * bspatom_kernel_slot_name(i) names them.  Launches on different streams overlap: the sums are sums of launch durations, not wall time. */
int bspatom_kernel_times(double *ms, int32_t *launches, int cap);
const char *bspatom_kernel_slot_name(int slot);

/* ---- the one exchange of the sharded path (csrc/comm.hip) ----------------------------------- */
/* One process per GPU, the l-loop of matrices.f90:242-248 sharded: the ranks exchange nothing while they solve; at the end their
 * result records are gathered.  These calls give a host without Python (bsp_atom_host.x) the RCCL all-gather that
 * bspatom_amd/parallel.py issues through torch.distributed.  No reference counterpart (the reference is one process).
 *   bspatom_run_token   an id shared by the processes of ONE launch and by no other launch: "<pid of the launcher>.<its start
 *                       time>[.<TORCHELASTIC_RUN_ID>]" (buf: >= 128 bytes).  Also names the files of the no-RCCL fallback.
 *   bspatom_comm_create collective over `world` processes (rank 0 .. world-1), each on its own GPU (the device of the process's
 *                       problems).  RCCL is loaded here (dlopen), its unique id travels through `dir`/ncclid.<token>.
 *                       BSPATOM_ERR_UNSUPPORTED (before anything is exchanged, the same on every rank): more ranks than GPUs
 *                       (ranks share a device) or no librccl -- the caller falls back to its file exchange.
 *   bspatom_comm_allgather  recv[r*count .. (r+1)*count) = rank r's send[0 .. count) on every rank (host buffers).
 *   bspatom_comm_collectives  number of all-gathers issued on this communicator. */
typedef struct bspatom_comm bspatom_comm;
int bspatom_run_token(char *buf, int cap);
int bspatom_comm_create(int rank, int world, const char *dir, bspatom_comm **out);
int bspatom_comm_allgather(bspatom_comm *c, const double *send, double *recv, long count);
int bspatom_comm_collectives(const bspatom_comm *c);
void bspatom_comm_destroy(bspatom_comm *c);

/* ---- LAPACK symbol boundary ---------------------------------------------------- */
/* Fortran-77 ABI of DSYGV as called at matrices.f90:248.  ITYPE=1, UPLO='U' or 'L'; A and B must
 * be banded with half-width <= 15 (they are, at the reference's call site); JOBZ='N' returns the
 * eigenvalues, JOBZ='V' additionally returns all n B-orthonormal eigenvectors (inverse iteration,
 * re-orthogonalised inside clusters).  LWORK >= max(1, 3n-1) or -1 (query) as for DSYGV.
 * info = -k for a bad k-th argument (LAPACK numbering), n+i if B is not positive definite, n if the GPU
 * path failed (message on stderr).  Trailing hidden CHARACTER lengths: size_t, as flang / gfortran pass them.
 * libbspatom_lapack.so exports the same routine under the plain name `dsygv_` (csrc/lapack_shim.c). */
void bsp_dsygv_(const int *itype, const char *jobz, const char *uplo, const int *n, double *a,
                const int *lda, double *b, const int *ldb, double *w, double *work, const int *lwork,
                int *info, size_t jobz_len, size_t uplo_len);

/* bsp_dsygv_ keeps its device buffers in a process-wide pool between calls (the reference calls DSYGV once per l in a loop); at
 * most 4 GiB stay parked after a call.  This returns every idle buffer of that pool to the driver. */
void bspatom_release_scratch(void);

/* ---- run-time switches (tests, A/B comparisons) ----------------------------------------------- */
/* The BSP_* environment variables of DESIGN.md 4.4 are read once per process; these two calls read and
 * change the same switches afterwards, by lower-case name without the prefix ("sb2st_ring",
 * "sb2st_version", "sb2st_force_abort", "panel_qr", "bisect" ...).  Unknown name: BSPATOM_ERR_ARG.
 * No reference counterpart (the reference has no switches on this path). */
int bspatom_set_option(const char *name, int value);
int bspatom_get_option(const char *name, int *value);

/* ---- stage-level entry points (parity tests, profiling; host buffers, column-major) ---------- */
/* C[b] = alpha * op(A[b]) op(B[b]) + beta * C[b], element strides as in csrc/common.h GemmDesc. */
int bspatom_stage_gemm(int M, int N, int K, int batch, const double *A, long sAm, long sAk, long bA,
                       long lenA, const double *B, long sBk, long sBn, long bB, long lenB, double *C,
                       long sCm, long sCn, long bC, long lenC, double alpha, double beta);
/* S = U^T U and C_l = U^-T H_l U^-1 from upper bands (n, k as above); C: nl x npad x npad. */
int bspatom_stage_standard_form(int n, int k, int nl, const double *SB, const double *HB, double *UB,
                                double *C, int32_t *info);
/* dense symmetric (npad multiple of 64, full storage) -> lower band AB[d + j*128], d <= 64 */
int bspatom_stage_sy2sb(int npad, int batch, const double *A, double *AB);
/* the panel factorisation of sy2sb alone (tests): panel = A[c0+64 .., c0 .. c0+63] of each dense npad x npad matrix (column-major).
 * On return the panel holds [R; 0]; V[b][c][0..m-1], W[b][c][0..m-1] (m = npad - c0 - 64) with I - V T V^T = I - W V^T orthogonal and
 * (I - W V^T)^T panel = [R; 0].  The panel QR inside LAPACK DSYTRD's blocked reduction (matrices.f90:248). */
int bspatom_stage_panel(int npad, int c0, int batch, double *A, double *V, double *W);
/* band (AB as above, leading n x n) -> tridiagonal d[n], e[n-1] (ld npad) */
int bspatom_stage_sb2st(int n, int npad, int batch, const double *AB, double *d, double *e);
/* first half of the two-step route (sb2st_version 9): band 64 -> band 16 in place, same layout */
int bspatom_stage_sb2sb(int n, int npad, int batch, double *AB);
/* band route (csrc/crawford.hip; BSP_ROUTE): the banded pencil (H_l, S) of nl channels, upper bands as bspatom_assemble returns
 * them, to the banded standard-form matrix orthogonally similar to L^-1 H_l L^-T (S = L L^T), half-width 2 (k - 1) - 1 <= 15,
 * in the layout above: AB[l][d + j*128] = A_l(j + d, j), npad = n rounded up to 64.  k - 1 <= 8.  info: 0, or the order of the
 * minor at which the factorisation of the (index-reversed) overlap broke down.  Replaces DPOTRF + DSYGST + the dense stage of
 * DSYTRD inside DSYGV (matrices.f90:248) in 6 n^2 (k - 1) flop and no dense matrix. */
int bspatom_stage_crawford(int n, int k, int nl, const double *SB, const double *HB, double *AB, int32_t *info);
/* eigenvalue m (0-based, ascending) of ONE banded pencil (H, S), upper bands as bspatom_assemble returns them, k - 1 <= 8, by
 * multisection on the inertia of H - x S (csrc/bandsect.hip): what starts the inverse iteration for the eigenvector the reference
 * consumes (matrices.f90:267) while the reductions of the batch are still running */
int bspatom_stage_band_eigenvalue(int n, int k, const double *SB, const double *HB, int m, double *lambda);
/* eigenvalues of tridiagonal matrices, ascending */
int bspatom_stage_bisect(int n, int batch, const double *d, const double *e, double *w);

#ifdef __cplusplus
}
#endif
#endif
