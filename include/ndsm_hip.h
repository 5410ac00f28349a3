/* libndsm_hip - C ABI of the MI355X-native multigrid path for NDSM.
 *
 * PART 1 is the drop-in boundary: exactly the dynamic symbols the reference's
 * shared object ndsmf.so exports (verified with `nm -D` on a build of
 * /root/reference/fortran), i.e. what its Python front-end binds through
 * ctypes (ndsm.py:136-207).  Names, argument lists, option-slot values and
 * return conventions are the reference's; each prototype cites the
 * BIND(C) procedure it replaces.
 *
 * PART 2 is additive (SURVEY.md 8b last row, 8f-4): a scalar Poisson entry, a
 * persistent device-resident solver handle, timing hooks.  Nothing in part 1
 * changes meaning because part 2 exists; all additive option slots are slots
 * the reference leaves unused (value 0 = reference behaviour).
 *
 * All arrays are Fortran order (x fastest): a numpy array of shape (3,nz,ny,nx)
 * in C order IS the (nx,ny,nz,3) array meant here (ndsm.py:161,210).
 * Everything is double precision; sizes in the reference ABI are C int / size_t.
 *
 * Errors: 0 = ok, 1 = V-cycle iteration did not reach vc_tol (reference
 * semantics), >= 9001 = device/runtime failure (text via ndsm_hip_last_error
 * and on stderr).  The library has no CPU fallback: without an MI355X every
 * solve returns 9001.  It never calls exit()/STOP (the reference does on
 * internal asserts, ndsm_root.f90:317-455).
 *
 * Threading: blocking calls, one library-owned HIP stream; not re-entrant (as
 * the reference: module-global DEBUG flag, ndsm_root.f90:64).
 */
#ifndef NDSM_HIP_H
#define NDSM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* =====================================================================
 * PART 1 - the reference ABI
 * ===================================================================== */

/* Replaces ndsm_vector_solve, fortran/ndsm_python_wrapper.f90:56-158.
 *   nsize    nx*ny*nz*3                                   (by value, :64)
 *   nshape4  [nx, ny, nz, 3]                              (:65, ndsm.py:161)
 *   ioptc    16 integer options, in/out; slots from the getters below
 *   ropt     16 real options, in/out
 *   x,y,z    mesh vectors of length nx, ny, nz (uniform spacing assumed)
 *   A        in: initial guess of the three Laplace solves (ndsm.py passes
 *            zeros); out: vector potential, (nx,ny,nz,3)
 *   B        in: field whose NORMAL component on the six faces is the
 *            boundary data; out: curl A, (nx,ny,nz,3)
 * returns ioptc[IOPT_IERR]: 0 ok, 1 not converged / bad mesh (see DESIGN.md
 * quirk Q3' for which solve's flag the reference actually returns).
 * After a device / runtime failure (>= 9001) the contents of A and B are unspecified (a worker thread has
 * begun to touch and fill them behind the solves). */
int ndsm_vector_solve(size_t nsize, const int *nshape4, int *ioptc, double *ropt, const double *x,
                      const double *y, const double *z, double *A, double *B);

/* Option-slot getters, fortran/ndsm_python_wrapper.f90:164-234.  ndsm.py never
 * hard-codes a slot; it asks the library (ndsm.py:155-174). */
int get_iopt_len(void);         /* :164  -> 16 */
int get_iopt_ierr(void);        /* :170  -> 16 (sic: the reference returns IOPT_LEN, not IOPT_IERR = 3) */
int get_iopt_ms(void);          /* :176  -> 0  smoothing sweeps */
int get_iopt_ncycles(void);     /* :182  -> 1  max V-cycles */
int get_iopt_debug(void);       /* :188  -> 5 */
int get_iopt_dumax(void);       /* :194  -> 6  1: max|du| metric, 0: mean|du| */
int get_iopt_iopt_nmaxex(void); /* :200  -> 7  max sweeps of the coarsest-grid solve (the doubled "iopt" is the reference's name) */
int get_iopt_true(void);        /* :206  -> 1 */
int get_iopt_false(void);       /* :212  -> 0 */
int get_ropt_tim(void);         /* :218  -> 2  out: wall time of the call, seconds */
int get_ropt_vtol(void);        /* :224  -> 0  V-cycle tolerance */
int get_ropt_ctol(void);        /* :230  -> 1  coarsest-grid tolerance */

/* =====================================================================
 * PART 2 - additive exports
 * ===================================================================== */

/* additive option slots (unused in the reference, ndsm_vector_potential.f90:40-57) */
int get_iopt_fail3d(void);   /* -> 8  out: bit c set if 3-D solve c (0=Ax,1=Ay,2=Az) missed vc_tol */
int get_iopt_ngrids(void);   /* -> 9  in : cap on the number of grid levels, 0 = reference rule
                                          floor(log2(nmin/2)) (ndsm_vector_potential.f90:631-632) */
int get_iopt_ncyc_out(void); /* -> 10 out: V-cycles used by the last solve that iterated */
int get_ropt_dulast(void);   /* -> 3  out: du of its last V-cycle */
/* Both are written by every call, never left from an earlier one: the first 3-D solve (A_x) always writes them, a
 * later component only if it ran more than one V-cycle.  When no solve iterated - ioptc[get_iopt_ncycles()] <= 0 -
 * they hold 0 and the largest finite double (Fortran HUGE, 1.797...e308: "no du was measured"), every solve counts
 * as not converged (ioptc[3] = 1, all bits of get_iopt_fail3d() set) and A keeps the initial guess with the
 * boundary values written into it.
 * Negative counts: ndsm_vector_solve and the ndsm_hip_vecpot_* entries take a negative ms, ncycles or nmaxex as 0,
 * as the reference's DO loops do (the slots themselves are returned as passed).  The additive solver handles are
 * stricter: ndsm_hip_mg_create, ndsm_hip_mg_set_ms and ndsm_hip_world_create refuse a negative ms or nmax_exact with
 * 9002; a negative nmax of ndsm_hip_mg_solve / ndsm_hip_world_solve runs no cycle, like 0 (returns 1, *ncycles = 0,
 * *du_last = HUGE, u untouched). */
int get_iopt_prec(void);     /* -> 11 in : 0 fp64 throughout (reference arithmetic); 1 mixed precision for the 3-D
                                          solves: fp64 residual + fp32 correction V-cycle on level 1 (BASELINE
                                          config[4]); where level 1 is too small for the fp32 kernels the
                                          fp64 path runs */

int ndsm_hip_device_count(void);
int ndsm_hip_init(int device);               /* < 0: LOCAL_RANK % device count; idempotent */
/* Releases what the library itself holds on the device (streams, events, metric scratch, the cached
 * vector-potential hierarchy, a live RCCL communicator).  Destroy solver / world handles first.  Any
 * later call re-initialises (ndsm_hip_init may then name another device). */
int ndsm_hip_shutdown(void);
void ndsm_hip_last_error(char *buf, int len);
int ndsm_hip_sync(void);                     /* wait for the library stream */
int ndsm_hip_timer_start(void);              /* hipEventRecord on the library stream */
int ndsm_hip_timer_stop(double *ms);         /* record + synchronise + elapsed */

/* laplace(u) = rhs with 'D'/'N' faces; the scalar problem the reference only
 * reaches internally (solve_poisson_bvp, ndsm_poisson.f90:63-155).
 *   bcs     2*ndim letters: lower faces of dim 1..ndim, then upper faces
 *           (RESHAPE(copt,[ndim,2]), ndsm_poisson.f90:244-245)
 *   u       in: initial guess INCLUDING the Dirichlet face values; out: solution
 *   rhs     may be NULL (= 0);   hist may be NULL (else du per V-cycle)
 * options in the same slots as ndsm_vector_solve; returns 0 / 1 / >= 9001. */
int ndsm_hip_poisson_solve(int ndim, const int *nshape, const double *x, const double *y,
                           const double *z, const char *bcs, int *ioptc, double *ropt, double *u,
                           const double *rhs, double *hist, int hist_len);

/* ---- persistent solver: hierarchy, tables and level arrays stay in HBM ---- */
int ndsm_hip_mg_create(int ndim, const int *nshape, const double *x, const double *y,
                       const double *z, const char *bcs, int ngrids /* 0 = reference rule */, int ms,
                       double ex_tol, int du_max, int nmax_exact, void **handle);
int ndsm_hip_mg_destroy(void *handle);
int ndsm_hip_mg_levels(void *handle, int ngrids_cap, int *shapes /* [ngrids_cap][3] */); /* returns ngrids */
int ndsm_hip_mg_set_ms(void *handle, int ms);
/* mode 0 fp64, 1 mixed where level 1 is large (>= 6 M points), 2 mixed wherever the fp32 kernels cover
 * level 1.  Returns 1 if ndsm_hip_mg_solve will run in mixed precision, 0 if fp64, < 0 bad mode. */
int ndsm_hip_mg_set_precision(void *handle, int mode);
/* which: 0 = u, 1 = rhs, 2 = residual scratch (level-1 sized), 3 = the partner array of u (out-of-place smoother
 * passes leave the result there and the two swap; for tests) */
int ndsm_hip_mg_upload(void *handle, int level, int which, const double *host);
int ndsm_hip_mg_download(void *handle, int level, int which, double *host);
/* declare rhs(1) == 0 (Laplace problem, the vector-potential case): kernels skip reading it; same bits */
int ndsm_hip_mg_zero_rhs(void *handle);
/* op: 0 relax (count sweeps), 1 residual -> scratch, 2 restrict scratch(level) -> rhs(level+1)
 * and zero u(level+1), 3 u(level) += P u(level+1), 4 coarsest-grid solve, 5/6 relax forced to
 * the two-pass / fused kernel, 8 relax (count sweeps) then residual -> scratch with the last
 * sweep and the residual in one launch where the level allows (9: or fail).  Asynchronous. */
int ndsm_hip_mg_op(void *handle, int op, int level, int count);
int ndsm_hip_mg_vcycle(void *handle, int ncycles);   /* asynchronous, no convergence test */
/* V-cycles to vc_tol: returns 0 converged, 1 not, >= 9001 error */
int ndsm_hip_mg_solve(void *handle, double vc_tol, int nmax, double *du_last, int *ncycles,
                      double *hist, int hist_len);
int ndsm_hip_mg_info(void *handle, int64_t *exact_sweeps, int64_t *unconverged_coarse_solves);

/* device memory on the library's GPU for callers without a HIP binding of their own (blocking copies on
 * the library stream); pointers from the caller's own hipMalloc work just as well */
int ndsm_hip_device_alloc(size_t bytes, void **p);
int ndsm_hip_device_free(void *p);
int ndsm_hip_memcpy_h2d(void *d_dst, const void *h_src, size_t bytes);
int ndsm_hip_memcpy_d2h(void *h_dst, const void *d_src, size_t bytes);

/* ---- persistent vector-potential solver ----
 * The reference rebuilds its grid hierarchy per component and per call (ndsm_vector_potential.f90:652-689,
 * ndsm_multigrid_core.f90:165-329).  Here everything that depends on the grid alone - the 3-D hierarchy and
 * its transfer tables, the three 2-D face hierarchies, device arrays for A, B and the six faces - lives in a
 * handle; time-series callers solve again and again on the same mesh.  (ndsm_vector_solve keeps ONE such
 * context internally, keyed by shape, mesh and level cap: a second call on the same mesh skips the set-up
 * without the caller changing anything.  ndsm_hip_shutdown drops it.)
 *   nshape4 = [nx,ny,nz,3], x,y,z as for ndsm_vector_solve; ngrids = level cap (0: reference rule) - a solve
 *   whose ioptc[get_iopt_ngrids()] differs from it fails with 9002.
 *   ndsm_hip_vecpot_solve        A, B HOST arrays: contents, options, return value as ndsm_vector_solve.
 *   ndsm_hip_vecpot_solve_device A, B DEVICE arrays (nx,ny,nz,3) on the library's GPU: B.n is extracted by a
 *                                kernel, nothing crosses PCIe but six fluxes and the 16-byte convergence
 *                                read-backs; results are complete in A, B when the call returns. */
int ndsm_hip_vecpot_create(const int nshape4[4], const double *x, const double *y, const double *z, int ngrids,
                           void **handle);
int ndsm_hip_vecpot_solve(void *handle, int ioptc[16], double ropt[16], double *A, double *B);
int ndsm_hip_vecpot_solve_device(void *handle, int ioptc[16], double ropt[16], double *dA, double *dB);
int ndsm_hip_vecpot_destroy(void *handle);

/* ---- the current-carrying field on the same handle (DESIGN.md "Vector potential of a current-carrying field") ----
 * The potential pipeline returns the potential field B_p = curl A_p of B.n.  These entries return A of the
 * field B itself (curl B != 0: a simulation, a force-free model, a data cube), in the same Coulomb gauge and
 * with the same tangential boundary values as A_p: the three 3-D problems get the right-hand side
 * -(curl_h B)_c (derivq's differences) and keep their boundary letters and Dirichlet data.  Uniform spacing,
 * as for ndsm_hip_vecpot_solve.  Options in the same slots, with the same meaning (ms, with Az's ms = 5;
 * ncycles, nmaxex, dumax, vtol, ctol, ngrids, prec, IOPT_FLXCRL = 4).
 * Returns 0 when every 2-D and 3-D solve reached vc_tol, 1 when at least one did not (NOT the reference's
 * quirk Q3'), >= 9001 errors (a HIP failure such as out of memory comes back as 9001, see
 * ndsm_hip_last_error); ioptc[IOPT_IERR] holds the same value.  ioptc[get_iopt_fail3d()]: bits 0-2 the field
 * solves Ax, Ay, Az; bits 3-5 the potential solves of a helicity call.
 *
 *   ndsm_hip_vecpot_solve_field        HOST arrays (nx,ny,nz,3).  A in: initial guess, out: A.  B in: the whole
 *                                      field (uploaded in full, 24 B/pt), out: curl A + flux-balance fields.
 *   ndsm_hip_vecpot_solve_field_device the same on DEVICE arrays of the library's GPU.
 *   ndsm_hip_vecpot_helicity           HOST arrays.  B in, read only.  A, Ap, Bp out: A of B, the potential
 *                                      field's A_p and B_p (both solves start from zero; A_p, B_p are the bits
 *                                      ndsm_hip_vecpot_solve returns for B and a zero guess).  out[8] (no 4 pi
 *                                      or mu0 factors; trapezoid weights w, h inside and h/2 on the end planes
 *                                      of each axis; B_rec = curl A + balance, the field solve's own output):
 *       out[0] H_R = sum w (A + Ap).(B - Bp)   relative helicity (Finn-Antonsen)
 *       out[1] H_J = sum w (A - Ap).(B - Bp)   helicity of the current-carrying part
 *       out[2] E   = 1/2 sum w |B|^2           out[3] E_p = 1/2 sum w |Bp|^2
 *       out[4] max |B_rec,c - B_c| (all c)     out[5] sqrt(sum w |B_rec - B|^2 / sum w)
 *       out[6] max |div_h B|                   out[7] max |div_h A|
 *                                      The sums are deterministic (fixed reduction order): the same input gives
 *                                      the same bits.  Device memory: five fields of 24 B/pt besides the
 *                                      hierarchy.
 *   ndsm_hip_vecpot_helicity_device    the same on DEVICE arrays; B_rec lives in library scratch.
 * Non-solenoidal input is not corrected: it shows in out[4], out[5] and out[6]. */
int ndsm_hip_vecpot_solve_field(void *h, int ioptc[16], double ropt[16], double *A, double *B);
int ndsm_hip_vecpot_solve_field_device(void *h, int ioptc[16], double ropt[16], double *dA, double *dB);
int ndsm_hip_vecpot_helicity(void *h, int ioptc[16], double ropt[16], const double *B, double *A, double *Ap,
                             double *Bp, double out[8]);
int ndsm_hip_vecpot_helicity_device(void *h, int ioptc[16], double ropt[16], const double *dB, double *dA,
                                    double *dAp, double *dBp, double out[8]);

/* ---- solenoidal projection (divergence cleaning) on the same handle (DESIGN.md "Solenoidal projection") ----
 * The helicity entries assume div B = 0.  These return B' = B - G_h phi, laplace_7(phi) = div_h B - c with all
 * six faces Neumann and c = sum w div_h B / sum w (trapezoid weights w, as above): div_h with derivq's
 * differences, G_h phi the centred difference inside and 0 on the two end planes of each axis, so
 *   - B.n on the six faces is left bitwise untouched: the potential field of B' is that of B, bit for bit;
 *   - a field with div_h B = 0 (each component independent of its own coordinate, say) comes back bitwise;
 *   - c, the uniform part (net boundary flux / volume), cannot be removed by any projection that keeps B.n:
 *     it stays in div_h B' and is reported;
 *   - div_h G_h is the wide stencil, not laplace_7: the projection is approximate (collocated), div_h B' is a
 *     truncation error, O(h^2) relative to the divergence removed, not zero.
 * The solve is the 3-D multigrid with the options in the usual slots (ms, ncycles, nmaxex, dumax, vtol, ctol,
 * ngrids: the handle's), from phi = 0, always fp64 (IOPT_PREC is accepted and ignored).  ioptc[IOPT_IERR],
 * ioptc[get_iopt_ncyc_out()], ropt[get_ropt_dulast()] report the solve.  The all-Neumann hierarchy is created
 * at the first projection on a handle and kept with it.  Device callers chain ndsm_hip_vecpot_project_device
 * -> ndsm_hip_vecpot_helicity_device on the same device arrays, nothing crosses PCIe in between.
 * Without a GPU both return 9001 whatever the handle (a NULL handle with a GPU: 9002); on every error out[4] is
 * cleared, and B is left untouched when the call fails before the projection runs. */
/* B in: the field (nx,ny,nz,3); out: B - G_h phi (B.n on the six faces untouched).
 * phi: (nx,ny,nz) out, may be NULL.  out[4]: [0] c = sum w div_h B / sum w (left in div_h B'),
 * [1] max|div_h B| before, [2] max|div_h B'| after, [3] 1/2 sum w |G_h phi|^2.  0 / 1 / >= 9001. */
int ndsm_hip_vecpot_project(void *h, int ioptc[16], double ropt[16], double *B, double *phi, double out[4]);
int ndsm_hip_vecpot_project_device(void *h, int ioptc[16], double ropt[16], double *dB, double *dphi, double out[4]);

/* ---- DeVore-gauge vector potentials and helicity on the same handle (DESIGN.md "DeVore-gauge vector potentials") --
 * A second, independent gauge for the helicity of ndsm_hip_vecpot_helicity: A_z = 0 (DeVore 2000), A and A_p from
 * cumulative integrals along z, no solve (Valori, Demoulin & Pariat 2012).  H_R and H_J are gauge invariant when
 * B.n = B_p.n on the faces and div B = 0, so the two gauges agree to the discretisation error; a larger gap
 * points at non-solenoidal input or a poorly converged solve.  With h_x, h_y, h_z the handle's spacings (as
 * ndsm_hip_vecpot_solve forms them), trapezoid sums in fp64 in this operand order (k = 0 is z0, k = nz-1 the top):
 *   base plane  b_x(i,0) = 0,  b_x(i,j) = b_x(i,j-1) - (B_z(i,j-1,0) + B_z(i,j,0)) * (0.25 h_y)
 *               b_y(0,j) = 0,  b_y(i,j) = b_y(i-1,j) + (B_z(i-1,j,0) + B_z(i,j,0)) * (0.25 h_x);  A(:,:,0) = (b_x, b_y, 0)
 *   A, up       A_x(k) = A_x(k-1) + (B_y(k-1) + B_y(k)) * (0.5 h_z),  A_y(k) = A_y(k-1) - (B_x(k-1) + B_x(k)) * (0.5 h_z)
 *   A_p, down   A_p(nz-1) = A(nz-1) (the same bits), then for k = nz-2 .. 0
 *               A_p,x(k) = A_p,x(k+1) - (B_p,y(k) + B_p,y(k+1)) * (0.5 h_z)
 *               A_p,y(k) = A_p,y(k+1) + (B_p,x(k) + B_p,x(k+1)) * (0.5 h_z)
 *   A_z = A_p,z = 0 exactly.
 * So curl A = B where div B = 0 (a divergent B shows as a B_z error growing with height, about -int div B dz),
 * and curl A_p = B_p where B_p,z = B_z on the top face.  n x A_p = n x A exactly on the top face; on the side
 * faces as far as B_p.n = B.n there (the difference on an x-face is int_z^z1 (B_p,x - B_x) dz'); on the bottom
 * face n x (A - A_p) is a 2-D gradient, which H_R and H_J do not see.
 * B_p is any field whose B.n matches B's: the library's potential field or the caller's own.  out[8] has the
 * layout of ndsm_hip_vecpot_helicity with B_rec = curl_h A (derivq's differences); out[7] = max |div_h A| is
 * the divergence of the DeVore gauge, not an error.  Deterministic.  Device memory: five fields of 24 B/pt (the
 * host entry stages B, B_p, A, A_p in the handle's scratch; B_rec is always the handle's); no multigrid
 * hierarchy is created.  Returns 0, or >= 9001 errors (9001 without a GPU whatever the arguments, and for a grid
 * whose five fields do not fit in device memory, refused before any allocation; 9002 a NULL handle or array);
 * out[8] is cleared on every failure.
 * Device chain for a DeVore-gauge helicity with the library's potential field: copy B, run
 * ndsm_hip_vecpot_solve_device on the copy (a zero A; the copy becomes B_p), then ndsm_hip_vecpot_devore_device
 * on B and that B_p - nothing crosses PCIe in between.  After ndsm_hip_vecpot_project_device the same chain gives
 * the helicity of the projected field. */
/* B, Bp in (nx,ny,nz,3), HOST arrays; A, Ap out. */
int ndsm_hip_vecpot_devore(void *h, const double *B, const double *Bp, double *A, double *Ap, double out[8]);
/* the same on DEVICE arrays of the library's GPU; A, Ap distinct from each other and from B, Bp */
int ndsm_hip_vecpot_devore_device(void *h, const double *dB, const double *dBp, double *dA, double *dAp,
                                  double out[8]);

/* ---- Field lines, and line integrals along them, on the same handle (DESIGN.md "Field-line tracing and field-line
 * helicity") -------------------------------------------------------------------------------------------------------
 * Traces the field lines of B through nseeds seed points and integrates a second field G along them: with G = A this
 * is the field-line helicity  int A.dl  (Yeates & Page 2018; Moraitis et al. 2019), usually with the DeVore-gauge A of
 * ndsm_hip_vecpot_devore.  The handle supplies the mesh only (lo_d = its first point, h_d = q_d[1] - q_d[0],
 * hi_d = lo_d + (n_d - 1) h_d per axis); no solve runs and no hierarchy is created.
 *   B, G      (nx,ny,nz,3) as everywhere; G may be NULL (every integral is 0)
 *   seeds     (3,nseeds): x, y, z of each seed in physical coordinates
 *   step      > 0, in units of min(h_x,h_y,h_z): ds = step * min(h)
 *   max_steps >= 1, finite; clamped to 2^24.  Every line ends after at most max_steps steps: a closed line costs
 *             max_steps steps and comes back NDSM_HIP_TRACE_UNFINISHED.
 *   direction +1 along B, -1 against B, 0 both.  nl = nseeds lines, or with 0 nl = 2 nseeds: line i (forward) and
 *             line nseeds + i (backward) belong to seed i.
 *   out       ends (3,nl), length (nl), integral (nl) doubles; status (nl), nsteps (nl) int32
 * Semantics, in fp64 in this operand order (device code is built without contraction, so a restatement in the same
 * order gives the same bits):
 *   interpolation  trilinear in the cell c_d = clamp(floor(u_d), 0, n_d - 2), u_d = (r_d - lo_d) / h_d, with the
 *                  unclamped f_d = u_d - c_d (a stage point outside the box extrapolates from the edge cell; a field
 *                  linear in x, y, z is reproduced wherever it is evaluated): along x first,
 *                  c00 = v000 + f_x (v100 - v000) ..., then y, c0 = c00 + f_y (c10 - c00), then z.
 *   ODE            dr/ds = sgn B/|B| (sgn = +1 forward, -1 backward), dI/ds = G.B/|B|, |B| = sqrt((Bx Bx + By By)
 *                  + Bz Bz), G.e = (Gx ex + Gy ey) + Gz ez.  The integrand carries no sgn: a backward line
 *                  accumulates the integral of G.dl taken in the direction of B, from its end to the seed, so for
 *                  both directions integral[i] + integral[nseeds + i] is int G.dl along the whole line through seed
 *                  i from the foot where B enters the box to the foot where it leaves.
 *   step           classical RK4 with fixed ds: k2 at r + (0.5 ds) k1, k3 at r + (0.5 ds) k2, k4 at r + ds k3,
 *                  r' = r + (ds / 6) (((k1 + 2 k2) + 2 k3) + k4), the same weights for I; length is the sum of the
 *                  ds taken.
 *   exit           r' outside [lo, hi]: the step is not accepted.  t = the smallest (face_d - r_d) / (r'_d - r_d)
 *                  over the axes that left (x before y before z on a tie), 0 <= t <= 1, is where the chord r -> r'
 *                  meets a face, and the step is REDONE as a full RK4 step of length t ds from the same r (stage 1
 *                  reused) for r and I alike; length += t ds.  Then the coordinate normal to that face is set to
 *                  the face's value and the other two are clamped to the box: an end point lies on its face
 *                  exactly and never outside.  status = the face.  The chord fraction is exact when the tangent's
 *                  normal component is constant over the step; on a general field the snap leaves O(kappa ds^2) in
 *                  the end point, kappa the line's curvature: end points are not fourth order in general.
 *   other ends     |B| not > 0 at any stage (zero or NaN): NDSM_HIP_TRACE_NULL, the line stops at the last
 *                  accepted point.  max_steps accepted steps: NDSM_HIP_TRACE_UNFINISHED.  A seed outside the box
 *                  (or not finite): NDSM_HIP_TRACE_OUTSIDE, end = seed, length = integral = 0, nsteps = 0.
 *   nsteps         the RK4 steps that moved the line: accepted steps plus the shortened exit step.
 * Each line depends on its own seed only: the same bits whatever the number of seeds, their order, or the direction
 * argument.  A seed on a face whose B points out of the box ends at once (one step of length 0, that face).
 * Returns 0, or >= 9001 errors: 9001 without a GPU whatever the arguments; 9002 a NULL handle or, with nseeds > 0,
 * a NULL B, seeds or output array; 9004 step <= 0 or not finite, max_steps < 1, a direction other than -1, 0, +1,
 * nseeds < 0.  nseeds == 0 succeeds and touches nothing.  On failure the host entry clears the nl entries of its
 * outputs (status 0 is no status); the device entry cannot clear device arrays without a device and leaves them.
 * Device memory: the host entry stages B and G in the handle's scratch (24 B/pt each). */
#define NDSM_HIP_TRACE_XLO 1        /* left through the face x = lo_x */
#define NDSM_HIP_TRACE_XHI 2
#define NDSM_HIP_TRACE_YLO 3
#define NDSM_HIP_TRACE_YHI 4
#define NDSM_HIP_TRACE_ZLO 5
#define NDSM_HIP_TRACE_ZHI 6
#define NDSM_HIP_TRACE_NULL 7       /* |B| not > 0 at a stage */
#define NDSM_HIP_TRACE_UNFINISHED 8 /* max_steps steps taken */
#define NDSM_HIP_TRACE_OUTSIDE 9    /* the seed is not in the box */
/* HOST arrays */
int ndsm_hip_vecpot_trace(void *h, const double *B, const double *G, int nseeds, const double *seeds, double step,
                          int max_steps, int direction, double *ends, double *length, double *integral,
                          int32_t *status, int32_t *nsteps);
/* the same on DEVICE arrays of the library's GPU (seeds and the five outputs too) */
int ndsm_hip_vecpot_trace_device(void *h, const double *dB, const double *dG, int nseeds, const double *dseeds,
                                 double step, int max_steps, int direction, double *dends, double *dlength,
                                 double *dintegral, int32_t *dstatus, int32_t *dnsteps);

/* ---- Nonlinear force-free field: the Grad-Rubin iteration on the same handle (DESIGN.md "Nonlinear force-free
 * field") ------------------------------------------------------------------------------------------------------------
 * A vector magnetogram gives B.n on the faces and, on the lower face, alpha0 = (curl B)_z / B_z.  The field that uses
 * both is the nonlinear force-free field, curl B = alpha B with B.grad alpha = 0 (Grad & Rubin 1958; Amari et al.
 * 1999, 2006; Wheatland 2006).  One pass k of the iteration:
 *   1. alpha^k: alpha0 carried from the lower face along the field lines of B^k to every node (the alpha map);
 *   2. J = alpha^k B^k;
 *   3. laplace(A_c) = -J_c, c = x, y, z, with the potential field's gauge, boundary letters and tangential data,
 *      warm-started from A^k, and B^{k+1} = curl A^{k+1} + the flux-balance fields.
 * Uniform spacing, the handle's mesh (lo_d, h_d, hi_d as for ndsm_hip_vecpot_trace).  Three pairs of entries:
 *
 * The alpha map (step 1 alone; no solve, no hierarchy: the handle supplies the mesh only)
 *   B         (nx,ny,nz,3)
 *   alpha0    (nx,ny), x fastest: the function on the face z = lo_z
 *   polarity  +1: the line of each node is followed against B (alpha0 is taken where B_z > 0 brings the current in);
 *             -1: along B.  Either way the line runs back to where its current entered the box.
 *   step, max_steps   as ndsm_hip_vecpot_trace
 *   out       alpha (nx,ny,nz) doubles; status (nx,ny,nz) int32, may be NULL
 *   One line per node, x fastest; there is no seed array: the seed of node (i,j,k) is r_d = lo_d + (double) i_d h_d,
 *   on the last node hi_d's own expression, so every node is inside the box, and the number of nodes is bounded by
 *   the launch (2^37), not by 2^31 - 1 lines.  The line, its end point and its status are bit for bit those of
 *   ndsm_hip_vecpot_trace from that seed with direction = -polarity (G = NULL).  Then
 *     status == NDSM_HIP_TRACE_ZLO   alpha = the bilinear interpolant of alpha0 at the end point's (x, y): the cell
 *                                    c_d = clamp(floor(u_d), 0, n_d - 2), the unclamped f_d = u_d - c_d, and
 *                                    c0 = v00 + f_x (v10 - v00), c1 = v01 + f_x (v11 - v01), alpha = c0 + f_y (c1 - c0)
 *     any other status               alpha = +0.0: a line that leaves through a side face or the top, ends at a null
 *                                    or does not finish within max_steps carries no current.
 *   Each node depends on its own line only.  9004: step <= 0 or not finite, max_steps < 1, polarity not +1 / -1.
 *
 * The solve for a prescribed current (steps 2-3 with the caller's J)
 *   J         (nx,ny,nz,3): the right-hand sides are rhs_c = -J_c
 *   A         in: the initial guess; out: the solution
 *   B         in: the field whose B.n on the six faces is kept (only its faces are read); out: curl A + balance
 *   Options in the usual slots, return value, ioptc[IOPT_IERR], ioptc[get_iopt_fail3d()] bits 0-2 and the refusal of
 *   a grid that cannot fit as ndsm_hip_vecpot_solve_field; J = 0 gives the potential field.
 *
 * The iteration
 *   B         in: supplies B.n on the six faces; out: the last pass's field
 *   alpha0, polarity, step, max_steps   as the alpha map
 *   start     0: B^0 is the potential field of that B.n and A^0 its A (the bits ndsm_hip_vecpot_solve_device gives
 *             from a zero guess); 1: B^0 = B and A^0 = the caller's A
 *   niter_max >= 1 passes at most; tol >= 0: the loop stops after the pass whose hist[k][0] < tol
 *   A         in (start 1): A^0; out: the last pass's A.  alpha, status (may be NULL): the last pass's alpha map
 *   hist      (niter_max rows of 4 doubles, on the HOST in both entries), row k of the passes run:
 *       [0] max over components and points of |B^{k+1} - B^k|
 *       [1] 1/2 sum w |B^{k+1}|^2 (trapezoid weights, as ndsm_hip_vecpot_helicity)
 *       [2] the current-weighted sine: sum w |J x B| / |B| over sum w |J|, J = curl_h B^{k+1} (derivq's differences);
 *           points where |B| is not > 0 are skipped; 0 when the denominator is 0
 *       [3] the number of nodes whose status is NDSM_HIP_TRACE_ZLO
 *       deterministic sums: the same input gives the same bits
 *   niter_out (one int, on the HOST in both entries): the passes run
 *   The face phase (B.n, the fluxes, the six 2-D solves) runs once per call, from the input B, never from an iterate.
 *   A pass is exactly the alpha map of B^k followed by the solve for J = alpha^k B^k (rhs_c = -(alpha B_c): one
 *   rounding and a sign) from the guess A^k with the input's B.n: the same kernels in the same order, the same bits.
 *   Returns 0, 1 when any 2-D or 3-D solve of any pass missed vc_tol, >= 9001 errors.  9004: polarity not +1 / -1,
 *   start not 0 / 1, niter_max < 1, tol < 0 or not finite, step <= 0 or not finite, max_steps < 1.
 *   Device memory besides the hierarchy: A, two fields B (the caller's and the handle's) and alpha, plus 4 B/pt of
 *   status; the host entry stages all of them.  A grid that cannot fit is refused (9001) before any allocation.
 *
 * All six: 9001 without a GPU whatever the arguments, 9002 a NULL handle or required array.  On failure the host
 * entries clear their outputs (with a live handle, whose grid gives their sizes; hist and niter_out always). */
/* HOST arrays */
int ndsm_hip_vecpot_alpha_map(void *h, const double *B, const double *alpha0, int polarity, double step,
                              int max_steps, double *alpha, int32_t *status);
/* the same on DEVICE arrays of the library's GPU */
int ndsm_hip_vecpot_alpha_map_device(void *h, const double *dB, const double *dalpha0, int polarity, double step,
                                     int max_steps, double *dalpha, int32_t *dstatus);
/* HOST arrays */
int ndsm_hip_vecpot_solve_current(void *h, int ioptc[16], double ropt[16], const double *J, double *A, double *B);
/* the same on DEVICE arrays of the library's GPU */
int ndsm_hip_vecpot_solve_current_device(void *h, int ioptc[16], double ropt[16], const double *dJ, double *dA,
                                         double *dB);
/* HOST arrays */
int ndsm_hip_vecpot_nlfff(void *h, int ioptc[16], double ropt[16], double *B, const double *alpha0, int polarity,
                          int start, int niter_max, double tol, double step, int max_steps, double *A, double *alpha,
                          int32_t *status, double *hist, int *niter_out);
/* the same on DEVICE arrays of the library's GPU (hist and niter_out stay on the host) */
int ndsm_hip_vecpot_nlfff_device(void *h, int ioptc[16], double ropt[16], double *dB, const double *dalpha0,
                                 int polarity, int start, int niter_max, double tol, double step, int max_steps,
                                 double *dA, double *dalpha, int32_t *dstatus, double *hist, int *niter_out);

/* ---- Optimization-method force-free field (DESIGN.md "Optimization-method force-free field") ------------------------
 * The other standard extrapolation (Wheatland, Sturrock & Roumeliotis 2000; Wiegelmann 2004), for the data a vector
 * magnetogram gives: all three components of B on the lower face.  The field is relaxed by pseudo-time steps that
 * lower  L = L_f + L_d,  L_f = sum W w |J x B|^2 / |B|^2,  L_d = sum W w (div_h B)^2,  with the six faces held fixed.
 * Everything is node-based on the handle's uniform mesh; differences are derivq's (centred inside, 3-point one-sided on
 * the end planes), J = curl_h B in ndsm_hip_vecpot_solve_field's expressions, W the trapezoid weight of
 * ndsm_hip_vecpot_helicity, w the caller's weight function.
 *   B         (nx,ny,nz,3) in and out.  start 1: in B^0.  start 0: in the magnetogram on the k = 0 plane (all three
 *             components) and B.n on the other five faces; B^0 is the potential field of the input's B.n (the bits
 *             ndsm_hip_vecpot_solve_device gives from a zero guess) with its whole k = 0 plane overwritten by the
 *             input's; the side and top faces keep the potential field's values.  out: the relaxed field; its face
 *             nodes are bit for bit those of B^0.
 *   w         (nx,ny,nz) in, or NULL for 1 everywhere (ndsm_amd.boundary_weight builds the usual cosine profile)
 *   At every node, faces included: D = div_h B, bb = (bx^2 + by^2) + bz^2, Omega = ((J x B) - D B) / bb (0 where bb
 *   is not > 0; such nodes add nothing to L), P = Omega x B, s = Omega.B.  On the interior nodes
 *     F  = curl_h P - Omega x J - grad_h s + Omega D + |Omega|^2 B
 *     F~ = w F - P x grad_h w - s grad_h w
 *   and dB/dt = F~ gives dL/dt = -2 sum |F~|^2 dV <= 0 in the continuum.
 *   One try: T = B + dt F~ inside, T = B on the faces; L of T; L_T < L (strictly; a NaN fails) accepts - T becomes the
 *   field, dt *= 1.01 - and anything else rejects: dt *= 0.5.  The decision is taken on the device, so nothing is read
 *   back between two checks.
 *   niter_max >= 1 tries at most.  dt0 > 0 the first step (a good value: 0.1 min(h)^2).  The loop stops before a try
 *   when dt < dt_min, and at a check - after every `check` tries - when L_prev - L <= tol L_prev, L_prev the L of the
 *   previous check (of the start at the first).
 *   hist      (hist_rows >= 2 rows of 6 doubles, on the HOST in both entries): [tries, L, L_f, L_d, dt, accepted].
 *             Row 0 is the start field, then one row per check, the final state always last; when the rows run out
 *             the last row is overwritten.  Deterministic sums: the same input gives the same bits.
 *   info      (3 ints, on the HOST in both entries): rows written, tries, stop reason (0 niter_max, 1 tol, 2 dt_min)
 *   Returns 0; 1 when a solve of start 0 missed vc_tol (options in the usual slots); >= 9001 errors: 9001 without a
 *   GPU whatever the arguments, 9002 a NULL handle, B, hist or info, 9004 start not 0 / 1, niter_max < 1, check < 1,
 *   hist_rows < 2, tol < 0 or not finite, dt0 <= 0 or not finite, dt_min < 0 or not finite.  A failed call clears
 *   hist and info.
 *   Device memory: a second field, two Omega fields and 32 KiB of state next to the caller's B (the host entry stages
 *   B and w as well), for the length of the call; start 0 also needs the hierarchy.  A grid that cannot fit is
 *   refused (9001) before any allocation.  Not included: a final divergence cleaning (ndsm_hip_vecpot_project). */
/* HOST arrays */
int ndsm_hip_vecpot_optimize(void *h, int ioptc[16], double ropt[16], double *B, const double *w, int start,
                             int niter_max, int check, double tol, double dt0, double dt_min, double *hist,
                             int hist_rows, int *info);
/* the same on DEVICE arrays of the library's GPU (hist and info stay on the host) */
int ndsm_hip_vecpot_optimize_device(void *h, int ioptc[16], double ropt[16], double *dB, const double *dw, int start,
                                    int niter_max, int check, double tol, double dt0, double dt_min, double *hist,
                                    int hist_rows, int *info);

/* ---- Measurement errors and a freed lower face (DESIGN.md "Measurement errors and a freed lower face") --------------
 * ndsm_hip_vecpot_optimize holds the lower face at whatever the caller puts there: the 2004 form of the method.  Since
 * Wiegelmann & Inhester (2010) and Wiegelmann et al. (2012) a measured magnetogram is fitted within its errors instead:
 * the functional gets a surface term on the k = 0 plane and that plane moves with the descent,
 *   L = (L_f + L_d) + nu L_m,   L_m = sum over ALL nodes of the k = 0 plane of
 *                                     W2 ((wm_x dx^2 + wm_y dy^2) + wm_z dz^2),   d = B(k = 0) - Bobs,
 * W2 the trapezoid weight of the plane (no z factor); every node of the plane adds, whatever |B| is.  Everything not
 * said here - the mesh, the differences, W, w, Omega, P, s, F~, the try, the decision, the stop rules, start, info - is
 * exactly as in ndsm_hip_vecpot_optimize above.
 *   Bobs      (nx,ny,3) in: the observation, the layout of ndsm_hip_vecpot_preprocess's B.  Only the target of the fit:
 *             the start field is built from B alone (start 0: the potential field of the input's B.n with the k = 0
 *             plane of the INPUT B put back).  Never written.
 *   wm        (nx,ny,3) in, or NULL for 1 everywhere: the confidence in each component at each pixel
 *             (ndsm_amd.measurement_weight builds the usual one: 1 for the vertical component, |B_t| / max |B_t| for the
 *             transverse ones)
 *   nu        >= 0, the weight of L_m in L
 *   free      1: the nodes of the k = 0 plane with 1 <= i <= nx - 2 and 1 <= j <= ny - 2 move,  T = B + dt H,
 *               H = (F~ + c G) - c (nu (wm (B - Bobs)))   per component,   c = 2 / h_z,
 *             F~ evaluated at the face node with the difference rows as they are there (centred in x and y, 3-point
 *             one-sided in z, for curl_h P, grad_h s and grad_h w alike), G = w (-P_y, P_x, -s) the surface term
 *             w (P x n + s n) of the variation for n = -z (w = 1 without a weight array).  2 / h_z is the node's
 *             surface weight over its volume weight: the face runs in the same pseudo-time as the interior.  H is the
 *             consistent discretisation of the continuum gradient, not the exact gradient of the discrete L (DESIGN.md
 *             gives the measured difference).  The rim of the plane (i = 0, nx - 1 or j = 0, ny - 1) belongs to the side
 *             faces: it and the five other faces are held, bit for bit.
 *             0: the whole plane is held and L_m is only reported; with nu = 0 the call is then
 *             ndsm_hip_vecpot_optimize bit for bit, in B, info and the columns of hist they share.
 *   hist      (hist_rows >= 2 rows of 7 doubles, on the HOST in both entries): [tries, L, L_f, L_d, L_m, dt, accepted];
 *             L is formed as (L_f + L_d) + nu L_m by the thread that decides, so the identity holds exactly.  Rows and
 *             info as in ndsm_hip_vecpot_optimize.  Deterministic sums, no atomics: the same input gives the same bits.
 *   Returns 0; 1 when a solve of start 0 missed vc_tol; >= 9001 errors: 9001 without a GPU whatever the arguments, 9002
 *   a NULL handle, B, Bobs, hist or info, 9004 ndsm_hip_vecpot_optimize's and: free not 0 / 1, nu negative or not
 *   finite.  A failed call clears hist and info, never B.
 *   Device memory: ndsm_hip_vecpot_optimize's (the state is 48 KiB); the host entry stages the two planes as well,
 *   once.  A grid that cannot fit is refused (9001) before any allocation.  Not included: separate weights for L_f
 *   and L_d, freed side and top faces, z-slab worlds, non-uniform spacing.  (The cascade with this term is
 *   ndsm_hip_vecpot_optimize_obs_cascade below.) */
/* HOST arrays */
int ndsm_hip_vecpot_optimize_obs(void *h, int ioptc[16], double ropt[16], double *B, const double *w,
                                 const double *Bobs, const double *wm, double nu, int free, int start, int niter_max,
                                 int check, double tol, double dt0, double dt_min, double *hist, int hist_rows,
                                 int *info);
/* the same on DEVICE arrays of the library's GPU (hist and info stay on the host) */
int ndsm_hip_vecpot_optimize_obs_device(void *h, int ioptc[16], double ropt[16], double *dB, const double *dw,
                                        const double *dBobs, const double *dwm, double nu, int free, int start,
                                        int niter_max, int check, double tol, double dt0, double dt_min, double *hist,
                                        int hist_rows, int *info);

/* ---- Coarse-to-fine cascade of the optimization method (DESIGN.md "Coarse-to-fine cascade") --------------------------
 * The descent of ndsm_hip_vecpot_optimize is a local pseudo-time relaxation: long-wavelength error decays over
 * thousands of tries on a fine grid and within a few hundred cheap ones on a coarse grid.  Production codes
 * (Wiegelmann 2008) therefore solve on a coarser grid first, interpolate to the next finer one and go on there.
 *
 * Resampling between two uniform meshes that span the same box (so no coordinates are needed).  Node arrays
 * (nx,ny,nz,ncomp); no handle.  The operator is separable: one 1-D rule along x, then y, then z, each axis by itself.
 * With ns source and nd destination nodes on an axis, in 64-bit whole numbers:
 *   mode 0, linear interpolation (any ns, nd >= 2): a = i (ns - 1), j = a div (nd - 1), r = a mod (nd - 1).  r = 0:
 *     the value is v[j], copied, and no other node is read.  Otherwise theta = double(r) / double(nd - 1) and the value
 *     is (1.0 - theta) v[j] + theta v[j + 1].
 *   mode 1, hat average (nd <= ns on every axis): node 0 copies v[0], node nd - 1 copies v[ns - 1].  Any other node i
 *     takes the source nodes f, ascending, whose weight q_f = (ns - 1) - |f (nd - 1) - i (ns - 1)| is > 0; its value
 *     is (sum double(q_f) v[f]) / double(sum q_f), the sum formed left to right from its first term, sum q_f a whole
 *     number.  A single such node is copied.  For a 2:1 nested pair this is the 1-2-1 full weighting.
 *   An axis of one node on both sides (a plane, such as ndsm_hip_vecpot_preprocess's magnetogram) is copied.
 * What follows: a face, edge or corner of dst depends on the same face, edge or corner of src only (the interior of src
 * may hold anything); ns = nd gives src bit for bit; a power of two - a weight of 1 - is reproduced exactly; mode 0
 * reproduces a function linear in x, y, z to rounding.  Deterministic: built without contraction, the operand order
 * above is the bits.
 *   Returns 0 or: 9001 without a GPU whatever the arguments; 9002 a NULL array or shape; 9004 ncomp < 1, a mode other
 *   than 0 or 1, an axis with fewer than 2 nodes on either side unless both have 1, nd > ns on an axis in mode 1.  A
 *   failed call leaves dst untouched.  src and dst must not overlap. */
/* HOST arrays */
int ndsm_hip_resample(const int nsrc[3], const int ndst[3], int ncomp, int mode, const double *src, double *dst);
/* the same on DEVICE arrays of the library's GPU */
int ndsm_hip_resample_device(const int nsrc[3], const int ndst[3], int ncomp, int mode, const double *dsrc,
                             double *ddst);

/* The cascade.  handles[0] is the handle of the finest mesh, the one B and w live on; handles[1 .. nlevels - 1] are
 * handles the caller created on coarser meshes of the same box (level l has no more nodes per axis than level l - 1;
 * the first and last coordinates of every axis equal the finest mesh's bit for bit: build each axis as first + k
 * (last - first) / (n - 1) with the end put in, numpy's linspace).  L = nlevels - 1 is the coarsest level.
 *   1. G_l = mode-1 resample of the input B, straight from the finest mesh, for l = 1 .. L; w_l = mode-0 resample of
 *      w when w is given.  G_0 = B, w_0 = w.
 *   2. Level L is ndsm_hip_vecpot_optimize_device on handles[L] with G_L, w_L and the caller's start: start 0 takes
 *      the potential field of G_L's B.n with G_L's k = 0 plane put back (faces depend on faces only, so the caller
 *      may leave the interior of B unset, as in the single-level call), start 1 starts from G_L.
 *   3. For l = L - 1 .. 0: B_l = mode-0 resample of the finished B_{l+1}.  start 0: the k = 0 plane of all three
 *      components is overwritten by G_l's; the side and top faces keep the interpolated values - on the finest level
 *      they are the prolonged boundary of the coarsest mesh's potential field, NOT the finest mesh's own potential
 *      field as in the single-level call.  start 1: all six faces are overwritten by G_l's, so the result's face
 *      nodes are the input's bit for bit.  Then ndsm_hip_vecpot_optimize_device with start 1 on handles[l] with w_l,
 *      niter_max[l], dt0[l], dt_min[l] and the shared check and tol.
 *   4. B is the finest level's result.  With nlevels = 1 the call is ndsm_hip_vecpot_optimize bit for bit, in B, hist
 *      and info.
 *   niter_max, dt0, dt_min   (nlevels each, on the HOST) per level, index 0 the finest
 *   hist      (nlevels, hist_rows, 6) and info (nlevels, 3), on the HOST in both entries, indexed by level; each
 *             level's rows and info are ndsm_hip_vecpot_optimize's; rows past the written ones are untouched.  A
 *             level that stops at dt_min (even before its first try) hands its field on like any other.
 *   Returns 0, or 1 when the coarsest level's potential solve missed vc_tol: the options in ioptc / ropt are that
 *   solve's, and the ngrids slot must be handles[L]'s.  >= 9001 errors, in this order: 9001 without a GPU; 9002 NULL
 *   handles, a NULL handle among them, NULL B, niter_max, dt0, dt_min, hist or info; 9004 nlevels < 1, start not 0 /
 *   1, a niter_max[l] < 1, check < 1, hist_rows < 2, tol, a dt0[l] or a dt_min[l] outside ndsm_hip_vecpot_optimize's
 *   rules, a coarser level with more nodes on an axis than the next finer one, a level whose box differs from the
 *   finest's.  A failed call clears the hist rows it was given and info; it never clears B.
 *   Device memory: every G_l and w_l first (together about 1/7 of a fine field); the levels one after the other, each
 *   level's buffers freed before the next finer level allocates; level 1's start is interpolated into the caller's
 *   device B, beside which the input stands (one field) only until its faces are pasted.  The peak is
 *   ndsm_hip_vecpot_optimize's on the finest level, and a finest grid that cannot fit is refused (9001) before any
 *   allocation.  The host entry stages B and w once; only history rows cross PCIe in between.
 *   Not included: z-slab worlds, a potential solve on every level, non-uniform spacing, a final
 *   ndsm_hip_vecpot_project. */
/* HOST arrays */
int ndsm_hip_vecpot_optimize_cascade(void *const *handles, int nlevels, int ioptc[16], double ropt[16], double *B,
                                     const double *w, int start, const int *niter_max, int check, double tol,
                                     const double *dt0, const double *dt_min, double *hist, int hist_rows, int *info);
/* the same on DEVICE arrays of the library's GPU (the per-level arrays, hist and info stay on the host) */
int ndsm_hip_vecpot_optimize_cascade_device(void *const *handles, int nlevels, int ioptc[16], double ropt[16],
                                            double *dB, const double *dw, int start, const int *niter_max, int check,
                                            double tol, const double *dt0, const double *dt_min, double *hist,
                                            int hist_rows, int *info);

/* ---- Cascade of the measurement fit (DESIGN.md "Cascade of the measurement fit") -------------------------------------
 * ndsm_hip_vecpot_optimize_obs run coarse-to-fine, as production codes do with measured data (Wiegelmann et al. 2012).
 * Two things are added to the cascade above: the observation and its confidence on every level, and a paste that
 * leaves the freed nodes alone.
 *
 * Confidence-weighted restriction.  The hat average is wrong for an observation with a confidence: a coarse pixel that
 * covers one trusted and three untrusted fine pixels must take the trusted value, not the mean.  Node arrays
 * (nx,ny,nz,ncomp) as for ndsm_hip_resample; wsrc has src's shape, wdst has dst's; nd <= ns on every axis.  All values
 * must be FINITE (an infinite value or weight gives NaN where it is a tap).  The taps of an axis are mode 1's: a
 * destination node with one tap - an end node, an axis of one node on both sides, an axis with ns = nd - copies it,
 * with q = 1 and qsum = 1; any other node takes the ascending source nodes f with q_f > 0, qsum = sum q_f.  The rule
 * is NOT normalised axis by axis.  For every destination node and component three sums run over the tensor of taps,
 * nested as ndsm_hip_resample nests its rule - for every z tap, for every y tap, the finished x sum; then the y sum;
 * then the z sum -, each sum left to right from its first term, each level sum double(q_f) (inner value):
 *   num   innermost term wsrc[f] src[f]        den   innermost term wsrc[f]        pln   innermost term src[f]
 * With Q = (double(qsum_x) double(qsum_y)) double(qsum_z):
 *   wdst = den / Q;   dst = num / den where den > 0.0, otherwise dst = pln / Q
 * - a patch without a trusted pixel (and a negative or NaN sum) gets the plain hat average, and wdst whatever den / Q
 * is.  A node with one tap on every axis (a corner; every node where ns = nd on all three axes) copies: dst = src[f]
 * itself, not (wsrc[f] src[f]) / wsrc[f], and wdst = wsrc[f].  What follows: a face, edge or corner of dst and wdst reads the same face, edge or corner of src and wsrc only;
 * ns = nd returns both arrays bit for bit; wsrc times a power of two leaves dst bit for bit and scales wdst exactly;
 * wsrc = 1 everywhere gives wdst = 1 exactly and dst = mode 1's value to a few ulp (one division instead of three).
 *   Returns 0 or: 9001 without a GPU whatever the arguments; 9002 a NULL array or shape; 9004 ncomp < 1, an axis with
 *   fewer than 2 nodes on either side unless both have 1, nd > ns on an axis.  A failed call leaves dst and wdst
 *   untouched.  The four arrays must not overlap. */
/* HOST arrays */
int ndsm_hip_resample_weighted(const int nsrc[3], const int ndst[3], int ncomp, const double *src, const double *wsrc,
                               double *dst, double *wdst);
/* the same on DEVICE arrays of the library's GPU */
int ndsm_hip_resample_weighted_device(const int nsrc[3], const int ndst[3], int ncomp, const double *dsrc,
                                      const double *dwsrc, double *ddst, double *dwdst);

/* The cascade.  Everything not said here is ndsm_hip_vecpot_optimize_cascade's: the handles, the boxes, G_l, w_l, the
 * per-level options, the memory order, the return values, ioptc / ropt.  Each level is ndsm_hip_vecpot_optimize_obs.
 *   Bobs, wm  (nx,ny,3) on the finest mesh, as for ndsm_hip_vecpot_optimize_obs; wm may be NULL.  Never written.
 *   nu        (nlevels, on the HOST in both entries) the weight of L_m per level, index 0 the finest
 *   free      0 or 1, shared by the levels
 *   Level data: with wm, (Bobs_l, wm_l) = the confidence-weighted restriction of (Bobs, wm), shapes (nx,ny,1) ->
 *     (nx_l,ny_l,1), ncomp 3, straight from the finest mesh; without wm, Bobs_l = mode-1 resample of Bobs and wm_l stays
 *     NULL.  The planes are computed with the G_l and lie beside them.
 *   Level L runs with the caller's start on G_L (the start field is built from G_L alone), with Bobs_L, wm_L, nu[L].
 *   A finer level l starts from the mode-0 resample of level l + 1's result.  free 0: the paste of
 *     ndsm_hip_vecpot_optimize_cascade (start 0: the k = 0 plane of G_l, start 1: its six faces).  free 1: the same
 *     paste WITHOUT the nodes of the k = 0 plane with 1 <= i <= nx_l - 2 and 1 <= j <= ny_l - 2 - start 0: the rim of the
 *     k = 0 plane only; start 1: the six faces minus those nodes.  The freed nodes keep the interpolated values: the
 *     level below has already moved them towards the fit, and G_l there would undo that.  Then
 *     ndsm_hip_vecpot_optimize_obs_device with start 1, Bobs_l, wm_l, nu[l].
 *   hist      (nlevels, hist_rows, 7), info (nlevels, 3): each level's are ndsm_hip_vecpot_optimize_obs's.
 *   nlevels = 1 is ndsm_hip_vecpot_optimize_obs bit for bit, in B, hist and info.  free 0 with every nu[l] = 0 is
 *   ndsm_hip_vecpot_optimize_cascade bit for bit in B, info and the columns of hist they share, whatever Bobs and wm
 *   hold.
 *   Errors: the union of the two parents', in ndsm_hip_vecpot_optimize_cascade's order: 9002 also for a NULL Bobs or
 *   nu; 9004 also for free not 0 / 1 or a nu[l] negative or not finite.  A failed call clears hist and info, never B.
 *   Device memory: the peak stays ndsm_hip_vecpot_optimize_obs's on the finest mesh, refused (9001) before any
 *   allocation when it cannot fit.  The host entry stages B, w, Bobs and wm once; only history rows cross PCIe in
 *   between.  Not included: freed side and top faces, a potential solve on every level, z-slab worlds, non-uniform
 *   spacing, a final ndsm_hip_vecpot_project. */
/* HOST arrays */
int ndsm_hip_vecpot_optimize_obs_cascade(void *const *handles, int nlevels, int ioptc[16], double ropt[16], double *B,
                                         const double *w, const double *Bobs, const double *wm, const double *nu,
                                         int free, int start, const int *niter_max, int check, double tol,
                                         const double *dt0, const double *dt_min, double *hist, int hist_rows,
                                         int *info);
/* the same on DEVICE arrays of the library's GPU (nu, the per-level arrays, hist and info stay on the host) */
int ndsm_hip_vecpot_optimize_obs_cascade_device(void *const *handles, int nlevels, int ioptc[16], double ropt[16],
                                                double *dB, const double *dw, const double *dBobs, const double *dwm,
                                                const double *nu, int free, int start, const int *niter_max, int check,
                                                double tol, const double *dt0, const double *dt_min, double *hist,
                                                int hist_rows, int *info);

/* ---- Magnetogram preprocessing (DESIGN.md "Magnetogram preprocessing") ---------------------------------------------
 * What comes before ndsm_hip_vecpot_optimize when the lower-face data are measured (Wiegelmann, Inhester & Sakurai
 * 2006): a photospheric vector magnetogram is not the boundary of a force-free field - its net Maxwell force and
 * torque (Aly's integrals) do not vanish and its transverse components are noisy.  The call moves it, within the
 * measurement error, towards a force-free, torque-free and smooth one by descending
 *   L = mu1 L1 + mu2 L2 + mu3h L3h + mu3z L3z + mu4 L4
 * on the k = 0 face of the handle's mesh: nx x ny nodes, spacings hx, hy, hh = hx hy, W the trapezoid weight of the
 * plane, x_i = (i - (nx-1)/2) hx and y_j = (j - (ny-1)/2) hy (moments about the centre), e = Bz^2 - Bx^2 - By^2,
 * Bo the observation:
 *   S1 = sum W Bx Bz   S2 = sum W By Bz   S3 = sum W e   S4 = sum W x e   S5 = sum W y e
 *   S6 = sum W (y Bx Bz - x By Bz)   S7 = sum W ((Bx-Box)^2 + (By-Boy)^2)   S8 = sum W (Bz-Boz)^2
 *   S9 = hh sum |Lambda|^2, Lambda_c the 5-point Laplacian of B_c on interior nodes, 0 on the edge nodes
 *   S10 = sum W |B|^2   S11 = sum W sqrt(x^2+y^2) |B|^2;   E = S10 and M = S11 of Bo, fixed for the call
 *   L1 = (S1^2+S2^2+S3^2)/E^2   L2 = (S4^2+S5^2+S6^2)/M^2   L3h = S7/E   L3z = S8/E   L4 = hh^2 S9/E
 * L is dimensionless: rescaling B or the mesh leaves it unchanged.  G = dL/dB is the exact discrete gradient at every
 * node, edge nodes included.
 *   B         (nx,ny,3) in: the magnetogram, out: the preprocessed one.  Nothing else of the handle is used or kept.
 *   obs       (nx,ny,3) in, the observation Bo, or NULL: the input B.  (A continued call passes the original.)
 *   mu        5 doubles on the HOST: mu1, mu2, mu3h, mu3z, mu4, each finite and >= 0
 *   One try: T = B - dt (E/hh) G, dt dimensionless; L of T; L_T < L (strictly; a NaN fails) accepts - T becomes the
 *   field, dt *= 1.01 - and anything else rejects: dt *= 0.5.  The decision is taken on the device, so nothing is read
 *   back between two checks.
 *   niter_max >= 1 tries at most.  dt0 > 0 the first step.  The loop stops before a try when dt < dt_min, and at a
 *   check - after every `check` tries - when L_prev - L <= tol L_prev, L_prev the L of the previous check (of the
 *   start at the first).
 *   hist      (hist_rows >= 2 rows of 17 doubles, on the HOST in both entries): [tries, L, L1, L2, L3h, L3z, L4, dt,
 *             accepted, S1, S2, S3, S4, S5, S6, S10, S11].  Row 0 is the start, then one row per check, the final
 *             state always last; when the rows run out the last row is overwritten.  (|S1|+|S2|+|S3|)/S10 and
 *             (|S4|+|S5|+|S6|)/S11 are the usual force and torque balance figures.  Deterministic sums: the same
 *             input gives the same bits.
 *   info      (3 ints, on the HOST in both entries): rows written, tries, stop reason (0 niter_max, 1 tol, 2 dt_min)
 *   Returns 0; >= 9001 errors: 9001 without a GPU whatever the arguments, 9002 a NULL handle, B, mu, hist or info,
 *   9004 a negative or non-finite mu, niter_max < 1, check < 1, hist_rows < 2, tol < 0 or not finite, dt0 <= 0 or not
 *   finite, dt_min < 0 or not finite, an observation whose E or M is not > 0.  A failed call clears hist and info,
 *   never B.
 *   Device memory: a second field, two Lambda fields, the observation and 176 KiB of state next to the caller's B
 *   (the host entry stages B as well), for the length of the call.  Not included: confidence masks, chromospheric
 *   terms, a flux-balance correction, an automatic call from ndsm_hip_vecpot_optimize - the caller puts the result
 *   on the k = 0 plane of the field handed to it. */
/* HOST arrays */
int ndsm_hip_vecpot_preprocess(void *h, double *B, const double *obs, const double mu[5], int niter_max, int check,
                               double tol, double dt0, double dt_min, double *hist, int hist_rows, int *info);
/* the same on DEVICE arrays of the library's GPU (mu, hist and info stay on the host) */
int ndsm_hip_vecpot_preprocess_device(void *h, double *dB, const double *dobs, const double mu[5], int niter_max,
                                      int check, double tol, double dt0, double dt_min, double *hist, int hist_rows,
                                      int *info);

/* ---- Field-line paths: the points of the same lines (DESIGN.md "Field-line paths") ---------------------------------
 * Where a line runs, not only where it ends: every `every`-th point of each traced line, with B, G and the running
 * integral at it - for drawing lines over a Q map, sampling a field along a loop, or following lines started near a
 * null.  Everything not said here is exactly as in ndsm_hip_vecpot_trace above: the lanes (nl = nseeds lines, or
 * 2 nseeds with direction 0, the forward block then the backward block), the cell, the interpolation, the RK4 step,
 * the exit step, the snap, the status codes, max_steps, step, seeds, B and G.
 *   trace outputs  ends, length, integral, status, nsteps are required and are bit for bit what ndsm_hip_vecpot_trace
 *                  returns for the same arguments.
 *   every          >= 1, the stride in steps between stored points.  With n = nsteps[l], line l stores its state after
 *                  0, every, 2 every, ... steps for each multiple < n, and always its final state after n steps - the
 *                  end point: on its face, the last accepted point of a NULL line, or the point after max_steps steps.
 *                  npts(l) = 1 if n = 0, else (n - 1) / every + 2 (integer division); with every = 1 that is n + 1.
 *   offsets, total offsets has nl + 1 int64 entries: the exclusive prefix sums of npts in lane order, offsets[nl] =
 *                  *total.  total is one int64 on the HOST in both entries.  Both are exact and complete whatever
 *                  max_points is.
 *   max_points     >= 0, the capacity of the point arrays in points: points, bpt, gpt are (3,max_points) - x, y, z per
 *                  point, as seeds -, ipt is (max_points).  The lines' points are concatenated in lane order; slot k of
 *                  the concatenation is written if and only if k < max_points: a line cut by the capacity is written up
 *                  to it and nothing at or beyond max_points is touched (call again with *total).  max_points = 0 is
 *                  the counting call: the four point arrays may be NULL and no second pass is launched.  With
 *                  max_points > 0 points is required; bpt, gpt, ipt may each be NULL and are then skipped; gpt and ipt
 *                  are ignored (not written) when G is NULL.
 *   per point      points: r after that many steps - point 0 carries the seed's bits, the last point those of ends.
 *                  bpt: the trilinear B at r, the interpolation's bits - the stage-1 value of the next step; for the
 *                  last point one extra evaluation at the final r, after the snap (on a NULL line it may be zero or
 *                  NaN and is stored as it is).  gpt: the same for G.  ipt: the running integral after that many
 *                  steps, 0 at point 0 and integral[l]'s bits at the last point.
 *   OUTSIDE lines  store one point: the seed's bits as given, NaN included, bpt = gpt = 0 and ipt = 0.  Nothing is
 *                  interpolated at a point that is not in the box.
 * The points are written by a second pass that repeats the trace with the same expressions, at offsets[l] + j for the
 * j-th stored point of line l; a line never writes outside [offsets[l], min(offsets[l + 1], max_points)).  The bits
 * do not depend on the number of seeds, their order, or the launch geometry.
 * Returns 0, or >= 9001 errors as the trace entries, and: 9004 also for every < 1 or max_points < 0; 9002 also for a
 * NULL total, with nseeds > 0 a NULL offsets, and with max_points > 0 a NULL points.  nseeds == 0 succeeds, sets
 * *total = 0 and touches nothing else.  On failure *total = 0, and the host entry also clears the nl entries of the
 * trace outputs, the nl + 1 entries of offsets and exactly max_points slots of each non-NULL point array; the device
 * entry leaves its device arrays.  On success nothing past the written slots is touched by either entry.
 * Device memory: the host entry stages B and G in the handle's scratch (24 B/pt each) and the points it brings home,
 * min(*total, max_points) of them (up to 80 B each). */
/* HOST arrays */
int ndsm_hip_vecpot_paths(void *h, const double *B, const double *G, int nseeds, const double *seeds, double step,
                          int max_steps, int direction, int every, int64_t max_points, double *ends, double *length,
                          double *integral, int32_t *status, int32_t *nsteps, int64_t *offsets, int64_t *total,
                          double *points, double *bpt, double *gpt, double *ipt);
/* the same on DEVICE arrays of the library's GPU (seeds, the five trace outputs, offsets and the four point arrays;
 * total stays on the host) */
int ndsm_hip_vecpot_paths_device(void *h, const double *dB, const double *dG, int nseeds, const double *dseeds,
                                 double step, int max_steps, int direction, int every, int64_t max_points,
                                 double *dends, double *dlength, double *dintegral, int32_t *dstatus,
                                 int32_t *dnsteps, int64_t *doffsets, int64_t *total, double *dpoints, double *dbpt,
                                 double *dgpt, double *dipt);

/* ---- Squashing factor Q and twist number along the same lines (DESIGN.md "Squashing factor and twist") -------------
 * Q of Titov (2007) at each seed - large where the field-line mapping between the two feet of the line is strongly
 * distorted (quasi-separatrix layers) - by the method of Scott, Pontin & Hornig (2017): two deviation vectors U, V
 * are integrated along the line with the gradient of B, so Q at ANY point of the volume comes from the one line
 * through it, no neighbour lines and no offset.  With G = curl B and integrand 1 the two integrals add up to 4 pi T_w,
 * T_w = (1 / 4 pi) int (curl B).B / |B|^2 dl the twist number (Berger & Prior 2006; Liu et al. 2016).
 * Everything not said here is as in the trace entries above: lo, h, hi, the clamped cell with unclamped fractions,
 * the order of the interpolation, ds = step * min(h), the status codes NDSM_HIP_TRACE_*, max_steps (clamped to 2^24;
 * every line ends after at most max_steps steps), a seed outside or not finite (NDSM_HIP_TRACE_OUTSIDE), fp64 + - * /
 * and sqrt only, in the operand order written here, no contraction.  Always both directions (Q needs both feet):
 * line i (forward) and line nseeds + i (backward) belong to seed i.
 *   B, G       (nx,ny,nz,3); G may be NULL (every integral is 0)
 *   integrand  0: dI/ds = G.B/|B| (as trace); 1: dI/ds = G.B/|B|^2 = ((Gx ex + Gy ey) + Gz ez) / |B|.
 *              G == B (the same pointer) with integrand 1 asks for the twist map: G is then curl_h B, formed on the
 *              device in the handle's scratch (24 B/pt) by the differences of the library's other curls (centred,
 *              3-point one-sided on the end planes; n_d >= 3), J and B interpolated separately - exact for a linear
 *              field.  (G = B itself would integrate 1: the length.)
 *   out        q (nseeds); ends (3,2 nseeds), length, integral (2 nseeds) doubles; status, nsteps (2 nseeds) int32
 * Semantics:
 *   gradient   M_cd = dB_c/dx_d is the exact derivative of the trilinear interpolant in the clamped cell of the stage
 *              point, from the same 8 corners per component v0 .. v7 (x fastest): with d00 = v1 - v0, d10 = v3 - v2,
 *              d01 = v5 - v4, d11 = v7 - v6, c00 = v0 + fx d00, c10 = v2 + fx d10, c01 = v4 + fx d01,
 *              c11 = v6 + fx d11, e0 = c10 - c00, e1 = c11 - c01, c0 = c00 + fy e0, c1 = c01 + fy e1, dz = c1 - c0
 *              (the value is c0 + fz dz, the bits of the trace entries' interpolation):
 *              d/dx = (dx0 + fz (dx1 - dx0)) / h_x with dx0 = d00 + fy (d10 - d00), dx1 = d01 + fy (d11 - d01);
 *              d/dy = (e0 + fz (e1 - e0)) / h_y;  d/dz = dz / h_z.  A field linear in x, y, z gets its exact gradient.
 *   ODE        per direction sgn = +1 / -1, state (r, U, V, I), m = |B(r)|: dr/ds = sgn B/m,
 *              dU_c/ds = sgn (((M_c0 U_0 + M_c1 U_1) + M_c2 U_2) / m), V likewise, dI/ds = the integrand (no sgn, as
 *              trace).  Classical RK4 with trace's weights for all ten components, the sum ((k1 + 2 k2) + 2 k3) + k4
 *              formed in this order; U and V of a stage are advanced with that stage's own M and m.
 *   start      e = B/m at the seed; a = the unit vector of the axis of the smallest |e_d| (x before y before z on a
 *              tie); w = a - (a.e) e, U0 = w / sqrt((w_x w_x + w_y w_y) + w_z w_z), V0 = e x U0 =
 *              (e_y U0_z - e_z U0_y, e_z U0_x - e_x U0_z, e_x U0_y - e_y U0_x).  Both directions start from the same
 *              U0, V0.  A seed where |B| is not > 0 is NDSM_HIP_TRACE_NULL in both directions.
 *   exit       as trace: the step whose end r' is outside is not accepted, the face and the chord fraction t are
 *              found the same way and the step is REDONE from r with s = t ds (stage 1 reused).  Then two
 *              refinements, always two: s <- s (face - r_ax) / (r'_ax - r_ax) with the r' of the redone step, and the
 *              step is redone again with the new s; a refinement is skipped when r'_ax == r_ax (a seed on a face
 *              whose line leaves at once has s = 0: its end is the seed, U, V are U0, V0, nsteps = 1).  Then the
 *              normal coordinate is set to the face's value and the other two are clamped, as trace; length += the
 *              last s.  Without the refinements the end misses the face by O(kappa ds^2) and Q of lines that end on a
 *              side face converges at between first and second order only.  THE END POINTS THEREFORE DIFFER FROM
 *              THOSE OF THE TRACE ENTRIES in the last digits of O(kappa ds^2), as do length and integral of the
 *              exit step.
 *   Q          at each end, on its face (axis ax), with B_e the interpolated B at the end point:
 *              Ut = U - (U_ax / B_e,ax) B_e, Vt likewise, b_n = |B_e,ax|.  With F, B the forward and backward ends and
 *              |B_s|^2 = (Bx Bx + By By) + Bz Bz of the interpolated field at the seed,
 *              Q = (((Ut_F.Ut_F)(Vt_B.Vt_B) + (Ut_B.Ut_B)(Vt_F.Vt_F)) - 2 ((Ut_F.Vt_F)(Ut_B.Vt_B))) * b_n,F * b_n,B
 *                  / |B_s|^2, every dot product as (x x + y y) + z z.
 *              Not clamped to >= 2: a caller sees the integration error instead of a floor.  Q = NaN unless both
 *              directions ended on a face, and when b_n is not > 0 at an end.  Q depends on the faces' geometry: a
 *              uniform field gives 2 between opposite faces and |B|^2 / |B_a B_c| between faces normal to different
 *              axes a and c.
 * Each seed depends on itself only: the same bits whatever the number of seeds or their order.
 * Returns 0, or >= 9001 errors: 9001 without a GPU whatever the arguments; 9002 a NULL handle or, with nseeds > 0,
 * a NULL B, seeds or output array; 9004 step <= 0 or not finite, max_steps < 1, an integrand other than 0, 1,
 * nseeds < 0.  nseeds == 0 succeeds and touches nothing.  On failure the host entry clears the nseeds entries of q
 * and the 2 nseeds entries of its other outputs; the device entry leaves its device arrays.
 * Device memory: the host entry stages B and G in the handle's scratch (24 B/pt each). */
/* HOST arrays */
int ndsm_hip_vecpot_squash(void *h, const double *B, const double *G, int integrand, int nseeds, const double *seeds,
                           double step, int max_steps, double *q, double *ends, double *length, double *integral,
                           int32_t *status, int32_t *nsteps);
/* the same on DEVICE arrays of the library's GPU (seeds and the six outputs too) */
int ndsm_hip_vecpot_squash_device(void *h, const double *dB, const double *dG, int integrand, int nseeds,
                                  const double *dseeds, double step, int max_steps, double *dq, double *dends,
                                  double *dlength, double *dintegral, int32_t *dstatus, int32_t *dnsteps);

/* ---- Perpendicular squashing factor on the same handle (DESIGN.md "Perpendicular squashing factor") ------------------
 * Q-perp of Titov (2007) next to Q: the squashing factor of the mapping between the planes PERPENDICULAR TO THE FIELD
 * at the two feet of the line, which does not depend on the faces the line happens to end on (a uniform field gives 2
 * for every pair of faces).  It is the quantity to look at in a cut through the volume, where the lines of one
 * structure leave through the top and through side faces.  Everything is as in the squash entries above - arguments,
 * lines, ODE, start, exit, integrals, G == B for the twist map, status codes, independence of the seeds -, and q,
 * ends, length, integral, status and nsteps of this entry are the bits of ndsm_hip_vecpot_squash on the same
 * arguments.  Only the projection at the two ends and the normalisation differ:
 *   out        qperp (nseeds) doubles, after q
 *   Q-perp     at each end, from the same U, V and the same B_e (the interpolated B at the end point) as Q:
 *              me = sqrt((Bx Bx + By By) + Bz Bz) of B_e, e = B_e / me (three divisions);
 *              du = (U_x e_x + U_y e_y) + U_z e_z, dv likewise with V;  Up = U - du e, Vp = V - dv e;
 *              puu = Up.Up, pvv = Vp.Vp, puv = Up.Vp, every dot product as (x x + y y) + z z.
 *              With F, B the forward and backward ends and |B_s|^2 of the seed as for Q,
 *              Q-perp = (((puu_F pvv_B + puu_B pvv_F) - 2 (puv_F puv_B)) * me_F) * me_B / |B_s|^2.
 *              Not clamped to >= 2, as Q is not.  Q-perp = NaN unless both directions ended on a face and me > 0 at
 *              both ends.  It does NOT need b_n > 0: a line that arrives tangent to its face has a Q-perp but no Q.
 * Returns and failures as the squash entries (9002 also for a NULL qperp with nseeds > 0); on failure the host entry
 * clears the nseeds entries of q and of qperp and the 2 nseeds entries of its other outputs.  nseeds == 0 succeeds and
 * touches nothing.  Device memory as the squash entries. */
/* HOST arrays */
int ndsm_hip_vecpot_squash_perp(void *h, const double *B, const double *G, int integrand, int nseeds,
                                const double *seeds, double step, int max_steps, double *q, double *qperp,
                                double *ends, double *length, double *integral, int32_t *status, int32_t *nsteps);
/* the same on DEVICE arrays of the library's GPU (seeds and the seven outputs too) */
int ndsm_hip_vecpot_squash_perp_device(void *h, const double *dB, const double *dG, int integrand, int nseeds,
                                       const double *dseeds, double step, int max_steps, double *dq, double *dqperp,
                                       double *dends, double *dlength, double *dintegral, int32_t *dstatus,
                                       int32_t *dnsteps);

/* ---- Null points of a field on the same handle (DESIGN.md "Null points") ---------------------------------------------
 * Where B = 0 and of what type: the other half of a field's skeleton next to the squashing factor (the trace and
 * squash entries end a line with NDSM_HIP_TRACE_NULL when it runs into one).  The field is the trilinear interpolant
 * of the trace entries in each of the (nx-1)(ny-1)(nz-1) cells - the same corners v0 .. v7 per component (x fastest),
 * the same operand order: along x, c00 = v0 + fx (v1 - v0) ..., then y, then z - and its gradient is the squash
 * entries' M.  lo, h as there.  A cell is named by the linear index of its low corner, cell = i + nx (j + ny k);
 * f = (fx, fy, fz) are the fractions within it.  fp64 + - * / and sqrt only, in the operand order written here, no
 * contraction: a restatement in the same order gives the same bits.
 *   B          (nx,ny,nz,3)
 *   max_nulls  >= 0: the capacity of the record arrays; 0 counts only (no record array is looked at)
 *   counts     int64[2], a HOST array in both entries: [0] the candidates of the screen, [1] the nulls found
 *   out        records: cell (int64), pos (3 each), jac (9 each), det, resid doubles; sign, iters int32
 * Semantics:
 *   screen     a cell is a CANDIDATE unless some component's eight corner values are all > 0 or all < 0 (strict
 *              comparisons: a zero corner never excludes a cell).  A cell with a NaN among its 24 corner values is not
 *              a candidate.  The interpolant lies between its corner extremes, so the screen loses no null.
 *   Newton     per candidate, in the fractions f.  NINE STARTS in this order, until one is accepted: (1/2, 1/2, 1/2),
 *              then (1/4 or 3/4)^3 with x fastest and z slowest: start s = 1 .. 8 has fx = 3/4 if (s - 1) & 1 else 1/4,
 *              fy by (s - 1) & 2, fz by (s - 1) & 4.  Per start AT MOST 20 ITERATIONS.  Each: b_a = B_a(f) and
 *              J_ab = dB_a/df_b are the value and gradient expressions of the squash entries WITHOUT the quotients by h:
 *              J_a0 = dx0 + fz (dx1 - dx0), J_a1 = e0 + fz (e1 - e0), J_a2 = dz.  The adjugate:
 *                A00 = J11 J22 - J12 J21   A01 = J02 J21 - J01 J22   A02 = J01 J12 - J02 J11
 *                A10 = J12 J20 - J10 J22   A11 = J00 J22 - J02 J20   A12 = J02 J10 - J00 J12
 *                A20 = J10 J21 - J11 J20   A21 = J01 J20 - J00 J21   A22 = J00 J11 - J01 J10
 *              det = (J00 A00 + J01 A10) + J02 A20 (cofactor expansion along the first row).  Not |det| > 0 (zero or
 *              NaN): the start fails.  delta_d = ((A_d0 b_0 + A_d1 b_1) + A_d2 b_2) / det - three quotients, no
 *              reciprocal - and f_d <- f_d - delta_d.  Not |f_d - 1/2| <= 2.5 on some axis (wandered off, NaN, Inf):
 *              the start fails.  max_d |delta_d| <= 2^-40: the start has CONVERGED (tested after the update, so a start
 *              that begins on the null uses one iteration).  A converged start is ACCEPTED when
 *              -2^-30 <= f_d <= 1 + 2^-30 on all three axes; one converged outside fails, and the next start is tried.
 *              At most one null per cell: the first accepted start.
 *   record     of an accepted cell (c_x, c_y, c_z its low corner's indices):
 *              pos_d = lo_d + (c_d + f_d) h_d, the sum formed first; jac = M_ab = dB_a/dx_b at f, row-major
 *              (a slowest), the bits of the squash entries' gradient, quotients by h included; det = det M by the same
 *              expansion; resid = sqrt((b_0 b_0 + b_1 b_1) + b_2 b_2) at the final f;
 *              sign = +1 for det M < 0 (a positive null: two eigenvalues with positive real part, the fan
 *              diverges), -1 for det M > 0, 0 otherwise; iters = 32 * (number of the start, 0 .. 8) + the iterations
 *              it used (1 .. 20).
 *   order      records come out in ascending cell, whatever the launch geometry, with the same bits on every run and
 *              from both entries.  counts[1] > max_nulls: the first max_nulls records in cell order are written and
 *              the call still returns 0 (call again with that capacity).  No result depends on the capacity of an
 *              internal buffer: both lists are sized from exact counts.  A null on a face, edge or node shared by
 *              cells is reported by each adjacent cell that accepts it - up to 2, 4 or 8 records; merging them is the
 *              caller's business (ndsm_amd.VecPot.nulls does).
 * The constants 20, 2.5, 2^-40 and 2^-30 are choices (DESIGN.md says why), not measurements.  A null of the
 * interpolant where det J = 0 (a degenerate null, or an all-zero cell) is not found: every start stops at the singular
 * guard.
 * Returns 0, or >= 9001 errors: 9001 without a GPU whatever the arguments; 9002 a NULL handle, B or counts, or with
 * max_nulls > 0 a NULL record array; 9004 max_nulls < 0.  On every failure counts is cleared; the host entry also clears
 * the max_nulls slots of every record array (on success the slots past min(counts[1], max_nulls) are zero), the
 * device entry leaves its device arrays (on success it writes the first min(counts[1], max_nulls) slots only).
 * Device memory: the host entry stages B in the handle's scratch (24 B/pt); the screen keeps 1 B + 1 bit per point,
 * the lists 8 B per candidate. */
/* HOST arrays */
int ndsm_hip_vecpot_nulls(void *h, const double *B, int max_nulls, int64_t *counts, int64_t *cell, double *pos,
                          double *jac, double *det, double *resid, int32_t *sign, int32_t *iters);
/* the same on DEVICE arrays of the library's GPU (B and the seven record arrays; counts stays on the host) */
int ndsm_hip_vecpot_nulls_device(void *h, const double *dB, int max_nulls, int64_t *counts, int64_t *dcell,
                                 double *dpos, double *djac, double *ddet, double *dresid, int32_t *dsign,
                                 int32_t *diters);

/* ---- Spine-fan skeleton of the nulls and null-to-null connections (DESIGN.md "Spine-fan skeleton") -------------------
 * From the records of the nulls entries to the skeleton they anchor: the type of each null from its Jacobian, its two
 * spine lines and a ring of fan lines, each traced AWAY from its null, and ended where it comes within a capture
 * radius of ANOTHER null - dr/ds = B/|B| has no rest point, so a fan line that runs into a null (the lines that
 * bracket a separator) would otherwise jitter round it for max_steps steps or drift off along its spine.  The handle
 * supplies the mesh only; no solve runs.  Everything not said here is as in the trace and paths entries above: lo, h,
 * hi, the clamped cell with unclamped fractions, the order of the interpolation, RK4 with ds = step * min(h), the exit
 * step, the snap, the status codes 1 - 9, max_steps (clamped to 2^24), fp64 + - * / and sqrt only, in the operand
 * order written here, no contraction: a restatement in the same order gives the same bits (tests/skeleton_model.py).
 *   B          (nx,ny,nz,3)
 *   pos, jac   nnulls records in the layout of the nulls entries: pos 3 each, jac 9 each, row-major (M_ab = dB_a/dx_b,
 *              a slowest).  The device arrays that ndsm_hip_vecpot_nulls_device wrote can be passed straight in.
 *              Merging duplicate records stays the caller's business.
 *   ring       (2,nring): the coefficients (c_j, s_j) of ring seed j - the caller's cos and sin of its angle; nothing
 *              is normalised here.  nring = 0: the spines alone (ring may be NULL).
 *   radius     > 0, finite: the distance of the seeds from their null, rho = radius * min(h).
 *   capture    >= 0, finite: the capture radius in units of min(h); 0 switches the capture test off.
 *   every, max_points, offsets, total, points, bpt: exactly as in ndsm_hip_vecpot_paths (there is no G).
 * Stage 1, the type of null m from M = jac (one lane per null):
 *   1. det M = (M00 A00 + M01 A10) + M02 A20 with A00 = M11 M22 - M12 M21, A10 = M12 M20 - M10 M22, A20 = M10 M21 -
 *      M11 M20 (the nulls entries' expansion).  s = +1 for det M > 0, -1 for det M < 0; otherwise (0 or NaN) the null
 *      has NO TYPE: kind = 0.
 *   2. N = s M (every entry times s).  The monic characteristic cubic of N is mu^3 - a mu^2 + b mu - c with
 *      a = (N00 + N11) + N22, b = ((N00 N11 - N01 N10) + (N00 N22 - N02 N20)) + (N11 N22 - N12 N21), c = det N by the
 *      expansion of 1 (c > 0).
 *   3. The lone eigenvalue mu - the only one with the sign of the determinant - is the largest real root of the cubic.
 *      Newton from mu = sqrt of the sum of the nine N_ab^2, added one by one in row-major order (the Frobenius norm: no
 *      eigenvalue exceeds it, and to the right of its largest root the cubic is convex and increasing, so the descent
 *      is monotone).  Per iteration, in Horner form: p = ((mu - a) mu + b) mu - c, p' = (3 mu - 2 a) mu + b,
 *      delta = p / p', mu <- mu - delta; |delta| <= 2^-40 |mu| (the new mu): converged.  AT MOST 40 ITERATIONS; not
 *      converged by then, or not mu > 0: kind = 0.
 *   4. t = a - mu, the sum of the other two eigenvalues.  Not t < 0 (they do not lie on the other side: a source or
 *      sink of data that is not solenoidal): kind = 0.
 *   5. C = adj(N - mu I): with J = N, J_dd = N_dd - mu, the nine expressions A00 .. A22 of the nulls entries above.  C has
 *      rank one: its columns are multiples of the spine vector v, its rows of the fan normal w.  Column j is (A0j, A1j,
 *      A2j), row i is (Ai0, Ai1, Ai2); the sum of squares of each is (x x + y y) + z z.  v is the column with the
 *      largest sum of squares - the lowest index on a tie -, each component divided by the sqrt of that sum, then
 *      negated as a whole if its component of largest modulus (the lowest index on a tie) is < 0.  w the same way from
 *      the rows.  A largest sum of squares that is not > 0: kind = 0.
 *   6. The fan basis, by the squash entries' start rule with w in place of e: j the axis of the smallest |w_d| (x
 *      before y before z on a tie), u_d = (1 if d = j else 0) - w_j w_d, e1 = u / sqrt((u0 u0 + u1 u1) + u2 u2),
 *      e2 = w x e1 = (w1 e1_2 - w2 e1_1, w2 e1_0 - w0 e1_2, w0 e1_1 - w1 e1_0).
 *   7. Out: kind = -s, so that +1 is the nulls entries' positive null (sign +1: the fan diverges), doubled to +-2
 *      for a spiral, t t - 4 (c / mu) < 0; eig = (s mu, s t, c / mu): the spine eigenvalue of M, then the sum and the
 *      product of its two fan eigenvalues; spine = v, normal = w.  With kind = 0 the three are zeros.
 * Stage 2, the lines: L = 2 + nring lanes per null, lane l = m L + q, nl = nnulls L lines.
 *   seeds      q = 0: pos_d + rho v_d; q = 1: pos_d - rho v_d; q = 2 + j: pos_d + rho (c_j e1_d + s_j e2_d).
 *   direction  every lane runs away from its null: the spine lanes trace with sgn = s, the fan lanes with sgn = -s
 *              (sgn as the direction of the trace entries: +1 along B).
 *   the line   exactly the line of ndsm_hip_vecpot_paths (without G) for that seed and direction: ends, length,
 *              status, nsteps, npts(l), offsets, *total, the stride every, the capacity max_points, the counting call
 *              with max_points = 0, points and the optional bpt are as there.  A seed outside the box (or not finite)
 *              is NDSM_HIP_TRACE_OUTSIDE.
 *   capture    with (capture min(h))^2 > 0, after every accepted FULL step - not at the seed, not after the exit step -
 *              with r the new point: for m' = 0 .. nnulls - 1 in ascending order, m' = m skipped, dx = r_0 - pos(m')_0,
 *              dy, dz likewise, ((dx dx + dy dy) + dz dz) <= (capture min(h))^2 (the product capture min(h) formed
 *              first, then squared).  The first m' that passes ends the line at r with status NDSM_HIP_SKEL_CAPTURED and
 *              hit[l] = m'; that step counts in nsteps and length.  Otherwise hit[l] = -1.
 *   no type    a null with kind = 0 gives L lines with status NDSM_HIP_SKEL_NONE: one point each with pos's bits as
 *              given (ends too), length 0, nsteps 0, hit -1, bpt 0; nothing is interpolated.
 * With capture = 0 every line's outputs and points are bit for bit those of ndsm_hip_vecpot_paths for that line's seed
 * and direction; a captured line is bit for bit the first nsteps[l] steps of that line.  The bits do not depend on the
 * number of nulls, their order (but hit names the FIRST null within reach), or the launch geometry.
 * The constants 40 and 2^-40 are choices (DESIGN.md says why), not measurements.
 * Returns 0, or >= 9001 errors: 9001 without a GPU whatever the arguments; 9002 a NULL handle or total, or with
 * nnulls > 0 a NULL B, pos, jac, kind, eig, spine, normal, ends, length, status, nsteps, hit or offsets, with nring > 0 a
 * NULL ring, with max_points > 0 a NULL points; 9004 nnulls < 0, nring < 0, every < 1, max_points < 0, a radius that is
 * not > 0 or not finite, a capture that is < 0 or not finite, step not > 0 or not finite, max_steps < 1.  nnulls == 0
 * succeeds, sets *total = 0 and touches nothing else.  On failure *total = 0, and the host entry also clears the nnulls
 * entries of the per-null outputs, the nl entries of the per-line outputs, the nl + 1 entries of offsets and exactly
 * max_points slots of each non-NULL point array; the device entry leaves its device arrays.  On success nothing past
 * the written slots is touched by either entry.
 * Device memory: the host entry stages B in the handle's scratch (24 B/pt) and the points it brings home,
 * min(*total, max_points) of them (up to 48 B each); both entries keep 32 B per line of seeds between the two passes. */
#define NDSM_HIP_SKEL_CAPTURED 10   /* came within the capture radius of another null: hit names it */
#define NDSM_HIP_SKEL_NONE 11       /* the line's null has no type (kind = 0): nothing was traced */
/* HOST arrays */
int ndsm_hip_vecpot_skeleton(void *h, const double *B, int nnulls, const double *pos, const double *jac, int nring,
                             const double *ring, double radius, double capture, double step, int max_steps, int every,
                             int64_t max_points, int32_t *kind, double *eig, double *spine, double *normal,
                             double *ends, double *length, int32_t *status, int32_t *nsteps, int32_t *hit,
                             int64_t *offsets, int64_t *total, double *points, double *bpt);
/* the same on DEVICE arrays of the library's GPU (B, pos, jac, ring and every output array; total stays on the host) */
int ndsm_hip_vecpot_skeleton_device(void *h, const double *dB, int nnulls, const double *dpos, const double *djac,
                                    int nring, const double *dring, double radius, double capture, double step,
                                    int max_steps, int every, int64_t max_points, int32_t *dkind, double *deig,
                                    double *dspine, double *dnormal, double *dends, double *dlength, int32_t *dstatus,
                                    int32_t *dnsteps, int32_t *dhit, int64_t *doffsets, int64_t *total,
                                    double *dpoints, double *dbpt);

/* ---- Separator lines: fan brackets between null pairs, refined on the device (DESIGN.md "Separator lines") -------------
 * The separator of two nulls of opposite sign is the field line in which their fans intersect: it leaves null m in its
 * fan and ends at null m'.  A fan line of m diverges from it like e^(lambda t), so a ring of fan seeds does not hit it;
 * but the fan lines on its two sides pass m' on the two sides of the fan of m' and leave along opposite spines.  A
 * BRACKET is an arc of the fan ring of m, given by two ring coefficient pairs a = (c_a, s_a) and b = (c_b, s_b), and the
 * null m'.  Each bracket is refined by one wave of 64 lanes: 64 directions inside the arc are traced at once, the lowest
 * lane whose line passes m' on another side than lane 0's narrows the arc to 1/63, and this is repeated until the arc is
 * narrower than tol.  The handle supplies the mesh only; no solve runs.  Everything not said here is as in the skeleton
 * and paths entries above; fp64 + - * / and sqrt only, in the operand order written here, no contraction: a
 * restatement in the same order gives the same bits (tests/separator_model.py).
 *   B          (nx,ny,nz,3)
 *   pos, kind, normal   nnulls entries: the pos given to, and the kind and normal written by, the skeleton entries.  The
 *              device arrays of ndsm_hip_vecpot_skeleton_device can be passed straight in.
 *   pair       (2,nbr) int32: the nulls (m, m') of each bracket, each in 0 .. nnulls - 1.
 *   arc        (4,nbr): (c_a, s_a, c_b, s_b) of each bracket - ring coefficients as the skeleton's ring; nothing is
 *              normalised on entry.
 *   radius     > 0, finite: rho = radius * min(h), as the skeleton's.
 *   capture    > 0, finite: the capture radius in units of min(h); it is REQUIRED here ((capture min(h))^2 > 0).
 *   rounds     >= 1: the most rounds a bracket is given.   tol  >= 0, finite: the width at which it has converged.
 *   every, max_points, offsets, total, points, bpt: exactly as in ndsm_hip_vecpot_paths (there is no G).
 * Per bracket (m, m'):
 *   1. Set-up.  w = normal(m); the fan basis e1, e2 from w by item 6 of the skeleton's stage 1, the same expressions
 *      and so the same bits.  rho as above.  The direction of every line is sg = +1 for kind(m) > 0, -1 for kind(m) < 0
 *      (the skeleton's fan lanes).  Unless m != m' and kind(m), kind(m') have strictly opposite signs the state is
 *      NDSM_HIP_SEP_NONE: nothing is traced.
 *   2. A round.  Lane i = 0 .. 63 has t = i / 63, c = (1 - t) c_a + t c_b, s = (1 - t) s_a + t s_b, n = sqrt(c c + s s),
 *      and the direction d_i = (c / n, s / n); a lane whose n is not > 0 traces nothing and has class 0.  Lanes 0 and 63
 *      take a and b unchanged (no division, no test of n).  The seed is pos(m)_d + rho (c e1_d + s e2_d) with the
 *      lane's (c, s).
 *   3. The line of a lane is the skeleton's fan line of that seed and direction with the capture test against m' ALONE.
 *      The closest-approach test runs at the points where the capture test runs - after every accepted FULL step, not at
 *      the seed, not after the exit step -: dx = r_0 - pos(m')_0, dy, dz likewise, d2 = (dx dx + dy dy) + dz dz.  Where
 *      d2 < the smallest d2 of the line so far (strictly; +infinity at first), g = (w'_0 dx + w'_1 dy) + w'_2 dz is
 *      kept, with w' = normal(m'): g belongs to the first point of the smallest d2.  Then d2 <= (capture min(h))^2 ends
 *      the line CAPTURED.
 *   4. The class of a lane: +1 for g >= 0, -1 for g < 0, 0 when the line has no such point (a seed outside the box, an
 *      exit or a null of the interpolant in the first step) or g is NaN.  In the linear regime near m', w' . (r - pos')
 *      keeps its sign along a line, so the class says along which spine of m' the line leaves.
 *   5. Narrowing.  i* is the lowest lane >= 1 whose class differs from lane 0's.  Lane 0 of class 0: state
 *      NDSM_HIP_SEP_GAP.  Else no such lane: NDSM_HIP_SEP_NO_CROSSING.  Else lane i* of class 0: NDSM_HIP_SEP_GAP.
 *      Otherwise a <- d_(i* - 1), b <- d_(i*) (lanes 0 and 63: a and b as they were) and width = sqrt((c_a - c_b)
 *      (c_a - c_b) + (s_a - s_b) (s_a - s_b)); width <= tol: converged; else another round, and when `rounds` are used
 *      up the state is NDSM_HIP_SEP_UNRESOLVED.
 *   6. A converged bracket is NDSM_HIP_SEP_FOUND when the lines of lanes i* - 1 and i* of its last round were both
 *      CAPTURED by m', else NDSM_HIP_SEP_FAR: a change of side that never comes near m' - every ring has one on the side
 *      that faces away from m'.
 * Out, per bracket: state; nrounds, the rounds run (0 for NONE); coef, the final (c_a, s_a, c_b, s_b) (the input arc for
 * NONE, NO_CROSSING and GAP); width, the expression of 5 on coef (0 for NONE); side, the class of lane 0 in the last
 * round (0 for NONE); dmin, the sqrt of the smallest d2 of the lines of lanes i* - 1 and i* of the last round (lanes 0
 * and 63 where there is no i*; +infinity for a line without a point; 0, 0 for NONE).
 * The separator polyline of a bracket is the fan line of its a side: for FOUND, FAR and UNRESOLVED the line of 3 from
 * the seed pos(m)_d + rho (c_a e1_d + s_a e2_d) of the final a, stored as the skeleton stores a line - ends, length,
 * status (1 - 9, NDSM_HIP_SKEL_CAPTURED), nsteps, npts, offsets, *total, points, bpt.  NONE, NO_CROSSING and GAP give
 * one point with pos(m)'s bits, status NDSM_HIP_SKEL_NONE, length 0, nsteps 0, bpt 0.
 * Property: for FOUND, FAR and UNRESOLVED the line equals, bit for bit, fan line 0 (lane 2) of null 0 of
 * ndsm_hip_vecpot_skeleton called with the two nulls (m, m'), the ring (c_a, s_a) taken from coef, and the same radius,
 * capture, step, max_steps and every.  The bits do not depend on the number of brackets or their order.
 * Returns 0, or >= 9001 errors: 9001 without a GPU whatever the arguments; 9002 a NULL handle or total, or with nbr > 0
 * a NULL B, pos, kind, normal, pair, arc, state, nrounds, coef, width, side, dmin, ends, length, status, nsteps or
 * offsets, with max_points > 0 a NULL points; 9004 nnulls < 0, nbr < 0, rounds < 1, a tol that is < 0 or not finite, a
 * capture or a radius that is not > 0 or not finite, every < 1, max_points < 0, step not > 0 or not finite, max_steps
 * < 1, or a pair index outside 0 .. nnulls - 1 (all pairs are checked before anything is written).  nbr == 0 succeeds,
 * sets *total = 0 and touches nothing else.  On failure *total = 0, and the host entry also clears the nbr entries of
 * the per-bracket outputs, the nbr + 1 entries of offsets and exactly max_points slots of each non-NULL point array; the
 * device entry leaves its device arrays.  On success nothing past the written slots is touched by either entry.
 * Device memory: the host entry stages B in the handle's scratch (24 B/pt) and the points it brings home; both entries
 * keep 32 B per bracket between the two passes. */
#define NDSM_HIP_SEP_NONE 0          /* m = m', or kind(m) kind(m') is not < 0: nothing was traced */
#define NDSM_HIP_SEP_FOUND 1         /* converged, both bracketing lines captured by m': the separator */
#define NDSM_HIP_SEP_FAR 2           /* converged on a change of side that does not come near m' */
#define NDSM_HIP_SEP_NO_CROSSING 3   /* every lane passes m' on lane 0's side */
#define NDSM_HIP_SEP_GAP 4           /* lane 0, or the first lane that differs from it, has no side */
#define NDSM_HIP_SEP_UNRESOLVED 5    /* still wider than tol after `rounds` rounds */
/* HOST arrays */
int ndsm_hip_vecpot_separators(void *h, const double *B, int nnulls, const double *pos, const int32_t *kind,
                               const double *normal, int nbr, const int32_t *pair, const double *arc, double radius,
                               double capture, double step, int max_steps, int rounds, double tol, int every,
                               int64_t max_points, int32_t *state, int32_t *nrounds, double *coef, double *width,
                               int32_t *side, double *dmin, double *ends, double *length, int32_t *status,
                               int32_t *nsteps, int64_t *offsets, int64_t *total, double *points, double *bpt);
/* the same on DEVICE arrays of the library's GPU (every array; total stays on the host) */
int ndsm_hip_vecpot_separators_device(void *h, const double *dB, int nnulls, const double *dpos, const int32_t *dkind,
                                      const double *dnormal, int nbr, const int32_t *dpair, const double *darc,
                                      double radius, double capture, double step, int max_steps, int rounds, double tol,
                                      int every, int64_t max_points, int32_t *dstate, int32_t *dnrounds, double *dcoef,
                                      double *dwidth, int32_t *dside, double *ddmin, double *dends, double *dlength,
                                      int32_t *dstatus, int32_t *dnsteps, int64_t *doffsets, int64_t *total,
                                      double *dpoints, double *dbpt);

/* =====================================================================
 * PART 3 - additive exports, multi-GPU
 *
 * One process per GPU.  Level 1 is cut into z-slabs, one per rank; every slab
 * carries `g` ghost planes per side; neighbours exchange 4 planes per two-sweep
 * pass over RCCL (ncclSend / ncclRecv on the library stream); the restricted
 * residual is gathered to rank 0, which runs levels >= 2 and scatters the coarse
 * correction back.  Results are bit-identical to the single-GPU solver (tests:
 * loop-back world on one GPU, 2-rank gloo model on the CPU).
 * ===================================================================== */

/* RCCL bootstrap: rank 0 fills id128 (128 bytes), the caller broadcasts it by its own means
 * (MPI, torch.distributed/gloo, a file), every rank then calls dist_init.  Requires
 * ndsm_hip_init(local device) first. */
int ndsm_hip_dist_unique_id(void *id128);
int ndsm_hip_dist_init(int rank, int nranks, const void *id128);
/* destroys the communicator after draining the library's streams; call on every rank once all
 * worlds are destroyed.  No-op without a communicator. */
int ndsm_hip_dist_finalize(void);
/* Collective transport self-test on the live communicator (meant for the 1-rank bring-up on a one-GPU
 * box, valid at any size): each rank sends nelem doubles to itself and receives them back through the
 * grouped ncclSend / ncclRecv pair a halo exchange uses, once on the main stream and once on the
 * communication stream between two fences (the order an overlapped pass issues them in), then runs the
 * 2-value (max, sum) all-reduce of the convergence metric.  0 = every byte arrived and the reduction is right. */
int ndsm_hip_dist_selftest(int nelem);
/* rank / size as the live RCCL communicator reports them (ncclCommUserRank, ncclCommCount);
 * *nranks = 0 when no communicator is up */
int ndsm_hip_dist_info(int *rank, int *nranks);

/* Slab plan for nranks ranks, 12 ints per rank: rank, z0, z1 (owned fine planes), g (ghost
 * depth), nloc (= z1 - z0 + 2 g), k0 (global index of local plane 0), ck0, ck1 (coarse planes it
 * restricts), pk0, pk1 (coarse planes it needs for prolongation), cb0, cb1 (coarse buffer window).
 * Pure host arithmetic (no GPU needed).  Returns 0, or 9002 when the shape cannot be cut that way. */
int ndsm_hip_slab_plan(const int *nshape, const double *x, const double *y, const double *z, int ngrids,
                       int nranks, int *out /* [nranks][12] */);

/* ndsm_vector_solve on the z-slab decomposition (BASELINE config[4]: 2048 x 2048 x 1024 across the
 * GPUs of a node).  Collective: every rank of the communicator calls it with the GLOBAL nshape4 =
 * [nx,ny,nz,3] and mesh vectors and with ITS planes [z0, z1) of A and B - the split
 * ndsm_hip_slab_plan reports for (nshape, ngrids = ioptc[get_iopt_ngrids()], nranks) - laid out
 * (nx, ny, z1-z0, 3) in Fortran order.  The O(N^(2/3)) face phase (fluxes, six 2-D solves, tangential
 * data) runs on rank 0 exactly as in ndsm_vector_solve, the three 3-D solves on z-slab worlds, flux
 * balance and curl on the slabs.  Options, return value and the contents of A (in: initial guess,
 * out: vector potential) and B (in: boundary normal component, out: curl A + correction) as for
 * ndsm_vector_solve - the same bits on the same input, with ioptc[get_iopt_prec()] != 0 the bits of the
 * single-GPU mixed-precision mode (the 3-D solves then run ndsm_hip_world_set_precision's scheme where
 * the slabs allow it).  nranks == 1 is ndsm_vector_solve.  Reference: none (shared-memory OpenMP only); pipeline of
 * ndsm_vector_potential.f90:130-497. */
int ndsm_hip_world_vector_solve(int rank, int nranks, const int nshape4[4], int ioptc[16], double ropt[16],
                                const double *x, const double *y, const double *z, double *A_slab, double *B_slab);

/* rank >= 0: this process holds slab `rank` (RCCL transport, after ndsm_hip_dist_init);
 * rank <  0: loop-back world - all nranks slabs on this GPU, neighbours reached by device copies
 *            (verification of the slab algebra on one GPU). */
int ndsm_hip_world_create(const int *nshape, const double *x, const double *y, const double *z,
                          const char *bcs, int ngrids, int ms, double ex_tol, int du_max, int nmax_exact,
                          int nranks, int rank, void **handle);
int ndsm_hip_world_destroy(void *handle);
int ndsm_hip_world_nlocal(void *handle);                          /* slabs held by this process */
/* how many levels are distributed (1 = only the finest; more where a rank's share of the next level
 * is still large: its restricted planes then never travel to rank 0; NDSM_HIP_DIST_LEVELS=k forces) */
int ndsm_hip_world_dist_levels(void *handle);
int ndsm_hip_world_slab(void *handle, int ilocal, int *info12);   /* its plan row */
/* which: 0 = u, 1 = rhs, 2 = residual.  host holds nplanes whole x-y planes starting at GLOBAL
 * plane gz0; the planes that fall into slab ilocal's window (ghosts included) are copied. */
int ndsm_hip_world_upload(void *handle, int ilocal, int which, const double *host, int gz0, int nplanes);
int ndsm_hip_world_download(void *handle, int ilocal, int which, double *host /* owned planes */);
/* Mixed precision on the slabs (BASELINE config[4]): as ndsm_hip_mg_set_precision - 0 fp64, != 0 fp64
 * residual + fp32 correction V-cycle on level 1 (halo exchange, restriction and prolongation of the
 * correction in fp32, everything from level 2 down unchanged).  Returns 1 if ndsm_hip_world_solve will
 * run mixed, 0 if the fp64 path stays (a slab out of the fp32 kernels' reach), < 0 bad arguments.
 * Same bits as the single-domain mixed mode. */
int ndsm_hip_world_set_precision(void *world, int mode);
int ndsm_hip_world_zero_rhs(void *handle);                        /* as ndsm_hip_mg_zero_rhs */
int ndsm_hip_world_relax(void *handle, int nsweeps);              /* collective */
int ndsm_hip_world_vcycle(void *handle, int ncycles);             /* collective, asynchronous */
/* collective; every rank returns the same history.  0 converged, 1 not, >= 9001 error */
int ndsm_hip_world_solve(void *handle, double vc_tol, int nmax, double *du_last, int *ncycles, double *hist,
                         int hist_len);

/* "hip=<path>;rccl=<path>": the shared objects this library's HIP / RCCL calls are bound to
 * (a process that also imports PyTorch holds two ROCm stacks) */
int ndsm_hip_bound_libs(char *buf, int len);

/* =====================================================================
 * PART 4 - development hooks (tests and tuning; no reference counterpart)
 * ===================================================================== */

/* Tile configuration of the fused smoother (csrc/smooth_fused.hip), the five values of the
 * NDSM_FUSED_CFG environment variable at run time: alternates for the two-sweep / one-sweep /
 * sweep+residual launches (0 = default), a fixed number of work items (0 = the launch's own choice),
 * and big = -1 by level size / 0 never / 1 always use the tiles of >= 64 M-point levels - so that the
 * parity tests can run the benchmarked 512^3 configurations on grids the oracle handles.
 * Results never depend on these values (bit for bit); only speed does. */
int ndsm_hip_debug_fused_cfg(int two, int one, int res, int work_items, int big);
/* Which launches a relax call makes (what = 0), or the z chunking of a fused launch (what = 1), as the one planner
 * behind every smoother entry decides them ("Which launch a relax call makes").  Host code: works without
 * a device and without ndsm_hip_init.
 * what = 0: grid[15] = ndim, n[3], lb[3], ub[3], all_neumann, k0, nzg, zown0, zown1; req[12] = nsweeps, variant,
 *   window, fp32, rhs, want_res, want_met, corr, coarse_plane, have[1], have[2], keep; knobs[8] = the five values of
 *   NDSM_FUSED_CFG, the two of NDSM_BLOCK_CFG, NDSM_HIP_NO_BLOCK.  out[0..5] = error code, passes, result buffer,
 *   residual covered, metric covered, interpolation only; then nine values per pass: kind, sweeps, mode,
 *   instantiation, block height, src, dst, interpolation first, mean shift.
 * what = 2: what = 0 with the zero-source field (a coarse level's zero first guess that was never written): req[13],
 *   req[12] = the source is zero; out[0..6], out[6] = the zeros have to be written first; ten values per pass, the
 *   tenth = this pass takes its source from a descriptor of zero records.
 * what = 1: req[6] = owned planes, tiles, workgroup slots, pipeline depth, residual pipeline, work-item override;
 *   out[0..1] = chunks, planes per chunk.
 * Returns 9002 for a null array, a value out of range or cap (entries of out) too small for the answer. */
int ndsm_hip_debug_relax_plan(int what, const int32_t *grid, const int64_t *req, const int64_t *knobs, int cap,
                              int32_t *out);
/* 0: the small levels at the bottom of a V-cycle run kernel by kernel even where the single-launch form
 * (csrc/tail.hip: all of them resident in LDS, one workgroup) covers them; 1 = default (environment
 * NDSM_HIP_NO_TAIL switches it off for a whole process).  Same bits either way. */
int ndsm_hip_debug_tail(int on);
/* 0: the descent of a V-cycle writes the zero first guess of every coarse level and the level's pre-smoothing loads
 * it, as before; 1 = default: where the first pre-smoothing launch of the level is an out-of-place fused pass the
 * restriction leaves u alone and that launch takes the zeros from a buffer descriptor of zero records (environment
 * NDSM_HIP_NO_ZERO_GUESS=1 switches it off for a whole process).  Same bits either way.
 * For the tests of this, ndsm_hip_mg_op has two more operations: 11 = u(level) is zero the way the descent leaves
 * it (declared while the feature is on, written otherwise), 12 = the restriction level -> level+1 the way the
 * descent of a V-cycle from level 1 does it. */
int ndsm_hip_debug_zero_guess(int on);
/* 1: u(level) of this ndsm_hip_mg_create handle is at present a zero guess that was declared and not written (any
 * download, upload or single operation that reads it writes the zeros first), 0: it is in memory */
int ndsm_hip_debug_u_declared_zero(void *handle, int level);
/* Which kernel an inter-level transfer takes is decided by the size of the fine level; this sets the sizes and the
 * streamed restriction's launch so that the parity tests can run every form on grids the oracle handles.  A negative
 * value restores the built-in choice of that knob; (-1, -1, -1, -1) restores all four.
 *   restrict_min_points: fine points from which a 3-D level pair is sent to the LDS-streamed restriction
 *     (csrc/restrict_stream.hip) instead of the gather kernel - built in: 6 Mi.  Read when a hierarchy is built: set it
 *     before ndsm_hip_mg_create / ndsm_hip_world_create.  The kernel's tile must still cover the pair's taps.
 *   prolong_min_points: fine points from which u_f += P u_c runs the LDS-tiled kernel - built in: 2 Mi.  Read at every
 *     call; nx >= 64 and at least 16 coarse points per axis are needed as before.
 *   rs_variant: 5, 8 or 10 - the form of the streamed restriction (environment NDSM_RS_VARIANT, which is read once per
 *     process; this overrides it at run time).  The launcher's own demotions stay: 10 -> 8 for odd nx, fp32 fine fields
 *     and planes of 2 GiB or more, -> 5 where the pair's z windows do not fit the schedule.  Another value >= 0: 9002.
 *   rs_chunk: coarse planes per z chunk of the streamed restriction, clamped to [1, min(planes, 64)].
 * Results never depend on these values (bit for bit); only speed does. */
int ndsm_hip_debug_transfer_cfg(long long restrict_min_points, long long prolong_min_points, int rs_variant,
                                int rs_chunk);
/* The kernels the transfers level -> level + 1 (level >= 1) of an ndsm_hip_mg_create handle take, as the launchers
 * themselves decide them: out[0] = 0 the gather restriction / 5, 8, 10 the streamed form after the demotions,
 * out[1], out[2] = coarse planes per chunk and chunks of that launch (0, 0 for the gather kernel), out[3] = 1 the
 * tiled prolongation / 0 the per-point one.  Needs ndsm_hip_init.  9002: no such level pair. */
int ndsm_hip_debug_transfer_form(void *handle, int level, int out[4]);

/* ---- Open-box potential field from a magnetogram (DESIGN.md "Open-box potential field") ------------------------------
 * Every entry that starts from a potential field reads B.n on all six faces of the box; a magnetogram gives the lower
 * face only.  The Green's-function field of the half space above the magnetogram (Schmidt 1964; Sakurai 1982) gives
 * the other five: it is evaluated on the faces, and the interior is solved by ndsm_hip_vecpot_solve.  The magnetogram
 * may be wider than the box - flux outside the box's footprint decides the side faces.  No handle.
 *
 * Source.  bz (nsx,nsy) on the uniform mesh xs (nsx >= 2), ys (nsy >= 2) at height zs.  hx = xs[1] - xs[0] and
 *   hy = ys[1] - ys[0], both > 0; c = (hx hy) / 6.283185307179586; npix = nsx nsy; pixel p = i + nsx j.
 * One target (X, Y, Z), w = Z - zs.  For pixel p: q = bz[p] c; dx = X - xs[i]; dy = Y - ys[j];
 *   r2 = (dx dx + dy dy) + w w; if r2 > 0: t = q / (r2 sqrt(r2)) and the three terms are dx t, dy t, w t; otherwise
 *   the pixel contributes no term (the punctured point rule for a target on a source node).
 * Order of the sum: a function of npix only - not of the targets, the entry or the launch.
 *   NS = min(64, ceil(npix / 4096)), len = ceil(npix / NS); slice s covers the pixels [s len, min(npix, (s + 1) len)).
 *   A slice sum starts at 0.0 and adds its terms left to right; the result is the slice sums added in ascending order,
 *   starting from slice 0's.  Built without contraction, with IEEE division and sqrt: the order above is the bits.
 * Targets on or below the plane.  w < 0: all three components are NaN.  w == 0: Bx and By are the sums; Bz is the
 *   bilinear interpolation of bz at (X, Y), 0 outside xs[0] <= X <= xs[nsx - 1], ys[0] <= Y <= ys[nsy - 1].  Inside,
 *   i0 is the largest node <= nsx - 2 with xs[i0] <= X, theta_x = (X - xs[i0]) / (xs[i0 + 1] - xs[i0]), likewise j0
 *   and theta_y; L(v0, v1, theta) = v0 if theta == 0, v1 if theta == 1, else (1.0 - theta) v0 + theta v1; and
 *   Bz = L(L(bz[i0,j0], bz[i0+1,j0], theta_x), L(bz[i0,j0+1], bz[i0+1,j0+1], theta_x), theta_y): a target that sits
 *   bitwise on a source node gets that pixel's value bit for bit.  Non-finite bz propagates.
 * The rule is first order in h for the tangential field on the plane itself (w == 0) and accurate to the truncation
 * of the magnetogram two or more mesh rows above it.  The punctured rule knows bitwise equality only: a target on the
 * plane that misses a source node by a rounding error gets a term of the order q / eps^2 from it.  Where the box
 * starts on the plane (z[0] == zs), build the box's x and y as slices of xs and ys (or pass the box's own x and y as
 * the source mesh), so that its nodes on the plane are source nodes bit for bit, or keep them well apart.
 *
 * ndsm_hip_green_points: B (3,npts) at pts (3,npts) - x, y, z of each point, as the seeds of ndsm_hip_vecpot_trace.
 * ndsm_hip_green_box: B (nx,ny,nz,3) on the box mesh x, y, z.  which = 0 writes the nodes with an index at either end
 *   of an axis and leaves every interior node of B untouched; which = 1 writes all nodes.  The same node gets the same
 *   bits from both, and from the points entry at its coordinates.
 * ndsm_hip_vecpot_open: ndsm_hip_green_box_device (which = 0) on the handle's mesh into the device B, then
 *   ndsm_hip_vecpot_solve_device, bit for bit that composition: A in the first guess, out A; B out (the host form
 *   starts from a B of zeros; the device form leaves the interior of dB as it is until the solve overwrites it).
 *   No field crosses PCIe in between.  Options and return value as ndsm_hip_vecpot_solve.
 * The mesh vectors xs, ys, x, y, z stay on the HOST in both forms, as for ndsm_hip_vecpot_create.
 *   Returns 0 or: 9001 without a GPU whatever the arguments; 9001 before anything is allocated - as soon as the shapes
 *   can be read, in all three entries - when the arrays and the scratch (at most 384 MiB: the targets go through in
 *   chunks) exceed the device's TOTAL memory.  That is a screen, not a reservation: it does not count what else is
 *   resident (a handle's hierarchies among it), and a call that passes it and finds too little memory free fails in
 *   its allocation, with 9001 as well and the outputs untouched.  9002 a NULL array, shape or handle; 9004 nsx or
 *   nsy < 2, a spacing not > 0, npts < 0, which outside 0/1, a box axis < 2, z[0] < zs.
 *   npts == 0 returns 0 and touches nothing.  A failed call leaves the outputs untouched. */
/* HOST arrays */
int ndsm_hip_green_points(const int nsrc[2], const double *xs, const double *ys, double zs, const double *bz, int npts,
                          const double *pts, double *B);
/* the same with bz, pts and B DEVICE arrays of the library's GPU */
int ndsm_hip_green_points_device(const int nsrc[2], const double *xs, const double *ys, double zs, const double *dbz,
                                 int npts, const double *dpts, double *dB);
/* HOST arrays */
int ndsm_hip_green_box(const int nsrc[2], const double *xs, const double *ys, double zs, const double *bz,
                       const int nshape[3], const double *x, const double *y, const double *z, int which, double *B);
/* the same with bz and B DEVICE arrays of the library's GPU */
int ndsm_hip_green_box_device(const int nsrc[2], const double *xs, const double *ys, double zs, const double *dbz,
                              const int nshape[3], const double *x, const double *y, const double *z, int which,
                              double *dB);
/* HOST arrays */
int ndsm_hip_vecpot_open(void *h, int ioptc[16], double ropt[16], const int nsrc[2], const double *xs,
                         const double *ys, double zs, const double *bz, double *A, double *B);
/* the same with bz, A and B DEVICE arrays of the library's GPU */
int ndsm_hip_vecpot_open_device(void *h, int ioptc[16], double ropt[16], const int nsrc[2], const double *xs,
                                const double *ys, double zs, const double *dbz, double *dA, double *dB);

/* ---- Constant-alpha (linear) force-free field of a magnetogram (DESIGN.md "Linear force-free field") ---------------
 * curl B = alpha B with one alpha for the whole half space above the magnetogram: the middle rung between the
 * potential field above and the nonlinear entries, and the only current-carrying field a line-of-sight magnetogram
 * gives.  B = integral of G bz dA' with the kernel of Chiu & Hilton (1977) for their C = 0 family - with R the
 * horizontal and r the full distance, Gamma = [z cos(alpha r) / r - cos(alpha z)] / (2 pi R),
 * Gx = (x / R) dGamma/dz + alpha Gamma y / R, Gy = (y / R) dGamma/dz - alpha Gamma x / R,
 * Gz = z [cos(alpha r) / r^3 + alpha sin(alpha r) / r^2] / (2 pi) - summed over the pixels as the potential field is:
 * the same all-pairs sum with a richer pair term, written so that nothing divides by R where R = 0.  No handle.
 *
 * Source, pixels, c, slices and fold: exactly those of ndsm_hip_green_points - NS = min(64, ceil(npix / 4096)) slices,
 *   each slice sum starting at 0.0 and adding left to right, the slice sums folded in ascending order.
 * alpha: a finite double of either sign, in 1 / (length unit of the mesh).
 * One target (X, Y, Z), w = Z - zs: ww = w w; sz = sin(alpha w); cz = cos(alpha w).
 * For pixel p: q = bz[p] c; dx = X - xs[i]; dy = Y - ys[j]; R2 = dx dx + dy dy; r2 = R2 + ww.
 *   If r2 > 0: r = sqrt(r2); t = q / (r2 r); ar = alpha r; cr = cos(ar); sr = sin(ar);
 *     Sx = Sx + (dx t) cr;  Sy = Sy + (dy t) cr;  Sz = Sz + (w t) (cr + ar sr);
 *     then, if R2 > 0: u = alpha (q / R2); e = sz - (ww / r2) sr; f = (w / r) cr - cz;
 *       Sx = Sx + u (dx e + dy f);  Sy = Sy + u (dy e - dx f).
 *   Otherwise the pixel contributes no term (the punctured rule of the potential field).
 *   Plain C++ without contraction, IEEE division and sqrt; sin and cos are the device library's double-precision
 *   functions (the pair's two come from one sincos call).  Up to those two functions the order above is the bits.
 * Targets on or below the plane: the rules of ndsm_hip_green_points - w < 0 gives NaN, at w == 0 Bz is the bilinear
 *   interpolation of bz.
 * alpha == 0 with a finite bz gives the bits of the Green's-function entries: cos 0 = 1 and sin 0 = 0 make every added
 *   quantity the old term or a zero of either sign.  For finite bz only: with alpha = 0 a non-finite pixel makes u NaN
 *   (0 times an infinity), where the potential entries give an infinity.
 * A hazard, wider than the punctured rule's.  e and f cancel to O(R^2) as R -> 0 at w > 0, where u is of the order
 *   1 / R^2: a target that misses the vertical through a source node by a rounding error gets a finite result that has
 *   lost digits, about eps z^2 / R^2 relative.  The rule is the punctured rule's, for every height: build the box's x
 *   and y as slices of xs and ys, so that box nodes are source nodes bit for bit, or keep them well away.
 * A limit of the solution.  It is not unique: the C = 0 member is the customary one.  The horizontal field falls only
 *   like 1 / R, so the result depends on the magnetogram's width more than the potential field does; and for
 *   |alpha| L of the order of 2 pi (L the magnetogram's width) the field oscillates with height and is of little use.
 *
 * ndsm_hip_lfff_points: B (3,npts) at pts (3,npts).  ndsm_hip_lfff_box: B (nx,ny,nz,3) on the box mesh x, y, z, which
 *   as for ndsm_hip_green_box.  The same node gets the same bits from the faces, the volume and the points entry.
 *   Returns, chunks, scratch and the memory screen: as the Green's-function entries, in their order - 9001, 9002,
 *   9004; a non-finite alpha is 9004.  npts == 0 returns 0 and touches nothing.  A failed call leaves the outputs
 *   untouched. */
/* HOST arrays */
int ndsm_hip_lfff_points(const int nsrc[2], const double *xs, const double *ys, double zs, const double *bz,
                         double alpha, int npts, const double *pts, double *B);
/* the same with bz, pts and B DEVICE arrays of the library's GPU */
int ndsm_hip_lfff_points_device(const int nsrc[2], const double *xs, const double *ys, double zs, const double *dbz,
                                double alpha, int npts, const double *dpts, double *dB);
/* HOST arrays */
int ndsm_hip_lfff_box(const int nsrc[2], const double *xs, const double *ys, double zs, const double *bz, double alpha,
                      const int nshape[3], const double *x, const double *y, const double *z, int which, double *B);
/* the same with bz and B DEVICE arrays of the library's GPU */
int ndsm_hip_lfff_box_device(const int nsrc[2], const double *xs, const double *ys, double zs, const double *dbz,
                             double alpha, const int nshape[3], const double *x, const double *y, const double *z,
                             int which, double *dB);

/* ---- Magnetic dips and bald patches of a field on the same handle (DESIGN.md "Dips and bald patches") ---------------
 * Where a field line is locally lowest: B_z = 0 with (B.grad)B_z > 0 (Titov, Priest & Demoulin 1993).  On the lower
 * boundary these points are the BALD PATCHES, the stretches of the polarity inversion line where field lines touch the
 * boundary from above - the third kind of separatrix next to the fans of the nulls and the quasi-separatrix layers -;
 * in the volume they are the DIPS that can hold the material of a filament (Aulanier & Demoulin 1998).  They are looked
 * for on the EDGES of the mesh.  fp64 + - * / only, in the operand order written here, no contraction: a restatement
 * in the same order gives the same bits.
 *   B           (nx,ny,nz,3) on the handle's mesh; lo_d, h_d its first point and spacing per axis (h_d = the difference
 *               of the first two mesh points); nodes are numbered node = i + nx (j + ny k)
 *   plane_only  0, or 1: the magnetogram's own question, see below
 *   max_dips    >= 0 (int64): the capacity of the record arrays; 0 counts only (no record array is looked at)
 *   counts      int64[3], a HOST array in both entries: (crossings, dips, bald patches), exact whatever the capacity
 *   out         records: edge (int64), pos, bpt, grad (3 each), curv doubles; flag int32
 * Semantics:
 *   gradient    nodal: G_d = the difference quotient of B_z along axis d at the node, the field entries' ddq with
 *               exactly its operand order: inside, G = (0 + v[-1] (-0.5 / h)) + v[+1] (0.5 / h); on the lower end
 *               plane ((0 + v[0] (-1.5 / h)) + v[+1] (2 / h)) + v[+2] (-0.5 / h); on the upper end plane
 *               ((0 + v[0] (1.5 / h)) + v[-1] (-2 / h)) + v[-2] (0.5 / h): centred inside and 3-point one-sided on
 *               the end planes.
 *   edges       edge e = 3 node + d, d = 0, 1, 2 for x, y, z, runs from node p to its +d neighbour p'.  A node on the
 *               upper end plane of axis d has no edge d.
 *   crossing    with a = B_z(p) and b = B_z(p'): the edge is a CROSSING iff (a > 0) != (b > 0).  A zero or NaN counts
 *               as not positive, so an exact zero at a node is reported by exactly one edge of each family.
 *   at it       t = a / (a - b): one quotient, no reciprocal.  Every nodal quantity q of B_x, B_y, B_z, G_x, G_y, G_z is
 *               taken as q_t = q(p) + t (q(p') - q(p)).  pos_d = lo_d + (i_d + t) h_d, the sum formed first; on the
 *               other two axes pos = lo + i h.  curv = B_x,t G_x,t + B_y,t G_y,t: (B.grad)B_z where B_z = 0; the z term
 *               is left out, not rounded in.
 *   dip         a crossing is a DIP iff curv > 0, strict.  There is no separate rule for values that are not finite: a
 *               NaN among the values that enter t or curv makes them NaN, the comparison false, and excludes the
 *               edge; so does every Inf that meets another Inf or a zero factor there (Inf - Inf, 0 Inf), as all do in
 *               a block of Inf over all three components.  G_z,t enters neither t nor curv: next to a block of NaN a
 *               record's grad_z can be NaN.  A lone Inf can pass - curv = +Inf where it reaches one of the two ends'
 *               values only, or a finite curv next to a B_z,t that is not finite on a z edge -: a field with Inf in it
 *               is the caller's to mask.
 *   record      of a dip: edge; pos; bpt = (B_x,t, B_y,t, B_z,t); grad = (G_x,t, G_y,t, G_z,t); curv; flag, bit 0: a
 *               BALD PATCH, k = 0 and d != 2 (an edge of the lower boundary plane).  The curvature of the field line
 *               at its lowest point is curv / (B_x,t^2 + B_y,t^2) (ndsm_amd's Dips.kappa).
 *   order       records come out in ascending edge, whatever the launch geometry, with the same bits on every run and
 *               from both entries: output positions come from counts and a scan - no atomic append, no sort, and no
 *               result that depends on an internal buffer's size.  counts[1] > max_dips: max_dips only truncates the
 *               records written - the first max_dips in edge order - and the call still returns 0.
 *   plane_only  = 1: only the nodes of k = 0 and the families 0 and 1 are looked at, at O(nx ny) cost (the gradient
 *               along z reads the planes k = 1, 2 at the crossings).  The records are, bit for bit, those records of
 *               the full call that carry flag bit 0, counts[0] counts the crossings of that plane's x and y edges, and
 *               counts[1] == counts[2].
 * Returns 0, or >= 9001 errors: 9001 without a GPU whatever the arguments; 9002 a NULL handle, B or counts, or with
 * max_dips > 0 a NULL record array; 9004 max_dips < 0, plane_only not 0 or 1, a mesh with fewer than 3 nodes on an
 * axis.  On every failure counts is cleared; the host entry also clears the max_dips slots of every record array (on
 * success the slots past min(counts[1], max_dips) are zero), the device entry leaves its device arrays (on success it
 * writes the first min(counts[1], max_dips) slots only).
 * Device memory: the host entry stages B in the handle's scratch (24 B/pt) and max_dips records (92 B each); the call
 * keeps 3 bits per node and 24 B per 1024 nodes. */
/* HOST arrays */
int ndsm_hip_vecpot_dips(void *h, const double *B, int plane_only, int64_t max_dips, int64_t *counts, int64_t *edge,
                         double *pos, double *bpt, double *grad, double *curv, int32_t *flag);
/* the same on DEVICE arrays of the library's GPU (B and the six record arrays; counts stays on the host) */
int ndsm_hip_vecpot_dips_device(void *h, const double *dB, int plane_only, int64_t max_dips, int64_t *counts,
                                int64_t *dedge, double *dpos, double *dbpt, double *dgrad, double *dcurv,
                                int32_t *dflag);

/* ---- Flow inversion and boundary fluxes (DESIGN.md "Flow inversion and boundary fluxes") ---------------------------
 * Every entry above reads one magnetogram.  These take two: the plasma velocity on the lower face from a pair of
 * vector magnetograms - a local affine fit of the normal component of the induction equation, in the manner of
 * DAVE4VM (Schuck 2008) -, the potential field's vector potential ON the plane, and with both the fluxes of relative
 * helicity and of magnetic energy through the face (Berger & Field 1984): how fast the H and E of
 * ndsm_hip_vecpot_helicity enter the box.  No handle.  Fields are component planes with x fastest, B (nsx,nsy,3); the
 * mesh is uniform, hx = xs[1] - xs[0] and hy = ys[1] - ys[0], both > 0; pixel (i,j) is c = i + nsx j.  fp64 + - * /
 * and sqrt only, in the operand order written here, no contraction: a restatement in the same order gives the same
 * bits (tests/flow_model.py).
 *
 * ndsm_hip_flow_fit.  B0, B1 (nsx,nsy,3) at two times dt apart (dt finite, != 0, of either sign); nsx, nsy >= 3;
 *   r the half width of the window, 1 <= r <= 16: the (2r+1)^2 pixels around a target, each with weight 1 (top-hat);
 *   rcond with 0 <= rcond < 1.  Out: V (nsx,nsy,3), coef (nsx,nsy,9), status (nsx,nsy; int32).
 *   staged    per pixel, seven quantities:  Bm_c = 0.5 (B0_c + B1_c) for c = x, y, z;  T = (B1_z - B0_z) / dt;
 *             Zx = ddq_x(Bm_z), Zy = ddq_y(Bm_z), D = ddq_x(Bm_x) + ddq_y(Bm_y), with ddq the nodal difference
 *             quotient of ndsm_hip_vecpot_dips ("gradient") in exactly its operand order: centred inside, 3-point
 *             one-sided on the end rows.
 *   model     inside the window of the target (i,j) the flow is affine, u = u0 + ux x' + uy y', v = v0 + vx x' + vy y',
 *             w = w0 + wx x' + wy y', with x' = (double)a hx and y' = (double)b hy at the window pixel (i + a, j + b).
 *             The residual of d_t B_z + div_h (B_z V_h - V_z B_h) there is T + s.p, p = (u0, ux, uy, v0, vx, vy, w0,
 *             wx, wy), and with every quantity taken at the window pixel
 *               s = ( Zx,  Zx x' + Bz,  Zx y',   Zy,  Zy x',  Zy y' + Bz,   -D,  -(D x') - Bx,  -(D y') - By ).
 *   sums      G_kl = sum s_k s_l (k <= l) and g_k = sum (-T) s_k over the window pixels that lie inside the
 *             magnetogram - windows are clipped, not padded -, b ascending outer, a ascending inner, every sum starting
 *             at 0.0: G_kl = G_kl + s_k s_l; g_k = g_k + (-T) s_k.
 *   scaling   d_k = 1.0 / sqrt(G_kk);  Gs_kl = (G_kl d_k) d_l;  gs_k = g_k d_k.
 *   LDL^T     of Gs without pivoting, k ascending; every inner sum starts at 0.0 and adds left to right:
 *               for j < k (ascending):  w_kj = Gs_jk - sum_{m<j} w_km L_jm;   L_kj = w_kj / D_j;
 *               D_k = Gs_kk - sum_{j<k} w_kj L_kj.
 *             Then y_k = gs_k - sum_{j<k} L_kj y_j (k ascending);  z_k = y_k / D_k;
 *             ps_k = z_k - sum_{j>k} L_jk ps_j (k descending, j ascending);  p_k = ps_k d_k.
 *   status    2: one of the seven staged quantities of a window pixel is not finite; V and coef are NaN.  Otherwise
 *             1: rank-deficient - the aperture problem -: some G_kk is not > 0, or some pivot D_k is not > rcond; V
 *             and coef are 0.0.  Otherwise 0: solved; coef = p, V = (p_0, p_3, p_6) = (u0, v0, w0).
 *   A separable running-sum form of the sums would be O(1) per pixel but has another order and cancellation; it is not
 *   what runs.  Device memory: seven planes of scratch (56 B per pixel), kept between calls and grown on demand.
 *
 * ndsm_hip_green_ap_points, ndsm_hip_green_ap_plane.  A_p with A_p.n = 0, div_h A_p = 0 and z.curl A_p = B_z on the
 *   plane: the third pair term of the all-pairs sum of ndsm_hip_green_points.  Source, c = (hx hy) /
 *   6.283185307179586, slices, order of the sum and fold: exactly those of ndsm_hip_green_points (zs is not needed).
 *   One target (X, Y) on the plane.  For pixel p: q = bz[p] c; dx = X - xs[i]; dy = Y - ys[j]; r2 = dx dx + dy dy; if
 *   r2 > 0: t = q / r2 and the two terms are (-dy) t and dx t; otherwise the pixel contributes no term (the punctured
 *   rule).  With the punctured rule the sum is second order in h on the source's own nodes: the singular part of the
 *   kernel is odd about the target, so the pixel left out costs O(h^2).
 *   _points: Ap (2,npts) at pts (2,npts).  _plane: Ap (nsx,nsy,2) on the source's own nodes (xs[i], ys[j]).  A node
 *   gets the same bits from both.  npts == 0 returns 0 and touches nothing.
 *
 * ndsm_hip_flow_flux.  B, V (nsx,nsy,3), Ap (nsx,nsy,2); nsx, nsy >= 2.  Out dens (nsx,nsy,4), per pixel
 *     h_em = 2.0 ((Apx Bx + Apy By) Vz)        h_sh = -2.0 ((Apx Vx + Apy Vy) Bz)
 *     s_em = (Bx Bx + By By) Vz                 s_sh = -((Bx Vx + By Vy) Bz)
 *   the emergence and shear terms of dH/dt = 2 int [(A_p.B_h) V_z - (A_p.V_h) B_z] dA and of the Poynting flux
 *   dE/dt = int [B_h^2 V_z - (B_h.V_h) B_z] dA - without 4 pi, as E = 1/2 sum w |B|^2 of ndsm_hip_vecpot_helicity.
 *   out[8], on the HOST in both forms: [0] sum w h_em, [1] sum w h_sh, [2] out[0] + out[1], [3] sum w s_em,
 *   [4] sum w s_sh, [5] out[3] + out[4], [6] sum w |Bz|, [7] sum w Bz;  w = wx(i) wy(j), wx = hx inside and 0.5 hx
 *   on both end rows, likewise wy: the trapezoid weights.  Each sum is sum = sum + w term in the order of the
 *   reduction behind ndsm_hip_vecpot_helicity: NB = min(nsy, 2048) blocks of 256 lanes; lane t of block b adds, from
 *   0.0, the rows j = b, b + NB, ... and in a row the pixels i = t, t + 256, ...; a halving tree over the lanes
 *   (lane t += lane t + o, o = 128 .. 1); then lane t of one block adds, from 0.0, the results of the blocks t,
 *   t + 256, ..., and the same tree.  No atomics: the same input gives the same bits.  One blocking read.
 *
 * The mesh vectors stay on the HOST in both forms.  Returns 0 or, in this order: 9001 without a GPU whatever the
 *   arguments; 9001 before anything is allocated - as soon as the shapes can be read - when the arrays and the scratch
 *   exceed the device's TOTAL memory (the screen of the Green's-function entries); 9002 a NULL array or shape; 9004 an
 *   axis < 2 (the fit: < 3), a spacing not > 0, npts < 0, and for the fit a dt that is 0 or not finite, r outside
 *   1..16, rcond outside [0, 1) or not finite.  A failed call leaves the outputs untouched. */
/* HOST arrays */
int ndsm_hip_flow_fit(const int nsrc[2], const double *xs, const double *ys, const double *B0, const double *B1,
                      double dt, int r, double rcond, double *V, double *coef, int32_t *status);
/* the same with B0, B1, V, coef and status DEVICE arrays of the library's GPU */
int ndsm_hip_flow_fit_device(const int nsrc[2], const double *xs, const double *ys, const double *dB0,
                             const double *dB1, double dt, int r, double rcond, double *dV, double *dcoef,
                             int32_t *dstatus);
/* HOST arrays */
int ndsm_hip_green_ap_points(const int nsrc[2], const double *xs, const double *ys, const double *bz, int npts,
                             const double *pts, double *Ap);
/* the same with bz, pts and Ap DEVICE arrays of the library's GPU */
int ndsm_hip_green_ap_points_device(const int nsrc[2], const double *xs, const double *ys, const double *dbz, int npts,
                                    const double *dpts, double *dAp);
/* HOST arrays */
int ndsm_hip_green_ap_plane(const int nsrc[2], const double *xs, const double *ys, const double *bz, double *Ap);
/* the same with bz and Ap DEVICE arrays of the library's GPU */
int ndsm_hip_green_ap_plane_device(const int nsrc[2], const double *xs, const double *ys, const double *dbz,
                                   double *dAp);
/* HOST arrays (out too) */
int ndsm_hip_flow_flux(const int nsrc[2], const double *xs, const double *ys, const double *B, const double *V,
                       const double *Ap, double *dens, double out[8]);
/* the same with B, V, Ap and dens DEVICE arrays of the library's GPU; out stays on the host */
int ndsm_hip_flow_flux_device(const int nsrc[2], const double *xs, const double *ys, const double *dB,
                              const double *dV, const double *dAp, double *ddens, double out[8]);

/* ---- Flux partitioning and connectivity (DESIGN.md "Flux partitioning and connectivity") ---------------------------
 * The nulls, spines and fans, separators, Q and the bald patches are the BOUNDARIES of the flux domains of a field.
 * These entries say what the domains are and how much flux each holds, the question of magnetic charge topology
 * (Barnes, Longcope & Leka 2005; Longcope 2005): the magnetogram falls into flux patches, and some amount of flux links
 * patch a to patch b.  fp64 + - * / only, in the operand order written here, no contraction: a numpy restatement in the
 * same order gives the same bits.
 *
 * The keyed sum.  Every sum below is grouped by a key that the data decide - a patch, a pair of patches.  The terms of
 * one key are taken in ascending pixel index; call the q-th of them rank q.  Lane l of 64 adds the ranks l, l + 64, ...
 * in that order, from 0.0.  Then v[l] = v[l] + v[l + d] for l < d, d = 32, 16, ... 1.  The sum is v[0].  A key with one
 * term adds only the tree's zeros to it, which leaves it unchanged except that a lone -0.0 becomes +0.0.  The same bits
 * on every run and from both entries: the terms of a key are brought together by a stable sort of (key, pixel), whose
 * result is unique, and nothing is added atomically.
 *
 * ndsm_hip_partition: no handle, a plane entry like the flow entries.
 *   nsrc, xs, ys  a uniform mesh with nsx, nsy >= 2; hx = xs[1] - xs[0], hy = ys[1] - ys[0] as the flow entries form
 *                 them, both > 0.  The mesh vectors are on the HOST in both forms.
 *   bz            (nsx,nsy), pixel p = i + nsx j; at most 2^31 - 1 pixels
 *   thr           >= 0, finite
 *   max_patches   >= 0 (int64): the capacity of the record arrays; 0 counts only (no record array is looked at)
 *   counts        int64[2], a HOST array in both forms: (pixels in, patches K), exact whatever the capacity
 *   label         int32 (nsx,nsy), always fully written
 *   records       of the first min(K, max_patches) patches: root int64, sign int32, npix int64, flux, sx, sy doubles
 * Semantics:
 *   in          pixel p is IN iff fabs(bz) > thr.  A NaN is not in.  Its sign is bz > 0.
 *   pointer     consider p itself and those of its 8 neighbours that lie inside the magnetogram, are in and have p's
 *               sign; there is no padding and no wrap.  ptr(p) is the candidate with the greatest |bz|; equal values go
 *               to the smallest pixel index.  So (|bz|, -index) strictly increases along pointers, there are no
 *               cycles, and plateaus drain to one pixel.
 *   root        the fixed point reached from p.  It is unique whatever way it is found.
 *   numbering   patches are k = 1 .. K in ascending root index.  label(p) = k, and 0 for pixels not in.
 *   weights     w(p) = wx(i) wy(j), the trapezoid weights of ndsm_hip_flow_flux: hx inside, 0.5 hx on both end rows,
 *               likewise wy.  f(p) = bz(p) w(p).
 *   table       of patch k: root; sign +1 or -1; npix; flux = sum f; sx = sum f xs[i] and sy = sum f ys[j] (the
 *               centroid is the quotient (sx / flux, sy / flux), ndsm_amd's Patches.centroid).  Every sum is a keyed
 *               sum over the patch's pixels.
 *   Infinities  +Inf and -Inf are in and are peaks like any other.  There is no special rule: a field with Inf in it
 *               is the caller's to mask, as in the dips entry.
 * Returns 0, or >= 9001 errors, in this order: 9001 without a GPU, whatever the arguments; 9001 from the memory screen
 * as soon as the shapes can be read (the arrays and 50 bytes of scratch a pixel against the device's memory); 9002 a
 * NULL nsrc, xs, ys, bz, counts or label, or with max_patches > 0 a NULL record array; 9004 fewer than 2 nodes on an
 * axis, more than 2^31 - 1 pixels, a spacing that is not > 0, a thr that is not finite and >= 0, max_patches < 0.  On
 * every failure counts is cleared.  The host form also clears its outputs - the max_patches rows of its records and,
 * once the shape has passed its checks, label.  The device form leaves them. */
/* HOST arrays */
int ndsm_hip_partition(const int nsrc[2], const double *xs, const double *ys, const double *bz, double thr,
                       int64_t max_patches, int64_t *counts, int32_t *label, int64_t *root, int32_t *sign,
                       int64_t *npix, double *flux, double *sx, double *sy);
/* the same with bz, label and the six record arrays DEVICE arrays of the library's GPU (counts stays on the host) */
int ndsm_hip_partition_device(const int nsrc[2], const double *xs, const double *ys, const double *dbz, double thr,
                              int64_t max_patches, int64_t *counts, int32_t *dlabel, int64_t *droot, int32_t *dsign,
                              int64_t *dnpix, double *dflux, double *dsx, double *dsy);

/* ndsm_hip_vecpot_connect: on a handle, since it traces through the volume.
 *   B             (nx,ny,nz,3) on the handle's mesh
 *   label, K      label int32 (nx,ny) on the lower face and K >= 0.  A label outside 1 .. K counts as 0, both for the
 *                 seed and at the destination, so every key is bounded whatever the caller passes.
 *   step, max_steps  as in ndsm_hip_vecpot_trace
 *   max_pairs     >= 0 (int64): the capacity of the pair arrays; 0 counts only
 *   counts        int64[2], a HOST array in both forms: (lines traced, distinct pairs M)
 *   per pixel     on (nx,ny): dest int32, ends (3,npix), length, status int32
 *   pairs         pa, pc int32, nlines int64, pflux double
 * Semantics:
 *   line of p   the seed is (x_i, y_j, lo_z) from the handle's mesh.  sgn = +1 if B_z(node) > 0 and -1 if < 0: the sign
 *               comes from the field that is traced, not from the label.  No line is traced if label(p) == 0 (after
 *               the 1 .. K rule), if B_z is 0 or NaN there, or if the seed is not inside the trace entry's box [lo, hi]
 *               (ndsm_hip_vecpot_trace answers NDSM_HIP_TRACE_OUTSIDE for it too); then dest = NDSM_HIP_CONNECT_NONE
 *               (-9), end = seed, length = 0 and status = NDSM_HIP_TRACE_OUTSIDE.  Otherwise one lane walks the trace
 *               entry's loop with that per-lane sgn: ends, length and status are BIT FOR BIT what
 *               ndsm_hip_vecpot_trace returns for that seed with direction sgn and G = NULL.
 *   class c     of the destination.  If status is ZLO, c is the label (after the 1 .. K rule) of the nearest pixel,
 *               i' = clamp((int)floor((x - lo_x) / h_x + 0.5), 0, nx - 1), likewise j'.  Otherwise c = -status, one of
 *               -1 .. -4, -6, -7, -8.  dest(p) = c.  c = a, a line that comes back to its own patch, is a pair like
 *               any other.
 *   pairs       the key is (a, c) with a = label(p).  Records come in ascending a, then ascending c.  nlines is the
 *               number of lines with that key; pflux is the keyed sum of fabs(B_z(p)) w(p), with w the trapezoid
 *               weight of the plane (h_x, h_y the handle's spacings).  The matrix is ONE-SIDED on purpose: Psi(a -> b)
 *               is counted from a's feet and Psi(b -> a) from b's (ndsm_amd's connectivity_matrix offers the
 *               symmetric mean).
 *   capacity    counts is exact whatever max_pairs; the first max_pairs records in key order are written and the call
 *               still returns 0 when there are more.
 * Returns 0, or >= 9001 errors: 9001 without a GPU whatever the arguments; 9002 a NULL handle, B, label, counts or
 * per-pixel array, or with max_pairs > 0 a NULL pair array; 9004 K < 0, max_pairs < 0, a step that is not > 0 and finite,
 * max_steps < 1.  On every failure counts is cleared; on a failure past the handle's check the host entry also clears
 * its per-pixel arrays and the max_pairs slots of its pair arrays, the device entry leaves its device arrays. */
#define NDSM_HIP_CONNECT_NONE (-9)
/* HOST arrays */
int ndsm_hip_vecpot_connect(void *h, const double *B, const int32_t *label, int K, double step, int max_steps,
                            int64_t max_pairs, int64_t *counts, int32_t *dest, double *ends, double *length,
                            int32_t *status, int32_t *pa, int32_t *pc, int64_t *nlines, double *pflux);
/* the same on DEVICE arrays of the library's GPU (B, label and the eight output arrays; counts stays on the host) */
int ndsm_hip_vecpot_connect_device(void *h, const double *dB, const int32_t *dlabel, int K, double step, int max_steps,
                                   int64_t max_pairs, int64_t *counts, int32_t *ddest, double *dends, double *dlength,
                                   int32_t *dstatus, int32_t *dpa, int32_t *dpc, int64_t *dnlines, double *dpflux);

#ifdef __cplusplus
}
#endif
#endif
