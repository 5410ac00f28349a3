/* Device layer of libndsm_hip: runtime + HIP kernel launchers (gfx950).
 *
 * This is the *internal* C interface between the Fortran 2003 host driver
 * (ndsm_amd/fsrc, bound through ISO_C_BINDING in ndsmh_iface.f90) and the
 * hand-written HIP kernels.  The drop-in boundary a user binds against is
 * include/ndsm_hip.h, not this file.
 *
 * Conventions
 *   - every function returns 0 on success, a non-zero HIP / NDSMK_E* code on
 *     failure; ndsmk_last_error() gives the text.  Nothing falls back to the CPU.
 *   - all kernels are enqueued on ONE library-owned HIP stream and return
 *     immediately unless stated "blocking".
 *   - arrays are Fortran order (x fastest); pointers are device pointers
 *     unless prefixed h_.
 *   - a level's geometry travels in ndsmk_grid (filled by the host driver with
 *     the reference's arithmetic, ndsm_optimized.f90:68-94).
 */
#ifndef NDSM_KERNELS_H
#define NDSM_KERNELS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
  NDSMK_OK = 0,
  NDSMK_ENODEV = 9001,   /* no HIP device visible */
  NDSMK_EARG = 9002,     /* shape/argument check failed on the host */
  NDSMK_ENCCL = 9003,    /* RCCL call failed */
  NDSMK_EVALUE = 9004    /* a scalar argument outside its range (the line entries, ndsmk_nulls) */
};

/* geometry + operator constants of one grid level (interoperable with the
 * Fortran TYPE, BIND(C) :: ndsmk_grid in ndsmh_iface.f90) */
typedef struct {
  int32_t ndim;          /* 2 or 3 */
  int32_t n[3];          /* nx, ny, nz (nz = 1 in 2-D) */
  int32_t lb[3], ub[3];  /* 0-based inclusive update bounds: shrink by one on 'D' faces */
  int32_t first_par;     /* colour of the first half-sweep: (i+j+k)&1 == first_par */
  int32_t all_neumann;   /* 1: subtract the mean after each sweep */
  int32_t k0;            /* global z index of local plane 0 (z-slab runs; may be negative), else 0 */
  int32_t nzg;           /* global nz (== n[2] unless z-slab) */
  int32_t zown0, zown1;  /* local planes [zown0, zown1) are owned (written); the rest are ghosts. 0, n[2] unless z-slab */
  double w[3];           /* 1/h^2 per dimension */
  double w1;             /* 1 / (2 (wx+wy+wz)) */
  double wc;             /* 2 (wx+wy+wz) */
} ndsmk_grid;

/* one inter-level transfer: 1-D tables per dimension, built on the host with
 * the reference's arithmetic (ndsm_interp.f90:373-435, :141-142, :229-281) */
typedef struct {
  int32_t nf[3], nc[3];   /* fine / coarse shapes */
  int32_t maxt[3];        /* taps reserved per coarse index and dim (row length of rw) */
  /* prolongation: per fine index i of dim d */
  const int32_t *plo[3];  /* lower bracket index into the coarse dim (0-based) */
  const double *pwl[3];   /* weight of the UPPER bracket point  wl = (q-ql)/dq */
  const double *pwh[3];   /* weight of the LOWER bracket point  wh = -(q-qh)/dq */
  /* restriction: per coarse index I of dim d */
  const int32_t *rlo[3];  /* first contributing fine index (0-based) */
  const int32_t *rcnt[3]; /* number of contributing fine points */
  const double *rw[3];    /* rw[d][I*maxt[d] + t] = c2 = |h_c - |q_f - q_c||  (ndsm_interp.f90:279-280) */
  double w2[3];           /* h_f / h_c^2 per dimension (ndsm_interp.f90:229) */
  /* z-slab windows (all zero / full range when not distributed).  The z tables are
   * always indexed with GLOBAL plane numbers; the arrays may hold a window. */
  int32_t f_k0;           /* global index of plane 0 of the fine array */
  int32_t f_beg, f_cnt;   /* local fine planes [f_beg, f_beg+f_cnt) are written by prolong_add */
  int32_t c_k0;           /* global index of plane 0 of the coarse array */
  int32_t c_beg, c_cnt;   /* local coarse planes [c_beg, c_beg+c_cnt) are written by restrict */
  int32_t stream_ok;      /* host-checked, restrict_stream.hip: bit 1 its tile covers this pair's taps,
                             bit 0 and the level is large enough for it to be the default; bit 2 + bits 8-31:
                             what the scheduled form needs to know about the z windows (launch_rs_t) */
} ndsmk_xfer;

/* ---- runtime ------------------------------------------------------- */
int ndsmk_device_count(void);
int ndsmk_init(int device);                 /* device < 0: LOCAL_RANK % count (else 0) */
int ndsmk_shutdown(void);
const char *ndsmk_last_error(void);
int ndsmk_note_error(int code, const char *what);   /* records the text, returns code */
int ndsmk_device_name(char *buf, int len);
void *ndsmk_stream(void);                   /* the library's hipStream_t */

int ndsmk_alloc(void **p, size_t bytes);
int ndsmk_free(void *p);
int ndsmk_h2d(void *dst, const void *h_src, size_t bytes);   /* blocking */
int ndsmk_d2h(void *h_dst, const void *src, size_t bytes);   /* blocking */
int ndsmk_d2d(void *dst, const void *src, size_t bytes);
// ghost planes of a smoothing pass: black points + perimeter only (halo.hip)
long long ndsmk_halo_packed_plane(int nx, int ny);
int ndsmk_halo_pack(const double *src, double *buf, int nx, int ny, int depth, int kg0, int first_par);
int ndsmk_halo_unpack(double *dst, const double *buf, int nx, int ny, int depth, int kg0, int first_par);
int ndsmk_halo_copy(double *dst, const double *src, int nx, int ny, int depth, int kg0, int first_par);
int ndsmk_fill0(void *p, size_t bytes);
int ndsmk_sync(void);                                        /* blocking */
int ndsmk_timer_start(void);                /* hipEventRecord on the library stream */
int ndsmk_timer_stop(double *ms);           /* blocking; elapsed between start and now */

/* background transfers: one worker thread + copy stream move the caller's host arrays while the main
 * thread drives the solves.  upload_unless_zero: scan the host array; copy it to d_dst unless every byte
 * is zero (*flag of ndsmk_bg_wait = 1: nothing copied, the caller zero-fills).  download: starts once the
 * main stream has passed the point of the call.  Tickets die in ndsmk_bg_drain (blocking, first error). */
int ndsmk_bg_upload_unless_zero(const void *h_src, void *d_dst, size_t bytes, int *ticket);
int ndsmk_bg_download(void *h_dst, const void *d_src, size_t bytes, int *ticket);
int ndsmk_bg_first_touch(void *h_dst, size_t bytes, int *ticket);   /* h_dst will be overwritten completely */
int ndsmk_bg_wait(int ticket, int *flag);
int ndsmk_bg_drain(void);
int ndsmk_host_alloc(void **p, size_t bytes);               /* pinned */
int ndsmk_host_free(void *p);
int ndsmk_mem_info(size_t *free_bytes, size_t *total_bytes);
int ndsmk_h2d_async(void *dst, const void *h_pinned_src, size_t bytes);
void ndsmk_at_reset(void (*fn)(void));                      /* fn runs at the next shutdown / re-target */
void ndsmk_on_low_memory(void (*fn)(void));                 /* fn runs when a device allocation fails, before one retry */

/* ---- kernels ------------------------------------------------------- */
/* nsweeps full red-black Gauss-Seidel sweeps (ndsm_optimized.f90:40-191 in
 * 3-D, ndsm_poisson.f90:451-549 in 2-D incl. the all-Neumann mean shift).
 * variant: 0 = pick the fastest valid kernel, 1 = two-pass colour kernels (in
 * place), 2 = fused z-streaming kernel (3-D only, out of place).
 * rhs == NULL means rhs is identically zero (never dereferenced; same bits).
 * ualt: a second array of the level's size (may be NULL: colour kernels only).
 * The fused kernel ping-pongs u <-> ualt once per sweep; on return
 * *result_in_alt = 1 means the swept field is in ualt and the caller must swap
 * its two pointers (result_in_alt == NULL: it is copied back into u). */
int ndsmk_relax(const ndsmk_grid *g, double *u, double *ualt, const double *rhs, int nsweeps, int variant,
                int *result_in_alt);
/* nsweeps sweeps, then r = rhs - L u of the result (fused into the last sweep's launch where possible) */
int ndsmk_relax_residual(const ndsmk_grid *g, double *u, double *ualt, const double *rhs, double *r, int nsweeps,
                         int variant, int *result_in_alt);
/* The zero first guess of a coarse level, kept out of memory: either call above on a level whose u
 * IS ZERO BUT WAS NEVER WRITTEN - u may hold anything.  Where the planner lets the first launch take its source from
 * a buffer descriptor of zero records (an out-of-place fused pass) u is never read; otherwise u is zero-filled first.
 * r == NULL: ndsmk_relax, else ndsmk_relax_residual.  Same bits as those calls on an array of zeros.
 * ndsmk_relax_zero_src_ok: 1 if that call would not have to write the zeros (has_rhs / with_res: rhs / r != NULL);
 * 0 always while the feature is off - NDSM_HIP_NO_ZERO_GUESS=1 in the environment, or ndsmk_debug_zero_guess(0)
 * (tests: A/B in one process; 1 = back to the default).  ndsmk_zero_guess_on: 1 / 0. */
int ndsmk_relax_zero_src(const ndsmk_grid *g, double *u, double *ualt, const double *rhs, double *r, int nsweeps,
                         int variant, int *result_in_alt);
int ndsmk_relax_zero_src_ok(const ndsmk_grid *g, int has_rhs, int nsweeps, int variant, int with_res);
int ndsmk_zero_guess_on(void);
int ndsmk_debug_zero_guess(int on);
/* r = rhs - L u, zero on Dirichlet faces (ndsm_optimized.f90:346-447 / ndsm_poisson.f90:280-353) */
int ndsmk_residual(const ndsmk_grid *g, const double *u, const double *rhs, double *r);
/* rhs_c = R r_f ; also u_c = 0 if u_c != NULL (ndsm_multigrid_core.f90:551,557-558) */
int ndsmk_restrict(const ndsmk_xfer *x, const double *r_f, double *rhs_c, double *u_c);
/* footprint of the LDS-streamed restriction, for the host-side coverage check */
void ndsmk_restrict_stream_tile(int *ci, int *cj, int *fx, int *fy, int *maxt);
/* u_f += P u_c (ndsm_multigrid_core.f90:659,672) */
int ndsmk_prolong_add(const ndsmk_xfer *x, const double *u_c, double *u_f);
/* Which form the two calls above take is decided by level size.  ndsmk_debug_transfer_cfg (tests) replaces the sizes
 * (fine points from which a pair is marked for the streamed restriction when its hierarchy is built / from which
 * ndsmk_prolong_add takes the tiled kernel), the streamed restriction's form (5, 8, 10 - NDSM_RS_VARIANT) and its coarse
 * planes per chunk; a negative value restores the built-in choice.  ndsmk_debug_transfer_form: out[0] = 0 gather /
 * 5, 8, 10 the streamed form ndsmk_restrict runs for x, out[1..2] = its kc and nkc, out[3] = 1 if ndsmk_prolong_add
 * runs the tiled kernel - answered by the functions the launchers themselves ask. */
long long ndsmk_restrict_stream_min_points(void);
int ndsmk_debug_transfer_cfg(long long restrict_min_points, long long prolong_min_points, int rs_variant, int rs_chunk);
int ndsmk_debug_transfer_form(const ndsmk_xfer *x, int out[4]);
/* blocking: out[0] = max|a-b|, out[1] = sum|a-b| ; then b <- a if copy != 0
 * (update_u, ndsm_multigrid_core.f90:1077-1122 ; du_metrics :808-853) */
int ndsmk_diff_metrics(const double *a, double *b, int64_t n, int copy, double *h_out2);
/* its two halves: enqueue on the selected stream / lane; wait for that stream and read the pair */
int ndsmk_diff_metrics_begin(const double *a, double *b, int64_t n, int copy);
int ndsmk_diff_metrics_end(double *h_out2);
/* coarsest-grid "exact" solve (ndsm_multigrid_core.f90:728-800): repeat
 * {test du <= ex_tol first; relax; du = max|.| or mean|.| of the change} at most
 * nmax times.  d_info (DEVICE, 2 x int64) accumulates [0] sweeps done and
 * [1] the number of solves that hit nmax unconverged; the call does not block
 * for grids of <= 2048 points.  scratch: n doubles (device). */
int ndsmk_solve_exact(const ndsmk_grid *g, double *u, const double *rhs, double *scratch,
                      double ex_tol, int use_max, int nmax, int64_t *d_info);
int ndsmk_solve_exact_on_device(const ndsmk_grid *g);   /* 1: that solve is one launch, nothing comes back to the host */

/* The bottom of a V-cycle as ONE single-workgroup launch (tail.hip): levels g[0..nlev-1] (g[nlev-1] the
 * coarsest grid, x[q] the transfer g[q] -> g[q+1], u[q] / rhs[q] their DEVICE arrays), all resident in LDS:
 * ms sweeps + residual + restriction down, solve_exact + ms sweeps, interpolation + 2 ms sweeps up.
 * ndsmk_tail_applies: 1 if these levels are covered (3-D, whole levels, <= 6144 points, <= 4 levels).
 * Bit-identical to the level-by-level kernels.  ndsmk_debug_tail(0 / 1): tests switch it off / on. */
int ndsmk_tail_applies(int nlev, const ndsmk_grid *g, const ndsmk_xfer *x);
int ndsmk_tail_cycle(int nlev, const ndsmk_grid *g, const ndsmk_xfer *x, double *const *u, double *const *rhs, int ms,
                     double ex_tol, int use_max, int nmax, int64_t *d_info);
int ndsmk_debug_tail(int on);

/* A += flux-balance fields, B = curl A (+ linear field when curl_first), all on
 * device arrays (nx,ny,nz,3); x,y,z are DEVICE mesh vectors, h_* host scalars
 * (ndsm_vector_potential.f90:453-477, :759-872, :880-950) */
int ndsmk_balance_curl(double *A, double *B, const int32_t *n3, const double *x, const double *y,
                       const double *z, const double *h_phi6, const double *h_span3,
                       const double *h_dq3, int curl_first);
/* the same on a z-slab: A (nx,ny,na,3) holds global planes [kg0, kg0+na) - one ghost plane per
 * neighbour -, B (nx,ny,nb,3) starts at A's local plane boff; n3 and x,y,z stay GLOBAL */
int ndsmk_balance_curl_slab(double *A, double *B, const int32_t *n3, int kg0, int na, int nb, int boff,
                            const double *x, const double *y, const double *z, const double *h_phi6,
                            const double *h_span3, const double *h_dq3, int curl_first);

/* one component (c = 0,1,2) of the flux-balance fields added to that component of A alone (same
 * expressions as ndsmk_balance_curl's first kernel: components can be finished one at a time), and the
 * curl alone: B = curl A on device arrays (nx,ny,nz,3) */
int ndsmk_balance_component(double *Ac, const int32_t *n3, int c, const double *x, const double *y, const double *z,
                            const double *h_phi6, const double *h_span3);
int ndsmk_curl(const double *A, double *B, const int32_t *n3, const double *h_dq3);
/* component c of B alone (needs the other two components of A only) */
int ndsmk_curl_component(const double *A, double *B, const int32_t *n3, const double *h_dq3, int c);

/* the current-carrying field (field.hip): rhs = -(curl B)_c of a device field B (nx,ny,nz,3) into a device
 * array (nx,ny,nz) - the same bits as -ndsmk_curl_component(B)_c -, and the blocking, deterministic reduction
 * behind ndsm_hip_vecpot_helicity (h_out8 as documented there) */
int ndsmk_curl_rhs(const double *B, double *rhs, const int32_t *n3, const double *h_dq3, int c);
int ndsmk_helicity_reduce(const double *A, const double *Ap, const double *B, const double *Bp, const double *Br,
                          const int32_t *n3, const double *h_dq3, double *h_out8);

/* the nonlinear force-free field (field.hip; semantics: include/ndsm_hip.h, ndsm_hip_vecpot_nlfff).  current_rhs: rhs
 * = -F_c (alpha NULL: F a prescribed current J) or rhs = -(alpha F_c) (F = B, the Grad-Rubin pass: the bits of numpy's
 * -(alpha * b)), F (nx,ny,nz,3), alpha, rhs (nx,ny,nz) DEVICE arrays; asynchronous.  nlfff_metrics: blocking,
 * deterministic; h_out4 = [max |B_c - Bold_c|, 1/2 sum w |B|^2, sum w |J x B| / |B| over sum w |J| with J = curl_h B,
 * the number of ZLO entries of status (nx,ny,nz; int32)]. */
int ndsmk_current_rhs(const double *F, const double *alpha, double *rhs, const int32_t *n3, int c);
int ndsmk_nlfff_metrics(const double *B, const double *Bold, const int32_t *status, const int32_t *n3,
                        const double *h_dq3, double *h_out4);

/* The optimization-method force-free solver (optimize.hip; semantics: include/ndsm_hip.h, ndsm_hip_vecpot_optimize).
 * B0, B1 (nx,ny,nz,3): the two field buffers, B0 holds the start; O (nx,ny,nz,3,2): the two Omega buffers; w (nx,ny,nz)
 * or NULL (1 everywhere); work: ndsmk_optimize_work_bytes() bytes, the state and the block partials; all DEVICE arrays.
 * begin: the state (dt0, buffer 0 current) and Omega, L of B0.  tries: ntries tries, each decided on the device; a dt
 * below dt_min stops the rest.  Both asynchronous.  row: blocking, h_row8 (host) = [tries, L, L_f, L_d, dt, accepted,
 * the index of the buffer that holds the current field, 1 once dt < dt_min]. */
size_t ndsmk_optimize_work_bytes(void);
int ndsmk_optimize_begin(double *B0, double *B1, double *O, const double *w, double *work, const int32_t *n3,
                         const double *h_dq3, double dt0, double dt_min);
int ndsmk_optimize_tries(double *B0, double *B1, double *O, const double *w, double *work, const int32_t *n3,
                         const double *h_dq3, double dt_min, int ntries);
int ndsmk_optimize_row(const double *work, double *h_row8);

/* The same with a measurement term and a freed lower face (optimize_obs.hip; semantics: include/ndsm_hip.h,
 * ndsm_hip_vecpot_optimize_obs).  B0, B1, O, w as above; Bobs (nx,ny,3): the observation on the k = 0 plane, never
 * written; wm (nx,ny,3) or NULL (1 everywhere); work: ndsmk_optimize_obs_work_bytes() bytes; all DEVICE arrays.  nu >=
 * 0 the weight of L_m in L; free 1: the nodes of the k = 0 plane off its rim move, 0: they are held.  begin, tries:
 * asynchronous, as above.  row: blocking, h_row9 (host) = [tries, L, L_f, L_d, L_m, dt, accepted, the index of the
 * buffer that holds the current field, 1 once dt < dt_min]. */
size_t ndsmk_optimize_obs_work_bytes(void);
int ndsmk_optimize_obs_begin(double *B0, double *B1, double *O, const double *w, const double *Bobs, const double *wm,
                             double *work, const int32_t *n3, const double *h_dq3, double nu, double dt0,
                             double dt_min);
int ndsmk_optimize_obs_tries(double *B0, double *B1, double *O, const double *w, const double *Bobs, const double *wm,
                             double *work, const int32_t *n3, const double *h_dq3, double nu, int free, double dt_min,
                             int ntries);
int ndsmk_optimize_obs_row(const double *work, double *h_row9);

/* The coarse-to-fine cascade's level changes (resample.hip; semantics: include/ndsm_hip.h, ndsm_hip_resample).
 * resample: dst (ndst3, ncomp) = src (nsrc3, ncomp) resampled on the same box, mode 0 linear interpolation, mode 1 hat
 * average (no axis of dst finer than src's); DEVICE arrays that do not overlap; 9004 for a bad ncomp, mode or shape.
 * resample_weighted: (dst, wdst) (ndst3, ncomp) = the confidence-weighted restriction of the observation src with its
 * confidence wsrc (nsrc3, ncomp) (semantics: ndsm_hip_resample_weighted); no axis of dst finer than src's; four DEVICE
 * arrays that do not overlap, finite values; 9004 for a bad ncomp or shape.
 * paste_faces: dst = src on the k = 0 plane (which = 0) or on the six faces (which = 1) of two (n3, ncomp) arrays;
 * which = 2, 3: the same minus the nodes of the k = 0 plane off its rim.
 * All asynchronous. */
int ndsmk_resample(const int32_t *nsrc3, const int32_t *ndst3, int ncomp, int mode, const double *src, double *dst);
int ndsmk_resample_weighted(const int32_t *nsrc3, const int32_t *ndst3, int ncomp, const double *src,
                            const double *wsrc, double *dst, double *wdst);
int ndsmk_paste_faces(const int32_t *n3, int ncomp, int which, const double *src, double *dst);

/* Green's-function field of the half space above a magnetogram (green.hip; semantics: include/ndsm_hip.h,
 * ndsm_hip_green_points).  bz (nsx,nsy), pts (3,npts) and B are DEVICE arrays; the mesh vectors h_* stay on the HOST.
 * green_points: B (3,npts) at pts.  green_box: B (nx,ny,nz,3) on the mesh h_x, h_y, h_z - which = 0 the nodes with an
 * index at either end of an axis (the others keep what they hold), 1 all nodes.  9004 for a source axis < 2, a spacing
 * not > 0, npts < 0, which outside 0/1, a box axis < 2 or h_z[0] < zs; npts = 0 touches nothing.  Both return when B is
 * complete.  green_fits: 0, or 9001 when caller_bytes plus the mesh vectors and the scratch exceed the device's memory
 * (n3 NULL: ntargets points; else the box entry with which). */
int ndsmk_green_fits(const int32_t *nsrc2, const int32_t *n3, int which, long long ntargets, double caller_bytes);
int ndsmk_green_points(const int32_t *nsrc2, const double *h_xs, const double *h_ys, double zs, const double *bz,
                       int npts, const double *pts, double *B);
int ndsmk_green_box(const int32_t *nsrc2, const double *h_xs, const double *h_ys, double zs, const double *bz,
                    const int32_t *n3, const double *h_x, const double *h_y, const double *h_z, int which, double *B);
/* The constant-alpha (linear force-free) field of the same source (green.hip; semantics: include/ndsm_hip.h,
 * ndsm_hip_lfff_points): the arguments of the two launchers above and alpha; a non-finite alpha is 9004 as well.  The
 * chunks, the scratch and ndsmk_green_fits are shared. */
int ndsmk_lfff_points(const int32_t *nsrc2, const double *h_xs, const double *h_ys, double zs, const double *bz,
                      double alpha, int npts, const double *pts, double *B);
int ndsmk_lfff_box(const int32_t *nsrc2, const double *h_xs, const double *h_ys, double zs, const double *bz,
                   double alpha, const int32_t *n3, const double *h_x, const double *h_y, const double *h_z, int which,
                   double *B);
/* The potential field's vector potential on the plane of the magnetogram (green.hip; semantics: include/ndsm_hip.h,
 * ndsm_hip_green_ap_points): the third pair term of the same all-pairs sum.  green_ap_points: Ap (2,npts) at pts
 * (2,npts); green_ap_plane: Ap (nsx,nsy,2) on the source's own nodes; bz, pts and Ap DEVICE arrays.  9004 for a source
 * axis < 2, a spacing not > 0, npts < 0; npts = 0 touches nothing.  Both return when Ap is complete; the chunks, the
 * scratch and ndsmk_green_fits are shared. */
int ndsmk_green_ap_points(const int32_t *nsrc2, const double *h_xs, const double *h_ys, const double *bz, int npts,
                          const double *pts, double *Ap);
int ndsmk_green_ap_plane(const int32_t *nsrc2, const double *h_xs, const double *h_ys, const double *bz, double *Ap);

/* Flows from two magnetograms and the boundary fluxes (flow.hip; semantics: include/ndsm_hip.h, ndsm_hip_flow_fit and
 * ndsm_hip_flow_flux).  flow_fit: B0, B1, V (nsx,nsy,3), coef (nsx,nsy,9), status (nsx,nsy; int32) DEVICE arrays; 9004
 * for an axis < 3, a spacing not > 0, dt not finite or 0, r outside 1..16, rcond outside [0, 1).  Returns when the
 * outputs are complete; seven planes of scratch are kept between calls and grown on demand.  flow_flux: B, V
 * (nsx,nsy,3), Ap (nsx,nsy,2), dens (nsx,nsy,4) DEVICE arrays, h_out8 on the HOST; 9004 for an axis < 2 or a spacing
 * not > 0; blocking, one read of the sums.  flow_fits: 0, or 9001 when caller_bytes plus (fit = 1) the fit's scratch exceed
 * the device's memory. */
int ndsmk_flow_fits(const int32_t *nsrc2, int fit, double caller_bytes);
int ndsmk_flow_fit(const int32_t *nsrc2, const double *h_xs, const double *h_ys, const double *B0, const double *B1,
                   double dt, int r, double rcond, double *V, double *coef, int32_t *status);
int ndsmk_flow_flux(const int32_t *nsrc2, const double *h_xs, const double *h_ys, const double *B, const double *V,
                    const double *Ap, double *dens, double *h_out8);

/* Magnetogram preprocessing (preprocess.hip; semantics: include/ndsm_hip.h, ndsm_hip_vecpot_preprocess).  B0, B1
 * (nx,ny,3): the two field buffers, B0 holds the start; La (nx,ny,3,2): the two Lambda buffers; obs (nx,ny,3): the
 * observation, never written; work: ndsmk_preprocess_work_bytes() bytes, the state and the block partials; all DEVICE
 * arrays.  n2, h_dq2: nodes and spacing of the plane; h_mu5 (host) = mu1, mu2, mu3h, mu3z, mu4.  begin: the state (dt0,
 * buffer 0 current), E and M of obs, then Lambda, the sums and L of B0.  tries: ntries tries, each decided on the
 * device; a dt below dt_min stops the rest.  Both asynchronous.  row: blocking, h_row21 (host) = the 17 doubles of a
 * history row, then [the index of the buffer that holds the current field, 1 once dt < dt_min, E, M]. */
size_t ndsmk_preprocess_work_bytes(void);
int ndsmk_preprocess_begin(double *B0, double *B1, double *La, const double *obs, double *work, const int32_t *n2,
                           const double *h_dq2, const double *h_mu5, double dt0, double dt_min);
int ndsmk_preprocess_tries(double *B0, double *B1, double *La, const double *obs, double *work, const int32_t *n2,
                           const double *h_dq2, const double *h_mu5, double dt_min, int ntries);
int ndsmk_preprocess_row(const double *work, double *h_row21);

/* the solenoidal projection (project.hip), all DEVICE arrays: rhs = div_h B - c into the projection solver's
 * level-1 rhs (c = sum w div_h B / sum w stays on the device); B -= G_h phi, the normal component on the end
 * planes of its axis untouched; then, blocking, max |div_h B'| and h_out4 = [c, max |div_h B| before, after,
 * 1/2 sum w |G_h phi|^2].  Deterministic reductions. */
int ndsmk_project_div_rhs(const double *B, double *rhs, const int32_t *n3, const double *h_dq3);
int ndsmk_project_grad_sub(double *B, const double *phi, const int32_t *n3, const double *h_dq3);
int ndsmk_project_div_max(const double *B, const int32_t *n3, const double *h_dq3, double *h_out4);

/* DeVore-gauge vector potentials (devore.hip), all DEVICE arrays (nx,ny,nz,3): A of B integrated up from the base
 * plane b of B_z(z0), A_p of Bp integrated down from A's top plane (A_p(nz-1) = A(nz-1) bitwise), A_z = A_p,z = 0.
 * Trapezoid cumulative sums, h/4 and h/2 formed here from h_dq3.  A, Ap distinct.  Asynchronous. */
int ndsmk_devore(const double *B, const double *Bp, double *A, double *Ap, const int32_t *n3, const double *h_dq3);

/* Field lines and line integrals (trace.hip; semantics: include/ndsm_hip.h, NDSM_HIP_TRACE_*).  B, G (G may be NULL:
 * integrals 0) DEVICE arrays (nx,ny,nz,3); seeds (3,nseeds), ends (3,nl), length, integral, status, nsteps (nl) DEVICE
 * arrays, nl = nseeds (direction +1 / -1) or 2 nseeds (0: the forward block, then the backward block).  lo3, h_dq3:
 * first mesh point and spacing per axis; step in units of min(h); max_steps is clamped to 2^24.  NDSMK_EVALUE for
 * step <= 0, max_steps < 1, another direction, nseeds < 0; nseeds == 0 launches nothing.  Asynchronous. */
enum {
  NDSMK_TRACE_XLO = 1, NDSMK_TRACE_XHI = 2, NDSMK_TRACE_YLO = 3, NDSMK_TRACE_YHI = 4, NDSMK_TRACE_ZLO = 5,
  NDSMK_TRACE_ZHI = 6, NDSMK_TRACE_NULL = 7, NDSMK_TRACE_UNFINISHED = 8, NDSMK_TRACE_OUTSIDE = 9
};
int ndsmk_trace(const double *B, const double *G, const int32_t *n3, const double *lo3, const double *h_dq3,
                int nseeds, const double *seeds, double step, int max_steps, int direction, double *ends,
                double *length, double *integral, int32_t *status, int32_t *nsteps);

/* The alpha map (alphamap.hip; semantics: include/ndsm_hip.h, ndsm_hip_vecpot_alpha_map): alpha0 (nx,ny) on the lower
 * face carried along the lines of B (nx,ny,nz,3) to every node, alpha (nx,ny,nz) and status (nx,ny,nz; int32, may be
 * NULL), all DEVICE arrays.  One lane per node (a size_t index: no 2^31 - 1 cap on the nodes), the node is the seed,
 * the line runs against B (polarity +1) or along it (-1) with ndsmk_trace's step rules.  NDSMK_EVALUE for step <= 0,
 * max_steps < 1, a polarity other than +1 / -1.  Asynchronous. */
int ndsmk_alpha_map(const double *B, const int32_t *n3, const double *lo3, const double *h_dq3, const double *alpha0,
                    int polarity, double step, int max_steps, double *alpha, int32_t *status);

/* Squashing factor and line integrals (squash.hip; semantics: include/ndsm_hip.h, ndsm_hip_vecpot_squash).  B, G (G may
 * be NULL: integrals 0) DEVICE arrays (nx,ny,nz,3); integrand 0: G.B/|B|, 1: G.B/|B|^2; seeds (3,nseeds), q (nseeds),
 * ends (3,2 nseeds), length, integral, status, nsteps (2 nseeds: the forward block, then the backward block) DEVICE
 * arrays.  Always both directions.  NDSMK_EVALUE for step <= 0, max_steps < 1, another integrand, nseeds < 0;
 * nseeds == 0 launches nothing.  Asynchronous. */
int ndsmk_squash(const double *B, const double *G, int integrand, const int32_t *n3, const double *lo3,
                 const double *h_dq3, int nseeds, const double *seeds, double step, int max_steps, double *q,
                 double *ends, double *length, double *integral, int32_t *status, int32_t *nsteps);

/* The same with the perpendicular squashing factor (semantics: include/ndsm_hip.h, ndsm_hip_vecpot_squash_perp): qperp
 * (nseeds) a DEVICE array after q; every other argument, check and output as ndsmk_squash, whose bits q, ends, length,
 * integral, status and nsteps hold.  Asynchronous. */
int ndsmk_squash_perp(const double *B, const double *G, int integrand, const int32_t *n3, const double *lo3,
                      const double *h_dq3, int nseeds, const double *seeds, double step, int max_steps, double *q,
                      double *qperp, double *ends, double *length, double *integral, int32_t *status, int32_t *nsteps);

/* Null points (nulls.hip; semantics: include/ndsm_hip.h, ndsm_hip_vecpot_nulls).  B a DEVICE array (nx,ny,nz,3); lo3,
 * h_dq3: first mesh point and spacing per axis.  h_counts2 (HOST, int64): the screen's candidates, the nulls found.  The
 * first min(found, max_nulls) records in ascending cell order go into the DEVICE arrays cell (int64), pos (3 each), jac
 * (9 each), det, resid (doubles), sign, iters (int32); with max_nulls == 0 they are not looked at.  NDSMK_EVALUE for
 * max_nulls < 0.  Blocks for the two counts; the records are written asynchronously. */
int ndsmk_nulls(const double *B, const int32_t *n3, const double *lo3, const double *h_dq3, int max_nulls,
                int64_t *h_counts2, int64_t *cell, double *pos, double *jac, double *det, double *resid, int32_t *sign,
                int32_t *iters);

/* Dips and bald patches (dips.hip; semantics: include/ndsm_hip.h, ndsm_hip_vecpot_dips).  B a DEVICE array (nx,ny,nz,3);
 * lo3, h_dq3: first mesh point and spacing per axis; plane_only 1: the nodes of k = 0 and the edges along x and y only.
 * h_counts3 (HOST, int64): crossings, dips, bald patches, exact whatever max_dips.  The first min(dips, max_dips) records
 * in ascending edge order go into the DEVICE arrays edge (int64), pos, bpt, grad (3 each), curv (doubles), flag (int32);
 * with max_dips == 0 they are not looked at.  NDSMK_EVALUE for max_dips < 0, a plane_only that is not 0 or 1 and a mesh
 * with fewer than 3 nodes on an axis.  Blocks for the three counts; the records are written asynchronously. */
int ndsmk_dips(const double *B, const int32_t *n3, const double *lo3, const double *h_dq3, int plane_only,
               int64_t max_dips, int64_t *h_counts3, int64_t *edge, double *pos, double *bpt, double *grad, double *curv,
               int32_t *flag);

/* Flux partitioning of a magnetogram (partition.hip; semantics: include/ndsm_hip.h, ndsm_hip_partition).  bz (nsx,nsy)
 * and label (nsx,nsy; int32) DEVICE arrays, h_xs, h_ys the mesh vectors on the HOST.  h_counts2 (HOST, int64): the pixels
 * in and the patches K, exact whatever max_patches.  The first min(K, max_patches) rows of the table in ascending root
 * go into the DEVICE arrays root (int64), sign (int32), npix (int64), flux, sx, sy (doubles); with max_patches == 0 they
 * are not looked at and nothing is sorted.  NDSMK_EVALUE for fewer than 2 nodes on an axis, a spacing that is not > 0, a
 * thr that is not finite and >= 0, max_patches < 0.  Blocks for the two counts and, with records, for the copies of the
 * mesh vectors.  ndsmk_partition_fits: 0, or NDSMK_ENODEV when caller_bytes plus the scratch of a call (50 bytes a pixel)
 * pass the device's total memory. */
int ndsmk_partition_fits(const int32_t *nsrc2, double caller_bytes);
int ndsmk_partition(const int32_t *nsrc2, const double *h_xs, const double *h_ys, const double *bz, double thr,
                    int64_t max_patches, int64_t *h_counts2, int32_t *label, int64_t *root, int32_t *sign, int64_t *npix,
                    double *flux, double *sx, double *sy);

/* Patch connectivity (connect.hip; semantics: include/ndsm_hip.h, ndsm_hip_vecpot_connect).  B (nx,ny,nz,3) and label
 * (nx,ny; int32) DEVICE arrays; lo3, h_dq3 as ndsmk_trace's, h_x (nx), h_y (ny) the mesh vectors on the HOST: the seeds
 * are their values.  h_counts2 (HOST, int64): the lines traced and the distinct pairs M, exact whatever max_pairs.  Per
 * pixel into the DEVICE arrays dest (int32), ends (3 each), length, status (int32); the first min(M, max_pairs) pairs in
 * ascending (a, c) into pa, pc (int32), nlines (int64), pflux, not looked at with max_pairs == 0.  NDSMK_EVALUE as
 * ndsmk_trace, and for K < 0 or max_pairs < 0.  Blocks for the two counts; the records are written asynchronously. */
int ndsmk_connect(const double *B, const int32_t *n3, const double *lo3, const double *h_dq3, const double *h_x,
                  const double *h_y, const int32_t *label, int K, double step, int max_steps, int64_t max_pairs,
                  int64_t *h_counts2, int32_t *dest, double *ends, double *length, int32_t *status, int32_t *pa,
                  int32_t *pc, int64_t *nlines, double *pflux);

/* Field-line paths (paths.hip; semantics: include/ndsm_hip.h, ndsm_hip_vecpot_paths), in two halves with the same
 * leading arguments, which are ndsmk_trace's.  ndsmk_paths_count: ndsmk_trace itself (ends, length, integral, status,
 * nsteps are its outputs), then offsets (nl + 1, int64, DEVICE) = the exclusive sums of the lines' point counts for the
 * stride every, offsets[nl] = the total, which also comes back in *h_total (HOST); blocks for it.  ndsmk_paths_fill:
 * slot k < max_points of the concatenation into points (3 each) and, where not NULL, bpt, gpt (3 each) and ipt (gpt,
 * ipt are not looked at without G), all DEVICE arrays; a line writes inside [offsets[l], min(offsets[l + 1],
 * max_points)) only; max_points == 0 launches nothing; asynchronous.  NDSMK_EVALUE as ndsmk_trace, and for every < 1,
 * max_points < 0, by both halves (the counting half takes max_points only to refuse what the filling half would: such a
 * call launches nothing); nseeds == 0 launches nothing (*h_total = 0). */
int ndsmk_paths_count(const double *B, const double *G, const int32_t *n3, const double *lo3, const double *h_dq3,
                      int nseeds, const double *seeds, double step, int max_steps, int direction, int every,
                      int64_t max_points, double *ends, double *length, double *integral, int32_t *status,
                      int32_t *nsteps, int64_t *offsets, int64_t *h_total);
int ndsmk_paths_fill(const double *B, const double *G, const int32_t *n3, const double *lo3, const double *h_dq3,
                     int nseeds, const double *seeds, double step, int max_steps, int direction, int every,
                     int64_t max_points, const int64_t *offsets, double *points, double *bpt, double *gpt, double *ipt);

/* Spine-fan skeleton of the nulls (skeleton.hip; semantics: include/ndsm_hip.h, ndsm_hip_vecpot_skeleton), in two halves
 * as the paths.  B a DEVICE array (nx,ny,nz,3); pos (3,nnulls), jac (9 each, row-major) the records of ndsmk_nulls, ring
 * (2,nring) the coefficients of the fan seeds, all DEVICE arrays; radius and capture in units of min(h).  L = 2 + nring
 * lines per null, nl = nnulls L.  ndsmk_skel_count: the type of every null - kind (nnulls), eig, spine, normal (3 each) -,
 * the seeds and directions of its lanes into the file's own scratch, then the lines: ends (3,nl), length, status,
 * nsteps, hit (nl) and offsets (nl + 1, int64) = the exclusive sums of the lines' point counts for the stride every,
 * offsets[nl] = the total, which also comes back in *h_total (HOST); blocks for it.  ndsmk_skel_fill, after the counting
 * half of the same call: slot k < max_points of the concatenation into points (3 each) and, where not NULL, bpt; a
 * line writes inside [offsets[l], min(offsets[l + 1], max_points)) only; max_points == 0 launches nothing;
 * asynchronous.  NDSMK_EVALUE by both halves for step <= 0, max_steps < 1, nnulls < 0, nring < 0, every < 1, max_points
 * < 0, a radius that is not > 0 or a capture that is < 0 (or not finite); nnulls == 0 launches nothing (*h_total = 0). */
enum { NDSMK_SKEL_CAPTURED = 10, NDSMK_SKEL_NONE = 11 };
int ndsmk_skel_count(const double *B, const int32_t *n3, const double *lo3, const double *h_dq3, int nnulls,
                     const double *pos, const double *jac, int nring, const double *ring, double radius,
                     double capture, double step, int max_steps, int every, int64_t max_points, int32_t *kind,
                     double *eig, double *spine, double *normal, double *ends, double *length, int32_t *status,
                     int32_t *nsteps, int32_t *hit, int64_t *offsets, int64_t *h_total);
int ndsmk_skel_fill(const double *B, const int32_t *n3, const double *lo3, const double *h_dq3, int nnulls,
                    const double *pos, int nring, double radius, double capture, double step, int max_steps, int every,
                    int64_t max_points, const int64_t *offsets, double *points, double *bpt);

/* Separator lines (separators.hip; semantics: include/ndsm_hip.h, ndsm_hip_vecpot_separators), in two halves as the
 * skeleton.  B a DEVICE array (nx,ny,nz,3); pos (3,nnulls), kind (nnulls), normal (3,nnulls) the skeleton's arrays of the
 * nulls, pair (2,nbr; int32) the nulls (m, m') and arc (4,nbr) the ring coefficients (c_a, s_a, c_b, s_b) of every
 * bracket, all DEVICE arrays; radius and capture in units of min(h).  ndsmk_sep_count: the pair indices are checked on the
 * device (blocks for the answer), then one wave per bracket refines it in up to `rounds` rounds - state, nrounds, side
 * (nbr; int32), coef (4,nbr), width (nbr), dmin (2,nbr) -, the seed and direction of each bracket's line go into the file's
 * own scratch, then the lines: ends (3,nbr), length, status, nsteps (nbr) and offsets (nbr + 1, int64) = the exclusive
 * sums of the lines' point counts for the stride every, offsets[nbr] = the total, which also comes back in *h_total
 * (HOST); blocks for it.  ndsmk_sep_fill, after the counting half of the same call: slot k < max_points of the
 * concatenation into points (3 each) and, where not NULL, bpt; a line writes inside [offsets[l], min(offsets[l + 1],
 * max_points)) only; max_points == 0 launches nothing; asynchronous.  NDSMK_EVALUE by both halves for step <= 0,
 * max_steps < 1, nnulls < 0, nbr < 0, rounds < 1, every < 1, max_points < 0, a radius or a capture that is not > 0, a tol
 * that is < 0 (or not finite), and by the counting half for a pair index outside 0 .. nnulls - 1 (nothing is written);
 * nbr == 0 launches nothing (*h_total = 0). */
int ndsmk_sep_count(const double *B, const int32_t *n3, const double *lo3, const double *h_dq3, int nnulls,
                    const double *pos, const int32_t *kind, const double *normal, int nbr, const int32_t *pair,
                    const double *arc, double radius, double capture, double step, int max_steps, int rounds,
                    double tol, int every, int64_t max_points, int32_t *state, int32_t *nrounds, double *coef,
                    double *width, int32_t *side, double *dmin, double *ends, double *length, int32_t *status,
                    int32_t *nsteps, int64_t *offsets, int64_t *h_total);
int ndsmk_sep_fill(const double *B, const int32_t *n3, const double *lo3, const double *h_dq3, int nnulls,
                   const double *pos, int nbr, const int32_t *pair, double radius, double capture, double step,
                   int max_steps, int rounds, double tol, int every, int64_t max_points, const int64_t *offsets,
                   double *points, double *bpt);

/* the face phase on the device (faces.hip): packed face buffers, six faces back to back */
int ndsmk_face_offsets(const int32_t *n3, int64_t *off6, int64_t *total);
int ndsmk_face_extract(const double *B, const int32_t *n3, double *faces);
int ndsmk_face_flux(const double *faces, const int32_t *n3, double h1h2, double *d_phi6);
int ndsmk_face_rhs(const double *faces, const int32_t *n3, int f, const double *d_phi6, double area, double *rhs);
int ndsmk_face_write(double *u, const int32_t *n3, const double *chi, int f, int c, double fac);
int ndsmk_face_put(double *u, const int32_t *n3, int f, const double *vals);

/* level-1 form for the V-cycle driver: three buffers (u on entry + two spares), `keep` (one of them
 * or NULL) is never written, *where = 0/1/2 names the buffer holding the result.  r: residual of the
 * result (may be NULL).  prev: have the launch of the last sweep evaluate max / sum |u_new - prev|
 * (*met_done = 1 if it did; ndsmk_fetch_fused_metric reads the pair, blocking). */
int ndsmk_relax3(const ndsmk_grid *g, double *u, double *a, double *b, const double *keep, const double *rhs,
                 int nsweeps, double *r, const double *prev, int *where, int *met_done,
                 const ndsmk_xfer *px /* != NULL: u += P uc first */, const double *uc);
int ndsmk_fetch_fused_metric(double *h_out2);

/* pieces of an overlapped z-slab pass: one fused pass over owned planes [z0, z1) only (u -> uout) */
int ndsmk_fused_window(const ndsmk_grid *g, const double *u, double *uout, const double *rhs, int nsweeps, int z0,
                       int z1, const ndsmk_xfer *px, const double *uc, const double *prev, int accumulate);
int ndsmk_fused_window_res(const ndsmk_grid *g, const double *u, double *uout, const double *rhs, double *rout, int z0,
                           int z1);
int ndsmk_fused_metric_ok(const ndsmk_grid *g);
int ndsmk_fused_prolong_ok(const ndsmk_grid *g, const double *rhs, int nsweeps);
/* two streams: 1 = later copies / RCCL calls go to the communication stream, 0 = main stream again;
 * fence(from, to): work enqueued on `from` so far precedes work enqueued on `to` from now on */
#define NDSMK_LANES 6
int ndsmk_select_lane(int lane);           /* -1: main stream */
int ndsmk_lane_fence(int lane, int to_main);
int ndsmk_lane_idle(int lane);   /* 1: the lane's stream has drained, 0: not yet (never blocks), < 0: error */
int ndsmk_lane_sync(int lane);
int ndsmk_capture_begin(void);             /* record what is enqueued on the selected lane ... */
int ndsmk_capture_end(void **exec);        /* ... into an executable graph */
int ndsmk_graph_launch(void *exec);        /* replay it on the selected lane / stream */
int ndsmk_graph_destroy(void *exec);
int ndsmk_select_stream(int which);
int ndsmk_stream_fence(int from, int to);

/* ---- mixed-precision mode (mixed.hip): level 1 as iterative refinement, correction in fp32 ---- */
/* unew = u + e ; ezero = 0 ; r = (float)(rhs - L unew) ; h_out2 = (max|e|, sum|e|), blocking.
 * e == NULL: r = residual of u, nothing else written.  rhs == NULL: zero right-hand side. */
int ndsmk_update_residual_f32(const ndsmk_grid *g, const double *u, double *unew, const double *rhs, const float *e,
                              float *ezero, float *r, double *h_out2);
/* nsweeps fp32 sweeps of L e = r (fused kernel only); r_out != NULL: residual of the swept equation */
int ndsmk_relax_f32(const ndsmk_grid *g, float *e, float *ealt, const float *r, int nsweeps, int force, float *r_out,
                    int *result_in_alt);
int ndsmk_restrict_f32(const ndsmk_xfer *x, const float *r_f, double *rhs_c, double *u_c);
int ndsmk_prolong_add_f32(const ndsmk_xfer *x, const double *u_c, float *e_f);

/* tests / tuning: the five values of NDSM_FUSED_CFG (smooth_fused.hip) at run time */
int ndsmk_debug_fused_cfg(int two, int one, int res, int work_items, int big);
/* the plan of a relax call / the z chunking of a fused launch, on the host (smooth.hip has the array layouts) */
int ndsmk_debug_relax_plan(int what, const int32_t *grid, const int64_t *req, const int64_t *knobs, int cap, int32_t *out);

#ifdef __cplusplus
}
#endif
#endif
