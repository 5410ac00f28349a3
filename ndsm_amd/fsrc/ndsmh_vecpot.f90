! libndsm_hip - physics driver around the device multigrid solver: current-free
! B = curl A in a box from B.n on its six faces.
!
! Reference being replaced: compute_vector_potential and its helpers,
! ndsm_vector_potential.f90:130-497 (+ :598-691 solve, :699-743 extract_bn,
! :759-872 curl/derivq, :880-950 add_flux_balance_fields, :977-1031
! compute_At_bcs, :1070-1106 trapz_2D).  Pipeline per call:
!   1. B.n on the six faces, face fluxes (trapezoid)               host, O(N^2/3)
!   2. six 2-D all-Neumann Poisson solves  laplace(chi) = B.n - mean DEVICE (mg_solve, ndim=2)
!   3. tangential Dirichlet data A_t = -grad(chi) x n              host, O(N^2/3)
!   4. three 3-D Laplace solves Ax, Ay, Az (the hot path)          DEVICE (mg_solve, ndim=3)
!   5. analytic flux-balance fields, B = curl A                    DEVICE (post.hip)
! Steps 1 and 3 touch only the six faces (O(N^2/3) points) and stay on the host;
! every Poisson solve and all O(N) work runs on the GPU, and A, B are
! downloaded once at the end.
!
! Quirks of the reference kept on purpose (SURVEY 8a):
!   Q2  the Az solve always uses ms = 5                 (:685)
!   Q3' the returned ierr is the flag of the LAST 2-D face solve: `solve` keeps
!       the 3-D flags in a local (:613) and :480 stores the variable last set
!       at :360.  The 3-D flags are reported additively in iopt slot 8.
!   Q4  face fluxes always use dq(1)*dq(2); grad(chi) uses the NORMAL spacing
!       (:301-305, :394-398) - exact only for dx = dy = dz.
module ndsmh_vecpot

  use, intrinsic :: iso_c_binding
  use, intrinsic :: iso_fortran_env, only: error_unit, int64
  use ndsmh_iface
  use ndsmh_mg
  implicit none
  private

  public :: vecpot_solve, poisson_solve
  public :: vecpot_ctx, vecpot_ctx_create, vecpot_ctx_destroy, vecpot_ctx_matches, vecpot_run, vecpot_cache_drop
  public :: vecpot_alpha_map, vecpot_nlfff, nlfff_args, vecpot_optimize, optimize_args, vecpot_preprocess, preprocess_args
  public :: vecpot_optimize_cascade, vecpot_ref, vecpot_optimize_obs, descent_ctl
  public :: vecpot_project, vecpot_devore, vecpot_lines, vecpot_paths, vecpot_nulls, vecpot_skeleton, vecpot_separators
  public :: vecpot_dips
  public :: vecpot_connect
  public :: VP_POTENTIAL, VP_FIELD, VP_HELICITY, VP_CURRENT, VP_NLFFF
  ! pieces the distributed driver (ndsmh_wvecpot) shares with vecpot_solve
  public :: face_data, face_axis, face_upper, face_t1, face_t2, face_order, face_copy, vecpot_faces, say
  public :: OPT_LEN, IOPT_MS, IOPT_NCYCLES, IOPT_FACE1, IOPT_IERR, IOPT_FLXCRL, IOPT_DEBUG, IOPT_DUMAX, &
            IOPT_NMAXEX, IOPT_FAIL3D, IOPT_NGRIDS, IOPT_NCYC_OUT, IOPT_PREC, ROPT_VTOL, ROPT_CTOL, ROPT_TIM, ROPT_DULAST
  public :: verbose

  ! option slots, 0-based like the reference (ndsm_vector_potential.f90:40-57)
  integer, parameter :: OPT_LEN = 16
  integer, parameter :: IOPT_MS = 0, IOPT_NCYCLES = 1, IOPT_FACE1 = 2, IOPT_IERR = 3, IOPT_FLXCRL = 4, &
                        IOPT_DEBUG = 5, IOPT_DUMAX = 6, IOPT_NMAXEX = 7
  ! additive slots (unused = 0 in the reference, so 0 keeps its behaviour)
  integer, parameter :: IOPT_FAIL3D = 8     ! out: bit c-1 set if 3-D solve c missed vc_tol
  integer, parameter :: IOPT_NGRIDS = 9     ! in : cap on the number of grid levels (0 = reference rule)
  integer, parameter :: IOPT_NCYC_OUT = 10  ! out: V-cycles used by the last 3-D solve that iterated
  integer, parameter :: IOPT_PREC = 11      ! in : 0 fp64 throughout (reference arithmetic), 1 mixed precision for the
                                            !      3-D solves (fp64 residual, fp32 correction V-cycle on level 1)
  integer, parameter :: ROPT_VTOL = 0, ROPT_CTOL = 1, ROPT_TIM = 2
  integer, parameter :: ROPT_DULAST = 3     ! out: du of the last V-cycle of the last 3-D solve

  logical, save :: verbose = .false.

  ! geometry of the six faces: normal axis, layer side, tangential axes
  integer, parameter :: face_axis(6) = [1, 1, 2, 2, 3, 3]
  logical, parameter :: face_upper(6) = [.false., .true., .false., .true., .false., .true.]
  integer, parameter :: face_t1(6) = [2, 2, 1, 1, 1, 1]
  integer, parameter :: face_t2(6) = [3, 3, 3, 3, 2, 2]
  ! A_t = -grad(chi) x n projected on (t1, t2):  (s1*dchi/dt2, s2*dchi/dt1)
  real(wp), parameter :: at_s1(6) = [-1, -1, +1, +1, -1, -1]
  real(wp), parameter :: at_s2(6) = [+1, +1, -1, -1, +1, +1]

  ! the four faces that carry tangential data of component c, in the order the reference writes them
  ! (:647-650, :663-666, :679-682; later writes win on shared edges)
  integer, parameter :: face_order(4, 3) = reshape([3, 4, 5, 6, 1, 2, 5, 6, 1, 2, 3, 4], [4, 3])

  ! what vecpot_run computes (DESIGN.md "Vector potential of a current-carrying field"):
  !   VP_POTENTIAL  the reference pipeline: the potential field of B.n and its A_p (ndsm_vector_solve)
  !   VP_FIELD      A of the whole field B: the 3-D problems get rhs_c = -(curl B)_c, same letters and data
  !   VP_HELICITY   one face phase, then the potential and the field 3-D phases, then the helicity reduction
  !   VP_CURRENT    A for a current J the caller prescribes: the 3-D problems get rhs_c = -J_c; B supplies B.n only
  !   VP_NLFFF      the Grad-Rubin iteration (DESIGN.md "Nonlinear force-free field"): one face phase, then per pass
  !                 the alpha map of B^k, the 3-D phase with rhs_c = -(alpha B^k_c) and the post phase -> B^{k+1}
  integer, parameter :: VP_POTENTIAL = 0, VP_FIELD = 1, VP_HELICITY = 2, VP_CURRENT = 3, VP_NLFFF = 4

  ! up to this many points the three 3-D component solves get a hierarchy each and run side by side (vecpot_run)
  integer(ik), parameter :: SIDE3D_MAX = 16_ik * 1024_ik * 1024_ik

  type :: face_data
    integer :: n1 = 0, n2 = 0
    real(wp), allocatable :: bn(:, :), chi(:, :), at1(:, :), at2(:, :)
  end type

  ! grid-bound state of the pipeline, reused across calls (vecpot_ctx_create)
  type :: vecpot_ctx
    logical :: live = .false.
    integer(c_int32_t) :: n3(3) = 0
    integer :: ngr = 0
    real(wp), allocatable :: qx(:), qy(:), qz(:)
    type(mg_solver) :: s3v(3), s2(6)        ! one 2-D hierarchy per face: the six face solves run side by side;
                                            ! s3v(1): the 3-D hierarchy; s3v(2:3): small grids only, where the three
                                            ! component solves run side by side as well (live3x)
    logical :: live3 = .false., live3x = .false., live2(6) = .false.
    type(c_ptr) :: dA = c_null_ptr, dB = c_null_ptr, dmesh = c_null_ptr
    type(c_ptr) :: dbn = c_null_ptr, dchi = c_null_ptr, dphi = c_null_ptr   ! packed faces: B.n, chi; six fluxes
    type(c_ptr) :: hbn = c_null_ptr                                         ! pinned staging of the six faces
    type(c_ptr) :: dF(3) = c_null_ptr       ! host-array helicity calls only: B, A_p, B_p (allocated at the first)
    type(mg_solver) :: sp                   ! the 3-D all-Neumann hierarchy of vecpot_project (created at the first)
    logical :: livep = .false.
    integer(ik) :: foff(6) = 0, ftotal = 0
  end type

  ! what a Grad-Rubin call takes besides A and B (vecpot_run, mode VP_NLFFF): alpha0 (nx,ny) in, alpha (nx,ny,nz) and
  ! status (nx,ny,nz; int32; may be c_null_ptr) out, DEVICE arrays; hist (4,niter_max) on the HOST; niter out
  type :: nlfff_args
    type(c_ptr) :: alpha0 = c_null_ptr, alpha = c_null_ptr, status = c_null_ptr, hist = c_null_ptr
    integer(c_int) :: polarity = 1, start = 0, niter_max = 1, max_steps = 1
    real(wp) :: tol = 0, step = 0.5_wp
    integer(c_int) :: niter = 0
  end type

  ! what every descent call takes (descent_open .. descent_close): at most niter_max tries, a look at L every check
  ! tries, the stop rule's tol, the first step and the smallest; hist (width,hist_rows) on the HOST; info out: rows
  ! written, tries, stop reason (0 niter_max, 1 tol, 2 dt_min)
  type :: descent_ctl
    type(c_ptr) :: hist = c_null_ptr
    integer(c_int) :: niter_max = 1, check = 1, hist_rows = 2
    real(wp) :: tol = 0, dt0 = 0, dt_min = 0
    integer(c_int) :: info(3) = 0
  end type

  ! what an optimization-method call takes besides B (vecpot_optimize): w (nx,ny,nz) in, on the side B is on, may be
  ! c_null_ptr (1 everywhere); hist rows have 6 entries.  With bobs the call has a measurement term and a freed lower
  ! face: bobs (nx,ny,3) in, the observation on the k = 0 plane, and wm (nx,ny,3) in, its per-component confidence, may
  ! be c_null_ptr (1 everywhere), both on the side B is on; nu the weight of L_m in L; free 1: the lower face moves, 0:
  ! it is held; hist rows then have 7 entries
  type, extends(descent_ctl) :: optimize_args
    type(c_ptr) :: w = c_null_ptr, bobs = c_null_ptr, wm = c_null_ptr
    integer(c_int) :: start = 0, free = 1
    real(wp) :: nu = 0
  end type

  ! one level of a cascade (vecpot_optimize_cascade): a context somebody else owns
  type :: vecpot_ref
    type(vecpot_ctx), pointer :: p => null()
  end type

  ! what a preprocessing call takes besides B (vecpot_preprocess): obs (nx,ny,3) in, on the side B is on, may be
  ! c_null_ptr (the input B is the observation); mu = mu1, mu2, mu3h, mu3z, mu4; hist rows have 17 entries
  type, extends(descent_ctl) :: preprocess_args
    type(c_ptr) :: obs = c_null_ptr
    real(wp) :: mu(5) = 0
  end type

  ! the check loop of a descent between descent_open and descent_close: the state row as the device holds it - a
  ! history row of `width` doubles, then the index of the current buffer and the stop flag (descent.hpp's DescentState)
  integer, parameter :: DESCENT_ROW_MAX = 21
  type :: descent_loop
    real(wp) :: row(DESCENT_ROW_MAX) = 0  ! the caller's ndsmk_*_row reads into it
    integer(c_int) :: n = 0               ! the tries of the interval to queue next (descent_more)
    integer :: width = 0
    integer(c_int) :: rows = 0, tries = 0
    real(wp) :: lprev = 0
    real(wp), pointer :: hh(:, :) => null()
  end type

  ! one array of a host-array line entry in its staging buffer (carve, fetch)
  type :: slice
    type(c_ptr) :: host                     ! the caller's array; c_null_ptr: absent, dev stays c_null_ptr
    integer(c_size_t) :: width, count       ! bytes per entry, entries
    logical :: home                         ! COMES_HOME: an output; GOES_UP: an input
    type(c_ptr) :: dev = c_null_ptr         ! its place on the device
  end type
  logical, parameter :: GOES_UP = .false., COMES_HOME = .true.

  type(vecpot_ctx), save, target :: cache
  logical, save :: cache_busy = .false.     ! ndsm_vector_solve is running on the cached context

contains

  ! debug trace in the reference's format, plus (NDSM_HIP_TIMING set) the wall time since the
  ! previous message - the device is drained first, so the figure belongs to the finished phase
  subroutine say(where, what)
    character(len=*), intent(in) :: where, what
    integer(int64) :: c, r
    real(wp) :: t
    integer :: st, rc
    logical, save :: first = .true., timing = .false.
    real(wp), save :: t_last = 0
    if (first) then
      call get_environment_variable("NDSM_HIP_TIMING", status=st)
      timing = (st == 0)
      first = .false.
    end if
    if (timing) then
      rc = ndsmk_sync()
      call system_clock(c, r)
      t = real(c, wp) / real(r, wp)
      write (error_unit, '(A,F12.6,A)') "TIMING(+", t - t_last, " s) before: "//what
      t_last = t
    end if
    if (verbose) write (error_unit, '(A)') "DEBUG("//where//"):"//what
  end subroutine

  ! ------------------------------------------------------------------
  ! Scalar Poisson problem on the device (host buffers in and out).
  ! u: initial guess incl. Dirichlet face data on entry, solution on exit.
  ! h_rhs = c_null_ptr means rhs == 0.
  ! ------------------------------------------------------------------
  function poisson_solve(ndim, nshape, qx, qy, qz, bcs, ms, ex_tol, use_max, nmax_exact, ngrids_req, &
                         vc_tol, nmax, h_u, h_rhs, du_last, ncycles, ierr, hist, precision) result(rc)
    integer, intent(in) :: ndim, ms, nmax_exact, ngrids_req, nmax
    integer, intent(in), optional :: precision
    integer(c_int32_t), intent(in) :: nshape(3)
    real(wp), intent(in) :: qx(:), qy(:), qz(:)
    character(len=1), intent(in) :: bcs(:)
    real(wp), intent(in) :: ex_tol, vc_tol
    logical, intent(in) :: use_max
    type(c_ptr), intent(in) :: h_u, h_rhs
    real(wp), intent(out) :: du_last
    integer, intent(out) :: ncycles, ierr
    real(wp), intent(inout), optional :: hist(:)
    integer(c_int) :: rc
    type(mg_solver) :: s
    integer(ik) :: sweeps, bad

    ierr = 1; ncycles = 0; du_last = huge(du_last)
    rc = mg_create(s, ndim, nshape, qx, qy, qz, bcs, ngrids_req)
    if (rc == 0) then
      s%ms = ms; s%ex_tol = ex_tol; s%use_max = use_max; s%nmax_exact = nmax_exact
      if (present(precision)) s%precision = precision
      rc = mg_set_u(s, h_u)
    end if
    if (rc == 0) then
      if (c_associated(h_rhs)) then
        rc = mg_set_rhs(s, h_rhs)
      else
        rc = mg_zero_rhs(s)
      end if
    end if
    if (rc == 0) rc = mg_solve(s, vc_tol, nmax, du_last, ncycles, ierr, hist)
    if (rc == 0) rc = mg_get_u(s, h_u)
    if (rc == 0) then
      if (ierr /= 0) print *, "Warning: IOPT_NCYCLES exceeded. V-cycle iteration may not have converged"
      rc = mg_read_info(s, sweeps, bad)
      if (rc == 0 .and. bad > 0) &
        print *, "Warning: IOPT_NMAXEX exceeded. Coarse-mesh solution may not have converged"
    end if
    call mg_destroy(s)
  end function

  ! ------------------------------------------------------------------
  ! Steps 1b-3 of the pipeline, on whole faces: fluxes of fc(:)%bn (:283-306), the six 2-D
  ! all-Neumann solves on the device (:338-365) and the tangential data A_t = -grad(chi) x n
  ! (:387-399, :977-1031).  In: fc(f)%bn (allocated with chi, at1, at2).  Out: phi, fc(f)%at1/at2,
  ! ierr2d = flag of the LAST face solve (Q3').
  ! ------------------------------------------------------------------
  function vecpot_faces(iopt, ropt, qx, qy, qz, dq, span, fc, phi, ierr2d) result(rc)
    integer(ik), intent(in) :: iopt(0:OPT_LEN - 1)
    real(wp), intent(in) :: ropt(0:OPT_LEN - 1)
    real(wp), intent(in), target :: qx(:), qy(:), qz(:)
    real(wp), intent(in) :: dq(3), span(3)
    type(face_data), intent(inout), target :: fc(6)
    real(wp), intent(out) :: phi(6)
    integer, intent(out) :: ierr2d
    integer(c_int) :: rc
    character(len=*), parameter :: me = "compute_vector_potential"
    type(mg_solver) :: s2(6)
    real(wp) :: area(6), du6(6), fac
    integer :: f, i, j, ncyc6(6), ierr6(6), st
    integer(ik) :: sweeps, bad
    integer(c_int32_t) :: fshape(3)
    logical :: live2(6)
    character(len=1) :: bc2(4)
    character(len=8) :: envbuf
    real(wp), pointer :: qa(:), qb(:)

    rc = 0
    live2 = .false.
    do f = 1, 6
      phi(f) = trapezoid(fc(f)%bn, dq(1), dq(2))            ! Q4
    end do
    area = [span(2) * span(3), span(2) * span(3), span(1) * span(3), span(1) * span(3), &
            span(1) * span(2), span(1) * span(2)]

    ! ---- 2. chi on every face: 2-D all-Neumann solves on the device ---
    call say(me, "Solve BVP on each boundary...")
    ! (one hierarchy per face, the six solves side by side: mg_solve_lanes, as in vecpot_run)
    ierr2d = 0
    bc2 = 'N'
    do f = 1, 6
      qa => axis_mesh(face_t1(f)); qb => axis_mesh(face_t2(f))
      fshape = [int(fc(f)%n1, c_int32_t), int(fc(f)%n2, c_int32_t), 1_c_int32_t]
      rc = mg_create(s2(f), 2, fshape, qa, qb, qb, bc2, int(iopt(IOPT_NGRIDS))); live2(f) = .true.
      if (rc /= 0) goto 900
      s2(f)%ms = max(0, int(iopt(IOPT_MS))); s2(f)%ex_tol = ropt(ROPT_CTOL); s2(f)%use_max = (iopt(IOPT_DUMAX) == 1)
      s2(f)%nmax_exact = max(0, int(iopt(IOPT_NMAXEX)))
      fc(f)%chi = 0
      fc(f)%bn = fc(f)%bn - phi(f) / area(f)
      rc = mg_set_u(s2(f), c_loc(fc(f)%chi)); if (rc /= 0) goto 900
      rc = mg_set_rhs(s2(f), c_loc(fc(f)%bn)); if (rc /= 0) goto 900
      rc = mg_reset_info(s2(f)); if (rc /= 0) goto 900
    end do
    call get_environment_variable("NDSM_HIP_FACE_LANES", envbuf, status=st)
    if (st == 0 .and. envbuf(1:1) == "0") then
      do f = 1, 6
        rc = mg_solve(s2(f), ropt(ROPT_VTOL), int(iopt(IOPT_NCYCLES)), du6(f), ncyc6(f), ierr6(f))
        if (rc /= 0) goto 900
      end do
    else
      rc = mg_solve_lanes(s2, ropt(ROPT_VTOL), int(iopt(IOPT_NCYCLES)), du6, ncyc6, ierr6)
      if (rc /= 0) goto 900
    end if
    do f = 1, 6
      rc = mg_get_u(s2(f), c_loc(fc(f)%chi)); if (rc /= 0) goto 900
      ierr2d = ierr6(f)
      if (ierr2d /= 0) print *, "Warning: IOPT_NCYCLES exceeded. V-cycle iteration may not have converged"
      if (mg_read_info(s2(f), sweeps, bad) == 0) then
        if (bad > 0) print *, "Warning: IOPT_NMAXEX exceeded. Coarse-mesh solution may not have converged"
      end if
      call mg_destroy(s2(f)); live2(f) = .false.
    end do

    ! ---- 3. A_t = -grad(chi) x n --------------------------------------
    call say(me, "Compute vector potential boundary conditions...")
    do f = 1, 6
      fac = 1.0_wp / (2.0_wp * dq(face_axis(f)))            ! Q4: the normal spacing
      do j = 1, fc(f)%n2
        do i = 1, fc(f)%n1
          call tangential(fc(f), f, i, j, fac)
        end do
      end do
    end do

900 continue
    do f = 1, 6
      if (live2(f)) call mg_destroy(s2(f))
    end do

  contains

    function axis_mesh(k) result(q)
      integer, intent(in) :: k
      real(wp), pointer :: q(:)
      select case (k)
      case (1); q => qx
      case (2); q => qy
      case default
        q => qz
      end select
    end function

  end function

  ! ------------------------------------------------------------------
  ! Persistent state of the pipeline (SURVEY 8f-4): everything that depends on the grid only -
  ! the 3-D hierarchy with its transfer tables, the three 2-D face hierarchies, device arrays for
  ! A, B, the mesh and the six faces, a pinned staging buffer - created once and reused by every
  ! later call on the same (shape, mesh, level cap).  The reference builds and frees all of it per
  ! component and per call (ndsm_vector_potential.f90:652-689, ndsm_multigrid_core.f90:165-329).
  ! ------------------------------------------------------------------
  function vecpot_ctx_matches(ctx, n3, qx, qy, qz, ngr) result(same)
    type(vecpot_ctx), intent(in) :: ctx
    integer(c_int32_t), intent(in) :: n3(3)
    real(wp), intent(in) :: qx(:), qy(:), qz(:)
    integer, intent(in) :: ngr
    logical :: same
    same = .false.
    if (.not. ctx%live) return
    if (any(ctx%n3 /= n3) .or. ctx%ngr /= ngr) return
    if (size(ctx%qx) /= size(qx) .or. size(ctx%qy) /= size(qy) .or. size(ctx%qz) /= size(qz)) return
    same = all(ctx%qx == qx) .and. all(ctx%qy == qy) .and. all(ctx%qz == qz)
  end function

  subroutine vecpot_ctx_destroy(ctx)
    type(vecpot_ctx), intent(inout) :: ctx
    integer :: p
    integer(c_int) :: rc
    ! (no transfer of this context is in flight here: vecpot_run drains its own before it returns, whatever its
    ! outcome - and draining here would void the tickets of ANOTHER context's running call when the low-memory
    ! hook evicts the cached one from inside it)
    if (ctx%live3) call mg_destroy(ctx%s3v(1))
    if (ctx%live3x) then
      call mg_destroy(ctx%s3v(2)); call mg_destroy(ctx%s3v(3))
    end if
    ctx%live3 = .false.; ctx%live3x = .false.
    if (ctx%livep) call mg_destroy(ctx%sp)
    ctx%livep = .false.
    do p = 1, 6
      if (ctx%live2(p)) call mg_destroy(ctx%s2(p))
      ctx%live2(p) = .false.
    end do
    rc = ndsmk_free(ctx%dA); ctx%dA = c_null_ptr
    rc = ndsmk_free(ctx%dB); ctx%dB = c_null_ptr
    do p = 1, 3
      rc = ndsmk_free(ctx%dF(p)); ctx%dF(p) = c_null_ptr
    end do
    rc = ndsmk_free(ctx%dmesh); ctx%dmesh = c_null_ptr
    rc = ndsmk_free(ctx%dbn); ctx%dbn = c_null_ptr
    rc = ndsmk_free(ctx%dchi); ctx%dchi = c_null_ptr
    rc = ndsmk_free(ctx%dphi); ctx%dphi = c_null_ptr
    rc = ndsmk_host_free(ctx%hbn); ctx%hbn = c_null_ptr
    if (allocated(ctx%qx)) deallocate (ctx%qx, ctx%qy, ctx%qz)
    ctx%live = .false.
  end subroutine

  ! the grid-only part: mesh copies, face buffers, the three 2-D hierarchies
  function vecpot_ctx_create(ctx, n3, qx, qy, qz, ngr) result(rc)
    type(vecpot_ctx), intent(inout), target :: ctx
    integer(c_int32_t), intent(in) :: n3(3)
    real(wp), intent(in) :: qx(:), qy(:), qz(:)
    integer, intent(in) :: ngr
    integer(c_int) :: rc
    integer :: pair, f
    integer(c_int32_t) :: fshape(3)
    integer(c_size_t) :: off_y, off_z
    character(len=1) :: bc2(4)
    real(wp), pointer :: qa(:), qb(:)

    call vecpot_ctx_destroy(ctx)
    rc = ndsmk_init(-1_c_int); if (rc /= 0) return
    ctx%n3 = n3; ctx%ngr = ngr
    allocate (ctx%qx(n3(1)), ctx%qy(n3(2)), ctx%qz(n3(3)))
    ctx%qx = qx(1:n3(1)); ctx%qy = qy(1:n3(2)); ctx%qz = qz(1:n3(3))
    ctx%live = .true.
    rc = ndsmk_face_offsets(n3, ctx%foff, ctx%ftotal); if (rc /= 0) return
    rc = ndsmk_alloc(ctx%dbn, int(ctx%ftotal, c_size_t) * 8_c_size_t); if (rc /= 0) return
    rc = ndsmk_alloc(ctx%dchi, int(ctx%ftotal, c_size_t) * 8_c_size_t); if (rc /= 0) return
    rc = ndsmk_alloc(ctx%dphi, 64_c_size_t); if (rc /= 0) return
    rc = ndsmk_host_alloc(ctx%hbn, int(ctx%ftotal + 8, c_size_t) * 8_c_size_t); if (rc /= 0) return
    off_y = int(n3(1), c_size_t) * 8_c_size_t
    off_z = off_y + int(n3(2), c_size_t) * 8_c_size_t
    rc = ndsmk_alloc(ctx%dmesh, off_z + int(n3(3), c_size_t) * 8_c_size_t); if (rc /= 0) return
    rc = ndsmk_h2d(ctx%dmesh, c_loc(ctx%qx), int(n3(1), c_size_t) * 8_c_size_t); if (rc /= 0) return
    rc = ndsmk_h2d(dptr_offset(ctx%dmesh, off_y), c_loc(ctx%qy), int(n3(2), c_size_t) * 8_c_size_t); if (rc /= 0) return
    rc = ndsmk_h2d(dptr_offset(ctx%dmesh, off_z), c_loc(ctx%qz), int(n3(3), c_size_t) * 8_c_size_t); if (rc /= 0) return
    bc2 = 'N'
    do f = 1, 6
      qa => ctx_axis(ctx, face_t1(f)); qb => ctx_axis(ctx, face_t2(f))
      fshape = [n3(face_t1(f)), n3(face_t2(f)), 1_c_int32_t]
      rc = mg_create(ctx%s2(f), 2, fshape, qa, qb, qb, bc2, ngr); ctx%live2(f) = .true.
      if (rc /= 0) return
    end do
  end function

  function ctx_axis(ctx, k) result(q)
    type(vecpot_ctx), intent(in), target :: ctx
    integer, intent(in) :: k
    real(wp), pointer :: q(:)
    select case (k)
    case (1); q => ctx%qx
    case (2); q => ctx%qy
    case default
      q => ctx%qz
    end select
  end function

  ! the library's own context behind ndsm_vector_solve (the reference ABI has no handle: SURVEY 8b
  ! "Ownership" - an internal cache keyed by shape and mesh is invisible to the caller); dropped by
  ! ndsm_hip_shutdown / a re-target of the runtime
  subroutine vecpot_cache_drop() bind(c)
    call vecpot_ctx_destroy(cache)
  end subroutine

  ! a device allocation somewhere in the library has failed: the cached context (13 GiB at 512^3) is only a
  ! convenience - give it back, unless ndsm_vector_solve is using it right now
  subroutine vecpot_cache_evict() bind(c)
    if (.not. cache%live .or. cache_busy) return
    call vecpot_ctx_destroy(cache)
  end subroutine

  function vecpot_solve(n3, iopt, ropt, qx, qy, qz, A, B) result(rc)
    integer(c_int32_t), intent(in) :: n3(3)
    integer(ik), intent(inout) :: iopt(0:OPT_LEN - 1)
    real(wp), intent(inout) :: ropt(0:OPT_LEN - 1)
    real(wp), intent(in), target :: qx(:), qy(:), qz(:)
    real(wp), intent(inout), target, contiguous :: A(:, :, :, :), B(:, :, :, :)
    integer(c_int) :: rc
    integer :: st
    if (any(n3 < 2)) then              ! :213-216 the reference's only input check
      iopt(IOPT_FAIL3D) = 0
      iopt(IOPT_IERR) = 1
      rc = 0
      return
    end if
    cache_busy = .true.      ! (an allocation failure below must not evict the context that is being built / used)
    call get_environment_variable("NDSM_HIP_NO_CACHE", status=st)      ! A/B testing: rebuild everything per call
    if (st == 0) call vecpot_ctx_destroy(cache)
    if (.not. vecpot_ctx_matches(cache, n3, qx, qy, qz, int(iopt(IOPT_NGRIDS)))) then
      rc = vecpot_ctx_create(cache, n3, qx, qy, qz, int(iopt(IOPT_NGRIDS)))
      if (rc /= 0) then
        call vecpot_ctx_destroy(cache)
        cache_busy = .false.
        return
      end if
      call ndsmk_at_reset(c_funloc(vecpot_cache_drop))
      call ndsmk_on_low_memory(c_funloc(vecpot_cache_evict))
    end if
    rc = vecpot_run(cache, iopt, ropt, c_loc(A), c_loc(B), .false.)
    cache_busy = .false.
    if (rc /= 0 .or. st == 0) call vecpot_ctx_destroy(cache)    ! after an error nothing is assumed about the device state
  end function

  ! ------------------------------------------------------------------
  ! The whole ndsm_vector_solve pipeline on a prepared context.  A, B: (nx,ny,nz,3), on the HOST
  ! (on_device = .false.: the reference ABI) or in HBM (on_device: the additive device-resident entry).
  !
  !   host entry  : B.n of the six faces is gathered on the host into pinned memory (the only part of B
  !                 that is ever read) and uploaded once, 8 N^(2/3) bytes; a worker thread checks the
  !                 initial guess and uploads only components that are not all zero; every finished
  !                 component of A is downloaded behind the next component's solve; B follows the curl.
  !   device entry: B.n is extracted by a kernel; nothing crosses PCIe but the six fluxes and the
  !                 16-byte convergence read-backs.
  ! Between the face upload and the downloads nothing else travels: fluxes, right-hand sides of the 2-D
  ! problems, chi, A_t and the face writes into the 3-D initial guess are device kernels (faces.hip).
  !
  ! mode (default VP_POTENTIAL, the above) selects what the three parts - face phase, 3-D phase, post phase
  ! (balance + curl) - are run for:
  !   VP_FIELD     A: initial guess in, A of the whole field out; B: the whole field in (host entry: uploaded,
  !                3N), curl A + balance out.  The 3-D right-hand sides are -(curl B)_c (field.hip).
  !   VP_HELICITY  B: the whole field, read only; A, Ap, Bp: out (both solves start from zero).  The face
  !                phase once; the potential 3-D + post phase -> Ap, Bp; the field 3-D + post phase -> A and
  !                B_rec (library scratch); the reduction of field.hip -> out8.
  !   VP_CURRENT   as VP_FIELD, with the right-hand sides -J_c of the caller's current pJ (nx,ny,nz,3; host entry:
  !                uploaded into the staging array dF(1)); B supplies B.n for the face phase and is not uploaded.
  !   VP_NLFFF     DEVICE arrays only (vecpot_nlfff stages the host entry's).  B in: supplies B.n, and with start = 1
  !                is B^0 (A in: A^0); start = 0: B^0, A^0 = the potential field of that B.n from a zero guess (the
  !                bits of the potential mode on device arrays).  The face phase runs ONCE, from the input B - the
  !                iterates' B.n equals it only to the solve tolerance.  Then up to niter_max passes (nlfff_loop);
  !                B^k and B^{k+1} alternate between pB and the library's dB, and the last one ends in pB.
  ! All of these: IOPT_IERR = 0 if every 2-D and 3-D solve reached vc_tol, else 1 (no Q3'); IOPT_FAIL3D bits 0-2 the
  ! field solves (of any pass), 3-5 the potential solves of a helicity call.
  ! ------------------------------------------------------------------
  ! The field modes keep up to five fields next to the 3-D hierarchy (at least five level-1 arrays): a grid the device
  ! cannot hold at all is refused (9001) before anything is allocated.  Level-1 arrays of a mode besides the hierarchy:
  ! A and B (field); five fields (helicity); A, B and J (current); A, two fields B, alpha and the status (Grad-Rubin).
  function mode_fits(ctx, md) result(rc)
    type(vecpot_ctx), intent(in) :: ctx
    integer, intent(in) :: md
    integer(c_int) :: rc
    integer(c_size_t) :: fr, tot
    integer :: k
    select case (md)
    case (VP_HELICITY); k = 15
    case (VP_CURRENT); k = 9
    case (VP_NLFFF); k = 11
    case default
      k = 6
    end select
    rc = ndsmk_mem_info(fr, tot); if (rc /= 0) return
    if (real(product(int(ctx%n3, ik)), wp) * 8.0_wp * real(merge(5, 0, .not. ctx%live3) + k, wp) > real(tot, wp)) &
      rc = ndsmk_note_error(NDSMK_ENODEV, "the grid needs more device memory than the device has"//c_null_char)
  end function

  function vecpot_run(ctx, iopt, ropt, pA, pB, on_device, mode, pAp, pBp, out8, pJ, nl) result(rc)
    type(vecpot_ctx), intent(inout), target :: ctx
    integer(ik), intent(inout) :: iopt(0:OPT_LEN - 1)
    real(wp), intent(inout) :: ropt(0:OPT_LEN - 1)
    type(c_ptr), intent(in) :: pA, pB
    logical, intent(in) :: on_device
    integer, intent(in), optional :: mode
    type(c_ptr), intent(in), optional :: pAp, pBp, pJ
    real(wp), intent(out), optional :: out8(8)
    type(nlfff_args), intent(inout), optional :: nl
    integer(c_int) :: rc

    character(len=*), parameter :: me = "compute_vector_potential"
    real(wp) :: dq(3), span(3), area(6), du_last, fac
    real(wp), target :: phi(6)
    real(wp), pointer, contiguous :: hA(:, :, :, :), hB(:, :, :, :), stage(:)
    integer(c_int32_t) :: n3(3)
    integer :: f, c, i, ierr2d, ierr3d, ncyc, st, md, shift
    integer :: ncyc6(6), ierr6(6), ncyc3(3), ierr3(3)
    real(wp) :: du6(6), du3(3)
    character(len=8) :: envbuf
    integer(ik) :: sweeps, bad, npts, cnt
    integer(c_int) :: tick_up(3), tick, zero_flag, rcb
    logical :: use_max, resident, host_faces, late_balance, bz_done, field, any2d
    character(len=1) :: bc3(6)
    type(c_ptr) :: dAout, dBout, u3, rhs2, u2, rhs3
    type(c_ptr) :: dBsrc, dAp, dBp, hAdst, hBdst
    type(c_ptr) :: dJ, dAl                  ! the 3-D right-hand sides are -(dJ)_c, or with dAl -(dAl dJ_c)
    type(c_ptr) :: dst, scr                 ! the status array of the Grad-Rubin passes; scr: the library's own
    integer(c_size_t) :: nb, off_y, off_z, fr, tot
    type(face_data), target :: fc(6)

    rc = 0
    md = VP_POTENTIAL
    if (present(mode)) md = mode
    field = .false.; shift = 0; any2d = .false.
    dBsrc = c_null_ptr; dAp = c_null_ptr; dBp = c_null_ptr
    dJ = c_null_ptr; dAl = c_null_ptr; scr = c_null_ptr
    if (md == VP_NLFFF .and. .not. (on_device .and. present(nl))) then
      rc = NDSMK_EARG
      return
    end if
    n3 = ctx%n3
    use_max = (iopt(IOPT_DUMAX) == 1)
    iopt(IOPT_FAIL3D) = 0
    span = [maxval(ctx%qx) - minval(ctx%qx), maxval(ctx%qy) - minval(ctx%qy), maxval(ctx%qz) - minval(ctx%qz)]
    dq = [ctx%qx(2) - ctx%qx(1), ctx%qy(2) - ctx%qy(1), ctx%qz(2) - ctx%qz(1)]      ! :201-221
    area = [span(2) * span(3), span(2) * span(3), span(1) * span(3), span(1) * span(3), &
            span(1) * span(2), span(1) * span(2)]
    npts = product(int(n3, ik))
    nb = int(npts, c_size_t) * 8_c_size_t
    off_y = int(n3(1), c_size_t) * 8_c_size_t
    off_z = off_y + int(n3(2), c_size_t) * 8_c_size_t
    late_balance = (iopt(IOPT_FLXCRL) == 1)     ! :455-465: curl first, fields added to A AND B afterwards
    bz_done = .false.
    call get_environment_variable("NDSM_HIP_HOST_FACES", status=st)   ! A/B testing: the host face phase (vecpot_faces)
    host_faces = (st == 0) .and. .not. on_device
    tick_up = -1
    hAdst = c_null_ptr; hBdst = c_null_ptr                             ! host arrays the results go home to
    if (.not. on_device) then
      call c_f_pointer(pA, hA, [int(n3(1)), int(n3(2)), int(n3(3)), 3])
      call c_f_pointer(pB, hB, [int(n3(1)), int(n3(2)), int(n3(3)), 3])
      hAdst = pA; hBdst = pB
    end if

    if (md /= VP_POTENTIAL) then
      rc = mode_fits(ctx, md); if (rc /= 0) return
    end if

    ! ---- device arrays of this call ----------------------------------
    if (.not. ctx%live3) then
      bc3 = 'D'; bc3(1) = 'N'; bc3(4) = 'N'
      rc = mg_create(ctx%s3v(1), 3, n3, ctx%qx, ctx%qy, ctx%qz, bc3, ctx%ngr); ctx%live3 = .true.
      if (rc /= 0) return
      rc = mg_zero_rhs(ctx%s3v(1)); if (rc /= 0) return            ! :640-641 rhs = 0
      ! The three component solves are independent (:643-689).  Up to a few million points a V-cycle is ~150 launches
      ! of a few microseconds each - dispatch latency, not bandwidth - and one host round trip: with a hierarchy per
      ! component they run side by side on three streams (mg_solve_lanes, as the six face solves do), each one the
      ! kernels it would run alone in the same order.  NDSM_HIP_NO_SIDE3D=1: one after the other (same bits).
      call get_environment_variable("NDSM_HIP_NO_SIDE3D", status=st)
      if (npts <= SIDE3D_MAX .and. st /= 0) then
        do c = 2, 3
          rc = mg_create(ctx%s3v(c), 3, n3, ctx%qx, ctx%qy, ctx%qz, bc3, ctx%ngr)
          if (rc == 0) rc = mg_zero_rhs(ctx%s3v(c))
          if (rc /= 0) then                                          ! (no memory for them: one after the other)
            call mg_destroy(ctx%s3v(c))
            if (c == 3) call mg_destroy(ctx%s3v(2))
            rc = 0
            exit
          end if
          if (c == 3) ctx%live3x = .true.
        end do
      end if
    end if
    resident = .true.
    if (on_device) then
      dAout = pA; dBout = pB
      if (md == VP_FIELD) dBsrc = pB                                 ! (read by the right-hand sides, then overwritten)
      if (md == VP_CURRENT) dJ = pJ
      if (md == VP_NLFFF .and. .not. c_associated(ctx%dB)) then      ! the second of the two fields B^k, B^{k+1}
        rc = ndsmk_alloc(ctx%dB, 3_c_size_t * nb); if (rc /= 0) return
      end if
      if (md == VP_HELICITY) then
        dBsrc = pB; dAp = pAp; dBp = pBp
        if (.not. c_associated(ctx%dB)) then                         ! B_rec
          rc = ndsmk_alloc(ctx%dB, 3_c_size_t * nb); if (rc /= 0) return
        end if
      end if
    else
      if (.not. c_associated(ctx%dA)) then
        rc = ndsmk_alloc(ctx%dA, 3_c_size_t * nb); if (rc /= 0) return
      end if
      if (.not. c_associated(ctx%dB)) then
        if (md == VP_POTENTIAL) then
          ! B next to the hierarchy if HBM has room for both; otherwise it takes the memory the 3-D
          ! hierarchy returns after the solves (the peak is then A + one hierarchy, as before)
          rc = ndsmk_mem_info(fr, tot); if (rc /= 0) return
          resident = fr >= 3_c_size_t * nb + ishft(1_c_size_t, 31)
          call get_environment_variable("NDSM_HIP_LEAN", status=st)      ! testing: take the small-HBM sequence
          if (st == 0) resident = .false.
        end if
        if (resident) then
          rc = ndsmk_alloc(ctx%dB, 3_c_size_t * nb); if (rc /= 0) return
        end if
      end if
      dAout = ctx%dA; dBout = ctx%dB
      if (md == VP_FIELD) then
        ! the whole field goes up: the right-hand sides are its curl (dB then receives curl A + balance)
        rc = ndsmk_h2d(ctx%dB, pB, 3_c_size_t * nb); if (rc /= 0) goto 900
        dBsrc = ctx%dB
      else if (md == VP_CURRENT) then
        rc = stage_field(ctx, 1, pJ); if (rc /= 0) goto 900
        dJ = ctx%dF(1)
      else if (md == VP_HELICITY) then
        do i = 1, 3
          if (.not. c_associated(ctx%dF(i))) then
            rc = ndsmk_alloc(ctx%dF(i), 3_c_size_t * nb); if (rc /= 0) goto 900
          end if
        end do
        rc = ndsmk_h2d(ctx%dF(1), pB, 3_c_size_t * nb); if (rc /= 0) goto 900
        dBsrc = ctx%dF(1); dAp = ctx%dF(2); dBp = ctx%dF(3)
      end if
      ! the worker thread looks at the caller's initial guess meanwhile: components that are not all zero
      ! (the reference's Python passes zeros, ndsm.py:176) go up into their slot of dA
      if (md /= VP_HELICITY) then
        do c = 1, 3
          rc = ndsmk_bg_upload_unless_zero(c_loc(hA(1, 1, 1, c)), dptr_offset(ctx%dA, int(c - 1, c_size_t) * nb), nb, &
                                           tick_up(c))
          if (rc /= 0) goto 900
        end do
      end if
    end if

    rc = face_phase(); if (rc /= 0) goto 900

    ! ---- 4. + 5. the 3-D phase and the post phase, once or (helicity) twice ----
    if (md == VP_NLFFF) then
      ! (the caller passes no status: the history still counts the lines, in a scratch array of 4 B/pt)
      dst = nl%status
      if (.not. c_associated(dst)) then
        rc = ndsmk_alloc(scr, nb / 2_c_size_t); if (rc /= 0) goto 900
        dst = scr
      end if
      rc = nlfff_loop(); if (rc /= 0) goto 900
    else if (md == VP_HELICITY) then
      ! the potential field of the same B.n -> Ap, Bp (FAIL3D bits 3-5) ...
      shift = 3
      dAout = dAp; dBout = dBp
      if (.not. on_device) then
        hAdst = pAp; hBdst = pBp
      end if
      rc = solve3_phase(); if (rc /= 0) goto 900
      rc = post_phase(); if (rc /= 0) goto 900
      ! ... then the whole field -> A and B_rec (library scratch: only the reduction reads it)
      field = .true.; shift = 0; bz_done = .false.
      if (on_device) then
        dAout = pA
      else
        dAout = ctx%dA
      end if
      dBout = ctx%dB
      if (.not. on_device) hAdst = pA
      hBdst = c_null_ptr
      rc = solve3_phase(); if (rc /= 0) goto 900
      rc = post_phase(); if (rc /= 0) goto 900
      call say(me, "Relative helicity...")
      rc = ndsmk_helicity_reduce(dAout, dAp, dBsrc, dBp, dBout, n3, dq, out8); if (rc /= 0) goto 900
    else
      field = (md == VP_FIELD)
      rc = solve3_phase(); if (rc /= 0) goto 900
      rc = post_phase(); if (rc /= 0) goto 900
    end if
    if (md == VP_POTENTIAL) then
      iopt(IOPT_IERR) = ierr2d                              ! Q3'
    else
      iopt(IOPT_IERR) = merge(1, 0, any2d .or. iopt(IOPT_FAIL3D) /= 0)
    end if
    call say(me, "Deallocate memory...")

900 continue
    rcb = ndsmk_bg_drain()                                  ! every byte of A and B is home (or the first error)
    if (rc == 0) rc = rcb
    if (rc == 0) rc = ndsmk_sync()
    if (c_associated(scr)) then
      if (rc /= 0) rcb = ndsmk_sync()                       ! (nothing may still write it)
      rcb = ndsmk_free(scr)
    end if
    if (.not. resident) then                                ! keep the peak at A + one hierarchy next time too
      rcb = ndsmk_free(ctx%dB); ctx%dB = c_null_ptr
    end if

  contains

    ! The Grad-Rubin passes, after the face phase.  Pass k: alpha^k = the alpha map of B^k; the three solves with
    ! rhs_c = -(alpha^k B^k_c), warm-started from A^k (pA, which finish3 overwrites component by component);
    ! B^{k+1} = curl A^{k+1} + balance into the other of the two fields; the history row of the pass.  Every phase is
    ! the one a VP_CURRENT call with J = alpha^k B^k and the initial guess A^k runs: the same kernels in the same order.
    function nlfff_loop() result(rc)
      integer(c_int) :: rc
      real(wp) :: lo(3), row(4)
      real(wp), pointer :: hh(:, :)
      type(c_ptr) :: dBk, dBn, dtmp
      integer :: it
      lo = [ctx%qx(1), ctx%qy(1), ctx%qz(1)]
      call c_f_pointer(nl%hist, hh, [4, int(nl%niter_max)])
      nl%niter = 0
      dBk = pB; dBn = ctx%dB
      if (nl%start == 0) then
        ! B^0, A^0: the potential field of the input's B.n from a zero guess (pB's faces have been read)
        rc = ndsmk_fill0(pA, 3_c_size_t * nb); if (rc /= 0) return
        rc = solve3_phase(); if (rc /= 0) return
        rc = post_phase(); if (rc /= 0) return
      end if
      do it = 1, int(nl%niter_max)
        call say(me, "Grad-Rubin pass: alpha along the field lines...")
        rc = ndsmk_alpha_map(dBk, n3, lo, dq, nl%alpha0, nl%polarity, nl%step, nl%max_steps, nl%alpha, dst)
        if (rc /= 0) return
        dJ = dBk; dAl = nl%alpha
        dBout = dBn; bz_done = .false.
        rc = solve3_phase(); if (rc /= 0) return
        rc = post_phase(); if (rc /= 0) return
        rc = ndsmk_nlfff_metrics(dBn, dBk, dst, n3, dq, row); if (rc /= 0) return
        hh(:, it) = row
        nl%niter = int(it, c_int)
        dtmp = dBk; dBk = dBn; dBn = dtmp
        if (row(1) < nl%tol) exit
      end do
      if (.not. c_associated(dBk, pB)) then
        rc = ndsmk_d2d(pB, dBk, 3_c_size_t * nb); if (rc /= 0) return
      end if
    end function

    ! 1.-3. B.n of the six faces, their fluxes, the six 2-D solves and chi (A_t is written per component by prep3)
    function face_phase() result(rc)
      integer(c_int) :: rc
      rc = 0
      ! ---- 1. B.n on the faces, their fluxes -----------------------------
      call say(me, "Allocate memory to hold boundary conditions...")
      if (host_faces) then
        do f = 1, 6
          fc(f)%n1 = n3(face_t1(f)); fc(f)%n2 = n3(face_t2(f))
          allocate (fc(f)%bn(fc(f)%n1, fc(f)%n2), fc(f)%chi(fc(f)%n1, fc(f)%n2))
          allocate (fc(f)%at1(fc(f)%n1, fc(f)%n2), fc(f)%at2(fc(f)%n1, fc(f)%n2))
          call face_gather(hB, n3, f, fc(f)%bn)
        end do
        rc = vecpot_faces(iopt, ropt, ctx%qx, ctx%qy, ctx%qz, dq, span, fc, phi, ierr2d)
        if (rc /= 0) return
        any2d = (ierr2d /= 0)                     ! (only the last flag comes back from vecpot_faces)
      else
        if (on_device) then
          rc = ndsmk_face_extract(pB, n3, ctx%dbn); if (rc /= 0) return
        else
          call c_f_pointer(ctx%hbn, stage, [ctx%ftotal + 8])
          do f = 1, 6
            call face_gather_flat(hB, n3, f, stage(ctx%foff(f) + 1:ctx%foff(f) + int(n3(face_t1(f)), ik) * int(n3(face_t2(f)), ik)))
          end do
          rc = ndsmk_h2d_async(ctx%dbn, ctx%hbn, int(ctx%ftotal, c_size_t) * 8_c_size_t); if (rc /= 0) return
          ! everything this call reads of the caller's arrays has been read (A: by the upload jobs queued above,
          ! B: its six faces just now); both will be overwritten completely.  Callers like numpy hand over
          ! untouched pages: the worker touches them (4 threads) before the downloads come, which then run at
          ! 50 GB/s instead of 13.  (Helicity: B is read only; A, Ap and Bp are the arrays that come home.)
          if (md == VP_HELICITY) then
            rc = ndsmk_bg_first_touch(pA, 3_c_size_t * nb, tick); if (rc /= 0) return
            rc = ndsmk_bg_first_touch(pAp, 3_c_size_t * nb, tick); if (rc /= 0) return
            rc = ndsmk_bg_first_touch(pBp, 3_c_size_t * nb, tick); if (rc /= 0) return
          else
            rc = ndsmk_bg_first_touch(pA, 3_c_size_t * nb, tick); if (rc /= 0) return
            rc = ndsmk_bg_first_touch(pB, 3_c_size_t * nb, tick); if (rc /= 0) return
          end if
        end if
        rc = ndsmk_face_flux(ctx%dbn, n3, dq(1) * dq(2), ctx%dphi); if (rc /= 0) return     ! Q4
        rc = ndsmk_d2h(c_loc(phi), ctx%dphi, 48_c_size_t); if (rc /= 0) return

        ! ---- 2. chi on every face: 2-D all-Neumann solves, right-hand side and result stay in HBM ----
        call say(me, "Solve BVP on each boundary...")
        ! The six problems are independent (:338-365 solves them one after the other) and each is dispatch
        ! latency plus one host round trip per V-cycle: they run in lockstep on six streams (mg_solve_lanes;
        ! every solve executes the kernels it would execute alone, in the same order - same bits).
        ! NDSM_HIP_FACE_LANES=0: one after the other (A/B testing).
        ierr2d = 0
        do f = 1, 6
          associate (s2 => ctx%s2(f))
            s2%ms = max(0, int(iopt(IOPT_MS))); s2%ex_tol = ropt(ROPT_CTOL); s2%use_max = use_max
            s2%nmax_exact = max(0, int(iopt(IOPT_NMAXEX)))
            rhs2 = mg_level_ptr(s2, 1, MG_BUF_RHS, cnt)
            u2 = mg_level_ptr(s2, 1, MG_BUF_U, cnt)
            rc = ndsmk_face_rhs(ctx%dbn, n3, int(f - 1, c_int), ctx%dphi, area(f), rhs2); if (rc /= 0) return
            call mg_mark_rhs_set(s2)
            rc = ndsmk_fill0(u2, int(cnt, c_size_t) * 8_c_size_t); if (rc /= 0) return
            rc = mg_reset_info(s2); if (rc /= 0) return
          end associate
        end do
        call get_environment_variable("NDSM_HIP_FACE_LANES", envbuf, status=st)
        if (st == 0 .and. envbuf(1:1) == "0") then
          do f = 1, 6
            rc = mg_solve(ctx%s2(f), ropt(ROPT_VTOL), int(iopt(IOPT_NCYCLES)), du6(f), ncyc6(f), ierr6(f))
            if (rc /= 0) return
          end do
        else
          rc = mg_solve_lanes(ctx%s2, ropt(ROPT_VTOL), int(iopt(IOPT_NCYCLES)), du6, ncyc6, ierr6)
          if (rc /= 0) return
        end if
        do f = 1, 6
          u2 = mg_level_ptr(ctx%s2(f), 1, MG_BUF_U, cnt)                  ! (the solver swaps its buffers)
          rc = ndsmk_d2d(dptr_offset(ctx%dchi, int(ctx%foff(f), c_size_t) * 8_c_size_t), u2, int(cnt, c_size_t) * 8_c_size_t)
          if (rc /= 0) return
          ierr2d = ierr6(f)
          if (ierr2d /= 0) any2d = .true.
          if (ierr2d /= 0) print *, "Warning: IOPT_NCYCLES exceeded. V-cycle iteration may not have converged"
          if (mg_read_info(ctx%s2(f), sweeps, bad) == 0) then
            if (bad > 0) print *, "Warning: IOPT_NMAXEX exceeded. Coarse-mesh solution may not have converged"
          end if
        end do
        call say(me, "Compute vector potential boundary conditions...")
      end if
    end function

    ! 4. the three 3-D Laplace / Poisson problems into dAout (finish3: + their flux-balance fields)
    function solve3_phase() result(rc)
      integer(c_int) :: rc
      call say(me, "Solve BVP 3D...")
      if (ctx%live3x .and. iopt(IOPT_PREC) == 0) then
        do c = 1, 3
          rc = prep3(ctx%s3v(c), c); if (rc /= 0) return
        end do
        rc = mg_solve_lanes(ctx%s3v, ropt(ROPT_VTOL), int(iopt(IOPT_NCYCLES)), du3, ncyc3, ierr3); if (rc /= 0) return
        do c = 1, 3
          rc = finish3(ctx%s3v(c), c, du3(c), ncyc3(c), ierr3(c)); if (rc /= 0) return
        end do
      else
        do c = 1, 3
          rc = prep3(ctx%s3v(1), c); if (rc /= 0) return
          rc = mg_solve(ctx%s3v(1), ropt(ROPT_VTOL), int(iopt(IOPT_NCYCLES)), du_last, ncyc, ierr3d)
          if (rc /= 0) return
          rc = finish3(ctx%s3v(1), c, du_last, ncyc, ierr3d); if (rc /= 0) return
        end do
      end if
      if (.not. on_device .and. .not. c_associated(ctx%dB)) then      ! HBM too small for both (see above)
        call mg_destroy(ctx%s3v(1)); ctx%live3 = .false.
        if (ctx%live3x) then
          call mg_destroy(ctx%s3v(2)); call mg_destroy(ctx%s3v(3)); ctx%live3x = .false.
        end if
        rc = ndsmk_alloc(ctx%dB, 3_c_size_t * nb); if (rc /= 0) return
        dBout = ctx%dB
      end if
    end function

    ! 5. B = curl A (and, IOPT_FLXCRL == 1, the fields afterwards) into dBout
    function post_phase() result(rc)
      integer(c_int) :: rc
      call say(me, "Compute B = curl(B) and flux correction...")
      if (late_balance) then
        print *, "FLAG SET: FLXCRL"
        rc = ndsmk_balance_curl(dAout, dBout, n3, ctx%dmesh, dptr_offset(ctx%dmesh, off_y), dptr_offset(ctx%dmesh, off_z), &
                                phi, span, dq, 1_c_int)
        if (rc /= 0) return
        if (c_associated(hAdst)) then
          rc = ndsmk_bg_download(hAdst, dAout, 3_c_size_t * nb, tick); if (rc /= 0) return
        end if
      else if (bz_done) then
        rc = ndsmk_curl_component(dAout, dBout, n3, dq, 0_c_int); if (rc /= 0) return
        rc = ndsmk_curl_component(dAout, dBout, n3, dq, 1_c_int); if (rc /= 0) return
      else
        rc = ndsmk_curl(dAout, dBout, n3, dq); if (rc /= 0) return
      end if
      if (c_associated(hBdst)) then
        rc = ndsmk_bg_download(hBdst, dBout, merge(2_c_size_t, 3_c_size_t, bz_done) * nb, tick); if (rc /= 0) return
      end if
    end function

    ! component c of the 3-D phase on solver s3: initial guess, Dirichlet data, right-hand side, boundary
    ! letters, options
    function prep3(s3, c) result(rc)
      type(mg_solver), intent(inout) :: s3
      integer, intent(in) :: c
      integer(c_int) :: rc
      integer :: i, f
      s3%ex_tol = ropt(ROPT_CTOL); s3%use_max = use_max; s3%nmax_exact = max(0, int(iopt(IOPT_NMAXEX)))
      s3%precision = int(iopt(IOPT_PREC))
      ! initial guess of component c -> the solver's level-1 array
      u3 = mg_level_ptr(s3, 1, MG_BUF_U, cnt)
      if (md == VP_HELICITY) then
        rc = ndsmk_fill0(u3, nb); if (rc /= 0) return
      else if (on_device) then
        rc = ndsmk_d2d(u3, dptr_offset(pA, int(c - 1, c_size_t) * nb), nb); if (rc /= 0) return
      else
        rc = ndsmk_bg_wait(tick_up(c), zero_flag); if (rc /= 0) return
        if (zero_flag /= 0) then
          rc = ndsmk_fill0(u3, nb)
        else
          rc = ndsmk_d2d(u3, dptr_offset(ctx%dA, int(c - 1, c_size_t) * nb), nb)
        end if
        if (rc /= 0) return
      end if
      ! its Dirichlet data: A_t on the four tangential faces, in the reference's order (later writes
      ! win on shared edges, :647-650, :663-666, :679-682)
      do i = 1, 4
        f = face_order(i, c)
        if (host_faces) then
          rc = face_upload(u3, n3, f, merge(1, 2, face_t1(f) == c), fc(f)); if (rc /= 0) return
        else
          fac = 1.0_wp / (2.0_wp * dq(face_axis(f)))            ! Q4: the normal spacing
          rc = ndsmk_face_write(u3, n3, ctx%dchi, int(f - 1, c_int), int(c - 1, c_int), fac); if (rc /= 0) return
        end if
      end do
      ! its right-hand side: -J_c or -(alpha B_c) for a prescribed current or a Grad-Rubin pass, -(curl B)_c for the
      ! whole field, 0 for the potential field (:640-641).  The solvers are cached: the state left by the previous
      ! call on this context is set either way.
      if (c_associated(dJ)) then
        rhs3 = mg_level_ptr(s3, 1, MG_BUF_RHS, cnt)
        rc = ndsmk_current_rhs(dJ, dAl, rhs3, n3, int(c - 1, c_int)); if (rc /= 0) return
        call mg_mark_rhs_set(s3)
      else if (field) then
        rhs3 = mg_level_ptr(s3, 1, MG_BUF_RHS, cnt)
        rc = ndsmk_curl_rhs(dBsrc, rhs3, n3, dq, int(c - 1, c_int)); if (rc /= 0) return
        call mg_mark_rhs_set(s3)
      else if (.not. s3%rhs1_zero) then
        rc = mg_zero_rhs(s3); if (rc /= 0) return
      end if
      bc3 = 'D'
      bc3(c) = 'N'; bc3(3 + c) = 'N'                        ! :655,:671,:687
      rc = mg_set_bcs(s3, bc3); if (rc /= 0) return
      s3%ms = merge(5, max(0, int(iopt(IOPT_MS))), c == 3)          ! Q2
      rc = mg_reset_info(s3)
    end function

    ! ... and what follows its solve: the result into A, the reference's warnings and outputs, its flux-balance
    ! field, its way home
    function finish3(s3, c, du_c, ncyc_c, ierr_c) result(rc)
      type(mg_solver), intent(inout) :: s3
      integer, intent(in) :: c, ncyc_c, ierr_c
      real(wp), intent(in) :: du_c
      integer(c_int) :: rc
      integer :: st3
      rc = mg_export_u(s3, dptr_offset(dAout, int(c - 1, c_size_t) * nb)); if (rc /= 0) return
      if (ierr_c /= 0) print *, "Warning: IOPT_NCYCLES exceeded. V-cycle iteration may not have converged"
      if (mg_read_info(s3, sweeps, bad) == 0) then
        if (bad > 0) print *, "Warning: IOPT_NMAXEX exceeded. Coarse-mesh solution may not have converged"
      end if
      if (ierr_c /= 0) iopt(IOPT_FAIL3D) = ior(iopt(IOPT_FAIL3D), ishft(1_ik, c - 1 + shift))
      if (ncyc_c > 1 .or. c == 1) then
        iopt(IOPT_NCYC_OUT) = ncyc_c
        ropt(ROPT_DULAST) = du_c
      end if
      ! default order (:467-477): the flux-balance fields come before the curl, so this component is final
      ! once its own field is added - and goes home behind the next component's solve
      if (.not. late_balance) then
        rc = ndsmk_balance_component(dptr_offset(dAout, int(c - 1, c_size_t) * nb), n3, int(c - 1, c_int), ctx%dmesh, &
                                     dptr_offset(ctx%dmesh, off_y), dptr_offset(ctx%dmesh, off_z), phi, span)
        if (rc /= 0) return
        if (c_associated(hAdst)) then
          rc = ndsmk_bg_download(dptr_offset(hAdst, int(c - 1, c_size_t) * nb), dptr_offset(dAout, int(c - 1, c_size_t) * nb), &
                                 nb, tick)
          if (rc /= 0) return
        end if
        ! B_z = d(A_y)/dx - d(A_x)/dy needs the two components that are final now: it is formed here and goes
        ! home behind the A_z solve as well (when B's device array exists already: not on the lean path; and not
        ! where B_z would overwrite the field the A_z solve still takes its right-hand side from)
        call get_environment_variable("NDSM_HIP_NO_EARLY_BZ", status=st3)      ! A/B testing: one curl at the end
        if (c == 2 .and. c_associated(dBout) .and. all(n3 >= 3) .and. st3 /= 0 .and. &
            .not. (field .and. c_associated(dBsrc, dBout))) then
          rc = ndsmk_curl_component(dAout, dBout, n3, dq, 2_c_int); if (rc /= 0) return
          if (c_associated(hBdst)) then
            rc = ndsmk_bg_download(dptr_offset(hBdst, 2_c_size_t * nb), dptr_offset(dBout, 2_c_size_t * nb), nb, tick)
            if (rc /= 0) return
          end if
          bz_done = .true.
        end if
      end if
    end function
  end function

  ! ------------------------------------------------------------------
  ! Solenoidal projection on a prepared context (DESIGN.md "Solenoidal projection"): B' = B - G_h phi,
  ! laplace_7(phi) = div_h B - c with all six faces Neumann, c = sum w div_h B / sum w (the part no projection
  ! that keeps B.n can remove).  pB: (nx,ny,nz,3) in and out, on the HOST or (on_device) in HBM; pphi: phi
  ! (nx,ny,nz) out, may be null.  out4: c, max |div_h B|, max |div_h B'|, 1/2 sum w |G_h phi|^2.
  ! The solve is the ordinary 3-D V-cycle with the usual options (ms, ncycles, nmaxex, dumax, vtol, ctol), from
  ! phi = 0, always fp64: IOPT_PREC is ignored (the mixed-precision cycle refuses all-Neumann levels).
  ! IOPT_IERR = 0 when the solve reached vc_tol, else 1; IOPT_NCYC_OUT, ROPT_DULAST of the solve.
  ! The hierarchy is created at the first projection on the context and kept with it.
  ! ------------------------------------------------------------------
  function vecpot_project(ctx, iopt, ropt, pB, pphi, on_device, out4) result(rc)
    type(vecpot_ctx), intent(inout), target :: ctx
    integer(ik), intent(inout) :: iopt(0:OPT_LEN - 1)
    real(wp), intent(inout) :: ropt(0:OPT_LEN - 1)
    type(c_ptr), intent(in) :: pB, pphi
    logical, intent(in) :: on_device
    real(wp), intent(out) :: out4(4)
    integer(c_int) :: rc
    character(len=*), parameter :: me = "solenoidal_projection"
    real(wp) :: dq(3), du
    integer(c_int32_t) :: n3(3)
    integer :: ncyc, ierr
    integer(ik) :: cnt, sweeps, bad
    integer(c_size_t) :: nb, fr, tot
    character(len=1) :: bcn(6)
    type(c_ptr) :: dB, u1, rhs1

    out4 = 0
    n3 = ctx%n3
    if (any(n3 < 3)) then
      rc = ndsmk_note_error(NDSMK_EARG, "the projection needs at least 3 points per axis"//c_null_char)
      return
    end if
    dq = [ctx%qx(2) - ctx%qx(1), ctx%qy(2) - ctx%qy(1), ctx%qz(2) - ctx%qz(1)]
    nb = int(product(int(n3, ik)), c_size_t) * 8_c_size_t
    ! the hierarchy (about six level-1 arrays) next to B and phi: a grid the device cannot hold at all is refused
    ! before anything is allocated
    rc = ndsmk_mem_info(fr, tot); if (rc /= 0) return
    if (real(nb, wp) * real(merge(6, 0, .not. ctx%livep) + 4, wp) > real(tot, wp)) then
      rc = ndsmk_note_error(NDSMK_ENODEV, "the grid needs more device memory than the device has"//c_null_char)
      return
    end if
    if (.not. ctx%livep) then
      bcn = 'N'
      rc = mg_create(ctx%sp, 3, n3, ctx%qx, ctx%qy, ctx%qz, bcn, ctx%ngr); ctx%livep = .true.
      if (rc /= 0) return
    end if
    if (on_device) then
      dB = pB
    else
      if (.not. c_associated(ctx%dB)) then
        rc = ndsmk_alloc(ctx%dB, 3_c_size_t * nb); if (rc /= 0) return
      end if
      dB = ctx%dB
      rc = ndsmk_h2d(dB, pB, 3_c_size_t * nb); if (rc /= 0) return
    end if
    associate (s => ctx%sp)
      s%ms = max(0, int(iopt(IOPT_MS))); s%ex_tol = ropt(ROPT_CTOL); s%use_max = (iopt(IOPT_DUMAX) == 1)
      s%nmax_exact = max(0, int(iopt(IOPT_NMAXEX)))
      s%precision = 0
      call say(me, "Divergence...")
      rhs1 = mg_level_ptr(s, 1, MG_BUF_RHS, cnt)
      rc = ndsmk_project_div_rhs(dB, rhs1, n3, dq); if (rc /= 0) return
      call mg_mark_rhs_set(s)
      u1 = mg_level_ptr(s, 1, MG_BUF_U, cnt)
      rc = ndsmk_fill0(u1, nb); if (rc /= 0) return
      rc = mg_reset_info(s); if (rc /= 0) return
      call say(me, "Solve BVP 3D (all Neumann)...")
      rc = mg_solve(s, ropt(ROPT_VTOL), int(iopt(IOPT_NCYCLES)), du, ncyc, ierr); if (rc /= 0) return
      if (ierr /= 0) print *, "Warning: IOPT_NCYCLES exceeded. V-cycle iteration may not have converged"
      if (mg_read_info(s, sweeps, bad) == 0) then
        if (bad > 0) print *, "Warning: IOPT_NMAXEX exceeded. Coarse-mesh solution may not have converged"
      end if
      call say(me, "Subtract grad phi...")
      u1 = mg_level_ptr(s, 1, MG_BUF_U, cnt)                  ! (the solver swaps its buffers)
      rc = ndsmk_project_grad_sub(dB, u1, n3, dq); if (rc /= 0) return
      rc = ndsmk_project_div_max(dB, n3, dq, out4); if (rc /= 0) return
      if (c_associated(pphi)) then
        if (on_device) then
          rc = ndsmk_d2d(pphi, u1, nb)
        else
          rc = ndsmk_d2h(pphi, u1, nb)
        end if
        if (rc /= 0) return
      end if
    end associate
    if (.not. on_device) then
      rc = ndsmk_d2h(pB, dB, 3_c_size_t * nb); if (rc /= 0) return
    end if
    rc = ndsmk_sync(); if (rc /= 0) return
    iopt(IOPT_IERR) = ierr
    iopt(IOPT_NCYC_OUT) = ncyc
    ropt(ROPT_DULAST) = du
  end function

  ! ------------------------------------------------------------------
  ! DeVore-gauge vector potentials and relative helicity on a prepared context (DESIGN.md "DeVore-gauge vector
  ! potentials"): A_z = 0, A of B integrated up from the base plane of B_z(z0), A_p of B_p integrated down from
  ! A's top plane (devore.hip), then B_rec = curl_h A into the context's scratch and the reduction of
  ! field.hip -> out8 (out8(8) = max |div_h A|: the gauge's divergence, not an error).  pB, pBp in, pA, pAp out,
  ! (nx,ny,nz,3) on the HOST (B and B_p go up, A and A_p come home) or (on_device) in HBM.  dq as in vecpot_run.
  ! No solve, no hierarchy: B_p is the caller's (any field whose B.n matches B's).
  ! ------------------------------------------------------------------
  function vecpot_devore(ctx, pB, pBp, pA, pAp, on_device, out8) result(rc)
    type(vecpot_ctx), intent(inout), target :: ctx
    type(c_ptr), intent(in) :: pB, pBp, pA, pAp
    logical, intent(in) :: on_device
    real(wp), intent(out) :: out8(8)
    integer(c_int) :: rc
    character(len=*), parameter :: me = "devore_potentials"
    real(wp) :: dq(3)
    integer(c_int32_t) :: n3(3)
    integer(c_size_t) :: nb, fr, tot
    integer :: i
    type(c_ptr) :: dB, dBp, dA, dAp

    out8 = 0
    n3 = ctx%n3
    if (any(n3 < 3)) then
      rc = ndsmk_note_error(NDSMK_EARG, "the DeVore gauge needs at least 3 points per axis"//c_null_char)
      return
    end if
    dq = [ctx%qx(2) - ctx%qx(1), ctx%qy(2) - ctx%qy(1), ctx%qz(2) - ctx%qz(1)]      ! as vecpot_run
    nb = int(product(int(n3, ik)), c_size_t) * 8_c_size_t
    ! five fields of 24 B/pt (B, B_p, A, A_p, B_rec): a grid the device cannot hold is refused before anything is
    ! allocated
    rc = ndsmk_mem_info(fr, tot); if (rc /= 0) return
    if (real(nb, wp) * 15.0_wp > real(tot, wp)) then
      rc = ndsmk_note_error(NDSMK_ENODEV, "the grid needs more device memory than the device has"//c_null_char)
      return
    end if
    if (.not. c_associated(ctx%dB)) then                           ! B_rec
      rc = ndsmk_alloc(ctx%dB, 3_c_size_t * nb); if (rc /= 0) return
    end if
    if (on_device) then
      dB = pB; dBp = pBp; dA = pA; dAp = pAp
    else
      ! the helicity entries' host staging: dF(1) B, dF(2) A_p, dF(3) B_p, dA A
      if (.not. c_associated(ctx%dA)) then
        rc = ndsmk_alloc(ctx%dA, 3_c_size_t * nb); if (rc /= 0) return
      end if
      do i = 1, 3
        if (.not. c_associated(ctx%dF(i))) then
          rc = ndsmk_alloc(ctx%dF(i), 3_c_size_t * nb); if (rc /= 0) return
        end if
      end do
      dB = ctx%dF(1); dAp = ctx%dF(2); dBp = ctx%dF(3); dA = ctx%dA
      rc = ndsmk_h2d(dB, pB, 3_c_size_t * nb); if (rc /= 0) return
      rc = ndsmk_h2d(dBp, pBp, 3_c_size_t * nb); if (rc /= 0) return
    end if
    call say(me, "DeVore gauge: base plane, columns up (A) and down (A_p)...")
    rc = ndsmk_devore(dB, dBp, dA, dAp, n3, dq); if (rc /= 0) return
    call say(me, "B_rec = curl(A)...")
    rc = ndsmk_curl(dA, ctx%dB, n3, dq); if (rc /= 0) return
    call say(me, "Relative helicity...")
    rc = ndsmk_helicity_reduce(dA, dAp, dB, dBp, ctx%dB, n3, dq, out8); if (rc /= 0) return
    if (.not. on_device) then
      rc = ndsmk_d2h(pA, dA, 3_c_size_t * nb); if (rc /= 0) return
      rc = ndsmk_d2h(pAp, dAp, 3_c_size_t * nb); if (rc /= 0) return
    end if
    rc = ndsmk_sync()
  end function

  ! ------------------------------------------------------------------
  ! Staging of the host-array line entries below.  Each of them names its arrays once, as a list of slices in the order
  ! of the kernel entry's arguments; carve gives every slice its place in one device buffer and sends the inputs up,
  ! fetch brings the outputs home, unstage frees.
  ! ------------------------------------------------------------------

  ! first point, spacing and shape of the context's mesh (dq as in vecpot_run)
  subroutine ctx_mesh(ctx, n3, lo, dq)
    type(vecpot_ctx), intent(in) :: ctx
    integer(c_int32_t), intent(out) :: n3(3)
    real(wp), intent(out) :: lo(3), dq(3)
    n3 = ctx%n3
    dq = [ctx%qx(2) - ctx%qx(1), ctx%qy(2) - ctx%qy(1), ctx%qz(2) - ctx%qz(1)]
    lo = [ctx%qx(1), ctx%qy(1), ctx%qz(1)]
  end subroutine

  ! the helicity entries' staging array dF(i), allocated at the first use; host (nx,ny,nz,3) goes up into it
  ! (c_null_ptr: nothing goes up)
  function stage_field(ctx, i, host) result(rc)
    type(vecpot_ctx), intent(inout) :: ctx
    integer, intent(in) :: i
    type(c_ptr), intent(in) :: host
    integer(c_int) :: rc
    integer(c_size_t) :: nb
    rc = 0
    nb = int(product(int(ctx%n3, ik)), c_size_t) * 24_c_size_t
    if (.not. c_associated(ctx%dF(i))) rc = ndsmk_alloc(ctx%dF(i), nb)
    if (rc == 0 .and. c_associated(host)) rc = ndsmk_h2d(ctx%dF(i), host, nb)
  end function

  ! buf: one device buffer of all slices of s that have a host array and a count > 0, each rounded up to a whole number
  ! of 8-byte words (so any order of the slices keeps 8-byte data aligned); the others get c_null_ptr.  The inputs go
  ! up.  Nothing to hold: no buffer.  On an error of a copy the buffer stays allocated for unstage.
  function carve(buf, s) result(rc)
    type(c_ptr), intent(out) :: buf
    type(slice), intent(inout) :: s(:)
    integer(c_int) :: rc
    integer(c_size_t) :: no, bytes(size(s))
    integer :: i
    rc = 0
    buf = c_null_ptr
    do i = 1, size(s)
      s(i)%dev = c_null_ptr
      bytes(i) = 0
      if (c_associated(s(i)%host)) bytes(i) = (s(i)%width * s(i)%count + 7_c_size_t) / 8_c_size_t * 8_c_size_t
    end do
    if (sum(bytes) == 0) return
    rc = ndsmk_alloc(buf, sum(bytes)); if (rc /= 0) return
    no = 0
    do i = 1, size(s)
      if (bytes(i) == 0) cycle
      s(i)%dev = dptr_offset(buf, no)
      no = no + bytes(i)
      if (rc == 0 .and. .not. s(i)%home) rc = ndsmk_h2d(s(i)%dev, s(i)%host, s(i)%width * s(i)%count)
    end do
  end function

  ! the outputs among the slices of s come home (rows given: that many entries of each instead of its count)
  function fetch(s, rows) result(rc)
    type(slice), intent(in) :: s(:)
    integer(c_size_t), intent(in), optional :: rows
    integer(c_int) :: rc
    integer(c_size_t) :: n
    integer :: i
    rc = 0
    do i = 1, size(s)
      n = s(i)%count
      if (present(rows)) n = rows
      if (rc == 0 .and. s(i)%home .and. c_associated(s(i)%dev) .and. n > 0) &
        rc = ndsmk_d2h(s(i)%host, s(i)%dev, s(i)%width * n)
    end do
  end function

  ! the buffers of carve are freed in the order given; the first error wins, and any error zeroes total
  subroutine unstage(rc, bufs, total)
    integer(c_int), intent(inout) :: rc
    type(c_ptr), intent(in) :: bufs(:)
    integer(c_int64_t), intent(inout), optional :: total
    integer(c_int) :: rc_free
    integer :: i
    do i = 1, size(bufs)
      if (c_associated(bufs(i))) then
        rc_free = ndsmk_free(bufs(i))
        if (rc == 0) rc = rc_free
      end if
    end do
    if (present(total) .and. rc /= 0) total = 0
  end subroutine

  ! ------------------------------------------------------------------
  ! The line entries on a prepared context (semantics in include/ndsm_hip.h): field lines of B from nseeds seeds with
  ! the line integral of G along them (squash false: ndsmk_trace, sel = direction; DESIGN.md "Field-line tracing and
  ! field-line helicity"), or the squashing factor Q at the seeds with the two ends of the line through each (squash
  ! true: ndsmk_squash, sel = integrand, always both directions; DESIGN.md "Squashing factor and twist").  The
  ! context supplies the mesh only: first point and spacing per axis, dq as in vecpot_run.  No solve, no hierarchy.
  ! pB, pG (pG may be c_null_ptr: integrals 0) (nx,ny,nz,3), pseeds (3,nseeds) in; pends (3,nl), plen, pint (nl)
  ! doubles and pstat, pnst (nl) int32 out, nl = 2 nseeds (squash, direction 0) or nseeds; pq (nseeds) doubles out
  ! for squash, not looked at for trace: on the HOST (B, G and the seeds go up into the helicity entries' staging
  ! arrays and a scratch buffer, the results come home) or (on_device) in HBM.  Squash with integrand 1 and pG the
  ! very pointer pB: G = curl_h B (ndsmk_curl into the staging array dF(2)), the twist map.  Squash with pqperp given
  ! (nseeds doubles out, where pq is): ndsmk_squash_perp, the perpendicular squashing factor next to Q (DESIGN.md
  ! "Perpendicular squashing factor").
  ! ------------------------------------------------------------------
  function vecpot_lines(ctx, squash, pB, pG, sel, nseeds, pseeds, step, max_steps, pq, pends, plen, pint, pstat, pnst, &
                        on_device, pqperp) result(rc)
    type(vecpot_ctx), intent(inout), target :: ctx
    logical, intent(in) :: squash, on_device
    type(c_ptr), intent(in) :: pB, pG, pseeds, pq, pends, plen, pint, pstat, pnst
    type(c_ptr), intent(in), optional :: pqperp
    integer(c_int), intent(in) :: sel, nseeds, max_steps
    real(wp), intent(in) :: step
    integer(c_int) :: rc, rc_free
    real(wp) :: dq(3), lo(3)
    integer(c_int32_t) :: n3(3)
    integer(c_size_t) :: nl, ns
    logical :: own_curl, perp
    type(c_ptr) :: dB, dG, buf, pqp
    type(slice) :: s(8)

    call ctx_mesh(ctx, n3, lo, dq)
    perp = squash .and. present(pqperp)
    pqp = c_null_ptr
    if (perp) pqp = pqperp
    if (nseeds <= 0 .or. step <= 0.0_wp .or. max_steps < 1 .or. sel < merge(0, -1, squash) .or. sel > 1) then
      ! (the argument errors are the kernel entry's to name; nothing is staged for them)
      rc = launch(pB, pG, pseeds, pq, pqp, pends, plen, pint, pstat, pnst)
      ! (trace synchronises here, squash does not: ndsmk_sync can return an earlier asynchronous error, so the call
      ! is part of what each entry returns)
      if (rc == 0 .and. .not. squash) rc = ndsmk_sync()
      return
    end if
    ns = int(nseeds, c_size_t)
    nl = ns * merge(2_c_size_t, 1_c_size_t, squash .or. sel == 0)
    ! G given as B itself with integrand 1: the twist map, G = curl_h B formed here in the staging array dF(2)
    own_curl = squash .and. sel == 1 .and. c_associated(pG) .and. c_associated(pG, pB)
    ! the helicity entries' host staging: dF(1) B, dF(2) G
    dB = pB
    dG = pG
    if (.not. on_device) then
      rc = stage_field(ctx, 1, pB); if (rc /= 0) return
      dB = ctx%dF(1)
      if (c_associated(pG) .and. .not. own_curl) then
        rc = stage_field(ctx, 2, pG); if (rc /= 0) return
        dG = ctx%dF(2)
      end if
    end if
    if (own_curl) then
      rc = stage_field(ctx, 2, c_null_ptr); if (rc /= 0) return
      dG = ctx%dF(2)
      call say("squashing_factor", "G = curl(B)...")
      rc = ndsmk_curl(dB, dG, n3, dq); if (rc /= 0) return
    end if
    if (on_device) then
      rc = launch(dB, dG, pseeds, pq, pqp, pends, plen, pint, pstat, pnst)
      if (rc /= 0) return
      rc = ndsmk_sync()
      return
    end if
    s = [slice(pseeds, 24, ns, GOES_UP), slice(merge(pq, c_null_ptr, squash), 8, ns, COMES_HOME), &
         slice(pends, 24, nl, COMES_HOME), slice(plen, 8, nl, COMES_HOME), slice(pint, 8, nl, COMES_HOME), &
         slice(pstat, 4, nl, COMES_HOME), slice(pnst, 4, nl, COMES_HOME), slice(pqp, 8, ns, COMES_HOME)]
    rc = carve(buf, s)
    if (rc == 0) then
      if (squash) then
        call say("squashing_factor", "Tracing field lines with their deviation vectors...")
      else
        call say("trace_field_lines", "Tracing field lines...")
      end if
      rc = launch(dB, dG, s(1)%dev, s(2)%dev, s(8)%dev, s(3)%dev, s(4)%dev, s(5)%dev, s(6)%dev, s(7)%dev)
    end if
    if (rc == 0) rc = fetch(s)
    if (rc == 0) rc = ndsmk_sync()
    rc_free = rc                                       ! (an error of the free is not returned here, unlike below)
    call unstage(rc_free, [buf])
  contains
    ! the kernel entry of this call on the given arrays (q: looked at by squash only, qperp by squash with pqperp)
    function launch(B, G, seeds, q, qperp, ends, length, integral, status, nsteps) result(rc)
      type(c_ptr), intent(in) :: B, G, seeds, q, qperp, ends, length, integral, status, nsteps
      integer(c_int) :: rc
      if (perp) then
        rc = ndsmk_squash_perp(B, G, sel, n3, lo, dq, nseeds, seeds, step, max_steps, q, qperp, ends, length, integral, &
                               status, nsteps)
      else if (squash) then
        rc = ndsmk_squash(B, G, sel, n3, lo, dq, nseeds, seeds, step, max_steps, q, ends, length, integral, status, &
                          nsteps)
      else
        rc = ndsmk_trace(B, G, n3, lo, dq, nseeds, seeds, step, max_steps, sel, ends, length, integral, status, nsteps)
      end if
    end function
  end function

  ! ------------------------------------------------------------------
  ! The alpha map on a prepared context (semantics in include/ndsm_hip.h, DESIGN.md "Nonlinear force-free field"):
  ! palpha0 (nx,ny) on the lower face carried along the lines of pB (nx,ny,nz,3) to every node, palpha (nx,ny,nz) and
  ! pstat (nx,ny,nz; int32, may be c_null_ptr) out - on the HOST (B goes up into the staging array dF(1), alpha0 and
  ! the results through a scratch buffer) or (on_device) in HBM.  The context supplies the mesh only, as in
  ! vecpot_lines: no solve, no hierarchy.
  ! ------------------------------------------------------------------
  function vecpot_alpha_map(ctx, pB, palpha0, polarity, step, max_steps, palpha, pstat, on_device) result(rc)
    type(vecpot_ctx), intent(inout), target :: ctx
    logical, intent(in) :: on_device
    type(c_ptr), intent(in) :: pB, palpha0, palpha, pstat
    integer(c_int), intent(in) :: polarity, max_steps
    real(wp), intent(in) :: step
    integer(c_int) :: rc
    real(wp) :: dq(3), lo(3)
    integer(c_int32_t) :: n3(3)
    integer(c_size_t) :: np, nf
    type(c_ptr) :: buf
    type(slice) :: s(3)

    call ctx_mesh(ctx, n3, lo, dq)
    if (on_device .or. .not. (step > 0.0_wp) .or. max_steps < 1 .or. (polarity /= 1 .and. polarity /= -1)) then
      ! (the argument errors are the kernel entry's to name; nothing is staged for them)
      rc = ndsmk_alpha_map(pB, n3, lo, dq, palpha0, polarity, step, max_steps, palpha, pstat)
      if (rc == 0) rc = ndsmk_sync()
      return
    end if
    nf = int(n3(1), c_size_t) * int(n3(2), c_size_t)
    np = nf * int(n3(3), c_size_t)
    rc = stage_field(ctx, 1, pB); if (rc /= 0) return
    s = [slice(palpha0, 8, nf, GOES_UP), slice(palpha, 8, np, COMES_HOME), slice(pstat, 4, np, COMES_HOME)]
    rc = carve(buf, s)
    if (rc == 0) then
      call say("alpha_map", "Carrying alpha along the field lines...")
      rc = ndsmk_alpha_map(ctx%dF(1), n3, lo, dq, s(1)%dev, polarity, step, max_steps, s(2)%dev, s(3)%dev)
    end if
    if (rc == 0) rc = fetch(s)
    if (rc == 0) rc = ndsmk_sync()
    call unstage(rc, [buf])
  end function

  ! ------------------------------------------------------------------
  ! The Grad-Rubin iteration on a prepared context (vecpot_run, mode VP_NLFFF; semantics in include/ndsm_hip.h).  nl
  ! holds the caller's alpha0, alpha, status (may be c_null_ptr: vecpot_run's scratch takes its place) and hist, and the
  ! scalars, which the C ABI has checked; nl%niter comes back.  pA, pB (nx,ny,nz,3) and nl's three arrays on the HOST
  ! (B, and with start = 1 A, go up into the staging arrays dF(1) and dA, alpha0 and the results through a scratch
  ! buffer; between the upload and the downloads nothing crosses PCIe but the fluxes and the per-cycle and per-pass
  ! read-backs) or (on_device) in HBM.  A grid whose arrays the device cannot hold is refused before anything is
  ! allocated.
  ! ------------------------------------------------------------------
  function vecpot_nlfff(ctx, iopt, ropt, pA, pB, nl, on_device) result(rc)
    type(vecpot_ctx), intent(inout), target :: ctx
    integer(ik), intent(inout) :: iopt(0:OPT_LEN - 1)
    real(wp), intent(inout) :: ropt(0:OPT_LEN - 1)
    type(c_ptr), intent(in) :: pA, pB
    type(nlfff_args), intent(inout) :: nl
    logical, intent(in) :: on_device
    integer(c_int) :: rc
    type(nlfff_args) :: dv
    integer(c_size_t) :: np, nf, nb3
    type(c_ptr) :: buf
    type(slice) :: s(3)

    nl%niter = 0
    nf = int(ctx%n3(1), c_size_t) * int(ctx%n3(2), c_size_t)
    np = nf * int(ctx%n3(3), c_size_t)
    nb3 = np * 24_c_size_t
    buf = c_null_ptr
    dv = nl
    if (.not. on_device) then
      rc = mode_fits(ctx, VP_NLFFF); if (rc /= 0) return
      if (.not. c_associated(ctx%dA)) then
        rc = ndsmk_alloc(ctx%dA, nb3); if (rc /= 0) return
      end if
      rc = stage_field(ctx, 1, pB); if (rc /= 0) return
      if (nl%start == 1) then
        rc = ndsmk_h2d(ctx%dA, pA, nb3); if (rc /= 0) return
      end if
      s = [slice(nl%alpha0, 8, nf, GOES_UP), slice(nl%alpha, 8, np, COMES_HOME), slice(nl%status, 4, np, COMES_HOME)]
      rc = carve(buf, s)
      dv%alpha0 = s(1)%dev; dv%alpha = s(2)%dev; dv%status = s(3)%dev
    else
      rc = 0
    end if
    if (rc == 0) then
      if (on_device) then
        rc = vecpot_run(ctx, iopt, ropt, pA, pB, .true., VP_NLFFF, nl=dv)
      else
        rc = vecpot_run(ctx, iopt, ropt, ctx%dA, ctx%dF(1), .true., VP_NLFFF, nl=dv)
        if (rc == 0) rc = ndsmk_d2h(pA, ctx%dA, nb3)
        if (rc == 0) rc = ndsmk_d2h(pB, ctx%dF(1), nb3)
        if (rc == 0) rc = fetch(s)
        if (rc == 0) rc = ndsmk_sync()
      end if
    end if
    nl%niter = dv%niter
    call unstage(rc, [buf])
  end function

  ! ------------------------------------------------------------------
  ! The check loop of the descents (vecpot_optimize, vecpot_preprocess), which all decide their steps on the device.
  ! The caller owns the kernel-layer calls and nothing else:
  !     <begin>;  <row> into lp%row;  call descent_open(lp, ctl, width)
  !     do while (descent_more(lp, ctl))
  !       <tries> with lp%n;  <row> into lp%row;  call descent_note(lp, ctl)
  !     end do
  !     rc = descent_close(lp, ctl, ...)
  ! Row 1 of the history is the start; every interval of ctl%check tries (the last may be shorter) adds a row, the last
  ! row being overwritten once hist_rows are full.  Stop reasons: 2 the device raised its stop flag (dt < dt_min), 1 L
  ! fell by no more than tol * L over a FULL interval, 0 niter_max.
  ! ------------------------------------------------------------------
  subroutine descent_open(lp, ctl, width)
    type(descent_loop), intent(inout) :: lp
    type(descent_ctl), intent(inout) :: ctl
    integer, intent(in) :: width
    lp%width = width
    call c_f_pointer(ctl%hist, lp%hh, [width, int(ctl%hist_rows)])
    lp%hh(:, 1) = lp%row(1:width)
    lp%rows = 1; lp%tries = 0
    lp%lprev = lp%row(2)
    ctl%info(3) = 0
    if (lp%row(width + 2) /= 0.0_wp) ctl%info(3) = 2
  end subroutine

  ! whether another interval runs; lp%n: its tries
  function descent_more(lp, ctl) result(more)
    type(descent_loop), intent(inout) :: lp
    type(descent_ctl), intent(in) :: ctl
    logical :: more
    more = ctl%info(3) == 0 .and. lp%tries < ctl%niter_max
    if (more) lp%n = min(ctl%check, ctl%niter_max - lp%tries)
  end function

  ! after the row of an interval has been read back
  subroutine descent_note(lp, ctl)
    type(descent_loop), intent(inout) :: lp
    type(descent_ctl), intent(inout) :: ctl
    lp%tries = lp%tries + lp%n
    lp%rows = min(lp%rows + 1_c_int, ctl%hist_rows)
    lp%hh(:, lp%rows) = lp%row(1:lp%width)
    if (lp%row(lp%width + 2) /= 0.0_wp) then
      ctl%info(3) = 2
    else if (lp%n == ctl%check) then
      if (lp%lprev - lp%row(2) <= ctl%tol * lp%lprev) ctl%info(3) = 1
      lp%lprev = lp%row(2)
    end if
  end subroutine

  ! info, then the result (nbytes) into dB0 when buffer 1 is the current one, home to pB for the host entry, and the sync
  function descent_close(lp, ctl, dB0, dB1, nbytes, pB, on_device) result(rc)
    type(descent_loop), intent(in) :: lp
    type(descent_ctl), intent(inout) :: ctl
    type(c_ptr), intent(in) :: dB0, dB1, pB
    integer(c_size_t), intent(in) :: nbytes
    logical, intent(in) :: on_device
    integer(c_int) :: rc
    ctl%info(1) = lp%rows
    ctl%info(2) = int(lp%row(1), c_int)
    if (lp%row(lp%width + 1) /= 0.0_wp) then
      rc = ndsmk_d2d(dB0, dB1, nbytes); if (rc /= 0) return
    end if
    if (.not. on_device) then
      rc = ndsmk_d2h(pB, dB0, nbytes); if (rc /= 0) return
    end if
    rc = ndsmk_sync()
  end function

  ! ------------------------------------------------------------------
  ! The optimization method on a prepared context (semantics in include/ndsm_hip.h, DESIGN.md "Optimization-method
  ! force-free field").  pB (nx,ny,nz,3) in and out and op%w (nx,ny,nz; may be c_null_ptr) in, on the HOST (both go up
  ! once, B comes home once; between the two only history rows cross PCIe) or (on_device) in HBM; op%hist on the HOST.
  ! start = 1: the input is B^0, the context supplies the mesh only - no solve, no hierarchy.  start = 0: B^0 is the
  ! potential field of the input's B.n (vecpot_run's potential mode on device arrays, a zero guess), its k = 0 plane
  ! then replaced by the input's.  One buffer holds the second field, the two Omega and the state for the length of
  ! the call; a grid whose arrays the device cannot hold is refused before it is allocated.  The tries of one check
  ! interval are queued without a read-back: the device decides each (optimize.hip).
  ! With op%bobs the call has a measurement term and a freed lower face (DESIGN.md "Measurement errors and a freed
  ! lower face"): op%bobs (nx,ny,3) and op%wm (nx,ny,3; may be c_null_ptr) on the side B is on - the host entry stages
  ! the two planes once, behind B and w.  The start field is the same, on B alone; the kernels are optimize_obs.hip's.
  ! ------------------------------------------------------------------
  function vecpot_optimize(ctx, iopt, ropt, pB, op, on_device) result(rc)
    type(vecpot_ctx), intent(inout), target :: ctx
    integer(ik), intent(inout) :: iopt(0:OPT_LEN - 1)
    real(wp), intent(inout) :: ropt(0:OPT_LEN - 1)
    type(c_ptr), intent(in) :: pB
    type(optimize_args), intent(inout) :: op
    logical, intent(in) :: on_device
    integer(c_int) :: rc
    real(wp) :: dq(3), lo(3)
    integer(c_int32_t) :: n3(3)
    integer(c_size_t) :: nb, pl3, wk, total, fr, tot, at
    integer :: k
    logical :: obs
    type(descent_loop) :: lp
    type(c_ptr) :: buf, dB0, dB1, dO, dwork, dw, dbobs, dwm

    op%info = 0
    buf = c_null_ptr
    obs = c_associated(op%bobs)
    call ctx_mesh(ctx, n3, lo, dq)
    nb = int(product(int(n3, ik)), c_size_t) * 8_c_size_t
    pl3 = 0
    if (obs) pl3 = int(n3(1), c_size_t) * int(n3(2), c_size_t) * 24_c_size_t   ! a plane of three components
    if (obs) then
      wk = ndsmk_optimize_obs_work_bytes()
    else
      wk = ndsmk_optimize_work_bytes()
    end if
    ! two fields, two Omega and w are 13 level-1 arrays; a potential start adds the 3-D hierarchy (at least five);
    ! with an observation, its two planes
    k = 13 + merge(5, 0, op%start == 0 .and. .not. ctx%live3)
    rc = ndsmk_mem_info(fr, tot); if (rc /= 0) return
    if (real(nb, wp) * real(k, wp) + 2.0_wp * real(pl3, wp) + real(wk, wp) > real(tot, wp)) then
      rc = ndsmk_note_error(NDSMK_ENODEV, "the grid needs more device memory than the device has"//c_null_char)
      return
    end if
    ! [B1 | Omega 0, Omega 1 | work], and for the host entry [B0 | w | Bobs | wm]
    total = 9_c_size_t * nb + wk
    if (.not. on_device) then
      total = total + merge(4_c_size_t, 3_c_size_t, c_associated(op%w)) * nb
      if (obs) total = total + merge(2_c_size_t, 1_c_size_t, c_associated(op%wm)) * pl3
    end if
    rc = ndsmk_alloc(buf, total); if (rc /= 0) return
    dB1 = buf
    dO = dptr_offset(buf, 3_c_size_t * nb)
    dwork = dptr_offset(buf, 9_c_size_t * nb)
    if (on_device) then
      dB0 = pB; dw = op%w; dbobs = op%bobs; dwm = op%wm
    else
      ! (the work area's size is a multiple of 8 bytes, so every array behind it is aligned as a double)
      at = 9_c_size_t * nb + wk
      dB0 = dptr_offset(buf, at)
      rc = ndsmk_h2d(dB0, pB, 3_c_size_t * nb); if (rc /= 0) goto 900
      at = at + 3_c_size_t * nb
      dw = c_null_ptr
      if (c_associated(op%w)) then
        dw = dptr_offset(buf, at)
        rc = ndsmk_h2d(dw, op%w, nb); if (rc /= 0) goto 900
        at = at + nb
      end if
      dbobs = c_null_ptr
      if (obs) then
        dbobs = dptr_offset(buf, at)
        rc = ndsmk_h2d(dbobs, op%bobs, pl3); if (rc /= 0) goto 900
        at = at + pl3
      end if
      dwm = c_null_ptr
      if (c_associated(op%wm)) then
        dwm = dptr_offset(buf, at)
        rc = ndsmk_h2d(dwm, op%wm, pl3); if (rc /= 0) goto 900
      end if
    end if

    rc = optimize_start(ctx, iopt, ropt, op%start, dB0, dB1, dO, n3, nb); if (rc /= 0) goto 900

    if (obs) then
      call say("optimize_obs", "Descent...")
      rc = ndsmk_optimize_obs_begin(dB0, dB1, dO, dw, dbobs, dwm, dwork, n3, dq, op%nu, op%dt0, op%dt_min)
    else
      call say("optimize", "Descent...")
      rc = ndsmk_optimize_begin(dB0, dB1, dO, dw, dwork, n3, dq, op%dt0, op%dt_min)
    end if
    if (rc /= 0) goto 900
    rc = row(); if (rc /= 0) goto 900
    call descent_open(lp, op%descent_ctl, merge(7, 6, obs))
    do while (descent_more(lp, op%descent_ctl))
      if (obs) then
        rc = ndsmk_optimize_obs_tries(dB0, dB1, dO, dw, dbobs, dwm, dwork, n3, dq, op%nu, op%free, op%dt_min, lp%n)
      else
        rc = ndsmk_optimize_tries(dB0, dB1, dO, dw, dwork, n3, dq, op%dt_min, lp%n)
      end if
      if (rc /= 0) goto 900
      rc = row(); if (rc /= 0) goto 900
      call descent_note(lp, op%descent_ctl)
    end do
    rc = descent_close(lp, op%descent_ctl, dB0, dB1, 3_c_size_t * nb, pB, on_device)
900 continue
    if (rc /= 0) op%info = 0
    call unstage(rc, [buf])
  contains
    function row() result(rc)
      integer(c_int) :: rc
      if (obs) then
        rc = ndsmk_optimize_obs_row(dwork, lp%row)
      else
        rc = ndsmk_optimize_row(dwork, lp%row)
      end if
    end function
  end function

  ! vecpot_optimize with the measurement term and the freed lower face: the observation op%bobs is required
  function vecpot_optimize_obs(ctx, iopt, ropt, pB, op, on_device) result(rc)
    type(vecpot_ctx), intent(inout), target :: ctx
    integer(ik), intent(inout) :: iopt(0:OPT_LEN - 1)
    real(wp), intent(inout) :: ropt(0:OPT_LEN - 1)
    type(c_ptr), intent(in) :: pB
    type(optimize_args), intent(inout) :: op
    logical, intent(in) :: on_device
    integer(c_int) :: rc
    rc = NDSMK_EARG
    if (c_associated(op%bobs)) rc = vecpot_optimize(ctx, iopt, ropt, pB, op, on_device)
  end function

  ! The start field of an optimization-method call, in dB0 (DEVICE).  start = 1: the input as it is.  start = 0: the
  ! potential field of the input's B.n with the input's k = 0 plane put back; dB1 keeps the input meanwhile and dO
  ! (Omega 0's place) holds the zero guess of A.  iopt(IOPT_IERR) = 1 when a solve missed vc_tol, else 0.
  function optimize_start(ctx, iopt, ropt, start, dB0, dB1, dO, n3, nb) result(rc)
    type(vecpot_ctx), intent(inout), target :: ctx
    integer(ik), intent(inout) :: iopt(0:OPT_LEN - 1)
    real(wp), intent(inout) :: ropt(0:OPT_LEN - 1)
    integer(c_int), intent(in) :: start
    type(c_ptr), intent(in) :: dB0, dB1, dO
    integer(c_int32_t), intent(in) :: n3(3)
    integer(c_size_t), intent(in) :: nb
    integer(c_int) :: rc
    integer(c_size_t) :: plane
    integer :: c
    rc = 0
    if (start /= 0) then
      iopt(IOPT_IERR) = 0
      return
    end if
    call say("optimize", "Potential start field...")
    rc = ndsmk_d2d(dB1, dB0, 3_c_size_t * nb); if (rc /= 0) return            ! (the magnetogram comes back from here)
    rc = ndsmk_fill0(dO, 3_c_size_t * nb); if (rc /= 0) return                ! A: a zero guess, in Omega 0's place
    rc = ndsmk_sync(); if (rc /= 0) return
    rc = vecpot_run(ctx, iopt, ropt, dO, dB0, .true., VP_POTENTIAL); if (rc /= 0) return
    iopt(IOPT_IERR) = merge(1_ik, 0_ik, iopt(IOPT_IERR) /= 0 .or. iopt(IOPT_FAIL3D) /= 0)
    plane = int(n3(1), c_size_t) * int(n3(2), c_size_t) * 8_c_size_t
    do c = 0, 2
      rc = ndsmk_d2d(dptr_offset(dB0, int(c, c_size_t) * nb), dptr_offset(dB1, int(c, c_size_t) * nb), plane)
      if (rc /= 0) return
    end do
  end function

  ! ------------------------------------------------------------------
  ! The coarse-to-fine cascade of the optimization method (semantics in include/ndsm_hip.h, DESIGN.md "Coarse-to-fine
  ! cascade").  lev(1) is the finest context - pB and ops(1)%w live on its mesh, on the HOST (both go up once, B comes
  ! home once) or (on_device) in HBM -, lev(2:) the coarser ones on the same box; ops(l) carries level l's niter_max,
  ! dt0, dt_min and history (HOST), its w and start are set here.  One level is vecpot_optimize itself.  Otherwise:
  ! G_l = the hat average of the input B and w_l = the interpolated w on every coarser level, straight from the finest;
  ! the coarsest level runs from G_L with the caller's start; every finer level starts from the interpolated result of
  ! the level below with the k = 0 plane (start 0) or the six faces (start 1) of G_l pasted over it.  Level 1's start
  ! is interpolated into the caller's device B, whose input stands beside it only until the faces are pasted: each
  ! level's buffers are freed before the next finer level allocates, so the peak is vecpot_optimize's on the finest.
  ! iopt, ropt: the options and results of the coarsest level's potential solve.
  ! With ops(1)%bobs every level is the measurement fit (DESIGN.md "Cascade of the measurement fit"): ops(1)%bobs
  ! (nx,ny,3), ops(1)%wm (the same; may be c_null_ptr) and ops(1)%free on the finest mesh, on the side B is on - the
  ! host entry stages the two planes once, behind B and w -, ops(l)%nu per level.  (Bobs_l, wm_l) = the
  ! confidence-weighted restriction of the two planes, straight from the finest (without wm: the hat average of Bobs);
  ! they lie behind G_l and w_l in the level's buffer.  With free = 1 the paste of a finer level leaves out the freed
  ! nodes of the k = 0 plane (which = start + 2): they keep the interpolated values the level below has fitted.
  ! ------------------------------------------------------------------
  function vecpot_optimize_cascade(lev, iopt, ropt, pB, ops, on_device) result(rc)
    type(vecpot_ref), intent(in) :: lev(:)
    integer(ik), intent(inout) :: iopt(0:OPT_LEN - 1)
    real(wp), intent(inout) :: ropt(0:OPT_LEN - 1)
    type(c_ptr), intent(in) :: pB
    type(optimize_args), intent(inout) :: ops(:)
    logical, intent(in) :: on_device
    integer(c_int) :: rc
    integer(c_int32_t) :: n3(3, size(lev)), n2(3, size(lev))
    integer(c_size_t) :: nb(size(lev)), pl3(size(lev)), wk, fr, tot, at
    integer(ik) :: iopt1(0:OPT_LEN - 1)
    real(wp) :: ropt1(0:OPT_LEN - 1)
    type(c_ptr) :: gb(size(lev)), bb(size(lev)), stage, keep, dB, dw, dbobs, dwm, dcur, dprev
    integer(c_int) :: start, which
    integer :: l, nl
    logical :: has_w, obs, has_wm

    nl = size(lev)
    start = ops(1)%start
    if (nl == 1) then
      rc = vecpot_optimize(lev(1)%p, iopt, ropt, pB, ops(1), on_device)
      return
    end if
    gb = c_null_ptr; bb = c_null_ptr; stage = c_null_ptr; keep = c_null_ptr
    has_w = c_associated(ops(1)%w)
    obs = c_associated(ops(1)%bobs)
    has_wm = obs .and. c_associated(ops(1)%wm)
    do l = 1, nl
      ops(l)%info = 0
      n3(:, l) = lev(l)%p%n3
      n2(:, l) = [n3(1, l), n3(2, l), 1_c_int32_t]
      nb(l) = int(product(int(n3(:, l), ik)), c_size_t) * 8_c_size_t
      pl3(l) = 0
      if (obs) pl3(l) = int(n3(1, l), c_size_t) * int(n3(2, l), c_size_t) * 24_c_size_t   ! a plane of three components
    end do
    ! the finest level's call, the largest by far, is vecpot_optimize's 13 level-1 arrays (and the two planes)
    if (obs) then
      wk = ndsmk_optimize_obs_work_bytes()
    else
      wk = ndsmk_optimize_work_bytes()
    end if
    rc = ndsmk_mem_info(fr, tot); if (rc /= 0) return
    if (real(nb(1), wp) * 13.0_wp + 2.0_wp * real(pl3(1), wp) + real(wk, wp) > real(tot, wp)) then
      rc = ndsmk_note_error(NDSMK_ENODEV, "the grid needs more device memory than the device has"//c_null_char)
      return
    end if
    if (on_device) then
      dB = pB; dw = ops(1)%w; dbobs = ops(1)%bobs; dwm = ops(1)%wm
    else
      ! [B | w | Bobs | wm]
      rc = ndsmk_alloc(stage, merge(4_c_size_t, 3_c_size_t, has_w) * nb(1) + merge(2_c_size_t, 1_c_size_t, has_wm) * pl3(1))
      if (rc /= 0) goto 900
      dB = stage
      rc = ndsmk_h2d(dB, pB, 3_c_size_t * nb(1)); if (rc /= 0) goto 900
      at = 3_c_size_t * nb(1)
      dw = c_null_ptr
      if (has_w) then
        dw = dptr_offset(stage, at)
        rc = ndsmk_h2d(dw, ops(1)%w, nb(1)); if (rc /= 0) goto 900
        at = at + nb(1)
      end if
      dbobs = c_null_ptr
      if (obs) then
        dbobs = dptr_offset(stage, at)
        rc = ndsmk_h2d(dbobs, ops(1)%bobs, pl3(1)); if (rc /= 0) goto 900
        at = at + pl3(1)
      end if
      dwm = c_null_ptr
      if (has_wm) then
        dwm = dptr_offset(stage, at)
        rc = ndsmk_h2d(dwm, ops(1)%wm, pl3(1)); if (rc /= 0) goto 900
      end if
    end if

    call say("optimize", "Cascade: level data...")
    do l = 2, nl
      ! [G_l | w_l | Bobs_l | wm_l]
      rc = ndsmk_alloc(gb(l), merge(4_c_size_t, 3_c_size_t, has_w) * nb(l) + merge(2_c_size_t, 1_c_size_t, has_wm) * pl3(l))
      if (rc /= 0) goto 900
      rc = ndsmk_resample(n3(:, 1), n3(:, l), 3_c_int, 1_c_int, dB, gb(l)); if (rc /= 0) goto 900
      at = 3_c_size_t * nb(l)
      ops(l)%w = c_null_ptr
      if (has_w) then
        ops(l)%w = dptr_offset(gb(l), at)
        rc = ndsmk_resample(n3(:, 1), n3(:, l), 1_c_int, 0_c_int, dw, ops(l)%w); if (rc /= 0) goto 900
        at = at + nb(l)
      end if
      ops(l)%bobs = c_null_ptr; ops(l)%wm = c_null_ptr
      if (obs) then
        ops(l)%free = ops(1)%free
        ops(l)%bobs = dptr_offset(gb(l), at)
        if (has_wm) then
          ops(l)%wm = dptr_offset(gb(l), at + pl3(l))
          rc = ndsmk_resample_weighted(n2(:, 1), n2(:, l), 3_c_int, dbobs, dwm, ops(l)%bobs, ops(l)%wm)
        else
          rc = ndsmk_resample(n2(:, 1), n2(:, l), 3_c_int, 1_c_int, dbobs, ops(l)%bobs)
        end if
        if (rc /= 0) goto 900
      end if
    end do
    ! a freed lower face keeps the values interpolated from the level below: the pastes leave its nodes out
    which = start
    if (obs) then
      if (ops(1)%free == 1) which = start + 2_c_int
    end if

    ! the coarsest level: G_L is its start field (start 1) or carries its magnetogram and B.n (start 0)
    ops(nl)%start = start
    rc = vecpot_optimize(lev(nl)%p, iopt, ropt, gb(nl), ops(nl), .true.); if (rc /= 0) goto 900
    dprev = gb(nl)
    do l = nl - 1, 1, -1
      if (l > 1) then
        rc = ndsmk_alloc(bb(l), 3_c_size_t * nb(l)); if (rc /= 0) goto 900
        dcur = bb(l)
        rc = ndsmk_resample(n3(:, l + 1), n3(:, l), 3_c_int, 0_c_int, dprev, dcur); if (rc /= 0) goto 900
        rc = ndsmk_paste_faces(n3(:, l), 3_c_int, which, gb(l), dcur); if (rc /= 0) goto 900
      else
        ! G_0 is the input itself: it stands aside while level 1's start is interpolated into the caller's array
        rc = ndsmk_alloc(keep, 3_c_size_t * nb(1)); if (rc /= 0) goto 900
        rc = ndsmk_d2d(keep, dB, 3_c_size_t * nb(1)); if (rc /= 0) goto 900
        dcur = dB
        rc = ndsmk_resample(n3(:, 2), n3(:, 1), 3_c_int, 0_c_int, dprev, dcur); if (rc /= 0) goto 900
        rc = ndsmk_paste_faces(n3(:, 1), 3_c_int, which, keep, dcur); if (rc /= 0) goto 900
      end if
      rc = ndsmk_sync(); if (rc /= 0) goto 900
      ! the level below is done with: its buffers go before this level's call allocates
      call unstage(rc, [keep, bb(l + 1), gb(l + 1)])
      keep = c_null_ptr; bb(l + 1) = c_null_ptr; gb(l + 1) = c_null_ptr
      if (rc /= 0) goto 900
      if (l == 1) then
        ops(1)%w = dw; ops(1)%bobs = dbobs; ops(1)%wm = dwm
      end if
      ops(l)%start = 1
      iopt1 = iopt; ropt1 = ropt
      rc = vecpot_optimize(lev(l)%p, iopt1, ropt1, dcur, ops(l), .true.); if (rc /= 0) goto 900
      dprev = dcur
    end do
    if (.not. on_device) then
      rc = ndsmk_d2h(pB, dB, 3_c_size_t * nb(1)); if (rc /= 0) goto 900
    end if
    rc = ndsmk_sync()
900 continue
    if (rc /= 0) then
      do l = 1, nl
        ops(l)%info = 0
      end do
    end if
    call unstage(rc, [keep, stage])
    call unstage(rc, gb)
    call unstage(rc, bb)
  end function

  ! ------------------------------------------------------------------
  ! Magnetogram preprocessing on a prepared context (semantics in include/ndsm_hip.h, DESIGN.md "Magnetogram
  ! preprocessing").  pB (nx,ny,3) in and out and pp%obs (the same; may be c_null_ptr: the input B) in, on the HOST
  ! (both go up once, B comes home once; between the two only history rows cross PCIe) or (on_device) in HBM; pp%hist
  ! on the HOST.  The context supplies the mesh of its lower face only - no solve, no hierarchy, nothing kept on it.
  ! One buffer holds the second field, the two Lambda, the observation and the state for the length of the call.  The
  ! tries of one check interval are queued without a read-back: the device decides each (preprocess.hip).
  ! ------------------------------------------------------------------
  function vecpot_preprocess(ctx, pB, pp, on_device) result(rc)
    type(vecpot_ctx), intent(inout), target :: ctx
    type(c_ptr), intent(in) :: pB
    type(preprocess_args), intent(inout) :: pp
    logical, intent(in) :: on_device
    integer(c_int) :: rc
    real(wp) :: dq(3), lo(3)
    integer(c_int32_t) :: n3(3)
    integer(c_size_t) :: nb, wk, total, fr, tot
    type(descent_loop) :: lp
    type(c_ptr) :: buf, dB0, dB1, dLa, dobs, dwork

    pp%info = 0
    buf = c_null_ptr
    call ctx_mesh(ctx, n3, lo, dq)
    nb = int(n3(1), c_size_t) * int(n3(2), c_size_t) * 24_c_size_t          ! one field of the plane
    wk = ndsmk_preprocess_work_bytes()
    ! [B1 | Lambda 0, Lambda 1 | obs | work], and for the host entry [B0]
    total = 4_c_size_t * nb + wk
    if (.not. on_device) total = total + nb
    rc = ndsmk_mem_info(fr, tot); if (rc /= 0) return
    if (real(total, wp) + merge(real(nb, wp), 0.0_wp, on_device) > real(tot, wp)) then
      rc = ndsmk_note_error(NDSMK_ENODEV, "the plane needs more device memory than the device has"//c_null_char)
      return
    end if
    rc = ndsmk_alloc(buf, total); if (rc /= 0) return
    dB1 = buf
    dLa = dptr_offset(buf, nb)
    dobs = dptr_offset(buf, 3_c_size_t * nb)
    dwork = dptr_offset(buf, 4_c_size_t * nb)
    if (on_device) then
      dB0 = pB
      if (c_associated(pp%obs)) then
        rc = ndsmk_d2d(dobs, pp%obs, nb)
      else
        rc = ndsmk_d2d(dobs, pB, nb)
      end if
      if (rc /= 0) goto 900
    else
      dB0 = dptr_offset(buf, 4_c_size_t * nb + wk)
      rc = ndsmk_h2d(dB0, pB, nb); if (rc /= 0) goto 900
      if (c_associated(pp%obs)) then
        rc = ndsmk_h2d(dobs, pp%obs, nb)
      else
        rc = ndsmk_d2d(dobs, dB0, nb)
      end if
      if (rc /= 0) goto 900
    end if

    call say("preprocess", "Descent...")
    rc = ndsmk_preprocess_begin(dB0, dB1, dLa, dobs, dwork, n3(1:2), dq(1:2), pp%mu, pp%dt0, pp%dt_min)
    if (rc /= 0) goto 900
    rc = ndsmk_preprocess_row(dwork, lp%row); if (rc /= 0) goto 900
    if (.not. (lp%row(20) > 0.0_wp .and. lp%row(21) > 0.0_wp)) then
      rc = ndsmk_note_error(NDSMK_EVALUE, "preprocess: the observation needs sum W |B|^2 > 0 and sum W r |B|^2 > 0"// &
                            c_null_char)
      goto 900
    end if
    call descent_open(lp, pp%descent_ctl, 17)
    do while (descent_more(lp, pp%descent_ctl))
      rc = ndsmk_preprocess_tries(dB0, dB1, dLa, dobs, dwork, n3(1:2), dq(1:2), pp%mu, pp%dt_min, lp%n)
      if (rc /= 0) goto 900
      rc = ndsmk_preprocess_row(dwork, lp%row); if (rc /= 0) goto 900
      call descent_note(lp, pp%descent_ctl)
    end do
    rc = descent_close(lp, pp%descent_ctl, dB0, dB1, nb, pB, on_device)
900 continue
    if (rc /= 0) pp%info = 0
    call unstage(rc, [buf])
  end function

  ! ------------------------------------------------------------------
  ! The path entries on a prepared context (semantics in include/ndsm_hip.h, DESIGN.md "Field-line paths"): the
  ! points of the lines that vecpot_lines traces, with B, G and the running integral at each.  The context supplies
  ! the mesh only, as in vecpot_lines: no solve, no hierarchy.  pB, pG, pseeds and the five trace outputs as there
  ! (sel = direction); every >= 1 the stride, max_points >= 0 the capacity of the point arrays; poff (nl + 1, int64)
  ! and total out; ppts (3,max_points), pbpt, pgpt (the same; c_null_ptr: skipped), pipt (max_points; likewise) out -
  ! on the HOST (B and G go up into the staging arrays dF(1) and dF(2), the seeds and the line outputs into a scratch
  ! buffer; after the counting half a second buffer of min(total, max_points) points is allocated, filled, and only
  ! what was written comes home) or (on_device) in HBM.  total is a host scalar either way.
  ! ------------------------------------------------------------------
  function vecpot_paths(ctx, pB, pG, sel, nseeds, pseeds, step, max_steps, every, max_points, pends, plen, pint, &
                        pstat, pnst, poff, total, ppts, pbpt, pgpt, pipt, on_device) result(rc)
    type(vecpot_ctx), intent(inout), target :: ctx
    logical, intent(in) :: on_device
    type(c_ptr), intent(in) :: pB, pG, pseeds, pends, plen, pint, pstat, pnst, poff, ppts, pbpt, pgpt, pipt
    integer(c_int), intent(in) :: sel, nseeds, max_steps, every
    integer(c_int64_t), intent(in) :: max_points
    real(wp), intent(in) :: step
    integer(c_int64_t), intent(out) :: total
    integer(c_int) :: rc
    real(wp) :: dq(3), lo(3)
    integer(c_int32_t) :: n3(3)
    integer(c_size_t) :: nl, ns, np
    type(c_ptr) :: dG, buf, pbuf
    type(slice) :: s(7), pt(4)

    total = 0
    call ctx_mesh(ctx, n3, lo, dq)
    if (on_device .or. nseeds <= 0 .or. step <= 0.0_wp .or. max_steps < 1 .or. sel < -1 .or. sel > 1 .or. &
        every < 1 .or. max_points < 0) then
      ! (the argument errors are the kernel entries' to name; nothing is staged for them)
      rc = ndsmk_paths_count(pB, pG, n3, lo, dq, nseeds, pseeds, step, max_steps, sel, every, max_points, pends, plen, &
                             pint, pstat, pnst, poff, total)
      if (rc == 0) rc = ndsmk_paths_fill(pB, pG, n3, lo, dq, nseeds, pseeds, step, max_steps, sel, every, max_points, &
                                         poff, ppts, pbpt, pgpt, pipt)
      if (rc == 0) rc = ndsmk_sync()
      if (rc /= 0) total = 0
      return
    end if
    ns = int(nseeds, c_size_t)
    nl = ns * merge(2_c_size_t, 1_c_size_t, sel == 0)
    ! the helicity entries' host staging: dF(1) B, dF(2) G
    rc = stage_field(ctx, 1, pB); if (rc /= 0) return
    dG = c_null_ptr
    if (c_associated(pG)) then
      rc = stage_field(ctx, 2, pG); if (rc /= 0) return
      dG = ctx%dF(2)
    end if
    pbuf = c_null_ptr
    s = [slice(pseeds, 24, ns, GOES_UP), slice(pends, 24, nl, COMES_HOME), slice(plen, 8, nl, COMES_HOME), &
         slice(pint, 8, nl, COMES_HOME), slice(pstat, 4, nl, COMES_HOME), slice(pnst, 4, nl, COMES_HOME), &
         slice(poff, 8, nl + 1, COMES_HOME)]
    rc = carve(buf, s)
    if (rc == 0) then
      call say("trace_paths", "Tracing field lines and counting their points...")
      rc = ndsmk_paths_count(ctx%dF(1), dG, n3, lo, dq, nseeds, s(1)%dev, step, max_steps, sel, every, max_points, &
                             s(2)%dev, s(3)%dev, s(4)%dev, s(5)%dev, s(6)%dev, s(7)%dev, total)
    end if
    ! the point arrays: min(total, max_points) slots each, carved from a second buffer (gpt, ipt: with G only)
    np = 0
    if (rc == 0) np = int(min(total, max_points), c_size_t)
    if (rc == 0 .and. np > 0) then
      pt = [slice(ppts, 24, np, COMES_HOME), slice(pbpt, 24, np, COMES_HOME), &
            slice(merge(pgpt, c_null_ptr, c_associated(pG)), 24, np, COMES_HOME), &
            slice(merge(pipt, c_null_ptr, c_associated(pG)), 8, np, COMES_HOME)]
      rc = carve(pbuf, pt)
      if (rc == 0) then
        call say("trace_paths", "Tracing again and storing the points...")
        rc = ndsmk_paths_fill(ctx%dF(1), dG, n3, lo, dq, nseeds, s(1)%dev, step, max_steps, sel, every, &
                              int(np, c_int64_t), s(7)%dev, pt(1)%dev, pt(2)%dev, pt(3)%dev, pt(4)%dev)
      end if
    end if
    if (rc == 0) rc = fetch(s)
    if (rc == 0 .and. np > 0) rc = fetch(pt)
    if (rc == 0) rc = ndsmk_sync()
    call unstage(rc, [pbuf, buf], total)
  end function

  ! ------------------------------------------------------------------
  ! The skeleton entries on a prepared context (semantics in include/ndsm_hip.h, DESIGN.md "Spine-fan skeleton"): the
  ! type of each null from its Jacobian, then its two spine lines and nring fan lines, traced away from it and ended
  ! where they come within `capture` of another null.  The context supplies the mesh only, as in vecpot_lines: no
  ! solve, no hierarchy.  pB (nx,ny,nz,3), ppos (3,nnulls), pjac (9 each), pring (2,nring) in; per null pkind, peig,
  ! pspine, pnormal out; per line (nl = nnulls (2 + nring)) pends, plen, pstat, pnst, phit out; poff (nl + 1, int64),
  ! total, ppts (3,max_points), pbpt (the same; c_null_ptr: skipped) as vecpot_paths - on the HOST (B goes up into the
  ! staging array dF(1), the nulls, the ring and the outputs into a scratch buffer; after the counting half a second
  ! buffer of min(total, max_points) points is allocated, filled, and only what was written comes home) or (on_device)
  ! in HBM.  total is a host scalar either way.
  ! ------------------------------------------------------------------
  function vecpot_skeleton(ctx, pB, nnulls, ppos, pjac, nring, pring, radius, capture, step, max_steps, every, &
                           max_points, pkind, peig, pspine, pnormal, pends, plen, pstat, pnst, phit, poff, total, &
                           ppts, pbpt, on_device) result(rc)
    type(vecpot_ctx), intent(inout), target :: ctx
    logical, intent(in) :: on_device
    type(c_ptr), intent(in) :: pB, ppos, pjac, pring, pkind, peig, pspine, pnormal, pends, plen, pstat, pnst, phit, poff, &
                               ppts, pbpt
    integer(c_int), intent(in) :: nnulls, nring, max_steps, every
    integer(c_int64_t), intent(in) :: max_points
    real(wp), intent(in) :: radius, capture, step
    integer(c_int64_t), intent(out) :: total
    integer(c_int) :: rc
    real(wp) :: dq(3), lo(3)
    integer(c_int32_t) :: n3(3)
    integer(c_size_t) :: nl, nm, nr, np
    type(c_ptr) :: buf, pbuf
    type(slice) :: s(13), pt(2)

    total = 0
    call ctx_mesh(ctx, n3, lo, dq)
    if (on_device .or. nnulls <= 0 .or. nring < 0 .or. step <= 0.0_wp .or. max_steps < 1 .or. every < 1 .or. &
        max_points < 0 .or. .not. (radius > 0.0_wp) .or. .not. (capture >= 0.0_wp) .or. radius > 1.0e300_wp .or. &
        capture > 1.0e300_wp .or. .not. (step <= 1.0e300_wp) .or. &
        int(nnulls, c_int64_t) * (2_c_int64_t + int(nring, c_int64_t)) > 2147483647_c_int64_t) then
      ! (the argument errors, more lines than a call takes among them, are the kernel entries' to name; nothing is
      ! staged for them)
      rc = ndsmk_skel_count(pB, n3, lo, dq, nnulls, ppos, pjac, nring, pring, radius, capture, step, max_steps, every, &
                            max_points, pkind, peig, pspine, pnormal, pends, plen, pstat, pnst, phit, poff, total)
      if (rc == 0) rc = ndsmk_skel_fill(pB, n3, lo, dq, nnulls, ppos, nring, radius, capture, step, max_steps, every, &
                                        max_points, poff, ppts, pbpt)
      if (rc == 0) rc = ndsmk_sync()
      if (rc /= 0) total = 0
      return
    end if
    nm = int(nnulls, c_size_t)
    nr = int(nring, c_size_t)
    nl = nm * (2_c_size_t + nr)
    rc = stage_field(ctx, 1, pB); if (rc /= 0) return
    pbuf = c_null_ptr
    ! (nring = 0: an empty slice, so the kernel entry gets c_null_ptr for ring, which it takes when nring <= 0)
    s = [slice(ppos, 24, nm, GOES_UP), slice(pjac, 72, nm, GOES_UP), slice(pring, 16, nr, GOES_UP), &
         slice(pkind, 4, nm, COMES_HOME), slice(peig, 24, nm, COMES_HOME), slice(pspine, 24, nm, COMES_HOME), &
         slice(pnormal, 24, nm, COMES_HOME), slice(pends, 24, nl, COMES_HOME), slice(plen, 8, nl, COMES_HOME), &
         slice(pstat, 4, nl, COMES_HOME), slice(pnst, 4, nl, COMES_HOME), slice(phit, 4, nl, COMES_HOME), &
         slice(poff, 8, nl + 1, COMES_HOME)]
    rc = carve(buf, s)
    if (rc == 0) then
      call say("find_skeleton", "Typing the nulls, tracing their spines and fans and counting the points...")
      rc = ndsmk_skel_count(ctx%dF(1), n3, lo, dq, nnulls, s(1)%dev, s(2)%dev, nring, s(3)%dev, radius, capture, step, &
                            max_steps, every, max_points, s(4)%dev, s(5)%dev, s(6)%dev, s(7)%dev, s(8)%dev, s(9)%dev, &
                            s(10)%dev, s(11)%dev, s(12)%dev, s(13)%dev, total)
    end if
    ! the point arrays: min(total, max_points) slots each, carved from a second buffer
    np = 0
    if (rc == 0) np = int(min(total, max_points), c_size_t)
    if (rc == 0 .and. np > 0) then
      pt = [slice(ppts, 24, np, COMES_HOME), slice(pbpt, 24, np, COMES_HOME)]
      rc = carve(pbuf, pt)
      if (rc == 0) then
        call say("find_skeleton", "Tracing again and storing the points...")
        rc = ndsmk_skel_fill(ctx%dF(1), n3, lo, dq, nnulls, s(1)%dev, nring, radius, capture, step, max_steps, every, &
                             int(np, c_int64_t), s(13)%dev, pt(1)%dev, pt(2)%dev)
      end if
    end if
    if (rc == 0) rc = fetch(s)
    if (rc == 0 .and. np > 0) rc = fetch(pt)
    if (rc == 0) rc = ndsmk_sync()
    call unstage(rc, [pbuf, buf], total)
  end function

  ! ------------------------------------------------------------------
  ! The separator entries on a prepared context (semantics in include/ndsm_hip.h, DESIGN.md "Separator lines"): each
  ! bracket - an arc (a, b) of the fan ring of null m and a null m' of the other sign - is refined by one wave until the
  ! arc is narrower than tol, and the fan line of its a side is stored as the skeleton stores a line.  The context
  ! supplies the mesh only, as in vecpot_skeleton.  pB (nx,ny,nz,3), ppos (3,nnulls), pkind (nnulls; int32), pnormal
  ! (3,nnulls), ppair (2,nbr; int32), parc (4,nbr) in; per bracket pstate, pnrounds, pside (int32), pcoef (4), pwidth,
  ! pdmin (2), pends (3), plen, pstat, pnst out; poff (nbr + 1, int64), total, ppts (3,max_points), pbpt (the same;
  ! c_null_ptr: skipped) as vecpot_skeleton - on the HOST (staged as there) or (on_device) in HBM.  total is a host scalar
  ! either way.
  ! ------------------------------------------------------------------
  function vecpot_separators(ctx, pB, nnulls, ppos, pkind, pnormal, nbr, ppair, parc, radius, capture, step, max_steps, &
                             rounds, tol, every, max_points, pstate, pnrounds, pcoef, pwidth, pside, pdmin, pends, plen, &
                             pstat, pnst, poff, total, ppts, pbpt, on_device) result(rc)
    type(vecpot_ctx), intent(inout), target :: ctx
    logical, intent(in) :: on_device
    type(c_ptr), intent(in) :: pB, ppos, pkind, pnormal, ppair, parc, pstate, pnrounds, pcoef, pwidth, pside, pdmin, &
                               pends, plen, pstat, pnst, poff, ppts, pbpt
    integer(c_int), intent(in) :: nnulls, nbr, max_steps, rounds, every
    integer(c_int64_t), intent(in) :: max_points
    real(wp), intent(in) :: radius, capture, step, tol
    integer(c_int64_t), intent(out) :: total
    integer(c_int) :: rc
    real(wp) :: dq(3), lo(3)
    integer(c_int32_t) :: n3(3)
    integer(c_size_t) :: nm, nq, np
    type(c_ptr) :: buf, pbuf
    type(slice) :: s(16), pt(2)

    total = 0
    call ctx_mesh(ctx, n3, lo, dq)
    if (on_device .or. nbr <= 0 .or. nnulls <= 0 .or. step <= 0.0_wp .or. max_steps < 1 .or. every < 1 .or. &
        rounds < 1 .or. max_points < 0 .or. .not. (radius > 0.0_wp) .or. .not. (capture > 0.0_wp) .or. &
        radius > 1.0e300_wp .or. capture > 1.0e300_wp .or. .not. (step <= 1.0e300_wp) .or. .not. (tol >= 0.0_wp) .or. &
        tol > 1.0e300_wp .or. int(nbr, c_int64_t) * 64_c_int64_t > 2147483647_c_int64_t) then
      ! (the argument errors, more brackets than a call takes among them, are the kernel entries' to name; nothing is
      ! staged for them)
      rc = ndsmk_sep_count(pB, n3, lo, dq, nnulls, ppos, pkind, pnormal, nbr, ppair, parc, radius, capture, step, &
                           max_steps, rounds, tol, every, max_points, pstate, pnrounds, pcoef, pwidth, pside, pdmin, &
                           pends, plen, pstat, pnst, poff, total)
      if (rc == 0) rc = ndsmk_sep_fill(pB, n3, lo, dq, nnulls, ppos, nbr, ppair, radius, capture, step, max_steps, rounds, &
                                       tol, every, max_points, poff, ppts, pbpt)
      if (rc == 0) rc = ndsmk_sync()
      if (rc /= 0) total = 0
      return
    end if
    nm = int(nnulls, c_size_t)
    nq = int(nbr, c_size_t)
    rc = stage_field(ctx, 1, pB); if (rc /= 0) return
    pbuf = c_null_ptr
    s = [slice(ppos, 24, nm, GOES_UP), slice(pkind, 4, nm, GOES_UP), slice(pnormal, 24, nm, GOES_UP), &
         slice(ppair, 8, nq, GOES_UP), slice(parc, 32, nq, GOES_UP), &
         slice(pstate, 4, nq, COMES_HOME), slice(pnrounds, 4, nq, COMES_HOME), slice(pcoef, 32, nq, COMES_HOME), &
         slice(pwidth, 8, nq, COMES_HOME), slice(pside, 4, nq, COMES_HOME), slice(pdmin, 16, nq, COMES_HOME), &
         slice(pends, 24, nq, COMES_HOME), slice(plen, 8, nq, COMES_HOME), slice(pstat, 4, nq, COMES_HOME), &
         slice(pnst, 4, nq, COMES_HOME), slice(poff, 8, nq + 1, COMES_HOME)]
    rc = carve(buf, s)
    if (rc == 0) then
      call say("find_separators", "Refining the brackets, tracing the separators and counting the points...")
      rc = ndsmk_sep_count(ctx%dF(1), n3, lo, dq, nnulls, s(1)%dev, s(2)%dev, s(3)%dev, nbr, s(4)%dev, s(5)%dev, radius, &
                           capture, step, max_steps, rounds, tol, every, max_points, s(6)%dev, s(7)%dev, s(8)%dev, &
                           s(9)%dev, s(10)%dev, s(11)%dev, s(12)%dev, s(13)%dev, s(14)%dev, s(15)%dev, s(16)%dev, total)
    end if
    ! the point arrays: min(total, max_points) slots each, carved from a second buffer
    np = 0
    if (rc == 0) np = int(min(total, max_points), c_size_t)
    if (rc == 0 .and. np > 0) then
      pt = [slice(ppts, 24, np, COMES_HOME), slice(pbpt, 24, np, COMES_HOME)]
      rc = carve(pbuf, pt)
      if (rc == 0) then
        call say("find_separators", "Tracing again and storing the points...")
        rc = ndsmk_sep_fill(ctx%dF(1), n3, lo, dq, nnulls, s(1)%dev, nbr, s(4)%dev, radius, capture, step, max_steps, &
                            rounds, tol, every, int(np, c_int64_t), s(16)%dev, pt(1)%dev, pt(2)%dev)
      end if
    end if
    if (rc == 0) rc = fetch(s)
    if (rc == 0 .and. np > 0) rc = fetch(pt)
    if (rc == 0) rc = ndsmk_sync()
    call unstage(rc, [pbuf, buf], total)
  end function

  ! ------------------------------------------------------------------
  ! The null-point entries on a prepared context (semantics in include/ndsm_hip.h, DESIGN.md "Null points"): the
  ! screen over every cell of B and the Newton iteration of the candidates (ndsmk_nulls).  The context supplies the
  ! mesh only, as in vecpot_lines.  pB (nx,ny,nz,3) in; counts(2) out on the host: candidates, nulls found; the first
  ! min(counts(2), max_nulls) records in ascending cell order out: pcell int64, ppos (3 each), pjac (9 each), pdet,
  ! pres doubles, psign, pit int32 - on the HOST (B goes up into the staging array dF(1), the records come home from a
  ! scratch buffer) or (on_device) in HBM.
  ! ------------------------------------------------------------------
  function vecpot_nulls(ctx, pB, max_nulls, counts, pcell, ppos, pjac, pdet, pres, psign, pit, on_device) result(rc)
    type(vecpot_ctx), intent(inout), target :: ctx
    logical, intent(in) :: on_device
    type(c_ptr), intent(in) :: pB, pcell, ppos, pjac, pdet, pres, psign, pit
    integer(c_int), intent(in) :: max_nulls
    integer(c_int64_t), intent(out) :: counts(2)
    integer(c_int) :: rc
    real(wp) :: dq(3), lo(3)
    integer(c_int32_t) :: n3(3)
    integer(c_size_t) :: nm
    type(c_ptr) :: buf
    type(slice) :: s(7)

    counts = 0
    call ctx_mesh(ctx, n3, lo, dq)
    if (on_device .or. max_nulls < 0) then
      ! (the argument errors are the kernel entry's to name; nothing is staged for them)
      rc = ndsmk_nulls(pB, n3, lo, dq, max_nulls, counts, pcell, ppos, pjac, pdet, pres, psign, pit)
      if (rc == 0) rc = ndsmk_sync()
      return
    end if
    rc = stage_field(ctx, 1, pB); if (rc /= 0) return
    ! one scratch buffer of max_nulls records (none for max_nulls = 0: the arrays are c_null_ptr)
    nm = int(max_nulls, c_size_t)
    s = [slice(pcell, 8, nm, COMES_HOME), slice(ppos, 24, nm, COMES_HOME), slice(pjac, 72, nm, COMES_HOME), &
         slice(pdet, 8, nm, COMES_HOME), slice(pres, 8, nm, COMES_HOME), slice(psign, 4, nm, COMES_HOME), &
         slice(pit, 4, nm, COMES_HOME)]
    rc = carve(buf, s); if (rc /= 0) return
    call say("find_nulls", "Screening the cells and iterating on the candidates...")
    rc = ndsmk_nulls(ctx%dF(1), n3, lo, dq, max_nulls, counts, s(1)%dev, s(2)%dev, s(3)%dev, s(4)%dev, s(5)%dev, &
                     s(6)%dev, s(7)%dev)
    if (rc == 0) rc = fetch(s, rows=int(min(counts(2), int(max_nulls, c_int64_t)), c_size_t))
    if (rc == 0) rc = ndsmk_sync()
    call unstage(rc, [buf])
  end function

  ! ------------------------------------------------------------------
  ! The dip entries on a prepared context (semantics in include/ndsm_hip.h, DESIGN.md "Dips and bald patches"): the
  ! edges of the mesh on which B_z changes sign with (B.grad)B_z > 0 at the crossing (ndsmk_dips).  The context
  ! supplies the mesh only, as in vecpot_nulls; no solve.  pB (nx,ny,nz,3) in; plane_only 1: the plane k = 0 and its x
  ! and y edges alone; counts(3) out on the host: crossings, dips, bald patches; the first min(counts(2), max_dips)
  ! records in ascending edge order out: pedge int64, ppos, pbpt, pgrad (3 each), pcurv doubles, pflag int32 - on the
  ! HOST (B goes up into the staging array dF(1), the records come home from a scratch buffer) or (on_device) in HBM.
  ! ------------------------------------------------------------------
  function vecpot_dips(ctx, pB, plane_only, max_dips, counts, pedge, ppos, pbpt, pgrad, pcurv, pflag, on_device) result(rc)
    type(vecpot_ctx), intent(inout), target :: ctx
    logical, intent(in) :: on_device
    type(c_ptr), intent(in) :: pB, pedge, ppos, pbpt, pgrad, pcurv, pflag
    integer(c_int), intent(in) :: plane_only
    integer(c_int64_t), intent(in) :: max_dips
    integer(c_int64_t), intent(out) :: counts(3)
    integer(c_int) :: rc
    real(wp) :: dq(3), lo(3)
    integer(c_int32_t) :: n3(3)
    integer(c_size_t) :: nm
    type(c_ptr) :: buf
    type(slice) :: s(6)

    counts = 0
    call ctx_mesh(ctx, n3, lo, dq)
    if (on_device .or. max_dips < 0 .or. plane_only < 0 .or. plane_only > 1 .or. any(n3 < 3)) then
      ! (the argument errors are the kernel entry's to name; nothing is staged for them)
      rc = ndsmk_dips(pB, n3, lo, dq, plane_only, max_dips, counts, pedge, ppos, pbpt, pgrad, pcurv, pflag)
      if (rc == 0) rc = ndsmk_sync()
      return
    end if
    rc = stage_field(ctx, 1, pB); if (rc /= 0) return
    ! one scratch buffer of max_dips records (none for max_dips = 0: the arrays are c_null_ptr)
    nm = int(max_dips, c_size_t)
    s = [slice(pedge, 8, nm, COMES_HOME), slice(ppos, 24, nm, COMES_HOME), slice(pbpt, 24, nm, COMES_HOME), &
         slice(pgrad, 24, nm, COMES_HOME), slice(pcurv, 8, nm, COMES_HOME), slice(pflag, 4, nm, COMES_HOME)]
    rc = carve(buf, s); if (rc /= 0) return
    call say("find_dips", "Voting on the edges and filling the records...")
    rc = ndsmk_dips(ctx%dF(1), n3, lo, dq, plane_only, max_dips, counts, s(1)%dev, s(2)%dev, s(3)%dev, s(4)%dev, &
                    s(5)%dev, s(6)%dev)
    if (rc == 0) rc = fetch(s, rows=int(min(counts(2), max_dips), c_size_t))
    if (rc == 0) rc = ndsmk_sync()
    call unstage(rc, [buf])
  end function

  ! ------------------------------------------------------------------
  ! The connectivity entries on a prepared context (semantics in include/ndsm_hip.h, DESIGN.md "Flux partitioning and
  ! connectivity"): one field line from every labelled pixel of the lower face and the (patch, class) pairs
  ! (ndsmk_connect).  The context supplies the mesh, its x and y vectors being the seeds; no solve.  pB (nx,ny,nz,3) and
  ! plabel (nx,ny; int32) in; counts(2) out on the host: lines traced, distinct pairs; per pixel pdest (int32), pends (3
  ! each), plen, pstat (int32) and the first min(counts(2), max_pairs) pairs ppa, ppc (int32), pnl (int64), ppf out - on
  ! the HOST (B goes up into the staging array dF(1), the rest through one scratch buffer) or (on_device) in HBM.
  ! ------------------------------------------------------------------
  function vecpot_connect(ctx, pB, plabel, K, step, max_steps, max_pairs, counts, pdest, pends, plen, pstat, ppa, ppc, &
                          pnl, ppf, on_device) result(rc)
    type(vecpot_ctx), intent(inout), target :: ctx
    logical, intent(in) :: on_device
    type(c_ptr), intent(in) :: pB, plabel, pdest, pends, plen, pstat, ppa, ppc, pnl, ppf
    integer(c_int), intent(in) :: K, max_steps
    real(wp), intent(in) :: step
    integer(c_int64_t), intent(in) :: max_pairs
    integer(c_int64_t), intent(out) :: counts(2)
    integer(c_int) :: rc
    real(wp) :: dq(3), lo(3)
    integer(c_int32_t) :: n3(3)
    integer(c_size_t) :: np, nm
    type(c_ptr) :: buf
    type(slice) :: s(9)

    counts = 0
    call ctx_mesh(ctx, n3, lo, dq)
    if (on_device .or. K < 0 .or. max_pairs < 0 .or. .not. (step > 0.0_wp) .or. max_steps < 1) then
      ! (the argument errors are the kernel entry's to name; nothing is staged for them)
      rc = ndsmk_connect(pB, n3, lo, dq, ctx%qx, ctx%qy, plabel, K, step, max_steps, max_pairs, counts, pdest, pends, &
                         plen, pstat, ppa, ppc, pnl, ppf)
      if (rc == 0) rc = ndsmk_sync()
      return
    end if
    rc = stage_field(ctx, 1, pB); if (rc /= 0) return
    np = int(n3(1), c_size_t) * int(n3(2), c_size_t)
    nm = int(min(max_pairs, int(np, c_int64_t)), c_size_t)     ! (no more pairs than lines)
    s = [slice(plabel, 4, np, GOES_UP), slice(pdest, 4, np, COMES_HOME), slice(pends, 24, np, COMES_HOME), &
         slice(plen, 8, np, COMES_HOME), slice(pstat, 4, np, COMES_HOME), &
         slice(ppa, 4, nm, COMES_HOME), slice(ppc, 4, nm, COMES_HOME), slice(pnl, 8, nm, COMES_HOME), &
         slice(ppf, 8, nm, COMES_HOME)]
    rc = carve(buf, s)
    if (rc == 0) then
      call say("find_connectivity", "Tracing from the lower face and summing the pairs...")
      rc = ndsmk_connect(ctx%dF(1), n3, lo, dq, ctx%qx, ctx%qy, s(1)%dev, K, step, max_steps, max_pairs, counts, &
                         s(2)%dev, s(3)%dev, s(4)%dev, s(5)%dev, s(6)%dev, s(7)%dev, s(8)%dev, s(9)%dev)
    end if
    if (rc == 0) rc = fetch(s(1:5))
    if (rc == 0) rc = fetch(s(6:9), rows=int(min(counts(2), max_pairs), c_size_t))
    if (rc == 0) rc = ndsmk_sync()
    call unstage(rc, [buf])
    if (rc /= 0) counts = 0
  end function

  ! B.n of face f (1..6) from the host field (extract_bn, :699-743)
  subroutine face_gather(hB, n3, f, bn)
    real(wp), intent(inout) :: hB(:, :, :, :)
    integer(c_int32_t), intent(in) :: n3(3)
    integer, intent(in) :: f
    real(wp), intent(inout) :: bn(:, :)
    integer :: ax, lay
    ax = face_axis(f)
    lay = merge(int(n3(ax)), 1, face_upper(f))
    call face_copy(hB(:, :, :, ax), ax, lay, bn, to_face=.true.)
  end subroutine

  subroutine face_gather_flat(hB, n3, f, flat)
    real(wp), intent(inout) :: hB(:, :, :, :)
    integer(c_int32_t), intent(in) :: n3(3)
    integer, intent(in) :: f
    real(wp), intent(inout), target, contiguous :: flat(:)
    real(wp), pointer :: bn(:, :)
    bn(1:n3(face_t1(f)), 1:n3(face_t2(f))) => flat
    call face_gather(hB, n3, f, bn)
  end subroutine

  ! host face data (at1 / at2 of vecpot_faces) -> boundary plane f of the device array u: the
  ! NDSM_HIP_HOST_FACES path of vecpot_run (A/B testing of the device face phase)
  function face_upload(u3, n3, f, which, fd) result(rc)
    type(c_ptr), intent(in) :: u3
    integer(c_int32_t), intent(in) :: n3(3)
    integer, intent(in) :: f, which
    type(face_data), intent(in), target :: fd
    integer(c_int) :: rc
    type(c_ptr) :: tmp
    integer(c_size_t) :: nbf
    nbf = int(fd%n1, c_size_t) * int(fd%n2, c_size_t) * 8_c_size_t
    rc = ndsmk_alloc(tmp, nbf); if (rc /= 0) return
    if (which == 1) then
      rc = ndsmk_h2d(tmp, c_loc(fd%at1), nbf)
    else
      rc = ndsmk_h2d(tmp, c_loc(fd%at2), nbf)
    end if
    if (rc == 0) rc = ndsmk_face_put(u3, n3, int(f - 1, c_int), tmp)
    if (ndsmk_free(tmp) /= 0) continue
  end function

  ! central differences of chi, zero on the face's own edges (:1007-1017)
  subroutine tangential(fd, f, i, j, fac)
    type(face_data), intent(inout) :: fd
    integer, intent(in) :: f, i, j
    real(wp), intent(in) :: fac
    real(wp) :: d1, d2
    d1 = 0; d2 = 0
    if (i > 1 .and. i < fd%n1) d1 = fac * (fd%chi(i + 1, j) - fd%chi(i - 1, j))
    if (j > 1 .and. j < fd%n2) d2 = fac * (fd%chi(i, j + 1) - fd%chi(i, j - 1))
    fd%at1(i, j) = at_s1(f) * d2
    fd%at2(i, j) = at_s2(f) * d1
  end subroutine

  ! copy a face layer of a 3-D array to / from a 2-D array (extract_bn, :699-743)
  subroutine face_copy(v, axis, lay, face, to_face)
    real(wp), intent(inout) :: v(:, :, :)
    integer, intent(in) :: axis, lay
    real(wp), intent(inout) :: face(:, :)
    logical, intent(in) :: to_face
    select case (axis)
    case (1)
      if (to_face) then
        face = v(lay, :, :)
      else
        v(lay, :, :) = face
      end if
    case (2)
      if (to_face) then
        face = v(:, lay, :)
      else
        v(:, lay, :) = face
      end if
    case (3)
      if (to_face) then
        face = v(:, :, lay)
      else
        v(:, :, lay) = face
      end if
    end select
  end subroutine

  ! 2-D trapezoid rule, weights 1 / 1/2 (edges) / 1/4 (corners) (:1070-1106).  The reference sums
  ! serially; the device kernel (faces.hip: face_flux_k) sums as a fixed tree - 1024 strided partial sums,
  ! a halving tree over each group of 64, the 16 group sums in order.  This host version walks the SAME
  ! tree, so the host face phase (the distributed driver's rank 0, NDSM_HIP_HOST_FACES) and the device
  ! face phase produce the same bits.
  function trapezoid(f, h1, h2) result(s)
    real(wp), intent(in) :: f(:, :), h1, h2
    real(wp) :: s, w
    real(wp) :: part(0:1023)
    integer :: a, b, n1, n2, p, n, t, o, l, q
    logical :: ea, eb
    n1 = size(f, 1); n2 = size(f, 2)
    n = n1 * n2
    part = 0
    do t = 0, min(1023, n - 1)
      do p = t, n - 1, 1024
        a = mod(p, n1); b = p / n1
        ea = (a == 0 .or. a == n1 - 1); eb = (b == 0 .or. b == n2 - 1)
        w = 1.0_wp
        if (ea .or. eb) w = 0.5_wp
        if (ea .and. eb) w = 0.25_wp
        part(t) = part(t) + w * f(a + 1, b + 1)
      end do
    end do
    do q = 0, 15
      o = 32
      do while (o > 0)
        do l = 0, o - 1
          part(64 * q + l) = part(64 * q + l) + part(64 * q + l + o)
        end do
        o = o / 2
      end do
    end do
    s = 0
    do q = 0, 15
      s = s + part(64 * q)
    end do
    s = s * (h1 * h2)
  end function

end module ndsmh_vecpot
