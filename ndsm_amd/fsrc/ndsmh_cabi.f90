! libndsm_hip - the C ABI (declared in include/ndsm_hip.h).
!
! Part 1 is the reference's complete dynamic symbol set, same names, same
! argument lists, same option-slot values: ndsm_python_wrapper.f90:56-158
! (ndsm_vector_solve) and :164-234 (twelve getters) - an unmodified ndsm.py
! (ndsm.py:136-207) can load this library in place of ndsmf.so.
! Part 2 is additive: a scalar Poisson entry and a persistent, device-resident
! solver handle (SURVEY 8b "additive exports", 8f-4).  Nothing in part 1 changes
! meaning because of part 2.
!
! Error behaviour: the reference returns 0/1 and STOPs the process on internal
! asserts.  Here nothing STOPs: device/runtime failures come back as return
! codes >= 9001 (ndsm_kernels.h) with the text on stderr and in
! ndsm_hip_last_error().  There is no CPU fallback.
module ndsmh_cabi

  use, intrinsic :: iso_c_binding
  use, intrinsic :: iso_fortran_env, only: error_unit
  use ndsmh_iface
  use ndsmh_grid, only: slab_t
  use ndsmh_mg
  use ndsmh_world
  use ndsmh_vecpot
  use ndsmh_wvecpot
  implicit none
  private

  interface
    function ndsmk_dist_unique_id(out128) bind(c, name="ndsmk_dist_unique_id") result(rc)
      import :: c_ptr, c_int
      type(c_ptr), value :: out128
      integer(c_int) :: rc
    end function
    function ndsmk_dist_init(rank, nranks, id128) bind(c, name="ndsmk_dist_init") result(rc)
      import :: c_ptr, c_int
      integer(c_int), value :: rank, nranks
      type(c_ptr), value :: id128
      integer(c_int) :: rc
    end function
    function ndsmk_dist_finalize() bind(c, name="ndsmk_dist_finalize") result(rc)
      import :: c_int
      integer(c_int) :: rc
    end function
    function ndsmk_dist_info(rank, nranks) bind(c, name="ndsmk_dist_info") result(rc)
      import :: c_int
      integer(c_int), intent(out) :: rank, nranks
      integer(c_int) :: rc
    end function
    function ndsmk_dist_selftest(nelem) bind(c, name="ndsmk_dist_selftest") result(rc)
      import :: c_int
      integer(c_int), value :: nelem
      integer(c_int) :: rc
    end function
    function ndsmk_shutdown() bind(c, name="ndsmk_shutdown") result(rc)
      import :: c_int
      integer(c_int) :: rc
    end function
  end interface

  interface
    function c_strlen(s) bind(c, name="strlen") result(n)
      import :: c_ptr, c_size_t
      type(c_ptr), value :: s
      integer(c_size_t) :: n
    end function
  end interface

  interface
    function c_memset(p, c, n) bind(c, name="memset") result(q)
      import :: c_ptr, c_int, c_size_t
      type(c_ptr), value :: p
      integer(c_int), value :: c
      integer(c_size_t), value :: n
      type(c_ptr) :: q
    end function
  end interface

contains

  ! wall clock in seconds (the reference uses OMP_GET_WTIME, ndsm_root.f90:521-536)
  function wall_seconds() result(t)
    real(c_double) :: t
    integer(c_int64_t) :: cnt, rate
    call system_clock(cnt, rate)
    t = real(cnt, c_double) / real(rate, c_double)
  end function

  subroutine report(where, rc)
    character(len=*), intent(in) :: where
    integer(c_int), intent(in) :: rc
    character(len=512) :: msg
    call fetch_error(msg)
    write (error_unit, '(A,I0)') "ERROR("//where//"):"//trim(msg)//":", rc
  end subroutine

  subroutine fetch_error(msg)
    character(len=*), intent(out) :: msg
    type(c_ptr) :: p
    character(kind=c_char), pointer :: cs(:)
    integer :: i, n
    msg = ""
    p = ndsmk_last_error()
    if (.not. c_associated(p)) return
    n = min(int(c_strlen(p)), len(msg))
    call c_f_pointer(p, cs, [n])
    do i = 1, n
      msg(i:i) = cs(i)
    end do
  end subroutine

  ! =====================================================================
  ! Part 1 - the reference's symbols
  ! =====================================================================

  ! ndsm_python_wrapper.f90:56-79.  nshape4 = [nx,ny,nz,3]; A: in = initial
  ! guess, out = vector potential; B: in = field whose normal boundary
  ! component is read, out = curl A (+ flux balance).
  function ndsm_vector_solve(nsize, nshape4, ioptc, ropt, x, y, z, A, B) bind(c, name="ndsm_vector_solve") &
      result(ierr)
    integer(c_size_t), value :: nsize
    integer(c_int), intent(in) :: nshape4(4)
    integer(c_int), intent(inout) :: ioptc(0:OPT_LEN - 1)
    real(c_double), intent(inout) :: ropt(0:OPT_LEN - 1)
    real(c_double), intent(in) :: x(nshape4(1)), y(nshape4(2)), z(nshape4(3))
    real(c_double), intent(inout), target :: A(nsize), B(nsize)
    integer(c_int) :: ierr
    integer(ik) :: iopt(0:OPT_LEN - 1)
    integer(c_int32_t) :: n3(3)
    real(c_double) :: t0
    real(c_double), pointer, contiguous :: A4(:, :, :, :), B4(:, :, :, :)
    integer(c_int) :: rc

    iopt = ioptc
    verbose = (iopt(IOPT_DEBUG) == 1)
    t0 = wall_seconds()
    n3 = nshape4(1:3)
    if (nshape4(4) /= 3 .or. int(nsize, ik) /= 3_ik * product(int(n3, ik))) then
      ioptc(IOPT_IERR) = 1
      ierr = 1
      return
    end if
    A4(1:n3(1), 1:n3(2), 1:n3(3), 1:3) => A
    B4(1:n3(1), 1:n3(2), 1:n3(3), 1:3) => B

    rc = vecpot_solve(n3, iopt, ropt, x, y, z, A4, B4)

    ropt(ROPT_TIM) = wall_seconds() - t0
    ioptc = int(iopt, c_int)
    if (rc /= 0) then
      call report("ndsm_vector_solve", rc)
      ioptc(IOPT_IERR) = rc
      ierr = rc
    else
      ierr = int(iopt(IOPT_IERR), c_int)
    end if
  end function

  ! The same call on a z-slab decomposition (additive; BASELINE config[4]): one process per GPU,
  ! every rank of the communicator (ndsm_hip_dist_init) calls it with the GLOBAL nshape4 and mesh
  ! and with ITS planes [z0, z1) of A and B - the split ndsm_hip_slab_plan reports - laid out
  ! (nx, ny, z1-z0, 3).  Options, return value and the contents of A and B as for
  ! ndsm_vector_solve; nranks == 1 is ndsm_vector_solve.
  function ndsm_hip_world_vector_solve(rank, nranks, nshape4, ioptc, ropt, x, y, z, A, B) &
      bind(c, name="ndsm_hip_world_vector_solve") result(ierr)
    integer(c_int), value :: rank, nranks
    integer(c_int), intent(in) :: nshape4(4)
    integer(c_int), intent(inout) :: ioptc(0:OPT_LEN - 1)
    real(c_double), intent(inout) :: ropt(0:OPT_LEN - 1)
    real(c_double), intent(in) :: x(nshape4(1)), y(nshape4(2)), z(nshape4(3))
    type(c_ptr), value :: A, B
    integer(c_int) :: ierr
    integer(ik) :: iopt(0:OPT_LEN - 1)
    integer(c_int32_t) :: n3(3)
    real(c_double) :: t0
    real(c_double), pointer, contiguous :: A4(:, :, :, :), B4(:, :, :, :)
    type(slab_t), allocatable :: plan(:)
    integer(c_int) :: rc
    integer :: nzl

    iopt = ioptc
    verbose = (iopt(IOPT_DEBUG) == 1)
    t0 = wall_seconds()
    n3 = nshape4(1:3)
    ierr = NDSMK_EARG
    if (nshape4(4) /= 3 .or. nranks < 1 .or. rank < 0 .or. rank >= nranks) return
    if (.not. c_associated(A) .or. .not. c_associated(B)) return
    rc = ndsmk_init(-1_c_int)
    if (rc == 0) then
      if (nranks == 1) then
        call c_f_pointer(A, A4, [int(n3(1)), int(n3(2)), int(n3(3)), 3])
        call c_f_pointer(B, B4, [int(n3(1)), int(n3(2)), int(n3(3)), 3])
        rc = vecpot_solve(n3, iopt, ropt, x, y, z, A4, B4)
      else if (any(n3 < 2)) then
        iopt(IOPT_IERR) = 1
      else
        rc = world_plan_only(n3, x, y, z, int(iopt(IOPT_NGRIDS)), int(nranks), plan)
        if (rc == 0) then
          nzl = plan(rank)%z1 - plan(rank)%z0
          call c_f_pointer(A, A4, [int(n3(1)), int(n3(2)), nzl, 3])
          call c_f_pointer(B, B4, [int(n3(1)), int(n3(2)), nzl, 3])
          rc = wvecpot_solve(n3, iopt, ropt, x, y, z, int(nranks), int(rank), A4, B4)
        end if
      end if
    end if
    ropt(ROPT_TIM) = wall_seconds() - t0
    ioptc = int(iopt, c_int)
    if (rc /= 0) then
      call report("ndsm_hip_world_vector_solve", rc)
      ioptc(IOPT_IERR) = rc
      ierr = rc
    else
      ierr = int(iopt(IOPT_IERR), c_int)
    end if
  end function

  ! ndsm_python_wrapper.f90:164-234 - slot indices, discovered at run time by ndsm.py:155-174
  function get_iopt_len() bind(c, name="get_iopt_len") result(v)
    integer(c_int) :: v
    v = OPT_LEN
  end function
  function get_iopt_ierr() bind(c, name="get_iopt_ierr") result(v)
    integer(c_int) :: v
    v = OPT_LEN            ! sic: the reference returns IOPT_LEN here (:170-174, quirk Q5)
  end function
  function get_iopt_ms() bind(c, name="get_iopt_ms") result(v)
    integer(c_int) :: v
    v = IOPT_MS
  end function
  function get_iopt_ncycles() bind(c, name="get_iopt_ncycles") result(v)
    integer(c_int) :: v
    v = IOPT_NCYCLES
  end function
  function get_iopt_debug() bind(c, name="get_iopt_debug") result(v)
    integer(c_int) :: v
    v = IOPT_DEBUG
  end function
  function get_iopt_dumax() bind(c, name="get_iopt_dumax") result(v)
    integer(c_int) :: v
    v = IOPT_DUMAX
  end function
  function get_iopt_iopt_nmaxex() bind(c, name="get_iopt_iopt_nmaxex") result(v)
    integer(c_int) :: v
    v = IOPT_NMAXEX
  end function
  function get_iopt_true() bind(c, name="get_iopt_true") result(v)
    integer(c_int) :: v
    v = 1
  end function
  function get_iopt_false() bind(c, name="get_iopt_false") result(v)
    integer(c_int) :: v
    v = 0
  end function
  function get_ropt_tim() bind(c, name="get_ropt_tim") result(v)
    integer(c_int) :: v
    v = ROPT_TIM
  end function
  function get_ropt_vtol() bind(c, name="get_ropt_vtol") result(v)
    integer(c_int) :: v
    v = ROPT_VTOL
  end function
  function get_ropt_ctol() bind(c, name="get_ropt_ctol") result(v)
    integer(c_int) :: v
    v = ROPT_CTOL
  end function

  ! =====================================================================
  ! Part 2 - additive exports
  ! =====================================================================

  function get_iopt_fail3d() bind(c, name="get_iopt_fail3d") result(v)
    integer(c_int) :: v
    v = IOPT_FAIL3D
  end function
  function get_iopt_ngrids() bind(c, name="get_iopt_ngrids") result(v)
    integer(c_int) :: v
    v = IOPT_NGRIDS
  end function
  function get_iopt_prec() bind(c, name="get_iopt_prec") result(v)
    integer(c_int) :: v
    v = IOPT_PREC
  end function
  function get_iopt_ncyc_out() bind(c, name="get_iopt_ncyc_out") result(v)
    integer(c_int) :: v
    v = IOPT_NCYC_OUT
  end function
  function get_ropt_dulast() bind(c, name="get_ropt_dulast") result(v)
    integer(c_int) :: v
    v = ROPT_DULAST
  end function

  function ndsm_hip_device_count() bind(c, name="ndsm_hip_device_count") result(n)
    integer(c_int) :: n
    n = ndsmk_device_count()
  end function

  function ndsm_hip_init(device) bind(c, name="ndsm_hip_init") result(rc)
    integer(c_int), value :: device
    integer(c_int) :: rc
    rc = ndsmk_init(device)
  end function

  ! releases everything the library holds on the device outside the caller's handles (streams, events,
  ! metric scratch, the cached vector-potential hierarchy, a live RCCL communicator); destroy solver /
  ! world handles first.  ndsm_hip_init (or any solve) brings the runtime up again, on any device.
  function ndsm_hip_shutdown() bind(c, name="ndsm_hip_shutdown") result(rc)
    integer(c_int) :: rc
    rc = ndsmk_shutdown()
  end function

  subroutine ndsm_hip_last_error(buf, n) bind(c, name="ndsm_hip_last_error")
    integer(c_int), value :: n
    character(kind=c_char), intent(out) :: buf(n)
    character(len=512) :: msg
    integer :: i, m
    call fetch_error(msg)
    m = min(len_trim(msg), n - 1)
    do i = 1, m
      buf(i) = msg(i:i)
    end do
    buf(m + 1) = c_null_char
  end subroutine

  function ndsm_hip_sync() bind(c, name="ndsm_hip_sync") result(rc)
    integer(c_int) :: rc
    rc = ndsmk_sync()
  end function
  function ndsm_hip_timer_start() bind(c, name="ndsm_hip_timer_start") result(rc)
    integer(c_int) :: rc
    rc = ndsmk_timer_start()
  end function
  function ndsm_hip_timer_stop(ms) bind(c, name="ndsm_hip_timer_stop") result(rc)
    real(c_double), intent(out) :: ms
    integer(c_int) :: rc
    rc = ndsmk_timer_stop(ms)
  end function

  ! Scalar Poisson problem laplace(u) = rhs, host buffers.  bcs = 2*ndim
  ! letters (lower faces, then upper faces).  Options in the same slots as
  ! ndsm_vector_solve; rhs may be NULL (zero); hist may be NULL.
  function ndsm_hip_poisson_solve(ndim, nshape, x, y, z, bcs, ioptc, ropt, u, rhs, hist, hist_len) &
      bind(c, name="ndsm_hip_poisson_solve") result(ierr)
    integer(c_int), value :: ndim, hist_len
    integer(c_int), intent(in) :: nshape(ndim)
    type(c_ptr), value :: x, y, z, u, rhs, hist
    character(kind=c_char), intent(in) :: bcs(2 * ndim)
    integer(c_int), intent(inout) :: ioptc(0:OPT_LEN - 1)
    real(c_double), intent(inout) :: ropt(0:OPT_LEN - 1)
    integer(c_int) :: ierr
    integer(c_int32_t) :: n3(3)
    real(c_double), pointer :: qx(:), qy(:), qz(:), hh(:)
    real(c_double), target :: dummy(2)
    character(len=1) :: bc(6)
    real(c_double) :: du_last, t0
    integer :: ncyc, ie, d
    integer(c_int) :: rc

    ierr = NDSMK_EARG
    if (ndim /= 2 .and. ndim /= 3) return
    t0 = wall_seconds()
    n3 = 1
    n3(1:ndim) = nshape(1:ndim)
    dummy = [0.0_wp, 1.0_wp]
    call c_f_pointer(x, qx, [n3(1)])
    call c_f_pointer(y, qy, [n3(2)])
    if (ndim == 3) then
      call c_f_pointer(z, qz, [n3(3)])
    else
      qz => dummy
    end if
    bc = 'N'
    do d = 1, 2 * ndim
      bc(d) = bcs(d)
    end do
    verbose = (ioptc(IOPT_DEBUG) == 1)
    if (c_associated(hist) .and. hist_len > 0) then
      call c_f_pointer(hist, hh, [hist_len])
      rc = poisson_solve(int(ndim), n3, qx, qy, qz, bc, int(ioptc(IOPT_MS)), ropt(ROPT_CTOL), &
                         ioptc(IOPT_DUMAX) == 1, int(ioptc(IOPT_NMAXEX)), int(ioptc(IOPT_NGRIDS)), &
                         ropt(ROPT_VTOL), int(ioptc(IOPT_NCYCLES)), u, rhs, du_last, ncyc, ie, hh, &
                         precision=int(ioptc(IOPT_PREC)))
    else
      rc = poisson_solve(int(ndim), n3, qx, qy, qz, bc, int(ioptc(IOPT_MS)), ropt(ROPT_CTOL), &
                         ioptc(IOPT_DUMAX) == 1, int(ioptc(IOPT_NMAXEX)), int(ioptc(IOPT_NGRIDS)), &
                         ropt(ROPT_VTOL), int(ioptc(IOPT_NCYCLES)), u, rhs, du_last, ncyc, ie, &
                         precision=int(ioptc(IOPT_PREC)))
    end if
    ropt(ROPT_TIM) = wall_seconds() - t0
    if (rc /= 0) then
      call report("ndsm_hip_poisson_solve", rc)
      ierr = rc
      return
    end if
    ioptc(IOPT_IERR) = ie
    ioptc(IOPT_NCYC_OUT) = ncyc
    ropt(ROPT_DULAST) = du_last
    ierr = ie
  end function

  ! ---- persistent device-resident solver ------------------------------

  function ndsm_hip_mg_create(ndim, nshape, x, y, z, bcs, ngrids, ms, ex_tol, du_max, nmax_exact, handle) &
      bind(c, name="ndsm_hip_mg_create") result(rc)
    integer(c_int), value :: ndim, ngrids, ms, du_max, nmax_exact
    real(c_double), value :: ex_tol
    integer(c_int), intent(in) :: nshape(ndim)
    type(c_ptr), value :: x, y, z
    character(kind=c_char), intent(in) :: bcs(2 * ndim)
    type(c_ptr), intent(out) :: handle
    integer(c_int) :: rc
    type(mg_solver), pointer :: s
    integer(c_int32_t) :: n3(3)
    real(c_double), pointer :: qx(:), qy(:), qz(:)
    real(c_double), target :: dummy(2)
    character(len=1) :: bc(6)
    integer :: d

    handle = c_null_ptr
    rc = NDSMK_EARG
    if (ndim /= 2 .and. ndim /= 3) return
    if (ms < 0 .or. nmax_exact < 0) return       ! (sweep counts: 0 is the least; the pipeline entries clamp instead)
    n3 = 1
    n3(1:ndim) = nshape(1:ndim)
    dummy = [0.0_wp, 1.0_wp]
    call c_f_pointer(x, qx, [n3(1)])
    call c_f_pointer(y, qy, [n3(2)])
    if (ndim == 3) then
      call c_f_pointer(z, qz, [n3(3)])
    else
      qz => dummy
    end if
    bc = 'N'
    do d = 1, 2 * ndim
      bc(d) = bcs(d)
    end do
    allocate (s)
    rc = mg_create(s, int(ndim), n3, qx, qy, qz, bc, int(ngrids))
    if (rc /= 0) then
      call mg_destroy(s)
      deallocate (s)
      return
    end if
    s%ms = ms; s%ex_tol = ex_tol; s%use_max = (du_max == 1); s%nmax_exact = nmax_exact
    handle = c_loc(s)
  end function

  function ndsm_hip_mg_destroy(handle) bind(c, name="ndsm_hip_mg_destroy") result(rc)
    type(c_ptr), value :: handle
    integer(c_int) :: rc
    type(mg_solver), pointer :: s
    rc = 0
    if (.not. c_associated(handle)) return
    call c_f_pointer(handle, s)
    call mg_destroy(s)
    deallocate (s)
  end function

  ! shapes(3, ngrids) in Fortran order; pass ngrids_cap = room in `shapes`
  function ndsm_hip_mg_levels(handle, ngrids_cap, shapes) bind(c, name="ndsm_hip_mg_levels") result(ng)
    type(c_ptr), value :: handle
    integer(c_int), value :: ngrids_cap
    integer(c_int), intent(out) :: shapes(3, ngrids_cap)
    integer(c_int) :: ng
    type(mg_solver), pointer :: s
    integer :: l
    call c_f_pointer(handle, s)
    ng = s%ngrids
    do l = 1, min(s%ngrids, int(ngrids_cap))
      shapes(:, l) = s%lev(l)%n
    end do
  end function

  function ndsm_hip_mg_set_ms(handle, ms) bind(c, name="ndsm_hip_mg_set_ms") result(rc)
    type(c_ptr), value :: handle
    integer(c_int), value :: ms
    integer(c_int) :: rc
    type(mg_solver), pointer :: s
    rc = NDSMK_EARG
    if (ms < 0) return
    call c_f_pointer(handle, s)
    s%ms = ms
    rc = 0
  end function

  ! 0: fp64 (reference arithmetic); 1: mixed precision where level 1 is large enough; 2: mixed
  ! wherever the fp32 kernels cover level 1.  Returns 1 if ndsm_hip_mg_solve will run mixed, else 0.
  function ndsm_hip_mg_set_precision(handle, mode) bind(c, name="ndsm_hip_mg_set_precision") result(rc)
    type(c_ptr), value :: handle
    integer(c_int), value :: mode
    integer(c_int) :: rc
    type(mg_solver), pointer :: s
    call c_f_pointer(handle, s)
    rc = -1
    if (mode < 0 .or. mode > 2) return
    s%precision = mode
    rc = merge(1_c_int, 0_c_int, mg_mixed_applies(s))
  end function

  ! which: 0 = u, 1 = rhs, 2 = residual scratch (level-1 sized, valid after op RESIDUAL), 3 = the partner array of u
  function ndsm_hip_mg_upload(handle, level, which, host) bind(c, name="ndsm_hip_mg_upload") result(rc)
    type(c_ptr), value :: handle, host
    integer(c_int), value :: level, which
    integer(c_int) :: rc
    type(mg_solver), pointer :: s
    type(c_ptr) :: d
    integer(ik) :: n
    call c_f_pointer(handle, s)
    if (which == MG_BUF_U) then      ! (a zero guess that was declared only is written out before it is replaced)
      rc = mg_ensure_u(s, int(level)); if (rc /= 0) return
    end if
    d = mg_level_ptr(s, int(level), int(which), n)
    rc = NDSMK_EARG
    if (.not. c_associated(d)) return
    rc = ndsmk_h2d(d, host, int(n, c_size_t) * 8_c_size_t)
    if (level == 1 .and. which == MG_BUF_RHS) call mg_mark_rhs_set(s)
  end function

  ! declare the level-1 right-hand side identically zero (Laplace problem): the
  ! kernels then never read it; results are bit-identical
  function ndsm_hip_mg_zero_rhs(handle) bind(c, name="ndsm_hip_mg_zero_rhs") result(rc)
    type(c_ptr), value :: handle
    integer(c_int) :: rc
    type(mg_solver), pointer :: s
    call c_f_pointer(handle, s)
    rc = mg_zero_rhs(s)
  end function

  function ndsm_hip_mg_download(handle, level, which, host) bind(c, name="ndsm_hip_mg_download") result(rc)
    type(c_ptr), value :: handle, host
    integer(c_int), value :: level, which
    integer(c_int) :: rc
    type(mg_solver), pointer :: s
    type(c_ptr) :: d
    integer(ik) :: n
    call c_f_pointer(handle, s)
    if (which == MG_BUF_U) then      ! (a zero guess that was declared only reads as zeros)
      rc = mg_ensure_u(s, int(level)); if (rc /= 0) return
    end if
    d = mg_level_ptr(s, int(level), int(which), n)
    rc = NDSMK_EARG
    if (.not. c_associated(d)) return
    rc = ndsmk_d2h(host, d, int(n, c_size_t) * 8_c_size_t)
  end function

  ! op: 0 relax(count sweeps) 1 residual 2 restrict(level->level+1) 3 prolong-add
  ! (level+1->level) 4 coarsest solve 5 relax via colour kernels 6 relax via fused kernel
  function ndsm_hip_mg_op(handle, op, level, count) bind(c, name="ndsm_hip_mg_op") result(rc)
    type(c_ptr), value :: handle
    integer(c_int), value :: op, level, count
    integer(c_int) :: rc
    type(mg_solver), pointer :: s
    call c_f_pointer(handle, s)
    rc = mg_op(s, int(op), int(level), int(count))
  end function

  ! enqueue ncycles V-cycles; returns without waiting for the GPU
  function ndsm_hip_mg_vcycle(handle, ncycles) bind(c, name="ndsm_hip_mg_vcycle") result(rc)
    type(c_ptr), value :: handle
    integer(c_int), value :: ncycles
    integer(c_int) :: rc
    type(mg_solver), pointer :: s
    integer :: i
    call c_f_pointer(handle, s)
    rc = 0
    do i = 1, ncycles
      rc = mg_vcycle(s)
      if (rc /= 0) return
    end do
  end function

  ! V-cycles to vc_tol on the resident problem: 0 converged, 1 not, >= 9001 error
  function ndsm_hip_mg_solve(handle, vc_tol, nmax, du_last, ncycles, hist, hist_len) &
      bind(c, name="ndsm_hip_mg_solve") result(ierr)
    type(c_ptr), value :: handle, hist
    real(c_double), value :: vc_tol
    integer(c_int), value :: nmax, hist_len
    real(c_double), intent(out) :: du_last
    integer(c_int), intent(out) :: ncycles
    integer(c_int) :: ierr
    type(mg_solver), pointer :: s
    real(c_double), pointer :: hh(:)
    integer :: nc, ie
    integer(c_int) :: rc
    call c_f_pointer(handle, s)
    if (c_associated(hist) .and. hist_len > 0) then
      call c_f_pointer(hist, hh, [hist_len])
      rc = mg_solve(s, vc_tol, int(nmax), du_last, nc, ie, hh)
    else
      rc = mg_solve(s, vc_tol, int(nmax), du_last, nc, ie)
    end if
    ncycles = nc
    ierr = merge(rc, int(ie, c_int), rc /= 0)
  end function

  function ndsm_hip_mg_info(handle, sweeps, unconverged) bind(c, name="ndsm_hip_mg_info") result(rc)
    type(c_ptr), value :: handle
    integer(c_int64_t), intent(out) :: sweeps, unconverged
    integer(c_int) :: rc
    type(mg_solver), pointer :: s
    call c_f_pointer(handle, s)
    rc = mg_read_info(s, sweeps, unconverged)
  end function

  ! ---- device memory for callers without a HIP binding of their own (ctypes) ----
  function ndsm_hip_device_alloc(bytes, p) bind(c, name="ndsm_hip_device_alloc") result(rc)
    integer(c_size_t), value :: bytes
    type(c_ptr), intent(out) :: p
    integer(c_int) :: rc
    p = c_null_ptr
    rc = ndsmk_init(-1_c_int)
    if (rc == 0) rc = ndsmk_alloc(p, bytes)
  end function
  function ndsm_hip_device_free(p) bind(c, name="ndsm_hip_device_free") result(rc)
    type(c_ptr), value :: p
    integer(c_int) :: rc
    rc = ndsmk_free(p)
  end function
  function ndsm_hip_memcpy_h2d(d_dst, h_src, bytes) bind(c, name="ndsm_hip_memcpy_h2d") result(rc)
    type(c_ptr), value :: d_dst, h_src
    integer(c_size_t), value :: bytes
    integer(c_int) :: rc
    rc = ndsmk_h2d(d_dst, h_src, bytes)
  end function
  function ndsm_hip_memcpy_d2h(h_dst, d_src, bytes) bind(c, name="ndsm_hip_memcpy_d2h") result(rc)
    type(c_ptr), value :: h_dst, d_src
    integer(c_size_t), value :: bytes
    integer(c_int) :: rc
    rc = ndsmk_d2h(h_dst, d_src, bytes)
  end function

  ! ---- persistent vector-potential handle (SURVEY 8f-4) ------------------
  ! Everything that depends on the grid alone - the 3-D hierarchy and its transfer tables, the three
  ! 2-D face hierarchies, device arrays for A, B and the faces - lives in the handle; a solve moves
  ! boundary data in and results out.  (ndsm_vector_solve keeps one such context internally, keyed by
  ! shape and mesh.)
  function ndsm_hip_vecpot_create(nshape4, x, y, z, ngrids, handle) bind(c, name="ndsm_hip_vecpot_create") result(rc)
    integer(c_int), intent(in) :: nshape4(4)
    type(c_ptr), value :: x, y, z
    integer(c_int), value :: ngrids
    type(c_ptr), intent(out) :: handle
    integer(c_int) :: rc
    type(vecpot_ctx), pointer :: ctx
    real(c_double), pointer :: qx(:), qy(:), qz(:)
    integer(c_int32_t) :: n3(3)
    handle = c_null_ptr
    rc = NDSMK_EARG
    n3 = nshape4(1:3)
    if (nshape4(4) /= 3 .or. any(n3 < 3)) return
    if (.not. (c_associated(x) .and. c_associated(y) .and. c_associated(z))) return
    call c_f_pointer(x, qx, [n3(1)])
    call c_f_pointer(y, qy, [n3(2)])
    call c_f_pointer(z, qz, [n3(3)])
    allocate (ctx)
    rc = vecpot_ctx_create(ctx, n3, qx, qy, qz, int(ngrids))
    if (rc /= 0) then
      call report("ndsm_hip_vecpot_create", rc)
      call vecpot_ctx_destroy(ctx)
      deallocate (ctx)
      return
    end if
    handle = c_loc(ctx)
  end function

  function ndsm_hip_vecpot_destroy(handle) bind(c, name="ndsm_hip_vecpot_destroy") result(rc)
    type(c_ptr), value :: handle
    integer(c_int) :: rc
    type(vecpot_ctx), pointer :: ctx
    rc = 0
    if (.not. c_associated(handle)) return
    call c_f_pointer(handle, ctx)
    call vecpot_ctx_destroy(ctx)
    deallocate (ctx)
  end function

  ! A, B: HOST arrays (nx,ny,nz,3), contents and options exactly as for ndsm_vector_solve
  function ndsm_hip_vecpot_solve(handle, ioptc, ropt, A, B) bind(c, name="ndsm_hip_vecpot_solve") result(ierr)
    type(c_ptr), value :: handle, A, B
    integer(c_int), intent(inout) :: ioptc(0:OPT_LEN - 1)
    real(c_double), intent(inout) :: ropt(0:OPT_LEN - 1)
    integer(c_int) :: ierr
    ierr = vecpot_handle_solve(handle, ioptc, ropt, A, B, .false., "ndsm_hip_vecpot_solve")
  end function

  ! A, B: DEVICE arrays (nx,ny,nz,3) of the GPU the library runs on (e.g. torch tensors' data_ptr()):
  ! nothing but six fluxes and the per-cycle 16-byte convergence read-backs crosses PCIe.  The call
  ! returns when the results are complete in A and B (the library stream is drained).
  function ndsm_hip_vecpot_solve_device(handle, ioptc, ropt, dA, dB) bind(c, name="ndsm_hip_vecpot_solve_device") &
      result(ierr)
    type(c_ptr), value :: handle, dA, dB
    integer(c_int), intent(inout) :: ioptc(0:OPT_LEN - 1)
    real(c_double), intent(inout) :: ropt(0:OPT_LEN - 1)
    integer(c_int) :: ierr
    ierr = vecpot_handle_solve(handle, ioptc, ropt, dA, dB, .true., "ndsm_hip_vecpot_solve_device")
  end function

  function vecpot_handle_solve(handle, ioptc, ropt, A, B, on_device, who) result(ierr)
    type(c_ptr), intent(in) :: handle, A, B
    integer(c_int), intent(inout) :: ioptc(0:OPT_LEN - 1)
    real(c_double), intent(inout) :: ropt(0:OPT_LEN - 1)
    logical, intent(in) :: on_device
    character(len=*), intent(in) :: who
    integer(c_int) :: ierr
    type(vecpot_ctx), pointer :: ctx
    integer(ik) :: iopt(0:OPT_LEN - 1)
    real(c_double) :: t0
    integer(c_int) :: rc
    ierr = NDSMK_EARG
    if (.not. (c_associated(handle) .and. c_associated(A) .and. c_associated(B))) return
    call c_f_pointer(handle, ctx)
    if (.not. ctx%live) return
    iopt = ioptc
    verbose = (iopt(IOPT_DEBUG) == 1)
    t0 = wall_seconds()
    rc = NDSMK_EARG
    if (int(iopt(IOPT_NGRIDS)) == ctx%ngr) rc = vecpot_run(ctx, iopt, ropt, A, B, on_device)
    ropt(ROPT_TIM) = wall_seconds() - t0
    ioptc = int(iopt, c_int)
    if (rc /= 0) then
      call report(who, rc)
      ioptc(IOPT_IERR) = rc
      ierr = rc
    else
      ierr = int(iopt(IOPT_IERR), c_int)
    end if
  end function

  ! ---- the current-carrying field on the same handle -------------------
  ! A of a field B with curl B /= 0 (the 3-D problems get rhs_c = -(curl B)_c, same boundary letters and data
  ! as the potential field), and the relative helicity of B against the potential field of its B.n.  Return
  ! value of all four: 0 every 2-D and 3-D solve reached vc_tol, 1 at least one did not, >= 9001 errors (a
  ! HIP failure code, e.g. out of memory, comes back as 9001; the text names it).

  ! A: in initial guess, out A; B: in the whole field, out curl A + balance.  HOST arrays (nx,ny,nz,3)
  function ndsm_hip_vecpot_solve_field(handle, ioptc, ropt, A, B) bind(c, name="ndsm_hip_vecpot_solve_field") &
      result(ierr)
    type(c_ptr), value :: handle, A, B
    integer(c_int), intent(inout) :: ioptc(0:OPT_LEN - 1)
    real(c_double), intent(inout) :: ropt(0:OPT_LEN - 1)
    integer(c_int) :: ierr
    real(c_double) :: out8(8)
    ierr = vecpot_handle_field(handle, ioptc, ropt, A, B, c_null_ptr, c_null_ptr, out8, VP_FIELD, .false., &
                               "ndsm_hip_vecpot_solve_field")
  end function

  ! the same on DEVICE arrays of the library's GPU
  function ndsm_hip_vecpot_solve_field_device(handle, ioptc, ropt, dA, dB) &
      bind(c, name="ndsm_hip_vecpot_solve_field_device") result(ierr)
    type(c_ptr), value :: handle, dA, dB
    integer(c_int), intent(inout) :: ioptc(0:OPT_LEN - 1)
    real(c_double), intent(inout) :: ropt(0:OPT_LEN - 1)
    integer(c_int) :: ierr
    real(c_double) :: out8(8)
    ierr = vecpot_handle_field(handle, ioptc, ropt, dA, dB, c_null_ptr, c_null_ptr, out8, VP_FIELD, .true., &
                               "ndsm_hip_vecpot_solve_field_device")
  end function

  ! B: in (read only); A, Ap, Bp: out; out8: H_R, H_J, E, E_p, max|B_rec,c - B_c|, rms|B_rec - B|, max|div_h B|,
  ! max|div_h A|.  HOST arrays (nx,ny,nz,3)
  function ndsm_hip_vecpot_helicity(handle, ioptc, ropt, B, A, Ap, Bp, out8) bind(c, name="ndsm_hip_vecpot_helicity") &
      result(ierr)
    type(c_ptr), value :: handle, B, A, Ap, Bp
    integer(c_int), intent(inout) :: ioptc(0:OPT_LEN - 1)
    real(c_double), intent(inout) :: ropt(0:OPT_LEN - 1)
    real(c_double), intent(out) :: out8(8)
    integer(c_int) :: ierr
    ierr = vecpot_handle_field(handle, ioptc, ropt, A, B, Ap, Bp, out8, VP_HELICITY, .false., "ndsm_hip_vecpot_helicity")
  end function

  ! the same on DEVICE arrays of the library's GPU
  function ndsm_hip_vecpot_helicity_device(handle, ioptc, ropt, dB, dA, dAp, dBp, out8) &
      bind(c, name="ndsm_hip_vecpot_helicity_device") result(ierr)
    type(c_ptr), value :: handle, dB, dA, dAp, dBp
    integer(c_int), intent(inout) :: ioptc(0:OPT_LEN - 1)
    real(c_double), intent(inout) :: ropt(0:OPT_LEN - 1)
    real(c_double), intent(out) :: out8(8)
    integer(c_int) :: ierr
    ierr = vecpot_handle_field(handle, ioptc, ropt, dA, dB, dAp, dBp, out8, VP_HELICITY, .true., &
                               "ndsm_hip_vecpot_helicity_device")
  end function

  function vecpot_handle_field(handle, ioptc, ropt, A, B, Ap, Bp, out8, md, on_device, who) result(ierr)
    type(c_ptr), intent(in) :: handle, A, B, Ap, Bp
    integer(c_int), intent(inout) :: ioptc(0:OPT_LEN - 1)
    real(c_double), intent(inout) :: ropt(0:OPT_LEN - 1)
    real(c_double), intent(out) :: out8(8)
    integer, intent(in) :: md
    logical, intent(in) :: on_device
    character(len=*), intent(in) :: who
    integer(c_int) :: ierr
    type(vecpot_ctx), pointer :: ctx
    integer(ik) :: iopt(0:OPT_LEN - 1)
    real(c_double) :: t0
    integer(c_int) :: rc
    out8 = 0
    ierr = ndsmk_init(-1_c_int)                        ! without a device: 9001, whatever the arguments
    if (ierr /= 0) return
    ierr = NDSMK_EARG
    if (.not. (c_associated(handle) .and. c_associated(A) .and. c_associated(B))) return
    if (md == VP_HELICITY .and. .not. (c_associated(Ap) .and. c_associated(Bp))) return
    call c_f_pointer(handle, ctx)
    if (.not. ctx%live) return
    iopt = ioptc
    verbose = (iopt(IOPT_DEBUG) == 1)
    t0 = wall_seconds()
    rc = NDSMK_EARG
    if (int(iopt(IOPT_NGRIDS)) == ctx%ngr) rc = vecpot_run(ctx, iopt, ropt, A, B, on_device, md, Ap, Bp, out8)
    ropt(ROPT_TIM) = wall_seconds() - t0
    ioptc = int(iopt, c_int)
    if (rc /= 0) then
      call report(who, rc)
      if (rc < NDSMK_ENODEV) rc = NDSMK_ENODEV
      ioptc(IOPT_IERR) = rc
      ierr = rc
    else
      ierr = int(iopt(IOPT_IERR), c_int)
    end if
  end function

  ! ---- solenoidal projection on the same handle ------------------------
  ! B in: the field (nx,ny,nz,3); out: B - G_h phi, laplace_7(phi) = div_h B - c with all six faces Neumann
  ! (B.n on the six faces untouched).  phi (nx,ny,nz) out, may be null.  out4: c = sum w div_h B / sum w (left in
  ! div_h B'), max |div_h B| before, max |div_h B'| after, 1/2 sum w |G_h phi|^2.  Return value: 0 the solve
  ! reached vc_tol, 1 it did not, >= 9001 errors (9002: an ngrids slot other than the handle's).

  ! HOST arrays
  function ndsm_hip_vecpot_project(handle, ioptc, ropt, B, phi, out4) bind(c, name="ndsm_hip_vecpot_project") &
      result(ierr)
    type(c_ptr), value :: handle, B, phi
    integer(c_int), intent(inout) :: ioptc(0:OPT_LEN - 1)
    real(c_double), intent(inout) :: ropt(0:OPT_LEN - 1)
    real(c_double), intent(out) :: out4(4)
    integer(c_int) :: ierr
    ierr = vecpot_handle_project(handle, ioptc, ropt, B, phi, out4, .false., "ndsm_hip_vecpot_project")
  end function

  ! the same on DEVICE arrays of the library's GPU
  function ndsm_hip_vecpot_project_device(handle, ioptc, ropt, dB, dphi, out4) &
      bind(c, name="ndsm_hip_vecpot_project_device") result(ierr)
    type(c_ptr), value :: handle, dB, dphi
    integer(c_int), intent(inout) :: ioptc(0:OPT_LEN - 1)
    real(c_double), intent(inout) :: ropt(0:OPT_LEN - 1)
    real(c_double), intent(out) :: out4(4)
    integer(c_int) :: ierr
    ierr = vecpot_handle_project(handle, ioptc, ropt, dB, dphi, out4, .true., "ndsm_hip_vecpot_project_device")
  end function

  function vecpot_handle_project(handle, ioptc, ropt, B, phi, out4, on_device, who) result(ierr)
    type(c_ptr), intent(in) :: handle, B, phi
    integer(c_int), intent(inout) :: ioptc(0:OPT_LEN - 1)
    real(c_double), intent(inout) :: ropt(0:OPT_LEN - 1)
    real(c_double), intent(out) :: out4(4)
    logical, intent(in) :: on_device
    character(len=*), intent(in) :: who
    integer(c_int) :: ierr
    type(vecpot_ctx), pointer :: ctx
    integer(ik) :: iopt(0:OPT_LEN - 1)
    real(c_double) :: t0
    integer(c_int) :: rc
    out4 = 0
    ierr = ndsmk_init(-1_c_int)                        ! without a device: 9001, whatever the arguments
    if (ierr /= 0) return
    ierr = NDSMK_EARG
    if (.not. (c_associated(handle) .and. c_associated(B))) return
    call c_f_pointer(handle, ctx)
    if (.not. ctx%live) return
    iopt = ioptc
    verbose = (iopt(IOPT_DEBUG) == 1)
    t0 = wall_seconds()
    rc = NDSMK_EARG
    if (int(iopt(IOPT_NGRIDS)) == ctx%ngr) rc = vecpot_project(ctx, iopt, ropt, B, phi, on_device, out4)
    ropt(ROPT_TIM) = wall_seconds() - t0
    ioptc = int(iopt, c_int)
    if (rc /= 0) then
      call report(who, rc)
      if (rc < NDSMK_ENODEV) rc = NDSMK_ENODEV
      ioptc(IOPT_IERR) = rc
      ierr = rc
    else
      ierr = int(iopt(IOPT_IERR), c_int)
    end if
  end function

  ! ---- DeVore-gauge vector potentials on the same handle ----------------
  ! B, Bp in (nx,ny,nz,3): the field and any field whose B.n matches it (the library's potential field or the
  ! caller's own); A, Ap out: A_z = 0, A of B up from the base plane, A_p of Bp down from A's top plane.  out8: the
  ! layout of ndsm_hip_vecpot_helicity with B_rec = curl_h A (out8(8) = max |div_h A|, the gauge's divergence).
  ! No solve runs.  Return value: 0, or >= 9001 errors (9002 a NULL array); out8 is cleared on every failure.

  ! HOST arrays
  function ndsm_hip_vecpot_devore(handle, B, Bp, A, Ap, out8) bind(c, name="ndsm_hip_vecpot_devore") result(ierr)
    type(c_ptr), value :: handle, B, Bp, A, Ap
    real(c_double), intent(out) :: out8(8)
    integer(c_int) :: ierr
    ierr = vecpot_handle_devore(handle, B, Bp, A, Ap, out8, .false., "ndsm_hip_vecpot_devore")
  end function

  ! the same on DEVICE arrays of the library's GPU
  function ndsm_hip_vecpot_devore_device(handle, dB, dBp, dA, dAp, out8) bind(c, name="ndsm_hip_vecpot_devore_device") &
      result(ierr)
    type(c_ptr), value :: handle, dB, dBp, dA, dAp
    real(c_double), intent(out) :: out8(8)
    integer(c_int) :: ierr
    ierr = vecpot_handle_devore(handle, dB, dBp, dA, dAp, out8, .true., "ndsm_hip_vecpot_devore_device")
  end function

  function vecpot_handle_devore(handle, B, Bp, A, Ap, out8, on_device, who) result(ierr)
    type(c_ptr), intent(in) :: handle, B, Bp, A, Ap
    real(c_double), intent(out) :: out8(8)
    logical, intent(in) :: on_device
    character(len=*), intent(in) :: who
    integer(c_int) :: ierr
    type(vecpot_ctx), pointer :: ctx
    integer(c_int) :: rc
    out8 = 0
    ierr = ndsmk_init(-1_c_int)                        ! without a device: 9001, whatever the arguments
    if (ierr /= 0) return
    ierr = NDSMK_EARG
    if (.not. (c_associated(handle) .and. c_associated(B) .and. c_associated(Bp) .and. c_associated(A) .and. &
               c_associated(Ap))) return
    call c_f_pointer(handle, ctx)
    if (.not. ctx%live) return
    rc = vecpot_devore(ctx, B, Bp, A, Ap, on_device, out8)
    if (rc /= 0) then
      call report(who, rc)
      if (rc < NDSMK_ENODEV) rc = NDSMK_ENODEV
      out8 = 0
    end if
    ierr = rc
  end function

  ! ---- field lines and line integrals on the same handle -----------------
  ! B (nx,ny,nz,3), G the same or NULL (integrals 0), seeds (3,nseeds) in physical coordinates; step > 0 in units
  ! of min(h), max_steps >= 1, direction +1 / -1 / 0 (both: nl = 2 nseeds lines, the forward block first; else nl =
  ! nseeds).  Out: ends (3,nl), length, integral (nl), status, nsteps (nl, int32).  The handle supplies the mesh; no
  ! solve runs.  Return value: 0, or >= 9001 errors (9002 a NULL handle or required array, 9004 a scalar out of
  ! range).  The host entry clears its outputs on every failure (as far as nseeds and the pointers allow).

  ! HOST arrays
  function ndsm_hip_vecpot_trace(handle, B, G, nseeds, seeds, step, max_steps, direction, ends, length, integral, &
                                 status, nsteps) bind(c, name="ndsm_hip_vecpot_trace") result(ierr)
    type(c_ptr), value :: handle, B, G, seeds, ends, length, integral, status, nsteps
    integer(c_int), value :: nseeds, max_steps, direction
    real(c_double), value :: step
    integer(c_int) :: ierr
    ierr = vecpot_handle_lines(handle, .false., B, G, direction, nseeds, seeds, step, max_steps, c_null_ptr, ends, &
                               length, integral, status, nsteps, .false., "ndsm_hip_vecpot_trace")
  end function

  ! the same on DEVICE arrays of the library's GPU (nothing is cleared: the outputs are not host memory)
  function ndsm_hip_vecpot_trace_device(handle, dB, dG, nseeds, dseeds, step, max_steps, direction, dends, dlength, &
                                        dintegral, dstatus, dnsteps) bind(c, name="ndsm_hip_vecpot_trace_device") &
      result(ierr)
    type(c_ptr), value :: handle, dB, dG, dseeds, dends, dlength, dintegral, dstatus, dnsteps
    integer(c_int), value :: nseeds, max_steps, direction
    real(c_double), value :: step
    integer(c_int) :: ierr
    ierr = vecpot_handle_lines(handle, .false., dB, dG, direction, nseeds, dseeds, step, max_steps, c_null_ptr, dends, &
                               dlength, dintegral, dstatus, dnsteps, .true., "ndsm_hip_vecpot_trace_device")
  end function

  ! ---- squashing factor and twist on the same handle ----------------------
  ! As the trace entries, always both directions: B, G (NULL: integrals 0), integrand 0 (G.B/|B|) or 1 (G.B/|B|^2),
  ! seeds (3,nseeds); out q (nseeds), ends (3,2 nseeds), length, integral (2 nseeds), status, nsteps (2 nseeds,
  ! int32), the forward block first.  Return value: 0, or >= 9001 errors (9002 a NULL handle or required array, 9004
  ! a scalar out of range).  The host entry clears its outputs on every failure.

  ! HOST arrays
  function ndsm_hip_vecpot_squash(handle, B, G, integrand, nseeds, seeds, step, max_steps, q, ends, length, integral, &
                                  status, nsteps) bind(c, name="ndsm_hip_vecpot_squash") result(ierr)
    type(c_ptr), value :: handle, B, G, seeds, q, ends, length, integral, status, nsteps
    integer(c_int), value :: integrand, nseeds, max_steps
    real(c_double), value :: step
    integer(c_int) :: ierr
    ierr = vecpot_handle_lines(handle, .true., B, G, integrand, nseeds, seeds, step, max_steps, q, ends, length, &
                               integral, status, nsteps, .false., "ndsm_hip_vecpot_squash")
  end function

  ! the same on DEVICE arrays of the library's GPU (nothing is cleared: the outputs are not host memory)
  function ndsm_hip_vecpot_squash_device(handle, dB, dG, integrand, nseeds, dseeds, step, max_steps, dq, dends, &
                                         dlength, dintegral, dstatus, dnsteps) &
      bind(c, name="ndsm_hip_vecpot_squash_device") result(ierr)
    type(c_ptr), value :: handle, dB, dG, dseeds, dq, dends, dlength, dintegral, dstatus, dnsteps
    integer(c_int), value :: integrand, nseeds, max_steps
    real(c_double), value :: step
    integer(c_int) :: ierr
    ierr = vecpot_handle_lines(handle, .true., dB, dG, integrand, nseeds, dseeds, step, max_steps, dq, dends, dlength, &
                               dintegral, dstatus, dnsteps, .true., "ndsm_hip_vecpot_squash_device")
  end function

  ! ---- perpendicular squashing factor on the same handle -------------------
  ! As the squash entries, with qperp (nseeds) after q: Titov's Q-perp, from the same deviation vectors at the same two
  ! ends projected onto the planes perpendicular to B there (semantics: include/ndsm_hip.h).  q, ends, length, integral,
  ! status and nsteps hold the bits of the squash entry on the same arguments.  Return value and clearing as there
  ! (qperp: nseeds entries, required with nseeds > 0).

  ! HOST arrays
  function ndsm_hip_vecpot_squash_perp(handle, B, G, integrand, nseeds, seeds, step, max_steps, q, qperp, ends, length, &
                                       integral, status, nsteps) bind(c, name="ndsm_hip_vecpot_squash_perp") result(ierr)
    type(c_ptr), value :: handle, B, G, seeds, q, qperp, ends, length, integral, status, nsteps
    integer(c_int), value :: integrand, nseeds, max_steps
    real(c_double), value :: step
    integer(c_int) :: ierr
    ierr = vecpot_handle_lines(handle, .true., B, G, integrand, nseeds, seeds, step, max_steps, q, ends, length, &
                               integral, status, nsteps, .false., "ndsm_hip_vecpot_squash_perp", qperp)
  end function

  ! the same on DEVICE arrays of the library's GPU (nothing is cleared: the outputs are not host memory)
  function ndsm_hip_vecpot_squash_perp_device(handle, dB, dG, integrand, nseeds, dseeds, step, max_steps, dq, dqperp, &
                                              dends, dlength, dintegral, dstatus, dnsteps) &
      bind(c, name="ndsm_hip_vecpot_squash_perp_device") result(ierr)
    type(c_ptr), value :: handle, dB, dG, dseeds, dq, dqperp, dends, dlength, dintegral, dstatus, dnsteps
    integer(c_int), value :: integrand, nseeds, max_steps
    real(c_double), value :: step
    integer(c_int) :: ierr
    ierr = vecpot_handle_lines(handle, .true., dB, dG, integrand, nseeds, dseeds, step, max_steps, dq, dends, dlength, &
                               dintegral, dstatus, dnsteps, .true., "ndsm_hip_vecpot_squash_perp_device", dqperp)
  end function

  ! ---- nonlinear force-free field (Grad-Rubin) on the same handle ------------
  ! Semantics: include/ndsm_hip.h.  Return values of all six: 0, 1 (the solving entries: a 2-D or 3-D solve missed
  ! vc_tol), or >= 9001 errors (9001 without a GPU whatever the arguments, 9002 a NULL handle or required array, 9004
  ! a scalar out of range).  The host entries clear their outputs on every failure.

  ! alpha0 (nx,ny) carried along the lines of B (nx,ny,nz,3) to every node: alpha (nx,ny,nz), status (nx,ny,nz; int32,
  ! may be NULL).  HOST arrays
  function ndsm_hip_vecpot_alpha_map(handle, B, alpha0, polarity, step, max_steps, alpha, status) &
      bind(c, name="ndsm_hip_vecpot_alpha_map") result(ierr)
    type(c_ptr), value :: handle, B, alpha0, alpha, status
    integer(c_int), value :: polarity, max_steps
    real(c_double), value :: step
    integer(c_int) :: ierr
    ierr = vecpot_handle_alpha_map(handle, B, alpha0, polarity, step, max_steps, alpha, status, .false., &
                                   "ndsm_hip_vecpot_alpha_map")
  end function

  ! the same on DEVICE arrays of the library's GPU (nothing is cleared: the outputs are not host memory)
  function ndsm_hip_vecpot_alpha_map_device(handle, dB, dalpha0, polarity, step, max_steps, dalpha, dstatus) &
      bind(c, name="ndsm_hip_vecpot_alpha_map_device") result(ierr)
    type(c_ptr), value :: handle, dB, dalpha0, dalpha, dstatus
    integer(c_int), value :: polarity, max_steps
    real(c_double), value :: step
    integer(c_int) :: ierr
    ierr = vecpot_handle_alpha_map(handle, dB, dalpha0, polarity, step, max_steps, dalpha, dstatus, .true., &
                                   "ndsm_hip_vecpot_alpha_map_device")
  end function

  ! the grid of ctx can size a clearing: live_ctx has given a live context
  function usable(ctx) result(yes)
    type(vecpot_ctx), pointer, intent(in) :: ctx
    logical :: yes
    yes = associated(ctx)
    if (yes) yes = ctx%live
  end function

  function vecpot_handle_alpha_map(handle, B, alpha0, polarity, step, max_steps, alpha, status, on_device, who) &
      result(ierr)
    type(c_ptr), intent(in) :: handle, B, alpha0, alpha, status
    integer(c_int), intent(in) :: polarity, max_steps
    real(c_double), intent(in) :: step
    logical, intent(in) :: on_device
    character(len=*), intent(in) :: who
    integer(c_int) :: ierr
    type(vecpot_ctx), pointer :: ctx
    ierr = live_ctx(handle, ctx)
    if (ierr == 0 .and. .not. (c_associated(B) .and. c_associated(alpha0) .and. c_associated(alpha))) ierr = NDSMK_EARG
    if (ierr == 0) ierr = reported(who, vecpot_alpha_map(ctx, B, alpha0, polarity, step, max_steps, alpha, status, &
                                                         on_device))
    if (ierr /= 0 .and. .not. on_device .and. usable(ctx)) &
      call clear_host([alpha, status], [8, 4], spread(product(int(ctx%n3, c_int64_t)), 1, 2))
  end function

  ! A for a prescribed current J (nx,ny,nz,3): laplace(A_c) = -J_c with the potential field's gauge, boundary letters
  ! and tangential data.  A: in initial guess, out A; B: in the field whose B.n is kept, out curl A + balance.  HOST
  ! arrays; options and IOPT_FAIL3D as ndsm_hip_vecpot_solve_field
  function ndsm_hip_vecpot_solve_current(handle, ioptc, ropt, J, A, B) bind(c, name="ndsm_hip_vecpot_solve_current") &
      result(ierr)
    type(c_ptr), value :: handle, J, A, B
    integer(c_int), intent(inout) :: ioptc(0:OPT_LEN - 1)
    real(c_double), intent(inout) :: ropt(0:OPT_LEN - 1)
    integer(c_int) :: ierr
    ierr = vecpot_handle_current(handle, ioptc, ropt, J, A, B, .false., "ndsm_hip_vecpot_solve_current")
  end function

  ! the same on DEVICE arrays of the library's GPU
  function ndsm_hip_vecpot_solve_current_device(handle, ioptc, ropt, dJ, dA, dB) &
      bind(c, name="ndsm_hip_vecpot_solve_current_device") result(ierr)
    type(c_ptr), value :: handle, dJ, dA, dB
    integer(c_int), intent(inout) :: ioptc(0:OPT_LEN - 1)
    real(c_double), intent(inout) :: ropt(0:OPT_LEN - 1)
    integer(c_int) :: ierr
    ierr = vecpot_handle_current(handle, ioptc, ropt, dJ, dA, dB, .true., "ndsm_hip_vecpot_solve_current_device")
  end function

  function vecpot_handle_current(handle, ioptc, ropt, J, A, B, on_device, who) result(ierr)
    type(c_ptr), intent(in) :: handle, J, A, B
    integer(c_int), intent(inout) :: ioptc(0:OPT_LEN - 1)
    real(c_double), intent(inout) :: ropt(0:OPT_LEN - 1)
    logical, intent(in) :: on_device
    character(len=*), intent(in) :: who
    integer(c_int) :: ierr
    type(vecpot_ctx), pointer :: ctx
    integer(ik) :: iopt(0:OPT_LEN - 1)
    real(c_double) :: t0
    integer(c_int) :: rc
    ierr = live_ctx(handle, ctx)
    if (ierr == 0 .and. .not. (c_associated(J) .and. c_associated(A) .and. c_associated(B))) ierr = NDSMK_EARG
    if (ierr == 0) then
      iopt = ioptc
      verbose = (iopt(IOPT_DEBUG) == 1)
      t0 = wall_seconds()
      rc = NDSMK_EARG
      if (int(iopt(IOPT_NGRIDS)) == ctx%ngr) rc = vecpot_run(ctx, iopt, ropt, A, B, on_device, VP_CURRENT, pJ=J)
      ropt(ROPT_TIM) = wall_seconds() - t0
      ioptc = int(iopt, c_int)
      ierr = reported(who, rc)
      if (ierr /= 0) ioptc(IOPT_IERR) = ierr            ! (as the field entries: ioptc is written by a call that ran)
      if (ierr == 0) ierr = int(iopt(IOPT_IERR), c_int)
    end if
    if (ierr >= NDSMK_ENODEV) then
      if (.not. on_device .and. usable(ctx)) &
        call clear_host([A, B], [8, 8], spread(3_c_int64_t * product(int(ctx%n3, c_int64_t)), 1, 2))
    end if
  end function

  ! The Grad-Rubin iteration.  B (nx,ny,nz,3) in: supplies B.n on the six faces (start 1: B^0 as well); out: the last
  ! pass's field.  alpha0 (nx,ny) in.  A (nx,ny,nz,3): in A^0 with start 1, out the last pass's A.  alpha (nx,ny,nz),
  ! status (nx,ny,nz; int32, may be NULL), hist (4,niter_max; on the HOST in both entries) and niter_out (one int, on
  ! the HOST in both entries) out.  HOST arrays
  function ndsm_hip_vecpot_nlfff(handle, ioptc, ropt, B, alpha0, polarity, start, niter_max, tol, step, max_steps, A, &
                                 alpha, status, hist, niter_out) bind(c, name="ndsm_hip_vecpot_nlfff") result(ierr)
    type(c_ptr), value :: handle, B, alpha0, A, alpha, status, hist, niter_out
    integer(c_int), intent(inout) :: ioptc(0:OPT_LEN - 1)
    real(c_double), intent(inout) :: ropt(0:OPT_LEN - 1)
    integer(c_int), value :: polarity, start, niter_max, max_steps
    real(c_double), value :: tol, step
    integer(c_int) :: ierr
    ierr = vecpot_handle_nlfff(handle, ioptc, ropt, B, alpha0, polarity, start, niter_max, tol, step, max_steps, A, &
                               alpha, status, hist, niter_out, .false., "ndsm_hip_vecpot_nlfff")
  end function

  ! the same on DEVICE arrays of the library's GPU: nothing crosses PCIe between the passes but the convergence
  ! read-backs and the four numbers of a history row
  function ndsm_hip_vecpot_nlfff_device(handle, ioptc, ropt, dB, dalpha0, polarity, start, niter_max, tol, step, &
                                        max_steps, dA, dalpha, dstatus, hist, niter_out) &
      bind(c, name="ndsm_hip_vecpot_nlfff_device") result(ierr)
    type(c_ptr), value :: handle, dB, dalpha0, dA, dalpha, dstatus, hist, niter_out
    integer(c_int), intent(inout) :: ioptc(0:OPT_LEN - 1)
    real(c_double), intent(inout) :: ropt(0:OPT_LEN - 1)
    integer(c_int), value :: polarity, start, niter_max, max_steps
    real(c_double), value :: tol, step
    integer(c_int) :: ierr
    ierr = vecpot_handle_nlfff(handle, ioptc, ropt, dB, dalpha0, polarity, start, niter_max, tol, step, max_steps, dA, &
                               dalpha, dstatus, hist, niter_out, .true., "ndsm_hip_vecpot_nlfff_device")
  end function

  function vecpot_handle_nlfff(handle, ioptc, ropt, B, alpha0, polarity, start, niter_max, tol, step, max_steps, A, &
                               alpha, status, hist, niter_out, on_device, who) result(ierr)
    type(c_ptr), intent(in) :: handle, B, alpha0, A, alpha, status, hist, niter_out
    integer(c_int), intent(inout) :: ioptc(0:OPT_LEN - 1)
    real(c_double), intent(inout) :: ropt(0:OPT_LEN - 1)
    integer(c_int), intent(in) :: polarity, start, niter_max, max_steps
    real(c_double), intent(in) :: tol, step
    logical, intent(in) :: on_device
    character(len=*), intent(in) :: who
    integer(c_int) :: ierr
    type(vecpot_ctx), pointer :: ctx
    type(nlfff_args) :: nl
    integer(ik) :: iopt(0:OPT_LEN - 1)
    integer(c_int), pointer :: nout
    real(c_double) :: t0
    integer(c_int) :: rc
    if (c_associated(niter_out)) then
      call c_f_pointer(niter_out, nout)
      nout = 0
    end if
    ierr = live_ctx(handle, ctx)
    if (ierr == 0 .and. .not. (c_associated(B) .and. c_associated(alpha0) .and. c_associated(A) .and. &
                               c_associated(alpha) .and. c_associated(hist) .and. c_associated(niter_out))) &
      ierr = NDSMK_EARG
    if (ierr == 0 .and. ((polarity /= 1 .and. polarity /= -1) .or. start < 0 .or. start > 1 .or. niter_max < 1 .or. .not. (tol >= 0.0_c_double) &
                         .or. tol > huge(tol) .or. .not. (step > 0.0_c_double) .or. step > 1.0e300_c_double .or. &
                         max_steps < 1)) &
      ierr = ndsmk_note_error(NDSMK_EVALUE, "nlfff: polarity +1 or -1, start 0 or 1, niter_max >= 1, tol >= 0 (finite), "// &
                              "step > 0 (finite) and max_steps >= 1"//c_null_char)
    if (ierr == 0) then
      nl%alpha0 = alpha0; nl%alpha = alpha; nl%status = status; nl%hist = hist
      nl%polarity = polarity; nl%start = start; nl%niter_max = niter_max; nl%max_steps = max_steps
      nl%tol = tol; nl%step = step
      iopt = ioptc
      verbose = (iopt(IOPT_DEBUG) == 1)
      t0 = wall_seconds()
      rc = NDSMK_EARG
      if (int(iopt(IOPT_NGRIDS)) == ctx%ngr) rc = vecpot_nlfff(ctx, iopt, ropt, A, B, nl, on_device)
      ropt(ROPT_TIM) = wall_seconds() - t0
      ioptc = int(iopt, c_int)
      ierr = reported(who, rc)
      if (ierr /= 0) ioptc(IOPT_IERR) = ierr            ! (as the field entries: ioptc is written by a call that ran)
      if (ierr == 0) then
        nout = nl%niter
        ierr = int(iopt(IOPT_IERR), c_int)
      end if
    end if
    if (ierr >= NDSMK_ENODEV) then
      if (c_associated(hist) .and. niter_max >= 1) call clear_host([hist], [32], [int(niter_max, c_int64_t)])
      if (.not. on_device .and. usable(ctx)) &
        call clear_host([A, B, alpha, status], [24, 24, 8, 4], spread(product(int(ctx%n3, c_int64_t)), 1, 4))
    end if
  end function

  ! The optimization method (semantics in include/ndsm_hip.h).  B (nx,ny,nz,3) in: the magnetogram on k = 0 and B.n on
  ! the faces (start 0) or B^0 (start 1); out: the relaxed field, its six faces those of B^0.  w (nx,ny,nz) in, may be
  ! NULL.  hist (hist_rows,6) and info (3 ints) out, on the HOST in both entries.  HOST arrays
  function ndsm_hip_vecpot_optimize(handle, ioptc, ropt, B, w, start, niter_max, check, tol, dt0, dt_min, hist, &
                                    hist_rows, info) bind(c, name="ndsm_hip_vecpot_optimize") result(ierr)
    type(c_ptr), value :: handle, B, w, hist, info
    integer(c_int), intent(inout) :: ioptc(0:OPT_LEN - 1)
    real(c_double), intent(inout) :: ropt(0:OPT_LEN - 1)
    integer(c_int), value :: start, niter_max, check, hist_rows
    real(c_double), value :: tol, dt0, dt_min
    integer(c_int) :: ierr
    ierr = vecpot_handle_optimize(handle, ioptc, ropt, B, w, start, niter_max, check, tol, dt0, dt_min, hist, &
                                  hist_rows, info, .false., "ndsm_hip_vecpot_optimize")
  end function

  ! the same on DEVICE arrays of the library's GPU: only history rows cross PCIe
  function ndsm_hip_vecpot_optimize_device(handle, ioptc, ropt, dB, dw, start, niter_max, check, tol, dt0, dt_min, &
                                           hist, hist_rows, info) &
      bind(c, name="ndsm_hip_vecpot_optimize_device") result(ierr)
    type(c_ptr), value :: handle, dB, dw, hist, info
    integer(c_int), intent(inout) :: ioptc(0:OPT_LEN - 1)
    real(c_double), intent(inout) :: ropt(0:OPT_LEN - 1)
    integer(c_int), value :: start, niter_max, check, hist_rows
    real(c_double), value :: tol, dt0, dt_min
    integer(c_int) :: ierr
    ierr = vecpot_handle_optimize(handle, ioptc, ropt, dB, dw, start, niter_max, check, tol, dt0, dt_min, hist, &
                                  hist_rows, info, .true., "ndsm_hip_vecpot_optimize_device")
  end function

  ! the four entries above and below: with Bobs (and then wm, nu, free) the measurement term and the freed lower face
  function vecpot_handle_optimize(handle, ioptc, ropt, B, w, start, niter_max, check, tol, dt0, dt_min, hist, &
                                  hist_rows, info, on_device, who, Bobs, wm, nu, free) result(ierr)
    type(c_ptr), intent(in) :: handle, B, w, hist, info
    integer(c_int), intent(inout) :: ioptc(0:OPT_LEN - 1)
    real(c_double), intent(inout) :: ropt(0:OPT_LEN - 1)
    integer(c_int), intent(in) :: start, niter_max, check, hist_rows
    real(c_double), intent(in) :: tol, dt0, dt_min
    logical, intent(in) :: on_device
    character(len=*), intent(in) :: who
    type(c_ptr), intent(in), optional :: Bobs, wm
    real(c_double), intent(in), optional :: nu
    integer(c_int), intent(in), optional :: free
    integer(c_int) :: ierr
    type(vecpot_ctx), pointer :: ctx
    type(optimize_args) :: op
    integer(ik) :: iopt(0:OPT_LEN - 1)
    integer(c_int), pointer :: iout(:)
    real(c_double) :: t0
    integer(c_int) :: rc
    logical :: obs, ok
    obs = present(Bobs)
    if (c_associated(info)) then
      call c_f_pointer(info, iout, [3])
      iout = 0
    end if
    ierr = live_ctx(handle, ctx)
    if (ierr == 0 .and. .not. (c_associated(B) .and. c_associated(hist) .and. c_associated(info))) ierr = NDSMK_EARG
    if (ierr == 0 .and. obs) then
      if (.not. c_associated(Bobs)) ierr = NDSMK_EARG
    end if
    if (ierr == 0) then
      ok = .not. (start < 0 .or. start > 1 .or. niter_max < 1 .or. check < 1 .or. hist_rows < 2 .or. &
                  .not. (tol >= 0.0_c_double) .or. tol > huge(tol) .or. .not. (dt0 > 0.0_c_double) .or. &
                  dt0 > huge(dt0) .or. .not. (dt_min >= 0.0_c_double) .or. dt_min > huge(dt_min))
      if (obs) then
        if (.not. ok .or. free < 0 .or. free > 1 .or. .not. (nu >= 0.0_c_double) .or. nu > huge(nu)) &
          ierr = ndsmk_note_error(NDSMK_EVALUE, "optimize_obs: free 0 or 1, nu >= 0, start 0 or 1, niter_max >= 1, "// &
                                  "check >= 1, hist_rows >= 2, tol >= 0, dt0 > 0 and dt_min >= 0 (all finite)"//c_null_char)
      else if (.not. ok) then
        ierr = ndsmk_note_error(NDSMK_EVALUE, "optimize: start 0 or 1, niter_max >= 1, check >= 1, hist_rows >= 2, "// &
                                "tol >= 0, dt0 > 0 and dt_min >= 0 (all finite)"//c_null_char)
      end if
    end if
    if (ierr == 0) then
      op%w = w; op%hist = hist
      if (obs) then
        op%bobs = Bobs; op%wm = wm; op%nu = nu; op%free = free
      end if
      op%start = start; op%niter_max = niter_max; op%check = check; op%hist_rows = hist_rows
      op%tol = tol; op%dt0 = dt0; op%dt_min = dt_min
      iopt = ioptc
      verbose = (iopt(IOPT_DEBUG) == 1)
      t0 = wall_seconds()
      rc = NDSMK_EARG
      if (int(iopt(IOPT_NGRIDS)) == ctx%ngr) then
        if (obs) then
          rc = vecpot_optimize_obs(ctx, iopt, ropt, B, op, on_device)
        else
          rc = vecpot_optimize(ctx, iopt, ropt, B, op, on_device)
        end if
      end if
      ropt(ROPT_TIM) = wall_seconds() - t0
      ioptc = int(iopt, c_int)
      ierr = reported(who, rc)
      if (ierr /= 0) ioptc(IOPT_IERR) = ierr            ! (as the field entries: ioptc is written by a call that ran)
      if (ierr == 0) then
        iout = op%info
        ierr = int(iopt(IOPT_IERR), c_int)
      end if
    end if
    if (ierr >= NDSMK_ENODEV) then
      if (c_associated(info)) iout = 0
      if (c_associated(hist) .and. hist_rows >= 1) &
        call clear_host([hist], [merge(56, 48, obs)], [int(hist_rows, c_int64_t)])
    end if
  end function

  ! The optimization method with a measurement term and a freed lower face (semantics in include/ndsm_hip.h).  B, w,
  ! start, niter_max .. info as ndsm_hip_vecpot_optimize; Bobs (nx,ny,3) in: the observation the k = 0 plane is fitted
  ! to; wm (nx,ny,3) in, may be NULL: its per-component confidence; nu >= 0; free 0 or 1.  hist (hist_rows,7).  HOST arrays
  function ndsm_hip_vecpot_optimize_obs(handle, ioptc, ropt, B, w, Bobs, wm, nu, free, start, niter_max, check, tol, &
                                        dt0, dt_min, hist, hist_rows, info) &
      bind(c, name="ndsm_hip_vecpot_optimize_obs") result(ierr)
    type(c_ptr), value :: handle, B, w, Bobs, wm, hist, info
    integer(c_int), intent(inout) :: ioptc(0:OPT_LEN - 1)
    real(c_double), intent(inout) :: ropt(0:OPT_LEN - 1)
    integer(c_int), value :: free, start, niter_max, check, hist_rows
    real(c_double), value :: nu, tol, dt0, dt_min
    integer(c_int) :: ierr
    ierr = vecpot_handle_optimize(handle, ioptc, ropt, B, w, start, niter_max, check, tol, dt0, dt_min, hist, &
                                  hist_rows, info, .false., "ndsm_hip_vecpot_optimize_obs", Bobs, wm, nu, free)
  end function

  ! the same on DEVICE arrays of the library's GPU: only history rows cross PCIe
  function ndsm_hip_vecpot_optimize_obs_device(handle, ioptc, ropt, dB, dw, dBobs, dwm, nu, free, start, niter_max, &
                                               check, tol, dt0, dt_min, hist, hist_rows, info) &
      bind(c, name="ndsm_hip_vecpot_optimize_obs_device") result(ierr)
    type(c_ptr), value :: handle, dB, dw, dBobs, dwm, hist, info
    integer(c_int), intent(inout) :: ioptc(0:OPT_LEN - 1)
    real(c_double), intent(inout) :: ropt(0:OPT_LEN - 1)
    integer(c_int), value :: free, start, niter_max, check, hist_rows
    real(c_double), value :: nu, tol, dt0, dt_min
    integer(c_int) :: ierr
    ierr = vecpot_handle_optimize(handle, ioptc, ropt, dB, dw, start, niter_max, check, tol, dt0, dt_min, hist, &
                                  hist_rows, info, .true., "ndsm_hip_vecpot_optimize_obs_device", dBobs, dwm, nu, free)
  end function

  ! Resampling of a node array between two uniform meshes on the same box (semantics in include/ndsm_hip.h).  src
  ! (nsrc,ncomp) in, dst (ndst,ncomp) out; mode 0 linear interpolation, 1 hat average.  No handle.  HOST arrays
  function ndsm_hip_resample(nsrc, ndst, ncomp, mode, src, dst) bind(c, name="ndsm_hip_resample") result(ierr)
    type(c_ptr), value :: nsrc, ndst, src, dst
    integer(c_int), value :: ncomp, mode
    integer(c_int) :: ierr
    ierr = resample_entry(nsrc, ndst, ncomp, mode, src, dst, .false., "ndsm_hip_resample")
  end function

  ! the same on DEVICE arrays of the library's GPU (they must not overlap)
  function ndsm_hip_resample_device(nsrc, ndst, ncomp, mode, dsrc, ddst) bind(c, name="ndsm_hip_resample_device") &
      result(ierr)
    type(c_ptr), value :: nsrc, ndst, dsrc, ddst
    integer(c_int), value :: ncomp, mode
    integer(c_int) :: ierr
    ierr = resample_entry(nsrc, ndst, ncomp, mode, dsrc, ddst, .true., "ndsm_hip_resample_device")
  end function

  function resample_entry(nsrc, ndst, ncomp, mode, src, dst, on_device, who) result(ierr)
    type(c_ptr), intent(in) :: nsrc, ndst, src, dst
    integer(c_int), intent(in) :: ncomp, mode
    logical, intent(in) :: on_device
    character(len=*), intent(in) :: who
    integer(c_int) :: ierr
    integer(c_int), pointer :: ns(:), nd(:)
    integer(c_int32_t) :: ns3(3), nd3(3)
    integer(c_size_t) :: bs, bd
    type(c_ptr) :: buf, ddst
    integer(c_int) :: rc
    integer :: d
    logical :: ok
    ierr = ndsmk_init(-1_c_int)
    if (ierr /= 0) return
    ierr = NDSMK_EARG
    if (.not. (c_associated(nsrc) .and. c_associated(ndst) .and. c_associated(src) .and. c_associated(dst))) return
    call c_f_pointer(nsrc, ns, [3])
    call c_f_pointer(ndst, nd, [3])
    ok = ncomp >= 1 .and. (mode == 0 .or. mode == 1)
    do d = 1, 3
      ok = ok .and. ((ns(d) == 1 .and. nd(d) == 1) .or. (ns(d) >= 2 .and. nd(d) >= 2))
      ok = ok .and. .not. (mode == 1 .and. nd(d) > ns(d))
    end do
    if (.not. ok) then
      ierr = ndsmk_note_error(NDSMK_EVALUE, "resample: ncomp >= 1, mode 0 or 1, at least 2 nodes per axis on both "// &
                              "sides (or 1 on both), and no axis finer than its source in mode 1"//c_null_char)
      return
    end if
    ns3 = ns; nd3 = nd
    if (on_device) then
      rc = ndsmk_resample(ns3, nd3, ncomp, mode, src, dst)
      if (rc == 0) rc = ndsmk_sync()
    else
      bs = int(product(int(ns3, c_int64_t)) * int(ncomp, c_int64_t) * 8_c_int64_t, c_size_t)
      bd = int(product(int(nd3, c_int64_t)) * int(ncomp, c_int64_t) * 8_c_int64_t, c_size_t)
      buf = c_null_ptr
      rc = ndsmk_alloc(buf, bs + bd)
      if (rc == 0) then
        ddst = dptr_offset(buf, bs)
        rc = ndsmk_h2d(buf, src, bs)
        if (rc == 0) rc = ndsmk_resample(ns3, nd3, ncomp, mode, buf, ddst)
        if (rc == 0) rc = ndsmk_d2h(dst, ddst, bd)
        if (rc == 0) rc = ndsmk_sync()
        d = ndsmk_free(buf)
        if (rc == 0) rc = int(d, c_int)
      end if
    end if
    ierr = reported(who, rc)
  end function

  ! ---- Green's-function field of the half space above a magnetogram (semantics in include/ndsm_hip.h) ----
  ! bz (nsx,nsy) on the mesh xs, ys at height zs; pts (3,npts) in, B (3,npts) out.  No handle.  The mesh vectors stay
  ! on the host in both forms.  HOST arrays
  function ndsm_hip_green_points(nsrc, xs, ys, zs, bz, npts, pts, B) bind(c, name="ndsm_hip_green_points") result(ierr)
    type(c_ptr), value :: nsrc, xs, ys, bz, pts, B
    real(c_double), value :: zs
    integer(c_int), value :: npts
    integer(c_int) :: ierr
    ierr = green_entry(.false., nsrc, xs, ys, zs, bz, npts, pts, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, &
                       0_c_int, B, .false., "ndsm_hip_green_points", .false., 0.0_c_double)
  end function

  ! the same with bz, pts and B DEVICE arrays of the library's GPU
  function ndsm_hip_green_points_device(nsrc, xs, ys, zs, dbz, npts, dpts, dB) &
      bind(c, name="ndsm_hip_green_points_device") result(ierr)
    type(c_ptr), value :: nsrc, xs, ys, dbz, dpts, dB
    real(c_double), value :: zs
    integer(c_int), value :: npts
    integer(c_int) :: ierr
    ierr = green_entry(.false., nsrc, xs, ys, zs, dbz, npts, dpts, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, &
                       0_c_int, dB, .true., "ndsm_hip_green_points_device", .false., 0.0_c_double)
  end function

  ! B (nx,ny,nz,3) on the box mesh x, y, z: which = 0 the nodes with an index at either end of an axis (every other
  ! node of B keeps what it holds), 1 all nodes.  HOST arrays
  function ndsm_hip_green_box(nsrc, xs, ys, zs, bz, nshape, x, y, z, which, B) bind(c, name="ndsm_hip_green_box") &
      result(ierr)
    type(c_ptr), value :: nsrc, xs, ys, bz, nshape, x, y, z, B
    real(c_double), value :: zs
    integer(c_int), value :: which
    integer(c_int) :: ierr
    ierr = green_entry(.true., nsrc, xs, ys, zs, bz, 0_c_int, c_null_ptr, nshape, x, y, z, which, B, .false., &
                       "ndsm_hip_green_box", .false., 0.0_c_double)
  end function

  ! the same with bz and B DEVICE arrays of the library's GPU
  function ndsm_hip_green_box_device(nsrc, xs, ys, zs, dbz, nshape, x, y, z, which, dB) &
      bind(c, name="ndsm_hip_green_box_device") result(ierr)
    type(c_ptr), value :: nsrc, xs, ys, dbz, nshape, x, y, z, dB
    real(c_double), value :: zs
    integer(c_int), value :: which
    integer(c_int) :: ierr
    ierr = green_entry(.true., nsrc, xs, ys, zs, dbz, 0_c_int, c_null_ptr, nshape, x, y, z, which, dB, .true., &
                       "ndsm_hip_green_box_device", .false., 0.0_c_double)
  end function

  ! the source of a Green's-function call: 0, or 9004 unless there are 2 nodes per axis and both spacings are > 0
  function green_source_ok(ns, xs, ys) result(ierr)
    integer(c_int), intent(in) :: ns(2)
    type(c_ptr), intent(in) :: xs, ys
    integer(c_int) :: ierr
    real(c_double), pointer :: qx(:), qy(:)
    ierr = NDSMK_EVALUE
    if (any(ns < 2)) return
    call c_f_pointer(xs, qx, [2])
    call c_f_pointer(ys, qy, [2])
    if (qx(2) - qx(1) > 0.0_c_double .and. qy(2) - qy(1) > 0.0_c_double) ierr = 0
  end function

  ! lfff: the constant-alpha field with that alpha (a non-finite alpha is 9004); otherwise alpha is not looked at
  function green_entry(box, nsrc, xs, ys, zs, bz, npts, pts, nshape, x, y, z, which, B, on_device, who, lfff, alpha) &
      result(ierr)
    logical, intent(in) :: box, on_device, lfff
    type(c_ptr), intent(in) :: nsrc, xs, ys, bz, pts, nshape, x, y, z, B
    real(c_double), intent(in) :: zs, alpha
    integer(c_int), intent(in) :: npts, which
    character(len=*), intent(in) :: who
    integer(c_int) :: ierr
    integer(c_int), pointer :: ns(:), nb(:)
    real(c_double), pointer :: qz(:)
    integer(c_int32_t) :: ns2(2)
    integer(c_int32_t), target :: n3(3)
    integer(c_size_t) :: bsrc, bout
    real(c_double) :: dsrc, dout
    type(c_ptr) :: buf, dpts, pout, p3
    integer(c_int) :: rc
    integer :: d
    ierr = ndsmk_init(-1_c_int)
    if (ierr /= 0) return
    ! a call the device cannot hold is refused before anything is allocated - as soon as its shapes can be read
    if (c_associated(nsrc) .and. (c_associated(nshape) .or. .not. box)) then
      call c_f_pointer(nsrc, ns, [2])
      ns2 = ns; n3 = 1; p3 = c_null_ptr
      if (box) then
        call c_f_pointer(nshape, nb, [3])
        n3 = nb; p3 = c_loc(n3)
      end if
      if (all(ns2 >= 1) .and. all(n3 >= 1) .and. npts >= 0) then
        ! (in doubles: three axes of up to 2^31 nodes overflow 64-bit whole numbers; past the screen they do not)
        dsrc = 8.0_c_double * product(real(ns2, c_double))
        dout = 24.0_c_double * merge(product(real(n3, c_double)), real(npts, c_double), box)
        ierr = ndsmk_green_fits(ns2, p3, merge(0_c_int, 1_c_int, which == 0), int(npts, c_long_long), &
                                merge(0.0_c_double, dsrc + dout * merge(1.0_c_double, 2.0_c_double, box), on_device))
        if (ierr /= 0) return
        bsrc = int(dsrc, c_size_t)
        bout = int(dout, c_size_t)
      end if
    end if
    ierr = NDSMK_EARG
    if (.not. (c_associated(nsrc) .and. c_associated(xs) .and. c_associated(ys) .and. c_associated(bz))) return
    if (box .and. .not. (c_associated(nshape) .and. c_associated(x) .and. c_associated(y) .and. c_associated(z) .and. &
                         c_associated(B))) return
    ierr = green_source_ok(ns, xs, ys)
    if (ierr == 0 .and. box) then
      call c_f_pointer(z, qz, [1])
      if (any(n3 < 2) .or. (which /= 0 .and. which /= 1) .or. .not. (qz(1) >= zs)) ierr = NDSMK_EVALUE
    end if
    if (ierr == 0 .and. npts < 0) ierr = NDSMK_EVALUE
    if (ierr == 0 .and. lfff .and. .not. (abs(alpha) <= huge(alpha))) ierr = NDSMK_EVALUE      ! (a NaN fails it too)
    if (ierr /= 0) then
      ierr = ndsmk_note_error(NDSMK_EVALUE, "green: at least 2 source nodes per axis, spacings > 0, npts >= 0, which "// &
                              "0 or 1, at least 2 box nodes per axis, z[0] >= zs and (lfff) a finite alpha"//c_null_char)
      return
    end if
    if (.not. box) then
      if (npts == 0) return
      ierr = NDSMK_EARG
      if (.not. (c_associated(pts) .and. c_associated(B))) return
    end if
    if (on_device) then
      rc = launch(bz, pts, B)
    else
      ! bz, then (points) pts, then B; which = 0 leaves nodes of B untouched, so B goes up first
      buf = c_null_ptr
      rc = ndsmk_alloc(buf, bsrc + bout * merge(1_c_size_t, 2_c_size_t, box))
      if (rc == 0) then
        dpts = dptr_offset(buf, bsrc)
        pout = dptr_offset(buf, bsrc + merge(0_c_size_t, bout, box))
        rc = ndsmk_h2d(buf, bz, bsrc)
        if (box) then
          if (rc == 0 .and. which == 0) rc = ndsmk_h2d(pout, B, bout)
        else
          if (rc == 0) rc = ndsmk_h2d(dpts, pts, bout)
        end if
        if (rc == 0) rc = launch(buf, dpts, pout)
        if (rc == 0) rc = ndsmk_d2h(B, pout, bout)
        d = ndsmk_free(buf)
        if (rc == 0) rc = int(d, c_int)
      end if
    end if
    ierr = reported(who, rc)
  contains
    ! the launcher of this entry on the device arrays dbz, dp (points only) and dout
    function launch(dbz, dp, dout) result(lrc)
      type(c_ptr), intent(in) :: dbz, dp, dout
      integer(c_int) :: lrc
      if (box .and. lfff) then
        lrc = ndsmk_lfff_box(ns2, xs, ys, zs, dbz, alpha, n3, x, y, z, which, dout)
      else if (box) then
        lrc = ndsmk_green_box(ns2, xs, ys, zs, dbz, n3, x, y, z, which, dout)
      else if (lfff) then
        lrc = ndsmk_lfff_points(ns2, xs, ys, zs, dbz, alpha, npts, dp, dout)
      else
        lrc = ndsmk_green_points(ns2, xs, ys, zs, dbz, npts, dp, dout)
      end if
    end function
  end function

  ! ---- Constant-alpha (linear force-free) field of a magnetogram (semantics in include/ndsm_hip.h) ----
  ! the arguments of the Green's-function entries and alpha, through the same path.  HOST arrays
  function ndsm_hip_lfff_points(nsrc, xs, ys, zs, bz, alpha, npts, pts, B) bind(c, name="ndsm_hip_lfff_points") &
      result(ierr)
    type(c_ptr), value :: nsrc, xs, ys, bz, pts, B
    real(c_double), value :: zs, alpha
    integer(c_int), value :: npts
    integer(c_int) :: ierr
    ierr = green_entry(.false., nsrc, xs, ys, zs, bz, npts, pts, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, &
                       0_c_int, B, .false., "ndsm_hip_lfff_points", .true., alpha)
  end function

  ! the same with bz, pts and B DEVICE arrays of the library's GPU
  function ndsm_hip_lfff_points_device(nsrc, xs, ys, zs, dbz, alpha, npts, dpts, dB) &
      bind(c, name="ndsm_hip_lfff_points_device") result(ierr)
    type(c_ptr), value :: nsrc, xs, ys, dbz, dpts, dB
    real(c_double), value :: zs, alpha
    integer(c_int), value :: npts
    integer(c_int) :: ierr
    ierr = green_entry(.false., nsrc, xs, ys, zs, dbz, npts, dpts, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, &
                       0_c_int, dB, .true., "ndsm_hip_lfff_points_device", .true., alpha)
  end function

  ! HOST arrays
  function ndsm_hip_lfff_box(nsrc, xs, ys, zs, bz, alpha, nshape, x, y, z, which, B) &
      bind(c, name="ndsm_hip_lfff_box") result(ierr)
    type(c_ptr), value :: nsrc, xs, ys, bz, nshape, x, y, z, B
    real(c_double), value :: zs, alpha
    integer(c_int), value :: which
    integer(c_int) :: ierr
    ierr = green_entry(.true., nsrc, xs, ys, zs, bz, 0_c_int, c_null_ptr, nshape, x, y, z, which, B, .false., &
                       "ndsm_hip_lfff_box", .true., alpha)
  end function

  ! the same with bz and B DEVICE arrays of the library's GPU
  function ndsm_hip_lfff_box_device(nsrc, xs, ys, zs, dbz, alpha, nshape, x, y, z, which, dB) &
      bind(c, name="ndsm_hip_lfff_box_device") result(ierr)
    type(c_ptr), value :: nsrc, xs, ys, dbz, nshape, x, y, z, dB
    real(c_double), value :: zs, alpha
    integer(c_int), value :: which
    integer(c_int) :: ierr
    ierr = green_entry(.true., nsrc, xs, ys, zs, dbz, 0_c_int, c_null_ptr, nshape, x, y, z, which, dB, .true., &
                       "ndsm_hip_lfff_box_device", .true., alpha)
  end function

  ! ---- Flows from two magnetograms, the plane's vector potential and the boundary fluxes (include/ndsm_hip.h) ----
  ! No handle; the mesh vectors stay on the host in both forms.  B0, B1 (nsx,nsy,3) in; V (nsx,nsy,3), coef (nsx,nsy,9)
  ! and status (nsx,nsy; int32) out.  HOST arrays
  function ndsm_hip_flow_fit(nsrc, xs, ys, B0, B1, dt, r, rcond, V, coef, status) bind(c, name="ndsm_hip_flow_fit") &
      result(ierr)
    type(c_ptr), value :: nsrc, xs, ys, B0, B1, V, coef, status
    real(c_double), value :: dt, rcond
    integer(c_int), value :: r
    integer(c_int) :: ierr
    ierr = flow_entry(1, nsrc, xs, ys, [B0, B1, c_null_ptr], [V, coef, status], dt, r, rcond, 0_c_int, c_null_ptr, &
                      .false., "ndsm_hip_flow_fit")
  end function

  ! the same with B0, B1, V, coef and status DEVICE arrays of the library's GPU
  function ndsm_hip_flow_fit_device(nsrc, xs, ys, dB0, dB1, dt, r, rcond, dV, dcoef, dstatus) &
      bind(c, name="ndsm_hip_flow_fit_device") result(ierr)
    type(c_ptr), value :: nsrc, xs, ys, dB0, dB1, dV, dcoef, dstatus
    real(c_double), value :: dt, rcond
    integer(c_int), value :: r
    integer(c_int) :: ierr
    ierr = flow_entry(1, nsrc, xs, ys, [dB0, dB1, c_null_ptr], [dV, dcoef, dstatus], dt, r, rcond, 0_c_int, &
                      c_null_ptr, .true., "ndsm_hip_flow_fit_device")
  end function

  ! B, V (nsx,nsy,3), Ap (nsx,nsy,2) in; dens (nsx,nsy,4) out; out (8) on the HOST in both forms.  HOST arrays
  function ndsm_hip_flow_flux(nsrc, xs, ys, B, V, Ap, dens, out) bind(c, name="ndsm_hip_flow_flux") result(ierr)
    type(c_ptr), value :: nsrc, xs, ys, B, V, Ap, dens, out
    integer(c_int) :: ierr
    ierr = flow_entry(2, nsrc, xs, ys, [B, V, Ap], [dens, c_null_ptr, c_null_ptr], 0.0_c_double, 0_c_int, &
                      0.0_c_double, 0_c_int, out, .false., "ndsm_hip_flow_flux")
  end function

  ! the same with B, V, Ap and dens DEVICE arrays of the library's GPU
  function ndsm_hip_flow_flux_device(nsrc, xs, ys, dB, dV, dAp, ddens, out) bind(c, name="ndsm_hip_flow_flux_device") &
      result(ierr)
    type(c_ptr), value :: nsrc, xs, ys, dB, dV, dAp, ddens, out
    integer(c_int) :: ierr
    ierr = flow_entry(2, nsrc, xs, ys, [dB, dV, dAp], [ddens, c_null_ptr, c_null_ptr], 0.0_c_double, 0_c_int, &
                      0.0_c_double, 0_c_int, out, .true., "ndsm_hip_flow_flux_device")
  end function

  ! bz (nsx,nsy) in; Ap (nsx,nsy,2) on the source's own nodes out.  HOST arrays
  function ndsm_hip_green_ap_plane(nsrc, xs, ys, bz, Ap) bind(c, name="ndsm_hip_green_ap_plane") result(ierr)
    type(c_ptr), value :: nsrc, xs, ys, bz, Ap
    integer(c_int) :: ierr
    ierr = flow_entry(3, nsrc, xs, ys, [bz, c_null_ptr, c_null_ptr], [Ap, c_null_ptr, c_null_ptr], 0.0_c_double, &
                      0_c_int, 0.0_c_double, 0_c_int, c_null_ptr, .false., "ndsm_hip_green_ap_plane")
  end function

  ! the same with bz and Ap DEVICE arrays of the library's GPU
  function ndsm_hip_green_ap_plane_device(nsrc, xs, ys, dbz, dAp) bind(c, name="ndsm_hip_green_ap_plane_device") &
      result(ierr)
    type(c_ptr), value :: nsrc, xs, ys, dbz, dAp
    integer(c_int) :: ierr
    ierr = flow_entry(3, nsrc, xs, ys, [dbz, c_null_ptr, c_null_ptr], [dAp, c_null_ptr, c_null_ptr], 0.0_c_double, &
                      0_c_int, 0.0_c_double, 0_c_int, c_null_ptr, .true., "ndsm_hip_green_ap_plane_device")
  end function

  ! bz (nsx,nsy) and pts (2,npts) in; Ap (2,npts) out.  HOST arrays
  function ndsm_hip_green_ap_points(nsrc, xs, ys, bz, npts, pts, Ap) bind(c, name="ndsm_hip_green_ap_points") &
      result(ierr)
    type(c_ptr), value :: nsrc, xs, ys, bz, pts, Ap
    integer(c_int), value :: npts
    integer(c_int) :: ierr
    ierr = flow_entry(4, nsrc, xs, ys, [bz, pts, c_null_ptr], [Ap, c_null_ptr, c_null_ptr], 0.0_c_double, 0_c_int, &
                      0.0_c_double, npts, c_null_ptr, .false., "ndsm_hip_green_ap_points")
  end function

  ! the same with bz, pts and Ap DEVICE arrays of the library's GPU
  function ndsm_hip_green_ap_points_device(nsrc, xs, ys, dbz, npts, dpts, dAp) &
      bind(c, name="ndsm_hip_green_ap_points_device") result(ierr)
    type(c_ptr), value :: nsrc, xs, ys, dbz, dpts, dAp
    integer(c_int), value :: npts
    integer(c_int) :: ierr
    ierr = flow_entry(4, nsrc, xs, ys, [dbz, dpts, c_null_ptr], [dAp, c_null_ptr, c_null_ptr], 0.0_c_double, 0_c_int, &
                      0.0_c_double, npts, c_null_ptr, .true., "ndsm_hip_green_ap_points_device")
  end function

  ! The eight entries above.  kind 1: the fit, 2: the fluxes, 3: the vector potential on the source's nodes, 4: at
  ! points.  pin, pout: the arrays a kind reads and writes, in the order of its launcher; the host forms stage them in
  ! one allocation and copy the outputs back, the device forms pass them on.  In this order: 9001 without a GPU; 9001
  ! from the memory screen as soon as the shapes can be read; 9002; 9004; nothing is written before the launch.
  function flow_entry(kind, nsrc, xs, ys, pin, pout, dt, r, rcond, npts, out8, on_device, who) result(ierr)
    integer, intent(in) :: kind
    type(c_ptr), intent(in) :: nsrc, xs, ys, pin(3), pout(3), out8
    real(c_double), intent(in) :: dt, rcond
    integer(c_int), intent(in) :: r, npts
    logical, intent(in) :: on_device
    character(len=*), intent(in) :: who
    integer(c_int) :: ierr
    integer(c_int), pointer :: ns(:)
    integer(c_int32_t) :: ns2(2)
    integer :: nin, nout, i, d
    real(c_double) :: bin(3), bout(3), npix, total
    integer(c_size_t) :: off(6), at
    type(c_ptr) :: buf, din(3), dout(3)
    integer(c_int) :: rc
    ierr = ndsmk_init(-1_c_int)
    if (ierr /= 0) return
    nin = merge(2, merge(3, merge(1, 2, kind == 3), kind == 2), kind == 1)
    nout = merge(3, 1, kind == 1)
    bin = 0.0_c_double; bout = 0.0_c_double
    ! a call the device cannot hold is refused before anything is allocated - as soon as its shapes can be read
    if (c_associated(nsrc)) then
      call c_f_pointer(nsrc, ns, [2])
      ns2 = ns
      if (all(ns2 >= 1) .and. npts >= 0) then
        npix = product(real(ns2, c_double))            ! (in doubles: past the screen the sizes fit whole numbers)
        select case (kind)
        case (1); bin(1:2) = 24.0_c_double * npix; bout = [24.0_c_double, 72.0_c_double, 4.0_c_double] * npix
        case (2); bin = [24.0_c_double, 24.0_c_double, 16.0_c_double] * npix; bout(1) = 32.0_c_double * npix
        case (3); bin(1) = 8.0_c_double * npix; bout(1) = 16.0_c_double * npix
        case default
          bin(1) = 8.0_c_double * npix; bin(2) = 16.0_c_double * real(npts, c_double)
          bout(1) = 16.0_c_double * real(npts, c_double)
        end select
        total = merge(0.0_c_double, sum(bin) + sum(bout), on_device)
        if (kind <= 2) then
          ierr = ndsmk_flow_fits(ns2, merge(1_c_int, 0_c_int, kind == 1), total)
        else
          ierr = ndsmk_green_fits(ns2, c_null_ptr, 1_c_int, &
                                  merge(int(npts, c_long_long), int(npix, c_long_long), kind == 4), total)
        end if
        if (ierr /= 0) return
      end if
    end if
    ierr = NDSMK_EARG
    if (.not. (c_associated(nsrc) .and. c_associated(xs) .and. c_associated(ys) .and. c_associated(pin(1)))) return
    if (kind /= 4) then
      do i = 1, nin
        if (.not. c_associated(pin(i))) return
      end do
      do i = 1, nout
        if (.not. c_associated(pout(i))) return
      end do
    end if
    if (kind == 2 .and. .not. c_associated(out8)) return
    ierr = green_source_ok(ns, xs, ys)
    if (ierr == 0 .and. npts < 0) ierr = NDSMK_EVALUE
    if (ierr == 0 .and. kind == 1) then
      if (any(ns < 3) .or. .not. (abs(dt) <= huge(dt)) .or. dt == 0.0_c_double .or. r < 1 .or. r > 16 .or. &
          .not. (rcond >= 0.0_c_double .and. rcond < 1.0_c_double)) ierr = NDSMK_EVALUE       ! (a NaN fails them too)
    end if
    if (ierr /= 0) then
      ierr = ndsmk_note_error(NDSMK_EVALUE, "flow: at least 2 nodes per axis (the fit: 3), spacings > 0, npts >= 0, "// &
                              "(the fit) a finite dt /= 0, 1 <= r <= 16 and 0 <= rcond < 1"//c_null_char)
      return
    end if
    if (kind == 4) then
      if (npts == 0) return
      ierr = NDSMK_EARG
      if (.not. (c_associated(pin(2)) .and. c_associated(pout(1)))) return
    end if
    if (on_device) then
      rc = launch(pin, pout)
    else
      at = 0
      do i = 1, nin
        off(i) = at; at = at + int(bin(i), c_size_t)
      end do
      do i = 1, nout
        off(3 + i) = at; at = at + int(bout(i), c_size_t)
      end do
      buf = c_null_ptr
      din = c_null_ptr; dout = c_null_ptr
      rc = ndsmk_alloc(buf, at)
      if (rc == 0) then
        do i = 1, nin
          din(i) = dptr_offset(buf, off(i))
          if (rc == 0) rc = ndsmk_h2d(din(i), pin(i), int(bin(i), c_size_t))
        end do
        do i = 1, nout
          dout(i) = dptr_offset(buf, off(3 + i))
        end do
        if (rc == 0) rc = launch(din, dout)
        do i = 1, nout
          if (rc == 0) rc = ndsmk_d2h(pout(i), dout(i), int(bout(i), c_size_t))
        end do
        d = ndsmk_free(buf)
        if (rc == 0) rc = int(d, c_int)
      end if
    end if
    ierr = reported(who, rc)
  contains
    function launch(a, b) result(lrc)
      type(c_ptr), intent(in) :: a(3), b(3)
      integer(c_int) :: lrc
      select case (kind)
      case (1); lrc = ndsmk_flow_fit(ns2, xs, ys, a(1), a(2), dt, r, rcond, b(1), b(2), b(3))
      case (2); lrc = ndsmk_flow_flux(ns2, xs, ys, a(1), a(2), a(3), b(1), out8)
      case (3); lrc = ndsmk_green_ap_plane(ns2, xs, ys, a(1), b(1))
      case default; lrc = ndsmk_green_ap_points(ns2, xs, ys, a(1), npts, a(2), b(1))
      end select
    end function
  end function

  ! ---- Flux partitioning of a magnetogram (include/ndsm_hip.h, ndsm_hip_partition) ----
  ! No handle; the mesh vectors and counts (2, int64) stay on the host in both forms.  bz (nsx,nsy) in; label (nsx,nsy;
  ! int32) and the first min(K, max_patches) rows of root (int64), sign (int32), npix (int64), flux, sx, sy out.
  ! HOST arrays
  function ndsm_hip_partition(nsrc, xs, ys, bz, thr, max_patches, counts, label, root, sign, npix, flux, sx, sy) &
      bind(c, name="ndsm_hip_partition") result(ierr)
    type(c_ptr), value :: nsrc, xs, ys, bz, counts, label, root, sign, npix, flux, sx, sy
    real(c_double), value :: thr
    integer(c_int64_t), value :: max_patches
    integer(c_int) :: ierr
    ierr = partition_entry(nsrc, xs, ys, bz, thr, max_patches, counts, label, [root, sign, npix, flux, sx, sy], .false., &
                           "ndsm_hip_partition")
  end function

  ! the same with bz, label and the record arrays DEVICE arrays of the library's GPU
  function ndsm_hip_partition_device(nsrc, xs, ys, dbz, thr, max_patches, counts, dlabel, droot, dsign, dnpix, dflux, dsx, &
                                     dsy) bind(c, name="ndsm_hip_partition_device") result(ierr)
    type(c_ptr), value :: nsrc, xs, ys, dbz, counts, dlabel, droot, dsign, dnpix, dflux, dsx, dsy
    real(c_double), value :: thr
    integer(c_int64_t), value :: max_patches
    integer(c_int) :: ierr
    ierr = partition_entry(nsrc, xs, ys, dbz, thr, max_patches, counts, dlabel, [droot, dsign, dnpix, dflux, dsx, dsy], &
                           .true., "ndsm_hip_partition_device")
  end function

  ! The two entries above.  The host form stages bz, label and the max_patches rows of the records in one allocation
  ! and copies the outputs back, the device form passes its arrays on.  In this order: 9001 without a GPU; 9001 from
  ! the memory screen as soon as the shapes can be read; 9002; 9004.  On every failure counts is cleared; the host form
  ! also clears the max_patches rows of its records and, once the shape has passed its checks, label.
  function partition_entry(nsrc, xs, ys, bz, thr, max_patches, counts, label, rec, on_device, who) result(ierr)
    type(c_ptr), intent(in) :: nsrc, xs, ys, bz, counts, label, rec(6)
    real(c_double), intent(in) :: thr
    integer(c_int64_t), intent(in) :: max_patches
    logical, intent(in) :: on_device
    character(len=*), intent(in) :: who
    integer(c_int) :: ierr
    integer, parameter :: width(6) = [8, 4, 8, 8, 8, 8]
    integer(c_int), pointer :: ns(:)
    integer(c_int64_t), pointer :: cnt(:)
    integer(c_int32_t) :: ns2(2)
    integer(c_int64_t) :: npix, rows
    integer(c_size_t) :: off(8), at, nb
    real(c_double) :: total
    type(c_ptr) :: buf, d(8)
    integer(c_int) :: rc
    integer :: i
    logical :: shape_ok, complete
    shape_ok = .false.
    call clear_host([counts], [8], [2_c_int64_t])
    ierr = ndsmk_init(-1_c_int)
    if (ierr /= 0) return
    ! a call the device cannot hold is refused before anything is allocated - as soon as its shapes can be read
    if (c_associated(nsrc)) then
      call c_f_pointer(nsrc, ns, [2])
      ns2 = ns
      if (all(ns2 >= 1)) then
        total = product(real(ns2, c_double)) * 12.0_c_double
        if (max_patches > 0) total = total + 44.0_c_double * real(max_patches, c_double)
        ierr = ndsmk_partition_fits(ns2, merge(0.0_c_double, total, on_device))
        if (ierr /= 0) return
      end if
    end if
    ierr = NDSMK_EARG
    complete = c_associated(nsrc) .and. c_associated(xs) .and. c_associated(ys) .and. c_associated(bz) .and. &
               c_associated(counts) .and. c_associated(label)
    if (max_patches > 0) then
      do i = 1, 6
        complete = complete .and. c_associated(rec(i))
      end do
    end if
    if (.not. complete) then
      call clear_outputs()
      return
    end if
    ierr = green_source_ok(ns, xs, ys)
    if (ierr == 0 .and. (.not. (thr >= 0.0_c_double .and. thr <= huge(thr)) .or. max_patches < 0)) ierr = NDSMK_EVALUE
    if (ierr == 0 .and. product(int(ns2, c_int64_t)) > int(huge(0_c_int32_t), c_int64_t)) ierr = NDSMK_EVALUE
    if (ierr /= 0) then
      ierr = ndsmk_note_error(NDSMK_EVALUE, "partition: at least 2 nodes per axis, at most 2^31 - 1 pixels, "// &
                              "spacings > 0, a finite thr >= 0 and max_patches >= 0"//c_null_char)
      call clear_outputs()
      return
    end if
    shape_ok = .true.
    npix = product(int(ns2, c_int64_t))
    call c_f_pointer(counts, cnt, [2])
    if (on_device) then
      rc = ndsmk_partition(ns2, xs, ys, bz, thr, max_patches, cnt, label, rec(1), rec(2), rec(3), rec(4), rec(5), rec(6))
    else
      ! bz, label, then the records, each on a multiple of 8 bytes
      off(1) = 0
      off(2) = int(8 * npix, c_size_t)
      at = off(2) + int((4 * npix + 7) / 8 * 8, c_size_t)
      do i = 1, 6
        off(2 + i) = at
        at = at + int((width(i) * min(max_patches, npix) + 7) / 8 * 8, c_size_t)     ! (K <= npix)
      end do
      buf = c_null_ptr
      rc = ndsmk_alloc(buf, at)
      if (rc == 0) then
        do i = 1, 8
          d(i) = dptr_offset(buf, off(i))
        end do
        rc = ndsmk_h2d(d(1), bz, int(8 * npix, c_size_t))
        if (rc == 0) rc = ndsmk_partition(ns2, xs, ys, d(1), thr, max_patches, cnt, d(2), d(3), d(4), d(5), d(6), d(7), &
                                          d(8))
        if (rc == 0) rc = ndsmk_d2h(label, d(2), int(4 * npix, c_size_t))
        rows = 0
        if (rc == 0) rows = min(cnt(2), max_patches)
        do i = 1, 6
          nb = int(width(i) * rows, c_size_t)
          if (rc == 0 .and. nb > 0) rc = ndsmk_d2h(rec(i), d(2 + i), nb)
        end do
        i = ndsmk_free(buf)
        if (rc == 0) rc = int(i, c_int)
      end if
    end if
    if (rc == 0) rc = ndsmk_sync()
    ierr = reported(who, rc)
    if (ierr /= 0) call clear_outputs()
  contains
    subroutine clear_outputs()
      call clear_host([counts], [8], [2_c_int64_t])
      if (on_device) return
      if (shape_ok) call clear_host([label], [4], [product(int(ns2, c_int64_t))])
      if (max_patches <= 0 .or. max_patches > huge(0_c_int64_t) / 8) return
      call clear_host(rec, width, [max_patches, max_patches, max_patches, max_patches, max_patches, max_patches])
    end subroutine
  end function

  ! The open-box potential field: ndsm_hip_green_box_device (which = 0) on the handle's mesh into the device B, then
  ! ndsm_hip_vecpot_solve_device - bit for bit that composition, no field crossing PCIe in between.  A: in the first
  ! guess, out A; B: out (its interior nodes are read by nothing).  HOST arrays (nx,ny,nz,3), bz (nsx,nsy)
  function ndsm_hip_vecpot_open(handle, ioptc, ropt, nsrc, xs, ys, zs, bz, A, B) bind(c, name="ndsm_hip_vecpot_open") &
      result(ierr)
    type(c_ptr), value :: handle, nsrc, xs, ys, bz, A, B
    integer(c_int), intent(inout) :: ioptc(0:OPT_LEN - 1)
    real(c_double), intent(inout) :: ropt(0:OPT_LEN - 1)
    real(c_double), value :: zs
    integer(c_int) :: ierr
    ierr = vecpot_handle_open(handle, ioptc, ropt, nsrc, xs, ys, zs, bz, A, B, .false., "ndsm_hip_vecpot_open")
  end function

  ! the same with bz, A and B DEVICE arrays of the library's GPU; the face nodes of dB are written, then the solve runs
  function ndsm_hip_vecpot_open_device(handle, ioptc, ropt, nsrc, xs, ys, zs, dbz, dA, dB) &
      bind(c, name="ndsm_hip_vecpot_open_device") result(ierr)
    type(c_ptr), value :: handle, nsrc, xs, ys, dbz, dA, dB
    integer(c_int), intent(inout) :: ioptc(0:OPT_LEN - 1)
    real(c_double), intent(inout) :: ropt(0:OPT_LEN - 1)
    real(c_double), value :: zs
    integer(c_int) :: ierr
    ierr = vecpot_handle_open(handle, ioptc, ropt, nsrc, xs, ys, zs, dbz, dA, dB, .true., "ndsm_hip_vecpot_open_device")
  end function

  function vecpot_handle_open(handle, ioptc, ropt, nsrc, xs, ys, zs, bz, A, B, on_device, who) result(ierr)
    type(c_ptr), intent(in) :: handle, nsrc, xs, ys, bz, A, B
    integer(c_int), intent(inout) :: ioptc(0:OPT_LEN - 1)
    real(c_double), intent(inout) :: ropt(0:OPT_LEN - 1)
    real(c_double), intent(in) :: zs
    logical, intent(in) :: on_device
    character(len=*), intent(in) :: who
    integer(c_int) :: ierr
    type(vecpot_ctx), pointer :: ctx
    integer(c_int), pointer :: ns(:)
    integer(c_int32_t) :: ns2(2)
    integer(c_int32_t), target :: n3(3)
    integer(c_size_t) :: bsrc, nb3
    type(c_ptr) :: buf, dA, dB
    integer(c_int) :: rc
    integer :: d
    ierr = live_ctx(handle, ctx)
    if (ierr /= 0) return
    n3 = ctx%n3
    ! as in green_entry: refused before anything is allocated, as soon as the shapes can be read (in doubles)
    if (c_associated(nsrc)) then
      call c_f_pointer(nsrc, ns, [2])
      ns2 = ns
      if (all(ns2 >= 1)) then
        ierr = ndsmk_green_fits(ns2, c_loc(n3), 0_c_int, 0_c_long_long, &
                                merge(0.0_c_double, 8.0_c_double * product(real(ns2, c_double)) + &
                                      48.0_c_double * product(real(n3, c_double)), on_device))
        if (ierr /= 0) return
      end if
    end if
    ierr = NDSMK_EARG
    if (.not. (c_associated(nsrc) .and. c_associated(xs) .and. c_associated(ys) .and. c_associated(bz) .and. &
               c_associated(A) .and. c_associated(B))) return
    ierr = green_source_ok(ns, xs, ys)
    if (ierr == 0 .and. .not. (ctx%qz(1) >= zs)) ierr = NDSMK_EVALUE
    if (ierr /= 0) then
      ierr = ndsmk_note_error(NDSMK_EVALUE, "vecpot_open: at least 2 source nodes per axis, spacings > 0 and "// &
                              "z[0] >= zs"//c_null_char)
      return
    end if
    bsrc = int(product(int(ns2, c_int64_t)) * 8_c_int64_t, c_size_t)
    nb3 = int(product(int(n3, c_int64_t)) * 24_c_int64_t, c_size_t)
    if (on_device) then
      rc = ndsmk_green_box(ns2, xs, ys, zs, bz, n3, c_loc(ctx%qx), c_loc(ctx%qy), c_loc(ctx%qz), 0_c_int, B)
      ierr = reported(who, rc)
      if (ierr == 0) ierr = vecpot_handle_solve(handle, ioptc, ropt, A, B, .true., who)
    else
      ! bz, A and a B of zeros on the device; only A and B come home
      buf = c_null_ptr
      rc = ndsmk_alloc(buf, bsrc + 2_c_size_t * nb3)
      if (rc == 0) then
        dA = dptr_offset(buf, bsrc)
        dB = dptr_offset(buf, bsrc + nb3)
        rc = ndsmk_h2d(buf, bz, bsrc)
        if (rc == 0) rc = ndsmk_h2d(dA, A, nb3)
        if (rc == 0) rc = ndsmk_fill0(dB, nb3)
        if (rc == 0) rc = ndsmk_green_box(ns2, xs, ys, zs, buf, n3, c_loc(ctx%qx), c_loc(ctx%qy), c_loc(ctx%qz), &
                                          0_c_int, dB)
        ierr = reported(who, rc)
        if (ierr == 0) then
          ierr = vecpot_handle_solve(handle, ioptc, ropt, dA, dB, .true., who)
          if (ierr < NDSMK_ENODEV) then
            rc = ndsmk_d2h(A, dA, nb3)
            if (rc == 0) rc = ndsmk_d2h(B, dB, nb3)
            if (rc /= 0) ierr = reported(who, rc)
          end if
        end if
        d = ndsmk_free(buf)
        if (ierr < NDSMK_ENODEV .and. d /= 0) ierr = reported(who, int(d, c_int))
      else
        ierr = reported(who, rc)
      end if
    end if
  end function

  ! The coarse-to-fine cascade of the optimization method (semantics in include/ndsm_hip.h).  handles (nlevels): the
  ! finest mesh's handle first, then coarser meshes of the same box.  B (nx,ny,nz,3) and w (nx,ny,nz; may be NULL) on
  ! the finest mesh, as for ndsm_hip_vecpot_optimize.  niter_max, dt0, dt_min (nlevels) per level; hist
  ! (nlevels,hist_rows,6) and info (nlevels,3) out, on the HOST in both entries.  HOST arrays
  function ndsm_hip_vecpot_optimize_cascade(handles, nlevels, ioptc, ropt, B, w, start, niter_max, check, tol, dt0, &
                                            dt_min, hist, hist_rows, info) &
      bind(c, name="ndsm_hip_vecpot_optimize_cascade") result(ierr)
    type(c_ptr), value :: handles, B, w, niter_max, dt0, dt_min, hist, info
    integer(c_int), intent(inout) :: ioptc(0:OPT_LEN - 1)
    real(c_double), intent(inout) :: ropt(0:OPT_LEN - 1)
    integer(c_int), value :: nlevels, start, check, hist_rows
    real(c_double), value :: tol
    integer(c_int) :: ierr
    ierr = vecpot_handle_cascade(handles, nlevels, ioptc, ropt, B, w, start, niter_max, check, tol, dt0, dt_min, hist, &
                                 hist_rows, info, .false., "ndsm_hip_vecpot_optimize_cascade")
  end function

  ! the same on DEVICE arrays of the library's GPU: only history rows cross PCIe
  function ndsm_hip_vecpot_optimize_cascade_device(handles, nlevels, ioptc, ropt, dB, dw, start, niter_max, check, tol, &
                                                   dt0, dt_min, hist, hist_rows, info) &
      bind(c, name="ndsm_hip_vecpot_optimize_cascade_device") result(ierr)
    type(c_ptr), value :: handles, dB, dw, niter_max, dt0, dt_min, hist, info
    integer(c_int), intent(inout) :: ioptc(0:OPT_LEN - 1)
    real(c_double), intent(inout) :: ropt(0:OPT_LEN - 1)
    integer(c_int), value :: nlevels, start, check, hist_rows
    real(c_double), value :: tol
    integer(c_int) :: ierr
    ierr = vecpot_handle_cascade(handles, nlevels, ioptc, ropt, dB, dw, start, niter_max, check, tol, dt0, dt_min, &
                                 hist, hist_rows, info, .true., "ndsm_hip_vecpot_optimize_cascade_device")
  end function

  ! the two entries above and the two below: with Bobs (and then wm, nu, free) every level is the measurement fit
  function vecpot_handle_cascade(handles, nlevels, ioptc, ropt, B, w, start, niter_max, check, tol, dt0, dt_min, hist, &
                                 hist_rows, info, on_device, who, Bobs, wm, nu, free) result(ierr)
    type(c_ptr), intent(in) :: handles, B, w, niter_max, dt0, dt_min, hist, info
    type(c_ptr), intent(in), optional :: Bobs, wm, nu
    integer(c_int), intent(in), optional :: free
    integer(c_int), intent(inout) :: ioptc(0:OPT_LEN - 1)
    real(c_double), intent(inout) :: ropt(0:OPT_LEN - 1)
    integer(c_int), intent(in) :: nlevels, start, check, hist_rows
    real(c_double), intent(in) :: tol
    logical, intent(in) :: on_device
    character(len=*), intent(in) :: who
    integer(c_int) :: ierr
    type(vecpot_ref), allocatable :: lev(:)
    type(optimize_args), allocatable :: ops(:)
    type(c_ptr), pointer :: hs(:)
    integer(c_int), pointer :: iout(:, :), nit(:)
    real(c_double), pointer :: d0(:), dm(:), nul(:)
    integer(ik) :: iopt(0:OPT_LEN - 1)
    real(c_double) :: t0
    integer(c_int) :: rc
    integer :: l, width
    logical :: ok, obs
    obs = present(Bobs)
    width = merge(7, 6, obs)
    nullify (iout)
    if (c_associated(info) .and. nlevels >= 1) then
      call c_f_pointer(info, iout, [3, int(nlevels)])
      iout = 0
    end if
    ierr = ndsmk_init(-1_c_int)
    if (ierr == 0 .and. .not. (c_associated(handles) .and. c_associated(B) .and. c_associated(niter_max) .and. &
                               c_associated(dt0) .and. c_associated(dt_min) .and. c_associated(hist) .and. &
                               c_associated(info))) ierr = NDSMK_EARG
    if (ierr == 0 .and. obs) then
      if (.not. (c_associated(Bobs) .and. c_associated(nu))) ierr = NDSMK_EARG
    end if
    if (ierr == 0 .and. nlevels >= 1) then
      call c_f_pointer(handles, hs, [int(nlevels)])
      allocate (lev(nlevels), ops(nlevels))
      do l = 1, nlevels
        if (ierr == 0) ierr = live_ctx(hs(l), lev(l)%p)
      end do
    end if
    if (ierr == 0) then
      ok = nlevels >= 1 .and. start >= 0 .and. start <= 1 .and. check >= 1 .and. hist_rows >= 2 .and. tol >= 0.0_c_double &
           .and. tol <= huge(tol)
      if (ok) then
        call c_f_pointer(niter_max, nit, [int(nlevels)])
        call c_f_pointer(dt0, d0, [int(nlevels)])
        call c_f_pointer(dt_min, dm, [int(nlevels)])
        do l = 1, nlevels
          ok = ok .and. nit(l) >= 1 .and. d0(l) > 0.0_c_double .and. d0(l) <= huge(tol) .and. dm(l) >= 0.0_c_double &
               .and. dm(l) <= huge(tol)
        end do
      end if
      if (ok .and. obs) then
        ok = free == 0 .or. free == 1
        call c_f_pointer(nu, nul, [int(nlevels)])
        do l = 1, nlevels
          ok = ok .and. nul(l) >= 0.0_c_double .and. nul(l) <= huge(tol)
        end do
        if (.not. ok) &
          ierr = ndsmk_note_error(NDSMK_EVALUE, "optimize_obs cascade: free 0 or 1, and on every level nu >= 0 "// &
                                  "(finite)"//c_null_char)
      else if (.not. ok) then
        ierr = ndsmk_note_error(NDSMK_EVALUE, "optimize cascade: nlevels >= 1, start 0 or 1, check >= 1, hist_rows >= 2, "// &
                                "tol >= 0, and on every level niter_max >= 1, dt0 > 0 and dt_min >= 0 (all finite)"// &
                                c_null_char)
      end if
    end if
    if (ierr == 0) then
      do l = 2, nlevels
        ok = ok .and. all(lev(l)%p%n3 <= lev(l - 1)%p%n3) .and. same_box(lev(l)%p, lev(1)%p)
      end do
      if (.not. ok) &
        ierr = ndsmk_note_error(NDSMK_EVALUE, "optimize cascade: every level spans the box of the finest mesh (the first "// &
                                "and last coordinates are compared bit for bit) with no more nodes per axis than the "// &
                                "level before it"//c_null_char)
    end if
    if (ierr == 0) then
      do l = 1, nlevels
        ops(l)%hist = dptr_offset(hist, int(l - 1, c_size_t) * int(hist_rows, c_size_t) * int(8 * width, c_size_t))
        ops(l)%start = start; ops(l)%niter_max = nit(l); ops(l)%check = check; ops(l)%hist_rows = hist_rows
        ops(l)%tol = tol; ops(l)%dt0 = d0(l); ops(l)%dt_min = dm(l)
        if (obs) then
          ops(l)%nu = nul(l); ops(l)%free = free
        end if
      end do
      ops(1)%w = w
      if (obs) then
        ops(1)%bobs = Bobs; ops(1)%wm = wm
      end if
      iopt = ioptc
      verbose = (iopt(IOPT_DEBUG) == 1)
      t0 = wall_seconds()
      rc = NDSMK_EARG
      if (int(iopt(IOPT_NGRIDS)) == lev(nlevels)%p%ngr) rc = vecpot_optimize_cascade(lev, iopt, ropt, B, ops, on_device)
      ropt(ROPT_TIM) = wall_seconds() - t0
      ioptc = int(iopt, c_int)
      ierr = reported(who, rc)
      if (ierr /= 0) ioptc(IOPT_IERR) = ierr            ! (as the field entries: ioptc is written by a call that ran)
      if (ierr == 0) then
        do l = 1, nlevels
          iout(:, l) = ops(l)%info
        end do
        ierr = int(iopt(IOPT_IERR), c_int)
      end if
    end if
    if (ierr >= NDSMK_ENODEV) then
      if (associated(iout)) iout = 0
      if (c_associated(hist) .and. hist_rows >= 1 .and. nlevels >= 1) &
        call clear_host([hist], [8 * width], [int(hist_rows, c_int64_t) * int(nlevels, c_int64_t)])
    end if
  contains
    ! the first and the last node of every axis, bit for bit
    function same_box(a, b) result(yes)
      type(vecpot_ctx), intent(in) :: a, b
      logical :: yes
      yes = same_bits(a%qx(1), b%qx(1)) .and. same_bits(a%qx(size(a%qx)), b%qx(size(b%qx))) .and. &
            same_bits(a%qy(1), b%qy(1)) .and. same_bits(a%qy(size(a%qy)), b%qy(size(b%qy))) .and. &
            same_bits(a%qz(1), b%qz(1)) .and. same_bits(a%qz(size(a%qz)), b%qz(size(b%qz)))
    end function
    function same_bits(u, v) result(yes)
      real(c_double), intent(in) :: u, v
      logical :: yes
      yes = transfer(u, 0_c_int64_t) == transfer(v, 0_c_int64_t)
    end function
  end function

  ! The cascade of the measurement fit (semantics in include/ndsm_hip.h): ndsm_hip_vecpot_optimize_cascade whose every
  ! level is ndsm_hip_vecpot_optimize_obs.  Bobs (nx,ny,3) and wm (nx,ny,3; may be NULL) on the finest mesh; nu
  ! (nlevels) per level, on the HOST in both entries; free 0 or 1.  hist (nlevels,hist_rows,7).  HOST arrays
  function ndsm_hip_vecpot_optimize_obs_cascade(handles, nlevels, ioptc, ropt, B, w, Bobs, wm, nu, free, start, &
                                                niter_max, check, tol, dt0, dt_min, hist, hist_rows, info) &
      bind(c, name="ndsm_hip_vecpot_optimize_obs_cascade") result(ierr)
    type(c_ptr), value :: handles, B, w, Bobs, wm, nu, niter_max, dt0, dt_min, hist, info
    integer(c_int), intent(inout) :: ioptc(0:OPT_LEN - 1)
    real(c_double), intent(inout) :: ropt(0:OPT_LEN - 1)
    integer(c_int), value :: nlevels, free, start, check, hist_rows
    real(c_double), value :: tol
    integer(c_int) :: ierr
    ierr = vecpot_handle_cascade(handles, nlevels, ioptc, ropt, B, w, start, niter_max, check, tol, dt0, dt_min, hist, &
                                 hist_rows, info, .false., "ndsm_hip_vecpot_optimize_obs_cascade", Bobs, wm, nu, free)
  end function

  ! the same on DEVICE arrays of the library's GPU: only history rows cross PCIe
  function ndsm_hip_vecpot_optimize_obs_cascade_device(handles, nlevels, ioptc, ropt, dB, dw, dBobs, dwm, nu, free, &
                                                       start, niter_max, check, tol, dt0, dt_min, hist, hist_rows, info) &
      bind(c, name="ndsm_hip_vecpot_optimize_obs_cascade_device") result(ierr)
    type(c_ptr), value :: handles, dB, dw, dBobs, dwm, nu, niter_max, dt0, dt_min, hist, info
    integer(c_int), intent(inout) :: ioptc(0:OPT_LEN - 1)
    real(c_double), intent(inout) :: ropt(0:OPT_LEN - 1)
    integer(c_int), value :: nlevels, free, start, check, hist_rows
    real(c_double), value :: tol
    integer(c_int) :: ierr
    ierr = vecpot_handle_cascade(handles, nlevels, ioptc, ropt, dB, dw, start, niter_max, check, tol, dt0, dt_min, &
                                 hist, hist_rows, info, .true., "ndsm_hip_vecpot_optimize_obs_cascade_device", dBobs, &
                                 dwm, nu, free)
  end function

  ! The confidence-weighted restriction of an observation with its confidence (semantics in include/ndsm_hip.h).  src,
  ! wsrc (nsrc,ncomp) in, dst, wdst (ndst,ncomp) out.  No handle.  HOST arrays
  function ndsm_hip_resample_weighted(nsrc, ndst, ncomp, src, wsrc, dst, wdst) &
      bind(c, name="ndsm_hip_resample_weighted") result(ierr)
    type(c_ptr), value :: nsrc, ndst, src, wsrc, dst, wdst
    integer(c_int), value :: ncomp
    integer(c_int) :: ierr
    ierr = resample_weighted_entry(nsrc, ndst, ncomp, src, wsrc, dst, wdst, .false., "ndsm_hip_resample_weighted")
  end function

  ! the same on DEVICE arrays of the library's GPU (they must not overlap)
  function ndsm_hip_resample_weighted_device(nsrc, ndst, ncomp, dsrc, dwsrc, ddst, dwdst) &
      bind(c, name="ndsm_hip_resample_weighted_device") result(ierr)
    type(c_ptr), value :: nsrc, ndst, dsrc, dwsrc, ddst, dwdst
    integer(c_int), value :: ncomp
    integer(c_int) :: ierr
    ierr = resample_weighted_entry(nsrc, ndst, ncomp, dsrc, dwsrc, ddst, dwdst, .true., &
                                   "ndsm_hip_resample_weighted_device")
  end function

  function resample_weighted_entry(nsrc, ndst, ncomp, src, wsrc, dst, wdst, on_device, who) result(ierr)
    type(c_ptr), intent(in) :: nsrc, ndst, src, wsrc, dst, wdst
    integer(c_int), intent(in) :: ncomp
    logical, intent(in) :: on_device
    character(len=*), intent(in) :: who
    integer(c_int) :: ierr
    integer(c_int), pointer :: ns(:), nd(:)
    integer(c_int32_t) :: ns3(3), nd3(3)
    integer(c_size_t) :: bs, bd
    type(c_ptr) :: buf, dwsrc, ddst, dwdst
    integer(c_int) :: rc
    integer :: d
    logical :: ok
    ierr = ndsmk_init(-1_c_int)
    if (ierr /= 0) return
    ierr = NDSMK_EARG
    if (.not. (c_associated(nsrc) .and. c_associated(ndst) .and. c_associated(src) .and. c_associated(wsrc) .and. &
               c_associated(dst) .and. c_associated(wdst))) return
    call c_f_pointer(nsrc, ns, [3])
    call c_f_pointer(ndst, nd, [3])
    ok = ncomp >= 1
    do d = 1, 3
      ok = ok .and. ((ns(d) == 1 .and. nd(d) == 1) .or. (ns(d) >= 2 .and. nd(d) >= 2)) .and. nd(d) <= ns(d)
    end do
    if (.not. ok) then
      ierr = ndsmk_note_error(NDSMK_EVALUE, "resample_weighted: ncomp >= 1, at least 2 nodes per axis on both sides "// &
                              "(or 1 on both), and no axis finer than its source"//c_null_char)
      return
    end if
    ns3 = ns; nd3 = nd
    if (on_device) then
      rc = ndsmk_resample_weighted(ns3, nd3, ncomp, src, wsrc, dst, wdst)
      if (rc == 0) rc = ndsmk_sync()
    else
      bs = int(product(int(ns3, c_int64_t)) * int(ncomp, c_int64_t) * 8_c_int64_t, c_size_t)
      bd = int(product(int(nd3, c_int64_t)) * int(ncomp, c_int64_t) * 8_c_int64_t, c_size_t)
      buf = c_null_ptr
      ! [src | wsrc | dst | wdst]
      rc = ndsmk_alloc(buf, 2_c_size_t * (bs + bd))
      if (rc == 0) then
        dwsrc = dptr_offset(buf, bs)
        ddst = dptr_offset(buf, 2_c_size_t * bs)
        dwdst = dptr_offset(buf, 2_c_size_t * bs + bd)
        rc = ndsmk_h2d(buf, src, bs)
        if (rc == 0) rc = ndsmk_h2d(dwsrc, wsrc, bs)
        if (rc == 0) rc = ndsmk_resample_weighted(ns3, nd3, ncomp, buf, dwsrc, ddst, dwdst)
        if (rc == 0) rc = ndsmk_d2h(dst, ddst, bd)
        if (rc == 0) rc = ndsmk_d2h(wdst, dwdst, bd)
        if (rc == 0) rc = ndsmk_sync()
        d = ndsmk_free(buf)
        if (rc == 0) rc = int(d, c_int)
      end if
    end if
    ierr = reported(who, rc)
  end function

  ! Magnetogram preprocessing (semantics in include/ndsm_hip.h).  B (nx,ny,3) in: the magnetogram on the handle's
  ! lower face; out: the preprocessed one.  obs (nx,ny,3) in, may be NULL (the input B).  mu (5) in.  hist (hist_rows,17)
  ! and info (3 ints) out, on the HOST in both entries.  HOST arrays
  function ndsm_hip_vecpot_preprocess(handle, B, obs, mu, niter_max, check, tol, dt0, dt_min, hist, hist_rows, info) &
      bind(c, name="ndsm_hip_vecpot_preprocess") result(ierr)
    type(c_ptr), value :: handle, B, obs, mu, hist, info
    integer(c_int), value :: niter_max, check, hist_rows
    real(c_double), value :: tol, dt0, dt_min
    integer(c_int) :: ierr
    ierr = vecpot_handle_preprocess(handle, B, obs, mu, niter_max, check, tol, dt0, dt_min, hist, hist_rows, info, &
                                    .false., "ndsm_hip_vecpot_preprocess")
  end function

  ! the same on DEVICE arrays of the library's GPU: only history rows cross PCIe
  function ndsm_hip_vecpot_preprocess_device(handle, dB, dobs, mu, niter_max, check, tol, dt0, dt_min, hist, &
                                             hist_rows, info) &
      bind(c, name="ndsm_hip_vecpot_preprocess_device") result(ierr)
    type(c_ptr), value :: handle, dB, dobs, mu, hist, info
    integer(c_int), value :: niter_max, check, hist_rows
    real(c_double), value :: tol, dt0, dt_min
    integer(c_int) :: ierr
    ierr = vecpot_handle_preprocess(handle, dB, dobs, mu, niter_max, check, tol, dt0, dt_min, hist, hist_rows, info, &
                                    .true., "ndsm_hip_vecpot_preprocess_device")
  end function

  function vecpot_handle_preprocess(handle, B, obs, mu, niter_max, check, tol, dt0, dt_min, hist, hist_rows, info, &
                                    on_device, who) result(ierr)
    type(c_ptr), intent(in) :: handle, B, obs, mu, hist, info
    integer(c_int), intent(in) :: niter_max, check, hist_rows
    real(c_double), intent(in) :: tol, dt0, dt_min
    logical, intent(in) :: on_device
    character(len=*), intent(in) :: who
    integer(c_int) :: ierr
    type(vecpot_ctx), pointer :: ctx
    type(preprocess_args) :: pp
    integer(c_int), pointer :: iout(:)
    real(c_double), pointer :: pmu(:)
    integer(c_int) :: rc
    if (c_associated(info)) then
      call c_f_pointer(info, iout, [3])
      iout = 0
    end if
    ierr = live_ctx(handle, ctx)
    if (ierr == 0 .and. .not. (c_associated(B) .and. c_associated(mu) .and. c_associated(hist) .and. &
                               c_associated(info))) ierr = NDSMK_EARG
    if (ierr == 0) then
      call c_f_pointer(mu, pmu, [5])
      pp%mu = pmu
      if (niter_max < 1 .or. check < 1 .or. hist_rows < 2 .or. &
          .not. all(pp%mu >= 0.0_c_double) .or. any(pp%mu > huge(tol)) .or. &
          .not. (tol >= 0.0_c_double) .or. tol > huge(tol) .or. .not. (dt0 > 0.0_c_double) .or. &
          dt0 > huge(dt0) .or. .not. (dt_min >= 0.0_c_double) .or. dt_min > huge(dt_min)) &
        ierr = ndsmk_note_error(NDSMK_EVALUE, "preprocess: mu >= 0, niter_max >= 1, check >= 1, hist_rows >= 2, "// &
                                "tol >= 0, dt0 > 0 and dt_min >= 0 (all finite)"//c_null_char)
    end if
    if (ierr == 0) then
      pp%obs = obs; pp%hist = hist
      pp%niter_max = niter_max; pp%check = check; pp%hist_rows = hist_rows
      pp%tol = tol; pp%dt0 = dt0; pp%dt_min = dt_min
      verbose = .false.
      rc = vecpot_preprocess(ctx, B, pp, on_device)
      ierr = reported(who, rc)
      if (ierr == 0) iout = pp%info
    end if
    if (ierr >= NDSMK_ENODEV) then
      if (c_associated(info)) iout = 0
      if (c_associated(hist) .and. hist_rows >= 1) call clear_host([hist], [136], [int(hist_rows, c_int64_t)])
    end if
  end function

  ! ---- shared by the handle entries of the line and null calls below ----------
  ! the prologue: the runtime is up (without a device: 9001, whatever the arguments), and handle is that of a live
  ! context, which comes back in ctx; else 9002
  function live_ctx(handle, ctx) result(rc)
    type(c_ptr), intent(in) :: handle
    type(vecpot_ctx), pointer, intent(out) :: ctx
    integer(c_int) :: rc
    nullify (ctx)
    rc = ndsmk_init(-1_c_int)
    if (rc /= 0) return
    rc = NDSMK_EARG
    if (.not. c_associated(handle)) return
    call c_f_pointer(handle, ctx)
    if (ctx%live) rc = 0
  end function

  ! the epilogue: an error of the driver is reported and comes back as 9001 at least
  function reported(who, rc) result(ierr)
    character(len=*), intent(in) :: who
    integer(c_int), intent(in) :: rc
    integer(c_int) :: ierr
    ierr = rc
    if (rc == 0) return
    call report(who, rc)
    if (ierr < NDSMK_ENODEV) ierr = NDSMK_ENODEV
  end function

  ! zeroes on the host: count entries of width bytes at every p that is not NULL
  subroutine clear_host(p, width, count)
    type(c_ptr), intent(in) :: p(:)
    integer, intent(in) :: width(:)
    integer(c_int64_t), intent(in) :: count(:)
    type(c_ptr) :: q
    integer :: i
    do i = 1, size(p)
      if (c_associated(p(i)) .and. count(i) > 0) &
        q = c_memset(p(i), 0_c_int, int(int(width(i), c_int64_t) * count(i), c_size_t))
    end do
  end subroutine

  ! the six line entries above: squash false, sel = direction, q = c_null_ptr for trace; squash true, sel = integrand
  ! for squash, and qperp given for squash_perp.  nl lines: 2 nseeds for squash and for both directions, else nseeds.
  function vecpot_handle_lines(handle, squash, B, G, sel, nseeds, seeds, step, max_steps, q, ends, length, integral, &
                               status, nsteps, on_device, who, qperp) result(ierr)
    type(c_ptr), intent(in) :: handle, B, G, seeds, q, ends, length, integral, status, nsteps
    type(c_ptr), intent(in), optional :: qperp
    logical, intent(in) :: squash, on_device
    integer(c_int), intent(in) :: sel, nseeds, max_steps
    real(c_double), intent(in) :: step
    character(len=*), intent(in) :: who
    integer(c_int) :: ierr
    type(vecpot_ctx), pointer :: ctx
    if (.not. on_device) call clear_outputs()
    ierr = live_ctx(handle, ctx)
    if (ierr /= 0) return
    ierr = NDSMK_EARG
    ! no seeds: no array is looked at
    if (nseeds > 0 .and. .not. (c_associated(B) .and. c_associated(seeds) .and. (c_associated(q) .or. .not. squash) .and. &
                                c_associated(ends) .and. c_associated(length) .and. c_associated(integral) .and. &
                                c_associated(status) .and. c_associated(nsteps))) return
    if (nseeds > 0 .and. present(qperp)) then
      if (.not. c_associated(qperp)) return
    end if
    ierr = reported(who, vecpot_lines(ctx, squash, B, G, sel, nseeds, seeds, step, max_steps, q, ends, length, integral, &
                                      status, nsteps, on_device, qperp))
    if (ierr /= 0 .and. .not. on_device) call clear_outputs()
  contains
    subroutine clear_outputs()
      integer(c_int64_t) :: ns, nl
      if (nseeds <= 0) return
      if (nseeds > huge(0) / 6) return
      ns = nseeds
      nl = ns * merge(2, 1, squash .or. sel == 0)
      call clear_host([q, ends, length, integral, status, nsteps], [8, 24, 8, 8, 4, 4], [ns, nl, nl, nl, nl, nl])
      if (present(qperp)) call clear_host([qperp], [8], [ns])
    end subroutine
  end function

  ! ---- field-line paths on the same handle ---------------------------------
  ! As the trace entries, with the points of every line: B, G, seeds, step, max_steps, direction and the five trace
  ! outputs as there; every >= 1 the stride in steps between stored points, max_points >= 0 the capacity of the point
  ! arrays (0: count only).  Out: offsets (nl + 1, int64), total (one int64, on the HOST in both entries), points
  ! (3,max_points), bpt, gpt (the same), ipt (max_points); bpt, gpt, ipt may be NULL.  Return value: 0, or >= 9001
  ! errors (9002 a NULL handle or total, with nseeds > 0 a NULL required array, with max_points > 0 also a NULL points;
  ! 9004 a scalar out of range).  On every failure total is cleared, and the host entry clears the nl entries of the
  ! trace outputs, the nl + 1 of offsets and the max_points slots of its point arrays.

  ! HOST arrays
  function ndsm_hip_vecpot_paths(handle, B, G, nseeds, seeds, step, max_steps, direction, every, max_points, ends, &
                                 length, integral, status, nsteps, offsets, total, points, bpt, gpt, ipt) &
      bind(c, name="ndsm_hip_vecpot_paths") result(ierr)
    type(c_ptr), value :: handle, B, G, seeds, ends, length, integral, status, nsteps, offsets, total, points, bpt, gpt, &
                          ipt
    integer(c_int), value :: nseeds, max_steps, direction, every
    integer(c_int64_t), value :: max_points
    real(c_double), value :: step
    integer(c_int) :: ierr
    ierr = vecpot_handle_paths(handle, B, G, nseeds, seeds, step, max_steps, direction, every, max_points, ends, &
                               length, integral, status, nsteps, offsets, total, points, bpt, gpt, ipt, .false., &
                               "ndsm_hip_vecpot_paths")
  end function

  ! the same on DEVICE arrays of the library's GPU (total stays on the host; no array is touched on the host)
  function ndsm_hip_vecpot_paths_device(handle, dB, dG, nseeds, dseeds, step, max_steps, direction, every, max_points, &
                                        dends, dlength, dintegral, dstatus, dnsteps, doffsets, total, dpoints, dbpt, &
                                        dgpt, dipt) bind(c, name="ndsm_hip_vecpot_paths_device") result(ierr)
    type(c_ptr), value :: handle, dB, dG, dseeds, dends, dlength, dintegral, dstatus, dnsteps, doffsets, total, dpoints, &
                          dbpt, dgpt, dipt
    integer(c_int), value :: nseeds, max_steps, direction, every
    integer(c_int64_t), value :: max_points
    real(c_double), value :: step
    integer(c_int) :: ierr
    ierr = vecpot_handle_paths(handle, dB, dG, nseeds, dseeds, step, max_steps, direction, every, max_points, dends, &
                               dlength, dintegral, dstatus, dnsteps, doffsets, total, dpoints, dbpt, dgpt, dipt, &
                               .true., "ndsm_hip_vecpot_paths_device")
  end function

  function vecpot_handle_paths(handle, B, G, nseeds, seeds, step, max_steps, direction, every, max_points, ends, &
                               length, integral, status, nsteps, offsets, total, points, bpt, gpt, ipt, on_device, &
                               who) result(ierr)
    type(c_ptr), intent(in) :: handle, B, G, seeds, ends, length, integral, status, nsteps, offsets, total, points, bpt, &
                               gpt, ipt
    integer(c_int), intent(in) :: nseeds, max_steps, direction, every
    integer(c_int64_t), intent(in) :: max_points
    real(c_double), intent(in) :: step
    logical, intent(in) :: on_device
    character(len=*), intent(in) :: who
    integer(c_int) :: ierr
    ierr = checked()
    if (ierr /= 0) call clear_outputs()
  contains
    function checked() result(rc)
      integer(c_int) :: rc
      type(vecpot_ctx), pointer :: ctx
      integer(c_int64_t), pointer :: tot
      rc = live_ctx(handle, ctx)
      if (rc /= 0) return
      rc = NDSMK_EARG
      if (.not. c_associated(total)) return
      call c_f_pointer(total, tot)
      tot = 0
      ! no seeds: no array is looked at; the scalars are the kernel layer's to judge (9004) once the arrays are there
      if (nseeds > 0) then
        if (.not. (c_associated(B) .and. c_associated(seeds) .and. c_associated(ends) .and. c_associated(length) .and. &
                   c_associated(integral) .and. c_associated(status) .and. c_associated(nsteps) .and. &
                   c_associated(offsets))) return
        if (max_points > 0 .and. .not. c_associated(points)) return
      end if
      rc = reported(who, vecpot_paths(ctx, B, G, direction, nseeds, seeds, step, max_steps, every, max_points, ends, &
                                      length, integral, status, nsteps, offsets, tot, points, bpt, gpt, ipt, on_device))
    end function

    ! total, and (host entry) the nl entries of the trace outputs, the nl + 1 of offsets and the max_points slots of
    ! every point array that is there
    subroutine clear_outputs()
      integer(c_int64_t) :: nl, np
      call clear_host([total], [8], [1_c_int64_t])
      if (on_device) return
      ! (no lines: no line array is touched)
      if (nseeds > 0 .and. nseeds <= huge(0) / 6) then
        nl = int(nseeds, c_int64_t) * merge(2, 1, direction == 0)
        call clear_host([ends, length, integral, status, nsteps, offsets], [24, 8, 8, 4, 4, 8], &
                        [nl, nl, nl, nl, nl, nl + 1])
      end if
      ! (no capacity: no point array is touched)
      if (max_points <= 0 .or. max_points > huge(0_c_int64_t) / 3) return
      np = max_points
      call clear_host([points, bpt, gpt, ipt], [24, 24, 24, 8], [np, np, np, np])
    end subroutine
  end function

  ! ---- spine-fan skeleton of the nulls on the same handle --------------------
  ! B (nx,ny,nz,3), pos (3,nnulls) and jac (9 each) - the nulls entries' records -, ring (2,nring), radius, capture,
  ! step, max_steps, every, max_points in.  Out per null: kind (int32), eig, spine, normal (3 each); per line (nl =
  ! nnulls (2 + nring)): ends (3 each), length, status, nsteps, hit (int32); offsets (nl + 1, int64), total (one int64,
  ! on the HOST in both entries), points (3,max_points), bpt (the same; may be NULL).  Return value: 0, or >= 9001
  ! errors (9002 a NULL handle or total, with nnulls > 0 a NULL required array, with nring > 0 a NULL ring, with
  ! max_points > 0 a NULL points; 9004 a scalar out of range).  On every failure total is cleared, and the host entry
  ! clears the nnulls and nl entries of its outputs, the nl + 1 of offsets and the max_points slots of its point arrays.

  ! HOST arrays
  function ndsm_hip_vecpot_skeleton(handle, B, nnulls, pos, jac, nring, ring, radius, capture, step, max_steps, every, &
                                    max_points, kind, eig, spine, normal, ends, length, status, nsteps, hit, offsets, &
                                    total, points, bpt) bind(c, name="ndsm_hip_vecpot_skeleton") result(ierr)
    type(c_ptr), value :: handle, B, pos, jac, ring, kind, eig, spine, normal, ends, length, status, nsteps, hit, &
                          offsets, total, points, bpt
    integer(c_int), value :: nnulls, nring, max_steps, every
    integer(c_int64_t), value :: max_points
    real(c_double), value :: radius, capture, step
    integer(c_int) :: ierr
    ierr = vecpot_handle_skeleton(handle, B, nnulls, pos, jac, nring, ring, radius, capture, step, max_steps, every, &
                                  max_points, kind, eig, spine, normal, ends, length, status, nsteps, hit, offsets, &
                                  total, points, bpt, .false., "ndsm_hip_vecpot_skeleton")
  end function

  ! the same on DEVICE arrays of the library's GPU (total stays on the host; no array is touched on the host)
  function ndsm_hip_vecpot_skeleton_device(handle, dB, nnulls, dpos, djac, nring, dring, radius, capture, step, &
                                           max_steps, every, max_points, dkind, deig, dspine, dnormal, dends, dlength, &
                                           dstatus, dnsteps, dhit, doffsets, total, dpoints, dbpt) &
      bind(c, name="ndsm_hip_vecpot_skeleton_device") result(ierr)
    type(c_ptr), value :: handle, dB, dpos, djac, dring, dkind, deig, dspine, dnormal, dends, dlength, dstatus, dnsteps, &
                          dhit, doffsets, total, dpoints, dbpt
    integer(c_int), value :: nnulls, nring, max_steps, every
    integer(c_int64_t), value :: max_points
    real(c_double), value :: radius, capture, step
    integer(c_int) :: ierr
    ierr = vecpot_handle_skeleton(handle, dB, nnulls, dpos, djac, nring, dring, radius, capture, step, max_steps, every, &
                                  max_points, dkind, deig, dspine, dnormal, dends, dlength, dstatus, dnsteps, dhit, &
                                  doffsets, total, dpoints, dbpt, .true., "ndsm_hip_vecpot_skeleton_device")
  end function

  function vecpot_handle_skeleton(handle, B, nnulls, pos, jac, nring, ring, radius, capture, step, max_steps, every, &
                                  max_points, kind, eig, spine, normal, ends, length, status, nsteps, hit, offsets, &
                                  total, points, bpt, on_device, who) result(ierr)
    type(c_ptr), intent(in) :: handle, B, pos, jac, ring, kind, eig, spine, normal, ends, length, status, nsteps, hit, &
                               offsets, total, points, bpt
    integer(c_int), intent(in) :: nnulls, nring, max_steps, every
    integer(c_int64_t), intent(in) :: max_points
    real(c_double), intent(in) :: radius, capture, step
    logical, intent(in) :: on_device
    character(len=*), intent(in) :: who
    integer(c_int) :: ierr
    ierr = checked()
    if (ierr /= 0) call clear_outputs()
  contains
    function checked() result(rc)
      integer(c_int) :: rc
      type(vecpot_ctx), pointer :: ctx
      integer(c_int64_t), pointer :: tot
      rc = live_ctx(handle, ctx)
      if (rc /= 0) return
      rc = NDSMK_EARG
      if (.not. c_associated(total)) return
      call c_f_pointer(total, tot)
      tot = 0
      ! no nulls: no array is looked at; the scalars are the kernel layer's to judge (9004) once the arrays are there
      if (nnulls > 0) then
        if (.not. (c_associated(B) .and. c_associated(pos) .and. c_associated(jac) .and. c_associated(kind) .and. &
                   c_associated(eig) .and. c_associated(spine) .and. c_associated(normal) .and. c_associated(ends) .and. &
                   c_associated(length) .and. c_associated(status) .and. c_associated(nsteps) .and. &
                   c_associated(hit) .and. c_associated(offsets))) return
        if (nring > 0 .and. .not. c_associated(ring)) return
        if (max_points > 0 .and. .not. c_associated(points)) return
      end if
      rc = reported(who, vecpot_skeleton(ctx, B, nnulls, pos, jac, nring, ring, radius, capture, step, max_steps, every, &
                                         max_points, kind, eig, spine, normal, ends, length, status, nsteps, hit, &
                                         offsets, tot, points, bpt, on_device))
    end function

    ! total, and (host entry) the nnulls entries of the per-null outputs, the nl entries of the per-line outputs, the
    ! nl + 1 of offsets and the max_points slots of every point array that is there
    subroutine clear_outputs()
      integer(c_int64_t) :: nm, nl, np
      call clear_host([total], [8], [1_c_int64_t])
      if (on_device) return
      nl = 0
      if (nnulls > 0 .and. nring >= 0) nl = int(nnulls, c_int64_t) * (2_c_int64_t + int(nring, c_int64_t))
      ! (no lines: no line array is touched)
      if (nl > 0 .and. nl <= huge(0) / 3) then
        nm = nnulls
        call clear_host([kind, eig, spine, normal, ends, length, status, nsteps, hit, offsets], &
                        [4, 24, 24, 24, 24, 8, 4, 4, 4, 8], [nm, nm, nm, nm, nl, nl, nl, nl, nl, nl + 1])
      end if
      ! (no capacity: no point array is touched)
      if (max_points <= 0 .or. max_points > huge(0_c_int64_t) / 3) return
      np = max_points
      call clear_host([points, bpt], [24, 24], [np, np])
    end subroutine
  end function

  ! ---- separator lines on the same handle ------------------------------------
  ! B (nx,ny,nz,3), pos (3,nnulls), kind (nnulls; int32), normal (3,nnulls) - the skeleton entries' arrays of the nulls -,
  ! pair (2,nbr; int32), arc (4,nbr), radius, capture, step, max_steps, rounds, tol, every, max_points in.  Out per
  ! bracket: state, nrounds (int32), coef (4 each), width, side (int32), dmin (2 each), ends (3 each), length, status,
  ! nsteps (int32); offsets (nbr + 1, int64), total (one int64, on the HOST in both entries), points (3,max_points), bpt
  ! (the same; may be NULL).  Return value: 0, or >= 9001 errors (9002 a NULL handle or total, with nbr > 0 a NULL
  ! required array, with max_points > 0 a NULL points; 9004 a scalar out of range or a pair index outside 0 .. nnulls - 1).
  ! On every failure total is cleared, and the host entry clears the nbr entries of its outputs, the nbr + 1 of offsets
  ! and the max_points slots of its point arrays.

  ! HOST arrays
  function ndsm_hip_vecpot_separators(handle, B, nnulls, pos, kind, normal, nbr, pair, arc, radius, capture, step, &
                                      max_steps, rounds, tol, every, max_points, state, nrounds, coef, width, side, &
                                      dmin, ends, length, status, nsteps, offsets, total, points, bpt) &
      bind(c, name="ndsm_hip_vecpot_separators") result(ierr)
    type(c_ptr), value :: handle, B, pos, kind, normal, pair, arc, state, nrounds, coef, width, side, dmin, ends, length, &
                          status, nsteps, offsets, total, points, bpt
    integer(c_int), value :: nnulls, nbr, max_steps, rounds, every
    integer(c_int64_t), value :: max_points
    real(c_double), value :: radius, capture, step, tol
    integer(c_int) :: ierr
    ierr = vecpot_handle_separators(handle, B, nnulls, pos, kind, normal, nbr, pair, arc, radius, capture, step, &
                                    max_steps, rounds, tol, every, max_points, state, nrounds, coef, width, side, dmin, &
                                    ends, length, status, nsteps, offsets, total, points, bpt, .false., &
                                    "ndsm_hip_vecpot_separators")
  end function

  ! the same on DEVICE arrays of the library's GPU (total stays on the host; no array is touched on the host)
  function ndsm_hip_vecpot_separators_device(handle, dB, nnulls, dpos, dkind, dnormal, nbr, dpair, darc, radius, capture, &
                                             step, max_steps, rounds, tol, every, max_points, dstate, dnrounds, dcoef, &
                                             dwidth, dside, ddmin, dends, dlength, dstatus, dnsteps, doffsets, total, &
                                             dpoints, dbpt) bind(c, name="ndsm_hip_vecpot_separators_device") result(ierr)
    type(c_ptr), value :: handle, dB, dpos, dkind, dnormal, dpair, darc, dstate, dnrounds, dcoef, dwidth, dside, ddmin, &
                          dends, dlength, dstatus, dnsteps, doffsets, total, dpoints, dbpt
    integer(c_int), value :: nnulls, nbr, max_steps, rounds, every
    integer(c_int64_t), value :: max_points
    real(c_double), value :: radius, capture, step, tol
    integer(c_int) :: ierr
    ierr = vecpot_handle_separators(handle, dB, nnulls, dpos, dkind, dnormal, nbr, dpair, darc, radius, capture, step, &
                                    max_steps, rounds, tol, every, max_points, dstate, dnrounds, dcoef, dwidth, dside, &
                                    ddmin, dends, dlength, dstatus, dnsteps, doffsets, total, dpoints, dbpt, .true., &
                                    "ndsm_hip_vecpot_separators_device")
  end function

  function vecpot_handle_separators(handle, B, nnulls, pos, kind, normal, nbr, pair, arc, radius, capture, step, &
                                    max_steps, rounds, tol, every, max_points, state, nrounds, coef, width, side, dmin, &
                                    ends, length, status, nsteps, offsets, total, points, bpt, on_device, who) &
      result(ierr)
    type(c_ptr), intent(in) :: handle, B, pos, kind, normal, pair, arc, state, nrounds, coef, width, side, dmin, ends, &
                               length, status, nsteps, offsets, total, points, bpt
    integer(c_int), intent(in) :: nnulls, nbr, max_steps, rounds, every
    integer(c_int64_t), intent(in) :: max_points
    real(c_double), intent(in) :: radius, capture, step, tol
    logical, intent(in) :: on_device
    character(len=*), intent(in) :: who
    integer(c_int) :: ierr
    ierr = checked()
    if (ierr /= 0) call clear_outputs()
  contains
    function checked() result(rc)
      integer(c_int) :: rc
      type(vecpot_ctx), pointer :: ctx
      integer(c_int64_t), pointer :: tot
      rc = live_ctx(handle, ctx)
      if (rc /= 0) return
      rc = NDSMK_EARG
      if (.not. c_associated(total)) return
      call c_f_pointer(total, tot)
      tot = 0
      ! no brackets: no array is looked at; the scalars are the kernel layer's to judge (9004) once the arrays are there
      if (nbr > 0) then
        if (.not. (c_associated(B) .and. c_associated(pos) .and. c_associated(kind) .and. c_associated(normal) .and. &
                   c_associated(pair) .and. c_associated(arc) .and. c_associated(state) .and. &
                   c_associated(nrounds) .and. c_associated(coef) .and. c_associated(width) .and. &
                   c_associated(side) .and. c_associated(dmin) .and. c_associated(ends) .and. c_associated(length) .and. &
                   c_associated(status) .and. c_associated(nsteps) .and. c_associated(offsets))) return
        if (max_points > 0 .and. .not. c_associated(points)) return
      end if
      rc = reported(who, vecpot_separators(ctx, B, nnulls, pos, kind, normal, nbr, pair, arc, radius, capture, step, &
                                           max_steps, rounds, tol, every, max_points, state, nrounds, coef, width, side, &
                                           dmin, ends, length, status, nsteps, offsets, tot, points, bpt, on_device))
    end function

    ! total, and (host entry) the nbr entries of the per-bracket outputs, the nbr + 1 of offsets and the max_points
    ! slots of every point array that is there
    subroutine clear_outputs()
      integer(c_int64_t) :: nq, np
      call clear_host([total], [8], [1_c_int64_t])
      if (on_device) return
      ! (no lines: no line array is touched)
      if (nbr > 0 .and. nbr <= huge(0) / 4) then
        nq = nbr
        call clear_host([state, nrounds, coef, width, side, dmin, ends, length, status, nsteps, offsets], &
                        [4, 4, 32, 8, 4, 16, 24, 8, 4, 4, 8], [nq, nq, nq, nq, nq, nq, nq, nq, nq, nq, nq + 1])
      end if
      ! (no capacity: no point array is touched)
      if (max_points <= 0 .or. max_points > huge(0_c_int64_t) / 3) return
      np = max_points
      call clear_host([points, bpt], [24, 24], [np, np])
    end subroutine
  end function

  ! ---- null points on the same handle --------------------------------------
  ! B (nx,ny,nz,3) in; max_nulls >= 0 the capacity of the record arrays; counts (2, int64, on the HOST in both
  ! entries): the screen's candidates, the nulls found.  Out, the first min(counts(2), max_nulls) records in ascending
  ! cell order: cell (int64), pos (3 each), jac (9 each), det, resid (doubles), sign, iters (int32).  The handle
  ! supplies the mesh; no solve runs.  Return value: 0, or >= 9001 errors (9002 a NULL handle, B or counts, or with
  ! max_nulls > 0 a NULL record array; 9004 max_nulls < 0).  On every failure counts is cleared, and the host entry
  ! clears the max_nulls slots of its record arrays.

  ! HOST arrays
  function ndsm_hip_vecpot_nulls(handle, B, max_nulls, counts, cell, pos, jac, det, resid, sign, iters) &
      bind(c, name="ndsm_hip_vecpot_nulls") result(ierr)
    type(c_ptr), value :: handle, B, counts, cell, pos, jac, det, resid, sign, iters
    integer(c_int), value :: max_nulls
    integer(c_int) :: ierr
    ierr = vecpot_handle_nulls(handle, B, max_nulls, counts, cell, pos, jac, det, resid, sign, iters, .false., &
                               "ndsm_hip_vecpot_nulls")
  end function

  ! the same on DEVICE arrays of the library's GPU (counts stays a host array; no record array is touched on the host)
  function ndsm_hip_vecpot_nulls_device(handle, dB, max_nulls, counts, dcell, dpos, djac, ddet, dresid, dsign, diters) &
      bind(c, name="ndsm_hip_vecpot_nulls_device") result(ierr)
    type(c_ptr), value :: handle, dB, counts, dcell, dpos, djac, ddet, dresid, dsign, diters
    integer(c_int), value :: max_nulls
    integer(c_int) :: ierr
    ierr = vecpot_handle_nulls(handle, dB, max_nulls, counts, dcell, dpos, djac, ddet, dresid, dsign, diters, .true., &
                               "ndsm_hip_vecpot_nulls_device")
  end function

  function vecpot_handle_nulls(handle, B, max_nulls, counts, cell, pos, jac, det, resid, sign, iters, on_device, who) &
      result(ierr)
    type(c_ptr), intent(in) :: handle, B, counts, cell, pos, jac, det, resid, sign, iters
    integer(c_int), intent(in) :: max_nulls
    logical, intent(in) :: on_device
    character(len=*), intent(in) :: who
    integer(c_int) :: ierr
    type(vecpot_ctx), pointer :: ctx
    integer(c_int64_t), pointer :: cnt(:)
    call clear_outputs()
    ierr = live_ctx(handle, ctx)
    if (ierr /= 0) return
    ierr = NDSMK_EARG
    if (.not. (c_associated(B) .and. c_associated(counts))) return
    if (max_nulls > 0 .and. .not. (c_associated(cell) .and. c_associated(pos) .and. c_associated(jac) .and. &
                                   c_associated(det) .and. c_associated(resid) .and. c_associated(sign) .and. &
                                   c_associated(iters))) return
    call c_f_pointer(counts, cnt, [2])
    ierr = reported(who, vecpot_nulls(ctx, B, max_nulls, cnt, cell, pos, jac, det, resid, sign, iters, on_device))
    if (ierr /= 0) call clear_outputs()
  contains
    ! counts, and (host entry) the max_nulls slots of every record array
    subroutine clear_outputs()
      integer(c_int64_t) :: nm
      call clear_host([counts], [8], [2_c_int64_t])
      if (on_device .or. max_nulls <= 0) return
      if (max_nulls > huge(0) / 9) return
      nm = max_nulls
      call clear_host([cell, pos, jac, det, resid, sign, iters], [8, 24, 72, 8, 8, 4, 4], [nm, nm, nm, nm, nm, nm, nm])
    end subroutine
  end function

  ! ---- dips and bald patches on the same handle ------------------------------
  ! B (nx,ny,nz,3) in; plane_only 0 or 1 (1: the plane k = 0 and its x and y edges alone); max_dips >= 0 the capacity of
  ! the record arrays; counts (3, int64, on the HOST in both entries): crossings, dips, bald patches.  Out, the first
  ! min(counts(2), max_dips) records in ascending edge order: edge (int64), pos, bpt, grad (3 each), curv (doubles),
  ! flag (int32).  The handle supplies the mesh; no solve runs.  Return value: 0, or >= 9001 errors (9002 a NULL handle,
  ! B or counts, or with max_dips > 0 a NULL record array; 9004 max_dips < 0, plane_only not 0 or 1, fewer than 3 nodes
  ! on an axis).  On every failure counts is cleared, and the host entry clears the max_dips slots of its record arrays.

  ! HOST arrays
  function ndsm_hip_vecpot_dips(handle, B, plane_only, max_dips, counts, edge, pos, bpt, grad, curv, flag) &
      bind(c, name="ndsm_hip_vecpot_dips") result(ierr)
    type(c_ptr), value :: handle, B, counts, edge, pos, bpt, grad, curv, flag
    integer(c_int), value :: plane_only
    integer(c_int64_t), value :: max_dips
    integer(c_int) :: ierr
    ierr = vecpot_handle_dips(handle, B, plane_only, max_dips, counts, edge, pos, bpt, grad, curv, flag, .false., &
                              "ndsm_hip_vecpot_dips")
  end function

  ! the same on DEVICE arrays of the library's GPU (counts stays a host array; no record array is touched on the host)
  function ndsm_hip_vecpot_dips_device(handle, dB, plane_only, max_dips, counts, dedge, dpos, dbpt, dgrad, dcurv, dflag) &
      bind(c, name="ndsm_hip_vecpot_dips_device") result(ierr)
    type(c_ptr), value :: handle, dB, counts, dedge, dpos, dbpt, dgrad, dcurv, dflag
    integer(c_int), value :: plane_only
    integer(c_int64_t), value :: max_dips
    integer(c_int) :: ierr
    ierr = vecpot_handle_dips(handle, dB, plane_only, max_dips, counts, dedge, dpos, dbpt, dgrad, dcurv, dflag, .true., &
                              "ndsm_hip_vecpot_dips_device")
  end function

  function vecpot_handle_dips(handle, B, plane_only, max_dips, counts, edge, pos, bpt, grad, curv, flag, on_device, who) &
      result(ierr)
    type(c_ptr), intent(in) :: handle, B, counts, edge, pos, bpt, grad, curv, flag
    integer(c_int), intent(in) :: plane_only
    integer(c_int64_t), intent(in) :: max_dips
    logical, intent(in) :: on_device
    character(len=*), intent(in) :: who
    integer(c_int) :: ierr
    type(vecpot_ctx), pointer :: ctx
    integer(c_int64_t), pointer :: cnt(:)
    call clear_outputs()
    ierr = live_ctx(handle, ctx)
    if (ierr /= 0) return
    ierr = NDSMK_EARG
    if (.not. (c_associated(B) .and. c_associated(counts))) return
    if (max_dips > 0 .and. .not. (c_associated(edge) .and. c_associated(pos) .and. c_associated(bpt) .and. &
                                  c_associated(grad) .and. c_associated(curv) .and. c_associated(flag))) return
    call c_f_pointer(counts, cnt, [3])
    ierr = reported(who, vecpot_dips(ctx, B, plane_only, max_dips, cnt, edge, pos, bpt, grad, curv, flag, on_device))
    if (ierr /= 0) call clear_outputs()
  contains
    ! counts, and (host entry) the max_dips slots of every record array
    subroutine clear_outputs()
      call clear_host([counts], [8], [3_c_int64_t])
      if (on_device .or. max_dips <= 0) return
      if (max_dips > huge(0_c_int64_t) / 24) return
      call clear_host([edge, pos, bpt, grad, curv, flag], [8, 24, 24, 24, 8, 4], &
                      [max_dips, max_dips, max_dips, max_dips, max_dips, max_dips])
    end subroutine
  end function

  ! ---- patch connectivity on the same handle ---------------------------------
  ! B (nx,ny,nz,3) and label (nx,ny; int32) in, K >= 0 the largest label that counts; step, max_steps as the trace
  ! entry's; max_pairs >= 0 the capacity of the pair arrays; counts (2, int64, on the HOST in both entries): lines
  ! traced, distinct pairs.  Out per pixel: dest (int32), ends (3 each), length, status (int32); the first min(counts(2),
  ! max_pairs) pairs in ascending (a, c): pa, pc (int32), nlines (int64), pflux.  The handle supplies the mesh; no solve
  ! runs.  Return value: 0, or >= 9001 errors (9002 a NULL handle, B, label, counts or per-pixel array, or with max_pairs
  ! > 0 a NULL pair array; 9004 K < 0, max_pairs < 0, step not > 0, max_steps < 1).  On every failure counts is cleared,
  ! and the host entry clears its per-pixel arrays and the max_pairs slots of its pair arrays.

  ! HOST arrays
  function ndsm_hip_vecpot_connect(handle, B, label, K, step, max_steps, max_pairs, counts, dest, ends, length, status, &
                                   pa, pc, nlines, pflux) bind(c, name="ndsm_hip_vecpot_connect") result(ierr)
    type(c_ptr), value :: handle, B, label, counts, dest, ends, length, status, pa, pc, nlines, pflux
    integer(c_int), value :: K, max_steps
    real(c_double), value :: step
    integer(c_int64_t), value :: max_pairs
    integer(c_int) :: ierr
    ierr = connect_entry(handle, B, label, K, step, max_steps, max_pairs, counts, [dest, ends, length, status], &
                         [pa, pc, nlines, pflux], .false., "ndsm_hip_vecpot_connect")
  end function

  ! the same on DEVICE arrays of the library's GPU (counts stays a host array; no output is touched on the host)
  function ndsm_hip_vecpot_connect_device(handle, dB, dlabel, K, step, max_steps, max_pairs, counts, ddest, dends, dlength, &
                                          dstatus, dpa, dpc, dnlines, dpflux) &
      bind(c, name="ndsm_hip_vecpot_connect_device") result(ierr)
    type(c_ptr), value :: handle, dB, dlabel, counts, ddest, dends, dlength, dstatus, dpa, dpc, dnlines, dpflux
    integer(c_int), value :: K, max_steps
    real(c_double), value :: step
    integer(c_int64_t), value :: max_pairs
    integer(c_int) :: ierr
    ierr = connect_entry(handle, dB, dlabel, K, step, max_steps, max_pairs, counts, [ddest, dends, dlength, dstatus], &
                         [dpa, dpc, dnlines, dpflux], .true., "ndsm_hip_vecpot_connect_device")
  end function

  function connect_entry(handle, B, label, K, step, max_steps, max_pairs, counts, pix, pair, on_device, who) result(ierr)
    type(c_ptr), intent(in) :: handle, B, label, counts, pix(4), pair(4)
    integer(c_int), intent(in) :: K, max_steps
    real(c_double), intent(in) :: step
    integer(c_int64_t), intent(in) :: max_pairs
    logical, intent(in) :: on_device
    character(len=*), intent(in) :: who
    integer(c_int) :: ierr
    type(vecpot_ctx), pointer :: ctx
    integer(c_int64_t), pointer :: cnt(:)
    integer :: i
    logical :: complete
    call clear_host([counts], [8], [2_c_int64_t])
    ierr = live_ctx(handle, ctx)
    if (ierr /= 0) return
    ierr = NDSMK_EARG
    complete = c_associated(B) .and. c_associated(label) .and. c_associated(counts)
    do i = 1, 4
      complete = complete .and. c_associated(pix(i)) .and. (max_pairs <= 0 .or. c_associated(pair(i)))
    end do
    if (.not. complete) then
      call clear_outputs()
      return
    end if
    call c_f_pointer(counts, cnt, [2])
    ierr = reported(who, vecpot_connect(ctx, B, label, K, step, max_steps, max_pairs, cnt, pix(1), pix(2), pix(3), pix(4), &
                                        pair(1), pair(2), pair(3), pair(4), on_device))
    if (ierr /= 0) call clear_outputs()
  contains
    ! counts, and (host entry) the per-pixel arrays and the max_pairs slots of every pair array
    subroutine clear_outputs()
      integer(c_int64_t) :: np
      call clear_host([counts], [8], [2_c_int64_t])
      if (on_device) return
      np = int(ctx%n3(1), c_int64_t) * int(ctx%n3(2), c_int64_t)
      call clear_host(pix, [4, 24, 8, 4], [np, np, np, np])
      if (max_pairs <= 0 .or. max_pairs > huge(0_c_int64_t) / 8) return
      call clear_host(pair, [4, 4, 8, 8], [max_pairs, max_pairs, max_pairs, max_pairs])
    end subroutine
  end function

  ! ---- z-slab decomposition over GPUs (SURVEY 8e) -----------------------

  ! rank 0 creates the 128-byte RCCL id; the launcher hands it to every rank
  function ndsm_hip_dist_unique_id(id128) bind(c, name="ndsm_hip_dist_unique_id") result(rc)
    type(c_ptr), value :: id128
    integer(c_int) :: rc
    rc = ndsmk_dist_unique_id(id128)
  end function

  function ndsm_hip_dist_init(rank, nranks, id128) bind(c, name="ndsm_hip_dist_init") result(rc)
    integer(c_int), value :: rank, nranks
    type(c_ptr), value :: id128
    integer(c_int) :: rc
    rc = ndsmk_dist_init(rank, nranks, id128)
  end function

  ! drains the library streams and destroys the communicator (collective: every rank calls it)
  function ndsm_hip_dist_finalize() bind(c, name="ndsm_hip_dist_finalize") result(rc)
    integer(c_int) :: rc
    rc = ndsmk_dist_finalize()
  end function

  ! rank and size as the RCCL communicator reports them (ncclCommUserRank / ncclCommCount);
  ! nranks = 0: no communicator is up
  function ndsm_hip_dist_info(rank, nranks) bind(c, name="ndsm_hip_dist_info") result(rc)
    integer(c_int), intent(out) :: rank, nranks
    integer(c_int) :: rc
    rc = ndsmk_dist_info(rank, nranks)
  end function

  ! transport self-test on the live communicator (collective): self send/recv of nelem doubles through
  ! the grouped ncclSend/ncclRecv pair of a halo exchange, on the main and on the communication stream,
  ! and the 2-value all-reduce; 0 = every byte arrived
  function ndsm_hip_dist_selftest(nelem) bind(c, name="ndsm_hip_dist_selftest") result(rc)
    integer(c_int), value :: nelem
    integer(c_int) :: rc
    rc = ndsmk_dist_selftest(nelem)
  end function

  ! The slab plan every rank derives (pure host arithmetic, no GPU needed).
  ! out(12, nranks): rank, z0, z1, g, nloc, k0, ck0, ck1, pk0, pk1, cb0, cb1
  function ndsm_hip_slab_plan(nshape, x, y, z, ngrids, nranks, out) bind(c, name="ndsm_hip_slab_plan") result(rc)
    integer(c_int), intent(in) :: nshape(3)
    integer(c_int), value :: ngrids, nranks
    type(c_ptr), value :: x, y, z
    integer(c_int), intent(out) :: out(12, nranks)
    integer(c_int) :: rc
    real(c_double), pointer :: qx(:), qy(:), qz(:)
    type(slab_t), allocatable :: plan(:)
    integer(c_int32_t) :: n3(3)
    integer :: r
    n3 = nshape
    call c_f_pointer(x, qx, [n3(1)])
    call c_f_pointer(y, qy, [n3(2)])
    call c_f_pointer(z, qz, [n3(3)])
    rc = world_plan_only(n3, qx, qy, qz, int(ngrids), int(nranks), plan)
    if (rc /= 0) return
    do r = 0, nranks - 1
      out(:, r + 1) = [plan(r)%rank, plan(r)%z0, plan(r)%z1, plan(r)%g, plan(r)%nloc, plan(r)%k0, plan(r)%ck0, &
                       plan(r)%ck1, plan(r)%pk0, plan(r)%pk1, plan(r)%cb0, plan(r)%cb1]
    end do
  end function

  ! rank >= 0: this process holds slab `rank` (RCCL transport, after ndsm_hip_dist_init);
  ! rank < 0 : loop-back world, all nranks slabs on this GPU (verification)
  function ndsm_hip_world_create(nshape, x, y, z, bcs, ngrids, ms, ex_tol, du_max, nmax_exact, nranks, rank, handle) &
      bind(c, name="ndsm_hip_world_create") result(rc)
    integer(c_int), intent(in) :: nshape(3)
    integer(c_int), value :: ngrids, ms, du_max, nmax_exact, nranks, rank
    real(c_double), value :: ex_tol
    type(c_ptr), value :: x, y, z
    character(kind=c_char), intent(in) :: bcs(6)
    type(c_ptr), intent(out) :: handle
    integer(c_int) :: rc
    type(mg_world), pointer :: w
    real(c_double), pointer :: qx(:), qy(:), qz(:)
    integer(c_int32_t) :: n3(3)
    character(len=1) :: bc(6)
    integer :: d, i
    handle = c_null_ptr
    rc = NDSMK_EARG
    if (ms < 0 .or. nmax_exact < 0) return       ! (as ndsm_hip_mg_create)
    n3 = nshape
    call c_f_pointer(x, qx, [n3(1)])
    call c_f_pointer(y, qy, [n3(2)])
    call c_f_pointer(z, qz, [n3(3)])
    do d = 1, 6
      bc(d) = bcs(d)
    end do
    rc = ndsmk_init(-1_c_int)
    if (rc /= 0) return
    allocate (w)
    rc = world_create(w, n3, qx, qy, qz, bc, int(ngrids), int(nranks), int(rank))
    if (rc /= 0) then
      call world_destroy(w)
      deallocate (w)
      return
    end if
    call world_set_params(w, int(ms), ex_tol, du_max == 1, int(nmax_exact))
    handle = c_loc(w)
  end function

  function ndsm_hip_world_destroy(handle) bind(c, name="ndsm_hip_world_destroy") result(rc)
    type(c_ptr), value :: handle
    integer(c_int) :: rc
    type(mg_world), pointer :: w
    rc = 0
    if (.not. c_associated(handle)) return
    call c_f_pointer(handle, w)
    call world_destroy(w)
    deallocate (w)
  end function

  function ndsm_hip_world_dist_levels(handle) bind(c, name="ndsm_hip_world_dist_levels") result(n)
    type(c_ptr), value :: handle
    integer(c_int) :: n
    type(mg_world), pointer :: w
    call c_f_pointer(handle, w)
    n = world_dist_levels(w)
  end function

  function ndsm_hip_world_nlocal(handle) bind(c, name="ndsm_hip_world_nlocal") result(n)
    type(c_ptr), value :: handle
    integer(c_int) :: n
    type(mg_world), pointer :: w
    call c_f_pointer(handle, w)
    n = w%nlocal
  end function

  ! info(12) of local slab ilocal (1-based): same fields as ndsm_hip_slab_plan
  function ndsm_hip_world_slab(handle, ilocal, info) bind(c, name="ndsm_hip_world_slab") result(rc)
    type(c_ptr), value :: handle
    integer(c_int), value :: ilocal
    integer(c_int), intent(out) :: info(12)
    integer(c_int) :: rc
    type(mg_world), pointer :: w
    call c_f_pointer(handle, w)
    rc = NDSMK_EARG
    if (ilocal < 1 .or. ilocal > w%nlocal) return
    associate (p => w%loc(ilocal)%sl)
      info = [p%rank, p%z0, p%z1, p%g, p%nloc, p%k0, p%ck0, p%ck1, p%pk0, p%pk1, p%cb0, p%cb1]
    end associate
    rc = 0
  end function

  ! host points at global plane gz0 of an (nx,ny,*) array holding nplanes planes
  function ndsm_hip_world_upload(handle, ilocal, which, host, gz0, nplanes) bind(c, name="ndsm_hip_world_upload") &
      result(rc)
    type(c_ptr), value :: handle, host
    integer(c_int), value :: ilocal, which, gz0, nplanes
    integer(c_int) :: rc
    type(mg_world), pointer :: w
    call c_f_pointer(handle, w)
    rc = world_upload(w, int(ilocal), int(which), host, int(gz0), int(nplanes))
  end function

  ! host receives the slab's owned planes [z0, z1)
  function ndsm_hip_world_download(handle, ilocal, which, host) bind(c, name="ndsm_hip_world_download") result(rc)
    type(c_ptr), value :: handle, host
    integer(c_int), value :: ilocal, which
    integer(c_int) :: rc
    type(mg_world), pointer :: w
    call c_f_pointer(handle, w)
    rc = world_download(w, int(ilocal), int(which), host)
  end function

  function ndsm_hip_world_relax(handle, nsweeps) bind(c, name="ndsm_hip_world_relax") result(rc)
    type(c_ptr), value :: handle
    integer(c_int), value :: nsweeps
    integer(c_int) :: rc
    type(mg_world), pointer :: w
    call c_f_pointer(handle, w)
    rc = world_relax(w, int(nsweeps))
  end function

  ! mode as ndsm_hip_mg_set_precision (0 fp64; /= 0 mixed: fp64 residual, fp32 correction V-cycle on the
  ! level-1 slabs).  Returns 1 if world_solve will run mixed, 0 if the fp64 path stays (a slab out of the
  ! fp32 kernels' reach: odd nx, < 64 x 16 points per plane), < 0 on a bad handle.
  function ndsm_hip_world_set_precision(handle, mode) bind(c, name="ndsm_hip_world_set_precision") result(on)
    type(c_ptr), value :: handle
    integer(c_int), value :: mode
    integer(c_int) :: on
    type(mg_world), pointer :: w
    on = -1
    if (.not. c_associated(handle) .or. mode < 0 .or. mode > 2) return
    call c_f_pointer(handle, w)
    on = merge(1_c_int, 0_c_int, world_set_precision(w, int(mode)))
  end function

  function ndsm_hip_world_zero_rhs(handle) bind(c, name="ndsm_hip_world_zero_rhs") result(rc)
    type(c_ptr), value :: handle
    integer(c_int) :: rc
    type(mg_world), pointer :: w
    integer :: i
    call c_f_pointer(handle, w)
    rc = 0
    do i = 1, w%nlocal
      rc = mg_zero_rhs(w%loc(i)); if (rc /= 0) return
    end do
  end function

  function ndsm_hip_bound_libs(buf, len) bind(c, name="ndsm_hip_bound_libs") result(rc)
    type(c_ptr), value :: buf
    integer(c_int), value :: len
    integer(c_int) :: rc
    interface
      function ndsmk_bound_libs(buf, len) bind(c, name="ndsmk_bound_libs") result(rc)
        import :: c_ptr, c_int
        type(c_ptr), value :: buf
        integer(c_int), value :: len
        integer(c_int) :: rc
      end function
    end interface
    rc = ndsmk_bound_libs(buf, len)
  end function

  ! development hook (tests, tuning): tile configuration of the fused smoother, the five values of
  ! NDSM_FUSED_CFG (smooth_fused.hip) - big = 1 runs the tiles of >= 64 M-point levels on any level
  function ndsm_hip_debug_fused_cfg(two, one, res, work_items, big) bind(c, name="ndsm_hip_debug_fused_cfg") result(rc)
    integer(c_int), value :: two, one, res, work_items, big
    integer(c_int) :: rc
    interface
      function ndsmk_debug_fused_cfg(two, one, res, work_items, big) bind(c, name="ndsmk_debug_fused_cfg") result(rc)
        import :: c_int
        integer(c_int), value :: two, one, res, work_items, big
        integer(c_int) :: rc
      end function
    end interface
    rc = ndsmk_debug_fused_cfg(two, one, res, work_items, big)
  end function

  ! development hook (tests, tools): the plan of a relax call (what = 0) or the z chunking of a fused launch
  ! (what = 1) as csrc/relax_plan.hpp decides them - host code, no device and no ndsm_hip_init needed
  function ndsm_hip_debug_relax_plan(what, grid, req, knobs, cap, out) bind(c, name="ndsm_hip_debug_relax_plan") result(rc)
    integer(c_int), value :: what, cap
    type(c_ptr), value :: grid, req, knobs, out
    integer(c_int) :: rc
    rc = ndsmk_debug_relax_plan(what, grid, req, knobs, cap, out)
  end function

  ! development hook: 0 = the levels of the V-cycle's tail run kernel by kernel even where the single-launch
  ! form (tail.hip) covers them, 1 = default
  function ndsm_hip_debug_tail(on) bind(c, name="ndsm_hip_debug_tail") result(rc)
    integer(c_int), value :: on
    integer(c_int) :: rc
    rc = ndsmk_debug_tail(on)
  end function

  ! development hook (tests): the level sizes from which the streamed restriction / the tiled prolongation run, the
  ! streamed restriction's form and its chunk length (transfer.hip, restrict_stream.hip); negative = built in
  function ndsm_hip_debug_transfer_cfg(restrict_min_points, prolong_min_points, rs_variant, rs_chunk) &
      bind(c, name="ndsm_hip_debug_transfer_cfg") result(rc)
    integer(c_long_long), value :: restrict_min_points, prolong_min_points
    integer(c_int), value :: rs_variant, rs_chunk
    integer(c_int) :: rc
    rc = ndsmk_debug_transfer_cfg(restrict_min_points, prolong_min_points, rs_variant, rs_chunk)
  end function

  ! development hook (tests): the kernels the transfers level -> level + 1 of an ndsm_hip_mg_create handle take
  function ndsm_hip_debug_transfer_form(handle, level, out) bind(c, name="ndsm_hip_debug_transfer_form") result(rc)
    type(c_ptr), value :: handle
    integer(c_int), value :: level
    integer(c_int), intent(out) :: out(4)
    integer(c_int) :: rc
    type(mg_solver), pointer :: s
    rc = NDSMK_EARG
    if (.not. c_associated(handle)) return
    call c_f_pointer(handle, s)
    rc = mg_transfer_form(s, int(level), out)
  end function

  function ndsm_hip_debug_zero_guess(on) bind(c, name="ndsm_hip_debug_zero_guess") result(rc)
    integer(c_int), value :: on
    integer(c_int) :: rc
    rc = ndsmk_debug_zero_guess(on)
  end function

  function ndsm_hip_debug_u_declared_zero(handle, level) bind(c, name="ndsm_hip_debug_u_declared_zero") result(yes)
    type(c_ptr), value :: handle
    integer(c_int), value :: level
    integer(c_int) :: yes
    type(mg_solver), pointer :: s
    call c_f_pointer(handle, s)
    yes = merge(1_c_int, 0_c_int, mg_u_declared_zero(s, int(level)))
  end function

  function ndsm_hip_world_vcycle(handle, ncycles) bind(c, name="ndsm_hip_world_vcycle") result(rc)
    type(c_ptr), value :: handle
    integer(c_int), value :: ncycles
    integer(c_int) :: rc
    type(mg_world), pointer :: w
    integer :: i
    call c_f_pointer(handle, w)
    rc = 0
    do i = 1, ncycles
      rc = world_vcycle(w)
      if (rc /= 0) return
    end do
  end function

  function ndsm_hip_world_solve(handle, vc_tol, nmax, du_last, ncycles, hist, hist_len) &
      bind(c, name="ndsm_hip_world_solve") result(ierr)
    type(c_ptr), value :: handle, hist
    real(c_double), value :: vc_tol
    integer(c_int), value :: nmax, hist_len
    real(c_double), intent(out) :: du_last
    integer(c_int), intent(out) :: ncycles
    integer(c_int) :: ierr
    type(mg_world), pointer :: w
    real(c_double), pointer :: hh(:)
    integer :: nc, ie
    integer(c_int) :: rc
    call c_f_pointer(handle, w)
    if (c_associated(hist) .and. hist_len > 0) then
      call c_f_pointer(hist, hh, [hist_len])
      rc = world_solve(w, vc_tol, int(nmax), du_last, nc, ie, hh)
    else
      rc = world_solve(w, vc_tol, int(nmax), du_last, nc, ie)
    end if
    ncycles = nc
    ierr = merge(rc, int(ie, c_int), rc /= 0)
  end function

end module ndsmh_cabi
