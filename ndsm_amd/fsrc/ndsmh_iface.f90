! libndsm_hip - ISO_C_BINDING shim between the Fortran 2003 host driver and the
! hand-written HIP kernels (ndsm_amd/csrc/ndsm_kernels.h).  Every interface
! below is a 1:1 image of a C prototype in that header; the two BIND(C) types
! mirror the C structs member for member.
!
! Kinds follow the reference's conventions (ndsm_root.f90:56-61): reals are
! C doubles, sizes and counters are 64-bit.
module ndsmh_iface

  use, intrinsic :: iso_c_binding
  implicit none
  public

  integer, parameter :: wp = c_double
  integer, parameter :: ik = c_int64_t

  ! error codes shared with ndsm_kernels.h
  integer(c_int), parameter :: NDSMK_OK = 0, NDSMK_ENODEV = 9001, NDSMK_EARG = 9002, NDSMK_ENCCL = 9003
  integer(c_int), parameter :: NDSMK_EVALUE = 9004

  type, bind(c) :: ndsmk_grid
    integer(c_int32_t) :: ndim = 3
    integer(c_int32_t) :: n(3) = 1
    integer(c_int32_t) :: lb(3) = 0, ub(3) = 0
    integer(c_int32_t) :: first_par = 0
    integer(c_int32_t) :: all_neumann = 0
    integer(c_int32_t) :: k0 = 0
    integer(c_int32_t) :: nzg = 1
    integer(c_int32_t) :: zown0 = 0, zown1 = 1
    real(c_double) :: w(3) = 0
    real(c_double) :: w1 = 0
    real(c_double) :: wc = 0
  end type

  type, bind(c) :: ndsmk_xfer
    integer(c_int32_t) :: nf(3) = 1, nc(3) = 1, maxt(3) = 1
    type(c_ptr) :: plo(3), pwl(3), pwh(3)
    type(c_ptr) :: rlo(3), rcnt(3), rw(3)
    real(c_double) :: w2(3) = 0
    integer(c_int32_t) :: f_k0 = 0, f_beg = 0, f_cnt = 1
    integer(c_int32_t) :: c_k0 = 0, c_beg = 0, c_cnt = 1
    integer(c_int32_t) :: stream_ok = 0
  end type

  interface

    function ndsmk_device_count() bind(c, name="ndsmk_device_count") result(n)
      import :: c_int
      integer(c_int) :: n
    end function

    function ndsmk_init(device) bind(c, name="ndsmk_init") result(rc)
      import :: c_int
      integer(c_int), value :: device
      integer(c_int) :: rc
    end function

    function ndsmk_last_error() bind(c, name="ndsmk_last_error") result(p)
      import :: c_ptr
      type(c_ptr) :: p
    end function

    function ndsmk_alloc(p, bytes) bind(c, name="ndsmk_alloc") result(rc)
      import :: c_ptr, c_size_t, c_int
      type(c_ptr), intent(out) :: p
      integer(c_size_t), value :: bytes
      integer(c_int) :: rc
    end function

    function ndsmk_free(p) bind(c, name="ndsmk_free") result(rc)
      import :: c_ptr, c_int
      type(c_ptr), value :: p
      integer(c_int) :: rc
    end function

    function ndsmk_h2d(dst, src, bytes) bind(c, name="ndsmk_h2d") result(rc)
      import :: c_ptr, c_size_t, c_int
      type(c_ptr), value :: dst, src
      integer(c_size_t), value :: bytes
      integer(c_int) :: rc
    end function

    function ndsmk_d2h(dst, src, bytes) bind(c, name="ndsmk_d2h") result(rc)
      import :: c_ptr, c_size_t, c_int
      type(c_ptr), value :: dst, src
      integer(c_size_t), value :: bytes
      integer(c_int) :: rc
    end function

    function ndsmk_halo_packed_plane(nx, ny) bind(c, name="ndsmk_halo_packed_plane") result(n)
      import :: c_int, c_long_long
      integer(c_int), value :: nx, ny
      integer(c_long_long) :: n
    end function
    function ndsmk_halo_pack(src, buf, nx, ny, depth, kg0, first_par) bind(c, name="ndsmk_halo_pack") result(rc)
      import :: c_ptr, c_int
      type(c_ptr), value :: src, buf
      integer(c_int), value :: nx, ny, depth, kg0, first_par
      integer(c_int) :: rc
    end function
    function ndsmk_halo_unpack(dst, buf, nx, ny, depth, kg0, first_par) bind(c, name="ndsmk_halo_unpack") result(rc)
      import :: c_ptr, c_int
      type(c_ptr), value :: dst, buf
      integer(c_int), value :: nx, ny, depth, kg0, first_par
      integer(c_int) :: rc
    end function
    function ndsmk_halo_copy(dst, src, nx, ny, depth, kg0, first_par) bind(c, name="ndsmk_halo_copy") result(rc)
      import :: c_ptr, c_int
      type(c_ptr), value :: dst, src
      integer(c_int), value :: nx, ny, depth, kg0, first_par
      integer(c_int) :: rc
    end function
    function ndsmk_d2d(dst, src, bytes) bind(c, name="ndsmk_d2d") result(rc)
      import :: c_ptr, c_size_t, c_int
      type(c_ptr), value :: dst, src
      integer(c_size_t), value :: bytes
      integer(c_int) :: rc
    end function

    function ndsmk_fill0(p, bytes) bind(c, name="ndsmk_fill0") result(rc)
      import :: c_ptr, c_size_t, c_int
      type(c_ptr), value :: p
      integer(c_size_t), value :: bytes
      integer(c_int) :: rc
    end function

    function ndsmk_sync() bind(c, name="ndsmk_sync") result(rc)
      import :: c_int
      integer(c_int) :: rc
    end function

    function ndsmk_timer_start() bind(c, name="ndsmk_timer_start") result(rc)
      import :: c_int
      integer(c_int) :: rc
    end function

    function ndsmk_timer_stop(ms) bind(c, name="ndsmk_timer_stop") result(rc)
      import :: c_int, c_double
      real(c_double), intent(out) :: ms
      integer(c_int) :: rc
    end function

    function ndsmk_relax(g, u, ualt, rhs, nsweeps, variant, result_in_alt) bind(c, name="ndsmk_relax") result(rc)
      import :: ndsmk_grid, c_ptr, c_int
      type(ndsmk_grid), intent(in) :: g
      type(c_ptr), value :: u, ualt, rhs
      integer(c_int), value :: nsweeps, variant
      integer(c_int), intent(out) :: result_in_alt
      integer(c_int) :: rc
    end function

    function ndsmk_relax_residual(g, u, ualt, rhs, r, nsweeps, variant, result_in_alt) &
        bind(c, name="ndsmk_relax_residual") result(rc)
      import :: ndsmk_grid, c_ptr, c_int
      type(ndsmk_grid), intent(in) :: g
      type(c_ptr), value :: u, ualt, rhs, r
      integer(c_int), value :: nsweeps, variant
      integer(c_int), intent(out) :: result_in_alt
      integer(c_int) :: rc
    end function

    ! the same two calls on a level whose u is zero and was never written: r = c_null_ptr: no residual
    function ndsmk_relax_zero_src(g, u, ualt, rhs, r, nsweeps, variant, result_in_alt) &
        bind(c, name="ndsmk_relax_zero_src") result(rc)
      import :: ndsmk_grid, c_ptr, c_int
      type(ndsmk_grid), intent(in) :: g
      type(c_ptr), value :: u, ualt, rhs, r
      integer(c_int), value :: nsweeps, variant
      integer(c_int), intent(out) :: result_in_alt
      integer(c_int) :: rc
    end function

    ! 1: that call would take the zeros from a descriptor of zero records, 0: it would write them first
    function ndsmk_relax_zero_src_ok(g, has_rhs, nsweeps, variant, with_res) &
        bind(c, name="ndsmk_relax_zero_src_ok") result(ok)
      import :: ndsmk_grid, c_int
      type(ndsmk_grid), intent(in) :: g
      integer(c_int), value :: has_rhs, nsweeps, variant, with_res
      integer(c_int) :: ok
    end function

    function ndsmk_zero_guess_on() bind(c, name="ndsmk_zero_guess_on") result(on)
      import :: c_int
      integer(c_int) :: on
    end function

    function ndsmk_debug_zero_guess(on) bind(c, name="ndsmk_debug_zero_guess") result(rc)
      import :: c_int
      integer(c_int), value :: on
      integer(c_int) :: rc
    end function

    ! px: c_loc of an ndsmk_xfer (u += P uc before the sweeps) or c_null_ptr
    function ndsmk_relax3(g, u, a, b, keep, rhs, nsweeps, r, prev, where, met_done, px, uc) &
        bind(c, name="ndsmk_relax3") result(rc)
      import :: ndsmk_grid, c_ptr, c_int
      type(ndsmk_grid), intent(in) :: g
      type(c_ptr), value :: u, a, b, keep, rhs, r, prev, px, uc
      integer(c_int), value :: nsweeps
      integer(c_int), intent(out) :: where, met_done
      integer(c_int) :: rc
    end function

    function ndsmk_fetch_fused_metric(h_out2) bind(c, name="ndsmk_fetch_fused_metric") result(rc)
      import :: c_int, c_double
      real(c_double), intent(out) :: h_out2(2)
      integer(c_int) :: rc
    end function

    function ndsmk_fused_window(g, u, uout, rhs, nsweeps, z0, z1, px, uc, prev, accumulate) &
        bind(c, name="ndsmk_fused_window") result(rc)
      import :: ndsmk_grid, c_ptr, c_int
      type(ndsmk_grid), intent(in) :: g
      type(c_ptr), value :: u, uout, rhs, px, uc, prev
      integer(c_int), value :: nsweeps, z0, z1, accumulate
      integer(c_int) :: rc
    end function

    function ndsmk_fused_window_res(g, u, uout, rhs, rout, z0, z1) bind(c, name="ndsmk_fused_window_res") result(rc)
      import :: ndsmk_grid, c_ptr, c_int
      type(ndsmk_grid), intent(in) :: g
      type(c_ptr), value :: u, uout, rhs, rout
      integer(c_int), value :: z0, z1
      integer(c_int) :: rc
    end function

    function ndsmk_fused_metric_ok(g) bind(c, name="ndsmk_fused_metric_ok") result(ok)
      import :: ndsmk_grid, c_int
      type(ndsmk_grid), intent(in) :: g
      integer(c_int) :: ok
    end function

    function ndsmk_fused_prolong_ok(g, rhs, nsweeps) bind(c, name="ndsmk_fused_prolong_ok") result(ok)
      import :: ndsmk_grid, c_ptr, c_int
      type(ndsmk_grid), intent(in) :: g
      type(c_ptr), value :: rhs
      integer(c_int), value :: nsweeps
      integer(c_int) :: ok
    end function

    function ndsmk_note_error(code, what) bind(c, name="ndsmk_note_error") result(rc)
      import :: c_int, c_char
      integer(c_int), value :: code
      character(kind=c_char), intent(in) :: what(*)
      integer(c_int) :: rc
    end function

    function ndsmk_select_lane(lane) bind(c, name="ndsmk_select_lane") result(rc)
      import :: c_int
      integer(c_int), value :: lane
      integer(c_int) :: rc
    end function

    function ndsmk_lane_idle(lane) bind(c, name="ndsmk_lane_idle") result(rc)
      import :: c_int
      integer(c_int), value :: lane
      integer(c_int) :: rc
    end function
    function ndsmk_lane_fence(lane, to_main) bind(c, name="ndsmk_lane_fence") result(rc)
      import :: c_int
      integer(c_int), value :: lane, to_main
      integer(c_int) :: rc
    end function

    function ndsmk_lane_sync(lane) bind(c, name="ndsmk_lane_sync") result(rc)
      import :: c_int
      integer(c_int), value :: lane
      integer(c_int) :: rc
    end function

    function ndsmk_capture_begin() bind(c, name="ndsmk_capture_begin") result(rc)
      import :: c_int
      integer(c_int) :: rc
    end function

    function ndsmk_capture_end(exec) bind(c, name="ndsmk_capture_end") result(rc)
      import :: c_int, c_ptr
      type(c_ptr), intent(out) :: exec
      integer(c_int) :: rc
    end function

    function ndsmk_graph_launch(exec) bind(c, name="ndsmk_graph_launch") result(rc)
      import :: c_int, c_ptr
      type(c_ptr), value :: exec
      integer(c_int) :: rc
    end function

    function ndsmk_graph_destroy(exec) bind(c, name="ndsmk_graph_destroy") result(rc)
      import :: c_int, c_ptr
      type(c_ptr), value :: exec
      integer(c_int) :: rc
    end function

    function ndsmk_diff_metrics_begin(a, b, n, copy) bind(c, name="ndsmk_diff_metrics_begin") result(rc)
      import :: c_ptr, c_int64_t, c_int
      type(c_ptr), value :: a, b
      integer(c_int64_t), value :: n
      integer(c_int), value :: copy
      integer(c_int) :: rc
    end function

    function ndsmk_diff_metrics_end(out2) bind(c, name="ndsmk_diff_metrics_end") result(rc)
      import :: c_int, c_double
      real(c_double), intent(out) :: out2(2)
      integer(c_int) :: rc
    end function

    function ndsmk_select_stream(which) bind(c, name="ndsmk_select_stream") result(rc)
      import :: c_int
      integer(c_int), value :: which
      integer(c_int) :: rc
    end function

    function ndsmk_stream_fence(from, to) bind(c, name="ndsmk_stream_fence") result(rc)
      import :: c_int
      integer(c_int), value :: from, to
      integer(c_int) :: rc
    end function

    function ndsmk_update_residual_f32(g, u, unew, rhs, e, ezero, r, h_out2) &
        bind(c, name="ndsmk_update_residual_f32") result(rc)
      import :: ndsmk_grid, c_ptr, c_int, c_double
      type(ndsmk_grid), intent(in) :: g
      type(c_ptr), value :: u, unew, rhs, e, ezero, r
      real(c_double), intent(out) :: h_out2(2)
      integer(c_int) :: rc
    end function

    function ndsmk_relax_f32(g, e, ealt, r, nsweeps, force, r_out, result_in_alt) &
        bind(c, name="ndsmk_relax_f32") result(rc)
      import :: ndsmk_grid, c_ptr, c_int
      type(ndsmk_grid), intent(in) :: g
      type(c_ptr), value :: e, ealt, r, r_out
      integer(c_int), value :: nsweeps, force
      integer(c_int), intent(out) :: result_in_alt
      integer(c_int) :: rc
    end function

    function ndsmk_restrict_f32(x, r_f, rhs_c, u_c) bind(c, name="ndsmk_restrict_f32") result(rc)
      import :: ndsmk_xfer, c_ptr, c_int
      type(ndsmk_xfer), intent(in) :: x
      type(c_ptr), value :: r_f, rhs_c, u_c
      integer(c_int) :: rc
    end function

    function ndsmk_prolong_add_f32(x, u_c, e_f) bind(c, name="ndsmk_prolong_add_f32") result(rc)
      import :: ndsmk_xfer, c_ptr, c_int
      type(ndsmk_xfer), intent(in) :: x
      type(c_ptr), value :: u_c, e_f
      integer(c_int) :: rc
    end function

    function ndsmk_residual(g, u, rhs, r) bind(c, name="ndsmk_residual") result(rc)
      import :: ndsmk_grid, c_ptr, c_int
      type(ndsmk_grid), intent(in) :: g
      type(c_ptr), value :: u, rhs, r
      integer(c_int) :: rc
    end function

    function ndsmk_restrict(x, r_f, rhs_c, u_c) bind(c, name="ndsmk_restrict") result(rc)
      import :: ndsmk_xfer, c_ptr, c_int
      type(ndsmk_xfer), intent(in) :: x
      type(c_ptr), value :: r_f, rhs_c, u_c
      integer(c_int) :: rc
    end function

    subroutine ndsmk_restrict_stream_tile(ci, cj, fx, fy, maxt) bind(c, name="ndsmk_restrict_stream_tile")
      import :: c_int
      integer(c_int), intent(out) :: ci, cj, fx, fy, maxt
    end subroutine

    function ndsmk_restrict_stream_min_points() bind(c, name="ndsmk_restrict_stream_min_points") result(n)
      import :: c_long_long
      integer(c_long_long) :: n
    end function

    function ndsmk_debug_transfer_cfg(restrict_min_points, prolong_min_points, rs_variant, rs_chunk) &
        bind(c, name="ndsmk_debug_transfer_cfg") result(rc)
      import :: c_long_long, c_int
      integer(c_long_long), value :: restrict_min_points, prolong_min_points
      integer(c_int), value :: rs_variant, rs_chunk
      integer(c_int) :: rc
    end function

    function ndsmk_debug_transfer_form(x, out) bind(c, name="ndsmk_debug_transfer_form") result(rc)
      import :: ndsmk_xfer, c_int
      type(ndsmk_xfer), intent(in) :: x
      integer(c_int), intent(out) :: out(4)
      integer(c_int) :: rc
    end function

    function ndsmk_prolong_add(x, u_c, u_f) bind(c, name="ndsmk_prolong_add") result(rc)
      import :: ndsmk_xfer, c_ptr, c_int
      type(ndsmk_xfer), intent(in) :: x
      type(c_ptr), value :: u_c, u_f
      integer(c_int) :: rc
    end function

    function ndsmk_diff_metrics(a, b, n, copy, out2) bind(c, name="ndsmk_diff_metrics") result(rc)
      import :: c_ptr, c_int64_t, c_int, c_double
      type(c_ptr), value :: a, b
      integer(c_int64_t), value :: n
      integer(c_int), value :: copy
      real(c_double), intent(out) :: out2(2)
      integer(c_int) :: rc
    end function

    function ndsmk_solve_exact(g, u, rhs, scratch, ex_tol, use_max, nmax, d_info) &
        bind(c, name="ndsmk_solve_exact") result(rc)
      import :: ndsmk_grid, c_ptr, c_int, c_double
      type(ndsmk_grid), intent(in) :: g
      type(c_ptr), value :: u, rhs, scratch, d_info
      real(c_double), value :: ex_tol
      integer(c_int), value :: use_max, nmax
      integer(c_int) :: rc
    end function

    function ndsmk_solve_exact_on_device(g) bind(c, name="ndsmk_solve_exact_on_device") result(ok)
      import :: ndsmk_grid, c_int
      type(ndsmk_grid), intent(in) :: g
      integer(c_int) :: ok
    end function

    function ndsmk_tail_applies(nlev, g, x) bind(c, name="ndsmk_tail_applies") result(ok)
      import :: ndsmk_grid, ndsmk_xfer, c_int
      integer(c_int), value :: nlev
      type(ndsmk_grid), intent(in) :: g(*)
      type(ndsmk_xfer), intent(in) :: x(*)
      integer(c_int) :: ok
    end function

    function ndsmk_tail_cycle(nlev, g, x, u, rhs, ms, ex_tol, use_max, nmax, d_info) &
        bind(c, name="ndsmk_tail_cycle") result(rc)
      import :: ndsmk_grid, ndsmk_xfer, c_ptr, c_int, c_double
      integer(c_int), value :: nlev
      type(ndsmk_grid), intent(in) :: g(*)
      type(ndsmk_xfer), intent(in) :: x(*)
      type(c_ptr), intent(in) :: u(*), rhs(*)
      integer(c_int), value :: ms
      real(c_double), value :: ex_tol
      integer(c_int), value :: use_max, nmax
      type(c_ptr), value :: d_info
      integer(c_int) :: rc
    end function

    function ndsmk_debug_relax_plan(what, grid, req, knobs, cap, out) bind(c, name="ndsmk_debug_relax_plan") result(rc)
      import :: c_int, c_ptr
      integer(c_int), value :: what, cap
      type(c_ptr), value :: grid, req, knobs, out
      integer(c_int) :: rc
    end function

    function ndsmk_debug_tail(on) bind(c, name="ndsmk_debug_tail") result(rc)
      import :: c_int
      integer(c_int), value :: on
      integer(c_int) :: rc
    end function

    function ndsmk_balance_curl(A, B, n3, x, y, z, phi6, span3, dq3, curl_first) &
        bind(c, name="ndsmk_balance_curl") result(rc)
      import :: c_ptr, c_int, c_int32_t, c_double
      type(c_ptr), value :: A, B, x, y, z
      integer(c_int32_t), intent(in) :: n3(3)
      real(c_double), intent(in) :: phi6(6), span3(3), dq3(3)
      integer(c_int), value :: curl_first
      integer(c_int) :: rc
    end function

    function ndsmk_balance_curl_slab(A, B, n3, kg0, na, nb, boff, x, y, z, phi6, span3, dq3, curl_first) &
        bind(c, name="ndsmk_balance_curl_slab") result(rc)
      import :: c_ptr, c_int, c_int32_t, c_double
      type(c_ptr), value :: A, B, x, y, z
      integer(c_int32_t), intent(in) :: n3(3)
      integer(c_int), value :: kg0, na, nb, boff
      real(c_double), intent(in) :: phi6(6), span3(3), dq3(3)
      integer(c_int), value :: curl_first
      integer(c_int) :: rc
    end function

    ! ---- background transfers, pinned memory (runtime.hip) ----
    function ndsmk_bg_upload_unless_zero(h_src, d_dst, bytes, ticket) bind(c, name="ndsmk_bg_upload_unless_zero") result(rc)
      import :: c_ptr, c_size_t, c_int
      type(c_ptr), value :: h_src, d_dst
      integer(c_size_t), value :: bytes
      integer(c_int), intent(out) :: ticket
      integer(c_int) :: rc
    end function
    function ndsmk_bg_download(h_dst, d_src, bytes, ticket) bind(c, name="ndsmk_bg_download") result(rc)
      import :: c_ptr, c_size_t, c_int
      type(c_ptr), value :: h_dst, d_src
      integer(c_size_t), value :: bytes
      integer(c_int), intent(out) :: ticket
      integer(c_int) :: rc
    end function
    function ndsmk_bg_first_touch(h_dst, bytes, ticket) bind(c, name="ndsmk_bg_first_touch") result(rc)
      import :: c_ptr, c_size_t, c_int
      type(c_ptr), value :: h_dst
      integer(c_size_t), value :: bytes
      integer(c_int), intent(out) :: ticket
      integer(c_int) :: rc
    end function
    function ndsmk_bg_wait(ticket, flag) bind(c, name="ndsmk_bg_wait") result(rc)
      import :: c_int
      integer(c_int), value :: ticket
      integer(c_int), intent(out) :: flag
      integer(c_int) :: rc
    end function
    function ndsmk_bg_drain() bind(c, name="ndsmk_bg_drain") result(rc)
      import :: c_int
      integer(c_int) :: rc
    end function
    function ndsmk_host_alloc(p, bytes) bind(c, name="ndsmk_host_alloc") result(rc)
      import :: c_ptr, c_size_t, c_int
      type(c_ptr), intent(out) :: p
      integer(c_size_t), value :: bytes
      integer(c_int) :: rc
    end function
    function ndsmk_host_free(p) bind(c, name="ndsmk_host_free") result(rc)
      import :: c_ptr, c_int
      type(c_ptr), value :: p
      integer(c_int) :: rc
    end function
    function ndsmk_mem_info(free_bytes, total_bytes) bind(c, name="ndsmk_mem_info") result(rc)
      import :: c_size_t, c_int
      integer(c_size_t), intent(out) :: free_bytes, total_bytes
      integer(c_int) :: rc
    end function
    function ndsmk_h2d_async(dst, src, bytes) bind(c, name="ndsmk_h2d_async") result(rc)
      import :: c_ptr, c_size_t, c_int
      type(c_ptr), value :: dst, src
      integer(c_size_t), value :: bytes
      integer(c_int) :: rc
    end function
    subroutine ndsmk_on_low_memory(fn) bind(c, name="ndsmk_on_low_memory")
      import :: c_funptr
      type(c_funptr), value :: fn
    end subroutine
    subroutine ndsmk_at_reset(fn) bind(c, name="ndsmk_at_reset")
      import :: c_funptr
      type(c_funptr), value :: fn
    end subroutine

    ! ---- one component of the flux balance, the curl alone (post.hip) ----
    function ndsmk_balance_component(Ac, n3, c, x, y, z, phi6, span3) bind(c, name="ndsmk_balance_component") result(rc)
      import :: c_ptr, c_int, c_int32_t, c_double
      type(c_ptr), value :: Ac, x, y, z
      integer(c_int32_t), intent(in) :: n3(3)
      integer(c_int), value :: c
      real(c_double), intent(in) :: phi6(6), span3(3)
      integer(c_int) :: rc
    end function
    function ndsmk_curl_component(A, B, n3, dq3, c) bind(c, name="ndsmk_curl_component") result(rc)
      import :: c_ptr, c_int, c_int32_t, c_double
      type(c_ptr), value :: A, B
      integer(c_int32_t), intent(in) :: n3(3)
      real(c_double), intent(in) :: dq3(3)
      integer(c_int), value :: c
      integer(c_int) :: rc
    end function

    function ndsmk_curl(A, B, n3, dq3) bind(c, name="ndsmk_curl") result(rc)
      import :: c_ptr, c_int, c_int32_t, c_double
      type(c_ptr), value :: A, B
      integer(c_int32_t), intent(in) :: n3(3)
      real(c_double), intent(in) :: dq3(3)
      integer(c_int) :: rc
    end function

    ! ---- the current-carrying field (field.hip) ----
    function ndsmk_curl_rhs(B, rhs, n3, dq3, c) bind(c, name="ndsmk_curl_rhs") result(rc)
      import :: c_ptr, c_int, c_int32_t, c_double
      type(c_ptr), value :: B, rhs
      integer(c_int32_t), intent(in) :: n3(3)
      real(c_double), intent(in) :: dq3(3)
      integer(c_int), value :: c
      integer(c_int) :: rc
    end function
    ! ---- the nonlinear force-free field (field.hip, alphamap.hip) ----
    function ndsmk_current_rhs(F, alpha, rhs, n3, c) bind(c, name="ndsmk_current_rhs") result(rc)
      import :: c_ptr, c_int, c_int32_t
      type(c_ptr), value :: F, alpha, rhs
      integer(c_int32_t), intent(in) :: n3(3)
      integer(c_int), value :: c
      integer(c_int) :: rc
    end function
    function ndsmk_nlfff_metrics(B, Bold, status, n3, dq3, out4) bind(c, name="ndsmk_nlfff_metrics") result(rc)
      import :: c_ptr, c_int, c_int32_t, c_double
      type(c_ptr), value :: B, Bold, status
      integer(c_int32_t), intent(in) :: n3(3)
      real(c_double), intent(in) :: dq3(3)
      real(c_double), intent(out) :: out4(4)
      integer(c_int) :: rc
    end function
    function ndsmk_alpha_map(B, n3, lo3, dq3, alpha0, polarity, step, max_steps, alpha, status) &
        bind(c, name="ndsmk_alpha_map") result(rc)
      import :: c_ptr, c_int, c_int32_t, c_double
      type(c_ptr), value :: B, alpha0, alpha, status
      integer(c_int32_t), intent(in) :: n3(3)
      real(c_double), intent(in) :: lo3(3), dq3(3)
      integer(c_int), value :: polarity, max_steps
      real(c_double), value :: step
      integer(c_int) :: rc
    end function
    ! ---- the optimization-method force-free solver (optimize.hip) ----
    function ndsmk_optimize_work_bytes() bind(c, name="ndsmk_optimize_work_bytes") result(nb)
      import :: c_size_t
      integer(c_size_t) :: nb
    end function
    function ndsmk_optimize_begin(B0, B1, O, w, work, n3, dq3, dt0, dt_min) bind(c, name="ndsmk_optimize_begin") &
        result(rc)
      import :: c_ptr, c_int, c_int32_t, c_double
      type(c_ptr), value :: B0, B1, O, w, work
      integer(c_int32_t), intent(in) :: n3(3)
      real(c_double), intent(in) :: dq3(3)
      real(c_double), value :: dt0, dt_min
      integer(c_int) :: rc
    end function
    function ndsmk_optimize_tries(B0, B1, O, w, work, n3, dq3, dt_min, ntries) bind(c, name="ndsmk_optimize_tries") &
        result(rc)
      import :: c_ptr, c_int, c_int32_t, c_double
      type(c_ptr), value :: B0, B1, O, w, work
      integer(c_int32_t), intent(in) :: n3(3)
      real(c_double), intent(in) :: dq3(3)
      real(c_double), value :: dt_min
      integer(c_int), value :: ntries
      integer(c_int) :: rc
    end function
    function ndsmk_optimize_row(work, row8) bind(c, name="ndsmk_optimize_row") result(rc)
      import :: c_ptr, c_int, c_double
      type(c_ptr), value :: work
      real(c_double), intent(out) :: row8(8)
      integer(c_int) :: rc
    end function
    ! ---- the same with a measurement term and a freed lower face (optimize_obs.hip) ----
    function ndsmk_optimize_obs_work_bytes() bind(c, name="ndsmk_optimize_obs_work_bytes") result(nb)
      import :: c_size_t
      integer(c_size_t) :: nb
    end function
    function ndsmk_optimize_obs_begin(B0, B1, O, w, Bobs, wm, work, n3, dq3, nu, dt0, dt_min) &
        bind(c, name="ndsmk_optimize_obs_begin") result(rc)
      import :: c_ptr, c_int, c_int32_t, c_double
      type(c_ptr), value :: B0, B1, O, w, Bobs, wm, work
      integer(c_int32_t), intent(in) :: n3(3)
      real(c_double), intent(in) :: dq3(3)
      real(c_double), value :: nu, dt0, dt_min
      integer(c_int) :: rc
    end function
    function ndsmk_optimize_obs_tries(B0, B1, O, w, Bobs, wm, work, n3, dq3, nu, free, dt_min, ntries) &
        bind(c, name="ndsmk_optimize_obs_tries") result(rc)
      import :: c_ptr, c_int, c_int32_t, c_double
      type(c_ptr), value :: B0, B1, O, w, Bobs, wm, work
      integer(c_int32_t), intent(in) :: n3(3)
      real(c_double), intent(in) :: dq3(3)
      real(c_double), value :: nu, dt_min
      integer(c_int), value :: free, ntries
      integer(c_int) :: rc
    end function
    function ndsmk_optimize_obs_row(work, row9) bind(c, name="ndsmk_optimize_obs_row") result(rc)
      import :: c_ptr, c_int, c_double
      type(c_ptr), value :: work
      real(c_double), intent(out) :: row9(9)
      integer(c_int) :: rc
    end function
    ! ---- the cascade's level changes (resample.hip) ----
    function ndsmk_resample(nsrc3, ndst3, ncomp, mode, src, dst) bind(c, name="ndsmk_resample") result(rc)
      import :: c_ptr, c_int, c_int32_t
      integer(c_int32_t), intent(in) :: nsrc3(3), ndst3(3)
      integer(c_int), value :: ncomp, mode
      type(c_ptr), value :: src, dst
      integer(c_int) :: rc
    end function
    function ndsmk_resample_weighted(nsrc3, ndst3, ncomp, src, wsrc, dst, wdst) &
        bind(c, name="ndsmk_resample_weighted") result(rc)
      import :: c_ptr, c_int, c_int32_t
      integer(c_int32_t), intent(in) :: nsrc3(3), ndst3(3)
      integer(c_int), value :: ncomp
      type(c_ptr), value :: src, wsrc, dst, wdst
      integer(c_int) :: rc
    end function
    function ndsmk_paste_faces(n3, ncomp, which, src, dst) bind(c, name="ndsmk_paste_faces") result(rc)
      import :: c_ptr, c_int, c_int32_t
      integer(c_int32_t), intent(in) :: n3(3)
      integer(c_int), value :: ncomp, which
      type(c_ptr), value :: src, dst
      integer(c_int) :: rc
    end function
    ! ---- the Green's-function field of a magnetogram (green.hip) ----
    function ndsmk_green_fits(nsrc2, n3, which, ntargets, caller_bytes) bind(c, name="ndsmk_green_fits") result(rc)
      import :: c_ptr, c_int, c_int32_t, c_long_long, c_double
      integer(c_int32_t), intent(in) :: nsrc2(2)
      type(c_ptr), value :: n3
      integer(c_int), value :: which
      integer(c_long_long), value :: ntargets
      real(c_double), value :: caller_bytes
      integer(c_int) :: rc
    end function
    function ndsmk_green_points(nsrc2, h_xs, h_ys, zs, bz, npts, pts, B) bind(c, name="ndsmk_green_points") result(rc)
      import :: c_ptr, c_int, c_int32_t, c_double
      integer(c_int32_t), intent(in) :: nsrc2(2)
      type(c_ptr), value :: h_xs, h_ys, bz, pts, B
      real(c_double), value :: zs
      integer(c_int), value :: npts
      integer(c_int) :: rc
    end function
    function ndsmk_green_box(nsrc2, h_xs, h_ys, zs, bz, n3, h_x, h_y, h_z, which, B) &
        bind(c, name="ndsmk_green_box") result(rc)
      import :: c_ptr, c_int, c_int32_t, c_double
      integer(c_int32_t), intent(in) :: nsrc2(2), n3(3)
      type(c_ptr), value :: h_xs, h_ys, bz, h_x, h_y, h_z, B
      real(c_double), value :: zs
      integer(c_int), value :: which
      integer(c_int) :: rc
    end function
    ! the constant-alpha field of the same source: the two launchers above with alpha
    function ndsmk_lfff_points(nsrc2, h_xs, h_ys, zs, bz, alpha, npts, pts, B) bind(c, name="ndsmk_lfff_points") &
        result(rc)
      import :: c_ptr, c_int, c_int32_t, c_double
      integer(c_int32_t), intent(in) :: nsrc2(2)
      type(c_ptr), value :: h_xs, h_ys, bz, pts, B
      real(c_double), value :: zs, alpha
      integer(c_int), value :: npts
      integer(c_int) :: rc
    end function
    function ndsmk_lfff_box(nsrc2, h_xs, h_ys, zs, bz, alpha, n3, h_x, h_y, h_z, which, B) &
        bind(c, name="ndsmk_lfff_box") result(rc)
      import :: c_ptr, c_int, c_int32_t, c_double
      integer(c_int32_t), intent(in) :: nsrc2(2), n3(3)
      type(c_ptr), value :: h_xs, h_ys, bz, h_x, h_y, h_z, B
      real(c_double), value :: zs, alpha
      integer(c_int), value :: which
      integer(c_int) :: rc
    end function
    ! the plane's vector potential of the same source: the third pair term
    function ndsmk_green_ap_points(nsrc2, h_xs, h_ys, bz, npts, pts, Ap) bind(c, name="ndsmk_green_ap_points") &
        result(rc)
      import :: c_ptr, c_int, c_int32_t
      integer(c_int32_t), intent(in) :: nsrc2(2)
      type(c_ptr), value :: h_xs, h_ys, bz, pts, Ap
      integer(c_int), value :: npts
      integer(c_int) :: rc
    end function
    function ndsmk_green_ap_plane(nsrc2, h_xs, h_ys, bz, Ap) bind(c, name="ndsmk_green_ap_plane") result(rc)
      import :: c_ptr, c_int, c_int32_t
      integer(c_int32_t), intent(in) :: nsrc2(2)
      type(c_ptr), value :: h_xs, h_ys, bz, Ap
      integer(c_int) :: rc
    end function
    ! ---- flows from two magnetograms and the boundary fluxes (flow.hip) ----
    function ndsmk_flow_fits(nsrc2, fit, caller_bytes) bind(c, name="ndsmk_flow_fits") result(rc)
      import :: c_int, c_int32_t, c_double
      integer(c_int32_t), intent(in) :: nsrc2(2)
      integer(c_int), value :: fit
      real(c_double), value :: caller_bytes
      integer(c_int) :: rc
    end function
    function ndsmk_flow_fit(nsrc2, h_xs, h_ys, B0, B1, dt, r, rcond, V, coef, status) &
        bind(c, name="ndsmk_flow_fit") result(rc)
      import :: c_ptr, c_int, c_int32_t, c_double
      integer(c_int32_t), intent(in) :: nsrc2(2)
      type(c_ptr), value :: h_xs, h_ys, B0, B1, V, coef, status
      real(c_double), value :: dt, rcond
      integer(c_int), value :: r
      integer(c_int) :: rc
    end function
    function ndsmk_flow_flux(nsrc2, h_xs, h_ys, B, V, Ap, dens, out8) bind(c, name="ndsmk_flow_flux") result(rc)
      import :: c_ptr, c_int, c_int32_t
      integer(c_int32_t), intent(in) :: nsrc2(2)
      type(c_ptr), value :: h_xs, h_ys, B, V, Ap, dens, out8
      integer(c_int) :: rc
    end function
    ! ---- magnetogram preprocessing (preprocess.hip) ----
    function ndsmk_preprocess_work_bytes() bind(c, name="ndsmk_preprocess_work_bytes") result(nb)
      import :: c_size_t
      integer(c_size_t) :: nb
    end function
    function ndsmk_preprocess_begin(B0, B1, La, obs, work, n2, dq2, mu5, dt0, dt_min) &
        bind(c, name="ndsmk_preprocess_begin") result(rc)
      import :: c_ptr, c_int, c_int32_t, c_double
      type(c_ptr), value :: B0, B1, La, obs, work
      integer(c_int32_t), intent(in) :: n2(2)
      real(c_double), intent(in) :: dq2(2), mu5(5)
      real(c_double), value :: dt0, dt_min
      integer(c_int) :: rc
    end function
    function ndsmk_preprocess_tries(B0, B1, La, obs, work, n2, dq2, mu5, dt_min, ntries) &
        bind(c, name="ndsmk_preprocess_tries") result(rc)
      import :: c_ptr, c_int, c_int32_t, c_double
      type(c_ptr), value :: B0, B1, La, obs, work
      integer(c_int32_t), intent(in) :: n2(2)
      real(c_double), intent(in) :: dq2(2), mu5(5)
      real(c_double), value :: dt_min
      integer(c_int), value :: ntries
      integer(c_int) :: rc
    end function
    function ndsmk_preprocess_row(work, row21) bind(c, name="ndsmk_preprocess_row") result(rc)
      import :: c_ptr, c_int, c_double
      type(c_ptr), value :: work
      real(c_double), intent(out) :: row21(21)
      integer(c_int) :: rc
    end function
    function ndsmk_helicity_reduce(A, Ap, B, Bp, Br, n3, dq3, out8) bind(c, name="ndsmk_helicity_reduce") result(rc)
      import :: c_ptr, c_int, c_int32_t, c_double
      type(c_ptr), value :: A, Ap, B, Bp, Br
      integer(c_int32_t), intent(in) :: n3(3)
      real(c_double), intent(in) :: dq3(3)
      real(c_double), intent(out) :: out8(8)
      integer(c_int) :: rc
    end function

    ! ---- the solenoidal projection (project.hip) ----
    function ndsmk_project_div_rhs(B, rhs, n3, dq3) bind(c, name="ndsmk_project_div_rhs") result(rc)
      import :: c_ptr, c_int, c_int32_t, c_double
      type(c_ptr), value :: B, rhs
      integer(c_int32_t), intent(in) :: n3(3)
      real(c_double), intent(in) :: dq3(3)
      integer(c_int) :: rc
    end function
    function ndsmk_project_grad_sub(B, phi, n3, dq3) bind(c, name="ndsmk_project_grad_sub") result(rc)
      import :: c_ptr, c_int, c_int32_t, c_double
      type(c_ptr), value :: B, phi
      integer(c_int32_t), intent(in) :: n3(3)
      real(c_double), intent(in) :: dq3(3)
      integer(c_int) :: rc
    end function
    function ndsmk_project_div_max(B, n3, dq3, out4) bind(c, name="ndsmk_project_div_max") result(rc)
      import :: c_ptr, c_int, c_int32_t, c_double
      type(c_ptr), value :: B
      integer(c_int32_t), intent(in) :: n3(3)
      real(c_double), intent(in) :: dq3(3)
      real(c_double), intent(out) :: out4(4)
      integer(c_int) :: rc
    end function

    ! ---- DeVore-gauge vector potentials (devore.hip) ----
    function ndsmk_devore(B, Bp, A, Ap, n3, dq3) bind(c, name="ndsmk_devore") result(rc)
      import :: c_ptr, c_int, c_int32_t, c_double
      type(c_ptr), value :: B, Bp, A, Ap
      integer(c_int32_t), intent(in) :: n3(3)
      real(c_double), intent(in) :: dq3(3)
      integer(c_int) :: rc
    end function

    ! ---- field lines and line integrals (trace.hip) ----
    function ndsmk_trace(B, G, n3, lo3, dq3, nseeds, seeds, step, max_steps, direction, ends, length, integral, &
                         status, nsteps) bind(c, name="ndsmk_trace") result(rc)
      import :: c_ptr, c_int, c_int32_t, c_double
      type(c_ptr), value :: B, G, seeds, ends, length, integral, status, nsteps
      integer(c_int32_t), intent(in) :: n3(3)
      real(c_double), intent(in) :: lo3(3), dq3(3)
      integer(c_int), value :: nseeds, max_steps, direction
      real(c_double), value :: step
      integer(c_int) :: rc
    end function

    ! ---- squashing factor and line integrals (squash.hip) ----
    function ndsmk_squash(B, G, integrand, n3, lo3, dq3, nseeds, seeds, step, max_steps, q, ends, length, integral, &
                          status, nsteps) bind(c, name="ndsmk_squash") result(rc)
      import :: c_ptr, c_int, c_int32_t, c_double
      type(c_ptr), value :: B, G, seeds, q, ends, length, integral, status, nsteps
      integer(c_int32_t), intent(in) :: n3(3)
      real(c_double), intent(in) :: lo3(3), dq3(3)
      integer(c_int), value :: integrand, nseeds, max_steps
      real(c_double), value :: step
      integer(c_int) :: rc
    end function

    ! the same with the perpendicular squashing factor qperp (nseeds) after q
    function ndsmk_squash_perp(B, G, integrand, n3, lo3, dq3, nseeds, seeds, step, max_steps, q, qperp, ends, length, &
                               integral, status, nsteps) bind(c, name="ndsmk_squash_perp") result(rc)
      import :: c_ptr, c_int, c_int32_t, c_double
      type(c_ptr), value :: B, G, seeds, q, qperp, ends, length, integral, status, nsteps
      integer(c_int32_t), intent(in) :: n3(3)
      real(c_double), intent(in) :: lo3(3), dq3(3)
      integer(c_int), value :: integrand, nseeds, max_steps
      real(c_double), value :: step
      integer(c_int) :: rc
    end function

    ! ---- null points (nulls.hip) ----
    function ndsmk_nulls(B, n3, lo3, dq3, max_nulls, counts2, cell, pos, jac, det, resid, sign, iters) &
        bind(c, name="ndsmk_nulls") result(rc)
      import :: c_ptr, c_int, c_int32_t, c_int64_t, c_double
      type(c_ptr), value :: B, cell, pos, jac, det, resid, sign, iters
      integer(c_int32_t), intent(in) :: n3(3)
      real(c_double), intent(in) :: lo3(3), dq3(3)
      integer(c_int), value :: max_nulls
      integer(c_int64_t), intent(out) :: counts2(2)
      integer(c_int) :: rc
    end function

    ! ---- dips and bald patches (dips.hip) ----
    function ndsmk_dips(B, n3, lo3, dq3, plane_only, max_dips, counts3, edge, pos, bpt, grad, curv, flag) &
        bind(c, name="ndsmk_dips") result(rc)
      import :: c_ptr, c_int, c_int32_t, c_int64_t, c_double
      type(c_ptr), value :: B, edge, pos, bpt, grad, curv, flag
      integer(c_int32_t), intent(in) :: n3(3)
      real(c_double), intent(in) :: lo3(3), dq3(3)
      integer(c_int), value :: plane_only
      integer(c_int64_t), value :: max_dips
      integer(c_int64_t), intent(out) :: counts3(3)
      integer(c_int) :: rc
    end function

    ! ---- flux partitioning of a magnetogram (partition.hip) and patch connectivity (connect.hip) ----
    function ndsmk_partition_fits(nsrc2, caller_bytes) bind(c, name="ndsmk_partition_fits") result(rc)
      import :: c_int, c_int32_t, c_double
      integer(c_int32_t), intent(in) :: nsrc2(2)
      real(c_double), value :: caller_bytes
      integer(c_int) :: rc
    end function
    function ndsmk_partition(nsrc2, h_xs, h_ys, bz, thr, max_patches, counts2, label, root, sign, npix, flux, sx, sy) &
        bind(c, name="ndsmk_partition") result(rc)
      import :: c_ptr, c_int, c_int32_t, c_int64_t, c_double
      integer(c_int32_t), intent(in) :: nsrc2(2)
      type(c_ptr), value :: h_xs, h_ys, bz, label, root, sign, npix, flux, sx, sy
      real(c_double), value :: thr
      integer(c_int64_t), value :: max_patches
      integer(c_int64_t), intent(out) :: counts2(2)
      integer(c_int) :: rc
    end function
    function ndsmk_connect(B, n3, lo3, dq3, h_x, h_y, label, K, step, max_steps, max_pairs, counts2, dest, ends, length, &
                           status, pa, pc, nlines, pflux) bind(c, name="ndsmk_connect") result(rc)
      import :: c_ptr, c_int, c_int32_t, c_int64_t, c_double
      type(c_ptr), value :: B, label, dest, ends, length, status, pa, pc, nlines, pflux
      integer(c_int32_t), intent(in) :: n3(3)
      real(c_double), intent(in) :: lo3(3), dq3(3), h_x(*), h_y(*)
      integer(c_int), value :: K, max_steps
      real(c_double), value :: step
      integer(c_int64_t), value :: max_pairs
      integer(c_int64_t), intent(out) :: counts2(2)
      integer(c_int) :: rc
    end function

    ! ---- field-line paths (paths.hip): the counting half (blocks for total) and the filling half ----
    function ndsmk_paths_count(B, G, n3, lo3, dq3, nseeds, seeds, step, max_steps, direction, every, max_points, ends, &
                               length, integral, status, nsteps, offsets, total) bind(c, name="ndsmk_paths_count") result(rc)
      import :: c_ptr, c_int, c_int32_t, c_int64_t, c_double
      type(c_ptr), value :: B, G, seeds, ends, length, integral, status, nsteps, offsets
      integer(c_int32_t), intent(in) :: n3(3)
      real(c_double), intent(in) :: lo3(3), dq3(3)
      integer(c_int), value :: nseeds, max_steps, direction, every
      real(c_double), value :: step
      integer(c_int64_t), value :: max_points
      integer(c_int64_t), intent(out) :: total
      integer(c_int) :: rc
    end function
    function ndsmk_paths_fill(B, G, n3, lo3, dq3, nseeds, seeds, step, max_steps, direction, every, max_points, &
                              offsets, points, bpt, gpt, ipt) bind(c, name="ndsmk_paths_fill") result(rc)
      import :: c_ptr, c_int, c_int32_t, c_int64_t, c_double
      type(c_ptr), value :: B, G, seeds, offsets, points, bpt, gpt, ipt
      integer(c_int32_t), intent(in) :: n3(3)
      real(c_double), intent(in) :: lo3(3), dq3(3)
      integer(c_int), value :: nseeds, max_steps, direction, every
      real(c_double), value :: step
      integer(c_int64_t), value :: max_points
      integer(c_int) :: rc
    end function

    ! ---- spine-fan skeleton of the nulls (skeleton.hip): typing and counting (blocks for total), then filling ----
    function ndsmk_skel_count(B, n3, lo3, dq3, nnulls, pos, jac, nring, ring, radius, capture, step, max_steps, every, &
                              max_points, kind, eig, spine, normal, ends, length, status, nsteps, hit, offsets, total) &
        bind(c, name="ndsmk_skel_count") result(rc)
      import :: c_ptr, c_int, c_int32_t, c_int64_t, c_double
      type(c_ptr), value :: B, pos, jac, ring, kind, eig, spine, normal, ends, length, status, nsteps, hit, offsets
      integer(c_int32_t), intent(in) :: n3(3)
      real(c_double), intent(in) :: lo3(3), dq3(3)
      integer(c_int), value :: nnulls, nring, max_steps, every
      real(c_double), value :: radius, capture, step
      integer(c_int64_t), value :: max_points
      integer(c_int64_t), intent(out) :: total
      integer(c_int) :: rc
    end function
    function ndsmk_skel_fill(B, n3, lo3, dq3, nnulls, pos, nring, radius, capture, step, max_steps, every, max_points, &
                             offsets, points, bpt) bind(c, name="ndsmk_skel_fill") result(rc)
      import :: c_ptr, c_int, c_int32_t, c_int64_t, c_double
      type(c_ptr), value :: B, pos, offsets, points, bpt
      integer(c_int32_t), intent(in) :: n3(3)
      real(c_double), intent(in) :: lo3(3), dq3(3)
      integer(c_int), value :: nnulls, nring, max_steps, every
      real(c_double), value :: radius, capture, step
      integer(c_int64_t), value :: max_points
      integer(c_int) :: rc
    end function

    ! ---- separator lines (separators.hip): check, refinement and counting (blocks for total), then filling ----
    function ndsmk_sep_count(B, n3, lo3, dq3, nnulls, pos, kind, normal, nbr, pair, arc, radius, capture, step, &
                             max_steps, rounds, tol, every, max_points, state, nrounds, coef, width, side, dmin, ends, &
                             length, status, nsteps, offsets, total) bind(c, name="ndsmk_sep_count") result(rc)
      import :: c_ptr, c_int, c_int32_t, c_int64_t, c_double
      type(c_ptr), value :: B, pos, kind, normal, pair, arc, state, nrounds, coef, width, side, dmin, ends, length, &
                            status, nsteps, offsets
      integer(c_int32_t), intent(in) :: n3(3)
      real(c_double), intent(in) :: lo3(3), dq3(3)
      integer(c_int), value :: nnulls, nbr, max_steps, rounds, every
      real(c_double), value :: radius, capture, step, tol
      integer(c_int64_t), value :: max_points
      integer(c_int64_t), intent(out) :: total
      integer(c_int) :: rc
    end function
    function ndsmk_sep_fill(B, n3, lo3, dq3, nnulls, pos, nbr, pair, radius, capture, step, max_steps, rounds, tol, &
                            every, max_points, offsets, points, bpt) bind(c, name="ndsmk_sep_fill") result(rc)
      import :: c_ptr, c_int, c_int32_t, c_int64_t, c_double
      type(c_ptr), value :: B, pos, pair, offsets, points, bpt
      integer(c_int32_t), intent(in) :: n3(3)
      real(c_double), intent(in) :: lo3(3), dq3(3)
      integer(c_int), value :: nnulls, nbr, max_steps, rounds, every
      real(c_double), value :: radius, capture, step, tol
      integer(c_int64_t), value :: max_points
      integer(c_int) :: rc
    end function

    ! ---- the face phase on the device (faces.hip) ----
    function ndsmk_face_offsets(n3, off6, total) bind(c, name="ndsmk_face_offsets") result(rc)
      import :: c_int, c_int32_t, c_int64_t
      integer(c_int32_t), intent(in) :: n3(3)
      integer(c_int64_t), intent(out) :: off6(6), total
      integer(c_int) :: rc
    end function
    function ndsmk_face_extract(B, n3, faces) bind(c, name="ndsmk_face_extract") result(rc)
      import :: c_ptr, c_int, c_int32_t
      type(c_ptr), value :: B, faces
      integer(c_int32_t), intent(in) :: n3(3)
      integer(c_int) :: rc
    end function
    function ndsmk_face_flux(faces, n3, h1h2, d_phi6) bind(c, name="ndsmk_face_flux") result(rc)
      import :: c_ptr, c_int, c_int32_t, c_double
      type(c_ptr), value :: faces, d_phi6
      integer(c_int32_t), intent(in) :: n3(3)
      real(c_double), value :: h1h2
      integer(c_int) :: rc
    end function
    function ndsmk_face_rhs(faces, n3, f, d_phi6, area, rhs) bind(c, name="ndsmk_face_rhs") result(rc)
      import :: c_ptr, c_int, c_int32_t, c_double
      type(c_ptr), value :: faces, d_phi6, rhs
      integer(c_int32_t), intent(in) :: n3(3)
      integer(c_int), value :: f
      real(c_double), value :: area
      integer(c_int) :: rc
    end function
    function ndsmk_face_put(u, n3, f, vals) bind(c, name="ndsmk_face_put") result(rc)
      import :: c_ptr, c_int, c_int32_t
      type(c_ptr), value :: u, vals
      integer(c_int32_t), intent(in) :: n3(3)
      integer(c_int), value :: f
      integer(c_int) :: rc
    end function
    function ndsmk_face_write(u, n3, chi, f, c, fac) bind(c, name="ndsmk_face_write") result(rc)
      import :: c_ptr, c_int, c_int32_t, c_double
      type(c_ptr), value :: u, chi
      integer(c_int32_t), intent(in) :: n3(3)
      integer(c_int), value :: f, c
      real(c_double), value :: fac
      integer(c_int) :: rc
    end function

  end interface

contains

  ! byte offset into a device allocation
  function dptr_offset(base, bytes) result(p)
    type(c_ptr), intent(in) :: base
    integer(c_size_t), intent(in) :: bytes
    type(c_ptr) :: p
    p = transfer(transfer(base, 0_c_intptr_t) + int(bytes, c_intptr_t), p)
  end function

end module ndsmh_iface
