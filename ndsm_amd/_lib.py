"""ctypes binding of libndsm_hip.so (C ABI: include/ndsm_hip.h).

Fails loudly: a missing library raises NdsmHipError at load time and a missing
GPU raises it at the first call that needs the device.  Nothing here computes
on the CPU.
"""
import collections
import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int)


class NdsmHipError(RuntimeError):
    pass


def lib_path():
    # NDSM_HIP_LIB: development override (A/B builds of the same library)
    return os.environ.get("NDSM_HIP_LIB") or os.path.join(HERE, "lib", "libndsm_hip.so")


def load_library(path=None):
    """Load libndsm_hip.so once and declare its prototypes."""
    global _LIB
    if _LIB is not None and path is None:
        return _LIB
    p = path or lib_path()
    if not os.path.exists(p):
        raise NdsmHipError(f"{p} not found - build it with `make -C ndsm_amd` "
                           "(or __graft_entry__.build()); there is no CPU fallback")
    # RTLD_DEEPBIND: the library and its own dependencies (/opt/rocm's libamdhip64, librccl) are
    # searched BEFORE the global scope.  Without it, a process that imported PyTorch first would
    # bind our hip*/nccl* calls to the second ROCm stack torch bundles (torch loads it RTLD_GLOBAL).
    mode = os.RTLD_NOW | os.RTLD_LOCAL | getattr(os, "RTLD_DEEPBIND", 0)
    # multi-process runs (one rank per GPU, RCCL): this pool's host driver does dmabuf IPC only; without the
    # variable RCCL's peer set-up fails with "hipIpcGetMemHandle: invalid argument".  It is read when the HSA
    # runtime comes up, i.e. at the first HIP call below - a caller's own value is left alone.
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    L = ctypes.CDLL(p, mode=mode)
    L.ndsm_vector_solve.restype = ctypes.c_int
    L.ndsm_hip_last_error.argtypes = [ctypes.c_char_p, ctypes.c_int]
    L.ndsm_hip_last_error.restype = None
    L.ndsm_hip_timer_stop.argtypes = [_dp]
    L.ndsm_hip_mg_create.argtypes = [ctypes.c_int, _ip, _dp, _dp, _dp, ctypes.c_char_p, ctypes.c_int, ctypes.c_int,
                                     ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
    L.ndsm_hip_mg_destroy.argtypes = [ctypes.c_void_p]
    L.ndsm_hip_mg_levels.argtypes = [ctypes.c_void_p, ctypes.c_int, _ip]
    L.ndsm_hip_mg_set_ms.argtypes = [ctypes.c_void_p, ctypes.c_int]
    L.ndsm_hip_mg_set_precision.argtypes = [ctypes.c_void_p, ctypes.c_int]
    L.ndsm_hip_mg_upload.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, _dp]
    L.ndsm_hip_mg_download.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, _dp]
    L.ndsm_hip_mg_zero_rhs.argtypes = [ctypes.c_void_p]
    L.ndsm_hip_mg_op.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    L.ndsm_hip_mg_vcycle.argtypes = [ctypes.c_void_p, ctypes.c_int]
    L.ndsm_hip_mg_solve.argtypes = [ctypes.c_void_p, ctypes.c_double, ctypes.c_int, _dp, _ip, _dp, ctypes.c_int]
    L.ndsm_hip_mg_info.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]
    L.ndsm_hip_poisson_solve.argtypes = [ctypes.c_int, _ip, _dp, _dp, _dp, ctypes.c_char_p, _ip, _dp, _dp, _dp, _dp,
                                         ctypes.c_int]
    L.ndsm_hip_dist_unique_id.argtypes = [ctypes.c_char_p]
    L.ndsm_hip_dist_init.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_char_p]
    L.ndsm_hip_slab_plan.argtypes = [_ip, _dp, _dp, _dp, ctypes.c_int, ctypes.c_int, _ip]
    L.ndsm_hip_world_create.argtypes = [_ip, _dp, _dp, _dp, ctypes.c_char_p, ctypes.c_int, ctypes.c_int,
                                        ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                        ctypes.POINTER(ctypes.c_void_p)]
    L.ndsm_hip_world_destroy.argtypes = [ctypes.c_void_p]
    L.ndsm_hip_world_nlocal.argtypes = [ctypes.c_void_p]
    L.ndsm_hip_world_dist_levels.argtypes = [ctypes.c_void_p]
    L.ndsm_hip_world_slab.argtypes = [ctypes.c_void_p, ctypes.c_int, _ip]
    L.ndsm_hip_world_upload.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, _dp, ctypes.c_int, ctypes.c_int]
    L.ndsm_hip_world_download.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, _dp]
    L.ndsm_hip_world_relax.argtypes = [ctypes.c_void_p, ctypes.c_int]
    L.ndsm_hip_world_zero_rhs.argtypes = [ctypes.c_void_p]
    L.ndsm_hip_world_vcycle.argtypes = [ctypes.c_void_p, ctypes.c_int]
    L.ndsm_hip_world_set_precision.argtypes = [ctypes.c_void_p, ctypes.c_int]
    L.ndsm_hip_world_solve.argtypes = [ctypes.c_void_p, ctypes.c_double, ctypes.c_int, _dp, _ip, _dp, ctypes.c_int]
    L.ndsm_hip_vecpot_create.argtypes = [_ip, _dp, _dp, _dp, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
    L.ndsm_hip_vecpot_solve.argtypes = [ctypes.c_void_p, _ip, _dp, _dp, _dp]
    L.ndsm_hip_vecpot_solve_device.argtypes = [ctypes.c_void_p, _ip, _dp, ctypes.c_void_p, ctypes.c_void_p]
    L.ndsm_hip_vecpot_destroy.argtypes = [ctypes.c_void_p]
    L.ndsm_hip_vecpot_solve_field.argtypes = [ctypes.c_void_p, _ip, _dp, _dp, _dp]
    L.ndsm_hip_vecpot_solve_field_device.argtypes = [ctypes.c_void_p, _ip, _dp, ctypes.c_void_p, ctypes.c_void_p]
    L.ndsm_hip_vecpot_helicity.argtypes = [ctypes.c_void_p, _ip, _dp, _dp, _dp, _dp, _dp, _dp]
    L.ndsm_hip_vecpot_helicity_device.argtypes = [ctypes.c_void_p, _ip, _dp, ctypes.c_void_p, ctypes.c_void_p,
                                                  ctypes.c_void_p, ctypes.c_void_p, _dp]
    L.ndsm_hip_vecpot_project.argtypes = [ctypes.c_void_p, _ip, _dp, _dp, _dp, _dp]
    L.ndsm_hip_vecpot_project_device.argtypes = [ctypes.c_void_p, _ip, _dp, ctypes.c_void_p, ctypes.c_void_p,
                                                 _dp]
    L.ndsm_hip_vecpot_devore.argtypes = [ctypes.c_void_p, _dp, _dp, _dp, _dp, _dp]
    L.ndsm_hip_vecpot_devore_device.argtypes = [ctypes.c_void_p] + [ctypes.c_void_p] * 4 + [_dp]
    _tr = [ctypes.c_int, ctypes.c_void_p, ctypes.c_double, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 5
    L.ndsm_hip_vecpot_trace.argtypes = [ctypes.c_void_p] * 3 + _tr
    L.ndsm_hip_vecpot_trace_device.argtypes = [ctypes.c_void_p] * 3 + _tr
    _am = [ctypes.c_void_p] * 3 + [ctypes.c_int, ctypes.c_double, ctypes.c_int] + [ctypes.c_void_p] * 2
    L.ndsm_hip_vecpot_alpha_map.argtypes = _am
    L.ndsm_hip_vecpot_alpha_map_device.argtypes = _am
    L.ndsm_hip_vecpot_solve_current.argtypes = [ctypes.c_void_p, _ip, _dp, _dp, _dp, _dp]
    L.ndsm_hip_vecpot_solve_current_device.argtypes = [ctypes.c_void_p, _ip, _dp] + [ctypes.c_void_p] * 3
    _nl = ([ctypes.c_void_p, _ip, _dp] + [ctypes.c_void_p] * 2 + [ctypes.c_int] * 3 + [ctypes.c_double] * 2 +
           [ctypes.c_int] + [ctypes.c_void_p] * 3 + [_dp, _ip])
    L.ndsm_hip_vecpot_nlfff.argtypes = _nl
    L.ndsm_hip_vecpot_nlfff_device.argtypes = _nl
    _op = ([ctypes.c_void_p, _ip, _dp] + [ctypes.c_void_p] * 2 + [ctypes.c_int] * 3 + [ctypes.c_double] * 3 +
           [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p])
    L.ndsm_hip_vecpot_optimize.argtypes = _op
    L.ndsm_hip_vecpot_optimize_device.argtypes = _op
    _ob = ([ctypes.c_void_p, _ip, _dp] + [ctypes.c_void_p] * 4 + [ctypes.c_double] + [ctypes.c_int] * 4 +
           [ctypes.c_double] * 3 + [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p])
    L.ndsm_hip_vecpot_optimize_obs.argtypes = _ob
    L.ndsm_hip_vecpot_optimize_obs_device.argtypes = _ob
    _oc = ([ctypes.c_void_p, ctypes.c_int, _ip, _dp] + [ctypes.c_void_p] * 2 + [ctypes.c_int, ctypes.c_void_p,
           ctypes.c_int, ctypes.c_double] + [ctypes.c_void_p] * 3 + [ctypes.c_int, ctypes.c_void_p])
    L.ndsm_hip_vecpot_optimize_cascade.argtypes = _oc
    L.ndsm_hip_vecpot_optimize_cascade_device.argtypes = _oc
    _rs = [_ip, _ip, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    L.ndsm_hip_resample.argtypes = _rs
    L.ndsm_hip_resample_device.argtypes = _rs
    _rw = [_ip, _ip, ctypes.c_int] + [ctypes.c_void_p] * 4
    L.ndsm_hip_resample_weighted.argtypes = _rw
    L.ndsm_hip_resample_weighted_device.argtypes = _rw
    _gs = [_ip, _dp, _dp, ctypes.c_double, ctypes.c_void_p]           # the source: nsrc, xs, ys, zs, bz
    L.ndsm_hip_green_points.argtypes = _gs + [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    L.ndsm_hip_green_points_device.argtypes = _gs + [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    L.ndsm_hip_green_box.argtypes = _gs + [_ip, _dp, _dp, _dp, ctypes.c_int, ctypes.c_void_p]
    L.ndsm_hip_green_box_device.argtypes = _gs + [_ip, _dp, _dp, _dp, ctypes.c_int, ctypes.c_void_p]
    _ls = _gs + [ctypes.c_double]                                      # the same and alpha
    L.ndsm_hip_lfff_points.argtypes = _ls + [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    L.ndsm_hip_lfff_points_device.argtypes = _ls + [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    L.ndsm_hip_lfff_box.argtypes = _ls + [_ip, _dp, _dp, _dp, ctypes.c_int, ctypes.c_void_p]
    L.ndsm_hip_lfff_box_device.argtypes = _ls + [_ip, _dp, _dp, _dp, ctypes.c_int, ctypes.c_void_p]
    L.ndsm_hip_vecpot_open.argtypes = [ctypes.c_void_p, _ip, _dp] + _gs + [ctypes.c_void_p] * 2
    L.ndsm_hip_vecpot_open_device.argtypes = [ctypes.c_void_p, _ip, _dp] + _gs + [ctypes.c_void_p] * 2
    _obc = ([ctypes.c_void_p, ctypes.c_int, _ip, _dp] + [ctypes.c_void_p] * 5 + [ctypes.c_int, ctypes.c_int,
            ctypes.c_void_p, ctypes.c_int, ctypes.c_double] + [ctypes.c_void_p] * 3 + [ctypes.c_int, ctypes.c_void_p])
    L.ndsm_hip_vecpot_optimize_obs_cascade.argtypes = _obc
    L.ndsm_hip_vecpot_optimize_obs_cascade_device.argtypes = _obc
    _pp = ([ctypes.c_void_p] * 4 + [ctypes.c_int] * 2 + [ctypes.c_double] * 3 +
           [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p])
    L.ndsm_hip_vecpot_preprocess.argtypes = _pp
    L.ndsm_hip_vecpot_preprocess_device.argtypes = _pp
    _pa = ([ctypes.c_int, ctypes.c_void_p, ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int64] +
           [ctypes.c_void_p] * 11)
    L.ndsm_hip_vecpot_paths.argtypes = [ctypes.c_void_p] * 3 + _pa
    L.ndsm_hip_vecpot_paths_device.argtypes = [ctypes.c_void_p] * 3 + _pa
    _sq = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_double, ctypes.c_int] + [ctypes.c_void_p] * 6
    L.ndsm_hip_vecpot_squash.argtypes = [ctypes.c_void_p] * 3 + _sq
    L.ndsm_hip_vecpot_squash_device.argtypes = [ctypes.c_void_p] * 3 + _sq
    L.ndsm_hip_vecpot_squash_perp.argtypes = [ctypes.c_void_p] * 3 + _sq + [ctypes.c_void_p]
    L.ndsm_hip_vecpot_squash_perp_device.argtypes = [ctypes.c_void_p] * 3 + _sq + [ctypes.c_void_p]
    _nu = [ctypes.c_void_p] * 2 + [ctypes.c_int] + [ctypes.c_void_p] * 8
    L.ndsm_hip_vecpot_nulls.argtypes = _nu
    L.ndsm_hip_vecpot_nulls_device.argtypes = _nu
    _di = [ctypes.c_void_p] * 2 + [ctypes.c_int, ctypes.c_int64] + [ctypes.c_void_p] * 7
    L.ndsm_hip_vecpot_dips.argtypes = _di
    L.ndsm_hip_vecpot_dips_device.argtypes = _di
    _pm = [_ip, _dp, _dp]                                              # the mesh of a plane: nsrc, xs, ys
    _ff = _pm + [ctypes.c_void_p] * 2 + [ctypes.c_double, ctypes.c_int, ctypes.c_double] + [ctypes.c_void_p] * 3
    L.ndsm_hip_flow_fit.argtypes = _ff
    L.ndsm_hip_flow_fit_device.argtypes = _ff
    L.ndsm_hip_green_ap_points.argtypes = _pm + [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    L.ndsm_hip_green_ap_points_device.argtypes = _pm + [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    L.ndsm_hip_green_ap_plane.argtypes = _pm + [ctypes.c_void_p] * 2
    L.ndsm_hip_green_ap_plane_device.argtypes = _pm + [ctypes.c_void_p] * 2
    L.ndsm_hip_flow_flux.argtypes = _pm + [ctypes.c_void_p] * 4 + [_dp]
    L.ndsm_hip_flow_flux_device.argtypes = _pm + [ctypes.c_void_p] * 4 + [_dp]
    _pt = _pm + [ctypes.c_void_p, ctypes.c_double, ctypes.c_int64] + [ctypes.c_void_p] * 8
    L.ndsm_hip_partition.argtypes = _pt
    L.ndsm_hip_partition_device.argtypes = _pt
    _cn = ([ctypes.c_void_p] * 3 + [ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_int64] +
           [ctypes.c_void_p] * 9)
    L.ndsm_hip_vecpot_connect.argtypes = _cn
    L.ndsm_hip_vecpot_connect_device.argtypes = _cn
    _sk = ([ctypes.c_void_p] * 2 + [ctypes.c_int] + [ctypes.c_void_p] * 2 + [ctypes.c_int, ctypes.c_void_p] +
           [ctypes.c_double] * 3 + [ctypes.c_int, ctypes.c_int, ctypes.c_int64] + [ctypes.c_void_p] * 13)
    L.ndsm_hip_vecpot_skeleton.argtypes = _sk
    L.ndsm_hip_vecpot_skeleton_device.argtypes = _sk
    _se = ([ctypes.c_void_p] * 2 + [ctypes.c_int] + [ctypes.c_void_p] * 3 + [ctypes.c_int] + [ctypes.c_void_p] * 2 +
           [ctypes.c_double] * 3 + [ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_int64] +
           [ctypes.c_void_p] * 14)
    L.ndsm_hip_vecpot_separators.argtypes = _se
    L.ndsm_hip_vecpot_separators_device.argtypes = _se
    L.ndsm_hip_device_alloc.argtypes = [ctypes.c_size_t, ctypes.POINTER(ctypes.c_void_p)]
    L.ndsm_hip_device_free.argtypes = [ctypes.c_void_p]
    L.ndsm_hip_memcpy_h2d.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    L.ndsm_hip_memcpy_d2h.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    L.ndsm_hip_debug_relax_plan.argtypes = [ctypes.c_int, _ip, ctypes.POINTER(ctypes.c_int64),
                                            ctypes.POINTER(ctypes.c_int64), ctypes.c_int, _ip]
    L.ndsm_hip_debug_zero_guess.argtypes = [ctypes.c_int]
    L.ndsm_hip_debug_u_declared_zero.argtypes = [ctypes.c_void_p, ctypes.c_int]
    L.ndsm_hip_debug_transfer_cfg.argtypes = [ctypes.c_longlong, ctypes.c_longlong, ctypes.c_int, ctypes.c_int]
    L.ndsm_hip_debug_transfer_form.argtypes = [ctypes.c_void_p, ctypes.c_int, _ip]
    if path is None:
        _LIB = L
    return L


def bound_libs(L=None):
    """paths of the HIP and RCCL shared objects our calls are bound to"""
    L = L or load_library()
    buf = ctypes.create_string_buffer(1024)
    L.ndsm_hip_bound_libs(buf, 1024)
    return dict(kv.split("=", 1) for kv in buf.value.decode().split(";"))


def last_error(L=None):
    L = L or load_library()
    buf = ctypes.create_string_buffer(512)
    L.ndsm_hip_last_error(buf, 512)
    return buf.value.decode(errors="replace")


def _check(rc, what, L=None):
    if rc != 0:
        raise NdsmHipError(f"{what} failed with code {rc}: {last_error(L)}")


def transfer_cfg(restrict_min_points=-1, prolong_min_points=-1, rs_variant=-1, rs_chunk=-1, L=None):
    """development hook (ndsm_hip_debug_transfer_cfg): the level sizes from which the streamed restriction (read when
    a solver is created) and the tiled prolongation run, the streamed restriction's form (5, 8, 10) and its coarse
    planes per chunk; negative = the built-in choice, no arguments = all four built in"""
    L = L or load_library()
    _check(L.ndsm_hip_debug_transfer_cfg(int(restrict_min_points), int(prolong_min_points), int(rs_variant),
                                         int(rs_chunk)), "ndsm_hip_debug_transfer_cfg", L)


def _d(a):
    return a.ctypes.data_as(_dp)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


# ops / buffers of ndsm_hip_mg_op, ndsm_hip_mg_upload (ndsmh_mg.f90)
BUF_U, BUF_RHS, BUF_R, BUF_UALT = 0, 1, 2, 3   # BUF_UALT: the partner array of u (tests)
OP_RELAX, OP_RESIDUAL, OP_RESTRICT, OP_PROLONG, OP_EXACT, OP_RELAX_COLOR, OP_RELAX_FUSED, _OP_RETIRED_7, OP_RELAX_RES, OP_RELAX_RES_FUSED = range(10)
OP_ZERO_U, OP_DESCEND = 11, 12   # tests of the zero first guess (ndsm_hip_debug_zero_guess in include/ndsm_hip.h)


class MGSolver:
    """Persistent device-resident multigrid solver (additive API).

    nshape: Fortran order [nx, ny(, nz)]; arrays are numpy C order (nz, ny, nx).
    bcs: 2*ndim letters, lower faces then upper faces, 'D' or 'N'.
    """

    def __init__(self, nshape, mesh, bcs, ngrids=0, ms=5, ex_tol=1e-13, du_max=True, nmax_exact=10000, lib=None):
        self.L = lib or load_library()
        self.ndim = len(nshape)
        ns = np.asarray(nshape, dtype=np.intc)
        m = [_f64(v) for v in mesh]
        while len(m) < 3:
            m.append(np.zeros(2))
        self.h = ctypes.c_void_p()
        rc = self.L.ndsm_hip_mg_create(self.ndim, ns.ctypes.data_as(_ip), _d(m[0]), _d(m[1]), _d(m[2]),
                                       bcs.encode(), int(ngrids), int(ms), float(ex_tol), 1 if du_max else 0,
                                       int(nmax_exact), ctypes.byref(self.h))
        _check(rc, "ndsm_hip_mg_create", self.L)
        shp = np.zeros((32, 3), dtype=np.intc)
        self.ngrids = self.L.ndsm_hip_mg_levels(self.h, 32, shp.ctypes.data_as(_ip))
        self.shapes = [tuple(int(v) for v in shp[l, :self.ndim]) for l in range(self.ngrids)]  # Fortran order

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            self.L.ndsm_hip_mg_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _npshape(self, level):
        return tuple(self.shapes[level - 1][::-1])

    def upload(self, level, which, arr):
        a = _f64(arr)
        assert a.shape == self._npshape(level if which != BUF_R else 1), (a.shape, self._npshape(level))
        _check(self.L.ndsm_hip_mg_upload(self.h, level, which, _d(a)), "upload", self.L)

    def download(self, level, which, shape_level=None):
        out = np.empty(self._npshape(shape_level or (level if which != BUF_R else 1)))
        if which == BUF_R and shape_level:
            full = np.empty(self._npshape(1))
            _check(self.L.ndsm_hip_mg_download(self.h, 1, which, _d(full)), "download", self.L)
            return full.ravel()[:out.size].reshape(out.shape).copy()
        _check(self.L.ndsm_hip_mg_download(self.h, level, which, _d(out)), "download", self.L)
        return out

    def zero_rhs(self):
        """rhs(1) == 0: the Laplace case of the vector potential; kernels then skip the rhs read"""
        _check(self.L.ndsm_hip_mg_zero_rhs(self.h), "zero_rhs", self.L)

    def set_precision(self, mode):
        """0 fp64, 1 mixed where level 1 is large, 2 mixed wherever the fp32 kernels apply;
        returns True if solve() will run in mixed precision"""
        rc = self.L.ndsm_hip_mg_set_precision(self.h, int(mode))
        if rc < 0:
            raise NdsmHipError(f"bad precision mode {mode}")
        return rc == 1

    def transfer_form(self, level):
        """(restriction form, kc, nkc, tiled prolongation) of the transfers level -> level + 1 as the launchers
        decide them now (ndsm_hip_debug_transfer_form): form 0 = gather, 5 / 8 / 10 = streamed"""
        out = np.zeros(4, dtype=np.intc)
        _check(self.L.ndsm_hip_debug_transfer_form(self.h, int(level), out.ctypes.data_as(_ip)), "transfer_form",
               self.L)
        return tuple(int(v) for v in out)

    def op(self, op, level, count=1):
        _check(self.L.ndsm_hip_mg_op(self.h, op, level, count), f"op {op}", self.L)

    def vcycle(self, n=1):
        _check(self.L.ndsm_hip_mg_vcycle(self.h, n), "vcycle", self.L)

    def solve(self, vc_tol=1e-10, nmax=1024, hist_len=0):
        du = ctypes.c_double(0)
        nc = ctypes.c_int(0)
        hist = np.zeros(max(hist_len, 1))
        ierr = self.L.ndsm_hip_mg_solve(self.h, float(vc_tol), int(nmax), ctypes.byref(du), ctypes.byref(nc), _d(hist),
                                        int(hist_len))
        if ierr >= 9000:
            _check(ierr, "ndsm_hip_mg_solve", self.L)
        return ierr, du.value, nc.value, hist[:min(hist_len, nc.value)].copy()

    def info(self):
        a, b = ctypes.c_int64(0), ctypes.c_int64(0)
        _check(self.L.ndsm_hip_mg_info(self.h, ctypes.byref(a), ctypes.byref(b)), "info", self.L)
        return a.value, b.value

    def sync(self):
        _check(self.L.ndsm_hip_sync(), "sync", self.L)

    def timed(self, fn):
        """Run fn() between two HIP events on the library stream; returns ms."""
        _check(self.L.ndsm_hip_timer_start(), "timer_start", self.L)
        fn()
        ms = ctypes.c_double(0)
        _check(self.L.ndsm_hip_timer_stop(ctypes.byref(ms)), "timer_stop", self.L)
        return ms.value


class VecPot:
    """Persistent vector-potential solver (additive): the grid hierarchies, transfer tables
    and device arrays are built once per (shape, mesh) and reused by every solve().

    x, y, z: mesh vectors; shape of the fields: numpy (3, nz, ny, nx)."""

    def __init__(self, x, y, z, ngrids=0, lib=None):
        self.L = lib or load_library()
        self.x, self.y, self.z = _f64(x), _f64(y), _f64(z)
        self.nshape4 = np.array([len(self.x), len(self.y), len(self.z), 3], dtype=np.intc)
        self.ngrids = int(ngrids)
        self.h = ctypes.c_void_p()
        self.last_projection = None
        rc = self.L.ndsm_hip_vecpot_create(self.nshape4.ctypes.data_as(_ip), _d(self.x), _d(self.y), _d(self.z),
                                           self.ngrids, ctypes.byref(self.h))
        _check(rc, "ndsm_hip_vecpot_create", self.L)

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            self.L.ndsm_hip_vecpot_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _options(self, niterex_max, ncycles_max, ex_tol, vc_tol, ms, mean, mixed_precision, flxcrl):
        L = self.L
        ioptc = np.zeros(16, dtype=np.intc)
        ropt = np.zeros(16)
        ioptc[L.get_iopt_ms()] = ms
        ioptc[L.get_iopt_ncycles()] = ncycles_max
        ioptc[L.get_iopt_iopt_nmaxex()] = niterex_max
        ioptc[L.get_iopt_dumax()] = 0 if mean else 1
        ioptc[L.get_iopt_ngrids()] = self.ngrids
        ioptc[L.get_iopt_prec()] = int(mixed_precision)
        ioptc[4] = 1 if flxcrl else 0          # IOPT_FLXCRL (ndsm_vector_potential.f90:44; no getter in the reference)
        ropt[L.get_ropt_vtol()] = vc_tol
        ropt[L.get_ropt_ctol()] = ex_tol
        return ioptc, ropt

    def solve(self, b, a_init=None, niterex_max=10000, ncycles_max=1024, ex_tol=1e-13, vc_tol=1e-10, ms=5, mean=False,
              mixed_precision=False, flxcrl=False, device=False):
        """b: (3,nz,ny,nx); returns (ierr, A, B) like ndsm.vector_potential.  device=True: the fields are
        staged in device memory first and the device-resident entry point runs (tests of that path)."""
        ioptc, ropt = self._options(niterex_max, ncycles_max, ex_tol, vc_tol, ms, mean, mixed_precision, flxcrl)
        shape = tuple(int(v) for v in self.nshape4[::-1])
        B = _f64(b).reshape(-1).copy()
        assert B.size == int(np.prod(shape)), (b.shape, shape)
        A = np.zeros(B.size) if a_init is None else _f64(a_init).reshape(-1).copy()
        if not device:
            ierr = self.L.ndsm_hip_vecpot_solve(self.h, ioptc.ctypes.data_as(_ip), _d(ropt), _d(A), _d(B))
        else:
            dA, dB = ctypes.c_void_p(), ctypes.c_void_p()
            _check(self.L.ndsm_hip_device_alloc(A.nbytes, ctypes.byref(dA)), "device_alloc", self.L)
            _check(self.L.ndsm_hip_device_alloc(B.nbytes, ctypes.byref(dB)), "device_alloc", self.L)
            try:
                _check(self.L.ndsm_hip_memcpy_h2d(dA, A.ctypes.data, A.nbytes), "h2d", self.L)
                _check(self.L.ndsm_hip_memcpy_h2d(dB, B.ctypes.data, B.nbytes), "h2d", self.L)
                ierr = self.L.ndsm_hip_vecpot_solve_device(self.h, ioptc.ctypes.data_as(_ip), _d(ropt), dA, dB)
                _check(self.L.ndsm_hip_memcpy_d2h(A.ctypes.data, dA, A.nbytes), "d2h", self.L)
                _check(self.L.ndsm_hip_memcpy_d2h(B.ctypes.data, dB, B.nbytes), "d2h", self.L)
            finally:
                self.L.ndsm_hip_device_free(dA)
                self.L.ndsm_hip_device_free(dB)
        if ierr >= 9000:
            _check(ierr, "ndsm_hip_vecpot_solve", self.L)
        self.last_ioptc, self.last_ropt = ioptc, ropt
        return ierr, A.reshape(shape), B.reshape(shape)

    def solve_open(self, bz, xs=None, ys=None, zs=None, a_init=None, niterex_max=10000, ncycles_max=1024,
                   ex_tol=1e-13, vc_tol=1e-10, ms=5, mean=False, mixed_precision=False, flxcrl=False, device=False):
        """The open-box potential field of the magnetogram bz (nsy,nsx) on the mesh xs, ys at height zs (defaults:
        the handle's x, y and z[0]): the Green's-function field of the half space above bz on the six faces, then
        solve() - in one call, bit for bit magnetogram_field() followed by solve(), and no field crosses PCIe in
        between (semantics: include/ndsm_hip.h, ndsm_hip_vecpot_open).  Returns (ierr, A, B) as solve()."""
        ns2, qx, qy, zs_, S = _green_source(self.x, self.y, self.z, bz, xs, ys, zs)
        shape = tuple(int(v) for v in self.nshape4[::-1])
        n = int(np.prod(shape))
        A = np.zeros(n) if a_init is None else self._field_arg(a_init, "solve_open")
        B = np.zeros(n)
        ioptc, ropt = self._options(niterex_max, ncycles_max, ex_tol, vc_tol, ms, mean, mixed_precision, flxcrl)
        head = (self.h, ioptc.ctypes.data_as(_ip), _d(ropt), ns2.ctypes.data_as(_ip), _d(qx), _d(qy), zs_)
        if not device:
            ierr = self.L.ndsm_hip_vecpot_open(*head, S.ctypes.data, A.ctypes.data, B.ctypes.data)
        else:
            ierr = self._on_device([S, A, B], lambda dS, dA, dB: self.L.ndsm_hip_vecpot_open_device(*head, dS, dA, dB))
        if ierr >= 9000:
            _check(ierr, "ndsm_hip_vecpot_open", self.L)
        self.last_ioptc, self.last_ropt = ioptc, ropt
        return ierr, A.reshape(shape), B.reshape(shape)

    def _field_arg(self, b, what):
        """b as a flat float64 copy; a shape other than (3, nz, ny, nx) is an argument error (9002)"""
        shape = tuple(int(v) for v in self.nshape4[::-1])
        a = np.asarray(b)
        if a.shape != shape:
            raise NdsmHipError(f"{what}: field of shape {a.shape}, the handle's grid needs {shape} (code 9002)")
        return _f64(a).reshape(-1).copy()

    def _on_device(self, host_arrays, call):
        """stage host_arrays in device memory, run call(*device pointers), copy every array back"""
        return _staged(self.L, host_arrays, call)

    def _entry(self, name, args, device, who=None):
        """One call of an entry that takes arrays: L.<name>(h, *args) on host arrays, or (device) L.<name>_device with
        the arrays staged in device memory first and copied back.  args in the order of the C prototype: a numpy
        array is passed by its address (host) or staged (device) - the same array twice is staged once -, anything
        else (a scalar, None, an address that holds in both modes, a pointer to an array already on the device) goes
        through as it is.  Raises NdsmHipError unless the entry returns 0, under the name of the entry that ran or
        `who`."""
        def host(a):
            return isinstance(a, np.ndarray)
        if not device:
            ierr = getattr(self.L, name)(self.h, *[a.ctypes.data if host(a) else a for a in args])
        else:
            name += "_device"
            staged = list({id(a): a for a in args if host(a)}.values())

            def call(*ptrs):
                dev = {id(a): p for a, p in zip(staged, ptrs)}
                return getattr(self.L, name)(self.h, *[dev[id(a)] if host(a) else a for a in args])
            ierr = self._on_device(staged, call)
        _check(ierr, who or name, self.L)

    def solve_field(self, b, a_init=None, niterex_max=10000, ncycles_max=1024, ex_tol=1e-13, vc_tol=1e-10, ms=5,
                    mean=False, mixed_precision=False, flxcrl=False, device=False):
        """Vector potential of the whole field b (3,nz,ny,nx), curl b != 0 allowed: the same gauge and tangential
        boundary values as solve()'s potential-field A_p.  Returns (ierr, A, B_rec), B_rec = curl A + the
        flux-balance fields; ierr 0 when every solve reached vc_tol, else 1.  device=True: the arrays are staged
        in device memory and the device-resident entry point runs."""
        ioptc, ropt = self._options(niterex_max, ncycles_max, ex_tol, vc_tol, ms, mean, mixed_precision, flxcrl)
        shape = tuple(int(v) for v in self.nshape4[::-1])
        B = self._field_arg(b, "solve_field")
        A = np.zeros(B.size) if a_init is None else self._field_arg(a_init, "solve_field")
        if not device:
            ierr = self.L.ndsm_hip_vecpot_solve_field(self.h, ioptc.ctypes.data_as(_ip), _d(ropt), _d(A), _d(B))
        else:
            ierr = self._on_device([A, B], lambda dA, dB: self.L.ndsm_hip_vecpot_solve_field_device(
                self.h, ioptc.ctypes.data_as(_ip), _d(ropt), dA, dB))
        if ierr >= 9000:
            _check(ierr, "ndsm_hip_vecpot_solve_field", self.L)
        self.last_ioptc, self.last_ropt = ioptc, ropt
        return ierr, A.reshape(shape), B.reshape(shape)

    def helicity(self, b, niterex_max=10000, ncycles_max=1024, ex_tol=1e-13, vc_tol=1e-10, ms=5, mean=False,
                 mixed_precision=False, flxcrl=False, device=False, return_fields=False, project=False,
                 gauge="coulomb"):
        """Relative magnetic helicity of b (3,nz,ny,nx) against the potential field of its B.n, in one call: the
        face phase once, the potential and the field 3-D solves, one deterministic reduction on the device.
        Returns a Helicity tuple (no 4 pi / mu0 factors; trapezoid weights): ierr, H_R (Finn-Antonsen),
        H_J = sum w (A - A_p).(B - B_p), E, E_p, E_free = E - E_p, recon_max / recon_rms of |B_rec - b|,
        divB_max, divA_max; with return_fields also A, A_p, B_p (else None).
        project=True: a copy of b is made solenoidal first (project(), same options) and the helicity is that of
        the projected field; ierr is the larger of the two, the Projection is kept as self.last_projection.
        gauge: "coulomb" (the above), "devore" (A_z = 0: b staged on the device, the potential solve on a copy
        gives B_p - the bits of solve() -, then devore_device; no field solves; B_rec = curl_h A, divA_max the
        gauge's divergence; ierr 1 when a solve of the potential field missed vc_tol) or "both" (helicity_device,
        then devore_device on the same device B and B_p: one potential solve; returns (coulomb, devore))."""
        if gauge not in ("coulomb", "devore", "both"):
            raise ValueError(f"gauge must be 'coulomb', 'devore' or 'both', not {gauge!r}")
        B = self._field_arg(b, "helicity")
        ierr_p = 0
        if project:
            pr = self.project(B.reshape(tuple(int(v) for v in self.nshape4[::-1])), niterex_max=niterex_max,
                              ncycles_max=ncycles_max, ex_tol=ex_tol, vc_tol=vc_tol, ms=ms, mean=mean, device=device)
            ierr_p = pr.ierr
            B = pr.B.reshape(-1).copy()
        ioptc, ropt = self._options(niterex_max, ncycles_max, ex_tol, vc_tol, ms, mean, mixed_precision, flxcrl)
        if gauge != "coulomb":
            return self._devore_chain(B, ioptc, ropt, gauge == "both", return_fields, ierr_p)
        shape = tuple(int(v) for v in self.nshape4[::-1])
        A, Ap, Bp = np.empty(B.size), np.empty(B.size), np.empty(B.size)
        out = np.zeros(8)
        if not device:
            ierr = self.L.ndsm_hip_vecpot_helicity(self.h, ioptc.ctypes.data_as(_ip), _d(ropt), _d(B), _d(A), _d(Ap),
                                                   _d(Bp), _d(out))
        else:
            ierr = self._on_device([B, A, Ap, Bp], lambda dB, dA, dAp, dBp: self.L.ndsm_hip_vecpot_helicity_device(
                self.h, ioptc.ctypes.data_as(_ip), _d(ropt), dB, dA, dAp, dBp, _d(out)))
        if ierr >= 9000:
            _check(ierr, "ndsm_hip_vecpot_helicity", self.L)
        self.last_ioptc, self.last_ropt = ioptc, ropt
        f = (A.reshape(shape), Ap.reshape(shape), Bp.reshape(shape)) if return_fields else (None, None, None)
        return _helicity_tuple(max(ierr, ierr_p), out, *f)

    def _devore_chain(self, B, ioptc, ropt, both, return_fields, ierr_p, after=None):
        """helicity(gauge="devore" / "both") on the device: B (flat) goes up once into two arrays; the potential
        field B_p comes from ndsm_hip_vecpot_solve_device on the copy (both: ndsm_hip_vecpot_helicity_device, the
        same B_p) and stays there for ndsm_hip_vecpot_devore_device.  Only the results come home.  after(d): called
        with the device arrays (B, Bp, A, Ap) while they are still resident."""
        L = self.L
        shape = tuple(int(v) for v in self.nshape4[::-1])
        names = ("B", "Bp", "A", "Ap") + (("Ac", "Apc") if both else ())
        d = {}
        out_c, out_d = np.zeros(8), np.zeros(8)
        try:
            for k in names:
                d[k] = ctypes.c_void_p()
                _check(L.ndsm_hip_device_alloc(B.nbytes, ctypes.byref(d[k])), "device_alloc", L)
            _check(L.ndsm_hip_memcpy_h2d(d["B"], B.ctypes.data, B.nbytes), "h2d", L)
            if both:
                ierr_s = L.ndsm_hip_vecpot_helicity_device(self.h, ioptc.ctypes.data_as(_ip), _d(ropt), d["B"],
                                                           d["Ac"], d["Apc"], d["Bp"], _d(out_c))
                if ierr_s >= 9000:
                    _check(ierr_s, "ndsm_hip_vecpot_helicity_device", L)
            else:
                # the copy of B becomes B_p; A: a zero initial guess in (its A_p out is not used)
                _check(L.ndsm_hip_memcpy_h2d(d["Bp"], B.ctypes.data, B.nbytes), "h2d", L)
                zero = np.zeros(B.size)
                _check(L.ndsm_hip_memcpy_h2d(d["A"], zero.ctypes.data, zero.nbytes), "h2d", L)
                ierr_s = L.ndsm_hip_vecpot_solve_device(self.h, ioptc.ctypes.data_as(_ip), _d(ropt), d["A"], d["Bp"])
                if ierr_s >= 9000:
                    _check(ierr_s, "ndsm_hip_vecpot_solve_device", L)
                ierr_s = 1 if ierr_s != 0 or ioptc[L.get_iopt_fail3d()] != 0 else 0
            self.last_ioptc, self.last_ropt = ioptc, ropt
            _check(L.ndsm_hip_vecpot_devore_device(self.h, d["B"], d["Bp"], d["A"], d["Ap"], _d(out_d)),
                   "ndsm_hip_vecpot_devore_device", L)
            if after is not None:
                after(d)
            host = {}
            for k in (names[1:] if return_fields else ()):
                host[k] = np.empty(B.size)
                _check(L.ndsm_hip_memcpy_d2h(host[k].ctypes.data, d[k], B.nbytes), "d2h", L)
        finally:
            for p in d.values():
                L.ndsm_hip_device_free(p)
        ierr = int(max(ierr_s, ierr_p))
        f = {k: v.reshape(shape) for k, v in host.items()}
        dv = _helicity_tuple(ierr, out_d, f.get("A"), f.get("Ap"), f.get("Bp"))
        if not both:
            return dv
        return _helicity_tuple(ierr, out_c, f.get("Ac"), f.get("Apc"), f.get("Bp")), dv

    def devore(self, b, bp, device=False):
        """Vector potentials of b and bp (3,nz,ny,nx) in the DeVore gauge A_z = 0, and the helicity of b against
        bp with them: no solve.  bp is any field whose B.n matches b's (solve()'s potential field, or the
        caller's own).  A: trapezoid integral of b up from the base plane (b_x, b_y of B_z(z0)); A_p: of bp down
        from A's top plane, so n x A_p = n x A on the top face exactly.  Returns a Helicity tuple with A, A_p
        (always) and B_p = bp; B_rec = curl_h A, divA_max = max |div_h A| is the gauge's divergence, ierr 0.
        device=True: the arrays are staged in device memory and the device-resident entry point runs."""
        shape = tuple(int(v) for v in self.nshape4[::-1])
        B = self._field_arg(b, "devore")
        Bp = self._field_arg(bp, "devore")
        A, Ap = np.empty(B.size), np.empty(B.size)
        out = np.zeros(8)
        if not device:
            ierr = self.L.ndsm_hip_vecpot_devore(self.h, _d(B), _d(Bp), _d(A), _d(Ap), _d(out))
        else:
            ierr = self._on_device([B, Bp, A, Ap], lambda dB, dBp, dA, dAp: self.L.ndsm_hip_vecpot_devore_device(
                self.h, dB, dBp, dA, dAp, _d(out)))
        _check(ierr, "ndsm_hip_vecpot_devore", self.L)
        return _helicity_tuple(0, out, A.reshape(shape), Ap.reshape(shape), Bp.reshape(shape))

    def trace(self, b, seeds, g=None, step=0.5, max_steps=None, direction="both", device=False):
        """Field lines of b (3,nz,ny,nx) through seeds (nseeds,3; x, y, z in physical coordinates) and the line
        integral of g (3,nz,ny,nx; None: no integral, zeros) along them, on the device (semantics:
        include/ndsm_hip.h, ndsm_hip_vecpot_trace).  Arc-length RK4 with the fixed step ds = step * min(h),
        trilinear interpolation; a line ends on a face of the box (the exit step is shortened so that it ends on
        the face), at a null of b, or after max_steps steps (None: default_max_steps(step) = ceil(4 (nx + ny +
        nz) / step), about four box crossings; at most 2**24).  direction: "forward" (along b), "backward" or
        "both".  Returns a FieldLines tuple: ends (ndir,nseeds,3), length, integral (ndir,nseeds), status, nsteps
        (ndir,nseeds; int32, status one of the TRACE_* codes), flh; ndir = 2 for "both" (row 0 forward, row 1
        backward), else 1.  A backward line's integral is that of g.dl taken in the direction of b, so flh =
        integral[0] + integral[1] is the integral of g.dl along the whole line through each seed from the foot
        where b enters the box to the foot where it leaves - with g = A the field-line helicity; flh is None for
        a single direction.  device=True: the arrays are staged in device memory and the device-resident entry
        point runs."""
        direction, step, max_steps = self._trace_args(step, max_steps, direction)
        B = self._field_arg(b, "trace")
        G = None if g is None else self._field_arg(g, "trace")
        S = self._seeds_arg(seeds)
        out = _trace_outputs(len(S), direction)
        if len(S) == 0:
            return _field_lines(out, direction)
        # (an error of the device entry has always been reported under the host entry's name here)
        self._entry("ndsm_hip_vecpot_trace", [B, G, len(S), S, step, max_steps, direction, *out], device,
                    who="ndsm_hip_vecpot_trace")
        return _field_lines(out, direction)

    def _alpha0_arg(self, alpha0, what):
        """alpha0 as a flat float64 copy; a shape other than (ny, nx) is an argument error (9002)"""
        shape = (int(self.nshape4[1]), int(self.nshape4[0]))
        a = np.asarray(alpha0)
        if a.shape != shape:
            raise NdsmHipError(f"{what}: alpha0 of shape {a.shape}, the handle's lower face needs {shape} (code 9002)")
        return _f64(a).reshape(-1).copy()

    def alpha_map(self, b, alpha0, polarity=1, step=0.5, max_steps=None, device=False):
        """alpha0 (ny,nx), a function on the lower face z = z[0], carried along the field lines of b (3,nz,ny,nx) to
        every grid node, on the device (semantics: include/ndsm_hip.h, ndsm_hip_vecpot_alpha_map): the line of each
        node is followed against b (polarity +1) or along it (-1) with trace()'s step rules; where it ends on the
        lower face alpha is the bilinear interpolant of alpha0 there, everywhere else 0.  Returns (alpha, status):
        (nz,ny,nx) float64 and int32 (the TRACE_* code of each node's line).  step, max_steps as trace().
        device=True: the arrays are staged in device memory and the device-resident entry point runs."""
        _direction, step, max_steps = self._trace_args(step, max_steps, "both")
        shape = tuple(int(v) for v in self.nshape4[2::-1])
        B = self._field_arg(b, "alpha_map")
        a0 = self._alpha0_arg(alpha0, "alpha_map")
        alpha = np.zeros(int(np.prod(shape)))
        status = np.zeros(alpha.size, dtype=np.int32)
        self._entry("ndsm_hip_vecpot_alpha_map", [B, a0, int(polarity), step, max_steps, alpha, status], device)
        return alpha.reshape(shape), status.reshape(shape)

    def solve_current(self, b, j, a_init=None, niterex_max=10000, ncycles_max=1024, ex_tol=1e-13, vc_tol=1e-10, ms=5,
                      mean=False, mixed_precision=False, flxcrl=False, device=False):
        """Vector potential of a prescribed current j (3,nz,ny,nx): laplace(A_c) = -j_c with the gauge, boundary
        letters and tangential boundary values of solve()'s potential field for the B.n of b (3,nz,ny,nx; only its
        six faces are read).  Returns (ierr, A, B), B = curl A + the flux-balance fields; ierr 0 when every solve
        reached vc_tol, else 1.  j = 0 gives the potential field.  device=True: the arrays are staged in device
        memory and the device-resident entry point runs."""
        ioptc, ropt = self._options(niterex_max, ncycles_max, ex_tol, vc_tol, ms, mean, mixed_precision, flxcrl)
        shape = tuple(int(v) for v in self.nshape4[::-1])
        B = self._field_arg(b, "solve_current")
        J = self._field_arg(j, "solve_current")
        A = np.zeros(B.size) if a_init is None else self._field_arg(a_init, "solve_current")
        if not device:
            ierr = self.L.ndsm_hip_vecpot_solve_current(self.h, ioptc.ctypes.data_as(_ip), _d(ropt), _d(J), _d(A), _d(B))
        else:
            ierr = self._on_device([J, A, B], lambda dJ, dA, dB: self.L.ndsm_hip_vecpot_solve_current_device(
                self.h, ioptc.ctypes.data_as(_ip), _d(ropt), dJ, dA, dB))
        if ierr >= 9000:
            _check(ierr, "ndsm_hip_vecpot_solve_current", self.L)
        self.last_ioptc, self.last_ropt = ioptc, ropt
        return ierr, A.reshape(shape), B.reshape(shape)

    def force_free(self, b, alpha0, polarity=1, start="potential", a_init=None, niter_max=20, tol=0.0, step=0.5,
                   max_steps=None, niterex_max=10000, ncycles_max=1024, ex_tol=1e-13, vc_tol=1e-10, ms=5, mean=False,
                   mixed_precision=False, flxcrl=False, device=False):
        """Nonlinear force-free field, curl B = alpha B, from the B.n of b (3,nz,ny,nx) on the six faces and alpha0
        (ny,nx) on the lower face, by the Grad-Rubin iteration on the device (semantics: include/ndsm_hip.h,
        ndsm_hip_vecpot_nlfff).  Each pass is alpha_map() of the current field followed by solve_current() for
        j = alpha * B, warm-started from the last A, always with the B.n of the input b.  start: "potential" (the
        first field is solve()'s potential field of b) or "given" (it is b itself, with a_init - None: zeros - as
        its A).  At most niter_max passes; the loop stops after the pass whose max |B_new - B_old| < tol.  polarity,
        step, max_steps as alpha_map().  Returns (ierr, A, B, alpha, status, hist): the last pass's fields and alpha
        map, and hist (npasses, 4): max |B_new - B_old|, the energy 1/2 sum w |B|^2, the current-weighted sine of
        the angle between curl_h B and B, and the number of nodes whose line reaches the lower face.  ierr 0 when
        every solve of every pass reached vc_tol, else 1.  device=True: the arrays are staged in device memory and
        the device-resident entry point runs."""
        if start not in ("potential", "given"):
            raise ValueError(f"start must be 'potential' or 'given', not {start!r}")
        _direction, step, max_steps = self._trace_args(step, max_steps, "both")
        shape = tuple(int(v) for v in self.nshape4[::-1])
        B = self._field_arg(b, "force_free")
        a0 = self._alpha0_arg(alpha0, "force_free")
        A = np.zeros(B.size) if a_init is None else self._field_arg(a_init, "force_free")
        ioptc, ropt = self._options(niterex_max, ncycles_max, ex_tol, vc_tol, ms, mean, mixed_precision, flxcrl)
        alpha = np.zeros(B.size // 3)
        status = np.zeros(alpha.size, dtype=np.int32)
        hist = np.zeros((max(int(niter_max), 1), 4))
        niter = ctypes.c_int(0)
        args = (int(polarity), 0 if start == "potential" else 1, int(niter_max), float(tol), step, max_steps)
        if not device:
            ierr = self.L.ndsm_hip_vecpot_nlfff(self.h, ioptc.ctypes.data_as(_ip), _d(ropt), B.ctypes.data, a0.ctypes.data,
                                                *args, A.ctypes.data, alpha.ctypes.data, status.ctypes.data, _d(hist),
                                                ctypes.byref(niter))
        else:
            ierr = self._on_device([B, a0, A, alpha, status], lambda dB, da0, dA, dal, dst: self.L.ndsm_hip_vecpot_nlfff_device(
                self.h, ioptc.ctypes.data_as(_ip), _d(ropt), dB, da0, *args, dA, dal, dst, _d(hist), ctypes.byref(niter)))
        if ierr >= 9000:
            _check(ierr, "ndsm_hip_vecpot_nlfff", self.L)
        self.last_ioptc, self.last_ropt = ioptc, ropt
        return (ierr, A.reshape(shape), B.reshape(shape), alpha.reshape(shape[1:]), status.reshape(shape[1:]),
                hist[:niter.value].copy())

    def _dt0_default(self):
        """the default first step of optimize() on this handle's mesh: 0.1 min(h)^2"""
        return 0.1 * min(float(q[1]) - float(q[0]) for q in (self.x, self.y, self.z)) ** 2

    def optimize(self, b, w=None, start="potential", niter_max=10000, check=50, tol=1e-4, dt0=None, dt_min=None,
                 hist_rows=None, niterex_max=10000, ncycles_max=1024, ex_tol=1e-13, vc_tol=1e-10, ms=5, mean=False,
                 mixed_precision=False, flxcrl=False, device=False):
        """Nonlinear force-free field from a vector magnetogram by the optimization method (Wheatland et al. 2000,
        Wiegelmann 2004) on the device (semantics: include/ndsm_hip.h, ndsm_hip_vecpot_optimize): b (3,nz,ny,nx) is
        relaxed by pseudo-time steps that lower L = sum W w (|J x B|^2 / |B|^2 + (div B)^2), its six faces held fixed.
        start: "potential" (the first field is solve()'s potential field of the B.n of b with the k = 0 plane of b -
        the magnetogram, all three components - put back) or "given" (it is b itself).  w (nz,ny,nx): the weight
        function, None for 1 everywhere (boundary_weight() builds the usual one).  At most niter_max tries; every
        `check` tries the loop looks at L and stops when it fell by no more than tol * L since the last look, or
        when dt < dt_min.  dt0: the first step (None: 0.1 min(h)^2); dt_min None: 1e-6 dt0.  hist_rows None: one row
        per check and two more.  Returns (ierr, B, hist, info): hist (rows, 6) = [tries, L, L_f, L_d, dt, accepted]
        - row 0 the start field, the final state last -, info = (rows, tries, stop reason: 0 niter_max, 1 tol,
        2 dt_min); ierr 1 when a solve of the potential start missed vc_tol.  The field is not cleaned of its
        remaining divergence: project() does that.  device=True: the arrays are staged in device memory and the
        device-resident entry point runs."""
        if start not in ("potential", "given"):
            raise ValueError(f"start must be 'potential' or 'given', not {start!r}")
        hist_rows, hist, info = _descent_options([niter_max], check, tol, [dt0], [dt_min], hist_rows, 6)
        shape = tuple(int(v) for v in self.nshape4[::-1])
        B = self._field_arg(b, "optimize")
        W = None
        if w is not None:
            W = np.asarray(w)
            if W.shape != shape[1:]:
                raise NdsmHipError(f"optimize: weight of shape {W.shape}, the handle's grid needs {shape[1:]} (code 9002)")
            W = _f64(W).reshape(-1).copy()
        dt0, dt_min = _descent_steps(dt0, dt_min, self._dt0_default())
        ioptc, ropt = self._options(niterex_max, ncycles_max, ex_tol, vc_tol, ms, mean, mixed_precision, flxcrl)
        args = (0 if start == "potential" else 1, int(niter_max), int(check), float(tol), float(dt0), float(dt_min),
                hist.ctypes.data, int(hist_rows), info.ctypes.data)
        if not device:
            ierr = self.L.ndsm_hip_vecpot_optimize(self.h, ioptc.ctypes.data_as(_ip), _d(ropt), B.ctypes.data,
                                                   None if W is None else W.ctypes.data, *args)
        elif W is None:
            ierr = self._on_device([B], lambda dB: self.L.ndsm_hip_vecpot_optimize_device(
                self.h, ioptc.ctypes.data_as(_ip), _d(ropt), dB, None, *args))
        else:
            ierr = self._on_device([B, W], lambda dB, dW: self.L.ndsm_hip_vecpot_optimize_device(
                self.h, ioptc.ctypes.data_as(_ip), _d(ropt), dB, dW, *args))
        if ierr >= 9000:
            _check(ierr, "ndsm_hip_vecpot_optimize", self.L)
        self.last_ioptc, self.last_ropt = ioptc, ropt
        return (ierr, B.reshape(shape)) + _descent_result(hist, info)

    def optimize_obs(self, b, bobs=None, wm=None, nu=0.01, free=True, w=None, start="potential", niter_max=10000,
                     check=50, tol=1e-4, dt0=None, dt_min=None, hist_rows=None, niterex_max=10000, ncycles_max=1024,
                     ex_tol=1e-13, vc_tol=1e-10, ms=5, mean=False, mixed_precision=False, flxcrl=False, device=False):
        """optimize() with the lower face fitted to a measured magnetogram within its errors (Wiegelmann & Inhester
        2010; semantics: include/ndsm_hip.h, ndsm_hip_vecpot_optimize_obs): L = (L_f + L_d) + nu L_m with
        L_m = sum W2 wm (B(k = 0) - bobs)^2 over the lower face, and with free=True that face - except its rim, which
        belongs to the side faces - moves with the descent.  bobs (3,ny,nx): the observation, None for a copy of b's
        k = 0 plane; it is only the target of the fit, the start field is built from b as in optimize().  wm (3,ny,nx):
        the confidence per pixel and component, None for 1 everywhere (measurement_weight() builds the usual one).
        nu >= 0: the weight of L_m.  free=False holds the face and only reports L_m; with nu = 0 that is optimize()
        bit for bit.  Everything else as optimize().  Returns (ierr, B, hist, info): hist (rows, 7) = [tries, L, L_f,
        L_d, L_m, dt, accepted].  device=True: the arrays are staged in device memory and the device-resident entry
        point runs."""
        if start not in ("potential", "given"):
            raise ValueError(f"start must be 'potential' or 'given', not {start!r}")
        if free not in (True, False, 0, 1):
            raise ValueError(f"free must be True or False, not {free!r}")
        if not (nu >= 0.0 and np.isfinite(nu)):
            raise ValueError(f"nu must be finite and >= 0, not {nu!r}")
        hist_rows, hist, info = _descent_options([niter_max], check, tol, [dt0], [dt_min], hist_rows, 7)
        shape = tuple(int(v) for v in self.nshape4[::-1])
        B = self._field_arg(b, "optimize_obs")
        W = None
        if w is not None:
            W = np.asarray(w)
            if W.shape != shape[1:]:
                raise NdsmHipError(f"optimize_obs: weight of shape {W.shape}, the handle's grid needs {shape[1:]} "
                                   "(code 9002)")
            W = _f64(W).reshape(-1).copy()
        pshape = (3,) + shape[2:]
        planes = []
        for name, v in (("observation", bobs), ("measurement weight", wm)):
            if v is None:
                planes.append(None)
                continue
            a = np.asarray(v)
            if a.shape != pshape:
                raise NdsmHipError(f"optimize_obs: {name} of shape {a.shape}, the handle's lower face needs {pshape} "
                                   "(code 9002)")
            planes.append(_f64(a).reshape(-1).copy())
        if planes[0] is None:
            planes[0] = B.reshape(shape)[:, 0].reshape(-1).copy()
        dt0, dt_min = _descent_steps(dt0, dt_min, self._dt0_default())
        ioptc, ropt = self._options(niterex_max, ncycles_max, ex_tol, vc_tol, ms, mean, mixed_precision, flxcrl)
        args = (float(nu), int(bool(free)), 0 if start == "potential" else 1, int(niter_max), int(check), float(tol),
                float(dt0), float(dt_min), hist.ctypes.data, int(hist_rows), info.ctypes.data)
        arrays = [B, W] + planes
        if not device:
            ierr = self.L.ndsm_hip_vecpot_optimize_obs(self.h, ioptc.ctypes.data_as(_ip), _d(ropt),
                                                       *[None if a is None else a.ctypes.data for a in arrays], *args)
        else:
            given = [a for a in arrays if a is not None]

            def call(*dev):
                it = iter(dev)
                ptrs = [None if a is None else next(it) for a in arrays]
                return self.L.ndsm_hip_vecpot_optimize_obs_device(self.h, ioptc.ctypes.data_as(_ip), _d(ropt), *ptrs,
                                                                  *args)
            ierr = self._on_device(given, call)
        if ierr >= 9000:
            _check(ierr, "ndsm_hip_vecpot_optimize_obs", self.L)
        self.last_ioptc, self.last_ropt = ioptc, ropt
        return (ierr, B.reshape(shape)) + _descent_result(hist, info)

    def optimize_cascade(self, coarser, b, w=None, start="potential", niter_max=10000, check=50, tol=1e-4, dt0=None,
                         dt_min=None, hist_rows=None, niterex_max=10000, ncycles_max=1024, ex_tol=1e-13, vc_tol=1e-10,
                         ms=5, mean=False, mixed_precision=False, flxcrl=False, device=False):
        """optimize() as a coarse-to-fine cascade (semantics: include/ndsm_hip.h, ndsm_hip_vecpot_optimize_cascade):
        this handle is the finest mesh, `coarser` a sequence of VecPot handles on coarser meshes of the same box, finest
        first (cascade_shapes() proposes their shapes).  b and w live on this handle's mesh.  The hat average of b -
        and the interpolated w - goes to every coarser level; the coarsest level runs optimize() with `start`, and
        every finer level starts from the interpolated result of the level below with the k = 0 plane ("potential") or
        all six faces ("given") of its own average of b put over it.  With start "potential" the side and top faces of
        the result are therefore the prolonged boundary of the coarsest mesh's potential field, not the finest mesh's
        own potential field as in optimize().  niter_max, dt0, dt_min: one value for every level or a sequence, one per
        level, finest first; dt0 None: 0.1 min(h)^2 of each level's own mesh, dt_min None: 1e-6 of that level's dt0.
        check, tol and hist_rows are shared.  Returns (ierr, B, hist, info): hist a list of per-level arrays
        (rows, 6), info a list of per-level tuples, both as optimize() gives them; ierr 1 when the coarsest level's
        potential solve missed vc_tol.  No coarser handle: optimize() itself, bit for bit."""
        levels, nit, d0, dm, hist_rows, hist, info, B, W = self._cascade_setup(
            "optimize_cascade", coarser, b, w, start, niter_max, check, tol, dt0, dt_min, hist_rows, 6)
        nl = len(levels)
        shape = tuple(int(v) for v in self.nshape4[::-1])
        ioptc, ropt = self._options(niterex_max, ncycles_max, ex_tol, vc_tol, ms, mean, mixed_precision, flxcrl)
        ioptc[self.L.get_iopt_ngrids()] = levels[-1].ngrids
        handles = (ctypes.c_void_p * nl)(*[V.h for V in levels])
        nit_a = np.array([int(v) for v in nit], dtype=np.intc)
        d0_a, dm_a = np.array(d0, dtype=np.float64), np.array(dm, dtype=np.float64)

        def call(fn, pB, pW):
            return fn(handles, nl, ioptc.ctypes.data_as(_ip), _d(ropt), pB, pW, 0 if start == "potential" else 1,
                      nit_a.ctypes.data, int(check), float(tol), d0_a.ctypes.data, dm_a.ctypes.data, hist.ctypes.data,
                      int(hist_rows), info.ctypes.data)
        if not device:
            ierr = call(self.L.ndsm_hip_vecpot_optimize_cascade, B.ctypes.data, None if W is None else W.ctypes.data)
        elif W is None:
            ierr = self._on_device([B], lambda dB: call(self.L.ndsm_hip_vecpot_optimize_cascade_device, dB, None))
        else:
            ierr = self._on_device([B, W], lambda dB, dW: call(self.L.ndsm_hip_vecpot_optimize_cascade_device, dB, dW))
        if ierr >= 9000:
            _check(ierr, "ndsm_hip_vecpot_optimize_cascade", self.L)
        self.last_ioptc, self.last_ropt = ioptc, ropt
        per_level = [_descent_result(hist[l], info[l]) for l in range(nl)]
        return ierr, B.reshape(shape), [h for h, _ in per_level], [i for _, i in per_level]

    def _cascade_setup(self, who, coarser, b, w, start, niter_max, check, tol, dt0, dt_min, hist_rows, width):
        """What optimize_cascade() and optimize_obs_cascade() share, checked before the library is reached: (levels,
        niter_max, dt0, dt_min per level - the steps with their defaults -, hist_rows, hist, info, B, W)"""
        levels = [self] + list(coarser)
        nl = len(levels)
        if start not in ("potential", "given"):
            raise ValueError(f"start must be 'potential' or 'given', not {start!r}")
        nit, d0, dm = (_per_level(name, v, nl) for name, v in (("niter_max", niter_max), ("dt0", dt0), ("dt_min", dt_min)))
        hist_rows, hist, info = _descent_options(nit, check, tol, d0, dm, hist_rows, width, nl)
        for V in levels[1:]:
            if not isinstance(V, VecPot):
                raise ValueError(f"coarser must hold VecPot handles, not {type(V).__name__}")
        for fine, V in zip(levels, levels[1:]):
            if any(int(c) > int(f) for c, f in zip(V.nshape4[:3], fine.nshape4[:3])):
                raise ValueError(f"a coarser level has more nodes than the level before it: {tuple(V.nshape4[:3])} "
                                 f"after {tuple(fine.nshape4[:3])}")
            for q, r in zip((V.x, V.y, V.z), (self.x, self.y, self.z)):
                if q[0].tobytes() != r[0].tobytes() or q[-1].tobytes() != r[-1].tobytes():
                    raise ValueError("every level must span the box of the finest mesh: first and last coordinates "
                                     f"{q[0]!r}, {q[-1]!r} against {r[0]!r}, {r[-1]!r}")
        shape = tuple(int(v) for v in self.nshape4[::-1])
        B = self._field_arg(b, who)
        W = None
        if w is not None:
            W = np.asarray(w)
            if W.shape != shape[1:]:
                raise NdsmHipError(f"{who}: weight of shape {W.shape}, the handle's grid needs {shape[1:]} "
                                   "(code 9002)")
            W = _f64(W).reshape(-1).copy()
        for l, V in enumerate(levels):
            d0[l], dm[l] = _descent_steps(d0[l], dm[l], V._dt0_default())
        return levels, nit, d0, dm, hist_rows, hist, info, B, W

    def optimize_obs_cascade(self, coarser, b, bobs=None, wm=None, nu=0.01, free=True, w=None, start="potential",
                             niter_max=10000, check=50, tol=1e-4, dt0=None, dt_min=None, hist_rows=None,
                             niterex_max=10000, ncycles_max=1024, ex_tol=1e-13, vc_tol=1e-10, ms=5, mean=False,
                             mixed_precision=False, flxcrl=False, device=False):
        """optimize_obs() as a coarse-to-fine cascade (semantics: include/ndsm_hip.h,
        ndsm_hip_vecpot_optimize_obs_cascade): the handles, b, w and the per-level options as optimize_cascade(); bobs,
        wm, free as optimize_obs(), on this handle's lower face (bobs None: a copy of b's k = 0 plane).  nu: one value
        for every level or a sequence, one per level, finest first.  Every coarser level gets the confidence-weighted
        restriction of (bobs, wm) - resample_weighted() -, or the hat average of bobs when wm is None.  The coarsest
        level runs optimize_obs() with `start`; every finer level starts from the interpolated result of the level
        below with its own average of b pasted over the k = 0 plane ("potential") or the six faces ("given") - with
        free=True without the freed nodes of the k = 0 plane, which keep what the level below has fitted.  Returns
        (ierr, B, hist, info): hist a list of per-level arrays (rows, 7), info a list of per-level tuples, both as
        optimize_obs() gives them.  No coarser handle: optimize_obs() itself, bit for bit; free=False with nu = 0:
        optimize_cascade() bit for bit."""
        if free not in (True, False, 0, 1):
            raise ValueError(f"free must be True or False, not {free!r}")
        levels, nit, d0, dm, hist_rows, hist, info, B, W = self._cascade_setup(
            "optimize_obs_cascade", coarser, b, w, start, niter_max, check, tol, dt0, dt_min, hist_rows, 7)
        nl = len(levels)
        nus = _per_level("nu", nu, nl)
        for v in nus:
            if not (v >= 0.0 and np.isfinite(v)):
                raise ValueError(f"nu must be finite and >= 0, not {v!r}")
        shape = tuple(int(v) for v in self.nshape4[::-1])
        pshape = (3,) + shape[2:]
        planes = []
        for name, v in (("observation", bobs), ("measurement weight", wm)):
            if v is None:
                planes.append(None)
                continue
            a = np.asarray(v)
            if a.shape != pshape:
                raise NdsmHipError(f"optimize_obs_cascade: {name} of shape {a.shape}, the handle's lower face needs "
                                   f"{pshape} (code 9002)")
            planes.append(_f64(a).reshape(-1).copy())
        if planes[0] is None:
            planes[0] = B.reshape(shape)[:, 0].reshape(-1).copy()
        ioptc, ropt = self._options(niterex_max, ncycles_max, ex_tol, vc_tol, ms, mean, mixed_precision, flxcrl)
        ioptc[self.L.get_iopt_ngrids()] = levels[-1].ngrids
        handles = (ctypes.c_void_p * nl)(*[V.h for V in levels])
        nit_a = np.array([int(v) for v in nit], dtype=np.intc)
        d0_a, dm_a = np.array(d0, dtype=np.float64), np.array(dm, dtype=np.float64)
        nu_a = np.array([float(v) for v in nus], dtype=np.float64)
        arrays = [B, W] + planes

        def call(fn, ptrs):
            return fn(handles, nl, ioptc.ctypes.data_as(_ip), _d(ropt), *ptrs, nu_a.ctypes.data, int(bool(free)),
                      0 if start == "potential" else 1, nit_a.ctypes.data, int(check), float(tol), d0_a.ctypes.data,
                      dm_a.ctypes.data, hist.ctypes.data, int(hist_rows), info.ctypes.data)
        if not device:
            ierr = call(self.L.ndsm_hip_vecpot_optimize_obs_cascade, [None if a is None else a.ctypes.data for a in arrays])
        else:
            def on_device(*dev):
                it = iter(dev)
                return call(self.L.ndsm_hip_vecpot_optimize_obs_cascade_device,
                            [None if a is None else next(it) for a in arrays])
            ierr = self._on_device([a for a in arrays if a is not None], on_device)
        if ierr >= 9000:
            _check(ierr, "ndsm_hip_vecpot_optimize_obs_cascade", self.L)
        self.last_ioptc, self.last_ropt = ioptc, ropt
        per_level = [_descent_result(hist[l], info[l]) for l in range(nl)]
        return ierr, B.reshape(shape), [h for h, _ in per_level], [i for _, i in per_level]

    def preprocess(self, bm, obs=None, mu=(1, 1, 1e-3, 1e-2, 1e-2), niter_max=10000, check=50, tol=1e-4, dt0=None,
                   dt_min=None, hist_rows=None, device=False):
        """Preprocessing of a measured vector magnetogram for optimize() (Wiegelmann, Inhester & Sakurai 2006) on the
        device (semantics: include/ndsm_hip.h, ndsm_hip_vecpot_preprocess): bm (3,ny,nx), the field on the lower face
        of the handle's mesh, is moved by descent steps that lower L = mu1 L1 + mu2 L2 + mu3h L3h + mu3z L3z + mu4 L4
        - net force, net torque, distance of the horizontal and of the vertical component from the observation,
        roughness.  obs (3,ny,nx): the observation the distance terms refer to, None for bm itself (a continued call
        passes the original).  mu = (mu1, mu2, mu3h, mu3z, mu4), each >= 0.  At most niter_max tries; every `check`
        tries the loop looks at L and stops when it fell by no more than tol * L since the last look, or when
        dt < dt_min.  dt0: the first step, dimensionless (None: 0.01); dt_min None: 1e-6 dt0.  The default mu and dt0
        are those of a numerical prototype on a synthetic field; they are NOT tuned on real data - choose mu3h, mu3z
        from the measurement errors.  hist_rows None: one row per check and two more.  Returns (ierr, Bm, hist, info):
        hist (rows, 17) = [tries, L, L1, L2, L3h, L3z, L4, dt, accepted, S1 .. S6, S10, S11] - row 0 the start, the
        final state last (magnetogram_balance() turns it into the force and torque figures) -, info = (rows, tries,
        stop reason: 0 niter_max, 1 tol, 2 dt_min).  Nothing of the handle changes; the caller puts Bm on the k = 0
        plane of the b handed to optimize().  device=True: the arrays are staged in device memory and the
        device-resident entry point runs."""
        hist_rows, hist, info = _descent_options([niter_max], check, tol, [dt0], [dt_min], hist_rows, 17)
        muv = np.array(mu, dtype=np.float64).reshape(-1)
        if muv.size != 5 or not (np.isfinite(muv).all() and (muv >= 0.0).all()):
            raise ValueError(f"mu must be five finite numbers >= 0, not {mu!r}")
        shape = (3,) + tuple(int(v) for v in self.nshape4[1::-1])
        arrays = []
        for name, v in (("magnetogram", bm), ("observation", obs)):
            if v is None:
                continue
            a = np.asarray(v)
            if a.shape != shape:
                raise NdsmHipError(f"preprocess: {name} of shape {a.shape}, the handle's lower face needs {shape} "
                                   "(code 9002)")
            arrays.append(_f64(a).reshape(-1).copy())
        B = arrays[0]
        dt0, dt_min = _descent_steps(dt0, dt_min, 0.01)
        args = (muv.ctypes.data, int(niter_max), int(check), float(tol), float(dt0), float(dt_min), hist.ctypes.data,
                int(hist_rows), info.ctypes.data)
        if not device:
            ierr = self.L.ndsm_hip_vecpot_preprocess(self.h, B.ctypes.data,
                                                     None if obs is None else arrays[1].ctypes.data, *args)
        elif obs is None:
            ierr = self._on_device([B], lambda dB: self.L.ndsm_hip_vecpot_preprocess_device(self.h, dB, None, *args))
        else:
            ierr = self._on_device(arrays, lambda dB, dO: self.L.ndsm_hip_vecpot_preprocess_device(self.h, dB, dO, *args))
        _check(ierr, "ndsm_hip_vecpot_preprocess", self.L)
        return (ierr, B.reshape(shape)) + _descent_result(hist, info)

    def paths(self, b, seeds, g=None, step=0.5, max_steps=None, direction="both", every=1, max_points=None,
              values=True, device=False):
        """The field lines of trace() as polylines (semantics: include/ndsm_hip.h, ndsm_hip_vecpot_paths): every
        `every`-th point of each line - the seed first, the end point always last - with b, g and the running integral
        of g at each.  b, seeds, g, step, max_steps, direction as trace().  max_points: the capacity of the first
        call; when the lines hold more points the call is repeated once with that number (None: a counting call,
        then one call of the exact size).  values=False: the points alone.  Returns a FieldPaths tuple: lines (the
        FieldLines of the same call, bit for bit trace()'s), offsets (nl + 1; int64: line l owns the rows offsets[l] ..
        offsets[l + 1] - 1, lane order: the forward lines, then for "both" the backward lines), points (total,3), b, g
        (total,3) and integral (total) at the points (b None with values=False; g and integral None without g too).
        path_of(paths, l) cuts out one line, whole_line(paths, i) joins the two directions of seed i.  device=True:
        the arrays are staged in device memory and the device-resident entry point runs."""
        direction, step, max_steps = self._trace_args(step, max_steps, direction)
        every, max_points = _paths_args(every, max_points)
        B = self._field_arg(b, "paths")
        G = None if g is None else self._field_arg(g, "paths")
        S = self._seeds_arg(seeds)
        ns = len(S)
        nl = ns * (2 if direction == 0 else 1)
        out = _trace_outputs(ns, direction)
        withb, withg = bool(values), bool(values) and G is not None
        if ns == 0:
            return _field_paths(out, direction, np.zeros(1, dtype=np.int64), np.zeros((0, 3)),
                                np.zeros((0, 3)) if withb else None, np.zeros((0, 3)) if withg else None,
                                np.zeros(0) if withg else None)
        def run(cap):
            offsets, total = np.zeros(nl + 1, dtype=np.int64), np.zeros(1, dtype=np.int64)
            m = max(cap, 1)
            pts = [np.zeros((m, 3)), np.zeros((m, 3)) if withb else None, np.zeros((m, 3)) if withg else None,
                   np.zeros(m) if withg else None]
            self._entry("ndsm_hip_vecpot_paths", [B, G, ns, S, step, max_steps, direction, every, cap, *out, offsets,
                                                  total.ctypes.data, *[a if cap else None for a in pts]], device)
            return int(total[0]), (offsets, pts)
        n, (offsets, pts) = _with_capacity(run, 0 if max_points is None else max_points)
        return _field_paths(out, direction, offsets, *[None if a is None else a[:n] for a in pts])

    def default_max_steps(self, step=0.5):
        """the max_steps that trace() uses for max_steps=None: ceil(4 (nx + ny + nz) / step)"""
        return int(np.ceil(4.0 * float(int(self.nshape4[0]) + int(self.nshape4[1]) + int(self.nshape4[2])) / step))

    def _trace_args(self, step, max_steps, direction):
        """(direction code, step, max_steps) of trace(); ValueError before anything is launched"""
        if direction not in _DIRECTIONS:
            raise ValueError(f"direction must be 'forward', 'backward' or 'both', not {direction!r}")
        step = float(step)
        if not (step > 0.0 and np.isfinite(step)):
            raise ValueError(f"step must be a positive finite number, not {step!r}")
        if max_steps is None:
            max_steps = self.default_max_steps(step)
        if int(max_steps) != max_steps or max_steps < 1:
            raise ValueError(f"max_steps must be an integer >= 1, not {max_steps!r}")
        return _DIRECTIONS[direction], step, int(min(int(max_steps), TRACE_MAX_STEPS))

    @staticmethod
    def _seeds_arg(seeds):
        S = np.asarray(seeds, dtype=np.float64)
        if S.ndim != 2 or S.shape[1] != 3:
            raise NdsmHipError(f"trace: seeds of shape {S.shape}, (nseeds, 3) is needed (code 9002)")
        if len(S) > TRACE_MAX_SEEDS:
            raise NdsmHipError(f"trace: {len(S)} seeds, at most {TRACE_MAX_SEEDS} per call (code 9002)")
        return np.ascontiguousarray(S).copy()

    def squashing(self, b, seeds, g=None, integrand=0, twist=False, step=0.5, max_steps=None, device=False):
        """Squashing factor Q (Titov 2007) of b (3,nz,ny,nx) at seeds (nseeds,3; anywhere in the box), on the device,
        from the one field line through each seed: two deviation vectors are integrated along it with the gradient
        of the trilinear interpolant (Scott, Pontin & Hornig 2017; semantics: include/ndsm_hip.h,
        ndsm_hip_vecpot_squash).  Lines, step and max_steps as trace(), always both directions; the end points differ
        from trace()'s in the last digits (the exit step is refined twice).  g (3,nz,ny,nx; None: zeros) is integrated
        along the lines, integrand 0: g.b/|b| (as trace), 1: g.b/|b|^2.  twist=True (not together with g): g =
        curl_h b is formed on the device, integrand 1, and twist = (integral[0] + integral[1]) / (4 pi) is the twist
        number T_w of the whole line.  Returns a QMap tuple: q (nseeds; NaN unless both directions ended on a face),
        twist (nseeds, NaN where q is; None without twist=True), ends (2,nseeds,3), length, integral (2,nseeds),
        status, nsteps (2,nseeds; int32), row 0 forward, row 1 backward.  Q is not clamped to >= 2 and depends on
        the faces the line ends on: 2 for a uniform field between opposite faces, |b|^2 / |b_a b_c| between faces
        normal to different axes a, c.  device=True: the arrays are staged in device memory and the device-resident
        entry point runs."""
        if integrand not in (0, 1) or isinstance(integrand, bool):
            raise ValueError(f"integrand must be 0 or 1, not {integrand!r}")
        if twist and g is not None:
            raise ValueError("twist=True forms g = curl b itself: give g or twist, not both")
        _d0, step, max_steps = self._trace_args(step, max_steps, "both")
        B = self._field_arg(b, "squashing")
        G = None if g is None else self._field_arg(g, "squashing")
        S = self._seeds_arg(seeds)
        out = [np.zeros(len(S))] + _trace_outputs(len(S), 0)
        if len(S) == 0:
            return _qmap(out, twist)
        if twist:
            integrand = 1
        # (the field passed as its own g with integrand 1 asks the library for g = curl b)
        self._entry("ndsm_hip_vecpot_squash", [B, B if twist else G, integrand, len(S), S, step, max_steps, *out],
                    device, who="ndsm_hip_vecpot_squash")
        return _qmap(out, twist)

    def squashing_perp(self, b, seeds, g=None, integrand=0, twist=False, step=0.5, max_steps=None, device=False):
        """Perpendicular squashing factor Q-perp (Titov 2007) of b next to Q, on the device (semantics:
        include/ndsm_hip.h, ndsm_hip_vecpot_squash_perp): squashing() with the deviation vectors at the two feet
        projected onto the planes perpendicular to b there instead of onto the faces, and |b| at the feet in place of
        |b_n|.  Q-perp does not depend on the faces a line ends on - a uniform field gives 2 for every pair - and is
        the quantity for cuts through the volume (seed_cut).  Arguments as squashing().  Returns a QPerpMap tuple: q
        (the bits of squashing()), q_perp (nseeds; NaN unless both directions ended on a face; a line that arrives
        tangent to its face has a q_perp but no q), twist (NaN where q_perp is: the twist of a line exists whenever
        both feet do; None without twist=True), ends, length, integral, status, nsteps as squashing(), bit for bit.
        Not clamped to >= 2."""
        if integrand not in (0, 1) or isinstance(integrand, bool):
            raise ValueError(f"integrand must be 0 or 1, not {integrand!r}")
        if twist and g is not None:
            raise ValueError("twist=True forms g = curl b itself: give g or twist, not both")
        _d0, step, max_steps = self._trace_args(step, max_steps, "both")
        B = self._field_arg(b, "squashing_perp")
        G = None if g is None else self._field_arg(g, "squashing_perp")
        S = self._seeds_arg(seeds)
        q, qperp, lines = np.zeros(len(S)), np.zeros(len(S)), _trace_outputs(len(S), 0)
        if len(S) == 0:
            return _qperpmap(q, qperp, lines, twist)
        if twist:
            integrand = 1
        # (the field passed as its own g with integrand 1 asks the library for g = curl b)
        self._entry("ndsm_hip_vecpot_squash_perp", [B, B if twist else G, integrand, len(S), S, step, max_steps, q,
                                                    qperp, *lines], device)
        return _qperpmap(q, qperp, lines, twist)

    def nulls(self, b, max_nulls=4096, merge=1e-6, device=False):
        """Null points of b (3,nz,ny,nx) and their types, on the device (semantics: include/ndsm_hip.h,
        ndsm_hip_vecpot_nulls): every cell of the mesh is screened (a component of one strict sign over the eight
        corners cannot vanish inside), and a Newton iteration on the trilinear interpolant runs in each remaining
        cell.  max_nulls: the capacity of the first call; when more are found the call is repeated once with that
        number (0: count only - ncandidates and nfound, no records).  merge (in units of min(h); None: the raw records): a null on a face, edge or node shared by cells is
        reported by each of them - records whose positions lie within merge of one already kept are dropped, the
        lowest cell kept.  Returns a Nulls tuple: position (n,3), cell (n; int64, i + nx (j + ny k) of the low
        corner), jacobian (n,3,3; dB_a/dx_b), sign (n; +1: det < 0, two eigenvalues with positive real part, the fan
        diverges; -1: det > 0; 0), spiral (n; a complex pair), eigenvalues (n,3; complex, numpy.linalg.eig of the
        jacobian), spine (n,3; the unit eigenvector of the eigenvalue whose real part has the lone sign), fan (n,2,3;
        the other two, complex for a spiral), det, residual (n; |b| at the position), ncandidates (the cells the
        screen left), nfound (the records before merging).  device=True: the arrays are staged in device memory and
        the device-resident entry point runs."""
        if (isinstance(max_nulls, bool) or not isinstance(max_nulls, (int, float, np.integer)) or
                not np.isfinite(max_nulls) or int(max_nulls) != max_nulls or not 0 <= max_nulls <= NULLS_MAX):
            raise ValueError(f"max_nulls must be an integer in 0 .. {NULLS_MAX}, not {max_nulls!r}")
        if merge is not None and not (isinstance(merge, (int, float)) and not isinstance(merge, bool) and
                                      merge >= 0.0 and np.isfinite(merge)):
            raise ValueError(f"merge must be None or a finite number >= 0, not {merge!r}")
        B = self._field_arg(b, "nulls")
        def run(cap):
            counts = np.zeros(2, dtype=np.int64)
            m = max(cap, 1)
            out = [np.zeros(m, dtype=np.int64), np.zeros((m, 3)), np.zeros((m, 3, 3)), np.zeros(m), np.zeros(m),
                   np.zeros(m, dtype=np.int32), np.zeros(m, dtype=np.int32)]
            self._entry("ndsm_hip_vecpot_nulls", [B, cap, counts.ctypes.data, *out], device)
            return int(counts[1]), (counts, out)
        n, (counts, out) = _with_capacity(run, int(max_nulls), count_only=True)
        hmin = min(float(q[1]) - float(q[0]) for q in (self.x, self.y, self.z))
        return _nulls_tuple([a[:n] for a in out], int(counts[0]), int(counts[1]), None if merge is None else
                            float(merge) * hmin)

    def dips(self, b, plane_only=False, max_dips=None, device=False):
        """Magnetic dips and bald patches of b (3,nz,ny,nx), on the device (semantics: include/ndsm_hip.h,
        ndsm_hip_vecpot_dips): the mesh edges on which b_z changes sign with (b.grad)b_z > 0 at the crossing - the
        points where a field line is locally lowest; on the plane k = 0 they are the bald patches, where field lines
        touch the lower boundary from above.  plane_only=True: the plane k = 0 and its x and y edges alone, the bald
        patches at O(nx ny) cost.  max_dips: the capacity of the first call; when more are found the call is repeated
        once with that number (None: a counting call, then one call of the exact size; 0: count only - ncrossings,
        ndips and nbald, no records).  Returns a Dips tuple:
        position (n,3), edge (n; int64, 3 node + axis), axis (n; 0, 1, 2: the edge runs along x, y, z), node (n,3; i,
        j, k of the edge's low node), b, grad (n,3; the field and the gradient of b_z at the position), curv (n;
        (b.grad)b_z there, > 0), kappa (n; curv / (b_x^2 + b_y^2), the field line's curvature at its lowest point),
        bald (n; bool), ncrossings (the edges on which b_z changes sign), ndips, nbald (exact counts whatever the
        capacity), in ascending edge.  device=True: the arrays are staged in device memory and the device-resident
        entry point runs."""
        plane_only, max_dips = _dips_args(plane_only, max_dips)
        B = self._field_arg(b, "dips")
        def run(cap):
            counts = np.zeros(3, dtype=np.int64)
            m = max(cap, 1)
            out = [np.zeros(m, dtype=np.int64), np.zeros((m, 3)), np.zeros((m, 3)), np.zeros((m, 3)), np.zeros(m),
                   np.zeros(m, dtype=np.int32)]
            self._entry("ndsm_hip_vecpot_dips", [B, plane_only, cap, counts.ctypes.data, *out], device)
            return int(counts[1]), (counts, out)
        if max_dips is None:
            n, (counts, out) = _with_capacity(run, 0)
        else:
            n, (counts, out) = _with_capacity(run, max_dips, count_only=True)
        return _dips_tuple([a[:n] for a in out], counts, int(self.nshape4[0]), int(self.nshape4[1]))

    def connectivity(self, b, label=None, K=None, thr=0.0, step=0.5, max_steps=None, max_pairs=None, device=False):
        """The connectivity fluxes between the flux patches of the lower face of b (3,nz,ny,nx), on the device
        (semantics: include/ndsm_hip.h, ndsm_hip_vecpot_connect): one field line from every labelled pixel, followed
        along b where b_z > 0 there and against it where b_z < 0, the class of the place where it ends - the patch
        of the nearest pixel when it comes back to the face, else minus its TRACE_* status - and per (patch, class)
        pair the number of lines and the flux |b_z| w at their feet.  label (ny,nx; integers, e.g.
        partition_magnetogram()'s) with K the largest label that counts (None: label.max()); label=None partitions
        b_z of the lower face with thr (thr must be 0 with a label) on the device (ndsm_hip_partition_device), and the
        label map goes into the connect call without crossing PCIe in between.  step, max_steps as trace()'s.  max_pairs: the capacity of
        the first call, repeated once when there are more pairs (None: a counting call, then one of the exact size;
        0: count only).  Returns a Connectivity tuple: dest (ny,nx; int32, CONNECT_NONE where no line starts), ends
        (ny,nx,3), length, status (ny,nx), pa, pc, nlines, pflux (n; in ascending (pa, pc)), ntraced, npairs (exact
        whatever the capacity), label (ny,nx; the map that was used), K.  device=True: the arrays are staged in
        device memory and the device-resident entry point runs."""
        _, step, max_steps = self._trace_args(step, max_steps, "forward")
        thr, max_pairs = _thr_arg(thr), _capacity_arg("max_pairs", max_pairs)
        nx, ny = int(self.nshape4[0]), int(self.nshape4[1])
        npix = nx * ny
        if label is None:
            if K is not None:
                raise ValueError("K is the partition's to find when label is None")
            if len(self.x) < 2 or len(self.y) < 2 or not (self.x[1] - self.x[0] > 0.0 and self.y[1] - self.y[0] > 0.0):
                raise ValueError("the partition needs at least 2 nodes per axis and spacings > 0")
            lab = None
        else:
            if thr != 0.0:
                raise ValueError("thr is the partition's, which does not run when a label is given")
            lab = np.asarray(label)
            if lab.shape != (ny, nx) or lab.dtype.kind not in "iu":
                raise ValueError(f"label of shape {lab.shape} and type {lab.dtype}, integers of shape {(ny, nx)} are "
                                 "needed")
            if K is None:
                K = max(int(lab.max()), 0)
            if isinstance(K, bool) or int(K) != K or not 0 <= K <= PATCHES_MAX:
                raise ValueError(f"K must be an integer in 0 .. {PATCHES_MAX}, not {K!r}")
            K = int(K)
            lab = np.clip(lab, -1, PATCHES_MAX).astype(np.int32).reshape(-1).copy()     # (outside 1 .. K stays outside)
        B = self._field_arg(b, "connectivity")
        L = self.L
        ns2 = np.array([nx, ny], dtype=np.intc)

        def run(cap):
            counts, pcounts = np.zeros(2, dtype=np.int64), np.zeros(2, dtype=np.int64)
            m = max(cap, 1)
            out = [np.zeros(npix, dtype=np.int32), np.zeros(3 * npix), np.zeros(npix), np.zeros(npix, dtype=np.int32)]
            pairs = [np.zeros(m, dtype=np.int32), np.zeros(m, dtype=np.int32), np.zeros(m, dtype=np.int64), np.zeros(m)]
            if lab is not None:
                self._entry("ndsm_hip_vecpot_connect", [B, lab, K, step, max_steps, cap, counts.ctypes.data, *out, *pairs],
                            device)
                return int(counts[1]), (counts, out, pairs, lab, K)
            own = np.zeros(npix, dtype=np.int32)

            def both(dB, dlab, *dout):
                rc = L.ndsm_hip_partition_device(ns2.ctypes.data_as(_ip), _d(self.x), _d(self.y),
                                                 ctypes.c_void_p(dB.value + 16 * (B.size // 3)), thr, 0,
                                                 pcounts.ctypes.data, dlab, None, None, None, None, None, None)
                if rc != 0:
                    return rc
                return L.ndsm_hip_vecpot_connect_device(self.h, dB, dlab, int(pcounts[1]), step, max_steps, cap,
                                                        counts.ctypes.data, *dout)
            _check(_staged(L, [B, own, *out, *pairs], both), "ndsm_hip_partition_device + ndsm_hip_vecpot_connect_device",
                   L)
            return int(counts[1]), (counts, out, pairs, own, int(pcounts[1]))
        if max_pairs is None:
            n, (counts, out, pairs, used, k) = _with_capacity(run, 0)
        else:
            n, (counts, out, pairs, used, k) = _with_capacity(run, max_pairs, count_only=True)
        return _connect_tuple(counts, out, pairs, n, used, k, ny, nx)

    def bald_patch_lines(self, b, dips, lift=1e-3, **paths_options):
        """The field lines that generate the bald-patch separatrix surface of b: the records of `dips` (a Dips tuple
        of dips() or bald_patches()) with `bald` seed one line each at position + (0, 0, lift h_z), traced in both
        directions by paths() (paths_options: its g, step, max_steps, every, max_points, values, device).  Returns
        paths()'s FieldPaths; whole_line(paths, i) joins the two halves of the line through bald patch i."""
        if (isinstance(lift, bool) or not isinstance(lift, (int, float, np.integer, np.floating)) or
                not (np.isfinite(lift) and lift >= 0.0)):
            raise ValueError(f"lift must be a finite number >= 0, not {lift!r}")
        if "direction" in paths_options:
            raise ValueError("bald_patch_lines traces in both directions: direction is not an option")
        return self.paths(b, _bald_seeds(dips, lift, float(self.z[1]) - float(self.z[0])), direction="both",
                          **paths_options)

    def skeleton(self, b, nulls=None, radius=0.5, nring=16, ring=None, capture=None, step=0.5, max_steps=None, every=1,
                 max_points=None, values=True, device=False):
        """The spine-fan skeleton of the nulls of b (3,nz,ny,nx), on the device (semantics: include/ndsm_hip.h,
        ndsm_hip_vecpot_skeleton): each null is typed from its Jacobian - the spine vector, the fan normal, the
        eigenvalues -, then its two spine lines and nring fan lines are traced away from it as paths() traces, and a
        line that comes within `capture` of ANOTHER null ends there (status SKEL_CAPTURED, hit = that null): the fan
        lines that bracket a separator.  nulls: a Nulls tuple (of nulls(), merged) or a (position, jacobian) pair;
        None: self.nulls(b).  radius: the distance of the seeds from their null, capture (None: radius; 0: off) the
        capture radius, both in units of min(h).  ring: (nring,2) coefficients (c_j, s_j) of the fan seeds pos + rho
        (c_j e1 + s_j e2) in the fan basis; None: the angles 2 pi (j + 1/2) / nring.  step, max_steps, every,
        max_points, values as paths().  Returns a Skeleton tuple: position (n,3), kind (n; +-1, +-2 for a spiral, the
        sign that of Nulls.sign; 0: no type), eig (n,3: the spine eigenvalue, the sum and the product of the fan
        eigenvalues), spine, normal (n,3), paths (a FieldPaths of the n (2 + nring) lines: lines.ends (n,L,3),
        length, status, nsteps (n,L); no integral), hit (n,L; -1: not captured).  Line q of null m is lane m L + q:
        q = 0, 1 the spine lines from pos +- rho spine, q = 2 + j ring seed j; spine_of, fan_of and connections
        read the result.  device=True: the arrays are staged in device memory and the device-resident entry point
        runs."""
        radius, capture, ring = _skeleton_args(radius, nring, ring, capture)
        _d0, step, max_steps = self._trace_args(step, max_steps, "forward")
        every, max_points = _paths_args(every, max_points)
        B = self._field_arg(b, "skeleton")
        if nulls is None:
            nulls = self.nulls(B.reshape(tuple(int(v) for v in self.nshape4[::-1])), device=device)
        pos, jac = _skeleton_nulls(nulls)
        n, nr = len(pos), len(ring)
        L = 2 + nr
        nl = n * L
        if nl > TRACE_MAX_SEEDS:
            raise NdsmHipError(f"skeleton: {nl} lines, at most {TRACE_MAX_SEEDS} per call (code 9002)")
        withb = bool(values)
        pernull = [np.zeros(n, dtype=np.int32), np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3))]
        lines = [np.zeros((n, L, 3)), np.zeros((n, L)), np.zeros((n, L), dtype=np.int32),
                 np.zeros((n, L), dtype=np.int32), np.zeros((n, L), dtype=np.int32)]
        if n == 0:
            return _skeleton_tuple(pos, nr, pernull, lines, np.zeros(1, dtype=np.int64), np.zeros((0, 3)),
                                   np.zeros((0, 3)) if withb else None)
        def run(cap):
            offsets, total = np.zeros(nl + 1, dtype=np.int64), np.zeros(1, dtype=np.int64)
            m = max(cap, 1)
            pts = [np.zeros((m, 3)), np.zeros((m, 3)) if withb else None]
            self._entry("ndsm_hip_vecpot_skeleton",
                        [B, n, pos, jac, nr, ring if nr else None, radius, capture, step, max_steps, every, cap, *pernull,
                         *lines, offsets, total.ctypes.data, *[a if cap else None for a in pts]], device)
            return int(total[0]), (offsets, pts)
        k, (offsets, pts) = _with_capacity(run, 0 if max_points is None else max_points)
        return _skeleton_tuple(pos, nr, pernull, lines, offsets, pts[0][:k], None if pts[1] is None else pts[1][:k])

    def separators(self, b, skeleton=None, pairs=None, brackets=None, radius=0.5, capture=None, step=0.5,
                   max_steps=None, rounds=10, tol=1e-12, every=1, ring=None, values=True, device=False):
        """The separator lines between nulls of opposite sign of b (3,nz,ny,nx), on the device (semantics:
        include/ndsm_hip.h, ndsm_hip_vecpot_separators): a bracket - an arc (c_a, s_a, c_b, s_b) of the fan ring of
        null m and a null m' - is refined by one wave, 64 directions a round, until the arc round the change of the
        side on which its fan lines pass m' is narrower than tol; the fan line of its a side is the separator.
        skeleton: a Skeleton of b (None: self.skeleton(b, radius, capture, step, max_steps)); its position, kind and
        normal are used.  brackets: a (pair (nbr,2), arc (nbr,4)) pair; None: for every ordered pair of typed nulls
        with opposite signs of kind (or the caller's `pairs`, a list of (m, m')) the nring cyclically adjacent arcs
        of the skeleton's ring (`ring`: its (nring,2) coefficients when it was not the default one) - most of them
        end in round 1 as SEP_NO_CROSSING; more than 65536 brackets ask for `pairs`.  radius, capture (None: radius;
        it must be > 0 here), step, max_steps, every as skeleton().  Returns a Separators tuple: pair (nbr,2), state
        (nbr; SEP_NONE, SEP_FOUND, SEP_FAR, SEP_NO_CROSSING, SEP_GAP, SEP_UNRESOLVED), coef (nbr,4: the final arc),
        width, side (nbr), dmin (nbr,2), paths (a FieldPaths of the nbr lines, one per bracket; one point where the
        state has no line).  separator_of reads the result.  device=True: the arrays are staged in device memory and
        the device-resident entry point runs."""
        radius, capture, rounds, tol = _separator_args(radius, capture, rounds, tol)
        _d0, step, max_steps = self._trace_args(step, max_steps, "forward")
        every, _mp = _paths_args(every, None)
        R = None if ring is None else _skeleton_ring(0, ring)
        if pairs is not None:
            pairs = np.asarray(pairs)
            if pairs.ndim != 2 or pairs.shape[1] != 2 or pairs.dtype.kind not in "iu":
                raise ValueError(f"pairs must be (npairs, 2) integers, not {pairs.dtype} {pairs.shape}")
        if brackets is not None:
            pair, arc = brackets
            pair, arc = np.asarray(pair), np.ascontiguousarray(np.asarray(arc, dtype=np.float64)).copy()
            if (pair.ndim != 2 or pair.shape[1] != 2 or pair.dtype.kind not in "iu" or arc.shape != (len(pair), 4) or
                    pairs is not None):
                raise ValueError("brackets must be a (pair (nbr, 2) integers, arc (nbr, 4)) pair, given without pairs")
        B = self._field_arg(b, "separators")
        if skeleton is None:
            skeleton = self.skeleton(B.reshape(tuple(int(v) for v in self.nshape4[::-1])), radius=radius, capture=capture,
                                     step=step, max_steps=max_steps, ring=R, values=False, device=device)
        pos = np.ascontiguousarray(np.asarray(skeleton.position, dtype=np.float64)).copy()
        kind = np.ascontiguousarray(np.asarray(skeleton.kind, dtype=np.int32)).copy()
        normal = np.ascontiguousarray(np.asarray(skeleton.normal, dtype=np.float64)).copy()
        n = len(pos)
        if pos.shape != (n, 3) or kind.shape != (n,) or normal.shape != (n, 3):
            raise NdsmHipError(f"separators: a skeleton of shapes {pos.shape}, {kind.shape}, {normal.shape} "
                               "(code 9002)")
        if brackets is None:
            if R is None:
                R = _skeleton_ring(int(np.asarray(skeleton.hit).shape[1]) - 2, None)
            pair, arc = _separator_brackets(kind, R, pairs)
        if len(pair) and (pair.min() < 0 or pair.max() >= n):
            raise ValueError(f"a pair index outside 0 .. {n - 1}")
        pair = np.ascontiguousarray(pair.astype(np.int32))
        nbr = len(pair)
        withb = bool(values)
        per = [np.zeros(nbr, dtype=np.int32), np.zeros(nbr, dtype=np.int32), np.zeros((nbr, 4)), np.zeros(nbr),
               np.zeros(nbr, dtype=np.int32), np.zeros((nbr, 2)), np.zeros((nbr, 3)), np.zeros(nbr),
               np.zeros(nbr, dtype=np.int32), np.zeros(nbr, dtype=np.int32)]
        if nbr == 0:
            return _separators_tuple(pair, per, np.zeros(1, dtype=np.int64), np.zeros((0, 3)),
                                     np.zeros((0, 3)) if withb else None)
        def run(cap):
            offsets, total = np.zeros(nbr + 1, dtype=np.int64), np.zeros(1, dtype=np.int64)
            pts = [np.zeros((cap, 3)), np.zeros((cap, 3)) if withb else None]
            self._entry("ndsm_hip_vecpot_separators", [B, n, pos, kind, normal, nbr, pair, arc, radius, capture, step,
                                                       max_steps, rounds, tol, every, cap, *per, offsets,
                                                       total.ctypes.data, *pts], device)
            return int(total[0]), (offsets, pts)
        # room for a few hundred points per line at first; the call is repeated once when the lines are longer
        k, (offsets, pts) = _with_capacity(run, int(min(nbr * min(-(-max_steps // every) + 2, 512), 2 ** 22)))
        return _separators_tuple(pair, per, offsets, pts[0][:k], None if pts[1] is None else pts[1][:k])

    def seed_plane(self, axis, value, n1, n2):
        """the (n1 n2, 3) seeds of a mesh-aligned cut through the handle's box: coordinate `axis` (0, 1, 2 = x, y, z)
        fixed at `value`, the other two (in the order x, y, z; the first of them fastest) n1 and n2 equally spaced
        points from face to face"""
        return seed_plane(self.x, self.y, self.z, axis, value, n1, n2)

    def seed_cut(self, origin, e1, e2, n1, n2):
        """the (n1 n2, 3) seeds origin + s e1 + t e2 of an oblique cut (see the module's seed_cut)"""
        return seed_cut(self.x, self.y, self.z, origin, e1, e2, n1, n2)

    def field_line_helicity(self, b, seeds, gauge="devore", a=None, step=0.5, max_steps=None, direction="both",
                            niterex_max=10000, ncycles_max=1024, ex_tol=1e-13, vc_tol=1e-10, ms=5, mean=False,
                            mixed_precision=False, flxcrl=False, return_fields=False):
        """Field-line helicity of b (3,nz,ny,nx): the integral of A.dl along the field line through each seed
        (trace() with g = A).  With a (3,nz,ny,nx) given, that A is used and no solve runs (the Helicity is None).
        Otherwise A comes from the helicity chain of the gauge - "devore" (helicity(gauge="devore")) or "coulomb"
        (helicity()) - ON THE DEVICE, and the lines are traced there before anything comes home: b goes up once,
        A and b do not cross PCIe in between.  Returns (FieldLines, Helicity): the lines (flh with
        direction="both") and the Helicity tuple of that chain, the bits helicity(gauge=gauge) returns (with
        return_fields its A, A_p, B_p)."""
        if gauge not in ("devore", "coulomb"):
            raise ValueError(f"gauge must be 'devore' or 'coulomb', not {gauge!r}")
        direction, step, max_steps = self._trace_args(step, max_steps, direction)
        B = self._field_arg(b, "field_line_helicity")
        S = self._seeds_arg(seeds)
        if a is not None:
            inv = {v: k for k, v in _DIRECTIONS.items()}
            return self.trace(b, S, g=a, step=step, max_steps=max_steps, direction=inv[direction]), None
        L = self.L
        out = _trace_outputs(len(S), direction)

        def lines(d):
            """trace on the resident B and A (d: the chain's device arrays)"""
            if len(S) == 0:
                return
            self._entry("ndsm_hip_vecpot_trace", [d["B"], d["A"], len(S), S, step, max_steps, direction, *out], True)

        ioptc, ropt = self._options(niterex_max, ncycles_max, ex_tol, vc_tol, ms, mean, mixed_precision, flxcrl)
        if gauge == "devore":
            hel = self._devore_chain(B, ioptc, ropt, False, return_fields, 0, after=lines)
            return _field_lines(out, direction), hel
        shape = tuple(int(v) for v in self.nshape4[::-1])
        d = {}
        o8 = np.zeros(8)
        host = {}
        try:
            for k in ("B", "A", "Ap", "Bp"):
                d[k] = ctypes.c_void_p()
                _check(L.ndsm_hip_device_alloc(B.nbytes, ctypes.byref(d[k])), "device_alloc", L)
            _check(L.ndsm_hip_memcpy_h2d(d["B"], B.ctypes.data, B.nbytes), "h2d", L)
            ierr = L.ndsm_hip_vecpot_helicity_device(self.h, ioptc.ctypes.data_as(_ip), _d(ropt), d["B"], d["A"],
                                                     d["Ap"], d["Bp"], _d(o8))
            if ierr >= 9000:
                _check(ierr, "ndsm_hip_vecpot_helicity_device", L)
            self.last_ioptc, self.last_ropt = ioptc, ropt
            lines(d)
            for k in (("A", "Ap", "Bp") if return_fields else ()):
                host[k] = np.empty(B.size)
                _check(L.ndsm_hip_memcpy_d2h(host[k].ctypes.data, d[k], B.nbytes), "d2h", L)
        finally:
            for p in d.values():
                L.ndsm_hip_device_free(p)
        f = {k: v.reshape(shape) for k, v in host.items()}
        return _field_lines(out, direction), _helicity_tuple(ierr, o8, f.get("A"), f.get("Ap"), f.get("Bp"))

    def project(self, b, niterex_max=10000, ncycles_max=1024, ex_tol=1e-13, vc_tol=1e-10, ms=5, mean=False,
                mixed_precision=False, flxcrl=False, device=False, return_phi=False):
        """Solenoidal projection (divergence cleaning) of b (3,nz,ny,nx): B' = b - G_h phi with laplace_7(phi) =
        div_h b - c, all six faces Neumann, c = sum w div_h b / sum w.  B.n on the six faces is left bitwise
        as it is, so the potential field does not change; c (net boundary flux / volume) cannot be removed by
        such a projection and stays in div_h B'.  Approximate (collocated): div_h B' is O(h^2) relative to
        what was removed, not zero.  Options as for solve_field; the solve is always fp64 (mixed_precision and
        flxcrl are accepted and ignored).  Returns a Projection tuple: ierr (0 the solve reached vc_tol, else
        1), B', phi (return_phi, else None), c, divB_before / divB_after (max |div_h|), E_removed =
        1/2 sum w |G_h phi|^2, ncycles, du_last.  device=True: the device-resident entry point runs."""
        shape = tuple(int(v) for v in self.nshape4[::-1])
        B = self._field_arg(b, "project")
        ioptc, ropt = self._options(niterex_max, ncycles_max, ex_tol, vc_tol, ms, mean, 0, False)
        phi = np.zeros(B.size // 3) if return_phi else None
        out = np.zeros(4)
        if not device:
            ierr = self.L.ndsm_hip_vecpot_project(self.h, ioptc.ctypes.data_as(_ip), _d(ropt), _d(B),
                                                  _d(phi) if return_phi else None, _d(out))
        else:
            arrays = [B, phi] if return_phi else [B]
            ierr = self._on_device(arrays, lambda dB, dphi=None: self.L.ndsm_hip_vecpot_project_device(
                self.h, ioptc.ctypes.data_as(_ip), _d(ropt), dB, dphi, _d(out)))
        if ierr >= 9000:
            _check(ierr, "ndsm_hip_vecpot_project", self.L)
        self.last_ioptc, self.last_ropt = ioptc, ropt
        p = Projection(int(ierr), B.reshape(shape), phi.reshape(shape[1:]) if return_phi else None, float(out[0]),
                       float(out[1]), float(out[2]), float(out[3]), int(ioptc[self.L.get_iopt_ncyc_out()]),
                       float(ropt[self.L.get_ropt_dulast()]))
        self.last_projection = p
        return p


Projection = collections.namedtuple("Projection", ["ierr", "B", "phi", "c", "divB_before", "divB_after", "E_removed",
                                                   "ncycles", "du_last"])


Helicity = collections.namedtuple("Helicity", ["ierr", "H_R", "H_J", "E", "E_p", "E_free", "recon_max", "recon_rms",
                                               "divB_max", "divA_max", "A", "A_p", "B_p"])


def _with_capacity(run, cap, count_only=False):
    """The two-attempt capacity rule of the entries with results of unknown length: run(cap) makes the call with room
    for cap records and returns (the number there are, its arrays); when that number is more than cap the call is made
    once more with that number (count_only: not from cap 0, which asks for the count alone).  Returns (the number of
    records the last call stored, its arrays)."""
    total, arrays = run(cap)
    if total > cap and not (count_only and cap == 0):
        cap = total
        total, arrays = run(cap)
    return min(total, cap), arrays


def _descent_options(niter_max, check, tol, dt0, dt_min, hist_rows, width, nlevels=None):
    """The options every descent (optimize, optimize_obs, optimize_cascade, preprocess) shares, checked: niter_max, dt0
    and dt_min are lists, one entry per level (a dt0 or dt_min of None is left for _descent_steps).  Returns (hist_rows
    - None: one row per check of the longest level and two more -, hist, info): the zeroed buffers of the call, hist
    (hist_rows, width) and info (3), with nlevels a leading axis of that length on both."""
    for name, v in [("niter_max", v) for v in niter_max] + [("check", check)]:
        if int(v) != v or v < 1:
            raise ValueError(f"{name} must be a whole number >= 1, not {v!r}")
    if not (tol >= 0.0 and np.isfinite(tol)):
        raise ValueError(f"tol must be finite and >= 0, not {tol!r}")
    for v in dt0:
        if v is not None and not (v > 0.0 and np.isfinite(v)):
            raise ValueError(f"dt0 must be finite and > 0, not {v!r}")
    for v in dt_min:
        if v is not None and not (v >= 0.0 and np.isfinite(v)):
            raise ValueError(f"dt_min must be finite and >= 0, not {v!r}")
    if hist_rows is None:
        hist_rows = -(-int(max(niter_max)) // int(check)) + 2
    if int(hist_rows) != hist_rows or hist_rows < 2:
        raise ValueError(f"hist_rows must be a whole number >= 2, not {hist_rows!r}")
    lead = () if nlevels is None else (nlevels,)
    return hist_rows, np.zeros(lead + (int(hist_rows), width)), np.zeros(lead + (3,), dtype=np.intc)


def _per_level(name, v, nlevels):
    """a per-level option of a cascade as a list: one value for every level, or a sequence with one per level"""
    if isinstance(v, (list, tuple, np.ndarray)):
        if len(v) != nlevels:
            raise ValueError(f"{name} needs one value per level ({nlevels}), not {len(v)}")
        return list(v)
    return [v] * nlevels


def _descent_steps(dt0, dt_min, dt0_default):
    """the first and the smallest step with their defaults: dt0_default, 1e-6 dt0"""
    if dt0 is None:
        dt0 = dt0_default
    if dt_min is None:
        dt_min = 1e-6 * dt0
    return dt0, dt_min


def _descent_result(hist, info):
    """(the written rows of hist, info as a tuple of ints) of one descent"""
    return hist[:int(info[0])].copy(), tuple(int(v) for v in info)


def _helicity_tuple(ierr, out, A, Ap, Bp):
    """a Helicity from the out[8] of the helicity / devore entries"""
    return Helicity(int(ierr), float(out[0]), float(out[1]), float(out[2]), float(out[3]), float(out[2] - out[3]),
                    float(out[4]), float(out[5]), float(out[6]), float(out[7]), A, Ap, Bp)


FieldLines = collections.namedtuple("FieldLines", ["ends", "length", "integral", "status", "nsteps", "flh"])

# status codes of a traced line (NDSM_HIP_TRACE_* in include/ndsm_hip.h): the face it left through, or why it stopped
TRACE_XLO, TRACE_XHI, TRACE_YLO, TRACE_YHI, TRACE_ZLO, TRACE_ZHI, TRACE_NULL, TRACE_UNFINISHED, TRACE_OUTSIDE = \
    range(1, 10)
TRACE_MAX_STEPS = 2 ** 24          # the library's ceiling of max_steps
TRACE_MAX_SEEDS = 2 ** 30 - 1      # per call (2 nseeds lines fit a C int)
_DIRECTIONS = {"forward": 1, "backward": -1, "both": 0}


def _trace_outputs(nseeds, direction):
    """[ends, length, integral, status, nsteps] of ndsm_hip_vecpot_trace for nseeds seeds, zeroed"""
    nd = 2 if direction == 0 else 1
    return [np.zeros((nd, nseeds, 3)), np.zeros((nd, nseeds)), np.zeros((nd, nseeds)),
            np.zeros((nd, nseeds), dtype=np.int32), np.zeros((nd, nseeds), dtype=np.int32)]


def _field_lines(out, direction):
    return FieldLines(*out, out[2][0] + out[2][1] if direction == 0 else None)


FieldPaths = collections.namedtuple("FieldPaths", ["lines", "offsets", "points", "b", "g", "integral"])
PATHS_MAX_POINTS = 2 ** 40         # capacity of one paths() call


def _paths_args(every, max_points):
    """(every, max_points) of paths(); ValueError before anything is launched"""
    def whole(v):
        return (not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating)) and np.isfinite(v)
                and int(v) == v)
    if not whole(every) or not 1 <= every <= 2 ** 31 - 1:
        raise ValueError(f"every must be an integer >= 1, not {every!r}")
    if max_points is not None and (not whole(max_points) or not 0 <= max_points <= PATHS_MAX_POINTS):
        raise ValueError(f"max_points must be None or an integer in 0 .. {PATHS_MAX_POINTS}, not {max_points!r}")
    return int(every), None if max_points is None else int(max_points)


def _field_paths(out, direction, offsets, points, b, g, integral):
    return FieldPaths(_field_lines(out, direction), offsets, points, b, g, integral)


def path_of(paths, l):
    """the rows of line l of a FieldPaths (lane order: l = i forward, nseeds + i backward for direction "both"):
    (points, b, g, integral), an absent array None"""
    nl = len(paths.offsets) - 1
    if int(l) != l or not 0 <= l < nl:
        raise IndexError(f"line {l!r} of {nl}")
    a, e = int(paths.offsets[int(l)]), int(paths.offsets[int(l) + 1])
    return tuple(None if v is None else v[a:e] for v in (paths.points, paths.b, paths.g, paths.integral))


def whole_line(paths, i):
    """the whole line through seed i of a FieldPaths traced in both directions: the backward line reversed, then the
    forward line, the seed once - from the foot where b enters the box to the foot where it leaves.  (points, b, g,
    integral), each joined the same way; integral is the integral of g.dl from the entry foot up to each point (the
    backward line's values are counted back from its total)."""
    if paths.lines.ends.shape[0] != 2:
        raise ValueError("whole_line needs paths traced with direction='both'")
    ns = paths.lines.ends.shape[1]
    if int(i) != i or not 0 <= i < ns:
        raise IndexError(f"seed {i!r} of {ns}")
    fwd, bwd = path_of(paths, int(i)), path_of(paths, ns + int(i))
    joined = [None if f is None else np.concatenate([w[:0:-1], f]) for f, w in zip(fwd[:3], bwd[:3])]
    integral = None
    if fwd[3] is not None:
        # a backward line accumulates g.dl in the direction of b from its points to the seed
        integral = np.concatenate([bwd[3][-1] - bwd[3][:0:-1], bwd[3][-1] + fwd[3]])
    return tuple(joined) + (integral,)


NULLS_MAX = 2 ** 24               # capacity of one nulls() call: 128 B of host arrays per slot
Nulls = collections.namedtuple("Nulls", ["position", "cell", "jacobian", "sign", "spiral", "eigenvalues", "spine", "fan",
                                          "det", "residual", "ncandidates", "nfound"])


def _nulls_tuple(rec, ncandidates, nfound, radius):
    """a Nulls tuple from the records [cell, pos, jac, det, resid, sign, iters] in cell order: records within
    `radius` of one already kept are dropped (None: none is), the types follow from numpy.linalg.eig"""
    cell, pos, jac, det, resid, sign, _iters = rec
    keep = np.ones(len(cell), dtype=bool)
    if radius is not None:
        for i in range(len(cell)):
            if keep[i]:
                near = np.sqrt(((pos[i + 1:] - pos[i]) ** 2).sum(axis=1)) <= radius
                keep[i + 1:] &= ~near
    cell, pos, jac, det, resid, sign = (a[keep].copy() for a in (cell, pos, jac, det, resid, sign))
    n = len(cell)
    lam, spine, fan = np.zeros((n, 3), dtype=complex), np.zeros((n, 3)), np.zeros((n, 2, 3), dtype=complex)
    for i in range(n):
        w, v = np.linalg.eig(jac[i])
        # the lone sign: the real eigenvalue whose real part's sign the other two do not share (for det = 0 or a
        # pure centre no such eigenvalue need exist: then the real eigenvalue of the largest modulus)
        sg = np.sign(w.real)
        lone = [k for k in range(3) if abs(w[k].imag) == 0.0 and sg[k] != 0 and np.all(np.delete(sg, k) == -sg[k])]
        if not lone:
            lone = sorted((k for k in range(3) if abs(w[k].imag) == 0.0), key=lambda k: -abs(w[k]))
        k = lone[0]
        rest = [j for j in range(3) if j != k]
        lam[i] = w[[k] + rest]
        spine[i] = v[:, k].real
        fan[i] = v[:, rest].T
    spiral = np.abs(lam.imag).max(axis=1) > 0.0 if n else np.zeros(0, dtype=bool)
    if np.all(fan.imag == 0.0):
        fan = fan.real
    return Nulls(pos, cell, jac, sign, spiral, lam, spine, fan, det, resid, ncandidates, nfound)


Skeleton = collections.namedtuple("Skeleton", ["position", "kind", "eig", "spine", "normal", "paths", "hit"])
SKEL_CAPTURED, SKEL_NONE = 10, 11  # status codes of a skeleton line beyond TRACE_* (NDSM_HIP_SKEL_*)


def _skeleton_ring(nring, ring):
    """the (nring,2) coefficients (c_j, s_j) of the fan seeds: `ring` as given, or the angles 2 pi (j + 1/2) / nring"""
    if ring is not None:
        R = np.ascontiguousarray(np.asarray(ring, dtype=np.float64))
        if R.ndim != 2 or R.shape[1] != 2:
            raise ValueError(f"ring must have the shape (nring, 2), not {R.shape}")
        return R.copy()
    if (isinstance(nring, bool) or not isinstance(nring, (int, np.integer)) or not 0 <= nring <= 2 ** 20):
        raise ValueError(f"nring must be an integer in 0 .. {2 ** 20}, not {nring!r}")
    ang = 2.0 * np.pi * (np.arange(int(nring)) + 0.5) / max(int(nring), 1)
    return np.stack([np.cos(ang), np.sin(ang)], axis=1).reshape(int(nring), 2)


def _skeleton_args(radius, nring, ring, capture):
    """(radius, capture, ring) of skeleton(); ValueError before anything is launched"""
    def number(v):
        return not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating)) and np.isfinite(v)
    if not number(radius) or not radius > 0.0:
        raise ValueError(f"radius must be a positive finite number, not {radius!r}")
    if capture is None:
        capture = radius
    if not number(capture) or capture < 0.0:
        raise ValueError(f"capture must be None or a finite number >= 0, not {capture!r}")
    return float(radius), float(capture), _skeleton_ring(nring, ring)


DIPS_MAX = 2 ** 28                # capacity of one dips() call: 92 B of host arrays per slot
Dips = collections.namedtuple("Dips", ["position", "edge", "axis", "node", "b", "grad", "curv", "kappa", "bald",
                                        "ncrossings", "ndips", "nbald"])


def _dips_args(plane_only, max_dips):
    """(plane_only as 0 / 1, max_dips or None) of dips(); ValueError before anything is launched"""
    if not isinstance(plane_only, (bool, np.bool_)):
        raise ValueError(f"plane_only must be True or False, not {plane_only!r}")
    if max_dips is not None and (isinstance(max_dips, bool) or
                                 not isinstance(max_dips, (int, float, np.integer, np.floating)) or
                                 not np.isfinite(max_dips) or int(max_dips) != max_dips or
                                 not 0 <= max_dips <= DIPS_MAX):
        raise ValueError(f"max_dips must be None or an integer in 0 .. {DIPS_MAX}, not {max_dips!r}")
    return int(bool(plane_only)), None if max_dips is None else int(max_dips)


def _dips_tuple(rec, counts, nx, ny):
    """a Dips tuple from the records [edge, pos, bpt, grad, curv, flag] and counts (crossings, dips, bald patches)"""
    edge, pos, bpt, grad, curv, flag = rec
    node = edge // 3
    ijk = np.stack([node % nx, (node // nx) % ny, node // (nx * ny)], axis=1)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        kappa = curv / (bpt[:, 0] * bpt[:, 0] + bpt[:, 1] * bpt[:, 1])
    return Dips(pos, edge, (edge % 3).astype(np.int32), ijk, bpt, grad, curv, kappa, (flag & 1).astype(bool),
                int(counts[0]), int(counts[1]), int(counts[2]))


def _bald_seeds(dips, lift, hz):
    """the seeds of bald_patch_lines: position + (0, 0, lift hz) of the records with bald"""
    pos, bald = np.asarray(dips.position, dtype=np.float64), np.asarray(dips.bald, dtype=bool)
    if pos.ndim != 2 or pos.shape[1] != 3 or bald.shape != pos.shape[:1]:
        raise NdsmHipError(f"bald_patch_lines: dips of shapes {pos.shape}, {bald.shape}: (n, 3) and (n) are needed "
                           "(code 9002)")
    return pos[bald] + np.array([0.0, 0.0, float(lift) * hz])


def _skeleton_nulls(nulls):
    """(pos (n,3), jac (n,3,3)) of a Nulls tuple or a (position, jacobian) pair, contiguous copies"""
    if hasattr(nulls, "position") and hasattr(nulls, "jacobian"):
        pos, jac = nulls.position, nulls.jacobian
    else:
        pos, jac = nulls
    pos = np.ascontiguousarray(np.asarray(pos, dtype=np.float64)).copy()
    jac = np.ascontiguousarray(np.asarray(jac, dtype=np.float64)).copy()
    if pos.ndim != 2 or pos.shape[1] != 3 or jac.shape != (len(pos), 3, 3):
        raise NdsmHipError(f"skeleton: nulls of shapes {pos.shape}, {jac.shape}: (n, 3) and (n, 3, 3) are needed "
                           "(code 9002)")
    return pos, jac


def _skeleton_tuple(pos, nring, pernull, lines, offsets, points, b):
    """a Skeleton from [kind, eig, spine, normal], [ends, length, status, nsteps, hit] (lane order) and the points"""
    n, L = len(pos), 2 + nring
    ends, length, status, nsteps, hit = lines
    fl = FieldLines(ends.reshape(n, L, 3), length.reshape(n, L), None, status.reshape(n, L), nsteps.reshape(n, L), None)
    return Skeleton(pos, *pernull, FieldPaths(fl, offsets, points, b, None, None), hit.reshape(n, L))


def _skeleton_null(sk, m):
    n = len(sk.position)
    if int(m) != m or not 0 <= m < n:
        raise IndexError(f"null {m!r} of {n}")
    return int(m), sk.hit.shape[1]


def spine_of(sk, m):
    """the two spine lines of null m of a Skeleton: [(points, b), (points, b)], from pos + rho spine and from
    pos - rho spine, each running away from the null (b None with values=False)"""
    m, L = _skeleton_null(sk, m)
    return [path_of(sk.paths, m * L + q)[:2] for q in (0, 1)]


def fan_of(sk, m):
    """the fan lines of null m of a Skeleton, one per ring seed: [(points, b), ...]"""
    m, L = _skeleton_null(sk, m)
    return [path_of(sk.paths, m * L + q)[:2] for q in range(2, L)]


def connections(sk):
    """the null-to-null connections of a Skeleton: a list of (m, m', ring indices) - the fan lines of null m that
    were captured by null m', ascending in m, then m'.  Neighbouring ring indices bracket a separator from m to m'."""
    out = []
    fan_hit = sk.hit[:, 2:]
    captured = sk.paths.lines.status[:, 2:] == SKEL_CAPTURED
    for m in range(len(sk.position)):
        for other in np.unique(fan_hit[m][captured[m]]):
            out.append((m, int(other), np.nonzero(captured[m] & (fan_hit[m] == other))[0]))
    return out


Separators = collections.namedtuple("Separators", ["pair", "state", "coef", "width", "side", "dmin", "paths"])
# states of a bracket (NDSM_HIP_SEP_*)
SEP_NONE, SEP_FOUND, SEP_FAR, SEP_NO_CROSSING, SEP_GAP, SEP_UNRESOLVED = range(6)
SEP_MAX_BRACKETS = 65536           # default brackets of one separators() call


def _separator_args(radius, capture, rounds, tol):
    """(radius, capture, rounds, tol) of separators(); ValueError before anything is launched"""
    def number(v):
        return not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating)) and np.isfinite(v)
    if not number(radius) or not radius > 0.0:
        raise ValueError(f"radius must be a positive finite number, not {radius!r}")
    if capture is None:
        capture = radius
    if not number(capture) or not capture > 0.0:
        raise ValueError(f"capture must be None or a positive finite number, not {capture!r}")
    if not number(rounds) or int(rounds) != rounds or not 1 <= rounds <= 2 ** 31 - 1:
        raise ValueError(f"rounds must be an integer >= 1, not {rounds!r}")
    if not number(tol) or tol < 0.0:
        raise ValueError(f"tol must be a finite number >= 0, not {tol!r}")
    return float(radius), float(capture), int(rounds), float(tol)


def _separator_brackets(kind, ring, pairs=None):
    """the default brackets: for every ordered pair (m, m') of typed nulls with opposite signs of kind (or `pairs`) the
    nring arcs (ring_j, ring_(j+1) cyclically), pair by pair, j ascending: pair (nbr,2) int32, arc (nbr,4)"""
    kind = np.asarray(kind)
    nr = len(ring)
    if pairs is None:
        plus, minus = np.nonzero(kind > 0)[0], np.nonzero(kind < 0)[0]
        if 2 * len(plus) * len(minus) * nr > SEP_MAX_BRACKETS:
            raise ValueError(f"{2 * len(plus) * len(minus)} pairs of nulls with {nr} arcs each are more than "
                             f"{SEP_MAX_BRACKETS} brackets: name the pairs to refine with pairs=")
        pairs = sorted([(int(m), int(o)) for m in plus for o in minus] + [(int(o), int(m)) for m in plus for o in minus])
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    if len(pairs) * nr > SEP_MAX_BRACKETS:
        raise ValueError(f"{len(pairs)} pairs with {nr} arcs each are more than {SEP_MAX_BRACKETS} brackets: name fewer "
                         "pairs")
    arcs = np.concatenate([ring, np.roll(ring, -1, axis=0)], axis=1).reshape(nr, 4)
    pair = np.repeat(pairs, nr, axis=0).astype(np.int32).reshape(-1, 2)
    return np.ascontiguousarray(pair), np.ascontiguousarray(np.tile(arcs, (len(pairs), 1))).reshape(-1, 4)


def _separators_tuple(pair, per, offsets, points, b):
    """a Separators from [state, nrounds, coef, width, side, dmin, ends, length, status, nsteps] and the points"""
    state, _nrounds, coef, width, side, dmin, ends, length, status, nsteps = per
    fl = FieldLines(ends, length, None, status, nsteps, None)
    return Separators(pair, state, coef, width, side, dmin, FieldPaths(fl, offsets, points, b, None, None))


def separator_of(result, m, m2):
    """the separators from null m to null m2 of a Separators: [(points, b), ...], one per SEP_FOUND bracket of that
    pair, each running from m to within the capture radius of m2 (b None with values=False)"""
    for v in (m, m2):
        if int(v) != v or v < 0:
            raise IndexError(f"null {v!r}")
    rows = np.nonzero((result.pair[:, 0] == m) & (result.pair[:, 1] == m2) & (result.state == SEP_FOUND))[0]
    return [path_of(result.paths, int(l))[:2] for l in rows]


QMap = collections.namedtuple("QMap", ["q", "twist", "ends", "length", "integral", "status", "nsteps"])


def _qmap(out, twist):
    """a QMap from [q, ends, length, integral, status, nsteps]; twist = (I_fwd + I_bwd) / 4 pi, NaN where q is"""
    tw = None
    if twist:
        tw = np.where(np.isnan(out[0]), np.nan, (out[3][0] + out[3][1]) / (4.0 * np.pi))
    return QMap(out[0], tw, *out[1:])


def seed_plane(x, y, z, axis, value, n1, n2):
    """the (n1 n2, 3) seeds of a cut through the box of the mesh x, y, z normal to `axis` (0, 1, 2) at `value`: n1 by
    n2 equally spaced points from face to face along the other two axes (in the order x, y, z; the first of them
    fastest), the box as the library forms it (lo = q[0], hi = lo + (n - 1) (q[1] - q[0]))"""
    if axis not in (0, 1, 2) or isinstance(axis, bool):
        raise ValueError(f"axis must be 0, 1 or 2, not {axis!r}")
    if int(n1) != n1 or int(n2) != n2 or n1 < 1 or n2 < 1:
        raise ValueError(f"n1 and n2 must be integers >= 1, not {n1!r}, {n2!r}")
    q = [_f64(v) for v in (x, y, z)]
    lo = [float(v[0]) for v in q]
    hi = [float(v[0]) + (len(v) - 1.0) * (float(v[1]) - float(v[0])) for v in q]
    a1, a2 = [d for d in range(3) if d != axis]
    u1 = lo[a1] + (hi[a1] - lo[a1]) * (np.arange(int(n1)) / max(int(n1) - 1, 1))
    u2 = lo[a2] + (hi[a2] - lo[a2]) * (np.arange(int(n2)) / max(int(n2) - 1, 1))
    u1, u2 = np.minimum(u1, hi[a1]), np.minimum(u2, hi[a2])
    out = np.empty((int(n2), int(n1), 3))
    out[:, :, axis] = float(value)
    out[:, :, a1] = u1[None, :]
    out[:, :, a2] = u2[:, None]
    return out.reshape(-1, 3)


QPerpMap = collections.namedtuple("QPerpMap", ["q", "q_perp", "twist", "ends", "length", "integral", "status",
                                              "nsteps"])


def _qperpmap(q, qperp, lines, twist):
    """a QPerpMap from q, q_perp and [ends, length, integral, status, nsteps]; twist = (I_fwd + I_bwd) / 4 pi, NaN
    where q_perp is"""
    tw = None
    if twist:
        tw = np.where(np.isnan(qperp), np.nan, (lines[2][0] + lines[2][1]) / (4.0 * np.pi))
    return QPerpMap(q, qperp, tw, *lines)


def seed_cut(x, y, z, origin, e1, e2, n1, n2):
    """the (n1 n2, 3) seeds origin + s e1 + t e2 of an oblique cut through the mesh x, y, z: s and t n1 and n2 equally
    spaced values in [0, 1] (a single one: 0), s fastest - the ordering of seed_plane, whose mesh-aligned cuts this
    complements.  origin, e1, e2: three finite numbers each, in physical coordinates.  Points outside the box are
    allowed: their lines come back with TRACE_OUTSIDE.  (The mesh takes no part: the cut is the caller's.)"""
    if int(n1) != n1 or int(n2) != n2 or n1 < 1 or n2 < 1:
        raise ValueError(f"n1 and n2 must be integers >= 1, not {n1!r}, {n2!r}")
    vec = []
    for name, v in (("origin", origin), ("e1", e1), ("e2", e2)):
        try:
            a = np.asarray(v, dtype=np.float64)
        except (TypeError, ValueError):
            a = None
        if a is None or a.shape != (3,) or not np.all(np.isfinite(a)):
            raise ValueError(f"{name} must be three finite numbers, not {v!r}")
        vec.append(a)
    s = np.arange(int(n1)) / max(int(n1) - 1, 1)
    t = np.arange(int(n2)) / max(int(n2) - 1, 1)
    out = vec[0][None, None, :] + s[None, :, None] * vec[1][None, None, :] + t[:, None, None] * vec[2][None, None, :]
    return out.reshape(-1, 3)


def _grid_handle(x, y, z, b, ngrids, lib):
    shape = np.shape(b)
    want = (3, len(z), len(y), len(x))
    if tuple(shape) != want:
        raise NdsmHipError(f"field of shape {tuple(shape)}, the mesh needs {want} (code 9002)")
    return VecPot(x, y, z, ngrids=ngrids, lib=lib)


def vector_potential_field(x, y, z, b, a_init=None, niterex_max=10000, ncycles_max=1024, ex_tol=1e-13, vc_tol=1e-10,
                           ms=5, mean=False, mixed_precision=False, flxcrl=False, ngrids=0, lib=None):
    """Vector potential A of the whole field b (3,nz,ny,nx) - curl b != 0 allowed - in the Coulomb gauge of
    `vector_potential`, with the same tangential boundary values as its potential-field A_p.  One-shot form of
    VecPot.solve_field: returns (ierr, A, B_rec), B_rec = curl A + flux-balance fields.  Raises NdsmHipError on
    device / runtime failures (>= 9001)."""
    V = _grid_handle(x, y, z, b, ngrids, lib)
    try:
        return V.solve_field(b, a_init=a_init, niterex_max=niterex_max, ncycles_max=ncycles_max, ex_tol=ex_tol,
                             vc_tol=vc_tol, ms=ms, mean=mean, mixed_precision=mixed_precision, flxcrl=flxcrl)
    finally:
        V.close()


def relative_helicity(x, y, z, b, niterex_max=10000, ncycles_max=1024, ex_tol=1e-13, vc_tol=1e-10, ms=5, mean=False,
                      mixed_precision=False, flxcrl=False, ngrids=0, return_fields=False, project=False, lib=None,
                      gauge="coulomb"):
    """Relative helicity, energies and reconstruction diagnostics of b (3,nz,ny,nx): one-shot form of
    VecPot.helicity (returns its Helicity tuple; project=True: of the solenoidal projection of b; gauge="devore":
    A_z = 0, "both": the (coulomb, devore) pair).  Raises NdsmHipError on device / runtime failures (>= 9001)."""
    if gauge not in ("coulomb", "devore", "both"):
        raise ValueError(f"gauge must be 'coulomb', 'devore' or 'both', not {gauge!r}")
    V = _grid_handle(x, y, z, b, ngrids, lib)
    try:
        return V.helicity(b, niterex_max=niterex_max, ncycles_max=ncycles_max, ex_tol=ex_tol, vc_tol=vc_tol, ms=ms,
                          mean=mean, mixed_precision=mixed_precision, flxcrl=flxcrl, return_fields=return_fields,
                          project=project, gauge=gauge)
    finally:
        V.close()


def devore_potentials(x, y, z, b, bp, lib=None):
    """DeVore-gauge (A_z = 0) vector potentials of b and bp (3,nz,ny,nx) and the helicity with them: one-shot form
    of VecPot.devore (returns its Helicity tuple, A and A_p filled).  No solve: bp is the caller's field with b's
    B.n (e.g. vector_potential's B).  Raises NdsmHipError on device / runtime failures (>= 9001)."""
    V = _grid_handle(x, y, z, b, 0, lib)
    try:
        return V.devore(b, bp)
    finally:
        V.close()


def trace_field_lines(x, y, z, b, seeds, g=None, step=0.5, max_steps=None, direction="both", lib=None):
    """Field lines of b (3,nz,ny,nx) through seeds (nseeds,3) and the line integral of g along them: one-shot form
    of VecPot.trace (returns its FieldLines tuple).  Raises NdsmHipError on device / runtime failures (>= 9001)."""
    V = _grid_handle(x, y, z, b, 0, lib)
    try:
        return V.trace(b, seeds, g=g, step=step, max_steps=max_steps, direction=direction)
    finally:
        V.close()


def boundary_alpha(x, y, b, bz_min):
    """alpha0 (ny,nx) of a field b (3,nz,ny,nx) on its lower face k = 0: (d_x B_y - d_y B_x) / B_z with numpy's
    second-order differences (np.gradient, edge_order=2) on the mesh vectors x, y; 0 where |B_z| < bz_min.  Plain
    numpy: the input of force_free() and map_alpha()."""
    b = np.asarray(b, dtype=np.float64)
    bx, by, bz = b[0, 0], b[1, 0], b[2, 0]
    jz = np.gradient(by, _f64(x), axis=1, edge_order=2) - np.gradient(bx, _f64(y), axis=0, edge_order=2)
    weak = np.abs(bz) < bz_min
    return np.where(weak, 0.0, jz / np.where(weak, 1.0, bz))


def map_alpha(x, y, z, b, alpha0, polarity=1, step=0.5, max_steps=None, lib=None):
    """alpha0 (ny,nx) on the lower face carried along the field lines of b (3,nz,ny,nx) to every node: one-shot form
    of VecPot.alpha_map (returns its (alpha, status)).  Raises NdsmHipError on device / runtime failures (>= 9001)."""
    V = _grid_handle(x, y, z, b, 0, lib)
    try:
        return V.alpha_map(b, alpha0, polarity=polarity, step=step, max_steps=max_steps)
    finally:
        V.close()


def vector_potential_current(x, y, z, b, j, a_init=None, niterex_max=10000, ncycles_max=1024, ex_tol=1e-13,
                             vc_tol=1e-10, ms=5, mean=False, mixed_precision=False, flxcrl=False, ngrids=0, lib=None):
    """Vector potential of a prescribed current j (3,nz,ny,nx) with the B.n of b on the six faces: one-shot form of
    VecPot.solve_current (returns its (ierr, A, B)).  Raises NdsmHipError on device / runtime failures (>= 9001)."""
    V = _grid_handle(x, y, z, b, ngrids, lib)
    try:
        return V.solve_current(b, j, a_init=a_init, niterex_max=niterex_max, ncycles_max=ncycles_max, ex_tol=ex_tol,
                               vc_tol=vc_tol, ms=ms, mean=mean, mixed_precision=mixed_precision, flxcrl=flxcrl)
    finally:
        V.close()


def force_free_field(x, y, z, b, alpha0, polarity=1, start="potential", a_init=None, niter_max=20, tol=0.0, step=0.5,
                     max_steps=None, niterex_max=10000, ncycles_max=1024, ex_tol=1e-13, vc_tol=1e-10, ms=5, mean=False,
                     mixed_precision=False, flxcrl=False, ngrids=0, lib=None):
    """Nonlinear force-free field from the B.n of b (3,nz,ny,nx) and alpha0 (ny,nx) on the lower face (e.g.
    boundary_alpha's) by the Grad-Rubin iteration: one-shot form of VecPot.force_free (returns its (ierr, A, B, alpha,
    status, hist)).  Raises NdsmHipError on device / runtime failures (>= 9001)."""
    V = _grid_handle(x, y, z, b, ngrids, lib)
    try:
        return V.force_free(b, alpha0, polarity=polarity, start=start, a_init=a_init, niter_max=niter_max, tol=tol,
                            step=step, max_steps=max_steps, niterex_max=niterex_max, ncycles_max=ncycles_max,
                            ex_tol=ex_tol, vc_tol=vc_tol, ms=ms, mean=mean, mixed_precision=mixed_precision,
                            flxcrl=flxcrl)
    finally:
        V.close()


def boundary_weight(shape, nd):
    """The weight function w (nz,ny,nx) of optimize() for a grid of that shape: 1 inside, and over the nd nodes next
    to the two side faces in x, the two in y and the top face a cosine fall 1/2 (1 + cos(pi (nd - d) / nd)), d the
    node distance to the face (0 on the face itself); the per-axis factors are multiplied.  The lower face - the
    magnetogram - is untouched.  nd = 0 gives ones.  Plain numpy."""
    nz, ny, nx = (int(v) for v in shape)
    nd = int(nd)
    if nd < 0:
        raise ValueError(f"nd must be >= 0, not {nd!r}")

    def profile(n, both):
        f = np.ones(n)
        for d in range(min(nd, n)):
            v = 0.5 * (1.0 + np.cos(np.pi * (nd - d) / nd))
            f[n - 1 - d] = min(f[n - 1 - d], v)
            if both:
                f[d] = min(f[d], v)
        return f
    return (profile(nz, False)[:, None, None] * profile(ny, True)[None, :, None]) * profile(nx, True)[None, None, :]


def force_free_optimize(x, y, z, b, w=None, start="potential", niter_max=10000, check=50, tol=1e-4, dt0=None,
                        dt_min=None, hist_rows=None, niterex_max=10000, ncycles_max=1024, ex_tol=1e-13, vc_tol=1e-10,
                        ms=5, mean=False, mixed_precision=False, flxcrl=False, ngrids=0, lib=None):
    """Nonlinear force-free field from the vector magnetogram on the lower face of b (3,nz,ny,nx) by the optimization
    method: one-shot form of VecPot.optimize (returns its (ierr, B, hist, info)).  Raises NdsmHipError on device /
    runtime failures (>= 9001)."""
    V = _grid_handle(x, y, z, b, ngrids, lib)
    try:
        return V.optimize(b, w=w, start=start, niter_max=niter_max, check=check, tol=tol, dt0=dt0, dt_min=dt_min,
                          hist_rows=hist_rows, niterex_max=niterex_max, ncycles_max=ncycles_max, ex_tol=ex_tol,
                          vc_tol=vc_tol, ms=ms, mean=mean, mixed_precision=mixed_precision, flxcrl=flxcrl)
    finally:
        V.close()


def measurement_weight(bobs, floor=0.0):
    """The confidence wm (3,ny,nx) of optimize_obs() for an observed magnetogram bobs (3,ny,nx), the usual choice for
    HMI data: 1 for the vertical component, and for both transverse components max(|B_t| / max |B_t|, floor) with
    |B_t| = sqrt(Bx^2 + By^2) - the transverse field is known far worse than the vertical one, and weak-field pixels
    hardly at all.  An all-zero transverse field gives `floor`.  0 <= floor <= 1.  Plain numpy."""
    a = np.asarray(bobs, dtype=np.float64)
    if a.ndim != 3 or a.shape[0] != 3:
        raise ValueError(f"bobs must have the shape (3, ny, nx), not {a.shape}")
    if not (0.0 <= floor <= 1.0):
        raise ValueError(f"floor must lie in [0, 1], not {floor!r}")
    bt = np.sqrt(a[0] * a[0] + a[1] * a[1])
    top = bt.max() if bt.size else 0.0
    t = np.maximum(bt / top, floor) if top > 0.0 else np.full(bt.shape, float(floor))
    return np.array([t, t, np.ones(bt.shape)])


def force_free_optimize_obs(x, y, z, b, bobs=None, wm=None, nu=0.01, free=True, w=None, start="potential",
                            niter_max=10000, check=50, tol=1e-4, dt0=None, dt_min=None, hist_rows=None,
                            niterex_max=10000, ncycles_max=1024, ex_tol=1e-13, vc_tol=1e-10, ms=5, mean=False,
                            mixed_precision=False, flxcrl=False, ngrids=0, lib=None):
    """Nonlinear force-free field whose lower face is fitted to the measured magnetogram bobs within its errors wm:
    one-shot form of VecPot.optimize_obs (returns its (ierr, B, hist, info)).  Raises NdsmHipError on device / runtime
    failures (>= 9001)."""
    V = _grid_handle(x, y, z, b, ngrids, lib)
    try:
        return V.optimize_obs(b, bobs=bobs, wm=wm, nu=nu, free=free, w=w, start=start, niter_max=niter_max,
                              check=check, tol=tol, dt0=dt0, dt_min=dt_min, hist_rows=hist_rows,
                              niterex_max=niterex_max, ncycles_max=ncycles_max, ex_tol=ex_tol, vc_tol=vc_tol, ms=ms,
                              mean=mean, mixed_precision=mixed_precision, flxcrl=flxcrl)
    finally:
        V.close()


RESAMPLE_MODES = {"linear": 0, "average": 1}


def resample(a, shape, mode="linear", device=False, lib=None):
    """A node array on a uniform mesh resampled to another uniform mesh on the same box, on the device (semantics:
    include/ndsm_hip.h, ndsm_hip_resample).  a: (ncomp, nz, ny, nx) or (nz, ny, nx); shape: the destination
    (nz, ny, nx).  mode "linear": linear interpolation, any two shapes; "average": the hat average (full weighting for
    a 2:1 pair), which cannot refine.  An axis of one node on both sides is copied.  A face, edge or corner of the
    result depends on the same face, edge or corner of a only.  device=True: the arrays are staged in device memory
    and the device-resident entry point runs."""
    if mode not in RESAMPLE_MODES:
        raise ValueError(f"mode must be 'linear' or 'average', not {mode!r}")
    src = np.asarray(a)
    if src.ndim not in (3, 4) or src.size == 0:
        raise NdsmHipError(f"resample: an array of shape {src.shape}, (ncomp, nz, ny, nx) or (nz, ny, nx) is needed "
                           "(code 9002)")
    dshape = tuple(int(v) for v in shape)
    if len(dshape) != 3 or any(int(v) != v for v in shape):
        raise ValueError(f"shape must be three whole numbers (nz, ny, nx), not {shape!r}")
    ncomp = 1 if src.ndim == 3 else src.shape[0]
    sshape = src.shape[-3:]
    for ns, nd in zip(sshape, dshape):
        if not ((ns == 1 and nd == 1) or (ns >= 2 and nd >= 2)):
            raise ValueError(f"an axis needs at least 2 nodes on both sides, or 1 on both: {sshape} -> {dshape}")
        if mode == "average" and nd > ns:
            raise ValueError(f"the hat average cannot refine: {sshape} -> {dshape}")
    L = lib or load_library()
    S = _f64(src).reshape(-1).copy()
    D = np.zeros(ncomp * int(np.prod(dshape)))
    ns3, nd3 = np.array(sshape[::-1], dtype=np.intc), np.array(dshape[::-1], dtype=np.intc)
    args = (ns3.ctypes.data_as(_ip), nd3.ctypes.data_as(_ip), ncomp, RESAMPLE_MODES[mode])
    if not device:
        _check(L.ndsm_hip_resample(*args, S.ctypes.data, D.ctypes.data), "ndsm_hip_resample", L)
    else:
        ptrs = []
        try:
            for h in (S, D):
                p = ctypes.c_void_p()
                _check(L.ndsm_hip_device_alloc(h.nbytes, ctypes.byref(p)), "device_alloc", L)
                ptrs.append(p)
            _check(L.ndsm_hip_memcpy_h2d(ptrs[0], S.ctypes.data, S.nbytes), "h2d", L)
            _check(L.ndsm_hip_resample_device(*args, ptrs[0], ptrs[1]), "ndsm_hip_resample_device", L)
            _check(L.ndsm_hip_memcpy_d2h(D.ctypes.data, ptrs[1], D.nbytes), "d2h", L)
        finally:
            for p in ptrs:
                L.ndsm_hip_device_free(p)
    return D.reshape(src.shape[:-3] + dshape)


def resample_weighted(a, wa, shape, device=False, lib=None):
    """The confidence-weighted restriction of an observation a with its confidence wa (the same shape) to a coarser
    uniform mesh on the same box, on the device (semantics: include/ndsm_hip.h, ndsm_hip_resample_weighted): every
    destination node takes sum q wa a / sum q wa over the taps of the hat average - a trusted pixel among untrusted
    ones gives its own value, not the mean -, its confidence the hat average of wa; where no tap is trusted, the plain
    hat average.  a: (ncomp, nz, ny, nx) or (nz, ny, nx), planes with nz = 1; shape: the destination (nz, ny, nx), no
    axis finer than a's.  The values must be finite.  Returns (a', wa').  device=True: the arrays are staged in device
    memory and the device-resident entry point runs."""
    src, wsrc = np.asarray(a), np.asarray(wa)
    if src.ndim not in (3, 4) or src.size == 0:
        raise NdsmHipError(f"resample_weighted: an array of shape {src.shape}, (ncomp, nz, ny, nx) or (nz, ny, nx) is "
                           "needed (code 9002)")
    if wsrc.shape != src.shape:
        raise NdsmHipError(f"resample_weighted: a confidence of shape {wsrc.shape} for an array of shape {src.shape} "
                           "(code 9002)")
    dshape = tuple(int(v) for v in shape)
    if len(dshape) != 3 or any(int(v) != v for v in shape):
        raise ValueError(f"shape must be three whole numbers (nz, ny, nx), not {shape!r}")
    ncomp = 1 if src.ndim == 3 else src.shape[0]
    sshape = src.shape[-3:]
    for ns, nd in zip(sshape, dshape):
        if not ((ns == 1 and nd == 1) or (ns >= 2 and nd >= 2)):
            raise ValueError(f"an axis needs at least 2 nodes on both sides, or 1 on both: {sshape} -> {dshape}")
        if nd > ns:
            raise ValueError(f"the weighted restriction cannot refine: {sshape} -> {dshape}")
    L = lib or load_library()
    S, WS = _f64(src).reshape(-1).copy(), _f64(wsrc).reshape(-1).copy()
    D, WD = np.zeros(ncomp * int(np.prod(dshape))), np.zeros(ncomp * int(np.prod(dshape)))
    ns3, nd3 = np.array(sshape[::-1], dtype=np.intc), np.array(dshape[::-1], dtype=np.intc)
    args = (ns3.ctypes.data_as(_ip), nd3.ctypes.data_as(_ip), ncomp)
    if not device:
        _check(L.ndsm_hip_resample_weighted(*args, S.ctypes.data, WS.ctypes.data, D.ctypes.data, WD.ctypes.data),
               "ndsm_hip_resample_weighted", L)
    else:
        ptrs = []
        try:
            for h in (S, WS, D, WD):
                p = ctypes.c_void_p()
                _check(L.ndsm_hip_device_alloc(h.nbytes, ctypes.byref(p)), "device_alloc", L)
                ptrs.append(p)
            _check(L.ndsm_hip_memcpy_h2d(ptrs[0], S.ctypes.data, S.nbytes), "h2d", L)
            _check(L.ndsm_hip_memcpy_h2d(ptrs[1], WS.ctypes.data, WS.nbytes), "h2d", L)
            _check(L.ndsm_hip_resample_weighted_device(*args, *ptrs), "ndsm_hip_resample_weighted_device", L)
            _check(L.ndsm_hip_memcpy_d2h(D.ctypes.data, ptrs[2], D.nbytes), "d2h", L)
            _check(L.ndsm_hip_memcpy_d2h(WD.ctypes.data, ptrs[3], WD.nbytes), "d2h", L)
        finally:
            for p in ptrs:
                L.ndsm_hip_device_free(p)
    return D.reshape(src.shape[:-3] + dshape), WD.reshape(src.shape[:-3] + dshape)


GREEN_WHICH = {"faces": 0, "volume": 1}


def _green_source(x, y, z, bz, xs, ys, zs):
    """the source of a Green's-function call as (nsrc, xs, ys, zs, bz flat): the magnetogram bz (nsy,nsx) on the mesh
    xs, ys at height zs; the defaults are the box's x, y and z[0].  ValueError for what the library would answer with
    9004 and for a bz that does not fit its mesh"""
    qx = _f64(x if xs is None else xs).reshape(-1)
    qy = _f64(y if ys is None else ys).reshape(-1)
    if zs is None:
        if z is None or len(z) == 0:
            raise ValueError("zs is needed")
        zs = z[0]
    zs = float(zs)
    if len(qx) < 2 or len(qy) < 2:
        raise ValueError(f"the source mesh needs at least 2 nodes per axis, not {len(qx)} x {len(qy)}")
    if not (qx[1] - qx[0] > 0.0 and qy[1] - qy[0] > 0.0):
        raise ValueError("the source mesh needs spacings > 0")
    S = np.asarray(bz)
    if S.shape != (len(qy), len(qx)):
        raise ValueError(f"bz of shape {S.shape}, the source mesh needs {(len(qy), len(qx))}")
    if z is not None and len(z) > 0 and not (z[0] >= zs):
        raise ValueError(f"the box starts below the magnetogram: z[0] = {z[0]!r} < zs = {zs!r}")
    return np.array([len(qx), len(qy)], dtype=np.intc), qx, qy, zs, _f64(S).reshape(-1).copy()


def _staged(L, host_arrays, call):
    """stage host_arrays in device memory, run call(*device pointers), copy every array back"""
    ptrs = []
    try:
        for a in host_arrays:
            p = ctypes.c_void_p()
            _check(L.ndsm_hip_device_alloc(a.nbytes, ctypes.byref(p)), "device_alloc", L)
            ptrs.append(p)
            _check(L.ndsm_hip_memcpy_h2d(p, a.ctypes.data, a.nbytes), "h2d", L)
        rc = call(*ptrs)
        for a, p in zip(host_arrays, ptrs):
            _check(L.ndsm_hip_memcpy_d2h(a.ctypes.data, p, a.nbytes), "d2h", L)
    finally:
        for p in ptrs:
            L.ndsm_hip_device_free(p)
    return rc


def _lfff_alpha(alpha):
    """alpha as a finite float; ValueError for what the library would answer with 9004"""
    try:
        a = np.asarray(alpha, dtype=np.float64)
    except (TypeError, ValueError):
        a = np.zeros(2)
    if a.ndim != 0 or not np.isfinite(a):
        raise ValueError(f"alpha must be one finite number, not {alpha!r}")
    return float(a)


def _field_points(kind, xs, ys, zs, bz, alpha, pts, device, lib):
    """green_field_points (kind "green", alpha unused) and lfff_field_points (kind "lfff"): B (npts,3) from
    ndsm_hip_<kind>_points or, for device=True, its _device form on staged arrays"""
    P = np.asarray(pts, dtype=np.float64)
    if P.ndim != 2 or P.shape[1] != 3:
        raise ValueError(f"pts of shape {P.shape}, (npts, 3) is needed")
    mid = (_lfff_alpha(alpha),) if kind == "lfff" else ()
    ns2, qx, qy, zs, S = _green_source(None, None, None, bz, xs, ys, zs)
    L = lib or load_library()
    P = np.ascontiguousarray(P).reshape(-1).copy()
    B = np.zeros(P.size)
    head = (ns2.ctypes.data_as(_ip), _d(qx), _d(qy), zs)
    name = f"ndsm_hip_{kind}_points" + ("_device" if device else "")
    fn = getattr(L, name)
    if not device:
        _check(fn(*head, S.ctypes.data, *mid, len(P) // 3, P.ctypes.data, B.ctypes.data), name, L)
    else:
        _check(_staged(L, [S, P, B], lambda dS, dP, dB: fn(*head, dS, *mid, len(P) // 3, dP, dB)), name, L)
    return B.reshape(-1, 3)


def _field_box(kind, x, y, z, bz, alpha, xs, ys, zs, which, device, lib):
    """magnetogram_field (kind "green", alpha unused) and linear_force_free_field (kind "lfff"): b (3,nz,ny,nx) from
    ndsm_hip_<kind>_box or, for device=True, its _device form on staged arrays"""
    if which not in GREEN_WHICH:
        raise ValueError(f"which must be 'faces' or 'volume', not {which!r}")
    mid = (_lfff_alpha(alpha),) if kind == "lfff" else ()
    qx, qy, qz = (_f64(v).reshape(-1) for v in (x, y, z))
    if min(len(qx), len(qy), len(qz)) < 2:
        raise ValueError(f"the box needs at least 2 nodes per axis, not {(len(qz), len(qy), len(qx))}")
    ns2, sx, sy, zs, S = _green_source(qx, qy, qz, bz, xs, ys, zs)
    L = lib or load_library()
    n3 = np.array([len(qx), len(qy), len(qz)], dtype=np.intc)
    B = np.zeros(3 * len(qx) * len(qy) * len(qz))
    head = (ns2.ctypes.data_as(_ip), _d(sx), _d(sy), zs)
    tail = (n3.ctypes.data_as(_ip), _d(qx), _d(qy), _d(qz), GREEN_WHICH[which])
    name = f"ndsm_hip_{kind}_box" + ("_device" if device else "")
    fn = getattr(L, name)
    if not device:
        _check(fn(*head, S.ctypes.data, *mid, *tail, B.ctypes.data), name, L)
    else:
        _check(_staged(L, [S, B], lambda dS, dB: fn(*head, dS, *mid, *tail, dB)), name, L)
    return B.reshape(3, len(qz), len(qy), len(qx))


def green_field_points(xs, ys, zs, bz, pts, device=False, lib=None):
    """The Green's-function field of the half space above the magnetogram bz (nsy,nsx) - given on the uniform mesh
    xs, ys at height zs - at the points pts (npts,3; x, y, z), on the device (semantics: include/ndsm_hip.h,
    ndsm_hip_green_points).  Returns B (npts,3).  Below the plane the field is NaN; on it Bz is the bilinear
    interpolation of bz (0 outside the mesh).  device=True: the arrays are staged in device memory and the
    device-resident entry point runs."""
    return _field_points("green", xs, ys, zs, bz, None, pts, device, lib)


def magnetogram_field(x, y, z, bz, xs=None, ys=None, zs=None, which="faces", device=False, lib=None):
    """The Green's-function field of the half space above the magnetogram bz (nsy,nsx) on the box mesh x, y, z, as the
    b (3,nz,ny,nx) every entry that starts from a potential field takes (semantics: include/ndsm_hip.h,
    ndsm_hip_green_box).  xs, ys, zs: the magnetogram's mesh and height, by default x, y and z[0] - it may be wider
    than the box, and the flux outside the box's footprint then shapes the side faces.  which "faces": the nodes of
    the six faces, zeros inside (all that solve(), force_free_field(), optimize(start="potential") and the cascades
    read); "volume": every node.  Where the box starts on the magnetogram's plane, take x and y as slices of xs and
    ys (xs[i0:i0 + nx]): a box node on the plane must be a source node bit for bit - the rule leaves that pixel out -
    or lie well away from every source node; a miss by a rounding error gives a term of the order 1 / eps^2.
    device=True: the arrays are staged in device memory and the device-resident entry point runs."""
    return _field_box("green", x, y, z, bz, None, xs, ys, zs, which, device, lib)


def lfff_field_points(xs, ys, zs, bz, alpha, pts, device=False, lib=None):
    """The constant-alpha force-free field (curl B = alpha B, Chiu & Hilton's half-space solution) above the
    magnetogram bz (nsy,nsx) - given on the uniform mesh xs, ys at height zs - at the points pts (npts,3; x, y, z), on
    the device (semantics: include/ndsm_hip.h, ndsm_hip_lfff_points).  alpha: one finite number of either sign, in
    1 / (length unit of the mesh), e.g. best_alpha()'s.  Returns B (npts,3); the plane rules are green_field_points',
    and alpha = 0 gives its bits.  device=True: the arrays are staged in device memory and the device-resident entry
    point runs."""
    return _field_points("lfff", xs, ys, zs, bz, alpha, pts, device, lib)


def linear_force_free_field(x, y, z, bz, alpha, xs=None, ys=None, zs=None, which="volume", device=False, lib=None):
    """The constant-alpha force-free field above the magnetogram bz (nsy,nsx) on the box mesh x, y, z, as the
    b (3,nz,ny,nx) that helicity(), trace(), squashing(), nulls() and optimize(start="given") take (semantics:
    include/ndsm_hip.h, ndsm_hip_lfff_box).  alpha, xs, ys, zs, device: as lfff_field_points and magnetogram_field;
    which "volume": every node; "faces": the nodes of the six faces, zeros inside.  Take x and y as slices of xs and
    ys: a box node must lie on the vertical through a source node bit for bit, or well away from it, at every
    height - a miss by a rounding error costs digits of the order eps z^2 / R^2.  The field depends on the
    magnetogram's width more than the potential field does (its horizontal part falls like 1 / R)."""
    return _field_box("lfff", x, y, z, bz, alpha, xs, ys, zs, which, device, lib)


def best_alpha(x, y, b, bz_min=0.0):
    """The least-squares alpha of a vector magnetogram: sum Jz Bz / sum Bz^2 over the pixels of the lower face k = 0
    of b (3,nz,ny,nx) with |Bz| >= bz_min, Jz = d_x B_y - d_y B_x formed with the differences of boundary_alpha().
    Plain numpy: the number lfff_field_points() and linear_force_free_field() take.  ValueError when no pixel
    qualifies or the sum of Bz^2 is 0."""
    b = np.asarray(b, dtype=np.float64)
    bx, by, bz = b[0, 0], b[1, 0], b[2, 0]
    jz = np.gradient(by, _f64(x), axis=1, edge_order=2) - np.gradient(bx, _f64(y), axis=0, edge_order=2)
    use = np.abs(bz) >= bz_min
    den = float(np.sum(bz[use] * bz[use]))
    if not den > 0.0:
        raise ValueError("no pixel with |Bz| >= bz_min and Bz != 0: alpha is undefined")
    return float(np.sum(jz[use] * bz[use])) / den


Flow = collections.namedtuple("Flow", ["v", "coef", "status"])
Fluxes = collections.namedtuple("Fluxes", ["dens", "helicity", "energy", "flux"])


def _plane_mesh(xs, ys, nmin):
    """the uniform mesh of a magnetogram as (nsrc, xs, ys); ValueError for what the library would answer with 9004"""
    qx, qy = _f64(xs).reshape(-1), _f64(ys).reshape(-1)
    if len(qx) < nmin or len(qy) < nmin:
        raise ValueError(f"the mesh needs at least {nmin} nodes per axis, not {len(qx)} x {len(qy)}")
    if not (qx[1] - qx[0] > 0.0 and qy[1] - qy[0] > 0.0):
        raise ValueError("the mesh needs spacings > 0")
    return np.array([len(qx), len(qy)], dtype=np.intc), qx, qy


def _plane_field(a, ncomp, qx, qy, name):
    """a (ncomp,nsy,nsx) as a flat float64 copy; ValueError for another shape"""
    A = np.asarray(a)
    want = (ncomp, len(qy), len(qx)) if ncomp else (len(qy), len(qx))
    if A.shape != want:
        raise ValueError(f"{name} of shape {A.shape}, the mesh needs {want}")
    return _f64(A).reshape(-1).copy()


def flow_fit(xs, ys, b0, b1, dt, r=5, rcond=1e-10, device=False, lib=None):
    """The plasma velocity on the plane of two vector magnetograms b0, b1 (3,nsy,nsx) taken dt apart on the uniform mesh
    xs, ys: a local affine fit of the normal component of the induction equation over top-hat windows of (2r+1)^2
    pixels, in the manner of DAVE4VM (Schuck 2008), on the device (semantics: include/ndsm_hip.h, ndsm_hip_flow_fit).
    Returns Flow(v (3,nsy,nsx), coef (9,nsy,nsx) = u0, ux, uy, v0, vx, vy, w0, wx, wy, status (nsy,nsx)): status 0
    solved; 1 rank-deficient (the aperture problem; a scaled pivot not above rcond), v and coef 0; 2 a value that is not
    finite in the window, v and coef NaN.  device=True: the arrays are staged in device memory and the device-resident
    entry point runs."""
    ns2, qx, qy = _plane_mesh(xs, ys, 3)
    dt, rcond = float(dt), float(rcond)
    if not np.isfinite(dt) or dt == 0.0:
        raise ValueError(f"dt must be finite and not 0, not {dt!r}")
    if int(r) != r or not 1 <= r <= 16:
        raise ValueError(f"r must be a whole number in 1..16, not {r!r}")
    if not 0.0 <= rcond < 1.0:
        raise ValueError(f"rcond must be in [0, 1), not {rcond!r}")
    B0, B1 = _plane_field(b0, 3, qx, qy, "b0"), _plane_field(b1, 3, qx, qy, "b1")
    L = lib or load_library()
    npix = len(qx) * len(qy)
    V, C, S = np.zeros(3 * npix), np.zeros(9 * npix), np.zeros(npix, dtype=np.int32)
    head = (ns2.ctypes.data_as(_ip), _d(qx), _d(qy))
    if not device:
        _check(L.ndsm_hip_flow_fit(*head, B0.ctypes.data, B1.ctypes.data, dt, int(r), rcond, V.ctypes.data, C.ctypes.data,
                                   S.ctypes.data), "ndsm_hip_flow_fit", L)
    else:
        _check(_staged(L, [B0, B1, V, C, S], lambda d0, d1, dV, dC, dS: L.ndsm_hip_flow_fit_device(
            *head, d0, d1, dt, int(r), rcond, dV, dC, dS)), "ndsm_hip_flow_fit_device", L)
    shape = (len(qy), len(qx))
    return Flow(V.reshape((3,) + shape), C.reshape((9,) + shape), S.reshape(shape))


def plane_vector_potential(xs, ys, bz, device=False, lib=None):
    """The potential field's vector potential on the plane of the magnetogram bz (nsy,nsx) itself - A_p.n = 0,
    div_h A_p = 0, z.curl A_p = bz - on the magnetogram's own nodes, on the device (semantics: include/ndsm_hip.h,
    ndsm_hip_green_ap_plane).  Returns ap (2,nsy,nsx).  device=True: the arrays are staged in device memory and the
    device-resident entry point runs."""
    ns2, qx, qy = _plane_mesh(xs, ys, 2)
    S = _plane_field(bz, 0, qx, qy, "bz")
    L = lib or load_library()
    A = np.zeros(2 * S.size)
    head = (ns2.ctypes.data_as(_ip), _d(qx), _d(qy))
    if not device:
        _check(L.ndsm_hip_green_ap_plane(*head, S.ctypes.data, A.ctypes.data), "ndsm_hip_green_ap_plane", L)
    else:
        _check(_staged(L, [S, A], lambda dS, dA: L.ndsm_hip_green_ap_plane_device(*head, dS, dA)),
               "ndsm_hip_green_ap_plane_device", L)
    return A.reshape(2, len(qy), len(qx))


def plane_vector_potential_points(xs, ys, bz, pts, device=False, lib=None):
    """The same vector potential at the points pts (npts,2; x, y) of the plane (semantics: include/ndsm_hip.h,
    ndsm_hip_green_ap_points).  Returns ap (npts,2).  A point that is a node of the mesh bit for bit gets the bits of
    plane_vector_potential() there."""
    P = np.asarray(pts, dtype=np.float64)
    if P.ndim != 2 or P.shape[1] != 2:
        raise ValueError(f"pts of shape {P.shape}, (npts, 2) is needed")
    ns2, qx, qy = _plane_mesh(xs, ys, 2)
    S = _plane_field(bz, 0, qx, qy, "bz")
    L = lib or load_library()
    P = np.ascontiguousarray(P).reshape(-1).copy()
    A = np.zeros(P.size)
    head = (ns2.ctypes.data_as(_ip), _d(qx), _d(qy))
    if not device:
        _check(L.ndsm_hip_green_ap_points(*head, S.ctypes.data, len(P) // 2, P.ctypes.data, A.ctypes.data),
               "ndsm_hip_green_ap_points", L)
    else:
        _check(_staged(L, [S, P, A], lambda dS, dP, dA: L.ndsm_hip_green_ap_points_device(*head, dS, len(P) // 2, dP, dA)),
               "ndsm_hip_green_ap_points_device", L)
    return A.reshape(-1, 2)


def boundary_fluxes(xs, ys, b, v, ap=None, status=None, device=False, lib=None):
    """The fluxes of relative helicity and of magnetic energy through the plane of the magnetogram b (3,nsy,nsx) under
    the flow v (3,nsy,nsx) (Berger & Field 1984; semantics: include/ndsm_hip.h, ndsm_hip_flow_flux).  ap (2,nsy,nsx):
    the potential field's vector potential on the plane; None computes it from b[2] on the device
    (ndsm_hip_green_ap_plane_device), and it goes into the fluxes without crossing PCIe in between.  status
    (nsy,nsx), e.g. flow_fit()'s: v is taken as 0 where it is not 0.  Returns Fluxes(dens (4,nsy,nsx) = h_em, h_sh,
    s_em, s_sh per pixel; helicity = (emergence, shear, total); energy = (emergence, shear, total) - no 4 pi, as
    relative_helicity()'s energies -; flux = (unsigned, signed) magnetic flux).  device=True: ap too is staged and the
    device-resident entry point runs."""
    ns2, qx, qy = _plane_mesh(xs, ys, 2)
    B, V = _plane_field(b, 3, qx, qy, "b"), _plane_field(v, 3, qx, qy, "v")
    A = None if ap is None else _plane_field(ap, 2, qx, qy, "ap")
    npix = len(qx) * len(qy)
    if status is not None:
        st = np.asarray(status)
        if st.shape != (len(qy), len(qx)):
            raise ValueError(f"status of shape {st.shape}, the mesh needs {(len(qy), len(qx))}")
        V.reshape(3, npix)[:, st.reshape(-1) != 0] = 0.0
    L = lib or load_library()
    D, out = np.zeros(4 * npix), np.zeros(8)
    head = (ns2.ctypes.data_as(_ip), _d(qx), _d(qy))
    if A is not None and not device:
        _check(L.ndsm_hip_flow_flux(*head, B.ctypes.data, V.ctypes.data, A.ctypes.data, D.ctypes.data, _d(out)),
               "ndsm_hip_flow_flux", L)
    elif A is not None:
        _check(_staged(L, [B, V, A, D], lambda dB, dV, dA, dD: L.ndsm_hip_flow_flux_device(*head, dB, dV, dA, dD, _d(out))),
               "ndsm_hip_flow_flux_device", L)
    else:
        A = np.zeros(2 * npix)

        def both(dB, dV, dA, dD):
            rc = L.ndsm_hip_green_ap_plane_device(*head, ctypes.c_void_p(dB.value + 16 * npix), dA)
            return rc if rc != 0 else L.ndsm_hip_flow_flux_device(*head, dB, dV, dA, dD, _d(out))
        _check(_staged(L, [B, V, A, D], both), "ndsm_hip_green_ap_plane_device + ndsm_hip_flow_flux_device", L)
    return Fluxes(D.reshape(4, len(qy), len(qx)), tuple(float(x) for x in out[0:3]), tuple(float(x) for x in out[3:6]),
                  (float(out[6]), float(out[7])))


Patches = collections.namedtuple("Patches", ["label", "root", "sign", "npix", "flux", "sx", "sy", "centroid", "nin", "K"])
Connectivity = collections.namedtuple("Connectivity", ["dest", "ends", "length", "status", "pa", "pc", "nlines", "pflux",
                                                       "ntraced", "npairs", "label", "K"])
CONNECT_NONE = -9                  # dest of a pixel from which no line is traced
PATCHES_MAX = 2 ** 31 - 1          # no more patches than pixels, and those fit a C int


def _capacity_arg(name, v):
    """a capacity (None, or a whole number in 0 .. PATCHES_MAX) as None or int; ValueError otherwise"""
    if v is None:
        return None
    if (isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v) or
            int(v) != v or not 0 <= v <= PATCHES_MAX):
        raise ValueError(f"{name} must be None or an integer in 0 .. {PATCHES_MAX}, not {v!r}")
    return int(v)


def _thr_arg(thr):
    """thr as a finite float >= 0; ValueError for what the library would answer with 9004"""
    try:
        t = float(thr)
    except (TypeError, ValueError):
        raise ValueError(f"thr must be a finite number >= 0, not {thr!r}") from None
    if not (np.isfinite(t) and t >= 0.0):
        raise ValueError(f"thr must be a finite number >= 0, not {thr!r}")
    return t


def partition_magnetogram(xs, ys, bz, thr=0.0, max_patches=None, device=False, lib=None):
    """The flux patches of the magnetogram bz (nsy,nsx) on the uniform mesh xs, ys, on the device (semantics:
    include/ndsm_hip.h, ndsm_hip_partition): a pixel is in where |bz| > thr; every pixel in points to the strongest
    pixel of its sign among itself and its 8 neighbours (equal values: the smallest index), and the pixels that reach
    the same peak form a patch.  Patches are numbered 1 .. K in ascending peak index.  max_patches: the capacity of the
    first call; when more are found the call is repeated once with that number (None: a counting call, then one call
    of the exact size; 0: count only, no table).  Returns Patches(label (nsy,nsx; int32, 0: not in), root (n; int64,
    the peak's pixel i + nsx j), sign (n; +1 / -1), npix (n), flux, sx, sy (n; the trapezoid sums of bz, bz x and bz y
    over the patch, with the same bits on every run), centroid (n,2) = (sx / flux, sy / flux), nin (the pixels in),
    K (the patches, exact whatever the capacity)).  device=True: the arrays are staged in device memory and the
    device-resident entry point runs."""
    ns2, qx, qy = _plane_mesh(xs, ys, 2)
    thr, max_patches = _thr_arg(thr), _capacity_arg("max_patches", max_patches)
    S = _plane_field(bz, 0, qx, qy, "bz")
    L = lib or load_library()
    head = (ns2.ctypes.data_as(_ip), _d(qx), _d(qy))

    def run(cap):
        counts = np.zeros(2, dtype=np.int64)
        m = max(cap, 1)
        label = np.zeros(S.size, dtype=np.int32)
        rec = [np.zeros(m, dtype=np.int64), np.zeros(m, dtype=np.int32), np.zeros(m, dtype=np.int64), np.zeros(m),
               np.zeros(m), np.zeros(m)]
        if not device:
            _check(L.ndsm_hip_partition(*head, S.ctypes.data, thr, cap, counts.ctypes.data, label.ctypes.data,
                                        *[a.ctypes.data for a in rec]), "ndsm_hip_partition", L)
        else:
            _check(_staged(L, [S, label, *rec], lambda dS, dl, *dr: L.ndsm_hip_partition_device(
                *head, dS, thr, cap, counts.ctypes.data, dl, *dr)), "ndsm_hip_partition_device", L)
        return int(counts[1]), (counts, label, rec)
    if max_patches is None:
        n, (counts, label, rec) = _with_capacity(run, 0)
    else:
        n, (counts, label, rec) = _with_capacity(run, max_patches, count_only=True)
    root, sign, npix, flux, sx, sy = [a[:n] for a in rec]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        centroid = np.stack([sx / flux, sy / flux], axis=1)
    return Patches(label.reshape(len(qy), len(qx)), root, sign, npix, flux, sx, sy, centroid, int(counts[0]),
                   int(counts[1]))


def _connect_tuple(counts, out, pairs, n, label, K, ny, nx):
    dest, ends, length, status = out
    return Connectivity(dest.reshape(ny, nx), ends.reshape(ny, nx, 3), length.reshape(ny, nx), status.reshape(ny, nx),
                        *[a[:n] for a in pairs], int(counts[0]), int(counts[1]), label.reshape(ny, nx), int(K))


def connectivity_matrix(conn, K=None, symmetric=False):
    """The connectivity fluxes of a Connectivity tuple as a dense (K, K + 1) array: entry (a - 1, c - 1) is the flux
    Psi(a -> c) at the feet in patch a of the lines that end in patch c, and the last column holds everything of
    patch a that did not land on a patch (an open class, or an unlabelled pixel).  K None: conn.K.  The matrix is
    one-sided, Psi(a -> b) counted from a's feet and Psi(b -> a) from b's; symmetric=True replaces both by their mean
    (the last column stays)."""
    K = conn.K if K is None else K
    if isinstance(K, bool) or int(K) != K or K < 0:
        raise ValueError(f"K must be an integer >= 0, not {K!r}")
    K = int(K)
    M = np.zeros((K, K + 1))
    for a, c, f in zip(conn.pa, conn.pc, conn.pflux):
        if 1 <= a <= K:
            M[a - 1, c - 1 if 1 <= c <= K else K] += f
    if symmetric:
        M[:, :K] = 0.5 * (M[:, :K] + M[:, :K].T)
    return M


def find_connectivity(x, y, z, b, label=None, K=None, thr=0.0, step=0.5, max_steps=None, max_pairs=None, lib=None):
    """The patch connectivity of b (3,nz,ny,nx): one-shot form of VecPot.connectivity (returns its Connectivity tuple).
    Raises NdsmHipError on device / runtime failures (>= 9001)."""
    _thr_arg(thr)
    _capacity_arg("max_pairs", max_pairs)
    V = _grid_handle(x, y, z, b, 0, lib)
    try:
        return V.connectivity(b, label=label, K=K, thr=thr, step=step, max_steps=max_steps, max_pairs=max_pairs)
    finally:
        V.close()


def potential_open(x, y, z, bz, xs=None, ys=None, zs=None, a_init=None, niterex_max=10000, ncycles_max=1024,
                   ex_tol=1e-13, vc_tol=1e-10, ms=5, mean=False, mixed_precision=False, flxcrl=False, ngrids=0,
                   lib=None):
    """The open-box potential field of the magnetogram bz (nsy,nsx): one-shot form of VecPot.solve_open (returns its
    (ierr, A, B)).  Raises NdsmHipError on device / runtime failures (>= 9001)."""
    _green_source(x, y, z, bz, xs, ys, zs)           # (a ValueError comes before the handle is made)
    V = VecPot(x, y, z, ngrids=ngrids, lib=lib)
    try:
        return V.solve_open(bz, xs=xs, ys=ys, zs=zs, a_init=a_init, niterex_max=niterex_max, ncycles_max=ncycles_max,
                            ex_tol=ex_tol, vc_tol=vc_tol, ms=ms, mean=mean, mixed_precision=mixed_precision,
                            flxcrl=flxcrl)
    finally:
        V.close()


def cascade_shapes(shape, levels, min_nodes=4):
    """The shapes (nz, ny, nx) of a cascade of that many levels, finest first: each axis follows n -> (n + 1) // 2
    (33 -> 17, 32 -> 16, 9 -> 5); an axis that would fall below min_nodes stays where it is.  ValueError when a
    level is asked for and no axis can shrink."""
    if int(levels) != levels or levels < 1:
        raise ValueError(f"levels must be a whole number >= 1, not {levels!r}")
    out = [tuple(int(n) for n in shape)]
    for _ in range(int(levels) - 1):
        nxt = tuple((n + 1) // 2 if (n + 1) // 2 >= min_nodes else n for n in out[-1])
        if nxt == out[-1]:
            raise ValueError(f"no axis of {out[-1]} can shrink further (min_nodes {min_nodes}): "
                             f"{len(out)} levels at the most")
        out.append(nxt)
    return out


def force_free_cascade(x, y, z, b, levels=3, shapes=None, w=None, start="potential", niter_max=10000, check=50,
                       tol=1e-4, dt0=None, dt_min=None, hist_rows=None, niterex_max=10000, ncycles_max=1024,
                       ex_tol=1e-13, vc_tol=1e-10, ms=5, mean=False, mixed_precision=False, flxcrl=False, lib=None):
    """Nonlinear force-free field from a vector magnetogram by the optimization method run as a coarse-to-fine
    cascade: one-shot form of VecPot.optimize_cascade (returns its (ierr, B, hist, info)).  shapes: the (nz, ny, nx)
    of every level, finest first (None: cascade_shapes() of b's grid for `levels`); every level's mesh is
    linspace(first, last, n) per axis, which keeps the end coordinates exact.  Raises NdsmHipError on device /
    argument errors."""
    handles = []
    try:
        _cascade_handles(handles, x, y, z, levels, shapes, lib)
        return handles[0].optimize_cascade(handles[1:], b, w=w, start=start, niter_max=niter_max, check=check, tol=tol,
                                           dt0=dt0, dt_min=dt_min, hist_rows=hist_rows, niterex_max=niterex_max,
                                           ncycles_max=ncycles_max, ex_tol=ex_tol, vc_tol=vc_tol, ms=ms, mean=mean,
                                           mixed_precision=mixed_precision, flxcrl=flxcrl)
    finally:
        for V in handles:
            V.close()


def force_free_obs_cascade(x, y, z, b, levels=3, shapes=None, bobs=None, wm=None, nu=0.01, free=True, w=None,
                           start="potential", niter_max=10000, check=50, tol=1e-4, dt0=None, dt_min=None,
                           hist_rows=None, niterex_max=10000, ncycles_max=1024, ex_tol=1e-13, vc_tol=1e-10, ms=5,
                           mean=False, mixed_precision=False, flxcrl=False, lib=None):
    """Nonlinear force-free field whose lower face is fitted to the measured magnetogram bobs within its errors wm, run
    as a coarse-to-fine cascade: one-shot form of VecPot.optimize_obs_cascade (returns its (ierr, B, hist, info)).
    levels, shapes and the meshes as force_free_cascade.  Raises NdsmHipError on device / argument errors."""
    handles = []
    try:
        _cascade_handles(handles, x, y, z, levels, shapes, lib)
        return handles[0].optimize_obs_cascade(handles[1:], b, bobs=bobs, wm=wm, nu=nu, free=free, w=w, start=start,
                                               niter_max=niter_max, check=check, tol=tol, dt0=dt0, dt_min=dt_min,
                                               hist_rows=hist_rows, niterex_max=niterex_max, ncycles_max=ncycles_max,
                                               ex_tol=ex_tol, vc_tol=vc_tol, ms=ms, mean=mean,
                                               mixed_precision=mixed_precision, flxcrl=flxcrl)
    finally:
        for V in handles:
            V.close()


def _cascade_handles(handles, x, y, z, levels, shapes, lib):
    """appends the handles of a one-shot cascade's levels, finest first, to `handles` (the caller closes them)"""
    x, y, z = _f64(x), _f64(y), _f64(z)
    if shapes is None:
        shapes = cascade_shapes((len(z), len(y), len(x)), levels)
    shapes = [tuple(int(n) for n in s) for s in shapes]
    if not shapes or shapes[0] != (len(z), len(y), len(x)):
        raise ValueError(f"shapes must start with the finest grid {(len(z), len(y), len(x))}, not {shapes[:1]}")
    handles.append(VecPot(x, y, z, lib=lib))
    for nz, ny, nx in shapes[1:]:
        handles.append(VecPot(*[np.linspace(q[0], q[-1], n) for q, n in ((x, nx), (y, ny), (z, nz))], lib=lib))


def preprocess_magnetogram(x, y, z, bm, obs=None, mu=(1, 1, 1e-3, 1e-2, 1e-2), niter_max=10000, check=50, tol=1e-4,
                           dt0=None, dt_min=None, hist_rows=None, lib=None):
    """Preprocessing of the vector magnetogram bm (3,ny,nx) on the lower face of the mesh x, y, z towards a force-free,
    torque-free, smooth one: one-shot form of VecPot.preprocess (returns its (ierr, Bm, hist, info); the defaults are
    not tuned on real data).  Raises NdsmHipError on device / runtime failures (>= 9001)."""
    want = (3, len(y), len(x))
    if tuple(np.shape(bm)) != want:
        raise NdsmHipError(f"magnetogram of shape {tuple(np.shape(bm))}, the mesh needs {want} (code 9002)")
    V = VecPot(x, y, z, lib=lib)
    try:
        return V.preprocess(bm, obs=obs, mu=mu, niter_max=niter_max, check=check, tol=tol, dt0=dt0, dt_min=dt_min,
                            hist_rows=hist_rows)
    finally:
        V.close()


def magnetogram_balance(hist):
    """(eps_force, eps_torque) per row of a preprocess() history (one row or many): (|S1| + |S2| + |S3|) / S10 and
    (|S4| + |S5| + |S6|) / S11, the net Maxwell force and torque of the magnetogram relative to its magnetic pressure
    force and its moment.  Plain numpy."""
    h = np.asarray(hist, dtype=np.float64)
    if h.shape[-1] != 17:
        raise ValueError(f"history rows have 17 entries, not {h.shape[-1]}")
    s = np.abs(h[..., 9:15])
    return (s[..., 0] + s[..., 1] + s[..., 2]) / h[..., 15], (s[..., 3] + s[..., 4] + s[..., 5]) / h[..., 16]


def trace_paths(x, y, z, b, seeds, g=None, step=0.5, max_steps=None, direction="both", every=1, max_points=None,
                values=True, lib=None):
    """The field lines of b (3,nz,ny,nx) through seeds (nseeds,3) as polylines, with b, g and the running integral of
    g at their points: one-shot form of VecPot.paths (returns its FieldPaths tuple).  Raises NdsmHipError on device /
    runtime failures (>= 9001)."""
    _paths_args(every, max_points)
    V = _grid_handle(x, y, z, b, 0, lib)
    try:
        return V.paths(b, seeds, g=g, step=step, max_steps=max_steps, direction=direction, every=every,
                       max_points=max_points, values=values)
    finally:
        V.close()


def squashing_factor(x, y, z, b, seeds, g=None, integrand=0, twist=False, step=0.5, max_steps=None, lib=None):
    """Squashing factor Q of b (3,nz,ny,nx) at seeds (nseeds,3), with the twist number (twist=True) or the line
    integral of g: one-shot form of VecPot.squashing (returns its QMap tuple).  Raises NdsmHipError on device /
    runtime failures (>= 9001)."""
    if twist and g is not None:
        raise ValueError("twist=True forms g = curl b itself: give g or twist, not both")
    V = _grid_handle(x, y, z, b, 0, lib)
    try:
        return V.squashing(b, seeds, g=g, integrand=integrand, twist=twist, step=step, max_steps=max_steps)
    finally:
        V.close()


def perpendicular_squashing(x, y, z, b, seeds, g=None, integrand=0, twist=False, step=0.5, max_steps=None, lib=None):
    """Perpendicular squashing factor Q-perp of b (3,nz,ny,nx) at seeds (nseeds,3) next to Q, with the twist number
    (twist=True) or the line integral of g: one-shot form of VecPot.squashing_perp (returns its QPerpMap tuple).
    Raises NdsmHipError on device / runtime failures (>= 9001)."""
    if twist and g is not None:
        raise ValueError("twist=True forms g = curl b itself: give g or twist, not both")
    V = _grid_handle(x, y, z, b, 0, lib)
    try:
        return V.squashing_perp(b, seeds, g=g, integrand=integrand, twist=twist, step=step, max_steps=max_steps)
    finally:
        V.close()


def find_nulls(x, y, z, b, max_nulls=4096, merge=1e-6, lib=None):
    """Null points of b (3,nz,ny,nx) and their types: one-shot form of VecPot.nulls (returns its Nulls tuple).
    Raises NdsmHipError on device / runtime failures (>= 9001)."""
    V = _grid_handle(x, y, z, b, 0, lib)
    try:
        return V.nulls(b, max_nulls=max_nulls, merge=merge)
    finally:
        V.close()


def find_dips(x, y, z, b, plane_only=False, max_dips=None, lib=None):
    """Magnetic dips and bald patches of b (3,nz,ny,nx): one-shot form of VecPot.dips (returns its Dips tuple).
    Raises NdsmHipError on device / runtime failures (>= 9001)."""
    _dips_args(plane_only, max_dips)
    V = _grid_handle(x, y, z, b, 0, lib)
    try:
        return V.dips(b, plane_only=plane_only, max_dips=max_dips)
    finally:
        V.close()


def bald_patches(x, y, z, b, max_dips=None, lib=None):
    """The bald patches of b (3,nz,ny,nx) - where field lines touch the plane k = 0 from above -: find_dips with
    plane_only=True (returns VecPot.dips' Dips tuple, every record with bald).  Raises NdsmHipError on device /
    runtime failures (>= 9001)."""
    return find_dips(x, y, z, b, plane_only=True, max_dips=max_dips, lib=lib)


def find_skeleton(x, y, z, b, nulls=None, radius=0.5, nring=16, ring=None, capture=None, step=0.5, max_steps=None,
                  every=1, max_points=None, values=True, lib=None):
    """The spine-fan skeleton of the nulls of b (3,nz,ny,nx) and the null-to-null connections: one-shot form of
    VecPot.skeleton (returns its Skeleton tuple).  Raises NdsmHipError on device / runtime failures (>= 9001)."""
    _skeleton_args(radius, nring, ring, capture)
    _paths_args(every, max_points)
    V = _grid_handle(x, y, z, b, 0, lib)
    try:
        return V.skeleton(b, nulls=nulls, radius=radius, nring=nring, ring=ring, capture=capture, step=step,
                          max_steps=max_steps, every=every, max_points=max_points, values=values)
    finally:
        V.close()


def find_separators(x, y, z, b, skeleton=None, pairs=None, brackets=None, radius=0.5, capture=None, step=0.5,
                    max_steps=None, rounds=10, tol=1e-12, every=1, ring=None, values=True, lib=None):
    """The separator lines between the nulls of b (3,nz,ny,nx): one-shot form of VecPot.separators (returns its
    Separators tuple).  Raises NdsmHipError on device / runtime failures (>= 9001)."""
    _separator_args(radius, capture, rounds, tol)
    _paths_args(every, None)
    V = _grid_handle(x, y, z, b, 0, lib)
    try:
        return V.separators(b, skeleton=skeleton, pairs=pairs, brackets=brackets, radius=radius, capture=capture,
                            step=step, max_steps=max_steps, rounds=rounds, tol=tol, every=every, ring=ring, values=values)
    finally:
        V.close()


def field_line_helicity(x, y, z, b, seeds, gauge="devore", a=None, step=0.5, max_steps=None, direction="both",
                        niterex_max=10000, ncycles_max=1024, ex_tol=1e-13, vc_tol=1e-10, ms=5, mean=False,
                        mixed_precision=False, flxcrl=False, ngrids=0, return_fields=False, lib=None):
    """Field-line helicity of b (3,nz,ny,nx) at seeds (nseeds,3): one-shot form of VecPot.field_line_helicity.
    Returns (FieldLines, Helicity); with a given the lines are traced with g = a and the Helicity is None, else A
    comes from the chain of the gauge ("devore" or "coulomb") on the device.  Raises NdsmHipError on device /
    runtime failures (>= 9001)."""
    if gauge not in ("devore", "coulomb"):
        raise ValueError(f"gauge must be 'devore' or 'coulomb', not {gauge!r}")
    V = _grid_handle(x, y, z, b, ngrids, lib)
    try:
        return V.field_line_helicity(b, seeds, gauge=gauge, a=a, step=step, max_steps=max_steps, direction=direction,
                                     niterex_max=niterex_max, ncycles_max=ncycles_max, ex_tol=ex_tol, vc_tol=vc_tol,
                                     ms=ms, mean=mean, mixed_precision=mixed_precision, flxcrl=flxcrl,
                                     return_fields=return_fields)
    finally:
        V.close()


def solenoidal_projection(x, y, z, b, niterex_max=10000, ncycles_max=1024, ex_tol=1e-13, vc_tol=1e-10, ms=5,
                          mean=False, mixed_precision=False, ngrids=0, return_phi=False, lib=None):
    """Divergence cleaning of b (3,nz,ny,nx): one-shot form of VecPot.project (returns its Projection tuple).
    Raises NdsmHipError on device / runtime failures (>= 9001)."""
    V = _grid_handle(x, y, z, b, ngrids, lib)
    try:
        return V.project(b, niterex_max=niterex_max, ncycles_max=ncycles_max, ex_tol=ex_tol, vc_tol=vc_tol, ms=ms,
                         mean=mean, mixed_precision=mixed_precision, return_phi=return_phi)
    finally:
        V.close()

SLAB_FIELDS = ("rank", "z0", "z1", "g", "nloc", "k0", "ck0", "ck1", "pk0", "pk1", "cb0", "cb1")


def slab_plan(nshape, mesh, nranks, ngrids=0, lib=None):
    """The z-slab plan every rank derives (host arithmetic only - works without a GPU)."""
    L = lib or load_library()
    ns = np.asarray(nshape, dtype=np.intc)
    m = [_f64(v) for v in mesh]
    out = np.zeros((nranks, 12), dtype=np.intc)
    rc = L.ndsm_hip_slab_plan(ns.ctypes.data_as(_ip), _d(m[0]), _d(m[1]), _d(m[2]), int(ngrids), int(nranks),
                              out.ctypes.data_as(_ip))
    if rc != 0:
        raise NdsmHipError(f"ndsm_hip_slab_plan failed with code {rc} (slabs thinner than the ghost depth?)")
    return [dict(zip(SLAB_FIELDS, (int(v) for v in row))) for row in out]


class World:
    """Level 1 split into z-slabs.  rank >= 0: this process owns slab `rank` (RCCL);
    rank < 0: loop-back, all slabs on this GPU.  Arrays are numpy (nz, ny, nx)."""

    def __init__(self, nshape, mesh, bcs, nranks, rank=-1, ngrids=0, ms=5, ex_tol=1e-13, du_max=True,
                 nmax_exact=10000, lib=None):
        self.L = lib or load_library()
        self.nshape = [int(v) for v in nshape]
        ns = np.asarray(nshape, dtype=np.intc)
        m = [_f64(v) for v in mesh]
        self.h = ctypes.c_void_p()
        rc = self.L.ndsm_hip_world_create(ns.ctypes.data_as(_ip), _d(m[0]), _d(m[1]), _d(m[2]), bcs.encode(),
                                          int(ngrids), int(ms), float(ex_tol), 1 if du_max else 0, int(nmax_exact),
                                          int(nranks), int(rank), ctypes.byref(self.h))
        _check(rc, "ndsm_hip_world_create", self.L)
        self.nlocal = self.L.ndsm_hip_world_nlocal(self.h)
        self.dist_levels = self.L.ndsm_hip_world_dist_levels(self.h)
        self.slabs = []
        for i in range(1, self.nlocal + 1):
            info = np.zeros(12, dtype=np.intc)
            _check(self.L.ndsm_hip_world_slab(self.h, i, info.ctypes.data_as(_ip)), "world_slab", self.L)
            self.slabs.append(dict(zip(SLAB_FIELDS, (int(v) for v in info))))

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            self.L.ndsm_hip_world_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def upload(self, which, arr):
        """arr: the GLOBAL field (nz, ny, nx); every local slab takes its window incl. ghosts"""
        a = _f64(arr)
        assert a.shape == tuple(self.nshape[::-1])
        for i in range(1, self.nlocal + 1):
            _check(self.L.ndsm_hip_world_upload(self.h, i, which, _d(a), 0, a.shape[0]), "world_upload", self.L)

    def upload_window(self, ilocal, which, window, gz0):
        """window: planes [gz0, gz0 + window.shape[0]) of the global field"""
        a = _f64(window)
        _check(self.L.ndsm_hip_world_upload(self.h, ilocal, which, _d(a), int(gz0), a.shape[0]), "world_upload", self.L)

    def download(self, which, out=None):
        """owned planes of every local slab -> (global-shaped array, filled where owned)"""
        nx, ny, nz = self.nshape
        if out is None:
            out = np.full((nz, ny, nx), np.nan)
        for i, sl in enumerate(self.slabs, start=1):
            buf = np.empty((sl["z1"] - sl["z0"], ny, nx))
            _check(self.L.ndsm_hip_world_download(self.h, i, which, _d(buf)), "world_download", self.L)
            out[sl["z0"]:sl["z1"]] = buf
        return out

    def relax(self, n=1):
        _check(self.L.ndsm_hip_world_relax(self.h, n), "world_relax", self.L)

    def set_precision(self, mode):
        """0 fp64, != 0 mixed (fp64 residual, fp32 correction V-cycle on the level-1 slabs);
        returns True if solve() will run in mixed precision"""
        rc = self.L.ndsm_hip_world_set_precision(self.h, int(mode))
        if rc < 0:
            raise NdsmHipError(f"bad precision mode {mode}")
        return rc == 1

    def zero_rhs(self):
        """Declare rhs == 0 on level 1 (Laplace problem): the kernels stop reading it; same bits."""
        _check(self.L.ndsm_hip_world_zero_rhs(self.h), "world_zero_rhs", self.L)

    def vcycle(self, n=1):
        _check(self.L.ndsm_hip_world_vcycle(self.h, n), "world_vcycle", self.L)

    def solve(self, vc_tol=1e-10, nmax=1024, hist_len=0):
        du = ctypes.c_double(0)
        nc = ctypes.c_int(0)
        hist = np.zeros(max(hist_len, 1))
        ierr = self.L.ndsm_hip_world_solve(self.h, float(vc_tol), int(nmax), ctypes.byref(du), ctypes.byref(nc),
                                           _d(hist), int(hist_len))
        if ierr >= 9000:
            _check(ierr, "ndsm_hip_world_solve", self.L)
        return ierr, du.value, nc.value, hist[:min(hist_len, nc.value)].copy()

    def sync(self):
        _check(self.L.ndsm_hip_sync(), "sync", self.L)

    def timed(self, fn):
        _check(self.L.ndsm_hip_timer_start(), "timer_start", self.L)
        fn()
        ms = ctypes.c_double(0)
        _check(self.L.ndsm_hip_timer_stop(ctypes.byref(ms)), "timer_stop", self.L)
        return ms.value


def dist_unique_id(lib=None):
    L = lib or load_library()
    buf = ctypes.create_string_buffer(128)
    _check(L.ndsm_hip_dist_unique_id(buf), "ndsm_hip_dist_unique_id", L)
    return buf.raw


def dist_init(rank, nranks, uid, lib=None):
    L = lib or load_library()
    _check(L.ndsm_hip_dist_init(int(rank), int(nranks), ctypes.c_char_p(uid)), "ndsm_hip_dist_init", L)


def dist_info(lib=None):
    """(rank, nranks) as the RCCL communicator itself reports them; nranks == 0: none is up"""
    L = lib or load_library()
    r, n = ctypes.c_int(0), ctypes.c_int(0)
    _check(L.ndsm_hip_dist_info(ctypes.byref(r), ctypes.byref(n)), "ndsm_hip_dist_info", L)
    return r.value, n.value


def dist_finalize(lib=None):
    L = lib or load_library()
    _check(L.ndsm_hip_dist_finalize(), "ndsm_hip_dist_finalize", L)


def poisson_solve(u, rhs, mesh, bcs, ms=5, ex_tol=1e-13, du_max=True, nmax_exact=10000, vc_tol=1e-10, nmax=1024,
                  ngrids=0, hist_len=0, lib=None, precision=0):
    """laplace(u) = rhs on the device.  u: initial guess + Dirichlet data,
    numpy order (nz, ny, nx).  precision: 0 fp64 (reference arithmetic), 1 mixed (fp64 residual,
    fp32 correction V-cycle on level 1) where level 1 is large enough, 2 mixed wherever possible.
    Returns (ierr, u, du_last, hist, ncycles)."""
    L = lib or load_library()
    u = _f64(u).copy()
    nd = u.ndim
    ns = np.asarray(u.shape[::-1], dtype=np.intc)
    m = [_f64(v) for v in mesh]
    while len(m) < 3:
        m.append(np.zeros(2))
    iopt = np.zeros(16, dtype=np.intc)
    ropt = np.zeros(16)
    iopt[L.get_iopt_ms()] = ms
    iopt[L.get_iopt_ncycles()] = nmax
    iopt[L.get_iopt_iopt_nmaxex()] = nmax_exact
    iopt[L.get_iopt_dumax()] = 1 if du_max else 0
    iopt[L.get_iopt_ngrids()] = ngrids
    iopt[L.get_iopt_prec()] = precision
    ropt[L.get_ropt_vtol()] = vc_tol
    ropt[L.get_ropt_ctol()] = ex_tol
    hist = np.zeros(max(hist_len, 1))
    rp = _d(_f64(rhs)) if rhs is not None else None
    rhs_keep = _f64(rhs) if rhs is not None else None
    rp = _d(rhs_keep) if rhs_keep is not None else None
    ierr = L.ndsm_hip_poisson_solve(nd, ns.ctypes.data_as(_ip), _d(m[0]), _d(m[1]), _d(m[2]), bcs.encode(),
                                    iopt.ctypes.data_as(_ip), _d(ropt), _d(u), rp, _d(hist), int(hist_len))
    if ierr >= 9000:
        _check(ierr, "ndsm_hip_poisson_solve", L)
    nc = int(iopt[L.get_iopt_ncyc_out()])
    return ierr, u, float(ropt[L.get_ropt_dulast()]), hist[:min(hist_len, nc)].copy(), nc
