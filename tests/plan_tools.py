"""Readable front end of ndsm_hip_debug_relax_plan for the tests: the plan of a relax call as dicts with names for the
enumerators of csrc/relax_plan.hpp."""
import ctypes

import numpy as np

from ndsm_amd import _lib

_ip = ctypes.POINTER(ctypes.c_int)

PLAN_KINDS = ("", "small3d", "small2d", "medium2d", "fused", "block", "color3d", "color2d")
PLAN_MODES = ("", "R", "M", "P")
PLAN_INSTS = ("", "F2 136x30/1024", "F2 136x30/1024 L1", "F2 136x22/768", "F2 72x28/512", "F1 132x23/768",
              "F1 132x31/1024", "F1R 136x22/768", "F2M 136x30/1024", "F1M 132x31/1024", "F1M 132x23/768",
              "F1P 132x31/1024", "F2P 136x30/1024")


def relax_plan(n, nsweeps, lb=None, ub=None, all_neumann=False, zown=None, k0=0, nzg=None, variant=0, window=False,
               fp32=False, rhs=True, want_res=False, want_met=False, corr=False, coarse_plane=0, nbufs=2, keep=-1,
               fused_cfg=(0, 0, 0, 0, -1), block_cfg=(0, 0), no_block=False, L=None):
    """The launches a relax call of `nsweeps` sweeps makes on a level of shape n = (nx, ny[, nz]), as the library's
    planner decides them (host code: no GPU needed).  Returns a dict: err (0 or 9002), passes (one dict each: kind,
    sweeps, mode '' / 'R' / 'M' / 'P', inst, odd_nx, bz, src, dst, prolong_first, mean_shift), result (buffer index),
    res_done, met_done, prolong_only."""
    L = L or _lib.load_library()
    n = list(n) + [1] * (3 - len(n))
    ndim = 3 if n[2] > 1 else 2
    lb = list(lb) if lb is not None else [0, 0, 0]
    ub = list(ub) if ub is not None else [m - 1 for m in n]
    zown = zown if zown is not None else (0, n[2])
    grid = np.array([ndim] + n + lb + ub + [int(all_neumann), k0, n[2] if nzg is None else nzg, zown[0], zown[1]],
                    dtype=np.intc)
    req = np.array([nsweeps, variant, window, fp32, rhs, want_res, want_met, corr, coarse_plane, nbufs >= 2, nbufs >= 3,
                    keep], dtype=np.int64)
    knobs = np.array(list(fused_cfg) + list(block_cfg) + [int(no_block)], dtype=np.int64)
    cap = 6 + 9 * max(nsweeps, 1)
    out = np.zeros(cap, dtype=np.intc)
    i64 = ctypes.POINTER(ctypes.c_int64)
    rc = L.ndsm_hip_debug_relax_plan(0, grid.ctypes.data_as(_ip), req.ctypes.data_as(i64), knobs.ctypes.data_as(i64),
                                     cap, out.ctypes.data_as(_ip))
    _lib._check(rc, "debug_relax_plan", L)
    rows = out[6:6 + 9 * out[1]].reshape(-1, 9)
    passes = [dict(kind=PLAN_KINDS[r[0]], sweeps=int(r[1]), mode=PLAN_MODES[r[2]], inst=PLAN_INSTS[r[3] & 15],
                   odd_nx=bool(r[3] & 16), bz=int(r[4]), src=int(r[5]), dst=int(r[6]), prolong_first=bool(r[7]),
                   mean_shift=bool(r[8])) for r in rows]
    return dict(err=int(out[0]), passes=passes, result=int(out[2]), res_done=bool(out[3]), met_done=bool(out[4]),
                prolong_only=bool(out[5]))


def fused_z_chunks(nzo, tiles, slots, depth, res=False, work_items=0, L=None):
    """(chunks, planes per chunk) of a fused launch over nzo owned planes (the planner's z chunking)"""
    L = L or _lib.load_library()
    req = np.array([nzo, tiles, slots, depth, res, work_items], dtype=np.int64)
    out = np.zeros(2, dtype=np.intc)
    rc = L.ndsm_hip_debug_relax_plan(1, None, req.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), None, 2,
                                     out.ctypes.data_as(_ip))
    _lib._check(rc, "debug_relax_plan", L)
    return int(out[0]), int(out[1])
