"""Wall time of a DeVore-gauge helicity against a Coulomb-gauge one, device-resident arrays (no PCIe in the timed
calls): usage time_devore.py [--devore-only] [n ...]   (default 128 256 512)

Per size, on one VecPot handle and the ABC field (tests/test_gpu_field.py), one warm-up call each, then the median
of three:
  solve     ndsm_hip_vecpot_solve_device (the potential field B_p of B.n)
  coulomb   ndsm_hip_vecpot_helicity_device (potential + three field solves + reduction)
  devore    the DeVore-gauge helicity chain: ndsm_hip_vecpot_solve_device on a copy of B (-> B_p), then
            ndsm_hip_vecpot_devore_device on B and B_p (the copy of B is staged outside the timed region)
  entry     ndsm_hip_vecpot_devore_device alone (base plane, columns, curl, reduction)
and |H_R(devore) - H_R(coulomb)| / |H_R(coulomb)|, the same for H_J.  --devore-only: the devore entry alone (a
warm-up and three calls per size), for a kernel trace of the scan kernels."""
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import ndsm_amd  # noqa: E402
from ndsm_amd import _lib  # noqa: E402
from test_gpu_field import abc_field  # noqa: E402

VC_TOL = 1e-10


def main(sizes, devore_only=False):
    L = ndsm_amd.load_library()
    assert L.ndsm_hip_init(-1) == 0, _lib.last_error(L)
    ip = ctypes.POINTER(ctypes.c_int)
    dp = ctypes.POINTER(ctypes.c_double)
    rows = []
    for n in sizes:
        mesh, b = abc_field([n, n, n])
        b = np.ascontiguousarray(b)
        V = ndsm_amd.VecPot(*mesh)
        nbytes = b.nbytes
        bufs = {}
        for k in ("B", "Bw", "A", "Ap", "Bp", "Ad", "Apd"):
            p = ctypes.c_void_p()
            assert L.ndsm_hip_device_alloc(nbytes, ctypes.byref(p)) == 0, _lib.last_error(L)
            bufs[k] = p
        zero = np.zeros_like(b)
        assert L.ndsm_hip_memcpy_h2d(bufs["B"], b.ctypes.data, nbytes) == 0

        def stage():             # outside the timed region: the copy of B, a zero initial guess
            assert L.ndsm_hip_memcpy_h2d(bufs["Bw"], b.ctypes.data, nbytes) == 0
            assert L.ndsm_hip_memcpy_h2d(bufs["A"], zero.ctypes.data, nbytes) == 0

        out_c, out_d, out_e = np.zeros(8), np.zeros(8), np.zeros(8)

        def devore_chain(io, ro):
            ierr = L.ndsm_hip_vecpot_solve_device(V.h, io, ro, bufs["A"], bufs["Bw"])
            rc = L.ndsm_hip_vecpot_devore_device(V.h, bufs["B"], bufs["Bw"], bufs["Ad"], bufs["Apd"],
                                                 out_d.ctypes.data_as(dp))
            return rc or ierr

        calls = {
            "solve": lambda io, ro: L.ndsm_hip_vecpot_solve_device(V.h, io, ro, bufs["A"], bufs["Bw"]),
            "coulomb": lambda io, ro: L.ndsm_hip_vecpot_helicity_device(V.h, io, ro, bufs["B"], bufs["A"], bufs["Ap"],
                                                                        bufs["Bp"], out_c.ctypes.data_as(dp)),
            "devore": devore_chain,
            # (B_p of the last devore chain is left in Bw)
            "entry": lambda io, ro: L.ndsm_hip_vecpot_devore_device(V.h, bufs["B"], bufs["Bw"], bufs["Ad"],
                                                                    bufs["Apd"], out_e.ctypes.data_as(dp)),
        }
        if devore_only:
            stage()
            ioptc, ropt = V._options(10000, 1024, 1e-13, VC_TOL, 5, False, 0, False)
            assert L.ndsm_hip_vecpot_solve_device(V.h, ioptc.ctypes.data_as(ip), ropt.ctypes.data_as(dp), bufs["A"],
                                                  bufs["Bw"]) in (0, 1)
            calls = {"entry": calls["entry"]}
        row = {"n": n}
        for name, fn in calls.items():
            ts = []
            for rep in range(4):
                ioptc, ropt = V._options(10000, 1024, 1e-13, VC_TOL, 5, False, 0, False)
                if name != "entry":
                    stage()
                t = time.perf_counter()
                ierr = fn(ioptc.ctypes.data_as(ip), ropt.ctypes.data_as(dp))
                dt = time.perf_counter() - t
                assert ierr in (0, 1), (name, ierr, _lib.last_error(L))
                if rep:
                    ts.append(dt)
            row[name + "_s"] = round(float(np.median(ts)), 5)
            row[name + "_ierr"] = int(ierr)
        if not devore_only:
            row.update(H_R_coulomb=float(out_c[0]), H_R_devore=float(out_d[0]), H_J_coulomb=float(out_c[1]),
                       H_J_devore=float(out_d[1]), dH_R_rel=float(abs(out_d[0] - out_c[0]) / abs(out_c[0])),
                       dH_J_rel=float(abs(out_d[1] - out_c[1]) / abs(out_c[1])), recon_rms_coulomb=float(out_c[5]),
                       recon_rms_devore=float(out_d[5]), devore_over_coulomb=round(row["devore_s"] / row["coulomb_s"], 3),
                       entry_equal=bool(np.array_equal(out_d, out_e)))
        row["scan_bytes"] = 80 * n ** 3                     # compulsory bytes of the columns kernel
        for p in bufs.values():
            L.ndsm_hip_device_free(p)
        V.close()
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


if __name__ == "__main__":
    args = sys.argv[1:]
    only = "--devore-only" in args
    main([int(a) for a in args if a != "--devore-only"] or [128, 256, 512], devore_only=only)
