"""Wall time of the solenoidal projection, device-resident arrays (no PCIe in the timed calls): usage
time_project.py [n ...]   (default 128 256 512)

Per size, on one VecPot handle and B = ABC + 0.3 grad(psi) (tests/test_gpu_project.py):
ndsm_hip_vecpot_project_device, and for scale ndsm_hip_vecpot_solve_device and ndsm_hip_vecpot_helicity_device on
the same handle; one warm-up call each, then the median of three.  V-cycles of the projection solve (ioptc slot
10).  The same all-Neumann problem is then solved once more through a standalone MGSolver (the right-hand side
div_h B - c made on the host) for mg_info: exact sweeps on the coarsest level and the number of coarsest solves
that ran to nmax_exact without reaching ex_tol (every all-Neumann level restricts a residual that is compatible
only to rounding), and its solve time alone."""
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
from golden_inputs import uniform_mesh  # noqa: E402
from test_gpu_project import EPS, abc, div, grad_psi, weights  # noqa: E402

VC_TOL = 1e-10


def main(sizes):
    L = ndsm_amd.load_library()
    assert L.ndsm_hip_init(-1) == 0, _lib.last_error(L)
    ip = ctypes.POINTER(ctypes.c_int)
    dp = ctypes.POINTER(ctypes.c_double)
    rows = []
    for n in sizes:
        mesh = uniform_mesh([n, n, n])
        b = np.ascontiguousarray(abc(mesh) + EPS * grad_psi(mesh))
        V = ndsm_amd.VecPot(*mesh)
        nbytes = b.nbytes
        bufs = {}
        for k in ("B", "Bw", "A", "Ap", "Bp"):
            p = ctypes.c_void_p()
            assert L.ndsm_hip_device_alloc(nbytes, ctypes.byref(p)) == 0, _lib.last_error(L)
            bufs[k] = p
        phi = ctypes.c_void_p()
        assert L.ndsm_hip_device_alloc(nbytes // 3, ctypes.byref(phi)) == 0, _lib.last_error(L)
        zero = np.zeros_like(b)

        def stage():             # outside the timed region: B in, a zero initial guess
            assert L.ndsm_hip_memcpy_h2d(bufs["Bw"], b.ctypes.data, nbytes) == 0
            assert L.ndsm_hip_memcpy_h2d(bufs["A"], zero.ctypes.data, nbytes) == 0

        assert L.ndsm_hip_memcpy_h2d(bufs["B"], b.ctypes.data, nbytes) == 0
        out4, out8 = np.zeros(4), np.zeros(8)
        calls = {
            "project": lambda io, ro: L.ndsm_hip_vecpot_project_device(V.h, io, ro, bufs["Bw"], phi,
                                                                       out4.ctypes.data_as(dp)),
            "solve": lambda io, ro: L.ndsm_hip_vecpot_solve_device(V.h, io, ro, bufs["A"], bufs["Bw"]),
            "helicity": lambda io, ro: L.ndsm_hip_vecpot_helicity_device(V.h, io, ro, bufs["B"], bufs["A"], bufs["Ap"],
                                                                         bufs["Bp"], out8.ctypes.data_as(dp)),
        }
        row = {"n": n}
        for name, fn in calls.items():
            ts = []
            for rep in range(4):
                ioptc, ropt = V._options(10000, 1024, 1e-13, VC_TOL, 5, False, 0, False)
                stage()
                t = time.perf_counter()
                ierr = fn(ioptc.ctypes.data_as(ip), ropt.ctypes.data_as(dp))
                dt = time.perf_counter() - t
                assert ierr in (0, 1), (name, ierr, _lib.last_error(L))
                if rep:
                    ts.append(dt)
            row[name + "_s"] = round(float(np.median(ts)), 4)
            row[name + "_ncyc"] = int(ioptc[10])
            row[name + "_ierr"] = int(ierr)
        row.update(c=float(out4[0]), divB_before=float(out4[1]), divB_after=float(out4[2]),
                   E_removed=float(out4[3]))
        for p in list(bufs.values()) + [phi]:
            L.ndsm_hip_device_free(p)
        V.close()
        # the same solve alone, for mg_info
        d = div(b, mesh)
        w = weights(mesh)
        rhs = d - (w * d).sum() / w.sum()
        S = _lib.MGSolver([n, n, n], mesh, "NNNNNN")
        S.upload(1, _lib.BUF_U, np.zeros_like(rhs))
        S.upload(1, _lib.BUF_RHS, rhs)
        t = time.perf_counter()
        ierr, du, nc, _ = S.solve(vc_tol=VC_TOL, nmax=1024)
        row["mg_solve_s"] = round(time.perf_counter() - t, 4)
        sweeps, unconverged = S.info()
        S.close()
        row.update(mg_ncyc=int(nc), mg_ierr=int(ierr), exact_sweeps=int(sweeps), coarse_unconverged=int(unconverged),
                   exact_sweeps_per_cycle=round(sweeps / max(1, nc), 1))
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


if __name__ == "__main__":
    main([int(a) for a in sys.argv[1:]] or [128, 256, 512])
