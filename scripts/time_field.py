"""Wall time of the current-carrying-field entries against the potential solve, device-resident arrays (no PCIe
in the timed calls): usage time_field.py [n ...]   (default 128 256 512)

Per size, on one VecPot handle and the ABC field (tests/test_gpu_field.py): ndsm_hip_vecpot_solve_device,
ndsm_hip_vecpot_solve_field_device and ndsm_hip_vecpot_helicity_device, one warm-up call each, then the median
of three; V-cycles of the last 3-D solve that iterated (ioptc slot 10).  helicity - solve - solve_field is what
the reduction costs beyond the two 3-D phases, less the face phase it saves."""
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


def main(sizes):
    L = ndsm_amd.load_library()
    assert L.ndsm_hip_init(-1) == 0, _lib.last_error(L)
    ip = ctypes.POINTER(ctypes.c_int)
    dp = ctypes.POINTER(ctypes.c_double)
    rows = []
    for n in sizes:
        mesh, b = abc_field([n, n, n])
        V = ndsm_amd.VecPot(*mesh)
        nbytes = b.nbytes
        bufs = {}
        for k in ("B", "A", "Ap", "Bp", "Bw"):
            p = ctypes.c_void_p()
            assert L.ndsm_hip_device_alloc(nbytes, ctypes.byref(p)) == 0, _lib.last_error(L)
            bufs[k] = p
        bc = np.ascontiguousarray(b)
        zero = np.zeros_like(bc)

        def stage():             # outside the timed region: B in, a zero initial guess
            assert L.ndsm_hip_memcpy_h2d(bufs["Bw"], bc.ctypes.data, nbytes) == 0
            assert L.ndsm_hip_memcpy_h2d(bufs["A"], zero.ctypes.data, nbytes) == 0

        assert L.ndsm_hip_memcpy_h2d(bufs["B"], bc.ctypes.data, nbytes) == 0
        out = np.zeros(8)
        calls = {
            "solve": lambda io, ro: L.ndsm_hip_vecpot_solve_device(V.h, io, ro, bufs["A"], bufs["Bw"]),
            "solve_field": lambda io, ro: L.ndsm_hip_vecpot_solve_field_device(V.h, io, ro, bufs["A"], bufs["Bw"]),
            "helicity": lambda io, ro: L.ndsm_hip_vecpot_helicity_device(V.h, io, ro, bufs["B"], bufs["A"], bufs["Ap"],
                                                                         bufs["Bp"], out.ctypes.data_as(dp)),
        }
        row = {"n": n}
        for name, fn in calls.items():
            ts = []
            for rep in range(4):
                ioptc, ropt = V._options(10000, 1024, 1e-13, 1e-10, 5, False, 0, False)
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
        row["H_R"] = float(out[0])
        row["recon_rms"] = float(out[5])
        row["helicity_minus_both_s"] = round(row["helicity_s"] - row["solve_s"] - row["solve_field_s"], 4)
        for p in bufs.values():
            L.ndsm_hip_device_free(p)
        V.close()
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


if __name__ == "__main__":
    main([int(a) for a in sys.argv[1:]] or [128, 256, 512])
