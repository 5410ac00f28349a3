"""The alpha map against the composite it replaces, and one Grad-Rubin pass against solve_field, timed with device
events in one run: usage probe_nlfff.py [--repeats R] [n ...]   (default 128, --repeats 5)

Per size n^3, on one VecPot handle and the flux tube of tests/alpha_model.py (q a = 1, B_z > 0: with polarity +1 every
line runs down to the lower face or out through a side), step 0.5, the default max_steps; every array stays in device
memory.  Each variant is warmed up once and then timed R times between two events on the library stream; the calls are
repeated inside one timed window until it is at least 0.2 s long; the variants of a pair alternate window by window.
  map        ndsm_hip_vecpot_alpha_map_device: alpha and status for the n^3 nodes
  trace      ndsm_hip_vecpot_trace_device with the n^3 node seeds, direction -1: the kernel of the composite a caller
             would build from the public trace (24 B/pt of seeds in, 52 B/pt out), without its host part
  interp     the composite's host part, wall clock: the numpy bilinear interpolation of the downloaded ends (the
             download itself is not included)
  pass       ndsm_hip_vecpot_nlfff_device, start = 1, niter_max = 1: one alpha map, three solves, the curl, the history
  field      ndsm_hip_vecpot_solve_field_device on the same grid from the same initial guess (zeros)
Reported per variant: median, min and max time of one call; the ratios of the medians.  The map's alpha is compared
with the composite's bit for bit on the way."""
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
from alpha_model import alpha_of_ends, flux_tube, node_seeds  # noqa: E402
from golden_inputs import uniform_mesh  # noqa: E402

WINDOW_S = 0.2


def main(sizes, repeats=5):
    L = ndsm_amd.load_library()
    assert L.ndsm_hip_init(-1) == 0, _lib.last_error(L)
    rows = []
    for n in sizes:
        mesh = uniform_mesh([n, n, n])
        b, alpha_true, _r, _a = flux_tube(mesh)
        b = np.ascontiguousarray(b)
        alpha0 = np.ascontiguousarray(alpha_true[0])
        V = ndsm_amd.VecPot(*mesh)
        N = n ** 3
        max_steps = V.default_max_steps(0.5)
        ioptc, ropt = V._options(10000, 1024, 1e-13, 1e-10, 5, False, False, False)
        host = {"B": b, "Bw": b.copy(), "A": np.zeros(3 * N), "alpha0": alpha0, "alpha": np.zeros(N),
                "status": np.zeros(N, dtype=np.int32), "seeds": np.ascontiguousarray(node_seeds(mesh)),
                "ends": np.zeros((N, 3)), "length": np.zeros(N), "integral": np.zeros(N),
                "tstatus": np.zeros(N, dtype=np.int32), "nsteps": np.zeros(N, dtype=np.int32)}
        dev = {}
        for k, a in host.items():
            dev[k] = ctypes.c_void_p()
            assert L.ndsm_hip_device_alloc(a.nbytes, ctypes.byref(dev[k])) == 0, _lib.last_error(L)
        for k in ("B", "alpha0", "seeds"):
            assert L.ndsm_hip_memcpy_h2d(dev[k], host[k].ctypes.data, host[k].nbytes) == 0
        hist, niter = np.zeros((1, 4)), ctypes.c_int(0)

        def fetch(k):
            assert L.ndsm_hip_memcpy_d2h(host[k].ctypes.data, dev[k], host[k].nbytes) == 0
            return host[k].copy()

        def reset():
            """the working copy of B and a zero A, as both solving variants start"""
            assert L.ndsm_hip_memcpy_h2d(dev["Bw"], host["B"].ctypes.data, host["B"].nbytes) == 0
            assert L.ndsm_hip_memcpy_h2d(dev["A"], host["A"].ctypes.data, host["A"].nbytes) == 0

        def amap():
            rc = L.ndsm_hip_vecpot_alpha_map_device(V.h, dev["B"], dev["alpha0"], 1, 0.5, max_steps, dev["alpha"],
                                                    dev["status"])
            assert rc == 0, _lib.last_error(L)

        def trace():
            rc = L.ndsm_hip_vecpot_trace_device(V.h, dev["B"], None, N, dev["seeds"], 0.5, max_steps, -1, dev["ends"],
                                                dev["length"], dev["integral"], dev["tstatus"], dev["nsteps"])
            assert rc == 0, _lib.last_error(L)

        def one_pass():
            rc = L.ndsm_hip_vecpot_nlfff_device(V.h, ioptc.ctypes.data_as(_lib._ip), _lib._d(ropt), dev["Bw"],
                                                dev["alpha0"], 1, 1, 1, 0.0, 0.5, max_steps, dev["A"], dev["alpha"],
                                                dev["status"], _lib._d(hist), ctypes.byref(niter))
            assert rc == 0, _lib.last_error(L)

        def field():
            rc = L.ndsm_hip_vecpot_solve_field_device(V.h, ioptc.ctypes.data_as(_lib._ip), _lib._d(ropt), dev["A"],
                                                      dev["Bw"])
            assert rc == 0, _lib.last_error(L)

        def timed(fn, count, before=None):
            total = 0.0
            for _ in range(count):
                if before:
                    before()
                assert L.ndsm_hip_timer_start() == 0
                fn()
                ms = ctypes.c_double(0)
                assert L.ndsm_hip_timer_stop(ctypes.byref(ms)) == 0
                total += ms.value * 1e-3
            return total / count

        def pair(name_a, fn_a, name_b, fn_b, before=None):
            fn_before = before or (lambda: None)
            fn_before(); fn_a(); fn_before(); fn_b()                  # warm-up
            count = max(1, int(np.ceil(WINDOW_S / timed(fn_a, 1, before))))
            ts = {name_a: [], name_b: []}
            for _ in range(repeats):
                ts[name_a].append(timed(fn_a, count, before))
                ts[name_b].append(timed(fn_b, count, before))
            out = {"calls_per_window_" + name_a: count}
            for name, t in ts.items():
                t.sort()
                out.update({name + "_ms": round(float(np.median(t)) * 1e3, 3), name + "_min_ms": round(t[0] * 1e3, 3),
                            name + "_max_ms": round(t[-1] * 1e3, 3)})
            out[name_a + "_over_" + name_b] = round(out[name_a + "_ms"] / out[name_b + "_ms"], 4)
            return out

        row = {"n": n, "nodes": N, "max_steps": max_steps, "field_MB": round(b.nbytes / 1e6, 1)}
        row.update(pair("map", amap, "trace", trace))
        alpha, status = fetch("alpha"), fetch("status")
        ends, tstatus = fetch("ends"), fetch("tstatus")
        t0 = time.perf_counter()
        want = alpha_of_ends(mesh, alpha0, ends, tstatus)
        row["interp_host_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        row["same_bits"] = bool(np.array_equal(alpha.view(np.uint64), want.view(np.uint64)) and
                                np.array_equal(status, tstatus))
        row["zlo_nodes"] = int((status == 5).sum())
        row["steps_max"] = int(fetch("nsteps").max())
        row.update(pair("pass", one_pass, "field", field, before=reset))
        row["pass_hist"] = hist[0].tolist()
        for p in dev.values():
            L.ndsm_hip_device_free(p)
        V.close()
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


if __name__ == "__main__":
    args = sys.argv[1:]
    repeats = 5
    if "--repeats" in args:
        i = args.index("--repeats")
        repeats = int(args[i + 1])
        del args[i:i + 2]
    main([int(a) for a in args] or [128], repeats=repeats)
