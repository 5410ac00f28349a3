"""Field-line paths on device-resident arrays, timed with device events: usage
time_paths.py [--repeats R] [--every E,E...] [n ...]   (default 128 256, --every 1,8, --repeats 5)

The protocol of time_trace.py.  Per size n^3, on one VecPot handle and the ABC field (tests/test_gpu_field.py): one
seed per node of the bottom face (n^2 seeds), both directions (2 n^2 lines), step 0.5, the default max_steps, G = B
(the values do not matter to the cost); B, G, the seeds and every output stay in device memory.  Per stride `every`:
a counting call gives the total, the four point arrays get exactly that many slots, and three variants are timed in
the same run - the trace entry with G, the counting call of the paths entry (max_points = 0) and the filling call
(max_points = total, all four point arrays) - each warmed up once and then timed R times between two events on the
library stream; the calls are repeated inside one timed window until it is at least 0.2 s long.  Reported per variant:
median, min and max time of one call; and the ratios counting / trace and filling / trace, the points and the bytes
a filling call stores (80 B per point)."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import ndsm_amd  # noqa: E402
from ndsm_amd import _lib  # noqa: E402
from test_gpu_field import abc_field  # noqa: E402

WINDOW_S = 0.2


def main(sizes, everys=(1, 8), repeats=5):
    L = ndsm_amd.load_library()
    assert L.ndsm_hip_init(-1) == 0, _lib.last_error(L)
    rows = []
    for n in sizes:
        mesh, b = abc_field([n, n, n])
        b = np.ascontiguousarray(b)
        V = ndsm_amd.VecPot(*mesh)
        X, Y = np.meshgrid(mesh[0], mesh[1], indexing="xy")
        seeds = np.ascontiguousarray(np.stack([X.ravel(), Y.ravel(), np.full(X.size, mesh[2][0])], axis=1))
        ns, nl = len(seeds), 2 * len(seeds)
        max_steps = V.default_max_steps(0.5)
        host = {"B": b, "seeds": seeds, "ends": np.zeros((nl, 3)), "length": np.zeros(nl), "integral": np.zeros(nl),
                "status": np.zeros(nl, dtype=np.int32), "nsteps": np.zeros(nl, dtype=np.int32),
                "offsets": np.zeros(nl + 1, dtype=np.int64)}
        dev = {}

        def alloc(nbytes):
            p = ctypes.c_void_p()
            assert L.ndsm_hip_device_alloc(nbytes, ctypes.byref(p)) == 0, _lib.last_error(L)
            return p
        for k, a in host.items():
            dev[k] = alloc(a.nbytes)
        for k in ("B", "seeds"):
            assert L.ndsm_hip_memcpy_h2d(dev[k], host[k].ctypes.data, host[k].nbytes) == 0
        lines = [dev[k] for k in ("ends", "length", "integral", "status", "nsteps")]
        total = np.zeros(1, dtype=np.int64)

        def trace():
            rc = L.ndsm_hip_vecpot_trace_device(V.h, dev["B"], dev["B"], ns, dev["seeds"], 0.5, max_steps, 0, *lines)
            assert rc == 0, _lib.last_error(L)

        def paths(every, cap, pts):
            rc = L.ndsm_hip_vecpot_paths_device(V.h, dev["B"], dev["B"], ns, dev["seeds"], 0.5, max_steps, 0, every, cap,
                                                *lines, dev["offsets"], total.ctypes.data, *pts)
            assert rc == 0, _lib.last_error(L)

        def timed(fn, count):
            assert L.ndsm_hip_timer_start() == 0
            for _ in range(count):
                fn()
            ms = ctypes.c_double(0)
            assert L.ndsm_hip_timer_stop(ctypes.byref(ms)) == 0
            return ms.value * 1e-3 / count

        def measure(fn):
            fn()                                              # warm-up
            first = timed(fn, 1)
            count = max(1, int(np.ceil(WINDOW_S / first)))
            ts = sorted(timed(fn, count) for _ in range(repeats))
            return float(np.median(ts)), ts[0], ts[-1]

        for every in everys:
            paths(every, 0, [None] * 4)
            npts = int(total[0])
            pts = [alloc(24 * npts), alloc(24 * npts), alloc(24 * npts), alloc(8 * npts)]
            row = {"n": n, "lines": nl, "max_steps": max_steps, "every": every, "points": npts,
                   "stored_MB": round(80 * npts / 1e6, 1)}
            for tag, fn in (("trace", trace), ("count", lambda: paths(every, 0, [None] * 4)),
                            ("fill", lambda: paths(every, npts, pts))):
                med, lo, hi = measure(fn)
                row.update({tag + "_ms": round(med * 1e3, 3), tag + "_min_ms": round(lo * 1e3, 3),
                            tag + "_max_ms": round(hi * 1e3, 3)})
            assert int(total[0]) == npts
            row["count_over_trace"] = round(row["count_ms"] / row["trace_ms"], 3)
            row["fill_over_trace"] = round(row["fill_ms"] / row["trace_ms"], 3)
            row["stored_GB_per_s"] = round(80 * npts / ((row["fill_ms"] - row["count_ms"]) * 1e-3) / 1e9, 1)
            for p in pts:
                L.ndsm_hip_device_free(p)
            print(json.dumps(row), flush=True)
            rows.append(row)
        for p in dev.values():
            L.ndsm_hip_device_free(p)
        V.close()
    return rows


if __name__ == "__main__":
    args = sys.argv[1:]
    opts = {"--repeats": "5", "--every": "1,8"}
    for o in list(opts):
        if o in args:
            i = args.index(o)
            opts[o] = args[i + 1]
            del args[i:i + 2]
    main([int(a) for a in args] or [128, 256], everys=tuple(int(e) for e in opts["--every"].split(",")),
         repeats=int(opts["--repeats"]))
