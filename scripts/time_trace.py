"""Field-line tracing on device-resident arrays, timed with device events: usage
time_trace.py [--flh-max N] [--repeats R] [n ...]   (default 128 256 512, --flh-max 256, --repeats 5)

Per size n^3, on one VecPot handle and the ABC field (tests/test_gpu_field.py): one seed per node of the bottom
face (n^2 seeds), both directions (2 n^2 lines), step 0.5, the default max_steps; B, G, the seeds and the outputs
stay in device memory.  Each variant - without G, with G (G = B: the values do not matter to the cost) - is warmed
up once and then timed R times between two events on the library stream; the calls are repeated inside one timed
window until it is at least 0.2 s long.  Reported per variant: median, min and max time of one call, lines/s, RK4
steps/s, and the gathered bytes/s = stages x 24 (48 with G) corner values x 8 B / time, where stages = 4 per
step + 3 per redone exit step (what the lanes ask for, not what leaves HBM: neighbouring corners share lines).
Up to n = --flh-max also the wall time of VecPot.field_line_helicity(gauge="devore") for those seeds against the
VecPot.helicity(gauge="devore") it contains (host arrays in, median of three after one warm-up each)."""
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

WINDOW_S = 0.2


def main(sizes, flh_max=256, repeats=5):
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
                "status": np.zeros(nl, dtype=np.int32), "nsteps": np.zeros(nl, dtype=np.int32)}
        dev = {}
        for k, a in host.items():
            dev[k] = ctypes.c_void_p()
            assert L.ndsm_hip_device_alloc(a.nbytes, ctypes.byref(dev[k])) == 0, _lib.last_error(L)
        for k in ("B", "seeds"):
            assert L.ndsm_hip_memcpy_h2d(dev[k], host[k].ctypes.data, host[k].nbytes) == 0

        def call(with_g):
            rc = L.ndsm_hip_vecpot_trace_device(V.h, dev["B"], dev["B"] if with_g else None, ns, dev["seeds"], 0.5,
                                                max_steps, 0, dev["ends"], dev["length"], dev["integral"],
                                                dev["status"], dev["nsteps"])
            assert rc == 0, _lib.last_error(L)

        def timed(with_g, count):
            assert L.ndsm_hip_timer_start() == 0
            for _ in range(count):
                call(with_g)
            ms = ctypes.c_double(0)
            assert L.ndsm_hip_timer_stop(ctypes.byref(ms)) == 0
            return ms.value * 1e-3 / count

        row = {"n": n, "seeds": ns, "lines": nl, "max_steps": max_steps, "field_MB": round(b.nbytes / 1e6, 1)}
        for with_g in (False, True):
            call(with_g)                                      # warm-up
            first = timed(with_g, 1)
            count = max(1, int(np.ceil(WINDOW_S / first)))
            ts = sorted(timed(with_g, count) for _ in range(repeats))
            for k in ("status", "nsteps"):
                assert L.ndsm_hip_memcpy_d2h(host[k].ctypes.data, dev[k], host[k].nbytes) == 0
            steps = int(host["nsteps"].astype(np.int64).sum())
            exits = int((host["status"] <= 6).sum())
            stages = 4 * steps + 3 * exits
            med = float(np.median(ts))
            tag = "G" if with_g else "noG"
            row.update({tag + "_ms": round(med * 1e3, 3), tag + "_min_ms": round(ts[0] * 1e3, 3),
                        tag + "_max_ms": round(ts[-1] * 1e3, 3), tag + "_calls_per_window": count,
                        tag + "_lines_per_s": round(nl / med), tag + "_steps_per_s": round(steps / med),
                        tag + "_gathered_GB_per_s": round(stages * (48 if with_g else 24) * 8 / med / 1e9, 1)})
            row.update(steps=steps, steps_max=int(host["nsteps"].max()), steps_mean=round(steps / nl, 1),
                       unfinished=int((host["status"] == _lib.TRACE_UNFINISHED).sum()),
                       null=int((host["status"] == _lib.TRACE_NULL).sum()))
        for p in dev.values():
            L.ndsm_hip_device_free(p)
        if n <= flh_max:
            for name, fn in (("helicity_devore_s", lambda: V.helicity(b, gauge="devore")),
                             ("flh_devore_s", lambda: V.field_line_helicity(b, seeds, gauge="devore"))):
                ts = []
                for rep in range(4):
                    t = time.perf_counter()
                    fn()
                    if rep:
                        ts.append(time.perf_counter() - t)
                row[name] = round(float(np.median(ts)), 4)
            row["flh_over_helicity"] = round(row["flh_devore_s"] / row["helicity_devore_s"], 3)
        V.close()
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


if __name__ == "__main__":
    args = sys.argv[1:]
    opts = {"--flh-max": 256, "--repeats": 5}
    for o in list(opts):
        if o in args:
            i = args.index(o)
            opts[o] = int(args[i + 1])
            del args[i:i + 2]
    main([int(a) for a in args] or [128, 256, 512], flh_max=opts["--flh-max"], repeats=opts["--repeats"])
