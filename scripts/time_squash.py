"""Squashing-factor maps on device-resident arrays, timed with device events, against the way to the same map
through the trace entry: usage time_squash.py [--repeats R] [n ...]   (default 128 256, --repeats 5)

Per size n^3, on one VecPot handle and the ABC field (tests/test_gpu_field.py), the protocol of time_trace.py: one
seed per node of the bottom face (n^2 seeds), step 0.5, the default max_steps; B, G, the seeds and the outputs stay
in device memory.  Each variant is warmed up once and then timed R times between two events on the library stream;
the calls are repeated inside one timed window until it is at least 0.2 s long.  Variants: squash without G and with
G (G = another array of the same size, integrand 1: the values do not matter to the cost), and the yardstick: ONE
ndsm_hip_vecpot_trace_device call, both directions, over five lines per seed - the seed and four neighbours at
+-delta in x and y, what finite differences of the foot points need - without and with G.  Reported per variant:
median, min and max time of one call; for squash also the steps of the longest line and the time per step of it
(the kernel ends with its longest line), and the ratio to the five-line trace."""
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


def main(sizes, repeats=5):
    L = ndsm_amd.load_library()
    assert L.ndsm_hip_init(-1) == 0, _lib.last_error(L)
    rows = []
    for n in sizes:
        mesh, b = abc_field([n, n, n])
        b = np.ascontiguousarray(b)
        V = ndsm_amd.VecPot(*mesh)
        X, Y = np.meshgrid(mesh[0], mesh[1], indexing="xy")
        seeds = np.ascontiguousarray(np.stack([X.ravel(), Y.ravel(), np.full(X.size, mesh[2][0])], axis=1))
        ns = len(seeds)
        delta = 1e-4 * (mesh[0][-1] - mesh[0][0])
        off = np.array([[0, 0, 0], [delta, 0, 0], [-delta, 0, 0], [0, delta, 0], [0, -delta, 0]])
        lo = np.array([q[0] for q in mesh])
        hi = np.array([q[0] + (len(q) - 1.0) * (q[1] - q[0]) for q in mesh])
        seeds5 = np.ascontiguousarray(np.minimum(np.maximum((seeds[None] + off[:, None]).reshape(-1, 3), lo), hi))
        n5, nl5 = len(seeds5), 2 * len(seeds5)
        max_steps = V.default_max_steps(0.5)
        host = {"B": b, "G": b[::-1].copy(), "seeds": seeds, "seeds5": seeds5, "q": np.zeros(ns),
                "ends": np.zeros((nl5, 3)), "length": np.zeros(nl5), "integral": np.zeros(nl5),
                "status": np.zeros(nl5, dtype=np.int32), "nsteps": np.zeros(nl5, dtype=np.int32)}
        dev = {}
        for k, a in host.items():
            dev[k] = ctypes.c_void_p()
            assert L.ndsm_hip_device_alloc(a.nbytes, ctypes.byref(dev[k])) == 0, _lib.last_error(L)
        for k in ("B", "G", "seeds", "seeds5"):
            assert L.ndsm_hip_memcpy_h2d(dev[k], host[k].ctypes.data, host[k].nbytes) == 0
        outs = [dev[k] for k in ("ends", "length", "integral", "status", "nsteps")]

        def squash(with_g):
            rc = L.ndsm_hip_vecpot_squash_device(V.h, dev["B"], dev["G"] if with_g else None, 1 if with_g else 0, ns,
                                                 dev["seeds"], 0.5, max_steps, dev["q"], *outs)
            assert rc == 0, _lib.last_error(L)

        def trace5(with_g):
            rc = L.ndsm_hip_vecpot_trace_device(V.h, dev["B"], dev["G"] if with_g else None, n5, dev["seeds5"], 0.5,
                                                max_steps, 0, *outs)
            assert rc == 0, _lib.last_error(L)

        def timed(fn, with_g, count):
            assert L.ndsm_hip_timer_start() == 0
            for _ in range(count):
                fn(with_g)
            ms = ctypes.c_double(0)
            assert L.ndsm_hip_timer_stop(ctypes.byref(ms)) == 0
            return ms.value * 1e-3 / count

        row = {"n": n, "seeds": ns, "max_steps": max_steps, "field_MB": round(b.nbytes / 1e6, 1)}
        for name, fn, nl in (("squash", squash, 2 * ns), ("trace5", trace5, nl5)):
            for with_g in (False, True):
                fn(with_g)                                    # warm-up
                first = timed(fn, with_g, 1)
                count = max(1, int(np.ceil(WINDOW_S / first)))
                ts = sorted(timed(fn, with_g, count) for _ in range(repeats))
                assert L.ndsm_hip_memcpy_d2h(host["nsteps"].ctypes.data, dev["nsteps"], host["nsteps"].nbytes) == 0
                st = host["nsteps"][:nl].astype(np.int64)
                med = float(np.median(ts))
                tag = name + ("_G" if with_g else "_noG")
                row.update({tag + "_ms": round(med * 1e3, 3), tag + "_min_ms": round(ts[0] * 1e3, 3),
                            tag + "_max_ms": round(ts[-1] * 1e3, 3), tag + "_calls_per_window": count,
                            tag + "_steps": int(st.sum()), tag + "_steps_max": int(st.max()),
                            tag + "_us_per_step_of_longest": round(med * 1e6 / max(int(st.max()), 1), 3)})
            if name == "squash":
                assert L.ndsm_hip_memcpy_d2h(host["q"].ctypes.data, dev["q"], host["q"].nbytes) == 0
                row["q_finite"] = int(np.isfinite(host["q"]).sum())
        for g in ("_noG", "_G"):
            row["squash_over_trace5" + g] = round(row["squash" + g + "_ms"] / row["trace5" + g + "_ms"], 3)
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
    main([int(a) for a in args] or [128, 256], repeats=repeats)
