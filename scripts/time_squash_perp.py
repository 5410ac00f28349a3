"""The perpendicular-squashing-factor entry against the squash entry, timed with device events in one run: usage
time_squash_perp.py [--repeats R] [n ...]   (default 128 256, --repeats 5)

The protocol of time_squash.py: per size n^3, on one VecPot handle and the ABC field (tests/test_gpu_field.py), one
seed per node of the bottom face (n^2 seeds), step 0.5, the default max_steps; B, G, the seeds and the outputs stay
in device memory.  Each variant is warmed up once and then timed R times between two events on the library stream;
the calls are repeated inside one timed window until it is at least 0.2 s long.  Variants: ndsm_hip_vecpot_squash_device
and ndsm_hip_vecpot_squash_perp_device, each without G and with G (another array of the same size, integrand 1: the
values do not matter to the cost), measured alternately so that a drift of the clocks meets both.  The two entries
run the same RK4 loop and differ in the epilogue of each lane only, so the expectation to confirm or refute is a ratio
of 1 to within the run-to-run spread.  Reported per variant: median, min and max time of one call; per G: the ratio of
the medians, and whether the two ranges overlap.  q and the line outputs of the two entries are compared bit for bit
on the way."""
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
        ns, nl = len(seeds), 2 * len(seeds)
        max_steps = V.default_max_steps(0.5)
        host = {"B": b, "G": b[::-1].copy(), "seeds": seeds, "q": np.zeros(ns), "qperp": np.zeros(ns),
                "ends": np.zeros((nl, 3)), "length": np.zeros(nl), "integral": np.zeros(nl),
                "status": np.zeros(nl, dtype=np.int32), "nsteps": np.zeros(nl, dtype=np.int32)}
        dev = {}
        for k, a in host.items():
            dev[k] = ctypes.c_void_p()
            assert L.ndsm_hip_device_alloc(a.nbytes, ctypes.byref(dev[k])) == 0, _lib.last_error(L)
        for k in ("B", "G", "seeds"):
            assert L.ndsm_hip_memcpy_h2d(dev[k], host[k].ctypes.data, host[k].nbytes) == 0
        outs = [dev[k] for k in ("ends", "length", "integral", "status", "nsteps")]
        names = ("q", "ends", "length", "integral", "status", "nsteps")

        def squash(with_g):
            rc = L.ndsm_hip_vecpot_squash_device(V.h, dev["B"], dev["G"] if with_g else None, 1 if with_g else 0, ns,
                                                 dev["seeds"], 0.5, max_steps, dev["q"], *outs)
            assert rc == 0, _lib.last_error(L)

        def perp(with_g):
            rc = L.ndsm_hip_vecpot_squash_perp_device(V.h, dev["B"], dev["G"] if with_g else None, 1 if with_g else 0,
                                                      ns, dev["seeds"], 0.5, max_steps, dev["q"], dev["qperp"], *outs)
            assert rc == 0, _lib.last_error(L)

        def fetch(keys):
            out = {}
            for k in keys:
                assert L.ndsm_hip_memcpy_d2h(host[k].ctypes.data, dev[k], host[k].nbytes) == 0
                out[k] = host[k].copy()
            return out

        def timed(fn, with_g, count):
            assert L.ndsm_hip_timer_start() == 0
            for _ in range(count):
                fn(with_g)
            ms = ctypes.c_double(0)
            assert L.ndsm_hip_timer_stop(ctypes.byref(ms)) == 0
            return ms.value * 1e-3 / count

        row = {"n": n, "seeds": ns, "max_steps": max_steps, "field_MB": round(b.nbytes / 1e6, 1)}
        for with_g in (False, True):
            g = "_G" if with_g else "_noG"
            squash(with_g)                                    # warm-up, and the bits to compare
            ref = fetch(names)
            perp(with_g)
            got = fetch(names + ("qperp",))
            row["same_bits" + g] = all(np.array_equal(ref[k], got[k], equal_nan=True) for k in names)
            row["qperp_finite" + g] = int(np.isfinite(got["qperp"]).sum())
            row["steps_max" + g] = int(got["nsteps"].max())
            count = max(1, int(np.ceil(WINDOW_S / timed(squash, with_g, 1))))
            ts = {"squash": [], "perp": []}
            for _ in range(repeats):                          # alternately
                ts["squash"].append(timed(squash, with_g, count))
                ts["perp"].append(timed(perp, with_g, count))
            for name, t in ts.items():
                t.sort()
                row.update({name + g + "_ms": round(float(np.median(t)) * 1e3, 3),
                            name + g + "_min_ms": round(t[0] * 1e3, 3),
                            name + g + "_max_ms": round(t[-1] * 1e3, 3)})
            row["calls_per_window" + g] = count
            row["perp_over_squash" + g] = round(row["perp" + g + "_ms"] / row["squash" + g + "_ms"], 4)
            row["ranges_overlap" + g] = bool(ts["perp"][0] <= ts["squash"][-1] and ts["squash"][0] <= ts["perp"][-1])
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
