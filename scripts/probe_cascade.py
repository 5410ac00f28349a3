"""The coarse-to-fine cascade of the optimization method, timed with device events in one run:
usage probe_cascade.py [--repeats R] [--resample N] [--cascade N]   (default --repeats 5 --resample 256 --cascade 129)

1. A level change next to a try.  N^3 <-> (N/2)^3 nodes, three components, arrays resident in device memory.  A timed
   window - between two events on the library stream - holds K calls of one kind, K chosen after one warm-up call so
   that a window is at least 0.1 s long; the kinds alternate window by window, R windows each:
     down   ndsm_hip_resample_device, mode 1 (hat average), N^3 -> (N/2)^3
     up     ndsm_hip_resample_device, mode 0 (linear),      (N/2)^3 -> N^3
     try    ndsm_hip_vecpot_optimize_device, start 1, no weight, check 50: 50 tries per call from the same field
   Reported: median, min and max per call (per try for `try`), and the share of 8 TB/s of the bytes a level change must
   move (24 B per node of both arrays).
2. What the cascade reaches.  N^3 -> ((N + 1) / 2)^3 -> ... three levels on [0, 2]^3 with the field of
   tests/test_cascade_model.py (the ABC field plus bump(mesh, 1) (1, 0.7, -0.5)), start 1, no weight, check 50, tol 0:
   the cascade with 100 tries on the finest level and at most 400 on the others, then the single-level call with as
   many tries as fit into the cascade's time (from the median time of a try measured before).  After one warm-up of
   each, R windows of each, alternating.  Reported: median time and final L of both, and the tries per level."""
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
from optimize_model import abc_field, bump, perturbed_abc  # noqa: E402

WINDOW_S = 0.1
PEAK = 8.0e12


def stats(ts, scale=1e6):
    ts = sorted(ts)
    return {"median": round(float(np.median(ts)) * scale, 2), "min": round(ts[0] * scale, 2), "max": round(ts[-1] * scale, 2)}


def timed(L, fn):
    assert L.ndsm_hip_timer_start() == 0
    out = fn()
    ms = ctypes.c_double(0)
    assert L.ndsm_hip_timer_stop(ctypes.byref(ms)) == 0
    return ms.value * 1e-3, out


def dev(L, a):
    p = ctypes.c_void_p()
    assert L.ndsm_hip_device_alloc(a.nbytes, ctypes.byref(p)) == 0, _lib.last_error(L)
    assert L.ndsm_hip_memcpy_h2d(p, a.ctypes.data, a.nbytes) == 0
    return p


def level_change(L, n, repeats):
    q = np.linspace(0.0, 1.0, n)
    mesh = [q, q, q]
    b = np.ascontiguousarray(perturbed_abc(mesh)[1])
    m = n // 2
    fine3, coarse3 = np.array([n] * 3, dtype=np.intc), np.array([m] * 3, dtype=np.intc)
    dF, dC = dev(L, b), dev(L, np.zeros(3 * m ** 3))
    dT = dev(L, b)
    V = ndsm_amd.VecPot(*mesh)
    ioptc, ropt = V._options(10000, 1024, 1e-13, 1e-10, 5, False, False, False)
    hist, info = np.zeros((3, 6)), np.zeros(3, dtype=np.intc)
    dt0 = 0.1 * (q[1] - q[0]) ** 2
    ip = _lib._ip

    def down():
        assert L.ndsm_hip_resample_device(fine3.ctypes.data_as(ip), coarse3.ctypes.data_as(ip), 3, 1, dF, dC) == 0

    def up():
        assert L.ndsm_hip_resample_device(coarse3.ctypes.data_as(ip), fine3.ctypes.data_as(ip), 3, 0, dC, dT) == 0

    def tries():
        rc = L.ndsm_hip_vecpot_optimize_device(V.h, ioptc.ctypes.data_as(ip), _lib._d(ropt), dT, None, 1, 50, 50, 0.0,
                                               dt0, 0.0, hist.ctypes.data, 3, info.ctypes.data)
        assert rc == 0 and info[1] == 50, (rc, info)

    def reset():
        assert L.ndsm_hip_memcpy_h2d(dT, b.ctypes.data, b.nbytes) == 0
    kinds = {"down": (down, 1), "up": (up, 1), "try": (tries, 50)}
    count = {}
    for k, (fn, per) in kinds.items():
        fn()                                                            # warm-up
        reset()
        t, _ = timed(L, fn)
        count[k] = max(1, int(np.ceil(WINDOW_S / t)))
    ts = {k: [] for k in kinds}
    for _ in range(repeats):
        for k, (fn, per) in kinds.items():
            reset()
            t, _ = timed(L, lambda: [fn() for _ in range(count[k])])
            ts[k].append(t / (count[k] * per))
    row = {"what": "level change", "n": n, "coarse": m, "calls_per_window": count}
    for k in kinds:
        row[k + "_us"] = stats(ts[k])
    moved = 24 * (n ** 3 + m ** 3)
    for k in ("down", "up"):
        row[k + "_share_of_peak"] = round(moved / (row[k + "_us"]["median"] * 1e-6) / PEAK, 4)
        row[k + "_over_try"] = round(row[k + "_us"]["median"] / row["try_us"]["median"], 3)
    for p in (dF, dC, dT):
        L.ndsm_hip_device_free(p)
    V.close()
    print(json.dumps(row), flush=True)
    return row


def reach(L, n, repeats):
    q = np.linspace(0.0, 2.0, n)
    mesh = [q, q, q]
    exact = abc_field(mesh)
    b = exact.copy()
    g = bump(mesh, 1)
    for c, a in enumerate((1.0, 0.7, -0.5)):
        b[c] += a * g
    shapes = ndsm_amd.cascade_shapes((n, n, n), 3)
    Vs = [ndsm_amd.VecPot(*[np.linspace(0.0, 2.0, m) for m in s[::-1]]) for s in shapes]
    nit = [100, 400, 400]

    def cascade():
        return Vs[0].optimize_cascade(Vs[1:], b, start="given", niter_max=nit, check=50, tol=0.0, device=True)

    def single(tries):
        return Vs[0].optimize(b, start="given", niter_max=tries, check=50, tol=0.0, device=True)
    # (device=True stages B through the library's helpers outside the entry; the windows below hold that copy for both)
    cascade()
    single(50)
    t50 = float(np.median([timed(L, lambda: single(50))[0] for _ in range(3)]))
    t100 = float(np.median([timed(L, lambda: single(100))[0] for _ in range(3)]))
    per_try = (t100 - t50) / 50.0
    tc0 = float(np.median([timed(L, cascade)[0] for _ in range(3)]))
    tries = max(50, int(round((tc0 - (t50 - 50 * per_try)) / per_try / 50.0)) * 50)
    tc, tsg, outc, outs = [], [], None, None
    for _ in range(repeats):
        t, outc = timed(L, cascade)
        tc.append(t)
        t, outs = timed(L, lambda: single(tries))
        tsg.append(t)
    row = {"what": "reach", "shapes": shapes, "cascade_ms": stats(tc, 1e3), "single_ms": stats(tsg, 1e3),
           "single_tries": tries, "us_per_fine_try": round(per_try * 1e6, 2),
           "cascade_tries": [i[1] for i in outc[3]], "cascade_stop": [i[2] for i in outc[3]],
           "cascade_L": float(outc[2][0][-1, 1]), "single_L": float(outs[2][-1, 1]), "start_L": float(outs[2][0, 1]),
           "cascade_max_error": float(np.abs(outc[1] - exact).max()), "single_max_error": float(np.abs(outs[1] - exact).max()),
           "single_L_after_100": float(single(100)[2][-1, 1])}
    for V in Vs:
        V.close()
    print(json.dumps(row), flush=True)
    return row


def main(argv):
    opts = {"--repeats": 5, "--resample": 256, "--cascade": 129}
    for k in list(opts):
        if k in argv:
            opts[k] = int(argv[argv.index(k) + 1])
    L = ndsm_amd.load_library()
    assert L.ndsm_hip_init(-1) == 0, _lib.last_error(L)
    if opts["--resample"] > 0:
        level_change(L, opts["--resample"], opts["--repeats"])
    if opts["--cascade"] > 0:
        reach(L, opts["--cascade"], opts["--repeats"])


if __name__ == "__main__":
    main(sys.argv[1:])
