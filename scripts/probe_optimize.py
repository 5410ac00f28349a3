"""The optimization-method solver timed per try, with device events in one run:
usage probe_optimize.py [--repeats R] [n ...]   (default 128 256, --repeats 5)

Per size n^3, on one VecPot handle and the perturbed ABC field of tests/optimize_model.py; B and w stay in device
memory, start = 1 (no solve), tol = 0, the default dt0.  A call of ndsm_hip_vecpot_optimize_device runs K tries, K a
multiple of 50 chosen after one warm-up call so that a timed window - one call between two events on the library
stream - is at least 0.2 s long; the field is reset (outside the window) before every call, so every window does the
same work.  tol = 0 ends a call at a check without progress (with check = 1: at every rejected try); the window then
goes on with a further call from the field and the step reached.  The window holds each call's own allocation, start
evaluation and final copy as well: at K >= 50 they are a per cent or so of it.  The variants alternate window by
window, R windows each:
  w50     with a weight array, check = 50: one read-back per 50 tries
  w1      the same with check = 1: a blocking read-back after every try - what the device-side decision saves
  now50   without a weight array (w = NULL), check = 50
Reported per variant: median, min and max time per try, the share of 8 TB/s that the traffic the two passes must move
(128 B per point and try with w, 120 without) makes at the median, and the accepted tries of the last call."""
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
from golden_inputs import uniform_mesh  # noqa: E402
from optimize_model import perturbed_abc, spacing  # noqa: E402

WINDOW_S = 0.2
PEAK = 8.0e12


def main(sizes, repeats=5):
    L = ndsm_amd.load_library()
    assert L.ndsm_hip_init(-1) == 0, _lib.last_error(L)
    for n in sizes:
        mesh = uniform_mesh([n, n, n])
        b = np.ascontiguousarray(perturbed_abc(mesh)[1])
        w = np.ascontiguousarray(ndsm_amd.boundary_weight(b.shape[1:], max(2, n // 16)))
        V = ndsm_amd.VecPot(*mesh)
        N = n ** 3
        dt0 = 0.1 * min(spacing(mesh)) ** 2
        ioptc, ropt = V._options(10000, 1024, 1e-13, 1e-10, 5, False, False, False)
        dB, dw = ctypes.c_void_p(), ctypes.c_void_p()
        assert L.ndsm_hip_device_alloc(b.nbytes, ctypes.byref(dB)) == 0, _lib.last_error(L)
        assert L.ndsm_hip_device_alloc(w.nbytes, ctypes.byref(dw)) == 0, _lib.last_error(L)
        assert L.ndsm_hip_memcpy_h2d(dw, w.ctypes.data, w.nbytes) == 0
        info = np.zeros(3, dtype=np.intc)

        def call(weight, check, tries):
            """one timed window of `tries` tries from the start field: seconds per try, the last history row"""
            assert L.ndsm_hip_memcpy_h2d(dB, b.ctypes.data, b.nbytes) == 0
            hist = np.zeros((tries // check + 2, 6))
            left, dt, accepted = tries, dt0, 0
            assert L.ndsm_hip_timer_start() == 0
            while left > 0:
                # (tol = 0 ends a call at a check without progress - with check = 1 at every rejected try: the next call
                # goes on from there with the step the last one reached)
                rc = L.ndsm_hip_vecpot_optimize_device(V.h, ioptc.ctypes.data_as(_lib._ip), _lib._d(ropt), dB,
                                                       dw if weight else None, 1, left, check, 0.0, dt, 0.0,
                                                       hist.ctypes.data, len(hist), info.ctypes.data)
                assert rc == 0 and info[1] > 0, (rc, info, _lib.last_error(L))
                left -= int(info[1])
                dt = float(hist[int(info[0]) - 1, 4])
                accepted += int(hist[int(info[0]) - 1, 5])
            ms = ctypes.c_double(0)
            assert L.ndsm_hip_timer_stop(ctypes.byref(ms)) == 0
            row = hist[int(info[0]) - 1].copy()
            row[5] = accepted
            return ms.value * 1e-3 / tries, row

        variants = {"w50": (True, 50), "w1": (True, 1), "now50": (False, 50)}
        t, _ = call(True, 50, 50)                                      # warm-up, and the size of a window
        tries = 50 * max(1, int(np.ceil(WINDOW_S / t / 50.0)))
        for v in variants.values():
            call(*v, 50)
        ts = {k: [] for k in variants}
        last = {}
        for _ in range(repeats):
            for k, v in variants.items():
                t, last[k] = call(*v, tries)
                ts[k].append(t)
        row = {"n": n, "nodes": N, "tries_per_window": tries, "arrays_MB": round(13 * 8 * N / 1e6, 1)}
        for k, t in ts.items():
            t.sort()
            med = float(np.median(t))
            bytes_per_try = (128 if variants[k][0] else 120) * N
            row.update({k + "_us": round(med * 1e6, 2), k + "_min_us": round(t[0] * 1e6, 2),
                        k + "_max_us": round(t[-1] * 1e6, 2), k + "_share_of_peak": round(bytes_per_try / med / PEAK, 4),
                        k + "_accepted": int(last[k][5]), k + "_L": float(last[k][1])})
        row["w1_over_w50"] = round(row["w1_us"] / row["w50_us"], 4)
        L.ndsm_hip_device_free(dB)
        L.ndsm_hip_device_free(dw)
        V.close()
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    args = sys.argv[1:]
    repeats = 5
    if "--repeats" in args:
        i = args.index("--repeats")
        repeats = int(args[i + 1])
        del args[i:i + 2]
    main([int(a) for a in args] or [128, 256], repeats=repeats)
