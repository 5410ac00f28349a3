"""The optimization method with a measurement term and a freed lower face timed per try against the plain one, with
device events in one run:
usage probe_optimize_obs.py [--repeats R] [n ...]   (default 128 256, --repeats 5)

probe_optimize.py's protocol.  Per size n^3, on one VecPot handle and the perturbed ABC field of
tests/optimize_model.py; B, w, Bobs and wm stay in device memory, start = 1 (no solve), tol = 0, check = 50, the
default dt0, w = boundary_weight(nd = max(2, n / 16)).  A call runs K tries, K a multiple of 50 chosen after one
warm-up call so that a timed window - the calls between two events on the library stream - is at least 0.2 s long; the
field is reset (outside the window) before every window, so every window does the same work.  tol = 0 ends a call at a
check without progress; the window then goes on with a further call from the field and the step reached.  The variants
alternate window by window, R windows each:
  plain   ndsm_hip_vecpot_optimize_device
  obs     ndsm_hip_vecpot_optimize_obs_device with free = 1, nu = 0.01, Bobs = the lower face plus a smooth pattern of
          height 0.1, wm = measurement_weight(Bobs, 0.05)
  held    the same with free = 0: the third sum alone
Reported per variant: median, min and max time per try and the accepted tries of the last window; obs and held over
plain at the medians."""
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
NU = 0.01


def main(sizes, repeats=5):
    L = ndsm_amd.load_library()
    assert L.ndsm_hip_init(-1) == 0, _lib.last_error(L)
    for n in sizes:
        mesh = uniform_mesh([n, n, n])
        b = np.ascontiguousarray(perturbed_abc(mesh)[1])
        w = np.ascontiguousarray(ndsm_amd.boundary_weight(b.shape[1:], max(2, n // 16)))
        u = np.linspace(0.0, 1.0, n)
        Y, X = np.meshgrid(u, u, indexing="ij")
        bobs = np.ascontiguousarray(b[:, 0] + 0.1 * np.array([np.cos(3.0 * X + Y), np.sin(2.0 * Y - X), 0.5 - X * Y]))
        wm = np.ascontiguousarray(ndsm_amd.measurement_weight(bobs, 0.05))
        V = ndsm_amd.VecPot(*mesh)
        dt0 = 0.1 * min(spacing(mesh)) ** 2
        ioptc, ropt = V._options(10000, 1024, 1e-13, 1e-10, 5, False, False, False)
        dev = []
        for a in (b, w, bobs, wm):
            p = ctypes.c_void_p()
            assert L.ndsm_hip_device_alloc(a.nbytes, ctypes.byref(p)) == 0, _lib.last_error(L)
            assert L.ndsm_hip_memcpy_h2d(p, a.ctypes.data, a.nbytes) == 0
            dev.append(p)
        dB, dw, dbobs, dwm = dev
        info = np.zeros(3, dtype=np.intc)

        def call(variant, tries):
            """one timed window of `tries` tries from the start field: seconds per try, accepted tries, L"""
            assert L.ndsm_hip_memcpy_h2d(dB, b.ctypes.data, b.nbytes) == 0
            cols = 6 if variant == "plain" else 7
            hist = np.zeros((tries // 50 + 2, cols))
            left, dt, accepted = tries, dt0, 0
            assert L.ndsm_hip_timer_start() == 0
            while left > 0:
                tail = (1, left, 50, 0.0, dt, 0.0, hist.ctypes.data, len(hist), info.ctypes.data)
                if variant == "plain":
                    rc = L.ndsm_hip_vecpot_optimize_device(V.h, ioptc.ctypes.data_as(_lib._ip), _lib._d(ropt), dB, dw,
                                                           *tail)
                else:
                    rc = L.ndsm_hip_vecpot_optimize_obs_device(V.h, ioptc.ctypes.data_as(_lib._ip), _lib._d(ropt), dB,
                                                               dw, dbobs, dwm, NU, 1 if variant == "obs" else 0, *tail)
                assert rc == 0 and info[1] > 0, (rc, info, _lib.last_error(L))
                left -= int(info[1])
                dt = float(hist[int(info[0]) - 1, cols - 2])
                accepted += int(hist[int(info[0]) - 1, cols - 1])
            ms = ctypes.c_double(0)
            assert L.ndsm_hip_timer_stop(ctypes.byref(ms)) == 0
            return ms.value * 1e-3 / tries, accepted, float(hist[int(info[0]) - 1, 1])

        variants = ("plain", "obs", "held")
        t = call("plain", 50)[0]                                       # warm-up, and the size of a window
        tries = 50 * max(1, int(np.ceil(WINDOW_S / t / 50.0)))
        for v in variants:
            call(v, 50)
        ts = {k: [] for k in variants}
        last = {}
        for _ in range(repeats):
            for k in variants:
                t, acc, lval = call(k, tries)
                ts[k].append(t)
                last[k] = (acc, lval)
        row = {"n": n, "nodes": n ** 3, "tries_per_window": tries}
        for k, t in ts.items():
            t.sort()
            row.update({k + "_us": round(float(np.median(t)) * 1e6, 2), k + "_min_us": round(t[0] * 1e6, 2),
                        k + "_max_us": round(t[-1] * 1e6, 2), k + "_accepted": last[k][0], k + "_L": last[k][1]})
        row["obs_over_plain"] = round(row["obs_us"] / row["plain_us"], 4)
        row["held_over_plain"] = round(row["held_us"] / row["plain_us"], 4)
        for p in dev:
            L.ndsm_hip_device_free(p)
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
