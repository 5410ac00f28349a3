"""The magnetogram preprocessing timed per try, with device events in one run:
usage probe_preprocess.py [--repeats R] [nx,ny ...]   (default 1024,512 4096,2048, --repeats 5)

Per plane of nx x ny nodes, on one VecPot handle (four planes in z: the call looks at the lower face alone) and the
test magnetogram of tests/preprocess_model.py; B stays in device memory, obs = NULL, the default mu and dt0, tol = 0.  A
call of ndsm_hip_vecpot_preprocess_device runs K tries, K a multiple of 50 chosen after one warm-up call so that a
timed window - one call between two events on the library stream - is at least 0.2 s long; the field is reset (outside
the window) before every call, so every window does the same work.  tol = 0 ends a call at a check without progress
(with check = 1: at every rejected try); the window then goes on with a further call from the field and the step
reached, the observation now the original.  The window holds each call's own allocation, copy of the observation,
start evaluation and final copy as well: at K >= 50 they are a per cent or so of it.  The variants alternate window by
window, R windows each:
  c50     check = 50: one read-back per 50 tries
  c1      check = 1: a blocking read-back after every try - what the device-side decision saves
Reported per variant: median, min and max time per try, the share of 8 TB/s that the traffic the two passes must move
(168 B per node and try: 72 in and 24 out in the update pass, 48 in and 24 out in the sums pass) makes at the median,
and the accepted tries of the last window."""
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
from preprocess_model import MU, test_magnetogram  # noqa: E402

WINDOW_S = 0.2
PEAK = 8.0e12
BYTES_PER_NODE = 168
DT0 = 0.01


def main(planes, repeats=5):
    L = ndsm_amd.load_library()
    assert L.ndsm_hip_init(-1) == 0, _lib.last_error(L)
    mu = np.array(MU, dtype=np.float64)
    for nx, ny in planes:
        mesh = uniform_mesh([nx, ny, 4])
        b = np.ascontiguousarray(test_magnetogram(mesh))
        V = ndsm_amd.VecPot(*mesh)
        N = nx * ny
        dB, dO = ctypes.c_void_p(), ctypes.c_void_p()
        assert L.ndsm_hip_device_alloc(b.nbytes, ctypes.byref(dB)) == 0, _lib.last_error(L)
        assert L.ndsm_hip_device_alloc(b.nbytes, ctypes.byref(dO)) == 0, _lib.last_error(L)
        assert L.ndsm_hip_memcpy_h2d(dO, b.ctypes.data, b.nbytes) == 0
        info = np.zeros(3, dtype=np.intc)

        def call(check, tries):
            """one timed window of `tries` tries from the start field: seconds per try, the last history row"""
            assert L.ndsm_hip_memcpy_h2d(dB, b.ctypes.data, b.nbytes) == 0
            hist = np.zeros((tries // check + 2, 17))
            left, dt, accepted, first = tries, DT0, 0, True
            assert L.ndsm_hip_timer_start() == 0
            while left > 0:
                rc = L.ndsm_hip_vecpot_preprocess_device(V.h, dB, None if first else dO, mu.ctypes.data, left, check,
                                                         0.0, dt, 0.0, hist.ctypes.data, len(hist), info.ctypes.data)
                assert rc == 0 and info[1] > 0, (rc, info, _lib.last_error(L))
                left -= int(info[1])
                dt = float(hist[int(info[0]) - 1, 7])
                accepted += int(hist[int(info[0]) - 1, 8])
                first = False
            ms = ctypes.c_double(0)
            assert L.ndsm_hip_timer_stop(ctypes.byref(ms)) == 0
            row = hist[int(info[0]) - 1].copy()
            row[8] = accepted
            return ms.value * 1e-3 / tries, row

        variants = {"c50": 50, "c1": 1}
        t, _ = call(50, 50)                                            # warm-up, and the size of a window
        tries = 50 * max(1, int(np.ceil(WINDOW_S / t / 50.0)))
        for c in variants.values():
            call(c, 50)
        ts = {k: [] for k in variants}
        last = {}
        for _ in range(repeats):
            for k, c in variants.items():
                t, last[k] = call(c, tries)
                ts[k].append(t)
        row = {"nx": nx, "ny": ny, "nodes": N, "tries_per_window": tries, "arrays_MB": round(15 * 8 * N / 1e6, 1),
               "bytes_per_try_MB": round(BYTES_PER_NODE * N / 1e6, 1)}
        for k, t in ts.items():
            t.sort()
            med = float(np.median(t))
            row.update({k + "_us": round(med * 1e6, 2), k + "_min_us": round(t[0] * 1e6, 2),
                        k + "_max_us": round(t[-1] * 1e6, 2),
                        k + "_share_of_peak": round(BYTES_PER_NODE * N / med / PEAK, 4),
                        k + "_accepted": int(last[k][8]), k + "_L": float(last[k][1])})
        row["c1_over_c50"] = round(row["c1_us"] / row["c50_us"], 4)
        L.ndsm_hip_device_free(dB)
        L.ndsm_hip_device_free(dO)
        V.close()
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    args = sys.argv[1:]
    repeats = 5
    if "--repeats" in args:
        i = args.index("--repeats")
        repeats = int(args[i + 1])
        del args[i:i + 2]
    main([tuple(int(v) for v in a.split(",")) for a in args] or [(1024, 512), (4096, 2048)], repeats=repeats)
