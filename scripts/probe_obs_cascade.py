"""The level data of the cascade of the measurement fit, timed with device events in one run:
usage probe_obs_cascade.py [--repeats R] [--plane N] [--levels N]   (default --repeats 5 --plane 1024 --levels 256)

The protocol is probe_cascade.py's: arrays resident in device memory; a timed window - between two events on the
library stream - holds K calls of one kind, K chosen after one warm-up call so that a window is at least 0.1 s long; the
kinds alternate window by window, R windows each; reported are median, min and max per call.  Nothing is asserted on
time.

1. The weighted restriction of a plane pair.  (N, N, 1) -> (N/2, N/2, 1), three components:
     weighted   ndsm_hip_resample_weighted_device: the observation and its confidence in, both out
     average    ndsm_hip_resample_device, mode 1, on the observation alone (what the level data were without wm)
   and the share of 8 TB/s of the bytes each must move (8 B per node and component of every array it reads or writes).
2. The whole level-data phase next to a try.  N^3 -> (N/2)^3:
     fields     G_l (mode 1, three components) and w_l (mode 0, one component): the level data of optimize_cascade
     planes     (Bobs_l, wm_l): the weighted restriction (N, N, 1) -> (N/2, N/2, 1), three components - what the
                measurement fit adds
     try        ndsm_hip_vecpot_optimize_obs_device, start 1, free 1, nu 0.01, with w and wm, check 50: 50 tries per
                call from the same field, reported per try
   The expectation is that the planes do not show next to the fields."""
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
from optimize_model import perturbed_abc  # noqa: E402

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


def windows(L, kinds, repeats, reset=lambda: None):
    """{kind: seconds per unit, one entry per window} and the calls per window; kinds: {name: (call, units per call)}"""
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
    return ts, count


def plane_pair(L, n, repeats):
    rng = np.random.default_rng(1)
    m = n // 2
    obs, conf = rng.uniform(-1.0, 1.0, 3 * n * n), 1.0 - rng.uniform(0.0, 1.0, 3 * n * n)
    fine3, coarse3 = np.array([n, n, 1], dtype=np.intc), np.array([m, m, 1], dtype=np.intc)
    dO, dW = dev(L, obs), dev(L, conf)
    dD, dWD = dev(L, np.zeros(3 * m * m)), dev(L, np.zeros(3 * m * m))
    ip = _lib._ip

    def weighted():
        assert L.ndsm_hip_resample_weighted_device(fine3.ctypes.data_as(ip), coarse3.ctypes.data_as(ip), 3, dO, dW, dD, dWD) == 0

    def average():
        assert L.ndsm_hip_resample_device(fine3.ctypes.data_as(ip), coarse3.ctypes.data_as(ip), 3, 1, dO, dD) == 0
    ts, count = windows(L, {"weighted": (weighted, 1), "average": (average, 1)}, repeats)
    row = {"what": "plane pair", "n": n, "coarse": m, "calls_per_window": count}
    moved = {"weighted": 2 * 24 * (n * n + m * m), "average": 24 * (n * n + m * m)}
    for k in ts:
        row[k + "_us"] = stats(ts[k])
        row[k + "_share_of_peak"] = round(moved[k] / (row[k + "_us"]["median"] * 1e-6) / PEAK, 4)
    for p in (dO, dW, dD, dWD):
        L.ndsm_hip_device_free(p)
    print(json.dumps(row), flush=True)
    return row


def level_data(L, n, repeats):
    q = np.linspace(0.0, 1.0, n)
    mesh = [q, q, q]
    b = np.ascontiguousarray(perturbed_abc(mesh)[1])
    rng = np.random.default_rng(2)
    m = n // 2
    w = np.ascontiguousarray(ndsm_amd.boundary_weight((n, n, n), 8))
    obs = np.ascontiguousarray(b[:, 0]) + 0.05 * rng.standard_normal((3, n, n))
    conf = np.ascontiguousarray(ndsm_amd.measurement_weight(obs, floor=0.05))
    fine3, coarse3 = np.array([n] * 3, dtype=np.intc), np.array([m] * 3, dtype=np.intc)
    fine2, coarse2 = np.array([n, n, 1], dtype=np.intc), np.array([m, m, 1], dtype=np.intc)
    dB, dW, dO, dC = dev(L, b), dev(L, w), dev(L, obs), dev(L, conf)
    dG, dWl = dev(L, np.zeros(3 * m ** 3)), dev(L, np.zeros(m ** 3))
    dOl, dCl = dev(L, np.zeros(3 * m * m)), dev(L, np.zeros(3 * m * m))
    dT = dev(L, b)
    V = ndsm_amd.VecPot(*mesh)
    ioptc, ropt = V._options(10000, 1024, 1e-13, 1e-10, 5, False, False, False)
    hist, info = np.zeros((3, 7)), np.zeros(3, dtype=np.intc)
    dt0 = 0.1 * (q[1] - q[0]) ** 2
    ip = _lib._ip

    def fields():
        assert L.ndsm_hip_resample_device(fine3.ctypes.data_as(ip), coarse3.ctypes.data_as(ip), 3, 1, dB, dG) == 0
        assert L.ndsm_hip_resample_device(fine3.ctypes.data_as(ip), coarse3.ctypes.data_as(ip), 1, 0, dW, dWl) == 0

    def planes():
        assert L.ndsm_hip_resample_weighted_device(fine2.ctypes.data_as(ip), coarse2.ctypes.data_as(ip), 3, dO, dC, dOl, dCl) == 0

    def tries():
        rc = L.ndsm_hip_vecpot_optimize_obs_device(V.h, ioptc.ctypes.data_as(ip), _lib._d(ropt), dT, dW, dO, dC, 0.01, 1, 1, 50,
                                                   50, 0.0, dt0, 0.0, hist.ctypes.data, 3, info.ctypes.data)
        assert rc == 0 and info[1] == 50, (rc, info)

    def reset():
        assert L.ndsm_hip_memcpy_h2d(dT, b.ctypes.data, b.nbytes) == 0
    ts, count = windows(L, {"fields": (fields, 1), "planes": (planes, 1), "try": (tries, 50)}, repeats, reset)
    row = {"what": "level data", "n": n, "coarse": m, "calls_per_window": count}
    for k in ts:
        row[k + "_us"] = stats(ts[k])
    row["planes_over_fields"] = round(row["planes_us"]["median"] / row["fields_us"]["median"], 4)
    row["level_data_over_try"] = round((row["planes_us"]["median"] + row["fields_us"]["median"]) / row["try_us"]["median"], 3)
    for p in (dB, dW, dO, dC, dG, dWl, dOl, dCl, dT):
        L.ndsm_hip_device_free(p)
    V.close()
    print(json.dumps(row), flush=True)
    return row


def main(argv):
    opts = {"--repeats": 5, "--plane": 1024, "--levels": 256}
    for k in list(opts):
        if k in argv:
            opts[k] = int(argv[argv.index(k) + 1])
    L = ndsm_amd.load_library()
    assert L.ndsm_hip_init(-1) == 0, _lib.last_error(L)
    if opts["--plane"] > 0:
        plane_pair(L, opts["--plane"], opts["--repeats"])
    if opts["--levels"] > 0:
        level_data(L, opts["--levels"], opts["--repeats"])


if __name__ == "__main__":
    main(sys.argv[1:])
